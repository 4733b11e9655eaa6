"""The tuple match term, as far as it can be checked without a GPU: the three C entries (``e2emv_gt_matches_tuple``,
``e2emv_match_loss_tuple``, ``e2emv_match_loss_tuple_backward``) are declared, bound, exported and refuse a NULL context; the Python front
makes fixed call sequences whose length does not depend on the tuple or batch size - recorded with a stand-in for the device context -;
every ``ValueError`` is raised before any call; and the premise of the exact targets test of tests/test_gpu_match_loss_tuple.py holds in
the oracle alone."""
import ctypes
import inspect
import os
import re

import pytest
import torch

from test_ba2view_backward import _stub_device

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"e2emv_gt_matches_tuple": 15, "e2emv_match_loss_tuple": 10, "e2emv_match_loss_tuple_backward": 9}


@pytest.mark.parametrize("name", list(NAMES))
def test_entry_is_declared_bound_exported_and_documented(lib_built, name):
    from e2e_multi_view_matching_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "e2emv.h")).read()
    assert name in set(re.findall(r"\b(e2emv_[a-z0-9_]+)\s*\(", hdr))
    decl = re.search(r"int %s\((.*?)\);" % name, hdr, re.S).group(1).split(",")
    sig = _lib.SIGNATURES[name]
    assert sig[0] is ctypes.c_int and len(sig[1]) == len(decl) == NAMES[name]
    assert hasattr(ctypes.CDLL(lib_built), name)
    assert open(os.path.join(ROOT, "INTEGRATION.md")).read().count("`%s`" % name) >= 1


def test_null_context_is_rejected(lib_built):
    from e2e_multi_view_matching_amd import _lib
    lib = _lib.load_library()
    assert lib.e2emv_gt_matches_tuple(None, 1, 2, 8, None, None, None, None, 4, 4, 5.0, 15.0, None, None, None) == _lib.EINVAL
    assert lib.e2emv_match_loss_tuple(None, 1, 1, 8, None, None, None, None, None, None) == _lib.EINVAL
    assert lib.e2emv_match_loss_tuple_backward(None, 1, 1, 8, None, None, None, None, None) == _lib.EINVAL


def test_the_functions_are_exported_from_the_package():
    import e2e_multi_view_matching_amd as E
    assert E.gt_matches_tuple is E.targets.gt_matches_tuple and "gt_matches_tuple" in E.__all__
    assert E.match_loss_tuple is E.targets.match_loss_tuple and "match_loss_tuple" in E.__all__
    assert "no autograd" not in E.targets.__doc__


def _stub(monkeypatch):
    from e2e_multi_view_matching_amd import targets
    rec = _stub_device(monkeypatch)
    monkeypatch.setattr(targets, "_dev_of", lambda *t: torch.device("cpu"))  # targets.py binds the name at import
    return rec


def _pairs(T):
    return [(i, j) for j in range(T) for i in range(j)]


def _data(T, B, N):
    data = {"ids": list(range(T))}
    for t in range(T):
        data["keypoints%d" % t] = torch.zeros(B, N, 2)
        data["intr%d" % t] = torch.eye(4)[None].repeat(B, 1, 1)
        data["pose%d" % t] = torch.eye(4)[None].repeat(B, 1, 1)
        data["depth%d" % t] = torch.ones(B, 6, 8)
    return data


def _scores(T, B, N, grad=True, skip_grad=()):
    result = {"scores_%d_%d" % p: torch.zeros(B, N + 1, N + 1, requires_grad=grad and p not in skip_grad) for p in _pairs(T)}
    P = len(result)
    return result, torch.zeros(P, B, 2, N + 1, dtype=torch.int64), torch.ones(P, B, 2, N + 1)


@pytest.mark.parametrize("T,B", [(3, 1), (3, 5), (5, 2)])
def test_call_sequences_do_not_depend_on_the_tuple_or_the_batch(monkeypatch, T, B):
    from e2e_multi_view_matching_amd import targets
    rec = _stub(monkeypatch)
    N, P = 9, T * (T - 1) // 2
    data = _data(T, B, N)
    keys = set(data)
    idx, w = targets.gt_matches_tuple(data, 5.0, 15.0)
    assert rec.calls == ["e2emv_gt_matches_tuple"] and set(data) == keys
    assert idx.shape == (P, B, 2, N + 1) and idx.dtype == torch.int64 and w.shape == idx.shape and w.dtype == torch.float32
    rec.calls.clear()
    targets.gt_matches_tuple({k: v for k, v in data.items() if k != "ids"}, 5.0, 15.0, n_images=T)
    assert rec.calls == ["e2emv_gt_matches_tuple"]
    rec.calls.clear()
    result, idx, w = _scores(T, B, N)
    loss = targets.match_loss_tuple(result, idx, w)
    assert rec.calls == ["e2emv_match_loss_tuple"]
    assert loss.dim() == 0 and loss.dtype == torch.float32 and loss.grad_fn is not None
    loss.backward()
    assert rec.calls == ["e2emv_match_loss_tuple", "e2emv_match_loss_tuple_backward"]
    for p in _pairs(T):
        g = result["scores_%d_%d" % p].grad
        assert g is not None and g.shape == (B, N + 1, N + 1) and g.dtype == torch.float32


def test_without_a_graph_only_the_forward_is_called(monkeypatch):
    from e2e_multi_view_matching_amd import targets
    rec = _stub(monkeypatch)
    result, idx, w = _scores(3, 2, 9, grad=False)
    loss = targets.match_loss_tuple(result, idx, w)
    assert rec.calls == ["e2emv_match_loss_tuple"] and loss.grad_fn is None and not loss.requires_grad and loss.dim() == 0
    rec.calls.clear()
    result, idx, w = _scores(3, 2, 9)
    with torch.no_grad():
        loss = targets.match_loss_tuple(result, idx, w)
    assert rec.calls == ["e2emv_match_loss_tuple"] and loss.grad_fn is None


def test_a_pair_that_needs_no_gradient_receives_none(monkeypatch):
    from e2e_multi_view_matching_amd import _lib, targets
    rec = _stub(monkeypatch)
    seen = []
    orig = _lib.ptr_array
    monkeypatch.setattr(_lib, "ptr_array", lambda tensors: (seen.append([t is None for t in tensors]), orig(tensors))[1])
    result, idx, w = _scores(3, 2, 9, skip_grad={(0, 2)})
    targets.match_loss_tuple(result, idx, w).backward()
    assert rec.calls == ["e2emv_match_loss_tuple", "e2emv_match_loss_tuple_backward"]
    assert result["scores_0_2"].grad is None and result["scores_0_1"].grad is not None and result["scores_1_2"].grad is not None
    assert seen[-1] == [False, True, False]  # the table of the backward call: a NULL entry for pair (0, 2)


def test_compute_match_loss_carries_the_graph_when_its_scores_do(monkeypatch):
    from e2e_multi_view_matching_amd import targets
    rec = _stub(monkeypatch)
    idx, w = torch.zeros(2, 2, 10, dtype=torch.int64), torch.ones(2, 2, 10)
    loss = targets.compute_match_loss(torch.zeros(2, 10, 10), idx, w)
    assert rec.calls == ["e2emv_match_loss"] and loss.grad_fn is None and loss.dim() == 0
    rec.calls.clear()
    lp = torch.zeros(2, 10, 10, requires_grad=True)
    with torch.no_grad():
        loss = targets.compute_match_loss(lp, idx, w)
    assert rec.calls == ["e2emv_match_loss"] and loss.grad_fn is None
    rec.calls.clear()
    loss = targets.compute_match_loss(lp, idx, w)
    assert rec.calls == ["e2emv_match_loss_tuple"] and loss.grad_fn is not None and loss.dim() == 0
    loss.backward()
    assert rec.calls == ["e2emv_match_loss_tuple", "e2emv_match_loss_tuple_backward"] and lp.grad.shape == (2, 10, 10)


def test_every_value_error_is_raised_before_any_call(monkeypatch):
    from e2e_multi_view_matching_amd import targets
    rec = _stub(monkeypatch)
    result, idx, w = _scores(3, 2, 9)
    with pytest.raises(ValueError, match="scores_0_2"):  # a missing pair
        targets.match_loss_tuple({k: v for k, v in result.items() if k != "scores_0_2"}, idx, w)
    with pytest.raises(ValueError, match="same number of keypoints"):  # image 2 has more keypoints than images 0 and 1
        targets.match_loss_tuple(dict(result, scores_0_2=torch.zeros(2, 10, 12), scores_1_2=torch.zeros(2, 10, 12)), idx, w)
    with pytest.raises(ValueError, match=r"\[B,N\+1,N\+1\]"):  # another batch size than the targets'
        targets.match_loss_tuple({k: torch.zeros(3, 10, 10) for k in result}, idx, w)
    with pytest.raises(ValueError, match=r"\[B,N\+1,N\+1\]"):  # another keypoint count than the targets'
        targets.match_loss_tuple({k: torch.zeros(2, 11, 11) for k in result}, idx, w)
    with pytest.raises(ValueError, match="indices"):
        targets.match_loss_tuple(result, idx.to(torch.int32), w)
    with pytest.raises(ValueError, match="indices"):
        targets.match_loss_tuple(result, idx[:, :, 0], w[:, :, 0])
    with pytest.raises(ValueError, match="weights"):
        targets.match_loss_tuple(result, idx, w.double())
    with pytest.raises(ValueError, match="weights"):
        targets.match_loss_tuple(result, idx, w[..., :-1])
    with pytest.raises(ValueError, match="no tuple"):  # two pairs: no tuple has them
        targets.match_loss_tuple(result, idx[:2], w[:2])
    data = _data(3, 2, 9)
    with pytest.raises(ValueError, match="2..8"):
        targets.gt_matches_tuple(data, 5.0, 15.0, n_images=1)
    with pytest.raises(ValueError, match="2..8"):
        targets.gt_matches_tuple(data, 5.0, 15.0, n_images=9)
    with pytest.raises(ValueError, match="depth1"):
        targets.gt_matches_tuple({k: v for k, v in data.items() if k != "depth1"}, 5.0, 15.0)
    with pytest.raises(ValueError, match="same N"):
        targets.gt_matches_tuple(dict(data, keypoints2=torch.zeros(2, 10, 2)), 5.0, 15.0)
    with pytest.raises(ValueError, match="intr1"):
        targets.gt_matches_tuple(dict(data, intr1=torch.eye(3)[None].repeat(2, 1, 1)), 5.0, 15.0)
    with pytest.raises(ValueError, match="depth maps"):
        targets.gt_matches_tuple(dict(data, depth2=torch.ones(2, 6, 9)), 5.0, 15.0)
    assert rec.calls == []


def test_the_path_has_no_host_synchronisation_in_its_source():
    from e2e_multi_view_matching_amd import targets
    for obj in (targets.gt_matches_tuple, targets.match_loss_tuple, targets._MatchLossTuple, targets._match_loss_tuple_call,
                targets.compute_match_loss):
        src = inspect.getsource(obj)
        for word in (".item(", ".cpu(", ".tolist(", "nonzero", "masked_select", "synchronize"):
            assert word not in src, (obj.__name__, word)


def test_exact_tuple_scene_premise_fp32_oracle_equals_fp64_oracle():
    """The premise of test_gpu_match_loss_tuple.py::test_targets_of_the_tuple_equal_the_per_pair_path on its exact scene, checked wherever
    the suite runs: for EVERY pair of the T-image scene the oracle returns identical targets in fp32 and fp64, and at N = 257 every pair
    holds what the scene is meant to hold - matches, exact arg-min ties, rows whose selected error sits ON a threshold, rows without depth."""
    import test_gpu_match_loss_tuple as G
    for T, B, N in G.TARGET_SHAPES:
        data, (i32, w32), (i64, w64), marg = G.exact_scene_and_oracle(T, B, N)
        P = T * (T - 1) // 2
        assert i32.shape == (P, B, 2, N + 1) and torch.equal(i32, i64), (T, B, N)
        assert torch.equal(w32, w64.to(w32.dtype)), (T, B, N)
        for t in range(T):  # every image's keypoints lie inside its depth map
            k, (H, W) = data["keypoints%d" % t], data["depth%d" % t].shape[-2:]
            assert float(k.min()) >= 0 and float(k[..., 0].max()) < W and float(k[..., 1].max()) < H
        if N < 257:
            continue
        for q, p in enumerate(G.pairs_of(T)):
            m = marg[q]
            fin = m["row_gap"].isfinite()
            n_match = int((i32[q][:, 0] >= 0).sum())
            n_tie = int((m["row_gap"][fin] == 0).sum()) + int((m["col_gap"][m["col_gap"].isfinite()] == 0).sum())
            n_on_thr = int((m["row_thr"] == 0).sum())
            n_bad = int((~fin).sum())
            print(f"T={T} N={N} pair {p}: {n_match} matches, {n_tie} exact ties, {n_on_thr} rows on a threshold, {n_bad} rows without depth")
            assert n_match >= 1 and n_tie >= 1 and n_on_thr >= 1 and n_bad >= 1, p
            assert float(w32[q].max()) > 0 and int((i32[q][:, 0, :-1] == -1).sum()) > 0
