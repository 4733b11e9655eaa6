"""The tuple pose loss, as far as it can be checked without a GPU: the three C entries (``e2emv_w8pt_tuple_backward``,
``e2emv_pose_loss_tuple``, ``e2emv_pose_loss_tuple_backward``) are declared, bound, exported and refuse a NULL context; the Python front
makes fixed call sequences whose length does not depend on the batch size - recorded with a stand-in for the device context -; and every
``ValueError`` of ``pose_loss_tuple`` is raised before any call."""
import ctypes
import os
import re

import pytest
import torch

from test_ba2view_backward import _stub_device

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"e2emv_w8pt_tuple_backward": 13, "e2emv_pose_loss_tuple": 10, "e2emv_pose_loss_tuple_backward": 8}


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
    assert lib.e2emv_w8pt_tuple_backward(None, 1, 2, 8, None, None, None, None, None, None, None, None, None) == _lib.EINVAL
    assert lib.e2emv_pose_loss_tuple(None, 1, 1, None, None, None, None, None, None, None) == _lib.EINVAL
    assert lib.e2emv_pose_loss_tuple_backward(None, 1, 1, None, None, None, None, None) == _lib.EINVAL


def test_the_function_is_exported_from_the_package():
    import e2e_multi_view_matching_amd as E
    assert E.pose_loss_tuple is E.pose.pose_loss_tuple and "pose_loss_tuple" in E.__all__


def _tuple(T, B, N, grad=True, skip_grad=()):
    data, result = {}, {}
    for t in range(T):
        data["keypoints%d" % t] = torch.zeros(B, N, 2)
        data["intr%d" % t] = torch.eye(4)[None].repeat(B, 1, 1)
        data["pose%d" % t] = torch.eye(4)[None].repeat(B, 1, 1)
    pairs = [(i, j) for j in range(T) for i in range(j)]
    for i, j in pairs:
        result["matches%d_%d_%d" % (i, i, j)] = torch.zeros(B, N, dtype=torch.int64)
        result["conf_scores_%d_%d" % (i, j)] = torch.ones(B, N, 1, requires_grad=grad and (i, j) not in skip_grad)
    return data, result, pairs


def test_run_weighted_8_point_tuple_call_sequences(monkeypatch):
    from e2e_multi_view_matching_amd import pose
    rec = _stub_device(monkeypatch)
    data, result, pairs = _tuple(3, 2, 8, grad=False)
    out = pose.run_weighted_8_point_tuple(data, result)
    assert rec.calls == ["e2emv_w8pt_tuple"] and all(out[p][0].grad_fn is None for p in pairs)
    rec.calls.clear()
    data, result, pairs = _tuple(3, 2, 8, skip_grad={(0, 2)})
    with torch.no_grad():  # gradients disabled: today's single call
        out = pose.run_weighted_8_point_tuple(data, result)
    assert rec.calls == ["e2emv_w8pt_tuple"] and all(out[p][0].grad_fn is None for p in pairs)
    rec.calls.clear()
    targets = {p: torch.eye(4)[None].repeat(2, 1, 1) for p in pairs}
    out = pose.run_weighted_8_point_tuple(data, result, choose_closest=True, targets=targets, determine_inliers=True)
    assert rec.calls == ["e2emv_w8pt_tuple"]
    for p in pairs:
        T, info = out[p]
        assert T.shape == (2, 4, 4) and T.requires_grad and not info["confidence"].requires_grad and info["confidence"].shape == (2, 8, 1)
        assert set(info) == {"kpts0_norm", "kpts1_norm", "confidence", "inliers", "pos_depth_mask", "F", "status"}
    sum(out[p][0].sum() for p in pairs).backward()
    assert rec.calls == ["e2emv_w8pt_tuple", "e2emv_w8pt_tuple_backward"]
    assert result["conf_scores_0_2"].grad is None                       # a pair that does not require grad gets None
    for p in ((0, 1), (1, 2)):
        g = result["conf_scores_%d_%d" % p].grad
        assert g is not None and g.shape == (2, 8, 1) and g.dtype == torch.float32
    # a missing pair: the per-pair fallback, untouched
    rec.calls.clear()
    del result["matches0_0_1"]
    with torch.no_grad():
        out = pose.run_weighted_8_point_tuple(data, result)
    assert out[(0, 1)] == (None, None) and rec.calls == ["e2emv_gather_matched", "e2emv_w8pt"] * 2


def _sequences(P, ba):
    fwd = ["e2emv_relative_pose"] * P + (["e2emv_gather_matched"] * P if ba else []) + ["e2emv_w8pt_tuple"] + \
        (["e2emv_apply_mask", "e2emv_ba_2view"] if ba else []) + ["e2emv_pose_loss_tuple"]
    bwd = ["e2emv_pose_loss_tuple_backward"] + (["e2emv_ba_2view_backward", "e2emv_apply_mask"] if ba else []) + ["e2emv_w8pt_tuple_backward"]
    return fwd, bwd


@pytest.mark.parametrize("ba", [0, 3])
@pytest.mark.parametrize("T,B", [(3, 1), (3, 5), (5, 2)])
def test_pose_loss_tuple_call_sequences_do_not_depend_on_the_batch(monkeypatch, ba, T, B):
    from e2e_multi_view_matching_amd import pose
    rec = _stub_device(monkeypatch)
    data, result, pairs = _tuple(T, B, 9)
    fwd, bwd = _sequences(len(pairs), ba)
    out = pose.pose_loss_tuple(data, result, ba_iterations=ba)
    assert rec.calls == fwd
    assert set(out) == {"rot_loss", "transl_loss", "poses"} and list(out["poses"]) == pairs
    assert out["rot_loss"].dim() == 0 and out["transl_loss"].dim() == 0 and out["rot_loss"].requires_grad and out["transl_loss"].requires_grad
    assert all(out["poses"][p].shape == (B, 4, 4) for p in pairs)
    (out["rot_loss"] + out["transl_loss"]).backward()
    assert rec.calls == fwd + bwd
    for i, j in pairs:
        g = result["conf_scores_%d_%d" % (i, j)].grad
        assert g is not None and g.shape == (B, 9, 1)
    # without a graph: the forward's calls alone, and losses without one
    rec.calls.clear()
    with torch.no_grad():
        out = pose.pose_loss_tuple(data, result, ba_iterations=ba)
    assert rec.calls == fwd and not out["rot_loss"].requires_grad


def test_pose_loss_tuple_raises_before_any_call(monkeypatch):
    from e2e_multi_view_matching_amd import pose
    rec = _stub_device(monkeypatch)
    data, result, _ = _tuple(3, 2, 7)
    with pytest.raises(ValueError, match="at least 8"):
        pose.pose_loss_tuple(data, result)
    data, result, _ = _tuple(3, 2, 9)
    with pytest.raises(ValueError, match="ba_iterations"):
        pose.pose_loss_tuple(data, result, ba_iterations=-1)
    bad = dict(data, keypoints2=torch.zeros(2, 10, 2))
    with pytest.raises(ValueError, match="same number of keypoints"):
        pose.pose_loss_tuple(bad, result)
    with pytest.raises(ValueError, match="pose1"):
        pose.pose_loss_tuple({k: v for k, v in data.items() if k != "pose1"}, result)
    with pytest.raises(ValueError, match="matches0_0_2"):
        pose.pose_loss_tuple(data, {k: v for k, v in result.items() if k != "matches0_0_2"})
    with pytest.raises(ValueError, match="conf_scores_1_2"):
        pose.pose_loss_tuple(data, {k: v for k, v in result.items() if k != "conf_scores_1_2"})
    assert rec.calls == []


@pytest.mark.parametrize("shape", [(3, 2, 65), (5, 2, 257)])
def test_the_oracle_comparison_is_well_conditioned_on_the_chosen_seeds(shape):
    """A premise of tests/test_gpu_pose_loss_tuple.py::test_tuple_gradient_against_autograd_through_the_oracle, in the oracle alone: for every
    (pair, sample) the fp64 gradient from the fp32-rounded camera coordinates and from coordinates formed in fp64 agree to 1e-4 relative - the
    gradient divides by the gap between the two smallest eigenvalues, and a sample where rounding the inputs moves it further than that
    cannot be held to 1e-3 on any fp32 implementation."""
    import test_gpu_pose_loss_tuple as G
    T, B, N = shape
    seed = G.ORACLE_SHAPES[shape]
    rounded, exact = G.oracle_gradients(T, B, N, seed, True), G.oracle_gradients(T, B, N, seed, False)
    worst = 0.0
    for p in G.pairs_of(T):
        for b in range(B):
            assert bool(rounded[p][b].isfinite().all()) and float(rounded[p][b].norm()) > 0
            worst = max(worst, float((rounded[p][b] - exact[p][b]).norm() / exact[p][b].norm()))
    print(f"{shape} seed {seed}: largest relative change of a gradient under fp32 rounding of the inputs {worst:.3e}")
    assert worst < 1e-4, (shape, seed, worst)


def test_pose_loss_tuple_has_no_boolean_indexing_and_no_item():
    """Nothing in the function's path synchronises with the host: no ``.item()``, no ``[valid]`` selection, no ``.cpu()`` / ``.tolist()`` in
    the source of the function and of the autograd Functions it goes through."""
    import inspect
    from e2e_multi_view_matching_amd import pose
    for obj in (pose.pose_loss_tuple, pose._PoseLossTuple, pose._W8ptTuplePose, pose._tuple_state, pose._w8pt_tuple_call, pose._pose_loss_tuple_call,
                pose._Ba2ViewPose, pose._MaskConfidence, pose.mask_confidence):
        src = inspect.getsource(obj)
        for word in (".item(", ".cpu(", ".tolist(", ".nonzero(", "[valid]", "[vb]", "masked_select", "synchronize"):
            assert word not in src, (obj.__name__, word)
