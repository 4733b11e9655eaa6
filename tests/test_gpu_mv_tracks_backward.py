"""GPU: backward pass of the track route (``e2emv_mv_tuple_ba_tracks_backward``, csrc/mvtracks.hip; Python:
``refine_tuple_poses_batch(..., tracks=True, repair_rounds=R)``) against autograd through the restated track weights
(tests/mvtracks_backward_restatement.py) -> the restated solver (tests/mvba_backward_restatement.py, ``R.run``) -> extrinsics, on the
problems the device copies out (``_tuple_problems_tracks``), contracted with a fixed-seed ``g_out_extr``.

Every comparison first asserts that it cannot pass vacuously: device and restatement took the same decisions (iterations and termination
of the summary), for max_iterations >= 1 at least one step was accepted, and the scene holds the track sizes it is meant to hold (the
seeds are checked on the CPU by tests/test_mv_tracks_backward.py with the host union-find and the host repair).

Cases (``CASES``), the smallest shapes at which the new code can go wrong:
    three_views       B = 2, T = 3, N = 40, threshold 0.6, pair (0, 2) without a matches entry: tracks of 2 and 3 views, a NULL d_gconf entry
    thinned           T = 5, 24 keypoints, 10 % wrong matches, thinned (see ``wrong_and_thinned_scene``), no repair: tracks of 2 .. 5 views,
                      dropped conflicts get zeros
    thinned_repaired  the same with 4 repair rounds: a cut edge inside its final track gets a gradient, cut edges between two tracks get 0
    cut_inside        the handcrafted graph of test_a_cut_edge_inside_its_final_track_still_weighs through ``_sparse_inputs`` (its three
                      keypoints moved onto one scene point, so that the solver has something to minimise), 2 rounds
    many              T = 3 with 400 keypoints: 280 tracks, more than the 256 threads of the weights kernel, and 840 observations, more than
                      the solver's 512 threads (planted scenes share 70 % of their keypoints: 300 keypoints give 210 tracks, which is
                      not what the case is for); max_iterations = 3 only
    ragged            the last image has 48 keypoints, the others N = 40 (Nmax > N); matches that point at rows >= 48 are dropped, matches
                      into rows 41 and 45 are edges and those rows members of tracks
    two_channels      three_views with a second confidence channel: the same gradient in channel 0, exactly 0 in channel 1

Bar, the scheme of tests/test_gpu_mv_ba_backward.py: elementwise |g - g_ref| <= REL_BAR max|g_ref| + 2^-24 |g_ref| (the last term is the
fp32 output format), max over the tuple's pairs; REL_BAR = ten times the largest distance to the restatement measured on the MI355X over
the cases (ten: the margin that file uses for rounding-order differences between a shared-algorithm restatement and the device); it stays
under GRADIENT_BAR = 1e-3, which every comparison also asserts.  max_iterations = 0 is exact: every gradient is 0.
Measured on the MI355X, largest |g - g_ref| / max|g_ref| over the tuples of a case, max_iterations = 1 / 3 / 50 (accepted steps):
    three_views       3.6e-08 (1 accepted)   3.4e-08 (3 accepted)   3.4e-08 (3 accepted)
    thinned           1.5e-08 (1 accepted)   4.2e-08 (3 accepted)   4.2e-08 (3 accepted)
    thinned_repaired  2.7e-08 (1 accepted)   3.6e-08 (3 accepted)   3.6e-08 (3 accepted)
    cut_inside        2.2e-08 (1 accepted)   2.9e-08 (3 accepted)   2.9e-08 (3 accepted)
    many                                     3.0e-08 (3 accepted)
    ragged            5.0e-08 (1 accepted)   2.5e-08 (3 accepted)   3.1e-08 (5 accepted)
    two_channels                             3.4e-08 (3 accepted)
The largest is 5.0e-8 (ragged after one accepted step): the distances are those of the fp32 output format (2^-24 = 6.0e-8 of a value),
the fp64 part below them is that of the solver level (2.5e-9 at most in tests/test_gpu_mv_ba_backward.py).  REL_BAR = 5.0e-7.
T = 2 against the pair route: no element differed (largest entry 0.0276).
"""
import functools

import numpy as np
import pytest
import torch

import mvba_backward_restatement as R
import mvtracks_backward_restatement as W
from test_gpu_mv_ba_backward import tuple_inputs
from test_gpu_mv_batch import _slice
from test_gpu_mv_track_repair import _sparse_inputs
from test_gpu_mv_tracks import _pairs, _perturbed_start, planted_scene

pytestmark = pytest.mark.gpu

MEASURED = 5.0e-8  # largest distance measured on the MI355X (see the table above)
GRADIENT_BAR = 1e-3
REL_BAR = 10 * MEASURED
EPS32 = 2.0 ** -24
GPU = torch.device("cuda", 0)


def _cut_inside_scene():
    T, N = 3, 70
    data, result = _sparse_inputs(T, N, W.CUT_GRAPH)
    gt = _perturbed_start(np.tile(np.eye(4), (T, 1, 1)), np.random.default_rng(0), rot=0.2, tr=0.5)
    X = np.array([0.3, -0.2, 5.0, 1.0])
    for t in range(T):  # keypoint 0 of every image = the projection of one scene point
        q = gt[t, :3] @ X
        K = data[f"intr{t}"][0].numpy()
        data[f"keypoints{t}"][0, 0] = torch.tensor([K[0, 0] * q[0] / q[2] + K[0, 2], K[1, 1] * q[1] / q[2] + K[1, 2]])
    return data, result, _perturbed_start(gt, np.random.default_rng(1))[None]


def _ragged_scene():
    T = 3
    data, result, _, start = planted_scene(43, T=T, n_kpts=40)
    extra = torch.from_numpy(np.random.default_rng(9).uniform(0, 640, (1, 8, 2)).astype(np.float32))
    data["keypoints2"] = torch.cat([data["keypoints2"], extra], 1).contiguous()
    m02, m12 = result["matches0_0_2"], result["matches1_1_2"]
    m02[0, [3, 11, 27]] = torch.tensor([48, 49, 60])  # at and behind the end of image 2: no edges
    for row, target in ((5, 41), (19, 45)):           # rows of image 2 that only the label stride Nmax reaches, as members of tracks:
        assert m12[0, row] >= 0
        data["keypoints2"][0, target] = data["keypoints2"][0, m12[0, row]]  # (the same image point: the geometry stays planted)
        m12[0, row] = target                          # keypoint `row` of image 1 now matches it, and the keypoint of image 0 that
        m02[0, result["matches0_0_1"][0] == row] = -1  # matches `row` loses its own match into image 2 (it would make a conflict)
    return data, result, start[None]


def _two_channels(result):
    out = dict(result)
    for k, c in result.items():
        if k.startswith("conf_scores_"):
            out[k] = torch.cat([c, c + 0.25], 2).contiguous()
    return out


@functools.lru_cache(maxsize=None)
def case(name):
    """(T, data, result, start [B,T,4,4], conf_thresh, repair_rounds, track sizes the scene is meant to hold)."""
    if name in ("three_views", "two_channels"):
        data, result, start, _ = tuple_inputs()
        return 3, data, (_two_channels(result) if name == "two_channels" else result), start, 0.6, 0, {2, 3}
    if name in ("thinned", "thinned_repaired"):
        data, result, _, start = W.wrong_and_thinned_scene()
        return 5, data, result, start[None], 0.0, 4 if name == "thinned_repaired" else 0, {2, 3, 4, 5}
    if name == "cut_inside":
        return (3,) + _cut_inside_scene() + (0.0, 2, {3})
    if name == "many":
        data, result, _, start = planted_scene(44, T=3, n_kpts=400)
        return 3, data, result, start[None], 0.0, 0, {3}
    if name == "ragged":
        return (3,) + _ragged_scene() + (0.0, 0, {3})
    raise KeyError(name)


CASES = {"three_views": (0, 1, 3, 50), "thinned": (0, 1, 3, 50), "thinned_repaired": (0, 1, 3, 50), "cut_inside": (0, 1, 3, 50), "many": (3,),
         "ragged": (0, 1, 3, 50), "two_channels": (3,)}


def g_extr(B, T):
    return np.random.default_rng(5).normal(size=(B, T, 4, 4))


def _to(result):
    return {k: v.to(GPU) for k, v in result.items()}


@functools.lru_cache(maxsize=None)
def device_problems(name):
    """What the device copies out for the case: (problems, label [B,T,Nmax] numpy, stats [B,4])."""
    from e2e_multi_view_matching_amd import multi_view
    T, data, result, start, thresh, rounds, _ = case(name)
    intr, kdim, nb = multi_view._tuple_intrinsics(T, data, GPU, len(start))
    problems, label, stats = multi_view._tuple_problems_tracks(T, data, _to(result), thresh, intr, kdim, nb, start, repair_rounds=rounds)
    return problems, label.cpu().numpy(), stats


@functools.lru_cache(maxsize=None)
def reference(name, K):
    """Per tuple (gradients per pair [N, channels] or None, info of the restated run, its extrinsics [T,3,4]): computed once, shared, left
    unchanged."""
    T, data, result, start, thresh, rounds, sizes = case(name)
    problems, label, stats = device_problems(name)
    out = []
    for b, pr in enumerate(problems):
        prob = dict(n_cams=T, fixed=0, intr=pr[2], cam_idx=pr[3], pt_idx=pr[4], obs=pr[5], wts=pr[6], cams=pr[7], pts=pr[8])
        edges, Nmax = W.kept_edges(T, data, result, b, thresh)
        assert Nmax == label.shape[2]
        assert set(np.bincount(pr[4])) == sizes, (name, b, np.bincount(np.bincount(pr[4])))  # the track sizes the scene is meant to hold
        conf = W.confidences(T, result, b)
        wts = W.restated_weights(label[b], edges, conf)
        assert np.allclose(wts.detach().numpy(), prob["wts"], rtol=1e-12, atol=0)  # the weights the device built
        co, _, info = R.run(prob, torch.tensor(prob["cams"]), torch.tensor(prob["pts"]), wts, K)
        Rm = R.transform(co, torch.zeros(T, 3, dtype=torch.float64))[1]
        E = torch.cat([Rm, co[:, 3:, None]], 2)
        have = [c for c in conf if c is not None]
        loss = (E * torch.as_tensor(g_extr(len(problems), T)[b, :, :3])).sum()
        grads = iter(torch.autograd.grad(loss, have, allow_unused=True) if loss.requires_grad else [None] * len(have))
        per_pair = [None if c is None else (lambda g: np.zeros(tuple(c.shape)) if g is None else g.numpy())(next(grads)) for c in conf]
        out.append((per_pair, info, E.detach().numpy(), W.inside_tracks(label[b], edges), edges))
    return out


def run_device(T, data, result, start, thresh, rounds, K, g, leave_out=()):
    """Forward and backward entry on the same labels: (gconf per pair [B,N,channels] numpy or None, out, summary, stats)."""
    from e2e_multi_view_matching_amd import _lib, multi_view
    inp, label, stats = multi_view._tracks_labels(T, data, _to(result), thresh, rounds)
    intr, kdim, nb = multi_view._tuple_intrinsics(T, data, GPU, len(start))
    out, summary = np.zeros_like(start), np.zeros((len(start), 4))
    multi_view._tracks_entry_call("e2emv_mv_tuple_ba_tracks", T, inp, label, stats, thresh, intr, kdim, nb, start, K, multi_view._p(out),
                                  multi_view._p(summary))
    gouts = [None if (c is None or q in leave_out) else torch.full_like(c, float("nan")) for q, c in enumerate(inp["conf"])]
    pg, owner = _lib.ptr_array(gouts)
    multi_view._tracks_entry_call("e2emv_mv_tuple_ba_tracks_backward", T, inp, label, stats, thresh, intr, kdim, nb, start, K,
                                  multi_view._p(np.ascontiguousarray(g)), pg)
    del owner
    return [None if go is None else go.cpu().numpy() for go in gouts], out, summary, stats


@functools.lru_cache(maxsize=None)
def device(name, K):
    T, data, result, start, thresh, rounds, _ = case(name)
    return run_device(T, data, result, start, thresh, rounds, K, g_extr(len(start), T))


@pytest.mark.parametrize("name,K", [(n, K) for n, Ks in CASES.items() for K in Ks])
def test_device_against_the_restatement(gpu, name, K):
    T, data, result, start, thresh, rounds, _ = case(name)
    gouts, out, summary, stats = device(name, K)
    ref = reference(name, K)
    assert REL_BAR < GRADIENT_BAR
    present = [q for q, (i, j) in enumerate(_pairs(T)) if f"matches{i}_{i}_{j}" in result]
    assert [q for q, g in enumerate(gouts) if g is not None] == present
    for b, (per_pair, info, E, inside, edges) in enumerate(ref):
        assert int(summary[b, 2]) == info["iterations"] and R.TERMS[int(summary[b, 3])] == info["termination"]  # the same decisions
        accepted = sum(a for _, _, a in info["schedule"]["passes"])
        assert accepted >= 1 or K == 0
        assert np.abs(E - out[b, :, :3]).max() < 1e-8
        scale = max(np.abs(r).max() for r in per_pair if r is not None)
        worst = 0.0
        for q in present:
            g, r = gouts[q][b].astype(np.float64), per_pair[q]
            assert g.shape == r.shape and np.isfinite(g).all()  # every element was written
            worst = max(worst, np.abs(g - r).max() / scale if scale > 0 else float(np.abs(g).max()))
        print(f"MEASURED {name} tuple {b} K={K} accepted={accepted} stats={stats[b].tolist()}: {worst:.2e} of max|g_ref| = {scale:.3g}")
        for q in present:
            g, r = gouts[q][b].astype(np.float64), per_pair[q]
            assert (np.abs(g - r) <= GRADIENT_BAR * scale).all()
            assert (np.abs(g - r) <= REL_BAR * scale + EPS32 * np.abs(r)).all()
            assert not g[:, 1:].any()  # channels above 0 are exactly 0
            if K == 0:
                assert not g.any()  # no step: every gradient is exactly 0
        if K > 0:  # non-zero exactly on the kept edges inside tracks: dropped rows, dropped conflicts and edges between tracks get 0
            hit = {q: np.zeros(gouts[q][b].shape[0], bool) for q in present}
            for (q, n, _, _), ins in zip(edges, inside):
                hit[q][n] = bool(ins)
            assert scale > 0 and inside.any()
            for q in present:
                assert np.array_equal(gouts[q][b][:, 0] != 0, hit[q]), (name, b, q)
            if name in ("thinned", "thinned_repaired"):
                assert not inside.all()
    if name == "many":
        assert (stats[:, 0] > 256).all() and (stats[:, 1] > 512).all(), stats
    if name == "ragged":
        assert data["keypoints2"].shape[1] == 48 > result["matches0_0_1"].shape[1] and int((result["matches0_0_2"] >= 48).sum()) == 3
        label = device_problems(name)[1]
        assert label.shape == (1, 3, 48) and (label[0, 2, [41, 45]] >= 0).all()
    if name == "two_channels":
        one = device("three_views", K)[0]
        assert all(np.array_equal(g[:, :, 0], o[:, :, 0]) for g, o in zip(gouts, one) if g is not None)


def test_two_images_agree_with_the_pair_route(gpu):
    """T = 2 with one-to-one matches: the gradient equals e2emv_mv_tuple_ba_backward + e2emv_mv_collect_backward on the same matches up to
    the fp32 rounding of both outputs (2^-24 of the value each) and the order in which D is summed (fp64, a few hundred terms: 1e-12 of
    the largest entry)."""
    from e2e_multi_view_matching_amd import _lib, multi_view
    data, result, _, start = planted_scene(23, drop=0.2, T=2)
    start, K, thresh = start[None], 3, 0.6
    g = g_extr(1, 2)
    (got,), out, summary, stats = run_device(2, data, result, start, thresh, 0, K, g)
    res = _to(result)
    inp = multi_view._collect_inputs(2, data, res)
    collected = multi_view._collect_call(2, inp, thresh)
    counts = collected[3].cpu().numpy()
    assert stats[0, 0] == counts[0] > 20 and int(summary[0, 2]) >= 1
    intr, kdim, nb = multi_view._tuple_intrinsics(2, data, GPU, 1)
    gm = torch.zeros_like(collected[2])
    multi_view._tuple_ba_call("e2emv_mv_tuple_ba_backward", 2, collected, counts, intr, kdim, nb, start, K, multi_view._p(g), _lib.ptr(gm))
    want = torch.full_like(inp["cs"][0], float("nan"))
    ptrs = [_lib.ptr_array(lst) for lst in (inp["ms"], inp["cs"], [want])]
    _lib.context(GPU).call("e2emv_mv_collect_backward", 1, 2, inp["N"], multi_view._p(inp["n1"]), ptrs[0][0], ptrs[1][0], 1, float(thresh),
                           _lib.ptr(gm), ptrs[2][0], _lib.stream_ptr(GPU))
    torch.cuda.synchronize()
    want = want.cpu().numpy().astype(np.float64)
    got = got.astype(np.float64)
    print("T = 2: largest difference to the pair route", np.abs(got - want).max(), "of", np.abs(want).max())
    assert np.abs(want).max() > 0 and np.array_equal(got != 0, want != 0)
    assert (np.abs(got - want) <= 2 * EPS32 * np.abs(want) + 1e-12 * np.abs(want).max()).all()


def _cat(parts):
    d0 = parts[0]
    return {k: (torch.cat([p[k] for p in parts], 0) if torch.is_tensor(v) else v) for k, v in d0.items()}


def test_batch_position_an_empty_tuple_and_repeatability(gpu):
    """[A, a tuple without any track, B]: the middle tuple returns its start and all its gradients are zero; A and B give the same words as
    each alone and in the order [B, A]; two runs give the same words."""
    T, K, rounds = 5, 3, 4
    dA, rA, _, sA = W.wrong_and_thinned_scene()
    dB, rB, _, sB = W.wrong_and_thinned_scene(seed=45)
    rE = {k: (torch.full_like(v, -1) if k.startswith("matches") else v.clone()) for k, v in rA.items()}
    sE = _perturbed_start(np.tile(np.eye(4), (T, 1, 1)), np.random.default_rng(2), rot=0.3, tr=1.0)
    data, result, start = _cat([dA, dA, dB]), _cat([rA, rE, rB]), np.stack([sA, sE, sB])
    g = g_extr(3, T)
    gouts, out, summary, stats = run_device(T, data, result, start, 0.0, rounds, K, g)
    assert stats[1].tolist()[:2] == [0, 0] and stats[0, 0] > 0 and stats[2, 0] > 0 and (summary[[0, 2], 2] >= 1).all()
    assert np.abs(out[1] - start[1]).max() < 1e-14 and np.array_equal(out[1, :, :3, 3], start[1, :, :3, 3])
    assert all(not go[1].any() and go[0].any() and go[2].any() and np.isfinite(go).all() for go in gouts)
    again = run_device(T, data, result, start, 0.0, rounds, K, g)
    assert all(np.array_equal(x, y) for x, y in zip(again[0], gouts)) and np.array_equal(again[1], out)
    for b, (d, r, s) in ((0, (dA, rA, sA)), (2, (dB, rB, sB))):
        alone = run_device(T, d, r, s[None], 0.0, rounds, K, g[b:b + 1])
        assert all(np.array_equal(x[0], y[b]) for x, y in zip(alone[0], gouts)) and np.array_equal(alone[1][0], out[b])
    swapped = run_device(T, _cat([dB, dA]), _cat([rB, rA]), np.stack([sB, sA]), 0.0, rounds, K, g[[2, 0]])
    assert all(np.array_equal(x[0], y[2]) and np.array_equal(x[1], y[0]) for x, y in zip(swapped[0], gouts))
    assert np.array_equal(swapped[1][0], out[2]) and np.array_equal(swapped[1][1], out[0])


def test_a_null_entry_leaves_its_pair_out(gpu):
    T, data, result, start, thresh, rounds, _ = case("thinned_repaired")
    full = device("thinned_repaired", 3)[0]
    part = run_device(T, data, result, start, thresh, rounds, 3, g_extr(1, T), leave_out=(1, 7))[0]
    assert part[1] is None and part[7] is None
    assert all(np.array_equal(p, f) for q, (p, f) in enumerate(zip(part, full)) if q not in (1, 7))


def test_python_route_fills_every_confidence_gradient(gpu):
    """A rotation-angle loss on ``refine_tuple_poses_batch(..., tracks=True, repair_rounds=4)`` reaches every present conf_scores_{i}_{j}:
    finite, non-zero exactly on the edges inside tracks; it is the C entry's gradient; without a graph the same extrinsics, no grad_fn."""
    from e2e_multi_view_matching_amd import multi_view
    T = 5
    data, result, gt, start = W.wrong_and_thinned_scene()
    del result["matches1_1_3"], result["conf_scores_1_3"]
    res = _to(result)
    confs = {k: v.clone().requires_grad_() for k, v in res.items() if k.startswith("conf_scores_")}
    res.update(confs)
    E = multi_view.refine_tuple_poses_batch(T, data, res, start[None], 0.0, tracks=True, repair_rounds=4)
    assert E.shape == (1, T, 4, 4) and E.dtype == torch.float64 and E.requires_grad
    G = torch.as_tensor(gt)[None]
    loss = 0.0
    for i, j in _pairs(T):  # tuple_pose_errors' rotation angle of every image pair
        rel_gt = G[:, j, :3, :3] @ G[:, i, :3, :3].transpose(1, 2)
        rel = E[:, j, :3, :3] @ E[:, i, :3, :3].transpose(1, 2)
        loss = loss + torch.acos((((rel_gt * rel).sum((1, 2)) - 1.0) / 2.0).clamp(-1.0, 1.0)).sum()
    loss.backward()
    label = multi_view.match_tracks(T, data, _to(result), 0.0, repair_rounds=4)[0].cpu().numpy()[0]
    edges, _ = W.kept_edges(T, data, result, 0, 0.0)
    inside = W.inside_tracks(label, edges)
    assert len(confs) == 9 and inside.any() and not inside.all()
    hit = {q: np.zeros(24, bool) for q in range(10)}
    for (q, n, _, _), ins in zip(edges, inside):
        hit[q][n] = bool(ins)
    for q, (i, j) in enumerate(_pairs(T)):
        if (i, j) == (1, 3):
            continue
        c = confs[f"conf_scores_{i}_{j}"]
        assert c.grad is not None and c.grad.shape == c.shape and c.grad.dtype == c.dtype and c.grad.device == c.device
        assert bool(c.grad.isfinite().all()) and np.array_equal(c.grad.cpu().numpy()[0, :, 0] != 0, hit[q]), (i, j)
    plain = multi_view.refine_tuple_poses_batch(T, data, {k: v.detach() for k, v in res.items()}, start[None], 0.0, tracks=True, repair_rounds=4)
    assert plain.grad_fn is None and not plain.requires_grad and np.array_equal(plain.numpy(), E.detach().numpy())
    with torch.no_grad():
        quiet = multi_view.refine_tuple_poses_batch(T, data, res, start[None], 0.0, tracks=True, repair_rounds=4)
    assert quiet.grad_fn is None and np.array_equal(quiet.numpy(), plain.numpy())
    with pytest.raises(ValueError, match="max_iterations"):
        multi_view.refine_tuple_poses_batch(T, data, res, start[None], 0.0, max_iterations=-1, tracks=True)


def test_error_paths(gpu):
    """NULL gradient arrays and a ``stats`` that disagrees with T are E2EMV_EINVAL before any launch; a tape larger than the device's
    memory is E2EMV_ENOMEM; the context goes on working."""
    from e2e_multi_view_matching_amd import _lib, multi_view
    T, data, result, start, thresh, rounds, _ = case("three_views")
    inp, label, stats = multi_view._tracks_labels(T, data, _to(result), thresh, rounds)
    intr, kdim, nb = multi_view._tuple_intrinsics(T, data, GPU, len(start))
    g = np.ascontiguousarray(g_extr(len(start), T))
    gouts = [None if c is None else torch.full_like(c, float("nan")) for c in inp["conf"]]
    pg, owner = _lib.ptr_array(gouts)

    def call(stats=stats, K=3, g_ptr=multi_view._p(g), pg=pg):
        try:
            multi_view._tracks_entry_call("e2emv_mv_tuple_ba_tracks_backward", T, inp, label, stats, thresh, intr, kdim, nb, start, K, g_ptr, pg)
        except _lib.E2EMVError as err:
            return err.code, str(err)
        return 0, ""

    assert call(g_ptr=None)[0] == _lib.EINVAL and call(pg=None)[0] == _lib.EINVAL
    for bad in ([stats[0, 0], T * stats[0, 0] + 1], [stats[0, 0], 2 * stats[0, 0] - 1], [-1, 0]):
        wrong = stats.copy()
        wrong[0, :2] = bad
        code, text = call(stats=wrong)
        assert code == _lib.EINVAL and "views per track" in text, (bad, code, text)
    code, text = call(K=2 ** 31 - 1)
    assert code == _lib.ENOMEM and "tape" in text
    assert all(bool(go.isnan().all()) for go in gouts if go is not None)  # nothing was written by the refused calls
    assert call() == (0, "")
    want = device("three_views", 3)[0]
    assert all(np.array_equal(go.cpu().numpy(), w) for go, w in zip(gouts, want) if go is not None)
    del owner
