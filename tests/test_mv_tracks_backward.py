"""Backward pass of the track route (``refine_tuple_poses_batch(..., tracks=True)``, ``e2emv_mv_tuple_ba_tracks_backward``), the part that
needs no device: the torch restatement of the track weights (tests/mvtracks_backward_restatement.py) is pinned against ``host_problem`` of
tests/test_gpu_mv_tracks.py, its closed-form adjoint - what the kernel implements - against autograd and central finite differences,
the zero rules are exact, and the Python front raises its errors before any device call.

Bars.  Weights: rtol 1e-12 (fp64 means and one sum of at most a few hundred values, the same order on both sides).  Closed form against
autograd: 1e-12 of the largest entry (both fp64, sums of two terms per edge and one dot product in another order).  Finite differences:
the step FD_H = 1e-4 and the bar FD_BAR of tests/test_mv_ba_backward.py (the weights are a rational function of the confidences; the
truncation error of a central difference at that step is some 1e-8 of the largest entry)."""
import inspect
import os

import numpy as np
import pytest
import torch

import mvtracks_backward_restatement as W
from test_gpu_mv_track_repair import _sparse_inputs, edge_arrays, host_repair
from test_gpu_mv_tracks import _pairs, host_edges, host_labels, host_problem, planted_scene
from test_mv_ba_backward import FD_BAR, FD_H, GRADIENT_BAR, _no_device

CUT_GRAPH = W.CUT_GRAPH


def _scene(name):
    """(T, data, result, conf_thresh, label [T, Nmax], extr [T,4,4]) of the three labellings the weights are pinned on."""
    if name == "three_views":
        T, thresh = 3, 0.6
        data, result, _, start = planted_scene(41, T=T, n_kpts=40)
    elif name == "wrong_matches":
        T, thresh = 5, 0.0
        data, result, _, start = planted_scene(3, wrong=0.1, T=T, n_kpts=24)
    elif name.startswith("thinned"):
        T, thresh = 5, 0.0
        data, result, _, start = W.wrong_and_thinned_scene()
    else:
        T, thresh = 3, 0.0
        data, result = _sparse_inputs(T, 70, CUT_GRAPH)
        start = np.tile(np.eye(4), (T, 1, 1))
    if name == "thinned_repaired":
        eid, x, y, conf, Nmax = edge_arrays(T, data, result, 0, thresh)
        label = host_repair(T, Nmax, eid, x, y, conf, 4)[0]
    elif name == "cut_inside":
        eid, x, y, conf, Nmax = edge_arrays(T, data, result, 0, thresh)
        label, stats, cuts, live = host_repair(T, Nmax, eid, x, y, conf, 2)
        # the 0.1 edge, row 0 of pair (0, 2) = edge id 70, is cut in round 1 and lies inside the final track
        assert [c.tolist() for c in cuts] == [[70], [1]] and stats.tolist() == [1, 3, 0, 2]
        assert label[0, 0] == label[2, 0] == 0
    else:
        edges, Nmax = host_edges(T, data, result, 0, thresh)
        label, stats = host_labels(T, Nmax, edges)
    return T, data, result, thresh, label, start


NAMES = ["three_views", "wrong_matches", "cut_inside", "thinned", "thinned_repaired"]


@pytest.mark.parametrize("name", NAMES)
def test_restated_weights_are_host_problems(name):
    T, data, result, thresh, label, start = _scene(name)
    edges, Nmax = W.kept_edges(T, data, result, 0, thresh)
    want = host_problem(T, data, 0, label, host_edges(T, data, result, 0, thresh)[0], start, svd_points=False)
    got = W.restated_weights(label, edges, W.confidences(T, result, 0)).detach().numpy()
    views = np.bincount(want[1])
    print(name, "tracks by views", np.bincount(views).tolist(), "largest relative difference", (np.abs(got - want[3]) / want[3]).max())
    assert got.shape == want[3].shape and len(got) > 0
    assert np.allclose(got, want[3], rtol=1e-12, atol=0)
    assert [p for _, p in W.track_observations(label)] == want[1].tolist()
    if name == "three_views":
        assert set(views) == {2, 3}
    if name.startswith("thinned"):
        assert set(views) == {2, 3, 4, 5}
    if name == "cut_inside":
        assert views.tolist() == [3] and [len(k) for k in W.observation_edges(label, edges)] == [2, 2, 2]  # the cut edge still counts


@pytest.mark.parametrize("name", NAMES)
def test_closed_form_is_autograd_and_finite_differences(name):
    T, data, result, thresh, label, _ = _scene(name)
    edges, _ = W.kept_edges(T, data, result, 0, thresh)
    conf = W.confidences(T, result, 0)
    O = len(W.track_observations(label))
    g_w = np.random.default_rng(11).normal(size=(O, 2))
    closed, auto = W.closed_form(label, edges, conf, g_w), W.autograd_form(label, edges, conf, g_w)
    scale = max(np.abs(a).max() for a in auto)
    worst = max(np.abs(c - a).max() for c, a in zip(closed, auto)) / scale
    print(f"{name}: closed form - autograd {worst:.2e} of the largest entry {scale:.3g}")
    assert scale > 0 and worst <= 1e-12
    inside = W.inside_tracks(label, edges)
    assert inside.any()
    for (q, n, _, _), ins in zip(edges, inside):
        assert (closed[q][n, 0] != 0.0) == bool(ins) and (auto[q][n, 0] != 0.0) == bool(ins)
    # central differences of <g_w, w(conf)> on edges inside tracks, every decision (labels, keep rule) held fixed

    def loss(q, n, d):
        c = [None if t is None else t.detach().clone() for t in conf]
        c[q][n, 0] += d
        return float((W.restated_weights(label, edges, c) * torch.as_tensor(g_w)).sum())

    rng = np.random.default_rng(7)
    worst = 0.0
    for k in rng.choice(np.flatnonzero(inside), size=min(6, int(inside.sum())), replace=False):
        q, n = edges[k][:2]
        d = (loss(q, n, FD_H) - loss(q, n, -FD_H)) / (2 * FD_H)
        worst = max(worst, abs(d - closed[q][n, 0]) / scale)
    print(f"{name}: finite differences - closed form {worst:.2e} of the largest entry")
    assert worst <= FD_BAR and FD_BAR < GRADIENT_BAR


def _both(T, data, result, thresh, label=None, seed=3):
    edges, Nmax = W.kept_edges(T, data, result, 0, thresh)
    if label is None:
        label = host_labels(T, Nmax, host_edges(T, data, result, 0, thresh)[0])[0]
    conf = W.confidences(T, result, 0)
    g_w = np.random.default_rng(seed).normal(size=(len(W.track_observations(label)), 2))
    return edges, label, W.closed_form(label, edges, conf, g_w), W.autograd_form(label, edges, conf, g_w)


def test_a_conflicting_component_gets_exact_zeros():
    """Without repair the wrong matches turn their components into conflicts: their nodes are unlabelled and every edge of theirs gets
    exactly 0, on rows that the keep rule keeps."""
    T = 5
    data, result, _, _ = planted_scene(3, wrong=0.1, T=T, n_kpts=24)
    edges, label, closed, auto = _both(T, data, result, 0.0)
    Nmax = label.shape[1]
    stats = host_labels(T, Nmax, host_edges(T, data, result, 0, 0.0)[0])[1]
    inside = W.inside_tracks(label, edges)
    assert stats[2] > 0 and stats[0] > 0 and (~inside).sum() > 0 and inside.sum() > 0
    lab = label.reshape(-1)
    for (q, n, x, y), ins in zip(edges, inside):
        if not ins:
            assert lab[x] == -1 and lab[y] == -1  # without cuts an edge outside a track lies in a dropped component
            assert closed[q][n, 0] == 0.0 and auto[q][n, 0] == 0.0
    # the handcrafted conflict: no track at all, every gradient exactly 0
    data, result = _sparse_inputs(3, 70, CUT_GRAPH)
    edges, label, closed, auto = _both(3, data, result, 0.0)
    assert (label == -1).all() and len(edges) == 4 and not any(g.any() for g in closed + auto)


def test_rows_the_keep_rule_drops_get_exact_zeros():
    """A row at the threshold (the comparison is strict), rows below it, and matches that point at or behind the last keypoint of the
    second image."""
    T, thresh = 3, 0.6
    data, result, _, _ = planted_scene(41, T=T, n_kpts=40)
    m01 = result["matches0_0_1"][0].numpy()
    at = int(np.flatnonzero(m01 >= 0)[0])
    result["conf_scores_0_1"][0, at, 0] = float(np.float32(thresh))
    data["keypoints2"] = data["keypoints2"][:, :30].contiguous()  # matches >= 30 into image 2 are no edges
    edges, label, closed, auto = _both(T, data, result, np.float32(thresh))
    kept = {(q, n) for q, n, _, _ in edges}
    seen = {"at": 0, "below": 0, "behind": 0}
    for q, (i, j) in enumerate(_pairs(T)):
        m = result[f"matches{i}_{i}_{j}"][0].numpy()
        c = result[f"conf_scores_{i}_{j}"][0, :, 0].numpy()
        n_j = data[f"keypoints{j}"].shape[1]
        for n in range(len(m)):
            dropped = m[n] < 0 or m[n] >= n_j or not c[n] > np.float32(thresh)
            assert dropped == ((q, n) not in kept)
            if dropped:
                assert closed[q][n, 0] == 0.0 and auto[q][n, 0] == 0.0
                seen["at"] += int(m[n] >= 0 and c[n] == np.float32(thresh))
                seen["below"] += int(m[n] >= 0 and c[n] < np.float32(thresh))
                seen["behind"] += int(m[n] >= n_j and c[n] > np.float32(thresh))
    assert seen["at"] == 1 and seen["below"] > 3 and seen["behind"] > 3, seen
    assert any(g.any() for g in closed)


def test_the_second_channel_gets_exact_zeros():
    T, thresh = 3, 0.6
    data, result, _, _ = planted_scene(41, T=T, n_kpts=40)
    for i, j in _pairs(T):
        c = result[f"conf_scores_{i}_{j}"]
        result[f"conf_scores_{i}_{j}"] = torch.cat([c, c + 0.25], 2)
    edges, label, closed, auto = _both(T, data, result, thresh)
    for g in closed + auto:
        assert g.shape == (40, 2) and g[:, 0].any() and not g[:, 1].any()


def test_the_thinned_scene_holds_what_the_device_tests_use_it_for():
    """Seed and thinning of ``wrong_and_thinned_scene``, checked with the host union-find and the host repair: without repair tracks of
    2 .. 5 views beside dropped conflicts; after 4 rounds tracks of 2 .. 5 views, at least one cut edge inside its final track (it
    gets a gradient) and cut edges whose ends lie in two different tracks (they get exactly 0)."""
    T = 5
    data, result, _, _ = W.wrong_and_thinned_scene()
    edges, Nmax = W.kept_edges(T, data, result, 0, 0.0)
    label0, stats0 = host_labels(T, Nmax, host_edges(T, data, result, 0, 0.0)[0])
    eid, x, y, conf, _ = edge_arrays(T, data, result, 0, 0.0)
    label4, stats4, cuts, _ = host_repair(T, Nmax, eid, x, y, conf, 4)
    sizes = lambda lab: set(np.unique(lab[lab >= 0], return_counts=True)[1])  # noqa: E731
    assert sizes(label0) == {2, 3, 4, 5} and sizes(label4) == {2, 3, 4, 5} and stats0[2] == 4 and stats4[0] > stats0[0]
    cut = {int(c) for rnd in cuts for c in rnd}
    lab = label4.reshape(-1)
    inside = W.inside_tracks(label4, edges)
    is_cut = np.array([q * 24 + n in cut for q, n, _, _ in edges])
    between = np.array([lab[a] >= 0 and lab[b] >= 0 and lab[a] != lab[b] for _, _, a, b in edges])
    assert (is_cut & inside).sum() >= 1 and (is_cut & between).sum() >= 1 and not (between & ~is_cut).any()
    g_w = np.random.default_rng(3).normal(size=(len(W.track_observations(label4)), 2))
    closed = W.closed_form(label4, edges, W.confidences(T, result, 0), g_w)
    for (q, n, _, _), ins in zip(edges, inside):
        assert (closed[q][n, 0] != 0.0) == bool(ins)


# ---- the Python front: every error before any device call ------------------------------------------------------------------------------
def test_the_defaults_are_the_pair_route():
    from e2e_multi_view_matching_amd import multi_view
    sig = inspect.signature(multi_view.refine_tuple_poses_batch)
    assert list(sig.parameters) == ["tuple_size", "data", "result", "extrinsics", "conf_thresh", "max_iterations", "tracks", "repair_rounds"]
    assert sig.parameters["tracks"].default is False and sig.parameters["repair_rounds"].default == 0
    assert sig.parameters["conf_thresh"].default == 0.0 and sig.parameters["max_iterations"].default == 50


def test_track_arguments_are_checked_before_any_device_call(monkeypatch):
    from e2e_multi_view_matching_amd import multi_view
    _no_device(monkeypatch)
    start = np.tile(np.eye(4), (2, 3, 1, 1))
    data = {f"keypoints{t}": torch.zeros(2, 8, 2) for t in range(3)}
    result = {"matches0_0_1": torch.zeros(2, 8, dtype=torch.int64), "conf_scores_0_1": torch.ones(2, 8, 1)}
    with pytest.raises(ValueError, match="keypoints"):
        multi_view.refine_tuple_poses_batch(3, {}, result, start, tracks=True)
    with pytest.raises(ValueError, match="keypoints"):  # per-pair keypoints give a keypoint no identity across pairs
        multi_view.refine_tuple_poses_batch(3, {"keypoints0_0_1": torch.zeros(2, 8, 2)}, result, start, tracks=True)
    with pytest.raises(ValueError, match="tracks=True"):
        multi_view.refine_tuple_poses_batch(3, data, result, start, repair_rounds=2)
    for bad in (-1, 65, 2.5, "4", None, True):
        with pytest.raises(ValueError, match="repair_rounds"):
            multi_view.refine_tuple_poses_batch(3, data, result, start, tracks=True, repair_rounds=bad)
    for bad in (-1, 2.5, None):
        with pytest.raises(ValueError, match="max_iterations"):
            multi_view.refine_tuple_poses_batch(3, data, result, start, max_iterations=bad, tracks=True)
    with pytest.raises(ValueError, match="extrinsics"):
        multi_view.refine_tuple_poses_batch(3, data, result, start[:, :2], tracks=True, repair_rounds=4)
    with pytest.raises(AssertionError, match="a device call was made"):  # the premise: a valid call goes on to the device
        multi_view.refine_tuple_poses_batch(3, data, result, start, tracks=True, repair_rounds=4)


def test_the_header_declares_the_entry():
    from e2e_multi_view_matching_amd import _lib
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "e2emv.h")).read()
    assert "int e2emv_mv_tuple_ba_tracks_backward(e2emv_ctx* ctx, int B, int T, int N, int Nmax, const int32_t* d_label, const int32_t* stats," in header
    assert "const double* g_out_extr,\n                                      float* const* d_gconf, void* stream);" in header
    restype, argtypes = _lib.SIGNATURES["e2emv_mv_tuple_ba_tracks_backward"]
    forward = _lib.SIGNATURES["e2emv_mv_tuple_ba_tracks"][1]
    assert restype is _lib.c_int and len(argtypes) == len(forward) == 21 and argtypes[:18] == forward[:18]  # the forward's arguments, two gradients
