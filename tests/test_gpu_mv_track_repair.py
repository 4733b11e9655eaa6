"""GPU: the repair stage of the track merging (``multi_view.match_tracks(..., repair_rounds=R)``, ``e2emv_mv_tracks_repair``;
csrc/mvtracks.hip) against a vectorised numpy restatement of its rounds that lives in this file, on the inputs and with the host
builders of tests/test_gpu_mv_tracks.py.  The restatement's own final labelling is checked against that file's union-find
(``host_labels`` over the live edges) wherever the input is small."""
import numpy as np
import pytest
import torch

from test_gpu_mv_batch import _random_match_inputs, _slice
from test_gpu_mv_tracks import (_pairs, _perturbed_start, _random_inputs, _to, host_edges, host_labels, host_problem, planted_scene,
                                two_tuples)  # noqa: F401  (two_tuples is a fixture)

pytestmark = pytest.mark.gpu


# ---- the host restatement ------------------------------------------------------------------------------------------------
def edge_arrays(T, data, result, b, conf_thresh):
    """Kept edges of batch element ``b`` as arrays ``(eid, x, y, conf)`` in ascending edge id ``q * N + n`` (pair ``q`` in
    ``_pairs`` order, row ``n``), nodes ``t * Nmax + n``, ``conf`` float32 of channel 0; and ``Nmax``.  The same selection as
    ``host_edges`` (asserted)."""
    n_img = [data[f"keypoints{t}"].shape[1] for t in range(T)]
    Nmax = max(n_img)
    N = next(v.shape[1] for k, v in result.items() if k.startswith("matches"))
    eid, xs, ys, cs = [], [], [], []
    for q, (i, j) in enumerate(_pairs(T)):
        if f"matches{i}_{i}_{j}" not in result:
            continue
        m = result[f"matches{i}_{i}_{j}"][b].cpu().numpy()
        c = result[f"conf_scores_{i}_{j}"][b].cpu().numpy().astype(np.float32).reshape(len(m), -1)
        assert len(m) == N
        n = np.nonzero((m >= 0) & (m < n_img[j]) & (c > np.float32(conf_thresh)).all(1))[0]
        eid.append(q * N + n); xs.append(i * Nmax + n); ys.append(j * Nmax + m[n]); cs.append(c[n, 0])
    eid, x, y, conf = (np.concatenate(v) for v in (eid, xs, ys, cs))
    want, want_Nmax = host_edges(T, data, result, b, conf_thresh)
    assert want_Nmax == Nmax and want == {(int(a), int(bb)): c for a, bb, c in zip(x, y, conf)}
    return eid.astype(np.int64), x.astype(np.int64), y.astype(np.int64), conf.astype(np.float32), Nmax


def _components(nodes, x, y):
    """Smallest node id of every node's connected component: min-label hooking of nodes and roots + pointer jumping, to the fixed
    point."""
    lab = np.arange(nodes)
    while True:
        new = lab.copy()
        for a, bb in ((x, y), (y, x)):
            np.minimum.at(new, a, lab[bb])
            np.minimum.at(new, lab[a], lab[bb])
        while not np.array_equal(new[new], new):
            new = new[new]
        if np.array_equal(new, lab):
            return lab
        lab = new


def host_repair(T, Nmax, eid, x, y, conf, rounds):
    """The specification: ``(label [T, Nmax] int32, stats [4] int32, cut edge ids per round)``."""
    nodes = T * Nmax
    live = np.ones(len(eid), bool)
    image = np.arange(nodes) // Nmax
    cuts = []
    for rnd in range(rounds + 1):
        lab = _components(nodes, x[live], y[live])
        per_image = np.bincount(lab * T + image, minlength=nodes * T).reshape(nodes, T)  # row r: nodes of root r per image
        conflict, size = (per_image > 1).any(1), per_image.sum(1)
        if rnd == rounds or not conflict.any():
            break
        sel = np.nonzero(live & conflict[lab[x]])[0]
        order = sel[np.lexsort((eid[sel], conf[sel] + np.float32(0.0), lab[x[sel]]))]  # root, then confidence (-0.0 = 0.0), then id
        first = np.unique(lab[x[order]], return_index=True)[1]
        assert len(first) == conflict.sum()
        live[order[first]] = False
        cuts.append(eid[order[first]])
    valid = ~conflict & (size >= 2)
    label = np.where(valid[lab], lab, -1).astype(np.int32).reshape(T, Nmax)
    stats = np.array([valid.sum(), size[valid].sum(), conflict.sum(), live.sum()], np.int32)
    return label, stats, cuts, live


def _restated(T, data, result, b, conf_thresh, rounds, union_find=True):
    eid, x, y, conf, Nmax = edge_arrays(T, data, result, b, conf_thresh)
    label, stats, cuts, live = host_repair(T, Nmax, eid, x, y, conf, rounds)
    if union_find:  # the final labelling is the existing union-find over the live edges
        want, want_stats = host_labels(T, Nmax, {(int(a), int(bb)): c for a, bb, c in zip(x[live], y[live], conf[live])})
        assert np.array_equal(label, want) and np.array_equal(stats, want_stats)
    return label, stats, cuts, len(eid)


# ---- device calls ------------------------------------------------------------------------------------------------------------
def _device_tracks(T, data, result, conf_thresh, gpu, **kw):
    from e2e_multi_view_matching_amd import multi_view
    label, stats = multi_view.match_tracks(T, data, _to(result, gpu), conf_thresh, **kw)
    assert label.dtype == torch.int32 and stats.dtype == torch.int32 and label.device.type == "cuda"
    return label.cpu().numpy(), stats.cpu().numpy()


def _raw_repair(T, data, result, conf_thresh, rounds, gpu):
    """``e2emv_mv_tracks_repair`` itself, whatever ``rounds``."""
    from e2e_multi_view_matching_amd import _lib, multi_view
    inp = multi_view._track_inputs(T, data, _to(result, gpu))
    label = torch.full((inp["B"], T, inp["Nmax"]), -7, dtype=torch.int32, device=gpu)
    stats = torch.full((inp["B"], 4), -7, dtype=torch.int32, device=gpu)
    pm, pc = _lib.ptr_array(inp["matches"]), _lib.ptr_array(inp["conf"])
    with torch.cuda.device(gpu):
        _lib.context(gpu).call("e2emv_mv_tracks_repair", inp["B"], T, inp["N"], multi_view._p(inp["n1"]), pm[0], pc[0], inp["channels"],
                               float(conf_thresh), rounds, _lib.ptr(label), _lib.ptr(stats), _lib.stream_ptr(gpu))
    return label.cpu().numpy(), stats.cpu().numpy()


def _device_problems(T, data, result, conf_thresh, extr, gpu, repair_rounds):
    from e2e_multi_view_matching_amd import multi_view
    intr, kdim, nb = multi_view._tuple_intrinsics(T, data, gpu, len(extr))
    return multi_view._tuple_problems_tracks(T, data, _to(result, gpu), conf_thresh, intr, kdim, nb, extr, repair_rounds=repair_rounds)


def _solve_tracks(T, data, result, conf_thresh, start, gpu, repair_rounds):
    from e2e_multi_view_matching_amd import multi_view
    intr, kdim, nb = multi_view._tuple_intrinsics(T, data, gpu, len(start))
    out, summary = np.zeros((len(start), T, 4, 4)), np.zeros((len(start), 4))
    _, stats = multi_view._tracks_ba_call("e2emv_mv_tuple_ba_tracks", T, data, _to(result, gpu), conf_thresh, intr, kdim, nb, start, 50,
                                          multi_view._p(out), multi_view._p(summary), repair_rounds=repair_rounds)
    return out, summary, stats


def _sparse_inputs(T, N, edges, seed=5):
    """One tuple whose only matches are ``edges = [(i, j, n, m, confidence)]``: keypoint ``n`` of image ``i`` matches keypoint ``m``
    of image ``j``; every other row is -1 with confidence 0.5."""
    data, _ = _random_match_inputs(1, T, N, seed=seed)
    result = {}
    for i, j in _pairs(T):
        result[f"matches{i}_{i}_{j}"] = torch.full((1, N), -1, dtype=torch.int64)
        result[f"conf_scores_{i}_{j}"] = torch.full((1, N, 1), 0.5)
    for i, j, n, m, c in edges:
        result[f"matches{i}_{i}_{j}"][0, n] = m
        result[f"conf_scores_{i}_{j}"][0, n, 0] = c
    return data, result


def _expect(T, N, tracks):
    """Label array of one tuple from ``{label: [(image, keypoint), ...]}``."""
    label = np.full((T, N), -1, np.int32)
    for r, members in tracks.items():
        for t, n in members:
            label[t, n] = r
    return label


# ---- 1 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("conf_thresh", [0.0, 0.3])
def test_no_rounds_is_todays_call(gpu, conf_thresh):
    """``repair_rounds=0`` is ``match_tracks`` as it was, and ``e2emv_mv_tracks_repair`` with ``rounds = 0`` gives the labels and
    stats of ``e2emv_mv_tracks``, exactly."""
    B, T, N, data, result = _random_inputs()
    label, stats = _device_tracks(T, data, result, conf_thresh, gpu)
    zero = _device_tracks(T, data, result, conf_thresh, gpu, repair_rounds=0)
    raw = _raw_repair(T, data, result, conf_thresh, 0, gpu)
    assert (stats[:, 2] > 0).all()
    for got in (zero, raw):
        assert np.array_equal(got[0], label) and np.array_equal(got[1], stats)


# ---- 2 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("conf_thresh", [0.0, 0.3])
def test_random_matches_against_the_restatement(gpu, conf_thresh):
    """B = 3, T = 4, N = 70, the last image 50 keypoints, a pair at -1 and a pair absent; rounds 1, 3, 8: labels and stats equal
    the restatement, each element alone equals its slice of the batch, and run to run.  On the restatement's own output the
    tracks grow strictly with the rounds and edges are cut, so the inputs cannot stop exercising the path."""
    B, T, N, data, result = _random_inputs()
    tracks = np.zeros((B, 4), int)
    tracks[:, 0] = [_restated(T, data, result, b, conf_thresh, 0)[1][0] for b in range(B)]
    for k, rounds in enumerate((1, 3, 8), 1):
        label, stats = _device_tracks(T, data, result, conf_thresh, gpu, repair_rounds=rounds)
        assert label.shape == (B, T, N) and stats.shape == (B, 4)
        for b in range(B):
            want, want_stats, cuts, edges = _restated(T, data, result, b, conf_thresh, rounds)
            assert want_stats[3] < edges and edges - want_stats[3] == sum(len(c) for c in cuts)
            tracks[b, k] = want_stats[0]
            assert np.array_equal(label[b], want), (rounds, b, np.nonzero(label[b] != want))
            assert np.array_equal(stats[b], want_stats), (rounds, b, stats[b], want_stats)
            alone = _device_tracks(T, _slice(data, b), _slice(result, b), conf_thresh, gpu, repair_rounds=rounds)
            assert np.array_equal(alone[0][0], label[b]) and np.array_equal(alone[1][0], stats[b])
        again = _device_tracks(T, data, result, conf_thresh, gpu, repair_rounds=rounds)
        assert np.array_equal(again[0], label) and np.array_equal(again[1], stats)
    print("threshold", conf_thresh, "tracks per element after 0 / 1 / 3 / 8 rounds:", tracks.tolist())
    assert (np.diff(tracks, axis=1) > 0).all(), tracks
    if conf_thresh == 0.0:
        assert tracks[0].tolist() == [19, 24, 31, 45]


# ---- 3 -------------------------------------------------------------------------------------------------------------------------
def test_a_star_needs_one_round_per_cut(gpu):
    """T = 2: keypoints 0 .. 3 of image 0 all match keypoint 0 of image 1 (0.9, 0.1, 0.2, 0.3).  One cut per component per round:
    after 2 rounds two edges are left and conflict; the third round leaves the 0.9 edge, and further rounds change nothing."""
    T, N = 2, 70
    data, result = _sparse_inputs(T, N, [(0, 1, n, 0, c) for n, c in enumerate((0.9, 0.1, 0.2, 0.3))])
    label, stats = _device_tracks(T, data, result, 0.0, gpu, repair_rounds=2)
    assert (label == -1).all() and stats[0].tolist() == [0, 0, 1, 2]
    for rounds in (3, 64):
        label, stats = _device_tracks(T, data, result, 0.0, gpu, repair_rounds=rounds)
        assert np.array_equal(label[0], _expect(T, N, {0: [(0, 0), (1, 0)]})) and stats[0].tolist() == [1, 2, 0, 1], (rounds, stats)
        assert np.array_equal(label[0], _restated(T, data, result, 0, 0.0, rounds)[0])


# ---- 4 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weak,conf_thresh", [((0.2, 0.2), 0.0), ((0.0, -0.0), -1.0)])
def test_ties_go_to_the_smaller_edge_id(gpu, weak, conf_thresh):
    """T = 3: the path (0,5) - (1,0) - (2,0) - (0,1) holds two keypoints of image 0.  Its end edges tie: (0,5) - (1,0) is row 5 of
    pair 0 (id 5), (0,1) - (2,0) is row 1 of pair 1 (id N + 1).  The smaller id is cut although its row is the larger one: the track
    is {(0,1), (1,0), (2,0)} with label 1; cutting the other edge would give label 5.  Second variant: +0.0 on the smaller id and
    -0.0 on the larger one tie as well (an order on the bit patterns would cut the -0.0 edge)."""
    T, N = 3, 70
    data, result = _sparse_inputs(T, N, [(0, 1, 5, 0, weak[0]), (1, 2, 0, 0, 0.9), (0, 2, 1, 0, weak[1])])
    if conf_thresh < 0:
        assert np.signbit(result["conf_scores_0_2"][0, 1, 0].numpy()) and not np.signbit(result["conf_scores_0_1"][0, 5, 0].numpy())
    assert _device_tracks(T, data, result, conf_thresh, gpu)[1][0].tolist() == [0, 0, 1, 3]
    label, stats = _device_tracks(T, data, result, conf_thresh, gpu, repair_rounds=1)
    want = _expect(T, N, {1: [(0, 1), (1, 0), (2, 0)]})
    assert np.array_equal(label[0], want), np.nonzero(label[0] >= 0)
    assert stats[0].tolist() == [1, 3, 0, 2]
    assert np.array_equal(_restated(T, data, result, 0, conf_thresh, 1)[0], want)


# ---- 5 -------------------------------------------------------------------------------------------------------------------------
def test_negative_confidences_order_as_floats(gpu):
    """``conf_thresh = -1``.  Star A: (0,0) - (1,0) at 0.25 and (0,1) - (1,0) at -0.5 loses the -0.5 edge (an unsigned order on the
    bits would cut 0.25).  Star B: (0,10) - (1,5) at -0.25 and (0,11) - (1,5) at -0.5 loses the -0.5 edge (a signed-integer order
    on the bits would cut -0.25).  In both the weaker edge has the larger id, so the tie rule cannot produce the result."""
    T, N = 2, 70
    data, result = _sparse_inputs(T, N, [(0, 1, 0, 0, 0.25), (0, 1, 1, 0, -0.5), (0, 1, 10, 5, -0.25), (0, 1, 11, 5, -0.5)])
    assert _device_tracks(T, data, result, -1.0, gpu)[1][0].tolist() == [0, 0, 2, 4]
    label, stats = _device_tracks(T, data, result, -1.0, gpu, repair_rounds=1)
    want = _expect(T, N, {0: [(0, 0), (1, 0)], 10: [(0, 10), (1, 5)]})
    assert np.array_equal(label[0], want), np.nonzero(label[0] >= 0)
    assert stats[0].tolist() == [2, 4, 0, 2]
    assert np.array_equal(_restated(T, data, result, 0, -1.0, 1)[0], want)


# ---- 6 -------------------------------------------------------------------------------------------------------------------------
def test_a_cut_edge_inside_its_final_track_still_weighs(gpu):
    """T = 3: the triangle (0,0) - (1,0) at 0.9, (1,0) - (2,0) at 0.8, (0,0) - (2,0) at 0.1 and (0,1) - (1,0) at 0.5.  Round 1 cuts
    the 0.1 edge (the component still conflicts), round 2 the 0.5 edge: the track {(0,0), (1,0), (2,0)}.  The problem is built on
    the ORIGINAL edges between members, so the cut 0.1 edge still counts: confidences 0.5, 0.85, 0.45 before normalisation.
    Against ``host_problem`` fed the repaired labels and the original edge dict: indices and observations exactly, weights
    within the 1e-12 relative of ``_check_problem`` (fp64 means of two fp32 values, a sum of three)."""
    T, N = 3, 70
    data, result = _sparse_inputs(T, N, [(0, 1, 0, 0, 0.9), (1, 2, 0, 0, 0.8), (0, 2, 0, 0, 0.1), (0, 1, 1, 0, 0.5)])
    want = _expect(T, N, {0: [(0, 0), (1, 0), (2, 0)]})
    label1, stats1 = _device_tracks(T, data, result, 0.0, gpu, repair_rounds=1)
    assert (label1 == -1).all() and stats1[0].tolist() == [0, 0, 1, 3]
    extr = _perturbed_start(np.tile(np.eye(4), (T, 1, 1)), np.random.default_rng(0), rot=0.2, tr=0.5)[None]
    (prob,), label, stats = _device_problems(T, data, result, 0.0, extr, gpu, repair_rounds=2)
    label = label.cpu().numpy()
    assert np.array_equal(label[0], want) and stats[0].tolist() == [1, 3, 0, 2]
    assert np.array_equal(_restated(T, data, result, 0, 0.0, 2)[0], want)
    edges, _ = host_edges(T, data, result, 0, 0.0)
    assert len(edges) == 4
    cam_idx, pt_idx, obs, wts, _ = host_problem(T, data, 0, want, edges, extr[0], svd_points=False)
    n_cams, fixed, intr4, d_cam, d_pt, d_obs, d_w, d_cams, d_pts = prob
    assert np.array_equal(d_cam, cam_idx) and d_cam.tolist() == [0, 1, 2] and np.array_equal(d_pt, pt_idx) and len(d_pts) == 1
    assert np.array_equal(d_obs, obs) and np.array_equal(d_w[:, 0], d_w[:, 1])
    f = lambda v: float(np.float32(v))  # noqa: E731
    conf = np.array([(f(0.9) + f(0.1)) / 2, (f(0.9) + f(0.8)) / 2, (f(0.1) + f(0.8)) / 2])
    assert np.abs(conf - [0.5, 0.85, 0.45]).max() < 1e-7
    print("weights before normalisation:", (d_w[:, 0] * 0.5 * (conf.sum() + 1e-3)).tolist(), "relative difference to the host builder",
          (np.abs(d_w - wts) / wts).max())
    assert (np.abs(d_w - wts) <= 1e-12 * np.abs(wts)).all()
    assert (np.abs(d_w[:, 0] * 0.5 * (conf.sum() + 1e-3) - conf) <= 1e-12 * conf).all()


# ---- 7 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rounds", [1, 5])
def test_zigzag_splits_by_edge_id_alone(gpu, rounds):
    """The input of ``test_zigzag_through_three_images``: one component through all 210 nodes (wider than a wave), every confidence
    0.5, so every cut is decided by the edge id.  The smallest live id is always a row of pair (0, 1) (the restatement: ids 0, 1, 2, 3, 4):
    round 1 frees node (0,0), every later round splits a track of 3 views off the front of the path, whose rest stays one
    conflict - 4 tracks after 5 rounds; many conflicting
    components in ONE round are the node-limit and planted-scene tests (185 and 24 cuts in their first rounds)."""
    T, N = 3, 70
    data, _ = _random_match_inputs(1, T, N, seed=1)
    n = np.arange(N)
    result = {"matches0_0_1": n.copy(), "matches0_0_2": np.where(n >= 1, n - 1, -1), "matches1_1_2": n.copy()}
    result = {k: torch.from_numpy(v.astype(np.int64)[None]) for k, v in result.items()}
    for i, j in _pairs(T):
        result[f"conf_scores_{i}_{j}"] = torch.full((1, N, 1), 0.5)
    want, want_stats, cuts, edges = _restated(T, data, result, 0, 0.0, rounds)
    assert edges == 3 * N - 1 and len(cuts) == rounds and [c.tolist() for c in cuts] == [[k] for k in range(rounds)]
    assert want_stats.tolist() == ([0, 0, 1, 208] if rounds == 1 else [4, 12, 1, 204])
    label, stats = _device_tracks(T, data, result, 0.0, gpu, repair_rounds=rounds)
    assert np.array_equal(label[0], want), np.nonzero(label[0] != want)
    assert np.array_equal(stats[0], want_stats), (stats[0], want_stats)


# ---- 8 -------------------------------------------------------------------------------------------------------------------------
def test_the_node_limit(gpu):
    """The input of ``test_the_node_limit`` of the label tests (T = 8 images of 2048 keypoints = 16384 nodes, threshold 0.1) with
    2 rounds against the restatement; more tracks than without repair; one keypoint more is ``E2EMV_ESHAPE`` before any launch;
    65 and -1 rounds are ``E2EMV_EINVAL``."""
    from e2e_multi_view_matching_amd import _lib
    T, N = 8, 2048
    rng = np.random.default_rng(6)
    data = {f"keypoints{t}": torch.zeros(1, N, 2) for t in range(T)}
    result = {}
    for i, j in _pairs(T):
        m = rng.integers(0, N, N)
        m[rng.uniform(size=N) < 0.93] = -1
        result[f"matches{i}_{i}_{j}"] = torch.from_numpy(m[None])
        result[f"conf_scores_{i}_{j}"] = torch.from_numpy(rng.uniform(0, 1, (1, N, 1)).astype(np.float32))
    want, want_stats, cuts, edges = _restated(T, data, result, 0, 0.1, 2, union_find=False)
    before = _restated(T, data, result, 0, 0.1, 0, union_find=False)[1]
    print("16384 nodes: stats without repair", before, "after 2 rounds", want_stats, "cuts per round", [len(c) for c in cuts])
    assert before[2] > 100 and want_stats[0] > before[0] and len(cuts) == 2 and len(cuts[0]) == before[2] and len(cuts[1]) > 0
    label, stats = _device_tracks(T, data, result, 0.1, gpu, repair_rounds=2)
    assert label.shape == (1, T, N) and np.array_equal(label[0], want) and np.array_equal(stats[0], want_stats), (stats[0], want_stats)
    for rounds in (65, -1):
        with pytest.raises(_lib.E2EMVError) as err:
            _raw_repair(T, data, result, 0.1, rounds, gpu)
        assert err.value.code == _lib.EINVAL
    data[f"keypoints{T - 1}"] = torch.zeros(1, N + 1, 2)
    with pytest.raises(_lib.E2EMVError) as err:
        _device_tracks(T, data, result, 0.1, gpu, repair_rounds=2)
    assert err.value.code == _lib.ESHAPE and "16384" in str(err.value)


# ---- 9 -------------------------------------------------------------------------------------------------------------------------
def test_problem_build_on_repaired_labels(gpu):
    """The random inputs with 3 rounds through ``_tuple_problems_tracks`` against ``host_problem`` on the restatement's labels and
    the original edges, as ``_check_problem`` with ``points=False``: indices, counts and observations exactly, weights within its
    1e-12 relative bar; each element alone builds the same bits."""
    B, T, N, data, result = _random_inputs()
    extr = np.stack([_perturbed_start(np.tile(np.eye(4), (T, 1, 1)), np.random.default_rng(b), rot=0.2, tr=0.5) for b in range(B)])
    problems, label, stats = _device_problems(T, data, result, 0.0, extr, gpu, repair_rounds=3)
    label = label.cpu().numpy()
    for b, prob in enumerate(problems):
        want_label, want_stats, _, _ = _restated(T, data, result, b, 0.0, 3)
        assert np.array_equal(label[b], want_label) and np.array_equal(stats[b], want_stats)
        edges, _ = host_edges(T, data, result, b, 0.0)
        cam_idx, pt_idx, obs, wts, _ = host_problem(T, data, b, want_label, edges, extr[b], svd_points=False)
        n_cams, fixed, intr4, d_cam, d_pt, d_obs, d_w, d_cams, d_pts = prob
        assert (n_cams, fixed, list(intr4)) == (T, 0, [1.0, 1.0, 0.0, 0.0])
        assert len(d_pts) == want_stats[0] > 0 and len(d_cam) == want_stats[1] == len(cam_idx)
        assert np.array_equal(d_cam, cam_idx) and np.array_equal(d_pt, pt_idx) and np.array_equal(d_obs, obs)
        assert np.array_equal(d_w[:, 0], d_w[:, 1])
        print("tuple", b, ":", want_stats, "weights: max relative difference", (np.abs(d_w - wts) / wts).max())
        assert (np.abs(d_w - wts) <= 1e-12 * np.abs(wts)).all() and abs(d_w[:, 0].sum() - 2.0) < 1e-3
        assert np.abs(d_cams[:, 3:] - extr[b][:, :3, 3]).max() == 0.0
        alone = _device_problems(T, _slice(data, b), _slice(result, b), 0.0, extr[b:b + 1], gpu, repair_rounds=3)[0][0]
        for u, v in zip(alone[3:], prob[3:]):
            assert np.array_equal(u, v, equal_nan=True)


# ---- 10 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,want4", [(21, [82, 410, 5, 1739]), (22, [100, 500, 3, 1726])])
def test_planted_scenes_with_wrong_matches(gpu, seed, want4):
    """The planted 5-tuples with 10 % wrong matches, 4 rounds: labels and stats equal the restatement (its stats are the values an
    fp64 numpy run of the rule gave); at least twice the tracks of 0 rounds; the solved track problem has every pair's pose error
    below 2.0 degrees, the bar of the label tests' planted scenes (``oracle.mvba.solve`` on the numpy-built problems: 0.90 and
    0.70).  Measured on an MI355X, tracks / conflicts left / max pose error (degrees) after 0, 1, 4, 8 rounds: seed 21: 35 / 24 /
    1.760, 59 / 11 / 0.785, 82 / 5 / 0.896, 96 / 2 / 0.533; seed 22: 39 / 31 / 0.791, 69 / 15 / 0.718, 100 / 3 / 0.700, 110 / 2 /
    0.641 - the figures of the fp64 host run."""
    from e2e_multi_view_matching_amd import multi_view
    T = 5
    data, result, gt, start = planted_scene(seed, wrong=0.1)
    want, want_stats, _, _ = _restated(T, data, result, 0, 0.0, 4)
    assert want_stats.tolist() == want4
    label, stats = _device_tracks(T, data, result, 0.0, gpu, repair_rounds=4)
    assert np.array_equal(label[0], want) and np.array_equal(stats[0], want_stats), (stats[0], want_stats)
    figures = {}
    for rounds in (0, 1, 4, 8):
        out, summary, st = _solve_tracks(T, data, result, 0.0, start[None], gpu, rounds)
        err_t, err_R = multi_view.tuple_pose_errors(out[0], np.linalg.inv(gt))
        figures[rounds] = (st[0].tolist(), max(err_t.max(), err_R.max()))
        print("seed", seed, "rounds", rounds, "stats", st[0].tolist(), "iterations", int(summary[0, 2]), "max pose error", figures[rounds][1],
              "mean", np.maximum(err_t, err_R).mean())
    assert figures[4][0] == want4 and figures[4][0][0] >= 2 * figures[0][0][0], figures
    assert figures[4][1] < 2.0, figures


# ---- 11 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("init", ["host", "device"])
def test_whole_path_with_repair(gpu, two_tuples, init):  # noqa: F811
    """``solve_tuple_poses_batch(5, ..., tracks=True, repair_rounds=4)``: finite [2, 5, 4, 4]; the batch is each element alone, bit
    for bit, and equal run to run; pose errors through ``eval_bundle_adjust_batch`` at the bars of the existing whole-path tests
    (max below 2.0 degrees, AUC@5 above 0.8), the figures of ``repair_rounds=0`` printed beside them."""
    from e2e_multi_view_matching_amd import multi_view, pose_auc
    dev, result = two_tuples
    whole = multi_view.solve_tuple_poses_batch(5, dev, result, init=init, tracks=True, repair_rounds=4)
    assert whole.shape == (2, 5, 4, 4) and whole.dtype == np.float64 and np.isfinite(whole).all()
    assert np.array_equal(whole, multi_view.solve_tuple_poses_batch(5, dev, result, init=init, tracks=True, repair_rounds=4))
    for b in range(2):
        alone = multi_view.solve_tuple_poses_batch(5, _slice(dev, b), _slice(result, b), init=init, tracks=True, repair_rounds=4)
        assert np.array_equal(alone[0], whole[b]), (b, np.abs(alone[0] - whole[b]).max())
    figures = {}
    for rounds in (0, 4):
        e = np.array(multi_view.eval_bundle_adjust_batch(5, dev, result, [[], [], []], init=init, tracks=True, repair_rounds=rounds)[0])
        figures[rounds] = (e, pose_auc(e, [5, 10, 20]))
        stats = multi_view.match_tracks(5, dev, result, repair_rounds=rounds)[1].cpu().numpy()
        print("init", init, "repair_rounds", rounds, "stats", stats.tolist(), "pose errors (degrees): max", e.max(), "mean", e.mean(), "auc", figures[rounds][1])
    e, auc = figures[4]
    assert len(e) == 2 * 10 and e.max() < 2.0 and auc[0] > 0.8, (e, auc)
