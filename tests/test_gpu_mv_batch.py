"""GPU: the multi-view pose back-end for a whole batch of tuples, in memory (multi_view.bundle_adjust_batch,
solve_tuple_poses_batch, eval_bundle_adjust_batch): every stage against the single-problem / CSV code it was derived from."""
import os

import numpy as np
import pytest
import torch

from test_mv_ba import _random_problem

pytestmark = pytest.mark.gpu

T5_CFG = {"GNN_layers": ["self", "cross"] * 2, "sinkhorn_iterations": 50, "multi_frame_matching": True, "tuple_size": 5}


def _args(prob):
    return (prob["n_cams"], prob["fixed"], prob["intr"], prob["cam_idx"], prob["pt_idx"], prob["obs"], prob["wts"], prob["cams"], prob["pts"])


def _ba_problems():
    probs = [_random_problem(10, 5, 600, views_per_point=2)[0], _random_problem(11, 3, 50, views_per_point=2)[0],
             _random_problem(12, 8, 1500, views_per_point=3)[0], _random_problem(13, 2, 5, views_per_point=2)[0]]
    empty = dict(n_cams=3, fixed=0, intr=np.array([1.0, 1.0, 0.0, 0.0]), cam_idx=np.zeros(0, np.int32), pt_idx=np.zeros(0, np.int32),
                 obs=np.zeros((0, 2)), wts=np.zeros((0, 2)), cams=np.random.default_rng(0).normal(0, 0.1, (3, 6)), pts=np.zeros((0, 3)))
    blind = dict(_random_problem(14, 3, 200, views_per_point=2)[0])  # a fourth camera that sees nothing
    blind["n_cams"] = 4
    blind["cams"] = np.concatenate([blind["cams"], [[0.1, -0.2, 0.05, 0.3, 0.2, -0.1]]])
    return probs + [empty, blind]


def test_batched_bundle_adjustment_is_the_single_one_bit_for_bit(gpu):
    """One launch over six problems of different sizes (one without points, one whose last camera has no observation) =
    ``bundle_adjust`` one at a time, in either order of the list; the first also against the oracle at the bars of
    ``test_gpu_solver_matches_oracle``."""
    from e2e_multi_view_matching_amd import multi_view
    from oracle import mvba
    probs = _ba_problems()
    single = [multi_view.bundle_adjust(*_args(p)) for p in probs]
    batch = multi_view.bundle_adjust_batch([_args(p) for p in probs])
    rev = multi_view.bundle_adjust_batch([_args(p) for p in reversed(probs)])[::-1]
    assert len(batch) == len(rev) == len(probs)
    for k, (one, many, back) in enumerate(zip(single, batch, rev)):
        for other in (many, back):
            assert np.array_equal(one[0], other[0]) and np.array_equal(one[1], other[1]), k
            assert one[2] == other[2], (k, one[2], other[2])
        assert one[0].shape == probs[k]["cams"].shape and one[1].shape == probs[k]["pts"].shape
    assert batch[4][2]["initial_cost"] == 0.0 and np.array_equal(batch[4][0], probs[4]["cams"])  # nothing to optimise
    assert np.array_equal(batch[5][0][3], probs[5]["cams"][3])  # the blind camera keeps its parameters
    assert batch[0][2]["final_cost"] < 0.05 * batch[0][2]["initial_cost"]
    oc, op, osum = mvba.solve(probs[0])
    gc, gp, gsum = batch[0]
    assert gsum["iterations"] == osum["iterations"] and gsum["termination"] == osum["termination"], (gsum, osum)
    assert abs(gsum["initial_cost"] - osum["initial_cost"]) <= 1e-10 * osum["initial_cost"]
    assert abs(gsum["final_cost"] - osum["final_cost"]) <= 1e-8 * osum["final_cost"]
    assert np.abs(gc - oc).max() < 1e-7 and np.abs(gp - op).max() < 1e-6


def test_batched_bundle_adjustment_validates_its_arguments(gpu):
    import ctypes
    from e2e_multi_view_matching_amd import _lib
    ctx = _lib.context(gpu)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    intr, cams, pts = np.array([1.0, 1, 0, 0] * 2), np.zeros((4, 6)), np.zeros((3, 3))
    ci, pi, obs, w = np.zeros(4, np.int32), np.zeros(4, np.int32), np.zeros((4, 2)), np.ones((4, 2))
    fixed = np.zeros(2, np.int32)

    def call(n_cams, pt_off, obs_off, cam_idx=ci):
        return ctx.lib.e2emv_mv_bundle_adjust_batch(ctx.h, 2, p(np.array(n_cams, np.int32)), p(fixed), p(intr), p(np.array(pt_off, np.int64)),
                                                   p(np.array(obs_off, np.int64)), p(cam_idx), p(pi), p(obs), p(w), p(cams), p(pts), 5, None, None)

    assert call([2, 2], [0, 2, 1], [0, 2, 4]) == _lib.ESHAPE and b"monotone" in ctx.lib.e2emv_last_error(ctx.h)
    assert call([2, 2], [1, 2, 3], [0, 2, 4]) == _lib.ESHAPE
    assert call([2, 9], [0, 2, 3], [0, 2, 4]) == _lib.EINVAL and b"cameras" in ctx.lib.e2emv_last_error(ctx.h)
    assert call([2, 2], [0, 2, 3], [0, 2, 4], np.array([0, 1, 2, 0], np.int32)) == _lib.EINVAL  # camera 2 of a 2-camera problem


def _random_match_inputs(B, T, N, seed):
    rng = np.random.default_rng(seed)
    data, result = {}, {}
    for v in range(T):
        data[f"keypoints{v}"] = torch.from_numpy(rng.uniform(0, 640, (B, N, 2)).astype(np.float32))
        K = np.tile(np.eye(4, dtype=np.float32), (B, 1, 1))
        K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2] = 600 + 10 * v, 590 + 10 * v, 320 + v, 240 - v
        data[f"intr{v}"] = torch.from_numpy(K)
    for j in range(T):
        for i in range(j):
            m = rng.integers(0, N, (B, N))
            m[rng.uniform(size=(B, N)) < 0.4] = -1
            result[f"matches{i}_{i}_{j}"] = torch.from_numpy(m.astype(np.int64))
            result[f"conf_scores_{i}_{j}"] = torch.from_numpy(rng.uniform(0, 1, (B, N, 1)).astype(np.float32))
    return data, result


@pytest.mark.parametrize("conf_thresh", [0.0, 0.3])
def test_collect_is_the_host_selection(gpu, conf_thresh):
    """``e2emv_mv_collect`` = ``_collect_matches`` on every sliced batch element: counts, and the kept keypoints / matched
    keypoints / confidences in ascending keypoint order (selection only, so exactly)."""
    from e2e_multi_view_matching_amd import multi_view
    B, T, N = 3, 3, 300
    data, result = _random_match_inputs(B, T, N, seed=5)
    result["matches0_0_2"][1] = -1  # a pair without any match inside the batch
    dev_result = {k: v.to(gpu) for k, v in result.items()}
    o0, o1, oc, count = (t.cpu().numpy() for t in multi_view._collect_matches_batch(T, data, dev_result, conf_thresh))
    pairs = multi_view._pairs(T)
    assert o0.shape == o1.shape == (B * len(pairs), N, 2) and oc.shape == (B * len(pairs), N) and count.dtype == np.int32
    for b in range(B):
        pw = multi_view._collect_matches(T, {k: v[b:b + 1] for k, v in data.items()}, {k: v[b:b + 1] for k, v in result.items()}, conf_thresh)
        for q, (i, j) in enumerate(pairs):
            r, want0, want1, wantc = b * len(pairs) + q, pw[f"mkpts{i}_{i}_{j}"], pw[f"mkpts{j}_{i}_{j}"], pw[f"conf{i}_{i}_{j}"]
            n = count[r]
            assert n == len(want0), (b, q, n, len(want0))
            assert np.array_equal(o0[r, :n], want0) and np.array_equal(o1[r, :n], want1) and np.array_equal(oc[r, :n], wantc[:, 0])
            assert not o0[r, n:].any() and not o1[r, n:].any() and not oc[r, n:].any()
    assert count[1 * len(pairs) + 1] == 0 and 0 < count.max() < N
    # a pair whose matches are missing altogether is a problem with count 0
    del dev_result["matches0_0_1"]
    count2 = multi_view._collect_matches_batch(T, data, dev_result, conf_thresh)[3].cpu().numpy()
    assert (count2[0::3] == 0).all() and np.array_equal(count2.reshape(B, 3)[:, 1:], count.reshape(B, 3)[:, 1:])


def test_problem_build_against_the_csv_writer(gpu, tmp_path):
    """The golden 4-tuple (set up as in ``test_host_logic_matches_reference_bundle_adjust_io``), extrinsics from the fixture:
    what ``e2emv_mv_tuple_problem`` builds on the device against the rows ``write_bundle_adjust_problem`` writes.  Indices
    and counts equal; observations equal exactly; weights within relative 1e-6 (fp64 sum here, numpy's fp32 there); points
    within 1e-5 * max(1, |X|)."""
    from e2e_multi_view_matching_amd import multi_view
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "multi_view_io_reference.npz"))
    T = 4
    data = {k: torch.from_numpy(g[k]) for k in g.files if k.startswith(("keypoints", "intr"))}
    result = {k: torch.from_numpy(g[k]).to(gpu) for k in g.files if k.startswith(("matches", "conf_scores"))}
    pw = multi_view.initialize_bundle_adjust(T, data, result, str(tmp_path / "ba_init_in.csv"))
    multi_view.write_bundle_adjust_problem(T, pw, g["extrinsics"], str(tmp_path / "ba_in.csv"))
    rows = [[float(x) for x in line.split(",")] for line in open(tmp_path / "ba_in.csv")]
    header, obs_rows, pt_rows = rows[0], np.array([r for r in rows if len(r) == 5]), np.array([r for r in rows if len(r) == 3])

    collected = multi_view._collect_matches_batch(T, data, result, 0.)
    counts = collected[3].cpu().numpy()
    intr, kdim, nb = multi_view._tuple_intrinsics(T, data, gpu, 1)
    (n_cams, fixed, intr4, cam_idx, pt_idx, obs_xy, obs_w, cams, pts), = multi_view._tuple_problems(T, collected, counts, intr, kdim, nb,
                                                                                                      g["extrinsics"][None])
    assert [n_cams, fixed, len(pts), len(cam_idx)] == [int(v) for v in header[:4]] and list(intr4) == header[4:]
    assert counts.sum() == len(pts) and len(obs_rows) == 2 * len(pts) == len(pt_rows) * 2
    assert np.array_equal(cam_idx, obs_rows[:, 0]) and np.array_equal(pt_idx, obs_rows[:, 1])
    # the same fp32 numbers: str(float32) round-trips to the float32 it was printed from (the text, read as fp64, is the shortest
    # decimal of that float32, not its exact value), and the arithmetic is the same two correctly rounded operations
    assert np.array_equal(obs_xy, obs_xy.astype(np.float32).astype(np.float64))
    assert np.array_equal(obs_xy.astype(np.float32), obs_rows[:, 2:4].astype(np.float32))
    assert np.array_equal(obs_w[:, 0], obs_w[:, 1])
    w_err = np.abs(obs_w[:, 0] - obs_rows[:, 4]) / np.maximum(1, np.abs(obs_rows[:, 4]))
    p_err = np.abs(pts - pt_rows).max(1) / np.maximum(1.0, np.abs(pt_rows).max(1))
    print("weights: max relative difference", w_err.max(), " points: max difference / max(1, |X|)", p_err.max())
    assert w_err.max() < 1e-6 and p_err.max() < 1e-5
    assert abs(obs_w[:, 0].sum() - 2.0) < 1e-3  # normalised to sum 2 over all observations
    # the start cameras are the fixture's extrinsics as angle-axis + translation
    assert np.abs(cams[:, 3:] - g["extrinsics"][:, :3, 3]).max() == 0.0


def _five_tuple_inputs(gpu, seeds, n_kpts, unmatched_first=False):
    """Tuples as in ``test_five_tuple_back_end`` / ``test_five_tuple_with_an_unmatched_image``, concatenated along the batch."""
    from e2e_multi_view_matching_amd import MultiViewMatcher
    from e2e_multi_view_matching_amd.synthetic import identity_like_state, make_tuples
    T = 5
    model = identity_like_state(MultiViewMatcher(T5_CFG).eval()).to(gpu)
    parts = [make_tuples(batch=1, tuple_size=T, n_kpts=n_kpts, seed=s, noise_px=0.5, max_angle=0.25, transl_sigma=0.4) for s in seeds]
    if unmatched_first:
        gen = torch.Generator().manual_seed(5)
        parts[0]["descriptors4"] = torch.nn.functional.normalize(torch.randn(1, 256, n_kpts, generator=gen), dim=1)  # unrelated content
    data = {k: (torch.cat([p[k] for p in parts], 0) if torch.is_tensor(v) else v) for k, v in parts[0].items()}
    dev = {k: (v.to(gpu) if torch.is_tensor(v) else v) for k, v in data.items()}
    for m in range(T):  # the reference's pose{m} are camera -> world
        dev[f"pose{m}"] = torch.linalg.inv(data[f"pose{m}"])
        dev[f"intr{m}"] = data[f"intr{m}"]
    with torch.no_grad():
        result = model(dev)
    return dev, result


def _slice(d, b):
    return {k: (v[b:b + 1] if torch.is_tensor(v) else v) for k, v in d.items()}


@pytest.fixture(scope="module")
def three_tuples(gpu):
    return _five_tuple_inputs(gpu, seeds=(20, 21, 22), n_kpts=512)


def test_whole_path_does_not_depend_on_the_batch(gpu, three_tuples):
    """``solve_tuple_poses_batch`` on the B = 3 matcher result = itself on each element's slice of that result, bit for bit."""
    from e2e_multi_view_matching_amd import multi_view
    dev, result = three_tuples
    whole = multi_view.solve_tuple_poses_batch(5, dev, result)
    assert whole.shape == (3, 5, 4, 4) and whole.dtype == np.float64 and np.isfinite(whole).all()
    for b in range(3):
        alone = multi_view.solve_tuple_poses_batch(5, _slice(dev, b), _slice(result, b))
        assert np.array_equal(alone[0], whole[b]), (b, np.abs(alone[0] - whole[b]).max())
    assert np.array_equal(whole, multi_view.solve_tuple_poses_batch(5, dev, result))  # and run to run


# max |E_batch - E_csv| over the three tuples as measured on an MI355X (3.4e-8, 3.7e-8, 1.9e-8; DESIGN.md section 1: the CSV
# path writes its fp32 observations as shortest decimals, half an fp32 ulp away from the numbers the batched path keeps); the
# bar is ten times it
MEASURED_BATCH_VS_CSV = 3.7e-8


def test_whole_path_against_the_csv_path(gpu, three_tuples, tmp_path):
    """The batched extrinsics against ``solve_tuple_poses`` per element (text rounds at 12 digits on the CSV path and the weight
    sums differ in their last bits; the LM iteration amplifies that); the pose errors against ground truth at the bars of
    ``test_five_tuple_back_end``; ``eval_bundle_adjust_batch`` on a B = 1 slice appends what ``eval_bundle_adjust`` appends."""
    from e2e_multi_view_matching_amd import multi_view, pose_auc
    dev, result = three_tuples
    whole = multi_view.solve_tuple_poses_batch(5, dev, result)
    diffs = []
    for b in range(3):
        csv = multi_view.solve_tuple_poses(5, _slice(dev, b), _slice(result, b), str(tmp_path / f"t{b}"))
        diffs.append(np.abs(whole[b] - csv).max())
    print("max |E_batch - E_csv| per tuple:", diffs)
    assert max(diffs) <= 10 * MEASURED_BATCH_VS_CSV, diffs
    errs = multi_view.eval_bundle_adjust_batch(5, dev, result, [[], [], []])
    e = np.array(errs[0])
    assert len(e) == 3 * 10 and len(errs[1]) == len(errs[2]) == 30
    auc = pose_auc(e, [5, 10, 20])
    print("pose errors (degrees): max", e.max(), "auc", auc)
    assert e.max() < 2.0 and auc[0] > 0.8, (e, auc)
    one = multi_view.eval_bundle_adjust_batch(5, _slice(dev, 1), _slice(result, 1), [[], [], []])
    ref = multi_view.eval_bundle_adjust(5, _slice(dev, 1), _slice(result, 1), str(tmp_path / "ref"), [[], [], []])
    assert [len(x) for x in one] == [len(x) for x in ref] == [10, 10, 10]
    assert np.array_equal(np.array(one[0]), e[10:20])  # batch element outer, pairs inside
    # the same entries in the same order: extrinsics that agree to the bar above give angles that agree to bar / sin(angle),
    # 1e-3 degrees down to errors of 1e-4 degrees
    assert np.abs(np.array(one) - np.array(ref)).max() < 1e-3


def test_a_degenerate_tuple_inside_a_batch(gpu):
    """Element 0: the input of ``test_five_tuple_with_an_unmatched_image`` (image 4 shares nothing with the others), element 1
    an ordinary tuple.  Element 1 is bit-identical to solving it alone; element 0 meets that test's assertions."""
    from e2e_multi_view_matching_amd import multi_view
    T = 5
    dev, result = _five_tuple_inputs(gpu, seeds=(77, 78), n_kpts=256, unmatched_first=True)
    assert all(int((result[f"matches{i}_{i}_4"][0] >= 0).sum()) < 8 for i in range(4))
    whole = multi_view.solve_tuple_poses_batch(T, dev, result)
    alone = multi_view.solve_tuple_poses_batch(T, _slice(dev, 1), _slice(result, 1))
    assert np.array_equal(alone[0], whole[1])
    assert np.isfinite(whole).all()
    err_t, err_R = multi_view.tuple_pose_errors(whole[0], [dev[f"pose{v}"][0].cpu().numpy() for v in range(T)])
    e = np.maximum(err_t, err_R)
    good = np.array([e[k] for k, (i, j) in enumerate(multi_view._pairs(T)) if j != 4])
    assert np.isfinite(good).all() and good.max() < 3.0, good
    # the averaging stage leaves the isolated camera at the identity
    collected = multi_view._collect_matches_batch(T, _slice(dev, 0), _slice(result, 0), 0.)
    counts = collected[3].cpu().numpy()
    assert (counts[[6, 7, 8, 9]] < 8).all() and (counts[:6] >= 8).all()
    intr, kdim, nb = multi_view._tuple_intrinsics(T, dev, gpu, 2)
    P = len(multi_view._pairs(T))
    T_d, inl = multi_view._w8pt_ba_on_device(gpu, collected[3], collected[0], collected[1], collected[2],
                                             torch.stack([intr[i][:1] for i, _ in multi_view._pairs(T)], 1).reshape(P, kdim, kdim).contiguous(),
                                             torch.stack([intr[j][:1] for _, j in multi_view._pairs(T)], 1).reshape(P, kdim, kdim).contiguous())
    T_h, inl_h = T_d.cpu().numpy(), inl.cpu().numpy()
    assert np.array_equal(T_h[6:], np.tile(np.eye(4, dtype=np.float32), (4, 1, 1))) and not inl_h[6:].any()  # below 8 matches: not solved
    rel = {pr: T_h[q].astype(np.float64) for q, pr in enumerate(multi_view._pairs(T)) if counts[q] >= 8}
    graph = np.zeros((T, T), dtype=int)
    for q, (i, j) in enumerate(multi_view._pairs(T)):
        graph[i, j] = counts[q] if counts[q] >= 8 else 0
    arrays, _ = multi_view._init_arrays(T, rel, {pr: int(inl_h[q].sum()) for q, pr in enumerate(multi_view._pairs(T))}, graph)
    start = multi_view._averaged_extrinsics(*arrays)
    assert np.isfinite(start).all() and np.abs(start[4] - np.eye(4)).max() < 1e-12
