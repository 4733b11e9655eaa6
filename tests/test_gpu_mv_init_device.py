"""GPU: the global initialisation of the multi-view back-end on the device (csrc/mvinit_device.hip: ``e2emv_mv_init_batch``,
``e2emv_mv_tuple_init``; ``multi_view.averaged_extrinsics_batch``, ``solve_tuple_poses_batch(..., init="device")``).  The
yardstick is always the host solver ``e2emv_mv_init`` (for the whole path: ``init="host"``), never the device code against
itself; what the device code is compared with itself for is independence of the batch, bit for bit."""
import ctypes

import numpy as np
import pytest
import torch
from scipy.spatial.transform import Rotation

from test_gpu_mv_batch import _five_tuple_inputs, _slice
from test_mv_init import cameras, global_rotations, libc, view_pairs

pytestmark = pytest.mark.gpu

# Largest |device - host| as measured on an MI355X (printed by the tests below); every bar is ten times its figure, the rule of
# MEASURED_BATCH_VS_CSV in test_gpu_mv_batch.py: 4000 ADMM steps (and, for the whole path, the LM loop behind them) amplify
# last-bit differences by a factor that varies with the input.  For scale: the host solver's own response to a one-ulp
# perturbation of its inputs is 1e-14 - 1e-13 in the median and up to 5.2e-12; a solver figure above 1e-10 (bar above 1e-9)
# would be a finding, not a tolerance.
MEASURED_SOLVER_VS_HOST = 8.9e-13  # e2emv_mv_init_batch against e2emv_mv_init on the same arrays (out_t; out_R: 7.7e-16)
MEASURED_STAGE_VS_HOST = 1.1e-12   # e2emv_mv_tuple_init against _init_arrays + _averaged_extrinsics (T = 8; T = 5: 4.1e-13)
MEASURED_WHOLE_VS_HOST = 4.2e-13   # solve_tuple_poses_batch(init="device") against init="host", after bundle adjustment
BATCH_VS_CSV_BAR = 3.7e-7         # the existing bar between the batched and the CSV path: the whole-path bar stays below it


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _colmajor(R):
    return np.asarray(R).T.reshape(-1)


def _scene(rng, n, noise=0.0, outlier=False, drop=lambda i, j: False, init_noise=0.05):
    """A seeded scene in the array form of ``e2emv_mv_init``: unit-norm baselines, pair rotations and directions perturbed by
    ``noise`` rad, optionally one gross outlier rotation; ``drop(i, j)`` removes pairs."""
    Rw = [np.eye(3)] + [Rotation.from_rotvec(rng.normal(0, 0.4, 3)).as_matrix() for _ in range(n - 1)]
    c = [np.zeros(3)] + [rng.normal(0, 1.0, 3) for _ in range(n - 1)]
    ids, pR, pp = [], [], []
    for j in range(n):
        for i in range(j):
            if drop(i, j):
                continue
            Rij = Rotation.from_rotvec(rng.normal(0, 1.0, 3) * noise).as_matrix() @ Rw[j] @ Rw[i].T
            pos = Rw[i] @ (c[j] - c[i])
            pos = pos / np.linalg.norm(pos) + rng.normal(0, 1.0, 3) * noise
            ids.append((i, j))
            pR.append(_colmajor(Rij))
            pp.append(pos / np.linalg.norm(pos))
    if outlier and ids:
        pR[len(ids) // 2] = _colmajor(Rotation.from_rotvec([0.9, -0.7, 0.4]).as_matrix())
    init = np.array([_colmajor(Rw[v] @ Rotation.from_rotvec(rng.normal(0, init_noise, 3)).as_matrix()) for v in range(n)])
    return (init, np.array(ids, np.int32).reshape(-1, 2), np.array(pR, np.float64).reshape(-1, 9), np.array(pp, np.float64).reshape(-1, 3))


def _gtest_scene(max_err, init_err, outlier=False):
    """The four cameras of the reference's gtests in array form (pairs from ``view_pairs``, start from ``global_rotations``)."""
    extr = cameras()
    ids, rots, poss = view_pairs(extr, max_err)
    init = global_rotations(extr, init_err)
    if outlier:
        k = [tuple(i) for i in ids].index((1, 2))
        rots[k] = -0.5 * rots[k]
    mat = lambda r: _colmajor(Rotation.from_rotvec(r).as_matrix())  # noqa: E731
    return (np.array([mat(r) for r in init]), ids, np.array([mat(r) for r in rots]), np.ascontiguousarray(poss)), extr


def _host(arrays):
    """``e2emv_mv_init`` on one problem: ``(extrinsics [n,4,4], status)``."""
    from e2e_multi_view_matching_amd import _lib
    init, ids, pR, pp = (np.ascontiguousarray(a) for a in arrays)
    n = len(init)
    oR, ot, st = np.zeros((n, 9)), np.zeros((n, 3)), ctypes.c_int32(-1)
    assert _lib.load_library().e2emv_mv_init(n, _p(init), len(ids), _p(ids), _p(pR), _p(pp), _p(oR), _p(ot), ctypes.byref(st)) == 0
    E = np.tile(np.eye(4), (n, 1, 1))
    E[:, :3, :3] = oR.reshape(n, 3, 3).transpose(0, 2, 1)
    E[:, :3, 3] = ot
    return E, st.value


def _mixed_batch():
    libc.srand(7)
    rng = np.random.default_rng(11)
    probs = [_gtest_scene(0.02, 0.03)[0], _gtest_scene(0.0, 0.0, outlier=True)[0], _gtest_scene(0.05, 0.0)[0]]
    for n in (2, 3, 5, 8):
        for noise in (0.0, 0.003, 0.02):
            probs.append(_scene(rng, n, noise))
    probs.append(_scene(rng, 5, 0.003, outlier=True))
    probs.append(_scene(rng, 8, 0.003, outlier=True))
    for iso in (0, 2, 4):  # a view without any pair
        probs.append(_scene(rng, 5, 0.003, drop=lambda i, j, iso=iso: iso in (i, j)))
    probs.append(_scene(rng, 5, 0.003, drop=lambda i, j: (i < 3) != (j < 3)))  # two components {0,1,2} {3,4}
    probs.append(_scene(rng, 8, 0.02, drop=lambda i, j: (i + j) % 3 == 0))  # missing pairs
    probs.append(_scene(rng, 3, 0.0, drop=lambda i, j: True))  # no pair at all
    return probs


def test_known_answers_of_the_reference_gtest(gpu):
    """BaInit.PerfectInitPerfectRel: the four-camera scene with perfect data, rotations and translations within 1e-6 of
    ground truth (the gtest's own bar), here through ``e2emv_mv_init_batch``."""
    from e2e_multi_view_matching_amd import multi_view
    libc.srand(1)
    arrays, extr = _gtest_scene(0.0, 0.0)
    (E,), status = multi_view.averaged_extrinsics_batch([arrays])
    assert status[0] == 0
    err_R = max(np.abs(E[v][:3, :3] - extr[v][:3, :3]).max() for v in range(4))
    err_t = max(np.abs(E[v][:3, 3] - extr[v][:3, 3]).max() for v in range(4))
    print("known answers: max |R - gt|", err_R, " max |t - gt|", err_t)
    assert err_R < 1e-6 and err_t < 1e-6


def test_solver_against_the_host_solver_on_the_same_arrays(gpu):
    """One batch of gtest scenes (noise, the outlier pair), seeded scenes with 2, 3, 5 and 8 views at pair noise 0 / 0.003 /
    0.02 rad, a gross outlier rotation, isolated views at ids 0, 2 and 4, two components, missing pairs and a problem without
    pairs: status words equal, numbers within ten times the measured difference."""
    from e2e_multi_view_matching_amd import multi_view
    probs = _mixed_batch()
    dev_E, dev_status = multi_view.averaged_extrinsics_batch([(a, None) for a in probs])  # the form _init_arrays returns
    d_R, d_t = [], []
    for k, arrays in enumerate(probs):
        E, st = _host(arrays)
        assert dev_status[k] == st, (k, dev_status[k], st)
        assert dev_E[k].shape == E.shape and np.isfinite(dev_E[k]).all(), k
        d_R.append(np.abs(dev_E[k][:, :3, :3] - E[:, :3, :3]).max())
        d_t.append(np.abs(dev_E[k][:, :3, 3] - E[:, :3, 3]).max())
    print("solver, device against host: max |dR| per problem", ["%.2e" % d for d in d_R])
    print("solver, device against host: max |dt| per problem", ["%.2e" % d for d in d_t])
    print("solver, device against host: max |dR| %.3e  max |dt| %.3e" % (max(d_R), max(d_t)))
    assert np.array_equal(dev_E[-1][:, :3, 3], np.zeros((3, 3)))  # no pair: initial rotations, zero translations
    assert max(d_R) <= 10 * MEASURED_SOLVER_VS_HOST and max(d_t) <= 10 * MEASURED_SOLVER_VS_HOST, (max(d_R), max(d_t))
    assert 10 * MEASURED_SOLVER_VS_HOST <= 1e-9


def test_a_problem_does_not_depend_on_its_batch(gpu):
    """Every problem alone = itself at every position of the mixed batch (the batch rotated and reversed), and run to run."""
    from e2e_multi_view_matching_amd import multi_view
    probs = _mixed_batch()
    whole, st = multi_view.averaged_extrinsics_batch(probs)
    again, st2 = multi_view.averaged_extrinsics_batch(probs)
    back, st3 = multi_view.averaged_extrinsics_batch(probs[::-1])
    assert np.array_equal(st, st2) and np.array_equal(st, st3[::-1])
    for k, arrays in enumerate(probs):
        (alone,), st1 = multi_view.averaged_extrinsics_batch([arrays])
        assert np.array_equal(alone, whole[k]) and np.array_equal(alone, again[k]) and np.array_equal(alone, back[len(probs) - 1 - k]), k
        assert st1[0] == st[k]
    n = len(probs)
    for shift in range(1, n):  # the batch rotated: every problem visits every position
        moved, st4 = multi_view.averaged_extrinsics_batch(probs[shift:] + probs[:shift])
        for k in range(n):
            assert np.array_equal(moved[(k - shift) % n], whole[k]) and st4[(k - shift) % n] == st[k], (shift, k)


def _synthetic_tuples(B, T, seed):
    """fp32 relative poses of B tuples of T images as the w8pt + two-view-BA stage leaves them (rotations rounded to fp32, not
    re-orthonormalised; unit translations), with match and inlier counts: counts pairwise distinct inside a tuple, some below 8,
    image T - 1 of tuple 1 unreachable from image 0, the heaviest pair of every tuple (always on the tree) below 20 inliers and,
    in tuple 0 (all pairs present), the lightest pair (never on the tree) as well."""
    from e2e_multi_view_matching_amd import multi_view
    rng = np.random.default_rng(seed)
    pairs = multi_view._pairs(T)
    P = len(pairs)
    rel = np.zeros((B, P, 4, 4), np.float32)
    counts = np.zeros((B, P), np.int32)
    n_inl = np.zeros((B, P), np.int32)
    for b in range(B):
        Rw = [np.eye(3)] + [Rotation.from_rotvec(rng.normal(0, 0.4, 3)).as_matrix() for _ in range(T - 1)]
        c = [np.zeros(3)] + [rng.normal(0, 1.0, 3) for _ in range(T - 1)]
        counts[b] = rng.permutation(np.arange(30, 30 + 17 * P, 17))[:P]
        n_inl[b] = counts[b] - rng.integers(0, 9, P)
        if b >= 2:  # pairs below 8 matches (not solved: the identity, no inlier)
            for small, q in zip((0, 5) if b % 2 else (2, 7), rng.choice(P, 2, replace=False)):
                counts[b, q] = small
        if b == 1:  # image T - 1 shares nothing with the others
            for q, (i, j) in enumerate(pairs):
                if j == T - 1:
                    counts[b, q] = i  # 0 .. T - 2 < 8, distinct
        for q, (i, j) in enumerate(pairs):
            if counts[b, q] < 8:
                rel[b, q] = np.eye(4)
                n_inl[b, q] = 0
                continue
            Rij = Rotation.from_rotvec(rng.normal(0, 0.004, 3)).as_matrix() @ Rw[j] @ Rw[i].T
            t = Rw[j] @ (c[i] - c[j])
            t = t / np.linalg.norm(t) + rng.normal(0, 0.004, 3)
            rel[b, q, :3, :3], rel[b, q, :3, 3], rel[b, q, 3, 3] = Rij, t / np.linalg.norm(t), 1.0
        n_inl[b, np.argmax(counts[b])] = 5
        if b == 0:
            n_inl[b, np.argmin(counts[b])] = 3
    return rel, counts, n_inl


def _host_stage(T, rel, counts, n_inl):
    """The initialisation stage of ``solve_tuple_poses_batch(init="host")`` for one tuple; also returns the pair list it kept."""
    from e2e_multi_view_matching_amd import multi_view
    graph = np.zeros((T, T), dtype=int)
    r, ic = {}, {}
    for q, (i, j) in enumerate(multi_view._pairs(T)):
        if counts[q] >= 8:
            r[(i, j)], ic[(i, j)] = rel[q].astype(np.float64), int(n_inl[q])
            graph[i, j] = counts[q]
    arrays, poses = multi_view._init_arrays(T, r, ic, graph)
    return multi_view._averaged_extrinsics(*arrays), [tuple(p) for p in arrays[1]], poses


def _device_stage(gpu, T, rel, counts, n_inl):
    from e2e_multi_view_matching_amd import _lib
    B = len(rel)
    d_rel = torch.from_numpy(np.ascontiguousarray(rel.reshape(-1, 16))).to(gpu)
    d_cnt, d_inl = torch.from_numpy(np.ascontiguousarray(counts.reshape(-1))).to(gpu), torch.from_numpy(np.ascontiguousarray(n_inl.reshape(-1))).to(gpu)
    extr = torch.empty((B, T, 16), dtype=torch.float64, device=gpu)
    status = torch.empty((B,), dtype=torch.int32, device=gpu)
    with torch.cuda.device(gpu):
        _lib.context(gpu).call("e2emv_mv_tuple_init", B, T, _lib.ptr(d_rel), _lib.ptr(d_inl), _lib.ptr(d_cnt), 8, 20, _lib.ptr(extr), _lib.ptr(status),
                               _lib.stream_ptr(gpu))
    return extr.cpu().numpy().reshape(B, T, 4, 4), status.cpu().numpy()


@pytest.mark.parametrize("B,T,seed", [(5, 5, 31), (1, 8, 32)])
def test_stage_against_the_python_stage(gpu, B, T, seed):
    """``e2emv_mv_tuple_init`` (spanning tree, chained start, pair selection, solver) against ``_init_arrays`` +
    ``_averaged_extrinsics`` per tuple on synthetic fp32 relative poses.  No tie rule is exercised: the counts of a tuple are
    pairwise distinct (asserted)."""
    from e2e_multi_view_matching_amd import multi_view
    rel, counts, n_inl = _synthetic_tuples(B, T, seed)
    pairs = multi_view._pairs(T)
    for b in range(B):
        assert len(set(counts[b])) == len(pairs), counts[b]
    assert (counts < 8).any() or B == 1
    dev, status = _device_stage(gpu, T, rel, counts, n_inl)
    diffs = []
    for b in range(B):
        want, kept, poses = _host_stage(T, rel[b], counts[b], n_inl[b])
        heavy, light = pairs[int(np.argmax(counts[b]))], pairs[int(np.argmin(counts[b]))]
        assert heavy in kept  # below 20 inliers but on the tree
        if b == 0:
            assert counts[b].min() >= 8 and light not in kept  # below 20 inliers and off the tree
        if b == 1 and B > 1:
            assert (T - 1) not in poses and np.abs(dev[b, T - 1] - np.eye(4)).max() < 1e-12  # unreachable: the identity
        assert status[b] == 0
        diffs.append(np.abs(dev[b] - want).max())
    print("stage, device against host (B = %d, T = %d): max |dE| per tuple" % (B, T), ["%.2e" % d for d in diffs])
    assert max(diffs) <= 10 * MEASURED_STAGE_VS_HOST, diffs
    assert 10 * MEASURED_STAGE_VS_HOST <= 1e-9
    # a tuple alone = itself at every position of a batch, and run to run
    again, _ = _device_stage(gpu, T, rel, counts, n_inl)
    assert np.array_equal(dev, again)
    back, _ = _device_stage(gpu, T, rel[::-1], counts[::-1], n_inl[::-1])
    assert np.array_equal(dev, back[::-1])
    for b in range(B):
        alone, _ = _device_stage(gpu, T, rel[b:b + 1], counts[b:b + 1], n_inl[b:b + 1])
        assert np.array_equal(alone[0], dev[b]), b
    for shift in range(1, B):  # the batch rotated: every tuple visits every position
        moved, _ = _device_stage(gpu, T, np.roll(rel, -shift, 0), np.roll(counts, -shift, 0), np.roll(n_inl, -shift, 0))
        assert np.array_equal(np.roll(moved, shift, 0), dev), shift


@pytest.fixture(scope="module")
def three_tuples(gpu):
    return _five_tuple_inputs(gpu, seeds=(20, 21, 22), n_kpts=512)


def test_whole_path_device_against_host(gpu, three_tuples):
    """``solve_tuple_poses_batch(init="device")`` against ``init="host"`` on the three 512-keypoint five-tuples: extrinsics within
    ten times the measured difference (and below the bar between the batched and the CSV path), pose errors at the bars of
    ``test_whole_path_against_the_csv_path``; the default is the host path, bit for bit; independent of the batch."""
    from e2e_multi_view_matching_amd import multi_view, pose_auc
    dev, result = three_tuples
    host = multi_view.solve_tuple_poses_batch(5, dev, result, init="host")
    assert np.array_equal(multi_view.solve_tuple_poses_batch(5, dev, result), host)
    tm = {}
    device = multi_view.solve_tuple_poses_batch(5, dev, result, init="device", timings=tm)
    assert sorted(tm) == ["build_and_bundle_adjust", "collect", "initialisation", "relative_poses"]
    assert device.shape == (3, 5, 4, 4) and device.dtype == np.float64 and np.isfinite(device).all()
    diffs = [np.abs(device[b] - host[b]).max() for b in range(3)]
    print("whole path, init=device against init=host: max |dE| per tuple", ["%.2e" % d for d in diffs])
    assert max(diffs) <= min(10 * MEASURED_WHOLE_VS_HOST, BATCH_VS_CSV_BAR), diffs
    errs = multi_view.eval_bundle_adjust_batch(5, dev, result, [[], [], []], init="device")
    e = np.array(errs[0])
    auc = pose_auc(e, [5, 10, 20])
    print("pose errors (degrees), init=device: max", e.max(), "auc", auc)
    assert len(e) == 30 and e.max() < 2.0 and auc[0] > 0.8, (e, auc)
    assert np.array_equal(device, multi_view.solve_tuple_poses_batch(5, dev, result, init="device"))  # run to run
    for b in range(3):
        alone = multi_view.solve_tuple_poses_batch(5, _slice(dev, b), _slice(result, b), init="device")
        assert np.array_equal(alone[0], device[b]), b


def test_a_degenerate_tuple_on_the_device_path(gpu):
    """The batch of ``test_a_degenerate_tuple_inside_a_batch`` (image 4 of element 0 shares nothing with the others) with
    ``init="device"``: that test's assertions, the isolated camera's start the identity, and device against host."""
    from e2e_multi_view_matching_amd import multi_view
    T = 5
    dev, result = _five_tuple_inputs(gpu, seeds=(77, 78), n_kpts=256, unmatched_first=True)
    host = multi_view.solve_tuple_poses_batch(T, dev, result, init="host")
    assert np.array_equal(multi_view.solve_tuple_poses_batch(T, dev, result), host)
    whole = multi_view.solve_tuple_poses_batch(T, dev, result, init="device")
    alone = multi_view.solve_tuple_poses_batch(T, _slice(dev, 1), _slice(result, 1), init="device")
    assert np.array_equal(alone[0], whole[1]) and np.isfinite(whole).all()
    diffs = [np.abs(whole[b] - host[b]).max() for b in range(2)]
    print("degenerate batch, init=device against init=host: max |dE| per tuple", ["%.2e" % d for d in diffs])
    assert max(diffs) <= min(10 * MEASURED_WHOLE_VS_HOST, BATCH_VS_CSV_BAR), diffs
    err_t, err_R = multi_view.tuple_pose_errors(whole[0], [dev[f"pose{v}"][0].cpu().numpy() for v in range(T)])
    e = np.maximum(err_t, err_R)
    good = np.array([e[k] for k, (i, j) in enumerate(multi_view._pairs(T)) if j != 4])
    assert np.isfinite(good).all() and good.max() < 3.0, good
    # the start the device stage hands to the bundle adjustment
    collected = multi_view._collect_matches_batch(T, dev, result, 0.)
    intr, kdim, nb = multi_view._tuple_intrinsics(T, dev, gpu, 2)
    pairs = multi_view._pairs(T)
    P = len(pairs)
    per_pair = lambda side: torch.stack([intr[pr[side]].expand(2, kdim, kdim) for pr in pairs], 1).reshape(2 * P, kdim, kdim).contiguous()  # noqa: E731
    T_d, inl = multi_view._w8pt_ba_on_device(gpu, collected[3], collected[0], collected[1], collected[2], per_pair(0), per_pair(1))
    start, counts = multi_view._tuple_init_on_device(T, T_d, inl, collected[3])
    assert np.array_equal(counts, collected[3].cpu().numpy()) and (counts[[6, 7, 8, 9]] < 8).all()
    assert np.isfinite(start).all() and np.abs(start[0, 4] - np.eye(4)).max() < 1e-12
    assert np.abs(start[:, 0] - np.eye(4)).max() < 1e-9  # camera 0 is the gauge


def test_entry_points_validate_their_arguments(gpu):
    from e2e_multi_view_matching_amd import _lib
    ctx = _lib.context(gpu)
    init = np.tile(np.eye(3).reshape(-1), (5, 1))
    pR, pp = np.tile(np.eye(3).reshape(-1), (3, 1)), np.tile([1.0, 0, 0], (3, 1))
    oR, ot, st = np.zeros((5, 9)), np.zeros((5, 3)), np.zeros(2, np.int32)

    def call(n_views, pair_off, ids, init_R=init, out=oR):
        ids = np.array(ids, np.int32).reshape(-1, 2)
        return ctx.lib.e2emv_mv_init_batch(ctx.h, 2, _p(np.array(n_views, np.int32)), None if init_R is None else _p(init_R),
                                           _p(np.array(pair_off, np.int64)), _p(ids), _p(pR), _p(pp), None if out is None else _p(out), _p(ot),
                                           _p(st), None)

    good = [(0, 1), (1, 2), (0, 1)]
    assert call([3, 2], [0, 2, 3], good) == _lib.OK
    assert call([3, 9], [0, 2, 3], good) == _lib.EINVAL and b"views" in ctx.lib.e2emv_last_error(ctx.h)
    assert call([0, 2], [0, 2, 3], good) == _lib.EINVAL
    assert call([3, 2], [0, 2, 3], [(0, 1), (1, 3), (0, 1)]) == _lib.EINVAL  # view 3 of a 3-view problem
    assert call([3, 2], [0, 2, 3], [(0, 1), (1, 2), (1, 1)]) == _lib.EINVAL  # i == j
    assert call([3, 2], [0, 2, 3], [(0, 1), (1, 0), (0, 1)]) == _lib.EINVAL  # the same pair twice
    assert call([3, 2], [0, 2, 1], good) == _lib.EINVAL and b"decrease" in ctx.lib.e2emv_last_error(ctx.h)
    assert call([3, 2], [1, 2, 3], good) == _lib.EINVAL and b"start at 0" in ctx.lib.e2emv_last_error(ctx.h)
    assert call([3, 2], [0, 2, 3], good, init_R=None) == _lib.EINVAL
    assert call([3, 2], [0, 2, 3], good, out=None) == _lib.EINVAL
    assert ctx.lib.e2emv_mv_init_batch(ctx.h, 0, None, None, None, None, None, None, None, None, None, None) == _lib.EINVAL

    d_rel = torch.eye(4, device=gpu).reshape(1, 16).repeat(10, 1).contiguous()
    d_i = torch.zeros(10, dtype=torch.int32, device=gpu)
    extr, status = torch.empty((1, 5, 16), dtype=torch.float64, device=gpu), torch.empty(1, dtype=torch.int32, device=gpu)
    P = _lib.ptr

    def tcall(B, T, rel=d_rel, out=extr):
        return ctx.lib.e2emv_mv_tuple_init(ctx.h, B, T, P(rel), P(d_i), P(d_i), 8, 20, P(out), P(status), _lib.stream_ptr(gpu))

    assert tcall(1, 5) == _lib.OK
    torch.cuda.synchronize()
    assert np.array_equal(extr.cpu().numpy().reshape(5, 4, 4), np.tile(np.eye(4), (5, 1, 1))) and int(status[0]) == 0  # no edge at all
    assert tcall(1, 9) == _lib.EINVAL and b"tuple" in ctx.lib.e2emv_last_error(ctx.h)
    assert tcall(1, 1) == _lib.EINVAL
    assert tcall(0, 5) == _lib.EINVAL
    assert tcall(1, 5, rel=None) == _lib.EINVAL
    assert tcall(1, 5, out=None) == _lib.EINVAL
