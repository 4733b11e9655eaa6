"""Drop-in for ``pose_optimization/multi_view/bundle_adjust_io.py`` and the ``eval_bundle_adjust`` routine of
``eval_multi_view.py:21-68``: pairwise poses -> spanning-tree initialisation -> global rotation /
position averaging -> weighted bundle adjustment, keeping the reference's CSV wire format (``ba_init_in/out.csv``,
``ba_in/out.csv``).

Same function names, arguments, dictionary keys and file layouts as the reference.  What differs is where the work runs:
* relative poses: the HIP w8pt + two-view BA kernels (``pose.py``) instead of kornia/pytorch3d ops, and the RANSAC
  baseline (``ransac.py``: 5-point RANSAC + recoverPose on the device) instead of OpenCV; all three methods on the CSV path
  and on the batched path (``rel_pose_method``);
* ``ba_initializer`` / ``bundle_adjuster``: not separate executables built on Theia/Ceres but entry points of
  libe2emv.so called in-process (``run_ba_initializer`` = host C++ averaging, ``run_bundle_adjuster`` = one HIP workgroup
  doing the whole LM/Schur optimisation; the batched path can run the averaging on the device instead, one wave per tuple:
  ``solve_tuple_poses_batch(..., init="device")``, ``averaged_extrinsics_batch``); ``python -m e2e_multi_view_matching_amd.multi_view ba_initializer <dir>`` and
  ``... bundle_adjuster <dir>`` give the reference's command-line shape;
* triangulation: ``cv2.triangulatePoints`` (OpenCV is absent) -> ``e2emv_mv_triangulate`` (same homogeneous DLT).
Host glue (dict plumbing, spanning tree via scipy like the reference, CSV text) stays in Python like the reference's.
No CPU fallback for the device parts.
"""
import ctypes
import logging
import os
import sys

import numpy as np
import torch
from scipy.sparse.csgraph import minimum_spanning_tree

from . import _lib
from .pose import LOSSES, _check_loss, mask_confidence, run_bundle_adjust_2_view  # noqa: F401  (LOSSES: part of this module's names)
from .ransac import MAX_MATCHES, estimate_poses_ransac, normalize_keypoints


def _dev():
    if not torch.cuda.is_available():
        raise RuntimeError("the multi-view back-end needs an MI355X (no CPU fallback)")
    return torch.device("cuda", torch.cuda.current_device())


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _w8pt_ba_on_device(dev, d_n, d_k0, d_k1, d_cf, d_K0, d_K1, n_iterations=10, loss=None, loss_scale=None):
    """The launch sequence behind every "w8pt_ba" relative pose, on device buffers: ``e2emv_w8pt_ragged`` (``d_n`` [Pn] int32
    rows in use of ``d_k0`` / ``d_k1`` [Pn,N,2], ``d_cf`` [Pn,N]; intrinsics [Pn,k,k]) -> confidences of negative-depth matches
    zeroed -> two-view bundle adjustment.  A problem with fewer than 8 rows comes back as the identity with no inlier.
    ``loss``, ``loss_scale``: the robust loss of the two-view bundle adjustment, as in ``run_bundle_adjust_2_view``.
    Returns ``(T [Pn,4,4] float32, inliers [Pn,N] uint8)`` on the device."""
    loss_kw = dict(loss=loss, loss_scale=loss_scale) if _check_loss(loss, loss_scale) else {}  # without a loss: the call as it always was
    ctx = _lib.context(dev)
    Pn, N = d_k0.shape[:2]
    kdim = d_K0.shape[-1]
    T = torch.empty((Pn, 4, 4), dtype=torch.float32, device=dev)
    k0n, k1n, cfn = torch.empty_like(d_k0), torch.empty_like(d_k1), torch.empty_like(d_cf)
    inl = torch.empty((Pn, N), dtype=torch.uint8, device=dev)
    pos = torch.empty((Pn, N), dtype=torch.uint8, device=dev)
    status = torch.empty((Pn,), dtype=torch.int32, device=dev)
    P = _lib.ptr
    with torch.cuda.device(dev):
        ctx.call("e2emv_w8pt_ragged", Pn, N, P(d_n), P(d_k0), P(d_k1), P(d_K0), P(d_K1), kdim, Pn, P(d_cf), 0, P(None), 1, P(T),
                 P(k0n), P(k1n), P(cfn), P(inl), P(pos), P(None), P(status), _lib.stream_ptr(dev))
    refined, ok = run_bundle_adjust_2_view(k0n, k1n, mask_confidence(cfn, pos), T, n_iterations=n_iterations, **loss_kw)
    T[ok] = refined
    return T, inl


def relative_poses_w8pt_ba(problems, n_iterations=10, loss=None, loss_scale=None):
    """Relative pose of MANY image pairs with different numbers of matches in one device pass: ragged weighted 8-point
    (``e2emv_w8pt_ragged``: every pair keeps its own Hartley statistics) -> confidences of negative-depth matches zeroed
    -> two-view bundle adjustment (zero-weight padding rows do not enter it).  ``problems`` = list of
    ``(intr0, intr1, mkpts0 [n,2], mkpts1 [n,2], conf [n,c])`` numpy tuples; returns one ``(success, R, t, inliers)`` per
    problem with the meaning of the reference's ``estimate_relative_pose_w8pt_ba`` (bundle_adjust_io.py:12-23):
    ``success`` is False below 8 matches.  ``loss``, ``loss_scale``: the robust loss of the two-view bundle adjustment, as in
    ``run_bundle_adjust_2_view`` (``ValueError`` before any device call)."""
    _check_loss(loss, loss_scale)
    out = [(False, None, None, None)] * len(problems)
    live = [q for q, pr in enumerate(problems) if pr[2].shape[0] >= 8]
    if not live:
        return out
    dev = _dev()
    n_per = np.array([problems[q][2].shape[0] for q in live], np.int32)
    Pn, Nmax = len(live), int(n_per.max())
    kdim = problems[live[0]][0].shape[-1]
    k0, k1 = np.zeros((Pn, Nmax, 2), np.float32), np.zeros((Pn, Nmax, 2), np.float32)
    cf = np.zeros((Pn, Nmax), np.float32)
    K0, K1 = np.zeros((Pn, kdim, kdim), np.float32), np.zeros((Pn, kdim, kdim), np.float32)
    for r, q in enumerate(live):
        intr0, intr1, m0, m1, conf = problems[q]
        k0[r, :n_per[r]], k1[r, :n_per[r]] = m0, m1
        cf[r, :n_per[r]] = np.asarray(conf).reshape(n_per[r], -1)[:, 0]
        K0[r], K1[r] = intr0, intr1
    up = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731
    T, inl = _w8pt_ba_on_device(dev, up(n_per), up(k0), up(k1), up(cf), up(K0), up(K1), n_iterations, loss, loss_scale)
    T_h, inl_h = T.cpu().numpy(), inl.cpu().numpy().astype(bool)
    for r, q in enumerate(live):
        out[q] = (True, T_h[r, :3, :3], T_h[r, :3, 3], inl_h[r, :n_per[r]])
    return out


def estimate_relative_pose_w8pt_ba(intr0, intr1, mkpts0, mkpts1, conf):
    """``estimate_relative_pose_w8pt_ba`` (bundle_adjust_io.py:12-23): numpy in, ``(success, R, t, inliers)`` out - the
    one-pair form of ``relative_poses_w8pt_ba``."""
    return relative_poses_w8pt_ba([(intr0, intr1, mkpts0, mkpts1, conf)])[0]


def relative_poses_ransac(problems, ba=False, n_iterations=10, loss=None, loss_scale=None):
    """Relative pose of MANY image pairs by the RANSAC baseline in one device pass: ``estimate_pose(..., thresh=1.0)``
    (5-point RANSAC + recoverPose, ``ransac.py``) for all pairs, then with ``ba`` the two-view bundle adjustment of every
    solved pair on its RANSAC inliers only, weighted by their confidences and started from the RANSAC pose (one batched
    launch; zero-weight padding rows do not enter it).  ``problems`` = list of ``(intr0, intr1, mkpts0 [n,2], mkpts1 [n,2],
    conf [n,c])``; returns one ``(success, R, t, inliers)`` per problem with the meaning of the reference's
    ``estimate_relative_pose_ransac`` / ``estimate_relative_pose_ransac_ba`` (bundle_adjust_io.py:25-58).  ``loss``,
    ``loss_scale``: the robust loss of the two-view bundle adjustment, as in ``run_bundle_adjust_2_view``; they need ``ba=True``
    (``ValueError`` before any device call: the RANSAC alone has no two-view bundle adjustment)."""
    loss_kw = dict(loss=loss, loss_scale=loss_scale) if _check_loss(loss, loss_scale) else {}
    if loss_kw and not ba:
        raise ValueError("loss={!r} needs ba=True: the RANSAC alone has no two-view bundle adjustment".format(loss))
    poses = estimate_poses_ransac([(m0, m1, K0, K1) for K0, K1, m0, m1, _ in problems], thresh=1.0)
    out = [(False, None, None, None) if r is None else (True, r[0], r[1], r[2]) for r in poses]
    solved = [q for q, r in enumerate(poses) if r is not None]
    if not ba or not solved:
        return out
    dev = _dev()
    n_in = [int(poses[q][2].sum()) for q in solved]
    Pn, Nmax = len(solved), max(n_in)
    k0, k1 = np.zeros((Pn, Nmax, 2), np.float32), np.zeros((Pn, Nmax, 2), np.float32)
    cf = np.zeros((Pn, Nmax), np.float32)
    T0 = np.tile(np.eye(4, dtype=np.float32), (Pn, 1, 1))
    for r, q in enumerate(solved):
        K0, K1, m0, m1, conf = problems[q]
        R, t, inl = poses[q]
        k0[r, :n_in[r]] = normalize_keypoints(m0[inl], K0)
        k1[r, :n_in[r]] = normalize_keypoints(m1[inl], K1)
        cf[r, :n_in[r]] = np.asarray(conf).reshape(len(m0), -1)[inl, 0]
        T0[r, :3, :3], T0[r, :3, 3] = R, t
    up = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731
    T = up(T0)
    refined, ok = run_bundle_adjust_2_view(up(k0), up(k1), up(cf), T, n_iterations=n_iterations, **loss_kw)
    T[ok] = refined
    T_h = T.cpu().numpy()
    for r, q in enumerate(solved):
        out[q] = (True, T_h[r, :3, :3], T_h[r, :3, 3], poses[q][2])
    return out


def estimate_relative_pose_ransac(intr0, intr1, mkpts0, mkpts1):
    """``estimate_relative_pose_ransac`` (bundle_adjust_io.py:44-54): ``(success, R, t, inliers)``."""
    return relative_poses_ransac([(intr0, intr1, mkpts0, mkpts1, np.ones((len(mkpts0), 1), np.float32))])[0]


def estimate_relative_pose_ransac_ba(intr0, intr1, mkpts0, mkpts1, conf):
    """``estimate_relative_pose_ransac_ba`` (bundle_adjust_io.py:25-42): RANSAC, then the two-view bundle adjustment on the
    inliers weighted by ``conf[inliers]``; ``(success, R, t, inliers)``."""
    return relative_poses_ransac([(intr0, intr1, mkpts0, mkpts1, conf)], ba=True)[0]


def _pairs(n_images):
    """Image pairs in the reference's enumeration order (second index outer): (0,1), (0,2), (1,2), (0,3), ..."""
    return [(i, j) for j in range(n_images) for i in range(j)]


def _key(kind, *ids):
    return kind + "_".join(str(i) for i in ids)


def _csv(values):
    return ",".join(str(v) for v in values) + "\n"  # str(x) is what "{}".format(x) writes in the reference


def _colmajor(R):
    return [R[r, c] for c in range(3) for r in range(3)]


def normalize_confidences(obs_xyc):
    """bundle_adjust_io.py:56-60: weights rescaled so that they sum to 2 over all observations (each match is seen twice)."""
    total = obs_xyc[:, 2:].sum(axis=0, keepdims=True) + 1e-3
    obs_xyc[:, 2:] = obs_xyc[:, 2:] / (0.5 * total)
    return obs_xyc


def _collect_matches(n_images, data, result, conf_thresh):
    """First stage of bundle_adjust_io.py:62-96: matched keypoints / confidences / intrinsics of batch element 0."""
    pw = {}
    for i, j in _pairs(n_images):
        mkey = _key("matches", str(i), i, j)
        if mkey not in result:
            continue
        if "keypoints" + str(i) in data:
            k0, k1 = data["keypoints" + str(i)], data["keypoints" + str(j)]
        else:
            k0, k1 = data[_key("keypoints", str(i), i, j)], data[_key("keypoints", str(j), i, j)]
        k0, k1 = k0[0].cpu().numpy(), k1[0].cpu().numpy()
        m = result[mkey][0].cpu().numpy()
        c = result[_key("conf_scores_", i, j)][0].cpu().numpy()
        keep = (m >= 0) & np.all(c > conf_thresh, -1)
        pw[_key("mkpts", str(i), i, j)] = k0[keep]
        pw[_key("mkpts", str(j), i, j)] = k1[m[keep]]
        pw[_key("conf", str(i), i, j)] = pw[_key("conf", str(j), i, j)] = c[keep]
        pw["intr" + str(i)] = data["intr" + str(i)][0].cpu().numpy()
        pw["intr" + str(j)] = data["intr" + str(j)][0].cpu().numpy()
    return pw


def _chain_along_tree(n_images, edges, rel_pose):
    """Absolute camera-to-world poses by walking the spanning tree outwards from image 0 (bundle_adjust_io.py:141-161):
    across edge (a, b), a < b:  pose_b = pose_a @ inv(T_a->b)  and  pose_a = pose_b @ T_a->b."""
    pose = {0: np.eye(4)}
    frontier = [0]
    while frontier:
        cur = frontier.pop()
        for a, b in edges:
            if cur == a and b not in pose:
                pose[b] = pose[a] @ np.linalg.inv(rel_pose[(a, b)])
                frontier.append(b)
            elif cur == b and a not in pose:
                pose[a] = pose[b] @ rel_pose[(a, b)]
                frontier.append(a)
    return pose


def _init_arrays(n_images, rel, inlier_count, graph, min_inliers=20):
    """Second stage of ``initialize_bundle_adjust`` (bundle_adjust_io.py:133-189) as arrays: ``rel`` {(i, j): 4x4 relative
    pose}, ``inlier_count`` {(i, j): count}, ``graph`` [n,n] int match-graph weights (0 = no edge) -> maximum spanning tree ->
    poses chained from image 0 -> the pairs worth keeping (``min_inliers`` or a tree edge).  Returns ``((init_R [n,9], pair_ids
    [k,2] int32, pair_R [k,9], pair_pos [k,3]), {image: camera-to-world 4x4})``, rotations column-major: the arguments of
    ``e2emv_mv_init`` and, as text, the rows of ``ba_init_in.csv``."""
    graph = np.array(graph, dtype=int)
    # maximum spanning tree = minimum spanning tree of (max - w + 1) on the existing edges (:135-138)
    has_edge = graph != 0
    graph[has_edge] = np.amax(graph) - graph[has_edge] + 1
    tree = minimum_spanning_tree(graph).toarray().astype(int)
    tree_edges = [(min(r, c), max(r, c)) for r, c in zip(*np.nonzero(tree))]
    abs_pose = {0: np.eye(4)}
    abs_pose.update(_chain_along_tree(n_images, tree_edges, rel))
    world_to_cam = [np.linalg.inv(abs_pose[v]) if v in abs_pose else np.eye(4) for v in range(n_images)]
    init_R = np.array([_colmajor(world_to_cam[v][:3, :3]) for v in range(n_images)], np.float64).reshape(n_images, 9)
    ids, pair_R, pair_pos = [], [], []
    for i, j in _pairs(n_images):
        if (i, j) in rel and (inlier_count[(i, j)] >= min_inliers or (i, j) in tree_edges):
            R = rel[(i, j)][:3, :3]
            ids.append((i, j))
            pair_R.append(_colmajor(R))
            pair_pos.append(-R.transpose() @ rel[(i, j)][:3, 3])  # camera j in the frame of camera i
    return (init_R, np.array(ids, np.int32).reshape(-1, 2), np.array(pair_R, np.float64).reshape(-1, 9),
            np.array(pair_pos, np.float64).reshape(-1, 3)), abs_pose


def _init_csv_lines(init_R, pair_ids, pair_R, pair_pos):
    """The arrays of ``_init_arrays`` as the rows of ``ba_init_in.csv``."""
    lines = [_csv([v] + list(R)) for v, R in enumerate(init_R)]  # 10 fields, ba_init.cpp:18-30
    lines += [_csv([int(i), int(j)] + list(R) + list(pos)) for (i, j), R, pos in zip(pair_ids, pair_R, pair_pos)]  # 14 fields, :31-50
    return lines


def _averaged_extrinsics(init_R, pair_ids, pair_R, pair_pos):
    """``e2emv_mv_init`` (= ``ba_initializer`` without its files) on the arrays of ``_init_arrays``: world-to-camera [n,4,4]."""
    n = len(init_R)
    init_R, pair_R, pair_pos = (np.ascontiguousarray(a, np.float64) for a in (init_R, pair_R, pair_pos))
    pair_ids = np.ascontiguousarray(pair_ids, np.int32)
    out_R, out_t, status = np.zeros((n, 9)), np.zeros((n, 3)), ctypes.c_int32(0)
    rc = _lib.load_library().e2emv_mv_init(n, _p(init_R), len(pair_ids), _p(pair_ids), _p(pair_R), _p(pair_pos), _p(out_R), _p(out_t),
                                           ctypes.byref(status))
    if rc != 0:
        raise _lib.E2EMVError(rc, "e2emv_mv_init failed")
    E = np.tile(np.eye(4), (n, 1, 1))
    E[:, :3, :3] = out_R.reshape(n, 3, 3).transpose(0, 2, 1)
    E[:, :3, 3] = out_t
    return E


def averaged_extrinsics_batch(problems):
    """``_averaged_extrinsics`` for MANY problems in one kernel launch on the device, one wave each (``e2emv_mv_init_batch``).
    ``problems``: list of ``_init_arrays`` outputs (``((init_R, pair_ids, pair_R, pair_pos), poses)``) or of the four arrays
    alone; at most 8 views and 28 pairs each, a pair of views at most once.  Returns ``(extrinsics, status)``: one world-to-camera
    ``[n,4,4]`` per problem and the int32 status words of the solver (bit 1: rotations failed, bit 2: positions failed; not
    raised, as on the host path).  Same solver and options as ``e2emv_mv_init``; the numbers agree to rounding."""
    if not problems:
        return [], np.zeros(0, np.int32)
    dev = _dev()
    arrays = [pr[0] if len(pr) == 2 else pr for pr in problems]
    n_views = np.array([len(a[0]) for a in arrays], np.int32)
    n_pairs = [len(a[1]) for a in arrays]
    cat = lambda k, dt, w: np.ascontiguousarray(np.concatenate([np.asarray(a[k], dt).reshape(-1, w) for a in arrays]))  # noqa: E731
    init_R, pair_ids, pair_R, pair_pos = cat(0, np.float64, 9), cat(1, np.int32, 2), cat(2, np.float64, 9), cat(3, np.float64, 3)
    if [len(np.asarray(a[2]).reshape(-1, 9)) for a in arrays] != n_pairs or [len(np.asarray(a[3]).reshape(-1, 3)) for a in arrays] != n_pairs:
        raise ValueError("averaged_extrinsics_batch: a problem's pair arrays disagree in length")
    pair_off = np.concatenate([[0], np.cumsum(n_pairs)]).astype(np.int64)
    tot = int(n_views.sum())
    out_R, out_t, status = np.zeros((tot, 9)), np.zeros((tot, 3)), np.zeros(len(arrays), np.int32)
    with torch.cuda.device(dev):
        _lib.context(dev).call("e2emv_mv_init_batch", len(arrays), _p(n_views), _p(init_R), _p(pair_off), _p(pair_ids), _p(pair_R), _p(pair_pos),
                               _p(out_R), _p(out_t), _p(status), _lib.stream_ptr(dev))
    E = np.tile(np.eye(4), (tot, 1, 1))
    E[:, :3, :3] = out_R.reshape(tot, 3, 3).transpose(0, 2, 1)
    E[:, :3, 3] = out_t
    off = np.concatenate([[0], np.cumsum(n_views)])
    return [E[off[k]:off[k + 1]].copy() for k in range(len(arrays))], status


def initialize_bundle_adjust(n_images, data, result, file_path, conf_thresh=0., rel_pose_method="w8pt_ba"):
    """``initialize_bundle_adjust`` (bundle_adjust_io.py:62-191): matches of batch element 0 -> pairwise poses on the device
    (``rel_pose_method`` "w8pt_ba": w8pt + two-view BA; "ransac" / "ransac_ba": the RANSAC baseline, without / with two-view
    BA on its inliers) -> maximum spanning tree of the inlier-count graph -> chained absolute poses -> ``ba_init_in.csv``.
    Returns the reference's ``pair_wise_data`` dictionary (same keys)."""
    _check_rel_pose_method(rel_pose_method)
    ransac = rel_pose_method != "w8pt_ba"
    min_inliers = 20
    pw = _collect_matches(n_images, data, result, conf_thresh)
    graph = np.zeros((n_images, n_images), dtype=int)
    rel = {}
    have = [(i, j) for i, j in _pairs(n_images) if _key("mkpts", str(i), i, j) in pw]
    # all pairs of the tuple in one device pass (they differ in their number of matches)
    problems = [(pw["intr" + str(i)], pw["intr" + str(j)], pw[_key("mkpts", str(i), i, j)], pw[_key("mkpts", str(j), i, j)],
                 pw[_key("conf", str(i), i, j)]) for i, j in have]
    solved = relative_poses_ransac(problems, ba=rel_pose_method == "ransac_ba") if ransac else relative_poses_w8pt_ba(problems)
    for (i, j), (ok, R, t, inl) in zip(have, solved):
        # w8pt_ba: every match is kept for the bundle adjustment, the inlier count only weights the match graph (:111-113,
        # :133); ransac / ransac_ba: matches and confidences are filtered to the RANSAC inliers (:104-131)
        pw[_key("inlier_count", i, j)] = inl.sum() if ok else 0
        if ok and ransac:
            for v in (i, j):
                pw[_key("mkpts", str(v), i, j)] = pw[_key("mkpts", str(v), i, j)][inl]
                pw[_key("conf", str(v), i, j)] = pw[_key("conf", str(v), i, j)][inl]
        if ok:
            T = np.eye(4)
            T[:3, :3], T[:3, 3] = R, t
            pw[_key("rel_pose", i, j)] = rel[(i, j)] = T
            graph[i, j] = len(pw[_key("mkpts", str(i), i, j)])

    inlier_count = {(i, j): pw[_key("inlier_count", i, j)] for i, j in rel}
    arrays, abs_pose = _init_arrays(n_images, rel, inlier_count, graph, min_inliers)
    for node, P in abs_pose.items():
        pw["abs_init_pose" + str(node)] = P
    lines = _init_csv_lines(*arrays)
    with open(file_path, "w") as f:
        f.writelines(lines)
    return pw


def triangulate_points(P0, P1, x0, x1):
    """``cv2.triangulatePoints`` + dehomogenisation as used at bundle_adjust_io.py:226-227; P [3,4], x [n,2] -> [n,3]."""
    ctx = _lib.context(_dev())
    n = x0.shape[0]
    P0, P1 = np.ascontiguousarray(P0, np.float64), np.ascontiguousarray(P1, np.float64)
    x0, x1 = np.ascontiguousarray(x0, np.float64), np.ascontiguousarray(x1, np.float64)
    out = np.zeros((n, 3))
    ctx.call("e2emv_mv_triangulate", n, _p(P0), _p(P1), _p(x0), _p(x1), _p(out), _lib.stream_ptr(_dev()))
    return out


def write_bundle_adjust_problem(n_images, pair_wise_data, extrinsics, file_path):
    """``write_bundle_adjust_problem`` (bundle_adjust_io.py:193-259): one 3-D point per match (no track merging), two
    observations each, confidences normalised to sum 2, intrinsics folded into the observations (header says f=1, c=0)."""
    if extrinsics.ndim != 3:
        extrinsics = np.array([np.eye(4) for _ in range(n_images)])
    pw = pair_wise_data
    cam_ids, pt_ids, obs, points = [], [], [], []
    n_pts = 0
    for i, j in _pairs(n_images):
        k0 = _key("mkpts", str(i), i, j)
        if k0 not in pw or pw[_key("inlier_count", i, j)] < 0:
            continue
        xy = []
        for v in (i, j):  # pixel -> normalised camera coordinates (in the keypoints' dtype, like the reference)
            K = pw["intr" + str(v)]
            xy.append((pw[_key("mkpts", str(v), i, j)] - K[[0, 1], [2, 2]][None]) / K[[0, 1], [0, 1]][None])
        m = xy[0].shape[0]
        X = triangulate_points(extrinsics[i, :3, :], extrinsics[j, :3, :], xy[0], xy[1]) if m else np.zeros((0, 3))
        for v, x in zip((i, j), xy):
            cam_ids.append(np.full(m, v, dtype=int))
            pt_ids.append(np.arange(n_pts, n_pts + m, dtype=int))
            obs.append(np.concatenate((x, pw[_key("conf", str(v), i, j)]), -1))
        n_pts += m
        points.append(X)
    cam_ids, pt_ids = np.concatenate(cam_ids, 0), np.concatenate(pt_ids, 0)
    obs = normalize_confidences(np.concatenate(obs, 0))
    if obs.shape[1] not in (3, 4):
        logging.error("Unexpected number of confidence values")
    lines = [_csv([n_images, 0, n_pts, 2 * n_pts, 1., 1., 0., 0.])]  # header: cameras, fixed camera, points, observations, f, c
    lines += [_csv([c, q] + list(o)) for c, q, o in zip(cam_ids, pt_ids, obs)]  # 5 / 6 fields, ba_problem.cpp:42-69
    lines += [_csv(_colmajor(extrinsics[v][:3, :3]) + list(extrinsics[v][:3, 3])) for v in range(n_images)]  # 12 fields
    lines += [_csv(X) for X in np.concatenate(points, 0)]  # 3 fields
    with open(file_path, "w") as f:
        f.writelines(lines)


def read_bundle_adjust_result(file_path):
    """``read_bundle_adjust_result`` (bundle_adjust_io.py:261-273): rows of column-major R + t -> list of 4x4 world-to-camera."""
    out = []
    for row in np.loadtxt(file_path, delimiter=",", ndmin=2):
        T = np.eye(4)
        T[:3, :3] = row[:9].reshape(3, 3).T
        T[:3, 3] = row[9:12]
        out.append(T)
    return out


def run_ba_initializer(directory):
    """The reference's ``ba_initializer <dir>`` (ba_initializer.cpp:7-23): ``<dir>/ba_init_in.csv`` -> ``ba_init_out.csv``."""
    lib = _lib.load_library()
    rc = lib.e2emv_mv_init_files(os.path.join(directory, "ba_init_in.csv").encode(), os.path.join(directory, "ba_init_out.csv").encode())
    if rc != 0:
        raise _lib.E2EMVError(rc, "ba_initializer failed on " + directory)


def run_bundle_adjuster(directory):
    """The reference's ``bundle_adjuster <dir>`` (bundle_adjuster.cpp:7-23): ``<dir>/ba_in.csv`` -> ``ba_out.csv``."""
    dev = _dev()
    ctx = _lib.context(dev)
    ctx.call("e2emv_mv_bundle_adjust_files", os.path.join(directory, "ba_in.csv").encode(), os.path.join(directory, "ba_out.csv").encode(),
             _lib.stream_ptr(dev))


def bundle_adjust(n_cams, fixed_cam, intr, cam_idx, pt_idx, obs_xy, obs_w, cams, pts, max_iterations=50, loss=None, loss_scale=None):
    """In-memory form of the device solver (``e2emv_mv_bundle_adjust``); returns ``(cams, pts, summary)``.
    ``loss``: ``None`` (default, the reference's squared loss), "huber" or "cauchy" with ``loss_scale`` = the scale ``a`` of the
    ``ceres::LossFunction`` in the units of the WEIGHTED residual (the batch of one of ``bundle_adjust_batch``); the costs of the
    summary are then ``1/2 sum rho``.  ``ValueError`` for another name, a loss without a scale, a scale without a loss, or a scale
    that is not a finite positive number."""
    if _check_loss(loss, loss_scale):
        return bundle_adjust_batch([(n_cams, fixed_cam, intr, cam_idx, pt_idx, obs_xy, obs_w, cams, pts)], max_iterations, loss, loss_scale)[0]
    dev = _dev()
    ctx = _lib.context(dev)
    cam_idx, pt_idx = np.ascontiguousarray(cam_idx, np.int32), np.ascontiguousarray(pt_idx, np.int32)
    obs_xy, obs_w = np.ascontiguousarray(obs_xy, np.float64), np.ascontiguousarray(obs_w, np.float64)
    cams, pts = np.array(cams, np.float64).reshape(-1, 6).copy(), np.array(pts, np.float64).reshape(-1, 3).copy()
    intr = np.ascontiguousarray(intr, np.float64)
    summary = np.zeros(4)
    ctx.call("e2emv_mv_bundle_adjust", int(n_cams), int(fixed_cam), len(pts), len(cam_idx), _p(intr), _p(cam_idx), _p(pt_idx), _p(obs_xy),
             _p(obs_w), _p(cams), _p(pts), int(max_iterations), _p(summary), _lib.stream_ptr(dev))
    return cams, pts, _ba_summary(summary)


def _ba_summary(summary):
    names = ["max_iterations", "gradient_tolerance", "parameter_tolerance", "function_tolerance", "invalid_steps", "radius"]
    return dict(initial_cost=summary[0], final_cost=summary[1], iterations=int(summary[2]), termination=names[int(summary[3])])


def bundle_adjust_batch(problems, max_iterations=50, loss=None, loss_scale=None):
    """Many bundle adjustments in ONE kernel launch, one workgroup each (``e2emv_mv_bundle_adjust_batch``).  ``problems``: list
    of the argument tuples of ``bundle_adjust`` ``(n_cams, fixed_cam, intr, cam_idx, pt_idx, obs_xy, obs_w, cams, pts)``; they
    may differ in every size, have no point, or cameras without observations.  Returns one ``(cams, pts, summary)`` per problem,
    bit for bit what ``bundle_adjust`` returns for it alone.  ``loss``, ``loss_scale``: as in ``bundle_adjust``, one loss and one
    absolute scale for the batch (``e2emv_mv_bundle_adjust_batch_loss``)."""
    code = _check_loss(loss, loss_scale)
    if not problems:
        return []
    dev = _dev()
    ctx = _lib.context(dev)
    n = len(problems)
    cat = lambda k, dt, w: np.ascontiguousarray(np.concatenate([np.asarray(pr[k], dt).reshape(-1, w) for pr in problems]))  # noqa: E731
    n_cams, fixed = np.array([pr[0] for pr in problems], np.int32), np.array([pr[1] for pr in problems], np.int32)
    intr, cam_idx, pt_idx = cat(2, np.float64, 4), cat(3, np.int32, 1), cat(4, np.int32, 1)
    obs_xy, obs_w, cams, pts = cat(5, np.float64, 2), cat(6, np.float64, 2), cat(7, np.float64, 6), cat(8, np.float64, 3)
    size = lambda k, w: [np.asarray(pr[k]).size // w for pr in problems]  # noqa: E731
    if size(7, 6) != list(n_cams) or size(4, 1) != size(3, 1) or size(5, 2) != size(3, 1) or size(6, 2) != size(3, 1):
        raise ValueError("bundle_adjust_batch: a problem's arrays disagree in length")
    pt_off = np.concatenate([[0], np.cumsum(size(8, 3))]).astype(np.int64)
    obs_off = np.concatenate([[0], np.cumsum(size(3, 1))]).astype(np.int64)
    summary = np.zeros((n, 4))
    head = (n, _p(n_cams), _p(fixed), _p(intr), _p(pt_off), _p(obs_off), _p(cam_idx), _p(pt_idx), _p(obs_xy), _p(obs_w), _p(cams), _p(pts),
            int(max_iterations), _p(summary))
    if code:
        ctx.call("e2emv_mv_bundle_adjust_batch_loss", *head, code, float(loss_scale), _lib.stream_ptr(dev))
    else:
        ctx.call("e2emv_mv_bundle_adjust_batch", *head, _lib.stream_ptr(dev))
    cam_off = np.concatenate([[0], np.cumsum(n_cams)])
    return [(cams[cam_off[k]:cam_off[k + 1]].copy(), pts[pt_off[k]:pt_off[k + 1]].copy(), _ba_summary(summary[k])) for k in range(n)]


def _check_iterations(who, max_iterations):
    if isinstance(max_iterations, bool) or not isinstance(max_iterations, (int, np.integer)) or max_iterations < 0:
        raise ValueError(f"{who}: max_iterations must be an integer >= 0 (got {max_iterations!r})")
    return int(max_iterations)


def bundle_adjust_batch_backward(problems, grads, max_iterations=50):
    """The reverse pass of ``bundle_adjust_batch`` (squared loss; ``e2emv_mv_bundle_adjust_batch_backward``, one launch for the batch).
    ``problems``: the argument of ``bundle_adjust_batch`` (the START cameras and points); ``grads[k] = (g_cams [C,6], g_pts [P,3] or
    None)`` = dLoss/d(what ``bundle_adjust_batch`` returned for problem k).  Returns one ``(g_obs_w [O,2], g_cams0 [C,6], g_pts0 [P,3])``
    per problem, numpy float64: the exact adjoint of the loop the device ran, its decisions, radius and Jacobi scales frozen.
    ``ValueError`` before any device call for arrays that disagree in length, a ``grads`` entry of the wrong shape and a negative or
    non-integer ``max_iterations``."""
    max_iterations = _check_iterations("bundle_adjust_batch_backward", max_iterations)
    if len(grads) != len(problems):
        raise ValueError(f"bundle_adjust_batch_backward: {len(problems)} problems but {len(grads)} grads entries")
    if not problems:
        return []
    n = len(problems)
    cat = lambda k, dt, w: np.ascontiguousarray(np.concatenate([np.asarray(pr[k], dt).reshape(-1, w) for pr in problems]))  # noqa: E731
    n_cams, fixed = np.array([pr[0] for pr in problems], np.int32), np.array([pr[1] for pr in problems], np.int32)
    intr, cam_idx, pt_idx = cat(2, np.float64, 4), cat(3, np.int32, 1), cat(4, np.int32, 1)
    obs_xy, obs_w, cams, pts = cat(5, np.float64, 2), cat(6, np.float64, 2), cat(7, np.float64, 6), cat(8, np.float64, 3)
    size = lambda k, w: [np.asarray(pr[k]).size // w for pr in problems]  # noqa: E731
    if size(7, 6) != list(n_cams) or size(4, 1) != size(3, 1) or size(5, 2) != size(3, 1) or size(6, 2) != size(3, 1):
        raise ValueError("bundle_adjust_batch_backward: a problem's arrays disagree in length")
    g_cams, g_pts = [], []
    for k, (g, C, P) in enumerate(zip(grads, size(7, 6), size(8, 3))):
        if len(g) != 2:
            raise ValueError(f"bundle_adjust_batch_backward: grads[{k}] must be a pair (g_cams, g_pts or None)")
        gc = np.asarray(g[0], np.float64)
        gp = np.zeros((P, 3)) if g[1] is None else np.asarray(g[1], np.float64)
        if gc.shape != (C, 6) or gp.shape != (P, 3):
            raise ValueError(f"bundle_adjust_batch_backward: grads[{k}] must be (g_cams [{C},6], g_pts [{P},3] or None)")
        g_cams.append(gc); g_pts.append(gp)
    g_cams, g_pts = np.ascontiguousarray(np.concatenate(g_cams)), np.ascontiguousarray(np.concatenate(g_pts))
    pt_off = np.concatenate([[0], np.cumsum(size(8, 3))]).astype(np.int64)
    obs_off = np.concatenate([[0], np.cumsum(size(3, 1))]).astype(np.int64)
    cam_off = np.concatenate([[0], np.cumsum(n_cams)])
    g_w, g_c0, g_p0 = np.zeros_like(obs_w), np.zeros_like(cams), np.zeros_like(pts)
    dev = _dev()
    ctx = _lib.context(dev)
    ctx.call("e2emv_mv_bundle_adjust_batch_backward", n, _p(n_cams), _p(fixed), _p(intr), _p(pt_off), _p(obs_off), _p(cam_idx), _p(pt_idx),
             _p(obs_xy), _p(obs_w), _p(cams), _p(pts), max_iterations, _p(g_cams), _p(g_pts), _p(g_w), _p(g_c0), _p(g_p0), _lib.stream_ptr(dev))
    return [(g_w[obs_off[k]:obs_off[k + 1]].copy(), g_c0[cam_off[k]:cam_off[k + 1]].copy(), g_p0[pt_off[k]:pt_off[k + 1]].copy()) for k in range(n)]


class _BundleAdjust(torch.autograd.Function):
    """``bundle_adjust`` forward, ``bundle_adjust_batch_backward`` for the graph (both on host arrays: the solver's interface)."""

    @staticmethod
    def forward(ctx, obs_w, cams, pts, head, max_iterations):
        n_cams, fixed_cam, intr, cam_idx, pt_idx, obs_xy = head
        w, c, p = (t.detach().cpu().numpy() for t in (obs_w, cams, pts))
        ctx.problem = (n_cams, fixed_cam, intr, cam_idx, pt_idx, obs_xy, w, c, p)
        ctx.max_iterations = max_iterations
        ctx.like = [(t.shape, t.device, t.dtype) for t in (obs_w, cams, pts)]
        co, po, _ = bundle_adjust(*ctx.problem, max_iterations=max_iterations)
        return torch.from_numpy(co), torch.from_numpy(po)

    @staticmethod
    def backward(ctx, g_cams, g_pts):
        gw, gc, gp = bundle_adjust_batch_backward([ctx.problem], [(g_cams.detach().cpu().numpy(), g_pts.detach().cpu().numpy())], ctx.max_iterations)[0]
        back = lambda g, t: torch.from_numpy(g).reshape(t[0]).to(t[1], t[2])  # noqa: E731
        need = ctx.needs_input_grad
        return tuple(back(g, t) if need[i] else None for i, (g, t) in enumerate(zip((gw, gc, gp), ctx.like))) + (None, None)


def bundle_adjust_torch(n_cams, fixed_cam, intr, cam_idx, pt_idx, obs_xy, obs_w, cams, pts, max_iterations=50, loss=None, loss_scale=None):
    """``bundle_adjust`` on tensors: returns ``(cams_out [C,6], pts_out [P,3])`` float64 and carries a graph to whichever of ``obs_w``,
    ``cams``, ``pts`` requires grad (``e2emv_mv_bundle_adjust_batch_backward``: the exact adjoint of the LM loop the device ran, squared
    loss only).  Without a graph it returns what ``bundle_adjust`` returns, bit for bit - with a loss too.  ``NotImplementedError`` for a
    graph together with ``loss="huber" | "cauchy"``; ``ValueError`` as ``bundle_adjust_batch_backward``; both before any device call."""
    max_iterations = _check_iterations("bundle_adjust_torch", max_iterations)
    code = _check_loss(loss, loss_scale)
    tens = [torch.as_tensor(t) for t in (obs_w, cams, pts)]
    graph = torch.is_grad_enabled() and any(t.requires_grad for t in tens)
    if graph and code:
        raise NotImplementedError("bundle_adjust_torch: no gradient through a robust loss (loss=%r): the backward pass is that of the squared loss" % (loss,))
    O = np.asarray(cam_idx).size
    if np.asarray(pt_idx).size != O or np.asarray(obs_xy).size != 2 * O or tens[0].numel() != 2 * O or tens[1].numel() != 6 * int(n_cams) or tens[2].numel() % 3:
        raise ValueError("bundle_adjust_torch: the problem's arrays disagree in length")
    if not graph:
        co, po, _ = bundle_adjust(n_cams, fixed_cam, intr, cam_idx, pt_idx, obs_xy, *(t.detach().cpu().numpy() for t in tens), max_iterations=max_iterations,
                                  loss=loss, loss_scale=loss_scale)
        return torch.from_numpy(co), torch.from_numpy(po)
    head = (int(n_cams), int(fixed_cam), np.asarray(intr, np.float64), np.asarray(cam_idx, np.int32), np.asarray(pt_idx, np.int32), np.asarray(obs_xy, np.float64))
    return _BundleAdjust.apply(tens[0], tens[1], tens[2], head, max_iterations)


class _RefineTuple(torch.autograd.Function):
    """Attaches the graph of ``refine_tuple_poses_batch``: the forward result is computed by the caller; the backward runs
    ``e2emv_mv_tuple_ba_backward`` and ``e2emv_mv_collect_backward``."""

    @staticmethod
    def forward(ctx, state, *confs):
        ctx.state = state
        ctx.meta = [(c.shape, c.dtype, c.device) for c in confs]
        return torch.from_numpy(state["out"])

    @staticmethod
    def backward(ctx, g):
        st = ctx.state
        inp, collected = st["inp"], st["collected"]
        dev, B, N = inp["dev"], inp["B"], inp["N"]
        g = np.ascontiguousarray(g.detach().cpu().numpy(), np.float64)
        gm = torch.zeros_like(collected[2])
        _tuple_ba_call("e2emv_mv_tuple_ba_backward", st["tuple_size"], collected, st["counts"], st["intr"], st["kdim"], st["nb"], st["start"],
                       st["max_iterations"], _p(g), _lib.ptr(gm))
        gouts = [None if c is None else torch.empty_like(c) for c in inp["cs"]]
        ptrs = [_lib.ptr_array(lst) for lst in (inp["ms"], inp["cs"], gouts)]
        with torch.cuda.device(dev):
            _lib.context(dev).call("e2emv_mv_collect_backward", B, st["tuple_size"], N, _p(inp["n1"]), ptrs[0][0], ptrs[1][0], inp["channels"],
                                   float(st["conf_thresh"]), _lib.ptr(gm), ptrs[2][0], _lib.stream_ptr(dev))
        have = [go for go in gouts if go is not None]
        return (None,) + tuple(go.reshape(shape).to(device, dtype) for go, (shape, dtype, device) in zip(have, ctx.meta))


class _RefineTupleTracks(torch.autograd.Function):
    """Attaches the graph of ``refine_tuple_poses_batch(..., tracks=True)``: the forward result is computed by the caller; the backward
    runs ``e2emv_mv_tuple_ba_tracks_backward`` on the labels and counts the forward ran with."""

    @staticmethod
    def forward(ctx, state, *confs):
        ctx.state = state
        ctx.meta = [(c.shape, c.dtype, c.device) for c in confs]
        return torch.from_numpy(state["out"])

    @staticmethod
    def backward(ctx, g):
        st = ctx.state
        inp = st["inp"]
        g = np.ascontiguousarray(g.detach().cpu().numpy(), np.float64)
        gouts = [None if c is None else torch.empty_like(c) for c in inp["conf"]]
        pg, owner = _lib.ptr_array(gouts)
        _tracks_entry_call("e2emv_mv_tuple_ba_tracks_backward", st["tuple_size"], inp, st["label"], st["stats"], st["conf_thresh"], st["intr"],
                           st["kdim"], st["nb"], st["start"], st["max_iterations"], _p(g), pg)
        del owner
        have = [go for go in gouts if go is not None]
        return (None,) + tuple(go.reshape(shape).to(device, dtype) for go, (shape, dtype, device) in zip(have, ctx.meta))


def _refine_tuple_tracks(tuple_size, data, result, start, conf_thresh, max_iterations, repair_rounds):
    inp, label, stats = _tracks_labels(tuple_size, data, result, conf_thresh, repair_rounds)
    if len(start) != inp["B"]:
        raise ValueError(f"refine_tuple_poses_batch: {len(start)} start tuples for a batch of {inp['B']}")
    intr, kdim, nb = _tuple_intrinsics(tuple_size, data, inp["dev"], inp["B"])
    out, summary = np.zeros_like(start), np.zeros((len(start), 4))
    _tracks_entry_call("e2emv_mv_tuple_ba_tracks", tuple_size, inp, label, stats, conf_thresh, intr, kdim, nb, start, max_iterations, _p(out),
                       _p(summary))
    confs = [result[_key("conf_scores_", i, j)] for (i, j), c in zip(_pairs(tuple_size), inp["conf"]) if c is not None]
    if not (torch.is_grad_enabled() and any(c.requires_grad for c in confs)):
        return torch.from_numpy(out)
    state = dict(out=out, inp=inp, label=label, stats=stats, intr=intr, kdim=kdim, nb=nb, start=start, tuple_size=tuple_size,
                 conf_thresh=conf_thresh, max_iterations=max_iterations)
    return _RefineTupleTracks.apply(state, *confs)


def refine_tuple_poses_batch(tuple_size, data, result, extrinsics, conf_thresh=0., max_iterations=50, tracks=False, repair_rounds=0):
    """The last stage of ``solve_tuple_poses_batch`` from given start poses, with a graph: ``extrinsics`` [B,T,4,4] world-to-camera start
    (a constant; the DLT start points made from it are constants too) -> the bundle-adjusted extrinsics, ``float64 [B,T,4,4]`` on the
    host, differentiable with respect to every ``conf_scores_{i}_{j}`` of ``result`` that requires grad (squared loss).
    ``tracks=False`` (default), the pair route: ``e2emv_mv_collect`` + ``e2emv_mv_tuple_ba`` forward, ``e2emv_mv_tuple_ba_backward`` +
    ``e2emv_mv_collect_backward`` backward: the gradient reaches channel 0 of the rows ``conf_thresh`` keeps, everything else gets 0.
    ``tracks=True``, the track route (needs per-image ``keypoints{t}``, as in ``solve_tuple_poses_batch``): the labels of
    ``match_tracks(..., repair_rounds=)`` are computed once, ``e2emv_mv_tuple_ba_tracks`` runs on them and
    ``e2emv_mv_tuple_ba_tracks_backward`` reverses it ON THE SAME LABELS: labels, keep rule and cuts are frozen; the gradient reaches
    channel 0 of every kept edge whose two keypoints lie in one track (a cut edge inside its final track included), everything else -
    dropped conflicts, edges between two tracks, rows the threshold drops, the other channels - gets exactly 0.
    Without a graph it returns what that last stage returns for the same start.  ``ValueError``, before any device call, for a start of
    another shape, a negative or non-integer ``max_iterations``, ``tracks=True`` without ``keypoints{t}``, and a ``repair_rounds``
    outside 0 .. 64 or non-zero without ``tracks``."""
    max_iterations = _check_iterations("refine_tuple_poses_batch", max_iterations)
    _check_repair_rounds(repair_rounds, tracks)
    if tracks:
        _check_tracks(tuple_size, data)
    start = np.ascontiguousarray(extrinsics.detach().cpu().numpy() if torch.is_tensor(extrinsics) else extrinsics, np.float64)
    if start.ndim != 4 or start.shape[1:] != (tuple_size, 4, 4):
        raise ValueError(f"refine_tuple_poses_batch: extrinsics must be [B,{tuple_size},4,4] (got {start.shape})")
    if tracks:
        return _refine_tuple_tracks(tuple_size, data, result, start, conf_thresh, max_iterations, repair_rounds)
    inp = _collect_inputs(tuple_size, data, result)
    if len(start) != inp["B"]:
        raise ValueError(f"refine_tuple_poses_batch: {len(start)} start tuples for a batch of {inp['B']}")
    collected = _collect_call(tuple_size, inp, conf_thresh)
    counts = collected[3].cpu().numpy()
    intr, kdim, nb = _tuple_intrinsics(tuple_size, data, inp["dev"], inp["B"])
    out, summary = np.zeros_like(start), np.zeros((len(start), 4))
    _tuple_ba_call("e2emv_mv_tuple_ba", tuple_size, collected, counts, intr, kdim, nb, start, max_iterations, _p(out), _p(summary))
    confs = [result[_key("conf_scores_", i, j)] for (i, j), c in zip(inp["pairs"], inp["cs"]) if c is not None]
    if not (torch.is_grad_enabled() and any(c.requires_grad for c in confs)):
        return torch.from_numpy(out)
    state = dict(out=out, inp=inp, collected=collected, counts=counts, intr=intr, kdim=kdim, nb=nb, start=start, tuple_size=tuple_size,
                 conf_thresh=conf_thresh, max_iterations=max_iterations)
    return _RefineTuple.apply(state, *confs)


def solve_tuple_poses(tuple_size, data, result, tmp_dir, rel_pose_method="w8pt_ba"):
    """Pairwise poses (``rel_pose_method`` as in ``initialize_bundle_adjust``) -> averaging -> weighted bundle adjustment for
    one tuple through the reference's four CSV files in ``tmp_dir``; returns the refined world-to-camera extrinsics
    [tuple_size,4,4]."""
    os.makedirs(tmp_dir, exist_ok=True)
    path = lambda name: os.path.join(tmp_dir, name)  # noqa: E731
    pair_wise_data = initialize_bundle_adjust(tuple_size, data, result, path("ba_init_in.csv"), rel_pose_method=rel_pose_method)
    run_ba_initializer(tmp_dir)
    start = np.array(read_bundle_adjust_result(path("ba_init_out.csv")))
    write_bundle_adjust_problem(tuple_size, pair_wise_data, start, path("ba_in.csv"))
    run_bundle_adjuster(tmp_dir)
    return np.array(read_bundle_adjust_result(path("ba_out.csv")))


def _collect_matches_batch(tuple_size, data, result, conf_thresh):
    """``_collect_matches`` for every batch element at once and on the device (``e2emv_mv_collect``): returns ``(mkpts0, mkpts1
    [B*P,N,2], conf [B*P,N], count [B*P] int32)`` device tensors, problem (b, pair q) at row ``b * P + q``, the kept matches in
    ascending keypoint order, rows behind the count zero.  A pair without a ``matches`` entry has count 0."""
    return _collect_call(tuple_size, _collect_inputs(tuple_size, data, result), conf_thresh)


def _collect_inputs(tuple_size, data, result):
    """What ``e2emv_mv_collect`` and ``e2emv_mv_collect_backward`` read: per pair the keypoints, matches and confidences as contiguous
    device tensors (``None`` for a pair without a ``matches`` entry), the keypoint counts of the second images and the shapes."""
    pairs = _pairs(tuple_size)
    keys = [_key("matches", str(i), i, j) for i, j in pairs]
    have = [k for k in keys if k in result]
    if not have:
        raise ValueError("no pair of the tuple has matches")
    dev = result[have[0]].device
    if dev.type != "cuda":
        dev = _dev()
    B, N = result[have[0]].shape[:2]
    prep = lambda t, dt: t.to(dev, dt).contiguous()  # noqa: E731
    k0s, k1s, ms, cs, n1, channels = [], [], [], [], [], None
    for (i, j), mkey in zip(pairs, keys):
        if mkey not in result:
            k0s.append(None); k1s.append(None); ms.append(None); cs.append(None); n1.append(0)
            continue
        if "keypoints" + str(i) in data:
            k0, k1 = data["keypoints" + str(i)], data["keypoints" + str(j)]
        else:
            k0, k1 = data[_key("keypoints", str(i), i, j)], data[_key("keypoints", str(j), i, j)]
        m, c = prep(result[mkey], torch.int64), prep(result[_key("conf_scores_", i, j)], torch.float32)
        c = c.reshape(B, N, -1)
        k0, k1 = prep(k0, torch.float32), prep(k1, torch.float32)
        if m.shape != (B, N) or k0.shape != (B, N, 2) or k1.shape[0] != B or k1.shape[2] != 2 or (channels not in (None, c.shape[2])):
            raise ValueError("matches / keypoints / conf_scores of pair {} disagree in shape".format((i, j)))
        channels = c.shape[2]
        k0s.append(k0); k1s.append(k1); ms.append(m); cs.append(c); n1.append(k1.shape[1])
    return dict(dev=dev, B=B, N=N, pairs=pairs, k0s=k0s, k1s=k1s, ms=ms, cs=cs, n1=np.array(n1, np.int32), channels=channels)


def _collect_call(tuple_size, inp, conf_thresh):
    dev, B, N, pairs, k0s, k1s, ms, cs, n1, channels = (inp[k] for k in ("dev", "B", "N", "pairs", "k0s", "k1s", "ms", "cs", "n1", "channels"))
    ctx = _lib.context(dev)
    Pn = B * len(pairs)
    o0 = torch.empty((Pn, N, 2), dtype=torch.float32, device=dev)
    o1, oc = torch.empty_like(o0), torch.empty((Pn, N), dtype=torch.float32, device=dev)
    count = torch.empty((Pn,), dtype=torch.int32, device=dev)
    ptrs = [_lib.ptr_array(lst) for lst in (k0s, k1s, ms, cs)]  # (pointer, owner) pairs: the owners live until the call returns
    with torch.cuda.device(dev):
        ctx.call("e2emv_mv_collect", B, tuple_size, N, ptrs[0][0], ptrs[1][0], _p(n1), ptrs[2][0], ptrs[3][0], channels, float(conf_thresh),
                 _lib.ptr(o0), _lib.ptr(o1), _lib.ptr(oc), _lib.ptr(count), _lib.stream_ptr(dev))
    return o0, o1, oc, count


def _tuple_intrinsics(tuple_size, data, dev, B):
    """``data["intr{v}"]`` of every image as contiguous float32 device tensors [nb,k,k] with one common layout."""
    intr = [data["intr" + str(v)].to(dev, torch.float32) for v in range(tuple_size)]
    intr = [(K.unsqueeze(0) if K.dim() == 2 else K).contiguous() for K in intr]
    kdim, nb = intr[0].shape[-1], intr[0].shape[0]
    if kdim not in (3, 4) or nb not in (1, B) or any(K.shape != (nb, kdim, kdim) for K in intr):
        raise ValueError("the intrinsics of a tuple must share one [1 | B, k, k] layout, k = 3 or 4")
    return intr, kdim, nb


def _tuple_ba_call(name, tuple_size, collected, counts, intr, kdim, nb, extrinsics, *tail):
    o0, o1, oc, _ = collected
    dev = o0.device
    pa, owner = _lib.ptr_array(intr)
    with torch.cuda.device(dev):
        _lib.context(dev).call(name, len(extrinsics), tuple_size, o0.shape[1], _p(counts), _lib.ptr(o0), _lib.ptr(o1), _lib.ptr(oc), pa, kdim, nb,
                               _p(extrinsics), *tail, _lib.stream_ptr(dev))
    del owner


def _tuple_init_on_device(tuple_size, T_d, inl, count, min_matches=8, min_inliers=20):
    """The initialisation stage on the device (``e2emv_mv_tuple_init``), enqueued behind the relative-pose stage on the current
    stream: ``T_d`` [B*P,4,4] float32, ``inl`` [B*P,N] uint8, ``count`` [B*P] int32 device tensors -> ``(extrinsics [B,T,4,4],
    counts [B*P] int32)`` on the host, brought back by ONE device-to-host copy (which is the only synchronisation).  The status
    words stay on the device: a failed averaging is not raised on the host path either."""
    return _tuple_init_launch(tuple_size, T_d, inl.sum(1, dtype=torch.int32).contiguous(), count, count, min_matches, min_inliers)


def _tuple_init_launch(tuple_size, T_d, n_inl, weight, ba_count, min_matches, min_inliers):
    """``e2emv_mv_tuple_init`` on ``T_d`` [B*P,4,4] float32, ``n_inl`` and ``weight`` [B*P] int32 (a pair is an edge of the match
    graph iff ``weight >= min_matches``); ``ba_count`` [B*P] int32 rides along in the one copy that brings the start extrinsics
    back.  Returns ``(extrinsics [B,T,4,4], ba_count)`` on the host."""
    dev = T_d.device
    P = len(_pairs(tuple_size))
    B = T_d.shape[0] // P
    extr = torch.empty((B, tuple_size * 16), dtype=torch.float64, device=dev)
    status = torch.empty((B,), dtype=torch.int32, device=dev)
    T_d, weight = T_d.contiguous(), weight.contiguous()
    with torch.cuda.device(dev):
        _lib.context(dev).call("e2emv_mv_tuple_init", B, tuple_size, _lib.ptr(T_d), _lib.ptr(n_inl), _lib.ptr(weight), int(min_matches),
                               int(min_inliers), _lib.ptr(extr), _lib.ptr(status), _lib.stream_ptr(dev))
    packed = torch.cat([extr, ba_count.reshape(B, P).double()], 1).cpu().numpy()
    start = np.ascontiguousarray(packed[:, :tuple_size * 16]).reshape(B, tuple_size, 4, 4)
    return start, np.ascontiguousarray(packed[:, tuple_size * 16:].astype(np.int32).reshape(-1))


def _ransac_on_device(tuple_size, collected, intr, kdim, nb, ba=False, seed=0, loss=None, loss_scale=None):
    """The launch sequence behind the "ransac" / "ransac_ba" relative poses of a batch of tuples, on the buffers of
    ``_collect_matches_batch`` and the intrinsics of ``_tuple_intrinsics``, nothing read back: ``e2emv_mv_ransac_prepare`` (fp64
    normalised keypoints, thresholds) -> ``e2emv_essential_ransac`` (threshold 1 pixel, conf 0.99999, 1000 iterations, as
    ``relative_poses_ransac``) -> ``e2emv_mv_ransac_filter`` (matches reduced to the inliers, pose as 4x4) -> with ``ba`` the
    two-view bundle adjustment of every solved pair on its inliers, 10 iterations started from the RANSAC pose
    (``e2emv_ba_2view`` directly: it returns the start of a pair it declares invalid, which is ``T[ok] = refined`` without the
    host's boolean indexing and its synchronisation; with ``loss`` / ``loss_scale``, which need ``ba``, ``e2emv_ba_2view_loss`` with
    that robust loss).  Per pair what ``relative_poses_ransac`` computes, bit for bit.  Returns a
    dict of device tensors: ``filtered`` (mkpts0, mkpts1 [B*P,N,2], conf [B*P,N]; a pair that was not solved keeps all its
    matches), ``T`` [B*P,4,4] float32 (the identity unless solved), ``ba_count`` (rows in use of ``filtered``), ``graph_w``
    (inliers of a solved pair, else 0) and the stages' own outputs ``kpts0n``, ``kpts1n``, ``thresh``, ``inliers``,
    ``n_inliers``, ``R``, ``t``, ``status``, ``T0``."""
    loss_code = _check_loss(loss, loss_scale)
    if loss_code and not ba:
        raise ValueError("loss={!r} needs ba=True: the RANSAC alone has no two-view bundle adjustment".format(loss))
    o0, o1, oc, count = collected
    dev = o0.device
    ctx = _lib.context(dev)
    Pn, N = o0.shape[:2]
    B = Pn // len(_pairs(tuple_size))
    if N > MAX_MATCHES:
        raise ValueError("the RANSAC relative poses take at most {} keypoints per image (got {})".format(MAX_MATCHES, N))
    new = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)  # noqa: E731
    f32, f64, i32 = torch.float32, torch.float64, torch.int32
    k0n, k1n, th = new((Pn, N, 2), f64), new((Pn, N, 2), f64), new((Pn,), f64)
    E, R, t = new((Pn, 3, 3), f64), new((Pn, 3, 3), f64), new((Pn, 3), f64)
    inl = new((Pn, N), torch.uint8)
    n_inl, n_ch, iters, status, ba_count, graph_w = (new((Pn,), i32) for _ in range(6))
    f0, f1, fc, T0 = new((Pn, N, 2), f32), new((Pn, N, 2), f32), new((Pn, N), f32), new((Pn, 4, 4), f32)
    f0n, f1n, fcn = (new((Pn, N, 2), f32), new((Pn, N, 2), f32), new((Pn, N), f32)) if ba else (None, None, None)
    pa, owner = _lib.ptr_array(intr)
    P, s = _lib.ptr, _lib.stream_ptr(dev)
    with torch.cuda.device(dev):
        ctx.call("e2emv_mv_ransac_prepare", B, tuple_size, N, P(o0), P(o1), P(count), pa, kdim, nb, 1.0, P(k0n), P(k1n), P(th), s)
        ctx.call("e2emv_essential_ransac", Pn, N, P(count), P(k0n), P(k1n), P(th), 0.99999, 1000, int(seed) & 0xFFFFFFFF, P(E), P(R), P(t),
                 P(inl), P(n_inl), P(n_ch), P(iters), P(status), s)
        ctx.call("e2emv_mv_ransac_filter", B, tuple_size, N, P(o0), P(o1), P(oc), P(count), P(k0n), P(k1n), P(inl), P(n_inl), P(R), P(t),
                 P(status), P(f0), P(f1), P(fc), P(f0n), P(f1n), P(fcn), P(T0), P(ba_count), P(graph_w), s)
        T = T0
        if ba:
            T, valid = new((Pn, 4, 4), f32), new((Pn,), torch.uint8)
            if loss_code:
                ctx.call("e2emv_ba_2view_loss", Pn, N, P(f0n), P(f1n), P(fcn), P(T0), 10, P(T), P(valid), loss_code, float(loss_scale), P(None), s)
            else:
                ctx.call("e2emv_ba_2view", Pn, N, P(f0n), P(f1n), P(fcn), P(T0), 10, P(T), P(valid), s)
    del owner
    return dict(filtered=(f0, f1, fc), T=T, ba_count=ba_count, graph_w=graph_w, kpts0n=k0n, kpts1n=k1n, thresh=th, inliers=inl,
                n_inliers=n_inl, R=R, t=t, status=status, T0=T0)


def _check_tracks(tuple_size, data, rel_pose_method="w8pt_ba"):
    """What ``tracks=True`` needs, checked on the host before any device call."""
    if rel_pose_method != "w8pt_ba":
        raise ValueError("tracks=True needs rel_pose_method=\"w8pt_ba\" (got {!r}): the RANSAC methods filter compacted rows that no "
                         "longer carry keypoint indices".format(rel_pose_method))
    missing = [t for t in range(tuple_size) if "keypoints" + str(t) not in data]
    if missing:
        raise ValueError("tracks=True needs the per-image keypoints{{t}} in data (missing for images {}): with per-pair keypoints "
                         "only, a keypoint has no identity across pairs".format(missing))


def _check_repair_rounds(repair_rounds, tracks=True):
    """``repair_rounds`` is an int in 0 .. 64 and 0 without tracks, checked on the host before any device call."""
    if isinstance(repair_rounds, bool) or not isinstance(repair_rounds, (int, np.integer)) or not 0 <= repair_rounds <= 64:
        raise ValueError("repair_rounds must be an int in 0 .. 64, not {!r}".format(repair_rounds))
    if repair_rounds and not tracks:
        raise ValueError("repair_rounds={} needs tracks=True: only the track problem has conflicts to repair".format(repair_rounds))


def _track_inputs(tuple_size, data, result):
    """Device arrays of the track entry points: per-image keypoints [B,n_t,2] float32, per pair (order of ``_pairs``) matches [B,N]
    int64 and confidences [B,N,channels] float32 (``None`` for a pair without a ``matches`` entry), ``n1`` = keypoints of every
    pair's second image, ``Nmax`` = ``max(N, n1)`` = the largest keypoint count (every image but the last is the first image of a
    pair, so it has ``N`` keypoints wherever that pair has matches)."""
    _check_tracks(tuple_size, data)
    pairs = _pairs(tuple_size)
    keys = [_key("matches", str(i), i, j) for i, j in pairs]
    have = [k for k in keys if k in result]
    if not have:
        raise ValueError("no pair of the tuple has matches")
    dev = result[have[0]].device
    if dev.type != "cuda":
        dev = _dev()
    B, N = result[have[0]].shape[:2]
    prep = lambda t, dt: t.to(dev, dt).contiguous()  # noqa: E731
    kpts = [prep(data["keypoints" + str(t)], torch.float32) for t in range(tuple_size)]
    if any(k.dim() != 3 or k.shape[0] != B or k.shape[2] != 2 for k in kpts):
        raise ValueError("keypoints{t} must be [B, n, 2]")
    ms, cs, channels = [], [], None
    for (i, j), mkey in zip(pairs, keys):
        if mkey not in result:
            ms.append(None); cs.append(None)
            continue
        m, c = prep(result[mkey], torch.int64), prep(result[_key("conf_scores_", i, j)], torch.float32).reshape(B, N, -1)
        if m.shape != (B, N) or kpts[i].shape[1] != N or (channels not in (None, c.shape[2])):
            raise ValueError("matches / keypoints / conf_scores of pair {} disagree in shape".format((i, j)))
        channels = c.shape[2]
        ms.append(m); cs.append(c)
    n_kpts = np.array([k.shape[1] for k in kpts], np.int32)
    n1 = np.array([n_kpts[j] for _, j in pairs], np.int32)
    return dict(dev=dev, B=B, N=N, Nmax=int(max(N, n1.max())), kpts=kpts, n_kpts=n_kpts, matches=ms, conf=cs, n1=n1, channels=channels)


def match_tracks(tuple_size, data, result, conf_thresh=0., _inputs=None, repair_rounds=0):
    """The pairwise matches of every tuple merged into tracks on the device (``e2emv_mv_tracks``, one launch, no synchronisation).
    Node = keypoint ``n`` of image ``t``, id ``t * Nmax + n`` (``Nmax`` = the largest keypoint count of the tuple's images); edge
    = every match ``_collect_matches_batch`` keeps; a track is a connected component of at least 2 nodes with at most ONE node
    per image (a component with two keypoints of one image is a conflict and is dropped).  Returns ``(label [B, T, Nmax] int32,
    stats [B, 4] int32)`` device tensors: the smallest node id of the node's track, or -1 for a node in no track;
    ``stats[b] = (tracks, observations, conflict components, edges)``.  At most 16384 nodes per tuple (``E2EMVError`` above).
    ``repair_rounds`` (int, 0 .. 64, else ``ValueError``): 0 (default) is the call above.  ``R > 0`` goes to
    ``e2emv_mv_tracks_repair`` (one launch as well): up to ``R`` rounds in each of which EVERY conflicting component loses its
    weakest live edge - smallest confidence of channel 0, then smallest edge id ``q * N + n`` - before the components are taken
    again; it ends early when nothing conflicts.  Labels are then the definitions above over the live edges, ``stats[b]`` counts
    the conflicts LEFT and the LIVE edges."""
    _check_repair_rounds(repair_rounds)
    inp = _inputs or _track_inputs(tuple_size, data, result)
    dev = inp["dev"]
    label = torch.empty((inp["B"], tuple_size, inp["Nmax"]), dtype=torch.int32, device=dev)
    stats = torch.empty((inp["B"], 4), dtype=torch.int32, device=dev)
    pm, pc = _lib.ptr_array(inp["matches"]), _lib.ptr_array(inp["conf"])  # (pointer, owner) pairs
    with torch.cuda.device(dev):
        head = (inp["B"], tuple_size, inp["N"], _p(inp["n1"]), pm[0], pc[0], inp["channels"], float(conf_thresh))
        tail = (_lib.ptr(label), _lib.ptr(stats), _lib.stream_ptr(dev))
        if repair_rounds:
            _lib.context(dev).call("e2emv_mv_tracks_repair", *head, int(repair_rounds), *tail)
        else:
            _lib.context(dev).call("e2emv_mv_tracks", *head, *tail)
    return label, stats


def _tracks_labels(tuple_size, data, result, conf_thresh, repair_rounds=0):
    """``(inp, label, stats)``: the device arrays of ``_track_inputs``, the labels of ``match_tracks`` on them and the one small copy of
    their counts to the host (tracks and observations per tuple lay out the workspace)."""
    _check_repair_rounds(repair_rounds)
    inp = _track_inputs(tuple_size, data, result)
    label, stats_d = match_tracks(tuple_size, data, result, conf_thresh, _inputs=inp, repair_rounds=repair_rounds)
    return inp, label, np.ascontiguousarray(stats_d.cpu().numpy())


def _tracks_entry_call(name, tuple_size, inp, label, stats, conf_thresh, intr, kdim, nb, extrinsics, *tail):
    """The track entry point ``name`` on given labels and counts (forward and backward run on the SAME ones)."""
    dev = inp["dev"]
    extrinsics = np.ascontiguousarray(extrinsics, np.float64)
    pk, pm, pc, pi = (_lib.ptr_array(lst) for lst in (inp["kpts"], inp["matches"], inp["conf"], intr))
    with torch.cuda.device(dev):
        _lib.context(dev).call(name, inp["B"], tuple_size, inp["N"], inp["Nmax"], _lib.ptr(label), _p(stats), pk[0], _p(inp["n_kpts"]), pm[0], pc[0],
                               inp["channels"], float(conf_thresh), pi[0], kdim, nb, _p(extrinsics), *tail, _lib.stream_ptr(dev))


def _tracks_ba_call(name, tuple_size, data, result, conf_thresh, intr, kdim, nb, extrinsics, *tail, repair_rounds=0):
    """Labels (``match_tracks``), the one small copy of their counts to the host, then the track entry point ``name``.  Returns
    ``(label, stats)``, the counts as a host array.  ``repair_rounds``: as in ``match_tracks``; the entry point takes the repaired
    labels like any others (it weighs a node by the KEPT edges between the members of its track, cut or not)."""
    inp, label, stats = _tracks_labels(tuple_size, data, result, conf_thresh, repair_rounds)
    _tracks_entry_call(name, tuple_size, inp, label, stats, conf_thresh, intr, kdim, nb, extrinsics, *tail)
    return label, stats


def _check_init(init):
    if init not in ("host", "device"):
        raise ValueError("init must be \"host\" or \"device\", not {!r}".format(init))


def _check_rel_pose_method(rel_pose_method):
    if rel_pose_method not in ("w8pt_ba", "ransac", "ransac_ba"):
        raise NotImplementedError("relative pose method {} is not defined".format(rel_pose_method))


def _check_pair_loss(pair_loss, pair_loss_scale, rel_pose_method):
    """The loss of the pairwise two-view stage: the rules of ``_check_loss``, and a method that has that stage."""
    if _check_loss(pair_loss, pair_loss_scale) and rel_pose_method == "ransac":
        raise ValueError("pair_loss={!r} needs rel_pose_method \"w8pt_ba\" or \"ransac_ba\": \"ransac\" has no two-view bundle "
                         "adjustment".format(pair_loss))


def solve_tuple_poses_batch(tuple_size, data, result, conf_thresh=0., timings=None, init="host", rel_pose_method="w8pt_ba", seed=0, tracks=False,
                            repair_rounds=0, loss=None, loss_scale=None, pair_loss=None, pair_loss_scale=None):
    """``solve_tuple_poses`` for EVERY batch element of the matcher result, in memory: returns the refined world-to-camera
    extrinsics ``float64 [B, tuple_size, 4, 4]``, camera 0 the gauge.  Stages: matches collected on the device (one launch) ->
    relative poses of all B * T(T-1)/2 pairs (``rel_pose_method``) -> one copy to the host, spanning tree and rotation /
    position averaging per tuple (``e2emv_mv_init``) -> all bundle-adjustment problems built on the device (one launch) and
    solved one workgroup per tuple (one launch).  No file, and no element's result depends on its batch neighbours.
    ``rel_pose_method``: the three of ``initialize_bundle_adjust``.  "w8pt_ba" (default): w8pt + two-view BA; every match goes to
    the bundle adjustment, pairs with at least 8 matches are the edges of the match graph, weighted by their match count.
    "ransac" / "ransac_ba": ``_ransac_on_device`` (``seed``: the RANSAC's sample stream; at most 4096 keypoints per image, else
    ``ValueError``), per pair bit for bit what ``relative_poses_ransac`` gives; the matches of a solved pair are reduced to its
    inliers on the device, the solved pairs are the edges, weighted by their inlier count, and a pair the RANSAC did not solve
    keeps all its matches for the bundle adjustment, as on the CSV path.  Another name raises ``NotImplementedError``.
    ``timings``: optional dict that receives the wall time of each stage in seconds (synchronises after every stage).
    ``init``: where the initialisation stage runs.  "host" (default): the loop above.  "device": ``e2emv_mv_tuple_init``, one
    launch for the batch (one wave per tuple: spanning tree, chained start, averaging) enqueued behind the relative poses; match
    counts and start extrinsics come back in one copy.  Same solver and options; the results agree to rounding (DESIGN.md
    section 1), equal match counts of two pairs of a tuple are ordered by ascending (i, j) there and by scipy here.
    ``tracks``: ``False`` (default): one 3-D point per pairwise match, like the reference.  ``True``: the first three stages stay
    as they are (the start comes from the pairwise relative poses) and the last stage bundle-adjusts the TRACKS of
    ``match_tracks`` - one point per scene point, seen by 2 .. T images; components with two keypoints of one image are dropped -
    built on the device (``e2emv_mv_tuple_ba_tracks``).  A tuple without any track returns its start.  Needs
    ``rel_pose_method="w8pt_ba"`` (the RANSAC methods filter rows that no longer carry keypoint indices) and per-image
    ``keypoints{t}`` in ``data`` (with per-pair keypoints only, a keypoint has no identity across pairs): ``ValueError``
    otherwise, before any device call.
    ``repair_rounds`` (int, 0 .. 64; must be 0 unless ``tracks=True``; ``ValueError`` otherwise, before any device call): 0
    (default) drops the conflicting components as described; ``R > 0`` repairs them first as in ``match_tracks``.
    ``loss``, ``loss_scale``: a robust loss in the last stage only (``None``, the default: the squared loss, the calls above;
    "huber" / "cauchy": ``e2emv_mv_tuple_ba_loss`` / ``e2emv_mv_tuple_ba_tracks_loss``), with either ``init``, every
    ``rel_pose_method`` and ``tracks`` / ``repair_rounds``.  ``loss_scale`` is RELATIVE here: the weights of a tuple are its
    confidences over a per-tuple constant, the scale is divided by the same constant on the device, and the loss acts on
    ``confidence x residual`` in normalised image coordinates - ``loss_scale`` = pixels / focal length at confidence 1 (one
    pixel at f = 600: ``1 / 600``), whatever the tuple's number of matches.  ``ValueError`` as in ``bundle_adjust``, before any
    device call.
    ``pair_loss``, ``pair_loss_scale``: a robust loss in the PAIRWISE stage, the two-view bundle adjustment of "w8pt_ba" and
    "ransac_ba" (``e2emv_ba_2view_loss``, see ``run_bundle_adjust_2_view``), independent of ``loss`` / ``loss_scale``; with
    either ``init`` and with ``tracks`` / ``repair_rounds``.  The scale is relative in the same way, per pair: pixels / focal
    length at confidence 1.  ``None`` (default): the calls above.  "ransac" has no two-view bundle adjustment: a ``pair_loss``
    with it is a ``ValueError``, like every bad loss argument before any device call."""
    import time
    _check_init(init)
    loss_code = _check_loss(loss, loss_scale)
    _check_rel_pose_method(rel_pose_method)
    _check_pair_loss(pair_loss, pair_loss_scale, rel_pose_method)
    _check_repair_rounds(repair_rounds, tracks)
    if tracks:
        _check_tracks(tuple_size, data, rel_pose_method)
    ransac = rel_pose_method != "w8pt_ba"
    # the last stage: without a loss the entry points and arguments it always had
    ba_suffix, loss_tail = ("_loss", (loss_code, float(loss_scale), None)) if loss_code else ("", ())
    pairs = _pairs(tuple_size)
    P = len(pairs)
    clock = [time.perf_counter()]

    def lap(name):
        if timings is not None:
            torch.cuda.synchronize()
            now = time.perf_counter()
            timings[name] = timings.get(name, 0.0) + now - clock[0]
            clock[0] = now

    collected = _collect_matches_batch(tuple_size, data, result, conf_thresh)
    o0, o1, oc, count = collected
    dev = o0.device
    B = o0.shape[0] // P
    lap("collect")
    intr, kdim, nb = _tuple_intrinsics(tuple_size, data, dev, B)
    if ransac:
        # what the later stages see of a pair: its inliers (n_inl, also its weight in the match graph: 0 = not solved, no edge)
        # and the rows the bundle adjustment takes from the filtered buffers
        st = _ransac_on_device(tuple_size, collected, intr, kdim, nb, ba=rel_pose_method == "ransac_ba", seed=seed, loss=pair_loss,
                               loss_scale=pair_loss_scale)
        collected, T_d, n_inl_d, ba_count_d, min_matches = st["filtered"] + (None,), st["T"], st["graph_w"], st["ba_count"], 1
    else:
        per_pair = lambda side: torch.stack([intr[pr[side]].expand(B, kdim, kdim) for pr in pairs], 1).reshape(B * P, kdim, kdim).contiguous()  # noqa: E731
        T_d, inl = _w8pt_ba_on_device(dev, count, o0, o1, oc, per_pair(0), per_pair(1), loss=pair_loss, loss_scale=pair_loss_scale)
        ba_count_d, min_matches = count, 8  # success of estimate_relative_pose_w8pt_ba; the match count is the weight
    if init == "device":
        lap("relative_poses")
        if ransac:
            start, counts = _tuple_init_launch(tuple_size, T_d, n_inl_d, n_inl_d, ba_count_d, min_matches, 20)
        else:
            start, counts = _tuple_init_on_device(tuple_size, T_d, inl, count)
        lap("initialisation")
        out, summary = np.zeros((B, tuple_size, 4, 4)), np.zeros((B, 4))
        if tracks:
            _tracks_ba_call("e2emv_mv_tuple_ba_tracks" + ba_suffix, tuple_size, data, result, conf_thresh, intr, kdim, nb, start, 50, _p(out),
                            _p(summary), *loss_tail, repair_rounds=repair_rounds)
        else:
            _tuple_ba_call("e2emv_mv_tuple_ba" + ba_suffix, tuple_size, collected, counts, intr, kdim, nb, start, 50, _p(out), _p(summary), *loss_tail)
        lap("build_and_bundle_adjust")
        return out
    # one device -> host copy for the whole batch: poses, inlier counts, match counts
    if not ransac:
        n_inl_d = inl.sum(1, dtype=torch.int32)
    packed = torch.cat([T_d.reshape(B * P, 16).double(), n_inl_d.double()[:, None], ba_count_d.double()[:, None]], 1).cpu().numpy()
    lap("relative_poses")
    rel_T, n_inl = packed[:, :16].reshape(B, P, 4, 4), packed[:, 16].astype(np.int64).reshape(B, P)
    counts = np.ascontiguousarray(packed[:, 17].astype(np.int32))
    weight = n_inl if ransac else counts.reshape(B, P)
    start = np.zeros((B, tuple_size, 4, 4))
    for b in range(B):
        graph = np.zeros((tuple_size, tuple_size), dtype=int)
        rel, inlier_count = {}, {}
        for q, (i, j) in enumerate(pairs):
            if weight[b, q] >= min_matches:
                rel[(i, j)], inlier_count[(i, j)] = rel_T[b, q], int(n_inl[b, q])
                graph[i, j] = weight[b, q]
        start[b] = _averaged_extrinsics(*_init_arrays(tuple_size, rel, inlier_count, graph)[0])
    lap("initialisation")
    out, summary = np.zeros((B, tuple_size, 4, 4)), np.zeros((B, 4))
    if tracks:
        _tracks_ba_call("e2emv_mv_tuple_ba_tracks" + ba_suffix, tuple_size, data, result, conf_thresh, intr, kdim, nb, start, 50, _p(out),
                        _p(summary), *loss_tail, repair_rounds=repair_rounds)
    else:
        _tuple_ba_call("e2emv_mv_tuple_ba" + ba_suffix, tuple_size, collected, counts, intr, kdim, nb, start, 50, _p(out), _p(summary), *loss_tail)
    lap("build_and_bundle_adjust")
    return out


def _tuple_problems(tuple_size, collected, counts, intr, kdim, nb, extrinsics):
    """The bundle-adjustment problems ``solve_tuple_poses_batch`` solves (``e2emv_mv_tuple_problem``), one argument tuple of
    ``bundle_adjust`` per batch element: what ``write_bundle_adjust_problem`` writes as text, built on the device."""
    extrinsics = np.ascontiguousarray(extrinsics, np.float64)
    B, P = len(extrinsics), len(_pairs(tuple_size))
    counts = np.ascontiguousarray(counts, np.int32)
    n_pts = counts.reshape(B, P).sum(1)
    tot = int(n_pts.sum())
    cam_idx, pt_idx = np.zeros(2 * tot, np.int32), np.zeros(2 * tot, np.int32)
    obs_xy, obs_w, cams, pts = np.zeros((2 * tot, 2)), np.zeros((2 * tot, 2)), np.zeros((B * tuple_size, 6)), np.zeros((tot, 3))
    _tuple_ba_call("e2emv_mv_tuple_problem", tuple_size, collected, counts, intr, kdim, nb, extrinsics, _p(cam_idx), _p(pt_idx), _p(obs_xy),
                   _p(obs_w), _p(cams), _p(pts))
    off = np.concatenate([[0], np.cumsum(n_pts)])
    return [(tuple_size, 0, np.array([1., 1., 0., 0.]), cam_idx[2 * off[b]:2 * off[b + 1]], pt_idx[2 * off[b]:2 * off[b + 1]],
             obs_xy[2 * off[b]:2 * off[b + 1]], obs_w[2 * off[b]:2 * off[b + 1]], cams[b * tuple_size:(b + 1) * tuple_size], pts[off[b]:off[b + 1]])
            for b in range(B)]


def _tuple_problems_tracks(tuple_size, data, result, conf_thresh, intr, kdim, nb, extrinsics, repair_rounds=0):
    """The track problems ``solve_tuple_poses_batch(..., tracks=True)`` solves (``e2emv_mv_tuple_problem_tracks``): ``(problems,
    label, stats)``, one argument tuple of ``bundle_adjust`` per batch element and what ``match_tracks`` returned (label on the
    device, stats on the host).  ``repair_rounds``: as in ``match_tracks``."""
    _check_repair_rounds(repair_rounds)
    inp = _track_inputs(tuple_size, data, result)
    stats = match_tracks(tuple_size, data, result, conf_thresh, _inputs=inp, repair_rounds=repair_rounds)[1].cpu().numpy()
    B = inp["B"]
    n_pts, n_obs = stats[:, 0].astype(np.int64), stats[:, 1].astype(np.int64)
    tp, to = int(n_pts.sum()), int(n_obs.sum())
    cam_idx, pt_idx = np.zeros(to, np.int32), np.zeros(to, np.int32)
    obs_xy, obs_w, cams, pts = np.zeros((to, 2)), np.zeros((to, 2)), np.zeros((B * tuple_size, 6)), np.zeros((tp, 3))
    label, stats = _tracks_ba_call("e2emv_mv_tuple_problem_tracks", tuple_size, data, result, conf_thresh, intr, kdim, nb, extrinsics, _p(cam_idx),
                                   _p(pt_idx), _p(obs_xy), _p(obs_w), _p(cams), _p(pts), repair_rounds=repair_rounds)
    po, oo = np.concatenate([[0], np.cumsum(n_pts)]), np.concatenate([[0], np.cumsum(n_obs)])
    return [(tuple_size, 0, np.array([1., 1., 0., 0.]), cam_idx[oo[b]:oo[b + 1]], pt_idx[oo[b]:oo[b + 1]], obs_xy[oo[b]:oo[b + 1]],
             obs_w[oo[b]:oo[b + 1]], cams[b * tuple_size:(b + 1) * tuple_size], pts[po[b]:po[b + 1]]) for b in range(B)], label, stats


def tuple_pose_errors(extrinsics, cam_to_world):
    """Angular errors (degrees) of every image pair of a tuple, pairs in ``_pairs`` order: predicted relative pose
    ``E_j inv(E_i)`` against ``inv(pose_j) pose_i``.  Returns ``(err_t [P], err_R [P])`` with upstream's conventions
    (``compute_pose_error``: translation error folded to <= 90 degrees)."""
    pairs = _pairs(len(extrinsics))
    i_idx, j_idx = np.array([p[0] for p in pairs]), np.array([p[1] for p in pairs])
    E, C = np.asarray(extrinsics, np.float64), np.asarray(cam_to_world, np.float64)
    gt = np.linalg.inv(C[j_idx]) @ C[i_idx]
    pred = E[j_idx] @ np.linalg.inv(E[i_idx])
    cos_r = np.clip((np.einsum("pab,pab->p", gt[:, :3, :3], pred[:, :3, :3]) - 1.0) / 2.0, -1.0, 1.0)
    tg, tp = gt[:, :3, 3], pred[:, :3, 3]
    with np.errstate(invalid="ignore", divide="ignore"):  # a zero translation (image without matches) gives nan, as upstream
        cos_t = np.clip(np.einsum("pa,pa->p", tg, tp) / (np.linalg.norm(tg, axis=1) * np.linalg.norm(tp, axis=1)), -1.0, 1.0)
    err_t = np.rad2deg(np.arccos(cos_t))
    return np.minimum(err_t, 180.0 - err_t), np.rad2deg(np.abs(np.arccos(cos_r)))


def eval_bundle_adjust(tuple_size, data, result, tmp_dir, pose_errors, verbose=False, rel_pose_method="w8pt_ba"):
    """``eval_bundle_adjust`` (eval_multi_view.py:21-68): the multi-view back-end for one tuple (batch element 0);
    extends ``pose_errors = [max errors, translation errors, rotation errors]`` by one entry per image pair.
    ``rel_pose_method``: as in ``initialize_bundle_adjust``."""
    extrinsics = solve_tuple_poses(tuple_size, data, result, tmp_dir, rel_pose_method=rel_pose_method)
    err_t, err_R = tuple_pose_errors(extrinsics, [data["pose" + str(v)][0].cpu().numpy() for v in range(tuple_size)])
    pose_errors[0].extend(np.maximum(err_t, err_R))
    pose_errors[1].extend(err_t)
    pose_errors[2].extend(err_R)
    if verbose:
        for (i, j), et, er in zip(_pairs(tuple_size), err_t, err_R):
            logging.info("%d -> %d: rot %5.1fdeg\tt %5.1fdeg", i, j, er, et)
    return pose_errors


def eval_bundle_adjust_batch(tuple_size, data, result, pose_errors, verbose=False, init="host", rel_pose_method="w8pt_ba", tracks=False,
                             repair_rounds=0, loss=None, loss_scale=None, pair_loss=None, pair_loss_scale=None):
    """``eval_bundle_adjust`` for every batch element through ``solve_tuple_poses_batch``: extends ``pose_errors = [max errors,
    translation errors, rotation errors]`` by ``B * T(T-1)/2`` entries, batch element outer, pairs in ``_pairs`` order inside
    (for ``B = 1`` the entries ``eval_bundle_adjust`` appends, in its order).  ``init``, ``rel_pose_method``, ``tracks``,
    ``repair_rounds``, ``loss``, ``loss_scale``, ``pair_loss``, ``pair_loss_scale``: as in ``solve_tuple_poses_batch``."""
    extrinsics = solve_tuple_poses_batch(tuple_size, data, result, init=init, rel_pose_method=rel_pose_method, tracks=tracks,
                                         repair_rounds=repair_rounds, loss=loss, loss_scale=loss_scale, pair_loss=pair_loss,
                                         pair_loss_scale=pair_loss_scale)
    poses = np.stack([data["pose" + str(v)].cpu().numpy() for v in range(tuple_size)], 1)  # [B,T,4,4]: one copy per image
    for b, E in enumerate(extrinsics):
        err_t, err_R = tuple_pose_errors(E, poses[b])
        pose_errors[0].extend(np.maximum(err_t, err_R))
        pose_errors[1].extend(err_t)
        pose_errors[2].extend(err_R)
        if verbose:
            for (i, j), et, er in zip(_pairs(tuple_size), err_t, err_R):
                logging.info("[%d] %d -> %d: rot %5.1fdeg\tt %5.1fdeg", b, i, j, er, et)
    return pose_errors


if __name__ == "__main__":
    if len(sys.argv) != 3 or sys.argv[1] not in ("ba_initializer", "bundle_adjuster"):
        sys.stderr.write("Usage: python -m e2e_multi_view_matching_amd.multi_view {ba_initializer|bundle_adjuster} <path to read and write>\n")
        sys.exit(1)
    (run_ba_initializer if sys.argv[1] == "ba_initializer" else run_bundle_adjuster)(sys.argv[2])
