"""The classical relative-pose baseline of the reference: SuperGlue's ``models/utils.py::estimate_pose`` (OpenCV
``findEssentialMat(RANSAC)`` + ``recoverPose``), computed by ``e2emv_essential_ransac`` (csrc/ransac.hip) for many image
pairs in one device pass.  Semantics and the deliberate differences from OpenCV: DESIGN.md §8.

numpy in, numpy out (upstream's contract); the host only normalises keypoints and packs the ragged batch.
"""
import numpy as np
import torch

from . import _lib

STATUS_OK, STATUS_FEW, STATUS_NO_MODEL, STATUS_NO_POSE, STATUS_BAD_COUNT = 0, 1, 2, 3, 4
MAX_MATCHES = 4096


def _dev():
    if not torch.cuda.is_available():
        raise RuntimeError("RANSAC pose estimation runs on an MI355X (no CPU fallback)")
    return torch.device("cuda", torch.cuda.current_device())


def normalize_keypoints(kpts, K):
    """``(x - K[[0,1],[2,2]]) / K[[0,1],[0,1]]`` in fp64 (upstream's estimate_pose); K is 3x3 or 4x4."""
    K = np.asarray(K, np.float64)
    return (np.asarray(kpts, np.float64) - K[[0, 1], [2, 2]][None]) / K[[0, 1], [0, 1]][None]


def essential_ransac(kpts0n, kpts1n, thresholds, conf=0.99999, seed=0, max_iters=1000):
    """RANSAC essential matrix + recoverPose of a ragged batch on the device (``e2emv_essential_ransac``).
    ``kpts0n`` / ``kpts1n``: lists of [M_p, 2] normalised keypoints (M_p <= 4096), ``thresholds``: per-problem normalised
    inlier thresholds.  Returns a dict of numpy arrays: ``E``, ``R`` [P,3,3], ``t`` [P,3], ``mask`` (list of [M_p] bool),
    ``n_inliers``, ``n_cheiral``, ``iters``, ``status`` [P]."""
    P = len(kpts0n)
    n_per = np.array([len(k) for k in kpts0n], np.int32)
    if P == 0:
        raise ValueError("essential_ransac: empty batch")
    if n_per.max() > MAX_MATCHES:
        raise ValueError("essential_ransac: at most {} matches per problem (got {})".format(MAX_MATCHES, int(n_per.max())))
    Mmax = max(int(n_per.max()), 1)
    k0, k1 = np.zeros((P, Mmax, 2)), np.zeros((P, Mmax, 2))
    for p in range(P):
        k0[p, :n_per[p]], k1[p, :n_per[p]] = kpts0n[p], kpts1n[p]
    dev = _dev()
    ctx = _lib.context(dev)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    d_n, d_k0, d_k1, d_th = up(n_per), up(k0), up(k1), up(np.asarray(thresholds, np.float64).reshape(P))
    f64, i32 = dict(dtype=torch.float64, device=dev), dict(dtype=torch.int32, device=dev)
    E, R, t = torch.empty((P, 3, 3), **f64), torch.empty((P, 3, 3), **f64), torch.empty((P, 3), **f64)
    inl = torch.empty((P, Mmax), dtype=torch.uint8, device=dev)
    n_inl, n_ch, iters, status = (torch.empty((P,), **i32) for _ in range(4))
    Pp = _lib.ptr
    with torch.cuda.device(dev):
        ctx.call("e2emv_essential_ransac", P, Mmax, Pp(d_n), Pp(d_k0), Pp(d_k1), Pp(d_th), float(conf), int(max_iters),
                 int(seed) & 0xFFFFFFFF, Pp(E), Pp(R), Pp(t), Pp(inl), Pp(n_inl), Pp(n_ch), Pp(iters), Pp(status), _lib.stream_ptr(dev))
    inl_h = inl.cpu().numpy().astype(bool)
    return {"E": E.cpu().numpy(), "R": R.cpu().numpy(), "t": t.cpu().numpy(), "mask": [inl_h[p, :n_per[p]] for p in range(P)],
            "n_inliers": n_inl.cpu().numpy(), "n_cheiral": n_ch.cpu().numpy(), "iters": iters.cpu().numpy(),
            "status": status.cpu().numpy()}


def estimate_poses_ransac(problems, thresh=1.0, conf=0.99999, seed=0):
    """``estimate_pose`` of many image pairs in one device pass.  ``problems``: list of ``(kpts0, kpts1, K0, K1)`` (pixel
    keypoints [M,2], 3x3 or 4x4 intrinsics).  Returns one ``(R [3,3], t [3], mask [M] bool)`` or ``None`` per problem."""
    out = [None] * len(problems)
    live = [q for q, pr in enumerate(problems) if len(pr[0]) >= 5]  # upstream: fewer than 5 matches -> None
    if not live:
        return out
    k0n, k1n, th = [], [], []
    for q in live:
        kpts0, kpts1, K0, K1 = problems[q]
        K0, K1 = np.asarray(K0, np.float64), np.asarray(K1, np.float64)
        f_mean = np.mean([K0[0, 0], K1[1, 1], K0[0, 0], K1[1, 1]])  # upstream's expression, kept as it is
        th.append(thresh / f_mean)
        k0n.append(normalize_keypoints(kpts0, K0))
        k1n.append(normalize_keypoints(kpts1, K1))
    r = essential_ransac(k0n, k1n, th, conf=conf, seed=seed)
    for i, q in enumerate(live):
        if r["status"][i] == STATUS_OK:
            out[q] = (r["R"][i], r["t"][i], r["mask"][i])
    return out


def estimate_pose(kpts0, kpts1, K0, K1, thresh, conf=0.99999):
    """SuperGlue's ``estimate_pose(kpts0, kpts1, K0, K1, thresh, conf)``: ``(R, t, mask)`` or ``None`` (fewer than 5
    matches, no RANSAC model, or no pose with a point in front of both cameras)."""
    return estimate_poses_ransac([(kpts0, kpts1, K0, K1)], thresh=thresh, conf=conf)[0]


def essential_5pt(x0, x1):
    """The 5-point minimal solver alone (``e2emv_essential_5pt``): x0, x1 [n,5,2] normalised -> (E [n,10,3,3], nsol [n])."""
    x0, x1 = np.ascontiguousarray(x0, np.float64), np.ascontiguousarray(x1, np.float64)
    n = x0.shape[0]
    dev = _dev()
    ctx = _lib.context(dev)
    d0, d1 = torch.from_numpy(x0).to(dev), torch.from_numpy(x1).to(dev)
    E = torch.empty((n, 10, 3, 3), dtype=torch.float64, device=dev)
    ns = torch.empty((n,), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        ctx.call("e2emv_essential_5pt", n, _lib.ptr(d0), _lib.ptr(d1), _lib.ptr(E), _lib.ptr(ns), _lib.stream_ptr(dev))
    return E.cpu().numpy(), ns.cpu().numpy()
