"""Oracle: two-view Levenberg-Marquardt bundle adjustment (SURVEY.md 8(f) "next" row 1).

TEST INFRASTRUCTURE (see oracle/__init__.py).  Restates
``pose_optimization/two_view/bundle_adjust_gauss_newton_2_view.py`` (``Observations`` :10-48, ``fill_J`` :50-67,
``compute_A_b`` :69-99, ``BundleAdjustGaussNewton2View.run`` :127-201) and ``run_bundle_adjust_2_view``
(``estimate_relative_pose.py:138-144``) sample by sample with the same dense normal equations: camera 0 fixed at the
identity, 6 pose + 3M point unknowns, Jacobi-preconditioned damped system ``D^-1 J^T J + lambda I`` solved densely, update
ALWAYS applied, best-residual pose kept, lambda /= 3.5 on improvement else *= 1.5, n_iterations + 1 residual
evaluations.  Pinned by tests/golden/ba2view_reference.npz (the reference's own class run in the build container).
"""
import torch

from . import kornia_fns as K
from .pytorch3d_fns import hat, se3_exp_map


def _normal_equations(extr1, pts, x0, x1, c):
    """One sample.  extr1 [4,4]; pts [M,3]; x0,x1 [M,2]; c [M] (normalised weights).  Dense J^T J, -J^T r, |r|^2."""
    M = pts.shape[0]
    dt = pts.dtype
    eye3 = torch.eye(3, dtype=dt)

    def proj(Ap):
        J = torch.zeros(M, 2, 3, dtype=dt)
        J[:, 0, 0] = 1.0 / Ap[:, 2]
        J[:, 0, 2] = -Ap[:, 0] / Ap[:, 2] ** 2
        J[:, 1, 1] = 1.0 / Ap[:, 2]
        J[:, 1, 2] = -Ap[:, 1] / Ap[:, 2] ** 2
        return Ap[:, :2] / Ap[:, 2:3], J

    Ap0 = pts
    Ap1 = pts @ extr1[:3, :3].T + extr1[:3, 3]
    pi0, Jp0 = proj(Ap0)
    pi1, Jp1 = proj(Ap1)
    n_unk = 6 + 3 * M
    J = torch.zeros(4 * M, n_unk, dtype=dt)  # observation order of the reference: all cam-0 rows, then all cam-1 rows
    r = torch.zeros(4 * M, dtype=dt)
    for i in range(M):
        J[2 * i:2 * i + 2, 6 + 3 * i:9 + 3 * i] = c[i] * Jp0[i]
        J[2 * M + 2 * i:2 * M + 2 * i + 2, 6 + 3 * i:9 + 3 * i] = c[i] * (Jp1[i] @ extr1[:3, :3])
        J[2 * M + 2 * i:2 * M + 2 * i + 2, :6] = c[i] * (Jp1[i] @ torch.cat([eye3, -hat(Ap1[i])], 1))
        r[2 * i:2 * i + 2] = c[i] * (pi0[i] - x0[i])
        r[2 * M + 2 * i:2 * M + 2 * i + 2] = c[i] * (pi1[i] - x1[i])
    return J.T @ J, -(J.T @ r), (r ** 2).sum()


def run_bundle_adjust_2_view(kpts0_norm, kpts1_norm, confidence, init_T021, n_iterations, lm_increase=1.5, lm_decrease=3.5,
                             homogeneous_sign=None, return_trajectory=False):
    """Returns (refined T_021 of the valid samples [n_valid,4,4], valid_batch [B] bool) like the reference.

    ``homogeneous_sign`` (+1 / -1): the DLT null vector of the triangulation has no defined sign, and the ``1 / (w + 1e-8)``
    of the de-homogenisation makes the start points depend on it (relative ~1e-8 / |w|).  With a sign given, every null
    vector is flipped so that its last component has that sign before it is de-homogenised; ``None`` keeps whatever the
    SVD returned.  Two runs with +1 and -1 bracket what an implementation with another null-vector routine may return.

    ``return_trajectory``: also returns, as a third value, one dict per valid sample with an entry for each residual
    evaluation ``it = 0..n_iterations``: ``best`` [n+1,4,4] the best pose AFTER that evaluation, ``rn`` [n+1] its residual,
    ``best_r`` [n+1] the best residual BEFORE the comparison (NaN at it = 0, which compares with nothing) and ``accepted``
    [n+1] bool (True at it = 0).  The loop does not look ahead: a run with n iterations is a prefix of a run with n' > n,
    and ``best[n]`` IS the result of ``n_iterations = n``.  One 10-iteration run yields the expected result of every
    ``n_iterations <= 10``."""
    conf = confidence.squeeze(-1) if confidence.dim() == 3 else confidence
    B = kpts0_norm.shape[0]
    dt = kpts0_norm.dtype
    valid = conf > 0.0
    valid_batch = valid.sum(-1) > 6
    out, trajectory = [], []
    for b in range(B):
        if not bool(valid_batch[b]):
            continue
        m = valid[b]
        x0, x1, c = kpts0_norm[b][m], kpts1_norm[b][m], conf[b][m]
        c = c / (0.5 * (2 * c.sum()).clamp(min=1e-6))  # each match is two observations (:45-48)
        extr1 = init_T021[b].clone().to(dt)
        P0 = torch.eye(4, dtype=dt)[:3]
        if homogeneous_sign is None:
            pts = K.triangulate_points(P0[None], extr1[None, :3], x0[None], x1[None])[0]
        else:
            h = K.triangulate_points_homogeneous(P0[None], extr1[None, :3], x0[None], x1[None])[0]
            flip = torch.where(torch.signbit(h[:, 3:]) != (homogeneous_sign < 0), -torch.ones_like(h[:, 3:]), torch.ones_like(h[:, 3:]))
            pts = K.convert_points_from_homogeneous(h * flip)
        lam = 0.1
        best_r, best = None, extr1.clone()
        tr = {"best": [], "rn": [], "best_r": [], "accepted": []}
        for it in range(n_iterations + 1):
            A, bvec, rn = _normal_equations(extr1, pts, x0, x1, c)
            tr["rn"].append(rn)
            tr["best_r"].append(rn * float("nan") if it == 0 else best_r)
            if it == 0:
                best_r, best = rn, extr1.clone()
                tr["accepted"].append(True)
            else:
                tr["accepted"].append(bool(rn < best_r))
                if rn < best_r:
                    best_r, best = rn, extr1.clone()
                    lam = lam / lm_decrease
                else:
                    lam = lam * lm_increase
            tr["best"].append(best)
            if it == n_iterations:
                break
            d = torch.diagonal(A)
            if bool((d > 0).all()):
                inv = 1.0 / d.clamp(min=1e-12)
                A = inv[:, None] * A
                bvec = inv * bvec
            A = A + torch.eye(A.shape[0], dtype=dt) * lam
            LU, piv, info = torch.linalg.lu_factor_ex(A)
            if int(info) != 0:
                continue
            dx = torch.linalg.lu_solve(LU, piv, bvec[:, None])[:, 0]
            delta = se3_exp_map(dx[None, :6]).permute(0, 2, 1)[0]
            extr1 = delta @ extr1
            pts = pts + dx[6:].view(-1, 3)
        out.append(best)
        trajectory.append({"best": torch.stack(tr["best"]), "rn": torch.stack(tr["rn"]), "best_r": torch.stack(tr["best_r"]),
                           "accepted": torch.tensor(tr["accepted"])})
    res = torch.stack(out) if out else torch.zeros(0, 4, 4, dtype=dt)
    if return_trajectory:
        return res, valid_batch, trajectory
    return res, valid_batch
