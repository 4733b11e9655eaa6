"""TEST HELPER (no test in here, never imported by the product path): the Levenberg-Marquardt loop of ``oracle/ba2view.py`` with a
robust loss, the fp64 restatement of what ``ba2view_kernel<LOSS>`` (csrc/ba2view.hip) computes through ``e2emv_ba_2view_loss``.

Same dense normal equations, Jacobi preconditioner, LU solve and bookkeeping as the oracle, statement for statement.  Added:

* the loss.  A residual block is one observation, so match i has two: ``s0 = |r0|^2`` (image 0) and ``s1 = |r1|^2`` (image 1) of
  the WEIGHTED residuals (weight ``conf / cden``, ``cden = 0.5 max(2 sum conf, 1e-6)``).  The cost that the bookkeeping compares
  is ``sum rho(s0) + sum rho(s1)`` (no factor 1/2, like the oracle's ``rn = sum s``).  The linearisation is Ceres' corrector for
  ``rho'' <= 0``: the two rows of a block - residual and Jacobian - times ``sqrt(rho'(s))``, before ``J^T J`` and ``J^T r`` are
  formed, so the positivity check of the diagonal and the 1e-12 floor of the preconditioner see the corrected system.
  ``rho`` and ``sqrt(rho')`` in the operation order csrc/mvba.h fixes (``a2 = a * a``):
      huber : s <= a2 ? (rho = s, sqrt(rho') = 1) : (t = sqrt(s); rho = 2 a t - a2; sqrt(rho') = sqrt(a / t))
      cauchy: q = s / a2; rho = a2 log1p(q); sqrt(rho') = sqrt(1 / (1 + q))
  The scale is relative: sample b runs with ``a_b = loss_scale / cden_b``, one fp64 division.
* ``homogeneous_sign`` and the trajectory, with the meaning they have in the oracle; the trajectory's keys are ``best`` [n+1,4,4]
  (best pose AFTER evaluation it), ``cost`` [n+1], ``best_cost`` [n+1] (best cost BEFORE the comparison, NaN at it = 0),
  ``best_cost_after`` [n+1], ``accepted`` [n+1] and, with Huber, ``inliers`` / ``outliers`` [n+1]: the observations on the first /
  second branch at that evaluation.
* the summary per valid sample, ``[cost at the start, best cost, evaluations that improved, a_b]`` (``a_b`` = 0 without a loss).

``loss=None`` is ``oracle.ba2view.run_bundle_adjust_2_view`` bit for bit: nothing is multiplied, the cost is its expression."""
import torch

from oracle import kornia_fns as K
from oracle.pytorch3d_fns import hat, se3_exp_map

LOSSES = (None, "huber", "cauchy")


def rho_sq(loss, a, s):
    """(rho(s), sqrt(rho'(s))) elementwise for an fp64 tensor ``s`` at the absolute scale ``a``."""
    if loss is None:
        return s, torch.ones_like(s)
    a = float(a)
    a2 = a * a
    if loss == "huber":
        small = s <= a2
        t = torch.sqrt(torch.where(small, torch.ones_like(s), s))
        return torch.where(small, s, 2.0 * a * t - a2), torch.where(small, torch.ones_like(s), torch.sqrt(a / t))
    if loss == "cauchy":
        q = s / a2
        return a2 * torch.log1p(q), torch.sqrt(1.0 / (1.0 + q))
    raise ValueError(loss)


def corrected_system(extr1, pts, x0, x1, c, loss=None, a=0.0):
    """One sample: ``(J [4M, 6+3M], r [4M], cost, s [2M])`` - the weighted Jacobian and residual in the oracle's row order (all
    image-0 rows, then all image-1 rows), corrected for ``loss`` at the absolute scale ``a``, the cost ``sum rho`` and the squared
    block norms before the correction (blocks in the same order)."""
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
    J = torch.zeros(4 * M, 6 + 3 * M, dtype=dt)
    r = torch.zeros(4 * M, dtype=dt)
    for i in range(M):
        J[2 * i:2 * i + 2, 6 + 3 * i:9 + 3 * i] = c[i] * Jp0[i]
        J[2 * M + 2 * i:2 * M + 2 * i + 2, 6 + 3 * i:9 + 3 * i] = c[i] * (Jp1[i] @ extr1[:3, :3])
        J[2 * M + 2 * i:2 * M + 2 * i + 2, :6] = c[i] * (Jp1[i] @ torch.cat([eye3, -hat(Ap1[i])], 1))
        r[2 * i:2 * i + 2] = c[i] * (pi0[i] - x0[i])
        r[2 * M + 2 * i:2 * M + 2 * i + 2] = c[i] * (pi1[i] - x1[i])
    e = (r * r).view(2 * M, 2)
    s = e[:, 0] + e[:, 1]
    if loss is None:
        return J, r, (r ** 2).sum(), s
    rho, sq = rho_sq(loss, a, s)
    rows = sq.repeat_interleave(2)
    return J * rows[:, None], r * rows, rho[:M].sum() + rho[M:].sum(), s


def run_bundle_adjust_2_view(kpts0_norm, kpts1_norm, confidence, init_T021, n_iterations, lm_increase=1.5, lm_decrease=3.5,
                             homogeneous_sign=None, loss=None, loss_scale=None):
    """``(refined T_021 of the valid samples [n_valid,4,4], valid_batch [B] bool, trajectories, summary [n_valid,4])``; the
    arguments of the oracle plus ``loss`` in ``LOSSES`` at the RELATIVE scale ``loss_scale``."""
    if loss not in LOSSES:
        raise ValueError(loss)
    conf = confidence.squeeze(-1) if confidence.dim() == 3 else confidence
    B = kpts0_norm.shape[0]
    dt = kpts0_norm.dtype
    valid = conf > 0.0
    valid_batch = valid.sum(-1) > 6
    out, trajectory, summary = [], [], []
    for b in range(B):
        if not bool(valid_batch[b]):
            continue
        m = valid[b]
        x0, x1, c = kpts0_norm[b][m], kpts1_norm[b][m], conf[b][m]
        cden = 0.5 * (2 * c.sum()).clamp(min=1e-6)
        c = c / cden  # each match is two observations
        a = float(loss_scale) / float(cden) if loss is not None else 0.0
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
        tr = {"best": [], "cost": [], "best_cost": [], "best_cost_after": [], "accepted": [], "inliers": [], "outliers": []}
        for it in range(n_iterations + 1):
            J, r, rn, s = corrected_system(extr1, pts, x0, x1, c, loss, a)
            A, bvec = J.T @ J, -(J.T @ r)
            tr["cost"].append(rn)
            tr["best_cost"].append(rn * float("nan") if it == 0 else best_r)
            tr["inliers"].append(int((s <= a * a).sum()))
            tr["outliers"].append(int((s > a * a).sum()))
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
            tr["best_cost_after"].append(best_r)
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
        trajectory.append({"best": torch.stack(tr["best"]), "cost": torch.stack(tr["cost"]), "best_cost": torch.stack(tr["best_cost"]),
                           "best_cost_after": torch.stack(tr["best_cost_after"]), "accepted": torch.tensor(tr["accepted"]),
                           "inliers": torch.tensor(tr["inliers"]), "outliers": torch.tensor(tr["outliers"])})
        summary.append(torch.stack([tr["cost"][0], best_r, torch.tensor(float(sum(tr["accepted"][1:])), dtype=dt), torch.tensor(a, dtype=dt)]))
    res = torch.stack(out) if out else torch.zeros(0, 4, 4, dtype=dt)
    return res, valid_batch, trajectory, (torch.stack(summary) if summary else torch.zeros(0, 4, dtype=dt))
