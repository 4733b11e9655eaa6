"""TEST HELPER (no test in here, never imported by the product path): ``oracle.mvba.solve``'s Levenberg-Marquardt loop with a
robust loss, the fp64 / long-double restatement of what ``mvba_kernel<LOSS>`` (csrc/mvba.hip, csrc/mvba.h) computes.

Semantics of a ``ceres::LossFunction`` where the reference passes NULL.  One residual block = one observation, ``r = (rx, ry)``
the WEIGHTED residual, ``s = rx^2 + ry^2``; the cost is ``1/2 sum rho(s)`` at the iterate, at the candidate and in the summary;
the linearisation is Ceres' corrector for ``rho'' <= 0``: residual and both Jacobian blocks of the observation times
``sqrt(rho'(s))``.  Everything else - gradient, blocks, Schur system, model cost change ``-m.(r + m/2)``, tolerances, radius,
terminations - is ``oracle.mvba.solve`` on the corrected ``r, J``, statement for statement.

``rho`` and ``sqrt(rho')`` in the operation order csrc/mvba.h fixes (``a2 = a * a``):
    huber : s <= a2 ? (rho = s, sqrt(rho') = 1) : (t = sqrt(s); rho = 2 a t - a2; sqrt(rho') = sqrt(a / t))
    cauchy: q = s / a2; rho = a2 log1p(q); sqrt(rho') = sqrt(1 / (1 + q))

Two properties the tests rely on, and why they hold:
  * ``loss=None`` is ``oracle.mvba.solve`` bit for bit: no statement of the loop differs, the cost is the oracle's expression.
  * Huber with a scale above every residual of the run is the loss-free run bit for bit: ``sqrt(rho') = 1`` and a product with
    1.0 is exact; ``rho = s`` enters the cost as its two terms ``rx^2, ry^2`` in the slots the loss-free sum has them in (an
    observation beyond the scale contributes ``rho, 0`` in the same two slots), so the sum is the same sum.

``stats`` (a dict the caller passes) receives, over every point evaluated - iterates and candidates -, ``min_knife``: the smallest
``|s - a^2| / a^2`` (how close any observation came to Huber's branch point; NaN residuals do not count), ``min_s`` / ``max_s``
and ``inliers`` / ``outliers``: how many evaluations took the first / second Huber branch."""
import numpy as np

from oracle import mvba

LOSSES = (None, "huber", "cauchy")


def rho_sq(loss, a, s):
    """(rho(s), sqrt(rho'(s))) elementwise, in the dtype of ``s``; ``a`` is converted to it."""
    if loss is None:
        return s, np.ones_like(s)
    a = s.dtype.type(a)
    a2 = a * a
    with np.errstate(invalid="ignore", divide="ignore"):
        if loss == "huber":
            small = s <= a2
            t = np.sqrt(np.where(small, s.dtype.type(1), s))
            return np.where(small, s, 2 * a * t - a2), np.where(small, s.dtype.type(1), np.sqrt(a / t))
        if loss == "cauchy":
            q = s / a2
            return a2 * np.log1p(q), np.sqrt(1 / (1 + q))
    raise ValueError(loss)


def corrected(prob, cams, pts, loss, a, stats=None, **lin):
    """(r, Jc, Jp, sum rho) at (cams, pts): ``oracle.mvba.linearise`` then the corrector.  ``lin``: linearise's keywords."""
    r, Jc, Jp = mvba.linearise(prob, cams, pts, **lin)
    if loss is None:
        return r, Jc, Jp, (r * r).sum()
    e = r * r
    s = e[:, 0] + e[:, 1]
    rho, sq = rho_sq(loss, a, s)
    if loss == "huber":  # rho = s stays the two terms it is made of (see the module docstring)
        small = s <= s.dtype.type(a) * s.dtype.type(a)
        terms = np.where(small[:, None], e, np.stack([rho, np.zeros_like(rho)], -1))
    else:
        terms = np.stack([rho, np.zeros_like(rho)], -1)
    if stats is not None:
        a2 = float(a) * float(a)
        sf = np.asarray(s, np.float64)
        ok = np.isfinite(sf)
        if ok.any():
            stats["min_knife"] = min(stats.get("min_knife", np.inf), float(np.abs(sf[ok] - a2).min() / a2))
            stats["min_s"] = min(stats.get("min_s", np.inf), float(sf[ok].min()))
            stats["max_s"] = max(stats.get("max_s", 0.0), float(sf[ok].max()))
            stats["inliers"] = stats.get("inliers", 0) + int((sf[ok] <= a2).sum())
            stats["outliers"] = stats.get("outliers", 0) + int((sf[ok] > a2).sum())
    return r * sq[:, None], Jc * sq[:, None, None], Jp * sq[:, None, None], terms.sum()


def solve(prob, max_iterations=50, loss=None, loss_scale=None, function_tolerance=1e-6, gradient_tolerance=1e-10, parameter_tolerance=1e-8,
          return_trajectory=False, point_inverse="lapack", reduced_solver="lapack", schur_right=False, expanded_rotation=False,
          divide=False, extended_linearise=False, dtype=np.float64, stats=None):
    """``oracle.mvba.solve`` (same arguments, same returns, same trajectory records) with ``loss`` in ``LOSSES`` at the ABSOLUTE
    scale ``loss_scale`` (units of the weighted residual).  ``dtype=np.longdouble``: the whole algorithm, the loss included, in
    numpy's widest float, rounded to fp64 where it returns and records."""
    if loss not in LOSSES:
        raise ValueError(loss)
    wide = dtype is not np.float64
    if wide:
        prob = dict(prob, intr=np.asarray(prob["intr"], dtype), obs=np.asarray(prob["obs"], dtype), wts=np.asarray(prob["wts"], dtype))
        point_inverse, reduced_solver = "adjugate", "unblocked"
    num = (lambda x: x) if wide else float
    lin = dict(expanded_rotation=expanded_rotation, divide=divide, extended=extended_linearise)
    ci, pi = prob["cam_idx"], prob["pt_idx"]
    C, P = len(prob["cams"]), len(prob["pts"])
    cams, pts = prob["cams"].astype(dtype).copy(), prob["pts"].astype(dtype).copy()
    free = np.array([c != prob["fixed"] for c in range(C)])
    radius, decrease, invalid = 1e4, 2.0, 0
    scale_c = scale_p = None
    summary = dict(iterations=0, termination="max_iterations")

    def blocks(Jc, Jp, r):
        U = np.zeros((C, 6, 6), dtype); gc = np.zeros((C, 6), dtype); V = np.zeros((P, 3, 3), dtype); gp = np.zeros((P, 3), dtype)
        np.add.at(U, ci, np.einsum("oki,okj->oij", Jc, Jc))
        np.add.at(gc, ci, np.einsum("oki,ok->oi", Jc, r))
        np.add.at(V, pi, np.einsum("oki,okj->oij", Jp, Jp))
        np.add.at(gp, pi, np.einsum("oki,ok->oi", Jp, r))
        return U, gc, V, gp

    r, Jc, Jp, total = corrected(prob, cams, pts, loss, loss_scale, stats, **lin)
    cost = 0.5 * num(total)
    summary["initial_cost"] = float(cost)
    it = 0
    traj = []

    def record(kind, termination="max_iterations", step_ratio=None, fn_ratio=None, rho=None):
        f = lambda x: None if x is None else float(x)  # noqa: E731
        traj.append(dict(cams=cams.astype(np.float64), pts=pts.astype(np.float64), cost=float(cost), radius=float(radius), decrease=decrease,
                         kind=kind, iterations=it, termination=termination, gmax=None, step_ratio=f(step_ratio), fn_ratio=f(fn_ratio), rho=f(rho)))

    record("start")
    while True:
        U, gc, V, gp = blocks(Jc, Jp, r)
        dc, dp = np.einsum("cii->ci", U).copy(), np.einsum("pii->pi", V).copy()
        if scale_c is None:
            scale_c, scale_p = 1.0 / (1.0 + np.sqrt(dc)), 1.0 / (1.0 + np.sqrt(dp))
        gmax = max(np.abs(gc[free]).max(initial=0.0), np.abs(gp).max(initial=0.0))
        traj[-1]["gmax"] = float(gmax)
        if gmax <= gradient_tolerance:
            summary["termination"] = traj[-1]["termination"] = "gradient_tolerance"
            break
        if it >= max_iterations:
            break
        it += 1
        lam_c = np.clip(dc * scale_c ** 2, 1e-6, 1e32) / radius / scale_c ** 2
        lam_p = np.clip(dp * scale_p ** 2, 1e-6, 1e32) / radius / scale_p ** 2
        Vd = V + np.einsum("pi,ij->pij", lam_p, np.eye(3))
        if point_inverse == "adjugate":
            Vinv = mvba._inv3_adjugate(Vd)
        elif point_inverse == "extended":
            Vinv = mvba._inv3_adjugate(Vd.astype(np.longdouble)).astype(np.float64)
        elif point_inverse == "cholesky":
            Linv = np.linalg.inv(np.linalg.cholesky(Vd))
            Vinv = np.transpose(Linv, (0, 2, 1)) @ Linv
        else:
            Vinv = np.linalg.inv(Vd)
        W = np.einsum("oki,okj->oij", Jc, Jp)  # [O,6,3]
        Y = W @ Vinv[pi]
        n = 6 * C
        S = np.zeros((C, 6, C, 6), dtype); rhs = -gc.copy()
        for c in range(C):
            S[c, :, c, :] = U[c] + np.diag(lam_c[c])
        order = np.argsort(pi, kind="stable")
        starts = np.searchsorted(pi[order], np.arange(P + 1))
        for p_ in range(P):
            oo = order[starts[p_]:starts[p_ + 1]]
            for a in oo:
                rhs[ci[a]] += W[a] @ (Vinv[p_] @ gp[p_]) if schur_right else Y[a] @ gp[p_]
                for b in oo:
                    S[ci[a], :, ci[b], :] -= W[a] @ (Vinv[p_] @ W[b].T) if schur_right else Y[a] @ W[b].T
        S = S.reshape(n, n); rhs = rhs.reshape(n)
        keep = np.repeat(free, 6)
        step_c = np.zeros(n, dtype)
        ok = True
        try:
            if reduced_solver == "unblocked":
                step_c[keep] = mvba._solve_spd_unblocked(S[np.ix_(keep, keep)], rhs[keep])
            else:
                L = np.linalg.cholesky(S[np.ix_(keep, keep)])
                step_c[keep] = np.linalg.solve(L.T, np.linalg.solve(L, rhs[keep]))
        except np.linalg.LinAlgError:
            ok = False
        step_c = step_c.reshape(C, 6)
        if ok:
            acc = gp.copy()
            np.add.at(acc, pi, np.einsum("oij,oi->oj", W, step_c[ci]))
            step_p = -np.einsum("pij,pj->pi", Vinv, acc)
            m = np.einsum("oki,oi->ok", Jc, step_c[ci]) + np.einsum("oki,oi->ok", Jp, step_p[pi])
            model_change = -num((m * (r + 0.5 * m)).sum())
            ok = model_change > 0.0
        if not ok:
            invalid += 1
            if invalid >= 5:
                summary["termination"] = "invalid_steps"
                record("invalid", "invalid_steps")
                break
            radius /= decrease
            decrease *= 2.0
            record("invalid")
            continue
        invalid = 0
        step_norm = np.sqrt((step_c[free] ** 2).sum() + (step_p ** 2).sum())
        x_norm = np.sqrt((cams[free] ** 2).sum() + (pts ** 2).sum())
        step_ratio = step_norm / (x_norm + parameter_tolerance)
        if step_norm <= parameter_tolerance * (x_norm + parameter_tolerance):
            summary["termination"] = "parameter_tolerance"
            record("stop", "parameter_tolerance", step_ratio)
            break
        cand_c, cand_p = cams + step_c * free[:, None], pts + step_p
        r2, Jc2, Jp2, total2 = corrected(prob, cand_c, cand_p, loss, loss_scale, stats, **lin)
        cand_cost = 0.5 * num(total2)
        change = cost - cand_cost
        fn_ratio = abs(change) / cost
        if abs(change) <= function_tolerance * cost:
            summary["termination"] = "function_tolerance"
            record("stop", "function_tolerance", step_ratio, fn_ratio)
            break
        rho = change / model_change
        accepted = rho > 1e-3
        if accepted:
            cams, pts, r, Jc, Jp, cost = cand_c, cand_p, r2, Jc2, Jp2, cand_cost
            radius = min(1e16, radius / max(1.0 / 3.0, 1.0 - (2.0 * rho - 1.0) ** 3))
            decrease = 2.0
        else:
            radius /= decrease
            decrease *= 2.0
        if radius < 1e-32:
            summary["termination"] = "radius"
        record("accepted" if accepted else "rejected", summary["termination"], step_ratio, fn_ratio, rho)
        if radius < 1e-32:
            break
    summary["iterations"] = it
    summary["final_cost"] = float(cost)
    cams, pts = cams.astype(np.float64), pts.astype(np.float64)
    if return_trajectory:
        return cams, pts, summary, traj
    return cams, pts, summary


def objective(prob, cams, pts, loss, a):
    """``1/2 sum rho(s)`` at (cams, pts), in the dtype of ``cams``."""
    return 0.5 * corrected(prob, cams, pts, loss, a)[3]


def gradient(prob, cams, pts, loss, a):
    """``J^T r`` of the corrected system as (g_cams [C,6] - zero for the fixed camera -, g_pts [P,3])."""
    r, Jc, Jp, _ = corrected(prob, cams, pts, loss, a)
    gc, gp = np.zeros(cams.shape, r.dtype), np.zeros(pts.shape, r.dtype)
    np.add.at(gc, prob["cam_idx"], np.einsum("oki,ok->oi", Jc, r))
    np.add.at(gp, prob["pt_idx"], np.einsum("oki,ok->oi", Jp, r))
    return gc, gp
