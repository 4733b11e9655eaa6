"""ORACLE (test infrastructure only - never imported by the product path): CPU restatement of the multi-view
bundle adjustment the reference delegates to Ceres.

Follows pose_optimization/multi_view/bundle_adjustment/problem/include/ba_problem.h:60-151 (the two residual
functors), problem/src/ba_problem.cpp:8-88 (CSV parser), :98-113 (WriteResult), :115-157 (Solve: DENSE_SCHUR,
squared loss, Ceres defaults).  Ceres 2.0 is an un-vendored dependency that is absent here, so the minimiser is a
restatement of its documented Levenberg-Marquardt trust-region loop (Ceres "Solving Non-linear Least Squares":
Jacobi column scaling fixed at the first iterate, lm diagonal = sqrt(clamp(diag(J^T J), 1e-6, 1e32) / radius),
step quality rho = cost change / model cost change, accept when rho > 1e-3, radius /= max(1/3, 1 - (2 rho - 1)^3)
on acceptance, radius /= 2, 4, 8, ... on rejection, initial radius 1e4, <= 50 iterations, function tolerance 1e-6,
gradient tolerance 1e-10, parameter tolerance 1e-8).  PARITY ANCHOR: the reference's own gtests
(problem/test/test_ba_problem.cpp:172-190) - known answers with tolerances - re-run in tests/test_mv_ba.py;
against Ceres itself parity is unpinned (no Ceres in the image).

Quirk kept (ba_problem.cpp:129-137, ba_problem.h:60-100): observations of the fixed camera are predicted with the
IDENTITY pose, whatever its row in the file says, and that camera's parameters are written back untouched.
"""
import numpy as np


def split_by_char(line, c=","):
    """io/src/file_utils.cpp:3-25 with allow_empty=False."""
    return [t for t in line.rstrip("\n").split(c) if t != ""]


def R_to_aa(R):
    """ceres::RotationMatrixToAngleAxis (via the quaternion); R is a proper 3x3 (row/col indexable)."""
    tr = R[0, 0] + R[1, 1] + R[2, 2]
    q = np.zeros(4)
    if tr >= 0:
        t = np.sqrt(tr + 1.0)
        q[0] = 0.5 * t
        t = 0.5 / t
        q[1], q[2], q[3] = (R[2, 1] - R[1, 2]) * t, (R[0, 2] - R[2, 0]) * t, (R[1, 0] - R[0, 1]) * t
    else:
        i = 0
        if R[1, 1] > R[0, 0]:
            i = 1
        if R[2, 2] > R[i, i]:
            i = 2
        j, k = (i + 1) % 3, (i + 2) % 3
        t = np.sqrt(R[i, i] - R[j, j] - R[k, k] + 1.0)
        q[i + 1] = 0.5 * t
        t = 0.5 / t
        q[0] = (R[k, j] - R[j, k]) * t
        q[j + 1] = (R[j, i] + R[i, j]) * t
        q[k + 1] = (R[k, i] + R[i, k]) * t
    s2 = q[1] ** 2 + q[2] ** 2 + q[3] ** 2
    if s2 > 0:
        s = np.sqrt(s2)
        two_theta = 2.0 * (np.arctan2(-s, -q[0]) if q[0] < 0 else np.arctan2(s, q[0]))
        return q[1:] * (two_theta / s)
    return 2.0 * q[1:]


def aa_to_R(w):
    """ceres::AngleAxisToRotationMatrix."""
    t2 = float(w @ w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if t2 > np.finfo(float).eps:
        th = np.sqrt(t2)
        k = K / th
        return np.eye(3) + np.sin(th) * k + (1 - np.cos(th)) * (k @ k)
    return np.eye(3) + K


def read_problem(path):
    """BaProblem::BaProblem (ba_problem.cpp:8-88): rows are classified by their field count."""
    hdr, cam_idx, pt_idx, obs, wts, cams, pts = None, [], [], [], [], [], []
    for line in open(path):
        el = split_by_char(line)
        n = len(el)
        if n == 8:
            hdr = dict(n_cams=int(el[0]), fixed=int(el[1]), n_pts=int(el[2]), n_obs=int(el[3]),
                       intr=np.array([float(x) for x in el[4:8]]))
        elif n == 3:
            pts.append([float(x) for x in el])
        elif 4 <= n <= 6:
            cam_idx.append(int(el[0]))
            pt_idx.append(int(el[1]))
            obs.append([float(el[2]), float(el[3])])
            wts.append([1.0, 1.0] if n == 4 else ([float(el[4])] * 2 if n == 5 else [float(el[4]), float(el[5])]))
        elif n == 12:
            R = np.array([float(x) for x in el[:9]]).reshape(3, 3).T  # column-major
            cams.append(np.concatenate([R_to_aa(R), [float(x) for x in el[9:]]]))
    return dict(hdr, cam_idx=np.array(cam_idx, np.int32), pt_idx=np.array(pt_idx, np.int32), obs=np.array(obs).reshape(-1, 2),
                wts=np.array(wts).reshape(-1, 2), cams=np.array(cams).reshape(-1, 6), pts=np.array(pts).reshape(-1, 3))


def write_result(path, cams):
    """BaProblem::WriteResult (ba_problem.cpp:98-113); setprecision(12) is sticky so it also covers t."""
    with open(path, "w") as f:
        for c in cams:
            R = aa_to_R(c[:3])
            f.write(",".join("%.12g" % x for x in R.T.reshape(-1)) + "," + ",".join("%.12g" % x for x in c[3:]) + "\n")


def _rotate(w, X, expanded=False):
    """ceres::AngleAxisRotatePoint and its derivative w.r.t. w (what autodiff yields; Gallego & Yezzi 2015 for the
    general branch, -[X]x for the first-order branch).  w [n,3], X [n,3] -> p [n,3], dp/dw [n,3,3], R [n,3,3].
    expanded: the Rodrigues matrix entry by entry as mv_transform writes it out (1 - v (k1^2 + k2^2), -s k2 + v k0 k1, ...)
    instead of I + s K + v K K - the same matrix, rounded elsewhere."""
    n = len(X)
    t2 = np.einsum("ni,ni->n", w, w)
    big = t2 > np.finfo(float).eps
    th = np.sqrt(np.where(big, t2, 1.0))
    k = w / th[:, None]

    def hat(v):
        H = np.zeros((len(v), 3, 3), v.dtype)
        H[:, 0, 1], H[:, 0, 2], H[:, 1, 0], H[:, 1, 2], H[:, 2, 0], H[:, 2, 1] = -v[:, 2], v[:, 1], v[:, 2], -v[:, 0], -v[:, 1], v[:, 0]
        return H

    Kh = hat(k)
    I = np.broadcast_to(np.eye(3), (n, 3, 3))
    Rb = I + np.sin(th)[:, None, None] * Kh + (1 - np.cos(th))[:, None, None] * (Kh @ Kh)
    if expanded:
        s, v, k0, k1, k2 = np.sin(th), 1.0 - np.cos(th), k[:, 0], k[:, 1], k[:, 2]
        Rb = np.stack([1 - v * (k1 * k1 + k2 * k2), -s * k2 + v * k0 * k1, s * k1 + v * k0 * k2,
                       s * k2 + v * k0 * k1, 1 - v * (k0 * k0 + k2 * k2), -s * k0 + v * k1 * k2,
                       -s * k1 + v * k0 * k2, s * k0 + v * k1 * k2, 1 - v * (k0 * k0 + k1 * k1)], -1).reshape(n, 3, 3)
    Rs = I + hat(w)
    R = np.where(big[:, None, None], Rb, Rs)
    p = np.einsum("nij,nj->ni", R, X)
    Xh = hat(X)
    G = (np.einsum("ni,nj->nij", w, w) + (np.transpose(Rb, (0, 2, 1)) - I) @ hat(w)) / np.where(big, t2, 1.0)[:, None, None]
    Jb = -(Rb @ (Xh @ G)) if expanded else -Rb @ Xh @ G
    J = np.where(big[:, None, None], Jb, -Xh)
    return p, J, R


def linearise(prob, cams, pts, expanded_rotation=False, divide=False, extended=False):
    """Residuals r [O,2] and Jacobians Jc [O,2,6] (zero rows for the fixed camera), Jp [O,2,3].
    divide: the prediction as the reference's functors write it, f * p / p_z + c (ba_problem.h:68-69), instead of the product
    with the reciprocal 1 / p_z that the Jacobians share.  extended: everything evaluated in numpy's widest float and rounded
    to fp64 once at the end - against it the fp64 evaluation shows its own rounding error."""
    if extended:
        wide = dict(prob, intr=np.asarray(prob["intr"], np.longdouble), obs=np.asarray(prob["obs"], np.longdouble),
                    wts=np.asarray(prob["wts"], np.longdouble))
        return tuple(np.asarray(a, np.float64) for a in linearise(wide, cams.astype(np.longdouble), pts.astype(np.longdouble), expanded_rotation, divide))
    ci, pi = prob["cam_idx"], prob["pt_idx"]
    fx, fy, cx, cy = prob["intr"]
    fixed = ci == prob["fixed"]
    c = cams[ci].copy()
    c[fixed] = 0.0  # identity pose for the fixed camera (ba_problem.h:66-79)
    X = pts[pi]
    p, dpdw, R = _rotate(c[:, :3], X, expanded_rotation)
    p = p + c[:, 3:]
    iz = 1.0 / p[:, 2]
    if divide:
        r = np.stack([fx * p[:, 0] / p[:, 2] + cx, fy * p[:, 1] / p[:, 2] + cy], -1) - prob["obs"]
    else:
        r = np.stack([fx * p[:, 0] * iz + cx, fy * p[:, 1] * iz + cy], -1) - prob["obs"]
    w = prob["wts"]
    r = r * w
    dpr = np.zeros((len(ci), 2, 3), p.dtype)
    dpr[:, 0, 0], dpr[:, 0, 2] = fx * iz, -fx * p[:, 0] * iz * iz
    dpr[:, 1, 1], dpr[:, 1, 2] = fy * iz, -fy * p[:, 1] * iz * iz
    dpr = dpr * w[:, :, None]
    Jc = np.concatenate([dpr @ dpdw, dpr], -1)
    Jc[fixed] = 0.0
    Jp = dpr @ R
    return r, Jc, Jp


def _inv3_adjugate(M):
    """Inverse of symmetric 3x3 blocks [P,3,3] through the adjugate, term for term what mvba_kernel's phase B computes."""
    m00, m10, m11, m20, m21, m22 = M[:, 0, 0], M[:, 1, 0], M[:, 1, 1], M[:, 2, 0], M[:, 2, 1], M[:, 2, 2]
    c00, c10, c20 = m11 * m22 - m21 * m21, m20 * m21 - m10 * m22, m10 * m21 - m20 * m11
    i = 1.0 / (m00 * c00 + m10 * c10 + m20 * c20)
    i00, i10, i20, i11, i21, i22 = c00 * i, c10 * i, c20 * i, (m00 * m22 - m20 * m20) * i, (m10 * m20 - m00 * m21) * i, (m00 * m11 - m10 * m10) * i
    return np.stack([np.stack([i00, i10, i20], -1), np.stack([i10, i11, i21], -1), np.stack([i20, i21, i22], -1)], -2)


def _solve_spd_unblocked(S, b):
    """S x = b by a left-looking column Cholesky and two substitutions, the order of operations of mvba_kernel's phase F
    (LAPACK blocks and pivots differently); raises LinAlgError where the kernel gives up (a pivot that is not > 0)."""
    n = len(b)
    L = np.zeros((n, n), S.dtype)
    for j in range(n):
        col = S[j:, j] - L[j:, :j] @ L[j, :j]
        if not col[0] > 0.0:
            raise np.linalg.LinAlgError("not positive definite")
        L[j:, j] = col / np.sqrt(col[0])
        L[j, j] = np.sqrt(col[0])
    x = b.copy()
    for j in range(n):
        x[j] /= L[j, j]
        x[j + 1:] -= L[j + 1:, j] * x[j]
    for j in range(n - 1, -1, -1):
        x[j] /= L[j, j]
        x[:j] -= L[j, :j] * x[j]
    return x


def solve(prob, max_iterations=50, function_tolerance=1e-6, gradient_tolerance=1e-10, parameter_tolerance=1e-8,
          return_trajectory=False, point_inverse="lapack", reduced_solver="lapack", schur_right=False, expanded_rotation=False,
          divide=False, extended_linearise=False, dtype=np.float64):
    """Returns (cams [C,6], pts [P,3], summary dict).  The fixed camera's parameters are returned untouched.  The keyword
    arguments after the tolerances are hooks of tests/test_gpu_mv_ba_steps.py; their defaults are the solver as it always was.

    return_trajectory=True appends a list of records, one for the start and one per pass through the loop: record k holds
    what solve(max_iterations=k) returns (cams, pts, cost, iterations, termination - for k beyond the last record, the last
    record), the trust region after the pass (radius, decrease), what the pass did (kind: "start", "accepted", "rejected",
    "invalid", or "stop" for a pass that ended on the parameter / function tolerance) and the quantities its decisions compared
    with their thresholds, None where the pass did not get that far: step_ratio = step_norm / (x_norm + 1e-8) against 1e-8,
    fn_ratio = |change| / cost against 1e-6, rho against 1e-3, and gmax, the gradient maximum AT record k's iterate (tested
    against 1e-10 before the iteration limit is: it decides between "gradient_tolerance" and "max_iterations" there).
    point_inverse="adjugate" inverts the 3x3 point blocks the way the kernel does instead of np.linalg.inv;
    expanded_rotation=True builds every rotation matrix entry by entry as the kernel does (see _rotate); divide=True
    predicts with a division as the reference's functors do (see linearise); reduced_solver="unblocked" solves the reduced camera
    system in the kernel's order of operations (see _solve_spd_unblocked); schur_right=True associates the Schur products to the
    right, W_a (V^-1 W_b^T) and W_a (V^-1 g_p) instead of (W_a V^-1) W_b^T and (W_a V^-1) g_p - the difference U - Y W^T cancels
    along the weakly determined directions (scale), so its rounding decides where the camera step lands there;
    extended_linearise=True evaluates residuals and Jacobians in extended precision (see linearise).  dtype=np.longdouble
    carries out the WHOLE algorithm in numpy's widest float (adjugate point blocks, unblocked reduced solve: LAPACK has no such
    type) and rounds what it returns and records to fp64: against it the fp64 run shows its own error."""
    wide = dtype is not np.float64
    if wide:
        prob = dict(prob, intr=np.asarray(prob["intr"], dtype), obs=np.asarray(prob["obs"], dtype), wts=np.asarray(prob["wts"], dtype))
        point_inverse, reduced_solver = "adjugate", "unblocked"
    num = (lambda x: x) if wide else float  # the fp64 path keeps the Python floats it always had
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

    r, Jc, Jp = linearise(prob, cams, pts, expanded_rotation, divide, extended_linearise)
    cost = 0.5 * num((r * r).sum())
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
            Vinv = _inv3_adjugate(Vd)
        elif point_inverse == "extended":  # the adjugate in the widest float there is, rounded once: LAPACK's own error shows
            Vinv = _inv3_adjugate(Vd.astype(np.longdouble)).astype(np.float64)
        elif point_inverse == "cholesky":  # Ceres' Schur eliminator inverts its point blocks through their LL^T factors
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
        # points couple the cameras that see them
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
                step_c[keep] = _solve_spd_unblocked(S[np.ix_(keep, keep)], rhs[keep])
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
        r2, Jc2, Jp2 = linearise(prob, cand_c, cand_p, expanded_rotation, divide, extended_linearise)
        cand_cost = 0.5 * num((r2 * r2).sum())
        change = cost - cand_cost
        # Ceres tests the function tolerance BEFORE it accepts the step (TrustRegionMinimizer::Minimize: ParameterTolerance-
        # Reached, FunctionToleranceReached, then IsStepSuccessful): the iterate stays at the previous point
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


VARIANTS = ("obs_reversed", "obs_shuffled", "pts_relabelled", "adjugate", "cholesky", "extended_inverse", "reduced_unblocked", "schur_right", "rotation_expanded", "projection_divided", "extended_linearise", "extended")


def solve_variant(prob, variant, seed=0, **kw):
    """solve() in other, equally legitimate fp64 arithmetic: the same problem with its observations in reverse or in a seeded
    random order (every sum over observations then runs in another order), with its points relabelled by a seeded permutation
    (sums over points), with the kernel's adjugate inverse of the point blocks, or with the kernel's entry-by-entry rotation
    matrices or the reference's division in the projection (every residual then rounds elsewhere, not only the sums).  Results - the trajectory's records too - come
    back in prob's own labelling, so they compare elementwise with solve(prob)."""
    q, back = dict(prob), None
    if variant in ("obs_reversed", "obs_shuffled"):
        O = len(prob["cam_idx"])
        order = np.arange(O)[::-1] if variant == "obs_reversed" else np.random.default_rng(seed).permutation(O)
        for k in ("cam_idx", "pt_idx", "obs", "wts"):
            q[k] = np.ascontiguousarray(np.asarray(prob[k])[order])
    elif variant == "pts_relabelled":
        perm = np.random.default_rng(seed).permutation(len(prob["pts"]))  # new point i is old point perm[i]
        back = np.argsort(perm)                                             # old point j is new point back[j]
        q["pts"] = np.asarray(prob["pts"])[perm]
        q["pt_idx"] = back[np.asarray(prob["pt_idx"])].astype(np.int32)
    elif variant == "adjugate":
        kw = dict(kw, point_inverse="adjugate")
    elif variant == "extended_inverse":
        kw = dict(kw, point_inverse="extended")
    elif variant == "reduced_unblocked":
        kw = dict(kw, reduced_solver="unblocked")
    elif variant == "schur_right":
        kw = dict(kw, schur_right=True)
    elif variant == "extended_linearise":
        kw = dict(kw, extended_linearise=True)
    elif variant == "extended":
        kw = dict(kw, dtype=np.longdouble)
    elif variant == "cholesky":
        kw = dict(kw, point_inverse="cholesky")
    elif variant == "rotation_expanded":
        kw = dict(kw, expanded_rotation=True)
    elif variant == "projection_divided":
        kw = dict(kw, divide=True)
    else:
        raise ValueError(variant)
    out = solve(q, **kw)
    if back is None:
        return out
    for rec in (out[3] if len(out) > 3 else []):
        rec["pts"] = rec["pts"][back]
    return (out[0], out[1][back]) + tuple(out[2:])


def triangulate_dlt(P0, P1, x0, x1):
    """cv2.triangulatePoints as used at bundle_adjust_io.py:226-227 (OpenCV is absent here; its algorithm is the
    homogeneous DLT: rows x*P[2]-P[0], y*P[2]-P[1] of both views, null vector by SVD).  P [3,4]; x [n,2] -> xyz [n,3]."""
    out = np.zeros((len(x0), 3))
    for i in range(len(x0)):
        A = np.stack([x0[i, 0] * P0[2] - P0[0], x0[i, 1] * P0[2] - P0[1], x1[i, 0] * P1[2] - P1[0], x1[i, 1] * P1[2] - P1[1]])
        X = np.linalg.svd(A)[2][-1]
        out[i] = X[:3] / X[3]
    return out
