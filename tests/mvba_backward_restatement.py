"""TEST INFRASTRUCTURE: torch fp64 restatement of the LM loop of mvba_kernel<kLossNone, MODE> (csrc/mvba.h), differentiable by autograd, and the
scenes the backward tests share (tests/test_mv_ba_backward.py on the CPU, tests/test_gpu_mv_ba_backward.py on the device).

The loop follows the kernel phase for phase: A residuals r = w (.) (pi(R(omega) X + t) - obs) with the ANALYTIC Jacobians of mv_transform
(Rodrigues for theta^2 > eps, first order below; the fixed camera is the identity and has a zero camera block), C / B the blocks U, V
and the gradients, D the damping clamp(diag s^2, 1e-6, 1e32) / radius / s^2, the adjugate inverse of the point blocks, E the Schur
complement, F a Cholesky solve, G the point steps, H the model cost change and the candidate cost, I the decisions.  Autograd through the
analytic Jacobians yields the second derivatives the device takes with tangent-carrying numbers.

FROZEN (detached or plain floats), exactly the list of csrc/mvba_backward.hip: the radius including its rho-dependent update, the Jacobi
scales of the first iterate, the accept / reject comparisons, every termination test, obs_xy and the intrinsics.  torch.clamp hands a
clamped damping no gradient (a column on a clamp has a constant lambda).  An unsolved or rejected pass leaves the iterate untouched.

run(...) decides for itself and records a SCHEDULE: the scales of the first iterate and (radius, solved, accepted) per pass.
run(..., schedule=s) replays with that schedule instead of deciding - what central finite differences are taken of, so that a perturbed
input cannot move a decision, the radius or a scale."""
import numpy as np
import torch

from oracle import mvba

EPS = 2.220446049250313e-16
TERMS = ["max_iterations", "gradient_tolerance", "parameter_tolerance", "function_tolerance", "invalid_steps", "radius"]


def _hat(v):
    z = torch.zeros_like(v[:, 0])
    return torch.stack([torch.stack([z, -v[:, 2], v[:, 1]], -1), torch.stack([v[:, 2], z, -v[:, 0]], -1), torch.stack([-v[:, 1], v[:, 0], z], -1)], -2)


def transform(cam, X):
    """mv_transform for rows of cameras [O,6] and points [O,3]: p [O,3], R [O,3,3], D = dp/dw [O,3,3]."""
    w = cam[:, :3]
    t2 = (w * w).sum(-1)
    big = t2 > EPS
    t2s = torch.where(big, t2, torch.ones_like(t2))
    th = torch.sqrt(t2s)
    k = w / th[:, None]
    s, c = torch.sin(th), torch.cos(th)
    v = 1.0 - c
    k0, k1, k2 = k[:, 0], k[:, 1], k[:, 2]
    Rb = torch.stack([1 - v * (k1 * k1 + k2 * k2), -s * k2 + v * k0 * k1, s * k1 + v * k0 * k2,
                      s * k2 + v * k0 * k1, 1 - v * (k0 * k0 + k2 * k2), -s * k0 + v * k1 * k2,
                      -s * k1 + v * k0 * k2, s * k0 + v * k1 * k2, 1 - v * (k0 * k0 + k1 * k1)], -1).reshape(-1, 3, 3)
    I = torch.eye(3, dtype=cam.dtype).expand(len(cam), 3, 3)
    wh, Xh = _hat(w), _hat(X)
    R = torch.where(big[:, None, None], Rb, I + wh)
    p = (R @ X[:, :, None])[:, :, 0] + cam[:, 3:]
    G = (w[:, :, None] * w[:, None, :] + (Rb.transpose(1, 2) - I) @ wh) / t2s[:, None, None]
    D = torch.where(big[:, None, None], -(Rb @ (Xh @ G)), -Xh)
    return p, R, D


def linearise(prob, cams, pts, wts):
    """Phase A: r [O,2], Jc [O,2,6] (zero for the fixed camera), Jp [O,2,3]."""
    ci, pi = prob["ci"], prob["pi"]
    fx, fy, cx, cy = prob["intr"]
    fixed = ci == prob["fixed"]
    cam = torch.where(fixed[:, None], torch.zeros_like(cams[ci]), cams[ci])  # the identity pose
    q, R, D = transform(cam, pts[pi])
    iz = 1.0 / q[:, 2]
    r = torch.stack([wts[:, 0] * (fx * q[:, 0] * iz + cx - prob["obs"][:, 0]), wts[:, 1] * (fy * q[:, 1] * iz + cy - prob["obs"][:, 1])], -1)
    z = torch.zeros_like(iz)
    E = torch.stack([torch.stack([wts[:, 0] * fx * iz, z, -wts[:, 0] * fx * q[:, 0] * iz * iz], -1),
                     torch.stack([z, wts[:, 1] * fy * iz, -wts[:, 1] * fy * q[:, 1] * iz * iz], -1)], -2)  # d(residual)/d(q) [O,2,3]
    Jc = torch.cat([E @ D, E], -1) * (~fixed)[:, None, None]
    return r, Jc, E @ R


def _inv3(M):
    m00, m10, m11, m20, m21, m22 = M[:, 0, 0], M[:, 1, 0], M[:, 1, 1], M[:, 2, 0], M[:, 2, 1], M[:, 2, 2]
    c00, c10, c20 = m11 * m22 - m21 * m21, m20 * m21 - m10 * m22, m10 * m21 - m20 * m11
    i = 1.0 / (m00 * c00 + m10 * c10 + m20 * c20)
    i00, i10, i20, i11, i21, i22 = c00 * i, c10 * i, c20 * i, (m00 * m22 - m20 * m20) * i, (m10 * m20 - m00 * m21) * i, (m00 * m11 - m10 * m10) * i
    return torch.stack([torch.stack([i00, i10, i20], -1), torch.stack([i10, i11, i21], -1), torch.stack([i20, i21, i22], -1)], -2)


def _tensors(prob):
    ci, pi = torch.as_tensor(np.asarray(prob["cam_idx"], np.int64)), torch.as_tensor(np.asarray(prob["pt_idx"], np.int64))
    C, P = len(prob["cams"]), len(prob["pts"])
    # pairs (a, b) of observations of the same point (a == b included): the couplings of the Schur complement
    A, B = np.nonzero(np.asarray(prob["pt_idx"])[:, None] == np.asarray(prob["pt_idx"])[None, :])
    free = torch.tensor([c != prob["fixed"] for c in range(C)])
    return dict(ci=ci, pi=pi, C=C, P=P, fixed=int(prob["fixed"]), intr=[float(x) for x in prob["intr"]], A=torch.as_tensor(A), B=torch.as_tensor(B),
                obs=torch.as_tensor(np.asarray(prob["obs"], np.float64)), free=free, keep=free.repeat_interleave(6))


def _step(T, cams, pts, wts, r, Jc, Jp, radius, scale_c, scale_p):
    """Phases C - G at one iterate: (solved, step_c [C,6], step_p [P,3], gmax)."""
    ci, pi, C, P = T["ci"], T["pi"], T["C"], T["P"]
    dd = cams.dtype
    U = torch.zeros(C, 6, 6, dtype=dd).index_add(0, ci, Jc.transpose(1, 2) @ Jc)
    gc = torch.zeros(C, 6, dtype=dd).index_add(0, ci, (Jc.transpose(1, 2) @ r[:, :, None])[:, :, 0])
    V = torch.zeros(P, 3, 3, dtype=dd).index_add(0, pi, Jp.transpose(1, 2) @ Jp)
    gp = torch.zeros(P, 3, dtype=dd).index_add(0, pi, (Jp.transpose(1, 2) @ r[:, :, None])[:, :, 0])
    dc, dp = torch.diagonal(U, dim1=1, dim2=2), torch.diagonal(V, dim1=1, dim2=2)
    lam_c = torch.clamp(dc * scale_c ** 2, 1e-6, 1e32) / radius / scale_c ** 2
    lam_p = torch.clamp(dp * scale_p ** 2, 1e-6, 1e32) / radius / scale_p ** 2
    Vinv = _inv3(V + torch.diag_embed(lam_p))
    W = Jc.transpose(1, 2) @ Jp  # [O,6,3]
    Y = W @ Vinv[pi]
    S = (U + torch.diag_embed(lam_c))[:, None] * torch.eye(C, dtype=dd)[:, :, None, None]  # [C,C,6,6]
    S = S.reshape(C * C, 6, 6).index_add(0, ci[T["A"]] * C + ci[T["B"]], -(Y[T["A"]] @ W[T["B"]].transpose(1, 2)))
    S = S.reshape(C, C, 6, 6).permute(0, 2, 1, 3).reshape(6 * C, 6 * C)
    rhs = (-gc).index_add(0, ci, (Y @ gp[pi][:, :, None])[:, :, 0]).reshape(6 * C)
    keep = T["keep"]
    Sk, bk = S[keep][:, keep], rhs[keep]
    Lf, info = torch.linalg.cholesky_ex(Sk)
    if int(info) != 0:
        return False, None, None
    xk = torch.cholesky_solve(bk[:, None], Lf)[:, 0]
    step_c = torch.zeros(6 * C, dtype=dd).index_put((torch.nonzero(keep)[:, 0],), xk).reshape(C, 6)
    acc = gp.index_add(0, pi, (W.transpose(1, 2) @ step_c[ci][:, :, None])[:, :, 0])
    step_p = -(Vinv @ acc[:, :, None])[:, :, 0]
    return True, step_c, step_p


def _gmax(T, r, Jc, Jp):
    gc = torch.zeros(T["C"], 6, dtype=r.dtype).index_add(0, T["ci"], (Jc.transpose(1, 2) @ r[:, :, None])[:, :, 0])
    gp = torch.zeros(T["P"], 3, dtype=r.dtype).index_add(0, T["pi"], (Jp.transpose(1, 2) @ r[:, :, None])[:, :, 0])
    gc, gp = gc.detach(), gp.detach()
    return max(float(gc[T["free"]].abs().max()) if bool(T["free"].any()) else 0.0, float(gp.abs().max()) if T["P"] else 0.0)


def _scales(T, Jc, Jp):
    U = torch.zeros(T["C"], 6, dtype=Jc.dtype).index_add(0, T["ci"], (Jc * Jc).sum(1))
    V = torch.zeros(T["P"], 3, dtype=Jc.dtype).index_add(0, T["pi"], (Jp * Jp).sum(1))
    return (1.0 / (1.0 + torch.sqrt(U))).detach(), (1.0 / (1.0 + torch.sqrt(V))).detach()


def run(prob, cams, pts, wts, max_iterations=50, schedule=None):
    """The loop.  cams [C,6], pts [P,3], wts [O,2]: fp64 tensors (with or without a graph); prob: the oracle's dict (its cams / pts / wts
    give the sizes only).  Returns (cams_out, pts_out, info): info["schedule"], info["iterations"], info["termination"], info["costs"]
    (initial, final), info["trajectory"] = per pass (cams, pts, cost) after it, info["margins"] = every quantity a decision compared with
    its threshold as (name, value, threshold)."""
    T = _tensors(prob)
    free = T["free"]
    if schedule is not None:
        scale_c, scale_p = schedule["scale_c"], schedule["scale_p"]
        for radius, solved, accepted in schedule["passes"]:
            if not (solved and accepted):
                continue
            r, Jc, Jp = linearise(T, cams, pts, wts)
            ok, step_c, step_p = _step(T, cams, pts, wts, r, Jc, Jp, radius, scale_c, scale_p)
            assert ok
            cams, pts = cams + step_c * free[:, None], pts + step_p
        return cams, pts, dict(schedule=schedule)
    radius, decrease, invalid, it, term = 1e4, 2.0, 0, 0, 0
    passes, traj, margins = [], [], []
    scale_c = scale_p = None
    r, Jc, Jp = linearise(T, cams, pts, wts)
    cost = 0.5 * float((r * r).sum().detach())
    cost0 = cost
    while True:
        if scale_c is None:
            scale_c, scale_p = _scales(T, Jc, Jp)
        gmax = _gmax(T, r, Jc, Jp)
        margins.append(("gmax", gmax, 1e-10))
        if gmax <= 1e-10:
            term = 1
            break
        if it >= max_iterations:
            break
        it += 1
        used = radius
        ok, step_c, step_p = _step(T, cams, pts, wts, r, Jc, Jp, radius, scale_c, scale_p)
        solved, accepted = ok, False
        if ok:
            m = (Jc @ step_c[T["ci"]][:, :, None])[:, :, 0] + (Jp @ step_p[T["pi"]][:, :, None])[:, :, 0]
            model = -float((m * (r + 0.5 * m)).sum().detach())
            ok = model > 0.0
        stop = False
        if not ok:
            invalid += 1
            if invalid >= 5:
                term, stop = 4, True
            radius /= decrease
            decrease *= 2.0
        else:
            invalid = 0
            step_norm = float(torch.sqrt((step_c[free] ** 2).sum() + (step_p ** 2).sum()).detach())
            x_norm = float(torch.sqrt((cams[free] ** 2).sum() + (pts ** 2).sum()).detach())
            margins.append(("step_ratio", step_norm / (x_norm + 1e-8), 1e-8))
            if step_norm <= 1e-8 * (x_norm + 1e-8):
                term, stop = 2, True
            else:
                cand_c, cand_p = cams + step_c * free[:, None], pts + step_p
                r2, Jc2, Jp2 = linearise(T, cand_c, cand_p, wts)
                cand_cost = 0.5 * float((r2 * r2).sum().detach())
                change = cost - cand_cost
                margins.append(("fn_ratio", abs(change) / cost, 1e-6))
                if abs(change) <= 1e-6 * cost:
                    term, stop = 3, True
                else:
                    rho = change / model
                    margins.append(("rho", rho, 1e-3))
                    if rho > 1e-3:
                        accepted = True
                        cams, pts, r, Jc, Jp, cost = cand_c, cand_p, r2, Jc2, Jp2, cand_cost
                        radius = min(1e16, radius / max(1.0 / 3.0, 1.0 - (2.0 * rho - 1.0) ** 3))
                        decrease = 2.0
                    else:
                        radius /= decrease
                        decrease *= 2.0
                    if radius < 1e-32:
                        term, stop = 5, True
        passes.append((used, bool(solved), bool(accepted)))
        traj.append((cams.detach().numpy().copy(), pts.detach().numpy().copy(), cost))
        if stop:
            break
    info = dict(schedule=dict(scale_c=scale_c, scale_p=scale_p, passes=passes), iterations=it, termination=TERMS[term], costs=(cost0, cost),
                trajectory=traj, margins=margins)
    return cams, pts, info


def gradients(prob, max_iterations, g_cams, g_pts=None, schedule=None):
    """(g_obs_w, g_cams0, g_pts0, info) of <g_cams, cams_out> + <g_pts, pts_out> by autograd through run()."""
    cams = torch.tensor(np.asarray(prob["cams"], np.float64), requires_grad=True)
    pts = torch.tensor(np.asarray(prob["pts"], np.float64), requires_grad=True)
    wts = torch.tensor(np.asarray(prob["wts"], np.float64), requires_grad=True)
    co, po, info = run(prob, cams, pts, wts, max_iterations, schedule)
    loss = (co * torch.as_tensor(g_cams)).sum()
    if g_pts is not None:
        loss = loss + (po * torch.as_tensor(g_pts)).sum()
    gw, gc, gp = torch.autograd.grad(loss, [wts, cams, pts], allow_unused=True)
    z = lambda g, x: np.zeros(x.shape) if g is None else g.numpy()  # noqa: E731
    return z(gw, wts), z(gc, cams), z(gp, pts), info


# ---- the scenes (planted, noisy, in the style of tests/test_gpu_mv_ba_steps.py) --------------------------------------------------------
def make_scene(seed, C, P, fixed=0, views=2, perturb=0.03, noise=2e-3, tracks=None, blind=None, aniso=True):
    """True cameras near the identity looking at points 4..8 in front of them; point p is seen by `views` distinct cameras (or by
    tracks[p] of them); `blind`: a camera that sees nothing.  The fixed camera is the identity in truth and has an arbitrary stored row."""
    rng = np.random.default_rng(seed)
    cams = np.concatenate([rng.normal(0, 0.25, (C, 3)), rng.normal(0, 0.4, (C, 3))], 1)
    if fixed >= 0:
        cams[fixed] = 0.0
    pts = np.stack([rng.uniform(-2, 2, P), rng.uniform(-2, 2, P), rng.uniform(4, 8, P)], 1)
    seeing = [c for c in range(C) if c != blind]
    ci, pi = [], []
    for p in range(P):
        k = views if tracks is None else tracks[p]
        ci += list(rng.choice(seeing, size=k, replace=False)) if k < len(seeing) else seeing
        pi += [p] * min(k, len(seeing))
    ci, pi = np.array(ci, np.int32), np.array(pi, np.int32)
    q = np.stack([mvba.aa_to_R(cams[c, :3]) @ pts[p] + cams[c, 3:] for c, p in zip(ci, pi)])
    assert q[:, 2].min() > 1.0
    obs = q[:, :2] / q[:, 2:] + noise * rng.normal(size=(len(ci), 2))
    w = rng.uniform(0.2, 2.0, (len(ci), 2))
    if not aniso:
        w[:, 1] = w[:, 0]
    start = cams + rng.normal(0, perturb, (C, 6))
    if fixed >= 0:
        start[fixed] = rng.normal(0, 0.3, 6)  # a stored row that is NOT the pose the solver uses
    return dict(n_cams=C, fixed=fixed, intr=np.array([1.0, 1.0, 0.0, 0.0]), cam_idx=ci, pt_idx=pi, obs=obs, wts=w, cams=start,
                pts=pts + rng.normal(0, perturb, pts.shape))


# name -> (builder, cotangent on the points too).  Seeds are chosen so that the premise tests of tests/test_mv_ba_backward.py hold for the
# restatement alone, never by what the device returns.
CASES = {
    "minimal": (lambda: make_scene(31, C=2, P=8), False),                                         # the smallest problem
    "dense_fixed_mid": (lambda: make_scene(32, C=3, P=180, fixed=1, views=3), True),              # O = 540 > 512, camera lists of 180 > 64
    "many_points": (lambda: make_scene(33, C=3, P=520), False),                                   # more points than threads
    "mixed_tracks": (lambda: make_scene(34, C=8, P=40, tracks=[2 + p % 7 for p in range(40)]), True),  # track lengths 2..8, 28 blocks on 8 waves
    "blind_camera": (lambda: make_scene(35, C=4, P=30, blind=2), False),                          # camera 2 without observations
    "far_start": (lambda: make_scene(36, C=3, P=30, perturb=0.24), True),                         # rejected steps, the radius shrinks
    "exact": (lambda: make_scene(37, C=3, P=30, noise=0.0, perturb=0.0), False),                  # stops on the gradient tolerance at once
}
ITERATIONS = [0, 1, 3, 50]


def cotangent(prob, seed, with_points):
    rng = np.random.default_rng(1000 + seed)
    g_cams = rng.normal(size=np.asarray(prob["cams"]).shape)
    return g_cams, (rng.normal(size=np.asarray(prob["pts"]).shape) if with_points else None)
