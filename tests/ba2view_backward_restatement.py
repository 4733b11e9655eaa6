"""TEST HELPER (no test in here, never imported by the product path): the reverse pass of the two-view LM loop, the fp64 restatement of
what ``ba2view_backward_kernel`` (csrc/ba2view.hip) computes through ``e2emv_ba_2view_backward``.  torch fp64, NO autograd: every
adjoint is written out, in the Schur form of the kernel, so that N = 257 costs milliseconds.

Forward (``forward_tape``): the loop of ``oracle/ba2view.py`` - same start (DLT triangulation with the null vector's sign forced),
same bookkeeping -, the damped normal equations solved through the Schur complement of the 3x3 point blocks instead of a dense LU.
Per evaluation k it records X_k, Rt_k, lambda_k, the ``precond`` flag, the singular-skip flag and the camera step dc_k, and ``kstar``, the
evaluation whose pose became the result (0 when nothing improved).

Backward (``backward``): the adjoint state (Rt_bar [3,4], X_bar [M,3]) starts as (gT rows 0-2, 0) at k* and goes through the steps
k*-1 ... 0.  One LM step solves M d = b, M = A + lambda D, A = J^T J, b = -J^T r, D = diag(max(A_jj, 1e-12)) with ``precond`` else I:

    d_bar = (adjoint of exp(dc) Rt_k w.r.t. dc,  X_bar_{k+1})          w = M^-1 d_bar   (the forward's matrix, another right side)
    J_bar = -(J w) d^T - (J d + r) w^T - 2 lambda J diag(w o d) [columns with D_jj = A_jj],     r_bar = -J w

and (J_bar, r_bar) of the two observations of a match go back through ``point_terms`` to X_bar_k, Rt_bar_k and the weight's adjoint.
After k = 0 the triangulation (first-order perturbation of the null vector of G = A^T A, then 1 / (X3 + 1e-8)) and the normalisation of
the weights.  lambda, the accept / reject comparisons and k* are piecewise constant and carry nothing.

``backward`` returns (gconf [N], gTinit [4,4]).  Row 3 of gTinit is what autograd through the oracle gives it: the oracle multiplies the
4x4 matrices, so its row 3 - (0 0 0 1) - meets the step's translation; the device reads rows 0-2 only and returns a zero row 3."""
import torch

from oracle import kornia_fns as K

F64 = torch.float64


def hat(w):
    o = torch.zeros((), dtype=F64)
    return torch.stack([o, -w[2], w[1], w[2], o, -w[0], -w[1], w[0], o]).view(3, 3)


def point_terms(Rt, X, x0, x1, c):
    """Rt [3,4]; X [M,3]; x0, x1 [M,2]; c [M] -> r0, r1 [M,2], Jp0, Jp1 [M,2,3], Jc [M,2,6]: csrc/ba2view.hip point_terms."""
    M = X.shape[0]
    R, t = Rt[:, :3], Rt[:, 3]
    iz0 = 1.0 / X[:, 2]
    r0 = c[:, None] * (X[:, :2] * iz0[:, None] - x0)
    Jp0 = torch.zeros(M, 2, 3, dtype=F64)
    Jp0[:, 0, 0] = c * iz0
    Jp0[:, 1, 1] = c * iz0
    Jp0[:, 0, 2] = -c * X[:, 0] * iz0 * iz0
    Jp0[:, 1, 2] = -c * X[:, 1] * iz0 * iz0
    a = X @ R.T + t
    iz = 1.0 / a[:, 2]
    r1 = c[:, None] * (a[:, :2] * iz[:, None] - x1)
    jp = torch.zeros(M, 2, 3, dtype=F64)  # c * J_proj
    jp[:, 0, 0] = c * iz
    jp[:, 1, 1] = c * iz
    jp[:, 0, 2] = -c * a[:, 0] * iz * iz
    jp[:, 1, 2] = -c * a[:, 1] * iz * iz
    Jp1 = jp @ R
    ha = torch.zeros(M, 3, 3, dtype=F64)
    ha[:, 0, 1], ha[:, 0, 2], ha[:, 1, 0], ha[:, 1, 2], ha[:, 2, 0], ha[:, 2, 1] = -a[:, 2], a[:, 1], a[:, 2], -a[:, 0], -a[:, 1], a[:, 0]
    Jc = torch.cat([jp, -(jp @ ha)], 2)
    return r0, r1, Jp0, Jp1, Jc


def point_terms_reverse(Rt, X, x0, x1, c, r0b, r1b, Jp0b, Jp1b, Jcb):
    """Adjoint of ``point_terms``: -> (X_bar [M,3], Rt_bar [3,4] summed over the matches, c_bar [M]).  Entries of the Jacobians that are
    structurally zero take no adjoint."""
    R, t = Rt[:, :3], Rt[:, 3]
    X0, X1, X2 = X[:, 0], X[:, 1], X[:, 2]
    iz0 = 1.0 / X2
    e00, e01 = X0 * iz0 - x0[:, 0], X1 * iz0 - x0[:, 1]
    cb = r0b[:, 0] * e00 + r0b[:, 1] * e01 + (Jp0b[:, 0, 0] + Jp0b[:, 1, 1]) * iz0 - (Jp0b[:, 0, 2] * X0 + Jp0b[:, 1, 2] * X1) * iz0 * iz0
    X0b = r0b[:, 0] * c * iz0 - Jp0b[:, 0, 2] * c * iz0 * iz0
    X1b = r0b[:, 1] * c * iz0 - Jp0b[:, 1, 2] * c * iz0 * iz0
    iz0b = c * (r0b[:, 0] * X0 + r0b[:, 1] * X1) + c * (Jp0b[:, 0, 0] + Jp0b[:, 1, 1]) - 2.0 * c * iz0 * (Jp0b[:, 0, 2] * X0 + Jp0b[:, 1, 2] * X1)
    X2b = -iz0b * iz0 * iz0
    a = X @ R.T + t
    a0, a1, a2 = a[:, 0], a[:, 1], a[:, 2]
    iz = 1.0 / a2
    j00, j02, j12 = c * iz, -c * a0 * iz * iz, -c * a1 * iz * iz
    j11 = j00
    cb = cb + r1b[:, 0] * (a0 * iz - x1[:, 0]) + r1b[:, 1] * (a1 * iz - x1[:, 1])
    a0b = r1b[:, 0] * c * iz
    a1b = r1b[:, 1] * c * iz
    izb = c * (r1b[:, 0] * a0 + r1b[:, 1] * a1)
    j00b = Jp1b[:, 0] @ R[0] + Jcb[:, 0, 0] + Jcb[:, 0, 4] * a2 - Jcb[:, 0, 5] * a1
    j02b = Jp1b[:, 0] @ R[2] + Jcb[:, 0, 2] + Jcb[:, 0, 3] * a1 - Jcb[:, 0, 4] * a0
    j11b = Jp1b[:, 1] @ R[1] + Jcb[:, 1, 1] - Jcb[:, 1, 3] * a2 + Jcb[:, 1, 5] * a0
    j12b = Jp1b[:, 1] @ R[2] + Jcb[:, 1, 2] + Jcb[:, 1, 3] * a1 - Jcb[:, 1, 4] * a0
    Rb = torch.zeros(3, 3, dtype=F64)
    Rb[0] = (Jp1b[:, 0] * j00[:, None]).sum(0)
    Rb[1] = (Jp1b[:, 1] * j11[:, None]).sum(0)
    Rb[2] = (Jp1b[:, 0] * j02[:, None] + Jp1b[:, 1] * j12[:, None]).sum(0)
    a0b = a0b - Jcb[:, 0, 4] * j02 - Jcb[:, 1, 4] * j12 + Jcb[:, 1, 5] * j11
    a1b = a1b + Jcb[:, 0, 3] * j02 - Jcb[:, 0, 5] * j00 + Jcb[:, 1, 3] * j12
    a2b = Jcb[:, 0, 4] * j00 - Jcb[:, 1, 3] * j11
    cb = cb + (j00b + j11b) * iz - (j02b * a0 + j12b * a1) * iz * iz
    izb = izb + (j00b + j11b) * c - 2.0 * c * iz * (j02b * a0 + j12b * a1)
    a0b = a0b - j02b * c * iz * iz
    a1b = a1b - j12b * c * iz * iz
    a2b = a2b - izb * iz * iz
    ab = torch.stack([a0b, a1b, a2b], 1)
    Rb = Rb + ab.T @ X
    Xb = torch.stack([X0b, X1b, X2b], 1) + ab @ R
    return Xb, torch.cat([Rb, ab.sum(0)[:, None]], 1), cb


def exp_coefficients(w):
    """(clamped, th, f1, f2, f3) of pytorch3d's se3_exp_map with its 1e-4 clamp of |w|^2."""
    n2 = (w * w).sum()
    clamped = bool(n2 < 1e-4)
    th = torch.clamp(n2, min=1e-4).sqrt()
    return clamped, th, th.sin() / th, (1.0 - th.cos()) / th ** 2, (th - th.sin()) / th ** 3


def exp_step(dc, Rt):
    """Rt [3,4] <- exp(dc) Rt with the bottom row (0 0 0 1) understood."""
    v, w = dc[:3], dc[3:]
    _, _, f1, f2, f3 = exp_coefficients(w)
    Kx = hat(w)
    K2 = Kx @ Kx
    eye = torch.eye(3, dtype=F64)
    Rd, Vm = eye + f1 * Kx + f2 * K2, eye + f2 * Kx + f3 * K2
    out = Rd @ Rt
    out[:, 3] += Vm @ v
    return out


def exp_step_reverse(dc, Rt, Rtb_next):
    """Adjoint of ``exp_step``: -> (dc_bar [6], the part of Rt_bar [3,4] that comes through the product, row-3 adjoint [4]).  In the clamped
    branch f1, f2, f3 are constants and the derivative flows through hat(w) only."""
    v, w = dc[:3], dc[3:]
    clamped, th, f1, f2, f3 = exp_coefficients(w)
    Kx = hat(w)
    K2 = Kx @ Kx
    eye = torch.eye(3, dtype=F64)
    Rd, Vm = eye + f1 * Kx + f2 * K2, eye + f2 * Kx + f3 * K2
    Rdb = Rtb_next @ Rt.T          # R part and t part at once: Rn = Rd R, tn = Rd t + td
    tdb = Rtb_next[:, 3]
    Vmb = torch.outer(tdb, v)
    vb = Vm.T @ tdb
    f1b, f2b, f3b = (Rdb * Kx).sum(), (Rdb * K2).sum() + (Vmb * Kx).sum(), (Vmb * K2).sum()
    K2b = f2 * Rdb + f3 * Vmb
    Kxb = f1 * Rdb + f2 * Vmb + K2b @ Kx.T + Kx.T @ K2b
    wb = torch.stack([Kxb[2, 1] - Kxb[1, 2], Kxb[0, 2] - Kxb[2, 0], Kxb[1, 0] - Kxb[0, 1]])
    if not clamped:
        s, c = th.sin(), th.cos()
        thb = f1b * (th * c - s) / th ** 2 + f2b * (th * s - 2.0 * (1.0 - c)) / th ** 3 + f3b * ((1.0 - c) * th - 3.0 * (th - s)) / th ** 4
        wb = wb + thb * w / th
    td = Vm @ v
    return torch.cat([vb, wb]), Rd.T @ Rtb_next, td @ Rtb_next


def _inv3(H):
    return torch.linalg.inv(H)


def lm_step(Rt, X, x0, x1, c, lam):
    """One LM step in the Schur form.  -> dict with the step (dc [6], dp [M,3]), ``precond``, ``ok`` and what the reverse needs."""
    r0, r1, Jp0, Jp1, Jc = point_terms(Rt, X, x0, x1, c)
    Hcc = (Jc.transpose(1, 2) @ Jc).sum(0)
    gc = -(Jc.transpose(1, 2) @ r1[:, :, None]).sum(0)[:, 0]
    Hpp = Jp0.transpose(1, 2) @ Jp0 + Jp1.transpose(1, 2) @ Jp1
    gp = -((Jp0.transpose(1, 2) @ r0[:, :, None]) + (Jp1.transpose(1, 2) @ r1[:, :, None]))[:, :, 0]
    Hcp = Jc.transpose(1, 2) @ Jp1  # [M,6,3]
    dpp, dcc = torch.diagonal(Hpp, dim1=1, dim2=2), torch.diagonal(Hcc)
    precond = bool((dpp > 0).all()) and bool((dcc > 0).all())
    Dp = dpp.clamp(min=1e-12) if precond else torch.ones_like(dpp)
    Dc = dcc.clamp(min=1e-12) if precond else torch.ones_like(dcc)
    Hppd = Hpp + lam * torch.diag_embed(Dp)
    inv = _inv3(Hppd)
    W = Hcp @ inv
    S = Hcc + lam * torch.diag(Dc) - (W @ Hcp.transpose(1, 2)).sum(0)
    rhs = gc - (W @ gp[:, :, None]).sum(0)[:, 0]
    LU, piv, info = torch.linalg.lu_factor_ex(S)
    st = dict(r0=r0, r1=r1, Jp0=Jp0, Jp1=Jp1, Jc=Jc, Hcp=Hcp, inv=inv, LU=LU, piv=piv, precond=precond, lam=lam, dpp=dpp, dcc=dcc,
              ok=int(info) == 0, cost=(r0 ** 2).sum() + (r1 ** 2).sum())
    if not st["ok"]:
        return st
    dc = torch.linalg.lu_solve(LU, piv, rhs[:, None])[:, 0]
    dp = (inv @ (gp - (Hcp.transpose(1, 2) @ dc))[:, :, None])[:, :, 0]
    st.update(dc=dc, dp=dp)
    return st


def lm_step_reverse(st, Rt, X, x0, x1, c, dcb, dpb):
    """Adjoint of ``lm_step`` for (dc_bar [6], dp_bar [M,3]) -> (X_bar [M,3], Rt_bar [3,4], c_bar [M]) THROUGH the step only."""
    Jp0, Jp1, Jc, r0, r1, Hcp, inv, lam = st["Jp0"], st["Jp1"], st["Jc"], st["r0"], st["r1"], st["Hcp"], st["inv"], st["lam"]
    dc, dp = st["dc"], st["dp"]
    # M w = d_bar through the same Schur complement
    W = Hcp @ inv
    rhs = dcb - (W @ dpb[:, :, None]).sum(0)[:, 0]
    wc = torch.linalg.lu_solve(st["LU"], st["piv"], rhs[:, None])[:, 0]
    wp = (inv @ (dpb - (Hcp.transpose(1, 2) @ wc))[:, :, None])[:, :, 0]
    jd0, jw0 = (Jp0 @ dp[:, :, None])[:, :, 0], (Jp0 @ wp[:, :, None])[:, :, 0]
    jd1 = Jc @ dc + (Jp1 @ dp[:, :, None])[:, :, 0]
    jw1 = Jc @ wc + (Jp1 @ wp[:, :, None])[:, :, 0]
    if st["precond"]:
        mp = (st["dpp"] >= 1e-12).to(F64) * (2.0 * lam)
        mc = (st["dcc"] >= 1e-12).to(F64) * (2.0 * lam)
    else:
        mp, mc = torch.zeros_like(st["dpp"]), torch.zeros_like(st["dcc"])
    wdp, wdc = mp * wp * dp, mc * wc * dc
    Jp0b = -jw0[:, :, None] * dp[:, None, :] - (jd0 + r0)[:, :, None] * wp[:, None, :] - Jp0 * wdp[:, None, :]
    Jp1b = -jw1[:, :, None] * dp[:, None, :] - (jd1 + r1)[:, :, None] * wp[:, None, :] - Jp1 * wdp[:, None, :]
    Jcb = -jw1[:, :, None] * dc[None, None, :] - (jd1 + r1)[:, :, None] * wc[None, None, :] - Jc * wdc[None, None, :]
    return point_terms_reverse(Rt, X, x0, x1, c, -jw0, -jw1, Jp0b, Jp1b, Jcb)


def triangulate(Rt, x0, x1, sign):
    P0 = torch.eye(4, dtype=F64)[:3]
    h = K.triangulate_points_homogeneous(P0[None], Rt[None], x0[None], x1[None])[0]
    flip = torch.where(torch.signbit(h[:, 3:]) != (sign < 0), -torch.ones_like(h[:, 3:]), torch.ones_like(h[:, 3:]))
    return K.convert_points_from_homogeneous(h * flip)


def triangulate_reverse(Rt, x0, x1, sign, Xb):
    """Adjoint of ``triangulate`` w.r.t. Rt: dv = -sum_{j != m} v_j v_j^T dG v / (l_j - l_m) for the null vector of G = A^T A."""
    M = x0.shape[0]
    A = torch.zeros(M, 4, 4, dtype=F64)
    A[:, 0, 0], A[:, 0, 2], A[:, 1, 1], A[:, 1, 2] = -1.0, x0[:, 0], -1.0, x0[:, 1]
    A[:, 2] = x1[:, :1] * Rt[2] - Rt[0]
    A[:, 3] = x1[:, 1:] * Rt[2] - Rt[1]
    lam, V = torch.linalg.eigh(A.transpose(1, 2) @ A)  # ascending: the null vector is column 0
    v = V[:, :, 0]
    v = v * torch.where(torch.signbit(v[:, 3:]) != (sign < 0), -torch.ones_like(v[:, 3:]), torch.ones_like(v[:, 3:]))
    big = v[:, 3].abs() > 1e-8
    sc = torch.where(big, 1.0 / (v[:, 3] + 1e-8), torch.ones_like(v[:, 3]))
    vb = torch.zeros(M, 4, dtype=F64)
    vb[:, :3] = Xb * sc[:, None]
    vb[:, 3] = torch.where(big, -(Xb * v[:, :3]).sum(1) * sc * sc, torch.zeros_like(sc))
    Gb = torch.zeros(M, 4, 4, dtype=F64)
    for j in range(1, 4):
        coef = -(V[:, :, j] * vb).sum(1) / (lam[:, j] - lam[:, 0])
        Gb = Gb + coef[:, None, None] * V[:, :, j][:, :, None] * v[:, None, :]
    Ab = A @ (Gb + Gb.transpose(1, 2))
    Rtb = torch.zeros(3, 4, dtype=F64)
    Rtb[0] = -Ab[:, 2].sum(0)
    Rtb[1] = -Ab[:, 3].sum(0)
    Rtb[2] = (x1[:, :1] * Ab[:, 2] + x1[:, 1:] * Ab[:, 3]).sum(0)
    return Rtb


def forward_tape(k0, k1, conf, T_init, n_iterations, sign, lm_increase=1.5, lm_decrease=3.5):
    """One sample: k0, k1 [N,2], conf [N], T_init [4,4] fp64.  -> None for an invalid sample, else the tape (a dict)."""
    m = conf > 0.0
    if int(m.sum()) <= 6:
        return None
    x0, x1, cf = k0[m], k1[m], conf[m]
    csum = 2 * cf.sum()
    cden = 0.5 * csum.clamp(min=1e-6)
    c = cf / cden
    Rt = T_init[:3].clone()
    X = triangulate(Rt, x0, x1, sign)
    lam, best_r, kstar = 0.1, None, 0
    tape = dict(mask=m, x0=x0, x1=x1, cf=cf, c=c, cden=cden, csum=csum, sign=sign, steps=[], cost=[], accepted=[], best_before=[])
    for it in range(n_iterations + 1):
        r0, r1 = point_terms(Rt, X, x0, x1, c)[:2]
        rn = (r0 ** 2).sum() + (r1 ** 2).sum()
        tape["cost"].append(float(rn))
        tape["best_before"].append(float("nan") if it == 0 else float(best_r))
        if it == 0:
            best_r = rn
            tape["accepted"].append(True)
        elif bool(rn < best_r):
            best_r, kstar = rn, it
            lam = lam / lm_decrease
            tape["accepted"].append(True)
        else:
            lam = lam * lm_increase
            tape["accepted"].append(False)
        if it == n_iterations:
            break
        st = lm_step(Rt, X, x0, x1, c, lam)
        st.update(Rt=Rt, X=X)
        tape["steps"].append(st)
        if not st["ok"]:
            continue
        Rt = exp_step(st["dc"], Rt)
        X = X + st["dp"]
    tape["kstar"] = kstar
    tape["best"] = tape["steps"][kstar]["Rt"] if kstar < len(tape["steps"]) else Rt
    return tape


def backward(tape, gT, N):
    """gT [4,4] (rows 0-2 used) -> (gconf [N], gTinit [4,4]) of one valid sample."""
    x0, x1, c = tape["x0"], tape["x1"], tape["c"]
    Rtb = gT[:3].clone().to(F64)
    row3 = torch.zeros(4, dtype=F64)
    Xb = torch.zeros(x0.shape[0], 3, dtype=F64)
    cb = torch.zeros(x0.shape[0], dtype=F64)
    gconf = torch.zeros(N, dtype=F64)
    gTinit = torch.zeros(4, 4, dtype=F64)
    if tape["kstar"] > 0:
        for k in range(tape["kstar"] - 1, -1, -1):
            st = tape["steps"][k]
            if not st["ok"]:
                continue
            dcb, Rtb_through, r3 = exp_step_reverse(st["dc"], st["Rt"], Rtb)
            dX, dRt, dcw = lm_step_reverse(st, st["Rt"], st["X"], x0, x1, c, dcb, Xb)
            Xb, Rtb, cb, row3 = Xb + dX, Rtb_through + dRt, cb + dcw, row3 + r3
        Rtb = Rtb + triangulate_reverse(tape["steps"][0]["Rt"], x0, x1, tape["sign"], Xb)
        g = cb / tape["cden"]
        if float(tape["csum"]) >= 1e-6:
            g = g - (cb * c).sum() / tape["cden"]
        gconf[tape["mask"]] = g
    gTinit[:3], gTinit[3] = Rtb, row3
    return gconf, gTinit


def run(k0, k1, conf, T_init, n_iterations, gT, sign):
    """Batched front: k0, k1 [B,N,2], conf [B,N], T_init, gT [B,4,4] -> (T [B,4,4], valid [B], gconf [B,N], gTinit [B,4,4], tapes).
    An invalid sample returns T_init, gconf = 0 and gTinit = rows 0-2 of gT."""
    k0, k1, conf, T_init, gT = (t.to(F64) for t in (k0, k1, conf, T_init, gT))
    B, N = conf.shape
    T, gconf, gTi, tapes = T_init.clone(), torch.zeros(B, N, dtype=F64), torch.zeros(B, 4, 4, dtype=F64), []
    valid = torch.zeros(B, dtype=torch.bool)
    for b in range(B):
        tape = forward_tape(k0[b], k1[b], conf[b], T_init[b], n_iterations, sign)
        tapes.append(tape)
        if tape is None:
            gTi[b, :3] = gT[b, :3]
            continue
        valid[b] = True
        T[b, :3] = tape["best"]
        gconf[b], gTi[b] = backward(tape, gT[b], N)
    return T, valid, gconf, gTi, tapes
