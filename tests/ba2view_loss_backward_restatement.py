"""TEST HELPER (no test in here, never imported by the product path): the reverse pass of the two-view LM loop WITH A ROBUST LOSS, the
fp64 restatement of what ``ba2view_backward_kernel<LOSS>`` (csrc/ba2view.hip) computes through ``e2emv_ba_2view_loss_backward``.

(a) ``run_autograd``: the dense robust loop of tests/ba2view_loss_restatement.py, statement for statement, with the pair's scale
    ``a = loss_scale / cden`` kept as a TENSOR (that file detaches it with ``float()``), so that ``torch.autograd`` reaches the confidences
    through the scale as well.  The trajectory's ``best`` carries the graph.

(b) ``forward_tape`` / ``backward`` / ``run``: the reverse written out by hand in the Schur form of the kernel, no autograd.  It reuses
    ``point_terms``, ``point_terms_reverse``, ``exp_step``, ``exp_step_reverse``, ``triangulate`` and ``triangulate_reverse`` of
    tests/ba2view_backward_restatement.py; the LM step and its reverse are that file's with the corrector in between.  The step solves the
    CORRECTED system ``r~ = sq r``, ``J~ = sq J`` per observation block (block 0: r0, Jp0; block 1: r1, Jp1, Jc), ``sq = sqrt(rho'(s))``,
    ``s = |r|^2`` of the uncorrected weighted residual; its reverse gives the adjoint of (r~, J~), and per block

        sq_bar = <r~_bar, r> + <J~_bar, J>       r_bar = sq r~_bar + 2 (dsq/ds) sq_bar r       J_bar = sq J~_bar       a_bar += (dsq/da) sq_bar
        cauchy: dsq/ds = -sq^3 / (2 a^2), dsq/da = sq^3 s / a^3        huber: s <= a^2: both 0, else dsq/ds = -sq / (4 s), dsq/da = sq / (2 a)

    before ``point_terms_reverse`` runs on (r_bar, J_bar).  ``a = loss_scale / cden`` and ``cden = sum conf`` while ``2 sum conf >= 1e-6``:
    every positive-confidence row gets ``-a_bar a / cden`` on top (``scale_gradient=False`` leaves that term out: ``a`` detached).  ``rho``
    itself, lambda, the comparisons and k* carry nothing.  ``loss=None`` performs the operations of tests/ba2view_backward_restatement.py
    and no other: nothing is multiplied by a 1 or added to a 0."""
import torch

import ba2view_backward_restatement as br
import ba2view_loss_restatement as rs
from oracle import kornia_fns as K
from oracle.pytorch3d_fns import se3_exp_map

F64 = torch.float64


# ------------------------------------------------------------------------------------------------ (a) dense loop, autograd through a


def rho_sq_tensor(loss, a, s):
    """``rs.rho_sq`` with ``a`` a 0-dim fp64 tensor that may carry a graph, in the operations that function performs: there ``a`` is a
    Python number, and torch evaluates number / tensor as the reciprocal times the number - so does this, to run its very trajectory."""
    a2 = a * a
    if loss == "huber":
        small = s <= a2
        t = torch.sqrt(torch.where(small, torch.ones_like(s), s))
        return torch.where(small, s, 2.0 * a * t - a2), torch.where(small, torch.ones_like(s), torch.sqrt(t.reciprocal() * a))
    if loss == "cauchy":
        q = s / a2
        return a2 * torch.log1p(q), torch.sqrt(1.0 / (1.0 + q))
    raise ValueError(loss)


def run_autograd(kpts0_norm, kpts1_norm, confidence, init_T021, n_iterations, homogeneous_sign, loss, loss_scale, lm_increase=1.5,
                 lm_decrease=3.5):
    """``rs.run_bundle_adjust_2_view`` with ``a`` a tensor: -> (T of the valid samples, valid_batch, trajectories)."""
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
        cden = 0.5 * (2 * c.sum()).clamp(min=1e-6)
        c = c / cden
        # (tensor over tensor: ONE fp64 division as on the device - a Python number over a tensor is a product with the reciprocal)
        a = torch.tensor(float(loss_scale), dtype=dt) / cden if loss is not None else None
        extr1 = init_T021[b].clone().to(dt)
        P0 = torch.eye(4, dtype=dt)[:3]
        h = K.triangulate_points_homogeneous(P0[None], extr1[None, :3], x0[None], x1[None])[0]
        flip = torch.where(torch.signbit(h[:, 3:]) != (homogeneous_sign < 0), -torch.ones_like(h[:, 3:]), torch.ones_like(h[:, 3:]))
        pts = K.convert_points_from_homogeneous(h * flip)
        M = pts.shape[0]
        lam = 0.1
        best_r, best = None, extr1.clone()
        tr = {"best": [], "cost": [], "accepted": []}
        for it in range(n_iterations + 1):
            J, r, rn, s = rs.corrected_system(extr1, pts, x0, x1, c)
            if loss is not None:
                rho, sq = rho_sq_tensor(loss, a, s)
                rows = sq.repeat_interleave(2)
                J, r, rn = J * rows[:, None], r * rows, rho[:M].sum() + rho[M:].sum()
            A, bvec = J.T @ J, -(J.T @ r)
            tr["cost"].append(rn.detach())
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
        trajectory.append({"best": torch.stack(tr["best"]), "cost": torch.stack(tr["cost"]), "accepted": torch.tensor(tr["accepted"])})
    res = torch.stack(out) if out else torch.zeros(0, 4, 4, dtype=dt)
    return res, valid_batch, trajectory


# ------------------------------------------------------------------------------------------------ (b) the reverse by hand, Schur form


def sq_derivatives(loss, a, s, sq):
    """(dsq/ds, dsq/da) elementwise; Huber's kink s = a^2 takes the first branch, like ``rho_sq``."""
    a = float(a)
    a2 = a * a
    if loss == "huber":
        small = s <= a2
        safe = torch.where(small, torch.ones_like(s), s)
        zero = torch.zeros_like(s)
        return torch.where(small, zero, -sq / (4.0 * safe)), torch.where(small, zero, sq / (2.0 * a))
    if loss == "cauchy":
        sq3 = sq * sq * sq
        return -sq3 / (2.0 * a2), sq3 * s / (a2 * a)
    raise ValueError(loss)


def evaluate(Rt, X, x0, x1, c, loss=None, a=0.0):
    """The terms of one evaluation as the step uses them (corrected under a loss), the cost that the bookkeeping compares, and under a
    loss the uncorrected terms, the squared block norms and sqrt(rho')."""
    r0, r1, Jp0, Jp1, Jc = br.point_terms(Rt, X, x0, x1, c)
    if loss is None:
        return dict(r0=r0, r1=r1, Jp0=Jp0, Jp1=Jp1, Jc=Jc, cost=(r0 ** 2).sum() + (r1 ** 2).sum())
    s0 = r0[:, 0] * r0[:, 0] + r0[:, 1] * r0[:, 1]
    s1 = r1[:, 0] * r1[:, 0] + r1[:, 1] * r1[:, 1]
    rho0, sq0 = rs.rho_sq(loss, a, s0)
    rho1, sq1 = rs.rho_sq(loss, a, s1)
    return dict(r0=r0 * sq0[:, None], r1=r1 * sq1[:, None], Jp0=Jp0 * sq0[:, None, None], Jp1=Jp1 * sq1[:, None, None], Jc=Jc * sq1[:, None, None],
                cost=rho0.sum() + rho1.sum(), raw=(r0, r1, Jp0, Jp1, Jc), s0=s0, s1=s1, sq0=sq0, sq1=sq1)


def lm_step(Rt, X, x0, x1, c, lam, loss=None, a=0.0):
    """``br.lm_step`` on the terms of ``evaluate``."""
    st = evaluate(Rt, X, x0, x1, c, loss, a)
    r0, r1, Jp0, Jp1, Jc = st["r0"], st["r1"], st["Jp0"], st["Jp1"], st["Jc"]
    Hcc = (Jc.transpose(1, 2) @ Jc).sum(0)
    gc = -(Jc.transpose(1, 2) @ r1[:, :, None]).sum(0)[:, 0]
    Hpp = Jp0.transpose(1, 2) @ Jp0 + Jp1.transpose(1, 2) @ Jp1
    gp = -((Jp0.transpose(1, 2) @ r0[:, :, None]) + (Jp1.transpose(1, 2) @ r1[:, :, None]))[:, :, 0]
    Hcp = Jc.transpose(1, 2) @ Jp1
    dpp, dcc = torch.diagonal(Hpp, dim1=1, dim2=2), torch.diagonal(Hcc)
    precond = bool((dpp > 0).all()) and bool((dcc > 0).all())
    Dp = dpp.clamp(min=1e-12) if precond else torch.ones_like(dpp)
    Dc = dcc.clamp(min=1e-12) if precond else torch.ones_like(dcc)
    Hppd = Hpp + lam * torch.diag_embed(Dp)
    inv = torch.linalg.inv(Hppd)
    W = Hcp @ inv
    S = Hcc + lam * torch.diag(Dc) - (W @ Hcp.transpose(1, 2)).sum(0)
    rhs = gc - (W @ gp[:, :, None]).sum(0)[:, 0]
    LU, piv, info = torch.linalg.lu_factor_ex(S)
    st.update(Hcp=Hcp, inv=inv, LU=LU, piv=piv, precond=precond, lam=lam, dpp=dpp, dcc=dcc, ok=int(info) == 0, loss=loss, a=a)
    if not st["ok"]:
        return st
    dc = torch.linalg.lu_solve(LU, piv, rhs[:, None])[:, 0]
    dp = (inv @ (gp - (Hcp.transpose(1, 2) @ dc))[:, :, None])[:, :, 0]
    st.update(dc=dc, dp=dp)
    return st


def lm_step_reverse(st, Rt, X, x0, x1, c, dcb, dpb):
    """Adjoint of ``lm_step`` for (dc_bar [6], dp_bar [M,3]) -> (X_bar [M,3], Rt_bar [3,4], c_bar [M], a_bar) THROUGH the step only."""
    Jp0, Jp1, Jc, r0, r1, Hcp, inv, lam = st["Jp0"], st["Jp1"], st["Jc"], st["r0"], st["r1"], st["Hcp"], st["inv"], st["lam"]
    dc, dp = st["dc"], st["dp"]
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
    r0b, r1b = -jw0, -jw1
    Jp0b = -jw0[:, :, None] * dp[:, None, :] - (jd0 + r0)[:, :, None] * wp[:, None, :] - Jp0 * wdp[:, None, :]
    Jp1b = -jw1[:, :, None] * dp[:, None, :] - (jd1 + r1)[:, :, None] * wp[:, None, :] - Jp1 * wdp[:, None, :]
    Jcb = -jw1[:, :, None] * dc[None, None, :] - (jd1 + r1)[:, :, None] * wc[None, None, :] - Jc * wdc[None, None, :]
    ab = torch.zeros((), dtype=F64)
    if st["loss"] is not None:  # (r0b ... Jcb) are the adjoints of the corrected blocks: back through the corrector, per block
        q0, q1, P0, P1, C1 = st["raw"]
        sq0, sq1 = st["sq0"], st["sq1"]
        sb0 = (r0b * q0).sum(1) + (Jp0b * P0).sum((1, 2))
        sb1 = (r1b * q1).sum(1) + (Jp1b * P1).sum((1, 2)) + (Jcb * C1).sum((1, 2))
        ds0, da0 = sq_derivatives(st["loss"], st["a"], st["s0"], sq0)
        ds1, da1 = sq_derivatives(st["loss"], st["a"], st["s1"], sq1)
        ab = (da0 * sb0).sum() + (da1 * sb1).sum()
        r0b = sq0[:, None] * r0b + (2.0 * ds0 * sb0)[:, None] * q0
        r1b = sq1[:, None] * r1b + (2.0 * ds1 * sb1)[:, None] * q1
        Jp0b, Jp1b, Jcb = sq0[:, None, None] * Jp0b, sq1[:, None, None] * Jp1b, sq1[:, None, None] * Jcb
    Xb, Rtb, cb = br.point_terms_reverse(Rt, X, x0, x1, c, r0b, r1b, Jp0b, Jp1b, Jcb)
    return Xb, Rtb, cb, ab


def forward_tape(k0, k1, conf, T_init, n_iterations, sign, loss=None, loss_scale=None, lm_increase=1.5, lm_decrease=3.5):
    """``br.forward_tape`` with a loss at the RELATIVE scale ``loss_scale``: -> None for an invalid sample, else the tape."""
    m = conf > 0.0
    if int(m.sum()) <= 6:
        return None
    x0, x1, cf = k0[m], k1[m], conf[m]
    csum = 2 * cf.sum()
    cden = 0.5 * csum.clamp(min=1e-6)
    c = cf / cden
    a = float(loss_scale) / float(cden) if loss is not None else 0.0
    Rt = T_init[:3].clone()
    X = br.triangulate(Rt, x0, x1, sign)
    lam, best_r, kstar = 0.1, None, 0
    tape = dict(mask=m, x0=x0, x1=x1, cf=cf, c=c, cden=cden, csum=csum, sign=sign, loss=loss, a=a, steps=[], cost=[], accepted=[],
                best_before=[], poses=[])
    for it in range(n_iterations + 1):
        rn = evaluate(Rt, X, x0, x1, c, loss, a)["cost"]
        tape["cost"].append(float(rn))
        tape["best_before"].append(float("nan") if it == 0 else float(best_r))
        tape["poses"].append(Rt)
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
        st = lm_step(Rt, X, x0, x1, c, lam, loss, a)
        st.update(Rt=Rt, X=X)
        tape["steps"].append(st)
        if not st["ok"]:
            continue
        Rt = br.exp_step(st["dc"], Rt)
        X = X + st["dp"]
    tape["kstar"] = kstar
    tape["best"] = tape["steps"][kstar]["Rt"] if kstar < len(tape["steps"]) else Rt
    return tape


def backward(tape, gT, N, scale_gradient=True):
    """gT [4,4] (rows 0-2 used) -> (gconf [N], gTinit [4,4]) of one valid sample; ``scale_gradient=False``: ``a`` detached."""
    x0, x1, c = tape["x0"], tape["x1"], tape["c"]
    Rtb = gT[:3].clone().to(F64)
    row3 = torch.zeros(4, dtype=F64)
    Xb = torch.zeros(x0.shape[0], 3, dtype=F64)
    cb = torch.zeros(x0.shape[0], dtype=F64)
    ab = torch.zeros((), dtype=F64)
    gconf = torch.zeros(N, dtype=F64)
    gTinit = torch.zeros(4, 4, dtype=F64)
    if tape["kstar"] > 0:
        for k in range(tape["kstar"] - 1, -1, -1):
            st = tape["steps"][k]
            if not st["ok"]:
                continue
            dcb, Rtb_through, r3 = br.exp_step_reverse(st["dc"], st["Rt"], Rtb)
            dX, dRt, dcw, da = lm_step_reverse(st, st["Rt"], st["X"], x0, x1, c, dcb, Xb)
            Xb, Rtb, cb, row3 = Xb + dX, Rtb_through + dRt, cb + dcw, row3 + r3
            if tape["loss"] is not None:
                ab = ab + da
        Rtb = Rtb + br.triangulate_reverse(tape["steps"][0]["Rt"], x0, x1, tape["sign"], Xb)
        g = cb / tape["cden"]
        if float(tape["csum"]) >= 1e-6:
            g = g - (cb * c).sum() / tape["cden"]
            if tape["loss"] is not None and scale_gradient:
                g = g - ab * tape["a"] / tape["cden"]
        gconf[tape["mask"]] = g
    gTinit[:3], gTinit[3] = Rtb, row3
    return gconf, gTinit


def run(k0, k1, conf, T_init, n_iterations, gT, sign, loss=None, loss_scale=None, scale_gradient=True):
    """``br.run`` with a loss: -> (T [B,4,4], valid [B], gconf [B,N], gTinit [B,4,4], tapes)."""
    k0, k1, conf, T_init, gT = (t.to(F64) for t in (k0, k1, conf, T_init, gT))
    B, N = conf.shape
    T, gconf, gTi, tapes = T_init.clone(), torch.zeros(B, N, dtype=F64), torch.zeros(B, 4, 4, dtype=F64), []
    valid = torch.zeros(B, dtype=torch.bool)
    for b in range(B):
        tape = forward_tape(k0[b], k1[b], conf[b], T_init[b], n_iterations, sign, loss, loss_scale)
        tapes.append(tape)
        if tape is None:
            gTi[b, :3] = gT[b, :3]
            continue
        valid[b] = True
        T[b, :3] = tape["best"]
        gconf[b], gTi[b] = backward(tape, gT[b], N, scale_gradient)
    return T, valid, gconf, gTi, tapes
