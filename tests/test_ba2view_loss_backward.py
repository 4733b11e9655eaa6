"""The backward pass of the two-view bundle adjustment through the Huber and Cauchy losses, as far as it can be checked without a GPU.

tests/ba2view_loss_backward_restatement.py holds (a) the dense robust LM loop of tests/ba2view_loss_restatement.py with the pair's scale
``a = loss_scale / cden`` kept as a tensor, and (b) the reverse written out by hand in the Schur form of the kernel; (b) is what the
device tests of tests/test_gpu_ba2view_loss_backward.py compare ``e2emv_ba_2view_loss_backward`` with.  Here: (a) runs the trajectory of
the pinned restatement; (b) IS ``torch.autograd`` through (a); without a loss (b) is tests/ba2view_backward_restatement.py exactly, and
with Huber at a scale no block reaches to rounding; the gradient through the scale is really there; one robust step's adjoint - the scale
among the variables - is the central difference of that step; the premises the comparisons rest on hold on every case used here or on the
device; the C entry is declared, bound, exported and refuses a NULL context; and the Python fronts make the calls they should and raise
what they should before any device call.

Cases and scales are those of tests/test_ba2view_loss.py: one pixel at f = 600, the clamp case at 3e-11."""
import ctypes
import functools
import os
import re

import pytest
import torch

import ba2view_backward_restatement as br
import ba2view_loss_backward_restatement as lb
import test_ba2view_backward as TB
import test_ba2view_loss as L
import test_pose_loss_tuple as PT
from test_ba2view_backward import cotangent, pattern
from test_gpu_ba_steps import N_ITERS, N_MAX, TIE_GAP, make_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64
LOSSES = L.LOSSES
CASES = ["a_n7", "b_n8_hole0", "c_n65", "f_n257_garbage", "k_n65_clamp"]
DEVICE_CASES = CASES + ["j_n257_outliers"]  # what tests/test_gpu_ba2view_loss_backward.py adds: its premises are asserted here too
HUBER_KINK_GAP = 1e-6  # the sign freedom moves s by about 1e-8 relative: both sign runs and the device stay on one branch


scene, scale_of = L.scene, L.scale_of


@functools.lru_cache(maxsize=None)
def restated(name, loss, sign, n, scale_gradient=True):
    """(T, gconf, gTinit, tape) of restatement (b): shared, never modified."""
    s = scene(name)
    T, valid, gconf, gTi, tapes = lb.run(s["k0"], s["k1"], s["conf"], s["T_init"], n, cotangent(), sign, loss, scale_of(name) if loss else None,
                                         scale_gradient)
    assert bool(valid.all())
    return T[0], gconf[0], gTi[0], tapes[0]


@functools.lru_cache(maxsize=None)
def autograd_gradients(name, loss, sign):
    """{n: (gconf [N], gTinit [4,4])} for every n of N_ITERS from ONE 10-iteration run of helper (a): the trajectory's best[n] is the result
    of n_iterations = n and carries the graph - through the scale too.  Also the trajectory (detached)."""
    s = scene(name)
    conf = s["conf"].double().clone().requires_grad_(True)
    Ti = s["T_init"].double().clone().requires_grad_(True)
    _, valid, traj = lb.run_autograd(s["k0"].double(), s["k1"].double(), conf, Ti, N_MAX, sign, loss, scale_of(name))
    assert bool(valid.all())
    gT = cotangent()[0].double()
    out = {}
    for n in N_ITERS:
        gc, gt = torch.autograd.grad((traj[0]["best"][n] * gT).sum(), [conf, Ti], retain_graph=True, allow_unused=True)
        out[n] = (torch.zeros_like(conf[0]) if gc is None else gc[0], gt[0])
    return out, {k: v.detach() for k, v in traj[0].items()}


# ------------------------------------------------------------------------------------------------ helper (a) and helper (b)


@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("name", CASES)
def test_helper_a_runs_the_trajectory_of_the_pinned_restatement(name, loss):
    """The scale as a tensor changes nothing in the forward: best, cost and accepted of tests/ba2view_loss_restatement.py within 1e-12."""
    for sign, want in zip((+1, -1), L.trajectories(name, loss)):
        _, got = autograd_gradients(name, loss, sign)
        assert torch.equal(got["accepted"], want["accepted"]), (name, loss, sign)
        for key in ("best", "cost"):
            err = float(((got[key] - want[key]).abs() / want[key].abs().clamp(min=1e-300)).max()) if key == "cost" else \
                float((got[key] - want[key]).abs().max() / want[key].abs().max())
            print(f"{name} {loss} sign={sign:+d} {key}: relative distance {err:.2e}")
            assert err <= 1e-12, (name, loss, sign, key, err)


@pytest.mark.parametrize("sign", [+1, -1])
@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("name", CASES)
def test_restatement_is_autograd_through_the_robust_loop(name, loss, sign):
    """gconf and gTinit of (b) against autograd through (a), every n of N_ITERS, both signs of the null vector.  Both sides are fp64
    evaluations of one function: the bar is 1e-9 max|g|, that of tests/test_ba2view_backward.py.  Measured (largest over the cases, n and
    sign, relative to max|g|): huber gconf 6.7e-11, gTinit 3.6e-12; cauchy gconf 1.1e-10, gTinit 4.0e-12, all at n = 10.  (On
    j_n257_outliers, which only the device tests use - 777 dense unknowns, wrong matches under the preconditioner's floor - the same
    comparison gives 1.3e-13 / 5.8e-13 at n = 3 and 5.4e-9 / 1.1e-9 at n = 10, huber / cauchy; it is not asserted.)"""
    want, traj = autograd_gradients(name, loss, sign)
    for n in N_ITERS:
        T, gconf, gTi, tape = restated(name, loss, sign, n)
        assert pattern(tape["accepted"]) == pattern(traj["accepted"].tolist())[:n], (name, n)
        assert float((T - traj["best"][n]).abs().max()) <= 1e-9, (name, n)
        gc, gt = want[n]
        for what, a, b in (("gconf", gconf, gc), ("gTinit", gTi, gt)):
            scale = float(b.abs().max())
            err = float((a - b).abs().max())
            print(f"{name} {loss} sign={sign:+d} n={n} {what}: |restated - autograd| = {err:.2e}, max|g| = {scale:.2e}, k* = {tape['kstar']}")
            assert bool(a.isfinite().all()) and err <= 1e-9 * scale, (name, loss, sign, n, what, err, scale)
        if n == 0:
            assert float(gconf.abs().max()) == 0.0 and torch.equal(gTi[:3], cotangent()[0, :3].double()) and float(gTi[3].abs().max()) == 0.0
        else:
            assert tape["kstar"] > 0 and float(gconf.abs().max()) > 0.0


@pytest.mark.parametrize("name", CASES)
def test_without_a_loss_the_helper_is_the_squared_loss_restatement_exactly(name):
    """loss=None: the bits of tests/ba2view_backward_restatement.py.  Huber at loss_scale = 1e6 puts every block on the first branch:
    only multiplications by 1 and additions of 0 differ, and the bar is 1e-12 max|g|."""
    s = scene(name)
    for sign in (+1, -1):
        for n in (1, 3, N_MAX):
            T0, _, gc0, gt0, tapes0 = br.run(s["k0"], s["k1"], s["conf"], s["T_init"], n, cotangent(), sign)
            T1, _, gc1, gt1, tapes1 = lb.run(s["k0"], s["k1"], s["conf"], s["T_init"], n, cotangent(), sign)
            assert torch.equal(T0, T1) and torch.equal(gc0, gc1) and torch.equal(gt0, gt1) and tapes0[0]["kstar"] == tapes1[0]["kstar"], (name, sign, n)
            assert tapes0[0]["cost"] == tapes1[0]["cost"]
            T2, _, gc2, gt2, tapes2 = lb.run(s["k0"], s["k1"], s["conf"], s["T_init"], n, cotangent(), sign, "huber", 1e6)
            assert all(bool((st["sq0"] == 1).all()) and bool((st["sq1"] == 1).all()) for st in tapes2[0]["steps"])
            for what, a, b in (("gconf", gc2, gc0), ("gTinit", gt2, gt0)):
                err, scale = float((a - b).abs().max()), float(b.abs().max())
                assert err <= 1e-12 * scale, (name, sign, n, what, err, scale)


def test_the_gradient_through_the_scale_is_really_there():
    """The same reverse with ``a`` detached: on at least one case gconf differs from the full one by more than 100 x 1e-3 max|g|; where the
    weights' denominator is the clamp constant the scale carries nothing and the two agree exactly.  gTinit never sees the term.
    Looked at for every n > 0 of N_ITERS: the term is largest in the first steps, where the residuals straddle the scale, and fades as the
    noise-free scenes converge below it.  Measured (largest over n, in max|g|): a_n7 0.039 / 0.055 (huber / cauchy), b_n8_hole0 0.084 /
    0.20, c_n65 0.007 / 0.021, f_n257_garbage 0.012 / 0.017; at n = 10 alone the largest is 0.0085."""
    apart = {}
    for name in CASES:
        for loss in LOSSES:
            for n in N_ITERS[1:]:
                _, gc, gt, _ = restated(name, loss, +1, n)
                _, gc_d, gt_d, _ = restated(name, loss, +1, n, False)
                assert torch.equal(gt, gt_d), (name, loss, n)
                apart[name, loss, n] = float((gc - gc_d).abs().max()) / float(gc.abs().max())
                if name == "k_n65_clamp":
                    assert torch.equal(gc, gc_d), (loss, n)
            print(f"{name} {loss}: |gconf - gconf(a detached)| / max|g| at n = {N_ITERS[1:]}: " + " ".join(f"{apart[name, loss, n]:.2e}" for n in N_ITERS[1:]))
    assert max(apart.values()) > 100.0 * 1e-3, apart


# ------------------------------------------------------------------------------------------------ one step against differences


@pytest.mark.parametrize("loss", LOSSES)
def test_robust_step_adjoint_is_the_central_difference_of_one_restated_step(loss):
    """One robust LM step of the 7-match scene at its start, lambda = 0.1: F = <G, Rt'> + <H, X'> for fixed random G, H as a function of
    the pose (12), the points (21), the weights (7) AND the absolute scale a (1), one coordinate at a time.  a lies midway between the two
    middle block norms (seven blocks on each Huber branch, none at the kink, as in tests/test_ba2view_loss.py).  h = 1e-5 for the first 40
    coordinates and 1e-5 a for a itself, whose size is 1e-3.  The bar is that of
    tests/test_ba2view_backward.py::test_step_adjoint_is_the_central_difference_of_one_restated_step, derived the same way:
    * truncation: (D(2h) - D(h)) / 3 estimates it; allowed is 3 x that (a block within h of Huber's kink adds O(h) x its share, which the
      same estimate sees);
    * rounding: the corrector scales rows by sqrt(rho') <= 1 before the Jacobi scaling, so the scaled matrix C + lambda I still has a
      unit-diagonal positive semi-definite C and a condition of at most kappa = (6 + 3 M + lambda) / lambda; an entry now goes through 8
      more roundings (s: 3, two square roots, two divisions, the product), 24 in all: F is off by at most 24 eps kappa S with S = sum |G o
      Rt'| + sum |H o X'|, and D(h) by 24 eps kappa S / h."""
    s = scene("a_n7")
    x0, x1, conf = s["k0"][0].double(), s["k1"][0].double(), s["conf"][0].double()
    c = conf / conf.sum()
    Rt = s["T_init"][0, :3].double()
    X = br.triangulate(Rt, x0, x1, +1)
    M, lam = 7, 0.1
    plain = lb.evaluate(Rt, X, x0, x1, c, "huber", 1.0)
    norms = torch.cat([plain["s0"], plain["s1"]]).sqrt().sort().values
    a = 0.5 * float(norms[M - 1] + norms[M])
    assert float(norms[M] / norms[M - 1]) > 1.01 and int((torch.cat([plain["s0"], plain["s1"]]) <= a * a).sum()) == M
    gen = torch.Generator().manual_seed(9)
    G, H = torch.randn(3, 4, generator=gen, dtype=F64), torch.randn(M, 3, generator=gen, dtype=F64)

    def step(Rt, X, c, a):
        st = lb.lm_step(Rt, X, x0, x1, c, lam, loss, a)
        assert st["ok"] and st["precond"]
        return br.exp_step(st["dc"], Rt), X + st["dp"], st

    Rn, Xn, st = step(Rt, X, c, a)
    dcb, through, _ = br.exp_step_reverse(st["dc"], Rt, G)
    dX, dRt, dcw, da = lb.lm_step_reverse(st, Rt, X, x0, x1, c, dcb, H)
    adj = torch.cat([(through + dRt).reshape(-1), (H + dX).reshape(-1), dcw, da.reshape(1)])

    def F(v):
        Rn, Xn, _ = step(v[:12].view(3, 4), v[12:12 + 3 * M].view(M, 3), v[12 + 3 * M:12 + 4 * M], float(v[-1]))
        return float((G * Rn).sum() + (H * Xn).sum())

    v0 = torch.cat([Rt.reshape(-1), X.reshape(-1), c, torch.tensor([a], dtype=F64)])
    S_abs = float((G * Rn).abs().sum() + (H * Xn).abs().sum())
    eps = 2.0 ** -52

    def D(k, h):
        e = torch.zeros_like(v0)
        e[k] = h
        return (F(v0 + e) - F(v0 - e)) / (2.0 * h)

    worst = 0.0
    for k in range(len(v0)):
        h = 1e-5 * (a if k == len(v0) - 1 else 1.0)
        rounding = 24.0 * eps * (6 + 3 * M + lam) / lam * S_abs / h
        d1, d2 = D(k, h), D(k, 2.0 * h)
        tol = abs(d2 - d1) + rounding
        worst = max(worst, abs(float(adj[k]) - d1) / tol)
        assert abs(float(adj[k]) - d1) <= tol, (loss, k, float(adj[k]), d1, tol)
    assert abs(float(adj[-1])) > 0.0  # the scale's adjoint is not a zero that a zero difference confirms
    print(loss, "largest |adjoint - D(h)| / bar", worst, "largest adjoint entry", float(adj.abs().max()), "a_bar", float(adj[-1]))


# ------------------------------------------------------------------------------------------------ premises


@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("name", DEVICE_CASES)
def test_premises_of_the_comparison_hold(name, loss):
    """Both signs decide alike and no comparison is closer than TIE_GAP; precond holds everywhere, no diagonal at the floor, no step at
    the boundary of the exponential's clamp; for Huber no observation of a taped evaluation before k* lies within 1e-6 (relative) of the
    kink, and both branches are populated at some evaluation before k*.

    The floor on j_n257_outliers: with 257 matches a weight is about 1/130, and the corrector scales the point block of a wrong match by
    rho' ~ (a / |r|)^(1 or 2), so the CORRECTED diagonal of such a point is 1e-13 .. 1e-17 - under the preconditioner's 1e-12 floor at
    every seed (118 .. 131) and start (0.03 / 0.05, 0.2 / 0.2, 0.45 / 0.3) tried, in the first evaluation at most of them.  That is what
    the loss does to a wrong match, not a property of a seed.  Below the floor D_jj is the constant 1e-12 and the reverse is as well
    defined as above it; what a comparison cannot stand is an entry AT the floor, which rounding could put on either side.  So there
    the premise is: no entry within 1e-6 (relative) of 1e-12, and both sign runs floor the same entries.  Every other case stays
    strictly above the floor, as in tests/test_ba2view_backward.py."""
    tp, tm = restated(name, loss, +1, N_MAX)[3], restated(name, loss, -1, N_MAX)[3]
    assert pattern(tp["accepted"]) == pattern(tm["accepted"]) and tp["kstar"] == tm["kstar"] > 0, name
    a2 = tp["a"] * tp["a"]
    assert tp["a"] == tm["a"] and tp["a"] > 0
    both = False
    for tr in (tp, tm):
        cost, before = torch.tensor(tr["cost"][1:], dtype=F64), torch.tensor(tr["best_before"][1:], dtype=F64)
        assert bool(cost.isfinite().all()) and float(((cost - before).abs() / before.abs()).min()) >= TIE_GAP, name
        for k, st in enumerate(tr["steps"]):
            assert st["ok"] and st["precond"], name
            if name == "j_n257_outliers":
                assert float((st["dpp"] - 1e-12).abs().min()) >= 1e-6 * 1e-12 and float(st["dcc"].min()) > 1e-12, name
                assert torch.equal(st["dpp"] < 1e-12, tm["steps"][k]["dpp"] < 1e-12), (name, k)
            else:
                assert float(st["dpp"].min()) > 1e-12 and float(st["dcc"].min()) > 1e-12, name
            n2 = float((st["dc"][3:] ** 2).sum())
            assert abs(n2 - 1e-4) > 1e-6 * 1e-4, (name, n2)
            if loss == "huber" and k < tr["kstar"]:
                sblocks = torch.cat([st["s0"], st["s1"]])
                assert float(((sblocks - a2).abs() / a2).min()) >= HUBER_KINK_GAP, (name, k)
                both = both or (bool((sblocks <= a2).any()) and bool((sblocks > a2).any()))
    assert both or loss != "huber", name
    print(f"{name} {loss}: pattern {pattern(tp['accepted'])}, k* = {tp['kstar']}, a = {tp['a']:.3e}")
    if name == "j_n257_outliers":  # a rejected step before k*, and both Huber branches live to the end
        assert "r" in pattern(tp["accepted"])[:tp["kstar"]], pattern(tp["accepted"])
        if loss == "huber":
            last = tp["steps"][tp["kstar"] - 1]
            sblocks = torch.cat([last["s0"], last["s1"]])
            assert bool((sblocks <= a2).any()) and bool((sblocks > a2).any())
    if name == "k_n65_clamp":
        assert float(tp["csum"]) < 1e-6 and float(tp["cden"]) == 5e-7
    else:
        assert float(tp["csum"]) >= 1e-6


def test_premise_an_early_kstar_with_rejected_steps_occurs():
    tape = restated("a_n7", "huber", +1, N_MAX)[3]
    assert 0 < tape["kstar"] < N_MAX and "r" in pattern(tape["accepted"]), (tape["kstar"], pattern(tape["accepted"]))


def test_restatement_of_an_invalid_sample():
    s = make_scene(8, 301)
    s["conf"][0, 6:] = 0.0
    T, valid, gconf, gTi, tapes = lb.run(s["k0"], s["k1"], s["conf"], s["T_init"], 3, cotangent(), +1, "cauchy", L.PIXEL)
    assert valid.tolist() == [False] and tapes == [None] and torch.equal(T, s["T_init"].double())
    assert float(gconf.abs().max()) == 0.0 and torch.equal(gTi[0, :3], cotangent()[0, :3].double()) and float(gTi[0, 3].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ C ABI and Python fronts

NAME, BASE = "e2emv_ba_2view_loss_backward", "e2emv_ba_2view_backward"


def test_header_declares_and_library_exports_the_entry(lib_built):
    from e2e_multi_view_matching_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "e2emv.h")).read()
    assert NAME in set(re.findall(r"\b(e2emv_[a-z0-9_]+)\s*\(", hdr))
    assert NAME in _lib.SIGNATURES and hasattr(ctypes.CDLL(lib_built), NAME) and hasattr(ctypes.CDLL(lib_built), BASE)
    norm = lambda t: [" ".join(x.split()) for x in t.split(",")]  # noqa: E731
    decl = norm(re.search(r"int %s\((.*?)\);" % NAME, hdr, re.S).group(1))
    old = norm(re.search(r"int %s\((.*?)\);" % BASE, hdr, re.S).group(1))
    # the squared-loss entry's arguments with the loss and its scale in front of the incoming gradient
    assert decl == old[:-4] + ["int loss", "double loss_scale"] + old[-4:]
    sig, sig_old = _lib.SIGNATURES[NAME], _lib.SIGNATURES[BASE]
    assert sig[0] is ctypes.c_int and len(sig[1]) == len(decl) == 14
    assert sig[1] == sig_old[1][:-4] + [ctypes.c_int, ctypes.c_double] + sig_old[1][-4:]
    assert open(os.path.join(ROOT, "INTEGRATION.md")).read().count("`%s`" % NAME) >= 1


def test_null_context_is_rejected(lib_built):
    from e2e_multi_view_matching_amd import _lib
    lib = _lib.load_library()
    assert lib.e2emv_ba_2view_loss_backward(None, 1, 8, None, None, None, None, 1, 2, 1.0, None, None, None, None) == _lib.EINVAL


def _pair(B=2, N=8):
    return torch.zeros(B, N, 2), torch.eye(4)[None].repeat(B, 1, 1)


@pytest.mark.parametrize("loss", LOSSES)
def test_run_bundle_adjust_2_view_call_sequences_with_a_loss(loss, monkeypatch):
    from e2e_multi_view_matching_amd import pose
    rec = TB._stub_device(monkeypatch)
    z, Ti = _pair()
    conf = torch.ones(2, 8, 1, requires_grad=True)
    T, vb = pose.run_bundle_adjust_2_view(z, z, conf, Ti, 3, loss=loss, loss_scale=1.0, loss_backward=True)
    assert rec.calls == ["e2emv_ba_2view_loss"] and T.grad_fn is not None
    T.sum().backward()
    assert rec.calls == ["e2emv_ba_2view_loss", "e2emv_ba_2view_loss_backward"] and conf.grad is not None and conf.grad.shape == conf.shape
    rec.calls.clear()
    Tg = Ti.clone().requires_grad_(True)  # the graph on the start pose alone, and the summary with it
    T, vb, summary = pose.run_bundle_adjust_2_view(z, z, torch.ones(2, 8), Tg, 3, loss=loss, loss_scale=1.0, loss_backward=True, return_summary=True)
    assert rec.calls == ["e2emv_ba_2view_loss"] and T.grad_fn is not None and summary.shape == (2, 4) and summary.dtype == torch.float64
    T.sum().backward()
    assert rec.calls == ["e2emv_ba_2view_loss", "e2emv_ba_2view_loss_backward"] and Tg.grad is not None and Tg.grad.shape == Tg.shape
    rec.calls.clear()
    with torch.no_grad():  # no graph asked for: the forward alone, whatever the keyword says
        T, vb = pose.run_bundle_adjust_2_view(z, z, conf, Ti, 3, loss=loss, loss_scale=1.0, loss_backward=True)
    assert rec.calls == ["e2emv_ba_2view_loss"] and T.grad_fn is None
    rec.calls.clear()
    conf.grad = None  # without a loss: exactly the calls of before
    T, vb = pose.run_bundle_adjust_2_view(z, z, conf, Ti, 3)
    T.sum().backward()
    assert rec.calls == ["e2emv_ba_2view", "e2emv_ba_2view_backward"]


def test_loss_backward_rules_hold_before_any_device_call(monkeypatch):
    from e2e_multi_view_matching_amd import pose
    L._no_device(monkeypatch)
    z, Ti = _pair(1)
    conf = torch.ones(1, 8, requires_grad=True)
    for c in (conf, conf.detach()):
        with pytest.raises(ValueError, match="loss_backward=True needs a loss"):
            pose.run_bundle_adjust_2_view(z, z, c, Ti, 3, loss_backward=True)
        for bad in (1, 0, None, "yes"):
            with pytest.raises(ValueError, match="loss_backward must be"):
                pose.run_bundle_adjust_2_view(z, z, c, Ti, 3, loss="cauchy", loss_scale=1.0, loss_backward=bad)
    with pytest.raises(NotImplementedError, match="squared.*loss_backward=True"):  # the default stays, and names the keyword
        pose.run_bundle_adjust_2_view(z, z, conf, Ti, 3, loss="huber", loss_scale=1.0)
    with pytest.raises(NotImplementedError, match="squared"):
        pose.run_bundle_adjust_2_view(z, z, conf, Ti, 3, loss="huber", loss_scale=1.0, loss_backward=False)
    with pytest.raises(AssertionError, match="a device call was made"):  # a good call passes the host checks and reaches for the device
        pose.run_bundle_adjust_2_view(z, z, conf, Ti, 3, loss="huber", loss_scale=1.0, loss_backward=True)


def _loss_sequences(P):
    fwd = ["e2emv_relative_pose"] * P + ["e2emv_gather_matched"] * P + ["e2emv_w8pt_tuple", "e2emv_apply_mask", "e2emv_ba_2view_loss",
                                                                        "e2emv_pose_loss_tuple"]
    bwd = ["e2emv_pose_loss_tuple_backward", "e2emv_ba_2view_loss_backward", "e2emv_apply_mask", "e2emv_w8pt_tuple_backward"]
    return fwd, bwd


@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("T,B", [(3, 1), (3, 5)])
def test_pose_loss_tuple_call_sequences_with_a_loss(monkeypatch, loss, T, B):
    from e2e_multi_view_matching_amd import pose
    rec = TB._stub_device(monkeypatch)
    data, result, pairs = PT._tuple(T, B, 9)
    fwd, bwd = _loss_sequences(len(pairs))
    out = pose.pose_loss_tuple(data, result, ba_iterations=3, ba_loss=loss, ba_loss_scale=L.PIXEL)
    assert rec.calls == fwd and out["rot_loss"].requires_grad
    (out["rot_loss"] + out["transl_loss"]).backward()
    assert rec.calls == fwd + bwd
    for i, j in pairs:
        g = result["conf_scores_%d_%d" % (i, j)].grad
        assert g is not None and g.shape == (B, 9, 1)
    rec.calls.clear()
    with torch.no_grad():
        out = pose.pose_loss_tuple(data, result, ba_iterations=3, ba_loss=loss, ba_loss_scale=L.PIXEL)
    assert rec.calls == fwd and not out["rot_loss"].requires_grad
    rec.calls.clear()  # the defaults: the squared-loss calls of tests/test_pose_loss_tuple.py
    out = pose.pose_loss_tuple(data, result, ba_iterations=3)
    (out["rot_loss"] + out["transl_loss"]).backward()
    assert rec.calls == sum(PT._sequences(len(pairs), 3), [])


def test_pose_loss_tuple_loss_rules_hold_before_any_call(monkeypatch):
    from e2e_multi_view_matching_amd import pose
    rec = TB._stub_device(monkeypatch)
    data, result, _ = PT._tuple(3, 2, 9)
    for loss, scale, match in L.BAD:
        with pytest.raises(ValueError, match=match):
            pose.pose_loss_tuple(data, result, ba_iterations=3, ba_loss=loss, ba_loss_scale=scale)
    for loss in LOSSES:
        with pytest.raises(ValueError, match="needs ba_iterations > 0"):
            pose.pose_loss_tuple(data, result, ba_loss=loss, ba_loss_scale=L.PIXEL)
        with pytest.raises(ValueError, match="needs ba_iterations > 0"):
            pose.pose_loss_tuple(data, result, ba_iterations=0, ba_loss=loss, ba_loss_scale=L.PIXEL)
    assert rec.calls == []
