"""The backward pass of the two-view bundle adjustment, as far as it can be checked without a GPU.

tests/ba2view_backward_restatement.py states the reverse of the LM loop by hand (fp64, Schur form, no autograd); it is what the device
tests of tests/test_gpu_ba2view_backward.py compare ``e2emv_ba_2view_backward`` with.  Here: it IS ``torch.autograd`` through the
pinned oracle (oracle/ba2view.py, dense normal equations, library LU and SVD); one step's adjoint is the central difference of that step;
the premises the comparison rests on hold on the chosen cases; the C entry is declared, bound, exported and refuses a NULL context; and
the Python front raises for a robust loss with a graph and leaves the call without a graph as it was.

Cases: the scenes of tests/test_gpu_ba_steps.py and tests/test_ba2view_loss.py up to 65 matches, and the 257-row scene with 157 masked
rows of garbage.  The clamp scenes are left out: their 2 sum(conf) lies below 1e-6, where the weights' denominator is a constant."""
import ctypes
import functools
import os
import re

import pytest
import torch

import ba2view_backward_restatement as br
import test_ba2view_loss as L
import test_gpu_ba_steps as S
from test_gpu_ba_steps import N_ITERS, N_MAX, TIE_GAP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64

CASES = {
    "a_n7": S.CASES["a_n7"],
    "b_n8_hole0": S.CASES["b_n8_hole0"],
    "c_n65": S.CASES["c_n65"],
    "f_n257_garbage": L.CASES["f_n257_garbage"][0],
}


@functools.lru_cache(maxsize=None)
def scene(name):
    return CASES[name]()


def cotangent(B=1, seed=5):
    """A fixed random cotangent on rows 0-2 of the result, fp32 values (the device takes it as fp32)."""
    g = torch.zeros(B, 4, 4)
    g[:, :3] = torch.randn(B, 3, 4, generator=torch.Generator().manual_seed(seed))
    return g


@functools.lru_cache(maxsize=None)
def oracle_gradients(name, sign):
    """{n: (gconf [N], gTinit [4,4])} for every n of N_ITERS from ONE 10-iteration oracle run: the trajectory's best[n] is the result of
    n_iterations = n and carries the graph.  Also the trajectory (detached)."""
    from oracle import ba2view as OB
    s = scene(name)
    conf = s["conf"].double().clone().requires_grad_(True)
    Ti = s["T_init"].double().clone().requires_grad_(True)
    _, valid, traj = OB.run_bundle_adjust_2_view(s["k0"].double(), s["k1"].double(), conf, Ti, N_MAX, homogeneous_sign=sign, return_trajectory=True)
    assert bool(valid.all())
    gT = cotangent()[0].double()
    out = {}
    for n in N_ITERS:
        gc, gt = torch.autograd.grad((traj[0]["best"][n] * gT).sum(), [conf, Ti], retain_graph=True, allow_unused=True)
        out[n] = (torch.zeros_like(conf[0]) if gc is None else gc[0], gt[0])
    return out, {k: v.detach() for k, v in traj[0].items()}


@functools.lru_cache(maxsize=None)
def restated(name, sign, n):
    s = scene(name)
    T, valid, gconf, gTi, tapes = br.run(s["k0"], s["k1"], s["conf"], s["T_init"], n, cotangent(), sign)
    assert bool(valid.all())
    return T[0], gconf[0], gTi[0], tapes[0]


def pattern(accepted):
    return "".join("A" if a else "r" for a in list(accepted)[1:])


# ------------------------------------------------------------------------------------------------ restatement against autograd


@pytest.mark.parametrize("sign", [+1, -1])
@pytest.mark.parametrize("name", list(CASES))
def test_restatement_is_autograd_through_the_oracle(name, sign):
    """gconf and rows 0-3 of gTinit, every n of N_ITERS, both signs of the null vector.  Both sides are fp64 evaluations of one function:
    the bar is 1e-9 max|g|.  Measured on the four cases (largest over n and sign, relative to max|g|): gconf 1.0e-10, gTinit 2.9e-12 at
    n = 5 and 10; 1.2e-13 and 1.8e-14 at n <= 3 (the restatement solves through the Schur complement, the oracle a dense LU)."""
    want, traj = oracle_gradients(name, sign)
    for n in N_ITERS:
        T, gconf, gTi, tape = restated(name, sign, n)
        assert pattern(tape["accepted"]) == pattern(traj["accepted"].tolist())[:n], (name, n)
        assert float((T - traj["best"][n]).abs().max()) <= 1e-9, (name, n)
        gc, gt = want[n]
        for what, a, b in (("gconf", gconf, gc), ("gTinit", gTi, gt)):
            scale = float(b.abs().max())
            err = float((a - b).abs().max())
            print(f"{name} sign={sign:+d} n={n} {what}: |restated - autograd| = {err:.2e}, max|g| = {scale:.2e}, k* = {tape['kstar']}")
            assert bool(a.isfinite().all()) and err <= 1e-9 * scale, (name, sign, n, what, err, scale)
        if n == 0:
            assert float(gconf.abs().max()) == 0.0 and torch.equal(gTi[:3], cotangent()[0, :3].double()) and float(gTi[3].abs().max()) == 0.0
        else:
            assert float(gt[3].abs().max()) > 0.0  # the oracle's row 3 is reached (a stated difference of the device, which returns 0)


def test_restatement_of_an_invalid_sample_and_of_masked_rows():
    s = S.make_scene(8, 301)
    s["conf"][0, 6:] = 0.0
    T, valid, gconf, gTi, tapes = br.run(s["k0"], s["k1"], s["conf"], s["T_init"], 3, cotangent(), +1)
    assert valid.tolist() == [False] and tapes == [None] and torch.equal(T, s["T_init"].double())
    assert float(gconf.abs().max()) == 0.0 and torch.equal(gTi[0, :3], cotangent()[0, :3].double()) and float(gTi[0, 3].abs().max()) == 0.0
    # masked rows get exactly 0 and their garbage reaches nothing
    f = scene("f_n257_garbage")
    _, gconf, gTi, _ = restated("f_n257_garbage", +1, 3)
    off = torch.ones(257, dtype=torch.bool)
    off[f["keep"]] = False
    assert bool((gconf[off] == 0).all()) and bool(gconf.isfinite().all()) and bool(gTi.isfinite().all()) and float(gconf[~off].abs().min()) > 0


# ------------------------------------------------------------------------------------------------ one step against differences


def test_step_adjoint_is_the_central_difference_of_one_restated_step():
    """One LM step of the 7-match scene at its start, lambda = 0.1: F = <G, Rt'> + <H, X'> for fixed random G, H as a function of the
    pose (12), the points (21) and the weights (7), one coordinate at a time, h = 1e-5.  The bar is derived:
    * truncation: D(h) - F' = h^2 F''' / 6 + ..., so (D(2h) - D(h)) / 3 estimates it; allowed is 3 x that;
    * rounding: the step solves a system whose Jacobi-scaled matrix C + lambda I has a unit-diagonal positive semi-definite C, so its
      largest eigenvalue is at most trace(C) + lambda = 6 + 3 M + lambda and its condition at most kappa = (6 + 3 M + lambda) / lambda;
      the step, and with it F, is off by at most 16 eps kappa S with S = sum |G o Rt'| + sum |H o X'| (16 roundings per entry as in
      tests/test_ba2view_loss.py), and D(h), a difference of two such values over 2h, by 16 eps kappa S / h."""
    s = scene("a_n7")
    x0, x1, conf = s["k0"][0].double(), s["k1"][0].double(), s["conf"][0].double()
    c = conf / conf.sum()
    Rt = s["T_init"][0, :3].double()
    X = br.triangulate(Rt, x0, x1, +1)
    M, lam = 7, 0.1
    gen = torch.Generator().manual_seed(9)
    G, H = torch.randn(3, 4, generator=gen, dtype=F64), torch.randn(M, 3, generator=gen, dtype=F64)

    def step(Rt, X, c):
        st = br.lm_step(Rt, X, x0, x1, c, lam)
        assert st["ok"] and st["precond"]
        return br.exp_step(st["dc"], Rt), X + st["dp"], st

    Rn, Xn, st = step(Rt, X, c)
    dcb, through, _ = br.exp_step_reverse(st["dc"], Rt, G)
    dX, dRt, dcw = br.lm_step_reverse(st, Rt, X, x0, x1, c, dcb, H)
    adj = torch.cat([(through + dRt).reshape(-1), (H + dX).reshape(-1), dcw])

    def F(v):
        Rn, Xn, _ = step(v[:12].view(3, 4), v[12:12 + 3 * M].view(M, 3), v[12 + 3 * M:])
        return float((G * Rn).sum() + (H * Xn).sum())

    v0 = torch.cat([Rt.reshape(-1), X.reshape(-1), c])
    S_abs = float((G * Rn).abs().sum() + (H * Xn).abs().sum())
    h, eps = 1e-5, 2.0 ** -52
    rounding = 16.0 * eps * (6 + 3 * M + lam) / lam * S_abs / h

    def D(k, h):
        e = torch.zeros_like(v0)
        e[k] = h
        return (F(v0 + e) - F(v0 - e)) / (2.0 * h)

    worst = 0.0
    for k in range(len(v0)):
        d1, d2 = D(k, h), D(k, 2.0 * h)
        tol = abs(d2 - d1) + rounding
        worst = max(worst, abs(float(adj[k]) - d1) / tol)
        assert abs(float(adj[k]) - d1) <= tol, (k, float(adj[k]), d1, tol)
    print("largest |adjoint - D(h)| / bar", worst, "largest adjoint entry", float(adj.abs().max()), "rounding term", rounding)


# ------------------------------------------------------------------------------------------------ premises


def test_premises_of_the_comparison_hold_on_the_chosen_cases():
    clamped_steps, free_steps, rejected_before_kstar, early_kstar = 0, 0, [], []
    for name in CASES:
        s = scene(name)
        cf = s["conf"][0][s["conf"][0] > 0].double()
        assert 2.0 * float(cf.sum()) > 1e-6, name  # the weights' denominator is the sum, not the clamp
        tp, tm = restated(name, +1, N_MAX)[3], restated(name, -1, N_MAX)[3]
        # both signs decide alike, none of the decisions on a tie
        assert pattern(tp["accepted"]) == pattern(tm["accepted"]) and tp["kstar"] == tm["kstar"], name
        for tr in (tp, tm):
            cost, before = torch.tensor(tr["cost"][1:], dtype=F64), torch.tensor(tr["best_before"][1:], dtype=F64)
            assert bool(cost.isfinite().all()) and float(((cost - before).abs() / before.abs()).min()) >= TIE_GAP, name
            for st in tr["steps"]:
                assert st["ok"] and st["precond"], name                       # precond everywhere, no skipped step
                assert float(st["dpp"].min()) > 1e-12 and float(st["dcc"].min()) > 1e-12, name  # no diagonal entry at the floor
                n2 = float((st["dc"][3:] ** 2).sum())
                assert abs(n2 - 1e-4) > 1e-6 * 1e-4, (name, n2)               # no step at the boundary of the exponential's clamp
                clamped_steps += n2 < 1e-4
                free_steps += n2 >= 1e-4
        p = pattern(tp["accepted"])
        print(f"{name}: pattern {p}, k* = {tp['kstar']}, clamped steps {[bool((st['dc'][3:] ** 2).sum() < 1e-4) for st in tp['steps']]}")
        if "r" in p[:tp["kstar"]]:
            rejected_before_kstar.append(name)
        if tp["kstar"] < N_MAX:
            early_kstar.append(name)
    assert clamped_steps > 0 and free_steps > 0, (clamped_steps, free_steps)
    assert rejected_before_kstar and early_kstar, (rejected_before_kstar, early_kstar)


# ------------------------------------------------------------------------------------------------ C ABI and Python front

NAME, BASE = "e2emv_ba_2view_backward", "e2emv_ba_2view"


def test_header_declares_and_library_exports_the_entry(lib_built):
    from e2e_multi_view_matching_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "e2emv.h")).read()
    assert NAME in set(re.findall(r"\b(e2emv_[a-z0-9_]+)\s*\(", hdr))
    assert NAME in _lib.SIGNATURES and hasattr(ctypes.CDLL(lib_built), NAME) and hasattr(ctypes.CDLL(lib_built), BASE)
    norm = lambda t: [" ".join(x.split()) for x in t.split(",")]  # noqa: E731
    decl = norm(re.search(r"int %s\((.*?)\);" % NAME, hdr, re.S).group(1))
    old = norm(re.search(r"int %s\((.*?)\);" % BASE, hdr, re.S).group(1))
    # the forward's inputs, then the incoming gradient, the two outputs and the stream
    assert decl == old[:-3] + ["const float* d_gT", "float* d_gconf", "float* d_gTinit", "void* stream"]
    sig = _lib.SIGNATURES[NAME]
    assert sig[0] is ctypes.c_int and len(sig[1]) == len(decl) == 12
    assert open(os.path.join(ROOT, "INTEGRATION.md")).read().count("`%s`" % NAME) >= 1


def test_null_context_is_rejected(lib_built):
    from e2e_multi_view_matching_amd import _lib
    lib = _lib.load_library()
    assert lib.e2emv_ba_2view_backward(None, 1, 8, None, None, None, None, 1, None, None, None, None) == _lib.EINVAL


class _Recorder:
    """Stands in for the device context: records the entry points that are called, fills nothing."""

    def __init__(self):
        self.calls = []

    def call(self, name, *args):
        self.calls.append(name)


def _stub_device(monkeypatch):
    from e2e_multi_view_matching_amd import _lib, pose
    rec = _Recorder()
    monkeypatch.setattr(_lib, "context", lambda dev: rec)
    monkeypatch.setattr(_lib, "stream_ptr", lambda dev: None)
    monkeypatch.setattr(pose, "_dev_of", lambda *t: torch.device("cpu"))

    class _NoDevice:
        def __init__(self, dev):
            pass

        def __enter__(self):
            return self

        def __exit__(self, *a):
            return False

    monkeypatch.setattr(torch.cuda, "device", _NoDevice)
    return rec


@pytest.mark.parametrize("loss", ["huber", "cauchy"])
def test_a_robust_loss_with_a_graph_raises_before_any_device_call(loss, monkeypatch):
    from e2e_multi_view_matching_amd import pose
    L._no_device(monkeypatch)
    z = torch.zeros(1, 8, 2)
    for conf, Ti in ((torch.ones(1, 8, requires_grad=True), torch.eye(4)[None]), (torch.ones(1, 8), torch.eye(4)[None].clone().requires_grad_(True))):
        with pytest.raises(NotImplementedError, match="squared"):
            pose.run_bundle_adjust_2_view(z, z, conf, Ti, 3, loss=loss, loss_scale=1.0)
        with torch.no_grad(), pytest.raises(AssertionError, match="a device call was made"):  # no graph asked for: the robust path as before
            pose.run_bundle_adjust_2_view(z, z, conf, Ti, 3, loss=loss, loss_scale=1.0)


def test_without_a_graph_the_existing_entry_is_called_and_with_one_the_function(monkeypatch):
    from e2e_multi_view_matching_amd import pose
    rec = _stub_device(monkeypatch)
    z = torch.zeros(2, 8, 2)
    T, vb = pose.run_bundle_adjust_2_view(z, z, torch.ones(2, 8), torch.eye(4)[None].repeat(2, 1, 1), 3)
    assert rec.calls == ["e2emv_ba_2view"] and T.grad_fn is None
    rec.calls.clear()
    pose.run_bundle_adjust_2_view(z, z, torch.ones(2, 8), torch.eye(4)[None].repeat(2, 1, 1), 3, return_summary=True)
    pose.run_bundle_adjust_2_view(z, z, torch.ones(2, 8), torch.eye(4)[None].repeat(2, 1, 1), 3, loss="cauchy", loss_scale=1.0)
    assert rec.calls == ["e2emv_ba_2view_loss", "e2emv_ba_2view_loss"]
    rec.calls.clear()
    conf = torch.ones(2, 8, 1, requires_grad=True)
    with torch.no_grad():
        pose.run_bundle_adjust_2_view(z, z, conf, torch.eye(4)[None].repeat(2, 1, 1), 3)
    assert rec.calls == ["e2emv_ba_2view"]
    rec.calls.clear()
    T, vb = pose.run_bundle_adjust_2_view(z, z, conf, torch.eye(4)[None].repeat(2, 1, 1), 3)
    assert rec.calls == ["e2emv_ba_2view"] and T.grad_fn is not None
    T.sum().backward()
    assert rec.calls == ["e2emv_ba_2view", "e2emv_ba_2view_backward"] and conf.grad is not None and conf.grad.shape == conf.shape


def test_mask_confidence_is_differentiable_through_the_same_kernel(monkeypatch):
    from e2e_multi_view_matching_amd import pose
    rec = _stub_device(monkeypatch)
    conf = torch.ones(2, 8, requires_grad=True)
    out = pose.mask_confidence(conf, torch.ones(2, 8, dtype=torch.bool))
    assert rec.calls == ["e2emv_apply_mask"] and out.grad_fn is not None
    out.sum().backward()
    assert rec.calls == ["e2emv_apply_mask", "e2emv_apply_mask"] and conf.grad.shape == conf.shape
    rec.calls.clear()
    assert pose.mask_confidence(conf.detach(), torch.ones(2, 8, dtype=torch.bool)).grad_fn is None and rec.calls == ["e2emv_apply_mask"]
