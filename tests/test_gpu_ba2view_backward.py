"""``e2emv_ba_2view_backward`` on the device against the fp64 restatement of the reverse pass (tests/ba2view_backward_restatement.py, which
tests/test_ba2view_backward.py pins to ``torch.autograd`` through oracle/ba2view.py), at the smallest shapes where ``ba2view_backward_kernel``
can go wrong: 6 positive confidences in 8 rows (invalid pair), 7 in 8 (smallest valid), 65 (a row in the second wave), 257 (thread 0 owns
two matches) with 157 masked rows of garbage, and two scenes with rejected steps; ``n_iterations`` 0, 1, 3, 10.

Method as in tests/test_gpu_ba_steps.py: kernel and restatement share the algorithm and fp64; the one freedom between them is the sign of
the DLT null vector, which ``1 / (w + 1e-8)`` turns into a relative ~1e-8 difference of the start points.  The restatement runs with the
sign forced both ways; delta_g = max |g+ - g-| brackets that freedom and the device has to be within

    |g - (g+ + g-) / 2|  <=  REL_BAR max|g|  +  4 delta_g          elementwise, for gconf and for rows 0-2 of gTinit.

REL_BAR = 1.3e-5 is ten times the largest distance measured on the MI355X (MEASURED below) and, with the largest 4 delta_g of 4e-6,
stays fifty times under the project's gradient bar of 1e-3 max|g|, which every comparison asserts.  The device sits on one
of the two sign runs rather than between them - its distance from the midpoint is about delta_g / 2 throughout - so what is measured
is the sign freedom and the fp32 rounding of the outputs (6e-8), not an error of the reverse pass."""
import functools

import numpy as np
import pytest
import torch

import ba2view_backward_restatement as br
import test_ba2view_loss as L
import test_gpu_ba_steps as S
from test_ba2view_backward import CASES as CPU_CASES
from test_ba2view_backward import cotangent, oracle_gradients, pattern

pytestmark = [pytest.mark.gpu]

REL_BAR = 1.3e-5
GRADIENT_BAR = 1e-3
N_ITERS = [0, 1, 3, 10]
# MEASURED (MI355X; |g - mid| / max|g| and delta_g / max|g|, largest over n = 1, 3, 10):
#   case               gconf                gTinit
#   a_n7               2.9e-7 / 5.8e-7      1.8e-7 / 2.7e-7
#   b_n8_hole0         2.4e-7 / 4.8e-7      3.5e-8 / 8.3e-8
#   c_n65              5.1e-7 / 9.9e-7      9.3e-8 / 1.8e-7
#   f_n257_garbage     1.5e-7 / 2.9e-7      6.6e-8 / 7.8e-8
#   i_n90_far          5.3e-8 / 1.1e-7      5.0e-8 / 1.7e-8
#   j_n257_outliers    8.0e-8 / 1.6e-7      8.6e-8 / 2.1e-7
#   a_n7, c_n65 against autograd through the oracle: the same figures to the digits shown
#   end to end (w8pt -> mask -> BA -> pose errors), conf.grad: 1.23e-6 / 1.7e-7 - the largest distance, from which REL_BAR follows;
#   the w8pt-only gradient of the same loss lies 0.85 max|g| away


def _six_of_eight():
    s = S.make_scene(8, 301)
    s["conf"][0, 6:] = 0.0
    return s


CASES = dict(CPU_CASES)
CASES.update({
    "six_of_8_invalid": _six_of_eight,
    "i_n90_far": S.CASES["i_n90_far"],                      # AAAArArArA: rejected steps before k*
    "j_n257_outliers": L.CASES["j_n257_outliers"][0],       # AAArArAAAr: k* = 9 < 10, every row valid, thread 0 owns rows 0 and 256
})


@functools.lru_cache(maxsize=None)
def scene(name):
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def restated(name, n):
    """((gconf+, gTinit+, tape+), (gconf-, gTinit-, tape-)) of a case: shared, never modified."""
    s = scene(name)
    out = []
    for sign in (+1, -1):
        _, _, gconf, gTi, tapes = br.run(s["k0"], s["k1"], s["conf"], s["T_init"], n, cotangent(), sign)
        out.append((gconf[0], gTi[0], tapes[0]))
    return tuple(out)


def device_backward(gpu, k0, k1, conf, Ti, n, gT, want_conf=True, want_T=True):
    """The C entry directly; outputs start as NaN so that an entry the kernel leaves out shows."""
    from e2e_multi_view_matching_amd import _lib
    ctx = _lib.context(gpu)
    k0, k1, conf, Ti, gT = (t.to(gpu, torch.float32).contiguous() for t in (k0, k1, conf, Ti, gT))
    B, N = conf.shape
    gconf = torch.full((B, N), float("nan"), device=gpu) if want_conf else None
    gTi = torch.full((B, 4, 4), float("nan"), device=gpu) if want_T else None
    with torch.cuda.device(gpu):
        ctx.call("e2emv_ba_2view_backward", B, N, _lib.ptr(k0), _lib.ptr(k1), _lib.ptr(conf), _lib.ptr(Ti), int(n), _lib.ptr(gT),
                 _lib.ptr(gconf), _lib.ptr(gTi), _lib.stream_ptr(gpu))
    torch.cuda.synchronize(gpu)
    return (gconf.cpu() if want_conf else None), (gTi.cpu() if want_T else None)


def _compare(tag, got, plus, minus):
    """-> (|got - mid| / max|g|, delta_g / max|g|) after asserting the bar."""
    got, mid = got.double(), 0.5 * (plus + minus)
    scale = float(mid.abs().max())
    delta = float((plus - minus).abs().max())
    dist = float((got - mid).abs().max())
    print(f"{tag}: |g - mid| = {dist:.3e}  delta_g = {delta:.3e}  max|g| = {scale:.3e}  -> {dist / max(scale, 1e-300):.2e} / {delta / max(scale, 1e-300):.2e}")
    assert bool(got.isfinite().all()), tag
    assert REL_BAR * scale + 4.0 * delta <= GRADIENT_BAR * scale or scale == 0.0, (tag, "the bracket makes the bar vacuous", delta, scale)
    assert dist <= REL_BAR * scale + 4.0 * delta, (tag, dist, scale, delta)
    return dist / max(scale, 1e-300), delta / max(scale, 1e-300)


@pytest.mark.parametrize("name", list(CASES))
def test_device_matches_the_restatement(gpu, name):
    s = scene(name)
    valid_pair = int((s["conf"] > 0).sum()) > 6
    assert valid_pair == (name != "six_of_8_invalid")
    for n in N_ITERS:
        gconf, gTi = device_backward(gpu, s["k0"], s["k1"], s["conf"], s["T_init"], n, cotangent())
        assert torch.equal(gTi[0, 3], torch.zeros(4)), (name, n)  # row 3: the device reads rows 0-2 of T_init only
        off = ~(s["conf"][0] > 0)
        assert bool((gconf[0, off] == 0).all()), (name, n)         # masked rows, whatever garbage they hold
        (gcp, gtp, tp), (gcm, gtm, tm) = restated(name, n)
        if not valid_pair or n == 0:
            assert tp is None or tp["kstar"] == 0
            assert bool((gconf == 0).all()) and torch.equal(gTi[0, :3], cotangent()[0, :3]), (name, n)
            continue
        assert pattern(tp["accepted"]) == pattern(tm["accepted"]) and tp["kstar"] == tm["kstar"] > 0, (name, n)
        _compare(f"{name} n={n} k*={tp['kstar']} [{pattern(tp['accepted'])}] gconf", gconf[0], gcp, gcm)
        _compare(f"{name} n={n} gTinit", gTi[0, :3], gtp[:3], gtm[:3])
    if name == "f_n257_garbage":
        assert int(off.sum()) == 157 and bool(s["k0"][0, off].isnan().any()) and float(s["conf"][0, 256]) > 0


@pytest.mark.parametrize("name", ["a_n7", "c_n65"])
def test_device_matches_autograd_through_the_oracle(gpu, name):
    """The same comparison fed from oracle/ba2view.py directly (dense normal equations, library LU and SVD, torch.autograd), so that the
    chain oracle -> device does not rest on the restatement alone."""
    s = scene(name)
    (want_p, _), (want_m, _) = oracle_gradients(name, +1), oracle_gradients(name, -1)
    for n in (1, 3, 10):
        gconf, gTi = device_backward(gpu, s["k0"], s["k1"], s["conf"], s["T_init"], n, cotangent())
        _compare(f"{name} n={n} gconf vs autograd", gconf[0], want_p[n][0], want_m[n][0])
        _compare(f"{name} n={n} gTinit vs autograd", gTi[0, :3], want_p[n][1][:3], want_m[n][1][:3])


def test_either_output_may_be_null(gpu):
    s = scene("c_n65")
    both = device_backward(gpu, s["k0"], s["k1"], s["conf"], s["T_init"], 3, cotangent())
    only_c = device_backward(gpu, s["k0"], s["k1"], s["conf"], s["T_init"], 3, cotangent(), want_T=False)
    only_T = device_backward(gpu, s["k0"], s["k1"], s["conf"], s["T_init"], 3, cotangent(), want_conf=False)
    neither = device_backward(gpu, s["k0"], s["k1"], s["conf"], s["T_init"], 3, cotangent(), want_conf=False, want_T=False)
    assert only_c[1] is None and only_T[0] is None and neither == (None, None)
    assert torch.equal(only_c[0], both[0]) and torch.equal(only_T[1], both[1]) and float(both[0].abs().max()) > 0


def test_shape_errors_and_a_tape_that_does_not_fit(gpu):
    """The shape rules of ``e2emv_ba_2view``; a tape whose size does not fit a size_t is E2EMV_ENOMEM from the host-side check - nothing is
    reserved, launched or read -, and the context goes on working."""
    from e2e_multi_view_matching_amd import _lib
    ctx = _lib.context(gpu)
    lib, h, sp = ctx.lib, ctx.h, _lib.stream_ptr(gpu)
    z = _lib.ptr(torch.zeros(64, device=gpu))
    call = lambda B, N, n: lib.e2emv_ba_2view_backward(h, B, N, z, z, z, z, n, z, z, z, sp)  # noqa: E731
    assert call(0, 8, 3) == _lib.ESHAPE and call(1, 0, 3) == _lib.ESHAPE and call(1, 8, -1) == _lib.ESHAPE
    assert lib.e2emv_ba_2view_backward(h, 1, 8, z, z, z, z, 3, None, z, z, sp) == _lib.EINVAL
    big = 2 ** 31 - 1
    assert call(big, big, big) == _lib.ENOMEM and b"size_t" in lib.e2emv_last_error(h)
    assert call(1, big, big) == _lib.ENOMEM and b"size_t" in lib.e2emv_last_error(h)
    s = scene("c_n65")
    gconf, gTi = device_backward(gpu, s["k0"], s["k1"], s["conf"], s["T_init"], 3, cotangent())
    assert bool(gconf.isfinite().all()) and bool(gTi.isfinite().all()) and float(gconf.abs().max()) > 0


def test_batch_position_independence_and_repeatability(gpu):
    """N = 257: [A, six positive confidences, B] and the permutations that put A first, last and alone; the same bits every time."""
    A, Bs = scene("f_n257_garbage"), scene("j_n257_outliers")
    six = S.make_scene(257, 302)
    six["conf"][0, np.setdiff1d(np.arange(257), [0, 17, 255, 256, 100, 200])] = 0.0
    assert int((six["conf"] > 0).sum()) == 6
    gT = cotangent(3, seed=8)
    alone = {id(x): device_backward(gpu, x["k0"], x["k1"], x["conf"], x["T_init"], 3, gT[i:i + 1]) for i, x in ((0, A), (2, Bs))}

    def run(order, rows):
        cat = lambda k: torch.cat([x[k] for x in order])  # noqa: E731
        return device_backward(gpu, cat("k0"), cat("k1"), cat("conf"), cat("T_init"), 3, gT[rows])

    gc, gt = run([A, six, Bs], [0, 1, 2])
    gc2, gt2 = run([A, six, Bs], [0, 1, 2])
    assert torch.equal(gc, gc2) and torch.equal(gt, gt2)                      # repeated call (NaN nowhere: equal means bits)
    assert bool(gc.isfinite().all()) and bool(gt.isfinite().all())
    assert torch.equal(gc[0:1], alone[id(A)][0]) and torch.equal(gt[0:1], alone[id(A)][1])
    assert torch.equal(gc[2:3], alone[id(Bs)][0]) and torch.equal(gt[2:3], alone[id(Bs)][1])
    assert bool((gc[1] == 0).all()) and torch.equal(gt[1, :3], gT[1, :3]) and bool((gt[1, 3] == 0).all())  # the invalid neighbour
    gc3, gt3 = run([Bs, six, A], [2, 1, 0])                                   # A last, B first
    assert torch.equal(gc3[2:3], alone[id(A)][0]) and torch.equal(gt3[2:3], alone[id(A)][1])
    assert torch.equal(gc3[0:1], alone[id(Bs)][0]) and torch.equal(gt3[0:1], alone[id(Bs)][1])


def test_python_route_fills_both_gradients(gpu):
    """``T.sum().backward()`` through ``run_bundle_adjust_2_view``: the gradients are those of the C entry for a cotangent of ones, the
    boolean selection of the valid samples works with an invalid sample in the batch, and without a graph nothing changes."""
    import e2e_multi_view_matching_amd as E
    A, six, C = scene("c_n65"), S.make_scene(65, 305), S.make_scene(65, 306)
    six["conf"][0, 6:] = 0.0
    cat = lambda k: torch.cat([x[k] for x in (A, six, C)]).to(gpu)  # noqa: E731
    conf = cat("conf").unsqueeze(-1).clone().requires_grad_(True)   # [B,N,1] as the reference passes it
    Ti = cat("T_init").clone().requires_grad_(True)
    T, vb = E.run_bundle_adjust_2_view(cat("k0"), cat("k1"), conf, Ti, n_iterations=3)
    assert vb.tolist() == [True, False, True] and T.shape == (2, 4, 4) and T.grad_fn is not None
    T.sum().backward()
    assert conf.grad is not None and conf.grad.shape == conf.shape and Ti.grad is not None and Ti.grad.shape == Ti.shape
    gT = torch.ones(3, 4, 4)
    gT[1] = 0.0  # the selection leaves the invalid sample out of the sum
    gc, gt = device_backward(gpu, cat("k0"), cat("k1"), cat("conf"), cat("T_init"), 3, gT)
    assert torch.equal(conf.grad.cpu()[..., 0], gc) and torch.equal(Ti.grad.cpu(), gt)
    assert float(gc[0].abs().max()) > 0 and float(gc[2].abs().max()) > 0 and bool((gc[1] == 0).all()) and bool((gt[1] == 0).all())
    # the same call without a graph: the bits of before, no grad_fn
    T0, vb0 = E.run_bundle_adjust_2_view(cat("k0"), cat("k1"), conf.detach(), Ti.detach(), n_iterations=3)
    assert T0.grad_fn is None and torch.equal(T0, T.detach()) and torch.equal(vb0, vb)
    with pytest.raises(NotImplementedError):
        E.run_bundle_adjust_2_view(cat("k0"), cat("k1"), conf, Ti, n_iterations=3, loss="huber", loss_scale=1 / 600)


def test_end_to_end_pose_loss_reaches_the_confidences_through_the_refinement(gpu):
    """conf (leaf) -> estimate_relative_pose_w8pt -> mask_confidence -> run_bundle_adjust_2_view -> pose errors -> backward(), the eval flow
    of eval_pairs.py:250-255 as a training step, against autograd over the oracle chain (oracle/w8pt.py, oracle/ba2view.py with the null
    vector's sign forced both ways, the pose errors of oracle/w8pt.py).  The target pose lies a few tenths of a radian from the estimate so
    that the arccos of the two errors is well conditioned on an fp32 pose.  The leaf goes into the mask (``info["confidence"]``, the
    normalised copy, carries no graph on the device; the bundle adjustment normalises its weights itself)."""
    import e2e_multi_view_matching_amd as E
    from oracle import ba2view as OB
    from oracle import w8pt as OW
    from test_gpu_backward import _two_view_scene
    B, N, n_it = 2, 64, 3
    k0, k1, Kc, Tgt, conf, _ = _two_view_scene(B, N, seed=21)
    _, _, _, Ttarget, _, _ = _two_view_scene(B, N, seed=22)
    k0 = (k0 - Kc[:, None, :2, 2]) / torch.stack([Kc[:, 0, 0], Kc[:, 1, 1]], -1)[:, None]
    k1 = (k1 - Kc[:, None, :2, 2]) / torch.stack([Kc[:, 0, 0], Kc[:, 1, 1]], -1)[:, None]
    Kc = torch.eye(4).unsqueeze(0).repeat(B, 1, 1)

    def errors(mod, T, target):
        return 1.5 * mod.compute_rotation_error(T, target) + 0.7 * mod.compute_translation_error_as_angle(T, target)

    grads = []
    for sign in (+1, -1):
        c_ref = conf.double().clone().requires_grad_(True)
        T0r, info_r = OW.estimate_relative_pose_w8pt(k0.double(), k1.double(), Kc.double(), Kc.double(), c_ref)
        cm = c_ref * info_r["pos_depth_mask"].unsqueeze(-1).double()
        T1r, vbr = OB.run_bundle_adjust_2_view(info_r["kpts0_norm"], info_r["kpts1_norm"], cm, T0r, n_it, homogeneous_sign=sign)
        assert bool(vbr.all())
        errors(OW, T1r, Ttarget.double()).backward()
        grads.append(c_ref.grad[..., 0])
    c = conf.to(gpu).clone().requires_grad_(True)
    T0, info = E.estimate_relative_pose_w8pt(k0.to(gpu), k1.to(gpu), Kc.to(gpu), Kc.to(gpu), c)
    assert torch.equal(info["pos_depth_mask"].cpu(), info_r["pos_depth_mask"])
    T1, vb = E.run_bundle_adjust_2_view(info["kpts0_norm"], info["kpts1_norm"], E.mask_confidence(c, info["pos_depth_mask"]), T0, n_iterations=n_it)
    assert bool(vb.all()) and T1.grad_fn is not None
    errors(E, T1, Ttarget.to(gpu)).backward()
    g_full = c.grad.cpu()[..., 0]
    dist, _ = _compare("end to end conf.grad", g_full, grads[0], grads[1])
    # the BA term really arrived: the gradient of the same loss on the w8pt pose alone is another one
    c2 = conf.to(gpu).clone().requires_grad_(True)
    T0b, _ = E.estimate_relative_pose_w8pt(k0.to(gpu), k1.to(gpu), Kc.to(gpu), Kc.to(gpu), c2)
    errors(E, T0b, Ttarget.to(gpu)).backward()
    apart = float((c2.grad.cpu()[..., 0] - g_full).abs().max()) / float(g_full.abs().max())
    print(f"w8pt-only gradient differs from the refined one by {apart:.2e} max|g|")
    assert apart > 100.0 * GRADIENT_BAR
