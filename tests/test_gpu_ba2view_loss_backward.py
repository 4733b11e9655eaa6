"""``e2emv_ba_2view_loss_backward`` on the device against the fp64 restatement of the reverse pass through the Huber and Cauchy losses
(tests/ba2view_loss_backward_restatement.py, which tests/test_ba2view_loss_backward.py pins to ``torch.autograd`` through the dense
robust loop with the scale as a tensor), at the smallest shapes where ``ba2view_backward_kernel<LOSS>`` can go wrong: 6 positive
confidences in 8 rows (invalid pair), 7 in 7 and in 8 (smallest valid, masked row 0), 65 (a row in the second wave), 257 (thread 0 owns
two matches) with 157 masked rows of garbage and with 10 % wrong matches, and 65 with the clamped denominator; ``n_iterations`` 0, 1, 3,
10; both losses at the case's scale of tests/test_ba2view_loss.py.

Method as in tests/test_gpu_ba2view_backward.py: kernel and restatement share the algorithm and fp64; the one freedom between them is the
sign of the DLT null vector.  The restatement runs with the sign forced both ways; delta_g = max |g+ - g-| brackets that freedom and the
device has to be within

    |g - (g+ + g-) / 2|  <=  REL_BAR max|g|  +  4 delta_g          elementwise, for gconf and for rows 0-2 of gTinit.

REL_BAR = 1.8e-5 is ten times the largest distance measured on the MI355X (1.77e-6, MEASURED below) and, with the largest 4 delta_g of
1.4e-5, stays thirty times under the project's gradient bar of 1e-3 max|g|, which every comparison asserts.  As in the
squared-loss tests the device sits on one of the two sign runs - its distance from the midpoint is about delta_g / 2 throughout -, so
what is measured is the sign freedom and the fp32 rounding of the outputs, not an error of the reverse pass.  The premises (both sign
runs decide alike, no decision on a tie, no observation at Huber's kink, ...) are asserted on the CPU by
tests/test_ba2view_loss_backward.py for every case used here."""
import functools

import numpy as np
import pytest
import torch

import ba2view_backward_restatement as br
import ba2view_loss_backward_restatement as lb
import test_ba2view_loss as L
import test_gpu_ba_steps as S
from test_ba2view_backward import cotangent, pattern
from test_ba2view_loss_backward import autograd_gradients

pytestmark = [pytest.mark.gpu]

REL_BAR = 1.8e-5
GRADIENT_BAR = 1e-3
N_ITERS = [0, 1, 3, 10]
LOSSES = ["huber", "cauchy"]
CODE = {None: 0, "huber": 1, "cauchy": 2}
# MEASURED (MI355X; |g - mid| / max|g| and delta_g / max|g|, largest over n = 1, 3, 10):
#   case               gconf huber        gconf cauchy       gTinit huber       gTinit cauchy
#   a_n7               3.5e-7 / 7.5e-7    3.9e-7 / 7.7e-7    1.5e-7 / 2.7e-7    2.0e-7 / 4.3e-7
#   b_n8_hole0         2.8e-7 / 5.7e-7    1.8e-6 / 3.5e-6    7.1e-8 / 8.6e-8    1.0e-7 / 1.1e-7
#   c_n65              4.5e-7 / 8.7e-7    5.8e-7 / 1.1e-6    8.8e-8 / 1.8e-7    8.5e-8 / 1.7e-7
#   f_n257_garbage     1.7e-7 / 3.3e-7    2.6e-7 / 5.0e-7    9.6e-8 / 2.0e-7    5.7e-8 / 1.0e-7
#   j_n257_outliers    1.4e-7 / 2.3e-7    1.4e-6 / 2.7e-6    4.6e-7 / 8.7e-7    1.2e-6 / 2.1e-6
#   k_n65_clamp        4.3e-7 / 9.1e-7    4.4e-7 / 8.1e-7    8.8e-8 / 1.8e-7    9.1e-8 / 1.8e-7
#   a_n7, c_n65 against autograd through helper (a): the same figures to the digits shown
#   huber at loss_scale = 1e6 against the squared-loss restatement: a_n7 2.9e-7 / 5.8e-7 and 1.7e-7 / 2.7e-7, c_n65 5.1e-7 / 9.9e-7 and
#   9.3e-8 / 1.8e-7 - the figures of tests/test_gpu_ba2view_backward.py
#   pose_loss_tuple, cauchy against squared on a 3-tuple with four wrong matches per sample: 0.20, 13 and 1.9 max|g| apart per pair


def _six_of_eight():
    s = S.make_scene(8, 301)
    s["conf"][0, 6:] = 0.0
    return s


CASES = {
    "six_of_8_invalid": (_six_of_eight, L.PIXEL),
    "a_n7": L.CASES["a_n7"],
    "b_n8_hole0": L.CASES["b_n8_hole0"],
    "c_n65": L.CASES["c_n65"],
    "f_n257_garbage": L.CASES["f_n257_garbage"],
    "j_n257_outliers": L.CASES["j_n257_outliers"],  # 10 % wrong matches, a rejected step before k*, both Huber branches live to the end
    "k_n65_clamp": L.CASES["k_n65_clamp"],
}


@functools.lru_cache(maxsize=None)
def scene(name):
    return CASES[name][0]()


def scale_of(name):
    return CASES[name][1]


@functools.lru_cache(maxsize=None)
def restated(name, loss, n, scale=None):
    """((gconf+, gTinit+, tape+), (gconf-, gTinit-, tape-)) of a case: shared, never modified."""
    s = scene(name)
    out = []
    for sign in (+1, -1):
        _, _, gconf, gTi, tapes = lb.run(s["k0"], s["k1"], s["conf"], s["T_init"], n, cotangent(), sign, loss,
                                         (scale_of(name) if scale is None else scale) if loss else None)
        out.append((gconf[0], gTi[0], tapes[0]))
    return tuple(out)


def device_backward(gpu, k0, k1, conf, Ti, n, gT, loss, scale, want_conf=True, want_T=True, entry="e2emv_ba_2view_loss_backward"):
    """The C entry directly; outputs start as NaN so that an entry the kernel leaves out shows."""
    from e2e_multi_view_matching_amd import _lib
    ctx = _lib.context(gpu)
    k0, k1, conf, Ti, gT = (t.to(gpu, torch.float32).contiguous() for t in (k0, k1, conf, Ti, gT))
    B, N = conf.shape
    gconf = torch.full((B, N), float("nan"), device=gpu) if want_conf else None
    gTi = torch.full((B, 4, 4), float("nan"), device=gpu) if want_T else None
    head = (B, N, _lib.ptr(k0), _lib.ptr(k1), _lib.ptr(conf), _lib.ptr(Ti), int(n))
    tail = (_lib.ptr(gT), _lib.ptr(gconf), _lib.ptr(gTi), _lib.stream_ptr(gpu))
    with torch.cuda.device(gpu):
        if entry == "e2emv_ba_2view_backward":
            ctx.call(entry, *head, *tail)
        else:
            ctx.call(entry, *head, CODE[loss], float(scale) if loss else 0.0, *tail)
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


@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("name", list(CASES))
def test_device_matches_the_restatement(gpu, name, loss):
    s = scene(name)
    valid_pair = int((s["conf"] > 0).sum()) > 6
    assert valid_pair == (name != "six_of_8_invalid")
    for n in N_ITERS:
        gconf, gTi = device_backward(gpu, s["k0"], s["k1"], s["conf"], s["T_init"], n, cotangent(), loss, scale_of(name))
        assert torch.equal(gTi[0, 3], torch.zeros(4)), (name, n)  # row 3: the device reads rows 0-2 of T_init only
        off = ~(s["conf"][0] > 0)
        assert bool((gconf[0, off] == 0).all()), (name, n)         # masked rows, whatever garbage they hold: exact zeros
        (gcp, gtp, tp), (gcm, gtm, tm) = restated(name, loss, n)
        if not valid_pair or n == 0:
            assert tp is None or tp["kstar"] == 0
            assert bool((gconf == 0).all()) and torch.equal(gTi[0, :3], cotangent()[0, :3]), (name, n)
            continue
        assert pattern(tp["accepted"]) == pattern(tm["accepted"]) and tp["kstar"] == tm["kstar"] > 0, (name, n)
        _compare(f"{name} {loss} n={n} k*={tp['kstar']} [{pattern(tp['accepted'])}] gconf", gconf[0], gcp, gcm)
        _compare(f"{name} {loss} n={n} gTinit", gTi[0, :3], gtp[:3], gtm[:3])
    if name == "f_n257_garbage":
        assert int(off.sum()) == 157 and bool(s["k0"][0, off].isnan().any()) and float(s["conf"][0, 256]) > 0


@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("name", ["a_n7", "c_n65"])
def test_device_matches_autograd_through_the_robust_loop(gpu, name, loss):
    """The same comparison fed from helper (a) directly (dense normal equations, library LU and SVD, torch.autograd through the scale),
    so that the chain autograd -> device does not rest on the hand-written reverse alone."""
    s = scene(name)
    (want_p, _), (want_m, _) = autograd_gradients(name, loss, +1), autograd_gradients(name, loss, -1)
    for n in (1, 3, 10):
        gconf, gTi = device_backward(gpu, s["k0"], s["k1"], s["conf"], s["T_init"], n, cotangent(), loss, scale_of(name))
        _compare(f"{name} {loss} n={n} gconf vs autograd", gconf[0], want_p[n][0], want_m[n][0])
        _compare(f"{name} {loss} n={n} gTinit vs autograd", gTi[0, :3], want_p[n][1][:3], want_m[n][1][:3])


@pytest.mark.parametrize("name", ["c_n65", "f_n257_garbage", "six_of_8_invalid"])
def test_loss_none_through_the_new_entry_is_the_squared_loss_entry_bit_for_bit(gpu, name):
    s = scene(name)
    for n in N_ITERS:
        old = device_backward(gpu, s["k0"], s["k1"], s["conf"], s["T_init"], n, cotangent(), None, None, entry="e2emv_ba_2view_backward")
        new = device_backward(gpu, s["k0"], s["k1"], s["conf"], s["T_init"], n, cotangent(), None, None)
        assert bool(old[0].isfinite().all()) and bool(old[1].isfinite().all())
        assert torch.equal(old[0], new[0]) and torch.equal(old[1], new[1]), (name, n)  # (NaN nowhere: equal means bits)
    assert name == "six_of_8_invalid" or float(new[0].abs().max()) > 0


@pytest.mark.parametrize("name", ["a_n7", "c_n65"])
def test_huber_at_a_scale_no_block_reaches_is_the_squared_loss(gpu, name):
    """loss_scale = 1e6: every block on Huber's first branch.  The device is within the bracket of the SQUARED-loss restatement."""
    s = scene(name)
    for n in (1, 3, 10):
        gconf, gTi = device_backward(gpu, s["k0"], s["k1"], s["conf"], s["T_init"], n, cotangent(), "huber", 1e6)
        want = [br.run(s["k0"], s["k1"], s["conf"], s["T_init"], n, cotangent(), sign) for sign in (+1, -1)]
        _compare(f"{name} huber 1e6 n={n} gconf vs squared", gconf[0], want[0][2][0], want[1][2][0])
        _compare(f"{name} huber 1e6 n={n} gTinit vs squared", gTi[0, :3], want[0][3][0, :3], want[1][3][0, :3])


@pytest.mark.parametrize("loss", LOSSES)
def test_either_output_may_be_null(gpu, loss):
    s = scene("c_n65")
    a = (gpu, s["k0"], s["k1"], s["conf"], s["T_init"], 3, cotangent(), loss, L.PIXEL)
    both = device_backward(*a)
    only_c, only_T, neither = device_backward(*a, want_T=False), device_backward(*a, want_conf=False), device_backward(*a, want_conf=False, want_T=False)
    assert only_c[1] is None and only_T[0] is None and neither == (None, None)
    assert torch.equal(only_c[0], both[0]) and torch.equal(only_T[1], both[1]) and float(both[0].abs().max()) > 0


@pytest.mark.parametrize("loss", LOSSES)
def test_batch_position_independence_and_repeatability(gpu, loss):
    """N = 257: [A, six positive confidences, B] and the permutations that put A first, last and alone; the same bits every time."""
    A, Bs = scene("f_n257_garbage"), scene("j_n257_outliers")
    six = S.make_scene(257, 302)
    six["conf"][0, np.setdiff1d(np.arange(257), [0, 17, 255, 256, 100, 200])] = 0.0
    assert int((six["conf"] > 0).sum()) == 6
    gT = cotangent(3, seed=8)
    alone = {id(x): device_backward(gpu, x["k0"], x["k1"], x["conf"], x["T_init"], 3, gT[i:i + 1], loss, L.PIXEL) for i, x in ((0, A), (2, Bs))}

    def run(order, rows):
        cat = lambda k: torch.cat([x[k] for x in order])  # noqa: E731
        return device_backward(gpu, cat("k0"), cat("k1"), cat("conf"), cat("T_init"), 3, gT[rows], loss, L.PIXEL)

    gc, gt = run([A, six, Bs], [0, 1, 2])
    gc2, gt2 = run([A, six, Bs], [0, 1, 2])
    assert torch.equal(gc, gc2) and torch.equal(gt, gt2)
    assert bool(gc.isfinite().all()) and bool(gt.isfinite().all())
    assert torch.equal(gc[0:1], alone[id(A)][0]) and torch.equal(gt[0:1], alone[id(A)][1])
    assert torch.equal(gc[2:3], alone[id(Bs)][0]) and torch.equal(gt[2:3], alone[id(Bs)][1])
    assert bool((gc[1] == 0).all()) and torch.equal(gt[1, :3], gT[1, :3]) and bool((gt[1, 3] == 0).all())  # the invalid neighbour
    gc3, gt3 = run([Bs, six, A], [2, 1, 0])
    assert torch.equal(gc3[2:3], alone[id(A)][0]) and torch.equal(gt3[2:3], alone[id(A)][1])
    assert torch.equal(gc3[0:1], alone[id(Bs)][0]) and torch.equal(gt3[0:1], alone[id(Bs)][1])
    assert float(gc[0].abs().max()) > 0 and float(gc[2].abs().max()) > 0


def test_a_bad_loss_or_scale_is_the_forwards_error_and_the_context_goes_on(gpu):
    from e2e_multi_view_matching_amd import _lib
    ctx = _lib.context(gpu)
    lib, h, sp = ctx.lib, ctx.h, _lib.stream_ptr(gpu)
    z = _lib.ptr(torch.zeros(64, device=gpu))
    bwd = lambda loss, scale, B=1, N=8, n=3: lib.e2emv_ba_2view_loss_backward(h, B, N, z, z, z, z, n, loss, scale, z, z, z, sp)  # noqa: E731
    fwd = lambda loss, scale: lib.e2emv_ba_2view_loss(h, 1, 8, z, z, z, z, 3, z, z, loss, scale, None, sp)  # noqa: E731
    for loss, scale, text in ((3, 1.0, b"unknown loss code"), (-1, 1.0, b"unknown loss code"), (1, 0.0, b"loss scale"), (2, -1.0, b"loss scale"),
                              (1, float("nan"), b"loss scale"), (2, float("inf"), b"loss scale")):
        assert fwd(loss, scale) == _lib.EINVAL and text in lib.e2emv_last_error(h)
        assert bwd(loss, scale) == _lib.EINVAL and text in lib.e2emv_last_error(h) and b"ba_2view_loss_backward" in lib.e2emv_last_error(h)
    # the shape, NULL and tape rules of e2emv_ba_2view_backward
    assert bwd(2, 1.0, B=0) == _lib.ESHAPE and bwd(2, 1.0, N=0) == _lib.ESHAPE and bwd(2, 1.0, n=-1) == _lib.ESHAPE
    assert lib.e2emv_ba_2view_loss_backward(h, 1, 8, z, z, z, z, 3, 2, 1.0, None, z, z, sp) == _lib.EINVAL
    big = 2 ** 31 - 1
    assert bwd(1, 1.0, B=big, N=big, n=big) == _lib.ENOMEM and b"size_t" in lib.e2emv_last_error(h)
    s = scene("c_n65")
    gconf, gTi = device_backward(gpu, s["k0"], s["k1"], s["conf"], s["T_init"], 3, cotangent(), "cauchy", L.PIXEL)
    assert bool(gconf.isfinite().all()) and bool(gTi.isfinite().all()) and float(gconf.abs().max()) > 0


@pytest.mark.parametrize("loss", LOSSES)
def test_python_route_fills_both_gradients(gpu, loss):
    """``T.sum().backward()`` through ``run_bundle_adjust_2_view(..., loss_backward=True)``: the gradients are the C entry's bits for a
    cotangent of ones, with an invalid sample in the batch; the summary comes along; without a graph nothing changes."""
    import e2e_multi_view_matching_amd as E
    A, six, C = scene("c_n65"), S.make_scene(65, 305), S.make_scene(65, 306)
    six["conf"][0, 6:] = 0.0
    cat = lambda k: torch.cat([x[k] for x in (A, six, C)]).to(gpu)  # noqa: E731
    conf = cat("conf").unsqueeze(-1).clone().requires_grad_(True)
    Ti = cat("T_init").clone().requires_grad_(True)
    T, vb, summary = E.run_bundle_adjust_2_view(cat("k0"), cat("k1"), conf, Ti, n_iterations=3, loss=loss, loss_scale=L.PIXEL, loss_backward=True,
                                                return_summary=True)
    assert vb.tolist() == [True, False, True] and T.shape == (2, 4, 4) and T.grad_fn is not None
    assert summary.shape == (3, 4) and float(summary[0, 3]) > 0 and bool((summary[1] == 0).all())
    T.sum().backward()
    assert conf.grad is not None and conf.grad.shape == conf.shape and Ti.grad is not None and Ti.grad.shape == Ti.shape
    gT = torch.ones(3, 4, 4)
    gT[1] = 0.0  # the selection leaves the invalid sample out of the sum
    gc, gt = device_backward(gpu, cat("k0"), cat("k1"), cat("conf"), cat("T_init"), 3, gT, loss, L.PIXEL)
    assert torch.equal(conf.grad.cpu()[..., 0], gc) and torch.equal(Ti.grad.cpu(), gt)
    assert float(gc[0].abs().max()) > 0 and float(gc[2].abs().max()) > 0 and bool((gc[1] == 0).all()) and bool((gt[1] == 0).all())
    T0, vb0 = E.run_bundle_adjust_2_view(cat("k0"), cat("k1"), conf.detach(), Ti.detach(), n_iterations=3, loss=loss, loss_scale=L.PIXEL)
    assert T0.grad_fn is None and torch.equal(T0, T.detach()) and torch.equal(vb0, vb)


def test_pose_loss_tuple_with_a_loss_reaches_every_confidence_and_differs_from_the_squared_loss(gpu):
    """``pose_loss_tuple(..., ba_iterations=3, ba_loss="cauchy", ba_loss_scale=1/600)`` on a 3-tuple: every ``conf_scores_{i}_{j}`` gets a
    finite gradient that is not zero, and on at least one pair it differs from the ``ba_loss=None`` gradient by more than 100 x 1e-3
    max|g| - the refinement really ran with the loss, forward and backward."""
    import e2e_multi_view_matching_amd as E
    import test_gpu_pose_loss_tuple as G
    T, B, N = 3, 2, 65
    d, res = G.scene(T, B, N, 3)
    d = dict(d)
    for t in range(T):  # make_tuples' poses map world -> camera, the reference's data["pose"] camera -> world
        d[f"pose{t}"] = torch.linalg.inv(d[f"pose{t}"].double()).float()
    res = {k: v.clone() for k, v in res.items()}
    for i, j in G.pairs_of(T):  # what a matcher in training does: the first four matches of every sample point at each other's partners
        m = res[f"matches{i}_{i}_{j}"]
        for b in range(B):
            rows = torch.nonzero(m[b] >= 0)[:4, 0]
            m[b, rows] = m[b, rows.roll(1)]
    dg = G._dev(d, gpu)
    grads = {}
    for loss, scale in ((None, None), ("cauchy", 1.0 / 600.0)):
        rg = G._leaves(res, gpu)
        out = E.pose_loss_tuple(dg, rg, ba_iterations=3, ba_loss=loss, ba_loss_scale=scale)
        (out["rot_loss"] + out["transl_loss"]).backward()
        grads[loss] = {p: rg["conf_scores_%d_%d" % p].grad.cpu() for p in G.pairs_of(T)}
    apart = {}
    for p in G.pairs_of(T):
        g, g0 = grads["cauchy"][p], grads[None][p]
        assert g.shape == (B, N, 1) and bool(g.isfinite().all()) and float(g.abs().max()) > 0, p
        apart[p] = float((g - g0).abs().max()) / float(g0.abs().max())
        print(f"pair {p}: |g(cauchy) - g(squared)| = {apart[p]:.3e} max|g|")
    assert max(apart.values()) > 100.0 * GRADIENT_BAR, apart
