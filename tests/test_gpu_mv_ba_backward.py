"""Backward pass of the multi-view bundle adjustment on the device (csrc/mvba_backward.hip, e2emv_mv_bundle_adjust_batch_backward)
against autograd through the torch restatement of the same loop (tests/mvba_backward_restatement.py, itself pinned on the CPU by
tests/test_mv_ba_backward.py against the fp64 oracle, against ties and against central finite differences).

Cases (mvba_backward_restatement.CASES): the smallest shapes at which the kernel can go wrong - C = 2 with 8 points; C = 3, fixed_cam = 1,
180 points seen by all cameras (O = 540: thread 0 owns two observations, camera lists longer than a wave); 520 points (more points than
threads); C = 8 with tracks of 2..8 (28 blocks of the reduced system on 8 waves); a camera without observations; a far start with
rejected steps and a shrinking radius; exact data that stops on the gradient tolerance at once - each after max_iterations = 0, 1, 3
and 50, a random fixed-seed cotangent on the cameras, and on the points in the cases flagged so.

Bar: elementwise |g - g_ref| <= REL_BAR max|g_ref| for g_obs_w, g_cams0 and g_pts0, REL_BAR = ten times the largest distance measured on
the MI355X; it stays under GRADIENT_BAR = 1e-3, which every comparison also asserts.  No sign freedom enters: the start
points are inputs here (no DLT).  Device and restatement share the algorithm, fp64 and every decision (asserted: iterations and
termination agree); they differ in where they round, and the reduced system is badly conditioned along the free scale of a scene, so
the distance is far above eps.  Measured on the MI355X, largest over the three outputs, per case for max_iterations = 1 / 3 / 50
(0 is exact: the cotangents pass through):
    minimal          4.1e-11 (1 accepted)   1.0e-10 (3 accepted)   4.9e-11 (5 accepted)
    dense_fixed_mid  3.3e-12 (1 accepted)   4.3e-11 (3 accepted)   3.8e-11 (4 accepted)
    many_points      1.3e-10 (1 accepted)   3.9e-10 (3 accepted)   5.1e-10 (5 accepted)
    mixed_tracks     3.3e-11 (1 accepted)   8.7e-11 (3 accepted)   1.2e-10 (8 accepted)
    blind_camera     6.7e-11 (1 accepted)   1.6e-10 (3 accepted)   1.2e-10 (5 accepted)
    far_start        1.3e-11 (1 accepted)   3.8e-10 (3 accepted)   2.5e-09 (17 accepted)
    exact            0.0e+00 (0 accepted)   0.0e+00 (0 accepted)   0.0e+00 (0 accepted)
The largest is 2.5e-9 (far_start after 17 accepted steps, g_cams0).
The tuple route (d_gmconf, fp32) adds the rounding of its output format, 2^-24 of the value, to the bar; measured 2.9e-8 and 5.0e-8 of
max|g_ref| on the two tuples (3 accepted steps each, at max_iterations 3 and 50 alike)."""
import functools

import numpy as np
import pytest

import mvba_backward_restatement as R

pytestmark = pytest.mark.gpu

MEASURED = 2.5e-9  # largest distance measured on the MI355X (see the table above)
REL_BAR = 10 * MEASURED
GRADIENT_BAR = 1e-3


def args(prob):
    return (prob["n_cams"], prob["fixed"], prob["intr"], prob["cam_idx"], prob["pt_idx"], prob["obs"], prob["wts"], prob["cams"], prob["pts"])


@functools.lru_cache(maxsize=None)
def reference(name, K):
    """(problem, g_cams, g_pts, (g_obs_w, g_cams0, g_pts0), info) of the restatement: computed once, shared, left unchanged."""
    build, with_points = R.CASES[name]
    prob = build()
    gc, gp = R.cotangent(prob, K, with_points)
    gw, gc0, gp0, info = R.gradients(prob, K, gc, gp)
    return prob, gc, gp, (gw, gc0, gp0), info


def device(gpu, problems, grads, K):
    from e2e_multi_view_matching_amd import multi_view
    return multi_view.bundle_adjust_batch_backward(problems, grads, K)


def raw(gpu, prob, K, g_cams, g_pts, want=(True, True, True), n_problems=1, pt_off=None, obs_off=None, cam_idx=None):
    """The C entry itself on one problem: outputs not wanted are NULL.  Returns (rc, g_obs_w, g_cams0, g_pts0)."""
    from e2e_multi_view_matching_amd import _lib
    ctx = _lib.context(gpu)
    c = lambda x, dt: np.ascontiguousarray(x, dt)  # noqa: E731
    P, O = len(prob["pts"]), len(prob["cam_idx"])
    n_cams, fixed = c([prob["n_cams"]], np.int32), c([prob["fixed"]], np.int32)
    po, oo = c([0, P] if pt_off is None else pt_off, np.int64), c([0, O] if obs_off is None else obs_off, np.int64)
    ci, pi = c(prob["cam_idx"] if cam_idx is None else cam_idx, np.int32), c(prob["pt_idx"], np.int32)
    keep = [n_cams, fixed, po, oo, ci, pi] + [c(prob[k], np.float64) for k in ("intr", "obs", "wts", "cams", "pts")]
    gc, gp = (None if g_cams is None else c(g_cams, np.float64)), (None if g_pts is None else c(g_pts, np.float64))
    outs = [np.full((O, 2), np.nan), np.full((len(prob["cams"]), 6), np.nan), np.full((P, 3), np.nan)]
    p = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    rc = ctx.lib.e2emv_mv_bundle_adjust_batch_backward(ctx.h, n_problems, p(n_cams), p(fixed), p(keep[6]), p(po), p(oo), p(ci), p(pi), p(keep[7]), p(keep[8]),
                                                       p(keep[9]), p(keep[10]), K, p(gc), p(gp), *(p(o) if w else None for o, w in zip(outs, want)),
                                                       _lib.stream_ptr(gpu))
    return (rc,) + tuple(outs)


@pytest.mark.parametrize("K", R.ITERATIONS)
@pytest.mark.parametrize("name", list(R.CASES))
def test_device_against_the_restatement(gpu, name, K):
    from e2e_multi_view_matching_amd import multi_view
    prob, gc, gp, ref, info = reference(name, K)
    summary = multi_view.bundle_adjust_batch([args(prob)], K)[0][2]
    assert (summary["iterations"], summary["termination"]) == (info["iterations"], info["termination"])  # the same decisions
    got = device(gpu, [args(prob)], [(gc, gp)], K)[0]
    worst = []
    for g, r in zip(got, ref):
        assert g.shape == r.shape and np.isfinite(g).all()
        scale = np.abs(r).max()
        worst.append(np.abs(g - r).max() / scale if scale > 0 else float(np.abs(g).max()))
    accepted = sum(a for _, _, a in info["schedule"]["passes"])
    print(f"MEASURED {name} K={K} accepted={accepted}: g_obs_w {worst[0]:.2e} g_cams0 {worst[1]:.2e} g_pts0 {worst[2]:.2e}")
    assert REL_BAR < GRADIENT_BAR
    for g, r in zip(got, ref):
        assert (np.abs(g - r) <= GRADIENT_BAR * np.abs(r).max()).all()
        assert (np.abs(g - r) <= REL_BAR * np.abs(r).max()).all()
    if accepted == 0:  # the cotangents pass through bit for bit and the weights get exact zeros
        assert not got[0].any() and np.array_equal(got[1], gc) and np.array_equal(got[2], np.zeros_like(got[2]) if gp is None else gp)
    f = prob["fixed"]
    assert np.array_equal(got[1][f], gc[f])  # the fixed camera's row passes through
    if name == "blind_camera":
        assert np.array_equal(got[1][2], gc[2])  # and the row of the camera without observations


def test_null_arguments_zero_and_doubled_cotangents(gpu):
    prob, gc, gp, _, _ = reference("mixed_tracks", 3)
    rc, gw, gc0, gp0 = raw(gpu, prob, 3, gc, gp)
    assert rc == 0 and gw.any() and np.isfinite(gw).all() and np.isfinite(gc0).all() and np.isfinite(gp0).all()
    for want in [(True, False, False), (False, True, False), (False, False, True), (False, True, True), (False, False, False)]:
        rc, *outs = raw(gpu, prob, 3, gc, gp, want)
        assert rc == 0
        for o, full, w in zip(outs, (gw, gc0, gp0), want):
            assert np.array_equal(o, full) if w else np.isnan(o).all()  # a NULL output is not written, the others do not change
    # g_pts NULL means zeros
    a, b = raw(gpu, prob, 3, gc, None), raw(gpu, prob, 3, gc, np.zeros_like(gp))
    assert a[0] == 0 and all(np.array_equal(x, y) for x, y in zip(a[1:], b[1:])) and not np.array_equal(a[1], gw)
    # a zero cotangent gives exact zeros; doubling the cotangent doubles every output bit for bit
    z = raw(gpu, prob, 3, np.zeros_like(gc), None)
    assert z[0] == 0 and not any(o.any() for o in z[1:])
    d = raw(gpu, prob, 3, 2.0 * gc, 2.0 * gp)
    assert d[0] == 0 and np.array_equal(d[1], 2.0 * gw) and np.array_equal(d[2], 2.0 * gc0) and np.array_equal(d[3], 2.0 * gp0)


def test_batch_position_independence_and_repeatability(gpu):
    """A problem alone, first, last and between problems of other sizes gives the same words; so do two runs."""
    names = ["dense_fixed_mid", "minimal", "blind_camera", "many_points"]
    items = {n: reference(n, 3) for n in names}
    one = lambda n: (args(items[n][0]), (items[n][1], items[n][2]))  # noqa: E731
    alone = device(gpu, [one("blind_camera")[0]], [one("blind_camera")[1]], 3)[0]
    for order in (["blind_camera", "minimal", "many_points"], ["many_points", "dense_fixed_mid", "blind_camera"], ["minimal", "blind_camera", "dense_fixed_mid"],
                  ["minimal", "blind_camera", "dense_fixed_mid"]):
        out = device(gpu, [one(n)[0] for n in order], [one(n)[1] for n in order], 3)
        for got, want in zip(out[order.index("blind_camera")], alone):
            assert np.array_equal(got, want)
    again = device(gpu, [one("blind_camera")[0]], [one("blind_camera")[1]], 3)[0]
    assert all(np.array_equal(x, y) for x, y in zip(again, alone))


def test_shape_errors_and_a_tape_that_cannot_be_reserved(gpu):
    """The shape rules are those of the forward entry (same codes); a tape larger than the device's memory is E2EMV_ENOMEM from the
    host-side check against the device's total memory - nothing is freed, reserved, launched or read -, and the context goes on
    working.  NOT exercised here: a tape below that total which ws_reserve still cannot allocate (it frees the arena, fails, and leaves
    the context with an empty one that the next call regrows) - reaching it means filling the device's memory."""
    from e2e_multi_view_matching_amd import _lib
    prob, gc, gp, _, _ = reference("many_points", 3)
    P, O = len(prob["pts"]), len(prob["cam_idx"])
    ctx = _lib.context(gpu)
    assert raw(gpu, prob, 3, gc, None, n_problems=0)[0] == _lib.EINVAL
    assert raw(gpu, prob, 3, gc, None, pt_off=[1, P])[0] == _lib.ESHAPE
    assert raw(gpu, prob, 3, gc, None, obs_off=[0, -1])[0] == _lib.ESHAPE
    bad = np.array(prob["cam_idx"]); bad[5] = prob["n_cams"]
    assert raw(gpu, prob, 3, gc, None, cam_idx=bad)[0] == _lib.EINVAL and b"refers to camera" in ctx.lib.e2emv_last_error(ctx.h)
    assert raw(gpu, prob, 3, None, None)[0] == _lib.EINVAL
    rc = raw(gpu, prob, 2 ** 31 - 1, gc, None)[0]
    assert rc == _lib.ENOMEM and b"tape" in ctx.lib.e2emv_last_error(ctx.h)
    rc, gw, gc0, gp0 = raw(gpu, prob, 3, gc, None)
    assert rc == 0 and np.isfinite(gw).all() and gw.any() and np.isfinite(gc0).all() and np.isfinite(gp0).all()
    assert O > 512 and P > 512


def test_python_route_fills_the_gradients(gpu):
    import torch
    from e2e_multi_view_matching_amd import multi_view
    prob = R.CASES["mixed_tracks"][0]()
    a = args(prob)
    w, c, p = (torch.tensor(np.asarray(prob[k], np.float64), requires_grad=True) for k in ("wts", "cams", "pts"))
    co, po = multi_view.bundle_adjust_torch(*a[:6], w, c, p, max_iterations=3)
    assert co.dtype == torch.float64 and co.requires_grad and po.requires_grad
    co.sum().backward()
    want = device(gpu, [a], [(np.ones_like(prob["cams"]), None)], 3)[0]
    for t, g in zip((w, c, p), want):
        assert t.grad is not None and t.grad.shape == t.shape and np.array_equal(t.grad.numpy(), g) and bool(t.grad.isfinite().all())
    assert float(w.grad.abs().max()) > 0
    # only the tensors that require grad get one
    w2 = torch.tensor(np.asarray(prob["wts"], np.float64), requires_grad=True)
    multi_view.bundle_adjust_torch(*a[:6], w2, prob["cams"], prob["pts"], max_iterations=3)[0].sum().backward()
    assert np.array_equal(w2.grad.numpy(), want[0])
    # without a graph: what bundle_adjust returns, bit for bit
    plain = multi_view.bundle_adjust(*a, max_iterations=3)
    co2, po2 = multi_view.bundle_adjust_torch(*a, max_iterations=3)
    assert np.array_equal(co2.numpy(), plain[0]) and np.array_equal(po2.numpy(), plain[1]) and not co2.requires_grad
    assert np.array_equal(co.detach().numpy(), plain[0]) and np.array_equal(po.detach().numpy(), plain[1])


# ---- the tuple route: collect -> weights -> solver -> extrinsics ----------------------------------------------------------------------
T3, THRESH = 3, 0.6   # B = 2 tuples of 3 images, N = 40 keypoints; confidences are U(0.5, 1), so the threshold cuts about a fifth
EPS32 = 2.0 ** -24    # d_gmconf is fp32: half an ulp of the value on top of the bar


@functools.lru_cache(maxsize=None)
def tuple_inputs():
    """Two planted 3-tuples (tests/test_gpu_mv_tracks.planted_scene) as one batch; pair (0, 2) has no matches entry."""
    import torch
    from test_gpu_mv_tracks import planted_scene
    parts = [planted_scene(s, T=T3, n_kpts=40) for s in (41, 42)]
    data = {k: (torch.cat([p[0][k] for p in parts], 0) if torch.is_tensor(v) else v) for k, v in parts[0][0].items()}
    result = {k: torch.cat([p[1][k] for p in parts], 0) for k in parts[0][1]}
    del result["matches0_0_2"], result["conf_scores_0_2"]
    return data, result, np.stack([p[3] for p in parts]), np.stack([p[2] for p in parts])


def _kept(result, i, j, n1):
    m, c = result[f"matches{i}_{i}_{j}"].cpu().numpy(), result[f"conf_scores_{i}_{j}"].detach().cpu().numpy()
    return (m >= 0) & (m < n1) & (c.reshape(c.shape[0], c.shape[1], -1) > np.float32(THRESH)).all(-1)


def test_tuple_route_against_the_restatement(gpu):
    """e2emv_mv_tuple_ba_backward against autograd through weights -> solver (the restatement) -> extrinsics on the problems the device
    built, same bar (plus the fp32 rounding of its output); then e2emv_mv_collect_backward: an exact scatter by the keep rule."""
    import torch
    from e2e_multi_view_matching_amd import _lib, multi_view
    data, result, start, _ = tuple_inputs()
    res = {k: v.to(gpu) for k, v in result.items()}
    inp = multi_view._collect_inputs(T3, data, res)
    collected = multi_view._collect_call(T3, inp, THRESH)
    counts = collected[3].cpu().numpy()
    by_pair = counts.reshape(2, 3)  # pairs (0, 1), (0, 2), (1, 2)
    kept = {(i, j): _kept(result, i, j, 40) for i, j in ((0, 1), (1, 2))}
    matched = {k: (result[f"matches{k[0]}_{k[0]}_{k[1]}"].numpy() >= 0) for k in kept}
    assert (by_pair[:, 1] == 0).all() and (by_pair[:, [0, 2]] >= 8).all()
    assert all((kept[k].sum(1) < matched[k].sum(1)).all() for k in kept)  # the threshold cuts rows
    assert np.array_equal(by_pair[:, 0], kept[(0, 1)].sum(1)) and np.array_equal(by_pair[:, 2], kept[(1, 2)].sum(1))
    intr, kdim, nb = multi_view._tuple_intrinsics(T3, data, gpu, 2)
    problems = multi_view._tuple_problems(T3, collected, counts, intr, kdim, nb, start)
    conf = collected[2].cpu().numpy().astype(np.float64)
    g_extr = np.random.default_rng(5).normal(size=(2, T3, 4, 4))
    p = lambda a: a.ctypes.data  # noqa: E731
    for K in (3, 50):
        gm = torch.full_like(collected[2], float("nan"))
        out, summary = np.zeros_like(start), np.zeros((2, 4))
        multi_view._tuple_ba_call("e2emv_mv_tuple_ba", T3, collected, counts, intr, kdim, nb, start, K, p(out), p(summary))
        multi_view._tuple_ba_call("e2emv_mv_tuple_ba_backward", T3, collected, counts, intr, kdim, nb, start, K, p(g_extr), _lib.ptr(gm))
        gm_h = gm.cpu().numpy().astype(np.float64)
        for b in range(2):
            pr = problems[b]
            prob = dict(n_cams=T3, fixed=0, intr=pr[2], cam_idx=pr[3], pt_idx=pr[4], obs=pr[5], wts=pr[6], cams=pr[7], pts=pr[8])
            c = torch.tensor(conf[3 * b:3 * b + 3], requires_grad=True)
            cnt = by_pair[b]
            H = 0.5 * (2.0 * sum(c[q, :cnt[q]].sum() for q in range(3)) + 1e-3)
            w_obs = torch.cat([torch.cat([c[q, :cnt[q]], c[q, :cnt[q]]]) for q in range(3)]) / H
            wts = torch.stack([w_obs, w_obs], 1)
            assert np.allclose(wts.detach().numpy(), prob["wts"], rtol=1e-12, atol=0)  # the weights the device built
            co, _, info = R.run(prob, torch.tensor(prob["cams"]), torch.tensor(prob["pts"]), wts, K)
            assert int(summary[b, 2]) == info["iterations"] and R.TERMS[int(summary[b, 3])] == info["termination"]
            Rm = R.transform(co, torch.zeros(T3, 3, dtype=torch.float64))[1]
            E = torch.cat([Rm, co[:, 3:, None]], 2)
            assert np.abs(E.detach().numpy() - out[b, :, :3]).max() < 1e-8
            ref = torch.autograd.grad((E * torch.as_tensor(g_extr[b, :, :3])).sum(), c)[0].numpy()
            got = gm_h[3 * b:3 * b + 3]
            worst = np.abs(got - ref).max() / np.abs(ref).max()
            print(f"MEASURED tuple {b} K={K}: d_gmconf {worst:.2e} (accepted {sum(a for _, _, a in info['schedule']['passes'])})")
            assert (np.abs(got - ref) <= GRADIENT_BAR * np.abs(ref).max()).all()
            assert (np.abs(got - ref) <= REL_BAR * np.abs(ref).max() + EPS32 * np.abs(ref)).all()
            for q in range(3):
                assert not got[q, cnt[q]:].any() and (cnt[q] == 0 or got[q, :cnt[q]].all())  # rows behind the count are exactly 0
    # the scatter: slot k of a pair block goes to channel 0 of its k-th kept row, everything else is exactly 0; a NULL entry is left out
    # (two confidence channels, the second above the first: the same rows are kept)
    cs = [None if c is None else torch.cat([c, c + 0.25], 2).contiguous() for c in inp["cs"]]
    gouts = [None if c is None else torch.full_like(c, float("nan")) for c in cs]
    ctx = _lib.context(gpu)
    for only in ([True, False, False], [False, False, True]):  # a NULL entry leaves that pair out: one pair per call
        ptrs = [_lib.ptr_array(lst) for lst in (inp["ms"], cs, [g if o else None for g, o in zip(gouts, only)])]
        ctx.call("e2emv_mv_collect_backward", 2, T3, 40, p(inp["n1"]), ptrs[0][0], ptrs[1][0], 2, float(THRESH), _lib.ptr(gm), ptrs[2][0],
                 _lib.stream_ptr(gpu))
        torch.cuda.synchronize()
        assert all(bool(g.isnan().all()) == (not done) for g, done in zip([gouts[0], gouts[2]], [True, only[2]]))
    gm_f = gm.cpu().numpy()
    for q, key in ((0, (0, 1)), (2, (1, 2))):
        go = gouts[q].cpu().numpy()
        want = np.zeros_like(go)
        for b in range(2):
            rows = np.flatnonzero(kept[key][b])
            want[b, rows, 0] = gm_f[3 * b + q, :len(rows)]
        assert np.array_equal(go, want) and np.abs(want).max() > 0 and not go[:, :, 1].any()
    assert gouts[1] is None


def test_refine_tuple_poses_batch_fills_every_confidence_gradient(gpu):
    """The Python route: a rotation-angle loss on the refined poses reaches every conf_scores_{i}_{j} - finite, non-zero on the kept rows
    only - and without a graph the same extrinsics come back as a constant."""
    import torch
    from e2e_multi_view_matching_amd import multi_view
    data, result, start, gt = tuple_inputs()
    res = {k: v.to(gpu) for k, v in result.items()}
    confs = {k: v.clone().requires_grad_() for k, v in res.items() if k.startswith("conf_scores_")}
    res.update(confs)
    E = multi_view.refine_tuple_poses_batch(T3, data, res, start, THRESH)
    assert E.shape == (2, T3, 4, 4) and E.dtype == torch.float64 and E.requires_grad
    G = torch.as_tensor(gt)
    loss = 0.0
    for i, j in ((0, 1), (0, 2), (1, 2)):  # tuple_pose_errors' rotation angle of every image pair
        rel_gt = G[:, j, :3, :3] @ G[:, i, :3, :3].transpose(1, 2)
        rel = E[:, j, :3, :3] @ E[:, i, :3, :3].transpose(1, 2)
        cos = ((rel_gt * rel).sum((1, 2)) - 1.0) / 2.0
        loss = loss + torch.acos(cos.clamp(-1.0, 1.0)).sum()
    loss.backward()
    assert sorted(confs) == ["conf_scores_0_1", "conf_scores_1_2"]
    for (i, j) in ((0, 1), (1, 2)):
        g = confs[f"conf_scores_{i}_{j}"].grad
        assert g is not None and g.shape == confs[f"conf_scores_{i}_{j}"].shape and bool(g.isfinite().all())
        g, keep = g.cpu().numpy().reshape(2, 40, -1), _kept(result, i, j, 40)
        assert (g[keep][:, 0] != 0).all() and not g[~keep].any() and not g[:, :, 1:].any()
    plain = multi_view.refine_tuple_poses_batch(T3, data, {k: v.detach() for k, v in res.items()}, start, THRESH)
    assert not plain.requires_grad and np.array_equal(plain.numpy(), E.detach().numpy())
    with pytest.raises(ValueError, match="max_iterations"):
        multi_view.refine_tuple_poses_batch(T3, data, res, start, THRESH, max_iterations=-1)
    with pytest.raises(ValueError, match="extrinsics"):
        multi_view.refine_tuple_poses_batch(T3, data, res, start[:, :2], THRESH)
