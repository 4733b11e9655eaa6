"""The tuple pose loss on the device (-m gpu): ``e2emv_w8pt_tuple_backward``, ``e2emv_pose_loss_tuple``, ``e2emv_pose_loss_tuple_backward``
and the Python front on top (``run_weighted_8_point_tuple`` with a graph, ``pose_loss_tuple``).

Scenes come from ``synthetic.make_tuples`` (default rho = 0.7: 30 % of the rows of every pair carry match -1) with random confidences.
Shapes (T, B, N): (2, 1, 8) the smallest N the solve takes; (3, 2, 65) pair order (0,1), (0,2), (1,2) and a row in the second wave;
(5, 2, 257) the second 256-block of the gather grid at the reference's tuple size; (8, 1, 16) ``E2EMV_MAX_TUPLE``, 28 pairs.

"Bit for bit" below is ``torch.equal`` on the int32 view of the fp32 values: at N = 8 a pair has at most 7 weighted rows, the 8-point problem is
rank-deficient and its gradient is whatever the eigen-solver's null space gives - the same bits on both paths, NaN or not."""
import ctypes
import functools

import pytest
import torch

SHAPES = [(2, 1, 8), (3, 2, 65), (5, 2, 257), (8, 1, 16)]
ORACLE_SHAPES = {(3, 2, 65): 3, (5, 2, 257): 5}  # shape -> seed (tests/test_pose_loss_tuple.py checks their conditioning on the CPU)
REL = 1e-3  # the project's gradient bar


def pairs_of(T):
    return [(i, j) for j in range(T) for i in range(j)]


@functools.lru_cache(maxsize=None)
def scene(T, B, N, seed, camera=False):
    """(data, result) on the CPU.  ``camera``: keypoints in camera coordinates made once in fp32, identity intrinsics from there on."""
    from e2e_multi_view_matching_amd.synthetic import make_tuples
    d = make_tuples(batch=B, tuple_size=T, n_kpts=N, seed=seed)
    g = torch.Generator().manual_seed(1000 + seed)
    res = {}
    for i, j in pairs_of(T):
        res[f"matches{i}_{i}_{j}"] = d[f"gt_matches{i}_{i}_{j}"]
        res[f"conf_scores_{i}_{j}"] = torch.rand(B, N, 1, generator=g) * 0.8 + 0.2
        assert bool((res[f"matches{i}_{i}_{j}"] < 0).any(dim=1).all()) and bool((res[f"matches{i}_{i}_{j}"] >= 0).any(dim=1).all())
    if camera:
        for t in range(T):
            K = d[f"intr{t}"]
            d[f"pixels{t}"] = d[f"keypoints{t}"]
            d[f"keypoints{t}"] = (d[f"keypoints{t}"] - K[:, None, :2, 2]) / torch.stack([K[:, 0, 0], K[:, 1, 1]], -1)[:, None]
            d[f"pixel_intr{t}"] = K
            d[f"intr{t}"] = torch.eye(4).unsqueeze(0).repeat(B, 1, 1)
    return d, res


def weights(T, B, seed):
    """The fixed random weights of the functional, one [B,3,4] per pair."""
    g = torch.Generator().manual_seed(2000 + seed)
    return {p: torch.randn(B, 3, 4, generator=g) for p in pairs_of(T)}


def functional(Tm, Wr):
    """The random linear + quadratic functional of the 3 x 4 pose of tests/test_gpu_backward.py::test_w8pt_pose_gradient_wrt_confidence."""
    Td, W = Tm.double(), Wr.to(Tm.device).double()
    return (Td[:, :3, :] * W).sum() + ((Td[:, :3, :] - 0.3) ** 2 * W.flip(1)).sum()


@functools.lru_cache(maxsize=None)
def oracle_gradients(T, B, N, seed, rounded=True):
    """{pair: dLoss/dconf_scores [B,N] fp64} by torch.autograd through oracle/w8pt.py in fp64.  ``rounded``: from the fp32 camera
    coordinates the device gets; else from camera coordinates formed in fp64 (the conditioning check of the host test)."""
    from oracle import w8pt as OW
    d, res = scene(T, B, N, seed, camera=True)
    Wr = weights(T, B, seed)
    data = {}
    for t in range(T):
        if rounded:
            data[f"keypoints{t}"] = d[f"keypoints{t}"].double()
        else:
            K = d[f"pixel_intr{t}"].double()
            data[f"keypoints{t}"] = (d[f"pixels{t}"].double() - K[:, None, :2, 2]) / torch.stack([K[:, 0, 0], K[:, 1, 1]], -1)[:, None]
        data[f"intr{t}"] = d[f"intr{t}"].double()
    out = {}
    for i, j in pairs_of(T):
        c = res[f"conf_scores_{i}_{j}"].double().clone().requires_grad_(True)
        r = {f"matches{i}_{i}_{j}": res[f"matches{i}_{i}_{j}"], f"conf_scores_{i}_{j}": c}
        Tm, _ = OW.run_weighted_8_point(data, r, i, j, choose_closest=True, target_T_021=d[f"T_{i}to{j}"].double())
        functional(Tm, Wr[(i, j)]).backward()
        out[(i, j)] = c.grad.reshape(B, N)
    return out


def _dev(d, gpu):
    return {k: (v.to(gpu) if torch.is_tensor(v) else v) for k, v in d.items()}


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype == torch.float32 and torch.equal(bits(a), bits(b))


def _leaves(res, gpu, no_grad=()):
    out = {}
    for k, v in res.items():
        v = v.to(gpu)
        if k.startswith("conf_scores") and k not in no_grad:
            v = v.clone().requires_grad_(True)
        out[k] = v
    return out


def _tuple_gradients(dg, res, gpu, T, Wr, closest, no_grad=()):
    import e2e_multi_view_matching_amd as E
    rg = _leaves(res, gpu, no_grad)
    pairs = pairs_of(T)
    targets = {(i, j): dg[f"T_{i}to{j}"] for i, j in pairs} if closest else None
    out = E.run_weighted_8_point_tuple(dg, rg, choose_closest=closest, targets=targets)
    assert all(out[p][0].requires_grad for p in pairs), "the tuple poses carry no graph"
    assert all(not out[p][1]["confidence"].requires_grad for p in pairs)
    sum(functional(out[p][0], Wr[p]) for p in pairs).backward()
    return {p: rg["conf_scores_%d_%d" % p].grad for p in pairs}, {p: out[p][0].detach() for p in pairs}


def _pair_gradients(dg, res, gpu, T, Wr, closest):
    import e2e_multi_view_matching_amd as E
    rg = _leaves(res, gpu)
    grads, poses = {}, {}
    for i, j in pairs_of(T):
        Tp, _ = E.run_weighted_8_point(dg, rg, i, j, choose_closest=closest, target_T_021=dg[f"T_{i}to{j}"] if closest else None)
        functional(Tp, Wr[(i, j)]).backward()
        grads[(i, j)], poses[(i, j)] = rg[f"conf_scores_{i}_{j}"].grad, Tp.detach()
    return grads, poses


# ------------------------------------------------------------------------------------------------ 1. bit-identity with the pair loop


@pytest.mark.gpu
@pytest.mark.parametrize("closest", [True, False])
@pytest.mark.parametrize("T,B,N", SHAPES)
def test_tuple_gradient_is_the_pair_loops_bit_for_bit(gpu, T, B, N, closest):
    """conf_scores.grad through run_weighted_8_point_tuple against run_weighted_8_point per pair: the same kernel, one workgroup per
    sample, fixed-order reductions.  Rows with match -1 get exactly 0; a pair that does not require grad gets None and leaves the others
    unchanged."""
    d, res = scene(T, B, N, 7)
    dg, Wr = _dev(d, gpu), weights(T, B, 7)
    gt, Tt = _tuple_gradients(dg, res, gpu, T, Wr, closest)
    gp, Tp = _pair_gradients(dg, res, gpu, T, Wr, closest)
    for p in pairs_of(T):
        assert same_bits(Tt[p], Tp[p]), p
        assert gt[p] is not None and gt[p].shape == (B, N, 1) and same_bits(gt[p], gp[p]), p
        off = res["matches%d_%d_%d" % (p[0], p[0], p[1])] < 0
        assert bool(off.any()) and bool((bits(gt[p].cpu().reshape(B, N)[off]) == 0).all()), p
        if N > 8:
            assert bool(gt[p].isfinite().all()) and float(gt[p].abs().max()) > 0, p
    if T > 2:
        skip = "conf_scores_0_2"
        g2, _ = _tuple_gradients(dg, res, gpu, T, Wr, closest, no_grad=(skip,))
        assert g2[(0, 2)] is None
        assert all(same_bits(g2[p], gt[p]) for p in pairs_of(T) if p != (0, 2))


def _forward_buffers(dg, res, gpu, T, closest=True):
    from e2e_multi_view_matching_amd import pose
    pairs = pairs_of(T)
    rg = {k: v.to(gpu) for k, v in res.items()}
    tg = [dg[f"T_{i}to{j}"].contiguous() for i, j in pairs] if closest else [None] * len(pairs)
    st = pose._tuple_state(dg, rg, T, pairs, gpu, tg, closest, False)
    conf = [rg[f"conf_scores_{i}_{j}"].reshape(st["B"], -1).contiguous() for i, j in pairs]
    pose._w8pt_tuple_call(st, conf)
    return st, conf


def _c_tuple_backward(st, conf, gT, gcf=None, leave_out=()):
    from e2e_multi_view_matching_amd import _lib
    B, T, N, P = st["B"], st["T"], st["N"], st["P"]
    gconf = [None if q in leave_out else torch.full((B, N), float("nan"), device=gT.device) for q in range(P)]
    pm, k1 = _lib.ptr_array(st["matches"])
    pc, k2 = _lib.ptr_array(conf)
    pg, k3 = _lib.ptr_array(gconf)
    o = st["out"]
    st["ctx"].call("e2emv_w8pt_tuple_backward", B, T, N, pm, pc, _lib.ptr(o["k0n"]), _lib.ptr(o["k1n"]), _lib.ptr(o["T"]), _lib.ptr(gT), _lib.ptr(gcf), pg,
                   _lib.stream_ptr(gT.device))
    return gconf


@pytest.mark.gpu
@pytest.mark.parametrize("T,B,N", SHAPES)
def test_c_entry_is_gather_backward_mask_per_pair(gpu, T, B, N):
    """e2emv_w8pt_tuple_backward against e2emv_gather_matched -> e2emv_w8pt_backward -> e2emv_apply_mask per pair, outputs pre-filled with NaN;
    a d_gcf of ones adds exactly the mask; a NULL d_gconf[q] leaves that pair out and the others unchanged."""
    from e2e_multi_view_matching_amd import _lib
    d, res = scene(T, B, N, 7)
    dg = _dev(d, gpu)
    st, conf = _forward_buffers(dg, res, gpu, T)
    ctx, P, o, s = st["ctx"], st["P"], st["out"], _lib.stream_ptr(gpu)
    gT = torch.zeros(P * B, 4, 4)
    gT[:, :3] = torch.randn(P * B, 3, 4, generator=torch.Generator().manual_seed(3))
    gT = gT.to(gpu)
    got = _c_tuple_backward(st, conf, gT)
    ones = _c_tuple_backward(st, conf, gT, gcf=torch.ones(P * B, N, device=gpu))
    for q, (i, j) in enumerate(pairs_of(T)):
        m = st["matches"][q]
        k1g, cout = torch.empty(B, N, 2, device=gpu), torch.full((B, N), float("nan"), device=gpu)
        ctx.call("e2emv_gather_matched", B, N, N, _lib.ptr(st["kpts"][j]), _lib.ptr(m), _lib.ptr(conf[q]), _lib.ptr(k1g), _lib.ptr(cout), s)
        g = torch.full((B, N), float("nan"), device=gpu)
        ctx.call("e2emv_w8pt_backward", B, N, _lib.ptr(o["k0n"][q]), _lib.ptr(o["k1n"][q]), _lib.ptr(cout), _lib.ptr(o["T"][q]), _lib.ptr(gT[q * B:(q + 1) * B]),
                 _lib.ptr(g), s)
        mask = (m >= 0).to(torch.uint8)
        want = torch.full((B, N), float("nan"), device=gpu)
        ctx.call("e2emv_apply_mask", B * N, _lib.ptr(g), _lib.ptr(mask), _lib.ptr(want), s)
        assert same_bits(got[q], want), (i, j)
        assert bool((bits(got[q])[m < 0] == 0).all()) and bool((m < 0).any()), (i, j)
        assert same_bits(ones[q], torch.where(m >= 0, g + 1.0, torch.zeros_like(g))), (i, j)
    if P > 1:
        part = _c_tuple_backward(st, conf, gT, leave_out=(1,))
        assert part[1] is None and all(same_bits(part[q], got[q]) for q in range(P) if q != 1)


# ------------------------------------------------------------------------------------------------ 2. against autograd through the oracle


@pytest.mark.gpu
@pytest.mark.parametrize("T,B,N", list(ORACLE_SHAPES))
def test_tuple_gradient_against_autograd_through_the_oracle(gpu, T, B, N):
    """Per (pair, sample): |g - g_ref| / |g_ref| < 1e-3 against torch.autograd through oracle/w8pt.py in fp64, both sides from the same fp32
    camera coordinates with identity intrinsics, choose_closest as in the training loop; no element is skipped.
    Measured on the MI355X: largest value 1.33e-07 at (3, 2, 65) (pair (0, 2), sample 1), 1.32e-07 at (5, 2, 257) (pair (0, 2), sample 0)."""
    seed = ORACLE_SHAPES[(T, B, N)]
    d, res = scene(T, B, N, seed, camera=True)
    want = oracle_gradients(T, B, N, seed)
    got, _ = _tuple_gradients(_dev(d, gpu), res, gpu, T, weights(T, B, seed), True)
    worst = 0.0
    for p in pairs_of(T):
        g = got[p].cpu().double().reshape(B, N)
        assert bool(g.isfinite().all()), p
        for b in range(B):
            rel = float((g[b] - want[p][b]).norm() / want[p][b].norm())
            worst = max(worst, rel)
            print(f"(T, B, N) = {(T, B, N)} pair {p} sample {b}: |g - g_ref| / |g_ref| = {rel:.3e}")
            assert rel < REL, (p, b, rel)
    print(f"(T, B, N) = {(T, B, N)}: largest relative gradient error {worst:.3e}")


# ------------------------------------------------------------------------------------------------ 3. the loss reductions


def _random_poses(n, seed, scale=0.4):
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(n, 3, generator=g) * scale
    Kx = torch.zeros(n, 3, 3)
    Kx[:, 0, 1], Kx[:, 0, 2], Kx[:, 1, 0], Kx[:, 1, 2], Kx[:, 2, 0], Kx[:, 2, 1] = -w[:, 2], w[:, 1], w[:, 2], -w[:, 0], -w[:, 1], w[:, 0]
    Tm = torch.eye(4).repeat(n, 1, 1)
    Tm[:, :3, :3] = torch.matrix_exp(Kx)
    Tm[:, :3, 3] = torch.randn(n, 3, generator=g)
    return Tm


def _loss_case(gpu, P, B):
    Ta, Tb = _random_poses(P * B, 11 + B), _random_poses(P * B, 12 + B)
    Tb[B + 1, :3, 3] = 0.0       # one invalid entry in pair 1
    Ta[B - 1, :3, 3] = 0.0       # and one in pair 0, on the predicted side
    return Ta.to(gpu), Tb.to(gpu)


def _c_pose_loss(ctx, gpu, P, B, Ta, Tb):
    from e2e_multi_view_matching_amd import _lib
    rot, tr = torch.full((P * B,), float("nan"), device=gpu), torch.full((P * B,), float("nan"), device=gpu)
    valid, l2 = torch.full((P * B,), 7, dtype=torch.uint8, device=gpu), torch.full((2,), float("nan"), device=gpu)
    ctx.call("e2emv_pose_loss_tuple", P, B, _lib.ptr(Ta), _lib.ptr(Tb), _lib.ptr(rot), _lib.ptr(tr), _lib.ptr(valid), _lib.ptr(l2), _lib.stream_ptr(gpu))
    return rot, tr, valid, l2


@pytest.mark.gpu
@pytest.mark.parametrize("P,B", [(3, 5), (2, 70), (28, 1)])
def test_pose_loss_tuple_is_the_ascending_sum_of_the_per_pair_means(gpu, P, B):
    """d_losses2 against the fp32 sum, in ascending q, of what e2emv_pose_error_means gives per pair - bit for bit; the per-element outputs
    too.  B = 70: more entries than the wave has lanes."""
    from e2e_multi_view_matching_amd import _lib
    ctx, s = _lib.context(gpu), _lib.stream_ptr(gpu)
    Ta, Tb = _loss_case(gpu, P, B) if B > 1 else (_random_poses(P, 5).to(gpu), _random_poses(P, 6).to(gpu))
    rot, tr, valid, l2 = _c_pose_loss(ctx, gpu, P, B, Ta, Tb)
    want = None
    for q in range(P):
        r, t, v, m2 = (torch.empty(B, device=gpu), torch.empty(B, device=gpu), torch.empty(B, dtype=torch.uint8, device=gpu), torch.empty(2, device=gpu))
        ctx.call("e2emv_pose_error_means", B, _lib.ptr(Ta[q * B:(q + 1) * B]), _lib.ptr(Tb[q * B:(q + 1) * B]), _lib.ptr(r), _lib.ptr(t), _lib.ptr(v), _lib.ptr(m2), s)
        assert same_bits(rot[q * B:(q + 1) * B], r) and same_bits(tr[q * B:(q + 1) * B], t) and torch.equal(valid[q * B:(q + 1) * B], v)
        want = m2.clone() if want is None else want + m2
    assert bool(want.isfinite().all()) and same_bits(l2, want), (l2, want)
    if B > 1:
        assert int(valid.sum()) == P * B - 2


@pytest.mark.gpu
def test_a_pair_without_a_valid_translation_makes_transl_loss_nan(gpu):
    from e2e_multi_view_matching_amd import _lib
    P, B = 3, 4
    Ta, Tb = _random_poses(P * B, 1).to(gpu), _random_poses(P * B, 2).to(gpu)
    Tb[B:2 * B, :3, 3] = 0.0
    _, _, valid, l2 = _c_pose_loss(_lib.context(gpu), gpu, P, B, Ta, Tb)
    assert valid.tolist() == [1] * B + [0] * B + [1] * B
    assert bool(l2[0].isfinite()) and float(l2[0]) > 0 and bool(l2[1].isnan())


@pytest.mark.gpu
@pytest.mark.parametrize("P,B", [(3, 5), (2, 70)])
def test_pose_loss_tuple_backward_is_pose_errors_backward_on_the_shares(gpu, P, B):
    """torch.equal to e2emv_pose_errors_backward fed g2[0] / B and g2[1] / n_valid_q formed in fp32; an invalid entry gets a zero translation
    share (column 3 of its gradient is exactly 0)."""
    from e2e_multi_view_matching_amd import _lib
    ctx, s = _lib.context(gpu), _lib.stream_ptr(gpu)
    Ta, Tb = _loss_case(gpu, P, B)
    _, _, valid, _ = _c_pose_loss(ctx, gpu, P, B, Ta, Tb)
    g2 = torch.tensor([1.7, -0.6], device=gpu)
    got = torch.full((P * B, 4, 4), float("nan"), device=gpu)
    ctx.call("e2emv_pose_loss_tuple_backward", P, B, _lib.ptr(Ta), _lib.ptr(Tb), _lib.ptr(g2), _lib.ptr(got), s)
    v = valid.bool().reshape(P, B)
    n_valid = v.sum(1, keepdim=True).to(torch.float32)
    g_rot = (g2[0] / torch.tensor(float(B), device=gpu)).expand(P * B).contiguous()
    g_tr = torch.where(v, (g2[1] / n_valid).expand(P, B), torch.zeros(P, B, device=gpu)).reshape(-1).contiguous()
    want = torch.full((P * B, 4, 4), float("nan"), device=gpu)
    ctx.call("e2emv_pose_errors_backward", P * B, _lib.ptr(Ta), _lib.ptr(Tb), _lib.ptr(g_rot), _lib.ptr(g_tr), _lib.ptr(want), s)
    assert torch.equal(got, want) and bool(got.isfinite().all())
    assert int((~v).sum()) == 2 and float(got[~v.reshape(-1)][:, :3, 3].abs().max()) == 0.0
    assert float(got[v.reshape(-1)][:, :3, 3].abs().sum(1).min()) > 0


# ------------------------------------------------------------------------------------------------ 4. pose_loss_tuple end to end


def _pair_loop(dg, res, gpu, T, ba, order):
    """The pose term of helpers.run_matcher with the existing differentiable per-pair functions, the pairs taken in ``order``."""
    import e2e_multi_view_matching_amd as E
    rg = _leaves(res, gpu)
    rot_loss, transl_loss, poses = 0.0, 0.0, {}
    for i, j in order:
        tgt = E.relative_pose(dg[f"pose{i}"], dg[f"pose{j}"])
        if ba == 0:
            Tp, info = E.run_weighted_8_point(dg, rg, i, j, choose_closest=True, target_T_021=tgt)
        else:
            k0, k1, K0, K1, conf = E.get_kpts(dg, rg, i, j)
            Tw, info = E.estimate_relative_pose_w8pt(k0, k1, K0, K1, conf, choose_closest=True, T_021=tgt)
            cm = E.mask_confidence(conf.squeeze(-1), info["pos_depth_mask"])
            refined, vb = E.run_bundle_adjust_2_view(info["kpts0_norm"], info["kpts1_norm"], cm, Tw, ba)
            Tp = Tw.clone()
            Tp[vb] = refined
        rot_loss = rot_loss + E.compute_rotation_error(Tp, tgt)
        transl_loss = transl_loss + E.compute_translation_error_as_angle(Tp, tgt)
        poses[(i, j)] = Tp.detach()
    (rot_loss + transl_loss).backward()
    return rot_loss.detach(), transl_loss.detach(), poses, {p: rg["conf_scores_%d_%d" % p].grad for p in order}


@pytest.mark.gpu
@pytest.mark.parametrize("ba", [0, 3])
def test_pose_loss_tuple_against_the_pair_loop(gpu, ba):
    """T = 3, B = 2, N = 257: losses, poses and conf_scores.grad of pose_loss_tuple against the per-pair loop of run_weighted_8_point /
    get_kpts + estimate_relative_pose_w8pt, mask_confidence, run_bundle_adjust_2_view, compute_rotation_error and
    compute_translation_error_as_angle.  Poses are torch.equal.  The bar of the losses and gradients is 10 x the distance between the
    pair loop run in ascending and in descending pair order - the rounding freedom of that path by itself - and must stay under
    1e-3 max|g| (1e-3 |loss|).  Sample 1 of pair (0, 2) has six positive confidences: the bundle adjustment leaves it at its w8pt pose.
    Measured on the MI355X, ba_iterations 0 and 3 alike: the two pair orders differ by 0 in both losses and in every gradient (with
    B = 2 a mean has one rounding whatever its order, the three-term sums happen to round alike here, and a pair's gradient does not
    depend on the order at all), so the bar is 0: pose_loss_tuple is the ascending loop bit for bit (rot_loss 0.118844263 /
    0.11772643, transl_loss 0.666468978 / 0.66067183 at 0 / 3 iterations; max|g| 3.3e-03 to 3.1e-02 per pair)."""
    import e2e_multi_view_matching_amd as E
    T, B, N = 3, 2, 257
    pairs = pairs_of(T)
    d, res = scene(T, B, N, 9)
    d = dict(d)
    for t in range(T):  # make_tuples' poses map world -> camera, the reference's data["pose"] camera -> world: target = inv(pose_j) @ pose_i
        d[f"pose{t}"] = torch.linalg.inv(d[f"pose{t}"].double()).float()
    res = {k: v.clone() for k, v in res.items()}
    c, m = res["conf_scores_0_2"], res["matches0_0_2"]
    keep = torch.nonzero(m[1] >= 0)[:6, 0]
    six = torch.zeros(N, 1)
    six[keep] = c[1][keep]
    c[1] = six
    dg = _dev(d, gpu)
    lr_a, lt_a, poses_a, g_a = _pair_loop(dg, res, gpu, T, ba, pairs)
    lr_d, lt_d, _, g_d = _pair_loop(dg, res, gpu, T, ba, pairs[::-1])
    rg = _leaves(res, gpu)
    out = E.pose_loss_tuple(dg, rg, ba_iterations=ba)
    assert out["rot_loss"].dim() == 0 and out["transl_loss"].dim() == 0 and out["rot_loss"].is_cuda
    (out["rot_loss"] + out["transl_loss"]).backward()
    for p in pairs:
        assert torch.equal(out["poses"][p].detach(), poses_a[p]), p
    if ba:  # the six-confidence sample stayed at its w8pt pose; the others moved
        Tw, _ = E.run_weighted_8_point(dg, {k: v.detach() for k, v in rg.items()}, 0, 2, choose_closest=True, target_T_021=E.relative_pose(dg["pose0"], dg["pose2"]))
        assert torch.equal(out["poses"][(0, 2)][1].detach(), Tw[1]) and not torch.equal(out["poses"][(0, 2)][0].detach(), Tw[0])
    for what, got, a, dsc in (("rot_loss", out["rot_loss"].detach(), lr_a, lr_d), ("transl_loss", out["transl_loss"].detach(), lt_a, lt_d)):
        bar, err = 10.0 * float((a - dsc).abs()), float((got - a).abs())
        print(f"ba={ba} {what}: {float(got):.9g}, pair loop {float(a):.9g}; |ascending - descending| = {bar / 10:.3e}, |tuple - ascending| = {err:.3e}")
        assert bool(got.isfinite()) and bar < 1e-3 * float(a.abs()) and err <= bar, (what, err, bar)
    for p in pairs:
        got, a, dsc = rg["conf_scores_%d_%d" % p].grad, g_a[p], g_d[p]
        assert got is not None and got.shape == (B, N, 1) and bool(got.isfinite().all()), p
        bar, err, scale = 10.0 * float((a - dsc).abs().max()), float((got - a).abs().max()), float(a.abs().max())
        print(f"ba={ba} pair {p}: max|g| = {scale:.3e}, |ascending - descending| = {bar / 10:.3e}, |tuple - ascending| = {err:.3e}")
        assert scale > 0 and bar < 1e-3 * scale and err <= bar, (p, err, bar, scale)
        off = res["matches%d_%d_%d" % (p[0], p[0], p[1])] < 0
        assert float(got.cpu().reshape(B, N)[off].abs().max()) == 0.0, p
    # the six-confidence sample passes its gradient through the w8pt solve (nothing comes back from the bundle adjustment)
    assert float(rg["conf_scores_0_2"].grad[1].abs().max()) > 0


# ------------------------------------------------------------------------------------------------ 5. batch position, repeatability


@pytest.mark.gpu
def test_batch_position_independence_and_repeatability(gpu):
    T, B, N = 5, 2, 257
    d, res = scene(T, B, N, 7)
    Wr = weights(T, B, 7)
    dg = _dev(d, gpu)
    g1, _ = _tuple_gradients(dg, res, gpu, T, Wr, True)
    g2, _ = _tuple_gradients(dg, res, gpu, T, Wr, True)
    swap = lambda v: v.flip(0).contiguous() if torch.is_tensor(v) else v  # noqa: E731
    gs, _ = _tuple_gradients({k: swap(v) for k, v in dg.items()}, {k: swap(v) for k, v in res.items()}, gpu, T, {p: swap(w) for p, w in Wr.items()}, True)
    for p in pairs_of(T):
        assert same_bits(g1[p], g2[p]), p
        assert same_bits(gs[p], g1[p].flip(0)), p
        assert not same_bits(g1[p][0], g1[p][1])


# ------------------------------------------------------------------------------------------------ 6. shape errors


@pytest.mark.gpu
def test_shape_and_null_errors_launch_nothing(gpu):
    from e2e_multi_view_matching_amd import _lib
    T, B, N = 3, 2, 65
    d, res = scene(T, B, N, 7)
    st, conf = _forward_buffers(_dev(d, gpu), res, gpu, T)
    ctx, o, P = st["ctx"], st["out"], st["P"]
    gT = torch.ones(P * B, 4, 4, device=gpu)
    gconf = [torch.full((B, N), float("nan"), device=gpu) for _ in range(P)]
    wide = lambda lst: _lib.ptr_array((lst * 12)[:36])  # noqa: E731  (tables long enough for T = 9)
    (pm, k1), (pc, k2), (pg, k3) = wide(st["matches"]), wide(conf), wide(gconf)
    fn, s = ctx.lib.e2emv_w8pt_tuple_backward, _lib.stream_ptr(gpu)
    tail = (_lib.ptr(o["k0n"]), _lib.ptr(o["k1n"]), _lib.ptr(o["T"]), _lib.ptr(gT), None, pg, s)
    assert fn(ctx.h, B, 9, N, pm, pc, *tail) == _lib.ESHAPE
    assert fn(ctx.h, B, 1, N, pm, pc, *tail) == _lib.ESHAPE
    assert fn(ctx.h, B, T, 7, pm, pc, *tail) == _lib.ESHAPE
    assert fn(ctx.h, 0, T, N, pm, pc, *tail) == _lib.ESHAPE
    assert fn(ctx.h, B, T, N, None, pc, *tail) == _lib.EINVAL
    hole, k4 = _lib.ptr_array([conf[0], None, conf[2]])
    assert fn(ctx.h, B, T, N, pm, hole, *tail) == _lib.EINVAL
    hole_m, k5 = _lib.ptr_array([st["matches"][0], st["matches"][1], None])
    assert fn(ctx.h, B, T, N, hole_m, pc, *tail) == _lib.EINVAL
    l2 = torch.full((2,), float("nan"), device=gpu)
    buf = torch.empty(P * B, device=gpu)
    v8 = torch.empty(P * B, dtype=torch.uint8, device=gpu)
    assert ctx.lib.e2emv_pose_loss_tuple(ctx.h, 0, B, _lib.ptr(gT), _lib.ptr(gT), _lib.ptr(buf), _lib.ptr(buf), _lib.ptr(v8), _lib.ptr(l2), s) == _lib.ESHAPE
    assert ctx.lib.e2emv_pose_loss_tuple_backward(ctx.h, P, 0, _lib.ptr(gT), _lib.ptr(gT), _lib.ptr(l2), _lib.ptr(gT), s) == _lib.ESHAPE
    torch.cuda.synchronize(gpu)
    assert all(bool(g.isnan().all()) for g in gconf) and bool(l2.isnan().all())  # nothing was launched
    assert fn(ctx.h, B, T, N, pm, pc, *tail) == _lib.OK                             # and the context works afterwards
    torch.cuda.synchronize(gpu)
    assert all(bool(g.isfinite().all()) for g in gconf)
