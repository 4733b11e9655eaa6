"""The match term of a whole tuple on the device (csrc/gtmatch.hip: ``e2emv_gt_matches_tuple``, ``e2emv_match_loss_tuple``,
``e2emv_match_loss_tuple_backward`` behind ``gt_matches_tuple`` / ``match_loss_tuple`` / ``_MatchLossTuple``).

Targets: the tuple call against the per-pair path (``relative_pose`` + ``compute_gt_matches_of_image_pair``), bit for bit, on an
exact scene and on a random one; on the exact scene also against the fp64 oracle with no tolerance on a decision.  The exact scene is
the recipe of tests/test_gpu_targets_exact.py for T images: focal length 256, depth 4, image t displaced by t * (0.5, -0.25, 0), so
that pair (i, j) reprojects by the exact integer shift (j - i) * (32, -16); repeated keypoints (exact arg-min ties), offsets whose
lengths sit ON both thresholds (5 and 15), a tenth of the depth pixels invalid.  Its premise - the fp32 and the fp64 oracle take every
decision alike on every pair - is checked without a GPU in tests/test_match_loss_tuple.py.

Loss: bitwise the fp32 sum, in pair order, of ``compute_match_loss`` per pair; against the fp64 oracle at
2^-23 * sum|terms| / B (the per-pair bar of test_match_loss_at_fp64_accuracy) + P * 2^-24 * sum_q |loss_q| (one fp32 rounding per
addition of the pair sum).

Backward: every element of d loss / d scores equals, with ``==``, the tensor built here from fp32 CPU arithmetic (g / B, one product,
at most one addition: all correctly rounded, so there is one right answer); against torch.autograd in fp64 through the oracle within
2^-22 relative (one division, one product, at most one addition, 2^-24 each).  The outputs start as NaN inside larger NaN buffers at
addresses 0, 4, 8 and 12 bytes past a 16-byte boundary: every element is written, nothing beside them."""
import functools

import numpy as np
import pytest
import torch

from test_gpu_targets_exact import OFFSETS

MAX_MATCHED, MIN_UNMATCHED = 5.0, 15.0
TARGET_SHAPES = [(2, 1, 1), (3, 2, 63), (3, 2, 64), (3, 3, 65), (5, 2, 257), (8, 1, 16)]
LOSS_SHAPES = [(1, 1, 1, False), (3, 3, 255, False), (10, 2, 256, True), (28, 1, 65, False)]
BWD_SHAPES = [(1, 1, 1), (3, 3, 63), (3, 2, 64), (3, 1, 65), (10, 2, 256), (2, 1, 1024)]
MARGIN = 64  # floats of NaN on either side of an output


def pairs_of(T):
    return [(i, j) for j in range(T) for i in range(j)]


def _f32(a):
    return torch.from_numpy(np.ascontiguousarray(a).astype(np.float32))


def exact_tuple_scene(T, B, N, seed):
    """-> data dict of fp32 tensors in the MatchingDataset layout: keypoints{t} [B,N,2], intr{t}, pose{t} [B,4,4], depth{t} [B,H,W]."""
    rng = np.random.default_rng(seed)
    H, W = 240 + 16 * (T - 1), 320 + 32 * (T - 1)  # every image's keypoints stay inside its depth map
    K = np.eye(4)
    K[0, 0] = K[1, 1] = 256.0
    K[0, 2], K[1, 2] = 160.0, 120.0
    k0 = np.stack([rng.integers(40, 240, (B, N)), rng.integers(60 + 16 * (T - 1), 200 + 16 * (T - 1), (B, N))], -1)
    for i in range(4, N, 5):  # every fifth keypoint repeats the one three places earlier: exact arg-min ties
        k0[:, i] = k0[:, i - 3]
    data = {"ids": list(range(T))}
    for t in range(T):
        # half of the keypoints of an image sit exactly on their reprojection, the others one of the offsets away: pair (i, j) sees
        # the difference of two offsets - 0, a threshold length (3-4-5, 9-12-15) or another integer vector
        off = np.array(OFFSETS)[rng.integers(0, len(OFFSETS), (B, N))] * (rng.uniform(size=(B, N, 1)) < 0.5)
        if t == 0:
            off = off * 0
        k = k0 + t * np.array([32, -16]) + off
        k = np.stack([k[b, rng.permutation(N)] for b in range(B)]) if t else k
        depth = np.full((B, H, W), 4.0)
        depth[rng.uniform(size=depth.shape) < 0.1] = 0.0
        pose = np.eye(4)
        pose[:3, 3] = (-0.5 * t, 0.25 * t, 0.0)  # inv(pose_j) @ pose_i = translation by (j - i) * (0.5, -0.25, 0)
        data["keypoints%d" % t] = _f32(k + rng.uniform(0, 0.99, k.shape))  # sub-pixel positions: the builder truncates them
        data["intr%d" % t] = _f32(np.broadcast_to(K, (B, 4, 4)))
        data["pose%d" % t] = _f32(np.broadcast_to(pose, (B, 4, 4)))
        data["depth%d" % t] = _f32(depth)
    return data


def random_tuple_scene(T, B, N, seed):
    """A scene with nothing exact about it, in the same layout: a plane at world depth 4 seen by T cameras displaced by random
    translations (also along the axis, so every image has its own depth), keypoints of image t = noisy reprojections of those of image 0
    for 70 % of them, random pixels for the rest, in random order; 8 % of the depth pixels are holes."""
    rng = np.random.default_rng(seed)
    H, W, f = 240, 320, 300.0
    K = np.eye(4)
    K[0, 0] = K[1, 1] = f
    K[0, 2], K[1, 2] = W / 2, H / 2
    k0 = np.stack([rng.uniform(60, 260, (B, N)), rng.uniform(50, 190, (B, N))], -1)
    data = {"ids": list(range(T))}
    for t in range(T):
        c = rng.normal(0, 0.15, (B, 3)) * (t > 0)  # camera t in the world; depth of the plane in it: 4 - c_z
        d0, dt = 4.0, 4.0 - c[:, 2]
        X = np.concatenate([(np.floor(k0) - K[:2, 2]) / f * d0, np.full((B, N, 1), d0)], -1) - c[:, None, :]
        k = X[..., :2] / X[..., 2:] * f + K[:2, 2] + rng.normal(0, 1.5, (B, N, 2)) * (t > 0)
        lost = rng.uniform(size=(B, N)) < 0.3
        k[lost] = np.stack([rng.uniform(0, W, int(lost.sum())), rng.uniform(0, H, int(lost.sum()))], -1)
        k = np.clip(k, 0, [W - 1, H - 1])
        k = np.stack([k[b, rng.permutation(N)] for b in range(B)]) if t else k
        depth = np.broadcast_to(dt[:, None, None], (B, H, W)).copy()
        depth[rng.uniform(size=depth.shape) < 0.08] = 0.0
        pose = np.broadcast_to(np.eye(4), (B, 4, 4)).copy()
        pose[:, :3, 3] = c
        data["keypoints%d" % t] = _f32(k)
        data["intr%d" % t] = _f32(np.broadcast_to(K, (B, 4, 4)))
        data["pose%d" % t] = _f32(pose)
        data["depth%d" % t] = _f32(depth)
    return data


def oracle_pair_args(data, i, j, conv=lambda t: t):
    """The arguments of the oracle's builder for pair (i, j) of an exact scene; the relative pose is the exact translation."""
    T = torch.eye(4).repeat(data["pose0"].shape[0], 1, 1)
    T[:, :3, 3] = data["pose%d" % i][:, :3, 3] - data["pose%d" % j][:, :3, 3]
    return [conv(t) for t in (data["keypoints%d" % i], data["keypoints%d" % j], data["intr%d" % i], data["intr%d" % j], T,
                              data["depth%d" % i], data["depth%d" % j])]


@functools.lru_cache(maxsize=None)
def exact_scene_and_oracle(T, B, N):
    """(data, fp32 oracle (indices, weights) stacked [P,B,2,N+1], fp64 oracle likewise, fp64 decision margins per pair) - once per shape."""
    from oracle import gt_matches as OG
    data = exact_tuple_scene(T, B, N, seed=100 * T + N)
    o32, o64, marg = [], [], []
    for i, j in pairs_of(T):
        o32.append(OG.compute_gt_matches_of_image_pair(*oracle_pair_args(data, i, j), MAX_MATCHED, MIN_UNMATCHED))
        o64.append(OG.compute_gt_matches_of_image_pair(*oracle_pair_args(data, i, j, lambda t: t.double()), MAX_MATCHED, MIN_UNMATCHED))
        marg.append(OG.decision_margins(*oracle_pair_args(data, i, j, lambda t: t.double()), MAX_MATCHED, MIN_UNMATCHED))
    stack = lambda o: (torch.stack([x[0] for x in o]), torch.stack([x[1] for x in o]))
    return data, stack(o32), stack(o64), marg


def _to(data, dev):
    return {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in data.items()}


def _bits(t):
    return t.contiguous().view(torch.int32)


# ---- targets ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("scene", ["exact", "random"])
@pytest.mark.parametrize("T,B,N", TARGET_SHAPES)
def test_targets_of_the_tuple_equal_the_per_pair_path(gpu, scene, T, B, N):
    import e2e_multi_view_matching_amd as E
    data = exact_scene_and_oracle(T, B, N)[0] if scene == "exact" else random_tuple_scene(T, B, N, seed=7 * T + N)
    d = _to(data, gpu)
    before = {k: v.clone() for k, v in d.items() if torch.is_tensor(v)}
    idx, w = E.gt_matches_tuple(d, MAX_MATCHED, MIN_UNMATCHED)
    P = T * (T - 1) // 2
    assert idx.shape == (P, B, 2, N + 1) and idx.dtype == torch.int64 and w.shape == idx.shape and w.dtype == torch.float32
    assert all(torch.equal(d[k], v) for k, v in before.items())  # does not touch data
    n_match = 0
    for q, (i, j) in enumerate(pairs_of(T)):
        rel = E.relative_pose(d["pose%d" % i], d["pose%d" % j])
        pi, pw = E.compute_gt_matches_of_image_pair(d["keypoints%d" % i], d["keypoints%d" % j], d["intr%d" % i], d["intr%d" % j], rel,
                                                    d["depth%d" % i], d["depth%d" % j], MAX_MATCHED, MIN_UNMATCHED)
        assert torch.equal(idx[q], pi), (q, int((idx[q] != pi).sum()))
        assert torch.equal(w[q], pw) and torch.equal(_bits(w[q]), _bits(pw)), q
        n_match += int((pi[:, 0] >= 0).sum())
    print(f"{scene} T={T} B={B} N={N}: {n_match} matches over {P} pairs")
    if N >= 63:
        assert n_match > 0
    i2, w2 = E.gt_matches_tuple({k: v for k, v in d.items() if k != "ids"}, MAX_MATCHED, MIN_UNMATCHED, n_images=T)
    assert torch.equal(i2, idx) and torch.equal(_bits(w2), _bits(w))
    if scene == "exact":  # the bar of test_gt_matches_exact_scene: indices equal, weights to 1e-6
        _, _, (oi, ow), _ = exact_scene_and_oracle(T, B, N)
        nd = int((idx.cpu() != oi).sum())
        dw = float((w.cpu().double() - ow.double()).abs().max())
        print(f"  against the fp64 oracle: {nd} differing indices, max|dw| = {dw:.2e}")
        assert nd == 0 and dw <= 1e-6


# ---- loss -------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def loss_inputs(P, B, N, mixed):
    """The generator of test_match_loss_at_fp64_accuracy per pair: -1 in about half the slots (slot N always), weights with zeros."""
    ft = N + 1
    lps, idxs, ws = [], [], []
    for q in range(P):
        g = torch.Generator().manual_seed(17 * N + B + 1000 * q)
        lp = torch.randn(B, ft, ft, generator=g)
        if not mixed:
            lp = torch.log_softmax(lp * 3.0, -1)
        idx = torch.randint(0, N, (B, 2, ft), generator=g)
        idx[torch.rand(B, 2, ft, generator=g) < 0.5] = -1
        idx[:, :, N] = -1
        w = torch.rand(B, 2, ft, generator=g)
        w[torch.rand(B, 2, ft, generator=g) < 0.3] = 0.0
        lps.append(lp)
        idxs.append(idx)
        ws.append(w)
    return lps, torch.stack(idxs), torch.stack(ws)


def _result(scores, T):
    return {"scores_%d_%d" % p: s for p, s in zip(pairs_of(T), scores)}


def _tuple_size(P):
    return next(t for t in range(2, 9) if t * (t - 1) // 2 == P)


@pytest.mark.gpu
@pytest.mark.parametrize("P,B,N,mixed", LOSS_SHAPES)
def test_loss_is_the_fp32_sum_of_the_per_pair_losses(gpu, P, B, N, mixed):
    import e2e_multi_view_matching_amd as E
    from e2e_multi_view_matching_amd import _lib, targets
    from oracle import gt_matches as OG
    lps, idx, w = loss_inputs(P, B, N, mixed)
    ft = N + 1
    scores = [lp.to(gpu) for lp in lps]
    di, dw = idx.to(gpu), w.to(gpu)
    per = torch.stack([E.compute_match_loss(scores[q], di[q], dw[q]) for q in range(P)]).cpu()
    want = torch.zeros((), dtype=torch.float32)
    for q in range(P):
        want = want + per[q]  # fp32, pair order, from 0.0f
    got = E.match_loss_tuple(_result(scores, _tuple_size(P)), di, dw)
    assert got.dim() == 0 and got.dtype == torch.float32 and got.is_cuda and got.grad_fn is None
    pair_loss = torch.full((P,), float("nan"), device=gpu)
    got2 = targets._match_loss_tuple_call(_lib.context(gpu), gpu, scores, di, dw, pair_loss)
    ref_q, terms = [], 0.0
    for q in range(P):
        ref_q.append(float(OG.compute_match_loss(lps[q].double(), idx[q], w[q].double())))
        t0 = lps[q].double().gather(2, (idx[q][:, 0] % ft).unsqueeze(-1)).squeeze(-1) * w[q][:, 0].double()
        t1 = lps[q].double().transpose(1, 2).gather(2, (idx[q][:, 1] % ft).unsqueeze(-1)).squeeze(-1) * w[q][:, 1].double()
        assert abs(-float(t0.sum() + t1.sum()) / B - ref_q[-1]) <= 1e-12 * max(1.0, abs(ref_q[-1]))  # the terms of the bar ARE the oracle's
        terms += float(t0.abs().sum() + t1.abs().sum())
    ref = sum(ref_q)
    bar = 2.0 ** -23 * terms / B + P * 2.0 ** -24 * sum(abs(x) for x in ref_q)
    print(f"P={P} B={B} N={N} mixed={mixed}: loss {float(got)!r} per-pair sum {float(want)!r} oracle {ref!r} |diff| {abs(float(got) - ref):.3e} bar {bar:.3e}")
    assert torch.equal(_bits(got.cpu().reshape(1)), _bits(want.reshape(1))), (float(got), float(want))
    assert torch.equal(_bits(got2.cpu().reshape(1)), _bits(want.reshape(1)))
    assert torch.equal(_bits(pair_loss.cpu()), _bits(per))
    assert abs(float(got) - ref) <= bar, (float(got), ref, bar)


# ---- backward ---------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def backward_inputs(P, B, N):
    """Targets as above, plus: negative indices other than -1; in every (pair, sample) one mutual match, so that (r, col0(r)) and
    (row1(c), c) are ONE element, with non-zero weights; non-zero weights on the dustbin slots, whose -1 / -1 make (N, N) a double term."""
    ft = N + 1
    _, idx, w = loss_inputs(P, B, N, False)
    idx, w = idx.clone(), w.clone()
    g = torch.Generator().manual_seed(5 * N + B)
    neg = torch.rand(P, B, 2, ft, generator=g) < 0.05
    idx[neg] = -torch.randint(1, ft + 1, (int(neg.sum()),), generator=g)  # -1 .. -ft
    idx[:, :, :, N] = -1
    w[:, :, 0, N], w[:, :, 1, N] = 0.75, 0.5
    r0, c0 = N // 2, N // 3
    idx[:, :, 0, r0], idx[:, :, 1, c0] = c0, r0
    w[:, :, 0, r0], w[:, :, 1, c0] = 0.625, 0.3
    return idx, w


def expected_gradient(idx, w, g, valid_only=False):
    """[P,B,ft,ft] fp32 on the CPU: gb = g32 / B32, -(gb * w) put at (r, col0(r)) and at (row1(c), c), accumulated into zeros."""
    P, B, _, ft = idx.shape
    gb = torch.tensor(g, dtype=torch.float32) / torch.tensor(float(B), dtype=torch.float32)
    out = torch.zeros(P, B, ft, ft)
    qi = torch.arange(P)[:, None, None].expand(P, B, ft)
    bi = torch.arange(B)[None, :, None].expand(P, B, ft)
    r = torch.arange(ft)[None, None, :].expand(P, B, ft)
    for s in (0, 1):
        i, v = idx[:, :, s], -(gb * w[:, :, s])
        ok = (i >= -ft) & (i < ft) if valid_only else torch.ones_like(i, dtype=torch.bool)
        j = torch.where(i < 0, i + ft, i)
        where = (qi[ok], bi[ok], r[ok], j[ok]) if s == 0 else (qi[ok], bi[ok], j[ok], r[ok])
        out.index_put_(where, v[ok], accumulate=True)
    return out


def run_backward(gpu, idx, w, g, leave_out=None):
    """One e2emv_match_loss_tuple_backward into NaN-filled outputs with NaN margins; pair q starts 4 * (q % 4) bytes past a 16-byte
    boundary.  -> (gradients [P,B,ft,ft] on the CPU (NaN for a pair left out), the whole buffers, the views)."""
    from e2e_multi_view_matching_amd import _lib
    P, B, _, ft = idx.shape
    n = B * ft * ft
    bufs = [torch.full((n + 2 * MARGIN + 4,), float("nan"), device=gpu) for _ in range(P)]
    outs = []
    for q, buf in enumerate(bufs):
        assert buf.data_ptr() % 16 == 0
        outs.append(buf[MARGIN + q % 4: MARGIN + q % 4 + n])
    pg, keep = _lib.ptr_array([None if q == leave_out else o for q, o in enumerate(outs)])
    gd = torch.tensor([g], dtype=torch.float32, device=gpu)
    di, dw = idx.to(gpu), w.to(gpu)
    with torch.cuda.device(gpu):
        _lib.context(gpu).call("e2emv_match_loss_tuple_backward", P, B, ft - 1, _lib.ptr(di), _lib.ptr(dw), _lib.ptr(gd), pg, _lib.stream_ptr(gpu))
    torch.cuda.synchronize()
    return torch.stack([o.cpu().reshape(B, ft, ft) for o in outs]), bufs, outs


def _margins_untouched(bufs, B, ft, skip=None):
    n = B * ft * ft
    for q, buf in enumerate(bufs):
        if q == skip:
            continue
        b = buf.cpu()
        lo = MARGIN + q % 4
        if not (bool(b[:lo].isnan().all()) and bool(b[lo + n:].isnan().all())):
            return False
    return True


@pytest.mark.gpu
@pytest.mark.parametrize("g", [1.0, 0.37])
@pytest.mark.parametrize("P,B,N", BWD_SHAPES)
def test_backward_writes_every_element_exactly(gpu, P, B, N, g):
    from oracle import gt_matches as OG
    idx, w = backward_inputs(P, B, N)
    ft = N + 1
    want = expected_gradient(idx, w, g)
    # the inputs hold what they are meant to: a coinciding element, and the (N, N) double term with both weights non-zero
    gb = float(torch.tensor(g, dtype=torch.float32) / torch.tensor(float(B), dtype=torch.float32))
    assert bool((want[:, :, N, N] == -(torch.tensor(gb) * 0.75) + -(torch.tensor(gb) * 0.5)).all())
    assert bool((want[:, :, N // 2, N // 3] == -(torch.tensor(gb) * 0.625) + -(torch.tensor(gb) * 0.3)).all()) or N == 1
    got, bufs, _ = run_backward(gpu, idx, w, g)
    n_nan, n_bad = int(got.isnan().sum()), int((got != want).sum())
    print(f"P={P} B={B} N={N} g={g}: {n_nan} NaN left, {n_bad} elements differ, {int((want != 0).sum())} non-zeros of {want.numel()}")
    assert n_nan == 0 and n_bad == 0
    assert _margins_untouched(bufs, B, ft)
    # torch.autograd in fp64 through the oracle: 2^-22 relative on every element
    lp = [torch.zeros(B, ft, ft, dtype=torch.float64, requires_grad=True) for _ in range(P)]
    g64 = float(torch.tensor(g, dtype=torch.float32))
    (sum(OG.compute_match_loss(lp[q], idx[q], w[q].double()) for q in range(P)) * g64).backward()
    ref = torch.stack([x.grad for x in lp])
    err = (got.double() - ref).abs()
    print(f"  against fp64 autograd: max relative error {float((err / ref.abs().clamp_min(1e-300))[ref != 0].max()):.3e} (bar {2.0 ** -22:.3e})")
    assert bool((err <= 2.0 ** -22 * ref.abs()).all())
    if g == 1.0 and P > 1:  # a NULL entry leaves that pair alone and the others bit-identical
        q0 = P // 2
        got2, bufs2, _ = run_backward(gpu, idx, w, g, leave_out=q0)
        assert bool(bufs2[q0].cpu().isnan().all())
        keep = [q for q in range(P) if q != q0]
        assert torch.equal(_bits(got2[keep]), _bits(got[keep])) and _margins_untouched(bufs2, B, ft, skip=q0)


@pytest.mark.gpu
def test_backward_ignores_indices_that_address_nothing(gpu):
    """An index outside [-ft, ft) contributes nothing and writes nowhere."""
    P, B, N = 3, 2, 64
    ft = N + 1
    idx, w = backward_inputs(P, B, N)
    idx = idx.clone()
    g = torch.Generator().manual_seed(3)
    bad = torch.rand(P, B, 2, ft, generator=g) < 0.2
    junk = torch.tensor([ft, ft + 1, -ft - 1, 2 ** 31, -2 ** 31, 2 ** 40 + 3, -2 ** 62, 2 ** 63 - 1, -2 ** 63, 2 ** 32 + 5, -2 ** 32 + 5])
    idx[bad] = junk[torch.randint(0, len(junk), (int(bad.sum()),), generator=g)]
    want = expected_gradient(idx, w, 0.37, valid_only=True)
    got, bufs, _ = run_backward(gpu, idx, w, 0.37)
    assert int(got.isnan().sum()) == 0 and int((got != want).sum()) == 0 and _margins_untouched(bufs, B, ft)


# ---- the Python front ---------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_no_host_synchronisation_from_the_targets_to_the_score_gradients(gpu):
    """``torch.cuda.set_sync_debug_mode("error")`` around gt_matches_tuple, match_loss_tuple and its backward down to d logZ; the scores
    are plain leaves, so the matcher's own backward is not inside the guarded region.  The gradients are the exact ones."""
    import e2e_multi_view_matching_amd as E
    T, B, N = 3, 2, 64
    d = _to(exact_scene_and_oracle(T, B, N)[0], gpu)
    g = torch.Generator().manual_seed(1)
    scores = [torch.log_softmax(torch.randn(B, N + 1, N + 1, generator=g), -1).to(gpu).requires_grad_(q != 1) for q in range(3)]
    result = _result(scores, T)
    E.match_loss_tuple(result, *E.gt_matches_tuple(d, MAX_MATCHED, MIN_UNMATCHED)).backward()  # first use: workspace, context
    for s in scores:
        s.grad = None
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        idx, w = E.gt_matches_tuple(d, MAX_MATCHED, MIN_UNMATCHED)
        loss = E.match_loss_tuple(result, idx, w)
        g0, g2 = torch.autograd.grad(loss, [scores[0], scores[2]])
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert loss.grad_fn is not None and loss.dim() == 0
    want = expected_gradient(idx.cpu(), w.cpu(), 1.0)
    assert bool((g0.cpu() == want[0]).all()) and bool((g2.cpu() == want[2]).all()) and float(want[0].abs().sum()) > 0
    with torch.no_grad():
        assert E.match_loss_tuple(result, idx, w).grad_fn is None
    assert torch.equal(_bits(E.match_loss_tuple(result, idx, w).detach().reshape(1)), _bits(loss.detach().reshape(1)))


def _model_and_oracle(cfg, data_kw, seed):
    """The model recipe of test_gpu_backward._grads, and autograd over the oracle with that file's _match_loss on its _targets."""
    import test_gpu_backward as GB
    from e2e_multi_view_matching_amd import MultiViewMatcher
    from e2e_multi_view_matching_amd.synthetic import make_tuples
    from oracle.matcher import matcher_forward
    torch.manual_seed(seed)
    model = MultiViewMatcher(cfg)
    GB._randomize_bn(model, seed)
    with torch.no_grad():
        model.bin_score.fill_(0.7)
        for prm in [model.kenc.encoder[-1].bias] + [l.mlp[-1].bias for l in model.gnn.layers]:
            prm.normal_(0.0, 0.05)
    data = make_tuples(seed=seed, **data_kw)
    T, B, N = data_kw["tuple_size"], data_kw["batch"], data_kw["n_kpts"]
    pairs = pairs_of(T)
    targets = [GB._targets(B, N, seed * 100 + n) for n in range(len(pairs))]
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    leaves = {k: sd[k].requires_grad_(True) for k, _ in model.named_parameters()}
    ocfg = dict(model.config)
    ocfg.update(full_output=False, grad=True)
    for k in ("mfma_precision", "autograd", "check_finite"):
        ocfg.pop(k, None)
    ref = matcher_forward(data, sd, ocfg)
    loss_ref = sum(GB._match_loss(ref["scores_%d_%d" % p], *targets[n]) for n, p in enumerate(pairs))
    loss_ref.backward()
    # the oracle's targets name the dustbin N, the device entry takes the reference's -1: both address column N
    idx_o = torch.stack([t[0] for t in targets])
    idx_d = torch.where(idx_o == N, torch.full_like(idx_o, -1), idx_o)
    assert bool((idx_d == -1).any()) and bool((torch.where(idx_d < 0, idx_d + N + 1, idx_d) == idx_o).all())
    return model, data, leaves, float(loss_ref.detach()), idx_d, torch.stack([t[1] for t in targets])


@pytest.mark.gpu
@pytest.mark.parametrize("T,B,N", [(3, 2, 64), (2, 2, 256)])
def test_parameter_gradients_end_to_end(gpu, T, B, N):
    import test_gpu_backward as GB
    import e2e_multi_view_matching_amd as E
    cfg = {"GNN_layers": ["self", "cross"], "sinkhorn_iterations": 50}
    if T > 2:
        cfg.update(multi_frame_matching=True, tuple_size=T)
    model, data, leaves, loss_ref, idx, w = _model_and_oracle(cfg, dict(batch=B, tuple_size=T, n_kpts=N), seed=20 + T)
    model = model.to(gpu).train()
    out = model(_to(data, gpu))
    loss = E.match_loss_tuple(out, idx.to(gpu), w.to(gpu))
    loss.backward()
    got = float(loss.detach())
    print(f"T={T} B={B} N={N}: loss {got!r} oracle {loss_ref!r}")
    assert abs(got - loss_ref) < 1e-3 * abs(loss_ref)
    worst = GB._check(model, leaves)  # _has_finite_gradients, and every parameter gradient within REL = 1e-3
    print(f"  worst relative gradient error {max(worst.values()):.3e}")
    assert GB._has_finite_gradients(model) and len(worst) == sum(1 for _ in model.parameters())


@pytest.mark.gpu
def test_compute_match_loss_on_training_scores_trains(gpu):
    """The defect: on the scores of a .train() forward the per-pair loss had no graph.  It has one now, and its backward is the tuple
    path at P = 1: d logZ bit for bit; bin_score.grad - behind the matcher's own backward, which accumulates with atomics in no fixed
    order - to 1e-5 relative."""
    import e2e_multi_view_matching_amd as E
    cfg = {"GNN_layers": ["self", "cross"], "sinkhorn_iterations": 50}
    model, data, _, _, idx, w = _model_and_oracle(cfg, dict(batch=2, tuple_size=2, n_kpts=64), seed=31)
    model = model.to(gpu).train()
    d, di, dw = _to(data, gpu), idx.to(gpu), w.to(gpu)
    seen = {}
    for name, fn in (("pair", lambda out: E.compute_match_loss(out["scores_0_1"], di[0], dw[0])),
                     ("tuple", lambda out: E.match_loss_tuple(out, di, dw))):
        model.zero_grad(set_to_none=True)
        out = model(d)
        assert out["scores_0_1"].requires_grad
        out["scores_0_1"].retain_grad()
        loss = fn(out)
        assert loss.grad_fn is not None and loss.dim() == 0
        loss.backward()
        seen[name] = (loss.detach().cpu(), out["scores_0_1"].grad.cpu(), model.bin_score.grad.detach().cpu().clone())
        if name == "pair":  # without a graph: today's entry, the same number
            plain = E.compute_match_loss(out["scores_0_1"].detach(), di[0], dw[0])
            assert plain.grad_fn is None and torch.equal(_bits(plain.cpu().reshape(1)), _bits(seen[name][0].reshape(1)))
    (l1, z1, b1), (l2, z2, b2) = seen["pair"], seen["tuple"]
    print(f"loss {float(l1)!r} / {float(l2)!r}, bin_score.grad {b1.flatten().tolist()} / {b2.flatten().tolist()}")
    assert torch.equal(_bits(l1.reshape(1)), _bits(l2.reshape(1))) and torch.equal(_bits(z1), _bits(z2))
    assert bool(b1.isfinite().all()) and float(b1.abs().max()) > 0
    assert float((b1 - b2).abs().max()) <= 1e-5 * float(b2.abs().max())
