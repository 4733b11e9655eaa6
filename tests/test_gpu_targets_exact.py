"""Ground-truth targets and the match loss with NO tolerance on a decision (csrc/gtmatch.hip: gt_transform, gt_argmin,
gt_finalize, match_loss_kernel).

The scene is built so that every number a decision is taken on is exact in fp32 AND in fp64: focal length 256 (a power
of two: inv(K) is exact), depth 4 everywhere, identity rotation, translation (0.5, -0.25, 0) - every keypoint reprojects
to the exact integer shift (+32, -16), every squared distance is an integer and the errors 5 and 15 (3-4-5 and 9-12-15
offsets) sit ON the two thresholds.  Copied keypoints give exact arg-min ties, invalid depth pixels give rows / columns
that are inf (first scene) or NaN (second scene, t = 0: 0/0) throughout.  The oracle returns identical targets in fp32
and fp64 there (the ungated premise test below), so the device - fp64 reprojection, fp32 errors - has to return them too:
indices equal, weights to 1e-6.  A wrong tie-break, `<` for `<=`, or a lane / wave / workgroup off-by-one has nowhere to
hide (tests/test_gpu_targets.py allows a few flips, excused only next to a boundary).

The match loss is a sum of exact fp32 x fp32 products in fp64: compared with the fp64 oracle at 2^-23 of the sum of the
absolute terms (the final cast to fp32 is 2^-24 relative; a factor two for the order of the fp64 sums)."""
import functools

import numpy as np
import pytest
import torch

H, W = 240, 320
OFFSETS = [(0, 0), (3, 4), (-4, 3), (9, 12), (12, -9), (6, 8), (20, 21), (1, 0), (0, 2), (5, 12)]
SIZES = [1, 63, 64, 65, 257, 1024]
NAN_SIZES = [1, 64, 257]


def exact_scene(B, N, seed, nan_scene=False):
    """-> dict of fp32 tensors: keypoints0/1 [B,N,2], K [B,4,4], T [B,4,4], depth0/1 [B,H,W]."""
    rng = np.random.default_rng(seed)
    K = np.eye(4)
    K[0, 0] = K[1, 1] = 256.0
    K[0, 2], K[1, 2] = 160.0, 120.0
    T = np.eye(4)
    shift = np.array([0, 0])
    if not nan_scene:
        T[:3, 3] = (0.5, -0.25, 0.0)
        shift = np.array([32, -16])
    k0 = np.stack([rng.integers(40, 240, (B, N)), rng.integers(60, 200, (B, N))], -1)
    for i in range(4, N, 5):  # every fifth keypoint repeats the one three places earlier: exact arg-min ties
        k0[:, i] = k0[:, i - 3]
    off = np.array(OFFSETS)[rng.integers(0, len(OFFSETS), (B, N))]
    k1 = k0 + shift + off
    k1 = np.stack([k1[b, rng.permutation(N)] for b in range(B)])
    depth = np.full((2, B, H, W), 4.0)
    if nan_scene:
        # a few keypoints sit on an invalid depth pixel: 0/0 = NaN rows and columns.  NaN counts as minimal, so ONE such
        # keypoint takes every arg-min of its pair and the pair ends without a match: the first pair has them in both images,
        # a middle pair (B = 3) in image 0 only, the last pair has none and keeps its matches next to the others
        for m, k in enumerate((k0, k1)):
            for b in range(B - 1 if m == 0 else 1):
                for i in rng.choice(N, size=min(3, N), replace=False):
                    depth[m, b, k[b, i, 1], k[b, i, 0]] = 0.0
    else:  # a tenth of the depth pixels invalid: x/0 = inf rows and columns
        depth[rng.uniform(size=depth.shape) < 0.1] = 0.0
    # sub-pixel positions: the builder truncates them
    k0 = k0 + rng.uniform(0, 0.99, k0.shape)
    k1 = k1 + rng.uniform(0, 0.99, k1.shape)
    f = lambda a: torch.from_numpy(np.ascontiguousarray(a).astype(np.float32))
    return {"keypoints0": f(k0), "keypoints1": f(k1), "K": f(np.broadcast_to(K, (B, 4, 4))), "T": f(np.broadcast_to(T, (B, 4, 4))),
            "depth0": f(depth[0]), "depth1": f(depth[1])}


def _args(d, conv=lambda t: t):
    return [conv(d[k]) for k in ("keypoints0", "keypoints1", "K", "K", "T", "depth0", "depth1")]


@functools.lru_cache(maxsize=None)
def scene_and_oracle(N, nan_scene):
    """(scene, fp32 oracle targets, fp64 oracle targets, fp64 margins), computed once per size."""
    from oracle import gt_matches as OG
    B = 3 if N == 257 else 2
    d = exact_scene(B, N, seed=1000 * int(nan_scene) + N, nan_scene=nan_scene)
    o32 = OG.compute_gt_matches_of_image_pair(*_args(d), 5.0, 15.0)
    o64 = OG.compute_gt_matches_of_image_pair(*_args(d, lambda t: t.double()), 5.0, 15.0)
    marg = OG.decision_margins(*_args(d, lambda t: t.double()), 5.0, 15.0)
    return d, o32, o64, marg


@pytest.mark.parametrize("nan_scene", [False, True], ids=["inf", "nan"])
def test_exact_scene_premise_fp32_oracle_equals_fp64_oracle(nan_scene):
    """The premise of the device tests, checked wherever the suite runs: on these scenes the oracle takes every decision
    identically in fp32 and fp64, and the scenes hold what they are meant to - matches, exact ties, errors ON both
    thresholds, rows without depth."""
    for N in (NAN_SIZES if nan_scene else SIZES):
        d, (i32, w32), (i64, w64), marg = scene_and_oracle(N, nan_scene)
        assert torch.equal(i32, i64), N
        assert torch.equal(w32, w64.to(w32.dtype)), N
        assert i32.shape == (3 if N == 257 else 2, 2, N + 1)
        if N == 1:
            assert float(w32.abs().max()) == 0.0
        if N >= 257:
            fin = marg["row_gap"].isfinite()
            n_match = int((i32[:, 0] >= 0).sum())
            n_tie = int((marg["row_gap"][fin] == 0).sum()) + int((marg["col_gap"][marg["col_gap"].isfinite()] == 0).sum())
            n_on_thr = int((marg["row_thr"] == 0).sum())
            n_bad = int((~fin).sum())
            print(f"N={N} nan={nan_scene}: {n_match} matches, {n_tie} exact ties, {n_on_thr} rows on a threshold, {n_bad} rows without margin")
            assert n_match >= 100 and n_tie > 0 and n_on_thr > 0 and n_bad > 0
            assert int((i32[:, 0, :-1] == -1).sum()) > 0 and float(w32.max()) > 0
            if nan_scene:  # a pair with a NaN keypoint has no match and no weight; the clean pair beside it has
                assert int((i32[:-1] >= 0).sum()) == 0 and float(w32[:-1].abs().max()) == 0.0 and int((i32[-1, 0] >= 0).sum()) >= 50
    if not nan_scene:  # over the sizes, selected errors sit ON both thresholds and narrowly on either side of them
        from oracle import gt_matches as OG
        emin = torch.cat([OG.reprojection_errors(*_args(scene_and_oracle(N, False)[0]))[0].min(2).values.reshape(-1) for N in SIZES])
        for v in (5.0, 15.0):
            on, below, above = int((emin == v).sum()), int(((emin < v) & (emin > v - 1)).sum()), int(((emin > v) & (emin < v + 1)).sum())
            print(f"selected error == {v}: {on} rows, within 1 px below: {below}, above: {above}")
            assert on > 0 and below > 0 and above > 0


@pytest.mark.gpu
@pytest.mark.parametrize("N", SIZES)
def test_gt_matches_exact_scene(gpu, N):
    import e2e_multi_view_matching_amd as E
    d, (oi, ow), _, _ = scene_and_oracle(N, False)
    idx, w = E.compute_gt_matches_of_image_pair(*[t.to(gpu) for t in _args(d)], 5.0, 15.0)
    idx, w = idx.cpu(), w.cpu()
    nd = int((idx != oi).sum())
    print(f"N={N}: {nd} differing indices, max|dw|={float((w - ow).abs().max()):.2e}, {int((oi[:, 0] >= 0).sum())} matches")
    assert idx.dtype == torch.int64 and torch.equal(idx, oi), (N, nd)
    assert float((w - ow).abs().max()) <= 1e-6


@pytest.mark.gpu
@pytest.mark.parametrize("N", NAN_SIZES)
def test_gt_matches_nan_rows_and_columns(gpu, N):
    """t = 0 and keypoints on invalid depth: their reprojection is 0/0.  NaN counts as minimal, the first NaN index wins."""
    import e2e_multi_view_matching_amd as E
    d, (oi, ow), _, _ = scene_and_oracle(N, True)
    idx, w = E.compute_gt_matches_of_image_pair(*[t.to(gpu) for t in _args(d)], 5.0, 15.0)
    idx, w = idx.cpu(), w.cpu()
    print(f"N={N}: {int((idx != oi).sum())} differing indices, max|dw|={float((w - ow).abs().max()):.2e}")
    assert torch.equal(idx, oi), N
    assert float((w - ow).abs().max()) <= 1e-6


@pytest.mark.gpu
@pytest.mark.parametrize("B,N,mixed", [(1, 1, False), (3, 255, False), (2, 256, True), (5, 700, False), (2, 1024, False)])
def test_match_loss_at_fp64_accuracy(gpu, B, N, mixed):
    """Random targets, -1 in about half the slots of both directions (slot N always), weights with zeros; `mixed`: a log_p
    of both signs, so that the terms cancel and the bar is the sum of their ABSOLUTE values."""
    import e2e_multi_view_matching_amd as E
    from oracle import gt_matches as OG
    g = torch.Generator().manual_seed(17 * N + B)
    ft = N + 1
    lp = torch.randn(B, ft, ft, generator=g)
    if not mixed:
        lp = torch.log_softmax(lp * 3.0, -1)
    idx = torch.randint(0, N, (B, 2, ft), generator=g)
    idx[torch.rand(B, 2, ft, generator=g) < 0.5] = -1
    idx[:, :, N] = -1
    w = torch.rand(B, 2, ft, generator=g)
    w[torch.rand(B, 2, ft, generator=g) < 0.3] = 0.0
    ref = float(OG.compute_match_loss(lp.double(), idx, w.double()))
    t0 = lp.double().gather(2, (idx[:, 0] % ft).unsqueeze(-1)).squeeze(-1) * w[:, 0].double()
    t1 = lp.double().transpose(1, 2).gather(2, (idx[:, 1] % ft).unsqueeze(-1)).squeeze(-1) * w[:, 1].double()
    assert abs(-float(t0.sum() + t1.sum()) / B - ref) <= 1e-12 * max(1.0, abs(ref))  # the terms of the bar ARE the oracle's
    bar = 2.0 ** -23 * float(t0.abs().sum() + t1.abs().sum()) / B
    got = float(E.compute_match_loss(lp.to(gpu), idx.to(gpu), w.to(gpu)))
    print(f"B={B} N={N} mixed={mixed}: loss {got!r} oracle {ref!r} |diff| {abs(got - ref):.3e} bar {bar:.3e}")
    assert int((idx[:, :, :N] == -1).sum()) > 0 or N == 1
    assert abs(got - ref) <= bar, (got, ref, bar)
