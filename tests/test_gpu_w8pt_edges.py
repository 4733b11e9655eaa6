"""The weighted 8-point family of csrc/pose.hip at its edges (-m gpu), against the fp64 oracle (oracle/w8pt.py + kornia_fns.py).

Two stages.  (a) INPUT: the kernel's own normalised coordinates and weights against the fp32 formula, with every sample and every
view on its own intrinsics (fx != fy, K0 != K1, junk in every entry ``normalize`` does not read) - an indexing slip reads
something visibly wrong.  (b) SOLVE: the device's normalised coordinates and weights go to the fp64 oracle with identity
intrinsics, which takes the fp32 input rounding out of the comparison; everything behind the normalisation (fp64 Gram matrix,
9 x 9 Jacobi, rank-2 projection, de-normalisation, decomposition, triangulation) is then held to ten times the measured
device-against-oracle figure, and the masks to the oracle's own decisions outside a 1e-4 margin.

The scenes are conditions of the tests: each test asserts what it needs of them (margin shares, a unique cheirality winner,
matches between the right and every wrong inlier threshold).  The committed seeds satisfy them with the oracle alone.
"""
import functools
import itertools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# Largest |device - fp64 oracle| of the solve stage over every case of this file (printed by the tests, -s shows them).  T and
# F / max|F| are fp32 outputs of fp64 arithmetic: the figure is output rounding.  N == 8 takes the smallest NON-null singular
# vector (thin-SVD quirk of the reference), conditioned by sigma7 / sigma8: its own pair of constants.
MEASURED_T = 3.32e-8     # N >= 9: dense N = 257 (3.311e-8); ragged 2.95e-8, tuple T = 8 3.26e-8 - half an fp32 ulp of an entry near 1
MEASURED_F = 9.42e-8     # N >= 9: tuple T = 8 (9.419e-8); dense 6.56e-8, ragged 5.12e-8
MEASURED_T_N8 = 2.95e-8  # ragged n = 8 (2.950e-8); dense 2.915e-8
MEASURED_F_N8 = 4.40e-8  # dense N = 8 (4.396e-8); ragged 2.53e-8
CAP, CAP_T_N8, CAP_F_N8 = 2e-6, 2e-5, 1e-4  # the bars (10 x measured) may not exceed: a tenth of the bars of test_gpu_pose.py for N >= 9

N_SIZES = (8, 9, 63, 64, 65, 255, 256, 257, 513)  # thin-SVD quirk, first full system, around the 64-lane wave and the 256-thread block
SEEDS = {8: 801, 9: 9, 63: 63, 64: 64, 65: 65, 255: 255, 256: 256, 257: 257, 513: 513}
FOCALS = (400.0, 700.0, 1100.0, 600.0)  # fx0, fy0, fx1, fy1 (+-5 % per sample): every wrong mean below is >= 20 % off the right one


# ---------------------------------------------------------------- scenes ----------------------------------------------------------------
def _rodrigues(axis, angle):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    S = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * S + (1 - np.cos(angle)) * S @ S


def _intrinsics(rng, fx, fy):
    """4 x 4: the four entries ``normalize`` reads, K22 = 1, distinct non-zero junk everywhere else (the skew entries, the
    last column, row 2 off the diagonal, row 3)."""
    K = 10.0 + 3.0 * rng.permutation(16).reshape(4, 4) + rng.uniform(0.1, 0.9)
    K[0, 0], K[1, 1] = fx * rng.uniform(0.95, 1.05), fy * rng.uniform(0.95, 1.05)
    K[0, 2], K[1, 2] = rng.uniform(300, 340), rng.uniform(220, 260)
    K[2, 2] = 1.0
    return K


def _project(K, X):
    return np.stack([K[0, 0] * X[:, 0] / X[:, 2] + K[0, 2], K[1, 1] * X[:, 1] / X[:, 2] + K[1, 2]], 1)


def _sample(rng, n):
    """One two-view problem of n correspondences: rotation of about 0.2 rad, unit baseline, depth 3-7 baselines, 0.5 px noise,
    a fifth gross outliers with confidence 0 and a fifth mild ones (1-6 px off, weight kept: epipolar errors on both sides of
    the 3 px threshold).  Gross outliers need 16 weighted rows left: below that (N = 8, 9) a zero-weight row would leave fewer
    than 8 independent design rows and the singular vector the reference selects would not be unique."""
    R = _rodrigues(rng.normal(size=3), rng.uniform(0.15, 0.25))
    t = rng.normal(size=3)
    t /= np.linalg.norm(t)
    K0, K1 = _intrinsics(rng, FOCALS[0], FOCALS[1]), _intrinsics(rng, FOCALS[2], FOCALS[3])
    z = rng.uniform(3.0, 7.0, n)
    px, py = rng.uniform(0, 2 * K0[0, 2], n), rng.uniform(0, 2 * K0[1, 2], n)
    X = np.stack([(px - K0[0, 2]) / K0[0, 0] * z, (py - K0[1, 2]) / K0[1, 1] * z, z], 1)
    k0 = np.stack([px, py], 1) + rng.normal(0, 0.5, (n, 2))
    k1 = _project(K1, X @ R.T + t) + rng.normal(0, 0.5, (n, 2))
    conf = rng.uniform(0.1, 1.0, n)
    n_gross = n // 5 if n - n // 5 >= 16 else 0
    n_mild = n // 5
    order = rng.permutation(n)
    gross, mild = order[:n_gross], order[n_gross:n_gross + n_mild]
    k1[gross] = rng.uniform(0, 1, (n_gross, 2)) * (2 * K1[0, 2], 2 * K1[1, 2])
    conf[gross] = 0.0
    ang, d = rng.uniform(0, 2 * np.pi, n_mild), rng.uniform(1.0, 6.0, n_mild)
    k1[mild] += np.stack([d * np.cos(ang), d * np.sin(ang)], 1)
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))  # noqa: E731
    return SimpleNamespace(k0=f32(k0), k1=f32(k1), K0=f32(K0), K1=f32(K1), conf=f32(conf), T=f32(T))


@functools.lru_cache(maxsize=None)
def _scene(B, N, seed):
    rng = np.random.default_rng(seed)
    ss = [_sample(rng, N) for _ in range(B)]
    return SimpleNamespace(**{k: torch.stack([getattr(s, k) for s in ss]) for k in ("k0", "k1", "K0", "K1", "conf", "T")})


def _kd(K, kdim):
    return K[..., :kdim, :kdim].contiguous()


# --------------------------------------------------------- the three device entries ---------------------------------------------------------
def _pack(T, info, B, N):
    c = lambda t: None if t is None else t.cpu()  # noqa: E731
    return SimpleNamespace(T=c(T), F=c(info["F"]), k0n=c(info["kpts0_norm"]), k1n=c(info["kpts1_norm"]),
                           cfn=c(info["confidence"]).reshape(B, N), inl=c(info["inliers"]).bool(), pos=c(info["pos_depth_mask"]).bool(),
                           status=c(info["status"]))


def _dense(gpu, k0, k1, K0, K1, conf, closest=False, Tgt=None):
    """``estimate_relative_pose_w8pt`` of pose.py (``e2emv_w8pt``) with determine_inliers; everything back on the CPU."""
    from e2e_multi_view_matching_amd import pose as P
    T, info = P.estimate_relative_pose_w8pt(k0.to(gpu), k1.to(gpu), K0.to(gpu), K1.to(gpu), conf.to(gpu), choose_closest=closest,
                                            T_021=Tgt.to(gpu) if closest else None, determine_inliers=True)
    return _pack(T, info, *k0.shape[:2])


def _ragged(gpu, n_per, k0, k1, K0, K1, conf, closest=False, Tgt=None, with_F=True):
    """One ``e2emv_w8pt_ragged`` launch as ``multi_view._w8pt_ba_on_device`` makes it (``with_F=False``: d_F null, the back-end's
    call).  The output buffers start as NaN / 2 / -1, so a row the kernels leave unwritten cannot pass for a zero."""
    from e2e_multi_view_matching_amd import _lib
    ctx = _lib.context(gpu)
    B, N = k0.shape[:2]
    up = lambda t: t.to(gpu).contiguous()  # noqa: E731
    d_n = up(torch.as_tensor(n_per, dtype=torch.int32))
    d_k0, d_k1, d_K0, d_K1, d_cf = up(k0), up(k1), up(K0), up(K1), up(conf)
    d_Tg = up(Tgt) if closest else None
    nan = lambda *s: torch.full(s, float("nan"), dtype=torch.float32, device=gpu)  # noqa: E731
    T, k0n, k1n, cfn, F = nan(B, 4, 4), nan(B, N, 2), nan(B, N, 2), nan(B, N), (nan(B, 3, 3) if with_F else None)
    inl = torch.full((B, N), 2, dtype=torch.uint8, device=gpu)
    pos = torch.full((B, N), 2, dtype=torch.uint8, device=gpu)
    status = torch.full((B,), -1, dtype=torch.int32, device=gpu)
    P = _lib.ptr
    with torch.cuda.device(gpu):
        ctx.call("e2emv_w8pt_ragged", B, N, P(d_n), P(d_k0), P(d_k1), P(d_K0), P(d_K1), K0.shape[-1], B, P(d_cf), 1 if closest else 0,
                 P(d_Tg), 1, P(T), P(k0n), P(k1n), P(cfn), P(inl), P(pos), P(F), P(status), _lib.stream_ptr(gpu))
    c = lambda t: None if t is None else t.cpu()  # noqa: E731
    return SimpleNamespace(T=c(T), F=c(F), k0n=c(k0n), k1n=c(k1n), cfn=c(cfn), inl=c(inl), pos=c(pos), status=c(status))


def _tuple(gpu, data, result, closest, targets):
    """``run_weighted_8_point_tuple`` (``e2emv_w8pt_tuple``): {(i, j): outputs on the CPU}."""
    from e2e_multi_view_matching_amd import pose as P
    dg = {k: v.to(gpu) for k, v in data.items()}
    rg = {k: v.to(gpu) for k, v in result.items()}
    tg = {p: v.to(gpu) for p, v in targets.items()} if closest else None
    out = P.run_weighted_8_point_tuple(dg, rg, choose_closest=closest, targets=tg, determine_inliers=True)
    B, N = data["keypoints0"].shape[:2]
    return {p: _pack(T, info, B, N) for p, (T, info) in out.items()}


def _pose_errors(gpu, T0, T1):
    """(rot [B], transl [B], rot reduce=False, transl reduce=False [n_valid], rot mean, transl mean) of pose.py, on the CPU."""
    from e2e_multi_view_matching_amd import pose as P
    a, b = T0.to(gpu), T1.to(gpu)
    rot, tr = P.pose_errors(a, b)
    return (rot.cpu(), tr.cpu(), P.compute_rotation_error(a, b, reduce=False).cpu(),
            P.compute_translation_error_as_angle(a, b, reduce=False).cpu(), P.compute_rotation_error(a, b).cpu(),
            P.compute_translation_error_as_angle(a, b).cpu())


def _relative_pose(gpu, pose_a, pose_b):
    from e2e_multi_view_matching_amd import targets
    return targets.relative_pose(pose_a.to(gpu), pose_b.to(gpu)).cpu()


# ------------------------------------------------------------- the two stages -------------------------------------------------------------
def _ulp32(x):
    """fp32 spacing at |x| (x fp32 or fp64)."""
    return torch.from_numpy(np.spacing(np.abs(x.numpy()).astype(np.float32))).double()


def _check_inputs(out, k0, k1, K0, K1, conf, exact=False):
    """Stage (a).  Coordinates: the fp32 formula (x - c) / f by torch on the CPU with each view's own K, one fp32 ulp (``exact``:
    no difference at all - a subtraction and a correctly rounded division have one fp32 result; measured 0 ulp everywhere).  Weights:
    conf / (sum + 1e-6) in fp64, 2 ulp - the kernel sums in fp64, rounds the sum to fp32 once, adds 1e-6 and divides in fp32:
    three roundings of half an ulp each."""
    from oracle import w8pt as O
    B, worst = k0.shape[0], 0.0
    for got, k, K in ((out.k0n, k0, K0), (out.k1n, k1, K1)):
        exp = O.normalize(k, K.expand(B, -1, -1))
        d = (got.double() - exp.double()).abs() / _ulp32(exp)
        worst = max(worst, float(d.max()))
        assert worst <= (0.0 if exact else 1.0), ("normalised coordinates", int((d > 1).sum()), worst)
    c64 = conf.reshape(B, -1).double()
    exp = c64 / (c64.sum(1, keepdim=True) + 1e-6)
    d = (out.cfn.double() - exp).abs() / _ulp32(exp)
    print(f"\n[w8pt-edges] inputs: coordinates within {worst:.2f} ulp, weights within {float(d.max()):.2f} ulp")
    assert float(d.max()) <= 2.0, ("weights", int((d > 2).sum()), float(d.max()))


def _cheirality_counts(F, x1, x2):
    """Matches in front of both cameras under each of the oracle's four candidates: [B, 4]."""
    from oracle import kornia_fns as KF
    Rs, ts = KF.motion_from_essential(F)
    B = F.shape[0]
    P1 = torch.eye(4, dtype=F.dtype)[:3].expand(B, 4, 3, 4)
    X = KF.triangulate_points(P1, torch.cat([Rs, ts], -1), x1[:, None].expand(-1, 4, -1, -1), x2[:, None].expand(-1, 4, -1, -1))
    return ((X[..., 2] > 0) & (KF.depth_from_point(Rs, ts, X) > 0)).sum(-1)


def _check_solve(out, K0, K1, closest, Tgt):
    """Stage (b) for a batch of full rows.  The fp64 oracle solves the DEVICE's normalised coordinates and weights with identity
    intrinsics (a uniform rescaling of the weights does not move a singular vector); the inlier threshold comes from the real
    intrinsics.  The masks must equal the oracle's except where the oracle's own |epi_err - thr| < 1e-4 thr or
    min(|depth0|, |depth1|) < 1e-6.  Returns the figures the callers hold to their bars."""
    from oracle import w8pt as O
    B, N = out.k0n.shape[:2]
    eye = torch.eye(3, dtype=torch.float64).repeat(B, 1, 1)
    x1, x2 = out.k0n.double(), out.k1n.double()
    T64, i64 = O.estimate_relative_pose_w8pt(x1, x2, eye, eye, out.cfn.double(), closest, Tgt.double() if closest else None, True)
    if not closest:  # condition on the scene: the cheirality vote has one winner (the candidate ORDER is SVD-sign dependent)
        top = _cheirality_counts(i64["F"], x1, x2).sort(-1, descending=True).values
        assert bool((top[:, 0] > top[:, 1]).all()), top
    K0, K1 = K0.expand(B, -1, -1).double(), K1.expand(B, -1, -1).double()
    thr = (3.0 / ((K0[:, 0, 0] + K0[:, 1, 1] + K1[:, 0, 0] + K1[:, 1, 1]) / 4.0))[:, None]
    err = i64["epi_err"]
    near = (err - thr).abs() < 1e-4 * thr
    marg = torch.minimum(i64["depth0"].abs(), i64["depth1"].abs()) < 1e-6
    pos64 = i64["pos_depth_mask"]
    inl64 = pos64 & (err <= thr)
    assert bool(((out.pos == pos64) | marg).all()), ("pos_depth_mask", int(((out.pos != pos64) & ~marg).sum()))
    assert bool(((out.inl == inl64) | near | marg).all()), ("inliers", int(((out.inl != inl64) & ~near & ~marg).sum()))
    Fd, F64 = out.F.double(), i64["F"]
    dF = (Fd / Fd.abs().amax((1, 2), keepdim=True) - F64 / F64.abs().amax((1, 2), keepdim=True)).abs().amax((1, 2))
    dT = (out.T.double() - T64).abs().amax((1, 2))
    return SimpleNamespace(dT=dT, dF=dF, n_margin=int((near | marg).sum()), err=err, thr=thr, near=near, marg=marg, pos64=pos64,
                           inl64=inl64)


def _bars(n):
    return (10 * MEASURED_T_N8, 10 * MEASURED_F_N8) if n == 8 else (10 * MEASURED_T, 10 * MEASURED_F)


def _hold(r, n, what):
    """Prints the figures of one case and holds them to the bars of its size."""
    dT, dF = float(r.dT.max()), float(r.dF.max())
    print(f"\n[w8pt-edges] {what}: max|dT| = {dT:.3e}  max|dF| = {dF:.3e}  in margin = {r.n_margin}")
    bT, bF = _bars(n)
    assert dT <= bT and dF <= bF, (what, dT, bT, dF, bF)


def _rows(out, b, n):
    """Sample b of a batch, its first n rows, as a batch of one."""
    return SimpleNamespace(T=out.T[b:b + 1], F=None if out.F is None else out.F[b:b + 1], k0n=out.k0n[b:b + 1, :n],
                           k1n=out.k1n[b:b + 1, :n], cfn=out.cfn[b:b + 1, :n], inl=out.inl[b:b + 1, :n].bool(),
                           pos=out.pos[b:b + 1, :n].bool(), status=out.status[b:b + 1])


def _same_bits(a, b, what):
    for k in ("T", "F", "k0n", "k1n", "cfn", "inl", "pos", "status"):
        x, y = getattr(a, k), getattr(b, k)
        if x is None or y is None:
            continue
        same = torch.equal(x.view(torch.int32), y.view(torch.int32)) if x.dtype == torch.float32 else torch.equal(x.to(torch.int32), y.to(torch.int32))
        assert same, (what, k)


# ------------------------------------------------- 1. two-stage parity of the dense solve -------------------------------------------------
def test_the_bars_sit_under_their_caps():
    assert 10 * MEASURED_T <= CAP and 10 * MEASURED_F <= CAP
    assert 10 * MEASURED_T_N8 <= CAP_T_N8 and 10 * MEASURED_F_N8 <= CAP_F_N8


@pytest.mark.parametrize("kdim", [4, 3])
@pytest.mark.parametrize("closest", [False, True])
@pytest.mark.parametrize("N", N_SIZES)
def test_dense_solve_in_two_stages(gpu, N, closest, kdim):
    B = 3
    s = _scene(B, N, SEEDS[N])
    K0, K1 = _kd(s.K0, kdim), _kd(s.K1, kdim)
    out = _dense(gpu, s.k0, s.k1, K0, K1, s.conf, closest, s.T)
    _check_inputs(out, s.k0, s.k1, K0, K1, s.conf)
    r = _check_solve(out, K0, K1, closest, s.T)
    assert r.n_margin <= 0.01 * B * N, r.n_margin  # condition on the seed: at most 1 % of the matches inside either margin
    assert int(out.status.abs().max()) == 0
    _hold(r, N, f"dense N={N} closest={closest} kdim={kdim}")


# ------------------------------------------- 2. the inlier threshold uses all four focal lengths -------------------------------------------
def _wrong_thresholds(K0, K1):
    fx0, fy0, fx1, fy1 = K0[:, 0, 0].double(), K0[:, 1, 1].double(), K1[:, 0, 0].double(), K1[:, 1, 1].double()
    return {"K0 only": 3.0 / ((fx0 + fy0) / 2), "K1 only": 3.0 / ((fx1 + fy1) / 2), "fx0, fy1 twice": 3.0 / ((fx0 + fy1) / 2),
            "fx0 alone": 3.0 / fx0}


@pytest.mark.parametrize("N", [n for n in N_SIZES if n >= 255])
def test_inlier_threshold_uses_all_four_focal_lengths(gpu, N):
    B = 3
    s = _scene(B, N, SEEDS[N])
    out = _dense(gpu, s.k0, s.k1, s.K0, s.K1, s.conf)
    r = _check_solve(out, s.K0, s.K1, False, s.T)
    for name, wrong in _wrong_thresholds(s.K0, s.K1).items():
        wrong = wrong[:, None]
        assert bool(((wrong - r.thr).abs() > 0.1 * r.thr).all()), name  # far more than the 1e-4 margin
        lo, hi = torch.minimum(wrong, r.thr), torch.maximum(wrong, r.thr)
        between = (r.err > lo) & (r.err <= hi) & r.pos64 & ~r.near & ~r.marg
        # condition on the scene: a kernel on this wrong threshold decides at least 3 matches of EVERY sample differently
        assert int(between.sum(1).min()) >= 3, (name, between.sum(1))
        assert bool((out.inl[between] == r.inl64[between]).all()), name


# ------------------------------------------- 3. ragged batches against the oracle, poisoned padding -------------------------------------------
RAGGED_N, RAGGED_SEED = 300, 3
RAGGED_N_PER = (0, 7, 8, 9, 64, 65, 255, 256, 257, 300)


@functools.lru_cache(maxsize=None)
def _ragged_batch():
    """The counts in a shuffled order, one scene per sample, every row beyond n_per[b] NaN in both keypoint arrays and in conf."""
    rng = np.random.default_rng(RAGGED_SEED)
    n_per = [int(n) for n in rng.permutation(RAGGED_N_PER)]
    ss = [_sample(rng, n) for n in n_per]
    B, N = len(n_per), RAGGED_N
    k0, k1, conf = torch.full((B, N, 2), float("nan")), torch.full((B, N, 2), float("nan")), torch.full((B, N), float("nan"))
    for b, (n, s) in enumerate(zip(n_per, ss)):
        k0[b, :n], k1[b, :n], conf[b, :n] = s.k0, s.k1, s.conf
    return SimpleNamespace(n_per=n_per, samples=ss, k0=k0, k1=k1, conf=conf, K0=torch.stack([s.K0 for s in ss]),
                           K1=torch.stack([s.K1 for s in ss]), T=torch.stack([s.T for s in ss]))


def _ragged_run(gpu, rb, idx=None, **kw):
    idx = list(range(len(rb.n_per))) if idx is None else idx
    return _ragged(gpu, [rb.n_per[b] for b in idx], rb.k0[idx], rb.k1[idx], rb.K0[idx], rb.K1[idx], rb.conf[idx], Tgt=rb.T[idx], **kw)


def _check_ragged_shape(out, n_per):
    """Padding rows read exactly 0 everywhere; a sample below 8 rows is the identity with F = 0, status 8 and only padding."""
    for k in ("T", "F", "k0n", "k1n", "cfn"):
        assert getattr(out, k) is None or bool(torch.isfinite(getattr(out, k)).all()), k
    for b, n in enumerate(n_per):
        live = n if n >= 8 else 0
        for k in ("k0n", "k1n", "cfn", "inl", "pos"):
            assert not bool(getattr(out, k)[b, live:].any()), (k, b, n)  # (-0.0, NaN and the buffers' initial values all count)
            assert not bool(torch.signbit(getattr(out, k)[b, live:].float()).any()), (k, b, n)
        if n < 8:
            assert torch.equal(out.T[b], torch.eye(4)) and int(out.status[b]) == 8, (b, n)
            assert out.F is None or not bool(out.F[b].any())
        else:
            assert int(out.status[b]) == 0, (b, n, int(out.status[b]))


@pytest.mark.parametrize("closest", [False, True])
def test_ragged_batch_against_the_dense_call_and_the_oracle(gpu, closest):
    rb = _ragged_batch()
    out = _ragged_run(gpu, rb, closest=closest)
    _check_ragged_shape(out, rb.n_per)
    if not closest:  # the back-end's call: no F buffer
        noF = _ragged_run(gpu, rb, with_F=False)
        _check_ragged_shape(noF, rb.n_per)
        _same_bits(noF, out, "d_F null")
    n_margin = 0
    for b, (n, s) in enumerate(zip(rb.n_per, rb.samples)):
        if n < 8:
            continue
        one = lambda t: t[None]  # noqa: E731
        mine = _rows(out, b, n)
        # the strided reductions do not depend on the row stride: the dense call on exactly these rows gives the same bits
        _same_bits(mine, _dense(gpu, one(s.k0), one(s.k1), one(s.K0), one(s.K1), one(s.conf), closest, one(s.T)), ("dense", b, n))
        _check_inputs(mine, one(s.k0), one(s.k1), one(s.K0), one(s.K1), one(s.conf))
        r = _check_solve(mine, one(s.K0), one(s.K1), closest, one(s.T))
        n_margin += r.n_margin
        _hold(r, n, f"ragged n={n} closest={closest}")
    assert n_margin <= 0.01 * sum(n for n in rb.n_per if n >= 8), n_margin


def test_ragged_sample_does_not_depend_on_its_batch(gpu):
    rb = _ragged_batch()
    B = len(rb.n_per)
    out = _ragged_run(gpu, rb)
    rev = _ragged_run(gpu, rb, idx=list(range(B))[::-1])
    for b in range(B):
        _same_bits(_rows(out, b, RAGGED_N), _rows(rev, B - 1 - b, RAGGED_N), ("reversed", b))
        alone = _ragged_run(gpu, rb, idx=[b])
        _check_ragged_shape(alone, [rb.n_per[b]])
        _same_bits(_rows(out, b, RAGGED_N), _rows(alone, 0, RAGGED_N), ("alone", b))


# --------------------------------------------------- 4. the tuple solve against the oracle pair loop ---------------------------------------------------
@functools.lru_cache(maxsize=None)
def _tuple_scene(B, T, N, seed, one_K=False):
    """T views of N world points per sample: every image lists them in its own order on its own intrinsics (per sample too,
    unless ``one_K``: one matrix per image for the whole batch); a fifth of every image's keypoints sit 1-6 px off; a fifth of
    every pair's matches are -1."""
    rng = np.random.default_rng(seed)
    Ks = [[_intrinsics(rng, rng.uniform(400, 1100), rng.uniform(400, 1100)) for _ in range(1 if one_K else B)] for _ in range(T)]
    kp, pose, order = np.zeros((T, B, N, 2)), np.zeros((T, B, 4, 4)), np.zeros((T, B, N), np.int64)
    for b in range(B):
        Xw = np.stack([rng.uniform(-2, 2, N), rng.uniform(-2, 2, N), rng.uniform(3, 7, N)], 1)
        for t in range(T):
            Pm = np.eye(4)
            Pm[:3, :3], Pm[:3, 3] = _rodrigues(rng.normal(size=3), rng.uniform(0.1, 0.2)), rng.uniform(-0.5, 0.5, 3)
            order[t, b] = rng.permutation(N)
            x = _project(Ks[t][0 if one_K else b], Xw[order[t, b]] @ Pm[:3, :3].T + Pm[:3, 3]) + rng.normal(0, 0.5, (N, 2))
            off = rng.permutation(N)[:N // 5]
            ang, d = rng.uniform(0, 2 * np.pi, len(off)), rng.uniform(1.0, 6.0, len(off))
            x[off] += np.stack([d * np.cos(ang), d * np.sin(ang)], 1)
            kp[t, b], pose[t, b] = x, Pm
    f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))  # noqa: E731
    data, result, targets = {}, {}, {}
    for t in range(T):
        data[f"keypoints{t}"] = f32(kp[t])
        data[f"intr{t}"] = f32(np.stack(Ks[t]))
    for j in range(T):
        for i in range(j):
            m = np.zeros((B, N), np.int64)
            for b in range(B):
                where_j = np.empty(N, np.int64)
                where_j[order[j, b]] = np.arange(N)
                m[b] = where_j[order[i, b]]
                m[b, rng.permutation(N)[:N // 5]] = -1
            result[f"matches{i}_{i}_{j}"] = torch.from_numpy(m)
            result[f"conf_scores_{i}_{j}"] = f32(rng.uniform(0.1, 1.0, (B, N, 1)))
            targets[(i, j)] = f32(np.stack([pose[j, b] @ np.linalg.inv(pose[i, b]) for b in range(B)]))
    return data, result, targets


def _check_tuple(gpu, B, T, N, seed, closest, one_K):
    from oracle import w8pt as O
    data, result, targets = _tuple_scene(B, T, N, seed, one_K)
    out = _tuple(gpu, data, result, closest, targets)
    pairs = [(i, j) for j in range(T) for i in range(j)]  # j outer, i inner: the order of the reference's loops
    assert list(out) == pairs
    n_margin, dT, dF = 0, 0.0, 0.0
    for (i, j) in pairs:
        k0, k1g, Ki, Kj, conf = O.get_kpts(data, result, i, j)
        assert bool((conf[result[f"matches{i}_{i}_{j}"] < 0] == 0).all())
        o = out[(i, j)]
        _check_inputs(o, k0, k1g, Ki, Kj, conf, exact=True)  # the gather is exact, and so is the fp32 formula behind it
        r = _check_solve(o, Ki, Kj, closest, targets[(i, j)])
        assert int(o.status.abs().max()) == 0, (i, j)
        n_margin, dT, dF = n_margin + r.n_margin, max(dT, float(r.dT.max())), max(dF, float(r.dF.max()))
        bT, bF = _bars(N)
        assert float(r.dT.max()) <= bT and float(r.dF.max()) <= bF, ((i, j), float(r.dT.max()), float(r.dF.max()))
    print(f"\n[w8pt-edges] tuple T={T} closest={closest} one_K={one_K}: max|dT| = {dT:.3e}  max|dF| = {dF:.3e}  in margin = {n_margin}")
    assert n_margin <= 0.01 * len(pairs) * B * N, n_margin
    return out


TUPLE_SEEDS = {2: 42, 3: 43, 5: 45, 8: 48}


@pytest.mark.parametrize("closest", [False, True])
@pytest.mark.parametrize("T", [2, 3, 5, 8])  # 8 = E2EMV_MAX_TUPLE: 28 pairs
def test_tuple_solve_against_the_oracle_pair_loop(gpu, T, closest):
    _check_tuple(gpu, 2, T, 64, TUPLE_SEEDS[T], closest, False)


def test_tuple_solve_with_one_matrix_per_image(gpu):
    """intr_batch == 1: each image has ONE matrix for the whole batch - and still its own."""
    _check_tuple(gpu, 2, 3, 64, 143, False, True)


def test_gather_matched_with_different_keypoint_counts(gpu):
    from e2e_multi_view_matching_amd import pose as P
    from oracle import w8pt as O
    rng = np.random.default_rng(11)
    B, N0, N1 = 3, 130, 77
    data = {"keypoints0": torch.from_numpy(rng.uniform(0, 600, (B, N0, 2)).astype(np.float32)),
            "keypoints1": torch.from_numpy(rng.uniform(0, 600, (B, N1, 2)).astype(np.float32)),
            "intr0": torch.eye(4).repeat(B, 1, 1), "intr1": 2 * torch.eye(4).repeat(B, 1, 1)}
    m = rng.integers(-1, N1, (B, N0))
    m[:, :4] = [-1, 0, N1 - 1, -1]
    result = {"matches0_0_1": torch.from_numpy(m), "conf_scores_0_1": torch.from_numpy(rng.uniform(0.1, 1, (B, N0, 1)).astype(np.float32))}
    assert int((m < 0).sum()) >= 2 * B
    k0, k1g, K0, K1, conf = P.get_kpts({k: v.to(gpu) for k, v in data.items()}, {k: v.to(gpu) for k, v in result.items()}, 0, 1)
    e0, e1g, eK0, eK1, econf = O.get_kpts(data, result, 0, 1)
    assert torch.equal(k0.cpu(), e0) and torch.equal(k1g.cpu(), e1g) and torch.equal(conf.cpu(), econf)
    assert torch.equal(K0.cpu(), eK0) and torch.equal(K1.cpu(), eK1)
    assert bool((conf.cpu()[result["matches0_0_1"] < 0] == 0).all())


# ----------------------------------------------------------------- 5. status word -----------------------------------------------------------------
def test_status_word_next_to_healthy_samples(gpu):
    rng = np.random.default_rng(5)
    N = 64
    ss = [_sample(rng, N) for _ in range(6)]
    ss[1].conf[:] = 0.0                                   # all-zero confidences
    ss[3].k1[:] = torch.tensor([123.0, 77.0])             # a pair without a match: every row gathers the same point, weight 0
    ss[3].conf[:] = 0.0
    n_per = [N, N, N, N, 5, N]                            # sample 4: too few rows
    st = lambda k, idx: torch.stack([getattr(ss[b], k) for b in idx])  # noqa: E731
    run = lambda idx: _ragged(gpu, [n_per[b] for b in idx], *(st(k, idx) for k in ("k0", "k1", "K0", "K1", "conf")))  # noqa: E731
    out = run(range(6))
    status = [int(v) for v in out.status]
    assert status[0] == status[2] == status[5] == 0, status
    assert status[1] & 1 and not status[1] & 8, status
    assert status[3] & 1 and status[3] & 4 and not status[3] & 8, status
    assert status[4] == 8, status
    for k in ("T", "F", "k0n", "k1n", "cfn"):
        assert bool(torch.isfinite(getattr(out, k)).all()), k
    R = out.T[3, :3, :3].double()
    assert float((R @ R.T - torch.eye(3, dtype=torch.float64)).abs().max()) < 1e-6 and abs(float(torch.det(R)) - 1) < 1e-6
    assert abs(float(out.T[3, :3, 3].double().norm()) - 1) < 1e-6
    assert torch.equal(out.T[4], torch.eye(4)) and not bool(out.F[4].any()) and not bool(out.inl[4].any() | out.pos[4].any())
    healthy = run([0, 2, 5])
    for a, b in zip([0, 2, 5], range(3)):
        _same_bits(_rows(out, a, N), _rows(healthy, b, N), ("healthy", a))
        r = _check_solve(_rows(out, a, N), ss[a].K0[None], ss[a].K1[None], False, ss[a].T[None])
        _hold(r, N, f"status batch, healthy sample {a}")


# ------------------------------------------------- 6. pose errors and relative pose at their edges -------------------------------------------------
DELTA = 1e-6  # an fp32 sum of nine products with sum|a g| <= 3 carries at most about this much in the cosine
ROT_KINDS = ("identical", "1e-4 apart", "0.5 apart", "pi - 1e-3 apart", "trace above 3", "trace below -1")
TR_KINDS = ("parallel", "antiparallel", "orthogonal", "product just above 1e-6", "product just below 1e-6", "zero vector")


def _unit(rng):
    v = rng.normal(size=3)
    return v / np.linalg.norm(v)


def _pose_pairs(B, seed):
    """B pairs (estimate, target) in fp32; entry e takes rotation kind e % 6 and translation kind (e + e // 6) % 6, so 36
    consecutive entries hold every combination."""
    rng = np.random.default_rng(seed)
    T0, T1 = np.tile(np.eye(4), (B, 1, 1)), np.tile(np.eye(4), (B, 1, 1))
    for e in range(B):
        R0 = _rodrigues(rng.normal(size=3), rng.uniform(0, np.pi))
        rk, tk = e % 6, (e + e // 6) % 6
        angle = (0.0, 1e-4, 0.5, np.pi - 1e-3, 0.0, np.pi)[rk]
        R1 = R0 @ _rodrigues(rng.normal(size=3), angle)
        if rk >= 4:  # orthonormal to within a few fp32 ulp, but the trace of R0^T R1 lies 2e-6 to 6e-6 outside [-1, 3]: the clamp runs
            R0, R1 = R0 * (1 + 1e-6), R1 * (1 + 1e-6)
        u, v = _unit(rng), _unit(rng)
        w = np.cross(u, v)
        s = rng.uniform(0.5, 2.0)
        t0, t1 = {0: (s * u, 2.5 * s * u), 1: (s * u, -0.7 * s * u), 2: (s * u, w / np.linalg.norm(w)),
                  3: (1e-3 * u, (1e-6 + 4e-9) / 1e-3 * v), 4: (1e-3 * u, (1e-6 - 4e-9) / 1e-3 * v), 5: (0 * u, v)}[tk]
        T0[e, :3, :3], T0[e, :3, 3], T1[e, :3, :3], T1[e, :3, 3] = R0, t0, R1, t1
    return torch.from_numpy(T0.astype(np.float32)), torch.from_numpy(T1.astype(np.float32))


def _angle_bar(angle64):
    """|d angle| <= 2 delta / max(sin(angle), sqrt(2 delta)): the conditioning of arccos for an error delta in the cosine."""
    return 2 * DELTA / torch.clamp(torch.sin(angle64), min=float(np.sqrt(2 * DELTA)))


@pytest.mark.parametrize("B", [1, 63, 64, 65, 130])  # around the 64-thread block and the 64-stride mean reduction
def test_pose_errors_at_their_edges(gpu, B):
    from oracle import w8pt as O
    T0, T1 = _pose_pairs(B, 600 + B)
    A, G = T0.double(), T1.double()
    rot64 = O.compute_rotation_error(A, G, reduce=False)
    n64 = A[:, :3, 3].norm(dim=-1) * G[:, :3, 3].norm(dim=-1)
    assert not bool(((n64 - 1e-6).abs() < 1e-9).any())  # condition on the inputs: no entry inside the band around the rule
    valid64 = n64 > 1e-6
    kinds = [(e + e // 6) % 6 for e in range(B)]
    assert all(bool(valid64[e]) == (k not in (4, 5)) for e, k in enumerate(kinds))  # above / below 1e-6 sit on their sides
    assert all(abs(float(n64[e]) - 1e-6) < 1e-8 for e, k in enumerate(kinds) if k in (3, 4))
    if B >= 36:  # both clamps run in the oracle too
        tr_ = torch.einsum("bij,bij->b", A[:, :3, :3], G[:, :3, :3])
        assert bool((tr_ > 3).any()) and bool((tr_ < -1).any())
    tr64 = O.compute_translation_error_as_angle(A, G, keep_shape=True)
    rot, tr, rot_nr, tr_nr, rot_mean, tr_mean = _pose_errors(gpu, T0, T1)
    bar_r, bar_t = _angle_bar(rot64), _angle_bar(tr64)
    d_r, d_t = (rot.double() - rot64).abs(), (tr.double() - tr64).abs()
    print(f"\n[w8pt-edges] pose errors B={B}: max rot diff / bar = {float((d_r / bar_r).max()):.3f}  transl = {float((d_t / bar_t).max()):.3f}")
    assert bool((d_r <= bar_r).all()), (d_r / bar_r).max()
    assert bool((d_t <= bar_t).all()), (d_t / bar_t).max()
    assert bool((tr[~valid64] == 0).all())
    # reduce=False: [B] rotations, exactly the valid translations (the shape of the reference's boolean indexing)
    assert torch.equal(rot_nr, rot)
    assert tr_nr.shape == O.compute_translation_error_as_angle(A, G, reduce=False).shape and torch.equal(tr_nr, tr[valid64])
    # means: rotation over all entries, translation over the valid ones; per-entry bars averaged, plus the fp32 reduction (at
    # most 3 strided additions and 6 shuffle steps deep, one division: 10 roundings of 2^-24 relative to the mean of magnitudes)
    red = 10 * 2.0 ** -24
    m_r, m_t = O.compute_rotation_error(A, G), O.compute_translation_error_as_angle(A, G)
    assert abs(float(rot_mean) - float(m_r)) <= float(bar_r.mean()) + red * float(m_r)
    if bool(valid64.any()):
        assert abs(float(tr_mean) - float(m_t)) <= float(bar_t[valid64].mean()) + red * float(m_t)
    else:
        assert bool(torch.isnan(tr_mean)) and bool(torch.isnan(m_t))
    # no valid entry at all: NaN like the reference's mean of nothing
    Z = T0.clone()
    Z[:, :3, 3] = 0
    out0 = _pose_errors(gpu, Z, T1)
    assert bool(torch.isnan(out0[5])) and out0[3].shape == (0,) and not bool(out0[1].any())
    assert abs(float(out0[4]) - float(m_r)) <= float(bar_r.mean()) + red * float(m_r)


def _rotation_group():
    """The 24 rotations by multiples of 90 degrees about the axes: signed permutation matrices of determinant +1."""
    out = []
    for perm in itertools.permutations(range(3)):
        for signs in itertools.product((1.0, -1.0), repeat=3):
            M = np.zeros((3, 3))
            M[range(3), perm] = signs
            if np.linalg.det(M) > 0:
                out.append(M)
    return out


def test_relative_pose_pivots(gpu):
    """pose_b = quarter and half turns about the axes and their compositions (the diagonal starts at 0: the pivot search must
    swap rows), the same followed by a small rotation (a diagonal of a few 1e-2: no division by zero, but an unpivoted
    elimination loses digits), and small rotations.  The kernel eliminates in fp64 and rounds once: 2 fp32 ulp of the largest
    entry of the row."""
    rng = np.random.default_rng(7)
    group = _rotation_group()
    assert len(group) == 24 and sum(1 for M in group if M[0, 0] == 0) >= 12
    Rb = group + [M @ _rodrigues(rng.normal(size=3), 0.05) for M in group] + [_rodrigues(rng.normal(size=3), 0.1) for _ in range(17)]
    B = len(Rb)  # 65: two blocks of 64
    pa, pb = np.tile(np.eye(4), (B, 1, 1)), np.tile(np.eye(4), (B, 1, 1))
    for e in range(B):
        pb[e, :3, :3], pb[e, :3, 3] = Rb[e], rng.uniform(-3, 3, 3)
        pa[e, :3, :3], pa[e, :3, 3] = _rodrigues(rng.normal(size=3), rng.uniform(0, 0.3)), rng.uniform(-3, 3, 3)
    pa, pb = torch.from_numpy(pa.astype(np.float32)), torch.from_numpy(pb.astype(np.float32))
    ref = torch.linalg.inv(pb.double()) @ pa.double()
    got = _relative_pose(gpu, pa, pb)
    bar = 2 * _ulp32(ref.abs().amax(-1, keepdim=True))
    d = (got.double() - ref).abs()
    print(f"\n[w8pt-edges] relative pose: max diff / bar = {float((d / bar).max()):.3f}")
    assert bool((d <= bar).all()), float((d / bar).max())
