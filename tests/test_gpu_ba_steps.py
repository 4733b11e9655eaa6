"""Two-view bundle adjustment, every LM step against the fp64 oracle at the sizes where the kernel changes path
(csrc/ba2view.hip: ba2view_kernel, small_linalg.h: triangulate_xyz).

One workgroup runs the whole Levenberg-Marquardt loop of a pair: three passes over the matches in 256-wide strides, the
point blocks eliminated through a Schur complement, a 6x6 solve on one lane, the reference's lambda / best-pose
bookkeeping.  oracle/ba2view.py builds the dense normal equations of the same problem in fp64 and records, for every
residual evaluation, the best pose so far: ONE 10-iteration run is the expected result of every n_iterations <= 10.

The bar has no term measured on the kernel.  Kernel and oracle share the algorithm and fp64; the one freedom they
legitimately have is the sign of the DLT null vector of the triangulation, which `1 / (w + 1e-8)` turns into a relative
~1e-8 / |w| difference of the start points.  The oracle is run with that sign forced to + (T+) and to - (T-) for all
points; delta(n) = max |T+(n) - T-(n)| brackets what the freedom is worth after n iterations (per-point sign patterns
stay inside the all-plus / all-minus pair) and the device has to be within

    |T - (T+(n) + T-(n)) / 2|  <=  2^-23 max(1, |T|)  +  4 delta(n)         elementwise,

fp32 rounding of the output plus four brackets, because the kernel's per-point signs are unknown.  The ungated premise
test keeps the bar honest wherever the suite runs: both oracle runs take the same accept / reject decisions, none of
them on a tie, delta stays below 5e-7 (1e-4 for the outlier scene at 10 iterations), and the two hard scenes really
contain rejected steps followed by accepted ones."""
import functools

import numpy as np
import pytest
import torch

N_MAX = 10
N_ITERS = [0, 1, 2, 3, 5, 10]
EPS32 = 2.0 ** -23
DELTA_CAP = 5e-7        # ~4x the sign bracket the oracle shows on clean scenes (<= 1.2e-7)
DELTA_CAP_J10 = 1e-4    # outlier scene at 10 iterations: keeps the bar from becoming vacuous, not a tolerance
TIE_GAP = 1e-6          # relative gap every rn-against-best_r comparison must have


def _rodrigues(w):
    th = np.linalg.norm(w)
    if th == 0.0:
        return np.eye(3)
    k = w / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


def _unit(rng):
    v = rng.normal(size=3)
    return v / np.linalg.norm(v)


def make_scene(N, seed, rot_pert=0.06, t_pert=0.1, noise=0.0, outliers=0.0):
    """Normalised coordinates, fp32: points at depth 3..8 in front of both cameras, a known pose and a perturbed copy of it
    as T_init, confidences in (0.1, 1].  -> dict(k0 [1,N,2], k1 [1,N,2], conf [1,N], T_init [1,4,4], T_true [4,4])."""
    rng = np.random.default_rng(seed)
    R = _rodrigues(_unit(rng) * rng.uniform(0.1, 0.25))
    t = np.array([1.0, 0.0, 0.0]) + rng.uniform(-0.2, 0.2, 3)
    z = rng.uniform(3.0, 8.0, N)
    X = np.stack([z * rng.uniform(-0.35, 0.35, N), z * rng.uniform(-0.35, 0.35, N), z], -1)
    Y = X @ R.T + t
    assert Y[:, 2].min() > 2.0
    k0 = X[:, :2] / X[:, 2:] + noise * rng.normal(size=(N, 2))
    k1 = Y[:, :2] / Y[:, 2:] + noise * rng.normal(size=(N, 2))
    if outliers > 0:
        bad = rng.choice(N, size=int(round(outliers * N)), replace=False)
        k1[bad] = rng.uniform(-0.4, 0.4, (len(bad), 2))
    conf = rng.uniform(0.1, 1.0, N)
    conf = 1.1 - conf  # (0.1, 1]
    T_true, T_init = np.eye(4), np.eye(4)
    T_true[:3, :3], T_true[:3, 3] = R, t
    T_init[:3, :3] = _rodrigues(_unit(rng) * rot_pert) @ R
    T_init[:3, 3] = t + t_pert * _unit(rng)
    f = lambda a: torch.from_numpy(np.ascontiguousarray(a).astype(np.float32))
    return {"k0": f(k0)[None], "k1": f(k1)[None], "conf": f(conf)[None], "T_init": f(T_init)[None], "T_true": f(T_true)}


def _mask_rows(s, keep, seed, garbage=False):
    """Every row outside `keep` is masked: confidence 0 - or, with `garbage`, a confidence from {0, -0.0, -1, NaN} and
    coordinates from {NaN, +inf, -inf, 1e30}: nothing of such a row may reach a sum."""
    rng = np.random.default_rng(seed)
    N = s["conf"].shape[1]
    off = np.setdiff1d(np.arange(N), keep)
    s["conf"][0, off] = 0.0
    if garbage:
        s["conf"][0, off] = torch.tensor([0.0, -0.0, -1.0, float("nan")])[rng.integers(0, 4, len(off))]
        bad = torch.tensor([float("nan"), float("inf"), float("-inf"), 1e30])
        for k in ("k0", "k1"):
            s[k][0, off] = bad[rng.integers(0, 4, (len(off), 2))]
    s["keep"] = torch.from_numpy(np.sort(keep))
    return s


def _scale_conf(s, total):
    """Confidences rescaled to sum to (about) `total`; stays fp32."""
    s["conf"] = (s["conf"].double() * (total / float(s["conf"].double().sum()))).float()
    return s


def _scattered(N, n, seed):
    return np.random.default_rng(seed).choice(N, size=n, replace=False)


# name -> scene builder.  Seeds are chosen so that the premise test holds (see there); the sizes are the kernel's paths.
# Scenes a to i are clean (no keypoint noise beyond fp32 rounding): the residual keeps falling for all 10 iterations and no
# comparison comes near a tie; on a noisy scene LM reaches the noise floor first and compares equal residuals.
# g: the last stride trip of N = 1024 has 256 rows, so "every valid row at index >= 768" means those 256.
CASES = {
    "a_n7": lambda: make_scene(7, 101),                                                    # smallest valid problem
    "b_n8_hole0": lambda: _mask_rows(make_scene(8, 102), np.arange(1, 8), 0),               # "> 6" rule, hole in front
    "c_n65": lambda: make_scene(65, 103),                                                  # one row in the second wave
    "d_n256": lambda: make_scene(256, 104),                                                # exactly one stride
    "e_n257": lambda: make_scene(257, 105),                                                # first row of the second trip
    "f_n300_garbage": lambda: _mask_rows(make_scene(300, 106), _scattered(300, 90, 6), 60, garbage=True),
    "g_n1024_tail": lambda: _mask_rows(make_scene(1024, 107), np.arange(768, 1024), 0),     # only the last stride trip works
    "h_n2048": lambda: _mask_rows(make_scene(2048, 108), _scattered(2048, 520, 8), 0),      # the back-end's largest row stride
    "i_n90_far": lambda: make_scene(90, 109, rot_pert=0.65, t_pert=0.3),        # rejected steps
    "j_n257_outliers": lambda: make_scene(257, 118, rot_pert=0.03, t_pert=0.05, noise=3e-4, outliers=0.10),                        # rejected steps, hard problem
    # confidence normalisation inside the max(2 sum c, 1e-6) clamp: the weights then sum to less than one.  "deep": so far
    # inside that the Jacobi preconditioner's 1e-12 floor of the diagonal takes over as well
    "k_n65_clamp": lambda: _scale_conf(make_scene(65, 103), 2e-7),
    "l_n65_clamp_deep": lambda: _scale_conf(make_scene(65, 103), 1e-10),
}
PARITY_CASES = [c for c in CASES if c[0] <= "j"]
CLAMP_CASES = [c for c in CASES if c[0] > "j"]


@functools.lru_cache(maxsize=None)
def scene(name):
    return CASES[name]()


def _oracle(s, sign, n=N_MAX):
    from oracle import ba2view as OB
    _, valid, traj = OB.run_bundle_adjust_2_view(s["k0"].double(), s["k1"].double(), s["conf"].double(), s["T_init"].double(), n,
                                                 homogeneous_sign=sign, return_trajectory=True)
    assert bool(valid.all())
    return traj[0]


@functools.lru_cache(maxsize=None)
def trajectories(name):
    """(T+ trajectory, T- trajectory) of a case: two 10-iteration oracle runs, shared by every test, never modified."""
    s = scene(name)
    return _oracle(s, +1), _oracle(s, -1)


def _delta(tp, tm, n):
    return float((tp["best"][n] - tm["best"][n]).abs().max())


def _pattern(tr):
    return "".join("A" if a else "r" for a in tr["accepted"][1:].tolist())


def _device(gpu, s, n, rows=None):
    import e2e_multi_view_matching_amd as E
    k0, k1, c = s["k0"], s["k1"], s["conf"]
    if rows is not None:
        k0, k1, c = k0[:, rows], k1[:, rows], c[:, rows]
    T, valid = E.run_bundle_adjust_2_view(k0.to(gpu), k1.to(gpu), c.to(gpu), s["T_init"].to(gpu), n_iterations=n)
    return T.cpu(), valid.cpu()


def _check_parity(gpu, name, rows=None):
    """The device at every n of N_ITERS against the midpoint of the two oracle trajectories; returns the outputs by n."""
    s = scene(name)
    tp, tm = trajectories(name)
    out = {}
    for n in N_ITERS:
        T, valid = _device(gpu, s, n, rows)
        assert valid.tolist() == [True], (name, n)
        assert T.dtype == torch.float32 and T.shape == (1, 4, 4)
        out[n] = T
        if n == 0:
            assert torch.equal(T, s["T_init"]), (name, "n_iterations = 0 must return T_init bit for bit")
            continue
        T = T[0].double()
        mid = 0.5 * (tp["best"][n] + tm["best"][n])
        delta = _delta(tp, tm, n)
        bar = EPS32 * T.abs().clamp(min=1.0) + 4.0 * delta
        dist = (T - mid).abs()
        print(f"{name} n={n}: |T - mid| = {float(dist.max()):.3e}  delta = {delta:.3e}  bar = {float(bar.min()):.3e}  [{_pattern(tp)[:n]}]")
        assert bool(T.isfinite().all()), (name, n)
        assert bool((dist <= bar).all()), (name, n, float(dist.max()), float(bar.min()), delta)
    return out


# ------------------------------------------------------------------------------------------------ premises (CPU)


@pytest.mark.parametrize("name", list(CASES))
def test_premise_sign_bracket_is_tight_and_no_decision_on_a_tie(name):
    """What the device bar rests on, checked wherever the suite runs."""
    s = scene(name)
    tp, tm = trajectories(name)
    n_valid = int((s["conf"] > 0).sum())
    print(f"{name}: N={s['conf'].shape[1]} valid={n_valid} pattern {_pattern(tp)}  delta(1,3,10) = "
          f"{_delta(tp, tm, 1):.2e} {_delta(tp, tm, 3):.2e} {_delta(tp, tm, 10):.2e}")
    # 1. the same decisions under either sign
    assert _pattern(tp) == _pattern(tm), (name, _pattern(tp), _pattern(tm))
    # 2. none of them on a tie
    for tr in (tp, tm):
        gap = ((tr["rn"][1:] - tr["best_r"][1:]).abs() / tr["best_r"][1:].abs())
        assert bool(tr["rn"].isfinite().all()) and float(gap.min()) >= TIE_GAP, (name, gap.tolist())
    # 3. the bracket is tight
    for n in range(1, N_MAX + 1):
        cap = DELTA_CAP if (n <= 3 or not name.startswith("j_")) else DELTA_CAP_J10
        if n <= 3 or n == N_MAX:
            assert _delta(tp, tm, n) <= cap, (name, n, _delta(tp, tm, n))
    assert _delta(tp, tm, 0) == 0.0 and torch.equal(tp["best"][0], s["T_init"][0].double())
    # 4. the hard scenes reject steps, and accept again after a rejection
    if name[0] in "ij":
        p = _pattern(tp)
        assert p.count("r") >= 2 and p.count("A") >= 2 and "rA" in p, (name, p)
    # what the scene is meant to hold
    if name.startswith("f_"):
        off = torch.ones(300, dtype=torch.bool)
        off[s["keep"]] = False
        c, k = s["conf"][0, off], torch.cat([s["k0"][0, off], s["k1"][0, off]], 1)
        assert n_valid == 90 and bool(c.isnan().any()) and bool((c == -1).any()) and bool(torch.signbit(c[c == 0]).any())
        assert bool((k[k.isfinite()] == torch.tensor(1e30)).all())
        assert bool(k.isnan().any()) and bool((k == float("inf")).any()) and bool((k == float("-inf")).any())
    if name.startswith("g_"):
        assert n_valid == 256 and int(s["keep"].min()) == 768
    if name.startswith("h_"):
        assert n_valid == 520
    if name.startswith("b_"):
        assert n_valid == 7 and float(s["conf"][0, 0]) == 0.0
    if name.startswith("k_") or name.startswith("l_"):
        assert float(s["conf"].double().sum()) < 5e-7


def test_premise_trajectory_is_a_prefix_and_defaults_are_unchanged():
    """best[n] of one 10-iteration run IS the result of n_iterations = n; without the hooks the oracle returns what it did."""
    from oracle import ba2view as OB
    s = scene("c_n65")
    a = [t.double() for t in (s["k0"], s["k1"], s["conf"], s["T_init"])]
    tp, _ = trajectories("c_n65")
    for n in (0, 2, 5):
        T, _, tr = OB.run_bundle_adjust_2_view(*a, n, homogeneous_sign=+1, return_trajectory=True)
        assert torch.equal(T[0], tp["best"][n]) and torch.equal(tr[0]["best"], tp["best"][:n + 1])
        assert torch.equal(tr[0]["rn"], tp["rn"][:n + 1]) and torch.equal(tr[0]["accepted"], tp["accepted"][:n + 1])
    # without the hooks: the two values of before, and the SVD's own signs decide the same way
    T, valid = OB.run_bundle_adjust_2_view(*a, 3)
    T3, valid3, tr = OB.run_bundle_adjust_2_view(*a, 3, return_trajectory=True)
    assert valid.tolist() == [True] and torch.equal(T, T3) and torch.equal(T[0], tr[0]["best"][3])
    assert _pattern(tr[0]) == _pattern(tp)[:3]


DEGENERATE = {
    # t = 0: both cameras share a centre, every pair of rays is parallel or identical, no depth is defined
    "pure_rotation": lambda: dict(make_scene(40, 201), T_init=_pure_rotation(make_scene(40, 201)["T_init"])),
    # identical keypoints under R = I: the rays of every match are parallel, the points start at infinity
    "same_kpts": lambda: _same_kpts(make_scene(40, 202)),
}


def _pure_rotation(T):
    T = T.clone()
    T[:, :3, 3] = 0.0
    return T


def _same_kpts(s):
    s["k1"] = s["k0"].clone()
    T = torch.eye(4)[None].clone()
    T[0, :3, 3] = s["T_init"][0, :3, 3]
    s["T_init"] = T
    return s


@pytest.mark.parametrize("name", list(DEGENERATE))
def test_premise_oracle_stays_finite_on_degenerate_starts(name):
    s = DEGENERATE[name]()
    for sign in (+1, -1):
        tr = _oracle(s, sign)
        assert bool(tr["best"].isfinite().all()), (name, sign)


# ------------------------------------------------------------------------------------------------ device


@pytest.mark.gpu
@pytest.mark.parametrize("name", PARITY_CASES)
def test_every_lm_step_matches_the_oracle(gpu, name):
    _check_parity(gpu, name)


@pytest.mark.gpu
def test_masked_rows_do_not_leak(gpu):
    """Case f: 210 of 300 rows are masked by 0 / -0.0 / -1 / NaN confidences and hold NaN / inf / 1e30 coordinates.  The
    result is that of the 90 valid rows alone (N = 90), both within the bar of the oracle, and finite."""
    name = "f_n300_garbage"
    s = scene(name)
    tp, tm = trajectories(name)
    full = _check_parity(gpu, name)
    compact = _check_parity(gpu, name, rows=s["keep"])
    for n in N_ITERS[1:]:
        a, b = full[n][0].double(), compact[n][0].double()
        assert bool(a.isfinite().all()) and bool(b.isfinite().all())
        bar = EPS32 * a.abs().clamp(min=1.0) + 4.0 * _delta(tp, tm, n)
        assert bool(((a - b).abs() <= bar).all()), (n, float((a - b).abs().max()))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["c_n65", "f_n300_garbage", "e_n257"])
def test_confidence_scale_by_a_power_of_two_changes_no_bit(gpu, name):
    """c / max(2 sum c, 1e-6): a power-of-two factor on every confidence is exact and cancels while the sum stays above the clamp."""
    s = scene(name)
    for n in (1, 10):
        T, _ = _device(gpu, s, n)
        for f in (2.0 ** 20, 2.0 ** -20):
            s2 = dict(s, conf=s["conf"] * f)
            assert float(s2["conf"][s2["conf"] > 0].double().sum()) > 5e-7
            T2, v2 = _device(gpu, s2, n)
            assert v2.tolist() == [True] and torch.equal(T, T2), (name, n, f, float((T - T2).abs().max()))


@pytest.mark.gpu
@pytest.mark.parametrize("name", CLAMP_CASES)
def test_confidence_normalisation_clamp_matches_the_oracle(gpu, name):
    _check_parity(gpu, name)


@pytest.mark.gpu
def test_batch_position_independence_and_repeatability(gpu):
    """B = 5 at N = 300: [A, six positive confidences, B, all zero, A].  Each pose is the bits of the sample run alone."""
    import e2e_multi_view_matching_amd as E
    A, Bs = scene("f_n300_garbage"), make_scene(300, 301)
    six = make_scene(300, 302)
    six["conf"][0, np.setdiff1d(np.arange(300), [0, 17, 255, 256, 257, 299])] = 0.0
    assert int((six["conf"] > 0).sum()) == 6
    zero = make_scene(300, 303)
    zero["conf"][:] = 0.0
    batch = [A, six, Bs, zero, A]
    cat = lambda k: torch.cat([s[k] for s in batch]).to(gpu)
    for n in (3, 10):
        T, valid = E.run_bundle_adjust_2_view(cat("k0"), cat("k1"), cat("conf"), cat("T_init"), n_iterations=n)
        T_again, valid_again = E.run_bundle_adjust_2_view(cat("k0"), cat("k1"), cat("conf"), cat("T_init"), n_iterations=n)
        assert valid.tolist() == [True, False, True, False, True] and T.shape == (3, 4, 4)
        assert torch.equal(T, T_again) and torch.equal(valid, valid_again)
        assert torch.equal(T[0], T[2])
        assert bool(T.isfinite().all())
        for i, s in ((0, A), (1, Bs), (2, A)):
            alone, v = _device(gpu, s, n)
            assert v.tolist() == [True] and torch.equal(alone[0], T[i].cpu()), (n, i)
        for s in (six, zero):
            alone, v = _device(gpu, s, n)
            assert v.tolist() == [False] and alone.shape == (0, 4, 4)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(DEGENERATE))
def test_degenerate_starts_stay_finite(gpu, name):
    """No parity here - the sign freedom decides on which side of the cameras the points start - but the best-pose rule (a
    NaN residual never compares below the best) keeps every output finite and a rigid motion."""
    s = DEGENERATE[name]()
    for n in (1, 3, 10):
        T, valid = _device(gpu, s, n)
        assert valid.tolist() == [True]
        assert bool(T.isfinite().all()), (name, n)
        R = T[0, :3, :3].double()
        assert float((R @ R.T - torch.eye(3, dtype=torch.float64)).abs().max()) <= 1e-6, (name, n)
        assert torch.equal(T[0, 3], torch.tensor([0.0, 0.0, 0.0, 1.0]))
