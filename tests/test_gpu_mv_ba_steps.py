"""Multi-view bundle adjustment, every LM step, every termination and the index edges of mvba_kernel (csrc/mvba.hip) against
the fp64 oracle (oracle/mvba.py).

One workgroup runs the whole Levenberg-Marquardt loop of a problem.  The oracle records its state after every pass through
the loop: ONE 50-iteration run is the expected result of every max_iterations <= 50 (proved below on the CPU), so the device
is looked at after k = 0, 1, 2, ... steps and a wrong accept that a later step repairs does not hide behind the end result.

The bar has no term measured on the kernel.  Kernel and oracle share the algorithm and fp64; what they legitimately differ in
is where they round.  The oracle is therefore run once as it is and once per variant of oracle.mvba.VARIANTS: observations
reversed / shuffled, points relabelled (the order of every sum); the point blocks inverted by the kernel's adjugate, by Cholesky
factors as Ceres does, or in extended precision; the Schur products associated to the right; the reduced system solved in the
kernel's order; rotation matrices and their derivative written out as the kernel does; the projection by the reference's division;
residuals and Jacobians in extended precision; and the WHOLE algorithm in extended precision, rounded to fp64 - against that run
the default one shows the reference's own error.  Re-ordered sums and another inverse alone share most of their roundings and
bracket too little: with only those four, the device's cost after step 1 of intrinsics_aniso sat 7.8 delta from mid.  That step
redone in long double has the default run's cost a relative 1.7e-11 below the exact one, every fp64 variant between 0.9e-11 and
2.9e-11 below it, and the device 4.5e-11 above: as accurate as the oracle, outside its cluster.  diff(k) is the largest elementwise difference between the default run and any variant after k steps, delta(k) its
running maximum over k' <= k, separately for cameras, points and (relative) cost, and the device has to be within

    |gpu - mid(k)|  <=  4 delta(k)        elementwise, mid = midpoint of the default run and the farthest variant,

the factor test_gpu_ba_steps.py uses for the same purpose.  Before the first accepted step the state is the input: cameras and
points come back bit for bit, final_cost is the bits of the device's own initial_cost, and that number keeps the 1e-10 relative
bar it has in test_mv_ba.py (the variants there only re-sum the same residuals: their costs differ by 0 to 2 ulp, which says
nothing about evaluating a residual with fused multiply-adds).  iterations and termination are compared exactly at every k.  The ungated premise tests keep that honest
wherever the suite runs: no decision of any oracle run sits within a relative 1e-3 of its threshold, all variants decide alike,
delta stays below 1e-8 (ten times under the project's end-of-run bar) for every scene up to k = 10 and for at least three
quarters of all (scene, k) pairs, and every scene really contains the case it is named after.

The "radius" termination is not here: it needs about 15 consecutive non-invalid rejections and no probed scene gets there."""
import functools

import numpy as np
import pytest

from oracle import mvba

KS = [0, 1, 2, 3, 4, 5, 6, 8, 10, 15, 20, 30, 50]
K_MAX = 50
FACTOR = 4.0
CHAOS_CAP = 1e-8    # delta of cameras and points beyond which only the decisions are compared
KNIFE = 1e-3        # relative distance every decision quantity keeps from its threshold
THRESHOLDS = {"rho": 1e-3, "fn_ratio": 1e-6, "step_ratio": 1e-8, "gmax": 1e-10}
EPS = float(np.finfo(float).eps)


def make_scene(seed, C=5, P=40, fixed=0, views=2, intr=(1.0, 1.0, 0.0, 0.0), aniso=False, perturb=0.03, noise=2e-3, wscale=1.0,
               rot_sigma=0.25):
    """A problem in the oracle's dict form: true cameras near the identity looking at points 4..8 in front of them, every
    point seen by `views` distinct cameras, a start perturbed by `perturb`.  The fixed camera is the identity in truth (its
    observations are predicted so) while its stored row is arbitrary; fixed = -1 frees every camera."""
    rng = np.random.default_rng(seed)
    cams = np.concatenate([rng.normal(0, rot_sigma, (C, 3)), rng.normal(0, 0.4, (C, 3))], 1)
    if fixed >= 0:
        cams[fixed] = 0.0
    pts = np.stack([rng.uniform(-2, 2, P), rng.uniform(-2, 2, P), rng.uniform(4, 8, P)], 1)
    ci = np.concatenate([rng.choice(C, size=views, replace=False) for _ in range(P)]).astype(np.int32)
    pi = np.repeat(np.arange(P), views).astype(np.int32)
    prob = _observe(rng, cams, pts, ci, pi, fixed, intr, aniso, noise, wscale)
    start = cams + rng.normal(0, perturb, (C, 6))
    if fixed >= 0:
        start[fixed] = rng.normal(0, 0.3, 6) if fixed > 0 else 0.0  # a stored row that is NOT the pose the solver uses
    prob["cams"], prob["pts"] = start, pts + rng.normal(0, perturb, pts.shape)
    return prob


def _observe(rng, cams, pts, ci, pi, fixed, intr, aniso, noise, wscale):
    fx, fy, cx, cy = intr
    q = np.stack([mvba.aa_to_R(cams[c, :3]) @ pts[p] + cams[c, 3:] for c, p in zip(ci, pi)])
    assert q[:, 2].min() > 1.0
    obs = np.stack([fx * q[:, 0] / q[:, 2] + cx, fy * q[:, 1] / q[:, 2] + cy], 1) + noise * rng.normal(size=(len(ci), 2))
    w = rng.uniform(0.2, 2.0, (len(ci), 2))
    if not aniso:
        w[:, 1] = w[:, 0]
    return dict(n_cams=len(cams), fixed=fixed, intr=np.array(intr, float), cam_idx=ci, pt_idx=pi, obs=obs, wts=w * wscale)


def _with(prob, **kw):
    out = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in prob.items()}
    for k, f in kw.items():
        out[k] = f(out[k])
    return out


def _nan_obs(prob):
    prob = _with(prob)
    o = int(np.flatnonzero(prob["cam_idx"] != prob["fixed"])[3])
    prob["obs"][o, 0] = np.nan
    return prob


def _small_rotation(seed):
    """Cameras 1, 2, 3 are free and start at w = 0, (1e-8, 0, 0) (|w|^2 <= eps: first-order branch) and (2e-8, 0, 0)
    (|w|^2 > eps: Rodrigues); their true rotations are small but well outside that range."""
    prob = make_scene(seed, C=4, P=40, rot_sigma=0.03)
    prob["cams"][1, :3] = 0.0
    prob["cams"][2, :3] = (1e-8, 0.0, 0.0)
    prob["cams"][3, :3] = (2e-8, 0.0, 0.0)
    return prob


STRIDE_COUNTS = {1: 0, 2: 1, 3: 64, 4: 65}  # camera -> length of its observation list (the wave's 64-lane stride)


def _strides(seed, P):
    """C = 8, two views per point and one observation more, O = 2 P + 1: cameras 1..4 have exactly 0, 1, 64 and 65
    observations, cameras 0 (fixed), 5, 6, 7 share the rest, and point 201 is seen twice by camera 5.  (Eight cameras because
    four lists of 0, 1, 64 and 65 observations cannot hold the observations of 513 points.)"""
    rng = np.random.default_rng(seed)
    C, big = 8, [0, 5, 6, 7]
    cams = np.concatenate([rng.normal(0, 0.25, (C, 3)), rng.normal(0, 0.4, (C, 3))], 1)
    cams[0] = 0.0
    pts = np.stack([rng.uniform(-2, 2, P), rng.uniform(-2, 2, P), rng.uniform(4, 8, P)], 1)
    second = [c for c, n in STRIDE_COUNTS.items() for _ in range(n)]
    ci, pi = [], []
    for p in range(P):
        a = big[p % 4]
        b = second[p] if p < len(second) else big[(p + 1 + p // 4 % 3) % 4]
        assert a != b
        ci += [a, b]; pi += [p, p]
    ci.append(ci[2 * 201]); pi.append(201)  # camera 5 (free) sees point 201 again (another noisy observation of it)
    ci, pi = np.array(ci, np.int32), np.array(pi, np.int32)
    order = rng.permutation(len(ci))         # observation lists are not sorted by point or camera
    prob = _observe(rng, cams, pts, ci[order], pi[order], 0, (1.0, 1.0, 0.0, 0.0), False, 2e-3, 1.0)
    start = cams + rng.normal(0, 0.03, (C, 6))
    start[0] = 0.0
    prob["cams"], prob["pts"] = start, pts + rng.normal(0, 0.03, pts.shape)
    return prob


# name -> builder.  Seeds are chosen so that the premise tests hold (see there), never by what the device returns.
SCENES = {
    "minimal": lambda: make_scene(11, C=2, P=7),                                       # smallest problem that still iterates
    "fixed_mid": lambda: make_scene(12, C=5, P=40, fixed=2),                           # maps s_fidx / s_free around camera 2
    "fixed_last_dense": lambda: make_scene(13, C=8, P=24, fixed=7, views=8),           # every point seen by all 8 cameras
    "no_fixed": lambda: make_scene(14, C=8, P=40, fixed=-1, views=3),                  # F = 8, n = 48, 36 blocks on 8 waves
    "intrinsics_aniso": lambda: make_scene(15, C=5, P=40, intr=(1.3, 0.8, 0.05, -0.03), aniso=True),
    "far_start": lambda: make_scene(24, C=5, P=40, perturb=0.24),                      # rejected steps, two in a row
    "exact": lambda: make_scene(17, C=5, P=40, noise=0.0),                             # gradient_tolerance
    "exact_heavy": lambda: make_scene(17, C=5, P=40, noise=0.0, wscale=100.0),         # parameter_tolerance
    "nan_obs": lambda: _nan_obs(make_scene(18, C=5, P=40)),                            # invalid_steps at iteration 5
    "small_rotation": lambda: _small_rotation(19),
    "strides_p513": lambda: _strides(21, 513),                                         # P = 513, O = 1027
    "strides_p512": lambda: _strides(21, 512),                                         # P = 512, O = 1025
    "strides_o513": lambda: _strides(21, 256),                                         # P = 256, O = 513
}


@functools.lru_cache(maxsize=None)
def scene(name):
    return SCENES[name]()


@functools.lru_cache(maxsize=None)
def trajectories(name):
    """{"default": trajectory, variant: trajectory, ...} of a scene: five 50-iteration oracle runs, shared by every test, never
    modified."""
    p = scene(name)
    out = {"default": mvba.solve(p, max_iterations=K_MAX, return_trajectory=True)[3]}
    for v in mvba.VARIANTS:
        out[v] = mvba.solve_variant(p, v, seed=1, max_iterations=K_MAX, return_trajectory=True)[3]
    return out


def _at(traj, k):
    """Record k of a trajectory = what max_iterations = k returns; a run that ended earlier stays at its last record."""
    return traj[min(k, len(traj) - 1)]


def _diff(a, b, key):
    """Largest elementwise difference of two records; the cost relative; NaN against NaN is no difference."""
    x, y = np.asarray(a[key], float), np.asarray(b[key], float)
    d = np.abs(x - y) / (np.abs(x) if key == "cost" else 1.0)
    d = np.where(np.isnan(x) & np.isnan(y), 0.0, d)
    d = np.where((x == y), 0.0, d)
    return float(d.max())


@functools.lru_cache(maxsize=None)
def bracket(name):
    """Per k of 0..50: delta[key][k] (running maximum of the largest default-to-variant difference) and far[key][k], the
    variant farthest from the default at k, for key in cams / pts / cost."""
    tr = trajectories(name)
    delta, far = {}, {}
    for key in ("cams", "pts", "cost"):
        d = np.array([[_diff(_at(tr["default"], k), _at(tr[v], k), key) for v in mvba.VARIANTS] for k in range(K_MAX + 1)])
        delta[key] = np.maximum.accumulate(d.max(1))
        far[key] = [mvba.VARIANTS[i] for i in d.argmax(1)]
    return delta, far


def _pattern(traj):
    return "".join({"accepted": "A", "rejected": "r", "invalid": "i", "stop": "."}[r["kind"]] for r in traj[1:])


def _decisions(traj):
    return [(r["kind"], r["iterations"], r["termination"]) for r in traj]


def _inside_cap(name, k):
    delta, _ = bracket(name)
    return delta["cams"][k] <= CHAOS_CAP and delta["pts"][k] <= CHAOS_CAP


def _variants_agree(name, k):
    tr = trajectories(name)
    return len({(_at(t, k)["iterations"], _at(t, k)["termination"]) for t in tr.values()}) == 1


# ------------------------------------------------------------------------------------------------ premises (CPU)


@pytest.mark.parametrize("name", ["far_start", "exact_heavy"])
def test_premise_record_k_is_the_run_truncated_at_k(name):
    """solve(p, max_iterations=k) is record k of one 50-iteration run, bit for bit, for every k - and the hooks change nothing."""
    p = scene(name)
    traj = trajectories(name)["default"]
    assert 2 <= len(traj) <= K_MAX + 1
    for k in range(K_MAX + 1):
        cams, pts, summary = mvba.solve(p, max_iterations=k)
        r = _at(traj, k)
        assert np.array_equal(cams, r["cams"]) and np.array_equal(pts, r["pts"]), (name, k)
        assert summary["final_cost"] == r["cost"] and summary["iterations"] == r["iterations"] == min(k, len(traj) - 1), (name, k)
        assert summary["termination"] == r["termination"], (name, k, summary, r["termination"])
        assert summary["initial_cost"] == traj[0]["cost"]
    assert [r["termination"] for r in traj[:-1]] == ["max_iterations"] * (len(traj) - 1)
    # a variant's trajectory has the same property (its records come back in the scene's own labelling)
    for v in mvba.VARIANTS:
        tv = trajectories(name)[v]
        for k in (0, 3, len(tv) - 1):
            cams, pts, summary = mvba.solve_variant(p, v, seed=1, max_iterations=k)
            assert np.array_equal(cams, tv[k]["cams"]) and np.array_equal(pts, tv[k]["pts"]) and summary["final_cost"] == tv[k]["cost"]


@pytest.mark.parametrize("name", list(SCENES))
def test_premise_no_knife_edges_and_bracket_under_the_cap(name):
    """What the device bar rests on, checked on the reference alone."""
    tr = trajectories(name)
    delta, _ = bracket(name)
    print(f"{name}: [{_pattern(tr['default'])}] {tr['default'][-1]['termination']}  delta cams/pts at k=1,5,10,50: " +
          " ".join(f"{delta['cams'][k]:.1e}/{delta['pts'][k]:.1e}" for k in (1, 5, 10, 50)))
    # 1. every variant takes the decisions of the default run
    for v in mvba.VARIANTS:
        assert _decisions(tr[v]) == _decisions(tr["default"]), (name, v, _pattern(tr[v]), _pattern(tr["default"]))
    # 2. none of them near its threshold
    for v, t in tr.items():
        for k, r in enumerate(t):
            for q, thr in THRESHOLDS.items():
                x = r[q]
                if x is None or (name == "nan_obs" and np.isnan(x)):  # a NaN never compares below: no edge to sit on
                    continue
                assert np.isfinite(x) and abs(x - thr) >= KNIFE * thr, (name, v, k, q, x)
    # 3. the bracket starts at zero, opens with the first accepted step and stays under the cap up to k = 10
    kinds = [r["kind"] for r in tr["default"]]
    first = kinds.index("accepted") if "accepted" in kinds else K_MAX + 1
    for key in ("cams", "pts"):
        assert np.all(delta[key][:first] == 0.0), (name, key)
        assert np.all(delta[key][first:] > 0.0), (name, key)
        assert delta[key][10] <= CHAOS_CAP, (name, key, delta[key][10])
    assert all(np.array_equal(t[0]["cams"], scene(name)["cams"]) and np.array_equal(t[0]["pts"], scene(name)["pts"]) for t in tr.values())
    # 4. outside the cap only decisions are compared, and only decisions every variant agrees on
    assert all(_inside_cap(name, k) or _variants_agree(name, k) for k in KS)


def test_premise_most_pairs_are_compared_on_values():
    outside = [(n, k) for n in SCENES for k in KS if not _inside_cap(n, k)]
    print("outside the cap:", outside)
    assert 4 * len(outside) <= len(SCENES) * len(KS), outside


def test_premise_scenes_hold_what_they_are_named_after():
    """The oracle's side of every case, so that a change of seed cannot silently empty one."""
    last = {n: trajectories(n)["default"][-1] for n in SCENES}
    pat = {n: _pattern(trajectories(n)["default"]) for n in SCENES}
    # terminations: the three rare ones, an iteration limit never reached by accident, and function_tolerance as everywhere else
    assert last["exact"]["termination"] == "gradient_tolerance" and last["exact"]["iterations"] < 20
    assert last["exact_heavy"]["termination"] == "parameter_tolerance" and last["exact_heavy"]["iterations"] < 20
    assert last["nan_obs"]["termination"] == "invalid_steps" and last["nan_obs"]["iterations"] == 5 and pat["nan_obs"] == "iiiii"
    nan = trajectories("nan_obs")["default"]
    assert all(np.isnan(r["cost"]) and np.array_equal(r["cams"], scene("nan_obs")["cams"]) and np.array_equal(r["pts"], scene("nan_obs")["pts"])
               for r in nan)
    assert [r["decrease"] for r in nan[:5]] == [2.0, 4.0, 8.0, 16.0, 32.0]  # the growing factor of consecutive failures
    assert int(np.isnan(scene("nan_obs")["obs"]).sum()) == 1
    for n in SCENES:
        if n != "nan_obs":
            assert pat[n].count("A") >= 3 and last[n]["cost"] < 0.05 * trajectories(n)["default"][0]["cost"], (n, pat[n])
    # far start: at least three rejected steps, two of them in a row, accepted ones after them; the factor grows and resets
    far = trajectories("far_start")["default"]
    assert pat["far_start"].count("r") >= 3 and "rr" in pat["far_start"] and "rA" in pat["far_start"], pat["far_start"]
    assert any(r["kind"] == "rejected" and r["decrease"] == 8.0 for r in far)
    assert all(r["decrease"] == 2.0 for r in far if r["kind"] == "accepted")
    # fixed cameras, intrinsics, weights
    assert scene("fixed_mid")["fixed"] == 2 and np.abs(scene("fixed_mid")["cams"][2]).min() > 0
    d = scene("fixed_last_dense")
    assert d["fixed"] == 7 and all(sorted(d["cam_idx"][d["pt_idx"] == p]) == list(range(8)) for p in range(24))
    assert scene("no_fixed")["fixed"] == -1 and scene("no_fixed")["n_cams"] == 8
    a = scene("intrinsics_aniso")
    assert tuple(a["intr"]) == (1.3, 0.8, 0.05, -0.03) and np.all(a["wts"][:, 0] != a["wts"][:, 1])
    assert np.array_equal(scene("exact_heavy")["wts"], 100.0 * scene("exact")["wts"])
    assert scene("minimal")["n_cams"] == 2 and len(scene("minimal")["pts"]) == 7
    # rotation branches of the three free cameras at the start; after the first accepted step all are on the Rodrigues branch
    t2 = (scene("small_rotation")["cams"][:, :3] ** 2).sum(1)
    assert t2[1] == 0.0 and 0.0 < t2[2] <= EPS and EPS < t2[3] < 1e-15 and scene("small_rotation")["fixed"] == 0
    assert pat["small_rotation"][0] == "A" and np.all((trajectories("small_rotation")["default"][1]["cams"][1:, :3] ** 2).sum(1) > 1e-6)
    # strides
    for n, P in (("strides_p513", 513), ("strides_p512", 512), ("strides_o513", 256)):
        s = scene(n)
        counts = np.bincount(s["cam_idx"], minlength=8)
        assert len(s["pts"]) == P and len(s["cam_idx"]) == 2 * P + 1 and s["n_cams"] == 8
        assert [int(counts[c]) for c in (1, 2, 3, 4)] == [0, 1, 64, 65] and all(counts[c] > 65 for c in (0, 5, 6, 7))
        pairs = np.stack([s["cam_idx"], s["pt_idx"]], 1)
        uniq, cnt = np.unique(pairs, axis=0, return_counts=True)
        assert cnt.max() == 2 and (cnt == 2).sum() == 1 and tuple(uniq[cnt == 2][0]) == (5, 201)
        assert np.bincount(s["pt_idx"], minlength=P).min() == 2


# ------------------------------------------------------------------------------------------------ device


def _args(p):
    return (p["n_cams"], p["fixed"], p["intr"], p["cam_idx"], p["pt_idx"], p["obs"], p["wts"], p["cams"], p["pts"])


@functools.lru_cache(maxsize=None)
def _device(k, reverse=False):
    """ONE launch of all scenes with max_iterations = k -> {name: (cams, pts, summary)}; shared by the tests below."""
    from e2e_multi_view_matching_amd import multi_view
    names = list(SCENES)[::-1] if reverse else list(SCENES)
    return dict(zip(names, multi_view.bundle_adjust_batch([_args(scene(n)) for n in names], max_iterations=k)))


def _same_bits(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def _compare(name, k, out=None):
    """The device at max_iterations = k against record k: asserts the decisions and the bars, prints every figure first and
    returns the largest |gpu - mid| / delta of cameras and points (None outside the cap)."""
    p, tr = scene(name), trajectories(name)
    delta, far = bracket(name)
    r = _at(tr["default"], k)
    cams, pts, summary = (out or _device(k))[name]
    # decisions, exactly
    assert (summary["iterations"], summary["termination"]) == (r["iterations"], r["termination"]), (name, k, summary, r["iterations"], r["termination"])
    # the fixed camera's row is the input's
    if p["fixed"] >= 0:
        assert _same_bits(cams[p["fixed"]], p["cams"][p["fixed"]]), (name, k)
    c0 = tr["default"][0]["cost"]
    if np.isnan(c0):
        assert np.isnan(summary["initial_cost"]) and np.isnan(summary["final_cost"]) and np.isnan(r["cost"]), (name, k, summary)
    else:
        assert abs(summary["initial_cost"] - c0) <= 1e-10 * c0, (name, k, summary["initial_cost"], c0)
    if not _inside_cap(name, k):
        return None
    ratio, bad = {}, []
    for key, got, start in (("cams", cams, p["cams"]), ("pts", pts, p["pts"])):
        if delta[key][k] == 0.0:  # nothing accepted yet: the input, bit for bit
            assert _same_bits(got, start), (name, k, key, float(np.abs(got - start).max()))
            continue
        mid = 0.5 * (r[key] + _at(tr[far[key][k]], k)[key])
        dist = np.abs(got - mid)
        ratio[key] = float(dist.max() / delta[key][k])
        if not (np.isfinite(got).all() and dist.max() <= FACTOR * delta[key][k]):
            bad.append((key, float(dist.max()), float(delta[key][k])))
    if not np.isnan(c0):
        if "accepted" not in [x["kind"] for x in tr["default"][:k + 1]]:  # still the input: the bits of initial_cost, judged above
            assert summary["final_cost"] == summary["initial_cost"], (name, k, summary)
            print(f"{name:18s} k={k:2d} it={summary['iterations']:2d} {summary['termination']:18s} input returned bit for bit")
            return 0.0
        mid = 0.5 * (r["cost"] + _at(tr[far["cost"][k]], k)["cost"])
        dist = abs(summary["final_cost"] - mid) / abs(mid)
        ratio["cost"] = float(dist / delta["cost"][k]) if delta["cost"][k] > 0 else (0.0 if dist == 0 else np.inf)
        if not dist <= FACTOR * delta["cost"][k]:
            bad.append(("cost", float(dist), float(delta["cost"][k])))
    print(f"{name:18s} k={k:2d} it={summary['iterations']:2d} {summary['termination']:18s} |gpu-mid|/delta " +
          " ".join(f"{key} {ratio[key]:.2f} (delta {delta[key][k]:.1e})" for key in ratio))
    assert not bad, (name, k, bad)
    return max([ratio[key] for key in ("cams", "pts") if key in ratio], default=0.0)


@pytest.mark.gpu
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("name", list(SCENES))
def test_every_lm_step_matches_the_oracle(gpu, name, k):
    _compare(name, k)


@pytest.mark.gpu
def test_report_pattern_bracket_and_ratio(gpu):
    """Per scene: the accept / reject pattern, delta at k = 1, 5, 10, 50 and the largest |gpu - mid| / delta over all k."""
    for name in SCENES:
        delta, _ = bracket(name)
        ratios = [x for x in (_compare(name, k) for k in KS) if x is not None]
        tr = trajectories(name)["default"]
        print(f"{name:18s} [{_pattern(tr)}] {tr[-1]['termination']}  delta cams/pts k=1,5,10,50: " +
              " ".join(f"{delta['cams'][k]:.1e}/{delta['pts'][k]:.1e}" for k in (1, 5, 10, 50)) +
              f"  max |gpu-mid|/delta = {max(ratios, default=0.0):.2f} over {len(ratios)} of {len(KS)} k")


@pytest.mark.gpu
@pytest.mark.parametrize("k", [5, 50])
def test_batch_order_changes_no_bit(gpu, k):
    a, b = _device(k), _device(k, reverse=True)
    for name in SCENES:
        assert _same_bits(a[name][0], b[name][0]) and _same_bits(a[name][1], b[name][1]), (name, k)
        assert np.array([list(a[name][2].values())[:3]]).tobytes() == np.array([list(b[name][2].values())[:3]]).tobytes(), (name, k)
        assert a[name][2]["termination"] == b[name][2]["termination"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["far_start", "strides_p513"])
def test_alone_returns_the_bits_of_the_batch(gpu, name):
    from e2e_multi_view_matching_amd import multi_view
    for k in (5, 50):
        cams, pts, summary = multi_view.bundle_adjust(*_args(scene(name)), max_iterations=k)
        b = _device(k)[name]
        assert _same_bits(cams, b[0]) and _same_bits(pts, b[1]) and summary == b[2], (name, k, summary, b[2])
