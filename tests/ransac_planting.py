"""Planted two-view scenes for the RANSAC loop of csrc/ransac.hip (shared by tests/test_ransac_planting.py on the CPU and
tests/test_gpu_ransac_loop.py on the device).

The sample of iteration ``it`` is ``draw_sample(seed, it, M)``: it depends on (seed, it, M) alone, so the matches can be
chosen after the indices are known.  A scene puts the five matches of a minimal problem at the sample of a chosen
iteration (a *plant*; all solutions of that problem are then the models of that iteration) and fills every other index
with a match that lies

    on two planted models   x1 = (E_a x0) x (E_b x0), dehomogenised: the meet of the two epipolar lines
    on one planted model    a random x1 projected onto the line E x0
    on none                 random

A match that is not meant to lie on a planted model (any solution of any plant) is drawn again until its squared Sampson
distance to that model is at least 100 t^2, so the count of a planted model is 5 + its fillers, exactly.  Every iteration
that runs and is not a plant has at least one "none" index in its sample (a sample made only of matches on a model would
find that model early); its models are whatever the solver gives and their counts whatever numpy counts: the reference is
always ``np_ransac`` on the hypotheses of the solver in use, never the intended counts.

``solve(x0 [n,5,2], x1 [n,5,2]) -> list of [k,9]`` is the minimal solver: ``np_solver`` here, ``essential_5pt`` on the
device; the order of its solutions is the model order m of an iteration (entry 10 it + m of the resolve kernel's walk).
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_ransac import np_five_point, np_ransac, rotation, sampson, update_num_iters  # noqa: E402
from test_ransac_host import draw_sample  # noqa: E402

THR = 1e-3           # normalised inlier threshold (half a pixel at f = 500)
FAR = 100.0          # a match off a planted model keeps FAR t^2 of squared Sampson distance from it
ON = 1e-12           # a match on a planted model lies within ON t^2 (rounding distance)


class PlantingError(Exception):
    pass


def np_solver(x0, x1):
    """numpy's action-matrix solver in the place of the device's (the order of its solutions is eig's)."""
    out = []
    for a, b in zip(x0, x1):
        try:
            out.append(np_five_point(a, b)[0])
        except np.linalg.LinAlgError:
            out.append(np.zeros((0, 9)))
    return out


def minimal_problems(rng, solve, n=64):
    """Random two-view minimal problems (as in test_minimal_solver_matches_action_matrix_solver), solved in one call:
    a list of (x0 [5,2], x1 [5,2], Es [k,9])."""
    x0s, x1s = [], []
    while len(x0s) < n:
        R, t = rotation(rng.normal(size=3) * 0.3), rng.normal(size=3)
        t /= np.linalg.norm(t)
        X = np.c_[rng.uniform(-1, 1, (5, 2)), rng.uniform(2, 6, 5)]
        Y = X @ R.T + t
        if Y[:, 2].min() < 0.5:
            continue
        x0s.append(X[:, :2] / X[:, 2:])
        x1s.append(Y[:, :2] / Y[:, 2:])
    return list(zip(x0s, x1s, solve(np.array(x0s), np.array(x1s))))


def niters_of(conf, count, M, max_iters=1000):
    return update_num_iters(conf, (M - count) / M, max_iters)


def least_count(conf, M, at_most):
    """The smallest inlier count whose record shrinks niters to ``at_most`` or below."""
    for c in range(5, M + 1):
        if niters_of(conf, c, M) <= at_most:
            return c
    raise PlantingError("no count of {} matches ends the loop by {}".format(M, at_most))


def _epiline(E, x0):
    return E.reshape(3, 3) @ np.r_[x0, 1.0]


def _filler(rng, on):
    """One match on the models ``on`` (none, one or two of them)."""
    x0 = rng.uniform(-0.5, 0.5, 2)
    if len(on) == 0:
        return x0, rng.uniform(-0.7, 0.7, 2)
    if len(on) == 1:
        a, b, c = _epiline(on[0], x0)
        x1 = rng.uniform(-0.7, 0.7, 2)
        return x0, x1 - (a * x1[0] + b * x1[1] + c) / (a * a + b * b) * np.r_[a, b]
    h = np.cross(_epiline(on[0], x0), _epiline(on[1], x0))
    if abs(h[2]) < 1e-3 * np.abs(h).max():
        return x0, None  # the two epipolar lines are close to parallel
    x1 = h[:2] / h[2]
    return x0, (x1 if np.abs(x1).max() <= 2.0 else None)


def _dist(E, x0, x1):
    return float(sampson(E, x0[None], x1[None])[0])


class Scene:
    """name; k0, k1 [M,2]; thr; the call's (seed, conf, max_iters); n_run: the iterations the reference loop is to run;
    check(records, ref, scene): the scenario's conditions on the reference side (asserts)."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def plant(rng, pool, M, its, need, fillers, n_run, thr=THR):
    """plant_once with the first eligible minimal problems for which the fillers can be drawn (two models of a problem
    can leave no match on both that is far from a third)."""
    err = None
    for skip in range(8):
        try:
            return plant_once(rng, pool, M, its, need, fillers, n_run, thr, skip)
        except PlantingError as e:
            err = err or e
    raise err


def plant_once(rng, pool, M, its, need, fillers, n_run, thr, skip):
    """``its[p]``: iteration of plant p, ``need[p]``: its minimal problem has more than need[p] solutions;
    ``fillers``: list of (((p, m), ...), count): count matches on those planted models.  Every iteration below n_run that
    is not a plant gets a "none" index.  ``skip``: eligible problems passed over for plant 0.  Returns (seed, k0, k1, [Es of plant p])."""
    t2 = thr * thr
    for seed in range(16):  # the first seed whose planted samples are disjoint
        samples = [draw_sample(seed, it, M) for it in its]
        flat = [i for s in samples for i in s]
        if all(s is not None for s in samples) and len(set(flat)) == len(flat):
            break
    else:
        raise PlantingError("no seed below 16 keeps the samples of iterations {} disjoint".format(its))
    # minimal problems: the first of the pool with enough solutions whose five matches are far from every other plant's models
    chosen, used = [], set()
    for p in range(len(its)):
        for j, (x0, x1, Es) in enumerate(pool):
            if j in used or len(Es) <= need[p]:
                continue
            if p == 0 and skip > 0:
                skip -= 1
                continue
            others = [E for q in chosen for E in q[2]]
            if all(_dist(E, x0[i], x1[i]) >= FAR * t2 for E in others for i in range(5)) and \
               all(_dist(E, q[0][i], q[1][i]) >= FAR * t2 for E in Es for q in chosen for i in range(5)):
                chosen.append((x0, x1, Es))
                used.add(j)
                break
        else:
            raise PlantingError("no minimal problem with more than {} solutions".format(need[p]))
    models = [(p, m, E) for p, q in enumerate(chosen) for m, E in enumerate(q[2])]
    # the "none" indices: one in every running sample that is not a plant, then up to what the fillers leave
    taken = set(flat)
    none = set()
    for it in range(n_run):
        if it in its:
            continue
        s = draw_sample(seed, it, M)
        if s is None:
            continue  # (64 draws without five distinct picks: the iteration has no model)
        if not none & set(s):
            free = [i for i in s if i not in taken]
            if not free:
                raise PlantingError("the sample of iteration {} lies inside the planted samples".format(it))
            none.add(free[0])
    rest = [i for i in range(M) if i not in taken and i not in none]
    n_fill = sum(c for _, c in fillers)
    if n_fill > len(rest):
        raise PlantingError("{} fillers, {} indices left beside {} forced outliers".format(n_fill, len(rest), len(none)))
    rest = list(rng.permutation(rest))
    kinds = {i: () for i in none}
    for on, c in fillers:
        for _ in range(c):
            kinds[rest.pop()] = tuple(on)
    for i in rest:
        kinds[i] = ()
    k0, k1 = np.zeros((M, 2)), np.zeros((M, 2))
    for p, s in enumerate(samples):
        k0[s], k1[s] = chosen[p][0], chosen[p][1]
    for i in sorted(kinds):
        on = kinds[i]
        Es_on = [chosen[p][2][m] for p, m in on]
        for _ in range(1000):
            x0, x1 = _filler(rng, Es_on)
            if x1 is None:
                continue
            if all(_dist(E, x0, x1) <= ON * t2 for E in Es_on) and \
               all(_dist(E, x0, x1) >= FAR * t2 for p, m, E in models if (p, m) not in on):
                break
        else:
            raise PlantingError("no match on {} and far from the other planted models in 1000 draws".format(on))
        k0[i], k1[i] = x0, x1
    return seed, k0, k1, [q[2] for q in chosen]


def count(E, sc):
    return int(np.sum(sampson(E, sc.k0, sc.k1) <= sc.thr ** 2))


# ---------------------------------------------------------------------------------------------------------------------
# the scenarios.  M is 200 - 400: large enough that the forced "none" indices (about one per running iteration) fit.
# ---------------------------------------------------------------------------------------------------------------------
def seam_scene(name, rng, pool, it_star, s, M, conf=0.9, tie=False):
    """Model a < s of iteration it* sets a record that shrinks niters to it* or below; model b >= s of the same iteration
    has more inliers (tie: exactly as many) and must still compete.  Where 10 it* + s is a multiple of 64 the two lie in
    different 64-entry chunks of the resolve kernel's walk.  (a, b) is the first pair, from (0, s), whose fillers can be
    drawn."""
    c_a = least_count(conf, M, it_star) + 2
    c_b = c_a if tie else c_a + 12
    err = None
    for a, b in [(a, b) for a in range(s) for b in (s, s + 1)]:
        if tie:  # 8 fillers on either model alone keep the two supports different
            fillers = [(((0, a), (0, b)), c_a - 13), (((0, a),), 8), (((0, b),), 8)]
        else:
            fillers = [(((0, a), (0, b)), c_a - 5), (((0, b),), c_b - c_a)]
        try:
            seed, k0, k1, Es = plant(rng, pool, M, [it_star], [b], fillers, it_star + 1)
            break
        except PlantingError as e:
            err = err or e
    else:
        raise err

    def check(rec, ref, sc):
        first = [r for r in rec if r[0] == it_star and r[1] < s]
        assert first and first[-1][3] <= it_star, rec[-3:]  # a record below the split ends the loop at this iteration
        assert ref["iters"] == it_star + 1, ref["iters"]
        if tie:
            assert ref["winner"] == (it_star, a) and count(Es[0][b], sc) == ref["best"], (ref["winner"], ref["best"])
        else:
            assert ref["winner"] == (it_star, b), ref["winner"]
    return Scene(name=name, seed=seed, conf=conf, max_iters=1000, M=M, thr=THR, k0=k0, k1=k1, n_run=it_star + 1, check=check)


def trap_scene(name, rng, pool, i1, M, conf=0.9, max_iters=1000, c_b=None, ahead=20):
    """A record at iteration i1 ends the loop at n1 = max(i1 + 1, niters); the sample of iteration n1, the first that does
    not run, is planted with a model of 15 more inliers."""
    if c_b is None:
        c_b = least_count(conf, M, i1 + ahead)
    n1 = max(i1 + 1, niters_of(conf, c_b, M, max_iters))
    fillers = [(((0, 0), (1, 0)), c_b - 35), (((0, 0),), 30), (((1, 0),), 45)]
    seed, k0, k1, Es = plant(rng, pool, M, [i1, n1], [0, 0], fillers, n1)

    def check(rec, ref, sc):
        assert ref["winner"] == (i1, 0) and ref["iters"] == n1, (ref["winner"], ref["iters"], n1)
        assert count(Es[1][0], sc) > ref["best"], (count(Es[1][0], sc), ref["best"])  # the trap would have won
    return Scene(name=name, seed=seed, conf=conf, max_iters=max_iters, M=M, thr=THR, k0=k0, k1=k1, n_run=n1, check=check,
                 trap=Es[1][0])


def two_scene(name, rng, pool, i1, c1, i2, c2, M, conf=0.9):
    """Model 0 of iteration i1 with c1 inliers, model 0 of iteration i2 > i1 with c2; niters after the first record stays
    above i2, so the second competes: it wins with c2 > c1 and loses with c2 == c1 (the strict rule)."""
    both = min(c1, c2) - 10
    fillers = [(((0, 0), (1, 0)), both), (((0, 0),), c1 - 5 - both), (((1, 0),), c2 - 5 - both)]
    n1 = niters_of(conf, c1, M)
    if n1 <= i2:
        raise PlantingError("a record of {} at {} ends the loop at {}, before {}".format(c1, i1, n1, i2))
    n_run = max(i2 + 1, niters_of(conf, c2, M)) if c2 > c1 else n1
    seed, k0, k1, Es = plant(rng, pool, M, [i1, i2], [0, 0], fillers, n_run)

    def check(rec, ref, sc):
        assert (i1, 0) in [r[:2] for r in rec], rec[-3:]
        assert ref["winner"] == ((i2, 0) if c2 > c1 else (i1, 0)) and ref["iters"] == n_run, (ref["winner"], ref["iters"])
        assert (count(Es[0][0], sc), count(Es[1][0], sc)) == (c1, c2)
    return Scene(name=name, seed=seed, conf=conf, max_iters=1000, M=M, thr=THR, k0=k0, k1=k1, n_run=n_run, check=check)


def single_scene(name, rng, pool, it_star, c, M, conf=0.9):
    """Nothing above a handful of inliers before iteration it*, whose model 0 has c."""
    n_run = max(it_star + 1, niters_of(conf, c, M))
    seed, k0, k1, Es = plant(rng, pool, M, [it_star], [0], [(((0, 0),), c - 5)], n_run)

    def check(rec, ref, sc):
        assert ref["winner"] == (it_star, 0) and ref["iters"] == n_run, (ref["winner"], ref["iters"])
        assert max([r[2] for r in rec[:-1]], default=0) < c // 4, rec  # the records before it stay small
    return Scene(name=name, seed=seed, conf=conf, max_iters=1000, M=M, thr=THR, k0=k0, k1=k1, n_run=n_run, check=check)


# name -> builder(rng, pool).  Splits 6 (iteration 25) and 8 (iteration 12) need a minimal problem with 8 or 10 real
# solutions.  Of 20000 random problems 26 had 8 and none had 10, so the pool's seed is searched once, here and not at run
# time: POOL_SEED is the first seed whose first POOL_SIZE problems hold one with 10 (problem 244; numpy's solver and the
# device's agree on the count), which serves both splits.  A pool without it fails those two scenes (PlantingError).
POOL_SEED, POOL_SIZE = 29, 256
SCENES = {
    "seam_it19_split2": lambda r, p: seam_scene("seam_it19_split2", r, p, 19, 2, 200),
    "seam_it51_split2": lambda r, p: seam_scene("seam_it51_split2", r, p, 51, 2, 200),
    "seam_it147_split2": lambda r, p: seam_scene("seam_it147_split2", r, p, 147, 2, 400),
    "seam_it6_split4": lambda r, p: seam_scene("seam_it6_split4", r, p, 6, 4, 300),
    "seam_it38_split4": lambda r, p: seam_scene("seam_it38_split4", r, p, 38, 4, 300),
    "control_it20_split2": lambda r, p: seam_scene("control_it20_split2", r, p, 20, 2, 200),
    "trap_past_the_end": lambda r, p: trap_scene("trap_past_the_end", r, p, 10, 400),
    "round_record_at_127_ends_at_128": lambda r, p: trap_scene("round_record_at_127_ends_at_128", r, p, 127, 400, ahead=1),
    "round_record_at_127_then_128": lambda r, p: two_scene("round_record_at_127_then_128", r, p, 127, 150, 128, 260, 400),
    "round_first_record_at_128": lambda r, p: single_scene("round_first_record_at_128", r, p, 128, 260, 400),
    "round_carried_best_met_by_equal": lambda r, p: two_scene("round_carried_best_met_by_equal", r, p, 100, 175, 135, 175, 400),
    "tie_same_iteration": lambda r, p: seam_scene("tie_same_iteration", r, p, 19, 2, 200, tie=True),
    "tie_other_iteration": lambda r, p: two_scene("tie_other_iteration", r, p, 10, 120, 15, 120, 200),
    "max_iters_1": lambda r, p: trap_scene("max_iters_1", r, p, 0, 400, max_iters=1, c_b=150),
    "max_iters_127": lambda r, p: trap_scene("max_iters_127", r, p, 126, 400, max_iters=127, c_b=150),
    "max_iters_128": lambda r, p: trap_scene("max_iters_128", r, p, 127, 400, max_iters=128, c_b=150),
    "max_iters_129": lambda r, p: trap_scene("max_iters_129", r, p, 128, 400, max_iters=129, c_b=150),
    "seam_it25_split6": lambda r, p: seam_scene("seam_it25_split6", r, p, 25, 6, 200),
    "seam_it12_split8": lambda r, p: seam_scene("seam_it12_split8", r, p, 12, 8, 300),
}


def build_scenes(solve, names=None):
    """The scenes (all, or those named), each from its own generator (a scene does not depend on which others are built),
    on one pool of minimal problems solved in one call."""
    pool = minimal_problems(np.random.default_rng(POOL_SEED), solve, POOL_SIZE)
    return {n: SCENES[n](np.random.default_rng([POOL_SEED, k]), pool)
            for k, n in enumerate(SCENES) if names is None or n in names}


# ---------------------------------------------------------------------------------------------------------------------
# the reference side
# ---------------------------------------------------------------------------------------------------------------------
def samples_of(sc, n):
    """The matches of the samples of iterations 0 .. n - 1 ([n,5,2] twice)."""
    idx = [draw_sample(sc.seed, it, sc.M) for it in range(n)]
    assert all(s is not None for s in idx)
    return sc.k0[np.array(idx)], sc.k1[np.array(idx)]


def pad(hyps, sc):
    return list(hyps) + [np.zeros((0, 9))] * (sc.max_iters + 1 - len(hyps))


def records(sc, hyps):
    """The sequential rule once more, keeping every record: (iteration, model, count, niters after it)."""
    t2, niters, best, out, it = sc.thr ** 2, sc.max_iters, 0, [], 0
    while it < niters:
        for m, E in enumerate(hyps[it]):
            good = int(np.sum(sampson(E, sc.k0, sc.k1) <= t2))
            if good > max(best, 4):
                best, niters = good, update_num_iters(sc.conf, (sc.M - good) / sc.M, niters)
                out.append((it, m, good, niters))
        it += 1
    return out, it


def reference(sc, hyps):
    """np_ransac on the scene, with the conditions every planted case must meet: clean (no scored match within 1e-5
    relative of t^2), the scenario's own (sc.check), and the two statements of the loop agree."""
    hyps = pad(hyps, sc)
    it_ref, best_ref, E_ref, clean = np_ransac(sc.k0, sc.k1, sc.thr, hyps, conf=sc.conf, max_iters=sc.max_iters)
    assert clean, sc.name
    rec, it2 = records(sc, hyps)
    assert rec and (it2, rec[-1][2]) == (it_ref, best_ref), (sc.name, it2, it_ref, rec[-1], best_ref)
    assert np.array_equal(hyps[rec[-1][0]][rec[-1][1]], E_ref), sc.name
    ref = {"iters": it_ref, "best": best_ref, "E": E_ref, "winner": rec[-1][:2],
           "mask": sampson(E_ref, sc.k0, sc.k1) <= sc.thr ** 2}
    sc.check(rec, ref, sc)
    return ref
