"""CPU: the planted RANSAC scenes of tests/ransac_planting.py, with numpy's action-matrix solver in the place of the
device's minimal solver.  Each builder must yield a scene whose reference run (np_ransac on the solver's hypotheses of the
documented sample stream) is clean - no scored match within 1e-5 relative of t^2 - and in its scenario: the record sits at
the planted (iteration, model), an earlier record of the same iteration below the split has already ended the loop there,
the trap past the end would have won, the tied counts are equal, ...  (the asserts of ``reference`` and of each scene's
``check``).  tests/test_gpu_ransac_loop.py builds the same scenes on the device's solver and holds the kernels to them."""
import numpy as np
import pytest

import ransac_planting as P
from test_ransac_host import draw_sample


@pytest.fixture(scope="module")
def scenes():
    return P.build_scenes(P.np_solver)


@pytest.mark.parametrize("name", list(P.SCENES))
def test_scene_is_clean_and_in_scenario(scenes, name):
    sc = scenes[name]
    ref = P.reference(sc, P.np_solver(*P.samples_of(sc, sc.n_run + 1)))
    assert ref["iters"] == sc.n_run and ref["best"] == int(ref["mask"].sum())
    # every running sample that is not the winner's holds a match far from the winning model (no early find)
    d = P.sampson(ref["E"], sc.k0, sc.k1)
    for it in range(ref["iters"]):
        if it != ref["winner"][0]:
            assert d[draw_sample(sc.seed, it, sc.M)].max() >= P.FAR * sc.thr ** 2, it


def test_planted_counts_are_exact(scenes):
    """A planted model's count is 5 + its fillers: matches on it lie at rounding distance, all others beyond 100 t^2."""
    sc = scenes["seam_it19_split2"]
    ref = P.reference(sc, P.np_solver(*P.samples_of(sc, sc.n_run + 1)))
    d = P.sampson(ref["E"], sc.k0, sc.k1) / sc.thr ** 2
    assert np.all((d <= 1e-6) | (d >= P.FAR)), np.sort(d[(d > 1e-6) & (d < P.FAR)])
    c_a = P.least_count(sc.conf, sc.M, 19) + 2
    assert ref["best"] == c_a + 12 and P.niters_of(sc.conf, c_a, sc.M) <= 19 < P.niters_of(sc.conf, c_a - 3, sc.M)


def test_a_scene_does_not_depend_on_the_others(scenes):
    one = P.build_scenes(P.np_solver, names=["tie_other_iteration"])["tie_other_iteration"]
    assert np.array_equal(one.k0, scenes["tie_other_iteration"].k0) and np.array_equal(one.k1, scenes["tie_other_iteration"].k1)
