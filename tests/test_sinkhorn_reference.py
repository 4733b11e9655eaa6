"""CPU: the fp64 Sinkhorn restatement of the GPU edge tests (tests/sinkhorn_restatement.py) against
``oracle.sinkhorn.log_optimal_transport`` run in fp64 (bar 1e-12), and the reference-side conditions the GPU file
(tests/test_gpu_sinkhorn_edges.py) relies on: how far the fp32 oracle is from fp64 on every case, how well the fp32 oracle
itself satisfies the two identities the GPU results are held to, and that the arg-max comparison leaves out next to nothing."""
import numpy as np
import pytest
import torch

import sinkhorn_restatement as sr
from oracle.sinkhorn import log_optimal_transport

PIN = 1e-12
ORACLE_ERROR_BAR = 1e-5      # measured: 5.8e-6 (2 ulp of fp32 at |Z| ~ 28)
ORACLE_COLUMN_BAR = 2e-6     # measured: 7.9e-7
ORACLE_RANK_BAR = 2e-5       # measured: 8.1e-6

# the shapes of the further GPU tests (rounds and segments with a few problems standing for the batch, one hostile problem
# among healthy ones, unaligned scores)
OTHER_SHAPES = [(5, 4, 250), (5, 4, 514), (5, 4, 1026), (3, 64, 514), (3, 64, 1026), (2, 64, 516), (2, 33, 256)]


@pytest.mark.parametrize("family,shape", sr.CASES, ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_restatement_and_the_conditions_of_the_gpu_file(family, shape):
    B, M, N = shape
    s = sr.scores(B, M, N)
    worst = {"pin": 0.0, "oracle": 0.0, "column": 0.0, "rank": 0.0}
    for alpha in sr.ALPHAS:
        ref = sr.case_reference(B, M, N, alpha)
        orc = sr.case_oracle(B, M, N, alpha)
        for iters in sr.ITERS_STREAM:
            z64 = log_optimal_transport(s.double(), alpha, iters).numpy()
            worst["pin"] = max(worst["pin"], float(np.abs(ref[iters] - z64).max()))
            err, col, rank, zmax = orc[iters]
            assert np.isfinite(ref[iters]).all() and zmax < 100.0
            worst["oracle"] = max(worst["oracle"], err)
            worst["rank"] = max(worst["rank"], rank)
            # the restatement itself satisfies both identities to fp64 rounding
            assert sr.rank_residual(ref[iters], s.numpy(), alpha) < 1e-12
            if iters:
                worst["column"] = max(worst["column"], col)
                assert sr.column_residual(ref[iters], M, N) < 1e-12
            rows, cols = sr.decided(ref[iters])
            # (columns: 1 % or one column - among three columns of 1000 rows each a single near-tie is already a third)
            assert (~rows).sum(1).max() <= sr.TIE_FRACTION * M and (~cols).sum(1).max() <= max(1.0, sr.TIE_FRACTION * N), (alpha, iters)
    print("%s %s: pin %.2e  oracle_error %.2e  column %.2e  rank %.2e" % (family, shape, worst["pin"], worst["oracle"], worst["column"], worst["rank"]))
    assert worst["pin"] <= PIN, worst
    assert worst["oracle"] <= ORACLE_ERROR_BAR, worst
    assert worst["column"] <= ORACLE_COLUMN_BAR, worst
    assert worst["rank"] <= ORACLE_RANK_BAR, worst


@pytest.mark.parametrize("shape", OTHER_SHAPES, ids=lambda v: "x".join(map(str, v)))
def test_restatement_on_the_shapes_of_the_further_tests(shape):
    B, M, N = shape
    s = sr.scores(B, M, N, seed=11)
    for alpha in (1.0, 3.7):
        ref = sr.sinkhorn_fp64_at(s.numpy(), alpha, sr.ITERS_STREAM)
        for iters in sr.ITERS_STREAM:
            z64 = log_optimal_transport(s.double(), alpha, iters).numpy()
            assert float(np.abs(ref[iters][0] - z64).max()) <= PIN, (alpha, iters)


def test_restatement_returns_the_potentials():
    """Z = C + u_i + v_j - norm from the u and v it returns; sinkhorn_fp64 is the snapshot of the same run."""
    s = sr.scores(2, 5, 7)
    Z, u, v = sr.sinkhorn_fp64(s.numpy(), 0.5, 4)
    assert u.shape == (2, 6) and v.shape == (2, 8)
    assert np.array_equal(Z, (sr.couplings(s, 0.5) + u[:, :, None] + v[:, None, :]) + np.log(12.0))
    assert np.array_equal(Z, sr.sinkhorn_fp64_at(s.numpy(), 0.5, (0, 4, 9))[4][0])
    assert sr.oracle_error(s, 0.5, 4) == float(np.abs(sr.oracle_fp32(s, 0.5, 4) - Z).max())


def test_the_identities_catch_what_they_are_for():
    """A wrong element breaks rank_residual by its size; a stale column potential breaks column_residual."""
    s = sr.scores(1, 6, 9)
    Z, u, v = sr.sinkhorn_fp64(s.numpy(), 1.0, 3)
    bad = Z.copy()
    bad[0, 2, 3] += 1e-3
    assert abs(sr.rank_residual(bad, s.numpy(), 1.0) - 1e-3) < 1e-9
    swapped = Z.copy()
    swapped[0, 1, [4, 5]] = swapped[0, 1, [5, 4]]                      # an element from the neighbouring column
    assert sr.rank_residual(swapped, s.numpy(), 1.0) > 1e-2
    stale = Z + 1e-3 * (np.arange(10) == 4)                          # column 4 carries the potential of another half-iteration
    assert sr.rank_residual(stale, s.numpy(), 1.0) < 1e-12 and abs(sr.column_residual(stale, 6, 9) - 1e-3) < 1e-9
    # the dustbin row of a result computed with another bin score in the hand-off of u[M]
    shifted = Z.copy()
    shifted[0, 6, :] += 2.7
    assert sr.rank_residual(shifted, s.numpy(), 1.0) < 1e-12 and sr.column_residual(shifted, 6, 9) > 1e-3


@pytest.mark.parametrize("N", sorted(sr.HOSTILE))
def test_the_hostile_problem_leaves_fp32_range_and_the_reference_stays_finite(N):
    """What the one-hostile-problem GPU test relies on: at randn * 160 and its iteration count the fp64 potentials have moved
    beyond 95 nats (b_j = exp(v_j) and a_i = exp(u_i + rowmax_i) of the exponential-domain kernels cannot be held in fp32, which
    ends at 88.7: the rescue pass has to run), the fp64 reference is finite and agrees with the oracle in fp64 to 1e-12 of its
    magnitude, and the fp32 oracle - the log-domain arithmetic of the rescue pass - is itself within 4e-3 of fp64 there, so
    that 5e-3 can be asked of the device.  Measured: 3.3e-3 (514 columns), 3.5e-3 (1026)."""
    M, alpha = 64, 1.0
    seed, iters = sr.HOSTILE[N]
    s = sr.scores(1, M, N, scale=sr.HOSTILE_SCALE, seed=seed)
    Z, u, v = sr.sinkhorn_fp64(s.numpy(), alpha, iters)
    z64 = log_optimal_transport(s.double(), alpha, iters).numpy()
    assert np.isfinite(Z).all()
    assert float(np.abs(Z - z64).max()) <= PIN * float(np.abs(Z).max())
    rowmax = np.maximum(s.numpy().astype(np.float64).max(2), alpha)
    moved = min(float(np.abs(v).max()), float(np.abs(u[:, :M] + rowmax).max()))
    err = sr.oracle_error(s, alpha, iters)
    print("hostile N %d: potentials moved %.1f nats, max |Z| %.0f, fp32 oracle error %.2e" % (N, moved, np.abs(Z).max(), err))
    assert moved >= 95.0, moved
    assert err <= 4e-3, err
    # ... while at 20 iterations nothing has left fp32's range at any scale: the drift is log 2 per iteration
    Z20, u20, v20 = sr.sinkhorn_fp64(s.numpy(), alpha, 20)
    assert max(float(np.abs(v20).max()), float(np.abs(u20[:, :M] + rowmax).max())) < 20.0
