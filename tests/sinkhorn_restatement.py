"""fp64 restatement of upstream ``log_optimal_transport`` in plain numpy, the case lists of the Sinkhorn edge tests and the
yardsticks they share (helper of tests/test_sinkhorn_reference.py and tests/test_gpu_sinkhorn_edges.py; no test lives here).

The restatement builds the explicit (M+1) x (N+1) coupling matrix and evaluates every log-sum-exp by the shifted formula; it
is pinned to ``oracle.sinkhorn.log_optimal_transport`` run in fp64 by the CPU test.  Everything a GPU test compares a kernel
with is computed here from the reference side alone: the fp64 result, the fp32 oracle's own distance from it, and two
identities of the result that need no reference at all (``column_residual``, ``rank_residual``)."""
import functools

import numpy as np
import torch

ALPHAS = (-2.5, 0.0, 1.0, 3.7)
ITERS = (1, 2, 3, 20)
ITERS_STREAM = (0,) + ITERS   # the log-domain chain also serves iters = 0

# family -> (pin, rows_per_workgroup the plan must report, [(B, M, N), ...]).  Each shape is the smallest that reaches its
# instance.  FULL: N == KT * 256 (for the register-addressed kernels also M a multiple of the workgroup's rows), no masked
# tails.  pairs: KT >= 4 and an even column slice ceil(N / G) - the exchange then moves 16-byte granule pairs.
FAMILIES = {
    "kt1": ("rows64", 32, [
        (2, 1, 1),        # one row, one column: every lane but one masked
        (2, 33, 255),     # two workgroups, ragged rows and columns
        (2, 32, 256),     # FULL
        (1, 1, 256),      # FULL, one row
    ]),
    "kt2": ("rows64", 32, [
        (2, 65, 257),     # the first column of the second chunk
        (2, 40, 511),     # ragged
        (2, 64, 512),     # FULL
    ]),
    "kt4": ("rows64", 64, [
        (2, 65, 513),     # two workgroups, column slice 257: odd, no pairs
        (2, 64, 514),     # one workgroup, slice 514: pairs
        (1, 1, 1024),     # FULL with pairs
        (1, 300, 1024),   # FULL, five workgroups, slice 205: odd, no pairs
    ]),
    "kt8": ("rows64", 32, [
        (2, 33, 1025),    # two workgroups, slice 513: odd, no pairs
        (2, 32, 1026),    # one workgroup: pairs
        (1, 1, 2048),     # FULL with pairs
        (1, 70, 2048),    # FULL, three workgroups, slice 683: odd, no pairs
    ]),
    "regs128": ("rows128", 128, [
        (2, 1, 514),      # one row
        (2, 129, 516),    # two workgroups, the second with one row
        (1, 130, 1024),   # full columns, ragged rows: not FULL
        (2, 128, 1024),   # FULL, one workgroup
        (1, 256, 1024),   # FULL, two workgroups
    ]),
    "regs2k": ("rows128", 64, [
        (2, 1, 1026),     # one row
        (1, 65, 1028),    # two workgroups, the second with one row
        (1, 64, 2048),    # FULL, one workgroup
        (1, 128, 2048),   # FULL, two workgroups
    ]),
    "aspect": (None, 32, [
        (1, 1000, 3),     # 32 workgroups exchanging three columns: most of them own no column slice
        (1, 2047, 5),     # 64 workgroups, five columns
    ]),
}
CASES = [(family, shape) for family, (_, _, shapes) in FAMILIES.items() for shape in shapes]

# The hostile problem of the rescue test: randn * HOSTILE_SCALE on 64 rows; width -> (seed, iters) at which the fp64 potentials
# have left the range of fp32's exponential (|v_j| and |u_i + rowmax_i| beyond 95 nats, fp32 ends at 88.7)
HOSTILE_SCALE = 160.0
HOSTILE = {514: (182, 160), 1026: (200, 160)}

TIE = 1e-5          # rows / columns whose two largest fp64 values lie closer than this are left out of the arg-max comparison
TIE_FRACTION = 0.01  # ... and no case may leave out more than this fraction of its rows or columns


def scores(B, M, N, scale=3.0, seed=None):
    """[B, M, N] fp32 scores, randn * scale from a seeded generator (the rule of tests/test_gpu_sinkhorn_resident.py)."""
    g = torch.Generator().manual_seed(7 * B + M + N if seed is None else seed)
    return torch.randn(B, M, N, generator=g) * scale


def _lse(x, axis):
    m = x.max(axis=axis, keepdims=True)
    return np.squeeze(m, axis) + np.log(np.exp(x - m).sum(axis=axis))


def couplings(s, alpha):
    """The explicit [B, M+1, N+1] fp64 coupling matrix: the scores, bordered by the bin score."""
    s = np.asarray(s, dtype=np.float64)
    B, M, N = s.shape
    C = np.full((B, M + 1, N + 1), float(alpha), dtype=np.float64)
    C[:, :M, :N] = s
    return C


def sinkhorn_fp64_at(s, alpha, iters_list):
    """{iters: (Z, u, v)} for every count of `iters_list` from ONE run of the recurrence (snapshots of the same u, v)."""
    C = couplings(s, alpha)
    B, M1, N1 = C.shape
    M, N = M1 - 1, N1 - 1
    norm = -np.log(float(M + N))
    log_mu = np.full((B, M1), norm)
    log_mu[:, M] = np.log(float(N)) + norm
    log_nu = np.full((B, N1), norm)
    log_nu[:, N] = np.log(float(M)) + norm
    u, v = np.zeros((B, M1)), np.zeros((B, N1))
    out = {}
    for k in range(max(iters_list) + 1):
        if k in iters_list:
            out[k] = ((C + u[:, :, None] + v[:, None, :]) - norm, u.copy(), v.copy())
        u = log_mu - _lse(C + v[:, None, :], 2)
        v = log_nu - _lse(C + u[:, :, None], 1)
    return out


def sinkhorn_fp64(s, alpha, iters):
    """Upstream ``log_optimal_transport`` in fp64: (Z [B, M+1, N+1], u [B, M+1], v [B, N+1]) as numpy arrays."""
    return sinkhorn_fp64_at(s, alpha, (iters,))[iters]


def oracle_fp32(s, alpha, iters):
    """The fp32 oracle's result as a numpy array."""
    from oracle.sinkhorn import log_optimal_transport
    return log_optimal_transport(s.float(), float(alpha), iters).numpy()


def oracle_error(s, alpha, iters):
    """max |oracle fp32 - restatement fp64|: what the reference itself loses to fp32 on this input."""
    return float(np.abs(oracle_fp32(s, alpha, iters).astype(np.float64) - sinkhorn_fp64(s, alpha, iters)[0]).max())


def column_residual(Z, M, N):
    """max over the N + 1 columns of |LSE_i Z[i, j] - t_j|, t_j = 0 for j < N and log M for j = N, evaluated in fp64.  The
    column update is the last half-iteration, so every exact result satisfies this with 0 for every iters >= 1."""
    Z = np.asarray(Z, dtype=np.float64)
    assert Z.shape[-2:] == (M + 1, N + 1)
    t = np.zeros(N + 1)
    t[N] = np.log(float(M))
    return float(np.abs(_lse(Z, Z.ndim - 2) - t).max())


def rank_residual(Z, s, alpha):
    """With D = Z - C: max |D[i, j] - D[i, 0] - D[0, j] + D[0, 0]|, 0 for anything of the form C + u_i + v_j - norm.  An
    element that took a wrong row, column or score breaks it."""
    D = np.asarray(Z, dtype=np.float64) - couplings(s, alpha)
    return float(np.abs(D - D[:, :, :1] - D[:, :1, :] + D[:, :1, :1]).max())


def ulp32(x):
    """One unit in the last place of fp32 at |x|."""
    return float(np.spacing(np.float32(abs(x))))


def argmax_of_core(Z):
    """(row arg-max [B, M], column arg-max [B, N]) over the M x N core."""
    core = np.asarray(Z)[:, :-1, :-1]
    return core.argmax(2), core.argmax(1)


def decided(Zref):
    """(rows [B, M], columns [B, N]) bool: where the two largest fp64 values of the core lie at least TIE apart, so that a
    result within the bar must pick the same element."""
    core = np.asarray(Zref)[:, :-1, :-1]

    def gap(axis):
        if core.shape[axis] < 2:
            return np.full(np.delete(core.shape, axis), np.inf)
        top = np.sort(core, axis=axis)
        return np.take(top, -1, axis) - np.take(top, -2, axis)
    return gap(2) >= TIE, gap(1) >= TIE


# ---- per-case references, computed once and shared by every test that needs them (callers must not write into them)

@functools.lru_cache(maxsize=4)
def case_reference(B, M, N, alpha):
    """{iters: Z fp64} for every count of ITERS_STREAM on scores(B, M, N)."""
    return {k: z for k, (z, _, _) in sinkhorn_fp64_at(scores(B, M, N).numpy(), alpha, ITERS_STREAM).items()}


@functools.lru_cache(maxsize=4)
def case_oracle(B, M, N, alpha):
    """{iters: (oracle_error, the fp32 oracle's column_residual, its rank_residual, max |Z|)} for every count of ITERS_STREAM."""
    s = scores(B, M, N)
    ref = case_reference(B, M, N, alpha)
    out = {}
    for k in ITERS_STREAM:
        z32 = oracle_fp32(s, alpha, k)
        out[k] = (float(np.abs(z32.astype(np.float64) - ref[k]).max()), column_residual(z32, M, N) if k else None,
                  rank_residual(z32, s.numpy(), alpha), float(np.abs(ref[k]).max()))
    return out
