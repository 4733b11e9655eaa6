"""Every Sinkhorn kernel instance at its smallest shapes (-m gpu), against the fp64 restatement of
tests/sinkhorn_restatement.py (itself pinned on the CPU by tests/test_sinkhorn_reference.py).

tests/test_gpu_sinkhorn_resident.py is thorough about scale; this file is about what scale hides: bin scores other than 1.0
behind every kernel, one to three iterations (Sinkhorn contracts: twenty iterations later a wrong half-iteration is mostly
forgotten), the register-addressed kernels on one small problem, the FULL / pair instances at small M, the rescue pass on one
problem among healthy neighbours, the copy path for unaligned scores, and rounds / segments with one-workgroup problems.
Which kernel serves a call is asserted from the launcher's plan before the call; a case whose plan is not the intended one fails.

Yardsticks (all from the reference side; nothing here is measured against the kernels):
  * |out - fp64| < 1e-4, the project's bar, as the hard limit;
  * the ratio r = |out - fp64|_max / max(oracle_error, 1 ulp of fp32 at max |Z|), oracle_error = |fp32 oracle - fp64|_max on
    the same input: how many times the reference's own fp32 error a kernel is off.  (The floor: no fp32 result can be expected
    nearer to fp64 than its last place, and on the 1 x 1 problem the oracle's error can be exactly 0.)  The bar is three times
    the worst r measured per kernel family on an MI355X (MEASURED_RATIO; the operation orders differ - exponential domain with
    one division per four rows against the oracle's log-sum-exps); a measured r above 8 would be a finding, not a tolerance;
  * column_residual and rank_residual, two identities of the result: at most four times the fp32 oracle's own residual on the
    same case plus 8 ulp of fp32 at max |Z| (the oracle's residual can be exactly 0 on the 1 x 1 problem);
  * arg-max over the core as in fp64, rows and columns whose two largest fp64 values lie within 1e-5 left out (the CPU test
    asserts that this leaves out at most 1 % of the rows of any case)."""
import contextlib

import numpy as np
import pytest
import torch

import sinkhorn_restatement as sr

pytestmark = pytest.mark.gpu

HARD_BAR = 1e-4
# Worst r per kernel family as measured on an MI355X (printed by test_report_of_the_measured_ratios); the asserted bar is three
# times the figure.  "stream": the log-domain chain under the `stream` pin over the same cases, iters = 0 included.
# (kt1 and stream: the 1 x 1 problem at one iteration, |out - fp64| = 2.5e-7 and 2.7e-7 against one ulp of 1.2e-7; the largest
# figure on any other shape is 1.81)
MEASURED_RATIO = {"kt1": 2.06, "kt2": 1.21, "kt4": 1.49, "kt8": 1.51, "regs128": 1.45, "regs2k": 1.47, "aspect": 1.63, "stream": 2.30}
# Worst (column_residual, rank_residual) per family as fractions of their bars, measured likewise; a figure above 1 fails
MEASURED_IDENTITY = {"kt1": (0.19, 0.16), "kt2": (0.10, 0.18), "kt4": (0.10, 0.16), "kt8": (0.09, 0.16), "regs128": (0.09, 0.17),
                     "regs2k": (0.09, 0.17), "aspect": (0.09, 0.16), "stream": (0.11, 0.20)}
# The hostile problem: randn * HOSTILE_SCALE, 160 being the figure of test_dynamic_range_of_the_exponential_domain.  The scale
# alone sends no 64-row problem to the rescue pass: measured on an MI355X, every kernel survives 160, 320 and 640 at 20 and at
# 100 iterations.  Where two rows have their maximum in one column the potentials drift apart by log 2 per iteration until the
# rows' second-best columns take over, so fp32's range (88 nats) is left only after ~130 iterations and only where that gap
# exceeds it.  sr.HOSTILE names, per width, a seed and an iteration count at which the fp64 potentials have moved by more than
# 95 nats at scale 160 (asserted on the CPU by tests/test_sinkhorn_reference.py): sinkhorn_rescued == 1 per call behind all
# four kernels there, and the rescued problem is 3.3e-3 (514 columns) and 3.5e-3 (1026) from fp64 - what the fp32 oracle is on
# the same input (3.3e-3, 3.5e-3): after 160 iterations that do not contract, fp32's log domain is no nearer than that.
HOSTILE_SCALE = sr.HOSTILE_SCALE
HOSTILE_BAR = 5e-3   # fp32 log domain at |logZ| ~ 1200: the existing bar of that regime

_worst = {}   # family -> [r, column ratio, rank ratio], filled by the tests, printed by the report


def _ctx(gpu):
    from e2e_multi_view_matching_amd import _lib
    return _lib.context(gpu)


@contextlib.contextmanager
def _pinned(ctx, pin):
    try:
        ctx.set_sinkhorn_kernel(pin)
        yield
    finally:
        ctx.set_sinkhorn_kernel(None)


def _assert_plan(ctx, B, M, N, iters, rows):
    """The launcher's plan for this call: one resident launch on `rows`-row workgroups, or (rows None) the log-domain chain."""
    plan = ctx.sinkhorn_plan(B, M, N, iters)
    if rows is None:
        assert plan == [], plan
    else:
        assert [(s["rows_per_workgroup"], s["problems"]) for s in plan] == [(rows, B)], (plan, rows)


def _no_events(ctx):
    st = ctx.stats(reset=True)
    assert st["sinkhorn_rescued"] == 0 and st["sinkhorn_bad"] == 0 and st["sinkhorn_timeouts"] == 0, st


def _judge(key, z, ref, orc, s, alpha, M, N, iters):
    """All per-result assertions against the fp64 reference `ref` and the fp32 oracle's figures `orc` of the same case."""
    err_o, col_o, rank_o, zmax = orc
    tag = (key, z.shape, alpha, iters)
    assert np.isfinite(z).all(), tag
    err = float(np.abs(z.astype(np.float64) - ref).max())
    ulp = sr.ulp32(zmax)
    r = err / max(err_o, ulp)
    rank = sr.rank_residual(z, s, alpha) / (4.0 * rank_o + 8.0 * ulp)
    col = sr.column_residual(z, M, N) / (4.0 * col_o + 8.0 * ulp) if iters else 0.0  # (iters = 0: no column update has run)
    w = _worst.setdefault(key, [0.0, 0.0, 0.0])
    w[:] = [max(w[0], r), max(w[1], col), max(w[2], rank)]
    print("%s %dx%dx%d alpha %+.1f iters %2d: err %.2e (oracle %.2e, r %.2f)  column %.2f  rank %.2f of their bars" % (
        key, z.shape[0], M, N, alpha, iters, err, err_o, r, col, rank))
    assert err < HARD_BAR, (tag, err)
    assert r <= 3.0 * MEASURED_RATIO[key], (tag, r)
    assert col <= 1.0, (tag, col)
    assert rank <= 1.0, (tag, rank)
    rows_ok, cols_ok = sr.decided(ref)
    (zr, zc), (rr, rc) = sr.argmax_of_core(z), sr.argmax_of_core(ref)
    assert np.array_equal(zr[rows_ok], rr[rows_ok]) and np.array_equal(zc[cols_ok], rc[cols_ok]), tag


_PARAMS = [pytest.param(family, shape, alpha, path, id="%s-%s-a%s-%s" % (family, "x".join(map(str, shape)), alpha, path))
           for family, shape in sr.CASES for alpha in sr.ALPHAS for path in ("resident", "stream")]


@pytest.mark.parametrize("family,shape,alpha,path", _PARAMS)
def test_every_instance_at_its_smallest_shapes(gpu, family, shape, alpha, path):
    """One to three and twenty iterations (the chain: also none) behind the kernel the case is meant for."""
    import e2e_multi_view_matching_amd as E
    ctx = _ctx(gpu)
    B, M, N = shape
    pin, rows, _ = sr.FAMILIES[family]
    if path == "stream":
        pin, rows, key, iters_list = "stream", None, "stream", sr.ITERS_STREAM
    else:
        key, iters_list = family, sr.ITERS
    s = sr.scores(B, M, N)
    sg = s.to(gpu)
    ref, orc = sr.case_reference(B, M, N, alpha), sr.case_oracle(B, M, N, alpha)
    ctx.stats(reset=True)
    outs = {}
    with _pinned(ctx, pin):
        for iters in iters_list:
            _assert_plan(ctx, B, M, N, iters, rows)
            out = E.log_optimal_transport(sg, alpha, iters)
            assert torch.equal(out, E.log_optimal_transport(sg, alpha, iters)), iters  # fixed reduction orders: bit-identical
            outs[iters] = out.cpu().numpy()
    _no_events(ctx)  # the kernel itself produced this, not the rescue pass behind it
    for iters in iters_list:
        _judge(key, outs[iters], ref[iters], orc[iters], s.numpy(), alpha, M, N, iters)


def _batch_judge(key, out, s, alpha, iters):
    """Every problem of a large batch of small problems against fp64: the hard bar and the family's ratio bar."""
    B, M, N = s.shape
    z = out.cpu().numpy()
    ref = sr.sinkhorn_fp64(s.numpy(), alpha, iters)[0]
    err_o = float(np.abs(sr.oracle_fp32(s, alpha, iters).astype(np.float64) - ref).max())
    err = np.abs(z.astype(np.float64) - ref).reshape(B, -1).max(1)
    r = float(err.max()) / max(err_o, sr.ulp32(np.abs(ref).max()))
    print("%s %dx%dx%d: worst problem %d, err %.2e (oracle %.2e, r %.2f)" % (key, B, M, N, int(err.argmax()), err.max(), err_o, r))
    assert np.isfinite(z).all()
    assert float(err.max()) < HARD_BAR, int(err.argmax())
    assert r <= 3.0 * MEASURED_RATIO[key], r
    assert sr.rank_residual(z, s.numpy(), alpha) <= 4.0 * sr.rank_residual(sr.oracle_fp32(s, alpha, iters), s.numpy(), alpha) + 8.0 * sr.ulp32(np.abs(ref).max())


ROUNDS_ALPHA, ROUNDS_ITERS = 3.7, 3


@pytest.mark.parametrize("family,pin,rows,M,N", [("kt1", "rows64", 32, 4, 250), ("kt4", "rows64", 64, 4, 514),
                                                 ("regs128", "rows128", 128, 4, 514), ("regs2k", "rows128", 64, 4, 1026)])
def test_three_rounds_of_one_workgroup_problems(gpu, family, pin, rows, M, N):
    """2 R + 1 problems of one workgroup each, R = what the chip holds at a time: three rounds of the same workgroups, the last
    one nearly empty (epochs keep counting, LDS is reused, idle slots).  Every problem against fp64, and five of them - at the
    round boundaries - bit for bit as when they run alone."""
    import e2e_multi_view_matching_amd as E
    ctx = _ctx(gpu)
    with _pinned(ctx, pin):
        R = ctx.sinkhorn_plan(4096, M, N, ROUNDS_ITERS)[0]["resident_problems"]
        B = 2 * R + 1
        assert 2 <= R <= 1024, R
        assert ctx.sinkhorn_plan(B, M, N, ROUNDS_ITERS) == [{"rows_per_workgroup": rows, "problems": B, "resident_problems": R, "rounds": 3}]
        s = sr.scores(B, M, N, seed=11)
        sg = s.to(gpu)
        ctx.stats(reset=True)
        full = E.log_optimal_transport(sg, ROUNDS_ALPHA, ROUNDS_ITERS)
        assert torch.equal(full, E.log_optimal_transport(sg, ROUNDS_ALPHA, ROUNDS_ITERS))
        for b in (0, R - 1, R, 2 * R - 1, 2 * R):
            assert torch.equal(E.log_optimal_transport(sg[b:b + 1].contiguous(), ROUNDS_ALPHA, ROUNDS_ITERS)[0], full[b]), b
        _no_events(ctx)
    _batch_judge(family, full, s, ROUNDS_ALPHA, ROUNDS_ITERS)


@pytest.mark.parametrize("family,M,N,big_rows,base_rows", [("regs128", 4, 514, 128, 64), ("regs2k", 4, 1026, 64, 32)])
def test_two_segments_of_one_workgroup_problems(gpu, family, M, N, big_rows, base_rows):
    """Without a pin R + 3 problems are two launches: a full round of the register-addressed kernel and three problems on the
    compiler-allocated one, whose scores and potentials start at problem R (the segment's pointer offsets)."""
    import e2e_multi_view_matching_amd as E
    ctx = _ctx(gpu)
    with _pinned(ctx, "rows128"):
        R = ctx.sinkhorn_plan(4096, M, N, ROUNDS_ITERS)[0]["resident_problems"]
    B = R + 3
    plan = ctx.sinkhorn_plan(B, M, N, ROUNDS_ITERS)
    assert [(seg["rows_per_workgroup"], seg["problems"], seg["rounds"]) for seg in plan] == [(big_rows, R, 1), (base_rows, 3, 1)], plan
    s = sr.scores(B, M, N, seed=12)
    sg = s.to(gpu)
    ctx.stats(reset=True)
    full = E.log_optimal_transport(sg, ROUNDS_ALPHA, ROUNDS_ITERS)
    assert torch.equal(full, E.log_optimal_transport(sg, ROUNDS_ALPHA, ROUNDS_ITERS))
    _no_events(ctx)
    # each segment is the pinned kernel on its part of the batch, bit for bit
    with _pinned(ctx, "rows128"):
        assert torch.equal(E.log_optimal_transport(sg[:R].contiguous(), ROUNDS_ALPHA, ROUNDS_ITERS), full[:R])
    with _pinned(ctx, "rows64"):
        assert torch.equal(E.log_optimal_transport(sg[R:].contiguous(), ROUNDS_ALPHA, ROUNDS_ITERS), full[R:])
    # (the ratio bar of the looser of the two kernels that served the batch)
    key = max((family, "kt4" if N <= 1024 else "kt8"), key=lambda k: MEASURED_RATIO[k])
    _batch_judge(key, full, s, ROUNDS_ALPHA, ROUNDS_ITERS)


@pytest.mark.parametrize("pin,rows,N", [("rows64", 64, 514), ("rows128", 128, 514), ("rows64", 32, 1026), ("rows128", 64, 1026)])
def test_one_hostile_problem_among_healthy_ones(gpu, pin, rows, N):
    """Problem 1 of 3 leaves fp32's range in the exponential domain: the rescue pass re-solves it (counted, nothing raised) and
    its neighbours come out bit for bit as beside an ordinary problem."""
    import e2e_multi_view_matching_amd as E
    from e2e_multi_view_matching_amd import _lib
    ctx = _ctx(gpu)
    M, alpha = 64, 1.0
    seed, iters = sr.HOSTILE[N]
    s = sr.scores(3, M, N, seed=13)
    hostile = s.clone()
    hostile[1] = sr.scores(1, M, N, scale=HOSTILE_SCALE, seed=seed)[0]
    ref = sr.sinkhorn_fp64(hostile[1:2].numpy(), alpha, iters)[0]
    assert np.isfinite(ref).all()
    with _pinned(ctx, pin):
        ctx.stats(reset=True)
        _assert_plan(ctx, 3, M, N, iters, rows)
        healthy = E.log_optimal_transport(s.to(gpu), alpha, iters)
        _no_events(ctx)
        _assert_plan(ctx, 3, M, N, iters, rows)
        out = E.log_optimal_transport(hostile.to(gpu), alpha, iters)
        assert ctx.lib.e2emv_sync(ctx.h, None) == _lib.OK
        st = ctx.stats(reset=True)  # (two observed range events would demote the context to the chain: the reset takes this one back)
        _assert_plan(ctx, 3, M, N, iters, rows)  # back on the resident kernel for the next call
    assert st["sinkhorn_bad"] == 0 and st["sinkhorn_timeouts"] == 0, st
    assert st["sinkhorn_rescued"] == 1, st
    assert torch.equal(out[0], healthy[0]) and torch.equal(out[2], healthy[2])
    z = out[1:2].cpu().numpy()
    err = float(np.abs(z.astype(np.float64) - ref).max())
    print("hostile %s N %d scale %g iters %d: max |Z| %.0f, err %.2e, rescued %d" % (pin, N, HOSTILE_SCALE, iters, np.abs(ref).max(), err, st["sinkhorn_rescued"]))
    assert np.isfinite(z).all() and err < HOSTILE_BAR, err
    assert float(np.abs(healthy.cpu().numpy().astype(np.float64) - sr.sinkhorn_fp64(s.numpy(), alpha, iters)[0]).max()) < HARD_BAR


@pytest.mark.parametrize("B,M,N", [(2, 64, 516), (2, 33, 256)])
def test_scores_that_are_not_16_byte_aligned(gpu, B, M, N):
    """N % 4 == 0 but the score pointer is 4 bytes past a 16-byte boundary: the call copies the scores into its workspace first
    and must give, bit for bit, what it gives for an aligned tensor of the same values.  (The launcher itself refuses an
    unaligned pointer: a call that returns has gone through the copy.)"""
    import e2e_multi_view_matching_amd as E
    ctx = _ctx(gpu)
    flat = torch.zeros(B * M * N + 1, dtype=torch.float32, device=gpu)
    view = flat[1:].view(B, M, N)
    s = sr.scores(B, M, N, seed=14)
    view.copy_(s)
    aligned = s.to(gpu)
    assert view.data_ptr() % 16 == 4 and aligned.data_ptr() % 16 == 0 and view.is_contiguous()
    ctx.stats(reset=True)
    for alpha, iters in ((3.7, 2), (-2.5, 20), (1.0, 0)):
        a = E.log_optimal_transport(view, alpha, iters)
        assert torch.equal(a, E.log_optimal_transport(aligned, alpha, iters)), (alpha, iters)
        assert float(np.abs(a.cpu().numpy().astype(np.float64) - sr.sinkhorn_fp64(s.numpy(), alpha, iters)[0]).max()) < HARD_BAR
    assert torch.equal(view.cpu(), s) and float(flat[0]) == 0.0  # the scores and the float in front of them are untouched
    _no_events(ctx)


def test_report_of_the_measured_ratios():
    """Prints what the tests above measured (the figures behind MEASURED_RATIO / MEASURED_IDENTITY) and holds the constants to
    the rule: a ratio above 8 is a finding, not a tolerance."""
    for key, (r, col, rank) in sorted(_worst.items()):
        print("measured %-8s r %.2f (recorded %.2f)  column %.2f  rank %.2f of their bars" % (key, r, MEASURED_RATIO[key], col, rank))
    assert all(v <= 8.0 for v in MEASURED_RATIO.values()), MEASURED_RATIO
