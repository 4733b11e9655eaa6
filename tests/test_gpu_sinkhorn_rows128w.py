"""sinkhorn_resident128w (-m gpu): 128 rows x <= 1024 columns per workgroup on EIGHT waves, two per SIMD - 12 of a wave's 16
rows in v64 .. v255, 4 in LDS, the 8 partial column vectors folded through 16 KB (csrc/sinkhorn_regs2.hip).  Every case runs
under the pin "rows128w" (the pin "rows128" keeps meaning sinkhorn_resident128); that the kernel really ran is asserted from the
launcher's plan and from the statistics.

Reference: the fp64 restatement of tests/sinkhorn_restatement.py.  Bars: those tests/test_gpu_sinkhorn_edges.py applies to the
`regs128` family (the hard bar 1e-4, three times that family's recorded ratio to the fp32 oracle's own error, the two identities
of the result, the arg-max of the decided rows and columns) - its judge functions are called, nothing is re-chosen here."""
import functools

import numpy as np
import pytest
import torch

import sinkhorn_restatement as sr
import test_gpu_sinkhorn_edges as edges

pytestmark = pytest.mark.gpu

PIN, FAMILY, ROWS = "rows128w", "regs128", 128
ITERS = (1, 2, 5)   # both parities of the dustbin ping-pong (bufU), and the first iterations, where a wrong half-step still shows


def _judged(fn, *args, key=FAMILY):
    """edges._judge / edges._batch_judge under the regs128 bars, without booking this kernel's figures in that file's report of
    sinkhorn_resident128."""
    before = {k: list(v) for k, v in edges._worst.items()}
    try:
        fn(key, *args)
    finally:
        edges._worst.clear()
        edges._worst.update(before)


@functools.lru_cache(maxsize=4)
def _reference(B, M, N, alpha):
    """({iters: Z fp64}, {iters: the fp32 oracle's figures as sr.case_oracle gives them}) on sr.scores(B, M, N); computed once."""
    s = sr.scores(B, M, N)
    ref = {k: z for k, (z, _, _) in sr.sinkhorn_fp64_at(s.numpy(), alpha, ITERS).items()}
    orc = {}
    for k in ITERS:
        z32 = sr.oracle_fp32(s, alpha, k)
        orc[k] = (float(np.abs(z32.astype(np.float64) - ref[k]).max()), sr.column_residual(z32, M, N), sr.rank_residual(z32, s.numpy(), alpha),
                  float(np.abs(ref[k]).max()))
    return ref, orc


def _ran_on_the_new_kernel(ctx, calls):
    st = ctx.stats(reset=True)
    assert st["sinkhorn_rows128_calls"] == calls, st
    assert st["sinkhorn_rescued"] == 0 and st["sinkhorn_bad"] == 0 and st["sinkhorn_timeouts"] == 0, st


SHAPES = [
    (1, 128, 516),     # one workgroup, no exchange partner; the smallest column count of the class
    (2, 129, 516),     # two workgroups, the second with one valid row (the ragged instance)
    (1, 128, 1020),    # the last chunk partly empty, the dustbin column behind a chunk edge
    (2, 1024, 1024),   # the FULL instance: 8 workgroups per problem
]


@pytest.mark.parametrize("alpha", sr.ALPHAS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_against_fp64_at_the_edge_shapes(gpu, shape, alpha):
    import e2e_multi_view_matching_amd as E
    ctx = edges._ctx(gpu)
    B, M, N = shape
    s = sr.scores(B, M, N)
    sg = s.to(gpu)
    ref, orc = _reference(B, M, N, alpha)
    ctx.stats(reset=True)
    outs = {}
    with edges._pinned(ctx, PIN):
        for iters in ITERS:
            edges._assert_plan(ctx, B, M, N, iters, ROWS)
            out = E.log_optimal_transport(sg, alpha, iters)
            assert torch.equal(out, E.log_optimal_transport(sg, alpha, iters)), iters  # fixed reduction orders: the same bits twice
            outs[iters] = out.cpu().numpy()
    _ran_on_the_new_kernel(ctx, 2 * len(ITERS))
    for iters in ITERS:
        _judged(edges._judge, outs[iters], ref[iters], orc[iters], s.numpy(), alpha, M, N, iters)


def test_three_rounds_and_each_problem_alone(gpu):
    """More problems than resident slots: 2 R + 3 one-workgroup problems of 128 x 516, R = what the chip holds at a time - the
    same workgroups walk three rounds, the epochs run on (3 iterations per round: their parity alternates between rounds), LDS
    and the register rows are reused.  The problems at the round boundaries against fp64, and bit for bit as when they run alone."""
    import e2e_multi_view_matching_amd as E
    ctx = edges._ctx(gpu)
    M, N, alpha, iters = 128, 516, edges.ROUNDS_ALPHA, edges.ROUNDS_ITERS
    with edges._pinned(ctx, PIN):
        R = ctx.sinkhorn_plan(4096, M, N, iters)[0]["resident_problems"]
        B = 2 * R + 3
        assert 2 <= R <= 1024, R
        assert ctx.sinkhorn_plan(B, M, N, iters) == [{"rows_per_workgroup": ROWS, "problems": B, "resident_problems": R, "rounds": 3}]
        s = sr.scores(B, M, N, seed=21)
        sg = s.to(gpu)
        ctx.stats(reset=True)
        full = E.log_optimal_transport(sg, alpha, iters)
        assert torch.equal(full, E.log_optimal_transport(sg, alpha, iters))
        sample = [0, R - 1, R, 2 * R - 1, 2 * R, 2 * R + 2]
        for b in sample:
            assert torch.equal(E.log_optimal_transport(sg[b:b + 1].contiguous(), alpha, iters)[0], full[b]), b
        _ran_on_the_new_kernel(ctx, 2 + len(sample))
    assert bool(torch.isfinite(full).all())
    _judged(edges._batch_judge, full[sample], s[sample], alpha, iters)


def test_two_segments_new_kernel_and_the_64_row_kernel(gpu):
    """Without a pin R + 3 one-workgroup problems are two launches: a full round of sinkhorn_resident128w and three problems on
    the 64-row kernel.  Every problem against fp64; each segment is the pinned kernel on its part of the batch, bit for bit."""
    import e2e_multi_view_matching_amd as E
    ctx = edges._ctx(gpu)
    M, N, alpha, iters = 20, 516, edges.ROUNDS_ALPHA, edges.ROUNDS_ITERS
    with edges._pinned(ctx, PIN):
        R = ctx.sinkhorn_plan(4096, M, N, iters)[0]["resident_problems"]
    B = R + 3
    plan = ctx.sinkhorn_plan(B, M, N, iters)
    assert [(seg["rows_per_workgroup"], seg["problems"], seg["rounds"]) for seg in plan] == [(ROWS, R, 1), (64, 3, 1)], plan
    s = sr.scores(B, M, N, seed=22)
    sg = s.to(gpu)
    ctx.stats(reset=True)
    full = E.log_optimal_transport(sg, alpha, iters)
    assert torch.equal(full, E.log_optimal_transport(sg, alpha, iters))
    _ran_on_the_new_kernel(ctx, 2)
    with edges._pinned(ctx, PIN):
        assert torch.equal(E.log_optimal_transport(sg[:R].contiguous(), alpha, iters), full[:R])
    with edges._pinned(ctx, "rows64"):
        assert torch.equal(E.log_optimal_transport(sg[R:].contiguous(), alpha, iters), full[R:])
    key = max((FAMILY, "kt4"), key=lambda k: edges.MEASURED_RATIO[k])  # (the ratio bar of the looser of the two kernels)
    _judged(edges._batch_judge, full, s, alpha, iters, key=key)


def test_matches_equal_the_streaming_chains(gpu):
    """The fused row / column arg-max of the final sweep feeds the match block: the same matches behind sinkhorn_resident128w as
    behind the log-domain chain (516 keypoints: the smallest count whose five 128-row workgroups exchange an even column slice)."""
    from e2e_multi_view_matching_amd import MultiViewMatcher
    from e2e_multi_view_matching_amd.synthetic import identity_like_state, make_tuples
    ctx = edges._ctx(gpu)
    torch.manual_seed(0)
    model = identity_like_state(MultiViewMatcher({"GNN_layers": ["self", "cross"], "sinkhorn_iterations": 50, "conf_mlp": True}).eval()).to(gpu)
    data = {k: (v.to(gpu) if torch.is_tensor(v) else v) for k, v in make_tuples(batch=3, tuple_size=3, n_kpts=516, seed=2).items()}
    model.config["multi_frame_matching"] = True
    ctx.stats(reset=True)
    with edges._pinned(ctx, PIN):
        edges._assert_plan(ctx, 9, 516, 516, 50, ROWS)
        a = model(data)
        assert ctx.stats()["sinkhorn_rows128_calls"] >= 1
    with edges._pinned(ctx, "stream"):
        b = model(data)
    for k in a:
        if k.startswith("matches"):
            assert torch.equal(a[k], b[k]), k
        elif k.startswith("scores_"):
            assert float((a[k] - b[k]).abs().max()) < 2e-5, k
    assert float((a["matches0_0_1"] >= 0).float().mean()) > 0.5
    st = ctx.stats(reset=True)
    assert st["sinkhorn_rescued"] == 0 and st["sinkhorn_bad"] == 0 and st["sinkhorn_timeouts"] == 0, st


def test_exchange_while_a_second_stream_keeps_the_chip_busy(gpu):
    """Co-residency: the kernel's eight waves must find their register rows and LDS untouched, and the hand-offs must not depend
    on timing, while a second stream streams 2 GB copies over the same CUs and memory queues.  (Every wait of the exchange is
    bounded: a give-up would be counted and rescued, not hang.)"""
    import e2e_multi_view_matching_amd as E
    ctx = edges._ctx(gpu)
    B, N, iters = 8, 516, 25
    s = sr.scores(B, N, N, seed=23).to(gpu)
    with edges._pinned(ctx, PIN):
        edges._assert_plan(ctx, B, N, N, iters, ROWS)
        ctx.stats(reset=True)
        quiet = E.log_optimal_transport(s, 1.0, iters)
        side = torch.cuda.Stream(device=gpu)
        big = torch.empty(256 * 1024 * 1024, dtype=torch.float32, device=gpu)
        other = torch.empty_like(big)
        for rep in range(6):
            with torch.cuda.stream(side):
                for _ in range(4):
                    other.copy_(big)
                    big.add_(1.0)
            out = E.log_optimal_transport(s, 1.0, iters)
            assert torch.equal(out, quiet), rep
        torch.cuda.synchronize()
        _ran_on_the_new_kernel(ctx, 7)
