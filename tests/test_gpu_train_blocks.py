"""Training path, stage by stage (-m gpu): the kernels of csrc/train.hip / csrc/train_kernels.h behind the three building-block
entry points (train_ops.linear_backward / sinkhorn / attention_backward: the host functions the training forward and backward
call) against the fp64 restatement of tests/train_blocks_restatement.py, element by element, at the shapes where they can go
wrong - and two product-level cases through MultiViewMatcher.train() that reach kernel instances no other test reaches.
tests/test_train_blocks.py checks on the CPU that the restatement is autograd through the oracle and that the case lists reach
what they are meant to reach.

Bars.  Every compared quantity is computed three times on the same fp32 inputs: by the kernels, by the restatement in fp64 (the
reference) and by the restatement in fp32 on the CPU (the yardstick).  Both errors are taken against fp64 and divided by the
quantity's natural scale (below); the assertion is  err < k * err32 + floor,  never looser than what the suite already grants
the same quantity (cap).

    quantity   scale                                          cap
    logZ, uv   absolute                                       1e-4 (test_sinkhorn_vs_oracle, test_gpu_backward.py)
    dC         max |dC_ref| of the problem                    -
    dalpha     sum |dC_ref| over the dustbin row and column   -
    gemm       sum |a||b| (+ |c|) per element                 2e-6 (test_gpu_kernels.py)
    attention  max |dqkv_ref| per (image, head, q|k|v)        -

k and floor were measured once on the MI355X over the whole case list (the kernels use __expf / __logf and sum in another order
than torch: some factor is owed).  Rule: r = the worst err / err32 over the quarter of the cases with the largest err32 (where
the yardstick stands clear of its own noise), k = 4 r; floor = 4 x the largest amount by which any case exceeds r * err32 (the
cases where the fp32 restatement happened to land close to fp64).  Measured (n = compared values of that kind):

    quantity    n    worst err   worst err32   r      exceeds r*err32 by   k    floor
    gemm       240   5.9e-07     4.2e-07       2.23   3.0e-08               9   1.2e-07
    logZ       165   2.3e-05     2.1e-05       2.04   1.6e-06               8   6.6e-06
    uv         165   2.0e-05     1.6e-05       2.46   4.2e-07              10   1.7e-06
    dC         367   3.9e-05     2.3e-05       3.99   3.9e-06              16   1.6e-05
    dalpha     367   8.6e-06     6.0e-06       8.02   1.4e-06              32   6.0e-06
    attention   49   2.0e-05     8.0e-06       5.84   0                    23   4.8e-07 (4 ulp of the scale: not measured)

Where the worst values sit.  logZ / uv: 100 iterations and score scale 10.  dC: the monotonic score patterns at 20 iterations -
nearly all mass sits in the dustbins and max |dC| is small against the terms that cancel into it.  attention: N = 1 with two
keys (T = 3, cross) - dS = P (dP - sum P dP) is the difference of two numbers ~8 that agree to 1 %, 2e-5 of max |dq| on the
device against 3.4e-6 for the fp32 restatement; every other attention case has err / err32 <= 2.0 and err <= 1.1e-6.
"""
import functools

import pytest
import torch

import test_gpu_backward as GB
import train_blocks_restatement as R

pytestmark = [pytest.mark.gpu]

# quantity -> (k, floor, cap)
BARS = {
    "logZ": (8.0, 6.6e-6, 1e-4),
    "uv": (10.0, 1.7e-6, 1e-4),
    "dC": (16.0, 1.6e-5, None),
    "dalpha": (32.0, 6e-6, None),
    "gemm": (9.0, 1.2e-7, 2e-6),
    "attention": (23.0, 4.8e-7, None),
}


def _check(quantity, err, err32, where):
    k, floor, cap = BARS[quantity]
    bar = k * err32 + floor
    if cap is not None:
        bar = min(bar, cap)
    print(f"MEASURE {quantity} err={err:.3e} err32={err32:.3e} bar={bar:.3e} {where}")
    assert err < bar, (quantity, where, err, err32, bar)


# ------------------------------------------------------------------------------------------------------- linear backward
def _linear_run(gpu, form, rows, accumulate, integers=False, start=None):
    from e2e_multi_view_matching_amd import train_ops
    n_out, n_in, ldy, ldx, off = R.LINEAR_FORMS[form]
    bufY, bufX, W, bufD = R.linear_operands(form, rows, integers)
    gY, gX, gW, gD = bufY.to(gpu), bufX.to(gpu), W.to(gpu), bufD.to(gpu)
    dW0 = torch.zeros_like(W) if start is None else start[0]
    db0 = torch.zeros(n_out) if start is None else start[1]
    dW, db = dW0.to(gpu), db0.to(gpu)
    train_ops.linear_backward(gY[:, off:off + n_out], gX[:, :n_in], gW, dW, db, gD[:, :n_in], accumulate=accumulate)
    torch.cuda.synchronize()
    assert torch.equal(gD[:, n_in:].cpu(), bufD[:, n_in:]), "columns of the dX buffer behind n_in were written"
    assert torch.equal(gY.cpu(), bufY) and torch.equal(gX.cpu(), bufX) and torch.equal(gW.cpu(), W), "an input was written"
    dX0 = bufD[:, :n_in] if accumulate else None
    return (dW.cpu(), db.cpu(), gD[:, :n_in].cpu()), (bufY[:, off:off + n_out], bufX[:, :n_in], W, dX0), (dW0, db0)


@pytest.mark.parametrize("form", list(R.LINEAR_FORMS))
def test_linear_backward_against_fp64(gpu, form):
    """dW, db and dX of every form the backward calls, at row counts around the K step (32), the tile (64), the rows of a
    column-sum workgroup (64, four at a time) and the K ranges of the weight gradient (1, 2 and 3 of them; ragged), dX written and
    accumulated; operand rows spanning e^+-2 in magnitude."""
    for rows in R.LINEAR_ROWS:
        for accumulate in (False, True):
            got, (dY, X, W, dX0), _ = _linear_run(gpu, form, rows, accumulate)
            ref, scale = R.linear_backward(dY, X, W, dX0)
            ref32, _ = R.linear_backward(dY, X, W, dX0, dtype=torch.float32)
            for name, g, r, r32, s in zip(("dW", "db", "dX"), got, ref, ref32, scale):
                assert g.shape == r.shape and bool(g.isfinite().all()), name
                err = float(((g.double() - r).abs() / s).max())
                err32 = float(((r32.double() - r).abs() / s).max())
                _check("gemm", err, err32, f"{name} {form} rows={rows} accumulate={accumulate}")


@pytest.mark.parametrize("form", list(R.LINEAR_FORMS))
def test_linear_backward_integer_operands_are_exact(gpu, form):
    """Integers in [-8, 8] (every partial sum below 2^24, tests/test_train_blocks.py): dW and db added onto integers, dX
    accumulated onto integers, must equal the integer result whatever the order of the atomics."""
    n_out, n_in = R.LINEAR_FORMS[form][:2]
    g = torch.Generator().manual_seed(5)
    for rows in R.LINEAR_ROWS:
        start = (torch.randint(-8, 9, (n_out, n_in), generator=g).float(), torch.randint(-8, 9, (n_out,), generator=g).float())
        got, (dY, X, W, dX0), (dW0, db0) = _linear_run(gpu, form, rows, True, integers=True, start=start)
        (dW, db, dX), _ = R.linear_backward(dY, X, W, dX0)
        assert torch.equal(got[0].double(), dW + dW0.double()), (form, rows, "dW")
        assert torch.equal(got[1].double(), db + db0.double()), (form, rows, "db")
        assert torch.equal(got[2].double(), dX), (form, rows, "dX")


# -------------------------------------------------------------------------------------------------------------- Sinkhorn
@functools.lru_cache(maxsize=None)
def _sinkhorn_forward_refs(N, B, iters, pattern):
    S = R.sinkhorn_scores(B, N, pattern)
    return S, R.sinkhorn_tape(S, R.ALPHA, iters), R.sinkhorn_tape(S, R.ALPHA, iters, dtype=torch.float32)


@functools.lru_cache(maxsize=None)
def _sinkhorn_reverse_refs(N, B, iters, pattern, gpattern):
    S, (_, uv), (_, uv32) = _sinkhorn_forward_refs(N, B, iters, pattern)
    G = R.sinkhorn_G(B, N, gpattern)
    return G, R.sinkhorn_reverse(S, R.ALPHA, uv, G), R.sinkhorn_reverse(S, R.ALPHA, uv32, G, dtype=torch.float32)


def _sinkhorn_case(gpu, N, cw, B, iters, pattern, gpatterns):
    from e2e_multi_view_matching_amd import train_ops
    S, (logZ, uv), (logZ32, uv32) = _sinkhorn_forward_refs(N, B, iters, pattern)
    where = f"N={N} cw={cw} B={B} iters={iters} {pattern}"
    Sg = S.to(gpu)
    first = None
    for gp in gpatterns:
        G, (dC, dalpha), (dC32, dalpha32) = _sinkhorn_reverse_refs(N, B, iters, pattern, gp)
        out = {k: v.cpu() for k, v in train_ops.sinkhorn(Sg, R.ALPHA, iters, col_width=cw, G=G.to(gpu), tape=True, pad_value=1e30).items()}
        assert all(bool(v.isfinite().all()) for v in out.values()), (where, gp)
        if first is None:
            first = out
            _check("logZ", float((out["logZ"].double() - logZ).abs().max()), float((logZ32.double() - logZ).abs().max()), where)
            assert out["uv"].shape == uv.shape and float(out["uv"][:, 0].abs().max()) == 0.0
            _check("uv", float((out["uv"].double() - uv).abs().max()), float((uv32.double() - uv).abs().max()), where)
        else:  # (the forward does not depend on G, and it has no atomics: the same bits)
            assert torch.equal(out["logZ"], first["logZ"]) and torch.equal(out["uv"], first["uv"]), (where, gp)
        if gp == "zero":
            assert float(out["dC"].abs().max()) == 0.0 and float(out["dalpha"]) == 0.0, (where, gp)
            continue
        assert out["dC"].shape == dC.shape
        top = dC.abs().amax((1, 2), keepdim=True)
        assert float(top.min()) > 0
        _check("dC", float(((out["dC"].double() - dC).abs() / top).max()), float(((dC32.double() - dC).abs() / top).max()), f"{where} G={gp}")
        dust = float(dC[:, :N, N].abs().sum() + dC[:, N, :].abs().sum())
        _check("dalpha", abs(float(out["dalpha"].double() - dalpha)) / dust, abs(float(dalpha32.double() - dalpha)) / dust, f"{where} G={gp}")


@pytest.mark.parametrize("cw", R.SINKHORN_WIDTHS)
@pytest.mark.parametrize("N", R.SINKHORN_N)
def test_sinkhorn_tape_and_reverse_sweep(gpu, N, cw):
    """logZ, every (u_t, v_t) of the tape, dC with its dustbin row and column, and dalpha - both column-kernel instances at every
    size: fewer rows than row phases (N + 1 < 1024 / cw), every residue of N + 1 against the four-rows-per-workgroup kernels,
    one and several (ragged) column workgroups; B 1 and 3; 0, 1, 2 and 20 iterations; four score and four G patterns."""
    for B, iters, pattern, gpatterns in R.SINKHORN_VARIANTS:
        _sinkhorn_case(gpu, N, cw, B, iters, pattern, gpatterns)


@pytest.mark.parametrize("case", R.SINKHORN_EXTRA, ids=lambda c: f"N{c[0]}-cw{c[1]}-B{c[2]}-it{c[3]}")
def test_sinkhorn_long_tape_and_the_products_width_rule(gpu, case):
    """100 iterations at N = 65 (both widths), and col_width = 0: the rule the training forward and backward apply."""
    _sinkhorn_case(gpu, *case)


# ---------------------------------------------------------------------------------------------------- attention backward
def _attention_case(gpu, B, T, N, cross, spiked=False):
    from e2e_multi_view_matching_amd import train_ops
    H, D = 4, 256
    qkv, datt = R.attention_operands(B, T, N, H, spiked)
    ref = R.attention_backward(qkv, datt, B, T, N, H, cross)
    ref32 = R.attention_backward(qkv, datt, B, T, N, H, cross, dtype=torch.float32)
    got = train_ops.attention_backward(qkv.to(gpu), datt.to(gpu), B, T, N, H, cross).cpu()
    assert got.shape == ref.shape and bool(got.isfinite().all())
    assert float(got[:, N:].abs().max()) == 0.0, "padded rows of dqkv must be exactly zero"
    blocks = lambda x: x[:, :N].double().reshape(B * T, N, 3, H, 64)
    top = blocks(ref).abs().amax((1, 4), keepdim=True)  # per (image, q|k|v, head)
    # a query with ONE key (N = 1 and one source image): softmax = 1, dS = 1 * (dP - 1 * dP) = 0 in any arithmetic - dq and dk are exactly zero
    dead = (top == 0).expand_as(blocks(ref))
    assert bool(dead.any()) == (N == 1 and (T == 2 or not cross)) and float(blocks(got)[dead].abs().max() if dead.any() else 0.0) == 0.0
    top = top.clamp_min(1e-300)
    err = float(((blocks(got) - blocks(ref)).abs() / top).max())
    err32 = float(((blocks(ref32) - blocks(ref)).abs() / top)[~dead].max())
    _check("attention", err, err32, f"N={N} T={T} cross={cross} B={B} spiked={spiked}")


@pytest.mark.parametrize("T,cross", R.ATTENTION_MODES)
@pytest.mark.parametrize("N", R.ATTENTION_N)
def test_attention_backward_against_fp64(gpu, N, T, cross):
    """dqkv element by element: one and two source images (the probabilities of a query row span both: ldP = 2 N), keypoint
    counts around the 64-wide GEMM tile and the 4-rows-per-workgroup softmax kernels, the padded rows of q|k|v and d att holding
    1e30 (never read), the padded rows of dqkv exactly zero."""
    for B in R.ATTENTION_B:
        _attention_case(gpu, B, T, N, cross)


@pytest.mark.parametrize("T,cross", [(2, False), (3, True)])
def test_attention_backward_peaked_softmax(gpu, T, cross):
    """A key aligned with a query and scaled x 6: that row's softmax is one key to within e^-30."""
    _attention_case(gpu, 2, T, 65, cross, spiked=True)


# ------------------------------------------------------------------------------------------------------------------- API
def test_library_refuses_what_the_product_cannot_produce(gpu):
    from e2e_multi_view_matching_amd import _lib
    ctx = _lib.context(gpu)
    buf = torch.zeros(1 << 16, device=gpu)
    p, s, n = _lib.ptr(buf), _lib.stream_ptr(gpu), None
    f = ctx.lib.e2emv_train_sinkhorn
    ok = (ctx.h, 1, 8, p, 8, 0.5, 2, 0, n, p, n, n, n, s)

    def swap(args, i, v):
        return args[:i] + (v,) + args[i + 1:]
    assert f(*swap(ok, 2, 0)) == f(*swap(ok, 2, 2049)) == f(*swap(ok, 1, 0)) == f(*swap(ok, 4, 7)) == _lib.ESHAPE
    assert f(*swap(ok, 6, -1)) == _lib.EINVAL
    for cw in (1, 16, 33, 128, -64):
        assert f(*swap(ok, 7, cw)) == _lib.EINVAL
    assert f(*swap(ok, 3, n)) == f(*swap(ok, 9, n)) == _lib.EINVAL
    assert f(*swap(ok, 8, p)) == _lib.EINVAL  # G without dC / dalpha
    f = ctx.lib.e2emv_train_attention_backward
    ok = (ctx.h, 1, 2, 8, 256, 4, 1, p, p, p, s)
    assert f(*swap(ok, 3, 0)) == f(*swap(ok, 3, 2049)) == f(*swap(ok, 2, 1)) == f(*swap(ok, 2, _lib.MAX_TUPLE + 1)) == _lib.ESHAPE
    assert f(*swap(ok, 1, 0)) == f(*swap(ok, 5, 8)) == f(*swap(ok, 4, 128)) == _lib.ESHAPE
    assert f(*swap(ok, 7, n)) == f(*swap(ok, 8, n)) == f(*swap(ok, 9, n)) == _lib.EINVAL
    f = ctx.lib.e2emv_train_linear_backward
    ok = (ctx.h, 4, 2, 3, p, 2, p, 3, p, 3, p, p, p, 0, s)
    assert f(*swap(ok, 1, 0)) == f(*swap(ok, 2, 0)) == f(*swap(ok, 3, 0)) == _lib.ESHAPE
    assert f(*swap(ok, 5, 1)) == f(*swap(ok, 7, 2)) == f(*swap(ok, 9, 2)) == _lib.ESHAPE
    for i in (4, 6, 8, 10, 11):
        assert f(*swap(ok, i, n)) == _lib.EINVAL
    torch.cuda.synchronize()
    assert float(buf.abs().max()) == 0.0, "a refused call wrote"


def test_a_tape_in_the_context_survives_the_block_calls(gpu):
    """forward_train, then all three blocks, then the backward of that forward: the gradients of a run without the blocks in
    between (the score gradients up to the order of the atomics, as test_device_side_weight_update_equals_the_host_commit)."""
    from e2e_multi_view_matching_amd import MultiViewMatcher, train_ops
    from e2e_multi_view_matching_amd.synthetic import make_tuples
    torch.manual_seed(2)
    model = MultiViewMatcher({"GNN_layers": ["self", "cross"], "sinkhorn_iterations": 10, "frozen_batchnorm": True}).to(gpu).train()
    data = {k: (v.to(gpu) if torch.is_tensor(v) else v) for k, v in make_tuples(batch=1, tuple_size=2, n_kpts=128, seed=2).items()}
    idx, w = GB._targets(1, 128, 20)
    idx, w = idx.to(gpu), w.to(gpu)

    def run(between):
        model.zero_grad()
        scores = model(data)["scores_0_1"]
        between()
        GB._match_loss(scores, idx, w).backward()
        return scores.detach().clone(), {k: p.grad.detach().clone() for k, p in model.named_parameters()}

    def blocks():
        _sinkhorn_case(gpu, 65, 64, 3, 2, "random1", ("dense",))
        _attention_case(gpu, 1, 3, 65, True)
        _linear_run(gpu, "mlp0", 400, False)

    s0, g0 = run(lambda: None)
    s1, g1 = run(blocks)
    assert torch.equal(s0, s1)
    scale = max(float(g.norm()) for g in g0.values())
    for k in g0:
        d = float((g0[k] - g1[k]).norm()) / max(float(g0[k].norm()), 1e-4 * scale)
        assert d < 1e-4, (k, d)


# --------------------------------------------------------------------------------------------------------- product level
def test_a_batch_that_fills_the_chip_takes_the_64_column_sinkhorn_kernels(gpu):
    """As many pairs as the chip has compute units at N = 63: B * ceil((N + 1) / 64) workgroups of 64 columns fill it, so the
    training forward and backward themselves run skt_col_kernel<64> / skb_uhalf_kernel<64> (every other training test stays on
    the 32-column instances).  Bars of test_gpu_backward.py."""
    B, N = torch.cuda.get_device_properties(gpu).multi_processor_count, 63
    assert B * ((N + 1 + 63) // 64) >= torch.cuda.get_device_properties(gpu).multi_processor_count
    assert R.col_width_of(B, N, B) == 64
    cfg = {"GNN_layers": ["self", "cross"], "sinkhorn_iterations": 20, "frozen_batchnorm": True}
    model, leaves, out, ref, pairs = GB._grads(cfg, dict(batch=B, tuple_size=2, n_kpts=N), gpu, seed=6)
    z, zr = out["scores_0_1"].detach().cpu(), ref["scores_0_1"].detach()
    assert float((z - zr).abs().max()) < 1e-4
    worst = GB._check(model, leaves)
    assert len(worst) == sum(1 for _ in model.parameters())


POSE_CASE = dict(B=2, N=200, data_seed=10)  # (tests/test_train_blocks.py: how the seed was chosen)


def test_pose_loss_with_200_keypoints_reaches_the_conf_head_at_400_rows(gpu):
    """conf_mlp with the pose term at N = 200, B = 2: the conf head's wgrad / dgrad / colsum run over rows = 400 (a ragged last K
    step; every other test hands them multiples of 128), the single output channel of conf_mlp.3 included, and conf_scatter_kernel
    meets unmatched rows.  Bars of test_gpu_backward.py.  The keypoints are make_tuples(seed=10), not the 9 of the 256-keypoint
    test: at seed 9 the gradient of conf_mlp.3.bias, the sum of d z over the matched rows, cancels to 4.7e-4 out of sum |d z| =
    9.8 - the fp32 oracle itself is 1.4e-4 off the fp64 oracle there, and the device, inside the bar in four runs, missed it with 1.02e-3 in
    a fifth (the order of the atomics): half an ulp of the terms.  The CPU file asserts that at seed 10 the reference
    stands 100 x clear of the bar for every parameter."""
    out, ref = GB._pose_loss_end_to_end(gpu, **POSE_CASE)
    m = ref["matches0_0_1"]
    assert int((m < 0).sum()) > 0 and int((m >= 0).sum()) > 0
