"""The persistent tile walk of every layer GEMM kernel against fp64 (-m gpu): gemm_nt_kernel<false> (gemm.hip), gemm_x3_kernel,
gemm_h2_kernel<2> and <4>, and the five instances of gemm_p2_kernel (fp32 | planes, each with and without the residual, and
q|k + V^T), through ops.gemm_nt, ops.gemm_bf16x3 (e2emv_gemm_bf16x3_ex: two K segments and a residual, as MLP0 and MLP1 run these
kernels), ops.gemm_p2 and ops.qkv_p2.

The other kernel-level GEMM tests launch at most 36 tiles: one tile per workgroup.  Here every shape comes from the device's CU
count through tests/gemm_walk_plan.py (the launchers' grid rule and the kernels' walk restated; tests/test_gemm_walk_plan.py):
the smallest tile count, 3 column tiles wide and no multiple of 8, at which workgroups walk ONE, TWO and THREE tiles.  M is cut
to leave a ragged last row tile and N to leave a partial column tile (gemm_h2<4> excepted: it runs only at N % 256 == 0).  Each
case prints the CU count, the shape, the tile count and how many workgroups walk 1 / 2 / 3 tiles, asserts that mix and that the
case is not on gemm_nt's `small` path.  On 256 CUs:

  kernel       tile       tiles            M       N     workgroups walking 3 / 2 / 1
  gemm_h2<2>   256 x 128  171 x 3 = 513    43739   300   7 / 243 / 6
  gemm_h2<4>   256 x 256  171 x 3 = 513    43739   768   7 / 243 / 6
  gemm_p2      256 x 256  171 x 3 = 513    43739   672 (integers, planes), 43584 x 704 (exponents: whole 64 x 64 blocks), 341 x 128 x 768 (q|k|v)
  gemm_x3      128 x 128  342 x 3 = 1026   43739   300   7 / 500 / 5
  gemm_nt      128 x 128  513 x 3 = 1539   65627   300   7 / 757 / 4
  gemm_nt, batched        103 x (3 x 5) = 1545   103 x [347 x 556], scale 1/16, 14 / 749 / 5: a workgroup's next tile (+ 96) lies 6 or 7 batch
                          elements on, in another row tile and another column tile
  (with 3 column tiles the step + slots changes the row tile and the column tile for 32 and 64 slots; gemm_nt's 96 slots step
  whole rows of tiles in the unbatched case - the batched case, 5 column tiles, covers the column change for it)

(a) EXACT.  Operands, bias and residual are integers of magnitude <= 8: exact in every plane form (bf16 x 3, fp16 x 2, the scaled
    planes), every product and every partial sum exact in fp32 (|sum| <= 64 x 256 + 16 < 2^24; the weights' power-of-two scale
    and gemm_nt's scale 1/16 are exact), so the fp32 output EQUALS the fp64 product, in any order of summation: bad == 0.  A
    stale LDS slab, an accumulator not cleared, or a tile, row or k taken from the neighbouring tile cannot pass.  Each kernel
    plain (no bias) and full (bias, ReLU, A2, residual), over K = 32 nk:

      nk   [A | A2] of the full leg   what the walk does differently there
      1    32                         gemm_h2<2>: the load position is TWO TILES ahead (prologue loads of tile 2 before tile 0's
                                      epilogue), every step is a first step, the slabs and the next lstore share a buffer with one
                                      barrier between them; gemm_x3 / gemm_nt: setup(next) + gload(0) with no K loop in between;
                                      gemm_p2: `overlap` off, ev_next at the boundary
      2    32 | 32                    gemm_p2: `overlap` off (vmcnt(0) every step), the A2 segment is the tile's last step
      3    64 | 32                    gemm_p2: `overlap` on (load position two steps ahead across the epilogue, vmcnt(40) /
                                      vmcnt(32)), still nk < 4
      4    64 | 64                    gemm_p2: nk >= 4 (the next tile's side-band fetched at K step 2)
      8    128 | 128                  the layer shape's K per segment at a quarter of its length
    gemm_p2 (fp32 output, without and with residual + ReLU) runs the sweep on one segment and again on 32|32, 64|64, 128|128.

(b) AGAINST fp64 at the bars the suite already holds the same kernels to at one tile per workgroup, random operands with rows
    spanning decades, error relative to sum |a||w| + |b| (+ |r|); each test prints the worst error it sees:
      gemm_p2 plane output / plane output + residual        7.5e-7 / 1e-6   (test_gpu_gemm_p2_shape.py: test_fp32_and_plane_outputs,
                                                                             test_residual_outputs)
      qkv_p2, 128-row images, an odd image count            1e-6            (test_qkv_and_transposed_v): V^T is indexed by image
                                                                            across the walk, M is no multiple of 256
      gemm_p2 with tile exponents, residual, fp32 | planes  1.5e-6, planes relative to the 64 x 64 block's largest element too
                                                            (test_tile_exponents, its three `choices`): consecutive tiles of a
                                                            workgroup carry different A, A2 and residual exponents - what the
                                                            integers cannot make.  K 64|64 (nk = 4: ev_next fetched at step 2)
                                                            and K1 = 64 alone (nk = 2: fetched at the boundary); all finite
      gemm_h2<2>, gemm_h2<4> / gemm_x3 with A2 + residual   5e-7 / 4e-7     (test_gpu_kernels.py)

gemm_p2_chain_kernel shares gp_kstep / gp_epilogue with gemm_p2_kernel and is held bit-equal to its launches by
tests/test_gpu_round5.py while its workgroups walk two row blocks: with gemm_p2's walk pinned here, so is the chain's.

That these tests notice a broken walk was checked against libraries built with one line altered at a time (none changes an
address), this file run once on each.  The tests that went red (the kernel-level GEMM tests of test_gpu_kernels.py,
test_gpu_planes.py and test_gpu_gemm_p2_shape.py stayed green on all five: they never reach a second tile):
  gemm_h2: the __syncthreads() at the bottom of the      (a) gemm_h2<2> at every nk (1, 2, 3, 4, 8), (b) gemm_h2<2> with A2 +
   tile loop dropped                                     residual; gemm_h2<4> (separate slab region) and everything else green
  gemm_p2: `ev = ev_next` dropped (the first tile's      (b) the tile-exponent case, all three `choices`, at K 64|64 and at
   exponents kept for every tile of the walk)            K1 = 64 alone; the integer cases (no exponents) and everything else green
  gemm_x3: zero_acc() after the epilogue dropped         (a) gemm_x3 at every nk, (b) gemm_x3 with A2 + residual
  gemm_nt: setup(tile) for setup(next) (the next tile's  (a) gemm_nt at every nk, unbatched and batched
   operand rows taken from the current tile)
  gemm_p2: advance() calls setup(tile) for               every gemm_p2 case of (a) and (b), q|k|v included
   setup(ld_tile)

Measured on the MI355X (256 CUs), worst error of (b): planes 2.3e-7, planes + residual 2.8e-7, q|k|v 2.7e-7, tile exponents
1.1e-7 .. 2.5e-7, gemm_h2<2> 2.3e-7, gemm_h2<4> 2.0e-7, gemm_x3 2.9e-7; the 45 cases take 26 s together, the slowest 1.3 s."""
import functools

import pytest
import torch

import gemm_walk_plan as G

pytestmark = pytest.mark.gpu

CUT_M, CUT_N = 37, 84  # rows the last row tile and columns the last column tile are short of
CUT_N_P2 = 96          # (gemm_p2's residual and plane output take N % 32 == 0)
KMAX = 256
NKS = (1, 2, 3, 4, 8)
SPLIT = {1: (32, 0), 2: (32, 32), 3: (64, 32), 4: (64, 64), 8: (128, 128)}  # [A | A2] of the full leg


def _cus(gpu):
    return torch.cuda.get_device_properties(gpu).multi_processor_count  # (the count the context sizes its grids by)


def _announce(gpu, kernel, M, N, K, batch=1):
    """print the case and assert that its launch walks one, two and three tiles per workgroup"""
    cus = _cus(gpu)
    tm, tn, total = G.tiles(kernel, M, N, batch)
    slots, per_xcd, walks = G.plan(total, cus, G.KERNELS[kernel][0])
    have = G.mix(walks)
    print(f"{cus} CUs, {kernel}: {batch} x [{M} x {N} x {K}] = {batch} x {tm} x {tn} = {total} tiles on {8 * slots} workgroups "
          f"(+{slots} per step): walking 3 / 2 / 1 tiles: {have.get(3, 0)} / {have.get(2, 0)} / {have.get(1, 0)}")
    assert set(have) == {1, 2, 3}, have
    assert not G.nt_small(batch, M, N, cus)
    assert G.offsets_fit(kernel, M, N, K)


def _shape(gpu, kernel):
    """(M, N) of the unbatched walking case of a kernel: 3 column tiles, the last one partial where the kernel allows it"""
    bn = G.KERNELS[kernel][2]
    N = {"gemm_h2<4>": 3 * bn, "gemm_p2": 3 * bn - CUT_N_P2}.get(kernel, 3 * bn - CUT_N)
    return G.rows_for(kernel, _cus(gpu), 3, CUT_M), N


# ---- (a) exact on integers ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def _ints(M, N):
    g = torch.Generator().manual_seed(M + N)
    r = lambda *s: torch.randint(-8, 9, s, generator=g).float()
    return r(M, KMAX), r(N, KMAX), r(N), r(M, N)


def _run_exact(gpu, kernel, run, nk, split):
    """plain leg (one K segment, no bias) and full leg (bias, ReLU, [A | A2] = split, residual) of run(A, W, **kw) against fp64"""
    M, N = _shape(gpu, kernel)
    K = 32 * nk
    _announce(gpu, kernel, M, N, K)
    A, W, b, R = _ints(M, N)
    A, W = A[:, :K].contiguous(), W[:, :K].contiguous()
    core = A.double() @ W.double().T
    K1, K2 = split
    assert K1 + K2 == K
    legs = [("plain", {}, core),
            ("full", dict(bias=b.to(gpu), relu=True, residual=R.to(gpu), A2=A[:, K1:].contiguous().to(gpu) if K2 else None),
             (core + b.double()).clamp_min(0) + R.double())]
    Wd = W.to(gpu)
    for name, kw, ref in legs:
        A1 = A[:, :K1].contiguous() if kw.get("A2") is not None else A
        out = run(A1.to(gpu), Wd, **kw).cpu()
        bad = int((out != ref.float()).sum())
        print(f"  {name} {split if kw.get('A2') is not None else K}: elements that differ: {bad}")
        assert bad == 0, (kernel, name, nk, bad)


@pytest.mark.parametrize("nk", NKS)
def test_gemm_nt_walk_is_exact(gpu, nk):
    from e2e_multi_view_matching_amd import ops
    _run_exact(gpu, "gemm_nt", ops.gemm_nt, nk, SPLIT[nk])


@pytest.mark.parametrize("nk", NKS)
def test_gemm_nt_batched_walk_is_exact(gpu, nk):
    """shaped like the score matrix: per batch element mdesc_i mdesc_j^T / 16 on 3 x 5 tiles, so that a workgroup's consecutive
    tiles belong to different batch elements (and to different row and column tiles)"""
    from e2e_multi_view_matching_amd import ops
    cus = _cus(gpu)
    total = G.walk_shape(cus, 3, 15)
    Bt, M, N, K = total // 15, 3 * 128 - CUT_M, 5 * 128 - CUT_N, 32 * nk
    _announce(gpu, "gemm_nt", M, N, K, batch=Bt)
    slots = G.grid(total, cus, 3)[0]
    assert slots >= 15  # the next tile of a workgroup is in another batch element
    g = torch.Generator().manual_seed(nk)
    A = torch.randint(-8, 9, (Bt, M, K), generator=g).float()
    W = torch.randint(-8, 9, (Bt, N, K), generator=g).float()
    ref = (torch.bmm(A.double(), W.double().transpose(1, 2)) / 16).float()
    out = ops.gemm_nt(A.to(gpu), W.to(gpu), scale=1.0 / 16).cpu()
    bad = int((out != ref).sum())
    print(f"  scores: elements that differ: {bad}")
    assert bad == 0, bad
    R = torch.randint(-8, 9, (Bt, M, N), generator=g).float()
    out = ops.gemm_nt(A.to(gpu), W.to(gpu), scale=1.0 / 16, relu=True, residual=R.to(gpu)).cpu()
    bad = int((out != ref.clamp_min(0) + R).sum())
    print(f"  scores, ReLU + residual: elements that differ: {bad}")
    assert bad == 0, bad


@pytest.mark.parametrize("nk", NKS)
def test_gemm_x3_walk_is_exact(gpu, nk):
    from e2e_multi_view_matching_amd import ops
    _run_exact(gpu, "gemm_x3", ops.gemm_bf16x3, nk, SPLIT[nk])


@pytest.mark.parametrize("nk", NKS)
@pytest.mark.parametrize("kernel", ["gemm_h2<2>", "gemm_h2<4>"])
def test_gemm_h2_walk_is_exact(gpu, kernel, nk):
    from e2e_multi_view_matching_amd import ops
    _run_exact(gpu, kernel, functools.partial(ops.gemm_bf16x3, f16x2=True), nk, SPLIT[nk])


@pytest.mark.parametrize("nk,split", [(nk, (32 * nk, 0)) for nk in NKS] + [(2, (32, 32)), (4, (64, 64)), (8, (128, 128))])
def test_gemm_p2_walk_is_exact(gpu, nk, split):
    """fp32 output: without the residual (plain) and with bias, ReLU and the residual read from its planes (full)"""
    from e2e_multi_view_matching_amd import ops
    _run_exact(gpu, "gemm_p2", ops.gemm_p2, nk, split)


# ---- (b) against fp64 at the existing bars -------------------------------------------------------------------------------------------------
def _decades(g, M, N, K):
    """operands of test_gpu_kernels.py / test_gpu_gemm_p2_shape.py: activation rows spanning about four decades"""
    A = (torch.randn(M, K, generator=g) * torch.exp(torch.randn(M, 1, generator=g) * 2)).clamp(-6e4, 6e4)
    W = torch.randn(N, K, generator=g) / K ** 0.5
    b = torch.randn(N, generator=g)
    return A, W, b


def _err(out, ref, scale):
    return float(((out.double() - ref).abs() / scale).max())


@functools.lru_cache(maxsize=1)
def _p2_random(M, N, K1, K2):
    g = torch.Generator().manual_seed(M + N)
    A, W, b = _decades(g, M, N, K1 + K2)
    R = torch.randn(M, N, generator=g) * 3
    core = A.double() @ W.double().T + b.double()
    scale = (A.double().abs() @ W.double().abs().T) + b.double().abs()
    return A, W, b, R, core, scale


@pytest.mark.parametrize("residual", [False, True])
def test_gemm_p2_plane_output_walk(gpu, residual):
    from e2e_multi_view_matching_amd import ops
    M, N = _shape(gpu, "gemm_p2")
    K1 = K2 = 128
    _announce(gpu, "gemm_p2", M, N, K1 + K2)
    A, W, b, R, core, scale = _p2_random(M, N, K1, K2)
    relu = residual  # (one leg each: plain planes, ReLU + residual planes)
    ref = core.clamp_min(0) + R.double() if residual else core
    if residual:
        scale = scale + R.double().abs()
    out = ops.gemm_p2(A[:, :K1].contiguous().to(gpu), W.to(gpu), bias=b.to(gpu), relu=relu, A2=A[:, K1:].contiguous().to(gpu),
                      residual=R.to(gpu) if residual else None, planes_out=True).cpu()
    e = _err(out, ref, scale)
    print(f"  planes{' + residual' if residual else ''}: worst error {e:.3g}")
    assert e < 5e-7 + 2.5e-7 + (2.5e-7 if residual else 0.0), e


def test_qkv_p2_walk(gpu):
    from e2e_multi_view_matching_amd import ops
    cus = _cus(gpu)
    tiles_m = G.walk_shape(cus, 1, 3) // 3
    n_rows, D = 128, 256
    n_img = 2 * tiles_m - 1  # odd: the last row tile holds one image, M is no multiple of 256
    M = n_img * n_rows
    _announce(gpu, "gemm_p2", M, 3 * D, D)
    assert n_img % 2 == 1 and M % 256 == 128
    g = torch.Generator().manual_seed(n_img)
    X = torch.randn(M, D, generator=g) * torch.exp(torch.randn(M, 1, generator=g))
    W = torch.randn(3 * D, D, generator=g) / D ** 0.5
    b = torch.randn(3 * D, generator=g)
    ref = X.double() @ W.double().T + b.double()
    scale = (X.double().abs() @ W.double().abs().T) + b.double().abs()
    out = ops.qkv_p2(X.to(gpu), W.to(gpu), b.to(gpu), n_rows).cpu()
    e = _err(out, ref, scale)
    print(f"  q|k|v, {n_img} images of {n_rows} rows: worst error {e:.3g}")
    assert e < 1e-6, e


@pytest.mark.parametrize("choices", [(1e-8, 1.0), (1e-9, 1e-3, 1.0, 1e5, 2e9), (7e4, 3e12)])
@pytest.mark.parametrize("K1,K2", [(64, 64), (64, 0)])
def test_gemm_p2_tile_exponents_walk(gpu, choices, K1, K2):
    """the block scales of test_tile_exponents over the walk: the exponents of the A, A2 and residual blocks differ from one tile
    of a workgroup to its next"""
    from e2e_multi_view_matching_amd import ops
    cus = _cus(gpu)
    tiles_m = G.walk_shape(cus, 1, 3) // 3
    M, N, K = (tiles_m - 1) * 256 + 64, 3 * 256 - 64, K1 + K2  # whole 64 x 64 blocks: the last row tile has one, the last column tile three
    _announce(gpu, "gemm_p2", M, N, K)
    g = torch.Generator().manual_seed(len(choices) + K)

    def block_scales(rows, cols):
        idx = torch.randint(len(choices), (rows // 64, cols // 64), generator=g)
        return torch.tensor(choices, dtype=torch.float32)[idx].repeat_interleave(64, 0).repeat_interleave(64, 1)

    A = torch.randn(M, K, generator=g) * block_scales(M, K)
    W = torch.randn(N, K, generator=g) / K ** 0.5
    b = torch.randn(N, generator=g) * max(choices)
    R = torch.randn(M, N, generator=g) * block_scales(M, N)
    core = A.double() @ W.double().T + b.double()
    scale = (A.double().abs() @ W.double().abs().T) + b.double().abs() + R.double().abs()
    A1, A2 = A[:, :K1].contiguous().to(gpu), (A[:, K1:].contiguous().to(gpu) if K2 else None)
    for relu, planes_out in ((False, False), (True, True)):
        ref = (core.clamp_min(0) if relu else core) + R.double()
        out = ops.gemm_p2(A1, W.to(gpu), bias=b.to(gpu), relu=relu, A2=A2, residual=R.to(gpu), planes_out=planes_out, exponents=True).cpu()
        assert torch.isfinite(out).all()
        if planes_out:  # 22 bits relative to the largest element of the 64 x 64 block
            blk = ref.abs().view(M // 64, 64, N // 64, 64).amax((1, 3), keepdim=True).expand(M // 64, 64, N // 64, 64).reshape(M, N)
            e = _err(out, ref, scale + blk)
        else:
            e = _err(out, ref, scale)
        print(f"  exponents {choices} K {K1}|{K2} relu {relu} planes {planes_out}: worst error {e:.3g}")
        assert e < 1.5e-6, (choices, relu, planes_out, e)


@pytest.mark.parametrize("kernel,bar", [("gemm_h2<2>", 5e-7), ("gemm_h2<4>", 5e-7), ("gemm_x3", 4e-7)])
def test_split_gemm_two_segments_and_residual_walk(gpu, kernel, bar):
    from e2e_multi_view_matching_amd import ops
    M, N = _shape(gpu, kernel)
    K1 = K2 = 128
    _announce(gpu, kernel, M, N, K1 + K2)
    g = torch.Generator().manual_seed(M + N)
    A, W, b = _decades(g, M, N, K1 + K2)
    R = torch.randn(M, N, generator=g) * 3
    ref = (A.double() @ W.double().T + b.double()).clamp_min(0) + R.double()
    scale = (A.double().abs() @ W.double().abs().T) + b.double().abs() + R.double().abs()
    out = ops.gemm_bf16x3(A[:, :K1].contiguous().to(gpu), W.to(gpu), bias=b.to(gpu), relu=True, f16x2=kernel != "gemm_x3",
                          A2=A[:, K1:].contiguous().to(gpu), residual=R.to(gpu)).cpu()
    e = _err(out, ref, scale)
    print(f"  {kernel} [A | A2] + ReLU + residual: worst error {e:.3g}")
    assert e < bar, e
