"""gemm_p2 on the 16x16x32 MFMA shape (-m gpu): the fragment map of the K step (lane -> row lane & 15, k-chunk lane >> 4) and the
accumulator -> slab map of the epilogue (four 16 x 16 blocks per 32 x 32 slab block), through the Python entry points against
fp64, on shapes that reach every part of both maps: partial row tiles (M no multiple of 256 or 64), a partial column tile, one
and two K segments of 256, every output form (fp32, planes, planes + residual, q|k + V^T) and non-zero tile exponents.

The bars are those of tests/test_gpu_planes.py for the same outputs (relative to sum |a||w| + |b| (+ |r|)).  One case more has no
bar at all: small integers are exact in both planes, their products and sums are exact in fp32, so every output element must
EQUAL the integer product - any element that took a wrong row, column or k shows."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _case(g, M, N, K):
    A = torch.randn(M, K, generator=g) * torch.exp(torch.randn(M, 1, generator=g) * 2)
    A = A.clamp(-6e4, 6e4)
    W = torch.randn(N, K, generator=g) / K ** 0.5
    b = torch.randn(N, generator=g)
    return A, W, b


def _err(out, ref, scale):
    return float(((out.double() - ref).abs() / scale).max())


# (plane output and the residual need N % 32 == 0 at the entry point; fp32 output N % 4 == 0)
SHAPES = [(257, 224, 256, 0), (1000, 480, 256, 256), (333, 768, 512, 0), (65, 288, 256, 256)]


@pytest.mark.parametrize("M,N,K1,K2", SHAPES + [(257, 200, 256, 0), (190, 36, 256, 256)])
def test_fp32_and_plane_outputs(gpu, M, N, K1, K2):
    """no residual: fp32 output (bar 5e-7, test_gemm_p2_has_fp32_class_accuracy) and plane output (+ 2.5e-7: 22 bits)"""
    import e2e_multi_view_matching_amd as E
    g = torch.Generator().manual_seed(M + N + K1)
    A, W, b = _case(g, M, N, K1 + K2)
    A1, A2 = A[:, :K1].contiguous(), (A[:, K1:].contiguous() if K2 else None)
    core = A.double() @ W.double().T + b.double()
    scale = (A.double().abs() @ W.double().abs().T) + b.double().abs()
    for relu in (False, True):
        ref = core.clamp_min(0) if relu else core
        for planes_out in ((False, True) if N % 32 == 0 else (False,)):
            out = E.gemm_p2(A1.to(gpu), W.to(gpu), bias=b.to(gpu), relu=relu, A2=A2.to(gpu) if K2 else None, planes_out=planes_out).cpu()
            e = _err(out, ref, scale)
            print("fp32/planes", (M, N, K1, K2), relu, planes_out, e)
            assert e < 5e-7 + (2.5e-7 if planes_out else 0.0), (relu, planes_out, e)


@pytest.mark.parametrize("M,N,K1,K2", SHAPES)
def test_residual_outputs(gpu, M, N, K1, K2):
    """residual read from its planes (bars of test_gemm_p2_plane_epilogue_two_segments_residual)"""
    import e2e_multi_view_matching_amd as E
    g = torch.Generator().manual_seed(M + N)
    A, W, b = _case(g, M, N, K1 + K2)
    R = torch.randn(M, N, generator=g) * 3
    A1, A2 = A[:, :K1].contiguous(), (A[:, K1:].contiguous() if K2 else None)
    core = A.double() @ W.double().T + b.double()
    scale = (A.double().abs() @ W.double().abs().T) + b.double().abs() + R.double().abs()
    for relu in (False, True):
        ref = (core.clamp_min(0) if relu else core) + R.double()
        for planes_out in (False, True):
            out = E.gemm_p2(A1.to(gpu), W.to(gpu), bias=b.to(gpu), relu=relu, A2=A2.to(gpu) if K2 else None, residual=R.to(gpu),
                            planes_out=planes_out).cpu()
            e = _err(out, ref, scale)
            print("residual", (M, N, K1, K2), relu, planes_out, e)
            assert e < 5e-7 + 2.5e-7 + (2.5e-7 if planes_out else 0.0), (relu, planes_out, e)


@pytest.mark.parametrize("n_img,n_rows", [(3, 128), (1, 384), (5, 128)])
def test_qkv_and_transposed_v(gpu, n_img, n_rows):
    """q | k planes and V^T (bar of test_qkv_projection_attention_operand_epilogue); the entry point takes
    images of whole 128-row blocks, so M = n_img x n_rows is a multiple of 128: chosen to be no multiple of 256"""
    import e2e_multi_view_matching_amd as E
    g = torch.Generator().manual_seed(n_rows)
    D = 256
    X = torch.randn(n_img * n_rows, D, generator=g) * torch.exp(torch.randn(n_img * n_rows, 1, generator=g))
    W = torch.randn(3 * D, D, generator=g) / D ** 0.5
    b = torch.randn(3 * D, generator=g)
    ref = X.double() @ W.double().T + b.double()
    scale = (X.double().abs() @ W.double().abs().T) + b.double().abs()
    out = E.qkv_p2(X.to(gpu), W.to(gpu), b.to(gpu), n_rows).cpu()
    e = _err(out, ref, scale)
    print("qkv", (n_img, n_rows), e)
    assert e < 1e-6, e


@pytest.mark.parametrize("choices", [(1e-8, 1.0), (1e-9, 1e-3, 1.0, 1e5, 2e9), (7e4, 3e12)])
@pytest.mark.parametrize("M,N", [(320, 192), (576, 448)])
def test_tile_exponents(gpu, choices, M, N):
    """non-zero tile exponents on both K segments, the residual and the output (bar of
    test_gemm_p2_tile_exponents_carry_fp32_range; the side-band needs whole 64 x 64 blocks)"""
    import e2e_multi_view_matching_amd as E
    g = torch.Generator().manual_seed(len(choices) + M)
    K1 = K2 = 256

    def block_scales(rows, cols):
        idx = torch.randint(len(choices), (rows // 64, cols // 64), generator=g)
        return torch.tensor(choices, dtype=torch.float32)[idx].repeat_interleave(64, 0).repeat_interleave(64, 1)

    A = torch.randn(M, K1 + K2, generator=g) * block_scales(M, K1 + K2)
    W = torch.randn(N, K1 + K2, generator=g) / (K1 + K2) ** 0.5
    b = torch.randn(N, generator=g) * max(choices)
    R = torch.randn(M, N, generator=g) * block_scales(M, N)
    A1, A2 = A[:, :K1].contiguous(), A[:, K1:].contiguous()
    core = A.double() @ W.double().T + b.double()
    scale = (A.double().abs() @ W.double().abs().T) + b.double().abs() + R.double().abs()
    for relu, planes_out in ((False, False), (True, True), (False, True)):
        ref = (core.clamp_min(0) if relu else core) + R.double()
        out = E.gemm_p2(A1.to(gpu), W.to(gpu), bias=b.to(gpu), relu=relu, A2=A2.to(gpu), residual=R.to(gpu), planes_out=planes_out,
                        exponents=True).cpu()
        assert torch.isfinite(out).all()
        e = _err(out, ref, scale)
        if planes_out:  # 22 bits relative to the largest element of the 64 x 64 block
            blk = ref.abs().view(M // 64, 64, N // 64, 64).amax((1, 3), keepdim=True).expand(M // 64, 64, N // 64, 64).reshape(M, N)
            e = float(((out.double() - ref).abs() / (scale + blk)).max())
        print("exponents", choices, (M, N), relu, planes_out, e)
        assert e < 1.5e-6, (choices, relu, planes_out, e)


@pytest.mark.parametrize("M,N,K1,K2", [(257, 200, 256, 0), (330, 520, 256, 256)])
def test_integer_operands_are_exact(gpu, M, N, K1, K2):
    """Integers of magnitude <= 8: exact in the high planes (low planes zero), the weights' power-of-two scale is exact, every
    product and every partial sum (<= 64 x 512 + 8 < 2^24) is exact in fp32: the fp32 output EQUALS the integer product, whatever
    the order of the sums.  Each (row, column, k) weighs differently, so an element read from a wrong place cannot pass."""
    import e2e_multi_view_matching_amd as E
    g = torch.Generator().manual_seed(M)
    K = K1 + K2
    A = torch.randint(-8, 9, (M, K), generator=g).float()
    W = torch.randint(-8, 9, (N, K), generator=g).float()
    b = torch.randint(-8, 9, (N,), generator=g).float()
    ref = (A.double() @ W.double().T + b.double()).float()
    A1, A2 = A[:, :K1].contiguous(), (A[:, K1:].contiguous() if K2 else None)
    out = E.gemm_p2(A1.to(gpu), W.to(gpu), bias=b.to(gpu), A2=A2.to(gpu) if K2 else None).cpu()
    bad = int((out != ref).sum())
    print("integers", (M, N, K1, K2), "elements that differ:", bad)
    assert bad == 0, bad
