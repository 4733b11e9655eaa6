"""The fused front of the f16x2 plane forward (csrc/kenc_fused.hip) against the launches it replaces (-m gpu).

ingest_transpose, the four keypoint-encoder GEMMs and to_planes_exp_kernel in ONE launch behind ingest_kenc0 that keeps every
intermediate on chip.  The kernel is written to run every output element through the same instructions in the same order, so
the comparison is on BYTES: the planes of x, their tile exponents and the block maxima through e2emv_encode_planes, and every
output tensor of a whole matcher forward.  Shapes sit on the kernel's block edges (128 rows per workgroup, 64 x 64 exponent
blocks, 32-row MFMA tiles): 1, 63, 64, 65, 128, 129 keypoints, a 3 x 3 batch of tuples (image indexing), and two images with
different keypoint counts and sizes."""
import pytest
import torch

pytestmark = pytest.mark.gpu

D = 256


@pytest.fixture(scope="module")
def front(gpu):
    """(context, model) with random weights and BatchNorm statistics committed, on the f16x2 plane kernels at every size"""
    import e2e_multi_view_matching_amd as E
    from test_gpu_matcher import _randomize_bn
    torch.manual_seed(7)
    model = E.MultiViewMatcher({"sinkhorn_iterations": 5, "conf_mlp": True, "match_threshold": 0.2, "GNN_layers": ["self", "cross"]}).eval()
    _randomize_bn(model, 7)
    model = model.to(gpu)
    ctx = E._lib.context(gpu)
    ctx.set_split_min_rows(0)
    before = ctx.precision()
    ctx.call("e2emv_set_precision", E._lib.PRECISION_F16X2)
    model._push_weights(ctx)
    try:
        yield ctx, model
    finally:
        ctx.set_kenc_fused(True)
        ctx.call("e2emv_set_precision", before)
        ctx.set_split_min_rows(-1)


def _inputs(gpu, B, Ns, sizes, dtype, layout, seed):
    """keypoints, scores, descriptors per image and the forward descriptor.  layout: "random" = normalised descriptors, "scaled"
    = every third keypoint's descriptor times 2^20 and every fifth's times 2^-30 (block maxima outside the exponents' dead
    zone), "integers" = descriptors that are small integers"""
    import e2e_multi_view_matching_amd as E
    g = torch.Generator().manual_seed(seed)
    fd = E._lib.ForwardDesc()
    kpts, scores, descs = [], [], []
    for m, (n, (w, h)) in enumerate(zip(Ns, sizes)):
        kpts.append((torch.rand((B, n, 2), generator=g) * torch.tensor([w, h])).to(gpu))
        scores.append(torch.rand((B, n), generator=g).to(gpu))
        d = torch.randn((B, D, n), generator=g)
        if layout == "integers":
            d = torch.randint(-8, 9, (B, D, n), generator=g).float()
        else:
            d = torch.nn.functional.normalize(d, dim=1)
        if layout == "scaled":
            d[:, :, ::3] *= 2.0 ** 20
            d[:, :, 1::5] *= 2.0 ** -30
        descs.append(d.to(dtype).contiguous().to(gpu))
        fd.img_w[m], fd.img_h[m] = float(w), float(h)
        fd.n_kpts_img[m] = n
    fd.batch, fd.tuple_size, fd.n_kpts = B, len(Ns), max(Ns)
    fd.sinkhorn_iters, fd.match_threshold = 5, 0.2
    fd.desc_dtype = E._lib.DESC_F16 if dtype == torch.float16 else E._lib.DESC_F32
    fd.flags = E._lib.FLAG_FULL_OUTPUT | (E._lib.FLAG_MULTI_FRAME if len(Ns) > 2 else 0)
    return fd, kpts, scores, descs


def _both(ctx, gpu, args):
    """(unfused, fused) outputs of e2emv_encode_planes, the launch counter of the fused kernel read around each"""
    import e2e_multi_view_matching_amd as E
    ctx.call("e2emv_set_precision", E._lib.PRECISION_F16X2)  # (a model's forward selects its own on every call)
    ctx.stats(reset=True)
    ctx.set_kenc_fused(False)
    ref = ctx.encode_planes(*args)
    st_ref = ctx.stats()
    assert st_ref["kenc_fused_launches"] == 0
    ctx.stats(reset=True)
    ctx.set_kenc_fused(True)
    out = ctx.encode_planes(*args)
    st = ctx.stats()
    assert st["kenc_fused_launches"] == 1
    return ref, out, st_ref, st


def _assert_bytes_equal(ref, out):
    for name, a, b in zip(("planes", "exponents", "block maxima"), ref, out):
        # (the maxima as their bit patterns: equal bytes, whatever the value)
        a, b = (a.view(torch.int32), b.view(torch.int32)) if a.dtype == torch.float32 else (a, b)
        assert torch.equal(a, b), (name, int((a != b).sum()), a.numel())


SHAPES = [(1, [1, 1]), (1, [63, 63]), (1, [64, 64]), (1, [65, 65]), (1, [128, 128]), (1, [129, 129]), (3, [200, 200, 200]), (2, [100, 37])]


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["desc_f32", "desc_f16"])
@pytest.mark.parametrize("B,Ns", SHAPES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, list) else str(v))
def test_fused_encoder_planes_equal_the_stages_byte_for_byte(gpu, front, B, Ns, dtype):
    ctx, _ = front
    sizes = [(640.0, 480.0), (512.0, 384.0)] if Ns == [100, 37] else [(640.0, 480.0)] * len(Ns)
    ref, out, _, st = _both(ctx, gpu, _inputs(gpu, B, Ns, sizes, dtype, "random", 11 + sum(Ns)))
    assert st["rescaled_blocks"] == 0  # an ordinary input: every block inside the dead zone
    _assert_bytes_equal(ref, out)
    assert int((out[0] != 0).sum()) > 0


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["desc_f32", "desc_f16"])
def test_fused_encoder_carries_the_tile_exponents(gpu, front, dtype):
    """descriptors far outside the dead zone of the tile exponents (fp16 descriptors: up to fp16's own range): the stages
    rescale blocks - checked first, so that the case is known to reach that arm - and the fused kernel picks the same exponents"""
    ctx, _ = front
    fd, kpts, scores, descs = _inputs(gpu, 2, [200, 200], [(640.0, 480.0)] * 2, torch.float32, "scaled", 5)
    if dtype == torch.float16:
        descs = [(d * 0.25).clamp(-60000.0, 60000.0).to(torch.float16) for d in descs]  # (2^18 |d|, cut off inside fp16's range)
        fd.desc_dtype = 1
    ref, out, st_ref, st = _both(ctx, gpu, (fd, kpts, scores, descs))
    assert st_ref["rescaled_blocks"] > 0
    assert st["rescaled_blocks"] == st_ref["rescaled_blocks"]
    assert int((ref[1] != 0).sum()) > 0
    _assert_bytes_equal(ref, out)


def test_fused_encoder_on_exactly_representable_descriptors(gpu, front):
    ctx, _ = front
    ref, out, _, _ = _both(ctx, gpu, _inputs(gpu, 2, [130, 130], [(640.0, 480.0)] * 2, torch.float32, "integers", 3))
    _assert_bytes_equal(ref, out)


@pytest.mark.parametrize("N", [128, 100])
def test_whole_matcher_outputs_equal_with_and_without_the_fused_front(gpu, front, N):
    import e2e_multi_view_matching_amd as E
    from e2e_multi_view_matching_amd.synthetic import make_tuples
    ctx, model = front
    data = {k: (v.to(gpu) if torch.is_tensor(v) else v) for k, v in make_tuples(seed=N, batch=2, tuple_size=2, n_kpts=N).items()}
    model.config["mfma_precision"] = "f16x2"
    outs = []
    for fused in (False, True):
        ctx.set_kenc_fused(fused)
        ctx.stats(reset=True)
        with torch.no_grad():
            out = model(data)
        md = E.last_descriptors(gpu)
        assert ctx.stats()["kenc_fused_launches"] == (1 if fused else 0)
        outs.append((out, md))
    (ref, md_ref), (out, md) = outs
    assert out.keys() == ref.keys() and any(torch.is_tensor(v) for v in ref.values())
    assert torch.equal(md, md_ref)
    for k, v in ref.items():
        if torch.is_tensor(v):
            assert torch.equal(out[k], v), k


def test_other_modes_keep_the_launch_per_stage(gpu, front, monkeypatch):
    """E2EMV_KENC=unfused at context creation, and the fp32 arithmetic on the default context: the forward runs, the fused
    kernel is never launched"""
    import e2e_multi_view_matching_amd as E
    from e2e_multi_view_matching_amd.synthetic import make_tuples
    ctx, model = front
    data = {k: (v.to(gpu) if torch.is_tensor(v) else v) for k, v in make_tuples(seed=1, batch=2, tuple_size=2, n_kpts=100).items()}
    ctx.set_kenc_fused(True)
    ctx.stats(reset=True)
    model.config["mfma_precision"] = "f32"
    with torch.no_grad():
        out = model(data)
    assert torch.isfinite(out["scores_0_1"]).all()
    assert ctx.stats()["kenc_fused_launches"] == 0
    model.config["mfma_precision"] = "f16x2"

    monkeypatch.setenv("E2EMV_KENC", "unfused")
    other = E._lib.Context(gpu.index)  # (a context of its own: the variable is read at creation)
    other.set_split_min_rows(0)
    other.call("e2emv_set_precision", E._lib.PRECISION_F16X2)
    model._push_weights(other)
    args = _inputs(gpu, 1, [65, 65], [(640.0, 480.0)] * 2, torch.float32, "random", 2)
    got = other.encode_planes(*args)
    assert other.stats()["kenc_fused_launches"] == 0
    ctx.set_kenc_fused(True)
    ctx.call("e2emv_set_precision", E._lib.PRECISION_F16X2)
    ctx.stats(reset=True)
    model._push_weights(ctx)
    ref = ctx.encode_planes(*args)
    assert ctx.stats()["kenc_fused_launches"] == 1
    _assert_bytes_equal(ref, got)
