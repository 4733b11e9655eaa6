"""GPU: e2emv_image_front (csrc/image_front.hip) and its front prepare_images against the fp64 restatement of
tests/image_front_restatement.py, each case under the bar tests/test_image_front_api.py measured for it (4 x the distance of the
fp32 restatement from the fp64 one, not below 4 ulp of 1.0).

The kernel's tile is 16 output rows x 64 output columns and it stages 8 source rows at a time; the shapes of the cases put output
edges inside a tile (16 x 21, 37 x 50), on a tile's edge (48 x 64) and across several tiles with ragged last ones (131 x 203:
8 + 1 tiles of rows, 3 + 1 of columns); rows of 150 bytes start at every 16-byte misalignment."""
import ctypes
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import image_front_restatement as R  # noqa: E402
from test_image_front_api import ULP4, bar  # noqa: E402

pytestmark = pytest.mark.gpu

TILE_ROWS, TILE_COLS = 16, 64


def test_the_tile_is_the_headers():
    from e2e_multi_view_matching_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert "#define E2EMV_IMAGE_FRONT_TILE %d " % TILE_COLS in open(os.path.join(root, "include", "e2emv.h")).read()
    assert (_lib.IMAGE_FRONT_TILE_ROWS, _lib.IMAGE_FRONT_TILE) == (TILE_ROWS, TILE_COLS)
    H, W = R.CASES["tiles_aa0"]["out_size"]
    assert H > 2 * TILE_ROWS and H % TILE_ROWS and W > 2 * TILE_COLS and W % TILE_COLS


@functools.lru_cache(maxsize=None)
def _reference(name):
    """(image, arguments, fp64 gray, fp64 colour) of a case: computed once, shared, never written to."""
    img, kw = R.case_inputs(name)
    g64, c64 = R.image_front(img, torch.float64, **kw)
    return img, kw, g64, c64


def _launches(ctx, fn):
    """What fn() returns and the kernel launches the library counted while it ran (its profile slots)."""
    from e2e_multi_view_matching_amd import _lib
    ctx.call("e2emv_profile", 1)
    try:
        _lib.profile_read(ctx, reset=True)
        out = fn()
        n = sum(v["launches"] for v in _lib.profile_read(ctx, reset=True).values())
    finally:
        ctx.call("e2emv_profile", 0)
    return out, n


@pytest.mark.parametrize("name", list(R.CASES))
def test_case_within_its_bar(gpu, name):
    import e2e_multi_view_matching_amd as E
    from e2e_multi_view_matching_amd import _lib
    img, kw, g64, c64 = _reference(name)
    dev_img = img.to(gpu)
    (gray, rgb), n = _launches(_lib.context(gpu), lambda: E.prepare_images(dev_img, return_rgb=True, **kw))
    assert gray.dtype == torch.float32 and gray.is_contiguous() and tuple(gray.shape) == tuple(g64.shape) and gray.device == gpu
    assert rgb.dtype == torch.float32 and rgb.is_contiguous() and tuple(rgb.shape) == tuple(c64.shape)
    eg = float((gray.cpu().double() - g64).abs().max())
    ec = float((rgb.cpu().double() - c64).abs().max())
    print(f"{name}: gray within {eg:.3e}, colour within {ec:.3e} of fp64; bar {bar(name):.3e}; {n} launches")
    assert eg <= bar(name) and ec <= bar(name)
    # one launch unless an image of the call has a contrast slot, then three - whatever B is
    order = kw["order"]
    contrast = order is not None and 1 in torch.as_tensor(order).reshape(-1).tolist()
    assert n == (3 if contrast else 1)
    # without return_rgb: the same gray bytes
    assert torch.equal(E.prepare_images(dev_img, **kw), gray)


def test_bytes_without_resize_and_jitter(gpu):
    """ToTensor's true division and the gray sum in torch's order of roundings: byte-equal to the fp32 restatement on the CPU."""
    import e2e_multi_view_matching_amd as E
    img = R.all_values_image()
    for c in range(3):
        assert len(set(img[..., c].reshape(-1).tolist())) == 256
    want, _ = R.image_front(img, torch.float32)
    got = E.prepare_images(img.to(gpu))
    assert torch.equal(got.cpu(), want)
    # and through a window that pads and crops (rows of the image start at every misalignment)
    img = R.make_image(2, 37, 50, 40)
    for window in ((-2, 0, 41, 50), (3, 9, 30, 30), (-3, -4, 30, 40), (20, 30, 30, 40)):
        want, _ = R.image_front(img, torch.float32, window=window)
        assert torch.equal(E.prepare_images(img.to(gpu), window=window).cpu(), want), window
    # a view that starts 1 .. 3 bytes off (the first granule of the first row reaches in front of the tensor's first byte)
    flat = torch.zeros(2 * 37 * 50 * 3 + 16, dtype=torch.uint8, device=gpu)
    want, _ = R.image_front(img, torch.float32)
    for off in (1, 2, 3, 7):
        view = flat[off:off + img.numel()].view(img.shape)
        view.copy_(img)
        assert view.data_ptr() % 16 == off
        assert torch.equal(E.prepare_images(view).cpu(), want), off


def test_same_call_same_bytes(gpu):
    import e2e_multi_view_matching_amd as E
    img, kw, _, _ = _reference("tiles_aa1")
    assert 1 in kw["order"]
    dev_img = img.to(gpu)
    first = [t.clone() for t in E.prepare_images(dev_img, return_rgb=True, **kw)]
    other, okw, _, _ = _reference("three_rows")
    E.prepare_images(other.to(gpu), **okw)  # (another shape in between: the workspace is shared)
    for _ in range(3):
        again = E.prepare_images(dev_img, return_rgb=True, **kw)
        assert torch.equal(again[0], first[0]) and torch.equal(again[1], first[1])


def test_an_image_does_not_depend_on_its_batch(gpu):
    """The partial sums of the contrast mean are per image: image b of a batch = the same image alone."""
    import e2e_multi_view_matching_amd as E
    img, kw, _, _ = _reference("three_rows")
    dev_img = img.to(gpu)
    whole = E.prepare_images(dev_img, **kw)
    for b in range(3):
        alone = E.prepare_images(dev_img[b:b + 1], **{**kw, "order": kw["order"][b], "factors": kw["factors"][b]})
        assert torch.equal(alone[0], whole[b])


def test_c_errors_launch_nothing(gpu):
    from e2e_multi_view_matching_amd import _lib
    ctx = _lib.context(gpu)
    lib = ctx.lib
    B, H, W = 2, 8, 9
    img = R.make_image(B, H, W, 41).to(gpu)
    gray = torch.full((B, 1, 4, 5), 7.0, device=gpu)
    rgb = torch.full((B, 3, 4, 5), 7.0, device=gpu)
    s = _lib.stream_ptr(gpu)
    good = dict(batch=B, in_height=H, in_width=W, win_top=0, win_left=0, win_height=H, win_width=W, out_height=4, out_width=5, antialias=0)

    def call(order=(0, 1, 2, 3), factors=(1.0, 1.0, 1.0, 0.0), h=ctx.h, img_p=_lib.ptr(img), gray_p=_lib.ptr(gray), desc=True, **over):
        d = _lib.ImageFrontDesc(**{**good, **over})
        o = None if order is None else (ctypes.c_int32 * (4 * B))(*(list(order) * B if len(order) == 4 else list(order)))
        f = None if factors is None else (ctypes.c_float * (4 * B))(*(list(factors) * B if len(factors) == 4 else list(factors)))
        return lib.e2emv_image_front(h, ctypes.byref(d) if desc else None, img_p, o, f, gray_p, _lib.ptr(rgb), s)

    def refused(**kw):
        rc = call(**kw)
        msg = lib.e2emv_last_error(ctx.h).decode()
        return rc == _lib.EINVAL and "e2emv_image_front" in msg

    assert call(h=None) == _lib.EINVAL
    assert refused(desc=False) and refused(img_p=None) and refused(gray_p=None)
    for key in ("batch", "in_height", "in_width", "out_height", "out_width"):  # non-positive sizes
        assert refused(**{key: 0}) and refused(**{key: -3}), key
    assert refused(win_height=0) and refused(win_width=0) and refused(win_height=-1)  # an empty window
    assert refused(antialias=2)
    assert refused(order=(0, 1, 2, 4)) and refused(order=(-2, 1, 2, 3))  # an entry outside -1..3
    assert refused(order=(0, 1, 2, 3, 0, 2, 2, 3))  # an op named twice (in the second image)
    assert refused(order=None) and refused(factors=None)  # one without the other
    nan, inf = float("nan"), float("inf")
    for f in ((nan, 1, 1, 0), (1, inf, 1, 0), (1, 1, -inf, 0), (1, 1, 1, nan)):  # not finite
        assert refused(factors=f), f
    for f in ((-0.01, 1, 1, 0), (1, -0.01, 1, 0), (1, 1, -0.01, 0)):  # negative
        assert refused(factors=f), f
    assert refused(factors=(1, 1, 1, 0.500001)) and refused(factors=(1, 1, 1, -0.500001))  # hue outside [-0.5, 0.5]
    assert refused(factors=(1, 1, 1, 0, 1, 1, 1, 0.75))  # (in the second image)
    assert refused(order=(-1, -1, -1, -1), factors=(nan, 1, 1, 0))  # (a skipped op's factor is checked too)
    # a horizontal scale beyond the tile's source strip: the shape error, nothing launched either
    wide = torch.zeros((1, 4, 64 * 8, 3), dtype=torch.uint8, device=gpu)
    d = _lib.ImageFrontDesc(**{**good, "batch": 1, "in_height": 4, "in_width": 512, "win_height": 4, "win_width": 512, "out_height": 4, "out_width": 5})
    assert lib.e2emv_image_front(ctx.h, ctypes.byref(d), _lib.ptr(wide), None, None, _lib.ptr(gray), None, s) == _lib.ESHAPE
    torch.cuda.synchronize()
    assert bool((gray == 7.0).all()) and bool((rgb == 7.0).all())  # nothing was launched
    # and the good call goes through
    assert call() == _lib.OK and call(order=None, factors=None) == _lib.OK
    torch.cuda.synchronize()
    assert float(gray.max()) <= 1.0 and float(rgb.max()) <= 1.0


def test_feeds_superpoint_as_it_is(gpu):
    import e2e_multi_view_matching_amd as E
    img = R.make_image(2, 70, 90, 42).to(gpu)
    order, factors = E.color_jitter_params(0.2, 1, 2, generator=torch.Generator().manual_seed(1))
    gray = E.prepare_images(img, out_size=(64, 64), window=(3, 13, 64, 64), order=order, factors=factors)
    assert tuple(gray.shape) == (2, 1, 64, 64) and gray.dtype == torch.float32 and gray.is_contiguous() and gray.device == gpu
    assert gray.to(torch.float32).contiguous().data_ptr() == gray.data_ptr()  # what SuperPoint.forward does to its input: no copy
    torch.manual_seed(0)
    sp = E.SuperPoint({"max_keypoints": 32}).eval().to(gpu)
    out = sp({"image": gray})
    assert len(out["keypoints"]) == 2
    for k, d in zip(out["keypoints"], out["descriptors"]):
        assert k.shape[1] == 2 and d.shape[0] == 256 and k.shape[0] == d.shape[1] > 0
        assert bool(torch.isfinite(k).all()) and bool(torch.isfinite(d).all())
    assert float(gray.min()) >= 0.0 and float(gray.max()) <= 1.0 + ULP4
