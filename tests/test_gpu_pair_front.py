"""GPU: e2emv_image_front_gray (csrc/image_front_pairs.hip) and its front prepare_pair_images against the float64 restatement of
tests/pair_front_restatement.py, each case under the bar tests/test_pair_front_api.py measures for it (4 x the distance of the
float32 restatement from the float64 one, not below 4 ulp of 1.0).

The kernel's tile is 32 x 32 output pixels; a tile stages the source lines its taps cover, or only the tapped ones beyond a
reduction by 2.  The cases (sized from the tile, see the restatement) put output edges inside a tile, on tile edges and across
several tiles with ragged last ones for each of the four turns, reduce by 2.01 (both ways of staging in one image), 5.4 and 8,
enlarge, and shrink an axis to one pixel; frames 37 bytes wide start their rows at every 16-byte misalignment."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pair_front_restatement as R  # noqa: E402
from test_pair_front_api import ULP4, bar  # noqa: E402

pytestmark = pytest.mark.gpu


def test_the_tile_is_the_headers():
    from e2e_multi_view_matching_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "e2emv.h")).read()
    assert "#define E2EMV_IMAGE_FRONT_GRAY_TILE_ROWS %d " % R.TILE_ROWS in hdr and "#define E2EMV_IMAGE_FRONT_GRAY_TILE_COLS %d " % R.TILE_COLS in hdr
    assert (_lib.IMAGE_FRONT_GRAY_TILE_ROWS, _lib.IMAGE_FRONT_GRAY_TILE_COLS) == (R.TILE_ROWS, R.TILE_COLS)
    assert "#define E2EMV_IMAGE_FRONT_GRAY_MAX_IMAGES %d " % _lib.IMAGE_FRONT_GRAY_MAX_IMAGES in hdr


@functools.lru_cache(maxsize=None)
def _reference(name):
    """(frames, turns, img_size, float64 outputs) of a case: computed once, shared, never written to."""
    frames, img_size = R.case_inputs(name)
    return [f for f, _ in frames], [r for _, r in frames], img_size, R.case_outputs(name, np.float64)


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
    frames, rots, img_size, want = _reference(name)
    dev = [torch.from_numpy(f).to(gpu) for f in frames]
    merge = name.startswith("merged")
    out, n = _launches(_lib.context(gpu), lambda: E.prepare_pair_images(dev, img_size, rots=rots, merge=merge))
    assert n == 1  # one launch whatever the list's length
    if merge:
        assert tuple(out.shape) == (len(frames), 1) + want[0].shape and out.dtype == torch.float32 and out.is_contiguous() and out.device == gpu
        out = [out[i:i + 1] for i in range(len(frames))]
    assert isinstance(out, list) and len(out) == len(frames)
    at = out[0].data_ptr()
    for i, (o, w64) in enumerate(zip(out, want)):
        assert o.dtype == torch.float32 and o.is_contiguous() and tuple(o.shape) == (1, 1) + w64.shape and o.device == gpu
        assert o.data_ptr() == at  # views of one allocation, in list order
        at += 4 * o.numel()
        err = float(np.abs(o[0, 0].cpu().numpy().astype(np.float64) - w64).max())
        print(f"{name}[{i}]: {frames[i].shape} rot {rots[i]} -> {w64.shape}: within {err:.3e} of float64; bar {bar(name):.3e}")
        assert err <= bar(name), (name, i, err)


def test_bytes_without_resize(gpu):
    """img_size == the longer side: uint8 / 255 of the turned image with the bytes of the fp32 division, for the four turns, at
    every misalignment of the rows (37 bytes a row) and of the frame's first byte."""
    import e2e_multi_view_matching_amd as E
    img = R.all_values_frame(45, 37, 80)
    flat = torch.zeros(45 * 37 + 32, dtype=torch.uint8, device=gpu)
    assert flat.data_ptr() % 16 == 0
    for off in (0, 1, 2, 3, 7, 15):
        view = flat[off:off + img.size].view(45, 37)
        view.copy_(torch.from_numpy(img))
        assert view.data_ptr() % 16 == off
        got = E.prepare_pair_images([view] * 4, 45, rots=[0, 1, 2, 3])
        for rot in range(4):
            want = np.rot90(img, k=rot).astype(np.float32) / np.float32(255)
            assert np.array_equal(got[rot][0, 0].cpu().numpy(), want), (off, rot)
    # several tiles per axis, and beside a resized image in the same call
    big = R.all_values_frame(70, 101, 81)
    other = R.make_frame(40, 50, 82)
    got = E.prepare_pair_images([torch.from_numpy(other).to(gpu), torch.from_numpy(big).to(gpu)], 101, rots=[0, 3])
    assert np.array_equal(got[1][0, 0].cpu().numpy(), np.rot90(big, k=3).astype(np.float32) / np.float32(255))
    assert tuple(got[0].shape) == (1, 1, 80, 101)
    # a non-contiguous frame is made contiguous
    wide = torch.from_numpy(R.make_frame(45, 74, 83)).to(gpu)
    got = E.prepare_pair_images([wide[:, ::2]], 45, rots=[1])
    assert np.array_equal(got[0][0, 0].cpu().numpy(), np.rot90(wide[:, ::2].cpu().numpy(), k=1).astype(np.float32) / np.float32(255))


def test_same_call_same_bytes(gpu):
    import e2e_multi_view_matching_amd as E
    frames, rots, img_size, _ = _reference("ragged_five")
    dev = [torch.from_numpy(f).to(gpu) for f in frames]
    first = [t.clone() for t in E.prepare_pair_images(dev, img_size, rots=rots)]
    o_frames, o_rots, o_size, _ = _reference("tiles_rot1")
    other = [torch.from_numpy(f).to(gpu) for f in o_frames]
    for _ in range(3):
        E.prepare_pair_images(other, o_size, rots=o_rots)  # (another shape set in between)
        again = E.prepare_pair_images(dev, img_size, rots=rots)
        assert all(torch.equal(a, b) for a, b in zip(again, first))


def test_an_image_does_not_depend_on_its_list(gpu):
    import e2e_multi_view_matching_amd as E
    frames, rots, img_size, _ = _reference("ragged_five")
    dev = [torch.from_numpy(f).to(gpu) for f in frames]
    whole = E.prepare_pair_images(dev, img_size, rots=rots)
    for i in range(len(dev)):
        assert torch.equal(E.prepare_pair_images([dev[i]], img_size, rots=[rots[i]])[0], whole[i])
    many = E.prepare_pair_images([dev[i % 5] for i in range(64)], img_size, rots=[rots[i % 5] for i in range(64)])  # 64 images in one call
    assert all(torch.equal(many[i], whole[i % 5]) for i in range(64))


def test_c_errors_launch_nothing(gpu):
    from e2e_multi_view_matching_amd import _lib
    ctx = _lib.context(gpu)
    lib = ctx.lib
    img = torch.from_numpy(R.make_frame(8, 9, 84)).to(gpu)
    out = torch.full((4096,), 7.0, device=gpu)
    s = _lib.stream_ptr(gpu)

    def call(n=2, h=ctx.h, recs=True, out_p=_lib.ptr(out), img_size=16, **over):
        arr = (_lib.GrayImage * max(n, 1))()
        for rec in arr:
            rec.data, rec.height, rec.width, rec.rot = img.data_ptr(), 8, 9, 0
        for k, v in over.items():  # (of the last record)
            setattr(arr[max(n, 1) - 1], k, v)
        return lib.e2emv_image_front_gray(h, n, arr if recs else None, img_size, out_p, s)

    def refused(code=_lib.EINVAL, **kw):
        rc = call(**kw)
        return rc == code and "e2emv_image_front_gray" in lib.e2emv_last_error(ctx.h).decode()

    assert call(h=None) == _lib.EINVAL
    assert refused(recs=False) and refused(out_p=None) and refused(data=None)
    assert refused(n=0) and refused(n=-1) and refused(n=_lib.IMAGE_FRONT_GRAY_MAX_IMAGES + 1)
    assert refused(height=0) and refused(width=-3) and refused(img_size=0) and refused(img_size=-5)
    assert refused(rot=4) and refused(rot=-1)
    assert refused(height=57, width=1, img_size=40)  # int((1 / 57) * 40) = 0 columns
    # beyond the limits: the shape error
    assert refused(_lib.ESHAPE, height=16385) and refused(_lib.ESHAPE, img_size=16385)
    assert refused(_lib.ESHAPE, height=16000, width=900, img_size=1000)  # a reduction by 16 (nothing is read: refused before the launch)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())  # nothing was launched
    # and the good call goes through: two images of 14 x 16
    assert call() == _lib.OK
    torch.cuda.synchronize()
    assert float(out[:2 * 14 * 16].max()) <= 1.0 and bool((out[2 * 14 * 16:] == 7.0).all())


def test_limits_that_must_hold(gpu):
    """A side of 16384, a reduction by 8 and an enlargement by 8 on both axes; the bars by the rule of the cases."""
    import e2e_multi_view_matching_amd as E

    def check(frame, rot, img_size, shape):
        got = E.prepare_pair_images([torch.from_numpy(frame).to(gpu)], img_size, rots=[rot])[0]
        w64, w32 = R.pair_front(frame, rot, img_size, np.float64), R.pair_front(frame, rot, img_size, np.float32)
        limit = max(4.0 * float(np.abs(w32.astype(np.float64) - w64).max()), ULP4)
        assert tuple(got.shape) == (1, 1) + shape == (1, 1) + w64.shape
        err = float(np.abs(got[0, 0].cpu().numpy().astype(np.float64) - w64).max())
        print(f"{frame.shape} rot {rot} -> {shape}: within {err:.3e} of float64; bar {limit:.3e}")
        assert err <= limit

    long = R.make_frame(16384, 16, 85)
    check(long, 0, 2048, (2048, 2))  # by 8 on both axes
    check(long, 1, 2048, (2, 2048))
    check(R.make_frame(20, 13, 86), 2, 160, (160, 104))  # enlarged by 8


def test_feeds_superpoint_as_it_is(gpu):
    import e2e_multi_view_matching_amd as E
    a, b = R.make_frame(100, 75, 87), R.make_frame(75, 100, 88)
    gray = E.prepare_pair_images([torch.from_numpy(a).to(gpu), torch.from_numpy(b).to(gpu)], 64, rots=[0, 1], merge=True)
    assert tuple(gray.shape) == (2, 1, 64, 48) and gray.dtype == torch.float32 and gray.is_contiguous() and gray.device == gpu
    assert gray.to(torch.float32).contiguous().data_ptr() == gray.data_ptr()  # what SuperPoint.forward does to its input: no copy
    want = torch.from_numpy(np.stack([R.pair_front(a, 0, 64, np.float32), R.pair_front(b, 1, 64, np.float32)])[:, None]).to(gpu)
    torch.manual_seed(0)
    sp = E.SuperPoint({"max_keypoints": 32}).eval().to(gpu)
    out, ref = sp({"image": gray}), sp({"image": want})
    assert len(out["keypoints"]) == 2
    for k, kr, d in zip(out["keypoints"], ref["keypoints"], out["descriptors"]):
        assert k.shape[1] == 2 and d.shape[0] == 256 and k.shape[0] == d.shape[1] > 0
        assert torch.equal(k, kr)  # the same keypoints as the restatement's image uploaded as float32
        assert bool(torch.isfinite(d).all())
    assert float(gray.min()) >= 0.0 and float(gray.max()) <= 1.0
