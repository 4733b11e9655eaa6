"""CPU: the restatement of the image front (tests/image_front_restatement.py) against colorsys and its own identities, the host
side of e2e_multi_view_matching_amd.images (parameter draws, intrinsics, argument errors) and THE BARS of tests/test_gpu_image_front.py:
per GPU case the largest distance of the fp32 restatement (the reference's arithmetic) from the fp64 one, measured here."""
import colorsys
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import image_front_restatement as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Per case of tests/test_gpu_image_front.py: max |fp32 restatement - fp64 restatement| over the gray and the colour output, as
# measured on the CPU (the value beside each constant), rounded up.  The device's bar for the case is 4 times the constant - for
# its contraction and its other summation order in the taps and in the mean - and not below 4 ulp of 1.0.
# (The resize cases without antialias are the coarse ones: aten computes the source index of a column in fp32, 6e-5 at column 1000.)
FP32_DISTANCE = {
    "down_aa0": 1.8e-06,              # 1.721e-06
    "up_aa0": 2.3e-06,                # 2.217e-06
    "tiles_aa0": 7.5e-05,             # 7.471e-05
    "down_aa1": 3.4e-07,              # 3.379e-07
    "up_aa1": 2.3e-06,                # 2.217e-06
    "tiles_aa1": 1.9e-05,             # 1.835e-05
    "noresize": 1.2e-07,              # 1.144e-07
    "noresize_tiles": 1.2e-06,        # 1.197e-06
    "window_pad": 1.2e-06,            # 1.102e-06
    "window_pad_noresize": 1.2e-07,   # 1.136e-07
    "window_crop": 1.5e-07,           # 1.423e-07
    "window_crop_noresize": 1.1e-07,  # 1.028e-07
    "window_over": 8.3e-08,           # 8.239e-08
    "window_over_noresize": 9.7e-08,  # 9.672e-08
    "orders24": 3.7e-06,              # 3.641e-06
    "orders24_noresize": 9.5e-07,     # 9.447e-07
    "skipped": 5.3e-07,               # 5.270e-07
    "contrast_first_last": 3.0e-06,   # 2.952e-06
    "contrast_absent": 3.1e-06,       # 3.046e-06
    "three_rows": 3.7e-06,            # 3.688e-06
    "broadcast_row": 3.6e-06,         # 3.554e-06
    "extremes": 2.4e-06,              # 2.307e-06
    "frame": 2.8e-04,                 # 2.779e-04
}
ULP4 = 4 * 2.0 ** -24  # 4 ulp of 1.0 (2.4e-7)


def bar(name):
    return max(4.0 * FP32_DISTANCE[name], ULP4)


def test_every_case_has_its_measured_distance():
    assert set(FP32_DISTANCE) == set(R.CASES)
    for name in R.CASES:
        d = R.fp32_distance(name)
        print(f"{name}: fp32 restatement within {d:.3e} of fp64, constant {FP32_DISTANCE[name]:.1e}, bar {bar(name):.2e}")
        # the constant is the measurement rounded up, not a number with slack in it (a quarter either way: torch.mean's
        # summation order, which the contrast cases see, depends on the number of threads)
        assert d <= 1.25 * FP32_DISTANCE[name] and FP32_DISTANCE[name] <= 1.25 * d + 1e-8, (name, d)


# ---------------------------------------------------------------- the restatement itself
def _hue_test_image():
    g = torch.Generator().manual_seed(5)
    x = torch.rand((3, 12, 12), generator=g, dtype=torch.float64)
    x[:, 0] = x[0, 0]                      # gray pixels
    x[:, 1, :6] = 0.0                      # pure black
    x[:, 1, 6:] = 1.0                      # pure white
    x[1, 2] = x[0, 2]                      # r = g
    x[2, 3] = x[1, 3]                      # g = b
    x[2, 4] = x[0, 4]                      # r = b
    x[1, 5] = x[0, 5]; x[2, 5, :6] = 0.0; x[2, 5, 6:] = 1.0   # r = g above / below b
    return x


def test_hue_conversion_is_colorsys():
    x = _hue_test_image()
    hsv = R.rgb2hsv(x)
    back = R.hsv2rgb(hsv)
    for i in range(x.shape[1]):
        for j in range(x.shape[2]):
            r, g, b = (float(v) for v in x[:, i, j])
            want = colorsys.rgb_to_hsv(r, g, b)
            got = tuple(float(v) for v in hsv[:, i, j])
            assert abs((got[0] - want[0] + 0.5) % 1.0 - 0.5) < 1e-14 and abs(got[1] - want[1]) < 1e-14 and got[2] == want[2], (i, j)
            rgb = colorsys.hsv_to_rgb(*want)
            assert max(abs(float(back[c, i, j]) - rgb[c]) for c in range(3)) < 1e-14, (i, j)
    for f in (-0.5, -0.2, 0.0, 0.3, 0.5):  # the shift as adjust_hue does it
        out = R.adjust_hue(x, f)
        for i in range(x.shape[1]):
            for j in range(0, x.shape[2], 3):
                h, s, v = colorsys.rgb_to_hsv(*(float(c) for c in x[:, i, j]))
                rgb = colorsys.hsv_to_rgb((h + f) % 1.0, s, v)
                assert max(abs(float(out[c, i, j]) - rgb[c]) for c in range(3)) < 1e-14, (f, i, j)


def test_neutral_factors_are_the_identity_in_every_order():
    img = R.make_image(1, 37, 50, 31)
    base = img.permute(0, 3, 1, 2).double() / 255
    worst = 0.0
    for order in R.ORDERS:
        for out_size in (None, (16, 21)):
            _, plain = R.image_front(img, torch.float64, out_size=out_size)
            _, rgb = R.image_front(img, torch.float64, out_size=out_size, order=order, factors=(1.0, 1.0, 1.0, 0.0))
            worst = max(worst, float((rgb - plain).abs().max()))
    assert float((R.image_front(img, torch.float64)[1] - base).abs().max()) == 0.0
    print(f"neutral jitter: within {worst:.2e} of the unjittered image")
    assert worst <= 1e-14


def test_degenerate_factors():
    img = R.make_image(1, 20, 30, 32)
    for dtype in (torch.float32, torch.float64):
        _, sat0 = R.image_front(img, dtype, order=(2, -1, -1, -1), factors=(1.0, 1.0, 0.0, 0.0))
        assert torch.equal(sat0[:, 0], sat0[:, 1]) and torch.equal(sat0[:, 1], sat0[:, 2])
        gray, bright0 = R.image_front(img, dtype, order=(0, -1, -1, -1), factors=(0.0, 1.0, 1.0, 0.0))
        assert float(bright0.abs().max()) == 0.0 and float(gray.abs().max()) == 0.0
        plain_gray, _ = R.image_front(img, dtype)
        _, con0 = R.image_front(img, dtype, order=(1, -1, -1, -1), factors=(1.0, 0.0, 1.0, 0.0))
        assert float((con0 - plain_gray.mean()).abs().max()) <= (1e-6 if dtype == torch.float32 else 1e-15)
        assert float(con0.max() - con0.min()) == 0.0


def test_take_window_pads_and_crops():
    x = torch.arange(2 * 3 * 5 * 7, dtype=torch.float64).reshape(2, 3, 5, 7) + 1
    w = R.take_window(x, (-2, 0, 9, 7))
    assert tuple(w.shape) == (2, 3, 9, 7) and float(w[:, :, :2].abs().max()) == 0 and float(w[:, :, 7:].abs().max()) == 0
    assert torch.equal(w[:, :, 2:7], x)
    assert torch.equal(R.take_window(x, (1, 2, 3, 4)), x[:, :, 1:4, 2:6])
    w = R.take_window(x, (3, 5, 4, 4))
    assert torch.equal(w[:, :, :2, :2], x[:, :, 3:, 5:]) and float(w[:, :, 2:].abs().max()) == 0 and float(w[:, :, :, 2:].abs().max()) == 0


# ---------------------------------------------------------------- images.py on the host
def test_exported_and_bound(lib_built):
    import e2e_multi_view_matching_amd as E
    from e2e_multi_view_matching_amd import _lib, images
    for name in ("prepare_images", "color_jitter_params", "window_intrinsics"):
        assert getattr(E, name) is getattr(images, name) and name in E.__all__
    assert hasattr(ctypes.CDLL(lib_built), "e2emv_image_front")
    hdr = open(os.path.join(ROOT, "include", "e2emv.h")).read()
    decl = re.search(r"int e2emv_image_front\(([^;]*)\);", hdr).group(1)
    assert len(decl.split(",")) == len(_lib.SIGNATURES["e2emv_image_front"][1]) == 8
    body = re.search(r"typedef struct \{([^}]*)\} e2emv_image_front_desc;", hdr).group(1)
    fields = re.findall(r"\b([a-z_]+)\s*[,;]", re.sub(r"/\*.*?\*/", "", body))
    assert fields == [f[0] for f in _lib.ImageFrontDesc._fields_]
    assert "#define E2EMV_IMAGE_FRONT_TILE %d " % _lib.IMAGE_FRONT_TILE in hdr and "#define E2EMV_IMAGE_FRONT_STRIP %d " % _lib.IMAGE_FRONT_STRIP in hdr


def test_color_jitter_params():
    from e2e_multi_view_matching_amd import color_jitter_params
    j, n, t = 0.3, 200, 5
    order, factors = color_jitter_params(j, n, t, generator=torch.Generator().manual_seed(7))
    assert tuple(order.shape) == (n * t, 4) and order.dtype == torch.int32 and tuple(factors.shape) == (n * t, 4) and factors.dtype == torch.float32
    assert not order.is_cuda and not factors.is_cuda
    assert all(sorted(row) == [0, 1, 2, 3] for row in order.tolist())
    assert float(factors[:, :3].min()) >= 1 - j - 1e-7 and float(factors[:, :3].max()) <= 1 + j + 1e-7
    assert float(factors[:, 3].min()) >= -j - 1e-7 and float(factors[:, 3].max()) <= j
    o, f = order.reshape(n, t, 4), factors.reshape(n, t, 4)
    assert bool((o == o[:, :1]).all()) and bool((f == f[:, :1]).all())          # one draw per tuple
    assert len({tuple(r) for r in o[:, 0].tolist()}) == 24                        # every permutation turns up in 200 draws
    assert len(set(f[:, 0, 0].tolist())) == n                                     # and the tuples differ
    for k in range(3):  # the whole range is used
        assert float(f[:, 0, k].min()) < 1 - 0.9 * j and float(f[:, 0, k].max()) > 1 + 0.9 * j
    assert float(f[:, 0, 3].min()) < -0.9 * j and float(f[:, 0, 3].max()) > 0.9 * j
    again = color_jitter_params(j, n, t, generator=torch.Generator().manual_seed(7))
    assert torch.equal(again[0], order) and torch.equal(again[1], factors)
    other = color_jitter_params(j, n, t, generator=torch.Generator().manual_seed(8))
    assert not torch.equal(other[1], factors)
    o0, f0 = color_jitter_params(0.0, 2, 3)
    assert torch.equal(f0, torch.tensor([[1.0, 1.0, 1.0, 0.0]]).expand(6, 4))
    for bad in (-0.1, 0.6):
        with pytest.raises(ValueError):
            color_jitter_params(bad, 1, 1)
    with pytest.raises(ValueError):
        color_jitter_params(0.2, 0, 5)


def _crop_intrinsics(K, crop_x, crop_y):  # the reference's two functions, matching_dataset.py:14-24
    K[0, 2] -= crop_x
    K[1, 2] -= crop_y
    return K


def _resize_intrinsics(K, fact_x, fact_y):
    K[0, 0] *= fact_x
    K[1, 1] *= fact_y
    K[0, 2] *= fact_x
    K[1, 2] *= fact_y
    return K


def test_window_intrinsics():
    from e2e_multi_view_matching_amd import window_intrinsics
    K = np.array([[1165.7, 0.0, 649.1], [0.0, 1165.7, 484.8], [0.0, 0.0, 1.0]], dtype=np.float32)
    # the padded ScanNet frame: cy + 2, then the resize to the depth map
    want = K.copy()
    want[1, 2] = want[1, 2] + 2
    want = _resize_intrinsics(want, 640 / 1296, 480 / 972)
    got = window_intrinsics(K, (-2, 0, 972, 1296), (480, 640))
    assert isinstance(got, np.ndarray) and got.dtype == np.float32 and got is not K and K[1, 2] == np.float32(484.8)
    np.testing.assert_array_equal(got, want)
    # a MegaDepth crop at an offset, then a resize
    want = _resize_intrinsics(_crop_intrinsics(K.copy(), 131, 7), 480 / 600, 480 / 600)
    np.testing.assert_array_equal(window_intrinsics(K, (7, 131, 600, 600), (480, 480)), want)
    # neither
    np.testing.assert_array_equal(window_intrinsics(K, (0, 0, 968, 1296), (968, 1296)), K)
    # tensors, batched
    Kt = torch.from_numpy(K).double().expand(3, 3, 3)
    got = window_intrinsics(Kt, (7, 131, 600, 600), (480, 480))
    assert torch.is_tensor(got) and tuple(got.shape) == (3, 3, 3) and got.dtype == torch.float64
    want = _resize_intrinsics(_crop_intrinsics(K.astype(np.float64), 131, 7), 480 / 600, 480 / 600)
    np.testing.assert_allclose(got[1].numpy(), want, rtol=1e-15)
    with pytest.raises(ValueError):
        window_intrinsics(K, (0, 0, 0, 5), (4, 4))
    with pytest.raises(ValueError):
        window_intrinsics(K[:2], (0, 0, 5, 5), (4, 4))


def test_prepare_images_argument_errors():
    from e2e_multi_view_matching_amd import prepare_images
    img = R.make_image(2, 8, 9, 1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        prepare_images(img)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        prepare_images(img, out_size=(4, 5), order=(0, 1, 2, 3), factors=(1.0, 1.0, 1.0, 0.0))
    with pytest.raises(TypeError, match="uint8"):
        prepare_images(img.float())
    with pytest.raises(TypeError):
        prepare_images(img.numpy())
    for bad in (img[0], img[..., :2], img.permute(0, 3, 1, 2), img[:, :, :, :, None]):
        with pytest.raises(ValueError, match="B,Hin,Win,3"):
            prepare_images(bad)
    ok = (1.0, 1.0, 1.0, 0.0)
    for order in ((0, 1, 2, 4), (0, 1, 2, -2), (0, 1, 1, 3), (0, 1, 2), [(0, 1, 2, 3)] * 3, (0.0, 1.0, 2.0, 3.0)):
        with pytest.raises(ValueError):
            prepare_images(img, order=order, factors=ok)
    for factors in ((-0.1, 1, 1, 0), (1, -0.1, 1, 0), (1, 1, -0.1, 0), (1, 1, 1, 0.51), (1, 1, 1, -0.51), (float("nan"), 1, 1, 0),
                    (1, float("inf"), 1, 0), (1, 1, 1), [ok] * 3):
        with pytest.raises(ValueError):
            prepare_images(img, order=(0, 1, 2, 3), factors=factors)
    with pytest.raises(ValueError):
        prepare_images(img, order=(0, 1, 2, 3))  # order without factors
    with pytest.raises(ValueError):
        prepare_images(img, window=(0, 0, 0, 9))
    with pytest.raises(ValueError):
        prepare_images(img, window=(0, 0, 8))
    with pytest.raises(ValueError):
        prepare_images(img, out_size=(0, 9))
