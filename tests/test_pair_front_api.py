"""CPU: the restatement of the pair loader's image stage (tests/pair_front_restatement.py) against np.rot90 and aten's bilinear
resize, the host side of e2e_multi_view_matching_amd.images for pair evaluation (output sizes, intrinsics, argument errors) and
THE BARS of tests/test_gpu_pair_front.py: per GPU case 4 x the largest distance of the float32 restatement (the reference's
arithmetic) from the float64 one, not below 4 ulp of 1.0 - measured here, by `bar`, every time."""
import ctypes
import functools
import os
import re
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pair_front_restatement as R  # noqa: E402
from e2e_multi_view_matching_amd import pair_intrinsics, pair_out_size, prepare_pair_images  # noqa: E402  (every test of this file and of
# tests/test_gpu_pair_front.py, which imports the bars from here, needs the feature: without it the file does not import)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ULP4 = 4 * 2.0 ** -24  # 4 ulp of 1.0 (2.4e-7)


@functools.lru_cache(maxsize=None)
def bar(name):
    """The device's bar for a case: 4 x the measured distance of the float32 restatement from the float64 one - for the
    device's contraction of a product into a sum - and not below 4 ulp of 1.0."""
    return max(4.0 * R.fp32_distance(name), ULP4)


def test_every_case_has_its_measured_bar():
    """The float32 form rounds the two weights 1 - f, three times in each of the two tap passes (at the scale of 255: half an ulp
    there is 3e-8 of the result) and once in the division: its distance from float64 stays below 2.5 ulp of 1.0 (3e-7) and the
    bars about 5e-7, whatever the case."""
    for name in R.CASES:
        d = R.fp32_distance(name)
        print(f"{name}: float32 restatement within {d:.3e} of float64, bar {bar(name):.3e}")
        assert d <= 2.5 * 2.0 ** -23, (name, d)
        assert ULP4 <= bar(name) <= 1.2e-6, (name, bar(name))


# ---------------------------------------------------------------- sizes
def _reference_size(h, w, img_size):  # eval_pairs.py:96-102 on the turned image, as written there
    if img_size != max(w, h):
        if h >= w:
            ar = w / h
            return (img_size, int(ar * img_size))
        ar = h / w
        return (int(ar * img_size), img_size)
    return (h, w)


def test_out_size_is_the_references_expression(lib_built):
    from e2e_multi_view_matching_amd import _lib
    lib = _lib.load_library()
    assert pair_out_size((10, 7), 0, 720) == (720, 503)          # 0.7 * 720 = 503.99..., not 504
    assert pair_out_size((7, 10), 0, 720) == (503, 720)
    assert pair_out_size((7, 10), 1, 720) == (720, 503)          # turned: 10 x 7
    assert pair_out_size((968, 1296), 0, 720) == (537, 720)
    assert pair_out_size((1296, 968), 0, 720) == (720, 537)
    assert pair_out_size((968, 1296), 3, 720) == (720, 537)
    assert pair_out_size((480, 640), 0, 1600) == (1200, 1600)    # enlarged
    assert pair_out_size((480, 640), 0, 640) == (480, 640) and pair_out_size((480, 640), 1, 640) == (640, 480)  # unchanged
    g = np.random.default_rng(0)
    sweep = [(10, 7, 720), (7, 10, 720), (968, 1296, 720), (480, 640, 1600), (480, 640, 640), (1, 1, 1), (16384, 16384, 16384), (16384, 2048, 2048)]
    sweep += [(int(h), int(w), int(s)) for h, w, s in zip(g.integers(1, 2000, 400), g.integers(1, 2000, 400), g.integers(1, 2000, 400))]
    sweep += [(h, w, s) for h in range(1, 30) for w in range(1, 30) for s in (1, 7, 29, 30, 720)]
    n_truncated = 0
    for H, W, s in sweep:
        for rot in range(4):
            h, w = (W, H) if rot % 2 else (H, W)
            want = _reference_size(h, w, s)
            assert pair_out_size((H, W), rot, s) == want, (H, W, rot, s)
            assert R.out_size(h, w, s) == want
            ho, wo = ctypes.c_int(-1), ctypes.c_int(-1)
            rc = lib.e2emv_image_front_gray_size(H, W, rot, s, ctypes.byref(ho), ctypes.byref(wo))
            assert (ho.value, wo.value) == want, (H, W, rot, s)
            assert rc == (_lib.OK if min(want) > 0 else _lib.EINVAL)
            by_integers = (s, s * w // h) if h >= w else (s * h // w, s)
            n_truncated += s != max(h, w) and want != by_integers
    assert n_truncated > 0  # the sweep holds sizes where the integer division gives another number
    for bad in ((0, 5, 0, 7), (5, -1, 0, 7), (5, 5, 4, 7), (5, 5, -1, 7), (5, 5, 0, 0)):
        ho, wo = ctypes.c_int(), ctypes.c_int()
        assert lib.e2emv_image_front_gray_size(*bad, ctypes.byref(ho), ctypes.byref(wo)) == _lib.EINVAL, bad
    assert lib.e2emv_image_front_gray_size(5, 5, 0, 7, None, None) == _lib.EINVAL
    for bad in (((0, 5), 0, 7), ((5, 5), 4, 7), ((5, 5), -1, 7), ((5, 5), 1.0, 7), ((5, 5), 0, 0)):
        with pytest.raises(ValueError):
            pair_out_size(*bad)


# ---------------------------------------------------------------- intrinsics
def _resize_intrinsics(K, fact_x, fact_y):  # the reference's, datasets/matching_dataset.py:19-24
    K[0, 0] *= fact_x
    K[1, 1] *= fact_y
    K[0, 2] *= fact_x
    K[1, 2] *= fact_y
    return K


def test_pair_intrinsics():
    from e2e_multi_view_matching_amd.metrics import rotate_intrinsics
    K = np.array([[1165.7, 0.0, 649.1], [0.0, 1170.2, 484.8], [0.0, 0.0, 1.0]])
    for dtype in (np.float64, np.float32):
        K0 = K.astype(dtype)
        for shape, img_size in (((968, 1296), 720), ((480, 640), 1600), ((480, 640), 640), ((1296, 968), 720)):
            for rot in range(4):
                img_shape = (shape[1], shape[0]) if rot % 2 else shape  # eval_pairs.py:91-104 on the turned image
                intr = K0.copy()
                if rot != 0:
                    intr = rotate_intrinsics(intr, img_shape, rot)
                if img_size != max(img_shape):
                    rs = pair_out_size(shape, rot, img_size)
                    intr = _resize_intrinsics(intr, rs[1] / img_shape[1], rs[0] / img_shape[0])
                keep = K0.copy()
                got = pair_intrinsics(K0, shape, rot, img_size)
                assert isinstance(got, np.ndarray) and got.dtype == dtype and got is not K0
                np.testing.assert_array_equal(K0, keep)  # the input is left as it is
                np.testing.assert_array_equal(got, intr)
    Kt = torch.from_numpy(K)
    got = pair_intrinsics(Kt, (968, 1296), 1, 720)
    assert torch.is_tensor(got) and got.dtype == torch.float64 and got.data_ptr() != Kt.data_ptr()
    np.testing.assert_array_equal(Kt.numpy(), K)
    np.testing.assert_array_equal(got.numpy(), pair_intrinsics(K, (968, 1296), 1, 720))
    with pytest.raises(ValueError):
        pair_intrinsics(K[:2], (968, 1296), 0, 720)
    with pytest.raises(ValueError):
        pair_intrinsics(K, (968, 1296), 5, 720)


# ---------------------------------------------------------------- argument errors: all of them before any device call
def test_prepare_pair_images_argument_errors():
    a = torch.from_numpy(R.make_frame(8, 9, 1))
    b = torch.from_numpy(R.make_frame(12, 9, 2))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        prepare_pair_images([a, b], 16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        prepare_pair_images([a, a], 16, rots=[0, 2], merge=True)
    with pytest.raises(TypeError, match="uint8"):
        prepare_pair_images([a, b.float()], 16)
    with pytest.raises(TypeError):
        prepare_pair_images([a.numpy()], 16)
    with pytest.raises(TypeError):
        prepare_pair_images(a, 16)
    for bad in (a[0], a[None], a[None, None]):
        with pytest.raises(ValueError, match="H,W"):
            prepare_pair_images([a, bad], 16)
    with pytest.raises(ValueError, match="empty"):
        prepare_pair_images([], 16)
    for rots in ([0, 4], [-1, 0], [0, 1.0], [0, None]):
        with pytest.raises(ValueError, match="turn"):
            prepare_pair_images([a, b], 16, rots=rots)
    for rots in ([0], [0, 1, 2]):
        with pytest.raises(ValueError, match="turns"):
            prepare_pair_images([a, b], 16, rots=rots)
    with pytest.raises(ValueError, match="merge"):
        prepare_pair_images([a, b], 16, merge=True)       # 14 x 16 and 16 x 12
    with pytest.raises(ValueError, match="merge"):
        prepare_pair_images([a, a], 16, rots=[0, 1], merge=True)
    with pytest.raises(ValueError):
        prepare_pair_images([a], 0)
    with pytest.raises(ValueError, match="side of 0"):
        prepare_pair_images([torch.zeros((57, 1), dtype=torch.uint8)], 40)  # int((1 / 57) * 40) = 0
    with pytest.raises(ValueError):
        prepare_pair_images([a] * 257, 16)


def test_exported_and_bound(lib_built):
    import e2e_multi_view_matching_amd as E
    from e2e_multi_view_matching_amd import _lib, images
    for name in ("prepare_pair_images", "pair_out_size", "pair_intrinsics"):
        assert getattr(E, name) is getattr(images, name) and name in E.__all__
    lib = ctypes.CDLL(lib_built)
    hdr = open(os.path.join(ROOT, "include", "e2emv.h")).read()
    for name, n_args in (("e2emv_image_front_gray", 6), ("e2emv_image_front_gray_size", 6)):
        assert hasattr(lib, name)
        decl = re.search(r"int %s\(([^;]*)\);" % name, hdr).group(1)
        assert len(decl.split(",")) == len(_lib.SIGNATURES[name][1]) == n_args
    body = re.search(r"typedef struct \{([^}]*)\} e2emv_gray_image;", hdr).group(1)
    fields = re.findall(r"\b([a-z_]+)\s*[,;]", re.sub(r"/\*.*?\*/", "", body))
    assert fields == [f[0] for f in _lib.GrayImage._fields_]
    for name, v in (("TILE_ROWS", _lib.IMAGE_FRONT_GRAY_TILE_ROWS), ("TILE_COLS", _lib.IMAGE_FRONT_GRAY_TILE_COLS),
                    ("MAX_IMAGES", _lib.IMAGE_FRONT_GRAY_MAX_IMAGES)):
        assert "#define E2EMV_IMAGE_FRONT_GRAY_%s %d " % (name, v) in hdr
    assert (R.TILE_ROWS, R.TILE_COLS) == (_lib.IMAGE_FRONT_GRAY_TILE_ROWS, _lib.IMAGE_FRONT_GRAY_TILE_COLS)
    assert _lib.IMAGE_FRONT_GRAY_MAX_IMAGES >= 64


# ---------------------------------------------------------------- the restatement itself
def test_turn_is_rot90():
    for H, W in ((5, 8), (8, 5), (1, 7), (7, 1), (6, 6)):
        img = R.make_frame(H, W, 3)
        for rot in range(4):
            got = R.turn(img, rot)
            assert got.dtype == np.uint8 and np.array_equal(got, np.rot90(img, k=rot)), (H, W, rot)


def test_unresized_is_the_division():
    img = R.all_values_frame(20, 16, 4)
    for rot in range(4):
        got = R.pair_front(img, rot, 20, np.float32)
        assert got.dtype == np.float32 and np.array_equal(got, np.rot90(img, k=rot).astype(np.float32) / np.float32(255))
        assert np.array_equal(got, (torch.from_numpy(np.rot90(img, k=rot).copy()).float() / 255).numpy())


def _dense(n_in, s, s1, w0, w1):
    M = np.zeros((len(s), n_in))
    np.add.at(M, (np.arange(len(s)), s), w0)
    np.add.at(M, (np.arange(len(s)), s1), w1)
    return M


def _axis_bound(n_in, n_out):
    """The most one axis can move an output whose inputs lie in [0, 1]: over the output indices, the larger of the summed
    positive and the summed negative weight differences between the float32 tap table and aten's double one."""
    s, s1, f = R.taps(n_in, n_out)
    t, t1, fd = R.double_taps(n_in, n_out)
    D = _dense(n_in, s, s1, (np.float32(1) - f).astype(np.float64), f.astype(np.float64)) - _dense(n_in, t, t1, 1.0 - fd, fd)
    return max(float(np.clip(D, 0, None).sum(axis=1).max()), float(np.clip(-D, 0, None).sum(axis=1).max()))


def _aten(x, h_out, w_out):
    t = torch.from_numpy(x)[None, None]
    return F.interpolate(t, size=(h_out, w_out), mode="bilinear", align_corners=False)[0, 0].numpy()


@pytest.mark.parametrize("shape, out", [((968, 1296), (537, 720)), ((37, 50), (47, 64)), ((211, 187), (105, 93)), ((330, 170), (61, 31)),
                                        ((520, 264), (65, 33)), ((480, 640), (1200, 1600)), ((57, 1), (171, 3)), ((2, 100), (1, 50))])
def test_resize_against_aten_within_the_tap_rounding(shape, out):
    """OpenCV rounds the tap position to float32, aten (in fp64) does not: the float64 restatement lies within the derived
    bound of aten's bilinear - the sum over the two axes of the largest weight difference of the two tables (values in [0, 1])."""
    x = R.make_frame(shape[0], shape[1], 70).astype(np.float64)
    got = R.resize(x, *out) / 255.0
    want = _aten(x, *out) / 255.0
    bound = _axis_bound(shape[0], out[0]) + _axis_bound(shape[1], out[1])
    d = float(np.abs(got - want).max())
    print(f"{shape} -> {out}: float64 restatement within {d:.3e} of aten's fp64 bilinear; bound from the tap tables {bound:.3e}")
    assert d <= bound + 1e-13  # (the fp64 evaluation of either side: a few 1e-16)
    assert bound < 2e-4        # float32 at positions up to 16384: the tables differ, but by a rounding of the position


@pytest.mark.parametrize("shape, out", [((33, 20), (66, 40)), ((128, 66), (64, 33)), ((16, 32), (32, 64)), ((64, 64), (16, 16))])
def test_resize_is_aten_where_the_taps_are_exact(shape, out):
    x = R.make_frame(shape[0], shape[1], 71).astype(np.float64)
    assert _axis_bound(shape[0], out[0]) == 0.0 and _axis_bound(shape[1], out[1]) == 0.0
    assert np.array_equal(R.resize(x, *out), _aten(x, *out))  # (dyadic weights on integers: nothing rounds on either side)


def test_cases_cover_what_they_claim():
    TR, TC = R.TILE_ROWS, R.TILE_COLS
    sizes = {name: [R.out_size(*((W, H) if rot % 2 else (H, W)), c["img_size"]) for H, W, _, rot in c["frames"]] for name, c in R.CASES.items()}
    for rot in range(4):
        (h, w), = sizes[f"inside_rot{rot}"]
        assert h < TR and w < TC and h != w
        (h, w), = sizes[f"edges_rot{rot}"]
        assert h % TR == 0 and w % TC == 0 and h != w
        (h, w), = sizes[f"tiles_rot{rot}"]
        assert h > 2 * TR and h % TR and w > 2 * TC and w % TC and h != w
    assert sizes["enlarge"] == [(47, 64)] and sizes["reduce_5"] == [(61, 31)] and sizes["reduce_8"] == [(65, 33)]
    assert sizes["factor_2_down"] == [(64, 33)] and sizes["factor_2_up"] == [(32, 64)]
    assert sizes["one_wide"][0][1] in (2, 3) and sizes["one_high"][0][0] in (2, 3) and sizes["two_wide_to_one"] == [(50, 1)]
    assert len(set(sizes["ragged_five"])) == 5 and len(sizes["list_of_one"]) == 1
    assert len(set(sizes["merged_pair"])) == 1 and len(set(sizes["merged_turned"])) == 1
    assert len(set(R.all_values_frame(45, 64, 55).reshape(-1).tolist())) == 256
