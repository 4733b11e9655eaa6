"""The references of tests/test_gpu_superpoint_encoder.py and their premises, checked in the references alone (no gpu mark): a
case that misses what it is meant to show fails here instead of passing there vacuously.

  integer convolutions   operands of magnitude <= 8 and K <= 1152: every partial sum of |x||w| (+ |b|) stays below 2^24, so the fp32
                         result is exact whatever the order of summation and must EQUAL the integer convolution; in every pooled
                         case each of the four pixels of every 2x2 block is, in at least one channel, the block's only maximum (and
                         positive there, so that the ReLU leg shows it too) - a pixel that never wins has unobserved taps
  the size list          every residue 0..7 of H and of W modulo 8, always H != W
  the fp64 layer chain   `layer_ref` - one layer of upstream in fp64 on the VALID region of its input, zero padding around that
                         region, floor pooling - chained over the oracle's own activations reproduces OS.dense_maps on the unpadded
                         image: what the masking / cropping of the device path has to equal
"""
import functools

import pytest
import torch
import torch.nn.functional as F

from oracle import superpoint as OS

# ---- A: the convolution kernel alone, integer operands ------------------------------------------------------------------------------
PAIRS = ((64, 64), (64, 128), (128, 128), (128, 256), (32, 96))
GEOMS = ((1, 1, 1), (1, 1, 7), (1, 2, 2), (3, 6, 10), (5, 4, 6), (1, 18, 14), (2, 16, 24))
INT_MAX = 8


@functools.lru_cache(maxsize=None)
def int_case(cin, cout, n, H, W):
    """-> x [n,H,W,cin] NHWC, w [cout,cin,3,3] (upstream layout), b [cout]: fp32 tensors of integers in -8 .. 8"""
    g = torch.Generator().manual_seed(1000003 * cin + 10007 * cout + 101 * n + 11 * H + W)
    r = lambda *s: torch.randint(-INT_MAX, INT_MAX + 1, s, generator=g).float()  # noqa: E731
    return r(n, H, W, cin), r(cout, cin, 3, 3), r(cout)


def int_reference(x, w, b, relu, pool, dtype=torch.float64):
    """F.conv2d on the CPU in `dtype` -> NHWC fp32 (exact: every value is an integer below 2^24)"""
    y = F.conv2d(x.permute(0, 3, 1, 2).to(dtype), w.to(dtype), b.to(dtype) if b is not None else None, padding=1)
    if relu:
        y = F.relu(y)
    if pool:
        y = F.max_pool2d(y, 2, 2)
    return y.permute(0, 2, 3, 1).contiguous().float()


def int_magnitude(x, w, b):
    """the largest value any partial sum of one output can reach: sum |x||w| + |b|"""
    return float(F.conv2d(x.permute(0, 3, 1, 2).double().abs(), w.double().abs(), b.double().abs(), padding=1).max())


def walk_geometry(num_cus, narrow):
    """(n_img, H, W) of the tile-walking case: more row tiles than the persistent grid has workgroups (3 per CU of 128 rows, the
    narrow variant 2 per CU of 256 rows), by a tenth, so that workgroups walk on to a second tile"""
    rows = (2 * 256 if narrow else 3 * 128) * num_cus
    W = (rows * 11 // 10 + 2 * 192 - 1) // (2 * 192)
    W += W % 2
    return 2, 192, W


def walk_tiles(num_cus, narrow):
    n, H, W = walk_geometry(num_cus, narrow)
    return (n * H * W + (255 if narrow else 127)) // (256 if narrow else 128)


# ---- B: the stack, layer by layer -------------------------------------------------------------------------------------------------------
# (the last two complete the residues: without them no height is 5 and no width is 3 or 6 modulo 8)
SIZES = ((1, 16, 16), (3, 16, 24), (2, 17, 31), (1, 23, 18), (1, 26, 45), (2, 27, 21), (1, 30, 20), (1, 36, 41), (2, 71, 97), (1, 21, 19),
         (1, 29, 22))
GAIN_CASE = (1, 36, 41, 1.3)  # (B, H, W, gain of OS.seeded_state): the widest cell's logits span about 55, e^-55 is still a normal fp32
PARENT = (None, 0, 1, 2, 3, 4, 5, 6, 7, 8, 7, 10)  # the tap layer l reads (None: the image)
POOLED = (1, 3, 5)
NO_RELU = (9, 11)
U = 2.0 ** -24


def image(B, H, W):
    from test_gpu_superpoint import _image
    return _image(B, H, W, seed=H + W)


def valid_size(l, H, W):
    """valid (rows, columns) of tap l for H x W images: the floors of upstream's pools"""
    if l == 0:
        return H, W
    if l <= 2:
        return H // 2, W // 2
    if l <= 4:
        return H // 4, W // 4
    return H // 8, W // 8


def layer_ref(l, sd, x):
    """Layer l of upstream in fp64 on x [B,C,h,w] fp64 (the VALID region of what it reads): zero padding around x, ReLU (not behind
    the two 1x1 heads), floor pooling behind conv1b / conv2b / conv3b.  -> (y, bar) NCHW fp64: bar is the rigorous bound of an fp32
    evaluation in ANY order of summation, 1.01 (K + 2) 2^-24 (sum |a||w| + |b|) elementwise (ReLU and max are exact and do not
    widen it: behind a pool the largest of the four bars)."""
    name, cin, cout, k = OS.LAYERS[l]
    w, b = sd[name + ".weight"].double(), sd[name + ".bias"].double()
    y = F.conv2d(x, w, b, padding=k // 2)
    bar = 1.01 * (k * k * cin + 2) * U * F.conv2d(x.abs(), w.abs(), b.abs(), padding=k // 2)
    if l not in NO_RELU:
        y = F.relu(y)
    if l in POOLED:
        y, bar = F.max_pool2d(y, 2, 2), F.max_pool2d(bar, 2, 2)
    return y, bar


def score_ref(logits, B, Hc, Wc, dtype=torch.float64):
    """softmax over the 65 logits of a cell, dustbin dropped, 8x8 depth-to-space: logits [B*Hc*Wc,65] -> [B,8Hc,8Wc] in `dtype`"""
    s = F.softmax(logits.to(dtype), 1)[:, :64].reshape(B, Hc, Wc, 8, 8)
    return s.permute(0, 1, 3, 2, 4).reshape(B, Hc * 8, Wc * 8)


def chain_ref(sd, img):
    """the 12 layers chained in fp64 from the image -> list of the 12 outputs (NCHW fp64)"""
    out = []
    for l in range(12):
        out.append(layer_ref(l, sd, img.double() if PARENT[l] is None else out[PARENT[l]])[0])
    return out


# ---- the premises -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cin,cout", PAIRS)
def test_integer_cases_stay_exact_and_show_every_pixel(cin, cout):
    assert 9 * cin <= 1152 and INT_MAX * INT_MAX * 1152 + INT_MAX < 2 ** 24
    for n, H, W in GEOMS:
        x, w, b = int_case(cin, cout, n, H, W)
        assert float(x.abs().max()) <= INT_MAX and float(w.abs().max()) <= INT_MAX and float(b.abs().max()) <= INT_MAX
        assert torch.equal(x, x.round()) and torch.equal(w, w.round()) and torch.equal(b, b.round())
        assert int_magnitude(x, w, b) < 2 ** 24
        full = int_reference(x, w, b, False, False)
        assert torch.equal(full, int_reference(x, w, b, False, False, torch.float32))  # fp32 on the CPU is as exact as fp64
        assert float(full.abs().max()) > 0
        if H % 2 or W % 2:
            continue
        # [n,H/2,W/2,4,C]: the four pixels of every block; a pixel "shows" where it is the only maximum (and positive: the ReLU leg)
        q = full.reshape(n, H // 2, 2, W // 2, 2, cout).permute(0, 1, 3, 2, 4, 5).reshape(n, H // 2, W // 2, 4, cout)
        top = q.max(3, keepdim=True).values
        only = (q == top) & ((q == top).sum(3, keepdim=True) == 1)
        assert bool(only.any(-1).all()), (cin, cout, n, H, W)
        assert bool((only & (q > 0)).any(-1).all()), (cin, cout, n, H, W)


def test_integer_fp32_reference_is_exact_at_a_walking_shape():
    """the tile-walking cases take their reference from F.conv2d in fp32 (their fp64 form would cost seconds): the same there"""
    for cin, cout in ((64, 128), (64, 64)):
        x, w, b = int_case(cin, cout, 2, 24, 52)
        assert torch.equal(int_reference(x, w, b, False, False, torch.float32), int_reference(x, w, b, False, False))
    for cus in (64, 256, 304):
        assert walk_tiles(cus, False) > 3 * cus and walk_tiles(cus, True) > 2 * cus
        for narrow in (False, True):
            n, H, W = walk_geometry(cus, narrow)
            assert H % 2 == 0 and W % 2 == 0 and n * H * W < 2 ** 22  # (a CPU reference of a second or two)


def test_size_list_covers_every_residue():
    assert {H % 8 for _, H, _ in SIZES} == set(range(8)) and {W % 8 for _, _, W in SIZES} == set(range(8))
    # (16 x 16, the smallest legal image, is the one square; the cell grids of most sizes are not square either)
    assert all(H != W for _, H, W in SIZES if (H, W) != (16, 16)) and sum(H // 8 != W // 8 for _, H, W in SIZES) >= 6
    assert all(H >= 16 and W >= 16 for _, H, W in SIZES)
    # every level's mask is exercised in both directions: somewhere the valid size is odd at level 1 and at level 2 (the pool floors)
    assert any(H % 2 for _, H, _ in SIZES) and any(W % 2 for _, _, W in SIZES)
    assert any((H // 2) % 2 for _, H, _ in SIZES) and any((W // 2) % 2 for _, _, W in SIZES)
    assert any((H // 4) % 2 for _, H, _ in SIZES) and any((W // 4) % 2 for _, _, W in SIZES)


def test_gain_case_spreads_the_logits():
    """some cell's 65 logits span more than 30 (the softmax then covers 13 decades), none so much that e^-span leaves fp32's
    normal range - there the fp32 reference error, relative, would be 1 and the bar derived from it empty"""
    B, H, W, gain = GAIN_CASE
    lg = chain_ref({k: v.double() for k, v in OS.seeded_state(0, gain=gain).items()}, image(B, H, W))[9]
    span = float((lg.amax(1) - lg.amin(1)).max())
    assert 30 < span < 80, span


@pytest.mark.parametrize("B,H,W", [(2, 17, 31), (1, 23, 18), (1, 36, 41)])
def test_layer_chain_reproduces_the_oracle(B, H, W):
    sd = {k: v.double() for k, v in OS.seeded_state(0).items()}
    img = image(B, H, W).double()
    outs = chain_ref(sd, img)
    for l in range(12):
        assert tuple(outs[l].shape[2:]) == valid_size(l, H, W), l
    s, d = OS.dense_maps(sd, img)
    Hc, Wc = H // 8, W // 8
    mine = score_ref(outs[9].permute(0, 2, 3, 1).reshape(-1, 65), B, Hc, Wc)
    assert float((mine - s).abs().max()) < 1e-14
    assert float((outs[11] - d).abs().max()) < 1e-12
