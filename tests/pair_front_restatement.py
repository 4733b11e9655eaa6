"""Not a test: the image stage of the reference's pair loader (``PairMatchingDataset.__getitem__``, eval_pairs.py:89-106) restated in
numpy as one function taking a dtype: the quarter turns by their index formulas, the output size in the reference's own
expression, OpenCV's ``INTER_LINEAR`` resize of a float32 image written out (two taps per axis, half-pixel centres, the tap
position rounded ONCE to float32, the horizontal pass first) and ``/ 255.``.  The tap positions and weights are the float32
values in both dtypes; in float32 the rest is the reference's arithmetic, in float64 it is the yardstick the device call is
measured against.  ``cv2`` is not a dependency and was not available where this was written: byte parity of the float32 form
with a real OpenCV build is unmeasured (OpenCV's SIMD paths may fuse a product into a sum).

Also here, because the CPU test (which measures the bars) and the GPU test (which holds the device to them) share them: the test
images and the list of cases.  The kernel's tile is TILE_ROWS x TILE_COLS output pixels (include/e2emv.h).
"""
import numpy as np

TILE_ROWS, TILE_COLS = 32, 32


# ---------------------------------------------------------------- steps 2-6
def turn(img, rot):
    """np.rot90(img, k=rot) by its index formulas: out[i, j] of the turned image [h, w]."""
    H, W = img.shape
    if rot == 0:
        return img
    h, w = (W, H) if rot % 2 else (H, W)
    i, j = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    if rot == 1:
        return img[j, W - 1 - i]
    if rot == 2:
        return img[H - 1 - i, W - 1 - j]
    if rot == 3:
        return img[H - 1 - j, i]
    raise ValueError(rot)


def out_size(h, w, img_size):
    """eval_pairs.py:96-102 for a turned image h x w."""
    if img_size == max(w, h):
        return h, w
    if h >= w:
        ar = w / h
        return img_size, int(ar * img_size)
    ar = h / w
    return int(ar * img_size), img_size


def taps(n_in, n_out):
    """(s, s1, f) per output index of one axis: OpenCV's table for a float32 image; f is float32."""
    scale = 1.0 / (float(n_out) / float(n_in))
    d = np.arange(n_out, dtype=np.float64)
    f = ((d + 0.5) * scale - 0.5).astype(np.float32)  # the product and the difference in double, one rounding
    s = np.floor(f).astype(np.int64)
    f = (f - s.astype(np.float32)).astype(np.float32)
    low, high = s < 0, s >= n_in - 1
    s = np.where(low, 0, s)
    f = np.where(low, np.float32(0), f)
    s = np.where(high, n_in - 1, s)
    f = np.where(high, np.float32(0), f).astype(np.float32)
    return s, np.minimum(s + 1, n_in - 1), f


def double_taps(n_in, n_out):
    """aten's table for the same axis in fp64 (upsample_bilinear2d, align_corners=False): (s, s1, f) with f in double."""
    scale = float(n_in) / float(n_out)
    src = np.maximum(scale * (np.arange(n_out, dtype=np.float64) + 0.5) - 0.5, 0.0)
    s = np.minimum(src.astype(np.int64), n_in - 1)
    s1 = np.minimum(s + 1, n_in - 1)
    return s, s1, np.where(s < n_in - 1, src - s, 0.0)


def resize(x, h_out, w_out):
    """x [h, w] in float32 or float64 (values 0..255) -> [h_out, w_out] in the same dtype: horizontal taps, then vertical."""
    dt = x.dtype.type
    h, w = x.shape
    sx, sx1, fx = taps(w, w_out)
    sy, sy1, fy = taps(h, h_out)
    a0, a1 = (np.float32(1) - fx).astype(dt), fx.astype(dt)
    b0, b1 = (np.float32(1) - fy).astype(dt), fy.astype(dt)
    rows = x[:, sx] * a0[None, :] + x[:, sx1] * a1[None, :]
    return rows[sy] * b0[:, None] + rows[sy1] * b1[:, None]


def pair_front(img_u8, rot, img_size, dtype):
    """One frame: uint8 [H, W] -> `dtype` [h_out, w_out], steps 2-6 of the loader."""
    dt = np.dtype(dtype).type
    x = turn(np.asarray(img_u8), rot)
    h, w = x.shape
    h_out, w_out = out_size(h, w, img_size)
    x = x.astype(dt)
    if (h_out, w_out) != (h, w):
        x = resize(x, h_out, w_out)
    return x / dt(255)


# ---------------------------------------------------------------- test images and cases
def make_frame(H, W, seed):
    """Seeded uint8 [H, W]; every byte value is present when the frame has at least 256 pixels (the first 256 pixels of a
    seeded permutation of the positions hold 0..255), with a black and a white block at two edges."""
    g = np.random.default_rng(seed)
    x = g.integers(0, 256, size=(H, W), dtype=np.uint8)
    if H >= 8 and W >= 8:
        x[H // 3:H // 3 + max(H // 8, 2), :max(W // 6, 2)] = 0
        x[H // 2:H // 2 + max(H // 8, 2), W - max(W // 6, 2):] = 255
    if H * W >= 256:
        x.reshape(-1)[g.permutation(H * W)[:256]] = np.arange(256, dtype=np.uint8)
    return x


def all_values_frame(H, W, seed):
    x = make_frame(H, W, seed)
    assert len(set(x.reshape(-1).tolist())) == 256
    return x


TR, TC = TILE_ROWS, TILE_COLS

# name -> dict(frames=[(H, W, seed, rot), ...], img_size).  Output sizes in the comments are (rows, columns).
CASES = {}


def _case(name, frames, img_size):
    CASES[name] = dict(frames=frames, img_size=img_size)


for _rot in range(4):
    # inside one tile: 23 x 37 stored; the turned image's longer side becomes 29 (rows 18 or columns 18)
    _case(f"inside_rot{_rot}", [(23, 37, 10 + _rot, _rot)], TC - 3)
    # exactly on tile edges: 96 x 48 stored -> longer side 2 * 32, the shorter one 32
    _case(f"edges_rot{_rot}", [(96, 48, 20 + _rot, _rot)], 2 * TR)
    # 211 x 187 stored -> 3 * 32 + 9 = 105 on the longer side (four tiles, the last one ragged) and 93 = 2 * 32 + 29 on the
    # shorter (three, the last one ragged); a reduction by 2.01, where some tiles stage the covered lines and some the tapped ones
    _case(f"tiles_rot{_rot}", [(211, 187, 30 + _rot, _rot)], 3 * TR + 9)
_case("enlarge", [(37, 50, 40, 0)], 64)            # 37 x 50 -> 47 x 64
_case("enlarge_turned", [(37, 50, 41, 3)], 64)     # 50 x 37 -> 64 x 47
_case("reduce_5", [(330, 170, 42, 0)], 61)         # by 5.41: only the tapped lines are staged
_case("reduce_5_turned", [(330, 170, 43, 1)], 61)
_case("reduce_8", [(520, 264, 44, 2)], 65)         # by 8
_case("reduce_8_turned", [(264, 520, 45, 3)], 65)
_case("factor_2_down", [(128, 66, 46, 0)], 64)     # tap positions exact in float32
_case("factor_2_up", [(32, 16, 47, 1)], 64)        # turned 16 x 32 -> 32 x 64
_case("one_wide", [(57, 1, 48, 0)], 171)           # 57 x 1 -> 171 x 2 or 3: every tap of the x axis clamps (s = 0 = n_in - 1)
_case("one_high", [(1, 57, 49, 0)], 171)           # 1 x 57 -> 2 or 3 x 171
_case("one_wide_turned", [(57, 1, 60, 1)], 171)    # turned: 1 x 57
_case("one_wide_as_it_is", [(57, 1, 64, 2)], 57)   # not resized
_case("two_wide_to_one", [(100, 2, 61, 0)], 50)    # 100 x 2 -> 50 x 1: the x axis has one output, both its taps are read
_case("two_high_to_one", [(2, 100, 62, 3)], 50)    # turned: 100 x 2 -> 50 x 1
_case("ragged_five", [(23, 37, 50, 0), (211, 187, 51, 1), (96, 60, 52, 2), (64, 40, 53, 3), (330, 170, 54, 0)], 64)
_case("list_of_one", [(45, 64, 55, 2)], 64)        # not resized
_case("merged_pair", [(97, 130, 56, 0), (97, 130, 57, 0)], 72)
_case("merged_turned", [(97, 130, 58, 1), (130, 97, 59, 0)], 72)  # a turned frame and an upright one of the same output


def case_inputs(name):
    """[(frame uint8 [H, W], rot), ...], img_size."""
    c = CASES[name]
    return [(make_frame(H, W, seed), rot) for H, W, seed, rot in c["frames"]], c["img_size"]


def case_outputs(name, dtype):
    frames, img_size = case_inputs(name)
    return [pair_front(f, rot, img_size, dtype) for f, rot in frames]


def fp32_distance(name):
    """The largest distance of the float32 restatement from the float64 one over the images of the case."""
    a, b = case_outputs(name, np.float32), case_outputs(name, np.float64)
    return max(float(np.abs(x.astype(np.float64) - y).max()) for x, y in zip(a, b))
