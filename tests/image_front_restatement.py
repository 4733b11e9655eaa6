"""Not a test: the image stage of the reference's data loader (``MatchingDataset.__getitem__``, datasets/matching_dataset.py:182-211)
restated in torch ops, one function taking a dtype.  In float32 it is the reference's arithmetic (torchvision's tensor forms of
ToTensor, resize, ColorJitter's four ops and rgb_to_grayscale, written out: torchvision is not a dependency); in float64 it is the
yardstick the device call is measured against.  The resize is ``torch.nn.functional.interpolate`` itself.

Also here, because the CPU test (which measures the bars) and the GPU test (which holds the device to them) share them: the test
images and the list of cases.
"""
import itertools

import torch
import torch.nn.functional as F

ORDERS = list(itertools.permutations(range(4)))  # the 24 orders of (brightness, contrast, saturation, hue)


# ---------------------------------------------------------------- torchvision's tensor ops, written out
def gray_of(img):
    r, g, b = img.unbind(dim=-3)
    return (0.2989 * r + 0.587 * g + 0.114 * b).unsqueeze(dim=-3)


def blend(img1, img2, ratio):
    return (ratio * img1 + (1.0 - ratio) * img2).clamp(0, 1.0)


def adjust_brightness(img, f):
    return blend(img, torch.zeros_like(img), f)


def adjust_contrast(img, f):
    mean = torch.mean(gray_of(img), dim=(-3, -2, -1), keepdim=True)
    return blend(img, mean, f)


def adjust_saturation(img, f):
    return blend(img, gray_of(img), f)


def rgb2hsv(img):
    r, g, b = img.unbind(dim=-3)
    maxc = torch.max(img, dim=-3).values
    minc = torch.min(img, dim=-3).values
    eqc = maxc == minc
    cr = maxc - minc
    ones = torch.ones_like(maxc)
    s = cr / torch.where(eqc, ones, maxc)
    cr_divisor = torch.where(eqc, ones, cr)
    rc = (maxc - r) / cr_divisor
    gc = (maxc - g) / cr_divisor
    bc = (maxc - b) / cr_divisor
    hr = (maxc == r) * (bc - gc)
    hg = ((maxc == g) & (maxc != r)) * (2.0 + rc - bc)
    hb = ((maxc != g) & (maxc != r)) * (4.0 + gc - rc)
    h = hr + hg + hb
    h = torch.fmod((h / 6.0 + 1.0), 1.0)
    return torch.stack((h, s, maxc), dim=-3)


def hsv2rgb(img):
    h, s, v = img.unbind(dim=-3)
    i = torch.floor(h * 6.0)
    f = (h * 6.0) - i
    i = i.to(dtype=torch.int32)
    p = torch.clamp((v * (1.0 - s)), 0.0, 1.0)
    q = torch.clamp((v * (1.0 - s * f)), 0.0, 1.0)
    t = torch.clamp((v * (1.0 - (s * (1.0 - f)))), 0.0, 1.0)
    i = i % 6
    mask = i.unsqueeze(dim=-3) == torch.arange(6, device=i.device).view(-1, 1, 1)
    a1 = torch.stack((v, q, p, p, t, v), dim=-3)
    a2 = torch.stack((t, v, v, q, p, p), dim=-3)
    a3 = torch.stack((p, p, t, v, v, q), dim=-3)
    a4 = torch.stack((a1, a2, a3), dim=-4)
    return torch.einsum("...ijk, ...xijk -> ...xjk", mask.to(dtype=img.dtype), a4)


def adjust_hue(img, f):
    hsv = rgb2hsv(img)
    h, s, v = hsv.unbind(dim=-3)
    h = (h + f) % 1.0
    return hsv2rgb(torch.stack((h, s, v), dim=-3))


OPS = (adjust_brightness, adjust_contrast, adjust_saturation, adjust_hue)


def jitter(img, order, factors):
    """One image [3,H,W]; order: four ints (-1 skips the slot), factors: four Python floats."""
    for op in order:
        if op >= 0:
            img = OPS[op](img, factors[op])
    return img


# ---------------------------------------------------------------- the pipeline
def take_window(x, window):
    """x [B,3,H,W]; window (top, left, height, width) in source coordinates, zeros outside the image."""
    if window is None:
        return x
    top, left, height, width = window
    H, W = x.shape[-2:]
    x = F.pad(x, (max(-left, 0), max(left + width - W, 0), max(-top, 0), max(top + height - H, 0)))
    t, l = max(top, 0), max(left, 0)
    return x[..., t:t + height, l:l + width]


def image_front(rgb_u8, dtype, out_size=None, window=None, antialias=False, order=None, factors=None):
    """rgb_u8 [B,Hin,Win,3] uint8 (CPU) -> (gray [B,1,Hout,Wout], rgb [B,3,Hout,Wout]) in `dtype`.  order / factors: None, or a
    row of four / B rows of four (ints, numbers)."""
    B = rgb_u8.shape[0]
    x = rgb_u8.permute(0, 3, 1, 2).to(dtype).div(255)  # ToTensor
    x = take_window(x, window)
    if out_size is not None and tuple(out_size) != tuple(x.shape[-2:]):
        x = F.interpolate(x, size=tuple(out_size), mode="bilinear", align_corners=False, antialias=bool(antialias))
    if order is not None:
        order = torch.as_tensor(order).reshape(-1, 4).expand(B, 4).tolist()
        factors = torch.as_tensor(factors, dtype=torch.float32).reshape(-1, 4).expand(B, 4).tolist()  # (fp32 values, as the library takes them)
        x = torch.stack([jitter(x[b], order[b], factors[b]) for b in range(B)])
    return gray_of(x), x


# ---------------------------------------------------------------- test images and cases
def make_image(B, H, W, seed):
    """Random uint8 RGB [B,H,W,3] with planted gray rows, an all-0 and an all-255 block and two-channel ties."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(0, 256, (B, H, W, 3), generator=g, dtype=torch.uint8)
    x[:, H // 5] = x[:, H // 5, :, :1].clone()                        # a gray row (r = g = b)
    x[:, H - 1] = x[:, H - 1, :, 2:].clone()                          # the last row too
    x[:, H // 3:H // 3 + max(H // 8, 2), :max(W // 6, 2)] = 0          # a black block at the left edge
    x[:, H // 2:H // 2 + max(H // 8, 2), W - max(W // 6, 2):] = 255    # a white block at the right edge
    x[:, 2 * H // 3, :, 1] = x[:, 2 * H // 3, :, 0].clone()           # r = g
    x[:, 2 * H // 3 + 1, :, 2] = x[:, 2 * H // 3 + 1, :, 1].clone()   # g = b
    x[:, :, W // 2, 2] = x[:, :, W // 2, 0].clone()                   # r = b down a column
    return x


def all_values_image():
    """[1,16,48,3]: every uint8 value in every channel, rows of 144 bytes and a few repeats."""
    v = torch.arange(768, dtype=torch.int64)
    return torch.stack(((v * 1) % 256, (v * 3 + 85) % 256, (v * 5 + 170) % 256), dim=-1).to(torch.uint8).reshape(1, 16, 48, 3)


def _rand_factors(n, seed):
    g = torch.Generator().manual_seed(seed)
    u = torch.rand((n, 4), generator=g)
    return torch.stack((0.6 + 0.8 * u[:, 0], 0.6 + 0.8 * u[:, 1], 0.6 + 0.8 * u[:, 2], -0.3 + 0.6 * u[:, 3]), dim=1).to(torch.float32)


FULL = (0.8, 1.3, 1.25, 0.1)

# name -> dict(image=(B, H, W, seed), out_size, window, antialias, order, factors).  The kernel's tile is 16 rows x 64 columns.
CASES = {}


def _case(name, image, out_size=None, window=None, antialias=False, order=None, factors=None):
    CASES[name] = dict(image=image, out_size=out_size, window=window, antialias=antialias, order=order, factors=factors)


for aa in (0, 1):
    _case(f"down_aa{aa}", (1, 37, 50, 1), (16, 21), antialias=aa)   # taps run off both edges; rows of 150 bytes
    _case(f"up_aa{aa}", (1, 37, 50, 2), (48, 64), antialias=aa)
    # 131 x 203 = 8 tiles of 16 rows + 3 rows, 3 tiles of 64 columns + 11 columns
    _case(f"tiles_aa{aa}", (1, 263, 410, 3), (131, 203), antialias=aa, order=(0, 2, 1, 3), factors=FULL)
_case("noresize", (2, 37, 50, 4), (37, 50))
_case("noresize_tiles", (1, 35, 131, 5), None, order=(3, 1, 0, 2), factors=FULL)  # 3 x 3 tiles, the last ones ragged
_case("window_pad", (1, 37, 50, 6), (20, 25), window=(-2, 0, 41, 50))
_case("window_pad_noresize", (1, 37, 50, 6), None, window=(-2, 0, 41, 50))
_case("window_crop", (1, 37, 50, 7), (24, 24), window=(3, 9, 30, 30))
_case("window_crop_noresize", (1, 37, 50, 7), None, window=(3, 9, 30, 30))
_case("window_over", (1, 37, 50, 8), (15, 20), window=(-3, -4, 30, 40), antialias=1)
_case("window_over_noresize", (2, 37, 50, 8), None, window=(20, 30, 30, 40))
_case("orders24", (24, 37, 50, 9), (16, 21), order=ORDERS, factors=_rand_factors(24, 10).tolist())
_case("orders24_noresize", (24, 19, 23, 11), None, order=ORDERS, factors=_rand_factors(24, 12).tolist())
_case("skipped", (3, 37, 50, 13), (16, 21), antialias=1, order=[(0, -1, 3, -1), (-1, -1, -1, -1), (2, -1, -1, 1)],
      factors=_rand_factors(3, 14).tolist())
_case("contrast_first_last", (2, 37, 50, 15), (16, 21), order=[(1, 0, 2, 3), (0, 2, 3, 1)], factors=_rand_factors(2, 16).tolist())
_case("contrast_absent", (2, 37, 50, 17), (16, 21), order=[(0, 2, 3, -1), (3, -1, 2, 0)], factors=_rand_factors(2, 18).tolist())
_case("three_rows", (3, 37, 50, 19), (48, 64), order=[(3, 2, 1, 0), (1, 3, 0, 2), (2, 0, 3, 1)], factors=_rand_factors(3, 20).tolist())
_case("broadcast_row", (2, 37, 50, 21), (16, 21), order=(2, 1, 3, 0), factors=FULL)
_case("extremes", (3, 37, 50, 22), (16, 21), order=[(0, 1, 2, 3), (3, 2, 1, 0), (1, 0, 3, 2)],
      factors=[(1.2, 0.7, 1.4, 0.5), (0.9, 1.5, 0.0, -0.5), (0.0, 1.3, 0.8, 0.25)])
_case("frame", (2, 968, 1296, 23), (480, 640), window=(-2, 0, 972, 1296), order=[(0, 1, 2, 3), (2, 1, 3, 0)],
      factors=[FULL, (1.3, 0.75, 0.7, -0.2)])


def case_inputs(name):
    c = CASES[name]
    kw = {k: c[k] for k in ("out_size", "window", "antialias", "order", "factors")}
    return make_image(*c["image"]), kw


def fp32_distance(name):
    """The largest distance of the fp32 restatement from the fp64 one over both outputs of the case."""
    img, kw = case_inputs(name)
    g32, c32 = image_front(img, torch.float32, **kw)
    g64, c64 = image_front(img, torch.float64, **kw)
    return max(float((g32.double() - g64).abs().max()), float((c32.double() - c64).abs().max()))
