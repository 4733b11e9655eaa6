"""The image stage of the reference's data loader (``MatchingDataset.__getitem__``, ``datasets/matching_dataset.py:182-211``) as one
library call on the device: ``ToTensor``, the 2-row zero padding of the large ScanNet frames / the square crop of MegaDepth (one
source window), ``resize`` to the depth map's size, ``ColorJitter`` with one parameter set per tuple and ``rgb_to_grayscale``.

* ``prepare_images``      - uint8 RGB ``[B,Hin,Win,3]`` on the device -> float32 gray ``[B,1,Hout,Wout]``, what ``SuperPoint`` takes
  (``e2emv_image_front``, csrc/image_front.hip).
* ``color_jitter_params`` - the draw of ``get_color_jitter_params`` (``matching_dataset.py:125-130``, ``167-169``): one per tuple.
* ``window_intrinsics``   - the change of the intrinsics that goes with a window and an output size.

And the image stage of its pair loader (``PairMatchingDataset.__getitem__``, ``eval_pairs.py:85-108``): ``np.rot90``, ``cv2.resize``
to ``img_size``, ``/ 255.`` for a list of decoded gray frames of any sizes, one launch.

* ``prepare_pair_images`` - list of uint8 gray ``[H,W]`` on the device, one turn each -> float32 ``[1,1,h_out,w_out]`` each
  (``e2emv_image_front_gray``, csrc/image_front_pairs.hip).
* ``pair_out_size``       - the output size of ``eval_pairs.py:96-102``, in its own arithmetic.
* ``pair_intrinsics``     - ``rotate_intrinsics`` + ``resize_intrinsics`` as ``eval_pairs.py:91-104`` applies them.

No torch op computes anything on the images; no CPU fallback.
"""
import ctypes
import math

import numpy as np
import torch

from . import _lib

BRIGHTNESS, CONTRAST, SATURATION, HUE = 0, 1, 2, 3
_NAMES = ("brightness", "contrast", "saturation", "hue")


def _window(window, Hin, Win):
    if window is None:
        return 0, 0, Hin, Win
    if len(window) != 4:
        raise ValueError(f"window must be (top, left, height, width), got {window!r}")
    top, left, height, width = (int(v) for v in window)
    if height <= 0 or width <= 0:
        raise ValueError(f"window {window!r} is empty")
    return top, left, height, width


def _rows(order, factors, B):
    """order / factors as validated host arrays [B,4] (int32, float32); a [4] row is repeated for the batch."""
    if (order is None) != (factors is None):
        raise ValueError("order and factors go together (both or neither)")
    if order is None:
        return None, None
    order = torch.as_tensor(order).detach().to("cpu")
    factors = torch.as_tensor(factors).detach().to("cpu")
    if order.is_floating_point() or order.dtype == torch.bool:
        raise ValueError(f"order must hold integers, got {order.dtype}")
    order = order.to(torch.int64)
    factors = factors.to(torch.float32)
    out = []
    for name, t in (("order", order), ("factors", factors)):
        if t.dim() == 1 and t.shape[0] == 4:
            t = t.unsqueeze(0).expand(B, 4)
        if tuple(t.shape) != (B, 4):
            raise ValueError(f"{name} must be [{B},4] or [4], got {tuple(t.shape)}")
        out.append(t.contiguous())
    order, factors = out
    for b, (ops, fs) in enumerate(zip(order.tolist(), factors.tolist())):  # (lists: indexing a tensor 8 B times costs more than the kernels)
        seen = set()
        for k in range(4):
            op, f = ops[k], fs[k]
            if op < -1 or op > 3:
                raise ValueError(f"order[{b}][{k}] = {op}: an op is 0..3 (brightness, contrast, saturation, hue), -1 skips the slot")
            if op >= 0 and op in seen:
                raise ValueError(f"order[{b}] names {_NAMES[op]} twice")
            seen.add(op)
            if not math.isfinite(f):
                raise ValueError(f"the {_NAMES[k]} factor of image {b} is not finite")
            if k < 3 and f < 0:
                raise ValueError(f"the {_NAMES[k]} factor of image {b} is negative ({f})")
            if k == 3 and not -0.5 <= f <= 0.5:
                raise ValueError(f"the hue factor of image {b} is {f}, outside [-0.5, 0.5]")
    return order.to(torch.int32).contiguous(), factors


def prepare_images(rgb_u8, out_size=None, window=None, antialias=False, order=None, factors=None, return_rgb=False):
    """``rgb_u8`` ``[B,Hin,Win,3]`` uint8 on the device (interleaved RGB, what a JPEG decoder hands out) -> gray ``[B,1,Hout,Wout]``
    float32, contiguous: ``ToTensor`` (a true division by 255), the source ``window``, the resize, the jitter, ``rgb_to_grayscale``.

    ``window``   ``(top, left, height, width)`` in source coordinates, default the whole image.  It may reach outside the image and
                 reads zeros there: the reference's padding of the 968 x 1296 ScanNet frames is ``(-2, 0, 972, 1296)``, the
                 MegaDepth crop a square inside the image; ``window_intrinsics`` gives the matching intrinsics.
    ``out_size`` ``(Hout, Wout)``, default the window's size (no resize: the values are copied).  The window is resized with the
                 semantics of ``torch.nn.functional.interpolate(mode="bilinear", align_corners=False, antialias=antialias)``, which
                 is what ``torchvision.transforms.functional.resize`` calls on a tensor.
    ``antialias`` defaults to ``False``: torchvision's default for tensors was off in the releases of the reference's time and
                 is on from 0.17 - pass the value of the torchvision whose images the model was trained on.
    ``order`` / ``factors``  ``[B,4]`` or ``[4]`` (repeated for the batch), host values (a device tensor is read back): ``order[b]`` names
                 the op of each of the four slots - 0 brightness, 1 contrast, 2 saturation, 3 hue, -1 skips the slot -,
                 ``factors[b]`` = (brightness, contrast, saturation, hue).  ``None`` = no jitter.  ``color_jitter_params`` draws them.
    ``return_rgb`` also returns the jittered colour image ``[B,3,Hout,Wout]`` the gray value is taken of: ``(gray, rgb)``.

    One launch, or three when an image has a contrast slot; no host synchronisation; the same call gives the same bytes."""
    if not torch.is_tensor(rgb_u8):
        raise TypeError(f"prepare_images takes a tensor, got {type(rgb_u8).__name__}")
    if rgb_u8.dtype != torch.uint8:
        raise TypeError(f"prepare_images takes uint8 images (the decoder's output), got {rgb_u8.dtype}")
    if rgb_u8.dim() != 4 or rgb_u8.shape[3] != 3:
        raise ValueError(f"prepare_images takes interleaved RGB [B,Hin,Win,3], got {tuple(rgb_u8.shape)}")
    B, Hin, Win, _ = (int(v) for v in rgb_u8.shape)
    if B <= 0 or Hin <= 0 or Win <= 0:
        raise ValueError(f"prepare_images: empty input {tuple(rgb_u8.shape)}")
    top, left, wh, ww = _window(window, Hin, Win)
    Hout, Wout = (wh, ww) if out_size is None else (int(out_size[0]), int(out_size[1]))
    if Hout <= 0 or Wout <= 0:
        raise ValueError(f"out_size {out_size!r} is empty")
    order, factors = _rows(order, factors, B)
    if not rgb_u8.is_cuda:
        raise RuntimeError("prepare_images needs its images on an MI355X (no CPU fallback)")
    dev = rgb_u8.device
    rgb_u8 = rgb_u8.contiguous()
    gray = torch.empty((B, 1, Hout, Wout), dtype=torch.float32, device=dev)
    rgb = torch.empty((B, 3, Hout, Wout), dtype=torch.float32, device=dev) if return_rgb else None
    d = _lib.ImageFrontDesc(batch=B, in_height=Hin, in_width=Win, win_top=top, win_left=left, win_height=wh, win_width=ww,
                            out_height=Hout, out_width=Wout, antialias=1 if antialias else 0)
    po = order.data_ptr() if order is not None else None
    pf = factors.data_ptr() if factors is not None else None
    ctx = _lib.context(dev)
    with torch.cuda.device(dev):
        ctx.call("e2emv_image_front", ctypes.byref(d), _lib.ptr(rgb_u8), ctypes.cast(po, ctypes.POINTER(ctypes.c_int32)),
                 ctypes.cast(pf, ctypes.POINTER(ctypes.c_float)), _lib.ptr(gray), _lib.ptr(rgb), _lib.stream_ptr(dev))
    return (gray, rgb) if return_rgb else gray


def color_jitter_params(jitter, n_tuples, tuple_size, generator=None):
    """The jitter parameters of ``n_tuples`` tuples of ``tuple_size`` images: ONE draw per tuple, repeated for the tuple's images, as
    ``matching_dataset.py:167-169`` does.  Returns ``(order [n_tuples * tuple_size, 4] int32, factors [.., 4] float32)`` on the host,
    the arguments of ``prepare_images``.  The order is a uniform random permutation of the four ops; brightness, contrast and
    saturation are uniform on ``[1 - jitter, 1 + jitter]``, hue on ``[-jitter, jitter]`` - ``ColorJitter.get_params``' distribution,
    not its random stream.  ``generator``: a CPU ``torch.Generator`` for a reproducible draw."""
    jitter = float(jitter)
    if not 0.0 <= jitter <= 0.5:
        raise ValueError(f"jitter must be in [0, 0.5] (the hue shift is at most half a turn), got {jitter}")
    n_tuples, tuple_size = int(n_tuples), int(tuple_size)
    if n_tuples <= 0 or tuple_size <= 0:
        raise ValueError(f"n_tuples and tuple_size must be positive, got {n_tuples}, {tuple_size}")
    order = torch.stack([torch.randperm(4, generator=generator) for _ in range(n_tuples)]).to(torch.int32)
    u = torch.rand((n_tuples, 4), generator=generator, dtype=torch.float64)
    lo = torch.tensor([1.0 - jitter] * 3 + [-jitter], dtype=torch.float64)
    factors = (lo + 2.0 * jitter * u).to(torch.float32)
    factors[:, :3].clamp_(min=0.0)
    factors[:, 3].clamp_(-0.5, 0.5)
    return (order.repeat_interleave(tuple_size, dim=0).contiguous(), factors.repeat_interleave(tuple_size, dim=0).contiguous())


def window_intrinsics(K, window, out_size):
    """The intrinsics ``K`` (``[...,3,3]``, tensor or array; a new object is returned) of the image ``prepare_images`` makes of
    ``window`` = (top, left, height, width) and ``out_size`` = (Hout, Wout): the reference's ``crop_intrinsics(K, left, top)`` followed
    by ``resize_intrinsics(K, Wout / width, Hout / height)``.  The padding case falls out of a negative ``top``: (-2, 0, H + 4, W)
    gives the ``cy + 2`` of ``matching_dataset.py:195``."""
    if window is None:
        raise ValueError("window_intrinsics needs the window (top, left, height, width); the whole image is (0, 0, Hin, Win)")
    top, left, height, width = _window(window, 0, 0)
    Hout, Wout = int(out_size[0]), int(out_size[1])
    K = K.clone() if torch.is_tensor(K) else np.array(K, copy=True)
    if tuple(K.shape[-2:]) != (3, 3):
        raise ValueError(f"K must be [...,3,3], got {tuple(K.shape)}")
    fact_x, fact_y = Wout / width, Hout / height
    K[..., 0, 2] -= left
    K[..., 1, 2] -= top
    K[..., 0, 0] *= fact_x
    K[..., 1, 1] *= fact_y
    K[..., 0, 2] *= fact_x
    K[..., 1, 2] *= fact_y
    return K


# ---------------------------------------------------------------- pair evaluation (PairMatchingDataset.__getitem__, eval_pairs.py:85-108)
def _rot(rot):
    if isinstance(rot, bool) or not isinstance(rot, (int, np.integer)):
        raise ValueError(f"a turn is an int in 0..3 (quarter turns counter-clockwise, np.rot90's k), got {rot!r}")
    if not 0 <= rot <= 3:
        raise ValueError(f"a turn is 0..3 quarter turns, got {rot}")
    return int(rot)


def pair_out_size(shape, rot, img_size):
    """``(h_out, w_out)`` of a frame of ``shape`` = (H, W) as decoded, turned by ``rot`` quarter turns and resized to ``img_size``:
    ``eval_pairs.py:96-102`` in its own arithmetic.  The turned image ``h x w`` keeps its size when ``img_size == max(h, w)``;
    otherwise ``h >= w`` gives ``(img_size, int((w / h) * img_size))`` and ``h < w`` gives ``(int((h / w) * img_size), img_size)`` -
    Python's doubles and truncation, not an integer division: 10 x 7 at 720 is 503 columns."""
    H, W = int(shape[0]), int(shape[1])
    img_size = int(img_size)
    if H <= 0 or W <= 0 or img_size <= 0:
        raise ValueError(f"pair_out_size: shape {tuple(shape)!r} and img_size {img_size} must be positive")
    h, w = (W, H) if _rot(rot) % 2 else (H, W)
    if img_size == max(h, w):
        return h, w
    if h >= w:
        ar = w / h
        return img_size, int(ar * img_size)
    ar = h / w
    return int(ar * img_size), img_size


def pair_intrinsics(K, shape, rot, img_size):
    """The 3 x 3 intrinsics of the image ``prepare_pair_images`` makes of a frame of ``shape`` = (H, W) as decoded
    (``eval_pairs.py:91-104``): for ``rot != 0`` ``rotate_intrinsics(K, turned_shape, rot)`` of ``metrics.py``, then
    ``resize_intrinsics(K, w_out / w, h_out / h)``.  ``K``: array or tensor; a new one is returned, the input is left as it is."""
    from .metrics import rotate_intrinsics
    tensor = torch.is_tensor(K)
    Kn = K.detach().cpu().numpy().copy() if tensor else np.array(K, copy=True)
    if tuple(Kn.shape) != (3, 3):
        raise ValueError(f"K must be [3,3], got {tuple(Kn.shape)}")
    H, W = int(shape[0]), int(shape[1])
    rot = _rot(rot)
    h, w = (W, H) if rot % 2 else (H, W)
    h_out, w_out = pair_out_size((H, W), rot, img_size)
    if rot != 0:
        Kn = rotate_intrinsics(Kn, (h, w), rot)
    if (h_out, w_out) != (h, w):
        fact_x, fact_y = w_out / w, h_out / h
        Kn[0, 0] *= fact_x
        Kn[1, 1] *= fact_y
        Kn[0, 2] *= fact_x
        Kn[1, 2] *= fact_y
    return torch.from_numpy(Kn).to(device=K.device, dtype=K.dtype) if tensor else Kn


def prepare_pair_images(frames, img_size, rots=None, merge=False):
    """The image stage of pair evaluation (``eval_pairs.py:89-106``) for a list of decoded gray frames, as one launch:
    ``np.rot90(img, k=rot)``, ``cv2.resize`` to ``pair_out_size`` (``INTER_LINEAR`` on the float32 image) and ``/ 255.``.

    ``frames``   list of uint8 ``[H,W]`` tensors on the device (``cv2.imread(.., IMREAD_GRAYSCALE)``), of any sizes; a
                 non-contiguous one is made contiguous.
    ``img_size`` the longer side of every output (``eval_pairs.py``'s ``--img_size``: 720 for ScanNet, 1600 for MegaDepth / YFCC).
    ``rots``     one int per frame, 0..3 quarter turns counter-clockwise (the ``rots`` of the YFCC pair list); default all 0.
    ``merge``    ``False``: a list of contiguous float32 ``[1,1,h_out,w_out]`` tensors, views of one allocation in list order.
                 ``True``: one ``[n,1,h_out,w_out]`` tensor, ``ValueError`` when the output sizes differ - ``run_super_point``'s
                 ``merge`` flag (``eval_pairs.py:131-146``): ScanNet pairs merge, MegaDepth and YFCC pairs do not.

    A frame that already has ``img_size`` as its longer side is not resized: ``uint8 / 255`` with the bytes of the fp32 division.
    No torch op computes anything on the images, no host synchronisation, no CPU fallback; the same call gives the same bytes."""
    if not isinstance(frames, (list, tuple)):
        raise TypeError(f"prepare_pair_images takes a list of tensors, got {type(frames).__name__}")
    if len(frames) == 0:
        raise ValueError("prepare_pair_images: an empty list")
    for f in frames:
        if not torch.is_tensor(f):
            raise TypeError(f"prepare_pair_images takes tensors, got {type(f).__name__}")
        if f.dtype != torch.uint8:
            raise TypeError(f"prepare_pair_images takes uint8 frames (the decoder's output), got {f.dtype}")
    for f in frames:
        if f.dim() != 2 or f.shape[0] <= 0 or f.shape[1] <= 0:
            raise ValueError(f"prepare_pair_images takes gray frames [H,W], got {tuple(f.shape)}")
    n = len(frames)
    if n > _lib.IMAGE_FRONT_GRAY_MAX_IMAGES:
        raise ValueError(f"prepare_pair_images: {n} frames, a call takes up to {_lib.IMAGE_FRONT_GRAY_MAX_IMAGES}")
    if rots is None:
        rots = [0] * n
    if len(rots) != n:
        raise ValueError(f"prepare_pair_images: {n} frames and {len(rots)} turns")
    rots = [_rot(r) for r in rots]
    img_size = int(img_size)
    if img_size <= 0:
        raise ValueError(f"img_size must be positive, got {img_size}")
    sizes = [pair_out_size(f.shape, r, img_size) for f, r in zip(frames, rots)]
    for (h, w), f, r in zip(sizes, frames, rots):
        if h <= 0 or w <= 0:
            raise ValueError(f"a frame of {tuple(f.shape)} turned by {r} has an output side of 0 at img_size {img_size}")
    if merge and any(s != sizes[0] for s in sizes):
        raise ValueError(f"merge=True needs one output size, got {sorted(set(sizes))}")
    if not all(f.is_cuda for f in frames):
        raise RuntimeError("prepare_pair_images needs its frames on an MI355X (no CPU fallback)")
    dev = frames[0].device
    if any(f.device != dev for f in frames):
        raise RuntimeError("prepare_pair_images: the frames of a call are on one device")
    frames = [f.contiguous() for f in frames]
    numel = [h * w for h, w in sizes]
    out = torch.empty(sum(numel), dtype=torch.float32, device=dev)
    recs = (_lib.GrayImage * n)()
    for rec, f, r in zip(recs, frames, rots):
        rec.data, rec.height, rec.width, rec.rot = f.data_ptr(), int(f.shape[0]), int(f.shape[1]), r
    ctx = _lib.context(dev)
    with torch.cuda.device(dev):
        ctx.call("e2emv_image_front_gray", n, recs, img_size, _lib.ptr(out), _lib.stream_ptr(dev))
    if merge:
        return out.view(n, 1, sizes[0][0], sizes[0][1])
    views, at = [], 0
    for (h, w), k in zip(sizes, numel):
        views.append(out[at:at + k].view(1, 1, h, w))
        at += k
    return views
