"""Drop-in for ``models.models.superpoint.SuperPoint`` (absent submodule of the reference; constructed at ``train.py:335-341``,
``eval_pairs.py:197-202``, ``eval_multi_view.py:135-140``; called by ``helpers.run_super_point``, ``helpers.py:83-96``).

An ``nn.Module`` shell holding upstream's parameters (``conv1a`` ... ``convDb``, so upstream ``superpoint_v1.pth`` loads with
``load_state_dict``); ``forward({"image": [batch, ...]})`` hands the images to ``e2emv_superpoint_forward`` (csrc/superpoint.hip:
NHWC implicit-GEMM convolutions on the fp32 matrix cores, fused NMS / top-k / descriptor sampling kernels) and returns the
reference's dict of per-image lists: ``keypoints`` [n,2] (x, y), ``scores`` [n], ``descriptors`` [256,n].  No torch op
computes anything; no CPU fallback.
"""
import ctypes
import warnings

import torch
from torch import nn

from . import _lib

LAYERS = [("conv1a", 1, 64, 3), ("conv1b", 64, 64, 3), ("conv2a", 64, 64, 3), ("conv2b", 64, 64, 3), ("conv3a", 64, 128, 3),
          ("conv3b", 128, 128, 3), ("conv4a", 128, 128, 3), ("conv4b", 128, 128, 3), ("convPa", 128, 256, 3), ("convPb", 256, 65, 1),
          ("convDa", 128, 256, 3), ("convDb", 256, 256, 1)]
MAX_KEYPOINTS_CAPACITY = 4096


class SuperPoint(nn.Module):
    default_config = {"descriptor_dim": 256, "nms_radius": 4, "keypoint_threshold": 0.005, "max_keypoints": -1, "remove_borders": 4,
                      "fill_with_random_keypoints": False}

    def __init__(self, config=None):
        super().__init__()
        self.config = {**self.default_config, **(config or {})}
        for name, cin, cout, k in LAYERS:
            setattr(self, name, nn.Conv2d(cin, cout, kernel_size=k, stride=1, padding=k // 2))
        mk = self.config["max_keypoints"]
        if mk == 0 or mk > MAX_KEYPOINTS_CAPACITY:
            raise ValueError('"max_keypoints" must be positive (<= {}) or -1'.format(MAX_KEYPOINTS_CAPACITY))
        self._token = _lib.new_owner_token()
        self.requires_grad_(False)  # the reference runs SuperPoint frozen, under no_grad (helpers.py:86)

    def _upload(self, ctx):
        # one SuperPoint weight set per context: re-upload whenever another instance (or other values) own it
        owner = (self._token, tuple((p.data_ptr(), p._version) for p in self.parameters()))
        if ctx.sp_weights_owner == owner:
            return
        ctx.sp_weights_owner = None
        for k, v in self.state_dict().items():
            t = v.detach().to("cpu", torch.float32).contiguous()
            shape = (ctypes.c_int64 * t.dim())(*t.shape)
            ctx.call("e2emv_set_weight", ("superpoint." + k).encode(), ctypes.c_void_p(t.data_ptr()), shape, t.dim())
        ctx.call("e2emv_superpoint_commit")
        ctx.sp_weights_owner = owner

    def forward(self, data):
        images = data["image"]
        if torch.is_tensor(images):
            images = [images]
        out = {"keypoints": [], "scores": [], "descriptors": []}
        for batch in images:  # helpers.py:73-81: one merged batch, or one entry per image of the tuple
            if not batch.is_cuda:
                raise RuntimeError("SuperPoint needs its images on an MI355X (no CPU fallback)")
            dev = batch.device
            ctx = _lib.context(dev)
            self._upload(ctx)
            B, C, H, W = batch.shape
            if C != 1:
                raise AssertionError("SuperPoint takes one-channel images, got {}".format(tuple(batch.shape)))
            # the encoder pools three times: only the top-left (H//8*8) x (W//8*8) region yields keypoints, but upstream's
            # convolutions SEE the rows / columns beyond it before the pools floor them away.  Same here: the image goes in
            # zero-padded to the next multiple of 8 and the library masks every encoder level to its valid size.
            Hv, Wv = H, W
            if H % 8 or W % 8:
                Hp, Wp = (H + 7) // 8 * 8, (W + 7) // 8 * 8
                batch = torch.nn.functional.pad(batch, (0, Wp - W, 0, Hp - H))
                H, W = Hp, Wp
            img = batch.to(torch.float32).contiguous()
            cfg = self.config
            K = cfg["max_keypoints"] if cfg["max_keypoints"] > 0 else MAX_KEYPOINTS_CAPACITY
            d = _lib.SuperPointDesc(valid_height=Hv, valid_width=Wv, batch=B, height=H, width=W, nms_radius=int(cfg["nms_radius"]), max_keypoints=K,
                                    remove_borders=int(cfg["remove_borders"]), fill_random=1 if cfg["fill_with_random_keypoints"] else 0,
                                    keypoint_threshold=float(cfg["keypoint_threshold"]), seed=int(cfg.get("seed", 0)))
            kpts = torch.empty((B, K, 2), dtype=torch.float32, device=dev)
            scores = torch.empty((B, K), dtype=torch.float32, device=dev)
            desc = torch.empty((B, 256, K), dtype=torch.float32, device=dev)
            count = torch.empty((B,), dtype=torch.int32, device=dev)
            smap = torch.empty((B, Hv // 8 * 8, Wv // 8 * 8), dtype=torch.float32, device=dev) if cfg.get("return_score_map") else None
            with torch.cuda.device(dev), ctx.py_lock:
                self._upload(ctx)  # (again, now under the lock: another thread's model may have taken the context's weight set)
                ctx.call("e2emv_superpoint_forward", ctypes.byref(d), _lib.ptr(img), _lib.ptr(kpts), _lib.ptr(scores), _lib.ptr(desc),
                         _lib.ptr(count), _lib.ptr(smap), _lib.stream_ptr(dev))
            n = count.tolist()
            if cfg["max_keypoints"] <= 0 and max(n) >= MAX_KEYPOINTS_CAPACITY:
                warnings.warn("SuperPoint(max_keypoints=-1): an image reached the device capacity of {} keypoints; the lowest-"
                              "scoring candidates beyond it were dropped (upstream keeps all)".format(MAX_KEYPOINTS_CAPACITY))
            for b in range(B):
                out["keypoints"].append(kpts[b, :n[b]])
                out["scores"].append(scores[b, :n[b]])
                out["descriptors"].append(desc[b, :, :n[b]])
            if smap is not None:
                out.setdefault("score_map", []).append(smap)
        return out


def tap_shapes(B, H, W):
    """Shapes of the 12 taps of ``encode`` for [B,1,H,W] images (NHWC; tap 9: the 65 detector logits per cell, cells as rows)."""
    Hp, Wp, Hc, Wc = (H + 7) // 8 * 8, (W + 7) // 8 * 8, H // 8, W // 8
    return ([(B, Hp, Wp, 64)] + [(B, Hp // 2, Wp // 2, 64)] * 2 + [(B, Hp // 4, Wp // 4, 64), (B, Hp // 4, Wp // 4, 128)] + [(B, Hc, Wc, 128)] * 3 +
            [(B, Hc, Wc, 256), (B * Hc * Wc, 65), (B, Hc, Wc, 256), (B, Hc, Wc, 256)])


def encode(model, images, taps=False):
    """The head of ``SuperPoint.forward`` alone (``e2emv_superpoint_encode``: a building block for per-kernel parity tests): ``images``
    [B,1,H,W] on the device, padded and uploaded as ``forward`` does, go through the launches ``forward`` runs in front of its
    detector tail.  Returns ``(score, dense)`` - ``score`` [B,H//8*8,W//8*8], the map upstream's ``simple_nms`` receives, ``dense``
    [B,256,H//8,W//8], the UNnormalised output of the descriptor head - and with ``taps`` a third value: the list of the 12 layers'
    outputs as the next stage reads them (``tap_shapes``: NHWC on the zero-padded grid, masked to the valid size, up to layer 4, on
    the cell grid from layer 5 on)."""
    if not images.is_cuda:
        raise RuntimeError("SuperPoint needs its images on an MI355X (no CPU fallback)")
    dev = images.device
    ctx = _lib.context(dev)
    B, C, H, W = images.shape
    if C != 1:
        raise AssertionError("SuperPoint takes one-channel images, got {}".format(tuple(images.shape)))
    Hv, Wv = H, W
    if H % 8 or W % 8:
        Hp, Wp = (H + 7) // 8 * 8, (W + 7) // 8 * 8
        images = torch.nn.functional.pad(images, (0, Wp - W, 0, Hp - H))
        H, W = Hp, Wp
    img = images.to(torch.float32).contiguous()
    d = _lib.SuperPointDesc(valid_height=Hv, valid_width=Wv, batch=B, height=H, width=W)
    score = torch.empty((B, Hv // 8 * 8, Wv // 8 * 8), dtype=torch.float32, device=dev)
    nhwc = torch.empty((B, Hv // 8, Wv // 8, 256), dtype=torch.float32, device=dev)
    # (filled with NaN: a tap the library did not write in full cannot pass for one)
    tl = [torch.full(s, float("nan"), dtype=torch.float32, device=dev) for s in tap_shapes(B, Hv, Wv)] if taps else []
    tp, keep = _lib.ptr_array(tl) if taps else (None, None)
    with torch.cuda.device(dev), ctx.py_lock:
        model._upload(ctx)
        ctx.call("e2emv_superpoint_encode", ctypes.byref(d), _lib.ptr(img), _lib.ptr(score), _lib.ptr(nhwc), tp, _lib.stream_ptr(dev))
    dense = nhwc.permute(0, 3, 1, 2)
    return (score, dense, tl) if taps else (score, dense)


def detect(score, dense=None, **config):
    """The detector tail alone (``e2emv_superpoint_detect``: a building block for per-kernel parity tests): ``score`` [B,H,W] fp32 on
    the device is the map upstream's ``simple_nms`` receives, ``dense`` (optional) [B,256,H/8,W/8] the UNnormalised output of the
    descriptor head.  ``config`` takes the keys of ``SuperPoint.default_config`` (+ ``seed``).  Returns per-image lists like
    ``SuperPoint.forward`` (``descriptors`` only with ``dense``) plus ``score_map`` [B,H,W], the NMS-ed map, and ``raw``: the whole
    output buffers ``(kpts [B,K,2], scores [B,K], count [B], desc [B,256,K] or None)`` including the slots beyond each count."""
    cfg = {**SuperPoint.default_config, **config}
    if not score.is_cuda:
        raise RuntimeError("SuperPoint needs its score map on an MI355X (no CPU fallback)")
    mk = cfg["max_keypoints"]
    if mk == 0 or mk > MAX_KEYPOINTS_CAPACITY:
        raise ValueError('"max_keypoints" must be positive (<= {}) or -1'.format(MAX_KEYPOINTS_CAPACITY))
    dev = score.device
    ctx = _lib.context(dev)
    B, H, W = score.shape
    score = score.to(torch.float32).contiguous()
    K = mk if mk > 0 else MAX_KEYPOINTS_CAPACITY
    d = _lib.SuperPointDesc(valid_height=0, valid_width=0, batch=B, height=H, width=W, nms_radius=int(cfg["nms_radius"]), max_keypoints=K,
                            remove_borders=int(cfg["remove_borders"]), fill_random=1 if cfg["fill_with_random_keypoints"] else 0,
                            keypoint_threshold=float(cfg["keypoint_threshold"]), seed=int(cfg.get("seed", 0)))
    kpts = torch.empty((B, K, 2), dtype=torch.float32, device=dev)
    scores = torch.empty((B, K), dtype=torch.float32, device=dev)
    count = torch.empty((B,), dtype=torch.int32, device=dev)
    smap = torch.empty((B, H, W), dtype=torch.float32, device=dev)
    desc = nhwc = None
    if dense is not None:
        if tuple(dense.shape) != (B, 256, H // 8, W // 8):
            raise AssertionError("dense must be [B,256,H/8,W/8], got {}".format(tuple(dense.shape)))
        nhwc = dense.to(dev, torch.float32).permute(0, 2, 3, 1).contiguous()
        desc = torch.empty((B, 256, K), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev), ctx.py_lock:
        ctx.call("e2emv_superpoint_detect", ctypes.byref(d), _lib.ptr(score), _lib.ptr(nhwc), _lib.ptr(kpts), _lib.ptr(scores), _lib.ptr(count),
                 _lib.ptr(desc), _lib.ptr(smap), _lib.stream_ptr(dev))
    n = count.tolist()
    out = {"keypoints": [kpts[b, :n[b]] for b in range(B)], "scores": [scores[b, :n[b]] for b in range(B)], "score_map": smap,
           "raw": (kpts, scores, count, desc)}
    if desc is not None:
        out["descriptors"] = [desc[b, :, :n[b]] for b in range(B)]
    return out
