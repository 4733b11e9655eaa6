"""Drop-in for ``pose_optimization/two_view/estimate_relative_pose.py`` and
``compute_pose_error.py`` on top of libe2emv.so.

Same names, argument order, keyword names, ``info`` keys and ``None`` conventions as the
reference (``estimate_relative_pose.py:9-14, 16-31, 84-136``; ``compute_pose_error.py:3-22``);
the arithmetic runs in the HIP kernels of ``csrc/pose.hip`` (fp64 Gram / Jacobi instead of
the reference's library SVDs).  The pose is differentiable with respect to the confidences (training, the pose loss:
``_W8ptPose`` / ``e2emv_w8pt_backward``; all pairs of a tuple at once: ``_W8ptTuplePose`` / ``e2emv_w8pt_tuple_backward`` and
``pose_loss_tuple``); keypoints and the candidate choice carry no gradient.  No CPU fallback.
"""
import ctypes

import numpy as np
import torch

from . import _lib


def _dev_of(*tensors):
    for t in tensors:
        if t is not None and t.is_cuda:
            return t.device
    return torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else None


def _prep(t, dev):
    return t.to(dev, torch.float32).contiguous()


def _intr_batch(K, B):
    """[k,k] or [1|B,k,k] intrinsics -> (contiguous [nb,k,k], k, nb)."""
    if K.dim() == 2:
        K = K.unsqueeze(0)
    kdim = K.shape[-1]
    if K.shape[-2:] != (kdim, kdim) or kdim not in (3, 4) or K.shape[0] not in (1, B):
        raise AssertionError(K.shape)
    return K, kdim, K.shape[0]


def normalize(kpts, intr):
    """``normalize`` (:9-14): pixel -> camera coordinates (``e2emv_normalize_kpts``; stand-alone callers:
    ``eval_pairs.py:240-241``)."""
    dev = _dev_of(kpts, intr)
    ctx = _lib.context(dev)
    squeeze = kpts.dim() == 2
    k = _prep(kpts.unsqueeze(0) if squeeze else kpts, dev)
    B, N = k.shape[:2]
    K, kdim, nb = _intr_batch(_prep(intr, dev), B)
    out = torch.empty_like(k)
    if B * N:
        with torch.cuda.device(dev):
            ctx.call("e2emv_normalize_kpts", B, N, _lib.ptr(k), _lib.ptr(K), kdim, nb, _lib.ptr(out), _lib.stream_ptr(dev))
    return out[0] if squeeze else out


def get_kpts(data, result, id0, id1):
    """``get_kpts`` (:16-31) through ``e2emv_gather_matched`` (index -1 wraps to the last
    keypoint and gets weight 0, exactly like the reference's fancy indexing)."""
    if "keypoints" + str(id0) in data:
        k0, k1 = data["keypoints" + str(id0)], data["keypoints" + str(id1)]
    else:
        k0, k1 = data["keypoints{}_{}_{}".format(id0, id0, id1)], data["keypoints{}_{}_{}".format(id1, id0, id1)]
    matches = result["matches{}_{}_{}".format(id0, id0, id1)]
    conf = result["conf_scores_{}_{}".format(id0, id1)]
    dev = _dev_of(matches, k0)
    ctx = _lib.context(dev)
    k0d, k1d = _prep(k0, dev), _prep(k1, dev)
    m = matches.to(dev, torch.int64).contiguous()
    if torch.is_grad_enabled() and conf.requires_grad:
        cout, k1g = _MaskedConfidence.apply(conf, ctx, dev, k1d, m)
        return k0d, k1g, data["intr" + str(id0)], data["intr" + str(id1)], cout.unsqueeze(-1)
    c = _prep(conf.reshape(conf.shape[0], -1), dev)
    B, N0 = m.shape
    k1g = torch.empty((B, N0, 2), dtype=torch.float32, device=dev)
    cout = torch.empty((B, N0), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        ctx.call("e2emv_gather_matched", B, N0, k1d.shape[1], _lib.ptr(k1d), _lib.ptr(m), _lib.ptr(c), _lib.ptr(k1g),
                 _lib.ptr(cout), _lib.stream_ptr(dev))
    return k0d, k1g, data["intr" + str(id0)], data["intr" + str(id1)], cout.unsqueeze(-1)


def estimate_relative_pose_w8pt(kpts0, kpts1, intr0, intr1, confidence, choose_closest=False, T_021=None,
                                determine_inliers=False):
    """``estimate_relative_pose_w8pt`` (:84-128).  Returns ``(T_021 [B,4,4], info)`` or
    ``(None, None)`` when fewer than 8 correspondences are given (:85-86)."""
    if kpts0.shape[1] < 8:
        return None, None
    if kpts0.shape != kpts1.shape:
        raise AssertionError(kpts0.shape, kpts1.shape)
    dev = _dev_of(kpts0, kpts1, intr0, confidence)
    if dev is None:
        raise RuntimeError("estimate_relative_pose_w8pt needs an MI355X (no CPU fallback)")
    ctx = _lib.context(dev)
    B, N = kpts0.shape[:2]
    conf_shape = confidence.shape
    conf2 = confidence.reshape(B, -1)
    if conf2.shape[1] != N:
        raise AssertionError(conf_shape)
    k0, k1, cf = _prep(kpts0, dev), _prep(kpts1, dev), _prep(conf2, dev)
    K0, K1 = _prep(intr0, dev), _prep(intr1, dev)
    kdim = K0.shape[-1]
    if K0.dim() == 2:
        K0, K1 = K0.unsqueeze(0), K1.unsqueeze(0)
    if K0.shape[-2:] != (kdim, kdim) or K1.shape != K0.shape or K0.shape[0] not in (1, B):
        raise AssertionError(K0.shape, K1.shape)
    Tg = _prep(T_021, dev) if (choose_closest and T_021 is not None) else None
    if choose_closest and Tg is None:
        raise ValueError("choose_closest=True needs T_021")
    args = (ctx, dev, B, N, k0, k1, K0, K1, kdim, Tg, bool(choose_closest), bool(determine_inliers), conf_shape)
    if torch.is_grad_enabled() and confidence.requires_grad:
        # training (pose loss, helpers.py:253-258): T carries the graph back to the confidences (csrc/pose.hip, w8pt_backward)
        holder = []
        T = _W8ptPose.apply(conf2.to(dev, torch.float32), args, holder)
        return T, holder[0]
    return _w8pt_call(cf, *args)


def _w8pt_call(cf, ctx, dev, B, N, k0, k1, K0, K1, kdim, Tg, choose_closest, determine_inliers, conf_shape):
    T = torch.empty((B, 4, 4), dtype=torch.float32, device=dev)
    k0n, k1n = torch.empty_like(k0), torch.empty_like(k1)
    cfn = torch.empty((B, N), dtype=torch.float32, device=dev)
    # (the kernels write the masks as 0 / 1 bytes - the storage format of torch.bool: no conversion kernel behind the call)
    inl = torch.empty((B, N), dtype=torch.bool, device=dev) if determine_inliers else None
    pos = torch.empty((B, N), dtype=torch.bool, device=dev)
    F = torch.empty((B, 3, 3), dtype=torch.float32, device=dev)
    status = torch.empty((B,), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        ctx.call("e2emv_w8pt", B, N, _lib.ptr(k0), _lib.ptr(k1), _lib.ptr(K0), _lib.ptr(K1), kdim, K0.shape[0], _lib.ptr(cf),
                 1 if choose_closest else 0, _lib.ptr(Tg), 1 if determine_inliers else 0, _lib.ptr(T), _lib.ptr(k0n),
                 _lib.ptr(k1n), _lib.ptr(cfn), _lib.ptr(inl), _lib.ptr(pos), _lib.ptr(F), _lib.ptr(status),
                 _lib.stream_ptr(dev))
    info = {"kpts0_norm": k0n, "kpts1_norm": k1n, "confidence": cfn.reshape(conf_shape),
            "inliers": inl, "pos_depth_mask": pos,
            "F": F, "status": status}
    return T, info


class _W8ptPose(torch.autograd.Function):
    """T = w8pt(confidence): ``e2emv_w8pt`` forward, ``e2emv_w8pt_backward`` for dLoss/dconfidence (the keypoints and the
    candidate choice carry no gradient).  ``holder`` receives the ``info`` dict of the forward."""

    @staticmethod
    def forward(fctx, conf, args, holder):
        cf = conf.contiguous()
        T, info = _w8pt_call(cf, *args)
        holder.append(info)
        fctx.args = args
        fctx.save_for_backward(cf, T, info["kpts0_norm"], info["kpts1_norm"])
        return T

    @staticmethod
    def backward(fctx, gT):
        cf, T, k0n, k1n = fctx.saved_tensors
        ctx, dev, B, N = fctx.args[:4]
        g = gT.to(torch.float32).contiguous()
        gconf = torch.empty((B, N), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            ctx.call("e2emv_w8pt_backward", B, N, _lib.ptr(k0n), _lib.ptr(k1n), _lib.ptr(cf), _lib.ptr(T), _lib.ptr(g), _lib.ptr(gconf),
                     _lib.stream_ptr(dev))
        return gconf, None, None


class _MaskedConfidence(torch.autograd.Function):
    """``confidence = (matches >= 0) * conf_scores`` of ``get_kpts`` (:27-29) with the gather of image 1's keypoints:
    forward ``e2emv_gather_matched``, backward ``e2emv_apply_mask``."""

    @staticmethod
    def forward(fctx, conf, ctx, dev, k1d, m):
        B, N0 = m.shape
        c = conf.reshape(B, -1).to(dev, torch.float32).contiguous()
        k1g = torch.empty((B, N0, 2), dtype=torch.float32, device=dev)
        cout = torch.empty((B, N0), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            ctx.call("e2emv_gather_matched", B, N0, k1d.shape[1], _lib.ptr(k1d), _lib.ptr(m), _lib.ptr(c), _lib.ptr(k1g),
                     _lib.ptr(cout), _lib.stream_ptr(dev))
        fctx.misc = (ctx, dev, m, conf.shape)
        fctx.mark_non_differentiable(k1g)
        return cout, k1g

    @staticmethod
    def backward(fctx, gcout, _gk):
        ctx, dev, m, shape = fctx.misc
        g = gcout.to(torch.float32).contiguous()
        return mask_confidence(g, m >= 0).reshape(shape), None, None, None, None


def run_weighted_8_point(data, result, id0, id1, choose_closest=False, target_T_021=None):
    """``run_weighted_8_point`` (:130-136)."""
    match_key = "matches{}_{}_{}".format(id0, id0, id1)
    if match_key in result and result[match_key].shape[1] != 0:
        kpts0, kpts1, intr0, intr1, confidence = get_kpts(data, result, id0, id1)
        return estimate_relative_pose_w8pt(kpts0, kpts1, intr0, intr1, confidence, choose_closest=choose_closest,
                                           T_021=target_T_021)
    return None, None


def run_weighted_8_point_tuple(data, result, choose_closest=False, targets=None, determine_inliers=False):
    """Weighted 8-point pose of EVERY pair of the tuple in one batched solve (``e2emv_w8pt_tuple``): what the reference
    does by calling ``run_weighted_8_point`` inside its pair loops (``helpers.py:250-258``, ``bundle_adjust_io.py:62-100``),
    with 4 kernel launches per tuple batch instead of 4 per pair.  Returns ``{(id0, id1): (T_021 [B,4,4], info)}`` with
    the per-pair values of ``estimate_relative_pose_w8pt`` (views into the batched outputs) and ``(None, None)`` for a pair
    whose matches are missing.  ``targets``: ``{(id0, id1): T_021 [B,4,4]}`` when ``choose_closest``.  Images with
    different keypoint counts (or per-pair keypoint keys) go through the per-pair call.  With gradients enabled and a
    ``conf_scores_{i}_{j}`` that requires grad, the poses are views of one ``_W8ptTuplePose`` output and carry the graph back to the
    confidences of their pair (ONE ``e2emv_w8pt_tuple_backward``, bit-identical to the per-pair gradient; a pair that does not require
    grad gets ``None``); ``info["confidence"]`` stays graph-free as in the per-pair function."""
    T = 0
    while "keypoints" + str(T) in data:
        T += 1
    pairs = [(i, j) for j in range(T) for i in range(j)]
    mkeys = ["matches{}_{}_{}".format(i, i, j) for i, j in pairs]
    shapes = {tuple(data["keypoints" + str(t)].shape) for t in range(T)}
    batched = T >= 2 and len(shapes) == 1 and all(k in result for k in mkeys) and next(iter(shapes))[1] >= 8
    if batched and choose_closest and (targets is None or any(p not in targets for p in pairs)):
        raise ValueError("choose_closest=True needs a target T_021 for every pair")
    if not batched:
        out = {}
        for (i, j) in pairs:
            tgt = targets[(i, j)] if (choose_closest and targets is not None) else None
            out[(i, j)] = run_weighted_8_point(data, result, i, j, choose_closest=choose_closest, target_T_021=tgt)
        return out
    dev = _dev_of(result[mkeys[0]], data["keypoints0"])
    tg = [_prep(targets[p], dev) for p in pairs] if choose_closest else [None] * len(pairs)
    st = _tuple_state(data, result, T, pairs, dev, tg, choose_closest, determine_inliers)
    confs = [result["conf_scores_{}_{}".format(i, j)] for i, j in pairs]
    if torch.is_grad_enabled() and any(c.requires_grad for c in confs):
        # training: the poses are views of ONE output that carries the graph back to every pair's confidences (e2emv_w8pt_tuple_backward)
        Tout = _W8ptTuplePose.apply(st, *confs)
    else:
        Tout = _w8pt_tuple_call(st, [_prep(c.reshape(st["B"], -1), dev) for c in confs])
    o = st["out"]
    out = {}
    for q, p in enumerate(pairs):
        info = {"kpts0_norm": o["k0n"][q], "kpts1_norm": o["k1n"][q], "confidence": o["cfn"][q].reshape(confs[q].shape),
                "inliers": o["inl"][q] if o["inl"] is not None else None, "pos_depth_mask": o["pos"][q], "F": o["F"][q],
                "status": o["status"][q]}
        out[p] = (Tout[q], info)
    return out


def _tuple_state(data, result, T, pairs, dev, tg, choose_closest, determine_inliers, want_cf=False):
    """The device inputs of ``e2emv_w8pt_tuple`` apart from the confidences, which the caller hands over on their own (they may carry a
    graph).  ``tg``: one target [B,4,4] per pair (or ``None`` each); ``want_cf``: the solve also returns the gathered confidences."""
    B, N = data["keypoints0"].shape[:2]
    kpts = [_prep(data["keypoints" + str(t)], dev) for t in range(T)]
    intr = [_intr_batch(_prep(data["intr" + str(t)], dev), B) for t in range(T)]
    kdim, nb = intr[0][1], intr[0][2]
    if any(k[1:] != (kdim, nb) for k in intr):
        raise AssertionError("intrinsics of a tuple must share their layout")
    matches = [result["matches{}_{}_{}".format(i, i, j)].to(dev, torch.int64).contiguous() for i, j in pairs]
    if any(m.shape != (B, N) for m in matches) or any(result["conf_scores_{}_{}".format(i, j)].numel() != B * N for i, j in pairs):
        raise AssertionError("matches / conf_scores must be [B, N]")
    return {"ctx": _lib.context(dev), "dev": dev, "B": B, "T": T, "N": N, "P": len(pairs), "pairs": pairs, "kpts": kpts,
            "intr": [k[0] for k in intr], "kdim": kdim, "nb": nb, "matches": matches, "tg": tg, "choose_closest": bool(choose_closest),
            "determine_inliers": bool(determine_inliers), "want_cf": bool(want_cf)}


def _w8pt_tuple_call(st, conf):
    """One ``e2emv_w8pt_tuple`` on the prepared confidences ``conf`` ([B,N] fp32 per pair); the outputs go to ``st["out"]``, T [P,B,4,4] is
    returned."""
    ctx, dev, B, T, N, P = (st[k] for k in ("ctx", "dev", "B", "T", "N", "P"))
    inliers = st["determine_inliers"]
    o = {"T": torch.empty((P, B, 4, 4), dtype=torch.float32, device=dev),
         "k0n": torch.empty((P, B, N, 2), dtype=torch.float32, device=dev),
         "k1n": torch.empty((P, B, N, 2), dtype=torch.float32, device=dev),
         "cfn": torch.empty((P, B, N), dtype=torch.float32, device=dev),
         "inl": torch.empty((P, B, N), dtype=torch.bool, device=dev) if inliers else None,  # (0 / 1 bytes, see above)
         "pos": torch.empty((P, B, N), dtype=torch.bool, device=dev),
         "F": torch.empty((P, B, 3, 3), dtype=torch.float32, device=dev),
         "status": torch.empty((P, B), dtype=torch.int32, device=dev)}
    keep, args = [], []
    for lst in (st["kpts"], st["intr"], st["matches"], conf, st["tg"]):
        pa, arr = _lib.ptr_array(lst)
        keep.append(arr)
        args.append(pa)
    with torch.cuda.device(dev):
        ctx.call("e2emv_w8pt_tuple", B, T, N, args[0], args[1], st["kdim"], st["nb"], args[2], args[3], 1 if st["choose_closest"] else 0,
                 args[4], 1 if inliers else 0, _lib.ptr(o["T"]), _lib.ptr(o["k0n"]), _lib.ptr(o["k1n"]), _lib.ptr(o["cfn"]),
                 _lib.ptr(o["inl"]), _lib.ptr(o["pos"]), _lib.ptr(o["F"]), _lib.ptr(o["status"]), _lib.stream_ptr(dev))
    st["out"] = o
    return o["T"]


class _W8ptTuplePose(torch.autograd.Function):
    """T [P,B,4,4] = w8pt of every pair of the tuple as a function of the P confidence tensors: ``e2emv_w8pt_tuple`` forward, ONE
    ``e2emv_w8pt_tuple_backward`` for all dLoss/dconf_scores (keypoints, matches and the candidate choice carry no gradient).  With
    ``st["want_cf"]`` a second output: the gathered confidences ``(matches >= 0) * conf_scores`` [P*B,N] of ``get_kpts``, written by
    ``e2emv_gather_matched`` per pair (the per-pair path's numbers); their adjoint joins the backward call as ``d_gcf``."""

    @staticmethod
    def forward(fctx, st, *confs):
        ctx, dev, B, N, P = (st[k] for k in ("ctx", "dev", "B", "N", "P"))
        conf = [_prep(c.reshape(B, -1), dev) for c in confs]
        cf = None
        if st["want_cf"]:
            cf = torch.empty((P * B, N), dtype=torch.float32, device=dev)
            k1g = torch.empty((B, N, 2), dtype=torch.float32, device=dev)  # (the call's other output: not used here)
            with torch.cuda.device(dev):
                for q, (i, j) in enumerate(st["pairs"]):
                    ctx.call("e2emv_gather_matched", B, N, N, _lib.ptr(st["kpts"][j]), _lib.ptr(st["matches"][q]), _lib.ptr(conf[q]),
                             _lib.ptr(k1g), _lib.ptr(cf[q * B:(q + 1) * B]), _lib.stream_ptr(dev))
        T = _w8pt_tuple_call(st, conf)
        fctx.st = {k: v for k, v in st.items() if k != "out"}  # (the outputs reach the backward as saved tensors only: no cycle through T)
        fctx.meta =[(c.shape, c.dtype, c.device) for c in confs]
        fctx.save_for_backward(T, st["out"]["k0n"], st["out"]["k1n"], *conf)
        return (T, cf) if st["want_cf"] else T

    @staticmethod
    def backward(fctx, gT, gcf=None):
        st = fctx.st
        ctx, dev, B, T_, N, P = (st[k] for k in ("ctx", "dev", "B", "T", "N", "P"))
        T, k0n, k1n = fctx.saved_tensors[:3]
        conf = list(fctx.saved_tensors[3:])
        g = _prep(gT, dev)
        gc = _prep(gcf, dev) if gcf is not None else None
        gconf = [torch.empty((B, N), dtype=torch.float32, device=dev) if fctx.needs_input_grad[1 + q] else None for q in range(P)]
        pm, keep_m = _lib.ptr_array(st["matches"])
        pc, keep_c = _lib.ptr_array(conf)
        pg, keep_g = _lib.ptr_array(gconf)
        with torch.cuda.device(dev):
            ctx.call("e2emv_w8pt_tuple_backward", B, T_, N, pm, pc, _lib.ptr(k0n), _lib.ptr(k1n), _lib.ptr(T), _lib.ptr(g), _lib.ptr(gc), pg,
                     _lib.stream_ptr(dev))
        return (None,) + tuple(None if gq is None else gq.reshape(shape).to(cdev, dtype) for gq, (shape, dtype, cdev) in zip(gconf, fctx.meta))


def _pose_error_buffers(T0, T1, means):
    dev = _dev_of(T0, T1)
    ctx = _lib.context(dev)
    a, b = _prep(T0, dev), _prep(T1, dev)
    B = a.shape[0]
    rot = torch.empty((B,), dtype=torch.float32, device=dev)
    tr = torch.empty((B,), dtype=torch.float32, device=dev)
    valid = torch.empty((B,), dtype=torch.bool, device=dev)  # (0 / 1 bytes)
    m2 = torch.empty((2,), dtype=torch.float32, device=dev) if means else None
    with torch.cuda.device(dev):
        ctx.call("e2emv_pose_error_means", B, _lib.ptr(a), _lib.ptr(b), _lib.ptr(rot), _lib.ptr(tr), _lib.ptr(valid),
                 _lib.ptr(m2), _lib.stream_ptr(dev))
    return rot, tr, valid, m2


def pose_errors(T0, T1):
    """Per-sample (rotation, translation-direction) angle errors in radians on the device, fixed shape [B] each
    (entries whose translation norm product is <= 1e-6 read 0)."""
    rot, tr, _, _ = _pose_error_buffers(T0, T1, means=False)
    return rot, tr


class _PoseErrors(torch.autograd.Function):
    """(rot [B], transl [B], valid [B]) = pose errors of T0 against T1 with the gradient w.r.t. T0 (``e2emv_pose_errors_backward``):
    the two error functions as the pose LOSS of ``helpers.run_matcher`` (helpers.py:256-258)."""

    @staticmethod
    def forward(fctx, T0, T1):
        rot, tr, valid, _ = _pose_error_buffers(T0, T1, means=False)
        fctx.save_for_backward(_prep(T0, rot.device), _prep(T1, rot.device))
        fctx.mark_non_differentiable(valid)
        return rot, tr, valid

    @staticmethod
    def backward(fctx, g_rot, g_tr, _gv):
        a, b = fctx.saved_tensors
        dev, B = a.device, a.shape[0]
        ctx = _lib.context(dev)
        gr = (torch.zeros(B, device=dev) if g_rot is None else g_rot).to(torch.float32).contiguous()
        gt = (torch.zeros(B, device=dev) if g_tr is None else g_tr).to(torch.float32).contiguous()
        gT = torch.empty((B, 4, 4), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            ctx.call("e2emv_pose_errors_backward", B, _lib.ptr(a), _lib.ptr(b), _lib.ptr(gr), _lib.ptr(gt), _lib.ptr(gT), _lib.stream_ptr(dev))
        return gT, None


def _wants_grad(T0):
    return torch.is_grad_enabled() and torch.is_tensor(T0) and T0.requires_grad


def compute_rotation_error(T0, T1, reduce=True):
    """``compute_rotation_error`` (compute_pose_error.py:3-12); the mean is reduced on the device.  Differentiable with respect to
    ``T0`` when it carries a graph (the rotation loss of ``helpers.run_matcher``)."""
    if _wants_grad(T0):
        rot, _, _ = _PoseErrors.apply(T0, T1)
        return rot.mean() if reduce else rot
    rot, _, _, m2 = _pose_error_buffers(T0, T1, means=reduce)
    return m2[0] if reduce else rot


def compute_translation_error_as_angle(T0, T1, reduce=True):
    """``compute_translation_error_as_angle`` (compute_pose_error.py:14-22): only the entries whose norm product
    exceeds 1e-6 count - ``reduce=True`` averages over them on the device, ``reduce=False`` returns exactly those
    entries (shape [n_valid], like the reference's boolean indexing).  Differentiable with respect to ``T0`` like the above."""
    if _wants_grad(T0):
        _, tr, valid = _PoseErrors.apply(T0, T1)
        sel = tr[valid]
        return sel.mean() if reduce else sel
    _, tr, valid, m2 = _pose_error_buffers(T0, T1, means=reduce)
    return m2[1] if reduce else tr[valid]


def mask_confidence(confidence, mask):
    """``confidence[~mask] = 0`` as a new tensor, on the device (``e2emv_apply_mask``): the step between the weighted 8-point
    solve and the two-view bundle adjustment (``eval_pairs.py:250-251``, ``bundle_adjust_io.py:18-19``).  Differentiable with respect
    to ``confidence`` (``_MaskConfidence``: the same kernel on the incoming gradient)."""
    if torch.is_grad_enabled() and confidence.requires_grad:
        return _MaskConfidence.apply(confidence, mask)
    dev = _dev_of(confidence, mask)
    ctx = _lib.context(dev)
    c = _prep(confidence, dev)
    m = mask.to(dev).reshape(c.shape).to(torch.uint8).contiguous() if mask.dtype != torch.uint8 else mask.to(dev).reshape(c.shape).contiguous()
    out = torch.empty_like(c)
    if c.numel():
        with torch.cuda.device(dev):
            ctx.call("e2emv_apply_mask", c.numel(), _lib.ptr(c), _lib.ptr(m), _lib.ptr(out), _lib.stream_ptr(dev))
    return out


class _MaskConfidence(torch.autograd.Function):
    """``mask_confidence`` with its gradient: ``e2emv_apply_mask`` forward, and on the incoming gradient backward."""

    @staticmethod
    def forward(fctx, confidence, mask):
        fctx.mask = mask
        return mask_confidence(confidence.detach(), mask)

    @staticmethod
    def backward(fctx, g):
        return mask_confidence(g, fctx.mask), None


LOSSES = {None: 0, "huber": 1, "cauchy": 2}  # E2EMV_LOSS_* of include/e2emv.h


def _check_loss(loss, loss_scale):
    """``loss`` is ``None``, "huber" or "cauchy"; a loss needs a finite positive ``loss_scale`` and no loss takes none: checked on
    the host before any device call.  Returns the code of the C ABI."""
    if not (loss is None or isinstance(loss, str)) or loss not in LOSSES:
        raise ValueError("loss must be None, \"huber\" or \"cauchy\", not {!r}".format(loss))
    if loss is None:
        if loss_scale is not None:
            raise ValueError("loss_scale={!r} needs a loss: without one there is nothing to scale".format(loss_scale))
        return 0
    if loss_scale is None:
        raise ValueError("loss={!r} needs a loss_scale".format(loss))
    if isinstance(loss_scale, bool) or not isinstance(loss_scale, (int, float, np.integer, np.floating)) or not np.isfinite(loss_scale) or not loss_scale > 0:
        raise ValueError("loss_scale must be a finite positive number, not {!r}".format(loss_scale))
    return LOSSES[loss]


def run_bundle_adjust_2_view(kpts0_norm, kpts1_norm, confidence, init_T021, n_iterations, check_lu_info_strict=False,
                             check_precond_strict=False, loss=None, loss_scale=None, return_summary=False, loss_backward=False):
    """``run_bundle_adjust_2_view`` (estimate_relative_pose.py:138-144): returns ``(refined T_021 of the valid samples
    [n_valid,4,4], valid_batch [B] bool)`` so that ``pred_T021[valid] = refined`` works as at ``eval_pairs.py:252-255``.
    Differentiable with respect to ``confidence`` and ``init_T021`` (``_Ba2ViewPose`` / ``e2emv_ba_2view_backward``: the exact reverse of
    the LM loop; keypoints, lambda and the accept / reject decisions carry no gradient).  A robust loss with a graph requested raises
    ``NotImplementedError`` before any device call unless ``loss_backward=True``: then ``T`` carries the graph of the robust loop
    (``e2emv_ba_2view_loss`` / ``e2emv_ba_2view_loss_backward``: through the corrector and through the pair's scale, which moves with
    the confidences).  ``loss_backward=True`` without a loss, or a value that is not a bool, is a ``ValueError``.
    The two ``*_strict`` flags only matter for singular systems, which the fp64 Schur solve reports the same way.
    ``loss``: ``None`` (default: the reference's squared loss, ``e2emv_ba_2view`` as always), "huber" or "cauchy"
    (``e2emv_ba_2view_loss``): a residual block is one observation - a match has one in each image -, the LM loop compares
    ``sum rho`` and the blocks are linearised with Ceres' corrector.  ``loss_scale`` is RELATIVE, as in
    ``multi_view.solve_tuple_poses_batch``: the weights of a pair are its confidences over a per-pair constant, the scale is
    divided by the same constant on the device, and the loss acts on ``confidence x residual`` in normalised image coordinates -
    ``loss_scale`` = pixels / focal length at confidence 1 (one pixel at f = 600: ``1 / 600``), whatever the number of matches.
    ``ValueError`` before any device call for another name, a loss without a scale, a scale without a loss, or a scale that is
    not a finite positive number.  ``return_summary``: a third value, ``float64 [B,4]`` on the device, for EVERY sample: cost at
    the start, best cost, number of evaluations that improved, the absolute scale used (0 without a loss); zero for an invalid
    sample."""
    code = _check_loss(loss, loss_scale)
    if not isinstance(loss_backward, bool):
        raise ValueError("loss_backward must be True or False, not {!r}".format(loss_backward))
    if loss_backward and not code:
        raise ValueError("loss_backward=True needs a loss: the squared loss (loss=None) has its backward pass without it")
    graph = torch.is_grad_enabled() and any(torch.is_tensor(t) and t.requires_grad for t in (confidence, init_T021))
    if graph and code and not loss_backward:
        raise NotImplementedError("run_bundle_adjust_2_view: loss={!r} with a graph: by default the gradient is that of the squared loss "
                                  "only (loss=None) - pass loss_backward=True for the backward pass through the robust loss, or detach "
                                  "confidence and init_T021 to refine without a graph".format(loss))
    dev = _dev_of(kpts0_norm, kpts1_norm, init_T021)
    ctx = _lib.context(dev)
    B, N = kpts0_norm.shape[:2]
    k0, k1 = _prep(kpts0_norm, dev), _prep(kpts1_norm, dev)
    if graph:
        holder = []
        conf_in, T_in = confidence.reshape(B, -1), init_T021
        To = _Ba2ViewPose.apply(conf_in, T_in, ctx, dev, k0, k1, int(n_iterations), bool(return_summary), holder, code,
                                float(loss_scale) if code else 0.0)
        vb, summary = holder
        return (To[vb], vb, summary) if return_summary else (To[vb], vb)
    cf = _prep(confidence.reshape(B, -1), dev)
    Ti = _prep(init_T021, dev)
    To = torch.empty((B, 4, 4), dtype=torch.float32, device=dev)
    valid = torch.empty((B,), dtype=torch.uint8, device=dev)
    summary = torch.empty((B, 4), dtype=torch.float64, device=dev) if return_summary else None
    head = (B, N, _lib.ptr(k0), _lib.ptr(k1), _lib.ptr(cf), _lib.ptr(Ti), int(n_iterations), _lib.ptr(To), _lib.ptr(valid))
    with torch.cuda.device(dev):
        if code or return_summary:
            ctx.call("e2emv_ba_2view_loss", *head, code, float(loss_scale) if code else 0.0, _lib.ptr(summary), _lib.stream_ptr(dev))
        else:
            ctx.call("e2emv_ba_2view", *head, _lib.stream_ptr(dev))
    vb = valid.bool()
    return (To[vb], vb, summary) if return_summary else (To[vb], vb)


class _Ba2ViewPose(torch.autograd.Function):
    """T [B,4,4] = two-view BA of every sample (an invalid one keeps its start): ``e2emv_ba_2view`` forward, ``e2emv_ba_2view_backward`` for
    dLoss/dconfidence and dLoss/dinit_T021.  ``holder`` receives ``valid_batch`` and the summary (or ``None``); the selection of the valid
    samples stays a torch op on top.  ``code``, ``loss_scale``: a robust loss (``LOSSES``) - then ``e2emv_ba_2view_loss`` forward and
    ``e2emv_ba_2view_loss_backward`` backward; code 0 makes the calls above."""

    @staticmethod
    def forward(fctx, conf, T_init, ctx, dev, k0, k1, n_iterations, want_summary, holder, code=0, loss_scale=0.0):
        B, N = k0.shape[:2]
        cf, Ti = _prep(conf, dev), _prep(T_init, dev)
        To = torch.empty((B, 4, 4), dtype=torch.float32, device=dev)
        valid = torch.empty((B,), dtype=torch.uint8, device=dev)
        summary = torch.empty((B, 4), dtype=torch.float64, device=dev) if want_summary else None
        head = (B, N, _lib.ptr(k0), _lib.ptr(k1), _lib.ptr(cf), _lib.ptr(Ti), n_iterations, _lib.ptr(To), _lib.ptr(valid))
        with torch.cuda.device(dev):
            if code or want_summary:
                ctx.call("e2emv_ba_2view_loss", *head, code, loss_scale if code else 0.0, _lib.ptr(summary), _lib.stream_ptr(dev))
            else:
                ctx.call("e2emv_ba_2view", *head, _lib.stream_ptr(dev))
        holder.extend([valid.bool(), summary])
        fctx.misc = (ctx, dev, n_iterations, conf.shape, conf.dtype, conf.device, T_init.dtype, T_init.device, code, loss_scale)
        fctx.save_for_backward(k0, k1, cf, Ti)
        return To

    @staticmethod
    def backward(fctx, gT):
        k0, k1, cf, Ti = fctx.saved_tensors
        ctx, dev, n_iterations, cshape, cdtype, cdev, tdtype, tdev, code, loss_scale = fctx.misc
        B, N = k0.shape[:2]
        g = _prep(gT, dev)
        gconf = torch.empty((B, N), dtype=torch.float32, device=dev) if fctx.needs_input_grad[0] else None
        gTi = torch.empty((B, 4, 4), dtype=torch.float32, device=dev) if fctx.needs_input_grad[1] else None
        head = (B, N, _lib.ptr(k0), _lib.ptr(k1), _lib.ptr(cf), _lib.ptr(Ti), n_iterations)
        with torch.cuda.device(dev):
            if code:
                ctx.call("e2emv_ba_2view_loss_backward", *head, code, loss_scale, _lib.ptr(g), _lib.ptr(gconf), _lib.ptr(gTi), _lib.stream_ptr(dev))
            else:
                ctx.call("e2emv_ba_2view_backward", *head, _lib.ptr(g), _lib.ptr(gconf), _lib.ptr(gTi), _lib.stream_ptr(dev))
        if gconf is not None:
            gconf = gconf.reshape(cshape).to(cdev, cdtype)
        if gTi is not None:
            gTi = gTi.to(tdev, tdtype)
        return gconf, gTi, None, None, None, None, None, None, None, None, None


class _PoseLossTuple(torch.autograd.Function):
    """losses2 [2] = (sum over the pairs of the mean rotation error, sum over the pairs of the mean translation-angle error over the valid
    entries) of T [P*B,4,4] against the targets: ``e2emv_pose_loss_tuple`` forward, ``e2emv_pose_loss_tuple_backward`` for dLoss/dT - the
    incoming gradient stays on the device."""

    @staticmethod
    def forward(fctx, T, Tgt, ctx, dev, P, B):
        a = _prep(T, dev)
        l2 = _pose_loss_tuple_call(ctx, dev, P, B, a, Tgt)
        fctx.misc = (ctx, dev, P, B, T.shape)
        fctx.save_for_backward(a, Tgt)
        return l2

    @staticmethod
    def backward(fctx, g2):
        a, Tgt = fctx.saved_tensors
        ctx, dev, P, B, shape = fctx.misc
        g = _prep(g2, dev)
        gT = torch.empty((P * B, 4, 4), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            ctx.call("e2emv_pose_loss_tuple_backward", P, B, _lib.ptr(a), _lib.ptr(Tgt), _lib.ptr(g), _lib.ptr(gT), _lib.stream_ptr(dev))
        return gT.reshape(shape), None, None, None, None, None


def _pose_loss_tuple_call(ctx, dev, P, B, T, Tgt):
    rot = torch.empty((P * B,), dtype=torch.float32, device=dev)
    tr = torch.empty((P * B,), dtype=torch.float32, device=dev)
    valid = torch.empty((P * B,), dtype=torch.uint8, device=dev)
    l2 = torch.empty((2,), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        ctx.call("e2emv_pose_loss_tuple", P, B, _lib.ptr(T), _lib.ptr(Tgt), _lib.ptr(rot), _lib.ptr(tr), _lib.ptr(valid), _lib.ptr(l2),
                 _lib.stream_ptr(dev))
    return l2


def pose_loss_tuple(data, result, ba_iterations=0, ba_loss=None, ba_loss_scale=None):
    """The pose term of ``helpers.run_matcher`` (helpers.py:243-260) for ALL pairs of the tuple at once: per pair the target
    ``inv(pose_j) @ pose_i``, ``run_weighted_8_point(..., choose_closest=True)``, rotation plus translation-angle error, summed over the
    pairs.  Returns ``{"rot_loss", "transl_loss", "poses": {(i, j): T_021 [B,4,4]}}``; the two losses are 0-dim device tensors that
    carry the graph back to every ``conf_scores_{i}_{j}`` that requires grad.  A fixed number of device calls whatever the batch size,
    and no host synchronisation: P ``e2emv_relative_pose`` into one target buffer, ``e2emv_w8pt_tuple``, ``e2emv_pose_loss_tuple``
    forward; ``e2emv_pose_loss_tuple_backward`` and ``e2emv_w8pt_tuple_backward`` backward.  ``ba_iterations > 0``: the loss is taken
    on the pose refined by the two-view bundle adjustment of all P*B samples in one call - the gathered confidences
    (P ``e2emv_gather_matched``), ``mask_confidence`` with the positive-depth mask, ``e2emv_ba_2view`` / ``e2emv_ba_2view_backward``; a
    sample with fewer than 7 usable matches keeps its w8pt pose and passes its gradient through.  ``ba_loss``, ``ba_loss_scale``: the
    loss of that refinement, with the meaning and the rules of ``run_bundle_adjust_2_view``'s ``loss`` and ``loss_scale`` (``None``, the
    default: the squared loss, the calls above; "huber" or "cauchy": ``e2emv_ba_2view_loss`` / ``e2emv_ba_2view_loss_backward`` in their
    place, the same number of calls) - wrong matches, which a matcher in training produces, pull the squared-loss refinement away
    and with it the pose the term is taken on.  ``ValueError`` before any device call: fewer than 8 keypoints, images with different
    keypoint counts, a missing ``pose{t}``, a missing pair in ``result``, a negative ``ba_iterations``, a bad ``ba_loss`` /
    ``ba_loss_scale`` pair, a ``ba_loss`` with ``ba_iterations == 0``."""
    T = 0
    while "keypoints" + str(T) in data:
        T += 1
    if T < 2 or T > _lib.MAX_TUPLE:
        raise ValueError("pose_loss_tuple takes tuples of 2..{} images, not {}".format(_lib.MAX_TUPLE, T))
    if isinstance(ba_iterations, bool) or int(ba_iterations) != ba_iterations or ba_iterations < 0:
        raise ValueError("ba_iterations must be a non-negative integer, not {!r}".format(ba_iterations))
    ba_iterations = int(ba_iterations)
    ba_code = _check_loss(ba_loss, ba_loss_scale)
    if ba_code and ba_iterations == 0:
        raise ValueError("ba_loss={!r} needs ba_iterations > 0: without a refinement there is nothing it acts on".format(ba_loss))
    shapes = {tuple(data["keypoints" + str(t)].shape) for t in range(T)}
    if len(shapes) != 1:
        raise ValueError("pose_loss_tuple needs the same number of keypoints in every image, got {}".format(sorted(shapes)))
    if next(iter(shapes))[1] < 8:
        raise ValueError("pose_loss_tuple needs at least 8 keypoints per image, got {}".format(next(iter(shapes))[1]))
    missing = ["pose" + str(t) for t in range(T) if "pose" + str(t) not in data]
    pairs = [(i, j) for j in range(T) for i in range(j)]
    missing += [k for i, j in pairs for k in ("matches{}_{}_{}".format(i, i, j), "conf_scores_{}_{}".format(i, j)) if k not in result]
    if missing:
        raise ValueError("pose_loss_tuple: missing {}".format(", ".join(missing)))
    dev = _dev_of(result["matches0_0_1"], data["keypoints0"])
    ctx = _lib.context(dev)
    B = data["keypoints0"].shape[0]
    P = len(pairs)
    poses = [_prep(data["pose" + str(t)], dev) for t in range(T)]
    Tgt = torch.empty((P * B, 4, 4), dtype=torch.float32, device=dev)
    tg = [Tgt[q * B:(q + 1) * B] for q in range(P)]
    with torch.cuda.device(dev):
        for q, (i, j) in enumerate(pairs):  # target of pair (i, j): inv(pose_j) @ pose_i (helpers.py:254)
            ctx.call("e2emv_relative_pose", B, _lib.ptr(poses[i]), _lib.ptr(poses[j]), _lib.ptr(tg[q]), _lib.stream_ptr(dev))
    st = _tuple_state(data, result, T, pairs, dev, tg, True, False, want_cf=ba_iterations > 0)
    confs = [result["conf_scores_{}_{}".format(i, j)] for i, j in pairs]
    graph = torch.is_grad_enabled() and any(c.requires_grad for c in confs)
    with torch.set_grad_enabled(graph):
        solved = _W8ptTuplePose.apply(st, *confs)
        o = st["out"]
        if ba_iterations > 0:
            Tw, cf = solved
            cm = mask_confidence(cf, o["pos"].reshape(P * B, -1))
            Tp = _Ba2ViewPose.apply(cm, Tw.reshape(P * B, 4, 4), ctx, dev, o["k0n"].reshape(P * B, -1, 2), o["k1n"].reshape(P * B, -1, 2),
                                    ba_iterations, False, [], ba_code, float(ba_loss_scale) if ba_code else 0.0)
        else:
            Tp = solved.reshape(P * B, 4, 4)
        l2 = _PoseLossTuple.apply(Tp, Tgt, ctx, dev, P, B) if graph else _pose_loss_tuple_call(ctx, dev, P, B, Tp, Tgt)
    Tq = Tp.reshape(P, B, 4, 4)
    return {"rot_loss": l2[0], "transl_loss": l2[1], "poses": {p: Tq[q] for q, p in enumerate(pairs)}}
