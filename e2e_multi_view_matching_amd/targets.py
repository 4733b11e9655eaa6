"""Match targets and match loss on the device: the two data-parallel N^2 steps of the reference's training and validation
passes, ``helpers.compute_gt_matches_of_image_pair`` (:121-203) and ``helpers.compute_match_loss`` (:228-241), on top of
libe2emv.so (``csrc/gtmatch.hip``).  The reference's own ``helpers.compute_gt_matches`` / ``helpers.run_matcher`` stay
the callers (they only loop over the pairs of a tuple); ``gt_matches_for_tuple`` is the batched equivalent of that loop
for device-resident data.  All pairs of a tuple at once: ``gt_matches_tuple`` (one call for every pair's targets) and
``match_loss_tuple`` (one call for the summed loss, one more for its backward to every ``scores_{i}_{j}``:
``_MatchLossTuple``); ``compute_match_loss`` carries the graph the same way when its scores require grad.  The targets
themselves carry no gradient.  No CPU fallback."""
import torch

from . import _lib
from .pose import _dev_of, _prep


def compute_gt_matches_of_image_pair(kpts0, kpts1, K0, K1, T0to1, depth0, depth1, max_matched_reproj_err,
                                     min_unmatched_reproj_err):
    """-> (indices [B,2,N+1] int64, weights [B,2,N+1] f32), exactly the pair ``helpers.py:203`` returns."""
    if kpts0.shape != kpts1.shape:
        raise AssertionError(kpts0.shape, kpts1.shape)
    dev = _dev_of(kpts0, depth0)
    ctx = _lib.context(dev)
    B, N = kpts0.shape[:2]
    k0, k1 = _prep(kpts0, dev), _prep(kpts1, dev)
    Ka, Kb, T = _prep(K0, dev), _prep(K1, dev), _prep(T0to1, dev)
    if Ka.shape[-2:] != (4, 4) or T.shape[-2:] != (4, 4):
        raise AssertionError("intrinsics and pose must be 4x4 (MatchingDataset layout)")
    d0, d1 = _prep(depth0, dev), _prep(depth1, dev)
    H, W = d0.shape[-2:]
    idx = torch.empty((B, 2, N + 1), dtype=torch.int64, device=dev)
    w = torch.empty((B, 2, N + 1), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        ctx.call("e2emv_gt_matches", B, N, _lib.ptr(k0), _lib.ptr(k1), _lib.ptr(Ka), _lib.ptr(Kb), _lib.ptr(T), _lib.ptr(d0),
                 _lib.ptr(d1), H, W, float(max_matched_reproj_err), float(min_unmatched_reproj_err), _lib.ptr(idx), _lib.ptr(w),
                 _lib.stream_ptr(dev))
    return idx, w


def relative_pose(pose_from, pose_to):
    """``inv(pose_to) @ pose_from`` per batch element on the device (the relative pose ``helpers.py:219, 254`` builds with
    torch ops): [B,4,4] x [B,4,4] -> [B,4,4]."""
    dev = _dev_of(pose_from, pose_to)
    ctx = _lib.context(dev)
    a, b = _prep(pose_from, dev), _prep(pose_to, dev)
    if a.shape != b.shape or a.shape[-2:] != (4, 4):
        raise AssertionError(a.shape, b.shape)
    out = torch.empty_like(a)
    with torch.cuda.device(dev):
        ctx.call("e2emv_relative_pose", a.shape[0], _lib.ptr(a), _lib.ptr(b), _lib.ptr(out), _lib.stream_ptr(dev))
    return out


def gt_matches_for_tuple(data, max_matched_reproj_err, min_unmatched_reproj_err, n_images=None):
    """Ground-truth match targets of every pair of a device-resident tuple: returns
    ``{(k, m): (indices, weights)}`` for k < m, the values ``helpers.compute_gt_matches`` stores under
    ``gt_indices_k_m`` / ``gt_weights_k_m``.  Does not touch ``data``."""
    if n_images is None:
        n_images = len(data["ids"])
    rel = {(k, m): relative_pose(data["pose%d" % k], data["pose%d" % m]) for m in range(n_images) for k in range(m)}
    return {km: compute_gt_matches_of_image_pair(data["keypoints%d" % km[0]], data["keypoints%d" % km[1]],
                                                 data["intr%d" % km[0]], data["intr%d" % km[1]], T_km,
                                                 data["depth%d" % km[0]], data["depth%d" % km[1]],
                                                 max_matched_reproj_err, min_unmatched_reproj_err)
            for km, T_km in rel.items()}




def gt_matches_tuple(data, max_matched_reproj_err, min_unmatched_reproj_err, n_images=None):
    """The targets of EVERY pair of a device-resident tuple in one library call (``e2emv_gt_matches_tuple``): returns
    ``(indices [P,B,2,N+1] int64, weights [P,B,2,N+1] f32)``, pair q = (i, j) in the order ``for j in range(T): for i in range(j)``;
    slice q is, bit for bit, what ``gt_matches_for_tuple`` returns under ``(i, j)`` - the relative poses are formed on the device as
    ``relative_pose`` forms them.  A fixed number of launches whatever the tuple and batch size, no host synchronisation.  Does not
    touch ``data``.  ``ValueError`` before any device call: a tuple size outside 2..8, a missing ``keypoints{t}`` / ``intr{t}`` /
    ``pose{t}`` / ``depth{t}``, images with different keypoint counts or depth-map sizes, intrinsics or poses that are not [B,4,4]."""
    T = len(data["ids"]) if n_images is None else int(n_images)
    if T < 2 or T > _lib.MAX_TUPLE:
        raise ValueError("gt_matches_tuple takes tuples of 2..{} images, not {}".format(_lib.MAX_TUPLE, T))
    missing = [k + str(t) for t in range(T) for k in ("keypoints", "intr", "pose", "depth") if k + str(t) not in data]
    if missing:
        raise ValueError("gt_matches_tuple: missing {}".format(", ".join(missing)))
    shapes = {tuple(data["keypoints" + str(t)].shape) for t in range(T)}
    if len(shapes) != 1 or len(next(iter(shapes))) != 3 or next(iter(shapes))[2] != 2 or 0 in next(iter(shapes)):
        raise ValueError("gt_matches_tuple needs keypoints [B,N,2] with the same N in every image, got {}".format(sorted(shapes)))
    B, N = data["keypoints0"].shape[:2]
    for t in range(T):
        for k in ("intr", "pose"):
            if tuple(data[k + str(t)].shape) != (B, 4, 4):
                raise ValueError("gt_matches_tuple: {}{} must be [B,4,4] (MatchingDataset layout), got {}".format(k, t, tuple(data[k + str(t)].shape)))
    dshapes = {tuple(data["depth" + str(t)].shape) for t in range(T)}
    dshape = next(iter(dshapes))
    if len(dshapes) != 1 or len(dshape) < 3 or dshape[0] != B or B * dshape[-2] * dshape[-1] != data["depth0"].numel() or 0 in dshape:
        raise ValueError("gt_matches_tuple needs depth maps [B,H,W] of one size, got {}".format(sorted(dshapes)))
    H, W = dshape[-2:]
    dev = _dev_of(data["keypoints0"], data["depth0"])
    ctx = _lib.context(dev)
    P = T * (T - 1) // 2
    keep, args = [], []
    for k in ("keypoints", "intr", "pose", "depth"):
        tensors = [_prep(data[k + str(t)], dev) for t in range(T)]
        pa, arr = _lib.ptr_array(tensors)
        keep += [tensors, arr]
        args.append(pa)
    idx = torch.empty((P, B, 2, N + 1), dtype=torch.int64, device=dev)
    w = torch.empty((P, B, 2, N + 1), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        ctx.call("e2emv_gt_matches_tuple", B, T, N, args[0], args[1], args[2], args[3], H, W, float(max_matched_reproj_err),
                 float(min_unmatched_reproj_err), _lib.ptr(idx), _lib.ptr(w), _lib.stream_ptr(dev))
    return idx, w


def _match_loss_tuple_call(ctx, dev, scores, idx, w, pair_loss=None):
    """One ``e2emv_match_loss_tuple`` on prepared inputs (``scores``: P contiguous fp32 [B,N+1,N+1]; ``idx`` / ``w`` [P,B,2,N+1]) -> the
    0-dim loss; ``pair_loss`` (fp32 [P], optional) receives the loss of every pair."""
    P, B, _, ft = idx.shape
    loss = torch.empty((), dtype=torch.float32, device=dev)
    ps, keep = _lib.ptr_array(scores)
    with torch.cuda.device(dev):
        ctx.call("e2emv_match_loss_tuple", P, B, ft - 1, ps, _lib.ptr(idx), _lib.ptr(w), _lib.ptr(loss), _lib.ptr(pair_loss),
                 _lib.stream_ptr(dev))
    return loss


class _MatchLossTuple(torch.autograd.Function):
    """loss = sum over the pairs of ``helpers.compute_match_loss`` as a function of the P score tensors: ``e2emv_match_loss_tuple``
    forward, ONE ``e2emv_match_loss_tuple_backward`` that writes every element of d loss / d scores of every pair that requires grad
    (``None`` and a NULL entry for the others); the incoming gradient stays on the device.  The targets carry no gradient."""

    @staticmethod
    def forward(fctx, idx, w, ctx, dev, *scores):
        lp = [_prep(s, dev) for s in scores]
        loss = _match_loss_tuple_call(ctx, dev, lp, idx, w)
        fctx.misc = (ctx, dev, [(s.shape, s.dtype, s.device) for s in scores])
        fctx.save_for_backward(idx, w)
        return loss

    @staticmethod
    def backward(fctx, g):
        idx, w = fctx.saved_tensors
        ctx, dev, meta = fctx.misc
        P, B, _, ft = idx.shape
        g = _prep(g, dev)
        grads = [torch.empty((B, ft, ft), dtype=torch.float32, device=dev) if fctx.needs_input_grad[4 + q] else None for q in range(P)]
        pg, keep = _lib.ptr_array(grads)
        with torch.cuda.device(dev):
            ctx.call("e2emv_match_loss_tuple_backward", P, B, ft - 1, _lib.ptr(idx), _lib.ptr(w), _lib.ptr(g), pg, _lib.stream_ptr(dev))
        return (None, None, None, None) + tuple(None if gq is None else gq.reshape(shape).to(sdev, dtype)
                                                for gq, (shape, dtype, sdev) in zip(grads, meta))


def match_loss_tuple(result, indices, weights):
    """The match term of ``helpers.run_matcher`` (helpers.py:250-253) for ALL pairs of the tuple: the sum over the pairs, in fp32 in
    pair order, of ``compute_match_loss(result["scores_{i}_{j}"], ...)`` on the targets ``indices`` / ``weights`` [P,B,2,N+1] of
    ``gt_matches_tuple`` - a 0-dim fp32 device tensor, bit for bit that sum.  One library call (``e2emv_match_loss_tuple``); when
    gradients are enabled and a score requires grad the result carries the graph back to the scores, and its backward is one more
    call (``e2emv_match_loss_tuple_backward``) for all pairs.  No host synchronisation.  ``ValueError`` before any device call:
    targets that are not int64 / fp32 [P,B,2,N+1] with P = T(T-1)/2 for a T in 2..8, a missing ``scores_{i}_{j}``, scores whose
    shapes differ (images with different keypoint counts) or are not [B,N+1,N+1]."""
    if indices.dim() != 4 or indices.shape[2] != 2 or indices.dtype != torch.int64 or 0 in indices.shape:
        raise ValueError("match_loss_tuple: indices must be int64 [P,B,2,N+1], got {} {}".format(indices.dtype, tuple(indices.shape)))
    if weights.shape != indices.shape or weights.dtype != torch.float32:
        raise ValueError("match_loss_tuple: weights must be float32 {}, got {} {}".format(tuple(indices.shape), weights.dtype, tuple(weights.shape)))
    P, B, _, ft = indices.shape
    T = next((t for t in range(2, _lib.MAX_TUPLE + 1) if t * (t - 1) // 2 == P), None)
    if T is None or ft < 2:
        raise ValueError("match_loss_tuple: targets [P,B,2,N+1] = {} belong to no tuple of 2..{} images with keypoints".format(
            tuple(indices.shape), _lib.MAX_TUPLE))
    names = ["scores_{}_{}".format(i, j) for j in range(T) for i in range(j)]
    missing = [n for n in names if n not in result]
    if missing:
        raise ValueError("match_loss_tuple: missing {}".format(", ".join(missing)))
    scores = [result[n] for n in names]
    shapes = {tuple(s.shape) for s in scores}
    if len(shapes) != 1 or any(len(s) != 3 or s[1] != s[2] for s in shapes):
        raise ValueError("match_loss_tuple needs the same number of keypoints in every image, got scores {}".format(sorted(shapes)))
    if next(iter(shapes)) != (B, ft, ft):
        raise ValueError("match_loss_tuple: scores must be [B,N+1,N+1] = {}, got {}".format((B, ft, ft), next(iter(shapes))))
    dev = _dev_of(*scores)
    ctx = _lib.context(dev)
    idx, w = indices.to(dev).contiguous(), weights.to(dev).contiguous()
    if torch.is_grad_enabled() and any(s.requires_grad for s in scores):
        return _MatchLossTuple.apply(idx, w, ctx, dev, *scores)
    return _match_loss_tuple_call(ctx, dev, [_prep(s, dev) for s in scores], idx, w)


def compute_match_loss(log_p, gt_indices_0_1, gt_weights_0_1):
    """``helpers.compute_match_loss``: scalar tensor (on the device).  On scores that require grad (gradients enabled) the value
    carries the graph: the tuple path with one pair, whose value is the same number (``0.0f + x == x``)."""
    dev = _dev_of(log_p)
    ctx = _lib.context(dev)
    idx = gt_indices_0_1.to(dev, torch.int64).contiguous()
    w = _prep(gt_weights_0_1, dev)
    if torch.is_grad_enabled() and log_p.requires_grad:
        return _MatchLossTuple.apply(idx.unsqueeze(0), w.unsqueeze(0), ctx, dev, log_p)
    lp = _prep(log_p, dev)
    B, ft = lp.shape[:2]
    loss = torch.empty((1,), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        ctx.call("e2emv_match_loss", B, ft - 1, _lib.ptr(lp), _lib.ptr(idx), _lib.ptr(w), _lib.ptr(loss), _lib.stream_ptr(dev))
    return loss[0]
