"""Forward + backward of the match term of a training step (helpers.run_matcher, helpers.py:243-253, after compute_gt_matches at
train.py:411), down to d logZ of every pair: the per-pair loop a training loop had to use against ``gt_matches_tuple`` / ``match_loss_tuple``,
both in this process on the same inputs.

Variant (a), ``pair_loop``: ``gt_matches_for_tuple`` for the targets, then per pair the reference's torch expression of
``helpers.compute_match_loss`` - its ``range(bs*ft)`` row index included, a Python list that torch copies to the device -, summed, ``.backward()``.
Variant (b), ``tuple``: ``gt_matches_tuple``, ``match_loss_tuple``, ``.backward()``.  The scores are plain leaf tensors, so the step ends at
d logZ.  Each variant is timed with its targets rebuilt in every step (as a training step does) and on targets built once.

Shapes: 8 tuples of 5 images (10 pairs) at 400 and at 1024 keypoints, on a scene with depth maps whose targets hold real matches.  Per shape:
3 warm-up steps of each variant, then --reps repetitions (default 9, at least 7) that ALTERNATE the two variants; a repetition is --inner
steps (forward, backward, gradients dropped) closed by one device synchronise, its time divided by --inner; the figure is the median over the
repetitions, the spread their minimum and maximum.  Also counted, in one untimed step each: the library calls of a step (a recording
wrapper around ``Context.call``) and the host synchronisations the step forces (``torch.cuda.set_sync_debug_mode("warn")``); and the backward
call alone (``e2emv_match_loss_tuple_backward``, 20 launches between two device synchronisations) with the store rate it reaches.

    python tools/bench_match_loss_tuple.py [--reps 9] [--inner 5] [--out profiles/match_loss_tuple.json]
"""
import argparse
import json
import os
import sys
import time
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import e2e_multi_view_matching_amd as E  # noqa: E402
from e2e_multi_view_matching_amd import _lib  # noqa: E402

MAX_MATCHED, MIN_UNMATCHED = 5.0, 15.0


def inputs(B, T, N, dev, seed=0):
    """A plane at depth 4 seen by T displaced cameras: keypoints of image t are noisy reprojections of those of image 0 for 70 % of them
    and random pixels for the rest, in random order; 8 % of the depth pixels are holes.  Scores: a log-softmax of noise, leaves."""
    rng = np.random.default_rng(seed)
    H, W, f = 480, 640, 600.0
    K = np.eye(4)
    K[0, 0] = K[1, 1] = f
    K[0, 2], K[1, 2] = W / 2, H / 2
    k0 = np.stack([rng.uniform(120, 520, (B, N)), rng.uniform(100, 380, (B, N))], -1)
    f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a).astype(np.float32)).to(dev)
    data = {"ids": list(range(T))}
    for t in range(T):
        c = rng.normal(0, 0.15, (B, 3)) * (t > 0)
        X = np.concatenate([(np.floor(k0) - K[:2, 2]) / f * 4.0, np.full((B, N, 1), 4.0)], -1) - c[:, None, :]
        k = X[..., :2] / X[..., 2:] * f + K[:2, 2] + rng.normal(0, 1.5, (B, N, 2)) * (t > 0)
        lost = rng.uniform(size=(B, N)) < 0.3
        k[lost] = np.stack([rng.uniform(0, W, int(lost.sum())), rng.uniform(0, H, int(lost.sum()))], -1)
        k = np.clip(k, 0, [W - 1, H - 1])
        k = np.stack([k[b, rng.permutation(N)] for b in range(B)]) if t else k
        depth = np.broadcast_to((4.0 - c[:, 2])[:, None, None], (B, H, W)).copy()
        depth[rng.uniform(size=depth.shape) < 0.08] = 0.0
        pose = np.broadcast_to(np.eye(4), (B, 4, 4)).copy()
        pose[:, :3, 3] = c
        data[f"keypoints{t}"], data[f"intr{t}"], data[f"pose{t}"], data[f"depth{t}"] = f32(k), f32(np.broadcast_to(K, (B, 4, 4))), f32(pose), f32(depth)
    g = torch.Generator().manual_seed(seed)
    pairs = [(i, j) for j in range(T) for i in range(j)]
    result = {f"scores_{i}_{j}": torch.log_softmax(torch.randn(B, N + 1, N + 1, generator=g), -1).to(dev).requires_grad_(True) for i, j in pairs}
    return data, result, pairs


def reference_match_loss(log_p, gt_indices, gt_weights):
    """``oracle.gt_matches.compute_match_loss`` - this project's statement of helpers.compute_match_loss (helpers.py:228-241) - on the
    device, with the row index the reference uses there: ``range(bs*ft)``, a Python list."""
    bs, ft, _ = log_p.shape
    i0, i1 = gt_indices[:, 0].reshape(bs * ft), gt_indices[:, 1].reshape(bs * ft)
    w0, w1 = gt_weights[:, 0].reshape(bs * ft), gt_weights[:, 1].reshape(bs * ft)
    r = range(bs * ft)
    l0 = -log_p.reshape(bs * ft, ft)[r, i0]
    l1 = -log_p.transpose(1, 2).reshape(bs * ft, ft)[r, i1]
    return (torch.dot(l0, w0) + torch.dot(l1, w1)) / bs


def pair_loop_step(data, result, pairs, cached):
    gt = cached["pair_loop"] if cached else E.gt_matches_for_tuple(data, MAX_MATCHED, MIN_UNMATCHED)
    loss = 0.0
    for i, j in pairs:
        loss = loss + reference_match_loss(result[f"scores_{i}_{j}"], *gt[(i, j)])
    loss.backward()
    return loss.detach()


def tuple_step(data, result, pairs, cached):
    idx, w = cached["tuple"] if cached else E.gt_matches_tuple(data, MAX_MATCHED, MIN_UNMATCHED)
    loss = E.match_loss_tuple(result, idx, w)
    loss.backward()
    return loss.detach()


def drop_grads(result):
    for v in result.values():
        v.grad = None


def counted(step, ctx, args):
    """(library calls, host synchronisations) of one step."""
    calls, orig = [], ctx.call
    ctx.call = lambda name, *a: (calls.append(name), orig(name, *a))[1]
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            step(*args)
    finally:
        torch.cuda.set_sync_debug_mode("default")
        del ctx.call
    torch.cuda.synchronize()
    drop_grads(args[1])
    return len(calls), sum("synchroniz" in str(x.message).lower() for x in w)


def backward_alone(ctx, dev, idx, w, n=20):
    """ms per e2emv_match_loss_tuple_backward and the rate of its stores, from n launches between two device synchronisations."""
    P, B, _, ft = idx.shape
    outs = [torch.empty((B, ft, ft), dtype=torch.float32, device=dev) for _ in range(P)]
    pg, keep = _lib.ptr_array(outs)
    g = torch.ones((1,), dtype=torch.float32, device=dev)
    call = lambda: ctx.call("e2emv_match_loss_tuple_backward", P, B, ft - 1, _lib.ptr(idx), _lib.ptr(w), _lib.ptr(g), pg, _lib.stream_ptr(dev))
    for _ in range(3):
        call()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        call()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / n
    return ms, P * B * ft * ft * 4 / (ms * 1e-3) / 1e9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "match_loss_tuple.json"))
    args = ap.parse_args()
    if args.reps < 7:
        ap.error("--reps must be at least 7")
    dev = torch.device("cuda", 0)
    ctx = _lib.context(dev)
    variants = {"pair_loop": pair_loop_step, "tuple": tuple_step}
    rows = []
    for N in (400, 1024):
        data, result, pairs = inputs(8, 5, N, dev)
        cache = {"pair_loop": E.gt_matches_for_tuple(data, MAX_MATCHED, MIN_UNMATCHED), "tuple": E.gt_matches_tuple(data, MAX_MATCHED, MIN_UNMATCHED)}
        n_match = int((cache["tuple"][0][:, :, 0] >= 0).sum())
        bwd_ms, bwd_gbs = backward_alone(ctx, dev, *cache["tuple"])
        for with_targets in (True, False):
            a = (data, result, pairs, None if with_targets else cache)
            row = {"tuples": 8, "tuple_size": 5, "pairs": len(pairs), "n_kpts": N, "targets_in_the_step": with_targets, "matches": n_match,
                   "reps": args.reps, "inner": args.inner, "backward_call_alone_ms": bwd_ms, "backward_call_alone_GB_per_s": bwd_gbs}
            losses = {}
            for name, step in variants.items():
                for _ in range(3):
                    losses[name] = float(step(*a))
                    drop_grads(result)
                torch.cuda.synchronize()
                row[name + "_library_calls"], row[name + "_host_syncs"] = counted(step, ctx, a)
            row["loss_pair_loop"], row["loss_tuple"] = losses["pair_loop"], losses["tuple"]
            ts = {name: [] for name in variants}
            for _ in range(args.reps):
                for name, step in variants.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(args.inner):
                        step(*a)
                        drop_grads(result)
                    torch.cuda.synchronize()
                    ts[name].append((time.perf_counter() - t0) * 1e3 / args.inner)
            for name in variants:
                row[name + "_ms"] = float(np.median(ts[name]))
                row[name + "_ms_min_max"] = [float(min(ts[name])), float(max(ts[name]))]
            row["speedup"] = row["pair_loop_ms"] / row["tuple_ms"]
            print(json.dumps(row), flush=True)
            rows.append(row)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump({"device": torch.cuda.get_device_name(dev), "method": __doc__.split("\n\n")[2], "rows": rows}, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
