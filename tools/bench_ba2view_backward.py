"""Timing of the two-view bundle adjustment and of its backward pass (``e2emv_ba_2view`` / ``e2emv_ba_2view_backward``; with ``--loss huber``
or ``cauchy``: ``e2emv_ba_2view_loss`` / ``e2emv_ba_2view_loss_backward`` at the relative scale ``--loss-scale``) on synthetic pairs:
points at depth 3..8 in front of both cameras, a pose perturbed by 0.06 rad / 0.1 as the start, 0.5 pixel (f = 600) of keypoint noise,
confidences in (0.1, 1] with every seventh at 0.  Default shapes: 32 pairs x 1024 matches and 80 pairs x 2048 matches, 10 iterations.  Per
shape one warm-up call of each entry (the workspace grows there), then --reps timed calls of each, alternating, each between two events
on the stream.  Prints one JSON line: median / min / max in milliseconds per shape and entry, and the fraction of pairs whose result
moved (a pair that stayed at its start has k* = 0 and no step to reverse).

    python tools/bench_ba2view_backward.py [--shapes 32x1024,80x2048] [--iterations 10] [--reps 9] [--loss none|huber|cauchy] [--loss-scale 0.0016667]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from e2e_multi_view_matching_amd import _lib  # noqa: E402


def rodrigues(w):
    th = np.linalg.norm(w)
    k = w / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


def make_pairs(B, N, seed):
    rng = np.random.default_rng(seed)
    k0, k1, Ti = np.zeros((B, N, 2)), np.zeros((B, N, 2)), np.zeros((B, 4, 4))
    unit = lambda: (lambda v: v / np.linalg.norm(v))(rng.normal(size=3))  # noqa: E731
    for b in range(B):
        R = rodrigues(unit() * rng.uniform(0.1, 0.25))
        t = np.array([1.0, 0.0, 0.0]) + rng.uniform(-0.2, 0.2, 3)
        z = rng.uniform(3.0, 8.0, N)
        X = np.stack([z * rng.uniform(-0.35, 0.35, N), z * rng.uniform(-0.35, 0.35, N), z], -1)
        Y = X @ R.T + t
        k0[b] = X[:, :2] / X[:, 2:] + rng.normal(size=(N, 2)) * 0.5 / 600.0
        k1[b] = Y[:, :2] / Y[:, 2:] + rng.normal(size=(N, 2)) * 0.5 / 600.0
        Ti[b] = np.eye(4)
        Ti[b, :3, :3] = rodrigues(unit() * 0.06) @ R
        Ti[b, :3, 3] = t + 0.1 * unit()
    conf = 1.1 - rng.uniform(0.1, 1.0, (B, N))
    conf[:, ::7] = 0.0
    f = lambda a: torch.from_numpy(np.ascontiguousarray(a).astype(np.float32))  # noqa: E731
    return f(k0), f(k1), f(conf), f(Ti)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="32x1024,80x2048")
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--loss", choices=["none", "huber", "cauchy"], default="none")
    ap.add_argument("--loss-scale", type=float, default=1.0 / 600.0, help="relative scale of the loss: one pixel at f = 600")
    args = ap.parse_args()
    code = {"none": 0, "huber": 1, "cauchy": 2}[args.loss]
    dev = torch.device("cuda", 0)
    ctx = _lib.context(dev)
    out = {"iterations": args.iterations, "reps": args.reps, "loss": args.loss, "loss_scale": args.loss_scale if code else None, "shapes": {}}
    for shape in args.shapes.split(","):
        B, N = (int(x) for x in shape.split("x"))
        k0, k1, conf, Ti = (t.to(dev) for t in make_pairs(B, N, seed=B * 10007 + N))
        gT = torch.zeros(B, 4, 4, device=dev)
        gT[:, :3] = torch.randn(B, 3, 4, generator=torch.Generator().manual_seed(1)).to(dev)
        To = torch.empty(B, 4, 4, device=dev)
        valid = torch.empty(B, dtype=torch.uint8, device=dev)
        gconf, gTi = torch.empty(B, N, device=dev), torch.empty(B, 4, 4, device=dev)
        stream = _lib.stream_ptr(dev)

        def forward():
            head = (B, N, _lib.ptr(k0), _lib.ptr(k1), _lib.ptr(conf), _lib.ptr(Ti), args.iterations, _lib.ptr(To), _lib.ptr(valid))
            if code:
                ctx.call("e2emv_ba_2view_loss", *head, code, args.loss_scale, None, stream)
            else:
                ctx.call("e2emv_ba_2view", *head, stream)

        def backward():
            head = (B, N, _lib.ptr(k0), _lib.ptr(k1), _lib.ptr(conf), _lib.ptr(Ti), args.iterations)
            if code:
                ctx.call("e2emv_ba_2view_loss_backward", *head, code, args.loss_scale, _lib.ptr(gT), _lib.ptr(gconf), _lib.ptr(gTi), stream)
            else:
                ctx.call("e2emv_ba_2view_backward", *head, _lib.ptr(gT), _lib.ptr(gconf), _lib.ptr(gTi), stream)

        times = {"forward": [], "backward": []}
        with torch.cuda.device(dev):
            backward()  # the larger workspace first: no regrow inside a timed call
            forward()
            torch.cuda.synchronize(dev)
            for _ in range(args.reps):
                for name, fn in (("forward", forward), ("backward", backward)):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    fn()
                    e1.record()
                    e1.synchronize()
                    times[name].append(e0.elapsed_time(e1))
        assert bool(valid.bool().all()) and bool(gconf.isfinite().all()) and bool(gTi.isfinite().all())
        moved = float((To - Ti).abs().flatten(1).max(1).values.gt(0).float().mean())
        out["shapes"][shape] = {k: {"median_ms": float(np.median(v)), "min_ms": float(np.min(v)), "max_ms": float(np.max(v))} for k, v in times.items()}
        out["shapes"][shape]["pairs_whose_result_moved"] = moved
        out["shapes"][shape]["gconf_max"] = float(gconf.abs().max())
    print(json.dumps(out))


if __name__ == "__main__":
    main()
