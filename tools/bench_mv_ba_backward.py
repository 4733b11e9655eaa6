"""Timing of the multi-view bundle adjustment and of its backward pass (``e2emv_mv_bundle_adjust_batch`` /
``e2emv_mv_bundle_adjust_batch_backward``) on the problems of B tuples of 5 images at 1024 keypoints: synthetic tuples through the
identity-like matcher as in tools/bench_mv_backend.py, matches collected and the problems built on the device
(``e2emv_mv_collect``, ``e2emv_mv_tuple_problem``: one point per match, two observations each, camera 0 fixed), the start the true
poses perturbed by 0.02 rad / 0.02 units.  Both entries take HOST arrays and are synchronous, so a timed call holds the upload of
the problem, one launch (the backward's replays the loop with its tape and reverses it) and the copy back.  One warm-up call of
each, then --reps timed calls of each, alternating.  Prints one JSON line per batch size and writes them to --out.

--tracks: the track route instead, on the same tuples and start: ``e2emv_mv_tuple_ba_tracks`` against
``e2emv_mv_tuple_ba_tracks_backward`` on the SAME labels (``match_tracks(..., repair_rounds=--repair-rounds)``, computed once, outside
the timed calls).  Both entries build the problems on the device from the labels, so a timed call holds the upload of records and start
cameras, the build launch, the solver launch (the backward's with its tape and the reverse walk, then the weights kernel) and the copy
back (the forward's: extrinsics; the backward's: nothing, the gradients stay on the device).

    python tools/bench_mv_ba_backward.py [--batches 8 32] [--tuple-size 5] [--kpts 1024] [--iterations 50] [--reps 5] [--out FILE]
                                         [--tracks [--repair-rounds R]]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from e2e_multi_view_matching_amd import MultiViewMatcher, multi_view  # noqa: E402
from e2e_multi_view_matching_amd.synthetic import identity_like_state, make_tuples  # noqa: E402


def inputs_of(B, T, kpts, gpu):
    cfg = {"GNN_layers": ["self", "cross"] * 2, "sinkhorn_iterations": 50, "multi_frame_matching": True, "tuple_size": T}
    model = identity_like_state(MultiViewMatcher(cfg).eval()).to(gpu)
    data = make_tuples(batch=B, tuple_size=T, n_kpts=kpts, seed=20, noise_px=0.5, max_angle=0.25, transl_sigma=0.4)
    dev = {k: (v.to(gpu) if torch.is_tensor(v) else v) for k, v in data.items()}
    for m in range(T):
        dev[f"intr{m}"] = data[f"intr{m}"]
    with torch.no_grad():
        result = model(dev)
    rng = np.random.default_rng(7)
    start = np.zeros((B, T, 4, 4))
    for b in range(B):
        E0 = data["pose0"][b].double().numpy()
        for m in range(T):
            E = data[f"pose{m}"][b].double().numpy() @ np.linalg.inv(E0)  # world -> camera, camera 0 the gauge
            if m:
                w = rng.normal(0, 0.02, 3)
                K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
                E[:3, :3] = (np.eye(3) + K + 0.5 * K @ K) @ E[:3, :3]
                E[:3, :3] = np.linalg.svd(E[:3, :3])[0] @ np.linalg.svd(E[:3, :3])[2]
                E[:3, 3] += rng.normal(0, 0.02, 3)
            start[b, m] = E
    return dev, result, start


def problems_of(B, T, kpts, gpu):
    dev, result, start = inputs_of(B, T, kpts, gpu)
    collected = multi_view._collect_matches_batch(T, dev, result, 0.)
    counts = collected[3].cpu().numpy()
    intr, kdim, nb = multi_view._tuple_intrinsics(T, dev, gpu, B)
    return multi_view._tuple_problems(T, collected, counts, intr, kdim, nb, start)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def stat(t):
    return dict(median=float(np.median(t)), min=float(np.min(t)), max=float(np.max(t)))


def tracks_line(B, args, gpu):
    from e2e_multi_view_matching_amd import _lib
    T = args.tuple_size
    dev, result, start = inputs_of(B, T, args.kpts, gpu)
    inp, label, stats = multi_view._tracks_labels(T, dev, result, 0., args.repair_rounds)
    intr, kdim, nb = multi_view._tuple_intrinsics(T, dev, gpu, B)
    out, summary = np.zeros_like(start), np.zeros((B, 4))
    g = np.ascontiguousarray(np.random.default_rng(3).normal(size=(B, T, 4, 4)))
    gouts = [None if c is None else torch.empty_like(c) for c in inp["conf"]]
    pg, owner = _lib.ptr_array(gouts)
    call = lambda name, *tail: multi_view._tracks_entry_call(name, T, inp, label, stats, 0., intr, kdim, nb, start, args.iterations, *tail)  # noqa: E731
    fwd = lambda: call("e2emv_mv_tuple_ba_tracks", multi_view._p(out), multi_view._p(summary))  # noqa: E731
    bwd = lambda: call("e2emv_mv_tuple_ba_tracks_backward", multi_view._p(g), pg)  # noqa: E731
    fwd(), bwd()
    tf, tb = [], []
    for _ in range(args.reps):
        tf.append(timed(fwd)[0])
        tb.append(timed(bwd)[0])
    del owner
    terms = ["max_iterations", "gradient_tolerance", "parameter_tolerance", "function_tolerance", "invalid_steps", "radius"]
    return dict(tool="bench_mv_ba_backward", route="tracks", repair_rounds=args.repair_rounds, batch=B, tuple_size=T, kpts=args.kpts,
                max_iterations=args.iterations, reps=args.reps, tracks_per_tuple=stats[:, 0].tolist(), observations_per_tuple=stats[:, 1].tolist(),
                iterations=[int(v) for v in summary[:, 2]], terminations=sorted(set(terms[int(v)] for v in summary[:, 3])), forward_ms=stat(tf),
                backward_ms=stat(tb), backward_over_forward=float(np.median(tb) / np.median(tf)),
                finite=bool(all(bool(go.isfinite().all()) for go in gouts)), max_abs_g_conf=float(max(float(go.abs().max()) for go in gouts)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[8, 32])
    ap.add_argument("--tuple-size", type=int, default=5)
    ap.add_argument("--kpts", type=int, default=1024)
    ap.add_argument("--iterations", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--tracks", action="store_true")
    ap.add_argument("--repair-rounds", type=int, default=0)
    args = ap.parse_args()
    gpu = torch.device("cuda", 0)
    lines = []
    for B in args.batches:
        if args.tracks:
            lines.append(tracks_line(B, args, gpu))
            print(json.dumps(lines[-1]), flush=True)
            continue
        problems = problems_of(B, args.tuple_size, args.kpts, gpu)
        rng = np.random.default_rng(3)
        grads = [(rng.normal(size=(args.tuple_size, 6)), None) for _ in problems]
        fwd = lambda: multi_view.bundle_adjust_batch(problems, args.iterations)  # noqa: E731
        bwd = lambda: multi_view.bundle_adjust_batch_backward(problems, grads, args.iterations)  # noqa: E731
        solved, back = fwd(), bwd()
        tf, tb = [], []
        for _ in range(args.reps):
            tf.append(timed(fwd)[0])
            tb.append(timed(bwd)[0])
        line = dict(tool="bench_mv_ba_backward", batch=B, tuple_size=args.tuple_size, kpts=args.kpts, max_iterations=args.iterations, reps=args.reps,
                    points_per_tuple=[len(p[8]) for p in problems], iterations=[s[2]["iterations"] for s in solved],
                    terminations=sorted(set(s[2]["termination"] for s in solved)), forward_ms=stat(tf), backward_ms=stat(tb),
                    backward_over_forward=float(np.median(tb) / np.median(tf)),
                    finite=bool(all(np.isfinite(g).all() for out in back for g in out)), max_abs_g_obs_w=float(max(np.abs(out[0]).max() for out in back)))
        print(json.dumps(line), flush=True)
        lines.append(line)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(lines, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
