"""Timing of the multi-view pose back-end on a batch of tuples: the CSV path (``solve_tuple_poses``, one tuple per call, looped
over the batch elements) next to the in-memory path (``solve_tuple_poses_batch``, the whole batch per call) on the same matcher
result.  Default shape: 8 tuples of 5 images at 1024 keypoints (configs[3] of BASELINE.json), identity-like matcher weights as
in tests/test_gpu_multi_view_flow.py.  One warm-up call of each path, then --reps timed calls of each, alternating; every timed
window ends with a device synchronise.  Prints one JSON line: median / min / max of both paths in milliseconds, the per-stage
split of the batched path (medians of a separate set of calls that synchronise after every stage) and the largest difference
between the two paths' extrinsics.  ``--init`` selects where the batched path runs its initialisation stage: ``host`` (the loop
over ``e2emv_mv_init``), ``device`` (``e2emv_mv_tuple_init``, one launch) or ``both`` (default): both batched forms are then
timed inside the same repetition loop, alternating, and the line also carries the device form's figures and the largest
difference between the two forms' extrinsics.  ``--rel-pose-method`` selects the relative poses of both paths: ``w8pt_ba``
(default), ``ransac`` or ``ransac_ba``.  ``--tracks``: the batched path bundle-adjusts the merged tracks
(``solve_tuple_poses_batch(..., tracks=True)``; the CSV path has no tracks and stays as it is, so the difference between the two
paths' extrinsics is then the effect of the tracks); the line also carries the track counts and the time of the label launch
and of labels + problem build + copy-out on their own (each synchronised), the share of the last stage the new kernels take.
``--repair-rounds R`` (with ``--tracks``): the labels come from ``e2emv_mv_tracks_repair`` with up to R rounds (0, the default, is
``e2emv_mv_tracks``).  ``--wrong F``: the identity-like matcher's matches are clean, so a repair has nothing to
do on them; F > 0 replaces every matched keypoint with probability F by a uniform random target of confidence U(0, 0.5) (the
``planted_scene`` recipe of tests/test_gpu_mv_tracks.py, ``default_rng(1000)``) before anything is timed, in both paths.
``--loss huber|cauchy --loss-scale S``: the batched path's last stage runs with that robust loss at the relative scale S
(``solve_tuple_poses_batch(..., loss=, loss_scale=)``; the CSV path has no loss, so the difference between the two paths'
extrinsics is then the effect of the loss).  The last stage's median / min / max is in ``build_and_bundle_adjust_ms`` per form.
``--pair-loss huber|cauchy --pair-loss-scale S``: the batched path's PAIRWISE stage, the two-view bundle adjustment of ``w8pt_ba`` /
``ransac_ba``, runs with that robust loss (``solve_tuple_poses_batch(..., pair_loss=, pair_loss_scale=)``; not with ``ransac``, which
has no such stage).  ``--wrong`` may be given without ``--tracks`` as well: wrong matches are what the losses are for.  The ``relative_poses`` stage's median / min / max is in
``relative_poses_ms`` per form, and ``max_pose_error_deg`` per form is the largest rotation / translation angle error of any image
pair of the batch against the ground truth.

    python tools/bench_mv_backend.py [--batch 8] [--tuple-size 5] [--kpts 1024] [--reps 7] [--init host|device|both]
                                     [--rel-pose-method w8pt_ba|ransac|ransac_ba] [--tracks [--repair-rounds 0] [--wrong 0.0]]
                                     [--loss huber|cauchy --loss-scale 0.00166667]
                                     [--pair-loss huber|cauchy --pair-loss-scale 0.00166667 [--wrong 0.0]]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from e2e_multi_view_matching_amd import MultiViewMatcher, multi_view  # noqa: E402
from e2e_multi_view_matching_amd.synthetic import identity_like_state, make_tuples  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--tuple-size", type=int, default=5)
    ap.add_argument("--kpts", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--init", choices=("host", "device", "both"), default="both")
    ap.add_argument("--rel-pose-method", choices=("w8pt_ba", "ransac", "ransac_ba"), default="w8pt_ba")
    ap.add_argument("--tracks", action="store_true")
    ap.add_argument("--repair-rounds", type=int, default=0)
    ap.add_argument("--wrong", type=float, default=0.0)
    ap.add_argument("--loss", choices=("huber", "cauchy"), default=None)
    ap.add_argument("--loss-scale", type=float, default=None)
    ap.add_argument("--pair-loss", choices=("huber", "cauchy"), default=None)
    ap.add_argument("--pair-loss-scale", type=float, default=None)
    args = ap.parse_args()
    if (args.loss is None) != (args.loss_scale is None):
        ap.error("--loss and --loss-scale go together")
    if (args.pair_loss is None) != (args.pair_loss_scale is None):
        ap.error("--pair-loss and --pair-loss-scale go together")
    if args.pair_loss and args.rel_pose_method == "ransac":
        ap.error("--pair-loss needs --rel-pose-method w8pt_ba or ransac_ba: ransac has no two-view bundle adjustment")
    loss_kw = dict(loss=args.loss, loss_scale=args.loss_scale) if args.loss else {}  # without a loss: the call as it always was
    if args.pair_loss:
        loss_kw.update(pair_loss=args.pair_loss, pair_loss_scale=args.pair_loss_scale)
    if args.repair_rounds and not args.tracks:
        ap.error("--repair-rounds needs --tracks")
    B, T, method = args.batch, args.tuple_size, args.rel_pose_method
    gpu = torch.device("cuda", 0)
    cfg = {"GNN_layers": ["self", "cross"] * 2, "sinkhorn_iterations": 50, "multi_frame_matching": True, "tuple_size": T}
    model = identity_like_state(MultiViewMatcher(cfg).eval()).to(gpu)
    data = make_tuples(batch=B, tuple_size=T, n_kpts=args.kpts, seed=20, noise_px=0.5, max_angle=0.25, transl_sigma=0.4)
    dev = {k: (v.to(gpu) if torch.is_tensor(v) else v) for k, v in data.items()}
    for m in range(T):
        dev[f"intr{m}"] = data[f"intr{m}"]
    with torch.no_grad():
        result = model(dev)
    if args.wrong:
        rng = np.random.default_rng(1000)
        result = {k: v.clone() for k, v in result.items()}
        for j in range(T):
            for i in range(j):
                m, c = result[f"matches{i}_{i}_{j}"], result[f"conf_scores_{i}_{j}"]
                hit = (m >= 0) & torch.from_numpy(rng.uniform(size=tuple(m.shape)) < args.wrong).to(gpu)
                m[hit] = torch.from_numpy(rng.integers(0, args.kpts, tuple(m.shape))).to(gpu)[hit]
                c[hit] = torch.from_numpy(rng.uniform(0.0, 0.5, tuple(m.shape))).to(c)[hit].reshape(-1, *c.shape[2:])
    slices = [({k: (v[b:b + 1] if torch.is_tensor(v) else v) for k, v in dev.items()}, {k: v[b:b + 1] for k, v in result.items()}) for b in range(B)]

    with tempfile.TemporaryDirectory() as tmp:
        def csv_path():
            return np.stack([multi_view.solve_tuple_poses(T, d, r, os.path.join(tmp, str(b)), rel_pose_method=method) for b, (d, r) in enumerate(slices)])

        forms = ("host", "device") if args.init == "both" else (args.init,)

        def batched(init, timings=None):
            return multi_view.solve_tuple_poses_batch(T, dev, result, timings=timings, init=init, rel_pose_method=method, tracks=args.tracks,
                                                      repair_rounds=args.repair_rounds, **loss_kw)

        def timed(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3, out

        e_csv = csv_path()  # warm-up (workspace growth, lazy module loads)
        e_batch = {f: batched(f) for f in forms}
        t_csv, t_batch = [], {f: [] for f in forms}
        for _ in range(args.reps):
            t_csv.append(timed(csv_path)[0])
            for f in forms:
                t_batch[f].append(timed(lambda: batched(f))[0])
        stages = {f: {} for f in forms}
        for _ in range(args.reps):
            for f in forms:
                tm = {}
                batched(f, tm)
                for k, v in tm.items():
                    stages[f].setdefault(k, []).append(v * 1e3)
        if args.tracks:
            intr, kdim, nb = multi_view._tuple_intrinsics(T, dev, gpu, B)
            R = args.repair_rounds
            t_label = [timed(lambda: multi_view.match_tracks(T, dev, result, repair_rounds=R))[0] for _ in range(args.reps + 1)][1:]
            t_build = [timed(lambda: multi_view._tuple_problems_tracks(T, dev, result, 0., intr, kdim, nb, e_batch[forms[0]], repair_rounds=R))[0]
                       for _ in range(args.reps + 1)][1:]
            track_stats = multi_view.match_tracks(T, dev, result, repair_rounds=R)[1].cpu().numpy()
    cam_to_world = np.linalg.inv(np.stack([data[f"pose{m}"].numpy().astype(np.float64) for m in range(T)], 1))  # [B,T,4,4]
    worst = lambda E: float(max(np.nanmax(np.maximum(*multi_view.tuple_pose_errors(E[b], cam_to_world[b]))) for b in range(B)))  # noqa: E731
    stat = lambda ts: {"median": float(np.median(ts)), "min": float(np.min(ts)), "max": float(np.max(ts))}  # noqa: E731
    first = forms[0]  # the form the unsuffixed keys describe: the host form unless --init device
    line = {"batch": B, "tuple_size": T, "n_kpts": args.kpts, "reps": args.reps, "init": args.init, "rel_pose_method": method, "csv_path_ms": stat(t_csv),
            "tracks": args.tracks, "repair_rounds": args.repair_rounds, "wrong": args.wrong, "batched_path_ms": stat(t_batch[first]), "batched_stage_ms": {k: float(np.median(v)) for k, v in stages[first].items()},
            "max_abs_extrinsics_difference": float(np.abs(e_csv - e_batch[first]).max()),
            "loss": args.loss, "loss_scale": args.loss_scale, "pair_loss": args.pair_loss, "pair_loss_scale": args.pair_loss_scale,
            "relative_poses_ms": {f: stat(stages[f]["relative_poses"]) for f in forms},
            "max_pose_error_deg": dict({f: worst(e_batch[f]) for f in forms}, csv=worst(e_csv)),
            "build_and_bundle_adjust_ms": {f: stat(stages[f]["build_and_bundle_adjust"]) for f in forms}}
    if args.init == "both":
        line["batched_path_device_init_ms"] = stat(t_batch["device"])
        line["batched_stage_device_init_ms"] = {k: float(np.median(v)) for k, v in stages["device"].items()}
        line["initialisation_stage_ms"] = {f: stat(stages[f]["initialisation"]) for f in forms}
        line["max_abs_extrinsics_difference_device_vs_host"] = float(np.abs(e_batch["device"] - e_batch["host"]).max())
    if args.tracks:
        line["track_labels_ms"], line["track_labels_build_copy_out_ms"] = stat(t_label), stat(t_build)
        line["tracks_observations_conflicts_edges"] = track_stats.sum(0).tolist()
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
