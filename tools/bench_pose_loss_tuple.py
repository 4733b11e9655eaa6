"""Forward + backward of the pose term of a training step (helpers.run_matcher with opt.pose_loss, helpers.py:243-260): the per-pair loop
of the existing differentiable functions against ``pose_loss_tuple``, both in this process on the same inputs.

Shapes: 8 tuples of 5 images (10 pairs) at 400 and at 1024 keypoints, ``ba_iterations`` 0 and 10.  Per shape: 3 warm-up steps of each
variant, then --reps repetitions (default 9, at least 7) that ALTERNATE the two variants; a repetition is --inner steps (forward,
backward, gradients dropped) closed by one device synchronise, its time divided by --inner; the figure is the median over the
repetitions, the spread their minimum and maximum.  Also counted, in one untimed step each: the library calls of a step (a recording
wrapper around ``Context.call``) and the host synchronisations the step forces (``torch.cuda.set_sync_debug_mode("warn")``).

    python tools/bench_pose_loss_tuple.py [--reps 9] [--inner 5] [--out profiles/pose_loss_tuple.json]
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
from e2e_multi_view_matching_amd.synthetic import make_tuples  # noqa: E402


def inputs(B, T, N, dev, seed=0):
    d = make_tuples(batch=B, tuple_size=T, n_kpts=N, seed=seed)
    g = torch.Generator().manual_seed(seed)
    pairs = [(i, j) for j in range(T) for i in range(j)]
    data = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in d.items()}
    for t in range(T):  # make_tuples' poses map world -> camera; data["pose"] of the reference maps camera -> world
        data[f"pose{t}"] = torch.linalg.inv(d[f"pose{t}"].double()).float().to(dev)
    result = {}
    for i, j in pairs:
        result[f"matches{i}_{i}_{j}"] = d[f"gt_matches{i}_{i}_{j}"].to(dev)
        result[f"conf_scores_{i}_{j}"] = (torch.rand(B, N, 1, generator=g) * 0.8 + 0.2).to(dev).requires_grad_(True)
    return data, result, pairs


def pair_loop_step(data, result, pairs, ba):
    rot_loss, transl_loss = 0.0, 0.0
    for i, j in pairs:
        tgt = E.relative_pose(data[f"pose{i}"], data[f"pose{j}"])
        if ba == 0:
            T, _ = E.run_weighted_8_point(data, result, i, j, choose_closest=True, target_T_021=tgt)
        else:
            k0, k1, K0, K1, conf = E.get_kpts(data, result, i, j)
            Tw, info = E.estimate_relative_pose_w8pt(k0, k1, K0, K1, conf, choose_closest=True, T_021=tgt)
            cm = E.mask_confidence(conf.squeeze(-1), info["pos_depth_mask"])
            refined, vb = E.run_bundle_adjust_2_view(info["kpts0_norm"], info["kpts1_norm"], cm, Tw, ba)
            T = Tw.clone()
            T[vb] = refined
        rot_loss = rot_loss + E.compute_rotation_error(T, tgt)
        transl_loss = transl_loss + E.compute_translation_error_as_angle(T, tgt)
    (rot_loss + transl_loss).backward()
    return rot_loss.detach(), transl_loss.detach()


def tuple_step(data, result, pairs, ba):
    out = E.pose_loss_tuple(data, result, ba_iterations=ba)
    (out["rot_loss"] + out["transl_loss"]).backward()
    return out["rot_loss"].detach(), out["transl_loss"].detach()


def drop_grads(result):
    for v in result.values():
        if v.requires_grad:
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_loss_tuple.json"))
    args = ap.parse_args()
    if args.reps < 7:
        ap.error("--reps must be at least 7")
    dev = torch.device("cuda", 0)
    ctx = _lib.context(dev)
    variants = {"pair_loop": pair_loop_step, "tuple": tuple_step}
    rows = []
    for N in (400, 1024):
        for ba in (0, 10):
            data, result, pairs = inputs(8, 5, N, dev)
            a = (data, result, pairs, ba)
            row = {"tuples": 8, "tuple_size": 5, "pairs": len(pairs), "n_kpts": N, "ba_iterations": ba, "reps": args.reps, "inner": args.inner}
            losses = {}
            for name, step in variants.items():
                for _ in range(3):
                    losses[name] = [float(x) for x in step(*a)]
                    drop_grads(result)
                torch.cuda.synchronize()
                row[name + "_library_calls"], row[name + "_host_syncs"] = counted(step, ctx, a)
            row["losses_pair_loop"], row["losses_tuple"] = losses["pair_loop"], losses["tuple"]
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
        json.dump({"device": torch.cuda.get_device_name(dev), "method": __doc__.split("\n\n")[1], "rows": rows}, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
