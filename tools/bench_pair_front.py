#!/usr/bin/env python
"""The image stage of pair evaluation (PairMatchingDataset.__getitem__, eval_pairs.py:85-108 of the reference) at the sizes of its
three benchmarks: decoded gray uint8 frames, np.rot90, cv2.resize to img_size, / 255.

Pairs:
  scannet   two frames of 968 x 1296 at img_size 720 -> 537 x 720 each, merged (ScanNet-1500)
  mixed     768 x 1024 upright and 1024 x 683 turned once, at img_size 1600 -> 1200 x 1600 and 1067 x 1600 (MegaDepth / YFCC: two
            sizes, one in-plane turn)
Arms, per pair:
  (a) E.prepare_pair_images: one e2emv_image_front_gray call, one launch
  (b) the float32 numpy restatement (tests/pair_front_restatement.py) on the CPU: what the reference's loader does with cv2 on
      the host (cv2 itself was NOT available where this was measured: no comparison with it, in time or in bytes).  The process
      may use 16 threads; numpy's indexing and elementwise operations run on one
  (c) the same steps as torch ops on the device (torch.rot90, F.interpolate bilinear in float32, / 255): what a user would write
      today without (a); aten's tap positions are not OpenCV's, so (c) is a time, not a reference
(a) and (c) start from the uint8 frames on the device, (b) from the uint8 frames on the host; no arm includes a host-device copy.

Repeats alternate between the arms; minimum, median and maximum of the per-call time of a warmed repeat are reported - quote
the maximum.  (a)'s time on the device alone is the library's event chain around its launch.  Its compulsory bytes - the frames
once, the float32 output once - over that time stand beside the 6.29 TB/s a copy kernel reaches on the MI355X.  The largest
distance of (a) from the float64 restatement is measured on the same frames.  Writes profiles/pair_front.json (--out)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import e2e_multi_view_matching_amd as E  # noqa: E402
from e2e_multi_view_matching_amd import _lib  # noqa: E402
import pair_front_restatement as R  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pair_front.json"))
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--steps", type=int, default=200, help="calls per repeat of the device arms")
ap.add_argument("--cpu-repeats", type=int, default=3, help="repeats of arm (b), one call each")
args = ap.parse_args()

dev = torch.device("cuda:0")
torch.set_num_threads(16)
COPY_TBPS = 6.29
PAIRS = {
    "scannet": dict(frames=[(968, 1296, 0), (968, 1296, 0)], img_size=720, merge=True),
    "mixed": dict(frames=[(768, 1024, 0), (1024, 683, 1)], img_size=1600, merge=False),
}


def per_step_ms(fn, steps, sync):
    if sync:
        torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(steps):
        fn()
    if sync:
        torch.cuda.synchronize()
    return (time.perf_counter() - t) / steps * 1e3


def summary(v):
    return {"min_ms": round(min(v), 4), "median_ms": round(statistics.median(v), 4), "max_ms": round(max(v), 4), "repeats_ms": [round(x, 4) for x in v]}


def device_ms(fn, steps):
    """(a)'s time on the device alone: the library's own event chain around its launches (e2emv_profile), per call."""
    ctx = _lib.context(dev)
    ctx.call("e2emv_profile", 1)
    try:
        _lib.profile_read(ctx, reset=True)
        for _ in range(steps):
            fn()
        slots = _lib.profile_read(ctx, reset=True)
    finally:
        ctx.call("e2emv_profile", 0)
    return sum(v["ms"] for v in slots.values()) / steps, sum(v["launches"] for v in slots.values()) // steps


def torch_ops(frames, rots, sizes):
    out = []
    for f, r, (h, w) in zip(frames, rots, sizes):
        x = torch.rot90(f, r).to(torch.float32)[None, None]
        if tuple(x.shape[-2:]) != (h, w):
            x = F.interpolate(x, size=(h, w), mode="bilinear", align_corners=False)
        out.append(x / 255.0)
    return out


rows = []
for name, pair in PAIRS.items():
    host = [R.make_frame(H, W, 100 + i) for i, (H, W, _) in enumerate(pair["frames"])]
    rots = [r for _, _, r in pair["frames"]]
    img_size = pair["img_size"]
    frames = [torch.from_numpy(f).to(dev) for f in host]
    sizes = [E.pair_out_size(f.shape, r, img_size) for f, r in zip(host, rots)]
    arms = {
        "a_prepare_pair_images": (lambda: E.prepare_pair_images(frames, img_size, rots=rots, merge=pair["merge"]), args.steps, True),
        "c_torch_ops_on_device": (lambda: torch_ops(frames, rots, sizes), max(args.steps // 4, 1), True),
        "b_numpy_restatement_on_cpu": (lambda: [R.pair_front(f, r, img_size, np.float32) for f, r in zip(host, rots)], 1, False),
    }
    got = arms["a_prepare_pair_images"][0]()
    got = [got[i] for i in range(len(host))] if pair["merge"] else [g[0] for g in got]
    want64 = [R.pair_front(f, r, img_size, np.float64) for f, r in zip(host, rots)]
    want32 = [R.pair_front(f, r, img_size, np.float32) for f, r in zip(host, rots)]
    dist64 = max(float(np.abs(g[0].cpu().numpy().astype(np.float64) - w).max()) for g, w in zip(got, want64))
    dist32 = max(float(np.abs(w32.astype(np.float64) - w).max()) for w32, w in zip(want32, want64))
    same_bytes = sum(int((g[0].cpu().numpy() != w32).sum()) for g, w32 in zip(got, want32))
    c_dist = max(float((c[0, 0].cpu().double() - torch.from_numpy(w)).abs().max()) for c, w in zip(torch_ops(frames, rots, sizes), want64))
    del got
    for arm, (fn, steps, sync) in arms.items():  # warm-up: allocator, clocks, code objects
        if arm != "b_numpy_restatement_on_cpu":
            for _ in range(20):
                fn()
    torch.cuda.synchronize()
    times = {k: [] for k in arms}
    for r in range(args.repeats):
        for arm, (fn, steps, sync) in arms.items():  # alternating: every arm sees the same drift of the machine
            if arm == "b_numpy_restatement_on_cpu" and r >= args.cpu_repeats:
                continue
            times[arm].append(per_step_ms(fn, steps, sync))
    res = {k: summary(v) for k, v in times.items()}
    a = res["a_prepare_pair_images"]
    dev_ms = [device_ms(arms["a_prepare_pair_images"][0], args.steps) for _ in range(args.repeats)]
    launches = dev_ms[0][1]
    dev_ms = summary([m for m, _ in dev_ms])
    bytes_compulsory = sum(f.size for f in host) + 4 * sum(h * w for h, w in sizes)
    rows.append({
        "pair": name, "frames": [list(f.shape) for f in host], "rots": rots, "img_size": img_size, "outputs": [list(s) for s in sizes],
        "arms": res,
        "a_max_distance_from_float64_restatement": dist64,
        "float32_restatement_max_distance_from_float64": dist32,
        "a_pixels_that_differ_from_the_float32_restatement": same_bytes,
        "c_max_distance_from_float64_restatement": c_dist,
        "a_compulsory_bytes": bytes_compulsory,
        "a_device_time": dev_ms, "a_launches_per_call": launches,
        "a_compulsory_bytes_over_max_device_time_TBps": round(bytes_compulsory / (dev_ms["max_ms"] * 1e-3) / 1e12, 4),
        "copy_rate_TBps": COPY_TBPS,
        "a_fraction_of_copy_rate": round(bytes_compulsory / (dev_ms["max_ms"] * 1e-3) / 1e12 / COPY_TBPS, 4),
        "c_over_a": round(res["c_torch_ops_on_device"]["max_ms"] / a["max_ms"], 2),
        "b_over_a": round(res["b_numpy_restatement_on_cpu"]["max_ms"] / a["max_ms"], 1),
        "a_beats_c_beyond_the_spread": bool(a["max_ms"] < res["c_torch_ops_on_device"]["min_ms"]),
    })
    print(json.dumps(rows[-1]), flush=True)

out = {
    "tool": "tools/bench_pair_front.py", "device": torch.cuda.get_device_name(0),
    "clock": "host clock around N calls ending in a device synchronise (arm b: around one call); per-call time of a repeat; "
             "a_device_time: HIP events of the library's profile slots around the launches of N calls",
    "cv2": "not available where this was measured: neither the time nor the bytes of cv2.resize were compared; arm b is the numpy "
           "restatement of its arithmetic",
    "repeats": args.repeats, "calls_per_repeat": {"a": args.steps, "c": max(args.steps // 4, 1), "b": 1}, "cpu_repeats": args.cpu_repeats,
    "cpu_threads": torch.get_num_threads(), "rows": rows,
}
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    json.dump(out, fh, indent=1)
    fh.write("\n")
