#!/usr/bin/env python
"""The image stage of a training step (MatchingDataset.__getitem__, datasets/matching_dataset.py:182-211 of the reference) at the
reference's frame: 968 x 1296 RGB frames, the 2-row padding window, resize to 480 x 640, full ColorJitter with contrast in the
second slot, gray.  40 frames (the reference's batch: 8 tuples of 5) and 8 frames, antialias off and on.

Arms, per shape:
  (a) E.prepare_images: one e2emv_image_front call (3 launches: the call has a contrast slot)
  (b) the fp32 torch restatement (tests/image_front_restatement.py) on the CPU, torch.set_num_threads(16): what the data-loader
      workers of the reference do, on the CPUs one GPU command gets
  (c) the same restatement with torch ops on the device: what a user would write today without (a)
(a) and (c) start from the uint8 frames on the device, (b) from the uint8 frames on the host; no arm includes a host-device copy.

Repeats alternate between the arms ((b), seconds per step, runs fewer); minimum, median and maximum of the per-step time of a
repeat are reported.  (a)'s compulsory bytes - the input once, the gray output once - over its minimum time stand beside the
6.29 TB/s a copy kernel reaches on the MI355X, and so do they over (a)'s time on the device alone (the library's event chain around
its launches; the call time includes the Python front and three launches).  Writes profiles/image_front.json (--out)."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import e2e_multi_view_matching_amd as E  # noqa: E402
from e2e_multi_view_matching_amd import _lib  # noqa: E402
import image_front_restatement as R  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "image_front.json"))
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--steps", type=int, default=10, help="calls per repeat of the device arms")
ap.add_argument("--cpu-repeats", type=int, default=3, help="repeats of arm (b), one call each")
ap.add_argument("--batches", type=int, nargs="+", default=[40, 8])
args = ap.parse_args()

dev = torch.device("cuda:0")
torch.set_num_threads(16)
HIN, WIN, HOUT, WOUT = 968, 1296, 480, 640
WINDOW = (-2, 0, HIN + 4, WIN)
ORDER, FACTORS = (0, 1, 2, 3), (0.8, 1.3, 1.25, 0.1)  # contrast in the second slot
COPY_TBPS = 6.29


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


rows = []
for B in args.batches:
    host = torch.randint(0, 256, (B, HIN, WIN, 3), generator=torch.Generator().manual_seed(B), dtype=torch.uint8)
    frames = host.to(dev)
    for aa in (0, 1):
        kw = dict(out_size=(HOUT, WOUT), window=WINDOW, antialias=bool(aa), order=ORDER, factors=FACTORS)
        arms = {
            "a_prepare_images": (lambda: E.prepare_images(frames, **kw), args.steps, True),
            "c_torch_ops_on_device": (lambda: R.image_front(frames, torch.float32, **kw)[0], max(args.steps // 5, 1), True),
            "b_torch_ops_on_16_cpus": (lambda: R.image_front(host, torch.float32, **kw)[0], 1, False),
        }
        # the three arms compute the same image
        ga, gc = arms["a_prepare_images"][0](), arms["c_torch_ops_on_device"][0]()
        agree = float((ga - gc).abs().max())
        del ga, gc
        for name, (fn, steps, sync) in arms.items():  # warm-up: tables, allocator, clocks
            if name != "b_torch_ops_on_16_cpus":
                for _ in range(3):
                    fn()
        torch.cuda.synchronize()
        times = {k: [] for k in arms}
        for r in range(args.repeats):
            for name, (fn, steps, sync) in arms.items():  # alternating: every arm sees the same drift of the machine
                if name == "b_torch_ops_on_16_cpus" and r >= args.cpu_repeats:
                    continue
                times[name].append(per_step_ms(fn, steps, sync))
        res = {k: summary(v) for k, v in times.items()}
        a = res["a_prepare_images"]
        dev_ms = [device_ms(arms["a_prepare_images"][0], args.steps) for _ in range(args.repeats)]
        launches = dev_ms[0][1]
        dev_ms = summary([m for m, _ in dev_ms])
        bytes_compulsory = B * HIN * WIN * 3 + B * HOUT * WOUT * 4
        rows.append({
            "frames": B, "antialias": aa, "arms": res,
            "a_vs_c_max_abs_difference": agree,
            "a_compulsory_bytes": bytes_compulsory,
            "a_device_time": dev_ms, "a_launches_per_call": launches,
            "a_compulsory_bytes_over_min_time_TBps": round(bytes_compulsory / (a["min_ms"] * 1e-3) / 1e12, 4),
            "a_compulsory_bytes_over_min_device_time_TBps": round(bytes_compulsory / (dev_ms["min_ms"] * 1e-3) / 1e12, 4),
            "copy_rate_TBps": COPY_TBPS,
            "a_fraction_of_copy_rate": round(bytes_compulsory / (dev_ms["min_ms"] * 1e-3) / 1e12 / COPY_TBPS, 4),
            "c_over_a": round(res["c_torch_ops_on_device"]["min_ms"] / a["min_ms"], 2),
            "b_over_a": round(res["b_torch_ops_on_16_cpus"]["min_ms"] / a["min_ms"], 1),
            "a_beats_c_beyond_the_spread": bool(a["max_ms"] < res["c_torch_ops_on_device"]["min_ms"]),
        })
        print(json.dumps(rows[-1]), flush=True)
    del frames, host
    torch.cuda.empty_cache()

out = {
    "tool": "tools/bench_image_front.py", "device": torch.cuda.get_device_name(0),
    "shape": {"input": [HIN, WIN, 3], "window": list(WINDOW), "output": [HOUT, WOUT], "order": list(ORDER), "factors": list(FACTORS)},
    "clock": "host clock around N calls ending in a device synchronise (arm b: around one call); per-call time of a repeat; "
             "a_device_time: HIP events of the library's profile slots around the launches of N calls",
    "repeats": args.repeats, "calls_per_repeat": {"a": args.steps, "c": max(args.steps // 5, 1), "b": 1}, "cpu_repeats": args.cpu_repeats,
    "cpu_threads": torch.get_num_threads(), "rows": rows,
}
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    json.dump(out, fh, indent=1)
    fh.write("\n")
