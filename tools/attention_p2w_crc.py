"""CRC32s of attention_p2w's output bytes at its smallest shapes: the record that a rework of the kernel's data movement (who
reads which fragment from where, and when) is compared against, bit for bit.

    python tools/attention_p2w_crc.py --write     # on an MI355X, from the commit whose bits are the reference

writes tests/golden/attention_p2w_parent_crc.json; tests/test_gpu_attention_p2w_bits.py recomputes the same CRCs and asserts
that they are equal.  Without --write the CRCs are printed and compared with the file.

A case = (name, B, nv, cross, key_split, scales): fp32 q|k|v of B tuples with nv[t] keypoints in image t, drawn as in
tests/test_gpu_attention_edges.py (randn * 1.5, rows padded to a multiple of 128), through E.attention_p2(..., waves=1).
scales = (q, k, v) factors that move the tile exponents off zero, with one 64-key block of image 0 three decades below the
others (the O accumulators are rescaled between tiles), as tests/test_gpu_planes.py does.

A second table, LINES_CASES, has a record of its own (--lines: tests/golden/attention_p2w_lines_crc.json, written from the
kernel whose Q rows still came in as fragment-shaped quarter lines; tests/test_gpu_attention_p2w_lines.py): the shapes at
which staging a wave's rows through LDS in whole lines can go wrong - clamped rows, masked stores, the end of the buffer
inside a wave's 64 rows."""
import json
import os
import sys
import zlib

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "attention_p2w_parent_crc.json")
H, D = 4, 256

CASES = [
    ("one-tile-self", 1, (64, 64), 0, False, None),          # one key tile: the peeled segments alone
    ("two-tiles-cross", 1, (128, 128), 1, False, None),      # one steady X / Y pair and the peel
    ("wrap-self", 1, (256, 256), 0, False, None),            # the three LDS regions wrap, every home rewritten three times
    ("wrap-ragged-cross", 1, (257, 257), 1, False, None),    # ... a last tile of one key, a second query tile with one valid row
    ("multi-source-cross", 1, (65, 1, 257), 1, False, None),  # T = 3: the walk from source to source (MULTI)
    ("key-split-cross", 1, (577, 70, 300), 1, True, None),   # the parts of the key split (PART)
    ("exponents-cross", 1, (200, 200), 1, False, (300.0, 1.0, 1e6)),  # tile exponents != 0, O rescaled between tiles
]

GOLDEN_LINES = os.path.join(ROOT, "tests", "golden", "attention_p2w_lines_crc.json")
LINES_CASES = [
    ("one-row-self", 1, (1, 1), 0, False, None),             # one valid row, one key: every staged row but one is a clamped duplicate, stores masked to 128 rows
    ("second-tuple-cross", 2, (129, 129), 1, False, None),   # b = img / T; the last image of the buffer ends inside a wave's 64 rows
    ("all-waves-self", 1, (256, 256), 0, False, None),       # n_rows = 256: four valid waves, no clamp anywhere
    ("piece-of-four-cross", 1, (260, 64, 130), 1, False, None),  # MULTI; a second query tile of 4 valid rows (one piece), an image whose tile 0 is half empty
    ("waves-beyond-cross", 1, (300, 300), 1, False, (300.0, 1.0, 1e6)),  # n_rows = 384: waves 2 and 3 of the second query tile lie beyond it; exponents
    ("key-split-cross", 1, (577, 70, 300), 1, True, None),   # PART: the staged Q in front of the fp32 records
]


def n_rows_of(nv):
    return (max(nv) + 127) // 128 * 128


def make_input(name, B, nv, cross, scales):
    T = len(nv)
    g = torch.Generator().manual_seed(1000 * T + sum(nv) + cross)
    qkv = torch.randn(B * T, n_rows_of(nv), 3 * D, generator=g) * 1.5
    if scales is not None:
        qkv[..., :D] *= scales[0]
        qkv[..., D:2 * D] *= scales[1]
        qkv[..., 2 * D:] *= scales[2]
        qkv[0, 64:128, 2 * D:] *= 1e-3
    return qkv


def parts_of(cus, B, nv, cross):
    """parts per leftover item of launch_attention_p2w, restated (as in tests/test_gpu_attention_edges.py)"""
    T = len(nv)
    n_items = 8 * ((B * T * H + 7) // 8) * ((max(nv) + 255) // 256)
    cus = max(8, cus // 8 * 8)
    r = n_items % cus
    min_tiles = min(sum((nv[s] + 63) // 64 for s in range(T) if (s != t if cross else s == t)) for t in range(T))
    return min(cus // r, 8, min_tiles) if r > 0 and 2 * r <= cus and r % 8 == 0 else 1


def output_of_case(dev, case):
    """the kernel's output [B*T, n_rows, D] of one case, on the host"""
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import e2e_multi_view_matching_amd as E
    from e2e_multi_view_matching_amd import _lib
    name, B, nv, cross, key_split, scales = case
    qkv = make_input(name, B, nv, cross, scales).to(dev)
    ctx = _lib.context(qkv.device)
    if key_split:
        parts = parts_of(torch.cuda.get_device_properties(dev).multi_processor_count, B, nv, cross)
        assert parts >= 2, (name, parts)  # precondition: the shape reaches the parts on this device
    try:
        ctx.set_attention_key_split(bool(key_split))
        out = E.attention_p2(qkv, B, len(nv), list(nv), H, cross, waves=1).cpu()
    finally:
        ctx.set_attention_key_split(True)
    return out


def crc_of_case(dev, case):
    """{image index: CRC32 of the bytes of its valid output rows} of one case, as a list"""
    return crc_of_output(case, output_of_case(dev, case))


def crc_of_output(case, out):
    name, B, nv = case[:3]
    T = len(nv)
    assert all(bool(torch.isfinite(out[g, :nv[g % T]]).all()) for g in range(B * T)), name
    return [zlib.crc32(out[g, :nv[g % T]].contiguous().numpy().tobytes()) for g in range(B * T)]


def main():
    dev = torch.device("cuda", 0)
    CASES, GOLDEN = (LINES_CASES, GOLDEN_LINES) if "--lines" in sys.argv else (globals()["CASES"], globals()["GOLDEN"])
    got = {c[0]: crc_of_case(dev, c) for c in CASES}
    again = {c[0]: crc_of_case(dev, c) for c in CASES}
    assert got == again, "two runs of the same build disagree"
    for k, v in got.items():
        print(k, " ".join("%08x" % x for x in v))
    if "--write" in sys.argv:
        with open(GOLDEN, "w") as fh:
            json.dump({"device": torch.cuda.get_device_properties(dev).gcnArchName.split(":")[0],
                       "compute_units": torch.cuda.get_device_properties(dev).multi_processor_count, "crc32": got}, fh, indent=1)
            fh.write("\n")
        print("wrote", GOLDEN)
    else:
        want = json.load(open(GOLDEN))["crc32"]
        bad = [k for k in got if got[k] != want.get(k)]
        print("differs from the record:" if bad else "equal to the record", " ".join(bad))
        return 1 if bad else 0
    return 0


if __name__ == "__main__":
    sys.exit(main())
