"""attention_p2w's output bits where its Q rows move through LDS in whole cache lines (-m gpu).

A wave stages its 64 query rows x 256 B in an LDS image of its own (16 LDS-direct pieces of 4 rows x 256 B, rows at and beyond
n_rows clamped to the last row per lane, issued in front of the walk's set-up; fragments read from the image into the
accumulator file), reads K(0) once for both streams and issues the pieces of the next two tiles between the MFMAs of the first
scores.  None of that touches an operand of an MFMA or of the softmax, or the order of the products: the output is the same
BYTES as that of the kernel that loaded Q in fragment-shaped quarter lines.  tests/golden/attention_p2w_lines_crc.json holds
the CRC32 of every image's valid output rows, written by tools/attention_p2w_crc.py --lines --write on an MI355X from that
earlier kernel.

So that the check does not rest on a record alone, the same outputs are held against the fp64 restatement
(tests/attention_restatement.py) at the bars of tests/test_gpu_attention_edges.py: max |out - fp64| over valid rows < 2e-5 and
< 3 err32 + 1e-6, err32 the fp32 kernel's error on the same input.  The case with operand scales (300, 1, 1e6) is outside the
data those bars were set for (randn x 1.5): its logits are 300 times larger, so fp32's own rounding of a logit (2^-24 of ~1e3)
moves a numerator by ~1e-4 of itself, and the output is 1e6 times larger.  It takes the bar of
tests/test_gpu_planes.py::test_attention_p2_tile_exponents_carry_fp32_range, which runs these scales: errors in units of
the v scale, err < 3 err32 + 3e-6.

Cases (tools/attention_p2w_crc.py: LINES_CASES), the smallest at which the new movement can go wrong: one valid row and one key
(every staged row but one a clamped duplicate, stores masked to 128 rows, the late pieces re-reading the only tile); a second
tuple whose last image ends the buffer inside a wave's 64 rows; n_rows = 256 exactly (no clamp anywhere); T = 3 with a second
query tile of 4 valid rows (one piece) and an image whose first query tile is half empty; n_rows = 384 with waves wholly beyond
it, tile exponents off zero; the key-split parts, which take the same Q path in front of their own epilogue."""
import functools
import importlib.util
import json
import os

import pytest
import torch

import attention_restatement as ar

pytestmark = pytest.mark.gpu

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("attention_p2w_crc", os.path.join(_ROOT, "tools", "attention_p2w_crc.py"))
crc = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(crc)

with open(crc.GOLDEN_LINES) as _fh:
    RECORD = json.load(_fh)

H = crc.H
BAR = 2e-5  # tests/test_gpu_attention_edges.py


def test_the_record_covers_every_case():
    assert sorted(RECORD["crc32"]) == sorted(c[0] for c in crc.LINES_CASES)
    assert all(len(RECORD["crc32"][c[0]]) == c[1] * len(c[2]) for c in crc.LINES_CASES)


@functools.lru_cache(maxsize=None)
def _output(dev, name):
    """the kernel's output of a case: computed once, shared by the two tests, never modified"""
    case = next(c for c in crc.LINES_CASES if c[0] == name)
    return crc.output_of_case(torch.device(dev), case)


@pytest.mark.parametrize("case", crc.LINES_CASES, ids=[c[0] for c in crc.LINES_CASES])
def test_output_bytes_equal_the_quarter_line_kernels(gpu, case):
    got = crc.crc_of_output(case, _output(str(gpu), case[0]))
    want = RECORD["crc32"][case[0]]
    print("attention-p2w-lines", case[0], " ".join("%08x" % x for x in got), "| record", " ".join("%08x" % x for x in want))
    assert got == want, (case[0], got, want)


@pytest.mark.parametrize("case", crc.LINES_CASES, ids=[c[0] for c in crc.LINES_CASES])
def test_outputs_are_inside_the_fp64_bar(gpu, case):
    import e2e_multi_view_matching_amd as E
    name, B, nv, cross, _, scales = case
    T = len(nv)
    qkv = crc.make_input(name, B, nv, cross, scales)
    ref = ar.attention_ref(qkv, B, T, nv, H, cross)
    out = _output(str(gpu), name)
    out32 = E.attention(qkv.to(gpu), B, T, list(nv), H, cross).cpu()
    vs = 1.0 if scales is None else scales[2]
    err, err32 = ar.valid_error(out, ref, T, nv) / vs, ar.valid_error(out32, ref, T, nv) / vs
    print(f"attention-p2w-lines {name} B={B} nv={nv} cross={cross}: err {err:.3e} err32 {err32:.3e} (units of the v scale {vs:g})")
    if scales is None:
        assert err < BAR, (name, err)
        assert err < 3 * err32 + 1e-6, (name, err, err32)
    else:
        assert err < 3 * err32 + 3e-6, (name, err, err32)
