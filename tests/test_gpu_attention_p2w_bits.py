"""attention_p2w's output bits against the record of the kernel as it was before its fragments moved into the accumulator
file (-m gpu).

The kernel reads every K / V^T fragment of a key tile from LDS once, in segment X, into a home in the accumulator file, and
both segments multiply out of the homes; the asm reads are waited for by hand-counted s_waitcnt lgkmcnt.  The MFMAs, their
order and their operands are those of the kernel that read each fragment once per segment, so the output is the same BYTES:
tests/golden/attention_p2w_parent_crc.json holds the CRC32 of every image's valid output rows, written by
tools/attention_p2w_crc.py on an MI355X from that earlier kernel.  A difference is a wrong wait or a stale home, not a
question of tolerance.

Cases (tools/attention_p2w_crc.py: CASES), the smallest at which the schedule can go wrong: one key tile (peeled segments
only), two (one steady X / Y pair), four and five (the LDS regions wrap, every home rewritten three times and more, a ragged
last tile, a second query tile with one valid row), three images (source walk), the key-split parts, operands that move the
tile exponents off zero."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("attention_p2w_crc", os.path.join(_ROOT, "tools", "attention_p2w_crc.py"))
crc = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(crc)

with open(crc.GOLDEN) as _fh:
    RECORD = json.load(_fh)


def test_the_record_covers_every_case():
    assert sorted(RECORD["crc32"]) == sorted(c[0] for c in crc.CASES)
    assert all(len(RECORD["crc32"][c[0]]) == c[1] * len(c[2]) for c in crc.CASES)


@pytest.mark.parametrize("case", crc.CASES, ids=[c[0] for c in crc.CASES])
def test_output_bytes_equal_the_parent_kernels(gpu, case):
    got = crc.crc_of_case(gpu, case)
    want = RECORD["crc32"][case[0]]
    print("attention-p2w-bits", case[0], " ".join("%08x" % x for x in got), "| record", " ".join("%08x" % x for x in want))
    assert got == want, (case[0], got, want)
