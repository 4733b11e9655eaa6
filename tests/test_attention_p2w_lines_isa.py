"""Q of attention_p2w_kernel moves in whole cache lines, read from the device assembly (host test: cross-compiles, needs no
GPU).

A wave's 64 query rows x 256 B come in by LDS-direct pieces of 4 rows x 256 B into an image of its own and go from there into
the accumulator file by ds_read_b128; a fragment-shaped global_load_dwordx4 (32 rows x 32 B at a row stride of 2 KB) touched
32 lines for a quarter of each.  The output rows of the whole-item instances leave in 16 global_store_dwordx4 per wave (two
lanes' halves traded by v_permlane32_swap; sending them through the image in whole lines was measured and did not pay:
profiles/attention_full_lines.log).  So
  - no instance holds a global_load_dwordx4 whose destination is in the accumulator file;
  - a whole-item instance (not PART) holds at most 16 global_store_dwordx4."""
import os
import re
import shutil
import subprocess

import pytest

from e2e_multi_view_matching_amd import build as B

from test_gemm_p2_isa import HIPCC, kernels_of


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    if not (os.path.isfile(HIPCC) and os.access(HIPCC, os.X_OK)) and shutil.which(HIPCC) is None:
        pytest.skip("no hipcc")
    d = tmp_path_factory.mktemp("attention_p2w_lines")
    cmd = [HIPCC, "-save-temps=obj"] + B.FLAGS + ["-c", os.path.join(B.CSRC, "attention_p2w.hip"), "-o", os.path.join(str(d), "attention_p2w.o")]
    r = subprocess.run(cmd, cwd=str(d), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    ks = [k for k in kernels_of(open(os.path.join(str(d), "attention_p2w-hip-amdgcn-amd-amdhsa-gfx950.s")).read()) if "attention_p2w_kernel" in k[0]]
    assert len(ks) == 8, [k[0] for k in ks]  # HAS_E x MULTI x PART
    return ks


def _code(body):
    return [l.split(";")[0].strip() for l in body.split("\n")]


def _is_part(name):
    """the third template argument of attention_p2w_kernel<HAS_E, MULTI, PART> in the mangled name: ...ILb?ELb?ELb1EE..."""
    m = re.search(r"attention_p2w_kernelILb([01])ELb([01])ELb([01])EE", name)
    assert m, name
    return m.group(3) == "1"


def test_the_instances_are_four_whole_item_and_four_part(kernels):
    assert sorted(_is_part(k[0]) for k in kernels) == [False] * 4 + [True] * 4


def test_no_fragment_shaped_global_load_into_the_accumulator_file(kernels):
    for name, body, _, _ in kernels:
        bad = [l for l in _code(body) if re.match(r"global_load_dwordx4\s+a\[", l)]
        print(name, "global_load_dwordx4 into a[..]:", len(bad))
        assert not bad, (name, bad[:2])


def test_whole_item_instances_store_their_rows_in_16_instructions(kernels):
    for name, body, _, _ in kernels:
        if _is_part(name):
            continue
        st = [l for l in _code(body) if l.startswith("global_store_dwordx4 ")]
        print(name, "global_store_dwordx4", len(st))
        assert len(st) <= 16, (name, len(st))
