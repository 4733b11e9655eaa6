"""Register budget and fragment traffic of attention_p2w.hip, read from the device assembly (host test: cross-compiles, needs
no GPU).

A wave of attention_p2w_kernel owns a SIMD (512 registers).  Its accumulator file holds O (64 registers), the Q fragments (64)
and the HOMES of the K / V^T fragments of a key tile (128): segment X of a tile reads each fragment from LDS once, into its
home, and both segments take their MFMA A operands from there.  Every instance (HAS_E x MULTI x PART) must therefore
  - fit the wave with no scratch and no spilled register, at most 256 registers on either side of accum_offset;
  - hold the 192 MFMAs of the parent (48 of the prologue's scores, 2 x 48 of a steady tile, 2 x 24 of the peeled last one);
  - hold at most 96 ds_read_b128 (one read per fragment and segment: 128; the homes: 32 prologue + 8 + 32 steady + 8 peeled = 80),
    at least 48 of them into the accumulator file;
  - take MFMA A operands from the accumulator file.
The asm LDS reads are not counted by the compiler, which takes a home for written where the read is issued: between a read and
the first MFMA that names its destination no v_accvgpr instruction may touch that destination (a copy there would move
the home's OLD contents)."""
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
    d = tmp_path_factory.mktemp("attention_p2w")
    cmd = [HIPCC, "-save-temps=obj"] + B.FLAGS + ["-c", os.path.join(B.CSRC, "attention_p2w.hip"), "-o", os.path.join(str(d), "attention_p2w.o")]
    r = subprocess.run(cmd, cwd=str(d), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    ks = [k for k in kernels_of(open(os.path.join(str(d), "attention_p2w-hip-amdgcn-amd-amdhsa-gfx950.s")).read()) if "attention_p2w_kernel" in k[0]]
    assert len(ks) == 8, [k[0] for k in ks]  # HAS_E x MULTI x PART
    return ks


def _code(body):
    return [l.split(";")[0].strip() for l in body.split("\n")]


def test_every_instance_fits_one_wave_per_simd_without_scratch(kernels):
    for name, body, f, d in kernels:
        print(name, "next_free_vgpr", d["next_free_vgpr"], "accum_offset", d["accum_offset"], "scratch", f["private_segment_fixed_size"],
              "spilled", f["vgpr_spill_count"])
        assert f["private_segment_fixed_size"] == 0 and f["vgpr_spill_count"] == 0 and "scratch_" not in body, (name, f)
        assert d["next_free_vgpr"] <= 512 and d["accum_offset"] <= 256 and d["next_free_vgpr"] - d["accum_offset"] <= 256, (name, d)


def test_every_instance_holds_the_192_mfmas_of_the_tile_program(kernels):
    for name, body, _, _ in kernels:
        mf = [l for l in _code(body) if l.startswith("v_mfma")]
        print(name, len(mf))
        assert len(mf) == 192 and all(l.startswith("v_mfma_f32_32x32x16_f16 ") for l in mf), (name, len(mf))


def test_fragments_are_read_once_into_the_accumulator_file(kernels):
    for name, body, _, _ in kernels:
        rd = [l for l in _code(body) if l.startswith("ds_read_b128 ")]
        to_acc = [l for l in rd if re.match(r"ds_read_b128\s+a\[", l)]
        print(name, "ds_read_b128", len(rd), "into the accumulator file", len(to_acc))
        assert len(rd) <= 96, (name, len(rd))
        assert len(to_acc) >= 48, (name, len(to_acc))


def test_no_compiler_copy_touches_a_home_between_its_read_and_its_first_use(kernels):
    for name, body, _, _ in kernels:
        pending = {}  # "a[lo:hi]" -> its registers, from the read to the first MFMA naming the quad (in the order of the text)
        for l in _code(body):
            m = re.match(r"ds_read_b128\s+(a\[(\d+):(\d+)\])", l)
            if m:
                pending[m.group(1)] = set(range(int(m.group(2)), int(m.group(3)) + 1))
            elif l.startswith("v_mfma"):
                for quad in re.findall(r"a\[\d+:\d+\]", l):
                    pending.pop(quad, None)
            elif "accvgpr" in l:
                regs = {int(x) for x in re.findall(r"\ba(\d+)\b", l)}
                assert not any(regs & p for p in pending.values()), (name, l)


def test_mfmas_take_their_a_operand_from_the_accumulator_file(kernels):
    for name, body, _, _ in kernels:
        mf = [l for l in _code(body) if l.startswith("v_mfma")]
        a_acc = [l for l in mf if re.match(r"v_mfma\S+\s+[av]\[\d+:\d+\],\s*a\[", l)]
        print(name, "MFMAs with A in the accumulator file", len(a_acc))
        # every MFMA of the segments (2 x 48 steady + 2 x 24 peeled); the prologue's 48 first scores read K through VGPRs
        assert len(a_acc) == 144, (name, len(a_acc))
