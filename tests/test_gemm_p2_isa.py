"""Register budget and MFMA shape of the plane GEMMs, read from the device assembly (host test: cross-compiles, needs no GPU).

gemm_p2.hip and gemm_p2c.hip run two waves per SIMD with 128 accumulator registers each and count their memory operations
(s_waitcnt vmcnt(N) with N > 0): a register spilled inside the K loop brings a scratch reload and an s_waitcnt vmcnt(0) into that
pipeline.  Every kernel of both files must therefore fit 256 registers per wave with no scratch and no spilled vector register,
and its K steps must be made of v_mfma_f32_16x16x32_f16 alone, 96 per step (csrc/gemm_p2_core.h: gp_kstep)."""
import os
import re
import shutil
import subprocess

import pytest

from e2e_multi_view_matching_amd import build as B

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
MFMAS_PER_KSTEP = 96


def kernels_of(asm_text):
    """[(name, body, metadata, descriptor)] of every kernel in a device assembly file"""
    out = []
    for m in re.finditer(r"^\s*\.amdhsa_kernel\s+(\S+)", asm_text, re.M):
        name = m.group(1)
        start = re.search(r"^%s:" % re.escape(name), asm_text, re.M)
        meta = re.search(r"\.name:\s+%s\n(.*?)\.wavefront_size" % re.escape(name), asm_text, re.S)
        assert start and meta, name
        fields = {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\s*$", meta.group(1), re.M)}
        desc = asm_text[m.end():asm_text.index(".end_amdhsa_kernel", m.end())]
        dfields = {k: int(v) for k, v in re.findall(r"\.amdhsa_(\w+)\s+(\d+)\s*$", desc, re.M)}
        out.append((name, asm_text[start.end():m.start()], fields, dfields))
    return out


@pytest.fixture(scope="module", params=["gemm_p2.hip", "gemm_p2c.hip"])
def kernels(request, tmp_path_factory):
    if not (os.path.isfile(HIPCC) and os.access(HIPCC, os.X_OK)) and shutil.which(HIPCC) is None:
        pytest.skip("no hipcc")
    d = tmp_path_factory.mktemp(request.param.replace(".hip", ""))
    stem = request.param.replace(".hip", "")
    cmd = [HIPCC, "-save-temps=obj"] + B.FLAGS + ["-c", os.path.join(B.CSRC, request.param), "-o", os.path.join(str(d), stem + ".o")]
    r = subprocess.run(cmd, cwd=str(d), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    ks = kernels_of(open(os.path.join(str(d), stem + "-hip-amdgcn-amd-amdhsa-gfx950.s")).read())
    assert ks, "no kernel found in the assembly of " + request.param
    return ks


def test_every_kernel_fits_two_waves_per_simd(kernels):
    """the kernel descriptor's allocation: vector registers [0, accum_offset) + accumulation registers [accum_offset, next_free_vgpr)
    in one unified file of 512 per SIMD lane - two waves fit when next_free_vgpr <= 256"""
    for name, _, f, d in kernels:
        print(name, "next_free_vgpr", d["next_free_vgpr"], "accum_offset", d["accum_offset"], "vgpr_count", f["vgpr_count"])
        assert d["next_free_vgpr"] <= 256 and d["accum_offset"] <= 256 and f["vgpr_count"] <= 256, (name, d, f)


def test_no_scratch_and_no_spilled_vector_register(kernels):
    for name, body, f, _ in kernels:
        print(name, "scratch", f["private_segment_fixed_size"], "spilled vector registers", f["vgpr_spill_count"])
    for name, body, f, _ in kernels:
        assert f["private_segment_fixed_size"] == 0 and f["vgpr_spill_count"] == 0 and "scratch_" not in body, (name, f)


def test_k_steps_are_96_mfmas_of_the_16x16x32_shape(kernels):
    for name, body, _, _ in kernels:
        n16 = len(re.findall(r"^\s*v_mfma_f32_16x16x32_f16\b", body, re.M))
        other = [l.split()[0] for l in body.split("\n") if l.strip().startswith("v_mfma") and "v_mfma_f32_16x16x32_f16" not in l]
        print(name, n16, other[:3])
        # a kernel holds the first K step of a tile (zero C operand) and the steady-state step, inlined once each or more
        assert not other and n16 >= 2 * MFMAS_PER_KSTEP and n16 % MFMAS_PER_KSTEP == 0, (name, n16, other[:3])
