"""sinkhorn_resident128w (csrc/sinkhorn_regs2.hip) runs two waves per SIMD: a wave has 256 vector registers and nothing else.
12 of its 16 rows live in v64 .. v255, addressed by number; the compiler is confined to v0 .. v63 and has no accumulation
registers to spill into, so anything that does not fit would go to scratch inside the iteration loop.  The device assembly the
build kept is the proof that it does not (no GPU needed; build.py runs the same check on every build)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _kept_asm():
    """The device assembly the build kept for the file of build.REGISTER_WINDOW_W (re-made from that one file when stale)."""
    from e2e_multi_view_matching_amd import build
    src = os.path.join(build.CSRC, build.REGISTER_WINDOW_W[0])
    asm = os.path.join(ROOT, "e2e_multi_view_matching_amd", "build", build.REGISTER_WINDOW_W[0].replace(".hip", ".s"))
    if not os.path.exists(asm) or os.path.getmtime(asm) < os.path.getmtime(src):
        subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + build.FLAGS + ["--cuda-device-only", "-S", src, "-o", asm],
                       check=True, capture_output=True)
    return asm


def test_sinkhorn128w_stays_inside_64_registers_without_scratch(lib_built):
    from e2e_multi_view_matching_amd import build
    asm = _kept_asm()
    assert build.REGISTER_WINDOW_W == ("sinkhorn_regs2.hip", ("sinkhorn_resident128w",), 64)
    assert build.REGISTER_WINDOW_W[0] in build.SOURCES
    assert build.check_register_window_vgpr(asm, "sinkhorn_resident128w", 64) == 4  # full tiles / ragged x 8 / 4 lanes per column pair in stage A
    # the check does fail for a window the kernel does not keep
    with pytest.raises(RuntimeError, match="outside its window"):
        build.check_register_window_vgpr(asm, "sinkhorn_resident128w", 48)
    txt = open(asm).read()
    for inst in ("ILb1ELi8E", "ILb0ELi8E", "ILb1ELi4E", "ILb0ELi4E"):
        at = txt.index(".name:", txt.index("amdhsa.kernels:"))  # this instance's entry of the metadata: "  - .agpr_count: ..." to .wavefront_size
        while "sinkhorn_resident128w" + inst not in txt[at:txt.index("\n", at)]:
            at = txt.index(".name:", at + 1)
        meta = txt[txt.rindex("- .agpr_count:", 0, at):txt.index(".wavefront_size", at)]
        # the code object's own account: 256 registers, none of them accumulation registers, nothing spilled, no scratch
        assert re.search(r"\.vgpr_count:\s+256\b", meta) and re.search(r"\.agpr_count:\s+0\b", meta), inst
        assert re.search(r"\.vgpr_spill_count:\s+0\b", meta) and re.search(r"\.private_segment_fixed_size:\s+0\b", meta), inst
        assert re.search(r"\.max_flat_workgroup_size:\s+512\b", meta), inst


def test_sinkhorn128w_addresses_its_rows_by_number(lib_built):
    """What DOES touch v64 .. v255: 192 writes per problem, and per iteration 8 packed operations per register row in each of
    the two passes (row sums, column sums)."""
    asm = _kept_asm()
    txt = open(asm).read()
    body = txt[txt.index("sinkhorn_resident128wILb1ELi8E"):]
    body = body[:body.index(".end_amdhsa_kernel")]
    mine = [ln for ln in body.splitlines() if re.search(r"\b(v_mov_b32|v_pk_(fma|mul)_f32).*v\[(0x[0-9a-f]+|\d+)[+\]]", ln)]
    assert len(mine) == 192 + 2 * (12 * 8)


def test_the_old_kernels_window_check_rejects_this_layout_and_vice_versa(lib_built):
    """The two checks are not interchangeable: sinkhorn_resident128 is allocated 256 + 256 registers, sinkhorn_resident128w 256."""
    from e2e_multi_view_matching_amd import build
    with pytest.raises(RuntimeError, match="256 \\+ 256"):
        build.check_register_window(_kept_asm(), "sinkhorn_resident128w", 64)
    old = os.path.join(ROOT, "e2e_multi_view_matching_amd", "build", build.REGISTER_WINDOW[0].replace(".hip", ".s"))
    if os.path.exists(old):
        with pytest.raises(RuntimeError, match="256 vector registers"):
            build.check_register_window_vgpr(old, "sinkhorn_resident128", 56)
