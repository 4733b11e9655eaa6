"""Register budget of the fused keypoint-encoder front, read from the kernel metadata (host test: cross-compiles, needs no GPU).

kenc_fused.hip keeps 64 accumulator registers, the 64 prefetched descriptor values of the residual and the operand fragments
of a K step in the registers of a wave that shares its SIMD with one other (512 threads per workgroup, one workgroup per CU): a
spilled register would put scratch traffic into the K loops.  The kernel must use no private segment and spill no vector
register."""
import os
import shutil
import subprocess

import pytest

from e2e_multi_view_matching_amd import build as B
from test_gemm_p2_isa import kernels_of

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    if not (os.path.isfile(HIPCC) and os.access(HIPCC, os.X_OK)) and shutil.which(HIPCC) is None:
        pytest.skip("no hipcc")
    d = tmp_path_factory.mktemp("kenc_fused")
    cmd = [HIPCC, "-save-temps=obj"] + B.FLAGS + ["-c", os.path.join(B.CSRC, "kenc_fused.hip"), "-o", os.path.join(str(d), "kenc_fused.o")]
    r = subprocess.run(cmd, cwd=str(d), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    ks = kernels_of(open(os.path.join(str(d), "kenc_fused-hip-amdgcn-amd-amdhsa-gfx950.s")).read())
    assert [name for name, *_ in ks if "kenc_fused_kernel" in name], "kenc_fused_kernel not found in the assembly"
    return ks


def test_kenc_fused_is_built_into_the_library():
    assert "kenc_fused.hip" in B.SOURCES


def test_no_private_segment_and_no_spilled_vector_register(kernels):
    for name, _, f, _ in kernels:
        print(name, "private segment", f["private_segment_fixed_size"], "spilled vector registers", f["vgpr_spill_count"], "vgpr_count", f["vgpr_count"])
        assert f["private_segment_fixed_size"] == 0 and f["vgpr_spill_count"] == 0, (name, f)
