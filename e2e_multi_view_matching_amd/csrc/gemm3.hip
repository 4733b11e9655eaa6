// bf16x3 operand splitting (the split-operand path of the bf16x3 mode):
//
//   x = x1 + x2 + x3,  x1 = bf16(x), x2 = bf16(x - x1), x3 = bf16(x - x1 - x2)   (|x - x1 - x2 - x3| <= 2^-26 |x|)
//   a*b ~= a1b1 + a1b2 + a2b1 + a1b3 + a2b2 + a3b1            (dropped terms <= 2^-25 |ab|)
//
// Every bf16 x bf16 product is exact in fp32 and the bf16 MFMAs accumulate in fp32, so a GEMM on split operands carries
// fp32-class rounding; bf16 keeps fp32's exponent range, so unlike an fp16 split there is no overflow/underflow hazard.
// "S3" layout: row r = [plane0 | plane1 | plane2], each ld bf16 wide.  The GEMM that consumes the planes is gemm_x3.hip (its
// first generation, every operand as planes in HBM, is retired); this file keeps the row splitter that makes S3 planes.
#include "common.h"

namespace e2emv {
__device__ __forceinline__ void split3(float v, __bf16& a, __bf16& b, __bf16& c) {
    a = (__bf16)v;
    const float r1 = v - (float)a;
    b = (__bf16)r1;
    const float r2 = r1 - (float)b;
    c = (__bf16)r2;
}

// fp32 [rows][C] -> S3 [rows][3][ld] (the weight planes of e2emv_gemm_bf16x3, split3_api.hip)
__global__ void split3_rows_kernel(const float* src, int64_t rows, int C, int64_t lds_, uint16_t* dst, int64_t ld) {
    const int64_t r = blockIdx.x;
    for (int c = threadIdx.x; c < C; c += blockDim.x) {
        __bf16 a, b, d;
        split3(src[r * lds_ + c], a, b, d);
        __bf16* o = reinterpret_cast<__bf16*>(dst + r * 3 * ld);
        o[c] = a; o[ld + c] = b; o[2 * ld + c] = d;
    }
}

int launch_split3(e2emv_ctx* ctx, const float* src, int64_t rows, int C, int64_t ld_src, uint16_t* dst, int64_t ld,
                  hipStream_t s) {
    if (rows <= 0 || C <= 0) return E2EMV_OK;
    hipLaunchKernelGGL(split3_rows_kernel, dim3((unsigned)rows), dim3(256), 0, s, src, rows, C, ld_src, dst, ld);
    E2EMV_CHECK_LAUNCH(ctx, "split3_rows_kernel");
    return E2EMV_OK;
}

}  // namespace e2emv
