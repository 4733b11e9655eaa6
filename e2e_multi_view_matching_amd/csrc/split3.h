// bf16x3 operand splitting (the split-operand path of the bf16x3 mode):
//
//   x = x1 + x2 + x3,  x1 = bf16(x), x2 = bf16(x - x1), x3 = bf16(x - x1 - x2)   (|x - x1 - x2 - x3| <= 2^-26 |x|)
//   a*b ~= a1b1 + a1b2 + a2b1 + a1b3 + a2b2 + a3b1            (dropped terms <= 2^-25 |ab|)
//
// Every bf16 x bf16 product is exact in fp32 and the bf16 MFMAs accumulate in fp32, so a contraction on split operands carries
// fp32-class rounding; bf16 keeps fp32's exponent range, so unlike an fp16 split there is no overflow/underflow hazard.
// "S3" layout: row r = [plane0 | plane1 | plane2], each ld bf16 wide.  The split is made by the consumers on the way into LDS
// (gemm_x3.hip, which inlines its own; attention_x3.hip) and, for the static weights, by the row splitter of split3_api.hip.
#pragma once

namespace e2emv {

__device__ __forceinline__ void split3(float v, __bf16& a, __bf16& b, __bf16& c) {
    a = (__bf16)v;
    const float r1 = v - (float)a;
    b = (__bf16)r1;
    const float r2 = r1 - (float)b;
    c = (__bf16)r2;
}

}  // namespace e2emv
