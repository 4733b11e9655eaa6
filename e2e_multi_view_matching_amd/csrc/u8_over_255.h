// ToTensor's / the pair loader's u8 / 255, shared by image_front.hip and image_front_pairs.hip.
#pragma once
#include <hip/hip_runtime.h>

namespace e2emv {

// u8 / 255 - a true fp32 division (x * (1 / 255) alone differs on 126 of the 256 values): the product and one fused
// correction step give the correctly rounded quotient for every byte (checked against the division for all 256 on the host,
// and by the byte tests on the device)
__device__ __forceinline__ float u8_over_255(unsigned byte) {
    const float x = float(byte), rcp = 1.0f / 255.0f;
    const float q = __fmul_rn(x, rcp);
    return fmaf(fmaf(-q, 255.0f, x), rcp, q);
}

}  // namespace e2emv
