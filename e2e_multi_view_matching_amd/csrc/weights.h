// Weights of the matcher as the kernels see them: one record per dense layer, built by e2emv_commit_weights (weights.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <vector>

struct e2emv_ctx;

namespace e2emv {

struct HostTensor {
    std::vector<float> data;
    std::vector<int64_t> shape;
};

struct DenseWeights {            // one dense layer y = W x + b, W [out][in] row-major, BN / merge already folded
    int out = 0, in = 0;
    const float* w = nullptr;  const float* b = nullptr;      // weight arena
    const uint16_t* w3 = nullptr;   // bf16 x 3 planes  [out][3][in]        (null: format not built for this layer)
    const uint16_t* wh = nullptr;   // fp16 x 2 planes  [out][{hi,lo}][in] of 2^s W
    const uint16_t* wp = nullptr;   // the same numbers in P2 blocks (p2.h)
    float hs = 0.f;                 // 2^-s
    float ba = 0.f;                 // max |b| (bound for the tile exponents, p2.h)
};

struct LayerWeights {
    DenseWeights qkv;   // [3D][D]   rows head-major: q | k | v
    DenseWeights mlp0;  // [2D][2D]  BN folded, attn.merge folded into the second K segment
    DenseWeights mlp1;  // [D][2D]
    int type = 0;       // 0 self, 1 cross
};

enum { WF_S3 = 1, WF_H2 = 2, WF_P2 = 4 };  // the 16-bit formats of a DenseWeights (w3, wh, wp)

// raw tensor `k` of e2emv_set_weight, or null
const HostTensor* find(e2emv_ctx* ctx, const std::string& k);

// Test entry points: the record of a layer whose fp32 weights d_W [out][in] and bias d_bias [out] (may be null) are on the
// device, with ONE 16-bit format made in d_planes by the host code of the commit path (WF_S3: out x 3 x in halves, else
// out x 2 x in).  Host-synchronising.
int dense_from_device(e2emv_ctx* ctx, const float* d_W, const float* d_bias, int out, int in, int format, uint16_t* d_planes,
                      DenseWeights& dw, hipStream_t s);

}  // namespace e2emv
