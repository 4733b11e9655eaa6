// Shared by the two split-operand attention kernels on the fp32 q|k|v matrix (attention_x3.hip: three bf16 planes, six products;
// attention_h2.hip: two fp16 planes, three products): parameters, tile sizes and the LDS image of a plane tile.
#pragma once
#include "attention_walk.h"
#include "common.h"

namespace e2emv {

typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;
typedef __attribute__((ext_vector_type(2))) unsigned int u32x2;

constexpr int A3_Q = 128, A3_KV = 64, A3_HD = 64;
constexpr int A3_LD = 72;                 // LDS row: 64 16-bit elements + 8 pad = 144 B (36 dwords: conflict-free b128 reads)
constexpr int A3_PLANE = 64 * A3_LD;      // 16-bit elements per LDS plane tile

struct Attn3fParams : AttnShape {
    const float* qkv;     // [n_img*n_rows][3D]  q | k | v, head-major channels
    float* out32;         // [n_img*n_rows][D]
    float q_scale;        // log2(e) / sqrt(64)
};

// the launchers' common part: checks, shape (nq in tiles of A3_Q queries) and the buffers
inline int attn3f_params(e2emv_ctx* ctx, const char* who, int B, int T, int n_rows, const int* nv, int D, int H, const float* qkv,
                         int cross, float* out32, Attn3fParams* p, int* n_valid) {
    if (int rc = attn_shape(ctx, who, B, T, n_rows, nv, D, H, cross, A3_Q, p, n_valid)) return rc;
    if (!qkv || !out32 || (uintptr_t)qkv % 16 || (uintptr_t)out32 % 16) return set_err(ctx, E2EMV_EINVAL, "%s: null / unaligned buffer", who);
    p->qkv = qkv; p->out32 = out32;
    p->q_scale = 0.125f * 1.4426950408889634f;
    return E2EMV_OK;
}

}  // namespace e2emv
