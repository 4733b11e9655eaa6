// Fused multi-head attention on the bf16 matrix pipe with fp32-class accuracy (operand splitting,
// see split3.h): every contraction is the 6-term product of 3-way bf16 splits accumulated in fp32.
//
// Same transposed, lane-owns-a-query structure as attention.hip:
//   S^T[key][q]  = sum over 6 (Ki, Qj) plane pairs of mfma_32x32x16_bf16(A = K rows, B = Q rows)
//   O^T[d][q]   += sum over 6 (Vi, Pj) plane pairs of mfma(A = V^T rows, B = P^T)
// V is stored TRANSPOSED in LDS, because the MFMA operand of the P.V product needs 8 consecutive
// KEYS per lane.  The softmax probabilities are split into
// three bf16 planes in registers; with the S^T accumulator layout (row = (r&3)+8(r>>2)+4(lane>>5))
// registers 8u..8u+7 of a lane are exactly the 8 K-slots that lane must supply for the u-th
// 16-key MFMA, provided the V^T tile is stored in LDS with the matching key order inside each
// 16-key group (pos = (k&3) + 4*((k>>3)&1) + 8*((k>>2)&1)) - so P never leaves its lane.
//
// Fed with the fp32 q|k|v matrix of the projection GEMM ([n_img*n_rows][3D], the fp32 kernel's layout): the three bf16 planes
// of Q (registers), K and V^T (LDS) are produced HERE, on the way in.  The q|k|v GEMM then is an ordinary split-operand GEMM with
// a 4-byte-per-element output; the price is that the query tiles of one (image, head) each split the same K / V tiles again
// (VALU work next to a matrix-bound loop).  q is scaled by log2(e)/sqrt(d) in fp32 before it is split.
#include "attention_split.h"
#include "split3.h"

namespace e2emv {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;

__global__ __launch_bounds__(256, 2) void attention3f_kernel(Attn3fParams p) {
    __shared__ __attribute__((aligned(16))) uint16_t Ks[3 * A3_PLANE];
    __shared__ __attribute__((aligned(16))) uint16_t Vs[3 * A3_PLANE];

    const AttnItem it = attn_item(p, blockIdx.x, A3_Q);
    if (!it.live) return;
    const int qt = it.qt, img = it.img, head = it.head, b = it.b, t = it.t;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, lh = lane >> 5;
    const int64_t ld = 3 * (int64_t)p.D;  // floats per q|k|v row

    // ---- Q fragments (B operand): lane (q, lh) holds Q_pl[q][16 s + 8 lh .. +7]
    const int q_row = qt * A3_Q + wave * 32 + l31;
    bf16x8 Qf[3][4];
    {
        const float* qp = p.qkv + ((int64_t)img * p.n_rows + q_row) * ld + head * A3_HD + lh * 8;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const f32x4 lo = *reinterpret_cast<const f32x4*>(qp + s * 16), hi = *reinterpret_cast<const f32x4*>(qp + s * 16 + 4);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                __bf16 a, bb, c;
                split3((e < 4 ? lo[e] : hi[e - 4]) * p.q_scale, a, bb, c);
                Qf[0][s][e] = a; Qf[1][s][e] = bb; Qf[2][s][e] = c;
            }
        }
    }

    f32x16 O0, O1;
#pragma unroll
    for (int r = 0; r < 16; ++r) { O0[r] = 0.f; O1[r] = 0.f; }
    float m_run = -1e30f, l_run = 0.f;

    using Walk = AttnKeyWalk<A3_KV>;
    const Walk walk(p, t);
    const int n_tiles = walk.n_tiles;

    // staging.  K tile (64 keys x 64 dims fp32): thread -> key row tid/4, 16 dims (tid&3)*16: 4 x 16 B, 64 B contiguous.
    // V tile: thread -> a 4 keys x 4 dims block: key block kb = (lane>>2) (16 blocks), dims 16*wave + 4*(lane&3): 4 x 16 B
    // from 4 consecutive key rows; after the split it owns, per dim, 4 consecutive keys = one 8-byte V^T write per plane.
    const int k_row = tid >> 2, k_c16 = (tid & 3) * 16;
    const int v_kb = lane >> 2, v_d0 = 16 * wave + 4 * (lane & 3);
    // V^T LDS position of keys 4 kb .. 4 kb + 3 inside their 16-key group (permuted order, see the header)
    const int v_lds = 16 * (v_kb >> 2) + 4 * ((v_kb & 3) >> 1) + 8 * (v_kb & 1);
    f32x4 rk[4], rv[4];
    auto gload = [&](const Walk::Pos& tp) {
        const int tt = walk.src(tp.si), kt = tp.kt;
        const float* base = p.qkv + ((int64_t)(b * p.T + tt) * p.n_rows + kt * A3_KV) * ld + head * A3_HD;
        const float* kp = base + p.D + (int64_t)k_row * ld + k_c16;
        const float* vp = base + 2 * p.D + (int64_t)(4 * v_kb) * ld + v_d0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            rk[i] = *reinterpret_cast<const f32x4*>(kp + 4 * i);
            rv[i] = *reinterpret_cast<const f32x4*>(vp + (int64_t)i * ld);
        }
    };
    auto lstore = [&]() {
        // K: 16 values -> 3 planes x 32 B
        bf16x8 kh[3][2];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                __bf16 a, bb, c;
                split3(rk[i][e], a, bb, c);
                kh[0][i >> 1][(i & 1) * 4 + e] = a; kh[1][i >> 1][(i & 1) * 4 + e] = bb; kh[2][i >> 1][(i & 1) * 4 + e] = c;
            }
#pragma unroll
        for (int pl = 0; pl < 3; ++pl) {
            uint16_t* kd = &Ks[pl * A3_PLANE + k_row * A3_LD + k_c16];
            *reinterpret_cast<bf16x8*>(kd) = kh[pl][0];
            *reinterpret_cast<bf16x8*>(kd + 8) = kh[pl][1];
        }
        // V^T: rv[i][e] = V[key 4 kb + i][dim d0 + e]
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            bf16x4 vh[3];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                __bf16 a, bb, c;
                split3(rv[i][e], a, bb, c);
                vh[0][i] = a; vh[1][i] = bb; vh[2][i] = c;
            }
#pragma unroll
            for (int pl = 0; pl < 3; ++pl)
                *reinterpret_cast<bf16x4*>(&Vs[pl * A3_PLANE + (v_d0 + e) * A3_LD + v_lds]) = vh[pl];
        }
    };

    constexpr int PA[6] = {2, 1, 0, 1, 0, 0};  // plane of the A operand (K or V^T), smallest terms first
    constexpr int PB[6] = {0, 1, 2, 0, 1, 0};  // plane of the B operand (Q or P)

    Walk::Pos cur{0, 0}, nxt{0, 0};
    gload(nxt);
    for (int tile = 0; tile < n_tiles; ++tile) {
        __syncthreads();
        lstore();
        __syncthreads();
        cur = nxt;
        if (tile + 1 < n_tiles) {
            walk.advance(nxt);
            gload(nxt);
        }
        const int valid_in_tile = walk.valid(cur);
#pragma unroll
        for (int sub = 0; sub < 2; ++sub) {
            if (sub * 32 >= valid_in_tile) break;
            f32x16 S;
#pragma unroll
            for (int r = 0; r < 16; ++r) S[r] = 0.f;
            const uint16_t* kp = &Ks[(sub * 32 + l31) * A3_LD + lh * 8];
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                bf16x8 kf[3];
#pragma unroll
                for (int pl = 0; pl < 3; ++pl) kf[pl] = *reinterpret_cast<const bf16x8*>(kp + pl * A3_PLANE + s * 16);
#pragma unroll
                for (int q = 0; q < 6; ++q) S = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf[PA[q]], Qf[PB[q]][s], S, 0, 0, 0);
            }
            if (valid_in_tile < sub * 32 + 32) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int key = sub * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                    if (key >= valid_in_tile) S[r] = -INFINITY;
                }
            }
            float mx = S[0];
#pragma unroll
            for (int r = 1; r < 16; ++r) mx = fmaxf(mx, S[r]);
            mx = fmaxf(mx, __shfl_xor(mx, 32));
            const float m_new = fmaxf(m_run, mx);
            const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
            float ps = 0.f;
            bf16x8 Pf[3][2];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float pv = __builtin_amdgcn_exp2f(S[r] - m_new);
                ps += pv;
                __bf16 a, bb, c;
                split3(pv, a, bb, c);
                Pf[0][r >> 3][r & 7] = a;
                Pf[1][r >> 3][r & 7] = bb;
                Pf[2][r >> 3][r & 7] = c;
            }
            l_run = l_run * alpha + ps;
            m_run = m_new;
#pragma unroll
            for (int r = 0; r < 16; ++r) { O0[r] *= alpha; O1[r] *= alpha; }
            const uint16_t* vp = &Vs[l31 * A3_LD + lh * 8];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                bf16x8 v0[3], v1[3];
#pragma unroll
                for (int pl = 0; pl < 3; ++pl) {
                    v0[pl] = *reinterpret_cast<const bf16x8*>(vp + pl * A3_PLANE + 16 * (2 * sub + u));
                    v1[pl] = *reinterpret_cast<const bf16x8*>(vp + pl * A3_PLANE + 32 * A3_LD + 16 * (2 * sub + u));
                }
#pragma unroll
                for (int q = 0; q < 6; ++q) {
                    O0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(v0[PA[q]], Pf[PB[q]][u], O0, 0, 0, 0);
                    O1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(v1[PA[q]], Pf[PB[q]][u], O1, 0, 0, 0);
                }
            }
        }
    }

    const float l_tot = l_run + __shfl_xor(l_run, 32);
    const float inv = 1.f / l_tot;
    float* op = p.out32 + ((int64_t)img * p.n_rows + q_row) * p.D + head * A3_HD + 4 * lh;
#pragma unroll
    for (int gq = 0; gq < 4; ++gq) {
        f32x4 a, c;
#pragma unroll
        for (int e = 0; e < 4; ++e) { a[e] = O0[gq * 4 + e] * inv; c[e] = O1[gq * 4 + e] * inv; }
        *reinterpret_cast<f32x4*>(op + 8 * gq) = a;
        *reinterpret_cast<f32x4*>(op + 32 + 8 * gq) = c;
    }
}

int launch_attention3f(e2emv_ctx* ctx, int B, int T, int n_rows, const int* nv, int D, int H, const float* qkv, int cross,
                       float* out32, hipStream_t s) {
    Attn3fParams p;
    int n_valid;
    if (int rc = attn3f_params(ctx, "attention3f", B, T, n_rows, nv, D, H, qkv, cross, out32, &p, &n_valid)) return rc;
    hipLaunchKernelGGL(attention3f_kernel, dim3(8 * p.gper * p.nq), dim3(256), 0, s, p);
    E2EMV_CHECK_LAUNCH(ctx, "attention3f_kernel");
    return E2EMV_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// The first generation of the kernel, a tested building block no forward path reaches (e2emv_attention_bf16x3 without
// bit1): Q|K arrive as S3 planes [row][3][2D] (q pre-scaled by log2(e)/sqrt(d)), V arrives TRANSPOSED, [img][3][D][n_rows],
// both made by split_qkv_kernel (split3_api.hip).
struct Attn3Params : AttnShape {
    const uint16_t* qk;   // S3 [n_img*n_rows][3][2D]
    const uint16_t* vt;   // [n_img][3][D][n_rows]
    uint16_t* out;        // S3 [n_img*n_rows][3][D] or null
    float* out32;         // fp32 [n_img*n_rows][D] or null
};

__global__ __launch_bounds__(256, 2) void attention3_kernel(Attn3Params p) {
    __shared__ __attribute__((aligned(16))) uint16_t Ks[3 * A3_PLANE];
    __shared__ __attribute__((aligned(16))) uint16_t Vs[3 * A3_PLANE];

    const AttnItem it = attn_item(p, blockIdx.x, A3_Q);
    if (!it.live) return;
    const int qt = it.qt, img = it.img, head = it.head, b = it.b, t = it.t;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, lh = lane >> 5;
    const int64_t qk_ld = 2 * (int64_t)p.D;        // plane width of the q|k matrix
    const int64_t qk_row = 3 * qk_ld;              // bf16 per row

    // ---- Q fragments (B operand): lane (q, lh) holds Q_pl[q][16 s + 8 lh .. +7]
    const int q_row = qt * A3_Q + wave * 32 + l31;
    bf16x8 Qf[3][4];
    {
        const uint16_t* qp = p.qk + ((int64_t)img * p.n_rows + q_row) * qk_row + head * A3_HD + lh * 8;
#pragma unroll
        for (int pl = 0; pl < 3; ++pl)
#pragma unroll
            for (int s = 0; s < 4; ++s) Qf[pl][s] = *reinterpret_cast<const bf16x8*>(qp + pl * qk_ld + s * 16);
    }

    f32x16 O0, O1;
#pragma unroll
    for (int r = 0; r < 16; ++r) { O0[r] = 0.f; O1[r] = 0.f; }
    float m_run = -1e30f, l_run = 0.f;

    using Walk = AttnKeyWalk<A3_KV>;
    const Walk walk(p, t);
    const int n_tiles = walk.n_tiles;

    // staging: 6 x 16-byte chunks of K and of V^T per thread: chunk i -> plane i>>1, row tid/8 + 32*(i&1), chunk tid&7
    const int st_row = tid >> 3, st_ch = tid & 7;
    u32x4 rk[6], rv[6];
    auto gload = [&](const Walk::Pos& tp) {
        const int tt = walk.src(tp.si), kt = tp.kt;
        const int simg = b * p.T + tt;
        const uint16_t* kbase = p.qk + ((int64_t)simg * p.n_rows + kt * A3_KV) * qk_row + p.D + head * A3_HD + st_ch * 8;
        const uint16_t* vbase = p.vt + ((int64_t)simg * 3 * p.D + head * A3_HD) * p.n_rows + kt * A3_KV + st_ch * 8;
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            const int pl = i >> 1, row = st_row + 32 * (i & 1);
            rk[i] = *reinterpret_cast<const u32x4*>(kbase + (int64_t)row * qk_row + pl * qk_ld);
            rv[i] = *reinterpret_cast<const u32x4*>(vbase + ((int64_t)pl * p.D + row) * p.n_rows);
        }
    };
    // V^T LDS position of this thread's two 4-key halves (key order permuted inside 16-key groups)
    const int v_grp = st_ch >> 1, v_pos = 4 * (st_ch & 1);
    auto lstore = [&]() {
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            const int pl = i >> 1, row = st_row + 32 * (i & 1);
            *reinterpret_cast<u32x4*>(&Ks[pl * A3_PLANE + row * A3_LD + st_ch * 8]) = rk[i];
            uint16_t* vd = &Vs[pl * A3_PLANE + row * A3_LD + 16 * v_grp + v_pos];
            *reinterpret_cast<u32x2*>(vd) = u32x2{rv[i][0], rv[i][1]};
            *reinterpret_cast<u32x2*>(vd + 8) = u32x2{rv[i][2], rv[i][3]};
        }
    };

    constexpr int PA[6] = {2, 1, 0, 1, 0, 0};  // plane of the A operand (K or V^T), smallest terms first
    constexpr int PB[6] = {0, 1, 2, 0, 1, 0};  // plane of the B operand (Q or P)

    Walk::Pos cur{0, 0}, nxt{0, 0};
    gload(nxt);
    for (int tile = 0; tile < n_tiles; ++tile) {
        __syncthreads();
        lstore();
        __syncthreads();
        cur = nxt;
        if (tile + 1 < n_tiles) {
            walk.advance(nxt);
            gload(nxt);
        }
        const int valid_in_tile = walk.valid(cur);
#pragma unroll
        for (int sub = 0; sub < 2; ++sub) {
            if (sub * 32 >= valid_in_tile) break;
            f32x16 S;
#pragma unroll
            for (int r = 0; r < 16; ++r) S[r] = 0.f;
            const uint16_t* kp = &Ks[(sub * 32 + l31) * A3_LD + lh * 8];
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                bf16x8 kf[3];
#pragma unroll
                for (int pl = 0; pl < 3; ++pl) kf[pl] = *reinterpret_cast<const bf16x8*>(kp + pl * A3_PLANE + s * 16);
#pragma unroll
                for (int q = 0; q < 6; ++q) S = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf[PA[q]], Qf[PB[q]][s], S, 0, 0, 0);
            }
            if (valid_in_tile < sub * 32 + 32) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int key = sub * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                    if (key >= valid_in_tile) S[r] = -INFINITY;
                }
            }
            float mx = S[0];
#pragma unroll
            for (int r = 1; r < 16; ++r) mx = fmaxf(mx, S[r]);
            mx = fmaxf(mx, __shfl_xor(mx, 32));
            const float m_new = fmaxf(m_run, mx);
            const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
            float ps = 0.f;
            bf16x8 Pf[3][2];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float pv = __builtin_amdgcn_exp2f(S[r] - m_new);
                ps += pv;
                __bf16 a, bb, c;
                split3(pv, a, bb, c);
                Pf[0][r >> 3][r & 7] = a;
                Pf[1][r >> 3][r & 7] = bb;
                Pf[2][r >> 3][r & 7] = c;
            }
            l_run = l_run * alpha + ps;
            m_run = m_new;
#pragma unroll
            for (int r = 0; r < 16; ++r) { O0[r] *= alpha; O1[r] *= alpha; }
            // O^T[d][q] += V^T[d][keys] P^T[keys][q]; 16-key group index inside the tile = 2*sub + u
            const uint16_t* vp = &Vs[l31 * A3_LD + lh * 8];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                bf16x8 v0[3], v1[3];
#pragma unroll
                for (int pl = 0; pl < 3; ++pl) {
                    v0[pl] = *reinterpret_cast<const bf16x8*>(vp + pl * A3_PLANE + 16 * (2 * sub + u));
                    v1[pl] = *reinterpret_cast<const bf16x8*>(vp + pl * A3_PLANE + 32 * A3_LD + 16 * (2 * sub + u));
                }
#pragma unroll
                for (int q = 0; q < 6; ++q) {
                    O0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(v0[PA[q]], Pf[PB[q]][u], O0, 0, 0, 0);
                    O1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(v1[PA[q]], Pf[PB[q]][u], O1, 0, 0, 0);
                }
            }
        }
    }

    const float l_tot = l_run + __shfl_xor(l_run, 32);
    const float inv = 1.f / l_tot;
    if (p.out32) {
        float* op = p.out32 + ((int64_t)img * p.n_rows + q_row) * p.D + head * A3_HD + 4 * lh;
#pragma unroll
        for (int gq = 0; gq < 4; ++gq) {
            f32x4 a, c;
#pragma unroll
            for (int e = 0; e < 4; ++e) { a[e] = O0[gq * 4 + e] * inv; c[e] = O1[gq * 4 + e] * inv; }
            *reinterpret_cast<f32x4*>(op + 8 * gq) = a;
            *reinterpret_cast<f32x4*>(op + 32 + 8 * gq) = c;
        }
    }
    if (p.out) {
        uint16_t* op = p.out + ((int64_t)img * p.n_rows + q_row) * 3 * p.D + head * A3_HD + 4 * lh;
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
#pragma unroll
            for (int gq = 0; gq < 4; ++gq) {
                bf16x4 h0, h1, h2;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float v = (dt ? O1[gq * 4 + e] : O0[gq * 4 + e]) * inv;
                    __bf16 a, bb, c;
                    split3(v, a, bb, c);
                    h0[e] = a; h1[e] = bb; h2[e] = c;
                }
                uint16_t* dst = op + 32 * dt + 8 * gq;
                *reinterpret_cast<bf16x4*>(dst) = h0;
                *reinterpret_cast<bf16x4*>(dst + p.D) = h1;
                *reinterpret_cast<bf16x4*>(dst + 2 * p.D) = h2;
            }
    }
}

int launch_attention3(e2emv_ctx* ctx, int B, int T, int n_rows, const int* nv, int D, int H, const uint16_t* qk,
                      const uint16_t* vt, int cross, uint16_t* out3, float* out32, hipStream_t s) {
    Attn3Params p;
    int n_valid;
    if (int rc = attn_shape(ctx, "attention3", B, T, n_rows, nv, D, H, cross, A3_Q, &p, &n_valid)) return rc;
    p.qk = qk; p.vt = vt; p.out = out3; p.out32 = out32;
    hipLaunchKernelGGL(attention3_kernel, dim3(8 * p.gper * p.nq), dim3(256), 0, s, p);
    E2EMV_CHECK_LAUNCH(ctx, "attention3_kernel");
    return E2EMV_OK;
}

}  // namespace e2emv
