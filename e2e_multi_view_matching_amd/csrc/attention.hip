// Fused multi-head attention softmax(q k^T / sqrt(d)) v for the attentional GNN, fp32 on the
// gfx950 matrix cores, flash-style (the H x N x N_src probability tensor the reference
// materialises per layer - upstream superglue.py `attention()`, einsum 'bdhn,bdhm->bhnm' -
// never exists).  Self layers attend inside an image, cross layers to every other image of
// the tuple (N_src = (T-1) N; T = 2 is upstream SuperGlue's swap).
//
// Layout: qkv [n_img][n_rows][3D], channels head-major (c = h*64 + dd; the upstream order
// c = dd*H + h is undone on the weights at load time, weights.hip), image g = b*T + t.
//
// Per workgroup: one (image, head, 128-query tile); 4 waves x 32 queries.  Everything is
// computed TRANSPOSED so that each lane owns ONE query (q = lane & 31) for its whole life:
//   S^T[key][q] = mfma(A = K tile rows, B = Q)          -> a lane holds 16 keys of its query
//   O^T[d][q]  += mfma(A = V^T,           B = P^T)      -> the B operand of step t is exactly
// register t of the exponentiated S^T accumulator (MFMA 32x32 C layout: row = (r&3)+8(r>>2)
// +4(lane>>5)), so P never moves between lanes or through LDS, the running max/sum are
// per-lane scalars (+ one lane^32 exchange), and rescaling O^T is lane-local.
// K tiles sit in LDS padded to 68 floats (conflict-free ds_read_b128, one read feeds four
// MFMAs through the same K-slot permutation as gemm.hip); V tiles unpadded (ds_read_b32 of
// 32 consecutive floats).  128 MFMAs (8192 cycles) per wave per 64-key tile against ~1.3k
// VALU cycles of softmax: the kernel is MFMA-issue bound by construction.
#include <algorithm>
#include <cstdlib>

#include "attention_walk.h"
#include "common.h"

namespace e2emv {

typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) float f32x4;

constexpr int ATT_Q = 128;   // queries per workgroup
constexpr int ATT_KV = 64;   // keys per LDS tile
constexpr int HD = 64;       // head dim
constexpr int KLD = 68;      // padded K row (floats)

struct AttnParams : AttnShape {
    const float* qkv;
    float* out;
    // key-split mode (small problems): split sp of ksplit handles a slice of the key tiles and writes UNNORMALISED partial
    // outputs + (running max, sum) per query; attention_merge_kernel folds them
    int ksplit;
    float* part_o;   // [n_img][H][n_rows][ksplit][64]
    float* part_ml;  // [n_img][H][n_rows][ksplit][2]
};

template <bool SPLIT = false>
__global__ __launch_bounds__(256, 3) void attention_kernel(AttnParams p) {
    __shared__ __attribute__((aligned(16))) float Ks[ATT_KV * KLD];
    __shared__ __attribute__((aligned(16))) float Vs[ATT_KV * HD];

    // key split: the ksplit parts of an item are neighbours on its XCD
    const int lin = blockIdx.x;
    const int sp = SPLIT ? (lin >> 3) % p.ksplit : 0;
    const AttnItem it = attn_item(p, SPLIT ? ((lin >> 3) / p.ksplit) << 3 | (lin & 7) : lin, ATT_Q);
    if (!it.live) return;
    const int qt = it.qt, img = it.img, head = it.head, b = it.b, t = it.t;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, lh = lane >> 5;
    const int64_t row_stride = 3 * (int64_t)p.D;
    const int64_t img_stride = (int64_t)p.n_rows * row_stride;

    // ---- Q fragment: lane (q, lh) holds Q[q][8s + 4lh .. +3], pre-scaled by log2(e)/sqrt(d)
    const int q_row = qt * ATT_Q + wave * 32 + l31;
    const float qscale = 0.125f * 1.4426950408889634f;
    f32x4 Qr[8];
    {
        const float* qp = p.qkv + img * img_stride + (int64_t)q_row * row_stride + head * HD + lh * 4;
#pragma unroll
        for (int s = 0; s < 8; ++s) {
            f32x4 v = *reinterpret_cast<const f32x4*>(qp + s * 8);
            Qr[s] = v * qscale;
        }
    }

    f32x16 O0, O1;
#pragma unroll
    for (int r = 0; r < 16; ++r) { O0[r] = 0.f; O1[r] = 0.f; }
    float m_run = -1e30f, l_run = 0.f;

    using Walk = AttnKeyWalk<ATT_KV>;
    const Walk walk(p, t);
    const int n_tiles = walk.n_tiles;

    // staging map: 4 float4 of K and of V per thread
    const int st_row = tid >> 4;         // 0..15 (+16*i)
    const int st_c4 = (tid & 15) * 4;
    f32x4 rk[4], rv[4];
    auto gload = [&](const Walk::Pos& tp) {
        const int tt = walk.src(tp.si), kt = tp.kt;
        const float* base = p.qkv + (b * p.T + tt) * img_stride + (int64_t)(kt * ATT_KV) * row_stride + head * HD + st_c4;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float* rp = base + (int64_t)(st_row + 16 * i) * row_stride;
            rk[i] = *reinterpret_cast<const f32x4*>(rp + p.D);
            rv[i] = *reinterpret_cast<const f32x4*>(rp + 2 * p.D);
        }
    };

    const int tile_lo = SPLIT ? (int)((int64_t)n_tiles * sp / p.ksplit) : 0;
    const int tile_hi = SPLIT ? (int)((int64_t)n_tiles * (sp + 1) / p.ksplit) : n_tiles;
    Walk::Pos cur{0, 0}, nxt = SPLIT ? walk.at(tile_lo) : Walk::Pos{0, 0};
    if (tile_lo < tile_hi) gload(nxt);
    for (int tile = tile_lo; tile < tile_hi; ++tile) {
        __syncthreads();  // everyone is done reading the previous tile
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            *reinterpret_cast<f32x4*>(&Ks[(st_row + 16 * i) * KLD + st_c4]) = rk[i];
            *reinterpret_cast<f32x4*>(&Vs[(st_row + 16 * i) * HD + st_c4]) = rv[i];
        }
        __syncthreads();
        cur = nxt;
        if (tile + 1 < tile_hi) {
            walk.advance(nxt);
            gload(nxt);
        }
        const int valid_in_tile = walk.valid(cur);  // >= 1
#pragma unroll
        for (int sub = 0; sub < 2; ++sub) {
            if (sub * 32 >= valid_in_tile) break;  // wave-uniform
            f32x16 S;
#pragma unroll
            for (int r = 0; r < 16; ++r) S[r] = 0.f;
            const float* kp = &Ks[(sub * 32 + l31) * KLD + lh * 4];
#pragma unroll
            for (int s = 0; s < 8; ++s) {
                f32x4 kf = *reinterpret_cast<const f32x4*>(kp + s * 8);
#pragma unroll
                for (int e = 0; e < 4; ++e) S = __builtin_amdgcn_mfma_f32_32x32x2f32(kf[e], Qr[s][e], S, 0, 0, 0);
            }
            if (valid_in_tile < sub * 32 + 32) {  // ragged tail: mask keys >= n_valid
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
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                S[r] = __builtin_amdgcn_exp2f(S[r] - m_new);
                ps += S[r];
            }
            l_run = l_run * alpha + ps;
            m_run = m_new;
#pragma unroll
            for (int r = 0; r < 16; ++r) { O0[r] *= alpha; O1[r] *= alpha; }
            // O^T[d][q] += V^T[d][key] P^T[key][q]
            const float* vp = &Vs[(sub * 32 + 4 * lh) * HD + l31];
#pragma unroll
            for (int tt = 0; tt < 16; ++tt) {
                const int krow = (tt & 3) + 8 * (tt >> 2);
                const float v0 = vp[krow * HD];
                const float v1 = vp[krow * HD + 32];
                O0 = __builtin_amdgcn_mfma_f32_32x32x2f32(v0, S[tt], O0, 0, 0, 0);
                O1 = __builtin_amdgcn_mfma_f32_32x32x2f32(v1, S[tt], O1, 0, 0, 0);
            }
        }
    }

    const float l_tot = l_run + __shfl_xor(l_run, 32);
    if (SPLIT) {
        const int64_t slot = (((int64_t)img * p.H + head) * p.n_rows + q_row) * p.ksplit + sp;
        float* po = p.part_o + slot * HD + 4 * lh;
#pragma unroll
        for (int gq = 0; gq < 4; ++gq) {
            f32x4 a, c;
#pragma unroll
            for (int e = 0; e < 4; ++e) { a[e] = O0[gq * 4 + e]; c[e] = O1[gq * 4 + e]; }
            *reinterpret_cast<f32x4*>(po + 8 * gq) = a;
            *reinterpret_cast<f32x4*>(po + 32 + 8 * gq) = c;
        }
        if (lh == 0) { p.part_ml[slot * 2] = m_run; p.part_ml[slot * 2 + 1] = l_tot; }
        return;
    }
    // padding queries of the last tile get zeros, not the softmax of whatever their q rows hold (attention_merge_kernel leaves them unwritten)
    const bool pad = q_row >= p.nv[t];
    const float inv = 1.f / l_tot;
    float* op = p.out + ((int64_t)img * p.n_rows + q_row) * p.D + head * HD + 4 * lh;
#pragma unroll
    for (int gq = 0; gq < 4; ++gq) {
        f32x4 a, c;
#pragma unroll
        for (int e = 0; e < 4; ++e) { a[e] = pad ? 0.f : O0[gq * 4 + e] * inv; c[e] = pad ? 0.f : O1[gq * 4 + e] * inv; }
        *reinterpret_cast<f32x4*>(op + 8 * gq) = a;
        *reinterpret_cast<f32x4*>(op + 32 + 8 * gq) = c;
    }
}

// folds the key-split partials: out[q][:] = sum_s O_s 2^(m_s - M) / sum_s l_s 2^(m_s - M)
__global__ __launch_bounds__(256) void attention_merge_kernel(AttnParams p) {
    // one thread per (image, head, query, 4 channels)
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int c4 = (int)(i & 15);
    const int64_t rowi = i >> 4;  // (img * H + head) * n_rows + q
    if (rowi >= (int64_t)p.groups * p.n_rows) return;
    const int q = (int)(rowi % p.n_rows);
    const int gh = (int)(rowi / p.n_rows), img = gh / p.H, head = gh % p.H;
    if (q >= p.nv[img % p.T]) return;
    float M = -1e30f;
    for (int s2 = 0; s2 < p.ksplit; ++s2) M = fmaxf(M, p.part_ml[(rowi * p.ksplit + s2) * 2]);
    float L = 0.f;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int s2 = 0; s2 < p.ksplit; ++s2) {
        const float w = __builtin_amdgcn_exp2f(p.part_ml[(rowi * p.ksplit + s2) * 2] - M);
        L += p.part_ml[(rowi * p.ksplit + s2) * 2 + 1] * w;
        acc += *reinterpret_cast<const f32x4*>(p.part_o + (rowi * p.ksplit + s2) * HD + 4 * c4) * w;
    }
    *reinterpret_cast<f32x4*>(p.out + ((int64_t)img * p.n_rows + q) * p.D + head * HD + 4 * c4) = acc * (1.f / L);
}

int attn_shape(e2emv_ctx* ctx, const char* who, int B, int T, int n_rows, const int* nv, int D, int H, int cross, int q_tile,
               AttnShape* out, int* n_valid) {
    if (T < 1 || T > E2EMV_MAX_TUPLE) return set_err(ctx, E2EMV_EINVAL, "%s: T=%d images per tuple", who, T);
    int nmax = 0;
    for (int t = 0; t < T; ++t) {
        if (nv[t] <= 0 || nv[t] > n_rows) return set_err(ctx, E2EMV_ESHAPE, "%s: image %d has %d keypoints (n_rows %d)", who, t, nv[t], n_rows);
        nmax = std::max(nmax, nv[t]);
    }
    if (D != H * HD) return set_err(ctx, E2EMV_ESHAPE, "%s: head dim must be 64 (D=%d H=%d)", who, D, H);
    if (n_rows % q_tile || nmax <= 0 || nmax > n_rows)
        return set_err(ctx, E2EMV_ESHAPE, "%s: n_rows=%d must be a multiple of %d and >= n_valid=%d", who, n_rows, q_tile, nmax);
    if (cross && T < 2) return set_err(ctx, E2EMV_ESHAPE, "%s: cross layer needs T >= 2", who);
    out->B = B; out->T = T; out->n_rows = n_rows; out->D = D; out->H = H; out->cross = cross;
    for (int t = 0; t < E2EMV_MAX_TUPLE; ++t) out->nv[t] = t < T ? nv[t] : 0;
    out->nq = (nmax + q_tile - 1) / q_tile;
    out->groups = B * T * H;
    out->gper = (out->groups + 7) / 8;
    *n_valid = nmax;
    return E2EMV_OK;
}

int attn_min_tiles(const AttnShape& s, int KV) {
    int min_tiles = 1 << 30;
    for (int t = 0; t < s.T; ++t) {
        int n = 0;
        for (int u = 0; u < s.T; ++u)
            if (s.cross ? u != t : u == t) n += (s.nv[u] + KV - 1) / KV;
        min_tiles = std::min(min_tiles, n);
    }
    return min_tiles;
}

int launch_attention(e2emv_ctx* ctx, int B, int T, int n_rows, const int* nv, int D, int H, const float* qkv,
                     int cross, float* out, hipStream_t s) {
    AttnParams p;
    int n_valid;
    if (int rc = attn_shape(ctx, "attention", B, T, n_rows, nv, D, H, cross, ATT_Q, &p, &n_valid)) return rc;
    p.qkv = qkv; p.out = out;
    dim3 grid(8 * p.gper * p.nq);
    // Small problems (batch 1-2 of the reference's eval loop): one workgroup per (image, head, 128 queries) leaves most CUs
    // idle while each workgroup walks all key tiles serially.  Split the key tiles over up to 8 workgroups + a merge pass.
    p.ksplit = 1; p.part_o = nullptr; p.part_ml = nullptr;
    {
        const int min_tiles = attn_min_tiles(p, ATT_KV);
        const int blocks = p.groups * p.nq;
        int ks = blocks * 2 <= ctx->num_cus ? ctx->num_cus / blocks : 1;
        ks = std::max(1, std::min(std::min(ks, 8), min_tiles));
        if (ks > 1) {
            const size_t rows = (size_t)p.groups * n_rows * ks;
            const size_t need = rows * (HD + 2) * sizeof(float);
            if (ctx->attn_part_bytes < need) {
                E2EMV_HIP(ctx, hipStreamSynchronize(s));
                if (ctx->d_attn_part) E2EMV_HIP(ctx, hipFree(ctx->d_attn_part));
                ctx->d_attn_part = nullptr; ctx->attn_part_bytes = 0;
                E2EMV_HIP(ctx, hipMalloc(reinterpret_cast<void**>(&ctx->d_attn_part), need));
                ctx->attn_part_bytes = need;
            }
            p.ksplit = ks;
            p.part_o = ctx->d_attn_part;
            p.part_ml = ctx->d_attn_part + rows * HD;
            hipLaunchKernelGGL((attention_kernel<true>), dim3(8 * p.gper * p.nq * ks), dim3(256), 0, s, p);
            const int64_t threads = (int64_t)p.groups * n_rows * 16;
            hipLaunchKernelGGL(attention_merge_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, p);
            E2EMV_CHECK_LAUNCH(ctx, "attention_kernel (key-split)");
            return E2EMV_OK;
        }
    }
    hipLaunchKernelGGL(attention_kernel<>, grid, dim3(256), 0, s, p);
    E2EMV_CHECK_LAUNCH(ctx, "attention_kernel");
    return E2EMV_OK;
}

}  // namespace e2emv

static int attention_entry(e2emv_ctx* ctx, int B, int T, int n_rows, const int* nv, int D, int H, const float* d_qkv, int cross,
                           float* d_out, void* stream) {
    E2EMV_ENTER(ctx, stream);
    e2emv::prof_begin(ctx, e2emv::PS_ATTN, (hipStream_t)stream);
    int rc = e2emv::launch_attention(ctx, B, T, n_rows, nv, D, H, d_qkv, cross, d_out, (hipStream_t)stream);
    e2emv::prof_end(ctx, (hipStream_t)stream);
    return rc;
}

extern "C" int e2emv_attention(e2emv_ctx* ctx, int B, int T, int n_rows, int n_valid, int D, int H, const float* d_qkv,
                               int cross, float* d_out, void* stream) {
    if (!ctx || !d_qkv || !d_out) return E2EMV_EINVAL;
    if (T < 1 || T > E2EMV_MAX_TUPLE) return E2EMV_EINVAL;
    int nv[E2EMV_MAX_TUPLE];
    for (int t = 0; t < E2EMV_MAX_TUPLE; ++t) nv[t] = n_valid;
    return attention_entry(ctx, B, T, n_rows, nv, D, H, d_qkv, cross, d_out, stream);
}

extern "C" int e2emv_attention_v(e2emv_ctx* ctx, int B, int T, int n_rows, const int* n_valid_per_image, int D, int H,
                                 const float* d_qkv, int cross, float* d_out, void* stream) {
    if (!ctx || !d_qkv || !d_out || !n_valid_per_image) return E2EMV_EINVAL;
    if (T < 1 || T > E2EMV_MAX_TUPLE) return E2EMV_EINVAL;
    return attention_entry(ctx, B, T, n_rows, n_valid_per_image, D, H, d_qkv, cross, d_out, stream);
}
