// The front of the f16x2 plane forward behind ingest_kenc0 in ONE launch: layers 1..4 of the keypoint encoder {3, 32, 64, 128,
// 256, 256}, the descriptor residual and the conversion of x to scaled planes with tile exponents.  It replaces ingest_transpose
// (forward.hip), two gemm_nt launches (gemm.hip), two gemm_h2 launches (gemm_h2.hip) and to_planes_exp_kernel (p2_tools.hip),
// which pass every row-local operand through HBM (about 640 MB at 65 536 rows against 134 MB of compulsory traffic: descriptors
// in, planes out), and it computes what they compute BIT FOR BIT: every output element goes through the same instructions in
// the same order -
//   * layer 0 stays ingest_kenc0's launch, read here from its [rows][32] output (8 MB): how hipcc contracts and pairs up the
//     statement w0 kx + w1 ky + w2 ks + b depends on the code around it (in ingest_kenc0 even and odd channels come out with
//     different products fused), so a second copy of the statement in this kernel does not round like the first;
//   * 32 -> 64 and 64 -> 128: v_mfma_f32_32x32x2_f32 into a zero accumulator, k in gemm_nt_kernel's slot order (lanes 0-31
//     take k = 8c + e, lanes 32-63 k = 8c + 4 + e, c outer, e inner), then + bias, relu_nan;
//   * 128 -> 256 and 256 -> 256: gemm_h2_kernel's arithmetic - activations split per element into fp16 planes hi, lo' =
//     fp16(2^11 (x - hi)), the committed weight planes, 2^-11 w_hi made in registers, v_mfma_f32_32x32x16_f16 per 16 k with
//     lanes 0-31 on k..k+7 and 32-63 on k+8..k+15, products in the order x_hi w_lo, x_lo' (2^-11 w_hi), x_hi w_hi; then
//     acc 2^-s rounded on its own, + bias, relu_nan (first) / + descriptor (second);
//   * planes: to_planes_exp_kernel's block maximum (a maximum has no order), p2_pick_exponent, p2_split_scaled, p2_index.
//
// Shape.  A workgroup of 8 waves owns 128 keypoint rows of one image (n_rows % 128 == 0: a block never straddles images) and
// every activation of those rows stays in LDS or registers:
//   * wave w owns the 32 output columns [32 w, 32 w + 32) of the wide layers and all 128 rows: 4 accumulator tiles (64
//     registers), the activation fragments come from LDS (row stride K + 8 halves: conflict-free ds_read_b128);
//   * the weight fragments are read straight from global memory into registers (lane = weight row, 16 bytes of k): every
//     fragment is used by one wave only, so staging it in LDS would add a store and a load and share nothing.  The wide
//     layers' planes (393 KB) are streamed once per workgroup from L2, 200 MB per 65 536 rows (64-row blocks: 400 MB);
//   * 128 rows are what fits: the 256-wide hidden layer as planes takes 128 x 264 x 2 x 2 B = 132 KB of the CU's 160 KB, and
//     its region carries, before it is written, the 32-, 64- and 128-wide layers, and afterwards the output staging slabs;
//   * the descriptor residual needs no transpose: in the accumulator layout a lane owns a ROW and a register a column, so for
//     one register the lanes 0-31 read 32 consecutive keypoints of one descriptor channel of the caller's [B][D][N] tensor -
//     a contiguous 128-byte (fp16: 64-byte) run.  The loads are issued behind the last layer's K loop, whose weight
//     fragments need the registers until then;
//   * the planes leave through wave-private LDS slabs (64 rows x 128 B) so that a store instruction covers whole 128-byte
//     pieces of 8 rows instead of 8 bytes of 64 rows (gemm_h2.hip measured the latter at 23 % of a GEMM).
// One workgroup per CU (135 KB of LDS, 2 waves per SIMD); 65 536 rows are 512 workgroups, two rounds on 256 CUs.
#include <hip/hip_fp16.h>

#include "common.h"
#include "ingest.h"
#include "p2.h"

namespace e2emv {

typedef __attribute__((ext_vector_type(16))) float kf_f32x16;
typedef __attribute__((ext_vector_type(4))) float kf_f32x4;
typedef __attribute__((ext_vector_type(8))) _Float16 kf_f16x8;

constexpr int KF_ROWS = 128;                     // rows of a workgroup
constexpr int KF_C0 = 32, KF_C1 = 64, KF_C2 = 128, KF_C3 = 256, KF_D = 256;
constexpr int KF_LD0 = KF_C0 + 4, KF_LD1 = KF_C1 + 4;  // fp32 rows, + 16 B: conflict-free ds_read_b128 (gemm.hip)
constexpr int KF_LD2 = KF_C2 + 8, KF_LD3 = KF_C3 + 8;  // fp16 plane rows, + 16 B
constexpr int KF_PL2 = KF_ROWS * KF_LD2, KF_PL3 = KF_ROWS * KF_LD3;  // halves per plane
// LDS map (bytes).  [0, OFF_WMAX): the planes of the 256-wide layer; before they are written the same bytes hold the planes of
// the 128-wide layer and, behind them, the fp32 rows of the 32- (ingest_kenc0's output) and 64-wide layers; after the last K loop the output slabs.
constexpr int KF_OFF_H2 = 0;
constexpr int KF_OFF_H0 = KF_OFF_H2 + 2 * KF_PL2 * 2;
constexpr int KF_OFF_H1 = KF_OFF_H0 + KF_ROWS * KF_LD0 * 4;
constexpr int KF_OFF_H3 = 0;
constexpr int KF_OFF_WMAX = KF_OFF_H3 + 2 * KF_PL3 * 2;
constexpr int KF_SLAB_LD = 144;                  // bytes per slab row: 64 B hi + 64 B lo + 16
constexpr int KF_SLAB = 64 * KF_SLAB_LD;         // one wave's slab: a 64-row block of its 32 columns
constexpr int KF_LDS = KF_OFF_WMAX + 2 * 8 * 4;
static_assert(KF_OFF_H1 + KF_ROWS * KF_LD1 * 4 <= KF_OFF_WMAX && 8 * KF_SLAB <= KF_OFF_WMAX, "LDS regions overlap");

struct KencFusedParams {
    IngestParams in;
    const float *w1, *b1, *w2, *b2;  // 32 -> 64, 64 -> 128: fp32 [out][in]
    const uint16_t *wh3, *wh4;       // 128 -> 256, 256 -> 256: fp16 planes [out][{hi, lo}][in] of 2^s W
    const float *b3, *b4;
    float hs3, hs4;                  // 2^-s
    uint16_t* xp;
    int* e_x;
    float* a_x;
    unsigned* stats;                 // count of blocks with a non-zero exponent
};

// acc 2^-s as gemm_h2_kernel makes it: a product rounded on its own (there it passes through LDS before the bias is added;
// here the register is made opaque so that -ffp-contract cannot fuse the product into that addition)
__device__ __forceinline__ float kf_scaled(float acc, float hs) {
    float v = acc * hs;
    asm volatile("" : "+v"(v));
    return v;
}

// One fp32 layer tile: acc[i] (32 output channels x 32 rows each, NI row tiles) += W[32 channels][K] x X[rows][K]^T, gemm_nt_kernel's
// K order.  xs = &X[lane's row of tile 0][4 lh] in LDS (row stride LDX floats), wg = &W[lane's channel][4 lh] in global memory.
template <int K, int LDX, int NI>
__device__ __forceinline__ void kf_layer_f32(kf_f32x16 (&acc)[NI], const float* xs, const float* wg) {
    kf_f32x4 w[K / 8];  // the lane's whole weight row (K / 2 floats of it): every load in flight before the first MFMA
#pragma unroll
    for (int c = 0; c < K / 8; ++c) w[c] = *reinterpret_cast<const kf_f32x4*>(wg + c * 8);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int c = 0; c < K / 8; ++c) {
        const kf_f32x4 w0 = w[c];
        kf_f32x4 x[NI];
#pragma unroll
        for (int i = 0; i < NI; ++i) x[i] = *reinterpret_cast<const kf_f32x4*>(xs + i * 32 * LDX + c * 8);
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int i = 0; i < NI; ++i) acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(w0[e], x[i][e], acc[i], 0, 0, 0);
    }
}

// One f16x2 layer: acc[i] (this wave's 32 output channels x row tile i, 4 tiles = 128 rows) over K, gemm_h2_kernel's arithmetic.
// xs = &hi plane[lane's row of tile 0][8 lh] in LDS (row stride LDX halves, lo plane PL halves further), wg = &WH[lane's
// channel][hi][8 lh] in global memory (lo plane K halves further).
// A step of 16 k takes 32 bytes of a weight row per plane, a quarter of a cache line, and the eight waves of the CU touch 64 KB
// of lines per step - twice the vector L1: loaded step by step every line would come from L2 four times.  So the fragments of FOUR
// steps (whole 128-byte lines: 8 loads) are issued back to back, a group ahead of their use, into a second set of registers.
template <int K, int LDX, int PL>
__device__ __forceinline__ void kf_layer_h2(kf_f32x16 (&acc)[4], const uint16_t* xs, const uint16_t* wg) {
    constexpr int NG = K / 64;
    kf_f16x8 wq[2][4][2];
    auto gload = [&](int g) {
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            wq[g & 1][t][0] = *reinterpret_cast<const kf_f16x8*>(wg + (4 * g + t) * 16);
            wq[g & 1][t][1] = *reinterpret_cast<const kf_f16x8*>(wg + K + (4 * g + t) * 16);
        }
    };
    gload(0);
#pragma unroll
    for (int g = 0; g < NG; ++g) {
        if (g + 1 < NG) gload(g + 1);
        __builtin_amdgcn_sched_barrier(0);  // (the loads stay in front of the group's MFMAs)
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int s = 4 * g + t;
            kf_f16x8 w[3];
            w[0] = wq[g & 1][t][0];
            w[1] = wq[g & 1][t][1];
            w[2] = w[0] * (_Float16)(1.f / 2048.f);  // 2^-11 w_hi: exact
            kf_f16x8 x[4][2];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int pl = 0; pl < 2; ++pl) x[i][pl] = *reinterpret_cast<const kf_f16x8*>(xs + pl * PL + i * 32 * LDX + s * 16);
            constexpr int PW[3] = {1, 2, 0}, PX[3] = {0, 1, 0};  // x_hi w_lo, x_lo' (2^-11 w_hi), x_hi w_hi
#pragma unroll
            for (int q = 0; q < 3; ++q)
#pragma unroll
                for (int i = 0; i < 4; ++i) acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_f16(w[PW[q]], x[i][PX[q]], acc[i], 0, 0, 0);
        }
    }
}

template <int N>
__device__ __forceinline__ void kf_zero(kf_f32x16 (&acc)[N]) {
#pragma unroll
    for (int i = 0; i < N; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
}

// four consecutive columns of one row as scaled planes: 8 bytes to the hi plane at dst, 8 bytes to the lo plane `lo_off` halves further
__device__ __forceinline__ void kf_store_planes(uint16_t* dst, int lo_off, float v0, float v1, float v2, float v3) {
    const P2Pair a = p2_split_scaled(v0, v1), c = p2_split_scaled(v2, v3);
    *reinterpret_cast<p2_u32x2*>(dst) = p2_u32x2{a.hi, c.hi};
    *reinterpret_cast<p2_u32x2*>(dst + lo_off) = p2_u32x2{a.lo, c.lo};
}

__global__ __launch_bounds__(512, 1) void kenc_fused_kernel(KencFusedParams p) {
    extern __shared__ __attribute__((aligned(16))) char kf_smem[];
    float* h0 = reinterpret_cast<float*>(kf_smem + KF_OFF_H0);
    float* h1 = reinterpret_cast<float*>(kf_smem + KF_OFF_H1);
    uint16_t* h2 = reinterpret_cast<uint16_t*>(kf_smem + KF_OFF_H2);
    uint16_t* h3 = reinterpret_cast<uint16_t*>(kf_smem + KF_OFF_H3);
    float* wmax = reinterpret_cast<float*>(kf_smem + KF_OFF_WMAX);  // [2 row blocks][8 waves]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, lh = lane >> 5;
    const int row0 = blockIdx.x * KF_ROWS, img = blockIdx.y;
    const int b = img / p.in.T, t = img % p.in.T;
    const int Nn = p.in.Nimg[t];
    const int64_t grow0 = (int64_t)img * p.in.n_rows + row0;  // first row of the block in the activation matrices

    // ---- layer 0 as ingest_kenc0 left it: 128 rows x 32 floats, contiguous; thread = (row, 8 channels)
    {
        const int r = tid >> 2, c0 = (tid & 3) * 8;
        const float* src = p.in.h0 + (grow0 + r) * KF_C0 + c0;
        const kf_f32x4 o0 = *reinterpret_cast<const kf_f32x4*>(src), o1 = *reinterpret_cast<const kf_f32x4*>(src + 4);
        *reinterpret_cast<kf_f32x4*>(&h0[r * KF_LD0 + c0]) = o0;
        *reinterpret_cast<kf_f32x4*>(&h0[r * KF_LD0 + c0 + 4]) = o1;
    }
    __syncthreads();

    // ---- 32 -> 64: wave = (row tile, channel tile)
    {
        const int rt = wave >> 1, ct = wave & 1;
        kf_f32x16 acc[1];
        kf_zero(acc);
        kf_layer_f32<KF_C0, KF_LD0, 1>(acc, &h0[(rt * 32 + l31) * KF_LD0 + lh * 4], p.w1 + (ct * 32 + l31) * KF_C0 + lh * 4);
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int n = ct * 32 + 8 * g + 4 * lh;
            kf_f32x4 v = *reinterpret_cast<const kf_f32x4*>(p.b1 + n);
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = relu_nan(acc[0][4 * g + e] + v[e]);
            *reinterpret_cast<kf_f32x4*>(&h1[(rt * 32 + l31) * KF_LD1 + n]) = v;
        }
    }
    __syncthreads();

    // ---- 64 -> 128: wave = (row half, channel tile); the output leaves as the planes the next layer's split makes of it
    {
        const int rh = wave >> 2, ct = wave & 3;
        kf_f32x16 acc[2];
        kf_zero(acc);
        kf_layer_f32<KF_C1, KF_LD1, 2>(acc, &h1[(rh * 64 + l31) * KF_LD1 + lh * 4], p.w2 + (ct * 32 + l31) * KF_C1 + lh * 4);
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int n = ct * 32 + 8 * g + 4 * lh;
            const kf_f32x4 bias = *reinterpret_cast<const kf_f32x4*>(p.b2 + n);
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                float v[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = relu_nan(acc[i][4 * g + e] + bias[e]);
                kf_store_planes(&h2[(rh * 64 + i * 32 + l31) * KF_LD2 + n], KF_PL2, v[0], v[1], v[2], v[3]);
            }
        }
    }
    __syncthreads();

    const int n0 = wave * 32;  // this wave's columns of the wide layers
    kf_f32x16 acc[4];

    // ---- 128 -> 256
    kf_zero(acc);
    kf_layer_h2<KF_C2, KF_LD2, KF_PL2>(acc, &h2[l31 * KF_LD2 + lh * 8], p.wh3 + (n0 + l31) * 2 * KF_C2 + lh * 8);
    __syncthreads();  // every wave has read the 128-wide planes: their bytes become the 256-wide ones
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const int n = n0 + 8 * g + 4 * lh;
        const kf_f32x4 bias = *reinterpret_cast<const kf_f32x4*>(p.b3 + n);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            float v[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = relu_nan(kf_scaled(acc[i][4 * g + e], p.hs3) + bias[e]);
            kf_store_planes(&h3[(i * 32 + l31) * KF_LD3 + n], KF_PL3, v[0], v[1], v[2], v[3]);
        }
    }
    __syncthreads();

    // ---- 256 -> 256, + bias, + descriptor: x
    kf_zero(acc);
    kf_layer_h2<KF_C3, KF_LD3, KF_PL3>(acc, &h3[l31 * KF_LD3 + lh * 8], p.wh4 + (n0 + l31) * 2 * KF_C3 + lh * 8);

    // ---- the residual: descriptor channel n0 + 8 g + 4 lh + e of keypoint row0 + 32 i + l31, in the accumulator layout; 0 beyond N
    float res[4][16];
    {
        const int64_t img_base = (int64_t)b * p.in.D * Nn;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int n = row0 + i * 32 + l31;
            const bool ok = n < Nn;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int d = n0 + 8 * (r >> 2) + 4 * lh + (r & 3);
                const int64_t o = img_base + (int64_t)d * Nn + n;
                float v = 0.f;
                if (ok) v = p.in.f16 ? __half2float(reinterpret_cast<const __half*>(p.in.desc[t])[o]) : reinterpret_cast<const float*>(p.in.desc[t])[o];
                res[i][r] = v;
            }
        }
    }
    float am[2] = {0.f, 0.f};  // max |x| of this wave's part of the two 64-row blocks
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const kf_f32x4 bias = *reinterpret_cast<const kf_f32x4*>(p.b4 + n0 + 8 * g + 4 * lh);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float v = (kf_scaled(acc[i][4 * g + e], p.hs4) + bias[e]) + res[i][4 * g + e];
                acc[i][4 * g + e] = v;
                am[i >> 1] = fmaxf(am[i >> 1], fabsf(v));
            }
    }
#pragma unroll
    for (int rb = 0; rb < 2; ++rb) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) am[rb] = fmaxf(am[rb], __shfl_xor(am[rb], o));
        if (lane == 0) wmax[rb * 8 + wave] = am[rb];
    }
    __syncthreads();  // the maxima are in place, and every wave has read the 256-wide planes: their bytes become the slabs

    // ---- planes of x: per 64-row block the exponent of the 64 x 64 block this wave shares with its neighbour, split, out through the slab
    char* slab = kf_smem + wave * KF_SLAB;
#pragma unroll
    for (int rb = 0; rb < 2; ++rb) {
        const float bm = fmaxf(wmax[rb * 8 + wave], wmax[rb * 8 + (wave ^ 1)]);
        const int ex = p2_pick_exponent(bm);
        const float f = p2_exp2i(-ex);
        if ((wave & 1) == 0 && lane == 0) {
            const int64_t eb = (grow0 / 64 + rb) * (KF_D / 64) + (wave >> 1);
            p.e_x[eb] = ex;
            p.a_x[eb] = bm;
            if (ex != 0) atomicAdd(p.stats, 1u);
        }
#pragma unroll
        for (int ii = 0; ii < 2; ++ii) {
            const int i = rb * 2 + ii;
#pragma unroll
            for (int g = 0; g < 4; ++g)
                kf_store_planes(reinterpret_cast<uint16_t*>(slab + (ii * 32 + l31) * KF_SLAB_LD) + 8 * g + 4 * lh, 32, acc[i][4 * g] * f,
                                acc[i][4 * g + 1] * f, acc[i][4 * g + 2] * f, acc[i][4 * g + 3] * f);
        }
        // row m of the P2 matrix: 2 D halves; this wave's 32-column block = the 128 bytes at half 64 wave (p2_index)
        char* dst = reinterpret_cast<char*>(p.xp + p2_index(grow0 + rb * 64, n0, KF_D));
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int r = k * 8 + (lane >> 3), ch = lane & 7;
            const p2_u32x4 v = *reinterpret_cast<const p2_u32x4*>(slab + r * KF_SLAB_LD + ch * 16);
            *reinterpret_cast<p2_u32x4*>(dst + (int64_t)r * (2 * KF_D * 2) + ch * 16) = v;
        }
    }
}

int launch_kenc_fused(e2emv_ctx* ctx, const IngestParams& in, const DenseWeights* kenc, uint16_t* xp, int* e_x, float* a_x, hipStream_t s) {
    const DenseWeights &l1 = kenc[0], &l2 = kenc[1], &l3 = kenc[2], &l4 = kenc[3];
    if (in.c0 != KF_C0 || in.D != KF_D || l1.in != KF_C0 || l1.out != KF_C1 || l2.in != KF_C1 || l2.out != KF_C2 || l3.in != KF_C2 || l3.out != KF_C3 ||
        l4.in != KF_C3 || l4.out != KF_D || !l3.wh || !l4.wh)
        return set_err(ctx, E2EMV_ESHAPE, "kenc_fused: the keypoint encoder is not {3, 32, 64, 128, 256, 256} with fp16 x 2 planes of the wide layers");
    if (in.n_rows <= 0 || in.n_rows % KF_ROWS || in.B <= 0 || in.T <= 0 || in.T > E2EMV_MAX_TUPLE)
        return set_err(ctx, E2EMV_ESHAPE, "kenc_fused: n_rows=%d must be a multiple of %d", in.n_rows, KF_ROWS);
    for (int t = 0; t < in.T; ++t)
        if (in.Nimg[t] <= 0 || in.Nimg[t] > in.n_rows) return set_err(ctx, E2EMV_ESHAPE, "kenc_fused: image %d has %d keypoints (n_rows %d)", t, in.Nimg[t], in.n_rows);
    const uintptr_t al = (uintptr_t)l1.w | (uintptr_t)l1.b | (uintptr_t)l2.w | (uintptr_t)l2.b | (uintptr_t)l3.wh | (uintptr_t)l3.b | (uintptr_t)l4.wh |
                         (uintptr_t)l4.b | (uintptr_t)xp;
    if (al % 16 || !in.h0 || (uintptr_t)in.h0 % 16 || !l1.w || !l1.b || !l2.w || !l2.b || !l3.b || !l4.b || !xp || !e_x || !a_x)
        return set_err(ctx, E2EMV_ESHAPE, "kenc_fused: weights, biases and the plane output must be 16-byte aligned");
    if (int rc = ensure_flags(ctx)) return rc;
    KencFusedParams p;
    p.in = in;
    p.w1 = l1.w; p.b1 = l1.b; p.w2 = l2.w; p.b2 = l2.b;
    p.wh3 = l3.wh; p.b3 = l3.b; p.hs3 = l3.hs; p.wh4 = l4.wh; p.b4 = l4.b; p.hs4 = l4.hs;
    p.xp = xp; p.e_x = e_x; p.a_x = a_x; p.stats = ctx->d_flags + 2;
    const void* fn = reinterpret_cast<const void*>(kenc_fused_kernel);
    if (int rc = ensure_dynamic_lds(ctx, fn, KF_LDS)) return rc;
    void* args[] = {&p};
    E2EMV_HIP(ctx, hipLaunchKernel(fn, dim3(in.n_rows / KF_ROWS, in.B * in.T), dim3(512), args, KF_LDS, s));
    E2EMV_CHECK_LAUNCH(ctx, "kenc_fused_kernel");
    ++ctx->stat_kenc_fused;
    return E2EMV_OK;
}

}  // namespace e2emv
