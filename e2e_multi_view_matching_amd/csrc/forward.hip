// e2emv_matcher_forward: the MultiViewMatcher.forward replacement (reference call sites
// helpers.py:246, eval_pairs.py:212, eval_multi_view.py:160; algorithm = upstream SuperGlue
// superglue.py SuperGlue.forward, see oracle/matcher.py for the restated spec).
//
//   ingest (descriptor transpose [B,D,N] -> [img][row][D], keypoint normalisation + first
//   keypoint-encoder layer)  ->  kenc MLP (MFMA GEMMs, last one adds the descriptors)
//   -> L x { q|k|v GEMM, fused attention, merge GEMM, MLP0 GEMM (+BN folded, ReLU) over the
//   un-materialised concat [x | message], MLP1 GEMM + residual }  -> final_proj GEMM
//   -> per pair: score GEMM (1/sqrt(D) fused) -> one-sweep Sinkhorn -> match block -> conf head.
//
// HBM layout: image g = b*T + t owns n_rows = round_up(N,128) rows of D contiguous channels
// in every activation buffer, so every GEMM sees one [B*T*n_rows] x D matrix, keys/queries of
// one image are contiguous, and a tuple's images are adjacent (cross-attention sources).
// Rows >= N are zeroed at ingest and stay finite; attention masks them as keys.
#include <hip/hip_fp16.h>

#include <algorithm>

#include "common.h"
#include "ingest.h"
#include "p2.h"

namespace e2emv {

typedef __attribute__((ext_vector_type(4))) float f32x4;

// [B][D][N] (N contiguous) -> [img][n_rows][D] (D contiguous); rows >= N := 0
__global__ __launch_bounds__(256) void ingest_transpose(IngestParams p) {
    __shared__ float tile[64][65];
    const int n0 = blockIdx.x * 64, d0 = blockIdx.y * 64, img = blockIdx.z;
    const int b = img / p.T, t = img % p.T;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int n = n0 + tx;
    for (int dd = ty; dd < 64; dd += 4) {
        float v = 0.f;
        if (n < p.Nimg[t]) {
            const int64_t o = ((int64_t)b * p.D + d0 + dd) * p.Nimg[t] + n;
            v = p.f16 ? __half2float(reinterpret_cast<const __half*>(p.desc[t])[o])
                      : reinterpret_cast<const float*>(p.desc[t])[o];
        }
        tile[dd][tx] = v;
    }
    __syncthreads();
    for (int nn = ty; nn < 64; nn += 4)
        p.x0[((int64_t)img * p.n_rows + n0 + nn) * p.D + d0 + tx] = tile[tx][nn];
}

// keypoint normalisation + kenc layer 0 (3 -> c0, BN folded, ReLU); rows >= N := 0
__global__ __launch_bounds__(256) void ingest_kenc0(IngestParams p) {
    const int row = blockIdx.x * 256 + threadIdx.x, img = blockIdx.y;
    if (row >= p.n_rows) return;
    const int b = img / p.T, t = img % p.T;
    float* out = p.h0 + ((int64_t)img * p.n_rows + row) * p.c0;
    const int Nn = p.Nimg[t];
    if (row >= Nn) {
        for (int c = 0; c < p.c0; c += 4) *reinterpret_cast<f32x4*>(out + c) = f32x4{0.f, 0.f, 0.f, 0.f};
        return;
    }
    const float W = p.img_w[t], H = p.img_h[t];
    const float sc = fmaxf(W, H) * 0.7f;
    const float kx = (p.kpts[t][((int64_t)b * Nn + row) * 2] - W / 2) / sc;
    const float ky = (p.kpts[t][((int64_t)b * Nn + row) * 2 + 1] - H / 2) / sc;
    const float ks = p.ksc[t][(int64_t)b * Nn + row];
    if (p.inp) *reinterpret_cast<f32x4*>(p.inp + ((int64_t)img * p.n_rows + row) * 4) = f32x4{kx, ky, ks, 0.f};
    for (int c = 0; c < p.c0; c += 4) {
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float* w = p.w0 + (c + e) * 3;
            o[e] = relu_nan(w[0] * kx + w[1] * ky + w[2] * ks + p.b0[c + e]);
        }
        *reinterpret_cast<f32x4*>(out + c) = o;
    }
}

// conf head, step 1: feat2[b][n][:] = mdesc_j[b][max(match,0)][:]
__global__ __launch_bounds__(256) void conf_gather_kernel(int N, int n_rows, int D, const float* mdesc_j, int64_t tuple_stride,
                                                          const int64_t* matches, float* out) {
    const int b = blockIdx.y;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= n_rows) return;
    int64_t j = row < N ? matches[(int64_t)b * N + row] : 0;
    if (j < 0) j = 0;
    const float* src = mdesc_j + b * tuple_stride + j * D;
    float* dst = out + ((int64_t)b * n_rows + row) * D;
    for (int c = lane * 4; c < D; c += 256) *reinterpret_cast<f32x4*>(dst + c) = *reinterpret_cast<const f32x4*>(src + c);
}

// f16x2 mode: both halves of the conf MLP's input in one matrix, feat[b][n][:] = [mdesc_i[b][n][:] | mdesc_j[b][max(match,0)][:]]
// (the fp16 x 2 GEMM takes one un-batched row-major operand)
__global__ __launch_bounds__(256) void conf_gather2_kernel(int N, int n_rows, int D, const float* mdesc_i, const float* mdesc_j, int64_t tuple_stride,
                                                           const int64_t* matches, float* out) {
    const int b = blockIdx.y;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= n_rows) return;
    int64_t j = row < N ? matches[(int64_t)b * N + row] : 0;
    if (j < 0) j = 0;
    const float* si = mdesc_i + b * tuple_stride + (int64_t)row * D;
    const float* sj = mdesc_j + b * tuple_stride + j * D;
    float* dst = out + ((int64_t)b * n_rows + row) * 2 * D;
    for (int c = lane * 4; c < D; c += 256) {
        *reinterpret_cast<f32x4*>(dst + c) = *reinterpret_cast<const f32x4*>(si + c);
        *reinterpret_cast<f32x4*>(dst + D + c) = *reinterpret_cast<const f32x4*>(sj + c);
    }
}

// conf head, last step: sigmoid(<hidden, w> + b) for matched keypoints, 0 otherwise;
// without conf_mlp the confidence is the match score (reference quirk E13)
__global__ __launch_bounds__(256) void conf_final_kernel(int N, int n_rows, int D, const float* hidden, const float* w, float bias,
                                                         const int64_t* matches, const float* mscores, int use_mlp, float* conf) {
    const int b = blockIdx.y;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= N) return;
    const bool valid = matches[(int64_t)b * N + row] >= 0;
    float r = 0.f;
    if (use_mlp) {
        const float* h = hidden + ((int64_t)b * n_rows + row) * D;
        float acc = 0.f;
        for (int c = lane * 4; c < D; c += 256) {
            f32x4 hv = *reinterpret_cast<const f32x4*>(h + c), wv = *reinterpret_cast<const f32x4*>(w + c);
            acc += hv[0] * wv[0] + hv[1] * wv[1] + hv[2] * wv[2] + hv[3] * wv[3];
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
        r = 1.f / (1.f + __expf(-(acc + bias)));
    } else {
        r = mscores[(int64_t)b * N + row];
    }
    if (lane == 0) conf[(int64_t)b * N + row] = valid ? r : 0.f;
}

static int round_up(int x, int m) { return (x + m - 1) / m * m; }

// arithmetic of the GNN's dense contractions in one forward call
enum class FwdMode {
    F32,           // fp32-MFMA kernels
    BF16X3,        // fp32 activations, split into three bf16 planes in the consumer (gemm_x3.hip, attention_x3.hip)
    F16X2,         // fp32 activations, split into two fp16 planes in the consumer (gemm_h2.hip, attention_h2f)
    F16X2_PLANES,  // activations stored as two fp16 planes (p2.h; gemm_p2.hip, gemm_p2c.hip, attention_p2.hip)
};

// what a forward call derives before its first launch: shapes, arithmetic and the carved workspace (plan_forward)
struct FwdPlan {
    int B, T, D, H;
    int Nt[E2EMV_MAX_TUPLE];  // per-image keypoint counts (eval_pairs.py feeds images with different numbers of keypoints)
    int N, n_rows, P, ldS;    // the largest count, rows per image in the activation buffers, pairs per tuple, score stride
    bool uniform, full;       // every image has N keypoints; E2EMV_FLAG_FULL_OUTPUT
    int64_t Mtot;             // rows of an activation buffer
    FwdMode mode;
    bool kenc_fused;          // F16X2_PLANES: ingest, keypoint encoder and the plane conversion of x in one launch (kenc_fused.hip)
    bool chain;               // F16X2_PLANES: MLP0, MLP1 and the next q | k | v (or final_proj) in one launch (gemm_p2c.hip)
    float *x, *att, *msg, *qkv, *hid, *S;
    char* skws;
    int *e_x, *e_att, *e_qk, *e_vt, *e_hid;
    float* a_x;
    int64_t* tmp_m0[kMaxGroups];
    float* tmp_ms0[kMaxGroups];
    bool f16x2() const { return mode == FwdMode::F16X2 || mode == FwdMode::F16X2_PLANES; }
};

}  // namespace e2emv

using namespace e2emv;

static int plan_forward(e2emv_ctx* ctx, const e2emv_forward_desc* fd, FwdPlan& p) {
    p = FwdPlan{};
    const int B = p.B = fd->batch, T = p.T = fd->tuple_size;
    const int D = p.D = ctx->model.desc_dim, H = p.H = ctx->model.num_heads;
    for (int t = 0; t < T; ++t) p.Nt[t] = fd->n_kpts_img[t] > 0 ? fd->n_kpts_img[t] : fd->n_kpts;
    const int N = p.N = *std::max_element(p.Nt, p.Nt + T);
    p.uniform = std::count(p.Nt, p.Nt + T, N) == T;
    p.n_rows = round_up(N, 128);
    const int64_t Mtot = p.Mtot = (int64_t)(B * T) * p.n_rows;
    const int P = p.P = T * (T - 1) / 2;
    const int ldS = p.ldS = round_up(N, 4);  // allocation stride; a pair (i, j) uses ld = round_up(N_j, 4)
    p.full = (fd->flags & E2EMV_FLAG_FULL_OUTPUT) != 0;

    // bf16x3 (split operands on the bf16 pipe) pays once the 128-row GEMM tiles fill the chip; calls below half a tile per
    // CU (a pair or two - the eval_pairs.py loop) run the fp32-MFMA kernels, whose 64 x 64 tile shape and key-split
    // attention are the latency-tuned forms.  Both arithmetic modes meet the same parity bar.
    const int64_t split_min = ctx->split_min_rows >= 0 ? ctx->split_min_rows : (int64_t)128 * (ctx->num_cus / 2);
    // f16x2 on PLANE activations: every producer epilogue emits the two fp16 planes, consumers load them straight into LDS.
    // Their operands are addressed with 32-bit byte offsets: the widest plane matrices, q | k and the hidden layer, are
    // Mtot x 2D x 4 bytes - beyond 2 GB, 2^20 rows at D = 256, the call runs on fp32 activations, split in the consumer.
    const bool planes = D == 256 && H == 4 && !ctx->layers.empty() && Mtot * 8 * D < ((int64_t)1 << 31);
    if (ctx->precision == E2EMV_PRECISION_F32 || Mtot < split_min) p.mode = FwdMode::F32;
    else if (ctx->precision != E2EMV_PRECISION_F16X2) p.mode = FwdMode::BF16X3;
    else p.mode = planes ? FwdMode::F16X2_PLANES : FwdMode::F16X2;

    // the front of the plane path in one launch: the encoder widths that kernel is written for, its wide layers with their fp16 x 2
    // planes (the forward's ingest never records the training tape's `inp`); every other call runs the launch per stage
    static const int kFusedDims[6] = {3, 32, 64, 128, 256, 256};
    const std::vector<int>& kd = ctx->kenc_dims;
    p.kenc_fused = p.mode == FwdMode::F16X2_PLANES && ctx->kenc_fused && kd.size() == 6 && std::equal(kd.begin(), kd.end(), kFusedDims) &&
                   ctx->kenc.size() == 4 && ctx->kenc[2].wh && ctx->kenc[3].wh;

    // f16x2 kernel generation 5: the row-local GEMMs between two attentions - MLP0, MLP1 of layer l and q | k | v of layer l + 1
    // (final_proj behind the last layer) - chained per 256-row block in ONE launch (gemm_p2c.hip).  A workgroup then walks 6 tiles
    // where the three launches walk ceil(2 rb / CUs) + ceil(rb / CUs) + ceil(3 rb / CUs) (rb = row blocks): chained when that is
    // not more (configs[1]: 256 row blocks on 256 CUs, 6 = 6, and 36 launches fewer per forward; T = 5 shapes with 160 / 320 row
    // blocks keep the three launches).  e2emv_set_f16x2_kernels: 4 = never, 105 = whenever the shapes allow.
    const int64_t rb = Mtot / 256, cu = std::max(1, ctx->num_cus);
    auto rounds = [&](int64_t tiles) { return (tiles + cu - 1) / cu; };
    p.chain = p.mode == FwdMode::F16X2_PLANES && ctx->gemm_chain && Mtot % 256 == 0 &&
              (ctx->gemm_chain == 2 || 6 * rounds(rb) <= rounds(2 * rb) + rounds(rb) + rounds(3 * rb));

    auto al = [](size_t bytes) { return (bytes + 255) & ~size_t(255); };
    const size_t sz_x = al((size_t)Mtot * D * 4), sz_qkv = al((size_t)Mtot * 3 * D * 4), sz_hid = al((size_t)Mtot * 2 * D * 4);
    const size_t sz_S = al((size_t)P * B * N * ldS * 4);
    const size_t sz_sk = sinkhorn_ws_bytes(P * B, N, N);
    const size_t sz_match = p.full ? (size_t)P * (al((size_t)B * N * 8) + al((size_t)B * N * 4)) : 0;
    // tile exponents of the plane tensors (p2.h): one int per 64 rows x 64 columns of x (4), attention output (4), q|k (8),
    // V^T (4), hidden (8)
    const size_t sz_e = p.mode == FwdMode::F16X2_PLANES ? al((size_t)(Mtot / 64) * 32 * sizeof(int)) : 0;  // + max |x| per block (4 floats)
    const size_t need = sz_x * 3 + sz_qkv + sz_hid + sz_S + sz_sk + sz_match + sz_e + 4096;
    if (int rc = ws_reserve(ctx, need)) return rc;
    char* w = ctx->d_ws;
    p.x = (float*)w; w += sz_x;
    p.att = (float*)w; w += sz_x;    // attention output, later mdesc
    p.msg = (float*)w; w += sz_x;    // x as planes (F16X2_PLANES), later conf gather / hidden
    p.qkv = (float*)w; w += sz_qkv;
    p.hid = (float*)w; w += sz_hid;
    p.S = (float*)w; w += sz_S;
    p.skws = w; w += sz_sk;
    p.e_x = (int*)w; w += sz_e;
    p.e_att = p.e_x + (Mtot / 64) * 4;
    p.e_qk = p.e_att + (Mtot / 64) * 4;
    p.e_vt = p.e_qk + (Mtot / 64) * 8;
    p.e_hid = p.e_vt + (Mtot / 64) * 4;
    p.a_x = (float*)(p.e_hid + (Mtot / 64) * 8);  // max |x| of the blocks: the residual's share of the bound that picks x's next exponent
    if (p.full)  // (matches0 / mscores0 of the pairs whose conf head needs them when the caller does not)
        for (int q = 0; q < P; ++q) {
            p.tmp_m0[q] = (int64_t*)w; w += al((size_t)B * N * 8);
            p.tmp_ms0[q] = (float*)w; w += al((size_t)B * N * 4);
        }
    return E2EMV_OK;
}

// The weight side of a GEMM over M rows with the dense layer w, one K segment: on fp32 activations ...
static GemmArgs dense_gemm(const DenseWeights& w, int M) {
    GemmArgs g;
    g.M = M; g.N = w.out; g.K = w.in; g.K1 = w.in; g.W = w.w; g.ldw = w.in; g.bias = w.b;
    return g;
}
// ... and on planes
static GemmP2Args dense_gemm_p2(const DenseWeights& w, int M) {
    GemmP2Args g;
    g.M = M; g.N = w.out; g.K = w.in; g.K1 = w.in; g.W = w.wp; g.out_scale = w.hs; g.bias = w.b; g.bias_amax = w.ba;
    return g;
}

// A GEMM on fp32 activations in the plan's arithmetic (profile slot "gemm"); g = dense_gemm(w) and the activation side.  Where
// the mode's form of the weights is null the fp32 kernel runs.
static int gemm_fp32_act(e2emv_ctx* ctx, const FwdPlan& p, const GemmArgs& g, const DenseWeights& w, hipStream_t s) {
    prof_begin(ctx, PS_GEMM, s);
    int rc;
    if (p.f16x2() && w.wh) rc = launch_gemm_h2(ctx, g, w.wh, g.K, w.hs, s);
    else if (p.mode == FwdMode::BF16X3 && w.w3) rc = launch_gemm_x3(ctx, g, w.w3, g.K, s);
    else rc = launch_gemm_nt(ctx, g, s);
    prof_end(ctx, s);
    return rc;
}

// the caller's inputs and layer 0 of the keypoint encoder as the ingest kernels take them
static IngestParams ingest_params(e2emv_ctx* ctx, const FwdPlan& p, const e2emv_forward_desc* fd, const float* const* d_kpts,
                                  const float* const* d_kscores, const void* const* d_desc) {
    IngestParams ip{};
    for (int t = 0; t < p.T; ++t) {
        ip.kpts[t] = d_kpts[t]; ip.ksc[t] = d_kscores[t]; ip.desc[t] = d_desc[t];
        ip.img_w[t] = fd->img_w[t]; ip.img_h[t] = fd->img_h[t]; ip.Nimg[t] = p.Nt[t];
    }
    ip.B = p.B; ip.T = p.T; ip.n_rows = p.n_rows; ip.D = p.D; ip.c0 = ctx->kenc_dims[1]; ip.f16 = fd->desc_dtype == E2EMV_DESC_F16;
    ip.w0 = ctx->kenc_w0; ip.b0 = ctx->kenc_b0;
    return ip;
}

// ingest, then keypoint encoder layers 1..n through the GEMM; the last adds the descriptors: x = the GNN's input
static int encode(e2emv_ctx* ctx, const FwdPlan& p, const e2emv_forward_desc* fd, const float* const* d_kpts,
                  const float* const* d_kscores, const void* const* d_desc, hipStream_t s) {
    const std::vector<int>& kd = ctx->kenc_dims;  // [3, c0, ..., D]
    const int c0 = kd[1];
    int64_t tot = 0;
    for (size_t i = 1; i + 1 < kd.size(); ++i) tot += kd[i];
    if (tot > 2 * p.D) return set_err(ctx, E2EMV_ESHAPE, "keypoint_encoder too wide for the workspace plan");
    IngestParams ip = ingest_params(ctx, p, fd, d_kpts, d_kscores, d_desc);
    ip.x0 = p.x; ip.h0 = p.hid;
    prof_begin(ctx, PS_INGEST, s);
    hipLaunchKernelGGL(ingest_transpose, dim3(p.n_rows / 64, p.D / 64, p.B * p.T), dim3(256), 0, s, ip);
    hipLaunchKernelGGL(ingest_kenc0, dim3((p.n_rows + 255) / 256, p.B * p.T), dim3(256), 0, s, ip);
    prof_end(ctx, s);
    E2EMV_CHECK_LAUNCH(ctx, "ingest kernels");

    float* cur = p.hid;  // [Mtot][c0]
    float* nxt = p.hid + p.Mtot * c0;
    for (const DenseWeights& w : ctx->kenc) {
        const bool last = &w == &ctx->kenc.back();
        GemmArgs g = dense_gemm(w, (int)p.Mtot);
        g.A = cur; g.lda = w.in;
        g.relu = !last;
        if (last) { g.R = p.x; g.ldr = p.D; g.C = p.x; g.ldc = p.D; }
        else { g.C = nxt; g.ldc = w.out; }
        // no bf16x3 planes; f16x2 mode: the wide layers (fan-in >= 128) on the fp16 x 2 kernel as well - same parity bar, 3x less
        // matrix-core time
        if (int rc = gemm_fp32_act(ctx, p, g, w, s)) return rc;
        cur = nxt;
        nxt = nxt + p.Mtot * w.out;
    }
    return E2EMV_OK;
}

// F32, BF16X3 and F16X2: the GNN layers and final_proj (mdesc = att) on fp32 activations
static int gnn_fp32_activations(e2emv_ctx* ctx, const FwdPlan& p, hipStream_t s) {
    const int D = p.D, M = (int)p.Mtot;
    for (const LayerWeights& L : ctx->layers) {
        // q|k|v = x Wqkv^T + b; the split modes' attention kernels split Q / K / V^T into planes on the way in
        GemmArgs g = dense_gemm(L.qkv, M);
        g.A = p.x; g.lda = D; g.C = p.qkv; g.ldc = 3 * D;
        int rc;
        if ((rc = gemm_fp32_act(ctx, p, g, L.qkv, s))) return rc;
        prof_begin(ctx, PS_ATTN, s);
        if (p.mode == FwdMode::F32) rc = launch_attention(ctx, p.B, p.T, p.n_rows, p.Nt, D, p.H, p.qkv, L.type, p.att, s);
        else if (p.mode == FwdMode::F16X2) rc = launch_attention_h2f(ctx, p.B, p.T, p.n_rows, p.Nt, D, p.H, p.qkv, L.type, p.att, s);
        else rc = launch_attention3f(ctx, p.B, p.T, p.n_rows, p.Nt, D, p.H, p.qkv, L.type, p.att, s);
        prof_end(ctx, s);
        if (rc) return rc;
        // hidden = relu(BN(W0 [x | message] + b0))   (concat never materialised: two K segments; the second is the attention
        // output, the merge conv folded into W0)
        g = dense_gemm(L.mlp0, M);
        g.K1 = D; g.A = p.x; g.lda = D; g.A2 = p.att; g.lda2 = D; g.relu = true; g.C = p.hid; g.ldc = 2 * D;
        if ((rc = gemm_fp32_act(ctx, p, g, L.mlp0, s))) return rc;
        // x += W1 hidden + b1
        g = dense_gemm(L.mlp1, M);
        g.A = p.hid; g.lda = 2 * D; g.R = p.x; g.ldr = D; g.C = p.x; g.ldc = D;
        if ((rc = gemm_fp32_act(ctx, p, g, L.mlp1, s))) return rc;
    }
    GemmArgs g = dense_gemm(ctx->final_proj, M);  // (no bf16x3 planes of final_proj)
    g.A = p.x; g.lda = D; g.C = p.att; g.ldc = D;
    return gemm_fp32_act(ctx, p, g, ctx->final_proj, s);
}

// F16X2_PLANES: x, the GNN's input, as scaled planes with their tile exponents (in p.msg, p.e_x, p.a_x) - layer 0 and then the
// rest of the front in one launch from the caller's inputs (kenc_fused.hip), or encode() and the conversion of the fp32 x it
// leaves in p.x.  Bit-identical.
static int encode_planes(e2emv_ctx* ctx, const FwdPlan& p, const e2emv_forward_desc* fd, const float* const* d_kpts,
                         const float* const* d_kscores, const void* const* d_desc, hipStream_t s) {
    if (!p.kenc_fused)
        if (int rc = encode(ctx, p, fd, d_kpts, d_kscores, d_desc, s)) return rc;
    uint16_t* xp = (uint16_t*)p.msg;
    prof_begin(ctx, PS_INGEST, s);
    // (the attention skips query tiles beyond the keypoints of an image: their exponent entries must not be stale)
    E2EMV_HIP(ctx, hipMemsetAsync(p.e_x, 0, (size_t)(p.Mtot / 64) * 28 * sizeof(int), s));
    int rc;
    if (p.kenc_fused) {
        IngestParams ip = ingest_params(ctx, p, fd, d_kpts, d_kscores, d_desc);
        ip.h0 = p.hid;  // layer 0 keeps its launch (kenc_fused.hip says why); the fused kernel takes it from there
        hipLaunchKernelGGL(ingest_kenc0, dim3((p.n_rows + 255) / 256, p.B * p.T), dim3(256), 0, s, ip);
        E2EMV_CHECK_LAUNCH(ctx, "ingest_kenc0");
        rc = launch_kenc_fused(ctx, ip, ctx->kenc.data(), xp, p.e_x, p.a_x, s);
    } else {
        rc = launch_to_planes(ctx, p.x, p.Mtot, p.D, p.D, xp, s, p.e_x, p.a_x);
    }
    prof_end(ctx, s);
    return rc;
}

// F16X2_PLANES: the GNN layers - a launch per GEMM or chained - and final_proj on the planes of x
static int gnn_planes(e2emv_ctx* ctx, const FwdPlan& p, hipStream_t s) {
    const int D = p.D, H = p.H, M = (int)p.Mtot;
    uint16_t* xp = (uint16_t*)p.msg;       // x as scaled planes (msg is free until the conf head)
    uint16_t* attp = (uint16_t*)p.att;     // attention output as scaled planes
    uint16_t* qkp = (uint16_t*)p.qkv;      // q | k plain planes [Mtot][2D]
    uint16_t* vtp = qkp + p.Mtot * 4 * D;  // V^T plain planes [n_img][H][64][n_rows]
    uint16_t* hidp = (uint16_t*)p.hid;     // hidden as scaled planes [Mtot][2D]
    int rc;
    auto qkv_args = [&](const LayerWeights& L) {
        GemmP2Args q = dense_gemm_p2(L.qkv, M);
        q.A = xp; q.lda = D; q.out = P2_OUT_QKV; q.Cp = qkp; q.Vt = vtp; q.n_rows = p.n_rows; q.heads = H;
        q.EA = p.e_x; q.EC = p.e_qk; q.EVt = p.e_vt;
        return q;
    };
    // final_proj: x arrives as planes with their tile exponents, any magnitude fp32 holds is fine
    GemmP2Args fin = dense_gemm_p2(ctx->final_proj, M);
    fin.A = xp; fin.lda = D; fin.out = P2_OUT_F32; fin.C32 = p.att; fin.ldc = D; fin.EA = p.e_x;
    for (size_t l = 0; l < ctx->layers.size(); ++l) {
        const LayerWeights& L = ctx->layers[l];
        if (!p.chain || l == 0) {  // (chained: the chain of layer l - 1 made this layer's q | k | v)
            prof_begin(ctx, PS_GEMM_QKV, s); rc = launch_gemm_p2(ctx, qkv_args(L), s); prof_end(ctx, s);
            if (rc) return rc;
        }
        prof_begin(ctx, PS_ATTN, s);
        rc = launch_attention_p2(ctx, p.B, p.T, p.n_rows, p.Nt, D, H, qkp, vtp, L.type, attp, s, p.e_qk, p.e_vt, p.e_att);
        prof_end(ctx, s);
        if (rc) return rc;
        // hidden = relu(W0 [x | attention] + b0)   (merge folded into W0, BN folded)
        GemmP2Args m0 = dense_gemm_p2(L.mlp0, M);
        m0.K1 = D; m0.A = xp; m0.lda = D; m0.A2 = attp; m0.lda2 = D; m0.relu = true; m0.out = P2_OUT_PLANES; m0.Cp = hidp; m0.ldc = 2 * D;
        m0.EA = p.e_x; m0.EA2 = p.e_att; m0.EC = p.e_hid;
        // x += W1 hidden + b1
        GemmP2Args m1 = dense_gemm_p2(L.mlp1, M);
        m1.A = hidp; m1.lda = 2 * D; m1.Rp = xp; m1.ldr = D; m1.out = P2_OUT_PLANES; m1.Cp = xp; m1.ldc = D;
        m1.EA = p.e_hid; m1.ER = p.e_x; m1.AR = p.a_x; m1.EC = p.e_x; m1.AC = p.a_x;
        if (p.chain) {
            const GemmP2Args st[3] = {m0, m1, l + 1 == ctx->layers.size() ? fin : qkv_args(ctx->layers[l + 1])};
            // MLP1's K steps 8 .. 15 read the hidden columns MLP0's SECOND tile stores right in front of it; q | k | v and
            // final_proj read x_new from their first K step on
            const int dep[3] = {P2_CHAIN_INDEP, (2 * D - 256) / 32, 0};
            prof_begin(ctx, PS_GEMM_CHAIN, s); rc = launch_gemm_p2_chain(ctx, st, dep, 3, s); prof_end(ctx, s);
            if (rc) return rc;
            continue;
        }
        prof_begin(ctx, PS_GEMM_MLP0, s); rc = launch_gemm_p2(ctx, m0, s); prof_end(ctx, s);
        if (rc) return rc;
        prof_begin(ctx, PS_GEMM_MLP1, s); rc = launch_gemm_p2(ctx, m1, s); prof_end(ctx, s);
        if (rc) return rc;
    }
    if (p.chain) return E2EMV_OK;  // (the last layer's chain ran final_proj)
    prof_begin(ctx, PS_GEMM, s); rc = launch_gemm_p2(ctx, fin, s); prof_end(ctx, s);
    return rc;
}

// All pairs: score GEMM (1/sqrt(D) fused) -> Sinkhorn -> matches, into so (one output group per pair).  With equal keypoint
// counts all P*B problems go through ONE Sinkhorn batch; a ragged tuple runs one batch per pair (M = N_i, N = N_j).
static int match_pairs(e2emv_ctx* ctx, const FwdPlan& p, const e2emv_forward_desc* fd, float* const* d_logZ, int64_t* const* d_m0,
                       int64_t* const* d_m1, float* const* d_ms0, float* const* d_ms1, float* const* d_conf, SinkhornOut& so,
                       hipStream_t s) {
    const int B = p.B, D = p.D, n_rows = p.n_rows;
    const int64_t tuple_stride = (int64_t)p.T * n_rows * D;
    const int64_t pair_stride = (int64_t)B * p.N * p.ldS;
    so.n_groups = p.P;
    so.group_batch = B;
    int rc;
    for (int pidx = 0; pidx < p.P; ++pidx) {
        const int i = tuple_pair(pidx).i, j = tuple_pair(pidx).j;
        const int Ni = p.Nt[i], Nj = p.Nt[j], ldj = round_up(Nj, 4);
        GemmArgs g;
        g.batch = B; g.M = Ni; g.N = Nj; g.K = D; g.K1 = D;
        g.A = p.att + (int64_t)i * n_rows * D; g.lda = D; g.sA = tuple_stride;
        g.W = p.att + (int64_t)j * n_rows * D; g.ldw = D; g.sW = tuple_stride;
        g.C = p.S + pidx * pair_stride; g.ldc = ldj; g.sC = (int64_t)Ni * ldj;
        g.scale = 1.0f / sqrtf((float)D);
        prof_begin(ctx, PS_SCORE, s); rc = launch_gemm_nt(ctx, g, s); prof_end(ctx, s);
        if (rc) return rc;
        const bool want_conf = p.full && d_conf && d_conf[pidx];
        SinkhornOut one;  // outputs of this pair: one group of B problems
        one.logZ[0] = d_logZ ? d_logZ[pidx] : nullptr;
        if (p.full) {
            one.m0[0] = (d_m0 && d_m0[pidx]) ? d_m0[pidx] : (want_conf ? p.tmp_m0[pidx] : nullptr);
            one.m1[0] = d_m1 ? d_m1[pidx] : nullptr;
            one.ms0[0] = (d_ms0 && d_ms0[pidx]) ? d_ms0[pidx] : (want_conf ? p.tmp_ms0[pidx] : nullptr);
            one.ms1[0] = d_ms1 ? d_ms1[pidx] : nullptr;
        }
        so.logZ[pidx] = one.logZ[0]; so.m0[pidx] = one.m0[0]; so.m1[pidx] = one.m1[0];
        so.ms0[pidx] = one.ms0[0]; so.ms1[pidx] = one.ms1[0];
        if (!p.uniform) {
            prof_begin(ctx, PS_SINKHORN, s);
            rc = launch_sinkhorn(ctx, B, Ni, Nj, p.S + pidx * pair_stride, ldj, ctx->bin_score, fd->sinkhorn_iters,
                                 fd->match_threshold, one, p.skws, s);
            prof_end(ctx, s);
            if (rc) return rc;
        }
    }
    if (p.uniform) {
        prof_begin(ctx, PS_SINKHORN, s);
        rc = launch_sinkhorn(ctx, p.P * B, p.N, p.N, p.S, p.ldS, ctx->bin_score, fd->sinkhorn_iters, fd->match_threshold, so, p.skws, s);
        prof_end(ctx, s);
        if (rc) return rc;
    }
    return E2EMV_OK;
}

// the conf head of every pair whose confidences the caller wants (full output), from the matches0 / mscores0 in so
static int conf_heads(e2emv_ctx* ctx, const FwdPlan& p, const SinkhornOut& so, float* const* d_conf, hipStream_t s) {
    const int B = p.B, D = p.D, n_rows = p.n_rows;
    const int64_t tuple_stride = (int64_t)p.T * n_rows * D;
    const bool use_mlp = ctx->model.conf_mlp != 0;
    const DenseWeights& c0 = ctx->conf0;
    float* gathered = p.msg;  // [B][n_rows][D] ([B][n_rows][2D] in the f16x2 modes)
    float* chid = p.hid;      // [B][n_rows][D]
    int rc;
    for (int pidx = 0; pidx < p.P; ++pidx) {
        const int i = tuple_pair(pidx).i, j = tuple_pair(pidx).j;
        if (!p.full || !d_conf || !d_conf[pidx]) continue;
        const int Ni = p.Nt[i];
        const float* mdesc_i = p.att + (int64_t)i * n_rows * D;
        const float* mdesc_j = p.att + (int64_t)j * n_rows * D;
        if (use_mlp && p.mode == FwdMode::F16X2_PLANES && c0.wp) {
            // plane kernels: [mdesc_i | mdesc_j(match)] -> planes with tile exponents -> conf_mlp.0 (+ BN, ReLU) on gemm_p2
            // (one pass: the gather is resolved in the source address of the plane conversion - p2_tools.hip)
            uint16_t* feat = (uint16_t*)p.qkv;  // [B * n_rows][2D]
            prof_begin(ctx, PS_CONF, s);
            rc = launch_conf_gather_planes(ctx, mdesc_i, mdesc_j, tuple_stride, so.m0[pidx], Ni, n_rows, B, D, feat, p.e_hid, s);
            prof_end(ctx, s);
            if (rc) return rc;
            GemmP2Args q = dense_gemm_p2(c0, B * n_rows);
            q.A = feat; q.lda = 2 * D; q.relu = true; q.out = P2_OUT_F32; q.C32 = chid; q.ldc = D; q.EA = p.e_hid;
            prof_begin(ctx, PS_GEMM, s); rc = launch_gemm_p2(ctx, q, s); prof_end(ctx, s);
            if (rc) return rc;
        } else if (use_mlp && p.f16x2() && c0.wh) {
            prof_begin(ctx, PS_CONF, s);
            hipLaunchKernelGGL(conf_gather2_kernel, dim3((n_rows + 3) / 4, B), dim3(256), 0, s, Ni, n_rows, D, mdesc_i, mdesc_j,
                               tuple_stride, so.m0[pidx], gathered);
            prof_end(ctx, s);
            GemmArgs c = dense_gemm(c0, B * n_rows);
            c.A = gathered; c.lda = 2 * D; c.relu = true; c.C = chid; c.ldc = D;
            prof_begin(ctx, PS_GEMM, s); rc = launch_gemm_h2(ctx, c, c0.wh, 2 * D, c0.hs, s); prof_end(ctx, s);
            if (rc) return rc;
        } else if (use_mlp) {
            prof_begin(ctx, PS_CONF, s);
            hipLaunchKernelGGL(conf_gather_kernel, dim3((n_rows + 3) / 4, B), dim3(256), 0, s, Ni, n_rows, D, mdesc_j, tuple_stride,
                               so.m0[pidx], gathered);
            prof_end(ctx, s);
            GemmArgs c = dense_gemm(c0, n_rows);
            c.batch = B; c.K1 = D;
            c.A = mdesc_i; c.lda = D; c.sA = tuple_stride;
            c.A2 = gathered; c.lda2 = D; c.sA2 = (int64_t)n_rows * D;
            c.relu = true; c.C = chid; c.ldc = D; c.sC = (int64_t)n_rows * D;
            prof_begin(ctx, PS_GEMM, s); rc = launch_gemm_nt(ctx, c, s); prof_end(ctx, s);
            if (rc) return rc;
        }
        prof_begin(ctx, PS_CONF, s);
        hipLaunchKernelGGL(conf_final_kernel, dim3((Ni + 3) / 4, B), dim3(256), 0, s, Ni, n_rows, D, chid, ctx->w_conf1,
                           ctx->b_conf1, so.m0[pidx], so.ms0[pidx], use_mlp ? 1 : 0, d_conf[pidx]);
        prof_end(ctx, s);
        E2EMV_CHECK_LAUNCH(ctx, "conf kernels");
    }
    return E2EMV_OK;
}

static int forward_joint(e2emv_ctx* ctx, const e2emv_forward_desc* fd, const float* const* d_kpts,
                         const float* const* d_kscores, const void* const* d_desc, float* const* d_logZ,
                         int64_t* const* d_m0, int64_t* const* d_m1, float* const* d_ms0, float* const* d_ms1,
                         float* const* d_conf, hipStream_t s) {
    FwdPlan p;
    if (int rc = plan_forward(ctx, fd, p)) return rc;
    if (p.mode == FwdMode::F16X2_PLANES) {
        if (int rc = encode_planes(ctx, p, fd, d_kpts, d_kscores, d_desc, s)) return rc;
        if (int rc = gnn_planes(ctx, p, s)) return rc;
    } else {
        if (int rc = encode(ctx, p, fd, d_kpts, d_kscores, d_desc, s)) return rc;
        if (int rc = gnn_fp32_activations(ctx, p, s)) return rc;
    }
    ctx->last_mdesc = p.att; ctx->md_imgs = p.B * p.T; ctx->md_rows = p.n_rows; ctx->md_n = p.N; ctx->md_dim = p.D;  // (e2emv_get_descriptors)
    SinkhornOut so;
    if (int rc = match_pairs(ctx, p, fd, d_logZ, d_m0, d_m1, d_ms0, d_ms1, d_conf, so, s)) return rc;
    return conf_heads(ctx, p, so, d_conf, s);
}

// the checks of a forward descriptor and its inputs that every entry point below starts with
static int check_forward_inputs(e2emv_ctx* ctx, const e2emv_forward_desc* fd, const float* const* d_kpts, const float* const* d_kscores,
                                const void* const* d_desc) {
    if (!ctx->committed) return set_err(ctx, E2EMV_ESTATE, "matcher_forward: weights not committed");
    const int B = fd->batch, T = fd->tuple_size;
    if (B <= 0 || T < 2 || T > E2EMV_MAX_TUPLE) return set_err(ctx, E2EMV_ESHAPE, "matcher_forward: batch=%d tuple_size=%d", B, T);
    for (int t = 0; t < T; ++t) {
        const int n = fd->n_kpts_img[t] > 0 ? fd->n_kpts_img[t] : fd->n_kpts;
        if (n <= 0 || n > 2048) return set_err(ctx, E2EMV_ESHAPE, "matcher_forward: image %d has n_kpts=%d, not in [1, 2048]", t, n);
    }
    if (fd->desc_dtype != E2EMV_DESC_F32 && fd->desc_dtype != E2EMV_DESC_F16) return set_err(ctx, E2EMV_EINVAL, "bad desc_dtype");
    if (fd->sinkhorn_iters < 0) return set_err(ctx, E2EMV_EINVAL, "negative sinkhorn_iters");
    for (int t = 0; t < T; ++t)
        if (!d_kpts[t] || !d_kscores[t] || !d_desc[t]) return set_err(ctx, E2EMV_EINVAL, "matcher_forward: null input for image %d", t);
    return E2EMV_OK;
}

extern "C" int e2emv_matcher_forward(e2emv_ctx* ctx, const e2emv_forward_desc* fd, const float* const* d_kpts,
                                     const float* const* d_kscores, const void* const* d_desc, float* const* d_logZ,
                                     int64_t* const* d_matches0, int64_t* const* d_matches1, float* const* d_mscores0,
                                     float* const* d_mscores1, float* const* d_conf, void* stream) {
    if (!ctx || !fd || !d_kpts || !d_kscores || !d_desc) return E2EMV_EINVAL;
    E2EMV_ENTER(ctx, stream);
    if (int rc = check_forward_inputs(ctx, fd, d_kpts, d_kscores, d_desc)) return rc;
    const int T = fd->tuple_size;
    (void)hipSetDevice(ctx->device);
    hipStream_t s = (hipStream_t)stream;
    if (T == 2 || (fd->flags & E2EMV_FLAG_MULTI_FRAME))
        return forward_joint(ctx, fd, d_kpts, d_kscores, d_desc, d_logZ, d_matches0, d_matches1, d_mscores0, d_mscores1, d_conf, s);
    // pairwise mode on a tuple: every pair goes through the 2-view network on its own
    for (int pidx = 0; pidx < T * (T - 1) / 2; ++pidx) {
        const int i = tuple_pair(pidx).i, j = tuple_pair(pidx).j;
        e2emv_forward_desc f2 = *fd;
        f2.tuple_size = 2;
        f2.img_w[0] = fd->img_w[i]; f2.img_h[0] = fd->img_h[i];
        f2.img_w[1] = fd->img_w[j]; f2.img_h[1] = fd->img_h[j];
        f2.n_kpts_img[0] = fd->n_kpts_img[i]; f2.n_kpts_img[1] = fd->n_kpts_img[j];
        for (int t = 2; t < E2EMV_MAX_TUPLE; ++t) f2.n_kpts_img[t] = 0;
        const float* kp[2] = {d_kpts[i], d_kpts[j]};
        const float* ks[2] = {d_kscores[i], d_kscores[j]};
        const void* de[2] = {d_desc[i], d_desc[j]};
        float* lz[1] = {d_logZ ? d_logZ[pidx] : nullptr};
        int64_t* m0[1] = {d_matches0 ? d_matches0[pidx] : nullptr};
        int64_t* m1[1] = {d_matches1 ? d_matches1[pidx] : nullptr};
        float* s0[1] = {d_mscores0 ? d_mscores0[pidx] : nullptr};
        float* s1[1] = {d_mscores1 ? d_mscores1[pidx] : nullptr};
        float* cf[1] = {d_conf ? d_conf[pidx] : nullptr};
        int rc = forward_joint(ctx, &f2, kp, ks, de, lz, m0, m1, s0, s1, cf, s);
        if (rc) return rc;
    }
    return E2EMV_OK;
}

// What the front of the plane forward hands to the GNN (e2emv.h): the planes of x, their tile exponents and block maxima, by the
// path e2emv_set_kenc_fused selects - a test compares the two without running a GNN.
extern "C" int e2emv_encode_planes(e2emv_ctx* ctx, const e2emv_forward_desc* fd, const float* const* d_kpts, const float* const* d_kscores,
                                   const void* const* d_desc, uint16_t* d_xp, int32_t* d_ex, float* d_ax, void* stream) {
    if (!ctx || !fd || !d_kpts || !d_kscores || !d_desc || !d_xp || !d_ex || !d_ax) return E2EMV_EINVAL;
    E2EMV_ENTER(ctx, stream);
    if (int rc = check_forward_inputs(ctx, fd, d_kpts, d_kscores, d_desc)) return rc;
    (void)hipSetDevice(ctx->device);
    hipStream_t s = (hipStream_t)stream;
    FwdPlan p;
    if (int rc = plan_forward(ctx, fd, p)) return rc;
    if (p.mode != FwdMode::F16X2_PLANES) return set_err(ctx, E2EMV_ESTATE, "encode_planes: this call would not run on the plane kernels");
    if (int rc = encode_planes(ctx, p, fd, d_kpts, d_kscores, d_desc, s)) return rc;
    const size_t blocks = (size_t)(p.Mtot / 64) * (p.D / 64);
    E2EMV_HIP(ctx, hipMemcpyAsync(d_xp, p.msg, (size_t)p.Mtot * p.D * 4, hipMemcpyDeviceToDevice, s));
    E2EMV_HIP(ctx, hipMemcpyAsync(d_ex, p.e_x, blocks * sizeof(int), hipMemcpyDeviceToDevice, s));
    E2EMV_HIP(ctx, hipMemcpyAsync(d_ax, p.a_x, blocks * sizeof(float), hipMemcpyDeviceToDevice, s));
    return E2EMV_OK;
}

// The matched descriptors (final_proj output, upstream's mdesc0 / mdesc1) of the last e2emv_matcher_forward call: what the
// score matrix was built from.  An audit output - parity tests compare it with the oracle's descriptors, the quantity the GNN
// arithmetic modes differ in (logZ is dominated by the fp32 Sinkhorn).
extern "C" int e2emv_get_descriptors(e2emv_ctx* ctx, float* d_out, int64_t capacity, int* n_img, int* n_kpts, int* dim, void* stream) {
    if (!ctx) return E2EMV_EINVAL;
    E2EMV_ENTER(ctx, stream);
    // (ws_reserve clears the pointer: it is valid only until the next call that uses the workspace)
    if (!ctx->last_mdesc) return set_err(ctx, E2EMV_ESTATE, "get_descriptors: no matcher_forward on this context since the workspace was last reused");
    if (n_img) *n_img = ctx->md_imgs;
    if (n_kpts) *n_kpts = ctx->md_n;
    if (dim) *dim = ctx->md_dim;
    if (!d_out) return E2EMV_OK;  // (size query)
    const int64_t need = (int64_t)ctx->md_imgs * ctx->md_n * ctx->md_dim;
    if (capacity < need) return set_err(ctx, E2EMV_ESHAPE, "get_descriptors: buffer of %lld floats, %lld needed", (long long)capacity, (long long)need);
    const size_t row = (size_t)ctx->md_dim * sizeof(float);
    E2EMV_HIP(ctx, hipMemcpy2DAsync(d_out, (size_t)ctx->md_n * row, ctx->last_mdesc, (size_t)ctx->md_rows * row, (size_t)ctx->md_n * row,
                                    (size_t)ctx->md_imgs, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return E2EMV_OK;
}
