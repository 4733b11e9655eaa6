// Test/bench entry points of the bf16x3 / f16x2 building blocks on plain fp32 buffers, so that the kernels of gemm_x3.hip,
// gemm_h2.hip, attention_x3.hip and attention_h2.hip can be checked in isolation against an fp64 reference.  The bf16x3 GEMM takes
// its weights as S3 planes: the row splitter that makes them is here, next to the q|k|v splitter of the first-generation attention.
#include "attention_walk.h"
#include "common.h"
#include "split3.h"

namespace e2emv {

// fp32 [rows][C] -> S3 [rows][3][ld]
__global__ void split3_rows_kernel(const float* src, int64_t rows, int C, int64_t lds_, uint16_t* dst, int64_t ld) {
    const int64_t r = blockIdx.x;
    for (int c = threadIdx.x; c < C; c += blockDim.x) {
        __bf16 a, b, d;
        split3(src[r * lds_ + c], a, b, d);
        __bf16* o = reinterpret_cast<__bf16*>(dst + r * 3 * ld);
        o[c] = a; o[ld + c] = b; o[2 * ld + c] = d;
    }
}

// qkv fp32 [rows][3D] -> qk S3 [rows][3][2D] (q scaled) + V^T [img][3][D][n_rows]
__global__ void split_qkv_kernel(const float* qkv, int n_rows, int D, float q_scale, uint16_t* qk, uint16_t* vt) {
    const int64_t row = blockIdx.x;
    const int img = (int)(row / n_rows), ml = (int)(row % n_rows);
    const float* src = qkv + row * 3 * D;
    __bf16* qo = reinterpret_cast<__bf16*>(qk + row * 3 * 2 * D);
    __bf16* vo = reinterpret_cast<__bf16*>(vt);
    for (int c = threadIdx.x; c < 3 * D; c += blockDim.x) {
        float v = src[c];
        if (c < D) v *= q_scale;
        __bf16 a, b, d;
        split3(v, a, b, d);
        if (c < 2 * D) {
            qo[c] = a; qo[2 * D + c] = b; qo[4 * D + c] = d;
        } else {
            const int n = c - 2 * D;
            vo[((int64_t)(img * 3 + 0) * D + n) * n_rows + ml] = a;
            vo[((int64_t)(img * 3 + 1) * D + n) * n_rows + ml] = b;
            vo[((int64_t)(img * 3 + 2) * D + n) * n_rows + ml] = d;
        }
    }
}

static int launch_split3(e2emv_ctx* ctx, const float* src, int64_t rows, int C, int64_t ld_src, uint16_t* dst, int64_t ld,
                         hipStream_t s) {
    if (rows <= 0 || C <= 0) return E2EMV_OK;
    hipLaunchKernelGGL(split3_rows_kernel, dim3((unsigned)rows), dim3(256), 0, s, src, rows, C, ld_src, dst, ld);
    E2EMV_CHECK_LAUNCH(ctx, "split3_rows_kernel");
    return E2EMV_OK;
}

}  // namespace e2emv

using namespace e2emv;

extern "C" int e2emv_gemm_bf16x3_ex(e2emv_ctx* ctx, int M, int Nout, int K, int K1, const float* d_A, const float* d_A2, const float* d_W,
                                    const float* d_bias, const float* d_R, float* d_C, int flags, void* stream) {
    if (!ctx || !d_A || !d_W || !d_C) return E2EMV_EINVAL;
    E2EMV_ENTER(ctx, stream);
    if (M <= 0 || Nout <= 0 || K <= 0 || K % 32 || K1 % 32 || K1 <= 0 || K1 > K || (K1 < K && !d_A2) || Nout % 4)
        return set_err(ctx, E2EMV_ESHAPE, "gemm_bf16x3: M=%d N=%d K=%d K1=%d", M, Nout, K, K1);
    hipStream_t s = (hipStream_t)stream;
    auto al = [](size_t b) { return (b + 255) & ~size_t(255); };
    int rc = ws_reserve(ctx, al((size_t)Nout * 3 * K * 2));
    if (rc) return rc;
    uint16_t* W3 = (uint16_t*)ctx->d_ws;
    // activations stay fp32, split on the way into LDS (gemm_x3.hip, gemm_h2.hip); [A | A2] are the two K segments, R the residual
    GemmArgs g;
    g.M = M; g.N = Nout; g.K = K; g.K1 = K1; g.A = d_A; g.lda = K1; g.bias = d_bias; g.C = d_C; g.ldc = Nout; g.relu = (flags & 1) != 0;
    if (K1 < K) { g.A2 = d_A2; g.lda2 = K - K1; }
    if (d_R) { g.R = d_R; g.ldr = Nout; }
    if (flags & 4) {  // f16x2 GEMM (gemm_h2.hip); the weight planes are made on the host as e2emv_commit_weights makes them
        DenseWeights dw;
        if ((rc = dense_from_device(ctx, d_W, d_bias, Nout, K, WF_H2, W3, dw, s))) return rc;
        prof_begin(ctx, PS_GEMM, s);
        rc = launch_gemm_h2(ctx, g, dw.wh, K, dw.hs, s);
        prof_end(ctx, s);
        return rc;
    }
    if (flags & 2) return set_err(ctx, E2EMV_EINVAL, "gemm_bf16x3: flags bit1 (the all-planes first-generation kernel) is retired");
    if ((rc = launch_split3(ctx, d_W, Nout, K, K, W3, K, s))) return rc;
    prof_begin(ctx, PS_GEMM, s);
    rc = launch_gemm_x3(ctx, g, W3, K, s);
    prof_end(ctx, s);
    return rc;
}

extern "C" int e2emv_gemm_bf16x3(e2emv_ctx* ctx, int M, int Nout, int K, const float* d_A, const float* d_W,
                                 const float* d_bias, float* d_C, int flags, void* stream) {
    return e2emv_gemm_bf16x3_ex(ctx, M, Nout, K, K, d_A, nullptr, d_W, d_bias, nullptr, d_C, flags, stream);
}

// body of e2emv_attention_bf16x3 / e2emv_attention_bf16x3_v: nv = valid keypoints of image t of a tuple, T entries
static int attention_bf16x3_entry(e2emv_ctx* ctx, int B, int T, int n_rows, const int* nv, int D, int H, const float* d_qkv, int cross,
                                  float* d_out, void* stream) {
    E2EMV_ENTER(ctx, stream);
    if (B <= 0 || T <= 0 || n_rows <= 0) return set_err(ctx, E2EMV_ESHAPE, "attention_bf16x3: empty problem");
    hipStream_t s = (hipStream_t)stream;
    const int64_t rows = (int64_t)B * T * n_rows;
    AttnShape shape;
    int n_valid;  // (the launchers check the shape too: here before the memset runs)
    if (int rc = attn_shape(ctx, "attention_bf16x3", B, T, n_rows, nv, D, H, cross & 1, 128, &shape, &n_valid)) return rc;
    uint16_t *qk = nullptr, *vt = nullptr;
    if (!(cross & 6)) {  // the first-generation kernel: pre-split planes made here by a helper kernel
        auto al = [](size_t b) { return (b + 255) & ~size_t(255); };
        const size_t sz_qk = al((size_t)rows * 3 * 2 * D * 2), sz_v = al((size_t)rows * 3 * D * 2);
        if (int rc = ws_reserve(ctx, sz_qk + sz_v)) return rc;
        qk = (uint16_t*)ctx->d_ws;
        vt = (uint16_t*)(ctx->d_ws + sz_qk);
        hipLaunchKernelGGL(split_qkv_kernel, dim3((unsigned)rows), dim3(256), 0, s, d_qkv, n_rows, D, 0.125f * 1.4426950408889634f, qk, vt);
        E2EMV_CHECK_LAUNCH(ctx, "split_qkv_kernel");
    }
    E2EMV_HIP(ctx, hipMemsetAsync(d_out, 0, (size_t)rows * D * sizeof(float), s));
    prof_begin(ctx, PS_ATTN, s);
    int rc;  // bit2: the fp16 x 2 form, bit1: the forward pass's bf16x3 kernel (planes made in the kernel)
    if (cross & 4) rc = launch_attention_h2f(ctx, B, T, n_rows, nv, D, H, d_qkv, cross & 1, d_out, s);
    else if (cross & 2) rc = launch_attention3f(ctx, B, T, n_rows, nv, D, H, d_qkv, cross & 1, d_out, s);
    else rc = launch_attention3(ctx, B, T, n_rows, nv, D, H, qk, vt, cross & 1, nullptr, d_out, s);
    prof_end(ctx, s);
    return rc;
}

extern "C" int e2emv_attention_bf16x3(e2emv_ctx* ctx, int B, int T, int n_rows, int n_valid, int D, int H, const float* d_qkv,
                                      int cross, float* d_out, void* stream) {
    if (!ctx || !d_qkv || !d_out) return E2EMV_EINVAL;
    int nv[E2EMV_MAX_TUPLE];
    for (int t = 0; t < E2EMV_MAX_TUPLE; ++t) nv[t] = n_valid;
    return attention_bf16x3_entry(ctx, B, T, n_rows, nv, D, H, d_qkv, cross, d_out, stream);
}

extern "C" int e2emv_attention_bf16x3_v(e2emv_ctx* ctx, int B, int T, int n_rows, const int* n_valid_per_image, int D, int H,
                                        const float* d_qkv, int cross, float* d_out, void* stream) {
    if (!ctx || !d_qkv || !d_out || !n_valid_per_image) return E2EMV_EINVAL;
    return attention_bf16x3_entry(ctx, B, T, n_rows, n_valid_per_image, D, H, d_qkv, cross, d_out, stream);
}
