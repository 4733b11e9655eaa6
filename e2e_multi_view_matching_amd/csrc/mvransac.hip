// The RANSAC relative-pose methods on the batched multi-view path (multi_view.solve_tuple_poses_batch(..., rel_pose_method=
// "ransac" | "ransac_ba")): the device glue between e2emv_mv_collect, e2emv_essential_ransac, the two-view bundle adjustment
// and e2emv_mv_tuple_init / e2emv_mv_tuple_ba.
//
//   prepare  what ransac.normalize_keypoints / estimate_poses_ransac do on the host for one pair at a time: the collected fp32
//            pixel keypoints of every pair -> fp64 normalised keypoints and the normalised inlier threshold
//   filter   what initialize_bundle_adjust does with the RANSAC mask (bundle_adjust_io.py:104-133): matches and confidences
//            reduced to the inliers IN THEIR ORDER, the relative pose as a 4x4, the match-graph weight
//
// One workgroup of 256 threads per problem (b, pair q), one launch each, nothing read back.  The host code is the bit-for-bit
// yardstick (multi_view.relative_poses_ransac): every number here is either copied or the result of the same correctly
// rounded fp64 operations in the same order.
#include <climits>
#include <cstdint>

#include "common.h"

namespace e2emv {

constexpr int kMrThreads = 256;
constexpr int kMrMaxCams = E2EMV_MAX_TUPLE;
constexpr int kMrMaxMatches = 4096;  // RANSAC_MAX_MATCHES of ransac.hip: the widest problem e2emv_essential_ransac takes

struct MrPrepareArgs {
    int P, N, kdim, intr_batch;
    double thresh;                  // pixels
    const float* k0; const float* k1;  // collected: [B*P,N,2]
    const int32_t* count;           // [B*P]
    const float* intr[kMrMaxCams];  // [intr_batch,kdim,kdim] per image
    double *k0n, *k1n;              // [B*P,N,2]
    double* th;                     // [B*P]
};

// image pair of problem q in the enumeration of e2emv_mv_collect: (i, j), i < j, j outer
__device__ __forceinline__ void mr_pair(int q, int& i, int& j) {
    j = 1;
    while (q >= j) { q -= j; ++j; }
    i = q;
}

__global__ __launch_bounds__(kMrThreads) void mv_ransac_prepare_kernel(MrPrepareArgs a) {
    const int pp = blockIdx.x, b = pp / a.P, q = pp - b * a.P, tid = threadIdx.x;
    int i, j;
    mr_pair(q, i, j);
    const size_t koff = a.intr_batch == 1 ? 0 : size_t(b) * a.kdim * a.kdim;
    const float* K0 = a.intr[i] + koff;
    const float* K1 = a.intr[j] + koff;
    // widened first: every operation below is fp64 on the exact values of the fp32 inputs
    const double fx0 = double(K0[0]), fy0 = double(K0[a.kdim + 1]), cx0 = double(K0[2]), cy0 = double(K0[a.kdim + 2]);
    const double fx1 = double(K1[0]), fy1 = double(K1[a.kdim + 1]), cx1 = double(K1[2]), cy1 = double(K1[a.kdim + 2]);
    const int n = min(max(a.count[pp], 0), a.N);
    const float* k0 = a.k0 + size_t(pp) * a.N * 2;
    const float* k1 = a.k1 + size_t(pp) * a.N * 2;
    double* o0 = a.k0n + size_t(pp) * a.N * 2;
    double* o1 = a.k1n + size_t(pp) * a.N * 2;
    for (int r = tid; r < a.N; r += kMrThreads) {
        const bool in = r < n;
        o0[2 * r] = in ? (double(k0[2 * r]) - cx0) / fx0 : 0.0;
        o0[2 * r + 1] = in ? (double(k0[2 * r + 1]) - cy0) / fy0 : 0.0;
        o1[2 * r] = in ? (double(k1[2 * r]) - cx1) / fx1 : 0.0;
        o1[2 * r + 1] = in ? (double(k1[2 * r + 1]) - cy1) / fy1 : 0.0;
    }
    // upstream's np.mean([K0[0,0], K1[1,1], K0[0,0], K1[1,1]]) in its order (the division by 4 is exact)
    if (tid == 0) a.th[pp] = a.thresh / ((((fx0 + fy1) + fx0) + fy1) / 4.0);
}

struct MrFilterArgs {
    int N;
    const float* k0; const float* k1; const float* conf;  // collected: [B*P,N,2] x2, [B*P,N]
    const int32_t* count;                                  // [B*P]
    const double* k0n; const double* k1n;                  // [B*P,N,2]
    const uint8_t* inl;                                    // [B*P,N]
    const int32_t* n_inl; const int32_t* status;           // [B*P]
    const double* R; const double* t;                      // [B*P,9], [B*P,3]
    float *f0, *f1, *fc;                                   // filtered pixels / confidences
    float *f0n, *f1n, *fcn;                                // filtered normalised keypoints / confidences (all NULL: not wanted)
    float* T0;                                             // [B*P,16]
    int32_t *ba_count, *graph_w;                           // [B*P]
};

// Ordered compaction by the RANSAC mask, the scheme of mv_collect_kernel (ballot prefix inside a wave, wave totals through LDS,
// a running base across the chunks of 256).  A problem whose RANSAC failed keeps every match (mask = all rows below its count).
__global__ __launch_bounds__(kMrThreads) void mv_ransac_filter_kernel(MrFilterArgs a) {
    __shared__ int s_wave[kMrThreads / 64];
    const int pp = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int N = a.N;
    const bool solved = a.status[pp] == 0;
    const int cnt = min(max(a.count[pp], 0), N);
    const size_t row0 = size_t(pp) * N;
    const float* k0 = a.k0 + row0 * 2;
    const float* k1 = a.k1 + row0 * 2;
    const float* conf = a.conf + row0;
    const double* k0n = a.k0n + row0 * 2;
    const double* k1n = a.k1n + row0 * 2;
    const uint8_t* inl = a.inl + row0;
    float* f0 = a.f0 + row0 * 2;
    float* f1 = a.f1 + row0 * 2;
    float* fc = a.fc + row0;
    float* f0n = a.f0n ? a.f0n + row0 * 2 : nullptr;
    float* f1n = a.f1n ? a.f1n + row0 * 2 : nullptr;
    float* fcn = a.fcn ? a.fcn + row0 : nullptr;
    int base = 0;
    for (int c0 = 0; c0 < cnt; c0 += kMrThreads) {
        const int n = c0 + tid;
        const bool keep = n < cnt && (!solved || inl[n] != 0);
        const unsigned long long mask = __ballot(keep);
        if (lane == 0) s_wave[wave] = __popcll(mask);
        __syncthreads();
        int off = base + __popcll(mask & ((1ull << lane) - 1ull)), total = 0;
        for (int w = 0; w < kMrThreads / 64; ++w) {
            if (w < wave) off += s_wave[w];
            total += s_wave[w];
        }
        if (keep) {
            f0[2 * off] = k0[2 * n]; f0[2 * off + 1] = k0[2 * n + 1];
            f1[2 * off] = k1[2 * n]; f1[2 * off + 1] = k1[2 * n + 1];
            fc[off] = conf[n];
            if (f0n) {  // the fp64 value rounded once, as an assignment into a float32 array does on the host
                f0n[2 * off] = float(k0n[2 * n]); f0n[2 * off + 1] = float(k0n[2 * n + 1]);
                f1n[2 * off] = float(k1n[2 * n]); f1n[2 * off + 1] = float(k1n[2 * n + 1]);
                fcn[off] = solved ? conf[n] : 0.f;  // no weight: the two-view bundle adjustment leaves an unsolved pair alone
            }
        }
        base += total;
        __syncthreads();
    }
    for (int n = base + tid; n < N; n += kMrThreads) {
        f0[2 * n] = 0.f; f0[2 * n + 1] = 0.f; f1[2 * n] = 0.f; f1[2 * n + 1] = 0.f; fc[n] = 0.f;
        if (f0n) { f0n[2 * n] = 0.f; f0n[2 * n + 1] = 0.f; f1n[2 * n] = 0.f; f1n[2 * n + 1] = 0.f; fcn[n] = 0.f; }
    }
    if (tid < 16) {
        const int r = tid >> 2, c = tid & 3;
        float v = r == c ? 1.f : 0.f;
        if (solved && r < 3) v = float(c < 3 ? a.R[size_t(pp) * 9 + 3 * r + c] : a.t[size_t(pp) * 3 + r]);
        a.T0[size_t(pp) * 16 + tid] = v;
    }
    if (tid == 0) {
        a.ba_count[pp] = solved ? a.n_inl[pp] : cnt;
        a.graph_w[pp] = solved ? a.n_inl[pp] : 0;
    }
}

// B, T, N of a batch of collected tuples: the checks both entry points share
static int mr_check_shape(e2emv_ctx* ctx, const char* who, int B, int T, int N) {
    if (B < 1 || N < 1) return set_err(ctx, E2EMV_EINVAL, "%s: bad argument (B, N >= 1, no NULL array)", who);
    if (T < 2 || T > kMrMaxCams) return set_err(ctx, E2EMV_EINVAL, "%s: tuple of %d images (2 <= T <= %d)", who, T, kMrMaxCams);
    if (N > kMrMaxMatches) return set_err(ctx, E2EMV_ESHAPE, "%s: N = %d (the RANSAC takes at most %d matches per pair)", who, N, kMrMaxMatches);
    const size_t rows = size_t(B) * (T * (T - 1) / 2) * N;
    if (rows > size_t(INT32_MAX) / 2) return set_err(ctx, E2EMV_ESHAPE, "%s: B * pairs * N = %zu is too large", who, rows);
    return E2EMV_OK;
}

}  // namespace e2emv

using namespace e2emv;

extern "C" int e2emv_mv_ransac_prepare(e2emv_ctx* ctx, int B, int T, int N, const float* d_mkpts0, const float* d_mkpts1,
                                       const int32_t* d_count, const float* const* d_intr, int kdim, int intr_batch, double thresh,
                                       double* d_kpts0n, double* d_kpts1n, double* d_thresh, void* stream) {
    if (!ctx) return E2EMV_EINVAL;
    E2EMV_ENTER(ctx, stream);
    if (!d_mkpts0 || !d_mkpts1 || !d_count || !d_intr || !d_kpts0n || !d_kpts1n || !d_thresh)
        return set_err(ctx, E2EMV_EINVAL, "mv_ransac_prepare: bad argument (B, N >= 1, no NULL array)");
    const int rc = mr_check_shape(ctx, "mv_ransac_prepare", B, T, N);
    if (rc) return rc;
    if (kdim != 3 && kdim != 4) return set_err(ctx, E2EMV_ESHAPE, "mv_ransac_prepare: intrinsics must be 3x3 or 4x4");
    if (intr_batch != 1 && intr_batch != B) return set_err(ctx, E2EMV_ESHAPE, "mv_ransac_prepare: intr_batch must be 1 or B");
    if (!(thresh > 0.0)) return set_err(ctx, E2EMV_EINVAL, "mv_ransac_prepare: thresh = %g pixels (> 0)", thresh);
    MrPrepareArgs a{};
    a.P = T * (T - 1) / 2; a.N = N; a.kdim = kdim; a.intr_batch = intr_batch; a.thresh = thresh;
    for (int t = 0; t < T; ++t) {
        if (!d_intr[t]) return set_err(ctx, E2EMV_EINVAL, "mv_ransac_prepare: NULL intrinsics of image %d", t);
        a.intr[t] = d_intr[t];
    }
    a.k0 = d_mkpts0; a.k1 = d_mkpts1; a.count = d_count; a.k0n = d_kpts0n; a.k1n = d_kpts1n; a.th = d_thresh;
    hipLaunchKernelGGL(mv_ransac_prepare_kernel, dim3(B * a.P), dim3(kMrThreads), 0, (hipStream_t)stream, a);
    E2EMV_CHECK_LAUNCH(ctx, "mv_ransac_prepare_kernel");
    return E2EMV_OK;
}

extern "C" int e2emv_mv_ransac_filter(e2emv_ctx* ctx, int B, int T, int N, const float* d_mkpts0, const float* d_mkpts1,
                                      const float* d_mconf, const int32_t* d_count, const double* d_kpts0n, const double* d_kpts1n,
                                      const uint8_t* d_inliers, const int32_t* d_n_inliers, const double* d_R, const double* d_t,
                                      const int32_t* d_status, float* d_fkpts0, float* d_fkpts1, float* d_fconf, float* d_fkpts0n,
                                      float* d_fkpts1n, float* d_fconfn, float* d_T0, int32_t* d_ba_count, int32_t* d_graph_w,
                                      void* stream) {
    if (!ctx) return E2EMV_EINVAL;
    E2EMV_ENTER(ctx, stream);
    if (!d_mkpts0 || !d_mkpts1 || !d_mconf || !d_count || !d_kpts0n || !d_kpts1n || !d_inliers || !d_n_inliers || !d_R || !d_t ||
        !d_status || !d_fkpts0 || !d_fkpts1 || !d_fconf || !d_T0 || !d_ba_count || !d_graph_w)
        return set_err(ctx, E2EMV_EINVAL, "mv_ransac_filter: bad argument (B, N >= 1, no NULL array)");
    if ((d_fkpts0n != nullptr) != (d_fkpts1n != nullptr) || (d_fkpts0n != nullptr) != (d_fconfn != nullptr))
        return set_err(ctx, E2EMV_EINVAL, "mv_ransac_filter: the normalised outputs are given all three or not at all");
    const int rc = mr_check_shape(ctx, "mv_ransac_filter", B, T, N);
    if (rc) return rc;
    MrFilterArgs a{};
    a.N = N;
    a.k0 = d_mkpts0; a.k1 = d_mkpts1; a.conf = d_mconf; a.count = d_count; a.k0n = d_kpts0n; a.k1n = d_kpts1n;
    a.inl = d_inliers; a.n_inl = d_n_inliers; a.status = d_status; a.R = d_R; a.t = d_t;
    a.f0 = d_fkpts0; a.f1 = d_fkpts1; a.fc = d_fconf; a.f0n = d_fkpts0n; a.f1n = d_fkpts1n; a.fcn = d_fconfn;
    a.T0 = d_T0; a.ba_count = d_ba_count; a.graph_w = d_graph_w;
    hipLaunchKernelGGL(mv_ransac_filter_kernel, dim3(B * (T * (T - 1) / 2)), dim3(kMrThreads), 0, (hipStream_t)stream, a);
    E2EMV_CHECK_LAUNCH(ctx, "mv_ransac_filter_kernel");
    return E2EMV_OK;
}
