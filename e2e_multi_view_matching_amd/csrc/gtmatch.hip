// Ground-truth match targets from depth + pose, and the match loss (SURVEY.md 8(f) "next" row 2): the other
// consumer of the matcher's log-assignment `scores_i_j` (helpers.run_matcher, helpers.py:243-253) and the
// quantity the reference's only explicit collective carries (validation loss, train.py:102-106).
//
// Restates helpers.py: transform_kpts :114-118, compute_gt_matches_of_image_pair :121-203, set_weight :205-213,
// compute_match_loss :228-241.  The reference materialises the B x N x N reprojection-error tensor (twice, plus
// expand temporaries) and runs ~40 torch ops on it; here the error of a keypoint pair is recomputed on the fly
// (two sqrt's) inside wave-per-row / wave-per-column arg-min kernels, nothing N x N ever touches HBM.
// Reference quirks kept: keypoints are truncated to integer pixels and those integers enter the errors; first index
// wins arg-min ties (NaN counts as minimal, as in torch); the dustbin slot N keeps index -1 and gets the un-match
// weight; index -1 in the loss addresses the last (dustbin) column.
//
// The match term of a training step for ALL pairs of a tuple: e2emv_gt_matches_tuple runs the three target kernels with
// the pair as one more grid dimension, on relative poses formed on the device; e2emv_match_loss_tuple sums the per-pair losses in
// pair order; e2emv_match_loss_tuple_backward writes d loss / d scores of every pair in one pass of stores.
#include "common.h"
#include "small_linalg.h"

namespace e2emv {

struct GtParams {
    int B, N, H, W;
    const float* k0;      // [B][N][2]
    const float* k1;
    const float* K0;      // [B][4][4]
    const float* K1;
    const float* T01;     // [B][4][4]
    const float* depth0;  // [B][H][W]
    const float* depth1;
    float max_matched, min_unmatched;
    // workspace (per direction s = 0: image 0 -> 1, s = 1: image 1 -> 0), all [2][B][N]
    float* ki;     // [2][B][N][2] truncated integer keypoints (as float)
    float* d;      // depth at the keypoint
    float* kto;    // [2][B][N][2] keypoint reprojected into the other image
    float* dto;    // its depth there
    float* emin;   // [2][B][N] min error along the row (s=0) / column (s=1)
    int* amin;     // [2][B][N] arg-min
    int64_t* idx;  // out [B][2][N+1]
    float* w;      // out [B][2][N+1]
};

__device__ bool inv4(const double* m, double* inv) {  // Gauss-Jordan with partial pivoting
    double a[4][8];
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) { a[i][j] = m[i * 4 + j]; a[i][4 + j] = (i == j) ? 1.0 : 0.0; }
    for (int c = 0; c < 4; ++c) {
        int p = c;
        for (int r = c + 1; r < 4; ++r)
            if (fabs(a[r][c]) > fabs(a[p][c])) p = r;
        if (!(fabs(a[p][c]) > 0.0)) return false;
        if (p != c)
            for (int k = 0; k < 8; ++k) { const double t = a[c][k]; a[c][k] = a[p][k]; a[p][k] = t; }
        const double d = 1.0 / a[c][c];
        for (int k = 0; k < 8; ++k) a[c][k] *= d;
        for (int r = 0; r < 4; ++r)
            if (r != c) {
                const double f = a[r][c];
                for (int k = 0; k < 8; ++k) a[r][k] -= f * a[c][k];
            }
    }
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) inv[i * 4 + j] = a[i][4 + j];
    return true;
}

__device__ void mul4(const double* a, const double* b, double* c) {
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            double s = 0.0;
            for (int k = 0; k < 4; ++k) s += a[i * 4 + k] * b[k * 4 + j];
            c[i * 4 + j] = s;
        }
}

// The three steps below are written once, as device functions of (problem, batch element b, direction s, block bx along the
// keypoints): the per-pair kernels call them with the grid's own indices, the tuple kernels with the pair as one more grid
// dimension and that pair's GtParams (pair_params).

// transform_kpts for both directions: grid (ceil(N/256), B, 2)
__device__ __forceinline__ void gt_transform_body(const GtParams& p, int b, int s, int bx) {
    __shared__ double M[16];
    const int i = bx * 256 + threadIdx.x;
    if (threadIdx.x == 0) {
        double Ka[16], Kb[16], T[16], Ti[16], Kai[16], tmp[16];
        const float* Ks = (s == 0 ? p.K0 : p.K1) + (int64_t)b * 16;
        const float* Kt = (s == 0 ? p.K1 : p.K0) + (int64_t)b * 16;
        for (int k = 0; k < 16; ++k) { Ka[k] = Ks[k]; Kb[k] = Kt[k]; T[k] = p.T01[(int64_t)b * 16 + k]; }
        if (s == 1) { inv4(T, Ti); for (int k = 0; k < 16; ++k) T[k] = Ti[k]; }
        inv4(Ka, Kai);
        mul4(Kb, T, tmp);
        mul4(tmp, Kai, M);  // K_target T K_source^-1
    }
    __syncthreads();
    if (i >= p.N) return;
    const float* k = (s == 0 ? p.k0 : p.k1) + ((int64_t)b * p.N + i) * 2;
    const float* depth = (s == 0 ? p.depth0 : p.depth1) + (int64_t)b * p.H * p.W;
    const int xi = (int)k[0], yi = (int)k[1];  // .long(): truncation toward zero
    const int xc = min(max(xi, 0), p.W - 1), yc = min(max(yi, 0), p.H - 1);
    const float d = depth[(int64_t)yc * p.W + xc];
    const double x = (double)xi * d, y = (double)yi * d;
    const double px = M[0] * x + M[1] * y + M[2] * d + M[3];
    const double py = M[4] * x + M[5] * y + M[6] * d + M[7];
    const double pz = M[8] * x + M[9] * y + M[10] * d + M[11];
    const int64_t o = ((int64_t)s * p.B + b) * p.N + i;
    p.ki[o * 2] = (float)xi; p.ki[o * 2 + 1] = (float)yi;
    p.d[o] = d;
    p.kto[o * 2] = (float)(px / pz); p.kto[o * 2 + 1] = (float)(py / pz);
    p.dto[o] = (float)pz;
}

// mean bidirectional reprojection error of (kpt i of image 0, kpt j of image 1)  (:136-138)
__device__ __forceinline__ float pair_err(float k0x, float k0y, float t01x, float t01y, float k1x, float k1y, float t10x, float t10y) {
    const float ax = t10x - k0x, ay = t10y - k0y;   // kpts1to0[j] - kpts0[i]
    const float bx = t01x - k1x, by = t01y - k1y;   // kpts0to1[i] - kpts1[j]
    return (sqrtf(ax * ax + ay * ay) + sqrtf(bx * bx + by * by)) / 2.0f;
}

__global__ __launch_bounds__(256) void gt_transform(GtParams p) { gt_transform_body(p, blockIdx.y, blockIdx.z, blockIdx.x); }

// arg-min along rows (s = 0: for each kpt0 the closest kpt1) and columns (s = 1); one wave per row/column
__device__ __forceinline__ void gt_argmin_body(const GtParams& p, int b, int s, int bx) {
    const int r = bx * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (r >= p.N) return;
    const int64_t o0 = (int64_t)b * p.N, o1 = ((int64_t)p.B + b) * p.N;
    float best = INFINITY;
    int bj = 0x7fffffff;
    bool bnan = false;
    if (s == 0) {
        const float k0x = p.ki[(o0 + r) * 2], k0y = p.ki[(o0 + r) * 2 + 1], tx = p.kto[(o0 + r) * 2], ty = p.kto[(o0 + r) * 2 + 1];
        for (int j = lane; j < p.N; j += 64) {
            const float e = pair_err(k0x, k0y, tx, ty, p.ki[(o1 + j) * 2], p.ki[(o1 + j) * 2 + 1], p.kto[(o1 + j) * 2], p.kto[(o1 + j) * 2 + 1]);
            const bool en = e != e;
            if (!bnan && (en || e < best)) { best = e; bj = j; bnan = en; }
        }
    } else {
        const float k1x = p.ki[(o1 + r) * 2], k1y = p.ki[(o1 + r) * 2 + 1], tx = p.kto[(o1 + r) * 2], ty = p.kto[(o1 + r) * 2 + 1];
        for (int i = lane; i < p.N; i += 64) {
            const float e = pair_err(p.ki[(o0 + i) * 2], p.ki[(o0 + i) * 2 + 1], p.kto[(o0 + i) * 2], p.kto[(o0 + i) * 2 + 1], k1x, k1y, tx, ty);
            const bool en = e != e;
            if (!bnan && (en || e < best)) { best = e; bj = i; bnan = en; }
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float ob = __shfl_xor(best, off);
        const int oj = __shfl_xor(bj, off);
        const bool on = __shfl_xor((int)bnan, off) != 0;
        bool take;
        if (on != bnan) take = on;                     // NaN is "minimal" (torch.argmin semantics)
        else if (on) take = oj < bj;                   // both NaN: first index
        else take = ob < best || (ob == best && oj < bj);
        if (take) { best = ob; bj = oj; bnan = on; }
    }
    if (lane == 0) {
        const int64_t o = ((int64_t)s * p.B + b) * p.N + r;
        p.emin[o] = best;
        p.amin[o] = bj == 0x7fffffff ? 0 : bj;
    }
}

__global__ __launch_bounds__(256) void gt_argmin(GtParams p) { gt_argmin_body(p, blockIdx.y, blockIdx.z, blockIdx.x); }

// match / drop logic and class-balancing weights (:147-203); one workgroup per pair
__device__ __forceinline__ void gt_finalize_body(const GtParams& p, int b) {
    __shared__ int scount[2];
    __shared__ float sw[2];
    const int tid = threadIdx.x, N = p.N;
    const int64_t o0 = (int64_t)b * N, o1 = ((int64_t)p.B + b) * N;
    int64_t* idx0 = p.idx + (int64_t)b * 2 * (N + 1);
    int64_t* idx1 = idx0 + (N + 1);
    float* w0 = p.w + (int64_t)b * 2 * (N + 1);
    float* w1 = w0 + (N + 1);
    if (tid < 2) scount[tid] = 0;
    for (int j = tid; j <= N; j += 256) { idx0[j] = -1; idx1[j] = -1; w0[j] = 0.f; w1[j] = 0.f; }
    __syncthreads();
    int mc = 0, dc = 0;
    for (int i = tid; i < N; i += 256) {
        const int i1 = p.amin[o0 + i];
        const float e = p.emin[o0 + i];
        const float d0 = p.d[o0 + i], md1 = p.d[o1 + i1];
        const bool vd0 = d0 > 1e-6f, vd1 = md1 > 1e-6f;
        bool match = (p.amin[o1 + i1] == i) && (e <= p.max_matched) && vd0 && vd1;
        if (match) {
            const float r01 = fabsf(p.dto[o0 + i] - md1) / md1;
            const float r10 = fabsf(p.dto[o1 + i1] - d0) / d0;
            match = (r01 < 0.1f) && (r10 < 0.1f);
        }
        if (match) {
            idx0[i] = i1;
            idx1[i1] = i;  // unique: mutual nearest neighbours
            ++mc;
        } else if (!vd0 || !vd1 || e <= p.min_unmatched) {
            w0[i] = -1.f;
            ++dc;
        }
    }
    __syncthreads();  // idx1 complete
    for (int j = tid; j < N; j += 256) {
        if (idx1[j] != -1) continue;
        const int i0 = p.amin[o1 + j];
        const bool invalid = !(p.d[o0 + i0] > 1e-6f) || !(p.d[o1 + j] > 1e-6f);
        if (invalid || p.emin[o1 + j] <= p.min_unmatched) { w1[j] = -1.f; ++dc; }
    }
    atomicAdd(&scount[0], mc);
    atomicAdd(&scount[1], dc);
    __syncthreads();
    if (tid == 0) {
        float mw = 2.f * (float)scount[0] / (2.f * (float)N - (float)scount[1]);
        float uw = 0.5f / (1.f - mw);
        mw = 0.5f / mw;
        if (!(isfinite(mw) && isfinite(uw))) { mw = 0.f; uw = 0.f; }
        sw[0] = mw; sw[1] = uw;
    }
    __syncthreads();
    const float mw = sw[0], uw = sw[1];
    for (int j = tid; j <= N; j += 256) {  // set_weight, including the dustbin slot (index -1 -> un-match weight)
        w0[j] = (w0[j] == -1.f) ? 0.f : (idx0[j] == -1 ? uw : mw);
        w1[j] = (w1[j] == -1.f) ? 0.f : (idx1[j] == -1 ? uw : mw);
    }
}

__global__ __launch_bounds__(256) void gt_finalize(GtParams p) { gt_finalize_body(p, blockIdx.x); }

// ---- the targets of every pair of a tuple: the same three steps, pair q = one more grid dimension ----
struct GtTupleParams {
    int B, N, H, W;
    const float* kpts[E2EMV_MAX_TUPLE];   // image t: [B][N][2]
    const float* K[E2EMV_MAX_TUPLE];      // [B][4][4]
    const float* pose[E2EMV_MAX_TUPLE];   // [B][4][4], data["pose t"]
    const float* depth[E2EMV_MAX_TUPLE];  // [B][H][W]
    unsigned char pi[kMaxGroups], pj[kMaxGroups];  // pair q = (pi[q], pj[q]), pi < pj
    float max_matched, min_unmatched;
    float* T01;        // workspace [P][B][4][4]: inv(pose_j) @ pose_i, fp32 as e2emv_relative_pose stores it
    char* ws;          // workspace of pair q at ws + q * ws_stride, laid out as e2emv_gt_matches lays out its own
    size_t ws_stride, sz2, sz1;
    int64_t* idx;      // out [P][B][2][N+1]
    float* w;          // out [P][B][2][N+1]
};

__device__ __forceinline__ GtParams pair_params(const GtTupleParams& t, int q) {
    GtParams p;
    const int i = t.pi[q], j = t.pj[q];
    p.B = t.B; p.N = t.N; p.H = t.H; p.W = t.W;
    p.k0 = t.kpts[i]; p.k1 = t.kpts[j]; p.K0 = t.K[i]; p.K1 = t.K[j]; p.depth0 = t.depth[i]; p.depth1 = t.depth[j];
    p.T01 = t.T01 + (int64_t)q * t.B * 16;
    p.max_matched = t.max_matched; p.min_unmatched = t.min_unmatched;
    char* w = t.ws + (size_t)q * t.ws_stride;
    p.ki = (float*)w; w += t.sz2;
    p.kto = (float*)w; w += t.sz2;
    p.d = (float*)w; w += t.sz1;
    p.dto = (float*)w; w += t.sz1;
    p.emin = (float*)w; w += t.sz1;
    p.amin = (int*)w;
    p.idx = t.idx + (int64_t)q * t.B * 2 * (t.N + 1);
    p.w = t.w + (int64_t)q * t.B * 2 * (t.N + 1);
    return p;
}

// relative pose of every (pair, batch element): grid (ceil(B/64), P)
__global__ __launch_bounds__(64) void gt_tuple_relative_pose(GtTupleParams t) {
    const int b = blockIdx.x * 64 + threadIdx.x, q = blockIdx.y;
    if (b >= t.B) return;
    relative_pose_one(t.pose[t.pi[q]] + (int64_t)b * 16, t.pose[t.pj[q]] + (int64_t)b * 16, t.T01 + ((int64_t)q * t.B + b) * 16);
}
// grid (ceil(N/256), B, 2P): z = 2q + s
__global__ __launch_bounds__(256) void gt_tuple_transform(GtTupleParams t) {
    gt_transform_body(pair_params(t, blockIdx.z >> 1), blockIdx.y, blockIdx.z & 1, blockIdx.x);
}
__global__ __launch_bounds__(256) void gt_tuple_argmin(GtTupleParams t) {
    gt_argmin_body(pair_params(t, blockIdx.z >> 1), blockIdx.y, blockIdx.z & 1, blockIdx.x);
}
// grid (B, P)
__global__ __launch_bounds__(256) void gt_tuple_finalize(GtTupleParams t) { gt_finalize_body(pair_params(t, blockIdx.y), blockIdx.x); }

// compute_match_loss: one workgroup per batch element -> partial sums, then one thread folds them
__device__ __forceinline__ void match_loss_body(int b, int N, const float* logp, const int64_t* idx, const float* w, double* partial) {
    __shared__ double red[4];
    const int tid = threadIdx.x, ft = N + 1;
    const float* lp = logp + (int64_t)b * ft * ft;
    const int64_t* i0 = idx + (int64_t)b * 2 * ft;
    const int64_t* i1 = i0 + ft;
    const float* w0 = w + (int64_t)b * 2 * ft;
    const float* w1 = w0 + ft;
    double acc = 0.0;
    for (int r = tid; r < ft; r += 256) {
        int64_t c0 = i0[r], c1 = i1[r];
        if (c0 < 0) c0 += ft;  // python negative index: -1 -> dustbin column
        if (c1 < 0) c1 += ft;
        acc -= (double)lp[(int64_t)r * ft + c0] * (double)w0[r];   // l0 = -log_p[b, r, idx0[r]]
        acc -= (double)lp[(int64_t)c1 * ft + r] * (double)w1[r];   // l1 = -log_p^T[b, r, idx1[r]] = -log_p[b, idx1[r], r]
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
    if ((tid & 63) == 0) red[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) partial[b] = red[0] + red[1] + red[2] + red[3];
}
__global__ __launch_bounds__(256) void match_loss_kernel(int B, int N, const float* logp, const int64_t* idx, const float* w,
                                                         double* partial) {
    match_loss_body(blockIdx.x, N, logp, idx, w, partial);
}
__global__ void match_loss_fold(int B, const double* partial, float* loss) {
    double s = 0.0;
    for (int b = 0; b < B; ++b) s += partial[b];
    loss[0] = (float)(s / B);
}

// ---- the match term of helpers.run_matcher over the P pairs of a tuple (helpers.py:250-253) ----
struct MatchLossTupleParams {
    int B, N;
    const float* logZ[kMaxGroups];  // pair q: [B][N+1][N+1]
    const int64_t* idx;             // [P][B][2][N+1]
    const float* w;                 // [P][B][2][N+1]
    double* partial;                // workspace [P][B]
};
// grid (B, P): match_loss_kernel on pair q
__global__ __launch_bounds__(256) void match_loss_tuple_kernel(MatchLossTupleParams p) {
    const int q = blockIdx.y;
    const int64_t o = (int64_t)q * p.B * 2 * (p.N + 1);
    match_loss_body(blockIdx.x, p.N, p.logZ[q], p.idx + o, p.w + o, p.partial + (int64_t)q * p.B);
}
// pair q folds as match_loss_fold does; the pairs are added in fp32 in ascending q like `match_loss = match_loss + ...`
__global__ void match_loss_tuple_fold(int P, int B, const double* partial, float* loss, float* pair_loss) {
    float total = 0.0f;
    for (int q = 0; q < P; ++q) {
        double s = 0.0;
        for (int b = 0; b < B; ++b) s += partial[(int64_t)q * B + b];
        const float l = (float)(s / B);
        if (pair_loss) pair_loss[q] = l;
        total = total + l;
    }
    loss[0] = total;
}

// Backward of the above to the scores: d loss / d logZ[q][b][r][c] = (c == col0(r) ? -(gb w0[r]) : 0) + (r == row1(c) ? -(gb w1[c]) : 0)
// with gb = g / B - at most 2 (N+1) non-zeros per problem, and every element is written here: no memset, no scatter, no atomics.
// A pure store stream.  Pair q's [B][ft][ft] is one flat array of B ft rows, cut into 16-byte vectors at the boundaries of its
// ADDRESS (a row of ft = 1025 floats is only 4-byte aligned).  Row rho starts phi(rho) = (a0 + rho ft) mod 4 elements into a vector
// (a0: the array's own start), so the rows rho = k mod 4 share one phase: a wave takes 64 such rows of one sample and 64 vectors of
// them, keeps the column terms row1(c), -(gb w1[c]) of its four columns in registers and streams down the rows - per row two
// compares, two selects and one add per element, and the row's own term from a lane that loaded it up front.  That covers every
// vector that lies inside one row.  The others - a vector that holds the start of a row at a position other than its first, the
// partial vectors at the two ends of the array (the end counts as the start of row B ft), and with ft < 4 every vector at a row
// start - go element by element, one lane per row start, as a 16-byte store where all four elements exist; no vector is left out
// and with ft >= 4 none is written twice.
struct MatchLossBwdParams {
    int B, N;
    const int64_t* idx;  // [P][B][2][N+1]
    const float* w;      // [P][B][2][N+1]
    const float* g;      // device, 1 float
    float* glogZ[kMaxGroups];  // pair q: [B][N+1][N+1], NULL = pair left out
};

// the term of an index vector at slot i of (sample bb, direction s): what it addresses (-1: nothing) and -(gb w)
__device__ __forceinline__ void match_loss_term(const int64_t* idx, const float* w, int ft, int bb, int s, int i, float gb, int& at, float& t) {
    const int64_t o = ((int64_t)bb * 2 + s) * ft + i;
    int64_t a = idx[o];
    if (a < 0) a += ft;  // python negative index, as match_loss_kernel
    at = (a >= 0 && a < ft) ? (int)a : -1;
    t = -__fmul_rn(gb, w[o]);
}
__device__ __forceinline__ float match_loss_grad(int r, int c, int c0, float t0, int r1, float t1) {
    return __fadd_rn(c == c0 ? t0 : 0.0f, r == r1 ? t1 : 0.0f);
}

constexpr int kBwdRows = 64;  // rows of one phase per wave = lanes

// grid (ceil(row slabs * column slabs / 4), 4 B, P): blockIdx.y = 4 b + k, a wave per (row slab, column slab)
__global__ __launch_bounds__(256) void match_loss_tuple_backward_kernel(MatchLossBwdParams p) {
    const int q = blockIdx.z, b = blockIdx.y >> 2, k = blockIdx.y & 3, ft = p.N + 1, lane = threadIdx.x & 63;
    float* out = p.glogZ[q];
    if (!out) return;
    const int64_t* idx = p.idx + (int64_t)q * p.B * 2 * ft;
    const float* w = p.w + (int64_t)q * p.B * 2 * ft;
    const float gb = __fdiv_rn(p.g[0], (float)p.B);
    const int64_t total = (int64_t)p.B * ft * ft;
    const int a0 = (int)(((uintptr_t)out >> 2) & 3);
    const int phi = (a0 + k * (ft & 3)) & 3;       // of the rows rho = b ft + r with rho mod 4 == k
    const int cs = (4 - phi) & 3;                  // first column of such a row on a vector boundary
    const int nv = ft >= cs ? (ft - cs) >> 2 : 0;  // vectors inside the row
    const int rk = (k - b * (ft & 3)) & 3;         // first such row of sample b
    const int cslabs = (ft / 4 + 63) / 64 > 0 ? (ft / 4 + 63) / 64 : 1;
    const int item = blockIdx.x * 4 + (threadIdx.x >> 6), rslab = item / cslabs, cslab = item - rslab * cslabs;
    const int r_mine = rk + 4 * (rslab * kBwdRows + lane);  // the row whose own term this lane holds
    if (rk + 4 * (rslab * kBwdRows) > ft) return;           // (row ft of the last sample is the end of the array)
    int c0_mine = -1;
    float t0_mine = 0.0f;
    if (r_mine < ft) match_loss_term(idx, w, ft, b, 0, r_mine, gb, c0_mine, t0_mine);
    const int j = cslab * 64 + lane, c = cs + 4 * j;
    const bool inside = j < nv;
    int r1[4] = {-1, -1, -1, -1};
    float t1[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (inside) {
#pragma unroll
        for (int u = 0; u < 4; ++u) match_loss_term(idx, w, ft, b, 1, c + u, gb, r1[u], t1[u]);
    }
    float* dst = out + ((int64_t)b * ft + rk + 4 * (rslab * kBwdRows)) * ft + c;
    for (int m = 0; m < kBwdRows; ++m) {  // (every lane walks the rows: lane m hands out the term of row m)
        const int r = rk + 4 * (rslab * kBwdRows + m);
        if (r >= ft) break;
        const int c0 = __builtin_amdgcn_readlane(c0_mine, m);
        const float t0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(t0_mine), m));
        if (inside)
            *reinterpret_cast<float4*>(dst) = make_float4(match_loss_grad(r, c, c0, t0, r1[0], t1[0]), match_loss_grad(r, c + 1, c0, t0, r1[1], t1[1]),
                                                          match_loss_grad(r, c + 2, c0, t0, r1[2], t1[2]), match_loss_grad(r, c + 3, c0, t0, r1[3], t1[3]));
        dst += (int64_t)4 * ft;
    }
    // the vector at the start of row r_mine, where it is none of the above
    if (cslab != 0 || (phi == 0 && ft >= 4) || r_mine > ft || (r_mine == ft && b != p.B - 1)) return;
    const int64_t e0 = ((int64_t)b * ft + r_mine) * ft - phi;
    float o[4];
    bool in[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int64_t e = e0 + u;
        in[u] = e >= 0 && e < total;
        o[u] = 0.0f;
        if (in[u]) {
            const int bb = (int)(e / ((int64_t)ft * ft)), rem = (int)(e - (int64_t)bb * ft * ft), r = rem / ft, cc = rem - r * ft;
            int c0, r1;
            float t0, t1;
            match_loss_term(idx, w, ft, bb, 0, r, gb, c0, t0);
            match_loss_term(idx, w, ft, bb, 1, cc, gb, r1, t1);
            o[u] = match_loss_grad(r, cc, c0, t0, r1, t1);
        }
    }
    if (in[0] && in[3]) {
        *reinterpret_cast<float4*>(out + e0) = make_float4(o[0], o[1], o[2], o[3]);
    } else {
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (in[u]) out[e0 + u] = o[u];
    }
}

}  // namespace e2emv

using namespace e2emv;

extern "C" int e2emv_gt_matches(e2emv_ctx* ctx, int B, int N, const float* d_kpts0, const float* d_kpts1, const float* d_K0,
                                const float* d_K1, const float* d_T0to1, const float* d_depth0, const float* d_depth1, int H,
                                int W, float max_matched_reproj_err, float min_unmatched_reproj_err, int64_t* d_indices,
                                float* d_weights, void* stream) {
    if (!ctx || !d_kpts0 || !d_kpts1 || !d_K0 || !d_K1 || !d_T0to1 || !d_depth0 || !d_depth1 || !d_indices || !d_weights)
        return E2EMV_EINVAL;
    E2EMV_ENTER(ctx, stream);
    if (B <= 0 || N <= 0 || H <= 0 || W <= 0) return set_err(ctx, E2EMV_ESHAPE, "gt_matches: B=%d N=%d H=%d W=%d", B, N, H, W);
    hipStream_t s = (hipStream_t)stream;
    auto al = [](size_t b) { return (b + 255) & ~size_t(255); };
    const size_t n2 = (size_t)2 * B * N;
    const size_t need = 2 * al(n2 * 2 * 4) + 4 * al(n2 * 4);
    int rc = ws_reserve(ctx, need);
    if (rc) return rc;
    GtParams p{};
    p.B = B; p.N = N; p.H = H; p.W = W;
    p.k0 = d_kpts0; p.k1 = d_kpts1; p.K0 = d_K0; p.K1 = d_K1; p.T01 = d_T0to1; p.depth0 = d_depth0; p.depth1 = d_depth1;
    p.max_matched = max_matched_reproj_err; p.min_unmatched = min_unmatched_reproj_err;
    char* w = ctx->d_ws;
    p.ki = (float*)w; w += al(n2 * 2 * 4);
    p.kto = (float*)w; w += al(n2 * 2 * 4);
    p.d = (float*)w; w += al(n2 * 4);
    p.dto = (float*)w; w += al(n2 * 4);
    p.emin = (float*)w; w += al(n2 * 4);
    p.amin = (int*)w;
    p.idx = d_indices; p.w = d_weights;
    prof_begin(ctx, PS_MISC, s);
    hipLaunchKernelGGL(gt_transform, dim3((N + 255) / 256, B, 2), dim3(256), 0, s, p);
    hipLaunchKernelGGL(gt_argmin, dim3((N + 3) / 4, B, 2), dim3(256), 0, s, p);
    hipLaunchKernelGGL(gt_finalize, dim3(B), dim3(256), 0, s, p);
    prof_end(ctx, s);
    E2EMV_CHECK_LAUNCH(ctx, "gt_matches kernels");
    return E2EMV_OK;
}

extern "C" int e2emv_match_loss(e2emv_ctx* ctx, int B, int N, const float* d_logZ, const int64_t* d_indices,
                                const float* d_weights, float* d_loss, void* stream) {
    if (!ctx || !d_logZ || !d_indices || !d_weights || !d_loss) return E2EMV_EINVAL;
    E2EMV_ENTER(ctx, stream);
    if (B <= 0 || N <= 0) return set_err(ctx, E2EMV_ESHAPE, "match_loss: B=%d N=%d", B, N);
    hipStream_t s = (hipStream_t)stream;
    int rc = ws_reserve(ctx, (size_t)B * 8 + 256);
    if (rc) return rc;
    double* partial = (double*)ctx->d_ws;
    prof_begin(ctx, PS_MISC, s);
    hipLaunchKernelGGL(match_loss_kernel, dim3(B), dim3(256), 0, s, B, N, d_logZ, d_indices, d_weights, partial);
    hipLaunchKernelGGL(match_loss_fold, dim3(1), dim3(1), 0, s, B, partial, d_loss);
    prof_end(ctx, s);
    E2EMV_CHECK_LAUNCH(ctx, "match_loss kernels");
    return E2EMV_OK;
}

extern "C" int e2emv_gt_matches_tuple(e2emv_ctx* ctx, int B, int T, int N, const float* const* d_kpts, const float* const* d_K,
                                      const float* const* d_pose, const float* const* d_depth, int H, int W,
                                      float max_matched_reproj_err, float min_unmatched_reproj_err, int64_t* d_indices,
                                      float* d_weights, void* stream) {
    if (!ctx || !d_kpts || !d_K || !d_pose || !d_depth || !d_indices || !d_weights) return E2EMV_EINVAL;
    E2EMV_ENTER(ctx, stream);
    if (T < 2 || T > E2EMV_MAX_TUPLE || B <= 0 || N <= 0 || H <= 0 || W <= 0)
        return set_err(ctx, E2EMV_ESHAPE, "gt_matches_tuple: B=%d T=%d N=%d H=%d W=%d", B, T, N, H, W);
    GtTupleParams t{};
    t.B = B; t.N = N; t.H = H; t.W = W;
    for (int m = 0; m < T; ++m) {
        if (!d_kpts[m] || !d_K[m] || !d_pose[m] || !d_depth[m]) return set_err(ctx, E2EMV_EINVAL, "gt_matches_tuple: null input for image %d", m);
        t.kpts[m] = d_kpts[m]; t.K[m] = d_K[m]; t.pose[m] = d_pose[m]; t.depth[m] = d_depth[m];
    }
    int P = 0;
    for (int j = 0; j < T; ++j)
        for (int i = 0; i < j; ++i, ++P) { t.pi[P] = (unsigned char)i; t.pj[P] = (unsigned char)j; }
    t.max_matched = max_matched_reproj_err; t.min_unmatched = min_unmatched_reproj_err;
    hipStream_t s = (hipStream_t)stream;
    auto al = [](size_t b) { return (b + 255) & ~size_t(255); };
    const size_t n2 = (size_t)2 * B * N;
    t.sz2 = al(n2 * 2 * 4); t.sz1 = al(n2 * 4);
    t.ws_stride = 2 * t.sz2 + 4 * t.sz1;
    const size_t sz_T = al((size_t)P * B * 16 * 4);
    int rc = ws_reserve(ctx, sz_T + (size_t)P * t.ws_stride);
    if (rc) return rc;
    t.T01 = (float*)ctx->d_ws;
    t.ws = ctx->d_ws + sz_T;
    t.idx = d_indices; t.w = d_weights;
    prof_begin(ctx, PS_MISC, s);
    hipLaunchKernelGGL(gt_tuple_relative_pose, dim3((B + 63) / 64, P), dim3(64), 0, s, t);
    hipLaunchKernelGGL(gt_tuple_transform, dim3((N + 255) / 256, B, 2 * P), dim3(256), 0, s, t);
    hipLaunchKernelGGL(gt_tuple_argmin, dim3((N + 3) / 4, B, 2 * P), dim3(256), 0, s, t);
    hipLaunchKernelGGL(gt_tuple_finalize, dim3(B, P), dim3(256), 0, s, t);
    prof_end(ctx, s);
    E2EMV_CHECK_LAUNCH(ctx, "gt_matches_tuple kernels");
    return E2EMV_OK;
}

extern "C" int e2emv_match_loss_tuple(e2emv_ctx* ctx, int P, int B, int N, const float* const* d_logZ, const int64_t* d_indices,
                                      const float* d_weights, float* d_loss, float* d_pair_loss, void* stream) {
    if (!ctx || !d_logZ || !d_indices || !d_weights || !d_loss) return E2EMV_EINVAL;
    E2EMV_ENTER(ctx, stream);
    if (P <= 0 || P > kMaxGroups || B <= 0 || N <= 0) return set_err(ctx, E2EMV_ESHAPE, "match_loss_tuple: pairs=%d B=%d N=%d", P, B, N);
    MatchLossTupleParams p{};
    p.B = B; p.N = N; p.idx = d_indices; p.w = d_weights;
    for (int q = 0; q < P; ++q) {
        if (!d_logZ[q]) return set_err(ctx, E2EMV_EINVAL, "match_loss_tuple: null scores for pair %d", q);
        p.logZ[q] = d_logZ[q];
    }
    hipStream_t s = (hipStream_t)stream;
    int rc = ws_reserve(ctx, (size_t)P * B * 8 + 256);
    if (rc) return rc;
    p.partial = (double*)ctx->d_ws;
    prof_begin(ctx, PS_MISC, s);
    hipLaunchKernelGGL(match_loss_tuple_kernel, dim3(B, P), dim3(256), 0, s, p);
    hipLaunchKernelGGL(match_loss_tuple_fold, dim3(1), dim3(1), 0, s, P, B, p.partial, d_loss, d_pair_loss);
    prof_end(ctx, s);
    E2EMV_CHECK_LAUNCH(ctx, "match_loss_tuple kernels");
    return E2EMV_OK;
}

extern "C" int e2emv_match_loss_tuple_backward(e2emv_ctx* ctx, int P, int B, int N, const int64_t* d_indices, const float* d_weights,
                                               const float* d_g, float* const* d_glogZ, void* stream) {
    if (!ctx || !d_indices || !d_weights || !d_g || !d_glogZ) return E2EMV_EINVAL;
    E2EMV_ENTER(ctx, stream);
    // (N+1)^2 has to fit an int (the position inside a sample), 4 B the grid's y
    if (P <= 0 || P > kMaxGroups || B <= 0 || B > 16383 || N <= 0 || N > 46338)
        return set_err(ctx, E2EMV_ESHAPE, "match_loss_tuple_backward: pairs=%d B=%d N=%d", P, B, N);
    MatchLossBwdParams p{};
    p.B = B; p.N = N; p.idx = d_indices; p.w = d_weights; p.g = d_g;
    for (int q = 0; q < P; ++q) p.glogZ[q] = d_glogZ[q];
    const int ft = N + 1, cslabs = (ft / 4 + 63) / 64 > 0 ? (ft / 4 + 63) / 64 : 1;
    const int rslabs = ((ft + 1 + 3) / 4 + kBwdRows - 1) / kBwdRows;  // rows of one phase of a sample, the array's end included
    hipLaunchKernelGGL(match_loss_tuple_backward_kernel, dim3((rslabs * cslabs + 3) / 4, 4 * B, P), dim3(256), 0, (hipStream_t)stream, p);
    E2EMV_CHECK_LAUNCH(ctx, "match_loss_tuple_backward_kernel");
    return E2EMV_OK;
}
