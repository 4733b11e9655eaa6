// Multi-view weighted reprojection bundle adjustment on the device (SURVEY.md 8(f) "next" row 3).
//
// Replaces the reference's `bundle_adjuster` executable: pose_optimization/multi_view/bundle_adjustment/
// problem/include/ba_problem.h:60-151 (the two reprojection functors), problem/src/ba_problem.cpp:8-88 (CSV parser),
// :98-113 (WriteResult), :115-157 (Solve = Ceres, DENSE_SCHUR, squared loss, default options), bundle_adjuster.cpp:7-23.
// Ceres 2.0 is absent here; the minimiser restates its documented Levenberg-Marquardt trust-region loop (see
// oracle/mvba.py, which this kernel is tested against to ~1e-9, and the reference's gtest known answers).
//
// Where the reference hands the whole problem to a CPU solver (autodiff Jacobians, dense Schur on one thread), ONE
// workgroup of 512 threads runs the entire optimisation without leaving the GPU:
//   A  thread / observation : residual + analytic Jacobians (2x6 camera, 2x3 point), cost
//   B  thread / point       : V_p = sum Jp^T Jp, g_p, damping, V_p^-1, Y_o = (Jc^T Jp) V_p^-1
//   C  wave   / camera      : U_c = sum Jc^T Jc, g_c            (per-camera observation lists, shuffle reductions)
//   E  wave   / camera pair : S_ab = [a==b](U_a + D_a) - sum_p Y_oa W_ob^T,  rhs_a = -g_a + sum_p Y_oa g_p
//   F  wave 0               : Cholesky + two triangular solves of the reduced camera system (<= 48 x 48, LDS)
//   G  thread / point       : dp = -V_p^-1 (g_p + sum_o W_o^T dc), candidate point
//   H  thread / observation : model cost change -m.(r + m/2), m = J d;  cost at the candidate
//   I  thread 0             : step acceptance, trust-region radius, termination tests
// All arithmetic fp64; every reduction has a fixed order (no atomics), so results are run-to-run identical.
// Opt-in robust loss (Huber, Cauchy; mvba.h): the kernel is a template over it, phases A and H apply Ceres' corrector and sum rho(s);
// without a loss it is the reference's squared loss (ba_problem.cpp:135,144 pass NULL) and the arithmetic it always was.
// Quirk kept (ba_problem.cpp:129-137): observations of the fixed camera are predicted with the identity pose and that
// camera's parameters are written back untouched.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <fstream>
#include <iomanip>

#include "common.h"
#include "mv_host.h"
#include "mvba.h"

namespace e2emv {

// (mv_block_reduce, mv_transform and mvba_kernel<LOSS, MODE> itself: mvba.h - the backward pass, mvba_backward.hip, replays the same statement)

// one thread per point
__global__ void mv_triangulate_kernel(int n, const double* P0, const double* P1, const double* x0, const double* x1, double* xyz) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    mv_dlt(P0, P1, x0[2 * i], x0[2 * i + 1], x1[2 * i], x1[2 * i + 1], xyz + 3 * i);
}


// ---- the in-memory path for a whole batch of tuples (multi_view.solve_tuple_poses_batch) ---------------------------------------
struct MvCollectArgs {
    int B, P, N, channels;  // problems = B * P, problem (b, q) at index b * P + q; N = keypoints of the first image = row stride
    float thresh;
    int n1[kMvMaxPairs];               // keypoints of the second image
    const float* k0[kMvMaxPairs];      // [B,N,2]
    const float* k1[kMvMaxPairs];      // [B,n1,2]
    const int64_t* match[kMvMaxPairs]; // [B,N] or NULL (no matches for this pair)
    const float* conf[kMvMaxPairs];    // [B,N,channels]
    float *o0, *o1, *oc;               // [B*P,N,2] x2, [B*P,N]
    int* count;                        // [B*P]
    const float* gin;                  // backward: [B*P,N] dLoss/d(oc)
    float* gout[kMvMaxPairs];          // backward: [B,N,channels] dLoss/d(conf) or NULL (pair left out)
};

// Ordered compaction, one workgroup per problem: keypoint n of the first image is kept when it has a match and every confidence
// channel is above the threshold; the kept rows keep their order (ballot prefix inside a wave, wave totals through LDS, a
// running base across the chunks of 256) because every later sum runs over them in that order.  Rows behind the count read 0.
// BWD: the same walk scatters gin back: row n of a kept match gets the value at its slot in channel 0, everything else of gout 0.
template <bool BWD>
__global__ __launch_bounds__(kMvRowThreads) void mv_collect_kernel(MvCollectArgs a) {
    __shared__ int s_wave[kMvRowThreads / 64];
    const int pp = blockIdx.x, b = pp / a.P, q = pp - b * a.P, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int N = a.N, n1 = a.n1[q];
    const int64_t* match = a.match[q] ? a.match[q] + size_t(b) * N : nullptr;
    const float* conf = a.conf[q] + size_t(b) * N * a.channels;
    if (BWD && !a.gout[q]) return;  // (the whole workgroup)
    const float* k0 = BWD ? nullptr : a.k0[q] + size_t(b) * N * 2;
    const float* k1 = BWD ? nullptr : a.k1[q] + size_t(b) * n1 * 2;
    float* o0 = BWD ? nullptr : a.o0 + size_t(pp) * N * 2;
    float* o1 = BWD ? nullptr : a.o1 + size_t(pp) * N * 2;
    float* oc = BWD ? nullptr : a.oc + size_t(pp) * N;
    const float* gin = BWD ? a.gin + size_t(pp) * N : nullptr;
    float* gout = BWD ? a.gout[q] + size_t(b) * N * a.channels : nullptr;
    int base = 0;
    if (match) {
        for (int c0 = 0; c0 < N; c0 += kMvRowThreads) {
            const int n = c0 + tid;
            int64_t m = -1;
            bool keep = false;
            if (n < N) {
                m = match[n];
                keep = m >= 0 && m < n1;
                for (int c = 0; c < a.channels; ++c) keep = keep && conf[size_t(n) * a.channels + c] > a.thresh;
            }
            const unsigned long long mask = __ballot(keep);
            if (lane == 0) s_wave[wave] = __popcll(mask);
            __syncthreads();
            int off = base + __popcll(mask & ((1ull << lane) - 1ull)), total = 0;
            for (int w = 0; w < kMvRowThreads / 64; ++w) {
                if (w < wave) off += s_wave[w];
                total += s_wave[w];
            }
            if (BWD) {
                if (n < N)
                    for (int c = 0; c < a.channels; ++c) gout[size_t(n) * a.channels + c] = (keep && c == 0) ? gin[off] : 0.f;
            } else if (keep) {
                o0[2 * off] = k0[2 * n]; o0[2 * off + 1] = k0[2 * n + 1];
                o1[2 * off] = k1[2 * m]; o1[2 * off + 1] = k1[2 * m + 1];
                oc[off] = conf[size_t(n) * a.channels];
            }
            base += total;
            __syncthreads();
        }
    }
    if (BWD) {
        if (!match)
            for (int i = tid; i < N * a.channels; i += kMvRowThreads) gout[i] = 0.f;
        return;
    }
    for (int n = base + tid; n < N; n += kMvRowThreads) {
        o0[2 * n] = 0.f; o0[2 * n + 1] = 0.f; o1[2 * n] = 0.f; o1[2 * n + 1] = 0.f; oc[n] = 0.f;
    }
    if (tid == 0) a.count[pp] = base;
}

// what the host knows of pair block q of tuple b once the match counts are on the host: with one point per match and two
// observations per point, every index list of the bundle adjustment has a closed form in the prefix sums of the counts
struct MvPairRec {
    int i, j, count;
    int pt_base;       // first point of the block; its observations are 2 * pt_base + [0, count) (image i) and + count + [0, count) (image j)
    int list_i, list_j;  // where the block's observations start in the observation lists of cameras i and j
};

struct MvBuildArgs {
    int P, T, N, kdim, intr_batch;
    const float* k0; const float* k1; const float* conf;  // collected: [B*P,N,2] x2, [B*P,N]
    const float* intr[kMvMaxCams];                         // [intr_batch,kdim,kdim] per image
    const double* proj;                                    // [B,T,3,4] world -> camera
    const MvPairRec* pairs;                                // [B*P]
    const MvbaArgs* recs;                                  // [B] the problems being built
    double loss_scale;                                     // relative scale of the robust loss (0: no loss)
};

// Bundle-adjustment problem of every tuple from the collected matches (write_bundle_adjust_problem without the text): thread =
// match.  blockIdx.y = pair block, blockIdx.x = chunk of 256 matches.
__global__ __launch_bounds__(kMvRowThreads) void mv_build_kernel(MvBuildArgs g) {
    __shared__ double s_red[kMvRowThreads / 64];
    const int pp = blockIdx.y, b = pp / g.P, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const MvPairRec rec = g.pairs[pp];
    const MvbaArgs& a = g.recs[b];
    // confidences of the tuple summed in fp64, always in this order (every workgroup of the tuple repeats it and gets the same
    // bits): thread-strided inside a pair block, blocks in pair order, then lanes, then waves
    double sum = 0.0;
    for (int q = 0; q < g.P; ++q) {
        const int cnt = g.pairs[b * g.P + q].count;
        const float* cf = g.conf + size_t(b * g.P + q) * g.N;
        for (int m = tid; m < cnt; m += kMvRowThreads) sum += double(cf[m]);
    }
    sum = wave_sum_d(sum);
    if (lane == 0) s_red[wave] = sum;
    __syncthreads();
    sum = s_red[0];
    for (int w = 1; w < kMvRowThreads / 64; ++w) sum += s_red[w];
    const double half_total = 0.5 * (2.0 * sum + 1e-3);  // every confidence is seen by two observations (normalize_confidences)
    if (blockIdx.x == 0 && blockIdx.y == b * g.P && tid == 0) {
        const_cast<int*>(a.pt_start)[a.P] = 2 * a.P;
        // the loss acts on confidence x residual whatever the tuple's size: its scale is divided by what the confidences are
        if (g.loss_scale > 0.0) const_cast<MvbaArgs&>(a).loss_a = g.loss_scale / half_total;
    }
    const int m = blockIdx.x * kMvRowThreads + tid;
    if (m >= rec.count) return;
    const size_t row = size_t(pp) * g.N + m;
    const int pt = rec.pt_base + m, oi = 2 * rec.pt_base + m, oj = oi + rec.count;
    double x[4];
#pragma unroll
    for (int v = 0; v < 2; ++v) {
        const int img = v ? rec.j : rec.i;
        const float* K = g.intr[img] + (g.intr_batch == 1 ? 0 : size_t(b) * g.kdim * g.kdim);
        const float* kp = (v ? g.k1 : g.k0) + 2 * row;
        // pixel -> normalised camera coordinates in fp32 like the host path: one rounded subtraction, one rounded division
        const float xn = (kp[0] - K[2]) / K[0], yn = (kp[1] - K[g.kdim + 2]) / K[g.kdim + 1];
        x[2 * v] = double(xn); x[2 * v + 1] = double(yn);
    }
    const double w = double(g.conf[row]) / half_total;
    int* cam_idx = const_cast<int*>(a.cam_idx); int* pt_idx = const_cast<int*>(a.pt_idx);
    double* obs = const_cast<double*>(a.obs); double* wts = const_cast<double*>(a.wts);
    cam_idx[oi] = rec.i; cam_idx[oj] = rec.j;
    pt_idx[oi] = pt; pt_idx[oj] = pt;
    obs[2 * oi] = x[0]; obs[2 * oi + 1] = x[1]; obs[2 * oj] = x[2]; obs[2 * oj + 1] = x[3];
    wts[2 * oi] = w; wts[2 * oi + 1] = w; wts[2 * oj] = w; wts[2 * oj + 1] = w;
    const_cast<int*>(a.pt_start)[pt] = 2 * pt;
    const_cast<int*>(a.pt_obs)[2 * pt] = oi;
    const_cast<int*>(a.pt_obs)[2 * pt + 1] = oj;
    const_cast<int*>(a.cam_obs)[rec.list_i + m] = oi;
    const_cast<int*>(a.cam_obs)[rec.list_j + m] = oj;
    mv_dlt(g.proj + size_t(b * g.T + rec.i) * 12, g.proj + size_t(b * g.T + rec.j) * 12, x[0], x[1], x[2], x[3], a.pts + 3 * size_t(pt));
}

// Reverse of the weights mv_build_kernel hands the solver: w = conf / H on the four weight entries of a match (x, y of both
// observations), H = 0.5 (2 sum conf + 1e-3) with the tuple's sum.  With s_m the sum of the four dLoss/dw of match m:
// dLoss/dconf_m = s_m / H - (sum_m' s_m' conf_m') / H^2.  One workgroup per tuple, the sums in the build's order; rows behind the
// count get 0.
struct MvWeightsBwdArgs {
    int P, N;
    const float* conf;          // collected [B*P,N]
    const MvPairRec* pairs;     // [B*P]
    const MvbaBwdArgs* bw;      // [B]: g_w
    float* gconf;               // [B*P,N]
};
__global__ __launch_bounds__(kMvRowThreads) void mv_weights_backward_kernel(MvWeightsBwdArgs g) {
    __shared__ double s_red[2 * (kMvRowThreads / 64)];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const double* gw = g.bw[b].g_w;
    double sum = 0.0, dot = 0.0;
    for (int q = 0; q < g.P; ++q) {
        const MvPairRec rec = g.pairs[b * g.P + q];
        const float* cf = g.conf + size_t(b * g.P + q) * g.N;
        for (int m = tid; m < rec.count; m += kMvRowThreads) {
            const size_t oi = 2 * size_t(rec.pt_base) + m, oj = oi + rec.count;
            const double c = double(cf[m]);
            sum += c;
            dot += (gw[2 * oi] + gw[2 * oi + 1] + gw[2 * oj] + gw[2 * oj + 1]) * c;
        }
    }
    sum = wave_sum_d(sum); dot = wave_sum_d(dot);
    if (lane == 0) { s_red[wave] = sum; s_red[kMvRowThreads / 64 + wave] = dot; }
    __syncthreads();
    sum = s_red[0]; dot = s_red[kMvRowThreads / 64];
    for (int w = 1; w < kMvRowThreads / 64; ++w) { sum += s_red[w]; dot += s_red[kMvRowThreads / 64 + w]; }
    const double H = 0.5 * (2.0 * sum + 1e-3);
    for (int q = 0; q < g.P; ++q) {
        const MvPairRec rec = g.pairs[b * g.P + q];
        float* out = g.gconf + size_t(b * g.P + q) * g.N;
        for (int m = tid; m < g.N; m += kMvRowThreads) {
            float v = 0.f;
            if (m < rec.count) {
                const size_t oi = 2 * size_t(rec.pt_base) + m, oj = oi + rec.count;
                v = float((gw[2 * oi] + gw[2 * oi + 1] + gw[2 * oj] + gw[2 * oj + 1]) / H - dot / (H * H));
            }
            out[m] = v;
        }
    }
}

// (MvLayout: mvba.h)
MvLayout mv_layout(char* base, size_t n, size_t totC, size_t totP, size_t totO, size_t extra) {
    MvLayout L{};
    size_t off = 0;
    auto take = [&](size_t bytes) { char* q = base + off; off += (bytes + 255) & ~size_t(255); return q; };
    L.recs = reinterpret_cast<MvbaArgs*>(take(n * sizeof(MvbaArgs)));
    L.cams = reinterpret_cast<double*>(take(totC * 6 * 8));
    L.cam_start = reinterpret_cast<int*>(take((totC + n) * 4));
    L.extra = take(extra);
    L.upload_bytes = off;
    auto dbl = [&](size_t k) { return reinterpret_cast<double*>(take(k * 8)); };
    auto i32 = [&](size_t k) { return reinterpret_cast<int*>(take(k * 4)); };
    L.pts = dbl(3 * totP); L.gp = dbl(3 * totP); L.dp = dbl(3 * totP); L.scale_p = dbl(3 * totP); L.cand = dbl(3 * totP); L.Vinv = dbl(6 * totP);
    L.obs = dbl(2 * totO); L.wts = dbl(2 * totO); L.r = dbl(2 * totO); L.Jc = dbl(12 * totO); L.Jp = dbl(6 * totO); L.Y = dbl(18 * totO);
    L.summary = dbl(4 * n);
    L.cam_idx = i32(totO); L.pt_idx = i32(totO); L.pt_obs = i32(totO); L.cam_obs = i32(totO); L.pt_start = i32(totP + n);
    L.bytes = off;
    return L;
}

// record of problem k: its sizes and its slices (c0 / p0 / o0 = cameras / points / observations of the problems before it)
MvbaArgs mv_record(const MvLayout& L, size_t k, size_t c0, size_t p0, size_t o0, int C, int fixed, int P, int O, int max_iters,
                   const double* intr, double loss_a) {
    MvbaArgs a{};
    a.loss_a = loss_a;
    a.C = C; a.fixed = fixed; a.P = P; a.O = O; a.max_iters = max_iters;
    a.fx = intr[0]; a.fy = intr[1]; a.cx = intr[2]; a.cy = intr[3];
    a.cam_idx = L.cam_idx + o0; a.pt_idx = L.pt_idx + o0; a.pt_obs = L.pt_obs + o0; a.cam_obs = L.cam_obs + o0;
    a.pt_start = L.pt_start + p0 + k; a.cam_start = L.cam_start + c0 + k;
    a.obs = L.obs + 2 * o0; a.wts = L.wts + 2 * o0;
    a.cams = L.cams + 6 * c0; a.pts = L.pts + 3 * p0;
    a.r = L.r + 2 * o0; a.Jc = L.Jc + 12 * o0; a.Jp = L.Jp + 6 * o0; a.Y = L.Y + 18 * o0;
    a.Vinv = L.Vinv + 6 * p0; a.gp = L.gp + 3 * p0; a.dp = L.dp + 3 * p0; a.scale_p = L.scale_p + 3 * p0; a.cand = L.cand + 3 * p0;
    a.summary = L.summary + 4 * k;
    return a;
}

int mv_launch_ba(e2emv_ctx* ctx, const MvLayout& L, int n, hipStream_t s, int loss) {
    prof_begin(ctx, PS_W8PT, s);
    if (loss == kLossHuber) hipLaunchKernelGGL((mvba_kernel<kLossHuber, kLmRun>), dim3(n), dim3(kMvThreads), 0, s, L.recs, (const MvbaBwdArgs*)nullptr);
    else if (loss == kLossCauchy) hipLaunchKernelGGL((mvba_kernel<kLossCauchy, kLmRun>), dim3(n), dim3(kMvThreads), 0, s, L.recs, (const MvbaBwdArgs*)nullptr);
    else hipLaunchKernelGGL((mvba_kernel<kLossNone, kLmRun>), dim3(n), dim3(kMvThreads), 0, s, L.recs, (const MvbaBwdArgs*)nullptr);
    E2EMV_CHECK_LAUNCH(ctx, "mvba_kernel");
    prof_end(ctx, s);
    return E2EMV_OK;
}

// what the tuple entry points bring back once the solver has run: cameras as extrinsics, summaries and (loss_a_out, may be
// NULL) the loss scale each record carried, [B]
int mv_tuple_results(e2emv_ctx* ctx, const MvLayout& L, int B, int T, double* out_extr, double* summary, double* loss_a_out, hipStream_t s) {
    std::vector<double> cams(size_t(B) * T * 6), sm(size_t(B) * 4);
    std::vector<MvbaArgs> recs(loss_a_out ? size_t(B) : 0);
    E2EMV_HIP(ctx, hipMemcpyAsync(cams.data(), L.cams, sizeof(double) * cams.size(), hipMemcpyDeviceToHost, s));
    E2EMV_HIP(ctx, hipMemcpyAsync(sm.data(), L.summary, sizeof(double) * sm.size(), hipMemcpyDeviceToHost, s));
    if (loss_a_out) E2EMV_HIP(ctx, hipMemcpyAsync(recs.data(), L.recs, sizeof(MvbaArgs) * recs.size(), hipMemcpyDeviceToHost, s));
    E2EMV_HIP(ctx, hipStreamSynchronize(s));
    for (size_t v = 0; v < size_t(B) * T; ++v) mv_cam_to_extr(&cams[6 * v], out_extr + 16 * v);
    if (summary) std::memcpy(summary, sm.data(), sizeof(double) * sm.size());
    for (size_t b = 0; b < recs.size(); ++b) loss_a_out[b] = recs[b].loss_a;
    return E2EMV_OK;
}

void mv_extr_to_cam(const double* E /* 4x4 row-major */, double* cam) {
    const double R[9] = {E[0], E[4], E[8], E[1], E[5], E[9], E[2], E[6], E[10]};  // column-major
    mv::R_to_aa(R, cam);
    cam[3] = E[3]; cam[4] = E[7]; cam[5] = E[11];
}
void mv_cam_to_extr(const double* cam, double* E) {
    double R[9];
    mv::aa_to_R(cam, R);
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) E[4 * r + c] = R[3 * c + r];
        E[4 * r + 3] = cam[3 + r];
    }
    E[12] = 0; E[13] = 0; E[14] = 0; E[15] = 1;
}

}  // namespace e2emv

using namespace e2emv;

namespace e2emv {
// the loss arguments of the *_loss entry points: a known code, and with a loss a finite scale > 0; *scale = 0 without a loss
int mv_check_loss(e2emv_ctx* ctx, const char* who, int loss, double* scale) {
    if (loss != kLossNone && loss != kLossHuber && loss != kLossCauchy) return set_err(ctx, E2EMV_EINVAL, "%s: unknown loss code %d", who, loss);
    if (loss == kLossNone) { *scale = 0.0; return E2EMV_OK; }
    if (!std::isfinite(*scale) || !(*scale > 0.0)) return set_err(ctx, E2EMV_EINVAL, "%s: the loss scale must be finite and > 0 (got %g)", who, *scale);
    return E2EMV_OK;
}
}  // namespace e2emv

namespace e2emv {
int mv_batch_check(e2emv_ctx* ctx, const char* who, int n_problems, const int32_t* n_cams, const int32_t* fixed_cam, const double* intr,
                   const int64_t* pt_off, const int64_t* obs_off, const int32_t* cam_idx, const int32_t* pt_idx, const double* obs_xy,
                   const double* obs_w, const double* cams, const double* pts, size_t* totC_out, size_t* totP_out, size_t* totO_out) {
    if (n_problems < 1 || !n_cams || !fixed_cam || !intr || !pt_off || !obs_off || !cams)
        return set_err(ctx, E2EMV_EINVAL, "%s: bad argument (n_problems >= 1, no NULL size / offset array)", who);
    const size_t n = size_t(n_problems);
    if (pt_off[0] != 0 || obs_off[0] != 0) return set_err(ctx, E2EMV_ESHAPE, "%s: offsets must start at 0", who);
    size_t totC = 0;
    for (size_t k = 0; k < n; ++k) {
        if (n_cams[k] < 1 || n_cams[k] > kMvMaxCams)
            return set_err(ctx, E2EMV_EINVAL, "%s: problem %zu has %d cameras (1 <= n_cams <= %d)", who, k, n_cams[k], kMvMaxCams);
        if (pt_off[k + 1] < pt_off[k] || obs_off[k + 1] < obs_off[k] || pt_off[k + 1] - pt_off[k] > INT32_MAX / 8 || obs_off[k + 1] - obs_off[k] > INT32_MAX / 32)
            return set_err(ctx, E2EMV_ESHAPE, "%s: offsets of problem %zu are not monotone (or the problem is too large)", who, k);
        totC += size_t(n_cams[k]);
    }
    const size_t totP = size_t(pt_off[n]), totO = size_t(obs_off[n]);
    if ((totP && !pts) || (totO && (!cam_idx || !pt_idx || !obs_xy || !obs_w)))
        return set_err(ctx, E2EMV_EINVAL, "%s: NULL array for %zu points / %zu observations", who, totP, totO);
    for (size_t k = 0; k < n; ++k) {
        const int C = n_cams[k], P = int(pt_off[k + 1] - pt_off[k]);
        for (int64_t o = obs_off[k]; o < obs_off[k + 1]; ++o)
            if (cam_idx[o] < 0 || cam_idx[o] >= C || pt_idx[o] < 0 || pt_idx[o] >= P)
                return set_err(ctx, E2EMV_EINVAL, "%s: observation %lld of problem %zu refers to camera %d / point %d", who,
                               (long long)(o - obs_off[k]), k, cam_idx[o], pt_idx[o]);
    }
    *totC_out = totC; *totP_out = totP; *totO_out = totO;
    return E2EMV_OK;
}

int mv_batch_upload(e2emv_ctx* ctx, int n_problems, const int32_t* n_cams, const int32_t* fixed_cam, const double* intr, const int64_t* pt_off,
                    const int64_t* obs_off, const int32_t* cam_idx, const int32_t* pt_idx, const double* obs_xy, const double* obs_w,
                    const double* cams, const double* pts, int max_iterations, double loss_scale, size_t totC, size_t totP, size_t totO,
                    size_t tail, MvLayout* Lout, hipStream_t s) {
    const size_t n = size_t(n_problems);
    const int rc = ws_reserve(ctx, mv_layout(nullptr, n, totC, totP, totO, 0).bytes + tail);
    if (rc) return rc;
    const MvLayout L = mv_layout(ctx->d_ws, n, totC, totP, totO, 0);
    // observation lists per point and per camera (stable order -> deterministic sums), indices local to their problem
    std::vector<MvbaArgs> recs(n);
    std::vector<int> pstart(totP + n, 0), pobs(totO), cstart(totC + n, 0), cobs(totO);
    size_t c0 = 0;
    for (size_t k = 0; k < n; ++k) {
        const size_t p0 = size_t(pt_off[k]), o0 = size_t(obs_off[k]);
        const int C = n_cams[k], P = int(pt_off[k + 1] - pt_off[k]), O = int(obs_off[k + 1] - obs_off[k]);
        int* ps = pstart.data() + p0 + k;
        int* cs = cstart.data() + c0 + k;
        const int32_t* ci = cam_idx + o0;
        const int32_t* pi = pt_idx + o0;
        for (int o = 0; o < O; ++o) { ++ps[pi[o] + 1]; ++cs[ci[o] + 1]; }
        for (int p = 0; p < P; ++p) ps[p + 1] += ps[p];
        for (int c = 0; c < C; ++c) cs[c + 1] += cs[c];
        std::vector<int> pf(ps, ps + P), cf(cs, cs + C);
        for (int o = 0; o < O; ++o) { pobs[o0 + pf[pi[o]]++] = o; cobs[o0 + cf[ci[o]]++] = o; }
        recs[k] = mv_record(L, k, c0, p0, o0, C, fixed_cam[k], P, O, max_iterations, intr + 4 * k, loss_scale);
        c0 += size_t(C);
    }
    E2EMV_HIP(ctx, hipMemcpyAsync(L.recs, recs.data(), sizeof(MvbaArgs) * n, hipMemcpyHostToDevice, s));
    E2EMV_HIP(ctx, hipMemcpyAsync(L.cams, cams, sizeof(double) * 6 * totC, hipMemcpyHostToDevice, s));
    E2EMV_HIP(ctx, hipMemcpyAsync(L.cam_start, cstart.data(), sizeof(int) * (totC + n), hipMemcpyHostToDevice, s));
    E2EMV_HIP(ctx, hipMemcpyAsync(L.pt_start, pstart.data(), sizeof(int) * (totP + n), hipMemcpyHostToDevice, s));
    if (totP) E2EMV_HIP(ctx, hipMemcpyAsync(L.pts, pts, sizeof(double) * 3 * totP, hipMemcpyHostToDevice, s));
    if (totO) {
        E2EMV_HIP(ctx, hipMemcpyAsync(L.obs, obs_xy, sizeof(double) * 2 * totO, hipMemcpyHostToDevice, s));
        E2EMV_HIP(ctx, hipMemcpyAsync(L.wts, obs_w, sizeof(double) * 2 * totO, hipMemcpyHostToDevice, s));
        E2EMV_HIP(ctx, hipMemcpyAsync(L.cam_idx, cam_idx, sizeof(int) * totO, hipMemcpyHostToDevice, s));
        E2EMV_HIP(ctx, hipMemcpyAsync(L.pt_idx, pt_idx, sizeof(int) * totO, hipMemcpyHostToDevice, s));
        E2EMV_HIP(ctx, hipMemcpyAsync(L.pt_obs, pobs.data(), sizeof(int) * totO, hipMemcpyHostToDevice, s));
        E2EMV_HIP(ctx, hipMemcpyAsync(L.cam_obs, cobs.data(), sizeof(int) * totO, hipMemcpyHostToDevice, s));
    }
    E2EMV_HIP(ctx, hipStreamSynchronize(s));  // the host staging vectors die at return
    *Lout = L;
    return E2EMV_OK;
}
}  // namespace e2emv

extern "C" int e2emv_mv_bundle_adjust_batch_loss(e2emv_ctx* ctx, int n_problems, const int32_t* n_cams, const int32_t* fixed_cam,
                                                 const double* intr, const int64_t* pt_off, const int64_t* obs_off, const int32_t* cam_idx,
                                                 const int32_t* pt_idx, const double* obs_xy, const double* obs_w, double* cams, double* pts,
                                                 int max_iterations, double* summary, int loss, double loss_scale, void* stream) {
    if (!ctx) return E2EMV_EINVAL;
    E2EMV_ENTER(ctx, stream);
    const int lc = mv_check_loss(ctx, "mv_bundle_adjust_batch", loss, &loss_scale);
    if (lc) return lc;
    size_t totC = 0, totP = 0, totO = 0;
    int rc = mv_batch_check(ctx, "mv_bundle_adjust_batch", n_problems, n_cams, fixed_cam, intr, pt_off, obs_off, cam_idx, pt_idx, obs_xy, obs_w, cams, pts,
                            &totC, &totP, &totO);
    if (rc) return rc;
    const size_t n = size_t(n_problems);
    hipStream_t s = (hipStream_t)stream;
    MvLayout L;
    rc = mv_batch_upload(ctx, n_problems, n_cams, fixed_cam, intr, pt_off, obs_off, cam_idx, pt_idx, obs_xy, obs_w, cams, pts, max_iterations, loss_scale,
                         totC, totP, totO, 0, &L, s);
    if (rc) return rc;
    const int lrc = mv_launch_ba(ctx, L, n_problems, s, loss);
    if (lrc) return lrc;
    E2EMV_HIP(ctx, hipMemcpyAsync(cams, L.cams, sizeof(double) * 6 * totC, hipMemcpyDeviceToHost, s));
    if (totP) E2EMV_HIP(ctx, hipMemcpyAsync(pts, L.pts, sizeof(double) * 3 * totP, hipMemcpyDeviceToHost, s));
    std::vector<double> sm(4 * n);
    E2EMV_HIP(ctx, hipMemcpyAsync(sm.data(), L.summary, sizeof(double) * 4 * n, hipMemcpyDeviceToHost, s));
    E2EMV_HIP(ctx, hipStreamSynchronize(s));
    if (summary) std::memcpy(summary, sm.data(), sizeof(double) * 4 * n);
    return E2EMV_OK;
}

extern "C" int e2emv_mv_bundle_adjust_batch(e2emv_ctx* ctx, int n_problems, const int32_t* n_cams, const int32_t* fixed_cam,
                                            const double* intr, const int64_t* pt_off, const int64_t* obs_off, const int32_t* cam_idx,
                                            const int32_t* pt_idx, const double* obs_xy, const double* obs_w, double* cams, double* pts,
                                            int max_iterations, double* summary, void* stream) {
    return e2emv_mv_bundle_adjust_batch_loss(ctx, n_problems, n_cams, fixed_cam, intr, pt_off, obs_off, cam_idx, pt_idx, obs_xy, obs_w, cams, pts,
                                             max_iterations, summary, kLossNone, 0.0, stream);
}

extern "C" int e2emv_mv_bundle_adjust(e2emv_ctx* ctx, int n_cams, int fixed_cam, int n_pts, int n_obs, const double* intr,
                                      const int32_t* cam_idx, const int32_t* pt_idx, const double* obs_xy, const double* obs_w,
                                      double* cams, double* pts, int max_iterations, double* summary, void* stream) {
    if (!ctx) return E2EMV_EINVAL;
    E2EMV_ENTER(ctx, stream);
    if (n_cams < 1 || n_cams > kMvMaxCams || n_pts < 0 || n_obs < 0 || !intr || !cams || (n_pts && !pts) ||
        (n_obs && (!cam_idx || !pt_idx || !obs_xy || !obs_w)))
        return set_err(ctx, E2EMV_EINVAL, "mv_bundle_adjust: bad argument (1 <= n_cams <= %d)", kMvMaxCams);
    for (int o = 0; o < n_obs; ++o)
        if (cam_idx[o] < 0 || cam_idx[o] >= n_cams || pt_idx[o] < 0 || pt_idx[o] >= n_pts)
            return set_err(ctx, E2EMV_EINVAL, "mv_bundle_adjust: observation %d refers to camera %d / point %d", o, cam_idx[o], pt_idx[o]);
    // the batch of one
    const int32_t nc = n_cams, fc = fixed_cam;
    const int64_t po[2] = {0, n_pts}, oo[2] = {0, n_obs};
    return e2emv_mv_bundle_adjust_batch(ctx, 1, &nc, &fc, intr, po, oo, cam_idx, pt_idx, obs_xy, obs_w, cams, pts, max_iterations, summary, stream);
}

extern "C" int e2emv_mv_collect(e2emv_ctx* ctx, int B, int T, int N, const float* const* d_kpts0, const float* const* d_kpts1,
                                const int32_t* n_kpts1, const int64_t* const* d_matches, const float* const* d_conf, int conf_channels,
                                float conf_thresh, float* d_mkpts0, float* d_mkpts1, float* d_mconf, int32_t* d_count, void* stream) {
    if (!ctx) return E2EMV_EINVAL;
    E2EMV_ENTER(ctx, stream);
    if (B < 1 || N < 1 || conf_channels < 1 || !d_kpts0 || !d_kpts1 || !n_kpts1 || !d_matches || !d_conf || !d_mkpts0 || !d_mkpts1 || !d_mconf || !d_count)
        return set_err(ctx, E2EMV_EINVAL, "mv_collect: bad argument (B, N, conf_channels >= 1, no NULL array)");
    if (T < 2 || T > kMvMaxCams) return set_err(ctx, E2EMV_EINVAL, "mv_collect: tuple of %d images (2 <= T <= %d)", T, kMvMaxCams);
    MvCollectArgs a{};
    a.B = B; a.P = T * (T - 1) / 2; a.N = N; a.channels = conf_channels; a.thresh = conf_thresh;
    if (size_t(B) * a.P * N > size_t(INT32_MAX) / 2) return set_err(ctx, E2EMV_ESHAPE, "mv_collect: B * pairs * N = %zu is too large", size_t(B) * a.P * N);
    for (int q = 0; q < a.P; ++q) {
        if (d_matches[q] && (!d_kpts0[q] || !d_kpts1[q] || !d_conf[q] || n_kpts1[q] < 1))
            return set_err(ctx, E2EMV_EINVAL, "mv_collect: pair %d has matches but no keypoints / confidences", q);
        a.k0[q] = d_kpts0[q]; a.k1[q] = d_kpts1[q]; a.match[q] = d_matches[q]; a.conf[q] = d_conf[q]; a.n1[q] = n_kpts1[q];
    }
    a.o0 = d_mkpts0; a.o1 = d_mkpts1; a.oc = d_mconf; a.count = d_count;
    hipLaunchKernelGGL(mv_collect_kernel<false>, dim3(B * a.P), dim3(kMvRowThreads), 0, (hipStream_t)stream, a);
    E2EMV_CHECK_LAUNCH(ctx, "mv_collect_kernel");
    return E2EMV_OK;
}

// stage 4 (and the uploads in front of it) shared by e2emv_mv_tuple_ba and e2emv_mv_tuple_problem; leaves the problems of the B
// tuples in the workspace, described by *L
namespace e2emv {
int mv_tuple_build(e2emv_ctx* ctx, const char* who, int B, int T, int N, const int32_t* counts, const float* d_mkpts0, const float* d_mkpts1,
                   const float* d_mconf, const float* const* d_intr, int kdim, int intr_batch, const double* extr, int max_iterations,
                   double loss_scale, size_t tail, MvLayout* L, size_t* totP_out, hipStream_t s) {
    if (B < 1 || N < 1 || !counts || !d_mkpts0 || !d_mkpts1 || !d_mconf || !d_intr || !extr)
        return set_err(ctx, E2EMV_EINVAL, "%s: bad argument (B, N >= 1, no NULL array)", who);
    if (T < 2 || T > kMvMaxCams) return set_err(ctx, E2EMV_EINVAL, "%s: tuple of %d images (2 <= T <= %d)", who, T, kMvMaxCams);
    if (kdim != 3 && kdim != 4) return set_err(ctx, E2EMV_ESHAPE, "%s: intrinsics must be 3x3 or 4x4", who);
    if (intr_batch != 1 && intr_batch != B) return set_err(ctx, E2EMV_ESHAPE, "%s: intr_batch must be 1 or B", who);
    const int P = T * (T - 1) / 2;
    for (int t = 0; t < T; ++t)
        if (!d_intr[t]) return set_err(ctx, E2EMV_EINVAL, "%s: NULL intrinsics of image %d", who, t);
    size_t totP = 0;
    for (int k = 0; k < B * P; ++k) {
        if (counts[k] < 0 || counts[k] > N) return set_err(ctx, E2EMV_EINVAL, "%s: count %d of pair block %d is outside [0, N = %d]", who, counts[k], k, N);
        totP += size_t(counts[k]);
    }
    if (size_t(B) * P * N > size_t(INT32_MAX) / 64) return set_err(ctx, E2EMV_ESHAPE, "%s: B * pairs * N = %zu is too large", who, size_t(B) * P * N);
    const size_t n = size_t(B), totC = n * T, totO = 2 * totP;
    const size_t proj_bytes = (totC * 12 * 8 + 255) & ~size_t(255), extra = proj_bytes + n * P * sizeof(MvPairRec);
    const int rc = ws_reserve(ctx, mv_layout(nullptr, n, totC, totP, totO, extra).bytes + tail);
    if (rc) return rc;
    *L = mv_layout(ctx->d_ws, n, totC, totP, totO, extra);
    // everything the host contributes in one staging block = one copy: records, start cameras, camera list starts, projection
    // matrices, pair records
    std::vector<char> stage(L->upload_bytes, 0);
    auto at = [&](const void* dev) { return stage.data() + (reinterpret_cast<const char*>(dev) - ctx->d_ws); };
    MvbaArgs* recs = reinterpret_cast<MvbaArgs*>(at(L->recs));
    double* cams = reinterpret_cast<double*>(at(L->cams));
    int* cstart = reinterpret_cast<int*>(at(L->cam_start));
    double* proj = reinterpret_cast<double*>(at(L->extra));
    MvPairRec* pairs = reinterpret_cast<MvPairRec*>(at(L->extra + proj_bytes));
    const double unit_intr[4] = {1.0, 1.0, 0.0, 0.0};  // the intrinsics are folded into the observations
    size_t p0 = 0;
    for (int b = 0; b < B; ++b) {
        const int32_t* cnt = counts + size_t(b) * P;
        int* cs = cstart + size_t(b) * T + b;  // [T + 1]
        int q = 0, pts_b = 0;
        for (int j = 0; j < T; ++j)
            for (int i = 0; i < j; ++i, ++q) { cs[i + 1] += cnt[q]; cs[j + 1] += cnt[q]; pts_b += cnt[q]; }
        for (int c = 0; c < T; ++c) cs[c + 1] += cs[c];
        int fill[kMvMaxCams];
        for (int c = 0; c < T; ++c) fill[c] = cs[c];
        q = 0;
        int pt_base = 0;
        for (int j = 0; j < T; ++j)
            for (int i = 0; i < j; ++i, ++q) {
                MvPairRec& r = pairs[size_t(b) * P + q];
                r.i = i; r.j = j; r.count = cnt[q]; r.pt_base = pt_base; r.list_i = fill[i]; r.list_j = fill[j];
                fill[i] += cnt[q]; fill[j] += cnt[q]; pt_base += cnt[q];
            }
        for (int t = 0; t < T; ++t) {
            const double* E = extr + (size_t(b) * T + t) * 16;
            std::memcpy(proj + (size_t(b) * T + t) * 12, E, 12 * sizeof(double));
            mv_extr_to_cam(E, cams + (size_t(b) * T + t) * 6);
        }
        recs[b] = mv_record(*L, size_t(b), size_t(b) * T, p0, 2 * p0, T, 0, pts_b, 2 * pts_b, max_iterations, unit_intr, 0.0);
        p0 += size_t(pts_b);
    }
    E2EMV_HIP(ctx, hipMemcpyAsync(ctx->d_ws, stage.data(), stage.size(), hipMemcpyHostToDevice, s));
    E2EMV_HIP(ctx, hipStreamSynchronize(s));  // the staging block dies at return
    MvBuildArgs g{};
    g.P = P; g.T = T; g.N = N; g.kdim = kdim; g.intr_batch = intr_batch;
    g.k0 = d_mkpts0; g.k1 = d_mkpts1; g.conf = d_mconf;
    for (int t = 0; t < T; ++t) g.intr[t] = d_intr[t];
    g.proj = reinterpret_cast<const double*>(L->extra);
    g.pairs = reinterpret_cast<const MvPairRec*>(L->extra + proj_bytes);
    g.recs = L->recs;
    g.loss_scale = loss_scale;
    hipLaunchKernelGGL(mv_build_kernel, dim3((N + kMvRowThreads - 1) / kMvRowThreads, B * P), dim3(kMvRowThreads), 0, s, g);
    E2EMV_CHECK_LAUNCH(ctx, "mv_build_kernel");
    *totP_out = totP;
    return E2EMV_OK;
}
}  // namespace e2emv

extern "C" int e2emv_mv_tuple_ba_loss(e2emv_ctx* ctx, int B, int T, int N, const int32_t* counts, const float* d_mkpts0,
                                      const float* d_mkpts1, const float* d_mconf, const float* const* d_intr, int kdim, int intr_batch,
                                      const double* extr, int max_iterations, double* out_extr, double* summary, int loss,
                                      double loss_scale, double* loss_a_out, void* stream) {
    if (!ctx) return E2EMV_EINVAL;
    E2EMV_ENTER(ctx, stream);
    if (!out_extr) return set_err(ctx, E2EMV_EINVAL, "mv_tuple_ba: NULL output");
    int rc = mv_check_loss(ctx, "mv_tuple_ba", loss, &loss_scale);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    MvLayout L;
    size_t totP = 0;
    rc = mv_tuple_build(ctx, "mv_tuple_ba", B, T, N, counts, d_mkpts0, d_mkpts1, d_mconf, d_intr, kdim, intr_batch, extr, max_iterations, loss_scale, 0, &L, &totP, s);
    if (rc) return rc;
    rc = mv_launch_ba(ctx, L, B, s, loss);
    if (rc) return rc;
    return mv_tuple_results(ctx, L, B, T, out_extr, summary, loss_a_out, s);
}

extern "C" int e2emv_mv_tuple_ba(e2emv_ctx* ctx, int B, int T, int N, const int32_t* counts, const float* d_mkpts0, const float* d_mkpts1,
                                 const float* d_mconf, const float* const* d_intr, int kdim, int intr_batch, const double* extr,
                                 int max_iterations, double* out_extr, double* summary, void* stream) {
    return e2emv_mv_tuple_ba_loss(ctx, B, T, N, counts, d_mkpts0, d_mkpts1, d_mconf, d_intr, kdim, intr_batch, extr, max_iterations, out_extr,
                                  summary, kLossNone, 0.0, nullptr, stream);
}

extern "C" int e2emv_mv_tuple_problem(e2emv_ctx* ctx, int B, int T, int N, const int32_t* counts, const float* d_mkpts0,
                                      const float* d_mkpts1, const float* d_mconf, const float* const* d_intr, int kdim, int intr_batch,
                                      const double* extr, int32_t* cam_idx, int32_t* pt_idx, double* obs_xy, double* obs_w, double* cams,
                                      double* pts, void* stream) {
    if (!ctx) return E2EMV_EINVAL;
    E2EMV_ENTER(ctx, stream);
    if (!cams) return set_err(ctx, E2EMV_EINVAL, "mv_tuple_problem: NULL output");
    hipStream_t s = (hipStream_t)stream;
    MvLayout L;
    size_t totP = 0;
    const int rc = mv_tuple_build(ctx, "mv_tuple_problem", B, T, N, counts, d_mkpts0, d_mkpts1, d_mconf, d_intr, kdim, intr_batch, extr, 0, 0.0, 0, &L, &totP, s);
    if (rc) return rc;
    if (totP && (!cam_idx || !pt_idx || !obs_xy || !obs_w || !pts)) return set_err(ctx, E2EMV_EINVAL, "mv_tuple_problem: NULL output for %zu points", totP);
    E2EMV_HIP(ctx, hipMemcpyAsync(cams, L.cams, sizeof(double) * 6 * B * T, hipMemcpyDeviceToHost, s));
    if (totP) {
        E2EMV_HIP(ctx, hipMemcpyAsync(cam_idx, L.cam_idx, sizeof(int) * 2 * totP, hipMemcpyDeviceToHost, s));
        E2EMV_HIP(ctx, hipMemcpyAsync(pt_idx, L.pt_idx, sizeof(int) * 2 * totP, hipMemcpyDeviceToHost, s));
        E2EMV_HIP(ctx, hipMemcpyAsync(obs_xy, L.obs, sizeof(double) * 4 * totP, hipMemcpyDeviceToHost, s));
        E2EMV_HIP(ctx, hipMemcpyAsync(obs_w, L.wts, sizeof(double) * 4 * totP, hipMemcpyDeviceToHost, s));
        E2EMV_HIP(ctx, hipMemcpyAsync(pts, L.pts, sizeof(double) * 3 * totP, hipMemcpyDeviceToHost, s));
    }
    E2EMV_HIP(ctx, hipStreamSynchronize(s));
    return E2EMV_OK;
}

extern "C" int e2emv_mv_tuple_ba_backward(e2emv_ctx* ctx, int B, int T, int N, const int32_t* counts, const float* d_mkpts0,
                                          const float* d_mkpts1, const float* d_mconf, const float* const* d_intr, int kdim, int intr_batch,
                                          const double* extr, int max_iterations, const double* g_out_extr, float* d_gmconf, void* stream) {
    if (!ctx) return E2EMV_EINVAL;
    E2EMV_ENTER(ctx, stream);
    const char* who = "mv_tuple_ba_backward";
    if (!g_out_extr || !d_gmconf) return set_err(ctx, E2EMV_EINVAL, "%s: NULL g_out_extr / d_gmconf", who);
    if (B < 1 || T < 2 || T > kMvMaxCams || N < 1 || !counts) return set_err(ctx, E2EMV_EINVAL, "%s: bad argument (B, N >= 1, 2 <= T <= %d, counts)", who, kMvMaxCams);
    const int P = T * (T - 1) / 2;
    std::vector<int> Cs(B, T), Ps(B, 0), Os(B, 0);
    for (int b = 0; b < B; ++b) {
        for (int q = 0; q < P; ++q) {
            const int c = counts[size_t(b) * P + q];
            if (c < 0 || c > N) return set_err(ctx, E2EMV_EINVAL, "%s: count %d of pair block %d is outside [0, N = %d]", who, c, b * P + q, N);
            Ps[b] += c;
        }
        Os[b] = 2 * Ps[b];
    }
    bool overflow = false;
    const size_t tail = mv_bwd_bytes(Cs, Ps, Os, max_iterations, &overflow);
    int rc = mv_bwd_fits(ctx, who, tail, overflow);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    MvLayout L;
    size_t totP = 0;
    rc = mv_tuple_build(ctx, who, B, T, N, counts, d_mkpts0, d_mkpts1, d_mconf, d_intr, kdim, intr_batch, extr, max_iterations, 0.0, tail, &L, &totP, s);
    if (rc) return rc;
    MvBwdLayout W;
    rc = mv_bwd_carve(ctx, ctx->d_ws + L.bytes, Cs, Ps, Os, max_iterations, true, &W, s);
    if (rc) return rc;
    const size_t totC = size_t(B) * T;
    E2EMV_HIP(ctx, hipMemsetAsync(W.cams_bar, 0, sizeof(double) * 6 * totC, s));
    if (totP) E2EMV_HIP(ctx, hipMemsetAsync(W.pts_bar, 0, sizeof(double) * 3 * totP, s));
    E2EMV_HIP(ctx, hipMemcpyAsync(W.g_extr, g_out_extr, sizeof(double) * 16 * totC, hipMemcpyHostToDevice, s));
    E2EMV_HIP(ctx, hipStreamSynchronize(s));  // g_out_extr is the caller's
    rc = mv_launch_ba_backward(ctx, L, W, B, s);
    if (rc) return rc;
    MvWeightsBwdArgs g{};
    g.P = P; g.N = N; g.conf = d_mconf; g.bw = W.recs; g.gconf = d_gmconf;
    const size_t proj_bytes = (totC * 12 * 8 + 255) & ~size_t(255);  // (mv_tuple_build: the pair records lie behind the projections)
    g.pairs = reinterpret_cast<const MvPairRec*>(L.extra + proj_bytes);
    hipLaunchKernelGGL(mv_weights_backward_kernel, dim3(B), dim3(kMvRowThreads), 0, s, g);
    E2EMV_CHECK_LAUNCH(ctx, "mv_weights_backward_kernel");
    E2EMV_HIP(ctx, hipStreamSynchronize(s));
    return E2EMV_OK;
}

extern "C" int e2emv_mv_collect_backward(e2emv_ctx* ctx, int B, int T, int N, const int32_t* n_kpts1, const int64_t* const* d_matches,
                                         const float* const* d_conf, int conf_channels, float conf_thresh, const float* d_gmconf,
                                         float* const* d_gconf, void* stream) {
    if (!ctx) return E2EMV_EINVAL;
    E2EMV_ENTER(ctx, stream);
    if (B < 1 || N < 1 || conf_channels < 1 || !n_kpts1 || !d_matches || !d_conf || !d_gmconf || !d_gconf)
        return set_err(ctx, E2EMV_EINVAL, "mv_collect_backward: bad argument (B, N, conf_channels >= 1, no NULL array)");
    if (T < 2 || T > kMvMaxCams) return set_err(ctx, E2EMV_EINVAL, "mv_collect_backward: tuple of %d images (2 <= T <= %d)", T, kMvMaxCams);
    MvCollectArgs a{};
    a.B = B; a.P = T * (T - 1) / 2; a.N = N; a.channels = conf_channels; a.thresh = conf_thresh;
    if (size_t(B) * a.P * N > size_t(INT32_MAX) / 2) return set_err(ctx, E2EMV_ESHAPE, "mv_collect_backward: B * pairs * N = %zu is too large", size_t(B) * a.P * N);
    for (int q = 0; q < a.P; ++q) {
        if (d_gconf[q] && d_matches[q] && (!d_conf[q] || n_kpts1[q] < 1))
            return set_err(ctx, E2EMV_EINVAL, "mv_collect_backward: pair %d has matches but no confidences", q);
        a.match[q] = d_matches[q]; a.conf[q] = d_conf[q]; a.n1[q] = n_kpts1[q]; a.gout[q] = d_gconf[q];
    }
    a.gin = d_gmconf;
    hipLaunchKernelGGL(mv_collect_kernel<true>, dim3(B * a.P), dim3(kMvRowThreads), 0, (hipStream_t)stream, a);
    E2EMV_CHECK_LAUNCH(ctx, "mv_collect_kernel<backward>");
    return E2EMV_OK;
}

extern "C" int e2emv_mv_bundle_adjust_files(e2emv_ctx* ctx, const char* in_csv, const char* out_csv, void* stream) {
    if (!ctx) return E2EMV_EINVAL;
    E2EMV_ENTER(ctx, stream);
    if (!in_csv || !out_csv) return set_err(ctx, E2EMV_EINVAL, "mv_bundle_adjust_files: NULL path");
    std::ifstream file(in_csv);
    if (!file) return set_err(ctx, E2EMV_EINVAL, "mv_bundle_adjust_files: cannot open %s", in_csv);
    int n_cams = -1, fixed = 0, n_pts = 0, n_obs = 0;
    double intr[4] = {1, 1, 0, 0};
    std::vector<int> ci, pi;
    std::vector<double> obs, wts, cams, pts;
    std::string line;
    try {
        while (std::getline(file, line)) {  // rows are classified by their field count (ba_problem.cpp:15-87)
            const auto el = mv::split_by_char(line, ',');
            const size_t k = el.size();
            if (k == 8) {
                n_cams = std::stoi(el[0]); fixed = std::stoi(el[1]); n_pts = std::stoi(el[2]); n_obs = std::stoi(el[3]);
                for (int i = 0; i < 4; ++i) intr[i] = std::stod(el[4 + i]);
            } else if (k == 3) {
                for (int i = 0; i < 3; ++i) pts.push_back(std::stod(el[i]));
            } else if (k >= 4 && k <= 6) {
                ci.push_back(std::stoi(el[0])); pi.push_back(std::stoi(el[1]));
                obs.push_back(std::stod(el[2])); obs.push_back(std::stod(el[3]));
                double wx = 1.0, wy = 1.0;
                if (k == 5) wx = wy = std::stod(el[4]);
                if (k == 6) { wx = std::stod(el[4]); wy = std::stod(el[5]); }
                wts.push_back(wx); wts.push_back(wy);
            } else if (k == 12) {
                double R[9], aa[3];
                for (int i = 0; i < 9; ++i) R[i] = std::stod(el[i]);
                mv::R_to_aa(R, aa);
                cams.insert(cams.end(), aa, aa + 3);
                for (int i = 9; i < 12; ++i) cams.push_back(std::stod(el[i]));
            }
        }
    } catch (...) {
        return set_err(ctx, E2EMV_EINVAL, "mv_bundle_adjust_files: malformed number in %s", in_csv);
    }
    if (n_cams < 1 || int(cams.size()) != 6 * n_cams || int(pts.size()) != 3 * n_pts || int(ci.size()) != n_obs)
        return set_err(ctx, E2EMV_ESHAPE, "mv_bundle_adjust_files: header says %d cameras / %d points / %d observations, file holds %zu / %zu / %zu",
                       n_cams, n_pts, n_obs, cams.size() / 6, pts.size() / 3, ci.size());
    double summary[4];
    const int rc = e2emv_mv_bundle_adjust(ctx, n_cams, fixed, n_pts, n_obs, intr, ci.data(), pi.data(), obs.data(), wts.data(), cams.data(),
                                          pts.data(), 50, summary, stream);
    if (rc) return rc;
    std::ofstream out(out_csv);
    if (!out) return set_err(ctx, E2EMV_EINVAL, "mv_bundle_adjust_files: cannot write %s", out_csv);
    for (int c = 0; c < n_cams; ++c) {  // WriteResult (ba_problem.cpp:98-113): R column-major then t
        double R[9];
        mv::aa_to_R(&cams[6 * c], R);
        for (int i = 0; i < 9; ++i) out << std::setprecision(12) << R[i] << ",";
        out << cams[6 * c + 3] << "," << cams[6 * c + 4] << "," << cams[6 * c + 5] << "\n";
    }
    return E2EMV_OK;
}

extern "C" int e2emv_mv_triangulate(e2emv_ctx* ctx, int n, const double* P0, const double* P1, const double* x0, const double* x1,
                                    double* xyz, void* stream) {
    if (!ctx) return E2EMV_EINVAL;
    E2EMV_ENTER(ctx, stream);
    if (n < 0 || !P0 || !P1 || (n && (!x0 || !x1 || !xyz))) return set_err(ctx, E2EMV_EINVAL, "mv_triangulate: bad argument");
    if (n == 0) return E2EMV_OK;
    hipStream_t s = (hipStream_t)stream;
    const size_t nd = 24 + size_t(n) * 7;
    int rc = ws_reserve(ctx, nd * 8 + 256);
    if (rc) return rc;
    double* d = reinterpret_cast<double*>(ctx->d_ws);
    E2EMV_HIP(ctx, hipMemcpyAsync(d, P0, 96, hipMemcpyHostToDevice, s));
    E2EMV_HIP(ctx, hipMemcpyAsync(d + 12, P1, 96, hipMemcpyHostToDevice, s));
    E2EMV_HIP(ctx, hipMemcpyAsync(d + 24, x0, 16 * size_t(n), hipMemcpyHostToDevice, s));
    E2EMV_HIP(ctx, hipMemcpyAsync(d + 24 + 2 * size_t(n), x1, 16 * size_t(n), hipMemcpyHostToDevice, s));
    double* dx = d + 24 + 4 * size_t(n);
    hipLaunchKernelGGL(mv_triangulate_kernel, dim3((n + 255) / 256), dim3(256), 0, s, n, d, d + 12, d + 24, d + 24 + 2 * size_t(n), dx);
    E2EMV_CHECK_LAUNCH(ctx, "mv_triangulate_kernel");
    E2EMV_HIP(ctx, hipMemcpyAsync(xyz, dx, 24 * size_t(n), hipMemcpyDeviceToHost, s));
    E2EMV_HIP(ctx, hipStreamSynchronize(s));
    return E2EMV_OK;
}
