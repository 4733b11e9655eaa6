// Declarations shared by the files of the multi-view bundle adjustment (mvba.hip: solver entries, pairwise problem build;
// mvba_backward.hip: the reverse pass; mvtracks.hip: track merging and the track problem build), and the solver kernel itself,
// mvba_kernel<LOSS, MODE>: the forward (mvba.hip) and the backward (mvba_backward.hip) instantiate the one statement of the LM loop.
#pragma once
#include <vector>

#include "common.h"
#include "small_linalg.h"

namespace e2emv {

constexpr int kMvThreads = 512;  // 8 waves = 2 per SIMD -> 256 VGPRs each (phase E keeps a 6x6 fp64 block per lane)
constexpr int kMvWaves = kMvThreads / 64;
constexpr int kMvMaxCams = E2EMV_MAX_TUPLE;
constexpr int kMvN = 6 * kMvMaxCams;  // reduced system order bound (48)

struct MvbaArgs {
    int C, fixed, P, O, max_iters;
    double fx, fy, cx, cy;
    const int *cam_idx, *pt_idx, *pt_start, *pt_obs, *cam_start, *cam_obs;
    const double *obs, *wts;
    double *cams, *pts;
    double *r, *Jc, *Jp, *Y, *Vinv, *gp, *dp, *scale_p, *cand;
    double* summary;  // [0] initial cost [1] final cost [2] iterations [3] termination code
    double loss_a;    // scale of the robust loss in the units of the weighted residual (the tuple builds divide it on the device)
};

struct MvbaBwdArgs;  // what the backward pass adds to a problem's record (below, in front of the kernel)

enum { kTermMaxIter = 0, kTermGradient = 1, kTermParameter = 2, kTermFunction = 3, kTermInvalid = 4, kTermRadius = 5 };

// Robust loss of an observation (a ceres::LossFunction where the reference passes NULL): s = rx^2 + ry^2 of the WEIGHTED
// residual, cost = 1/2 sum rho(s).  Both losses have rho'' <= 0, so Ceres' corrector scales the residual and both Jacobian
// blocks of the observation by sqrt(rho'(s)) and nothing else.  The codes are those of include/e2emv.h.
enum { kLossNone = E2EMV_LOSS_NONE, kLossHuber = E2EMV_LOSS_HUBER, kLossCauchy = E2EMV_LOSS_CAUCHY };

// rho(s) and sqrt(rho'(s)) at scale a, a2 = a * a.  THE operation order (tests restate it):
//   huber : s <= a2 ? (rho = s, sqrt(rho') = 1) : (t = sqrt(s); rho = 2 a t - a2; sqrt(rho') = sqrt(a / t))
//   cauchy: q = s / a2; rho = a2 log1p(q); sqrt(rho') = sqrt(1 / (1 + q))
// s = 0 takes Huber's first branch (no division); a NaN s fails the comparison and stays NaN through the second.
template <int LOSS>
__device__ __forceinline__ void mv_loss(double s, double a, double a2, double* rho, double* sq) {
    if (LOSS == kLossHuber) {
        if (s <= a2) {
            *rho = s; *sq = 1.0;
        } else {
            const double t = sqrt(s);
            *rho = 2.0 * a * t - a2; *sq = sqrt(a / t);
        }
    } else if (LOSS == kLossCauchy) {
        const double q = s / a2;
        *rho = a2 * log1p(q); *sq = sqrt(1.0 / (1.0 + q));
    } else {
        *rho = s; *sq = 1.0;
    }
}

__device__ __forceinline__ double mv_wmax(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
    return v;
}

// ---- scalars of the residual: fp64, and fp64 with one tangent (the backward pass takes second derivatives of the residual as the
// tangent of the analytic Jacobians, mvba_backward.hip).  mv_transform is written once over both; with T = double
// every expression is the one the solver always evaluated.
struct MvDual {
    double v, d;
    __host__ __device__ MvDual(double v_ = 0.0, double d_ = 0.0) : v(v_), d(d_) {}
};
__host__ __device__ __forceinline__ double mv_val(double x) { return x; }
__host__ __device__ __forceinline__ double mv_val(const MvDual& x) { return x.v; }
__host__ __device__ __forceinline__ MvDual operator-(const MvDual& a) { return MvDual(-a.v, -a.d); }
__host__ __device__ __forceinline__ MvDual operator+(const MvDual& a, const MvDual& b) { return MvDual(a.v + b.v, a.d + b.d); }
__host__ __device__ __forceinline__ MvDual operator+(const MvDual& a, double b) { return MvDual(a.v + b, a.d); }
__host__ __device__ __forceinline__ MvDual operator+(double a, const MvDual& b) { return MvDual(a + b.v, b.d); }
__host__ __device__ __forceinline__ MvDual operator-(const MvDual& a, const MvDual& b) { return MvDual(a.v - b.v, a.d - b.d); }
__host__ __device__ __forceinline__ MvDual operator-(const MvDual& a, double b) { return MvDual(a.v - b, a.d); }
__host__ __device__ __forceinline__ MvDual operator-(double a, const MvDual& b) { return MvDual(a - b.v, -b.d); }
__host__ __device__ __forceinline__ MvDual operator*(const MvDual& a, const MvDual& b) { return MvDual(a.v * b.v, a.d * b.v + a.v * b.d); }
__host__ __device__ __forceinline__ MvDual operator*(const MvDual& a, double b) { return MvDual(a.v * b, a.d * b); }
__host__ __device__ __forceinline__ MvDual operator*(double a, const MvDual& b) { return MvDual(a * b.v, a * b.d); }
__host__ __device__ __forceinline__ MvDual operator/(const MvDual& a, const MvDual& b) {
    const double q = a.v / b.v;
    return MvDual(q, (a.d - q * b.d) / b.v);
}
__host__ __device__ __forceinline__ MvDual operator/(const MvDual& a, double b) { return MvDual(a.v / b, a.d / b); }
__host__ __device__ __forceinline__ MvDual operator/(double a, const MvDual& b) {
    const double q = a / b.v;
    return MvDual(q, -q * b.d / b.v);
}
__host__ __device__ __forceinline__ MvDual& operator+=(MvDual& a, const MvDual& b) { a.v += b.v; a.d += b.d; return a; }
__host__ __device__ __forceinline__ double mv_sqrt(double x) { return sqrt(x); }
__host__ __device__ __forceinline__ double mv_sin(double x) { return sin(x); }
__host__ __device__ __forceinline__ double mv_cos(double x) { return cos(x); }
__host__ __device__ __forceinline__ MvDual mv_sqrt(const MvDual& x) { const double s = sqrt(x.v); return MvDual(s, 0.5 * x.d / s); }
__host__ __device__ __forceinline__ MvDual mv_sin(const MvDual& x) { return MvDual(sin(x.v), cos(x.v) * x.d); }
__host__ __device__ __forceinline__ MvDual mv_cos(const MvDual& x) { return MvDual(cos(x.v), -sin(x.v) * x.d); }

constexpr int kMvMaxPairs = kMvMaxCams * (kMvMaxCams - 1) / 2;
constexpr int kMvRowThreads = 256;

// homogeneous DLT of two views (cv2.triangulatePoints at bundle_adjust_io.py:226-227): P0, P1 [3,4] row-major
__device__ __forceinline__ void mv_dlt(const double* P0, const double* P1, double x0x, double x0y, double x1x, double x1y, double* xyz) {
    double A[16];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        A[k] = x0x * P0[8 + k] - P0[k];
        A[4 + k] = x0y * P0[8 + k] - P0[4 + k];
        A[8 + k] = x1x * P1[8 + k] - P1[k];
        A[12 + k] = x1y * P1[8 + k] - P1[4 + k];
    }
    // smallest eigenvector of A^T A by cyclic Jacobi (fp64)
    double M[16], V[16];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            M[4 * r + c] = A[r] * A[c] + A[4 + r] * A[4 + c] + A[8 + r] * A[8 + c] + A[12 + r] * A[12 + c];
            V[4 * r + c] = r == c ? 1.0 : 0.0;
        }
    for (int sweep = 0; sweep < 30; ++sweep) {
        double off = 0;
        for (int p = 0; p < 4; ++p)
            for (int q = p + 1; q < 4; ++q) off += M[4 * p + q] * M[4 * p + q];
        if (off < 1e-300) break;
        for (int p = 0; p < 4; ++p)
            for (int q = p + 1; q < 4; ++q) {
                const double apq = M[4 * p + q];
                if (apq == 0.0) continue;
                const double theta = (M[4 * q + q] - M[4 * p + p]) / (2.0 * apq);
                const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                for (int k = 0; k < 4; ++k) {
                    const double mkp = M[4 * k + p], mkq = M[4 * k + q];
                    M[4 * k + p] = c * mkp - s * mkq;
                    M[4 * k + q] = s * mkp + c * mkq;
                }
                for (int k = 0; k < 4; ++k) {
                    const double mpk = M[4 * p + k], mqk = M[4 * q + k];
                    M[4 * p + k] = c * mpk - s * mqk;
                    M[4 * q + k] = s * mpk + c * mqk;
                }
                for (int k = 0; k < 4; ++k) {
                    const double vkp = V[4 * k + p], vkq = V[4 * k + q];
                    V[4 * k + p] = c * vkp - s * vkq;
                    V[4 * k + q] = s * vkp + c * vkq;
                }
            }
    }
    int m = 0;
    for (int k = 1; k < 4; ++k)
        if (M[5 * k] < M[5 * m]) m = k;
    const double w = V[12 + m];
    xyz[0] = V[m] / w;
    xyz[1] = V[4 + m] / w;
    xyz[2] = V[8 + m] / w;
}

// Device memory of a batch of problems inside the context workspace.  First what the host uploads in one piece (records, start
// cameras, camera list starts, `extra` bytes of the caller), then the per-observation / per-point arrays; problem k owns the
// slice behind its camera / point / observation offsets in each of them.
struct MvLayout {
    MvbaArgs* recs; double* cams; int* cam_start; char* extra;
    size_t upload_bytes;
    double *pts, *gp, *dp, *scale_p, *cand, *Vinv, *obs, *wts, *r, *Jc, *Jp, *Y, *summary;
    int *cam_idx, *pt_idx, *pt_obs, *cam_obs, *pt_start;
    size_t bytes;
};

MvLayout mv_layout(char* base, size_t n, size_t totC, size_t totP, size_t totO, size_t extra);
// record of problem k: its sizes and its slices (c0 / p0 / o0 = cameras / points / observations of the problems before it)
MvbaArgs mv_record(const MvLayout& L, size_t k, size_t c0, size_t p0, size_t o0, int C, int fixed, int P, int O, int max_iters,
                   const double* intr, double loss_a);
int mv_launch_ba(e2emv_ctx* ctx, const MvLayout& L, int n, hipStream_t s, int loss);
int mv_check_loss(e2emv_ctx* ctx, const char* who, int loss, double* scale);
int mv_tuple_results(e2emv_ctx* ctx, const MvLayout& L, int B, int T, double* out_extr, double* summary, double* loss_a_out, hipStream_t s);
// the checks of e2emv_mv_bundle_adjust_batch (also those of its backward entry): totals out
int mv_batch_check(e2emv_ctx* ctx, const char* who, int n_problems, const int32_t* n_cams, const int32_t* fixed_cam, const double* intr,
                   const int64_t* pt_off, const int64_t* obs_off, const int32_t* cam_idx, const int32_t* pt_idx, const double* obs_xy,
                   const double* obs_w, const double* cams, const double* pts, size_t* totC, size_t* totP, size_t* totO);
// reserves the layout of the checked batch and `tail` bytes behind it, builds the observation lists and uploads everything
int mv_batch_upload(e2emv_ctx* ctx, int n_problems, const int32_t* n_cams, const int32_t* fixed_cam, const double* intr, const int64_t* pt_off,
                    const int64_t* obs_off, const int32_t* cam_idx, const int32_t* pt_idx, const double* obs_xy, const double* obs_w,
                    const double* cams, const double* pts, int max_iterations, double loss_scale, size_t totC, size_t totP, size_t totO,
                    size_t tail, MvLayout* L, hipStream_t s);
// the tuple build (mvba.hip): problems of B tuples in the workspace, `tail` bytes reserved behind the layout
int mv_tuple_build(e2emv_ctx* ctx, const char* who, int B, int T, int N, const int32_t* counts, const float* d_mkpts0, const float* d_mkpts1,
                   const float* d_mconf, const float* const* d_intr, int kdim, int intr_batch, const double* extr, int max_iterations,
                   double loss_scale, size_t tail, MvLayout* L, size_t* totP_out, hipStream_t s);
// the reverse pass' share of the workspace (mvba_backward.hip): everything behind the layout of the problems
struct MvBwdLayout {
    MvbaBwdArgs* recs;
    double *cams_bar, *pts_bar, *wp, *fac_p, *g_w, *g_extr;  // [totC,6] [totP,3] x3 [totO,2] [totC,16]
};
// bytes of that share (0 and *overflow = true when they do not fit a size_t); Cs / Ps / Os: sizes per problem
size_t mv_bwd_bytes(const std::vector<int>& Cs, const std::vector<int>& Ps, const std::vector<int>& Os, int max_iterations, bool* overflow);
// E2EMV_ENOMEM when the share exceeds the device's memory (nothing freed, reserved or launched)
int mv_bwd_fits(e2emv_ctx* ctx, const char* who, size_t bytes, bool overflow);
// carves the share at `tail` and uploads its records (with_extr: the records point at g_extr)
int mv_bwd_carve(e2emv_ctx* ctx, char* tail, const std::vector<int>& Cs, const std::vector<int>& Ps, const std::vector<int>& Os, int max_iterations,
                 bool with_extr, MvBwdLayout* out, hipStream_t s);
int mv_launch_ba_backward(e2emv_ctx* ctx, const MvLayout& L, const MvBwdLayout& W, int n, hipStream_t s);
void mv_extr_to_cam(const double* E /* 4x4 row-major */, double* cam);
void mv_cam_to_extr(const double* cam, double* E);


// block-wide reduction of up to 4 values (sum for k < nsum, max for the rest); all threads get the result
template <int NV, int NSUM>
__device__ __forceinline__ void mv_block_reduce(double (&v)[NV], double* scratch /* [kMvWaves*NV] */) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < NV; ++k) v[k] = k < NSUM ? wave_sum_d(v[k]) : mv_wmax(v[k]);
    __syncthreads();
    if (lane == 0)
#pragma unroll
        for (int k = 0; k < NV; ++k) scratch[wave * NV + k] = v[k];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        double a = scratch[k];
        for (int w = 1; w < kMvWaves; ++w) a = k < NSUM ? a + scratch[w * NV + k] : fmax(a, scratch[w * NV + k]);
        v[k] = a;
    }
}

// p = R(w) X + t and (optionally) R and dp/dw (ceres::AngleAxisRotatePoint under autodiff: Rodrigues for theta^2 > eps,
// first-order X + w x X below).  identity: the fixed camera.
template <typename T>
__host__ __device__ __forceinline__ void mv_transform(const T* cam, bool identity, const T X[3], T p[3], T R[9] /*row-major*/,
                                                      T D[9] /* dp/dw row-major */, bool jac) {
    if (identity) {
        p[0] = X[0]; p[1] = X[1]; p[2] = X[2];
        if (jac) {
            R[0] = 1; R[1] = 0; R[2] = 0; R[3] = 0; R[4] = 1; R[5] = 0; R[6] = 0; R[7] = 0; R[8] = 1;
#pragma unroll
            for (int i = 0; i < 9; ++i) D[i] = 0;
        }
        return;
    }
    const T w0 = cam[0], w1 = cam[1], w2 = cam[2];
    const T t2 = w0 * w0 + w1 * w1 + w2 * w2;
    T Rl[9];
    const bool big = mv_val(t2) > 2.220446049250313e-16;
    if (big) {
        const T th = mv_sqrt(t2), k0 = w0 / th, k1 = w1 / th, k2 = w2 / th;
        const T s = mv_sin(th), c = mv_cos(th), v = 1.0 - c;
        // R = I + s K + v K^2
        Rl[0] = 1 - v * (k1 * k1 + k2 * k2); Rl[1] = -s * k2 + v * k0 * k1;       Rl[2] = s * k1 + v * k0 * k2;
        Rl[3] = s * k2 + v * k0 * k1;        Rl[4] = 1 - v * (k0 * k0 + k2 * k2); Rl[5] = -s * k0 + v * k1 * k2;
        Rl[6] = -s * k1 + v * k0 * k2;       Rl[7] = s * k0 + v * k1 * k2;        Rl[8] = 1 - v * (k0 * k0 + k1 * k1);
    } else {
        Rl[0] = 1; Rl[1] = -w2; Rl[2] = w1; Rl[3] = w2; Rl[4] = 1; Rl[5] = -w0; Rl[6] = -w1; Rl[7] = w0; Rl[8] = 1;
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) p[i] = Rl[3 * i] * X[0] + Rl[3 * i + 1] * X[1] + Rl[3 * i + 2] * X[2] + cam[3 + i];
    if (!jac) return;
#pragma unroll
    for (int i = 0; i < 9; ++i) R[i] = Rl[i];
    // [X]x
    const T Xh[9] = {T(0), -X[2], X[1], X[2], T(0), -X[0], -X[1], X[0], T(0)};
    if (!big) {
#pragma unroll
        for (int i = 0; i < 9; ++i) D[i] = -Xh[i];
        return;
    }
    // G = (w w^T + (R^T - I) [w]x) / theta^2 ;  D = -R [X]x G
    const T wh[9] = {T(0), -w2, w1, w2, T(0), -w0, -w1, w0, T(0)};
    const T w[3] = {w0, w1, w2};
    T G[9], Tm[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            T a = w[i] * w[j];
#pragma unroll
            for (int k = 0; k < 3; ++k) a += (Rl[3 * k + i] - (k == i ? 1.0 : 0.0)) * wh[3 * k + j];
            G[3 * i + j] = a / t2;
        }
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) Tm[3 * i + j] = Xh[3 * i] * G[j] + Xh[3 * i + 1] * G[3 + j] + Xh[3 * i + 2] * G[6 + j];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) D[3 * i + j] = -(Rl[3 * i] * Tm[j] + Rl[3 * i + 1] * Tm[3 + j] + Rl[3 * i + 2] * Tm[6 + j]);
}

// x = (L L^T)^-1 rhs by two substitutions with the Cholesky factor in the lower triangle of S (one wave, lane = row): phase F's
// substitution for the reverse pass' right-hand side.  Phase F keeps its own copy inline - called from there, hipcc duplicated a
// division and the kernel's instruction stream was no longer the one every existing test was pinned on.
__device__ __forceinline__ void mv_chol_solve(const double* s_S, int n, const double* s_rhs, double* s_x) {
    const int lane = threadIdx.x & 63;
    double b = lane < n ? s_rhs[lane] : 0.0;
    for (int j = 0; j < n; ++j) {  // L y = b
        const double yj = __shfl(b, j) / s_S[j * kMvN + j];
        if (lane == j) b = yj;
        else if (lane > j && lane < n) b -= s_S[lane * kMvN + j] * yj;
    }
    for (int j = n - 1; j >= 0; --j) {  // L^T x = y
        const double xj = __shfl(b, j) / s_S[j * kMvN + j];
        if (lane == j) b = xj;
        else if (lane < j) b -= s_S[j * kMvN + lane] * xj;
    }
    if (lane < n) s_x[lane] = b;
}

// One workgroup per problem: blockIdx.x selects the problem's record (sizes, intrinsics, fixed camera and the addresses of
// ITS slices of the shared index / data / scratch arrays and of its summary slot).  Nothing below knows of the other
// workgroups: several problems may share a CU (24 KB of LDS, 8 waves each), none shares a byte of global memory.
// LOSS: the robust loss (mvba.h).  Only phases A and H know of it: A stores the CORRECTED r, Jc, Jp (scaled by sqrt(rho')) and sums
// rho(s) into the cost, H sums rho(s) at the candidate; B - G and the model cost change read the stored arrays as they are.  The
// kLossNone instantiation is the kernel as it always was, operation for operation.
//
// The loop is stated once, here, for two users.  MODE kLmRun: the solver.  kLmTape: the backward pass (mvba_backward.hip) - the same
// run, which also records per pass the radius it used and whether the reduced system was solved and the step accepted, and per
// accepted step the iterate it started from; when the run has ended the accepted steps are walked from last to first THROUGH THE
// SAME PHASES A - G (rev: the taped iterate and radius are put back, no decision is taken, no loop state touched) and each is
// reversed by mv_reverse_step.  Recording and the reverse walk are compile-time branches: kLmRun is the kernel as it always was,
// instruction for instruction (the loop stays in the __global__ function itself - as an inlined device function hipcc contracted
// the robust-loss instantiations' sums differently).
struct MvTape {
    double* it;  // [max_iters,3] radius, solved, accepted of pass k
    double* x;   // [max_iters, 6 C + 3 P] cameras and points before accepted step j
};
struct MvbaBwdArgs {
    MvTape tape;
    double* cams_bar;  // [C,6]  in: dLoss/d(cams_out), out: dLoss/d(cams_start)
    double* pts_bar;   // [P,3]  in: dLoss/d(pts_out),  out: dLoss/d(pts_start)
    double* wp;        // [P,3]  point part of w
    double* fac_p;     // [P,3]  2 / radius on the unclamped point columns, 0 on the clamped
    double* g_w;       // [O,2]  dLoss/d(obs_w)
    const double* g_extr;  // [C,4,4] or NULL: dLoss/d(mv_cam_to_extr(cams_out)), taken to cams_bar when the run has ended (tuple route)
};
// what mv_reverse_step reads of the loop's LDS (and its own three vectors: cbar by camera, wc and fac by free camera)
struct MvRevLds {
    const double *cams, *dc, *U, *scale, *S;
    double *rhs, *cbar, *wc, *fac;
    const int *fidx, *free_;
};
enum { kLmRun = 0, kLmTape = 1 };
// The three calls of the reverse walk.  They are DEFINED in mvba_backward.hip, behind this header: mvba_kernel<LOSS, kLmTape> may be
// instantiated in that file only (mv_launch_ba_backward is how every other file reaches it); kLmRun never calls them.
// the run has ended: g_extr, if given, goes through mv_cam_to_extr at the final cameras into cams_bar
__device__ void mv_reverse_begin(const MvbaArgs& a, const MvbaBwdArgs& b, const double* s_cams, double* s_cbar);
// the reverse of one accepted step
__device__ void mv_reverse_step(const MvbaArgs& a, const MvbaBwdArgs& b, const MvRevLds& r, double radius, int F, int n);
// the next accepted pass below k: its iterate and radius go back into place; false when there is none
__device__ bool mv_reverse_next(const MvbaArgs& a, const MvbaBwdArgs& b, double* s_cams, double* s_ctl, int& k, int& j);

template <int LOSS, int MODE>
__global__ __launch_bounds__(kMvThreads) void mvba_kernel(const MvbaArgs* __restrict__ recs, const MvbaBwdArgs* __restrict__ bws) {
    const MvbaArgs& a = recs[blockIdx.x];
    const double loss_a = LOSS != kLossNone ? a.loss_a : 0.0, loss_a2 = loss_a * loss_a;
    __shared__ double s_cams[kMvN], s_cand[kMvN], s_scale[kMvN], s_lam[kMvN], s_gc[kMvN], s_dc[kMvN], s_rhs[kMvN];
    __shared__ double s_U[kMvMaxCams * 36];
    __shared__ double s_S[kMvN * kMvN];
    __shared__ double s_red[kMvWaves * 4];
    __shared__ double s_ctl[8];  // 0 radius 1 decrease 2 cost 3 - 4 - 5 solve ok 6 accept
    __shared__ int s_fidx[kMvMaxCams], s_free[kMvMaxCams], s_state[4];  // state: 0 stop flag, 1 iterations, 2 termination, 3 invalid count
    __shared__ double s_rev[MODE == kLmTape ? 3 * kMvN : 1];  // cbar, wc, fac of the reverse walk
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int C = a.C, P = a.P, O = a.O;

    if (tid < 6 * C) s_cams[tid] = a.cams[tid];
    if (tid == 0) {
        int F = 0;
        for (int c = 0; c < C; ++c) {
            s_fidx[c] = (c == a.fixed) ? -1 : F;
            if (c != a.fixed) s_free[F++] = c;
        }
        s_state[0] = 0; s_state[1] = 0; s_state[2] = kTermMaxIter; s_state[3] = 0;
        s_ctl[0] = 1e4; s_ctl[1] = 2.0;
    }
    [[maybe_unused]] bool rev = false;
    [[maybe_unused]] int rev_k = 0, rev_j = 0, n_acc = 0;
    if constexpr (MODE == kLmTape) {
        const MvbaBwdArgs& b = bws[blockIdx.x];
        for (int i = tid; i < 2 * O; i += kMvThreads) b.g_w[i] = 0.0;
        if (tid < 6 * C) s_rev[tid] = b.cams_bar[tid];
    }
    __syncthreads();
    int F = 0;
    for (int c = 0; c < C; ++c) F += (c != a.fixed);
    const int n = 6 * F;
    bool first = true;

    while (true) {
        // ---- A: residuals, Jacobians, cost at the current iterate ------------------------------------------------
        double red[4] = {0, 0, 0, 0};
        for (int o = tid; o < O; o += kMvThreads) {
            const int c = a.cam_idx[o], p = a.pt_idx[o];
            const double X[3] = {a.pts[3 * p], a.pts[3 * p + 1], a.pts[3 * p + 2]};
            double q[3], R[9], D[9];
            const bool fixed = (c == a.fixed);
            mv_transform<double>(&s_cams[6 * c], fixed, X, q, R, D, true);
            const double iz = 1.0 / q[2], wx = a.wts[2 * o], wy = a.wts[2 * o + 1];
            double rx = wx * (a.fx * q[0] * iz + a.cx - a.obs[2 * o]), ry = wy * (a.fy * q[1] * iz + a.cy - a.obs[2 * o + 1]);
            // d(residual)/d(q): rows weighted
            double e00 = wx * a.fx * iz, e02 = -wx * a.fx * q[0] * iz * iz, e11 = wy * a.fy * iz, e12 = -wy * a.fy * q[1] * iz * iz;
            if (LOSS == kLossNone) {
                red[0] += rx * rx + ry * ry;
            } else {
                // the corrector: residual and both Jacobian blocks (through the rows of d(residual)/d(q)) times sqrt(rho')
                double rho, sq;
                mv_loss<LOSS>(rx * rx + ry * ry, loss_a, loss_a2, &rho, &sq);
                red[0] += rho;
                rx *= sq; ry *= sq;
                e00 *= sq; e02 *= sq; e11 *= sq; e12 *= sq;
            }
            a.r[2 * o] = rx; a.r[2 * o + 1] = ry;
            double* jc = a.Jc + 12 * size_t(o);
            double* jp = a.Jp + 6 * size_t(o);
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                jc[k] = fixed ? 0.0 : e00 * D[k] + e02 * D[6 + k];
                jc[6 + k] = fixed ? 0.0 : e11 * D[3 + k] + e12 * D[6 + k];
                jp[k] = e00 * R[k] + e02 * R[6 + k];
                jp[3 + k] = e11 * R[3 + k] + e12 * R[6 + k];
            }
            jc[3] = fixed ? 0.0 : e00; jc[4] = 0.0; jc[5] = fixed ? 0.0 : e02;
            jc[9] = 0.0; jc[10] = fixed ? 0.0 : e11; jc[11] = fixed ? 0.0 : e12;
        }
        {
            double v[1] = {red[0]};
            mv_block_reduce<1, 1>(v, s_red);
            if (tid == 0) {
                s_ctl[2] = 0.5 * v[0];
                if (first) a.summary[0] = 0.5 * v[0];
            }
        }
        // ---- C: camera blocks U_c, g_c (a wave per free camera) -------------------------------------------------
        __syncthreads();  // Jc / r of all observations are in memory
        for (int f = wave; f < F; f += kMvWaves) {
            const int c = s_free[f];
            double u[21], g[6];
#pragma unroll
            for (int i = 0; i < 21; ++i) u[i] = 0;
#pragma unroll
            for (int i = 0; i < 6; ++i) g[i] = 0;
            for (int k = a.cam_start[c] + lane; k < a.cam_start[c + 1]; k += 64) {
                const int o = a.cam_obs[k];
                const double* jc = a.Jc + 12 * size_t(o);
                double j0[6], j1[6];
#pragma unroll
                for (int i = 0; i < 6; ++i) { j0[i] = jc[i]; j1[i] = jc[6 + i]; }
                const double rx = a.r[2 * o], ry = a.r[2 * o + 1];
                int t = 0;
#pragma unroll
                for (int i = 0; i < 6; ++i) {
                    g[i] += j0[i] * rx + j1[i] * ry;
#pragma unroll
                    for (int j = 0; j <= i; ++j) u[t++] += j0[i] * j0[j] + j1[i] * j1[j];
                }
            }
#pragma unroll
            for (int i = 0; i < 21; ++i) u[i] = wave_sum_d(u[i]);
#pragma unroll
            for (int i = 0; i < 6; ++i) g[i] = wave_sum_d(g[i]);
            if (lane == 0) {
                int t = 0;
                for (int i = 0; i < 6; ++i) {
                    s_gc[6 * f + i] = g[i];
                    for (int j = 0; j <= i; ++j) { s_U[36 * f + 6 * i + j] = u[t]; s_U[36 * f + 6 * j + i] = u[t]; ++t; }
                }
            }
        }
        __syncthreads();
        // ---- D: camera scaling / damping, camera part of the gradient norm --------------------------------------
        double gmax = 0.0;
        if (tid < n) {
            const double d = s_U[36 * (tid / 6) + 7 * (tid % 6)];
            if (first) s_scale[tid] = 1.0 / (1.0 + sqrt(d));
            const double sc = s_scale[tid];
            s_lam[tid] = fmin(fmax(d * sc * sc, 1e-6), 1e32) / s_ctl[0] / (sc * sc);
            gmax = fabs(s_gc[tid]);
        }
        // ---- B: point blocks ---------------------------------------------------------------------------------------
        const double radius = s_ctl[0];
        for (int p = tid; p < P; p += kMvThreads) {
            double V[6] = {0, 0, 0, 0, 0, 0}, g[3] = {0, 0, 0};  // V: 00 10 11 20 21 22
            for (int k = a.pt_start[p]; k < a.pt_start[p + 1]; ++k) {
                const int o = a.pt_obs[k];
                const double* jp = a.Jp + 6 * size_t(o);
                const double rx = a.r[2 * o], ry = a.r[2 * o + 1];
                V[0] += jp[0] * jp[0] + jp[3] * jp[3];
                V[1] += jp[1] * jp[0] + jp[4] * jp[3];
                V[2] += jp[1] * jp[1] + jp[4] * jp[4];
                V[3] += jp[2] * jp[0] + jp[5] * jp[3];
                V[4] += jp[2] * jp[1] + jp[5] * jp[4];
                V[5] += jp[2] * jp[2] + jp[5] * jp[5];
                g[0] += jp[0] * rx + jp[3] * ry;
                g[1] += jp[1] * rx + jp[4] * ry;
                g[2] += jp[2] * rx + jp[5] * ry;
            }
            const double d[3] = {V[0], V[2], V[5]};
            double lam[3];
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                double sc;
                if (first) { sc = 1.0 / (1.0 + sqrt(d[i])); a.scale_p[3 * p + i] = sc; }
                else sc = a.scale_p[3 * p + i];
                lam[i] = fmin(fmax(d[i] * sc * sc, 1e-6), 1e32) / radius / (sc * sc);
                gmax = fmax(gmax, fabs(g[i]));
                a.gp[3 * p + i] = g[i];
            }
            const double m00 = V[0] + lam[0], m10 = V[1], m11 = V[2] + lam[1], m20 = V[3], m21 = V[4], m22 = V[5] + lam[2];
            // inverse of the symmetric 3x3 through its adjugate
            const double c00 = m11 * m22 - m21 * m21, c10 = m20 * m21 - m10 * m22, c20 = m10 * m21 - m20 * m11;
            const double det = m00 * c00 + m10 * c10 + m20 * c20, id = 1.0 / det;
            const double i00 = c00 * id, i10 = c10 * id, i20 = c20 * id, i11 = (m00 * m22 - m20 * m20) * id, i21 = (m10 * m20 - m00 * m21) * id,
                         i22 = (m00 * m11 - m10 * m10) * id;
            double* vi = a.Vinv + 6 * size_t(p);
            vi[0] = i00; vi[1] = i10; vi[2] = i11; vi[3] = i20; vi[4] = i21; vi[5] = i22;
            for (int k = a.pt_start[p]; k < a.pt_start[p + 1]; ++k) {
                const int o = a.pt_obs[k];
                if (a.cam_idx[o] == a.fixed) continue;
                const double* jc = a.Jc + 12 * size_t(o);
                const double* jp = a.Jp + 6 * size_t(o);
                double* y = a.Y + 18 * size_t(o);
#pragma unroll
                for (int i = 0; i < 6; ++i) {
                    const double w0 = jc[i] * jp[0] + jc[6 + i] * jp[3], w1 = jc[i] * jp[1] + jc[6 + i] * jp[4], w2 = jc[i] * jp[2] + jc[6 + i] * jp[5];
                    y[3 * i] = w0 * i00 + w1 * i10 + w2 * i20;
                    y[3 * i + 1] = w0 * i10 + w1 * i11 + w2 * i21;
                    y[3 * i + 2] = w0 * i20 + w1 * i21 + w2 * i22;
                }
            }
        }
        {
            double v[1] = {gmax};
            mv_block_reduce<1, 0>(v, s_red);  // also orders the Y / Vinv / gp writes before phase E
            if (tid == 0 && !rev) {
                if (v[0] <= 1e-10) { s_state[0] = 1; s_state[2] = kTermGradient; }
                else if (s_state[1] >= a.max_iters) { s_state[0] = 1; }
                else s_state[1] += 1;
            }
        }
        first = false;
        __syncthreads();
        if (!rev && s_state[0]) {
            if constexpr (MODE == kLmTape) {  // the run has ended: walk its accepted steps backwards
                rev = true; rev_k = s_state[1]; rev_j = n_acc;
                mv_reverse_begin(a, bws[blockIdx.x], s_cams, s_rev);
                if (mv_reverse_next(a, bws[blockIdx.x], s_cams, s_ctl, rev_k, rev_j)) continue;
            }
            break;
        }
        // ---- E: reduced camera system (a wave per block of the upper triangle) ----------------------------------
        const int nblk = F * (F + 1) / 2;
        for (int blk = wave; blk < nblk; blk += kMvWaves) {
            int fa = 0, rem = blk;
            while (rem >= F - fa) { rem -= F - fa; ++fa; }
            const int fb = fa + rem, ca = s_free[fa], cb = s_free[fb];
            double acc[36], rh[6];
#pragma unroll
            for (int i = 0; i < 36; ++i) acc[i] = 0;
#pragma unroll
            for (int i = 0; i < 6; ++i) rh[i] = 0;
            for (int k = a.cam_start[ca] + lane; k < a.cam_start[ca + 1]; k += 64) {
                const int o = a.cam_obs[k], p = a.pt_idx[o];
                double y[18];
                const double* yo = a.Y + 18 * size_t(o);
#pragma unroll
                for (int i = 0; i < 18; ++i) y[i] = yo[i];
                if (fa == fb) {
                    const double g0 = a.gp[3 * p], g1 = a.gp[3 * p + 1], g2 = a.gp[3 * p + 2];
#pragma unroll
                    for (int i = 0; i < 6; ++i) rh[i] += y[3 * i] * g0 + y[3 * i + 1] * g1 + y[3 * i + 2] * g2;
                }
                for (int k2 = a.pt_start[p]; k2 < a.pt_start[p + 1]; ++k2) {
                    const int o2 = a.pt_obs[k2];
                    if (a.cam_idx[o2] != cb) continue;
                    const double* jc = a.Jc + 12 * size_t(o2);
                    const double* jp = a.Jp + 6 * size_t(o2);
#pragma unroll
                    for (int j = 0; j < 6; ++j) {
                        const double w0 = jc[j] * jp[0] + jc[6 + j] * jp[3], w1 = jc[j] * jp[1] + jc[6 + j] * jp[4], w2 = jc[j] * jp[2] + jc[6 + j] * jp[5];
#pragma unroll
                        for (int i = 0; i < 6; ++i) acc[6 * i + j] += y[3 * i] * w0 + y[3 * i + 1] * w1 + y[3 * i + 2] * w2;
                    }
                }
            }
#pragma unroll
            for (int i = 0; i < 36; ++i) acc[i] = wave_sum_d(acc[i]);
            if (fa == fb)
#pragma unroll
                for (int i = 0; i < 6; ++i) rh[i] = wave_sum_d(rh[i]);
            if (lane == 0) {
                for (int i = 0; i < 6; ++i) {
                    for (int j = 0; j < 6; ++j) {
                        double v = -acc[6 * i + j];
                        if (fa == fb) v += s_U[36 * fa + 6 * i + j] + (i == j ? s_lam[6 * fa + i] : 0.0);
                        s_S[(6 * fa + i) * kMvN + 6 * fb + j] = v;
                        if (fa != fb) s_S[(6 * fb + j) * kMvN + 6 * fa + i] = v;
                    }
                    if (fa == fb) s_rhs[6 * fa + i] = -s_gc[6 * fa + i] + rh[i];
                }
            }
        }
        __syncthreads();
        // ---- F: Cholesky + solves by wave 0 (lane = row) -------------------------------------------------------
        if (wave == 0) {
            bool ok = true;
            // a camera without observations has an all-zero row: keep it at zero step
            for (int j = 0; j < n && ok; ++j) {
                double s = 0.0;
                if (lane >= j && lane < n) {
                    s = s_S[lane * kMvN + j];
                    for (int k = 0; k < j; ++k) s -= s_S[lane * kMvN + k] * s_S[j * kMvN + k];
                }
                const double d = __shfl(s, j);
                if (!(d > 0.0)) { ok = false; break; }
                const double sd = sqrt(d);
                if (lane >= j && lane < n) s_S[lane * kMvN + j] = (lane == j) ? sd : s / sd;
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                __builtin_amdgcn_wave_barrier();
            }
            if (ok) {
                double b = lane < n ? s_rhs[lane] : 0.0;
                for (int j = 0; j < n; ++j) {  // L y = b
                    const double yj = __shfl(b, j) / s_S[j * kMvN + j];
                    if (lane == j) b = yj;
                    else if (lane > j && lane < n) b -= s_S[lane * kMvN + j] * yj;
                }
                for (int j = n - 1; j >= 0; --j) {  // L^T x = y
                    const double xj = __shfl(b, j) / s_S[j * kMvN + j];
                    if (lane == j) b = xj;
                    else if (lane < j) b -= s_S[j * kMvN + lane] * xj;
                }
                if (lane < n) s_dc[lane] = b;
            }
            if (lane == 0) s_ctl[5] = ok ? 1.0 : 0.0;
        }
        __syncthreads();
        const bool solved = s_ctl[5] != 0.0;
        double r4[4] = {0, 0, 0, 0};  // step norm^2, x norm^2, model change, candidate cost*2
        if (solved) {
            if (tid < n) {
                const int c = s_free[tid / 6];
                s_cand[6 * c + tid % 6] = s_cams[6 * c + tid % 6] + s_dc[tid];
                r4[0] += s_dc[tid] * s_dc[tid];
                r4[1] += s_cams[6 * c + tid % 6] * s_cams[6 * c + tid % 6];
            }
            if (tid < 6 && a.fixed >= 0 && a.fixed < C) s_cand[6 * a.fixed + tid] = s_cams[6 * a.fixed + tid];
            // ---- G: point steps ------------------------------------------------------------------------------------
            for (int p = tid; p < P; p += kMvThreads) {
                double g0 = a.gp[3 * p], g1 = a.gp[3 * p + 1], g2 = a.gp[3 * p + 2];
                for (int k = a.pt_start[p]; k < a.pt_start[p + 1]; ++k) {
                    const int o = a.pt_obs[k], f = s_fidx[a.cam_idx[o]];
                    if (f < 0) continue;
                    const double* jc = a.Jc + 12 * size_t(o);
                    const double* jp = a.Jp + 6 * size_t(o);
                    double q0 = 0, q1 = 0;
#pragma unroll
                    for (int i = 0; i < 6; ++i) { q0 += jc[i] * s_dc[6 * f + i]; q1 += jc[6 + i] * s_dc[6 * f + i]; }
                    g0 += jp[0] * q0 + jp[3] * q1;
                    g1 += jp[1] * q0 + jp[4] * q1;
                    g2 += jp[2] * q0 + jp[5] * q1;
                }
                const double* vi = a.Vinv + 6 * size_t(p);
                const double d0 = -(vi[0] * g0 + vi[1] * g1 + vi[3] * g2), d1 = -(vi[1] * g0 + vi[2] * g1 + vi[4] * g2),
                             d2 = -(vi[3] * g0 + vi[4] * g1 + vi[5] * g2);
                a.dp[3 * p] = d0; a.dp[3 * p + 1] = d1; a.dp[3 * p + 2] = d2;
                const double x0 = a.pts[3 * p], x1 = a.pts[3 * p + 1], x2 = a.pts[3 * p + 2];
                a.cand[3 * p] = x0 + d0; a.cand[3 * p + 1] = x1 + d1; a.cand[3 * p + 2] = x2 + d2;
                r4[0] += d0 * d0 + d1 * d1 + d2 * d2;
                r4[1] += x0 * x0 + x1 * x1 + x2 * x2;
            }
            __syncthreads();
            // ---- H: model cost change and candidate cost (not on the reverse walk: nothing is decided there) ------------
            for (int o = tid; o < (rev ? 0 : O); o += kMvThreads) {
                const int c = a.cam_idx[o], p = a.pt_idx[o], f = s_fidx[c];
                const double* jc = a.Jc + 12 * size_t(o);
                const double* jp = a.Jp + 6 * size_t(o);
                const double d0 = a.dp[3 * p], d1 = a.dp[3 * p + 1], d2 = a.dp[3 * p + 2];
                double m0 = jp[0] * d0 + jp[1] * d1 + jp[2] * d2, m1 = jp[3] * d0 + jp[4] * d1 + jp[5] * d2;
                if (f >= 0)
#pragma unroll
                    for (int i = 0; i < 6; ++i) { m0 += jc[i] * s_dc[6 * f + i]; m1 += jc[6 + i] * s_dc[6 * f + i]; }
                r4[2] -= m0 * (a.r[2 * o] + 0.5 * m0) + m1 * (a.r[2 * o + 1] + 0.5 * m1);
                const double X[3] = {a.cand[3 * p], a.cand[3 * p + 1], a.cand[3 * p + 2]};
                double q[3];
                mv_transform<double>(&s_cand[6 * c], c == a.fixed, X, q, nullptr, nullptr, false);
                const double iz = 1.0 / q[2];
                const double rx = a.wts[2 * o] * (a.fx * q[0] * iz + a.cx - a.obs[2 * o]), ry = a.wts[2 * o + 1] * (a.fy * q[1] * iz + a.cy - a.obs[2 * o + 1]);
                if (LOSS == kLossNone) {
                    r4[3] += rx * rx + ry * ry;
                } else {
                    double rho, sq;
                    mv_loss<LOSS>(rx * rx + ry * ry, loss_a, loss_a2, &rho, &sq);
                    r4[3] += rho;
                }
            }
        }
        if constexpr (MODE == kLmTape) {
            if (rev) {  // phases A - G are those of the taped step: reverse it, then on to the accepted step before it
                const MvbaBwdArgs& b = bws[blockIdx.x];
                const MvRevLds rl{s_cams, s_dc, s_U, s_scale, s_S, s_rhs, s_rev, s_rev + kMvN, s_rev + 2 * kMvN, s_fidx, s_free};
                if (solved) mv_reverse_step(a, b, rl, radius, F, n);
                if (mv_reverse_next(a, b, s_cams, s_ctl, rev_k, rev_j)) continue;
                break;
            }
        }
        mv_block_reduce<4, 4>(r4, s_red);
        // ---- I: trust-region bookkeeping (thread 0) --------------------------------------------------------------
        if (tid == 0) {
            const double cost = s_ctl[2], model = r4[2], cand_cost = 0.5 * r4[3];
            s_ctl[6] = 0.0;  // accept flag
            if (!solved || !(model > 0.0)) {
                s_state[3] += 1;
                if (s_state[3] >= 5) { s_state[0] = 1; s_state[2] = kTermInvalid; }
                s_ctl[0] /= s_ctl[1];
                s_ctl[1] *= 2.0;
            } else {
                s_state[3] = 0;
                if (sqrt(r4[0]) <= 1e-8 * (sqrt(r4[1]) + 1e-8)) {
                    s_state[0] = 1; s_state[2] = kTermParameter;
                } else {
                    const double change = cost - cand_cost, rho = change / model;
                    if (fabs(change) <= 1e-6 * cost) {
                        // Ceres checks the function tolerance before the accept test: the iterate stays where it was
                        s_state[0] = 1; s_state[2] = kTermFunction;
                    } else {
                        if (rho > 1e-3) {
                            s_ctl[6] = 1.0;
                            s_ctl[2] = cand_cost;
                            s_ctl[0] = fmin(1e16, s_ctl[0] / fmax(1.0 / 3.0, 1.0 - (2.0 * rho - 1.0) * (2.0 * rho - 1.0) * (2.0 * rho - 1.0)));
                            s_ctl[1] = 2.0;
                        } else {
                            s_ctl[0] /= s_ctl[1];
                            s_ctl[1] *= 2.0;
                        }
                        if (s_ctl[0] < 1e-32) { s_state[0] = 1; s_state[2] = kTermRadius; }
                    }
                }
            }
        }
        if constexpr (MODE == kLmTape) if (tid == 0) {
            double* rec = bws[blockIdx.x].tape.it + 3 * size_t(s_state[1] - 1);
            rec[0] = radius; rec[1] = solved ? 1.0 : 0.0; rec[2] = s_ctl[6];
        }
        __syncthreads();
        if (s_ctl[6] != 0.0) {
            if constexpr (MODE == kLmTape) {
                double* x = bws[blockIdx.x].tape.x + size_t(n_acc) * (6 * size_t(C) + 3 * size_t(P));
                if (tid < 6 * C) x[tid] = s_cams[tid];
                for (int i = tid; i < 3 * P; i += kMvThreads) x[6 * C + i] = a.pts[i];
            }
            if constexpr (MODE == kLmTape) ++n_acc;
            if (tid < 6 * C) s_cams[tid] = s_cand[tid];
            for (int i = tid; i < 3 * P; i += kMvThreads) a.pts[i] = a.cand[i];
        }
        __syncthreads();
        if (s_state[0]) {
            if constexpr (MODE == kLmTape) {
                rev = true; rev_k = s_state[1]; rev_j = n_acc;
                mv_reverse_begin(a, bws[blockIdx.x], s_cams, s_rev);
                if (mv_reverse_next(a, bws[blockIdx.x], s_cams, s_ctl, rev_k, rev_j)) continue;
            }
            break;
        }
    }
    if (tid < 6 * C) a.cams[tid] = s_cams[tid];
    if (tid == 0) {
        a.summary[1] = s_ctl[2];
        a.summary[2] = double(s_state[1]);
        a.summary[3] = double(s_state[2]);
    }
    if constexpr (MODE == kLmTape) {
        __syncthreads();
        if (tid < 6 * C) bws[blockIdx.x].cams_bar[tid] = s_rev[tid];
    }
}

}  // namespace e2emv
