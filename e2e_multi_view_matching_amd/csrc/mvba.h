// Declarations shared by the files of the multi-view bundle adjustment (mvba.hip: solver, pairwise problem build;
// mvtracks.hip: track merging and the track problem build).
#pragma once
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
void mv_extr_to_cam(const double* E /* 4x4 row-major */, double* cam);
void mv_cam_to_extr(const double* cam, double* E);

}  // namespace e2emv
