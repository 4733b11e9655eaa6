// Two-view Levenberg-Marquardt bundle adjustment (SURVEY.md 8(f) "next" row 1): the refinement the
// reference runs right after the weighted 8-point solve in its default eval mode (`w8pt_ba`,
// eval_pairs.py:250-255; bundle_adjust_io.py:18-22).
//
// Restates pose_optimization/two_view/bundle_adjust_gauss_newton_2_view.py (Observations :10-48,
// fill_J :50-67, compute_A_b :69-99, BundleAdjustGaussNewton2View.run :127-201) and
// run_bundle_adjust_2_view (estimate_relative_pose.py:138-144).  Camera 0 is fixed at the identity;
// unknowns = 6 pose parameters of camera 1 + 3 per matched point.
//
// The reference builds the dense (6+3M)^2 normal matrix per sample in Python and LU-factorises it
// (M <= 2048 -> 6150^2 fp32 per iteration).  The structure is block-arrow: the point blocks are
// independent 3x3's.  Here ONE workgroup per pair eliminates them analytically (Schur complement):
//   (Hcc' - sum_p Hcp Hpp'^-1 Hcp^T) dc = gc - sum_p Hcp Hpp'^-1 gp,   dp = Hpp'^-1 (gp - Hcp^T dc)
// with H' = H + lambda * diag(H) - algebraically the reference's Jacobi-preconditioned damped system
// (D^-1 J^T J + lambda I) d = D^-1 b.  All accumulation in fp64, reductions by wavefront shuffles,
// the 6x6 solve by one lane.  Same LM control flow as the reference: update ALWAYS applied, best-residual
// pose kept, lambda /= 3.5 on improvement else *= 1.5, n_iterations + 1 residual evaluations.
//
// Robust loss (e2emv_ba_2view_loss; a ceres::LossFunction in a solver that has none upstream): a residual block is one
// observation, so a match has two - s0 = |r0|^2 in image 0, s1 = |r1|^2 in image 1, on the weighted residuals.  The cost the LM
// bookkeeping compares is sum rho(s0) + sum rho(s1); the linearisation is Ceres' corrector for rho'' <= 0, applied once per block
// in point_terms: r0, Jp0 times sqrt(rho'(s0)) and r1, Jp1, Jc times sqrt(rho'(s1)), so that the three passes, the positivity
// check and the preconditioner's floor all see the system that is solved.  rho and sqrt(rho') are mv_loss of mvba.h.
//
// Backward pass (e2emv_ba_2view_backward, e2emv_ba_2view_loss_backward; second half of this file): the exact reverse of the loop, to
// the confidences and the start pose, for the squared loss and for both robust losses - through the corrector and through the pair's
// scale a_b = loss_scale / cden_b.
#include "common.h"
#include "mvba.h"
#include "small_linalg.h"

namespace e2emv {

// block-wide sum of NV doubles (256 threads); result valid in every thread
template <int NV>
__device__ __forceinline__ void block_sum_n(double (&v)[NV], double* red /* [4][NV] */) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const double s = wave_sum_d(v[i]);
        if (lane == 0) red[wave * NV + i] = s;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NV; ++i) v[i] = red[i] + red[NV + i] + red[2 * NV + i] + red[3 * NV + i];
}

// symmetric 3x3 (a00 a01 a02 a11 a12 a22) inverse; returns false when singular
__device__ __forceinline__ bool inv3_sym(const double* a, double* inv) {
    const double c00 = a[3] * a[5] - a[4] * a[4], c01 = a[2] * a[4] - a[1] * a[5], c02 = a[1] * a[4] - a[2] * a[3];
    const double det = a[0] * c00 + a[1] * c01 + a[2] * c02;
    if (!(fabs(det) > 0.0)) return false;
    const double id = 1.0 / det;
    inv[0] = c00 * id; inv[1] = c01 * id; inv[2] = c02 * id;
    inv[3] = (a[0] * a[5] - a[2] * a[2]) * id; inv[4] = (a[1] * a[2] - a[0] * a[4]) * id;
    inv[5] = (a[0] * a[3] - a[1] * a[1]) * id;
    return true;
}

struct BaParams {
    int B, N, n_it;
    const float* k0;    // [B][N][2] normalised keypoints image 0
    const float* k1;
    const float* conf;  // [B][N]
    const float* Tin;   // [B][4][4]
    float* Tout;        // [B][4][4]
    uint8_t* valid;     // [B]
    double* X;          // workspace [B][N][3]
    float lm_inc, lm_dec;
    double loss_scale;  // relative: pair b runs with a_b = loss_scale / cden_b, the denominator of its weights
    double* summary;    // [B][4] or NULL: cost at the start, best cost, evaluations that improved, a_b
};

// per-point quantities for the current pose: residuals and Jacobian blocks (already confidence weighted)
struct PointTerms {
    double r0[2], r1[2];
    double Jp0[2][3], Jp1[2][3], Jc[2][6];
};
// Returns the match's share of the cost: |r0|^2 + |r1|^2 without a loss (today's expression), rho(s0) + rho(s1) with one - taken
// BEFORE the corrector scales the blocks.
template <int LOSS>
__device__ __forceinline__ double point_terms(const double* Rt, const double* X, double x0, double y0, double x1, double y1,
                                              double c, double la, double la2, PointTerms& q) {
    // camera 0: identity
    const double iz0 = 1.0 / X[2];
    q.r0[0] = c * (X[0] * iz0 - x0);
    q.r0[1] = c * (X[1] * iz0 - y0);
    q.Jp0[0][0] = c * iz0; q.Jp0[0][1] = 0.0; q.Jp0[0][2] = -c * X[0] * iz0 * iz0;
    q.Jp0[1][0] = 0.0; q.Jp0[1][1] = c * iz0; q.Jp0[1][2] = -c * X[1] * iz0 * iz0;
    // camera 1: Ap = R X + t
    const double a0 = Rt[0] * X[0] + Rt[1] * X[1] + Rt[2] * X[2] + Rt[9];
    const double a1 = Rt[3] * X[0] + Rt[4] * X[1] + Rt[5] * X[2] + Rt[10];
    const double a2 = Rt[6] * X[0] + Rt[7] * X[1] + Rt[8] * X[2] + Rt[11];
    const double iz = 1.0 / a2;
    q.r1[0] = c * (a0 * iz - x1);
    q.r1[1] = c * (a1 * iz - y1);
    const double j00 = c * iz, j02 = -c * a0 * iz * iz, j11 = c * iz, j12 = -c * a1 * iz * iz;  // c * J_proj (2x3)
#pragma unroll
    for (int k = 0; k < 3; ++k) {  // J_proj R
        q.Jp1[0][k] = j00 * Rt[k] + j02 * Rt[6 + k];
        q.Jp1[1][k] = j11 * Rt[3 + k] + j12 * Rt[6 + k];
    }
    // J_proj [I | -hat(Ap)],  hat(a) = [[0,-a2,a1],[a2,0,-a0],[-a1,a0,0]]
    q.Jc[0][0] = j00; q.Jc[0][1] = 0.0; q.Jc[0][2] = j02;
    q.Jc[1][0] = 0.0; q.Jc[1][1] = j11; q.Jc[1][2] = j12;
    q.Jc[0][3] = -(j02 * (-a1));          // -(J row . hat column 0) ; hat col0 = (0, a2, -a1)
    q.Jc[0][4] = -(j00 * (-a2) + j02 * a0);   // hat col1 = (-a2, 0, a0)
    q.Jc[0][5] = -(j00 * a1);                 // hat col2 = (a1, -a0, 0)
    q.Jc[1][3] = -(j11 * a2 + j12 * (-a1));
    q.Jc[1][4] = -(j12 * a0);
    q.Jc[1][5] = -(j11 * (-a0));
    if (LOSS == kLossNone) return q.r0[0] * q.r0[0] + q.r0[1] * q.r0[1] + q.r1[0] * q.r1[0] + q.r1[1] * q.r1[1];
    double rho0, sq0, rho1, sq1;
    mv_loss<LOSS>(q.r0[0] * q.r0[0] + q.r0[1] * q.r0[1], la, la2, &rho0, &sq0);
    mv_loss<LOSS>(q.r1[0] * q.r1[0] + q.r1[1] * q.r1[1], la, la2, &rho1, &sq1);
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        q.r0[r] *= sq0;
        q.r1[r] *= sq1;
#pragma unroll
        for (int k = 0; k < 3; ++k) { q.Jp0[r][k] *= sq0; q.Jp1[r][k] *= sq1; }
#pragma unroll
        for (int k = 0; k < 6; ++k) q.Jc[r][k] *= sq1;
    }
    return rho0 + rho1;
}

// The point block of one match, as every pass over the matches forms it: Hpp = Jp^T Jp (symmetric 3x3, packed a00 a01 a02 a11 a12 a22)
__device__ __forceinline__ void point_hpp(const PointTerms& q, double* Hpp) {
    int idx = 0;
#pragma unroll
    for (int u = 0; u < 3; ++u)
#pragma unroll
        for (int v = u; v < 3; ++v)
            Hpp[idx++] = q.Jp0[0][u] * q.Jp0[0][v] + q.Jp0[1][u] * q.Jp0[1][v] + q.Jp1[0][u] * q.Jp1[0][v] + q.Jp1[1][u] * q.Jp1[1][v];
}
// its damping: lambda times the (floored) diagonal under the Jacobi preconditioner, lambda I without
__device__ __forceinline__ void point_damp(double* Hpp, double lam, bool precond) {
    Hpp[0] += lam * (precond ? fmax(Hpp[0], 1e-12) : 1.0);
    Hpp[3] += lam * (precond ? fmax(Hpp[3], 1e-12) : 1.0);
    Hpp[5] += lam * (precond ? fmax(Hpp[5], 1e-12) : 1.0);
}
// gp = -Jp^T r
__device__ __forceinline__ void point_gp(const PointTerms& q, double* gp) {
#pragma unroll
    for (int u = 0; u < 3; ++u) gp[u] = -(q.Jp0[0][u] * q.r0[0] + q.Jp0[1][u] * q.r0[1] + q.Jp1[0][u] * q.r1[0] + q.Jp1[1][u] * q.r1[1]);
}
// Hcp = Jc^T Jp1 (6x3): camera 0 is fixed, so only the observation in image 1 couples the pose and the point
__device__ __forceinline__ void point_hcp(const PointTerms& q, double (&Hcp)[6][3]) {
#pragma unroll
    for (int u = 0; u < 6; ++u)
#pragma unroll
        for (int v = 0; v < 3; ++v) Hcp[u][v] = q.Jc[0][u] * q.Jp1[0][v] + q.Jc[1][u] * q.Jp1[1][v];
}
// one row of W = Hcp Hpp'^-1
__device__ __forceinline__ void point_w_row(const double* h, const double* inv, double* w) {
    w[0] = h[0] * inv[0] + h[1] * inv[1] + h[2] * inv[2];
    w[1] = h[0] * inv[1] + h[1] * inv[3] + h[2] * inv[4];
    w[2] = h[0] * inv[2] + h[1] * inv[4] + h[2] * inv[5];
}
// y = Hpp'^-1 x
__device__ __forceinline__ void point_solve(const double* inv, const double* x, double* y) {
    y[0] = inv[0] * x[0] + inv[1] * x[1] + inv[2] * x[2];
    y[1] = inv[1] * x[0] + inv[3] * x[1] + inv[4] * x[2];
    y[2] = inv[2] * x[0] + inv[4] * x[1] + inv[5] * x[2];
}

// [M | rhs] of the reduced camera system in LDS and its solution by Gaussian elimination with partial pivoting (fp64), one lane:
// a = camera block (21 packed, then 6 right-hand sides), s = what the point blocks take from it.  M6 is in LDS because the pivot
// search indexes its rows at run time, which in a private array means scratch memory.  A singular system or a non-finite
// solution returns false: the reference skips the update when LU reports info != 0.
template <int NA>
__device__ __forceinline__ bool schur6_solve(double (&M6)[6][7], const double (&a)[NA], const double (&s)[27], double lam, bool precond,
                                             double* x) {
    const int dpos[6] = {0, 6, 11, 15, 18, 20};
    int idx = 0;
    for (int u = 0; u < 6; ++u)
        for (int v = u; v < 6; ++v) {
            const double h = a[idx] - s[idx];
            M6[u][v] = h;
            M6[v][u] = h;
            ++idx;
        }
    for (int u = 0; u < 6; ++u) {
        M6[u][u] += lam * (precond ? fmax(a[dpos[u]], 1e-12) : 1.0);
        M6[u][6] = a[21 + u] - s[21 + u];
    }
    bool ok = true;
    for (int c = 0; c < 6 && ok; ++c) {
        int piv = c;
        for (int r = c + 1; r < 6; ++r)
            if (fabs(M6[r][c]) > fabs(M6[piv][c])) piv = r;
        if (!(fabs(M6[piv][c]) > 0.0)) { ok = false; break; }
        if (piv != c)
            for (int k = 0; k < 7; ++k) { const double t = M6[c][k]; M6[c][k] = M6[piv][k]; M6[piv][k] = t; }
        for (int r = c + 1; r < 6; ++r) {
            const double f = M6[r][c] / M6[c][c];
            for (int k = c; k < 7; ++k) M6[r][k] -= f * M6[c][k];
        }
    }
    if (ok) {
        for (int c = 5; c >= 0; --c) {
            double v = M6[c][6];
            for (int k = c + 1; k < 6; ++k) v -= M6[c][k] * x[k];
            x[c] = v / M6[c][c];
            ok = ok && isfinite(x[c]);
        }
    }
    return ok;
}

// pytorch3d's se3_exp_map with its 1e-4 clamp of |w|^2 (:193-195): coefficients and matrices of exp(dc), dc = (v, w)
struct ExpTerms {
    double th, f1, f2, f3;
    bool clamped;
    double Kx[9], K2[9], Rd[9], Vm[9];
};
__device__ __forceinline__ void se3_exp_terms(const double* dc, ExpTerms& e) {
    const double wx = dc[3], wy = dc[4], wz = dc[5];
    const double n2 = wx * wx + wy * wy + wz * wz;
    const double th2 = fmax(n2, 1e-4), th = sqrt(th2);
    e.clamped = n2 < 1e-4;
    e.th = th;
    e.f1 = sin(th) / th; e.f2 = (1.0 - cos(th)) / th2; e.f3 = (th - sin(th)) / (th2 * th);
    const double Kx[9] = {0, -wz, wy, wz, 0, -wx, -wy, wx, 0};
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) e.K2[i * 3 + j] = Kx[i * 3] * Kx[j] + Kx[i * 3 + 1] * Kx[3 + j] + Kx[i * 3 + 2] * Kx[6 + j];
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        const double d = (i % 4 == 0) ? 1.0 : 0.0;
        e.Kx[i] = Kx[i];
        e.Rd[i] = d + e.f1 * Kx[i] + e.f2 * e.K2[i];
        e.Vm[i] = d + e.f2 * Kx[i] + e.f3 * e.K2[i];
    }
}
// extr1 <- exp(dc) extr1: out = exp(dc) Rt (R row-major 0..8, t 9..11)
__device__ __forceinline__ void se3_exp_left(const double* dc, const double* Rt, double* out) {
    ExpTerms e;
    se3_exp_terms(dc, e);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const double td = e.Vm[i * 3] * dc[0] + e.Vm[i * 3 + 1] * dc[1] + e.Vm[i * 3 + 2] * dc[2];
#pragma unroll
        for (int j = 0; j < 3; ++j) out[i * 3 + j] = e.Rd[i * 3] * Rt[j] + e.Rd[i * 3 + 1] * Rt[3 + j] + e.Rd[i * 3 + 2] * Rt[6 + j];
        out[9 + i] = e.Rd[i * 3] * Rt[9] + e.Rd[i * 3 + 1] * Rt[10] + e.Rd[i * 3 + 2] * Rt[11] + td;
    }
}

constexpr int kBaRec = 20;  // doubles per evaluation record: Rt (12), lambda, flags (1 precond, 2 update skipped), dc (6)

// What the loop keeps besides the pose it moves: the forward the best pose and the figures of its summary, the tape k* alone
template <bool TAPE>
struct BaLmKept {
    double best[12], startR;
    int improved;
};
template <>
struct BaLmKept<true> {
    int kstar;  // the evaluation whose pose became the result
};
// LDS of one pair's workgroup
template <bool TAPE>
struct BaLmShared {
    double red[4 * 32];
    double Rt[12], delta[6];
    double lam, bestR;
    double M6[6][7];
    int flags;  // bit0: skip update this iteration
    BaLmKept<TAPE> kept;
};

// THE Levenberg-Marquardt loop of one pair, for the forward (TAPE = false) and for the replay in front of the reverse pass (TAPE =
// true): the reverse pass is right only if the replay takes every accept / reject / skip decision as the forward did, and this being
// one text is what guarantees it.  Evaluation `it` reads its points at Xs + it * xs and writes the moved ones at Xs + (it + 1) * xs:
// xs = 0 updates them in place (forward), xs = 3 N keeps every X_k (tape), and a point or a step that is not moved is then copied.
// The tape also writes one record of kBaRec doubles per evaluation to recs.  Returns the validity of the pair (more than 6 positive
// confidences; nothing else is done without); csum = sum of the confidences, cden = the weights' denominator, la = the loss scale.
template <int LOSS, bool TAPE>
__device__ __forceinline__ bool ba2view_lm(BaLmShared<TAPE>& sh, int N, int n_it, const float* k0, const float* k1, const float* cf,
                                           const float* Ti, double* Xs, size_t xs, double* recs, float lm_inc, float lm_dec,
                                           double loss_scale, double& csum, double& cden, double& la) {
    const int tid = threadIdx.x;
    // confidence normalisation (:45-48: each match = two observations) and validity (:132-136)
    double st[2] = {0.0, 0.0};
    for (int i = tid; i < N; i += 256)
        if (cf[i] > 0.f) { st[0] += (double)cf[i]; st[1] += 1.0; }
    block_sum_n<2>(st, sh.red);
    csum = st[0];
    cden = 0.5 * fmax(2.0 * st[0], 1e-6);
    la = LOSS != kLossNone ? loss_scale / cden : 0.0;
    const double la2 = la * la;
    if (!(st[1] > 6.5)) return false;

    if (tid < 12) {
        const int r = tid < 9 ? tid / 3 : tid - 9, c = tid < 9 ? tid % 3 : 3;
        sh.Rt[tid] = (double)Ti[r * 4 + c];   // R row-major (0..8), t (9..11)
        if constexpr (!TAPE) sh.kept.best[tid] = sh.Rt[tid];
    }
    if (tid == 0) {
        sh.lam = 0.1; sh.bestR = 0.0; sh.flags = 0;
        if constexpr (TAPE) { sh.kept.kstar = 0; } else { sh.kept.improved = 0; sh.kept.startR = 0.0; }
    }
    __syncthreads();
    for (int i = tid; i < N; i += 256)
        if (cf[i] > 0.f) triangulate_xyz(k0[2 * i], k0[2 * i + 1], k1[2 * i], k1[2 * i + 1], sh.Rt, Xs + 3 * i);
    __syncthreads();

    for (int it = 0; it <= n_it; ++it) {
        const double* X = Xs + it * xs;
        double* Xn = Xs + (it + 1) * xs;  // written only when it < n_it
        double Rt[12];
#pragma unroll
        for (int k = 0; k < 12; ++k) Rt[k] = sh.Rt[k];
        // ---- pass 1: residual norm, camera block Hcc (21), gc (6), positivity of the diagonal
        double a[29];
#pragma unroll
        for (int k = 0; k < 29; ++k) a[k] = 0.0;
        for (int i = tid; i < N; i += 256) {
            if (!(cf[i] > 0.f)) continue;
            PointTerms q;
            a[27] += point_terms<LOSS>(Rt, X + 3 * i, k0[2 * i], k0[2 * i + 1], k1[2 * i], k1[2 * i + 1], (double)cf[i] / cden, la, la2, q);
            int idx = 0;
#pragma unroll
            for (int u = 0; u < 6; ++u) {
#pragma unroll
                for (int v = u; v < 6; ++v) a[idx++] += q.Jc[0][u] * q.Jc[0][v] + q.Jc[1][u] * q.Jc[1][v];
                a[21 + u] -= q.Jc[0][u] * q.r1[0] + q.Jc[1][u] * q.r1[1];
            }
            // point diagonal must be > 0 for the Jacobi preconditioner (:171-173)
            bool pos = true;
#pragma unroll
            for (int k = 0; k < 3; ++k)
                pos = pos && (q.Jp0[0][k] * q.Jp0[0][k] + q.Jp0[1][k] * q.Jp0[1][k] + q.Jp1[0][k] * q.Jp1[0][k] + q.Jp1[1][k] * q.Jp1[1][k]) > 0.0;
            if (!pos) a[28] += 1.0;
        }
        block_sum_n<29>(a, sh.red);
        // ---- LM bookkeeping (:150-161), identical in every thread
        const double rn = a[27];
        if (tid == 0) {
            if (it == 0) {
                sh.bestR = rn;
                if constexpr (!TAPE) sh.kept.startR = rn;
            } else if (rn < sh.bestR) {
                sh.bestR = rn;
                if constexpr (TAPE) {
                    sh.kept.kstar = it;
                } else {
                    ++sh.kept.improved;
#pragma unroll
                    for (int k = 0; k < 12; ++k) sh.kept.best[k] = Rt[k];
                }
                sh.lam = sh.lam / (double)lm_dec;
            } else {
                sh.lam = sh.lam * (double)lm_inc;
            }
        }
        __syncthreads();
        if (it == n_it) break;
        const double lam = sh.lam;
        // camera diagonal positions in the packed upper triangle: 0, 6, 11, 15, 18, 20
        const int dpos[6] = {0, 6, 11, 15, 18, 20};
        bool precond = a[28] < 0.5;
#pragma unroll
        for (int u = 0; u < 6; ++u) precond = precond && a[dpos[u]] > 0.0;

        // ---- pass 2: Schur complement of the point blocks
        double s[27];
#pragma unroll
        for (int k = 0; k < 27; ++k) s[k] = 0.0;
        for (int i = tid; i < N; i += 256) {
            if (!(cf[i] > 0.f)) continue;
            PointTerms q;
            point_terms<LOSS>(Rt, X + 3 * i, k0[2 * i], k0[2 * i + 1], k1[2 * i], k1[2 * i + 1], (double)cf[i] / cden, la, la2, q);
            double Hpp[6], gp[3], Hcp[6][3], inv[6];
            point_hpp(q, Hpp);
            point_gp(q, gp);
            point_hcp(q, Hcp);
            point_damp(Hpp, lam, precond);
            if (!inv3_sym(Hpp, inv)) continue;
            double W[6][3];
#pragma unroll
            for (int u = 0; u < 6; ++u) point_w_row(Hcp[u], inv, W[u]);
            int idx = 0;
#pragma unroll
            for (int u = 0; u < 6; ++u) {
#pragma unroll
                for (int v = u; v < 6; ++v) s[idx++] += W[u][0] * Hcp[v][0] + W[u][1] * Hcp[v][1] + W[u][2] * Hcp[v][2];
                s[21 + u] += W[u][0] * gp[0] + W[u][1] * gp[1] + W[u][2] * gp[2];
            }
        }
        block_sum_n<27>(s, sh.red);
        if (tid == 0) {
            const bool ok = schur6_solve(sh.M6, a, s, lam, precond, sh.delta);
            sh.flags = ok ? 0 : 1;
            if constexpr (TAPE) {
                double* rec = recs + (size_t)it * kBaRec;
#pragma unroll
                for (int k = 0; k < 12; ++k) rec[k] = Rt[k];
                rec[12] = lam;
                rec[13] = (double)((precond ? 1 : 0) | (ok ? 0 : 2));
#pragma unroll
                for (int k = 0; k < 6; ++k) rec[14 + k] = ok ? sh.delta[k] : 0.0;
            }
        }
        __syncthreads();
        if (sh.flags & 1) {  // singular system: the update is skipped, the next evaluation sees the same points
            if (Xn != X) {
                for (int i = tid; i < N; i += 256)
                    if (cf[i] > 0.f) { Xn[3 * i] = X[3 * i]; Xn[3 * i + 1] = X[3 * i + 1]; Xn[3 * i + 2] = X[3 * i + 2]; }
                __syncthreads();
            }
            continue;
        }
        double dc[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) dc[k] = sh.delta[k];
        // ---- pass 3: back-substitute the points with the OLD pose, then move the pose
        for (int i = tid; i < N; i += 256) {
            if (!(cf[i] > 0.f)) continue;
            PointTerms q;
            point_terms<LOSS>(Rt, X + 3 * i, k0[2 * i], k0[2 * i + 1], k1[2 * i], k1[2 * i + 1], (double)cf[i] / cden, la, la2, q);
            double Hpp[6], rhs[3], Hcp[6][3], inv[6], d[3];
            point_hpp(q, Hpp);
            point_gp(q, rhs);
            point_hcp(q, Hcp);
#pragma unroll
            for (int u = 0; u < 3; ++u)
#pragma unroll
                for (int w = 0; w < 6; ++w) rhs[u] -= Hcp[w][u] * dc[w];
            point_damp(Hpp, lam, precond);
            if (!inv3_sym(Hpp, inv)) {  // this point stays where it is
                if (Xn != X) { Xn[3 * i] = X[3 * i]; Xn[3 * i + 1] = X[3 * i + 1]; Xn[3 * i + 2] = X[3 * i + 2]; }
                continue;
            }
            point_solve(inv, rhs, d);
            Xn[3 * i] = X[3 * i] + d[0];
            Xn[3 * i + 1] = X[3 * i + 1] + d[1];
            Xn[3 * i + 2] = X[3 * i + 2] + d[2];
        }
        __syncthreads();
        if (tid == 0) {
            double Rn[12];
            se3_exp_left(dc, Rt, Rn);
#pragma unroll
            for (int i = 0; i < 12; ++i) sh.Rt[i] = Rn[i];
        }
        __syncthreads();
    }
    return true;
}

template <int LOSS>
__global__ __launch_bounds__(256) void ba2view_kernel(BaParams p) {
    __shared__ BaLmShared<false> sh;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int N = p.N;
    const float* Ti = p.Tin + (int64_t)b * 16;
    if (tid < 16) p.Tout[(int64_t)b * 16 + tid] = Ti[tid];
    double csum, cden, la;
    const bool valid = ba2view_lm<LOSS, false>(sh, N, p.n_it, p.k0 + (int64_t)b * N * 2, p.k1 + (int64_t)b * N * 2, p.conf + (int64_t)b * N, Ti,
                                               p.X + (int64_t)b * N * 3, 0, nullptr, p.lm_inc, p.lm_dec, p.loss_scale, csum, cden, la);
    if (tid == 0) p.valid[b] = valid ? 1 : 0;
    if (!valid) {
        if (p.summary && tid < 4) p.summary[(int64_t)b * 4 + tid] = 0.0;
        return;
    }
    if (tid < 12) {
        const int r = tid < 9 ? tid / 3 : tid - 9, c = tid < 9 ? tid % 3 : 3;
        p.Tout[(int64_t)b * 16 + r * 4 + c] = (float)sh.kept.best[tid];
    }
    if (p.summary && tid == 0) {
        double* sm = p.summary + (int64_t)b * 4;
        sm[0] = sh.kept.startR; sm[1] = sh.bestR; sm[2] = (double)sh.kept.improved; sm[3] = la;
    }
}

}  // namespace e2emv

using namespace e2emv;

// both entry points; `who` names the caller in error texts
static int ba2view_run(e2emv_ctx* ctx, const char* who, int B, int N, const float* d_kpts0n, const float* d_kpts1n, const float* d_conf,
                       const float* d_T_init, int n_iterations, float* d_T_out, uint8_t* d_valid, int loss, double loss_scale,
                       double* d_summary, void* stream) {
    if (!ctx || !d_kpts0n || !d_kpts1n || !d_conf || !d_T_init || !d_T_out || !d_valid) return E2EMV_EINVAL;
    E2EMV_ENTER(ctx, stream);
    int rc = mv_check_loss(ctx, who, loss, &loss_scale);
    if (rc) return rc;
    if (B <= 0 || N <= 0 || n_iterations < 0) return set_err(ctx, E2EMV_ESHAPE, "%s: B=%d N=%d iterations=%d", who, B, N, n_iterations);
    hipStream_t s = (hipStream_t)stream;
    rc = ws_reserve(ctx, (size_t)B * N * 3 * sizeof(double) + 256);
    if (rc) return rc;
    BaParams p{};
    p.B = B; p.N = N; p.n_it = n_iterations;
    p.k0 = d_kpts0n; p.k1 = d_kpts1n; p.conf = d_conf; p.Tin = d_T_init; p.Tout = d_T_out; p.valid = d_valid;
    p.X = (double*)ctx->d_ws;
    p.lm_inc = 1.5f; p.lm_dec = 3.5f;
    p.loss_scale = loss_scale; p.summary = d_summary;
    prof_begin(ctx, PS_W8PT, s);
    if (loss == kLossHuber) hipLaunchKernelGGL(ba2view_kernel<kLossHuber>, dim3(B), dim3(256), 0, s, p);
    else if (loss == kLossCauchy) hipLaunchKernelGGL(ba2view_kernel<kLossCauchy>, dim3(B), dim3(256), 0, s, p);
    else hipLaunchKernelGGL(ba2view_kernel<kLossNone>, dim3(B), dim3(256), 0, s, p);
    prof_end(ctx, s);
    E2EMV_CHECK_LAUNCH(ctx, "ba2view_kernel");
    return E2EMV_OK;
}

extern "C" int e2emv_ba_2view(e2emv_ctx* ctx, int B, int N, const float* d_kpts0n, const float* d_kpts1n, const float* d_conf,
                              const float* d_T_init, int n_iterations, float* d_T_out, uint8_t* d_valid, void* stream) {
    return ba2view_run(ctx, "ba_2view", B, N, d_kpts0n, d_kpts1n, d_conf, d_T_init, n_iterations, d_T_out, d_valid, E2EMV_LOSS_NONE, 0.0,
                       nullptr, stream);
}

extern "C" int e2emv_ba_2view_loss(e2emv_ctx* ctx, int B, int N, const float* d_kpts0n, const float* d_kpts1n, const float* d_conf,
                                   const float* d_T_init, int n_iterations, float* d_T_out, uint8_t* d_valid, int loss, double loss_scale,
                                   double* d_summary, void* stream) {
    return ba2view_run(ctx, "ba_2view_loss", B, N, d_kpts0n, d_kpts1n, d_conf, d_T_init, n_iterations, d_T_out, d_valid, loss, loss_scale,
                       d_summary, stream);
}

// ---- backward pass of ba2view_kernel<LOSS>: dLoss/dconf and dLoss/dT_init from dLoss/dT_out (e2emv_ba_2view_backward for the squared
// loss, e2emv_ba_2view_loss_backward for all three) ----
//
// Phase 1 replays the forward loop from the inputs - ba2view_lm<LOSS, true>, the very function the forward kernel runs, so that
// every accept / reject decision is the forward's - and keeps a tape in the workspace: X_k of every evaluation, and per evaluation a
// record (Rt_k, lambda_k, precond, skipped, dc_k).  k* = the evaluation whose pose became the result.  Phase 2 walks k = k*-1 .. 0 with the
// adjoint state (Rt_bar in LDS, X_bar in the workspace).  One LM step solves M d = b, M = A + lambda D, A = J^T J, b = -J^T r, D =
// diag(max(A_jj, 1e-12)) under precond, else I.  With d_bar = (adjoint of exp(dc) Rt_k w.r.t. dc, X_bar_{k+1}) and M w = d_bar -
// the forward's Schur complement with another right-hand side -
//     J_bar = -(J w) d^T - (J d + r) w^T - 2 lambda J diag(w o d) [columns with D_jj = A_jj],   r_bar = -J w,
// per match (two observations, 6 camera + 3 point columns), taken back through point_terms to X_bar_k, Rt_bar_k and the weight's
// adjoint.  After k = 0: the triangulation (first-order perturbation of the null vector of G = A^T A from the Jacobi eigenpairs,
// then 1 / (X3 + 1e-8)) and the normalisation of the weights.  lambda, the comparisons and k* are piecewise constant.
// Phase 2 forms the point blocks with the loop's helpers (point_hpp, point_damp, point_hcp, point_w_row, point_solve) and solves its
// 6x6 system with the loop's schur6_solve.
//
// With a loss the system that is solved is the CORRECTED one, r~ = sq r and J~ = sq J per observation block (block 0: r0, Jp0; block
// 1: r1, Jp1, Jc), sq = sqrt(rho'(s)), s = |r|^2 of the uncorrected weighted residual, at the pair's scale a = loss_scale / cden.  The
// formulas above then give the adjoint of (r~, J~), and one more step takes it to the uncorrected terms and to a, per block:
//     sq_bar = <r~_bar, r> + <J~_bar, J>,   r_bar = sq r~_bar + 2 (dsq/ds) sq_bar r,   J_bar = sq J~_bar,   a_bar += (dsq/da) sq_bar
//     cauchy: dsq/ds = -sq^3 / (2 a^2), dsq/da = sq^3 s / a^3;   huber: s <= a^2: both 0, else dsq/ds = -sq / (4 s), dsq/da = sq / (2 a)
// with (r, J) from point_terms<kLossNone> and sq from mv_loss on top of it, in the order point_terms<LOSS> uses; point_terms_reverse
// runs unchanged on (r_bar, J_bar).  a_bar is summed over matches and steps per thread and across the workgroup once, at the end:
// a = loss_scale / cden with cden = sum conf gives every positive-confidence row -a_bar a / cden (nothing where cden is the clamp).
// rho itself - the costs that are compared - carries nothing.  All of it is compiled for LOSS != kLossNone only.
namespace e2emv {

struct BaBwdParams {
    int B, N, n_it;
    const float *k0, *k1, *conf, *Tin, *gT;
    float* gconf;   // [B][N] or NULL
    float* gTin;    // [B][4][4] or NULL
    double* ws;     // per pair: X tape [n_it + 1][N][3], X_bar [N][3], c_bar [N], records [n_it + 1][kBaRec]
    size_t stride;  // doubles per pair
    float lm_inc, lm_dec;
};
// ... and with a loss (the squared-loss kernel keeps the arguments it has)
struct BaBwdLossParams : BaBwdParams {
    double loss_scale;  // relative, as in BaParams
};
template <int LOSS>
struct BaBwdArgs { using type = BaBwdLossParams; };
template <>
struct BaBwdArgs<kLossNone> { using type = BaBwdParams; };

// d sqrt(rho'(s)) / ds and / da of mv_loss<LOSS> (sq = its sqrt(rho'(s))); Huber's kink at s = a2 takes the first branch, like mv_loss
template <int LOSS>
__device__ __forceinline__ void mv_loss_sq_reverse(double s, double sq, double a, double a2, double* dsq_ds, double* dsq_da) {
    if (LOSS == kLossHuber) {
        if (s <= a2) {
            *dsq_ds = 0.0; *dsq_da = 0.0;
        } else {
            *dsq_ds = -sq / (4.0 * s); *dsq_da = sq / (2.0 * a);
        }
    } else {
        const double sq3 = sq * sq * sq;
        *dsq_ds = -sq3 / (2.0 * a2); *dsq_da = sq3 * s / (a2 * a);
    }
}

// adjoint of se3_exp_left: nb = adjoint of the new pose -> dcb [6], and tb [12] = the part of the old pose's adjoint that comes
// through the product.  In the clamped branch f1, f2, f3 are constants: the derivative flows through hat(w) only.
__device__ __forceinline__ void se3_exp_left_reverse(const double* dc, const double* Rt, const double* nb, double* dcb, double* tb) {
    ExpTerms e;
    se3_exp_terms(dc, e);
    double Rdb[9], Vmb[9], K2b[9], Kxb[9];
    double f1b = 0.0, f2b = 0.0, f3b = 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            Rdb[i * 3 + j] = nb[i * 3] * Rt[j * 3] + nb[i * 3 + 1] * Rt[j * 3 + 1] + nb[i * 3 + 2] * Rt[j * 3 + 2] + nb[9 + i] * Rt[9 + j];
            Vmb[i * 3 + j] = nb[9 + i] * dc[j];
        }
#pragma unroll
    for (int j = 0; j < 3; ++j) dcb[j] = e.Vm[j] * nb[9] + e.Vm[3 + j] * nb[10] + e.Vm[6 + j] * nb[11];
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        f1b += Rdb[i] * e.Kx[i];
        f2b += Rdb[i] * e.K2[i] + Vmb[i] * e.Kx[i];
        f3b += Vmb[i] * e.K2[i];
        K2b[i] = e.f2 * Rdb[i] + e.f3 * Vmb[i];
    }
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            double v = e.f1 * Rdb[i * 3 + j] + e.f2 * Vmb[i * 3 + j];
#pragma unroll
            for (int k = 0; k < 3; ++k) v += K2b[i * 3 + k] * e.Kx[j * 3 + k] + e.Kx[k * 3 + i] * K2b[k * 3 + j];  // K2b Kx^T + Kx^T K2b
            Kxb[i * 3 + j] = v;
        }
    dcb[3] = Kxb[7] - Kxb[5];
    dcb[4] = Kxb[2] - Kxb[6];
    dcb[5] = Kxb[3] - Kxb[1];
    if (!e.clamped) {
        const double th = e.th, sn = sin(th), cs = cos(th), th2 = th * th;
        const double thb = f1b * (th * cs - sn) / th2 + f2b * (th * sn - 2.0 * (1.0 - cs)) / (th2 * th) +
                           f3b * ((1.0 - cs) * th - 3.0 * (th - sn)) / (th2 * th2);
#pragma unroll
        for (int k = 0; k < 3; ++k) dcb[3 + k] += thb * dc[3 + k] / th;
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) tb[i * 3 + j] = e.Rd[i] * nb[j] + e.Rd[3 + i] * nb[3 + j] + e.Rd[6 + i] * nb[6 + j];
        tb[9 + i] = e.Rd[i] * nb[9] + e.Rd[3 + i] * nb[10] + e.Rd[6 + i] * nb[11];
    }
}

// adjoint of point_terms<kLossNone>: qb holds the adjoints of q's entries (those of the structural zeros are not read) -> Xb [3],
// g [12] += the pose's share, returns the weight's adjoint
__device__ __forceinline__ double point_terms_reverse(const double* Rt, const double* X, double x0, double y0, double x1, double y1, double c,
                                                      const PointTerms& qb, double* Xb, double* g) {
    const double iz0 = 1.0 / X[2];
    double cb = qb.r0[0] * (X[0] * iz0 - x0) + qb.r0[1] * (X[1] * iz0 - y0) + (qb.Jp0[0][0] + qb.Jp0[1][1]) * iz0 -
                (qb.Jp0[0][2] * X[0] + qb.Jp0[1][2] * X[1]) * iz0 * iz0;
    Xb[0] = qb.r0[0] * c * iz0 - qb.Jp0[0][2] * c * iz0 * iz0;
    Xb[1] = qb.r0[1] * c * iz0 - qb.Jp0[1][2] * c * iz0 * iz0;
    const double iz0b = c * (qb.r0[0] * X[0] + qb.r0[1] * X[1]) + c * (qb.Jp0[0][0] + qb.Jp0[1][1]) -
                        2.0 * c * iz0 * (qb.Jp0[0][2] * X[0] + qb.Jp0[1][2] * X[1]);
    Xb[2] = -iz0b * iz0 * iz0;
    const double a0 = Rt[0] * X[0] + Rt[1] * X[1] + Rt[2] * X[2] + Rt[9];
    const double a1 = Rt[3] * X[0] + Rt[4] * X[1] + Rt[5] * X[2] + Rt[10];
    const double a2 = Rt[6] * X[0] + Rt[7] * X[1] + Rt[8] * X[2] + Rt[11];
    const double iz = 1.0 / a2;
    const double j00 = c * iz, j02 = -c * a0 * iz * iz, j11 = c * iz, j12 = -c * a1 * iz * iz;
    cb += qb.r1[0] * (a0 * iz - x1) + qb.r1[1] * (a1 * iz - y1);
    double ab[3] = {qb.r1[0] * c * iz, qb.r1[1] * c * iz, 0.0};
    double izb = c * (qb.r1[0] * a0 + qb.r1[1] * a1);
    double j00b = qb.Jc[0][0] + qb.Jc[0][4] * a2 - qb.Jc[0][5] * a1;
    double j02b = qb.Jc[0][2] + qb.Jc[0][3] * a1 - qb.Jc[0][4] * a0;
    double j11b = qb.Jc[1][1] - qb.Jc[1][3] * a2 + qb.Jc[1][5] * a0;
    double j12b = qb.Jc[1][2] + qb.Jc[1][3] * a1 - qb.Jc[1][4] * a0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        j00b += qb.Jp1[0][k] * Rt[k];
        j02b += qb.Jp1[0][k] * Rt[6 + k];
        j11b += qb.Jp1[1][k] * Rt[3 + k];
        j12b += qb.Jp1[1][k] * Rt[6 + k];
        g[k] += qb.Jp1[0][k] * j00;
        g[3 + k] += qb.Jp1[1][k] * j11;
        g[6 + k] += qb.Jp1[0][k] * j02 + qb.Jp1[1][k] * j12;
    }
    ab[0] += -qb.Jc[0][4] * j02 - qb.Jc[1][4] * j12 + qb.Jc[1][5] * j11;
    ab[1] += qb.Jc[0][3] * j02 - qb.Jc[0][5] * j00 + qb.Jc[1][3] * j12;
    ab[2] += qb.Jc[0][4] * j00 - qb.Jc[1][3] * j11;
    cb += (j00b + j11b) * iz - (j02b * a0 + j12b * a1) * iz * iz;
    izb += (j00b + j11b) * c - 2.0 * c * iz * (j02b * a0 + j12b * a1);
    ab[0] -= j02b * c * iz * iz;
    ab[1] -= j12b * c * iz * iz;
    ab[2] -= izb * iz * iz;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int k = 0; k < 3; ++k) g[3 * r + k] += ab[r] * X[k];
        g[9 + r] += ab[r];
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) Xb[k] += ab[0] * Rt[k] + ab[1] * Rt[3 + k] + ab[2] * Rt[6 + k];
    return cb;
}

// adjoint of triangulate_xyz w.r.t. the pose: g [12] += .  The null vector v of G = A^T A moves by dv = -sum_{j != m} v_j v_j^T dG v /
// (l_j - l_m); with u = -sum_j v_j (v_j . v_bar) / (l_j - l_m) the adjoint of A is (A u) v^T + (A v) u^T, of which rows 2 and 3 hold the pose.
__device__ __forceinline__ void triangulate_reverse(double x1, double y1, double x2, double y2, const double* Rt, const double* Xb, double* g) {
    double Ar[4][4];
    Ar[0][0] = -1.0; Ar[0][1] = 0.0; Ar[0][2] = x1; Ar[0][3] = 0.0;
    Ar[1][0] = 0.0; Ar[1][1] = -1.0; Ar[1][2] = y1; Ar[1][3] = 0.0;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        Ar[2][j] = x2 * Rt[6 + j] - Rt[j];
        Ar[3][j] = y2 * Rt[6 + j] - Rt[3 + j];
    }
    Ar[2][3] = x2 * Rt[11] - Rt[9];
    Ar[3][3] = y2 * Rt[11] - Rt[10];
    double G[4][4], V[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = i; j < 4; ++j) {
            const double v = Ar[0][i] * Ar[0][j] + Ar[1][i] * Ar[1][j] + Ar[2][i] * Ar[2][j] + Ar[3][i] * Ar[3][j];
            G[i][j] = v;
            G[j][i] = v;
        }
    jacobi_static<4>(G, V);
    int m = 0;
    double gm = G[0][0];
#pragma unroll
    for (int i = 1; i < 4; ++i)
        if (G[i][i] < gm) { gm = G[i][i]; m = i; }
    double v[4], vb[4], u[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = (m == 0) ? V[i][0] : (m == 1) ? V[i][1] : (m == 2) ? V[i][2] : V[i][3];
    const bool big = fabs(v[3]) > 1e-8;
    const double sc = big ? 1.0 / (v[3] + 1e-8) : 1.0;
    vb[0] = Xb[0] * sc; vb[1] = Xb[1] * sc; vb[2] = Xb[2] * sc;
    vb[3] = big ? -(Xb[0] * v[0] + Xb[1] * v[1] + Xb[2] * v[2]) * sc * sc : 0.0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const double gap = G[j][j] - gm;
        if (j == m || !(fabs(gap) > 0.0)) continue;
        const double coef = -(V[0][j] * vb[0] + V[1][j] * vb[1] + V[2][j] * vb[2] + V[3][j] * vb[3]) / gap;
#pragma unroll
        for (int i = 0; i < 4; ++i) u[i] += coef * V[i][j];
    }
    double Au[2], Av[2];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        Au[r] = Ar[2 + r][0] * u[0] + Ar[2 + r][1] * u[1] + Ar[2 + r][2] * u[2] + Ar[2 + r][3] * u[3];
        Av[r] = Ar[2 + r][0] * v[0] + Ar[2 + r][1] * v[1] + Ar[2 + r][2] * v[2] + Ar[2 + r][3] * v[3];
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const double b2 = Au[0] * v[j] + Av[0] * u[j], b3 = Au[1] * v[j] + Av[1] * u[j];  // adjoint of Ar[2][j], Ar[3][j]
        const int o = j < 3 ? j : 9;                                                        // R column j, or t
        g[o] -= b2;
        g[o + (j < 3 ? 3 : 1)] -= b3;
        g[o + (j < 3 ? 6 : 2)] += x2 * b2 + y2 * b3;
    }
}

template <int LOSS>
__global__ __launch_bounds__(256) void ba2view_backward_kernel(typename BaBwdArgs<LOSS>::type p) {
    __shared__ BaLmShared<true> sh;
    __shared__ double sRtBar[12], sDcBar[6];
    double* const red = sh.red;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int N = p.N;
    const float* k0 = p.k0 + (int64_t)b * N * 2;
    const float* k1 = p.k1 + (int64_t)b * N * 2;
    const float* cf = p.conf + (int64_t)b * N;
    const float* Ti = p.Tin + (int64_t)b * 16;
    const float* gT = p.gT + (int64_t)b * 16;
    double* tape = p.ws + (size_t)b * p.stride;                 // X_k at tape + k * N * 3
    double* Xbar = tape + (size_t)(p.n_it + 1) * N * 3;
    double* cbar = Xbar + (size_t)N * 3;
    double* recs = cbar + N;
    const size_t xs = (size_t)N * 3;

    // ---- phase 1: the forward loop again, with the tape
    double csum, cden, la;
    double loss_scale = 0.0;
    if constexpr (LOSS != kLossNone) loss_scale = p.loss_scale;
    const bool valid = ba2view_lm<LOSS, true>(sh, N, p.n_it, k0, k1, cf, Ti, tape, xs, recs, p.lm_inc, p.lm_dec, loss_scale, csum, cden, la);
    const int kstar = valid ? sh.kept.kstar : 0;
    double la2 = 0.0;
    [[maybe_unused]] double abar = 0.0;  // adjoint of the pair's scale: this thread's matches, all steps
    if constexpr (LOSS != kLossNone) la2 = la * la;

    // ---- phase 2: the steps k* - 1 .. 0 in reverse
    if (tid < 12) {
        const int r = tid < 9 ? tid / 3 : tid - 9, c = tid < 9 ? tid % 3 : 3;
        sRtBar[tid] = (double)gT[r * 4 + c];
    }
    for (int i = tid; i < N; i += 256) {
        Xbar[3 * i] = 0.0; Xbar[3 * i + 1] = 0.0; Xbar[3 * i + 2] = 0.0;
        cbar[i] = 0.0;
    }
    for (int k = kstar - 1; k >= 0; --k) {
        __syncthreads();
        const double* rec = recs + (size_t)k * kBaRec;
        const int flags = (int)rec[13];
        if (flags & 2) continue;  // a skipped update is the identity
        const double* X = tape + k * xs;
        const bool precond = (flags & 1) != 0;
        const double lam = rec[12];
        double Rt[12], dc[6];
#pragma unroll
        for (int i = 0; i < 12; ++i) Rt[i] = rec[i];
#pragma unroll
        for (int i = 0; i < 6; ++i) dc[i] = rec[14 + i];
        if (tid == 0) {
            double nb[12], dcb[6], tb[12];
#pragma unroll
            for (int i = 0; i < 12; ++i) nb[i] = sRtBar[i];
            se3_exp_left_reverse(dc, Rt, nb, dcb, tb);
#pragma unroll
            for (int i = 0; i < 12; ++i) sRtBar[i] = tb[i];
#pragma unroll
            for (int i = 0; i < 6; ++i) sDcBar[i] = dcb[i];
        }
        // pass A: M w = d_bar through the forward's Schur complement
        double a[27], s[27];
#pragma unroll
        for (int i = 0; i < 27; ++i) { a[i] = 0.0; s[i] = 0.0; }
        for (int i = tid; i < N; i += 256) {
            if (!(cf[i] > 0.f)) continue;
            PointTerms q;
            point_terms<LOSS>(Rt, X + 3 * i, k0[2 * i], k0[2 * i + 1], k1[2 * i], k1[2 * i + 1], (double)cf[i] / cden, la, la2, q);
            int idx = 0;
#pragma unroll
            for (int u = 0; u < 6; ++u)
#pragma unroll
                for (int v = u; v < 6; ++v) a[idx++] += q.Jc[0][u] * q.Jc[0][v] + q.Jc[1][u] * q.Jc[1][v];
            double Hpp[6], Hcp[6][3], inv[6];
            point_hpp(q, Hpp);
            point_hcp(q, Hcp);
            point_damp(Hpp, lam, precond);
            if (!inv3_sym(Hpp, inv)) continue;
            const double xb0 = Xbar[3 * i], xb1 = Xbar[3 * i + 1], xb2 = Xbar[3 * i + 2];
            idx = 0;
#pragma unroll
            for (int u = 0; u < 6; ++u) {
                double w[3];
                point_w_row(Hcp[u], inv, w);
#pragma unroll
                for (int v = u; v < 6; ++v) s[idx++] += w[0] * Hcp[v][0] + w[1] * Hcp[v][1] + w[2] * Hcp[v][2];
                s[21 + u] += w[0] * xb0 + w[1] * xb1 + w[2] * xb2;
            }
        }
        block_sum_n<27>(a, red);
        block_sum_n<27>(s, red);
        if (tid == 0) {
#pragma unroll
            for (int u = 0; u < 6; ++u) a[21 + u] = sDcBar[u];
            if (!schur6_solve(sh.M6, a, s, lam, precond, sh.delta))
                for (int u = 0; u < 6; ++u) sh.delta[u] = 0.0;
        }
        __syncthreads();
        const int dpos[6] = {0, 6, 11, 15, 18, 20};
        double wc[6], wdc[6];  // w of the camera, and 2 lambda w o d on the columns whose damping follows the diagonal
#pragma unroll
        for (int u = 0; u < 6; ++u) {
            wc[u] = sh.delta[u];
            wdc[u] = (precond && a[dpos[u]] >= 1e-12) ? 2.0 * lam * wc[u] * dc[u] : 0.0;
        }
        // pass B: the step and w per match, J_bar and r_bar, back through point_terms
        double g[12];
#pragma unroll
        for (int i = 0; i < 12; ++i) g[i] = 0.0;
        for (int i = tid; i < N; i += 256) {
            if (!(cf[i] > 0.f)) continue;
            const double c = (double)cf[i] / cden;
            PointTerms q;
            point_terms<LOSS>(Rt, X + 3 * i, k0[2 * i], k0[2 * i + 1], k1[2 * i], k1[2 * i + 1], c, la, la2, q);
            double Hpp[6], Hcp[6][3], inv[6], gd[3], gw[3], dp[3], wp[3], wdp[3];
            const double xb[3] = {Xbar[3 * i], Xbar[3 * i + 1], Xbar[3 * i + 2]};
            point_hpp(q, Hpp);
            point_gp(q, gd);
            point_hcp(q, Hcp);
#pragma unroll
            for (int u = 0; u < 3; ++u) {
                gw[u] = xb[u];
#pragma unroll
                for (int w = 0; w < 6; ++w) {
                    gd[u] -= Hcp[w][u] * dc[w];
                    gw[u] -= Hcp[w][u] * wc[w];
                }
            }
            const bool f0 = precond && Hpp[0] >= 1e-12, f1 = precond && Hpp[3] >= 1e-12, f2 = precond && Hpp[5] >= 1e-12;
            point_damp(Hpp, lam, precond);
            if (!inv3_sym(Hpp, inv)) {  // the forward left this point where it was: only its camera columns took part
#pragma unroll
                for (int u = 0; u < 6; ++u) inv[u] = 0.0;
            }
            point_solve(inv, gd, dp);
            point_solve(inv, gw, wp);
            wdp[0] = f0 ? 2.0 * lam * wp[0] * dp[0] : 0.0;
            wdp[1] = f1 ? 2.0 * lam * wp[1] * dp[1] : 0.0;
            wdp[2] = f2 ? 2.0 * lam * wp[2] * dp[2] : 0.0;
            PointTerms qb;
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                double jd0 = 0.0, jw0 = 0.0, jd1 = 0.0, jw1 = 0.0;
#pragma unroll
                for (int u = 0; u < 3; ++u) {
                    jd0 += q.Jp0[r][u] * dp[u];
                    jw0 += q.Jp0[r][u] * wp[u];
                    jd1 += q.Jp1[r][u] * dp[u];
                    jw1 += q.Jp1[r][u] * wp[u];
                }
#pragma unroll
                for (int u = 0; u < 6; ++u) {
                    jd1 += q.Jc[r][u] * dc[u];
                    jw1 += q.Jc[r][u] * wc[u];
                }
                const double e0 = jd0 + q.r0[r], e1 = jd1 + q.r1[r];
                qb.r0[r] = -jw0;
                qb.r1[r] = -jw1;
#pragma unroll
                for (int u = 0; u < 3; ++u) {
                    qb.Jp0[r][u] = -jw0 * dp[u] - e0 * wp[u] - q.Jp0[r][u] * wdp[u];
                    qb.Jp1[r][u] = -jw1 * dp[u] - e1 * wp[u] - q.Jp1[r][u] * wdp[u];
                }
#pragma unroll
                for (int u = 0; u < 6; ++u) qb.Jc[r][u] = -jw1 * dc[u] - e1 * wc[u] - q.Jc[r][u] * wdc[u];
            }
            if constexpr (LOSS != kLossNone) {  // qb is the adjoint of the corrected blocks: back through the corrector, per block
                PointTerms qr;
                point_terms<kLossNone>(Rt, X + 3 * i, k0[2 * i], k0[2 * i + 1], k1[2 * i], k1[2 * i + 1], c, 0.0, 0.0, qr);
                const double s0 = qr.r0[0] * qr.r0[0] + qr.r0[1] * qr.r0[1], s1 = qr.r1[0] * qr.r1[0] + qr.r1[1] * qr.r1[1];
                double rho0, sq0, rho1, sq1, ds0, da0, ds1, da1;
                mv_loss<LOSS>(s0, la, la2, &rho0, &sq0);
                mv_loss<LOSS>(s1, la, la2, &rho1, &sq1);
                mv_loss_sq_reverse<LOSS>(s0, sq0, la, la2, &ds0, &da0);
                mv_loss_sq_reverse<LOSS>(s1, sq1, la, la2, &ds1, &da1);
                double sb0 = 0.0, sb1 = 0.0;  // sq_bar of the two blocks
#pragma unroll
                for (int r = 0; r < 2; ++r) {
                    sb0 += qb.r0[r] * qr.r0[r];
                    sb1 += qb.r1[r] * qr.r1[r];
#pragma unroll
                    for (int u = 0; u < 3; ++u) {
                        sb0 += qb.Jp0[r][u] * qr.Jp0[r][u];
                        sb1 += qb.Jp1[r][u] * qr.Jp1[r][u];
                    }
#pragma unroll
                    for (int u = 0; u < 6; ++u) sb1 += qb.Jc[r][u] * qr.Jc[r][u];
                }
                abar += da0 * sb0 + da1 * sb1;
                const double t0 = 2.0 * ds0 * sb0, t1 = 2.0 * ds1 * sb1;
#pragma unroll
                for (int r = 0; r < 2; ++r) {
                    qb.r0[r] = sq0 * qb.r0[r] + t0 * qr.r0[r];
                    qb.r1[r] = sq1 * qb.r1[r] + t1 * qr.r1[r];
#pragma unroll
                    for (int u = 0; u < 3; ++u) { qb.Jp0[r][u] *= sq0; qb.Jp1[r][u] *= sq1; }
#pragma unroll
                    for (int u = 0; u < 6; ++u) qb.Jc[r][u] *= sq1;
                }
            }
            double Xb[3];
            cbar[i] += point_terms_reverse(Rt, X + 3 * i, k0[2 * i], k0[2 * i + 1], k1[2 * i], k1[2 * i + 1], c, qb, Xb, g);
            Xbar[3 * i] = xb[0] + Xb[0];
            Xbar[3 * i + 1] = xb[1] + Xb[1];
            Xbar[3 * i + 2] = xb[2] + Xb[2];
        }
        block_sum_n<12>(g, red);
        if (tid < 12) sRtBar[tid] += g[tid];
    }
    __syncthreads();
    double t2[2] = {0.0, 0.0};
    if (kstar > 0) {
        // the start points: X_0 = tri(Rt_0)
        double Rt[12], g[12];
#pragma unroll
        for (int i = 0; i < 12; ++i) { Rt[i] = recs[i]; g[i] = 0.0; }
        if constexpr (LOSS != kLossNone) t2[1] = abar;
        for (int i = tid; i < N; i += 256) {
            if (!(cf[i] > 0.f)) continue;
            triangulate_reverse(k0[2 * i], k0[2 * i + 1], k1[2 * i], k1[2 * i + 1], Rt, Xbar + 3 * i, g);
            t2[0] += cbar[i] * ((double)cf[i] / cden);
        }
        block_sum_n<12>(g, red);
        if (tid < 12) sRtBar[tid] += g[tid];
        block_sum_n<2>(t2, red);
    }
    __syncthreads();
    if (p.gconf) {
        // weights c_i = conf_i / cden, cden = sum conf while 2 sum conf >= 1e-6 (a constant below that)
        double shift = 2.0 * csum >= 1e-6 ? t2[0] / cden : 0.0;
        if constexpr (LOSS != kLossNone) {  // the scale a = loss_scale / cden moves with the same denominator
            if (2.0 * csum >= 1e-6) shift += t2[1] * la / cden;
        }
        for (int i = tid; i < N; i += 256)
            p.gconf[(int64_t)b * N + i] = (kstar > 0 && cf[i] > 0.f) ? (float)(cbar[i] / cden - shift) : 0.f;
    }
    if (p.gTin && tid < 16) {
        const int r = tid >> 2, c = tid & 3;
        p.gTin[(int64_t)b * 16 + tid] = r < 3 ? (float)sRtBar[c < 3 ? r * 3 + c : 9 + r] : 0.f;
    }
}

}  // namespace e2emv

// both entry points of the reverse pass; `who` names the caller in error texts
static int ba2view_backward_run(e2emv_ctx* ctx, const char* who, int B, int N, const float* d_kpts0n, const float* d_kpts1n,
                                const float* d_conf, const float* d_T_init, int n_iterations, int loss, double loss_scale, const float* d_gT,
                                float* d_gconf, float* d_gTinit, void* stream) {
    if (!ctx || !d_kpts0n || !d_kpts1n || !d_conf || !d_T_init || !d_gT) return E2EMV_EINVAL;
    E2EMV_ENTER(ctx, stream);
    int rc = mv_check_loss(ctx, who, loss, &loss_scale);
    if (rc) return rc;
    if (B <= 0 || N <= 0 || n_iterations < 0) return set_err(ctx, E2EMV_ESHAPE, "%s: B=%d N=%d iterations=%d", who, B, N, n_iterations);
    if (!d_gconf && !d_gTinit) return E2EMV_OK;
    // doubles per pair: X tape (n + 1) N 3, X_bar N 3, c_bar N, records (n + 1) kBaRec - in size_t, and an overflow is an error
    const size_t evals = (size_t)n_iterations + 1, cap = ~(size_t)0 / sizeof(double);
    const size_t per_eval = (size_t)N * 3 + kBaRec;
    if (evals > (cap - (size_t)N * 4) / per_eval)
        return set_err(ctx, E2EMV_ENOMEM, "%s: the tape of N=%d, %d iterations does not fit a size_t", who, N, n_iterations);
    const size_t stride = evals * per_eval + (size_t)N * 4;
    if ((size_t)B > (cap - 32) / stride)
        return set_err(ctx, E2EMV_ENOMEM, "%s: the tape of B=%d N=%d, %d iterations does not fit a size_t", who, B, N, n_iterations);
    rc = ws_reserve(ctx, (size_t)B * stride * sizeof(double) + 256);
    if (rc) return rc;
    BaBwdLossParams p{};
    p.B = B; p.N = N; p.n_it = n_iterations;
    p.k0 = d_kpts0n; p.k1 = d_kpts1n; p.conf = d_conf; p.Tin = d_T_init; p.gT = d_gT; p.gconf = d_gconf; p.gTin = d_gTinit;
    p.ws = (double*)ctx->d_ws; p.stride = stride;
    p.lm_inc = 1.5f; p.lm_dec = 3.5f;
    p.loss_scale = loss_scale;
    hipStream_t s = (hipStream_t)stream;
    prof_begin(ctx, PS_W8PT, s);
    if (loss == kLossHuber) hipLaunchKernelGGL(ba2view_backward_kernel<kLossHuber>, dim3(B), dim3(256), 0, s, p);
    else if (loss == kLossCauchy) hipLaunchKernelGGL(ba2view_backward_kernel<kLossCauchy>, dim3(B), dim3(256), 0, s, p);
    else hipLaunchKernelGGL(ba2view_backward_kernel<kLossNone>, dim3(B), dim3(256), 0, s, (const BaBwdParams&)p);
    prof_end(ctx, s);
    E2EMV_CHECK_LAUNCH(ctx, "ba2view_backward_kernel");
    return E2EMV_OK;
}

extern "C" int e2emv_ba_2view_backward(e2emv_ctx* ctx, int B, int N, const float* d_kpts0n, const float* d_kpts1n, const float* d_conf,
                                       const float* d_T_init, int n_iterations, const float* d_gT, float* d_gconf, float* d_gTinit,
                                       void* stream) {
    return ba2view_backward_run(ctx, "ba_2view_backward", B, N, d_kpts0n, d_kpts1n, d_conf, d_T_init, n_iterations, E2EMV_LOSS_NONE, 0.0, d_gT,
                                d_gconf, d_gTinit, stream);
}

extern "C" int e2emv_ba_2view_loss_backward(e2emv_ctx* ctx, int B, int N, const float* d_kpts0n, const float* d_kpts1n, const float* d_conf,
                                            const float* d_T_init, int n_iterations, int loss, double loss_scale, const float* d_gT,
                                            float* d_gconf, float* d_gTinit, void* stream) {
    return ba2view_backward_run(ctx, "ba_2view_loss_backward", B, N, d_kpts0n, d_kpts1n, d_conf, d_T_init, n_iterations, loss, loss_scale, d_gT,
                                d_gconf, d_gTinit, stream);
}
