// Global pose initialisation of the multi-view back-end on the DEVICE: what mv::run_init of mvinit.hip does on one host
// thread (rotation averaging by L1 steps + IRLS, least-unsquared-deviation positions by ADMM, re-basing onto camera 0),
// restated for ONE WAVE PER PROBLEM so that a batch of tuples pays the 4000 sequential ADMM iterations once.  Options and
// tolerances are copied from mvinit.hip, not re-tuned; the problem (<= 8 views, <= 28 pairs) and its whole working set live
// in LDS, all arithmetic is fp64, every reduction has a fixed order and there is no atomic: a problem's result depends on
// neither its neighbours nor its position in the batch.
//
// The ADMM iteration decides the kernel.  S = [A; G] has at most three non-zeros per row, so S x is three gathers per row
// (two rows per lane) and S^T v a walk over per-column lists (<= 7 rows, lane = column).  The one dense operation is the
// solve with the constant S^T S: the prologue factors it (wave Cholesky, lane = row), inverts it column by column (lane =
// right-hand side, the host's forward / back substitution on a unit vector) and every lane keeps ITS row of the inverse in
// registers; the solve is then one matrix-vector product against a vector broadcast from LDS instead of 2n dependent
// substitution steps.  The lane's column list sits in registers too, and the five norms of the stopping test are summed
// together on the DPP cross-lane path; the iteration count is uniform in the wave, so the early exit is a uniform branch.
//
// Two kernels share the routine: mvi_batch_kernel takes problems in the array form of the host entry point (the means to
// test the solver against it), mvi_tuple_kernel builds each tuple's problem from the relative poses of the w8pt + two-view
// BA stage (maximum spanning tree, chained start poses, pair selection: _init_arrays of multi_view.py) and solves it.
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "common.h"

namespace e2emv {

constexpr int kMviViews = E2EMV_MAX_TUPLE;
constexpr int kMviPairs = kMviViews * (kMviViews - 1) / 2;  // 28
constexpr int kMviRows = 4 * kMviPairs;                     // 3E residual rows + E scale rows
constexpr int kMviN = 3 * (kMviViews - 1) + kMviPairs;      // 49 unknowns: free positions + one scale per pair
constexpr int kMviDeg = 8;                                  // rows per column list (a view has <= 7 pairs, a scale 4 rows)
constexpr int kMviThreads = 64;

struct MviSmem {
    double L[kMviN * kMviN];  // S^T S, then its Cholesky factor (row-major, stride n)
    double X[kMviN * kMviN];  // (S^T S)^-1: column c is written and read by lane c
    double lcoef[kMviN * kMviDeg];
    double v0[kMviRows], v1[kMviRows], v2[kMviRows];
    double rwc[kMviRows];
    double y[64], x[64];
    double prot[kMviPairs * 3], ppos[kMviPairs * 3];  // pairs: angle-axis of R_ij, position of camera j in camera i
    double rot[kMviViews * 3], Rm[kMviViews * 9], res[kMviPairs * 3], w[kMviPairs], pos[kMviViews * 3], nrm[kMviViews];
    double out_R[kMviViews * 9], out_t[kMviViews * 3];
    double pose[kMviViews * 12];  // tuple kernel: chained camera-to-world [R | t], row-major 3x4
    int lrow[kMviN * kMviDeg];
    int rca[kMviRows], rcb[kMviRows], rcc[kMviRows];  // columns of a row's -1, +1 and weighted entry (-1: none)
    int pi[kMviPairs], pj[kMviPairs], lo[kMviViews], hi[kMviViews], col[kMviViews];
    int qw[kMviPairs], qorder[kMviPairs], qtree[kMviPairs], qi[kMviPairs], qj[kMviPairs], par[kMviViews], reached[kMviViews];
    int n_views, E, n_free, status;
};

// ---- rotations (column-major 3x3 <-> angle-axis): mv::aa_to_R / mv::R_to_aa of mvinit.hip -------------------------------
__device__ __forceinline__ void mvi_aa_to_R(const double* aa, double* R) {
    const double t2 = aa[0] * aa[0] + aa[1] * aa[1] + aa[2] * aa[2];
    if (t2 > 2.220446049250313e-16) {
        const double th = sqrt(t2), wx = aa[0] / th, wy = aa[1] / th, wz = aa[2] / th;
        const double c = cos(th), s = sin(th), k = 1.0 - c;
        R[0] = c + wx * wx * k;
        R[1] = wz * s + wx * wy * k;
        R[2] = -wy * s + wx * wz * k;
        R[3] = wx * wy * k - wz * s;
        R[4] = c + wy * wy * k;
        R[5] = wx * s + wy * wz * k;
        R[6] = wy * s + wx * wz * k;
        R[7] = -wx * s + wy * wz * k;
        R[8] = c + wz * wz * k;
    } else {  // first-order
        R[0] = 1; R[1] = aa[2]; R[2] = -aa[1];
        R[3] = -aa[2]; R[4] = 1; R[5] = aa[0];
        R[6] = aa[1]; R[7] = -aa[0]; R[8] = 1;
    }
}

// the branch of the quaternion extraction whose largest diagonal entry is (i, i); called with literal indices only
__device__ __forceinline__ void mvi_quat_case(const double* R, int i, int j, int k, double* q) {
    double t = sqrt(R[i * 3 + i] - R[j * 3 + j] - R[k * 3 + k] + 1.0);
    q[i + 1] = 0.5 * t;
    t = 0.5 / t;
    q[0] = (R[j * 3 + k] - R[k * 3 + j]) * t;  // M(k, j) - M(j, k), M(r, c) = R[c * 3 + r]
    q[j + 1] = (R[i * 3 + j] + R[j * 3 + i]) * t;
    q[k + 1] = (R[i * 3 + k] + R[k * 3 + i]) * t;
}

__device__ __forceinline__ void mvi_R_to_aa(const double* R, double* aa) {
    const double m00 = R[0], m10 = R[1], m20 = R[2], m01 = R[3], m11 = R[4], m21 = R[5], m02 = R[6], m12 = R[7], m22 = R[8];
    double q[4];
    const double tr = m00 + m11 + m22;
    if (tr >= 0.0) {
        double t = sqrt(tr + 1.0);
        q[0] = 0.5 * t;
        t = 0.5 / t;
        q[1] = (m21 - m12) * t;
        q[2] = (m02 - m20) * t;
        q[3] = (m10 - m01) * t;
    } else {
        int i = 0;
        if (m11 > m00) i = 1;
        if (m22 > (i == 0 ? m00 : m11)) i = 2;
        if (i == 0) mvi_quat_case(R, 0, 1, 2, q);
        else if (i == 1) mvi_quat_case(R, 1, 2, 0, q);
        else mvi_quat_case(R, 2, 0, 1, q);
    }
    const double s2 = q[1] * q[1] + q[2] * q[2] + q[3] * q[3];
    if (s2 > 0.0) {
        const double s = sqrt(s2);
        const double two_theta = 2.0 * (q[0] < 0.0 ? atan2(-s, -q[0]) : atan2(s, q[0]));
        const double k = two_theta / s;
        aa[0] = q[1] * k; aa[1] = q[2] * k; aa[2] = q[3] * k;
    } else {
        aa[0] = 2.0 * q[1]; aa[1] = 2.0 * q[2]; aa[2] = 2.0 * q[3];
    }
}

__device__ __forceinline__ void mvi_mat3_mul(const double* A, const double* B, double* C) {  // col-major C = A B
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int r = 0; r < 3; ++r) C[c * 3 + r] = A[r] * B[c * 3] + A[3 + r] * B[c * 3 + 1] + A[6 + r] * B[c * 3 + 2];
}
__device__ __forceinline__ void mvi_mat3_T(const double* A, double* B) {
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int r = 0; r < 3; ++r) B[c * 3 + r] = A[r * 3 + c];
}
__device__ __forceinline__ void mvi_load3(const double* src, double* dst) { dst[0] = src[0]; dst[1] = src[1]; dst[2] = src[2]; }
__device__ __forceinline__ void mvi_load9(const double* src, double* dst) {
#pragma unroll
    for (int i = 0; i < 9; ++i) dst[i] = src[i];
}

// Wave sums on the DPP cross-lane path (no LDS crossbar round trips): four exchanges inside each row of 16 lanes (partners add
// the same two numbers, a + b is commutative, so all 16 end with the same bits), then the four row sums read from lanes 0,
// 16, 32 and 48 and added in that order.  Every lane ends with the same bits, in an order that depends on nothing but the lane.
template <int CTRL>
__device__ __forceinline__ double mvi_dpp(double v) {
    const long long b = __builtin_bit_cast(long long, v);
    const int lo = int(b), hi = int(b >> 32);
    const unsigned l2 = unsigned(__builtin_amdgcn_update_dpp(lo, lo, CTRL, 0xF, 0xF, false));
    const unsigned h2 = unsigned(__builtin_amdgcn_update_dpp(hi, hi, CTRL, 0xF, 0xF, false));
    return __builtin_bit_cast(double, (long long)(((unsigned long long)h2 << 32) | l2));
}
__device__ __forceinline__ double mvi_readlane(double v, int lane) {
    const long long b = __builtin_bit_cast(long long, v);
    const unsigned l2 = unsigned(__builtin_amdgcn_readlane(int(b), lane)), h2 = unsigned(__builtin_amdgcn_readlane(int(b >> 32), lane));
    return __builtin_bit_cast(double, (long long)(((unsigned long long)h2 << 32) | l2));
}
template <int NV>
__device__ __forceinline__ void mvi_wsum(double (&v)[NV]) {
#pragma unroll
    for (int k = 0; k < NV; ++k) v[k] += mvi_dpp<0xB1>(v[k]);   // quad_perm [1,0,3,2]
#pragma unroll
    for (int k = 0; k < NV; ++k) v[k] += mvi_dpp<0x4E>(v[k]);   // quad_perm [2,3,0,1]
#pragma unroll
    for (int k = 0; k < NV; ++k) v[k] += mvi_dpp<0x141>(v[k]);  // row_half_mirror
#pragma unroll
    for (int k = 0; k < NV; ++k) v[k] += mvi_dpp<0x140>(v[k]);  // row_mirror
#pragma unroll
    for (int k = 0; k < NV; ++k) v[k] = (mvi_readlane(v[k], 0) + mvi_readlane(v[k], 16)) + (mvi_readlane(v[k], 32) + mvi_readlane(v[k], 48));
}

// ---- connected components and gauges ---------------------------------------------------------------------------------------
// lo[v] / hi[v]: lowest / highest view id of v's component (labels spread along the pairs; n_views sweeps cover any diameter)
__device__ __forceinline__ void mvi_components(MviSmem& s) {
    if (threadIdx.x == 0) {
        for (int v = 0; v < s.n_views; ++v) { s.lo[v] = v; s.hi[v] = v; }
        for (int sweep = 0; sweep < s.n_views; ++sweep)
            for (int e = 0; e < s.E; ++e) {
                const int i = s.pi[e], j = s.pj[e];
                const int a = min(s.lo[i], s.lo[j]), b = max(s.hi[i], s.hi[j]);
                s.lo[i] = a; s.lo[j] = a; s.hi[i] = b; s.hi[j] = b;
            }
    }
    __syncthreads();
}
// column index of every view (-1 = gauge of its component: its highest / lowest id); returns the number of free views
__device__ __forceinline__ int mvi_gauge_columns(MviSmem& s, bool highest) {
    if (threadIdx.x == 0) {
        int n_free = 0;
        for (int v = 0; v < s.n_views; ++v) s.col[v] = ((highest ? s.hi[v] : s.lo[v]) == v) ? -1 : n_free++;
        s.n_free = n_free;
    }
    __syncthreads();
    return s.n_free;
}

// ---- the sparse system S = [A; G] ------------------------------------------------------------------------------------------
// rows 3e + d (e < E): -1 at the column of view i, +1 at that of view j (gauge views have none) and, for positions, the weight
// -dir_e[d] at the scale column np + e; rows 3E + e (positions only): 1 at np + e.  Then the column lists in ascending row
// order.  Returns the longest list (uniform).
__device__ __forceinline__ int mvi_build_system(MviSmem& s, bool positions, int np, int m1, int m, int n) {
    const int lane = threadIdx.x;
    for (int r = lane; r < m; r += kMviThreads) {
        if (r < m1) {
            const int e = r / 3, d = r - 3 * e, ci = s.col[s.pi[e]], cj = s.col[s.pj[e]];
            s.rca[r] = ci >= 0 ? 3 * ci + d : -1;
            s.rcb[r] = cj >= 0 ? 3 * cj + d : -1;
            s.rcc[r] = positions ? np + e : -1;
            double wc = 0.0;
            if (positions) {  // world-frame direction of the baseline: R_i^T p_ij
                double aa[3], Ri[9];
                mvi_load3(&s.rot[3 * s.pi[e]], aa);
                mvi_aa_to_R(aa, Ri);
                const double p0 = s.ppos[3 * e], p1 = s.ppos[3 * e + 1], p2 = s.ppos[3 * e + 2];
                const double d0 = Ri[0] * p0 + Ri[1] * p1 + Ri[2] * p2, d1 = Ri[3] * p0 + Ri[4] * p1 + Ri[5] * p2,
                             d2 = Ri[6] * p0 + Ri[7] * p1 + Ri[8] * p2;
                wc = -(d == 0 ? d0 : (d == 1 ? d1 : d2));
            }
            s.rwc[r] = wc;
        } else {
            s.rca[r] = -1; s.rcb[r] = np + (r - m1); s.rcc[r] = -1; s.rwc[r] = 0.0;
        }
    }
    __syncthreads();
    int cnt = 0;
    if (lane < n) {
        for (int r = 0; r < m; ++r) {
            double c = 0.0;
            bool hit = true;
            if (s.rca[r] == lane) c = -1.0;
            else if (s.rcb[r] == lane) c = 1.0;
            else if (s.rcc[r] == lane) c = s.rwc[r];
            else hit = false;
            if (hit && cnt < kMviDeg) { s.lrow[lane * kMviDeg + cnt] = r; s.lcoef[lane * kMviDeg + cnt] = c; ++cnt; }
        }
        for (int t = cnt; t < kMviDeg; ++t) { s.lrow[lane * kMviDeg + t] = 0; s.lcoef[lane * kMviDeg + t] = 0.0; }
    }
    int deg = cnt;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) deg = max(deg, __shfl_xor(deg, o));
    __syncthreads();
    return deg;
}

// wave Cholesky of the n x n matrix in s.L (lane = row; the host's operation order); false when it is not positive definite
__device__ __forceinline__ bool mvi_cholesky(MviSmem& s, int n) {
    const int lane = threadIdx.x;
    for (int j = 0; j < n; ++j) {
        double a = 0.0;
        if (lane >= j && lane < n) {
            a = s.L[lane * n + j];
            for (int k = 0; k < j; ++k) a -= s.L[lane * n + k] * s.L[j * n + k];
        }
        const double d = __shfl(a, j);
        if (!(d > 0.0)) return false;
        const double sd = sqrt(d);
        if (lane >= j && lane < n) s.L[lane * n + j] = (lane == j) ? sd : a / sd;
        __syncthreads();
    }
    return true;
}

// S^T diag(w) S into s.L (w per PAIR, nullptr = 1; entry by entry, rows ascending like the host's normal_matrix), factored.
__device__ __forceinline__ bool mvi_normal_cholesky(MviSmem& s, int n, int deg, const double* w) {
    for (int idx = threadIdx.x; idx < n * n; idx += kMviThreads) {
        const int i = idx / n, j = idx - i * n;
        double acc = 0.0;
        for (int t = 0; t < deg; ++t) {
            const int r = s.lrow[i * kMviDeg + t];
            double ai = s.lcoef[i * kMviDeg + t];
            if (w) ai *= w[r / 3];
            const double sj = s.rca[r] == j ? -1.0 : (s.rcb[r] == j ? 1.0 : (s.rcc[r] == j ? s.rwc[r] : 0.0));
            acc += ai * sj;
        }
        s.L[idx] = acc;
    }
    __syncthreads();
    return mvi_cholesky(s, n);
}

// (S^T S)^-1 into s.X from the factor in s.L: lane c runs the host's chol_solve on the unit vector e_c, in its own column
__device__ __forceinline__ void mvi_invert(MviSmem& s, int n) {
    const int c = threadIdx.x;
    if (c < n) {
        for (int i = 0; i < n; ++i) {
            double a = (i == c) ? 1.0 : 0.0;
            for (int k = 0; k < i; ++k) a -= s.L[i * n + k] * s.X[k * n + c];
            s.X[i * n + c] = a / s.L[i * n + i];
        }
        for (int i = n - 1; i >= 0; --i) {
            double a = s.X[i * n + c];
            for (int k = i + 1; k < n; ++k) a -= s.L[k * n + i] * s.X[k * n + c];
            s.X[i * n + c] = a / s.L[i * n + i];
        }
    }
    __syncthreads();
}

// ADMM for  min |A x - b|_1  s.t. the trailing m - m1 rows >= g  (admm_l1 of mvinit.hip: rho = alpha = 1, z = S x - bs, soft
// threshold on the first m1 rows, projection on z >= 0 behind them).  The system and (S^T S)^-1 are in s; b = bsrc[0 .. m1).
// The solution is left in s.x[0 .. n).  NPAD >= n: length of the register row of the inverse.
template <int NPAD>
__device__ __forceinline__ void mvi_admm(MviSmem& s, int m1, int m, int n, int deg, int max_iterations, double abs_tol, double rel_tol,
                                         const double* bsrc, double g) {
    const double rho = 1.0, alpha = 1.0, kappa = 1.0 / rho;
    const int lane = threadIdx.x;
    double row[NPAD];
#pragma unroll
    for (int k = 0; k < NPAD; ++k) row[k] = (lane < n && k < n) ? s.X[k * n + lane] : 0.0;
    // the two rows of this lane
    const int r0 = lane, r1 = lane + kMviThreads;
    const bool in0 = r0 < m, in1 = r1 < m;
    const int a0 = in0 ? s.rca[r0] : -1, b0 = in0 ? s.rcb[r0] : -1, c0 = in0 ? s.rcc[r0] : -1;
    const int a1 = in1 ? s.rca[r1] : -1, b1 = in1 ? s.rcb[r1] : -1, c1 = in1 ? s.rcc[r1] : -1;
    const double w0 = in0 ? s.rwc[r0] : 0.0, w1 = in1 ? s.rwc[r1] : 0.0;
    const double bs0 = in0 ? (r0 < m1 ? bsrc[r0] : g) : 0.0, bs1 = in1 ? (r1 < m1 ? bsrc[r1] : g) : 0.0;
    double z0 = 0.0, z1 = 0.0, u0 = 0.0, u1 = 0.0;
    double nb[1] = {bs0 * bs0 + bs1 * bs1};
    mvi_wsum(nb);
    const double norm_bs = sqrt(nb[0]);
    const double sqrt_m = sqrt(double(m)), sqrt_n = sqrt(double(n));
    // this lane's column list (padded with weight 0 on row 0)
    int lr[kMviDeg];
    double lc[kMviDeg];
#pragma unroll
    for (int t = 0; t < kMviDeg; ++t) {
        lr[t] = lane < n ? s.lrow[lane * kMviDeg + t] : 0;
        lc[t] = lane < n ? s.lcoef[lane * kMviDeg + t] : 0.0;
    }
    // y = S^T (bs + z - u) of the first iteration
    __syncthreads();
    if (in0) s.v0[r0] = bs0;
    if (in1) s.v0[r1] = bs1;
    __syncthreads();
    double y = 0.0;
#pragma unroll
    for (int t = 0; t < kMviDeg; ++t)
        if (t < deg) y += lc[t] * s.v0[lr[t]];
    for (int it = 0; it < max_iterations; ++it) {
        s.y[lane] = y;  // lanes >= n hold 0
        __syncthreads();
        // x = (S^T S)^-1 y: the register row against the broadcast vector, four partial sums
        double acc[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int k = 0; k < NPAD; ++k) acc[k & 3] += row[k] * s.y[k];
        s.x[lane] = (acc[0] + acc[1]) + (acc[2] + acc[3]);
        __syncthreads();
        double red[5] = {0.0, 0.0, 0.0, 0.0, 0.0};  // |S x - z - bs|^2, |z|^2, |S x|^2, |S^T dz|^2, |S^T rho u|^2
        if (in0) {
            const double sx = (a0 >= 0 ? -s.x[a0] : 0.0) + (b0 >= 0 ? s.x[b0] : 0.0) + (c0 >= 0 ? w0 * s.x[c0] : 0.0);
            const double zold = z0, axh = alpha * sx + (1.0 - alpha) * (zold + bs0), v = axh - bs0 + u0;
            z0 = r0 < m1 ? (v > kappa ? v - kappa : (v < -kappa ? v + kappa : 0.0)) : (v > 0.0 ? v : 0.0);
            u0 += axh - z0 - bs0;
            const double pr = sx - z0 - bs0;
            red[0] += pr * pr; red[1] += z0 * z0; red[2] += sx * sx;
            s.v0[r0] = bs0 + z0 - u0; s.v1[r0] = -rho * (z0 - zold); s.v2[r0] = rho * u0;
        }
        if (in1) {
            const double sx = (a1 >= 0 ? -s.x[a1] : 0.0) + (b1 >= 0 ? s.x[b1] : 0.0) + (c1 >= 0 ? w1 * s.x[c1] : 0.0);
            const double zold = z1, axh = alpha * sx + (1.0 - alpha) * (zold + bs1), v = axh - bs1 + u1;
            z1 = r1 < m1 ? (v > kappa ? v - kappa : (v < -kappa ? v + kappa : 0.0)) : (v > 0.0 ? v : 0.0);
            u1 += axh - z1 - bs1;
            const double pr = sx - z1 - bs1;
            red[0] += pr * pr; red[1] += z1 * z1; red[2] += sx * sx;
            s.v0[r1] = bs1 + z1 - u1; s.v1[r1] = -rho * (z1 - zold); s.v2[r1] = rho * u1;
        }
        __syncthreads();
        // one walk over the column list: S^T of the next right-hand side, of dz and of rho u
        y = 0.0;
        double sdz = 0.0, sru = 0.0;
#pragma unroll
        for (int t = 0; t < kMviDeg; ++t)
            if (t < deg) { y += lc[t] * s.v0[lr[t]]; sdz += lc[t] * s.v1[lr[t]]; sru += lc[t] * s.v2[lr[t]]; }
        red[3] = sdz * sdz; red[4] = sru * sru;
        mvi_wsum(red);
        const double r_norm = sqrt(red[0]), s_norm = sqrt(red[3]);
        const double eps_pri = sqrt_m * abs_tol + rel_tol * fmax(fmax(sqrt(red[2]), sqrt(red[1])), norm_bs);
        const double eps_dual = sqrt_n * abs_tol + rel_tol * sqrt(red[4]);
        if (r_norm < eps_pri && s_norm < eps_dual) break;
    }
    __syncthreads();
}

__device__ __forceinline__ void mvi_admm_any(MviSmem& s, int m1, int m, int n, int deg, int max_iterations, double abs_tol, double rel_tol,
                                             const double* bsrc, double g) {
    if (n <= 24) mvi_admm<24>(s, m1, m, n, deg, max_iterations, abs_tol, rel_tol, bsrc, g);
    else mvi_admm<52>(s, m1, m, n, deg, max_iterations, abs_tol, rel_tol, bsrc, g);
}

// ---- robust rotation averaging (estimate_rotations of mvinit.hip) -------------------------------------------------------------
__device__ __forceinline__ void mvi_refresh(MviSmem& s) {
    const int v = threadIdx.x;
    if (v < s.n_views) {
        double aa[3], R[9];
        mvi_load3(&s.rot[3 * v], aa);
        mvi_aa_to_R(aa, R);
#pragma unroll
        for (int i = 0; i < 9; ++i) s.Rm[9 * v + i] = R[i];
    }
    __syncthreads();
}
__device__ __forceinline__ void mvi_residuals(MviSmem& s) {  // log(R_j^T R_ij R_i), lane = pair
    const int e = threadIdx.x;
    if (e < s.E) {
        double aa[3], Rij[9], Ri[9], Rj[9], T1[9], RjT[9], loop[9], r[3];
        mvi_load3(&s.prot[3 * e], aa);
        mvi_aa_to_R(aa, Rij);
        mvi_load9(&s.Rm[9 * s.pi[e]], Ri);
        mvi_load9(&s.Rm[9 * s.pj[e]], Rj);
        mvi_mat3_mul(Rij, Ri, T1);
        mvi_mat3_T(Rj, RjT);
        mvi_mat3_mul(RjT, T1, loop);
        mvi_R_to_aa(loop, r);
        s.res[3 * e] = r[0]; s.res[3 * e + 1] = r[1]; s.res[3 * e + 2] = r[2];
    }
    __syncthreads();
}
// R_v <- R_v exp(step_v) with the step in s.x; returns the mean step angle, summed in view order like the host
__device__ __forceinline__ double mvi_apply(MviSmem& s) {
    const int v = threadIdx.x;
    if (v < s.n_views && s.col[v] >= 0) {
        double sv[3], dR[9], Rv[9], Rn[9], aa[3];
        mvi_load3(&s.x[3 * s.col[v]], sv);
        mvi_aa_to_R(sv, dR);
        mvi_load9(&s.Rm[9 * v], Rv);
        mvi_mat3_mul(Rv, dR, Rn);
        mvi_R_to_aa(Rn, aa);
        s.rot[3 * v] = aa[0]; s.rot[3 * v + 1] = aa[1]; s.rot[3 * v + 2] = aa[2];
        s.nrm[v] = sqrt(sv[0] * sv[0] + sv[1] * sv[1] + sv[2] * sv[2]);
    }
    __syncthreads();
    double avg = 0.0;
    for (int u = 0; u < s.n_views; ++u)
        if (s.col[u] >= 0) avg += s.nrm[u];
    const double mean = avg / s.n_free;
    mvi_refresh(s);
    return mean;
}

__device__ __forceinline__ bool mvi_estimate_rotations(MviSmem& s) {
    const int max_l1_steps = 5, max_irls_steps = 100;
    const double l1_step_tol = 1e-3, irls_step_tol = 1e-3, sigma = 5.0 * M_PI / 180.0;
    const int lane = threadIdx.x;
    // gauge: the rotation of the LAST view of every connected component is held at its initial value
    const int n_free = mvi_gauge_columns(s, true);
    const int E = s.E, nu = 3 * n_free;
    if (s.n_views < 2 || E == 0 || n_free == 0) return s.n_views >= 1;
    const int deg = mvi_build_system(s, false, 0, 3 * E, 3 * E, nu);
    mvi_refresh(s);
    mvi_residuals(s);
    // stage 1: L1 steps (the factor of A^T A is the same for all of them)
    if (!mvi_normal_cholesky(s, nu, deg, nullptr)) return false;
    mvi_invert(s, nu);
    int cap = 5;
    for (int it = 0; it < max_l1_steps; ++it) {
        mvi_admm<24>(s, 3 * E, 3 * E, nu, deg, cap, 1e-4, 1e-2, s.res, 0.0);
        const double avg = mvi_apply(s);
        mvi_residuals(s);
        if (avg <= l1_step_tol) break;
        cap *= 2;
    }
    // stage 2: IRLS
    for (int it = 0; it < max_irls_steps; ++it) {
        if (lane < E) {
            const double r0 = s.res[3 * lane], r1 = s.res[3 * lane + 1], r2 = s.res[3 * lane + 2];
            const double t = (r0 * r0 + r1 * r1 + r2 * r2) + sigma * sigma;
            s.w[lane] = sigma / (t * t);
        }
        __syncthreads();
        if (!mvi_normal_cholesky(s, nu, deg, s.w)) return false;
        // step = (A^T W A)^-1 A^T W res: wave forward / back substitution, lane = row
        double b = 0.0;
        if (lane < nu)
            for (int t = 0; t < deg; ++t) {
                const int r = s.lrow[lane * kMviDeg + t];
                b += s.lcoef[lane * kMviDeg + t] * (s.w[r / 3] * s.res[r]);
            }
        for (int j = 0; j < nu; ++j) {  // L y = b
            const double yj = __shfl(b, j) / s.L[j * nu + j];
            if (lane == j) b = yj;
            else if (lane > j && lane < nu) b -= s.L[lane * nu + j] * yj;
        }
        for (int j = nu - 1; j >= 0; --j) {  // L^T x = y
            const double xj = __shfl(b, j) / s.L[j * nu + j];
            if (lane == j) b = xj;
            else if (lane < j) b -= s.L[j * nu + lane] * xj;
        }
        __syncthreads();
        s.x[lane] = b;
        __syncthreads();
        const double avg = mvi_apply(s);
        mvi_residuals(s);
        if (avg <= irls_step_tol) break;
    }
    return true;
}

// ---- least-unsquared-deviation positions (estimate_positions of mvinit.hip) -----------------------------------------------------
__device__ __forceinline__ bool mvi_estimate_positions(MviSmem& s) {
    const int lane = threadIdx.x;
    // gauge: the lowest view of every connected component sits at the origin
    const int n_free = mvi_gauge_columns(s, false);
    const int E = s.E, np = 3 * n_free, nu = np + E;
    if (lane < 3 * kMviViews) s.pos[lane] = 0.0;
    __syncthreads();
    if (s.n_views < 2 || E == 0 || n_free == 0) return s.n_views >= 1;
    const int deg = mvi_build_system(s, true, np, 3 * E, 4 * E, nu);
    if (lane < 3 * E) s.res[lane] = 0.0;  // b = 0
    if (lane + kMviThreads < 3 * E) s.res[lane + kMviThreads] = 0.0;
    __syncthreads();
    if (!mvi_normal_cholesky(s, nu, deg, nullptr)) return false;
    mvi_invert(s, nu);
    mvi_admm_any(s, 3 * E, 4 * E, nu, deg, 4000, 1e-10, 1e-10, s.res, 1.0);
    if (lane < s.n_views && s.col[lane] >= 0)
#pragma unroll
        for (int d = 0; d < 3; ++d) s.pos[3 * lane + d] = s.x[3 * s.col[lane] + d];
    __syncthreads();
    return true;
}

// run_init of mvinit.hip on the problem in s (n_views, E, pi / pj, rot = angle-axis of the initial rotations, prot, ppos):
// leaves out_R (column-major), out_t and the status bits (2: rotations failed, 4: positions failed) in s
__device__ __forceinline__ void mvi_solve(MviSmem& s) {
    const int lane = threadIdx.x;
    __syncthreads();
    mvi_components(s);
    int status = 0;
    if (!mvi_estimate_rotations(s)) status |= 2;
    __syncthreads();
    if (!mvi_estimate_positions(s)) status |= 4;
    __syncthreads();
    // t = -R * position, then the world frame is re-based onto camera 0 for the views of camera 0's component
    if (lane < s.n_views) {
        const double I3[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
        double aa[3], R0[9], R0T[9], R[9], out[9];
        mvi_load3(&s.rot[0], aa);
        mvi_aa_to_R(aa, R0);
        mvi_mat3_T(R0, R0T);
        mvi_load3(&s.rot[3 * lane], aa);
        mvi_aa_to_R(aa, R);
        const double p0 = s.pos[3 * lane], p1 = s.pos[3 * lane + 1], p2 = s.pos[3 * lane + 2];
#pragma unroll
        for (int r = 0; r < 3; ++r) s.out_t[3 * lane + r] = -(R[r] * p0 + R[3 + r] * p1 + R[6 + r] * p2);
        const bool with0 = s.lo[lane] == s.lo[0];
#pragma unroll
        for (int i = 0; i < 9; ++i) R0T[i] = with0 ? R0T[i] : I3[i];
        mvi_mat3_mul(R, R0T, out);
#pragma unroll
        for (int i = 0; i < 9; ++i) s.out_R[9 * lane + i] = out[i];
    }
    if (lane == 0) s.status = status;
    __syncthreads();
}

// ---- kernel 1: problems in the array form of the host entry point ------------------------------------------------------------
struct MviBatchArgs {
    const int* n_views;     // [n]
    const int* view_off;    // [n + 1]
    const int64_t* pair_off;  // [n + 1]
    const int* pair_ids;    // [totE, 2]
    const double *init_R, *pair_R, *pair_pos;  // [totV, 9], [totE, 9], [totE, 3]
    double *out_R, *out_t;  // [totV, 9], [totV, 3]
    int* status;            // [n]
};

__global__ __launch_bounds__(kMviThreads) void mvi_batch_kernel(MviBatchArgs a) {
    __shared__ MviSmem s;
    const int k = blockIdx.x, lane = threadIdx.x;
    const int nv = a.n_views[k], v0 = a.view_off[k];
    const int64_t e0 = a.pair_off[k];
    const int E = int(a.pair_off[k + 1] - e0);
    if (lane == 0) { s.n_views = nv; s.E = E; }
    if (lane < nv) {
        double R[9], aa[3];
        mvi_load9(a.init_R + 9 * size_t(v0 + lane), R);
        mvi_R_to_aa(R, aa);
        s.rot[3 * lane] = aa[0]; s.rot[3 * lane + 1] = aa[1]; s.rot[3 * lane + 2] = aa[2];
    }
    if (lane < E) {
        double R[9], aa[3];
        mvi_load9(a.pair_R + 9 * size_t(e0 + lane), R);
        mvi_R_to_aa(R, aa);
        s.prot[3 * lane] = aa[0]; s.prot[3 * lane + 1] = aa[1]; s.prot[3 * lane + 2] = aa[2];
        s.pi[lane] = a.pair_ids[2 * size_t(e0 + lane)];
        s.pj[lane] = a.pair_ids[2 * size_t(e0 + lane) + 1];
#pragma unroll
        for (int d = 0; d < 3; ++d) s.ppos[3 * lane + d] = a.pair_pos[3 * size_t(e0 + lane) + d];
    }
    mvi_solve(s);
    if (lane < nv) {
#pragma unroll
        for (int i = 0; i < 9; ++i) a.out_R[9 * size_t(v0 + lane) + i] = s.out_R[9 * lane + i];
#pragma unroll
        for (int d = 0; d < 3; ++d) a.out_t[3 * size_t(v0 + lane) + d] = s.out_t[3 * lane + d];
    }
    if (lane == 0) a.status[k] = s.status;
}

// ---- kernel 2: the initialisation stage of the batched path, from the relative poses on the device -----------------------------
struct MviTupleArgs {
    int T, P, min_matches, min_inliers;
    const float* rel_T;    // [B*P, 16] row-major 4x4, pair order of the collect stage (second index outer)
    const int* n_inliers;  // [B*P]
    const int* count;      // [B*P]
    double* extr;          // [B, T, 16] row-major world -> camera
    int* status;           // [B]
};

// [R | t] of a relative pose, fp32 widened; its rotation block is orthonormal only to fp32, so every inverse below is a real
// matrix inverse (adjugate / determinant of the 3x3 block and -R^-1 t), never the transpose
__device__ __forceinline__ void mvi_load_rel(const float* T, double* R /* row-major 3x3 */, double* t) {
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c) R[3 * r + c] = double(T[4 * r + c]);
        t[r] = double(T[4 * r + 3]);
    }
}
__device__ __forceinline__ void mvi_inv_rt(const double* R, const double* t, double* Ri, double* ti) {
    const double c00 = R[4] * R[8] - R[5] * R[7], c01 = R[5] * R[6] - R[3] * R[8], c02 = R[3] * R[7] - R[4] * R[6];
    const double id = 1.0 / (R[0] * c00 + R[1] * c01 + R[2] * c02);
    Ri[0] = c00 * id; Ri[1] = (R[2] * R[7] - R[1] * R[8]) * id; Ri[2] = (R[1] * R[5] - R[2] * R[4]) * id;
    Ri[3] = c01 * id; Ri[4] = (R[0] * R[8] - R[2] * R[6]) * id; Ri[5] = (R[2] * R[3] - R[0] * R[5]) * id;
    Ri[6] = c02 * id; Ri[7] = (R[1] * R[6] - R[0] * R[7]) * id; Ri[8] = (R[0] * R[4] - R[1] * R[3]) * id;
#pragma unroll
    for (int r = 0; r < 3; ++r) ti[r] = -(Ri[3 * r] * t[0] + Ri[3 * r + 1] * t[1] + Ri[3 * r + 2] * t[2]);
}
// s.pose[dst] = s.pose[src] * [R | t]
__device__ __forceinline__ void mvi_chain(MviSmem& s, int dst, int src, const double* R, const double* t) {
    double A[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) A[i] = s.pose[12 * src + i];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c) s.pose[12 * dst + 4 * r + c] = A[4 * r] * R[c] + A[4 * r + 1] * R[3 + c] + A[4 * r + 2] * R[6 + c];
        s.pose[12 * dst + 4 * r + 3] = A[4 * r] * t[0] + A[4 * r + 1] * t[1] + A[4 * r + 2] * t[2] + A[4 * r + 3];
    }
}

// One wave per tuple: _init_arrays + _averaged_extrinsics of multi_view.py.  Pairs with count >= min_matches are the edges of
// the match graph, weighted by their count; the start poses are chained from image 0 along its maximum spanning tree (Kruskal
// in descending weight, equal weights in ascending row-major (i, j) - a documented rule of this kernel, scipy's order among
// equal weights is not defined); the solver gets the pairs with n_inliers >= min_inliers or on the tree.
__global__ __launch_bounds__(kMviThreads) void mvi_tuple_kernel(MviTupleArgs a) {
    __shared__ MviSmem s;
    const int b = blockIdx.x, lane = threadIdx.x, T = a.T, P = a.P;
    const float* rel = a.rel_T + size_t(b) * P * 16;
    int qi = 0, qj = 1, wq = 0;
    if (lane < P) {
        int base = 0;
        while (lane >= base + qj) { base += qj; ++qj; }
        qi = lane - base;
        const int cnt = a.count[b * P + lane];
        wq = cnt >= a.min_matches ? cnt : 0;
        s.qw[lane] = wq; s.qi[lane] = qi; s.qj[lane] = qj; s.qtree[lane] = 0;
    }
    if (lane < T) { s.par[lane] = lane; s.reached[lane] = lane == 0; }
    if (lane < 12) s.pose[lane] = (lane == 0 || lane == 5 || lane == 10) ? 1.0 : 0.0;
    __syncthreads();
    // edges in descending weight, ties in ascending row-major (i, j)
    const bool edge = lane < P && wq > 0;
    if (edge) {
        int rank = 0;
        for (int q = 0; q < P; ++q) {
            const int w2 = s.qw[q];
            if (w2 > wq || (w2 == wq && w2 > 0 && s.qi[q] * T + s.qj[q] < qi * T + qj)) ++rank;
        }
        s.qorder[rank] = lane;
    }
    const int n_edges = __popcll(__ballot(edge));
    __syncthreads();
    if (lane == 0) {
        for (int r = 0; r < n_edges; ++r) {  // Kruskal
            const int q = s.qorder[r];
            int ra = s.qi[q], rb = s.qj[q];
            while (s.par[ra] != ra) ra = s.par[ra];
            while (s.par[rb] != rb) rb = s.par[rb];
            if (ra != rb) { s.par[ra] = rb; s.qtree[q] = 1; }
        }
        // camera-to-world poses outwards from image 0: pose_b = pose_a inv(T_ab), pose_a = pose_b T_ab
        for (int sweep = 1; sweep < T; ++sweep)
            for (int q = 0; q < P; ++q) {
                if (!s.qtree[q]) continue;
                const int i = s.qi[q], j = s.qj[q];
                if (s.reached[i] == s.reached[j]) continue;
                double R[9], t[3];
                mvi_load_rel(rel + 16 * q, R, t);
                if (s.reached[i]) {
                    double Ri[9], ti[3];
                    mvi_inv_rt(R, t, Ri, ti);
                    mvi_chain(s, j, i, Ri, ti);
                    s.reached[j] = 1;
                } else {
                    mvi_chain(s, i, j, R, t);
                    s.reached[i] = 1;
                }
            }
    }
    __syncthreads();
    // initial rotations: the rotation block of the inverse of each chained pose; images not reached from image 0: the identity
    if (lane < T) {
        double Rc[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};  // column-major
        if (s.reached[lane]) {
            double R[9], t[3], Ri[9], ti[3];
#pragma unroll
            for (int r = 0; r < 3; ++r) {
#pragma unroll
                for (int c = 0; c < 3; ++c) R[3 * r + c] = s.pose[12 * lane + 4 * r + c];
                t[r] = s.pose[12 * lane + 4 * r + 3];
            }
            mvi_inv_rt(R, t, Ri, ti);
            mvi_mat3_T(Ri, Rc);  // row-major -> column-major
        }
        double aa[3];
        mvi_R_to_aa(Rc, aa);
        s.rot[3 * lane] = aa[0]; s.rot[3 * lane + 1] = aa[1]; s.rot[3 * lane + 2] = aa[2];
    }
    // the pair list, in pair order
    const bool keep = edge && (a.n_inliers[b * P + lane] >= a.min_inliers || s.qtree[lane]);
    const unsigned long long mask = __ballot(keep);
    if (keep) {
        const int e = __popcll(mask & ((1ull << lane) - 1ull));
        double R[9], t[3], Rc[9], aa[3];
        mvi_load_rel(rel + 16 * lane, R, t);
        mvi_mat3_T(R, Rc);
        mvi_R_to_aa(Rc, aa);
        s.prot[3 * e] = aa[0]; s.prot[3 * e + 1] = aa[1]; s.prot[3 * e + 2] = aa[2];
        s.pi[e] = qi; s.pj[e] = qj;
#pragma unroll
        for (int r = 0; r < 3; ++r) s.ppos[3 * e + r] = (-R[r]) * t[0] + (-R[3 + r]) * t[1] + (-R[6 + r]) * t[2];  // -R^T t
    }
    if (lane == 0) { s.n_views = T; s.E = __popcll(mask); }
    mvi_solve(s);
    if (lane < T) {
        double* E = a.extr + (size_t(b) * T + lane) * 16;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
#pragma unroll
            for (int c = 0; c < 3; ++c) E[4 * r + c] = s.out_R[9 * lane + 3 * c + r];
            E[4 * r + 3] = s.out_t[3 * lane + r];
        }
        E[12] = 0.0; E[13] = 0.0; E[14] = 0.0; E[15] = 1.0;
    }
    if (lane == 0) a.status[b] = s.status;
}

}  // namespace e2emv

using namespace e2emv;

extern "C" int e2emv_mv_init_batch(e2emv_ctx* ctx, int n_problems, const int32_t* n_views, const double* init_R, const int64_t* pair_off,
                                   const int32_t* pair_ids, const double* pair_R, const double* pair_pos, double* out_R, double* out_t,
                                   int32_t* status, void* stream) {
    if (!ctx) return E2EMV_EINVAL;
    E2EMV_ENTER(ctx, stream);
    if (n_problems < 1 || !n_views || !init_R || !pair_off || !out_R || !out_t)
        return set_err(ctx, E2EMV_EINVAL, "mv_init_batch: bad argument (n_problems >= 1, no NULL size / offset / rotation array)");
    const size_t n = size_t(n_problems);
    if (pair_off[0] != 0) return set_err(ctx, E2EMV_EINVAL, "mv_init_batch: offsets must start at 0");
    std::vector<int> view_off(n + 1, 0);
    for (size_t k = 0; k < n; ++k) {
        if (n_views[k] < 1 || n_views[k] > kMviViews)
            return set_err(ctx, E2EMV_EINVAL, "mv_init_batch: problem %zu has %d views (1 <= n_views <= %d)", k, n_views[k], kMviViews);
        if (pair_off[k + 1] < pair_off[k] || pair_off[k + 1] - pair_off[k] > kMviPairs)
            return set_err(ctx, E2EMV_EINVAL, "mv_init_batch: offsets of problem %zu decrease or give it more than %d pairs", k, kMviPairs);
        view_off[k + 1] = view_off[k] + n_views[k];
    }
    const size_t totV = size_t(view_off[n]), totE = size_t(pair_off[n]);
    if (totE && (!pair_ids || !pair_R || !pair_pos)) return set_err(ctx, E2EMV_EINVAL, "mv_init_batch: NULL pair array for %zu pairs", totE);
    for (size_t k = 0; k < n; ++k) {
        bool seen[kMviViews][kMviViews] = {};
        for (int64_t e = pair_off[k]; e < pair_off[k + 1]; ++e) {
            const int i = pair_ids[2 * e], j = pair_ids[2 * e + 1];
            if (i < 0 || j < 0 || i >= n_views[k] || j >= n_views[k] || i == j)
                return set_err(ctx, E2EMV_EINVAL, "mv_init_batch: pair %lld of problem %zu joins views %d and %d", (long long)(e - pair_off[k]), k, i, j);
            if (seen[i][j]) return set_err(ctx, E2EMV_EINVAL, "mv_init_batch: problem %zu lists the views %d and %d twice", k, i, j);
            seen[i][j] = seen[j][i] = true;
        }
    }
    hipStream_t s = (hipStream_t)stream;
    // one staging block: sizes, offsets, ids, then the fp64 inputs; the outputs follow it in the workspace
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t at = off; off += (bytes + 255) & ~size_t(255); return at; };
    const size_t o_nv = take(n * 4), o_vo = take((n + 1) * 4), o_po = take((n + 1) * 8), o_ids = take(totE * 8), o_iR = take(totV * 72),
                 o_pR = take(totE * 72), o_pp = take(totE * 24), upload = off, o_oR = take(totV * 72), o_ot = take(totV * 24), o_st = take(n * 4);
    const int rc = ws_reserve(ctx, off);
    if (rc) return rc;
    std::vector<char> stage(upload, 0);
    std::memcpy(stage.data() + o_nv, n_views, n * 4);
    std::memcpy(stage.data() + o_vo, view_off.data(), (n + 1) * 4);
    std::memcpy(stage.data() + o_po, pair_off, (n + 1) * 8);
    std::memcpy(stage.data() + o_iR, init_R, totV * 72);
    if (totE) {
        std::memcpy(stage.data() + o_ids, pair_ids, totE * 8);
        std::memcpy(stage.data() + o_pR, pair_R, totE * 72);
        std::memcpy(stage.data() + o_pp, pair_pos, totE * 24);
    }
    E2EMV_HIP(ctx, hipMemcpyAsync(ctx->d_ws, stage.data(), upload, hipMemcpyHostToDevice, s));
    char* w = ctx->d_ws;
    MviBatchArgs a{};
    a.n_views = reinterpret_cast<const int*>(w + o_nv); a.view_off = reinterpret_cast<const int*>(w + o_vo);
    a.pair_off = reinterpret_cast<const int64_t*>(w + o_po); a.pair_ids = reinterpret_cast<const int*>(w + o_ids);
    a.init_R = reinterpret_cast<const double*>(w + o_iR); a.pair_R = reinterpret_cast<const double*>(w + o_pR);
    a.pair_pos = reinterpret_cast<const double*>(w + o_pp);
    a.out_R = reinterpret_cast<double*>(w + o_oR); a.out_t = reinterpret_cast<double*>(w + o_ot); a.status = reinterpret_cast<int*>(w + o_st);
    prof_begin(ctx, PS_W8PT, s);
    hipLaunchKernelGGL(mvi_batch_kernel, dim3(n_problems), dim3(kMviThreads), 0, s, a);
    E2EMV_CHECK_LAUNCH(ctx, "mvi_batch_kernel");
    prof_end(ctx, s);
    std::vector<int32_t> st(n);
    E2EMV_HIP(ctx, hipMemcpyAsync(out_R, a.out_R, totV * 72, hipMemcpyDeviceToHost, s));
    E2EMV_HIP(ctx, hipMemcpyAsync(out_t, a.out_t, totV * 24, hipMemcpyDeviceToHost, s));
    E2EMV_HIP(ctx, hipMemcpyAsync(st.data(), a.status, n * 4, hipMemcpyDeviceToHost, s));
    E2EMV_HIP(ctx, hipStreamSynchronize(s));  // the staging block and st die at return
    if (status) std::memcpy(status, st.data(), n * 4);
    return E2EMV_OK;
}

extern "C" int e2emv_mv_tuple_init(e2emv_ctx* ctx, int B, int T, const float* d_rel_T, const int32_t* d_n_inliers, const int32_t* d_count,
                                   int min_matches, int min_inliers, double* d_extr, int32_t* d_status, void* stream) {
    if (!ctx) return E2EMV_EINVAL;
    E2EMV_ENTER(ctx, stream);
    if (B < 1 || !d_rel_T || !d_n_inliers || !d_count || !d_extr || !d_status)
        return set_err(ctx, E2EMV_EINVAL, "mv_tuple_init: bad argument (B >= 1, no NULL array)");
    if (T < 2 || T > kMviViews) return set_err(ctx, E2EMV_EINVAL, "mv_tuple_init: tuple of %d images (2 <= T <= %d)", T, kMviViews);
    if (min_matches < 1) return set_err(ctx, E2EMV_EINVAL, "mv_tuple_init: min_matches = %d (>= 1: a pair without matches is no edge)", min_matches);
    MviTupleArgs a{};
    a.T = T; a.P = T * (T - 1) / 2; a.min_matches = min_matches; a.min_inliers = min_inliers;
    a.rel_T = d_rel_T; a.n_inliers = d_n_inliers; a.count = d_count; a.extr = d_extr; a.status = d_status;
    hipStream_t s = (hipStream_t)stream;
    prof_begin(ctx, PS_W8PT, s);
    hipLaunchKernelGGL(mvi_tuple_kernel, dim3(B), dim3(kMviThreads), 0, s, a);
    E2EMV_CHECK_LAUNCH(ctx, "mvi_tuple_kernel");
    prof_end(ctx, s);
    return E2EMV_OK;
}
