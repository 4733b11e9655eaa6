// Backward pass of the multi-view bundle adjustment (mvba_kernel<kLossNone>, mvba.h): from dLoss/d(cams_out, pts_out) to
// dLoss/d(obs_w), dLoss/d(cams_start), dLoss/d(pts_start).  DESIGN 1, "Backward pass of the multi-view stage".
//
// The gradient is the exact adjoint of the loop the device runs with its decisions frozen - not implicit differentiation of a
// converged minimiser.  One workgroup per problem, fp64, no atomics, the forward's reduction orders.
//
// REPLAY.  mvba_kernel<kLossNone, kLmTape> is the solver itself (one statement, mvba.h) that also records, per pass, the radius it used
// and whether the step was solved and accepted, and per accepted step the iterate it started from.  When the run has ended the same
// kernel walks the accepted steps backwards: this file holds what it calls there (mv_reverse_begin, mv_reverse_next, mv_reverse_step),
// the only instantiation of that kernel (mv_launch_ba_backward), the reverse pass' share of the workspace and the C entry of the solver
// level.  The tuple level (e2emv_mv_tuple_ba_backward, e2emv_mv_collect_backward) sits with the tuple build in mvba.hip, that of the
// track route (e2emv_mv_tuple_ba_tracks_backward) with the track build in mvtracks.hip; their dLoss/d(extrinsics) enters here, in
// mv_reverse_begin, at the cameras the run ended with.
//
// REVERSE.  The accepted steps are walked from last to first with the adjoint state cams_bar (LDS) and pts_bar (workspace).  An
// accepted step is x+ = x + d,  d = -M^-1 g,  M = J^T J + Lambda,  g = J^T r,  Lambda_ii = clamp(diag(J^T J)_ii s_i^2) / radius / s_i^2:
//   1  phases A - G of the loop recompute r, Jc, Jp, U, V, Y, Vinv, the factor of the reduced system and d at the taped iterate
//   2  M w = x+_bar: the forward's Schur complement, Cholesky factor (phase F) and back-substitution (phase G), another right side
//   3  per observation  J_bar = -(J w) d^T - (J d + r) w^T - 2 J diag(w o d) / radius  (last term on unclamped columns only),
//      r_bar = -J w
//   4  (J_bar, r_bar) back through phase A, r = w (.) (pi(R(omega) X + t) - obs) and its analytic Jacobians: with u_k the unweighted
//      residual of row k and v_k = (Jc_bar, Jp_bar)[k], theta = (camera, point),
//          theta_bar = sum_k w_k (r_bar_k grad u_k + H_k v_k),     w_k_bar = r_bar_k u_k + v_k . grad u_k
//      H_k v_k, the second derivatives of mv_transform, is the tangent of the analytic gradient evaluated on fp64 numbers that carry
//      one tangent (MvDual): the branch taken (Rodrigues for theta^2 > eps, first order below) is the forward's, decided on the value
//   5  point adjoints summed in the order of the point lists, camera adjoints in the order of the camera lists (lane-strided, then
//      the wave sum of phase C); the weight adjoints accumulate over the steps
//
// WHAT CARRIES NO GRADIENT (frozen, as in the torch restatement tests/mvba_backward_restatement.py):
//   - the radius, including its rho-dependent update radius / max(1/3, 1 - (2 rho - 1)^3)
//   - the Jacobi scales of the first iterate (s_scale, scale_p)
//   - the accept and reject comparisons and all termination tests
//   - obs_xy and the intrinsics
// A column whose damping sits on a clamp (1e-6 or 1e32) has a constant lambda and drops the 2 / radius term.  An unsolved step
// (Cholesky failed) and a rejected step are the identity.  The fixed camera's row passes through (its observations are predicted
// with the identity pose and give that row nothing), and so does the row of a camera without observations.  A problem that stopped
// before any accepted step returns g_obs_w = 0, g_cams0 = g_cams, g_pts0 = g_pts.
#include <cstdint>
#include <vector>

#include "common.h"
#include "mvba.h"

namespace e2emv {

// gradient of the unweighted residual row k (k = 0: x, 1: y) with respect to (camera 6, point 3) and the row's prediction
template <typename T>
__host__ __device__ __forceinline__ void mv_row_gradient(const T* cam, bool fixed, const T X[3], double fx, double fy, double cx, double cy, int k,
                                                         T g[9], T* pred) {
    T q[3], R[9], D[9];
    mv_transform<T>(cam, fixed, X, q, R, D, true);
    const T iz = 1.0 / q[2];
    const double f = k ? fy : fx;
    const T e = f * iz, e2 = -(f * q[k] * iz * iz);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        g[i] = e * D[3 * k + i] + e2 * D[6 + i];
        g[6 + i] = e * R[3 * k + i] + e2 * R[6 + i];
    }
    g[3] = k ? T(0) : e; g[4] = k ? e : T(0); g[5] = e2;
    if (fixed)
#pragma unroll
        for (int i = 0; i < 6; ++i) g[i] = T(0);
    *pred = f * q[k] * iz + (k ? cy : cx);
}

// step 4 for one observation: rbar [2], Jbar [2][9] (camera 6, point 3) -> theta_bar [9], wbar [2]
__host__ __device__ __forceinline__ void mv_obs_reverse(const double* cam, bool fixed, const double X[3], double fx, double fy, double cx, double cy,
                                                        const double obs[2], const double w[2], const double rbar[2], const double Jbar[18],
                                                        double theta_bar[9], double wbar[2]) {
#pragma unroll
    for (int i = 0; i < 9; ++i) theta_bar[i] = 0.0;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const double* v = Jbar + 9 * k;
        MvDual camd[6], Xd[3], g[9], pred;
#pragma unroll
        for (int i = 0; i < 6; ++i) camd[i] = MvDual(cam[i], fixed ? 0.0 : v[i]);
#pragma unroll
        for (int i = 0; i < 3; ++i) Xd[i] = MvDual(X[i], v[6 + i]);
        mv_row_gradient<MvDual>(camd, fixed, Xd, fx, fy, cx, cy, k, g, &pred);
        double dot = 0.0;
#pragma unroll
        for (int i = 0; i < 9; ++i) {
            dot += v[i] * g[i].v;
            theta_bar[i] += w[k] * (rbar[k] * g[i].v + g[i].d);
        }
        wbar[k] = rbar[k] * (pred.v - obs[k]) + dot;
    }
}

// dLoss/d(extrinsics of the final cameras) -> cams_bar, thread = camera: E = [R(w) | t] (mv_cam_to_extr), dR/dw_i column by column as
// the tangent of mv_transform on the unit vectors (the rotation matrix the solver itself uses, in the branch the value takes)
__device__ __forceinline__ void mv_reverse_begin(const MvbaArgs& a, const MvbaBwdArgs& b, const double* s_cams, double* s_cbar) {
    const int c = threadIdx.x;
    if (!b.g_extr || c >= a.C) return;
    const double* g = b.g_extr + 16 * c;
    for (int i = 0; i < 3; ++i) {
        MvDual cam[6];
#pragma unroll
        for (int k = 0; k < 3; ++k) cam[k] = MvDual(s_cams[6 * c + k], k == i ? 1.0 : 0.0);
        double acc = 0.0;
        for (int j = 0; j < 3; ++j) {
            const MvDual X[3] = {MvDual(j == 0 ? 1.0 : 0.0), MvDual(j == 1 ? 1.0 : 0.0), MvDual(j == 2 ? 1.0 : 0.0)};
            MvDual p[3];
            mv_transform<MvDual>(cam, false, X, p, nullptr, nullptr, false);
            acc += g[j] * p[0].d + g[4 + j] * p[1].d + g[8 + j] * p[2].d;
        }
        s_cbar[6 * c + i] += acc;
        s_cbar[6 * c + 3 + i] += g[4 * i + 3];
    }
}

__device__ __forceinline__ bool mv_reverse_next(const MvbaArgs& a, const MvbaBwdArgs& b, double* s_cams, double* s_ctl, int& k, int& j) {
    const int tid = threadIdx.x;
    do --k; while (k >= 0 && b.tape.it[3 * size_t(k) + 2] == 0.0);  // rejected, unsolved or a stop: the identity
    if (k < 0 || j <= 0) return false;
    --j;
    const double* x = b.tape.x + size_t(j) * (6 * size_t(a.C) + 3 * size_t(a.P));
    __syncthreads();
    if (tid < 6 * a.C) s_cams[tid] = x[tid];
    for (int i = tid; i < 3 * a.P; i += kMvThreads) a.pts[i] = x[6 * a.C + i];
    if (tid == 0) s_ctl[0] = b.tape.it[3 * size_t(k)];
    __syncthreads();
    return true;
}

// steps 2 - 5 for the accepted step whose phases A - G the loop has just run again (step 1): r, Jc, Jp, Y, Vinv, gp, dp in the
// workspace, U, the scales, the Cholesky factor and dc in LDS
__device__ __forceinline__ void mv_reverse_step(const MvbaArgs& a, const MvbaBwdArgs& b, const MvRevLds& L, double radius, int F, int n) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int P = a.P, O = a.O;
    double* const s_cbar = L.cbar; double* const s_wc = L.wc; double* const s_fac = L.fac;
    {
        // ---- 2: M w = x+_bar ----------------------------------------------------------------------------------------------------
        if (tid < n) {
            const double d = L.U[36 * (tid / 6) + 7 * (tid % 6)], sc = L.scale[tid], v = d * sc * sc;
            s_fac[tid] = (v >= 1e-6 && v <= 1e32) ? 2.0 / radius : 0.0;
        }
        for (int f = wave; f < F; f += kMvWaves) {
            const int c = L.free_[f];
            double rh[6] = {0, 0, 0, 0, 0, 0};
            for (int q = a.cam_start[c] + lane; q < a.cam_start[c + 1]; q += 64) {
                const int o = a.cam_obs[q], p = a.pt_idx[o];
                const double* y = a.Y + 18 * size_t(o);
                const double g0 = b.pts_bar[3 * p], g1 = b.pts_bar[3 * p + 1], g2 = b.pts_bar[3 * p + 2];
#pragma unroll
                for (int i = 0; i < 6; ++i) rh[i] += y[3 * i] * g0 + y[3 * i + 1] * g1 + y[3 * i + 2] * g2;
            }
#pragma unroll
            for (int i = 0; i < 6; ++i) rh[i] = wave_sum_d(rh[i]);
            if (lane == 0)
#pragma unroll
                for (int i = 0; i < 6; ++i) L.rhs[6 * f + i] = s_cbar[6 * c + i] - rh[i];
        }
        __syncthreads();
        if (wave == 0) mv_chol_solve(L.S, n, L.rhs, s_wc);
        __syncthreads();
        for (int p = tid; p < P; p += kMvThreads) {
            double g0 = b.pts_bar[3 * p], g1 = b.pts_bar[3 * p + 1], g2 = b.pts_bar[3 * p + 2];
            double d[3] = {0, 0, 0};
            for (int q = a.pt_start[p]; q < a.pt_start[p + 1]; ++q) {
                const int o = a.pt_obs[q], f = L.fidx[a.cam_idx[o]];
                const double* jp = a.Jp + 6 * size_t(o);
                d[0] += jp[0] * jp[0] + jp[3] * jp[3];
                d[1] += jp[1] * jp[1] + jp[4] * jp[4];
                d[2] += jp[2] * jp[2] + jp[5] * jp[5];
                if (f < 0) continue;
                const double* jc = a.Jc + 12 * size_t(o);
                double q0 = 0, q1 = 0;
#pragma unroll
                for (int i = 0; i < 6; ++i) { q0 += jc[i] * s_wc[6 * f + i]; q1 += jc[6 + i] * s_wc[6 * f + i]; }
                g0 -= jp[0] * q0 + jp[3] * q1;
                g1 -= jp[1] * q0 + jp[4] * q1;
                g2 -= jp[2] * q0 + jp[5] * q1;
            }
            const double* vi = a.Vinv + 6 * size_t(p);
            b.wp[3 * p] = vi[0] * g0 + vi[1] * g1 + vi[3] * g2;
            b.wp[3 * p + 1] = vi[1] * g0 + vi[2] * g1 + vi[4] * g2;
            b.wp[3 * p + 2] = vi[3] * g0 + vi[4] * g1 + vi[5] * g2;
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const double sc = a.scale_p[3 * p + i], v = d[i] * sc * sc;
                b.fac_p[3 * p + i] = (v >= 1e-6 && v <= 1e32) ? 2.0 / radius : 0.0;
            }
        }
        __syncthreads();
        // ---- 3, 4: per observation; its nine adjoints go where its Y was (no longer needed) --------------------------------------
        for (int o = tid; o < O; o += kMvThreads) {
            const int c = a.cam_idx[o], p = a.pt_idx[o], f = L.fidx[c];
            const bool fixed = (c == a.fixed);
            const double* jc = a.Jc + 12 * size_t(o);
            const double* jp = a.Jp + 6 * size_t(o);
            double dl[9], w[9], fac[9];
#pragma unroll
            for (int i = 0; i < 6; ++i) {
                dl[i] = f >= 0 ? L.dc[6 * f + i] : 0.0;
                w[i] = f >= 0 ? s_wc[6 * f + i] : 0.0;
                fac[i] = f >= 0 ? s_fac[6 * f + i] : 0.0;
            }
#pragma unroll
            for (int i = 0; i < 3; ++i) { dl[6 + i] = a.dp[3 * p + i]; w[6 + i] = b.wp[3 * p + i]; fac[6 + i] = b.fac_p[3 * p + i]; }
            double rbar[2], Jbar[18];
#pragma unroll
            for (int k2 = 0; k2 < 2; ++k2) {
                double J[9];
#pragma unroll
                for (int i = 0; i < 6; ++i) J[i] = jc[6 * k2 + i];
#pragma unroll
                for (int i = 0; i < 3; ++i) J[6 + i] = jp[3 * k2 + i];
                double jw = 0.0, m = a.r[2 * o + k2];
#pragma unroll
                for (int i = 0; i < 9; ++i) { jw += J[i] * w[i]; m += J[i] * dl[i]; }
                rbar[k2] = -jw;
#pragma unroll
                for (int i = 0; i < 9; ++i) Jbar[9 * k2 + i] = -jw * dl[i] - m * w[i] - J[i] * (w[i] * dl[i]) * fac[i];
            }
            const double X[3] = {a.pts[3 * p], a.pts[3 * p + 1], a.pts[3 * p + 2]};
            const double ob[2] = {a.obs[2 * o], a.obs[2 * o + 1]}, wt[2] = {a.wts[2 * o], a.wts[2 * o + 1]};
            double tb[9], wbar[2];
            mv_obs_reverse(&L.cams[6 * c], fixed, X, a.fx, a.fy, a.cx, a.cy, ob, wt, rbar, Jbar, tb, wbar);
            b.g_w[2 * o] += wbar[0]; b.g_w[2 * o + 1] += wbar[1];
            double* y = a.Y + 18 * size_t(o);
#pragma unroll
            for (int i = 0; i < 9; ++i) y[i] = tb[i];
        }
        __syncthreads();
        // ---- 5: the adjoint of the iterate: x_bar = x+_bar + what came through r and J -----------------------------------------
        for (int p = tid; p < P; p += kMvThreads) {
            double g0 = 0, g1 = 0, g2 = 0;
            for (int q = a.pt_start[p]; q < a.pt_start[p + 1]; ++q) {
                const double* y = a.Y + 18 * size_t(a.pt_obs[q]);
                g0 += y[6]; g1 += y[7]; g2 += y[8];
            }
            b.pts_bar[3 * p] += g0; b.pts_bar[3 * p + 1] += g1; b.pts_bar[3 * p + 2] += g2;
        }
        for (int f = wave; f < F; f += kMvWaves) {
            const int c = L.free_[f];
            double g[6] = {0, 0, 0, 0, 0, 0};
            for (int q = a.cam_start[c] + lane; q < a.cam_start[c + 1]; q += 64) {
                const double* y = a.Y + 18 * size_t(a.cam_obs[q]);
#pragma unroll
                for (int i = 0; i < 6; ++i) g[i] += y[i];
            }
#pragma unroll
            for (int i = 0; i < 6; ++i) g[i] = wave_sum_d(g[i]);
            if (lane == 0)
#pragma unroll
                for (int i = 0; i < 6; ++i) s_cbar[6 * c + i] += g[i];
        }
    }
}

// ---- host side: the reverse pass' share of the workspace, and the one place that launches mvba_kernel<kLossNone, kLmTape> ------------
static size_t mv_bwd_doubles(const std::vector<int>& Cs, const std::vector<int>& Ps, const std::vector<int>& Os, int max_iterations, bool* overflow) {
    size_t totC = 0, totP = 0, totO = 0;
    for (size_t k = 0; k < Cs.size(); ++k) { totC += size_t(Cs[k]); totP += size_t(Ps[k]); totO += size_t(Os[k]); }
    // the tape (3 + 6 C + 3 P per pass), cams_bar, g_extr, pts_bar, wp, fac_p, g_w - in size_t, and an overflow is an error
    const size_t iters = max_iterations > 0 ? size_t(max_iterations) : 0, cap = ~size_t(0) / sizeof(double) / 2;
    const size_t per_pass = 3 * Cs.size() + 6 * totC + 3 * totP, fixed_part = 22 * totC + 9 * totP + 2 * totO;
    *overflow = iters && per_pass > (cap - fixed_part) / iters;
    return *overflow ? 0 : iters * per_pass + fixed_part;
}

size_t mv_bwd_bytes(const std::vector<int>& Cs, const std::vector<int>& Ps, const std::vector<int>& Os, int max_iterations, bool* overflow) {
    const size_t d = mv_bwd_doubles(Cs, Ps, Os, max_iterations, overflow);
    return *overflow ? 0 : ((Cs.size() * sizeof(MvbaBwdArgs) + 255) & ~size_t(255)) + d * sizeof(double);
}

int mv_bwd_fits(e2emv_ctx* ctx, const char* who, size_t bytes, bool overflow) {
    if (overflow) return set_err(ctx, E2EMV_ENOMEM, "%s: the tape does not fit a size_t", who);
    // a tape beyond the device's whole memory is refused here: nothing is freed, reserved or launched for it
    size_t mem_free = 0, mem_total = 0;
    E2EMV_HIP(ctx, hipMemGetInfo(&mem_free, &mem_total));
    if (bytes > mem_total) return set_err(ctx, E2EMV_ENOMEM, "%s: the tape needs %zu bytes, the device has %zu", who, bytes, mem_total);
    return E2EMV_OK;
}

int mv_bwd_carve(e2emv_ctx* ctx, char* tail, const std::vector<int>& Cs, const std::vector<int>& Ps, const std::vector<int>& Os, int max_iterations,
                 bool with_extr, MvBwdLayout* out, hipStream_t s) {
    const size_t n = Cs.size(), iters = max_iterations > 0 ? size_t(max_iterations) : 0;
    size_t totC = 0, totP = 0, totO = 0;
    for (size_t k = 0; k < n; ++k) { totC += size_t(Cs[k]); totP += size_t(Ps[k]); totO += size_t(Os[k]); }
    MvBwdLayout W{};
    W.recs = reinterpret_cast<MvbaBwdArgs*>(tail);
    double* d = reinterpret_cast<double*>(tail + ((n * sizeof(MvbaBwdArgs) + 255) & ~size_t(255)));
    W.cams_bar = d; d += 6 * totC;
    W.g_extr = d;   d += 16 * totC;
    W.pts_bar = d;  d += 3 * totP;
    W.wp = d;       d += 3 * totP;
    W.fac_p = d;    d += 3 * totP;
    W.g_w = d;      d += 2 * totO;
    std::vector<MvbaBwdArgs> bw(n);
    size_t c0 = 0, p0 = 0, o0 = 0;
    for (size_t k = 0; k < n; ++k) {
        bw[k].tape.it = d; d += 3 * iters;
        bw[k].tape.x = d;  d += iters * (6 * size_t(Cs[k]) + 3 * size_t(Ps[k]));
        bw[k].cams_bar = W.cams_bar + 6 * c0; bw[k].pts_bar = W.pts_bar + 3 * p0; bw[k].wp = W.wp + 3 * p0; bw[k].fac_p = W.fac_p + 3 * p0;
        bw[k].g_w = W.g_w + 2 * o0;
        bw[k].g_extr = with_extr ? W.g_extr + 16 * c0 : nullptr;
        c0 += size_t(Cs[k]); p0 += size_t(Ps[k]); o0 += size_t(Os[k]);
    }
    E2EMV_HIP(ctx, hipMemcpyAsync(W.recs, bw.data(), sizeof(MvbaBwdArgs) * n, hipMemcpyHostToDevice, s));
    E2EMV_HIP(ctx, hipStreamSynchronize(s));  // bw dies at return
    *out = W;
    return E2EMV_OK;
}

int mv_launch_ba_backward(e2emv_ctx* ctx, const MvLayout& L, const MvBwdLayout& W, int n, hipStream_t s) {
    prof_begin(ctx, PS_W8PT, s);
    hipLaunchKernelGGL((mvba_kernel<kLossNone, kLmTape>), dim3(n), dim3(kMvThreads), 0, s, L.recs, W.recs);
    E2EMV_CHECK_LAUNCH(ctx, "mvba_kernel<kLmTape>");
    prof_end(ctx, s);
    return E2EMV_OK;
}

}  // namespace e2emv

using namespace e2emv;

extern "C" int e2emv_mv_bundle_adjust_batch_backward(e2emv_ctx* ctx, int n_problems, const int32_t* n_cams, const int32_t* fixed_cam,
                                                     const double* intr, const int64_t* pt_off, const int64_t* obs_off,
                                                     const int32_t* cam_idx, const int32_t* pt_idx, const double* obs_xy,
                                                     const double* obs_w, const double* cams, const double* pts, int max_iterations,
                                                     const double* g_cams, const double* g_pts, double* g_obs_w, double* g_cams0,
                                                     double* g_pts0, void* stream) {
    if (!ctx) return E2EMV_EINVAL;
    E2EMV_ENTER(ctx, stream);
    const char* who = "mv_bundle_adjust_batch_backward";
    size_t totC = 0, totP = 0, totO = 0;
    int rc = mv_batch_check(ctx, who, n_problems, n_cams, fixed_cam, intr, pt_off, obs_off, cam_idx, pt_idx, obs_xy, obs_w, cams, pts, &totC, &totP, &totO);
    if (rc) return rc;
    if (!g_cams) return set_err(ctx, E2EMV_EINVAL, "%s: NULL g_cams", who);
    if (!g_obs_w && !g_cams0 && !g_pts0) return E2EMV_OK;
    const size_t n = size_t(n_problems);
    std::vector<int> Cs(n), Ps(n), Os(n);
    for (size_t k = 0; k < n; ++k) { Cs[k] = n_cams[k]; Ps[k] = int(pt_off[k + 1] - pt_off[k]); Os[k] = int(obs_off[k + 1] - obs_off[k]); }
    bool overflow = false;
    const size_t tail = mv_bwd_bytes(Cs, Ps, Os, max_iterations, &overflow);
    rc = mv_bwd_fits(ctx, who, tail, overflow);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    MvLayout L;
    rc = mv_batch_upload(ctx, n_problems, n_cams, fixed_cam, intr, pt_off, obs_off, cam_idx, pt_idx, obs_xy, obs_w, cams, pts, max_iterations, 0.0, totC,
                         totP, totO, tail, &L, s);
    if (rc) return rc;
    MvBwdLayout W;
    rc = mv_bwd_carve(ctx, ctx->d_ws + L.bytes, Cs, Ps, Os, max_iterations, false, &W, s);
    if (rc) return rc;
    E2EMV_HIP(ctx, hipMemcpyAsync(W.cams_bar, g_cams, sizeof(double) * 6 * totC, hipMemcpyHostToDevice, s));
    if (totP) {
        if (g_pts) E2EMV_HIP(ctx, hipMemcpyAsync(W.pts_bar, g_pts, sizeof(double) * 3 * totP, hipMemcpyHostToDevice, s));
        else E2EMV_HIP(ctx, hipMemsetAsync(W.pts_bar, 0, sizeof(double) * 3 * totP, s));
    }
    rc = mv_launch_ba_backward(ctx, L, W, n_problems, s);
    if (rc) return rc;
    if (g_cams0) E2EMV_HIP(ctx, hipMemcpyAsync(g_cams0, W.cams_bar, sizeof(double) * 6 * totC, hipMemcpyDeviceToHost, s));
    if (g_pts0 && totP) E2EMV_HIP(ctx, hipMemcpyAsync(g_pts0, W.pts_bar, sizeof(double) * 3 * totP, hipMemcpyDeviceToHost, s));
    if (g_obs_w && totO) E2EMV_HIP(ctx, hipMemcpyAsync(g_obs_w, W.g_w, sizeof(double) * 2 * totO, hipMemcpyDeviceToHost, s));
    E2EMV_HIP(ctx, hipStreamSynchronize(s));
    return E2EMV_OK;
}
