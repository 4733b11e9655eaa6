// RANSAC essential matrix + recoverPose on the device: SuperGlue's estimate_pose (models/utils.py) with OpenCV's
// findEssentialMat(method=RANSAC) / recoverPose semantics, for a ragged batch of P problems in one call.
//
//   init      one lane per problem: iteration budget (niters = max_iters), best count 0
//   rounds of RANSAC_ROUND iterations, launched ceil(max_iters / RANSAC_ROUND) times with no readback in between; a problem
//   whose niters is at or below a round's first iteration returns at once in every kernel of that round:
//     hyp      one lane per iteration: the sample (five_point.h hash), the 5-point solver in fp64, up to 10 E's
//     score    one lane per hypothesis (iteration, model): the problem's matches stream through LDS in tiles and every lane
//              reads the same match (broadcast), counting its inliers in a register
//     resolve  one wave per problem: the sequential rule "a model replaces the best only with strictly more inliers than
//              max(best, 4); each new best shrinks niters" over the round's (iteration, model) order.  A wave prefix-max
//              over 64 entries at a time finds the few entries that set a new running maximum; only those are walked in
//              order (an entry of an iteration at or past niters ends the problem's loop; all models of a running
//              iteration compete, also where the iteration straddles two 64-entry chunks)
//   finalize  one workgroup per problem: the inlier mask of the best E, then recoverPose of every candidate
//              (SVD, four (R, t), DLT triangulation + depth tests) and the candidate with the most points in front
#include "common.h"
#include "five_point.h"
#include "small_linalg.h"

#include <cfloat>

namespace e2emv {

constexpr int RANSAC_ROUND = 128;        // iterations per round
constexpr int RANSAC_MAX_MATCHES = 4096;
constexpr int RANSAC_TILE = 512;         // matches per LDS tile of the scoring kernel (512 x 32 B)
constexpr int ST_NITERS = 0, ST_BEST = 1, ST_LAST_IT = 2, ST_NCAND = 3;

struct RansacParams {
    int P, Mmax, max_iters;
    uint32_t seed;
    double conf;
    const int32_t* n_per;
    const double* k0;      // [P, Mmax, 2]
    const double* k1;
    const double* thresh;  // [P]
    int* st;               // [P, 4]
    double* stE;           // [P, 10, 9] candidates of recoverPose
    double* hypE;          // [P, ROUND, 10, 9]
    int* nsol;             // [P, ROUND]
    int* counts;           // [P, ROUND * 10]
};

__device__ __forceinline__ int problem_size(const RansacParams& p, int q) {
    const int M = p.n_per[q];
    return (M < 0 || M > p.Mmax) ? -1 : M;
}

// OpenCV's RANSACUpdateNumIters(p, ep, modelPoints = 5, maxIters)
__device__ __forceinline__ int update_num_iters(double p, double ep, int max_iters) {
    p = fmin(fmax(p, 0.0), 1.0);
    ep = fmin(fmax(ep, 0.0), 1.0);
    double num = fmax(1.0 - p, DBL_MIN);
    double denom = 1.0 - pow(1.0 - ep, 5.0);
    if (denom < DBL_MIN) return 0;
    num = log(num);
    denom = log(denom);
    return (denom >= 0.0 || -num >= max_iters * (-denom)) ? max_iters : (int)rint(num / denom);
}

__global__ void ransac_init_kernel(RansacParams p) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= p.P) return;
    const int M = problem_size(p, q);
    int* st = p.st + 4 * q;
    st[ST_NITERS] = M < 5 ? 0 : (M == 5 ? 1 : p.max_iters);
    st[ST_BEST] = 0;
    st[ST_LAST_IT] = -1;
    st[ST_NCAND] = 0;
}

__global__ void __launch_bounds__(64) ransac_hyp_kernel(RansacParams p, int r0) {
    const int q = blockIdx.y;
    const int itl = blockIdx.x * 64 + threadIdx.x;
    const int it = r0 + itl;
    const int M = problem_size(p, q);
    int* nsol = p.nsol + (size_t)q * RANSAC_ROUND + itl;
    if (M < 5 || it >= p.st[4 * q + ST_NITERS]) {
        *nsol = 0;
        return;
    }
    int idx[5] = {0, 1, 2, 3, 4};
    if (M > 5 && !fivept::draw_sample(p.seed, (uint32_t)it, (uint32_t)M, idx)) {
        *nsol = 0;
        return;
    }
    double x0[5], y0[5], x1[5], y1[5];
    const double* k0 = p.k0 + (size_t)q * p.Mmax * 2;
    const double* k1 = p.k1 + (size_t)q * p.Mmax * 2;
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        x0[k] = k0[2 * idx[k]];
        y0[k] = k0[2 * idx[k] + 1];
        x1[k] = k1[2 * idx[k]];
        y1[k] = k1[2 * idx[k] + 1];
    }
    double Es[10][9];
    const int n = fivept::solve5(x0, y0, x1, y1, Es);
    double* out = p.hypE + ((size_t)q * RANSAC_ROUND + itl) * 90;
    for (int s = 0; s < n; ++s)
#pragma unroll
        for (int k = 0; k < 9; ++k) out[9 * s + k] = Es[s][k];
    *nsol = n;
}

__global__ void __launch_bounds__(256) ransac_score_kernel(RansacParams p, int r0) {
    __shared__ double4 tile[RANSAC_TILE];
    const int q = blockIdx.y;
    const int M = problem_size(p, q);
    const int niters = p.st[4 * q + ST_NITERS];
    const int h = blockIdx.x * 256 + threadIdx.x;  // hypothesis of the round: iteration h / 10, model h % 10
    // (block-uniform exits: a problem without sampling, or every iteration of this block at or past niters)
    if (M <= 5 || r0 + (int)(blockIdx.x * 256) / 10 >= niters) return;
    const int itl = h / 10, m = h % 10;
    const bool valid = r0 + itl < niters && m < p.nsol[(size_t)q * RANSAC_ROUND + itl];
    double E[9];
    const double* src = p.hypE + ((size_t)q * RANSAC_ROUND + itl) * 90 + 9 * m;
#pragma unroll
    for (int k = 0; k < 9; ++k) E[k] = valid ? src[k] : 0.0;
    const double t2 = p.thresh[q] * p.thresh[q];
    const double* k0 = p.k0 + (size_t)q * p.Mmax * 2;
    const double* k1 = p.k1 + (size_t)q * p.Mmax * 2;
    int count = 0;
    for (int base = 0; base < M; base += RANSAC_TILE) {
        const int nt = min(RANSAC_TILE, M - base);
        __syncthreads();
        for (int i = threadIdx.x; i < nt; i += 256)
            tile[i] = make_double4(k0[2 * (base + i)], k0[2 * (base + i) + 1], k1[2 * (base + i)], k1[2 * (base + i) + 1]);
        __syncthreads();
        if (valid)
            for (int i = 0; i < nt; ++i) {
                const double4 v = tile[i];
                count += fivept::sampson_inlier(E, v.x, v.y, v.z, v.w, t2) ? 1 : 0;
            }
    }
    p.counts[(size_t)q * RANSAC_ROUND * 10 + h] = valid ? count : -1;
}

__global__ void __launch_bounds__(64) ransac_resolve_kernel(RansacParams p, int r0) {
    const int q = blockIdx.x;
    const int lane = threadIdx.x;
    const int M = problem_size(p, q);
    int* st = p.st + 4 * q;
    int niters = st[ST_NITERS];
    if (M < 5 || r0 >= niters) return;
    double* cand = p.stE + (size_t)q * 90;
    const double* hyp = p.hypE + (size_t)q * RANSAC_ROUND * 90;
    if (M == 5) {  // no sampling: every solution of the minimal problem is a candidate, the mask is all ones
        const int n = p.nsol[(size_t)q * RANSAC_ROUND];
        for (int k = lane; k < 9 * n; k += 64) cand[k] = hyp[k];
        if (lane == 0) {
            st[ST_NCAND] = n;
            st[ST_BEST] = n > 0 ? 5 : 0;
            st[ST_LAST_IT] = 0;
        }
        return;
    }
    int best = st[ST_BEST], last_it = st[ST_LAST_IT], run = best, best_k = -1;
    const int* counts = p.counts + (size_t)q * RANSAC_ROUND * 10;
    for (int c = 0; c < RANSAC_ROUND * 10 / 64; ++c) {
        // the whole chunk lies past the loop's end - unless it opens with the rest of the iteration that set the last best:
        // ten entries per iteration and 64 per chunk leave iterations 6, 12, 19, 25 (mod 32) in two chunks, and a record of
        // the models before the seam may have shrunk niters to that very iteration, whose other models still compete
        const int it0 = r0 + (c * 64) / 10;
        if (it0 >= niters && it0 != last_it) break;
        const int k = c * 64 + lane;
        const int cnt = counts[k];
        int v = cnt;  // inclusive prefix maximum over the wave
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int o = __shfl_up(v, off, 64);
            if (lane >= off) v = max(v, o);
        }
        int excl = __shfl_up(v, 1, 64);
        if (lane == 0) excl = -1;
        const bool rec = cnt > max(max(excl, run), 4);
        uint64_t mask = __ballot(rec);
        bool stop = false;
        while (mask) {  // wave-uniform walk over the entries that set a new maximum, in (iteration, model) order
            const int b = __ffsll((unsigned long long)mask) - 1;
            mask &= mask - 1;
            const int kk = c * 64 + b;
            const int itb = r0 + kk / 10;
            const int cb = __shfl(cnt, b, 64);
            // an iteration runs iff it is below niters when it starts; every model of a running iteration is scored
            if (itb != last_it && itb >= niters) {
                stop = true;
                break;
            }
            best = cb;
            best_k = kk;
            last_it = itb;
            niters = update_num_iters(p.conf, (double)(M - cb) / (double)M, niters);
        }
        if (stop) break;
        run = max(run, __shfl(v, 63, 64));
    }
    if (best_k >= 0)
        for (int k = lane; k < 9; k += 64) cand[k] = hyp[(size_t)(best_k / 10) * 90 + 9 * (best_k % 10) + k];
    if (lane == 0) {
        st[ST_NITERS] = niters;
        st[ST_BEST] = best;
        st[ST_LAST_IT] = last_it;
        if (best_k >= 0) st[ST_NCAND] = 1;
    }
}

// SVD of E -> OpenCV's decomposeEssentialMat: U, V with det +1, R1 = U W V^T, R2 = U W^T V^T, t = U[:, 2]
__device__ bool decompose_essential(const double* E, double* R1, double* R2, double* t) {
    double A[3][3], V[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) A[i][j] = E[i] * E[j] + E[3 + i] * E[3 + j] + E[6 + i] * E[6 + j];
    jacobi_static<3>(A, V);
    int o[3] = {0, 1, 2};  // eigenvalues of E^T E descending
    if (A[o[1]][o[1]] > A[o[0]][o[0]]) { int s = o[0]; o[0] = o[1]; o[1] = s; }
    if (A[o[2]][o[2]] > A[o[1]][o[1]]) { int s = o[1]; o[1] = o[2]; o[2] = s; }
    if (A[o[1]][o[1]] > A[o[0]][o[0]]) { int s = o[0]; o[0] = o[1]; o[1] = s; }
    double v[3][3], u[3][3];
#pragma unroll
    for (int k = 0; k < 2; ++k)
#pragma unroll
        for (int i = 0; i < 3; ++i) v[k][i] = V[i][o[k]];
    v[2][0] = v[0][1] * v[1][2] - v[0][2] * v[1][1];
    v[2][1] = v[0][2] * v[1][0] - v[0][0] * v[1][2];
    v[2][2] = v[0][0] * v[1][1] - v[0][1] * v[1][0];
    for (int k = 0; k < 2; ++k) {
        double n = 0.0;
        for (int i = 0; i < 3; ++i) {
            u[k][i] = E[3 * i] * v[k][0] + E[3 * i + 1] * v[k][1] + E[3 * i + 2] * v[k][2];
            n += u[k][i] * u[k][i];
        }
        if (!(n > 1e-300)) return false;  // rank < 2: no decomposition
        n = 1.0 / sqrt(n);
        for (int i = 0; i < 3; ++i) u[k][i] *= n;
    }
    u[2][0] = u[0][1] * u[1][2] - u[0][2] * u[1][1];
    u[2][1] = u[0][2] * u[1][0] - u[0][0] * u[1][2];
    u[2][2] = u[0][0] * u[1][1] - u[0][1] * u[1][0];
    bool ok = true;
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) {
            R1[3 * i + j] = -u[1][i] * v[0][j] + u[0][i] * v[1][j] + u[2][i] * v[2][j];
            R2[3 * i + j] = u[1][i] * v[0][j] - u[0][i] * v[1][j] + u[2][i] * v[2][j];
            ok &= isfinite(R1[3 * i + j]) && isfinite(R2[3 * i + j]);
        }
        t[i] = u[2][i];
        ok &= isfinite(t[i]);
    }
    return ok;
}

// recoverPose's test of one match against [R | t]: homogeneous DLT point X (P0 = [I | 0]) with z w > 0, z / w below the
// distance threshold, and depth in the second camera in (0, threshold)
__device__ bool in_front(double x0, double y0, double x1, double y1, const double* R, const double* t, double dist) {
    double Rt[12];
#pragma unroll
    for (int k = 0; k < 9; ++k) Rt[k] = R[k];
    Rt[9] = t[0]; Rt[10] = t[1]; Rt[11] = t[2];
    double Ar[4][4];
    Ar[0][0] = -1.0; Ar[0][1] = 0.0; Ar[0][2] = x0; Ar[0][3] = 0.0;
    Ar[1][0] = 0.0; Ar[1][1] = -1.0; Ar[1][2] = y0; Ar[1][3] = 0.0;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        Ar[2][j] = x1 * Rt[6 + j] - Rt[j];
        Ar[3][j] = y1 * Rt[6 + j] - Rt[3 + j];
    }
    Ar[2][3] = x1 * Rt[11] - Rt[9];
    Ar[3][3] = y1 * Rt[11] - Rt[10];
    double G[4][4], V[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = i; j < 4; ++j) {
            const double s = Ar[0][i] * Ar[0][j] + Ar[1][i] * Ar[1][j] + Ar[2][i] * Ar[2][j] + Ar[3][i] * Ar[3][j];
            G[i][j] = s;
            G[j][i] = s;
        }
    jacobi_static<4>(G, V);
    int mi = 0;
#pragma unroll
    for (int i = 1; i < 4; ++i)
        if (G[i][i] < G[mi][mi]) mi = i;
    double X[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) X[i] = (mi == 0) ? V[i][0] : (mi == 1) ? V[i][1] : (mi == 2) ? V[i][2] : V[i][3];
    if (!(X[2] * X[3] > 0.0)) return false;
    const double X0 = X[0] / X[3], X1 = X[1] / X[3], X2 = X[2] / X[3];
    if (!(X2 < dist)) return false;
    const double z2 = R[6] * X0 + R[7] * X1 + R[8] * X2 + t[2];
    return z2 > 0.0 && z2 < dist;
}

__global__ void __launch_bounds__(256) ransac_finalize_kernel(RansacParams p, double* d_E, double* d_R, double* d_t, uint8_t* d_inl,
                                                              int32_t* d_ninl, int32_t* d_ncheir, int32_t* d_iters, int32_t* d_status) {
    __shared__ double sR[2][9], st_[3], bestR[9], bestt[3], bestE[9];
    __shared__ int s_cnt[5], s_ok, s_best_n;
    const int q = blockIdx.x, tid = threadIdx.x;
    const int M = problem_size(p, q);
    const int* st = p.st + 4 * q;
    const int ncand = M >= 5 ? st[ST_NCAND] : 0;
    const double* k0 = p.k0 + (size_t)q * p.Mmax * 2;
    const double* k1 = p.k1 + (size_t)q * p.Mmax * 2;
    uint8_t* inl = d_inl + (size_t)q * p.Mmax;
    if (tid == 0) {
        s_cnt[4] = 0;
        s_best_n = 0;
    }
    __syncthreads();
    // RANSAC inlier mask of the best E (M == 5: all ones); padding rows and failed problems read 0
    const double* E0 = p.stE + (size_t)q * 90;
    const double t2 = p.thresh[q] * p.thresh[q];
    int n_in = 0;
    for (int i = tid; i < p.Mmax; i += 256) {
        bool v = false;
        if (ncand > 0 && i < M) v = (M == 5) || fivept::sampson_inlier(E0, k0[2 * i], k0[2 * i + 1], k1[2 * i], k1[2 * i + 1], t2);
        inl[i] = v ? 1 : 0;
        n_in += v ? 1 : 0;
    }
    atomicAdd(&s_cnt[4], n_in);
    for (int c = 0; c < ncand; ++c) {
        if (tid == 0) {
            s_ok = decompose_essential(p.stE + (size_t)q * 90 + 9 * c, &sR[0][0], &sR[1][0], st_) ? 1 : 0;
            s_cnt[0] = s_cnt[1] = s_cnt[2] = s_cnt[3] = 0;
        }
        __syncthreads();
        if (s_ok) {
            int g[4] = {0, 0, 0, 0};
            const double nt[3] = {-st_[0], -st_[1], -st_[2]};
            for (int i = tid; i < M; i += 256) {
                if (!inl[i]) continue;
                const double x0 = k0[2 * i], y0 = k0[2 * i + 1], x1 = k1[2 * i], y1 = k1[2 * i + 1];
                g[0] += in_front(x0, y0, x1, y1, sR[0], st_, 1e9);
                g[1] += in_front(x0, y0, x1, y1, sR[1], st_, 1e9);
                g[2] += in_front(x0, y0, x1, y1, sR[0], nt, 1e9);
                g[3] += in_front(x0, y0, x1, y1, sR[1], nt, 1e9);
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) atomicAdd(&s_cnt[k], g[k]);
        }
        __syncthreads();
        if (tid == 0 && s_ok) {
            const int* g = s_cnt;  // recoverPose's choice: ties go to the first of (R1,t), (R2,t), (R1,-t), (R2,-t)
            int sel;
            if (g[0] >= g[1] && g[0] >= g[2] && g[0] >= g[3]) sel = 0;
            else if (g[1] >= g[0] && g[1] >= g[2] && g[1] >= g[3]) sel = 1;
            else if (g[2] >= g[0] && g[2] >= g[1] && g[2] >= g[3]) sel = 2;
            else sel = 3;
            if (g[sel] > s_best_n) {  // estimate_pose keeps the E of the largest count, only when it is above 0
                s_best_n = g[sel];
                const double sg = sel >= 2 ? -1.0 : 1.0;
                for (int k = 0; k < 9; ++k) {
                    bestR[k] = sR[sel & 1][k];
                    bestE[k] = p.stE[(size_t)q * 90 + 9 * c + k];
                }
                for (int k = 0; k < 3; ++k) bestt[k] = sg * st_[k];
            }
        }
        __syncthreads();
    }
    __syncthreads();
    if (tid == 0) {
        const bool ok = s_best_n > 0;
        for (int k = 0; k < 9; ++k) {
            d_E[9 * q + k] = ok ? bestE[k] : 0.0;
            d_R[9 * q + k] = ok ? bestR[k] : 0.0;
        }
        for (int k = 0; k < 3; ++k) d_t[3 * q + k] = ok ? bestt[k] : 0.0;
        d_ninl[q] = s_cnt[4];
        d_ncheir[q] = s_best_n;
        // iterations run: the loop ends at the first iteration >= niters after the last new best
        d_iters[q] = M < 5 ? 0 : (M == 5 ? 1 : max(st[ST_LAST_IT] + 1, st[ST_NITERS]));
        d_status[q] = M < 0 ? 4 : M < 5 ? 1 : ncand == 0 ? 2 : ok ? 0 : 3;
    }
}

__global__ void __launch_bounds__(64) five_point_kernel(int n, const double* x0, const double* x1, double* E, int32_t* nsol) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    double a[5], b[5], c[5], d[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        a[k] = x0[10 * i + 2 * k];
        b[k] = x0[10 * i + 2 * k + 1];
        c[k] = x1[10 * i + 2 * k];
        d[k] = x1[10 * i + 2 * k + 1];
    }
    double Es[10][9];
    const int ns = fivept::solve5(a, b, c, d, Es);
    for (int s = 0; s < 10; ++s)
#pragma unroll
        for (int k = 0; k < 9; ++k) E[(size_t)i * 90 + 9 * s + k] = s < ns ? Es[s][k] : 0.0;
    nsol[i] = ns;
}

}  // namespace e2emv

using namespace e2emv;

extern "C" int e2emv_essential_ransac(e2emv_ctx* ctx, int P, int Mmax, const int32_t* d_n_per, const double* d_kpts0n,
                                      const double* d_kpts1n, const double* d_thresh, double conf, int max_iters, uint32_t seed,
                                      double* d_E, double* d_R, double* d_t, uint8_t* d_inliers, int32_t* d_n_inliers,
                                      int32_t* d_n_cheiral, int32_t* d_iters, int32_t* d_status, void* stream) {
    if (!ctx || !d_n_per || !d_kpts0n || !d_kpts1n || !d_thresh || !d_E || !d_R || !d_t || !d_inliers || !d_n_inliers ||
        !d_n_cheiral || !d_iters || !d_status)
        return E2EMV_EINVAL;
    E2EMV_ENTER(ctx, stream);
    if (P <= 0 || Mmax <= 0 || Mmax > RANSAC_MAX_MATCHES)
        return set_err(ctx, E2EMV_ESHAPE, "essential_ransac: P=%d Mmax=%d (1 <= Mmax <= %d)", P, Mmax, RANSAC_MAX_MATCHES);
    if (max_iters <= 0 || max_iters > (1 << 20)) return set_err(ctx, E2EMV_ESHAPE, "essential_ransac: max_iters=%d", max_iters);
    if (!(conf >= 0.0 && conf <= 1.0)) return set_err(ctx, E2EMV_EINVAL, "essential_ransac: conf=%g outside [0, 1]", conf);
    hipStream_t s = (hipStream_t)stream;
    auto al = [](size_t n) { return (n + 255) & ~size_t(255); };
    const size_t sz_st = al((size_t)P * 4 * 4), sz_stE = al((size_t)P * 90 * 8), sz_hyp = al((size_t)P * RANSAC_ROUND * 90 * 8),
                 sz_ns = al((size_t)P * RANSAC_ROUND * 4), sz_cnt = al((size_t)P * RANSAC_ROUND * 10 * 4);
    int rc = ws_reserve(ctx, sz_st + sz_stE + sz_hyp + sz_ns + sz_cnt);
    if (rc) return rc;
    char* w = ctx->d_ws;
    RansacParams p{};
    p.P = P; p.Mmax = Mmax; p.max_iters = max_iters; p.seed = seed; p.conf = conf;
    p.n_per = d_n_per; p.k0 = d_kpts0n; p.k1 = d_kpts1n; p.thresh = d_thresh;
    p.st = (int*)w; w += sz_st;
    p.stE = (double*)w; w += sz_stE;
    p.hypE = (double*)w; w += sz_hyp;
    p.nsol = (int*)w; w += sz_ns;
    p.counts = (int*)w;
    prof_begin(ctx, PS_W8PT, s);
    hipLaunchKernelGGL(ransac_init_kernel, dim3((P + 63) / 64), dim3(64), 0, s, p);
    E2EMV_CHECK_LAUNCH(ctx, "ransac_init_kernel");
    const int rounds = (max_iters + RANSAC_ROUND - 1) / RANSAC_ROUND;
    for (int r = 0; r < rounds; ++r) {
        const int r0 = r * RANSAC_ROUND;
        hipLaunchKernelGGL(ransac_hyp_kernel, dim3(RANSAC_ROUND / 64, P), dim3(64), 0, s, p, r0);
        E2EMV_CHECK_LAUNCH(ctx, "ransac_hyp_kernel");
        hipLaunchKernelGGL(ransac_score_kernel, dim3(RANSAC_ROUND * 10 / 256, P), dim3(256), 0, s, p, r0);
        E2EMV_CHECK_LAUNCH(ctx, "ransac_score_kernel");
        hipLaunchKernelGGL(ransac_resolve_kernel, dim3(P), dim3(64), 0, s, p, r0);
        E2EMV_CHECK_LAUNCH(ctx, "ransac_resolve_kernel");
    }
    hipLaunchKernelGGL(ransac_finalize_kernel, dim3(P), dim3(256), 0, s, p, d_E, d_R, d_t, d_inliers, d_n_inliers, d_n_cheiral,
                       d_iters, d_status);
    prof_end(ctx, s);
    E2EMV_CHECK_LAUNCH(ctx, "ransac_finalize_kernel");
    return E2EMV_OK;
}

extern "C" int e2emv_essential_5pt(e2emv_ctx* ctx, int n, const double* d_x0, const double* d_x1, double* d_E, int32_t* d_nsol,
                                   void* stream) {
    if (!ctx || !d_x0 || !d_x1 || !d_E || !d_nsol) return E2EMV_EINVAL;
    E2EMV_ENTER(ctx, stream);
    if (n <= 0) return set_err(ctx, E2EMV_ESHAPE, "essential_5pt: n=%d", n);
    hipStream_t s = (hipStream_t)stream;
    prof_begin(ctx, PS_W8PT, s);
    hipLaunchKernelGGL(five_point_kernel, dim3((n + 63) / 64), dim3(64), 0, s, n, d_x0, d_x1, d_E, d_nsol);
    prof_end(ctx, s);
    E2EMV_CHECK_LAUNCH(ctx, "five_point_kernel");
    return E2EMV_OK;
}
