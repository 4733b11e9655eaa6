// Sinkhorn log-space optimal transport with dustbins + mutual-arg-max matching.
//
// Restates upstream SuperGlue `log_optimal_transport` / `log_sinkhorn_iterations` and the
// match block of `SuperGlue.forward` (superglue.py; the reference runs them inside its
// absent MultiViewMatcher.forward - call sites helpers.py:246, eval_pairs.py:212).
//
// HBM plan.  The reference (torch) runs, per iteration, two `Z + v` adds and two
// logsumexp's over the (N+1)^2 couplings: ~10 sweeps.  SURVEY.md 8(d)'s byte model charges
// 2 sweeps / iteration.  Here ONE sweep per iteration:
//   * the couplings matrix is never built: the dustbin row/column are the constant alpha, so
//     only the aligned core S [M][ldS] is streamed and the dustbin terms are added
//     analytically;
//   * a workgroup owns 16 full rows (4 waves x 4 rows, 64 floats per lane in registers):
//     it computes u for its rows (row LSE = wave shuffles only) and, FROM THE SAME REGISTERS,
//     the per-column partial (max, sum-exp) of S + u over its 16 rows (cross-wave through
//     LDS).  `sinkhorn_combine` (64 columns x 4 chunk ranges per workgroup) folds the M/16 partials into
//     v and the two dustbin scalars.
// Row loads are 16 B per lane, 1 KiB contiguous per wave instruction.
// The final sweep writes logZ = couplings + u + v + log(M+N) densely ([M+1][N+1], the API
// layout) and fuses the row/column arg-max needed by the match block, so Z is never re-read.
//
//
// That launch chain is the fallback today (iters == 0, the `stream` pin, devices that cannot hold a problem's workgroups at
// once), its FINAL sweep the last step of every call, and the reference the resident kernels are tested against.  This file
// also holds what runs behind the resident kernels of sinkhorn_resident.hip / sinkhorn_regs.hip - sinkhorn_rescue - and the
// match block with its stand-alone entry e2emv_extract_matches.  sinkhorn.hip drives all of it.
#include <utility>

#include "sinkhorn_internal.h"
#include "sinkhorn_exchange.h"  // f32x4, SKR_GAVE_UP_NAN (sinkhorn_rescue recognises a give-up by its NaN)

namespace e2emv {

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// block-wide (256 threads) max / sum through LDS scratch (>= 8 floats)
__device__ __forceinline__ float block_max(float v, float* red) {
    v = wave_max(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    float r = red[0];
    for (int i = 1; i < (int)(blockDim.x >> 6); ++i) r = fmaxf(r, red[i]);
    return r;
}
__device__ __forceinline__ float block_sum(float v, float* red) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    float r = red[0];
    for (int i = 1; i < (int)(blockDim.x >> 6); ++i) r += red[i];
    return r;
}


// One sweep of S: u for 16 rows + column partials of S + u.  KT = ceil(ldS / 256).
// FULL = (N == ldS == KT*256): every lane owns valid columns only, so the per-element column guards (which
// hipcc turns into ~90 exec-mask branches) disappear - the case of the 256/512/1024/2048-keypoint configs.
template <int KT, bool FINAL, bool FULL>
__global__ __launch_bounds__(256) void sinkhorn_sweep(SkParams p) {
    extern __shared__ __attribute__((aligned(16))) float lds[];  // [4 waves][2][KT*256]
    const int b = blockIdx.y, chunk = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int row0 = chunk * SK_ROWS + wave * 4;
    const float* Sb = p.S + (int64_t)b * p.M * p.ldS;
    const float* vb = p.v + (int64_t)b * p.ldV;

    if (FINAL && chunk == p.chunks) {
        // dustbin row of logZ: (alpha + u_M) + v_j + log(M+N)
        float* const zbase = p.logZ[b / p.group_batch];
        if (zbase) {
            const float uM = p.u[(int64_t)b * (p.M + 1) + p.M];
            float* zr = zbase + ((int64_t)(b % p.group_batch) * (p.M + 1) + p.M) * (p.N + 1);
            for (int j = tid; j <= p.N; j += 256) zr[j] = ((p.alpha + uM) + vb[j]) - p.norm;
        }
        return;
    }

    float z[4][KT][4];
    float vv[KT][4];
    int col[KT];
#pragma unroll
    for (int k = 0; k < KT; ++k) {
        col[k] = 4 * (lane + 64 * k);
        f32x4 t = (FULL || col[k] < p.ldS) ? *reinterpret_cast<const f32x4*>(vb + col[k]) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int e = 0; e < 4; ++e) vv[k][e] = t[e];
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int row = min(row0 + r, p.M - 1);
#pragma unroll
        for (int k = 0; k < KT; ++k) {
            f32x4 t = (FULL || col[k] < p.ldS) ? *reinterpret_cast<const f32x4*>(Sb + (int64_t)row * p.ldS + col[k])
                                       : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int e = 0; e < 4; ++e) z[r][k][e] = t[e];
        }
    }
    const float vN = vb[p.N];
    float ur[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const bool rvalid = row0 + r < p.M;
        if (!FINAL) {
            // u_i = log_mu - LSE_j(S_ij + v_j  U  alpha + v_N)
            float mx = p.alpha + vN;
#pragma unroll
            for (int k = 0; k < KT; ++k)
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (FULL || col[k] + e < p.N) mx = fmaxf(mx, z[r][k][e] + vv[k][e]);
            mx = wave_max(mx);
            float sm = 0.f;
#pragma unroll
            for (int k = 0; k < KT; ++k)
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (FULL || col[k] + e < p.N) sm += __expf(z[r][k][e] + vv[k][e] - mx);
            sm = wave_sum(sm) + __expf(p.alpha + vN - mx);
            ur[r] = p.norm - (mx + __logf(sm));
            if (rvalid && lane == 0) p.u[(int64_t)b * (p.M + 1) + row0 + r] = ur[r];
        } else {
            ur[r] = p.u[(int64_t)b * (p.M + 1) + min(row0 + r, p.M - 1)];
        }
        if (!rvalid) ur[r] = -INFINITY;  // ragged last chunk: row does not exist
    }

    float* lm = lds + (wave * 2 + 0) * (KT * 256);
    float* ls = lds + (wave * 2 + 1) * (KT * 256);
    if (!FINAL) {
        // (max, sum-exp) of this wave's u values: feeds the dustbin column v_N in sinkhorn_combine
        const float uwm = fmaxf(fmaxf(ur[0], ur[1]), fmaxf(ur[2], ur[3]));
        const float uwm_s = (uwm == -INFINITY) ? 0.f : uwm;
        const float uws = __expf(ur[0] - uwm_s) + __expf(ur[1] - uwm_s) + __expf(ur[2] - uwm_s) + __expf(ur[3] - uwm_s);
        // column partials over this wave's 4 rows: (max, sum exp) of S_ij + u_i
#pragma unroll
        for (int k = 0; k < KT; ++k) {
            f32x4 m4, s4;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float y0 = z[0][k][e] + ur[0], y1 = z[1][k][e] + ur[1], y2 = z[2][k][e] + ur[2], y3 = z[3][k][e] + ur[3];
                float m = fmaxf(fmaxf(y0, y1), fmaxf(y2, y3));
                float mm = (m == -INFINITY) ? 0.f : m;
                m4[e] = m;
                s4[e] = __expf(y0 - mm) + __expf(y1 - mm) + __expf(y2 - mm) + __expf(y3 - mm);
            }
            *reinterpret_cast<f32x4*>(lm + col[k]) = m4;
            *reinterpret_cast<f32x4*>(ls + col[k]) = s4;
        }
        __syncthreads();
        // fold the 4 waves; thread owns 4 consecutive columns per 1024-column group
        for (int c = tid * 4; c < p.ldS; c += 1024) {
            f32x4 M4 = *reinterpret_cast<const f32x4*>(lds + c);
#pragma unroll
            for (int w = 1; w < 4; ++w) {
                f32x4 t = *reinterpret_cast<const f32x4*>(lds + (w * 2) * (KT * 256) + c);
#pragma unroll
                for (int e = 0; e < 4; ++e) M4[e] = fmaxf(M4[e], t[e]);
            }
            f32x4 S4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                f32x4 tm = *reinterpret_cast<const f32x4*>(lds + (w * 2) * (KT * 256) + c);
                f32x4 ts = *reinterpret_cast<const f32x4*>(lds + (w * 2 + 1) * (KT * 256) + c);
#pragma unroll
                for (int e = 0; e < 4; ++e) S4[e] += ts[e] * __expf(tm[e] - M4[e]);  // exp(-inf) = 0 for empty waves
            }
            const int64_t o = ((int64_t)b * p.chunks + chunk) * p.ldS + c;
            *reinterpret_cast<f32x4*>(p.pm + o) = M4;
            *reinterpret_cast<f32x4*>(p.ps + o) = S4;
        }
        __syncthreads();  // the fold is done with the LDS image: reuse its head for the u partials
        if (lane == 0) { lds[wave] = uwm; lds[4 + wave] = uws; }
        __syncthreads();
        if (tid == 0) {
            const float M4 = fmaxf(fmaxf(lds[0], lds[1]), fmaxf(lds[2], lds[3]));
            float S4 = 0.f;
            for (int w = 0; w < 4; ++w) S4 += lds[4 + w] * __expf(lds[w] - M4);
            p.upm[(int64_t)b * p.chunks + chunk] = M4;
            p.ups[(int64_t)b * p.chunks + chunk] = S4;
        }
    } else {
        // final: write logZ rows, row arg-max (first max wins), column partial arg-max
        int* li = reinterpret_cast<int*>(ls);
        float* const zbase = p.logZ[b / p.group_batch];
        const int bl = b % p.group_batch;
        float cm[KT][4];
        int ci[KT][4];
#pragma unroll
        for (int k = 0; k < KT; ++k)
#pragma unroll
            for (int e = 0; e < 4; ++e) { cm[k][e] = -INFINITY; ci[k][e] = 0; }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = row0 + r;
            const bool rvalid = row < p.M;  // wave-uniform
            float best = -INFINITY;
            int bj = 0x7fffffff;
            float* zr = zbase ? zbase + ((int64_t)bl * (p.M + 1) + row) * (p.N + 1) : nullptr;
#pragma unroll
            for (int k = 0; k < KT; ++k)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int j = col[k] + e;
                    if (FULL || j < p.N) {
                        // same association as the reference: ((couplings + u) + v) - norm
                        const float zz = ((z[r][k][e] + ur[r]) + vv[k][e]) - p.norm;
                        if (rvalid) {
                            if (zr) zr[j] = zz;
                            if (zz > best) { best = zz; bj = j; }
                            if (zz > cm[k][e]) { cm[k][e] = zz; ci[k][e] = row; }
                        }
                    }
                }
            if (rvalid) {
                if (zr && lane == 0) zr[p.N] = ((p.alpha + ur[r]) + vN) - p.norm;
                // wave arg-max, lowest index on ties (torch CPU max semantics)
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) {
                    float ob = __shfl_xor(best, o);
                    int oj = __shfl_xor(bj, o);
                    if (ob > best || (ob == best && oj < bj)) { best = ob; bj = oj; }
                }
                if (lane == 0) {
                    p.max0[(int64_t)b * p.M + row] = best;
                    // no element compared greater than -inf (a row of -inf or NaN): index 0, as torch.max gives; match_finalize
                    // indexes its LDS arrays with this value
                    p.idx0[(int64_t)b * p.M + row] = bj == 0x7fffffff ? 0 : bj;
                }
            }
        }
#pragma unroll
        for (int k = 0; k < KT; ++k)
#pragma unroll
            for (int e = 0; e < 4; ++e) { lm[col[k] + e] = cm[k][e]; li[col[k] + e] = ci[k][e]; }
        __syncthreads();
        for (int c = tid; c < p.ldS; c += 256) {
            float bm = lds[c];
            int bi = reinterpret_cast<int*>(lds + (KT * 256))[c];
#pragma unroll
            for (int w = 1; w < 4; ++w) {  // waves own increasing rows: strict > keeps the first
                float m = lds[(w * 2) * (KT * 256) + c];
                int i = reinterpret_cast<int*>(lds + (w * 2 + 1) * (KT * 256))[c];
                if (m > bm) { bm = m; bi = i; }
            }
            const int64_t o = ((int64_t)b * p.chunks + chunk) * p.ldS + c;
            p.pv[o] = bm;
            p.pi[o] = bi;
        }
    }
}

// Fold the column partials into v.  grid (ceil(ldV/64), B), 64 columns x 4 chunk ranges per workgroup; the partial rows
// are read as coalesced 256-byte wave loads.  Every workgroup first recomputes the
// dustbin-ROW potential u_M of this iteration from the previous v (N+1 values, L2-resident);
// workgroup x == 0 also produces the dustbin-COLUMN potential v_N from the u partials.
// v is double-buffered (reads p.v, writes p.v_next) because workgroups of one launch overlap.
__global__ __launch_bounds__(256) void sinkhorn_combine(SkParams p) {
    __shared__ float red[8];
    const int b = blockIdx.y, tid = threadIdx.x;
    const float* vprev = p.v + (int64_t)b * p.ldV;
    float* vb = p.v_next + (int64_t)b * p.ldV;
    // u_M = log_mu_M - (alpha + LSE(v_0..v_N)),  log_mu_M = log N + norm
    float vm = -INFINITY;
    for (int j = tid; j <= p.N; j += 256) vm = fmaxf(vm, vprev[j]);
    vm = block_max(vm, red);
    float vs = 0.f;
    for (int j = tid; j <= p.N; j += 256) vs += __expf(vprev[j] - vm);
    vs = block_sum(vs, red);
    const float uM = (__logf((float)p.N) + p.norm) - (p.alpha + vm + __logf(vs));
    // v_j = log_nu - LSE_i(S_ij + u_i  U  alpha + u_M).  64 columns per workgroup, the chunk list of a column split over
    // 4 threads (4x the loads in flight, 4x the workgroups: the plain one-thread-per-column form ran 160 workgroups on
    // 256 CUs and was latency-bound at 9.7 us); the 4 partial (max, sum) pairs are merged in a fixed order.
    __shared__ float pm4[4][64], ps4[4][64];
    const int part = tid >> 6, cl = tid & 63;
    const int j = blockIdx.x * 64 + cl;
    if (j < p.N) {
        const int cps = (p.chunks + 3) >> 2, c0 = part * cps, c1 = min(p.chunks, c0 + cps);
        float Mx = part == 0 ? p.alpha + uM : -INFINITY, Sx = part == 0 ? 1.f : 0.f;
        const float* pm = p.pm + (int64_t)b * p.chunks * p.ldS + j;
        const float* ps = p.ps + (int64_t)b * p.chunks * p.ldS + j;
#pragma unroll 8
        for (int ch = c0; ch < c1; ++ch) {
            const float m = pm[(int64_t)ch * p.ldS], s = ps[(int64_t)ch * p.ldS];
            const float nm = fmaxf(Mx, m);
            Sx = Sx * __expf(Mx - nm) + s * __expf(m - nm);
            Mx = nm;
        }
        pm4[part][cl] = Mx;
        ps4[part][cl] = Sx;
    }
    __syncthreads();
    if (part == 0) {
        if (j < p.N) {
            float Mx = pm4[0][cl], Sx = ps4[0][cl];
#pragma unroll
            for (int q = 1; q < 4; ++q) {
                const float m = pm4[q][cl], s2 = ps4[q][cl];
                if (s2 > 0.f) {  // an empty part (fewer than 4 chunks) contributes nothing
                    const float nm = fmaxf(Mx, m);
                    Sx = Sx * __expf(Mx - nm) + s2 * __expf(m - nm);
                    Mx = nm;
                }
            }
            vb[j] = p.norm - (Mx + __logf(Sx));
        } else if (j > p.N && j < p.ldV) {
            vb[j] = 0.f;
        }
    }
    if (blockIdx.x == 0) {
        // v_N = log_nu_N - (alpha + LSE(u_0..u_M)),  log_nu_N = log M + norm
        float um = (tid == 0) ? uM : -INFINITY;
        for (int c = tid; c < p.chunks; c += 256) um = fmaxf(um, p.upm[(int64_t)b * p.chunks + c]);
        um = block_max(um, red);
        float us = (tid == 0) ? __expf(uM - um) : 0.f;
        for (int c = tid; c < p.chunks; c += 256)
            us += p.ups[(int64_t)b * p.chunks + c] * __expf(p.upm[(int64_t)b * p.chunks + c] - um);
        us = block_sum(us, red);
        if (tid == 0) {
            vb[p.N] = (__logf((float)p.M) + p.norm) - (p.alpha + um + __logf(us));
            p.u[(int64_t)b * (p.M + 1) + p.M] = uM;  // read by the final sweep
        }
    }
}

__global__ void sinkhorn_init(SkParams p, int B) {
    const int b = blockIdx.x;
    float* vb = p.v + (int64_t)b * p.ldV;
    for (int j = threadIdx.x; j < p.ldV; j += blockDim.x) vb[j] = 0.f;
}

// degenerate iters == 0: u = 0 (the reference returns couplings + 0 + 0 - norm)
__global__ void sinkhorn_zero_u(SkParams p) {
    const int b = blockIdx.x;
    float* ub = p.u + (int64_t)b * (p.M + 1);
    for (int i = threadIdx.x; i <= p.M; i += blockDim.x) ub[i] = 0.f;
}

struct MatchParams {
    int M, N, chunks;
    int64_t ldS;
    const float* max0;  // [B][M]
    const int* idx0;    // [B][M]
    const float* pv;    // [B][chunks][ldS]
    const int* pi;
    const int* idx1_in;  // [B][N] when the column arg-max is already final (dense path), else null
    float thr;
    int group_batch;
    int64_t* m0[kMaxGroups];
    int64_t* m1[kMaxGroups];
    float* ms0[kMaxGroups];
    float* ms1[kMaxGroups];
};

// Mutual check (match block of SuperGlue.forward).  One workgroup per pair, indices in LDS; 1024 threads: the kernel is a chain of
// dependent loads per column (the chunk partials of the column arg-max) on as few workgroups as there are pairs - 256 threads
// took 35 us for 32 pairs of 1024 keypoints.
constexpr int MF_THREADS = 1024;
__global__ __launch_bounds__(MF_THREADS) void match_finalize(MatchParams p) {
    extern __shared__ int sidx[];  // idx0 [M] | idx1 [N] | valid0 [M]
    int* i0 = sidx;
    int* i1 = sidx + p.M;
    int* v0 = sidx + p.M + p.N;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int grp = b / p.group_batch, bl = b % p.group_batch;
    int64_t* const om0 = p.m0[grp];
    int64_t* const om1 = p.m1[grp];
    float* const oms0 = p.ms0[grp];
    float* const oms1 = p.ms1[grp];
    for (int i = tid; i < p.M; i += MF_THREADS) i0[i] = p.idx0[(int64_t)b * p.M + i];
    for (int j = tid; j < p.N; j += MF_THREADS) {
        if (p.idx1_in) {
            i1[j] = p.idx1_in[(int64_t)b * p.N + j];
        } else {
            const int64_t o = (int64_t)b * p.chunks * p.ldS + j;
            float bm = p.pv[o];
            int bi = p.pi[o];
            // chunks own increasing rows: strict > keeps the first.  Both arrays are read unconditionally, 8 chunks at a
            // time, so the loads of a group are in flight together (the loop used to be one dependent L2 round trip per chunk)
            int ch = 1;
            for (; ch + 8 <= p.chunks; ch += 8) {
                float m[8];
                int ix[8];
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    m[q] = p.pv[o + (int64_t)(ch + q) * p.ldS];
                    ix[q] = p.pi[o + (int64_t)(ch + q) * p.ldS];
                }
#pragma unroll
                for (int q = 0; q < 8; ++q)
                    if (m[q] > bm) { bm = m[q]; bi = ix[q]; }
            }
            for (; ch < p.chunks; ++ch) {
                const float m = p.pv[o + (int64_t)ch * p.ldS];
                if (m > bm) { bm = m; bi = p.pi[o + (int64_t)ch * p.ldS]; }
            }
            i1[j] = bi;
        }
    }
    __syncthreads();
    for (int i = tid; i < p.M; i += MF_THREADS) {
        const int j = i0[i];
        const bool mutual = i1[j] == i;
        const float sc = mutual ? __expf(p.max0[(int64_t)b * p.M + i]) : 0.f;
        const bool valid = mutual && sc > p.thr;
        v0[i] = valid;
        if (oms0) oms0[(int64_t)bl * p.M + i] = sc;
        if (om0) om0[(int64_t)bl * p.M + i] = valid ? (int64_t)j : (int64_t)-1;
    }
    __syncthreads();
    for (int j = tid; j < p.N; j += MF_THREADS) {
        const int i = i1[j];
        const bool mutual = i0[i] == j;
        // mscores1 = where(mutual1, mscores0.gather(idx1), 0): mscores0[i] is exp(max0[i]) iff i is mutual
        const bool mut_i = i1[i0[i]] == i;
        const float sc = (mutual && mut_i) ? __expf(p.max0[(int64_t)b * p.M + i]) : 0.f;
        if (oms1) oms1[(int64_t)bl * p.N + j] = sc;
        if (om1) om1[(int64_t)bl * p.N + j] = (mutual && v0[i]) ? (int64_t)i : (int64_t)-1;
    }
}

// ---- dense-logZ arg-max (stand-alone e2emv_extract_matches) ----
__global__ __launch_bounds__(256) void dense_row_argmax(const float* Z, int M, int N, float* max0, int* idx0) {
    const int b = blockIdx.y, row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= M) return;
    const float* zr = Z + ((int64_t)b * (M + 1) + row) * (N + 1);
    float best = -INFINITY;
    int bj = 0x7fffffff;
    for (int j = lane; j < N; j += 64) {
        float zz = zr[j];
        if (zz > best) { best = zz; bj = j; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        float ob = __shfl_xor(best, o);
        int oj = __shfl_xor(bj, o);
        if (ob > best || (ob == best && oj < bj)) { best = ob; bj = oj; }
    }
    if (lane == 0) { max0[(int64_t)b * M + row] = best; idx0[(int64_t)b * M + row] = bj == 0x7fffffff ? 0 : bj; }  // as in the final sweep
}
__global__ __launch_bounds__(256) void dense_col_argmax(const float* Z, int M, int N, int* idx1) {
    const int b = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
    if (j >= N) return;
    const float* zc = Z + (int64_t)b * (M + 1) * (N + 1) + j;
    float best = -INFINITY;
    int bi = 0;
    for (int i = 0; i < M; ++i) {
        float zz = zc[(int64_t)i * (N + 1)];
        if (zz > best) { best = zz; bi = i; }
    }
    idx1[(int64_t)b * N + j] = bi;
}

__global__ void pad_copy_rows(const float* src, int64_t rows, int N, float* dst, int64_t ld) {
    const int64_t r = blockIdx.x;
    for (int j = threadIdx.x; j < ld; j += blockDim.x) dst[r * ld + j] = j < N ? src[r * N + j] : 0.f;
}

// ---- rescue pass behind the resident kernel -----------------------------------------------------------------------------
// One workgroup per problem looks at the potentials the resident kernel left.  All finite (every call of an ordinary
// network): return - the pass costs one launch of B idle workgroups.  Otherwise (a scaling left fp32's range in the
// exponential domain, or an inter-workgroup wait gave up under contention) this workgroup re-solves ITS problem alone in
// the log domain, upstream's u = log_mu - LSE_j(C + v), v = log_nu - LSE_i(C + u): no range limit, no inter-workgroup
// wait, scores streamed from L2 / HBM twice per iteration (milliseconds per problem - a rare path).  flags[3] counts the
// rescued problems; flags[1] the problems whose potentials are non-finite even so (non-finite scores: a real error,
// reported by e2emv_sync).
__global__ __launch_bounds__(1024) void sinkhorn_rescue(SkParams p, int iters, unsigned* flags) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int M = p.M, N = p.N;
    float* ub = p.u + (int64_t)b * (M + 1);
    float* vb = p.v + (int64_t)b * p.ldV;
    bool bad = false, gave_up = false;
    for (int i = tid; i <= M; i += 1024) { const float x = ub[i]; bad = bad || !(fabsf(x) < INFINITY); gave_up = gave_up || __float_as_uint(x) == SKR_GAVE_UP_NAN; }
    for (int j = tid; j <= N; j += 1024) { const float x = vb[j]; bad = bad || !(fabsf(x) < INFINITY); gave_up = gave_up || __float_as_uint(x) == SKR_GAVE_UP_NAN; }
    if (!__syncthreads_or(bad ? 1 : 0)) return;
    const int timed_out = __syncthreads_or(gave_up ? 1 : 0);  // THIS problem's reason (the launch-global flag says nothing about it)
    float* su = lds;            // [M + 1]
    float* sv = lds + (M + 1);  // [N + 1]
    const float* Sb = p.S + (int64_t)b * M * p.ldS;
    for (int j = tid; j <= N; j += 1024) sv[j] = 0.f;
    __syncthreads();
    const float log_mu_bin = __logf((float)N) + p.norm, log_nu_bin = __logf((float)M) + p.norm;
    for (int it = 0; it < iters; ++it) {
        for (int i = wave; i <= M; i += 16) {  // one wave per row
            float mx = -INFINITY;
            for (int j = lane; j <= N; j += 64) mx = fmaxf(mx, ((i < M && j < N) ? Sb[(int64_t)i * p.ldS + j] : p.alpha) + sv[j]);
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
            float sm = 0.f;
            for (int j = lane; j <= N; j += 64) sm += __expf(((i < M && j < N) ? Sb[(int64_t)i * p.ldS + j] : p.alpha) + sv[j] - mx);
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) sm += __shfl_xor(sm, o);
            if (lane == 0) su[i] = (i < M ? p.norm : log_mu_bin) - (mx + __logf(sm));
        }
        __syncthreads();
        for (int j = tid; j <= N; j += 1024) {  // one thread per column, running maximum
            float mx = -INFINITY, sm = 0.f;
            for (int i = 0; i <= M; ++i) {
                const float x = ((i < M && j < N) ? Sb[(int64_t)i * p.ldS + j] : p.alpha) + su[i];
                if (x > mx) { sm = sm * __expf(mx - x) + 1.f; mx = x; } else { sm += __expf(x - mx); }
            }
            sv[j] = (j < N ? p.norm : log_nu_bin) - (mx + __logf(sm));
        }
        __syncthreads();
    }
    if (iters <= 0) {
        for (int i = tid; i <= M; i += 1024) su[i] = 0.f;
        __syncthreads();
    }
    bad = false;
    for (int i = tid; i <= M; i += 1024) { ub[i] = su[i]; bad = bad || !(fabsf(su[i]) < INFINITY); }
    for (int j = tid; j < p.ldV; j += 1024) {
        const float x = j <= N ? sv[j] : 0.f;
        vb[j] = x;
        bad = bad || !(fabsf(x) < INFINITY);
    }
    const int still = __syncthreads_or(bad ? 1 : 0);
    // [1] non-finite even in the log domain (non-finite scores: an error); otherwise rescued - [6] when a wait of the resident
    // kernel gave up on THIS problem (contention: says nothing about the model), [3] when not (a scaling left fp32's range)
    if (tid == 0) atomicAdd(flags + (still ? 1 : (timed_out ? 6 : 3)), 1u);
}

// streaming chain: the potentials of a problem with non-finite scores are non-finite - counted like the resident path's
// (flags[1], reported by e2emv_sync / check_finite)
__global__ __launch_bounds__(256) void sinkhorn_check_finite(SkParams p, unsigned* flags) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const float* ub = p.u + (int64_t)b * (p.M + 1);
    const float* vb = p.v + (int64_t)b * p.ldV;
    bool bad = false;
    for (int i = tid; i <= p.M; i += 256) bad = bad || !(fabsf(ub[i]) < INFINITY);
    for (int j = tid; j <= p.N; j += 256) bad = bad || !(fabsf(vb[j]) < INFINITY);
    if (__syncthreads_or(bad ? 1 : 0) && tid == 0) atomicAdd(flags + 1, 1u);
}

template <int KT>
static void launch_sweeps(const SkParams& p, int B, bool final, hipStream_t s) {
    const size_t lds = sizeof(float) * 8 * KT * 256;
    const bool full = p.N == p.ldS && p.N == KT * 256;
    if (!final) {
        if (full) hipLaunchKernelGGL((sinkhorn_sweep<KT, false, true>), dim3(p.chunks, B), dim3(256), lds, s, p);
        else hipLaunchKernelGGL((sinkhorn_sweep<KT, false, false>), dim3(p.chunks, B), dim3(256), lds, s, p);
    } else {
        if (full) hipLaunchKernelGGL((sinkhorn_sweep<KT, true, true>), dim3(p.chunks + 1, B), dim3(256), lds, s, p);
        else hipLaunchKernelGGL((sinkhorn_sweep<KT, true, false>), dim3(p.chunks + 1, B), dim3(256), lds, s, p);
    }
}

static void sweep(const SkParams& p, int B, bool final, hipStream_t s) {
    switch (KT_of(p.ldS)) {
        case 1: launch_sweeps<1>(p, B, final, s); break;
        case 2: launch_sweeps<2>(p, B, final, s); break;
        case 4: launch_sweeps<4>(p, B, final, s); break;
        default: launch_sweeps<8>(p, B, final, s); break;
    }
}

void sk_pad_copy_rows(const float* src, int64_t rows, int N, float* dst, int64_t ld, hipStream_t s) {
    hipLaunchKernelGGL(pad_copy_rows, dim3((unsigned)rows), dim3(256), 0, s, src, rows, N, dst, ld);
}

void sk_stream_iterate(SkParams& p, int B, int iters, hipStream_t s) {
    hipLaunchKernelGGL(sinkhorn_init, dim3(B), dim3(256), 0, s, p, B);
    if (iters <= 0) hipLaunchKernelGGL(sinkhorn_zero_u, dim3(B), dim3(256), 0, s, p);
    for (int it = 0; it < iters; ++it) {
        sweep(p, B, false, s);
        hipLaunchKernelGGL(sinkhorn_combine, dim3((unsigned)((p.ldV + 63) / 64), B), dim3(256), 0, s, p);
        std::swap(p.v, p.v_next);
    }
}

void sk_check_finite(const SkParams& p, int B, unsigned* flags, hipStream_t s) {
    hipLaunchKernelGGL(sinkhorn_check_finite, dim3(B), dim3(256), 0, s, p, flags);
}

void sk_rescue(const SkParams& p, int B, int iters, unsigned* flags, hipStream_t s) {
    hipLaunchKernelGGL(sinkhorn_rescue, dim3(B), dim3(1024), sizeof(float) * (size_t)(p.M + p.N + 2), s, p, iters, flags);
}

void sk_final_sweep(const SkParams& p, int B, hipStream_t s) { sweep(p, B, true, s); }

void sk_match(const SkParams& p, int B, float match_thr, const SinkhornOut& out, hipStream_t s) {
    MatchParams mp{};
    mp.M = p.M; mp.N = p.N; mp.chunks = p.chunks; mp.ldS = p.ldS;
    mp.max0 = p.max0; mp.idx0 = p.idx0; mp.pv = p.pv; mp.pi = p.pi; mp.idx1_in = nullptr;
    mp.thr = match_thr;
    mp.group_batch = p.group_batch;
    for (int g = 0; g < out.n_groups; ++g) {
        mp.m0[g] = out.m0[g]; mp.m1[g] = out.m1[g]; mp.ms0[g] = out.ms0[g]; mp.ms1[g] = out.ms1[g];
    }
    hipLaunchKernelGGL(match_finalize, dim3(B), dim3(MF_THREADS), sizeof(int) * (2 * p.M + p.N), s, mp);
}

}  // namespace e2emv

using namespace e2emv;

extern "C" int e2emv_extract_matches(e2emv_ctx* ctx, int B, int M, int N, const float* d_logZ, float match_threshold,
                                     int64_t* d_matches0, int64_t* d_matches1, float* d_mscores0, float* d_mscores1,
                                     void* stream) {
    if (!ctx || !d_logZ) return E2EMV_EINVAL;
    E2EMV_ENTER(ctx, stream);
    if (B <= 0 || M <= 0 || N <= 0) return set_err(ctx, E2EMV_ESHAPE, "extract_matches: bad sizes");
    if ((size_t)(2 * M + N) * 4 > 60000) return set_err(ctx, E2EMV_ESHAPE, "extract_matches: too many keypoints");
    hipStream_t s = (hipStream_t)stream;
    auto al = [](size_t n) { return (n * 4 + 255) & ~size_t(255); };
    int rc = ws_reserve(ctx, 2 * al((size_t)B * M) + al((size_t)B * N));
    if (rc) return rc;
    char* w = ctx->d_ws;
    float* max0 = (float*)w; w += al((size_t)B * M);
    int* idx0 = (int*)w; w += al((size_t)B * M);
    int* idx1 = (int*)w;
    prof_begin(ctx, PS_MATCH, s);
    hipLaunchKernelGGL(dense_row_argmax, dim3((M + 3) / 4, B), dim3(256), 0, s, d_logZ, M, N, max0, idx0);
    hipLaunchKernelGGL(dense_col_argmax, dim3((N + 255) / 256, B), dim3(256), 0, s, d_logZ, M, N, idx1);
    MatchParams mp{};
    mp.M = M; mp.N = N; mp.chunks = 0; mp.ldS = 0;
    mp.max0 = max0; mp.idx0 = idx0; mp.idx1_in = idx1; mp.thr = match_threshold;
    mp.group_batch = B;
    mp.m0[0] = d_matches0; mp.m1[0] = d_matches1; mp.ms0[0] = d_mscores0; mp.ms1[0] = d_mscores1;
    hipLaunchKernelGGL(match_finalize, dim3(B), dim3(MF_THREADS), sizeof(int) * (2 * M + N), s, mp);
    prof_end(ctx, s);
    E2EMV_CHECK_LAUNCH(ctx, "extract_matches kernels");
    return E2EMV_OK;
}
