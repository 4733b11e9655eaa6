// Sinkhorn, resident kernel with K in compiler-allocated registers: sinkhorn_resident<KT, FULL, PAIR, RW>, 8 waves, 32 / 64 rows
// per workgroup, all iterations in one launch (the protocol: sinkhorn_exchange.h; the kernels with 128 / 64 rows per workgroup
// in registers addressed by number: sinkhorn_regs.hip).  sinkhorn.hip gets an instance through sinkhorn_resident_kernel().
#include "sinkhorn_internal.h"
#include "sinkhorn_exchange.h"

namespace e2emv {

// dynamic LDS of sinkhorn_resident<KT, ...>, in floats: what the kernel carves and the launch is sized from
template <int KT>
struct SkResidentLds {
    static constexpr int W = KT * 256;          // padded column count held by a wave
    static constexpr int fold = 0;              // [8 waves][W] partial column sums
    static constexpr int vbuf = fold + 8 * W;   // [W + 4]: b of the current iteration (+ b_N at [W])
    static constexpr int red = vbuf + W + 4;    // [32] small reductions
    static constexpr int total = red + 32;
};

template <int KT, bool FULL, bool PAIR = false, int RW = 4>
__global__ __launch_bounds__(512, (KT <= 4 && RW == 4) ? 4 : 2) void sinkhorn_resident(SkResParams p) {
    using L = SkResidentLds<KT>;
    constexpr int W = L::W;                           // padded column count held by a wave
    // RW rows per wave: 64 matrix values per lane at RW = 4 (KT <= 4: two workgroups per
                                                      // CU), 128 at KT = 8 (one per CU - half as many workgroups exchange)
    constexpr int ROWS = 8 * RW;                      // rows per workgroup
    constexpr int CPT = (W + 511) / 512;              // columns a thread folds / publishes
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* fold = lds + L::fold, *vbuf = lds + L::vbuf, *red = lds + L::red;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // scalar: LDS bases and row numbers stay out of the VGPRs
    const int grp = blockIdx.x / p.G, w = blockIdx.x % p.G;
    const int G = p.G, cs = p.cs, N = p.N, M = p.M;
    const int row0 = w * ROWS + wave * RW;
    u64* const bufA = p.bufA + (int64_t)grp * G * G * cs;
    u64* const bufB = p.bufB + (int64_t)grp * G * cs;
    u64* const bufU2 = p.bufU + (int64_t)grp * 2 * G;  // [epoch parity][G]
    bool dead = false;
    int col[KT];
#pragma unroll
    for (int k = 0; k < KT; ++k) col[k] = 4 * (lane + 64 * k);
    // marginals in the linear domain (log_mu = norm, log_mu_M = log N + norm, ...; norm = -log(M + N))
    const float mu = 1.0f / (float)(M + N), muM = (float)N / (float)(M + N), nuN = (float)M / (float)(M + N);
    // stage-A destination of the columns this thread folds: consumer region wc = c / cs, producer slot w, column jl
    int dstA[CPT];
#pragma unroll
    for (int i = 0; i < CPT; ++i) {
        const int c = tid + 512 * i, wc = c / cs, jl = c - wc * cs;
        dstA[i] = (wc * G + w) * cs + jl;
    }
    // pair mode: a thread owns CPT ADJACENT columns and every granule travels as half of a 16-byte pair (needs an even
    // column slice per consumer so that a pair never straddles two consumer regions)
    // (PAIR is chosen by the launcher: KT >= 4 and cs even)
    constexpr bool pair = PAIR && (CPT % 2 == 0);
    const __amdgpu_buffer_rsrc_t rsA = __builtin_amdgcn_make_buffer_rsrc(bufA, 0, G * G * cs * 8, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsB = __builtin_amdgcn_make_buffer_rsrc(bufB, 0, G * cs * 8, 0x00020000);
    unsigned round = 0;
    for (int b = grp; b < p.B; b += p.n_res, ++round) {
        const unsigned ebase = round * (unsigned)p.iters;  // epochs run on without a gap: their parity alternates
        const float* Sb = p.S + (int64_t)b * M * p.ldS;
        // ---- load the 4 rows of this wave, shift by the row maximum, exponentiate once
        f32x2 K[RW][KT][2];
        float mrow[RW], rK[RW];
#pragma unroll
        for (int r = 0; r < RW; ++r) {
            const int row = min(row0 + r, M - 1);
            float zz[KT][4];
            float mx = p.alpha;
#pragma unroll
            for (int k = 0; k < KT; ++k) {
                const f32x4 t = (FULL || col[k] < p.ldS) ? *reinterpret_cast<const f32x4*>(Sb + (int64_t)row * p.ldS + col[k])
                                                         : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    zz[k][e] = t[e];
                    if (FULL || col[k] + e < N) mx = fmaxf(mx, t[e]);
                }
            }
            mx = wave_max_dpp(mx);
            const bool rvalid = row0 + r < M;  // ragged tail: the row does not exist -> K = 0, a = 0
            mrow[r] = mx;
            rK[r] = rvalid ? exp_accurate(p.alpha - mx) : 0.f;
#pragma unroll
            for (int k = 0; k < KT; ++k)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float kv = (rvalid && (FULL || col[k] + e < N)) ? exp_accurate(zz[k][e] - mx) : 0.f;
                    K[r][k][e >> 1][e & 1] = kv;
                }
        }
        // b = exp(v) = 1, b_N = 1 (v starts at 0)
        for (int c = tid; c < W + 4; c += 512) vbuf[c] = (c < N || c == W) ? 1.f : 0.f;
        __syncthreads();
        float bN = 1.f, aM = 0.f;
        float a[RW];
#pragma unroll
        for (int r = 0; r < RW; ++r) a[r] = 0.f;

        for (int it = 0; it < p.iters; ++it) {
            const unsigned epoch = ebase + (unsigned)it + 1u;
            // the thread index, made opaque once per iteration: the exchange addresses below are then recomputed (a few
            // integer ops) instead of being hoisted out of the loop as dozens of 64-bit loop invariants that would spill
            int tq = tid;
            asm volatile("" : "+v"(tq));
            u64* const bufU = bufU2 + (epoch & 1u) * (unsigned)G;
            // ---- row half-iteration: a_i = mu / (sum_j K_ij b_j + r_i b_N) for the wave's 4 rows; a_M from sum_j b_j
            {
                f32x2 acc[RW], accb = {0.f, 0.f};
#pragma unroll
                for (int r = 0; r < RW; ++r) acc[r] = f32x2{0.f, 0.f};
#pragma unroll
                for (int k = 0; k < KT; ++k) {
                    const f32x4 b4 = *reinterpret_cast<const f32x4*>(vbuf + col[k]);  // 0 beyond N
                    const f32x2 blo = {b4[0], b4[1]}, bhi = {b4[2], b4[3]};
                    accb += blo + bhi;
#pragma unroll
                    for (int r = 0; r < RW; ++r) {
                        acc[r] = __builtin_elementwise_fma(K[r][k][0], blo, acc[r]);
                        acc[r] = __builtin_elementwise_fma(K[r][k][1], bhi, acc[r]);
                    }
                }
                // four row sums per reduction, arriving in lanes (l & 3): ONE division gives the a_i of four rows, read back as scalars
                static_assert(RW % 4 == 0, "rows of a wave in groups of four");
#pragma unroll
                for (int g = 0; g < RW / 4; ++g) {
                    const float s4 = wave_sum4_dpp(acc[4 * g][0] + acc[4 * g][1], acc[4 * g + 1][0] + acc[4 * g + 1][1],
                                                   acc[4 * g + 2][0] + acc[4 * g + 2][1], acc[4 * g + 3][0] + acc[4 * g + 3][1], lane);
                    const int q = lane & 3;
                    const float rk = q == 0 ? rK[4 * g] : (q == 1 ? rK[4 * g + 1] : (q == 2 ? rK[4 * g + 2] : rK[4 * g + 3]));
                    const float a4 = (row0 + 4 * g + q < M) ? mu / fmaf(rk, bN, s4) : 0.f;
#pragma unroll
                    for (int qq = 0; qq < 4; ++qq) a[4 * g + qq] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(a4), qq));
                }
                aM = muM / (wave_sum_dpp(accb[0] + accb[1]) + bN);
            }
            // ---- column half-iteration, this wave's part: sum over its 4 rows of K_ij a_i -> LDS
            {
                float* lf = fold + wave * W;
#pragma unroll
                for (int k = 0; k < KT; ++k) {
                    f32x2 lo = K[0][k][0] * f32x2{a[0], a[0]}, hi = K[0][k][1] * f32x2{a[0], a[0]};
#pragma unroll
                    for (int r = 1; r < RW; ++r) {
                        lo = __builtin_elementwise_fma(K[r][k][0], f32x2{a[r], a[r]}, lo);
                        hi = __builtin_elementwise_fma(K[r][k][1], f32x2{a[r], a[r]}, hi);
                    }
                    *reinterpret_cast<f32x4*>(lf + col[k]) = f32x4{lo[0], lo[1], hi[0], hi[1]};
                }
                float ra = rK[0] * a[0];
#pragma unroll
                for (int r = 1; r < RW; ++r) ra = fmaf(rK[r], a[r], ra);
                if (lane == 0) red[wave] = ra;  // dustbin column
            }
            __syncthreads();
            // ---- fold the 8 waves, publish the workgroup's partial column sums (stage A) and its dustbin-column sum
            if constexpr (pair) {
                float fT[CPT];
#pragma unroll
                for (int i = 0; i < CPT; ++i) {
                    const int c = CPT * tq + i;
                    float T = fold[c];
#pragma unroll
                    for (int wv = 1; wv < 8; ++wv) T += fold[wv * W + c];
                    fT[i] = T;  // (columns >= N hold zeros: K is zero there)
                }
#pragma unroll
                for (int i = 0; i < CPT; i += 2) {
                    const int c = CPT * tq + i, wc = c / cs, jl = c - wc * cs;
                    if (FULL || c < N) granule_store2(rsA, (unsigned)((wc * G + w) * cs + jl) * 8u, epoch, fT[i], fT[i + 1]);
                }
                if (tq == 0) {
                    float U = red[0];
                    for (int wv = 1; wv < 8; ++wv) U += red[wv];
                    granule_store(bufU + w, epoch, U);
                }
            } else {
                float fT[CPT];
#pragma unroll
                for (int i = 0; i < CPT; ++i) {
                    const int c = tq + 512 * i;
                    fT[i] = 0.f;
                    if (c < W && (FULL || c < N)) {
                        float T = fold[c];
#pragma unroll
                        for (int wv = 1; wv < 8; ++wv) T += fold[wv * W + c];
                        fT[i] = T;
                    }
                }
#pragma unroll
                for (int i = 0; i < CPT; ++i) {  // all stores after all LDS work: nothing waits behind a write-through store
                    const int c = tq + 512 * i;
                    if (c < W && (FULL || c < N)) granule_store(bufA + dstA[i], epoch, fT[i]);
                }
                if (tq == 0) {
                    float U = red[0];
                    for (int wv = 1; wv < 8; ++wv) U += red[wv];
                    granule_store(bufU + w, epoch, U);
                }
            }
            // ---- stage A consume: my slice of columns over all producers -> b_j = nu / (sum + a_M), published as stage B
            if constexpr (pair) {
                exchange_consume_a<512, 16>(rsA, rsB, tq, w, G, cs, N, epoch, mu, aM, p.timeout, dead);
            } else {
                const int q = tq & 15, cg = tq >> 4;
                const u64* base = bufA + (int64_t)w * G * cs;  // my consumer region: [producer][cs]
                for (int j0 = 0; j0 < cs; j0 += 32) {
                    const int jl = j0 + cg, c = w * cs + jl;
                    const bool act = jl < cs && c < N;
                    float T = 0.f;
                    for (int g0 = 0; g0 < G; g0 += 64) {  // wave-uniform trip count
                        int off[4];
                        unsigned val[4];
                        int n = 0;
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            const int g = g0 + q + 16 * i;
                            off[i] = 0;
                            if (act && g < G) { off[i] = g * cs + jl; n = i + 1; }
                        }
                        granule_wait<4>(base, off, n, epoch, val, p.timeout, dead);
#pragma unroll
                        for (int i = 0; i < 4; ++i)
                            if (i < n) T += __uint_as_float(val[i]);
                    }
#pragma unroll
                    for (int o = 8; o > 0; o >>= 1) T += __shfl_xor(T, o);
                    if (act && q == 0) granule_store(bufB + c, epoch, mu / (T + aM));  // nu_j = mu
                }
            }
            // ---- b_N = nu_N / (sum_i r_i a_i + a_M) from the G workgroup sums (wave 0)
            exchange_bn(bufU, wave, lane, G, epoch, nuN, aM, vbuf + W, p.timeout, dead);
            // ---- stage B consume: all of b into LDS
            if constexpr (pair) {
                static_assert(W % 1024 == 0, "whole passes of 512 threads x one pair");
                exchange_consume_b<512, 1>(rsB, vbuf, W, tq, N, epoch, p.timeout, dead);
            } else
            for (int c0 = 0; c0 < W; c0 += 1024) {  // wave-uniform trip count
                const int ca = c0 + tq, cb = c0 + 512 + tq;
                int off[2] = {ca < N ? ca : 0, cb < N ? cb : 0};
                unsigned val[2];
                granule_wait<2>(bufB, off, cb < N ? 2 : (ca < N ? 1 : 0), epoch, val, p.timeout, dead);
                if (ca < W) vbuf[ca] = ca < N ? __uint_as_float(val[0]) : 0.f;
                if (cb < W) vbuf[cb] = cb < N ? __uint_as_float(val[1]) : 0.f;
            }
            if (__syncthreads_or(dead ? 1 : 0)) dead = true;
            bN = vbuf[W];
        }

        // ---- hand the potentials to the final sweep (logZ, fused arg-max): u = log a - m of this workgroup's rows, and
        // from workgroup 0 the dustbin-row potential and v = log b.  A scaling that left fp32's range (zero, infinite,
        // NaN) or a give-up in the exchange is counted in the sticky error word; its NaN / inf reaches the outputs.
        {
            // (a give-up marks ITS problem with a NaN of its own payload: the rescue pass books the problem as a timeout - contention,
            // says nothing about the model - only when it finds that mark; a scaling that left fp32's range yields inf / the default NaN)
            const float qnan = __uint_as_float(SKR_GAVE_UP_NAN);
            float* ub = p.u + (int64_t)b * (M + 1);
            bool bad = false;
#pragma unroll
            for (int r = 0; r < RW; ++r)
                if (row0 + r < M) {
                    bad = bad || !(a[r] > 0.f) || !(a[r] < INFINITY);
                    if (lane == 0) ub[row0 + r] = dead ? qnan : __logf(a[r]) - mrow[r];
                }
            if (w == 0) {
                float* vb = p.v + (int64_t)b * p.ldV;
                for (int j = tid; j < p.ldV; j += 512) {
                    const float bj = j < N ? vbuf[j] : (j == N ? bN : 1.f);
                    bad = bad || !(bj > 0.f) || !(bj < INFINITY);
                    vb[j] = dead ? qnan : __logf(bj);
                }
                bad = bad || !(aM > 0.f) || !(aM < INFINITY);
                if (tid == 0) ub[M] = dead ? qnan : __logf(aM) - p.alpha;
            }
            if (__syncthreads_or(bad ? 1 : 0) && tid == 0) atomicAdd(p.timeout + 4, 1u);  // also: LDS is reused by the next problem
        }
    }
}

template <int KT, int RW>
static SkKernel resident_instance(bool full, bool pairs) {
    SkKernel k;
    k.fn = full ? (const void*)sinkhorn_resident<KT, true, false, RW> : (const void*)sinkhorn_resident<KT, false, false, RW>;
    if constexpr (KT >= 4)  // (pair mode needs an even number of columns per thread)
        if (pairs) k.fn = full ? (const void*)sinkhorn_resident<KT, true, true, RW> : (const void*)sinkhorn_resident<KT, false, true, RW>;
    k.rows = 8 * RW; k.threads = 512;
    k.lds = sizeof(float) * (size_t)SkResidentLds<KT>::total;
    return k;
}

SkKernel sinkhorn_resident_kernel(int KT, bool full, bool pairs) {
    switch (KT) {  // (RW as skr_rw: 8 rows per wave at KT == 4)
        case 1: return resident_instance<1, 4>(full, false);
        case 2: return resident_instance<2, 4>(full, false);
        case 4: return resident_instance<4, 8>(full, pairs);
        default: return resident_instance<8, 4>(full, pairs);
    }
}

}  // namespace e2emv
