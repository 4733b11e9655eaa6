// Sinkhorn, resident kernels with K in registers addressed by number: sinkhorn_resident128 (<= 1024 columns, 128 rows per
// workgroup) and sinkhorn_resident2k (<= 2048 columns, 64 rows per workgroup).  The row passes are different algorithms on
// purpose; the exchange between a problem's workgroups is the one of sinkhorn_exchange.h.  The build keeps
// this file's device assembly and checks that the compiler stayed inside its register window (build.py: REGISTER_WINDOW).
// sinkhorn.hip gets an instance through sinkhorn_regs_kernel().
#include <utility>

#include "sinkhorn_internal.h"
#include "sinkhorn_exchange.h"

namespace e2emv {

// ---- 128 rows per workgroup: ALL problems of a 32-pair batch resident at once (round 5) -----------------------------------------
// sinkhorn_resident keeps 64 rows x 1024 columns per workgroup (one per CU) in registers: 16 problems of 1024 x 1024 fill the chip,
// a batch of 32 runs as two rounds of 100 iterations, and an iteration is bound by the exchange, not by the arithmetic.  Here a
// workgroup owns 128 rows - 8 workgroups per problem, 32 problems resident, ONE round - which needs 512 KB of couplings per CU,
// the size of the register file.  What makes it fit:
//   * FOUR waves per workgroup, one per SIMD: a wave then has 512 registers per lane (256 VGPRs + 256 AGPRs); 24 of its 32 rows live
//     there (384 values per lane - hipcc parks what does not fit the VGPRs in the accumulator file, one v_accvgpr_read per use),
//     8 rows in LDS (128 KB per workgroup);
//   * ONE pass over the couplings per iteration: a_i depends on row i's sum alone (rows are whole inside a wave), so a row's
//     column contribution K_ij a_i is accumulated right behind its row sum - no a[] array, no second sweep over K (the row
//     kernel's two half-iterations read K twice: twice the accumulator-file reads and LDS traffic here);
//   * the fold buffer holds the 4 waves' partial column sums (16 KB).
// Exchange, epochs, give-up protocol, rescue: the row kernel's (pair mode), with the lane mappings of 256 threads.  An iteration
// costs about twice the arithmetic per CU and the same two hops, for half as many rounds: chosen by the launcher when it saves
// rounds (more than 16 problems of 513 ... 1024 columns).
template <int... I, class F>
__device__ __forceinline__ void sk_static_for_impl(std::integer_sequence<int, I...>, F&& f) { (f(std::integral_constant<int, I>{}), ...); }
template <int N, class F>
__device__ __forceinline__ void sk_static_for(F&& f) { sk_static_for_impl(std::make_integer_sequence<int, N>{}, f); }
// rows of a wave: 12 in vector registers v64 .. v255, 12 in accumulation registers a64 .. a255, 8 in LDS
constexpr int SK128_RV = 12, SK128_RA = 12, SK128_RL = 8, SK128_RR = SK128_RV + SK128_RA, SK128_R0 = 64;
constexpr int sk128_base(int r) { return SK128_R0 + 16 * (r < SK128_RV ? r : r - SK128_RV); }
#include "sinkhorn128_rows.h"
// dynamic LDS of sinkhorn_resident128, in floats: what the kernel carves and the launch is sized from
struct Sk128Lds {
    static constexpr int W = 1024, RW = SK128_RR + SK128_RL, ROWS = 4 * RW;
    static constexpr int klds = 0;                       // [4 waves][RL rows][W]: the LDS-resident rows of K
    static constexpr int fold = klds + 4 * SK128_RL * W; // [4][W] partial column sums
    static constexpr int vbuf = fold + 4 * W;            // [W + 4]: b of the current iteration (+ b_N at [W])
    static constexpr int red = vbuf + W + 4;             // [32]
    static constexpr int rks = red + 32;                 // [ROWS] r_i = exp(alpha - rowmax_i)
    static constexpr int mrs = rks + ROWS;               // [ROWS] rowmax_i
    static constexpr int asv = mrs + ROWS;               // [ROWS] a_i of the last iteration (for the potentials)
    static constexpr int total = asv + ROWS;
};
template <bool FULL>
__global__ __launch_bounds__(256, 1) __attribute__((amdgpu_num_vgpr(56))) void sinkhorn_resident128(SkResParams p) {
    using L = Sk128Lds;
    constexpr int KT = 4, W = L::W, RW = L::RW, ROWS = L::ROWS;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* klds = lds + L::klds, *fold = lds + L::fold, *vbuf = lds + L::vbuf, *red = lds + L::red;
    float* rks = lds + L::rks, *mrs = lds + L::mrs, *asv = lds + L::asv;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    int grp, w;
    u64* bufU2;
    float mu, muM, nuN;
    __amdgpu_buffer_rsrc_t rsA, rsB;
    exchange_setup(p, grp, w, bufU2, mu, muM, nuN, rsA, rsB);
    const int G = p.G, cs = p.cs, N = p.N, M = p.M;
    const int row0 = w * ROWS + wave * RW;
    bool dead = false;
    float* const kl = klds + wave * SK128_RL * W + 4 * lane;  // this lane's first chunk of the wave's LDS rows (chunk k: + 256 k)
    unsigned round = 0;
    for (int b = grp; b < p.B; b += p.n_res, ++round) {
        const unsigned ebase = round * (unsigned)p.iters;
        const float* Sb = p.S + (int64_t)b * M * p.ldS;
        // ---- load the wave's 32 rows, shift by the row maximum, exponentiate once; rows 24 - 31 go to LDS
        // 24 of the wave's 32 rows live in registers the compiler does not allocate: amdgpu_num_vgpr(56) confines it to v0 - v55
        // (and a0 - a55 as its spill space); v56 - v63 are the row pass's temporaries, v64 - v255 hold rows 0 - 11 and a64 - a255
        // rows 12 - 23, as [16 r + 4 k + e].  hipcc's allocator cannot keep 384 values in place for a whole call (it spills
        // exactly the long-lived ones: profiles/r5_sinkhorn_blocks.log), so these registers are written (v_mov / v_accvgpr_write,
        // once per problem) and read (the row pass in sinkhorn128_rows.h, twice per iteration) by number.  The clobber sizes the
        // wave's allocation at 256 + 256 registers; tests/test_host_and_abi.py disassembles the kernel and checks that nothing
        // outside these statements touches a register above v55 / a55.
        asm volatile("" ::: "v255", "a255");
        sk_static_for<RW>([&](auto r_c) {
            constexpr int r = decltype(r_c)::value;
            const int row = FULL ? row0 + r : min(row0 + r, M - 1);
            f32x4 zz[KT];
            float mx = p.alpha;
#pragma unroll
            for (int k = 0; k < KT; ++k) {
                const int c = 4 * (lane + 64 * k);
                zz[k] = (FULL || c < p.ldS) ? *reinterpret_cast<const f32x4*>(Sb + (int64_t)row * p.ldS + c) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (FULL || c + e < N) mx = fmaxf(mx, zz[k][e]);
            }
            mx = wave_max_dpp(mx);
            const bool rvalid = FULL || row0 + r < M;
            if (lane == 0) {
                mrs[wave * RW + r] = mx;
                rks[wave * RW + r] = rvalid ? exp_accurate(p.alpha - mx) : 0.f;
            }
            sk_static_for<KT>([&](auto k_c) {
                constexpr int k = decltype(k_c)::value;
                const int c = 4 * (lane + 64 * k);
                f32x4 kv;
#pragma unroll
                for (int e = 0; e < 4; ++e) kv[e] = (rvalid && (FULL || c + e < N)) ? exp_accurate(zz[k][e] - mx) : 0.f;
                if constexpr (r < SK128_RV) {
                    const float k0 = kv[0], k1 = kv[1], k2 = kv[2], k3 = kv[3];
                    asm volatile("v_mov_b32 v[%4], %0\n\tv_mov_b32 v[%4+1], %1\n\tv_mov_b32 v[%4+2], %2\n\tv_mov_b32 v[%4+3], %3"
                                 :: "v"(k0), "v"(k1), "v"(k2), "v"(k3), "n"(sk128_base(r) + 4 * k));
                } else if constexpr (r < SK128_RR) {
                    const float k0 = kv[0], k1 = kv[1], k2 = kv[2], k3 = kv[3];
                    asm volatile("v_accvgpr_write_b32 a[%4], %0\n\tv_accvgpr_write_b32 a[%4+1], %1\n\tv_accvgpr_write_b32 a[%4+2], %2\n\tv_accvgpr_write_b32 a[%4+3], %3"
                                 :: "v"(k0), "v"(k1), "v"(k2), "v"(k3), "n"(sk128_base(r) + 4 * k));
                } else {
                    *reinterpret_cast<f32x4*>(kl + (r - SK128_RR) * W + 256 * k) = kv;
                }
            });
            if (r & 1) __builtin_amdgcn_sched_barrier(0);  // two rows in flight
        });
        for (int c = tid; c < W + 4; c += 256) vbuf[c] = (c < N || c == W) ? 1.f : 0.f;
        __syncthreads();
        float bN = 1.f, aM = 0.f;

        for (int it = 0; it < p.iters; ++it) {
            const unsigned epoch = ebase + (unsigned)it + 1u;
            int tq = tid;
            asm volatile("" : "+v"(tq));
            u64* const bufU = bufU2 + (epoch & 1u) * (unsigned)G;
            const bool last = it + 1 == p.iters;
            // ---- the wave's 32 rows in three phases, so that no latency-bound chain stands between two streams of multiply-adds:
            //   (1) row sums of all rows (asm), four rows folded into one register by two butterflies;
            //   (2) the 8 reductions over quads and rows and the 8 divisions - independent chains, interleaved by the compiler;
            //   (3) column sums of all rows (asm) with the a_i as scalars.  LDS rows are read in both (1) and (3).
            f32x2 cl[KT], ch[KT];  // partial column sums of this lane's 16 columns (pairs 0 - 1 | 2 - 3 of each chunk)
            float ra = 0.f;         // sum of r_i a_i over the wave's rows (dustbin column)
            {
                const unsigned kl_a = (unsigned)(uintptr_t)(__attribute__((address_space(3))) float*)kl;
                float t4[RW / 4];   // group g: lane l holds the sum of row 4 g + (l & 3) over the lane's quad
                {
                    f32x2 blo[KT], bhi[KT];
                    f32x2 accb = {0.f, 0.f};
#pragma unroll
                    for (int k = 0; k < KT; ++k) {
                        const f32x4 b4 = *reinterpret_cast<const f32x4*>(vbuf + 4 * (lane + 64 * k));  // 0 beyond N
                        blo[k] = f32x2{b4[0], b4[1]};
                        bhi[k] = f32x2{b4[2], b4[3]};
                        accb += blo[k] + bhi[k];
                    }
                    aM = muM / (wave_sum_dpp(accb[0] + accb[1]) + bN);
                    // every asm statement of the register rows also fetches ONE LDS row, consumed right behind it (the LDS latency
                    // hides under the statement's multiply-adds): rows 0 - 2 with the vector-register groups, 3 - 7 with the first five
                    // pair statements of the accumulation-register groups
                    float x[SK128_RL];
                    auto lds_row_sum = [&](const f32x4 (&t)[4], int j) __attribute__((always_inline)) {
                        f32x2 acc = {0.f, 0.f};
#pragma unroll
                        for (int k = 0; k < KT; ++k) {
                            acc = __builtin_elementwise_fma(f32x2{t[k][0], t[k][1]}, blo[k], acc);
                            acc = __builtin_elementwise_fma(f32x2{t[k][2], t[k][3]}, bhi[k], acc);
                        }
                        x[j] = acc[0] + acc[1];
                        asm volatile("" : "+v"(x[j]));
                    };
                    sk_static_for<SK128_RR / 4>([&](auto g_c) {
                        constexpr int g = decltype(g_c)::value, r0 = 4 * g;
                        constexpr int B0 = sk128_base(r0), B1 = sk128_base(r0 + 1), B2 = sk128_base(r0 + 2), B3 = sk128_base(r0 + 3);
                        f32x2 acc[4];
                        f32x4 t[4];
                        if constexpr (r0 < SK128_RV) {
                            sk128_rs4v_l<B0, B1, B2, B3, g * W * 4>(acc, blo, bhi, t, kl_a);
                            lds_row_sum(t, g);
                        } else {
                            constexpr int j0 = SK128_RV / 4 + 2 * (g - SK128_RV / 4);  // LDS rows of this group's two pair statements
                            sk128_rs2a_l<B0, B1, j0 * W * 4>(acc[0], acc[1], blo, bhi, t, kl_a);
                            lds_row_sum(t, j0);
                            if constexpr (j0 + 1 < SK128_RL) {
                                sk128_rs2a_l<B2, B3, (j0 + 1) * W * 4>(acc[2], acc[3], blo, bhi, t, kl_a);
                                lds_row_sum(t, j0 + 1);
                            } else {
                                sk128_rs2a<B2, B3>(acc[2], acc[3], blo, bhi);
                            }
                        }
                        t4[g] = wave_sum4_quads(acc[0][0] + acc[0][1], acc[1][0] + acc[1][1], acc[2][0] + acc[2][1], acc[3][0] + acc[3][1], lane);
                        asm volatile("" : "+v"(t4[g]));
                    });
                    static_assert(SK128_RV / 4 + 2 * (SK128_RA / 4) - 1 >= SK128_RL, "an asm statement per LDS row");
                    t4[SK128_RR / 4] = wave_sum4_quads(x[0], x[1], x[2], x[3], lane);
                    t4[SK128_RR / 4 + 1] = wave_sum4_quads(x[4], x[5], x[6], x[7], lane);
                }
                // (2) a_i of four rows per division; the scalars for phase 3; the dustbin statistic sum_i r_i a_i per lane class
                float as[RW];
                float ra4 = 0.f;
                int l3 = lane & 3;
                asm volatile("" : "+v"(l3));  // (per iteration: the 8 LDS addresses below are otherwise hoisted out of the loop and spilled)
#pragma unroll
                for (int g = 0; g < RW / 4; ++g) {
                    const float s_r = wave_sum4_rows(t4[g]);
                    const int rl = wave * RW + 4 * g + l3;
                    const float rk = rks[rl];
                    const float ar = (FULL || row0 + 4 * g + l3 < M) ? mu / fmaf(rk, bN, s_r) : 0.f;
                    ra4 = fmaf(rk, ar, ra4);
                    if (last) asv[rl] = ar;  // for the potentials (16 lanes write the same value to the same word)
#pragma unroll
                    for (int q = 0; q < 4; ++q) as[4 * g + q] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(ar), q));
                }
                ra = (__int_as_float(__builtin_amdgcn_readlane(__float_as_int(ra4), 0)) + __int_as_float(__builtin_amdgcn_readlane(__float_as_int(ra4), 1)))
                     + (__int_as_float(__builtin_amdgcn_readlane(__float_as_int(ra4), 2)) + __int_as_float(__builtin_amdgcn_readlane(__float_as_int(ra4), 3)));
                // (3)
#pragma unroll
                for (int k = 0; k < KT; ++k) { cl[k] = f32x2{0.f, 0.f}; ch[k] = f32x2{0.f, 0.f}; }
                sk_static_for<SK128_RR / 4>([&](auto g_c) {
                    constexpr int r0 = 4 * decltype(g_c)::value;
                    constexpr int B0 = sk128_base(r0), B1 = sk128_base(r0 + 1), B2 = sk128_base(r0 + 2), B3 = sk128_base(r0 + 3);
                    const f32x2 a2[4] = {f32x2{as[r0], as[r0]}, f32x2{as[r0 + 1], as[r0 + 1]}, f32x2{as[r0 + 2], as[r0 + 2]}, f32x2{as[r0 + 3], as[r0 + 3]}};
                    if constexpr (r0 < SK128_RV) sk128_rc4v<B0, B1, B2, B3>(cl, ch, a2);
                    else sk128_rc4a<B0, B1, B2, B3>(cl, ch, a2);
                });
                sk_static_for<SK128_RL / 2>([&](auto g_c) {  // LDS rows again, two per statement (32 registers: b is dead by now)
                    constexpr int r = 2 * decltype(g_c)::value;
                    f32x4 t0, t1, t2, t3, t4_, t5, t6, t7;
                    asm volatile("ds_read_b128 %0, %8 offset:%9\n\tds_read_b128 %1, %8 offset:%9+1024\n\t"
                                 "ds_read_b128 %2, %8 offset:%9+2048\n\tds_read_b128 %3, %8 offset:%9+3072\n\t"
                                 "ds_read_b128 %4, %8 offset:%9+4096\n\tds_read_b128 %5, %8 offset:%9+4096+1024\n\t"
                                 "ds_read_b128 %6, %8 offset:%9+4096+2048\n\tds_read_b128 %7, %8 offset:%9+4096+3072\n\ts_waitcnt lgkmcnt(0)"
                                 : "=&v"(t0), "=&v"(t1), "=&v"(t2), "=&v"(t3), "=&v"(t4_), "=&v"(t5), "=&v"(t6), "=&v"(t7) : "v"(kl_a), "n"(r * W * 4));
                    const f32x4 t[2][KT] = {{t0, t1, t2, t3}, {t4_, t5, t6, t7}};
#pragma unroll
                    for (int j = 0; j < 2; ++j) {
                        const f32x2 a2 = {as[SK128_RR + r + j], as[SK128_RR + r + j]};
#pragma unroll
                        for (int k = 0; k < KT; ++k) {
                            cl[k] = __builtin_elementwise_fma(f32x2{t[j][k][0], t[j][k][1]}, a2, cl[k]);
                            ch[k] = __builtin_elementwise_fma(f32x2{t[j][k][2], t[j][k][3]}, a2, ch[k]);
                        }
                    }
                    // (here, not sunk to the end of the pass with the rows kept in scratch until then)
                    asm volatile("" : "+v"(cl[0]), "+v"(cl[1]), "+v"(cl[2]), "+v"(cl[3]), "+v"(ch[0]), "+v"(ch[1]), "+v"(ch[2]), "+v"(ch[3]));
                });
            }
            // ---- the 4 waves' partial column sums -> LDS
            {
                float* lf = fold + wave * W + 4 * lane;
#pragma unroll
                for (int k = 0; k < KT; ++k) *reinterpret_cast<f32x4*>(lf + 256 * k) = f32x4{cl[k][0], cl[k][1], ch[k][0], ch[k][1]};
                if (lane == 0) red[wave] = ra;
                __syncthreads();
            }
            // ---- publish the workgroup's partial column sums (stage A, 16-byte pairs: 4 adjacent columns per thread) and its dustbin sum
            {
                const int c = 4 * tq;
                const f32x4 t0 = *reinterpret_cast<const f32x4*>(fold + c), t1 = *reinterpret_cast<const f32x4*>(fold + W + c);
                const f32x4 t2 = *reinterpret_cast<const f32x4*>(fold + 2 * W + c), t3 = *reinterpret_cast<const f32x4*>(fold + 3 * W + c);
                const f32x4 T = (t0 + t1) + (t2 + t3);
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const int cc = c + 2 * h, wc = cc / cs, jl = cc - wc * cs;
                    if (FULL || cc < N) granule_store2(rsA, (unsigned)((wc * G + w) * cs + jl) * 8u, epoch, T[2 * h], T[2 * h + 1]);
                }
                if (tq == 0) {
                    const float U = (red[0] + red[1]) + (red[2] + red[3]);
                    granule_store(bufU + w, epoch, U);
                }
            }
            // ---- the exchange (sinkhorn_exchange.h): stage A consume + stage B publish, b_N, stage B consume
            exchange_consume_a<256, 4>(rsA, rsB, tq, w, G, cs, N, epoch, mu, aM, p.timeout, dead);
            exchange_bn(bufU, wave, lane, G, epoch, nuN, aM, vbuf + W, p.timeout, dead);
            static_assert(W == 2 * 256 * 2, "one pass");
            exchange_consume_b<256, 2>(rsB, vbuf, W, tq, N, epoch, p.timeout, dead);
            if (__syncthreads_or(dead ? 1 : 0)) dead = true;
            bN = vbuf[W];
        }

        store_potentials<ROWS>(p, b, w, tid, asv, mrs, vbuf, bN, aM, dead);
    }
}


// ---- the same construction for 1025 .. 2048 columns: 64 rows per workgroup ---------------------------------------------------
// A row of K is 32 registers per lane here ([32 r + 16 h + 4 k + e]: h = the column half, chunk 4 h + k covers columns
// 4 (lane + 64 (4 h + k)) .. + 3).  A wave holds 16 rows: 6 in v64 .. v255, 6 in a64 .. a255, 4 in LDS (128 KB for the
// workgroup), so a problem of 2048 rows is 32 workgroups (64 with the 32-row workgroups of sinkhorn_resident<8>) and eight
// problems are resident instead of four.  The compiler's 56 registers cannot hold b (32) and the column partials (32) at once:
//   * row sums: per column half - b of the half (16 registers), the rows in pairs (sk_rs2v / sk128_rs2a, LDS rows through 16
//     registers), each row's partial sum added into ONE register per row;
//   * four 4-way reductions, a_i of four rows per division (as in sinkhorn_resident128);
//   * column sums: per half 16 registers of partials, both halves kept (b is dead by then) until the fold;
//   * the fold of the 4 waves goes through 16 KB (LDS is full): waves 2 and 3 write, waves 0 and 1 add theirs and write
//     back, then all threads publish fold[0] + fold[1].
constexpr int SK2K_RV = 6, SK2K_RA = 6, SK2K_RL = 4, SK2K_RR = SK2K_RV + SK2K_RA, SK2K_RW = SK2K_RR + SK2K_RL;
constexpr int sk2k_base(int r, int h) { return 64 + 32 * (r < SK2K_RV ? r : r - SK2K_RV) + 16 * h; }
struct Sk2kLds {  // dynamic LDS of sinkhorn_resident2k, in floats
    static constexpr int W = 2048, RW = SK2K_RW, ROWS = 4 * RW;
    static constexpr int klds = 0;                       // [4 waves][RL rows][W]: the LDS-resident rows of K
    static constexpr int fold = klds + 4 * SK2K_RL * W;  // [2][W] partial column sums
    static constexpr int vbuf = fold + 2 * W;            // [W + 4]: b of the current iteration (+ b_N at [W])
    static constexpr int red = vbuf + W + 4;             // [32]
    static constexpr int rks = red + 32;                 // [ROWS] r_i = exp(alpha - rowmax_i)
    static constexpr int mrs = rks + ROWS;               // [ROWS] rowmax_i
    static constexpr int asv = mrs + ROWS;               // [ROWS] a_i of the last iteration (for the potentials)
    static constexpr int total = asv + ROWS;
};
template <bool FULL>
__global__ __launch_bounds__(256, 1) __attribute__((amdgpu_num_vgpr(56))) void sinkhorn_resident2k(SkResParams p) {
    using L = Sk2kLds;
    constexpr int W = L::W, RW = L::RW, ROWS = L::ROWS;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* klds = lds + L::klds, *fold = lds + L::fold, *vbuf = lds + L::vbuf, *red = lds + L::red;
    float* rks = lds + L::rks, *mrs = lds + L::mrs, *asv = lds + L::asv;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    int grp, w;
    u64* bufU2;
    float mu, muM, nuN;
    __amdgpu_buffer_rsrc_t rsA, rsB;
    exchange_setup(p, grp, w, bufU2, mu, muM, nuN, rsA, rsB);
    const int G = p.G, cs = p.cs, N = p.N, M = p.M;
    const int row0 = w * ROWS + wave * RW;
    bool dead = false;
    float* const kl = klds + wave * SK2K_RL * W + 4 * lane;  // this lane's first chunk of the wave's LDS rows (chunk c: + 256 c)
    unsigned round = 0;
    for (int b = grp; b < p.B; b += p.n_res, ++round) {
        const unsigned ebase = round * (unsigned)p.iters;
        const float* Sb = p.S + (int64_t)b * M * p.ldS;
        asm volatile("" ::: "v255", "a255");  // (the wave is allocated 256 + 256 registers: see sinkhorn_resident128)
        // ---- load the wave's 16 rows, shift by the row maximum, exponentiate once
        sk_static_for<RW>([&](auto r_c) {
            constexpr int r = decltype(r_c)::value;
            const int row = FULL ? row0 + r : min(row0 + r, M - 1);
            f32x4 zz[8];
            float mx = p.alpha;
#pragma unroll
            for (int c8 = 0; c8 < 8; ++c8) {
                const int c = 4 * (lane + 64 * c8);
                zz[c8] = (FULL || c < p.ldS) ? *reinterpret_cast<const f32x4*>(Sb + (int64_t)row * p.ldS + c) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (FULL || c + e < N) mx = fmaxf(mx, zz[c8][e]);
            }
            mx = wave_max_dpp(mx);
            const bool rvalid = FULL || row0 + r < M;
            if (lane == 0) {
                mrs[wave * RW + r] = mx;
                rks[wave * RW + r] = rvalid ? exp_accurate(p.alpha - mx) : 0.f;
            }
            sk_static_for<8>([&](auto c_c) {
                constexpr int c8 = decltype(c_c)::value, h = c8 >> 2, k = c8 & 3;
                const int c = 4 * (lane + 64 * c8);
                f32x4 kv;
#pragma unroll
                for (int e = 0; e < 4; ++e) kv[e] = (rvalid && (FULL || c + e < N)) ? exp_accurate(zz[c8][e] - mx) : 0.f;
                if constexpr (r < SK2K_RV) {
                    const float k0 = kv[0], k1 = kv[1], k2 = kv[2], k3 = kv[3];
                    asm volatile("v_mov_b32 v[%4], %0\n\tv_mov_b32 v[%4+1], %1\n\tv_mov_b32 v[%4+2], %2\n\tv_mov_b32 v[%4+3], %3"
                                 :: "v"(k0), "v"(k1), "v"(k2), "v"(k3), "n"(sk2k_base(r, h) + 4 * k));
                } else if constexpr (r < SK2K_RR) {
                    const float k0 = kv[0], k1 = kv[1], k2 = kv[2], k3 = kv[3];
                    asm volatile("v_accvgpr_write_b32 a[%4], %0\n\tv_accvgpr_write_b32 a[%4+1], %1\n\tv_accvgpr_write_b32 a[%4+2], %2\n\tv_accvgpr_write_b32 a[%4+3], %3"
                                 :: "v"(k0), "v"(k1), "v"(k2), "v"(k3), "n"(sk2k_base(r, h) + 4 * k));
                } else {
                    *reinterpret_cast<f32x4*>(kl + (r - SK2K_RR) * W + 256 * c8) = kv;
                }
            });
            __builtin_amdgcn_sched_barrier(0);  // one row in flight
        });
        for (int c = tid; c < W + 4; c += 256) vbuf[c] = (c < N || c == W) ? 1.f : 0.f;
        __syncthreads();
        float bN = 1.f, aM = 0.f;
        const unsigned kl_a = (unsigned)(uintptr_t)(__attribute__((address_space(3))) float*)kl;

        for (int it = 0; it < p.iters; ++it) {
            const unsigned epoch = ebase + (unsigned)it + 1u;
            int tq = tid;
            asm volatile("" : "+v"(tq));
            u64* const bufU = bufU2 + (epoch & 1u) * (unsigned)G;
            const bool last = it + 1 == p.iters;
            // ---- row sums, per column half: one register per row
            float accp[RW];
#pragma unroll
            for (int r = 0; r < RW; ++r) accp[r] = 0.f;
            f32x2 accb = {0.f, 0.f};
            sk_static_for<2>([&](auto h_c) {
                constexpr int h = decltype(h_c)::value;
                f32x2 blo[4], bhi[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const f32x4 b4 = *reinterpret_cast<const f32x4*>(vbuf + 4 * (lane + 64 * (4 * h + k)));  // 0 beyond N
                    blo[k] = f32x2{b4[0], b4[1]};
                    bhi[k] = f32x2{b4[2], b4[3]};
                    accb += blo[k] + bhi[k];
                }
                // register rows in pairs; the first four pair statements also fetch one LDS row (half) each, consumed right behind them
                auto lds_row_sum = [&](const f32x4 (&t)[4], int j) __attribute__((always_inline)) {
                    f32x2 acc = {0.f, 0.f};
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        acc = __builtin_elementwise_fma(f32x2{t[k][0], t[k][1]}, blo[k], acc);
                        acc = __builtin_elementwise_fma(f32x2{t[k][2], t[k][3]}, bhi[k], acc);
                    }
                    accp[SK2K_RR + j] += acc[0] + acc[1];
                    asm volatile("" : "+v"(accp[SK2K_RR + j]));
                };
                sk_static_for<SK2K_RV / 2>([&](auto p_c) {
                    constexpr int pp = decltype(p_c)::value, r0 = 2 * pp;
                    f32x2 acc[4];
                    f32x4 t[4];
                    sk_rs2v_l<sk2k_base(r0, h), sk2k_base(r0 + 1, h), (pp * W + 1024 * h) * 4>(acc, blo, bhi, t, kl_a);
                    accp[r0] += (acc[0][0] + acc[0][1]) + (acc[2][0] + acc[2][1]);
                    accp[r0 + 1] += (acc[1][0] + acc[1][1]) + (acc[3][0] + acc[3][1]);
                    asm volatile("" : "+v"(accp[r0]), "+v"(accp[r0 + 1]));
                    lds_row_sum(t, pp);
                });
                sk_static_for<SK2K_RA / 2>([&](auto p_c) {
                    constexpr int pp = decltype(p_c)::value, r0 = SK2K_RV + 2 * pp;
                    f32x2 a0, a1;
                    if constexpr (SK2K_RV / 2 + pp < SK2K_RL) {
                        f32x4 t[4];
                        sk128_rs2a_l<sk2k_base(r0, h), sk2k_base(r0 + 1, h), ((SK2K_RV / 2 + pp) * W + 1024 * h) * 4>(a0, a1, blo, bhi, t, kl_a);
                        lds_row_sum(t, SK2K_RV / 2 + pp);
                    } else {
                        sk128_rs2a<sk2k_base(r0, h), sk2k_base(r0 + 1, h)>(a0, a1, blo, bhi);
                    }
                    accp[r0] += a0[0] + a0[1];
                    accp[r0 + 1] += a1[0] + a1[1];
                    asm volatile("" : "+v"(accp[r0]), "+v"(accp[r0 + 1]));
                });
            });
            aM = muM / (wave_sum_dpp(accb[0] + accb[1]) + bN);
            // ---- a_i: four rows per reduction and division; the scalars a_i for the column sums
            float as[RW];
            float ra4 = 0.f;
#pragma unroll
            for (int g = 0; g < RW / 4; ++g) {
                const float s_r = wave_sum4_dpp(accp[4 * g], accp[4 * g + 1], accp[4 * g + 2], accp[4 * g + 3], lane);
                const int rl = wave * RW + 4 * g + (lane & 3);
                const float rk = rks[rl];
                const float ar = (FULL || row0 + 4 * g + (lane & 3) < M) ? mu / fmaf(rk, bN, s_r) : 0.f;
                ra4 = fmaf(rk, ar, ra4);
                if (last) asv[rl] = ar;
#pragma unroll
                for (int q = 0; q < 4; ++q) as[4 * g + q] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(ar), q));
            }
            const float ra = (__int_as_float(__builtin_amdgcn_readlane(__float_as_int(ra4), 0)) + __int_as_float(__builtin_amdgcn_readlane(__float_as_int(ra4), 1)))
                             + (__int_as_float(__builtin_amdgcn_readlane(__float_as_int(ra4), 2)) + __int_as_float(__builtin_amdgcn_readlane(__float_as_int(ra4), 3)));
            // ---- column sums, per half; both halves stay in registers until the fold
            f32x2 cl[2][4], ch[2][4];
            sk_static_for<2>([&](auto h_c) {
                constexpr int h = decltype(h_c)::value;
#pragma unroll
                for (int k = 0; k < 4; ++k) { cl[h][k] = f32x2{0.f, 0.f}; ch[h][k] = f32x2{0.f, 0.f}; }
                auto lds_row_cols = [&](const f32x4 (&t)[4], int j) __attribute__((always_inline)) {
                    const f32x2 a2 = {as[SK2K_RR + j], as[SK2K_RR + j]};
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        cl[h][k] = __builtin_elementwise_fma(f32x2{t[k][0], t[k][1]}, a2, cl[h][k]);
                        ch[h][k] = __builtin_elementwise_fma(f32x2{t[k][2], t[k][3]}, a2, ch[h][k]);
                    }
                    asm volatile("" : "+v"(cl[h][0]), "+v"(cl[h][1]), "+v"(cl[h][2]), "+v"(cl[h][3]), "+v"(ch[h][0]), "+v"(ch[h][1]), "+v"(ch[h][2]), "+v"(ch[h][3]));
                };
                sk_static_for<SK2K_RV / 2>([&](auto p_c) {
                    constexpr int pp = decltype(p_c)::value, r0 = 2 * pp;
                    f32x4 t[4];
                    sk_rc2v_l<sk2k_base(r0, h), sk2k_base(r0 + 1, h), (pp * W + 1024 * h) * 4>(cl[h], ch[h], f32x2{as[r0], as[r0]}, f32x2{as[r0 + 1], as[r0 + 1]}, t, kl_a);
                    lds_row_cols(t, pp);
                });
                sk_static_for<SK2K_RA / 2>([&](auto p_c) {
                    constexpr int pp = decltype(p_c)::value, r0 = SK2K_RV + 2 * pp;
                    if constexpr (SK2K_RV / 2 + pp < SK2K_RL) {
                        f32x4 t[4];
                        sk_rc2a_l<sk2k_base(r0, h), sk2k_base(r0 + 1, h), ((SK2K_RV / 2 + pp) * W + 1024 * h) * 4>(cl[h], ch[h], f32x2{as[r0], as[r0]}, f32x2{as[r0 + 1], as[r0 + 1]}, t, kl_a);
                        lds_row_cols(t, SK2K_RV / 2 + pp);
                    } else {
                        sk_rc2a<sk2k_base(r0, h), sk2k_base(r0 + 1, h)>(cl[h], ch[h], f32x2{as[r0], as[r0]}, f32x2{as[r0 + 1], as[r0 + 1]});
                    }
                });
            });
            // ---- fold of the 4 waves through 16 KB: waves 2, 3 write; waves 0, 1 add theirs and write back
            {
                float* lf = fold + (wave & 1) * W + 4 * lane;
                if (wave >= 2) {
#pragma unroll
                    for (int h = 0; h < 2; ++h)
#pragma unroll
                        for (int k = 0; k < 4; ++k) *reinterpret_cast<f32x4*>(lf + 256 * (4 * h + k)) = f32x4{cl[h][k][0], cl[h][k][1], ch[h][k][0], ch[h][k][1]};
                }
                if (lane == 0) red[wave] = ra;
                __syncthreads();
                if (wave < 2) {
#pragma unroll
                    for (int h = 0; h < 2; ++h)
#pragma unroll
                        for (int k = 0; k < 4; ++k) {
                            const f32x4 o = *reinterpret_cast<const f32x4*>(lf + 256 * (4 * h + k));
                            *reinterpret_cast<f32x4*>(lf + 256 * (4 * h + k)) = f32x4{cl[h][k][0] + o[0], cl[h][k][1] + o[1], ch[h][k][0] + o[2], ch[h][k][1] + o[3]};
                        }
                }
                __syncthreads();
            }
            // ---- publish the workgroup's partial column sums (stage A, 16-byte pairs: 8 adjacent columns per thread) and its dustbin sum
            {
                const int c = 8 * tq;
#pragma unroll
                for (int q4 = 0; q4 < 2; ++q4) {
                    const f32x4 T = *reinterpret_cast<const f32x4*>(fold + c + 4 * q4) + *reinterpret_cast<const f32x4*>(fold + W + c + 4 * q4);
#pragma unroll
                    for (int hh = 0; hh < 2; ++hh) {
                        const int cc = c + 4 * q4 + 2 * hh, wc = cc / cs, jl = cc - wc * cs;
                        if (FULL || cc < N) granule_store2(rsA, (unsigned)((wc * G + w) * cs + jl) * 8u, epoch, T[2 * hh], T[2 * hh + 1]);
                    }
                }
                if (tq == 0) {
                    const float U = (red[0] + red[1]) + (red[2] + red[3]);
                    granule_store(bufU + w, epoch, U);
                }
            }
            // ---- the exchange (sinkhorn_exchange.h): stage A consume + stage B publish, b_N, stage B consume
            // (8 lanes per column pair, each two producers per wait; four per wait - all 32 producers in one round trip - was
            // slower: 4.1 against 2.9 us for this stage, the polls themselves load the memory system)
            exchange_consume_a<256, 8>(rsA, rsB, tq, w, G, cs, N, epoch, mu, aM, p.timeout, dead);
            exchange_bn(bufU, wave, lane, G, epoch, nuN, aM, vbuf + W, p.timeout, dead);
            static_assert(W == 2 * 256 * 4, "one pass");
            exchange_consume_b<256, 4>(rsB, vbuf, W, tq, N, epoch, p.timeout, dead);
            if (__syncthreads_or(dead ? 1 : 0)) dead = true;
            bN = vbuf[W];
        }

        store_potentials<ROWS>(p, b, w, tid, asv, mrs, vbuf, bN, aM, dead);
    }
}

SkKernel sinkhorn_regs_kernel(int KT, bool full) {
    SkKernel k;
    if (KT == 4) {
        k.fn = full ? (const void*)sinkhorn_resident128<true> : (const void*)sinkhorn_resident128<false>;
        k.rows = Sk128Lds::ROWS; k.lds = sizeof(float) * (size_t)Sk128Lds::total;
    } else {
        k.fn = full ? (const void*)sinkhorn_resident2k<true> : (const void*)sinkhorn_resident2k<false>;
        k.rows = Sk2kLds::ROWS; k.lds = sizeof(float) * (size_t)Sk2kLds::total;
    }
    k.threads = 256; k.big = true;
    return k;
}

}  // namespace e2emv
