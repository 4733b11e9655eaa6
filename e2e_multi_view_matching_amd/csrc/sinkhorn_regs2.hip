// Sinkhorn, resident kernel with K in registers addressed by number, two waves per SIMD: sinkhorn_resident128w (<= 1024 columns,
// 128 rows per workgroup).  The same 512 KB of couplings per CU as sinkhorn_resident128 (sinkhorn_regs.hip), held by EIGHT waves
// of 256 architectural registers each and no accumulation registers.  The exchange between a problem's workgroups
// is the one of sinkhorn_exchange.h at 512 threads.  The build keeps this file's device assembly and checks that the compiler
// stayed inside its register window and uses no scratch (build.py: REGISTER_WINDOW_W).  sinkhorn.hip gets an instance through
// sinkhorn_regs2_kernel().
#include <utility>

#include "sinkhorn_internal.h"
#include "sinkhorn_exchange.h"

namespace e2emv {

// One wave alone on a SIMD (sinkhorn_resident128: 4 waves of 256 + 256 registers) issues a vector instruction every 4 cycles at
// best and reads half of its rows through v_accvgpr_read; two waves per SIMD feed the vector pipe at its full rate.  Here a wave
// owns 16 rows: 12 in v64 .. v255 as [16 r + 4 k + e] (k = 256-column chunk, e = element of the lane's 4 adjacent columns), 4 in
// LDS (8 waves x 4 rows x 4 KB = 128 KB).  The compiler is confined to v0 .. v63: on gfx950 amdgpu_num_vgpr(n) budgets 2 n
// registers of the unified file and halves them only when accumulation registers are in use, so the attribute reads 32 (with 64
// hipcc allocates up to v127 - on top of the rows).  There is no accumulation-register spill space (256 registers per wave is the
// whole budget at two waves per SIMD), so whatever the compiler cannot hold in its window would go to scratch: the build refuses
// the file unless the private segment is empty.  Row pass: the three phases of
// sinkhorn_resident128 on the vector-register blocks of sinkhorn128_rows.h.  LDS has no room for 8 partial column vectors
// (128 + 32 + 4 KB > 160 KB): the fold goes through 16 KB as in sinkhorn_resident2k - waves 4 .. 7 write, waves 0 .. 3 add theirs
// and write back.
template <int... I, class F>
__device__ __forceinline__ void skw_static_for_impl(std::integer_sequence<int, I...>, F&& f) { (f(std::integral_constant<int, I>{}), ...); }
template <int N, class F>
__device__ __forceinline__ void skw_static_for(F&& f) { skw_static_for_impl(std::make_integer_sequence<int, N>{}, f); }
// rows of a wave: 12 in vector registers v64 .. v255, 4 in LDS
constexpr int SKW_RV = 12, SKW_RL = 4, SKW_RW = SKW_RV + SKW_RL, SKW_R0 = 64, SKW_WAVES = 8;
constexpr int skw_base(int r) { return SKW_R0 + 16 * r; }
#include "sinkhorn128_rows.h"
// dynamic LDS of sinkhorn_resident128w, in floats: what the kernel carves and the launch is sized from
struct Sk128wLds {
    static constexpr int W = 1024, RW = SKW_RW, ROWS = SKW_WAVES * RW;
    static constexpr int klds = 0;                               // [8 waves][RL rows][W]: the LDS-resident rows of K
    static constexpr int fold = klds + SKW_WAVES * SKW_RL * W;   // [4][W] partial column sums (of waves i and i + 4)
    static constexpr int vbuf = fold + 4 * W;                    // [W + 4]: b of the current iteration (+ b_N at [W])
    static constexpr int red = vbuf + W + 4;                     // [32]
    static constexpr int rks = red + 32;                         // [ROWS] r_i = exp(alpha - rowmax_i)
    static constexpr int mrs = rks + ROWS;                       // [ROWS] rowmax_i
    static constexpr int asv = mrs + ROWS;                       // [ROWS] a_i of the last iteration (for the potentials)
    static constexpr int total = asv + ROWS;
};
static_assert(Sk128wLds::ROWS == 128, "128 rows per workgroup");
static_assert(Sk128wLds::total * 4 <= 160 * 1024, "the LDS of a CU");
static_assert(SKW_R0 + 16 * SKW_RV == 256, "the register rows end at v255");

template <bool FULL, int LP>
__global__ __launch_bounds__(512, 1) __attribute__((amdgpu_num_vgpr(32))) void sinkhorn_resident128w(SkResParams p) {
    using L = Sk128wLds;
    constexpr int KT = 4, W = L::W, RW = L::RW, ROWS = L::ROWS;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* klds = lds + L::klds, *fold = lds + L::fold, *vbuf = lds + L::vbuf, *red = lds + L::red;
    float* rks = lds + L::rks, *mrs = lds + L::mrs, *asv = lds + L::asv;
    // (the launch is 512 x 1 x 1: said here, the workgroup-wide OR behind every iteration needs no y / z index - two registers of
    // the window held through the whole call otherwise)
    __builtin_assume(__builtin_amdgcn_workitem_id_y() == 0);
    __builtin_assume(__builtin_amdgcn_workitem_id_z() == 0);
    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    int grp, w;
    u64* bufU2;
    float mu, muM, nuN;
    __amdgpu_buffer_rsrc_t rsA, rsB;
    exchange_setup(p, grp, w, bufU2, mu, muM, nuN, rsA, rsB);
    const int G = p.G, cs = p.cs, N = p.N, M = p.M;
    const int row0_ = w * ROWS + wave * RW;
    bool dead = false;
    float* const klw = klds + wave * SKW_RL * W;  // the wave's LDS rows (a lane's chunk k: + 4 lane + 256 k)
    unsigned epoch = 0;  // runs on over the problems of this workgroup: round * iters + it + 1
    for (int b = grp; b < p.B; b += p.n_res) {
        const float* Sb = p.S + (int64_t)b * M * p.ldS;
        // (opaque once per problem: the 16 row offsets are scalar work of the load, not 32 scalar registers held through the call)
        int row0 = row0_;
        asm volatile("" : "+s"(row0));
        // ---- load the wave's 16 rows, shift by the row maximum, exponentiate once; rows 12 - 15 go to LDS
        // The clobber sizes the wave's allocation at 256 vector registers and no accumulation registers; v64 - v255 are written
        // (v_mov, once per problem) and read (the row pass, twice per iteration) by number.
        asm volatile("" ::: "v255");
        skw_static_for<RW>([&](auto r_c) {
            constexpr int r = decltype(r_c)::value;
            // (the lane index, made opaque once per row: column masks and addresses are then recomputed - a few integer operations -
            // instead of living through the whole call as loop invariants that the window of 64 registers cannot hold)
            int lane = tid & 63;
            asm volatile("" : "+v"(lane));
            float* const kl = klw + 4 * lane;
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
            skw_static_for<KT>([&](auto k_c) {
                constexpr int k = decltype(k_c)::value;
                const int c = 4 * (lane + 64 * k);
                f32x4 kv;
#pragma unroll
                for (int e = 0; e < 4; ++e) kv[e] = (rvalid && (FULL || c + e < N)) ? exp_accurate(zz[k][e] - mx) : 0.f;
                if constexpr (r < SKW_RV) {
                    const float k0 = kv[0], k1 = kv[1], k2 = kv[2], k3 = kv[3];
                    asm volatile("v_mov_b32 v[%4], %0\n\tv_mov_b32 v[%4+1], %1\n\tv_mov_b32 v[%4+2], %2\n\tv_mov_b32 v[%4+3], %3"
                                 :: "v"(k0), "v"(k1), "v"(k2), "v"(k3), "n"(skw_base(r) + 4 * k));
                } else {
                    *reinterpret_cast<f32x4*>(kl + (r - SKW_RV) * W + 256 * k) = kv;
                }
            });
            if (r & 1) __builtin_amdgcn_sched_barrier(0);  // two rows in flight
        });
        {
            int t0 = tid;
            asm volatile("" : "+v"(t0));
            for (int c = t0; c < W + 4; c += 512) vbuf[c] = (c < N || c == W) ? 1.f : 0.f;
        }
        __syncthreads();
        float bN = 1.f, aM = 0.f;

        for (int it = 0; it < p.iters; ++it) {
            ++epoch;
            int tq = tid;
            asm volatile("" : "+v"(tq));
            const int lane = tq & 63;
            float* const kl = klw + 4 * lane;
            u64* const bufU = bufU2 + (epoch & 1u) * (unsigned)G;
            const bool last = it + 1 == p.iters;
            // ---- the wave's 16 rows in the three phases of sinkhorn_resident128: (1) row sums of all rows, four rows folded into
            // one register by two butterflies; (2) the 4 reductions over quads and rows and the 4 divisions; (3) column sums of all
            // rows with the a_i as scalars.  Every LDS row is fetched inside a register-row statement, in (1) and in (3).
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
                    float x[SKW_RL];
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
                    // rows 0 - 7: two statements of four rows, LDS rows 0 and 1 behind them
                    skw_static_for<2>([&](auto g_c) {
                        constexpr int g = decltype(g_c)::value, r0 = 4 * g;
                        f32x2 acc[4];
                        f32x4 t[4];
                        sk128_rs4v_l<skw_base(r0), skw_base(r0 + 1), skw_base(r0 + 2), skw_base(r0 + 3), g * W * 4>(acc, blo, bhi, t, kl_a);
                        lds_row_sum(t, g);
                        t4[g] = wave_sum4_quads(acc[0][0] + acc[0][1], acc[1][0] + acc[1][1], acc[2][0] + acc[2][1], acc[3][0] + acc[3][1], lane);
                        asm volatile("" : "+v"(t4[g]));
                    });
                    // rows 8 - 11: two statements of two rows (four chains: the halves of a chunk apart), LDS rows 2 and 3
                    {
                        float s[4];
                        skw_static_for<2>([&](auto h_c) {
                            constexpr int h = decltype(h_c)::value, r0 = 8 + 2 * h;
                            f32x2 acc[4];
                            f32x4 t[4];
                            sk_rs2v_l<skw_base(r0), skw_base(r0 + 1), (2 + h) * W * 4>(acc, blo, bhi, t, kl_a);
                            lds_row_sum(t, 2 + h);
                            s[2 * h] = (acc[0][0] + acc[0][1]) + (acc[2][0] + acc[2][1]);
                            s[2 * h + 1] = (acc[1][0] + acc[1][1]) + (acc[3][0] + acc[3][1]);
                            asm volatile("" : "+v"(s[2 * h]), "+v"(s[2 * h + 1]));
                        });
                        t4[2] = wave_sum4_quads(s[0], s[1], s[2], s[3], lane);
                    }
                    t4[3] = wave_sum4_quads(x[0], x[1], x[2], x[3], lane);
                }
                // (2) a_i of four rows per division; the scalars for phase 3; the dustbin statistic sum_i r_i a_i per lane class
                float as[RW];
                float ra4 = 0.f;
                int l3 = lane & 3;
                asm volatile("" : "+v"(l3));  // (per iteration: the LDS addresses below are otherwise hoisted out of the loop)
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
                // (3) rows 0 - 7 in pairs, each statement with one LDS row consumed right behind it; rows 8 - 11 in one statement
#pragma unroll
                for (int k = 0; k < KT; ++k) { cl[k] = f32x2{0.f, 0.f}; ch[k] = f32x2{0.f, 0.f}; }
                skw_static_for<SKW_RL>([&](auto j_c) {
                    constexpr int j = decltype(j_c)::value, r0 = 2 * j;
                    f32x4 t[4];
                    sk_rc2v_l<skw_base(r0), skw_base(r0 + 1), j * W * 4>(cl, ch, f32x2{as[r0], as[r0]}, f32x2{as[r0 + 1], as[r0 + 1]}, t, kl_a);
                    const f32x2 a2 = {as[SKW_RV + j], as[SKW_RV + j]};
#pragma unroll
                    for (int k = 0; k < KT; ++k) {
                        cl[k] = __builtin_elementwise_fma(f32x2{t[k][0], t[k][1]}, a2, cl[k]);
                        ch[k] = __builtin_elementwise_fma(f32x2{t[k][2], t[k][3]}, a2, ch[k]);
                    }
                    asm volatile("" : "+v"(cl[0]), "+v"(cl[1]), "+v"(cl[2]), "+v"(cl[3]), "+v"(ch[0]), "+v"(ch[1]), "+v"(ch[2]), "+v"(ch[3]));
                });
                {
                    const f32x2 a2[4] = {f32x2{as[8], as[8]}, f32x2{as[9], as[9]}, f32x2{as[10], as[10]}, f32x2{as[11], as[11]}};
                    sk128_rc4v<skw_base(8), skw_base(9), skw_base(10), skw_base(11)>(cl, ch, a2);
                }
            }
            // ---- fold of the 8 waves through 16 KB: waves 4 - 7 write; waves 0 - 3 add theirs and write back
            {
                float* lf = fold + (wave & 3) * W + 4 * lane;
                if (wave >= 4) {
#pragma unroll
                    for (int k = 0; k < KT; ++k) *reinterpret_cast<f32x4*>(lf + 256 * k) = f32x4{cl[k][0], cl[k][1], ch[k][0], ch[k][1]};
                }
                if (lane == 0) red[wave] = ra;
                __syncthreads();
                if (wave < 4) {
#pragma unroll
                    for (int k = 0; k < KT; ++k) {
                        const f32x4 o = *reinterpret_cast<const f32x4*>(lf + 256 * k);
                        *reinterpret_cast<f32x4*>(lf + 256 * k) = f32x4{cl[k][0] + o[0], cl[k][1] + o[1], ch[k][0] + o[2], ch[k][1] + o[3]};
                    }
                }
                __syncthreads();
            }
            // ---- publish the workgroup's partial column sums (stage A, 16-byte pairs: 2 adjacent columns per thread) and its dustbin sum
            {
                const int c = 2 * tq, wc = c / cs, jl = c - wc * cs;
                const f32x2 T = (*reinterpret_cast<const f32x2*>(fold + c) + *reinterpret_cast<const f32x2*>(fold + W + c))
                                + (*reinterpret_cast<const f32x2*>(fold + 2 * W + c) + *reinterpret_cast<const f32x2*>(fold + 3 * W + c));
                if (FULL || c < N) granule_store2(rsA, (unsigned)((wc * G + w) * cs + jl) * 8u, epoch, T[0], T[1]);
                if (tq == 0) {
                    const float U = ((red[0] + red[1]) + (red[2] + red[3])) + ((red[4] + red[5]) + (red[6] + red[7]));
                    granule_store(bufU + w, epoch, U);
                }
            }
            // ---- the exchange (sinkhorn_exchange.h), at 512 threads as sinkhorn_resident<4> runs it: stage A consume (LP lanes per
            // column pair: chosen per problem shape, sinkhorn_regs2_kernel) + stage B publish, b_N, stage B consume
            exchange_consume_a<512, LP>(rsA, rsB, tq, w, G, cs, N, epoch, mu, aM, p.timeout, dead);
            exchange_bn(bufU, wave, lane, G, epoch, nuN, aM, vbuf + W, p.timeout, dead);
            static_assert(W == 2 * 512, "one pass");
            exchange_consume_b<512, 1>(rsB, vbuf, W, tq, N, epoch, p.timeout, dead);
            if (__syncthreads_or(dead ? 1 : 0)) dead = true;
            bN = vbuf[W];
        }

        // (the thread and problem indices, opaque once more: the addresses of the potentials are computed here, behind the iterations)
        int ts = tid, bs = b;
        asm volatile("" : "+v"(ts), "+s"(bs));
        store_potentials<ROWS>(p, bs, w, ts, asv, mrs, vbuf, bN, aM, dead);
    }
}

SkKernel sinkhorn_regs2_kernel(bool full, int G) {
    SkKernel k;
    // stage A: 8 lanes per column pair cover 128 columns per wait - one wait for the slice of a problem of 8 or more workgroups
    // (at most 1024 / 8 columns), one producer per lane up to 8 workgroups, two up to 16; a wider slice (fewer workgroups) is
    // covered in fewer waits by 4 lanes per pair (256 columns per wait).  Measured at 32 x 1024 x 1024 / 32 x 640 x 1020, ms per
    // call of 100 iterations: 16 lanes 0.765 / 0.885, 8 lanes 0.664 / 0.736, 4 lanes 0.694 / 0.691 (profiles/sinkhorn_rows128w.log)
    if (G >= 8) k.fn = full ? (const void*)sinkhorn_resident128w<true, 8> : (const void*)sinkhorn_resident128w<false, 8>;
    else k.fn = full ? (const void*)sinkhorn_resident128w<true, 4> : (const void*)sinkhorn_resident128w<false, 4>;
    k.rows = Sk128wLds::ROWS; k.lds = sizeof(float) * (size_t)Sk128wLds::total;
    k.threads = 512; k.big = true;
    return k;
}

}  // namespace e2emv
