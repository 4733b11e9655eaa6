// Feasibility probe for the successor of gemm_p2c: the K loop of a WAVE-PRIVATE row-block GEMM.
//
// gemm_p2 / gemm_p2c: 8 waves (two per SIMD) share a 256 x 256 tile, a K step takes ~3750 - 4000 cycles for 3072 of matrix pipe
// whether or not the waves meet at a barrier - the two instruction streams of a SIMD do not interleave without loss.
// The wave-private form: 4 waves per workgroup, ONE per SIMD (512 registers), a wave owns 32 rows and ALL 512 output columns of
// MLP0 (16 accumulator blocks of 32 x 32 = 256 accumulation registers), its activation fragments come straight from global memory
// (nobody else needs them), the weight slices of a K step (512 rows x 128 B = 64 KB) go through a two-slot LDS ring filled by
// LDS-direct loads that the matrix waves issue THEMSELVES, one per 6 MFMA slots.  What nobody knows without measuring: does that
// stream keep the matrix pipe busy?  This file is that measurement and nothing else: the f16x2 arithmetic of gemm_p2 (x = hi +
// 2^-11 lo', 2^s W = w_hi + w_lo, three products per block), M x 512 x 512, no epilogue but a checksum (full fp32 output with
// --check, compared with a host evaluation of the same planes).
//
//
// MFMA shape (round 7): every variant exists twice, SHAPE 32 = v_mfma_f32_32x32x16_f16 (the product's shape so far: 16 accumulator blocks
// of 16 registers, 96 MFMAs of 8 passes per K step) and SHAPE 16 = v_mfma_f32_16x16x32_f16 (the same 32 x 512 output tile per wave as 2 x 32
// blocks of 4 registers, 192 MFMAs of 4 passes per step, a lane's fragment = row lane & 15, 16-byte k-chunk lane >> 4: one instruction covers
// the 32 k of a step).  Same planes, same three products per block, same reads / multiplies / LDS-direct loads per step.  The default run
// alternates the two shapes in one process; --ablations prints the round-6 list of what each part of the stream costs
// (32x32x16, as profiles/r6_wp_gemm.log has it); --clock runs long dispatches of the full stream of each shape for a counter pass
// (GRBM_GUI_ACTIVE / 8 / wall = the clock the chip holds under that stream).
//
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 tools/wp_gemm.hip -o tools/wp_gemm.bin && ./tools/wp_gemm.bin [--check | --clock | --ablations]
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <type_traits>
#include <vector>

typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;
typedef __attribute__((ext_vector_type(4))) unsigned u32x4;

constexpr int N_OUT = 512, K_IN = 512, ROWS_WG = 128, BK = 32;
constexpr int SLICEB = N_OUT * 128;  // one K step of the weights: 512 rows x 128 B = 64 KB
constexpr int LDSB = 2 * SLICEB;

__device__ __forceinline__ void mfma_a(f32x16& c, f16x8 a, f16x8 b) {  // accumulator in the accumulation registers
    asm volatile("v_mfma_f32_32x32x16_f16 %0, %1, %2, %0" : "+a"(c) : "v"(a), "v"(b));
}
__device__ __forceinline__ void mfma_a0(f32x16& c, f16x8 a, f16x8 b) {
    asm volatile("v_mfma_f32_32x32x16_f16 %0, %1, %2, 0" : "=&a"(c) : "v"(a), "v"(b));
}
__device__ __forceinline__ void mfma16_a(f32x4& c, f16x8 a, f16x8 b) {
    asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, %0" : "+a"(c) : "v"(a), "v"(b));
}
__device__ __forceinline__ void mfma16_a0(f32x4& c, f16x8 a, f16x8 b) {
    asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, 0" : "=&a"(c) : "v"(a), "v"(b));
}
__device__ __forceinline__ unsigned pk_mul(unsigned x, unsigned k) {
    unsigned d;
    asm volatile("v_pk_mul_f16 %0, %1, %2" : "=v"(d) : "v"(x), "v"(k));
    return d;
}
__device__ __forceinline__ void glds16(__amdgpu_buffer_rsrc_t rsrc, char* dst, unsigned voffset, unsigned soffset) {
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (__attribute__((address_space(3))) void*)dst, 16, voffset, soffset, 0, 0);
}

template <int I, int N, class F>
__device__ __forceinline__ void static_for(F&& f) {
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        static_for<I + 1, N>(f);
    }
}

// MODE 0: checksum only; 1: full fp32 output C [M][512]
// ABL (timing only, wrong results): 1 no LDS-direct loads in the loop, 2 no multiplies, 4 no fragment reads in the loop, 8 no activation loads,
// 16 no end-of-step wait / barrier
template <int MODE, int ABL = 0>
__global__ __launch_bounds__(256, 1) void wp_mlp0_kernel(const uint16_t* A, const uint16_t* W, float* C, float* sums, int M, int blocks_per_wg, int k_reps) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, lh = lane >> 5;
    const unsigned lda_b = K_IN * 4, ldw_b = K_IN * 4;
    const __amdgpu_buffer_rsrc_t rsW = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t*>(W), 0, N_OUT * K_IN * 4, 0x00020000);
    // loader: a wave moves 128 weight rows of a K step: 16 LDS-direct loads of 8 rows x 128 B; lane -> (row lane >> 3, position lane & 7),
    // source chunk = position ^ ((row >> 1) & 7) (the swizzle of p2.h, applied on the source side)
    unsigned w_vo[2];  // rows 0-7 / 8-15 of a 16-row pair differ in the swizzle's bit 2 only: two offsets, the rest in the scalar offset
    {
        const unsigned r = lane >> 3, pos = lane & 7;
        w_vo[0] = r * ldw_b + ((pos ^ ((r >> 1) & 7)) * 16u);
        w_vo[1] = r * ldw_b + ((pos ^ (((r + 8) >> 1) & 7)) * 16u);
    }
    auto load_piece = [&](int slot, int kt, int i) __attribute__((always_inline)) {  // piece i = 0..15 of this wave's 128 rows
        const unsigned row0 = 128u * (unsigned)wave + 8u * (unsigned)i;
        glds16(rsW, smem + slot * SLICEB + row0 * 128, w_vo[i & 1], row0 * ldw_b + (unsigned)kt * 128u);
    };
    // fragment addresses: W row block j (32 rows), lane row l31, chunk c = 4 plane + 2 ks + lh at position c ^ ((l31 >> 1) & 7)
    const unsigned lds0 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) char*)smem;
    const unsigned swz = (l31 >> 1) & 7;
    unsigned fa[2][2];  // [plane][ks]
#pragma unroll
    for (int pl = 0; pl < 2; ++pl)
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) fa[pl][ks] = lds0 + (unsigned)(l31 * 128) + (((unsigned)(4 * pl + 2 * ks + lh) ^ swz) << 4);
    typedef __attribute__((address_space(3))) const f16x8* lds_frag_t;
    auto wfrag = [&](int slot, int j, int pl, int ks) __attribute__((always_inline)) {
        return *reinterpret_cast<lds_frag_t>((uintptr_t)(fa[pl][ks] + (unsigned)(slot * SLICEB + j * 32 * 128)));
    };
    unsigned k2048 = 0x10001000u;
    asm volatile("" : "+v"(k2048));

    for (int blk = 0; blk < blocks_per_wg; ++blk) {
        const int row_base = (blockIdx.x * blocks_per_wg + blk) * ROWS_WG + wave * 32;
        if (row_base >= M) break;
        const char* xrow = reinterpret_cast<const char*>(A) + (size_t)(row_base + l31) * lda_b + lh * 16;
        f32x16 acc[16];
        f16x8 xf[2][2][2];  // [buffer][plane][ks]: the activation fragments of a K step, straight from global memory
        auto load_x = [&](int b, int kt) __attribute__((always_inline)) {
#pragma unroll
            for (int pl = 0; pl < 2; ++pl)
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) xf[b][pl][ks] = *reinterpret_cast<const f16x8*>(xrow + kt * 128 + pl * 64 + ks * 32);
        };
        constexpr int NK = K_IN / BK;
        // prologue: slice 0 into slot 0, the fragments of step 0
#pragma unroll
        for (int i = 0; i < 16; ++i) load_piece(0, 0, i);
        load_x(0, 0);
        if (ABL & 8) load_x(1, 0);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
        auto step = [&](auto FIRST, auto SLOT, int kt) __attribute__((always_inline)) {
            constexpr bool first = decltype(FIRST)::value;
            constexpr int slot = decltype(SLOT)::value;  // (compile-time: the fragment buffers are registers)
            // one stream: 96 MFMAs (2 k-halves x 16 weight blocks x 3 products); behind them, slot by slot: the next block's two
            // fragment reads + the four multiplies that make 2^-11 w_hi, one LDS-direct load of the NEXT slice every 6th slot, the
            // next step's activation fragments in the first slots
            f16x8 wh[3], wl[3];  // the fragments of blocks g, g + 1, g + 2: read TWO blocks (6 MFMA slots) ahead of their use
            wl[0] = wfrag(slot, 0, 1, 0);
            wh[0] = wfrag(slot, 0, 0, 0);
            wl[1] = wfrag(slot, 1, 1, 0);
            wh[1] = wfrag(slot, 1, 0, 0);
            if (ABL & 4) { wl[2] = wl[0]; wh[2] = wh[1]; }
            const bool more = kt + 1 < NK;
            __builtin_amdgcn_sched_barrier(0);
            // blocks in PAIRS (j, j + 1), their products alternating: no MFMA reads the accumulator the MFMA right before it wrote
            static_for<0, 16>([&](auto GG) __attribute__((always_inline)) {
                constexpr int gg = decltype(GG)::value, g0 = 2 * gg, ks = g0 >> 4, j = g0 & 15, p0 = g0 % 3, p1 = (g0 + 1) % 3;
                const u32x4 whu0 = __builtin_bit_cast(u32x4, wh[p0]), whu1 = __builtin_bit_cast(u32x4, wh[p1]);
                u32x4 w2u0, w2u1;
                // slots 0, 1: x_hi w_lo of both blocks; the multiplies
                if constexpr (first && ks == 0) mfma_a0(acc[j], wl[p0], xf[slot][0][ks]); else mfma_a(acc[j], wl[p0], xf[slot][0][ks]);
#pragma unroll
                for (int e = 0; e < 4; ++e) w2u0[e] = (ABL & 2) ? whu0[e] : pk_mul(whu0[e], k2048);
                __builtin_amdgcn_sched_barrier(0);
                if constexpr (first && ks == 0) mfma_a0(acc[j + 1], wl[p1], xf[slot][0][ks]); else mfma_a(acc[j + 1], wl[p1], xf[slot][0][ks]);
#pragma unroll
                for (int e = 0; e < 4; ++e) w2u1[e] = (ABL & 2) ? whu1[e] : pk_mul(whu1[e], k2048);
                __builtin_amdgcn_sched_barrier(0);
                // slots 2, 3: x_lo' (2^-11 w_hi); a piece of the next slice behind each (16 pieces over the first 8 pairs), the next step's
                // activation fragments behind pair 0
                mfma_a(acc[j], __builtin_bit_cast(f16x8, w2u0), xf[slot][1][ks]);
                if constexpr (gg < 8 && !(ABL & 1)) { if (more) load_piece(slot ^ 1, kt + 1, 2 * gg); }
                if constexpr (gg == 0 && !(ABL & 8)) { if (more) load_x(slot ^ 1, kt + 1); }
                __builtin_amdgcn_sched_barrier(0);
                mfma_a(acc[j + 1], __builtin_bit_cast(f16x8, w2u1), xf[slot][1][ks]);
                if constexpr (gg < 8 && !(ABL & 1)) { if (more) load_piece(slot ^ 1, kt + 1, 2 * gg + 1); }
                __builtin_amdgcn_sched_barrier(0);
                // slots 4, 5: x_hi w_hi; then the fragments of the pair after next go into the buffers this pair's high planes leave... (two
                // blocks ahead: buffers (g0 + 2) % 3 = the one block g0 - 1 used, and - behind slot 5 - (g0 + 3) % 3 = p0)
                mfma_a(acc[j], wh[p0], xf[slot][0][ks]);
                if constexpr (g0 + 2 < 32 && !(ABL & 4)) {
                    wl[(g0 + 2) % 3] = wfrag(slot, (g0 + 2) & 15, 1, (g0 + 2) >> 4);
                    wh[(g0 + 2) % 3] = wfrag(slot, (g0 + 2) & 15, 0, (g0 + 2) >> 4);
                }
                __builtin_amdgcn_sched_barrier(0);
                mfma_a(acc[j + 1], wh[p1], xf[slot][0][ks]);
                if constexpr (g0 + 3 < 32 && !(ABL & 4)) {
                    wl[p0] = wfrag(slot, (g0 + 3) & 15, 1, (g0 + 3) >> 4);
                    wh[p0] = wfrag(slot, (g0 + 3) & 15, 0, (g0 + 3) >> 4);
                }
                __builtin_amdgcn_sched_barrier(0);
            });
            // the next slice has landed (everybody's pieces) and everybody is through this one
            if constexpr (!(ABL & 16)) {
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
            }
        };
        step(std::true_type{}, std::integral_constant<int, 0>{}, 0);
        step(std::false_type{}, std::integral_constant<int, 1>{}, 1);
        for (int kt = 2; kt < NK; kt += 2) {
            step(std::false_type{}, std::integral_constant<int, 0>{}, kt);
            step(std::false_type{}, std::integral_constant<int, 1>{}, kt + 1);
        }
        // (timing only: the same 16 steps again, k_reps - 1 times - the per-workgroup overhead drops out of the difference)
        for (int rep = 1; rep < k_reps; ++rep)
            for (int kt = 0; kt < NK; kt += 2) {
                step(std::false_type{}, std::integral_constant<int, 0>{}, kt);
                step(std::false_type{}, std::integral_constant<int, 1>{}, kt + 1 < NK - 1 ? kt + 1 : NK - 2);
            }
        asm volatile("s_nop 15" : "+a"(acc[0]), "+a"(acc[1]), "+a"(acc[2]), "+a"(acc[3]), "+a"(acc[4]), "+a"(acc[5]), "+a"(acc[6]), "+a"(acc[7]),
                     "+a"(acc[8]), "+a"(acc[9]), "+a"(acc[10]), "+a"(acc[11]), "+a"(acc[12]), "+a"(acc[13]), "+a"(acc[14]), "+a"(acc[15]));
        if (MODE == 0) {
            float s = 0.f;
#pragma unroll
            for (int j = 0; j < 16; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) s += acc[j][r];
            sums[(size_t)(blockIdx.x * blocks_per_wg + blk) * 256 + tid] = s;
        } else {
            // lane (x row l31, half lh) holds output columns 32 j + 8 (r >> 2) + 4 lh + (r & 3)
            float* crow = C + (size_t)(row_base + l31) * N_OUT;
#pragma unroll
            for (int j = 0; j < 16; ++j)
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    *reinterpret_cast<f32x4*>(crow + 32 * j + 8 * q + 4 * lh) = f32x4{acc[j][4 * q], acc[j][4 * q + 1], acc[j][4 * q + 2], acc[j][4 * q + 3]};
        }
    }
}

// ---- the same kernel on v_mfma_f32_16x16x32_f16.  acc[jn][i]: weight block jn (16 output columns) x activation row block i (16 rows);
// a group = one weight block: 6 MFMAs (3 products x 2 row blocks) where the 32x32x16 form has a PAIR of blocks per 6 - the same 4 multiplies
// and 2 fragment reads per 3 x 16 passes.  Fragment of lane l: row l & 15, chunk 4 plane + (l >> 4) at position chunk ^ ((row >> 1) & 7): the
// image and its swizzle are the 32x32x16 form's (a ds_read_b128 lane group {0-3, 12-15, 20-27} = rows 0-3, 12-15 of chunk c and rows 4-11
// of chunk c ^ 1: positions c ^ {0, 1, 6, 7} and c ^ 1 ^ {2, 3, 4, 5}, all eight, on both row parities: conflict-free)
template <int MODE, int ABL = 0>
__global__ __launch_bounds__(256, 1) void wp_mlp0_kernel16(const uint16_t* A, const uint16_t* W, float* C, float* sums, int M, int blocks_per_wg, int k_reps) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l15 = lane & 15, lq = lane >> 4;
    const unsigned lda_b = K_IN * 4, ldw_b = K_IN * 4;
    const __amdgpu_buffer_rsrc_t rsW = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t*>(W), 0, N_OUT * K_IN * 4, 0x00020000);
    unsigned w_vo[2];
    {
        const unsigned r = lane >> 3, pos = lane & 7;
        w_vo[0] = r * ldw_b + ((pos ^ ((r >> 1) & 7)) * 16u);
        w_vo[1] = r * ldw_b + ((pos ^ (((r + 8) >> 1) & 7)) * 16u);
    }
    auto load_piece = [&](int slot, int kt, int i) __attribute__((always_inline)) {
        const unsigned row0 = 128u * (unsigned)wave + 8u * (unsigned)i;
        glds16(rsW, smem + slot * SLICEB + row0 * 128, w_vo[i & 1], row0 * ldw_b + (unsigned)kt * 128u);
    };
    const unsigned lds0 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) char*)smem;
    const unsigned swz = (l15 >> 1) & 7;
    unsigned fa[2];  // [plane]
#pragma unroll
    for (int pl = 0; pl < 2; ++pl) fa[pl] = lds0 + (unsigned)(l15 * 128) + (((unsigned)(4 * pl + lq) ^ swz) << 4);
    typedef __attribute__((address_space(3))) const f16x8* lds_frag_t;
    auto wfrag = [&](int slot, int jn, int pl) __attribute__((always_inline)) {
        return *reinterpret_cast<lds_frag_t>((uintptr_t)(fa[pl] + (unsigned)(slot * SLICEB + jn * 16 * 128)));
    };
    unsigned k2048 = 0x10001000u;
    asm volatile("" : "+v"(k2048));

    for (int blk = 0; blk < blocks_per_wg; ++blk) {
        const int row_base = (blockIdx.x * blocks_per_wg + blk) * ROWS_WG + wave * 32;
        if (row_base >= M) break;
        const char* xrow = reinterpret_cast<const char*>(A) + (size_t)(row_base + l15) * lda_b + lq * 16;
        f32x4 acc[32][2];
        f16x8 xf[2][2][2];  // [buffer][plane][row block]
        auto load_x = [&](int b, int kt) __attribute__((always_inline)) {
#pragma unroll
            for (int pl = 0; pl < 2; ++pl)
#pragma unroll
                for (int i = 0; i < 2; ++i) xf[b][pl][i] = *reinterpret_cast<const f16x8*>(xrow + (size_t)i * 16 * lda_b + kt * 128 + pl * 64);
        };
        constexpr int NK = K_IN / BK;
#pragma unroll
        for (int i = 0; i < 16; ++i) load_piece(0, 0, i);
        load_x(0, 0);
        if (ABL & 8) load_x(1, 0);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
        auto step = [&](auto FIRST, auto SLOT, int kt) __attribute__((always_inline)) {
            constexpr bool first = decltype(FIRST)::value;
            constexpr int slot = decltype(SLOT)::value;
            f16x8 wh[3], wl[3];  // the fragments of blocks g, g + 1, g + 2: read two blocks (12 MFMA slots of 4 passes) ahead of their use
            wl[0] = wfrag(slot, 0, 1);
            wh[0] = wfrag(slot, 0, 0);
            wl[1] = wfrag(slot, 1, 1);
            wh[1] = wfrag(slot, 1, 0);
            if (ABL & 4) { wl[2] = wl[0]; wh[2] = wh[1]; }
            const bool more = kt + 1 < NK;
            __builtin_amdgcn_sched_barrier(0);
            static_for<0, 32>([&](auto GG) __attribute__((always_inline)) {
                constexpr int g = decltype(GG)::value, pb = g % 3;
                const u32x4 whu = __builtin_bit_cast(u32x4, wh[pb]);
                u32x4 w2u;
                // slots 0, 1: x_hi w_lo of both row blocks; the multiplies behind the first
                if constexpr (first) mfma16_a0(acc[g][0], wl[pb], xf[slot][0][0]); else mfma16_a(acc[g][0], wl[pb], xf[slot][0][0]);
#pragma unroll
                for (int e = 0; e < 4; ++e) w2u[e] = (ABL & 2) ? whu[e] : pk_mul(whu[e], k2048);
                __builtin_amdgcn_sched_barrier(0);
                if constexpr (first) mfma16_a0(acc[g][1], wl[pb], xf[slot][0][1]); else mfma16_a(acc[g][1], wl[pb], xf[slot][0][1]);
                __builtin_amdgcn_sched_barrier(0);
                // slots 2, 3: x_lo' (2^-11 w_hi); a piece of the next slice behind the first (16 pieces over the first 16 blocks), the next
                // step's activation fragments behind block 0
                mfma16_a(acc[g][0], __builtin_bit_cast(f16x8, w2u), xf[slot][1][0]);
                if constexpr (g < 16 && !(ABL & 1)) { if (more) load_piece(slot ^ 1, kt + 1, g); }
                if constexpr (g == 0 && !(ABL & 8)) { if (more) load_x(slot ^ 1, kt + 1); }
                __builtin_amdgcn_sched_barrier(0);
                mfma16_a(acc[g][1], __builtin_bit_cast(f16x8, w2u), xf[slot][1][1]);
                __builtin_amdgcn_sched_barrier(0);
                // slots 4, 5: x_hi w_hi; the fragments of block g + 2 go into the buffers block g - 1 used
                mfma16_a(acc[g][0], wh[pb], xf[slot][0][0]);
                if constexpr (g + 2 < 32 && !(ABL & 4)) {
                    wl[(g + 2) % 3] = wfrag(slot, g + 2, 1);
                    wh[(g + 2) % 3] = wfrag(slot, g + 2, 0);
                }
                __builtin_amdgcn_sched_barrier(0);
                mfma16_a(acc[g][1], wh[pb], xf[slot][0][1]);
                __builtin_amdgcn_sched_barrier(0);
            });
            if constexpr (!(ABL & 16)) {
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
            }
        };
        step(std::true_type{}, std::integral_constant<int, 0>{}, 0);
        step(std::false_type{}, std::integral_constant<int, 1>{}, 1);
        for (int kt = 2; kt < NK; kt += 2) {
            step(std::false_type{}, std::integral_constant<int, 0>{}, kt);
            step(std::false_type{}, std::integral_constant<int, 1>{}, kt + 1);
        }
        for (int rep = 1; rep < k_reps; ++rep)
            for (int kt = 0; kt < NK; kt += 2) {
                step(std::false_type{}, std::integral_constant<int, 0>{}, kt);
                step(std::false_type{}, std::integral_constant<int, 1>{}, kt + 1 < NK - 1 ? kt + 1 : NK - 2);
            }
#pragma unroll
        for (int j = 0; j < 32; j += 8)
            asm volatile("s_nop 15" : "+a"(acc[j][0]), "+a"(acc[j][1]), "+a"(acc[j + 1][0]), "+a"(acc[j + 1][1]), "+a"(acc[j + 2][0]), "+a"(acc[j + 2][1]), "+a"(acc[j + 3][0]),
                         "+a"(acc[j + 3][1]), "+a"(acc[j + 4][0]), "+a"(acc[j + 4][1]), "+a"(acc[j + 5][0]), "+a"(acc[j + 5][1]), "+a"(acc[j + 6][0]), "+a"(acc[j + 6][1]),
                         "+a"(acc[j + 7][0]), "+a"(acc[j + 7][1]));
        if (MODE == 0) {
            float s = 0.f;
#pragma unroll
            for (int j = 0; j < 32; ++j)
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int r = 0; r < 4; ++r) s += acc[j][i][r];
            sums[(size_t)(blockIdx.x * blocks_per_wg + blk) * 256 + tid] = s;
        } else {
            // lane (x row 16 i + l15, quarter lq) holds output columns 16 jn + 4 lq + (0..3)
#pragma unroll
            for (int j = 0; j < 32; ++j)
#pragma unroll
                for (int i = 0; i < 2; ++i) *reinterpret_cast<f32x4*>(C + (size_t)(row_base + 16 * i + l15) * N_OUT + 16 * j + 4 * lq) = acc[j][i];
        }
    }
}

static uint16_t f2h(float f) { _Float16 h = (_Float16)f; uint16_t u; memcpy(&u, &h, 2); return u; }
static float h2f(uint16_t u) { _Float16 h; memcpy(&h, &u, 2); return (float)h; }

int main(int argc, char** argv) {
    const bool check = argc > 1 && !strcmp(argv[1], "--check");
    const bool clock = argc > 1 && !strcmp(argv[1], "--clock");
    const bool ablations = argc > 1 && !strcmp(argv[1], "--ablations");
    const int M = check ? 256 : 65536;
    hipDeviceProp_t prop;
    hipGetDeviceProperties(&prop, 0);
    const int cus = prop.multiProcessorCount;
    // planes: A scaled (hi, lo' = 2^11 (x - hi)), W plain (hi, lo) of values of magnitude ~2^13 (the library's 2^s W)
    std::vector<uint16_t> hA((size_t)M * K_IN * 2), hW((size_t)N_OUT * K_IN * 2);
    std::vector<float> xa((size_t)M * K_IN), xw((size_t)N_OUT * K_IN);
    unsigned s = 12345u;
    auto rnd = [&]() { s = s * 1664525u + 1013904223u; return ((float)(s >> 8) / 16777216.f - 0.5f) * 2.f; };
    auto idx = [&](size_t m, int k) { return m * 2 * K_IN + (size_t)(k >> 5) * 64 + (k & 31); };
    for (size_t m = 0; m < (size_t)M; ++m)
        for (int k = 0; k < K_IN; ++k) {
            const float v = rnd();
            const uint16_t hi = f2h(v), lo = f2h(2048.f * (v - h2f(hi)));
            hA[idx(m, k)] = hi; hA[idx(m, k) + 32] = lo;
            xa[m * K_IN + k] = h2f(hi) + h2f(lo) / 2048.f;
        }
    for (size_t n = 0; n < (size_t)N_OUT; ++n)
        for (int k = 0; k < K_IN; ++k) {
            const float v = rnd() * 8192.f;
            const uint16_t hi = f2h(v), lo = f2h(v - h2f(hi));
            hW[idx(n, k)] = hi; hW[idx(n, k) + 32] = lo;
            xw[n * K_IN + k] = h2f(hi) + h2f(lo);
        }
    uint16_t *dA, *dW;
    float *dC, *dS;
    hipMalloc(&dA, hA.size() * 2); hipMalloc(&dW, hW.size() * 2);
    hipMalloc(&dC, (size_t)M * N_OUT * 4); hipMalloc(&dS, (size_t)(M / ROWS_WG) * 256 * 4);
    hipMemcpy(dA, hA.data(), hA.size() * 2, hipMemcpyHostToDevice);
    hipMemcpy(dW, hW.data(), hW.size() * 2, hipMemcpyHostToDevice);
    char host[256] = "?";
    if (FILE* f = fopen("/proc/sys/kernel/hostname", "r")) { if (fscanf(f, "%255s", host) != 1) strcpy(host, "?"); fclose(f); }
    char bus[64] = "?";
    hipDeviceGetPCIBusId(bus, sizeof bus, 0);
    printf("box %s, device %s at PCI %s (%s), %d CUs\n", host, prop.name[0] ? prop.name : "(no marketing name reported)", bus, prop.gcnArchName, cus);
    if (check) {
        int bad = 0;
        struct Chk { const char* name; const void* fn; };
        const Chk chk[] = {{"32x32x16", (const void*)wp_mlp0_kernel<1>}, {"16x16x32", (const void*)wp_mlp0_kernel16<1>}};
        for (const Chk& c : chk) {
            hipFuncSetAttribute(c.fn, hipFuncAttributeMaxDynamicSharedMemorySize, LDSB);
            hipMemset(dC, 0xff, (size_t)M * N_OUT * 4);
            int Mv = M, one = 1;
            void* args[] = {&dA, &dW, &dC, &dS, &Mv, &one, &one};
            hipLaunchKernel(c.fn, dim3(M / ROWS_WG), dim3(256), args, LDSB, 0);
            std::vector<float> hC((size_t)M * N_OUT);
            if (hipMemcpy(hC.data(), dC, hC.size() * 4, hipMemcpyDeviceToHost) != hipSuccess) { printf("%s: the launch failed\n", c.name); return 1; }
            double worst = 0.0;
            for (int m = 0; m < M; m += 7)
                for (int n = 0; n < N_OUT; n += 5) {
                    double ref = 0.0, mag = 0.0;
                    for (int k = 0; k < K_IN; ++k) { ref += (double)xa[(size_t)m * K_IN + k] * xw[(size_t)n * K_IN + k]; mag += fabs((double)xa[(size_t)m * K_IN + k] * xw[(size_t)n * K_IN + k]); }
                    const double e = fabs(hC[(size_t)m * N_OUT + n] - ref) / mag;
                    worst = e == e ? fmax(worst, e) : 1.0;
                }
            printf("check %s: max |C - ref| / sum |a||w| = %.3g over a sample of outputs (3-product f16x2: the dropped lo x lo term is 2^-22)\n", c.name, worst);
            if (!(worst < 2e-6)) bad = 1;
        }
        return bad;
    }
    hipEvent_t e0, e1;
    hipEventCreate(&e0); hipEventCreate(&e1);
    struct Var { const char* name; const void* fn; };
    auto time_variant = [&](int round, const Var& v) {
        const int grid = M / ROWS_WG;
        hipFuncSetAttribute(v.fn, hipFuncAttributeMaxDynamicSharedMemorySize, LDSB);
        int Mv = M, bv = 1;
        double us_r[2];
        for (int ri = 0; ri < 2; ++ri) {
            int kr = ri ? 5 : 1;
            void* args[] = {&dA, &dW, &dC, &dS, &Mv, &bv, &kr};
            for (int rep = 0; rep < 3; ++rep) hipLaunchKernel(v.fn, dim3(grid), dim3(256), args, LDSB, 0);
            hipDeviceSynchronize();
            const int n = 10;
            hipEventRecord(e0);
            for (int rep = 0; rep < n; ++rep) hipLaunchKernel(v.fn, dim3(grid), dim3(256), args, LDSB, 0);
            hipEventRecord(e1); hipEventSynchronize(e1);
            float ms_; hipEventElapsedTime(&ms_, e0, e1);
            us_r[ri] = 1e3 * ms_ / n;
        }
        const double per_step = (us_r[1] - us_r[0]) / (4.0 * 16.0 * ((M / ROWS_WG + cus - 1) / cus));  // us per K step and CU, overhead-free
        if (round >= 0) printf("round %d  ", round);
        printf("%-32s %6.1f us per launch; steady state %5.0f ns per K step = %4.0f TF fp32-equivalent (of 833 nominal)\n", v.name, us_r[0], 1e3 * per_step,
               2.0 * 128 * 512 * 32 * cus / per_step / 1e6);
    };
    if (clock) {
        // long dispatches of the full stream, the shapes alternating: for a counter pass (the clock = GRBM_GUI_ACTIVE / 8 / wall)
        const Var cv[] = {{"32x32x16 full stream", (const void*)wp_mlp0_kernel<0, 0>}, {"16x16x32 full stream", (const void*)wp_mlp0_kernel16<0, 0>}};
        for (const Var& v : cv) hipFuncSetAttribute(v.fn, hipFuncAttributeMaxDynamicSharedMemorySize, LDSB);
        for (int round = 0; round < 4; ++round)
            for (const Var& v : cv) {
                int Mv = M, bv = 1, kr = 40;
                void* args[] = {&dA, &dW, &dC, &dS, &Mv, &bv, &kr};
                hipEventRecord(e0);
                for (int rep = 0; rep < 3; ++rep) hipLaunchKernel(v.fn, dim3(M / ROWS_WG), dim3(256), args, LDSB, 0);
                hipEventRecord(e1); hipEventSynchronize(e1);
                float ms_; hipEventElapsedTime(&ms_, e0, e1);
                printf("%-24s %8.1f us per launch of %d x 16 K steps\n", v.name, 1e3 * ms_ / 3, kr);
            }
        return 0;
    }
    if (ablations) {
        // the round-6 list (profiles/r6_wp_gemm.log): what each part of the wave-private stream costs, on the 32x32x16 shape it was measured on
        const Var av[] = {{"full stream", (const void*)wp_mlp0_kernel<0, 0>}, {"no LDS-direct loads", (const void*)wp_mlp0_kernel<0, 1>}, {"no multiplies", (const void*)wp_mlp0_kernel<0, 2>},
                          {"no fragment reads", (const void*)wp_mlp0_kernel<0, 4>}, {"no activation loads", (const void*)wp_mlp0_kernel<0, 8>},
                          {"no end-of-step wait / barrier", (const void*)wp_mlp0_kernel<0, 16>}, {"MFMAs + multiplies only", (const void*)wp_mlp0_kernel<0, 29>},
                          {"MFMAs only", (const void*)wp_mlp0_kernel<0, 31>}, {"full stream (again)", (const void*)wp_mlp0_kernel<0, 0>},
                          {"MFMAs only (again)", (const void*)wp_mlp0_kernel<0, 31>}};
        for (const Var& v : av) time_variant(-1, v);
        return 0;
    }
    // the shapes alternate, variant by variant, three times over (discard each arm's first line: the chip is not yet in its steady state)
    const Var vars[] = {{"32x32x16 full stream", (const void*)wp_mlp0_kernel<0, 0>}, {"16x16x32 full stream", (const void*)wp_mlp0_kernel16<0, 0>},
                        {"32x32x16 no end-of-step wait", (const void*)wp_mlp0_kernel<0, 16>}, {"16x16x32 no end-of-step wait", (const void*)wp_mlp0_kernel16<0, 16>},
                        {"32x32x16 MFMAs + multiplies", (const void*)wp_mlp0_kernel<0, 29>}, {"16x16x32 MFMAs + multiplies", (const void*)wp_mlp0_kernel16<0, 29>},
                        {"32x32x16 MFMAs only", (const void*)wp_mlp0_kernel<0, 31>}, {"16x16x32 MFMAs only", (const void*)wp_mlp0_kernel16<0, 31>}};
    for (int round = 0; round < 4; ++round)
        for (const Var& v : vars) time_variant(round, v);
    return 0;
}
