// Plane-in / plane-out "NT" GEMM of the f16x2 arithmetic mode:  C[m][n] = act(sum_k A[m][k] W[n][k] + bias[n]) (+ R[m][n])
//
// Same arithmetic as gemm_h2.hip (x = x_hi + 2^-11 x_lo', weights 2^s W = w_hi + w_lo, three fp16 MFMA products per
// block into one fp32 accumulator), but the activation arrives ALREADY as the two planes (p2.h): whoever produced it
// split it once, in its epilogue.  What that buys in the K loop, per 256 x 256 x 32 step and workgroup:
//   * no fp32 -> plane split (40 VALU per thread) and no ds_write at all: the 64 KB of operand planes go from global
//     memory straight into LDS, 64 buffer_load_dwordx4 ... lds per step (8 per wave), each a full 128-byte line per row;
//   * LDS double-buffered (2 x 64 KB), ONE barrier per K step: the loads of step g + 1 are issued right after the barrier
//     that opens step g and have that whole step (96 MFMAs per wave) to land;
//   * bank-conflict-free fragment reads without padding (XOR swizzle applied on the source address, p2.h).
// The epilogue goes through per-wave LDS slabs (32 rows x 32 floats, the 16-byte chunks of a row XOR-swizzled by the row) so that bias / ReLU / residual / the plane split
// work on 8 consecutive columns of one row per lane and every store covers 64-byte row segments; the residual is read
// back from its planes (22 bits) in the same layout.  Output kinds: fp32, scaled planes (the next GEMM's operand), or
// the attention operands q | k (plain planes, q pre-scaled) + V^T (transposed plain planes, keys in the order of the
// transposed-score registers) - attention_p2.hip then never touches an fp32 q|k|v matrix.
#include <cstdlib>
#include <type_traits>

#include "gemm_p2_core.h"
#include "gemm_walk.h"

namespace e2emv {

template <int OUT, bool HAS_R = false>
__global__ __launch_bounds__(512, 1) void gemm_p2_kernel(GemmP2Params p) {
    extern __shared__ __attribute__((aligned(16))) char smem_p2[];

    const GemmWalk walk(p.total, blockIdx.x, gridDim.x);
    if (walk.empty()) return;
    int tile = walk.tile;
    const int t_end = walk.t_end, slots = walk.slots;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave >> 1, wc = wave & 1;
    const int nk = p.K / P2_BK, nk1 = p.K1 / P2_BK;

    const __amdgpu_buffer_rsrc_t rsA = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t*>(p.A), 0, (int)p.a_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsA2 = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t*>(p.A2), 0, (int)p.a2_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsW = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t*>(p.W), 0, (int)p.w_bytes, 0x00020000);

    // ---- loader: wave w moves rows 32 w .. 32 w + 31 of the activation tile and of the weight tile, 4 + 4 LDS-direct loads
    // per K step; one load = 8 rows x 128 B, lane -> (row lane >> 3, LDS position lane & 7), source chunk = position ^ swizzle
    const int ld_r = lane >> 3, ld_p = lane & 7;
    unsigned a_vo[4], a2_vo[4], w_vo[4];
    auto setup = [&](int t) {
        const auto [tm, tn] = gemm_tile(t, p.tiles_n);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int row = 32 * wave + 8 * i + ld_r;
            const unsigned c = (unsigned)(ld_p ^ ((row >> 1) & 7));
            const unsigned gm = (unsigned)min(tm * P2_BM + row, p.M - 1);
            a_vo[i] = gm * p.lda_b + c * 16u;
            a2_vo[i] = gm * p.lda2_b + c * 16u;
            const unsigned gn = (unsigned)min(tn * P2_BN + row, p.N - 1);
            w_vo[i] = gn * p.ldw_b + c * 16u;
        }
    };
    auto issue = [&](int buf, int kt, unsigned dep) {
        char* dst = smem_p2 + buf * P2_BUFB + 32 * wave * P2_ROWB;
        if (kt < nk1) {
            const unsigned so = (unsigned)kt * 128u;
#pragma unroll
            for (int i = 0; i < 4; ++i) p2_glds16(rsA, dst + i * 1024, a_vo[i] + dep, so);
        } else {
            const unsigned so = (unsigned)(kt - nk1) * 128u;
#pragma unroll
            for (int i = 0; i < 4; ++i) p2_glds16(rsA2, dst + i * 1024, a2_vo[i] + dep, so);
        }
        const unsigned sw = (unsigned)kt * 128u;
#pragma unroll
        for (int i = 0; i < 4; ++i) p2_glds16(rsW, dst + P2_TILEB + i * 1024, w_vo[i] + dep, sw);
    };

    // ---- fragments (gp_kstep): lane l = (row l & 15 of a 16-row block, k-chunk l >> 4); chunk index c = 4 plane + (l >> 4), stored at
    // position c ^ ((row >> 1) & 7)
    p2_acc_t acc;

    // ---- the K step: gp_kstep (gemm_p2_core.h), software-pipelined inside the wave

    // ---- epilogue: gp_epilogue (gemm_p2_core.h)

    // ---- pipeline.  Step g = (tile, kt) in execution order lives in LDS buffer g & 1.  A step opens with "my loads of this
    // step have landed" + ONE barrier (everybody's have; everybody is done reading the other buffer); the loads of step
    // g + 1 then go into the other buffer.  The two waves that share a SIMD (w and w + 4) take OPPOSITE orders: waves 4-7
    // issue their 8 loads first and compute after, waves 0-3 compute first and issue after (s_memtime stamps: with both
    // issuing first the matrix pipe idled ~700-1000 cycles per step).
    // Across an epilogue the load position runs TWO steps ahead: the loads of step L + 1 went out during the tile's last
    // step L as always, those of step L + 2 go out right after it (its buffer is free: the slabs live behind the tile
    // buffers) - both BEFORE the 32 stores of the epilogue.  vmcnt retires in issue order, so step L + 1 waits with
    // vmcnt(40) (8 loads of L + 2 and 32 stores may stay in flight) and step L + 2 with vmcnt(32): the store burst of the
    // epilogue - every CU of the chip reaches it at the same time - drains under two K steps of the next tile instead of
    // in front of them.  Barriers are raw s_barrier: __syncthreads() would add vmcnt(0) while LDS-direct loads are in flight.
    int ld_tile = tile, ld_kt = 0;
    bool ld_valid = true;
    auto advance = [&]() {
        if (ld_kt + 1 < nk) { ++ld_kt; return; }
        if (ld_tile + slots < t_end) {
            ld_tile += slots;
            ld_kt = 0;
            setup(ld_tile);
        } else {
            ld_valid = false;
        }
    };
    setup(tile);
    issue(0, 0, 0u);
    advance();
    const bool issue_first = wave >= 4;
    const bool overlap = nk >= 3;
    // tile exponents of the A operand (p2.h): the accumulators live at the exponent of the CURRENT K block; when it changes
    // they are rescaled (exact: a power of two) - a wave-uniform branch that an ordinary network never takes
    // The exponents of a tile's K blocks are fetched ONCE, by one vector load (lane i: block i of this wave's 64 rows; the
    // next tile's before the epilogue of this one), and read with v_readlane in the loop: no memory operation there.
    // Lanes 32, 33 / 34, 35 of the same load bring the exponents / max |x| of the two residual blocks this wave adds in the
    // tile's epilogue (a dependent load there would cost an L2 / HBM round trip per tile with the matrix pipe idle).
    const bool has_e = p.EA != nullptr || (HAS_R && p.ER != nullptr);
    int e_run = 0, cur_kt = 0;
    int ev = 0, ev_next = 0;
    auto fetch_e = [&](int t) {
        int v = 0;
        if (has_e) {
            const auto [tm_, tn_] = gemm_tile(t, p.tiles_n);
            const int erow = tm_ * 4 + wr;
            const int nb1 = nk1 >> 1, nb = (nk + 1) >> 1;
            if (erow * 64 < p.M) {
                if (lane < nb) {
                    if (p.EA) v = lane < nb1 ? p.EA[erow * p.eld_a + lane] : (p.EA2 ? p.EA2[erow * p.eld_a2 + lane - nb1] : 0);
                } else if (HAS_R && p.ER && lane >= 32 && lane < 36) {
                    const int cb = tn_ * 4 + wc * 2 + (lane & 1);
                    if (cb < p.eld_r) {
                        if (lane < 34) v = p.ER[erow * p.eld_r + cb];
                        else if (p.AR) v = __builtin_bit_cast(int, p.AR[erow * p.eld_r + cb]);
                    }
                }
            }
        }
        return v;
    };
    ev = fetch_e(tile);
    int since = 8;       // K steps since the last epilogue
    bool ahead = false;  // the loads of the step after next were issued before that epilogue
    int buf = 0;
    auto step = [&](auto FIRST) {
        if (since == 0 && ahead) asm volatile("s_waitcnt vmcnt(40)" ::: "memory");
        else if (since <= 1 && overlap) asm volatile("s_waitcnt vmcnt(32)" ::: "memory");  // (since == 0 without `ahead`: 8 loads, then the stores)
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
        if (has_e) {
            const int e_step = p.EA ? __builtin_amdgcn_readlane(ev, cur_kt >> 1) : 0;
            if (!decltype(FIRST)::value && e_step != e_run) {
                asm volatile("s_nop 15");  // (the previous step's asm MFMAs -> the VALU below: hipcc does not pad an asm's results)
                const int d = e_run - e_step;
                const float f = d < -126 ? 0.f : p2_exp2i(d);
#pragma unroll
                for (int j = 0; j < P2_ACC_J; ++j)
#pragma unroll
                    for (int i = 0; i < P2_ACC_I; ++i)
#pragma unroll
                        for (int r = 0; r < 4; ++r) acc[j][i][r] *= f;
            }
            e_run = e_step;
            // the NEXT tile's exponents: loaded beside the operand loads of K step 2, picked up at the head of step 3, right
            // behind that step's vmcnt(0) - the wait hipcc attaches to the use is then free.  (Fetched at the tile boundary the
            // wait would sit behind the epilogue's 32 stores and drain them.)
            if (nk >= 4 && tile + slots < t_end) {
                if (cur_kt == 2) ev_next = fetch_e(tile + slots);
                if (cur_kt == 3) asm volatile("" : "+v"(ev_next));
            }
        }
        ++cur_kt;
        const bool ldv = ld_valid && !(since == 0 && ahead);
        if (issue_first && ldv) issue(buf ^ 1, ld_kt, 0u);
        gp_kstep<decltype(FIRST)::value>(smem_p2, buf, wr, wc, lane, acc);
        if (!issue_first && ldv) {
            unsigned dep = 0;
            asm("" : "+v"(dep) : "v"(acc[P2_ACC_J - 1][P2_ACC_I - 1]));  // scheduling-only: keeps the loads behind the MFMAs
            issue(buf ^ 1, ld_kt, dep);
        }
        if (ldv) advance();
        if (since == 0) ahead = false;
        ++since;
        buf ^= 1;
    };
    for (;;) {
        step(std::true_type{});
        for (int kt = 1; kt < nk; ++kt) step(std::false_type{});
        if (overlap && ld_valid) {
            // the buffer of the step just computed is free once every wave is through it: the loads of the step after next
            asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
            unsigned dep = 0;
            asm("" : "+v"(dep) : "v"(acc[P2_ACC_J - 1][P2_ACC_I - 1]));
            issue(buf ^ 1, ld_kt, dep);
            advance();
            ahead = true;
        }
        cur_kt = 0;
        if (has_e && nk < 4 && tile + slots < t_end) ev_next = fetch_e(tile + slots);
        gp_acc_fence(acc);
        // (gemm_tile's decode, written out: through the header every instance of this kernel got another instruction stream)
        gp_epilogue<OUT, HAS_R>(p, smem_p2, acc, wave, tile / p.tiles_n, tile % p.tiles_n, e_run, ev);
        ev = ev_next;
        since = overlap ? 0 : 8;
        tile += slots;
        if (tile >= t_end) break;
    }
}

// validates one GEMM and fills its kernel parameter block (shared with the chained launch, gemm_p2c.hip)
int fill_gemm_p2_params(e2emv_ctx* ctx, const GemmP2Args& a, GemmP2Params& p) {
    if (a.M <= 0 || a.N <= 0 || a.K <= 0) return set_err(ctx, E2EMV_ESHAPE, "gemm_p2: empty problem");
    int K1;
    if (int rc = gemm_k_segments(ctx, "gemm_p2", a.K, a.K1, a.A2 != nullptr, &K1)) return rc;
    if (K1 <= 0) return set_err(ctx, E2EMV_ESHAPE, "gemm_p2: K=%d K1=%d must be multiples of 32", a.K, K1);  // the planes' first segment is never empty
    if (!a.A || !a.W || a.lda % 32 || a.lda < K1 || (a.A2 && (a.lda2 % 32 || a.lda2 < a.K - K1)))
        return set_err(ctx, E2EMV_ESHAPE, "gemm_p2: operand planes need whole 32-column blocks (lda=%lld lda2=%lld)", (long long)a.lda, (long long)a.lda2);
    if ((uintptr_t)a.A % 16 || (a.A2 && (uintptr_t)a.A2 % 16) || (uintptr_t)a.W % 16 || (a.bias && (uintptr_t)a.bias % 16) || (a.Rp && (uintptr_t)a.Rp % 16))
        return set_err(ctx, E2EMV_ESHAPE, "gemm_p2: operands must be 16-byte aligned");
    if (a.Rp && (a.ldr % 32 || a.ldr < a.N)) return set_err(ctx, E2EMV_ESHAPE, "gemm_p2: residual planes need ldr %% 32 == 0");
    const int64_t a_bytes = (int64_t)a.M * a.lda * 4, a2_bytes = a.A2 ? (int64_t)a.M * a.lda2 * 4 : 16, w_bytes = (int64_t)a.N * a.K * 4;
    if (a_bytes >= ((int64_t)1 << 31) || a2_bytes >= ((int64_t)1 << 31) || w_bytes >= ((int64_t)1 << 31))
        return set_err(ctx, E2EMV_ESHAPE, "gemm_p2: operand larger than 2 GB (M=%d lda=%lld): 32-bit byte offsets", a.M, (long long)a.lda);
    p = GemmP2Params{};
    p.A = a.A; p.A2 = a.A2 ? a.A2 : a.A; p.W = a.W;
    p.a_bytes = (unsigned)a_bytes; p.a2_bytes = (unsigned)(a.A2 ? a2_bytes : a_bytes); p.w_bytes = (unsigned)w_bytes;
    p.lda_b = (unsigned)(a.lda * 4); p.lda2_b = (unsigned)((a.A2 ? a.lda2 : a.lda) * 4); p.ldw_b = (unsigned)(a.K * 4);
    p.bias = a.bias; p.Rp = a.Rp; p.ldr = a.ldr;
    p.C32 = a.C32; p.Cp = a.Cp; p.Vt = a.Vt; p.ldc = a.ldc;
    p.M = a.M; p.N = a.N; p.K = a.K; p.K1 = K1;
    p.tiles_n = (a.N + P2_BN - 1) / P2_BN;
    p.total = ((a.M + P2_BM - 1) / P2_BM) * p.tiles_n;
    p.relu = a.relu ? 1 : 0;
    p.out_scale = a.out_scale;
    p.col_scale[0] = p.col_scale[1] = p.col_scale[2] = 1.f;
    p.n_rows = a.n_rows; p.heads = a.heads;
    p.EA = a.EA; p.EA2 = a.EA2; p.ER = a.ER; p.EC = a.EC; p.EVt = a.EVt; p.AR = a.AR; p.AC = a.AC;
    p.eld_a = (int)(a.lda / 64); p.eld_a2 = (int)(a.lda2 / 64); p.eld_r = (int)(a.ldr / 64); p.eld_c = (int)(a.ldc / 64);
    p.bias_amax = a.bias ? a.bias_amax : 0.f;
    if (a.EA && (a.lda % 64 || K1 % 64 || (a.A2 && (a.lda2 % 64 || (a.K - K1) % 64)) || a.M % 64))
        return set_err(ctx, E2EMV_ESHAPE, "gemm_p2: tile exponents need 64-column / 64-row blocks (lda=%lld K1=%d M=%d)", (long long)a.lda, K1, a.M);
    if ((a.EC || a.EVt) && (a.M % 64 || (a.out == P2_OUT_PLANES && a.ldc % 64))) return set_err(ctx, E2EMV_ESHAPE, "gemm_p2: output exponents need 64 x 64 blocks");
    if (a.ER && (a.ldr % 64 || a.M % 64)) return set_err(ctx, E2EMV_ESHAPE, "gemm_p2: residual exponents need 64 x 64 blocks");
    if (int rc = ensure_flags(ctx)) return rc;
    p.stats = ctx->d_flags + 2;
    switch (a.out) {
        case P2_OUT_F32:
            if (!a.C32 || a.N % 4 || a.ldc % 4 || (uintptr_t)a.C32 % 16) return set_err(ctx, E2EMV_ESHAPE, "gemm_p2: fp32 output needs N %% 4 == 0, ldc %% 4 == 0");
            break;
        case P2_OUT_PLANES:
            if (!a.Cp || a.N % 8 || a.ldc % 32 || a.ldc < a.N || (uintptr_t)a.Cp % 16) return set_err(ctx, E2EMV_ESHAPE, "gemm_p2: plane output needs N %% 8 == 0, ldc %% 32 == 0");
            break;
        case P2_OUT_QKV:
            if (!a.Cp || !a.Vt || a.N != 3 * P2_BN || a.heads != 4 || a.n_rows <= 0 || a.n_rows % 32 || a.M % a.n_rows || a.relu || a.Rp ||
                (uintptr_t)a.Cp % 16 || (uintptr_t)a.Vt % 16)
                return set_err(ctx, E2EMV_ESHAPE, "gemm_p2: q|k|v output needs N = 768 (4 heads of 64), n_rows %% 32 == 0, M %% n_rows == 0");
            p.ldc = 2 * P2_BN;
            p.eld_c = 8;
            p.col_scale[0] = 0.125f * 1.4426950408889634f * P2_QS;  // log2(e) / sqrt(64), then the plane pre-scale
            p.col_scale[2] = P2_VS;
            break;
        default: return set_err(ctx, E2EMV_EINVAL, "gemm_p2: unknown output kind %d", a.out);
    }
    if (!ctx->d_dummy) E2EMV_HIP(ctx, hipMalloc((void**)&ctx->d_dummy, 4096));
    p.dummy = ctx->d_dummy;
    return E2EMV_OK;
}

int launch_gemm_p2(e2emv_ctx* ctx, const GemmP2Args& a, hipStream_t s) {
    GemmP2Params p;
    if (int rc = fill_gemm_p2_params(ctx, a, p)) return rc;
    const void* fn = nullptr;
    switch (a.out) {
        case P2_OUT_F32: fn = a.Rp ? reinterpret_cast<const void*>(gemm_p2_kernel<P2_OUT_F32, true>) : reinterpret_cast<const void*>(gemm_p2_kernel<P2_OUT_F32, false>); break;
        case P2_OUT_PLANES: fn = a.Rp ? reinterpret_cast<const void*>(gemm_p2_kernel<P2_OUT_PLANES, true>) : reinterpret_cast<const void*>(gemm_p2_kernel<P2_OUT_PLANES, false>); break;
        default: fn = reinterpret_cast<const void*>(gemm_p2_kernel<P2_OUT_QKV, false>); break;
    }
    const int sl = gemm_slots(p.total, ctx->num_cus, 1);
    const size_t lds = P2_LDSB;
    if (int rc = ensure_dynamic_lds(ctx, fn, lds)) return rc;
    void* args[] = {&p};
    E2EMV_HIP(ctx, hipLaunchKernel(fn, dim3(8 * sl), dim3(512), args, lds, s));
    E2EMV_CHECK_LAUNCH(ctx, "gemm_p2_kernel");
    return E2EMV_OK;
}

}  // namespace e2emv
