// Sinkhorn log-space optimal transport with dustbins + mutual-arg-max matching: the host side of a call.
//
// Restates upstream SuperGlue `log_optimal_transport` / `log_sinkhorn_iterations` and the
// match block of `SuperGlue.forward` (superglue.py; the reference runs them inside its
// absent MultiViewMatcher.forward - call sites helpers.py:246, eval_pairs.py:212).
//
// A call = workspace, plan, launches.  The default path is a RESIDENT kernel: all iterations in one launch, in the exponential
// domain, K = exp(S - rowmax) kept on chip for the whole call, the workgroups of a problem exchanging column sums through tagged
// granules (the protocol: sinkhorn_exchange.h):
//   sinkhorn_resident<KT, ...>   8 waves, 32 / 64 rows per workgroup, K in 64 / 128 compiler-allocated registers per lane
//                                (sinkhorn_resident.hip)
//   sinkhorn_resident128         4 waves, 128 rows x <= 1024 columns: 24 of a wave's 32 rows in registers the kernel addresses
//                                by number (v64 - v255, a64 - a255; the compiler confined to 56), 8 in LDS - 32 problems resident
//   sinkhorn_resident2k          the same for <= 2048 columns, 64 rows per workgroup - 8 problems resident instead of 4
//                                (both: sinkhorn_regs.hip)
//   sinkhorn_resident128w        128 rows x <= 1024 columns on 8 waves, two per SIMD: 12 of a wave's 16 rows in v64 - v255, 4 in
//                                LDS, no accumulation registers (sinkhorn_regs2.hip) - the launcher's 128-row kernel of choice
// followed by sinkhorn_rescue (problems that left fp32's range or gave up on a wait: re-solved in the log domain) and the final
// sweep of the log-domain launch chain (sinkhorn_stream.hip), which is also the fallback for everything the plan does not take.
#include <algorithm>
#include <cmath>

#include "sinkhorn_internal.h"
#include "sinkhorn_exchange.h"  // SkResParams

namespace e2emv {

// ---- workspace: every region of a call, walked once.  base == null: sizes only
struct SkWorkspace {
    float *u, *v0, *v1;   // [B][M+1]; v ping-pong [B][ldS + 4]
    float *pm, *ps;       // [B][chunks][ldS] column partials (re-used as pv / pi by the final sweep)
    float *upm, *ups;     // [B][chunks]
    float* max0;          // [B][M]
    int* idx0;            // [B][M]
    char* granules;       // granule buffers of the resident kernels (segments run one after the other: each carves its own A | B | U here)
    size_t bytes;         // all of it
};

// geometry of the resident kernel for a problem size and `slots` co-resident workgroups
struct ResidentPlan {
    int G, n_res, cs;
    size_t bytesA, bytesB, bytesU;
};
static ResidentPlan resident_plan(int B, int M, int N, int slots, int rows_per_wg = 0) {
    ResidentPlan r;
    const int rows = rows_per_wg > 0 ? rows_per_wg : skr_rows(round_up(N, 4));
    r.G = (M + rows - 1) / rows;
    r.n_res = std::max(1, std::min(B, slots / std::max(r.G, 1)));
    r.cs = (N + r.G - 1) / r.G;
    auto al = [](size_t n) { return (n + 255) & ~size_t(255); };
    r.bytesA = al((size_t)r.n_res * r.G * r.G * r.cs * 8);
    r.bytesB = al((size_t)r.n_res * r.G * r.cs * 8);
    r.bytesU = al((size_t)r.n_res * 2 * r.G * 8);
    return r;
}
static size_t resident_ws_bytes(int B, int M, int N, int slots) {
    if (round_up(N, 4) > 2048) return 0;
    // n_res grows with the slot count until it reaches B: the largest plan is the one at `slots`
    const ResidentPlan r = resident_plan(B, M, N, slots);
    return r.bytesA + r.bytesB + r.bytesU + 256;
}

static SkWorkspace carve_workspace(char* base, int B, int M, int N, int64_t ldS) {
    const int chunks = (M + SK_ROWS - 1) / SK_ROWS;
    size_t off = 0;
    auto take = [&](size_t bytes) { char* r = base ? base + off : nullptr; off += (bytes + 255) & ~size_t(255); return r; };
    auto floats = [&](size_t n) { return (float*)take(n * 4); };
    SkWorkspace w;
    w.u = floats((size_t)B * (M + 1));
    w.v0 = floats((size_t)B * (ldS + 4));
    w.v1 = floats((size_t)B * (ldS + 4));
    w.pm = floats((size_t)B * chunks * ldS);
    w.ps = floats((size_t)B * chunks * ldS);
    w.upm = floats((size_t)B * chunks);
    w.ups = floats((size_t)B * chunks);
    w.max0 = floats((size_t)B * M);
    w.idx0 = (int*)floats((size_t)B * M);
    w.granules = take(resident_ws_bytes(B, M, N, 1024));  // (upper bound: 4 workgroups / CU)
    w.bytes = off;
    return w;
}

size_t sinkhorn_ws_bytes(int B, int M, int N) { return carve_workspace(nullptr, B, M, N, round_up(N, 4)).bytes; }

// ---- the launcher's plan, shared by launch_sinkhorn and the e2emv_sinkhorn_plan query (bench.py reports it instead of re-deriving it)
struct SkSegment { int b0 = 0, n = 0; SkKernel k; int resident = 0; };
struct SkPlan { int n_seg = 0; SkSegment seg[2]; };  // n_seg == 0: the log-domain launch chain
// sinkhorn_resident128w as the automatic 128-row kernel at 513 .. 1024 columns (0.71 against 0.87 ms of the default workload's
// step), and what one round of it costs in eighths of a round of the 64-row kernel.  Measured at 1024 x 1024, 100 iterations, ms
// per call: 16 problems 0.619 against 0.574 on the 64-row kernel (1.08), 32 problems 0.661 (1.22 of a full 64-row round of 0.54);
// 80 problems as 64 + 16 on the 64-row kernel 1.874, all three rounds on this kernel 1.921 - a remainder of one 64-row round
// stays there, two or more go to one more round of this kernel (profiles/sinkhorn_rows128w.log)
constexpr bool SK_AUTO_ROWS128W = true;
constexpr int SK_ROWS128W_ROUND_8THS = 10;  // 1.22, rounded up

// `count`: this is a real call (the demotion counters of the context advance); false for the query
static int plan_sinkhorn(e2emv_ctx* ctx, int B, int M, int N, int64_t ldS, int iters, bool count, SkPlan& plan) {
    plan = SkPlan{};
    bool resident = iters >= 1 && ldS <= 2048;
    // which kernel: the context's pin (e2emv_set_sinkhorn_kernel; initialised ONCE from E2EMV_SINKHORN when the context is made)
    const int pin = ctx->sinkhorn_kernel;
    if (pin == E2EMV_SINKHORN_STREAM) resident = false;
    // once a call of this context reported scores outside the exponential-domain kernel's range (e2emv_sync / e2emv_get_stats),
    // the model at hand is served by the log-domain chain: slower, no range limit
    // (demotion needs two observed range events; after 16 calls on the chain the resident kernel gets another try - a model whose
    // scores really are out of its range is demoted again by the next event)
    if (ctx->sinkhorn_stream) {
        if (!count) resident = false;
        else if (++ctx->sk_stream_calls > 16) { ctx->sinkhorn_stream = false; ctx->sk_stream_calls = 0; ctx->sk_range_strikes = 1; }
        else resident = false;
    }
    if (!resident) return E2EMV_OK;
    // A call is served by one or two resident launches (segments of the batch): the kernels with K in registers addressed by number
    // (sinkhorn_resident128 / 128w at 513 .. 1024 columns, sinkhorn_resident2k at 1025 .. 2048: twice the rows per workgroup, twice the
    // problems resident, a round 1.6 - 1.75 times as long (sinkhorn_resident128w: 1.1 - 1.25) - measured 0.83 - 0.94 against 0.51 - 0.53 ms per 100 iterations at
    // 1024 x 1024, 1.21 against 0.80 at 2048 x 2048) take every FULL round of theirs, the remainder goes to whichever is cheaper:
    // rounds of the compiler-allocated kernel, or one more round of the big one.  80 problems of 1024 x 1024 = 64 + 16.
    // Pin rows64: never the big kernels; rows128: the big kernel for the whole batch whenever the shape allows it - with a pin a
    // problem's result does not depend on its batch neighbours (tests compare a problem alone with the same problem in a batch).
    // At 513 .. 1024 columns there are two 128-row kernels: sinkhorn_resident128 (4 waves) is what the pin rows128 means,
    // sinkhorn_resident128w (8 waves, two per SIMD: the row pass at the full rate of the vector pipe) is the pin rows128w and what
    // the launcher takes by itself (SK_AUTO_ROWS128W).  The two add a workgroup's column partials in different orders.
    SkKernel kbase, kbig;
    const bool wide = pin == E2EMV_SINKHORN_ROWS128W || (pin == E2EMV_SINKHORN_AUTO && SK_AUTO_ROWS128W);
    const bool full = N == ldS && N == KT_of(ldS) * 256;
    // granule pairs (16-byte exchange stores / loads): a thread must own an even number of columns and a consumer's column
    // slice must be even
    const int G0 = (M + skr_rows(ldS) - 1) / skr_rows(ldS);
    const bool pairs = KT_of(ldS) >= 4 && ((N + G0 - 1) / G0) % 2 == 0;
    kbase = sinkhorn_resident_kernel(KT_of(ldS), full, pairs);
    if (KT_of(ldS) == 4) {
        const int G128 = (M + 127) / 128, cs128 = (N + G128 - 1) / G128;
        if (cs128 % 2 == 0 && G128 <= 16) kbig = wide ? sinkhorn_regs2_kernel(full && M % 128 == 0, G128) : sinkhorn_regs_kernel(4, full && M % 128 == 0);  // (full rows AND columns)
    } else if (KT_of(ldS) == 8) {
        const int G2k = (M + 63) / 64, cs2k = (N + G2k - 1) / G2k;
        if (cs2k % 2 == 0 && G2k <= 64) kbig = sinkhorn_regs_kernel(8, full && M % 64 == 0);
    }
    static std::map<std::pair<int, const void*>, int> occupancy;  // (device, kernel) -> resident workgroups per CU
    static std::mutex occupancy_mu;
    for (SkKernel* k : {&kbase, &kbig}) {
        if (!k->fn) continue;
        std::lock_guard<std::mutex> lk(occupancy_mu);
        auto it = occupancy.find({ctx->device, k->fn});
        if (it == occupancy.end()) {
            int nb = 0;
            if (k->lds > 48 * 1024 && ensure_dynamic_lds(ctx, k->fn, k->lds) != E2EMV_OK) {
                (void)hipGetLastError();  // a device with less LDS: the streaming chain serves the call
                nb = 0;
            } else if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k->fn, k->threads, k->lds) != hipSuccess) {
                (void)hipGetLastError();
                nb = 0;
            }
            it = occupancy.emplace(std::make_pair(ctx->device, k->fn), std::min(nb, 2)).first;
        }
        k->wg_per_cu = it->second;
        const int G = (M + k->rows - 1) / k->rows;
        if (k->wg_per_cu < 1 || G > k->wg_per_cu * ctx->num_cus) k->fn = nullptr;  // cannot hold a problem's workgroups at once
    }
    if (!kbase.fn) { if (kbig.fn) kbase = kbig; else return E2EMV_OK; }
    auto res_of = [&](const SkKernel& k) { return std::max(1, (k.wg_per_cu * ctx->num_cus) / std::max((M + k.rows - 1) / k.rows, 1)); };
    auto add = [&](int b0, int n, const SkKernel& k) {
        SkSegment& sg = plan.seg[plan.n_seg++];
        sg.b0 = b0; sg.n = n; sg.k = k; sg.resident = std::min(n, res_of(k));
    };
    if (!kbig.fn || kbase.big || pin == E2EMV_SINKHORN_ROWS64) {
        add(0, B, kbase);
    } else if (pin == E2EMV_SINKHORN_ROWS128 || pin == E2EMV_SINKHORN_ROWS128W) {
        add(0, B, kbig);
    } else {
        const int res_big = res_of(kbig), res_base = res_of(kbase);
        int n_big = (B / res_big) * res_big;   // every full round of the big kernel (it holds twice the problems at < 2 x the time)
        const int rem = B - n_big;
        // the remainder too: one round of the big kernel (1.6 base rounds; sinkhorn_resident128w: SK_ROWS128W_ROUND_8THS / 8) against
        // two or more of the base kernel
        const int big_round_8ths = (wide && KT_of(ldS) == 4) ? SK_ROWS128W_ROUND_8THS : 13;
        if (rem > 0 && 8 * ((rem + res_base - 1) / res_base) > big_round_8ths) n_big = B;
        if (n_big > 0) add(0, n_big, kbig);
        if (n_big < B) add(n_big, B - n_big, kbase);
    }
    return E2EMV_OK;
}

// every polled word of a resident launch starts from 0 (epochs count from 1), and so does the launch's give-up flag
__global__ __launch_bounds__(256) void skr_zero_kernel(uint4* buf, size_t n16, unsigned* flag) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n16; i += (size_t)gridDim.x * 256) buf[i] = uint4{0u, 0u, 0u, 0u};
    if (blockIdx.x == 0 && threadIdx.x == 0) flag[0] = 0u;
}

static void launch_resident(const void* fn, dim3 grid, dim3 block, size_t lds, hipStream_t s, SkResParams& par) {
    void* args[] = {&par};
    (void)hipLaunchKernel(fn, grid, block, args, lds, s);
}

int launch_sinkhorn(e2emv_ctx* ctx, int B, int M, int N, const float* S, int64_t ldS, float alpha, int iters,
                    float match_thr, const SinkhornOut& out, char* ws, hipStream_t s) {
    if (B <= 0 || M <= 0 || N <= 0) return set_err(ctx, E2EMV_ESHAPE, "sinkhorn: empty problem");
    if (ldS % 4 || ldS < N || ((uintptr_t)S % 16)) return set_err(ctx, E2EMV_ESHAPE, "sinkhorn: score rows must be 16-byte aligned");
    if (ldS > 2048) return set_err(ctx, E2EMV_ESHAPE, "sinkhorn: N=%d > 2048 keypoints not supported", N);
    if ((size_t)(2 * M + N) * 4 > 60000) return set_err(ctx, E2EMV_ESHAPE, "sinkhorn: M=%d too large", M);
    SkParams p{};
    p.S = S; p.ldS = ldS; p.M = M; p.N = N;
    p.chunks = (M + SK_ROWS - 1) / SK_ROWS;
    p.alpha = alpha;
    p.norm = -logf((float)(M + N));
    const SkWorkspace wsp = carve_workspace(ws, B, M, N, ldS);
    p.u = wsp.u;
    p.ldV = ldS + 4;
    p.pm = wsp.pm; p.ps = wsp.ps; p.upm = wsp.upm; p.ups = wsp.ups;
    p.max0 = wsp.max0; p.idx0 = wsp.idx0;
    p.pv = p.pm;
    p.pi = (int*)p.ps;
    const int gb = out.group_batch > 0 ? out.group_batch : B;
    if (out.n_groups < 1 || out.n_groups > kMaxGroups || gb * out.n_groups != B)
        return set_err(ctx, E2EMV_EINVAL, "sinkhorn: %d groups x %d != batch %d", out.n_groups, gb, B);
    p.group_batch = gb;
    bool want_match = false;
    for (int g = 0; g < kMaxGroups; ++g) {
        p.logZ[g] = g < out.n_groups ? out.logZ[g] : nullptr;
        if (g < out.n_groups && (out.m0[g] || out.m1[g] || out.ms0[g] || out.ms1[g])) want_match = true;
    }
    p.v = wsp.v0;
    p.v_next = wsp.v1;

    // ---- resident path: all iterations in one launch (S read once); the streaming chain below is the fallback for
    // iters == 0, for the `stream` pin and for devices that cannot hold a problem's workgroups at once (plan_sinkhorn above)
    SkPlan plan;
    if (int rc_p = plan_sinkhorn(ctx, B, M, N, ldS, iters, true, plan)) return rc_p;
    if (plan.n_seg > 0) {
        if (int rc_f = ensure_flags(ctx)) return rc_f;
        const SkSegment* seg = plan.seg;
        const int n_seg = plan.n_seg;
        for (int si = 0; si < n_seg; ++si) {
            const SkKernel& k = seg[si].k;
            const int b0 = seg[si].b0, nb = seg[si].n;
            const ResidentPlan rp = resident_plan(nb, M, N, k.wg_per_cu * ctx->num_cus, k.rows);
            SkResParams rpar{};
            rpar.S = S + (int64_t)b0 * M * ldS; rpar.ldS = ldS; rpar.M = M; rpar.N = N; rpar.B = nb; rpar.iters = iters;
            rpar.alpha = alpha; rpar.norm = p.norm;
            rpar.G = rp.G; rpar.n_res = rp.n_res; rpar.cs = rp.cs;
            char* gw = wsp.granules;
            rpar.bufA = (u64*)gw; gw += rp.bytesA;
            rpar.bufB = (u64*)gw; gw += rp.bytesB;
            rpar.bufU = (u64*)gw; gw += rp.bytesU;
            rpar.timeout = ctx->d_flags;
            rpar.u = p.u + (int64_t)b0 * (M + 1); rpar.v = p.v + (int64_t)b0 * p.ldV; rpar.ldV = p.ldV;
            // every polled word starts from 0 in every launch (epochs count from 1)
            // (ONE launch for the granule buffers and the give-up flag: two hipMemsetAsync were two fill kernels of ~14 us each per segment)
            hipLaunchKernelGGL(skr_zero_kernel, dim3((unsigned)std::min<size_t>(1024, ((rp.bytesA + rp.bytesB + rp.bytesU) / 16 + 255) / 256)), dim3(256), 0, s,
                               reinterpret_cast<uint4*>(wsp.granules), (rp.bytesA + rp.bytesB + rp.bytesU) / 16, ctx->d_flags);
            E2EMV_CHECK_LAUNCH(ctx, "skr_zero_kernel");
            launch_resident(k.fn, dim3((unsigned)(rp.n_res * rp.G)), dim3(k.threads), k.lds, s, rpar);
            E2EMV_CHECK_LAUNCH(ctx, "sinkhorn_resident");
        }
        if (seg[0].k.big) ++ctx->stat_sinkhorn_rows128;
        // problems the exponential-domain kernel could not finish are re-solved in the log domain before anything reads u, v
        sk_rescue(p, B, iters, ctx->d_flags, s);
        E2EMV_CHECK_LAUNCH(ctx, "sinkhorn_rescue");
    } else {
        sk_stream_iterate(p, B, iters, s);
        if (ensure_flags(ctx) == E2EMV_OK) sk_check_finite(p, B, ctx->d_flags, s);
    }
    sk_final_sweep(p, B, s);  // logZ + fused arg-max from the final potentials (one more read of the scores)
    E2EMV_CHECK_LAUNCH(ctx, "sinkhorn kernels");
    if (want_match) {
        sk_match(p, B, match_thr, out, s);
        E2EMV_CHECK_LAUNCH(ctx, "match_finalize");
    }
    return E2EMV_OK;
}

}  // namespace e2emv

using namespace e2emv;

extern "C" int e2emv_set_sinkhorn_kernel(e2emv_ctx* ctx, int kernel) {
    if (!ctx) return E2EMV_EINVAL;
    E2EMV_LOCK(ctx);
    if (kernel < E2EMV_SINKHORN_AUTO || kernel > E2EMV_SINKHORN_ROWS128W) return set_err(ctx, E2EMV_EINVAL, "set_sinkhorn_kernel: %d (E2EMV_SINKHORN_AUTO .. _ROWS128W)", kernel);
    ctx->sinkhorn_kernel = kernel;
    return E2EMV_OK;
}

extern "C" int e2emv_sinkhorn_plan(e2emv_ctx* ctx, int B, int M, int N, int iters, int* plan_out, int n) {
    if (!ctx || !plan_out || n < 1) return E2EMV_EINVAL;
    E2EMV_LOCK(ctx);
    (void)hipSetDevice(ctx->device);
    if (B <= 0 || M <= 0 || N <= 0 || iters < 0) return set_err(ctx, E2EMV_ESHAPE, "sinkhorn_plan: bad sizes");
    SkPlan plan;
    if (int rc = plan_sinkhorn(ctx, B, M, N, round_up(N, 4), iters, false, plan)) return rc;
    for (int i = 0; i < n; ++i) plan_out[i] = 0;
    plan_out[0] = plan.n_seg;
    for (int si = 0; si < plan.n_seg && 1 + 4 * (si + 1) <= n; ++si) {
        const SkSegment& sg = plan.seg[si];
        plan_out[1 + 4 * si + 0] = sg.k.rows;                               // rows of a problem per workgroup
        plan_out[1 + 4 * si + 1] = sg.n;                                    // problems of the batch this launch takes
        plan_out[1 + 4 * si + 2] = sg.resident;                             // problems resident at a time
        plan_out[1 + 4 * si + 3] = (sg.n + sg.resident - 1) / sg.resident;  // rounds
    }
    return E2EMV_OK;
}

extern "C" int e2emv_sinkhorn(e2emv_ctx* ctx, int B, int M, int N, const float* d_scores, float bin_score, int iters,
                              float* d_logZ, void* stream) {
    if (!ctx || !d_scores || !d_logZ) return E2EMV_EINVAL;
    E2EMV_ENTER(ctx, stream);
    if (B <= 0 || M <= 0 || N <= 0 || iters < 0) return set_err(ctx, E2EMV_ESHAPE, "sinkhorn: bad sizes");
    hipStream_t s = (hipStream_t)stream;
    const int ldS = round_up(N, 4);
    const bool need_copy = (N % 4 != 0) || ((uintptr_t)d_scores % 16 != 0);
    size_t need = sinkhorn_ws_bytes(B, M, N) + (need_copy ? (((size_t)B * M * ldS * 4 + 255) & ~size_t(255)) : 0);
    int rc = ws_reserve(ctx, need);
    if (rc) return rc;
    char* ws = ctx->d_ws;
    const float* S = d_scores;
    prof_begin(ctx, PS_SINKHORN, s);
    if (need_copy) {
        float* Sp = (float*)ws;
        ws += ((size_t)B * M * ldS * 4 + 255) & ~size_t(255);
        sk_pad_copy_rows(d_scores, (int64_t)B * M, N, Sp, (int64_t)ldS, s);
        S = Sp;
    }
    SinkhornOut out;
    out.logZ[0] = d_logZ;
    rc = launch_sinkhorn(ctx, B, M, N, S, ldS, bin_score, iters, 0.f, out, ws, s);
    prof_end(ctx, s);
    return rc;
}
