// Context lifecycle, memory helpers, workspace arena, the HIP-event profiling hooks, statistics and the settings API of
// libe2emv.so.  (Weights: weights.hip.)
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>

#include "common.h"

namespace e2emv {

int set_err(e2emv_ctx* ctx, int code, const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    if (ctx) ctx->err = buf;
    return code;
}

int ensure_dynamic_lds(e2emv_ctx* ctx, const void* kernel, size_t bytes) {
    static std::map<std::pair<int, const void*>, size_t> done;
    static std::mutex mu;
    std::lock_guard<std::mutex> lk(mu);
    size_t& have = done[{ctx->device, kernel}];
    if (have >= bytes) return E2EMV_OK;
    E2EMV_HIP(ctx, hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    have = bytes;
    return E2EMV_OK;
}

int ensure_flags(e2emv_ctx* ctx) {
    if (ctx->d_flags) return E2EMV_OK;
    E2EMV_HIP(ctx, hipMalloc((void**)&ctx->d_flags, 256));
    E2EMV_HIP(ctx, hipMemset(ctx->d_flags, 0, 256));
    E2EMV_NULL_STREAM_FENCE(ctx);
    return E2EMV_OK;
}

int ws_reserve(e2emv_ctx* ctx, size_t bytes) {
    // every entry point that carves the arena comes through here first: whatever the previous call left in it (the matched
    // descriptors e2emv_get_descriptors hands out) is about to be overwritten, or freed by the regrow below
    ctx->last_mdesc = nullptr;
    if (bytes <= ctx->ws_bytes) return E2EMV_OK;
    E2EMV_HIP(ctx, hipDeviceSynchronize());
    if (ctx->d_ws) E2EMV_HIP(ctx, hipFree(ctx->d_ws));
    ctx->d_ws = nullptr;
    ctx->ws_bytes = 0;
    size_t want = bytes + bytes / 8 + (size_t(1) << 20);
    void* p = nullptr;
    if (hipMalloc(&p, want) != hipSuccess) {
        (void)hipGetLastError();
        return set_err(ctx, E2EMV_ENOMEM, "workspace allocation of %zu bytes failed", want);
    }
    // padded rows of activation buffers must start finite (see forward.hip)
    E2EMV_HIP(ctx, hipMemset(p, 0, want));
    E2EMV_NULL_STREAM_FENCE(ctx);
    ctx->d_ws = static_cast<char*>(p);
    ctx->ws_bytes = want;
    return E2EMV_OK;
}

static hipEvent_t take_event(e2emv_ctx* ctx) {
    if (!ctx->event_pool.empty()) {
        hipEvent_t e = ctx->event_pool.back();
        ctx->event_pool.pop_back();
        return e;
    }
    hipEvent_t e;
    (void)hipEventCreate(&e);
    return e;
}

void prof_begin(e2emv_ctx* ctx, int slot, hipStream_t s) {
    if (!ctx->prof) return;
    if (!ctx->prof_events.empty() && ctx->prof_events.back().slot == slot && ctx->prof_stream == s) {
        ++ctx->prof_events.back().launches;  // same family as the launch before: the interval goes on
        return;
    }
    ProfEvent pe;
    pe.ev = take_event(ctx);
    pe.slot = slot;
    pe.launches = 1;
    (void)hipEventRecord(pe.ev, s);
    ctx->prof_stream = s;
    ctx->prof_events.push_back(pe);
}

void prof_close(e2emv_ctx* ctx) {
    if (!ctx->prof || ctx->prof_events.empty() || ctx->prof_events.back().slot < 0) return;
    ProfEvent pe;
    pe.ev = take_event(ctx);
    pe.slot = -1;
    pe.launches = 0;
    (void)hipEventRecord(pe.ev, ctx->prof_stream);
    ctx->prof_events.push_back(pe);
}

CallGuard::~CallGuard() { prof_close(c); }

}  // namespace e2emv

using namespace e2emv;

static const char* kProfNames[PS_COUNT] = {"ingest", "gemm", "attention", "score_gemm", "sinkhorn",
                                           "match", "conf", "w8pt", "misc", "gemm_qkv", "gemm_mlp0", "gemm_mlp1", "gemm_chain"};

extern "C" {

int e2emv_version(void) { return E2EMV_ABI_VERSION; }

int e2emv_create(e2emv_ctx** out, int device) {
    if (!out) return E2EMV_EINVAL;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
        (void)hipGetLastError();
        return E2EMV_EHIP;
    }
    if (device < 0 || device >= n) return E2EMV_EINVAL;
    if (hipSetDevice(device) != hipSuccess) return E2EMV_EHIP;
    hipDeviceProp_t p;
    if (hipGetDeviceProperties(&p, device) != hipSuccess) return E2EMV_EHIP;
    if (strncmp(p.gcnArchName, "gfx950", 6) != 0) return E2EMV_EHIP;  // kernels are gfx950-only
    e2emv_ctx* ctx = new (std::nothrow) e2emv_ctx();
    if (!ctx) return E2EMV_ENOMEM;
    ctx->device = device;
    ctx->num_cus = p.multiProcessorCount;
    if (const char* e = getenv("E2EMV_F16X2_KERNELS")) {  // r4: a launch per GEMM (the chain's A/B arm and the T = 5 path); other values: ignored
        if (strcmp(e, "r4") == 0) ctx->gemm_chain = 0;
    }

    if (const char* e = getenv("E2EMV_KENC")) {  // unfused: the keypoint encoder as a launch per stage (the fused kernel's A/B arm)
        if (strcmp(e, "unfused") == 0) ctx->kenc_fused = false;
    }
    if (const char* e = getenv("E2EMV_SINKHORN")) {  // the Sinkhorn kernel pin (e2emv_set_sinkhorn_kernel): read here, once
        ctx->sinkhorn_kernel = strcmp(e, "rows64") == 0 ? E2EMV_SINKHORN_ROWS64 : strcmp(e, "rows128") == 0 ? E2EMV_SINKHORN_ROWS128
                               : strcmp(e, "rows128w") == 0 ? E2EMV_SINKHORN_ROWS128W
                               : strcmp(e, "stream") == 0 ? E2EMV_SINKHORN_STREAM : E2EMV_SINKHORN_AUTO;
    }

    // default arithmetic of the dense GNN contractions: the split-operand fp16 x 2 path (22-bit operands, fp32 accumulate;
    // every parity test runs in all three modes at the same bar); E2EMV_PRECISION=bf16x3 selects the 24-bit bf16 x 3
    // split, =f32 the exact fp32-MFMA kernels
    ctx->precision = E2EMV_PRECISION_F16X2;
    if (const char* e = getenv("E2EMV_PRECISION")) {
        ctx->precision = E2EMV_PRECISION_F32;
        if (strcmp(e, "bf16x3") == 0) ctx->precision = E2EMV_PRECISION_BF16X3;
        if (strcmp(e, "f16x2") == 0) ctx->precision = E2EMV_PRECISION_F16X2;
    }
    *out = ctx;
    return E2EMV_OK;
}

void e2emv_destroy(e2emv_ctx* ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    (void)hipDeviceSynchronize();
    e2emv::train_free(ctx);
    e2emv::optim_free(ctx);
    e2emv::image_front_free(ctx);
    e2emv::image_front_gray_free(ctx);
    if (ctx->d_ws) (void)hipFree(ctx->d_ws);
    if (ctx->d_warena) (void)hipFree(ctx->d_warena);
    if (ctx->d_w3arena) (void)hipFree(ctx->d_w3arena);
    if (ctx->d_sparena) (void)hipFree(ctx->d_sparena);
    if (ctx->d_attn_part) (void)hipFree(ctx->d_attn_part);
    if (ctx->d_flags) (void)hipFree(ctx->d_flags);
    if (ctx->d_dummy) (void)hipFree(ctx->d_dummy);
    for (auto& pe : ctx->prof_events) (void)hipEventDestroy(pe.ev);
    for (auto e : ctx->event_pool) (void)hipEventDestroy(e);
    delete ctx;
}

const char* e2emv_last_error(const e2emv_ctx* ctx) { return ctx ? ctx->err.c_str() : "null context"; }

int e2emv_malloc(e2emv_ctx* ctx, void** d_ptr, size_t bytes) {
    if (!ctx || !d_ptr) return E2EMV_EINVAL;
    E2EMV_LOCK(ctx);
    (void)hipSetDevice(ctx->device);
    if (hipMalloc(d_ptr, bytes ? bytes : 1) != hipSuccess) {
        (void)hipGetLastError();
        return set_err(ctx, E2EMV_ENOMEM, "hipMalloc(%zu) failed", bytes);
    }
    return E2EMV_OK;
}

int e2emv_free(e2emv_ctx* ctx, void* d_ptr) {
    if (!ctx) return E2EMV_EINVAL;
    E2EMV_LOCK(ctx);
    if (d_ptr) E2EMV_HIP(ctx, hipFree(d_ptr));
    return E2EMV_OK;
}

int e2emv_h2d(e2emv_ctx* ctx, void* d_dst, const void* src, size_t bytes, void* stream) {
    if (!ctx || (!d_dst && bytes) || (!src && bytes)) return E2EMV_EINVAL;
    E2EMV_ENTER(ctx, stream);
    E2EMV_HIP(ctx, hipMemcpyAsync(d_dst, src, bytes, hipMemcpyHostToDevice, (hipStream_t)stream));
    return E2EMV_OK;
}

int e2emv_d2h(e2emv_ctx* ctx, void* dst, const void* d_src, size_t bytes, void* stream) {
    if (!ctx || (!dst && bytes) || (!d_src && bytes)) return E2EMV_EINVAL;
    E2EMV_ENTER(ctx, stream);
    E2EMV_HIP(ctx, hipMemcpyAsync(dst, d_src, bytes, hipMemcpyDeviceToHost, (hipStream_t)stream));
    return E2EMV_OK;
}

// Rescue counts the host has just read from the device: `range` problems whose scalings left the exponential-domain kernel's
// range (a property of the model: the second observation moves the context to the log-domain chain), `timeouts` problems given
// up because an inter-workgroup wait ran out (contention, e.g. a co-tenant process: counted, never a reason to demote)
static void note_rescues(e2emv_ctx* ctx, unsigned range, unsigned timeouts) {
    const unsigned zero = 0;
    if (range) {
        (void)hipMemcpy(ctx->d_flags + 3, &zero, sizeof(zero), hipMemcpyHostToDevice);
        ctx->stat_sinkhorn_rescued += range;
        if (++ctx->sk_range_strikes >= 2) { ctx->sinkhorn_stream = true; ctx->sk_stream_calls = 0; }
    }
    if (timeouts) {
        (void)hipMemcpy(ctx->d_flags + 6, &zero, sizeof(zero), hipMemcpyHostToDevice);
        ctx->stat_sinkhorn_rescued += timeouts;
        ctx->stat_sinkhorn_timeouts += timeouts;
    }
}

int e2emv_sync(e2emv_ctx* ctx, void* stream) {
    if (!ctx) return E2EMV_EINVAL;
    E2EMV_ENTER(ctx, stream);
    E2EMV_HIP(ctx, hipStreamSynchronize((hipStream_t)stream));
    if (ctx->d_flags) {
        // [1]: Sinkhorn problems whose potentials are non-finite even after the log-domain rescue pass = non-finite scores
        // [3]: problems the rescue pass re-solved (finite outputs; a context that keeps needing it moves to the log-domain chain)
        unsigned f[7] = {0, 0, 0, 0, 0, 0, 0};
        E2EMV_HIP(ctx, hipMemcpy(f, ctx->d_flags, sizeof(f), hipMemcpyDeviceToHost));
        note_rescues(ctx, f[3], f[6]);
        if (f[1]) {
            unsigned zero = 0;
            (void)hipMemcpy(ctx->d_flags + 1, &zero, sizeof(zero), hipMemcpyHostToDevice);
            ctx->stat_sinkhorn_bad += f[1];
            return set_err(ctx, E2EMV_EHIP, "sinkhorn: %u problem(s) with non-finite scores (an activation left the range of the arithmetic "
                           "mode, or the inputs were non-finite) - the outputs of those problems are NaN/inf", f[1]);
        }
    }
    E2EMV_NULL_STREAM_FENCE(ctx);  // (the flag resets above)
    return E2EMV_OK;
}

int e2emv_set_precision(e2emv_ctx* ctx, int precision) {
    if (!ctx) return E2EMV_EINVAL;
    E2EMV_LOCK(ctx);
    if (precision != E2EMV_PRECISION_F32 && precision != E2EMV_PRECISION_BF16X3 && precision != E2EMV_PRECISION_F16X2)
        return set_err(ctx, E2EMV_EINVAL, "unknown precision %d", precision);
    ctx->precision = precision;
    return E2EMV_OK;
}

int e2emv_get_stats(e2emv_ctx* ctx, uint64_t* stats, int n, int reset) {
    if (!ctx || !stats || n < 0) return E2EMV_EINVAL;
    E2EMV_LOCK(ctx);
    (void)hipSetDevice(ctx->device);
    E2EMV_HIP(ctx, hipDeviceSynchronize());
    unsigned f[7] = {0, 0, 0, 0, 0, 0, 0};
    if (ctx->d_flags) E2EMV_HIP(ctx, hipMemcpy(f, ctx->d_flags, sizeof(f), hipMemcpyDeviceToHost));
    ctx->stat_sinkhorn_bad += f[1];
    if (ctx->d_flags) note_rescues(ctx, f[3], f[6]);
    const uint64_t v[7] = {(uint64_t)f[2], ctx->stat_sinkhorn_bad, ctx->stat_sinkhorn_rescued, (uint64_t)f[5], ctx->stat_sinkhorn_timeouts, ctx->stat_sinkhorn_rows128,
                           ctx->stat_kenc_fused};
    for (int i = 0; i < n; ++i) stats[i] = i < 7 ? v[i] : 0;
    if (ctx->d_flags && f[1]) E2EMV_HIP(ctx, hipMemset(ctx->d_flags + 1, 0, sizeof(unsigned)));  // moved into the host-side total
    if (reset) {
        ctx->stat_sinkhorn_bad = 0;
        ctx->stat_sinkhorn_rescued = 0;
        ctx->stat_sinkhorn_timeouts = 0;
        ctx->stat_sinkhorn_rows128 = 0;
        ctx->stat_kenc_fused = 0;
        ctx->sk_range_strikes = 0;
        ctx->sk_stream_calls = 0;
        ctx->sinkhorn_stream = false;  // (a reset also returns the Sinkhorn to the resident kernel)
        if (ctx->d_flags) E2EMV_HIP(ctx, hipMemset(ctx->d_flags + 2, 0, sizeof(unsigned)));
        if (ctx->d_flags) E2EMV_HIP(ctx, hipMemset(ctx->d_flags + 5, 0, sizeof(unsigned)));
    }
    E2EMV_NULL_STREAM_FENCE(ctx);
    return E2EMV_OK;
}

int e2emv_set_f16x2_kernels(e2emv_ctx* ctx, int generation) {
    if (!ctx) return E2EMV_EINVAL;
    E2EMV_LOCK(ctx);
    const bool always = generation == 105;  // generation 5 with the GEMM chain on every shape that allows it (tests, A/B runs)
    if (always) generation = 5;
    if (generation != 4 && generation != 5)
        return set_err(ctx, E2EMV_EINVAL, "f16x2 kernel generation %d: this library selects 5 (default), 105 or 4 (generations 2 and 3 are retired)", generation);
    ctx->gemm_chain = generation == 5 ? (always ? 2 : 1) : 0;
    return E2EMV_OK;
}

int e2emv_set_attention_key_split(e2emv_ctx* ctx, int on) {
    if (!ctx) return E2EMV_EINVAL;
    E2EMV_LOCK(ctx);
    ctx->attn_key_split = on != 0;
    return E2EMV_OK;
}

int e2emv_set_kenc_fused(e2emv_ctx* ctx, int on) {
    if (!ctx) return E2EMV_EINVAL;
    E2EMV_LOCK(ctx);
    ctx->kenc_fused = on != 0;
    return E2EMV_OK;
}

int e2emv_set_split_min_rows(e2emv_ctx* ctx, int64_t min_rows) {
    if (!ctx) return E2EMV_EINVAL;
    E2EMV_LOCK(ctx);
    ctx->split_min_rows = min_rows < 0 ? -1 : min_rows;
    return E2EMV_OK;
}

int e2emv_get_precision(e2emv_ctx* ctx, int* precision) {
    if (!ctx || !precision) return E2EMV_EINVAL;
    E2EMV_LOCK(ctx);
    *precision = ctx->precision;
    return E2EMV_OK;
}

int e2emv_profile(e2emv_ctx* ctx, int enable) {
    if (!ctx) return E2EMV_EINVAL;
    E2EMV_LOCK(ctx);
    if (!enable) prof_close(ctx);
    ctx->prof = enable != 0;
    return E2EMV_OK;
}

int e2emv_profile_read(e2emv_ctx* ctx, float* ms, int64_t* launches, int n_slots, int reset) {
    if (!ctx) return E2EMV_EINVAL;
    E2EMV_LOCK(ctx);
    prof_close(ctx);
    E2EMV_HIP(ctx, hipDeviceSynchronize());
    for (size_t i = 0; i < ctx->prof_events.size(); ++i) {
        const ProfEvent& pe = ctx->prof_events[i];
        float t = 0.f;
        if (pe.slot >= 0 && pe.slot < E2EMV_PROF_SLOTS && i + 1 < ctx->prof_events.size()) {
            if (hipEventElapsedTime(&t, pe.ev, ctx->prof_events[i + 1].ev) == hipSuccess) {
                ctx->prof_ms[pe.slot] += t;
                ctx->prof_n[pe.slot] += pe.launches;
            } else {
                (void)hipGetLastError();
            }
        }
        ctx->event_pool.push_back(pe.ev);
    }
    ctx->prof_events.clear();
    for (int i = 0; i < n_slots && i < E2EMV_PROF_SLOTS; ++i) {
        if (ms) ms[i] = ctx->prof_ms[i];
        if (launches) launches[i] = ctx->prof_n[i];
    }
    if (reset)
        for (int i = 0; i < E2EMV_PROF_SLOTS; ++i) {
            ctx->prof_ms[i] = 0.f;
            ctx->prof_n[i] = 0;
        }
    return E2EMV_OK;
}

const char* e2emv_profile_name(int slot) { return (slot >= 0 && slot < PS_COUNT) ? kProfNames[slot] : ""; }

}  // extern "C"
