// The optimiser step of the training loop on the device (train.py:419-426 of the reference): the finite-gradient gate
// (has_finite_gradients), clip_grad_value_ and torch.optim.Adam.step() over ALL parameter tensors of a call.
//
//   e2emv_grads_finite   memset(flag) -> grads_finite_kernel                                  (1 launch)
//   e2emv_adam_step      [memset(flag) -> grads_finite_kernel ->] adam_update_kernel -> adam_finish_kernel   (2 or 3 launches)
//
// Work is cut into chunks of E2EMV_OPTIM_CHUNK elements that never cross a tensor; a workgroup of 256 threads takes one chunk at
// a time, 16 bytes per lane and access where the tensor's base pointers allow it, and strides over the chunk list (the grid is
// capped at kMaxGrid workgroups).  Per call the host builds ONE block - tensor records, then the chunk list - and the device copy
// of it is kept between calls: a training loop hands over the same pointers every step, so the block is compared with the last
// one uploaded and copied (pinned buffer, one stream-ordered hipMemcpyAsync) only when it differs.  The block lives in a buffer
// of its own, not in ctx->d_ws: nothing of the shared workspace (the matched descriptors of the last forward) is touched.
//
// Ordering inside a call: the flag is cleared by a memset node in front of the check launch and set by one atomic OR per
// workgroup that saw a non-finite value; the update launch only READS the flag and the step scalars (it computes with step + 1);
// the steps and the counters are advanced by the one-workgroup launch behind it.  No workgroup reads a word another workgroup
// of the same launch writes.
#include <climits>
#include <cstring>

#include "common.h"

namespace e2emv {

namespace {

constexpr int kChunk = E2EMV_OPTIM_CHUNK;
constexpr int kThreads = 256;
constexpr int kMaxGrid = 2048;  // 256 CUs x 8 workgroups: beyond that the chunk list is strided
static_assert(kChunk == 4 * 4 * kThreads, "a full chunk is four 16-byte accesses per lane");

struct OptimTensor {  // 64 bytes
    float* p;
    const float* g;
    float* m;
    float* v;
    float* step;
    int64_t numel;
    float lr;
    int vec;  // every base pointer the kernels touch is 16-byte aligned
    int64_t pad;
};
static_assert(sizeof(OptimTensor) == 64, "tensor record");

struct OptimChunk {
    int tensor;
    int index;  // chunk `index` of that tensor: elements [index * kChunk, min(numel, (index + 1) * kChunk))
};

// The pointers come out of a table, where the compiler only knows them as generic: named as global memory they are read and
// written with global_load / global_store_dwordx4 instead of the flat forms.
typedef float f4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) float gfloat;
typedef __attribute__((address_space(1))) f4 gf4;

__device__ __forceinline__ int nonfinite(float x) { return (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u; }

__global__ __launch_bounds__(kThreads) void grads_finite_kernel(const OptimTensor* __restrict__ tab, const OptimChunk* __restrict__ chunks,
                                                                  int n_chunks, int32_t* __restrict__ flag) {
    int bad = 0;
    for (int c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const OptimChunk ch = chunks[c];
        const OptimTensor& T = tab[ch.tensor];
        const int64_t base = int64_t(ch.index) * kChunk;
        const int64_t left = T.numel - base;
        const int len = left < kChunk ? int(left) : kChunk;
        const gfloat* __restrict__ g = (const gfloat*)(T.g + base);
        int done = 0;
        if (T.vec) {
            const int nvec = len >> 2;
            const gf4* __restrict__ g4 = (const gf4*)(g);
            if (nvec == kChunk / 4) {
                f4 x[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) x[k] = g4[k * kThreads + threadIdx.x];
#pragma unroll
                for (int k = 0; k < 4; ++k) bad |= nonfinite(x[k].x) | nonfinite(x[k].y) | nonfinite(x[k].z) | nonfinite(x[k].w);
            } else {
                for (int i = threadIdx.x; i < nvec; i += kThreads) {
                    const f4 x = g4[i];
                    bad |= nonfinite(x.x) | nonfinite(x.y) | nonfinite(x.z) | nonfinite(x.w);
                }
            }
            done = nvec << 2;
        }
        for (int i = done + threadIdx.x; i < len; i += kThreads) bad |= nonfinite(g[i]);
    }
    if (__syncthreads_or(bad) && threadIdx.x == 0) atomicOr(flag, 1);
}

// beta^n for the integer n a step scalar holds (square and multiply in fp64: at most 2 * 64 products, each 2^-53)
__device__ __forceinline__ double pow_int(double b, unsigned long long n) {
    double r = 1.0;
    while (n) {
        if (n & 1) r *= b;
        b *= b;
        n >>= 1;
    }
    return r;
}

struct AdamScalars {
    float w1, b2, w2, eps, clip;  // 1 - beta1, beta2, 1 - beta2
    float step_size, bc2_sqrt;    // lr / (1 - beta1^t), sqrt(1 - beta2^t): fp64, rounded once
};

// torch.optim.Adam's element (clip_grad_value_ first), in its order of operations, fp32
__device__ __forceinline__ void adam_element(const AdamScalars& a, float& p, float g, float& m, float& v) {
    if (a.clip > 0.f) g = g < -a.clip ? -a.clip : (g > a.clip ? a.clip : g);  // (a NaN stays a NaN, as in torch.clamp)
    m = fmaf(g - m, a.w1, m);
    v = fmaf(a.b2, v, a.w2 * (g * g));
    const float denom = sqrtf(v) / a.bc2_sqrt + a.eps;
    p = p - a.step_size * (m / denom);
}

__device__ __forceinline__ void adam_vec4(const AdamScalars& a, f4& p, const f4& g, f4& m, f4& v) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        float xp = p[j], xm = m[j], xv = v[j];
        adam_element(a, xp, g[j], xm, xv);
        p[j] = xp; m[j] = xm; v[j] = xv;
    }
}

__global__ __launch_bounds__(kThreads) void adam_update_kernel(const OptimTensor* __restrict__ tab, const OptimChunk* __restrict__ chunks,
                                                                 int n_chunks, const int32_t* __restrict__ flag, double beta1, double beta2,
                                                                 float eps, float clip) {
    if (flag && *flag) return;  // a non-finite gradient somewhere in the call: nothing is written
    AdamScalars a;
    a.w1 = float(1.0 - beta1);
    a.b2 = float(beta2);
    a.w2 = float(1.0 - beta2);
    a.eps = eps;
    a.clip = clip;
    for (int c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const OptimChunk ch = chunks[c];
        const OptimTensor& T = tab[ch.tensor];
        const float t = *T.step + 1.f;  // (read only: adam_finish_kernel advances it)
        const unsigned long long ti = t >= 1.f ? (t < 9.2e18f ? (unsigned long long)(t) : ~0ull) : 0ull;  // (a step scalar holds a count)
        a.step_size = float(double(T.lr) / (1.0 - pow_int(beta1, ti)));
        a.bc2_sqrt = float(sqrt(1.0 - pow_int(beta2, ti)));
        const int64_t base = int64_t(ch.index) * kChunk;
        const int64_t left = T.numel - base;
        const int len = left < kChunk ? int(left) : kChunk;
        gfloat* __restrict__ p = (gfloat*)(T.p + base);
        const gfloat* __restrict__ g = (const gfloat*)(T.g + base);
        gfloat* __restrict__ m = (gfloat*)(T.m + base);
        gfloat* __restrict__ v = (gfloat*)(T.v + base);
        int done = 0;
        if (T.vec) {
            const int nvec = len >> 2;
            gf4* __restrict__ p4 = (gf4*)(p);
            const gf4* __restrict__ g4 = (const gf4*)(g);
            gf4* __restrict__ m4 = (gf4*)(m);
            gf4* __restrict__ v4 = (gf4*)(v);
            if (nvec == kChunk / 4) {  // a full chunk: two halves of eight 16-byte loads in flight per lane
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    f4 xp[2], xg[2], xm[2], xv[2];
#pragma unroll
                    for (int k = 0; k < 2; ++k) {
                        const int i = (2 * h + k) * kThreads + threadIdx.x;
                        xg[k] = g4[i]; xp[k] = p4[i]; xm[k] = m4[i]; xv[k] = v4[i];
                    }
#pragma unroll
                    for (int k = 0; k < 2; ++k) {
                        const int i = (2 * h + k) * kThreads + threadIdx.x;
                        adam_vec4(a, xp[k], xg[k], xm[k], xv[k]);
                        p4[i] = xp[k]; m4[i] = xm[k]; v4[i] = xv[k];
                    }
                }
            } else {
                for (int i = threadIdx.x; i < nvec; i += kThreads) {
                    f4 xp = p4[i], xm = m4[i], xv = v4[i];
                    const f4 xg = g4[i];
                    adam_vec4(a, xp, xg, xm, xv);
                    p4[i] = xp; m4[i] = xm; v4[i] = xv;
                }
            }
            done = nvec << 2;
        }
        for (int i = done + threadIdx.x; i < len; i += kThreads) {
            float xp = p[i], xm = m[i], xv = v[i];
            adam_element(a, xp, g[i], xm, xv);
            p[i] = xp; m[i] = xm; v[i] = xv;
        }
    }
}

// one workgroup, behind the update launch: the step scalars and the counters
__global__ __launch_bounds__(kThreads) void adam_finish_kernel(const OptimTensor* __restrict__ tab, int n, const int32_t* __restrict__ flag,
                                                                 int32_t* __restrict__ counters) {
    const bool skipped = flag && *flag;
    if (!skipped)
        for (int i = threadIdx.x; i < n; i += kThreads) *tab[i].step += 1.f;
    if (threadIdx.x == 0 && counters) counters[skipped ? 1 : 0] += 1;
}

// ---- host: the per-call block and its device copy ----
struct OptimSlot {  // [0] the gradients of e2emv_grads_finite, [1] the tensors of e2emv_adam_step
    char* d = nullptr;
    size_t d_bytes = 0;
    char* h = nullptr;  // pinned: the source of the stream-ordered copy
    size_t h_bytes = 0;
    hipEvent_t copied = nullptr;  // behind the last copy out of `h`
    bool pending = false;
    std::vector<char> last;  // what `d` holds (empty: nothing valid)
};

struct OptimState {
    OptimSlot slot[2];
    int32_t* d_flag = nullptr;
};

OptimState* optim_state(e2emv_ctx* ctx) {
    if (!ctx->optim) ctx->optim = new OptimState();
    return static_cast<OptimState*>(ctx->optim);
}

int ensure_flag(e2emv_ctx* ctx, OptimState* st) {
    if (st->d_flag) return E2EMV_OK;
    E2EMV_HIP(ctx, hipMalloc((void**)&st->d_flag, 256));
    return E2EMV_OK;
}

struct OptimBlock {
    std::vector<char> bytes;
    size_t chunk_off = 0;
    int n_chunks = 0;
};

// Validates the counts and lays the block out; the caller fills the records (rec(i)) before optim_upload.
int optim_block(e2emv_ctx* ctx, const char* who, int n, const int64_t* numel, OptimBlock* B) {
    if (n < 0) return set_err(ctx, E2EMV_ESHAPE, "%s: n = %d", who, n);
    int64_t total = 0;
    for (int i = 0; i < n; ++i) {
        if (numel[i] < 0) return set_err(ctx, E2EMV_ESHAPE, "%s: tensor %d has numel %lld", who, i, (long long)numel[i]);
        total += numel[i] / kChunk + (numel[i] % kChunk != 0);
        if (total > INT_MAX) return set_err(ctx, E2EMV_ESHAPE, "%s: more than %d chunks of %d elements", who, INT_MAX, kChunk);
    }
    B->n_chunks = int(total);
    B->chunk_off = size_t(n) * sizeof(OptimTensor);
    B->bytes.assign(B->chunk_off + size_t(total) * sizeof(OptimChunk), 0);
    OptimChunk* ch = reinterpret_cast<OptimChunk*>(B->bytes.data() + B->chunk_off);
    for (int i = 0; i < n; ++i) {
        const int64_t k = numel[i] / kChunk + (numel[i] % kChunk != 0);
        for (int64_t j = 0; j < k; ++j) *ch++ = OptimChunk{i, int(j)};
    }
    return E2EMV_OK;
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// The device copy of the block: kept when the bytes are those of the last upload, else one stream-ordered copy out of the
// pinned buffer (whose previous copy is waited for first: it ended a table change ago).
int optim_upload(e2emv_ctx* ctx, OptimSlot& S, const OptimBlock& B, hipStream_t s) {
    const size_t n = B.bytes.size();
    if (n == 0 || (S.last.size() == n && std::memcmp(S.last.data(), B.bytes.data(), n) == 0)) return E2EMV_OK;
    S.last.clear();
    if (S.pending) {
        E2EMV_HIP(ctx, hipEventSynchronize(S.copied));
        S.pending = false;
    }
    if (!S.copied) E2EMV_HIP(ctx, hipEventCreateWithFlags(&S.copied, hipEventDisableTiming));
    if (n > S.d_bytes) {
        E2EMV_HIP(ctx, hipStreamSynchronize(s));  // kernels of an earlier call may still read the old block
        if (S.d) E2EMV_HIP(ctx, hipFree(S.d));
        S.d = nullptr;
        S.d_bytes = 0;
        const size_t want = n + n / 4 + 4096;
        if (hipMalloc((void**)&S.d, want) != hipSuccess) {
            (void)hipGetLastError();
            S.d = nullptr;
            return set_err(ctx, E2EMV_ENOMEM, "optimiser table of %zu bytes", want);
        }
        S.d_bytes = want;
    }
    if (n > S.h_bytes) {
        if (S.h) E2EMV_HIP(ctx, hipHostFree(S.h));
        S.h = nullptr;
        S.h_bytes = 0;
        const size_t want = n + n / 4 + 4096;
        if (hipHostMalloc((void**)&S.h, want, hipHostMallocDefault) != hipSuccess) {
            (void)hipGetLastError();
            S.h = nullptr;
            return set_err(ctx, E2EMV_ENOMEM, "pinned staging buffer of %zu bytes", want);
        }
        S.h_bytes = want;
    }
    std::memcpy(S.h, B.bytes.data(), n);
    E2EMV_HIP(ctx, hipMemcpyAsync(S.d, S.h, n, hipMemcpyHostToDevice, s));
    E2EMV_HIP(ctx, hipEventRecord(S.copied, s));
    S.pending = true;
    S.last = B.bytes;
    return E2EMV_OK;
}

inline int grid_for(int n_chunks) { return n_chunks < kMaxGrid ? n_chunks : kMaxGrid; }

}  // namespace

void optim_free(e2emv_ctx* ctx) {
    OptimState* st = static_cast<OptimState*>(ctx->optim);
    if (!st) return;
    for (OptimSlot& S : st->slot) {
        if (S.d) (void)hipFree(S.d);
        if (S.h) (void)hipHostFree(S.h);
        if (S.copied) (void)hipEventDestroy(S.copied);
    }
    if (st->d_flag) (void)hipFree(st->d_flag);
    delete st;
    ctx->optim = nullptr;
}

}  // namespace e2emv

using namespace e2emv;

extern "C" {

int e2emv_grads_finite(e2emv_ctx* ctx, int n, const float* const* d_grad, const int64_t* numel, int32_t* d_flag, void* stream) {
    if (!ctx) return E2EMV_EINVAL;
    if (!d_flag || (n > 0 && (!d_grad || !numel))) return set_err(ctx, E2EMV_EINVAL, "e2emv_grads_finite: NULL argument");
    OptimBlock B;
    int rc = optim_block(ctx, "e2emv_grads_finite", n, numel, &B);
    if (rc) return rc;
    OptimTensor* rec = reinterpret_cast<OptimTensor*>(B.bytes.data());
    for (int i = 0; i < n; ++i) {
        if (!d_grad[i] && numel[i] > 0) return set_err(ctx, E2EMV_EINVAL, "e2emv_grads_finite: NULL gradient %d", i);
        rec[i].g = d_grad[i];
        rec[i].numel = numel[i];
        rec[i].vec = aligned16(d_grad[i]);
    }
    E2EMV_ENTER(ctx, stream);
    hipStream_t s = (hipStream_t)stream;
    OptimSlot& S = optim_state(ctx)->slot[0];
    rc = optim_upload(ctx, S, B, s);
    if (rc) return rc;
    E2EMV_HIP(ctx, hipMemsetAsync(d_flag, 0, sizeof(int32_t), s));
    if (B.n_chunks == 0) return E2EMV_OK;
    prof_begin(ctx, PS_MISC, s);
    hipLaunchKernelGGL(grads_finite_kernel, dim3(grid_for(B.n_chunks)), dim3(kThreads), 0, s, reinterpret_cast<const OptimTensor*>(S.d),
                       reinterpret_cast<const OptimChunk*>(S.d + B.chunk_off), B.n_chunks, d_flag);
    E2EMV_CHECK_LAUNCH(ctx, "grads_finite_kernel");
    return E2EMV_OK;
}

int e2emv_adam_step(e2emv_ctx* ctx, int n, float* const* d_param, const float* const* d_grad, float* const* d_exp_avg,
                    float* const* d_exp_avg_sq, float* const* d_step, const int64_t* numel, const float* lr, double beta1,
                    double beta2, double eps, float clip_value, int skip_nonfinite, int32_t* d_counters, void* stream) {
    if (!ctx) return E2EMV_EINVAL;
    if (n > 0 && (!d_param || !d_grad || !d_exp_avg || !d_exp_avg_sq || !d_step || !numel || !lr))
        return set_err(ctx, E2EMV_EINVAL, "e2emv_adam_step: NULL table");
    OptimBlock B;
    int rc = optim_block(ctx, "e2emv_adam_step", n, numel, &B);
    if (rc) return rc;
    OptimTensor* rec = reinterpret_cast<OptimTensor*>(B.bytes.data());
    for (int i = 0; i < n; ++i) {
        if (!d_step[i] || (numel[i] > 0 && (!d_param[i] || !d_grad[i] || !d_exp_avg[i] || !d_exp_avg_sq[i])))  // (an empty tensor has no storage)
            return set_err(ctx, E2EMV_EINVAL, "e2emv_adam_step: NULL pointer for tensor %d", i);
        rec[i].p = d_param[i];
        rec[i].g = d_grad[i];
        rec[i].m = d_exp_avg[i];
        rec[i].v = d_exp_avg_sq[i];
        rec[i].step = d_step[i];
        rec[i].numel = numel[i];
        rec[i].lr = lr[i];
        rec[i].vec = aligned16(d_param[i]) && aligned16(d_grad[i]) && aligned16(d_exp_avg[i]) && aligned16(d_exp_avg_sq[i]);
    }
    E2EMV_ENTER(ctx, stream);
    hipStream_t s = (hipStream_t)stream;
    OptimState* st = optim_state(ctx);
    OptimSlot& S = st->slot[1];
    rc = optim_upload(ctx, S, B, s);
    if (rc) return rc;
    const OptimTensor* tab = reinterpret_cast<const OptimTensor*>(S.d);
    const OptimChunk* chunks = reinterpret_cast<const OptimChunk*>(S.d + B.chunk_off);
    const int32_t* flag = nullptr;
    prof_begin(ctx, PS_MISC, s);
    if (skip_nonfinite) {
        rc = ensure_flag(ctx, st);
        if (rc) return rc;
        E2EMV_HIP(ctx, hipMemsetAsync(st->d_flag, 0, sizeof(int32_t), s));
        if (B.n_chunks > 0) {
            hipLaunchKernelGGL(grads_finite_kernel, dim3(grid_for(B.n_chunks)), dim3(kThreads), 0, s, tab, chunks, B.n_chunks, st->d_flag);
            E2EMV_CHECK_LAUNCH(ctx, "grads_finite_kernel");
        }
        flag = st->d_flag;
    }
    if (B.n_chunks > 0) {
        hipLaunchKernelGGL(adam_update_kernel, dim3(grid_for(B.n_chunks)), dim3(kThreads), 0, s, tab, chunks, B.n_chunks, flag, beta1, beta2,
                           float(eps), clip_value);
        E2EMV_CHECK_LAUNCH(ctx, "adam_update_kernel");
    }
    if (n > 0 || d_counters) {
        hipLaunchKernelGGL(adam_finish_kernel, dim3(1), dim3(kThreads), 0, s, tab, n, flag, d_counters);
        E2EMV_CHECK_LAUNCH(ctx, "adam_finish_kernel");
    }
    return E2EMV_OK;
}

}  // extern "C"
