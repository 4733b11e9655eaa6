// Weight ingestion of libe2emv.so: e2emv_set_weight / e2emv_commit_weights (BN folding, head-major re-ordering, merge conv
// folded into MLP0), the host-side splits of a weight matrix into the 16-bit formats of the split-operand kernels, and the
// packing of every dense layer into the two device arenas - one DenseWeights record per layer (weights.h).  No kernels.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "common.h"
#include "p2.h"

namespace e2emv {

const HostTensor* find(e2emv_ctx* ctx, const std::string& k) {
    auto it = ctx->raw.find(k);
    return it == ctx->raw.end() ? nullptr : &it->second;
}

namespace {

inline uint16_t f2h(float f) {
    const _Float16 h = (_Float16)f;  // round to nearest even
    uint16_t u;
    memcpy(&u, &h, 2);
    return u;
}
inline float h2f(uint16_t u) {
    _Float16 h;
    memcpy(&h, &u, 2);
    return (float)h;
}
// fp32 -> bf16 (round to nearest even) and back, host side - same arithmetic as the device split
inline uint16_t f2bf(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);  // NaN
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}
inline float bf2f(uint16_t h) {
    uint32_t u = (uint32_t)h << 16;
    float f;
    memcpy(&f, &u, 4);
    return f;
}

constexpr size_t npos = (size_t)-1;

// a new 256-byte aligned segment of n halves at the end of `out`; returns its offset
size_t grow(std::vector<uint16_t>& out, size_t n) {
    const size_t off = (out.size() + 127) & ~size_t(127);
    out.resize(off + n);
    return off;
}

// weights [rows][cols] fp32 -> S3 [rows][3][cols] bf16 planes appended to `out`; returns the offset
size_t add_split3(std::vector<uint16_t>& out, const std::vector<float>& w, int rows, int cols) {
    const size_t off = grow(out, (size_t)rows * 3 * cols);
    for (int r = 0; r < rows; ++r)
        for (int c = 0; c < cols; ++c) {
            const float v = w[(size_t)r * cols + c];
            const uint16_t a = f2bf(v);
            const float r1 = v - bf2f(a);
            const uint16_t b = f2bf(r1);
            const float r2 = r1 - bf2f(b);
            const uint16_t d = f2bf(r2);
            uint16_t* o = &out[off + (size_t)r * 3 * cols];
            o[c] = a; o[cols + c] = b; o[2 * cols + c] = d;
        }
    return off;
}

// The fp16 formats hold 2^s W, s = the power of two that brings max |w| into [2^13, 2^14): lo (and the 2^-11 hi the kernels
// derive) then stay normal fp16 numbers for every |w| >= 2^-16 max |w|.  The kernels' output scale is 2^-s.
int f16_shift(const std::vector<float>& w) {
    float mx = 0.f;
    for (float v : w) mx = std::max(mx, std::fabs(v));
    int e = 0;
    if (mx > 0.f && std::isfinite(mx)) (void)std::frexp(mx, &e);  // mx = m 2^e, m in [0.5, 1)
    return 14 - e;
}

// weights [rows][cols] fp32 -> fp16 {hi, lo} of 2^sh W appended to `out`, lo the UNSCALED residual fp16(v - hi); element (r, c)
// goes to index(r, c) (hi) and index(r, c) + lo_step (lo)
template <typename Index>
size_t add_split_f16(std::vector<uint16_t>& out, const std::vector<float>& w, int rows, int cols, int sh, size_t lo_step, Index index) {
    const float sc = std::ldexp(1.f, sh);
    const size_t off = grow(out, (size_t)rows * 2 * cols);
    for (int r = 0; r < rows; ++r)
        for (int c = 0; c < cols; ++c) {
            const float v = w[(size_t)r * cols + c] * sc;
            const uint16_t hi = f2h(v);
            uint16_t* o = &out[off + index(r, c)];
            o[0] = hi; o[lo_step] = f2h(v - h2f(hi));
        }
    return off;
}
// ... as planes [rows][{hi, lo}][cols] (the "f16x2" weight format of gemm_h2.hip)
size_t add_split_h2(std::vector<uint16_t>& out, const std::vector<float>& w, int rows, int cols, int sh) {
    return add_split_f16(out, w, rows, cols, sh, cols, [=](int r, int c) { return (size_t)r * 2 * cols + c; });
}
// ... as P2 planes [rows][cols / 32 blocks of {32 hi, 32 lo}] (p2.h; gemm_p2.hip)
size_t add_split_p2(std::vector<uint16_t>& out, const std::vector<float>& w, int rows, int cols, int sh) {
    return add_split_f16(out, w, rows, cols, sh, 32, [=](int r, int c) { return (size_t)p2_index(r, c, cols); });
}

// Appends the 16-bit formats `formats` (WF_*) of dw's weights w to `u16` - S3, then fp16 x 2, then P2 - and fills dw.hs and
// dw.ba (b: the bias); returns the offsets {w3, wh, wp}, npos where the format was not asked for
struct PlaneOffsets {
    size_t w3 = npos, wh = npos, wp = npos;
};
PlaneOffsets add_planes(std::vector<uint16_t>& u16, const std::vector<float>& w, const std::vector<float>& b, int formats, DenseWeights& dw) {
    PlaneOffsets o;
    const int sh = f16_shift(w);
    if (formats & WF_S3) o.w3 = add_split3(u16, w, dw.out, dw.in);
    if (formats & WF_H2) o.wh = add_split_h2(u16, w, dw.out, dw.in, sh);
    if (formats & WF_P2) o.wp = add_split_p2(u16, w, dw.out, dw.in, sh);
    dw.hs = (formats & (WF_H2 | WF_P2)) ? std::ldexp(1.f, -sh) : 0.f;
    dw.ba = 0.f;
    for (float v : b) dw.ba = std::max(dw.ba, std::fabs(v));
    return o;
}
void point_planes(DenseWeights& dw, const PlaneOffsets& o, const uint16_t* base) {
    dw.w3 = o.w3 == npos ? nullptr : base + o.w3;
    dw.wh = o.wh == npos ? nullptr : base + o.wh;
    dw.wp = o.wp == npos ? nullptr : base + o.wp;
}

// The two host arenas of a commit.  add_dense appends a layer to both and remembers where; resolve turns the offsets into
// device pointers once the arenas are uploaded.
struct Packer {
    std::vector<float> f32;     // fp32 weights and biases, 256-B aligned segments
    std::vector<uint16_t> u16;  // split (bf16 x 3 / fp16 x 2 / P2) planes of the GEMM weights
    struct Slot {
        DenseWeights* dst;
        size_t w, b;
        PlaneOffsets planes;
    };
    std::vector<Slot> slots;
    size_t add(const std::vector<float>& v) {
        size_t off = (f32.size() + 63) & ~size_t(63);
        f32.resize(off);
        f32.insert(f32.end(), v.begin(), v.end());
        return off;
    }
    // `dst` must stay where it is until resolve
    void add_dense(DenseWeights& dst, const std::vector<float>& w, const std::vector<float>& b, int out, int in, int formats) {
        dst = DenseWeights();
        dst.out = out; dst.in = in;
        const size_t ow = add(w), ob = add(b);
        slots.push_back({&dst, ow, ob, add_planes(u16, w, b, formats, dst)});
    }
    void resolve(const float* base32, const uint16_t* base16) {
        for (const Slot& s : slots) {
            s.dst->w = base32 + s.w;
            s.dst->b = base32 + s.b;
            point_planes(*s.dst, s.planes, base16);
        }
    }
};

// conv weight [out][in](,1) -> checked copy
int get_conv(e2emv_ctx* ctx, const std::string& prefix, int out, int in, std::vector<float>& w,
             std::vector<float>& b) {
    const HostTensor* tw = find(ctx, prefix + ".weight");
    const HostTensor* tb = find(ctx, prefix + ".bias");
    if (!tw || !tb) return set_err(ctx, E2EMV_ESTATE, "missing weight '%s.{weight,bias}'", prefix.c_str());
    if ((int64_t)tw->data.size() != (int64_t)out * in || (int64_t)tb->data.size() != out)
        return set_err(ctx, E2EMV_ESHAPE, "'%s': expected [%d,%d], got %zu elements", prefix.c_str(), out, in,
                       tw->data.size());
    w = tw->data;
    b = tb->data;
    return E2EMV_OK;
}

// fold eval-mode BatchNorm1d `bn` (if present) into conv (w [out][in], b [out])
int fold_bn(e2emv_ctx* ctx, const std::string& bn, int out, int in, std::vector<float>& w, std::vector<float>& b) {
    const HostTensor* mean = find(ctx, bn + ".running_mean");
    if (!mean) return E2EMV_OK;  // fork without BN: nothing to fold
    const HostTensor* var = find(ctx, bn + ".running_var");
    const HostTensor* g = find(ctx, bn + ".weight");
    const HostTensor* be = find(ctx, bn + ".bias");
    if (!var || !g || !be || (int)mean->data.size() != out || (int)var->data.size() != out ||
        (int)g->data.size() != out || (int)be->data.size() != out)
        return set_err(ctx, E2EMV_ESHAPE, "BatchNorm '%s' incomplete or wrong size", bn.c_str());
    for (int o = 0; o < out; ++o) {
        // same association as the unfolded op order: (x - mean) / sqrt(var + eps) * g + beta
        double s = (double)g->data[o] / std::sqrt((double)var->data[o] + 1e-5);
        for (int i = 0; i < in; ++i) w[(size_t)o * in + i] = (float)((double)w[(size_t)o * in + i] * s);
        b[o] = (float)(((double)b[o] - (double)mean->data[o]) * s + (double)be->data[o]);
    }
    return E2EMV_OK;
}

// makes the device arena *arena (*have elements) at least n elements large; synchronises when it has to grow
template <typename T>
int grow_arena(e2emv_ctx* ctx, T** arena, size_t* have, size_t n, const char* what) {
    if (n <= *have) return E2EMV_OK;
    E2EMV_HIP(ctx, hipDeviceSynchronize());
    if (*arena) E2EMV_HIP(ctx, hipFree(*arena));
    *arena = nullptr;
    *have = 0;
    void* p = nullptr;
    if (hipMalloc(&p, std::max<size_t>(n, 1) * sizeof(T)) != hipSuccess) {
        (void)hipGetLastError();
        return set_err(ctx, E2EMV_ENOMEM, "%s allocation failed", what);
    }
    *arena = (T*)p;
    *have = n;
    return E2EMV_OK;
}

}  // namespace

int dense_from_device(e2emv_ctx* ctx, const float* d_W, const float* d_bias, int out, int in, int format, uint16_t* d_planes,
                      DenseWeights& dw, hipStream_t s) {
    std::vector<float> hw((size_t)out * in), hb(d_bias ? out : 0);
    E2EMV_HIP(ctx, hipStreamSynchronize(s));
    E2EMV_HIP(ctx, hipMemcpy(hw.data(), d_W, hw.size() * sizeof(float), hipMemcpyDeviceToHost));
    if (d_bias) E2EMV_HIP(ctx, hipMemcpy(hb.data(), d_bias, hb.size() * sizeof(float), hipMemcpyDeviceToHost));
    dw = DenseWeights();
    dw.out = out; dw.in = in; dw.w = d_W; dw.b = d_bias;
    std::vector<uint16_t> planes;
    const PlaneOffsets o = add_planes(planes, hw, hb, format, dw);  // (one format: at offset 0)
    E2EMV_HIP(ctx, hipMemcpy(d_planes, planes.data(), planes.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
    point_planes(dw, o, d_planes);
    return E2EMV_OK;
}

}  // namespace e2emv

using namespace e2emv;

extern "C" int e2emv_set_weight(e2emv_ctx* ctx, const char* key, const float* data, const int64_t* shape, int ndim) {
    if (!ctx || !key || !data || ndim < 0 || ndim > 4 || (ndim && !shape)) return E2EMV_EINVAL;
    E2EMV_LOCK(ctx);
    std::string k(key);
    if (k.rfind("module.", 0) == 0) k = k.substr(7);
    HostTensor t;
    int64_t n = 1;
    for (int i = 0; i < ndim; ++i) {
        if (shape[i] < 0) return set_err(ctx, E2EMV_ESHAPE, "negative dim in '%s'", key);
        t.shape.push_back(shape[i]);
        n *= shape[i];
    }
    t.data.assign(data, data + n);
    const bool sp = k.rfind("superpoint.", 0) == 0;  // front-end weights (superpoint.hip) live beside the matcher's
    ctx->raw[k] = std::move(t);
    if (sp) ctx->sp_committed = false; else ctx->committed = false;
    return E2EMV_OK;
}

extern "C" int e2emv_commit_weights(e2emv_ctx* ctx, const e2emv_model_desc* m) {
    if (!ctx || !m) return E2EMV_EINVAL;
    E2EMV_LOCK(ctx);
    const int D = m->desc_dim, H = m->num_heads;
    if (D <= 0 || H <= 0 || D % H != 0 || D / H != 64 || D % 64 != 0)
        return set_err(ctx, E2EMV_ESHAPE, "descriptor_dim %d / num_heads %d: head dim must be 64", D, H);
    if (m->n_kenc < 1 || m->n_kenc > E2EMV_MAX_KENC || m->n_layers < 0 || m->n_layers > E2EMV_MAX_LAYERS)
        return set_err(ctx, E2EMV_ESHAPE, "bad layer counts");
    (void)hipSetDevice(ctx->device);
    const int d = D / H;
    Packer pk;
    int rc;
    std::vector<float> w, b;
    // ---- keypoint encoder: no bf16x3 planes; the wide layers (fan-in >= 128) also as fp16 x 2 planes ----
    std::vector<int> dims = {3};
    for (int i = 0; i < m->n_kenc; ++i) dims.push_back(m->kenc[i]);
    dims.push_back(D);
    for (size_t i = 1; i + 1 < dims.size(); ++i)
        if (dims[i] % 32 != 0) return set_err(ctx, E2EMV_ESHAPE, "keypoint_encoder width %d not a multiple of 32", dims[i]);
    const int nk = (int)dims.size() - 1;
    std::vector<DenseWeights> kenc(nk);
    for (int i = 0; i < nk; ++i) {
        std::string p = "kenc.encoder." + std::to_string(3 * i);
        if ((rc = get_conv(ctx, p, dims[i + 1], dims[i], w, b))) return rc;
        if (i < nk - 1 && (rc = fold_bn(ctx, "kenc.encoder." + std::to_string(3 * i + 1), dims[i + 1], dims[i], w, b)))
            return rc;
        pk.add_dense(kenc[i], w, b, dims[i + 1], dims[i], dims[i] >= 128 ? WF_H2 : 0);
    }
    // ---- GNN layers: all three 16-bit formats ----
    std::vector<LayerWeights> layers(m->n_layers);
    for (int l = 0; l < m->n_layers; ++l) {
        LayerWeights& L = layers[l];
        L.type = m->layer_types[l] ? 1 : 0;
        std::string base = "gnn.layers." + std::to_string(l);
        std::vector<float> wqkv((size_t)3 * D * D), bqkv((size_t)3 * D);
        for (int p = 0; p < 3; ++p) {
            if ((rc = get_conv(ctx, base + ".attn.proj." + std::to_string(p), D, D, w, b))) return rc;
            for (int h = 0; h < H; ++h)
                for (int dd = 0; dd < d; ++dd) {
                    int src = dd * H + h, dst = p * D + h * d + dd;  // upstream channel -> head-major
                    memcpy(&wqkv[(size_t)dst * D], &w[(size_t)src * D], sizeof(float) * D);
                    bqkv[dst] = b[src];
                }
        }
        pk.add_dense(L.qkv, wqkv, bqkv, 3 * D, D, WF_S3 | WF_H2 | WF_P2);
        if ((rc = get_conv(ctx, base + ".attn.merge", D, D, w, b))) return rc;
        std::vector<float> wm((size_t)D * D);
        for (int o = 0; o < D; ++o)
            for (int h = 0; h < H; ++h)
                for (int dd = 0; dd < d; ++dd) wm[(size_t)o * D + h * d + dd] = w[(size_t)o * D + dd * H + h];
        const std::vector<float> bmerge = b;
        if ((rc = get_conv(ctx, base + ".mlp.0", 2 * D, 2 * D, w, b))) return rc;
        if ((rc = fold_bn(ctx, base + ".mlp.1", 2 * D, 2 * D, w, b))) return rc;
        {
            // MLP0([x | merge(o)]) = W0x x + (W0m Wmerge) o + (b0 + W0m bmerge): the merge conv is
            // linear and feeds nothing else, so it is folded into MLP0's second K segment (fp64 on
            // the host).  Saves one GEMM (2 N D^2 flops) and one activation round trip per layer.
            std::vector<double> acc((size_t)2 * D * D, 0.0);
            for (int o = 0; o < 2 * D; ++o) {
                const float* w0m = &w[(size_t)o * 2 * D + D];
                double* ao = &acc[(size_t)o * D];
                double bb = b[o];
                for (int k = 0; k < D; ++k) {
                    const double wk = w0m[k];
                    const float* wr = &wm[(size_t)k * D];
                    for (int c = 0; c < D; ++c) ao[c] += wk * (double)wr[c];
                    bb += wk * (double)bmerge[k];
                }
                b[o] = (float)bb;
            }
            for (int o = 0; o < 2 * D; ++o)
                for (int c = 0; c < D; ++c) w[(size_t)o * 2 * D + D + c] = (float)acc[(size_t)o * D + c];
        }
        pk.add_dense(L.mlp0, w, b, 2 * D, 2 * D, WF_S3 | WF_H2 | WF_P2);
        if ((rc = get_conv(ctx, base + ".mlp.3", D, 2 * D, w, b))) return rc;
        pk.add_dense(L.mlp1, w, b, D, 2 * D, WF_S3 | WF_H2 | WF_P2);
    }
    // ---- final_proj and the conf head: fp16 x 2 and P2 (no bf16x3 planes) ----
    DenseWeights final_proj, conf0;
    if ((rc = get_conv(ctx, "final_proj", D, D, w, b))) return rc;
    pk.add_dense(final_proj, w, b, D, D, WF_H2 | WF_P2);
    const HostTensor* bs = find(ctx, "bin_score");
    if (!bs || bs->data.size() != 1) return set_err(ctx, E2EMV_ESTATE, "missing scalar 'bin_score'");
    size_t wc1 = 0;
    float bc1 = 0.f;
    if (m->conf_mlp) {
        if ((rc = get_conv(ctx, "conf_mlp.0", D, 2 * D, w, b))) return rc;
        if ((rc = fold_bn(ctx, "conf_mlp.1", D, 2 * D, w, b))) return rc;
        pk.add_dense(conf0, w, b, D, 2 * D, WF_H2 | WF_P2);
        if ((rc = get_conv(ctx, "conf_mlp.3", 1, D, w, b))) return rc;
        wc1 = pk.add(w);
        bc1 = b[0];
    }
    // ---- upload ----
    if ((rc = grow_arena(ctx, &ctx->d_warena, &ctx->warena_floats, pk.f32.size(), "weight arena"))) return rc;
    if ((rc = grow_arena(ctx, &ctx->d_w3arena, &ctx->w3arena_elems, pk.u16.size(), "bf16x3 weight arena"))) return rc;
    E2EMV_HIP(ctx, hipDeviceSynchronize());  // no forward may be in flight while weights change
    E2EMV_HIP(ctx, hipMemcpy(ctx->d_warena, pk.f32.data(), pk.f32.size() * sizeof(float), hipMemcpyHostToDevice));
    if (!pk.u16.empty())
        E2EMV_HIP(ctx, hipMemcpy(ctx->d_w3arena, pk.u16.data(), pk.u16.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
    pk.resolve(ctx->d_warena, ctx->d_w3arena);
    ctx->kenc_dims = dims;
    ctx->kenc_w0 = kenc[0].w;
    ctx->kenc_b0 = kenc[0].b;
    ctx->kenc.assign(kenc.begin() + 1, kenc.end());
    ctx->layers = layers;
    ctx->final_proj = final_proj;
    ctx->conf0 = conf0;  // (all null without conf_mlp)
    ctx->w_conf1 = m->conf_mlp ? ctx->d_warena + wc1 : nullptr;
    ctx->b_conf1 = bc1;
    ctx->bin_score = bs->data[0];
    ctx->model = *m;
    ctx->committed = true;
    E2EMV_NULL_STREAM_FENCE(ctx);  // (the arenas and the weight planes uploaded above)
    return E2EMV_OK;
}
