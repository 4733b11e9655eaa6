// Training path (VERDICT r2 row g): the matcher forward with a tape and the backward of the match loss and of the
// pose loss, so that the reference's `run_matcher` -> `train_loss.backward()` (helpers.py:243-260, train.py:406-425) runs
// through this library in both training stages.  Reference arithmetic: fp32 everywhere (the f32 kernels of the inference path
// for the forward, train_kernels.h for the rest).
//
// What is differentiated: keypoint encoder, the L x {q|k|v projection, attention, merge, MLP}, final_proj, the score
// matrix, the dustbin score, the unrolled log-domain Sinkhorn (the reverse sweep walks the stored u_t, v_t of every
// iteration - the same gradient torch.autograd computes through upstream's log_optimal_transport, not an implicit
// differentiation) and the conf_mlp head (e2emv_conf_forward_train; the pose loss reaches it through pose.hip's
// e2emv_w8pt_backward).  BatchNorm layers normalise with their RUNNING statistics (E2EMV_BN_FROZEN, frozen-statistics
// fine-tuning: the reference builds its DDP wrapper with broadcast_buffers=False "until BatchNorm stats are updated",
// train.py:351-356; their affine parameters get gradients through the folded convolution) or with the statistics of the
// batch (E2EMV_BN_BATCH, torch's training-mode BatchNorm1d: the BN layers stay unfolded, bn_* kernels of train_kernels.h).
// Still forward-only: ragged keypoint counts, the confidences of a model without conf_mlp (the match score).
//
// The backward is a sequence of general fp32 MFMA GEMMs (dgrad: dY W, wgrad: dY^T X with the row contraction split over
// workgroups) and row-wise kernels; the attention backward re-computes the probabilities from the saved q|k|v.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "ingest.h"
#include "train_kernels.h"

namespace e2emv {

struct TrainLayer {
    size_t wqkv, bqkv, wm, bm, w0, b0, w1, b1;  // offsets (floats) into the folded arena: q|k|v [3D][D] head-major rows,
    int type;                                    // merge [D][D] head-major columns, MLP0 [2D][2D] BN folded, MLP1 [D][2D]
};

struct RawRef {
    size_t off, numel;
};

struct TrainState {
    e2emv_model_desc model{};
    // folded weights and their gradients (same offsets)
    float* d_w = nullptr;
    float* d_gw = nullptr;
    size_t w_floats = 0;
    std::vector<size_t> kw, kb;  // keypoint encoder layers 0..n (BN folded)
    std::vector<int> kdims;      // [3, c0, ..., D]
    std::vector<TrainLayer> layers;
    size_t wf = 0, bf = 0, alpha = 0;
    size_t wc0 = 0, bc0 = 0, wc1 = 0, bc1 = 0;  // conf_mlp.0 (+ BN conf_mlp.1) [D][2D], conf_mlp.3 [1][D]
    bool conf_mlp = false;
    float bin_score = 1.f;
    // upstream parameters (for the unfolding) and their gradients (same offsets)
    float* d_raw = nullptr;
    float* d_graw = nullptr;
    size_t raw_floats = 0;
    std::map<std::string, RawRef> raw;
    int* d_maps = nullptr;  // [0, D): upstream channel -> head-major channel
    // tape of the last forward
    char* d_tape = nullptr;
    size_t tape_bytes = 0;
    bool have_tape = false;
    int B = 0, T = 0, N = 0, n_rows = 0, iters = 0, P = 0, ldS = 0;
    int64_t Mtot = 0;
    float* t_inp = nullptr;               // [Mtot][4] normalised keypoints + score
    std::vector<float*> t_kh;             // hidden activations of the keypoint encoder (post ReLU)
    std::vector<float*> t_x;              // x_0 ... x_L
    std::vector<float*> t_qkv, t_att, t_msg, t_h;
    float* t_mdesc = nullptr;
    float* t_S = nullptr;                 // [P*B][N][ldS]
    float* t_uv = nullptr;                // [P*B][iters + 1][2][N + 1]: u_t, v_t (t = 0: zeros)
    std::vector<float*> t_cfeat, t_chid;  // conf head, per pair: [B][N][2D] input, [B][N][D] hidden (post ReLU)
    std::vector<const int64_t*> t_cmatch; // matches the conf head of a pair was run with (caller's buffer, must stay alive until backward)
    // batch-statistics BatchNorm (bn_mode E2EMV_BN_BATCH): the BatchNorm layers are NOT folded into their convolutions; the tape
    // keeps each one's conv output y and the statistics of every call
    int bn_mode = E2EMV_BN_FROZEN;
    struct Bn {
        std::string name;     // module prefix (kenc.encoder.{1,4,..}, gnn.layers.{l}.mlp.1, conf_mlp.1)
        int C;
        size_t gamma, beta;   // offsets in the raw arena (and in the raw gradient arena)
    };
    std::vector<Bn> bns;                  // encoder BNs 1 .. nk-1 (bns[j - 1]), then the L GNN MLPs, then conf_mlp.1
    std::vector<float*> t_ky, t_kst;      // encoder BN j (j = 1 .. nk-1): y [Mtot][kdims[j]], statistics [T][3][kdims[j]]
    std::vector<float*> t_hy, t_hst;      // GNN layer l: y [Mtot][2D], statistics [T][3][2D]
    std::vector<float*> t_cy;             // conf head of pair q: y [B*N][D]
    float* t_cst = nullptr;               // [P][3][D]
    double* t_part = nullptr;             // forward partial sums (bn_chunks_max x calls x 2 x C doubles)
};

static TrainState* ts_of(e2emv_ctx* ctx) { return static_cast<TrainState*>(ctx->train); }

void train_free(e2emv_ctx* ctx) {
    TrainState* t = ts_of(ctx);
    if (!t) return;
    for (void* p : {(void*)t->d_w, (void*)t->d_gw, (void*)t->d_raw, (void*)t->d_graw, (void*)t->d_maps, (void*)t->d_tape})
        if (p) (void)hipFree(p);
    delete t;
    ctx->train = nullptr;
}

static int launch_gg(e2emv_ctx* ctx, const GG& g, hipStream_t s) {
    if (g.M <= 0 || g.N <= 0 || g.K <= 0 || g.batch <= 0) return E2EMV_OK;
    dim3 grid((g.N + GG_T - 1) / GG_T, (g.M + GG_T - 1) / GG_T, g.batch * g.splits);
    hipLaunchKernelGGL(gg_kernel, grid, dim3(256), 0, s, g);
    E2EMV_CHECK_LAUNCH(ctx, "gg_kernel");
    return E2EMV_OK;
}

// wgrad: dW [n_out][n_in] (row stride ldw) += dY^T X over `rows` rows (dY [rows][ldy], X [rows][ldx])
static int wgrad(e2emv_ctx* ctx, const float* dY, int64_t ldy, int n_out, const float* X, int64_t ldx, int n_in, int64_t rows, float* dW, int64_t ldw,
                 hipStream_t s) {
    GG g;
    g.M = n_out; g.N = n_in; g.K = (int)rows;
    g.A = dY; g.am = 1; g.ak = ldy;
    g.B = X; g.bk = ldx; g.bn = 1;
    g.C = dW; g.ldc = ldw;
    g.mode = 2;
    g.splits = (int)std::max<int64_t>(1, std::min<int64_t>(256, rows / 512));
    return launch_gg(ctx, g, s);
}
// dgrad: dX [rows][n_in] (row stride ldx) (+)= dY [rows][n_out] W [n_out][n_in]
static int dgrad(e2emv_ctx* ctx, const float* dY, int64_t ldy, int n_out, const float* W, int64_t ldw, int n_in, int64_t rows, float* dX, int64_t ldx,
                 bool accumulate, hipStream_t s) {
    GG g;
    g.M = (int)rows; g.N = n_in; g.K = n_out;
    g.A = dY; g.am = ldy; g.ak = 1;
    g.B = W; g.bk = ldw; g.bn = 1;
    g.C = dX; g.ldc = ldx;
    g.mode = accumulate ? 1 : 0;
    return launch_gg(ctx, g, s);
}
static int colsum(e2emv_ctx* ctx, const float* X, int64_t rows, int N, int64_t ld, float* out, hipStream_t s) {
    const int64_t per = 64;  // (rows per workgroup: short loops, many workgroups - a bias gradient of 8192 x 768 fills the chip)
    hipLaunchKernelGGL(colsum_kernel, dim3((N + 255) / 256, (unsigned)((rows + per - 1) / per)), dim3(256), 0, s, X, rows, N, ld, out, per);
    E2EMV_CHECK_LAUNCH(ctx, "colsum_kernel");
    return E2EMV_OK;
}
static unsigned ew_grid(int64_t n) { return (unsigned)std::min<int64_t>((n + 255) / 256, 4096); }

// ---- batch-statistics BatchNorm launches (train_kernels.h, BnCall) ----
constexpr int BN_MAX_CHUNKS = 64;  // (64 rows per chunk: 16 per thread, 4 steps of 4 loads in flight)
static int bn_chunks(int64_t rows) { return (int)std::max<int64_t>(1, std::min<int64_t>(BN_MAX_CHUNKS, (rows + 63) / 64)); }
// BN `j` of the tape over the T images ([b][t][n_rows][C] arena): one call per image
static BnCall bn_images(const TrainState* t, int j, float* y, float* out, float* stats, double* part) {
    BnCall a;
    const TrainState::Bn& bn = t->bns[j];
    a.y = y; a.out = out; a.stats = stats; a.part = part;
    a.gamma = t->d_raw + bn.gamma; a.beta = t->d_raw + bn.beta;
    a.dgamma = t->d_graw + bn.gamma; a.dbeta = t->d_graw + bn.beta;
    a.C = bn.C; a.N = t->N; a.nseg = t->B; a.seg_rows = t->n_rows;
    a.seg_stride = (int64_t)t->T * t->n_rows; a.z_stride = t->n_rows;
    a.chunks = bn_chunks((int64_t)t->B * t->N);
    return a;
}
// conf_mlp.1 on one pair's dense [B*N][D] features: one call
static BnCall bn_conf(const TrainState* t, float* y, float* out, float* stats, double* part) {
    BnCall a = bn_images(t, (int)t->bns.size() - 1, y, out, stats, part);
    a.N = a.seg_rows = t->B * t->N; a.nseg = 1; a.seg_stride = 0; a.z_stride = 0;
    return a;
}
static int bn_forward(e2emv_ctx* ctx, const BnCall& a, int calls, hipStream_t s) {
    const dim3 grid((a.C + 63) / 64, a.chunks, calls);
    hipLaunchKernelGGL(bn_stats_kernel, grid, dim3(256), 0, s, a, 0);
    hipLaunchKernelGGL(bn_stats_kernel, grid, dim3(256), 0, s, a, 1);
    hipLaunchKernelGGL(bn_apply_kernel, grid, dim3(256), 0, s, a);
    E2EMV_CHECK_LAUNCH(ctx, "batchnorm forward kernels");
    return E2EMV_OK;
}
static int bn_backward(e2emv_ctx* ctx, const BnCall& a, int calls, hipStream_t s) {
    const dim3 grid((a.C + 63) / 64, a.chunks, calls);
    hipLaunchKernelGGL(bn_bwd_stats_kernel, grid, dim3(256), 0, s, a);
    hipLaunchKernelGGL(bn_bwd_apply_kernel, grid, dim3(256), 0, s, a);
    E2EMV_CHECK_LAUNCH(ctx, "batchnorm backward kernels");
    return E2EMV_OK;
}

// ---- the unrolled Sinkhorn of one pair (M = N): B problems, S / alpha in `sk`; uv [b][t][{u, v}][N + 1], t = 0 .. iters ----
// columns per workgroup of the column kernels: col_width 32 / 64 forces the instance, 0 = by the size of the grid
static bool sk_col32(const e2emv_ctx* ctx, int B, int N, int col_width) {
    if (col_width) return col_width == 32;
    return (int64_t)B * ((N + 1 + 63) / 64) < ctx->num_cus;  // (64-column workgroups would not fill the chip)
}
// forward with a tape: u_t, v_t of every iteration into uv (uv[b][0] = zeros on entry), the log assignment into logZ [B][N+1][N+1]
static int sinkhorn_tape_forward(e2emv_ctx* ctx, const SkT& sk, int B, int iters, float* uv, float* logZ, int col_width, hipStream_t s) {
    const int N = sk.N;
    const int64_t uvs = (int64_t)(iters + 1) * 2 * (N + 1);  // per problem
    const bool col32 = sk_col32(ctx, B, N, col_width);
    for (int it = 1; it <= iters; ++it) {
        float* u_t = uv + (int64_t)it * 2 * (N + 1);
        float* v_t = u_t + (N + 1);
        const float* v_p = uv + (int64_t)(it - 1) * 2 * (N + 1) + (N + 1);
        hipLaunchKernelGGL(skt_row_kernel, dim3((N + 1 + 3) / 4, B), dim3(256), 0, s, sk, v_p, u_t, uvs, uvs);
        if (col32) hipLaunchKernelGGL((skt_col_kernel<32>), dim3((N + 1 + 31) / 32, B), dim3(1024), 0, s, sk, (const float*)u_t, v_t, uvs, uvs);
        else hipLaunchKernelGGL((skt_col_kernel<64>), dim3((N + 1 + 63) / 64, B), dim3(1024), 0, s, sk, (const float*)u_t, v_t, uvs, uvs);
    }
    const float* u_T = uv + (int64_t)iters * 2 * (N + 1);
    hipLaunchKernelGGL(skt_out_kernel, dim3(ew_grid((int64_t)(N + 1) * (N + 1)), B), dim3(256), 0, s, sk, u_T, u_T + (N + 1), uvs, uvs, logZ);
    E2EMV_CHECK_LAUNCH(ctx, "sinkhorn training kernels");
    return E2EMV_OK;
}
// reverse sweep over the tape: G = dLoss / dlogZ [B][N+1][N+1] -> dC [B][N+1][N+1] (written), *dalpha += its dustbin row and
// column; du, dv, dv2: scratch [B][N + 1] each (du is left zeroed when iters > 0)
static int sinkhorn_tape_backward(e2emv_ctx* ctx, const SkT& sk, int B, int iters, const float* uv, const float* G, float* dC, float* du, float* dv,
                                  float* dv2, float* dalpha, int col_width, hipStream_t s) {
    const int N = sk.N;
    const int64_t uvs = (int64_t)(iters + 1) * 2 * (N + 1);
    E2EMV_HIP(ctx, hipMemsetAsync(dv, 0, (size_t)B * (N + 1) * sizeof(float), s));
    hipLaunchKernelGGL(skb_init_kernel, dim3((N + 1 + 3) / 4, B), dim3(256), 0, s, N, N, G, dC, du, dv, (int64_t)(N + 1), (int64_t)(N + 1));
    float* dv_cur = dv;
    float* dv_nxt = dv2;
    const bool col32 = sk_col32(ctx, B, N, col_width);
    for (int it = iters; it >= 1; --it) {
        const float* u_t = uv + (int64_t)it * 2 * (N + 1);
        const float* v_t = u_t + (N + 1);
        const float* v_p = uv + (int64_t)(it - 1) * 2 * (N + 1) + (N + 1);
        hipLaunchKernelGGL(skb_vhalf_kernel, dim3((N + 1 + 3) / 4, B), dim3(256), 0, s, sk, u_t, v_t, (const float*)dv_cur, du, dC, uvs, uvs, (int64_t)(N + 1));
        if (col32) hipLaunchKernelGGL((skb_uhalf_kernel<32>), dim3((N + 1 + 31) / 32, B), dim3(1024), 0, s, sk, u_t, v_p, (const float*)du, dv_nxt, dC, uvs, uvs, (int64_t)(N + 1));
        else hipLaunchKernelGGL((skb_uhalf_kernel<64>), dim3((N + 1 + 63) / 64, B), dim3(1024), 0, s, sk, u_t, v_p, (const float*)du, dv_nxt, dC, uvs, uvs, (int64_t)(N + 1));
        E2EMV_HIP(ctx, hipMemsetAsync(du, 0, (size_t)B * (N + 1) * sizeof(float), s));
        std::swap(dv_cur, dv_nxt);
    }
    E2EMV_CHECK_LAUNCH(ctx, "sinkhorn backward kernels");
    hipLaunchKernelGGL(skb_alpha_kernel, dim3(B), dim3(256), 0, s, N, N, (const float*)dC, dalpha);
    return E2EMV_OK;
}
static SkT sk_problem(const float* S, int64_t ldS, int N, float alpha) {
    SkT sk{};
    sk.S = S; sk.ldS = ldS; sk.M = N; sk.N = N; sk.alpha = alpha;
    sk.norm = -logf((float)(2 * N)); sk.logM = logf((float)N); sk.logN = logf((float)N);
    return sk;
}

}  // namespace e2emv

using namespace e2emv;

namespace {

struct Pack {
    std::vector<float> host;
    size_t add(const std::vector<float>& v) {
        size_t off = (host.size() + 63) & ~size_t(63);
        host.resize(off);
        host.insert(host.end(), v.begin(), v.end());
        return off;
    }
};

// conv `prefix` [out][in] (+ the BatchNorm `bn` behind it when present) -> folded copies; the raw tensors go to `raw`
int conv_bn(e2emv_ctx* ctx, TrainState* t, Pack& raw, const std::string& prefix, const std::string& bn, int out, int in, std::vector<float>& w,
            std::vector<float>& b) {
    const HostTensor* tw = find(ctx, prefix + ".weight");
    const HostTensor* tb = find(ctx, prefix + ".bias");
    if (!tw || !tb || (int64_t)tw->data.size() != (int64_t)out * in || (int)tb->data.size() != out)
        return set_err(ctx, E2EMV_ESTATE, "train_commit: '%s.{weight,bias}' missing or not [%d,%d]", prefix.c_str(), out, in);
    w = tw->data;
    b = tb->data;
    t->raw[prefix + ".weight"] = {raw.add(w), w.size()};
    t->raw[prefix + ".bias"] = {raw.add(b), b.size()};
    if (bn.empty()) return E2EMV_OK;
    const HostTensor* mean = find(ctx, bn + ".running_mean");
    if (!mean) return E2EMV_OK;
    const HostTensor* var = find(ctx, bn + ".running_var");
    const HostTensor* g = find(ctx, bn + ".weight");
    const HostTensor* be = find(ctx, bn + ".bias");
    if (!var || !g || !be || (int)mean->data.size() != out || (int)var->data.size() != out || (int)g->data.size() != out || (int)be->data.size() != out)
        return set_err(ctx, E2EMV_ESHAPE, "train_commit: BatchNorm '%s' incomplete", bn.c_str());
    t->raw[bn + ".weight"] = {raw.add(g->data), (size_t)out};
    t->raw[bn + ".bias"] = {raw.add(be->data), (size_t)out};
    t->raw[bn + ".running_mean"] = {raw.add(mean->data), (size_t)out};
    t->raw[bn + ".running_var"] = {raw.add(var->data), (size_t)out};
    if (t->bn_mode == E2EMV_BN_BATCH) {  // batch statistics: the convolution stays raw, the BatchNorm runs on the tape
        t->bns.push_back({bn, out, t->raw[bn + ".weight"].off, t->raw[bn + ".bias"].off});
        return E2EMV_OK;
    }
    for (int o = 0; o < out; ++o) {
        const double sc = (double)g->data[o] / std::sqrt((double)var->data[o] + 1e-5);
        for (int i = 0; i < in; ++i) w[(size_t)o * in + i] = (float)((double)w[(size_t)o * in + i] * sc);
        b[o] = (float)(((double)b[o] - (double)mean->data[o]) * sc + (double)be->data[o]);
    }
    return E2EMV_OK;
}

}  // namespace

// host part of e2emv_train_commit: folds BatchNorm / head order of the tensors handed over with e2emv_set_weight into the
// packed training weights (pk) and keeps the raw parameters (raw) for the un-folding of the gradients
static int train_build(e2emv_ctx* ctx, const e2emv_model_desc* m, TrainState* t, Pack& pk, Pack& raw) {
    const int D = m->desc_dim, H = m->num_heads;
    t->model = *m;
    const int d = D / H;
    std::vector<float> w, b;
    int rc;
    t->kdims = {3};
    for (int i = 0; i < m->n_kenc; ++i) t->kdims.push_back(m->kenc[i]);
    t->kdims.push_back(D);
    for (int c : t->kdims)
        if (c > 2 * D || (c != 3 && c % 4)) return set_err(ctx, E2EMV_ESHAPE, "train_commit: encoder width %d", c);
    const int nk = (int)t->kdims.size() - 1;
    for (int i = 0; i < nk; ++i) {
        const std::string pfx = "kenc.encoder." + std::to_string(3 * i);
        if ((rc = conv_bn(ctx, t, raw, pfx, i < nk - 1 ? "kenc.encoder." + std::to_string(3 * i + 1) : std::string(), t->kdims[i + 1], t->kdims[i], w, b))) return rc;
        t->kw.push_back(pk.add(w));
        t->kb.push_back(pk.add(b));
    }
    t->layers.resize(m->n_layers);
    for (int l = 0; l < m->n_layers; ++l) {
        TrainLayer& L = t->layers[l];
        L.type = m->layer_types[l] ? 1 : 0;
        const std::string base = "gnn.layers." + std::to_string(l);
        std::vector<float> wqkv((size_t)3 * D * D), bqkv((size_t)3 * D);
        for (int p = 0; p < 3; ++p) {
            if ((rc = conv_bn(ctx, t, raw, base + ".attn.proj." + std::to_string(p), "", D, D, w, b))) return rc;
            for (int h = 0; h < H; ++h)
                for (int dd = 0; dd < d; ++dd) {
                    const int src = dd * H + h, dst = p * D + h * d + dd;
                    memcpy(&wqkv[(size_t)dst * D], &w[(size_t)src * D], sizeof(float) * D);
                    bqkv[dst] = b[src];
                }
        }
        L.wqkv = pk.add(wqkv);
        L.bqkv = pk.add(bqkv);
        if ((rc = conv_bn(ctx, t, raw, base + ".attn.merge", "", D, D, w, b))) return rc;
        std::vector<float> wm((size_t)D * D);
        for (int o = 0; o < D; ++o)
            for (int h = 0; h < H; ++h)
                for (int dd = 0; dd < d; ++dd) wm[(size_t)o * D + h * d + dd] = w[(size_t)o * D + dd * H + h];
        L.wm = pk.add(wm);
        L.bm = pk.add(b);
        if ((rc = conv_bn(ctx, t, raw, base + ".mlp.0", base + ".mlp.1", 2 * D, 2 * D, w, b))) return rc;
        L.w0 = pk.add(w);
        L.b0 = pk.add(b);
        if ((rc = conv_bn(ctx, t, raw, base + ".mlp.3", "", D, 2 * D, w, b))) return rc;
        L.w1 = pk.add(w);
        L.b1 = pk.add(b);
    }
    if ((rc = conv_bn(ctx, t, raw, "final_proj", "", D, D, w, b))) return rc;
    t->wf = pk.add(w);
    t->bf = pk.add(b);
    t->conf_mlp = m->conf_mlp != 0;
    if (t->conf_mlp) {
        if ((rc = conv_bn(ctx, t, raw, "conf_mlp.0", "conf_mlp.1", D, 2 * D, w, b))) return rc;
        t->wc0 = pk.add(w);
        t->bc0 = pk.add(b);
        if ((rc = conv_bn(ctx, t, raw, "conf_mlp.3", "", 1, D, w, b))) return rc;
        t->wc1 = pk.add(w);
        t->bc1 = pk.add(b);
    }
    const HostTensor* bs = find(ctx, "bin_score");
    if (!bs || bs->data.size() != 1) return set_err(ctx, E2EMV_ESTATE, "train_commit: missing scalar 'bin_score'");
    t->bin_score = bs->data[0];
    t->alpha = pk.add(std::vector<float>{bs->data[0]});
    t->raw["bin_score"] = {raw.add(bs->data), 1};
    if (t->bn_mode == E2EMV_BN_BATCH && t->bns.size() != (size_t)(nk - 1 + m->n_layers + (t->conf_mlp ? 1 : 0)))
        return set_err(ctx, E2EMV_ESTATE, "train_commit: batch-statistics BatchNorm needs every BatchNorm's running_mean / running_var");
    t->w_floats = pk.host.size();
    t->raw_floats = raw.host.size();
    return E2EMV_OK;
}

extern "C" int e2emv_train_commit(e2emv_ctx* ctx, const e2emv_model_desc* m) {
    if (!ctx || !m) return E2EMV_EINVAL;
    E2EMV_LOCK(ctx);
    const int D = m->desc_dim, H = m->num_heads;
    if (D <= 0 || H <= 0 || D % H || D / H != 64) return set_err(ctx, E2EMV_ESHAPE, "train_commit: head dim must be 64 (D=%d H=%d)", D, H);
    if (m->n_kenc < 1 || m->n_kenc > E2EMV_MAX_KENC || m->n_layers < 0 || m->n_layers > E2EMV_MAX_LAYERS) return set_err(ctx, E2EMV_ESHAPE, "train_commit: bad layer counts");
    (void)hipSetDevice(ctx->device);
    TrainState* t = new TrainState();
    t->bn_mode = ctx->train_bn_mode;
    Pack pk, raw;
    {   // (every optimiser step comes through here: no re-allocation while the ~50 MB packs grow)
        const TrainState* prev = ts_of(ctx);
        size_t total = 0;
        for (const auto& kv : ctx->raw) total += kv.second.data.size() + 64;
        pk.host.reserve(prev ? prev->w_floats + 64 : total);
        raw.host.reserve(prev ? prev->raw_floats + 64 : total);
    }
    if (int rc = train_build(ctx, m, t, pk, raw)) { delete t; return rc; }
    // Every optimiser step comes through here (the parameters changed).  A context that already trains this model keeps
    // its arenas and its tape: the new values are copied over the old ones - no free / malloc, one synchronisation (the
    // previous step's kernels may still read the weights)
    TrainState* old = ts_of(ctx);
    E2EMV_HIP(ctx, hipDeviceSynchronize());
    const bool reuse = old && old->w_floats == t->w_floats && old->raw_floats == t->raw_floats && memcmp(&old->model, m, sizeof(*m)) == 0 && old->d_w && old->d_maps;
    if (reuse) {
        t->d_w = old->d_w; t->d_gw = old->d_gw; t->d_raw = old->d_raw; t->d_graw = old->d_graw; t->d_maps = old->d_maps;
        t->d_tape = old->d_tape; t->tape_bytes = old->tape_bytes;
        delete old;  // (the host side only: the device buffers moved over)
        ctx->train = t;
        E2EMV_HIP(ctx, hipMemcpy(t->d_w, pk.host.data(), t->w_floats * sizeof(float), hipMemcpyHostToDevice));
        E2EMV_HIP(ctx, hipMemcpy(t->d_raw, raw.host.data(), t->raw_floats * sizeof(float), hipMemcpyHostToDevice));
        E2EMV_HIP(ctx, hipMemset(t->d_graw, 0, t->raw_floats * sizeof(float)));
        E2EMV_NULL_STREAM_FENCE(ctx);
        return E2EMV_OK;
    }
    train_free(ctx);
    ctx->train = t;
    const int d = D / H;
    E2EMV_HIP(ctx, hipMalloc((void**)&t->d_w, t->w_floats * sizeof(float)));
    E2EMV_HIP(ctx, hipMalloc((void**)&t->d_gw, t->w_floats * sizeof(float)));
    E2EMV_HIP(ctx, hipMalloc((void**)&t->d_raw, t->raw_floats * sizeof(float)));
    E2EMV_HIP(ctx, hipMalloc((void**)&t->d_graw, t->raw_floats * sizeof(float)));
    E2EMV_HIP(ctx, hipMemcpy(t->d_w, pk.host.data(), t->w_floats * sizeof(float), hipMemcpyHostToDevice));
    E2EMV_HIP(ctx, hipMemcpy(t->d_raw, raw.host.data(), t->raw_floats * sizeof(float), hipMemcpyHostToDevice));
    E2EMV_HIP(ctx, hipMemset(t->d_graw, 0, t->raw_floats * sizeof(float)));
    std::vector<int> map(D);
    for (int h = 0; h < H; ++h)
        for (int dd = 0; dd < d; ++dd) map[dd * H + h] = h * d + dd;
    E2EMV_HIP(ctx, hipMalloc((void**)&t->d_maps, D * sizeof(int)));
    E2EMV_HIP(ctx, hipMemcpy(t->d_maps, map.data(), D * sizeof(int), hipMemcpyHostToDevice));
    E2EMV_NULL_STREAM_FENCE(ctx);
    return E2EMV_OK;
}

static size_t al256(size_t b) { return (b + 255) & ~size_t(255); }

// After an optimiser step: the new parameter values straight from the caller's DEVICE tensors into the training arena of a
// context that already trains this model - D2D copies into the raw arena, the folds (BatchNorm, head order) as kernels, all
// in stream order: no host copy of the weights, no synchronisation, the tape and the arenas stay.
extern "C" int e2emv_train_update(e2emv_ctx* ctx, const e2emv_model_desc* m, int n, const char* const* keys, const float* const* d_params,
                                  const int64_t* numels, float bin_score, void* stream) {
    if (!ctx || !m || n < 0 || (n && (!keys || !d_params || !numels))) return E2EMV_EINVAL;
    E2EMV_ENTER(ctx, stream);
    TrainState* t = ts_of(ctx);
    if (!t || !t->d_w || !t->d_raw || !t->d_maps || memcmp(&t->model, m, sizeof(*m)) != 0)
        return set_err(ctx, E2EMV_ESTATE, "train_update: no training arena of this model on the context (e2emv_train_commit first)");
    if (t->bn_mode != ctx->train_bn_mode)
        return set_err(ctx, E2EMV_ESTATE, "train_update: the BatchNorm mode changed since e2emv_train_commit (commit again)");
    (void)hipSetDevice(ctx->device);
    hipStream_t s = (hipStream_t)stream;
    // pass 1 validates every entry, pass 2 enqueues: a rejected call leaves the raw arena, the folded weights and the tape as
    // they were (the caller's owner record still describes them)
    size_t seen = 0;
    std::vector<std::pair<size_t, int>> copies;  // (offset in the raw arena, entry)
    copies.reserve(t->raw.size());
    for (int i = 0; i < n; ++i) {
        if (!keys[i] || !d_params[i]) return set_err(ctx, E2EMV_EINVAL, "train_update: null entry %d", i);
        std::string k(keys[i]);
        if (k.rfind("module.", 0) == 0) k = k.substr(7);
        auto it = t->raw.find(k);
        if (it == t->raw.end()) continue;  // (a tensor the differentiable path does not use)
        if ((int64_t)it->second.numel != numels[i])
            return set_err(ctx, E2EMV_ESHAPE, "train_update: '%s' has %zu elements, not %lld", keys[i], it->second.numel, (long long)numels[i]);
        copies.emplace_back(it->second.off, i);
        ++seen;
    }
    if (seen != t->raw.size()) return set_err(ctx, E2EMV_ESTATE, "train_update: %zu of the %zu tensors of the model handed over", seen, t->raw.size());
    // from here on the arena is being rewritten: a failure below (a HIP error) must not leave a tape that pairs with it
    t->have_tape = false;
    for (const auto& c : copies)
        E2EMV_HIP(ctx, hipMemcpyAsync(t->d_raw + c.first, d_params[c.second], numels[c.second] * sizeof(float), hipMemcpyDeviceToDevice, s));
    const int D = m->desc_dim;
    float* W = t->d_w;
    auto ref = [&](const std::string& k) -> const float* { auto it = t->raw.find(k); return it == t->raw.end() ? nullptr : t->d_raw + it->second.off; };
    auto fold = [&](const std::string& conv, const std::string& bn, float* Wf, float* bf, int64_t ldwf, int rows, int cols, const int* rmap, int rbase, const int* cmap) {
        FoldArgs a{};
        a.W = ref(conv + ".weight"); a.b = ref(conv + ".bias");
        if (!bn.empty() && ref(bn + ".running_mean") && t->bn_mode == E2EMV_BN_FROZEN) { a.gamma = ref(bn + ".weight"); a.beta = ref(bn + ".bias"); a.mean = ref(bn + ".running_mean"); a.var = ref(bn + ".running_var"); }
        a.Wf = Wf + (int64_t)rbase * ldwf; a.bf = bf + rbase; a.ldwf = ldwf; a.col0 = 0; a.rows = rows; a.cols = cols; a.rmap = rmap; a.cmap = cmap;
        hipLaunchKernelGGL(fold_kernel, dim3(rows), dim3(256), 0, s, a);
    };
    const int nk = (int)t->kdims.size() - 1;
    for (int i = 0; i < nk; ++i)
        fold("kenc.encoder." + std::to_string(3 * i), i < nk - 1 ? "kenc.encoder." + std::to_string(3 * i + 1) : std::string(), W + t->kw[i], W + t->kb[i], t->kdims[i],
             t->kdims[i + 1], t->kdims[i], nullptr, 0, nullptr);
    for (int l = 0; l < (int)t->layers.size(); ++l) {
        const TrainLayer& Lw = t->layers[l];
        const std::string base = "gnn.layers." + std::to_string(l);
        for (int p = 0; p < 3; ++p) fold(base + ".attn.proj." + std::to_string(p), "", W + Lw.wqkv, W + Lw.bqkv, D, D, D, t->d_maps, p * D, nullptr);
        fold(base + ".attn.merge", "", W + Lw.wm, W + Lw.bm, D, D, D, nullptr, 0, t->d_maps);
        fold(base + ".mlp.0", base + ".mlp.1", W + Lw.w0, W + Lw.b0, 2 * D, 2 * D, 2 * D, nullptr, 0, nullptr);
        fold(base + ".mlp.3", "", W + Lw.w1, W + Lw.b1, 2 * D, D, 2 * D, nullptr, 0, nullptr);
    }
    fold("final_proj", "", W + t->wf, W + t->bf, D, D, D, nullptr, 0, nullptr);
    if (t->conf_mlp) {
        fold("conf_mlp.0", "conf_mlp.1", W + t->wc0, W + t->bc0, 2 * D, D, 2 * D, nullptr, 0, nullptr);
        fold("conf_mlp.3", "", W + t->wc1, W + t->bc1, D, 1, D, nullptr, 0, nullptr);
    }
    E2EMV_CHECK_LAUNCH(ctx, "fold kernels");
    E2EMV_HIP(ctx, hipMemcpyAsync(W + t->alpha, ref("bin_score"), sizeof(float), hipMemcpyDeviceToDevice, s));
    t->bin_score = bin_score;
    E2EMV_HIP(ctx, hipMemsetAsync(t->d_graw, 0, t->raw_floats * sizeof(float), s));
    t->have_tape = false;
    return E2EMV_OK;
}

extern "C" int e2emv_matcher_forward_train(e2emv_ctx* ctx, const e2emv_forward_desc* fd, const float* const* d_kpts, const float* const* d_kscores,
                                           const void* const* d_desc, float* const* d_logZ, void* stream) {
    if (!ctx || !fd || !d_kpts || !d_kscores || !d_desc || !d_logZ) return E2EMV_EINVAL;
    E2EMV_ENTER(ctx, stream);
    TrainState* t = ts_of(ctx);
    if (!t) return set_err(ctx, E2EMV_ESTATE, "matcher_forward_train: e2emv_train_commit first");
    const int B = fd->batch, T = fd->tuple_size, N = fd->n_kpts;
    const int D = t->model.desc_dim, H = t->model.num_heads, L = (int)t->layers.size();
    if (B <= 0 || T < 2 || T > E2EMV_MAX_TUPLE || N <= 0 || N > 2048) return set_err(ctx, E2EMV_ESHAPE, "matcher_forward_train: batch=%d tuple_size=%d n_kpts=%d", B, T, N);
    if (T > 2 && !(fd->flags & E2EMV_FLAG_MULTI_FRAME)) return set_err(ctx, E2EMV_ESHAPE, "matcher_forward_train: tuples of more than 2 images need multi_frame_matching");
    for (int i = 0; i < T; ++i)
        if (fd->n_kpts_img[i] > 0 && fd->n_kpts_img[i] != N) return set_err(ctx, E2EMV_ESHAPE, "matcher_forward_train: all images of a call carry the same number of keypoints");
    if (fd->sinkhorn_iters < 0) return set_err(ctx, E2EMV_EINVAL, "negative sinkhorn_iters");
    if (t->bn_mode != ctx->train_bn_mode)
        return set_err(ctx, E2EMV_ESTATE, "matcher_forward_train: the BatchNorm mode changed since e2emv_train_commit (commit again)");
    const bool bnb = t->bn_mode == E2EMV_BN_BATCH;
    if (bnb && (int64_t)B * N < 2) return set_err(ctx, E2EMV_ESHAPE, "matcher_forward_train: batch statistics need more than one value per channel");
    (void)hipSetDevice(ctx->device);
    hipStream_t s = (hipStream_t)stream;
    const int n_rows = (N + 127) / 128 * 128, n_img = B * T, P = T * (T - 1) / 2, iters = fd->sinkhorn_iters, ldS = (N + 3) / 4 * 4;
    const int64_t Mtot = (int64_t)n_img * n_rows;
    const int nk = (int)t->kdims.size() - 1;
    // ---- tape ----
    size_t need = al256((size_t)Mtot * 4 * 4);
    for (int i = 1; i < nk; ++i) need += al256((size_t)Mtot * t->kdims[i] * 4);
    need += (size_t)(L + 1) * al256((size_t)Mtot * D * 4) + (size_t)L * (al256((size_t)Mtot * 3 * D * 4) + 2 * al256((size_t)Mtot * D * 4) + al256((size_t)Mtot * 2 * D * 4));
    need += al256((size_t)Mtot * D * 4) + al256((size_t)P * B * N * ldS * 4) + al256((size_t)P * B * (iters + 1) * 2 * (N + 1) * 4);
    if (t->conf_mlp) need += (size_t)P * (al256((size_t)B * N * 2 * D * 4) + al256((size_t)B * N * D * 4));
    if (bnb) {  // y and the statistics of every BatchNorm, the partial sums
        for (int j = 1; j < nk; ++j) need += al256((size_t)Mtot * t->kdims[j] * 4) + al256((size_t)T * 3 * t->kdims[j] * 4);
        need += (size_t)L * (al256((size_t)Mtot * 2 * D * 4) + al256((size_t)T * 3 * 2 * D * 4));
        if (t->conf_mlp) need += (size_t)P * al256((size_t)B * N * D * 4) + al256((size_t)P * 3 * D * 4);
        need += al256((size_t)T * BN_MAX_CHUNKS * 2 * 2 * D * 8);
    }
    if (need > t->tape_bytes) {
        E2EMV_HIP(ctx, hipDeviceSynchronize());
        if (t->d_tape) E2EMV_HIP(ctx, hipFree(t->d_tape));
        t->d_tape = nullptr;
        t->tape_bytes = 0;
        if (hipMalloc((void**)&t->d_tape, need) != hipSuccess) {
            (void)hipGetLastError();
            return set_err(ctx, E2EMV_ENOMEM, "matcher_forward_train: tape of %zu bytes", need);
        }
        t->tape_bytes = need;
    }
    E2EMV_HIP(ctx, hipMemsetAsync(t->d_tape, 0, need, s));  // padded rows must be finite zeros wherever a GEMM does not write them
    char* w = t->d_tape;
    auto take = [&](size_t bytes) { float* p = (float*)w; w += al256(bytes); return p; };
    t->t_inp = take((size_t)Mtot * 4 * 4);
    t->t_kh.assign(nk, nullptr);
    for (int i = 1; i < nk; ++i) t->t_kh[i] = take((size_t)Mtot * t->kdims[i] * 4);  // t_kh[i]: output of encoder layer i - 1 (width kdims[i])
    t->t_x.assign(L + 1, nullptr);
    for (int l = 0; l <= L; ++l) t->t_x[l] = take((size_t)Mtot * D * 4);
    t->t_qkv.assign(L, nullptr); t->t_att.assign(L, nullptr); t->t_msg.assign(L, nullptr); t->t_h.assign(L, nullptr);
    for (int l = 0; l < L; ++l) {
        t->t_qkv[l] = take((size_t)Mtot * 3 * D * 4);
        t->t_att[l] = take((size_t)Mtot * D * 4);
        t->t_msg[l] = take((size_t)Mtot * D * 4);
        t->t_h[l] = take((size_t)Mtot * 2 * D * 4);
    }
    t->t_mdesc = take((size_t)Mtot * D * 4);
    t->t_S = take((size_t)P * B * N * ldS * 4);
    t->t_uv = take((size_t)P * B * (iters + 1) * 2 * (N + 1) * 4);
    t->t_cfeat.assign(P, nullptr); t->t_chid.assign(P, nullptr); t->t_cmatch.assign(P, nullptr);
    if (t->conf_mlp)
        for (int q = 0; q < P; ++q) {
            t->t_cfeat[q] = take((size_t)B * N * 2 * D * 4);
            t->t_chid[q] = take((size_t)B * N * D * 4);
        }
    t->t_ky.assign(nk, nullptr); t->t_kst.assign(nk, nullptr); t->t_hy.assign(L, nullptr); t->t_hst.assign(L, nullptr); t->t_cy.assign(P, nullptr);
    t->t_cst = nullptr; t->t_part = nullptr;
    if (bnb) {
        for (int j = 1; j < nk; ++j) { t->t_ky[j] = take((size_t)Mtot * t->kdims[j] * 4); t->t_kst[j] = take((size_t)T * 3 * t->kdims[j] * 4); }
        for (int l = 0; l < L; ++l) { t->t_hy[l] = take((size_t)Mtot * 2 * D * 4); t->t_hst[l] = take((size_t)T * 3 * 2 * D * 4); }
        if (t->conf_mlp) {
            for (int q = 0; q < P; ++q) t->t_cy[q] = take((size_t)B * N * D * 4);
            t->t_cst = take((size_t)P * 3 * D * 4);
        }
        t->t_part = (double*)take((size_t)T * BN_MAX_CHUNKS * 2 * 2 * D * 8);
    }
    t->B = B; t->T = T; t->N = N; t->n_rows = n_rows; t->iters = iters; t->P = P; t->ldS = ldS; t->Mtot = Mtot;
    t->have_tape = false;

    // ---- ingest: descriptors -> x_0 (desc part), keypoints -> encoder layer 0 ----
    int Nt[E2EMV_MAX_TUPLE] = {0};
    IngestParams ip{};
    for (int i = 0; i < T; ++i) {
        if (!d_kpts[i] || !d_kscores[i] || !d_desc[i]) return set_err(ctx, E2EMV_EINVAL, "matcher_forward_train: null input for image %d", i);
        ip.kpts[i] = d_kpts[i]; ip.ksc[i] = d_kscores[i]; ip.desc[i] = d_desc[i];
        ip.img_w[i] = fd->img_w[i]; ip.img_h[i] = fd->img_h[i];
        ip.Nimg[i] = N; Nt[i] = N;
    }
    ip.B = B; ip.T = T; ip.n_rows = n_rows; ip.D = D; ip.c0 = t->kdims[1]; ip.f16 = fd->desc_dtype == E2EMV_DESC_F16;
    ip.w0 = t->d_w + t->kw[0]; ip.b0 = t->d_w + t->kb[0]; ip.x0 = t->t_x[0]; ip.h0 = t->t_kh[1]; ip.inp = t->t_inp;
    hipLaunchKernelGGL(ingest_transpose, dim3(n_rows / 64, D / 64, n_img), dim3(256), 0, s, ip);
    hipLaunchKernelGGL(ingest_kenc0, dim3((n_rows + 255) / 256, n_img), dim3(256), 0, s, ip);
    E2EMV_CHECK_LAUNCH(ctx, "ingest kernels");
    int rc;
    if (bnb) {  // layer 0 again, without the BatchNorm ingest_kenc0 fuses: y, then the batch-statistics BN + ReLU over t_kh[1]
        const int c0 = t->kdims[1];
        hipLaunchKernelGGL(kenc0_conv_kernel, dim3(ew_grid(Mtot * c0)), dim3(256), 0, s, (const float*)t->t_inp, (const float*)t->d_w + t->kw[0],
                           (const float*)t->d_w + t->kb[0], c0, Mtot, t->t_ky[1]);
        E2EMV_CHECK_LAUNCH(ctx, "kenc0_conv_kernel");
        if ((rc = bn_forward(ctx, bn_images(t, 0, t->t_ky[1], t->t_kh[1], t->t_kst[1], t->t_part), T, s))) return rc;
    }
    // encoder layers 1 .. nk-1; the last adds the descriptors (x_0 = desc + kenc)
    for (int i = 1; i < nk; ++i) {
        const int cin = t->kdims[i], cout = t->kdims[i + 1];
        const bool last = i == nk - 1;
        GemmArgs g;
        g.M = (int)Mtot; g.N = cout; g.K = cin; g.K1 = cin; g.A = t->t_kh[i]; g.lda = cin;
        g.W = t->d_w + t->kw[i]; g.ldw = cin; g.bias = t->d_w + t->kb[i]; g.relu = !last && !bnb;
        if (last) { g.R = t->t_x[0]; g.ldr = D; g.C = t->t_x[0]; g.ldc = D; }
        else { g.C = bnb ? t->t_ky[i + 1] : t->t_kh[i + 1]; g.ldc = cout; }
        if ((rc = launch_gemm_nt(ctx, g, s))) return rc;
        if (bnb && !last && (rc = bn_forward(ctx, bn_images(t, i, t->t_ky[i + 1], t->t_kh[i + 1], t->t_kst[i + 1], t->t_part), T, s))) return rc;
    }
    // ---- attentional GNN (merge NOT folded: its parameters get their own gradients) ----
    for (int l = 0; l < L; ++l) {
        const TrainLayer& Lw = t->layers[l];
        GemmArgs g;
        g.M = (int)Mtot; g.N = 3 * D; g.K = D; g.K1 = D; g.A = t->t_x[l]; g.lda = D; g.W = t->d_w + Lw.wqkv; g.ldw = D; g.bias = t->d_w + Lw.bqkv;
        g.C = t->t_qkv[l]; g.ldc = 3 * D;
        if ((rc = launch_gemm_nt(ctx, g, s))) return rc;
        if ((rc = launch_attention(ctx, B, T, n_rows, Nt, D, H, t->t_qkv[l], Lw.type, t->t_att[l], s))) return rc;
        g = GemmArgs();
        g.M = (int)Mtot; g.N = D; g.K = D; g.K1 = D; g.A = t->t_att[l]; g.lda = D; g.W = t->d_w + Lw.wm; g.ldw = D; g.bias = t->d_w + Lw.bm;
        g.C = t->t_msg[l]; g.ldc = D;
        if ((rc = launch_gemm_nt(ctx, g, s))) return rc;
        g = GemmArgs();
        g.M = (int)Mtot; g.N = 2 * D; g.K = 2 * D; g.K1 = D; g.A = t->t_x[l]; g.lda = D; g.A2 = t->t_msg[l]; g.lda2 = D;
        g.W = t->d_w + Lw.w0; g.ldw = 2 * D; g.bias = t->d_w + Lw.b0; g.relu = !bnb; g.C = bnb ? t->t_hy[l] : t->t_h[l]; g.ldc = 2 * D;
        if ((rc = launch_gemm_nt(ctx, g, s))) return rc;
        if (bnb && (rc = bn_forward(ctx, bn_images(t, nk - 1 + l, t->t_hy[l], t->t_h[l], t->t_hst[l], t->t_part), T, s))) return rc;
        g = GemmArgs();
        g.M = (int)Mtot; g.N = D; g.K = 2 * D; g.K1 = 2 * D; g.A = t->t_h[l]; g.lda = 2 * D; g.W = t->d_w + Lw.w1; g.ldw = 2 * D; g.bias = t->d_w + Lw.b1;
        g.R = t->t_x[l]; g.ldr = D; g.C = t->t_x[l + 1]; g.ldc = D;
        if ((rc = launch_gemm_nt(ctx, g, s))) return rc;
    }
    {
        GemmArgs g;
        g.M = (int)Mtot; g.N = D; g.K = D; g.K1 = D; g.A = t->t_x[L]; g.lda = D; g.W = t->d_w + t->wf; g.ldw = D; g.bias = t->d_w + t->bf;
        g.C = t->t_mdesc; g.ldc = D;
        if ((rc = launch_gemm_nt(ctx, g, s))) return rc;
    }
    // ---- scores, Sinkhorn (log domain, u_t / v_t of every iteration kept), log assignment ----
    const int64_t tuple_stride = (int64_t)T * n_rows * D;
    SkT sk = sk_problem(nullptr, ldS, N, t->bin_score);
    const int64_t uvs = (int64_t)(iters + 1) * 2 * (N + 1);  // per problem
    int pidx = 0;
    for (int j = 0; j < T; ++j)
        for (int i = 0; i < j; ++i, ++pidx) {
            float* S = t->t_S + (int64_t)pidx * B * N * ldS;
            GemmArgs g;
            g.batch = B; g.M = N; g.N = N; g.K = D; g.K1 = D;
            g.A = t->t_mdesc + (int64_t)i * n_rows * D; g.lda = D; g.sA = tuple_stride;
            g.W = t->t_mdesc + (int64_t)j * n_rows * D; g.ldw = D; g.sW = tuple_stride;
            g.C = S; g.ldc = ldS; g.sC = (int64_t)N * ldS;
            g.scale = 1.0f / sqrtf((float)D);
            if ((rc = launch_gemm_nt(ctx, g, s))) return rc;
            sk.S = S;
            float* uv = t->t_uv + (int64_t)pidx * B * uvs;  // [b][t][{u, v}][N + 1]
            if (!d_logZ[pidx]) return set_err(ctx, E2EMV_EINVAL, "matcher_forward_train: null logZ for pair %d", pidx);
            if ((rc = sinkhorn_tape_forward(ctx, sk, B, iters, uv, d_logZ[pidx], 0, s))) return rc;
        }
    t->have_tape = true;
    return E2EMV_OK;
}

// confidence head of pair `pair` (order (0,1), (0,2), (1,2), ...) on the mdesc of the tape: conf[b][n] = sigmoid(conf_mlp([mdesc_i[n] |
// mdesc_j[match n]])) for matched n, 0 otherwise.  d_matches0 must stay alive until e2emv_matcher_backward (it is read again).
extern "C" int e2emv_conf_forward_train(e2emv_ctx* ctx, int pair, const int64_t* d_matches0, float* d_conf, void* stream) {
    if (!ctx || !d_matches0 || !d_conf) return E2EMV_EINVAL;
    E2EMV_ENTER(ctx, stream);
    TrainState* t = ts_of(ctx);
    if (!t || !t->have_tape) return set_err(ctx, E2EMV_ESTATE, "conf_forward_train: no tape - e2emv_matcher_forward_train first");
    if (!t->conf_mlp) return set_err(ctx, E2EMV_ESTATE, "conf_forward_train: the committed model has no conf_mlp");
    if (pair < 0 || pair >= t->P) return set_err(ctx, E2EMV_EINVAL, "conf_forward_train: pair %d of %d", pair, t->P);
    (void)hipSetDevice(ctx->device);
    hipStream_t s = (hipStream_t)stream;
    const int B = t->B, T = t->T, N = t->N, n_rows = t->n_rows, D = t->model.desc_dim;
    int pi = 0, pj = 1, q = 0;
    for (int j = 0; j < T; ++j)
        for (int i = 0; i < j; ++i, ++q)
            if (q == pair) { pi = i; pj = j; }
    const int64_t tuple_stride = (int64_t)T * n_rows * D;
    float* feat = t->t_cfeat[pair];
    float* hid = t->t_chid[pair];
    hipLaunchKernelGGL(conf_feat_kernel, dim3((N + 3) / 4, B), dim3(256), 0, s, N, D, (const float*)t->t_mdesc + (int64_t)pi * n_rows * D,
                       (const float*)t->t_mdesc + (int64_t)pj * n_rows * D, tuple_stride, d_matches0, feat);
    E2EMV_CHECK_LAUNCH(ctx, "conf_feat_kernel");
    GemmArgs g;
    g.M = B * N; g.N = D; g.K = 2 * D; g.K1 = 2 * D; g.A = feat; g.lda = 2 * D; g.W = t->d_w + t->wc0; g.ldw = 2 * D; g.bias = t->d_w + t->bc0;
    const bool bnb = t->bn_mode == E2EMV_BN_BATCH;
    g.relu = !bnb; g.C = bnb ? t->t_cy[pair] : hid; g.ldc = D;
    if (int rc = launch_gemm_nt(ctx, g, s)) return rc;
    if (bnb)
        if (int rc = bn_forward(ctx, bn_conf(t, t->t_cy[pair], hid, t->t_cst + (int64_t)pair * 3 * D, t->t_part), 1, s)) return rc;
    hipLaunchKernelGGL(conf_fwd_kernel, dim3((unsigned)(((int64_t)B * N + 3) / 4)), dim3(256), 0, s, (int64_t)B * N, D, (const float*)hid,
                       (const float*)t->d_w + t->wc1, (const float*)t->d_w + t->bc1, d_matches0, d_conf);
    E2EMV_CHECK_LAUNCH(ctx, "conf_fwd_kernel");
    t->t_cmatch[pair] = d_matches0;
    return E2EMV_OK;
}

// attention backward of one layer (head dim 64): qkv [B*T][n_rows][3D] (N valid rows per image), d att [B*T][n_rows][D] ->
// dqkv [B*T][n_rows][3D] (zeroed here); P / dP: scratch [B*H][N][ldP] each, ldP = N keys per source image
static int attention_backward(e2emv_ctx* ctx, int B, int T, int N, int n_rows, int D, int H, bool cross, const float* qkv, const float* datt, float* dqkv,
                              float* Pb, float* dPb, hipStream_t s) {
    const int n_src = cross ? T - 1 : 1;
    const int64_t ldP = (int64_t)n_src * N;
    const int64_t img3 = (int64_t)n_rows * 3 * D, img1 = (int64_t)n_rows * D;
    E2EMV_HIP(ctx, hipMemsetAsync(dqkv, 0, (size_t)B * T * n_rows * 3 * D * sizeof(float), s));
    int rc;
    for (int tq = 0; tq < T; ++tq) {
        auto src_of = [&](int si) { return !cross ? tq : (si < tq ? si : si + 1); };
        for (int pass = 0; pass < 2; ++pass)  // P = q k^T / 8 (pass 0), dP = dO v^T (pass 1)
            for (int si = 0; si < n_src; ++si) {
                const int ts = src_of(si);
                GG g;
                g.batch = B * H; g.inner = H; g.M = N; g.N = N; g.K = 64;
                if (pass == 0) { g.A = qkv + tq * img3; g.am = 3 * D; g.az0 = T * img3; g.az1 = 64; g.alpha = 0.125f; }
                else { g.A = datt + tq * img1; g.am = D; g.az0 = T * img1; g.az1 = 64; }
                g.ak = 1;
                g.B = qkv + ts * img3 + (pass == 0 ? D : 2 * D); g.bk = 1; g.bn = 3 * D; g.bz0 = T * img3; g.bz1 = 64;
                g.C = (pass == 0 ? Pb : dPb) + (int64_t)si * N; g.ldc = ldP; g.cz0 = (int64_t)H * N * ldP; g.cz1 = (int64_t)N * ldP;
                if ((rc = launch_gg(ctx, g, s))) return rc;
            }
        hipLaunchKernelGGL(softmax_rows_kernel, dim3((N + 3) / 4, B * H), dim3(256), 0, s, Pb, N, (int)ldP, ldP, (int64_t)N * ldP);
        hipLaunchKernelGGL(softmax_bwd_rows_kernel, dim3((N + 3) / 4, B * H), dim3(256), 0, s, (const float*)Pb, dPb, N, (int)ldP, ldP, (int64_t)N * ldP, 0.125f);
        E2EMV_CHECK_LAUNCH(ctx, "softmax backward kernels");
        for (int si = 0; si < n_src; ++si) {
            const int ts = src_of(si);
            GG g;  // dq += dS k
            g.batch = B * H; g.inner = H; g.M = N; g.N = 64; g.K = N;
            g.A = dPb + (int64_t)si * N; g.am = ldP; g.ak = 1; g.az0 = (int64_t)H * N * ldP; g.az1 = (int64_t)N * ldP;
            g.B = qkv + ts * img3 + D; g.bk = 3 * D; g.bn = 1; g.bz0 = T * img3; g.bz1 = 64;
            g.C = dqkv + tq * img3; g.ldc = 3 * D; g.cz0 = T * img3; g.cz1 = 64; g.mode = 1;
            if ((rc = launch_gg(ctx, g, s))) return rc;
            g = GG();  // dk += dS^T q
            g.batch = B * H; g.inner = H; g.M = N; g.N = 64; g.K = N;
            g.A = dPb + (int64_t)si * N; g.am = 1; g.ak = ldP; g.az0 = (int64_t)H * N * ldP; g.az1 = (int64_t)N * ldP;
            g.B = qkv + tq * img3; g.bk = 3 * D; g.bn = 1; g.bz0 = T * img3; g.bz1 = 64;
            g.C = dqkv + ts * img3 + D; g.ldc = 3 * D; g.cz0 = T * img3; g.cz1 = 64; g.mode = 1;
            if ((rc = launch_gg(ctx, g, s))) return rc;
            g = GG();  // dv += P^T dO
            g.batch = B * H; g.inner = H; g.M = N; g.N = 64; g.K = N;
            g.A = Pb + (int64_t)si * N; g.am = 1; g.ak = ldP; g.az0 = (int64_t)H * N * ldP; g.az1 = (int64_t)N * ldP;
            g.B = datt + tq * img1; g.bk = D; g.bn = 1; g.bz0 = T * img1; g.bz1 = 64;
            g.C = dqkv + ts * img3 + 2 * D; g.ldc = 3 * D; g.cz0 = T * img3; g.cz1 = 64; g.mode = 1;
            if ((rc = launch_gg(ctx, g, s))) return rc;
        }
    }
    return E2EMV_OK;
}

extern "C" int e2emv_matcher_backward(e2emv_ctx* ctx, const float* const* d_dlogZ, const float* const* d_dconf, void* stream) {
    if (!ctx || !d_dlogZ) return E2EMV_EINVAL;
    E2EMV_ENTER(ctx, stream);
    TrainState* t = ts_of(ctx);
    if (!t || !t->have_tape) return set_err(ctx, E2EMV_ESTATE, "matcher_backward: no tape - e2emv_matcher_forward_train first");
    (void)hipSetDevice(ctx->device);
    hipStream_t s = (hipStream_t)stream;
    const int B = t->B, T = t->T, N = t->N, n_rows = t->n_rows, iters = t->iters, P = t->P, ldS = t->ldS;
    const int D = t->model.desc_dim, H = t->model.num_heads, L = (int)t->layers.size();
    const int64_t Mtot = t->Mtot;
    const int nk = (int)t->kdims.size() - 1;
    const int n_src_max = T > 2 ? T - 1 : 1;
    // ---- workspace ----
    const size_t sz_x = al256((size_t)Mtot * D * 4), sz_2 = al256((size_t)Mtot * 2 * D * 4), sz_3 = al256((size_t)Mtot * 3 * D * 4);
    const size_t sz_C = al256((size_t)B * (N + 1) * (N + 1) * 4), sz_v = al256((size_t)B * (N + 1) * 4);
    const size_t sz_P = al256((size_t)B * H * N * n_src_max * N * 4);
    const bool bnb = t->bn_mode == E2EMV_BN_BATCH;
    const size_t sz_bn = bnb ? al256((size_t)T * BN_MAX_CHUNKS * 2 * 2 * D * 8) : 0;
    const size_t need = 3 * sz_x + 2 * sz_2 + sz_3 + sz_C + 3 * sz_v + 2 * sz_P + sz_bn + 4096;
    int rc = ws_reserve(ctx, need);
    if (rc) return rc;
    char* w = ctx->d_ws;
    auto take = [&](size_t bytes) { float* p = (float*)w; w += bytes; return p; };
    float* dx = take(sz_x);
    float* datt = take(sz_x);
    float* dmd = take(sz_x);
    float* dh = take(sz_2);
    float* dcat = take(sz_2);
    float* dqkv = take(sz_3);
    float* dC = take(sz_C);
    float* du = take(sz_v);
    float* dv = take(sz_v);
    float* dv2 = take(sz_v);
    float* Pb = take(sz_P);
    float* dPb = take(sz_P);
    double* bpart = bnb ? (double*)take(sz_bn) : nullptr;
    float* gw = t->d_gw;
    const float* W = t->d_w;
    E2EMV_HIP(ctx, hipMemsetAsync(gw, 0, t->w_floats * sizeof(float), s));
    E2EMV_HIP(ctx, hipMemsetAsync(dmd, 0, (size_t)Mtot * D * sizeof(float), s));
    // ---- Sinkhorn reverse sweep and the score matrix, per pair ----
    const int64_t tuple_stride = (int64_t)T * n_rows * D;
    SkT sk = sk_problem(nullptr, ldS, N, t->bin_score);
    const int64_t uvs = (int64_t)(iters + 1) * 2 * (N + 1);
    const int64_t per = (int64_t)(N + 1) * (N + 1);
    int pidx = 0;
    for (int j = 0; j < T; ++j)
        for (int i = 0; i < j; ++i, ++pidx) {
            if (!d_dlogZ[pidx]) continue;  // no gradient reaches this pair's scores
            sk.S = t->t_S + (int64_t)pidx * B * N * ldS;
            const float* uv = t->t_uv + (int64_t)pidx * B * uvs;
            if ((rc = sinkhorn_tape_backward(ctx, sk, B, iters, uv, d_dlogZ[pidx], dC, du, dv, dv2, gw + t->alpha, 0, s))) return rc;
            // scores = md_i md_j^T / sqrt(D):  d md_i += dS md_j / sqrt(D),  d md_j += dS^T md_i / sqrt(D)
            const float sc = 1.0f / sqrtf((float)D);
            GG g;
            g.batch = B; g.M = N; g.N = D; g.K = N;
            g.A = dC; g.am = N + 1; g.ak = 1; g.az0 = per;
            g.B = t->t_mdesc + (int64_t)j * n_rows * D; g.bk = D; g.bn = 1; g.bz0 = tuple_stride;
            g.C = dmd + (int64_t)i * n_rows * D; g.ldc = D; g.cz0 = tuple_stride; g.alpha = sc; g.mode = 1;
            if ((rc = launch_gg(ctx, g, s))) return rc;
            g = GG();
            g.batch = B; g.M = N; g.N = D; g.K = N;
            g.A = dC; g.am = 1; g.ak = N + 1; g.az0 = per;
            g.B = t->t_mdesc + (int64_t)i * n_rows * D; g.bk = D; g.bn = 1; g.bz0 = tuple_stride;
            g.C = dmd + (int64_t)j * n_rows * D; g.ldc = D; g.cz0 = tuple_stride; g.alpha = sc; g.mode = 1;
            if ((rc = launch_gg(ctx, g, s))) return rc;
        }
    // ---- confidence heads (pose loss): d conf -> conf_mlp gradients and two more contributions to d mdesc ----
    if (bnb && t->conf_mlp) {  // conf_mlp.1's dgamma / dbeta are summed over the pairs below (zero when no pair has a d conf)
        E2EMV_HIP(ctx, hipMemsetAsync(t->d_graw + t->bns.back().gamma, 0, (size_t)D * sizeof(float), s));
        E2EMV_HIP(ctx, hipMemsetAsync(t->d_graw + t->bns.back().beta, 0, (size_t)D * sizeof(float), s));
    }
    if (d_dconf && t->conf_mlp) {
        int q = 0;
        for (int j = 0; j < T; ++j)
            for (int i = 0; i < j; ++i, ++q) {
                if (!d_dconf[q]) continue;
                if (!t->t_cmatch[q]) return set_err(ctx, E2EMV_ESTATE, "matcher_backward: d conf for pair %d without e2emv_conf_forward_train", q);
                const int64_t rows = (int64_t)B * N;
                float* dz = du;       // [B*N]      (B (N + 1) floats available)
                float* dhc = dcat;    // [B*N][D]
                float* dfeat = dh;    // [B*N][2D]
                hipLaunchKernelGGL(conf_bwd_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, rows, D, (const float*)t->t_chid[q],
                                   W + t->wc1, W + t->bc1, t->t_cmatch[q], d_dconf[q], dz, dhc);
                E2EMV_CHECK_LAUNCH(ctx, "conf_bwd_kernel");
                if ((rc = wgrad(ctx, dz, 1, 1, t->t_chid[q], D, D, rows, gw + t->wc1, D, s))) return rc;
                if ((rc = colsum(ctx, dz, rows, 1, 1, gw + t->bc1, s))) return rc;
                if (bnb) {  // dhc: d hidden (ReLU mask applied) -> d y of conf_mlp.0
                    BnCall a = bn_conf(t, t->t_cy[q], dhc, t->t_cst + (int64_t)q * 3 * D, bpart);
                    a.h = t->t_chid[q];
                    a.accumulate = 1;
                    if ((rc = bn_backward(ctx, a, 1, s))) return rc;
                }
                if ((rc = wgrad(ctx, dhc, D, D, t->t_cfeat[q], 2 * D, 2 * D, rows, gw + t->wc0, 2 * D, s))) return rc;
                if ((rc = colsum(ctx, dhc, rows, D, D, gw + t->bc0, s))) return rc;
                if ((rc = dgrad(ctx, dhc, D, D, W + t->wc0, 2 * D, 2 * D, rows, dfeat, 2 * D, false, s))) return rc;
                hipLaunchKernelGGL(conf_scatter_kernel, dim3((N + 3) / 4, B), dim3(256), 0, s, N, D, (const float*)dfeat, t->t_cmatch[q],
                                   dmd + (int64_t)i * n_rows * D, dmd + (int64_t)j * n_rows * D, tuple_stride, bnb ? 1 : 0);
                E2EMV_CHECK_LAUNCH(ctx, "conf_scatter_kernel");
            }
        E2EMV_HIP(ctx, hipMemsetAsync(du, 0, (size_t)B * (N + 1) * sizeof(float), s));
    }
    // ---- final_proj ----
    if ((rc = wgrad(ctx, dmd, D, D, t->t_x[L], D, D, Mtot, gw + t->wf, D, s))) return rc;
    if ((rc = colsum(ctx, dmd, Mtot, D, D, gw + t->bf, s))) return rc;
    if ((rc = dgrad(ctx, dmd, D, D, W + t->wf, D, D, Mtot, dx, D, false, s))) return rc;
    // ---- GNN layers, last to first; dx = d x_{l+1} on entry, d x_l on exit ----
    for (int l = L - 1; l >= 0; --l) {
        const TrainLayer& Lw = t->layers[l];
        // x_{l+1} = x_l + W1 h + b1
        if ((rc = dgrad(ctx, dx, D, D, W + Lw.w1, 2 * D, 2 * D, Mtot, dh, 2 * D, false, s))) return rc;
        if ((rc = wgrad(ctx, dx, D, D, t->t_h[l], 2 * D, 2 * D, Mtot, gw + Lw.w1, 2 * D, s))) return rc;
        if ((rc = colsum(ctx, dx, Mtot, D, D, gw + Lw.b1, s))) return rc;
        // h = relu(W0 [x_l | msg] + b0)
        if (bnb) {  // h = relu(BN(y)), y = W0 [x_l | msg] + b0 (batch statistics): dh -> dy
            BnCall a = bn_images(t, nk - 1 + l, t->t_hy[l], dh, t->t_hst[l], bpart);
            a.h = t->t_h[l];
            if ((rc = bn_backward(ctx, a, T, s))) return rc;
        } else {
            hipLaunchKernelGGL(relu_bwd_kernel, dim3(ew_grid(Mtot * 2 * D)), dim3(256), 0, s, dh, (const float*)t->t_h[l], Mtot * 2 * D);
        }
        if ((rc = dgrad(ctx, dh, 2 * D, 2 * D, W + Lw.w0, 2 * D, 2 * D, Mtot, dcat, 2 * D, false, s))) return rc;
        if ((rc = wgrad(ctx, dh, 2 * D, 2 * D, t->t_x[l], D, D, Mtot, gw + Lw.w0, 2 * D, s))) return rc;
        if ((rc = wgrad(ctx, dh, 2 * D, 2 * D, t->t_msg[l], D, D, Mtot, gw + Lw.w0 + D, 2 * D, s))) return rc;
        if ((rc = colsum(ctx, dh, Mtot, 2 * D, 2 * D, gw + Lw.b0, s))) return rc;
        hipLaunchKernelGGL(add2d_kernel, dim3(ew_grid(Mtot * D)), dim3(256), 0, s, dx, (int64_t)D, (const float*)dcat, (int64_t)2 * D, Mtot, D);
        // msg = Wm att + bm   (d msg = dcat[:, D:])
        if ((rc = dgrad(ctx, dcat + D, 2 * D, D, W + Lw.wm, D, D, Mtot, datt, D, false, s))) return rc;
        if ((rc = wgrad(ctx, dcat + D, 2 * D, D, t->t_att[l], D, D, Mtot, gw + Lw.wm, D, s))) return rc;
        if ((rc = colsum(ctx, dcat + D, Mtot, D, 2 * D, gw + Lw.bm, s))) return rc;
        // att = attention(q|k|v)
        if ((rc = attention_backward(ctx, B, T, N, n_rows, D, H, Lw.type != 0, t->t_qkv[l], datt, dqkv, Pb, dPb, s))) return rc;
        // q|k|v = Wqkv x_l + b
        if ((rc = dgrad(ctx, dqkv, 3 * D, 3 * D, W + Lw.wqkv, D, D, Mtot, dx, D, true, s))) return rc;
        if ((rc = wgrad(ctx, dqkv, 3 * D, 3 * D, t->t_x[l], D, D, Mtot, gw + Lw.wqkv, D, s))) return rc;
        if ((rc = colsum(ctx, dqkv, Mtot, 3 * D, 3 * D, gw + Lw.bqkv, s))) return rc;
        E2EMV_CHECK_LAUNCH(ctx, "layer backward kernels");
    }
    // ---- keypoint encoder: x_0 = desc + kenc(keypoints); dx = d kenc output ----
    {
        float* cur = dx;  // gradient w.r.t. the output of encoder layer i (width kdims[i + 1])
        float* bufs[2] = {dh, dcat};
        int bi = 0;
        for (int i = nk - 1; i >= 1; --i) {
            const int cin = t->kdims[i], cout = t->kdims[i + 1];
            if (i < nk - 1 && bnb) {
                BnCall a = bn_images(t, i, t->t_ky[i + 1], cur, t->t_kst[i + 1], bpart);
                a.h = t->t_kh[i + 1];
                if ((rc = bn_backward(ctx, a, T, s))) return rc;
            } else if (i < nk - 1) {
                hipLaunchKernelGGL(relu_bwd_kernel, dim3(ew_grid(Mtot * cout)), dim3(256), 0, s, cur, (const float*)t->t_kh[i + 1], Mtot * cout);
            }
            if ((rc = wgrad(ctx, cur, cout, cout, t->t_kh[i], cin, cin, Mtot, gw + t->kw[i], cin, s))) return rc;
            if ((rc = colsum(ctx, cur, Mtot, cout, cout, gw + t->kb[i], s))) return rc;
            if ((rc = dgrad(ctx, cur, cout, cout, W + t->kw[i], cin, cin, Mtot, bufs[bi], cin, false, s))) return rc;
            cur = bufs[bi];
            bi ^= 1;
        }
        // layer 0: 3 -> c0 (+ BN folded, ReLU); its input is re-derived from the keypoints: not kept, the gradient w.r.t. it is not needed
        const int c0 = t->kdims[1];
        if (bnb) {
            BnCall a = bn_images(t, 0, t->t_ky[1], cur, t->t_kst[1], bpart);
            a.h = t->t_kh[1];
            if ((rc = bn_backward(ctx, a, T, s))) return rc;
        } else {
            hipLaunchKernelGGL(relu_bwd_kernel, dim3(ew_grid(Mtot * c0)), dim3(256), 0, s, cur, (const float*)t->t_kh[1], Mtot * c0);
        }
        if ((rc = wgrad(ctx, cur, c0, c0, t->t_inp, 4, 3, Mtot, gw + t->kw[0], 3, s))) return rc;
        if ((rc = colsum(ctx, cur, Mtot, c0, c0, gw + t->kb[0], s))) return rc;
        E2EMV_CHECK_LAUNCH(ctx, "encoder backward kernels");
    }
    // ---- folded gradients -> gradients of the upstream parameters ----
    auto ref = [&](const std::string& k) -> float* { auto it = t->raw.find(k); return it == t->raw.end() ? nullptr : t->d_raw + it->second.off; };
    auto gref = [&](const std::string& k) -> float* { auto it = t->raw.find(k); return it == t->raw.end() ? nullptr : t->d_graw + it->second.off; };
    auto unfold = [&](const std::string& conv, const std::string& bn, const float* dWf, const float* dbf, int64_t ldwf, int col0, int rows, int cols, const int* rmap,
                      int rbase, const int* cmap) {
        UnfoldArgs a{};
        a.dWf = dWf + (int64_t)rbase * ldwf; a.dbf = dbf + rbase; a.ldwf = ldwf; a.col0 = col0;
        a.W = ref(conv + ".weight"); a.b = ref(conv + ".bias");
        if (!bn.empty() && ref(bn + ".running_mean") && t->bn_mode == E2EMV_BN_FROZEN) {  // (batch statistics: dgamma / dbeta come from bn_backward)
            a.gamma = ref(bn + ".weight"); a.beta = ref(bn + ".bias"); a.mean = ref(bn + ".running_mean"); a.var = ref(bn + ".running_var");
            a.dgamma = gref(bn + ".weight"); a.dbeta = gref(bn + ".bias");
        }
        a.rmap = rmap; a.cmap = cmap; a.rows = rows; a.cols = cols;
        a.dW = gref(conv + ".weight"); a.db = gref(conv + ".bias");
        hipLaunchKernelGGL(unfold_kernel, dim3(rows), dim3(256), 0, s, a);
    };
    for (int i = 0; i < nk; ++i)
        unfold("kenc.encoder." + std::to_string(3 * i), i < nk - 1 ? "kenc.encoder." + std::to_string(3 * i + 1) : std::string(), gw + t->kw[i], gw + t->kb[i], t->kdims[i],
               0, t->kdims[i + 1], t->kdims[i], nullptr, 0, nullptr);
    for (int l = 0; l < L; ++l) {
        const TrainLayer& Lw = t->layers[l];
        const std::string base = "gnn.layers." + std::to_string(l);
        for (int p = 0; p < 3; ++p) unfold(base + ".attn.proj." + std::to_string(p), "", gw + Lw.wqkv, gw + Lw.bqkv, D, 0, D, D, t->d_maps, p * D, nullptr);
        unfold(base + ".attn.merge", "", gw + Lw.wm, gw + Lw.bm, D, 0, D, D, nullptr, 0, t->d_maps);
        unfold(base + ".mlp.0", base + ".mlp.1", gw + Lw.w0, gw + Lw.b0, 2 * D, 0, 2 * D, 2 * D, nullptr, 0, nullptr);
        unfold(base + ".mlp.3", "", gw + Lw.w1, gw + Lw.b1, 2 * D, 0, D, 2 * D, nullptr, 0, nullptr);
    }
    unfold("final_proj", "", gw + t->wf, gw + t->bf, D, 0, D, D, nullptr, 0, nullptr);
    if (t->conf_mlp) {
        unfold("conf_mlp.0", "conf_mlp.1", gw + t->wc0, gw + t->bc0, 2 * D, 0, D, 2 * D, nullptr, 0, nullptr);
        unfold("conf_mlp.3", "", gw + t->wc1, gw + t->bc1, D, 0, 1, D, nullptr, 0, nullptr);
    }
    E2EMV_HIP(ctx, hipMemcpyAsync(gref("bin_score"), gw + t->alpha, sizeof(float), hipMemcpyDeviceToDevice, s));
    E2EMV_CHECK_LAUNCH(ctx, "unfold kernels");
    return E2EMV_OK;
}

extern "C" int e2emv_get_grad(e2emv_ctx* ctx, const char* key, float* d_dst, int64_t numel, void* stream) {
    if (!ctx || !key || !d_dst) return E2EMV_EINVAL;
    E2EMV_ENTER(ctx, stream);
    TrainState* t = ts_of(ctx);
    if (!t) return set_err(ctx, E2EMV_ESTATE, "get_grad: e2emv_train_commit first");
    std::string k(key);
    if (k.rfind("module.", 0) == 0) k = k.substr(7);
    auto it = t->raw.find(k);
    if (it == t->raw.end()) return set_err(ctx, E2EMV_EINVAL, "get_grad: no gradient for '%s'", key);
    if ((int64_t)it->second.numel != numel) return set_err(ctx, E2EMV_ESHAPE, "get_grad: '%s' has %zu elements, not %lld", key, it->second.numel, (long long)numel);
    E2EMV_HIP(ctx, hipMemcpyAsync(d_dst, t->d_graw + it->second.off, numel * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return E2EMV_OK;
}

extern "C" int e2emv_train_set_batchnorm(e2emv_ctx* ctx, int mode, float momentum) {
    if (!ctx) return E2EMV_EINVAL;
    if (mode != E2EMV_BN_FROZEN && mode != E2EMV_BN_BATCH) return set_err(ctx, E2EMV_EINVAL, "train_set_batchnorm: mode %d", mode);
    if (!(momentum >= 0.f && momentum <= 1.f)) return set_err(ctx, E2EMV_EINVAL, "train_set_batchnorm: momentum %g outside [0, 1]", (double)momentum);
    E2EMV_LOCK(ctx);
    ctx->train_bn_mode = mode;
    ctx->train_bn_momentum = momentum;
    return E2EMV_OK;
}

// torch's running-buffer update for the BatchNorm calls of the last forward_train (T per encoder / GNN BatchNorm, image order)
// and of its conf forwards (one per pair that ran, pair order) - onto the caller's device buffers, stream-ordered
extern "C" int e2emv_train_running_update(e2emv_ctx* ctx, int n, const char* const* keys, float* const* d_running_mean, float* const* d_running_var,
                                          void* stream) {
    if (!ctx || n < 0 || (n && (!keys || !d_running_mean || !d_running_var))) return E2EMV_EINVAL;
    E2EMV_ENTER(ctx, stream);
    TrainState* t = ts_of(ctx);
    if (!t || !t->have_tape) return set_err(ctx, E2EMV_ESTATE, "train_running_update: no tape - e2emv_matcher_forward_train first");
    if (t->bn_mode != E2EMV_BN_BATCH) return set_err(ctx, E2EMV_ESTATE, "train_running_update: the tape was made with frozen BatchNorm statistics");
    std::vector<int> which(n);
    for (int i = 0; i < n; ++i) {  // (all entries checked before the first launch)
        if (!keys[i] || !d_running_mean[i] || !d_running_var[i]) return set_err(ctx, E2EMV_EINVAL, "train_running_update: null entry %d", i);
        std::string k(keys[i]);
        if (k.rfind("module.", 0) == 0) k = k.substr(7);
        which[i] = -1;
        for (size_t j = 0; j < t->bns.size(); ++j)
            if (t->bns[j].name == k) which[i] = (int)j;
        if (which[i] < 0) return set_err(ctx, E2EMV_EINVAL, "train_running_update: no BatchNorm '%s' in the committed model", keys[i]);
    }
    hipStream_t s = (hipStream_t)stream;
    const int nk = (int)t->kdims.size() - 1, L = (int)t->layers.size();
    const int64_t cnt = (int64_t)t->B * t->N;
    const double unbias = (double)cnt / (double)(cnt - 1);
    const float m = ctx->train_bn_momentum;
    for (int i = 0; i < n; ++i) {
        const int j = which[i], C = t->bns[j].C;
        const dim3 grid((C + 255) / 256);
        if (j < nk - 1 + L) {
            const float* st = j < nk - 1 ? t->t_kst[j + 1] : t->t_hst[j - (nk - 1)];
            hipLaunchKernelGGL(bn_running_kernel, grid, dim3(256), 0, s, C, t->T, st, m, unbias, d_running_mean[i], d_running_var[i]);
        } else {
            for (int q = 0; q < t->P; ++q)
                if (t->t_cmatch[q])
                    hipLaunchKernelGGL(bn_running_kernel, grid, dim3(256), 0, s, C, 1, (const float*)t->t_cst + (int64_t)q * 3 * C, m, unbias,
                                       d_running_mean[i], d_running_var[i]);
        }
    }
    E2EMV_CHECK_LAUNCH(ctx, "bn_running_kernel");
    return E2EMV_OK;
}

// ---- building blocks of the training path: one stage each, through the functions the forward / backward above call ----------
// They need no committed model and no tape; their scratch is the context's workspace, a tape in the context is left alone.

// y = x W^T + b over `rows` rows: wgrad, colsum and dgrad as e2emv_matcher_backward calls them for a dense layer
extern "C" int e2emv_train_linear_backward(e2emv_ctx* ctx, int64_t rows, int n_out, int n_in, const float* d_dY, int64_t ldy, const float* d_X, int64_t ldx,
                                           const float* d_W, int64_t ldw, float* d_dW, float* d_db, float* d_dX, int accumulate, void* stream) {
    if (!ctx || !d_dY || !d_X || !d_W || !d_dW || !d_db) return E2EMV_EINVAL;
    E2EMV_ENTER(ctx, stream);
    if (rows < 1 || rows > (int64_t)64 * 65535 || n_out < 1 || n_in < 1 || n_out > 65535 * 64 || n_in > 65535 * 64)
        return set_err(ctx, E2EMV_ESHAPE, "train_linear_backward: rows=%lld n_out=%d n_in=%d", (long long)rows, n_out, n_in);
    if (ldy < n_out || ldx < n_in || ldw < n_in)
        return set_err(ctx, E2EMV_ESHAPE, "train_linear_backward: a row stride is shorter than its row (ldy=%lld ldx=%lld ldw=%lld)", (long long)ldy,
                       (long long)ldx, (long long)ldw);
    (void)hipSetDevice(ctx->device);
    hipStream_t s = (hipStream_t)stream;
    int rc;
    if ((rc = wgrad(ctx, d_dY, ldy, n_out, d_X, ldx, n_in, rows, d_dW, ldw, s))) return rc;
    if ((rc = colsum(ctx, d_dY, rows, n_out, ldy, d_db, s))) return rc;
    if (d_dX && (rc = dgrad(ctx, d_dY, ldy, n_out, d_W, ldw, n_in, rows, d_dX, ldx, accumulate != 0, s))) return rc;
    return E2EMV_OK;
}

// the unrolled Sinkhorn of B problems of N x N scores with its tape, and (d_G given) the reverse sweep over that tape
extern "C" int e2emv_train_sinkhorn(e2emv_ctx* ctx, int B, int N, const float* d_S, int64_t ldS, float alpha, int iters, int col_width, const float* d_G,
                                    float* d_logZ, float* d_uv, float* d_dC, float* d_dalpha, void* stream) {
    if (!ctx || !d_S || !d_logZ || (d_G && (!d_dC || !d_dalpha))) return E2EMV_EINVAL;
    E2EMV_ENTER(ctx, stream);
    if (B < 1 || B > 65535 || N < 1 || N > 2048 || ldS < N) return set_err(ctx, E2EMV_ESHAPE, "train_sinkhorn: B=%d N=%d ldS=%lld", B, N, (long long)ldS);
    if (iters < 0) return set_err(ctx, E2EMV_EINVAL, "negative sinkhorn_iters");
    if (col_width != 0 && col_width != 32 && col_width != 64) return set_err(ctx, E2EMV_EINVAL, "train_sinkhorn: col_width %d (0, 32 or 64)", col_width);
    (void)hipSetDevice(ctx->device);
    hipStream_t s = (hipStream_t)stream;
    const size_t sz_uv = al256((size_t)B * (iters + 1) * 2 * (N + 1) * 4), sz_v = al256((size_t)B * (N + 1) * 4);
    int rc = ws_reserve(ctx, sz_uv + 3 * sz_v);
    if (rc) return rc;
    char* w = ctx->d_ws;
    auto take = [&](size_t bytes) { float* p = (float*)w; w += bytes; return p; };
    float* uv = take(sz_uv);
    float* du = take(sz_v);
    float* dv = take(sz_v);
    float* dv2 = take(sz_v);
    E2EMV_HIP(ctx, hipMemsetAsync(uv, 0, sz_uv, s));  // (u_0 = v_0 = 0, as on the zeroed tape)
    const SkT sk = sk_problem(d_S, ldS, N, alpha);
    if ((rc = sinkhorn_tape_forward(ctx, sk, B, iters, uv, d_logZ, col_width, s))) return rc;
    if (d_uv) E2EMV_HIP(ctx, hipMemcpyAsync(d_uv, uv, (size_t)B * (iters + 1) * 2 * (N + 1) * sizeof(float), hipMemcpyDeviceToDevice, s));
    if (!d_G) return E2EMV_OK;
    E2EMV_HIP(ctx, hipMemsetAsync(d_dalpha, 0, sizeof(float), s));
    return sinkhorn_tape_backward(ctx, sk, B, iters, uv, d_G, d_dC, du, dv, dv2, d_dalpha, col_width, s);
}

// attention backward of one layer on q|k|v and d att of the tape's layout (n_rows = N rounded up to 128 rows per image)
extern "C" int e2emv_train_attention_backward(e2emv_ctx* ctx, int B, int T, int N, int D, int H, int cross, const float* d_qkv, const float* d_datt,
                                              float* d_dqkv, void* stream) {
    if (!ctx || !d_qkv || !d_datt || !d_dqkv) return E2EMV_EINVAL;
    E2EMV_ENTER(ctx, stream);
    if (D <= 0 || H <= 0 || D != H * 64) return set_err(ctx, E2EMV_ESHAPE, "train_attention_backward: head dim must be 64 (D=%d H=%d)", D, H);
    if (B < 1 || (int64_t)B * H > 65535 || T < 2 || T > E2EMV_MAX_TUPLE || N < 1 || N > 2048)
        return set_err(ctx, E2EMV_ESHAPE, "train_attention_backward: batch=%d tuple_size=%d n_kpts=%d", B, T, N);
    (void)hipSetDevice(ctx->device);
    hipStream_t s = (hipStream_t)stream;
    const int n_rows = (N + 127) / 128 * 128, n_src = cross ? T - 1 : 1;
    const size_t sz_P = al256((size_t)B * H * N * n_src * N * 4);
    int rc = ws_reserve(ctx, 2 * sz_P);
    if (rc) return rc;
    float* Pb = (float*)ctx->d_ws;
    float* dPb = (float*)(ctx->d_ws + sz_P);
    return attention_backward(ctx, B, T, N, n_rows, D, H, cross != 0, d_qkv, d_datt, d_dqkv, Pb, dPb, s);
}
