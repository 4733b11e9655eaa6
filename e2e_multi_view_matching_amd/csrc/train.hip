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

// A dense layer of the folded arena: weight [out][in] and bias [out] at these offsets (floats) of d_w, their gradients at the
// same offsets of d_gw
struct TrainDense { size_t w, b; int out, in; };

struct TrainLayer {
    TrainDense qkv, merge, mlp0, mlp1;  // q|k|v [3D][D] head-major rows, merge [D][D] head-major columns, MLP0 [2D][2D] BN folded,
    int type;                           // MLP1 [D][2D]
};

struct RawRef { size_t off, numel; };

struct TrainState {
    e2emv_model_desc model{};
    // folded weights and their gradients (same offsets)
    float* d_w = nullptr;
    float* d_gw = nullptr;
    size_t w_floats = 0;
    std::vector<TrainDense> kenc;  // keypoint encoder layers 0..n (BN folded)
    std::vector<int> kdims;        // [3, c0, ..., D]
    std::vector<TrainLayer> layers;
    TrainDense final_proj{};
    TrainDense conf0{}, conf1{};  // conf_mlp.0 (+ BN conf_mlp.1) [D][2D], conf_mlp.3 [1][D]
    size_t alpha = 0;
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

// The weight side of a forward GEMM over `rows` rows with the dense layer d, one K segment
static GemmArgs dense_gemm(const TrainState* t, const TrainDense& d, int64_t rows) {
    GemmArgs g;
    g.M = (int)rows; g.N = d.out; g.K = d.in; g.K1 = d.in; g.W = t->d_w + d.w; g.ldw = d.in; g.bias = t->d_w + d.b;
    return g;
}
// Backward of y = x W^T + b over `rows` rows, W [n_out][n_in] (row stride ldw): dW += dY^T X, db += the column sums of dY and, with
// a dX, dX (+)= dY W - three launches, none reads what another writes.  X2: the input is [X | X2] in two buffers of n_in / 2 columns
// each (MLP0's [x | msg]); the weight gradient is then two wgrad calls, the second at column n_in / 2 of dW.
static int linear_backward(e2emv_ctx* ctx, const float* W, float* dW, int64_t ldw, float* db, int n_out, int n_in, int64_t rows, const float* dY, int64_t ldy,
                           const float* X, int64_t ldx, const float* X2, int64_t ldx2, float* dX, int64_t ldx_out, bool accumulate, hipStream_t s) {
    const int k1 = X2 ? n_in / 2 : n_in;
    int rc;
    if ((rc = wgrad(ctx, dY, ldy, n_out, X, ldx, k1, rows, dW, ldw, s))) return rc;
    if (X2 && (rc = wgrad(ctx, dY, ldy, n_out, X2, ldx2, n_in - k1, rows, dW + k1, ldw, s))) return rc;
    if ((rc = colsum(ctx, dY, rows, n_out, ldy, db, s))) return rc;
    if (dX && (rc = dgrad(ctx, dY, ldy, n_out, W, ldw, n_in, rows, dX, ldx_out, accumulate, s))) return rc;
    return E2EMV_OK;
}
// ... of the dense layer d of the folded arena, its gradients into d_gw
static int dense_backward(e2emv_ctx* ctx, const TrainState* t, const TrainDense& d, int64_t rows, const float* dY, int64_t ldy, const float* X, int64_t ldx,
                          float* dX, int64_t ldx_out, bool accumulate, hipStream_t s, const float* X2 = nullptr, int64_t ldx2 = 0) {
    return linear_backward(ctx, t->d_w + d.w, t->d_gw + d.w, d.in, t->d_gw + d.b, d.out, d.in, rows, dY, ldy, X, ldx, X2, ldx2, dX, ldx_out, accumulate, s);
}

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
// Backward of the activation behind a layer of C channels over the T images, g [Mtot][C]: d h on entry, d y on exit.  Batch
// statistics: h = relu(BN_j(y)) with the tape's y and statistics (dgamma / dbeta of BN j written); frozen: h = relu(y), the
// BatchNorm is folded into the layer
static int activation_backward(e2emv_ctx* ctx, const TrainState* t, int j, int C, float* y, float* stats, const float* h, float* g, double* bpart, hipStream_t s) {
    if (t->bn_mode == E2EMV_BN_BATCH) {
        BnCall a = bn_images(t, j, y, g, stats, bpart);
        a.h = h;
        return bn_backward(ctx, a, t->T, s);
    }
    hipLaunchKernelGGL(relu_bwd_kernel, dim3(ew_grid(t->Mtot * C)), dim3(256), 0, s, g, h, t->Mtot * C);
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
        t->kenc.push_back({pk.add(w), pk.add(b), t->kdims[i + 1], t->kdims[i]});
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
        L.qkv = {pk.add(wqkv), pk.add(bqkv), 3 * D, D};
        if ((rc = conv_bn(ctx, t, raw, base + ".attn.merge", "", D, D, w, b))) return rc;
        std::vector<float> wm((size_t)D * D);
        for (int o = 0; o < D; ++o)
            for (int h = 0; h < H; ++h)
                for (int dd = 0; dd < d; ++dd) wm[(size_t)o * D + h * d + dd] = w[(size_t)o * D + dd * H + h];
        L.merge = {pk.add(wm), pk.add(b), D, D};
        if ((rc = conv_bn(ctx, t, raw, base + ".mlp.0", base + ".mlp.1", 2 * D, 2 * D, w, b))) return rc;
        L.mlp0 = {pk.add(w), pk.add(b), 2 * D, 2 * D};
        if ((rc = conv_bn(ctx, t, raw, base + ".mlp.3", "", D, 2 * D, w, b))) return rc;
        L.mlp1 = {pk.add(w), pk.add(b), D, 2 * D};
    }
    if ((rc = conv_bn(ctx, t, raw, "final_proj", "", D, D, w, b))) return rc;
    t->final_proj = {pk.add(w), pk.add(b), D, D};
    t->conf_mlp = m->conf_mlp != 0;
    if (t->conf_mlp) {
        if ((rc = conv_bn(ctx, t, raw, "conf_mlp.0", "conf_mlp.1", D, 2 * D, w, b))) return rc;
        t->conf0 = {pk.add(w), pk.add(b), D, 2 * D};
        if ((rc = conv_bn(ctx, t, raw, "conf_mlp.3", "", 1, D, w, b))) return rc;
        t->conf1 = {pk.add(w), pk.add(b), 1, D};
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

// Every upstream convolution of the model, in the order the fold (e2emv_train_update) and the un-fold (unfold_grads) launch them:
// fn(conv, bn, d, rows, rbase, rmap, cmap) - the convolution, the BatchNorm behind it ("" = none), the dense layer of the folded
// arena that holds its `rows` output channels from row rbase on, the head-order maps of its rows / columns (null = upstream order)
template <class F>
static void for_each_folded(const TrainState* t, F&& fn) {
    const int nk = (int)t->kenc.size(), D = t->model.desc_dim;
    for (int i = 0; i < nk; ++i)
        fn("kenc.encoder." + std::to_string(3 * i), i < nk - 1 ? "kenc.encoder." + std::to_string(3 * i + 1) : std::string(), t->kenc[i], t->kenc[i].out, 0, nullptr, nullptr);
    for (size_t l = 0; l < t->layers.size(); ++l) {
        const TrainLayer& Lw = t->layers[l];
        const std::string base = "gnn.layers." + std::to_string(l);
        for (int p = 0; p < 3; ++p) fn(base + ".attn.proj." + std::to_string(p), "", Lw.qkv, D, p * D, t->d_maps, nullptr);
        fn(base + ".attn.merge", "", Lw.merge, D, 0, nullptr, t->d_maps);
        fn(base + ".mlp.0", base + ".mlp.1", Lw.mlp0, 2 * D, 0, nullptr, nullptr);
        fn(base + ".mlp.3", "", Lw.mlp1, D, 0, nullptr, nullptr);
    }
    fn("final_proj", "", t->final_proj, D, 0, nullptr, nullptr);
    if (t->conf_mlp) {
        fn("conf_mlp.0", "conf_mlp.1", t->conf0, D, 0, nullptr, nullptr);
        fn("conf_mlp.3", "", t->conf1, 1, 0, nullptr, nullptr);
    }
}

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
    float* W = t->d_w;
    auto ref = [&](const std::string& k) -> const float* { auto it = t->raw.find(k); return it == t->raw.end() ? nullptr : t->d_raw + it->second.off; };
    for_each_folded(t, [&](const std::string& conv, const std::string& bn, const TrainDense& d, int rows, int rbase, const int* rmap, const int* cmap) {
        FoldArgs a{};
        a.W = ref(conv + ".weight"); a.b = ref(conv + ".bias");
        if (!bn.empty() && ref(bn + ".running_mean") && t->bn_mode == E2EMV_BN_FROZEN) { a.gamma = ref(bn + ".weight"); a.beta = ref(bn + ".bias"); a.mean = ref(bn + ".running_mean"); a.var = ref(bn + ".running_var"); }
        a.Wf = W + d.w + (int64_t)rbase * d.in; a.bf = W + d.b + rbase; a.ldwf = d.in; a.col0 = 0; a.rows = rows; a.cols = d.in; a.rmap = rmap; a.cmap = cmap;
        hipLaunchKernelGGL(fold_kernel, dim3(rows), dim3(256), 0, s, a);
    });
    E2EMV_CHECK_LAUNCH(ctx, "fold kernels");
    E2EMV_HIP(ctx, hipMemcpyAsync(W + t->alpha, ref("bin_score"), sizeof(float), hipMemcpyDeviceToDevice, s));
    t->bin_score = bin_score;
    E2EMV_HIP(ctx, hipMemsetAsync(t->d_graw, 0, t->raw_floats * sizeof(float), s));
    t->have_tape = false;
    return E2EMV_OK;
}

// ---- the forward with a tape, in stages --------------------------------------------------------------------------------------
// what e2emv_matcher_forward_train refuses before it touches the tape
static int check_train_inputs(e2emv_ctx* ctx, const TrainState* t, const e2emv_forward_desc* fd) {
    const int B = fd->batch, T = fd->tuple_size, N = fd->n_kpts;
    if (B <= 0 || T < 2 || T > E2EMV_MAX_TUPLE || N <= 0 || N > 2048) return set_err(ctx, E2EMV_ESHAPE, "matcher_forward_train: batch=%d tuple_size=%d n_kpts=%d", B, T, N);
    if (T > 2 && !(fd->flags & E2EMV_FLAG_MULTI_FRAME)) return set_err(ctx, E2EMV_ESHAPE, "matcher_forward_train: tuples of more than 2 images need multi_frame_matching");
    for (int i = 0; i < T; ++i)
        if (fd->n_kpts_img[i] > 0 && fd->n_kpts_img[i] != N) return set_err(ctx, E2EMV_ESHAPE, "matcher_forward_train: all images of a call carry the same number of keypoints");
    if (fd->sinkhorn_iters < 0) return set_err(ctx, E2EMV_EINVAL, "negative sinkhorn_iters");
    if (t->bn_mode != ctx->train_bn_mode)
        return set_err(ctx, E2EMV_ESTATE, "matcher_forward_train: the BatchNorm mode changed since e2emv_train_commit (commit again)");
    if (t->bn_mode == E2EMV_BN_BATCH && (int64_t)B * N < 2) return set_err(ctx, E2EMV_ESHAPE, "matcher_forward_train: batch statistics need more than one value per channel");
    return E2EMV_OK;
}

// The tape of a forward of B tuples of T images, N keypoints each, `iters` Sinkhorn iterations: its regions in order, each on a
// 256-byte boundary.  Returns the byte count.  base == nullptr: the count only, *t is left as it is; with a base the shape and
// every t_* pointer of *t are set (t_cmatch: reset - no conf head has run on this tape).
static size_t carve_tape(TrainState* t, char* base, int B, int T, int N, int iters) {
    TrainState sizes_only;
    TrainState* o = base ? t : &sizes_only;
    const int D = t->model.desc_dim, L = (int)t->layers.size(), nk = (int)t->kenc.size();
    const int n_rows = (N + 127) / 128 * 128, P = T * (T - 1) / 2, ldS = (N + 3) / 4 * 4;
    const size_t Mtot = (size_t)B * T * n_rows, BN = (size_t)B * N;
    const bool bnb = t->bn_mode == E2EMV_BN_BATCH;
    size_t off = 0;
    auto take = [&](size_t bytes) { float* p = base ? (float*)(base + off) : nullptr; off += al256(bytes); return p; };
    for (auto* v : {&o->t_kh, &o->t_ky, &o->t_kst}) v->assign(nk, nullptr);  // (a slot without a region stays null)
    for (auto* v : {&o->t_qkv, &o->t_att, &o->t_msg, &o->t_h, &o->t_hy, &o->t_hst}) v->assign(L, nullptr);
    for (auto* v : {&o->t_cfeat, &o->t_chid, &o->t_cy}) v->assign(P, nullptr);
    o->t_x.assign(L + 1, nullptr); o->t_cmatch.assign(P, nullptr); o->t_cst = nullptr; o->t_part = nullptr;
    o->t_inp = take(Mtot * 4 * 4);
    for (int i = 1; i < nk; ++i) o->t_kh[i] = take(Mtot * t->kdims[i] * 4);  // t_kh[i]: output of encoder layer i - 1 (width kdims[i])
    for (int l = 0; l <= L; ++l) o->t_x[l] = take(Mtot * D * 4);
    for (int l = 0; l < L; ++l) { o->t_qkv[l] = take(Mtot * 3 * D * 4); o->t_att[l] = take(Mtot * D * 4); o->t_msg[l] = take(Mtot * D * 4); o->t_h[l] = take(Mtot * 2 * D * 4); }
    o->t_mdesc = take(Mtot * D * 4);
    o->t_S = take((size_t)P * BN * ldS * 4);
    o->t_uv = take((size_t)P * B * (iters + 1) * 2 * (N + 1) * 4);
    if (t->conf_mlp)
        for (int q = 0; q < P; ++q) { o->t_cfeat[q] = take(BN * 2 * D * 4); o->t_chid[q] = take(BN * D * 4); }
    if (bnb) {  // y and the statistics of every BatchNorm, the partial sums
        for (int j = 1; j < nk; ++j) { o->t_ky[j] = take(Mtot * t->kdims[j] * 4); o->t_kst[j] = take((size_t)T * 3 * t->kdims[j] * 4); }
        for (int l = 0; l < L; ++l) { o->t_hy[l] = take(Mtot * 2 * D * 4); o->t_hst[l] = take((size_t)T * 3 * 2 * D * 4); }
        if (t->conf_mlp) {
            for (int q = 0; q < P; ++q) o->t_cy[q] = take(BN * D * 4);
            o->t_cst = take((size_t)P * 3 * D * 4);
        }
        o->t_part = (double*)take((size_t)T * BN_MAX_CHUNKS * 2 * 2 * D * 8);
    }
    o->B = B; o->T = T; o->N = N; o->n_rows = n_rows; o->iters = iters; o->P = P; o->ldS = ldS; o->Mtot = (int64_t)Mtot;
    return off;
}

// ingest (descriptors -> the desc part of x_0, keypoints -> encoder layer 0) and the keypoint encoder: x_0 = desc + kenc
static int encode_train(e2emv_ctx* ctx, TrainState* t, const e2emv_forward_desc* fd, const float* const* d_kpts, const float* const* d_kscores,
                        const void* const* d_desc, hipStream_t s) {
    const int B = t->B, T = t->T, N = t->N, n_rows = t->n_rows, D = t->model.desc_dim, nk = (int)t->kenc.size();
    const int64_t Mtot = t->Mtot;
    const bool bnb = t->bn_mode == E2EMV_BN_BATCH;
    const float *w0 = t->d_w + t->kenc[0].w, *b0 = t->d_w + t->kenc[0].b;  // layer 0 (3 -> c0) runs inside the ingest
    const int c0 = t->kenc[0].out;
    IngestParams ip{};
    for (int i = 0; i < T; ++i) {
        if (!d_kpts[i] || !d_kscores[i] || !d_desc[i]) return set_err(ctx, E2EMV_EINVAL, "matcher_forward_train: null input for image %d", i);
        ip.kpts[i] = d_kpts[i]; ip.ksc[i] = d_kscores[i]; ip.desc[i] = d_desc[i];
        ip.img_w[i] = fd->img_w[i]; ip.img_h[i] = fd->img_h[i]; ip.Nimg[i] = N;
    }
    ip.B = B; ip.T = T; ip.n_rows = n_rows; ip.D = D; ip.c0 = c0; ip.f16 = fd->desc_dtype == E2EMV_DESC_F16;
    ip.w0 = w0; ip.b0 = b0; ip.x0 = t->t_x[0]; ip.h0 = t->t_kh[1]; ip.inp = t->t_inp;
    hipLaunchKernelGGL(ingest_transpose, dim3(n_rows / 64, D / 64, B * T), dim3(256), 0, s, ip);
    hipLaunchKernelGGL(ingest_kenc0, dim3((n_rows + 255) / 256, B * T), dim3(256), 0, s, ip);
    E2EMV_CHECK_LAUNCH(ctx, "ingest kernels");
    int rc;
    if (bnb) {  // layer 0 again, without the BatchNorm ingest_kenc0 fuses: y, then the batch-statistics BN + ReLU over t_kh[1]
        hipLaunchKernelGGL(kenc0_conv_kernel, dim3(ew_grid(Mtot * c0)), dim3(256), 0, s, (const float*)t->t_inp, w0, b0, c0, Mtot, t->t_ky[1]);
        E2EMV_CHECK_LAUNCH(ctx, "kenc0_conv_kernel");
        if ((rc = bn_forward(ctx, bn_images(t, 0, t->t_ky[1], t->t_kh[1], t->t_kst[1], t->t_part), T, s))) return rc;
    }
    // encoder layers 1 .. nk-1; the last adds the descriptors (x_0 = desc + kenc)
    for (int i = 1; i < nk; ++i) {
        const TrainDense& d = t->kenc[i];
        const bool last = i == nk - 1;
        GemmArgs g = dense_gemm(t, d, Mtot);
        g.A = t->t_kh[i]; g.lda = d.in; g.relu = !last && !bnb;
        if (last) { g.R = t->t_x[0]; g.ldr = D; g.C = t->t_x[0]; g.ldc = D; }
        else { g.C = bnb ? t->t_ky[i + 1] : t->t_kh[i + 1]; g.ldc = d.out; }
        if ((rc = launch_gemm_nt(ctx, g, s))) return rc;
        if (bnb && !last && (rc = bn_forward(ctx, bn_images(t, i, t->t_ky[i + 1], t->t_kh[i + 1], t->t_kst[i + 1], t->t_part), T, s))) return rc;
    }
    return E2EMV_OK;
}

// attentional GNN: x_l -> x_{l+1}, every intermediate on the tape (merge NOT folded: its parameters get their own gradients)
static int gnn_train(e2emv_ctx* ctx, TrainState* t, hipStream_t s) {
    const int D = t->model.desc_dim, L = (int)t->layers.size(), nk = (int)t->kenc.size();
    const int64_t Mtot = t->Mtot;
    const bool bnb = t->bn_mode == E2EMV_BN_BATCH;
    int Nt[E2EMV_MAX_TUPLE] = {0};
    for (int i = 0; i < t->T; ++i) Nt[i] = t->N;
    int rc;
    for (int l = 0; l < L; ++l) {
        const TrainLayer& Lw = t->layers[l];
        GemmArgs g = dense_gemm(t, Lw.qkv, Mtot);
        g.A = t->t_x[l]; g.lda = D; g.C = t->t_qkv[l]; g.ldc = 3 * D;
        if ((rc = launch_gemm_nt(ctx, g, s))) return rc;
        if ((rc = launch_attention(ctx, t->B, t->T, t->n_rows, Nt, D, t->model.num_heads, t->t_qkv[l], Lw.type, t->t_att[l], s))) return rc;
        g = dense_gemm(t, Lw.merge, Mtot);
        g.A = t->t_att[l]; g.lda = D; g.C = t->t_msg[l]; g.ldc = D;
        if ((rc = launch_gemm_nt(ctx, g, s))) return rc;
        g = dense_gemm(t, Lw.mlp0, Mtot);  // two K segments: [x_l | msg]
        g.K1 = D; g.A = t->t_x[l]; g.lda = D; g.A2 = t->t_msg[l]; g.lda2 = D;
        g.relu = !bnb; g.C = bnb ? t->t_hy[l] : t->t_h[l]; g.ldc = 2 * D;
        if ((rc = launch_gemm_nt(ctx, g, s))) return rc;
        if (bnb && (rc = bn_forward(ctx, bn_images(t, nk - 1 + l, t->t_hy[l], t->t_h[l], t->t_hst[l], t->t_part), t->T, s))) return rc;
        g = dense_gemm(t, Lw.mlp1, Mtot);
        g.A = t->t_h[l]; g.lda = 2 * D; g.R = t->t_x[l]; g.ldr = D; g.C = t->t_x[l + 1]; g.ldc = D;
        if ((rc = launch_gemm_nt(ctx, g, s))) return rc;
    }
    return E2EMV_OK;
}

// final_proj, then per pair: scores, Sinkhorn (log domain, u_t / v_t of every iteration kept), log assignment into d_logZ
static int scores_train(e2emv_ctx* ctx, TrainState* t, float* const* d_logZ, hipStream_t s) {
    const int B = t->B, N = t->N, n_rows = t->n_rows, ldS = t->ldS, D = t->model.desc_dim;
    int rc;
    GemmArgs f = dense_gemm(t, t->final_proj, t->Mtot);
    f.A = t->t_x.back(); f.lda = D; f.C = t->t_mdesc; f.ldc = D;
    if ((rc = launch_gemm_nt(ctx, f, s))) return rc;
    const int64_t tuple_stride = (int64_t)t->T * n_rows * D;
    SkT sk = sk_problem(nullptr, ldS, N, t->bin_score);
    const int64_t uvs = (int64_t)(t->iters + 1) * 2 * (N + 1);  // per problem
    for (int q = 0; q < t->P; ++q) {
        const TuplePair pr = tuple_pair(q);
        float* S = t->t_S + (int64_t)q * B * N * ldS;
        GemmArgs g;
        g.batch = B; g.M = N; g.N = N; g.K = D; g.K1 = D;
        g.A = t->t_mdesc + (int64_t)pr.i * n_rows * D; g.lda = D; g.sA = tuple_stride;
        g.W = t->t_mdesc + (int64_t)pr.j * n_rows * D; g.ldw = D; g.sW = tuple_stride;
        g.C = S; g.ldc = ldS; g.sC = (int64_t)N * ldS; g.scale = 1.0f / sqrtf((float)D);
        if ((rc = launch_gemm_nt(ctx, g, s))) return rc;
        sk.S = S;
        float* uv = t->t_uv + (int64_t)q * B * uvs;  // [b][t][{u, v}][N + 1]
        if (!d_logZ[q]) return set_err(ctx, E2EMV_EINVAL, "matcher_forward_train: null logZ for pair %d", q);
        if ((rc = sinkhorn_tape_forward(ctx, sk, B, t->iters, uv, d_logZ[q], 0, s))) return rc;
    }
    return E2EMV_OK;
}

extern "C" int e2emv_matcher_forward_train(e2emv_ctx* ctx, const e2emv_forward_desc* fd, const float* const* d_kpts, const float* const* d_kscores,
                                           const void* const* d_desc, float* const* d_logZ, void* stream) {
    if (!ctx || !fd || !d_kpts || !d_kscores || !d_desc || !d_logZ) return E2EMV_EINVAL;
    E2EMV_ENTER(ctx, stream);
    TrainState* t = ts_of(ctx);
    if (!t) return set_err(ctx, E2EMV_ESTATE, "matcher_forward_train: e2emv_train_commit first");
    if (int rc = check_train_inputs(ctx, t, fd)) return rc;
    (void)hipSetDevice(ctx->device);
    hipStream_t s = (hipStream_t)stream;
    const size_t need = carve_tape(t, nullptr, fd->batch, fd->tuple_size, fd->n_kpts, fd->sinkhorn_iters);
    if (need > t->tape_bytes) {
        E2EMV_HIP(ctx, hipDeviceSynchronize());
        if (t->d_tape) E2EMV_HIP(ctx, hipFree(t->d_tape));
        t->d_tape = nullptr; t->tape_bytes = 0;
        if (hipMalloc((void**)&t->d_tape, need) != hipSuccess) {
            (void)hipGetLastError();
            return set_err(ctx, E2EMV_ENOMEM, "matcher_forward_train: tape of %zu bytes", need);
        }
        t->tape_bytes = need;
    }
    E2EMV_HIP(ctx, hipMemsetAsync(t->d_tape, 0, need, s));  // padded rows must be finite zeros wherever a GEMM does not write them
    carve_tape(t, t->d_tape, fd->batch, fd->tuple_size, fd->n_kpts, fd->sinkhorn_iters);
    t->have_tape = false;
    if (int rc = encode_train(ctx, t, fd, d_kpts, d_kscores, d_desc, s)) return rc;
    if (int rc = gnn_train(ctx, t, s)) return rc;
    if (int rc = scores_train(ctx, t, d_logZ, s)) return rc;
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
    const int pi = tuple_pair(pair).i, pj = tuple_pair(pair).j;
    const int64_t tuple_stride = (int64_t)T * n_rows * D;
    float* feat = t->t_cfeat[pair];
    float* hid = t->t_chid[pair];
    hipLaunchKernelGGL(conf_feat_kernel, dim3((N + 3) / 4, B), dim3(256), 0, s, N, D, (const float*)t->t_mdesc + (int64_t)pi * n_rows * D,
                       (const float*)t->t_mdesc + (int64_t)pj * n_rows * D, tuple_stride, d_matches0, feat);
    E2EMV_CHECK_LAUNCH(ctx, "conf_feat_kernel");
    GemmArgs g = dense_gemm(t, t->conf0, (int64_t)B * N);
    g.A = feat; g.lda = 2 * D;
    const bool bnb = t->bn_mode == E2EMV_BN_BATCH;
    g.relu = !bnb; g.C = bnb ? t->t_cy[pair] : hid; g.ldc = D;
    if (int rc = launch_gemm_nt(ctx, g, s)) return rc;
    if (bnb)
        if (int rc = bn_forward(ctx, bn_conf(t, t->t_cy[pair], hid, t->t_cst + (int64_t)pair * 3 * D, t->t_part), 1, s)) return rc;
    hipLaunchKernelGGL(conf_fwd_kernel, dim3((unsigned)(((int64_t)B * N + 3) / 4)), dim3(256), 0, s, (int64_t)B * N, D, (const float*)hid,
                       (const float*)t->d_w + t->conf1.w, (const float*)t->d_w + t->conf1.b, d_matches0, d_conf);
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

// ---- the backward over the tape, in stages -----------------------------------------------------------------------------------
// Scratch of e2emv_matcher_backward in the context's workspace.  Gradients of activations: dx, datt, dmd [Mtot][D], dh, dcat
// [Mtot][2D], dqkv [Mtot][3D]; Sinkhorn: dC [B][N+1][N+1], du, dv, dv2 [B][N+1]; attention: Pb, dPb [B*H][N][n_src N]; bpart: the
// partial sums of the BatchNorm backward (batch statistics only)
struct BackwardWs { float *dx, *datt, *dmd, *dh, *dcat, *dqkv, *dC, *du, *dv, *dv2, *Pb, *dPb; double* bpart; size_t bytes; };
// base == nullptr: the byte count only
static BackwardWs carve_backward_ws(const TrainState* t, char* base) {
    const size_t Mtot = (size_t)t->Mtot, D = t->model.desc_dim, B = t->B, N = t->N, H = t->model.num_heads;
    const size_t n_src_max = t->T > 2 ? t->T - 1 : 1;
    size_t off = 0;
    auto take = [&](size_t bytes) { float* p = base ? (float*)(base + off) : nullptr; off += al256(bytes); return p; };
    BackwardWs w;
    w.dx = take(Mtot * D * 4); w.datt = take(Mtot * D * 4); w.dmd = take(Mtot * D * 4);
    w.dh = take(Mtot * 2 * D * 4); w.dcat = take(Mtot * 2 * D * 4);
    w.dqkv = take(Mtot * 3 * D * 4); w.dC = take(B * (N + 1) * (N + 1) * 4);
    w.du = take(B * (N + 1) * 4); w.dv = take(B * (N + 1) * 4); w.dv2 = take(B * (N + 1) * 4);
    w.Pb = take(B * H * N * n_src_max * N * 4); w.dPb = take(B * H * N * n_src_max * N * 4);
    w.bpart = t->bn_mode == E2EMV_BN_BATCH ? (double*)take((size_t)t->T * BN_MAX_CHUNKS * 2 * 2 * D * 8) : nullptr;
    w.bytes = off + 4096;
    return w;
}

// Sinkhorn reverse sweep and the score matrix, per pair with a d logZ: -> d alpha, d mdesc (added to w.dmd)
static int scores_backward(e2emv_ctx* ctx, const TrainState* t, const BackwardWs& w, const float* const* d_dlogZ, hipStream_t s) {
    const int B = t->B, N = t->N, n_rows = t->n_rows, D = t->model.desc_dim;
    const int64_t tuple_stride = (int64_t)t->T * n_rows * D;
    SkT sk = sk_problem(nullptr, t->ldS, N, t->bin_score);
    const int64_t uvs = (int64_t)(t->iters + 1) * 2 * (N + 1), per = (int64_t)(N + 1) * (N + 1);
    int rc;
    for (int q = 0; q < t->P; ++q) {
        if (!d_dlogZ[q]) continue;  // no gradient reaches this pair's scores
        const TuplePair pr = tuple_pair(q);
        sk.S = t->t_S + (int64_t)q * B * N * t->ldS;
        const float* uv = t->t_uv + (int64_t)q * B * uvs;
        if ((rc = sinkhorn_tape_backward(ctx, sk, B, t->iters, uv, d_dlogZ[q], w.dC, w.du, w.dv, w.dv2, t->d_gw + t->alpha, 0, s))) return rc;
        // scores = md_i md_j^T / sqrt(D):  d md_i += dS md_j / sqrt(D),  d md_j += dS^T md_i / sqrt(D)
        for (int side = 0; side < 2; ++side) {  // (side 1: dS read transposed)
            const int to = side ? pr.j : pr.i, from = side ? pr.i : pr.j;
            GG g;
            g.batch = B; g.M = N; g.N = D; g.K = N;
            g.A = w.dC; g.am = side ? 1 : N + 1; g.ak = side ? N + 1 : 1; g.az0 = per;
            g.B = t->t_mdesc + (int64_t)from * n_rows * D; g.bk = D; g.bn = 1; g.bz0 = tuple_stride;
            g.C = w.dmd + (int64_t)to * n_rows * D; g.ldc = D; g.cz0 = tuple_stride; g.alpha = 1.0f / sqrtf((float)D); g.mode = 1;
            if ((rc = launch_gg(ctx, g, s))) return rc;
        }
    }
    return E2EMV_OK;
}

// confidence heads (pose loss): d conf of every pair that has one -> conf_mlp gradients and two more contributions to d mdesc
static int conf_heads_backward(e2emv_ctx* ctx, const TrainState* t, const BackwardWs& w, const float* const* d_dconf, hipStream_t s) {
    const int B = t->B, N = t->N, n_rows = t->n_rows, D = t->model.desc_dim;
    const int64_t tuple_stride = (int64_t)t->T * n_rows * D, rows = (int64_t)B * N;
    const bool bnb = t->bn_mode == E2EMV_BN_BATCH;
    int rc;
    if (bnb && t->conf_mlp) {  // conf_mlp.1's dgamma / dbeta are summed over the pairs below (zero when no pair has a d conf)
        E2EMV_HIP(ctx, hipMemsetAsync(t->d_graw + t->bns.back().gamma, 0, (size_t)D * sizeof(float), s));
        E2EMV_HIP(ctx, hipMemsetAsync(t->d_graw + t->bns.back().beta, 0, (size_t)D * sizeof(float), s));
    }
    if (!d_dconf || !t->conf_mlp) return E2EMV_OK;
    float* dz = w.du;       // [B*N]      (B (N + 1) floats available)
    float* dhc = w.dcat;    // [B*N][D]
    float* dfeat = w.dh;    // [B*N][2D]
    for (int q = 0; q < t->P; ++q) {
        if (!d_dconf[q]) continue;
        if (!t->t_cmatch[q]) return set_err(ctx, E2EMV_ESTATE, "matcher_backward: d conf for pair %d without e2emv_conf_forward_train", q);
        const TuplePair pr = tuple_pair(q);
        hipLaunchKernelGGL(conf_bwd_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, rows, D, (const float*)t->t_chid[q],
                           (const float*)t->d_w + t->conf1.w, (const float*)t->d_w + t->conf1.b, t->t_cmatch[q], d_dconf[q], dz, dhc);
        E2EMV_CHECK_LAUNCH(ctx, "conf_bwd_kernel");
        if ((rc = dense_backward(ctx, t, t->conf1, rows, dz, 1, t->t_chid[q], D, nullptr, 0, false, s))) return rc;  // (d hidden: conf_bwd_kernel's dhc)
        if (bnb) {  // dhc: d hidden (ReLU mask applied) -> d y of conf_mlp.0; frozen: it is d y already
            BnCall a = bn_conf(t, t->t_cy[q], dhc, t->t_cst + (int64_t)q * 3 * D, w.bpart);
            a.h = t->t_chid[q]; a.accumulate = 1;
            if ((rc = bn_backward(ctx, a, 1, s))) return rc;
        }
        if ((rc = dense_backward(ctx, t, t->conf0, rows, dhc, D, t->t_cfeat[q], 2 * D, dfeat, 2 * D, false, s))) return rc;
        hipLaunchKernelGGL(conf_scatter_kernel, dim3((N + 3) / 4, B), dim3(256), 0, s, N, D, (const float*)dfeat, t->t_cmatch[q],
                           w.dmd + (int64_t)pr.i * n_rows * D, w.dmd + (int64_t)pr.j * n_rows * D, tuple_stride, bnb ? 1 : 0);
        E2EMV_CHECK_LAUNCH(ctx, "conf_scatter_kernel");
    }
    E2EMV_HIP(ctx, hipMemsetAsync(w.du, 0, (size_t)B * (N + 1) * sizeof(float), s));
    return E2EMV_OK;
}

// GNN layer l: w.dx = d x_{l+1} on entry, d x_l on exit
static int gnn_layer_backward(e2emv_ctx* ctx, const TrainState* t, const BackwardWs& w, int l, hipStream_t s) {
    const int D = t->model.desc_dim, nk = (int)t->kenc.size();
    const int64_t Mtot = t->Mtot;
    const TrainLayer& Lw = t->layers[l];
    int rc;
    // x_{l+1} = x_l + W1 h + b1
    if ((rc = dense_backward(ctx, t, Lw.mlp1, Mtot, w.dx, D, t->t_h[l], 2 * D, w.dh, 2 * D, false, s))) return rc;
    // h = relu(W0 [x_l | msg] + b0), batch statistics: relu(BN(W0 [x_l | msg] + b0))
    if ((rc = activation_backward(ctx, t, nk - 1 + l, 2 * D, t->t_hy[l], t->t_hst[l], t->t_h[l], w.dh, w.bpart, s))) return rc;
    if ((rc = dense_backward(ctx, t, Lw.mlp0, Mtot, w.dh, 2 * D, t->t_x[l], D, w.dcat, 2 * D, false, s, t->t_msg[l], D))) return rc;
    hipLaunchKernelGGL(add2d_kernel, dim3(ew_grid(Mtot * D)), dim3(256), 0, s, w.dx, (int64_t)D, (const float*)w.dcat, (int64_t)2 * D, Mtot, D);
    // msg = Wm att + bm   (d msg = dcat[:, D:])
    if ((rc = dense_backward(ctx, t, Lw.merge, Mtot, w.dcat + D, 2 * D, t->t_att[l], D, w.datt, D, false, s))) return rc;
    // att = attention(q|k|v)
    if ((rc = attention_backward(ctx, t->B, t->T, t->N, t->n_rows, D, t->model.num_heads, Lw.type != 0, t->t_qkv[l], w.datt, w.dqkv, w.Pb, w.dPb, s))) return rc;
    // q|k|v = Wqkv x_l + b
    if ((rc = dense_backward(ctx, t, Lw.qkv, Mtot, w.dqkv, 3 * D, t->t_x[l], D, w.dx, D, true, s))) return rc;
    E2EMV_CHECK_LAUNCH(ctx, "layer backward kernels");
    return E2EMV_OK;
}

// keypoint encoder, last layer to first: x_0 = desc + kenc(keypoints), w.dx = d kenc output.  Layer 0's input is the [Mtot][4]
// keypoint record of the tape (3 columns used); no gradient w.r.t. it is needed
static int encoder_backward(e2emv_ctx* ctx, const TrainState* t, const BackwardWs& w, hipStream_t s) {
    const int nk = (int)t->kenc.size();
    float* cur = w.dx;  // gradient w.r.t. the output of encoder layer i (width kdims[i + 1])
    float* bufs[2] = {w.dh, w.dcat};
    int rc;
    for (int i = nk - 1; i >= 0; --i) {
        const TrainDense& d = t->kenc[i];
        if (i < nk - 1 && (rc = activation_backward(ctx, t, i, d.out, t->t_ky[i + 1], t->t_kst[i + 1], t->t_kh[i + 1], cur, w.bpart, s))) return rc;
        float* dX = i ? bufs[(nk - 1 - i) & 1] : nullptr;
        if ((rc = dense_backward(ctx, t, d, t->Mtot, cur, d.out, i ? t->t_kh[i] : t->t_inp, i ? d.in : 4, dX, d.in, false, s))) return rc;
        cur = dX;
    }
    E2EMV_CHECK_LAUNCH(ctx, "encoder backward kernels");
    return E2EMV_OK;
}

// folded gradients (d_gw) -> gradients of the upstream parameters (d_graw)
static int unfold_grads(e2emv_ctx* ctx, const TrainState* t, hipStream_t s) {
    const float* gw = t->d_gw;
    auto ref = [&](const std::string& k) -> float* { auto it = t->raw.find(k); return it == t->raw.end() ? nullptr : t->d_raw + it->second.off; };
    auto gref = [&](const std::string& k) -> float* { auto it = t->raw.find(k); return it == t->raw.end() ? nullptr : t->d_graw + it->second.off; };
    for_each_folded(t, [&](const std::string& conv, const std::string& bn, const TrainDense& d, int rows, int rbase, const int* rmap, const int* cmap) {
        UnfoldArgs a{};
        a.dWf = gw + d.w + (int64_t)rbase * d.in; a.dbf = gw + d.b + rbase; a.ldwf = d.in; a.col0 = 0;
        a.W = ref(conv + ".weight"); a.b = ref(conv + ".bias");
        if (!bn.empty() && ref(bn + ".running_mean") && t->bn_mode == E2EMV_BN_FROZEN) {  // (batch statistics: dgamma / dbeta come from bn_backward)
            a.gamma = ref(bn + ".weight"); a.beta = ref(bn + ".bias"); a.mean = ref(bn + ".running_mean"); a.var = ref(bn + ".running_var");
            a.dgamma = gref(bn + ".weight"); a.dbeta = gref(bn + ".bias");
        }
        a.rmap = rmap; a.cmap = cmap; a.rows = rows; a.cols = d.in;
        a.dW = gref(conv + ".weight"); a.db = gref(conv + ".bias");
        hipLaunchKernelGGL(unfold_kernel, dim3(rows), dim3(256), 0, s, a);
    });
    E2EMV_HIP(ctx, hipMemcpyAsync(gref("bin_score"), gw + t->alpha, sizeof(float), hipMemcpyDeviceToDevice, s));
    E2EMV_CHECK_LAUNCH(ctx, "unfold kernels");
    return E2EMV_OK;
}

extern "C" int e2emv_matcher_backward(e2emv_ctx* ctx, const float* const* d_dlogZ, const float* const* d_dconf, void* stream) {
    if (!ctx || !d_dlogZ) return E2EMV_EINVAL;
    E2EMV_ENTER(ctx, stream);
    TrainState* t = ts_of(ctx);
    if (!t || !t->have_tape) return set_err(ctx, E2EMV_ESTATE, "matcher_backward: no tape - e2emv_matcher_forward_train first");
    (void)hipSetDevice(ctx->device);
    hipStream_t s = (hipStream_t)stream;
    int rc = ws_reserve(ctx, carve_backward_ws(t, nullptr).bytes);
    if (rc) return rc;
    const BackwardWs w = carve_backward_ws(t, ctx->d_ws);
    const int D = t->model.desc_dim, L = (int)t->layers.size();
    E2EMV_HIP(ctx, hipMemsetAsync(t->d_gw, 0, t->w_floats * sizeof(float), s));
    E2EMV_HIP(ctx, hipMemsetAsync(w.dmd, 0, (size_t)t->Mtot * D * sizeof(float), s));
    if ((rc = scores_backward(ctx, t, w, d_dlogZ, s))) return rc;
    if ((rc = conf_heads_backward(ctx, t, w, d_dconf, s))) return rc;
    // final_proj: w.dx = d x_L
    if ((rc = dense_backward(ctx, t, t->final_proj, t->Mtot, w.dmd, D, t->t_x[L], D, w.dx, D, false, s))) return rc;
    for (int l = L - 1; l >= 0; --l)
        if ((rc = gnn_layer_backward(ctx, t, w, l, s))) return rc;
    if ((rc = encoder_backward(ctx, t, w, s))) return rc;
    return unfold_grads(ctx, t, s);
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

// y = x W^T + b over `rows` rows: linear_backward, the function dense_backward runs for every dense layer of the backward
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
    return linear_backward(ctx, d_W, d_dW, ldw, d_db, n_out, n_in, rows, d_dY, ldy, d_X, ldx, nullptr, 0, d_dX, ldx, accumulate != 0, (hipStream_t)stream);
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
