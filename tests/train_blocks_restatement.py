"""Plain-torch restatement of three stages of the training path (csrc/train.hip, csrc/train_kernels.h), the dtype a parameter:
at float64 the reference, at float32 the yardstick of tests/test_gpu_train_blocks.py (helper of that file and of
tests/test_train_blocks.py; no test lives here).

Sinkhorn: the couplings, the tape (u_t, v_t of every iteration) and the reverse sweep over that tape, half iteration by half
iteration in the kernels' order - not autograd.  Attention backward: per query image over its source list.  Linear backward:
the three products of a dense layer."""
import math

import torch


# ------------------------------------------------------------------------------------------------------------- Sinkhorn
def couplings(S, alpha):
    """S [B,N,N] -> C [B,N+1,N+1]: the dustbin row and column hold alpha."""
    B, N, _ = S.shape
    C = torch.full((B, N + 1, N + 1), float(alpha), dtype=S.dtype)
    C[:, :N, :N] = S
    return C


def _marginals(N, dtype):
    norm = -math.log(2 * N)
    log_mu = torch.full((N + 1,), norm, dtype=dtype)
    log_mu[N] = math.log(N) + norm
    return norm, log_mu, log_mu.clone()  # (M = N: log_nu has the same values)


def sinkhorn_tape(S, alpha, iters, dtype=torch.float64):
    """-> logZ [B,N+1,N+1], uv [B,iters+1,2,N+1] (uv[:, t, 0] = u_t, uv[:, t, 1] = v_t, t = 0: zeros)."""
    C = couplings(S.to(dtype), alpha)
    B, N = C.shape[0], C.shape[1] - 1
    norm, log_mu, log_nu = _marginals(N, dtype)
    uv = torch.zeros((B, iters + 1, 2, N + 1), dtype=dtype)
    for t in range(1, iters + 1):
        v_prev = uv[:, t - 1, 1]
        u = log_mu - torch.logsumexp(C + v_prev[:, None, :], dim=2)   # row pass
        v = log_nu - torch.logsumexp(C + u[:, :, None], dim=1)        # column pass
        uv[:, t, 0], uv[:, t, 1] = u, v
    logZ = C + uv[:, iters, 0][:, :, None] + uv[:, iters, 1][:, None, :] - norm
    return logZ, uv


def sinkhorn_reverse(S, alpha, uv, G, dtype=torch.float64):
    """The reverse sweep over a tape: G = dLoss / dlogZ -> dC [B,N+1,N+1] (d couplings, dustbins included), dalpha (scalar: the
    dustbin row and column of dC summed over all problems).  dS = dC[:, :N, :N]."""
    C = couplings(S.to(dtype), alpha)
    uv, G = uv.to(dtype), G.to(dtype)
    B, N = C.shape[0], C.shape[1] - 1
    iters = uv.shape[1] - 1
    _, log_mu, log_nu = _marginals(N, dtype)
    # init: logZ = C + u_T + v_T - norm
    dC = G.clone()
    du = G.sum(2)
    dv = G.sum(1)
    for t in range(iters, 0, -1):
        u_t, v_t, v_prev = uv[:, t, 0], uv[:, t, 1], uv[:, t - 1, 1]
        # v-half: v_t = log_nu - LSE_i(C + u_t)
        P = torch.exp(C + u_t[:, :, None] + v_t[:, None, :] - log_nu[None, None, :])
        W = dv[:, None, :] * P
        dC = dC - W
        du = du - W.sum(2)
        # u-half: u_t = log_mu - LSE_j(C + v_{t-1})
        P = torch.exp(C + v_prev[:, None, :] + u_t[:, :, None] - log_mu[None, :, None])
        W = du[:, :, None] * P
        dC = dC - W
        dv = -W.sum(1)
        du = torch.zeros_like(du)
    dalpha = dC[:, :N, N].sum() + dC[:, N, :].sum()
    return dC, dalpha


def col_width_of(B, N, num_cus):
    """Columns per workgroup the product picks for the two column kernels."""
    return 32 if B * ((N + 1 + 63) // 64) < num_cus else 64


def empty_phases(N, col_width):
    """Row phases of a column workgroup (1024 threads: 1024 / col_width phases, phase p takes rows p, p + phases, ...) that get no
    row of the N + 1."""
    return max(0, 1024 // col_width - (N + 1))


# ------------------------------------------------------------------------------------------------------------ attention
def attention_sources(T, tq, cross):
    return [s for s in range(T) if s != tq] if cross else [tq]


def attention_backward(qkv, datt, B, T, N, H, cross, dtype=torch.float64):
    """dqkv [B*T, n_rows, 3D]: per query image tq of a tuple, over its source images: P = softmax(q k^T / 8), dP = dO v^T,
    dS = P (dP - sum_j P dP) / 8, dq += dS k, dk_s += dS^T q, dv_s += P^T dO.  Only the first N rows of an image are read; the
    others of the result are zero."""
    n_img, n_rows, D3 = qkv.shape
    D = D3 // 3
    d = D // H
    scale = 1.0 / d ** 0.5
    out = torch.zeros((n_img, n_rows, D3), dtype=dtype)
    for g in range(n_img):
        b, tq = divmod(g, T)
        srcs = attention_sources(T, tq, cross)
        q = qkv[g, :N, :D].to(dtype).reshape(N, H, d)
        kk = torch.cat([qkv[b * T + s, :N, D:2 * D] for s in srcs], 0).to(dtype).reshape(-1, H, d)
        vv = torch.cat([qkv[b * T + s, :N, 2 * D:] for s in srcs], 0).to(dtype).reshape(-1, H, d)
        dO = datt[g, :N].to(dtype).reshape(N, H, d)
        P = torch.softmax(torch.einsum("nhd,mhd->hnm", q, kk) * scale, -1)
        dP = torch.einsum("nhd,mhd->hnm", dO, vv)
        dS = P * (dP - (P * dP).sum(-1, keepdim=True)) * scale
        out[g, :N, :D] += torch.einsum("hnm,mhd->nhd", dS, kk).reshape(N, D)
        dk = torch.einsum("hnm,nhd->mhd", dS, q).reshape(-1, D)
        dv = torch.einsum("hnm,nhd->mhd", P, dO).reshape(-1, D)
        for si, s in enumerate(srcs):
            out[b * T + s, :N, D:2 * D] += dk[si * N:(si + 1) * N]
            out[b * T + s, :N, 2 * D:] += dv[si * N:(si + 1) * N]
    return out


# --------------------------------------------------------------------------------------------------------------- linear
def linear_backward(dY, X, W, dX0=None, dtype=torch.float64):
    """y = x W^T + b: dW = dY^T X, db = column sums of dY, dX = dY W (+ dX0).  Returns each with the sum of the magnitudes of
    its terms (the natural scale of its rounding error): (dW, db, dX), (sW, sb, sX)."""
    dY, X, W = dY.to(dtype), X.to(dtype), W.to(dtype)
    dW, db, dX = dY.T @ X, dY.sum(0), dY @ W
    sW, sb, sX = dY.abs().T @ X.abs(), dY.abs().sum(0), dY.abs() @ W.abs()
    if dX0 is not None:
        dX = dX + dX0.to(dtype)
        sX = sX + dX0.to(dtype).abs()
    return (dW, db, dX), (sW, sb, sX)


def linear_partial_sum_bound(dY, X, W, dX0=None):
    """Largest magnitude any partial sum of the three products can reach, whatever the order of the additions: the sums of the
    magnitudes of the terms."""
    _, (sW, sb, sX) = linear_backward(dY, X, W, dX0)
    return max(float(sW.max()), float(sb.max()), float(sX.max()))


# ------------------------------------------------------------------------------------------- case lists and their inputs
# (shared by tests/test_train_blocks.py, which checks on the CPU what the lists are supposed to reach, and
# tests/test_gpu_train_blocks.py, which runs them)
ALPHA = float(torch.tensor(0.7, dtype=torch.float32))  # (a value fp32 holds exactly: every side gets the same dustbin score)
SINKHORN_N = (1, 3, 30, 31, 32, 63, 64, 65, 127, 200)
SINKHORN_WIDTHS = (32, 64)
# (B, iters, score pattern, G patterns) run at EVERY (N, width): every B, iteration count, score and G pattern at every size
SINKHORN_VARIANTS = (
    (1, 0, "random1", ("dense", "match", "dustbin", "zero")),
    (3, 1, "random10", ("dense", "match", "dustbin", "zero")),
    (1, 2, "increasing", ("dense", "match", "dustbin", "zero")),
    (3, 20, "decreasing", ("dense", "match", "dustbin", "zero")),
    (3, 20, "random1", ("match", "dense")),
    (1, 20, "random10", ("match", "dense")),
    (3, 2, "increasing", ("match",)),
    (1, 1, "decreasing", ("match",)),
)
# (N, width, B, iters, score pattern, G patterns) run once
SINKHORN_EXTRA = (
    (65, 64, 3, 100, "random10", ("match", "dense")),
    (65, 32, 1, 100, "random1", ("match",)),
    (200, 0, 3, 20, "random1", ("match", "dense")),
    (64, 0, 1, 2, "random10", ("dense",)),
)


def sinkhorn_cases():
    """Every (N, width, B, iters, score pattern, G patterns) the GPU file runs."""
    for N in SINKHORN_N:
        for cw in SINKHORN_WIDTHS:
            for B, iters, pat, gs in SINKHORN_VARIANTS:
                yield N, cw, B, iters, pat, gs
    yield from SINKHORN_EXTRA


def _gen(*key):
    return torch.Generator().manual_seed(hash(tuple(int(k) if not isinstance(k, str) else sum(map(ord, k)) for k in key)) % (2 ** 31))


def sinkhorn_scores(B, N, pattern):
    """fp32 scores [B,N,N].  random1 / random10: normal, scale 1 / 10.  increasing / decreasing: every column strictly
    increasing / decreasing down the rows in steps of 0.05 +- 0.01, all scores at least 12 below the dustbin score - the
    dustbin column then dominates every row sum, u_1 is constant over the rows to ~1e-3, and the column pass of iteration 1
    sees C + u_1 strictly monotonic down the N score rows of every column: the online maximum of skt_col_kernel moves at every
    step of every phase (increasing) or at none (decreasing; the dustbin row below them, at alpha, moves it once)."""
    g = _gen(B, N, pattern)
    if pattern in ("random1", "random10"):
        return (torch.randn((B, N, N), generator=g) * (1.0 if pattern == "random1" else 10.0)).float()
    steps = 0.05 + 0.02 * (torch.rand((B, N, N), generator=g) - 0.5)
    ramp = torch.cumsum(steps, 1)                    # strictly increasing down the rows
    if pattern == "decreasing":
        ramp = ramp.flip(1)
    col = torch.rand((B, 1, N), generator=g)         # a level per column
    return (ALPHA - 12.0 - 0.05 * 1.2 * N + ramp - col).float()


def sinkhorn_G(B, N, pattern):
    """dLoss / dlogZ [B,N+1,N+1] fp32.  dense: normal.  match: the match loss's own shape (test_gpu_backward._match_loss): -w at
    (i, partner of i) for every row i and at (partner of j, j) for every column j, unmatched ones on the dustbin column / row,
    exact zeros elsewhere.  dustbin: normal on the dustbin row and column only.  zero: all zero."""
    g = _gen(B, N, "G" + pattern)
    G = torch.zeros((B, N + 1, N + 1))
    if pattern == "dense":
        G = torch.randn((B, N + 1, N + 1), generator=g)
    elif pattern == "dustbin":
        G[:, N, :] = torch.randn((B, N + 1), generator=g)
        G[:, :, N] = torch.randn((B, N + 1), generator=g)
    elif pattern == "match":
        for b in range(B):
            perm = torch.randperm(N, generator=g)
            matched = torch.rand(N, generator=g) < 0.6
            w = torch.rand((2, N), generator=g) + 0.5
            for i in range(N):
                j = int(perm[i]) if matched[i] else N
                G[b, i, j] -= w[0, i]
                if matched[i]:
                    G[b, i, j] -= w[1, j]
            for j in set(range(N)) - {int(perm[i]) for i in range(N) if matched[i]}:
                G[b, N, j] -= w[1, j]
    else:
        assert pattern == "zero"
    return G.float()


LINEAR_ROWS = (1, 31, 33, 400, 511, 512, 1027, 1536)
# name -> (n_out, n_in, ldy, ldx, column offset of dY inside its buffer): the forms e2emv_matcher_backward calls
LINEAR_FORMS = {
    "encoder0": (32, 3, 32, 4, 0),       # wgrad of encoder layer 0: the keypoint rows are [x, y, score, -]
    "encoder1": (64, 32, 64, 32, 0),
    "conf_out": (1, 256, 1, 256, 0),     # conf_mlp.3: one output channel
    "mlp0": (256, 512, 256, 512, 0),
    "merge_slice": (256, 256, 512, 256, 256),  # d msg = dcat[:, D:]: a column slice of a [rows][2D] buffer
}


def linear_operands(form, rows, integers=False):
    """fp32 (buffer of dY [rows][ldy], X [rows][ldx], W [n_out][n_in], dX0 [rows][ldx]); the columns of the dY / X buffers that
    the layer does not use hold 1e30: a kernel that read them would show it.  integers: every value an integer in [-8, 8];
    otherwise normal values, every row of dY and X scaled by e^s, s uniform in [-2, 2]."""
    n_out, n_in, ldy, ldx, off = LINEAR_FORMS[form]
    g = _gen(rows, form, int(integers))
    if integers:
        dY, X, W, dX0 = (torch.randint(-8, 9, s, generator=g).float() for s in ((rows, n_out), (rows, n_in), (n_out, n_in), (rows, n_in)))
    else:
        dY = torch.randn((rows, n_out), generator=g) * torch.exp(4 * torch.rand((rows, 1), generator=g) - 2)
        X = torch.randn((rows, n_in), generator=g) * torch.exp(4 * torch.rand((rows, 1), generator=g) - 2)
        W = torch.randn((n_out, n_in), generator=g) / n_in ** 0.5
        dX0 = torch.randn((rows, n_in), generator=g)
    bufY = torch.full((rows, ldy), 1e30)
    bufY[:, off:off + n_out] = dY
    bufX = torch.full((rows, ldx), 1e30)
    bufX[:, :n_in] = X
    bufD = torch.full((rows, ldx), 1e30)
    bufD[:, :n_in] = dX0
    return bufY.float(), bufX.float(), W.float(), bufD.float()


def linear_splits(rows):
    """K ranges of the weight-gradient GEMM (wgrad of train.hip), their length (a multiple of the 32-deep K step) and whether the
    last range / the last K step is ragged."""
    splits = max(1, min(256, rows // 512))
    kper = ((rows + splits - 1) // splits + 31) // 32 * 32
    return splits, kper


ATTENTION_N = (1, 5, 63, 64, 65, 130)
ATTENTION_MODES = ((2, False), (2, True), (3, True), (3, False))  # (T, cross)
ATTENTION_B = (1, 2)


def attention_operands(B, T, N, H=4, spiked=False):
    """fp32 qkv [B*T, n_rows, 3*64*H], datt [B*T, n_rows, 64*H]; rows N.. of every image hold 1e30.  spiked: in every image key 0
    of every head is 6 x query N // 2 of the FIRST image of its tuple - aligned with a query of the same image (self) or of
    another one (cross): that query's softmax row is peaked on one key."""
    D = 64 * H
    n_rows = (N + 127) // 128 * 128
    g = _gen(B, T, N, int(spiked))
    qkv = torch.full((B * T, n_rows, 3 * D), 1e30)
    datt = torch.full((B * T, n_rows, D), 1e30)
    qkv[:, :N] = torch.randn((B * T, N, 3 * D), generator=g)
    datt[:, :N] = torch.randn((B * T, N, D), generator=g)
    if spiked:
        for b in range(B):
            for t in range(T):
                qkv[b * T + t, 0, D:2 * D] = 6.0 * qkv[b * T, N // 2, :D]
    return qkv.float(), datt.float()
