"""Three stages of the training path alone (building blocks for per-kernel parity tests): thin ctypes wrappers of
``e2emv_train_linear_backward``, ``e2emv_train_sinkhorn`` and ``e2emv_train_attention_backward`` - the host functions
``e2emv_matcher_forward_train`` / ``e2emv_matcher_backward`` call, on the caller's tensors.  torch = memory only; arguments the
library would refuse raise ValueError here, before any device call."""
import torch

from . import _lib
from .ops import _ctx

MAX_KPTS = 2048


def _strided_rows(name, t, rows, cols):
    """fp32 [rows, >= cols] with unit column stride; returns its row stride (the leading dimension)."""
    if t.dtype != torch.float32 or t.dim() != 2 or t.shape[0] != rows or t.shape[1] < cols or (t.shape[1] > 1 and t.stride(1) != 1):
        raise ValueError(f"linear_backward: {name} must be fp32 [{rows}, >= {cols}] with unit column stride")
    ld = int(t.stride(0)) if rows > 1 else max(int(t.stride(0)), cols)
    if ld < cols:
        raise ValueError(f"linear_backward: the rows of {name} overlap")
    return ld


def linear_backward(dY, X, W, dW, db, dX=None, accumulate=False):
    """Backward of y = x W^T + b on strided fp32 views: dY [rows, n_out], X [rows, n_in], W [n_out, n_in] with unit column stride;
    the row stride is the leading dimension, so a column slice of a wider buffer is passed as it is.  dW (the row stride of W) and
    db [n_out] are ADDED to, dX (the row stride of X; optional) is written, or added to with ``accumulate``.  In place."""
    if W.dim() != 2 or dY.dim() != 2 or min(W.shape) < 1 or dY.shape[0] < 1:
        raise ValueError("linear_backward: W [n_out, n_in] and dY [rows, n_out] must be non-empty matrices")
    (n_out, n_in), rows = (int(n) for n in W.shape), int(dY.shape[0])
    ldy, ldx, ldw = _strided_rows("dY", dY, rows, n_out), _strided_rows("X", X, rows, n_in), _strided_rows("W", W, n_out, n_in)
    if _strided_rows("dW", dW, n_out, n_in) != ldw or (dX is not None and _strided_rows("dX", dX, rows, n_in) != ldx):
        raise ValueError("linear_backward: dW / dX share the row stride of W / X")
    if db.dtype != torch.float32 or db.numel() != n_out or not db.is_contiguous():
        raise ValueError(f"linear_backward: db must be fp32 [{n_out}]")
    ctx = _ctx(dY)
    with torch.cuda.device(dY.device):
        ctx.call("e2emv_train_linear_backward", rows, n_out, n_in, _lib.ptr(dY), ldy, _lib.ptr(X), ldx, _lib.ptr(W), ldw, _lib.ptr(dW), _lib.ptr(db),
                 _lib.ptr(dX), 1 if accumulate else 0, _lib.stream_ptr(dY.device))


def sinkhorn(S, alpha, iters, col_width=0, G=None, tape=False, pad_value=0.0):
    """The unrolled log-domain Sinkhorn of the training forward on scores S [B, N, N] (stored with the product's row stride, N
    rounded up to 4) and, with G = dLoss / dlogZ [B, N+1, N+1], its reverse sweep.  col_width: 0 = the product's choice of column
    kernel, 32 / 64 = that instance; pad_value: what the padding columns of the stored scores hold (never read).  Returns
    {"logZ" [B,N+1,N+1], "uv" [B,iters+1,2,N+1] (``tape``), "dC" [B,N+1,N+1] and "dalpha" [] (with G)}."""
    if S.dim() != 3 or S.shape[1] != S.shape[2]:
        raise ValueError("sinkhorn: S must be [B, N, N]")
    B, N = int(S.shape[0]), int(S.shape[1])
    if B < 1 or not 1 <= N <= MAX_KPTS:
        raise ValueError(f"sinkhorn: B={B}, N={N} (N in 1..{MAX_KPTS})")
    if col_width not in (0, 32, 64):
        raise ValueError("sinkhorn: col_width is 0, 32 or 64")
    if int(iters) < 0:
        raise ValueError("sinkhorn: negative iters")
    if G is not None and tuple(G.shape) != (B, N + 1, N + 1):
        raise ValueError(f"sinkhorn: G must be [{B}, {N + 1}, {N + 1}]")
    ctx = _ctx(S)
    dev = S.device
    ldS = (N + 3) // 4 * 4
    Sp = torch.full((B, N, ldS), float(pad_value), dtype=torch.float32, device=dev)
    Sp[:, :, :N] = S
    out = {"logZ": torch.empty((B, N + 1, N + 1), dtype=torch.float32, device=dev)}
    if tape:
        out["uv"] = torch.empty((B, int(iters) + 1, 2, N + 1), dtype=torch.float32, device=dev)
    g = None
    if G is not None:
        g = G.to(torch.float32).contiguous()
        out["dC"] = torch.empty((B, N + 1, N + 1), dtype=torch.float32, device=dev)
        out["dalpha"] = torch.empty((), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        ctx.call("e2emv_train_sinkhorn", B, N, _lib.ptr(Sp), ldS, float(alpha), int(iters), int(col_width), _lib.ptr(g), _lib.ptr(out["logZ"]),
                 _lib.ptr(out.get("uv")), _lib.ptr(out.get("dC")), _lib.ptr(out.get("dalpha")), _lib.stream_ptr(dev))
    return out


def attention_backward(qkv, datt, B, T, N, H, cross):
    """Backward of ``ops.attention``: qkv [B*T, n_rows, 3D] head-major, datt = dLoss / d out [B*T, n_rows, D], n_rows = N rounded up
    to 128, N valid rows per image -> dqkv [B*T, n_rows, 3D] (rows N.. of an image: zeros)."""
    if not 1 <= int(N) <= MAX_KPTS or not 2 <= int(T) <= _lib.MAX_TUPLE or int(B) < 1:
        raise ValueError(f"attention_backward: B={B}, T={T}, N={N} (T in 2..{_lib.MAX_TUPLE}, N in 1..{MAX_KPTS})")
    n_rows = (int(N) + 127) // 128 * 128
    if qkv.dim() != 3 or qkv.shape[0] != B * T or qkv.shape[1] != n_rows or qkv.shape[2] % 3:
        raise ValueError(f"attention_backward: qkv must be [{B * T}, {n_rows}, 3D]")
    D = int(qkv.shape[2]) // 3
    if D != 64 * int(H):
        raise ValueError("attention_backward: head dim must be 64")
    if tuple(datt.shape) != (B * T, n_rows, D):
        raise ValueError(f"attention_backward: datt must be [{B * T}, {n_rows}, {D}]")
    ctx = _ctx(qkv)
    q, d = qkv.contiguous().float(), datt.contiguous().float()
    out = torch.empty_like(q)
    with torch.cuda.device(q.device):
        ctx.call("e2emv_train_attention_backward", int(B), int(T), int(N), D, int(H), 1 if cross else 0, _lib.ptr(q), _lib.ptr(d), _lib.ptr(out),
                 _lib.stream_ptr(q.device))
    return out
