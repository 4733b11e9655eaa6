"""fp64 reference of the attention building blocks on a ragged tuple (helper of tests/test_attention_reference.py and
tests/test_gpu_attention_edges.py; no test lives here).

Layout of the kernels: qkv [B*T, n_rows, 3D] = q | k | v with head-major channels (c = h*d + dd), image g = b*T + t."""
import torch


def attention_ref(qkv, B, T, nv, H, cross):
    """softmax(q k^T / sqrt(d)) v per head, fp64 -> [B*T, n_rows, D].  nv: an int or T ints, the valid keypoints of image t of
    every tuple.  Queries of image (b, t): its first nv[t] rows.  Keys and values: the first nv[s] rows of every other image s
    of tuple b, concatenated in image order (cross), or the image's own first nv[t] rows (self).  Rows at and beyond nv[t] of
    the result stay zero: they are never to be compared."""
    nv = [int(nv)] * T if isinstance(nv, int) else [int(n) for n in nv]
    assert len(nv) == T
    n_img, n_rows, D3 = qkv.shape
    assert n_img == B * T and all(1 <= n <= n_rows for n in nv)
    D = D3 // 3
    d = D // H
    x = qkv.double()
    q, k, v = (x[..., i * D:(i + 1) * D].reshape(n_img, n_rows, H, d) for i in range(3))
    out = torch.zeros(n_img, n_rows, H, d, dtype=torch.float64)
    for b in range(B):
        for t in range(T):
            g = b * T + t
            srcs = [s for s in range(T) if s != t] if cross else [t]
            kk = torch.cat([k[b * T + s, :nv[s]] for s in srcs], 0)
            vv = torch.cat([v[b * T + s, :nv[s]] for s in srcs], 0)
            logits = torch.einsum("nhd,mhd->hnm", q[g, :nv[t]], kk) / d ** 0.5
            out[g, :nv[t]] = torch.einsum("hnm,mhd->nhd", torch.softmax(logits, -1), vv)
    return out.reshape(n_img, n_rows, D)


def valid_error(out, ref, T, nv):
    """max |out - ref| over the valid rows of every image (out, ref: [B*T, n_rows, D])."""
    nv = [int(nv)] * T if isinstance(nv, int) else list(nv)
    return max(float((out[g, :nv[g % T]].double() - ref[g, :nv[g % T]].double()).abs().max()) for g in range(out.shape[0]))
