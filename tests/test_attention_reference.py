"""CPU: the fp64 ragged-tuple attention reference of the GPU edge tests (tests/attention_restatement.py) against the two
statements of the operation the suite already trusts - ``_attention_ref`` of tests/test_gpu_kernels.py (uniform counts) and
``oracle.matcher.attention`` fed per image the way ``oracle.matcher.gnn`` feeds it.  fp64 against fp64: the bar is 1e-12."""
import pytest
import torch

import attention_restatement as ar
from oracle import matcher as OM

H, D = 4, 256
BAR = 1e-12
RAGGED = [(2, (33, 70)), (3, (65, 1, 40)), (5, (1, 64, 65, 30, 129))]


def _qkv(B, T, n_rows, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B * T, n_rows, 3 * D, generator=g, dtype=torch.float64) * 1.5


def _through_the_oracle(qkv, B, T, nv, cross):
    """``oracle.matcher.attention`` per image on the [1, d, H, n] views of q, k, v; sources concatenated along the keypoint
    axis as ``oracle.matcher.gnn`` does for "cross"."""
    n_img, n_rows, _ = qkv.shape
    d = D // H

    def view(g, part, n):  # rows [n, (h, dd)] -> [1, dd, h, n]
        return qkv[g, :n, part * D:(part + 1) * D].reshape(n, H, d).permute(2, 1, 0).unsqueeze(0)

    out = torch.zeros(n_img, n_rows, D, dtype=torch.float64)
    for b in range(B):
        for t in range(T):
            g = b * T + t
            srcs = [s for s in range(T) if s != t] if cross else [t]
            k = torch.cat([view(b * T + s, 1, nv[s]) for s in srcs], dim=3)
            v = torch.cat([view(b * T + s, 2, nv[s]) for s in srcs], dim=3)
            o, prob = OM.attention(view(g, 0, nv[t]), k, v)
            assert prob.shape == (1, H, nv[t], sum(nv[s] for s in srcs))
            out[g, :nv[t]] = o[0].permute(2, 1, 0).reshape(nv[t], D)
    return out


@pytest.mark.parametrize("cross", [0, 1])
@pytest.mark.parametrize("B,T,n_rows,n_valid", [(2, 2, 128, 128), (1, 3, 128, 77), (2, 5, 128, 1)])
def test_uniform_counts_equal_the_reference_of_the_kernel_tests(B, T, n_rows, n_valid, cross):
    from test_gpu_kernels import _attention_ref
    qkv = _qkv(B, T, n_rows, 100 + n_valid)
    want = _attention_ref(qkv, B, T, n_valid, H, cross)
    for nv in (n_valid, [n_valid] * T):
        got = ar.attention_ref(qkv, B, T, nv, H, cross)
        assert float((got - want).abs().max()) < BAR
        assert ar.valid_error(got, want, T, nv) < BAR


@pytest.mark.parametrize("cross", [0, 1])
@pytest.mark.parametrize("T,nv", RAGGED)
def test_ragged_tuples_equal_the_oracle_attention(T, nv, cross):
    B, n_rows = 2, 256 if max(nv) > 128 else 128
    qkv = _qkv(B, T, n_rows, 7 * T + cross)
    got = ar.attention_ref(qkv, B, T, nv, H, cross)
    want = _through_the_oracle(qkv, B, T, nv, cross)
    assert ar.valid_error(got, want, T, nv) < BAR
    for g in range(B * T):  # rows at and beyond the count stay zero
        assert not got[g, nv[g % T]:].any()
    # with every count equal to the largest it is the uniform reference again (the ragged one differs from it: the counts matter)
    from test_gpu_kernels import _attention_ref
    top = max(nv)
    assert float((ar.attention_ref(qkv, B, T, [top] * T, H, cross) - _attention_ref(qkv, B, T, top, H, cross)).abs().max()) < BAR
    assert ar.valid_error(got, _attention_ref(qkv, B, T, top, H, cross), T, nv) > 1e-3


def test_padding_rows_do_not_reach_the_reference():
    T, nv = 3, (65, 1, 40)
    qkv = _qkv(2, T, 128, 5)
    ref = ar.attention_ref(qkv, 2, T, nv, H, 1)
    noisy = qkv.clone()
    for g in range(2 * T):
        noisy[g, nv[g % T]:] = 1e3
    assert torch.equal(ar.attention_ref(noisy, 2, T, nv, H, 1), ref)
