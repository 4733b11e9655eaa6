"""Building blocks of the training path, as far as they can be checked without a GPU (the device side: tests/test_gpu_train_blocks.py).

* The restatement (tests/train_blocks_restatement.py) that serves the GPU file as fp64 reference and fp32 yardstick is itself
  checked in fp64 against torch.autograd through the oracle: the Sinkhorn tape and its reverse sweep against
  ``oracle.sinkhorn.log_optimal_transport`` (logZ, dS, dalpha) on the GPU file's case list, the attention backward against
  ``oracle.matcher.attention`` over the same source lists.  Bar 1e-10 of the largest reference value: two fp64 evaluations of
  the same function in different orders; measured here at most 5e-14 (Sinkhorn, 100 iterations at N = 65) and 2e-15 (attention).
* The premises the GPU cases rest on: the exact-integer linear cases keep every partial sum below 2^24; the Sinkhorn case list
  reaches both column-kernel widths (forced, and for the product-level case by the product's own rule), empty row phases at
  both widths, every residue of (N + 1) % 4 and an N that is no multiple of 4; the monotonic score patterns are monotonic where
  the column kernel sees them; the linear row counts reach 1, 2 and 3 K ranges, a ragged last K step and a ragged last range.
* The three entry points are declared, bound and exported; a null context is E2EMV_EINVAL; the Python wrappers refuse what the
  library would refuse before any device call."""
import ctypes
import os
import re

import pytest
import torch

import train_blocks_restatement as R
from oracle import matcher as OM
from oracle import sinkhorn as OS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("e2emv_train_linear_backward", "e2emv_train_sinkhorn", "e2emv_train_attention_backward")
AUTOGRAD_BAR = 1e-10


# ------------------------------------------------------------------------------------------ restatement against autograd
def _distinct_sinkhorn_problems():
    seen = set()
    for N, cw, B, iters, pat, gs in R.sinkhorn_cases():
        for gp in gs:
            if (N, B, iters, pat, gp) not in seen:
                seen.add((N, B, iters, pat, gp))
                yield N, B, iters, pat, gp


@pytest.mark.parametrize("N", sorted({c[0] for c in R.sinkhorn_cases()}))
def test_sinkhorn_restatement_is_autograd_through_the_oracle(N):
    worst = 0.0
    for n, B, iters, pat, gp in _distinct_sinkhorn_problems():
        if n != N:
            continue
        S = R.sinkhorn_scores(B, N, pat).double()
        G = R.sinkhorn_G(B, N, gp).double()
        logZ, uv = R.sinkhorn_tape(S, R.ALPHA, iters)
        dC, dalpha = R.sinkhorn_reverse(S, R.ALPHA, uv, G)
        Sa = S.clone().requires_grad_(True)
        aa = torch.tensor(R.ALPHA, dtype=torch.float64, requires_grad=True)
        Z = OS.log_optimal_transport(Sa, aa, iters)
        gS, ga = torch.autograd.grad((Z * G).sum(), (Sa, aa), allow_unused=True)
        gS = torch.zeros_like(S) if gS is None else gS
        ga = torch.zeros(()) if ga is None else ga
        e = [float((logZ - Z.detach()).abs().max()) / max(1.0, float(Z.detach().abs().max())),
             float((dC[:, :N, :N] - gS).abs().max()) / max(float(gS.abs().max()), 1e-300),
             abs(float(dalpha - ga)) / max(float(dC[:, :N, N].abs().sum() + dC[:, N, :].abs().sum()), 1e-300)]
        if gp == "zero":
            assert float(dC.abs().max()) == 0.0 and float(dalpha) == 0.0
            e = e[:1]
        assert max(e) < AUTOGRAD_BAR, (N, B, iters, pat, gp, e)
        worst = max(worst, max(e))
    print(f"N={N}: worst relative difference to autograd {worst:.2e}")


@pytest.mark.parametrize("T,cross", R.ATTENTION_MODES)
@pytest.mark.parametrize("spiked", [False, True])
def test_attention_restatement_is_autograd_through_the_oracle(T, cross, spiked):
    H, D, d = 4, 256, 64
    for N in R.ATTENTION_N:
        for B in R.ATTENTION_B:
            qkv, datt = R.attention_operands(B, T, N, H, spiked)
            mine = R.attention_backward(qkv, datt, B, T, N, H, cross)
            x = qkv[:, :N].double().requires_grad_(True)
            loss = 0.0
            for g in range(B * T):
                b, tq = divmod(g, T)
                srcs = R.attention_sources(T, tq, cross)
                to_oracle = lambda m: m.reshape(-1, H, d).permute(2, 1, 0)[None]  # head-major rows -> [1, d, H, n]
                q = to_oracle(x[g, :, :D])
                k = to_oracle(torch.cat([x[b * T + s, :, D:2 * D] for s in srcs], 0))
                v = to_oracle(torch.cat([x[b * T + s, :, 2 * D:] for s in srcs], 0))
                o, _ = OM.attention(q, k, v)
                loss = loss + (o[0].permute(2, 1, 0).reshape(N, D) * datt[g, :N].double()).sum()
            (gx,) = torch.autograd.grad(loss, x)
            assert float(mine[:, N:].abs().max()) == 0.0
            err = float((mine[:, :N] - gx).abs().max()) / float(gx.abs().max())
            assert err < AUTOGRAD_BAR, (T, cross, N, B, err)


def test_linear_restatement_is_autograd():
    bufY, bufX, W, bufD = R.linear_operands("encoder1", 33)
    dY, X = bufY.double(), bufX.double()
    Wd = W.double().requires_grad_(True)
    Xd = X.clone().requires_grad_(True)
    b = torch.zeros(64, dtype=torch.float64, requires_grad=True)
    gX, gW, gb = torch.autograd.grad(((Xd @ Wd.T + b) * dY).sum(), (Xd, Wd, b))
    (dW, db, dX), _ = R.linear_backward(dY, X, W)
    for mine, ref in ((dW, gW), (db, gb), (dX, gX)):
        assert float((mine - ref).abs().max()) < AUTOGRAD_BAR * float(ref.abs().max())


# -------------------------------------------------------------------------------------------------------------- premises
def test_integer_cases_keep_every_partial_sum_exact():
    """Integers in [-8, 8]: a partial sum of any subset of the terms, in any order, is an integer of magnitude at most the sum of
    the magnitudes of all terms; below 2^24 fp32 holds it exactly, so the device result must equal the integer result."""
    for form in R.LINEAR_FORMS:
        n_out, n_in, ldy, ldx, off = R.LINEAR_FORMS[form]
        for rows in R.LINEAR_ROWS:
            bufY, bufX, W, bufD = R.linear_operands(form, rows, integers=True)
            dY, X, dX0 = bufY[:, off:off + n_out], bufX[:, :n_in], bufD[:, :n_in]
            for t in (dY, X, W, dX0):
                assert bool((t == t.round()).all()) and float(t.abs().max()) <= 8
            # (+ 8 * 64 rows: the test starts dW and db from integers in [-8, 8] too)
            assert R.linear_partial_sum_bound(dY, X, W, dX0) + 8 < 2 ** 24


def test_linear_rows_reach_every_split_form():
    forms = {rows: R.linear_splits(rows) for rows in R.LINEAR_ROWS}
    assert {s for s, _ in forms.values()} == {1, 2, 3}
    ragged_step = [rows for rows, (s, kper) in forms.items() if rows % 32]                 # the last K step is partial
    ragged_range = [rows for rows, (s, kper) in forms.items() if s > 1 and rows % kper]    # the last range is shorter
    empty_tail = [rows for rows, (s, kper) in forms.items() if (s - 1) * kper >= rows]
    assert ragged_step and ragged_range and not empty_tail
    # every range but the last is a whole number of 32-deep K steps: no K step straddles two ranges, so inside the kernel the
    # guard of a step against the end of its range can only bite in the last range, where that end is K itself
    assert all(kper % 32 == 0 for _, kper in forms.values())
    assert any(rows < 32 for rows in R.LINEAR_ROWS) and any(rows % 64 and rows > 64 for rows in R.LINEAR_ROWS)
    # colsum walks 64 rows per workgroup, four at a time: a remainder of 1 and of 3 rows behind the groups of four, and none
    assert {min(64, rows - rows // 64 * 64) % 4 for rows in R.LINEAR_ROWS} >= {0, 1, 3}


@pytest.mark.parametrize("num_cus", [256, 304, 64])
def test_sinkhorn_case_list_reaches_every_variant(num_cus):
    cases = list(R.sinkhorn_cases())
    forced = {(N, cw) for N, cw, *_ in cases if cw}
    assert forced >= {(N, cw) for N in R.SINKHORN_N for cw in (32, 64)}
    assert {cw for N, cw, *_ in cases} == {0, 32, 64}
    assert {B for _, _, B, *_ in cases} == {1, 3}
    assert {it for _, _, _, it, *_ in cases} == {0, 1, 2, 20, 100}
    for N in R.SINKHORN_N:
        here = [c for c in cases if c[0] == N and c[1]]
        for cw in (32, 64):
            mine = [c for c in here if c[1] == cw]
            assert {c[2] for c in mine} == {1, 3} and {c[3] for c in mine} >= {0, 1, 2, 20}
            assert {c[4] for c in mine} == {"random1", "random10", "increasing", "decreasing"}
            assert {g for c in mine for g in c[5]} == {"dense", "match", "dustbin", "zero"}
    # empty row phases at both widths, and sizes without any
    for cw in (32, 64):
        empties = {N: R.empty_phases(N, cw) for N in R.SINKHORN_N}
        assert any(e > 0 for e in empties.values()) and any(e == 0 for e in empties.values()), (cw, empties)
        assert empties[1] == 1024 // cw - 2
    assert R.empty_phases(30, 32) == 1 and R.empty_phases(31, 32) == 0 and R.empty_phases(30, 64) == 0
    assert {(N + 1) % 4 for N in R.SINKHORN_N} == {0, 1, 2, 3}
    assert any(N % 4 for N in R.SINKHORN_N) and {N % 4 for N in R.SINKHORN_N} == {0, 1, 2, 3}
    # more than one column workgroup at both widths, and a ragged last one
    assert any((N + 1) > 64 and (N + 1) % 64 for N in R.SINKHORN_N) and any((N + 1) > 32 and (N + 1) % 32 for N in R.SINKHORN_N)
    # what the product's rule picks for the cases that leave the width to it, on a chip of num_cus compute units: the forced
    # widths above do not depend on it; the product-level case of the GPU file (B = number of compute units, N = 63) is the one
    # that reaches the 64-column instances through the rule
    assert R.col_width_of(num_cus, 63, num_cus) == 64
    assert all(R.col_width_of(B, N, num_cus) == 32 for N, cw, B, *_ in cases if cw == 0) or num_cus < 12
    assert R.col_width_of(2, 256, 256) == 32  # (the largest Sinkhorn of the other training tests: 10 workgroups)


@pytest.mark.parametrize("pattern", ["increasing", "decreasing"])
def test_monotonic_score_patterns_are_monotonic_where_the_column_kernel_sees_them(pattern):
    """Column pass of iteration 1 walks x[i] = C[i][j] + u_1[i] down every column: strictly increasing over the N score rows -
    the online maximum moves at every step - or strictly decreasing - it never moves."""
    for N in R.SINKHORN_N:
        if N < 2:
            continue
        S = R.sinkhorn_scores(3, N, pattern)
        _, uv = R.sinkhorn_tape(S, R.ALPHA, 1)
        x = S.double() + uv[:, 1, 0, :N, None]
        step = x[:, 1:] - x[:, :-1]
        assert bool((step > 0.02).all()) if pattern == "increasing" else bool((step < -0.02).all()), N
        assert float(S.max()) < R.ALPHA - 12.0 + 1e-6


def test_reference_of_the_product_level_pose_case_is_well_conditioned():
    """The stage-2 case of the GPU file is held to 1e-3 per parameter tensor against the fp32 oracle.  That bar means something
    only where the fp32 oracle itself is far inside it: the data seed is the first from 9 (the seed of the 256-keypoint test)
    upward at which the fp32 oracle agrees with the fp64 oracle to 1e-5 on every parameter gradient.  Seed 9 is not: the gradient
    of conf_mlp.3.bias is a sum over the matched rows that cancels to 5e-5 of the sum of its magnitudes (1.4e-4 between the two
    oracles).  Decided here on the CPU, from the oracle alone."""
    import test_gpu_backward as GB
    import test_gpu_train_blocks as GT

    def oracle_disagreement(seed):
        case = dict(GT.POSE_CASE, data_seed=seed)
        g32 = GB._pose_loss_reference(**case)["leaves"]
        g64 = GB._pose_loss_reference(**case, dtype=torch.float64)["leaves"]
        # (a bias on the keys has a zero gradient: noise on both sides, test_gpu_backward._check)
        return max(float((g32[k].grad.double() - g64[k].grad).norm() / g64[k].grad.norm()) for k in g32 if not k.endswith("attn.proj.1.bias"))

    assert GT.POSE_CASE["B"] == 2 and GT.POSE_CASE["N"] == 200
    seeds = range(9, GT.POSE_CASE["data_seed"] + 1)
    found = [oracle_disagreement(seed) for seed in seeds]
    print("fp32 oracle against fp64 oracle, worst parameter, per data seed:", dict(zip(seeds, found)))
    assert all(d >= 1e-5 for d in found[:-1]) and found[-1] < 1e-5, found


def test_reference_of_the_all_regions_case_is_well_conditioned():
    """test_gpu_backward.test_every_tape_region_at_once holds the device to 1e-3 per parameter tensor against the fp64 oracle.  Its data
    seed is the first from 1 upward at which the problem is well conditioned in the device's own precision, decided here from the
    oracle alone: the fp32 oracle agrees with the fp64 oracle to 1e-4 on every parameter gradient (a tenth of the bar: nine tenths
    are left to the device's other summation orders), both make the same matches (the conf heads gather by them), every pair has
    matches for its conf head and no parameter has a zero gradient.  The shape is the one at which every tape region exists and
    no two kinds of region have the same size."""
    import test_gpu_backward as GB
    c = GB.TAPE_CASE
    assert (c["B"], c["N"], c["T"], c["iters"]) == (2, 129, 3, 3)
    n_rows, ldS = (c["N"] + 127) // 128 * 128, (c["N"] + 3) // 4 * 4
    assert n_rows == 256 != c["N"] and ldS == 132 != c["N"]

    def conditioned(seed):
        r64, r32 = GB._all_regions_reference(seed), GB._all_regions_reference(seed, dtype=torch.float32)
        cfg = r64["model"].config
        assert cfg["conf_mlp"] and cfg["frozen_batchnorm"] is False and cfg["GNN_layers"] == ["self", "cross"] and len(r64["pairs"]) == 3
        g64, g32 = r64["leaves"], r32["leaves"]
        # (the loss does not depend on these biases: noise on both sides, test_gpu_backward._check)
        worst = max(float((g32[k].grad.double() - g64[k].grad).norm() / g64[k].grad.norm()) for k in g64
                    if not k.endswith("attn.proj.1.bias") and k not in r64["free"])
        m64, m32 = ([r["ref"][f"matches{i}_{i}_{j}"] for i, j in r["pairs"]] for r in (r64, r32))
        print(f"data seed {seed}: fp32 oracle against fp64 oracle, worst parameter {worst:.2e}; matches per pair {[int((m >= 0).sum()) for m in m64]}")
        return (worst < 1e-4 and all(torch.equal(a, b) for a, b in zip(m64, m32)) and all(int((m >= 0).sum()) > 0.3 * c["B"] * c["N"] for m in m64)
                and all(float(g.grad.norm()) > 0 for k, g in g64.items() if k not in r64["free"]))

    found = [conditioned(seed) for seed in range(1, c["data_seed"] + 1)]
    assert not any(found[:-1]) and found[-1], found


def test_spiked_attention_case_is_peaked():
    qkv, _ = R.attention_operands(1, 2, 65, spiked=True)
    q, k = qkv[0, 32, :64].double(), qkv[0, 0, 256:320].double()
    assert float(q @ k) / 8 > 30 and torch.equal(qkv[1, 0, 256:512], qkv[0, 0, 256:512])


# ------------------------------------------------------------------------------------------------------------------ API
def test_header_declares_and_library_exports_the_blocks(lib_built):
    from e2e_multi_view_matching_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "e2emv.h")).read()
    declared = set(re.findall(r"\b(e2emv_[a-z0-9_]+)\s*\(", hdr))
    lib = ctypes.CDLL(lib_built)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NEW:
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
        decl = re.search(r"int %s\((.*?)\);" % name, hdr, re.S).group(1)
        assert len(decl.split(",")) == len(_lib.SIGNATURES[name][1]), name
        assert doc.count("`%s`" % name) >= 1, name


def test_null_context_and_null_buffers_are_rejected(lib_built):
    from e2e_multi_view_matching_amd import _lib
    lib = _lib.load_library()
    assert lib.e2emv_train_linear_backward(None, 4, 2, 2, None, 2, None, 2, None, 2, None, None, None, 0, None) == _lib.EINVAL
    assert lib.e2emv_train_sinkhorn(None, 1, 4, None, 4, 0.5, 1, 0, None, None, None, None, None, None) == _lib.EINVAL
    assert lib.e2emv_train_attention_backward(None, 1, 2, 4, 256, 4, 0, None, None, None, None) == _lib.EINVAL


def _no_device(monkeypatch):
    from e2e_multi_view_matching_amd import _lib, train_ops

    def no_device(*a, **k):
        raise AssertionError("a device call was made")
    monkeypatch.setattr(_lib, "context", no_device)
    monkeypatch.setattr(train_ops, "_ctx", no_device)
    return train_ops


def test_wrappers_refuse_bad_arguments_before_any_device_call(monkeypatch):
    ops = _no_device(monkeypatch)
    z = torch.zeros
    for N in (0, 2049):
        with pytest.raises(ValueError, match="N"):
            ops.sinkhorn(z((1, N, N)), 0.5, 3)
        with pytest.raises(ValueError, match="N"):
            ops.attention_backward(z((2, 128, 768)), z((2, 128, 256)), 1, 2, N, 4, False)
    for cw in (1, 16, 48, 128, -32):
        with pytest.raises(ValueError, match="col_width"):
            ops.sinkhorn(z((1, 8, 8)), 0.5, 3, col_width=cw)
    with pytest.raises(ValueError, match="iters"):
        ops.sinkhorn(z((1, 8, 8)), 0.5, -1)
    with pytest.raises(ValueError, match="G must be"):
        ops.sinkhorn(z((1, 8, 8)), 0.5, 1, G=z((1, 8, 8)))
    with pytest.raises(ValueError, match=r"\[B, N, N\]"):
        ops.sinkhorn(z((1, 8, 9)), 0.5, 1)
    for T in (1, 9):
        with pytest.raises(ValueError, match="T"):
            ops.attention_backward(z((T, 128, 768)), z((T, 128, 256)), 1, T, 5, 4, True)
    with pytest.raises(ValueError, match="qkv must be"):
        ops.attention_backward(z((2, 64, 768)), z((2, 64, 256)), 1, 2, 5, 4, True)   # rows not padded to 128
    with pytest.raises(ValueError, match="head dim"):
        ops.attention_backward(z((2, 128, 768)), z((2, 128, 256)), 1, 2, 5, 8, True)
    with pytest.raises(ValueError, match="datt must be"):
        ops.attention_backward(z((2, 128, 768)), z((2, 128, 128)), 1, 2, 5, 4, True)
    dY, X, W = z((8, 4)), z((8, 3)), z((4, 3))
    with pytest.raises(ValueError, match=r"X must be fp32 \[7,"):  # (the row count is dY's)
        ops.linear_backward(z((7, 4)), X, W, z((4, 3)), z(4))
    with pytest.raises(ValueError, match="dY"):
        ops.linear_backward(z((8, 3)), X, W, z((4, 3)), z(4))
    with pytest.raises(ValueError, match="X"):
        ops.linear_backward(dY, z((8, 2)), W, z((4, 3)), z(4))
    with pytest.raises(ValueError, match="db"):
        ops.linear_backward(dY, X, W, z((4, 3)), z(5))
    with pytest.raises(ValueError, match="dW"):
        ops.linear_backward(dY, X, W, z((4, 3), dtype=torch.float64), z(4))
    with pytest.raises(ValueError, match="unit column stride"):
        ops.linear_backward(z((4, 8)).T, X, W, z((4, 3)), z(4))
    with pytest.raises(AssertionError, match="a device call"):  # (the checks passed: only then is the device asked for)
        ops.linear_backward(dY, X, W, z((4, 3)), z(4))
