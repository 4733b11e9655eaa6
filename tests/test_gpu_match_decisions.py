"""Arg-max ties and threshold edges of the match block (-m gpu): csrc/sinkhorn_stream.hip - dense_row_argmax,
dense_col_argmax, the FINAL branch of sinkhorn_sweep<KT, FINAL, FULL> and match_finalize.

An index has no tolerance, and random scores never tie: every other test of the suite leaves "lowest index on ties"
(across the lanes of a wave), "strict > keeps the first" (across the four waves of a workgroup, the k-tiles of a lane, the
row chunks of a problem) and the 8-at-a-time chunk merge of match_finalize with its remainder loop unreached.  Here the
ties are planted at the distances at which those rules change hands:

  row maximum tied at columns   j, j+1 with j % 4 < 3 (one lane's quad) | j, j+4 (the neighbouring lane) | j, j+256 (the next
                                k-tile of the same lane) | lane 0 against lane 63 (j, j+252 with j % 256 < 4)
  column maximum tied at rows   r, r+1 with r % 4 < 3 (one wave) | r, r+4 with r % 16 < 12 (the next wave of the workgroup) |
                                r, r+16 (the next chunk) | r, r+144 (past one merge group of 8 chunks)

The reference operation is oracle.sinkhorn.extract_matches (torch.max: the first maximal index) and the requirement is
torch.equal.  Part 1 hands crafted log-assignments to the stand-alone entry (E.extract_matches); part 2 reaches the fused
form behind the Sinkhorn paths through MultiViewMatcher with duplicated keypoints and applies the reference operation to
the scores the device itself produced - which holds whether or not two duplicates came out bit-equal.

Exact ties in the device's scores in part 2, as measured on the MI355X (the test prints, per case and class, planted pairs
whose two cells are bit-equal and the maximum of their row / column, over planted pairs):
  f32, 0 iterations     every planted pair of every class at every shape (REQUIRED: at least one per class - identical inputs
                        go through identical arithmetic there)
  f32, 20 iterations    every planted pair of every class at every shape (recorded)
  f16x2, 0 iterations   every planted pair of every class at every shape (recorded)
  f16x2, 20 iterations  every planted pair of every class at every shape (recorded)
Duplicated keypoints stay bit-equal through the split-operand GEMMs and through the resident Sinkhorn kernels: a column's (row's)
potential depends on the values of its column (row) alone, summed in an order that does not depend on where the column sits.

That the tests notice a wrong rule was checked against libraries built with one rule turned at a time in each merge level
(">" for "<" on the index in the lane merge; ">=" for ">" inside a lane, inside a wave, across the waves, in the 8-chunk groups
and in the remainder loop of match_finalize, in both dense kernels): every such build failed here, in exactly the classes that
level owns."""
import functools
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# (name, distance between the two tied columns of a row, where the first may sit): a lane owns columns 4l .. 4l+3 of every
# 256-column k-tile
COL_CLASSES = (("quad", 1, lambda j: j % 4 < 3), ("lane", 4, lambda j: j % 256 < 252), ("ktile", 256, lambda j: True),
               ("lane0_63", 252, lambda j: j % 256 < 4))
# (name, distance between the two tied rows of a column, where the first may sit): a wave owns 4 rows, a chunk 16
ROW_CLASSES = (("wave", 1, lambda r: r % 4 < 3), ("next_wave", 4, lambda r: r % 16 < 12), ("next_chunk", 16, lambda r: True),
               ("past_merge", 16 * 9, lambda r: True))
THR = 0.2
EDGE = 2.0 ** -12  # far above the error of __expf (~1e-7), far below anything a user could see


# ---------------------------------------------------------------------------------------------------------------- part 1
def _free(rng, n, used, need, pred=lambda k: True):
    """an index k (random order) with k + o unused and in range for every offset o of `need`"""
    for k in rng.permutation(n):
        k = int(k)
        if pred(k) and all(0 <= k + o < n and (k + o) not in used for o in need):
            return k
    return None


def crafted_logZ(B, M, N, seed, neg_inf_row=False):
    """-> (Z [B,M+1,N+1], plants {class: [(b, row or column with the tied maximum)]}, expectations [(b, "m0"|"m1", index, value at THR, value at 0.0, class)]).

    Core: integers in [-48, 0] divided by 4 - about M/49 (N/49) cells of every column (row) hold its maximum, so ties at
    arbitrary distances and non-mutual maxima are everywhere.  Planted on top, each on rows and columns of its own that
    are lowered to <= -0.25 elsewhere, so that the planted cells are the ONLY maxima of their rows and columns and a wrong
    tie-break changes the outcome: (i; j, j+d) = 0 gives matches0[i] = j, matches1[j] = i, matches1[j+d] = -1, and
    (r, r+d; c) = 0 gives matches1[c] = r, matches0[r] = c, matches0[r+d] = -1.  Two more isolated cells hold
    log(THR (1 +- 2^-12)): matched / not matched at THR, both matched at 0."""
    rng = np.random.default_rng(seed)
    g = torch.Generator().manual_seed(seed)
    Z = torch.randn(B, M + 1, N + 1, generator=g)  # the dustbin row and column: random, finite, never looked at
    core = torch.randint(-48, 1, (B, M, N), generator=g).float() / 4.0
    small = min(M, N) < 64  # too few rows / columns for every class in every problem: class k goes to problem k % B
    classes = [("col", n, d, ok) for n, d, ok in COL_CLASSES if d < N] + [("row", n, d, ok) for n, d, ok in ROW_CLASSES if d < M]
    classes.sort(key=lambda c: -c[2])  # the widest first: it has the fewest places to go
    plants = {f"{kind}:{name}": [] for kind, name, _, _ in classes}
    expect = []
    for b in range(B):
        ur, uc = set(), set()
        for k, (kind, name, d, ok) in enumerate(classes):
            if small and k % B != b:
                continue
            for _ in range(1 if small else 3):
                if kind == "col":
                    i, j = _free(rng, M, ur, (0,)), _free(rng, N, uc, (0, d), ok)
                    if i is None or j is None:
                        break
                    ur.add(i), uc.update((j, j + d))
                    core[b, i, :].clamp_(max=-0.25), core[b, :, j].clamp_(max=-0.25), core[b, :, j + d].clamp_(max=-0.25)
                    core[b, i, j] = core[b, i, j + d] = 0.0
                    expect += [(b, "m0", i, j, j, name), (b, "m1", j, i, i, name), (b, "m1", j + d, -1, -1, name)]
                else:
                    r, c = _free(rng, M, ur, (0, d), ok), _free(rng, N, uc, (0,))
                    if r is None or c is None:
                        break
                    ur.update((r, r + d)), uc.add(c)
                    core[b, r, :].clamp_(max=-0.25), core[b, r + d, :].clamp_(max=-0.25), core[b, :, c].clamp_(max=-0.25)
                    core[b, r, c] = core[b, r + d, c] = 0.0
                    expect += [(b, "m1", c, r, r, name), (b, "m0", r, c, c, name), (b, "m0", r + d, -1, -1, name)]
                plants[f"{kind}:{name}"].append((b, i) if kind == "col" else (b, c))  # the row / column with the tied maximum
        # the threshold cells (at every shape): upper side in the first problem, lower side in the last
        for s in [s for s, bb in ((+1, 0), (-1, B - 1)) if bb == b]:
            i, j = _free(rng, M, ur, (0,)), _free(rng, N, uc, (0,))
            assert i is not None and j is not None, (B, M, N, "no room for a threshold cell")
            ur.add(i), uc.add(j)
            core[b, i, :].clamp_(max=-2.0), core[b, :, j].clamp_(max=-2.0)
            core[b, i, j] = math.log(THR * (1.0 + s * EDGE))
            expect += [(b, "m0", i, j if s > 0 else -1, j, "threshold"), (b, "m1", j, i if s > 0 else -1, i, "threshold")]
        if neg_inf_row and b == 0:
            i = _free(np.random.default_rng(seed + 1), M, ur, (0,))
            i = 0 if i is None else i  # (a single row: it IS the threshold row, whose expectations go)
            core[b, i, :] = -math.inf
            expect = [e for e in expect if not (e[0] == b and ((e[1] == "m0" and e[2] == i) or (e[1] == "m1" and e[3] == i)))]
            expect.append((b, "m0", i, -1, -1, "neg_inf_row"))
            neg_row = i
    assert all(plants.values()), (B, M, N, plants)  # every class the shape has room for is planted
    if neg_inf_row:
        plants["neg_inf_row"] = neg_row
    Z[:, :M, :N] = core
    return Z, plants, expect


DENSE_SHAPES = [(2, 1, 1), (2, 17, 5), (2, 144, 256), (1, 160, 257), (2, 1024, 1024), (1, 2048, 2047), (1, 700, 2048)]


@pytest.mark.parametrize("neg_inf_row", [False, True], ids=["finite", "neg_inf_row"])
@pytest.mark.parametrize("B,M,N", DENSE_SHAPES)
def test_dense_match_decisions(gpu, B, M, N, neg_inf_row):
    """(a) planted ties, (b) both sides of the threshold, (c) non-mutual maxima, (d) a row of -inf (index 0 as torch.max
    gives, score 0 - the arg-max kernels clamp their "nothing compared greater" sentinel)."""
    import e2e_multi_view_matching_amd as E
    from oracle.sinkhorn import extract_matches
    Z, plants, expect = crafted_logZ(B, M, N, seed=7 * M + N, neg_inf_row=neg_inf_row)
    core = Z[:, :M, :N]
    # non-vacuity, counted on the tensor itself: every class that fits the shape is planted, and its rows / columns do
    # attain their maximum more than once
    fits = [f"col:{n}" for n, d, _ in COL_CLASSES if d < N] + [f"row:{n}" for n, d, _ in ROW_CLASSES if d < M]
    multi_rows = (core == core.max(2, keepdim=True).values).sum(2) > 1
    multi_cols = (core == core.max(1, keepdim=True).values).sum(1) > 1
    tied = {k: sum(int((multi_rows if k.startswith("col:") else multi_cols)[b, x]) for b, x in plants[k]) for k in fits}
    print(f"({B},{M},{N}) planted rows / columns with a tied maximum {tied}; in all {int(multi_rows.sum())} rows, {int(multi_cols.sum())} columns")
    for k in fits:
        assert tied[k] > 0, (k, tied)
    Zg = Z.to(gpu)
    for thr in (THR, 0.0):
        i0, i1, s0, s1 = extract_matches(Z, thr)
        m0, m1, ms0, ms1 = (t.cpu() for t in E.extract_matches(Zg, thr))
        # the planted outcomes, stated: the oracle agrees with the construction and the device with both
        wrong = set()
        for b, which, k, at_thr, at_zero, cls in expect:
            want = at_thr if thr == THR else at_zero
            assert int((i0 if which == "m0" else i1)[b, k]) == want, (cls, b, which, k, want, thr)
            if int((m0 if which == "m0" else m1)[b, k]) != want:
                wrong.add(cls)
        assert not wrong, (B, M, N, thr, "planted classes decided wrongly", sorted(wrong))
        assert torch.equal(m0, i0) and torch.equal(m1, i1), (B, M, N, thr, int((m0 != i0).sum()), int((m1 != i1).sum()))
        for a, r in ((ms0, s0), (ms1, s1)):
            assert float(((a - r).abs() / r.abs().clamp(min=1.0)).max()) < 2e-6
        if thr == 0.0:  # exp(z) > 0: every mutual pair of a finite row is a match
            assert torch.equal(m0 >= 0, s0 > 0)
        # (c) non-mutual maxima: matches1 follows valid0.gather, mscores1 follows mscores0.gather
        idx0, idx1 = core.max(2).indices, core.max(1).indices
        non_mutual = idx1.gather(1, idx0) != torch.arange(M)[None]
        if M >= 144 and N >= 144:
            assert int(non_mutual.sum()) > M // 4, int(non_mutual.sum())
        assert bool((m0[non_mutual] == -1).all()) and bool((ms0[non_mutual] == 0).all())
    if neg_inf_row:
        i = plants["neg_inf_row"]
        assert int(m0[0, i]) == -1 and float(ms0[0, i]) == 0.0
        assert bool((ms1[0][idx1[0] == i] == 0).all())


# ---------------------------------------------------------------------------------------------------------------- part 2
def planted_tuples(n0, n1, B, seed, T=2):
    """make_tuples, then keypoint + score + descriptor of chosen keypoints copied onto partners: in image 1 duplicate COLUMNS
    (j -> j+d, j the ground-truth match of a row i: row i's maximum is tied), in image 0 duplicate ROWS (r -> r+d, r matched to
    a column c: column c's maximum is tied).  -> (data, {class: [(b, row, col, d)]})."""
    from e2e_multi_view_matching_amd.synthetic import make_tuples
    N = max(n0, n1)
    data = make_tuples(batch=B, tuple_size=T, n_kpts=N, seed=seed)
    for m, n in ((0, n0), (1, n1)):
        data[f"keypoints{m}"] = data[f"keypoints{m}"][:, :n].contiguous()
        data[f"scores{m}"] = data[f"scores{m}"][:, :n].contiguous()
        data[f"descriptors{m}"] = data[f"descriptors{m}"][:, :, :n].contiguous()
    gt = data["gt_matches0_0_1"]
    rng = np.random.default_rng(seed)

    def copy(m, b, src, dst):
        data[f"keypoints{m}"][b, dst] = data[f"keypoints{m}"][b, src]
        data[f"scores{m}"][b, dst] = data[f"scores{m}"][b, src]
        data[f"descriptors{m}"][b, :, dst] = data[f"descriptors{m}"][b, :, src]

    plants = {}
    for b in range(B):
        u0, u1 = set(), set()
        pairs = [(int(i), int(gt[b, i])) for i in rng.permutation(n0) if 0 <= int(gt[b, i]) < n1]
        for name, d, ok in COL_CLASSES:
            got = plants.setdefault(f"col:{name}", [])
            k = 0
            for i, j in pairs:
                if k == 3:
                    break
                if j + d < n1 and not ({j, j + d} & u1) and i not in u0 and ok(j):
                    copy(1, b, j, j + d)
                    u1.update((j, j + d)), u0.add(i)
                    got.append((b, i, j, d))
                    k += 1
        for name, d, ok in ROW_CLASSES:
            got = plants.setdefault(f"row:{name}", [])
            k = 0
            for r, c in pairs:
                if k == 3:
                    break
                if r + d < n0 and not ({r, r + d} & u0) and c not in u1 and ok(r):
                    copy(0, b, r, r + d)
                    u0.update((r, r + d)), u1.add(c)
                    got.append((b, r, c, d))
                    k += 1
    return data, {k: v for k, v in plants.items() if v}


def count_ties(Z, plants):
    """{class: (plants whose two cells are bit-equal AND the maximum of their row / column, plants)} in the scores Z."""
    out = {}
    M, N = Z.shape[1] - 1, Z.shape[2] - 1
    for k, lst in plants.items():
        n = 0
        for b, i, j, d in lst:
            if k.startswith("col:"):
                n += bool(Z[b, i, j] == Z[b, i, j + d]) and bool(Z[b, i, j] == Z[b, i, :N].max())
            else:
                n += bool(Z[b, i, j] == Z[b, i + d, j]) and bool(Z[b, i, j] == Z[b, :M, j].max())
        out[k] = (n, len(lst))
    return out


@pytest.fixture(scope="module")
def matcher(gpu):
    import e2e_multi_view_matching_amd as E
    from e2e_multi_view_matching_amd.synthetic import identity_like_state
    torch.manual_seed(0)
    model = identity_like_state(E.MultiViewMatcher({"GNN_layers": ["self", "cross"], "conf_mlp": False, "full_output": True}).eval())
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    return model.to(gpu), sd


@functools.lru_cache(maxsize=None)
def _scene(n0, n1, T):
    B = 2 if max(n0, n1) <= 512 else 1
    return planted_tuples(n0, n1, B, seed=n0 + n1, T=T)


_REF = {}


def reference_scores(sd, n0, n1, T, iters):
    """the oracle's scores of every pair: once per (scene, iteration count), shared by the thresholds and arithmetic modes"""
    from oracle.matcher import matcher_forward
    key = (n0, n1, T, iters)
    if key not in _REF:
        data, _ = _scene(n0, n1, T)
        cfg = {"GNN_layers": ["self", "cross"], "conf_mlp": False, "sinkhorn_iterations": iters, "full_output": False,
               "tuple_size": T, "multi_frame_matching": T > 2}
        ref = matcher_forward(data, sd, cfg)
        _REF[key] = {k: v for k, v in ref.items() if k.startswith("scores_")}
    return _REF[key]


def _run_fused(gpu, matcher, n0, n1, T, iters, mode):
    from oracle.sinkhorn import extract_matches
    model, sd = matcher
    data, plants = _scene(n0, n1, T)
    ref = reference_scores(sd, n0, n1, T, iters)
    dev = {k: (v.to(gpu) if torch.is_tensor(v) else v) for k, v in data.items()}
    pairs = [(i, j) for j in range(T) for i in range(j)]
    ties = None
    for thr in (0.0, THR):
        model.config.update({"sinkhorn_iterations": iters, "match_threshold": thr, "mfma_precision": mode, "tuple_size": T,
                             "multi_frame_matching": T > 2})
        with torch.no_grad():
            out = model(dev)
        for i, j in pairs:
            Z = out[f"scores_{i}_{j}"].cpu()
            m0, m1 = out[f"matches{i}_{i}_{j}"].cpu(), out[f"matches{j}_{i}_{j}"].cpu()
            # the reference operation on the numbers the device produced
            i0, i1, _, _ = extract_matches(Z, thr)
            if not (torch.equal(m0, i0) and torch.equal(m1, i1)):
                wrong = sorted(k for k, lst in plants.items() for b, r, c, d in lst if (i, j) == (0, 1) and (
                    m0[b, r] != i0[b, r] or m1[b, c] != i1[b, c] or (k.startswith("row:") and m0[b, r + d] != i0[b, r + d])
                    or (k.startswith("col:") and m1[b, c + d] != i1[b, c + d])))
                raise AssertionError(((n0, n1), T, iters, mode, thr, (i, j), int((m0 != i0).sum()), int((m1 != i1).sum()),
                                      "planted classes decided wrongly", sorted(set(wrong))))
            dz = float((Z - ref[f"scores_{i}_{j}"]).abs().max())
            assert dz < 1e-4, ((n0, n1), T, iters, mode, (i, j), dz)
            if (i, j) == (0, 1) and ties is None:
                ties = count_ties(Z, plants)
                n_matched = int((m0 >= 0).sum())
    print(f"fused n0={n0} n1={n1} T={T} iters={iters} {mode}: ties/planted " + ", ".join(f"{k} {a}/{n}" for k, (a, n) in ties.items()) + f"; {n_matched} matched at thr 0")
    for name, d, _ in COL_CLASSES:  # every class the shape has room for is planted
        if d + (4 if name != "lane0_63" else 0) < n1:
            assert f"col:{name}" in plants, (name, n1)
    for name, d, _ in ROW_CLASSES:
        if d + 4 < n0:
            assert f"row:{name}" in plants, (name, n0)
    if mode == "f32" and iters == 0:  # identical inputs, identical arithmetic: every planted class ties exactly
        for k, (a, n) in ties.items():
            assert a > 0, (k, a, n)
    return ties


FUSED_SHAPES = [(200, 250), (256, 256), (300, 512), (640, 1000), (1024, 1024), (1100, 2048), (2048, 1500)]


@pytest.mark.usefixtures("split_always")
@pytest.mark.parametrize("mode", ["f32", "f16x2"])
@pytest.mark.parametrize("iters", [0, 20])
@pytest.mark.parametrize("n0,n1", FUSED_SHAPES)
def test_fused_match_decisions(gpu, matcher, n0, n1, iters, mode):
    """sinkhorn_sweep<KT, FINAL = true, FULL> + match_finalize behind the matcher: KT = 1, 2, 4, 8 by n1 <= 256, 512, 1024,
    2048, FULL at n1 = 256, 512, 1024, 2048; chunks = ceil(n0 / 16) from 13 to 128 (merge groups of 8 with remainders 4, 7, 2,
    7, 7, 4, 7)."""
    _run_fused(gpu, matcher, n0, n1, 2, iters, mode)


@pytest.mark.usefixtures("split_always")
@pytest.mark.parametrize("mode", ["f32", "f16x2"])
@pytest.mark.parametrize("iters", [0, 20])
def test_fused_match_decisions_three_views(gpu, matcher, iters, mode):
    """Two 3-tuples of 300 keypoints, multi-frame matching: six problems in three output groups (group_batch 2 < B 6), KT = 2
    with ragged tiles.  Every pair is checked; the planted ties are those of pair (0, 1)."""
    _run_fused(gpu, matcher, 300, 300, 3, iters, mode)
