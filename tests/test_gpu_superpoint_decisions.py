"""NMS, threshold, border and top-k decisions of the SuperPoint front-end, and its descriptor sampling (-m gpu):
csrc/superpoint.hip - sp_nms_kernel, sp_select_kernel, sp_sample_kernel - reached through the building-block entry
e2emv_superpoint_detect (superpoint.detect), which runs the tail of e2emv_superpoint_forward on a score map the test supplies.

NMS and selection consist of comparisons and copies of fp32 values: on the same input map the NMS-ed map, the keypoints, their
order, the scores and the counts must EQUAL those of oracle/superpoint.py (simple_nms, select_keypoints) - torch.equal, no
tolerance, no excluded share.  Random scores never tie, never sit on the threshold and never put a peak on a tile seam, so the
maps here are planted at the places where the kernels' geometry changes hands:

  sp_nms_kernel     32x32 tiles with an r-wide halo, -inf outside the image, five launches (two suppression rounds): equal maxima
                    inside one window (also across the seams x = 31|32, y = 31|32 and their corner); a lower peak at Chebyshev
                    distance r (suppressed) and r + 1 (kept) from a higher one that sits in the neighbouring tile, so that the
                    last halo column / row decides; peaks in the outermost rows, columns and corners; descending chains
                    0.9, 0.8, ... spaced 3 apart (r = 4), of which upstream's two rounds keep the 1st, 3rd and 5th and lose the
                    7th; constant, single-peak, random and quantised (plateau) maps; the oracle's own score map of an image
  sp_select_kernel  compaction in chunks of 1024, score > threshold (strict), the border band, 4-pass radix select, the ordered
                    pick of `want` equal scores carried over chunks, bitonic sort of (score, ~index) keys: scores at the
                    threshold and one ulp beside it; every border width; n = K - 1, K, K + 1 candidates; a group of equal
                    scores straddling rank K whose members lie in different chunks; all-equal maps; scores that differ only in
                    their lowest / highest byte; subnormal scores; batches whose images must not influence one another
  sp_sample_kernel  bilinear grid_sample(align_corners=True) with zero padding of the L2-normalised cells, renormalised:
                    keypoints in the corners and along the edges (part of the footprint is padding), next to cell centres, at
                    random pixels; an all-zero cell (the 1e-12 clamp); a map of one unit vector

Sizes: 16x16 (one partial tile), 40x72 (2x3 tiles with partial ones, 2880 pixels - no multiple of 1024), 64x64 (exact tiles, four
full chunks), 72x136 (9792 pixels: more than the capacity 4096, ten chunks).

Sampling is compared with sample_descriptors in fp64 on fp64-normalised cells.  The bar is the fp32 torch oracle's own distance
from fp64 on the same inputs (err32): err <= 4 * err32 + 1e-6 (a different, equally valid operation order, with a floor for
where err32 happens to be tiny), never above 1e-4.  Measured on the MI355X (test_sampling_against_fp64 prints them), max |error|
of a descriptor component against fp64, cells = Gaussian vectors of random scale (gauss | with all-zero cells):
  2x2 cells,   81 keypoints    device 3.5e-08 | 3.2e-08    fp32 torch oracle 8.0e-08 | 6.4e-08
  5x9 cells,  227 keypoints    device 9.5e-08 | 2.0e-07    fp32 torch oracle 1.2e-07 | 2.2e-07
  9x17 cells, 507 keypoints    device 2.1e-07 | 2.1e-07    fp32 torch oracle 2.0e-07 | 2.0e-07

test_planted_maps_hit_their_targets (no gpu mark) checks in the oracle alone that the planted maps produce the situations
they are meant to produce - a planting that misses its target fails there instead of passing here vacuously.

That these tests notice a wrong rule was checked against libraries built with one rule altered at a time.  Every such build
failed here; the tests that went red (the other groups' tests plant with threshold 0 on maps with zeros and with r = 0, so an
alteration of `>` or of the r = 0 pool reaches them too):
  `s > thr` -> `s >=`                     test_threshold_edges; and, the zeros of their maps becoming candidates at threshold 0,
                                          test_nms_planted, test_topk_n_against_K, test_topk_more_candidates..., test_topk_images...,
                                          test_sampling_*
  `y < H - border` -> `<=`                test_border_band (both sizes), test_nms_oracle_score_map (border 4 and 2); nothing else
  index term dropped from the sort key    every test that cuts (n > K): all test_topk_*, test_nms_planted[72-136-*],
                                          test_nms_oracle_score_map, test_threshold_*, test_border_band; no test without a cut
  eq_seen not accumulated                 test_topk_tie_group_across_chunks, test_topk_byte_patterns[low], [top] (run without the
                                          maps of more than 4096 candidates, where the altered kernel would leave its key array)
  row-max loop one element short          all but two tests (at r = 0 the pool becomes empty): every test_nms_planted case with
                                          r >= 1 among them
  a third suppression round               test_nms_planted at r = 1 and r = 4 (the chains and plateaus), test_nms_oracle_score_map,
                                          test_topk_more_candidates... (its r = 1 leg); nothing at r = 0
  three radix passes                      test_topk_byte_patterns[low16], [low], [top] (same restriction as eq_seen)
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import superpoint as OS

SIZES = ((16, 16), (40, 72), (64, 64), (72, 136))
RADII = (0, 1, 4, 16)
TILE, CHUNK, CAP = 32, 1024, 4096
KS = (1, 2, 3, 1000, 1024, 1025, 4096)
GRIDS = ((2, 2), (5, 9), (9, 17))


def _f32(x):
    return float(np.float32(x))


def _bits(u):
    return torch.from_numpy(np.asarray(u, dtype=np.uint32).view(np.float32).copy())


def _distinct(n, lo, hi, gen):
    """n distinct fp32 values in (lo, hi), in random order"""
    v = torch.linspace(lo, hi, n + 2, dtype=torch.float64)[1:-1].float()
    assert len(torch.unique(v)) == n
    return v[torch.randperm(n, generator=gen)]


# ------------------------------------------------------------------------------------------------------------ NMS plantings
def _seam(n):
    """(first pixel right of / below the seam that the plantings straddle): the tile seam, or the middle of a one-tile map"""
    return TILE if n > TILE else n // 2


@functools.lru_cache(maxsize=None)
def nms_cases(H, W):
    """-> (maps [B,H,W], meta): meta[i] = (kind, info) names what image i is to show.  The same maps run at every radius."""
    maps, meta = [], []

    def add(kind, info, pts, base=None):
        m = torch.zeros(H, W) if base is None else base.clone()
        for (y, x), v in pts:
            assert 0 <= y < H and 0 <= x < W, (kind, info, y, x)
            m[y, x] = v
        maps.append(m)
        meta.append((kind, info))

    sy, sx = _seam(H), _seam(W)
    add("single", None, [((H // 2, W // 3), 0.7)])
    add("constant", None, [], base=torch.full((H, W), 1.0 / 65.0))
    edge = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (0, W // 2), (H - 1, W // 2 - 1), (H // 2, 0), (H // 2 - 1, W - 1)]
    add("edges", tuple(edge), [(p, 0.9 - 0.1 * i) for i, p in enumerate(edge)])
    add("edges", tuple(edge), [(p, 0.2 + 0.1 * i) for i, p in enumerate(edge)])
    # two equal maxima inside one window: side by side, diagonal, across the seams, around the seam corner
    for a, b in (((5, 5), (5, 6)), ((5, 5), (6, 5)), ((5, 5), (6, 6)), ((5, 6), (6, 5)), ((5, sx - 1), (5, sx)), ((sy - 1, 5), (sy, 5)),
                 ((sy - 1, sx - 1), (sy, sx)), ((sy - 1, sx), (sy, sx - 1)), ((sy - 1, sx - 1), (sy - 1, sx)), ((sy - 1, sx - 1), (sy, sx - 1)),
                 ((sy, sx), (sy, sx + 1)), ((sy, sx), (sy + 1, sx))):
        add("tie", (a, b), [(a, 0.5), (b, 0.5)])
    # a lower peak at distance d from a higher one in the neighbouring tile, on either side of the seam, d = r and r + 1 for every
    # radius of RADII (at another radius the same image is one more map to agree on)
    for r in RADII[1:]:
        for d in (r, r + 1):
            for axis, (dy, dx) in (("x", (0, 1)), ("y", (1, 0)), ("diag", (1, 1))):
                for side in (-1, 1):  # the higher peak lies left of / above (-1) or right of / below (+1) the lower one
                    ly = (sy if side < 0 else sy - 1) if dy else 7
                    lx = (sx if side < 0 else sx - 1) if dx else 7
                    hy, hx = ly + side * d * dy, lx + side * d * dx
                    if 0 <= hy < H and 0 <= hx < W:
                        add("pair", (r, d, axis, side, (ly, lx), (hy, hx)), [((ly, lx), 0.8), ((hy, hx), 0.9)])
    # descending chains 0.9, 0.8, ... 0.1 spaced 3 apart: within a tile, across a seam, and descending towards the seam's other side
    if W >= 45:
        for axis, x0, step in (("x", 2, 3), ("x", 20, 3), ("x", 44, -3)):
            pos = tuple((12, x0 + step * k) for k in range(9))
            add("chain", pos, [(p, _f32(0.9 - 0.1 * k)) for k, p in enumerate(pos)])
    if H >= 40:
        y1 = 20 if H >= 45 else 11
        for axis, y0, step in (("y", 2, 3), ("y", y1, 3), ("y", y1 + 24, -3)):
            pos = tuple((y0 + step * k, 12) for k in range(9))
            add("chain", pos, [(p, _f32(0.9 - 0.1 * k)) for k, p in enumerate(pos)])
    g = torch.Generator().manual_seed(H * 1000 + W)
    add("random", None, [], base=torch.rand(H, W, generator=g))
    add("plateaus", None, [], base=torch.randint(0, 8, (H, W), generator=g).float() / 8.0)  # ties everywhere, also with 0
    add("plateaus", None, [], base=(torch.rand(H, W, generator=g) * 64).floor() / 64.0)
    return torch.stack(maps), tuple(meta)


@functools.lru_cache(maxsize=None)
def nms_reference(H, W, r):
    return OS.simple_nms(nms_cases(H, W)[0], r)


def nms_three_rounds(scores, r):
    """simple_nms with one suppression round more than upstream runs (premise test only: what the chains' 7th peak needs)"""
    mp = lambda x: F.max_pool2d(x, kernel_size=2 * r + 1, stride=1, padding=r)  # noqa: E731
    zeros = torch.zeros_like(scores)
    mask = scores == mp(scores)
    for _ in range(3):
        supp = mp(mask.float()) > 0
        ss = torch.where(supp, zeros, scores)
        mask = mask | ((ss == mp(ss)) & ~supp)
    return torch.where(mask, scores, zeros)


# ---------------------------------------------------------------------------------------------------------- top-k plantings
def sparse_map(H, W, n, gen, lo=0.1, hi=0.9):
    """n pixels at random places with distinct scores in (lo, hi), zeros elsewhere"""
    m = torch.zeros(H * W)
    m[torch.randperm(H * W, generator=gen)[:n]] = _distinct(n, lo, hi, gen)
    return m.view(H, W)


@functools.lru_cache(maxsize=None)
def n_against_K_case(K):
    """-> (maps [3,H,W] with K - 1, K and K + 1 candidates, H, W)"""
    H, W = (40, 72) if K <= 1025 else (72, 136)
    g = torch.Generator().manual_seed(K)
    return torch.stack([sparse_map(H, W, n, g) for n in (K - 1, K, K + 1)])


TIE_K, TIE_SCORE = 1024, 0.5
TIE_GROUP = (900, 950, 1000, 1023, 1024, 1025, 1500, 2047, 2048, 2500, 3071, 3072, 3500)
TIE_WANT = (1, 6, 10, 13)


@functools.lru_cache(maxsize=None)
def tie_group_case():
    """64x64, every pixel a candidate (4 chunks of 1024), K = 1024.  Image i: TIE_K - TIE_WANT[i] distinct scores above 0.5 at random
    pixels (many behind the group in index order), the 13 pixels of TIE_GROUP at exactly 0.5, distinct lower scores elsewhere: the
    cut takes the TIE_WANT[i] lowest-index members of the group."""
    H = W = 64
    g = torch.Generator().manual_seed(7)
    maps = []
    grp = torch.tensor(TIE_GROUP)
    for want in TIE_WANT:
        m = _distinct(H * W, 0.05, 0.45, g)
        rest = torch.tensor(sorted(set(range(H * W)) - set(TIE_GROUP)))
        hi = rest[torch.randperm(len(rest), generator=g)[:TIE_K - want]]
        m[hi] = _distinct(len(hi), 0.55, 0.95, g)
        m[grp] = TIE_SCORE
        maps.append(m.view(H, W))
    return torch.stack(maps)


@functools.lru_cache(maxsize=None)
def byte_pattern_case(which):
    """-> (maps [B,H,W], K).  low: bit patterns 0x3F0000xx (0.5 ...), only the fourth radix pass tells them apart - 256 distinct ones
    on 16x16 and, on 40x72, each of them 11 or 12 times.  top: patterns 0xtt345678, the first pass decides everything; tt = 0 is
    subnormal.  subnormal: subnormal and ordinary scores mixed, with ties among the subnormal ones."""
    g = torch.Generator().manual_seed(11)
    if which == "low16":
        return _bits(0x3F000000 + torch.randperm(256, generator=g).numpy()).view(1, 16, 16), 100
    if which == "low":
        lowbyte = (torch.randperm(2880, generator=g) % 256).numpy()
        return _bits(0x3F000000 + lowbyte).view(1, 40, 72), 1000
    if which == "top":
        top = (torch.randperm(2880, generator=g) % 128).numpy().astype(np.uint32)
        return _bits((top << 24) | 0x00345678).view(1, 40, 72), 1000
    assert which == "subnormal"
    u = torch.randint(1, 0x00800000, (2880,), generator=g).numpy().astype(np.uint32)  # subnormal patterns
    u[::3] = _distinct(960, 1e-3, 0.9, g).numpy().view(np.uint32)
    u[1::12] = 0x00000001  # the smallest positive number, many times
    u[5::12] = 0
    return _bits(u).view(1, 40, 72), 2000


# ----------------------------------------------------------------------------------------------------------- sampling inputs
@functools.lru_cache(maxsize=None)
def sampling_case(Hc, Wc, kind):
    """-> (score [1,H,W] with the keypoint pixels planted (r = 0, border 0: every planted pixel is a keypoint, row-major order),
    dense [1,256,Hc,Wc] unnormalised, zero cells [(cy, cx)])."""
    H, W = 8 * Hc, 8 * Wc
    g = torch.Generator().manual_seed(Hc * 100 + Wc)
    pix = {(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)}
    pix |= {(y, x) for y in (0, H - 1) for x in range(1, W, 3)} | {(y, x) for x in (0, W - 1) for y in range(1, H, 3)}
    pix |= {(8 * cy + o, 8 * cx + o) for cy in range(Hc) for cx in range(Wc) for o in (3, 4)}  # the pixels around a cell's centre
    pix |= {(int(y), int(x)) for y, x in zip(torch.randint(1, H - 1, (60,), generator=g), torch.randint(1, W - 1, (60,), generator=g))}
    pix = sorted(pix)
    assert len(pix) <= 1024
    score = torch.zeros(H, W)
    score[tuple(torch.tensor(pix).t())] = _distinct(len(pix), 0.1, 0.9, g)
    zero_cells = []
    if kind == "unit":
        u = F.normalize(torch.randn(256, generator=g), dim=0)
        dense = u.view(1, 256, 1, 1) * torch.exp(torch.randn(1, 1, Hc, Wc, generator=g))
    else:
        dense = torch.randn(1, 256, Hc, Wc, generator=g) * torch.exp(torch.randn(1, 1, Hc, Wc, generator=g))
        if kind == "zero_cell":
            zero_cells = [(0, 0)] + ([(Hc // 2, Wc // 2)] if Hc > 2 else [])
            for cy, cx in zero_cells:
                dense[0, :, cy, cx] = 0.0
    return score[None], dense, zero_cells


def sampling_references(score, dense):
    """-> (keypoints [n,2] (x, y), fp64 reference [256,n], fp32 torch oracle [256,n]) of image 0"""
    kp, _ = OS.select_keypoints(score[0], 0.0, 0, CAP)
    kxy = torch.flip(kp, [1])
    ref64 = OS.sample_descriptors(kxy.double()[None], F.normalize(dense.double(), p=2, dim=1), 8)[0]
    ref32 = OS.sample_descriptors(kxy.float()[None], F.normalize(dense, p=2, dim=1), 8)[0]
    return kxy.float(), ref64, ref32


# ------------------------------------------------------------------------------------------------- the ungated premise test
def test_planted_maps_hit_their_targets():
    """CPU, oracle only: every planting produces the situation it is named after."""
    for H, W in SIZES:
        maps, meta = nms_cases(H, W)
        kinds = [k for k, _ in meta]
        assert kinds.count("tie") == 12 and kinds.count("edges") == 2
        if min(H, W) > TILE:  # both seams exist: pairs on both sides of both seams and across the corner, chains in both directions
            for r in RADII[1:]:
                for axis in ("x", "y", "diag"):
                    sides = {(i[1], i[3]) for k, i in meta if k == "pair" and i[0] == r and i[2] == axis}
                    assert {(r, -1), (r + 1, -1)} <= sides and (r == 16 or {(r, 1), (r + 1, 1)} <= sides), (H, W, r, axis)
            assert kinds.count("chain") == 6
        for r in RADII[1:]:
            ref = nms_reference(H, W, r)
            for i, (kind, info) in enumerate(meta):
                if kind == "tie":  # both equal maxima survive
                    (a, b) = info
                    assert ref[i][a] == 0.5 and ref[i][b] == 0.5 and int((ref[i] > 0).sum()) == 2
                elif kind == "pair" and info[0] == r:  # suppressed at distance r, kept at r + 1; the higher one always stays
                    _, d, axis, side, lo, hi = info
                    assert max(abs(lo[0] - hi[0]), abs(lo[1] - hi[1])) == d
                    assert ref[i][hi] == _f32(0.9) and bool(ref[i][lo] > 0) == (d == r + 1), (H, W, info)
                    if min(H, W) > TILE:  # the higher peak lies in the neighbouring tile: the halo decides
                        assert any(lo[k] // TILE != hi[k] // TILE for k in (0, 1))
                elif kind == "chain" and r == 4:
                    kept = [bool(ref[i][p] > 0) for p in info]
                    assert len(info) >= 8 and kept[:7] == [True, False, True, False, True, False, False], (H, W, info, kept)
                    third = nms_three_rounds(maps[i][None], 4)[0]
                    assert bool(third[info[6]] > 0)  # a local maximum that only a third round would recover
                    if info[0][0] != info[-1][0]:
                        assert {p[0] // TILE for p in info} == {0, 1} or info[0][0] == 2
                    else:
                        assert {p[1] // TILE for p in info} == {0, 1} or info[0][1] == 2
                elif kind == "constant":
                    assert torch.equal(ref[i], maps[i])  # every pixel is a maximum
                elif kind == "single":
                    assert int((ref[i] > 0).sum()) == 1
    # threshold: the three neighbours of the threshold are three different numbers
    thr, up, down = threshold_values()
    assert down < thr < up and _f32(thr) == thr
    # n against K
    for K in KS:
        maps = n_against_K_case(K)
        for b, n in enumerate((K - 1, K, K + 1)):
            kp, sc = OS.select_keypoints(maps[b], 0.0, 0, K)
            idx = kp[:, 0] * maps.shape[2] + kp[:, 1]
            assert int((maps[b] > 0).sum()) == n and len(kp) == min(n, K)
            if n <= K:
                assert bool((idx[1:] > idx[:-1]).all())  # row-major
            else:  # score-descending: the K highest, the lowest one dropped
                assert torch.equal(sc, torch.sort(maps[b][maps[b] > 0], descending=True)[0][:K])
    # the tie group straddles rank K and the kept members span two chunks of the compaction
    maps = tie_group_case()
    for b, want in enumerate(TIE_WANT):
        flat = maps[b].flatten()
        assert int((flat > 0).sum()) == 64 * 64  # every pixel is a candidate: chunk of a candidate = pixel index // 1024
        assert int((flat > TIE_SCORE).sum()) == TIE_K - want and int((flat == TIE_SCORE).sum()) == len(TIE_GROUP)
        kp, sc = OS.select_keypoints(maps[b], 0.0, 0, TIE_K)
        idx = (kp[:, 0] * 64 + kp[:, 1])[sc == TIE_SCORE].tolist()
        assert idx == list(TIE_GROUP[:want]) and float(sc[-1]) == TIE_SCORE
        behind = torch.nonzero(flat > TIE_SCORE).flatten()
        assert int((behind > TIE_GROUP[-1]).sum()) > 50  # higher scores behind the whole group in index order
    assert any(0 < w < len(TIE_GROUP) and len({i // CHUNK for i in TIE_GROUP[:w]}) >= 2 for w in TIE_WANT)
    assert len({i // CHUNK for i in TIE_GROUP}) == 4
    # byte patterns
    for which in ("low16", "low"):
        u = byte_pattern_case(which)[0].numpy().view(np.uint32)
        assert len(np.unique(u >> 8)) == 1 and len(np.unique(u & 255)) == 256  # the upper 24 bits are shared
    u = byte_pattern_case("top")[0].numpy().view(np.uint32)
    assert len(np.unique(u & 0x00FFFFFF)) == 1 and len(np.unique(u >> 24)) == 128 and np.isfinite(u.view(np.float32)).all()
    m, K = byte_pattern_case("subnormal")
    tiny = np.finfo(np.float32).tiny
    sub = (m > 0) & (m < float(tiny))
    assert int(sub.sum()) > 1000 and int((m >= float(tiny)).sum()) == 960 and int((m > 0).sum()) > K  # the cut falls among subnormals
    kp, sc = OS.select_keypoints(m[0], 0.0, 0, K)
    assert float(sc[-1]) < float(tiny) and float(sc[-1]) > 0
    # sampling: the keypoints include the four corners, and the zero cell is hit
    for Hc, Wc in GRIDS:
        score, dense, zero_cells = sampling_case(Hc, Wc, "zero_cell")
        kxy, ref64, ref32 = sampling_references(score, dense)
        H, W = 8 * Hc, 8 * Wc
        have = {(int(x), int(y)) for x, y in kxy.tolist()}
        assert {(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1)} <= have and len(have) == len(kxy) == int((score > 0).sum())
        assert bool(torch.isfinite(ref64).all()) and int((ref64.norm(dim=0) < 0.5).sum()) >= 1  # a footprint of zeros and padding only


def threshold_values():
    thr = _f32(0.015)
    return thr, float(np.nextafter(np.float32(thr), np.float32(np.inf))), float(np.nextafter(np.float32(thr), np.float32(-np.inf)))


# --------------------------------------------------------------------------------------------------------------- GPU side
def _detect(gpu, score, dense=None, **cfg):
    from e2e_multi_view_matching_amd.superpoint import detect
    return detect(score.to(gpu), None if dense is None else dense.to(gpu), **cfg)


def _check_exact(out, score, r, thr, border, K, nms_ref=None):
    """NMS-ed map, counts, keypoints, order and scores equal the oracle's; the slots beyond each count are zero"""
    ref = OS.simple_nms(score, r) if nms_ref is None else nms_ref
    smap = out["score_map"].cpu()
    assert torch.equal(smap, ref), f"NMS map differs at {int((smap != ref).sum())} pixels, first {torch.nonzero(smap != ref)[:4].tolist()}"
    kpts, scores, count, desc = (t.cpu() if t is not None else None for t in out["raw"])
    for b in range(score.shape[0]):
        kp, sc = OS.select_keypoints(ref[b], thr, border, K)
        n = len(kp)
        assert int(count[b]) == n, (b, int(count[b]), n)
        assert torch.equal(out["keypoints"][b].cpu(), torch.flip(kp, [1]).float()), f"image {b}: keypoints or their order differ"
        assert torch.equal(out["scores"][b].cpu(), sc), f"image {b}: scores differ"
        assert not kpts[b, n:].any() and not scores[b, n:].any()
        if desc is not None:
            assert not desc[b, :, n:].any()


@pytest.mark.gpu
@pytest.mark.parametrize("r", RADII)
@pytest.mark.parametrize("H,W", SIZES)
def test_nms_planted(gpu, H, W, r):
    maps, _ = nms_cases(H, W)
    out = _detect(gpu, maps, nms_radius=r, keypoint_threshold=0.0, remove_borders=0, max_keypoints=CAP)
    _check_exact(out, maps, r, 0.0, 0, CAP, nms_reference(H, W, r))


@pytest.mark.gpu
def test_nms_oracle_score_map(gpu):
    """The oracle's own pre-NMS fp32 score map of a seeded image: both stages on realistic data, with no allowance."""
    g = torch.Generator().manual_seed(5)
    img = torch.rand(2, 1, 120, 160, generator=g)
    img = F.avg_pool2d(F.pad(img, (2, 2, 2, 2), mode="reflect"), 5, 1)
    score, _ = OS.dense_maps(OS.seeded_state(0), img)
    thr = _f32(0.005)
    for r, border, K in ((4, 4, CAP), (3, 0, 256), (1, 2, 1000)):
        out = _detect(gpu, score, nms_radius=r, keypoint_threshold=thr, remove_borders=border, max_keypoints=K)
        _check_exact(out, score, r, thr, border, K)
        assert all(len(k) > 100 for k in out["keypoints"])


@pytest.mark.gpu
def test_threshold_edges(gpu):
    """score > threshold, strictly: the threshold itself and its lower neighbour are excluded, its upper neighbour is kept"""
    thr, up, down = threshold_values()
    m = torch.zeros(1, 16, 16)
    m[0, 3, 4], m[0, 3, 9], m[0, 8, 2], m[0, 12, 12], m[0, 15, 15], m[0, 0, 0] = thr, up, down, 0.5, up, thr
    out = _detect(gpu, m, nms_radius=0, keypoint_threshold=thr, remove_borders=0, max_keypoints=CAP)
    _check_exact(out, m, 0, thr, 0, CAP)
    assert out["keypoints"][0].cpu().tolist() == [[9.0, 3.0], [12.0, 12.0], [15.0, 15.0]]
    full = torch.full((1, 40, 72), thr)  # a whole map on the threshold, a few pixels one ulp above: chunks 0, 1 and 2
    for i in (0, 1023, 1024, 2047, 2879):
        full.view(-1)[i] = up
    for K in (CAP, 3):
        out = _detect(gpu, full, nms_radius=0, keypoint_threshold=thr, remove_borders=0, max_keypoints=K)
        _check_exact(out, full, 0, thr, 0, K)
        assert int(out["raw"][2][0]) == min(K, 5)


@pytest.mark.gpu
def test_threshold_negative_keeps_zeros(gpu):
    """upstream's score_map > threshold with a negative threshold keeps the zeros, as candidates of score 0 (lowest index first)"""
    g = torch.Generator().manual_seed(3)
    m = torch.stack([torch.zeros(16, 16), sparse_map(16, 16, 40, g), torch.zeros(16, 16)])
    for K in (CAP, 256, 100, 30):
        out = _detect(gpu, m, nms_radius=0, keypoint_threshold=-0.5, remove_borders=0, max_keypoints=K)
        _check_exact(out, m, 0, -0.5, 0, K)
        assert out["raw"][2].tolist() == [min(K, 256)] * 3


@pytest.mark.gpu
@pytest.mark.parametrize("H,W", SIZES[:2])
def test_border_band(gpu, H, W):
    """Every pixel is a candidate (r = 0, distinct positive scores), so the band y, x in [border, size - border) is tested at each
    of its pixels: border - 1, border, size - border - 1, size - border and all others; border 0; bands that are empty."""
    g = torch.Generator().manual_seed(H)
    m = _distinct(H * W, 0.1, 0.9, g).view(1, H, W)
    for border in (0, 1, 2, 4, 7, H // 2 - 1, H // 2, H // 2 + 1, H, 1000):
        for K in (CAP, 50):
            out = _detect(gpu, m, nms_radius=0, keypoint_threshold=0.0, remove_borders=border, max_keypoints=K)
            _check_exact(out, m, 0, 0.0, border, K)
            band = max(H - 2 * border, 0) * max(W - 2 * border, 0)
            assert int(out["raw"][2][0]) == min(band, K)
            if band == 0:
                assert not any(bool(t.any()) for t in out["raw"][:3])


@pytest.mark.gpu
@pytest.mark.parametrize("K", KS)
def test_topk_n_against_K(gpu, K):
    """K - 1 and K candidates come out in row-major order, K + 1 score-descending with the lowest dropped"""
    maps = n_against_K_case(K)
    out = _detect(gpu, maps, nms_radius=0, keypoint_threshold=0.0, remove_borders=0, max_keypoints=K)
    _check_exact(out, maps, 0, 0.0, 0, K)
    assert out["raw"][2].tolist() == [K - 1, K, K]


@pytest.mark.gpu
def test_topk_tie_group_across_chunks(gpu):
    maps = tie_group_case()
    out = _detect(gpu, maps, nms_radius=0, keypoint_threshold=0.0, remove_borders=0, max_keypoints=TIE_K)
    _check_exact(out, maps, 0, 0.0, 0, TIE_K)
    for b, want in enumerate(TIE_WANT):  # said once more without the oracle: the lowest-index `want` of the group, in index order, last
        tail = out["keypoints"][b][TIE_K - want:].cpu()
        assert (tail[:, 1] * 64 + tail[:, 0]).tolist() == [float(i) for i in TIE_GROUP[:want]]


@pytest.mark.gpu
@pytest.mark.parametrize("H,W", SIZES)
def test_topk_all_equal(gpu, H, W):
    """A constant map: every pixel ties, the first K pixel indices are kept (72x136: 9792 candidates for the capacity 4096)"""
    m = torch.full((2, H, W), 1.0 / 65.0)
    m[1] = 0.25
    for K in sorted({1, 255, min(CAP, H * W - 1), CAP}):
        out = _detect(gpu, m, nms_radius=0, keypoint_threshold=0.0, remove_borders=0, max_keypoints=K)
        _check_exact(out, m, 0, 0.0, 0, K)
        n = min(K, H * W)
        kp = out["keypoints"][1].cpu()
        assert torch.equal(kp[:, 1] * W + kp[:, 0], torch.arange(n).float())


@pytest.mark.gpu
@pytest.mark.parametrize("which", ("low16", "low", "top", "subnormal"))
def test_topk_byte_patterns(gpu, which):
    maps, K = byte_pattern_case(which)
    for k in (K, K // 2 + 1, 1):
        out = _detect(gpu, maps, nms_radius=0, keypoint_threshold=0.0, remove_borders=0, max_keypoints=k)
        _check_exact(out, maps, 0, 0.0, 0, k)


@pytest.mark.gpu
def test_topk_more_candidates_than_capacity_72x136(gpu):
    g = torch.Generator().manual_seed(21)
    m = torch.stack([_distinct(72 * 136, 0.01, 0.99, g).view(72, 136), (torch.rand(72, 136, generator=g) * 512).floor() / 512 + 1 / 1024])
    for r in (0, 1):
        out = _detect(gpu, m, nms_radius=r, keypoint_threshold=0.0, remove_borders=0, max_keypoints=CAP)
        _check_exact(out, m, r, 0.0, 0, CAP)
    assert out["raw"][2].tolist()[0] < CAP  # (r = 1 leaves fewer than the capacity on the distinct map; r = 0 filled it)


@pytest.mark.gpu
def test_topk_images_do_not_influence_one_another(gpu):
    """B = 3: a full image, an image without a candidate, an image with exactly K; and each alone gives what it gave in the batch"""
    K, H, W = 1000, 40, 72
    g = torch.Generator().manual_seed(4)
    m = torch.stack([_distinct(H * W, 0.1, 0.9, g).view(H, W), torch.zeros(H, W), sparse_map(H, W, K, g)])
    _, dense, _ = sampling_case(5, 9, "gauss")
    dense = dense.expand(3, -1, -1, -1).contiguous()
    cfg = dict(nms_radius=0, keypoint_threshold=0.0, remove_borders=0, max_keypoints=K)
    out = _detect(gpu, m, dense, **cfg)
    _check_exact(out, m, 0, 0.0, 0, K)
    assert out["raw"][2].tolist() == [K, 0, K]
    for order in ((2, 1, 0), (1,), (0,)):
        alone = _detect(gpu, m[list(order)], dense[list(order)], **cfg)
        for i, b in enumerate(order):
            for a, c in zip(alone["raw"], out["raw"]):
                assert torch.equal(a[i], c[b])
    again = _detect(gpu, m, dense, **cfg)  # two runs: bit-identical outputs, descriptors included
    assert all(torch.equal(a, c) for a, c in zip(again["raw"], out["raw"])) and torch.equal(again["score_map"], out["score_map"])


@pytest.mark.gpu
@pytest.mark.parametrize("Hc,Wc", GRIDS)
@pytest.mark.parametrize("kind", ("gauss", "zero_cell"))
def test_sampling_against_fp64(gpu, Hc, Wc, kind):
    score, dense, zero_cells = sampling_case(Hc, Wc, kind)
    kxy, ref64, ref32 = sampling_references(score, dense)
    out = _detect(gpu, score, dense, nms_radius=0, keypoint_threshold=0.0, remove_borders=0, max_keypoints=1024)
    _check_exact(out, score, 0, 0.0, 0, 1024)
    assert torch.equal(out["keypoints"][0].cpu(), kxy)
    de = out["descriptors"][0].cpu()
    assert bool(torch.isfinite(de).all())
    err32 = float((ref32.double() - ref64).abs().max())
    err = float((de.double() - ref64).abs().max())
    print(f"sampling {Hc}x{Wc} {kind}: device {err:.2e}, fp32 oracle {err32:.2e} (max |error| against fp64, {len(kxy)} keypoints)")
    assert err <= 4 * err32 + 1e-6 and err <= 1e-4, (err, err32)
    nz = ref64.norm(dim=0) > 0.5  # (a footprint made of all-zero cells and padding gives the zero vector in the oracle too)
    assert bool(nz.all()) == (not zero_cells)
    assert float((de[:, nz].double().norm(dim=0) - 1).abs().max()) <= 1e-6
    assert not de[:, ~nz].any()


@pytest.mark.gpu
@pytest.mark.parametrize("Hc,Wc", GRIDS)
def test_sampling_constant_unit_vector(gpu, Hc, Wc):
    """Every cell holds a multiple of one unit vector: the bilinear weights - zero padding included - cancel in the renormalisation"""
    score, dense, _ = sampling_case(Hc, Wc, "unit")
    u = F.normalize(dense[0, :, 0, 0].double(), dim=0)
    out = _detect(gpu, score, dense, nms_radius=0, keypoint_threshold=0.0, remove_borders=0, max_keypoints=1024)
    de = out["descriptors"][0].cpu().double()
    assert de.shape[1] == int((score > 0).sum())
    assert float((de - u[:, None]).abs().max()) <= 1e-6


@pytest.mark.gpu
def test_detect_argument_checks(gpu):
    from e2e_multi_view_matching_amd import _lib
    ok = torch.rand(1, 16, 24)
    assert len(_detect(gpu, ok, max_keypoints=5)["keypoints"][0]) <= 5
    for bad, cfg in ((torch.rand(1, 8, 24), {}), (torch.rand(1, 20, 24), {}), (ok, {"nms_radius": 17}), (ok, {"nms_radius": -1}), (ok, {"remove_borders": -1})):
        with pytest.raises(_lib.E2EMVError):
            _detect(gpu, bad, **cfg)
    with pytest.raises(ValueError):
        _detect(gpu, ok, max_keypoints=CAP + 1)
    with pytest.raises(AssertionError):
        _detect(gpu, ok, torch.rand(1, 256, 3, 3))
    with pytest.raises(RuntimeError):
        from e2e_multi_view_matching_amd.superpoint import detect
        detect(ok)  # CPU tensor: no fallback
