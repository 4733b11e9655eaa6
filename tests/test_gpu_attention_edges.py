"""The attention kernels at ragged tuples and key-tile edges (-m gpu), against the fp64 reference of
tests/attention_restatement.py (itself pinned on the CPU by tests/test_attention_reference.py).

Every launcher sizes three things from the per-image keypoint counts nv[t]: the 64-key tiles of each source image, the early
exit of query tiles and the walk from one source of a cross layer to the next.  The stand-alone entry points take the counts
through ``n_valid`` as a sequence (``e2emv_attention_v``, ``e2emv_attention_bf16x3_v``, ``e2emv_attention_p2_v``), so each
kernel runs here on its own: counts of 1, counts on and around every multiple of 32 / 64 / 128 / 256, a one-key source between
long ones, sources that end exactly on a tile boundary, the key-split parts of attention_p2w over sources of different length,
and padding rows filled with keys that would dominate the softmax if one were read.

Bars are the ones of tests/test_gpu_kernels.py and tests/test_gpu_planes.py: max |out - fp64| over valid rows < 2e-5 and, for the
split-operand kernels, < 3 err32 + 1e-6 with err32 the error of the fp32 kernel on the same input; key split against no key
split < 8e-6.  Each test prints its figures before it asserts; the last test prints the worst per kernel."""
import functools

import pytest
import torch

import attention_restatement as ar

pytestmark = pytest.mark.gpu

D, H = 256, 4
BAR = 2e-5
SPLIT_BAR = 8e-6

# the nine ways to a kernel: fp32; bf16x3 planes / fused / its f16x2 form; the plane kernels by key count, with 4 and 8 waves;
# attention_p2w without and with its key split
SELECTIONS = ["attention", "planes", "fused", "f16x2", "p2-auto", "p2-4w", "p2-8w", "p2w-whole", "p2w-split"]
NO_BLOCK_EXPONENTS = ("attention", "planes", "fused", "f16x2")  # operands rounded element by element: a masked key cannot move a bit

UNIFORM = [1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257]
RAGGED_T2 = [(1, 128), (128, 1), (33, 200), (257, 64), (300, 513)]
RAGGED_T3 = [(65, 1, 257), (64, 128, 192), (63, 130, 5), (300, 513, 64)]
RAGGED = [(2, nv) for nv in RAGGED_T2 + RAGGED_T3 + [(1, 64, 65, 300, 129)]] + [(1, (70, 1, 64, 129, 33, 200, 2, 65))]  # (B, nv)
KEY_SPLIT = [((577, 70, 300), 1), ((130, 577, 64), 1), ((1000, 300), 0)]  # (nv, cross), B = 1

WORST = {}  # selection -> largest error over valid rows in the accuracy tests (cases 1 to 3)


def _n_rows(nv):
    return (max(nv) + 127) // 128 * 128


@functools.lru_cache(maxsize=2)
def _case(B, nv, cross):
    """(qkv, fp64 reference) of a case: made once, shared by the selections (which pytest runs back to back), never modified."""
    T = len(nv)
    g = torch.Generator().manual_seed(1000 * T + sum(nv) + cross)
    qkv = torch.randn(B * T, _n_rows(nv), 3 * D, generator=g) * 1.5
    return qkv, ar.attention_ref(qkv, B, T, nv, H, cross)


_ERR32 = {}


def _err32(gpu, B, nv, cross):
    key = (B, nv, cross)
    if key not in _ERR32:
        qkv, ref = _case(B, nv, cross)
        _ERR32[key] = ar.valid_error(_run("attention", qkv.to(gpu), B, nv, cross).cpu(), ref, len(nv), nv)
    return _ERR32[key]


def _run(sel, qkv, B, nv, cross, key_split=None):
    """One call of a selection on device tensor qkv.  nv: an int (the uniform entry point) or a tuple (the per-image one).
    key_split: None = the context's default (on), except for the two p2w selections, which are the split off / on."""
    import e2e_multi_view_matching_amd as E
    from e2e_multi_view_matching_amd import _lib
    T = qkv.shape[0] // B
    n = nv if isinstance(nv, int) else list(nv)
    if sel == "attention":
        return E.attention(qkv, B, T, n, H, cross)
    if sel in ("planes", "fused", "f16x2"):
        return E.attention_bf16x3(qkv, B, T, n, H, cross, kernel=sel)
    waves = {"p2-auto": 0, "p2-4w": 4, "p2-8w": 8, "p2w-whole": 1, "p2w-split": 1}[sel]
    if sel.startswith("p2w"):
        key_split = sel == "p2w-split"
    if key_split is None:
        return E.attention_p2(qkv, B, T, n, H, cross, waves=waves)
    ctx = _lib.context(qkv.device)
    try:
        ctx.set_attention_key_split(key_split)
        return E.attention_p2(qkv, B, T, n, H, cross, waves=waves)
    finally:
        ctx.set_attention_key_split(True)


def _check_accuracy(gpu, sel, B, nv, cross, out=None, tag=""):
    T = len(nv)
    qkv, ref = _case(B, nv, cross)
    if out is None:
        out = _run(sel, qkv.to(gpu), B, nv, cross).cpu()
    for g in range(B * T):
        assert bool(torch.isfinite(out[g, :nv[g % T]]).all()), (sel, nv, g)
    err, err32 = ar.valid_error(out, ref, T, nv), _err32(gpu, B, nv, cross)
    WORST[sel] = max(WORST.get(sel, 0.0), err)
    print(f"attention-edges {tag} {sel} B={B} nv={nv} cross={cross}: err {err:.3e} err32 {err32:.3e}")
    assert err < BAR, (sel, nv, cross, err)
    if sel != "attention":
        assert err < 3 * err32 + 1e-6, (sel, nv, cross, err, err32)
    return out


# ---------------------------------------------------------------------------------------------- 1. uniform counts at every tile edge
@pytest.mark.parametrize("cross", [0, 1])
@pytest.mark.parametrize("n_valid", UNIFORM)
@pytest.mark.parametrize("sel", SELECTIONS)
def test_uniform_counts_at_every_tile_edge(gpu, sel, n_valid, cross):
    """One key (a softmax over one element), 32 | 33 (whether the second 32-key half of a tile runs), a last key tile of 1 and of
    63 keys, a query tile with one valid row; through the uniform entry point and, bit for bit the same, the per-image one."""
    nv = (n_valid, n_valid)
    qkv, _ = _case(1, nv, cross)
    dev = qkv.to(gpu)
    out = _run(sel, dev, 1, n_valid, cross).cpu()
    _check_accuracy(gpu, sel, 1, nv, cross, out=out, tag="uniform")
    out_v = _run(sel, dev, 1, nv, cross).cpu()
    assert torch.equal(out_v[:, :n_valid], out[:, :n_valid])


# ---------------------------------------------------------------------------------------------- 2. ragged tuples
@pytest.mark.parametrize("cross", [0, 1])
@pytest.mark.parametrize("B,nv", RAGGED)
@pytest.mark.parametrize("sel", SELECTIONS)
def test_ragged_tuples(gpu, sel, B, nv, cross):
    """Per-image counts: a one-key source before, between and after long ones, sources that end exactly on a 64-key tile, images
    without queries in the later query tiles, T = 2 .. 8 (T > 2, cross: the source-to-source walk), two tuples per call."""
    _check_accuracy(gpu, sel, B, nv, cross, tag="ragged")


# ---------------------------------------------------------------------------------------------- 3. ragged tuples through the key-split parts
def _p2w_parts(cus, B, nv, cross):
    """Parts per leftover item of launch_attention_p2w (attention_p2w.hip), restated: items of 256 queries per (image, head),
    r = items beyond whole rounds of CUs; r <= half a round and a multiple of 8 -> min(CUs / r, 8, fewest key tiles of an item)."""
    T = len(nv)
    n_items = 8 * ((B * T * H + 7) // 8) * ((max(nv) + 255) // 256)
    cus = max(8, cus // 8 * 8)
    r = n_items % cus
    min_tiles = min(sum((nv[s] + 63) // 64 for s in range(T) if (s != t if cross else s == t)) for t in range(T))
    return min(cus // r, 8, min_tiles) if r > 0 and 2 * r <= cus and r % 8 == 0 else 1


@pytest.mark.parametrize("nv,cross", KEY_SPLIT)
def test_ragged_tuples_through_the_key_split_parts(gpu, nv, cross):
    """attention_p2w's parts find their first tile by walking t0 tiles across the sources, and attention_p2w_combine derives the
    same tile count from nv again: sources of different length (the fewest-tiles item of (577, 70, 300) walks 7 tiles over two
    sources in 5 parts on 256 CUs; its image 1 has no queries in query tiles 1 and 2)."""
    parts = _p2w_parts(torch.cuda.get_device_properties(gpu).multi_processor_count, 1, nv, cross)
    assert parts >= 2, (nv, parts)  # precondition: the shape reaches the parts on this device
    whole = _check_accuracy(gpu, "p2w-whole", 1, nv, cross, tag="key-split")
    split = _check_accuracy(gpu, "p2w-split", 1, nv, cross, tag="key-split")
    d = ar.valid_error(split, whole, len(nv), nv)
    print(f"attention-edges key-split nv={nv} cross={cross}: {parts} parts, split - whole {d:.3e}")
    assert d < SPLIT_BAR, (nv, d)


# ---------------------------------------------------------------------------------------------- 3b. the fp32 kernel's key split
def _attention_parts(cus, B, nv, cross):
    """(ks, [per image t: the (first, last + 1) key tile of each part]) of launch_attention (attention.hip), restated: workgroups of
    128 queries per (image, head); fewer than half the CUs busy -> min(CUs / workgroups, 8, fewest key tiles of an image) parts,
    part sp of an image with n tiles walks [n sp / ks, n (sp + 1) / ks)."""
    T = len(nv)
    tiles = [sum((nv[s] + 63) // 64 for s in range(T) if (s != t if cross else s == t)) for t in range(T)]
    blocks = B * T * H * ((max(nv) + 127) // 128)
    ks = max(1, min(cus // blocks if blocks * 2 <= cus else 1, 8, min(tiles)))
    return ks, [[(n * sp // ks, n * (sp + 1) // ks) for sp in range(ks)] for n in tiles]


# (nv, image t, tile a part must begin on, (source image, tile inside it) of that tile)
ATTENTION_KEY_SPLIT = [((128, 64, 192), 0, 1, (2, 0)),   # t = 0: sources of 1 + 3 tiles; a part begins on the first tile of the second
                       ((64, 320, 64), 0, 3, (1, 3))]    # t = 0: sources of 5 + 1 tiles; a part begins in the middle of the first


@pytest.mark.parametrize("nv,t,tile,where", ATTENTION_KEY_SPLIT)
def test_fp32_key_split_parts_begin_inside_the_walk(gpu, nv, t, tile, where):
    """attention_kernel<SPLIT> finds the first tile of a part by a search over the sources and walks on from there with the
    cursor the other kernels use: a part that begins exactly where a source begins, and one that begins inside a source."""
    ks, parts = _attention_parts(torch.cuda.get_device_properties(gpu).multi_processor_count, 1, nv, 1)
    print(f"attention-edges fp32 key split nv={nv}: {ks} parts, image {t}: {parts[t]}")
    # precondition: on this device a part of image t begins on the tile the case is about (not on tile 0)
    assert ks >= 2 and tile > 0 and tile in [lo for lo, _ in parts[t]], (nv, ks, parts[t])
    sources = [(s, k) for s in range(len(nv)) if s != t for k in range((nv[s] + 63) // 64)]
    assert sources[tile] == where, (nv, sources)
    _check_accuracy(gpu, "attention", 1, nv, 1, tag="fp32-key-split")


# ---------------------------------------------------------------------------------------------- 4. padding rows cannot leak
def _padded(qkv, nv, fill, seed):
    """qkv with the rows at and beyond nv[t] of every image zeroed (fill = 0) or made hostile (fill = 1): q and v a fresh draw of
    the data's magnitude, key row j a copy of query row j mod nv[t] of the same image - read as a key it meets that query at a logit
    of |q_head|^2 / 8, about 18 against a spread of 2.25 of the real logits, and takes over its softmax.  fill = 2: the hostile k
    and v over zero q rows."""
    T = len(nv)
    x = qkv.clone()
    g = torch.Generator().manual_seed(seed)
    for img in range(x.shape[0]):
        n = nv[img % T]
        if n == x.shape[1]:
            continue
        if not fill:
            x[img, n:] = 0
            continue
        x[img, n:] = torch.randn(x.shape[1] - n, 3 * D, generator=g) * 1.5
        x[img, n:, D:2 * D] = x[img, torch.arange(n, x.shape[1]) % n, :D]
        if fill == 2:
            x[img, n:, :D] = 0
    return x


@pytest.mark.parametrize("cross", [0, 1])
@pytest.mark.parametrize("nv", RAGGED_T2 + RAGGED_T3)
@pytest.mark.parametrize("sel", SELECTIONS)
def test_padding_rows_cannot_leak(gpu, sel, nv, cross):
    """The same valid rows over zero padding and over hostile padding: both inside the fp64 bar; bit-identical where operands
    are rounded element by element (the plane kernels share a 64-row tile exponent with their padding rows, so their bits may
    move - by rounding, inside the bar); the fp32 kernel leaves zeros at and beyond nv[t] of an output that started as zeros.

    "f16x2" (attention_h2f_kernel) is bit-identical over hostile keys and values, but not over hostile QUERY rows: its running
    maximum is lazy, and whether a tile moves it is decided for the whole wave (a ballot over the wave's 32 queries, padding
    queries included).  A padding query whose logits outgrow its maximum by 2^5 makes the valid queries of its wave take
    max(m, own maximum) as their reference a tile earlier than they would have: the same softmax, p rounded at another power
    of two (measured: the error against fp64 is the same to four digits in both runs, 14 of 18 cases differ in bits).  No key
    is read: so for this kernel the bits are compared over hostile k and v with zero q rows, the fp64 bar over all three."""
    B, T = 2, len(nv)
    qkv, ref = _case(B, nv, cross)
    outs = {}
    for fill in (0, 1, 2) if sel == "f16x2" else (0, 1):
        out = _run(sel, _padded(qkv, nv, fill, 77 + sum(nv)).to(gpu), B, nv, cross).cpu()
        err = ar.valid_error(out, ref, T, nv)
        print(f"attention-edges padding fill={fill} {sel} nv={nv} cross={cross}: err {err:.3e}")
        assert err < BAR, (sel, nv, cross, fill, err)
        if sel == "attention":
            for g in range(B * T):
                assert not out[g, nv[g % T]:].any(), (nv, cross, fill, g)
        outs[fill] = out
    if sel in NO_BLOCK_EXPONENTS:
        hostile = outs[2 if sel == "f16x2" else 1]
        for g in range(B * T):
            assert torch.equal(outs[0][g, :nv[g % T]], hostile[g, :nv[g % T]]), (sel, nv, cross, g)


# ---------------------------------------------------------------------------------------------- 5. fixed order
ORDER_NV = (65, 1, 257)


@pytest.mark.parametrize("cross", [0, 1])
@pytest.mark.parametrize("sel", SELECTIONS)
def test_a_second_call_returns_the_same_bits(gpu, sel, cross):
    qkv, _ = _case(2, ORDER_NV, cross)
    dev = qkv.to(gpu)
    first, second = _run(sel, dev, 2, ORDER_NV, cross).cpu(), _run(sel, dev, 2, ORDER_NV, cross).cpu()
    for g in range(6):
        assert torch.equal(first[g, :ORDER_NV[g % 3]], second[g, :ORDER_NV[g % 3]]), (sel, cross, g)


@pytest.mark.parametrize("cross", [0, 1])
@pytest.mark.parametrize("sel", [s for s in SELECTIONS if s != "p2w-split"])
def test_a_tuple_does_not_depend_on_its_batch_neighbour(gpu, sel, cross):
    """With attention_p2w's key split off (its part count follows the number of items of the call), tuple b of a two-tuple call is
    the same tuple run alone, bit for bit: img / T and img % T address the right images and nothing crosses a tuple."""
    qkv, _ = _case(2, ORDER_NV, cross)
    dev = qkv.to(gpu)
    both = _run(sel, dev, 2, ORDER_NV, cross, key_split=False).cpu()
    for b in range(2):
        alone = _run(sel, dev[3 * b:3 * b + 3].contiguous(), 1, ORDER_NV, cross, key_split=False).cpu()
        for t in range(3):
            assert torch.equal(both[3 * b + t, :ORDER_NV[t]], alone[t, :ORDER_NV[t]]), (sel, cross, b, t)


# ---------------------------------------------------------------------------------------------- 6. errors, not launches
ENTRY_POINTS = [("attention", "e2emv_attention_v"), ("planes", "e2emv_attention_bf16x3_v"), ("p2-auto", "e2emv_attention_p2_v")]


@pytest.mark.parametrize("sel,symbol", ENTRY_POINTS)
def test_bad_counts_are_errors_and_the_context_stays_usable(gpu, sel, symbol):
    import ctypes
    from e2e_multi_view_matching_amd import _lib
    nv = (65, 1, 128)
    qkv, ref = _case(1, nv, 1)
    dev = qkv.to(gpu)
    for bad in ((65, 0, 128), (0, 1, 128), (65, 1, 129), (65, 1, -3)):  # 0 and n_rows + 1, first, middle and last image
        with pytest.raises(_lib.E2EMVError) as e:
            _run(sel, dev, 1, bad, 1)
        assert e.value.code == _lib.ESHAPE, (bad, str(e.value))
    with pytest.raises(ValueError):
        _run(sel, dev, 1, (65, 1), 1)  # two counts for three images: refused before the library is called
    # a NULL array, and more images than E2EMV_MAX_TUPLE (before the array would be read past its end)
    ctx = _lib.context(gpu)
    out = torch.zeros(3, 128, D, device=gpu)
    counts = (ctypes.c_int * 3)(*nv)
    fn = getattr(ctx.lib, symbol)
    with torch.cuda.device(gpu):
        sp = _lib.stream_ptr(gpu)
        assert fn(ctx.h, 1, 3, 128, None, D, H, _lib.ptr(dev), 1, _lib.ptr(out), sp) == _lib.EINVAL
        assert fn(ctx.h, 1, 9, 128, counts, D, H, _lib.ptr(dev), 1, _lib.ptr(out), sp) in (_lib.EINVAL, _lib.ESHAPE)
    torch.cuda.synchronize(gpu)
    assert not out.any()  # nothing ran
    got = _run(sel, dev, 1, nv, 1).cpu()
    assert ar.valid_error(got, ref, 3, nv) < BAR


def test_zz_report_worst_errors():
    """Not a check of its own: the headroom of every kernel under the 2e-5 bar over the cases above, for whoever reworks one."""
    for sel in SELECTIONS:
        if sel in WORST:
            print(f"attention-edges worst {sel}: {WORST[sel]:.3e} (bar {BAR:.0e})")
            assert WORST[sel] < BAR
