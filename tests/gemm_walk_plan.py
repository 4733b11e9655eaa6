"""The persistent tile walk of the layer GEMMs restated in plain Python (helper of tests/test_gemm_walk_plan.py, tests/test_gemm_walk.py
and tests/test_gpu_gemm_walk.py; no test lives here).  The library states the rule once, in csrc/gemm_walk.h (GemmWalk, gemm_slots,
gemm_tile); this file stays independent of it, and tests/test_gemm_walk.py holds the header to it on the host.

Every dense GEMM kernel (gemm_nt_kernel, gemm_x3_kernel, gemm_h2_kernel<2|4>, gemm_p2_kernel<...>) is launched by the same rule,
    per_xcd = ceil(total / 8),   slots = min(per_xcd, max(1, num_cus * wg_per_cu / 8)),   grid = 8 * slots workgroups,
and walks by the same rule: workgroup id = (xcd = id & 7, slot = id >> 3) takes tiles xcd * per_xcd + slot, + slots, ... below
min((xcd + 1) * per_xcd, total).  Tiles are numbered column tile fastest: tile = (batch element * tiles_m + row tile) * tiles_n +
column tile (only gemm_nt has a batch)."""
import collections

# kernel -> (workgroups per CU of its launcher, rows of a tile, columns of a tile)
KERNELS = {
    "gemm_nt": (3, 128, 128),      # (the 128 x 128 shape: not `small`, not the narrow convolution variant)
    "gemm_x3": (2, 128, 128),
    "gemm_h2<2>": (1, 256, 128),   # N % 256 != 0
    "gemm_h2<4>": (1, 256, 256),   # N % 256 == 0
    "gemm_p2": (1, 256, 256),
}


def grid(total, cus, wg_per_cu):
    """(slots, per_xcd) of a launch over `total` tiles"""
    per_xcd = (total + 7) // 8
    return min(per_xcd, max(1, cus * wg_per_cu // 8)), per_xcd


def plan(total, cus, wg_per_cu):
    """(slots, per_xcd, {workgroup id: [tiles in the order it walks them]}); a workgroup whose first tile lies beyond its XCD's
    range returns at once and has an empty list"""
    slots, per_xcd = grid(total, cus, wg_per_cu)
    walks = {}
    for wg in range(8 * slots):
        xcd, slot = wg & 7, wg >> 3
        t_end = min((xcd + 1) * per_xcd, total)
        walks[wg] = list(range(xcd * per_xcd + slot, t_end, slots))
    return slots, per_xcd, walks


def mix(walks):
    """{tiles walked: number of workgroups that walk so many}, idle workgroups left out"""
    return dict(collections.Counter(len(t) for t in walks.values() if t))


def walk_shape(cus, wg_per_cu, tiles_n, lengths=(1, 2, 3)):
    """The smallest tile count, a multiple of tiles_n and no multiple of 8 (the XCD ranges are then unequal), at which some
    workgroup walks each of `lengths` tiles.  The step from a workgroup's tile to its next, + slots, changes the row tile AND
    the column tile when slots is no multiple of the column tiles: with 3 column tiles that holds for one and two workgroups per
    CU (32 and 64 slots on 256 CUs), not for gemm_nt's three (96 slots) - its batched case has 5 column tiles for that."""
    limit = 8 * (max(lengths) + 1) * max(1, cus * wg_per_cu // 8) + 8 * tiles_n
    for total in range(tiles_n, limit + 1, tiles_n):
        if total % 8 == 0:
            continue
        have = mix(plan(total, cus, wg_per_cu)[2])
        if all(n in have for n in lengths):
            return total
    raise AssertionError(f"no tile count up to {limit} walks {lengths} on {cus} CUs x {wg_per_cu}")


def nt_small(batch, M, N, cus):
    """launch_gemm_nt's choice of the 64 x 64 latency shape (another kernel instance: gemm_nt_kernel<false, 0>)"""
    return batch * ((M + 127) // 128) * ((N + 127) // 128) * 2 <= cus


def tiles(kernel, M, N, batch=1):
    """(tiles_m, tiles_n, total) of a launch"""
    _, bm, bn = KERNELS[kernel]
    tm, tn = (M + bm - 1) // bm, (N + bn - 1) // bn
    return tm, tn, batch * tm * tn


def rows_for(kernel, cus, tiles_n, cut):
    """M of the walking case of `kernel` with tiles_n column tiles: walk_shape's row tiles, the last one `cut` rows short"""
    wg_per_cu, bm, _ = KERNELS[kernel]
    assert 0 < cut < bm
    total = walk_shape(cus, wg_per_cu, tiles_n)
    return (total // tiles_n) * bm - cut


def offsets_fit(kernel, M, N, K1, K2=0):
    """the launchers' 32-bit operand offset checks (gemm_h2: elements below 2^30, weight planes below 2^31 halves; gemm_p2: bytes
    below 2^31; gemm_nt and gemm_x3 address with 64-bit pointers)"""
    K = K1 + K2
    if kernel.startswith("gemm_h2"):
        return M * K1 < 2 ** 30 and M * max(K2, 1) < 2 ** 30 and N * 2 * K < 2 ** 31
    if kernel == "gemm_p2":
        return M * K1 * 4 < 2 ** 31 and M * max(K2, 1) * 4 < 2 ** 31 and N * K * 4 < 2 ** 31
    return True
