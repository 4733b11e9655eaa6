"""CPU: the restated grid rule and tile walk of the layer GEMMs (tests/gemm_walk_plan.py) cover every tile once, and the shapes
tests/test_gpu_gemm_walk.py derives from them have workgroups that walk one, two and three tiles - on the MI355X's 256 CUs and on
two other CU counts - while staying inside the launchers' 32-bit operand offsets."""
import pytest

import gemm_walk_plan as G

CU_COUNTS = (32, 256, 304)


@pytest.mark.parametrize("cus", (8, 20) + CU_COUNTS)
@pytest.mark.parametrize("wg_per_cu", (1, 2, 3))
def test_every_tile_is_walked_exactly_once(cus, wg_per_cu):
    cap = cus * wg_per_cu // 8 * 8
    for total in list(range(1, 70)) + [cap - 1, cap, cap + 1, 2 * cap - 3, 2 * cap + 1, 3 * cap + 5, 1539]:
        if total < 1:
            continue
        slots, per_xcd, walks = G.plan(total, cus, wg_per_cu)
        assert len(walks) == 8 * slots and slots <= per_xcd and 8 * per_xcd >= total
        seen = sorted(t for w in walks.values() for t in w)
        assert seen == list(range(total)), (total, cus, wg_per_cu)
        for wg, w in walks.items():  # a workgroup stays inside its XCD's range and steps by the slot count
            assert all(t // per_xcd == (wg & 7) for t in w)
            assert all(b - a == slots for a, b in zip(w, w[1:]))


def test_walk_shapes_on_256_cus():
    """the figures of the GPU test's table"""
    assert G.walk_shape(256, 1, 3) == 171 * 3
    assert G.walk_shape(256, 2, 3) == 342 * 3
    assert G.walk_shape(256, 3, 3) == 513 * 3
    assert G.walk_shape(256, 3, 15) == 103 * 15  # the batched score-matrix case: 103 elements of 3 x 5 tiles
    assert G.mix(G.plan(513, 256, 1)[2]) == {3: 7, 2: 7 * 31 + 26, 1: 6}


@pytest.mark.parametrize("cus", CU_COUNTS)
@pytest.mark.parametrize("kernel,tiles_n", [(k, 3) for k in sorted(G.KERNELS)] + [("gemm_nt", 15)])
def test_walk_shapes_mix_one_two_and_three_tiles(cus, kernel, tiles_n):
    wg_per_cu, bm, bn = G.KERNELS[kernel]
    total = G.walk_shape(cus, wg_per_cu, tiles_n)
    assert total % tiles_n == 0 and total % 8 != 0
    slots, per_xcd, walks = G.plan(total, cus, wg_per_cu)
    have = G.mix(walks)
    assert set(have) == {1, 2, 3}, have
    # tile -> tile + slots changes the column tile as well as the row tile (3 column tiles; 5 in the batched case of 3 x 5 tiles).
    # gemm_nt's slot count, 3 workgroups per CU, is itself a multiple of 3: its unbatched case steps whole rows of tiles and the
    # batched case is the one that changes the column
    assert slots % (3 if tiles_n == 3 else 5) != 0 or (kernel == "gemm_nt" and tiles_n == 3)
    # no smaller count qualifies
    for smaller in range(tiles_n, total, tiles_n):
        if smaller % 8:
            assert not {1, 2, 3} <= set(G.mix(G.plan(smaller, cus, wg_per_cu)[2]))
    # the case built on it: a ragged last row tile, the launch has exactly these tiles, operands inside 32-bit offsets at K = 256
    if tiles_n == 3:
        M = G.rows_for(kernel, cus, 3, 37)
        N = 3 * bn - (0 if kernel == "gemm_h2<4>" else 84)
        assert G.tiles(kernel, M, N) == (total // 3, 3, total)
        assert M % bm != 0
        assert G.offsets_fit(kernel, M, N, 256) and G.offsets_fit(kernel, M, N, 128, 128)
        assert not G.nt_small(1, M, N, cus)
        assert M * N < 2 ** 31


def test_nt_small_rule():
    assert G.nt_small(1, 128, 128, 256) and G.nt_small(2, 1024, 1024, 256) and not G.nt_small(1, 2048, 1024 + 1, 256)
