"""The tile walk, the grid rule and the tile decode every dense GEMM shares (csrc/gemm_walk.h), run on the host (needs no GPU).

A stand-alone program includes the header.  For every (total, cus, wg_per_cu) it reads it prints ``gemm_slots`` and, for every
workgroup id of the launch of 8 * slots workgroups, the tiles that ``GemmWalk`` visits, in order; for every (tiles_m, tiles_n) it
reads it prints both decodes of every tile index.  The expectation is tests/gemm_walk_plan.py, the independent restatement in
Python that tests/test_gpu_gemm_walk.py sizes its shapes by, and ``divmod``.

Cases: every total in 1 .. 200 and the walk_shape totals of tests/test_gemm_walk_plan.py, on 32, 256 and 304 CUs, with 1, 2 and 3
workgroups per CU; tiles_n in 1 .. 5 and tiles_m in 1 .. 4 (three batch elements in the batched form)."""
import os
import subprocess

import pytest

import gemm_walk_plan as G
from test_gemm_walk_plan import CU_COUNTS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCH = 3

MAIN = r"""
#include <cstdio>
#include "gemm_walk.h"
using namespace e2emv;
int main() {
    char what;
    int a, b, c;
    while (std::scanf(" %c %d %d %d", &what, &a, &b, &c) == 4) {
        if (what == 'w') {  // total, cus, wg_per_cu
            const int slots = gemm_slots(a, b, c);
            std::printf("%d", slots);
            for (int wg = 0; wg < 8 * slots; ++wg) {
                const GemmWalk w(a, wg, 8 * slots);
                std::printf(" | %d", w.empty() ? 1 : 0);
                for (int t = w.tile; t < w.t_end; t += w.slots) std::printf(" %d", t);
            }
        } else {  // batch, tiles_m, tiles_n
            for (int t = 0; t < b * c; ++t) {
                const GemmTile d = gemm_tile(t, c);
                std::printf(" %d %d", d.tm, d.tn);
            }
            std::printf(" |");
            for (int t = 0; t < a * b * c; ++t) {
                const GemmTileZ d = gemm_tile(t, b, c);
                std::printf(" %d %d %d", d.z, d.tm, d.tn);
            }
        }
        std::printf("\n");
    }
    return 0;
}
"""


def _walk_cases():
    cases = []
    for cus in CU_COUNTS:
        # the totals of test_gemm_walk_plan.py: 3 column tiles for every kernel's workgroups per CU, gemm_nt's batched 3 x 5 tiles
        shapes = {G.walk_shape(cus, w, 3) for w in (1, 2, 3)} | {G.walk_shape(cus, G.KERNELS["gemm_nt"][0], 15)}
        for wg_per_cu in (1, 2, 3):
            cases += [(total, cus, wg_per_cu) for total in sorted(set(range(1, 201)) | shapes)]
    return cases


def _decode_cases():
    return [(BATCH, tiles_m, tiles_n) for tiles_m in range(1, 5) for tiles_n in range(1, 6)]


@pytest.fixture(scope="module")
def walked(tmp_path_factory):
    d = tmp_path_factory.mktemp("gemm_walk")
    src, exe = os.path.join(str(d), "walk_main.cpp"), os.path.join(str(d), "walk_main")
    with open(src, "w") as fh:
        fh.write(MAIN)
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "e2e_multi_view_matching_amd", "csrc"), src, "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    walks, decodes = _walk_cases(), _decode_cases()
    text = "".join("w %d %d %d\n" % c for c in walks) + "".join("d %d %d %d\n" % c for c in decodes)
    r = subprocess.run([exe], input=text, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
    assert r.returncode == 0, r.stdout
    lines = r.stdout.splitlines()
    assert len(lines) == len(walks) + len(decodes)
    return walks, lines[:len(walks)], decodes, lines[len(walks):]


def test_grid_rule_and_walk_match_the_restatement(walked):
    walks, lines, _, _ = walked
    print(f"gemm-walk: {len(walks)} launches")
    for (total, cus, wg_per_cu), line in zip(walks, lines):
        head, *groups = line.split("|")
        slots, per_xcd, want = G.plan(total, cus, wg_per_cu)
        assert int(head) == slots == G.grid(total, cus, wg_per_cu)[0], (total, cus, wg_per_cu, head)
        assert len(groups) == 8 * slots
        for wg, g in enumerate(groups):
            empty, *tiles = [int(x) for x in g.split()]
            assert tiles == want[wg], (total, cus, wg_per_cu, wg, tiles)
            assert empty == (not tiles), (total, cus, wg_per_cu, wg)


def test_every_tile_is_visited_exactly_once(walked):
    walks, lines, _, _ = walked
    for (total, cus, wg_per_cu), line in zip(walks, lines):
        seen = sorted(int(x) for g in line.split("|")[1:] for x in g.split()[1:])
        assert seen == list(range(total)), (total, cus, wg_per_cu)


def test_tile_decodes_are_divmod(walked):
    _, _, decodes, lines = walked
    for (batch, tiles_m, tiles_n), line in zip(decodes, lines):
        flat, batched = ([int(x) for x in part.split()] for part in line.split("|"))
        assert list(zip(flat[0::2], flat[1::2])) == [divmod(t, tiles_n) for t in range(tiles_m * tiles_n)], (tiles_m, tiles_n)
        want = [(t // (tiles_m * tiles_n),) + divmod(t % (tiles_m * tiles_n), tiles_n) for t in range(batch * tiles_m * tiles_n)]
        assert list(zip(batched[0::3], batched[1::3], batched[2::3])) == want, (batch, tiles_m, tiles_n)
