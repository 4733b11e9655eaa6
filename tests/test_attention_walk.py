"""The key-tile walk every attention kernel shares (csrc/attention_walk.h: AttnKeyWalk), run on the host (needs no GPU).

A stand-alone program includes the header, builds the walk of every case it reads and prints the number of tiles, the cursor
sequence (source image, tile inside it, valid keys) that ``advance`` produces from {0, 0}, and ``at(k)`` for every tile.  The
expectation is written here a second time, from the definition: the sources of image t are t itself (self layer) or every other
image of the tuple in ascending order (cross layer), each with ceil(nv / 64) tiles of 64 keys, the last one short.

Cases: every t, both layer types and KV = 64 over every count in {1, 63, 64, 65, 128, 129}^T for T = 1..3 and over the tuples
of tests/test_gpu_attention_edges.py (T up to 8).  A cross layer needs T >= 2 (attn_shape refuses T = 1 before a walk is built)."""
import itertools
import os
import subprocess

import pytest

import test_gpu_attention_edges as edges

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KV = 64
COUNTS = (1, 63, 64, 65, 128, 129)

MAIN = r"""
#include <cstdio>
#include "attention_walk.h"
using namespace e2emv;
int main() {
    int T, cross, t;
    while (std::scanf("%d %d %d", &T, &cross, &t) == 3) {
        AttnShape s{};
        s.T = T; s.cross = cross;
        for (int i = 0; i < T; ++i) if (std::scanf("%d", &s.nv[i]) != 1) return 1;
        const AttnKeyWalk<64> w(s, t);
        std::printf("%d |", w.n_tiles);
        AttnKeyWalk<64>::Pos p{0, 0};
        for (int k = 0; k < w.n_tiles; ++k) {
            std::printf(" %d %d %d", w.src(p.si), p.kt, w.valid(p));
            if (k + 1 < w.n_tiles) w.advance(p);
        }
        std::printf(" |");
        for (int k = 0; k < w.n_tiles; ++k) {
            const AttnKeyWalk<64>::Pos a = w.at(k);
            std::printf(" %d %d", w.src(a.si), a.kt);
        }
        std::printf("\n");
    }
    return 0;
}
"""


def _cases():
    tuples = [nv for T in (1, 2, 3) for nv in itertools.product(COUNTS, repeat=T)]
    tuples += [tuple(nv) for _, nv in edges.RAGGED] + [tuple(nv) for nv, _ in edges.KEY_SPLIT]
    assert {len(nv) for nv in tuples} >= {1, 2, 3, 5, 8}
    return [(nv, cross, t) for nv in tuples for cross in ((0, 1) if len(nv) >= 2 else (0,)) for t in range(len(nv))]


def _expected(nv, cross, t):
    """[(source image, tile inside it, valid keys of the tile)] in the order a query of image t meets them"""
    sources = [s for s in range(len(nv)) if s != t] if cross else [t]
    return [(s, k, nv[s] - k * KV) for s in sources for k in range(-(-nv[s] // KV))]


@pytest.fixture(scope="module")
def walked(tmp_path_factory):
    d = tmp_path_factory.mktemp("attention_walk")
    src, exe = os.path.join(str(d), "walk_main.cpp"), os.path.join(str(d), "walk_main")
    with open(src, "w") as fh:
        fh.write(MAIN)
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "e2e_multi_view_matching_amd", "csrc"), src, "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    cases = _cases()
    text = "".join(f"{len(nv)} {cross} {t} {' '.join(map(str, nv))}\n" for nv, cross, t in cases)
    r = subprocess.run([exe], input=text, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
    assert r.returncode == 0, r.stdout
    lines = r.stdout.splitlines()
    assert len(lines) == len(cases)
    out = []
    for line in lines:
        n, seq, at = line.split("|")
        seq, at = [int(x) for x in seq.split()], [int(x) for x in at.split()]
        out.append((int(n), list(zip(seq[0::3], seq[1::3], seq[2::3])), list(zip(at[0::2], at[1::2]))))
    return cases, out


def test_the_cursor_visits_every_tile_of_every_source_in_order(walked):
    cases, out = walked
    print(f"attention-walk: {len(cases)} cases, {sum(n for n, _, _ in out)} tiles")
    for (nv, cross, t), (n_tiles, seq, _) in zip(cases, out):
        want = _expected(nv, cross, t)
        assert n_tiles == len(want), (nv, cross, t, n_tiles)
        assert seq == want, (nv, cross, t, seq)


def test_at_is_the_kth_position_of_the_cursor(walked):
    cases, out = walked
    for (nv, cross, t), (_, seq, at) in zip(cases, out):
        assert at == [(s, k) for s, k, _ in seq], (nv, cross, t, at)
