// What every attention kernel and launcher shares, written once: the shape of a call, the decoding of a workgroup's work item and
// the walk over the key tiles of a tuple's source images.  Integer work only; the header makes no HIP call, so the walk also
// compiles for the host (tests/test_attention_walk.py enumerates it against a restatement in Python).
#pragma once
#include "../../include/e2emv.h"

#ifdef __HIPCC__
#define ATTN_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define ATTN_HD inline
#endif

namespace e2emv {

// The base of every attention kernel's parameter struct (filled by attn_shape).
struct AttnShape {
    int B, T, n_rows, D, H, cross;
    int nv[E2EMV_MAX_TUPLE];  // valid keypoints (queries and keys) of image t of a tuple
    int nq, groups, gper;     // query tiles per image, (image, head) groups, groups per XCD
};

// Key tiles of KV keys that the queries of image t walk: its own (self layer) or, source after source, those of every other
// image of the tuple in ascending order (cross layer).  Sources may differ in length; the last tile of each may be short.
template <int KV>
struct AttnKeyWalk {
    struct Pos { int si, kt; };  // source index, tile inside that source
    const int* nv;  // the shape's counts (the walk keeps no reference to the shape itself)
    int cross, t, n_src, n_tiles;
    ATTN_HD AttnKeyWalk(const AttnShape& shape, int t_) : nv(shape.nv), cross(shape.cross), t(t_), n_src(shape.cross ? shape.T - 1 : 1), n_tiles(0) {
        for (int si = 0; si < n_src; ++si) n_tiles += tiles(si);
    }
    ATTN_HD int src(int si) const { return !cross ? t : (si < t ? si : si + 1); }  // image of the tuple behind source si
    ATTN_HD int tiles(int si) const { return (nv[src(si)] + KV - 1) / KV; }
    // one tile on; from the last tile of a source to the first of the next (the last source is never left)
    ATTN_HD void advance(Pos& p) const {
        if (++p.kt * KV >= nv[src(p.si)] && p.si + 1 < n_src) { ++p.si; p.kt = 0; }
    }
    // linear tile index -> position (a search over the sources: for where a walk begins, not for every tile)
    ATTN_HD Pos at(int tile) const {
        int si = 0;
        for (;; ++si) {
            const int n = tiles(si);
            if (tile < n || si + 1 == n_src) break;
            tile -= n;
        }
        return Pos{si, tile};
    }
    ATTN_HD int valid(const Pos& p) const { return nv[src(p.si)] - p.kt * KV; }  // keys of the tile, >= 1; > KV: a full tile
};

#ifdef __HIPCC__
// Work item of workgroup `lin` of a grid of 8 * gper * nq: XCD-aware, all query tiles of one (image, head) share an XCD (K / V
// stay in its L2).  live = false: nothing to do (a group beyond the last, or a query tile beyond the keypoints of a shorter
// image of a ragged tuple).
struct AttnItem {
    int qt, img, head, b, t;
    bool live;
};
__device__ inline __attribute__((always_inline)) AttnItem attn_item(const AttnShape& s, int lin, int QT) {
    AttnItem it{};
    const int xcd = lin & 7, idx = lin >> 3;
    const int g = xcd * s.gper + idx / s.nq;
    if (g >= s.groups) return it;
    it.qt = idx % s.nq;
    it.img = g / s.H; it.head = g % s.H;
    it.b = it.img / s.T; it.t = it.img % s.T;
    it.live = it.qt * QT < s.nv[it.t];
    return it;
}
#endif

// ---- host side (attention.hip) ----
// The checks every launcher makes, then the shape: 0 < nv[t] <= n_rows, D == 64 H, n_rows a multiple of q_tile, a cross layer
// has another image to look at.  `who` prefixes the message.  *n_valid = the longest image; out->nq counts tiles of q_tile
// queries (a launcher whose kernel takes more per workgroup sets nq again).
int attn_shape(e2emv_ctx* ctx, const char* who, int B, int T, int n_rows, const int* nv, int D, int H, int cross, int q_tile,
               AttnShape* out, int* n_valid);
// key tiles a query walks, smallest over the images of the tuple (what a split along the keys can be cut into)
int attn_min_tiles(const AttnShape& s, int KV);

}  // namespace e2emv

#undef ATTN_HD
