// What every dense GEMM kernel (gemm.hip, gemm_x3.hip, gemm_h2.hip, gemm_p2.hip) and its launcher share, written once: the
// persistent tile walk, the decoding of a tile index and the grid rule.  Integer work only; the header makes no HIP call, so the
// walk also compiles for the host (tests/test_gemm_walk.py enumerates it against the restatement in tests/gemm_walk_plan.py).
#pragma once
#include "../../include/e2emv.h"

#ifdef __HIPCC__
#define GEMM_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define GEMM_HD inline
#endif

namespace e2emv {

// Persistent kernels: a launch is 8 * slots workgroups; workgroup (xcd = id & 7, slot = id >> 3) walks tiles
// xcd * per_xcd + slot, + slots, ... of its XCD's contiguous tile range, so the tiles in flight on one XCD are neighbours
// (shared A panels stay in that L2):  for (t = tile; t < t_end; t += slots).  Tiles are numbered column tile fastest.
struct GemmWalk {
    int tile, t_end, slots;
    GEMM_HD GemmWalk(int total, unsigned wg, unsigned wgs) : slots(wgs >> 3) {
        const int xcd = wg & 7, slot = wg >> 3, per_xcd = (total + 7) / 8, t_begin = xcd * per_xcd;
        t_end = t_begin + per_xcd < total ? t_begin + per_xcd : total;
        tile = t_begin + slot;
    }
    GEMM_HD bool empty() const { return tile >= t_end; }  // the first tile lies beyond the range: nothing to do
};
// The grid rule: a launch over `total` tiles is 8 * gemm_slots(...) workgroups - every XCD its share of the workgroups the chip
// holds at `wg_per_cu` per CU, and no more slots than its range has tiles.
GEMM_HD int gemm_slots(int total, int cus, int wg_per_cu) {
    const int per_xcd = (total + 7) / 8, resident = cus * wg_per_cu >= 8 ? cus * wg_per_cu / 8 : 1;
    return per_xcd < resident ? per_xcd : resident;
}

// tile index -> (row tile, column tile), and gemm_nt's batched form -> (batch element, row tile, column tile)
struct GemmTile { int tm, tn; };
struct GemmTileZ { int z, tm, tn; };
GEMM_HD GemmTile gemm_tile(int t, int tiles_n) {
    const int tm = t / tiles_n;
    return GemmTile{tm, t - tm * tiles_n};  // (written so, not with %: gemm_h2 / gemm_p2 compile to another instruction stream)
}
GEMM_HD GemmTileZ gemm_tile(int t, int tiles_m, int tiles_n) {
    const int tiles_mn = tiles_m * tiles_n, z = t / tiles_mn;
    const GemmTile r = gemm_tile(t - z * tiles_mn, tiles_n);
    return GemmTileZ{z, r.tm, r.tn};
}

// ---- host side (gemm.hip): the operand checks the launchers share; `who` prefixes the message ----
struct GemmArgs;
// K segments of an A operand that may come in two pieces [A | A2]: *K1_out = columns of the first (K without an A2); whole K tiles
int gemm_k_segments(e2emv_ctx* ctx, const char* who, int K, int K1, bool has_A2, int* K1_out);
// gemm_x3 / gemm_h2: weights and output present, every row an access touches 16-byte aligned (`ldw_name`: the weight stride in
// the message), no output scale
int gemm_rows16(e2emv_ctx* ctx, const char* who, const GemmArgs& a, const void* W, int64_t ldw, const char* ldw_name);

}  // namespace e2emv

#undef GEMM_HD
