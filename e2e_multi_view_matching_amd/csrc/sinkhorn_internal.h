// Sinkhorn, internal: what the files of the family share on the host side.  sinkhorn.hip (workspace, plan, launch) calls the
// log-domain chain and the match block of sinkhorn_stream.hip through the functions below and gets the resident kernels of
// sinkhorn_resident.hip / sinkhorn_regs.hip / sinkhorn_regs2.hip as SkKernel descriptions.  (Other files need only common.h: sinkhorn_ws_bytes,
// launch_sinkhorn, SinkhornOut.)
#pragma once
#include "common.h"

namespace e2emv {

constexpr int SK_ROWS = 16;  // rows per workgroup of the log-domain sweep (4 waves x 4 rows)

static inline int round_up(int x, int m) { return (x + m - 1) / m * m; }
// column class of a padded row length: the KT (256-column chunks per wave) the kernels are instantiated for
static inline int KT_of(int64_t ldS) {
    const int kt = (int)((ldS + 255) / 256);
    return kt <= 2 ? kt : (kt <= 4 ? 4 : 8);
}
// rows per workgroup: 8 waves x RW rows.  RW = 8 at 513 .. 1024 columns (128 values per lane, one workgroup per CU: against
// RW = 4 - 64 values per lane, two workgroups per CU - the same number of resident problems, HALF as many workgroups in a
// problem's exchange and half the granule traffic), RW = 4 elsewhere
static inline int skr_rw(int64_t ldS) { return (ldS > 512 && ldS <= 1024) ? 8 : 4; }
static inline int skr_rows(int64_t ldS) { return 8 * skr_rw(ldS); }

struct SkParams {
    const float* S;     // [B][M][ldS]
    int64_t ldS;
    int M, N;
    int chunks;         // ceil(M / SK_ROWS)
    float alpha;        // bin score
    float norm;         // -log(M+N)
    float* u;           // [B][M+1]
    float* v;           // [B][ldV]  (ldV = ldS + 4, v[N] = dustbin column)
    int64_t ldV;
    float* pm;          // [B][chunks][ldS] partial column max
    float* ps;          // [B][chunks][ldS] partial column sum-exp
    float* v_next;      // [B][ldV]  written by sinkhorn_combine (ping-pong with v)
    float* upm;         // [B][chunks] partial max of u over a chunk's rows
    float* ups;         // [B][chunks] partial sum-exp of u over a chunk's rows
    // final sweep
    float* logZ[kMaxGroups];  // per output group: [group_batch][M+1][N+1] or null
    int group_batch;    // batch elements per output group
    float* max0;        // [B][M] row max of the core (value of logZ)
    int* idx0;          // [B][M]
    float* pv;          // [B][chunks][ldS] partial column max value (final)
    int* pi;            // [B][chunks][ldS] partial column arg-max row (final)
};

// ---- sinkhorn_stream.hip: the log-domain launch chain, the rescue pass, the match block
void sk_pad_copy_rows(const float* src, int64_t rows, int N, float* dst, int64_t ld, hipStream_t s);
// all iterations of the chain (p.v / p.v_next end up swapped so that p.v is the last v)
void sk_stream_iterate(SkParams& p, int B, int iters, hipStream_t s);
// non-finite potentials behind the chain are counted in flags[1], like the resident path's
void sk_check_finite(const SkParams& p, int B, unsigned* flags, hipStream_t s);
// problems whose potentials the resident kernel left non-finite are re-solved in the log domain
void sk_rescue(const SkParams& p, int B, int iters, unsigned* flags, hipStream_t s);
// logZ + fused arg-max from the final potentials (one more read of the scores)
void sk_final_sweep(const SkParams& p, int B, hipStream_t s);
// mutual check on the arg-max the final sweep left in p
void sk_match(const SkParams& p, int B, float match_thr, const SinkhornOut& out, hipStream_t s);

// ---- a resident kernel as the planner sees it
struct SkKernel { const void* fn = nullptr; int rows = 0, threads = 512, wg_per_cu = 0; size_t lds = 0; bool big = false; };
// sinkhorn_resident.hip: the instance for (KT, full tiles, 16-byte granule pairs); fn, rows, threads, lds
SkKernel sinkhorn_resident_kernel(int KT, bool full, bool pairs);
// sinkhorn_regs.hip: sinkhorn_resident128 (KT == 4) / sinkhorn_resident2k (KT == 8), full = full rows AND columns; fn, rows, threads, lds, big
SkKernel sinkhorn_regs_kernel(int KT, bool full);
// sinkhorn_regs2.hip: sinkhorn_resident128w (KT == 4: 128 rows per workgroup on 8 waves, two per SIMD), full as above, G = workgroups
// per problem (the instance's stage-A lane mapping follows the width of a column slice); fn, rows, threads, lds, big
SkKernel sinkhorn_regs2_kernel(bool full, int G);

}  // namespace e2emv
