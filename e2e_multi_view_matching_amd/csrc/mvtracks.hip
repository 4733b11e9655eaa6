// Track merging for the batched multi-view back-end: the pairwise matches of a T-tuple become tracks (one 3-D point per scene
// point, seen by 2 .. T images) and the bundle-adjustment problem is built from the tracks instead of one point per match.
//
// Semantics (DESIGN.md section 1 quotes them):
//   node      keypoint n of image t of tuple b, id t * Nmax + n, Nmax = the label row stride (the largest keypoint count)
//   edge      pair q = (i, j) in the order of e2emv_mv_collect: every keypoint n of image i that mv_collect_kernel keeps
//             (0 <= match < n_kpts_j, every confidence channel > conf_thresh) joins (i, n) and (j, match) and carries the
//             confidence of channel 0; a pair without matches has no edge
//   label     the smallest node id of the node's connected component (a unique fixed point: any propagation order ends there)
//   track     a component of >= 2 nodes with AT MOST ONE node per image; a component with two keypoints of one image is a
//             conflict and contributes nothing
//   repair    (e2emv_mv_tracks_repair, rounds >= 0; a stage between "edge" and "label") edge id e = q * N + n, every kept edge
//             starts LIVE.  One round: components over the live edges; in EVERY conflicting component the live edge with the
//             smallest key (confidence of channel 0 compared as floats with <, -0.0 = +0.0; then the smaller edge id) is cut,
//             exactly one per component per round.  The stage ends after `rounds` rounds or when no component conflicts; label,
//             track and conflict are then the definitions above over the live edges (a component that still conflicts
//             contributes nothing, a node that lost all its live edges is in no track).  rounds = 0 is e2emv_mv_tracks bit for
//             bit.  The problem does NOT see the cuts: labels and stats are the only interface to mv_tracks_emit_kernel, and a
//             node's confidence stays the mean of the KEPT (original) edges between it and the other members of its track.  A cut
//             edge whose ends land in different tracks drops out by that rule; a cut edge that lay on a cycle, so that both its
//             ends end in the same valid track, still counts - it is consistent with the track it ended in.
//   problem   points = tracks in ascending label, observations of a point in ascending image, concatenated in point order;
//             index lists as e2emv_mv_bundle_adjust_batch builds them; camera 0 fixed, f = 1, c = 0
//   weight    node confidence = fp64 mean of its kept edges' confidences (ascending other image); weights = confidence /
//             (0.5 (sum + 1e-3)), sum over the tuple's observations in a fixed order
//   start     homogeneous DLT over the k views (rows x P[2] - P[0], y P[2] - P[1]), smallest eigenvector of the 4x4 normal
//             matrix by the cyclic Jacobi of mv_dlt; for k = 2 mv_dlt itself
// Nothing crosses tuples, no floating-point atomics: a tuple's labels, problem and solution are bit-identical alone, at any batch
// position and run to run.  The integer LDS atomics used (min, or, add) have order-independent results.
//
// LIMIT: T * Nmax <= 16384 nodes per tuple (8 images of 2048 keypoints): mv_tracks_kernel keeps a 32-bit label per node (native
// LDS atomic min; 16 bits would do for the ids but LDS has no 16-bit atomic), 8 image bits and one conflict bit per root in LDS
// = 5.125 bytes per node, 82 KiB at the limit, of the 160 KiB one workgroup may declare on gfx950.  Above the limit the entry
// points return E2EMV_ESHAPE before any launch.  mv_tracks_repair_kernel adds a 32-bit arg-min key per root (the 64-bit key
// (confidence, edge id) would not fit: it is found in two 32-bit passes, first the smallest confidence, then the smallest edge
// id among the edges that have it) = 9.125 bytes per node, 146 KiB at the limit, and one dead bit per edge id: P * N <= (T - 1) / 2
// * T * Nmax <= 3.5 * 16384 bits = 7 KiB.  153 KiB + 32 bytes of static LDS at the limit; the same limit holds.
#include <algorithm>
#include <cstdint>
#include <cstring>

#include "common.h"
#include "mv_host.h"
#include "mvba.h"

namespace e2emv {

constexpr int kMvTrackThreads = 1024;
constexpr int kMvTrackMaxNodes = 16384;

struct MvEdgeArgs {
    int B, T, P, N, Nmax, channels;  // N = rows of every match array (keypoints of a pair's first image), Nmax = label row stride
    float thresh;
    int n1[kMvMaxPairs];                // keypoints of the second image
    unsigned char pi[kMvMaxPairs], pj[kMvMaxPairs];
    const int64_t* match[kMvMaxPairs];  // [B,N] or NULL (no matches for this pair)
    const float* conf[kMvMaxPairs];     // [B,N,channels]
};

// the match of keypoint n of the first image of pair q of tuple b when mv_collect_kernel keeps it (the edge), else -1; *c0 its
// confidence (channel 0)
__device__ __forceinline__ int mv_edge(const MvEdgeArgs& a, int b, int q, int n, float* c0) {
    const int64_t* match = a.match[q];
    if (!match) return -1;
    const size_t row = size_t(b) * a.N + n;
    const int64_t m = match[row];
    bool keep = m >= 0 && m < a.n1[q];
    const float* conf = a.conf[q] + row * a.channels;
    for (int c = 0; c < a.channels; ++c) keep = keep && conf[c] > a.thresh;
    if (c0) *c0 = conf[0];
    return keep ? int(m) : -1;
}

__device__ __forceinline__ int mv_pair_index(int i, int j) { return j * (j - 1) / 2 + i; }  // i < j, j outer

// Connected components of one tuple per workgroup, labels in LDS: min-label propagation over the edges (atomic min on the larger
// label's node and on the edge's own end) followed by pointer jumping (every label is a node of the same component with an id
// not above the node's, so chains end at a root), until a sweep changes nothing.  Labels only decrease, so the loop ends; the
// bound of `nodes` sweeps holds whatever the input.  Then the images of every component are OR-ed into 8 bits of its root, a
// second hit of a set bit marks the conflict, and every node writes its track's label or -1.
// stats[b] = {tracks, observations (nodes in tracks), conflict components, edges}.
__global__ __launch_bounds__(kMvTrackThreads) void mv_tracks_kernel(MvEdgeArgs a, int* __restrict__ out_label, int* __restrict__ out_stats) {
    extern __shared__ __attribute__((aligned(16))) int s_trk[];
    __shared__ int s_changed, s_stats[4];
    const int b = blockIdx.x, tid = threadIdx.x, nodes = a.T * a.Nmax, n_edges = a.P * a.N;
    int* s_label = s_trk;                                                 // [nodes]
    unsigned* s_mask = reinterpret_cast<unsigned*>(s_trk + nodes);         // [(nodes + 3) / 4]: 8 image bits per root
    unsigned* s_bad = s_mask + (nodes + 3) / 4;                            // [(nodes + 31) / 32]: conflict bit per root
    for (int x = tid; x < nodes; x += kMvTrackThreads) s_label[x] = x;
    for (int x = tid; x < (nodes + 3) / 4; x += kMvTrackThreads) s_mask[x] = 0u;
    for (int x = tid; x < (nodes + 31) / 32; x += kMvTrackThreads) s_bad[x] = 0u;
    if (tid < 4) s_stats[tid] = 0;
    int edges = 0;
    for (int sweep = 0; sweep < nodes; ++sweep) {
        if (tid == 0) s_changed = 0;
        __syncthreads();
        bool changed = false;
        for (int e = tid; e < n_edges; e += kMvTrackThreads) {
            const int q = e / a.N, n = e - q * a.N;
            const int m = mv_edge(a, b, q, n, nullptr);
            if (m < 0) continue;
            if (sweep == 0) ++edges;
            const int x = a.pi[q] * a.Nmax + n, y = a.pj[q] * a.Nmax + m;
            const int lx = s_label[x], ly = s_label[y];
            if (lx == ly) continue;
            const int lo = min(lx, ly), hi = max(lx, ly);
            atomicMin(&s_label[hi], lo);
            atomicMin(&s_label[lx > ly ? x : y], lo);
            changed = true;
        }
        if (changed) s_changed = 1;
        __syncthreads();
        for (int x = tid; x < nodes; x += kMvTrackThreads) {
            int l = s_label[x];
            while (true) {
                const int up = s_label[l];
                if (up == l) break;
                l = up;
            }
            s_label[x] = l;
        }
        const int again = s_changed;
        __syncthreads();
        if (!again) break;
    }
    for (int x = tid; x < nodes; x += kMvTrackThreads) {
        const int t = x / a.Nmax, r = s_label[x];
        const unsigned bit = 1u << (t + 8 * (r & 3));
        if (atomicOr(&s_mask[r >> 2], bit) & bit) atomicOr(&s_bad[r >> 5], 1u << (r & 31));
    }
    __syncthreads();
    int tracks = 0, obs = 0, bad = 0;
    for (int x = tid; x < nodes; x += kMvTrackThreads) {
        const int r = s_label[x];
        const int views = __popc((s_mask[r >> 2] >> (8 * (r & 3))) & 0xffu);
        const bool conflict = (s_bad[r >> 5] >> (r & 31)) & 1u, valid = !conflict && views >= 2;
        out_label[size_t(b) * nodes + x] = valid ? r : -1;
        if (r == x) { tracks += valid; obs += valid ? views : 0; bad += conflict; }
    }
    atomicAdd(&s_stats[0], tracks); atomicAdd(&s_stats[1], obs); atomicAdd(&s_stats[2], bad); atomicAdd(&s_stats[3], edges);
    __syncthreads();
    if (tid < 4) out_stats[4 * b + tid] = s_stats[tid];
}

// float -> unsigned whose unsigned order is the float order (no NaN reaches it: a kept edge has conf > thresh); -0.0 ties +0.0
__device__ __forceinline__ unsigned mv_conf_key(float c) {
    unsigned u = __float_as_uint(c);
    if ((u << 1) == 0u) u = 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

constexpr unsigned kMvNoKey = 0xffffffffu;  // above every confidence key (it is the key of a NaN) and every edge id
constexpr int kMvRepairMaxRounds = 64;
constexpr int kMvRepairMaxEdgeIds = 64 * kMvTrackThreads;  // one candidate bit per edge id a thread visits, in one 64-bit register

// mv_tracks_kernel with the repair stage of the header comment: the labelling of mv_tracks_kernel (the same sweeps over the LIVE
// edges, the same classification) once per round, then one cut per conflicting component:
//   1. every live edge of a conflicting root takes an atomic min of its confidence key on s_key[root];
//   2. every thread notes, one bit per edge id it visits, the live edges whose key equals that minimum (the candidates);
//   3. s_key is reset and the candidates take an atomic min of their edge id on s_key[root];
//   4. the candidate whose id is the minimum sets its bit in the dead-edge bitmap.
// Both minima are unique values, so the cut does not depend on the order of the atomics.  Before the next round the nodes of the
// conflicting components go back to their own ids (labels only decrease: a stale label would keep a split component glued;
// the other components have no cut and keep their converged labels), mask and conflict bits are cleared.
// Bounds: rounds <= `rounds` <= 64 (the host checks), sweeps <= nodes per round, pointer chains end at a root as in
// mv_tracks_kernel, edge ids per thread <= 64 (P * N <= kMvRepairMaxEdgeIds, the host checks).  rounds = 0 is mv_tracks_kernel.
// stats[b] = {tracks, observations, conflict components left, live edges}.
__global__ __launch_bounds__(kMvTrackThreads) void mv_tracks_repair_kernel(MvEdgeArgs a, int rounds, int* __restrict__ out_label,
                                                                            int* __restrict__ out_stats) {
    extern __shared__ __attribute__((aligned(16))) int s_trk[];
    __shared__ int s_changed, s_any_bad, s_stats[4];
    const int b = blockIdx.x, tid = threadIdx.x, nodes = a.T * a.Nmax, n_edges = a.P * a.N;
    const int mask_words = (nodes + 3) / 4, bad_words = (nodes + 31) / 32, dead_words = (n_edges + 31) / 32;
    int* s_label = s_trk;                                              // [nodes]
    unsigned* s_mask = reinterpret_cast<unsigned*>(s_trk + nodes);      // [mask_words]: 8 image bits per root
    unsigned* s_bad = s_mask + mask_words;                              // [bad_words]: conflict bit per root
    unsigned* s_dead = s_bad + bad_words;                               // [dead_words]: cut bit per edge id
    unsigned* s_key = s_dead + dead_words;                              // [nodes]: arg-min key per root
    for (int x = tid; x < nodes; x += kMvTrackThreads) s_label[x] = x;
    for (int x = tid; x < mask_words; x += kMvTrackThreads) s_mask[x] = 0u;
    for (int x = tid; x < bad_words; x += kMvTrackThreads) s_bad[x] = 0u;
    for (int x = tid; x < dead_words; x += kMvTrackThreads) s_dead[x] = 0u;
    if (tid < 4) s_stats[tid] = 0;
    int edges = 0;
    for (int round = 0;; ++round) {
        edges = 0;
        for (int sweep = 0; sweep < nodes; ++sweep) {
            if (tid == 0) s_changed = 0;
            __syncthreads();
            bool changed = false;
            for (int e = tid; e < n_edges; e += kMvTrackThreads) {
                if ((s_dead[e >> 5] >> (e & 31)) & 1u) continue;
                const int q = e / a.N, n = e - q * a.N;
                const int m = mv_edge(a, b, q, n, nullptr);
                if (m < 0) continue;
                if (sweep == 0) ++edges;
                const int x = a.pi[q] * a.Nmax + n, y = a.pj[q] * a.Nmax + m;
                const int lx = s_label[x], ly = s_label[y];
                if (lx == ly) continue;
                const int lo = min(lx, ly), hi = max(lx, ly);
                atomicMin(&s_label[hi], lo);
                atomicMin(&s_label[lx > ly ? x : y], lo);
                changed = true;
            }
            if (changed) s_changed = 1;
            __syncthreads();
            for (int x = tid; x < nodes; x += kMvTrackThreads) {
                int l = s_label[x];
                while (true) {
                    const int up = s_label[l];
                    if (up == l) break;
                    l = up;
                }
                s_label[x] = l;
            }
            const int again = s_changed;
            __syncthreads();
            if (!again) break;
        }
        for (int x = tid; x < nodes; x += kMvTrackThreads) {
            const int t = x / a.Nmax, r = s_label[x];
            const unsigned bit = 1u << (t + 8 * (r & 3));
            if (atomicOr(&s_mask[r >> 2], bit) & bit) atomicOr(&s_bad[r >> 5], 1u << (r & 31));
        }
        if (tid == 0) s_any_bad = 0;
        __syncthreads();
        if (round >= rounds) break;  // uniform: the labels of the last round are the result
        bool any = false;
        for (int x = tid; x < bad_words; x += kMvTrackThreads) any = any || s_bad[x] != 0u;
        if (any) s_any_bad = 1;
        for (int x = tid; x < nodes; x += kMvTrackThreads) s_key[x] = kMvNoKey;
        __syncthreads();
        if (!s_any_bad) break;  // uniform: nothing conflicts, nothing to cut
        // 1. the smallest confidence among the live edges of every conflicting root
        for (int e = tid; e < n_edges; e += kMvTrackThreads) {
            if ((s_dead[e >> 5] >> (e & 31)) & 1u) continue;
            const int q = e / a.N, n = e - q * a.N;
            float c;
            if (mv_edge(a, b, q, n, &c) < 0) continue;
            const int r = s_label[a.pi[q] * a.Nmax + n];
            if ((s_bad[r >> 5] >> (r & 31)) & 1u) atomicMin(&s_key[r], mv_conf_key(c));
        }
        __syncthreads();
        // 2. the candidates: bit k of `cand` is edge id tid + k * 1024
        unsigned long long cand = 0ull;
        int k = 0;
        for (int e = tid; e < n_edges; e += kMvTrackThreads, ++k) {
            if ((s_dead[e >> 5] >> (e & 31)) & 1u) continue;
            const int q = e / a.N, n = e - q * a.N;
            float c;
            if (mv_edge(a, b, q, n, &c) < 0) continue;
            const int r = s_label[a.pi[q] * a.Nmax + n];
            if (((s_bad[r >> 5] >> (r & 31)) & 1u) && s_key[r] == mv_conf_key(c)) cand |= 1ull << k;
        }
        __syncthreads();
        // 3. the smallest edge id among them
        for (int x = tid; x < nodes; x += kMvTrackThreads) s_key[x] = kMvNoKey;
        __syncthreads();
        k = 0;
        for (int e = tid; e < n_edges; e += kMvTrackThreads, ++k) {
            if (!((cand >> k) & 1ull)) continue;
            const int q = e / a.N, n = e - q * a.N;
            atomicMin(&s_key[s_label[a.pi[q] * a.Nmax + n]], unsigned(e));
        }
        __syncthreads();
        // 4. the cut
        k = 0;
        for (int e = tid; e < n_edges; e += kMvTrackThreads, ++k) {
            if (!((cand >> k) & 1ull)) continue;
            const int q = e / a.N, n = e - q * a.N;
            if (s_key[s_label[a.pi[q] * a.Nmax + n]] == unsigned(e)) atomicOr(&s_dead[e >> 5], 1u << (e & 31));
        }
        __syncthreads();
        // the next round starts the cut components from their own ids
        for (int x = tid; x < nodes; x += kMvTrackThreads) {
            const int r = s_label[x];
            if ((s_bad[r >> 5] >> (r & 31)) & 1u) s_label[x] = x;
        }
        __syncthreads();  // s_bad is read above and cleared below
        for (int x = tid; x < mask_words; x += kMvTrackThreads) s_mask[x] = 0u;
        for (int x = tid; x < bad_words; x += kMvTrackThreads) s_bad[x] = 0u;
    }
    int tracks = 0, obs = 0, bad = 0;
    for (int x = tid; x < nodes; x += kMvTrackThreads) {
        const int r = s_label[x];
        const int views = __popc((s_mask[r >> 2] >> (8 * (r & 3))) & 0xffu);
        const bool conflict = (s_bad[r >> 5] >> (r & 31)) & 1u, valid = !conflict && views >= 2;
        out_label[size_t(b) * nodes + x] = valid ? r : -1;
        if (r == x) { tracks += valid; obs += valid ? views : 0; bad += conflict; }
    }
    atomicAdd(&s_stats[0], tracks); atomicAdd(&s_stats[1], obs); atomicAdd(&s_stats[2], bad); atomicAdd(&s_stats[3], edges);
    __syncthreads();
    if (tid < 4) out_stats[4 * b + tid] = s_stats[tid];
}

// dehomogenised smallest eigenvector of the symmetric 4x4 M (row-major, destroyed): the cyclic Jacobi of mv_dlt, statement for
// statement, for the normal matrix of k >= 3 views (mv_dlt keeps its own copy: its kernels compile to the code they always had)
__device__ __forceinline__ void mv_null4(double* M, double* xyz) {
    double V[16];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) V[4 * r + c] = r == c ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 30; ++sweep) {
        double off = 0;
        for (int p = 0; p < 4; ++p)
            for (int q = p + 1; q < 4; ++q) off += M[4 * p + q] * M[4 * p + q];
        if (off < 1e-300) break;
        for (int p = 0; p < 4; ++p)
            for (int q = p + 1; q < 4; ++q) {
                const double apq = M[4 * p + q];
                if (apq == 0.0) continue;
                const double theta = (M[4 * q + q] - M[4 * p + p]) / (2.0 * apq);
                const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                for (int k = 0; k < 4; ++k) {
                    const double mkp = M[4 * k + p], mkq = M[4 * k + q];
                    M[4 * k + p] = c * mkp - s * mkq;
                    M[4 * k + q] = s * mkp + c * mkq;
                }
                for (int k = 0; k < 4; ++k) {
                    const double mpk = M[4 * p + k], mqk = M[4 * q + k];
                    M[4 * p + k] = c * mpk - s * mqk;
                    M[4 * q + k] = s * mpk + c * mqk;
                }
                for (int k = 0; k < 4; ++k) {
                    const double vkp = V[4 * k + p], vkq = V[4 * k + q];
                    V[4 * k + p] = c * vkp - s * vkq;
                    V[4 * k + q] = s * vkp + c * vkq;
                }
            }
    }
    int m = 0;
    for (int k = 1; k < 4; ++k)
        if (M[5 * k] < M[5 * m]) m = k;
    const double w = V[12 + m];
    xyz[0] = V[m] / w;
    xyz[1] = V[4 + m] / w;
    xyz[2] = V[8 + m] / w;
}

struct MvEmitArgs {
    MvEdgeArgs e;
    int kdim, intr_batch;
    int n_img[kMvMaxCams];          // keypoints of every image
    const float* kpts[kMvMaxCams];  // [B,n_img[t],2]
    const float* intr[kMvMaxCams];  // [intr_batch,kdim,kdim]
    const int* label;               // [B,T,Nmax] of mv_tracks_kernel
    const double* proj;             // [B,T,3,4] world -> camera
    int* member;                    // [points of the batch,T] scratch: the keypoint of image t in the point, or -1
    const MvbaArgs* recs;           // [B] the problems being built
    double loss_scale;              // relative scale of the robust loss (0: no loss)
};

// The track problem of one tuple per workgroup, from its labels.  Roots (label == own id) in ascending id are the points (ordered
// compaction: ballot prefix inside a wave, wave totals through LDS, a running base over the chunks of 256, as mv_collect_kernel);
// every labelled node enters its point's row of `member`.  Then per point: observation offset = exclusive prefix of the view
// counts, position in camera t's list = number of earlier points seen by t (the same compaction per camera), both ascending
// in the observation index as the host lists of e2emv_mv_bundle_adjust_batch.  Every write is bounded by the record's sizes: a
// label array that disagrees with the counts the record was sized from gives a wrong problem, not a write outside it.
__global__ __launch_bounds__(kMvRowThreads) void mv_tracks_emit_kernel(MvEmitArgs g) {
    extern __shared__ __attribute__((aligned(16))) unsigned short s_pidx[];  // [nodes]: point of a root, 0xffff otherwise
    __shared__ int s_wave[(kMvMaxCams + 1) * (kMvRowThreads / 64)], s_cnt[kMvMaxCams], s_cstart[kMvMaxCams + 1];
    __shared__ double s_red[kMvRowThreads / 64];
    const MvEdgeArgs& e = g.e;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int T = e.T, Nmax = e.Nmax, nodes = T * Nmax;
    const MvbaArgs& a = g.recs[b];
    const int P = a.P, O = a.O;
    int* member = g.member + size_t(a.pts - g.recs[0].pts) / 3 * T;
    const int* label = g.label + size_t(b) * nodes;
    int* cam_idx = const_cast<int*>(a.cam_idx); int* pt_idx = const_cast<int*>(a.pt_idx);
    int* pt_start = const_cast<int*>(a.pt_start); int* pt_obs = const_cast<int*>(a.pt_obs);
    int* cam_start = const_cast<int*>(a.cam_start); int* cam_obs = const_cast<int*>(a.cam_obs);
    double* obs = const_cast<double*>(a.obs); double* wts = const_cast<double*>(a.wts);
    const unsigned long long below = (1ull << lane) - 1ull;

    for (int i = tid; i < P * T; i += kMvRowThreads) member[i] = -1;
    if (tid < kMvMaxCams) s_cnt[tid] = 0;
    int base = 0;
    for (int c0 = 0; c0 < nodes; c0 += kMvRowThreads) {
        const int x = c0 + tid;
        const bool root = x < nodes && label[x] == x;
        const unsigned long long mask = __ballot(root);
        if (lane == 0) s_wave[wave] = __popcll(mask);
        __syncthreads();
        int off = base + __popcll(mask & below), total = 0;
        for (int w = 0; w < kMvRowThreads / 64; ++w) {
            if (w < wave) off += s_wave[w];
            total += s_wave[w];
        }
        if (x < nodes) s_pidx[x] = (root && off < P) ? (unsigned short)off : (unsigned short)0xffff;
        base += total;
        __syncthreads();
    }
    int cnt[kMvMaxCams];
#pragma unroll
    for (int t = 0; t < kMvMaxCams; ++t) cnt[t] = 0;
    for (int x = tid; x < nodes; x += kMvRowThreads) {
        const int L = label[x], t = x / Nmax, n = x - t * Nmax;
        if (L < 0 || L >= nodes || n >= g.n_img[t]) continue;
        const int p = s_pidx[L];
        if (p >= P) continue;
        member[p * T + t] = n;
#pragma unroll
        for (int u = 0; u < kMvMaxCams; ++u) cnt[u] += (u == t);
    }
#pragma unroll
    for (int t = 0; t < kMvMaxCams; ++t)
        if (cnt[t]) atomicAdd(&s_cnt[t], cnt[t]);
    __syncthreads();  // the rows of `member` and the camera totals are complete
    if (tid == 0) {
        int c = 0;
        for (int t = 0; t < T; ++t) { s_cstart[t] = c; cam_start[t] = c; c += s_cnt[t]; }
        s_cstart[T] = c; cam_start[T] = c;
        pt_start[P] = O;
    }
    __syncthreads();

    int o_base = 0, c_base[kMvMaxCams];
#pragma unroll
    for (int t = 0; t < kMvMaxCams; ++t) c_base[t] = 0;
    double conf_sum = 0.0;
    for (int c0 = 0; c0 < P; c0 += kMvRowThreads) {
        const int p = c0 + tid;
        int mem[kMvMaxCams], k = 0;
#pragma unroll
        for (int t = 0; t < kMvMaxCams; ++t) {
            mem[t] = (p < P && t < T) ? member[p * T + t] : -1;
            k += mem[t] >= 0;
        }
        // exclusive prefix of the view counts: inclusive scan inside the wave, then the waves in front
        int incl = k;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int up = __shfl_up(incl, d);
            if (lane >= d) incl += up;
        }
        int rank[kMvMaxCams];
#pragma unroll
        for (int t = 0; t < kMvMaxCams; ++t) {
            const unsigned long long mask = __ballot(mem[t] >= 0);
            rank[t] = __popcll(mask & below);
            if (lane == 0) s_wave[(t + 1) * (kMvRowThreads / 64) + wave] = __popcll(mask);
        }
        if (lane == 63) s_wave[wave] = incl;
        __syncthreads();
        int o0 = o_base + incl - k;
        for (int w = 0; w < kMvRowThreads / 64; ++w) {
            if (w < wave) o0 += s_wave[w];
            o_base += s_wave[w];
        }
#pragma unroll
        for (int t = 0; t < kMvMaxCams; ++t) {
            rank[t] += c_base[t];
            for (int w = 0; w < kMvRowThreads / 64; ++w) {
                const int tot = s_wave[(t + 1) * (kMvRowThreads / 64) + w];
                if (w < wave) rank[t] += tot;
                c_base[t] += tot;
            }
        }
        if (p < P && o0 + k <= O) {
            pt_start[p] = o0;
            double x[2 * kMvMaxCams];
            int o = o0;
#pragma unroll
            for (int t = 0; t < kMvMaxCams; ++t) {
                x[2 * t] = 0.0; x[2 * t + 1] = 0.0;
                if (mem[t] < 0) continue;
                const float* K = g.intr[t] + (g.intr_batch == 1 ? 0 : size_t(b) * g.kdim * g.kdim);
                const float* kp = g.kpts[t] + (size_t(b) * g.n_img[t] + mem[t]) * 2;
                // pixel -> normalised camera coordinates in fp32 like mv_build_kernel: one rounded subtraction, one rounded division
                const float xn = (kp[0] - K[2]) / K[0], yn = (kp[1] - K[g.kdim + 2]) / K[g.kdim + 1];
                x[2 * t] = double(xn); x[2 * t + 1] = double(yn);
                // confidence of the node: mean of its kept edges, other image ascending
                double cs = 0.0;
                int ce = 0;
#pragma unroll
                for (int u = 0; u < kMvMaxCams; ++u) {
                    if (u == t || mem[u] < 0) continue;
                    float c = 0.f;
                    int m = -1;
                    if (u < t) {
                        if (mem[u] < e.N) m = mv_edge(e, b, mv_pair_index(u, t), mem[u], &c);
                        if (m != mem[t]) continue;
                    } else {
                        if (mem[t] < e.N) m = mv_edge(e, b, mv_pair_index(t, u), mem[t], &c);
                        if (m != mem[u]) continue;
                    }
                    cs += double(c);
                    ++ce;
                }
                const double cn = ce ? cs / double(ce) : 0.0;
                conf_sum += cn;
                cam_idx[o] = t; pt_idx[o] = p; pt_obs[o] = o;
                obs[2 * o] = x[2 * t]; obs[2 * o + 1] = x[2 * t + 1];
                wts[2 * o] = cn;
                const int slot = s_cstart[t] + rank[t];
                if (slot < O) cam_obs[slot] = o;
                ++o;
            }
            const double* proj = g.proj + size_t(b) * T * 12;
            double* X = a.pts + 3 * size_t(p);
            if (k == 2) {
                int t0 = -1, t1 = -1;
#pragma unroll
                for (int t = kMvMaxCams - 1; t >= 0; --t)
                    if (mem[t] >= 0) { t1 = t1 < 0 ? t : t1; t0 = t; }
                double x0x = 0, x0y = 0, x1x = 0, x1y = 0;
#pragma unroll
                for (int t = 0; t < kMvMaxCams; ++t) {
                    if (t == t0) { x0x = x[2 * t]; x0y = x[2 * t + 1]; }
                    if (t == t1) { x1x = x[2 * t]; x1y = x[2 * t + 1]; }
                }
                mv_dlt(proj + 12 * t0, proj + 12 * t1, x0x, x0y, x1x, x1y, X);
            } else {
                double M[16];
#pragma unroll
                for (int i = 0; i < 16; ++i) M[i] = 0.0;
#pragma unroll
                for (int t = 0; t < kMvMaxCams; ++t) {
                    if (mem[t] < 0) continue;
                    const double* Pm = proj + 12 * t;
                    double r0[4], r1[4];
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        r0[c] = x[2 * t] * Pm[8 + c] - Pm[c];
                        r1[c] = x[2 * t + 1] * Pm[8 + c] - Pm[4 + c];
                    }
#pragma unroll
                    for (int r = 0; r < 4; ++r)
#pragma unroll
                        for (int c = 0; c < 4; ++c) M[4 * r + c] += r0[r] * r0[c] + r1[r] * r1[c];
                }
                mv_null4(M, X);
            }
        }
        __syncthreads();
    }
    // sum of the node confidences in a fixed order (points strided over the threads, then lanes, then waves), the weights
    conf_sum = wave_sum_d(conf_sum);
    if (lane == 0) s_red[wave] = conf_sum;
    __syncthreads();
    double total = s_red[0];
    for (int w = 1; w < kMvRowThreads / 64; ++w) total += s_red[w];
    const double half_total = 0.5 * (total + 1e-3);
    // the loss scale relative to the weights, as in mv_build_kernel
    if (tid == 0 && g.loss_scale > 0.0) const_cast<MvbaArgs&>(a).loss_a = g.loss_scale / half_total;
    for (int o = tid; o < O; o += kMvRowThreads) {
        const double w = wts[2 * o] / half_total;
        wts[2 * o] = w; wts[2 * o + 1] = w;
    }
}

// Reverse of the weights mv_tracks_emit_kernel hands the solver ("Backward pass of the track route").  Observation o is a
// node of a track; c_o = the mean of its e_o kept edges inside the track, H = 0.5 (sum_o c_o + 1e-3), w_o = c_o / H on both weight
// entries.  With G_o = g_w[2o] + g_w[2o+1] of the solver's reverse pass and D = sum_o G_o w_o:
//     cbar_o = (G_o - 0.5 D) / H,     confbar of an edge inside a track = cbar_o / e_o of its one end + cbar_o / e_o of the other.
// Every decision is the forward's: the labels, the keep rule (mv_edge), the members of a point (`member`, as the emit kernel left
// it in the workspace) and the observation offsets (pt_start).  One workgroup per tuple, fp64, no atomics.
//   pass 1  over the points, strided over the threads like the emit kernel's chunks: e_o recounted as that kernel counts `ce`, the sum
//           of the node confidences and D in its order (a thread's points ascending, then lanes, then waves - H has the forward's
//           bits); `share[o]` = cbar_o / e_o; `node_obs` = the observation of a node, -1 for a node in no track
//   pass 2  thread = (pair, row): an edge the keep rule keeps whose ends carry the same label >= 0 gathers the shares of its two ends
//           into channel 0; every other element of d_gconf[q][b] is written 0 (a NULL d_gconf[q] leaves the pair out)
// A tuple without tracks (P = 0) reads nothing of its empty problem and writes zeros.  Every index is bounded by the record's sizes:
// labels that disagree with the counts give a wrong gradient, not an access outside the workspace.
struct MvTracksBwdArgs {
    MvEdgeArgs e;
    const int* label;              // [B,T,Nmax]
    const int* member;             // [points of the batch,T] of the emit kernel
    const MvbaArgs* recs;          // [B]
    const MvbaBwdArgs* bw;         // [B]: g_w
    double* share;                 // [observations of the batch]
    int* node_obs;                 // [B,T,Nmax]
    float* gconf[kMvMaxPairs];     // [B,N,channels] or NULL
};
__global__ __launch_bounds__(kMvRowThreads) void mv_tracks_weights_backward_kernel(MvTracksBwdArgs g) {
    __shared__ double s_red[2 * (kMvRowThreads / 64)];
    const MvEdgeArgs& e = g.e;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int T = e.T, Nmax = e.Nmax, nodes = T * Nmax;
    const MvbaArgs& a = g.recs[b];
    const int P = a.P, O = a.O;
    const int* member = g.member + size_t(a.pts - g.recs[0].pts) / 3 * T;
    const int* label = g.label + size_t(b) * nodes;
    int* node_obs = g.node_obs + size_t(b) * nodes;
    double* share = g.share + size_t(a.obs - g.recs[0].obs) / 2;
    const double* gw = g.bw[b].g_w;
    for (int x = tid; x < nodes; x += kMvRowThreads) node_obs[x] = -1;
    for (int o = tid; o < O; o += kMvRowThreads) share[o] = 0.0;
    __syncthreads();
    double conf_sum = 0.0, dot = 0.0;
    for (int p = tid; p < P; p += kMvRowThreads) {
        int mem[kMvMaxCams], k = 0;
#pragma unroll
        for (int t = 0; t < kMvMaxCams; ++t) {
            mem[t] = t < T ? member[p * T + t] : -1;
            if (mem[t] >= Nmax) mem[t] = -1;
            k += mem[t] >= 0;
        }
        int o = a.pt_start[p];
        if (o < 0 || o + k > O) continue;
#pragma unroll
        for (int t = 0; t < kMvMaxCams; ++t) {
            if (mem[t] < 0) continue;
            // confidence of the node: mean of its kept edges, other image ascending (mv_tracks_emit_kernel)
            double cs = 0.0;
            int ce = 0;
#pragma unroll
            for (int u = 0; u < kMvMaxCams; ++u) {
                if (u == t || mem[u] < 0) continue;
                float c = 0.f;
                int m = -1;
                if (u < t) {
                    if (mem[u] < e.N) m = mv_edge(e, b, mv_pair_index(u, t), mem[u], &c);
                    if (m != mem[t]) continue;
                } else {
                    if (mem[t] < e.N) m = mv_edge(e, b, mv_pair_index(t, u), mem[t], &c);
                    if (m != mem[u]) continue;
                }
                cs += double(c);
                ++ce;
            }
            conf_sum += ce ? cs / double(ce) : 0.0;
            dot += (gw[2 * o] + gw[2 * o + 1]) * a.wts[2 * o];
            share[o] = double(ce);
            node_obs[t * Nmax + mem[t]] = o;
            ++o;
        }
    }
    conf_sum = wave_sum_d(conf_sum); dot = wave_sum_d(dot);
    if (lane == 0) { s_red[wave] = conf_sum; s_red[kMvRowThreads / 64 + wave] = dot; }
    __syncthreads();  // also: every share and node_obs of pass 1 is written
    double total = s_red[0];
    dot = s_red[kMvRowThreads / 64];
    for (int w = 1; w < kMvRowThreads / 64; ++w) { total += s_red[w]; dot += s_red[kMvRowThreads / 64 + w]; }
    const double H = 0.5 * (total + 1e-3);
    for (int o = tid; o < O; o += kMvRowThreads) {
        const double ce = share[o];
        share[o] = ce > 0.0 ? (gw[2 * o] + gw[2 * o + 1] - 0.5 * dot) / H / ce : 0.0;
    }
    __syncthreads();
    for (int q = 0; q < e.P; ++q) {
        float* out = g.gconf[q];
        if (!out) continue;
        for (int n = tid; n < e.N; n += kMvRowThreads) {
            float v = 0.f;
            const int m = mv_edge(e, b, q, n, nullptr);
            if (m >= 0) {
                const int x = e.pi[q] * Nmax + n, y = e.pj[q] * Nmax + m, L = label[x];
                if (L >= 0 && L == label[y]) {
                    const int ox = node_obs[x], oy = node_obs[y];
                    if (ox >= 0 && oy >= 0) v = float(share[ox] + share[oy]);
                }
            }
            float* row = out + (size_t(b) * e.N + n) * e.channels;
            row[0] = v;
            for (int c = 1; c < e.channels; ++c) row[c] = 0.f;
        }
    }
}

// argument checks and the edge description shared by the three entry points
static int mv_edge_args(e2emv_ctx* ctx, const char* who, int B, int T, int N, int Nmax, const int32_t* n1, const int64_t* const* d_matches,
                        const float* const* d_conf, int channels, float thresh, MvEdgeArgs* a) {
    if (B < 1 || N < 1 || channels < 1 || !n1 || !d_matches || !d_conf) return set_err(ctx, E2EMV_EINVAL, "%s: bad argument (B, N, conf_channels >= 1, no NULL array)", who);
    if (T < 2 || T > kMvMaxCams) return set_err(ctx, E2EMV_EINVAL, "%s: tuple of %d images (2 <= T <= %d)", who, T, kMvMaxCams);
    *a = MvEdgeArgs{};
    a->B = B; a->T = T; a->P = T * (T - 1) / 2; a->N = N; a->channels = channels; a->thresh = thresh;
    int q = 0, widest = N;
    for (int j = 0; j < T; ++j)
        for (int i = 0; i < j; ++i, ++q) {
            if (d_matches[q] && (!d_conf[q] || n1[q] < 1)) return set_err(ctx, E2EMV_EINVAL, "%s: pair %d has matches but no confidences / keypoints", who, q);
            a->match[q] = d_matches[q]; a->conf[q] = d_conf[q]; a->n1[q] = d_matches[q] ? n1[q] : 0;
            a->pi[q] = (unsigned char)i; a->pj[q] = (unsigned char)j;
            widest = std::max(widest, int(n1[q]));  // also of a pair without matches: the stride covers every image the caller names
        }
    a->Nmax = Nmax > 0 ? Nmax : widest;
    if (a->Nmax < widest) return set_err(ctx, E2EMV_ESHAPE, "%s: label stride %d below the keypoint count %d", who, a->Nmax, widest);
    if (size_t(T) * size_t(a->Nmax) > size_t(kMvTrackMaxNodes))
        return set_err(ctx, E2EMV_ESHAPE, "%s: %d images of up to %d keypoints are %zu nodes (limit %d)", who, T, a->Nmax, size_t(T) * a->Nmax, kMvTrackMaxNodes);
    if (size_t(B) * T * a->Nmax > size_t(INT32_MAX) / 64) return set_err(ctx, E2EMV_ESHAPE, "%s: B * T * Nmax = %zu is too large", who, size_t(B) * T * a->Nmax);
    return E2EMV_OK;
}

// the track problems of the B tuples in the workspace, described by *L (the counterpart of mv_tuple_build): `tail` bytes are reserved
// behind the layout; emit_out (may be NULL) receives what the emit kernel was launched with - the edges, the labels, `member`, the records
static int mv_tracks_build(e2emv_ctx* ctx, const char* who, int B, int T, int N, int Nmax, const int32_t* d_label, const int32_t* stats,
                           const float* const* d_kpts, const int32_t* n_kpts, const int64_t* const* d_matches, const float* const* d_conf,
                           int channels, float thresh, const float* const* d_intr, int kdim, int intr_batch, const double* extr,
                           int max_iterations, double loss_scale, size_t tail, MvLayout* L, size_t* totP_out, size_t* totO_out, MvEmitArgs* emit_out,
                           hipStream_t s) {
    if (!d_label || !stats || !d_kpts || !n_kpts || !d_intr || !extr || Nmax < 1) return set_err(ctx, E2EMV_EINVAL, "%s: bad argument (Nmax >= 1, no NULL array)", who);
    if (T < 2 || T > kMvMaxCams) return set_err(ctx, E2EMV_EINVAL, "%s: tuple of %d images (2 <= T <= %d)", who, T, kMvMaxCams);
    if (kdim != 3 && kdim != 4) return set_err(ctx, E2EMV_ESHAPE, "%s: intrinsics must be 3x3 or 4x4", who);
    if (intr_batch != 1 && intr_batch != B) return set_err(ctx, E2EMV_ESHAPE, "%s: intr_batch must be 1 or B", who);
    int32_t n1[kMvMaxPairs];
    int q = 0;
    for (int j = 0; j < T; ++j)
        for (int i = 0; i < j; ++i, ++q) n1[q] = n_kpts[j];
    MvEmitArgs g{};
    int rc = mv_edge_args(ctx, who, B, T, N, Nmax, n1, d_matches, d_conf, channels, thresh, &g.e);
    if (rc) return rc;
    for (int t = 0; t < T; ++t) {
        if (!d_intr[t] || !d_kpts[t]) return set_err(ctx, E2EMV_EINVAL, "%s: NULL intrinsics / keypoints of image %d", who, t);
        if (n_kpts[t] < 1 || n_kpts[t] > Nmax) return set_err(ctx, E2EMV_EINVAL, "%s: image %d has %d keypoints (1 <= n <= Nmax = %d)", who, t, n_kpts[t], Nmax);
        g.n_img[t] = n_kpts[t]; g.kpts[t] = d_kpts[t]; g.intr[t] = d_intr[t];
    }
    q = 0;
    for (int j = 0; j < T; ++j)
        for (int i = 0; i < j; ++i, ++q)
            if (d_matches[q] && n_kpts[i] < N) return set_err(ctx, E2EMV_EINVAL, "%s: pair %d has %d match rows but image %d only %d keypoints", who, q, N, i, n_kpts[i]);
    size_t totP = 0, totO = 0;
    for (int b = 0; b < B; ++b) {
        const int Pb = stats[4 * b], Ob = stats[4 * b + 1];
        if (Pb < 0 || Ob < 2 * Pb || Ob > T * Pb || Ob > T * Nmax)
            return set_err(ctx, E2EMV_EINVAL, "%s: tuple %d counts %d tracks / %d observations (2 .. %d views per track, at most %d nodes)", who, b, Pb, Ob, T, T * Nmax);
        totP += size_t(Pb); totO += size_t(Ob);
    }
    const size_t n = size_t(B), totC = n * T;
    const size_t proj_bytes = (totC * 12 * 8 + 255) & ~size_t(255), extra = proj_bytes + totP * T * sizeof(int);
    rc = ws_reserve(ctx, mv_layout(nullptr, n, totC, totP, totO, extra).bytes + tail);
    if (rc) return rc;
    *L = mv_layout(ctx->d_ws, n, totC, totP, totO, extra);
    // one staging block = one copy: records, start cameras, (zero) camera list starts, projection matrices
    std::vector<char> stage(L->upload_bytes - (extra - proj_bytes), 0);
    auto at = [&](const void* dev) { return stage.data() + (reinterpret_cast<const char*>(dev) - ctx->d_ws); };
    MvbaArgs* recs = reinterpret_cast<MvbaArgs*>(at(L->recs));
    double* cams = reinterpret_cast<double*>(at(L->cams));
    double* proj = reinterpret_cast<double*>(at(L->extra));
    const double unit_intr[4] = {1.0, 1.0, 0.0, 0.0};  // the intrinsics are folded into the observations
    size_t p0 = 0, o0 = 0;
    for (int b = 0; b < B; ++b) {
        for (int t = 0; t < T; ++t) {
            const double* E = extr + (size_t(b) * T + t) * 16;
            std::memcpy(proj + (size_t(b) * T + t) * 12, E, 12 * sizeof(double));
            mv_extr_to_cam(E, cams + (size_t(b) * T + t) * 6);
        }
        recs[b] = mv_record(*L, size_t(b), size_t(b) * T, p0, o0, T, 0, stats[4 * b], stats[4 * b + 1], max_iterations, unit_intr, 0.0);
        p0 += size_t(stats[4 * b]); o0 += size_t(stats[4 * b + 1]);
    }
    E2EMV_HIP(ctx, hipMemcpyAsync(ctx->d_ws, stage.data(), stage.size(), hipMemcpyHostToDevice, s));
    E2EMV_HIP(ctx, hipStreamSynchronize(s));  // the staging block dies at return
    g.kdim = kdim; g.intr_batch = intr_batch;
    g.label = d_label;
    g.proj = reinterpret_cast<const double*>(L->extra);
    g.member = reinterpret_cast<int*>(L->extra + proj_bytes);
    g.recs = L->recs;
    g.loss_scale = loss_scale;
    const size_t lds = size_t(T) * Nmax * sizeof(unsigned short);
    rc = ensure_dynamic_lds(ctx, reinterpret_cast<const void*>(mv_tracks_emit_kernel), lds);
    if (rc) return rc;
    hipLaunchKernelGGL(mv_tracks_emit_kernel, dim3(B), dim3(kMvRowThreads), lds, s, g);
    E2EMV_CHECK_LAUNCH(ctx, "mv_tracks_emit_kernel");
    *totP_out = totP; *totO_out = totO;
    if (emit_out) *emit_out = g;
    return E2EMV_OK;
}

}  // namespace e2emv

using namespace e2emv;

extern "C" int e2emv_mv_tracks(e2emv_ctx* ctx, int B, int T, int N, const int32_t* n_kpts1, const int64_t* const* d_matches,
                               const float* const* d_conf, int conf_channels, float conf_thresh, int32_t* d_label, int32_t* d_stats,
                               void* stream) {
    if (!ctx) return E2EMV_EINVAL;
    E2EMV_ENTER(ctx, stream);
    if (!d_label || !d_stats) return set_err(ctx, E2EMV_EINVAL, "mv_tracks: NULL output");
    MvEdgeArgs a;
    int rc = mv_edge_args(ctx, "mv_tracks", B, T, N, 0, n_kpts1, d_matches, d_conf, conf_channels, conf_thresh, &a);
    if (rc) return rc;
    const size_t nodes = size_t(T) * a.Nmax, lds = (nodes + (nodes + 3) / 4 + (nodes + 31) / 32) * 4;
    rc = ensure_dynamic_lds(ctx, reinterpret_cast<const void*>(mv_tracks_kernel), lds);
    if (rc) return rc;
    hipLaunchKernelGGL(mv_tracks_kernel, dim3(B), dim3(kMvTrackThreads), lds, (hipStream_t)stream, a, d_label, d_stats);
    E2EMV_CHECK_LAUNCH(ctx, "mv_tracks_kernel");
    return E2EMV_OK;
}

extern "C" int e2emv_mv_tracks_repair(e2emv_ctx* ctx, int B, int T, int N, const int32_t* n_kpts1, const int64_t* const* d_matches,
                                      const float* const* d_conf, int conf_channels, float conf_thresh, int rounds, int32_t* d_label,
                                      int32_t* d_stats, void* stream) {
    if (!ctx) return E2EMV_EINVAL;
    E2EMV_ENTER(ctx, stream);
    if (!d_label || !d_stats) return set_err(ctx, E2EMV_EINVAL, "mv_tracks_repair: NULL output");
    if (rounds < 0 || rounds > kMvRepairMaxRounds) return set_err(ctx, E2EMV_EINVAL, "mv_tracks_repair: %d rounds (0 <= rounds <= %d)", rounds, kMvRepairMaxRounds);
    MvEdgeArgs a;
    int rc = mv_edge_args(ctx, "mv_tracks_repair", B, T, N, 0, n_kpts1, d_matches, d_conf, conf_channels, conf_thresh, &a);
    if (rc) return rc;
    const size_t nodes = size_t(T) * a.Nmax, edge_ids = size_t(a.P) * N;  // N <= Nmax: edge_ids <= (T - 1) / 2 * nodes <= 3.5 * 16384
    if (edge_ids > size_t(kMvRepairMaxEdgeIds)) return set_err(ctx, E2EMV_ESHAPE, "mv_tracks_repair: %zu edge ids (limit %d)", edge_ids, kMvRepairMaxEdgeIds);
    const size_t lds = (2 * nodes + (nodes + 3) / 4 + (nodes + 31) / 32 + (edge_ids + 31) / 32) * 4;
    rc = ensure_dynamic_lds(ctx, reinterpret_cast<const void*>(mv_tracks_repair_kernel), lds);
    if (rc) return rc;
    hipLaunchKernelGGL(mv_tracks_repair_kernel, dim3(B), dim3(kMvTrackThreads), lds, (hipStream_t)stream, a, rounds, d_label, d_stats);
    E2EMV_CHECK_LAUNCH(ctx, "mv_tracks_repair_kernel");
    return E2EMV_OK;
}

extern "C" int e2emv_mv_tuple_ba_tracks_loss(e2emv_ctx* ctx, int B, int T, int N, int Nmax, const int32_t* d_label, const int32_t* stats,
                                             const float* const* d_kpts, const int32_t* n_kpts, const int64_t* const* d_matches,
                                             const float* const* d_conf, int conf_channels, float conf_thresh, const float* const* d_intr,
                                             int kdim, int intr_batch, const double* extr, int max_iterations, double* out_extr,
                                             double* summary, int loss, double loss_scale, double* loss_a_out, void* stream) {
    if (!ctx) return E2EMV_EINVAL;
    E2EMV_ENTER(ctx, stream);
    if (!out_extr) return set_err(ctx, E2EMV_EINVAL, "mv_tuple_ba_tracks: NULL output");
    int rc = mv_check_loss(ctx, "mv_tuple_ba_tracks", loss, &loss_scale);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    MvLayout L;
    size_t totP = 0, totO = 0;
    rc = mv_tracks_build(ctx, "mv_tuple_ba_tracks", B, T, N, Nmax, d_label, stats, d_kpts, n_kpts, d_matches, d_conf, conf_channels,
                         conf_thresh, d_intr, kdim, intr_batch, extr, max_iterations, loss_scale, 0, &L, &totP, &totO, nullptr, s);
    if (rc) return rc;
    rc = mv_launch_ba(ctx, L, B, s, loss);
    if (rc) return rc;
    return mv_tuple_results(ctx, L, B, T, out_extr, summary, loss_a_out, s);
}

extern "C" int e2emv_mv_tuple_ba_tracks(e2emv_ctx* ctx, int B, int T, int N, int Nmax, const int32_t* d_label, const int32_t* stats,
                                        const float* const* d_kpts, const int32_t* n_kpts, const int64_t* const* d_matches,
                                        const float* const* d_conf, int conf_channels, float conf_thresh, const float* const* d_intr,
                                        int kdim, int intr_batch, const double* extr, int max_iterations, double* out_extr,
                                        double* summary, void* stream) {
    return e2emv_mv_tuple_ba_tracks_loss(ctx, B, T, N, Nmax, d_label, stats, d_kpts, n_kpts, d_matches, d_conf, conf_channels, conf_thresh,
                                         d_intr, kdim, intr_batch, extr, max_iterations, out_extr, summary, kLossNone, 0.0, nullptr, stream);
}

extern "C" int e2emv_mv_tuple_problem_tracks(e2emv_ctx* ctx, int B, int T, int N, int Nmax, const int32_t* d_label, const int32_t* stats,
                                             const float* const* d_kpts, const int32_t* n_kpts, const int64_t* const* d_matches,
                                             const float* const* d_conf, int conf_channels, float conf_thresh,
                                             const float* const* d_intr, int kdim, int intr_batch, const double* extr, int32_t* cam_idx,
                                             int32_t* pt_idx, double* obs_xy, double* obs_w, double* cams, double* pts, void* stream) {
    if (!ctx) return E2EMV_EINVAL;
    E2EMV_ENTER(ctx, stream);
    if (!cams) return set_err(ctx, E2EMV_EINVAL, "mv_tuple_problem_tracks: NULL output");
    hipStream_t s = (hipStream_t)stream;
    MvLayout L;
    size_t totP = 0, totO = 0;
    const int rc = mv_tracks_build(ctx, "mv_tuple_problem_tracks", B, T, N, Nmax, d_label, stats, d_kpts, n_kpts, d_matches, d_conf,
                                   conf_channels, conf_thresh, d_intr, kdim, intr_batch, extr, 0, 0.0, 0, &L, &totP, &totO, nullptr, s);
    if (rc) return rc;
    if (totP && (!cam_idx || !pt_idx || !obs_xy || !obs_w || !pts)) return set_err(ctx, E2EMV_EINVAL, "mv_tuple_problem_tracks: NULL output for %zu points", totP);
    E2EMV_HIP(ctx, hipMemcpyAsync(cams, L.cams, sizeof(double) * 6 * B * T, hipMemcpyDeviceToHost, s));
    if (totP) {
        E2EMV_HIP(ctx, hipMemcpyAsync(cam_idx, L.cam_idx, sizeof(int) * totO, hipMemcpyDeviceToHost, s));
        E2EMV_HIP(ctx, hipMemcpyAsync(pt_idx, L.pt_idx, sizeof(int) * totO, hipMemcpyDeviceToHost, s));
        E2EMV_HIP(ctx, hipMemcpyAsync(obs_xy, L.obs, sizeof(double) * 2 * totO, hipMemcpyDeviceToHost, s));
        E2EMV_HIP(ctx, hipMemcpyAsync(obs_w, L.wts, sizeof(double) * 2 * totO, hipMemcpyDeviceToHost, s));
        E2EMV_HIP(ctx, hipMemcpyAsync(pts, L.pts, sizeof(double) * 3 * totP, hipMemcpyDeviceToHost, s));
    }
    E2EMV_HIP(ctx, hipStreamSynchronize(s));
    return E2EMV_OK;
}

extern "C" int e2emv_mv_tuple_ba_tracks_backward(e2emv_ctx* ctx, int B, int T, int N, int Nmax, const int32_t* d_label, const int32_t* stats,
                                                 const float* const* d_kpts, const int32_t* n_kpts, const int64_t* const* d_matches,
                                                 const float* const* d_conf, int conf_channels, float conf_thresh, const float* const* d_intr,
                                                 int kdim, int intr_batch, const double* extr, int max_iterations, const double* g_out_extr,
                                                 float* const* d_gconf, void* stream) {
    if (!ctx) return E2EMV_EINVAL;
    E2EMV_ENTER(ctx, stream);
    const char* who = "mv_tuple_ba_tracks_backward";
    if (!g_out_extr || !d_gconf) return set_err(ctx, E2EMV_EINVAL, "%s: NULL g_out_extr / d_gconf", who);
    if (B < 1 || T < 2 || T > kMvMaxCams || Nmax < 1 || !stats) return set_err(ctx, E2EMV_EINVAL, "%s: bad argument (B, Nmax >= 1, 2 <= T <= %d, stats)", who, kMvMaxCams);
    // the tape is sized from the counts the labels were made with (mv_tracks_build's rule for them)
    std::vector<int> Cs(B, T), Ps(B, 0), Os(B, 0);
    for (int b = 0; b < B; ++b) {
        const int Pb = stats[4 * b], Ob = stats[4 * b + 1];
        if (Pb < 0 || Ob < 2 * Pb || Ob > T * Pb || size_t(Ob) > size_t(T) * size_t(Nmax))
            return set_err(ctx, E2EMV_EINVAL, "%s: tuple %d counts %d tracks / %d observations (2 .. %d views per track, at most %zu nodes)", who, b, Pb, Ob, T, size_t(T) * Nmax);
        Ps[b] = Pb; Os[b] = Ob;
    }
    bool overflow = false;
    const size_t tape = mv_bwd_bytes(Cs, Ps, Os, max_iterations, &overflow);
    int rc = mv_bwd_fits(ctx, who, tape, overflow);
    if (rc) return rc;
    // behind the solver's share: cbar_o / e_o per observation and the observation of every node
    size_t sumO = 0;
    for (int b = 0; b < B; ++b) sumO += size_t(Os[b]);
    const size_t tape_al = (tape + 255) & ~size_t(255), share_bytes = (sumO * sizeof(double) + 255) & ~size_t(255);
    const size_t tail = tape_al + share_bytes + size_t(B) * T * size_t(Nmax) * sizeof(int);
    hipStream_t s = (hipStream_t)stream;
    MvLayout L;
    MvEmitArgs emit{};
    size_t totP = 0, totO = 0;
    rc = mv_tracks_build(ctx, who, B, T, N, Nmax, d_label, stats, d_kpts, n_kpts, d_matches, d_conf, conf_channels, conf_thresh, d_intr, kdim,
                         intr_batch, extr, max_iterations, 0.0, tail, &L, &totP, &totO, &emit, s);
    if (rc) return rc;
    char* base = ctx->d_ws + L.bytes;
    MvBwdLayout W;
    rc = mv_bwd_carve(ctx, base, Cs, Ps, Os, max_iterations, true, &W, s);
    if (rc) return rc;
    const size_t totC = size_t(B) * T;
    E2EMV_HIP(ctx, hipMemsetAsync(W.cams_bar, 0, sizeof(double) * 6 * totC, s));
    if (totP) E2EMV_HIP(ctx, hipMemsetAsync(W.pts_bar, 0, sizeof(double) * 3 * totP, s));
    E2EMV_HIP(ctx, hipMemcpyAsync(W.g_extr, g_out_extr, sizeof(double) * 16 * totC, hipMemcpyHostToDevice, s));
    E2EMV_HIP(ctx, hipStreamSynchronize(s));  // g_out_extr is the caller's
    rc = mv_launch_ba_backward(ctx, L, W, B, s);
    if (rc) return rc;
    MvTracksBwdArgs g{};
    g.e = emit.e; g.label = emit.label; g.member = emit.member; g.recs = L.recs; g.bw = W.recs;
    g.share = reinterpret_cast<double*>(base + tape_al);
    g.node_obs = reinterpret_cast<int*>(base + tape_al + share_bytes);
    for (int q = 0; q < g.e.P; ++q) g.gconf[q] = d_gconf[q];
    hipLaunchKernelGGL(mv_tracks_weights_backward_kernel, dim3(B), dim3(kMvRowThreads), 0, s, g);
    E2EMV_CHECK_LAUNCH(ctx, "mv_tracks_weights_backward_kernel");
    E2EMV_HIP(ctx, hipStreamSynchronize(s));
    return E2EMV_OK;
}
