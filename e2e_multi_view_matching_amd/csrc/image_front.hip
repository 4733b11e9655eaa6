// The image front of a tuple on the device (MatchingDataset.__getitem__ of the reference, datasets/matching_dataset.py:182-211):
// ToTensor, the zero padding / square crop as ONE source window, the bilinear resize (antialias 0 | 1, aten's semantics),
// ColorJitter with one parameter row per image and rgb_to_grayscale.  uint8 RGB [B][Hin][Win][3] in, float32 gray
// [B][1][Hout][Wout] out (and, for audits, the jittered colour image [B][3][Hout][Wout]).
//
//   no image of the call has a contrast slot:   image_front_kernel<.., 2>                                          (1 launch)
//   otherwise:   image_front_kernel<.., 1> -> image_front_mean_kernel -> image_front_kernel<.., 2>                 (3 launches)
//
// A workgroup of 256 threads makes one tile of kTH x kTW output pixels, four pixels per thread (column = lane, so a wave
// writes 256 contiguous bytes of an output row).  The source rows the tile needs are walked in chunks of kRC rows:
//   (a) stage   the chunk's bytes come in as aligned 16-byte loads - a row is 3 * Win bytes and starts anywhere, so the first and
//               the last granule of a row are partly outside it: a granule is loaded only when at least one of its bytes belongs
//               to the row (it then lies in a page that is mapped) and every byte outside the image becomes 0.0 - become
//               u8 / 255 with the bytes of the true fp32 division (a product and one fused correction: x * (1 / 255) alone
//               differs on 126 values) and land as fp32 in LDS, at the position the byte has inside its granule row (`head` = the misalignment);
//   (b) rows    the horizontal taps of every (source row, output column) pair: LDS -> the intermediate H[row][channel][column] in LDS;
//   (c) columns every thread adds the chunk's rows to its 4 x 3 accumulators, each with the weight the row has for the pixel's
//               row (0 outside its vertical taps; the tile's horizontal weights and the chunk's vertical ones sit in LDS).
// A window of the output's size skips (b) and (c): the pixel is the staged value itself, no arithmetic touches it.
// The three channels stay in registers from there through the jitter to the gray value.
//
// The contrast blend needs the mean gray value of the whole image as it stands at that slot: pass 1 runs the resample and the
// ops in front of the contrast slot, leaves one fp32 partial sum per tile (summed in a fixed tree) and parks the resized colour
// pixels as fp32 in a workspace; one workgroup per image adds the partials in a fixed order in fp64; pass 2 takes the parked
// pixels back (images of the call without a contrast slot are not touched by pass 1 and are resampled in pass 2).  No atomics
// anywhere: a call gives the same bytes every time.  Resampling again in pass 2 instead of parking was measured too
// (0.46 / 0.53 ms on the device against 0.35 / 0.39 ms for 40 frames, antialias off / on): the kernel is bound by
// the arithmetic and the barriers of the resample, not by the 24 bytes per output pixel the workspace moves.
//
// Tap tables (xmin, xsize, weights per output column and row) are made on the host in fp64 per call shape and kept, with the
// two workspaces and the parameter rows, in a state of the context: nothing is allocated after the first call of a shape.
#include <climits>
#include <cmath>
#include <cstring>
#include <memory>

#include "common.h"
#include "u8_over_255.h"

namespace e2emv {

namespace {

constexpr int kThreads = 256;
constexpr int kTW = 64;         // output tile: columns (= lanes of a wave)
constexpr int kTH = 16;         //              rows (4 per thread)
constexpr int kRC = 8;          // source rows staged at a time
constexpr int kStripPx = E2EMV_IMAGE_FRONT_STRIP;  // source columns one tile may span
constexpr int kStripF = 3 * kStripPx + 32;         // floats of a staged row: its bytes, the head (< 16) and the granule round-up (< 16)
constexpr int kMaxTaps = 16;  // horizontal taps per output column (13 at the widest strip)
constexpr int kPixPerThread = kTH * kTW / kThreads;
static_assert(kPixPerThread == 4 && kThreads / kTW == 4, "thread t: column t % 64, rows t / 64 + 4 k");
static_assert(kTH % kRC == 0, "identity path: a chunk is a whole number of tile rows");

struct ImgParam {  // 48 bytes per image
    int32_t order[4];
    float f[4];    // brightness, contrast, saturation, hue
    float omf[4];  // float(1.0 - double(f)), torchvision's (1.0 - ratio)
};

struct Taps {  // one axis
    const int* mn;
    const int* sz;
    const float* w;  // [out][k]
    int k;
};

struct FrontArgs {
    const uint8_t* rgb;
    float* gray;
    float* rgb_out;
    const ImgParam* par;  // null: no jitter
    Taps tx, ty;
    int B, Hin, Win, top, left, Hout, Wout, tiles_x, tiles_y;
    float* partial;     // [B][tiles_x * tiles_y], written by pass 1
    const float* mean;  // [B], read by pass 2
    float* park;        // [B][3][Hout][Wout]: the resized colour image, written by pass 1, read by pass 2 (null: no contrast slot in the call)
};

__device__ __forceinline__ float clamp01(float x) { return fminf(fmaxf(x, 0.f), 1.f); }

// rgb_to_grayscale in torch's order of fp32 operations, every product and sum rounded on its own: where the output must be
// torch's bytes.  The library is built with -ffp-contract=fast, under which the back end fuses the inlined __fmul_rn /
// __fadd_rn into v_fma all the same (seen in the assembly): each product passes through an empty asm statement, which the
// compiler cannot look through.
__device__ __forceinline__ float gray_rn(float r, float g, float b) {
    float t0 = __fmul_rn(0.2989f, r), t1 = __fmul_rn(0.587f, g), t2 = __fmul_rn(0.114f, b);
    asm volatile("" : "+v"(t0), "+v"(t1), "+v"(t2));
    float s = __fadd_rn(t0, t1);
    asm volatile("" : "+v"(s));
    return __fadd_rn(s, t2);
}

// torchvision's adjust_hue on one pixel: _rgb2hsv, h = (h + f) mod 1, _hsv2rgb
__device__ __forceinline__ void hue_pixel(float hf, float& r, float& g, float& b) {
    const float maxc = fmaxf(r, fmaxf(g, b));
    const float minc = fminf(r, fminf(g, b));
    const bool eqc = maxc == minc;
    const float cr = maxc - minc;
    const float s = cr / (eqc ? 1.f : maxc);
    const float div = eqc ? 1.f : cr;
    const float rc = (maxc - r) / div, gc = (maxc - g) / div, bc = (maxc - b) / div;
    float h;
    if (maxc == r) h = bc - gc;
    else if (maxc == g) h = 2.f + rc - bc;
    else h = 4.f + gc - rc;
    h = fmodf(h / 6.f + 1.f, 1.f);
    h = h + hf;
    h = h - floorf(h);  // python's % 1.0 (may round to 1.0: i % 6 below takes it)
    const float h6 = h * 6.f;
    const float fi = floorf(h6);
    const float f = h6 - fi;
    int i = int(fi) % 6;
    if (i < 0) i += 6;
    const float v = maxc;
    const float p = clamp01(v * (1.f - s));
    const float q = clamp01(v * (1.f - s * f));
    const float t = clamp01(v * (1.f - s * (1.f - f)));
    switch (i) {
        case 0: r = v; g = t; b = p; break;
        case 1: r = q; g = v; b = p; break;
        case 2: r = p; g = v; b = t; break;
        case 3: r = p; g = q; b = v; break;
        case 4: r = t; g = p; b = v; break;
        default: r = v; g = p; b = q; break;
    }
}

// The slots of one image on one pixel.  UNTIL_CONTRAST: stop in front of the contrast slot (pass 1).
template <bool UNTIL_CONTRAST>
__device__ __forceinline__ void jitter_pixel(const ImgParam& P, unsigned slots, float mean, float& r, float& g, float& b) {
#pragma unroll 1
    for (int slot = 0; slot < 4; ++slot) {
        const int op = int((slots >> (8 * slot)) & 255u);  // (255: a skipped slot)
        if (op == 0) {
            r = clamp01(P.f[0] * r); g = clamp01(P.f[0] * g); b = clamp01(P.f[0] * b);
        } else if (op == 1) {
            if (UNTIL_CONTRAST) return;
            const float m = P.omf[1] * mean;
            r = clamp01(P.f[1] * r + m); g = clamp01(P.f[1] * g + m); b = clamp01(P.f[1] * b + m);
        } else if (op == 2) {
            const float m = P.omf[2] * gray_rn(r, g, b);
            r = clamp01(P.f[2] * r + m); g = clamp01(P.f[2] * g + m); b = clamp01(P.f[2] * b + m);
        } else if (op == 3) {
            hue_pixel(P.f[3], r, g, b);
        }
    }
}

__device__ __forceinline__ bool has_contrast(const ImgParam& P) {
    return P.order[0] == 1 || P.order[1] == 1 || P.order[2] == 1 || P.order[3] == 1;
}

// (ToTensor's u8 / 255 with the bytes of the true fp32 division: u8_over_255 of u8_over_255.h, shared with image_front_pairs.hip)

typedef unsigned int u4 __attribute__((ext_vector_type(4)));
typedef float f4 __attribute__((ext_vector_type(4)));

// IDENT: the window has the output's size.  PASS 1: partial gray sums in front of the contrast slot; PASS 2: the outputs.
template <bool IDENT, int PASS>
__global__ __launch_bounds__(kThreads) void image_front_kernel(const FrontArgs a) {
    __shared__ __attribute__((aligned(16))) float S[kRC][kStripF];
    __shared__ float H[kRC][3][kTW];
    __shared__ float WX[kMaxTaps][kTW];  // the horizontal weights of the tile's columns (0 beyond a column's taps)
    __shared__ float WY[kTH][kRC];       // the vertical weight of (tile row, chunk row), 0 outside the row's tap range
    __shared__ float red[kThreads];

    const int tid = threadIdx.x;
    const int tiles = a.tiles_x * a.tiles_y;
    const int b = blockIdx.x / tiles;
    const int tile = blockIdx.x - b * tiles;
    const int tile_y = tile / a.tiles_x;
    const int tile_x = tile - tile_y * a.tiles_x;

    ImgParam P;
    P.order[0] = P.order[1] = P.order[2] = P.order[3] = -1;
    if (a.par) P = a.par[b];
    if (PASS == 1 && !has_contrast(P)) return;  // (the whole workgroup: nobody waits at a barrier)
    // the four slots in one register: a loop over an array would put it into scratch memory
    const unsigned slots = (unsigned(P.order[0]) & 255u) | (unsigned(P.order[1]) & 255u) << 8 | (unsigned(P.order[2]) & 255u) << 16 |
                           (unsigned(P.order[3]) & 255u) << 24;

    const int x0 = tile_x * kTW, y0 = tile_y * kTH;
    const int xl = min(x0 + kTW, a.Wout) - 1, yl = min(y0 + kTH, a.Hout) - 1;
    // the source rectangle of the tile, in window coordinates
    const int sx0 = IDENT ? x0 : a.tx.mn[x0];
    const int sx1 = IDENT ? xl + 1 : a.tx.mn[xl] + a.tx.sz[xl];
    const int sy0 = IDENT ? y0 : a.ty.mn[y0];
    const int sy1 = IDENT ? yl + 1 : a.ty.mn[yl] + a.ty.sz[yl];
    const int strip_bytes = 3 * (sx1 - sx0);
    const int off0 = 3 * (a.left + sx0);  // byte of the strip's first pixel inside its image row (may be negative)
    const int row_bytes = 3 * a.Win;
    const int max_granules = (strip_bytes + 15 + 15) >> 4;
    const uint8_t* img = a.rgb + size_t(b) * a.Hin * row_bytes;

    // this thread's pixels: column cx, rows y0 + q + 4 k
    const int cx = tid & (kTW - 1), q = tid >> 6;
    const int x = x0 + cx;
    const bool col_ok = x <= xl;
    int xmn = 0, xsz = 0;
    if (!IDENT && col_ok) { xmn = a.tx.mn[x]; xsz = a.tx.sz[x]; }
    if (!IDENT)
        for (int j = q; j < a.tx.k; j += kThreads / kTW) WX[j][cx] = (col_ok && j < xsz) ? a.tx.w[size_t(x) * a.tx.k + j] : 0.f;
    float acc[kPixPerThread][3];
#pragma unroll
    for (int k = 0; k < kPixPerThread; ++k) acc[k][0] = acc[k][1] = acc[k][2] = 0.f;

    // pass 2 of an image with a contrast slot: pass 1 has parked the resized pixels, nothing is resampled
    const bool from_park = PASS == 2 && a.park && has_contrast(P);
    const int sy_end = from_park ? sy0 : sy1;
    for (int r0 = sy0; r0 < sy_end; r0 += kRC) {
        const int nr = min(kRC, sy1 - r0);
        __syncthreads();  // WX (first round); S, H and WY of the round before are no longer read
        if (!IDENT && tid < kTH * kRC) {
            const int yy = tid / kRC, i = tid - yy * kRC;
            const int y = y0 + yy, r = r0 + i;
            float w = 0.f;
            if (y <= yl && i < nr) {
                const int mn = a.ty.mn[y];
                if (r >= mn && r < mn + a.ty.sz[y]) w = a.ty.w[size_t(y) * a.ty.k + (r - mn)];
            }
            WY[yy][i] = w;
        }
        // ---- (a) stage: granule g of chunk row i
        for (int t = tid; t < nr * max_granules; t += kThreads) {
            const int i = t / max_granules, g = t - i * max_granules;
            const int iy = a.top + r0 + i;
            const bool row_ok = iy >= 0 && iy < a.Hin;
            const uint8_t* rowp = img + size_t(row_ok ? iy : 0) * row_bytes;
            const int head = row_ok ? int((reinterpret_cast<uintptr_t>(rowp) + off0) & 15) : 0;
            if (g * 16 >= head + strip_bytes) continue;
            const int p0 = off0 - head + 16 * g;  // byte of the image row the granule starts at (16-byte aligned address)
            f4 v[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = f4{0.f, 0.f, 0.f, 0.f};
            if (row_ok && p0 + 16 > 0 && p0 < row_bytes) {  // at least one byte of the row: the granule's page is mapped
                const u4 raw = *reinterpret_cast<const u4*>(rowp + p0);
                if (p0 >= 0 && p0 + 16 <= row_bytes) {  // all of it inside the row
#pragma unroll
                    for (int e = 0; e < 16; ++e) v[e >> 2][e & 3] = u8_over_255((raw[e >> 2] >> (8 * (e & 3))) & 255u);
                } else {
#pragma unroll
                    for (int e = 0; e < 16; ++e) {
                        const int p = p0 + e;
                        v[e >> 2][e & 3] = (p >= 0 && p < row_bytes) ? u8_over_255((raw[e >> 2] >> (8 * (e & 3))) & 255u) : 0.f;
                    }
                }
            }
            f4* dst = reinterpret_cast<f4*>(&S[i][16 * g]);
#pragma unroll
            for (int e = 0; e < 4; ++e) dst[e] = v[e];
        }
        __syncthreads();
        if (IDENT) {
#pragma unroll
            for (int k = 0; k < kPixPerThread; ++k) {
                const int y = y0 + q + 4 * k;
                if (col_ok && y >= r0 && y < r0 + nr) {
                    const int i = y - r0;
                    const int iy = a.top + y;
                    const bool row_ok = iy >= 0 && iy < a.Hin;
                    const int head = row_ok ? int((reinterpret_cast<uintptr_t>(img + size_t(iy) * row_bytes) + off0) & 15) : 0;
                    const float* s = &S[i][head + 3 * cx];
                    acc[k][0] = s[0]; acc[k][1] = s[1]; acc[k][2] = s[2];
                }
            }
            continue;
        }
        // ---- (b) the horizontal taps of (row i, column cx)
        for (int i = q; i < nr; i += kThreads / kTW) {
            float r = 0.f, g = 0.f, bl = 0.f;
            if (col_ok) {
                const int iy = a.top + r0 + i;
                const bool row_ok = iy >= 0 && iy < a.Hin;
                const int head = row_ok ? int((reinterpret_cast<uintptr_t>(img + size_t(iy) * row_bytes) + off0) & 15) : 0;
                const float* s = &S[i][head + 3 * (xmn - sx0)];
                for (int j = 0; j < xsz; ++j) {
                    const float wj = WX[j][cx];
                    r = fmaf(wj, s[3 * j], r); g = fmaf(wj, s[3 * j + 1], g); bl = fmaf(wj, s[3 * j + 2], bl);
                }
            }
            H[i][0][cx] = r; H[i][1][cx] = g; H[i][2][cx] = bl;
        }
        __syncthreads();
        // ---- (c) every row of the chunk into the thread's pixels, with the weight the row has for the pixel's row (0 outside its taps)
#pragma unroll
        for (int i = 0; i < kRC; ++i) {
            if (i < nr) {
                const float h0 = H[i][0][cx], h1 = H[i][1][cx], h2 = H[i][2][cx];
#pragma unroll
                for (int k = 0; k < kPixPerThread; ++k) {
                    const float w = WY[q + 4 * k][i];
                    acc[k][0] = fmaf(w, h0, acc[k][0]);
                    acc[k][1] = fmaf(w, h1, acc[k][1]);
                    acc[k][2] = fmaf(w, h2, acc[k][2]);
                }
            }
        }
    }

    if ((PASS == 1 && a.park) || from_park) {  // park the resized pixels as fp32 / take them back
        const size_t pl = size_t(a.Hout) * a.Wout;
#pragma unroll
        for (int k = 0; k < kPixPerThread; ++k) {
            const int y = y0 + q + 4 * k;
            if (!col_ok || y > yl) continue;
            float* c = a.park + size_t(b) * 3 * pl + size_t(y) * a.Wout + x;
            if (PASS == 1) { c[0] = acc[k][0]; c[pl] = acc[k][1]; c[2 * pl] = acc[k][2]; }
            else { acc[k][0] = c[0]; acc[k][1] = c[pl]; acc[k][2] = c[2 * pl]; }
        }
    }
    // ---- jitter, gray, output
    const float mean = (PASS == 2 && a.mean) ? a.mean[b] : 0.f;
    float part = 0.f;
    const size_t plane = size_t(a.Hout) * a.Wout;
#pragma unroll
    for (int k = 0; k < kPixPerThread; ++k) {
        const int y = y0 + q + 4 * k;
        if (!col_ok || y > yl) continue;
        float r = acc[k][0], g = acc[k][1], bl = acc[k][2];
        if (a.par) jitter_pixel<PASS == 1>(P, slots, mean, r, g, bl);
        const float gr = gray_rn(r, g, bl);
        if (PASS == 1) {
            part += gr;
        } else {
            const size_t o = size_t(y) * a.Wout + x;
            a.gray[size_t(b) * plane + o] = gr;
            if (a.rgb_out) {
                float* c = a.rgb_out + size_t(b) * 3 * plane + o;
                c[0] = r; c[plane] = g; c[2 * plane] = bl;
            }
        }
    }
    if (PASS == 1) {  // the tile's sum, in a fixed tree
        red[tid] = part;
        __syncthreads();
        for (int s = kThreads / 2; s > 0; s >>= 1) {
            if (tid < s) red[tid] += red[tid + s];
            __syncthreads();
        }
        if (tid == 0) a.partial[size_t(b) * tiles + tile] = red[0];
    }
}

// one workgroup per image: the partial sums of its tiles in a fixed order, fp64
__global__ __launch_bounds__(kThreads) void image_front_mean_kernel(const ImgParam* __restrict__ par, const float* __restrict__ partial,
                                                                      int tiles, double inv_pixels, float* __restrict__ mean) {
    __shared__ double red[kThreads];
    const int b = blockIdx.x, tid = threadIdx.x;
    if (!has_contrast(par[b])) return;
    double s = 0.0;
    for (int t = tid; t < tiles; t += kThreads) s += double(partial[size_t(b) * tiles + t]);
    red[tid] = s;
    __syncthreads();
    for (int h = kThreads / 2; h > 0; h >>= 1) {
        if (tid < h) red[tid] += red[tid + h];
        __syncthreads();
    }
    if (tid == 0) mean[b] = float(red[0] * inv_pixels);
}

// ---- host ----
struct AxisTaps {
    std::vector<int> mn, sz;
    std::vector<float> w;
    int k = 0;
};

// aten's tap tables of one axis, in fp64 (torch.nn.functional.interpolate, mode="bilinear", align_corners=False)
void make_taps(int in, int out, int antialias, AxisTaps* T) {
    const double scale = double(in) / double(out);
    T->mn.assign(out, 0);
    T->sz.assign(out, 0);
    if (!antialias) {  // upsample_bilinear2d: source index clamped at 0, the second tap dropped at the last pixel
        T->k = 2;
        T->w.assign(size_t(out) * 2, 0.f);
        for (int i = 0; i < out; ++i) {
            double src = scale * (i + 0.5) - 0.5;
            if (src < 0.0) src = 0.0;
            int i0 = int(src);
            if (i0 > in - 1) i0 = in - 1;
            const double l1 = src - i0;
            T->mn[i] = i0;
            if (i0 < in - 1) {
                T->sz[i] = 2;
                T->w[2 * size_t(i)] = float(1.0 - l1);
                T->w[2 * size_t(i) + 1] = float(l1);
            } else {
                T->sz[i] = 1;
                T->w[2 * size_t(i)] = 1.f;
            }
        }
        return;
    }
    // _upsample_bilinear2d_aa: triangle filter, support 0.5 * max(scale, 1) * 2, weights normalised by their sum
    const double support = scale >= 1.0 ? scale : 1.0;
    const double invscale = scale >= 1.0 ? 1.0 / scale : 1.0;
    const int k = int(std::ceil(support)) * 2 + 1;
    T->k = k;
    T->w.assign(size_t(out) * k, 0.f);
    std::vector<double> w(k);
    for (int i = 0; i < out; ++i) {
        const double center = scale * (i + 0.5);
        long long xmin = (long long)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        long long xsize = (long long)(center + support + 0.5);
        if (xsize > in) xsize = in;
        xsize -= xmin;
        if (xsize < 0) xsize = 0;
        if (xsize > k) xsize = k;
        double total = 0.0;
        for (int j = 0; j < xsize; ++j) {
            double v = std::fabs((j + xmin - center + 0.5) * invscale);
            w[j] = v < 1.0 ? 1.0 - v : 0.0;
            total += w[j];
        }
        int n = int(xsize);
        while (n > 1 && w[n - 1] == 0.0) --n;  // (a tap of weight 0 at the end of the support: not read)
        for (int j = 0; j < n; ++j) T->w[size_t(i) * k + j] = float(total != 0.0 ? w[j] / total : w[j]);
        T->mn[i] = int(xmin);
        T->sz[i] = n;
    }
}

struct FrontShape {  // the device tables of one (window size, output size, antialias)
    int wh, ww, Hout, Wout, aa;
    char* d = nullptr;
    std::vector<char> h;  // what was uploaded (kept: the source of the stream-ordered copy)
    Taps tx{}, ty{};
};

constexpr int kParamSlots = 8;

struct ImageFrontState {
    std::vector<std::unique_ptr<FrontShape>> shapes;
    float* d_partial = nullptr;  // [B * tiles] partial sums, then [B] means
    size_t partial_floats = 0;
    float* d_park = nullptr;  // [B][3][Hout][Wout] fp32: the resized colour image between pass 1 and pass 2
    size_t park_floats = 0;
    ImgParam* d_par = nullptr;
    int par_rows = 0;
    // pinned staging of the parameter rows: a ring, so that a call does not wait for the copy of the call before it
    ImgParam* h_par[kParamSlots] = {nullptr};
    int h_rows[kParamSlots] = {0};
    hipEvent_t copied[kParamSlots] = {nullptr};
    bool pending[kParamSlots] = {false};
    int next = 0;
};

ImageFrontState* front_state(e2emv_ctx* ctx) {
    if (!ctx->image_front) ctx->image_front = new ImageFrontState();
    return static_cast<ImageFrontState*>(ctx->image_front);
}

size_t align256(size_t n) { return (n + 255) & ~size_t(255); }

int front_shape(e2emv_ctx* ctx, ImageFrontState* st, const e2emv_image_front_desc& d, bool ident, hipStream_t s, FrontShape** out) {
    for (auto& p : st->shapes)
        if (p->wh == d.win_height && p->ww == d.win_width && p->Hout == d.out_height && p->Wout == d.out_width && p->aa == d.antialias) {
            *out = p.get();
            return E2EMV_OK;
        }
    std::unique_ptr<FrontShape> F(new FrontShape());
    F->wh = d.win_height; F->ww = d.win_width; F->Hout = d.out_height; F->Wout = d.out_width; F->aa = d.antialias;
    if (!ident) {
        AxisTaps X, Y;
        make_taps(d.win_width, d.out_width, d.antialias, &X);
        make_taps(d.win_height, d.out_height, d.antialias, &Y);
        for (int x0 = 0; x0 < d.out_width; x0 += kTW) {  // what one tile reads of a source row has to fit its LDS strip
            const int xl = std::min(x0 + kTW, d.out_width) - 1;
            int lo = INT_MAX, hi = 0;
            for (int x = x0; x <= xl; ++x) {
                lo = std::min(lo, X.mn[x]);
                hi = std::max(hi, X.mn[x] + X.sz[x]);
            }
            if (lo != X.mn[x0] || hi != X.mn[xl] + X.sz[xl] || hi - lo > kStripPx || hi - lo < 1)
                return set_err(ctx, E2EMV_ESHAPE, "e2emv_image_front: %d output columns need %d source columns, more than the %d of a tile (width %d -> %d)",
                               xl - x0 + 1, hi - lo, kStripPx, d.win_width, d.out_width);
        }
        if (X.k > kMaxTaps)
            return set_err(ctx, E2EMV_ESHAPE, "e2emv_image_front: %d horizontal taps per column, more than %d (width %d -> %d)", X.k, kMaxTaps, d.win_width, d.out_width);
        for (int y = 0; y + 1 < d.out_height; ++y)
            if (Y.mn[y + 1] < Y.mn[y] || Y.mn[y + 1] + Y.sz[y + 1] < Y.mn[y] + Y.sz[y])
                return set_err(ctx, E2EMV_ESHAPE, "e2emv_image_front: the vertical tap ranges are not monotone (height %d -> %d)", d.win_height, d.out_height);
        size_t off[6], n = 0;
        const size_t bytes[6] = {X.mn.size() * 4, X.sz.size() * 4, X.w.size() * 4, Y.mn.size() * 4, Y.sz.size() * 4, Y.w.size() * 4};
        for (int i = 0; i < 6; ++i) { off[i] = n; n += align256(bytes[i]); }
        F->h.assign(n, 0);
        const void* src[6] = {X.mn.data(), X.sz.data(), X.w.data(), Y.mn.data(), Y.sz.data(), Y.w.data()};
        for (int i = 0; i < 6; ++i) std::memcpy(F->h.data() + off[i], src[i], bytes[i]);
        if (hipMalloc((void**)&F->d, n) != hipSuccess) {
            (void)hipGetLastError();
            return set_err(ctx, E2EMV_ENOMEM, "e2emv_image_front: tap tables of %zu bytes", n);
        }
        if (hipMemcpyAsync(F->d, F->h.data(), n, hipMemcpyHostToDevice, s) != hipSuccess) {
            (void)hipGetLastError();
            (void)hipFree(F->d);
            return set_err(ctx, E2EMV_EHIP, "e2emv_image_front: upload of the tap tables failed");
        }
        F->tx = Taps{(const int*)(F->d + off[0]), (const int*)(F->d + off[1]), (const float*)(F->d + off[2]), X.k};
        F->ty = Taps{(const int*)(F->d + off[3]), (const int*)(F->d + off[4]), (const float*)(F->d + off[5]), Y.k};
    }
    *out = F.get();
    st->shapes.push_back(std::move(F));
    return E2EMV_OK;
}

// One parameter row per image from the caller's HOST arrays; EINVAL with a message for what ColorJitter cannot mean.
int front_params(e2emv_ctx* ctx, int B, const int32_t* order, const float* factors, std::vector<ImgParam>* rows, bool* any_contrast) {
    static const char* names[4] = {"brightness", "contrast", "saturation", "hue"};
    rows->resize(B);
    *any_contrast = false;
    for (int b = 0; b < B; ++b) {
        ImgParam& P = (*rows)[b];
        int seen = 0;
        for (int k = 0; k < 4; ++k) {
            const int op = order[4 * b + k];
            if (op < -1 || op > 3) return set_err(ctx, E2EMV_EINVAL, "e2emv_image_front: order[%d][%d] = %d, not in -1..3", b, k, op);
            if (op >= 0) {
                if (seen & (1 << op)) return set_err(ctx, E2EMV_EINVAL, "e2emv_image_front: order[%d] names %s twice", b, names[op]);
                seen |= 1 << op;
            }
            P.order[k] = op;
            const float f = factors[4 * b + k];
            if (!std::isfinite(f)) return set_err(ctx, E2EMV_EINVAL, "e2emv_image_front: the %s factor of image %d is not finite", names[k], b);
            if (k < 3 && f < 0.f) return set_err(ctx, E2EMV_EINVAL, "e2emv_image_front: the %s factor of image %d is negative (%g)", names[k], b, double(f));
            if (k == 3 && (f < -0.5f || f > 0.5f))
                return set_err(ctx, E2EMV_EINVAL, "e2emv_image_front: the hue factor of image %d is %g, outside [-0.5, 0.5]", b, double(f));
            P.f[k] = f;
            P.omf[k] = float(1.0 - double(f));
        }
        if (seen & 2) *any_contrast = true;
    }
    return E2EMV_OK;
}

int front_upload_params(e2emv_ctx* ctx, ImageFrontState* st, const std::vector<ImgParam>& rows, hipStream_t s) {
    const int B = int(rows.size());
    if (B > st->par_rows) {
        E2EMV_HIP(ctx, hipStreamSynchronize(s));  // kernels of an earlier call may still read the old rows
        if (st->d_par) E2EMV_HIP(ctx, hipFree(st->d_par));
        st->d_par = nullptr;
        st->par_rows = 0;
        if (hipMalloc((void**)&st->d_par, size_t(B) * sizeof(ImgParam)) != hipSuccess) {
            (void)hipGetLastError();
            st->d_par = nullptr;
            return set_err(ctx, E2EMV_ENOMEM, "e2emv_image_front: %d parameter rows", B);
        }
        st->par_rows = B;
    }
    const int k = st->next;
    st->next = (k + 1) % kParamSlots;
    if (st->pending[k]) {
        E2EMV_HIP(ctx, hipEventSynchronize(st->copied[k]));  // (the copy of kParamSlots calls ago)
        st->pending[k] = false;
    }
    if (!st->copied[k]) E2EMV_HIP(ctx, hipEventCreateWithFlags(&st->copied[k], hipEventDisableTiming));
    if (B > st->h_rows[k]) {
        if (st->h_par[k]) E2EMV_HIP(ctx, hipHostFree(st->h_par[k]));
        st->h_par[k] = nullptr;
        st->h_rows[k] = 0;
        if (hipHostMalloc((void**)&st->h_par[k], size_t(B) * sizeof(ImgParam), hipHostMallocDefault) != hipSuccess) {
            (void)hipGetLastError();
            st->h_par[k] = nullptr;
            return set_err(ctx, E2EMV_ENOMEM, "e2emv_image_front: pinned staging of %d parameter rows", B);
        }
        st->h_rows[k] = B;
    }
    std::memcpy(st->h_par[k], rows.data(), size_t(B) * sizeof(ImgParam));
    E2EMV_HIP(ctx, hipMemcpyAsync(st->d_par, st->h_par[k], size_t(B) * sizeof(ImgParam), hipMemcpyHostToDevice, s));
    E2EMV_HIP(ctx, hipEventRecord(st->copied[k], s));
    st->pending[k] = true;
    return E2EMV_OK;
}

template <bool IDENT>
void launch_front(int pass, int grid, hipStream_t s, const FrontArgs& a) {
    if (pass == 1) hipLaunchKernelGGL((image_front_kernel<IDENT, 1>), dim3(grid), dim3(kThreads), 0, s, a);
    else hipLaunchKernelGGL((image_front_kernel<IDENT, 2>), dim3(grid), dim3(kThreads), 0, s, a);
}

}  // namespace

void image_front_free(e2emv_ctx* ctx) {
    ImageFrontState* st = static_cast<ImageFrontState*>(ctx->image_front);
    if (!st) return;
    for (auto& p : st->shapes)
        if (p->d) (void)hipFree(p->d);
    if (st->d_partial) (void)hipFree(st->d_partial);
    if (st->d_park) (void)hipFree(st->d_park);
    if (st->d_par) (void)hipFree(st->d_par);
    for (int k = 0; k < kParamSlots; ++k) {
        if (st->h_par[k]) (void)hipHostFree(st->h_par[k]);
        if (st->copied[k]) (void)hipEventDestroy(st->copied[k]);
    }
    delete st;
    ctx->image_front = nullptr;
}

}  // namespace e2emv

using namespace e2emv;

extern "C" {

int e2emv_image_front(e2emv_ctx* ctx, const e2emv_image_front_desc* desc, const uint8_t* d_rgb, const int32_t* order, const float* factors,
                      float* d_gray, float* d_rgb_out, void* stream) {
    if (!ctx) return E2EMV_EINVAL;
    if (!desc || !d_rgb || !d_gray) return set_err(ctx, E2EMV_EINVAL, "e2emv_image_front: NULL argument");
    if ((order == nullptr) != (factors == nullptr)) return set_err(ctx, E2EMV_EINVAL, "e2emv_image_front: order and factors go together");
    const e2emv_image_front_desc d = *desc;
    if (d.batch <= 0 || d.in_height <= 0 || d.in_width <= 0 || d.out_height <= 0 || d.out_width <= 0)
        return set_err(ctx, E2EMV_EINVAL, "e2emv_image_front: batch %d, input %d x %d, output %d x %d: sizes must be positive", d.batch, d.in_height,
                       d.in_width, d.out_height, d.out_width);
    if (d.win_height <= 0 || d.win_width <= 0)
        return set_err(ctx, E2EMV_EINVAL, "e2emv_image_front: empty window (%d x %d)", d.win_height, d.win_width);
    if (d.antialias != 0 && d.antialias != 1) return set_err(ctx, E2EMV_EINVAL, "e2emv_image_front: antialias = %d", d.antialias);
    const int64_t lim = INT_MAX / 4;  // (byte offsets inside a row and window coordinates are ints in the kernel)
    if (d.in_width > lim || d.win_width > lim || d.win_height > lim || std::llabs((long long)d.win_left) > lim || std::llabs((long long)d.win_top) > lim ||
        int64_t(d.win_left) + d.win_width > lim || int64_t(d.win_top) + d.win_height > lim)
        return set_err(ctx, E2EMV_ESHAPE, "e2emv_image_front: image or window too large");
    const int tiles_x = (d.out_width + kTW - 1) / kTW, tiles_y = (d.out_height + kTH - 1) / kTH;
    const int64_t grid = int64_t(d.batch) * tiles_x * tiles_y;
    if (grid > INT_MAX) return set_err(ctx, E2EMV_ESHAPE, "e2emv_image_front: %lld tiles", (long long)grid);
    std::vector<ImgParam> rows;
    bool any_contrast = false;
    if (order) {
        int rc = front_params(ctx, d.batch, order, factors, &rows, &any_contrast);
        if (rc) return rc;
    }
    const bool ident = d.win_height == d.out_height && d.win_width == d.out_width;

    E2EMV_ENTER(ctx, stream);
    hipStream_t s = (hipStream_t)stream;
    ImageFrontState* st = front_state(ctx);
    FrontShape* F = nullptr;
    int rc = front_shape(ctx, st, d, ident, s, &F);
    if (rc) return rc;
    if (order) {
        rc = front_upload_params(ctx, st, rows, s);
        if (rc) return rc;
    }
    const int tiles = tiles_x * tiles_y;
    if (any_contrast) {
        const size_t want = size_t(grid) + size_t(d.batch);
        if (want > st->partial_floats) {
            E2EMV_HIP(ctx, hipStreamSynchronize(s));
            if (st->d_partial) E2EMV_HIP(ctx, hipFree(st->d_partial));
            st->d_partial = nullptr;
            st->partial_floats = 0;
            if (hipMalloc((void**)&st->d_partial, want * sizeof(float)) != hipSuccess) {
                (void)hipGetLastError();
                st->d_partial = nullptr;
                return set_err(ctx, E2EMV_ENOMEM, "e2emv_image_front: %zu partial sums", want);
            }
            st->partial_floats = want;
        }
        const size_t park = size_t(d.batch) * 3 * d.out_height * d.out_width;
        if (park > st->park_floats) {
            E2EMV_HIP(ctx, hipStreamSynchronize(s));
            if (st->d_park) E2EMV_HIP(ctx, hipFree(st->d_park));
            st->d_park = nullptr;
            st->park_floats = 0;
            if (hipMalloc((void**)&st->d_park, park * sizeof(float)) != hipSuccess) {
                (void)hipGetLastError();
                st->d_park = nullptr;
                return set_err(ctx, E2EMV_ENOMEM, "e2emv_image_front: workspace of %zu bytes for the resized colour image", park * sizeof(float));
            }
            st->park_floats = park;
        }
    }
    FrontArgs a{};
    a.rgb = d_rgb; a.gray = d_gray; a.rgb_out = d_rgb_out;
    a.par = order ? st->d_par : nullptr;
    a.tx = F->tx; a.ty = F->ty;
    a.B = d.batch; a.Hin = d.in_height; a.Win = d.in_width; a.top = d.win_top; a.left = d.win_left;
    a.Hout = d.out_height; a.Wout = d.out_width; a.tiles_x = tiles_x; a.tiles_y = tiles_y;
    a.partial = st->d_partial;
    a.mean = any_contrast ? st->d_partial + size_t(grid) : nullptr;
    a.park = any_contrast ? st->d_park : nullptr;
    prof_begin(ctx, PS_MISC, s);
    if (any_contrast) {
        if (ident) launch_front<true>(1, int(grid), s, a); else launch_front<false>(1, int(grid), s, a);
        E2EMV_CHECK_LAUNCH(ctx, "image_front_kernel (pass 1)");
        prof_begin(ctx, PS_MISC, s);
        hipLaunchKernelGGL(image_front_mean_kernel, dim3(d.batch), dim3(kThreads), 0, s, st->d_par, st->d_partial, tiles,
                           1.0 / (double(d.out_height) * double(d.out_width)), st->d_partial + size_t(grid));
        E2EMV_CHECK_LAUNCH(ctx, "image_front_mean_kernel");
        prof_begin(ctx, PS_MISC, s);
    }
    if (ident) launch_front<true>(2, int(grid), s, a); else launch_front<false>(2, int(grid), s, a);
    E2EMV_CHECK_LAUNCH(ctx, "image_front_kernel");
    return E2EMV_OK;
}

}  // extern "C"
