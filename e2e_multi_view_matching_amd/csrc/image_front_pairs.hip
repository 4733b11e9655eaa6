// The image front of pair evaluation on the device (PairMatchingDataset.__getitem__ of the reference, eval_pairs.py:85-108):
// np.rot90, cv2.resize (INTER_LINEAR on a float32 image) and / 255. for a LIST of decoded gray frames of any sizes, each with
// its number of quarter turns.  uint8 [H][W] per image in, float32 [h_out][w_out] per image out, one behind the other in one
// buffer: one launch for the whole list.
//
// A workgroup of 256 threads makes one tile of kTH x kTW output pixels of one image, four pixels per thread; it finds its
// (image, tile) by a binary search over the first-tile column of the call's image table.
//
// The turn is never carried out: a pixel (r, c) of the TURNED image is the stored pixel
//     rot 0: (r, c)     rot 1: (c, W-1-r)     rot 2: (H-1-r, W-1-c)     rot 3: (H-1-c, r)
// so one turned axis runs along the stored rows' index (the LINE axis: the turned rows for an even turn, the turned columns
// for an odd one) and the other along the stored columns (the SPAN axis), each possibly mirrored.  What a tile reads is a set
// of stored rows (its lines) and one range of stored columns (its span):
//   lines  every output index of the tile on the line axis has two taps, s and s + 1.  Where the taps of the tile cover no
//          more than 2 * (its outputs) lines - every enlargement and reductions up to 2 - the covered range is staged as it
//          is (slot = line - first line); beyond that only the tapped lines are (slot = 2 * output + tap), so that a
//          reduction by 8 stages 64 lines, not 250;
//   span   the stored columns between the first and the last tap on the span axis.
//   (a) stage   every line's span comes in along the STORED row, as aligned 16-byte loads (consecutive threads take consecutive
//               granules of a line) - for odd turns too, where an output row walks a stored column.  A row starts anywhere,
//               so the first and the last granule of a span are partly outside it; a granule is loaded only when at least
//               one of its bytes belongs to the span (it then lies in a page that is mapped), and the bytes outside are never
//               read back.  The bytes land in LDS as they are, at the position they have inside their granule row; a line's
//               pitch is an odd number of dwords, so that the 32 lanes that walk a stored column (odd turns) hit 32 banks.
//   (b) taps    every thread reads the 2 x 2 bytes of each of its pixels from LDS: the horizontal taps on the values 0..255
//               first, then the vertical ones, then the fp32 division by 255 - OpenCV's order.  An image that is not resized
//               takes u8_over_255 of its one byte, the bytes of the true division (shared with image_front.hip).
// Tap positions and weights are computed in the kernel by the arithmetic of OpenCV's resize (tap_of below, the same
// function the host uses to size the staging): no tables.  No atomics: a call gives the same bytes every time.
//
// The kernel moves 1 byte in and 4 bytes out per output pixel at scale 1 and does about 20 operations on it: it is bound by
// the traffic and by LDS, and at the sizes of an evaluation pair (two frames of ~1 MB) by the launch itself.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "common.h"
#include "u8_over_255.h"

namespace e2emv {

namespace {

constexpr int kThreads = 256;
constexpr int kTH = E2EMV_IMAGE_FRONT_GRAY_TILE_ROWS;
constexpr int kTW = E2EMV_IMAGE_FRONT_GRAY_TILE_COLS;
constexpr int kMaxImages = E2EMV_IMAGE_FRONT_GRAY_MAX_IMAGES;
constexpr int kMaxSide = 16384;
constexpr int kPixPerThread = kTH * kTW / kThreads;
constexpr int kRowStep = kThreads / kTW;          // thread t: column t % kTW, rows t / kTW + kRowStep * k
constexpr int kMaxSlots = 2 * (kTH > kTW ? kTH : kTW);  // lines a tile stages at most
constexpr int kLdsDwords = 6144;                  // 24 KB of staged bytes
constexpr int kRing = 8;
static_assert(kPixPerThread == 4 && kTW == 32 && kTH == 32, "thread t: column t % 32, rows t / 32 + 8 k");
static_assert(kMaxSlots <= kThreads && kTH + kTW <= kThreads, "one thread per slot / per tap of the tile");

struct GrayImage {  // 64 bytes per image: the table of a call
    const uint8_t* src;
    float* dst;
    double scale_y, scale_x;  // per axis of the TURNED image: 1.0 / (double(n_out) / double(n_in))
    int32_t H, W;             // as stored
    int32_t rot;
    int32_t h_out, w_out;
    int32_t tiles_x;
    int32_t first_tile;       // of the call's tiles, the first one of this image
    int32_t ident;            // not resized
};
static_assert(sizeof(GrayImage) == 64, "the table row");

struct Tap {
    int s;
    float f;
};

// OpenCV's tap of output index d on an axis of n_in pixels (resizeLinear's table, for a float32 image): the position in
// double, ONE rounding to float32, the fraction in float32.  The product and the difference stay two roundings.
__host__ __device__ inline Tap tap_of(int d, double scale, int n_in) {
    double t = (double(d) + 0.5) * scale;
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("" : "+v"(t));  // (-ffp-contract=fast would fuse the product into the difference)
#else
    volatile double keep = t;
    t = keep;
#endif
    float f = float(t - 0.5);
    int s = int(floorf(f));
    f -= float(s);
    if (s < 0) { s = 0; f = 0.f; }
    if (s >= n_in - 1) { s = n_in - 1; f = 0.f; }
    return Tap{s, f};
}

typedef unsigned int u4 __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(kThreads) void image_front_gray_kernel(const GrayImage* __restrict__ tab, int n) {
    __shared__ uint32_t S[kLdsDwords];
    __shared__ int TYs[kTH], TXs[kTW];
    __shared__ float TYf[kTH], TXf[kTW];
    __shared__ int SlotRow[kMaxSlots], SlotOff[kMaxSlots];

    const int tid = threadIdx.x;
    const int wg = blockIdx.x;
    int lo = 0, hi = n - 1;  // the last image whose first tile is <= wg
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (tab[mid].first_tile <= wg) lo = mid; else hi = mid - 1;
    }
    const GrayImage g = tab[lo];
    const int tile = wg - g.first_tile;
    const int tile_y = tile / g.tiles_x, tile_x = tile - tile_y * g.tiles_x;
    const int y0 = tile_y * kTH, x0 = tile_x * kTW;
    const int ny = min(kTH, g.h_out - y0), nx = min(kTW, g.w_out - x0);
    if (ny <= 0 || nx <= 0) return;  // (not a tile of the table: the whole workgroup)
    const bool odd = (g.rot & 1) != 0;
    const int h = odd ? g.W : g.H, w = odd ? g.H : g.W;  // the turned image

    // the taps of the tile's rows and columns (an index beyond the image repeats the last one)
    if (tid < kTH) {
        const Tap t = tap_of(min(y0 + tid, g.h_out - 1), g.scale_y, h);
        TYs[tid] = t.s; TYf[tid] = t.f;
    } else if (tid < kTH + kTW) {
        const int j = tid - kTH;
        const Tap t = tap_of(min(x0 + j, g.w_out - 1), g.scale_x, w);
        TXs[j] = t.s; TXf[j] = t.f;
    }
    __syncthreads();

    // lines (stored rows, extent H) and span (stored columns, extent W) of the tile
    const int* Ls = odd ? TXs : TYs;
    const int* Ps = odd ? TYs : TXs;
    const int nl = odd ? nx : ny, np = odd ? ny : nx;
    const bool flipL = g.rot >= 2, flipP = g.rot == 1 || g.rot == 2;
    const int l_first = Ls[0], l_last = min(Ls[nl - 1] + 1, g.H - 1);
    const int p_first = Ps[0], p_last = min(Ps[np - 1] + 1, g.W - 1);
    const int span = p_last - p_first + 1;
    const int C0 = flipP ? g.W - 1 - p_last : p_first;  // the span's first stored column
    const int range = l_last - l_first + 1;
    const bool dense = range <= 2 * nl;
    const int nslots = dense ? range : 2 * nl;
    const int ng = (span + 30) >> 4;  // granules of a line: its span, the head (< 16) and the round-up (< 16)
    const int pitch = 4 * ng + 1;     // dwords, odd
    if (nslots * pitch > kLdsDwords) return;  // (refused on the host; the whole workgroup)
    if (tid < nslots) {
        const int l = dense ? l_first + tid : min(Ls[tid >> 1] + (tid & 1), g.H - 1);
        const int R = flipL ? g.H - 1 - l : l;
        SlotRow[tid] = R;
        SlotOff[tid] = tid * pitch * 4 + int((reinterpret_cast<uintptr_t>(g.src) + size_t(R) * g.W + C0) & 15);
    }
    __syncthreads();

    // ---- (a) stage: granule gi of slot's line
    for (int t = tid; t < nslots * ng; t += kThreads) {
        const int slot = t / ng, gi = t - slot * ng;
        const uint8_t* p = g.src + size_t(SlotRow[slot]) * g.W + C0;
        const int head = int(reinterpret_cast<uintptr_t>(p) & 15);
        if (16 * gi >= head + span) continue;  // no byte of the span in it
        const u4 raw = *reinterpret_cast<const u4*>(p - head + 16 * gi);
        uint32_t* d = &S[slot * pitch + 4 * gi];
        d[0] = raw.x; d[1] = raw.y; d[2] = raw.z; d[3] = raw.w;
    }
    __syncthreads();

    // ---- (b) taps
    const uint8_t* Sb = reinterpret_cast<const uint8_t*>(S);
    const int cx = tid & (kTW - 1), q = tid / kTW;
    if (cx >= nx) return;
    const int sx = TXs[cx], sx1 = min(sx + 1, w - 1);
    const float a1 = TXf[cx], a0 = 1.0f - a1;
    // the staged byte of the turned pixel (r, c), tap ky of the tile's row yy / tap kx of its column cx
    auto px = [&](int r, int c, int yy, int ky, int kx) -> unsigned {
        const int l = odd ? c : r, p = odd ? r : c;
        const int slot = dense ? l - l_first : (odd ? 2 * cx + kx : 2 * yy + ky);
        return Sb[SlotOff[slot] + (flipP ? p_last - p : p - p_first)];
    };
#pragma unroll
    for (int k = 0; k < kPixPerThread; ++k) {
        const int yy = q + kRowStep * k;
        if (yy >= ny) break;
        const int sy = TYs[yy], sy1 = min(sy + 1, h - 1);
        float v;
        if (g.ident) {
            v = u8_over_255(px(sy, sx, yy, 0, 0));
        } else {
            const float b1 = TYf[yy], b0 = 1.0f - b1;
            const float p00 = float(px(sy, sx, yy, 0, 0)), p01 = float(px(sy, sx1, yy, 0, 1));
            const float p10 = float(px(sy1, sx, yy, 1, 0)), p11 = float(px(sy1, sx1, yy, 1, 1));
            const float h0 = p00 * a0 + p01 * a1, h1 = p10 * a0 + p11 * a1;
            v = __fdiv_rn(h0 * b0 + h1 * b1, 255.0f);
        }
        g.dst[size_t(y0 + yy) * g.w_out + (x0 + cx)] = v;
    }
}

// ---- host ----
void out_size(int H, int W, int rot, int img_size, int* h_out, int* w_out) {
    const int h = (rot & 1) ? W : H, w = (rot & 1) ? H : W;
    if (img_size == std::max(h, w)) { *h_out = h; *w_out = w; return; }
    // eval_pairs.py:97-102 as written: the ratio, then its product with img_size, in double; truncation
    if (h >= w) {
        const double ar = double(w) / double(h);
        *h_out = img_size; *w_out = int(ar * double(img_size));
    } else {
        const double ar = double(h) / double(w);
        *h_out = int(ar * double(img_size)); *w_out = img_size;
    }
}

// What the tiles of one axis need at most: lines (were it the line axis) and span bytes (were it the span axis).
void axis_need(int n_in, int n_out, double scale, int tile, int* max_slots, int* max_span) {
    *max_slots = *max_span = 0;
    for (int d0 = 0; d0 < n_out; d0 += tile) {
        const int dl = std::min(d0 + tile, n_out) - 1;
        const int first = tap_of(d0, scale, n_in).s, last = std::min(tap_of(dl, scale, n_in).s + 1, n_in - 1);
        const int range = last - first + 1;
        *max_span = std::max(*max_span, range);
        *max_slots = std::max(*max_slots, std::min(range, 2 * (dl - d0 + 1)));
    }
}

struct GrayFrontState {
    GrayImage* d_tab = nullptr;  // [kMaxImages]
    // pinned staging of the table: a ring, so that a call does not wait for the copy of the call before it
    GrayImage* h_tab = nullptr;  // [kRing][kMaxImages]
    hipEvent_t copied[kRing] = {nullptr};
    bool pending[kRing] = {false};
    int next = 0;
};

int gray_state(e2emv_ctx* ctx, GrayFrontState** out) {
    if (!ctx->image_front_gray) {
        GrayFrontState* st = new GrayFrontState();
        ctx->image_front_gray = st;  // (freed with the context whatever fails below)
        if (hipMalloc((void**)&st->d_tab, size_t(kMaxImages) * sizeof(GrayImage)) != hipSuccess ||
            hipHostMalloc((void**)&st->h_tab, size_t(kRing) * kMaxImages * sizeof(GrayImage), hipHostMallocDefault) != hipSuccess) {
            (void)hipGetLastError();
            image_front_gray_free(ctx);
            return set_err(ctx, E2EMV_ENOMEM, "e2emv_image_front_gray: the image table and its pinned ring");
        }
        for (int k = 0; k < kRing; ++k)
            if (hipEventCreateWithFlags(&st->copied[k], hipEventDisableTiming) != hipSuccess) {
                (void)hipGetLastError();
                image_front_gray_free(ctx);
                return set_err(ctx, E2EMV_EHIP, "e2emv_image_front_gray: hipEventCreateWithFlags failed");
            }
    }
    *out = static_cast<GrayFrontState*>(ctx->image_front_gray);
    return E2EMV_OK;
}

}  // namespace

void image_front_gray_free(e2emv_ctx* ctx) {
    GrayFrontState* st = static_cast<GrayFrontState*>(ctx->image_front_gray);
    if (!st) return;
    if (st->d_tab) (void)hipFree(st->d_tab);
    if (st->h_tab) (void)hipHostFree(st->h_tab);
    for (int k = 0; k < kRing; ++k)
        if (st->copied[k]) (void)hipEventDestroy(st->copied[k]);
    delete st;
    ctx->image_front_gray = nullptr;
}

}  // namespace e2emv

using namespace e2emv;

extern "C" {

int e2emv_image_front_gray_size(int height, int width, int rot, int img_size, int* h_out, int* w_out) {
    if (!h_out || !w_out || height <= 0 || width <= 0 || img_size <= 0 || rot < 0 || rot > 3) return E2EMV_EINVAL;
    if (height > kMaxSide || width > kMaxSide || img_size > kMaxSide) return E2EMV_ESHAPE;
    out_size(height, width, rot, img_size, h_out, w_out);
    return (*h_out > 0 && *w_out > 0) ? E2EMV_OK : E2EMV_EINVAL;
}

int e2emv_image_front_gray(e2emv_ctx* ctx, int n, const e2emv_gray_image* images, int img_size, float* d_out, void* stream) {
    if (!ctx) return E2EMV_EINVAL;
    if (!images || !d_out) return set_err(ctx, E2EMV_EINVAL, "e2emv_image_front_gray: NULL argument");
    if (n <= 0 || n > kMaxImages) return set_err(ctx, E2EMV_EINVAL, "e2emv_image_front_gray: %d images, a call takes 1..%d", n, kMaxImages);
    if (img_size <= 0) return set_err(ctx, E2EMV_EINVAL, "e2emv_image_front_gray: img_size = %d", img_size);
    if (img_size > kMaxSide) return set_err(ctx, E2EMV_ESHAPE, "e2emv_image_front_gray: img_size = %d, more than %d", img_size, kMaxSide);
    GrayImage rows[kMaxImages];
    int64_t tiles = 0, floats = 0;
    for (int i = 0; i < n; ++i) {
        const e2emv_gray_image& im = images[i];
        if (!im.data) return set_err(ctx, E2EMV_EINVAL, "e2emv_image_front_gray: image %d has no data", i);
        if (im.height <= 0 || im.width <= 0)
            return set_err(ctx, E2EMV_EINVAL, "e2emv_image_front_gray: image %d is %d x %d: sizes must be positive", i, im.height, im.width);
        if (im.rot < 0 || im.rot > 3) return set_err(ctx, E2EMV_EINVAL, "e2emv_image_front_gray: image %d: rot = %d, not in 0..3", i, im.rot);
        if (im.height > kMaxSide || im.width > kMaxSide)
            return set_err(ctx, E2EMV_ESHAPE, "e2emv_image_front_gray: image %d is %d x %d, a side may have %d pixels", i, im.height, im.width, kMaxSide);
        GrayImage& g = rows[i];
        g.src = im.data;
        g.H = im.height; g.W = im.width; g.rot = im.rot;
        out_size(g.H, g.W, g.rot, img_size, &g.h_out, &g.w_out);
        if (g.h_out <= 0 || g.w_out <= 0)
            return set_err(ctx, E2EMV_EINVAL, "e2emv_image_front_gray: image %d (%d x %d, rot %d) at img_size %d has an output side of 0", i, im.height,
                           im.width, im.rot, img_size);
        const bool odd = (g.rot & 1) != 0;
        const int h = odd ? g.W : g.H, w = odd ? g.H : g.W;
        g.ident = (g.h_out == h && g.w_out == w) ? 1 : 0;
        g.scale_y = 1.0 / (double(g.h_out) / double(h));
        g.scale_x = 1.0 / (double(g.w_out) / double(w));
        // what a tile stages has to fit: lines from the axis that runs along the stored rows, the span from the other one
        int slots_y, span_y, slots_x, span_x;
        axis_need(h, g.h_out, g.scale_y, kTH, &slots_y, &span_y);
        axis_need(w, g.w_out, g.scale_x, kTW, &slots_x, &span_x);
        const int slots = odd ? slots_x : slots_y, span = (odd ? span_y : span_x) + 1;  // (+ 1: never tighter than the kernel's own count)
        if (int64_t(slots) * (4 * ((span + 30) >> 4) + 1) > kLdsDwords)
            return set_err(ctx, E2EMV_ESHAPE,
                           "e2emv_image_front_gray: image %d (%d x %d, rot %d -> %d x %d): a tile needs %d source lines of %d bytes, more than "
                           "the %d bytes a workgroup stages (a reduction beyond about 10)", i, im.height, im.width, im.rot, g.h_out, g.w_out, slots,
                           span, kLdsDwords * 4);
        g.tiles_x = (g.w_out + kTW - 1) / kTW;
        g.first_tile = int(tiles);
        g.dst = d_out + floats;
        tiles += int64_t(g.tiles_x) * ((g.h_out + kTH - 1) / kTH);
        floats += int64_t(g.h_out) * g.w_out;
    }
    // (kMaxImages images of kMaxSide^2 pixels: 2^26 tiles)
    E2EMV_ENTER(ctx, stream);
    hipStream_t s = (hipStream_t)stream;
    GrayFrontState* st = nullptr;
    int rc = gray_state(ctx, &st);
    if (rc) return rc;
    const int k = st->next;
    st->next = (k + 1) % kRing;
    if (st->pending[k]) {
        E2EMV_HIP(ctx, hipEventSynchronize(st->copied[k]));  // (the copy of kRing calls ago)
        st->pending[k] = false;
    }
    GrayImage* h = st->h_tab + size_t(k) * kMaxImages;
    std::memcpy(h, rows, size_t(n) * sizeof(GrayImage));
    E2EMV_HIP(ctx, hipMemcpyAsync(st->d_tab, h, size_t(n) * sizeof(GrayImage), hipMemcpyHostToDevice, s));
    E2EMV_HIP(ctx, hipEventRecord(st->copied[k], s));
    st->pending[k] = true;
    prof_begin(ctx, PS_MISC, s);
    hipLaunchKernelGGL(image_front_gray_kernel, dim3((unsigned)tiles), dim3(kThreads), 0, s, st->d_tab, n);
    E2EMV_CHECK_LAUNCH(ctx, "image_front_gray_kernel");
    return E2EMV_OK;
}

}  // extern "C"
