// The CLIs' image steps around the forward, on the device (the reference does them with cv2 on the
// host): scripts/inference.py:105-108 and scripts/benchmark.py:105 (decoded uint8 image -> / 255 ->
// INTER_LINEAR to the model size) and scripts/inference.py:147-160 (probability map -> INTER_LINEAR
// back to the image's size -> > threshold -> 255).
//
// Both are held BITWISE to unet_amd/imageproc.py: resize_linear.  The sampling tables come from the
// host (linear_coords); the lerp is plain fp32 in NumPy's order, and this object is compiled with
// -ffp-contract=off so that no multiply-add is fused (NumPy rounds after every operation).
//
//   image_resize_u8  one thread per output pixel, all its channels: gathers 4 x c source bytes
//                    (byte loads: rows of a packed uint8 image are at any alignment), writes c floats.
//   mask_resize      the store-bound one (oh * ow bytes from a source that stays in cache).  A row is
//                    cut at the 16-byte boundaries of its ADDRESS: one thread per piece, so every
//                    full piece is one aligned 16-byte store and consecutive lanes store consecutive
//                    16 bytes; the row's head and tail pieces go out as naturally aligned 8/4/2/1-byte
//                    stores.  Across its run a thread keeps the last two source columns' values
//                    (an enlargement re-reads each source column ~ow/w times).
#include "common.h"

namespace unet {
namespace {

constexpr int IP_BLOCK = 256;
constexpr int RUN = 16;  // output bytes per thread of mask_resize: one 16-byte store

__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// a + (b - a) * f with a rounding after each operation (the object is built with -ffp-contract=off)
__device__ __forceinline__ float lerp1(float a, float b, float f) { return a + (b - a) * f; }

__device__ __forceinline__ unet_lerp_coord ld_coord(const unet_lerp_coord* t, int i) {
    const int4 v = *reinterpret_cast<const int4*>(t + i);
    unet_lerp_coord c;
    c.i0 = v.x;
    c.i1 = v.y;
    c.frac = __int_as_float(v.z);
    c.reserved = 0;
    return c;
}

template <int C>
__global__ __launch_bounds__(IP_BLOCK) void image_resize_u8_kernel(const unsigned char* __restrict__ src, int sh,
                                                                   int sw, const unet_lerp_coord* __restrict__ ytab,
                                                                   const unet_lerp_coord* __restrict__ xtab, int oh,
                                                                   int ow, int reverse, float* __restrict__ dst) {
    const int64_t p = (int64_t)blockIdx.x * IP_BLOCK + threadIdx.x;
    if (p >= (int64_t)oh * ow) return;
    const int oy = (int)(p / ow), ox = (int)(p - (int64_t)oy * ow);
    const unet_lerp_coord cy = ld_coord(ytab, oy), cx = ld_coord(xtab, ox);
    const int64_t r0 = (int64_t)clampi(cy.i0, sh - 1) * sw, r1 = (int64_t)clampi(cy.i1, sh - 1) * sw;
    const int x0 = clampi(cx.i0, sw - 1), x1 = clampi(cx.i1, sw - 1);
    const unsigned char* pa = src + (r0 + x0) * C;
    const unsigned char* pb = src + (r0 + x1) * C;
    const unsigned char* pc = src + (r1 + x0) * C;
    const unsigned char* pd = src + (r1 + x1) * C;
    float* o = dst + p * C;
#pragma unroll
    for (int k = 0; k < C; ++k) {
        const int s = reverse ? C - 1 - k : k;
        const float a = (float)pa[s] / 255.0f, b = (float)pb[s] / 255.0f;
        const float c = (float)pc[s] / 255.0f, d = (float)pd[s] / 255.0f;
        o[k] = lerp1(lerp1(a, b, cx.frac), lerp1(c, d, cx.frac), cy.frac);
    }
}

// Two source columns (their values in the run's two source rows) a thread holds from one output x
// to the next: when the next x needs a column it already has, no load is issued.
struct ColPair {
    int i0, i1;  // source x of the held columns (-1: none)
    float t0, b0, t1, b1;
};
__device__ __forceinline__ void col_advance(ColPair& h, const float* __restrict__ top, const float* __restrict__ bot,
                                            int x0, int x1) {
    float t0, b0, t1, b1;
    if (x0 == h.i0) {
        t0 = h.t0, b0 = h.b0;
    } else if (x0 == h.i1) {
        t0 = h.t1, b0 = h.b1;
    } else {
        t0 = top[x0], b0 = bot[x0];
    }
    if (x1 == x0) {
        t1 = t0, b1 = b0;
    } else if (x1 == h.i1) {
        t1 = h.t1, b1 = h.b1;
    } else {
        t1 = top[x1], b1 = bot[x1];
    }
    h.i0 = x0, h.i1 = x1;
    h.t0 = t0, h.b0 = b0, h.t1 = t1, h.b1 = b1;
}

// The low `len` (1..16) bytes of (lo, hi) to p .. p + len - 1 and nowhere else: one 16-byte store
// where the piece is whole and aligned, else the widest naturally aligned store that still fits.
__device__ __forceinline__ void store_piece(unsigned char* p, uint64_t lo, uint64_t hi, int len) {
    if (len == RUN && ((uintptr_t)p & 15) == 0) {
        *reinterpret_cast<uint4*>(p) =
            make_uint4((unsigned)lo, (unsigned)(lo >> 32), (unsigned)hi, (unsigned)(hi >> 32));
        return;
    }
    while (len > 0) {
        const uintptr_t a = (uintptr_t)p;
        int n;
        if (len >= 8 && (a & 7) == 0) {
            *reinterpret_cast<uint64_t*>(p) = lo;
            lo = hi, hi = 0;
            p += 8, len -= 8;
            continue;
        } else if (len >= 4 && (a & 3) == 0) {
            *reinterpret_cast<unsigned*>(p) = (unsigned)lo;
            n = 4;
        } else if (len >= 2 && (a & 1) == 0) {
            *reinterpret_cast<unsigned short*>(p) = (unsigned short)lo;
            n = 2;
        } else {
            *p = (unsigned char)lo;
            n = 1;
        }
        lo = (lo >> (8 * n)) | (hi << (64 - 8 * n));
        hi >>= 8 * n;
        p += n, len -= n;
    }
}

// pieces of a row of ow bytes at address `row`: piece 0 is the head up to the first 16-byte boundary
// (empty when the row starts on one), piece k >= 1 the k-th 16 bytes after it, cut at the row's end
__device__ __forceinline__ void piece_range(const unsigned char* row, int ow, int k, int& xs, int& xe) {
    int head = (int)((16 - ((uintptr_t)row & 15)) & 15);
    if (head > ow) head = ow;
    if (k == 0) {
        xs = 0, xe = head;
    } else {
        xs = head + (k - 1) * RUN;
        xe = xs + RUN < ow ? xs + RUN : ow;
    }
}

__global__ __launch_bounds__(IP_BLOCK) void mask_resize_bin_kernel(const float* __restrict__ prob, int h, int w,
                                                                   const unet_lerp_coord* __restrict__ ytab,
                                                                   const unet_lerp_coord* __restrict__ xtab, int oh,
                                                                   int ow, int pieces, float thr,
                                                                   unsigned char* __restrict__ mask) {
    const int64_t t = (int64_t)blockIdx.x * IP_BLOCK + threadIdx.x;
    if (t >= (int64_t)oh * pieces) return;
    const int oy = (int)(t / pieces), k = (int)(t - (int64_t)oy * pieces);
    unsigned char* row = mask + (int64_t)oy * ow;
    int xs, xe;
    piece_range(row, ow, k, xs, xe);
    if (xs >= xe) return;
    const unet_lerp_coord cy = ld_coord(ytab, oy);
    const float* top = prob + (int64_t)clampi(cy.i0, h - 1) * w;
    const float* bot = prob + (int64_t)clampi(cy.i1, h - 1) * w;
    ColPair hold;
    hold.i0 = hold.i1 = -1;
    hold.t0 = hold.b0 = hold.t1 = hold.b1 = 0.f;
    uint64_t lo = 0, hi = 0;
#pragma unroll
    for (int j = 0; j < RUN; ++j) {
        const int x = xs + j;
        if (x < xe) {
            const unet_lerp_coord cx = ld_coord(xtab, x);
            col_advance(hold, top, bot, clampi(cx.i0, w - 1), clampi(cx.i1, w - 1));
            const float v = lerp1(lerp1(hold.t0, hold.t1, cx.frac), lerp1(hold.b0, hold.b1, cx.frac), cy.frac);
            const uint64_t byte = v > thr ? 255u : 0u;
            if (j < 8)
                lo |= byte << (8 * j);
            else
                hi |= byte << (8 * (j - 8));
        }
    }
    store_piece(row + xs, lo, hi, xe - xs);
}

__global__ __launch_bounds__(IP_BLOCK) void mask_resize_argmax_kernel(const float* __restrict__ prob, int h, int w,
                                                                      int ncls,
                                                                      const unet_lerp_coord* __restrict__ ytab,
                                                                      const unet_lerp_coord* __restrict__ xtab, int oh,
                                                                      int ow, int pieces,
                                                                      unsigned char* __restrict__ mask) {
    const int64_t t = (int64_t)blockIdx.x * IP_BLOCK + threadIdx.x;
    if (t >= (int64_t)oh * pieces) return;
    const int oy = (int)(t / pieces), k = (int)(t - (int64_t)oy * pieces);
    unsigned char* row = mask + (int64_t)oy * ow;
    int xs, xe;
    piece_range(row, ow, k, xs, xe);
    if (xs >= xe) return;
    const unet_lerp_coord cy = ld_coord(ytab, oy);
    const float* top = prob + (int64_t)clampi(cy.i0, h - 1) * w * ncls;
    const float* bot = prob + (int64_t)clampi(cy.i1, h - 1) * w * ncls;
    uint64_t lo = 0, hi = 0;
#pragma unroll 1
    for (int j = 0; j < RUN; ++j) {
        const int x = xs + j;
        if (x >= xe) break;
        const unet_lerp_coord cx = ld_coord(xtab, x);
        const int64_t o0 = (int64_t)clampi(cx.i0, w - 1) * ncls, o1 = (int64_t)clampi(cx.i1, w - 1) * ncls;
        float best = 0.f;
        unsigned arg = 0;
        for (int c = 0; c < ncls; ++c) {
            const float v = lerp1(lerp1(top[o0 + c], top[o1 + c], cx.frac), lerp1(bot[o0 + c], bot[o1 + c], cx.frac),
                                  cy.frac);
            if (c == 0 || v > best) {  // strict: the first index wins a tie, as np.argmax
                best = v;
                arg = (unsigned)c;
            }
        }
        if (j < 8)
            lo |= (uint64_t)arg << (8 * j);
        else
            hi |= (uint64_t)arg << (8 * (j - 8));
    }
    store_piece(row + xs, lo, hi, xe - xs);
}

}  // namespace
}  // namespace unet

using namespace unet;

extern "C" int unet_image_resize_u8(const unsigned char* src, int sh, int sw, int c, const unet_lerp_coord* ytab,
                                    const unet_lerp_coord* xtab, int oh, int ow, int reverse_channels, float* dst,
                                    unet_stream_t stream) {
    UNET_CHECK_ARG(src && ytab && xtab && dst, "unet_image_resize_u8: null pointer");
    UNET_CHECK_ARG(sh > 0 && sw > 0 && oh > 0 && ow > 0, "unet_image_resize_u8: sizes must be positive");
    UNET_CHECK_ARG(c == 1 || c == 3, "unet_image_resize_u8: c must be 1 or 3, got %d", c);
    UNET_CHECK_ARG(((uintptr_t)ytab | (uintptr_t)xtab) % 16 == 0 && (uintptr_t)dst % 4 == 0,
                   "unet_image_resize_u8: tables must be 16-byte aligned, dst 4-byte aligned");
    const unsigned grid = (unsigned)cdiv((int64_t)oh * ow, IP_BLOCK);
    hipStream_t st = as_stream(stream);
    if (c == 3)
        image_resize_u8_kernel<3><<<grid, IP_BLOCK, 0, st>>>(src, sh, sw, ytab, xtab, oh, ow, reverse_channels, dst);
    else
        image_resize_u8_kernel<1><<<grid, IP_BLOCK, 0, st>>>(src, sh, sw, ytab, xtab, oh, ow, reverse_channels, dst);
    UNET_CHECK_LAUNCH("unet_image_resize_u8");
    return 0;
}

extern "C" int unet_mask_resize(const float* prob, int h, int w, int ncls, const unet_lerp_coord* ytab,
                                const unet_lerp_coord* xtab, int oh, int ow, float threshold, unsigned char* mask,
                                unet_stream_t stream) {
    UNET_CHECK_ARG(prob && ytab && xtab && mask, "unet_mask_resize: null pointer");
    UNET_CHECK_ARG(h > 0 && w > 0 && oh > 0 && ow > 0, "unet_mask_resize: sizes must be positive");
    UNET_CHECK_ARG(ncls >= 1 && ncls <= 255, "unet_mask_resize: ncls must be 1..255 (a uint8 class index), got %d",
                   ncls);
    UNET_CHECK_ARG(((uintptr_t)ytab | (uintptr_t)xtab) % 16 == 0 && (uintptr_t)prob % 4 == 0,
                   "unet_mask_resize: tables must be 16-byte aligned, prob 4-byte aligned");
    // a head piece, then ceil(ow / 16) pieces at most; a piece past the row's end does nothing
    const int pieces = 1 + (int)cdiv(ow, RUN);
    const unsigned grid = (unsigned)cdiv((int64_t)oh * pieces, IP_BLOCK);
    hipStream_t st = as_stream(stream);
    if (ncls == 1)
        mask_resize_bin_kernel<<<grid, IP_BLOCK, 0, st>>>(prob, h, w, ytab, xtab, oh, ow, pieces, threshold, mask);
    else
        mask_resize_argmax_kernel<<<grid, IP_BLOCK, 0, st>>>(prob, h, w, ncls, ytab, xtab, oh, ow, pieces, mask);
    UNET_CHECK_LAUNCH("unet_mask_resize");
    return 0;
}
