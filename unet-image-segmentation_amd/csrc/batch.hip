// The training input's last per-step host work, on the device: a batch is gathered out of a
// device-resident uint8 sample cache (unet_amd/device_data.py) and converted to the fp32 the engine
// reads.  dst[i] = src[slot] (mirrored along w where the slot entry is negative) as float / 255,
// BITWISE NumPy's a.astype(float32) / 255.0: the IEEE divide, no reciprocal (this object is built
// with -ffp-contract=off like imageproc.hip).
//
// The kernel writes 4 bytes per byte it reads, so the stores set its time:
//   quad path  (w % 4 == 0, src 4-byte and dst 16-byte aligned): one thread per 4 output floats, one
//              16-byte store, consecutive lanes at consecutive addresses (1 KiB per wave store).  Its
//              4 source bytes are one dword load; a row is w*c/4 whole dwords, so every row and
//              every sample starts on a dword.  Mirrored, c = 1: the mirrored dword, bytes reversed.
//              Mirrored, c = 3: 4 pixels are 3 dwords; the thread loads the mirrored group's three
//              and picks its 4 bytes (pixel order reversed, channel order kept).
//   byte path  (any other w or alignment): one thread per output float, byte loads, dword stores.
// A slot table entry is clamped into [0, n-1] (like the unet_lerp_coord tables): no table can make
// the kernel read outside src.  No LDS, no scratch.
//
// unet_batch_affine_u8 is the same batch with Keras' random affine augmentation in it: every batch
// position carries six fp32 numbers [m00 m01 o0 m10 m11 o1] (unet_amd/augment.py builds them, the
// horizontal flip folded in), output pixel (r, q) samples its source at (m00 r + m01 q + o0,
// m10 r + m11 q + o1), nearest or bilinear, the border replicated or a constant outside.  Every
// operation is one fp32 rounding in a fixed order (the contract is in include/unet_hip.h and restated
// in NumPy as augment.affine_u8_reference), so the result is BITWISE the host's.  The source
// sample fits in L2 and its taps are byte gathers, never staged; at order 1 those gathers (four per
// output value), not the stores, set the time (profiles/device_augment.txt):
//   quad path  (w % 4 == 0, dst 16-byte aligned): one thread per 4 consecutive pixels of a row, whole
//              16-byte stores, one for c = 1, three for c = 3.
//   byte path  (any other w or alignment): one thread per output float.
#include "common.h"
#include "dispatch.h"

namespace unet {
namespace {

constexpr int BG_BLOCK = 256;
constexpr unsigned BG_MAX_GRID_Y = 65535;

__device__ __forceinline__ int clamp_slot(int s, int n) { return s < 0 ? 0 : (s > n - 1 ? n - 1 : s); }

__device__ __forceinline__ float4 unpack255(unsigned v) {
    return make_float4((float)(v & 0xffu) / 255.0f, (float)((v >> 8) & 0xffu) / 255.0f,
                       (float)((v >> 16) & 0xffu) / 255.0f, (float)(v >> 24) / 255.0f);
}

// Q: dwords (= output quads) per sample, rowq: per row.  grid.x covers a sample, grid.y the batch.
template <int C>
__global__ __launch_bounds__(BG_BLOCK) void batch_gather_quad_kernel(const unsigned char* __restrict__ src, int n,
                                                                     int rowq, int Q, const int* __restrict__ slots,
                                                                     int b, float* __restrict__ dst) {
    const unsigned q = blockIdx.x * BG_BLOCK + threadIdx.x;
    if (q >= (unsigned)Q) return;
    for (int i = blockIdx.y; i < b; i += gridDim.y) {
        const int e = slots[i];
        const bool flip = e < 0;
        const unsigned* sp = reinterpret_cast<const unsigned*>(src + (int64_t)clamp_slot(flip ? ~e : e, n) * Q * 4);
        unsigned v;
        if (!flip) {
            v = sp[q];
        } else {
            const unsigned row = q / (unsigned)rowq, j = q - row * rowq;
            const unsigned* r = sp + row * rowq;
            if (C == 1) {
                v = __builtin_bswap32(r[rowq - 1 - j]);
            } else {
                // output group g (4 pixels, 12 bytes) is source group rowq/3 - 1 - g with its pixels in
                // reverse order: source bytes s0..s11 -> s9 s10 s11 | s6 s7 s8 | s3 s4 s5 | s0 s1 s2
                const unsigned g = j / 3u, t = j - 3u * g;
                const unsigned* p = r + (rowq - 3 - 3 * g);
                const unsigned d0 = p[0], d1 = p[1], d2 = p[2];
                if (t == 0)
                    v = (d2 >> 8) | ((d1 >> 16) << 24);                                        // s9 s10 s11 s6
                else if (t == 1)
                    v = (d1 >> 24) | ((d2 & 0xffu) << 8) | ((d0 >> 24) << 16) | (d1 << 24);    // s7 s8 s3 s4
                else
                    v = ((d1 >> 8) & 0xffu) | (d0 << 8);                                       // s5 s0 s1 s2
            }
        }
        reinterpret_cast<float4*>(dst)[(int64_t)i * Q + q] = unpack255(v);
    }
}

// E: bytes (= output floats) per sample, roww = w * C.
template <int C>
__global__ __launch_bounds__(BG_BLOCK) void batch_gather_byte_kernel(const unsigned char* __restrict__ src, int n,
                                                                     int w, int E, const int* __restrict__ slots,
                                                                     int b, float* __restrict__ dst) {
    const unsigned p = blockIdx.x * BG_BLOCK + threadIdx.x;
    if (p >= (unsigned)E) return;
    const unsigned roww = (unsigned)w * C;
    const unsigned r = p % roww, x = r / C, k = r - x * C;
    const unsigned mirrored = p - r + ((unsigned)w - 1 - x) * C + k;
    for (int i = blockIdx.y; i < b; i += gridDim.y) {
        const int e = slots[i];
        const bool flip = e < 0;
        const unsigned char* sp = src + (int64_t)clamp_slot(flip ? ~e : e, n) * E;
        dst[(int64_t)i * E + p] = (float)sp[flip ? mirrored : p] / 255.0f;
    }
}

// ---------------------------------------------------------------------------- affine warp ---
struct AffineRec {
    float m00, m01, o0, m10, m11, o1;
};

__device__ __forceinline__ AffineRec load_rec(const float* __restrict__ xforms, int i) {
    const float* t = xforms + (int64_t)i * 6;
    return AffineRec{t[0], t[1], t[2], t[3], t[4], t[5]};
}

// One output pixel (r, q) of the sample sp (h x w pixels, C bytes apart): NV values of it, from the
// byte sp points at, before the division.  fmaxf / fminf return the other operand for a NaN and the
// integer indices are clamped from both sides, so no record makes the kernel read outside the sample.
template <int C, int NV, int ORDER, bool FILL>
__device__ __forceinline__ void affine_pixel(const unsigned char* __restrict__ sp, int h, int w, const AffineRec& m,
                                             unsigned r, unsigned q, float cval, float* v) {
    const float fr = (float)r, fq = (float)q;
    const float hm = (float)(h - 1), wm = (float)(w - 1);
    float sy = (m.m00 * fr + m.m01 * fq) + m.o0;
    float sx = (m.m10 * fr + m.m11 * fq) + m.o1;
    const bool outside = sy < 0.0f || sy > hm || sx < 0.0f || sx > wm;
    sy = fminf(fmaxf(sy, 0.0f), hm);
    sx = fminf(fmaxf(sx, 0.0f), wm);
    if (ORDER == 0) {
        const int y = max(min((int)floorf(sy + 0.5f), h - 1), 0);
        const int x = max(min((int)floorf(sx + 0.5f), w - 1), 0);
        const unsigned char* p = sp + ((int64_t)y * w + x) * C;
#pragma unroll
        for (int k = 0; k < NV; ++k) v[k] = (float)p[k];
    } else {
        const int y0 = max(min((int)floorf(sy), max(h - 2, 0)), 0), y1 = min(y0 + 1, h - 1);
        const int x0 = max(min((int)floorf(sx), max(w - 2, 0)), 0), x1 = min(x0 + 1, w - 1);
        const float fy = sy - (float)y0, fx = sx - (float)x0;
        const unsigned char* r0 = sp + (int64_t)y0 * w * C;
        const unsigned char* r1 = sp + (int64_t)y1 * w * C;
#pragma unroll
        for (int k = 0; k < NV; ++k) {
            const float p00 = (float)r0[x0 * C + k], p01 = (float)r0[x1 * C + k];
            const float p10 = (float)r1[x0 * C + k], p11 = (float)r1[x1 * C + k];
            const float top = p00 + fx * (p01 - p00);
            const float bot = p10 + fx * (p11 - p10);
            v[k] = top + fy * (bot - top);
        }
    }
    if (FILL && outside) {
#pragma unroll
        for (int k = 0; k < NV; ++k) v[k] = cval;
    }
}

// G = h * w / 4 groups of 4 consecutive pixels per sample (w % 4 == 0: a group never leaves its row).
template <int C, int ORDER, bool FILL>
__global__ __launch_bounds__(BG_BLOCK) void batch_affine_quad_kernel(const unsigned char* __restrict__ src, int n,
                                                                     int h, int w, int G,
                                                                     const int* __restrict__ slots,
                                                                     const float* __restrict__ xforms, int b,
                                                                     float cval, float* __restrict__ dst) {
    const unsigned g = blockIdx.x * BG_BLOCK + threadIdx.x;
    if (g >= (unsigned)G) return;
    const unsigned roww = (unsigned)w / 4u;
    const unsigned r = g / roww, q0 = (g - r * roww) * 4u;
    const int64_t E = (int64_t)G * 4 * C;
    for (int i = blockIdx.y; i < b; i += gridDim.y) {
        const unsigned char* sp = src + (int64_t)clamp_slot(slots[i], n) * E;
        const AffineRec m = load_rec(xforms, i);
        float v[4 * C];
#pragma unroll
        for (int j = 0; j < 4; ++j) affine_pixel<C, C, ORDER, FILL>(sp, h, w, m, r, q0 + j, cval, v + j * C);
        float4* o = reinterpret_cast<float4*>(dst + (int64_t)i * E) + (int64_t)g * C;
#pragma unroll
        for (int t = 0; t < C; ++t)
            o[t] = make_float4(v[4 * t] / 255.0f, v[4 * t + 1] / 255.0f, v[4 * t + 2] / 255.0f, v[4 * t + 3] / 255.0f);
    }
}

// E = h * w * C output floats per sample, one per thread.
template <int C, int ORDER, bool FILL>
__global__ __launch_bounds__(BG_BLOCK) void batch_affine_byte_kernel(const unsigned char* __restrict__ src, int n,
                                                                     int h, int w, int E,
                                                                     const int* __restrict__ slots,
                                                                     const float* __restrict__ xforms, int b,
                                                                     float cval, float* __restrict__ dst) {
    const unsigned p = blockIdx.x * BG_BLOCK + threadIdx.x;
    if (p >= (unsigned)E) return;
    const unsigned px = p / C, k = p - px * C;
    const unsigned r = px / (unsigned)w, q = px - r * (unsigned)w;
    for (int i = blockIdx.y; i < b; i += gridDim.y) {
        const unsigned char* sp = src + (int64_t)clamp_slot(slots[i], n) * E;
        const AffineRec m = load_rec(xforms, i);
        float v;
        affine_pixel<C, 1, ORDER, FILL>(sp + k, h, w, m, r, q, cval, &v);
        dst[(int64_t)i * E + p] = v / 255.0f;
    }
}

}  // namespace
}  // namespace unet

using namespace unet;

extern "C" int unet_batch_gather_u8(const unsigned char* src, int n, int h, int w, int c, const int* slots, int b,
                                    float* dst, unet_stream_t stream) {
    UNET_CHECK_ARG(src && slots && dst, "unet_batch_gather_u8: null pointer");
    UNET_CHECK_ARG(n > 0 && h > 0 && w > 0 && b > 0, "unet_batch_gather_u8: sizes must be positive");
    UNET_CHECK_ARG(c == 1 || c == 3, "unet_batch_gather_u8: c must be 1 or 3, got %d", c);
    UNET_CHECK_ARG((int64_t)h * w * c <= INT32_MAX, "unet_batch_gather_u8: a sample of %d x %d x %d exceeds 2^31 bytes",
                   h, w, c);
    UNET_CHECK_ARG(((uintptr_t)dst | (uintptr_t)slots) % 4 == 0,
                   "unet_batch_gather_u8: dst and slots must be 4-byte aligned");
    const int E = h * w * c;
    const unsigned gy = (unsigned)b < BG_MAX_GRID_Y ? (unsigned)b : BG_MAX_GRID_Y;
    hipStream_t st = as_stream(stream);
    if (w % 4 == 0 && (uintptr_t)src % 4 == 0 && (uintptr_t)dst % 16 == 0) {
        const int Q = E / 4, rowq = w / 4 * c;
        const dim3 grid((unsigned)cdiv(Q, BG_BLOCK), gy);
        if (c == 3)
            batch_gather_quad_kernel<3><<<grid, BG_BLOCK, 0, st>>>(src, n, rowq, Q, slots, b, dst);
        else
            batch_gather_quad_kernel<1><<<grid, BG_BLOCK, 0, st>>>(src, n, rowq, Q, slots, b, dst);
    } else {
        const dim3 grid((unsigned)cdiv(E, BG_BLOCK), gy);
        if (c == 3)
            batch_gather_byte_kernel<3><<<grid, BG_BLOCK, 0, st>>>(src, n, w, E, slots, b, dst);
        else
            batch_gather_byte_kernel<1><<<grid, BG_BLOCK, 0, st>>>(src, n, w, E, slots, b, dst);
    }
    UNET_CHECK_LAUNCH("unet_batch_gather_u8");
    return 0;
}

extern "C" int unet_batch_affine_u8(const unsigned char* src, int n, int h, int w, int c, const int* slots,
                                    const float* xforms, int b, int order, int fill_constant, float cval, float* dst,
                                    unet_stream_t stream) {
    UNET_CHECK_ARG(src && slots && xforms && dst, "unet_batch_affine_u8: null pointer");
    UNET_CHECK_ARG(n > 0 && h > 0 && w > 0 && b > 0, "unet_batch_affine_u8: sizes must be positive");
    UNET_CHECK_ARG(c == 1 || c == 3, "unet_batch_affine_u8: c must be 1 or 3, got %d", c);
    UNET_CHECK_ARG(order == 0 || order == 1, "unet_batch_affine_u8: order must be 0 or 1, got %d", order);
    UNET_CHECK_ARG((int64_t)h * w * c <= INT32_MAX, "unet_batch_affine_u8: a sample of %d x %d x %d exceeds 2^31 bytes",
                   h, w, c);
    UNET_CHECK_ARG(((uintptr_t)dst | (uintptr_t)slots | (uintptr_t)xforms) % 4 == 0,
                   "unet_batch_affine_u8: dst, slots and xforms must be 4-byte aligned");
    const int E = h * w * c;
    const unsigned gy = (unsigned)b < BG_MAX_GRID_Y ? (unsigned)b : BG_MAX_GRID_Y;
    hipStream_t st = as_stream(stream);
    const bool quad = w % 4 == 0 && (uintptr_t)dst % 16 == 0;
    with_int<3, 1>(c, [&](auto C) {
        with_int<0, 1>(order, [&](auto O) {
            with_bool(fill_constant != 0, [&](auto F) {
                if (quad) {
                    const int G = h * (w / 4);
                    batch_affine_quad_kernel<C(), O(), F()><<<dim3((unsigned)cdiv(G, BG_BLOCK), gy), BG_BLOCK, 0, st>>>(
                        src, n, h, w, G, slots, xforms, b, cval, dst);
                } else {
                    batch_affine_byte_kernel<C(), O(), F()><<<dim3((unsigned)cdiv(E, BG_BLOCK), gy), BG_BLOCK, 0, st>>>(
                        src, n, h, w, E, slots, xforms, b, cval, dst);
                }
            });
        });
    });
    UNET_CHECK_LAUNCH("unet_batch_affine_u8");
    return 0;
}
