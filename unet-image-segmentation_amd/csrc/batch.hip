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
#include "common.h"

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
