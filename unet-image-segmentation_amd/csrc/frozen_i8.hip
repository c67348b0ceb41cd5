// Frozen int8 inference (ABI 14): the kernels behind UNetModel.freeze(dtype="int8").
//
// The arithmetic contract is stated in include/unet_hip.h ("Frozen int8 inference") and restated in
// NumPy by tests/i8_emulation.py; these kernels implement exactly it.  Activations are NHWC bytes:
// uint8 (x = s q, q in [0, 255]) after a ReLU, int8 (q in [-127, 127]) after an upsample; spatial
// padding is q = 0.  The pointwise GEMMs run on v_mfma_i32_32x32x32_i8 with exact int32 accumulators.
//
// MFMA operands (32x32x32, 8-bit): lane l, r = l & 31, hh = l >> 5 holds 16 bytes of A row r and
// 16 bytes of B column r.  Both operands give lane half hh the channels 16 hh .. 16 hh + 15 of the
// K step in the same element slots, so the product is right whatever order the instruction walks
// k in.  The accumulator map is the fp16 kernels': register i of the lane is
// D[row (i & 3) + 8 (i >> 2) + 4 hh][col r].  GEMM rows are pixels, columns are output channels.
#include "common.h"
#include "dispatch.h"

namespace unet {
namespace {

typedef int intx4 __attribute__((ext_vector_type(4)));
typedef int intx16 __attribute__((ext_vector_type(16)));
typedef unsigned char u8;

constexpr int kBlock = 256;   // 4 waves, 32 GEMM rows each
constexpr int kRows = 128;    // GEMM rows per block
constexpr int kMinBlocks = 512;  // below this a launch takes narrower column blocks
constexpr int kKC = 64;       // channels of one LDS halo chunk (tile policy)
constexpr int kHaloW = 18, kHaloH = 10, kHaloPx = kHaloW * kHaloH;
constexpr int kHaloLd = kKC + 16;  // bytes per halo pixel: one byte per channel, 16-B slots 5 p + s

__device__ __forceinline__ uint4 ldg16(const u8* p) { return *reinterpret_cast<const uint4*>(p); }
__device__ __forceinline__ intx4 as_i4(uint4 v) { return __builtin_bit_cast(intx4, v); }

struct SrcView {
    const u8* src0;
    const u8* src1;
    int c0, c1;
    int sg0, sg1;  // the source holds int8 (else uint8)
};
// 16 channels c..c+15 of pixel `pix` of the logical tensor (c % 16 == 0, c0 % 16 == 0)
__device__ __forceinline__ uint4 view_ld(const SrcView& v, size_t pix, int c) {
    return c < v.c0 ? ldg16(v.src0 + pix * (size_t)v.c0 + c) : ldg16(v.src1 + pix * (size_t)v.c1 + (c - v.c0));
}

template <bool SG>
__device__ __forceinline__ float byte_f32(unsigned word, int j) {
    if constexpr (SG) return (float)(int)(signed char)(word >> (8 * j));
    return (float)((word >> (8 * j)) & 0xffu);
}
// depthwise accumulation of one tap for 4 channels (one dword of the pixel): a[j] = fmaf(x[j], w[j], a[j])
template <bool SG>
__device__ __forceinline__ void tap_fma4(float* a, unsigned word, float4 w) {
    a[0] = fmaf(byte_f32<SG>(word, 0), w.x, a[0]);
    a[1] = fmaf(byte_f32<SG>(word, 1), w.y, a[1]);
    a[2] = fmaf(byte_f32<SG>(word, 2), w.z, a[2]);
    a[3] = fmaf(byte_f32<SG>(word, 3), w.w, a[3]);
}

// clamp(rintf(v), lo, hi) as an integer
__device__ __forceinline__ int quant(float v, float lo, float hi) { return (int)fminf(fmaxf(rintf(v), lo), hi); }
__device__ __forceinline__ unsigned pack4(const float* a) {
    return (unsigned)(quant(a[0], -127.f, 127.f) & 0xff) | ((unsigned)(quant(a[1], -127.f, 127.f) & 0xff) << 8) |
           ((unsigned)(quant(a[2], -127.f, 127.f) & 0xff) << 16) | ((unsigned)quant(a[3], -127.f, 127.f) << 24);
}

// Where GEMM row `m` of the launch lives in the image (the fp16 kernels' row orders).
struct RowPos {
    bool valid;
    int img, y, x;
};
template <bool TILE>
__device__ __forceinline__ RowPos row_pos(int64_t m, int64_t M, int h, int w, bool window_order, int tile_img,
                                          int tile_y0, int tile_x0) {
    RowPos p;
    if constexpr (TILE) {
        // m = row inside the 8 x 16 tile's 128: wave = m >> 5 owns image rows 2 wave, 2 wave + 1;
        // bit 0 = column bit 0, bit 1 = row, bits 2.. = column bits 1..: a 2x2 pool window is
        // rows 4 q .. 4 q + 3, the four accumulator registers 4 g .. 4 g + 3 of one lane
        const int ml = (int)m & 31, wv = (int)m >> 5;
        p.valid = true;
        p.img = tile_img;
        p.y = tile_y0 + 2 * wv + ((ml >> 1) & 1);
        p.x = tile_x0 + (ml & 1) + 2 * (ml >> 2);
    } else {
        p.valid = m < M;
        const int64_t mm = p.valid ? m : 0;
        if (window_order) {  // (img, y / 2, x / 2) row-major windows, 4 rows each
            const int w2 = w >> 1, h2 = h >> 1;
            const int64_t q = mm >> 2;
            p.img = (int)(q / ((int64_t)h2 * w2));
            const int rem = (int)(q % ((int64_t)h2 * w2));
            p.y = 2 * (rem / w2) + (((int)mm >> 1) & 1);
            p.x = 2 * (rem % w2) + ((int)mm & 1);
        } else {
            p.img = (int)(mm / ((int64_t)h * w));
            const int rem = (int)(mm % ((int64_t)h * w));
            p.y = rem / w;
            p.x = rem % w;
        }
    }
    return p;
}

// Epilogue staging: a wave's 32 x (32 EG) result (and its 8 pooled rows) as bytes in LDS, so the
// global stores are 16 bytes of contiguous channels per lane.
template <int EG>
struct Stage {
    static constexpr int kLd = 32 * EG + 16;                  // bytes per row
    static constexpr int kWaveBytes = (32 + 8) * kLd;         // 32 rows + 8 pooled rows
    static constexpr int kBytes = 4 * kWaveBytes;
};

// ------------------------------------------------------------------ separable conv ----
template <int NT, bool TILE>
__global__ __launch_bounds__(kBlock) void i8_sep_kernel(SrcView v, int n, int h, int w, const float* __restrict__ taps_g,
                                                        int cout, const u8* __restrict__ pw,
                                                        const float* __restrict__ mult,
                                                        const float* __restrict__ bias_q, u8* __restrict__ out,
                                                        u8* __restrict__ out_pool) {
    constexpr int EG = NT < 4 ? NT : 4;
    using St = Stage<EG>;
    // tile policy: the chunk's halo (one byte per channel), then its depthwise taps [9][kKC] fp32
    constexpr int kHaloBytes = TILE ? kHaloPx * kHaloLd : 0;
    constexpr int kTapBytes = TILE ? 9 * kKC * 4 : 0;
    constexpr int kSmem = St::kBytes > kHaloBytes + kTapBytes ? St::kBytes : kHaloBytes + kTapBytes;
    __shared__ __attribute__((aligned(16))) u8 smem[kSmem];
    float* const taps = reinterpret_cast<float*>(smem + kHaloBytes);

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, hh = lane >> 5;
    const int C = v.c0 + v.c1;
    const int nb0 = blockIdx.y * (32 * NT);
    const int64_t M = (int64_t)n * h * w;
    const bool pooled = out_pool != nullptr;

    int tile_img = 0, tile_y0 = 0, tile_x0 = 0;
    if constexpr (TILE) {
        const int tx_n = w >> 4, ty_n = h >> 3;
        const int t = blockIdx.x;
        tile_img = t / (tx_n * ty_n);
        const int rem = t % (tx_n * ty_n);
        tile_y0 = (rem / tx_n) * 8;
        tile_x0 = (rem % tx_n) * 16;
    }
    const int64_t m_wave = TILE ? (int64_t)wave * 32 : (int64_t)blockIdx.x * kRows + wave * 32;
    const RowPos me = row_pos<TILE>(m_wave + r, M, h, w, pooled, tile_img, tile_y0, tile_x0);

    intx16 acc[NT];
#pragma unroll
    for (int i = 0; i < NT; ++i)
#pragma unroll
        for (int j = 0; j < 16; ++j) acc[i][j] = 0;

    for (int kc0 = 0; kc0 < C; kc0 += kKC) {
        const int kcn = (C - kc0) < kKC ? (C - kc0) : kKC;
        if constexpr (TILE) {
            __syncthreads();
            const int segs = kcn >> 4;
            for (int idx = tid; idx < kHaloPx * segs; idx += kBlock) {
                const int p = idx / segs, s = idx - p * segs;
                const int gy = tile_y0 + p / kHaloW - 1, gx = tile_x0 + p % kHaloW - 1;
                uint4 val = make_uint4(0, 0, 0, 0);
                if (gy >= 0 && gy < h && gx >= 0 && gx < w)
                    val = view_ld(v, ((size_t)tile_img * h + gy) * w + gx, kc0 + 16 * s);
                *reinterpret_cast<uint4*>(smem + p * kHaloLd + 16 * s) = val;
            }
            const int quads = kcn >> 2;
            for (int idx = tid; idx < 9 * quads; idx += kBlock) {
                const int t = idx / quads, q = idx - t * quads;
                st4(taps + t * kKC + 4 * q, ld4(taps_g + (size_t)t * C + kc0 + 4 * q));
            }
            __syncthreads();
        }
        for (int ks = 0; ks < kcn; ks += 32) {
            const int cl = ks + 16 * hh;  // channel inside the chunk
            const int c = kc0 + cl;       // channel of the logical tensor
            float a[16];
#pragma unroll
            for (int j = 0; j < 16; ++j) a[j] = 0.f;
            // the nine taps of the lane's 16 channels, for a uint8 or an int8 source
            auto depthwise = [&](auto SG) {
#pragma unroll
                for (int t = 0; t < 9; ++t) {
                    const int dy = t / 3 - 1, dx = t % 3 - 1;
                    uint4 xv;
                    const float* tp;
                    if constexpr (TILE) {
                        const int ly = me.y - tile_y0 + 1 + dy, lx = me.x - tile_x0 + 1 + dx;
                        xv = *reinterpret_cast<const uint4*>(smem + (ly * kHaloW + lx) * kHaloLd + cl);
                        tp = taps + t * kKC + cl;
                    } else {
                        tp = taps_g + (size_t)t * C + c;
                        const int yy = me.y + dy, xx = me.x + dx;
                        xv = make_uint4(0, 0, 0, 0);
                        if (me.valid && yy >= 0 && yy < h && xx >= 0 && xx < w)
                            xv = view_ld(v, ((size_t)me.img * h + yy) * w + xx, c);
                    }
                    tap_fma4<SG()>(a + 0, xv.x, ld4(tp + 0));
                    tap_fma4<SG()>(a + 4, xv.y, ld4(tp + 4));
                    tap_fma4<SG()>(a + 8, xv.z, ld4(tp + 8));
                    tap_fma4<SG()>(a + 12, xv.w, ld4(tp + 12));
                }
            };
            if (c < v.c0 ? v.sg0 : v.sg1)
                depthwise(std::true_type{});
            else
                depthwise(std::false_type{});
            intx4 af;
            af[0] = (int)pack4(a + 0);
            af[1] = (int)pack4(a + 4);
            af[2] = (int)pack4(a + 8);
            af[3] = (int)pack4(a + 12);
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const intx4 bf = as_i4(ldg16(pw + (size_t)(nb0 + nt * 32 + r) * C + c));
                acc[nt] = __builtin_amdgcn_mfma_i32_32x32x32_i8(af, bf, acc[nt], 0, 0, 0);
            }
        }
    }

    // epilogue: q = clamp(rint(acc mult + bias_q), 0, 255) (the clamp is the ReLU), staged through
    // LDS in groups of EG column tiles
    u8* const st = smem + wave * St::kWaveBytes;
    u8* const stp = st + 32 * St::kLd;
#pragma unroll
    for (int g0 = 0; g0 < NT; g0 += EG) {
        __syncthreads();
#pragma unroll
        for (int e = 0; e < EG; ++e) {
            const int col = e * 32 + r;
            const float mu = mult[nb0 + (g0 + e) * 32 + r];
            const float b = bias_q[nb0 + (g0 + e) * 32 + r];
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                int mx = 0;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int reg = 4 * g + i;
                    const int row = (reg & 3) + 8 * (reg >> 2) + 4 * hh;
                    const int o = quant(fmaf((float)acc[g0 + e][reg], mu, b), 0.f, 255.f);
                    st[row * St::kLd + col] = (u8)o;
                    mx = o > mx ? o : mx;
                }
                stp[(hh + 2 * g) * St::kLd + col] = (u8)mx;
            }
        }
        __syncthreads();
        constexpr int kChunks = EG * 2;  // 16-B chunks per row
        for (int idx = lane; idx < 32 * kChunks; idx += 64) {
            const int row = idx / kChunks, ch = idx - row * kChunks;
            const RowPos p = row_pos<TILE>(m_wave + row, M, h, w, pooled, tile_img, tile_y0, tile_x0);
            if (p.valid) {
                const size_t pix = ((size_t)p.img * h + p.y) * w + p.x;
                *reinterpret_cast<uint4*>(out + pix * cout + nb0 + g0 * 32 + ch * 16) =
                    *reinterpret_cast<const uint4*>(st + row * St::kLd + ch * 16);
            }
        }
        if (pooled) {
            for (int idx = lane; idx < 8 * kChunks; idx += 64) {
                const int q = idx / kChunks, ch = idx - q * kChunks;
                // the window's first row tells where it is
                const RowPos p = row_pos<TILE>(m_wave + 4 * q, M, h, w, true, tile_img, tile_y0, tile_x0);
                if (p.valid) {
                    const size_t pix = ((size_t)p.img * (h >> 1) + (p.y >> 1)) * (w >> 1) + (p.x >> 1);
                    *reinterpret_cast<uint4*>(out_pool + pix * cout + nb0 + g0 * 32 + ch * 16) =
                        *reinterpret_cast<const uint4*>(stp + q * St::kLd + ch * 16);
                }
            }
        }
    }
}

// --------------------------------------------------------------- transposed conv ----
// GEMM rows = input pixels, K = cin, columns = (a, b, co) of the Keras (2, 2, cout, cin) kernel,
// which is already [column][k] with k contiguous.  A = the uint8 input XOR 0x80 (q - 128 as int8);
// the epilogue adds 128 colsum back, so acc32 is the exact product with q.
template <int NT>
__global__ __launch_bounds__(kBlock) void i8_convt_kernel(const u8* __restrict__ x, int n, int h, int w, int cin,
                                                          int cout, const u8* __restrict__ kern,
                                                          const int* __restrict__ colsum,
                                                          const float* __restrict__ mult,
                                                          const float* __restrict__ bias_q, u8* __restrict__ out) {
    using St = Stage<NT>;
    __shared__ __attribute__((aligned(16))) u8 smem[St::kBytes];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, hh = lane >> 5;
    const int nb0 = blockIdx.y * (32 * NT);
    const int64_t M = (int64_t)n * h * w;
    const int64_t m_wave = (int64_t)blockIdx.x * kRows + wave * 32;
    const int64_t m = m_wave + r;
    const bool valid = m < M;

    intx16 acc[NT];
#pragma unroll
    for (int i = 0; i < NT; ++i)
#pragma unroll
        for (int j = 0; j < 16; ++j) acc[i][j] = 0;

    for (int k0 = 0; k0 < cin; k0 += 32) {
        const int c = k0 + 16 * hh;
        uint4 av = make_uint4(0, 0, 0, 0);
        if (valid) av = ldg16(x + (size_t)m * cin + c);
        av.x ^= 0x80808080u, av.y ^= 0x80808080u, av.z ^= 0x80808080u, av.w ^= 0x80808080u;
        const intx4 af = as_i4(av);
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const intx4 bf = as_i4(ldg16(kern + (size_t)(nb0 + nt * 32 + r) * cin + c));
            acc[nt] = __builtin_amdgcn_mfma_i32_32x32x32_i8(af, bf, acc[nt], 0, 0, 0);
        }
    }

    u8* const st = smem + wave * St::kWaveBytes;
#pragma unroll
    for (int e = 0; e < NT; ++e) {
        const int col = e * 32 + r;
        const int fix = 128 * colsum[nb0 + col];
        const float mu = mult[nb0 + col];
        const float b = bias_q[(nb0 + col) % cout];
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const int row = (reg & 3) + 8 * (reg >> 2) + 4 * hh;
            st[row * St::kLd + col] = (u8)quant(fmaf((float)(acc[e][reg] + fix), mu, b), -127.f, 127.f);
        }
    }
    __syncthreads();
    // a lane keeps its 16-byte column chunk and walks the rows: the (a, b, co) split of the column
    // is computed once, the row's (img, y, x) in 32-bit arithmetic (the entry point bounds M)
    constexpr int kChunks = NT * 2, kRowStep = 64 / kChunks;
    const int ch = lane % kChunks;
    const int col = nb0 + ch * 16;
    const int ab = col / cout, co = col - ab * cout;
    const unsigned hw = (unsigned)h * (unsigned)w;
    for (int row = lane / kChunks; row < 32; row += kRowStep) {
        const int64_t mr = m_wave + row;
        if (mr < M) {
            const unsigned mu = (unsigned)mr;
            const unsigned img = mu / hw, rem = mu - img * hw;
            const unsigned y = rem / (unsigned)w, xx = rem - y * (unsigned)w;
            const size_t pix = ((size_t)img * (2 * h) + 2 * y + (ab >> 1)) * (2 * w) + 2 * xx + (ab & 1);
            *reinterpret_cast<uint4*>(out + pix * cout + co) =
                *reinterpret_cast<const uint4*>(st + row * St::kLd + ch * 16);
        }
    }
}

// ------------------------------------------------------------------- image block ----
// f16_image_kernel's work split and fp32 arithmetic (one thread: 8 output channels of up to
// kImagePx pixels of one image row); the output is q = clamp(rint(relu(z) / s_out), 0, 255).
constexpr int kImagePx = 8;
__global__ __launch_bounds__(kBlock) void i8_image_kernel(const float* __restrict__ x, int n, int h, int w, int cin,
                                                          const float* __restrict__ dw, int cout,
                                                          const float* __restrict__ pw, const float* __restrict__ bias,
                                                          float s_out, u8* __restrict__ out) {
    const int groups = cout >> 3;
    const int items = w * groups;  // (pixel, channel group) pairs of the row
    const int img = blockIdx.x / h, y = blockIdx.x - img * h;
    const size_t row0 = ((size_t)img * h + y) * w;  // first pixel of the row
    const bool fixed = kBlock % groups == 0;
    float pk[4][8], bb[8];
    int co_held = -1;
    for (int i = 0; i < kImagePx; ++i) {
        const int idx = (blockIdx.y * kImagePx + i) * kBlock + threadIdx.x;
        if (idx >= items) return;
        const int xx = idx / groups;
        const int co = (idx - xx * groups) * 8;
        if (!fixed || co_held != co) {
            co_held = co;
#pragma unroll
            for (int ci = 0; ci < 4; ++ci) {
                const float4 p0 = ci < cin ? ld4(pw + (size_t)ci * cout + co) : f4(0.f);
                const float4 p1 = ci < cin ? ld4(pw + (size_t)ci * cout + co + 4) : f4(0.f);
                pk[ci][0] = p0.x, pk[ci][1] = p0.y, pk[ci][2] = p0.z, pk[ci][3] = p0.w;
                pk[ci][4] = p1.x, pk[ci][5] = p1.y, pk[ci][6] = p1.z, pk[ci][7] = p1.w;
            }
            const float4 b0 = ld4(bias + co), b1 = ld4(bias + co + 4);
            bb[0] = b0.x, bb[1] = b0.y, bb[2] = b0.z, bb[3] = b0.w;
            bb[4] = b1.x, bb[5] = b1.y, bb[6] = b1.z, bb[7] = b1.w;
        }
        float yv[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const int dy = t / 3 - 1, sx = xx + t % 3 - 1;
            if (y + dy < 0 || y + dy >= h || sx < 0 || sx >= w) continue;
            const float* px = x + (size_t)((int64_t)row0 + (int64_t)dy * w + sx) * cin;
#pragma unroll
            for (int ci = 0; ci < 4; ++ci)
                if (ci < cin) yv[ci] = fmaf(px[ci], dw[t * cin + ci], yv[ci]);
        }
        unsigned res[2] = {0u, 0u};
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            float o = 0.f;
#pragma unroll
            for (int ci = 0; ci < 4; ++ci) o = fmaf(yv[ci], pk[ci][j], o);  // channels past cin: 0 * 0
            res[j >> 2] |= (unsigned)quant(relu(o + bb[j]) / s_out, 0.f, 255.f) << (8 * (j & 3));
        }
        *reinterpret_cast<uint2*>(out + (row0 + xx) * cout + co) = make_uint2(res[0], res[1]);
    }
}

// -------------------------------------------------------------------------- head ----
// Eight lanes per pixel: lane `sub` reads the 8-byte chunks sub, sub + 8, ... of the pixel's
// channels, the partial logits meet in three shuffles.  The input scale is folded into `kern`.
__device__ __forceinline__ float head_logit(const u8* __restrict__ px, int cin, int sub, const float* __restrict__ kern,
                                            int ncls, int c, float b) {
    float l = 0.f;
    for (int k = 8 * sub; k < cin; k += 64) {
        const uint2 xv = *reinterpret_cast<const uint2*>(px + k);
#pragma unroll
        for (int j = 0; j < 4; ++j) l = fmaf(byte_f32<false>(xv.x, j), kern[(size_t)(k + j) * ncls + c], l);
#pragma unroll
        for (int j = 0; j < 4; ++j) l = fmaf(byte_f32<false>(xv.y, j), kern[(size_t)(k + 4 + j) * ncls + c], l);
    }
    l += __shfl_xor(l, 1, 64);
    l += __shfl_xor(l, 2, 64);
    l += __shfl_xor(l, 4, 64);
    return l + b;
}

__global__ __launch_bounds__(kBlock) void i8_head_kernel(const u8* __restrict__ x, int64_t M, int cin, int ncls,
                                                         const float* __restrict__ kern, const float* __restrict__ bias,
                                                         float* __restrict__ prob) {
    const int64_t m = ((int64_t)blockIdx.x * kBlock + threadIdx.x) >> 3;
    const int sub = threadIdx.x & 7;
    const bool valid = m < M;  // lanes past the end keep running for the shuffles, on pixel 0
    const u8* px = x + (size_t)(valid ? m : 0) * cin;
    if (ncls == 1) {
        const float l = head_logit(px, cin, sub, kern, 1, 0, bias[0]);
        if (valid && sub == 0) prob[m] = 1.f / (1.f + expf(-l));
        return;
    }
    float mx = -INFINITY, s = 0.f;  // online softmax: max and sum in one pass over the classes
    for (int c = 0; c < ncls; ++c) {
        const float l = head_logit(px, cin, sub, kern, ncls, c, bias[c]);
        const float mn = fmaxf(mx, l);
        s = s * expf(mx - mn) + expf(l - mn);
        mx = mn;
    }
    const float inv = 1.f / s;
    for (int c = 0; c < ncls; ++c) {
        const float l = head_logit(px, cin, sub, kern, ncls, c, bias[c]);
        if (valid && sub == (c & 7)) prob[(size_t)m * ncls + c] = expf(l - mx) * inv;
    }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace
}  // namespace unet

using namespace unet;

extern "C" int unet_i8_image_block(const float* x, int n, int h, int w, int cin, const float* dw_kernel, int cout,
                                   const float* pw_folded, const float* bias, float out_scale, unsigned char* out,
                                   unet_stream_t stream) {
    UNET_CHECK_ARG(x && dw_kernel && pw_folded && bias && out, "unet_i8_image_block: null pointer");
    UNET_CHECK_ARG(n > 0 && h > 0 && w > 0, "unet_i8_image_block: empty tensor (%d, %d, %d)", n, h, w);
    UNET_CHECK_ARG(cin >= 1 && cin <= 4, "unet_i8_image_block: cin %d not in 1..4", cin);
    UNET_CHECK_ARG(cout > 0 && cout % 32 == 0, "unet_i8_image_block: cout %d not a positive multiple of 32", cout);
    UNET_CHECK_ARG(out_scale > 0.f && out_scale < INFINITY, "unet_i8_image_block: out_scale %g not positive and finite",
                   (double)out_scale);
    UNET_CHECK_ARG(aligned16(pw_folded) && aligned16(bias) && aligned16(out),
                   "unet_i8_image_block: pw_folded / bias / out must be 16-byte aligned");
    const int64_t items = (int64_t)w * (cout / 8);  // per image row
    UNET_CHECK_ARG((int64_t)n * h < (1ll << 31) && items < (1ll << 30) && cdiv(items, kBlock * kImagePx) < 65536,
                   "unet_i8_image_block: tensor too large");
    const dim3 grid((unsigned)(n * h), (unsigned)cdiv(items, kBlock * kImagePx));
    i8_image_kernel<<<grid, kBlock, 0, as_stream(stream)>>>(x, n, h, w, cin, dw_kernel, cout, pw_folded, bias,
                                                            out_scale, out);
    UNET_CHECK_LAUNCH("unet_i8_image_block");
    return 0;
}

extern "C" int unet_i8_sepconv(const unet_i8_view* x, int n, int h, int w, const float* taps, int cout,
                               const signed char* pw_q, const float* mult, const float* bias_q, unsigned char* out,
                               unsigned char* out_pool, int route, unet_stream_t stream) {
    UNET_CHECK_ARG(x && taps && pw_q && mult && bias_q && out, "unet_i8_sepconv: null pointer");
    UNET_CHECK_ARG(n > 0 && h > 0 && w > 0, "unet_i8_sepconv: empty tensor (%d, %d, %d)", n, h, w);
    UNET_CHECK_ARG(x->mode == UNET_I8_VIEW_PLAIN || x->mode == UNET_I8_VIEW_CONCAT, "unet_i8_sepconv: bad view mode %d",
                   x->mode);
    SrcView v;
    v.src0 = reinterpret_cast<const u8*>(x->src0);
    v.c0 = x->c0;
    v.sg0 = x->signed0 != 0;
    const bool cat = x->mode == UNET_I8_VIEW_CONCAT;
    v.src1 = cat ? reinterpret_cast<const u8*>(x->src1) : nullptr;
    v.c1 = cat ? x->c1 : 0;
    v.sg1 = cat && x->signed1 != 0;
    UNET_CHECK_ARG(v.src0 && (!cat || v.src1), "unet_i8_sepconv: null view source");
    UNET_CHECK_ARG(v.c0 > 0 && (!cat || v.c1 > 0) && (v.c0 + v.c1) % 32 == 0,
                   "unet_i8_sepconv: view channels (%d, %d) must be positive and sum to a multiple of 32", v.c0, v.c1);
    UNET_CHECK_ARG(!cat || v.c0 % 16 == 0, "unet_i8_sepconv: concat c0 %d not a multiple of 16", v.c0);
    UNET_CHECK_ARG(cout > 0 && cout % 32 == 0, "unet_i8_sepconv: cout %d not a positive multiple of 32", cout);
    UNET_CHECK_ARG(route >= 0 && route <= 2, "unet_i8_sepconv: bad route %d", route);
    UNET_CHECK_ARG(!out_pool || (h % 2 == 0 && w % 2 == 0), "unet_i8_sepconv: out_pool needs even h, w (%d, %d)", h,
                   w);
    UNET_CHECK_ARG(aligned16(v.src0) && aligned16(v.src1) && aligned16(taps) && aligned16(pw_q) && aligned16(out) &&
                       aligned16(out_pool),
                   "unet_i8_sepconv: tensors must be 16-byte aligned");
    const bool can_tile = h % 8 == 0 && w % 16 == 0;
    UNET_CHECK_ARG(route != 2 || can_tile, "unet_i8_sepconv: route 2 (tile) needs h %% 8 == 0 and w %% 16 == 0");
    const bool tile = route == 2 || (route == 0 && can_tile);
    const int64_t M = (int64_t)n * h * w;
    const int64_t gx = tile ? M / kRows : cdiv(M, kRows);
    // columns per block: unet_f16_sepconv's rule (128 where that divides cout, narrower while the
    // grid would leave the 256 CUs fewer than two blocks each)
    int nt = cout % 128 == 0 ? 4 : cout % 64 == 0 ? 2 : 1;
    while (nt > 1 && gx * (cout / (32 * nt)) < kMinBlocks) nt >>= 1;
    UNET_CHECK_ARG(gx < (1ll << 31), "unet_i8_sepconv: tensor too large");
    const dim3 grid((unsigned)gx, (unsigned)(cout / (32 * nt)));
    const u8* pw = reinterpret_cast<const u8*>(pw_q);
    hipStream_t s = as_stream(stream);
    with_int<4, 2, 1>(nt, [&](auto NT) {
        with_bool(tile, [&](auto TILE) {
            i8_sep_kernel<NT(), TILE()><<<grid, kBlock, 0, s>>>(v, n, h, w, taps, cout, pw, mult, bias_q, out, out_pool);
        });
    });
    UNET_CHECK_LAUNCH("unet_i8_sepconv");
    return 0;
}

extern "C" int unet_i8_conv_transpose2x2(const unsigned char* x, int n, int h, int w, int cin, int cout,
                                         const signed char* kernel_q, const int32_t* colsum, const float* mult,
                                         const float* bias_q, signed char* out, unet_stream_t stream) {
    UNET_CHECK_ARG(x && kernel_q && colsum && mult && bias_q && out, "unet_i8_conv_transpose2x2: null pointer");
    UNET_CHECK_ARG(n > 0 && h > 0 && w > 0, "unet_i8_conv_transpose2x2: empty tensor (%d, %d, %d)", n, h, w);
    UNET_CHECK_ARG(cin > 0 && cin % 32 == 0, "unet_i8_conv_transpose2x2: cin %d not a positive multiple of 32", cin);
    UNET_CHECK_ARG(cout > 0 && cout % 32 == 0, "unet_i8_conv_transpose2x2: cout %d not a positive multiple of 32",
                   cout);
    UNET_CHECK_ARG(aligned16(x) && aligned16(kernel_q) && aligned16(out),
                   "unet_i8_conv_transpose2x2: tensors must be 16-byte aligned");
    const int N = 4 * cout;  // a multiple of 128
    const int64_t M = (int64_t)n * h * w;
    UNET_CHECK_ARG(M < (1ll << 31), "unet_i8_conv_transpose2x2: tensor too large");
    const dim3 grid((unsigned)cdiv(M, kRows), (unsigned)(N / 128));
    i8_convt_kernel<4><<<grid, kBlock, 0, as_stream(stream)>>>(x, n, h, w, cin, cout,
                                                               reinterpret_cast<const u8*>(kernel_q), colsum, mult,
                                                               bias_q, reinterpret_cast<u8*>(out));
    UNET_CHECK_LAUNCH("unet_i8_conv_transpose2x2");
    return 0;
}

extern "C" int unet_i8_head(const unsigned char* x, int n, int h, int w, int cin, int ncls, const float* kernel,
                            const float* bias, float* prob, unet_stream_t stream) {
    UNET_CHECK_ARG(x && kernel && bias && prob, "unet_i8_head: null pointer");
    UNET_CHECK_ARG(n > 0 && h > 0 && w > 0, "unet_i8_head: empty tensor (%d, %d, %d)", n, h, w);
    UNET_CHECK_ARG(cin > 0 && cin % 8 == 0, "unet_i8_head: cin %d not a positive multiple of 8", cin);
    UNET_CHECK_ARG(ncls >= 1, "unet_i8_head: ncls %d < 1", ncls);
    UNET_CHECK_ARG(aligned16(x), "unet_i8_head: x must be 16-byte aligned");
    const int64_t M = (int64_t)n * h * w;
    UNET_CHECK_ARG(cdiv(M * 8, kBlock) < (1ll << 31), "unet_i8_head: tensor too large");
    i8_head_kernel<<<dim3((unsigned)cdiv(M * 8, kBlock)), kBlock, 0, as_stream(stream)>>>(x, M, cin, ncls, kernel, bias,
                                                                                         prob);
    UNET_CHECK_LAUNCH("unet_i8_head");
    return 0;
}
