// Frozen half-precision inference (ABI 13): the kernels behind UNetModel.freeze().
//
// BatchNorm is folded into the pointwise weights on the host (unet_amd/frozen.py), so a conv
// block is depthwise 3x3 -> pointwise GEMM -> + bias -> ReLU.  Activations are NHWC fp16 and are
// stored already activated; the pointwise GEMMs run on v_mfma_f32_32x32x16_f16 with fp32
// accumulators.  Rounding to fp16 (nearest even) happens at exactly four places: the folded
// weights (host), each block's depthwise output, each block's output, each upsample's output.
//
// MFMA lane maps (32x32x16, 16-bit operands): lane l, r = l & 31, hh = l >> 5 holds
// A[row r][k = 8 hh + j] and B[k = 8 hh + j][col r], j = 0..7; the accumulator register i of that
// lane is D[row (i & 3) + 8 (i >> 2) + 4 hh][col r].  GEMM rows are pixels, columns are output
// channels.
#include "common.h"
#include "dispatch.h"

namespace unet {
namespace {

typedef _Float16 halfx8 __attribute__((ext_vector_type(8)));
typedef _Float16 half_t;

constexpr int kBlock = 256;   // 4 waves, 32 GEMM rows each
constexpr int kRows = 128;    // GEMM rows per block
constexpr int kMinBlocks = 512;  // below this a launch takes narrower column blocks
constexpr int kKC = 64;       // channels of one LDS halo chunk (tile policy)
constexpr int kHaloW = 18, kHaloH = 10, kHaloPx = kHaloW * kHaloH;
constexpr int kHaloLd = kKC + 8;  // halves per halo pixel: 144 B, 16-B slots 9 p + s are conflict free

__device__ __forceinline__ uint4 ldg16(const half_t* p) { return *reinterpret_cast<const uint4*>(p); }
__device__ __forceinline__ halfx8 as_h8(uint4 v) { return __builtin_bit_cast(halfx8, v); }

struct SrcView {
    const half_t* src0;
    const half_t* src1;
    int c0, c1;
};
// 8 channels c..c+7 of pixel `pix` of the logical tensor (c % 8 == 0, c0 % 16 == 0)
__device__ __forceinline__ uint4 view_ld(const SrcView& v, size_t pix, int c) {
    return c < v.c0 ? ldg16(v.src0 + pix * (size_t)v.c0 + c) : ldg16(v.src1 + pix * (size_t)v.c1 + (c - v.c0));
}

// depthwise accumulation of one tap for 8 channels: a[j] = fmaf(x[j], w[j], a[j]) (the one order
// both tap-fetch policies share)
__device__ __forceinline__ void tap_fma(float (&a)[8], uint4 xv, float4 w0, float4 w1) {
    const halfx8 x = as_h8(xv);
    a[0] = fmaf((float)x[0], w0.x, a[0]);
    a[1] = fmaf((float)x[1], w0.y, a[1]);
    a[2] = fmaf((float)x[2], w0.z, a[2]);
    a[3] = fmaf((float)x[3], w0.w, a[3]);
    a[4] = fmaf((float)x[4], w1.x, a[4]);
    a[5] = fmaf((float)x[5], w1.y, a[5]);
    a[6] = fmaf((float)x[6], w1.z, a[6]);
    a[7] = fmaf((float)x[7], w1.w, a[7]);
}

// Where GEMM row `m` of the launch lives in the image.
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

// Epilogue staging: a wave's 32 x (32 EG) result (and its 8 pooled rows) as fp16 in LDS, so the
// global stores are 16 bytes of contiguous channels per lane.
template <int EG>
struct Stage {
    static constexpr int kLd = 32 * EG + 8;                    // halves per row
    static constexpr int kWaveHalves = (32 + 8) * kLd;         // 32 rows + 8 pooled rows
    static constexpr int kBytes = 4 * kWaveHalves * 2;
};

// ------------------------------------------------------------------ separable conv ----
template <int NT, bool TILE>
__global__ __launch_bounds__(kBlock) void f16_sep_kernel(SrcView v, int n, int h, int w, const float* __restrict__ dw,
                                                         int cout, const half_t* __restrict__ pw,
                                                         const float* __restrict__ bias, half_t* __restrict__ out,
                                                         half_t* __restrict__ out_pool) {
    constexpr int EG = NT < 4 ? NT : 4;
    using St = Stage<EG>;
    // tile policy: the chunk's halo, then its depthwise taps [9][kKC] fp32 (every lane of a half
    // wave reads the same 32 bytes per tap: an LDS broadcast instead of a 1-KiB vector load)
    constexpr int kHaloBytes = TILE ? kHaloPx * kHaloLd * 2 : 0;
    constexpr int kTapBytes = TILE ? 9 * kKC * 4 : 0;
    constexpr int kSmem = St::kBytes > kHaloBytes + kTapBytes ? St::kBytes : kHaloBytes + kTapBytes;
    __shared__ __attribute__((aligned(16))) unsigned char smem_raw[kSmem];
    half_t* const smem = reinterpret_cast<half_t*>(smem_raw);
    float* const taps = reinterpret_cast<float*>(smem_raw + kHaloBytes);

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

    floatx16 acc[NT];
#pragma unroll
    for (int i = 0; i < NT; ++i)
#pragma unroll
        for (int j = 0; j < 16; ++j) acc[i][j] = 0.f;

    for (int kc0 = 0; kc0 < C; kc0 += kKC) {
        const int kcn = (C - kc0) < kKC ? (C - kc0) : kKC;
        if constexpr (TILE) {
            __syncthreads();
            const int segs = kcn >> 3;
            for (int idx = tid; idx < kHaloPx * segs; idx += kBlock) {
                const int p = idx / segs, s = idx - p * segs;
                const int gy = tile_y0 + p / kHaloW - 1, gx = tile_x0 + p % kHaloW - 1;
                uint4 val = make_uint4(0, 0, 0, 0);
                if (gy >= 0 && gy < h && gx >= 0 && gx < w)
                    val = view_ld(v, ((size_t)tile_img * h + gy) * w + gx, kc0 + 8 * s);
                *reinterpret_cast<uint4*>(smem + p * kHaloLd + 8 * s) = val;
            }
            const int quads = kcn >> 2;
            for (int idx = tid; idx < 9 * quads; idx += kBlock) {
                const int t = idx / quads, q = idx - t * quads;
                st4(taps + t * kKC + 4 * q, ld4(dw + (size_t)t * C + kc0 + 4 * q));
            }
            __syncthreads();
        }
        for (int ks = 0; ks < kcn; ks += 16) {
            const int cl = ks + 8 * hh;   // channel inside the chunk
            const int c = kc0 + cl;       // channel of the logical tensor
            float a[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) a[j] = 0.f;
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                const int dy = t / 3 - 1, dx = t % 3 - 1;
                uint4 xv;
                float4 w0, w1;
                if constexpr (TILE) {
                    const int ly = me.y - tile_y0 + 1 + dy, lx = me.x - tile_x0 + 1 + dx;
                    xv = *reinterpret_cast<const uint4*>(smem + (ly * kHaloW + lx) * kHaloLd + cl);
                    w0 = ld4(taps + t * kKC + cl);
                    w1 = ld4(taps + t * kKC + cl + 4);
                } else {
                    w0 = ld4(dw + (size_t)t * C + c);
                    w1 = ld4(dw + (size_t)t * C + c + 4);
                    const int yy = me.y + dy, xx = me.x + dx;
                    xv = make_uint4(0, 0, 0, 0);
                    if (me.valid && yy >= 0 && yy < h && xx >= 0 && xx < w)
                        xv = view_ld(v, ((size_t)me.img * h + yy) * w + xx, c);
                }
                tap_fma(a, xv, w0, w1);
            }
            halfx8 af;
#pragma unroll
            for (int j = 0; j < 8; ++j) af[j] = (half_t)a[j];
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const halfx8 bf = as_h8(ldg16(pw + (size_t)(nb0 + nt * 32 + r) * C + c));
                acc[nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af, bf, acc[nt], 0, 0, 0);
            }
        }
    }

    // epilogue: + bias, ReLU, fp16, staged through LDS in groups of EG column tiles
    half_t* const st = smem + wave * St::kWaveHalves;
    half_t* const stp = st + 32 * St::kLd;
#pragma unroll
    for (int g0 = 0; g0 < NT; g0 += EG) {
        __syncthreads();
#pragma unroll
        for (int e = 0; e < EG; ++e) {
            const int col = e * 32 + r;
            const float b = bias[nb0 + (g0 + e) * 32 + r];
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                half_t mx = (half_t)0.f;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int reg = 4 * g + i;
                    const int row = (reg & 3) + 8 * (reg >> 2) + 4 * hh;
                    const half_t o = (half_t)relu(acc[g0 + e][reg] + b);
                    st[row * St::kLd + col] = o;
                    mx = o > mx ? o : mx;
                }
                stp[(hh + 2 * g) * St::kLd + col] = mx;
            }
        }
        __syncthreads();
        constexpr int kChunks = EG * 4;  // 16-B chunks per row
        for (int idx = lane; idx < 32 * kChunks; idx += 64) {
            const int row = idx / kChunks, ch = idx - row * kChunks;
            const RowPos p = row_pos<TILE>(m_wave + row, M, h, w, pooled, tile_img, tile_y0, tile_x0);
            if (p.valid) {
                const size_t pix = ((size_t)p.img * h + p.y) * w + p.x;
                *reinterpret_cast<uint4*>(out + pix * cout + nb0 + g0 * 32 + ch * 8) =
                    *reinterpret_cast<const uint4*>(st + row * St::kLd + ch * 8);
            }
        }
        if (pooled) {
            for (int idx = lane; idx < 8 * kChunks; idx += 64) {
                const int q = idx / kChunks, ch = idx - q * kChunks;
                // the window's first row tells where it is
                const RowPos p = row_pos<TILE>(m_wave + 4 * q, M, h, w, true, tile_img, tile_y0, tile_x0);
                if (p.valid) {
                    const size_t pix = ((size_t)p.img * (h >> 1) + (p.y >> 1)) * (w >> 1) + (p.x >> 1);
                    *reinterpret_cast<uint4*>(out_pool + pix * cout + nb0 + g0 * 32 + ch * 8) =
                        *reinterpret_cast<const uint4*>(stp + q * St::kLd + ch * 8);
                }
            }
        }
    }
}

// --------------------------------------------------------------- transposed conv ----
// GEMM rows = input pixels, K = cin, columns = (a, b, co) of the Keras (2, 2, cout, cin) kernel,
// which is already [column][k] with k contiguous.
template <int NT>
__global__ __launch_bounds__(kBlock) void f16_convt_kernel(const half_t* __restrict__ x, int n, int h, int w, int cin,
                                                           int cout, const half_t* __restrict__ kern,
                                                           const float* __restrict__ bias, half_t* __restrict__ out) {
    using St = Stage<NT>;
    __shared__ __attribute__((aligned(16))) unsigned char smem_raw[St::kBytes];
    half_t* const smem = reinterpret_cast<half_t*>(smem_raw);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, hh = lane >> 5;
    const int nb0 = blockIdx.y * (32 * NT);
    const int64_t M = (int64_t)n * h * w;
    const int64_t m_wave = (int64_t)blockIdx.x * kRows + wave * 32;
    const int64_t m = m_wave + r;
    const bool valid = m < M;

    floatx16 acc[NT];
#pragma unroll
    for (int i = 0; i < NT; ++i)
#pragma unroll
        for (int j = 0; j < 16; ++j) acc[i][j] = 0.f;

    for (int k0 = 0; k0 < cin; k0 += 16) {
        const int c = k0 + 8 * hh;
        uint4 av = make_uint4(0, 0, 0, 0);
        if (valid) av = ldg16(x + (size_t)m * cin + c);
        const halfx8 af = as_h8(av);
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const halfx8 bf = as_h8(ldg16(kern + (size_t)(nb0 + nt * 32 + r) * cin + c));
            acc[nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af, bf, acc[nt], 0, 0, 0);
        }
    }

    half_t* const st = smem + wave * St::kWaveHalves;
#pragma unroll
    for (int e = 0; e < NT; ++e) {
        const int col = e * 32 + r;
        const float b = bias[(nb0 + col) % cout];
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const int row = (reg & 3) + 8 * (reg >> 2) + 4 * hh;
            st[row * St::kLd + col] = (half_t)(acc[e][reg] + b);
        }
    }
    __syncthreads();
    // a lane keeps its 16-byte column chunk and walks the rows: the (a, b, co) split of the column
    // is computed once, the row's (img, y, x) in 32-bit arithmetic (the entry point bounds M)
    constexpr int kChunks = NT * 4, kRowStep = 64 / kChunks;
    const int ch = lane % kChunks;
    const int col = nb0 + ch * 8;
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
                *reinterpret_cast<const uint4*>(st + row * St::kLd + ch * 8);
        }
    }
}

// ------------------------------------------------------------------- image block ----
// One thread: 8 output channels of up to kImagePx pixels of ONE image row (blockIdx.x = the row,
// so (img, y) cost the block one scalar division).  All fp32 up to the output rounding.  The
// folded weights of the thread's channel group stay in registers over its pixels where the
// block size is a multiple of the group count (cout = 64: 8 groups).
constexpr int kImagePx = 8;
__global__ __launch_bounds__(kBlock) void f16_image_kernel(const float* __restrict__ x, int n, int h, int w, int cin,
                                                           const float* __restrict__ dw, int cout,
                                                           const float* __restrict__ pw, const float* __restrict__ bias,
                                                           half_t* __restrict__ out) {
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
        halfx8 res;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            float o = 0.f;
#pragma unroll
            for (int ci = 0; ci < 4; ++ci) o = fmaf(yv[ci], pk[ci][j], o);  // channels past cin: 0 * 0
            res[j] = (half_t)relu(o + bb[j]);
        }
        *reinterpret_cast<uint4*>(out + (row0 + xx) * cout + co) = __builtin_bit_cast(uint4, res);
    }
}

// -------------------------------------------------------------------------- head ----
// Eight lanes per pixel: lane `sub` reads the 16-byte chunks sub, sub + 8, ... of the pixel's
// channels (a wave reads whole 128-byte runs), the partial logits meet in three shuffles.
__device__ __forceinline__ float head_logit(const half_t* __restrict__ px, int cin, int sub,
                                            const float* __restrict__ kern, int ncls, int c, float b) {
    float l = 0.f;
    for (int k = 8 * sub; k < cin; k += 64) {
        const halfx8 xv = as_h8(ldg16(px + k));
#pragma unroll
        for (int j = 0; j < 8; ++j) l = fmaf((float)xv[j], kern[(size_t)(k + j) * ncls + c], l);
    }
    l += __shfl_xor(l, 1, 64);
    l += __shfl_xor(l, 2, 64);
    l += __shfl_xor(l, 4, 64);
    return l + b;
}

__global__ __launch_bounds__(kBlock) void f16_head_kernel(const half_t* __restrict__ x, int64_t M, int cin, int ncls,
                                                          const float* __restrict__ kern,
                                                          const float* __restrict__ bias, float* __restrict__ prob) {
    const int64_t m = ((int64_t)blockIdx.x * kBlock + threadIdx.x) >> 3;
    const int sub = threadIdx.x & 7;
    const bool valid = m < M;  // lanes past the end keep running for the shuffles, on pixel 0
    const half_t* px = x + (size_t)(valid ? m : 0) * cin;
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

extern "C" int unet_f16_image_block(const float* x, int n, int h, int w, int cin, const float* dw_kernel, int cout,
                                    const float* pw_folded, const float* bias, unsigned short* out,
                                    unet_stream_t stream) {
    UNET_CHECK_ARG(x && dw_kernel && pw_folded && bias && out, "unet_f16_image_block: null pointer");
    UNET_CHECK_ARG(n > 0 && h > 0 && w > 0, "unet_f16_image_block: empty tensor (%d, %d, %d)", n, h, w);
    UNET_CHECK_ARG(cin >= 1 && cin <= 4, "unet_f16_image_block: cin %d not in 1..4", cin);
    UNET_CHECK_ARG(cout > 0 && cout % 8 == 0, "unet_f16_image_block: cout %d not a positive multiple of 8", cout);
    UNET_CHECK_ARG(aligned16(pw_folded) && aligned16(bias) && aligned16(out),
                   "unet_f16_image_block: pw_folded / bias / out must be 16-byte aligned");
    const int64_t items = (int64_t)w * (cout / 8);  // per image row
    UNET_CHECK_ARG((int64_t)n * h < (1ll << 31) && items < (1ll << 30) && cdiv(items, kBlock * kImagePx) < 65536,
                   "unet_f16_image_block: tensor too large");
    const dim3 grid((unsigned)(n * h), (unsigned)cdiv(items, kBlock * kImagePx));
    f16_image_kernel<<<grid, kBlock, 0, as_stream(stream)>>>(
        x, n, h, w, cin, dw_kernel, cout, pw_folded, bias, reinterpret_cast<half_t*>(out));
    UNET_CHECK_LAUNCH("unet_f16_image_block");
    return 0;
}

extern "C" int unet_f16_sepconv(const unet_f16_view* x, int n, int h, int w, const float* dw_kernel, int cout,
                                const unsigned short* pw_t, const float* bias, unsigned short* out,
                                unsigned short* out_pool, int route, unet_stream_t stream) {
    UNET_CHECK_ARG(x && dw_kernel && pw_t && bias && out, "unet_f16_sepconv: null pointer");
    UNET_CHECK_ARG(n > 0 && h > 0 && w > 0, "unet_f16_sepconv: empty tensor (%d, %d, %d)", n, h, w);
    UNET_CHECK_ARG(x->mode == UNET_F16_VIEW_PLAIN || x->mode == UNET_F16_VIEW_CONCAT,
                   "unet_f16_sepconv: bad view mode %d", x->mode);
    SrcView v;
    v.src0 = reinterpret_cast<const half_t*>(x->src0);
    v.c0 = x->c0;
    const bool cat = x->mode == UNET_F16_VIEW_CONCAT;
    v.src1 = cat ? reinterpret_cast<const half_t*>(x->src1) : nullptr;
    v.c1 = cat ? x->c1 : 0;
    UNET_CHECK_ARG(v.src0 && (!cat || v.src1), "unet_f16_sepconv: null view source");
    UNET_CHECK_ARG(v.c0 > 0 && v.c0 % 16 == 0 && (!cat || (v.c1 > 0 && v.c1 % 16 == 0)),
                   "unet_f16_sepconv: view channels (%d, %d) must be positive multiples of 16", v.c0, v.c1);
    UNET_CHECK_ARG(cout > 0 && cout % 32 == 0, "unet_f16_sepconv: cout %d not a positive multiple of 32", cout);
    UNET_CHECK_ARG(route >= 0 && route <= 2, "unet_f16_sepconv: bad route %d", route);
    UNET_CHECK_ARG(!out_pool || (h % 2 == 0 && w % 2 == 0), "unet_f16_sepconv: out_pool needs even h, w (%d, %d)", h,
                   w);
    UNET_CHECK_ARG(aligned16(v.src0) && aligned16(v.src1) && aligned16(dw_kernel) && aligned16(pw_t) &&
                       aligned16(out) && aligned16(out_pool),
                   "unet_f16_sepconv: tensors must be 16-byte aligned");
    const bool can_tile = h % 8 == 0 && w % 16 == 0;
    UNET_CHECK_ARG(route != 2 || can_tile, "unet_f16_sepconv: route 2 (tile) needs h %% 8 == 0 and w %% 16 == 0");
    const bool tile = route == 2 || (route == 0 && can_tile);
    const int64_t M = (int64_t)n * h * w;
    const int64_t gx = tile ? M / kRows : cdiv(M, kRows);
    // Columns per block: 128 where that divides cout (the depthwise output is recomputed per column
    // block), narrower while the grid would leave the 256 CUs fewer than two blocks each.  (A
    // 256-column block needs 128 accumulator registers: one wave per SIMD, nothing hides a load.)
    int nt = cout % 128 == 0 ? 4 : cout % 64 == 0 ? 2 : 1;
    while (nt > 1 && gx * (cout / (32 * nt)) < kMinBlocks) nt >>= 1;
    UNET_CHECK_ARG(gx < (1ll << 31), "unet_f16_sepconv: tensor too large");
    const dim3 grid((unsigned)gx, (unsigned)(cout / (32 * nt)));
    half_t* o = reinterpret_cast<half_t*>(out);
    half_t* op = reinterpret_cast<half_t*>(out_pool);
    const half_t* pw = reinterpret_cast<const half_t*>(pw_t);
    hipStream_t s = as_stream(stream);
    with_int<4, 2, 1>(nt, [&](auto NT) {
        with_bool(tile, [&](auto TILE) {
            f16_sep_kernel<NT(), TILE()><<<grid, kBlock, 0, s>>>(v, n, h, w, dw_kernel, cout, pw, bias, o, op);
        });
    });
    UNET_CHECK_LAUNCH("unet_f16_sepconv");
    return 0;
}

extern "C" int unet_f16_conv_transpose2x2(const unsigned short* x, int n, int h, int w, int cin, int cout,
                                          const unsigned short* kernel, const float* bias, unsigned short* out,
                                          unet_stream_t stream) {
    UNET_CHECK_ARG(x && kernel && bias && out, "unet_f16_conv_transpose2x2: null pointer");
    UNET_CHECK_ARG(n > 0 && h > 0 && w > 0, "unet_f16_conv_transpose2x2: empty tensor (%d, %d, %d)", n, h, w);
    UNET_CHECK_ARG(cin > 0 && cin % 16 == 0, "unet_f16_conv_transpose2x2: cin %d not a positive multiple of 16", cin);
    UNET_CHECK_ARG(cout > 0 && cout % 8 == 0, "unet_f16_conv_transpose2x2: cout %d not a positive multiple of 8",
                   cout);
    UNET_CHECK_ARG(aligned16(x) && aligned16(kernel) && aligned16(out),
                   "unet_f16_conv_transpose2x2: tensors must be 16-byte aligned");
    const int N = 4 * cout;
    const int nt = N % 128 == 0 ? 4 : N % 64 == 0 ? 2 : 1;
    const int64_t M = (int64_t)n * h * w;
    UNET_CHECK_ARG(M < (1ll << 31), "unet_f16_conv_transpose2x2: tensor too large");
    const dim3 grid((unsigned)cdiv(M, kRows), (unsigned)(N / (32 * nt)));
    const half_t* xs = reinterpret_cast<const half_t*>(x);
    const half_t* ks = reinterpret_cast<const half_t*>(kernel);
    half_t* o = reinterpret_cast<half_t*>(out);
    hipStream_t s = as_stream(stream);
    with_int<4, 2, 1>(nt, [&](auto NT) {
        f16_convt_kernel<NT()><<<grid, kBlock, 0, s>>>(xs, n, h, w, cin, cout, ks, bias, o);
    });
    UNET_CHECK_LAUNCH("unet_f16_conv_transpose2x2");
    return 0;
}

extern "C" int unet_f16_head(const unsigned short* x, int n, int h, int w, int cin, int ncls, const float* kernel,
                             const float* bias, float* prob, unet_stream_t stream) {
    UNET_CHECK_ARG(x && kernel && bias && prob, "unet_f16_head: null pointer");
    UNET_CHECK_ARG(n > 0 && h > 0 && w > 0, "unet_f16_head: empty tensor (%d, %d, %d)", n, h, w);
    UNET_CHECK_ARG(cin > 0 && cin % 8 == 0, "unet_f16_head: cin %d not a positive multiple of 8", cin);
    UNET_CHECK_ARG(ncls >= 1, "unet_f16_head: ncls %d < 1", ncls);
    UNET_CHECK_ARG(aligned16(x), "unet_f16_head: x must be 16-byte aligned");
    const int64_t M = (int64_t)n * h * w;
    UNET_CHECK_ARG(cdiv(M * 8, kBlock) < (1ll << 31), "unet_f16_head: tensor too large");
    f16_head_kernel<<<dim3((unsigned)cdiv(M * 8, kBlock)), kBlock, 0, as_stream(stream)>>>(
        reinterpret_cast<const half_t*>(x), M, cin, ncls, kernel, bias, prob);
    UNET_CHECK_LAUNCH("unet_f16_head");
    return 0;
}
