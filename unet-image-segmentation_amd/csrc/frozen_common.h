// The one skeleton of the frozen-inference kernels: everything that does not depend on the element
// type.  frozen.hip (fp16, ABI 13) and frozen_i8.hip (int8, ABI 14) each add a precision traits
// struct P and their entry points; a change to the tiling, the halo, the row orders, the pooled
// epilogue or the column-block policy is made here, once, for every precision.
//
// A conv block is depthwise 3x3 -> pointwise GEMM -> per-column epilogue; activations are NHWC and
// are stored already activated.  GEMM rows are pixels, columns are output channels.  Both MFMAs
// (32x32x16 fp16, 32x32x32 int8) give lane l, r = l & 31, hh = l >> 5 one 16-byte A operand of row r
// and one 16-byte B operand of column r, P::kLane channels from P::kLane hh of the K step, and keep
// D[row (i & 3) + 8 (i >> 2) + 4 hh][col r] in accumulator register i of that lane.
//
// What a precision P supplies:
//   Elem, kLane (channels of a 16-byte load: 8 / 16), kStep (channels of one MFMA: 2 kLane),
//   kHaloLd (elements per LDS halo pixel), Frag / Acc / mfma() (operand and accumulator vectors,
//   the builtin);
//   View (the kernel's source view), with_source() (calls its argument with the kind of source
//   channel c comes from), tap_fma() (one depthwise tap, a[j] = fmaf(x[j], w[j], a[j]) over the
//   kLane channels of a 16-byte load) and round_a() (a -> the A operand);
//   sep_col() / sep_out() and convt_a() / convt_col() / convt_out() (one column's epilogue values
//   from the arrays the kernel takes, accumulator -> stored element, the upsample's A operand; Out
//   is the type the pooled max compares);
//   Image8 / image_put() / image_store() (rounds, packs and stores the image block's 8 fp32
//   results) and head_ld8() / head_x() (8 channels of the head's input).
#pragma once
#include "common.h"
#include "dispatch.h"

namespace unet {
namespace frozen {

constexpr int kBlock = 256;   // 4 waves, 32 GEMM rows each
constexpr int kRows = 128;    // GEMM rows per block
constexpr int kMinBlocks = 512;  // below this a launch takes narrower column blocks
constexpr int kKC = 64;       // channels of one LDS halo chunk (tile policy)
constexpr int kHaloW = 18, kHaloH = 10, kHaloPx = kHaloW * kHaloH;
constexpr int kImagePx = 8;   // pixels per thread of the image block

constexpr int ilog2(int v) { return v <= 1 ? 0 : 1 + ilog2(v >> 1); }

template <class T>
__device__ __forceinline__ uint4 ldg16(const T* p) { return *reinterpret_cast<const uint4*>(p); }

// P::kLane channels c.. of pixel `pix` of the logical tensor (c % kLane == 0, c0 % 16 == 0)
template <class View>
__device__ __forceinline__ uint4 view_ld(const View& v, size_t pix, int c) {
    return c < v.c0 ? ldg16(v.src0 + pix * (size_t)v.c0 + c) : ldg16(v.src1 + pix * (size_t)v.c1 + (c - v.c0));
}

// The 8 x 16 tile of block blockIdx.x (tile policy; zeros for the rows policy).
struct Tile {
    int img, y0, x0;
};
template <bool TILE>
__device__ __forceinline__ Tile tile_of_block(int h, int w) {
    Tile tl = {0, 0, 0};
    if constexpr (TILE) {
        const int tx_n = w >> 4, ty_n = h >> 3;
        const int t = blockIdx.x;
        tl.img = t / (tx_n * ty_n);
        const int rem = t % (tx_n * ty_n);
        tl.y0 = (rem / tx_n) * 8;
        tl.x0 = (rem % tx_n) * 16;
    }
    return tl;
}

// Where GEMM row `m` of the launch lives in the image.
struct RowPos {
    bool valid;
    int img, y, x;
};
template <bool TILE>
__device__ __forceinline__ RowPos row_pos(int64_t m, int64_t M, int h, int w, bool window_order, const Tile& tl) {
    RowPos p;
    if constexpr (TILE) {
        // m = row inside the 8 x 16 tile's 128: wave = m >> 5 owns image rows 2 wave, 2 wave + 1;
        // bit 0 = column bit 0, bit 1 = row, bits 2.. = column bits 1..: a 2x2 pool window is
        // rows 4 q .. 4 q + 3, the four accumulator registers 4 g .. 4 g + 3 of one lane
        const int ml = (int)m & 31, wv = (int)m >> 5;
        p.valid = true;
        p.img = tl.img;
        p.y = tl.y0 + 2 * wv + ((ml >> 1) & 1);
        p.x = tl.x0 + (ml & 1) + 2 * (ml >> 2);
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

// Epilogue staging: a wave's 32 x (32 EG) result (and its 8 pooled rows) as stored elements in
// LDS, so the global stores are 16 bytes of contiguous channels per lane.
template <class P, int EG>
struct Stage {
    static constexpr int kLd = 32 * EG + P::kLane;            // elements per row (16 bytes of padding)
    static constexpr int kWaveElems = (32 + 8) * kLd;         // 32 rows + 8 pooled rows
    static constexpr int kBytes = 4 * kWaveElems * (int)sizeof(typename P::Elem);
};

// ------------------------------------------------------------------ separable conv ----
// epi...: the precision's per-column epilogue arrays, in the order its entry point passes them
// (their element types Epi are named at the launch: a pack in the middle of the list is not deduced).
template <class P, int NT, bool TILE, class... Epi>
__global__ __launch_bounds__(kBlock) void sep_kernel(typename P::View v, int n, int h, int w,
                                                     const float* __restrict__ dw, int cout,
                                                     const typename P::Elem* __restrict__ pw,
                                                     const Epi* __restrict__... epi,
                                                     typename P::Elem* __restrict__ out,
                                                     typename P::Elem* __restrict__ out_pool) {
    using Elem = typename P::Elem;
    constexpr int EG = NT < 4 ? NT : 4;
    using St = Stage<P, EG>;
    // tile policy: the chunk's halo, then its depthwise taps [9][kKC] fp32 (every lane of a half
    // wave reads the same bytes per tap: an LDS broadcast instead of a 1-KiB vector load)
    constexpr int kHaloBytes = TILE ? kHaloPx * P::kHaloLd * (int)sizeof(Elem) : 0;
    constexpr int kTapBytes = TILE ? 9 * kKC * 4 : 0;
    constexpr int kSmem = St::kBytes > kHaloBytes + kTapBytes ? St::kBytes : kHaloBytes + kTapBytes;
    __shared__ __attribute__((aligned(16))) unsigned char smem_raw[kSmem];
    Elem* const smem = reinterpret_cast<Elem*>(smem_raw);
    float* const taps = reinterpret_cast<float*>(smem_raw + kHaloBytes);

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, hh = lane >> 5;
    const int C = v.c0 + v.c1;
    const int nb0 = blockIdx.y * (32 * NT);
    const int64_t M = (int64_t)n * h * w;
    const bool pooled = out_pool != nullptr;

    const Tile tl = tile_of_block<TILE>(h, w);
    const int64_t m_wave = TILE ? (int64_t)wave * 32 : (int64_t)blockIdx.x * kRows + wave * 32;
    const RowPos me = row_pos<TILE>(m_wave + r, M, h, w, pooled, tl);

    typename P::Acc acc[NT];
#pragma unroll
    for (int i = 0; i < NT; ++i)
#pragma unroll
        for (int j = 0; j < 16; ++j) acc[i][j] = 0;

    for (int kc0 = 0; kc0 < C; kc0 += kKC) {
        const int kcn = (C - kc0) < kKC ? (C - kc0) : kKC;
        if constexpr (TILE) {
            __syncthreads();
            const int segs = kcn >> ilog2(P::kLane);
            for (int idx = tid; idx < kHaloPx * segs; idx += kBlock) {
                const int p = idx / segs, s = idx - p * segs;
                const int gy = tl.y0 + p / kHaloW - 1, gx = tl.x0 + p % kHaloW - 1;
                uint4 val = make_uint4(0, 0, 0, 0);  // spatial padding: the element 0
                if (gy >= 0 && gy < h && gx >= 0 && gx < w)
                    val = view_ld(v, ((size_t)tl.img * h + gy) * w + gx, kc0 + P::kLane * s);
                *reinterpret_cast<uint4*>(smem + p * P::kHaloLd + P::kLane * s) = val;
            }
            const int quads = kcn >> 2;
            for (int idx = tid; idx < 9 * quads; idx += kBlock) {
                const int t = idx / quads, q = idx - t * quads;
                st4(taps + t * kKC + 4 * q, ld4(dw + (size_t)t * C + kc0 + 4 * q));
            }
            __syncthreads();
        }
        for (int ks = 0; ks < kcn; ks += P::kStep) {
            const int cl = ks + P::kLane * hh;  // channel inside the chunk
            const int c = kc0 + cl;             // channel of the logical tensor
            // the nine taps of the lane's kLane channels in fp32, in tap order (the one order both
            // tap-fetch policies share), then rounded once to the A operand
            float a[P::kLane];
#pragma unroll
            for (int j = 0; j < P::kLane; ++j) a[j] = 0.f;
            P::with_source(v, c, [&](auto SRC) {
#pragma unroll
                for (int t = 0; t < 9; ++t) {
                    const int dy = t / 3 - 1, dx = t % 3 - 1;
                    uint4 xv;
                    const float* tp;
                    if constexpr (TILE) {
                        const int ly = me.y - tl.y0 + 1 + dy, lx = me.x - tl.x0 + 1 + dx;
                        xv = *reinterpret_cast<const uint4*>(smem + (ly * kHaloW + lx) * P::kHaloLd + cl);
                        tp = taps + t * kKC + cl;
                    } else {
                        tp = dw + (size_t)t * C + c;
                        const int yy = me.y + dy, xx = me.x + dx;
                        xv = make_uint4(0, 0, 0, 0);
                        if (me.valid && yy >= 0 && yy < h && xx >= 0 && xx < w)
                            xv = view_ld(v, ((size_t)me.img * h + yy) * w + xx, c);
                    }
                    P::tap_fma(SRC, a, xv, tp);
                }
            });
            const typename P::Frag af = P::round_a(a);
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const auto bf = __builtin_bit_cast(typename P::Frag, ldg16(pw + (size_t)(nb0 + nt * 32 + r) * C + c));
                acc[nt] = P::mfma(af, bf, acc[nt]);
            }
        }
    }

    // epilogue: P::sep_out per element, staged through LDS in groups of EG column tiles
    Elem* const st = smem + wave * St::kWaveElems;
    Elem* const stp = st + 32 * St::kLd;
#pragma unroll
    for (int g0 = 0; g0 < NT; g0 += EG) {
        __syncthreads();
#pragma unroll
        for (int e = 0; e < EG; ++e) {
            const int col = e * 32 + r;
            const auto cp = P::sep_col(nb0 + (g0 + e) * 32 + r, epi...);
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                typename P::Out mx = 0;  // every stored element is >= 0 (ReLU)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int reg = 4 * g + i;
                    const int row = (reg & 3) + 8 * (reg >> 2) + 4 * hh;
                    const typename P::Out o = P::sep_out(acc[g0 + e][reg], cp);
                    st[row * St::kLd + col] = (Elem)o;
                    mx = o > mx ? o : mx;
                }
                stp[(hh + 2 * g) * St::kLd + col] = (Elem)mx;
            }
        }
        __syncthreads();
        constexpr int kChunks = EG * 32 / P::kLane;  // 16-B chunks per row
        for (int idx = lane; idx < 32 * kChunks; idx += 64) {
            const int row = idx / kChunks, ch = idx - row * kChunks;
            const RowPos p = row_pos<TILE>(m_wave + row, M, h, w, pooled, tl);
            if (p.valid) {
                const size_t pix = ((size_t)p.img * h + p.y) * w + p.x;
                *reinterpret_cast<uint4*>(out + pix * cout + nb0 + g0 * 32 + ch * P::kLane) =
                    *reinterpret_cast<const uint4*>(st + row * St::kLd + ch * P::kLane);
            }
        }
        if (pooled) {
            for (int idx = lane; idx < 8 * kChunks; idx += 64) {
                const int q = idx / kChunks, ch = idx - q * kChunks;
                // the window's first row tells where it is
                const RowPos p = row_pos<TILE>(m_wave + 4 * q, M, h, w, true, tl);
                if (p.valid) {
                    const size_t pix = ((size_t)p.img * (h >> 1) + (p.y >> 1)) * (w >> 1) + (p.x >> 1);
                    *reinterpret_cast<uint4*>(out_pool + pix * cout + nb0 + g0 * 32 + ch * P::kLane) =
                        *reinterpret_cast<const uint4*>(stp + q * St::kLd + ch * P::kLane);
                }
            }
        }
    }
}

// --------------------------------------------------------------- transposed conv ----
// GEMM rows = input pixels, K = cin, columns = (a, b, co) of the Keras (2, 2, cout, cin) kernel,
// which is already [column][k] with k contiguous.  No activation.
template <class P, int NT, class... Epi>
__global__ __launch_bounds__(kBlock) void convt_kernel(const typename P::Elem* __restrict__ x, int n, int h, int w,
                                                       int cin, int cout, const typename P::Elem* __restrict__ kern,
                                                       const Epi* __restrict__... epi,
                                                       typename P::Elem* __restrict__ out) {
    using Elem = typename P::Elem;
    using St = Stage<P, NT>;
    __shared__ __attribute__((aligned(16))) unsigned char smem_raw[St::kBytes];
    Elem* const smem = reinterpret_cast<Elem*>(smem_raw);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, hh = lane >> 5;
    const int nb0 = blockIdx.y * (32 * NT);
    const int64_t M = (int64_t)n * h * w;
    const int64_t m_wave = (int64_t)blockIdx.x * kRows + wave * 32;
    const int64_t m = m_wave + r;
    const bool valid = m < M;

    typename P::Acc acc[NT];
#pragma unroll
    for (int i = 0; i < NT; ++i)
#pragma unroll
        for (int j = 0; j < 16; ++j) acc[i][j] = 0;

    for (int k0 = 0; k0 < cin; k0 += P::kStep) {
        const int c = k0 + P::kLane * hh;
        uint4 av = make_uint4(0, 0, 0, 0);
        if (valid) av = ldg16(x + (size_t)m * cin + c);
        const typename P::Frag af = P::convt_a(av);
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const auto bf = __builtin_bit_cast(typename P::Frag, ldg16(kern + (size_t)(nb0 + nt * 32 + r) * cin + c));
            acc[nt] = P::mfma(af, bf, acc[nt]);
        }
    }

    Elem* const st = smem + wave * St::kWaveElems;
#pragma unroll
    for (int e = 0; e < NT; ++e) {
        const int col = e * 32 + r;
        const auto cp = P::convt_col(nb0 + col, cout, epi...);
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const int row = (reg & 3) + 8 * (reg >> 2) + 4 * hh;
            st[row * St::kLd + col] = P::convt_out(acc[e][reg], cp);
        }
    }
    __syncthreads();
    // a lane keeps its 16-byte column chunk and walks the rows: the (a, b, co) split of the column
    // is computed once, the row's (img, y, x) in 32-bit arithmetic (the entry point bounds M)
    constexpr int kChunks = NT * 32 / P::kLane, kRowStep = 64 / kChunks;
    const int ch = lane % kChunks;
    const int col = nb0 + ch * P::kLane;
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
                *reinterpret_cast<const uint4*>(st + row * St::kLd + ch * P::kLane);
        }
    }
}

// ------------------------------------------------------------------- image block ----
// One thread: 8 output channels of up to kImagePx pixels of ONE image row (blockIdx.x = the row,
// so (img, y) cost the block one scalar division).  All fp32 up to relu(z); Out rounds and stores
// the 8 results (par...: what P::image_put needs besides, named at the launch).  The folded weights of the thread's channel group stay in registers over its
// pixels where the block size is a multiple of the group count (cout = 64: 8 groups).
template <class P, class... Par>
__global__ __launch_bounds__(kBlock) void image_kernel(const float* __restrict__ x, int n, int h, int w, int cin,
                                                       const float* __restrict__ dw, int cout,
                                                       const float* __restrict__ pw, const float* __restrict__ bias,
                                                       Par... par, typename P::Elem* __restrict__ out) {
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
        typename P::Image8 res;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            float o = 0.f;
#pragma unroll
            for (int ci = 0; ci < 4; ++ci) o = fmaf(yv[ci], pk[ci][j], o);  // channels past cin: 0 * 0
            P::image_put(res, j, relu(o + bb[j]), par...);
        }
        P::image_store(res, out + (row0 + xx) * cout + co);
    }
}

// -------------------------------------------------------------------------- head ----
// Eight lanes per pixel: lane `sub` reads the 8-channel chunks sub, sub + 8, ... of the pixel
// (P::head_ld8), the partial logits meet in three shuffles.
template <class P>
__device__ __forceinline__ float head_logit(const typename P::Elem* __restrict__ px, int cin, int sub,
                                            const float* __restrict__ kern, int ncls, int c, float b) {
    float l = 0.f;
    for (int k = 8 * sub; k < cin; k += 64) {
        const auto xv = P::head_ld8(px + k);
#pragma unroll
        for (int j = 0; j < 8; ++j) l = fmaf(P::head_x(xv, j), kern[(size_t)(k + j) * ncls + c], l);
    }
    l += __shfl_xor(l, 1, 64);
    l += __shfl_xor(l, 2, 64);
    l += __shfl_xor(l, 4, 64);
    return l + b;
}

template <class P>
__global__ __launch_bounds__(kBlock) void head_kernel(const typename P::Elem* __restrict__ x, int64_t M, int cin,
                                                      int ncls, const float* __restrict__ kern,
                                                      const float* __restrict__ bias, float* __restrict__ prob) {
    const int64_t m = ((int64_t)blockIdx.x * kBlock + threadIdx.x) >> 3;
    const int sub = threadIdx.x & 7;
    const bool valid = m < M;  // lanes past the end keep running for the shuffles, on pixel 0
    const typename P::Elem* px = x + (size_t)(valid ? m : 0) * cin;
    if (ncls == 1) {
        const float l = head_logit<P>(px, cin, sub, kern, 1, 0, bias[0]);
        if (valid && sub == 0) prob[m] = 1.f / (1.f + expf(-l));
        return;
    }
    float mx = -INFINITY, s = 0.f;  // online softmax: max and sum in one pass over the classes
    for (int c = 0; c < ncls; ++c) {
        const float l = head_logit<P>(px, cin, sub, kern, ncls, c, bias[c]);
        const float mn = fmaxf(mx, l);
        s = s * expf(mx - mn) + expf(l - mn);
        mx = mn;
    }
    const float inv = 1.f / s;
    for (int c = 0; c < ncls; ++c) {
        const float l = head_logit<P>(px, cin, sub, kern, ncls, c, bias[c]);
        if (valid && sub == (c & 7)) prob[(size_t)m * ncls + c] = expf(l - mx) * inv;
    }
}

// --------------------------------------------------------------------- host side ----
inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// Column tiles (of 32) per block of a sepconv launch with gx row blocks: 128 columns where that
// divides cout (the depthwise output is recomputed per column block), narrower while the grid
// would leave the 256 CUs fewer than two blocks each.  (A 256-column block needs 128 accumulator
// registers: one wave per SIMD, nothing hides a load.)
inline int sep_col_tiles(int cout, int64_t gx) {
    int nt = cout % 128 == 0 ? 4 : cout % 64 == 0 ? 2 : 1;
    while (nt > 1 && gx * (cout / (32 * nt)) < kMinBlocks) nt >>= 1;
    return nt;
}

// The argument checks every sepconv entry point shares (`who` names it in the messages), then the
// launch geometry.  The view and alignment checks stay with the precision.
struct SepPlan {
    bool tile;
    int nt;
    dim3 grid;
};
inline int sep_plan(const char* who, bool pointers, int n, int h, int w, int cout, const void* out_pool, int route,
                    SepPlan* plan) {
    UNET_CHECK_ARG(pointers, "%s: null pointer", who);
    UNET_CHECK_ARG(n > 0 && h > 0 && w > 0, "%s: empty tensor (%d, %d, %d)", who, n, h, w);
    UNET_CHECK_ARG(cout > 0 && cout % 32 == 0, "%s: cout %d not a positive multiple of 32", who, cout);
    UNET_CHECK_ARG(route >= 0 && route <= 2, "%s: bad route %d", who, route);
    UNET_CHECK_ARG(!out_pool || (h % 2 == 0 && w % 2 == 0), "%s: out_pool needs even h, w (%d, %d)", who, h, w);
    const bool can_tile = h % 8 == 0 && w % 16 == 0;
    UNET_CHECK_ARG(route != 2 || can_tile, "%s: route 2 (tile) needs h %% 8 == 0 and w %% 16 == 0", who);
    plan->tile = route == 2 || (route == 0 && can_tile);
    const int64_t M = (int64_t)n * h * w;
    const int64_t gx = plan->tile ? M / kRows : cdiv(M, kRows);
    UNET_CHECK_ARG(gx < (1ll << 31), "%s: tensor too large", who);
    plan->nt = sep_col_tiles(cout, gx);
    plan->grid = dim3((unsigned)gx, (unsigned)(cout / (32 * plan->nt)));
    return 0;
}

}  // namespace frozen
}  // namespace unet
