// Head forward: the four kernel families and unet_head_fwd (route policy: head_plan.h).
#include "head.h"

namespace unet {
namespace {

// Binary head, Cin = 4G (G lanes per pixel, one channel quad each): every lane issues U
// independent float4 loads (U pixels, each wave's loads contiguous 1 KB runs), applies the
// BN+ReLU view, dots with its kernel quad held in registers, and the G lanes of a pixel reduce
// with xor shuffles.  No LDS, no barriers: the loads of a wave stay in flight together.
template <int MODE, int G>
__global__ __launch_bounds__(256) void head_fwd_bin_kernel(DView v, int64_t M, const float* __restrict__ W,
                                                           const float* __restrict__ bias, float* __restrict__ prob) {
    constexpr int PPW = 64 / G;  // pixels per wave per slot
    constexpr int U = 4;
    constexpr int PB = 4 * U * PPW;  // pixels per block iteration
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int q = lane % G, ps = lane / G;
    const int c = 4 * q;
    const float4 wk = ld4(W + c);  // Keras (1, 1, Cin, 1): W[c]
    float4 sc = f4(1.f), sh = f4(0.f);
    if constexpr (MODE == UNET_VIEW_BNRELU) {
        sc = ld4(v.sc0 + c);
        sh = ld4(v.sh0 + c);
    }
    const float b = bias ? bias[0] : 0.f;
    for (int64_t base = (int64_t)blockIdx.x * PB; base < M; base += (int64_t)gridDim.x * PB) {
        const int64_t p0 = base + wave * U * PPW + ps;
        float4 x[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t m = p0 + u * PPW;
            x[u] = m < M ? ld4(v.src0 + m * (4 * G) + c) : f4(0.f);
        }
        float s[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            float4 a = x[u];
            if constexpr (MODE == UNET_VIEW_BNRELU) a = bnrelu4(a, sc, sh);
            s[u] = fmaf(a.x, wk.x, fmaf(a.y, wk.y, fmaf(a.z, wk.z, a.w * wk.w)));
        }
#pragma unroll
        for (int off = G / 2; off > 0; off >>= 1)
#pragma unroll
            for (int u = 0; u < U; ++u) s[u] += __shfl_xor(s[u], off, 64);
        if (q == 0) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int64_t m = p0 + u * PPW;
                if (m < M) prob[m] = 1.0f / (1.0f + expf(-(s[u] + b)));
            }
        }
    }
}

// Pixel tile of TP = 8192 / Cin (binary) or 4096 / Cin (multi-class) pixels: the tile's activations are staged through LDS with
// coalesced float4 loads (one lane per channel quad), then one lane per pixel forms the logits.
template <int MODE, int NC>
__global__ __launch_bounds__(256) void head_fwd_kernel(DView v, int64_t M, int ncls, const float* __restrict__ W,
                                                       const float* __restrict__ bias, float* __restrict__ prob,
                                                       bool al) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int Cin = v.c0, CQ = Cin / 4, LA = Cin + 1, TP = head_fwd_tp(Cin, NC != 1);
    float* Ws = smem;                // [Cin][NC]
    float* bs = Ws + kMaxCin * NC;   // [NC]
    float* A = bs + NC;              // [TP][Cin + 1]
    STAGE_KERNEL(Ws, W, Cin, NC, ncls)
    if (threadIdx.x < NC) bs[threadIdx.x] = (threadIdx.x < ncls && bias) ? bias[threadIdx.x] : 0.f;
    for (int64_t m0 = (int64_t)blockIdx.x * TP; m0 < M; m0 += (int64_t)gridDim.x * TP) {
        __syncthreads();
        for (int idx = threadIdx.x; idx < TP * CQ; idx += 256) {
            const int p = idx / CQ, kq = idx - (idx / CQ) * CQ;
            const int64_t m = m0 + p;
            float4 x = f4(0.f);
            if (m < M) x = head_row4<MODE>(v, m, 4 * kq, al);
            float* a = A + p * LA + 4 * kq;
            a[0] = x.x;
            a[1] = x.y;
            a[2] = x.z;
            a[3] = x.w;
        }
        __syncthreads();
        const int p = threadIdx.x;
        const int64_t m = m0 + p;
        if (p >= TP || m >= M) continue;
        float l[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) l[c] = bs[c];
        for (int k = 0; k < Cin; ++k) {
            const float a = A[p * LA + k];
#pragma unroll
            for (int c = 0; c < NC; ++c) l[c] = fmaf(a, Ws[k * NC + c], l[c]);
        }
        if (ncls == 1) {
            prob[m] = 1.0f / (1.0f + expf(-l[0]));
        } else {
            SOFTMAX_REGS(l, NC, ncls, inv);
#pragma unroll
            for (int c = 0; c < NC; ++c)
                if (c < ncls) prob[m * ncls + c] = l[c] * inv;
        }
    }
}

// Multi-class head forward, one pixel per thread over 256-pixel tiles (Cin <= 64): the tile's
// activations staged through LDS with coalesced float4 loads (view applied), the kernel as
// [Cin][NC] rows read 4 classes at a time (ds_read_b128, one address per wave: broadcast), logits
// in NC registers (NC = the class count rounded up to 4), softmax, probabilities out.
// (The earlier one-float-per-class LDS reads over 32 padded classes made the 21-class head
// LDS-bound: 153 us per batch-8 forward, profiles/r4j_cfg4_trace.txt.)
template <int MODE, int NC>
__global__ __launch_bounds__(256) void head_fwdm_kernel(DView v, int64_t M, int ncls, const float* __restrict__ W,
                                                        const float* __restrict__ bias, float* __restrict__ prob,
                                                        bool al) {
    constexpr int CMAX = 64, LA = CMAX + 4;
    __shared__ __attribute__((aligned(16))) float Ws[CMAX * NC];
    __shared__ __attribute__((aligned(16))) float A[256 * LA];
    const int Cin = v.c0, CQ = Cin / 4;
    STAGE_KERNEL(Ws, W, Cin, NC, ncls)
    float bl[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) bl[c] = (c < ncls && bias) ? bias[c] : 0.f;
    for (int64_t m0 = (int64_t)blockIdx.x * 256; m0 < M; m0 += (int64_t)gridDim.x * 256) {
        __syncthreads();
        for (int idx = threadIdx.x; idx < 256 * CQ; idx += 256) {
            const int p = idx / CQ, kq = idx - p * CQ;
            const int64_t m = m0 + p;
            const float4 x = m < M ? head_row4<MODE>(v, m, 4 * kq, al) : f4(0.f);
            *reinterpret_cast<float4*>(&A[p * LA + 4 * kq]) = x;
        }
        __syncthreads();
        const int64_t m = m0 + threadIdx.x;
        if (m >= M) continue;
        float l[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) l[c] = bl[c];
        for (int k4 = 0; k4 < CQ; ++k4) {
            const float4 a4 = *reinterpret_cast<const float4*>(&A[threadIdx.x * LA + 4 * k4]);
            const float av[4] = {a4.x, a4.y, a4.z, a4.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float* wr = &Ws[(4 * k4 + j) * NC];
#pragma unroll
                for (int c4 = 0; c4 < NC / 4; ++c4) {
                    const float4 w4 = *reinterpret_cast<const float4*>(wr + 4 * c4);
                    l[4 * c4 + 0] = fmaf(av[j], w4.x, l[4 * c4 + 0]);
                    l[4 * c4 + 1] = fmaf(av[j], w4.y, l[4 * c4 + 1]);
                    l[4 * c4 + 2] = fmaf(av[j], w4.z, l[4 * c4 + 2]);
                    l[4 * c4 + 3] = fmaf(av[j], w4.w, l[4 * c4 + 3]);
                }
            }
        }
        SOFTMAX_REGS(l, NC, ncls, inv);
#pragma unroll
        for (int c = 0; c < NC; ++c)
            if (c < ncls) prob[m * ncls + c] = l[c] * inv;
    }
}

// Multi-class head forward on the matrix cores (Cin = 8 KC <= 64, ncls <= 32): one wave per
// 32-pixel subtile, logits^T (32 classes x 32 pixels) = W^T x^T by v_mfma_f32_32x32x2_f32 with
// the kernel as the register-resident A operand and each lane's pixel row as B (lane (lo, hi)
// loads channels 8t + 4hi .. + 3 of pixel lo as float4, t < KC: k step 4t + i is channel
// 8t + 4hi + i on either operand), the bias as the accumulator's start.  Lane (lo, hi) then holds
// 16 of pixel lo's logits (classes acc_row(r, hi)); the softmax combines the two halves with one
// lane swap, and the wave's 32 x ncls probabilities leave through LDS as contiguous float4 runs.
// The next subtile's rows are loaded before this one's products (software prefetch).
// row of accumulator register r of a v_mfma_f32_32x32x2_f32 tile in lane half hi
__device__ __forceinline__ int hx_row(int r, int hi) { return (r & 3) + 8 * (r >> 2) + 4 * hi; }
template <int MODE, int KC>
__global__ __launch_bounds__(256) void head_fwdx_kernel(DView v, int64_t M, int ncls, const float* __restrict__ W,
                                                        const float* __restrict__ bias, float* __restrict__ prob,
                                                        bool vec) {
    __shared__ __attribute__((aligned(16))) float scs[8 * KC], shs[8 * KC];
    __shared__ __attribute__((aligned(16))) float ob[4][32 * 32];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lo = lane & 31, hi = lane >> 5;
    constexpr int CIN = 8 * KC;
    if constexpr (MODE == UNET_VIEW_BNRELU) {
        for (int i = threadIdx.x; i < CIN; i += 256) {
            scs[i] = v.sc0[i];
            shs[i] = v.sh0[i];
        }
    }
    float wa[4 * KC];
#pragma unroll
    for (int t = 0; t < KC; ++t)
#pragma unroll
        for (int i = 0; i < 4; ++i) wa[4 * t + i] = lo < ncls ? W[(8 * t + 4 * hi + i) * ncls + lo] : 0.f;
    float bl[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int c = hx_row(r, hi);
        bl[r] = (c < ncls && bias) ? bias[c] : 0.f;
    }
    __syncthreads();
    float* o = ob[wave];
    const int64_t nsub = (M + 31) / 32, step = (int64_t)gridDim.x * 4;
    int64_t sub = (int64_t)blockIdx.x * 4 + wave;
    float4 xn[KC];
    auto load = [&](int64_t sb) {
        const int64_t px = sb * 32 + lo;
#pragma unroll
        for (int t = 0; t < KC; ++t) xn[t] = (sb < nsub && px < M) ? ld4(v.src0 + px * CIN + 8 * t + 4 * hi) : f4(0.f);
    };
    load(sub);
    for (; sub < nsub; sub += step) {
        float4 x[KC];
#pragma unroll
        for (int t = 0; t < KC; ++t) x[t] = xn[t];
        load(sub + step);
        if constexpr (MODE == UNET_VIEW_BNRELU) {
#pragma unroll
            for (int t = 0; t < KC; ++t)
                x[t] = bnrelu4(x[t], *reinterpret_cast<const float4*>(&scs[8 * t + 4 * hi]),
                               *reinterpret_cast<const float4*>(&shs[8 * t + 4 * hi]));
        }
        floatx16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = bl[r];
#pragma unroll
        for (int t = 0; t < KC; ++t) {
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wa[4 * t + 0], x[t].x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wa[4 * t + 1], x[t].y, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wa[4 * t + 2], x[t].z, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wa[4 * t + 3], x[t].w, acc, 0, 0, 0);
        }
        float mx = -INFINITY;
#pragma unroll
        for (int r = 0; r < 16; ++r)
            if (hx_row(r, hi) < ncls) mx = fmaxf(mx, acc[r]);
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        float e[16], sum = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            e[r] = hx_row(r, hi) < ncls ? expf(acc[r] - mx) : 0.f;
            sum += e[r];
        }
        sum += __shfl_xor(sum, 32, 64);
        const float inv = 1.0f / sum;
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int r = 0; r < 16; ++r)
            if (hx_row(r, hi) < ncls) o[lo * ncls + hx_row(r, hi)] = e[r] * inv;
        __builtin_amdgcn_wave_barrier();
        const int64_t p0 = sub * 32;
        const int cnt = (int)((M - p0 < 32 ? M - p0 : 32) * ncls);
        float* dst = prob + p0 * ncls;
        const int c4n = vec ? cnt >> 2 : 0;
        for (int i = lane; i < c4n; i += 64) st4(dst + 4 * i, *reinterpret_cast<const float4*>(&o[4 * i]));
        for (int i = 4 * c4n + lane; i < cnt; i += 64) dst[i] = o[i];
        __builtin_amdgcn_wave_barrier();
    }
}

}  // namespace
}  // namespace unet

using namespace unet;

extern "C" int unet_head_fwd(const unet_view* x, int n, int h, int w, int ncls, const float* kernel,
                             const float* bias, float* prob, unet_stream_t stream) {
    if (check_view(x, "unet_head_fwd", true)) return -1;
    UNET_CHECK_ARG(x->mode == UNET_VIEW_PLAIN || x->mode == UNET_VIEW_BNRELU,
                   "unet_head_fwd: input view must be PLAIN or BNRELU");
    UNET_CHECK_ARG(x->drop_rate == 0.f, "unet_head_fwd: dropout on the head input is not supported");
    UNET_CHECK_ARG(x->c0 <= kMaxCin, "unet_head_fwd: Cin %d > %d", x->c0, kMaxCin);
    UNET_CHECK_ARG(ncls >= 1 && ncls <= kMaxCls, "unet_head_fwd: num_classes %d out of [1,%d]", ncls, kMaxCls);
    UNET_CHECK_ARG(kernel && prob && n > 0 && h > 0 && w > 0, "unet_head_fwd: bad args");
    const DView v = make_dview(*x);
    const int64_t M = (int64_t)n * h * w;
    hipStream_t st = as_stream(stream);
    const bool src_al = (uintptr_t)x->src0 % 16 == 0;  // else the general kernels read src0 by elements
    const HeadFwdPlan p = head_fwd_plan(x->c0, ncls, M, src_al, (uintptr_t)kernel % 16 == 0);
    with_int<UNET_VIEW_BNRELU, UNET_VIEW_PLAIN>(x->mode, [&](auto MODE) {
        switch (p.route) {
            case HEAD_FWD_BIN:
                with_int<8, 16, 32, 64>(x->c0 / 4, [&](auto GQ) {
                    head_fwd_bin_kernel<MODE(), GQ()><<<p.grid, 256, 0, st>>>(v, M, kernel, bias, prob);
                });
                break;
            case HEAD_FWD_MFMA:  // multi-class on the matrix cores
                with_int<16, 32, 64>(x->c0, [&](auto CIN) {
                    head_fwdx_kernel<MODE(), CIN() / 8><<<p.grid, 256, 0, st>>>(v, M, ncls, kernel, bias, prob,
                                                                                (uintptr_t)prob % 16 == 0);
                });
                break;
            case HEAD_FWD_REG:  // multi-class: the register-logit kernel
                with_bucket<4, 8, 16, 24, 32>(ncls, [&](auto NC) {
                    head_fwdm_kernel<MODE(), NC()><<<p.grid, 256, 0, st>>>(v, M, ncls, kernel, bias, prob, src_al);
                });
                break;
            default:
                with_bool(ncls > 1, [&](auto MULTI) {
                    head_fwd_kernel<MODE(), MULTI() ? kMaxCls : 1><<<p.grid, 256, p.lds, st>>>(v, M, ncls, kernel, bias,
                                                                                               prob, src_al);
                });
        }
    });
    UNET_CHECK_LAUNCH("unet_head_fwd");
    return 0;
}
