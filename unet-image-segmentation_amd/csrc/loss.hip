// Dice / IoU sums with their finalize, and the MeanIoU confusion counts.
#include "head.h"

namespace unet {
namespace {

// part[n][blk][3][ncls] = {sum t*p, sum t, sum p} over this block's pixels of image n
template <int NC>
__global__ __launch_bounds__(256) void dice_partial_kernel(const float* __restrict__ yt, const float* __restrict__ yp,
                                                           int64_t hw, int ncls, int64_t ppb,
                                                           float* __restrict__ part) {
    const int n = blockIdx.y, blk = blockIdx.x, nblk = gridDim.x;
    float I[NC], T[NC], P[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) I[c] = T[c] = P[c] = 0.f;
    const int64_t p0 = (int64_t)blk * ppb;
    const int64_t p1 = p0 + ppb < hw ? p0 + ppb : hw;
    for (int64_t p = p0 + threadIdx.x; p < p1; p += 256) {
        const int64_t base = ((int64_t)n * hw + p) * ncls;
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            if (c < ncls) {
                const float t = yt[base + c], q = yp[base + c];
                I[c] = fmaf(t, q, I[c]);
                T[c] += t;
                P[c] += q;
            }
        }
    }
    __shared__ float red[4][3 * NC];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        const float a = wave_sum(I[c]), b = wave_sum(T[c]), d = wave_sum(P[c]);
        if (lane == 0) {
            red[wave][c] = a;
            red[wave][NC + c] = b;
            red[wave][2 * NC + c] = d;
        }
    }
    __syncthreads();
    if (threadIdx.x < 3 * NC) {
        const int j = threadIdx.x / NC, c = threadIdx.x % NC;
        if (c < ncls) {
            const float s = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
            part[(((int64_t)n * nblk + blk) * 3 + j) * ncls + c] = s;
        }
    }
}

// Multi-class form: the block's pixel rows (ncls contiguous floats each) staged a 256-pixel tile
// at a time through LDS with coalesced loads, then lane (class c, 32-row group g) sums its column
// slice; the 8 groups are combined in a fixed order at the end.  (The one-lane-per-pixel form
// read 21-float rows lane-strided: 77 us for the batch-8 21-class sums, profiles/r4j_cfg4_trace.txt.)
template <int NC>
__global__ __launch_bounds__(256) void dice_partial_m_kernel(const float* __restrict__ yt, const float* __restrict__ yp,
                                                             int64_t hw, int ncls, int64_t ppb, float* __restrict__ part) {
    __shared__ float Ys[256 * NC], Qs[256 * NC];
    const int n = blockIdx.y, blk = blockIdx.x, nblk = gridDim.x;
    const int c = threadIdx.x % NC, g = threadIdx.x / NC;
    float I = 0.f, T = 0.f, P = 0.f;
    const int64_t p0 = (int64_t)blk * ppb;
    const int64_t p1 = p0 + ppb < hw ? p0 + ppb : hw;
    for (int64_t t0 = p0; t0 < p1; t0 += 256) {
        const int np = p1 - t0 < 256 ? (int)(p1 - t0) : 256;
        const int cnt = np * ncls;
        const int64_t f0 = ((int64_t)n * hw + t0) * ncls;
        __syncthreads();
        for (int i = threadIdx.x; i < cnt; i += 256) {
            Ys[i] = yt[f0 + i];
            Qs[i] = yp[f0 + i];
        }
        __syncthreads();
        if (g < 8 && c < ncls) {
            const int r1 = (g + 1) * 32 < np ? (g + 1) * 32 : np;
            for (int r = g * 32; r < r1; ++r) {
                const float y = Ys[r * ncls + c], q = Qs[r * ncls + c];
                I = fmaf(y, q, I);
                T += y;
                P += q;
            }
        }
    }
    __syncthreads();
    if (g < 8) {
        Ys[g * NC + c] = I;
        Ys[8 * NC + g * NC + c] = T;
        Ys[16 * NC + g * NC + c] = P;
    }
    __syncthreads();
    if (threadIdx.x < 3 * NC) {
        const int j = threadIdx.x / NC, cc = threadIdx.x % NC;
        if (cc < ncls) {
            float sacc = 0.f;
            for (int q = 0; q < 8; ++q) sacc += Ys[j * 8 * NC + q * NC + cc];
            part[(((int64_t)n * nblk + blk) * 3 + j) * ncls + cc] = sacc;
        }
    }
}

// Per (image, class) term: the block partials summed in double by a group of lanes and an
// xor-shuffle tree (fixed lane order); the dice / iou terms then summed by one wave in a fixed
// order -- deterministic, and no thread walks all nblk partials or all terms serially.
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__global__ __launch_bounds__(1024) void dice_finalize_kernel(const float* part, int N, int nblk, int ncls,
                                                            float smooth, float* __restrict__ sums,
                                                            float* __restrict__ result) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    constexpr int kMaxTerms = 1024;  // terms kept in LDS for the ordered sum (N * ncls beyond: second pass)
    __shared__ float td[kMaxTerms], ti[kMaxTerms];
    __shared__ double acc[2];
    // all partials staged in LDS with coalesced loads when they fit: the per-term walks
    // then wait on LDS, not on a dependent global load a term
    constexpr int kStage = 34816;  // 136 KB
    __shared__ float pst[kStage];
    const int64_t total = (int64_t)N * nblk * 3 * ncls;
    if (total <= kStage) {
        // 8 independent loads in flight per thread (a load-store pair per iteration exposed the
        // load latency ~32 times: 31 us for 8 x 21-class partials)
        const int bd = blockDim.x;
        for (int i0 = threadIdx.x; i0 < (int)total; i0 += 8 * bd) {
            float t[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) t[u] = i0 + u * bd < (int)total ? part[i0 + u * bd] : 0.f;
#pragma unroll
            for (int u = 0; u < 8; ++u)
                if (i0 + u * bd < (int)total) pst[i0 + u * bd] = t[u];
        }
        __syncthreads();
        part = pst;
    }
    if (threadIdx.x == 0) acc[0] = acc[1] = 0.0;
    // 8 lanes a term (lane g sums partials g, g + 8, ... in double, then an xor tree within the
    // group): 128 terms at a time instead of one a wave; the terms' dice / iou values are then
    // summed by one wave (lane t: terms t, t + 64, ..., then its xor tree) -- fixed orders both
    constexpr int G = 8;
    const int grp = threadIdx.x / G, gl = threadIdx.x % G, ngrp = (int)(blockDim.x / G);
    for (int base = 0; base < N * ncls; base += kMaxTerms) {
        const int nt = N * ncls - base < kMaxTerms ? N * ncls - base : kMaxTerms;
        for (int k0 = 0; k0 < nt; k0 += ngrp) {  // (uniform trip count: the shuffles see every lane)
            const int k = k0 + grp;
            const int idx = base + (k < nt ? k : 0), n = idx / ncls, c = idx % ncls;
            double I = 0.0, T = 0.0, P = 0.0;
            if (k < nt)
                for (int b = gl; b < nblk; b += G) {
                    const int64_t o = (((int64_t)n * nblk + b) * 3) * ncls + c;
                    I += part[o];
                    T += part[o + ncls];
                    P += part[o + 2 * ncls];
                }
#pragma unroll
            for (int o = G / 2; o > 0; o >>= 1) {
                I += __shfl_xor(I, o, 64);
                T += __shfl_xor(T, o, 64);
                P += __shfl_xor(P, o, 64);
            }
            if (gl == 0 && k < nt) {
                const float fi = (float)I, ft = (float)T, fp = (float)P;
                if (sums) {
                    sums[idx * 3 + 0] = fi;
                    sums[idx * 3 + 1] = ft;
                    sums[idx * 3 + 2] = fp;
                }
                td[k] = (2.0f * fi + smooth) / (ft + fp + smooth);
                ti[k] = (fi + smooth) / (ft + fp - fi + smooth);
            }
        }
        __syncthreads();
        if (wave == 0) {
            double d = 0.0, i = 0.0;
            for (int k = lane; k < nt; k += 64) {
                d += (double)td[k];
                i += (double)ti[k];
            }
            d = wave_sum_d(d);
            i = wave_sum_d(i);
            if (lane == 0) {
                acc[0] += d;
                acc[1] += i;
            }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double cnt = (double)N * ncls;
        const float dice = (float)(acc[0] / cnt);
        result[0] = 1.0f - dice;
        result[1] = dice;
        result[2] = (float)(acc[1] / cnt);
    }
}

template <int K>
__device__ __forceinline__ void miou_count(float tv, float q, float thr, unsigned int* h) {
    const long long t = (long long)tv;  // Keras casts to int64 (truncation), then range-checks
    const long long p = thr < 0.f ? (long long)q : (q > thr ? 1 : 0);
    if (t >= 0 && t < K && p >= 0 && p < K) {
        const int b = (int)(t * K + p);
#pragma unroll
        for (int i = 0; i < K * K; ++i) h[i] += b == i ? 1u : 0u;
    }
}
// K x K confusion counts, float4 loads (four elements a lane per load pair; the count % 4 tail by
// the first threads)
template <int K>
__global__ __launch_bounds__(256) void meaniou_small_kernel(const float* __restrict__ yt, const float* __restrict__ yp,
                                                            int64_t count, float thr,
                                                            unsigned long long* __restrict__ conf) {
    unsigned int h[K * K];
#pragma unroll
    for (int i = 0; i < K * K; ++i) h[i] = 0;
    const int64_t n4 = count / 4;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        const float4 t = ld4(yt + 4 * i), q = ld4(yp + 4 * i);
        miou_count<K>(t.x, q.x, thr, h);
        miou_count<K>(t.y, q.y, thr, h);
        miou_count<K>(t.z, q.z, thr, h);
        miou_count<K>(t.w, q.w, thr, h);
    }
    if (blockIdx.x == 0 && threadIdx.x < count - 4 * n4) {
        const int64_t i = 4 * n4 + threadIdx.x;
        miou_count<K>(yt[i], yp[i], thr, h);
    }
    __shared__ unsigned int red[4][K * K];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int b = 0; b < K * K; ++b) {
        unsigned int v = h[b];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        if (lane == 0) red[wave][b] = v;
    }
    __syncthreads();
    if (threadIdx.x < K * K) {
        const unsigned int s = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
        if (s) atomicAdd(conf + threadIdx.x, (unsigned long long)s);
    }
}

__global__ __launch_bounds__(256) void meaniou_kernel(const float* __restrict__ yt, const float* __restrict__ yp,
                                                      int64_t count, int K, float thr,
                                                      unsigned long long* __restrict__ conf) {
    __shared__ unsigned int hist[kMaxCls * kMaxCls];
    for (int b = threadIdx.x; b < K * K; b += 256) hist[b] = 0;
    __syncthreads();
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (int64_t)gridDim.x * 256) {
        const long long t = (long long)yt[i];
        const float q = yp[i];
        const long long p = thr < 0.f ? (long long)q : (q > thr ? 1 : 0);
        if (t >= 0 && t < K && p >= 0 && p < K) atomicAdd(&hist[t * K + p], 1u);
    }
    __syncthreads();
    for (int b = threadIdx.x; b < K * K; b += 256)
        if (hist[b]) atomicAdd(conf + b, (unsigned long long)hist[b]);
}

}  // namespace
}  // namespace unet

using namespace unet;

extern "C" size_t unet_dice_workspace(int n, int64_t hw, int ncls) {
    if (n <= 0 || hw <= 0 || ncls <= 0) return 0;
    DicePlan d = dice_plan(n, hw);
    return align_up((size_t)n * d.nblk * 3 * ncls * sizeof(float), 256);
}

extern "C" int unet_dice_fwd(const float* y_true, const float* y_pred, int n, int64_t hw, int ncls, float smooth,
                             float* sums, float* result, void* ws, size_t ws_bytes, unet_stream_t stream) {
    UNET_CHECK_ARG(y_true && y_pred && result && n > 0 && hw > 0, "unet_dice_fwd: bad args");
    UNET_CHECK_ARG(ncls >= 1 && ncls <= kMaxCls, "unet_dice_fwd: num_classes %d out of [1,%d]", ncls, kMaxCls);
    const size_t need = unet_dice_workspace(n, hw, ncls);
    UNET_CHECK_ARG(ws && ws_bytes >= need, "unet_dice_fwd: workspace %zu < %zu", ws_bytes, need);
    DicePlan d = dice_plan(n, hw);
    hipStream_t st = as_stream(stream);
    float* part = static_cast<float*>(ws);
    dim3 grid(d.nblk, n);
    if (ncls == 1)
        dice_partial_kernel<1><<<grid, 256, 0, st>>>(y_true, y_pred, hw, ncls, d.ppb, part);
    else
        with_bucket<4, 8, 16, 24, 32>(ncls, [&](auto NC) {
            dice_partial_m_kernel<NC()><<<grid, 256, 0, st>>>(y_true, y_pred, hw, ncls, d.ppb, part);
        });
    UNET_CHECK_LAUNCH("unet_dice_fwd(partial)");
    dice_finalize_kernel<<<1, n * ncls >= 64 ? 1024 : 256, 0, st>>>(part, n, d.nblk, ncls, smooth, sums, result);
    UNET_CHECK_LAUNCH("unet_dice_fwd(finalize)");
    return 0;
}

extern "C" int unet_meaniou_update(const float* y_true, const float* y_pred, int64_t count, int num_classes,
                                   float threshold, uint64_t* confusion, unet_stream_t stream) {
    UNET_CHECK_ARG(y_true && y_pred && confusion && count >= 0, "unet_meaniou_update: bad args");
    UNET_CHECK_ARG(num_classes >= 1 && num_classes <= kMaxCls, "unet_meaniou_update: num_classes out of [1,%d]",
                   kMaxCls);
    if (count == 0) return 0;
    hipStream_t st = as_stream(stream);
    auto* conf = reinterpret_cast<unsigned long long*>(confusion);
    if (num_classes == 2 && ((uintptr_t)y_true | (uintptr_t)y_pred) % 16 == 0)
        meaniou_small_kernel<2><<<tile_grid(cdiv(count, 4), 256, 2048), 256, 0, st>>>(y_true, y_pred, count, threshold,
                                                                                      conf);
    else
        meaniou_kernel<<<tile_grid(count, 256, 2048), 256, 0, st>>>(y_true, y_pred, count, num_classes, threshold, conf);
    UNET_CHECK_LAUNCH("unet_meaniou_update");
    return 0;
}
