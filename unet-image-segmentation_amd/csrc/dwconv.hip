// Depthwise 3x3 half of SeparableConv2D (reference: model/u_net.py:14-20; Keras
// SeparableConv2D = tf.nn.separable_conv2d, depthwise stage = DepthwiseConv2dNative,
// stride 1, 'same' zero padding, depth_multiplier 1, kernel (3,3,C,1)).
//
// HBM-bound (18 flop per output element): each lane owns one (pixel, 4-channel)
// quad (one channel where a source of the view is not a whole number of quads); consecutive lanes walk consecutive channel quads of one pixel, so every
// wave reads/writes contiguous NHWC rows (coalesced 16-B accesses).  The 3x3 halo
// re-reads hit L1/L2.  The input is read through an activation view (BN+ReLU,
// max-pool, concat, dropout fused on load).
#include "dwtile.h"

namespace unet {

namespace {

using dw::kThreads;

// 32-bit index math (the launchers check that every tensor has < 2^31 elements)
__device__ __forceinline__ void decompose(int p, int H, int W, int& n, int& h, int& w) {
    w = p % W;
    const int t = p / W;
    h = t % H;
    n = t / H;
}

// One body per flat kernel over a lane: a channel quad (float4, VEC) or one channel (float).  The lane of channel
// index cq covers channels [cq * LW, cq * LW + LW).
template <bool VEC>
using lane_t = std::conditional_t<VEC, float4, float>;
template <bool VEC>
constexpr int LW = VEC ? 4 : 1;
template <bool VEC>
__device__ __forceinline__ lane_t<VEC> lane_ld(const float* p) {
    if constexpr (VEC) return ld4(p);
    else return *p;
}
template <bool VEC>
__device__ __forceinline__ lane_t<VEC> lane_zero() {
    if constexpr (VEC) return f4(0.f);
    else return 0.f;
}
__device__ __forceinline__ void lane_st(float* p, float4 x) { st4(p, x); }
__device__ __forceinline__ void lane_st(float* p, float x) { *p = x; }
__device__ __forceinline__ float4 lane_fma(float4 a, float4 b, float4 c) { return fma4(a, b, c); }
__device__ __forceinline__ float lane_fma(float a, float b, float c) { return fmaf(a, b, c); }
__device__ __forceinline__ float4 lane_add(float4 a, float4 b) { return add4(a, b); }
__device__ __forceinline__ float lane_add(float a, float b) { return a + b; }
// dropout of the lane at logical linear index i
__device__ __forceinline__ float4 lane_drop(const DView& v, uint64_t i, float4 x) {
    return mul4(x, drop_mult4(v.seed, i, v.rate, v.inv_keep));
}
__device__ __forceinline__ float lane_drop(const DView& v, uint64_t i, float x) {
    return x * drop_mult(v.seed, i, v.rate, v.inv_keep);
}
// the view's value at (n, hh, ww), channels c.., dropout applied
template <int MODE, bool DROP, bool VEC>
__device__ __forceinline__ lane_t<VEC> tap(const DView& v, int n, int hh, int ww, int H, int W, int c) {
    lane_t<VEC> x;
    if constexpr (VEC) x = view_load4<MODE>(v, n, hh, ww, H, W, c);
    else x = view_load1<MODE>(v, n, hh, ww, H, W, c);
    if constexpr (DROP) x = lane_drop(v, ((uint64_t)((int64_t)(n * H + hh) * W + ww)) * v.C + c, x);
    return x;
}

// ------------------------------------------------------------------ forward ----
template <int MODE, bool DROP, bool VEC>
__global__ __launch_bounds__(kThreads) void dw_fwd_kernel(DView v, int N, int H, int W,
                                                          const float* __restrict__ K,
                                                          float* __restrict__ Y) {
    const int C = v.C;
    const int CQ = VEC ? C / 4 : C;
    const int total = N * H * W * CQ;
    for (int idx = blockIdx.x * kThreads + threadIdx.x; idx < total; idx += gridDim.x * kThreads) {
        const int cq = idx % CQ;
        const int p = idx / CQ;
        int n, h, w;
        decompose(p, H, W, n, h, w);
        const int c = cq * LW<VEC>;
        lane_t<VEC> acc = lane_zero<VEC>();
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const int hh = h + i - 1;
            if (hh < 0 || hh >= H) continue;
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const int ww = w + j - 1;
                if (ww < 0 || ww >= W) continue;
                acc = lane_fma(tap<MODE, DROP, VEC>(v, n, hh, ww, H, W, c), lane_ld<VEC>(K + (i * 3 + j) * C + c), acc);
            }
        }
        lane_st(Y + p * C + c, acc);
    }
}

// ------------------------------------------------------------ backward data ----
// dx[h,w] = sum_{i,j} dy[h-i+1, w-j+1] * k[i,j]; then dropout, then routed per view.
template <int MODE, bool DROP, bool VEC>
__global__ __launch_bounds__(kThreads) void dw_bwd_data_kernel(DView v, int N, int H, int W,
                                                               const float* __restrict__ K,
                                                               const float* __restrict__ dY,
                                                               float* __restrict__ dx0,
                                                               float* __restrict__ dx1) {
    const int C = v.C;
    const int CQ = VEC ? C / 4 : C;
    const int total = N * H * W * CQ;
    for (int idx = blockIdx.x * kThreads + threadIdx.x; idx < total; idx += gridDim.x * kThreads) {
        const int cq = idx % CQ;
        const int p = idx / CQ;
        int n, h, w;
        decompose(p, H, W, n, h, w);
        const int c = cq * LW<VEC>;
        lane_t<VEC> acc = lane_zero<VEC>();
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const int hh = h - i + 1;
            if (hh < 0 || hh >= H) continue;
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const int ww = w - j + 1;
                if (ww < 0 || ww >= W) continue;
                acc = lane_fma(lane_ld<VEC>(dY + ((int64_t)(n * H + hh) * W + ww) * C + c),
                               lane_ld<VEC>(K + (i * 3 + j) * C + c), acc);
            }
        }
        if constexpr (DROP) acc = lane_drop(v, (uint64_t)p * C + c, acc);
        if constexpr (MODE == UNET_VIEW_PLAIN || MODE == UNET_VIEW_BNRELU) {
            lane_st(dx0 + p * C + c, acc);
        } else if constexpr (MODE == UNET_VIEW_CONCAT) {
            if (c < v.c0)
                lane_st(dx0 + p * v.c0 + c, acc);
            else
                lane_st(dx1 + p * v.c1 + (c - v.c0), acc);
        } else {  // POOL_BNRELU: route to the first max of the 2x2 window (row-major scan)
            const int W2 = 2 * W;
            const int64_t b = ((int64_t)(n * 2 * H + 2 * h) * W2 + 2 * w) * v.c0 + c;
            const int64_t off[4] = {0, v.c0, (int64_t)W2 * v.c0, (int64_t)W2 * v.c0 + v.c0};
            if constexpr (VEC) {
                const float4 sc = ld4(v.sc0 + c), sh = ld4(v.sh0 + c);
                float4 xv[4], g[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    xv[q] = bnrelu4(ld4(v.src0 + b + off[q]), sc, sh);
                    g[q] = ld4(dx0 + b + off[q]);
                }
                pool_route(g, xv, acc);
#pragma unroll
                for (int q = 0; q < 4; ++q) st4(dx0 + b + off[q], g[q]);
            } else {  // one channel: only the maximum's gradient is touched
                const float sc = v.sc0[c], sh = v.sh0[c];
                dx0[b + off[pool_first_max(bnrelu(v.src0[b], sc, sh), bnrelu(v.src0[b + off[1]], sc, sh),
                                           bnrelu(v.src0[b + off[2]], sc, sh), bnrelu(v.src0[b + off[3]], sc, sh))]] += acc;
            }
        }
    }
}

// ---------------------------------------------------------- backward filter ----
// dk[i,j,c] = sum_p x(p + (i-1, j-1))[c] * dy[p][c].  Block = CT channel lanes x PL
// pixel lanes over a pixel chunk (CQ lanes per pixel; all three from dw_filter_plan, which derives the grid
// from the same numbers); fixed-order LDS reduction -> partial[chunk][9][C].
template <int MODE, bool DROP, bool VEC>
__global__ __launch_bounds__(kThreads) void dw_bwd_filter_kernel(DView v, int N, int H, int W,
                                                                 const float* __restrict__ dY,
                                                                 float* __restrict__ part, int CQ, int CT, int PL,
                                                                 int64_t ppc) {
    const int C = v.C;
    const int tid = threadIdx.x;
    const int cl = tid % CT;
    const int pl = tid / CT;
    const int cq = blockIdx.x * CT + cl;
    const int c = cq * LW<VEC>;
    const int P = N * H * W;
    const int p0 = blockIdx.y * (int)ppc;
    const int p1 = p0 + (int)ppc < P ? p0 + (int)ppc : P;
    __shared__ lane_t<VEC> red[kThreads];

    const bool active = pl < PL && cq < CQ;
    lane_t<VEC> acc[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) acc[t] = lane_zero<VEC>();
    if (active) {
        for (int p = p0 + pl; p < p1; p += PL) {
            int n, h, w;
            decompose(p, H, W, n, h, w);
            const lane_t<VEC> g = lane_ld<VEC>(dY + p * C + c);
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const int hh = h + i - 1;
                if (hh < 0 || hh >= H) continue;
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    const int ww = w + j - 1;
                    if (ww < 0 || ww >= W) continue;
                    acc[i * 3 + j] = lane_fma(tap<MODE, DROP, VEC>(v, n, hh, ww, H, W, c), g, acc[i * 3 + j]);
                }
            }
        }
    }
    // fixed-order reduction over the PL pixel lanes, one tap at a time
    float* out = part + (int64_t)blockIdx.y * 9 * C;
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        red[tid] = acc[t];
        __syncthreads();
        if (pl == 0 && cq < CQ) {
            lane_t<VEC> s = red[cl];
            for (int q = 1; q < PL; ++q) s = lane_add(s, red[q * CT + cl]);
            lane_st(out + t * C + c, s);
        }
        __syncthreads();
    }
}

// ----------------------------------------------------------------- materialize ----
template <int MODE, bool DROP, bool VEC>
__global__ __launch_bounds__(kThreads) void view_materialize_kernel(DView v, int N, int H, int W,
                                                                    float* __restrict__ out) {
    const int C = v.C;
    const int CQ = VEC ? C / 4 : C;
    const int total = N * H * W * CQ;
    for (int idx = blockIdx.x * kThreads + threadIdx.x; idx < total; idx += gridDim.x * kThreads) {
        const int cq = idx % CQ;
        const int p = idx / CQ;
        int n, h, w;
        decompose(p, H, W, n, h, w);
        lane_st(out + p * C + cq * LW<VEC>, tap<MODE, DROP, VEC>(v, n, h, w, H, W, cq * LW<VEC>));
    }
}

}  // namespace

}  // namespace unet

using namespace unet;
using dw::DW_TILED;

// The checks every entry point shares, then the plan of the call.  Returns 0 or -1.
static int plan_for(const unet_view* x, int n, int h, int w, const char* op, dw::DwPlan& p) {
    if (check_view(x, op)) return -1;
    UNET_CHECK_ARG(n > 0 && h > 0 && w > 0, "%s: bad shape n=%d h=%d w=%d", op, n, h, w);
    UNET_CHECK_ARG(dw::index_fits(x->mode, x->c0, x->c1, n, h, w), "%s: tensor too large for 32-bit indexing", op);
    p = dw::dw_plan(x->mode, x->c0, x->c1, n, h, w);
    return 0;
}

extern "C" int unet_dwconv3x3_fwd(const unet_view* x, int n, int h, int w, const float* dw_kernel, float* y,
                                  unet_stream_t stream) {
    const char* op = "unet_dwconv3x3_fwd";
    dw::DwPlan p;
    if (plan_for(x, n, h, w, op, p)) return -1;
    UNET_CHECK_ARG(dw_kernel && y, "%s: null kernel/output", op);
    const DView v = make_dview(*x);
    hipStream_t st = as_stream(stream);
    if (p.route == DW_TILED) return dw_tiled_fwd(p, v, x->mode, x->drop_rate > 0.f, dw_kernel, y, st);
    with_view(x->mode, x->drop_rate > 0.f, [&](auto M, auto D) {
        with_bool(p.vec(), [&](auto V) {
            dw_fwd_kernel<M(), D(), V()><<<p.flat_grid, kThreads, 0, st>>>(v, n, h, w, dw_kernel, y);
        });
    });
    UNET_CHECK_LAUNCH(op);
    return 0;
}

extern "C" int unet_view_materialize(const unet_view* x, int n, int h, int w, float* out, unet_stream_t stream) {
    const char* op = "unet_view_materialize";
    dw::DwPlan p;
    if (plan_for(x, n, h, w, op, p)) return -1;
    UNET_CHECK_ARG(out, "%s: null output", op);
    const DView v = make_dview(*x);
    hipStream_t st = as_stream(stream);
    with_view(x->mode, x->drop_rate > 0.f, [&](auto M, auto D) {  // flat kernels only, whatever the route
        with_bool(p.vec(), [&](auto V) {
            view_materialize_kernel<M(), D(), V()><<<p.flat_grid, kThreads, 0, st>>>(v, n, h, w, out);
        });
    });
    UNET_CHECK_LAUNCH(op);
    return 0;
}

extern "C" int unet_dwconv3x3_bwd_data(const unet_view* x, int n, int h, int w, const float* dw_kernel,
                                       const float* dy, float* dx0, float* dx1, unet_stream_t stream) {
    const char* op = "unet_dwconv3x3_bwd_data";
    dw::DwPlan p;
    if (plan_for(x, n, h, w, op, p)) return -1;
    UNET_CHECK_ARG(dw_kernel && dy && dx0, "%s: null pointer", op);
    UNET_CHECK_ARG(x->mode != UNET_VIEW_CONCAT || dx1, "%s: CONCAT view needs dx1", op);
    const DView v = make_dview(*x);
    hipStream_t st = as_stream(stream);
    if (p.route == DW_TILED) return dw_tiled_bwd_data(p, v, x->mode, x->drop_rate > 0.f, dw_kernel, dy, dx0, dx1, st);
    with_view(x->mode, x->drop_rate > 0.f, [&](auto M, auto D) {
        with_bool(p.vec(), [&](auto V) {
            dw_bwd_data_kernel<M(), D(), V()><<<p.flat_grid, kThreads, 0, st>>>(v, n, h, w, dw_kernel, dy, dx0, dx1);
        });
    });
    UNET_CHECK_LAUNCH(op);
    return 0;
}

extern "C" int unet_dwconv3x3_bwd_data_bnstats_slabs(const unet_view* x, int n, int h, int w) {
    return x ? dw::dw_bnstats_slabs(x->mode, x->c0, n, h, w) : 0;
}

extern "C" int unet_dwconv3x3_bwd_data_bnstats(const unet_view* x, int n, int h, int w, const float* dw_kernel,
                                               const float* dy, float* dx0, const float* mean, const float* rstd,
                                               float* bn_partials, unet_stream_t stream) {
    const char* op = "unet_dwconv3x3_bwd_data_bnstats";
    dw::DwPlan p;
    if (plan_for(x, n, h, w, op, p)) return -1;
    UNET_CHECK_ARG(dw_kernel && dy && dx0 && bn_partials, "%s: null pointer", op);
    UNET_CHECK_ARG(dw::dw_bnstats_slabs(x->mode, x->c0, n, h, w) > 0,
                   "%s: needs a POOL_BNRELU or BNRELU view with channels %% 4 == 0 (tiled path)", op);
    UNET_CHECK_ARG((mean == nullptr) == (rstd == nullptr), "%s: mean and rstd go together", op);
    return dw_tiled_bwd_data_bnstats(p, make_dview(*x), x->mode, x->drop_rate > 0.f, dw_kernel, dy, dx0, mean, rstd,
                                     bn_partials, as_stream(stream));
}

extern "C" int unet_dwconv3x3_bwd_data_bnstats_dwf(const unet_view* x, int n, int h, int w, const float* dw_kernel,
                                                   const float* dy, float* dx0, const float* mean, const float* rstd,
                                                   float* bn_partials, float* dw_partials, unet_stream_t stream) {
    const char* op = "unet_dwconv3x3_bwd_data_bnstats_dwf";
    dw::DwPlan p;
    if (plan_for(x, n, h, w, op, p)) return -1;
    UNET_CHECK_ARG(dw_kernel && dy && dx0 && bn_partials && dw_partials, "%s: null pointer", op);
    UNET_CHECK_ARG(dw::dw_bnstats_dwf_ok(x->mode, x->c0, x->drop_rate, n, h, w),
                   "%s: needs a BNRELU view without dropout, channels %% 4 == 0 (tiled path)", op);
    UNET_CHECK_ARG((mean == nullptr) == (rstd == nullptr), "%s: mean and rstd go together", op);
    UNET_CHECK_ARG((uintptr_t)dw_partials % 16 == 0, "%s: dw_partials must be 16-B aligned", op);
    return dw_tiled_bwd_data_bnstats(p, make_dview(*x), x->mode, false, dw_kernel, dy, dx0, mean, rstd, bn_partials,
                                     as_stream(stream), dw_partials);
}

extern "C" int unet_reduce_slabs(float* slabs, int S, int64_t len, float* out, unet_stream_t stream) {
    UNET_CHECK_ARG(slabs && out && S > 0 && len > 0, "unet_reduce_slabs: bad arguments");
    return reduce_slabs(slabs, S, len, out, len, len, as_stream(stream));
}

extern "C" size_t unet_dwconv3x3_bwd_filter_workspace(int n, int h, int w, int c) {
    return dw::dw_filter_workspace(n, h, w, c);
}

extern "C" int unet_dwconv3x3_bwd_filter(const unet_view* x, int n, int h, int w, const float* dy,
                                         float* d_dw_kernel, void* ws, size_t ws_bytes, unet_stream_t stream) {
    const char* op = "unet_dwconv3x3_bwd_filter";
    dw::DwPlan p;
    if (plan_for(x, n, h, w, op, p)) return -1;
    UNET_CHECK_ARG(dy && d_dw_kernel, "%s: null pointer", op);
    const dw::DwFilterPlan f = dw::dw_filter_plan(x->mode, x->c0, x->c1, n, h, w);
    // the caller sized ws by the view-less query, which covers every view of these channels
    const size_t need = dw::dw_filter_workspace(n, h, w, p.C);
    UNET_CHECK_ARG(ws && ws_bytes >= need, "%s: workspace %zu < %zu", op, ws_bytes, need);
    const DView v = make_dview(*x);
    hipStream_t st = as_stream(stream);
    float* part = static_cast<float*>(ws);
    if (p.route == DW_TILED) {
        if (int rc = dw_tiled_bwd_filter(f, v, x->mode, x->drop_rate > 0.f, dy, part, st)) return rc;
    } else {
        with_view(x->mode, x->drop_rate > 0.f, [&](auto M, auto D) {
            with_bool(p.vec(), [&](auto V) {
                dw_bwd_filter_kernel<M(), D(), V()><<<dim3(f.grid_x, f.grid_y), kThreads, 0, st>>>(
                    v, n, h, w, dy, part, p.CQ, f.CT, f.PL, f.ppc);
            });
        });
        UNET_CHECK_LAUNCH(op);
    }
    return reduce_slabs(part, f.S, (int64_t)9 * p.C, d_dw_kernel, (int64_t)9 * p.C, (int64_t)9 * p.C, st);
}
