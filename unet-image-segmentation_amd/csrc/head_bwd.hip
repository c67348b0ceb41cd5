// Head backward: the four kernel families and the backward entry points (route policy: head_plan.h).
#include "head.h"

namespace unet {
namespace {

// Binary head (ncls == 1), fully fused backward over 256-pixel tiles:
//   phase 1: one lane per pixel -> dlogit = dL/dp * p (1 - p) into LDS (and the db sum);
//   phase 2: one lane per (pixel, channel quad), coalesced: dx = W dlogit, and
//            dW += relu(bn(z)) * dlogit accumulated in registers across tiles;
//   end: fixed-order LDS reduction -> per-block partials of dW (Cin) and db (1).
// STATS (BNRELU view): dx is the whole da of the last decoder block, so the kernel also emits
// that block's BatchNorm-backward partial sums (bnpart[block][0][c] = sum g, [1][c] = sum g*xhat,
// g = dx*[z*sc+sh > 0], xhat = (z-mu)*rs) instead of leaving them to a pass over (dx, z).
// DLOUT (with STATS): dx = dlogit (x) W is rank one; only dlogit goes out (one float per pixel,
// `dx` is the dlogit buffer) and the consumer forms dx on load with the same product.
template <int MODE, int LOSS, bool STATS = false, bool DLOUT = false>
__global__ __launch_bounds__(256) void head_bwd1_kernel(DView v, int64_t M, int64_t hw, const float* __restrict__ W,
                                                        const float* __restrict__ prob, const float* __restrict__ yt,
                                                        const float* __restrict__ sums, float smooth, float gscale,
                                                        float* __restrict__ dx, float* __restrict__ part_w,
                                                        float* __restrict__ part_b, const float* __restrict__ mu = nullptr,
                                                        const float* __restrict__ rs = nullptr,
                                                        float* __restrict__ bnpart = nullptr) {
    main_stream_prio();
    __shared__ float dls[256];
    __shared__ float4 red[256];
    const int Cin = v.c0, CQ = Cin / 4;
    const int kq = threadIdx.x % CQ;  // CQ divides 256 (launcher checks)
    const float4 w4 = ld4(W + 4 * kq);
    float4 dw = f4(0.f);
    float db = 0.f;
    float4 s1 = f4(0.f), s2 = f4(0.f), hsc = f4(1.f), hsh = f4(0.f), smu = f4(0.f), srs = f4(0.f);
    if constexpr (STATS) {
        hsc = ld4(v.sc0 + 4 * kq);
        hsh = ld4(v.sh0 + 4 * kq);
        if (mu) {
            smu = ld4(mu + 4 * kq);
            srs = ld4(rs + 4 * kq);
        }
    }
    for (int64_t m0 = (int64_t)blockIdx.x * 256; m0 < M; m0 += (int64_t)gridDim.x * 256) {
        __syncthreads();
        {
            const int64_t m = m0 + threadIdx.x;
            float dl = 0.f;
            if (m < M) {
                const float p = prob[m];
                const float g = loss_grad<LOSS>(yt[m], sums + (m / hw) * 3, smooth, gscale);
                dl = g * p * (1.0f - p);
            }
            dls[threadIdx.x] = dl;
            if constexpr (DLOUT) {
                if (m < M) dx[m] = dl;
            }
            db += dl;
        }
        __syncthreads();
        for (int p = threadIdx.x / CQ; p < 256; p += 256 / CQ) {
            const int64_t m = m0 + p;
            if (m >= M) break;
            const float dl = dls[p];
            if constexpr (STATS) {
                const float4 zr = ld4(v.src0 + m * Cin + 4 * kq);
                const float4 a = bnrelu4(zr, hsc, hsh);
                dw = fma4(a, f4(dl), dw);
                const float4 d = mul4(w4, f4(dl));
                if constexpr (!DLOUT) st4(dx + m * Cin + 4 * kq, d);
                const float4 gm = make_float4(a.x > 0.f ? d.x : 0.f, a.y > 0.f ? d.y : 0.f, a.z > 0.f ? d.z : 0.f,
                                              a.w > 0.f ? d.w : 0.f);
                s1 = add4(s1, gm);
                const float4 xh = make_float4((zr.x - smu.x) * srs.x, (zr.y - smu.y) * srs.y, (zr.z - smu.z) * srs.z,
                                              (zr.w - smu.w) * srs.w);
                s2 = fma4(gm, xh, s2);
            } else {
                const float4 a = row_load4<MODE, false>(v, m, 4 * kq);
                dw = fma4(a, f4(dl), dw);
                st4(dx + m * Cin + 4 * kq, mul4(w4, f4(dl)));
            }
        }
    }
    if constexpr (STATS) {  // fixed-order per-channel-quad sums of the block's threads
        BLOCK_SUM_STRIDE(red, s1, CQ, t, st4(bnpart + (int64_t)blockIdx.x * 2 * Cin + 4 * threadIdx.x, t));
        BLOCK_SUM_STRIDE(red, s2, CQ, t, st4(bnpart + (int64_t)blockIdx.x * 2 * Cin + Cin + 4 * threadIdx.x, t));
    }
    BLOCK_SUM_STRIDE(red, dw, CQ, s, st4(part_w + (int64_t)blockIdx.x * Cin + 4 * threadIdx.x, s));
    const float dbs = wave_sum(db);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) dls[threadIdx.x >> 6] = dbs;
    __syncthreads();
    if (threadIdx.x == 0) part_b[blockIdx.x] = dls[0] + dls[1] + dls[2] + dls[3];
}

// Multi-class head: dlogit (softmax backward) to global for the weight-gradient GEMM, and dx
// written coalesced per (pixel, channel quad) from LDS copies of W and the tile's dlogits.
template <int NC, int LOSS>
__global__ __launch_bounds__(256) void head_bwd_kernel(int64_t M, int64_t hw, int Cin, int ncls,
                                                       const float* __restrict__ W, const float* __restrict__ prob,
                                                       const float* __restrict__ yt, const float* __restrict__ sums,
                                                       float smooth, float gscale, float* __restrict__ dlogit,
                                                       float* __restrict__ dx) {
    __shared__ float Ws[kMaxCin * NC];
    __shared__ float dls[256 * NC];
    STAGE_KERNEL(Ws, W, Cin, NC, ncls)
    const int CQ = Cin / 4;
    for (int64_t m0 = (int64_t)blockIdx.x * 256; m0 < M; m0 += (int64_t)gridDim.x * 256) {
        __syncthreads();
        {
            SOFTMAX_BWD(dl, NC, LOSS, m0 + threadIdx.x, M, hw, ncls, prob, yt, sums, smooth, gscale, dlogit,
                        dls[threadIdx.x * NC + c] = dl[c]);
        }
        __syncthreads();
        for (int idx = threadIdx.x; idx < 256 * CQ; idx += 256) {
            const int p = idx / CQ, kq = idx - (idx / CQ) * CQ;
            const int64_t m = m0 + p;
            if (m >= M) continue;
            float4 o = f4(0.f);
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                const float d = dls[p * NC + c];
                o.x = fmaf(Ws[(4 * kq + 0) * NC + c], d, o.x);
                o.y = fmaf(Ws[(4 * kq + 1) * NC + c], d, o.y);
                o.z = fmaf(Ws[(4 * kq + 2) * NC + c], d, o.z);
                o.w = fmaf(Ws[(4 * kq + 3) * NC + c], d, o.w);
            }
            st4(dx + m * Cin + 4 * kq, o);
        }
    }
}

// Multi-class head backward over 256-pixel tiles: one thread per pixel forms the softmax-backward
// dlogit (to global for the weight gradient, and into an LDS row of NC + 4 floats), then one
// thread per (pixel, channel quad) forms dx = W dlogit with its 4 x NC kernel values held in
// registers and the pixel's dlogits read 4 at a time (broadcast ds_read_b128).  (The earlier form
// re-read the kernel from LDS for every output and stored dlogit rows 32 floats apart, 32-way
// bank conflicts: 715 us per batch-8 backward, profiles/r4j_cfg4_trace.txt.)
template <int NC, int LOSS>
__global__ __launch_bounds__(256) void head_bwdm_kernel(int64_t M, int64_t hw, int Cin, int ncls,
                                                        const float* __restrict__ W, const float* __restrict__ prob,
                                                        const float* __restrict__ yt, const float* __restrict__ sums,
                                                        float smooth, float gscale, float* __restrict__ dlogit,
                                                        float* __restrict__ dx) {
    constexpr int LD = NC + 4;
    __shared__ __attribute__((aligned(16))) float dls[256 * LD];
    const int CQ = Cin / 4;  // divides 256 (launcher)
    const int kq = threadIdx.x % CQ, pp = threadIdx.x / CQ, PS = 256 / CQ;
    float wr[4][NC];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int c = 0; c < NC; ++c) wr[j][c] = c < ncls ? W[(4 * kq + j) * ncls + c] : 0.f;
    for (int64_t m0 = (int64_t)blockIdx.x * 256; m0 < M; m0 += (int64_t)gridDim.x * 256) {
        {
            SOFTMAX_BWD(dl, NC, LOSS, m0 + threadIdx.x, M, hw, ncls, prob, yt, sums, smooth, gscale, dlogit, (void)0);
#pragma unroll
            for (int c4 = 0; c4 < NC / 4; ++c4)
                *reinterpret_cast<float4*>(&dls[threadIdx.x * LD + 4 * c4]) =
                    make_float4(dl[4 * c4], dl[4 * c4 + 1], dl[4 * c4 + 2], dl[4 * c4 + 3]);
        }
        __syncthreads();
        for (int p = pp; p < 256; p += PS) {
            const int64_t m = m0 + p;
            if (m >= M) break;
            float4 o = f4(0.f);
#pragma unroll
            for (int c4 = 0; c4 < NC / 4; ++c4) {
                const float4 d = *reinterpret_cast<const float4*>(&dls[p * LD + 4 * c4]);
                const float dv[4] = {d.x, d.y, d.z, d.w};
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    o.x = fmaf(wr[0][4 * c4 + i], dv[i], o.x);
                    o.y = fmaf(wr[1][4 * c4 + i], dv[i], o.y);
                    o.z = fmaf(wr[2][4 * c4 + i], dv[i], o.z);
                    o.w = fmaf(wr[3][4 * c4 + i], dv[i], o.w);
                }
            }
            st4(dx + m * Cin + 4 * kq, o);
        }
        __syncthreads();
    }
}

// Multi-class head, fully fused backward (ncls <= 24, Cin <= 64 with Cin / 2 dividing 256) over
// 256-pixel tiles -- one pass instead of dlogit out + a weight-gradient GEMM + a column sum (+ the
// BN-backward statistics pass over (dx, z) of the last decoder block):
//   stage  : the tile's prob and y_true rows (ncls contiguous floats a pixel) into LDS, float4;
//   phase 1: one lane per pixel -> dlogit = p (dL/dp - sum_c dL/dp_c p_c), LDS rows of NC + 4;
//   phase 2: one lane per (pixel, channel pair): dx = W dlogit with W's two rows in registers,
//            dW += x dlogit^T in registers across tiles, (STATS) the BN-backward partials of dx;
//            lanes < 8 NC: the tile's dlogit column sums (db), 32 rows each;
//   end    : fixed-order LDS reductions -> per-block partials of dW (Cin x ncls), db (ncls) and
//            (STATS) bnpart[block][0 | 1][c] = sum g | sum g xhat, g = dx [z sc + sh > 0].
typedef float f2v __attribute__((ext_vector_type(2)));
template <int MODE, int NC, int LOSS, bool STATS>
__global__ __launch_bounds__(256) void head_bwdmf_kernel(DView v, int64_t M, int64_t hw, int ncls,
                                                         const float* __restrict__ W, const float* __restrict__ prob,
                                                         const float* __restrict__ yt, const float* __restrict__ sums,
                                                         float smooth, float gscale, bool vec, float* __restrict__ dx,
                                                         float* __restrict__ part_w, float* __restrict__ part_b,
                                                         const float* __restrict__ mu, const float* __restrict__ rs,
                                                         float* __restrict__ bnpart, int ko) {
    main_stream_prio();
    constexpr int LD = NC + 4;
    __shared__ __attribute__((aligned(16))) float Pt[256 * NC];
    __shared__ __attribute__((aligned(16))) float Gt[256 * NC];
    __shared__ __attribute__((aligned(16))) float dls[256 * LD];
    __shared__ float cf[2 * NC * 3];  // the tile's per-(image, class) dice sums (hw >= 256: <= 2 images)
    const bool cfl = hw >= 256;
    const int Cin = v.c0, CP = Cin / 2;
    const int kp = threadIdx.x % CP, pp = threadIdx.x / CP, PS = 256 / CP;
    const int c0 = 2 * kp;
    // the channel pair's kernel rows and weight-gradient sums as float pairs (packed FMAs)
    f2v wr[NC], dw[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        wr[c] = c < ncls ? f2v{W[c0 * ncls + c], W[(c0 + 1) * ncls + c]} : f2v{0.f, 0.f};
        dw[c] = f2v{0.f, 0.f};
    }
    float2 hsc = make_float2(1.f, 1.f), hsh = make_float2(0.f, 0.f), smu = hsh, srs = hsh, s1 = hsh, s2 = hsh;
    if constexpr (MODE == UNET_VIEW_BNRELU) {
        hsc = *reinterpret_cast<const float2*>(v.sc0 + c0);
        hsh = *reinterpret_cast<const float2*>(v.sh0 + c0);
    }
    if constexpr (STATS) {
        if (mu) {
            smu = *reinterpret_cast<const float2*>(mu + c0);
            srs = *reinterpret_cast<const float2*>(rs + c0);
        }
    }
    const int dbc = threadIdx.x % NC, dbq = threadIdx.x / NC;  // db: column, 32-row group
    float dbp = 0.f;
    for (int64_t m0 = (int64_t)blockIdx.x * 256; m0 < M; m0 += (int64_t)gridDim.x * 256) {
        const int np = M - m0 < 256 ? (int)(M - m0) : 256;
        const int cnt = np * ncls;
        const float* pg = prob + m0 * ncls;
        const float* yg = yt + m0 * ncls;
        __syncthreads();
        const int c4n = vec ? cnt >> 2 : 0;
        for (int i0 = threadIdx.x; i0 < c4n; i0 += 256 * 3) {  // 3 + 3 float4 loads in flight
            float4 tp[3], ty[3];
#pragma unroll
            for (int u = 0; u < 3; ++u) {
                const int i = i0 + 256 * u;
                tp[u] = i < c4n && !(ko & 8) ? ld4(pg + 4 * i) : f4(0.5f);
                ty[u] = i < c4n && !(ko & 8) ? ld4(yg + 4 * i) : f4(0.5f);
            }
#pragma unroll
            for (int u = 0; u < 3; ++u) {
                const int i = i0 + 256 * u;
                if (i < c4n) {
                    reinterpret_cast<float4*>(Pt)[i] = tp[u];
                    reinterpret_cast<float4*>(Gt)[i] = ty[u];
                }
            }
        }
        for (int i = 4 * c4n + threadIdx.x; i < cnt; i += 256) {
            Pt[i] = pg[i];
            Gt[i] = yg[i];
        }
        const int64_t n0 = m0 / hw;
        if (cfl && threadIdx.x < 2 * ncls * 3) {
            const int64_t o = n0 * ncls * 3 + threadIdx.x;
            cf[threadIdx.x] = o < (M / hw) * ncls * 3 ? sums[o] : 0.f;
        }
        __syncthreads();
        {
            const int p = threadIdx.x;
            float dl[NC];
#pragma unroll
            for (int c = 0; c < NC; ++c) dl[c] = 0.f;
            if (p < np && !(ko & 64)) {
                const int64_t nimg = (m0 + p) / hw;
                const float* s3 = cfl ? cf + (nimg - n0) * ncls * 3 : sums + nimg * ncls * 3;
                float s = 0.f;
#pragma unroll
                for (int c = 0; c < NC; ++c)
                    if (c < ncls) {
                        const float g = (ko & 1) ? Gt[p * ncls + c] : loss_grad<LOSS>(Gt[p * ncls + c], s3 + 3 * c, smooth, gscale);
                        dl[c] = g;
                        s = fmaf(g, Pt[p * ncls + c], s);
                    }
#pragma unroll
                for (int c = 0; c < NC; ++c)
                    if (c < ncls) dl[c] = Pt[p * ncls + c] * (dl[c] - s);
            }
#pragma unroll
            for (int c4 = 0; c4 < NC / 4; ++c4)
                *reinterpret_cast<float4*>(&dls[p * LD + 4 * c4]) =
                    make_float4(dl[4 * c4], dl[4 * c4 + 1], dl[4 * c4 + 2], dl[4 * c4 + 3]);
        }
        __syncthreads();
        if (threadIdx.x < 8 * NC && !(ko & 16)) {
            float t = 0.f;
            for (int q = 0; q < 32; ++q) t += dls[(dbq * 32 + q) * LD + dbc];
            dbp += t;
        }
        // input pairs four pixels at a time, the next four loaded before this four's dx stores
        // (vmcnt counts stores too: a load issued after a store waits for it)
        constexpr int U = 4;
        float2 zq[U];
        auto zload = [&](int pb) {
#pragma unroll
            for (int u = 0; u < U; ++u)
                zq[u] = pb + u * PS < np && !(ko & 2)
                            ? *reinterpret_cast<const float2*>(v.src0 + (m0 + pb + u * PS) * Cin + c0)
                            : make_float2(0.5f, 0.5f);
        };
        zload(pp);
        for (int pb = pp; pb < np; pb += U * PS) {
            float2 zc[U];
#pragma unroll
            for (int u = 0; u < U; ++u) zc[u] = zq[u];
            if (pb + U * PS < np) zload(pb + U * PS);
#pragma unroll
            for (int u = 0; u < U; ++u) {
            const int p = pb + u * PS;
            if (p >= np) break;
            const int64_t m = m0 + p;
            const float2 zr = zc[u];
            float2 a = zr;
            if constexpr (MODE == UNET_VIEW_BNRELU)
                a = make_float2(fmaxf(fmaf(zr.x, hsc.x, hsh.x), 0.f), fmaxf(fmaf(zr.y, hsc.y, hsh.y), 0.f));
            f2v o = {0.f, 0.f};
            const f2v a2 = {a.x, a.y};
#pragma unroll
            for (int c4 = 0; c4 < ((ko & 32) ? 0 : NC / 4); ++c4) {
                const float4 d = *reinterpret_cast<const float4*>(&dls[p * LD + 4 * c4]);
                const float dv[4] = {d.x, d.y, d.z, d.w};
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const f2v dd = {dv[i], dv[i]};
                    o = __builtin_elementwise_fma(wr[4 * c4 + i], dd, o);
                    dw[4 * c4 + i] = __builtin_elementwise_fma(a2, dd, dw[4 * c4 + i]);
                }
            }
            const float ox = o.x, oy = o.y;
            if (!(ko & 4)) *reinterpret_cast<float2*>(dx + m * Cin + c0) = make_float2(ox, oy);
            if constexpr (STATS) {
                const float gx = a.x > 0.f ? ox : 0.f, gy = a.y > 0.f ? oy : 0.f;
                s1.x += gx;
                s1.y += gy;
                s2.x = fmaf(gx, (zr.x - smu.x) * srs.x, s2.x);
                s2.y = fmaf(gy, (zr.y - smu.y) * srs.y, s2.y);
            }
            }
        }
    }
    // per-block partials, each a fixed-order sum over the block's lanes
    float4* red = reinterpret_cast<float4*>(Pt);  // 256 float4 (Pt holds 256 NC >= 1024 floats)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int c4 = 0; c4 < NC / 4; ++c4) {
            const float4 d = j == 0 ? make_float4(dw[4 * c4].x, dw[4 * c4 + 1].x, dw[4 * c4 + 2].x, dw[4 * c4 + 3].x)
                                    : make_float4(dw[4 * c4].y, dw[4 * c4 + 1].y, dw[4 * c4 + 2].y, dw[4 * c4 + 3].y);
            BLOCK_SUM_STRIDE(red, d, CP, t, {
                float* o = part_w + (int64_t)blockIdx.x * Cin * ncls + (2 * threadIdx.x + j) * ncls + 4 * c4;
                if (4 * c4 + 0 < ncls) o[0] = t.x;
                if (4 * c4 + 1 < ncls) o[1] = t.y;
                if (4 * c4 + 2 < ncls) o[2] = t.z;
                if (4 * c4 + 3 < ncls) o[3] = t.w;
            });
        }
    if constexpr (STATS) {
        BLOCK_SUM_STRIDE(red, make_float4(s1.x, s1.y, s2.x, s2.y), CP, t, {
            float* o = bnpart + (int64_t)blockIdx.x * 2 * Cin + 2 * threadIdx.x;
            o[0] = t.x;
            o[1] = t.y;
            o[Cin] = t.z;
            o[Cin + 1] = t.w;
        });
    }
    __syncthreads();
    Gt[threadIdx.x] = dbp;
    __syncthreads();
    if (threadIdx.x < ncls) {
        float t = 0.f;
        for (int q = 0; q < 8; ++q) t += Gt[q * NC + threadIdx.x];
        part_b[(int64_t)blockIdx.x * ncls + threadIdx.x] = t;
    }
}

}  // namespace
}  // namespace unet

using namespace unet;

extern "C" size_t unet_head_bwd_workspace(int n, int h, int w, int cin, int ncls) {
    if (n <= 0 || h <= 0 || w <= 0 || cin <= 0 || ncls <= 0) return 0;
    const int64_t M = (int64_t)n * h * w;
    return head_bwd_workspace_bytes(cin, ncls, M, head_wgrad_workspace(M, cin, ncls), colsum_workspace(M, ncls));
}

extern "C" int unet_head_bwd_bnstats_slabs(const unet_view* x, int n, int h, int w, int ncls) {
    if (!x || n <= 0 || h <= 0 || w <= 0) return 0;
    return head_bwd_bnstats_slabs(x->mode, x->c0, ncls, (int64_t)n * h * w);
}

namespace {
// out: dx, or with rank_one (unet_head_bwd_bnstats' binary form, bnpart given) the per-pixel dlogit;
// bnpart (with mu, rs or without): the fused routes also emit the BatchNorm-backward partials.
int head_bwd_impl(const unet_view* x, int n, int h, int w, int ncls, const float* kernel, const float* prob,
                  const float* y_true, const float* sums, float smooth, int loss_kind, float loss_scale, float* out,
                  bool rank_one, float* dkernel, float* dbias, void* ws, size_t ws_bytes, const float* mu,
                  const float* rs, float* bnpart, unet_stream_t stream) {
    if (check_view(x, "unet_head_bwd", true)) return -1;
    UNET_CHECK_ARG(loss_scale > 0.0f && loss_scale < 1e30f, "unet_head_bwd: loss_scale must be finite and > 0");
    UNET_CHECK_ARG(x->mode == UNET_VIEW_PLAIN || x->mode == UNET_VIEW_BNRELU,
                   "unet_head_bwd: input view must be PLAIN or BNRELU");
    UNET_CHECK_ARG(x->c0 <= kMaxCin, "unet_head_bwd: Cin %d > %d", x->c0, kMaxCin);
    UNET_CHECK_ARG(ncls >= 1 && ncls <= kMaxCls, "unet_head_bwd: num_classes out of range");
    UNET_CHECK_ARG(loss_kind == UNET_LOSS_DICE || loss_kind == UNET_LOSS_IOU, "unet_head_bwd: bad loss_kind");
    UNET_CHECK_ARG(kernel && prob && y_true && sums && out && dkernel && dbias, "unet_head_bwd: null pointer");
    UNET_CHECK_ARG(n > 0 && h > 0 && w > 0, "unet_head_bwd: bad dimensions %d x %d x %d", n, h, w);
    const size_t need = unet_head_bwd_workspace(n, h, w, x->c0, ncls);
    UNET_CHECK_ARG(ws && ws_bytes >= need, "unet_head_bwd: workspace %zu < %zu", ws_bytes, need);
    const int64_t M = (int64_t)n * h * w;
    const int64_t hw = (int64_t)h * w;
    hipStream_t st = as_stream(stream);
    // d(mean over the n*ncls (image, class) terms)/dp, times the caller's loss scale (data
    // parallelism with unequal shards: n_local * world / n_global, 1 otherwise)
    const float gscale = loss_scale / (float)((int64_t)n * ncls);
    const DView v = make_dview(*x);
    const HeadBwdPlan p = head_bwd_plan(x->c0, ncls, M);
    const int grid = p.grid;
    float* part_w = static_cast<float*>(ws);  // fused routes
    float* part_b = part_w + p.part_b_off;
    float* dlg = static_cast<float*>(ws);  // dlogit routes
    switch (p.route) {
        case HEAD_BWD_BIN_FUSED:
            with_int<UNET_LOSS_DICE, UNET_LOSS_IOU>(loss_kind, [&](auto L) {
                if (bnpart && rank_one) {
                    head_bwd1_kernel<UNET_VIEW_BNRELU, L(), true, true><<<grid, 256, 0, st>>>(
                        v, M, hw, kernel, prob, y_true, sums, smooth, gscale, out, part_w, part_b, mu, rs, bnpart);
                } else if (bnpart) {
                    head_bwd1_kernel<UNET_VIEW_BNRELU, L(), true><<<grid, 256, 0, st>>>(
                        v, M, hw, kernel, prob, y_true, sums, smooth, gscale, out, part_w, part_b, mu, rs, bnpart);
                } else {
                    with_int<UNET_VIEW_BNRELU, UNET_VIEW_PLAIN>(x->mode, [&](auto MODE) {
                        head_bwd1_kernel<MODE(), L()><<<grid, 256, 0, st>>>(v, M, hw, kernel, prob, y_true, sums, smooth,
                                                                            gscale, out, part_w, part_b);
                    });
                }
            });
            UNET_CHECK_LAUNCH("unet_head_bwd");
            return reduce_slabs_pair(part_w, x->c0, dkernel, part_b, 1, dbias, grid, st);
        case HEAD_BWD_MC_FUSED: {
            const bool vec = ((uintptr_t)prob | (uintptr_t)y_true) % 16 == 0;
            const int ko = lab_knob("UNET_HEAD_KO", 0);  // lab timing knock-outs (0 in the product)
            auto launch = [&](auto MODE, auto STATS) {
                with_int<UNET_LOSS_DICE, UNET_LOSS_IOU>(loss_kind, [&](auto L) {
                    with_bucket<4, 8, 16, 24>(ncls, [&](auto NC) {
                        head_bwdmf_kernel<MODE(), NC(), L(), STATS()><<<grid, 256, 0, st>>>(
                            v, M, hw, ncls, kernel, prob, y_true, sums, smooth, gscale, vec, out, part_w, part_b, mu, rs,
                            bnpart, ko);
                    });
                });
            };
            if (bnpart) launch(Int<UNET_VIEW_BNRELU>{}, std::true_type{});
            else if (x->mode == UNET_VIEW_BNRELU) launch(Int<UNET_VIEW_BNRELU>{}, std::false_type{});
            else launch(Int<UNET_VIEW_PLAIN>{}, std::false_type{});
            UNET_CHECK_LAUNCH("unet_head_bwd");
            return reduce_slabs_pair(part_w, (int64_t)x->c0 * ncls, dkernel, part_b, ncls, dbias, grid, st);
        }
        case HEAD_BWD_MC_REG:  // kernel in registers, dlogit rows in LDS
            with_int<UNET_LOSS_DICE, UNET_LOSS_IOU>(loss_kind, [&](auto L) {
                with_bucket<4, 8, 16, 24, 32>(ncls, [&](auto NC) {
                    head_bwdm_kernel<NC(), L()><<<grid, 256, 0, st>>>(M, hw, x->c0, ncls, kernel, prob, y_true, sums,
                                                                      smooth, gscale, dlg, out);
                });
            });
            break;
        default:
            with_int<UNET_LOSS_DICE, UNET_LOSS_IOU>(loss_kind, [&](auto L) {
                with_bool(ncls == 1, [&](auto ONE) {
                    head_bwd_kernel<ONE() ? 1 : kMaxCls, L()><<<grid, 256, 0, st>>>(M, hw, x->c0, ncls, kernel, prob,
                                                                                    y_true, sums, smooth, gscale, dlg, out);
                });
            });
    }
    UNET_CHECK_LAUNCH("unet_head_bwd");
    void* ws2 = static_cast<char*>(ws) + p.dlogit_bytes;
    const size_t ws2_bytes = ws_bytes - p.dlogit_bytes;
    int rc = head_wgrad(x, M, dlg, ncls, dkernel, ws2, ws2_bytes, st);
    if (rc) return rc;
    return colsum(dlg, M, ncls, dbias, ws2, ws2_bytes, st);
}
}  // namespace

extern "C" int unet_head_bwd_bnstats(const unet_view* x, int n, int h, int w, int ncls, const float* kernel,
                                     const float* prob, const float* y_true, const float* sums, float smooth,
                                     int loss_kind, float loss_scale, float* dx, float* dlogit, float* dkernel,
                                     float* dbias, const float* mean,
                                     const float* rstd, float* bn_partials, void* ws, size_t ws_bytes,
                                     unet_stream_t stream) {
    UNET_CHECK_ARG(unet_head_bwd_bnstats_slabs(x, n, h, w, ncls) > 0,
                   "unet_head_bwd_bnstats: needs a BNRELU view with Cin %% 4 == 0 (multi-class: <= 24 classes, "
                   "Cin in {4, 8, 16, 32, 64})");
    UNET_CHECK_ARG(ncls == 1 || dlogit == nullptr, "unet_head_bwd_bnstats: the dlogit form is binary-only");
    UNET_CHECK_ARG(bn_partials, "unet_head_bwd_bnstats: null bn_partials");
    UNET_CHECK_ARG((mean == nullptr) == (rstd == nullptr), "unet_head_bwd_bnstats: mean and rstd go together");
    UNET_CHECK_ARG((dx == nullptr) != (dlogit == nullptr), "unet_head_bwd_bnstats: give exactly one of dx, dlogit");
    return head_bwd_impl(x, n, h, w, ncls, kernel, prob, y_true, sums, smooth, loss_kind, loss_scale,
                         dlogit ? dlogit : dx, dlogit != nullptr, dkernel, dbias, ws, ws_bytes, mean, rstd, bn_partials,
                         stream);
}

extern "C" int unet_head_bwd(const unet_view* x, int n, int h, int w, int ncls, const float* kernel,
                             const float* prob, const float* y_true, const float* sums, float smooth, int loss_kind,
                             float loss_scale, float* dx, float* dkernel, float* dbias, void* ws, size_t ws_bytes,
                             unet_stream_t stream) {
    return head_bwd_impl(x, n, h, w, ncls, kernel, prob, y_true, sums, smooth, loss_kind, loss_scale, dx, false, dkernel,
                         dbias, ws, ws_bytes, nullptr, nullptr, nullptr, stream);
}
