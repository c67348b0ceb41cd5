// BatchNormalization + ReLU of conv_block, backward (the forward is bn_fwd.hip): two passes over (da, z),
// per-channel sums (g, g*xhat) then the elementwise dz, with the ReLU mask and the consumer's dropout mask
// recomputed, not stored; or the sums alone, finished into the (mu, p, q) coefficients with which the data
// gradient GEMMs form dz on load.  The workspace layout, the grids and the route of a call are bn_plan.h's.
#include "bn_plan.h"
#include "dispatch.h"
#include "lastblock.h"
#include "view.h"

namespace unet {

using namespace bn;

namespace {
// The gated gradient g = da * drop * [z*sc+sh > 0] of four channels, and of one; i: the element's linear index
template <bool DROP>
__device__ __forceinline__ float4 gated_grad4(float4 g, const float4& zz, const float4& s4, const float4& h4,
                                              uint64_t seed, uint64_t i, float rate, float inv_keep) {
    if constexpr (DROP) g = mul4(g, drop_mult4(seed, i, rate, inv_keep));
    g.x = fmaf(zz.x, s4.x, h4.x) > 0.f ? g.x : 0.f;
    g.y = fmaf(zz.y, s4.y, h4.y) > 0.f ? g.y : 0.f;
    g.z = fmaf(zz.z, s4.z, h4.z) > 0.f ? g.z : 0.f;
    g.w = fmaf(zz.w, s4.w, h4.w) > 0.f ? g.w : 0.f;
    return g;
}
template <bool DROP>
__device__ __forceinline__ float gated_grad(float g, float zz, float s1, float h1, uint64_t seed, uint64_t i,
                                            float rate, float inv_keep) {
    if constexpr (DROP) g *= drop_mult(seed, i, rate, inv_keep);
    return fmaf(zz, s1, h1) > 0.f ? g : 0.f;
}

// partial[chunk][0][c] = sum g, partial[chunk][1][c] = sum g*xhat over the chunk's rows (RedPlan geometry)
template <bool DROP, bool VEC>
__global__ __launch_bounds__(256) void bn_bwd_reduce_kernel(const float* __restrict__ da, const float* __restrict__ z,
                                                            int64_t M, int C, const float* __restrict__ mean,
                                                            const float* __restrict__ rstd,
                                                            const float* __restrict__ sc, const float* __restrict__ sh,
                                                            float rate, float inv_keep, uint64_t seed, int CT,
                                                            int64_t rpc, float* __restrict__ part,
                                                            unsigned* __restrict__ cnt = nullptr, int ncnt = 0) {
    if (cnt && blockIdx.x == 0 && blockIdx.y == 0)  // the statistics launch that follows counts on them
        for (int i = threadIdx.x; i < ncnt; i += blockDim.x) cnt[i] = 0u;
    const int CQ = VEC ? C / 4 : C;
    const int PL = 256 / CT;
    const int tid = threadIdx.x, cl = tid % CT, pl = tid / CT;
    const int cq = blockIdx.x * CT + cl;
    const int64_t r0 = (int64_t)blockIdx.y * rpc;
    const int64_t r1 = r0 + rpc < M ? r0 + rpc : M;
    __shared__ float4 red[2][256];
    float4 sg = f4(0.f), sgx = f4(0.f);
    if (pl < PL && cq < CQ) {
        if constexpr (VEC) {
            const int c = cq * 4;
            const float4 s4 = ld4(sc + c), h4 = ld4(sh + c), mu = ld4(mean + c), rs = ld4(rstd + c);
            auto accum = [&](int64_t m, float4 zz, float4 g) {
                g = gated_grad4<DROP>(g, zz, s4, h4, seed, (uint64_t)m * C + c, rate, inv_keep);
                sg = add4(sg, g);
                const float4 xh = make_float4((zz.x - mu.x) * rs.x, (zz.y - mu.y) * rs.y, (zz.z - mu.z) * rs.z,
                                              (zz.w - mu.w) * rs.w);
                sgx = fma4(g, xh, sgx);
            };
            int64_t m = r0 + pl;
            for (; m + 3 * PL < r1; m += 4 * PL) {  // 8 loads in flight per thread
                float4 zz[4], dd[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    zz[u] = ld4(z + (m + u * PL) * C + c);
                    dd[u] = ld4(da + (m + u * PL) * C + c);
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) accum(m + u * PL, zz[u], dd[u]);
            }
            for (; m < r1; m += PL) accum(m, ld4(z + m * C + c), ld4(da + m * C + c));
        } else {
            const int c = cq;
            const float s1 = sc[c], h1 = sh[c], mu = mean[c], rs = rstd[c];
            for (int64_t m = r0 + pl; m < r1; m += PL) {
                const float zz = z[m * C + c];
                const float g = gated_grad<DROP>(da[m * C + c], zz, s1, h1, seed, (uint64_t)m * C + c, rate, inv_keep);
                sg.x += g;
                sgx.x = fmaf(g, (zz - mu) * rs, sgx.x);
            }
        }
    }
    red[0][tid] = sg;
    red[1][tid] = sgx;
    __syncthreads();
    if (pl == 0 && cq < CQ) {
        float4 a = red[0][cl], b = red[1][cl];
        for (int q = 1; q < PL; ++q) {
            a = add4(a, red[0][q * CT + cl]);
            b = add4(b, red[1][q * CT + cl]);
        }
        float* out = part + (int64_t)blockIdx.y * 2 * C;
        if constexpr (VEC) {
            st4(out + cq * 4, a);
            st4(out + C + cq * 4, b);
        } else {
            out[cq] = a.x;
            out[C + cq] = b.x;
        }
    }
}

template <bool DROP, bool VEC>
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(const float* __restrict__ da, const float* __restrict__ z,
                                                           int64_t M, int C, const float* __restrict__ mean,
                                                           const float* __restrict__ rstd,
                                                           const float* __restrict__ sc, const float* __restrict__ sh,
                                                           float rate, float inv_keep, uint64_t seed, int use_bn,
                                                           const float* __restrict__ sums, float* __restrict__ dz) {
    const int CQ = VEC ? C / 4 : C;
    const int64_t total = M * CQ;
    const float invM = 1.0f / (float)M;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
        const int cq = (int)(idx % CQ);
        const int64_t m = idx / CQ;
        if constexpr (VEC) {
            const int c = cq * 4;
            const float4 zz = ld4(z + m * C + c), s4 = ld4(sc + c), h4 = ld4(sh + c);
            const float4 g = gated_grad4<DROP>(ld4(da + m * C + c), zz, s4, h4, seed, (uint64_t)m * C + c, rate,
                                               inv_keep);
            float4 o = g;
            if (use_bn) {
                const float4 mu = ld4(mean + c), rs = ld4(rstd + c);
                const float4 sb = ld4(sums + c), sgx = ld4(sums + C + c);
                o.x = s4.x * (g.x - sb.x * invM - (zz.x - mu.x) * rs.x * sgx.x * invM);
                o.y = s4.y * (g.y - sb.y * invM - (zz.y - mu.y) * rs.y * sgx.y * invM);
                o.z = s4.z * (g.z - sb.z * invM - (zz.z - mu.z) * rs.z * sgx.z * invM);
                o.w = s4.w * (g.w - sb.w * invM - (zz.w - mu.w) * rs.w * sgx.w * invM);
            }
            st4(dz + m * C + c, o);
        } else {
            const int c = cq;
            const float zz = z[m * C + c];
            const float g = gated_grad<DROP>(da[m * C + c], zz, sc[c], sh[c], seed, (uint64_t)m * C + c, rate, inv_keep);
            float o = g;
            if (use_bn) o = sc[c] * (g - sums[c] * invM - (zz - mean[c]) * rstd[c] * sums[C + c] * invM);
            dz[m * C + c] = o;
        }
    }
}

// scatter the reduced sums: dbeta = sums[0], dgamma = sums[1]
__global__ void bn_bwd_store_kernel(const float* sums, int C, int use_bn, float* dgamma, float* dbeta) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    if (dbeta) dbeta[c] = sums[c];
    if (use_bn && dgamma) dgamma[c] = sums[C + c];
}

// Channel c's dbeta = S1, dgamma = S2 and the dz coefficients of A_BNBWD loads (gemm_rows.hip; common.h
// bn_bwd_dz4): coef = (mu, p, q) with p = S1 / M, q = rstd * S2 / M (zeros without BatchNorm: dz = g).
// mu_, rs_: the channel's mean and rstd, expanded in place, so a load passed here runs only with use_bn.
// (A macro: through an inlined function bn_bwd_stats_kernel compiled to another register allocation.)
#define BN_WRITE_COEF(c_, C_, s1_, s2_, invM_, use_bn_, mu_, rs_, dgamma_, dbeta_, coef_) \
    do {                                                                                  \
        if (dbeta_) dbeta_[c_] = s1_;                                                     \
        if (use_bn_ && dgamma_) dgamma_[c_] = s2_;                                        \
        coef_[c_] = use_bn_ ? mu_ : 0.f;                                                  \
        coef_[C_ + c_] = use_bn_ ? s1_ * invM_ : 0.f;                                     \
        coef_[2 * C_ + c_] = use_bn_ ? rs_ * (s2_ * invM_) : 0.f;                         \
    } while (0)

__global__ void bn_bwd_coef_kernel(const float* sums, int C, int64_t M, int use_bn, const float* mean,
                                   const float* rstd, float* dgamma, float* dbeta, float* coef) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    const float s1 = sums[c], s2 = sums[C + c];
    const float invM = 1.0f / (float)M;
    BN_WRITE_COEF(c, C, s1, s2, invM, use_bn, mean[c], rstd[c], dgamma, dbeta, coef);
}

// Statistics-only finish: the fixed-order slab reduction of (S1, S2) fused with the coefficient
// kernel above, in ONE launch.  Block (x, y) = 16 channel quads x 16 slab groups over slabs
// [64 y, 64 y + 64) (all S slabs when the grid has one row); groups are combined by wave shuffles
// and a 4-wave LDS step (4 KB of LDS: the block still fits beside side-stream GEMM blocks that
// hold most of a CU's LDS -- the 32 KB version waited up to 140 us for a slot, r1zd).  With
// several rows each block publishes its chunk row (double) and the last block of column x to
// arrive (lastblock.h) sums the rows in order and writes dgamma / dbeta / coef.
constexpr int kLQ = kFinishQuads, kSG = 16;
__device__ __forceinline__ void group_reduce8(double* a, double (*red)[8][kLQ]) {
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        a[k] += __shfl_xor(a[k], 16);
        a[k] += __shfl_xor(a[k], 32);
    }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane < kLQ) {
#pragma unroll
        for (int k = 0; k < 8; ++k) red[w][k][lane] = a[k];
    }
    __syncthreads();
    if (threadIdx.x < kLQ) {
        const int t = threadIdx.x;
#pragma unroll
        for (int k = 0; k < 8; ++k) a[k] = ((red[0][k][t] + red[1][k][t]) + red[2][k][t]) + red[3][k][t];
    }
}
// a[0..3] += u (a quad's S1), a[4..7] += v (its S2)
__device__ __forceinline__ void accum8(double* a, const float4& u, const float4& v) {
    a[0] += (double)u.x; a[1] += (double)u.y; a[2] += (double)u.z; a[3] += (double)u.w;
    a[4] += (double)v.x; a[5] += (double)v.y; a[6] += (double)v.z; a[7] += (double)v.w;
}
__global__ __launch_bounds__(256) void bn_bwd_stats_kernel(const float* __restrict__ part, int S, int C, int64_t M,
                                                           int use_bn, const float* mean, const float* rstd,
                                                           float* dgamma, float* dbeta, float* coef,
                                                           double* chunks, unsigned* cnt) {
    main_stream_prio();
    const int q = threadIdx.x % kLQ, g = threadIdx.x / kLQ;
    const int c = (blockIdx.x * kLQ + q) * 4;
    const int nch = gridDim.y;
    const int s0 = blockIdx.y * kGroupSlabs, s1 = nch == 1 || s0 + kGroupSlabs > S ? S : s0 + kGroupSlabs;
    __shared__ double red[4][8][kLQ];
    __shared__ int flag;
    // the writers' mean / rstd loaded up front: loaded after the first output store they would each
    // wait for it (the pointers may alias), a chain of 8 round trips at the end of the launch
    float mu[4] = {0.f, 0.f, 0.f, 0.f}, rs[4] = {0.f, 0.f, 0.f, 0.f};
    if (threadIdx.x < kLQ && c < C && use_bn) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            mu[k] = mean[c + k];
            rs[k] = rstd[c + k];
        }
    }
    double a[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (c < C) {
        int s = s0 + g;
        for (; s + 3 * kSG < s1; s += 4 * kSG) {  // 8 loads in flight
            float4 u[4], v[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                u[k] = ld4(part + (int64_t)(s + k * kSG) * 2 * C + c);
                v[k] = ld4(part + (int64_t)(s + k * kSG) * 2 * C + C + c);
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) accum8(a, u[k], v[k]);
        }
        for (; s < s1; s += kSG) accum8(a, ld4(part + (int64_t)s * 2 * C + c), ld4(part + (int64_t)s * 2 * C + C + c));
    }
    group_reduce8(a, red);
    if (nch > 1) {
        if (threadIdx.x < kLQ && c < C) {
            double* row = chunks + (int64_t)blockIdx.y * 2 * C;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                st_agent(row + c + k, a[k]);
                st_agent(row + C + c + k, a[4 + k]);
            }
        }
        if (!last_arrival(cnt + blockIdx.x, (unsigned)nch, &flag)) return;
#pragma unroll
        for (int k = 0; k < 8; ++k) a[k] = 0.0;
        if (c < C) {
            int r = g;
            for (; r + kSG < nch; r += 2 * kSG) {
                double u[2][8];
#pragma unroll
                for (int h = 0; h < 2; ++h)
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        u[h][k] = ld_agent(chunks + (int64_t)(r + h * kSG) * 2 * C + c + k);
                        u[h][4 + k] = ld_agent(chunks + (int64_t)(r + h * kSG) * 2 * C + C + c + k);
                    }
#pragma unroll
                for (int h = 0; h < 2; ++h)
#pragma unroll
                    for (int k = 0; k < 8; ++k) a[k] += u[h][k];
            }
            for (; r < nch; r += kSG)
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    a[k] += ld_agent(chunks + (int64_t)r * 2 * C + c + k);
                    a[4 + k] += ld_agent(chunks + (int64_t)r * 2 * C + C + c + k);
                }
        }
        group_reduce8(a, red);
    }
    if (threadIdx.x >= kLQ || c >= C) return;
    const float invM = 1.0f / (float)M;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int cc = c + k;
        const float s1v = (float)a[k], s2v = (float)a[4 + k];
        BN_WRITE_COEF(cc, C, s1v, s2v, invM, use_bn, mu[k], rs[k], dgamma, dbeta, coef);
    }
}

// dgamma / dbeta / coef from S slabs [S][2c] (c % 4 == 0) in one launch; with more than 64 slabs
// it needs `scratch` (f.nch x 2c doubles) and cdiv(c, 64) counters that are zero on entry
// (left zero on exit).
int bwd_stats_finish(const float* part, int S, int c, int64_t m, int use_bn, const float* mean, const float* rstd,
                     float* dgamma, float* dbeta, float* coef, const StatsFinish& f, double* scratch, unsigned* cnt,
                     hipStream_t st) {
    if (lab_knob("UNET_SKIP_BNBWD", 0)) return 0;  // lab: upper bound of folding the launch away
    bn_bwd_stats_kernel<<<dim3(f.grid_x, (unsigned)f.nch), 256, 0, st>>>(part, S, c, m, use_bn, mean, rstd, dgamma,
                                                                        dbeta, coef, scratch, cnt);
    UNET_CHECK_LAUNCH("bn backward statistics (finish)");
    return 0;
}

// coef_out: the statistics-only entry (no dz pass)
int bn_relu_bwd_impl(const float* da, const float* z, int64_t m, int c, const float* mean, const float* rstd,
                     const float* scale, const float* shift, int use_bn, float drop_rate, uint64_t drop_seed,
                     float* dgamma, float* dbeta, float* dz, float* coef_out, void* ws, size_t ws_bytes,
                     unet_stream_t stream) {
    UNET_CHECK_ARG(da && z && scale && shift && (dz || coef_out) && m > 0 && c > 0, "unet_bn_relu_bwd: bad args");
    UNET_CHECK_ARG(!use_bn || (mean && rstd), "unet_bn_relu_bwd: use_bn needs mean/rstd");
    UNET_CHECK_ARG(drop_rate >= 0.f && drop_rate < 1.f, "unet_bn_relu_bwd: bad drop_rate");
    const BwdWorkspace w = bwd_workspace(m, c, coef_out != nullptr);
    UNET_CHECK_ARG(ws && ws_bytes >= w.bytes, "unet_bn_relu_bwd: workspace %zu < %zu", ws_bytes, w.bytes);
    hipStream_t st = as_stream(stream);
    const RedPlan& p = w.red;
    char* base = static_cast<char*>(ws);
    float* part = reinterpret_cast<float*>(base);
    float* sums = reinterpret_cast<float*>(base + w.sums_off);
    double* scratch = reinterpret_cast<double*>(base + w.scratch_off);
    unsigned* cnt = reinterpret_cast<unsigned*>(base + w.counter_off);
    const float* mu = use_bn ? mean : scale;  // unused when !use_bn (mask only)
    const float* rs = use_bn ? rstd : scale;
    const float inv_keep = drop_rate > 0.f ? 1.0f / (1.0f - drop_rate) : 1.0f;
    const bool drop = drop_rate > 0.f;
    dim3 grid(p.ctiles, (unsigned)p.chunks);
    with_bool(drop, [&](auto D) {
        with_bool(w.vec, [&](auto V) {
            bn_bwd_reduce_kernel<D(), V()><<<grid, 256, 0, st>>>(da, z, m, c, mu, rs, scale, shift, drop_rate, inv_keep,
                                                                 drop_seed, p.CT, p.rpc, part, w.ncnt ? cnt : nullptr,
                                                                 w.ncnt);
        });
    });
    UNET_CHECK_LAUNCH("unet_bn_relu_bwd(reduce)");
    if (w.route == BWD_STATS_FINISH)
        return bwd_stats_finish(part, (int)p.chunks, c, m, use_bn, mean, rstd, dgamma, dbeta, coef_out,
                                stats_finish((int)p.chunks, c), scratch, cnt, st);
    int rc = reduce_slabs(part, (int)p.chunks, (int64_t)2 * c, sums, (int64_t)2 * c, (int64_t)2 * c, st);
    if (rc) return rc;
    if (w.route == BWD_STATS_SLABS) {
        bn_bwd_coef_kernel<<<(unsigned)cdiv(c, 256), 256, 0, st>>>(sums, c, m, use_bn, mean, rstd, dgamma, dbeta,
                                                                    coef_out);
        UNET_CHECK_LAUNCH("unet_bn_relu_bwd_stats(coef)");
        return 0;
    }
    bn_bwd_store_kernel<<<(unsigned)cdiv(c, 256), 256, 0, st>>>(sums, c, use_bn, dgamma, dbeta);
    UNET_CHECK_LAUNCH("unet_bn_relu_bwd(store)");
    with_bool(drop, [&](auto D) {
        with_bool(w.vec, [&](auto V) {
            bn_bwd_apply_kernel<D(), V()><<<w.apply_grid, 256, 0, st>>>(da, z, m, c, mu, rs, scale, shift, drop_rate,
                                                                        inv_keep, drop_seed, use_bn, sums, dz);
        });
    });
    UNET_CHECK_LAUNCH("unet_bn_relu_bwd(apply)");
    return 0;
}
}  // namespace

}  // namespace unet

using namespace unet;

extern "C" int unet_bn_bwd_coef(const float* sums, int64_t m, int c, int use_bn, const float* mean,
                                const float* rstd, float* coef, unet_stream_t stream) {
    UNET_CHECK_ARG(sums && coef && m > 0 && c > 0, "unet_bn_bwd_coef: bad args");
    UNET_CHECK_ARG(!use_bn || (mean && rstd), "unet_bn_bwd_coef: use_bn needs mean/rstd");
    bn_bwd_coef_kernel<<<(unsigned)cdiv(c, 256), 256, 0, as_stream(stream)>>>(sums, c, m, use_bn, mean, rstd, nullptr,
                                                                               nullptr, coef);
    UNET_CHECK_LAUNCH("unet_bn_bwd_coef");
    return 0;
}

extern "C" size_t unet_bn_relu_bwd_workspace(int64_t m, int c) {
    if (m <= 0 || c <= 0) return 0;
    return bwd_workspace(m, c).bytes;
}

extern "C" int unet_bn_relu_bwd(const float* da, const float* z, int64_t m, int c, const float* mean,
                                const float* rstd, const float* scale, const float* shift, int use_bn,
                                float drop_rate, uint64_t drop_seed, float* dgamma, float* dbeta, float* dz,
                                void* ws, size_t ws_bytes, unet_stream_t stream) {
    UNET_CHECK_ARG(dz, "unet_bn_relu_bwd: null dz");
    return bn_relu_bwd_impl(da, z, m, c, mean, rstd, scale, shift, use_bn, drop_rate, drop_seed, dgamma, dbeta, dz,
                            nullptr, ws, ws_bytes, stream);
}

extern "C" size_t unet_bn_stats_partials_size(int S, int c) {
    if (S <= 0 || c <= 0) return 0;
    return stats_finish(S, c).bytes;  // slabs | double scratch | in-launch finish counters
}

extern "C" int unet_bn_relu_bwd_stats_finish(float* partials, int S, int64_t m, int c, const float* mean,
                                             const float* rstd, int use_bn, float* dgamma, float* dbeta, float* coef,
                                             unet_stream_t stream) {
    UNET_CHECK_ARG(partials && coef && S > 0 && m > 0 && c > 0, "unet_bn_relu_bwd_stats_finish: bad args");
    UNET_CHECK_ARG(c % 4 == 0, "unet_bn_relu_bwd_stats_finish: channels must be a multiple of 4");
    UNET_CHECK_ARG(!use_bn || (mean && rstd), "unet_bn_relu_bwd_stats_finish: use_bn needs mean/rstd");
    const StatsFinish f = stats_finish(S, c);
    char* base = reinterpret_cast<char*>(partials);
    return bwd_stats_finish(partials, S, c, m, use_bn, mean, rstd, dgamma, dbeta, coef, f,
                            reinterpret_cast<double*>(base + f.scratch_off),
                            reinterpret_cast<unsigned*>(base + f.counter_off), as_stream(stream));
}

extern "C" int unet_bn_relu_bwd_stats(const float* da, const float* z, int64_t m, int c, const float* mean,
                                      const float* rstd, const float* scale, const float* shift, int use_bn,
                                      float drop_rate, uint64_t drop_seed, float* dgamma, float* dbeta, float* coef,
                                      void* ws, size_t ws_bytes, unet_stream_t stream) {
    UNET_CHECK_ARG(coef, "unet_bn_relu_bwd_stats: null coef");
    return bn_relu_bwd_impl(da, z, m, c, mean, rstd, scale, shift, use_bn, drop_rate, drop_seed, dgamma, dbeta,
                            nullptr, coef, ws, ws_bytes, stream);
}
