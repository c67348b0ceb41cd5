// BatchNormalization of conv_block, forward (reference model/u_net.py:22-25; Keras 3
// BatchNormalization defaults: momentum 0.99, epsilon 1e-3, batch statistics from
// tf.nn.moments = biased variance, moving stats updated with the same biased variance).
//
// Forward statistics come from the pointwise-GEMM epilogue as per-128-row (mean, M2)
// partials; unet_bn_finalize combines them with Chan's formula in double, in a fixed
// order, and emits the folded affine (scale, shift) that activation views apply on load.
// The backward is bn_bwd.hip; the buffers' layout and the grids are bn_plan.h's.
#include "bn_plan.h"
#include "lastblock.h"

namespace unet {

using namespace bn;

namespace {
// Pass 1: per (chunk of kChunkParts partials, channel) sums of the moments shifted by
// K_c = mean of partial 0 (no cancellation when |mean| >> std):  S1 = sum n_b (mean_b - K),
// S2 = sum M2_b + n_b (mean_b - K)^2, in double, fixed order (4 lanes, then lane order).
// Coalesced: consecutive threads read consecutive channels of one partial row.
__device__ __forceinline__ void chunk_sums(const float2* __restrict__ part, int64_t nblk, int64_t M, int C, int c,
                                           int lane, int chunk, double& s1, double& s2, float& k_out) {
    const int64_t b0 = (int64_t)chunk * kChunkParts;
    const int64_t b1 = b0 + kChunkParts < nblk ? b0 + kChunkParts : nblk;
    s1 = 0.0;
    s2 = 0.0;
    if (c < C) {
        // every load of the lane (K and its 16 partials) in flight at once: the finish is a chain of
        // dependent round trips on the critical path, so each batch saved is ~1 us per launch
        constexpr int PER = kChunkParts / 4;
        const float2 k0 = part[c];
        float2 pv[PER];
#pragma unroll
        for (int i = 0; i < PER; ++i) {  // branch-free: a clamped row past the chunk, masked below
            const int64_t b = b0 + lane + 4 * i;
            pv[i] = part[(b < b1 ? b : b0) * C + c];
        }
        k_out = k0.x;
        const double K = (double)k0.x;
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int64_t b = b0 + lane + 4 * i;
            if (b < b1) {
                const float2 pm = pv[i];
                const int64_t rows = (M - b * kStatsRows) < kStatsRows ? (M - b * kStatsRows) : kStatsRows;
                const double d = (double)pm.x - K;
                const double nd = (double)rows * d;
                s1 += nd;
                s2 += (double)pm.y + nd * d;
            }
        }
    }
}

// The finish of channel c: its (mean, biased var) -> rstd, the folded affine, the moving update.  gamma, beta
// and the moving statistics arrive as values (gv, bv, mmv, mvv), so a kernel can load them before its
// reduction; they are expanded in place, each under its condition (has_gamma, has_beta, update), so a load
// passed here runs only where the parameter exists.  (A macro: through an inlined function the tail of
// bn_finalize_kernel compiled to another schedule.)
#define BN_FINISH_CHANNEL(c_, mean_, var_, has_gamma_, has_beta_, gv_, bv_, eps_, momentum_, update_, mmv_, mvv_,   \
                          moving_mean_, moving_var_, mean_out_, rstd_out_, scale_out_, shift_out_)                    \
    do {                                                                                                              \
        const float rstd_ = 1.0f / sqrtf(var_ + eps_);                                                                \
        if (has_gamma_) {                                                                                             \
            const float sc_ = gv_ * rstd_;                                                                            \
            scale_out_[c_] = sc_;                                                                                     \
            shift_out_[c_] = bv_ - mean_ * sc_;                                                                       \
        } else { /* use_batch_norm=False: relu(z + bias) */                                                           \
            scale_out_[c_] = 1.0f;                                                                                    \
            shift_out_[c_] = has_beta_ ? bv_ : 0.f;                                                                   \
        }                                                                                                             \
        if (mean_out_) mean_out_[c_] = mean_;                                                                         \
        if (rstd_out_) rstd_out_[c_] = rstd_;                                                                         \
        if (update_) {                                                                                                \
            moving_mean_[c_] = mmv_ * momentum_ + mean_ * (1.0f - momentum_);                                         \
            moving_var_[c_] = mvv_ * momentum_ + var_ * (1.0f - momentum_);                                           \
        }                                                                                                             \
    } while (0)

// Pass 2 (same launch, lastblock.h): every block publishes its chunk row (sc1 stores); the last
// block of each 64-channel column to arrive sums the rows (4 lanes over interleaved chunks,
// combined in lane order) -> mean, biased var, folded affine, moving update.  One chunk: the
// block's own sums are final.
__global__ __launch_bounds__(256) void bn_finalize_kernel(const float2* __restrict__ part, int64_t nblk, int64_t M,
                                                          int C, double* __restrict__ chunks, unsigned* cnt,
                                                          const float* __restrict__ gamma,
                                                          const float* __restrict__ beta, float eps, float momentum,
                                                          float* moving_mean, float* moving_var, int update_moving,
                                                          float* mean_out, float* rstd_out, float* scale_out,
                                                          float* shift_out, double* moments) {
    const int c = blockIdx.x * 64 + (threadIdx.x & 63);
    const int lane = threadIdx.x >> 6;  // = the wave: lane 0 is wave 0, which finalizes
    const int nch = gridDim.y;
    // the finalize's other inputs loaded up front, beside the chunk's partials (its own round trips
    // would otherwise follow the reduction's)
    float gv = 1.f, bv = 0.f, mmv = 0.f, mvv = 0.f;
    if (lane == 0 && c < C && !moments) {
        if (gamma) gv = gamma[c];
        if (beta) bv = beta[c];
        if (update_moving && moving_mean && moving_var) {
            mmv = moving_mean[c];
            mvv = moving_var[c];
        }
    }
    double s1, s2;
    float K = 0.f;  // mean of partial 0 (the shift)
    chunk_sums(part, nblk, M, C, c, lane, blockIdx.y, s1, s2, K);
    __shared__ double r1[256], r2[256];
    __shared__ int flag;
    r1[threadIdx.x] = s1;
    r2[threadIdx.x] = s2;
    __syncthreads();
    if (lane == 0 && c < C)
        for (int l = 1; l < 4; ++l) {
            s1 += r1[threadIdx.x + 64 * l];
            s2 += r2[threadIdx.x + 64 * l];
        }
    if (nch > 1) {
        if (lane == 0 && c < C) {
            st_agent(chunks + ((int64_t)blockIdx.y * C + c) * 2, s1);
            st_agent(chunks + ((int64_t)blockIdx.y * C + c) * 2 + 1, s2);
        }
        if (!last_arrival(cnt + blockIdx.x, (unsigned)nch, &flag)) return;
        s1 = 0.0;
        s2 = 0.0;
        if (c < C) {
            constexpr int FB = 16;  // chunk rows per lane in flight at once (same order of the sums)
            for (int k0 = lane; k0 < nch; k0 += 4 * FB) {
                double a1[FB], a2[FB];
#pragma unroll
                for (int i = 0; i < FB; ++i) {
                    const int k = k0 + 4 * i;
                    a1[i] = k < nch ? ld_agent(chunks + ((int64_t)k * C + c) * 2) : 0.0;
                    a2[i] = k < nch ? ld_agent(chunks + ((int64_t)k * C + c) * 2 + 1) : 0.0;
                }
#pragma unroll
                for (int i = 0; i < FB; ++i)
                    if (k0 + 4 * i < nch) {
                        s1 += a1[i];
                        s2 += a2[i];
                    }
            }
        }
        __syncthreads();  // r1/r2 were read above by lane 0 before the arrival barrier; reuse
        r1[threadIdx.x] = s1;
        r2[threadIdx.x] = s2;
        __syncthreads();
        if (lane == 0 && c < C)
            for (int l = 1; l < 4; ++l) {
                s1 += r1[threadIdx.x + 64 * l];
                s2 += r2[threadIdx.x + 64 * l];
            }
    }
    if (lane != 0 || c >= C) return;
    if (moments) {  // SyncBN: this replica's (count, mean, M2) for the cross-replica combine
        if (c == 0) moments[0] = (double)M;
        moments[1 + c] = (double)K + s1 / (double)M;
        moments[1 + C + c] = s2 - s1 * (s1 / (double)M);
        return;
    }
    const double dm = s1 / (double)M;
    const float mean = (float)((double)K + dm);
    double vd = s2 / (double)M - dm * dm;
    const float var = (float)(vd > 0.0 ? vd : 0.0);
    BN_FINISH_CHANNEL(c, mean, var, gamma, beta, gv, bv, eps, momentum, (update_moving && moving_mean && moving_var),
                      mmv, mvv, moving_mean, moving_var, mean_out, rstd_out, scale_out, shift_out);
}

// SyncBN: the replicas' records [world][1 + 2C] = (count, mean[C], M2[C]) combined in rank order
// (Chan's parallel formula, double; every replica runs the same order on the same gathered records,
// so all end bitwise identical), then the finalize of the global-batch statistics.
__global__ void bn_finalize_moments_kernel(const double* __restrict__ recs, int world, int C,
                                           const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                           float momentum, float* moving_mean, float* moving_var, int update_moving,
                                           float* mean_out, float* rstd_out, float* scale_out, float* shift_out) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    const int64_t R = 1 + 2 * (int64_t)C;
    double n = recs[0], mu = recs[1 + c], m2 = recs[1 + C + c];
    for (int r = 1; r < world; ++r) {
        const double nr = recs[r * R], mr = recs[r * R + 1 + c], m2r = recs[r * R + 1 + C + c];
        const double nt = n + nr;
        if (nr <= 0.0) continue;
        const double d = mr - mu;
        mu += d * (nr / nt);
        m2 += m2r + d * d * (n * nr / nt);
        n = nt;
    }
    const double vd = m2 / n;
    const float mean = (float)mu, var = (float)(vd > 0.0 ? vd : 0.0);
    BN_FINISH_CHANNEL(c, mean, var, gamma, beta, gamma[c], beta[c], eps, momentum,
                      (update_moving && moving_mean && moving_var), moving_mean[c], moving_var[c], moving_mean,
                      moving_var, mean_out, rstd_out, scale_out, shift_out);
}

// inference: the finish of the moving statistics, nothing updated
__global__ void bn_infer_kernel(const float* gamma, const float* beta, const float* mm, const float* mv, int C,
                                float eps, float* scale, float* shift) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    float* const none = nullptr;
    const float mean = gamma ? mm[c] : 0.f, var = gamma ? mv[c] : 0.f;  // (without gamma they may be null)
    BN_FINISH_CHANNEL(c, mean, var, gamma, beta, gamma[c], beta[c], eps, 0.f, false, 0.f, 0.f, none, none, none, none,
                      scale, shift);
}

// the finalize over a partials buffer (bn_plan.h: partials | chunk rows | counters); moments: the SyncBN record
// instead of the finish
void launch_finalize(float* bn_partials, int64_t m, int c, const float* gamma, const float* beta, float eps,
                     float momentum, float* moving_mean, float* moving_var, int update_moving, float* mean, float* rstd,
                     float* scale, float* shift, double* moments, hipStream_t st) {
    const FwdPartials f = fwd_partials(m, c);
    char* base = reinterpret_cast<char*>(bn_partials);
    bn_finalize_kernel<<<dim3(f.grid_x, (unsigned)f.nch), 256, 0, st>>>(
        reinterpret_cast<const float2*>(base), f.nblk, m, c, reinterpret_cast<double*>(base + f.chunks_off),
        reinterpret_cast<unsigned*>(base + f.counter_off), gamma, beta, eps, momentum, moving_mean, moving_var,
        update_moving, mean, rstd, scale, shift, moments);
}
}  // namespace

}  // namespace unet

using namespace unet;

extern "C" size_t unet_bn_partials_size(int64_t m, int c) {
    if (m <= 0 || c <= 0) return 0;
    return fwd_partials(m, c).bytes;
}

extern "C" int unet_bn_finalize(float* bn_partials, int64_t m, int c, const float* gamma, const float* beta,
                                float eps, float momentum, float* moving_mean, float* moving_var, int update_moving,
                                float* mean, float* rstd, float* scale, float* shift, unet_stream_t stream) {
    UNET_CHECK_ARG(bn_partials && scale && shift && m > 0 && c > 0, "unet_bn_finalize: bad args");
    UNET_CHECK_ARG(!gamma || beta, "unet_bn_finalize: gamma without beta");
    if (lab_knob("UNET_SKIP_BNFIN", 0)) return 0;  // lab: upper bound of folding the launch away
    launch_finalize(bn_partials, m, c, gamma, beta, eps, momentum, moving_mean, moving_var, update_moving, mean, rstd,
                    scale, shift, nullptr, as_stream(stream));
    UNET_CHECK_LAUNCH("unet_bn_finalize");
    return 0;
}

extern "C" int unet_bn_moments(float* bn_partials, int64_t m, int c, double* moments, unet_stream_t stream) {
    UNET_CHECK_ARG(bn_partials && moments && m > 0 && c > 0, "unet_bn_moments: bad args");
    launch_finalize(bn_partials, m, c, nullptr, nullptr, 0.f, 0.f, nullptr, nullptr, 0, nullptr, nullptr, nullptr,
                    nullptr, moments, as_stream(stream));
    UNET_CHECK_LAUNCH("unet_bn_moments");
    return 0;
}

extern "C" int unet_bn_finalize_moments(const double* moments, int world, int c, const float* gamma,
                                        const float* beta, float eps, float momentum, float* moving_mean,
                                        float* moving_var, int update_moving, float* mean, float* rstd, float* scale,
                                        float* shift, unet_stream_t stream) {
    UNET_CHECK_ARG(moments && world > 0 && c > 0 && scale && shift, "unet_bn_finalize_moments: bad args");
    UNET_CHECK_ARG(!gamma || beta, "unet_bn_finalize_moments: gamma without beta");
    bn_finalize_moments_kernel<<<(unsigned)cdiv(c, 256), 256, 0, as_stream(stream)>>>(
        moments, world, c, gamma, beta, eps, momentum, moving_mean, moving_var, update_moving, mean, rstd, scale,
        shift);
    UNET_CHECK_LAUNCH("unet_bn_finalize_moments");
    return 0;
}

extern "C" int unet_bn_infer_params(const float* gamma, const float* beta, const float* moving_mean,
                                    const float* moving_var, int c, float eps, float* scale, float* shift,
                                    unet_stream_t stream) {
    UNET_CHECK_ARG(scale && shift && c > 0, "unet_bn_infer_params: bad args");
    UNET_CHECK_ARG(!gamma || (beta && moving_mean && moving_var), "unet_bn_infer_params: missing BN tensors");
    bn_infer_kernel<<<(unsigned)cdiv(c, 256), 256, 0, as_stream(stream)>>>(gamma, beta, moving_mean, moving_var, c,
                                                                           eps, scale, shift);
    UNET_CHECK_LAUNCH("unet_bn_infer_params");
    return 0;
}
