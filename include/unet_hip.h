/*
 * unet_hip.h — C-ABI of libunet_hip.so, the MI355X (gfx950) engine for the
 * separable-conv U-Net hot path of planck-epoch/unet-image-segmentation.
 *
 * The reference has no native code and no FFI: every op on the path is an
 * implicit TensorFlow kernel emitted by a Keras layer.  Each entry point below
 * names the Keras layer / reference function it replaces (file:line in the
 * reference).  The reference-side binding a maintainer would add (ctypes) is
 * shown in INTEGRATION.md.
 *
 * Conventions (all entry points):
 *   - tensors are NHWC float32, dense (row stride = channel count), device
 *     memory owned by the caller; nothing here allocates device memory;
 *   - weights use the Keras layouts (see each function);
 *   - every call is asynchronous on `stream` (a hipStream_t; NULL = default);
 *   - return 0 on success, < 0 for an invalid argument, > 0 for a hipError_t;
 *     unet_last_error() gives a thread-local message for the last failure;
 *   - reductions are deterministic (fixed order, no float atomics): the same
 *     inputs give bitwise-identical outputs run to run;
 *   - ops needing scratch take (ws, ws_bytes); query the size with the
 *     matching *_workspace() function.  ws_bytes equal to that answer is
 *     sufficient, a larger value changes no result, and the workspace's
 *     contents before the call do not matter;
 *   - a call writes only inside its outputs, its workspace and the caller-
 *     sized partials buffers; a call that returns < 0 has written nothing;
 *   - pointers are at least 4-byte aligned.  Which operands may stop there
 *     (an element-wise kernel is chosen from the pointer) and which must be
 *     16-byte aligned (refused with < 0 otherwise) is listed in DESIGN.md
 *     section 3.1; 16-byte alignment of everything is always accepted.
 */
#ifndef UNET_HIP_H
#define UNET_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UNET_ABI_VERSION 18

typedef void* unet_stream_t; /* hipStream_t */

/* ---------------------------------------------------------------------------
 * Activation views.  Producers store raw (pre-BatchNorm) conv outputs; a
 * consumer reads the activation it needs through a view, which applies the
 * BatchNormalization affine + ReLU of model/u_net.py:22-25 on load, and
 * optionally MaxPooling2D (u_net.py:69), Concatenate (u_net.py:95-96) and
 * Dropout (u_net.py:77-78, 97-98).  The logical tensor is (n, h, w, c0 + c1).
 * ------------------------------------------------------------------------ */
enum {
    UNET_VIEW_PLAIN = 0,       /* x = src0                                    */
    UNET_VIEW_BNRELU = 1,      /* x = relu(src0 * scale0 + shift0)            */
    UNET_VIEW_POOL_BNRELU = 2, /* x = maxpool2x2(relu(src0*scale0+shift0)),
                                  src0 is (n, 2h, 2w, c0)                     */
    UNET_VIEW_CONCAT = 3       /* x = [src0 (raw, c0) | relu(src1*scale1+shift1) (c1)] */
};

typedef struct unet_view {
    int32_t mode;
    int32_t c0;
    int32_t c1;          /* CONCAT only, else 0 */
    int32_t reserved0;
    const float* src0;
    const float* scale0; /* per-channel, BNRELU / POOL_BNRELU */
    const float* shift0;
    const float* src1;   /* CONCAT: skip tensor (n, h, w, c1) */
    const float* scale1;
    const float* shift1;
    float drop_rate;     /* Dropout on the logical tensor; 0 = off */
    int32_t reserved1;
    uint64_t drop_seed;  /* keep(i) = u(splitmix64(seed + i*golden)) >= rate */
} unet_view;

int unet_abi_version(void);
const char* unet_last_error(void);

/* Cross-stream ordering for a caller that splits the backward over two HIP
 * streams of one device (the reference has no counterpart: TF schedules its
 * own graph).  The event carries no timing and only a device-scope release
 * (hipEventDisableSystemFence): ordering between the streams, not visibility
 * to the host.  unet_stream_wait_stream records `event` on `producer` and
 * makes `waiter` wait for it; the event can be reused at once.              */
int unet_event_create(void** event);
int unet_event_destroy(void* event);
int unet_stream_wait_stream(unet_stream_t waiter, unet_stream_t producer,
                            void* event);

/* Channel-strided copy: dst[r * dst_ld + c] = src[r * src_ld + c] for r < rows, c < cols.
 * The image block's 3 -> 4 channel zero padding (model/u_net.py:58 Input of 3 channels; the pad
 * channel of dst is left as it is) and the Keras-shaped (3, 3, 3, 1) / (1, 1, 3, 64) slices of
 * its padded kernels and their gradients, so no step copy goes through a framework kernel.   */
int unet_copy_strided(const float* src, int64_t rows, int cols, int64_t src_ld, float* dst,
                      int64_t dst_ld, unet_stream_t stream);

/* Split-precision weights: for each segment i (segs[4 i .. 4 i + 3] = source offset, rows,
 * cols, destination offset; host array, offsets in elements), dst + dst_off holds three bf16
 * planes [3][cols][rows] (transposed) with src[r][c] == hi + mid + lo exactly (round-to-nearest
 * bf16 of the value, then of each remainder).  One launch for every pointwise kernel of a step.
 * dst offsets must be multiples of 8 (16-B planes); rows * cols per plane.                  */
#define UNET_SPLIT_MAX_SEGS 64
int unet_split_x3(const float* src, const int64_t* segs, int nseg, unsigned short* dst,
                  unet_stream_t stream);
/* The same split with the planes in the source layout, [3][rows][cols] (ABI 12): the operand
 * layout of the split-precision data-gradient GEMM (unet_pointwise_bwd_data_bnrelu_x3 reads
 * pw_kernel (Cin, Cout) with k = Cout contiguous).                                            */
int unet_split_x3_keep(const float* src, const int64_t* segs, int nseg, unsigned short* dst,
                       unet_stream_t stream);
/* Both layouts in one launch: segs[5 i .. 5 i + 4] = source offset, rows, cols, destination
 * offset, keep (non-zero: [3][rows][cols], else [3][cols][rows]); the train step's one split per
 * weight update (ABI 12).                                                                      */
int unet_split_x3_mixed(const float* src, const int64_t* segs, int nseg, unsigned short* dst,
                        unet_stream_t stream);

/* Writes the logical tensor of a view, out (n, h, w, c0 + c1): the activation relu(bn(z)),
 * its max-pool, or the (dropped-out) concat.  The training path never needs this (consumers
 * read views directly); it serves eager conv_block outputs and inspection.                 */
int unet_view_materialize(const unet_view* x, int n, int h, int w, float* out,
                          unet_stream_t stream);

/* ----- SeparableConv2D(f, 3, padding='same') — model/u_net.py:14-20 --------
 * Depthwise half: y[n,h,w,c] = sum_{i,j<3} x[n,h+i-1,w+j-1,c] * k[i,j,c],
 * zero padding.  dw_kernel is Keras `depthwise_kernel` (3, 3, C, 1).       */
int unet_dwconv3x3_fwd(const unet_view* x, int n, int h, int w,
                       const float* dw_kernel, float* y, unet_stream_t stream);

/* Gradient w.r.t. the view's input.  Routing by view mode:
 *   PLAIN / BNRELU : dx0 (n,h,w,c0) = d(logical x)   (store)
 *   POOL_BNRELU    : dx0 (n,2h,2w,c0) += grad routed to the first max of each
 *                    2x2 window (accumulates: the skip path stored first)
 *   CONCAT         : dx0 (n,h,w,c0) = grad of the upsample half (store),
 *                    dx1 (n,h,w,c1) = grad of the skip half (store)
 * Dropout (if the view has it) is applied to the gradient first.          */
int unet_dwconv3x3_bwd_data(const unet_view* x, int n, int h, int w,
                            const float* dw_kernel, const float* dy,
                            float* dx0, float* dx1, unet_stream_t stream);
/* POOL_BNRELU view (the MaxPooling2D of u_net.py:69 feeding the next encoder
 * block) or BNRELU view (block1 -> block2 of a stage): unet_dwconv3x3_bwd_data
 * plus the BatchNorm-backward partial sums of the view's block, whose da this
 * launch completes (POOL: adds the pooled half of the gradient to the stored
 * skip half, reading the block's raw z for the argmax anyway; BNRELU: writes
 * all of da and reads z once for the ReLU mask): bn_partials[s][0][c] = sum g, [s][1][c] = sum g*xhat over
 * slab s, g = da*[z*scale+shift > 0], xhat = (z-mean)*rstd (mean/rstd NULL when
 * use_batch_norm=False).  Replaces unet_bn_relu_bwd_stats's pass over (da, z);
 * finish with unet_bn_relu_bwd_stats_finish.  _slabs returns the slab count S
 * (bn_partials holds S*2*C floats), 0 if the shape has no such path.          */
int unet_dwconv3x3_bwd_data_bnstats_slabs(const unet_view* x, int n, int h, int w);
/* (bn_partials: unet_bn_stats_partials_size(S, C) bytes, see the finish below) */
int unet_dwconv3x3_bwd_data_bnstats(const unet_view* x, int n, int h, int w,
                                    const float* dw_kernel, const float* dy,
                                    float* dx0, const float* mean,
                                    const float* rstd, float* bn_partials,
                                    unet_stream_t stream);
/* The same for a BNRELU view without dropout (round 6, ABI 12) that ALSO accumulates the
 * layer's depthwise FILTER gradient from the same registers (d_dw[t][c] = sum_q x[q] dy[q - off(t)],
 * x[q] = relu(z sc + sh) from the z the statistics read anyway): per tile a fixed-order [9][C]
 * slab into dw_partials ([S][9][C], S = _slabs(...)); unet_reduce_slabs(dw_partials, S, 9 C,
 * d_dw_kernel) sums them in tile order.  Replaces unet_dwconv3x3_bwd_filter's second pass over
 * dy and the view for such a block (model/u_net.py:14-20, the GradientTape's depthwise gradient). */
int unet_dwconv3x3_bwd_data_bnstats_dwf(const unet_view* x, int n, int h, int w,
                                        const float* dw_kernel, const float* dy, float* dx0,
                                        const float* mean, const float* rstd, float* bn_partials,
                                        float* dw_partials, unet_stream_t stream);
/* out[l] = sum_{s < S} slabs[s * len + l], summed in a fixed order (deterministic); slabs is
 * scratch (overwritten).  The reduction of unet_dwconv3x3_bwd_data_bnstats_dwf's slabs.        */
int unet_reduce_slabs(float* slabs, int S, int64_t len, float* out, unet_stream_t stream);

/* Workspace bytes of unet_dwconv3x3_bwd_filter; the value covers every view of c channels
 * (c = c0 + c1 for a concat view, however the channels are split).                             */
size_t unet_dwconv3x3_bwd_filter_workspace(int n, int h, int w, int c);
/* d_dw_kernel (3,3,C,1) = sum over pixels of x(shifted) * dy (overwrites). */
int unet_dwconv3x3_bwd_filter(const unet_view* x, int n, int h, int w,
                              const float* dy, float* d_dw_kernel,
                              void* ws, size_t ws_bytes, unet_stream_t stream);

/* Pointwise half: z[m, co] = sum_ci y[m, ci] * k[ci, co];  pw_kernel is Keras
 * `pointwise_kernel` (1, 1, Cin, Cout).  If bn_partials != NULL the epilogue
 * also writes per-tile BatchNorm statistics (count-weighted mean and M2 per
 * channel) for unet_bn_finalize.                                            */
size_t unet_bn_partials_size(int64_t m, int c); /* bytes of bn_partials */
int unet_pointwise_fwd(const float* y, int64_t m, int cin, int cout,
                       const float* pw_kernel, float* z, float* bn_partials,
                       unet_stream_t stream);
/* The same with pw_kernel_x3 = unet_split_x3(pw_kernel) ([3][Cout][Cin], unet_sepconv_fwd's planes;
 * ABI 12): the bf16x6 split-precision GEMM of unet_pointwise_bwd_data_bnrelu_x3 where cin % 32 == 0. */
int unet_pointwise_fwd_x3(const float* y, int64_t m, int cin, int cout, const float* pw_kernel,
                          const unsigned short* pw_kernel_x3, float* z, float* bn_partials,
                          unet_stream_t stream);
/* dy[m, ci] = sum_co dz[m, co] * k[ci, co] */
int unet_pointwise_bwd_data(const float* dz, int64_t m, int cin, int cout,
                            const float* pw_kernel, float* dy,
                            unet_stream_t stream);
size_t unet_pointwise_bwd_filter_workspace(int64_t m, int cin, int cout);
/* d_pw_kernel[ci, co] = sum_m y[m, ci] * dz[m, co] (overwrites) */
int unet_pointwise_bwd_filter(const float* y, const float* dz, int64_t m,
                              int cin, int cout, float* d_pw_kernel,
                              void* ws, size_t ws_bytes, unet_stream_t stream);
/* Fused SeparableConv2D: depthwise 3x3 of the view -> pointwise 1x1 (+ BatchNorm partials as
 * unet_pointwise_fwd), the depthwise result never leaving the chip except as the optional `y`
 * (needed by the pointwise weight gradient in training; NULL for inference).  Supported when
 * unet_sepconv_fwd_supported() says so (h % 8 == 0, w % 16 == 0, channels % 4 == 0).     */
int unet_sepconv_fwd_supported(const unet_view* x, int n, int h, int w, int cout);
int unet_sepconv_fwd(const unet_view* x, int n, int h, int w, const float* dw_kernel,
                     int cout, const float* pw_kernel,
                     const unsigned short* pw_kernel_x3, float* y, float* z,
                     float* bn_partials, float* z_pool_sel, const float* gamma,
                     unet_stream_t stream);
/* pw_kernel_x3 (optional): pw_kernel split by unet_split_x3 ([3][Cout][Cin] bf16 planes).  With
 * it the register-A kernel runs its split-precision MFMA variant where it exists (channels
 * % 16 == 0, no max-pool view): every product of the pointwise GEMM is formed from the three
 * bf16 parts of both operands, x == hi + mid + lo exactly, and summed as the six significant
 * part products on v_mfma_f32_32x32x16_bf16 with fp32 accumulation (error ~2^-23 |a b| per
 * product, below fp32 accumulation rounding: DESIGN.md "Split-precision MFMA").              */
/* z_pool_sel (optional, (N, h/2, w/2, cout)): the encoder stage's MaxPooling2D((2,2))
 * (model/u_net.py:69) prepared for its consumer: per 2x2 window of z and channel, the raw
 * value the max-pool of relu(z * scale + shift) selects -- the window max where gamma >= 0,
 * the min where gamma < 0 (gamma = the block's BN gamma; NULL = no BatchNorm: max).  scale has
 * gamma's sign and fmaf / relu are monotone, so a BNRELU view of z_pool_sel reads exactly the
 * pooled activation, one value per output pixel instead of four.  Written by the kernel's
 * epilogue (register-A schedule) or by unet_pool_select after it.  The max-pool BACKWARD still
 * routes through z (first maximum of the window): POOL_BNRELU views of z.
 * unet_pool_select: h and w even; c % 4 == 0 reads channel quads (z, out, gamma 16-B aligned),
 * any other c one channel per thread.                                                       */
int unet_pool_select(const float* z, int n, int h, int w, int c, const float* gamma,
                     float* out, unet_stream_t stream);
/* Kernel schedule of unet_sepconv_fwd (process-wide; returns the previous value, < 0 on a bad
 * value).  AUTO: the register-A kernel (each lane computes the depthwise output straight in the
 * MFMA operand layout) for BN+ReLU / concat / plain views of >= 64 input and output channels
 * and for max-pool views of >= 64 inputs and 64..128 outputs; the LDS-A-tile kernel otherwise
 * (max-pool views of > 128 outputs: its 256-wide tile pools each halo element once for all
 * columns).  TILE / RK force one (RK fails with -1 where it does not exist): both are
 * parity-tested (tests/test_ops_gpu.py).  With pw_kernel_x3, 64 / 128 input and output channels and
 * a plain / BN+ReLU / concat view, RK runs the register-A kernel PERSISTENT over pixel tiles
 * (sepconv_px.hip: a block walks a run of tiles as one stream of k-stages, the next stages' loads
 * in flight across tile boundaries); AUTO does so only where that measured faster inside the train
 * step (128 outputs from 64 inputs or with z_pool_sel); RK1 forces the one-tile-per-block
 * register-A kernel (same products, same per-tile statistics partials up to the order of the
 * 4-wave combine).
 * Without pw_kernel_x3 the results are identical: both
 * form each output as the same k-ordered fmaf chain.  With pw_kernel_x3 the register-A kernel
 * runs its split-precision (bf16x6 MFMA) variant, whose summation order differs (results within
 * fp32 rounding, not bitwise), while TILE ignores the split planes and gives the fmaf-chain
 * results: the output then depends on the schedule.                                          */
enum { UNET_SEPCONV_AUTO = 0, UNET_SEPCONV_TILE = 1, UNET_SEPCONV_RK = 2, UNET_SEPCONV_RK1 = 3 };
int unet_sepconv_set_schedule(int schedule);

/* Both weight gradients of a SeparableConv2D (model/u_net.py:14-20; the pixel reductions of
 * Keras' implicit backward, scripts/train.py:308) in one pass WITHOUT the depthwise output y:
 *   d_pw_kernel[ci, co] = sum_m y[m, ci] * dz[m, co],  y = depthwise3x3(view x) recomputed
 *   d_dw_kernel[t, ci]  = sum_m x[m + off(t), ci] * dy[m, ci]
 * so the training forward need not store y (unet_sepconv_fwd with y = NULL).  Replaces
 * unet_pointwise_bwd_filter over a stored y + unet_dwconv3x3_bwd_filter; both overwritten.
 * Supported (unet_sepconv_bwd_filter_supported) for the HBM-bound 64-output blocks of the
 * widest level: input channels % 64 == 0, 64 output channels, PLAIN / BNRELU / CONCAT view,
 * h % 8 == 0, w % 16 == 0; dy / dz / the depthwise kernel / view sources 16-B aligned.       */
int unet_sepconv_bwd_filter_supported(const unet_view* x, int n, int h, int w, int cout);
size_t unet_sepconv_bwd_filter_workspace(int n, int h, int w, int cin, int cout);
int unet_sepconv_bwd_filter(const unet_view* x, int n, int h, int w, const float* dw_kernel,
                            const float* dy, const float* dz, int cout, float* d_dw_kernel,
                            float* d_pw_kernel, void* ws, size_t ws_bytes, unet_stream_t stream);
/* The same pass for a 64-output block ALSO doing the block's BatchNorm + ReLU backward and
 * pointwise data gradient (model/u_net.py:14-25, the GradientTape of scripts/train.py:308): per
 * pixel tile dz = scale (g - p - (z - mu) q), g = da [z scale + shift > 0] with coef = (mu, p, q)
 * from unet_bn_relu_bwd_stats(_finish) (exactly unet_pointwise_bwd_data_bnrelu's dz), then
 * dy = dz . pw_kernel^T (written out, for the depthwise data gradient), d_pw_kernel = y^T dz and
 * d_dw_kernel as above; dz never goes to memory (bytes: da, z, the input view, dy).  No dropout
 * on either side.  Workspace as unet_sepconv_bwd_filter.
 * da may be NULL when da_dlogit (m floats) and da_kernel (cout floats) are given: the binary
 * head's gradient is rank one, da[m][c] = da_dlogit[m] * da_kernel[c] (unet_head_bwd_bnstats'
 * dlogit output and the head's 1x1 kernel, model/u_net.py:105-112), formed on load with the
 * same product the head would have stored (ABI 10).                                          */
int unet_sepconv_bwd_fused(const unet_view* x, int n, int h, int w, const float* dw_kernel,
                           const float* pw_kernel, const float* da, const float* da_dlogit,
                           const float* da_kernel, const float* z,
                           const float* scale, const float* shift, const float* coef, int cout,
                           float* dy, float* d_dw_kernel, float* d_pw_kernel, void* ws,
                           size_t ws_bytes, unet_stream_t stream);

/* ----- BatchNormalization() — model/u_net.py:22-23 (Keras defaults:
 * momentum 0.99, epsilon 1e-3, biased batch variance for both the output
 * and the moving-variance update).  Training: reduces bn_partials into the
 * batch mean / variance, writes mean, rstd = 1/sqrt(var+eps), and the affine
 * scale = gamma*rstd, shift = beta - mean*scale consumed by views; updates
 * moving stats when update_moving != 0.  gamma == NULL means
 * use_batch_norm=False: scale = 1, shift = beta (the sepconv bias).
 * One launch: 64-partial chunk sums, then the last block of each 64-channel
 * column to finish sums the chunk rows.  The tail of bn_partials (past the
 * per-tile partials) holds the chunk rows and ceil(c/64) arrival counters:
 * the buffer must hold unet_bn_partials_size bytes and its counters must be
 * zero before the first call (allocate it zeroed once; calls leave them
 * zero; the statistics producers never write past the per-tile partials).   */
int unet_bn_finalize(float* bn_partials, int64_t m, int c,
                     const float* gamma, const float* beta, float eps,
                     float momentum, float* moving_mean, float* moving_var,
                     int update_moving, float* mean, float* rstd,
                     float* scale, float* shift, unet_stream_t stream);
/* SyncBN under data parallelism (SURVEY §8(e) option; off by default: the reference's
 * tf.distribute default, and Keras BatchNormalization(synchronized=False), normalise each
 * replica over its own shard).  unet_bn_moments reduces this replica's partials (as
 * unet_bn_finalize does, same counters) to a record of 1 + 2c doubles: (count, mean[c], M2[c]);
 * the caller gathers the replicas' records ([world][1 + 2c], rank order) and
 * unet_bn_finalize_moments combines them in rank order (Chan's parallel formula, double) and
 * finalizes exactly as unet_bn_finalize with the global-batch mean / biased variance.  Every
 * replica combining the same gathered records ends with identical statistics.
 * Backward: unet_bn_bwd_coef forms coef = (mean, S1/m, rstd*S2/m) from the all-reduced sums
 * sums[0..c) = sum g, sums[c..2c) = sum g*xhat over all replicas (m = the global pixel count);
 * the replica's own dgamma / dbeta stay its local sums (the gradient all-reduce averages them). */
int unet_bn_moments(float* bn_partials, int64_t m, int c, double* moments, unet_stream_t stream);
int unet_bn_finalize_moments(const double* moments, int world, int c, const float* gamma,
                             const float* beta, float eps, float momentum, float* moving_mean,
                             float* moving_var, int update_moving, float* mean, float* rstd,
                             float* scale, float* shift, unet_stream_t stream);
int unet_bn_bwd_coef(const float* sums, int64_t m, int c, int use_bn, const float* mean,
                     const float* rstd, float* coef, unet_stream_t stream);

/* Inference: scale/shift from the moving statistics. */
int unet_bn_infer_params(const float* gamma, const float* beta,
                         const float* moving_mean, const float* moving_var,
                         int c, float eps, float* scale, float* shift,
                         unet_stream_t stream);
/* Backward of a = dropout(relu(z*scale+shift)):
 *   g = da * keep/(1-rate) * [z*scale+shift > 0]
 *   dbeta = sum g, dgamma = sum g*xhat (xhat = (z-mean)*rstd)
 *   dz = scale*(g - dbeta/M - xhat*dgamma/M)    (use_bn != 0)
 *   dz = g, dbeta = sum g, dgamma untouched       (use_bn == 0, bias grad)  */
size_t unet_bn_relu_bwd_workspace(int64_t m, int c);
int unet_bn_relu_bwd(const float* da, const float* z, int64_t m, int c,
                     const float* mean, const float* rstd, const float* scale,
                     const float* shift, int use_bn, float drop_rate,
                     uint64_t drop_seed, float* dgamma, float* dbeta,
                     float* dz, void* ws, size_t ws_bytes,
                     unet_stream_t stream);
/* Statistics half of unet_bn_relu_bwd (same workspace): dgamma / dbeta and the
 * per-channel coefficients coef[3c] = (mean, dbeta/M, rstd*dgamma/M) (zeros when
 * use_bn == 0) with which unet_pointwise_bwd_data_bnrelu forms dz on load, so dz
 * never takes a separate HBM pass.  Same reference lines as unet_bn_relu_bwd.     */
int unet_bn_relu_bwd_stats(const float* da, const float* z, int64_t m, int c,
                           const float* mean, const float* rstd,
                           const float* scale, const float* shift, int use_bn,
                           float drop_rate, uint64_t drop_seed, float* dgamma,
                           float* dbeta, float* coef, void* ws, size_t ws_bytes,
                           unet_stream_t stream);
/* Finish of the statistics from S producer-side partial slabs ([S][2][c],
 * fixed-order double reduction): the outputs of unet_bn_relu_bwd_stats, in one
 * launch (64-slab chunk sums; the last block of each channel range to finish
 * sums the chunk rows).  The partials buffer holds
 * unet_bn_stats_partials_size(S, c) bytes: the slabs, the chunk rows, then
 * ceil(c/64) arrival counters that must be zero before the first call --
 * allocate the buffer zeroed once; every call leaves them zero again.        */
size_t unet_bn_stats_partials_size(int S, int c);
int unet_bn_relu_bwd_stats_finish(float* partials, int S, int64_t m, int c,
                                  const float* mean, const float* rstd,
                                  int use_bn, float* dgamma, float* dbeta,
                                  float* coef, unet_stream_t stream);
/* Pointwise data gradient of a conv_block whose output went through BN + ReLU
 * (+ dropout): dz = scale*(g - coef_p - (z - coef_mu)*coef_q),
 * g = da * keep/(1-rate) * [z*scale+shift > 0], is formed while loading the GEMM
 * operand; dy[m, ci] = sum_co dz[m, co] * k[ci, co].  If dz != NULL the formed dz
 * is also stored (the pointwise weight gradient reads it).  cin, cout % 4 == 0.
 * Replaces the backward of model/u_net.py:20-25 (SeparableConv2D pointwise ->
 * BatchNormalization -> ReLU) for the data path.                                 */
int unet_pointwise_bwd_data_bnrelu(const float* da, const float* z, int64_t m,
                                   int cin, int cout, const float* pw_kernel,
                                   const float* scale, const float* shift,
                                   const float* coef, float drop_rate,
                                   uint64_t drop_seed, float* dy, float* dz,
                                   unet_stream_t stream);
/* The same with pw_kernel_x3 = unet_split_x3_keep(pw_kernel) ([3][Cin][Cout] bf16 planes, 16-B
 * aligned; ABI 12): where cout % 32 == 0 the GEMM runs the six significant bf16 part products
 * of both operands on v_mfma_f32_32x32x16_bf16 with fp32 accumulation (the A operand, dz, is
 * split exactly as it is formed), the split-precision form of unet_sepconv_fwd's pw_kernel_x3:
 * fp32-accurate (relative error ~2^-23 per product), not bitwise equal to the fp32-MFMA route.
 * pw_kernel is still read where the route does not apply.                                   */
int unet_pointwise_bwd_data_bnrelu_x3(const float* da, const float* z, int64_t m,
                                      int cin, int cout, const float* pw_kernel,
                                      const unsigned short* pw_kernel_x3,
                                      const float* scale, const float* shift,
                                      const float* coef, float drop_rate,
                                      uint64_t drop_seed, float* dy, float* dz,
                                      unet_stream_t stream);

/* The image block (enc1_block1 over the 3-channel input zero-padded to 4):
 * unet_pointwise_bwd_data_bnrelu without dropout, cin == 4, cout 32 or 64,
 * that also writes the pointwise kernel gradient d_pw_kernel[ci][co] =
 * sum_m y[m,ci] dz[m,co] (y: the depthwise output, m x 4) from the dz it forms
 * on load, so dz is never stored (one streaming pass over da, z, y).
 * Workspace: _workspace(m, cin, cout) bytes (0: shape not supported).      */
size_t unet_pointwise_bwd_data_bnrelu_wgrad_workspace(int64_t m, int cin,
                                                      int cout);
int unet_pointwise_bwd_data_bnrelu_wgrad(const float* da, const float* z,
                                         int64_t m, int cin, int cout,
                                         const float* pw_kernel,
                                         const float* scale, const float* shift,
                                         const float* coef, const float* y,
                                         float* dy, float* d_pw_kernel,
                                         void* ws, size_t ws_bytes,
                                         unet_stream_t stream);

/* The image block's two weight gradients in ONE streaming pass (its data gradient is
 * never needed): as unet_pointwise_bwd_data_bnrelu_wgrad, but the dy it forms per
 * pixel is not stored, it is contracted at once with the pixel's 3x3 neighbourhood
 * of x into the depthwise kernel gradient.  x: the (n, h, w, 4) input the forward
 * read (channels past wcin zero), pw_kernel (4, cout) padded the same way.  Outputs
 * in the Keras shapes of the wcin-channel layer: d_dw_kernel (3, 3, wcin, 1),
 * d_pw_kernel (1, 1, wcin, cout) -- both overwritten.  cout 32 or 64.
 * Replaces the backward of the first SeparableConv2D (model/u_net.py:14-20 for
 * the first conv_block, u_net.py:62) for its weights.
 * Workspace: _workspace(n, h, w, cout) bytes (0: shape not supported).       */
size_t unet_image_block_bwd_wgrad_workspace(int n, int h, int w, int cout);
int unet_image_block_bwd_wgrad(const float* x, int n, int h, int w, int wcin,
                               int cout, const float* pw_kernel,
                               const float* scale, const float* shift,
                               const float* coef, const float* da,
                               const float* z, const float* y,
                               float* d_dw_kernel, float* d_pw_kernel,
                               void* ws, size_t ws_bytes,
                               unet_stream_t stream);

/* ----- Conv2DTranspose(f, 2, strides=2, padding='same') — u_net.py:88-94 --
 * out[n, 2i+a, 2j+b, co] = bias[co] + sum_ci x[n,i,j,ci] * k[a,b,co,ci];
 * kernel is Keras (2, 2, Cout, Cin), x a view of (n, h, w, Cin).           */
int unet_conv_transpose2x2_fwd(const unet_view* x, int n, int h, int w,
                               int cout, const float* kernel,
                               const float* bias, float* out,
                               unet_stream_t stream);
/* The same with kernel_x3 = unet_split_x3_keep(kernel as (4 cout, cin)) (ABI 12): the bf16x6
 * split-precision GEMM of unet_pointwise_bwd_data_bnrelu_x3 where cin % 32 == 0.            */
int unet_conv_transpose2x2_fwd_x3(const unet_view* x, int n, int h, int w, int cout,
                                  const float* kernel, const unsigned short* kernel_x3,
                                  const float* bias, float* out, unet_stream_t stream);
size_t unet_conv_transpose2x2_bwd_workspace(int n, int h, int w, int cin,
                                            int cout);
/* dx (n,h,w,Cin) = grad w.r.t. the view output (NULL: skip); dkernel, dbias
 * overwrite (both NULL: data gradient only, so the weight gradient can be a
 * separate call with dx = NULL, e.g. on another stream). */
int unet_conv_transpose2x2_bwd(const unet_view* x, int n, int h, int w,
                               int cout, const float* kernel,
                               const float* dout, float* dx, float* dkernel,
                               float* dbias, void* ws, size_t ws_bytes,
                               unet_stream_t stream);
/* Data gradient only, for a BNRELU view (the decoder block2 / bottleneck
 * output feeding the upsample, u_net.py:88): dx is then the whole da of the
 * view's block, so the GEMM epilogue also emits that block's BatchNorm-backward
 * partials in the unet_dwconv3x3_bwd_data_bnstats format (S = _slabs(...)
 * slabs, one per row tile: 128 rows, or 64 rows when the 128-row grid would
 * hold <= 256 tiles of 64 columns (round 5); always size and finish with the
 * S the query returns; mean/rstd NULL when use_batch_norm=False; finish with
 * unet_bn_relu_bwd_stats_finish).  Replaces unet_bn_relu_bwd_stats's separate
 * pass over (da, z).  A view with dropout (the bottleneck's, u_net.py:77-78;
 * round 5, no signature change): the partials are those of g = da * mask, as
 * unet_bn_relu_bwd_stats(..., drop_rate, drop_seed, ...) forms them; dx stays
 * the gradient w.r.t. the dropout output.  _slabs: 0 if the view or shape has
 * no such path.                                                              */
int unet_conv_transpose2x2_bwd_data_bnstats_slabs(const unet_view* x, int n,
                                                  int h, int w, int cout);
int unet_conv_transpose2x2_bwd_data_bnstats(const unet_view* x, int n, int h,
                                            int w, int cout,
                                            const float* kernel,
                                            const float* dout, float* dx,
                                            const float* mean,
                                            const float* rstd,
                                            float* bn_partials,
                                            unet_stream_t stream);
/* The same with kernel_x3t = unet_split_x3(kernel as (4 cout, cin)) ([3][cin][4 cout] planes,
 * ABI 12): the bf16x6 GEMM where cout % 8 == 0 and the partials are per 128-row tile.      */
int unet_conv_transpose2x2_bwd_data_bnstats_x3(const unet_view* x, int n, int h, int w, int cout,
                                               const float* kernel, const unsigned short* kernel_x3t,
                                               const float* dout, float* dx, const float* mean,
                                               const float* rstd, float* bn_partials,
                                               unet_stream_t stream);

/* ----- Output layer Conv2D(ncls, 1, activation) — u_net.py:105-112 --------
 * prob = sigmoid(x.k + b) (ncls == 1) or softmax over channels.            */
int unet_head_fwd(const unet_view* x, int n, int h, int w, int ncls,
                  const float* kernel, const float* bias, float* prob,
                  unet_stream_t stream);

/* ----- dice_coef / iou_coef / dice_loss — utils/metrics.py:6-62,
 * utils/loss.py:9-48.  Per (batch, channel) sums over H, W:
 * sums[b][c] = {sum t*p, sum t, sum p};  result = {1 - mean dice,
 * mean dice, mean iou}.  smooth = K.epsilon() = 1e-7 in the reference.     */
enum { UNET_LOSS_DICE = 0, UNET_LOSS_IOU = 1 };
size_t unet_dice_workspace(int n, int64_t hw, int ncls);
int unet_dice_fwd(const float* y_true, const float* y_pred, int n,
                  int64_t hw, int ncls, float smooth, float* sums,
                  float* result, void* ws, size_t ws_bytes,
                  unet_stream_t stream);
/* Backward of (1 - mean dice) [or 1 - mean iou] through the head
 * activation and the 1x1 conv: dx (n,h,w,Cin) grad w.r.t. the head input
 * view; dkernel (1,1,Cin,ncls), dbias (ncls) overwrite.  loss_scale (> 0)
 * multiplies the loss gradient: 1 for the reference's single-process step;
 * n_local * world / n_global for a data-parallel shard, so that the summed
 * all-reduce times 1/world is the gradient of the global-batch mean.       */
size_t unet_head_bwd_workspace(int n, int h, int w, int cin, int ncls);
int unet_head_bwd(const unet_view* x, int n, int h, int w, int ncls,
                  const float* kernel, const float* prob,
                  const float* y_true, const float* sums, float smooth,
                  int loss_kind, float loss_scale, float* dx, float* dkernel,
                  float* dbias,
                  void* ws, size_t ws_bytes, unet_stream_t stream);
/* Head on a BNRELU view (binary; or multi-class with <= 24 classes and
 * Cin in {4, 8, 16, 32, 64}, one fused pass; other multi-class shapes: the
 * _slabs query returns 0 and the call is refused -- use unet_head_bwd plus
 * unet_bn_relu_bwd_stats): unet_head_bwd plus the BatchNorm-backward
 * partial sums of the head input's block (dx is all of its da; bn_partials
 * layout and finish as unet_dwconv3x3_bwd_data_bnstats).  _slabs: S, or 0.
 * Binary only: dx may be NULL when dlogit (m floats) is given: dx = dlogit
 * (x) kernel is rank one, so only dL/dlogit per pixel is stored and the
 * consumer forms dx on load (unet_sepconv_bwd_fused's da_dlogit; ABI 10).   */
int unet_head_bwd_bnstats_slabs(const unet_view* x, int n, int h, int w, int ncls);
int unet_head_bwd_bnstats(const unet_view* x, int n, int h, int w, int ncls,
                          const float* kernel, const float* prob,
                          const float* y_true, const float* sums, float smooth,
                          int loss_kind, float loss_scale, float* dx,
                          float* dlogit, float* dkernel, float* dbias,
                          const float* mean, const float* rstd,
                          float* bn_partials, void* ws, size_t ws_bytes,
                          unet_stream_t stream);

/* ----- keras.metrics.MeanIoU(num_classes) — scripts/train.py:231,
 * scripts/benchmark.py:237,269.  Confusion counts (rows = true, cols =
 * pred) accumulate into `confusion` (num_classes^2 uint64).  threshold < 0:
 * Keras cast semantics (float -> int64 truncation, as in training on raw
 * probabilities); threshold >= 0: pred = (p > threshold) (benchmark.py:260).
 * Labels outside [0, num_classes) are skipped.                             */
int unet_meaniou_update(const float* y_true, const float* y_pred,
                        int64_t count, int num_classes, float threshold,
                        uint64_t* confusion, unet_stream_t stream);

/* ----- keras.optimizers.AdamW — scripts/train.py:226 (Keras 3 update):
 *   p -= p*wd*lr;  g *= grad_scale;  m += (g-m)(1-b1);  v += (g^2-v)(1-b2);
 *   p -= m*alpha / (sqrt(v) + eps),  alpha = lr*sqrt(1-b2^t)/(1-b1^t).      */
int unet_adamw_step(float* param, const float* grad, float* m, float* v,
                    int64_t count, float lr, float weight_decay, float beta1,
                    float beta2, float eps, float alpha, float grad_scale,
                    unet_stream_t stream);

/* ----- Frozen half-precision inference (ABI 13) ----------------------------------------------
 * The deployment step of the reference (scripts/tensorflow_lite/convert_to_tflite.py --float16):
 * a trained model frozen into a half-precision inference artefact.  BatchNormalization
 * (model/u_net.py:22-23) is folded into the pointwise weights on the host (unet_amd/frozen.py:
 * pw' = pointwise_kernel * gamma / sqrt(moving_variance + eps), bias' = beta - moving_mean * scale),
 * so a conv_block is depthwise 3x3 -> pointwise -> + bias' -> ReLU.  Activations are NHWC fp16
 * (passed as unsigned short), dense, 16-byte aligned, and are stored ALREADY ACTIVATED: no
 * BN / ReLU / max-pool views exist on this path.  Products run on v_mfma_f32_32x32x16_f16 with fp32
 * accumulators.  Rounding to fp16 (nearest even) happens at exactly: the folded pointwise and
 * upsample kernels (host), each block's depthwise output, each block's output after bias + ReLU,
 * each upsample's output after bias.  Everything else (the image, the image block, depthwise
 * sums, accumulators, biases, the head) is fp32.                                               */
enum { UNET_F16_VIEW_PLAIN = 0, /* x = src0 (n, h, w, c0)                     */
       UNET_F16_VIEW_CONCAT = 1 /* x = [src0 (c0) | src1 (c1)] (u_net.py:95-96) */ };
typedef struct unet_f16_view {
    int32_t mode;
    int32_t c0;          /* multiple of 16 */
    int32_t c1;          /* CONCAT only (multiple of 16), else 0 */
    int32_t reserved0;
    const unsigned short* src0;
    const unsigned short* src1;
} unet_f16_view;

/* The image block (enc1_block1, model/u_net.py:62) on the caller's UNPADDED fp32 image
 * (n, h, w, cin <= 4): out (n, h, w, cout) fp16 = relu(depthwise3x3(x) . pw_folded + bias), all
 * in fp32 up to the output rounding.  dw_kernel (3, 3, cin, 1), pw_folded (cin, cout) fp32,
 * cout % 8 == 0.                                                                               */
int unet_f16_image_block(const float* x, int n, int h, int w, int cin, const float* dw_kernel,
                         int cout, const float* pw_folded, const float* bias,
                         unsigned short* out, unet_stream_t stream);
/* A folded conv_block (model/u_net.py:5-26): out (n, h, w, cout) fp16 =
 * relu(fp16(depthwise3x3(x)) . pw_t^T + bias).  dw_kernel is the Keras (3, 3, C, 1) fp32 kernel,
 * C = c0 + c1; pw_t the folded pointwise kernel as fp16 [cout][C] (k contiguous); bias fp32;
 * cout % 32 == 0.  out_pool (optional, (n, h/2, w/2, cout), h and w even): MaxPooling2D((2,2))
 * (u_net.py:69) of out, written by the same launch.  route selects how taps are fetched:
 * 0 = auto, 1 = rows (any shape: taps from global memory under bounds predicates), 2 = tile
 * (8 x 16-pixel tiles with an fp16 halo in LDS; needs h % 8 == 0 and w % 16 == 0, refused
 * otherwise); auto takes tile where it applies.  Both give bitwise the same result.           */
int unet_f16_sepconv(const unet_f16_view* x, int n, int h, int w, const float* dw_kernel,
                     int cout, const unsigned short* pw_t, const float* bias,
                     unsigned short* out, unsigned short* out_pool, int route,
                     unet_stream_t stream);
/* Conv2DTranspose(f, 2, strides=2) (u_net.py:88-94) on fp16: x (n, h, w, cin), kernel the Keras
 * (2, 2, cout, cin) layout rounded to fp16, bias fp32; out (n, 2h, 2w, cout) fp16 = x . k + bias
 * (no activation).  cin % 16 == 0, cout % 8 == 0.                                              */
int unet_f16_conv_transpose2x2(const unsigned short* x, int n, int h, int w, int cin, int cout,
                               const unsigned short* kernel, const float* bias,
                               unsigned short* out, unet_stream_t stream);
/* Output layer (u_net.py:105-112) on an fp16 input (n, h, w, cin), cin % 8 == 0: fp32 kernel
 * (1, 1, cin, ncls) and bias, fp32 prob (n, h, w, ncls) = sigmoid (ncls == 1) or softmax.      */
int unet_f16_head(const unsigned short* x, int n, int h, int w, int cin, int ncls,
                  const float* kernel, const float* bias, float* prob, unet_stream_t stream);

/* ----- Frozen int8 inference (ABI 14) --------------------------------------------------------
 * The reference converter's next mode (int8 with a representative dataset): the folded network
 * with one-byte activations and v_mfma_i32_32x32x32_i8 products.  Scales come from a calibration
 * run (unet_amd/frozen.py: collect_ranges, quantize_weights).  THE ARITHMETIC CONTRACT, which the
 * kernels and the test emulator (tests/i8_emulation.py) both implement exactly:
 *
 * Storage.  NHWC bytes, dense, 16-byte aligned.  Post-ReLU activations (every conv block's output
 * and its max-pool) are uint8, x = s q, q in [0, 255]; upsample outputs (signed) are int8, q in
 * [-127, 127].  Spatial padding is q = 0 in both types.  Scales: s = max|.| / 255 (uint8) or / 127
 * (int8) over the calibration set, s = 1 where the maximum is 0.
 *
 * Conv block.  taps[t][c] = dw[t][c] s_in[c] / s_y in fp32 (host; s_in is per input channel, so a
 * concat of an int8 half and a uint8 half with different scales needs no rescaling pass).
 *   a = 0; for t = 0..8: a = fmaf((float)x_q[t][c], taps[t][c], a)
 *   y_q = clamp(rintf(a), -127, 127) as int8                          (the A operand)
 *   B = the folded pointwise kernel as int8, per-output-channel scale s_w[co] = max|pw'[:, co]| / 127
 *       (1 where the column is all zero); acc is int32, exact
 *   v = fmaf((float)acc, mult[co], bias_q[co]);  q_out = clamp(rintf(v), 0, 255)
 * with mult = s_y s_w[co] / s_out and bias_q = bias[co] / s_out computed in float64 on the host and
 * rounded to fp32.  The clamp is the ReLU; the max-pool is the max of the four q_out.
 *
 * Upsample (Conv2DTranspose 2x2).  A = the uint8 input XOR 0x80 (q - 128 as int8); B = the kernel as
 * int8 with one scale per column (a, b, co); colsum[col] = sum_k B[col][k] in int32 (host).
 *   acc32 = acc + 128 colsum[col]  (int32);  v = fmaf((float)acc32, mult[col], bias_q[co])
 *   q = clamp(rintf(v), -127, 127)
 * (float)acc32 is the int32 -> fp32 conversion, round to nearest even: at cin = 1024 |acc32| can
 * exceed 2^24, which is allowed and part of the contract.
 *
 * Image block (enc1_block1).  fp32 input and arithmetic as unet_f16_image_block;
 * q = clamp(rintf(relu(z) / s_out), 0, 255).
 * Head.  Reads uint8; fp32 kernel with the input scale folded in on the host; fp32 probabilities. */
enum { UNET_I8_VIEW_PLAIN = 0, /* x = src0 (n, h, w, c0)                     */
       UNET_I8_VIEW_CONCAT = 1 /* x = [src0 (c0) | src1 (c1)] (u_net.py:95-96) */ };
typedef struct unet_i8_view {
    int32_t mode;
    int32_t c0;          /* CONCAT: a multiple of 16; c0 + c1 is a multiple of 32 */
    int32_t c1;          /* CONCAT only, else 0 */
    int32_t signed0;     /* src0 holds int8 (nonzero) or uint8 (0) */
    int32_t signed1;     /* the same for src1 */
    int32_t reserved0;
    const void* src0;
    const void* src1;
} unet_i8_view;

/* The image block on the caller's unpadded fp32 image (n, h, w, cin <= 4): out (n, h, w, cout)
 * uint8 with scale out_scale.  dw_kernel (3, 3, cin, 1), pw_folded (cin, cout), bias fp32;
 * cout % 32 == 0.                                                                             */
int unet_i8_image_block(const float* x, int n, int h, int w, int cin, const float* dw_kernel,
                        int cout, const float* pw_folded, const float* bias, float out_scale,
                        unsigned char* out, unet_stream_t stream);
/* A quantised conv_block: taps fp32 [9][C], C = c0 + c1; pw_q int8 [cout][C] (k contiguous); mult and
 * bias_q fp32 [cout]; out (n, h, w, cout) uint8; out_pool (optional, h and w even) its 2x2 max from
 * the same launch.  C and cout must be multiples of 32 and a concat's c0 a multiple of 16; anything
 * else is refused.  route as unet_f16_sepconv (0 auto, 1 rows, 2 tile; bitwise the same result). */
int unet_i8_sepconv(const unet_i8_view* x, int n, int h, int w, const float* taps, int cout,
                    const signed char* pw_q, const float* mult, const float* bias_q,
                    unsigned char* out, unsigned char* out_pool, int route, unet_stream_t stream);
/* Conv2DTranspose(f, 2, strides=2) on a uint8 input (n, h, w, cin): kernel_q int8 in the Keras
 * (2, 2, cout, cin) layout, colsum int32 and mult fp32 per column [4 cout], bias_q fp32 [cout];
 * out (n, 2h, 2w, cout) int8.  cin and cout multiples of 32.                                   */
int unet_i8_conv_transpose2x2(const unsigned char* x, int n, int h, int w, int cin, int cout,
                              const signed char* kernel_q, const int32_t* colsum,
                              const float* mult, const float* bias_q, signed char* out,
                              unet_stream_t stream);
/* Output layer on a uint8 input (n, h, w, cin), cin % 8 == 0: fp32 kernel (1, 1, cin, ncls) with the
 * input scale folded in, fp32 bias, fp32 prob = sigmoid (ncls == 1) or softmax.                */
int unet_i8_head(const unsigned char* x, int n, int h, int w, int cin, int ncls,
                 const float* kernel, const float* bias, float* prob, unet_stream_t stream);

/* ----- Device-side image pipeline (ABI 15) ---------------------------------------------------
 * The CLIs' image steps around the forward, which the reference does with cv2 on the host:
 * scripts/inference.py:105-108 and scripts/benchmark.py:105 (cv2.resize of the decoded image to
 * the model size, INTER_LINEAR, then / 255.0), and scripts/inference.py:147-160 (cv2.resize of the
 * probability map back to the image's size, INTER_LINEAR, then > threshold -> 255).
 *
 * Sampling coordinates come from the host (unet_amd/imageproc.py: linear_coords, float64, half-pixel
 * centres with edge clamping), one table per axis with one entry per OUTPUT row / column:
 * source indices i0 <= i1 and the fp32 weight of i1.  The same function feeds the NumPy path, so
 * the two cannot drift apart.
 *
 * THE ARITHMETIC CONTRACT, every operation rounded to fp32 and none contracted into an fma (this
 * object is built with -ffp-contract=off), for the four taps a = s[y.i0][x.i0], b = s[y.i0][x.i1],
 * c = s[y.i1][x.i0], d = s[y.i1][x.i1]:
 *   top = a + (b - a) * x.frac;  bot = c + (d - c) * x.frac;  out = top + (bot - top) * y.frac
 * which is bitwise what resize_linear (unet_amd/imageproc.py) computes in NumPy.                 */
typedef struct unet_lerp_coord {
    int32_t i0;       /* first source index, 0 <= i0 < n_in                 */
    int32_t i1;       /* second source index, min(i0 + 1, n_in - 1)         */
    float frac;       /* weight of i1, in [0, 1)                            */
    int32_t reserved; /* 0; keeps an entry one 16-byte load                 */
} unet_lerp_coord;

/* uint8 image (sh, sw, c), c = 1 or 3, densely packed (rows at any byte alignment) -> fp32
 * (oh, ow, c) at dst: s = (float)byte / 255.0f (correctly rounded), then the contract above per
 * channel.  reverse_channels != 0 reads source channel c - 1 - k for output channel k (RGB as
 * decoded -> the BGR the reference feeds).  ytab has oh entries, xtab ow; dst is the caller's slot
 * inside an (N, oh, ow, c) batch tensor.  Equals resize_linear(img.astype(float32) / 255, oh, ow). */
int unet_image_resize_u8(const unsigned char* src, int sh, int sw, int c,
                         const unet_lerp_coord* ytab, const unet_lerp_coord* xtab, int oh, int ow,
                         int reverse_channels, float* dst, unet_stream_t stream);
/* fp32 probabilities (h, w, ncls) of one image -> uint8 mask (oh, ow), exactly oh * ow bytes at any
 * byte alignment.  ncls == 1: 255 where the interpolated probability > threshold (strict), else 0.
 * 1 < ncls <= 255: the index of the largest interpolated class probability, the first on ties
 * (np.argmax); threshold is ignored.                                                             */
int unet_mask_resize(const float* prob, int h, int w, int ncls, const unet_lerp_coord* ytab,
                     const unet_lerp_coord* xtab, int oh, int ow, float threshold,
                     unsigned char* mask, unet_stream_t stream);

/* ----- Device-side largest-contour box (ABI 16) ----------------------------------------------
 * The last step of scripts/inference.py (reference :173-187): cv2.findContours(mask, RETR_EXTERNAL,
 * CHAIN_APPROX_SIMPLE), the contour of largest cv2.contourArea (the first on ties), its
 * cv2.boundingRect.  unet_amd/imageproc.py: largest_external_contour traces the borders on the
 * host; border following is serial, so the kernels compute a closed form that equals it exactly.
 *
 * THE CONTRACT.  Foreground is mask != 0; the image outside its frame is background.
 *   O  the outer background: the background pixels that reach the frame through background
 *      4-neighbours.  F, the filled image, is everything else: the foreground, its holes, and any
 *      component nested inside a hole.
 *   The 8-connected components of F are the external contours, one to one, in the order of their
 *   first pixel in raster order.  Per component:
 *      boundingRect  its bounding box (x, y, w, h);
 *      area2         twice its contourArea, an integer: the sum over the 2x2 pixel cells that lie
 *                    wholly inside the image of 2 [all four pixels in F] + [exactly three in F]
 *                    (a cell with three or more F pixels lies in one component).
 *   Selection: the largest area2; on ties the component whose first raster pixel has the smallest
 *   linear index (also when every area is 0).  No foreground: count = 0 and every field 0.
 * Every value is an integer and no result depends on the order in which blocks or atomics arrive:
 * the record is deterministic.  unet_amd/imageproc.py: external_contour_stats_filled restates the
 * contract in NumPy; tests/test_contour_host.py holds it equal to the tracer.                    */
typedef struct unet_contour_box {
    int32_t count;      /* external contours found; 0: the other fields are 0 */
    int32_t x, y, w, h; /* boundingRect of the selected contour */
    int32_t first;      /* linear index y*W+x of its first pixel in raster order */
    int64_t area2;      /* twice its contourArea */
} unet_contour_box;     /* 32 bytes */

/* Bytes of workspace unet_mask_largest_contour needs for an (h, w) mask, a multiple of 256: int32
 * labels, int32 area sums and one byte per pixel, behind a 256-byte header.  0 for sizes the call
 * refuses.                                                                                      */
size_t unet_mask_largest_contour_workspace(int h, int w);
/* mask: h * w densely packed bytes at any byte alignment.  out: device memory, 8-byte aligned,
 * written in full by the call (no pre-zeroing asked of the caller).  ws: device memory, 16-byte
 * aligned, ws_bytes >= the query's answer; its contents before the call do not matter and no byte
 * beyond the query's answer is touched.  Refused with an error message: a null pointer, h < 1 or
 * w < 1, h * w > 2^30 (linear indices and area2 are kept in int32), a short workspace.  Ten small
 * launches on `stream`; no kernel waits for another workgroup.                                  */
int unet_mask_largest_contour(const unsigned char* mask, int h, int w, unet_contour_box* out,
                              void* ws, size_t ws_bytes, unet_stream_t stream);

/* ----- Device-resident training set: batch gather (ABI 17) -----------------------------------
 * The training input of scripts/train.py (reference :169-220: ImageDataGenerator, rescale 1/255,
 * horizontal_flip) once the decoded, resized samples live on the device as uint8
 * (unet_amd/device_data.py): one call builds the fp32 frame batch (c = 3), a second the mask batch
 * (c = 1, any byte value).
 *
 * src: n samples of h * w * c bytes each, dense, at any byte alignment.  slots: b device int32
 * entries.  An entry e >= 0 takes sample e as stored; e < 0 takes sample ~e mirrored along w (pixel
 * order reversed, channel order inside a pixel kept).  The decoded index is clamped to [0, n-1] on
 * the device, the rule the unet_lerp_coord tables follow: no table makes the kernel read outside
 * src.  dst: (b, h, w, c) fp32,
 *     dst[i][y][x][k] = (float)src[s][y][flip ? w-1-x : x][k] / 255.0f
 * with the IEEE divide, correctly rounded: bitwise NumPy's a.astype(float32) / 255.0 (of a[:, ::-1]
 * where mirrored).  Every element of dst is written and nothing else.
 * One launch.  w % 4 == 0 with src 4-byte and dst 16-byte aligned takes the 16-byte-store kernel;
 * any other w or alignment a byte-wise one with the same result.  Refused with an error message and
 * no launch: a null pointer, n, h, w or b < 1, c outside {1, 3}, h * w * c > 2^31 - 1, dst or slots
 * not 4-byte aligned.                                                                            */
int unet_batch_gather_u8(const unsigned char* src, int n, int h, int w, int c, const int* slots,
                         int b, float* dst, unet_stream_t stream);

/* ----- Random affine augmentation, warped on the device (ABI 18) ------------------------------
 * The batch gather with Keras' ImageDataGenerator rotation / shift / shear / zoom in it
 * (apply_affine_transform; unet_amd/augment.py draws the parameters and builds the records).
 *
 * src: as above.  slots: b device int32 sample indices, clamped to [0, n-1] on the device; there is
 * no flip encoding, the flip is in the record.  xforms: (b, 6) device fp32, the transform record of
 * each batch position, [m00 m01 o0 m10 m11 o1]: output pixel (r, q) samples source row
 * m00 r + m01 q + o0 and source column m10 r + m11 q + o1.  order: 0 nearest, 1 bilinear.
 * fill_constant: 0 replicates the border (Keras fill_mode "nearest"), else pixels whose source point
 * lies outside the image take cval (in 0..255 units).  dst: (b, h, w, c) fp32.
 *
 * The arithmetic is fp32, one rounding per operation, no contraction, in this order:
 *     sy = (m00 * (float)r + m01 * (float)q) + o0;   sx = (m10 * (float)r + m11 * (float)q) + o1
 *     outside = sy < 0 || sy > h-1 || sx < 0 || sx > w-1
 *     sy = clamp(sy, 0, h-1);   sx = clamp(sx, 0, w-1)
 *     order 1:  y0 = min((int)floorf(sy), max(h-2, 0)), y1 = min(y0 + 1, h-1), fy = sy - (float)y0,
 *               likewise x0, x1, fx; per channel, the four bytes converted to float,
 *               top = p00 + fx * (p01 - p00), bot = p10 + fx * (p11 - p10), v = top + fy * (bot - top)
 *     order 0:  v = p[min((int)floorf(sy + 0.5f), h-1)][min((int)floorf(sx + 0.5f), w-1)]
 *     fill_constant: v = outside ? cval : v
 *     dst = v / 255.0f (the IEEE divide)
 * bitwise augment.affine_u8_reference.  The identity record reproduces unet_batch_gather_u8 of the
 * plain sample, the record [1 0 0 0 -1 w-1] that of the mirrored one.  A non-finite record reads
 * inside the sample like any other: a NaN coordinate is not outside and clamps to 0 (fmaxf / fminf
 * return the other operand), an infinite one is outside and clamps to the border.  Every element of dst is written and nothing else.
 * One launch.  w % 4 == 0 with dst 16-byte aligned takes the 16-byte-store kernel (a thread owns 4
 * consecutive pixels of a row); any other w or alignment a one-float-per-thread one with the same
 * result.  Refused with an error message and no launch: a null pointer, n, h, w or b < 1, c outside
 * {1, 3}, order outside {0, 1}, h * w * c > 2^31 - 1, dst, slots or xforms not 4-byte aligned.     */
int unet_batch_affine_u8(const unsigned char* src, int n, int h, int w, int c, const int* slots,
                         const float* xforms, int b, int order, int fill_constant, float cval,
                         float* dst, unet_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* UNET_HIP_H */
