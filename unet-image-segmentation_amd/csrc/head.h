// Output layer + loss + metric kernels: what head_fwd.hip, head_bwd.hip and loss.hip share.
//   head      : Conv2D(num_classes, 1, activation=sigmoid|softmax)   model/u_net.py:105-112
//   dice/iou  : dice_coef / iou_coef / dice_loss / iou_loss            utils/metrics.py:6-62,
//                                                                      utils/loss.py:9-48
//   MeanIoU   : keras.metrics.MeanIoU(num_classes)                     scripts/train.py:231,
//                                                                      scripts/benchmark.py:237-277
// The head is HBM-bound (64 -> ncls per pixel).  Binary: a lane group per pixel, xor-shuffle
// dot products (head_fwd_bin_kernel); multi-class: one lane per pixel, the (Cin x ncls) kernel in
// LDS (broadcast reads).  Dice sums are per (image, class) over H*W: per-block
// partials, then one fixed-order finalize in double.  Which kernel a call runs: head_plan.h.
#pragma once
#include "dispatch.h"
#include "head_plan.h"
#include "view.h"

namespace unet {

// gemm_wgrad.hip: the dlogit routes' weight gradient (their bias gradient is common.h's colsum)
int head_wgrad(const unet_view* x, int64_t M, const float* dlogit, int ncls, float* dkernel, void* ws,
               size_t ws_bytes, hipStream_t st);
size_t head_wgrad_workspace(int64_t M, int cin, int ncls);

// Channels [c, c + 4) of row m for the two general forward kernels.  al = false: src0 is only 4-byte
// aligned (the caller's predicate sent it here), so the row is read element by element.
template <int MODE>
__device__ __forceinline__ float4 head_row4(const DView& v, int64_t m, int c, bool al) {
    if (al) return row_load4<MODE, false>(v, m, c);
    return make_float4(row_load1<MODE, false>(v, m, c), row_load1<MODE, false>(v, m, c + 1),
                       row_load1<MODE, false>(v, m, c + 2), row_load1<MODE, false>(v, m, c + 3));
}

// The Keras (1, 1, Cin, ncls) kernel W into LDS as Ws[Cin][NC], classes past ncls zero (a macro for the
// reason given at SOFTMAX_REGS)
#define STAGE_KERNEL(Ws, W, Cin, NC, ncls)                    \
    for (int i_ = threadIdx.x; i_ < Cin * NC; i_ += 256) {    \
        const int k_ = i_ / NC, c_ = i_ - k_ * NC;            \
        Ws[i_] = c_ < ncls ? W[k_ * ncls + c_] : 0.f;         \
    }

// Softmax over the first ncls of the NC logits l[] held in registers: l[c] = exp(l[c] - max) (0 past
// ncls); declares `inv` = 1 / sum, and the caller stores l[c] * inv.  (A macro, as SOFTMAX_BWD and
// BLOCK_SUM_STRIDE below: through inlined functions the kernels compiled differently.  Every name the
// macros read is an argument; what they declare besides the named results ends in an underscore.)
#define SOFTMAX_REGS(l, NC, ncls, inv)                \
    float mx_ = -INFINITY;                            \
    _Pragma("unroll") for (int c = 0; c < NC; ++c)    \
        if (c < ncls) mx_ = fmaxf(mx_, l[c]);         \
    float s_ = 0.f;                                   \
    _Pragma("unroll") for (int c = 0; c < NC; ++c) {  \
        l[c] = c < ncls ? expf(l[c] - mx_) : 0.f;     \
        s_ += l[c];                                   \
    }                                                 \
    const float inv = 1.0f / s_

// d(loss)/d(prob) for one (pixel, class) from the per-(image, class) sums
template <int LOSS>
__device__ __forceinline__ float loss_grad(float t, const float* s3, float smooth, float gscale) {
    const float I = s3[0], T = s3[1], P = s3[2];
    if constexpr (LOSS == UNET_LOSS_DICE) {
        const float nm = 2.0f * I + smooth, den = T + P + smooth;
        return -gscale * (2.0f * t * den - nm) / (den * den);
    } else {
        const float j = I + smooth, u = T + P - I + smooth;
        return -gscale * (t * u - j * (1.0f - t)) / (u * u);
    }
}

// Softmax (ncls == 1: sigmoid) backward of pixel m of M (hw pixels an image): declares dl[NC] with
// dl[c] = p_c (dL/dp_c - sum_k dL/dp_k p_k), zero past ncls and past M, and stores it to dlogit.  The
// trailing statements run once per class c < NC, after dl[c] is final and before its dlogit store.
#define SOFTMAX_BWD(dl, NC, LOSS, m, M, hw, ncls, prob, yt, sums, smooth, gscale, dlogit, ...)                   \
    const int64_t m_ = m;                                                                                        \
    float p_[NC], dl[NC];                                                                                        \
    _Pragma("unroll") for (int c = 0; c < NC; ++c) {                                                             \
        p_[c] = 0.f;                                                                                             \
        dl[c] = 0.f;                                                                                             \
        if (c < ncls && m_ < M) {                                                                                \
            p_[c] = prob[m_ * ncls + c];                                                                         \
            dl[c] = loss_grad<LOSS>(yt[m_ * ncls + c], sums + ((m_ / hw) * ncls + c) * 3, smooth, gscale);       \
        }                                                                                                        \
    }                                                                                                            \
    float s_ = 0.f;                                                                                              \
    _Pragma("unroll") for (int c = 0; c < NC; ++c) s_ = fmaf(dl[c], p_[c], s_);                                  \
    _Pragma("unroll") for (int c = 0; c < NC; ++c) {                                                             \
        dl[c] = p_[c] * (dl[c] - s_);                                                                            \
        __VA_ARGS__;                                                                                             \
        if (c < ncls && m_ < M) dlogit[m_ * ncls + c] = dl[c];                                                   \
    }

// Fixed-order block sum of one float4 per thread (v) over the threads of equal threadIdx.x % groups
// (groups divides 256; red: 256 float4 of LDS): the threads below `groups` run the trailing statements with their
// group's sum in the float4 `t`.  A macro: through an inlined function the kernels compiled differently.
#define BLOCK_SUM_STRIDE(red, v, groups, t, ...)                                            \
    do {                                                                                    \
        __syncthreads();                                                                    \
        red[threadIdx.x] = v;                                                               \
        __syncthreads();                                                                    \
        if (threadIdx.x < groups) {                                                         \
            float4 t = red[threadIdx.x];                                                    \
            for (int q = threadIdx.x + groups; q < 256; q += groups) t = add4(t, red[q]);   \
            __VA_ARGS__;                                                                    \
        }                                                                                   \
    } while (0)

}  // namespace unet
