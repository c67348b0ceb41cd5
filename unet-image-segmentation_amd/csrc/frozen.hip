// Frozen half-precision inference (ABI 13): the kernels behind UNetModel.freeze().  The kernel
// skeleton is frozen_common.h; this file is its fp16 precision and the entry points.
//
// BatchNorm is folded into the pointwise weights on the host (unet_amd/frozen.py), so a conv
// block is depthwise 3x3 -> pointwise GEMM -> + bias -> ReLU.  Activations are NHWC fp16 and are
// stored already activated; the pointwise GEMMs run on v_mfma_f32_32x32x16_f16 with fp32
// accumulators.  Rounding to fp16 (nearest even) happens at exactly four places: the folded
// weights (host), each block's depthwise output, each block's output, each upsample's output.
//
// MFMA lane maps (32x32x16, 16-bit operands): lane l, r = l & 31, hh = l >> 5 holds
// A[row r][k = 8 hh + j] and B[k = 8 hh + j][col r], j = 0..7; the accumulator register i of that
// lane is D[row (i & 3) + 8 (i >> 2) + 4 hh][col r].
#include "frozen_common.h"

namespace unet {
namespace {

using namespace frozen;

typedef _Float16 halfx8 __attribute__((ext_vector_type(8)));
typedef _Float16 half_t;

struct F16 {
    using Elem = half_t;
    using Out = half_t;
    using Frag = halfx8;
    using Acc = floatx16;
    static constexpr int kLane = 8, kStep = 16;
    static constexpr int kHaloLd = kKC + 8;  // halves per halo pixel: 144 B, 16-B slots 9 p + s are conflict free

    static __device__ __forceinline__ Acc mfma(Frag a, Frag b, Acc c) {
        return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
    }

    struct View {
        const half_t* src0;
        const half_t* src1;
        int c0, c1;
    };
    // fp16 activations are one kind of source: the tag is unused
    template <class F>
    static __device__ __forceinline__ void with_source(const View&, int, F&& f) {
        f(std::false_type{});
    }
    static __device__ __forceinline__ void tap_fma(std::false_type, float (&a)[8], uint4 xv, const float* w) {
        const halfx8 x = __builtin_bit_cast(halfx8, xv);
        const float4 w0 = ld4(w), w1 = ld4(w + 4);
        a[0] = fmaf((float)x[0], w0.x, a[0]);
        a[1] = fmaf((float)x[1], w0.y, a[1]);
        a[2] = fmaf((float)x[2], w0.z, a[2]);
        a[3] = fmaf((float)x[3], w0.w, a[3]);
        a[4] = fmaf((float)x[4], w1.x, a[4]);
        a[5] = fmaf((float)x[5], w1.y, a[5]);
        a[6] = fmaf((float)x[6], w1.z, a[6]);
        a[7] = fmaf((float)x[7], w1.w, a[7]);
    }
    // the depthwise output's one rounding to fp16
    static __device__ __forceinline__ Frag round_a(const float (&a)[8]) {
        halfx8 af;
#pragma unroll
        for (int j = 0; j < 8; ++j) af[j] = (half_t)a[j];
        return af;
    }

    // conv block epilogue: + bias, ReLU, fp16
    static __device__ __forceinline__ float sep_col(int col, const float* bias) { return bias[col]; }
    static __device__ __forceinline__ half_t sep_out(float acc, float b) { return (half_t)relu(acc + b); }

    // upsample: + bias (bias per co, the column is (a, b, co)), fp16
    static __device__ __forceinline__ Frag convt_a(uint4 av) { return __builtin_bit_cast(halfx8, av); }
    static __device__ __forceinline__ float convt_col(int col, int cout, const float* bias) {
        return bias[col % cout];
    }
    static __device__ __forceinline__ half_t convt_out(float acc, float b) { return (half_t)(acc + b); }

    // image block: 8 halves, one 16-byte store
    using Image8 = halfx8;
    static __device__ __forceinline__ void image_put(Image8& res, int j, float z) { res[j] = (half_t)z; }
    static __device__ __forceinline__ void image_store(Image8 res, half_t* out) {
        *reinterpret_cast<uint4*>(out) = __builtin_bit_cast(uint4, res);
    }

    // head: one 16-byte chunk, a wave reads whole 128-byte runs
    static __device__ __forceinline__ halfx8 head_ld8(const half_t* p) { return __builtin_bit_cast(halfx8, ldg16(p)); }
    static __device__ __forceinline__ float head_x(halfx8 xv, int j) { return (float)xv[j]; }
};

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
    image_kernel<F16><<<grid, kBlock, 0, as_stream(stream)>>>(x, n, h, w, cin, dw_kernel, cout, pw_folded, bias,
                                                              reinterpret_cast<half_t*>(out));
    UNET_CHECK_LAUNCH("unet_f16_image_block");
    return 0;
}

extern "C" int unet_f16_sepconv(const unet_f16_view* x, int n, int h, int w, const float* dw_kernel, int cout,
                                const unsigned short* pw_t, const float* bias, unsigned short* out,
                                unsigned short* out_pool, int route, unet_stream_t stream) {
    SepPlan plan;
    if (int rc = sep_plan("unet_f16_sepconv", x && dw_kernel && pw_t && bias && out, n, h, w, cout, out_pool, route,
                          &plan))
        return rc;
    UNET_CHECK_ARG(x->mode == UNET_F16_VIEW_PLAIN || x->mode == UNET_F16_VIEW_CONCAT,
                   "unet_f16_sepconv: bad view mode %d", x->mode);
    F16::View v;
    v.src0 = reinterpret_cast<const half_t*>(x->src0);
    v.c0 = x->c0;
    const bool cat = x->mode == UNET_F16_VIEW_CONCAT;
    v.src1 = cat ? reinterpret_cast<const half_t*>(x->src1) : nullptr;
    v.c1 = cat ? x->c1 : 0;
    UNET_CHECK_ARG(v.src0 && (!cat || v.src1), "unet_f16_sepconv: null view source");
    UNET_CHECK_ARG(v.c0 > 0 && v.c0 % 16 == 0 && (!cat || (v.c1 > 0 && v.c1 % 16 == 0)),
                   "unet_f16_sepconv: view channels (%d, %d) must be positive multiples of 16", v.c0, v.c1);
    UNET_CHECK_ARG(aligned16(v.src0) && aligned16(v.src1) && aligned16(dw_kernel) && aligned16(pw_t) &&
                       aligned16(out) && aligned16(out_pool),
                   "unet_f16_sepconv: tensors must be 16-byte aligned");
    half_t* o = reinterpret_cast<half_t*>(out);
    half_t* op = reinterpret_cast<half_t*>(out_pool);
    const half_t* pw = reinterpret_cast<const half_t*>(pw_t);
    hipStream_t s = as_stream(stream);
    with_int<4, 2, 1>(plan.nt, [&](auto NT) {
        with_bool(plan.tile, [&](auto TILE) {
            sep_kernel<F16, NT(), TILE(), float><<<plan.grid, kBlock, 0, s>>>(v, n, h, w, dw_kernel, cout, pw, bias, o, op);
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
        convt_kernel<F16, NT(), float><<<grid, kBlock, 0, s>>>(xs, n, h, w, cin, cout, ks, bias, o);
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
    head_kernel<F16><<<dim3((unsigned)cdiv(M * 8, kBlock)), kBlock, 0, as_stream(stream)>>>(
        reinterpret_cast<const half_t*>(x), M, cin, ncls, kernel, bias, prob);
    UNET_CHECK_LAUNCH("unet_f16_head");
    return 0;
}
