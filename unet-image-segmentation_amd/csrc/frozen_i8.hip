// Frozen int8 inference (ABI 14): the kernels behind UNetModel.freeze(dtype="int8").  The kernel
// skeleton is frozen_common.h; this file is its int8 precision and the entry points.
//
// The arithmetic contract is stated in include/unet_hip.h ("Frozen int8 inference") and restated in
// NumPy by tests/i8_emulation.py; these kernels implement exactly it.  Activations are NHWC bytes:
// uint8 (x = s q, q in [0, 255]) after a ReLU, int8 (q in [-127, 127]) after an upsample; spatial
// padding is q = 0.  The pointwise GEMMs run on v_mfma_i32_32x32x32_i8 with exact int32 accumulators.
//
// MFMA operands (32x32x32, 8-bit): lane l, r = l & 31, hh = l >> 5 holds 16 bytes of A row r and
// 16 bytes of B column r.  Both operands give lane half hh the channels 16 hh .. 16 hh + 15 of the
// K step in the same element slots, so the product is right whatever order the instruction walks
// k in.  The accumulator map is the fp16 MFMA's (frozen_common.h).
#include "frozen_common.h"

namespace unet {
namespace {

using namespace frozen;

typedef int intx4 __attribute__((ext_vector_type(4)));
typedef int intx16 __attribute__((ext_vector_type(16)));
typedef unsigned char u8;

template <bool SG>
__device__ __forceinline__ float byte_f32(unsigned word, int j) {
    if constexpr (SG) return (float)(int)(signed char)(word >> (8 * j));
    return (float)((word >> (8 * j)) & 0xffu);
}
// depthwise accumulation of one tap for 4 channels (one dword of the pixel): a[j] = fmaf(x[j], w[j], a[j])
template <bool SG>
__device__ __forceinline__ void tap_fma4(float* a, unsigned word, float4 w) {
    a[0] = fmaf(byte_f32<SG>(word, 0), w.x, a[0]);
    a[1] = fmaf(byte_f32<SG>(word, 1), w.y, a[1]);
    a[2] = fmaf(byte_f32<SG>(word, 2), w.z, a[2]);
    a[3] = fmaf(byte_f32<SG>(word, 3), w.w, a[3]);
}

// clamp(rintf(v), lo, hi) as an integer
__device__ __forceinline__ int quant(float v, float lo, float hi) { return (int)fminf(fmaxf(rintf(v), lo), hi); }
__device__ __forceinline__ unsigned pack4(const float* a) {
    return (unsigned)(quant(a[0], -127.f, 127.f) & 0xff) | ((unsigned)(quant(a[1], -127.f, 127.f) & 0xff) << 8) |
           ((unsigned)(quant(a[2], -127.f, 127.f) & 0xff) << 16) | ((unsigned)quant(a[3], -127.f, 127.f) << 24);
}

struct I8 {
    using Elem = u8;
    using Out = int;
    using Frag = intx4;
    using Acc = intx16;
    static constexpr int kLane = 16, kStep = 32;
    static constexpr int kHaloLd = kKC + 16;  // bytes per halo pixel: one byte per channel, 16-B slots 5 p + s

    static __device__ __forceinline__ Acc mfma(Frag a, Frag b, Acc c) {
        return __builtin_amdgcn_mfma_i32_32x32x32_i8(a, b, c, 0, 0, 0);
    }

    struct View {
        const u8* src0;
        const u8* src1;
        int c0, c1;
        int sg0, sg1;  // the source holds int8 (else uint8)
    };
    // the source of channel c holds int8 (true_type) or uint8
    template <class F>
    static __device__ __forceinline__ void with_source(const View& v, int c, F&& f) {
        if (c < v.c0 ? v.sg0 : v.sg1)
            f(std::true_type{});
        else
            f(std::false_type{});
    }
    // w = the taps dw s_in / s_y of the 16 channels
    template <class SG>
    static __device__ __forceinline__ void tap_fma(SG, float (&a)[16], uint4 xv, const float* w) {
        tap_fma4<SG::value>(a + 0, xv.x, ld4(w + 0));
        tap_fma4<SG::value>(a + 4, xv.y, ld4(w + 4));
        tap_fma4<SG::value>(a + 8, xv.z, ld4(w + 8));
        tap_fma4<SG::value>(a + 12, xv.w, ld4(w + 12));
    }
    // the depthwise output's quantisation to int8 [-127, 127]
    static __device__ __forceinline__ Frag round_a(const float (&a)[16]) {
        intx4 af;
        af[0] = (int)pack4(a + 0);
        af[1] = (int)pack4(a + 4);
        af[2] = (int)pack4(a + 8);
        af[3] = (int)pack4(a + 12);
        return af;
    }

    // conv block epilogue: q = clamp(rint(acc mult + bias_q), 0, 255) (the clamp is the ReLU)
    struct Col {
        int fix;  // 128 colsum (upsample)
        float mu, b;
    };
    static __device__ __forceinline__ Col sep_col(int col, const float* mult, const float* bias_q) {
        return {0, mult[col], bias_q[col]};
    }
    static __device__ __forceinline__ int sep_out(int acc, Col cp) {
        return quant(fmaf((float)acc, cp.mu, cp.b), 0.f, 255.f);
    }

    // upsample: A = the uint8 input XOR 0x80 (q - 128 as int8); the epilogue adds 128 colsum back,
    // so acc32 is the exact product with q; out int8 [-127, 127] (bias_q per co, the rest per column)
    static __device__ __forceinline__ Frag convt_a(uint4 av) {
        av.x ^= 0x80808080u, av.y ^= 0x80808080u, av.z ^= 0x80808080u, av.w ^= 0x80808080u;
        return __builtin_bit_cast(intx4, av);
    }
    static __device__ __forceinline__ Col convt_col(int col, int cout, const int* colsum, const float* mult,
                                                    const float* bias_q) {
        return {128 * colsum[col], mult[col], bias_q[col % cout]};
    }
    static __device__ __forceinline__ u8 convt_out(int acc, Col cp) {
        return (u8)quant(fmaf((float)(acc + cp.fix), cp.mu, cp.b), -127.f, 127.f);
    }

    // image block: q = clamp(rint(relu(z) / s_out), 0, 255), 8 bytes, one 8-byte store
    struct Image8 {
        unsigned w[2] = {0u, 0u};
    };
    static __device__ __forceinline__ void image_put(Image8& res, int j, float z, float s_out) {
        res.w[j >> 2] |= (unsigned)quant(z / s_out, 0.f, 255.f) << (8 * (j & 3));
    }
    static __device__ __forceinline__ void image_store(Image8 res, u8* out) {
        *reinterpret_cast<uint2*>(out) = make_uint2(res.w[0], res.w[1]);
    }

    // head: one 8-byte chunk of uint8; the input scale is folded into the head's kernel
    static __device__ __forceinline__ uint2 head_ld8(const u8* p) { return *reinterpret_cast<const uint2*>(p); }
    static __device__ __forceinline__ float head_x(uint2 xv, int j) { return byte_f32<false>(j < 4 ? xv.x : xv.y, j & 3); }
};

}  // namespace
}  // namespace unet

using namespace unet;

extern "C" int unet_i8_image_block(const float* x, int n, int h, int w, int cin, const float* dw_kernel, int cout,
                                   const float* pw_folded, const float* bias, float out_scale, unsigned char* out,
                                   unet_stream_t stream) {
    UNET_CHECK_ARG(x && dw_kernel && pw_folded && bias && out, "unet_i8_image_block: null pointer");
    UNET_CHECK_ARG(n > 0 && h > 0 && w > 0, "unet_i8_image_block: empty tensor (%d, %d, %d)", n, h, w);
    UNET_CHECK_ARG(cin >= 1 && cin <= 4, "unet_i8_image_block: cin %d not in 1..4", cin);
    UNET_CHECK_ARG(cout > 0 && cout % 32 == 0, "unet_i8_image_block: cout %d not a positive multiple of 32", cout);
    UNET_CHECK_ARG(out_scale > 0.f && out_scale < INFINITY, "unet_i8_image_block: out_scale %g not positive and finite",
                   (double)out_scale);
    UNET_CHECK_ARG(aligned16(pw_folded) && aligned16(bias) && aligned16(out),
                   "unet_i8_image_block: pw_folded / bias / out must be 16-byte aligned");
    const int64_t items = (int64_t)w * (cout / 8);  // per image row
    UNET_CHECK_ARG((int64_t)n * h < (1ll << 31) && items < (1ll << 30) && cdiv(items, kBlock * kImagePx) < 65536,
                   "unet_i8_image_block: tensor too large");
    const dim3 grid((unsigned)(n * h), (unsigned)cdiv(items, kBlock * kImagePx));
    image_kernel<I8, float><<<grid, kBlock, 0, as_stream(stream)>>>(x, n, h, w, cin, dw_kernel, cout, pw_folded, bias,
                                                             out_scale, out);
    UNET_CHECK_LAUNCH("unet_i8_image_block");
    return 0;
}

extern "C" int unet_i8_sepconv(const unet_i8_view* x, int n, int h, int w, const float* taps, int cout,
                               const signed char* pw_q, const float* mult, const float* bias_q, unsigned char* out,
                               unsigned char* out_pool, int route, unet_stream_t stream) {
    SepPlan plan;
    if (int rc = sep_plan("unet_i8_sepconv", x && taps && pw_q && mult && bias_q && out, n, h, w, cout, out_pool,
                          route, &plan))
        return rc;
    UNET_CHECK_ARG(x->mode == UNET_I8_VIEW_PLAIN || x->mode == UNET_I8_VIEW_CONCAT, "unet_i8_sepconv: bad view mode %d",
                   x->mode);
    I8::View v;
    v.src0 = reinterpret_cast<const u8*>(x->src0);
    v.c0 = x->c0;
    v.sg0 = x->signed0 != 0;
    const bool cat = x->mode == UNET_I8_VIEW_CONCAT;
    v.src1 = cat ? reinterpret_cast<const u8*>(x->src1) : nullptr;
    v.c1 = cat ? x->c1 : 0;
    v.sg1 = cat && x->signed1 != 0;
    UNET_CHECK_ARG(v.src0 && (!cat || v.src1), "unet_i8_sepconv: null view source");
    UNET_CHECK_ARG(v.c0 > 0 && (!cat || v.c1 > 0) && (v.c0 + v.c1) % 32 == 0,
                   "unet_i8_sepconv: view channels (%d, %d) must be positive and sum to a multiple of 32", v.c0, v.c1);
    UNET_CHECK_ARG(!cat || v.c0 % 16 == 0, "unet_i8_sepconv: concat c0 %d not a multiple of 16", v.c0);
    UNET_CHECK_ARG(aligned16(v.src0) && aligned16(v.src1) && aligned16(taps) && aligned16(pw_q) && aligned16(out) &&
                       aligned16(out_pool),
                   "unet_i8_sepconv: tensors must be 16-byte aligned");
    const u8* pw = reinterpret_cast<const u8*>(pw_q);
    hipStream_t s = as_stream(stream);
    with_int<4, 2, 1>(plan.nt, [&](auto NT) {
        with_bool(plan.tile, [&](auto TILE) {
            sep_kernel<I8, NT(), TILE(), float, float><<<plan.grid, kBlock, 0, s>>>(
                v, n, h, w, taps, cout, pw, mult, bias_q, out, out_pool);
        });
    });
    UNET_CHECK_LAUNCH("unet_i8_sepconv");
    return 0;
}

extern "C" int unet_i8_conv_transpose2x2(const unsigned char* x, int n, int h, int w, int cin, int cout,
                                         const signed char* kernel_q, const int32_t* colsum, const float* mult,
                                         const float* bias_q, signed char* out, unet_stream_t stream) {
    UNET_CHECK_ARG(x && kernel_q && colsum && mult && bias_q && out, "unet_i8_conv_transpose2x2: null pointer");
    UNET_CHECK_ARG(n > 0 && h > 0 && w > 0, "unet_i8_conv_transpose2x2: empty tensor (%d, %d, %d)", n, h, w);
    UNET_CHECK_ARG(cin > 0 && cin % 32 == 0, "unet_i8_conv_transpose2x2: cin %d not a positive multiple of 32", cin);
    UNET_CHECK_ARG(cout > 0 && cout % 32 == 0, "unet_i8_conv_transpose2x2: cout %d not a positive multiple of 32",
                   cout);
    UNET_CHECK_ARG(aligned16(x) && aligned16(kernel_q) && aligned16(out),
                   "unet_i8_conv_transpose2x2: tensors must be 16-byte aligned");
    const int N = 4 * cout;  // a multiple of 128
    const int64_t M = (int64_t)n * h * w;
    UNET_CHECK_ARG(M < (1ll << 31), "unet_i8_conv_transpose2x2: tensor too large");
    const dim3 grid((unsigned)cdiv(M, kRows), (unsigned)(N / 128));
    convt_kernel<I8, 4, int, float, float><<<grid, kBlock, 0, as_stream(stream)>>>(
        x, n, h, w, cin, cout, reinterpret_cast<const u8*>(kernel_q), colsum, mult, bias_q, reinterpret_cast<u8*>(out));
    UNET_CHECK_LAUNCH("unet_i8_conv_transpose2x2");
    return 0;
}

extern "C" int unet_i8_head(const unsigned char* x, int n, int h, int w, int cin, int ncls, const float* kernel,
                            const float* bias, float* prob, unet_stream_t stream) {
    UNET_CHECK_ARG(x && kernel && bias && prob, "unet_i8_head: null pointer");
    UNET_CHECK_ARG(n > 0 && h > 0 && w > 0, "unet_i8_head: empty tensor (%d, %d, %d)", n, h, w);
    UNET_CHECK_ARG(cin > 0 && cin % 8 == 0, "unet_i8_head: cin %d not a positive multiple of 8", cin);
    UNET_CHECK_ARG(ncls >= 1, "unet_i8_head: ncls %d < 1", ncls);
    UNET_CHECK_ARG(aligned16(x), "unet_i8_head: x must be 16-byte aligned");
    const int64_t M = (int64_t)n * h * w;
    UNET_CHECK_ARG(cdiv(M * 8, kBlock) < (1ll << 31), "unet_i8_head: tensor too large");
    head_kernel<I8><<<dim3((unsigned)cdiv(M * 8, kBlock)), kBlock, 0, as_stream(stream)>>>(x, M, cin, ncls, kernel, bias,
                                                                                          prob);
    UNET_CHECK_LAUNCH("unet_i8_head");
    return 0;
}
