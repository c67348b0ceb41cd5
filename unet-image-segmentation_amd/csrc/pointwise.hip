// Pointwise (1x1) convolution entry points: forward with BatchNorm statistics, data gradients
// (plain, and through a BatchNorm + ReLU backward), weight gradient.  All are rows / weight-gradient
// GEMMs (gemm.h); the streaming dz pass of the widest data gradients lives here too.
#include "gemm.h"

using namespace unet;

namespace {
int pw_fwd(const float* y, int64_t m, int cin, int cout, const float* pw_kernel, const unsigned short* pw_kernel_x3,
           float* z, float* bn_partials, unet_stream_t stream) {
    UNET_CHECK_ARG(y && pw_kernel && z, "unet_pointwise_fwd: null pointer");
    UNET_CHECK_ARG(m > 0 && cin > 0 && cout > 0, "unet_pointwise_fwd: bad sizes");
    UNET_CHECK_ARG(fits_i32(m, cin) && fits_i32(m, cout), "unet_pointwise_fwd: tensor too large");
    RowsArgs a{};
    a.a = plain_view(y, cin);
    a.M = m;
    a.K = cin;
    a.B = pw_kernel;
    a.Bx = pw_kernel_x3;  // [3][cout][cin]: k = ci contiguous
    a.sbk = cout;
    a.sbn = 1;
    a.N = cout;
    a.C = z;
    a.ldc = cout;
    a.stats = reinterpret_cast<float2*>(bn_partials);
    hipStream_t st = as_stream(stream);
    if (bn_partials) return launch_rows<A_PLAIN, false, E_STATS>(a, st, "unet_pointwise_fwd");
    return launch_rows<A_PLAIN, false, E_STORE>(a, st, "unet_pointwise_fwd");
}
}  // namespace

extern "C" int unet_pointwise_fwd(const float* y, int64_t m, int cin, int cout, const float* pw_kernel, float* z,
                                  float* bn_partials, unet_stream_t stream) {
    return pw_fwd(y, m, cin, cout, pw_kernel, nullptr, z, bn_partials, stream);
}
extern "C" int unet_pointwise_fwd_x3(const float* y, int64_t m, int cin, int cout, const float* pw_kernel,
                                     const unsigned short* pw_kernel_x3, float* z, float* bn_partials,
                                     unet_stream_t stream) {
    if (check_planes(pw_kernel_x3, "unet_pointwise_fwd_x3: pw_kernel_x3")) return -1;
    return pw_fwd(y, m, cin, cout, pw_kernel, pw_kernel_x3, z, bn_partials, stream);
}

extern "C" int unet_pointwise_bwd_data(const float* dz, int64_t m, int cin, int cout, const float* pw_kernel,
                                       float* dy, unet_stream_t stream) {
    UNET_CHECK_ARG(dz && pw_kernel && dy, "unet_pointwise_bwd_data: null pointer");
    UNET_CHECK_ARG(m > 0 && cin > 0 && cout > 0, "unet_pointwise_bwd_data: bad sizes");
    UNET_CHECK_ARG(fits_i32(m, cin) && fits_i32(m, cout), "unet_pointwise_bwd_data: tensor too large");
    RowsArgs a{};
    a.a = plain_view(dz, cout);
    a.M = m;
    a.K = cout;
    a.B = pw_kernel;  // B(k = co, n = ci) = k[ci][co]
    a.sbk = 1;
    a.sbn = cout;
    a.N = cin;
    a.C = dy;
    a.ldc = cin;
    return launch_rows<A_PLAIN, false, E_STORE>(a, as_stream(stream), "unet_pointwise_bwd_data");
}

namespace {
// dz of a BatchNorm + ReLU (+ dropout) block output from (da, z) and coef = (mu, p, q), as the
// A_BNBWD operand load forms it (common.h bn_bwd_dz4): one streaming pass (float4 per
// thread-iteration).
template <bool DROP>
__global__ __launch_bounds__(256) void bn_bwd_dz_kernel(const float* __restrict__ da, const float* __restrict__ z,
                                                        int64_t M, int C, const float* __restrict__ sc,
                                                        const float* __restrict__ sh, const float* __restrict__ coef,
                                                        float rate, float inv_keep, uint64_t seed,
                                                        float* __restrict__ dz) {
    const int CQ = C / 4;
    const int total = (int)(M * CQ);  // < 2^29 (the caller checks M * C < 2^31): 32-bit index math
    for (int idx = blockIdx.x * 256 + threadIdx.x; idx < total; idx += gridDim.x * 256) {
        const int c = (idx % CQ) * 4;
        const int o = idx * 4;  // = m * C + c
        float4 v = ld4(da + o);
        const float4 zz = ld4(z + o), csc = ld4(sc + c), csh = ld4(sh + c);
        const float4 cmu = ld4(coef + c), cp = ld4(coef + C + c), cq = ld4(coef + 2 * C + c);
        if constexpr (DROP) v = mul4(v, drop_mult4(seed, (uint64_t)o, rate, inv_keep));
        bn_bwd_dz4(v, zz, csc, csh, cmu, cp, cq);
        st4(dz + o, v);
    }
}

int pw_bwd_data_bnrelu(const float* da, const float* z, int64_t m, int cin, int cout, const float* pw_kernel,
                       const unsigned short* pw_kernel_x3, const float* scale, const float* shift, const float* coef,
                       float drop_rate, uint64_t drop_seed, float* dy, float* dz, unet_stream_t stream) {
    UNET_CHECK_ARG(da && z && pw_kernel && scale && shift && coef && dy, "unet_pointwise_bwd_data_bnrelu: null pointer");
    UNET_CHECK_ARG(m > 0 && cin > 0 && cout > 0, "unet_pointwise_bwd_data_bnrelu: bad sizes");
    UNET_CHECK_ARG(fits_i32(m, cin) && fits_i32(m, cout), "unet_pointwise_bwd_data_bnrelu: tensor too large");
    UNET_CHECK_ARG(drop_rate >= 0.f && drop_rate < 1.f, "unet_pointwise_bwd_data_bnrelu: bad drop_rate");
    UNET_CHECK_ARG(((uintptr_t)z | (uintptr_t)coef | (uintptr_t)scale | (uintptr_t)shift | (uintptr_t)dz) % 16 == 0,
                   "unet_pointwise_bwd_data_bnrelu: operands must be 16-B aligned");
    RowsArgs a{};
    a.a = plain_view(da, cout);
    a.a.sc0 = scale;
    a.a.sh0 = shift;
    a.a.rate = drop_rate;
    a.a.inv_keep = drop_rate > 0.f ? 1.0f / (1.0f - drop_rate) : 1.0f;
    a.a.seed = drop_seed;
    a.z = z;
    a.coef = coef;
    a.side = dz;
    a.M = m;
    a.K = cout;
    a.B = pw_kernel;  // B(k = co, n = ci) = k[ci][co]
    a.Bx = pw_kernel_x3;
    a.sbk = 1;
    a.sbn = cout;
    a.N = cin;
    a.C = dy;
    a.ldc = cin;
    hipStream_t st = as_stream(stream);
    // The bottleneck-adjacent data gradients (1024 channels on either side: 4+ N-tiles of 256 each
    // re-forming the same dz tile from (da, z), or 1024-deep k-loops of the BN-backward operand
    // load) form dz once in a streaming pass (~6 TB/s) and run the plain GEMM on it: 12-24 us
    // faster per launch (tools/bench_dgrad.py, profiles/r2h_dgrad_split.log); narrower shapes
    // measured equal or slower that way and keep the fused operand load.
    if (dz && (cin >= 1024 || cout >= 1024) && cout % 4 == 0 && rows_vec_ok(a, A_BNBWD)) {
        const int64_t work = m * (cout / 4);
        const unsigned grid = (unsigned)(work / 256 < 4096 ? cdiv(work, 256) : 4096);
        if (drop_rate > 0.f)
            bn_bwd_dz_kernel<true><<<grid, 256, 0, st>>>(da, z, m, cout, scale, shift, coef, drop_rate, a.a.inv_keep,
                                                         drop_seed, dz);
        else
            bn_bwd_dz_kernel<false><<<grid, 256, 0, st>>>(da, z, m, cout, scale, shift, coef, 0.f, 1.f, 0, dz);
        UNET_CHECK_LAUNCH("unet_pointwise_bwd_data_bnrelu(dz)");
        RowsArgs p{};
        p.a = plain_view(dz, cout);
        p.M = m;
        p.K = cout;
        p.B = pw_kernel;
        p.Bx = pw_kernel_x3;
        p.sbk = 1;
        p.sbn = cout;
        p.N = cin;
        p.C = dy;
        p.ldc = cin;
        return launch_rows<A_PLAIN, false, E_STORE>(p, st, "unet_pointwise_bwd_data_bnrelu");
    }
    if (drop_rate > 0.f)
        return launch_rows<A_BNBWD, true, E_STORE>(a, st, "unet_pointwise_bwd_data_bnrelu");
    return launch_rows<A_BNBWD, false, E_STORE>(a, st, "unet_pointwise_bwd_data_bnrelu");
}
}  // namespace

extern "C" int unet_pointwise_bwd_data_bnrelu(const float* da, const float* z, int64_t m, int cin, int cout,
                                              const float* pw_kernel, const float* scale, const float* shift,
                                              const float* coef, float drop_rate, uint64_t drop_seed, float* dy,
                                              float* dz, unet_stream_t stream) {
    return pw_bwd_data_bnrelu(da, z, m, cin, cout, pw_kernel, nullptr, scale, shift, coef, drop_rate, drop_seed, dy,
                              dz, stream);
}

extern "C" int unet_pointwise_bwd_data_bnrelu_x3(const float* da, const float* z, int64_t m, int cin, int cout,
                                                 const float* pw_kernel, const unsigned short* pw_kernel_x3,
                                                 const float* scale, const float* shift, const float* coef,
                                                 float drop_rate, uint64_t drop_seed, float* dy, float* dz,
                                                 unet_stream_t stream) {
    if (check_planes(pw_kernel_x3, "unet_pointwise_bwd_data_bnrelu_x3: pw_kernel_x3")) return -1;
    return pw_bwd_data_bnrelu(da, z, m, cin, cout, pw_kernel, pw_kernel_x3, scale, shift, coef, drop_rate, drop_seed,
                              dy, dz, stream);
}

extern "C" size_t unet_pointwise_bwd_filter_workspace(int64_t m, int cin, int cout) {
    if (m <= 0 || cin <= 0 || cout <= 0) return 0;
    return wgrad_workspace(m, cin, cout);
}

extern "C" int unet_pointwise_bwd_filter(const float* y, const float* dz, int64_t m, int cin, int cout,
                                         float* d_pw_kernel, void* ws, size_t ws_bytes, unet_stream_t stream) {
    UNET_CHECK_ARG(y && dz && d_pw_kernel, "unet_pointwise_bwd_filter: null pointer");
    UNET_CHECK_ARG(m > 0 && cin > 0 && cout > 0, "unet_pointwise_bwd_filter: bad sizes");
    WgradArgs a{};
    a.a = plain_view(y, cin);
    a.P = cin;
    a.b = plain_view(dz, cout);
    a.Q = cout;
    a.M = m;
    return run_wgrad(a, W_PLAIN, W_PLAIN, d_pw_kernel, ws, ws_bytes, as_stream(stream), "unet_pointwise_bwd_filter");
}
