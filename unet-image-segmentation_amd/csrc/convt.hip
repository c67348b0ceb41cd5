// Conv2DTranspose(2, stride 2) entry points.  The taps do not overlap, so the forward is a rows
// GEMM [M, Cin] x [Cin, 4 Cout] with a pixel-shuffle + bias epilogue, the data gradient a rows
// GEMM with a pixel-unshuffle A operand, and the kernel gradient a weight-gradient GEMM (gemm.h).
#include "gemm.h"

using namespace unet;

namespace {
int convt_fwd(const unet_view* x, int n, int h, int w, int cout, const float* kernel, const unsigned short* kernel_x3,
              const float* bias, float* out, unet_stream_t stream) {
    if (check_view(x, "unet_conv_transpose2x2_fwd")) return -1;
    UNET_CHECK_ARG(x->mode == UNET_VIEW_PLAIN || x->mode == UNET_VIEW_BNRELU,
                   "unet_conv_transpose2x2_fwd: input view must be PLAIN or BNRELU");
    UNET_CHECK_ARG(kernel && out && n > 0 && h > 0 && w > 0 && cout > 0, "unet_conv_transpose2x2_fwd: bad args");
    const int cin = x->c0;
    const int64_t M = (int64_t)n * h * w;
    UNET_CHECK_ARG(fits_i32(M, cin) && fits_i32(4 * M, cout), "unet_conv_transpose2x2_fwd: tensor too large");
    RowsArgs a{};
    a.a = make_dview(*x);
    a.M = M;
    a.K = cin;
    a.B = kernel;  // B(k = ci, n = (a, b, co)) = k[(a*2+b)*cout + co][ci]
    a.Bx = kernel_x3;
    a.sbk = 1;
    a.sbn = cin;
    a.N = 4 * cout;
    a.C = out;
    a.bias = bias;
    a.sH = h;
    a.sW = w;
    a.sf = cout;
    hipStream_t st = as_stream(stream);
    const bool drop = x->drop_rate > 0.f;
    if (x->mode == UNET_VIEW_PLAIN) {
        if (drop) return launch_rows<A_PLAIN, true, E_SHUFFLE>(a, st, "unet_conv_transpose2x2_fwd");
        return launch_rows<A_PLAIN, false, E_SHUFFLE>(a, st, "unet_conv_transpose2x2_fwd");
    }
    if (drop) return launch_rows<A_BNRELU, true, E_SHUFFLE>(a, st, "unet_conv_transpose2x2_fwd");
    return launch_rows<A_BNRELU, false, E_SHUFFLE>(a, st, "unet_conv_transpose2x2_fwd");
}
}  // namespace

extern "C" int unet_conv_transpose2x2_fwd(const unet_view* x, int n, int h, int w, int cout, const float* kernel,
                                          const float* bias, float* out, unet_stream_t stream) {
    return convt_fwd(x, n, h, w, cout, kernel, nullptr, bias, out, stream);
}
extern "C" int unet_conv_transpose2x2_fwd_x3(const unet_view* x, int n, int h, int w, int cout, const float* kernel,
                                             const unsigned short* kernel_x3, const float* bias, float* out,
                                             unet_stream_t stream) {
    if (check_planes(kernel_x3, "unet_conv_transpose2x2_fwd_x3: kernel_x3")) return -1;
    return convt_fwd(x, n, h, w, cout, kernel, kernel_x3, bias, out, stream);
}

namespace {
bool convt_fused_bias() {  // lab build UNET_CONVT_FUSED_BIAS=0: separate colsum pass (A/B switch)
    return lab_knob("UNET_CONVT_FUSED_BIAS", 1) != 0;
}
}  // namespace

extern "C" size_t unet_conv_transpose2x2_bwd_workspace(int n, int h, int w, int cin, int cout) {
    if (n <= 0 || h <= 0 || w <= 0 || cin <= 0 || cout <= 0) return 0;
    const int64_t M = (int64_t)n * h * w;
    const WgradPlan wp = wgrad_plan(M, 4 * cout, cin);
    size_t a = wgrad_workspace(M, 4 * cout, cin) + align_up((size_t)wp.S * 4 * cout * sizeof(float), 256);
    size_t b = colsum_workspace(4 * M, cout);
    return a > b ? a : b;
}

extern "C" int unet_conv_transpose2x2_bwd(const unet_view* x, int n, int h, int w, int cout, const float* kernel,
                                          const float* dout, float* dx, float* dkernel, float* dbias, void* ws,
                                          size_t ws_bytes, unet_stream_t stream) {
    if (check_view(x, "unet_conv_transpose2x2_bwd")) return -1;
    UNET_CHECK_ARG(x->mode == UNET_VIEW_PLAIN || x->mode == UNET_VIEW_BNRELU,
                   "unet_conv_transpose2x2_bwd: input view must be PLAIN or BNRELU");
    UNET_CHECK_ARG(kernel && dout && n > 0 && h > 0 && w > 0 && cout > 0, "unet_conv_transpose2x2_bwd: bad args");
    UNET_CHECK_ARG((dkernel == nullptr) == (dbias == nullptr) && (dx || dkernel),
                   "unet_conv_transpose2x2_bwd: dkernel and dbias go together; nothing to compute");
    const int cin = x->c0;
    const int64_t M = (int64_t)n * h * w;
    UNET_CHECK_ARG(fits_i32(M, cin) && fits_i32(4 * M, cout), "unet_conv_transpose2x2_bwd: tensor too large");
    hipStream_t st = as_stream(stream);
    const size_t need = unet_conv_transpose2x2_bwd_workspace(n, h, w, cin, cout);
    UNET_CHECK_ARG(ws && ws_bytes >= need, "unet_conv_transpose2x2_bwd: workspace %zu < %zu", ws_bytes, need);
    // data gradient w.r.t. the view output: dx[m, ci] = sum_{(a,b,co)} dU'[m, (a,b,co)] k[(a,b,co)][ci]
    if (dx) {
        RowsArgs a{};
        a.a = plain_view(dout, cout);
        a.M = M;
        a.K = 4 * cout;
        a.uH = h;
        a.uW = w;
        a.uf = cout;
        a.B = kernel;
        a.sbk = cin;
        a.sbn = 1;
        a.N = cin;
        a.C = dx;
        a.ldc = cin;
        int rc = launch_rows<A_UNSHUFFLE, false, E_STORE>(a, st, "unet_conv_transpose2x2_bwd(data)");
        if (rc) return rc;
    }
    if (!dkernel) return 0;  // data gradient only
    // kernel gradient: dk[(a,b,co)][ci] = sum_m dU'[m, (a,b,co)] x[m, ci]
    WgradArgs wa{};
    wa.a = plain_view(dout, cout);
    wa.P = 4 * cout;
    wa.uH = h;
    wa.uW = w;
    wa.uf = cout;
    wa.b = make_dview(*x);
    wa.Q = cin;
    wa.M = M;
    // bias gradient: the q-tile-0 blocks of the kernel-gradient GEMM also sum dU' over their m slice
    // ([S][4][cout] after the slabs), so dU' is read once; = one fixed-order reduction of 4S rows
    const WgradPlan wp = wgrad_plan(M, 4 * cout, cin);
    const size_t slab_bytes = align_up((size_t)wp.S * 4 * cout * cin * sizeof(float), 256);
    const bool fuse_bias = convt_fused_bias() && cin % 4 == 0 && cout % 4 == 0 &&
                           ((uintptr_t)dout | (uintptr_t)x->src0) % 16 == 0 &&
                           ws_bytes >= slab_bytes + (size_t)wp.S * 4 * cout * sizeof(float);
    if (fuse_bias) wa.colpart = reinterpret_cast<float*>(static_cast<char*>(ws) + slab_bytes);
    int rc = run_wgrad(wa, W_UNSHUFFLE, x->mode == UNET_VIEW_BNRELU ? W_BNRELU : W_PLAIN, dkernel, ws, ws_bytes, st,
                       "unet_conv_transpose2x2_bwd(filter)");
    if (rc) return rc;
    if (fuse_bias) return reduce_slabs(wa.colpart, 4 * wp.S, cout, dbias, cout, cout, st);
    return colsum(dout, 4 * M, cout, dbias, ws, ws_bytes, st);
}

extern "C" int unet_conv_transpose2x2_bwd_data_bnstats_slabs(const unet_view* x, int n, int h, int w, int cout) {
    if (!x || x->mode != UNET_VIEW_BNRELU || !(x->drop_rate >= 0.f && x->drop_rate < 1.f) || n <= 0 || h <= 0 ||
        w <= 0 || cout <= 0)
        return 0;
    if (x->c0 % 4 || cout % 4) return 0;
    const int64_t M = (int64_t)n * h * w;
    if (!fits_i32(M, x->c0) || !fits_i32(4 * M, cout)) return 0;
    return (int)cdiv(M, convt_bnpart_bm(M, x->c0));
}

namespace {
int convt_bwd_data_bnstats(const unet_view* x, int n, int h, int w, int cout, const float* kernel,
                           const unsigned short* kernel_x3t, const float* dout, float* dx, const float* mean,
                           const float* rstd, float* bn_partials, unet_stream_t stream) {
    if (check_view(x, "unet_conv_transpose2x2_bwd_data_bnstats")) return -1;
    const int S = unet_conv_transpose2x2_bwd_data_bnstats_slabs(x, n, h, w, cout);
    UNET_CHECK_ARG(S > 0, "unet_conv_transpose2x2_bwd_data_bnstats: needs a BNRELU view (dropout rate in [0, 1)) "
                          "and channel counts divisible by 4");
    UNET_CHECK_ARG(kernel && dout && dx && bn_partials && x->scale0 && x->shift0,
                   "unet_conv_transpose2x2_bwd_data_bnstats: bad args");
    UNET_CHECK_ARG((mean == nullptr) == (rstd == nullptr), "unet_conv_transpose2x2_bwd_data_bnstats: mean/rstd go together");
    const int cin = x->c0;
    RowsArgs a{};
    a.a = plain_view(dout, cout);
    a.M = (int64_t)n * h * w;
    a.K = 4 * cout;
    a.uH = h;
    a.uW = w;
    a.uf = cout;
    a.B = kernel;
    // (split-precision route only where the partials are per 128-row tile, as the _slabs query said)
    a.Bx = convt_bnpart_bm(a.M, cin) == 128 ? kernel_x3t : nullptr;
    a.sbk = cin;
    a.sbn = 1;
    a.N = cin;
    a.C = dx;
    a.ldc = cin;
    a.z = x->src0;
    a.bsc = x->scale0;
    a.bsh = x->shift0;
    a.bmu = mean;
    a.brs = rstd;
    a.bnpart = bn_partials;
    // a dropout view (the bottleneck output, u_net.py:77-78): the partials are those of the
    // BN + ReLU backward of g = da * mask, as unet_bn_relu_bwd_stats forms them
    a.ep_rate = x->drop_rate;
    a.ep_inv_keep = x->drop_rate > 0.f ? 1.0f / (1.0f - x->drop_rate) : 1.0f;
    a.ep_seed = x->drop_seed;
    UNET_CHECK_ARG(rows_vec_ok(a, A_UNSHUFFLE) && ((uintptr_t)dx | (uintptr_t)x->src0) % 16 == 0,
                   "unet_conv_transpose2x2_bwd_data_bnstats: operands must be 16-B aligned");
    return launch_rows<A_UNSHUFFLE, false, E_BNPART>(a, as_stream(stream), "unet_conv_transpose2x2_bwd_data_bnstats");
}
}  // namespace

extern "C" int unet_conv_transpose2x2_bwd_data_bnstats(const unet_view* x, int n, int h, int w, int cout,
                                                       const float* kernel, const float* dout, float* dx,
                                                       const float* mean, const float* rstd, float* bn_partials,
                                                       unet_stream_t stream) {
    return convt_bwd_data_bnstats(x, n, h, w, cout, kernel, nullptr, dout, dx, mean, rstd, bn_partials, stream);
}
extern "C" int unet_conv_transpose2x2_bwd_data_bnstats_x3(const unet_view* x, int n, int h, int w, int cout,
                                                          const float* kernel, const unsigned short* kernel_x3t,
                                                          const float* dout, float* dx, const float* mean,
                                                          const float* rstd, float* bn_partials, unet_stream_t stream) {
    if (check_planes(kernel_x3t, "unet_conv_transpose2x2_bwd_data_bnstats_x3: kernel_x3t")) return -1;
    return convt_bwd_data_bnstats(x, n, h, w, cout, kernel, kernel_x3t, dout, dx, mean, rstd, bn_partials, stream);
}
