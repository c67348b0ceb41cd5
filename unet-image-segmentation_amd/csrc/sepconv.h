// Shared definitions of the fused SeparableConv2D forward kernels (sepconv.hip: the entry points, the
// LDS-A-tile schedule and the pooling-selection pass; sepconv_rk.hip: the register-A schedule, fp32 and
// split precision; sepconv_px.hip: the persistent split-precision schedule).  Which of them a call runs,
// and the tile constants, are sepconv_plan.h's.  Reference model/u_net.py:14-23.
#pragma once
#include "dispatch.h"
#include "sepconv_plan.h"
#include "view.h"

namespace unet {
namespace sep {

constexpr int HHp = TH + 2, HWp = TW + 2;  // halo of one M tile
enum { E_STORE = 0, E_STATS = 1 };

__device__ __forceinline__ int acc_row(int r, int hi) { return (r & 3) + 8 * (r >> 2) + 4 * hi; }

struct SepArgs {
    DView x;
    int N, H, W, Cin, Cout;
    const float* dk;  // (3,3,Cin,1)
    const float* pk;  // (1,1,Cin,Cout): B(k, n) = pk[k*Cout + n] (n-contiguous)
    float* y;         // optional (N,H,W,Cin)
    float* z;         // (N,H,W,Cout)
    float2* stats;    // [M/128][Cout]
    const unsigned short* pkx;  // optional bf16x3 split of pk: planes [3][Cout][Cin] (unet_split_x3)
    float* zsel;         // optional (N,H/2,W/2,Cout): the 2x2 pooling selection of z (pool_select_kernel)
    const float* gamma;  // zsel: BN gamma (its sign orders the window), NULL = no BN (max)
};

// The raw z value of a 2x2 window that the max-pool of relu(z * s + b) takes, with s of the sign of
// gamma: the max where gamma >= 0 (+0 included), the min where gamma < 0.  fmaf is monotone in z,
// so relu(fmaf(sel, s, b)) is bitwise the max over the window of relu(fmaf(z, s, b)).
__device__ __forceinline__ float pool_sel(float a, float b, float c, float d, bool neg) {
    return neg ? fminf(fminf(a, b), fminf(c, d)) : fmaxf(fmaxf(a, b), fmaxf(c, d));
}

// ... of four channels at once; n*: the sign of each channel's gamma
__device__ __forceinline__ float4 pool_sel4(float4 a, float4 b, float4 c, float4 d, bool nx, bool ny, bool nz, bool nw) {
    return make_float4(pool_sel(a.x, b.x, c.x, d.x, nx), pool_sel(a.y, b.y, c.y, d.y, ny), pool_sel(a.z, b.z, c.z, d.z, nz),
                       pool_sel(a.w, b.w, c.w, d.w, nw));
}

// The launchers turn the plan's route, tile width and grid into template arguments; the caller checks the launch.
// register-A schedule (sepconv_rk.hip), routes SEP_RK and SEP_RK_X6 (split precision, reads a.pkx)
void launch_rk(const SepArgs& a, const SepFwdPlan& p, int mode, bool drop, bool stats, bool write_y, hipStream_t st);
// persistent split-precision schedule (sepconv_px.hip), route SEP_PX (reads a.pkx)
void launch_px(const SepArgs& a, const SepFwdPlan& p, int mode, bool drop, bool stats, bool write_y, hipStream_t st);

}  // namespace sep
}  // namespace unet
