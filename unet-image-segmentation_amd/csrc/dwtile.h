// Tiled depthwise 3x3 path (dwtile.hip), called by the unet_dwconv3x3_* entry points (dwconv.hip) with the
// plan of the call (dw_plan.h, route DW_TILED).
#pragma once
#include "dispatch.h"
#include "dw_plan.h"
#include "view.h"

namespace unet {

// The gradient of a 2x2 max-pool window goes to its first maximum in row-major order.  xv: the window's four
// values, g: their stored gradients, which take acc (one channel or four).
__device__ __forceinline__ int pool_first_max(float x0, float x1, float x2, float x3) {
    float best = x0;
    int arg = 0;
    if (x1 > best) { best = x1; arg = 1; }
    if (x2 > best) { best = x2; arg = 2; }
    if (x3 > best) { best = x3; arg = 3; }
    return arg;
}
__device__ __forceinline__ void pool_route(float& g0, float& g1, float& g2, float& g3, float x0, float x1, float x2,
                                           float x3, float acc) {
    const int arg = pool_first_max(x0, x1, x2, x3);
    g0 += arg == 0 ? acc : 0.f;
    g1 += arg == 1 ? acc : 0.f;
    g2 += arg == 2 ? acc : 0.f;
    g3 += arg == 3 ? acc : 0.f;
}
__device__ __forceinline__ void pool_route(float4 (&g)[4], const float4 (&xv)[4], const float4& acc) {
    pool_route(g[0].x, g[1].x, g[2].x, g[3].x, xv[0].x, xv[1].x, xv[2].x, xv[3].x, acc.x);
    pool_route(g[0].y, g[1].y, g[2].y, g[3].y, xv[0].y, xv[1].y, xv[2].y, xv[3].y, acc.y);
    pool_route(g[0].z, g[1].z, g[2].z, g[3].z, xv[0].z, xv[1].z, xv[2].z, xv[3].z, acc.z);
    pool_route(g[0].w, g[1].w, g[2].w, g[3].w, xv[0].w, xv[1].w, xv[2].w, xv[3].w, acc.w);
}

int dw_tiled_fwd(const dw::DwPlan& p, const DView& v, int mode, bool drop, const float* K, float* Y, hipStream_t st);
int dw_tiled_bwd_data(const dw::DwPlan& p, const DView& v, int mode, bool drop, const float* K, const float* dY, float* dx0,
                      float* dx1, hipStream_t st);
int dw_tiled_bwd_data_bnstats(const dw::DwPlan& p, const DView& v, int mode, bool drop, const float* K, const float* dY,
                              float* dx0, const float* mu, const float* rs, float* bnpart, hipStream_t st,
                              float* dwpart = nullptr);
int dw_tiled_bwd_filter(const dw::DwFilterPlan& f, const DView& v, int mode, bool drop, const float* dY, float* part,
                        hipStream_t st);

}  // namespace unet
