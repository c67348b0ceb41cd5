// Tiled depthwise 3x3 path (dwtile.hip), called by the unet_dwconv3x3_* entry points (dwconv.hip).
#pragma once
#include "dispatch.h"
#include "view.h"

namespace unet {

int dw_tiled_fwd(const DView& v, int mode, bool drop, int N, int H, int W, const float* K, float* Y, hipStream_t st);
int dw_tiled_bwd_data(const DView& v, int mode, bool drop, int N, int H, int W, const float* K, const float* dY,
                      float* dx0, float* dx1, hipStream_t st);
size_t dw_tiled_filter_partials(int N, int H, int W, int C);
int dw_tiled_bwd_data_bnstats(const DView& v, int mode, bool drop, int N, int H, int W, const float* K,
                              const float* dY, float* dx0, const float* mu, const float* rs, float* bnpart,
                              hipStream_t st, float* dwpart = nullptr);
size_t dw_tiled_ntiles(int N, int H, int W, int C);
int dw_tiled_bwd_filter(const DView& v, int mode, bool drop, int N, int H, int W, const float* dY, float* part,
                        int* S_out, hipStream_t st);
bool dw_tiled_ok(int C);

}  // namespace unet
