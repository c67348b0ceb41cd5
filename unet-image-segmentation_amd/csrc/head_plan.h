// Host policy of the output layer and its loss: which kernel family a head call runs, its grid, and
// where its scratch lives.  No kernels, pure functions of the problem (view mode, Cin = c0, class
// count, pixel count M >= 1, and the pointer-alignment bits the launchers test), pinned by
// tests/head_plan_check.cpp.  One function, head_fwd_tp, is __host__ __device__: head_fwd_kernel calls
// it too, so the general forward's pixel tile has one formula.  Callers have validated
// c0 % 4 == 0 (check_view's need_vec4), c0 <= kMaxCin, 1 <= ncls <= kMaxCls and n, h, w > 0.
#pragma once
#include "common.h"  // cdiv, align_up

namespace unet {

constexpr int kMaxCin = 256;
constexpr int kMaxCls = 32;

// blocks of a grid-stride kernel over `work` items, `tile` a block pass: at least one, at most cap
inline int tile_grid(int64_t work, int tile, int cap) {
    const int64_t g = cdiv(work, tile);
    return (int)(g > cap ? cap : g < 1 ? 1 : g);
}

// ----------------------------------------------------------------------------- forward ----
enum { HEAD_FWD_BIN, HEAD_FWD_MFMA, HEAD_FWD_REG, HEAD_FWD_GENERAL };
// pixel tile of the general forward kernel (head_fwd_kernel computes the same): its LDS stays <= 64 KB
__host__ __device__ inline int head_fwd_tp(int c0, bool multi) {
    const int tp = (multi ? 4096 : 8192) / c0;
    return tp < 256 ? tp : 256;
}
struct HeadFwdPlan {
    int route, grid;
    int tp;      // GENERAL: pixels per tile
    size_t lds;  // GENERAL: dynamic LDS bytes ([kMaxCin][NC] kernel, [NC] bias, [tp][c0 + 1] rows)
};
inline HeadFwdPlan head_fwd_plan(int c0, int ncls, int64_t M, bool src_al, bool kernel_al) {
    const bool multi = ncls > 1;
    if (!multi && (c0 == 32 || c0 == 64 || c0 == 128 || c0 == 256) && src_al && kernel_al)
        return {HEAD_FWD_BIN, tile_grid(M, 16 * (64 / (c0 / 4)), 4096), 0, 0};  // c0 / 4 lanes a pixel
    if (multi && (c0 == 16 || c0 == 32 || c0 == 64) && src_al) return {HEAD_FWD_MFMA, tile_grid(M, 128, 2048), 0, 0};
    if (multi && c0 <= 64) return {HEAD_FWD_REG, tile_grid(M, 256, 4096), 0, 0};
    const int tp = head_fwd_tp(c0, multi), nc = multi ? kMaxCls : 1;
    return {HEAD_FWD_GENERAL, tile_grid(M, tp, 4096), tp,
            ((size_t)kMaxCin * nc + nc + (size_t)tp * (c0 + 1)) * sizeof(float)};
}

// ---------------------------------------------------------------------------- backward ----
// The fused routes leave per-block partials of dW and db in the workspace; the dlogit routes store
// dlogit there and hand the rest to the weight-gradient GEMM and the column sum.
enum { HEAD_BWD_BIN_FUSED, HEAD_BWD_MC_FUSED, HEAD_BWD_MC_REG, HEAD_BWD_GENERAL };
constexpr int kHeadFusedMaxGrid = 1024;  // the largest grid of a fused route (BIN_FUSED)
// part_w = [blocks][c0 * ncls] floats at 0, part_b = [blocks][ncls] floats at part_b_off
struct HeadFusedLayout {
    size_t part_b_off, bytes;
};
inline HeadFusedLayout head_fused_layout(int blocks, int c0, int ncls) {
    const size_t off = align_up((size_t)blocks * c0 * ncls, 64);
    return {off, (off + align_up((size_t)blocks * ncls, 64)) * sizeof(float)};
}
inline size_t head_dlogit_bytes(int64_t M, int ncls) { return align_up((size_t)M * ncls * sizeof(float), 256); }
struct HeadBwdPlan {
    int route, grid;
    size_t part_b_off;    // fused routes: part_b's offset in floats (part_w at 0)
    size_t dlogit_bytes;  // dlogit routes: ws2, the GEMM's and the column sum's scratch, starts here
    bool fused() const { return route == HEAD_BWD_BIN_FUSED || route == HEAD_BWD_MC_FUSED; }
};
inline HeadBwdPlan head_bwd_plan(int c0, int ncls, int64_t M) {
    HeadBwdPlan p{};
    // grids: BIN_FUSED and GENERAL by measurement; MC_FUSED 2 blocks a CU (77 KB of LDS at 24 classes),
    // one wave of blocks
    if (ncls == 1 && 256 % (c0 / 4) == 0) p = {HEAD_BWD_BIN_FUSED, tile_grid(M, 256, kHeadFusedMaxGrid)};
    else if (ncls > 1 && ncls <= 24 && c0 <= 64 && 256 % (c0 / 2) == 0) p = {HEAD_BWD_MC_FUSED, tile_grid(M, 256, 512)};
    else if (ncls > 1 && 256 % (c0 / 4) == 0) p = {HEAD_BWD_MC_REG, tile_grid(M, 256, 2048)};
    else p = {HEAD_BWD_GENERAL, tile_grid(M, 256, 4096)};
    if (p.fused()) p.part_b_off = head_fused_layout(p.grid, c0, ncls).part_b_off;
    else p.dlogit_bytes = head_dlogit_bytes(M, ncls);
    return p;
}
// unet_head_bwd_workspace: what any route's layout can need -- the fused layout at its largest grid, or
// dlogit and the larger of the weight-gradient and column-sum scratch -- whichever route the shape takes
inline size_t head_bwd_workspace_bytes(int c0, int ncls, int64_t M, size_t wgrad_bytes, size_t colsum_bytes) {
    const size_t fused = head_fused_layout(kHeadFusedMaxGrid, c0, ncls).bytes;
    const size_t gen = head_dlogit_bytes(M, ncls) + (wgrad_bytes > colsum_bytes ? wgrad_bytes : colsum_bytes);
    return align_up(fused > gen ? fused : gen, 256);
}
// unet_head_bwd_bnstats_slabs: the fused routes emit one BatchNorm-backward slab per block of a BNRELU view
inline int head_bwd_bnstats_slabs(int mode, int c0, int ncls, int64_t M) {
    if (mode != UNET_VIEW_BNRELU || M <= 0 || c0 <= 0 || c0 % 4 || c0 > kMaxCin || ncls < 1 || ncls > kMaxCls) return 0;
    const HeadBwdPlan p = head_bwd_plan(c0, ncls, M);
    return p.fused() ? p.grid : 0;
}

// -------------------------------------------------------------------------------- dice ----
// nblk blocks of ppb pixels per image: ~1024 blocks in all, at least 1024 pixels a block
struct DicePlan {
    int nblk;
    int64_t ppb;
};
inline DicePlan dice_plan(int n, int64_t hw) {
    DicePlan d;
    int64_t want = cdiv(1024, n);
    int64_t maxb = cdiv(hw, 1024);
    int64_t b = want < maxb ? want : maxb;
    if (b < 1) b = 1;
    d.ppb = cdiv(hw, b);
    d.nblk = (int)cdiv(hw, d.ppb);
    return d;
}

}  // namespace unet
