// Host policy of the depthwise 3x3 family (dwconv.hip's flat kernels, dwtile.hip's tiled ones): which
// kernel a call runs, at what tile shape and grid, and how the filter gradient cuts its work into slabs and
// sizes its workspace.  No kernels, pure functions of the problem and, in the lab build, of the lab knobs;
// pinned by tests/dw_plan_check.cpp.  A change of a route, a tile shape or a block count is a change here and
// in that file's pinned rows.
#pragma once
#include "common.h"  // cdiv, align_up, grid_for, lab_knob

namespace unet {
namespace dw {

constexpr int TH = 8;          // pixel rows of a tile; its columns are TW = kThreads / qt
constexpr int kThreads = 256;  // every kernel of the family

inline int view_channels(int mode, int c0, int c1) { return c0 + (mode == UNET_VIEW_CONCAT ? c1 : 0); }
// float4 lanes: every source of the view is read in whole quads
inline bool view_vec(int mode, int c0, int c1) { return c0 % 4 == 0 && (mode != UNET_VIEW_CONCAT || c1 % 4 == 0); }
// 32-bit element indices, the 2x2 source of a max-pool view included
inline bool index_fits(int mode, int c0, int c1, int n, int h, int w) {
    return (int64_t)n * h * w * view_channels(mode, c0, c1) * (mode == UNET_VIEW_POOL_BNRELU ? 4 : 1) < (int64_t(1) << 31);
}

// channel quads per tile (0: no tiled kernel for this width)
inline int qt_for(int C) {
    if (C <= 0 || C % 4) return 0;
    if (C % 64 == 0) return 16;  // (8 quads x 32 columns measured -0.6 % img/s, round 2)
    const int q = C / 4;
    return (q == 1 || q == 2 || q == 4 || q == 8) ? q : 0;
}

enum { DW_FLAT_SCALAR, DW_FLAT_VEC, DW_TILED };
struct DwPlan {
    int route;
    int n, h, w, C;
    int CQ, flat_grid;                              // flat: lanes per pixel (quads or channels), grid-stride grid
    int qt, tw, tiles_w, tiles_h, chunks, ntiles;   // tiled: grid (ntiles, chunks) of 8 x tw pixels x 4 qt channels
    bool vec() const { return route != DW_FLAT_SCALAR; }
};
inline DwPlan dw_plan(int mode, int c0, int c1, int n, int h, int w) {
    DwPlan p{};
    p.n = n, p.h = h, p.w = w;
    p.C = view_channels(mode, c0, c1);
    const bool vec = view_vec(mode, c0, c1);
    p.qt = vec ? qt_for(p.C) : 0;
    p.route = p.qt ? DW_TILED : vec ? DW_FLAT_VEC : DW_FLAT_SCALAR;
    p.CQ = vec ? p.C / 4 : p.C;
    p.flat_grid = grid_for((int64_t)n * h * w * p.CQ);  // (unet_view_materialize has flat kernels only)
    if (p.qt) {
        p.tw = kThreads / p.qt;
        p.tiles_w = (int)cdiv(w, p.tw);
        p.tiles_h = (int)cdiv(h, TH);
        p.chunks = p.C / (4 * p.qt);
        p.ntiles = n * p.tiles_w * p.tiles_h;
    }
    return p;
}

// Filter gradient: S slabs of [9][C] in the workspace, summed in order by reduce_slabs.  Tiled: one slab per
// persistent block of grid (S, chunks).  Flat: grid (ctiles, S) of CT channel lanes x PL pixel lanes, one
// slab per chunk of ppc pixels.
struct DwFilterPlan {
    DwPlan p;
    int S;
    unsigned grid_x, grid_y;
    int CT, PL;   // flat (the lanes per pixel are p.CQ)
    int64_t ppc;  // flat
    size_t bytes;
};
inline size_t dw_filter_workspace(int n, int h, int w, int c);
inline DwFilterPlan dw_filter_plan(int mode, int c0, int c1, int n, int h, int w) {
    DwFilterPlan f{};
    const DwPlan& p = f.p = dw_plan(mode, c0, c1, n, h, w);
    const size_t slab = (size_t)9 * p.C * sizeof(float);
    if (p.route == DW_TILED) {
        // persistent blocks over all channel chunks: 1024 (~4 per CU), 512 at batch <= 8 (fewer slabs to
        // reduce; configs[4] batch 8 -0.8 %, configs[3] and batch 16 / 32 within the spread or slower with
        // 512, profiles/r5d_step_ab.txt d8_* / d16_* / dq_*)
        int target = lab_knob("UNET_DWF_BLOCKS", n <= lab_knob("UNET_DWF_SMALL_N", 8) ? 512 : 1024);
        if (target < 1) target = 1024;
        int g = (int)cdiv(target, p.chunks);
        if (g > p.ntiles) g = p.ntiles;
        if (g < 1) g = 1;
        f.S = g;
        f.grid_x = (unsigned)g;
        f.grid_y = (unsigned)p.chunks;
    } else {
        f.CT = p.CQ < 64 ? p.CQ : 64;
        f.PL = kThreads / f.CT;
        const int ctiles = (int)cdiv(p.CQ, f.CT);
        const int64_t P = (int64_t)n * h * w;
        const int64_t want = cdiv(2048, ctiles);
        const int64_t maxc = cdiv(P, 256);  // at least ~256 pixels per chunk
        int64_t chunks = want < maxc ? want : maxc;
        // The workspace query knows the channel count, not the view: a concat split off the quads
        // (c0 % 4 != 0, C % 4 == 0) runs here in scalar lanes with the slabs the query gave a view of C
        // channels in whole quads
        if (mode == UNET_VIEW_CONCAT && p.route == DW_FLAT_SCALAR && p.C % 4 == 0) {
            const int64_t cap = (int64_t)(dw_filter_workspace(n, h, w, p.C) / slab);
            if (chunks > cap) chunks = cap;
        }
        if (chunks < 1) chunks = 1;
        f.ppc = cdiv(P, chunks);
        f.S = (int)cdiv(P, f.ppc);
        f.grid_x = (unsigned)ctiles;
        f.grid_y = (unsigned)f.S;
    }
    f.bytes = align_up((size_t)f.S * slab, 256);
    return f;
}
// the C-ABI's view-less query: what a view of c channels in whole quads takes, which covers every view of c channels
inline size_t dw_filter_workspace(int n, int h, int w, int c) {
    if (n <= 0 || h <= 0 || w <= 0 || c <= 0) return 0;
    return dw_filter_plan(UNET_VIEW_PLAIN, c, 0, n, h, w).bytes;
}

// Data gradient that also emits the view block's BatchNorm-backward partials: max-pool or BN+ReLU view on
// the tiled route, one [2][C] slab per tile (0: no such kernel).  With the filter-gradient slabs ([9][C] per
// tile) besides: BN+ReLU view without dropout.
inline int dw_bnstats_slabs(int mode, int c0, int n, int h, int w) {
    if ((mode != UNET_VIEW_POOL_BNRELU && mode != UNET_VIEW_BNRELU) || n <= 0 || h <= 0 || w <= 0) return 0;
    const DwPlan p = dw_plan(mode, c0, 0, n, h, w);
    return p.route == DW_TILED ? p.ntiles : 0;
}
inline bool dw_bnstats_dwf_ok(int mode, int c0, float drop_rate, int n, int h, int w) {
    return mode == UNET_VIEW_BNRELU && drop_rate == 0.f && dw_bnstats_slabs(mode, c0, n, h, w) > 0;
}

}  // namespace dw
}  // namespace unet
