// Host policy of the fused SeparableConv2D family: which forward kernel a call runs (sepconv.hip's
// LDS-A-tile schedule, sepconv_rk.hip's register-A schedule in fp32 or split precision, sepconv_px.hip's
// persistent one), at what tile width and grid, and how the backward (sepwgrad.hip) cuts its pixel tiles
// into slices and lays out its workspace.  No kernels, pure functions of the problem and, in the lab build,
// of the lab knobs; pinned by tests/sepconv_plan_check.cpp.  A change of a forward route or tile width is a
// change here and in that file's pinned rows.
#pragma once
#include "common.h"  // cdiv, align_up, lab_knob

namespace unet {
namespace sep {

constexpr int TH = 8, TW = 16;    // pixel rectangle of one forward M tile; the shape granularity of the C-ABI
constexpr int BK = 16;            // channels per k-stage
constexpr int BTH = 4, BTW = 16;  // pixel rectangle of one backward tile
constexpr int CI = 64;            // backward: input channels per block (ci group)

inline int view_channels(int mode, int c0, int c1) { return c0 + (mode == UNET_VIEW_CONCAT ? c1 : 0); }

// ----------------------------------------------------------------------------- forward ----
inline bool sep_fwd_supported(int mode, int c0, int c1, int n, int h, int w, int cout) {
    if (n <= 0 || h <= 0 || w <= 0 || cout <= 0) return false;
    const int C = view_channels(mode, c0, c1);
    if (h % TH || w % TW || C % 4 || cout % 4) return false;
    if (mode == UNET_VIEW_CONCAT && c0 % 4) return false;
    const int64_t M = (int64_t)n * h * w, lim = int64_t(1) << 31;  // 32-bit element indices, the 2x2 source included
    return M * C < lim && M * cout < lim && M * C * (mode == UNET_VIEW_POOL_BNRELU ? 4 : 1) < lim;
}

// register-A schedule: BN+ReLU / concat / plain views of >= 64 channels; max-pool views only up to 128
// output channels: wider layers keep the LDS-A-tile kernel's 256-wide 8-wave tile, which pools each halo
// element once for all columns (measured: tools/lab/sep_rk_lab.hip, enc3_block1 / enc4_block1)
inline bool rk_supported(int mode, int cin, int cout) {
    return mode >= UNET_VIEW_PLAIN && mode <= UNET_VIEW_CONCAT && cin >= 64 && cout >= 64 &&
           (mode != UNET_VIEW_POOL_BNRELU || cout <= 128);
}
// its split-precision (bf16x6) variant, given the split planes of the pointwise kernel
inline bool rk_x6_supported(int mode, int cin) { return mode != UNET_VIEW_POOL_BNRELU && cin % 16 == 0 && cin >= 64; }
// persistent split-precision schedule, given the split planes
inline bool px_supported(int mode, int c0, int cin, int cout, bool zsel, bool all_shapes) {
    if (lab_knob("UNET_PX", 1) == 0) return false;  // (lab: UNET_PX=0 keeps the one-tile kernel)
    if (mode != UNET_VIEW_PLAIN && mode != UNET_VIEW_BNRELU && mode != UNET_VIEW_CONCAT) return false;
    if ((cin != 64 && cin != 128) || (cout != 64 && cout != 128)) return false;
    // Only the shapes where it wins INSIDE the train step: 128 outputs from 64 inputs or with the
    // pool-selection epilogue (enc2_block1 79.0 -> 78.2 us, enc2_block2 147.2 -> 138.8 us).  Isolated
    // on a repeated input it also beats the one-tile kernel on 64 -> 64 (1.09-1.14x,
    // profiles/r4l_px_lab.log), but in the step enc1_block2 165 -> 173, dec1_block2 137 -> 158,
    // dec1_block1 258 -> 265, dec2_block2 133 -> 136 us (profiles/r4q_px_in_step.txt).
    // all_shapes (schedule RK) or UNET_PX_ALL=1 (lab) take every supported shape.
    if (!all_shapes && lab_knob("UNET_PX_ALL", 0) == 0 && !(cout == 128 && (cin == 64 || zsel))) return false;
    return !(mode == UNET_VIEW_CONCAT && c0 % 16);
}

enum { SEP_REFUSED, SEP_TILE, SEP_RK, SEP_RK_X6, SEP_PX };
struct SepFwdPlan {
    int route;
    int bn;  // output columns of a block's tile: 64, 128 or 256
    unsigned grid_x, grid_y;
    int threads;
    int ntiles, per, pd;  // PX: pixel tiles, tiles per block behind grid_x, prefetch depth
    bool pool_pass;       // the pooling selection is written by unet_pool_select after the kernel
};
// For a shape sep_fwd_supported accepts.  schedule: UNET_SEPCONV_AUTO / TILE / RK (register-A or refuse,
// persistent wherever it exists) / RK1 (never persistent); has_pkx: the caller gave the bf16x3 split of
// the pointwise kernel; want_zsel: it asked for the pooling selection.
inline SepFwdPlan sep_fwd_plan(int schedule, int mode, int c0, int c1, int cout, int n, int h, int w, bool has_pkx,
                               bool want_zsel) {
    const int cin = view_channels(mode, c0, c1);
    const int64_t mt = (int64_t)n * (h / TH) * (w / TW);
    SepFwdPlan p{};
    p.grid_x = (unsigned)mt;
    p.threads = 256;
    if (schedule == UNET_SEPCONV_TILE || !rk_supported(mode, cin, cout)) {
        if (schedule == UNET_SEPCONV_RK) return p;  // SEP_REFUSED
        // the 256-wide, 8-wave tile when it still gives every CU (256) a block; else 128 (measured:
        // tools/bench_sepconv.py, profiles/r1i_sepconv_bn_sweep.log)
        p.route = SEP_TILE;
        p.bn = cout <= 64 ? 64 : cout <= 128 ? 128 : 256;
        if (p.bn == 256 && mt * cdiv(cout, 256) < 256) p.bn = 128;
        p.threads = p.bn == 256 ? 512 : 256;
        p.pool_pass = want_zsel;
    } else if (has_pkx && schedule != UNET_SEPCONV_RK1 &&
               px_supported(mode, c0, cin, cout, want_zsel, schedule == UNET_SEPCONV_RK)) {
        // two blocks per CU; equal runs of tiles (the grid is the tile count / the tiles per block)
        p.route = SEP_PX;
        p.bn = cout;
        p.ntiles = (int)mt;
        const int slots = 256 * lab_knob("UNET_PX_BPC", 2);
        p.per = (p.ntiles + slots - 1) / slots;
        p.grid_x = (unsigned)((p.ntiles + p.per - 1) / p.per);
        p.grid_y = 1;
        p.pd = lab_knob("UNET_PX_PD", 2);
        return p;
    } else {
        // split precision with >= 256 outputs: one 256-column tile (two blocks per CU), so the
        // depthwise and its halo are evaluated once per pixel tile instead of once per 128 columns,
        // and the 64 x 64 level's 512 pixel tiles fill the 512 block slots in one round
        p.route = has_pkx && rk_x6_supported(mode, cin) ? SEP_RK_X6 : SEP_RK;
        p.bn = cout <= 64 ? 64 : (p.route == SEP_RK_X6 && cout >= 256 ? 256 : 128);
    }
    p.grid_y = (unsigned)cdiv(cout, p.bn);
    return p;
}

// ---------------------------------------------------------------------------- backward ----
// 64 outputs (the 256 x 256 level) or 128 (the 128 x 128 level: 142 KB of LDS; isolated it is slower than
// the separate launches, 224 vs 188 us in tools/bench_sepwgrad.py, but it lets the forward skip the y
// store -- the engine chooses per level)
inline bool sep_bwd_supported(int mode, int c0, int c1, int n, int h, int w, int cout) {
    if (n <= 0 || h <= 0 || w <= 0 || (cout != 64 && cout != 128)) return false;
    if (mode != UNET_VIEW_PLAIN && mode != UNET_VIEW_BNRELU && mode != UNET_VIEW_CONCAT) return false;
    const int C = view_channels(mode, c0, c1);
    if (C <= 0 || C % CI || h % TH || w % TW) return false;
    if (mode == UNET_VIEW_CONCAT && c0 % 4) return false;
    const int64_t M = (int64_t)n * h * w;
    return M * C < (int64_t(1) << 31) && M * cout < (int64_t(1) << 31);
}

// Each block walks a run of tps pixel tiles of one ci group and leaves one slab per gradient; S slices:
// two blocks per CU (77 KB of LDS each), a multiple of 8 (the XCD map).  (Fewer blocks, leaving CUs to the
// main stream: -1.7 / -0.3 % img/s in round 2; 2-8x as many, finer runs: no gain,
// profiles/r3m_fb_split_ab.log.)  Workspace: pw slabs [S][cin][cout] at 0, dw slabs [S][9][cin] at dw_slab_off.
struct SepBwdPlan {
    int tiles, ncig, S, tps, blocks;
    size_t dw_slab_off, bytes;
};
inline SepBwdPlan sep_bwd_plan(int n, int h, int w, int cin, int cout, int cus) {
    SepBwdPlan p;
    p.tiles = n * (h / BTH) * (w / BTW);
    p.ncig = cin / CI;
    p.S = (int)cdiv(cdiv(2 * cus, p.ncig), 8) * 8;
    p.tps = (int)cdiv(p.tiles, p.S);
    p.blocks = p.S * p.ncig;
    p.dw_slab_off = align_up((size_t)p.S * cin * cout * sizeof(float), 256);
    p.bytes = p.dw_slab_off + align_up((size_t)p.S * 9 * cin * sizeof(float), 256);
    return p;
}

}  // namespace sep
}  // namespace unet
