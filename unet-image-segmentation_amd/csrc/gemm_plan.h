// Operand / epilogue modes and tile policy of the rows and weight-gradient GEMMs: no device code,
// pure functions of the problem shape (in the lab build they also read lab_knob values), pinned by tests/gemm_plan_check.cpp.
#pragma once
#include "common.h"  // cdiv, lab_knob

namespace unet {

constexpr int BK = 16;  // k (rows GEMM) or m (weight gradient) per stage of the 16-deep kernels

// A_BNBWD: A = dz of a BatchNorm + ReLU (+ dropout) output, formed on load from the incoming
// gradient da (a.src0) and the raw pre-BN z: g = da * drop * [z*sc+sh > 0],
// dz = sc * (g - p - (z - mu) * q) with per-channel (mu, p, q) = coef[0..3C) (see bn_bwd.hip).
enum { A_PLAIN = 0, A_BNRELU = 1, A_UNSHUFFLE = 2, A_BNBWD = 3 };
// E_BNPART: E_STORE, and the stored C is the complete da of a BatchNorm + ReLU block whose raw
// z is g.z (same [M][N] layout): the tile also emits that block's BN-backward partial sums
// bnpart[tile][0][n] = sum g, bnpart[tile][1][n] = sum g * xhat, g = da * [z*sc+sh > 0],
// xhat = (z - mu) * rs (the dwtile.hip STATS format, finished by unet_bn_relu_bwd_stats_finish).
enum { E_STORE = 0, E_STATS = 1, E_SHUFFLE = 2, E_BNPART = 3 };
// W_BNBWD (B operand, vectorised kernel only): B = dz of a BatchNorm + ReLU output formed on load
// from da (b.src0) and the raw z as A_BNBWD does (coef = (mu, p, q)), so the data-gradient
// GEMM need not store dz for this kernel.
enum { W_PLAIN = 0, W_BNRELU = 1, W_UNSHUFFLE = 2, W_BNBWD = 3 };


// Tile configuration of the vectorised rows GEMM: BN columns x BK k per stage (BM = 128).
// Chosen per operand mode from lab timings (tools/lab/gemm_lab.hip) on the U-Net shapes:
// the BatchNorm-backward data gradient forms its A operand per N-tile, so it prefers the
// 256-wide tile when the grid still fills the chip, and BK = 32 otherwise; plain operands
// take BK = 32 from K = 256 on.  Lab build: UNET_ROWS_BN / UNET_ROWS_BK override (tuning only).
struct RowsCfg {
    int bn, bk;
    int bm = 128;
};
inline RowsCfg rows_cfg(int amode, int64_t M, int K, int N) {
    const int env_bn = lab_knob("UNET_ROWS_BN", 0);
    if (env_bn > 0) return RowsCfg{env_bn, lab_knob("UNET_ROWS_BK", 16)};
    // grids of 128 x 128 tiles that leave CUs idle (the deep levels at small batch: 2048-8192
    // rows; up to one block per CU) take 64-wide N tiles, twice the blocks (<= 256 rather than
    // < 256 blocks: -0.4 % per step at batch 16 and batch 8, profiles/r5d_step_ab.txt nw_*)
    const bool narrow = lab_knob("UNET_ROWS_NARROW", 1) && N > 64 &&
                        cdiv(M, 128) * cdiv(N, 128) < lab_knob("UNET_ROWS_NARROW_LT", 257);
    if (amode == A_BNBWD) {
        // lab: UNET_BNBWD_BK16 = 1 stages BK = 16 (40 KB of LDS instead of 72 KB at 128 columns:
        // co-residency with the side stream's weight-gradient blocks)
        const int bk = lab_knob("UNET_BNBWD_BK16", 0) ? 16 : 32;
        // under-filled grids (the 16 x 16 level at batch 8): 64-row x 128-column tiles instead of
        // 128 x 64, the same block count with half the N-tiles re-forming each dz tile
        // (tools/lab/gemm_lab.hip LAB_BATCH=8, profiles/r5_lab/r5d_rows_b8.log: 76 -> 65.5 us)
        if (narrow && N >= 128 && lab_knob("UNET_BNBWD_BM64", 1)) return RowsCfg{128, 32, 64};
        if (N <= 64 || narrow) return RowsCfg{64, bk};
        if (N >= 256 && cdiv(M, 128) * cdiv(N, 256) >= 512) return RowsCfg{256, 16};
        return RowsCfg{128, bk};
    }
    const int bk32_k = lab_knob("UNET_BK32_MIN_K", 256);  // smallest K that takes BK = 32
    if (N <= 64) return RowsCfg{64, 16};
    // (the ConvT data gradient keeps BK = 16: BK = 32 runs its kernels 5-20 % faster alone but the
    // step slower beside the side stream, profiles/r5d_step_ab.txt bk_*; lab UNET_UNSHUFFLE_BK32)
    const bool bk32 = K >= bk32_k && (amode != A_UNSHUFFLE || lab_knob("UNET_UNSHUFFLE_BK32", 0));
    if (narrow) return RowsCfg{64, bk32 ? 32 : 16};
    return RowsCfg{128, bk32 ? 32 : 16};
}

// Split-precision (bf16x6) rows GEMM: taken when the caller hands pre-split B planes and
// the k-loop is whole 32-deep stages.  (Round 3's form -- B split in every block, 16-deep stages in
// a double buffer at one block per CU -- was load-latency bound and no faster than fp32 MFMA,
// profiles/r3_x6_rows_ab.jsonl; lab UNET_X6 = 0 turns the route off for A/B runs.)
// Grids of fewer than 256 128 x 128 tiles keep the fp32 route, whose narrow tiles fill the chip (the
// bottleneck's data gradient at batch 16, 32 x 4 tiles: 61 vs 77 us, profiles/r6x_rows_x6.txt), and so
// do outputs of <= 64 columns (enc2_block1's data gradient: 98 us, 110 with 128-column split tiles
// half masked, 110 with 64-column ones, profiles/r6v2_x6_n64.txt).
inline bool rows_x6(int amode, int64_t M, int K, int N, bool has_planes) {
    return has_planes && K % 32 == 0 && N > 64 && (amode != A_BNBWD || K <= 512) &&
           cdiv(M, 128) * cdiv(N, 128) >= lab_knob("UNET_X6_MIN_TILES", 256) && lab_knob("UNET_X6", 1) != 0;
}

// Row-tile height of the ConvTranspose data gradient with BatchNorm partials (E_BNPART): 64
// when the 128-row grid holds at most one block per CU (the bottleneck at batch 8: 16 x 16
// blocks of 128 x 64) -- twice the blocks.  The partials are per row tile, so the slab count
// (unet_conv_transpose2x2_bwd_data_bnstats_slabs) follows.  Lab: UNET_CONVT_BM64 = 0 off,
// 2 takes 64 x 128 tiles (the same block count, half the N-tiles).
inline int convt_bnpart_bm(int64_t M, int N) {
    const int mode = lab_knob("UNET_CONVT_BM64", 1);
    return mode && cdiv(M, 128) * cdiv(N, 64) <= 256 ? 64 : 128;
}

// Weight gradient: bp x bq tiles over [P][Q], the pixels split into S slices of mslice rows
struct WgradPlan {
    int bp, bq, tiles, S;
    int64_t mslice;
};
inline WgradPlan wgrad_plan(int64_t M, int P, int Q) {
    WgradPlan w;
    w.bp = P > 64 ? 128 : 64;
    w.bq = Q > 64 ? 128 : 64;
    w.tiles = (int)(cdiv(P, w.bp) * cdiv(Q, w.bq));
    int target = lab_knob("UNET_WGRAD_BLOCKS", 1024);  // ~4 blocks per CU
    if (target < 1) target = 1024;
    int64_t want = cdiv(target, w.tiles);
    int64_t maxs = M / lab_knob("UNET_WGRAD_MINROWS", 512);  // >= 32 k-steps per block: fewer, cheaper slabs
    if (maxs < 1) maxs = 1;
    int64_t S = want < maxs ? want : maxs;
    if (S < 1) S = 1;
    w.mslice = cdiv(cdiv(M, S), BK) * BK;
    w.S = (int)cdiv(M, w.mslice);
    return w;
}

}  // namespace unet
