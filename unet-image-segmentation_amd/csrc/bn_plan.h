// Host policy of the BatchNorm family (bn_fwd.hip, bn_bwd.hip) and of colsum (runtime.hip): how each buffer
// the kernels share is laid out, at what grid each kernel runs and which launches a backward call takes.  No
// kernels, pure functions of the problem; pinned by tests/bn_plan_check.cpp.  Every size query of the C ABI
// and every launch site reads its offsets and grids here, so a query and its launch cannot disagree.
#pragma once
#include "common.h"  // cdiv, align_up, grid_for

namespace unet {
namespace bn {

constexpr int kStatsRows = 128;   // rows of one forward (mean, M2) partial: the pointwise GEMM's tile
constexpr int kChunkParts = 64;   // partials per first-pass block of the finalize
constexpr int kGroupSlabs = 64;   // slabs per first-pass block of the backward statistics' finish
constexpr int kColBlock = 64;     // channels per finalize block, and per arrival counter of either finish
constexpr int kFinishQuads = 16;  // channel quads per block of the backward statistics' finish

// Forward partials buffer of m rows x c channels:
// nblk x c (mean, M2) float pairs | nch x c (S1, S2) double chunk rows | cdiv(c, 64) arrival counters (u32,
// zero at allocation, left zero).  The finalize runs grid (grid_x, nch): one block per 64 channels and chunk.
struct FwdPartials {
    int64_t nblk;
    int nch;
    size_t chunks_off, counter_off, bytes;
    unsigned grid_x;
};
inline FwdPartials fwd_partials(int64_t m, int c) {
    FwdPartials f;
    f.nblk = cdiv(m, kStatsRows);
    f.nch = (int)cdiv(f.nblk, kChunkParts);
    f.chunks_off = align_up((size_t)f.nblk * c * 2 * sizeof(float), 256);
    f.counter_off = f.chunks_off + align_up((size_t)f.nch * c * 2 * sizeof(double), 256);
    f.bytes = f.counter_off + (size_t)cdiv(c, kColBlock) * sizeof(unsigned);
    f.grid_x = (unsigned)cdiv(c, kColBlock);
    return f;
}

// Column-block x row-lane geometry of the column reductions (bn_bwd_reduce_kernel, colsum_kernel): grid
// (ctiles, chunks) of CT column lanes (quads when vec) x 256 / CT row lanes; rows [chunk * rpc, ...).
// vec = false: one column per lane although cols % 4 == 0 (a source that is not 16-byte aligned); it never
// asks for more chunks than the vec plan, so the workspace queries (vec plan) cover it.
struct RedPlan {
    int ctiles, CT;
    int64_t chunks, rpc;
};
inline RedPlan red_plan(int64_t rows, int cols, bool vec = true) {
    RedPlan p;
    const int CQ = vec && cols % 4 == 0 ? cols / 4 : cols;
    p.CT = CQ < 64 ? CQ : 64;
    p.ctiles = (int)cdiv(CQ, p.CT);
    int64_t want = cdiv(1024, p.ctiles);
    int64_t maxc = cdiv(rows, 128);
    p.chunks = want < maxc ? want : maxc;
    if (p.chunks < 1) p.chunks = 1;
    p.rpc = cdiv(rows, p.chunks);
    p.chunks = cdiv(rows, p.rpc);
    return p;
}

// colsum's workspace: chunks x cols floats.  need: what this plan's launch writes; bytes: the query.
struct ColsumPlan {
    RedPlan red;
    size_t need, bytes;
};
inline ColsumPlan colsum_plan(int64_t rows, int cols, bool vec = true) {
    ColsumPlan p;
    p.red = red_plan(rows, cols, vec);
    p.need = (size_t)p.red.chunks * cols * sizeof(float);
    p.bytes = align_up(p.need, 256);
    return p;
}

// Finish of the backward statistics over S slabs of [2][c] floats (c % 4 == 0), in a producer's partials buffer:
// S slabs | nch x 2c double chunk rows | cdiv(c, 64) arrival counters (u32, zero on entry, left zero).
// Grid (grid_x, nch): 16 channel quads x the slabs [64 y, 64 y + 64); with one row the block's sums are final.
struct StatsFinish {
    unsigned grid_x;
    int nch;
    size_t scratch_off, counter_off, bytes;
};
inline StatsFinish stats_finish(int S, int c) {
    StatsFinish f;
    f.grid_x = (unsigned)cdiv(c / 4, kFinishQuads);
    f.nch = (int)cdiv(S, kGroupSlabs);
    f.scratch_off = align_up((size_t)S * 2 * c * sizeof(float), 256);
    f.counter_off = f.scratch_off + align_up((size_t)f.nch * 2 * c * sizeof(double), 256);
    f.bytes = f.counter_off + (size_t)cdiv(c, kColBlock) * sizeof(unsigned);
    return f;
}

// unet_bn_relu_bwd / unet_bn_relu_bwd_stats over m rows x c channels.  Workspace:
// red.chunks slabs of [2][c] floats | the sums [2][c] | the finish's double chunk rows | its counters.
// Every route starts with the reduce launch (grid (red.ctiles, red.chunks)), then
//   BWD_DZ            reduce_slabs, the dgamma / dbeta store and the elementwise dz pass (grid apply_grid)
//   BWD_STATS_FINISH  one finish launch over the slabs (stats_finish(red.chunks, c); the reduce launch zeroes
//                     its ncnt counters)
//   BWD_STATS_SLABS   reduce_slabs and the coefficient kernel: channels that are no whole quads
enum { BWD_DZ, BWD_STATS_FINISH, BWD_STATS_SLABS };
struct BwdWorkspace {
    RedPlan red;
    bool vec;  // float4 lanes
    int route, ncnt, apply_grid;
    size_t sums_off, scratch_off, counter_off, bytes;
};
inline BwdWorkspace bwd_workspace(int64_t m, int c, bool stats_only = false) {
    BwdWorkspace w;
    w.red = red_plan(m, c);
    w.vec = c % 4 == 0;
    w.route = !stats_only ? BWD_DZ : w.vec ? BWD_STATS_FINISH : BWD_STATS_SLABS;
    w.ncnt = w.route == BWD_STATS_FINISH ? (int)cdiv(c, kColBlock) : 0;
    w.apply_grid = grid_for(m * (w.vec ? c / 4 : c));
    w.sums_off = align_up((size_t)w.red.chunks * 2 * c * sizeof(float), 256);
    w.scratch_off = w.sums_off + align_up((size_t)2 * c * sizeof(float), 256);
    w.counter_off = w.scratch_off + align_up((size_t)cdiv(w.red.chunks, kGroupSlabs) * 2 * c * sizeof(double), 256);
    w.bytes = w.counter_off + align_up((size_t)cdiv(c, kColBlock) * sizeof(unsigned), 256);
    return w;
}

}  // namespace bn
}  // namespace unet
