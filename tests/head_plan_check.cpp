// Stand-alone host check of the head's route policy (csrc/head_plan.h: head_fwd_plan, head_bwd_plan, the
// fused workspace layout, the slab query), compiled and run by test_head_plan_host.py; host pass only, no
// GPU.  The pinned rows follow by hand from the launch conditions csrc/head.hip had before it was split.
// Exit status 0 = every check passed; otherwise the failing lines are printed.
#include <cstdio>

#include "gemm_plan.h"  // wgrad_plan: the weight-gradient scratch of the dlogit routes
#include "head_plan.h"

using namespace unet;

static int g_failed = 0;
#define CHECK(cond)                                               \
    do {                                                          \
        if (!(cond)) {                                            \
            std::printf("FAILED line %d: %s\n", __LINE__, #cond); \
            ++g_failed;                                           \
        }                                                         \
    } while (0)

// grid / tp: -1 = not pinned by this row
struct Row {
    int c0, ncls;
    long long M;
    bool src_al;
    int fwd, fwd_grid, tp, bwd, bwd_grid;
    bool runs_bwd = true;  // kOps: the test behind the row also runs the backward
};
static const Row kRows[] = {
    {64, 1, 1048576, true, HEAD_FWD_BIN, 4096, -1, HEAD_BWD_BIN_FUSED, 1024},
    {64, 21, 524288, true, HEAD_FWD_MFMA, 2048, -1, HEAD_BWD_MC_FUSED, 512},
    {64, 1, 129, true, HEAD_FWD_BIN, 3, -1, HEAD_BWD_BIN_FUSED, 1},
    {64, 1, 129, false, HEAD_FWD_GENERAL, 2, 128, HEAD_BWD_BIN_FUSED, 1},
    {48, 1, 129, true, HEAD_FWD_GENERAL, 1, 170, HEAD_BWD_GENERAL, -1},
    {48, 21, 129, true, HEAD_FWD_REG, -1, -1, HEAD_BWD_GENERAL, -1},
    {128, 21, 63, true, HEAD_FWD_GENERAL, 2, 32, HEAD_BWD_MC_REG, -1},
    {64, 32, 129, true, HEAD_FWD_MFMA, -1, -1, HEAD_BWD_MC_REG, -1},
    {64, 21, 129, false, HEAD_FWD_REG, -1, -1, HEAD_BWD_MC_FUSED, -1},
    {4, 3, 300, true, HEAD_FWD_REG, -1, -1, HEAD_BWD_MC_FUSED, 2},
};

// The heads tests/test_ops_gpu.py and tests/test_fenced_ops_gpu.py run, as (Cin, classes, pixels, src0
// aligned) with the routes they take: every forward route is reached by a test that runs the forward,
// every backward route by a test that runs the backward (rows of forward-only tests end in `false`).
static const Row kOps[] = {
    // test_head_fwd_binary (Cin 32 .. 256 and 48; 240, 15, 7680, 1, 127, 129 pixels)
    {32, 1, 240, true, HEAD_FWD_BIN, 2, -1, HEAD_BWD_BIN_FUSED, -1, false},
    {256, 1, 7680, true, HEAD_FWD_BIN, 480, -1, HEAD_BWD_BIN_FUSED, -1, false},
    {48, 1, 127, true, HEAD_FWD_GENERAL, 1, 170, HEAD_BWD_GENERAL, -1, false},
    // test_head_dice (240 pixels), test_head_bwd_bnstats (768, 1517 pixels: dice and backward only)
    {64, 1, 240, true, HEAD_FWD_BIN, 4, -1, HEAD_BWD_BIN_FUSED, 1},
    {64, 21, 240, true, HEAD_FWD_MFMA, 2, -1, HEAD_BWD_MC_FUSED, 1},
    {64, 1, 768, true, HEAD_FWD_BIN, 12, -1, HEAD_BWD_BIN_FUSED, 3},
    {64, 5, 1517, true, HEAD_FWD_MFMA, 12, -1, HEAD_BWD_MC_FUSED, 6},
    // test_head_multiclass_shapes (classes 2, 3, 8, 21, 32)
    {64, 21, 7680, true, HEAD_FWD_MFMA, 60, -1, HEAD_BWD_MC_FUSED, 30},
    {64, 32, 7680, true, HEAD_FWD_MFMA, 60, -1, HEAD_BWD_MC_REG, 30},
    {16, 2, 286, true, HEAD_FWD_MFMA, 3, -1, HEAD_BWD_MC_FUSED, 2},
    {48, 8, 323, true, HEAD_FWD_REG, 2, -1, HEAD_BWD_GENERAL, 2},
    {128, 3, 63, true, HEAD_FWD_GENERAL, 2, 32, HEAD_BWD_MC_REG, 1},
    {4, 3, 300, true, HEAD_FWD_REG, 2, -1, HEAD_BWD_MC_FUSED, 2},
    {4, 32, 300, true, HEAD_FWD_REG, 2, -1, HEAD_BWD_MC_REG, 2},
    {64, 21, 646, true, HEAD_FWD_MFMA, 6, -1, HEAD_BWD_MC_FUSED, 3},
    {16, 8, 127, true, HEAD_FWD_MFMA, 1, -1, HEAD_BWD_MC_FUSED, 1},
    {48, 21, 129, true, HEAD_FWD_REG, 1, -1, HEAD_BWD_GENERAL, 1},
    // test_head_fwd_skewed_src (src0 4 bytes off, 129 pixels; forward only)
    {16, 1, 129, false, HEAD_FWD_GENERAL, 1, 256, HEAD_BWD_BIN_FUSED, -1, false},
    {64, 1, 129, false, HEAD_FWD_GENERAL, 2, 128, HEAD_BWD_BIN_FUSED, 1, false},
    {16, 3, 129, false, HEAD_FWD_REG, 1, -1, HEAD_BWD_MC_FUSED, -1, false},
    {64, 3, 129, false, HEAD_FWD_REG, 1, -1, HEAD_BWD_MC_FUSED, 1, false},
    // test_head_bwd_skewed (prob or y_true 4 bytes off, src0 aligned; dice and backward, Cin 64, 129 pixels)
    {64, 1, 129, true, HEAD_FWD_BIN, 3, -1, HEAD_BWD_BIN_FUSED, 1},
    {64, 3, 129, true, HEAD_FWD_MFMA, 2, -1, HEAD_BWD_MC_FUSED, 1},
    {64, 21, 129, true, HEAD_FWD_MFMA, 2, -1, HEAD_BWD_MC_FUSED, 1},
};

static void check_row(const Row& r, bool* fwd_seen, bool* bwd_seen) {
    const HeadFwdPlan f = head_fwd_plan(r.c0, r.ncls, r.M, r.src_al, true);
    const HeadBwdPlan b = head_bwd_plan(r.c0, r.ncls, r.M);
    const bool ok = f.route == r.fwd && (r.fwd_grid < 0 || f.grid == r.fwd_grid) && (r.tp < 0 || f.tp == r.tp) &&
                    b.route == r.bwd && (r.bwd_grid < 0 || b.grid == r.bwd_grid);
    if (!ok)
        std::printf("Cin %d classes %d M %lld aligned %d: forward route %d grid %d tp %d, backward route %d grid %d\n",
                    r.c0, r.ncls, r.M, (int)r.src_al, f.route, f.grid, f.tp, b.route, b.grid);
    CHECK(ok);
    if (fwd_seen) {
        fwd_seen[f.route] = true;
        if (r.runs_bwd) bwd_seen[b.route] = true;
    }
}

int main() {
    for (const Row& r : kRows) check_row(r, nullptr, nullptr);
    // the binary vector kernel also wants the kernel pointer aligned
    CHECK(head_fwd_plan(64, 1, 129, true, false).route == HEAD_FWD_GENERAL);
    bool fwd_seen[4] = {}, bwd_seen[4] = {};
    for (const Row& r : kOps) check_row(r, fwd_seen, bwd_seen);
    for (int i = 0; i < 4; ++i) CHECK(fwd_seen[i] && bwd_seen[i]);

    const long long kM[] = {1, 127, 129, 255, 257, 262145, 1 << 20};
    for (int c0 = 4; c0 <= kMaxCin; c0 += 4)
        for (int ncls = 1; ncls <= kMaxCls; ++ncls)
            for (long long M : kM) {
                const HeadBwdPlan b = head_bwd_plan(c0, ncls, M);
                CHECK(b.grid >= 1 && b.grid <= cdiv(M, 256));
                // The workspace holds what the route's layout touches.  The weight-gradient scratch is
                // wgrad_workspace's formula restated over wgrad_plan (gemm_wgrad.hip cannot be built
                // without device code); the column sum's plan is bn_plan.h's, pinned by bn_plan_check.cpp, so the
                // bound is checked for a column-sum need below and above the weight gradient's.
                const WgradPlan w = wgrad_plan(M, c0, ncls);
                const size_t wg = align_up((size_t)w.S * c0 * ncls * sizeof(float), 256);
                for (size_t cs : {(size_t)0, wg + 4096}) {
                    const size_t ws = head_bwd_workspace_bytes(c0, ncls, M, wg, cs);
                    // never below the formula callers have sized their buffers by
                    const size_t fused1024 =
                        (align_up((size_t)1024 * c0 * ncls, 64) + align_up((size_t)1024 * ncls, 64)) * sizeof(float);
                    const size_t gen = align_up((size_t)M * ncls * sizeof(float), 256) + (wg > cs ? wg : cs);
                    CHECK(ws == align_up(fused1024 > gen ? fused1024 : gen, 256));
                    if (b.fused()) {
                        const HeadFusedLayout l = head_fused_layout(b.grid, c0, ncls);
                        CHECK(b.part_b_off == l.part_b_off && l.bytes <= ws);
                        CHECK(b.part_b_off >= (size_t)b.grid * c0 * ncls);                    // part_w fits below part_b
                        CHECK((b.part_b_off + (size_t)b.grid * ncls) * sizeof(float) <= ws);  // part_b fits
                    } else {
                        CHECK(b.dlogit_bytes == align_up((size_t)M * ncls * sizeof(float), 256));
                        CHECK(b.dlogit_bytes + (wg > cs ? wg : cs) <= ws);
                    }
                }
                // one BatchNorm-backward slab per block of a fused route, BNRELU views only
                const int slabs = head_bwd_bnstats_slabs(UNET_VIEW_BNRELU, c0, ncls, M);
                CHECK((slabs > 0) == b.fused() && (!b.fused() || slabs == b.grid));
                CHECK(head_bwd_bnstats_slabs(UNET_VIEW_PLAIN, c0, ncls, M) == 0);
                // forward: the general kernel's dynamic LDS fits, whatever sends a head there
                for (int al = 0; al < 2; ++al) {
                    const HeadFwdPlan f = head_fwd_plan(c0, ncls, M, al != 0, al != 0);
                    CHECK(f.grid >= 1);
                    if (f.route != HEAD_FWD_GENERAL) continue;
                    CHECK(f.tp >= 1 && f.tp == head_fwd_tp(c0, ncls > 1) && f.lds <= 64 * 1024);
                    CHECK(f.grid <= cdiv(M, f.tp));
                }
            }
    CHECK(head_bwd_bnstats_slabs(UNET_VIEW_BNRELU, 6, 1, 129) == 0 && head_bwd_bnstats_slabs(UNET_VIEW_BNRELU, 64, 0, 129) == 0 &&
          head_bwd_bnstats_slabs(UNET_VIEW_BNRELU, 260, 1, 129) == 0 && head_bwd_bnstats_slabs(UNET_VIEW_BNRELU, 64, 33, 129) == 0);
    if (g_failed) return 1;
    std::printf("head_plan_check OK\n");
    return 0;
}
