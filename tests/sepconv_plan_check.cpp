// Stand-alone host check of the fused separable-conv policy (csrc/sepconv_plan.h: sep_fwd_supported,
// sep_fwd_plan, sep_bwd_supported, sep_bwd_plan), compiled and run by test_sepconv_plan_host.py; host pass
// only, no GPU.  The pinned rows follow by hand from the launch conditions unet_sepconv_fwd, launch,
// launch_rk, launch_px and sw_plan had before the plan header existed.
// Exit status 0 = every check passed; otherwise the failing lines are printed.
#include <cstdio>

#include "sepconv_plan.h"

using namespace unet;
using namespace unet::sep;

static int g_failed = 0;
#define CHECK(cond)                                               \
    do {                                                          \
        if (!(cond)) {                                            \
            std::printf("FAILED line %d: %s\n", __LINE__, #cond); \
            ++g_failed;                                           \
        }                                                         \
    } while (0)

enum { AUTO = UNET_SEPCONV_AUTO, TILE = UNET_SEPCONV_TILE, RK = UNET_SEPCONV_RK, RK1 = UNET_SEPCONV_RK1 };
enum { PLAIN = UNET_VIEW_PLAIN, BNRELU = UNET_VIEW_BNRELU, POOL = UNET_VIEW_POOL_BNRELU, CONCAT = UNET_VIEW_CONCAT };

struct Row {
    int schedule, mode, c0, c1, cout, n, h, w;
    bool pkx, zsel;
    int route, bn, gx, gy, threads;  // bn .. threads: not pinned for SEP_REFUSED
    bool pool_pass;
    int per = 0;  // PX: tiles per block
};
static const Row kRows[] = {
    // LDS-A-tile schedule: fewer than 64 input or output channels; 64 / 128 / 256 columns, 256 only where
    // the grid keeps >= 256 blocks (1 x 128 x 256 pixels = 256 tiles)
    {AUTO, BNRELU, 16, 0, 64, 1, 8, 16, false, false, SEP_TILE, 64, 1, 1, 256, false},
    {AUTO, PLAIN, 16, 0, 128, 3, 8, 16, false, false, SEP_TILE, 128, 3, 1, 256, false},
    {AUTO, BNRELU, 16, 0, 256, 1, 128, 256, false, false, SEP_TILE, 256, 256, 1, 512, false},
    {AUTO, BNRELU, 16, 0, 256, 1, 120, 256, false, false, SEP_TILE, 128, 240, 2, 256, false},
    {AUTO, BNRELU, 16, 0, 512, 1, 64, 256, false, false, SEP_TILE, 256, 128, 2, 512, false},   // 128 tiles x 2 column tiles
    {AUTO, BNRELU, 16, 0, 512, 127, 8, 16, false, false, SEP_TILE, 128, 127, 4, 256, false},
    {AUTO, CONCAT, 16, 16, 256, 1, 8, 16, false, false, SEP_TILE, 128, 1, 2, 256, false},
    {AUTO, BNRELU, 8, 0, 8, 1, 8, 16, false, false, SEP_TILE, 64, 1, 1, 256, false},
    {AUTO, BNRELU, 64, 0, 32, 1, 8, 16, true, false, SEP_TILE, 64, 1, 1, 256, false},          // 32 outputs
    // ... with the pooling selection as a pass of its own
    {AUTO, BNRELU, 16, 0, 64, 3, 8, 16, false, true, SEP_TILE, 64, 3, 1, 256, true},
    {TILE, BNRELU, 64, 0, 128, 3, 8, 16, true, true, SEP_TILE, 128, 3, 1, 256, true},           // forced
    {TILE, BNRELU, 256, 0, 256, 2, 64, 64, true, false, SEP_TILE, 128, 64, 2, 256, false},
    // max-pool view with more than 128 outputs keeps the LDS-A-tile kernel
    {AUTO, POOL, 64, 0, 192, 1, 8, 16, false, true, SEP_TILE, 128, 1, 2, 256, true},
    {AUTO, POOL, 256, 0, 512, 16, 32, 32, true, false, SEP_TILE, 256, 128, 2, 512, false},
    // register-A schedule, fp32: 64 / 128 columns, never 256
    {AUTO, BNRELU, 64, 0, 64, 1, 8, 16, false, false, SEP_RK, 64, 1, 1, 256, false},
    {AUTO, BNRELU, 64, 0, 128, 3, 8, 16, false, true, SEP_RK, 128, 3, 1, 256, false},
    {AUTO, BNRELU, 96, 0, 192, 2, 8, 32, false, false, SEP_RK, 128, 4, 2, 256, false},
    {AUTO, BNRELU, 256, 0, 256, 1, 16, 32, false, false, SEP_RK, 128, 4, 2, 256, false},
    {AUTO, POOL, 64, 0, 128, 2, 8, 16, true, true, SEP_RK, 128, 2, 1, 256, false},              // max-pool view: no x6
    {AUTO, POOL, 128, 0, 64, 1, 16, 32, true, false, SEP_RK, 64, 4, 1, 256, false},
    {AUTO, PLAIN, 68, 0, 100, 1, 8, 16, true, false, SEP_RK, 128, 1, 1, 256, false},            // Cin % 16 != 0: no x6
    {RK, BNRELU, 64, 0, 128, 1, 8, 16, false, false, SEP_RK, 128, 1, 1, 256, false},             // no planes: no px
    // split precision: 64 / 128 columns, 256 from 256 outputs
    {AUTO, BNRELU, 64, 0, 64, 3, 8, 16, true, true, SEP_RK_X6, 64, 3, 1, 256, false},            // no px for 64 -> 64
    {AUTO, BNRELU, 128, 0, 128, 1, 8, 16, true, false, SEP_RK_X6, 128, 1, 1, 256, false},        // nor 128 -> 128 without zsel
    {AUTO, BNRELU, 128, 0, 64, 1, 8, 16, true, true, SEP_RK_X6, 64, 1, 1, 256, false},
    {AUTO, BNRELU, 96, 0, 192, 2, 8, 32, true, false, SEP_RK_X6, 128, 4, 2, 256, false},
    {AUTO, BNRELU, 64, 0, 256, 1, 16, 32, true, true, SEP_RK_X6, 256, 4, 1, 256, false},
    {AUTO, BNRELU, 64, 0, 320, 2, 8, 16, true, false, SEP_RK_X6, 256, 2, 2, 256, false},
    {RK, CONCAT, 72, 56, 128, 1, 8, 16, true, false, SEP_RK_X6, 128, 1, 1, 256, false},          // c0 % 16 != 0: no px
    {RK1, BNRELU, 64, 0, 128, 1, 8, 16, true, false, SEP_RK_X6, 128, 1, 1, 256, false},
    {RK1, BNRELU, 128, 0, 128, 7, 88, 208, true, true, SEP_RK_X6, 128, 1001, 1, 256, false},
    // persistent: under AUTO 128 outputs from 64 inputs or with the pooling selection; under RK all four pairs
    {AUTO, BNRELU, 64, 0, 128, 3, 8, 16, true, false, SEP_PX, 128, 3, 1, 256, false, 1},
    {AUTO, BNRELU, 128, 0, 128, 7, 88, 208, true, true, SEP_PX, 128, 501, 1, 256, false, 2},    // 1001 tiles
    {AUTO, CONCAT, 32, 32, 128, 1, 8, 16, true, false, SEP_PX, 128, 1, 1, 256, false, 1},
    {RK, CONCAT, 32, 32, 64, 1, 8, 16, true, false, SEP_PX, 64, 1, 1, 256, false, 1},
    {RK, PLAIN, 64, 0, 128, 1, 8, 16, true, true, SEP_PX, 128, 1, 1, 256, false, 1},
    {RK, PLAIN, 128, 0, 64, 3, 8, 16, true, true, SEP_PX, 64, 3, 1, 256, false, 1},
    {RK, CONCAT, 64, 64, 128, 3, 8, 16, true, false, SEP_PX, 128, 3, 1, 256, false, 1},
    {RK, BNRELU, 64, 0, 64, 513, 8, 16, true, false, SEP_PX, 64, 257, 1, 256, false, 2},        // 513 tiles, 512 slots
    // forced register-A schedule on a shape without such a kernel
    {RK, PLAIN, 4, 0, 64, 1, 8, 16, false, false, SEP_REFUSED},
    {RK, BNRELU, 64, 0, 32, 1, 8, 16, false, false, SEP_REFUSED},
    {RK, POOL, 64, 0, 192, 1, 8, 16, false, true, SEP_REFUSED},
};

// The 18 conv blocks of the 256 x 256 network (filters 64 .. 512, bottleneck 1024) as the train step calls
// unet_sepconv_fwd, at batch 16; the batch-32 grids follow from `tiles`.  Split planes for every block of
// >= 64 input channels, the pooling selection for every encoder block2 (enc2_block1 /
// enc2_block2 persistent, the 64 x 64 level on the 256-column split-precision tile, the image block on the
// LDS-A-tile kernel).  The two bottleneck blocks (16 x 16) run unfused in the step; their rows pin what a
// direct call takes.
struct Net {
    const char* name;
    int mode, c0, c1, cout, hw;
    bool pkx, zsel;
    int route, bn, gy;
};
static const Net kNet[] = {
    {"enc1_block1", PLAIN, 4, 0, 64, 256, false, false, SEP_TILE, 64, 1},
    {"enc1_block2", BNRELU, 64, 0, 64, 256, true, true, SEP_RK_X6, 64, 1},
    {"enc2_block1", BNRELU, 64, 0, 128, 128, true, false, SEP_PX, 128, 1},
    {"enc2_block2", BNRELU, 128, 0, 128, 128, true, true, SEP_PX, 128, 1},
    {"enc3_block1", BNRELU, 128, 0, 256, 64, true, false, SEP_RK_X6, 256, 1},
    {"enc3_block2", BNRELU, 256, 0, 256, 64, true, true, SEP_RK_X6, 256, 1},
    {"enc4_block1", BNRELU, 256, 0, 512, 32, true, false, SEP_RK_X6, 256, 2},
    {"enc4_block2", BNRELU, 512, 0, 512, 32, true, true, SEP_RK_X6, 256, 2},
    {"bneck_block1", BNRELU, 512, 0, 1024, 16, true, false, SEP_RK_X6, 256, 4},
    {"bneck_block2", BNRELU, 1024, 0, 1024, 16, true, false, SEP_RK_X6, 256, 4},
    {"dec4_block1", CONCAT, 512, 512, 512, 32, true, false, SEP_RK_X6, 256, 2},
    {"dec4_block2", BNRELU, 512, 0, 512, 32, true, false, SEP_RK_X6, 256, 2},
    {"dec3_block1", CONCAT, 256, 256, 256, 64, true, false, SEP_RK_X6, 256, 1},
    {"dec3_block2", BNRELU, 256, 0, 256, 64, true, false, SEP_RK_X6, 256, 1},
    {"dec2_block1", CONCAT, 128, 128, 128, 128, true, false, SEP_RK_X6, 128, 1},
    {"dec2_block2", BNRELU, 128, 0, 128, 128, true, false, SEP_RK_X6, 128, 1},
    {"dec1_block1", CONCAT, 64, 64, 64, 256, true, false, SEP_RK_X6, 64, 1},
    {"dec1_block2", BNRELU, 64, 0, 64, 256, true, false, SEP_RK_X6, 64, 1},
};

// The forward shapes tests/test_ops_gpu.py runs, (mode, n, h, w, c0, c1, cout): SEP_CASES (schedules AUTO
// and TILE, and RK for >= 64 input channels, without split planes), the cases of
// test_fused_sepconv_split_precision (AUTO, with planes) and PX_CASES (RK1 and RK, with planes).
struct Shape {
    int mode, n, h, w, c0, c1, cout;
    bool zsel = false;
};
static const Shape kSepCases[] = {
    {0, 2, 16, 32, 16, 0, 64}, {1, 2, 8, 16, 64, 0, 128},  {1, 1, 16, 16, 128, 0, 96},  {2, 2, 8, 16, 32, 0, 64},
    {3, 2, 8, 32, 32, 32, 64}, {3, 1, 16, 16, 16, 16, 256}, {1, 1, 8, 16, 8, 0, 8},      {1, 2, 8, 32, 96, 0, 192},
    {3, 1, 16, 16, 64, 68, 64}, {0, 1, 8, 16, 68, 0, 100},  {1, 1, 16, 32, 256, 0, 256}, {2, 2, 8, 16, 64, 0, 128},
    {2, 1, 16, 32, 128, 0, 64}, {1, 4, 128, 128, 64, 0, 192}, {1, 1, 8, 16, 64, 0, 64},  {1, 3, 8, 16, 64, 0, 64},
    {3, 3, 8, 16, 64, 64, 128},
};
static const Shape kX6Cases[] = {
    {1, 2, 8, 16, 64, 0, 64},   {1, 1, 16, 32, 128, 0, 128},  {3, 1, 16, 16, 64, 64, 64}, {0, 2, 8, 32, 96, 0, 192},
    {1, 1, 8, 16, 256, 0, 256}, {3, 1, 8, 16, 256, 256, 512}, {1, 2, 8, 16, 64, 0, 320},
};
static const Shape kPxCases[] = {
    {1, 2, 8, 16, 64, 0, 128, true},     {1, 3, 64, 96, 64, 0, 128, false},   {1, 7, 88, 208, 128, 0, 128, true},
    {3, 2, 32, 64, 64, 64, 64, false},   {3, 1, 16, 32, 64, 64, 128, false},  {0, 2, 64, 64, 128, 0, 64, true},
    {1, 4, 128, 128, 128, 0, 128, true}, {3, 2, 256, 256, 64, 64, 64, false}, {1, 2, 256, 256, 64, 0, 64, true},
    {1, 1, 8, 16, 64, 0, 64, true},      {3, 3, 8, 16, 64, 64, 128, false},
};
// SW_CASES (mode, n, h, w, c0, c1, cout) with the plan at 256 CUs: tiles, ci groups, slices, tiles per slice
struct SwRow {
    int mode, n, h, w, c0, c1, cout, tiles, ncig, S, tps;
};
static const SwRow kSwCases[] = {
    {1, 2, 8, 16, 64, 0, 64, 4, 1, 512, 1},     {1, 1, 16, 32, 64, 0, 64, 8, 1, 512, 1},
    {0, 2, 8, 32, 64, 0, 64, 8, 1, 512, 1},     {3, 1, 16, 16, 32, 32, 64, 4, 1, 512, 1},
    {3, 2, 8, 16, 36, 28, 64, 4, 1, 512, 1},    {3, 1, 16, 32, 64, 64, 64, 8, 2, 256, 1},
    {3, 1, 8, 16, 128, 128, 64, 2, 4, 128, 1},  {1, 3, 64, 96, 64, 0, 64, 288, 1, 512, 1},
    {1, 2, 16, 32, 128, 0, 128, 16, 2, 256, 1}, {3, 1, 16, 32, 128, 128, 128, 8, 4, 128, 1},
    {1, 1, 8, 16, 64, 0, 64, 2, 1, 512, 1},     {1, 3, 8, 16, 64, 0, 64, 6, 1, 512, 1},
};

static bool g_seen[SEP_PX + 1][3];  // route x {64, 128, 256} columns, over the shapes of the op tests
static SepFwdPlan plan_of(int schedule, const Shape& s, bool pkx, bool zsel) {
    CHECK(sep_fwd_supported(s.mode, s.c0, s.c1, s.n, s.h, s.w, s.cout));
    const SepFwdPlan p = sep_fwd_plan(schedule, s.mode, s.c0, s.c1, s.cout, s.n, s.h, s.w, pkx, zsel);
    if (p.route != SEP_REFUSED) g_seen[p.route][p.bn / 128] = true;
    return p;
}

// what every plan must satisfy; returns the route
static int check_plan(int schedule, int mode, int c0, int c1, int cout, int n, int h, int w, bool pkx, bool zsel) {
    const SepFwdPlan p = sep_fwd_plan(schedule, mode, c0, c1, cout, n, h, w, pkx, zsel);
    const int cin = c0 + (mode == CONCAT ? c1 : 0);
    const long long mt = (long long)n * (h / 8) * (w / 16);
    CHECK(p.route >= SEP_REFUSED && p.route <= SEP_PX);
    if (p.route == SEP_REFUSED) {
        CHECK(schedule == RK);
        return p.route;
    }
    CHECK((long long)p.grid_x * p.grid_y >= 1);
    CHECK(p.bn == 64 || p.bn == 128 || p.bn == 256);
    CHECK(p.pool_pass == (zsel && p.route == SEP_TILE));
    CHECK(schedule != TILE || p.route == SEP_TILE);
    CHECK(schedule != RK || p.route != SEP_TILE);
    CHECK(schedule != RK1 || p.route != SEP_PX);
    // persistent exactly where: planes, 64 / 128 channels in and out, no max-pool view, a concat split at a
    // k-stage, and under AUTO only the shapes measured faster inside the step
    CHECK((p.route == SEP_PX) ==
          ((schedule == AUTO || schedule == RK) && pkx && mode != POOL && (cin == 64 || cin == 128) &&
           (cout == 64 || cout == 128) && (mode != CONCAT || c0 % 16 == 0) &&
           (schedule == RK || (cout == 128 && (cin == 64 || zsel)))));
    if (p.route == SEP_PX) {
        const int slots = 512;
        CHECK(pkx && p.ntiles == mt && p.grid_y == 1 && p.threads == 256 && p.bn == cout && p.pd == 2);
        CHECK((int)p.grid_x <= slots && (long long)p.grid_x * p.per >= p.ntiles &&
              p.ntiles > (long long)(p.grid_x - 1) * p.per);
        CHECK((cin == 64 || cin == 128) && (cout == 64 || cout == 128) && mode != POOL);
        CHECK(schedule == RK || (cout == 128 && (cin == 64 || zsel)));
        return p.route;
    }
    CHECK(p.grid_x == mt && (long long)p.grid_y * p.bn >= cout && (long long)(p.grid_y - 1) * p.bn < cout);
    CHECK(p.bn >= 128 || cout <= 64);
    if (p.route == SEP_TILE) {
        CHECK(p.threads == (p.bn == 256 ? 512 : 256));
        // 256 columns exactly where there are more than 128 outputs and the grid keeps >= 256 blocks
        CHECK((p.bn == 256) == (cout > 128 && mt * ((cout + 255) / 256) >= 256));
    } else {
        CHECK(p.threads == 256 && cin >= 64 && cout >= 64 && (mode != POOL || cout <= 128));
        CHECK((p.route == SEP_RK_X6) == (pkx && mode != POOL && cin % 16 == 0));
        CHECK((p.bn == 256) == (p.route == SEP_RK_X6 && cout >= 256));  // 256 columns only with split precision
    }
    return p.route;
}

int main() {
    for (const Row& r : kRows) {
        CHECK(sep_fwd_supported(r.mode, r.c0, r.c1, r.n, r.h, r.w, r.cout));
        const SepFwdPlan p = sep_fwd_plan(r.schedule, r.mode, r.c0, r.c1, r.cout, r.n, r.h, r.w, r.pkx, r.zsel);
        const bool ok = p.route == r.route &&
                        (r.route == SEP_REFUSED || (p.bn == r.bn && (int)p.grid_x == r.gx && (int)p.grid_y == r.gy &&
                                                    p.threads == r.threads && p.pool_pass == r.pool_pass)) &&
                        (r.route != SEP_PX || (p.per == r.per && p.ntiles == r.n * (r.h / 8) * (r.w / 16)));
        if (!ok)
            std::printf("schedule %d mode %d %d+%d -> %d, %d x %d x %d, planes %d zsel %d: route %d bn %d grid %u x %u "
                        "threads %d per %d pool_pass %d\n", r.schedule, r.mode, r.c0, r.c1, r.cout, r.n, r.h, r.w,
                        (int)r.pkx, (int)r.zsel, p.route, p.bn, p.grid_x, p.grid_y, p.threads, p.per, (int)p.pool_pass);
        CHECK(ok);
    }
    for (int batch : {16, 32})
        for (const Net& b : kNet) {
            CHECK(sep_fwd_supported(b.mode, b.c0, b.c1, batch, b.hw, b.hw, b.cout));
            const SepFwdPlan p = sep_fwd_plan(AUTO, b.mode, b.c0, b.c1, b.cout, batch, b.hw, b.hw, b.pkx, b.zsel);
            const int tiles = batch * (b.hw / 8) * (b.hw / 16);
            // the persistent blocks: 2048 / 4096 tiles over 512 block slots, 4 / 8 tiles per block
            const bool ok = p.route == b.route && p.bn == b.bn && (int)p.grid_y == b.gy && p.pool_pass == false &&
                            (b.route == SEP_PX ? (int)p.grid_x == 512 && p.per == tiles / 512 && p.ntiles == tiles
                                               : (int)p.grid_x == tiles);
            if (!ok) std::printf("%s batch %d: route %d bn %d grid %u x %u per %d\n", b.name, batch, p.route, p.bn, p.grid_x, p.grid_y, p.per);
            CHECK(ok);
        }

    // the op tests' shapes: every route and tile width the product can take is run by one of them
    for (const Shape& s : kSepCases) {
        const int cin = s.c0 + s.c1;
        CHECK(plan_of(TILE, s, false, false).route == SEP_TILE);
        CHECK(plan_of(AUTO, s, false, false).route == (cin >= 64 && s.cout >= 64 ? SEP_RK : SEP_TILE));
        if (cin >= 64) CHECK(plan_of(RK, s, false, false).route == SEP_RK);
    }
    for (const Shape& s : kX6Cases) {
        CHECK(plan_of(AUTO, s, false, false).route == SEP_RK);
        CHECK(plan_of(AUTO, s, true, false).route == SEP_RK_X6);
    }
    for (const Shape& s : kPxCases) {
        CHECK(plan_of(RK1, s, true, s.zsel).route == SEP_RK_X6);
        CHECK(plan_of(RK, s, true, s.zsel).route == SEP_PX);
    }
    for (int bn = 0; bn < 3; ++bn) {
        CHECK(g_seen[SEP_TILE][bn] && g_seen[SEP_RK_X6][bn]);
        CHECK(g_seen[SEP_RK][bn] == (bn < 2) && g_seen[SEP_PX][bn] == (bn < 2));  // no such kernel at 256 columns
    }
    for (const SwRow& r : kSwCases) {
        CHECK(sep_bwd_supported(r.mode, r.c0, r.c1, r.n, r.h, r.w, r.cout));
        const int cin = r.c0 + r.c1;
        const SepBwdPlan p = sep_bwd_plan(r.n, r.h, r.w, cin, r.cout, 256);
        CHECK(p.tiles == r.tiles && p.ncig == r.ncig && p.S == r.S && p.tps == r.tps && p.blocks == r.S * r.ncig);
        CHECK(p.dw_slab_off == (size_t)r.S * cin * r.cout * 4 && p.bytes == p.dw_slab_off + (size_t)r.S * 9 * cin * 4);
    }
    // dec1_block1 at batch 16 on 256 and 304 CUs: 16 * 64 * 16 = 16384 tiles of 4 x 16 pixels, two ci groups
    {
        const SepBwdPlan a = sep_bwd_plan(16, 256, 256, 128, 64, 256), b = sep_bwd_plan(16, 256, 256, 128, 64, 304);
        CHECK(a.tiles == 16384 && a.ncig == 2 && a.S == 256 && a.tps == 64 && a.blocks == 512);
        CHECK(b.S == 304 && b.tps == 54 && b.blocks == 608);
    }

    // sweeps: the plan is total over the supported shapes and keeps its invariants
    const int kCh[] = {4, 8, 16, 36, 60, 64, 68, 72, 96, 100, 128, 192, 256, 320, 512, 1024};
    const int kNHW[][3] = {{1, 8, 16}, {3, 8, 16}, {1, 16, 32}, {2, 64, 64}, {1, 128, 256}, {7, 88, 208},
                           {127, 8, 16}, {16, 32, 32}, {16, 128, 128}, {32, 256, 256}};
    long long plans = 0, supported_bwd = 0;
    for (int mode = PLAIN; mode <= CONCAT; ++mode)
        for (int cin : kCh)
            for (int cout : kCh)
                for (const auto& d : kNHW)
                    for (int split = 0; split < (mode == CONCAT ? 3 : 1); ++split) {
                        // concat: the first source takes half, a quarter rounded to 4, or all but 4 channels
                        const int c0 = mode != CONCAT ? cin : split == 0 ? cin / 2 : split == 1 ? (cin / 4 + 3) / 4 * 4 : cin - 4;
                        const int c1 = mode != CONCAT ? 0 : cin - c0;
                        if (c0 <= 0 || (mode == CONCAT && c1 <= 0)) continue;
                        const int n = d[0], h = d[1], w = d[2];
                        const bool fs = sep_fwd_supported(mode, c0, c1, n, h, w, cout);
                        const long long M = (long long)n * h * w, lim = 1ll << 31;
                        CHECK(fs == (c0 % 4 == 0 && M * cin * (mode == POOL ? 4 : 1) < lim && M * cout < lim));
                        if (fs)
                            for (int schedule = AUTO; schedule <= RK1; ++schedule)
                                for (int f = 0; f < 4; ++f) {
                                    check_plan(schedule, mode, c0, c1, cout, n, h, w, f & 1, f & 2);
                                    ++plans;
                                }
                        // backward: the workspace query of the library is plan.bytes where a PLAIN view of cin
                        // channels is supported (the most any view of cin channels can be), else 0
                        const bool bs = sep_bwd_supported(mode, c0, c1, n, h, w, cout);
                        const bool any = sep_bwd_supported(PLAIN, cin, 0, n, h, w, cout);
                        CHECK(!bs || any);
                        CHECK(any == (cin % 64 == 0 && (cout == 64 || cout == 128) && M * cin < lim && M * cout < lim));
                        CHECK(bs == (any && mode != POOL && c0 % 4 == 0));
                        if (!any) continue;
                        ++supported_bwd;
                        for (int cus : {256, 304, 64}) {
                            const SepBwdPlan p = sep_bwd_plan(n, h, w, cin, cout, cus);
                            CHECK(p.tiles == M / 64 && p.ncig == cin / 64 && p.blocks == p.S * p.ncig);
                            CHECK(p.S % 8 == 0 && p.S * p.ncig >= 2 * cus && (p.S - 8) * p.ncig < 2 * cus);
                            CHECK(p.tps >= 1 && (long long)p.tps * p.S >= p.tiles && (long long)(p.tps - 1) * p.S < p.tiles);
                            CHECK(p.dw_slab_off % 256 == 0 && p.dw_slab_off >= (size_t)p.S * cin * cout * 4);
                            CHECK(p.bytes == p.dw_slab_off + align_up((size_t)p.S * 9 * cin * 4, 256));
                        }
                    }
    CHECK(plans > 100000 && supported_bwd > 100);
    // shapes no view supports: granularity, sign, and the 2^31 index bounds (the 2 x 2 source of a max-pool view)
    CHECK(!sep_fwd_supported(BNRELU, 64, 0, 1, 12, 16, 64) && !sep_fwd_supported(BNRELU, 64, 0, 1, 8, 24, 64));
    CHECK(!sep_fwd_supported(BNRELU, 62, 0, 1, 8, 16, 64) && !sep_fwd_supported(BNRELU, 64, 0, 1, 8, 16, 66));
    CHECK(!sep_fwd_supported(CONCAT, 34, 30, 1, 8, 16, 64) && !sep_fwd_supported(BNRELU, 64, 0, 0, 8, 16, 64));
    CHECK(sep_fwd_supported(BNRELU, 64, 0, 127, 512, 512, 64) && !sep_fwd_supported(BNRELU, 64, 0, 128, 512, 512, 64));
    CHECK(sep_fwd_supported(POOL, 64, 0, 31, 512, 512, 64) && !sep_fwd_supported(POOL, 64, 0, 32, 512, 512, 64));
    CHECK(!sep_bwd_supported(BNRELU, 64, 0, 128, 512, 512, 64) && !sep_bwd_supported(BNRELU, 0, 0, 1, 8, 16, 64));
    CHECK(!sep_bwd_supported(BNRELU, 64, 0, 1, 8, 16, 96) && !sep_bwd_supported(BNRELU, 64, 0, 1, 12, 16, 64));
    if (g_failed) return 1;
    std::printf("sepconv_plan_check OK\n");
    return 0;
}
