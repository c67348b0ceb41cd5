// Stand-alone host check of the depthwise 3x3 family's policy (csrc/dw_plan.h: dw_plan, dw_filter_plan,
// dw_filter_workspace, dw_bnstats_slabs, dw_bnstats_dwf_ok), compiled and run by test_dw_plan_host.py; host pass
// only, no GPU.  The pinned rows are what dwconv.hip and dwtile.hip decided before the plan header existed: the
// route and tile geometry follow from their launch conditions, the workspace bytes and the BatchNorm slab
// counts were read from that library's two host-only queries (test_dw_plan_host.py asks this library's queries
// for a few of them again).
// Exit status 0 = every check passed; otherwise the failing lines are printed.
#include <cstdio>

#include "dw_plan.h"

using namespace unet;
using namespace unet::dw;

static int g_failed = 0;
#define CHECK(cond)                                               \
    do {                                                          \
        if (!(cond)) {                                            \
            std::printf("FAILED line %d: %s\n", __LINE__, #cond); \
            ++g_failed;                                           \
        }                                                         \
    } while (0)

enum { PLAIN = UNET_VIEW_PLAIN, BNRELU = UNET_VIEW_BNRELU, POOL = UNET_VIEW_POOL_BNRELU, CONCAT = UNET_VIEW_CONCAT };

struct Row {
    int mode, n, h, w, c0, c1;
    int route, qt, tiles_w, tiles_h, chunks, ntiles;  // qt .. ntiles: 0 off the tiled route
    int S;                                            // filter-gradient slabs
    size_t ws;                                        // unet_dwconv3x3_bwd_filter_workspace(n, h, w, c0 + c1)
    int slabs;                                        // unet_dwconv3x3_bwd_data_bnstats_slabs
};
static void check_row(const Row& r) {
    const DwPlan p = dw_plan(r.mode, r.c0, r.c1, r.n, r.h, r.w);
    const DwFilterPlan f = dw_filter_plan(r.mode, r.c0, r.c1, r.n, r.h, r.w);
    const int C = r.c0 + r.c1;
    const bool ok = p.route == r.route && p.qt == r.qt && p.tiles_w == r.tiles_w && p.tiles_h == r.tiles_h &&
                    p.chunks == r.chunks && p.ntiles == r.ntiles && p.C == C && (p.qt == 0 || p.tw * p.qt == 256) &&
                    f.S == r.S && dw_filter_workspace(r.n, r.h, r.w, C) == r.ws && f.bytes <= r.ws &&
                    dw_bnstats_slabs(r.mode, r.c0, r.n, r.h, r.w) == r.slabs &&
                    (r.route == DW_TILED ? (int)f.grid_x == r.S && (int)f.grid_y == r.chunks : (int)f.grid_y == r.S);
    if (!ok)
        std::printf("mode %d %d x %d x %d, %d+%d: route %d qt %d tiles %d x %d chunks %d ntiles %d S %d grid %u x %u ws %zu "
                    "slabs %d\n", r.mode, r.n, r.h, r.w, r.c0, r.c1, p.route, p.qt, p.tiles_w, p.tiles_h, p.chunks, p.ntiles, f.S,
                    f.grid_x, f.grid_y, dw_filter_workspace(r.n, r.h, r.w, C), dw_bnstats_slabs(r.mode, r.c0, r.n, r.h, r.w));
    CHECK(ok);
}

// The depthwise halves of the 18 conv blocks of the 256 x 256 network at batch 8, 16 and 32: all tiled; the
// persistent filter-gradient blocks are 512 over the channel chunks at batch 8 and 1024 above, capped by the
// tile count.  ntiles = batch x tiles_w x tiles_h, the workspace S slabs of [9][C], BatchNorm slabs = ntiles
// for the BN+ReLU and max-pool views.
struct Net {
    const char* name;
    int mode, c0, c1, hw, qt, tiles_w, tiles_h, chunks, S8, S16, S32;
};
static const Net kNet[] = {
    {"enc1_block1", PLAIN, 4, 0, 256, 1, 1, 32, 1, 256, 512, 1024},
    {"enc1_block2", BNRELU, 64, 0, 256, 16, 16, 32, 1, 512, 1024, 1024},
    {"enc2_block1", POOL, 64, 0, 128, 16, 8, 16, 1, 512, 1024, 1024},
    {"enc2_block2", BNRELU, 128, 0, 128, 16, 8, 16, 2, 256, 512, 512},
    {"enc3_block1", POOL, 128, 0, 64, 16, 4, 8, 2, 256, 512, 512},
    {"enc3_block2", BNRELU, 256, 0, 64, 16, 4, 8, 4, 128, 256, 256},
    {"enc4_block1", POOL, 256, 0, 32, 16, 2, 4, 4, 64, 128, 256},
    {"enc4_block2", BNRELU, 512, 0, 32, 16, 2, 4, 8, 64, 128, 128},
    {"bneck_block1", POOL, 512, 0, 16, 16, 1, 2, 8, 16, 32, 64},
    {"bneck_block2", BNRELU, 1024, 0, 16, 16, 1, 2, 16, 16, 32, 64},
    {"dec4_block1", CONCAT, 512, 512, 32, 16, 2, 4, 16, 32, 64, 64},
    {"dec4_block2", BNRELU, 512, 0, 32, 16, 2, 4, 8, 64, 128, 128},
    {"dec3_block1", CONCAT, 256, 256, 64, 16, 4, 8, 8, 64, 128, 128},
    {"dec3_block2", BNRELU, 256, 0, 64, 16, 4, 8, 4, 128, 256, 256},
    {"dec2_block1", CONCAT, 128, 128, 128, 16, 8, 16, 4, 128, 256, 256},
    {"dec2_block2", BNRELU, 128, 0, 128, 16, 8, 16, 2, 256, 512, 512},
    {"dec1_block1", CONCAT, 64, 64, 256, 16, 16, 32, 2, 256, 512, 512},
    {"dec1_block2", BNRELU, 64, 0, 256, 16, 16, 32, 1, 512, 1024, 1024},
};
// three of them with the queries' values as the library returned them
static const Row kNetQueries[] = {
    {BNRELU, 8, 256, 256, 64, 0, DW_TILED, 16, 16, 32, 1, 4096, 512, 1179648, 4096},
    {POOL, 16, 32, 32, 256, 0, DW_TILED, 16, 2, 4, 4, 128, 128, 1179648, 128},
    {CONCAT, 32, 32, 32, 512, 512, DW_TILED, 16, 2, 4, 16, 256, 64, 2359296, 0},
};

// VIEW_CASES of tests/test_ops_gpu.py as they were before the two views split off the quads joined them
static const Row kViewCases[] = {
    {PLAIN, 2, 9, 7, 3, 0, DW_FLAT_SCALAR, 0, 0, 0, 0, 0, 1, 256, 0},
    {PLAIN, 2, 16, 16, 16, 0, DW_TILED, 4, 1, 2, 1, 4, 4, 2304, 0},
    {BNRELU, 2, 12, 10, 32, 0, DW_TILED, 8, 1, 2, 1, 4, 4, 4608, 4},
    {POOL, 2, 8, 8, 16, 0, DW_TILED, 4, 1, 1, 1, 2, 2, 1280, 2},
    {CONCAT, 2, 8, 6, 16, 16, DW_TILED, 8, 1, 1, 1, 2, 2, 2304, 0},
    {CONCAT, 2, 8, 8, 8, 8, DW_TILED, 4, 1, 1, 1, 2, 2, 1280, 0},
    {BNRELU, 1, 4, 4, 64, 0, DW_TILED, 16, 1, 1, 1, 1, 1, 2304, 1},
    {PLAIN, 1, 1, 1, 8, 0, DW_TILED, 2, 1, 1, 1, 1, 1, 512, 0},
    {BNRELU, 1, 1, 1, 3, 0, DW_FLAT_SCALAR, 0, 0, 0, 0, 0, 1, 256, 0},
    {BNRELU, 1, 1, 127, 16, 0, DW_TILED, 4, 2, 1, 1, 2, 2, 1280, 2},
    {POOL, 1, 1, 127, 8, 0, DW_TILED, 2, 1, 1, 1, 1, 1, 512, 1},
    {CONCAT, 1, 3, 43, 8, 4, DW_FLAT_VEC, 0, 0, 0, 0, 0, 1, 512, 0},
    {PLAIN, 1, 3, 43, 68, 0, DW_FLAT_VEC, 0, 0, 0, 0, 0, 1, 2560, 0},
};
// test_dwconv_bwd_data_bnstats (max-pool and BN+ReLU views)
static const Row kBnstatsCases[] = {
    {POOL, 2, 8, 16, 64, 0, DW_TILED, 16, 1, 1, 1, 2, 2, 4608, 2},
    {POOL, 2, 5, 7, 16, 0, DW_TILED, 4, 1, 1, 1, 2, 2, 1280, 2},
    {POOL, 1, 4, 4, 128, 0, DW_TILED, 16, 1, 1, 2, 1, 1, 4608, 1},
    {POOL, 3, 8, 8, 8, 0, DW_TILED, 2, 1, 1, 1, 3, 3, 1024, 3},
    {POOL, 4, 64, 144, 64, 0, DW_TILED, 16, 9, 8, 1, 288, 288, 663552, 288},
    {POOL, 1, 1, 1, 8, 0, DW_TILED, 2, 1, 1, 1, 1, 1, 512, 1},
    {POOL, 1, 1, 127, 16, 0, DW_TILED, 4, 2, 1, 1, 2, 2, 1280, 2},
    {POOL, 1, 3, 43, 32, 0, DW_TILED, 8, 2, 1, 1, 2, 2, 2304, 2},
    {BNRELU, 2, 8, 16, 64, 0, DW_TILED, 16, 1, 1, 1, 2, 2, 4608, 2},
    {BNRELU, 2, 5, 7, 16, 0, DW_TILED, 4, 1, 1, 1, 2, 2, 1280, 2},
    {BNRELU, 1, 4, 4, 128, 0, DW_TILED, 16, 1, 1, 2, 1, 1, 4608, 1},
    {BNRELU, 3, 8, 8, 8, 0, DW_TILED, 2, 1, 1, 1, 3, 3, 1024, 3},
    {BNRELU, 4, 64, 144, 64, 0, DW_TILED, 16, 9, 8, 1, 288, 288, 663552, 288},
    {BNRELU, 1, 1, 1, 8, 0, DW_TILED, 2, 1, 1, 1, 1, 1, 512, 1},
    {BNRELU, 1, 1, 127, 16, 0, DW_TILED, 4, 2, 1, 1, 2, 2, 1280, 2},
    {BNRELU, 1, 3, 43, 32, 0, DW_TILED, 8, 2, 1, 1, 2, 2, 2304, 2},
};
// tests/test_dwf_gpu.py
static const Row kDwfCases[] = {
    {BNRELU, 2, 16, 16, 128, 0, DW_TILED, 16, 1, 2, 2, 4, 4, 18432, 4},
    {BNRELU, 1, 9, 21, 64, 0, DW_TILED, 16, 2, 2, 1, 4, 4, 9216, 4},
    {BNRELU, 3, 8, 40, 32, 0, DW_TILED, 8, 2, 1, 1, 6, 6, 6912, 6},
    {BNRELU, 2, 5, 7, 8, 0, DW_TILED, 2, 1, 1, 1, 2, 2, 768, 2},
    {BNRELU, 1, 33, 17, 4, 0, DW_TILED, 1, 1, 5, 1, 5, 5, 768, 5},
    {BNRELU, 2, 32, 32, 256, 0, DW_TILED, 16, 2, 4, 4, 16, 16, 147456, 16},
};
// the views of tests/test_dwconv_bits_gpu.py, in its order: every named case reaches the route it claims
static const Row kBitsCases[] = {
    {PLAIN, 2, 9, 7, 3, 0, DW_FLAT_SCALAR, 0, 0, 0, 0, 0, 1, 256, 0},
    {BNRELU, 1, 1, 1, 3, 0, DW_FLAT_SCALAR, 0, 0, 0, 0, 0, 1, 256, 0},
    {POOL, 1, 3, 43, 3, 0, DW_FLAT_SCALAR, 0, 0, 0, 0, 0, 1, 256, 0},
    {CONCAT, 1, 1, 127, 5, 6, DW_FLAT_SCALAR, 0, 0, 0, 0, 0, 1, 512, 0},
    {CONCAT, 1, 3, 43, 6, 2, DW_FLAT_SCALAR, 0, 0, 0, 0, 0, 1, 512, 0},
    {BNRELU, 1, 3, 43, 12, 0, DW_FLAT_VEC, 0, 0, 0, 0, 0, 1, 512, 0},
    {POOL, 2, 9, 7, 12, 0, DW_FLAT_VEC, 0, 0, 0, 0, 0, 1, 512, 0},
    {CONCAT, 1, 1, 127, 8, 4, DW_FLAT_VEC, 0, 0, 0, 0, 0, 1, 512, 0},
    {PLAIN, 1, 3, 43, 68, 0, DW_FLAT_VEC, 0, 0, 0, 0, 0, 1, 2560, 0},
    {CONCAT, 2, 9, 7, 32, 36, DW_FLAT_VEC, 0, 0, 0, 0, 0, 1, 2560, 0},
    {BNRELU, 1, 3, 43, 260, 0, DW_FLAT_VEC, 0, 0, 0, 0, 0, 1, 9472, 0},
    {POOL, 1, 1, 1, 260, 0, DW_FLAT_VEC, 0, 0, 0, 0, 0, 1, 9472, 0},
    {PLAIN, 1, 3, 43, 4, 0, DW_TILED, 1, 1, 1, 1, 1, 1, 256, 0},
    {POOL, 1, 1, 127, 8, 0, DW_TILED, 2, 1, 1, 1, 1, 1, 512, 1},
    {BNRELU, 1, 1, 1, 8, 0, DW_TILED, 2, 1, 1, 1, 1, 1, 512, 1},
    {CONCAT, 2, 9, 7, 8, 8, DW_TILED, 4, 1, 2, 1, 4, 4, 2304, 0},
    {BNRELU, 1, 3, 43, 32, 0, DW_TILED, 8, 2, 1, 1, 2, 2, 2304, 2},
    {POOL, 2, 9, 7, 32, 0, DW_TILED, 8, 1, 2, 1, 4, 4, 4608, 4},
    {BNRELU, 1, 16, 64, 64, 0, DW_TILED, 16, 4, 2, 1, 8, 8, 18432, 8},
    {PLAIN, 1, 16, 48, 64, 0, DW_TILED, 16, 3, 2, 1, 6, 6, 13824, 0},
    {CONCAT, 1, 3, 43, 64, 64, DW_TILED, 16, 3, 1, 2, 3, 3, 13824, 0},
    {POOL, 2, 9, 7, 128, 0, DW_TILED, 16, 1, 2, 2, 4, 4, 18432, 4},
    {BNRELU, 1, 64, 80, 1024, 0, DW_TILED, 16, 5, 8, 16, 40, 32, 1179648, 40},
    {BNRELU, 1, 56, 80, 1024, 0, DW_TILED, 16, 5, 7, 16, 35, 32, 1179648, 35},
    {POOL, 2, 9, 7, 16, 0, DW_TILED, 4, 1, 2, 1, 4, 4, 2304, 4},
    {POOL, 1, 3, 43, 128, 0, DW_TILED, 16, 3, 1, 2, 3, 3, 13824, 3},
    {POOL, 1, 16, 64, 64, 0, DW_TILED, 16, 4, 2, 1, 8, 8, 18432, 8},
    {BNRELU, 2, 9, 7, 32, 0, DW_TILED, 8, 1, 2, 1, 4, 4, 4608, 4},
    {BNRELU, 1, 1, 1, 4, 0, DW_TILED, 1, 1, 1, 1, 1, 1, 256, 1},
    {BNRELU, 1, 3, 43, 128, 0, DW_TILED, 16, 3, 1, 2, 3, 3, 13824, 3},
    {BNRELU, 1, 33, 17, 4, 0, DW_TILED, 1, 1, 5, 1, 5, 5, 768, 5},
    {BNRELU, 2, 5, 7, 8, 0, DW_TILED, 2, 1, 1, 1, 2, 2, 768, 2},
    {BNRELU, 2, 9, 7, 16, 0, DW_TILED, 4, 1, 2, 1, 4, 4, 2304, 4},
    {BNRELU, 1, 16, 48, 128, 0, DW_TILED, 16, 3, 2, 2, 6, 6, 27648, 6},
    {BNRELU, 1, 1, 127, 256, 0, DW_TILED, 16, 8, 1, 4, 8, 8, 73728, 8},
};

// What the entry points did before dw_plan.h, restated: the filter gradient's launch grid and the workspace
// query both followed C % 4, the flat kernel's lanes followed the view (view_vec).
struct Before {
    int ctiles, S, CQ_dev, CT_dev;
    size_t ws;
};
static Before before(int mode, int c0, int c1, int n, int h, int w) {
    const int C = view_channels(mode, c0, c1);
    const int CQ = C % 4 == 0 ? C / 4 : C, CT = CQ < 64 ? CQ : 64;
    Before b;
    b.ctiles = (CQ + CT - 1) / CT;
    const long long P = (long long)n * h * w, want = (2048 + b.ctiles - 1) / b.ctiles, maxc = (P + 255) / 256;
    long long chunks = want < maxc ? want : maxc;
    if (chunks < 1) chunks = 1;
    const long long ppc = (P + chunks - 1) / chunks;
    b.S = (int)((P + ppc - 1) / ppc);
    b.CQ_dev = view_vec(mode, c0, c1) ? C / 4 : C;
    b.CT_dev = b.CQ_dev < 64 ? b.CQ_dev : 64;
    b.ws = dw_filter_workspace(n, h, w, C);  // (unchanged for every C: pinned by the rows above)
    return b;
}

int main() {
    for (const Net& b : kNet)
        for (int batch : {8, 16, 32}) {
            const int C = b.c0 + b.c1, nt = batch * b.tiles_w * b.tiles_h, S = batch == 8 ? b.S8 : batch == 16 ? b.S16 : b.S32;
            check_row({b.mode, batch, b.hw, b.hw, b.c0, b.c1, DW_TILED, b.qt, b.tiles_w, b.tiles_h, b.chunks, nt, S,
                       align_up((size_t)S * 9 * C * 4, 256), b.mode == BNRELU || b.mode == POOL ? nt : 0});
        }
    for (const Row& r : kNetQueries) check_row(r);
    for (const Row& r : kViewCases) check_row(r);
    for (const Row& r : kBnstatsCases) check_row(r);
    for (const Row& r : kDwfCases) check_row(r);
    for (const Row& r : kBitsCases) check_row(r);
    // flat vector lanes off the tiled widths: 17 quads in one channel tile, 65 quads in two
    CHECK(dw_filter_plan(PLAIN, 68, 0, 1, 3, 43).grid_x == 1 && dw_filter_plan(PLAIN, 68, 0, 1, 3, 43).CT == 17);
    CHECK(dw_filter_plan(BNRELU, 260, 0, 1, 3, 43).grid_x == 2 && dw_filter_plan(BNRELU, 260, 0, 1, 3, 43).CT == 64);
    // more than one pixel chunk on the flat routes: 2 x 64 x 64 pixels in chunks of 256
    CHECK(dw_filter_plan(PLAIN, 3, 0, 2, 64, 64).S == 32 && dw_filter_plan(PLAIN, 3, 0, 2, 64, 64).ppc == 256);
    CHECK(dw_filter_plan(PLAIN, 520, 0, 16, 256, 256).S == 683 && dw_filter_plan(PLAIN, 520, 0, 16, 256, 256).grid_x == 3);

    // The two defects, as rows.  (1, 8, 128, 6 + 2): the query sized one tiled slab for C = 8, the launch was
    // the scalar flat kernel over 4 pixel chunks; (1, 8, 512, 6 + 2) likewise, 16 chunks.  (1, 3, 43, 34 + 34)
    // and (., 130 + 126): the grid had one channel tile per 64 QUADS, the scalar kernel covers 64 CHANNELS per tile.
    {
        const Before a = before(CONCAT, 6, 2, 1, 8, 128), b = before(CONCAT, 6, 2, 1, 8, 512);
        CHECK(a.ws == 512 && a.S == 4 && (size_t)a.S * 9 * 8 * 4 == 1152 && (size_t)a.S * 9 * 8 * 4 > a.ws);
        CHECK(b.ws == 1280 && b.S == 16 && (size_t)b.S * 9 * 8 * 4 == 4608 && (size_t)b.S * 9 * 8 * 4 > b.ws);
        const Before c = before(CONCAT, 34, 34, 1, 3, 43), d = before(CONCAT, 130, 126, 1, 3, 43);
        CHECK(c.ctiles == 1 && c.CQ_dev == 68 && c.CT_dev == 64 && c.ctiles * c.CT_dev < c.CQ_dev);
        CHECK(d.ctiles == 1 && d.CQ_dev == 256 && d.ctiles * d.CT_dev == 64);
        const int kFixed[][5] = {{6, 2, 1, 8, 128}, {6, 2, 1, 8, 512}, {34, 34, 1, 3, 43}, {130, 126, 1, 3, 43}};
        for (const auto& s : kFixed) {
            const DwFilterPlan f = dw_filter_plan(CONCAT, s[0], s[1], s[2], s[3], s[4]);
            CHECK(f.p.route == DW_FLAT_SCALAR && (int)f.grid_x * f.CT >= f.p.CQ && f.p.CQ == s[0] + s[1]);
            CHECK((size_t)f.S * 9 * f.p.C * 4 <= dw_filter_workspace(s[2], s[3], s[4], f.p.C));
        }
        CHECK(dw_filter_plan(CONCAT, 6, 2, 1, 8, 128).S == 1 && dw_filter_plan(CONCAT, 6, 2, 1, 8, 512).S == 4);
        CHECK(dw_filter_plan(CONCAT, 34, 34, 1, 3, 43).grid_x == 2 && dw_filter_plan(CONCAT, 130, 126, 1, 3, 43).grid_x == 4);
    }

    // sweep: every view check_view accepts, for the plan's invariants
    const int kCh[] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 16, 32, 34, 64, 68, 126, 128, 130, 256};
    const int kNHW[][3] = {{1, 1, 1}, {1, 1, 127}, {1, 3, 43}, {2, 9, 7}, {1, 8, 128}, {1, 8, 512}, {2, 64, 64}, {3, 17, 300},
                           {8, 128, 128}, {16, 256, 256}};
    long long plans = 0, unaligned = 0, overran = 0, uncovered = 0;
    for (int mode = PLAIN; mode <= CONCAT; ++mode)
        for (int c0 : kCh)
            for (int c1 : kCh) {
                if (mode != CONCAT && c1 != kCh[0]) continue;  // c1 is read for concat views only
                for (const auto& d : kNHW) {
                    const int n = d[0], h = d[1], w = d[2], C = view_channels(mode, c0, c1);
                    if (!index_fits(mode, c0, c1, n, h, w)) continue;
                    const DwPlan p = dw_plan(mode, c0, c1, n, h, w);
                    const DwFilterPlan f = dw_filter_plan(mode, c0, c1, n, h, w);
                    const bool vec = c0 % 4 == 0 && (mode != CONCAT || c1 % 4 == 0);
                    const bool tiled = vec && (C % 64 == 0 || C == 4 || C == 8 || C == 16 || C == 32);
                    ++plans;
                    CHECK(p.route == (tiled ? DW_TILED : vec ? DW_FLAT_VEC : DW_FLAT_SCALAR) && p.vec() == vec && p.C == C);
                    CHECK(p.CQ == (vec ? C / 4 : C) && p.flat_grid >= 1 && p.flat_grid <= 65536);
                    CHECK(p.flat_grid == 65536 || (long long)p.flat_grid * 256 >= (long long)n * h * w * p.CQ);
                    CHECK(f.p.route == p.route && f.S >= 1 && f.bytes == align_up((size_t)f.S * 9 * C * 4, 256));
                    // the slabs fit what the view-less query returns for C
                    CHECK((size_t)f.S * 9 * C * 4 <= dw_filter_workspace(n, h, w, C));
                    if (tiled) {
                        CHECK(p.qt * p.tw == 256 && p.chunks * 4 * p.qt == C && p.tiles_w * p.tw >= w && (p.tiles_w - 1) * p.tw < w);
                        CHECK(p.tiles_h * TH >= h && (p.tiles_h - 1) * TH < h && p.ntiles == n * p.tiles_w * p.tiles_h);
                        CHECK((int)f.grid_x == f.S && (int)f.grid_y == p.chunks && f.S <= p.ntiles);
                        CHECK(f.S == p.ntiles || f.S * p.chunks >= (n <= 8 ? 512 : 1024));
                    } else {
                        // the grid covers every lane of a pixel, for the lane width the route launches
                        CHECK(f.CT == (p.CQ < 64 ? p.CQ : 64) && f.PL == 256 / f.CT && f.PL >= 1);
                        CHECK((long long)f.grid_x * f.CT >= p.CQ && (long long)(f.grid_x - 1) * f.CT < p.CQ);
                        CHECK((int)f.grid_y == f.S && f.ppc * f.S >= (long long)n * h * w && f.ppc * (f.S - 1) < (long long)n * h * w);
                    }
                    const bool off_quads = mode == CONCAT && c0 % 4 != 0 && C % 4 == 0;
                    const Before b = before(mode, c0, c1, n, h, w);
                    if (!off_quads) {  // every other view: the plan is what it was
                        if (!tiled) CHECK((int)f.grid_x == b.ctiles && f.S == b.S && p.CQ == b.CQ_dev && f.CT == b.CT_dev);
                        CHECK(f.bytes == b.ws);
                    } else {
                        ++unaligned;
                        overran += (size_t)b.S * 9 * C * 4 > b.ws;
                        uncovered += b.ctiles * b.CT_dev < b.CQ_dev;
                    }
                    // BatchNorm partials exactly where unet_dwconv3x3_bwd_data_bnstats admits the view
                    const int slabs = dw_bnstats_slabs(mode, c0, n, h, w);
                    CHECK((slabs > 0) == ((mode == BNRELU || mode == POOL) && tiled) && (slabs == 0 || slabs == p.ntiles));
                    CHECK(dw_bnstats_dwf_ok(mode, c0, 0.f, n, h, w) == (mode == BNRELU && tiled));
                    CHECK(!dw_bnstats_dwf_ok(mode, c0, 0.2f, n, h, w));
                }
            }
    CHECK(plans > 4000 && unaligned > 100 && overran > 10 && uncovered > 10);
    // no plan for no problem; the 2^31 index bound (the 2 x 2 source of a max-pool view)
    CHECK(dw_filter_workspace(0, 8, 8, 8) == 0 && dw_filter_workspace(1, 8, 8, 0) == 0 && dw_bnstats_slabs(BNRELU, 8, 1, 0, 8) == 0);
    CHECK(dw_bnstats_slabs(CONCAT, 8, 1, 8, 8) == 0 && dw_bnstats_slabs(PLAIN, 8, 1, 8, 8) == 0 && dw_bnstats_slabs(BNRELU, 12, 1, 8, 8) == 0);
    CHECK(index_fits(BNRELU, 64, 0, 127, 512, 512) && !index_fits(BNRELU, 64, 0, 128, 512, 512));
    CHECK(index_fits(POOL, 64, 0, 31, 512, 512) && !index_fits(POOL, 64, 0, 32, 512, 512));
    CHECK(index_fits(CONCAT, 32, 32, 127, 512, 512) && !index_fits(CONCAT, 32, 32, 128, 512, 512));
    if (g_failed) return 1;
    std::printf("dw_plan_check OK\n");
    return 0;
}
