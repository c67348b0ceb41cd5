// Stand-alone host check of the BatchNorm family's policy (csrc/bn_plan.h: fwd_partials, red_plan, bwd_workspace,
// stats_finish, colsum_plan), compiled and run by test_bn_plan_host.py; host pass only, no GPU.  The pinned rows
// are what bn.hip and lastblock.h computed before the plan header existed: that arithmetic was compiled on its own
// once and its values are the literals below; the three byte counts were also read from that library's size queries
// (test_bn_plan_host.py asks this library's queries for a dozen of them again).
// Exit status 0 = every check passed; otherwise the failing lines are printed.
#include <cstdio>

#include "bn_plan.h"

using namespace unet;
using namespace unet::bn;

static int g_failed = 0;
#define CHECK(cond)                                               \
    do {                                                          \
        if (!(cond)) {                                            \
            std::printf("FAILED line %d: %s\n", __LINE__, #cond); \
            ++g_failed;                                           \
        }                                                         \
    } while (0)

// ------------------------------------------------------------------ forward partials (unet_bn_partials_size) ---
struct Fwd {
    int64_t m;
    int c;
    int64_t nblk;
    int nch;
    size_t chunks_off, counter_off, bytes;
    unsigned grid_x;  // the finalize runs grid (grid_x, nch)
};
static void check_fwd(const Fwd& r) {
    const FwdPartials f = fwd_partials(r.m, r.c);
    const bool ok = f.nblk == r.nblk && f.nch == r.nch && f.chunks_off == r.chunks_off &&
                    f.counter_off == r.counter_off && f.bytes == r.bytes && f.grid_x == r.grid_x;
    if (!ok)
        std::printf("fwd m %lld c %d: nblk %lld nch %d offsets %zu %zu bytes %zu grid_x %u\n", (long long)r.m, r.c,
                    (long long)f.nblk, f.nch, f.chunks_off, f.counter_off, f.bytes, f.grid_x);
    CHECK(ok);
}
// the default net's five levels (m = batch x H x W, c = the width of the level's encoder and decoder blocks: 18
// blocks, the bottleneck's two included) at batch 8, 16 and 32
static const Fwd kFwdNet[] = {
    {524288, 64, 4096, 64, 2097152, 2162688, 2162692, 1},
    {131072, 128, 1024, 16, 1048576, 1081344, 1081352, 2},
    {32768, 256, 256, 4, 524288, 540672, 540688, 4},
    {8192, 512, 64, 1, 262144, 270336, 270368, 8},
    {2048, 1024, 16, 1, 131072, 147456, 147520, 16},
    {1048576, 64, 8192, 128, 4194304, 4325376, 4325380, 1},
    {262144, 128, 2048, 32, 2097152, 2162688, 2162696, 2},
    {65536, 256, 512, 8, 1048576, 1081344, 1081360, 4},
    {16384, 512, 128, 2, 524288, 540672, 540704, 8},
    {4096, 1024, 32, 1, 262144, 278528, 278592, 16},
    {2097152, 64, 16384, 256, 8388608, 8650752, 8650756, 1},
    {524288, 128, 4096, 64, 4194304, 4325376, 4325384, 2},
    {131072, 256, 1024, 16, 2097152, 2162688, 2162704, 4},
    {32768, 512, 256, 4, 1048576, 1081344, 1081376, 8},
    {8192, 1024, 64, 1, 524288, 540672, 540736, 16},
};
// test_ops_gpu.py (test_pointwise_and_bn_stats, test_bn_sync_moments, the fused separable-conv cases),
// test_fenced_ops_gpu.py and test_degenerate_ops_gpu.py
static const Fwd kFwdTests[] = {
    {100, 64, 1, 1, 512, 1536, 1540, 1},
    {256, 64, 2, 1, 1024, 2048, 2052, 1},
    {300, 128, 3, 1, 3072, 5120, 5128, 2},
    {128, 256, 1, 1, 2048, 6144, 6160, 4},
    {77, 96, 1, 1, 768, 2304, 2312, 2},
    {512, 512, 4, 1, 16384, 24576, 24608, 8},
    {24653, 64, 193, 4, 98816, 102912, 102916, 1},
    {24653, 128, 193, 4, 197632, 205824, 205832, 2},
    {1, 4, 1, 1, 256, 512, 516, 1},
    {1, 48, 1, 1, 512, 1280, 1284, 1},
    {1, 68, 1, 1, 768, 2048, 2056, 2},
    {127, 4, 1, 1, 256, 512, 516, 1},
    {127, 48, 1, 1, 512, 1280, 1284, 1},
    {127, 68, 1, 1, 768, 2048, 2056, 2},
    {129, 4, 2, 1, 256, 512, 516, 1},
    {129, 48, 2, 1, 768, 1536, 1540, 1},
    {129, 68, 2, 1, 1280, 2560, 2568, 2},
    {3000, 64, 24, 1, 12288, 13312, 13316, 1},
    {2000, 64, 16, 1, 8192, 9216, 9220, 1},
    {5000, 64, 40, 1, 20480, 21504, 21508, 1},
    {9000, 128, 71, 2, 72704, 76800, 76808, 2},
    {33653, 128, 263, 5, 269312, 279552, 279560, 2},
    {128, 96, 1, 1, 768, 2304, 2312, 2},
    {129, 96, 2, 1, 1536, 3072, 3080, 2},
    {1000, 96, 8, 1, 6144, 7680, 7688, 2},
    {1257, 96, 10, 1, 7680, 9216, 9224, 2},
    {5000, 256, 40, 1, 81920, 86016, 86032, 4},
    {1024, 64, 8, 1, 4096, 5120, 5124, 1},
    {256, 128, 2, 1, 2048, 4096, 4104, 2},
    {256, 96, 2, 1, 1536, 3072, 3080, 2},
    {512, 64, 4, 1, 2048, 3072, 3076, 1},
    {256, 256, 2, 1, 4096, 8192, 8208, 4},
    {128, 8, 1, 1, 256, 512, 516, 1},
    {512, 192, 4, 1, 6144, 9216, 9228, 3},
    {128, 100, 1, 1, 1024, 2816, 2824, 2},
    {512, 256, 4, 1, 8192, 12288, 12304, 4},
    {65536, 192, 512, 8, 786432, 811008, 811020, 3},
    {128, 64, 1, 1, 512, 1536, 1540, 1},
    {384, 64, 3, 1, 1536, 2560, 2564, 1},
    {384, 128, 3, 1, 3072, 5120, 5128, 2},
    {300, 64, 3, 1, 1536, 2560, 2564, 1},
    {8229, 128, 65, 2, 66560, 70656, 70664, 2},
    {8229, 64, 65, 2, 33280, 35328, 35332, 1},
    {8229, 32, 65, 2, 16640, 17664, 17668, 1},
    {512, 128, 4, 1, 4096, 6144, 6152, 2},
    {1024, 128, 8, 1, 8192, 10240, 10248, 2},
};
// test_bn_bits_gpu.py (unet_bn_finalize, unet_bn_moments)
static const Fwd kFwdBits[] = {
    {1, 3, 1, 1, 256, 512, 516, 1},
    {1, 64, 1, 1, 512, 1536, 1540, 1},
    {1, 68, 1, 1, 768, 2048, 2056, 2},
    {129, 3, 2, 1, 256, 512, 516, 1},
    {129, 64, 2, 1, 1024, 2048, 2052, 1},
    {129, 68, 2, 1, 1280, 2560, 2568, 2},
    {8192, 3, 64, 1, 1536, 1792, 1796, 1},
    {8192, 64, 64, 1, 32768, 33792, 33796, 1},
    {8192, 68, 64, 1, 34816, 36096, 36104, 2},
    {8193, 3, 65, 2, 1792, 2048, 2052, 1},
    {8193, 64, 65, 2, 33280, 35328, 35332, 1},
    {8193, 68, 65, 2, 35584, 37888, 37896, 2},
    {40997, 3, 321, 6, 7936, 8448, 8452, 1},
    {40997, 64, 321, 6, 164352, 170496, 170500, 1},
    {40997, 68, 321, 6, 174848, 181504, 181512, 2},
    {524293, 3, 4097, 65, 98560, 101888, 101892, 1},
    {524293, 64, 4097, 65, 2097664, 2164224, 2164228, 1},
    {524293, 68, 4097, 65, 2228992, 2299904, 2299912, 2},
};

// --------------------------------------------------------- backward workspace (unet_bn_relu_bwd_workspace) ---
struct Bwd {
    int64_t m;
    int c;
    int ctiles, CT;
    int64_t chunks, rpc;
    size_t sums_off, scratch_off, counter_off, bytes;
    int stats_route, ncnt;  // unet_bn_relu_bwd_stats; unet_bn_relu_bwd is BWD_DZ without counters
    int apply_grid;
    unsigned fin_gx;  // grid of the finish launch on the BWD_STATS_FINISH route (0 x 0 otherwise)
    int fin_nch;
};
static void check_bwd(const Bwd& r) {
    const BwdWorkspace s = bwd_workspace(r.m, r.c, true), d = bwd_workspace(r.m, r.c);
    const StatsFinish f = stats_finish((int)s.red.chunks, r.c);
    const bool fin = r.stats_route == BWD_STATS_FINISH;
    const bool ok = s.red.ctiles == r.ctiles && s.red.CT == r.CT && s.red.chunks == r.chunks && s.red.rpc == r.rpc &&
                    s.sums_off == r.sums_off && s.scratch_off == r.scratch_off && s.counter_off == r.counter_off &&
                    s.bytes == r.bytes && s.route == r.stats_route && s.ncnt == r.ncnt && s.apply_grid == r.apply_grid &&
                    s.vec == (r.c % 4 == 0) && (!fin || (f.grid_x == r.fin_gx && f.nch == r.fin_nch)) &&
                    // the dz entry: the same geometry and layout, its own route
                    d.route == BWD_DZ && d.ncnt == 0 && d.red.chunks == r.chunks && d.red.rpc == r.rpc &&
                    d.red.CT == r.CT && d.red.ctiles == r.ctiles && d.sums_off == r.sums_off && d.bytes == r.bytes &&
                    d.apply_grid == r.apply_grid && d.vec == s.vec;
    if (!ok)
        std::printf("bwd m %lld c %d: ctiles %d CT %d chunks %lld rpc %lld offsets %zu %zu %zu bytes %zu route %d ncnt %d "
                    "apply grid %d finish %u x %d\n", (long long)r.m, r.c, s.red.ctiles, s.red.CT, (long long)s.red.chunks,
                    (long long)s.red.rpc, s.sums_off, s.scratch_off, s.counter_off, s.bytes, s.route, s.ncnt, s.apply_grid,
                    f.grid_x, f.nch);
    CHECK(ok);
}
static const Bwd kBwdNet[] = {
    {524288, 64, 1, 16, 1024, 512, 524288, 524800, 541184, 541440, BWD_STATS_FINISH, 1, 32768, 1, 16},
    {131072, 128, 1, 32, 1024, 128, 1048576, 1049600, 1082368, 1082624, BWD_STATS_FINISH, 2, 16384, 2, 16},
    {32768, 256, 1, 64, 256, 128, 524288, 526336, 542720, 542976, BWD_STATS_FINISH, 4, 8192, 4, 4},
    {8192, 512, 2, 64, 64, 128, 262144, 266240, 274432, 274688, BWD_STATS_FINISH, 8, 4096, 8, 1},
    {2048, 1024, 4, 64, 16, 128, 131072, 139264, 155648, 155904, BWD_STATS_FINISH, 16, 2048, 16, 1},
    {1048576, 64, 1, 16, 1024, 1024, 524288, 524800, 541184, 541440, BWD_STATS_FINISH, 1, 65536, 1, 16},
    {262144, 128, 1, 32, 1024, 256, 1048576, 1049600, 1082368, 1082624, BWD_STATS_FINISH, 2, 32768, 2, 16},
    {65536, 256, 1, 64, 512, 128, 1048576, 1050624, 1083392, 1083648, BWD_STATS_FINISH, 4, 16384, 4, 8},
    {16384, 512, 2, 64, 128, 128, 524288, 528384, 544768, 545024, BWD_STATS_FINISH, 8, 8192, 8, 2},
    {4096, 1024, 4, 64, 32, 128, 262144, 270336, 286720, 286976, BWD_STATS_FINISH, 16, 4096, 16, 1},
    {2097152, 64, 1, 16, 1024, 2048, 524288, 524800, 541184, 541440, BWD_STATS_FINISH, 1, 65536, 1, 16},
    {524288, 128, 1, 32, 1024, 512, 1048576, 1049600, 1082368, 1082624, BWD_STATS_FINISH, 2, 65536, 2, 16},
    {131072, 256, 1, 64, 1024, 128, 2097152, 2099200, 2164736, 2164992, BWD_STATS_FINISH, 4, 32768, 4, 16},
    {32768, 512, 2, 64, 256, 128, 1048576, 1052672, 1085440, 1085696, BWD_STATS_FINISH, 8, 16384, 8, 4},
    {8192, 1024, 4, 64, 64, 128, 524288, 532480, 548864, 549120, BWD_STATS_FINISH, 16, 8192, 16, 1},
};
// test_ops_gpu.py (test_bn_relu_bwd, the data gradients that form dz on load, the three producers' statistics
// tests, test_sepconv_bwd_fused), test_fenced_ops_gpu.py and test_degenerate_ops_gpu.py
static const Bwd kBwdTests[] = {
    {300, 16, 1, 4, 3, 100, 512, 768, 1024, 1280, BWD_STATS_FINISH, 1, 5, 1, 1},
    {1000, 64, 1, 16, 8, 125, 4096, 4608, 5632, 5888, BWD_STATS_FINISH, 1, 63, 1, 1},
    {96, 3, 1, 3, 1, 96, 256, 512, 768, 1024, BWD_STATS_SLABS, 0, 2, 0, 0},
    {1, 4, 1, 1, 1, 1, 256, 512, 768, 1024, BWD_STATS_FINISH, 1, 1, 1, 1},
    {1, 48, 1, 12, 1, 1, 512, 1024, 1792, 2048, BWD_STATS_FINISH, 1, 1, 1, 1},
    {1, 68, 1, 17, 1, 1, 768, 1536, 2816, 3072, BWD_STATS_FINISH, 2, 1, 2, 1},
    {127, 4, 1, 1, 1, 127, 256, 512, 768, 1024, BWD_STATS_FINISH, 1, 1, 1, 1},
    {127, 48, 1, 12, 1, 127, 512, 1024, 1792, 2048, BWD_STATS_FINISH, 1, 6, 1, 1},
    {127, 68, 1, 17, 1, 127, 768, 1536, 2816, 3072, BWD_STATS_FINISH, 2, 9, 2, 1},
    {129, 4, 1, 1, 2, 65, 256, 512, 768, 1024, BWD_STATS_FINISH, 1, 1, 1, 1},
    {129, 48, 1, 12, 2, 65, 768, 1280, 2048, 2304, BWD_STATS_FINISH, 1, 7, 1, 1},
    {129, 68, 1, 17, 2, 65, 1280, 2048, 3328, 3584, BWD_STATS_FINISH, 2, 9, 2, 1},
    {300, 64, 1, 16, 3, 100, 1536, 2048, 3072, 3328, BWD_STATS_FINISH, 1, 19, 1, 1},
    {37, 32, 1, 8, 1, 37, 256, 512, 1024, 1280, BWD_STATS_FINISH, 1, 2, 1, 1},
    {1000, 32, 1, 8, 8, 125, 2048, 2304, 2816, 3072, BWD_STATS_FINISH, 1, 32, 1, 1},
    {40000, 64, 1, 16, 313, 128, 160256, 160768, 165888, 166144, BWD_STATS_FINISH, 1, 2500, 1, 5},
    {300000, 64, 1, 16, 1024, 293, 524288, 524800, 541184, 541440, BWD_STATS_FINISH, 1, 18750, 1, 16},
    {300, 32, 1, 8, 3, 100, 768, 1024, 1536, 1792, BWD_STATS_FINISH, 1, 10, 1, 1},
    {1000, 128, 1, 32, 8, 125, 8192, 9216, 11264, 11520, BWD_STATS_FINISH, 2, 125, 2, 1},
    {257, 64, 1, 16, 3, 86, 1536, 2048, 3072, 3328, BWD_STATS_FINISH, 1, 17, 1, 1},
    {128, 8, 1, 2, 1, 128, 256, 512, 768, 1024, BWD_STATS_FINISH, 1, 1, 1, 1},
    {520, 64, 1, 16, 5, 104, 2560, 3072, 4096, 4352, BWD_STATS_FINISH, 1, 33, 1, 1},
    {128, 128, 1, 32, 1, 128, 1024, 2048, 4096, 4352, BWD_STATS_FINISH, 2, 16, 2, 1},
    {35, 64, 1, 16, 1, 35, 512, 1024, 2048, 2304, BWD_STATS_FINISH, 1, 3, 1, 1},
    {72, 256, 1, 64, 1, 72, 2048, 4096, 8192, 8448, BWD_STATS_FINISH, 4, 18, 4, 1},
    {512, 128, 1, 32, 4, 128, 4096, 5120, 7168, 7424, BWD_STATS_FINISH, 2, 64, 2, 1},
    {36864, 128, 1, 32, 288, 128, 294912, 295936, 306176, 306432, BWD_STATS_FINISH, 2, 4608, 2, 5},
    {1, 64, 1, 16, 1, 1, 512, 1024, 2048, 2304, BWD_STATS_FINISH, 1, 1, 1, 1},
    {127, 64, 1, 16, 1, 127, 512, 1024, 2048, 2304, BWD_STATS_FINISH, 1, 8, 1, 1},
    {256, 64, 1, 16, 2, 128, 1024, 1536, 2560, 2816, BWD_STATS_FINISH, 1, 16, 1, 1},
    {70, 16, 1, 4, 1, 70, 256, 512, 768, 1024, BWD_STATS_FINISH, 1, 2, 1, 1},
    {16, 128, 1, 32, 1, 16, 1024, 2048, 4096, 4352, BWD_STATS_FINISH, 2, 2, 2, 1},
    {192, 8, 1, 2, 2, 96, 256, 512, 768, 1024, BWD_STATS_FINISH, 1, 2, 1, 1},
    {36864, 64, 1, 16, 288, 128, 147456, 147968, 153088, 153344, BWD_STATS_FINISH, 1, 2304, 1, 5},
    {1, 8, 1, 2, 1, 1, 256, 512, 768, 1024, BWD_STATS_FINISH, 1, 1, 1, 1},
    {127, 16, 1, 4, 1, 127, 256, 512, 768, 1024, BWD_STATS_FINISH, 1, 2, 1, 1},
    {129, 32, 1, 8, 2, 65, 512, 768, 1280, 1536, BWD_STATS_FINISH, 1, 5, 1, 1},
    {306, 64, 1, 16, 3, 102, 1536, 2048, 3072, 3328, BWD_STATS_FINISH, 1, 20, 1, 1},
    {135, 16, 1, 4, 2, 68, 256, 512, 768, 1024, BWD_STATS_FINISH, 1, 3, 1, 1},
    {768, 64, 1, 16, 6, 128, 3072, 3584, 4608, 4864, BWD_STATS_FINISH, 1, 48, 1, 1},
    {1517, 64, 1, 16, 12, 127, 6144, 6656, 7680, 7936, BWD_STATS_FINISH, 1, 95, 1, 1},
    {512, 64, 1, 16, 4, 128, 2048, 2560, 3584, 3840, BWD_STATS_FINISH, 1, 32, 1, 1},
    {128, 64, 1, 16, 1, 128, 512, 1024, 2048, 2304, BWD_STATS_FINISH, 1, 8, 1, 1},
    {384, 64, 1, 16, 3, 128, 1536, 2048, 3072, 3328, BWD_STATS_FINISH, 1, 24, 1, 1},
};
// test_bn_bits_gpu.py (unet_bn_relu_bwd, unet_bn_relu_bwd_stats)
static const Bwd kBwdBits[] = {
    {1, 4, 1, 1, 1, 1, 256, 512, 768, 1024, BWD_STATS_FINISH, 1, 1, 1, 1},
    {300, 3, 1, 3, 3, 100, 256, 512, 768, 1024, BWD_STATS_SLABS, 0, 4, 0, 0},
    {300, 6, 1, 6, 3, 100, 256, 512, 768, 1024, BWD_STATS_SLABS, 0, 8, 0, 0},
    {300, 68, 1, 17, 3, 100, 1792, 2560, 3840, 4096, BWD_STATS_FINISH, 2, 20, 2, 1},
    {300, 260, 2, 64, 3, 100, 6400, 8704, 13056, 13312, BWD_STATS_FINISH, 5, 77, 5, 1},
    {8320, 4, 1, 1, 65, 128, 2304, 2560, 2816, 3072, BWD_STATS_FINISH, 1, 33, 1, 2},
    {8320, 6, 1, 6, 65, 128, 3328, 3584, 3840, 4096, BWD_STATS_SLABS, 0, 195, 0, 0},
};

// --------------------------------------------- producer-side statistics slabs (unet_bn_stats_partials_size) ---
struct Fin {
    int S, c;
    unsigned grid_x;
    int nch;
    size_t scratch_off, counter_off, bytes;
};
static void check_fin(const Fin& r) {
    const StatsFinish f = stats_finish(r.S, r.c);
    const bool ok = f.grid_x == r.grid_x && f.nch == r.nch && f.scratch_off == r.scratch_off &&
                    f.counter_off == r.counter_off && f.bytes == r.bytes;
    if (!ok)
        std::printf("finish S %d c %d: grid %u x %d offsets %zu %zu bytes %zu\n", r.S, r.c, f.grid_x, f.nch,
                    f.scratch_off, f.counter_off, f.bytes);
    CHECK(ok);
}
// the default net's depthwise producers: one slab per tile (tiles per image x batch 8, 16, 32) of the view's channels
static const Fin kFinNet[] = {
    {4096, 64, 1, 64, 2097152, 2162688, 2162692},
    {1024, 64, 1, 16, 524288, 540672, 540676},
    {1024, 128, 2, 16, 1048576, 1081344, 1081352},
    {256, 128, 2, 4, 262144, 270336, 270344},
    {256, 256, 4, 4, 524288, 540672, 540688},
    {64, 256, 4, 1, 131072, 135168, 135184},
    {64, 512, 8, 1, 262144, 270336, 270368},
    {16, 512, 8, 1, 65536, 73728, 73760},
    {16, 1024, 16, 1, 131072, 147456, 147520},
    {8192, 64, 1, 128, 4194304, 4325376, 4325380},
    {2048, 64, 1, 32, 1048576, 1081344, 1081348},
    {2048, 128, 2, 32, 2097152, 2162688, 2162696},
    {512, 128, 2, 8, 524288, 540672, 540680},
    {512, 256, 4, 8, 1048576, 1081344, 1081360},
    {128, 256, 4, 2, 262144, 270336, 270352},
    {128, 512, 8, 2, 524288, 540672, 540704},
    {32, 512, 8, 1, 131072, 139264, 139296},
    {32, 1024, 16, 1, 262144, 278528, 278592},
    {16384, 64, 1, 256, 8388608, 8650752, 8650756},
    {4096, 128, 2, 64, 4194304, 4325376, 4325384},
    {1024, 256, 4, 16, 2097152, 2162688, 2162704},
    {256, 512, 8, 4, 1048576, 1081344, 1081376},
    {64, 1024, 16, 1, 524288, 540672, 540736},
};
// test_fenced_ops_gpu.py's host-made slabs and the slab counts of the ConvT, depthwise and head producers in
// test_ops_gpu.py and test_degenerate_ops_gpu.py
static const Fin kFinTests[] = {
    {1, 4, 1, 1, 256, 512, 516},
    {1, 48, 1, 1, 512, 1280, 1284},
    {1, 68, 2, 1, 768, 2048, 2056},
    {2, 4, 1, 1, 256, 512, 516},
    {2, 48, 1, 1, 768, 1536, 1540},
    {2, 68, 2, 1, 1280, 2560, 2568},
    {65, 4, 1, 2, 2304, 2560, 2564},
    {65, 48, 1, 2, 25088, 26624, 26628},
    {65, 68, 2, 2, 35584, 37888, 37896},
    {2, 128, 2, 1, 2048, 4096, 4104},
    {1, 64, 1, 1, 512, 1536, 1540},
    {2, 256, 4, 1, 4096, 8192, 8208},
    {8, 128, 2, 1, 8192, 10240, 10248},
    {288, 128, 2, 5, 294912, 305152, 305160},
    {2, 64, 1, 1, 1024, 2048, 2052},
    {3, 68, 2, 1, 1792, 3072, 3080},
    {2, 16, 1, 1, 256, 512, 516},
    {1, 128, 2, 1, 1024, 3072, 3080},
    {3, 8, 1, 1, 256, 512, 516},
    {288, 64, 1, 5, 147456, 152576, 152580},
    {1, 8, 1, 1, 256, 512, 516},
    {2, 32, 1, 1, 512, 1024, 1028},
    {8, 64, 1, 1, 4096, 5120, 5124},
    {6, 16, 1, 1, 768, 1024, 1028},
    {3, 64, 1, 1, 1536, 2560, 2564},
    {6, 64, 1, 1, 3072, 4096, 4100},
};
// test_bn_bits_gpu.py (unet_bn_relu_bwd_stats_finish)
static const Fin kFinBits[] = {
    {1, 4, 1, 1, 256, 512, 516},
    {1, 64, 1, 1, 512, 1536, 1540},
    {1, 68, 2, 1, 768, 2048, 2056},
    {63, 4, 1, 1, 2048, 2304, 2308},
    {63, 64, 1, 1, 32256, 33280, 33284},
    {63, 68, 2, 1, 34304, 35584, 35592},
    {64, 4, 1, 1, 2048, 2304, 2308},
    {64, 64, 1, 1, 32768, 33792, 33796},
    {64, 68, 2, 1, 34816, 36096, 36104},
    {65, 4, 1, 2, 2304, 2560, 2564},
    {65, 64, 1, 2, 33280, 35328, 35332},
    {65, 68, 2, 2, 35584, 37888, 37896},
    {2049, 4, 1, 33, 65792, 68096, 68100},
    {2049, 64, 1, 33, 1049088, 1082880, 1082884},
    {2049, 68, 2, 33, 1114880, 1150976, 1150984},
};

// ------------------------------------------------------------------------------------------------- colsum ---
// bias gradients of the head (rows = pixels, cols = classes) and of Conv2DTranspose (rows = 4 x pixels): the plan
// in float4 lanes, the plan of a source that is not 16-byte aligned, and colsum_workspace
struct Col {
    int64_t rows;
    int cols;
    int ctiles, CT;
    int64_t chunks, rpc;
    int s_ctiles, s_CT;
    int64_t s_chunks, s_rpc;
    size_t bytes;
};
static const Col kColsum[] = {
    {1048576, 1, 1, 1, 1024, 1024, 1, 1, 1024, 1024, 4096},
    {524288, 21, 1, 21, 1024, 512, 1, 21, 1024, 512, 86016},
    {16384, 512, 2, 64, 128, 128, 8, 64, 128, 128, 262144},
    {524288, 64, 1, 16, 1024, 512, 1, 64, 1024, 512, 262144},
    {768, 5, 1, 5, 6, 128, 1, 5, 6, 128, 256},
    {1517, 5, 1, 5, 12, 127, 1, 5, 12, 127, 256},
    {300, 3, 1, 3, 3, 100, 1, 3, 3, 100, 256},
    {129, 68, 1, 17, 2, 65, 2, 64, 2, 65, 768},
    {70, 16, 1, 4, 1, 70, 1, 16, 1, 70, 256},
};
static void check_col(const Col& r) {
    const ColsumPlan v = colsum_plan(r.rows, r.cols), s = colsum_plan(r.rows, r.cols, false);
    CHECK(v.red.ctiles == r.ctiles && v.red.CT == r.CT && v.red.chunks == r.chunks && v.red.rpc == r.rpc);
    CHECK(s.red.ctiles == r.s_ctiles && s.red.CT == r.s_CT && s.red.chunks == r.s_chunks && s.red.rpc == r.s_rpc);
    CHECK(v.bytes == r.bytes && v.need <= v.bytes && s.need <= v.bytes);
}

// ------------------------------------------------------------------------------------------------- sweeps ---
static bool aligned(size_t v) { return v % 256 == 0; }
static void check_red(int64_t rows, int cols) {
    const RedPlan v = red_plan(rows, cols), s = red_plan(rows, cols, false);
    for (const RedPlan& p : {v, s}) {
        CHECK(p.CT >= 1 && p.CT <= 64 && p.chunks >= 1 && p.rpc >= 1);
        CHECK(p.chunks * p.rpc >= rows && rows > (p.chunks - 1) * p.rpc);
    }
    CHECK((int64_t)v.CT * v.ctiles >= (cols % 4 == 0 ? cols / 4 : cols) && (int64_t)s.CT * s.ctiles >= cols);
    CHECK(s.chunks <= v.chunks);  // the scalar plan runs in the workspace the query sized for the vector plan
}
static void sweep() {
    const int64_t ms[] = {1, 127, 128, 129, 8192, 8193, 524288, 524293};
    const int cs[] = {1, 3, 4, 6, 64, 68, 260, 1024};
    const int Ss[] = {1, 63, 64, 65, 2049};
    for (int64_t m : ms)
        for (int c : cs) {
            const size_t ncnt = (size_t)cdiv(c, 64);
            const FwdPartials f = fwd_partials(m, c);
            CHECK(f.nblk * kStatsRows >= m && m > (f.nblk - 1) * kStatsRows);
            CHECK((int64_t)f.nch * kChunkParts >= f.nblk && f.nblk > (int64_t)(f.nch - 1) * kChunkParts);
            CHECK((size_t)f.nblk * c * 8 <= f.chunks_off && f.chunks_off + (size_t)f.nch * c * 16 <= f.counter_off);
            CHECK(f.counter_off + ncnt * 4 == f.bytes && aligned(f.chunks_off) && aligned(f.counter_off));
            CHECK(f.grid_x == ncnt);  // one counter per block column

            check_red(m, c);
            for (bool stats : {false, true}) {
                const BwdWorkspace w = bwd_workspace(m, c, stats);
                const size_t rows = (size_t)cdiv(w.red.chunks, kGroupSlabs);
                CHECK((size_t)w.red.chunks * 2 * c * 4 <= w.sums_off && w.sums_off + (size_t)2 * c * 4 <= w.scratch_off);
                CHECK(w.scratch_off + rows * 2 * c * 8 <= w.counter_off && w.counter_off + ncnt * 4 <= w.bytes);
                CHECK(aligned(w.sums_off) && aligned(w.scratch_off) && aligned(w.counter_off));
                CHECK(w.route == (!stats ? BWD_DZ : c % 4 == 0 ? BWD_STATS_FINISH : BWD_STATS_SLABS));
                CHECK(w.ncnt == (w.route == BWD_STATS_FINISH ? (int)ncnt : 0));
                CHECK(w.apply_grid >= 1 && w.apply_grid <= 65536);
                if (w.route == BWD_STATS_FINISH) {  // the finish launch finds its chunk rows and counters in the workspace
                    const StatsFinish f2 = stats_finish((int)w.red.chunks, c);
                    CHECK((size_t)f2.nch == rows && (size_t)f2.grid_x == ncnt);  // block column x counts on counter x
                }
            }
            const ColsumPlan cv = colsum_plan(m, c), csc = colsum_plan(m, c, false);
            CHECK(cv.need <= cv.bytes && csc.need <= cv.bytes);
        }
    for (int S : Ss)
        for (int c : cs) {
            if (c % 4) continue;  // the finish takes whole quads only
            const size_t ncnt = (size_t)cdiv(c, 64);
            const StatsFinish f = stats_finish(S, c);
            CHECK((int64_t)f.nch * kGroupSlabs >= S && S > (f.nch - 1) * kGroupSlabs);
            CHECK((size_t)S * 2 * c * 4 <= f.scratch_off && f.scratch_off + (size_t)f.nch * 2 * c * 8 <= f.counter_off);
            CHECK(f.counter_off + ncnt * 4 == f.bytes && aligned(f.scratch_off) && aligned(f.counter_off));
            CHECK((int)f.grid_x * kFinishQuads * 4 >= c && ((int)f.grid_x - 1) * kFinishQuads * 4 < c);
            CHECK((size_t)f.grid_x == ncnt);  // block column x counts on counter x: counters number cdiv(c, 64)
        }
}

int main() {
    for (const Fwd& r : kFwdNet) check_fwd(r);
    for (const Fwd& r : kFwdTests) check_fwd(r);
    for (const Fwd& r : kFwdBits) check_fwd(r);
    for (const Bwd& r : kBwdNet) check_bwd(r);
    for (const Bwd& r : kBwdTests) check_bwd(r);
    for (const Bwd& r : kBwdBits) check_bwd(r);
    for (const Fin& r : kFinNet) check_fin(r);
    for (const Fin& r : kFinTests) check_fin(r);
    for (const Fin& r : kFinBits) check_fin(r);
    for (const Col& r : kColsum) check_col(r);
    sweep();
    CHECK(grid_for(0) == 1 && grid_for(256) == 1 && grid_for(257) == 2 && grid_for((int64_t)1 << 40) == 65536);
    if (g_failed) {
        std::printf("bn_plan_check: %d checks failed\n", g_failed);
        return 1;
    }
    std::printf("bn_plan_check OK\n");
    return 0;
}
