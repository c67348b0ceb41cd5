// Stand-alone host check of the GEMM tile policy (csrc/gemm_plan.h: rows_cfg, rows_x6, convt_bnpart_bm,
// wgrad_plan), compiled and run by test_gemm_plan_host.py; host pass only, no GPU.  The tables hold
// what the functions returned at the commit before csrc/gemm.hip was split, for every rows GEMM and
// weight gradient of the 256 x 256 train step (widths 64..1024, five levels) at batch 16, 8 and 32.
// Exit status 0 = every check passed; otherwise the failing lines are printed.
#include <cstdio>

#include "gemm_plan.h"

using namespace unet;

static int g_failed = 0;
#define CHECK(cond)                                               \
    do {                                                          \
        if (!(cond)) {                                            \
            std::printf("FAILED line %d: %s\n", __LINE__, #cond); \
            ++g_failed;                                           \
        }                                                         \
    } while (0)

// rows GEMM (amode, M, K, N): x6 = rows_x6 when the caller hands weight planes (without planes it is
// false); {bn, bk, bm} = rows_cfg (planes or not).  Per level: pointwise forward (A_PLAIN, E_STATS and
// E_STORE share the policy) and its BatchNorm-backward data gradient (A_BNBWD) of block 1, block 2 and
// the decoder's concat block; then the ConvT forward (A_BNRELU) and data gradient (A_UNSHUFFLE).
struct RowsCase {
    int amode;
    long long M;
    int K, N;
    bool x6;
    int bn, bk, bm;
};
static const RowsCase kRows[] = {
    // batch 16
    {A_PLAIN, 1048576, 64, 64, false, 64, 16, 128},
    {A_BNBWD, 1048576, 64, 64, false, 64, 32, 128},
    {A_PLAIN, 1048576, 128, 64, false, 64, 16, 128},
    {A_BNBWD, 1048576, 64, 128, true, 128, 32, 128},
    {A_PLAIN, 262144, 64, 128, true, 128, 16, 128},
    {A_BNBWD, 262144, 128, 64, false, 64, 32, 128},
    {A_PLAIN, 262144, 128, 128, true, 128, 16, 128},
    {A_BNBWD, 262144, 128, 128, true, 128, 32, 128},
    {A_PLAIN, 262144, 256, 128, true, 128, 32, 128},
    {A_BNBWD, 262144, 128, 256, true, 256, 16, 128},
    {A_PLAIN, 65536, 128, 256, true, 128, 16, 128},
    {A_BNBWD, 65536, 256, 128, true, 128, 32, 128},
    {A_PLAIN, 65536, 256, 256, true, 128, 32, 128},
    {A_BNBWD, 65536, 256, 256, true, 256, 16, 128},
    {A_PLAIN, 65536, 512, 256, true, 128, 32, 128},
    {A_BNBWD, 65536, 256, 512, true, 256, 16, 128},
    {A_PLAIN, 16384, 256, 512, true, 128, 32, 128},
    {A_BNBWD, 16384, 512, 256, true, 128, 32, 64},
    {A_PLAIN, 16384, 512, 512, true, 128, 32, 128},
    {A_BNBWD, 16384, 512, 512, true, 128, 32, 128},
    {A_PLAIN, 16384, 1024, 512, true, 128, 32, 128},
    {A_BNBWD, 16384, 512, 1024, true, 256, 16, 128},
    {A_PLAIN, 16384, 512, 1024, true, 128, 32, 128},  // (the GEMM the step runs there: dz pass + plain, cin >= 1024)
    {A_PLAIN, 4096, 512, 1024, true, 64, 32, 128},
    {A_BNBWD, 4096, 1024, 512, false, 128, 32, 64},
    {A_PLAIN, 4096, 1024, 1024, true, 64, 32, 128},
    {A_BNBWD, 4096, 1024, 1024, false, 128, 32, 64},
    {A_BNRELU, 4096, 1024, 2048, true, 128, 32, 128},
    {A_UNSHUFFLE, 4096, 2048, 1024, true, 64, 16, 128},
    {A_BNRELU, 16384, 512, 1024, true, 128, 32, 128},
    {A_UNSHUFFLE, 16384, 1024, 512, true, 128, 16, 128},
    {A_BNRELU, 65536, 256, 512, true, 128, 32, 128},
    {A_UNSHUFFLE, 65536, 512, 256, true, 128, 16, 128},
    {A_BNRELU, 262144, 128, 256, true, 128, 16, 128},
    {A_UNSHUFFLE, 262144, 256, 128, true, 128, 16, 128},
    // batch 8
    {A_PLAIN, 524288, 64, 64, false, 64, 16, 128},
    {A_BNBWD, 524288, 64, 64, false, 64, 32, 128},
    {A_PLAIN, 524288, 128, 64, false, 64, 16, 128},
    {A_BNBWD, 524288, 64, 128, true, 128, 32, 128},
    {A_PLAIN, 131072, 64, 128, true, 128, 16, 128},
    {A_BNBWD, 131072, 128, 64, false, 64, 32, 128},
    {A_PLAIN, 131072, 128, 128, true, 128, 16, 128},
    {A_BNBWD, 131072, 128, 128, true, 128, 32, 128},
    {A_PLAIN, 131072, 256, 128, true, 128, 32, 128},
    {A_BNBWD, 131072, 128, 256, true, 256, 16, 128},
    {A_PLAIN, 32768, 128, 256, true, 128, 16, 128},
    {A_BNBWD, 32768, 256, 128, true, 128, 32, 64},
    {A_PLAIN, 32768, 256, 256, true, 128, 32, 128},
    {A_BNBWD, 32768, 256, 256, true, 128, 32, 128},
    {A_PLAIN, 32768, 512, 256, true, 128, 32, 128},
    {A_BNBWD, 32768, 256, 512, true, 256, 16, 128},
    {A_PLAIN, 8192, 256, 512, true, 64, 32, 128},
    {A_BNBWD, 8192, 512, 256, false, 128, 32, 64},
    {A_PLAIN, 8192, 512, 512, true, 64, 32, 128},
    {A_BNBWD, 8192, 512, 512, true, 128, 32, 64},
    {A_PLAIN, 8192, 1024, 512, true, 64, 32, 128},
    {A_BNBWD, 8192, 512, 1024, true, 128, 32, 128},
    {A_PLAIN, 8192, 512, 1024, true, 128, 32, 128},
    {A_PLAIN, 2048, 512, 1024, false, 64, 32, 128},
    {A_BNBWD, 2048, 1024, 512, false, 128, 32, 64},
    {A_PLAIN, 2048, 1024, 1024, false, 64, 32, 128},
    {A_BNBWD, 2048, 1024, 1024, false, 128, 32, 64},
    {A_BNRELU, 2048, 1024, 2048, true, 64, 32, 128},
    {A_UNSHUFFLE, 2048, 2048, 1024, false, 64, 16, 128},
    {A_BNRELU, 8192, 512, 1024, true, 128, 32, 128},
    {A_UNSHUFFLE, 8192, 1024, 512, true, 64, 16, 128},
    {A_BNRELU, 32768, 256, 512, true, 128, 32, 128},
    {A_UNSHUFFLE, 32768, 512, 256, true, 128, 16, 128},
    {A_BNRELU, 131072, 128, 256, true, 128, 16, 128},
    {A_UNSHUFFLE, 131072, 256, 128, true, 128, 16, 128},
    // batch 32
    {A_PLAIN, 2097152, 64, 64, false, 64, 16, 128},
    {A_BNBWD, 2097152, 64, 64, false, 64, 32, 128},
    {A_PLAIN, 2097152, 128, 64, false, 64, 16, 128},
    {A_BNBWD, 2097152, 64, 128, true, 128, 32, 128},
    {A_PLAIN, 524288, 64, 128, true, 128, 16, 128},
    {A_BNBWD, 524288, 128, 64, false, 64, 32, 128},
    {A_PLAIN, 524288, 128, 128, true, 128, 16, 128},
    {A_BNBWD, 524288, 128, 128, true, 128, 32, 128},
    {A_PLAIN, 524288, 256, 128, true, 128, 32, 128},
    {A_BNBWD, 524288, 128, 256, true, 256, 16, 128},
    {A_PLAIN, 131072, 128, 256, true, 128, 16, 128},
    {A_BNBWD, 131072, 256, 128, true, 128, 32, 128},
    {A_PLAIN, 131072, 256, 256, true, 128, 32, 128},
    {A_BNBWD, 131072, 256, 256, true, 256, 16, 128},
    {A_PLAIN, 131072, 512, 256, true, 128, 32, 128},
    {A_BNBWD, 131072, 256, 512, true, 256, 16, 128},
    {A_PLAIN, 32768, 256, 512, true, 128, 32, 128},
    {A_BNBWD, 32768, 512, 256, true, 128, 32, 128},
    {A_PLAIN, 32768, 512, 512, true, 128, 32, 128},
    {A_BNBWD, 32768, 512, 512, true, 256, 16, 128},
    {A_PLAIN, 32768, 1024, 512, true, 128, 32, 128},
    {A_BNBWD, 32768, 512, 1024, true, 256, 16, 128},
    {A_PLAIN, 32768, 512, 1024, true, 128, 32, 128},
    {A_PLAIN, 8192, 512, 1024, true, 128, 32, 128},
    {A_BNBWD, 8192, 1024, 512, false, 128, 32, 64},
    {A_PLAIN, 8192, 1024, 1024, true, 128, 32, 128},
    {A_BNBWD, 8192, 1024, 1024, false, 128, 32, 128},
    {A_BNRELU, 8192, 1024, 2048, true, 128, 32, 128},
    {A_UNSHUFFLE, 8192, 2048, 1024, true, 128, 16, 128},
    {A_BNRELU, 32768, 512, 1024, true, 128, 32, 128},
    {A_UNSHUFFLE, 32768, 1024, 512, true, 128, 16, 128},
    {A_BNRELU, 131072, 256, 512, true, 128, 32, 128},
    {A_UNSHUFFLE, 131072, 512, 256, true, 128, 16, 128},
    {A_BNRELU, 524288, 128, 256, true, 128, 16, 128},
    {A_UNSHUFFLE, 524288, 256, 128, true, 128, 16, 128},
};

// convt_bnpart_bm(M, N): the ConvT data gradients with BatchNorm partials
struct BmCase {
    long long M;
    int N, bm;
};
static const BmCase kBm[] = {
    {4096, 1024, 128},
    {16384, 512, 128},
    {65536, 256, 128},
    {262144, 128, 128},
    {2048, 1024, 64},
    {8192, 512, 128},
    {32768, 256, 128},
    {131072, 128, 128},
    {8192, 1024, 128},
    {32768, 512, 128},
    {131072, 256, 128},
    {524288, 128, 128},
};

// wgrad_plan(M, P, Q) -> bp, bq, tiles, S, mslice: pointwise and ConvT weight gradients
struct WgradCase {
    long long M;
    int P, Q, bp, bq, tiles, S;
    long long mslice;
};
static const WgradCase kWgrad[] = {
    {1048576, 64, 64, 64, 64, 1, 1024, 1024},
    {1048576, 128, 64, 128, 64, 1, 1024, 1024},
    {262144, 64, 128, 64, 128, 1, 512, 512},
    {262144, 128, 128, 128, 128, 1, 512, 512},
    {262144, 256, 128, 128, 128, 2, 512, 512},
    {65536, 128, 256, 128, 128, 2, 128, 512},
    {65536, 256, 256, 128, 128, 4, 128, 512},
    {65536, 512, 256, 128, 128, 8, 128, 512},
    {16384, 256, 512, 128, 128, 8, 32, 512},
    {16384, 512, 512, 128, 128, 16, 32, 512},
    {16384, 1024, 512, 128, 128, 32, 32, 512},
    {4096, 512, 1024, 128, 128, 32, 8, 512},
    {4096, 1024, 1024, 128, 128, 64, 8, 512},
    {4096, 2048, 1024, 128, 128, 128, 8, 512},
    {16384, 1024, 512, 128, 128, 32, 32, 512},
    {65536, 512, 256, 128, 128, 8, 128, 512},
    {262144, 256, 128, 128, 128, 2, 512, 512},
    {524288, 64, 64, 64, 64, 1, 1024, 512},
    {524288, 128, 64, 128, 64, 1, 1024, 512},
    {131072, 64, 128, 64, 128, 1, 256, 512},
    {131072, 128, 128, 128, 128, 1, 256, 512},
    {131072, 256, 128, 128, 128, 2, 256, 512},
    {32768, 128, 256, 128, 128, 2, 64, 512},
    {32768, 256, 256, 128, 128, 4, 64, 512},
    {32768, 512, 256, 128, 128, 8, 64, 512},
    {8192, 256, 512, 128, 128, 8, 16, 512},
    {8192, 512, 512, 128, 128, 16, 16, 512},
    {8192, 1024, 512, 128, 128, 32, 16, 512},
    {2048, 512, 1024, 128, 128, 32, 4, 512},
    {2048, 1024, 1024, 128, 128, 64, 4, 512},
    {2048, 2048, 1024, 128, 128, 128, 4, 512},
    {8192, 1024, 512, 128, 128, 32, 16, 512},
    {32768, 512, 256, 128, 128, 8, 64, 512},
    {131072, 256, 128, 128, 128, 2, 256, 512},
    {2097152, 64, 64, 64, 64, 1, 1024, 2048},
    {2097152, 128, 64, 128, 64, 1, 1024, 2048},
    {524288, 64, 128, 64, 128, 1, 1024, 512},
    {524288, 128, 128, 128, 128, 1, 1024, 512},
    {524288, 256, 128, 128, 128, 2, 512, 1024},
    {131072, 128, 256, 128, 128, 2, 256, 512},
    {131072, 256, 256, 128, 128, 4, 256, 512},
    {131072, 512, 256, 128, 128, 8, 128, 1024},
    {32768, 256, 512, 128, 128, 8, 64, 512},
    {32768, 512, 512, 128, 128, 16, 64, 512},
    {32768, 1024, 512, 128, 128, 32, 32, 1024},
    {8192, 512, 1024, 128, 128, 32, 16, 512},
    {8192, 1024, 1024, 128, 128, 64, 16, 512},
    {8192, 2048, 1024, 128, 128, 128, 8, 1024},
    {32768, 1024, 512, 128, 128, 32, 32, 1024},
    {131072, 512, 256, 128, 128, 8, 128, 1024},
    {524288, 256, 128, 128, 128, 2, 512, 1024},
};

// The rows GEMMs the op tests launch (test_ops_gpu.py, test_x6_gpu.py, test_fenced_ops_gpu.py), as
// (amode, M, K, N, planes handed): pointwise forward (A_PLAIN, K = cin, N = cout), plain data gradient
// (A_PLAIN, K = cout, N = cin), BatchNorm-backward data gradient (A_BNBWD, K = cout, N = cin; from 1024
// channels on, the dz pass + the A_PLAIN GEMM), ConvT forward (A_BNRELU / A_PLAIN, K = cin, N = 4 cout)
// and data gradient (A_UNSHUFFLE, K = 4 cout, N = cin).  Expected values follow from the rules in
// gemm_plan.h by hand; x6 is what rows_x6 answers with those planes.  Only shapes the vectorised
// kernel takes (K, N multiples of 4) are listed: the scalar kernel has no tile policy.
struct OpRowsCase {
    int amode;
    long long M;
    int K, N;
    bool planes, x6;
    int bn, bk, bm;
};
static const OpRowsCase kOpRows[] = {
    // test_pointwise_and_bn_stats / test_pointwise_bwd (fp32 only)
    {A_PLAIN, 256, 64, 64, false, false, 64, 16, 128},
    {A_PLAIN, 300, 64, 128, false, false, 64, 16, 128},      // 3 tiles: narrow
    {A_PLAIN, 77, 32, 96, false, false, 64, 16, 128},
    {A_PLAIN, 512, 256, 512, false, false, 64, 32, 128},     // 16 tiles: narrow, K >= 256
    {A_PLAIN, 24653, 64, 64, false, false, 64, 16, 128},
    {A_PLAIN, 24653, 32, 128, false, false, 64, 16, 128},    // 193 tiles: narrow
    {A_PLAIN, 129, 64, 68, false, false, 64, 16, 128},       // the row x column tails
    {A_PLAIN, 127, 64, 48, false, false, 64, 16, 128},
    {A_PLAIN, 1, 64, 4, false, false, 64, 16, 128},
    {A_PLAIN, 129, 68, 64, false, false, 64, 16, 128},       // their data gradient (K = cout, N = cin)
    {A_PLAIN, 200, 512, 256, false, false, 64, 32, 128},     // test_pointwise_bwd (200, 256, 512)
    {A_PLAIN, 64, 1024, 1024, false, false, 64, 32, 128},
    // test_pointwise_fwd_x3
    {A_PLAIN, 33000, 96, 160, true, true, 128, 16, 128},     // 258 x 2 tiles
    {A_PLAIN, 33000, 96, 160, false, false, 128, 16, 128},
    {A_PLAIN, 16384, 512, 1024, true, true, 128, 32, 128},
    {A_PLAIN, 4096, 256, 256, true, false, 64, 32, 128},     // 64 tiles: narrow, fp32 route
    {A_PLAIN, 200, 48, 64, true, false, 64, 16, 128},
    // test_pointwise_bwd_data_bnrelu(_x3)
    {A_BNBWD, 300, 32, 16, false, false, 64, 32, 128},
    {A_BNBWD, 1000, 128, 64, false, false, 64, 32, 128},
    {A_BNBWD, 257, 64, 128, false, false, 128, 32, 64},      // 3 tiles, N >= 128: 64-row tiles
    {A_BNBWD, 129, 68, 64, false, false, 64, 32, 128},
    {A_BNBWD, 33000, 128, 96, true, true, 128, 32, 128},     // 258 tiles
    {A_BNBWD, 33000, 128, 96, false, false, 128, 32, 128},
    {A_BNBWD, 16384, 256, 256, true, true, 128, 32, 64},     // 128 x 2 = 256 tiles: still narrow (< 257)
    {A_BNBWD, 33000, 64, 512, true, true, 256, 16, 128},     // 258 x 2 >= 512
    {A_BNBWD, 33000, 64, 512, false, false, 256, 16, 128},
    {A_BNBWD, 33000, 48, 64, true, false, 64, 32, 128},      // K % 32 != 0
    {A_BNBWD, 4096, 256, 512, true, false, 128, 32, 64},     // 128 tiles
    {A_BNBWD, 40000, 64, 40, true, false, 64, 32, 128},
    {A_PLAIN, 33000, 1024, 128, true, true, 128, 32, 128},   // cout 1024: dz pass + plain GEMM
    {A_PLAIN, 33000, 1024, 128, false, false, 128, 32, 128},
    {A_PLAIN, 520, 64, 1024, false, false, 64, 16, 128},     // test_ops (520, 1024, 64)
    // ConvT forward / data gradient (test_conv_transpose, test_conv_transpose_fwd_x3, test_convt_bwd_data_bnstats_x3)
    {A_BNRELU, 32, 64, 128, false, false, 64, 16, 128},
    {A_BNRELU, 129, 64, 128, false, false, 64, 16, 128},
    {A_BNRELU, 33020, 64, 128, true, true, 128, 16, 128},    // (2, 130, 127, 64, 32): 258 tiles
    {A_BNRELU, 16384, 256, 512, true, true, 128, 32, 128},
    {A_BNRELU, 17589, 96, 160, true, true, 128, 16, 128},
    {A_BNRELU, 16, 1024, 2048, true, false, 64, 32, 128},
    {A_UNSHUFFLE, 129, 128, 64, false, false, 64, 16, 128},
    {A_UNSHUFFLE, 33020, 128, 64, true, false, 64, 16, 128},
    {A_UNSHUFFLE, 16384, 512, 256, true, true, 64, 16, 128},   // 256 tiles: narrow
    {A_UNSHUFFLE, 64, 2048, 1024, true, false, 64, 16, 128},
};

// convt_bnpart_bm for test_convt_bwd_data_bnstats(_x3): (M, N = cin)
static const BmCase kOpBm[] = {
    {128, 128, 64}, {35, 64, 64},  {72, 256, 64},      {512, 128, 64},  {36864, 128, 128},
    {1, 64, 64},    {127, 64, 64}, {129, 68, 64},      {33020, 64, 128}, {16384, 256, 128},
    {64, 1024, 64}, {72, 48, 64},
};

static void check_rows(int amode, long long M, int K, int N, bool x6, int bn, int bk, int bm) {
    const RowsCfg c = rows_cfg(amode, M, K, N);
    const bool ok = rows_x6(amode, M, K, N, true) == x6 && !rows_x6(amode, M, K, N, false) && c.bn == bn &&
                    c.bk == bk && c.bm == bm;
    if (!ok)
        std::printf("rows amode %d M %lld K %d N %d: x6 %d cfg {%d, %d, %d}, expected x6 %d {%d, %d, %d}\n", amode, M,
                    K, N, (int)rows_x6(amode, M, K, N, true), c.bn, c.bk, c.bm, (int)x6, bn, bk, bm);
    CHECK(ok);
}

int main() {
    // anchors derived by hand from the policy's rules
    check_rows(A_BNBWD, 16384, 512, 512, true, 128, 32, 128);   // 128 x 4 = 512 tiles of 128 x 128: X6
    check_rows(A_BNBWD, 65536, 256, 256, true, 256, 16, 128);   // 512 row tiles x 1: the 256-wide tile
    check_rows(A_BNBWD, 2048, 512, 512, false, 128, 32, 64);    // 64 tiles: under-filled, 64-row tiles, not X6
    check_rows(A_PLAIN, 4096, 1024, 512, false, 64, 32, 128);   // 128 tiles: narrow, not X6
    check_rows(A_PLAIN, 4096, 1024, 1024, true, 64, 32, 128);   // exactly 256 tiles: X6
    CHECK(convt_bnpart_bm(4096, 1024) == 128 && convt_bnpart_bm(2048, 1024) == 64);
    {
        const WgradPlan w = wgrad_plan(1048576, 64, 64);
        CHECK(w.bp == 64 && w.bq == 64 && w.tiles == 1 && w.S == 1024 && w.mslice == 1024);
    }
    for (const RowsCase& r : kRows) check_rows(r.amode, r.M, r.K, r.N, r.x6, r.bn, r.bk, r.bm);
    for (const BmCase& b : kBm) {
        const int bm = convt_bnpart_bm(b.M, b.N);
        if (bm != b.bm) std::printf("convt_bnpart_bm(%lld, %d) = %d, expected %d\n", b.M, b.N, bm, b.bm);
        CHECK(bm == b.bm);
    }
    for (const WgradCase& e : kWgrad) {
        const WgradPlan w = wgrad_plan(e.M, e.P, e.Q);
        const bool ok = w.bp == e.bp && w.bq == e.bq && w.tiles == e.tiles && w.S == e.S && w.mslice == e.mslice;
        if (!ok)
            std::printf("wgrad_plan(%lld, %d, %d) = {%d, %d, %d, %d, %lld}\n", e.M, e.P, e.Q, w.bp, w.bq, w.tiles, w.S,
                        (long long)w.mslice);
        CHECK(ok);
        CHECK(w.mslice % BK == 0 && (long long)w.S * w.mslice >= e.M);
    }
    // the op tests' shapes: each reaches the tile it is listed with, and every value the policy can
    // return is reached by a case whose M is not a multiple of the 128-row tile
    {
        const int kCfgs[][3] = {{64, 16, 128}, {64, 32, 128}, {128, 16, 128}, {128, 32, 128}, {256, 16, 128}, {128, 32, 64}};
        bool seen[6] = {}, x6_on = false, x6_off = false, bm64 = false, bm128 = false;
        for (const OpRowsCase& r : kOpRows) {
            const RowsCfg c = rows_cfg(r.amode, r.M, r.K, r.N);
            const bool x6 = rows_x6(r.amode, r.M, r.K, r.N, r.planes);
            const bool ok = x6 == r.x6 && c.bn == r.bn && c.bk == r.bk && c.bm == r.bm;
            if (!ok)
                std::printf("op rows amode %d M %lld K %d N %d planes %d: x6 %d cfg {%d, %d, %d}\n", r.amode, r.M, r.K, r.N,
                            (int)r.planes, (int)x6, c.bn, c.bk, c.bm);
            CHECK(ok);
            CHECK(r.K % 4 == 0 && r.N % 4 == 0);
            if (r.M % 128 == 0) continue;
            for (int i = 0; i < 6; ++i)
                // (the split-precision route runs its own 128 x 32 tile whatever rows_cfg says)
                if (!x6 && c.bn == kCfgs[i][0] && c.bk == kCfgs[i][1] && c.bm == kCfgs[i][2]) seen[i] = true;
            (x6 ? x6_on : x6_off) = true;
        }
        for (int i = 0; i < 6; ++i) {
            if (!seen[i]) std::printf("no ragged-M op case reaches {%d, %d, bm %d}\n", kCfgs[i][0], kCfgs[i][1], kCfgs[i][2]);
            CHECK(seen[i]);
        }
        CHECK(x6_on && x6_off);
        for (const BmCase& b : kOpBm) {
            const int bm = convt_bnpart_bm(b.M, b.N);
            if (bm != b.bm) std::printf("op convt_bnpart_bm(%lld, %d) = %d, expected %d\n", b.M, b.N, bm, b.bm);
            CHECK(bm == b.bm);
            if (b.M % 128) (bm == 64 ? bm64 : bm128) = true;
        }
        CHECK(bm64 && bm128);
        // the weight-gradient slice tail of test_pointwise_bwd (1033, 64, 68): two slices, the last ragged
        const WgradPlan w = wgrad_plan(1033, 64, 68);
        CHECK(w.S == 2 && w.mslice == 528 && w.bp == 64 && w.bq == 128 && 1033 - w.mslice < w.mslice);
    }
    if (g_failed) return 1;
    std::printf("gemm_plan_check OK\n");
    return 0;
}
