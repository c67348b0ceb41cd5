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
    if (g_failed) return 1;
    std::printf("gemm_plan_check OK\n");
    return 0;
}
