// Stand-alone host check of sep_col_tiles (csrc/frozen_common.h), the column-block policy of the
// frozen sepconv launches (compiled and run by test_frozen_policy_host.py; host pass only, no GPU).
// Exit status 0 = every check passed; otherwise the failing lines are printed.
#include <cstdio>

#include "frozen_common.h"

using unet::frozen::sep_col_tiles;

static int g_failed = 0;
#define CHECK(cond)                                                    \
    do {                                                               \
        if (!(cond)) {                                                 \
            std::printf("FAILED line %d: %s\n", __LINE__, #cond);      \
            ++g_failed;                                                \
        }                                                              \
    } while (0)

int main() {
    // 128 columns (nt 4) where that divides cout, else 64, else 32; halved while gx * column blocks < 512
    const int64_t gx[4] = {1, 64, 256, 4096};
    const int cout[5] = {32, 64, 96, 128, 256};
    const int want[5][4] = {{1, 1, 1, 1},   // 32: one tile is all there is
                            {1, 1, 1, 2},   // 64: 2 once gx alone reaches 512
                            {1, 1, 1, 1},   // 96: not a multiple of 64
                            {1, 1, 2, 4},   // 128: 256 x 2 blocks = 512 keeps nt 2
                            {1, 1, 4, 4}};  // 256: 256 x 2 blocks = 512 keeps nt 4
    for (int i = 0; i < 5; ++i)
        for (int j = 0; j < 4; ++j) {
            const int nt = sep_col_tiles(cout[i], gx[j]);
            if (nt != want[i][j]) std::printf("cout %d gx %lld: nt %d, expected %d\n", cout[i], (long long)gx[j], nt, want[i][j]);
            CHECK(nt == want[i][j]);
            CHECK(cout[i] % (32 * nt) == 0);
        }
    if (g_failed) return 1;
    std::printf("frozen_policy_check OK\n");
    return 0;
}
