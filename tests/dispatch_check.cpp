// Stand-alone host check of csrc/dispatch.h (compiled and run by test_dispatch_host.py).
// Exit status 0 = every check passed; otherwise the failing lines are printed.
#include <cstdio>

#include "dispatch.h"

using namespace unet;

static int g_failed = 0;
#define CHECK(cond)                                                    \
    do {                                                               \
        if (!(cond)) {                                                 \
            std::printf("FAILED line %d: %s\n", __LINE__, #cond);      \
            ++g_failed;                                                \
        }                                                              \
    } while (0)

template <int MODE, bool DROP>
int view_code() {
    return 10 * MODE + (DROP ? 1 : 0);
}

template <int A, int B>
int pair_code() {
    static_assert(!(A == 2 && B == 8), "the excluded combination must stay uninstantiated");
    return 100 * A + B;
}

int main() {
    // with_int: the first equal value, else the last one
    auto id = [](auto V) { return (int)V(); };
    CHECK((with_int<16, 8, 4, 2, 1>(16, id)) == 16);
    CHECK((with_int<16, 8, 4, 2, 1>(4, id)) == 4);
    CHECK((with_int<16, 8, 4, 2, 1>(1, id)) == 1);
    CHECK((with_int<16, 8, 4, 2, 1>(3, id)) == 1);
    CHECK((with_int<16, 8, 4, 2, 1>(-7, id)) == 1);
    CHECK((with_int<5, 7, 5, 9>(5, [](auto V) { return (int)V(); })) == 5);
    CHECK((with_int<3>(99, id)) == 3);

    // with_bool
    CHECK(with_bool(true, [](auto B) { return B() ? 1 : 2; }) == 1);
    CHECK(with_bool(false, [](auto B) { return B() ? 1 : 2; }) == 2);

    // with_view: 4 modes x 2, the constants usable as template arguments; other modes -> CONCAT
    auto code = [](auto M, auto D) { return view_code<M(), D()>(); };
    const int modes[4] = {UNET_VIEW_PLAIN, UNET_VIEW_BNRELU, UNET_VIEW_POOL_BNRELU, UNET_VIEW_CONCAT};
    for (int m : modes)
        for (int d = 0; d < 2; ++d) CHECK(with_view(m, d != 0, code) == 10 * m + d);
    CHECK(with_view(17, false, code) == 10 * UNET_VIEW_CONCAT);
    CHECK(with_view(-1, true, code) == 10 * UNET_VIEW_CONCAT + 1);

    // with_bucket: the first bound >= v
    CHECK((with_bucket<4, 8, 16, 24, 32>(1, id)) == 4);
    CHECK((with_bucket<4, 8, 16, 24, 32>(5, id)) == 8);
    CHECK((with_bucket<4, 8, 16, 24, 32>(16, id)) == 16);
    CHECK((with_bucket<4, 8, 16, 24, 32>(17, id)) == 24);
    CHECK((with_bucket<4, 8, 16, 24, 32>(32, id)) == 32);
    CHECK((with_bucket<4, 8, 16, 24, 32>(33, id)) == 32);

    // nested dispatch with one combination pruned by `if constexpr`: it compiles (pair_code<2, 8>
    // would trip its static_assert) and the pruned arm returns the sentinel
    auto nested = [](int a, int b) {
        return with_int<1, 2, 3>(a, [&](auto A) {
            return with_int<4, 8>(b, [&](auto B) {
                if constexpr (A() == 2 && B() == 8) return -1;
                else return pair_code<A(), B()>();
            });
        });
    };
    CHECK(nested(1, 4) == 104);
    CHECK(nested(2, 4) == 204);
    CHECK(nested(2, 8) == -1);
    CHECK(nested(3, 8) == 308);
    CHECK(nested(9, 9) == 308);

    // void lambdas (the launch sites) go through as well
    int hit = 0;
    with_view(UNET_VIEW_BNRELU, true, [&](auto M, auto D) { hit = view_code<M(), D()>(); });
    CHECK(hit == 11);

    if (g_failed == 0) std::printf("dispatch_check OK\n");
    return g_failed ? 1 : 0;
}
