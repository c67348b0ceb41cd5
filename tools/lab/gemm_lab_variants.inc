// Variants of the rows GEMM timed by gemm_lab.hip (product kernel, tile configs).
#include "gemm_x.inc"
#define VAR(name, ...)                                                                          \
    {                                                                                           \
        double us = timeit([&] { __VA_ARGS__; });                                               \
        double d = maxdiff(C1, C0, n);                                                          \
        printf("  %-34s %8.1f us %7.1f TF/s  diff %.2e\n", name, us, fl / us * 1e-6, d);       \
        CK(hipMemset(C1, 0, n * 4));                                                            \
    }
template <int BM, int BN, int BKk, int AMODE, bool DROP, int EPI>
static void ltm(RowsArgs a, float* C) {
    a.C = C;
    dim3 grid((unsigned)cdiv(a.M, BM), (unsigned)cdiv(a.N, BN));
    if (a.sbk == 1) gemm_rows_vec<BM, BN, BKk, AMODE, DROP, EPI, true, false><<<grid, 256, 0, 0>>>(a);
    else gemm_rows_vec<BM, BN, BKk, AMODE, DROP, EPI, false, false><<<grid, 256, 0, 0>>>(a);
}
template <int BN, int BKk, int AMODE, bool DROP, int EPI>
static void lt2(RowsArgs a, float* C) { a.C = C; a.ko = getenv("LAB_KO") ? atoi(getenv("LAB_KO")) : 0; launch_rows_v2<BN, BKk, AMODE, DROP, EPI>(a, 0); }
template <int BN, int BKk, int AMODE, bool DROP, int EPI>
static void lt(RowsArgs a, float* C) { a.C = C; launch_rows_tile<BN, BKk, AMODE, DROP, EPI>(a, 0); }

static void stamps_report(const char* tag, unsigned nblocks) {
    std::vector<unsigned long long> h(4 * (size_t)nblocks);
    CK(hipMemcpyFromSymbol(h.data(), HIP_SYMBOL(lab_rows_stamps), 8 * 4 * (size_t)nblocks));
    unsigned long long s0 = ~0ull, s1 = 0, e0 = ~0ull, e1 = 0;
    std::vector<double> life, loop;
    for (unsigned b = 0; b < nblocks; ++b) {
        const unsigned long long* t = &h[4 * b];
        s0 = std::min(s0, t[0]); s1 = std::max(s1, t[0]); e0 = std::min(e0, t[3]); e1 = std::max(e1, t[3]);
        life.push_back((double)(t[3] - t[0]) * 0.01); loop.push_back((double)(t[2] - t[1]) / 2390.0);
    }
    std::sort(life.begin(), life.end()); std::sort(loop.begin(), loop.end());
    printf("  [stamps %s] blocks %u: first start -> last end %.1f us; starts spread %.1f us, ends spread %.1f us; "
           "block lifetime median %.1f us (min %.1f max %.1f); k-loop median %.1f us (max %.1f) at 2.39 GHz\n", tag,
           nblocks, (e1 - s0) * 0.01, (s1 - s0) * 0.01, (e1 - e0) * 0.01, life[life.size() / 2], life.front(),
           life.back(), loop[loop.size() / 2], loop.back());
}
template <bool D>
static void run_bnbwd(RowsArgs a, float* C0, float* C1, double fl, size_t n) {
        a.C = C0; launch_rows<A_BNBWD, D, E_STORE>(a, 0, "x");
        CK(hipDeviceSynchronize());
        VAR("product", a.C = C1; launch_rows<A_BNBWD, D, E_STORE>(a, 0, "x"));
        if (getenv("LAB_STAMPS")) {
            const RowsCfg c = rows_cfg(A_BNBWD, a.M, a.K, a.N);
            RowsArgs b = a; b.C = C1; b.ko = 0x20000;
            for (int rep = 0; rep < 3; ++rep) {
                if (c.bn == 256) launch_rows_tile<256, 16, A_BNBWD, D, E_STORE>(b, 0);
                else if (c.bn == 64) launch_rows_tile<64, 32, A_BNBWD, D, E_STORE>(b, 0);
                else launch_rows_tile<128, 32, A_BNBWD, D, E_STORE>(b, 0);
            }
            CK(hipDeviceSynchronize());
            stamps_report("product cfg", (unsigned)(cdiv(a.M, 128) * cdiv(a.N, c.bn)));
        }
        VAR("64x32", lt<64, 32, A_BNBWD, D, E_STORE>(a, C1));
        VAR("128x16", lt<128, 16, A_BNBWD, D, E_STORE>(a, C1));
        VAR("128x32", lt<128, 32, A_BNBWD, D, E_STORE>(a, C1));
        VAR("256x16", lt<256, 16, A_BNBWD, D, E_STORE>(a, C1));
        VAR("BM64 128x32", (ltm<64, 128, 32, A_BNBWD, D, E_STORE>(a, C1)));
        VAR("BM64 256x16", (ltm<64, 256, 16, A_BNBWD, D, E_STORE>(a, C1)));
        VAR("BM64 256x32", (ltm<64, 256, 32, A_BNBWD, D, E_STORE>(a, C1)));
        VAR("v2 64x32", lt2<64, 32, A_BNBWD, D, E_STORE>(a, C1));
        VAR("v2 128x16", lt2<128, 16, A_BNBWD, D, E_STORE>(a, C1));
        VAR("v2 128x32", lt2<128, 32, A_BNBWD, D, E_STORE>(a, C1));
        VAR("v2 256x16", lt2<256, 16, A_BNBWD, D, E_STORE>(a, C1));
        VAR("v2 256x32", lt2<256, 32, A_BNBWD, D, E_STORE>(a, C1));
}

static void run_variants(int mode, RowsArgs a, float* C0, float* C1, double fl, size_t n) {
    const RowsCfg c = rows_cfg(mode == 0 ? A_PLAIN : A_BNBWD, a.M, a.K, a.N);
    printf("  [product cfg %dx%d]\n", c.bn, c.bk);
    if (mode == 0) {
        a.C = C0; launch_rows<A_PLAIN, false, E_STATS>(a, 0, "x");
        CK(hipDeviceSynchronize());
        VAR("product", a.C = C1; launch_rows<A_PLAIN, false, E_STATS>(a, 0, "x"));
        VAR("64x16", lt<64, 16, A_PLAIN, false, E_STATS>(a, C1));
        VAR("64x32", lt<64, 32, A_PLAIN, false, E_STATS>(a, C1));
        VAR("128x16", lt<128, 16, A_PLAIN, false, E_STATS>(a, C1));
        VAR("128x32", lt<128, 32, A_PLAIN, false, E_STATS>(a, C1));
        VAR("256x16", lt<256, 16, A_PLAIN, false, E_STATS>(a, C1));
        VAR("BM64 128x32", (ltm<64, 128, 32, A_PLAIN, false, E_STATS>(a, C1)));
        VAR("BM64 256x32", (ltm<64, 256, 32, A_PLAIN, false, E_STATS>(a, C1)));
        VAR("v2 64x16", lt2<64, 16, A_PLAIN, false, E_STATS>(a, C1));
        VAR("v2 64x32", lt2<64, 32, A_PLAIN, false, E_STATS>(a, C1));
        VAR("v2 128x16", lt2<128, 16, A_PLAIN, false, E_STATS>(a, C1));
        VAR("v2 128x32", lt2<128, 32, A_PLAIN, false, E_STATS>(a, C1));
        VAR("v2 128x64", lt2<128, 64, A_PLAIN, false, E_STATS>(a, C1));
        VAR("v2 256x16", lt2<256, 16, A_PLAIN, false, E_STATS>(a, C1));
        VAR("v2 256x32", lt2<256, 32, A_PLAIN, false, E_STATS>(a, C1));
        if (getenv("LAB_X")) {
        VAR("x0 128x128x16 (no stats)", launch_x<128, 128, 16, 0>(a, C1));
        VAR("x6 LDS+MFMA only", launch_x<128, 128, 16, 6>(a, C1));
        VAR("x12 +A gload only", launch_x<128, 128, 16, 12>(a, C1));
        VAR("x13 +B gload only", launch_x<128, 128, 16, 13>(a, C1));
        VAR("x1 +barrier", launch_x<128, 128, 16, 1>(a, C1));
        VAR("x9 +gload+lds write, no barrier", launch_x<128, 128, 16, 9>(a, C1));
        VAR("x10 +gload only", launch_x<128, 128, 16, 10>(a, C1));
        VAR("x11 +lds write+barrier only", launch_x<128, 128, 16, 11>(a, C1));
        VAR("x0 BK32", launch_x<128, 128, 32, 0>(a, C1));
        VAR("x9 BK32", launch_x<128, 128, 32, 9>(a, C1));
        VAR("x10 BK32", launch_x<128, 128, 32, 10>(a, C1));
        VAR("x7 MFMA only", launch_x<128, 128, 16, 7>(a, C1));
        VAR("x7 MFMA only 4-acc order", launch_x<128, 128, 16, 8>(a, C1));
        }
    } else if (mode == 2) {  // Conv2DTranspose forward: pixel-shuffle + bias epilogue
        a.C = C0; launch_rows<A_PLAIN, false, E_SHUFFLE>(a, 0, "x");
        CK(hipDeviceSynchronize());
        VAR("product", a.C = C1; launch_rows<A_PLAIN, false, E_SHUFFLE>(a, 0, "x"));
        VAR("128x16", lt<128, 16, A_PLAIN, false, E_SHUFFLE>(a, C1));
        VAR("128x32", lt<128, 32, A_PLAIN, false, E_SHUFFLE>(a, C1));
        VAR("256x16", lt<256, 16, A_PLAIN, false, E_SHUFFLE>(a, C1));
        VAR("64x32", lt<64, 32, A_PLAIN, false, E_SHUFFLE>(a, C1));
        VAR("BM64 128x32", (ltm<64, 128, 32, A_PLAIN, false, E_SHUFFLE>(a, C1)));
        VAR("BM64 256x32", (ltm<64, 256, 32, A_PLAIN, false, E_SHUFFLE>(a, C1)));
        VAR("v2 128x32", lt2<128, 32, A_PLAIN, false, E_SHUFFLE>(a, C1));
        VAR("v2 128x64", lt2<128, 64, A_PLAIN, false, E_SHUFFLE>(a, C1));
        VAR("v2 256x32", lt2<256, 32, A_PLAIN, false, E_SHUFFLE>(a, C1));
    } else if (mode == 3) {  // Conv2DTranspose data gradient: A unshuffled on load
        a.C = C0; launch_rows<A_UNSHUFFLE, false, E_STORE>(a, 0, "x");
        CK(hipDeviceSynchronize());
        VAR("product", a.C = C1; launch_rows<A_UNSHUFFLE, false, E_STORE>(a, 0, "x"));
        VAR("128x16", lt<128, 16, A_UNSHUFFLE, false, E_STORE>(a, C1));
        VAR("128x32", lt<128, 32, A_UNSHUFFLE, false, E_STORE>(a, C1));
        VAR("256x16", lt<256, 16, A_UNSHUFFLE, false, E_STORE>(a, C1));
        VAR("64x32", lt<64, 32, A_UNSHUFFLE, false, E_STORE>(a, C1));
        VAR("BM64 128x32", (ltm<64, 128, 32, A_UNSHUFFLE, false, E_STORE>(a, C1)));
        VAR("BM64 256x32", (ltm<64, 256, 32, A_UNSHUFFLE, false, E_STORE>(a, C1)));
        VAR("v2 128x16", lt2<128, 16, A_UNSHUFFLE, false, E_STORE>(a, C1));
        VAR("v2 128x32", lt2<128, 32, A_UNSHUFFLE, false, E_STORE>(a, C1));
        VAR("v2 256x32", lt2<256, 32, A_UNSHUFFLE, false, E_STORE>(a, C1));
    } else if (getenv("LAB_DROP")) {
        run_bnbwd<true>(a, C0, C1, fl, n);
    } else {
        a.a.rate = 0.f;
        run_bnbwd<false>(a, C0, C1, fl, n);
    }
}
