// The rows GEMM C[M, N] = A[M, K] . B[K, N] (see gemm.h): the scalar fall-back kernel, the
// vectorised kernel (fp32 and split-precision bf16x6 "X6" k-loops, four epilogues), and
// launch_rows, which picks the tile (gemm_plan.h) and the kernel.
#include <type_traits>

#include "dispatch.h"
#include "gemm.h"

namespace unet {
namespace {

template <int BM, int BN, int AMODE, bool DROP, int EPI>
__global__ __launch_bounds__(256) void gemm_rows_kernel(RowsArgs g) {
    constexpr int LDA = BM + 4, LDB = BN + 4;
    constexpr int TM = BM / 64, TN = BN / 64;
    constexpr int AR = BM / 16;  // A elements per thread per stage
    constexpr int BR = BN / 16;  // B elements per thread per stage
    __shared__ float As[2][BK][LDA];
    __shared__ float Bs[2][BK][LDB];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int lo = lane & 31, hi = lane >> 5;
    const int64_t m0 = (int64_t)blockIdx.x * BM;
    const int n0 = blockIdx.y * BN;
    const int M_rem = (int)((g.M - m0) < BM ? (g.M - m0) : BM);

    // ---- A staging geometry: k-lane ak, rows arow0 + 16 r
    const int ak = tid & 15;
    const int arow0 = tid >> 4;
    int aoff[AR];
#pragma unroll
    for (int r = 0; r < AR; ++r) {
        const int rr = arow0 + 16 * r;
        if (rr < M_rem) {
            const int64_t m = m0 + rr;
            if constexpr (AMODE == A_UNSHUFFLE) {
                const int64_t hw = (int64_t)g.uH * g.uW;
                const int n = (int)(m / hw);
                const int rem = (int)(m - (int64_t)n * hw);
                const int i = rem / g.uW, j = rem - (rem / g.uW) * g.uW;
                aoff[r] = ((n * 2 * g.uH + 2 * i) * 2 * g.uW + 2 * j) * g.uf;
            } else {
                aoff[r] = (int)(m * g.a.c0);
            }
        } else {
            aoff[r] = -1;
        }
    }
    // ---- B staging geometry
    const bool bkc = g.sbk == 1;
    int bk_[BR], bn_[BR];
#pragma unroll
    for (int r = 0; r < BR; ++r) {
        if (bkc) {
            bk_[r] = tid & 15;
            bn_[r] = (tid >> 4) + 16 * r;
        } else {
            bn_[r] = tid % BN;
            bk_[r] = tid / BN + (256 / BN) * r;
        }
    }

    float ra[AR], rb[BR];
    auto load_stage = [&](int k0) {
        const int k = k0 + ak;
        const bool kv = k < g.K;
        int koff = k;
        float sc = 1.f, sh = 0.f;
        if constexpr (AMODE == A_UNSHUFFLE) koff = shuffle_tap_off(k, g.uW, g.uf);
        if constexpr (AMODE == A_BNRELU) {
            if (kv) {
                sc = g.a.sc0[k];
                sh = g.a.sh0[k];
            }
        }
#pragma unroll
        for (int r = 0; r < AR; ++r) {
            float v = 0.f;
            if (kv && aoff[r] >= 0) {
                v = g.a.src0[aoff[r] + koff];
                if constexpr (AMODE == A_BNRELU) v = bnrelu(v, sc, sh);
                if constexpr (DROP)
                    v *= drop_mult(g.a.seed, (uint64_t)(m0 + arow0 + 16 * r) * g.a.C + k, g.a.rate, g.a.inv_keep);
            }
            ra[r] = v;
        }
#pragma unroll
        for (int r = 0; r < BR; ++r) {
            const int kk = k0 + bk_[r], nn = n0 + bn_[r];
            rb[r] = (kk < g.K && nn < g.N) ? g.B[kk * g.sbk + nn * g.sbn] : 0.f;
        }
    };
    auto store_stage = [&](int buf) {
#pragma unroll
        for (int r = 0; r < AR; ++r) As[buf][ak][arow0 + 16 * r] = ra[r];
#pragma unroll
        for (int r = 0; r < BR; ++r) Bs[buf][bk_[r]][bn_[r]] = rb[r];
    };

    floatx16 acc[TM][TN];
#pragma unroll
    for (int tm = 0; tm < TM; ++tm)
#pragma unroll
        for (int tn = 0; tn < TN; ++tn)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[tm][tn][r] = 0.f;

    const int nk = (g.K + BK - 1) / BK;
    load_stage(0);
    store_stage(0);
    __syncthreads();
    for (int kt = 0; kt < nk; ++kt) {
        const int buf = kt & 1;
        if (kt + 1 < nk) load_stage((kt + 1) * BK);
#pragma unroll
        for (int kk = 0; kk < BK / 2; ++kk) {
            float av[TM], bv[TN];
#pragma unroll
            for (int tm = 0; tm < TM; ++tm) av[tm] = As[buf][2 * kk + hi][wm * (BM / 2) + tm * 32 + lo];
#pragma unroll
            for (int tn = 0; tn < TN; ++tn) bv[tn] = Bs[buf][2 * kk + hi][wn * (BN / 2) + tn * 32 + lo];
#pragma unroll
            for (int tm = 0; tm < TM; ++tm)
#pragma unroll
                for (int tn = 0; tn < TN; ++tn)
                    acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[tm], bv[tn], acc[tm][tn], 0, 0, 0);
        }
        if (kt + 1 < nk) store_stage(buf ^ 1);
        __syncthreads();
    }

    // ---------------------------------------------------------------- epilogue
    if constexpr (EPI == E_STORE || EPI == E_STATS) {
#pragma unroll
        for (int tm = 0; tm < TM; ++tm)
#pragma unroll
            for (int tn = 0; tn < TN; ++tn) {
                const int n = n0 + wn * (BN / 2) + tn * 32 + lo;
                if (n >= g.N) continue;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int rr = wm * (BM / 2) + tm * 32 + acc_row(r, hi);
                    if (rr < M_rem) g.C[(m0 + rr) * g.ldc + n] = acc[tm][tn][r];
                }
            }
    }
    if constexpr (EPI == E_STATS) {
        // per-column (count, mean, M2) over this block's valid rows: two passes in registers
        float* red = &As[0][0][0];
        float mean[TN];
#pragma unroll
        for (int tn = 0; tn < TN; ++tn) {
            const int col = wn * (BN / 2) + tn * 32 + lo;
            float s = 0.f;
#pragma unroll
            for (int tm = 0; tm < TM; ++tm)
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    if (wm * (BM / 2) + tm * 32 + acc_row(r, hi) < M_rem) s += acc[tm][tn][r];
            s += __shfl_xor(s, 32, 64);
            if (hi == 0) red[wm * BN + col] = s;
        }
        __syncthreads();
#pragma unroll
        for (int tn = 0; tn < TN; ++tn) {
            const int col = wn * (BN / 2) + tn * 32 + lo;
            mean[tn] = (red[col] + red[BN + col]) / (float)M_rem;
        }
        __syncthreads();
#pragma unroll
        for (int tn = 0; tn < TN; ++tn) {
            const int col = wn * (BN / 2) + tn * 32 + lo;
            float q = 0.f;
#pragma unroll
            for (int tm = 0; tm < TM; ++tm)
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    if (wm * (BM / 2) + tm * 32 + acc_row(r, hi) < M_rem) {
                        const float d = acc[tm][tn][r] - mean[tn];
                        q = fmaf(d, d, q);
                    }
            q += __shfl_xor(q, 32, 64);
            if (hi == 0) red[wm * BN + col] = q;
        }
        __syncthreads();
        if (wm == 0 && hi == 0) {
#pragma unroll
            for (int tn = 0; tn < TN; ++tn) {
                const int col = wn * (BN / 2) + tn * 32 + lo;
                const int n = n0 + col;
                if (n < g.N) g.stats[(int64_t)blockIdx.x * g.N + n] = make_float2(mean[tn], red[col] + red[BN + col]);
            }
        }
    }
    if constexpr (EPI == E_SHUFFLE) {
        const int64_t hw = (int64_t)g.sH * g.sW;
#pragma unroll
        for (int tn = 0; tn < TN; ++tn) {
            const int n = n0 + wn * (BN / 2) + tn * 32 + lo;
            if (n >= g.N) continue;
            const int ab = n / g.sf;
            const int co = n - ab * g.sf;
            const int a = ab >> 1, b = ab & 1;
            const float bias = g.bias ? g.bias[co] : 0.f;
#pragma unroll
            for (int tm = 0; tm < TM; ++tm)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int rr = wm * (BM / 2) + tm * 32 + acc_row(r, hi);
                    if (rr >= M_rem) continue;
                    const int64_t m = m0 + rr;
                    const int img = (int)(m / hw);
                    const int rem = (int)(m - img * hw);
                    const int i = rem / g.sW, j = rem - (rem / g.sW) * g.sW;
                    const int64_t o = ((int64_t)(img * 2 * g.sH + 2 * i + a) * (2 * g.sW) + 2 * j + b) * g.sf + co;
                    g.C[o] = acc[tm][tn][r] + bias;
                }
        }
    }
}

// ---------------------------------------------------------------- vectorised rows GEMM ----
// As[m][BK+4], Bs[n][BK+4] (k contiguous).  In a group of 8 k, MFMA step s takes k-slot 0 =
// k0+s and k-slot 1 = k0+4+s, so lane (row, half) feeds 4 consecutive MFMAs from ONE
// ds_read_b128 of its row.  Row stride BK+4 floats makes those reads conflict-free.
//
// X6 (split precision, see common.h split4 / mfma_x6): the staged A values are split into three
// bf16 planes as they are written to LDS ([row][k] images, k contiguous, row stride BK + 8 bf16 =
// conflict-free ds_read_b128); B arrives pre-split (g.Bx, [3][N][K] planes written once per weight
// update by unet_split_x3_ex) and is copied 16 bytes at a time.  Every 16-deep k step runs the six
// v_mfma_f32_32x32x16_bf16 of mfma_x6 per 32x32 tile: 6 x 32 cycles instead of the 8 x 64 of
// v_mfma_f32_32x32x2_f32, at fp32 accuracy.  The bf16 MFMA leaves 24 of its 32 issue cycles to
// VALU (the f32 MFMA shares the FP32 vector datapath), so the BN-backward operand transform and
// the split hide under the matrix work.  With 2.7x fewer matrix cycles per stage the load latency
// is what a stage must cover: X6 stages BK = 32 in ONE LDS buffer (61 KB at 128 x 128: two blocks
// per CU), loads of stage k+1 in registers while stage k computes, two barriers per stage (the
// co-resident block's MFMAs fill the store phase).  Loads, operand views and epilogues are shared.
#ifdef UNET_LAB_BUILD
__device__ unsigned long long lab_rows_stamps[65536 * 4];  // ROWS_STAMP (gemm.h): [block][4]
#endif

// The split-precision k-loop's form of UNET_BN_BWD_DZ4 (common.h), with the one contraction the
// expression allows written out: dz = sc * (g - p - (z - mu) * q) either rounds the product and
// subtracts (FUSE = false) or takes one fma (FUSE = true).  Under -ffp-contract=fast the compiler
// chose per inlined copy of store_stage -- separate rounding for stage 0, fma inside the loop -- and
// a restructured loop flipped the choice, which changes dz and dy bits (tests/test_rows_bits_gpu.py
// holds them).  The call sites now name the form; the results are those of that earlier code.
template <bool FUSE>
__device__ __forceinline__ float bn_bwd_dz_as(float g, float z, float sc, float sh, float mu, float p, float q) {
    g = fmaf(z, sc, sh) > 0.f ? g : 0.f;
    if constexpr (FUSE) {
        return sc * fmaf(-(z - mu), q, g - p);
    } else {
        float t = (z - mu) * q;
        asm("" : "+v"(t));  // (the rounded product: -ffp-contract=fast fuses across anything less)
        return sc * ((g - p) - t);
    }
}
template <bool FUSE>
__device__ __forceinline__ float4 bn_bwd_dz4_as(float4 g, float4 z, float4 sc, float4 sh, float4 mu, float4 p,
                                                float4 q) {
    return make_float4(bn_bwd_dz_as<FUSE>(g.x, z.x, sc.x, sh.x, mu.x, p.x, q.x),
                       bn_bwd_dz_as<FUSE>(g.y, z.y, sc.y, sh.y, mu.y, p.y, q.y),
                       bn_bwd_dz_as<FUSE>(g.z, z.z, sc.z, sh.z, mu.z, p.z, q.z),
                       bn_bwd_dz_as<FUSE>(g.w, z.w, sc.w, sh.w, mu.w, p.w, q.w));
}

template <int BM, int BN, int BK, int AMODE, bool DROP, int EPI, bool BKC, bool X6 = false>
__global__ __launch_bounds__(256, X6 ? 2 : 1) void gemm_rows_vec(RowsArgs g) {
    main_stream_prio();
    ROWS_STAGGER(g);
    ROWS_STAMP(g, 0);
    constexpr int LR = BK + 4;     // A (and k-contiguous B) LDS row stride, floats
    constexpr int LB = BN + 4;     // k-major B LDS row stride (n-contiguous weights)
    constexpr int XR = BK + 8;     // X6: bf16 row stride of the split planes
    constexpr int KQ = BK / 4;
    constexpr int NQ = BN / 4;
    constexpr int AQ = BM * KQ / 256;
    constexpr int BQ = BN * KQ / 256;
    constexpr int TM = BM / 64, TN = BN / 64;
    constexpr int BSZ = BKC ? BN * LR : BK * LB;
    constexpr int F32_BYTES = 4 * 2 * (BM * LR + BSZ);
    // X6 + BatchNorm backward: the five per-channel operand vectors (scale, shift, mu, p, q) of all
    // K <= X6_KMAX channels sit in LDS (read per stage), not in 20 live registers across the k-loop
    constexpr int X6_KMAX = 512;
    constexpr bool XCOEF = X6 && AMODE == A_BNBWD;
    constexpr int X6_BYTES = 2 * 3 * (BM + BN) * XR + (XCOEF ? 4 * 5 * X6_KMAX : 0);  // one buffer
    static_assert(!X6 || BK == 32, "X6 rows GEMM: 32-deep stages");
    __shared__ __attribute__((aligned(16))) char smem[X6 ? X6_BYTES : F32_BYTES];
    float* xcoef = reinterpret_cast<float*>(smem + 2 * 3 * (BM + BN) * XR);  // XCOEF: [5][X6_KMAX]
    // fp32 images (the X6 path uses the first bytes of As as epilogue scratch only)
    float (*As)[BM * LR] = reinterpret_cast<float (*)[BM * LR]>(smem);
    float (*Bs)[BSZ] = reinterpret_cast<float (*)[BSZ]>(smem + 4 * 2 * BM * LR);
    // X6 planes: Ax[plane * BM + row][k], Bx[plane * BN + col][k]
    unsigned short* Ax = reinterpret_cast<unsigned short*>(smem);
    unsigned short* Bx = Ax + 3 * BM * XR;
    // X6: B chunks (8 bf16 of one plane row) per thread and stage
    constexpr int XCH = BK / 8, XQ = 3 * BN * XCH / 256;
    static_assert(!X6 || (3 * BN * XCH) % 256 == 0, "X6: whole B chunks per thread");

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int lo = lane & 31, hi = lane >> 5;
    int mt, nt;  // row tile, column tile (the N-tiles of a row tile share its A rows through one L2)
    xcd_group_order(gridDim.x, gridDim.y, mt, nt);
    const int m0 = mt * BM;
    const int n0 = nt * BN;
    const int M_rem = (g.M - m0) < BM ? (int)(g.M - m0) : BM;
    const int K = g.K;

    // A: this thread stages k-quad kq of rows arow + (256/KQ) r
    const int kq = tid % KQ;
    const int arow = tid / KQ;
    int aoff[AQ];
#pragma unroll
    for (int r = 0; r < AQ; ++r) {
        const int rr = arow + (256 / KQ) * r;
        if (rr < M_rem) {
            const int m = m0 + rr;
            if constexpr (AMODE == A_UNSHUFFLE) {  // (0, 0) tap of pixel m: dU row 2 (m / uW), column 2 (m % uW)
                const int ur = m / g.uW;
                aoff[r] = (4 * ur * g.uW + 2 * (m - ur * g.uW)) * g.uf;
            } else {
                aoff[r] = m * g.a.c0;
            }
        } else {
            aoff[r] = -1;
        }
    }
    // B: per-thread element offsets at k0 = 0 (-1: column out of range); k advances by sbk
    const int sbk = (int)g.sbk, sbn = (int)g.sbn;
    const int bq_k = BKC ? tid % KQ : tid / NQ;      // k-quad (BKC) or k-row (n-contiguous)
    const int bq_n = BKC ? tid / KQ : tid % NQ;      // column (BKC) or n-quad
    int boff[BQ];
#pragma unroll
    for (int r = 0; r < BQ; ++r) {
        if constexpr (BKC) {
            const int n = n0 + bq_n + (256 / KQ) * r;
            boff[r] = n < g.N ? n * sbn + 4 * bq_k : -1;
        } else {
            const int n = n0 + 4 * bq_n;
            boff[r] = n < g.N ? (bq_k + (256 / NQ) * r) * sbk + n : -1;
        }
    }

    // Loads are issued unconditionally from clamped addresses; validity masks, the view
    // transform and dropout are applied when the registers are written to LDS, so no load is
    // waited for before the stage's MFMAs.
    float4 ra[AQ], rb[BQ];
    float4 rz[AMODE == A_BNBWD ? AQ : 1];
    float4 csc, csh, cmu, cp, cq;  // per-stage channel constants of this thread's k-quad
    int ak = 0;                    // k of this thread's A quad in the staged k-stage
    bool bok[BQ];
    uint4 rx[X6 ? XQ : 1];        // X6: staged B plane chunks
    bool xok[X6 ? XQ : 1];
    int xoff[X6 ? XQ : 1], xlds[X6 ? XQ : 1];  // chunk's plane-row element offset at k0 = 0 (-1: out of range) / LDS slot
    if constexpr (X6) {
        const int64_t plane = (int64_t)g.N * K;
#pragma unroll
        for (int j = 0; j < XQ; ++j) {
            const int c = tid + 256 * j;
            const int p = c / (BN * XCH), rem = c - p * (BN * XCH);
            const int row = rem / XCH, kc = rem - row * XCH;
            const int n = n0 + row;
            xoff[j] = n < g.N ? (int)(p * plane + (int64_t)n * K) + 8 * kc : -1;
            xlds[j] = (p * BN + row) * XR + 8 * kc;
        }
    }
    auto load_stage = [&](int k0) {
        const int k = k0 + 4 * kq;
        ak = k;
        if (k0 > 0 && ROWS_KO(g, 4)) return;  // lab: no k-loop operand loads
        const int kc = k < K ? k : 0;
        int koff = kc;
        if constexpr (AMODE == A_UNSHUFFLE) koff = shuffle_tap_off(kc, g.uW, g.uf);
        if constexpr ((AMODE == A_BNRELU || AMODE == A_BNBWD) && !XCOEF) {
            csc = ld4(g.a.sc0 + kc);
            csh = ld4(g.a.sh0 + kc);
        }
        if constexpr (AMODE == A_BNBWD && !XCOEF) {
            cmu = ld4(g.coef + kc);
            cp = ld4(g.coef + K + kc);
            cq = ld4(g.coef + 2 * K + kc);
        }
#pragma unroll
        for (int r = 0; r < AQ; ++r) {
            const int o = (aoff[r] < 0 ? 0 : aoff[r]) + koff;
            ra[r] = ld4(g.a.src0 + o);
            if constexpr (AMODE == A_BNBWD) rz[r] = ld4(g.z + o);
        }
        if constexpr (X6) {
#pragma unroll
            for (int j = 0; j < XQ; ++j) {  // (K % BK == 0 on this route: every chunk's k exists)
                xok[j] = xoff[j] >= 0;
                rx[j] = *reinterpret_cast<const uint4*>(g.Bx + (xok[j] ? xoff[j] + k0 : 0));
            }
        } else {
#pragma unroll
        for (int r = 0; r < BQ; ++r) {
            const int kk = BKC ? k0 + 4 * bq_k : k0 + bq_k + (256 / NQ) * r;
            bok[r] = boff[r] >= 0 && kk < K;
            rb[r] = ld4(g.B + (bok[r] ? boff[r] + (BKC ? k0 : k0 * sbk) : 0));
        }
        }
    };
    auto store_stage = [&](int buf, auto fuse) {
        const bool kv = ak < K;
        if constexpr (XCOEF) {  // (ak < K on this route: K % 32 == 0)
            csc = *reinterpret_cast<const float4*>(xcoef + ak);
            csh = *reinterpret_cast<const float4*>(xcoef + X6_KMAX + ak);
            cmu = *reinterpret_cast<const float4*>(xcoef + 2 * X6_KMAX + ak);
            cp = *reinterpret_cast<const float4*>(xcoef + 3 * X6_KMAX + ak);
            cq = *reinterpret_cast<const float4*>(xcoef + 4 * X6_KMAX + ak);
        }
#pragma unroll
        for (int r = 0; r < AQ; ++r) {
            float4 v = ra[r];
            if constexpr (AMODE == A_BNRELU) v = bnrelu4(v, csc, csh);
            if constexpr (DROP) {
                const uint64_t i = (uint64_t)(m0 + arow + (256 / KQ) * r) * g.a.C + (kv ? ak : 0);
                v = mul4(v, drop_mult4(g.a.seed, i, g.a.rate, g.a.inv_keep));
            }
            if constexpr (AMODE == A_BNBWD) {
                const float4 zz = rz[r];
                if constexpr (X6) {
                    v = bn_bwd_dz4_as<decltype(fuse)::value>(v, zz, csc, csh, cmu, cp, cq);
                } else {
                    UNET_BN_BWD_DZ4(v, zz, csc, csh, cmu, cp, cq);  // (as text: see common.h)
                }
            }
            if (!kv || aoff[r] < 0) v = f4(0.f);
            if constexpr (AMODE == A_BNBWD) {
                if (g.side && nt == 0 && kv && aoff[r] >= 0 && !ROWS_KO(g, 2)) st4(g.side + aoff[r] + ak, v);
            }
            const int row = arow + (256 / KQ) * r;
            if constexpr (X6) {
                const Split4 sp = split4(v);
                unsigned short* d = Ax + row * XR + 4 * kq;
                *reinterpret_cast<uint2*>(d) = sp.h;
                *reinterpret_cast<uint2*>(d + BM * XR) = sp.m;
                *reinterpret_cast<uint2*>(d + 2 * BM * XR) = sp.l;
            } else {
                *reinterpret_cast<float4*>(&As[buf][row * LR + 4 * kq]) = v;
            }
        }
        if constexpr (X6) {
#pragma unroll
            for (int j = 0; j < XQ; ++j)
                *reinterpret_cast<uint4*>(Bx + xlds[j]) = xok[j] ? rx[j] : make_uint4(0u, 0u, 0u, 0u);
            return;
        }
#pragma unroll
        for (int r = 0; r < BQ; ++r) {
            const float4 v = bok[r] ? rb[r] : f4(0.f);
            if constexpr (BKC) {
                *reinterpret_cast<float4*>(&Bs[buf][(bq_n + (256 / KQ) * r) * LR + 4 * bq_k]) = v;
            } else {
                *reinterpret_cast<float4*>(&Bs[buf][(bq_k + (256 / NQ) * r) * LB + 4 * bq_n]) = v;
            }
        }
    };

    floatx16 acc[TM][TN];
#pragma unroll
    for (int tm = 0; tm < TM; ++tm)
#pragma unroll
        for (int tn = 0; tn < TN; ++tn)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[tm][tn][r] = 0.f;

    const int nk = (K + BK - 1) / BK;
    if constexpr (XCOEF) {
        for (int i = tid; i < K; i += 256) {
            xcoef[i] = g.a.sc0[i];
            xcoef[X6_KMAX + i] = g.a.sh0[i];
            xcoef[2 * X6_KMAX + i] = g.coef[i];
            xcoef[3 * X6_KMAX + i] = g.coef[K + i];
            xcoef[4 * X6_KMAX + i] = g.coef[2 * K + i];
        }
    }
    load_stage(0);
    if constexpr (XCOEF) __syncthreads();
    store_stage(0, std::false_type{});
    __syncthreads();
    ROWS_STAMP(g, 1);
    if constexpr (X6) {
        auto mfma_stage = [&]() {
#pragma unroll
            for (int ks = 0; ks < BK / 16; ++ks) {
                // the wave's B fragments for this 16-deep step, then one row tile's A fragments at a
                // time (36 operand registers instead of 48)
                bf16x8 bfr[TN][3];
#pragma unroll
                for (int p = 0; p < 3; ++p)
#pragma unroll
                    for (int tn = 0; tn < TN; ++tn)
                        bfr[tn][p] = *reinterpret_cast<const bf16x8*>(
                            Bx + (p * BN + wn * (BN / 2) + tn * 32 + lo) * XR + ks * 16 + 8 * hi);
#pragma unroll
                for (int tm = 0; tm < TM; ++tm) {
                    bf16x8 af[3];
#pragma unroll
                    for (int p = 0; p < 3; ++p)
                        af[p] = *reinterpret_cast<const bf16x8*>(
                            Ax + (p * BM + wm * (BM / 2) + tm * 32 + lo) * XR + ks * 16 + 8 * hi);
#pragma unroll
                    for (int tn = 0; tn < TN; ++tn) acc[tm][tn] = mfma_x6(af, bfr[tn], acc[tm][tn]);
                }
            }
        };
        // The last stage is peeled off, so load_stage is unconditional inside the loop and the staged
        // registers live from the loads to the store phase of the SAME iteration.  Under
        // `if (kt + 1 < nk) load_stage(..)` they are carried around the loop instead, and the
        // compiler copies them to the carried set right behind the loads: a wait for the whole
        // prefetch in front of the stage's MFMAs (tools/kloop_waits.py checks it).
        for (int kt = 0; kt + 1 < nk; ++kt) {
            load_stage((kt + 1) * BK);
            __builtin_amdgcn_sched_barrier(0);  // every load is issued before the first MFMA ...
            mfma_stage();
            __builtin_amdgcn_sched_barrier(0);  // ... and nothing that consumes one moves up among them
            // one buffer: every wave's fragment reads are done before the next stage overwrites it
            __syncthreads();
            store_stage(0, std::true_type{});
            __syncthreads();
        }
        if (nk > 0) mfma_stage();
        __syncthreads();
    } else {
    for (int kt = 0; kt < nk; ++kt) {
        const int buf = kt & 1;
        if (kt + 1 < nk) load_stage((kt + 1) * BK);
        {
#pragma unroll
        for (int kg = 0; kg < BK / 8; ++kg) {
            float4 af[TM], bf[TN];
#pragma unroll
            for (int tm = 0; tm < TM; ++tm)
                af[tm] = *reinterpret_cast<const float4*>(&As[buf][(wm * (BM / 2) + tm * 32 + lo) * LR + kg * 8 + 4 * hi]);
#pragma unroll
            for (int tn = 0; tn < TN; ++tn) {
                const int col = wn * (BN / 2) + tn * 32 + lo;
                if constexpr (BKC) {
                    bf[tn] = *reinterpret_cast<const float4*>(&Bs[buf][col * LR + kg * 8 + 4 * hi]);
                } else {
                    const float* bp = &Bs[buf][(kg * 8 + 4 * hi) * LB + col];
                    bf[tn] = make_float4(bp[0], bp[LB], bp[2 * LB], bp[3 * LB]);
                }
            }
#pragma unroll
            for (int tm = 0; tm < TM; ++tm)
#pragma unroll
                for (int tn = 0; tn < TN; ++tn) {
                    acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[tm].x, bf[tn].x, acc[tm][tn], 0, 0, 0);
                    acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[tm].y, bf[tn].y, acc[tm][tn], 0, 0, 0);
                    acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[tm].z, bf[tn].z, acc[tm][tn], 0, 0, 0);
                    acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[tm].w, bf[tn].w, acc[tm][tn], 0, 0, 0);
                }
        }
        }
        if (kt + 1 < nk) store_stage(buf ^ 1, std::true_type{});
        __syncthreads();
    }
    }

    ROWS_STAMP(g, 2);
    const bool full = M_rem == BM;  // every row of the tile exists: no per-row checks
    if constexpr (EPI == E_STORE || EPI == E_STATS || EPI == E_BNPART) {
        const int ldc = (int)g.ldc;
#pragma unroll
        for (int tm = 0; tm < TM; ++tm)
#pragma unroll
            for (int tn = 0; tn < TN; ++tn) {
                const int n = n0 + wn * (BN / 2) + tn * 32 + lo;
                if (n >= g.N) continue;
                const int rb0 = wm * (BM / 2) + tm * 32 + 4 * hi;  // acc_row(r, hi) = rb0 + acc_row(r, 0)
                float* cp = g.C + (int64_t)(m0 + rb0) * g.ldc + n;
                if (ROWS_KO(g, 1)) continue;  // lab: no C stores
                if (full) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) cp[acc_row(r, 0) * ldc] = acc[tm][tn][r];
                } else {
#pragma unroll
                    for (int r = 0; r < 16; ++r)
                        if (rb0 + acc_row(r, 0) < M_rem) cp[acc_row(r, 0) * ldc] = acc[tm][tn][r];
                }
            }
    }
    if constexpr (EPI == E_STATS) {
        // Per-wave (mean, M2) over its BM/2 rows, then one Chan combine of the two row-halves
        // (one barrier); the partial is the (mean, M2) of the tile's M_rem rows.
        float2* red = reinterpret_cast<float2*>(&As[0][0]);
        const int wr0 = wm * (BM / 2);
        const int cnt = M_rem - wr0 < 0 ? 0 : (M_rem - wr0 < BM / 2 ? M_rem - wr0 : BM / 2);
#pragma unroll
        for (int tn = 0; tn < TN; ++tn) {
            const int col = wn * (BN / 2) + tn * 32 + lo;
            float s = 0.f;
#pragma unroll
            for (int tm = 0; tm < TM; ++tm)
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    if (full || wr0 + tm * 32 + acc_row(r, hi) < M_rem) s += acc[tm][tn][r];
            s += __shfl_xor(s, 32, 64);
            const float mean = cnt > 0 ? s / (float)cnt : 0.f;
            float q = 0.f;
#pragma unroll
            for (int tm = 0; tm < TM; ++tm)
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    if (full || wr0 + tm * 32 + acc_row(r, hi) < M_rem) {
                        const float d = acc[tm][tn][r] - mean;
                        q = fmaf(d, d, q);
                    }
            q += __shfl_xor(q, 32, 64);
            if (hi == 0) red[wm * BN + col] = make_float2(mean, q);
        }
        __syncthreads();
        if (wm == 0 && hi == 0) {
            const float na = (float)(M_rem < BM / 2 ? M_rem : BM / 2);
            const float nb = (float)M_rem - na;
#pragma unroll
            for (int tn = 0; tn < TN; ++tn) {
                const int col = wn * (BN / 2) + tn * 32 + lo;
                const int n = n0 + col;
                const float2 a = red[col], b = red[BN + col];
                float2 o = a;
                if (nb > 0.f) {
                    const float d = b.x - a.x;
                    const float f = nb / (float)M_rem;
                    o.x = a.x + d * f;
                    o.y = a.y + b.y + d * d * na * f;
                }
                if (n < g.N) g.stats[(int64_t)mt * g.N + n] = o;
            }
        }
    }
    if constexpr (EPI == E_BNPART) {
        // per column: this lane's 16*TM rows, the other row half (hi), then the other wave row (LDS);
        // fixed order, so the partials are deterministic
        float2* red = reinterpret_cast<float2*>(&As[0][0]);
        const int ldc = (int)g.ldc;
#pragma unroll
        for (int tn = 0; tn < TN; ++tn) {
            const int col = wn * (BN / 2) + tn * 32 + lo;
            const int n = n0 + col;
            float s1 = 0.f, s2 = 0.f;
            if (n < g.N) {
                const float sc = g.bsc[n], sh = g.bsh[n];
                const float mu = g.bmu ? g.bmu[n] : 0.f, rs = g.brs ? g.brs[n] : 0.f;
#pragma unroll
                for (int tm = 0; tm < TM; ++tm) {
                    const int rb0 = wm * (BM / 2) + tm * 32 + 4 * hi;
                    const float* zp = g.z + (int64_t)(m0 + rb0) * g.ldc + n;
                    float zv[16];
#pragma unroll
                    for (int r = 0; r < 16; ++r)
                        zv[r] = (full || rb0 + acc_row(r, 0) < M_rem) ? zp[acc_row(r, 0) * ldc] : 0.f;
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const bool in = full || rb0 + acc_row(r, 0) < M_rem;
                        float gm = (in && fmaf(zv[r], sc, sh) > 0.f) ? acc[tm][tn][r] : 0.f;
                        if (g.ep_rate > 0.f)  // (uniform) the consumer read the activation through dropout
                            gm *= drop_mult(g.ep_seed, (uint64_t)(m0 + rb0 + acc_row(r, 0)) * g.N + n, g.ep_rate,
                                            g.ep_inv_keep);
                        s1 += gm;
                        s2 = fmaf(gm, (zv[r] - mu) * rs, s2);
                    }
                }
            }
            s1 += __shfl_xor(s1, 32, 64);
            s2 += __shfl_xor(s2, 32, 64);
            if (hi == 0) red[wm * BN + col] = make_float2(s1, s2);
        }
        __syncthreads();
        if (wm == 0 && hi == 0) {
            float* out = g.bnpart + (int64_t)mt * 2 * g.N;
#pragma unroll
            for (int tn = 0; tn < TN; ++tn) {
                const int col = wn * (BN / 2) + tn * 32 + lo;
                const int n = n0 + col;
                const float2 a = red[col], b = red[BN + col];
                if (n < g.N) {
                    out[n] = a.x + b.x;
                    out[g.N + n] = a.y + b.y;
                }
            }
        }
    }
    if constexpr (EPI == E_SHUFFLE) {
        // output pixel offset (a = b = 0 tap) of each tile row: one row per thread through LDS
        // (the loop ended on a barrier) instead of two runtime integer divisions per accumulator
        // row in every thread (~2000 VALU instructions per thread)
        int* orow = reinterpret_cast<int*>(&As[0][0]);
        if (tid < BM) {
            const int m = m0 + tid;
            const int ur = m / g.sW;  // image row over the batch; output row 2 ur, column 2 (m % sW)
            orow[tid] = tid < M_rem ? (4 * ur * g.sW + 2 * (m - ur * g.sW)) * g.sf : -1;
        }
        __syncthreads();
        int obase[TM][16];
#pragma unroll
        for (int tm = 0; tm < TM; ++tm)
#pragma unroll
            for (int r = 0; r < 16; ++r) obase[tm][r] = orow[wm * (BM / 2) + tm * 32 + acc_row(r, hi)];
#pragma unroll
        for (int tn = 0; tn < TN; ++tn) {
            const int n = n0 + wn * (BN / 2) + tn * 32 + lo;
            if (n >= g.N) continue;
            const int ab = n / g.sf;
            const int co = n - ab * g.sf;
            const int toff = (ab >> 1) * (2 * g.sW * g.sf) + (ab & 1) * g.sf + co;
            const float bias = g.bias ? g.bias[co] : 0.f;
#pragma unroll
            for (int tm = 0; tm < TM; ++tm)
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    if (obase[tm][r] >= 0) g.C[(int64_t)obase[tm][r] + toff] = acc[tm][tn][r] + bias;
        }
    }
    ROWS_STAMP(g, 3);
}


template <int BN, int BKk, int AMODE, bool DROP, int EPI, bool X6 = false, int BM = 128>
void launch_rows_tile(const RowsArgs& a, hipStream_t st) {
    dim3 grid((unsigned)cdiv(a.M, BM), (unsigned)cdiv(a.N, BN));
    if (X6 || a.sbk == 1) gemm_rows_vec<BM, BN, BKk, AMODE, DROP, EPI, true, X6><<<grid, 256, 0, st>>>(a);
    else gemm_rows_vec<BM, BN, BKk, AMODE, DROP, EPI, false, X6><<<grid, 256, 0, st>>>(a);
}

}  // namespace

bool rows_vec_ok(const RowsArgs& a, int amode) {
    if (a.K % 4 || a.N % 4) return false;
    if (a.sbk * (int64_t)a.K + a.sbn * (int64_t)a.N >= (int64_t(1) << 31)) return false;
    if (amode == A_UNSHUFFLE && a.uf % 4) return false;
    if (amode != A_UNSHUFFLE && a.a.c0 % 4) return false;
    if (a.sbk != 1 && a.sbn != 1) return false;
    return ((uintptr_t)a.a.src0 | (uintptr_t)a.B) % 16 == 0;
}

template <int AMODE, bool DROP, int EPI>
int launch_rows(const RowsArgs& a0, hipStream_t st, const char* what) {
    RowsArgs a = a0;
    a.ko = lab_knob("UNET_ROWS_KO", 0);  // 1 no C stores, 2 no dz side copy, 4 no k-loop loads (lab)
    if (rows_vec_ok(a, AMODE)) {
        const RowsCfg c = rows_cfg(AMODE, a.M, a.K, a.N);
        if (rows_x6(AMODE, a.M, a.K, a.N, a.Bx != nullptr)) {
            launch_rows_tile<128, 32, AMODE, DROP, EPI, true>(a, st);
            UNET_CHECK_LAUNCH(what);
            return 0;
        }
        if constexpr (AMODE == A_BNBWD && EPI == E_STORE) {
            if (c.bm == 64) {
                launch_rows_tile<128, 32, AMODE, DROP, EPI, false, 64>(a, st);
                UNET_CHECK_LAUNCH(what);
                return 0;
            }
        }
        if constexpr (AMODE == A_UNSHUFFLE && EPI == E_BNPART) {
            if (convt_bnpart_bm(a.M, (int)a.N) == 64) {
                if (lab_knob("UNET_CONVT_BM64", 1) == 2) launch_rows_tile<128, 16, AMODE, DROP, EPI, false, 64>(a, st);
                else if (c.bk == 32) launch_rows_tile<64, 32, AMODE, DROP, EPI, false, 64>(a, st);
                else launch_rows_tile<64, 16, AMODE, DROP, EPI, false, 64>(a, st);
                UNET_CHECK_LAUNCH(what);
                return 0;
            }
        }
        // the (bn, bk) pairs that have a kernel, as 100 bn + bk; any other pair runs 128 x 16
        with_int<6416, 6432, 12832, 25616, 12816>(100 * c.bn + c.bk, [&](auto T) {
            launch_rows_tile<T() / 100, T() % 100, AMODE, DROP, EPI>(a, st);
        });
        UNET_CHECK_LAUNCH(what);
        return 0;
    }
    if constexpr (AMODE == A_BNBWD || EPI == E_BNPART) {  // vectorised kernel only
        UNET_CHECK_ARG(false, "%s: needs channel counts divisible by 4 and 16-B aligned operands", what);
    } else {
        with_bucket<64, 128>((int)a.N, [&](auto BN) {
            dim3 grid((unsigned)cdiv(a.M, 128), (unsigned)cdiv(a.N, BN()));
            gemm_rows_kernel<128, BN(), AMODE, DROP, EPI><<<grid, 256, 0, st>>>(a);
        });
        UNET_CHECK_LAUNCH(what);
    }
    return 0;
}

// the operand mode / dropout / epilogue triples the entry points use (pointwise.hip, convt.hip)
template int launch_rows<A_PLAIN, false, E_STORE>(const RowsArgs&, hipStream_t, const char*);
template int launch_rows<A_PLAIN, false, E_STATS>(const RowsArgs&, hipStream_t, const char*);
template int launch_rows<A_BNBWD, false, E_STORE>(const RowsArgs&, hipStream_t, const char*);
template int launch_rows<A_BNBWD, true, E_STORE>(const RowsArgs&, hipStream_t, const char*);
template int launch_rows<A_PLAIN, false, E_SHUFFLE>(const RowsArgs&, hipStream_t, const char*);
template int launch_rows<A_PLAIN, true, E_SHUFFLE>(const RowsArgs&, hipStream_t, const char*);
template int launch_rows<A_BNRELU, false, E_SHUFFLE>(const RowsArgs&, hipStream_t, const char*);
template int launch_rows<A_BNRELU, true, E_SHUFFLE>(const RowsArgs&, hipStream_t, const char*);
template int launch_rows<A_UNSHUFFLE, false, E_STORE>(const RowsArgs&, hipStream_t, const char*);
template int launch_rows<A_UNSHUFFLE, false, E_BNPART>(const RowsArgs&, hipStream_t, const char*);

}  // namespace unet
