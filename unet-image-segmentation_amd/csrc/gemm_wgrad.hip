// The weight-gradient GEMM C[P, Q] = sum_m A[m, P] . B[m, Q] (see gemm.h): the scalar fall-back
// kernel, the vectorised kernel, and run_wgrad, which splits the pixels into slices
// (gemm_plan.h wgrad_plan), launches one block per (tile, slice) and sums the slabs in order.
// fp32 MFMA is the only route: a split-precision (bf16x6) form that split both operands as they
// were staged measured slower on every train-step shape (profiles/r6w_wgrad_x6_ab.txt) and was
// removed; a future one would read pre-split planes from memory as the rows GEMM does for B.
#include "dispatch.h"
#include "gemm.h"

namespace unet {
namespace {

template <int BP, int BQ, int AMODE, bool ADROP, int BMODE, bool BDROP>
__global__ __launch_bounds__(256) void gemm_wgrad_kernel(WgradArgs g) {
    constexpr int LDA = BP + 4, LDB = BQ + 4;
    constexpr int TM = BP / 64, TN = BQ / 64;
    constexpr int AR = BP / 16, BR = BQ / 16;
    constexpr int AS = 256 / BP, BS = 256 / BQ;  // row steps between a thread's staged elements
    __shared__ float As[2][BK][LDA];
    __shared__ float Bs[2][BK][LDB];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wp = wave >> 1, wq = wave & 1;
    const int lo = lane & 31, hi = lane >> 5;
    const int ntp = (g.P + BP - 1) / BP;
    const int p0 = (blockIdx.x % ntp) * BP;
    const int q0 = (blockIdx.x / ntp) * BQ;
    const int64_t mb = (int64_t)blockIdx.y * g.mslice;
    const int64_t me = mb + g.mslice < g.M ? mb + g.mslice : g.M;

    // A: this thread stages column p = p0 + ap, rows amm + AS*r of each stage
    const int ap = tid % BP, amm = tid / BP;
    const int p = p0 + ap;
    const bool pv = p < g.P;
    float asc = 1.f, ash = 0.f;
    int poff = p;
    if constexpr (AMODE == W_BNRELU) {
        if (pv) {
            asc = g.a.sc0[p];
            ash = g.a.sh0[p];
        }
    }
    if constexpr (AMODE == W_UNSHUFFLE) {
        const int ab = p / g.uf;
        const int co = p - ab * g.uf;
        poff = (ab >> 1) * (2 * g.uW * g.uf) + (ab & 1) * g.uf + co;
    }
    const int bq = tid % BQ, bmm = tid / BQ;
    const int q = q0 + bq;
    const bool qv = q < g.Q;
    float bsc = 1.f, bsh = 0.f;
    if constexpr (BMODE == W_BNRELU) {
        if (qv) {
            bsc = g.b.sc0[q];
            bsh = g.b.sh0[q];
        }
    }

    float ra[AR], rb[BR];
    auto load_stage = [&](int64_t k0) {
#pragma unroll
        for (int r = 0; r < AR; ++r) {
            const int64_t m = k0 + amm + AS * r;
            float v = 0.f;
            if (pv && m < me) {
                if constexpr (AMODE == W_UNSHUFFLE) {
                    const int64_t hw = (int64_t)g.uH * g.uW;
                    const int n = (int)(m / hw);
                    const int rem = (int)(m - n * hw);
                    const int i = rem / g.uW, j = rem - (rem / g.uW) * g.uW;
                    v = g.a.src0[(int64_t)((n * 2 * g.uH + 2 * i) * 2 * g.uW + 2 * j) * g.uf + poff];
                } else {
                    v = g.a.src0[m * g.a.c0 + p];
                    if constexpr (AMODE == W_BNRELU) v = bnrelu(v, asc, ash);
                    if constexpr (ADROP) v *= drop_mult(g.a.seed, (uint64_t)m * g.a.C + p, g.a.rate, g.a.inv_keep);
                }
            }
            ra[r] = v;
        }
#pragma unroll
        for (int r = 0; r < BR; ++r) {
            const int64_t m = k0 + bmm + BS * r;
            float v = 0.f;
            if (qv && m < me) {
                v = g.b.src0[m * g.b.c0 + q];
                if constexpr (BMODE == W_BNRELU) v = bnrelu(v, bsc, bsh);
                if constexpr (BDROP) v *= drop_mult(g.b.seed, (uint64_t)m * g.b.C + q, g.b.rate, g.b.inv_keep);
            }
            rb[r] = v;
        }
    };
    auto store_stage = [&](int buf) {
#pragma unroll
        for (int r = 0; r < AR; ++r) As[buf][amm + AS * r][ap] = ra[r];
#pragma unroll
        for (int r = 0; r < BR; ++r) Bs[buf][bmm + BS * r][bq] = rb[r];
    };

    floatx16 acc[TM][TN];
#pragma unroll
    for (int tm = 0; tm < TM; ++tm)
#pragma unroll
        for (int tn = 0; tn < TN; ++tn)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[tm][tn][r] = 0.f;

    const int nk = (int)((me - mb + BK - 1) / BK);
    if (nk > 0) {
        load_stage(mb);
        store_stage(0);
    }
    __syncthreads();
    for (int kt = 0; kt < nk; ++kt) {
        const int buf = kt & 1;
        if (kt + 1 < nk) load_stage(mb + (int64_t)(kt + 1) * BK);
#pragma unroll
        for (int kk = 0; kk < BK / 2; ++kk) {
            float av[TM], bv[TN];
#pragma unroll
            for (int tm = 0; tm < TM; ++tm) av[tm] = As[buf][2 * kk + hi][wp * (BP / 2) + tm * 32 + lo];
#pragma unroll
            for (int tn = 0; tn < TN; ++tn) bv[tn] = Bs[buf][2 * kk + hi][wq * (BQ / 2) + tn * 32 + lo];
#pragma unroll
            for (int tm = 0; tm < TM; ++tm)
#pragma unroll
                for (int tn = 0; tn < TN; ++tn)
                    acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[tm], bv[tn], acc[tm][tn], 0, 0, 0);
        }
        if (kt + 1 < nk) store_stage(buf ^ 1);
        __syncthreads();
    }
    float* slab = g.slab + (int64_t)blockIdx.y * g.P * g.Q;
#pragma unroll
    for (int tm = 0; tm < TM; ++tm)
#pragma unroll
        for (int tn = 0; tn < TN; ++tn) {
            const int qq = q0 + wq * (BQ / 2) + tn * 32 + lo;
            if (qq >= g.Q) continue;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int pp = p0 + wp * (BP / 2) + tm * 32 + acc_row(r, hi);
                if (pp < g.P) slab[(int64_t)pp * g.Q + qq] = acc[tm][tn][r];
            }
        }
}

// ------------------------------------------------------------- vectorised wgrad GEMM ----
// k-major LDS images As[m][BP + 4], Bs[m][BQ + 4] as in the scalar kernel, staged a float4 of
// channels at a time; the operand views (BN + ReLU, dropout, unshuffle, BN backward) are applied
// on load.
template <int BP, int BQ, int AMODE, bool ADROP, int BMODE, bool BDROP>
__global__ __launch_bounds__(256, 1) void gemm_wgrad_vec(WgradArgs g) {
    constexpr int LDA = BP + 4, LDB = BQ + 4;
    constexpr int TM = BP / 64, TN = BQ / 64;
    constexpr int PQ = BP / 4, QQ = BQ / 4;          // quads per m-row
    constexpr int AR = BK * PQ / 256, BR = BK * QQ / 256;
    constexpr int AS = 256 / PQ, BS = 256 / QQ;  // m-row step between a thread's quads
    __shared__ __attribute__((aligned(16))) char smem[4 * 2 * BK * (LDA + LDB)];
    float (*As)[BK * LDA] = reinterpret_cast<float (*)[BK * LDA]>(smem);
    float (*Bs)[BK * LDB] = reinterpret_cast<float (*)[BK * LDB]>(smem + 4 * 2 * BK * LDA);

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wp = wave >> 1, wq = wave & 1;
    const int lo = lane & 31, hi = lane >> 5;
    const int ntp = (g.P + BP - 1) / BP;
    int tile, slice;  // the (p, q) tiles of an m-slice read the same y / dz rows: one XCD's L2
    xcd_group_order_sx(gridDim.x, gridDim.y, tile, slice);
    const int p0 = (tile % ntp) * BP;
    const int q0 = (tile / ntp) * BQ;
    const int mb = (int)(slice * g.mslice);
    const int me = (int)((mb + g.mslice) < g.M ? (mb + g.mslice) : g.M);

    const int apq = tid % PQ, amm = tid / PQ;
    const int p = p0 + 4 * apq;
    const bool pv = p < g.P;
    float4 asc = f4(1.f), ash = f4(0.f);
    int poff = p;
    if constexpr (AMODE == W_BNRELU) {
        if (pv) {
            asc = ld4(g.a.sc0 + p);
            ash = ld4(g.a.sh0 + p);
        }
    }
    if constexpr (AMODE == W_UNSHUFFLE) {
        const int ab = p / g.uf;
        const int co = p - ab * g.uf;
        poff = (ab >> 1) * (2 * g.uW * g.uf) + (ab & 1) * g.uf + co;
    }
    const int bqq = tid % QQ, bmm = tid / QQ;
    const int q = q0 + 4 * bqq;
    const bool qv = q < g.Q;
    float4 bsc = f4(1.f), bsh = f4(0.f), bmu = f4(0.f), bp_ = f4(0.f), bq_ = f4(0.f);
    if constexpr (BMODE == W_BNRELU || BMODE == W_BNBWD) {
        if (qv) {
            bsc = ld4(g.b.sc0 + q);
            bsh = ld4(g.b.sh0 + q);
        }
    }
    if constexpr (BMODE == W_BNBWD) {
        if (qv) {
            bmu = ld4(g.bcoef + q);
            bp_ = ld4(g.bcoef + g.Q + q);
            bq_ = ld4(g.bcoef + 2 * g.Q + q);
        }
    }

    float4 ra[AR], rb[BR];
    // W_UNSHUFFLE: pixel m = (image row ur = m / uW over the batch, column uj) of the upsample input;
    // its (0, 0) tap in dU is row 2 ur, column 2 uj.  Tracked incrementally (the stages advance m
    // by BK) instead of two runtime divisions per row and stage.
    int ur[AMODE == W_UNSHUFFLE ? AR : 1], uj[AMODE == W_UNSHUFFLE ? AR : 1];
    if constexpr (AMODE == W_UNSHUFFLE) {
#pragma unroll
        for (int r = 0; r < AR; ++r) {
            const int m = mb + amm + AS * r;
            ur[r] = m / g.uW;
            uj[r] = m - ur[r] * g.uW;
        }
    }
    auto load_stage = [&](int k0) {
#pragma unroll
        for (int r = 0; r < AR; ++r) {
            const int m = k0 + amm + AS * r;
            float4 v = f4(0.f);
            if (pv && m < me) {
                if constexpr (AMODE == W_UNSHUFFLE) {
                    v = ld4(g.a.src0 + (4 * ur[r] * g.uW + 2 * uj[r]) * g.uf + poff);
                } else {
                    v = ld4(g.a.src0 + (int64_t)m * g.a.c0 + p);
                    if constexpr (AMODE == W_BNRELU) v = bnrelu4(v, asc, ash);
                    if constexpr (ADROP) {
                        const uint64_t i = (uint64_t)m * g.a.C + p;
                        v = mul4(v, drop_mult4(g.a.seed, i, g.a.rate, g.a.inv_keep));
                    }
                }
            }
            ra[r] = v;
        }
#pragma unroll
        for (int r = 0; r < BR; ++r) {
            const int m = k0 + bmm + BS * r;
            float4 v = f4(0.f);
            if (qv && m < me) {
                v = ld4(g.b.src0 + (int64_t)m * g.b.c0 + q);
                if constexpr (BMODE == W_BNRELU) v = bnrelu4(v, bsc, bsh);
                if constexpr (BMODE == W_BNBWD)
                    bn_bwd_dz4(v, ld4(g.bz + (int64_t)m * g.b.c0 + q), bsc, bsh, bmu, bp_, bq_);
                if constexpr (BDROP) {
                    const uint64_t i = (uint64_t)m * g.b.C + q;
                    v = mul4(v, drop_mult4(g.b.seed, i, g.b.rate, g.b.inv_keep));
                }
            }
            rb[r] = v;
        }
        if constexpr (AMODE == W_UNSHUFFLE) {
#pragma unroll
            for (int r = 0; r < AR; ++r) {
                uj[r] += BK;
                while (uj[r] >= g.uW) {
                    uj[r] -= g.uW;
                    ++ur[r];
                }
            }
        }
    };
    const bool csum_on = g.colpart != nullptr && tile < ntp;  // q-tile 0 blocks sum A's columns
    float4 csum = f4(0.f);
    auto store_stage = [&](int buf) {
#pragma unroll
        for (int r = 0; r < AR; ++r) *reinterpret_cast<float4*>(&As[buf][(amm + AS * r) * LDA + 4 * apq]) = ra[r];
#pragma unroll
        for (int r = 0; r < BR; ++r) *reinterpret_cast<float4*>(&Bs[buf][(bmm + BS * r) * LDB + 4 * bqq]) = rb[r];
        if (csum_on) {
#pragma unroll
            for (int r = 0; r < AR; ++r) csum = add4(csum, ra[r]);
        }
    };

    floatx16 acc[TM][TN];
#pragma unroll
    for (int tm = 0; tm < TM; ++tm)
#pragma unroll
        for (int tn = 0; tn < TN; ++tn)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[tm][tn][r] = 0.f;

    const int nk = (me - mb + BK - 1) / BK;
    if (nk > 0) {
        load_stage(mb);
        store_stage(0);
    }
    __syncthreads();
    for (int kt = 0; kt < nk; ++kt) {
        const int buf = kt & 1;
        if (kt + 1 < nk) load_stage(mb + (kt + 1) * BK);
#pragma unroll
        for (int kk = 0; kk < BK / 2; ++kk) {
            float av[TM], bv[TN];
#pragma unroll
            for (int tm = 0; tm < TM; ++tm) av[tm] = As[buf][(2 * kk + hi) * LDA + wp * (BP / 2) + tm * 32 + lo];
#pragma unroll
            for (int tn = 0; tn < TN; ++tn) bv[tn] = Bs[buf][(2 * kk + hi) * LDB + wq * (BQ / 2) + tn * 32 + lo];
#pragma unroll
            for (int tm = 0; tm < TM; ++tm)
#pragma unroll
                for (int tn = 0; tn < TN; ++tn)
                    acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[tm], bv[tn], acc[tm][tn], 0, 0, 0);
        }
        if (kt + 1 < nk) store_stage(buf ^ 1);
        __syncthreads();
    }
    if (csum_on) {  // fixed-order sum over the m-rows of each column quad (the loop ended on a barrier)
        float4* T = reinterpret_cast<float4*>(&As[0][0]);
        T[tid] = csum;
        __syncthreads();
        if (tid < PQ && pv) {
            float4 t = T[tid];
            for (int j = 1; j < AS; ++j) t = add4(t, T[j * PQ + tid]);
            st4(g.colpart + (int64_t)slice * g.P + p, t);
        }
    }
    float* slab = g.slab + (int64_t)slice * g.P * g.Q;
#pragma unroll
    for (int tm = 0; tm < TM; ++tm)
#pragma unroll
        for (int tn = 0; tn < TN; ++tn) {
            const int qq = q0 + wq * (BQ / 2) + tn * 32 + lo;
            if (qq >= g.Q) continue;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int pp = p0 + wp * (BP / 2) + tm * 32 + acc_row(r, hi);
                if (pp < g.P) slab[(int64_t)pp * g.Q + qq] = acc[tm][tn][r];
            }
        }
}

template <int AMODE, bool ADROP, int BMODE, bool BDROP>
void launch_wgrad_t(const WgradArgs& a, const WgradPlan& w, hipStream_t st) {
    dim3 grid((unsigned)w.tiles, (unsigned)w.S);
    const unsigned pad = (unsigned)lab_knob("UNET_WGRAD_LDSPAD", 0);  // lab: dynamic LDS pad (fewer blocks per CU)
    const bool vec = a.P % 4 == 0 && a.Q % 4 == 0 && (AMODE != W_UNSHUFFLE || a.uf % 4 == 0) &&
                     (AMODE == W_UNSHUFFLE || a.a.c0 % 4 == 0) && a.b.c0 % 4 == 0 &&
                     ((uintptr_t)a.a.src0 | (uintptr_t)a.b.src0) % 16 == 0;
    const bool vk = vec || BMODE == W_BNBWD;
    with_int<128, 64>(w.bp, [&](auto BP) {
        with_int<128, 64>(w.bq, [&](auto BQ) {
            if (vk) gemm_wgrad_vec<BP(), BQ(), AMODE, ADROP, BMODE, BDROP><<<grid, 256, pad, st>>>(a);
            else if constexpr (BMODE != W_BNBWD)  // (W_BNBWD: the vectorised kernel only)
                gemm_wgrad_kernel<BP(), BQ(), AMODE, ADROP, BMODE, BDROP><<<grid, 256, pad, st>>>(a);
        });
    });
}

}  // namespace

// out[P][Q] (row stride ldo) = sum_m A(m, p) B(m, q)
int run_wgrad(WgradArgs a, int amode, int bmode, float* out, void* ws, size_t ws_bytes, hipStream_t st,
              const char* what) {
    WgradPlan w = wgrad_plan(a.M, a.P, a.Q);
    const size_t need = (size_t)w.S * a.P * a.Q * sizeof(float);
    UNET_CHECK_ARG(ws && ws_bytes >= need, "%s: workspace %zu < %zu", what, ws_bytes, need);
    a.mslice = w.mslice;
    a.slab = static_cast<float*>(ws);
    const bool ad = a.a.rate > 0.f, bd = a.b.rate > 0.f;
    if (amode == W_PLAIN && bmode == W_PLAIN) {
        launch_wgrad_t<W_PLAIN, false, W_PLAIN, false>(a, w, st);
    } else if (amode == W_UNSHUFFLE && (bmode == W_BNRELU || bmode == W_PLAIN)) {
        with_int<W_BNRELU, W_PLAIN>(bmode, [&](auto BM) {
            with_bool(bd, [&](auto BD) { launch_wgrad_t<W_UNSHUFFLE, false, BM(), BD()>(a, w, st); });
        });
    } else if (amode == W_BNRELU && bmode == W_PLAIN) {
        with_bool(ad, [&](auto AD) { launch_wgrad_t<W_BNRELU, AD(), W_PLAIN, false>(a, w, st); });
    } else {
        UNET_CHECK_ARG(false, "%s: unsupported wgrad operand modes %d/%d", what, amode, bmode);
    }
    UNET_CHECK_LAUNCH(what);
    return reduce_slabs(a.slab, w.S, (int64_t)a.P * a.Q, out, (int64_t)a.P * a.Q, (int64_t)a.P * a.Q, st);
}

size_t wgrad_workspace(int64_t M, int P, int Q) {
    WgradPlan w = wgrad_plan(M, P, Q);
    return align_up((size_t)w.S * P * Q * sizeof(float), 256);
}

// head dW = sum_m x(m, k) dlogit(m, c): used by head_bwd.hip (declared in head.h)
int head_wgrad(const unet_view* x, int64_t M, const float* dlogit, int ncls, float* dkernel, void* ws, size_t ws_bytes,
               hipStream_t st) {
    WgradArgs a{};
    a.a = make_dview(*x);
    a.P = x->c0;
    a.b = plain_view(dlogit, ncls);
    a.Q = ncls;
    a.M = M;
    return run_wgrad(a, x->mode == UNET_VIEW_BNRELU ? W_BNRELU : W_PLAIN, W_PLAIN, dkernel, ws, ws_bytes, st,
                     "unet_head_bwd(filter)");
}
size_t head_wgrad_workspace(int64_t M, int cin, int ncls) { return wgrad_workspace(M, cin, ncls); }

}  // namespace unet
