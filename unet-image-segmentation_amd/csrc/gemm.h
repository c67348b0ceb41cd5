// FP32 MFMA GEMMs for the dense parts of the U-Net hot path (gfx950, v_mfma_f32_32x32x2_f32,
// exact f32: a k-ordered fmaf chain per output): what the translation units share.
//
//   gemm_rows  (gemm_rows.hip)  : C[M, N] = A[M, K] . B[K, N]   rows = pixels (NHWC), B = a small weight matrix
//                  - pointwise half of SeparableConv2D fwd (model/u_net.py:14-20) with a
//                    BatchNorm-statistics epilogue (u_net.py:22-23),
//                  - its data gradient,
//                  - Conv2DTranspose(2, stride 2) fwd (u_net.py:88-94) as [M, Cin] x [Cin, 4 Cout]
//                    with a pixel-shuffle + bias epilogue (non-overlapping 2x2 taps),
//                  - Conv2DTranspose data gradient (pixel-unshuffle A operand).
//   gemm_wgrad (gemm_wgrad.hip) : C[P, Q] = sum_m A[m, P] . B[m, Q]  (weight gradients, reduction over pixels),
//                split over m into slices; slices are summed in a fixed order (reduce_slabs),
//                so results are bitwise reproducible.
//   The entry points that fill RowsArgs / WgradArgs: pointwise.hip, convt.hip, imgblock.hip, head_bwd.hip.
//   The tile policy (host only): gemm_plan.h.
//
// Tiling (both kernels): 256 threads = 2x2 waves; each wave owns a (BM/2)x(BN/2) block of
// 32x32 MFMA tiles.  Operands are staged global -> registers -> LDS (k-major [BK][rows+4]
// images, so each MFMA operand fetch is one conflict-free ds_read_b32 per lane), double
// buffered: the next stage's global loads are in flight while the current stage's MFMAs run.
// The A operand passes through an activation view (BN+ReLU / dropout / unshuffle) on load.
#pragma once
#include "gemm_plan.h"
#include "view.h"

namespace unet {

struct RowsArgs {
    DView a;  // A operand: PLAIN/BNRELU -> a.src0[m * a.c0 + k]; UNSHUFFLE -> a.src0 = dU
    int64_t M;
    int K;
    int uH, uW, uf;  // UNSHUFFLE: m = (n, i, j) over uH x uW, dU is (n, 2uH, 2uW, uf)
    const float* B;
    int64_t sbk, sbn;
    int N;
    float* C;
    int64_t ldc;
    const float* bias;
    float2* stats;
    int sH, sW, sf;  // SHUFFLE epilogue: m = (n, i, j) over sH x sW, out (n, 2sH, 2sW, sf)
    const float* z;     // A_BNBWD: pre-BN z (same layout as a.src0)
    const float* coef;  // A_BNBWD: (mu, p, q) x C
    float* side;        // A_BNBWD: optional copy of the formed A (= dz), written by N-tile 0
    const float *bsc, *bsh, *bmu, *brs;  // E_BNPART: per-column BN scale/shift, mean/rstd (NULL: no xhat)
    float* bnpart;                       // E_BNPART: [cdiv(M, BM)][2][N] partial sums, one slab per row tile
                                         //   (BM = 64 or 128, convt_bnpart_bm; sized by the _slabs query)
    float ep_rate, ep_inv_keep;          // E_BNPART: dropout between the block and C's consumer (rate 0: none);
    uint64_t ep_seed;                    //   g also carries the mask of element (m, n) (common.h drop_mult)
    int ko;  // lab build only (UNET_ROWS_KO): knock-out bits for timing decompositions, else 0
    const unsigned short* Bx;  // split-precision route: B as three bf16 planes [3][N][K] (k contiguous), or NULL
};

struct WgradArgs {
    DView a;
    int P;
    int uH, uW, uf;  // A UNSHUFFLE geometry (m over uH x uW, dU (n, 2uH, 2uW, uf))
    DView b;
    int Q;
    int64_t M, mslice;
    float* slab;  // [S][P][Q]
    const float* bz;     // W_BNBWD: raw z (same layout as b.src0)
    const float* bcoef;  // W_BNBWD: (mu, p, q) x Q
    float* colpart;      // optional [S][P]: column sums of A over the block's m slice (vectorised kernel, q-tile 0)
};

// ------------------------------------------------------------------------ host interface ----
// C = A . B through the vectorised kernel where rows_vec_ok holds, else the scalar one (A_BNBWD and
// E_BNPART: vectorised only).  Defined in gemm_rows.hip, instantiated there for the
// (AMODE, DROP, EPI) triples the entry points use.
template <int AMODE, bool DROP, int EPI>
int launch_rows(const RowsArgs& a, hipStream_t st, const char* what);
bool rows_vec_ok(const RowsArgs& a, int amode);
// out[P][Q] = sum_m A(m, p) B(m, q); ws holds wgrad_workspace(M, P, Q) bytes (gemm_wgrad.hip)
int run_wgrad(WgradArgs a, int amode, int bmode, float* out, void* ws, size_t ws_bytes, hipStream_t st,
              const char* what);
size_t wgrad_workspace(int64_t M, int P, int Q);

inline DView plain_view(const float* p, int c) {
    unet_view v{};
    v.mode = UNET_VIEW_PLAIN;
    v.c0 = c;
    v.src0 = p;
    return make_dview(v);
}
inline bool fits_i32(int64_t a, int64_t b) { return a * b < (int64_t(1) << 31); }
// the `*_x3` entry points' operand check (B as three bf16 planes, read 16 bytes at a time);
// what = "entry point: argument"
inline int check_planes(const unsigned short* p, const char* what) {
    UNET_CHECK_ARG(p && (uintptr_t)p % 16 == 0, "%s must be a 16-B aligned plane set", what);
    return 0;
}

// ---------------------------------------------------------------------- device helpers ----
__device__ __forceinline__ int acc_row(int r, int hi) { return (r & 3) + 8 * (r >> 2) + 4 * hi; }

// XCD-aware placement: workgroups go to the 8 XCDs round-robin by linear id (x fastest), and each
// XCD has its own L2.  For a (groups x sibs) grid whose sibling blocks read the same operand rows
// (the N-tiles of one row tile, the (p, q) tiles of one m-slice), renumber the linear id so that
// all siblings of a group run on one XCD and share those rows through its L2 instead of each
// fetching them from HBM.  Needs groups % 8 == 0 (else the grid order is kept); same tiles, same
// arithmetic -- only where each tile runs changes.  grid x = groups, y = sibs.
__device__ __forceinline__ void xcd_group_order(int groups, int sibs, int& grp, int& sib) {
    grp = blockIdx.x;
    sib = blockIdx.y;
    if (sibs > 1 && (groups & 7) == 0) {
        const int L = blockIdx.x + blockIdx.y * groups, u = L >> 3;
        grp = (u / sibs) * 8 + (L & 7);
        sib = u % sibs;
    }
}
// the same with the siblings along grid x (the weight-gradient GEMMs: x = (p, q) tile, y = m-slice)
__device__ __forceinline__ void xcd_group_order_sx(int sibs, int groups, int& sib, int& grp) {
    sib = blockIdx.x;
    grp = blockIdx.y;
    if (sibs > 1 && (groups & 7) == 0) {
        const int L = blockIdx.x + blockIdx.y * sibs, u = L >> 3;
        grp = (u / sibs) * 8 + (L & 7);
        sib = u % sibs;
    }
}

// Pixel (un)shuffle: channel c = (a, b, co) of the [.., 4 f] side of a Conv2DTranspose(2, stride 2)
// GEMM lives at tap (a, b) of its pixel's 2x2 output patch in the (n, 2H, 2W, f) tensor; this is
// its element offset from the patch's (0, 0) tap.
__device__ __forceinline__ int shuffle_tap_off(int c, int W, int f) {
    const int ab = c / f;
    const int co = c - ab * f;
    return (ab >> 1) * (2 * W * f) + (ab & 1) * f + co;
}

// The accumulator-zero loop, the k-major MFMA stage and the weight-gradient slab store stay written
// out in each kernel: routed through inlined helpers the compiler scheduled the kernels differently
// (profiles/gemm_split_check.txt).

// ---------------------------------------------------------------------------- lab hooks ----
// Timing decompositions of the vectorised rows GEMM, live in the lab build only (RowsArgs::ko =
// UNET_ROWS_KO): bits 0-2 knock out C stores / the dz side copy / the k-loop operand loads;
// bits 8-15 = stagger (that many s_sleep 32, ~2048 cycles each) for the second half of the grid's
// blocks (bit 16: the odd blocks instead), so the two blocks sharing a CU do not run in lockstep;
// bit 17 = per-block stamps into lab_rows_stamps[block][4] (thread 0 only): s_memrealtime (100 MHz,
// device-wide) at start and end, s_memtime (shader cycles, per XCD) after the prologue stage and
// after the k-loop.
#ifdef UNET_LAB_BUILD
#define ROWS_KO(g, bit) (((g).ko & (bit)) != 0)
__device__ __forceinline__ void lab_stagger(int ko) {
    const int n = (ko >> 8) & 255;
    if (n == 0) return;
    const unsigned lin = blockIdx.x + blockIdx.y * gridDim.x, tot = gridDim.x * gridDim.y;
    const bool late = (ko & 0x10000) ? (lin & 1) : (lin >= tot / 2);
    if (late)
        for (int i = 0; i < n; ++i) __builtin_amdgcn_s_sleep(32);
}
#define ROWS_STAGGER(g) lab_stagger((g).ko)
// (lab_rows_stamps is defined in gemm_rows.hip, the one file that expands ROWS_STAMP)
#define ROWS_STAMP(g, i)                                                                       \
    do {                                                                                       \
        if (((g).ko & 0x20000) && threadIdx.x == 0) {                                          \
            const unsigned lin_ = blockIdx.x + blockIdx.y * gridDim.x;                         \
            if (lin_ < 65536) lab_rows_stamps[4 * lin_ + (i)] =                               \
                ((i) == 0 || (i) == 3) ? __builtin_amdgcn_s_memrealtime() : __builtin_amdgcn_s_memtime(); \
        }                                                                                      \
    } while (0)
#else
#define ROWS_KO(g, bit) false
#define ROWS_STAGGER(g) ((void)0)
#define ROWS_STAMP(g, i) ((void)0)
#endif

}  // namespace unet
