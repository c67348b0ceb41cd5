// The last step of scripts/inference.py on the device: uint8 mask in, the bounding box of the
// external contour of largest cv2.contourArea out (reference scripts/inference.py:173-187;
// unet_amd/imageproc.py: largest_external_contour is the host tracer).  Border following is serial;
// the kernels compute the closed form of include/unet_hip.h ("Device-side largest-contour box"),
// which unet_amd/imageproc.py restates in NumPy (external_contour_stats_filled) and
// tests/test_contour_host.py holds equal to the tracer.  Integers only: results do not depend on
// the order in which blocks or atomics arrive.
//
// Labelling is union-find with the smallest linear index of a component as its root, so a label
// only ever decreases:
//   find   follows parents, each strictly smaller than its child, until a node is its own parent
//   union  links the larger of two roots under the smaller with an atomic min and goes on from the
//          value the atomic returned; it retries only when that value was smaller than the root it
//          meant to link (somebody else linked it first), so every retry lowers an index.
// No kernel waits for another workgroup: the phases meet at kernel boundaries on the stream.
//
//   A  the outer background O: background labelled with 4-connectivity; a background pixel on the
//      image border is united with the virtual outside node -1; O is the background whose root is
//      -1, F (the filled image) everything else.
//        cc_local<BG>   32x32 tile per block, labels in LDS, tile roots written as global indices
//        cc_merge<BG>   one thread per pixel on a tile seam: unions across it, agent-scope atomics
//        cc_fill        one byte per pixel: in F?  (and zeroes the per-root area sums)
//   B  the 8-connected components of F: cc_local<F>, cc_merge<F>, cc_flatten (label := root)
//   C  cc_area     twice the contour area, per 2x2 pixel cell, summed per root (a block whose cells
//                  share one root adds once)
//      cc_select   64-bit max over the roots of (area2 << 32) | ~first: the largest area, on ties
//                  the first in raster order; counts the roots
//      cc_bbox     min / max of x and y over the pixels of the winning root
//      cc_record   writes the 32-byte unet_contour_box
#include <limits.h>

#include "common.h"

namespace unet {
namespace {

constexpr int CC_BLOCK = 256;
constexpr int TILE = 32;          // a block labels a TILE x TILE tile, four rows per thread
constexpr int PER = 8;            // cells / pixels per thread of the two kernels that reduce per block
constexpr int NONE = INT_MAX;     // LDS label of a pixel outside the set: never a union's target
constexpr int OUTSIDE = -1;       // the virtual node of everything beyond the frame
constexpr int64_t MAX_PIXELS = (int64_t)1 << 30;  // linear indices and area2 are int32
constexpr size_t HEADER_BYTES = 256;

constexpr int WG = __HIP_MEMORY_SCOPE_WORKGROUP;
constexpr int AGENT = __HIP_MEMORY_SCOPE_AGENT;

struct Header {                 // the workspace's first bytes: the selection's accumulators
    unsigned long long best;    // max over the roots of (area2 << 32) | ~first; 0: no root
    int count;                  // roots = external contours
    int minx, miny, maxx, maxy;
};

// membership of the set a phase labels: the background of the mask, or the filled image
template <bool BG>
__device__ __forceinline__ bool member(unsigned char v) {
    return BG ? v == 0 : v != 0;
}

// the root of i (OUTSIDE for the virtual node); every step goes to a strictly smaller index
template <int SCOPE>
__device__ __forceinline__ int uf_find(int* lab, int i) {
    while (i >= 0) {
        const int parent = __hip_atomic_load(lab + i, __ATOMIC_RELAXED, SCOPE);
        if (parent == i) break;
        i = parent;
    }
    return i;
}

// Unites the components of a and b.  The larger root a (>= 0, so it has a slot) is put under the
// smaller with an atomic min.  The returned value decides: a itself, and a was still a root, now
// linked; anything else is smaller than a (somebody linked a first) and the slot now holds the
// smaller of that and b, so uniting the returned value with b completes the link whichever it was.
template <int SCOPE>
__device__ __forceinline__ void uf_union(int* lab, int a, int b) {
    for (;;) {
        a = uf_find<SCOPE>(lab, a);
        b = uf_find<SCOPE>(lab, b);
        if (a == b) return;
        if (a < b) {
            const int t = a;
            a = b;
            b = t;
        }
        const int old = __hip_atomic_fetch_min(lab + a, b, __ATOMIC_RELAXED, SCOPE);
        if (old == a) return;
        a = old;
    }
}

template <bool BG>
__global__ __launch_bounds__(CC_BLOCK) void cc_local_kernel(const unsigned char* __restrict__ src, int H, int W,
                                                            int tilesX, int* __restrict__ L, Header* hdr) {
    __shared__ int lab[TILE * TILE];
    const int tid = threadIdx.x, lx = tid & (TILE - 1), ly0 = tid >> 5;
    const int tx0 = (int)(blockIdx.x % (unsigned)tilesX) * TILE, ty0 = (int)(blockIdx.x / (unsigned)tilesX) * TILE;
    const int gx = tx0 + lx;
    if (BG && blockIdx.x == 0 && tid == 0) {  // the selection runs kernels later
        hdr->best = 0;
        hdr->count = 0;
        hdr->minx = hdr->miny = INT_MAX;
        hdr->maxx = hdr->maxy = -1;
    }
    bool in[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int ly = ly0 + 8 * k, gy = ty0 + ly;
        in[k] = gx < W && gy < H && member<BG>(src[gy * W + gx]);
        // a wave holds two tile rows; a pixel starts under the first pixel of its run in the row
        const unsigned row = (unsigned)(__ballot(in[k]) >> (tid & 32));
        const unsigned gaps = ~row & ((1u << lx) - 1u);
        const int start = gaps ? 32 - __clz(gaps) : 0;
        lab[ly * TILE + lx] = in[k] ? ly * TILE + start : NONE;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int ly = ly0 + 8 * k, gy = ty0 + ly, p = ly * TILE + lx;
        if (!in[k]) continue;
        if (ly > 0) {
            if (__hip_atomic_load(lab + p - TILE, __ATOMIC_RELAXED, WG) != NONE) {
                uf_union<WG>(lab, p, p - TILE);  // its row neighbours are in its run already
            } else if (!BG) {
                if (lx > 0 && __hip_atomic_load(lab + p - TILE - 1, __ATOMIC_RELAXED, WG) != NONE)
                    uf_union<WG>(lab, p, p - TILE - 1);
                if (lx < TILE - 1 && __hip_atomic_load(lab + p - TILE + 1, __ATOMIC_RELAXED, WG) != NONE)
                    uf_union<WG>(lab, p, p - TILE + 1);
            }
        }
        if (BG && (gx == 0 || gy == 0 || gx == W - 1 || gy == H - 1)) uf_union<WG>(lab, p, OUTSIDE);
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int ly = ly0 + 8 * k, gy = ty0 + ly;
        if (!in[k]) continue;
        const int r = uf_find<WG>(lab, ly * TILE + lx);
        L[gy * W + gx] = r < 0 ? OUTSIDE : (ty0 + (r >> 5)) * W + tx0 + (r & (TILE - 1));
    }
}

// Pixel p on a seam, q the pixel straight across it; along the seam the next pixel is `step` words on
// and p sits at position pos of len.  With q in the set the one union p - q also serves q's seam
// neighbours (they touch q), and it is left to the previous pixel's thread where that pixel and its
// own opposite are in the set AND in the same two tiles as p and q: the two pairs are then joined
// inside their tiles already.  (Not across a tile corner: there the previous pair's link is itself a
// seam union, and two seams could each leave the corner to the other.)  Without q, 8-connectivity
// still crosses the seam diagonally.
template <bool BG>
__device__ __forceinline__ void merge_across(const unsigned char* __restrict__ src, int* L, int p, int q, int step,
                                             int pos, int len) {
    if (member<BG>(src[q])) {
        if ((pos & (TILE - 1)) != 0 && member<BG>(src[p - step]) && member<BG>(src[q - step])) return;
        uf_union<AGENT>(L, p, q);
    } else if (!BG) {
        if (pos > 0 && member<BG>(src[q - step])) uf_union<AGENT>(L, p, q - step);
        if (pos < len - 1 && member<BG>(src[q + step])) uf_union<AGENT>(L, p, q + step);
    }
}

// One thread per pixel that lies on a seam between tiles: the first column of every tile column but
// the first (nV seams of H pixels), then the first row of every tile row but the first (seams of W
// pixels).  It unites its pixel with the neighbours across the seam.  Every access to L here is an
// agent-scope atomic: other workgroups change L while this one reads it.
template <bool BG>
__global__ __launch_bounds__(CC_BLOCK) void cc_merge_kernel(const unsigned char* __restrict__ src, int H, int W, int nV,
                                                            int64_t total, int* L) {
    int64_t t = (int64_t)blockIdx.x * CC_BLOCK + threadIdx.x;
    if (t >= total) return;
    const int64_t vertical = (int64_t)nV * H;
    if (t < vertical) {
        const int s = (int)(t / H), y = (int)(t - (int64_t)s * H), x = (s + 1) * TILE;
        const int p = y * W + x;
        if (member<BG>(src[p])) merge_across<BG>(src, L, p, p - 1, W, y, H);
    } else {
        t -= vertical;
        const int s = (int)(t / W), x = (int)(t - (int64_t)s * W), y = (s + 1) * TILE;
        const int p = y * W + x;
        if (member<BG>(src[p])) merge_across<BG>(src, L, p, p - W, 1, x, W);
    }
}

// in F: the foreground, and the background that does not reach the frame.  L is complete (earlier
// kernels wrote it), so plain loads.
__global__ __launch_bounds__(CC_BLOCK) void cc_fill_kernel(const unsigned char* __restrict__ mask, int n,
                                                           const int* __restrict__ L, unsigned char* __restrict__ kind,
                                                           int* __restrict__ area) {
    const int i = (int)((int64_t)blockIdx.x * CC_BLOCK + threadIdx.x);
    if (i >= n) return;
    bool filled = mask[i] != 0;
    if (!filled) {
        int r = i;
        while (r >= 0) {
            const int parent = L[r];
            if (parent == r) break;
            r = parent;
        }
        filled = r != OUTSIDE;
    }
    kind[i] = filled ? 1 : 0;
    area[i] = 0;
}

// label := root, in place beside the other workgroups' finds: agent-scope atomics again
__global__ __launch_bounds__(CC_BLOCK) void cc_flatten_kernel(const unsigned char* __restrict__ kind, int n, int* L) {
    const int i = (int)((int64_t)blockIdx.x * CC_BLOCK + threadIdx.x);
    if (i >= n || !kind[i]) return;
    __hip_atomic_store(L + i, uf_find<AGENT>(L, i), __ATOMIC_RELAXED, AGENT);
}

__device__ __forceinline__ int wave_sum_int(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// A thread per 2x2 pixel cell inside the image, PER cells per thread: 2 if all four pixels are in F,
// 1 if three are, added to the sum of the cell's component (three or more F pixels of a cell are
// 8-adjacent).  Every add to one root's sum goes to one address, so they are combined first: a thread
// sums the cells of the first root it meets, a wave whose threads agree on the root sums them, and
// the block adds its waves' sums once where their roots agree.  Whatever disagrees is added as it is.
__global__ __launch_bounds__(CC_BLOCK) void cc_area_kernel(const unsigned char* __restrict__ kind, int H, int W,
                                                           const int* __restrict__ L, int* area) {
    __shared__ int s_root[CC_BLOCK / 64], s_sum[CC_BLOCK / 64];
    const int tid = threadIdx.x, lane = tid & 63, cw = W - 1;
    const int64_t cells = (int64_t)(H - 1) * cw, base = (int64_t)blockIdx.x * (CC_BLOCK * PER);
    int my_root = -1, my_sum = 0;
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        const int64_t t = base + j * CC_BLOCK + tid;
        if (t >= cells) continue;
        const int y = (int)(t / cw), x = (int)(t - (int64_t)y * cw), p = y * W + x;
        const int k00 = kind[p], k01 = kind[p + 1], k10 = kind[p + W], k11 = kind[p + W + 1];
        const int s = k00 + k01 + k10 + k11;
        const int c = s == 4 ? 2 : (s == 3 ? 1 : 0);
        if (c == 0) continue;
        const int root = L[k00 ? p : p + 1];
        if (my_root < 0) my_root = root;
        if (root == my_root)
            my_sum += c;
        else
            atomicAdd(area + root, c);
    }
    int wave_root = -1, wave_total = 0;
    const unsigned long long active = __ballot(my_sum > 0);
    if (active != 0) {  // the whole wave takes the same way
        const int r0 = __shfl(my_root, __ffsll((long long)active) - 1, 64);
        if (__all(my_sum == 0 || my_root == r0)) {
            wave_root = r0;
            wave_total = wave_sum_int(my_sum);
        } else if (my_sum > 0) {
            atomicAdd(area + my_root, my_sum);
        }
    }
    if (lane == 0) {
        s_root[tid >> 6] = wave_root;
        s_sum[tid >> 6] = wave_total;
    }
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int a = 0; a < CC_BLOCK / 64; ++a) {
            int sum = s_sum[a];
            if (sum == 0) continue;
#pragma unroll
            for (int b = a + 1; b < CC_BLOCK / 64; ++b) {
                if (s_root[b] == s_root[a]) {
                    sum += s_sum[b];
                    s_sum[b] = 0;
                }
            }
            atomicAdd(area + s_root[a], sum);
        }
    }
}

__global__ __launch_bounds__(CC_BLOCK) void cc_select_kernel(const unsigned char* __restrict__ kind, int n,
                                                             const int* __restrict__ L, const int* __restrict__ area,
                                                             Header* hdr) {
    const int i = (int)((int64_t)blockIdx.x * CC_BLOCK + threadIdx.x);
    const bool root = i < n && kind[i] && L[i] == i;
    const unsigned long long roots = __ballot(root);
    if (roots == 0) return;  // the whole wave
    unsigned hi = root ? (unsigned)area[i] : 0u, lo = root ? ~(unsigned)i : 0u;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned ohi = __shfl_xor(hi, o, 64), olo = __shfl_xor(lo, o, 64);
        if (ohi > hi || (ohi == hi && olo > lo)) hi = ohi, lo = olo;
    }
    if ((threadIdx.x & 63) == 0) {
        atomicMax(&hdr->best, ((unsigned long long)hi << 32) | lo);
        atomicAdd(&hdr->count, __popcll(roots));
    }
}

// The extents of the winning root's pixels, PER pixels per thread, reduced over the wave and the
// block; the block's atomics are issued only where they would still move an extent (the value read
// first may be stale, which costs an atomic that changes nothing, never a missed one: extents only
// grow).
__global__ __launch_bounds__(CC_BLOCK) void cc_bbox_kernel(const unsigned char* __restrict__ kind, int H, int W,
                                                           const int* __restrict__ L, Header* hdr) {
    __shared__ int s_ext[CC_BLOCK / 64][4];
    const int tid = threadIdx.x, n = H * W;
    const int64_t base = (int64_t)blockIdx.x * (CC_BLOCK * PER);
    // best and count are an earlier kernel's; this one changes only the four extents
    const int winner = hdr->count > 0 ? (int)~(unsigned)hdr->best : -1;
    int x0 = INT_MAX, y0 = INT_MAX, x1 = -1, y1 = -1;
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        const int64_t t = base + j * CC_BLOCK + tid;
        if (t >= n) continue;
        const int i = (int)t;
        if (!kind[i] || L[i] != winner) continue;
        const int y = i / W, x = i - y * W;
        x0 = min(x0, x), y0 = min(y0, y), x1 = max(x1, x), y1 = max(y1, y);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        x0 = min(x0, __shfl_xor(x0, o, 64));
        y0 = min(y0, __shfl_xor(y0, o, 64));
        x1 = max(x1, __shfl_xor(x1, o, 64));
        y1 = max(y1, __shfl_xor(y1, o, 64));
    }
    if ((tid & 63) == 0) {
        s_ext[tid >> 6][0] = x0;
        s_ext[tid >> 6][1] = y0;
        s_ext[tid >> 6][2] = x1;
        s_ext[tid >> 6][3] = y1;
    }
    __syncthreads();
    if (tid != 0) return;
#pragma unroll
    for (int a = 1; a < CC_BLOCK / 64; ++a) {
        x0 = min(x0, s_ext[a][0]), y0 = min(y0, s_ext[a][1]);
        x1 = max(x1, s_ext[a][2]), y1 = max(y1, s_ext[a][3]);
    }
    if (x1 < 0) return;  // no pixel of the winner in this block
    if (x0 < __hip_atomic_load(&hdr->minx, __ATOMIC_RELAXED, AGENT)) atomicMin(&hdr->minx, x0);
    if (y0 < __hip_atomic_load(&hdr->miny, __ATOMIC_RELAXED, AGENT)) atomicMin(&hdr->miny, y0);
    if (x1 > __hip_atomic_load(&hdr->maxx, __ATOMIC_RELAXED, AGENT)) atomicMax(&hdr->maxx, x1);
    if (y1 > __hip_atomic_load(&hdr->maxy, __ATOMIC_RELAXED, AGENT)) atomicMax(&hdr->maxy, y1);
}

__global__ void cc_record_kernel(const Header* __restrict__ hdr, unet_contour_box* __restrict__ out) {
    unet_contour_box b;
    b.count = hdr->count;
    b.x = b.y = b.w = b.h = b.first = 0;
    b.area2 = 0;
    if (b.count > 0) {
        b.x = hdr->minx;
        b.y = hdr->miny;
        b.w = hdr->maxx - hdr->minx + 1;
        b.h = hdr->maxy - hdr->miny + 1;
        b.first = (int32_t)~(unsigned)hdr->best;
        b.area2 = (int64_t)(hdr->best >> 32);
    }
    *out = b;
}

struct Layout {
    size_t labels, area, kind, total;
};
Layout layout(int h, int w) {
    const size_t n = (size_t)h * (size_t)w;
    Layout l;
    l.labels = HEADER_BYTES;
    l.area = l.labels + align_up(4 * n, 256);
    l.kind = l.area + align_up(4 * n, 256);
    l.total = l.kind + align_up(n, 256);
    return l;
}

}  // namespace
}  // namespace unet

using namespace unet;

static_assert(sizeof(unet_contour_box) == 32, "unet_contour_box is 32 bytes");
static_assert(sizeof(Header) <= HEADER_BYTES, "the header fits its slot");

extern "C" size_t unet_mask_largest_contour_workspace(int h, int w) {
    if (h < 1 || w < 1 || (int64_t)h * w > MAX_PIXELS) return 0;
    return layout(h, w).total;
}

extern "C" int unet_mask_largest_contour(const unsigned char* mask, int h, int w, unet_contour_box* out, void* ws,
                                         size_t ws_bytes, unet_stream_t stream) {
    UNET_CHECK_ARG(mask && out && ws, "unet_mask_largest_contour: null pointer");
    UNET_CHECK_ARG(h >= 1 && w >= 1, "unet_mask_largest_contour: sizes must be positive, got %d x %d", h, w);
    UNET_CHECK_ARG((int64_t)h * w <= MAX_PIXELS,
                   "unet_mask_largest_contour: %d x %d is more than 2^30 pixels (indices and area2 are int32)", h, w);
    const Layout l = layout(h, w);
    UNET_CHECK_ARG(ws_bytes >= l.total, "unet_mask_largest_contour: workspace of %zu bytes, %zu needed", ws_bytes,
                   l.total);
    UNET_CHECK_ARG((uintptr_t)ws % 16 == 0 && (uintptr_t)out % 8 == 0,
                   "unet_mask_largest_contour: workspace must be 16-byte aligned, out 8-byte aligned");
    char* base = static_cast<char*>(ws);
    Header* hdr = reinterpret_cast<Header*>(base);
    int* L = reinterpret_cast<int*>(base + l.labels);
    int* area = reinterpret_cast<int*>(base + l.area);
    unsigned char* kind = reinterpret_cast<unsigned char*>(base + l.kind);
    const int n = h * w;
    const int tilesX = (int)cdiv(w, TILE), tilesY = (int)cdiv(h, TILE);
    const unsigned tiles = (unsigned)(tilesX * tilesY), pixels = (unsigned)cdiv(n, CC_BLOCK);
    const int64_t seams = (int64_t)(tilesX - 1) * h + (int64_t)(tilesY - 1) * w;
    const unsigned seam_blocks = (unsigned)cdiv(seams, CC_BLOCK);
    const int64_t cells = (int64_t)(h - 1) * (w - 1);
    hipStream_t st = as_stream(stream);

    cc_local_kernel<true><<<tiles, CC_BLOCK, 0, st>>>(mask, h, w, tilesX, L, hdr);
    if (seams > 0) cc_merge_kernel<true><<<seam_blocks, CC_BLOCK, 0, st>>>(mask, h, w, tilesX - 1, seams, L);
    cc_fill_kernel<<<pixels, CC_BLOCK, 0, st>>>(mask, n, L, kind, area);

    cc_local_kernel<false><<<tiles, CC_BLOCK, 0, st>>>(kind, h, w, tilesX, L, hdr);
    if (seams > 0) cc_merge_kernel<false><<<seam_blocks, CC_BLOCK, 0, st>>>(kind, h, w, tilesX - 1, seams, L);
    cc_flatten_kernel<<<pixels, CC_BLOCK, 0, st>>>(kind, n, L);

    if (cells > 0) cc_area_kernel<<<(unsigned)cdiv(cells, CC_BLOCK * PER), CC_BLOCK, 0, st>>>(kind, h, w, L, area);
    cc_select_kernel<<<pixels, CC_BLOCK, 0, st>>>(kind, n, L, area, hdr);
    cc_bbox_kernel<<<(unsigned)cdiv(n, CC_BLOCK * PER), CC_BLOCK, 0, st>>>(kind, h, w, L, hdr);
    cc_record_kernel<<<1, 1, 0, st>>>(hdr, out);
    UNET_CHECK_LAUNCH("unet_mask_largest_contour");
    return 0;
}
