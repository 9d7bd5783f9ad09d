// ccl.hip -- xdemhip_label: connected components of a class plane (scipy.ndimage.label's numbering); xdemhip_label_table: class, pixel
// count, bounding box and first pixel of every component; xdemhip_outlines: the outline rings of every component of a label plane in the
// vertex-table layout xdemhip_rasterize reads (geoutils' Raster.polygonize).  DESIGN.md 5r has the rule and the passes, include/xdemhip.h
// states the rule, tests/polygonize_oracle.py restates it in NumPy and every value of the test switch "ccl_route" returns its bits.  The
// only floating-point arithmetic is x = c + a j, y = f + e i (the Makefile builds this file with -ffp-contract=off).
//
// Labelling: union-find on a parent plane of linear indexes, parent[p] <= p always, so the root of a component is its smallest linear
// index whatever order the unions arrive in.  Every hand-off between workgroups is a kernel boundary: no spin-waiting, no flags, no grid
// barrier; every loop is a find or a union whose root strictly decreases.  (B = bytes per pixel, uint8 classes)
//   tile      a workgroup labels one tile of rows x columns in LDS (atomicMin unions with the left, upper and -- connectivity 8 --
//             upper diagonal neighbours), writes the tile-local roots as global linear indexes, -1 on background     read 1, write 4
//   border    a thread per pixel of a tile's first row or column unions it with its neighbours across the tile edge (the diagonal pair
//             at a four-tile corner among them): atomicMin retry loops, parents read through agent-scope atomic loads only: a plain
//             load may come from a vector L1 or another XCD's L2 that another workgroup's atomicMin never reached     (borders only)
//   flatten   every pixel finds its root, written to the label plane                                                  read 4+, write 4
//   number    roots are flagged (root[p] == p), counted per chunk of 1024 pixels, the counts scanned by one workgroup, and every root
//             stores rank + 1 where its parent was; then label[p] = that number of root[p]                            read 12, write 4
//   table     per-lane runs of equal labels within a row, flushed with 64-bit integer atomics keyed by label (add, min, max); the runs
//             of the workgroup's first label are gathered in LDS and flushed once                                       read 5
// Tracing, over the E corner edges only (edges whose successor changes direction; see the header for the successor rule):
//   corners   counted per pixel from its 3 x 3 neighbourhood, scanned by chunk as above, scattered in edge-number order: corner k of the
//             list is the k-th smallest corner edge, so an edge number is turned into a list index by a binary search
//   walk      each corner takes its successor and walks the straight run to the next corner of its ring (at most max(H, W) steps)
//   leader    pointer jumping, the minimum list index over 2^r successors after r rounds; one launch per round, double-buffered
//   rank      list ranking of the cycle cut at its leader, the same way: the distance to the leader
//   rings     leaders flagged and scanned; component, leader, length and the exact int64 signed area (integer atomics) of every ring
//             are fetched, ordered on the host by a stable counting sort on the component, and the ring offsets go back
//   gather    every corner writes its vertex at ring offset + position
// The number of rounds is ceil(log2(4 H W)), a bound on log2 E from the shape alone: the launch count of a call depends on H and W only.
#include "common.h"
#include "rank_select.h"
#include "../../include/xdemhip_test.h"

#include <limits.h>

#include <cmath>

namespace {

typedef unsigned long long u64;

constexpr int CCL_NT = 256;                    // threads of every workgroup here
constexpr int CCL_CHUNK = 1024;                // items of one workgroup of the counting scans: 256 lanes x 4
constexpr int CCL_LDS_BUDGET = 160 * 1024;
constexpr int CCL_RUN = 16;                    // consecutive pixels one thread of the table pass walks

struct CclPlan {
    int tr, tc, lds_bytes;
    int64_t tiles_r, tiles_c;
};

// 64 x 64 pixels: a class word and a parent word each, 32 KiB of LDS: four workgroups per CU, 16 pixels per lane.
inline CclPlan ccl_plan(int64_t H, int64_t W, int route_switch) {
    CclPlan p;
    p.tr = p.tc = route_switch == 2 ? 2 : 64;
    p.tiles_r = (H + p.tr - 1) / p.tr;
    p.tiles_c = (W + p.tc - 1) / p.tc;
    p.lds_bytes = p.tr * p.tc * 2 * (int)sizeof(int);
    return p;
}

#define CCL_LAUNCH(ctx, ...)             \
    do {                                 \
        hipLaunchKernelGGL(__VA_ARGS__); \
        ++(ctx)->ccl_launches;           \
    } while (0)

// ---- union-find ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int ccl_lds_find(int* par, int x) {
    int p;
    while ((p = __hip_atomic_load(par + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) != x) x = p;
    return x;
}
__device__ __forceinline__ void ccl_lds_union(int* par, int a, int b) {
    for (;;) {
        a = ccl_lds_find(par, a);
        b = ccl_lds_find(par, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(par + a, b);   // a > b: the larger root goes under the smaller
        if (old == a) return;
        a = old;                                 // somebody linked a first: go on from where it points
    }
}
__device__ __forceinline__ int32_t ccl_find(int32_t* par, int32_t x) {
    int32_t p;
    while ((p = __hip_atomic_load(par + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) != x) x = p;
    return x;
}
__device__ __forceinline__ void ccl_union(int32_t* par, int32_t a, int32_t b) {
    for (;;) {
        a = ccl_find(par, a);
        b = ccl_find(par, b);
        if (a == b) return;
        if (a < b) { const int32_t t = a; a = b; b = t; }
        const int32_t old = atomicMin(par + a, b);
        if (old == a) return;
        a = old;
    }
}

// ---- tile ---------------------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(CCL_NT) void ccl_tile_kernel(const T* __restrict__ cls, int32_t* __restrict__ parent, int64_t H, int64_t W, int tr, int tc,
                                                          int64_t tiles_c, int conn) {
    extern __shared__ int ccl_lds[];
    const int n = tr * tc;
    int* lc = ccl_lds;
    int* par = ccl_lds + n;
    const int64_t ty = (int64_t)blockIdx.x / tiles_c, tx = (int64_t)blockIdx.x - ty * tiles_c;
    const int64_t r0 = ty * tr, c0 = tx * tc;
    for (int i = threadIdx.x; i < n; i += CCL_NT) {
        const int lr = i / tc, lx = i - lr * tc;
        const int64_t r = r0 + lr, c = c0 + lx;
        lc[i] = r < H && c < W ? (int)cls[(size_t)r * (size_t)W + (size_t)c] : 0;
        par[i] = i;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += CCL_NT) {
        const int v = lc[i];
        if (!v) continue;
        const int lr = i / tc, lx = i - lr * tc;
        if (lx > 0 && lc[i - 1] == v) ccl_lds_union(par, i, i - 1);
        if (lr > 0) {
            if (lc[i - tc] == v) ccl_lds_union(par, i, i - tc);
            if (conn == 8) {
                if (lx > 0 && lc[i - tc - 1] == v) ccl_lds_union(par, i, i - tc - 1);
                if (lx < tc - 1 && lc[i - tc + 1] == v) ccl_lds_union(par, i, i - tc + 1);
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += CCL_NT) {
        const int lr = i / tc, lx = i - lr * tc;
        const int64_t r = r0 + lr, c = c0 + lx;
        if (r >= H || c >= W) continue;
        int32_t out = -1;
        if (lc[i]) {
            const int root = ccl_lds_find(par, i);
            const int rr = root / tc, rx = root - rr * tc;
            out = (int32_t)((r0 + rr) * W + c0 + rx);
        }
        parent[(size_t)r * (size_t)W + (size_t)c] = out;
    }
}

// ---- border: items [0, n_hb) are the pixels of the first rows of tile rows 1 .., the rest those of the first columns of tile columns 1 ..
template <typename T>
__global__ __launch_bounds__(CCL_NT) void ccl_border_kernel(const T* __restrict__ cls, int32_t* parent, int64_t H, int64_t W, int tr, int tc,
                                                            int64_t n_hb, int64_t n_items, int conn) {
    const int64_t i = (int64_t)blockIdx.x * CCL_NT + threadIdx.x;
    if (i >= n_items) return;
    if (i < n_hb) {
        const int64_t b = i / W, c = i - b * W, r = (b + 1) * tr;
        const int64_t p = r * W + c;
        const T v = cls[p];
        if (!v) return;
        if (cls[p - W] == v) ccl_union(parent, (int32_t)p, (int32_t)(p - W));
        if (conn == 8) {
            if (c > 0 && cls[p - W - 1] == v) ccl_union(parent, (int32_t)p, (int32_t)(p - W - 1));
            if (c < W - 1 && cls[p - W + 1] == v) ccl_union(parent, (int32_t)p, (int32_t)(p - W + 1));
        }
    } else {
        const int64_t j = i - n_hb, b = j / H, r = j - b * H, c = (b + 1) * tc;
        const int64_t p = r * W + c;
        const T v = cls[p];
        if (!v) return;
        if (cls[p - 1] == v) ccl_union(parent, (int32_t)p, (int32_t)(p - 1));
        if (conn == 8) {
            if (r > 0 && cls[p - W - 1] == v) ccl_union(parent, (int32_t)p, (int32_t)(p - W - 1));
            if (r < H - 1 && cls[p + W - 1] == v) ccl_union(parent, (int32_t)p, (int32_t)(p + W - 1));
        }
    }
}

__global__ __launch_bounds__(CCL_NT) void ccl_flatten_kernel(int32_t* parent, int32_t* __restrict__ root, int64_t n) {
    const int64_t p = (int64_t)blockIdx.x * CCL_NT + threadIdx.x;
    if (p >= n) return;
    root[p] = parent[p] < 0 ? -1 : ccl_find(parent, (int32_t)p);
}

__global__ __launch_bounds__(CCL_NT) void ccl_relabel_kernel(int32_t* __restrict__ label, const int32_t* __restrict__ number, int64_t n) {
    const int64_t p = (int64_t)blockIdx.x * CCL_NT + threadIdx.x;
    if (p >= n) return;
    const int32_t r = label[p];
    label[p] = r < 0 ? 0 : number[r];
}

// ---- counting scans: F::count(i) items of item i, F::emit(i, at) places them from `at` on; the order of the items is the order of i ----
template <typename F>
__global__ __launch_bounds__(CCL_NT) void ccl_count_kernel(F f, int64_t n, u64* __restrict__ cnt) {
    __shared__ int s[CCL_NT];
    const int64_t base = (int64_t)blockIdx.x * CCL_CHUNK + (int64_t)threadIdx.x * 4;
    int c = 0;
    for (int k = 0; k < 4; ++k)
        if (base + k < n) c += f.count(base + k);
    const int incl = xd::rank_block_scan(c, s);
    if (threadIdx.x == CCL_NT - 1) cnt[blockIdx.x] = (u64)incl;
}
template <typename F>
__global__ __launch_bounds__(CCL_NT) void ccl_emit_kernel(F f, int64_t n, const u64* __restrict__ off) {
    __shared__ int s[CCL_NT];
    const int64_t base = (int64_t)blockIdx.x * CCL_CHUNK + (int64_t)threadIdx.x * 4;
    int c[4], sum = 0;
    for (int k = 0; k < 4; ++k) {
        c[k] = base + k < n ? f.count(base + k) : 0;
        sum += c[k];
    }
    const int incl = xd::rank_block_scan(sum, s);
    u64 at = off[blockIdx.x] + (u64)(incl - sum);
    for (int k = 0; k < 4; ++k)
        if (c[k]) {
            f.emit(base + k, at);
            at += (u64)c[k];
        }
}

struct CclRoots {   // the roots of a flattened plane; root number k (from 0) stores k + 1 in `number`
    const int32_t* root;
    int32_t* number;
    __device__ int count(int64_t i) const { return root[i] == (int32_t)i; }
    __device__ void emit(int64_t i, u64 at) const { number[i] = (int32_t)(at + 1ull); }
};

// ---- table --------------------------------------------------------------------------------------------------------------------------
enum { CCL_T_CLASS = 0, CCL_T_COUNT, CCL_T_RMIN, CCL_T_RMAX, CCL_T_CMIN, CCL_T_CMAX, CCL_T_FIRST, CCL_T_COLS };

__global__ __launch_bounds__(CCL_NT) void ccl_table_init_kernel(long long* __restrict__ t, int64_t K) {
    const int64_t i = (int64_t)blockIdx.x * CCL_NT + threadIdx.x;
    if (i >= K) return;
    t[CCL_T_CLASS * K + i] = 0;
    t[CCL_T_COUNT * K + i] = 0;
    t[CCL_T_RMIN * K + i] = LLONG_MAX;
    t[CCL_T_RMAX * K + i] = -1;
    t[CCL_T_CMIN * K + i] = LLONG_MAX;
    t[CCL_T_CMAX * K + i] = -1;
    t[CCL_T_FIRST * K + i] = LLONG_MAX;
}

// `count` pixels of component L within rows r_lo .. r_hi and columns c_lo .. c_hi, the first of them at linear index `first`
template <typename T>
__device__ __forceinline__ void ccl_table_flush(long long* t, int64_t K, int32_t L, const T* __restrict__ cls, int64_t count, int64_t r_lo, int64_t r_hi,
                                                int64_t c_lo, int64_t c_hi, int64_t first) {
    if (L < 1 || L > K) return;   // (background, or a label plane that is not this table's: nothing is written out of bounds)
    const int64_t i = L - 1;
    atomicAdd(reinterpret_cast<u64*>(t + CCL_T_COUNT * K + i), (u64)count);
    atomicMin(t + CCL_T_RMIN * K + i, (long long)r_lo);
    atomicMax(t + CCL_T_RMAX * K + i, (long long)r_hi);
    atomicMin(t + CCL_T_CMIN * K + i, (long long)c_lo);
    atomicMax(t + CCL_T_CMAX * K + i, (long long)c_hi);
    atomicMin(t + CCL_T_FIRST * K + i, (long long)first);
    t[CCL_T_CLASS * K + i] = (long long)cls[first];   // (every pixel of a component holds the same class)
}

// A lane walks CCL_RUN consecutive pixels and flushes every run of one label within one row.  Runs of the label of the workgroup's
// first pixel are gathered in LDS first and flushed once per workgroup: the atomics of a component of 10^8 pixels would otherwise
// queue up at the same seven words (a same-address atomic takes some 25 ns there).
template <typename T>
__global__ __launch_bounds__(CCL_NT) void ccl_table_kernel(const T* __restrict__ cls, const int32_t* __restrict__ label, int64_t H, int64_t W, int64_t K,
                                                           long long* t) {
    __shared__ int s_count, s_rlo, s_rhi, s_clo, s_chi, s_first;
    const int64_t n = H * W;
    const int64_t b0 = (int64_t)blockIdx.x * CCL_NT * CCL_RUN;   // (the grid covers n: b0 < n)
    const int64_t p0 = b0 + (int64_t)threadIdx.x * CCL_RUN;
    const int64_t p1 = p0 + CCL_RUN < n ? p0 + CCL_RUN : n;
    const int32_t Lb = label[b0];
    if (threadIdx.x == 0) {
        s_count = 0;
        s_rlo = s_clo = s_first = INT_MAX;
        s_rhi = s_chi = -1;
    }
    __syncthreads();
    if (p0 < n) {
        int64_t start = p0;
        int32_t L = label[p0];
        for (int64_t p = p0 + 1; p <= p1; ++p) {
            const bool end = p == p1 || label[p] != L || p % W == 0;
            if (!end) continue;
            const int64_t r = start / W, c_lo = start - r * W, c_hi = p - 1 - r * W;
            if (L == Lb) {
                atomicAdd(&s_count, (int)(p - start));
                atomicMin(&s_rlo, (int)r);
                atomicMax(&s_rhi, (int)r);
                atomicMin(&s_clo, (int)c_lo);
                atomicMax(&s_chi, (int)c_hi);
                atomicMin(&s_first, (int)start);
            } else {
                ccl_table_flush(t, K, L, cls, p - start, r, r, c_lo, c_hi, start);
            }
            if (p < p1) {
                start = p;
                L = label[p];
            }
        }
    }
    __syncthreads();
    if (threadIdx.x == 0 && s_count > 0) ccl_table_flush(t, K, Lb, cls, s_count, s_rlo, s_rhi, s_clo, s_chi, s_first);
}

// ---- edges --------------------------------------------------------------------------------------------------------------------------
// sides 0 top, 1 left, 2 bottom, 3 right; an edge runs with its pixel on the left: top west, left south, bottom east, right north
__device__ __forceinline__ int ccl_dr(int side) { return side == 1 ? 1 : (side == 3 ? -1 : 0); }
__device__ __forceinline__ int ccl_dc(int side) { return side == 0 ? -1 : (side == 2 ? 1 : 0); }
__device__ __forceinline__ int ccl_nr(int side) { return side == 0 ? -1 : (side == 2 ? 1 : 0); }   // towards the pixel across the edge
__device__ __forceinline__ int ccl_nc(int side) { return side == 1 ? -1 : (side == 3 ? 1 : 0); }

__device__ __forceinline__ bool ccl_member(const int32_t* __restrict__ lab, int64_t H, int64_t W, int64_t r, int64_t c, int32_t L) {
    return r >= 0 && r < H && c >= 0 && c < W && lab[r * W + c] == L;
}
// what follows the edge on `side` of pixel (r, c) of component L: -1 no edge there; 0 straight on (the same side of the pixel ahead);
// 1 a left turn (the next side of this pixel); 2 a right turn (the previous side of the pixel ahead on the far side of the edge: taken
// whenever that pixel is a member, so at a pinch vertex the ring keeps hugging the non-member pixel on its right)
__device__ __forceinline__ int ccl_edge_turn(const int32_t* __restrict__ lab, int64_t H, int64_t W, int64_t r, int64_t c, int side, int32_t L) {
    const int dr = ccl_dr(side), dc = ccl_dc(side), nr = ccl_nr(side), nc = ccl_nc(side);
    if (ccl_member(lab, H, W, r + nr, c + nc, L)) return -1;
    if (ccl_member(lab, H, W, r + nr + dr, c + nc + dc, L)) return 2;
    return ccl_member(lab, H, W, r + dr, c + dc, L) ? 0 : 1;
}

struct CclCorners {   // the corner edges of a label plane, in edge-number order
    const int32_t* lab;
    int64_t H, W;
    int64_t* cedge;
    __device__ int count(int64_t p) const {
        const int32_t L = lab[p];
        if (!L) return 0;
        const int64_t r = p / W, c = p - r * W;
        int n = 0;
        for (int side = 0; side < 4; ++side) n += ccl_edge_turn(lab, H, W, r, c, side, L) > 0;
        return n;
    }
    __device__ void emit(int64_t p, u64 at) const {
        const int32_t L = lab[p];
        const int64_t r = p / W, c = p - r * W;
        for (int side = 0; side < 4; ++side)
            if (ccl_edge_turn(lab, H, W, r, c, side, L) > 0) cedge[at++] = 4 * p + side;
    }
};

// next[k] = the list index of the corner that follows corner k on its ring
__global__ __launch_bounds__(CCL_NT) void ccl_walk_kernel(const int32_t* __restrict__ lab, int64_t H, int64_t W, const int64_t* __restrict__ cedge, int64_t E,
                                                          int32_t* __restrict__ next) {
    const int64_t k = (int64_t)blockIdx.x * CCL_NT + threadIdx.x;
    if (k >= E) return;
    const int64_t e = cedge[k], p = e >> 2;
    int side = (int)(e & 3);
    int64_t r = p / W, c = p - r * W;
    const int32_t L = lab[p];
    if (ccl_edge_turn(lab, H, W, r, c, side, L) == 1) {
        side = (side + 1) & 3;
    } else {
        r += ccl_nr(side) + ccl_dr(side);
        c += ccl_nc(side) + ccl_dc(side);
        side = (side + 3) & 3;
    }
    const int dr = ccl_dr(side), dc = ccl_dc(side);
    while (ccl_edge_turn(lab, H, W, r, c, side, L) == 0) {   // (a straight run ends inside the raster: at most max(H, W) steps)
        r += dr;
        c += dc;
    }
    const int64_t target = 4 * (r * W + c) + side;
    int64_t lo = 0, hi = E - 1;   // (target is a corner edge: it is in the list)
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (cedge[mid] < target) lo = mid + 1;
        else hi = mid;
    }
    next[k] = (int32_t)lo;
}

// ---- pointer jumping over the corners -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(CCL_NT) void ccl_min_first_kernel(const int32_t* __restrict__ next, int32_t* __restrict__ m, int32_t* __restrict__ nx, int64_t E) {
    const int64_t k = (int64_t)blockIdx.x * CCL_NT + threadIdx.x;
    if (k >= E) return;
    const int32_t j = next[k];
    m[k] = j < (int32_t)k ? j : (int32_t)k;
    nx[k] = next[j];
}
__global__ __launch_bounds__(CCL_NT) void ccl_min_round_kernel(const int32_t* __restrict__ m_in, const int32_t* __restrict__ nx_in, int32_t* __restrict__ m_out,
                                                               int32_t* __restrict__ nx_out, int64_t E) {
    const int64_t k = (int64_t)blockIdx.x * CCL_NT + threadIdx.x;
    if (k >= E) return;
    const int32_t j = nx_in[k], a = m_in[k], b = m_in[j];
    m_out[k] = b < a ? b : a;
    nx_out[k] = nx_in[j];
}
// the cycle cut at its leader: the leader points to itself with weight 0, every other corner to its successor with weight 1
__global__ __launch_bounds__(CCL_NT) void ccl_rank_first_kernel(const int32_t* __restrict__ next, const int32_t* __restrict__ lead, int32_t* __restrict__ w,
                                                                int32_t* __restrict__ nx, int64_t E) {
    const int64_t k = (int64_t)blockIdx.x * CCL_NT + threadIdx.x;
    if (k >= E) return;
    const bool is_lead = lead[k] == (int32_t)k;
    w[k] = is_lead ? 0 : 1;
    nx[k] = is_lead ? (int32_t)k : next[k];
}
__global__ __launch_bounds__(CCL_NT) void ccl_rank_round_kernel(const int32_t* __restrict__ w_in, const int32_t* __restrict__ nx_in, int32_t* __restrict__ w_out,
                                                                int32_t* __restrict__ nx_out, int64_t E) {
    const int64_t k = (int64_t)blockIdx.x * CCL_NT + threadIdx.x;
    if (k >= E) return;
    const int32_t j = nx_in[k];
    w_out[k] = w_in[k] + w_in[j];
    nx_out[k] = nx_in[j];
}

struct CclLeaders {   // the leaders of the rings; leader number k (from 0) stores k in `ring`
    const int32_t* lead;
    int32_t* ring;
    __device__ int count(int64_t i) const { return lead[i] == (int32_t)i; }
    __device__ void emit(int64_t i, u64 at) const { ring[i] = (int32_t)at; }
};

__device__ __forceinline__ void ccl_vertex(int64_t e, int64_t W, int64_t* i, int64_t* j) {   // the end vertex of an edge
    const int64_t p = e >> 2, r = p / W, c = p - r * W;
    const int side = (int)(e & 3);
    *i = r + (side == 1 || side == 2);
    *j = c + (side >= 2);
}

struct CclRing {
    int32_t label, lead, len, pad;
    long long area2;   // twice the signed area in map orientation (x = j, y = -i)
};

__global__ __launch_bounds__(CCL_NT) void ccl_ring_kernel(const int32_t* __restrict__ lab, int64_t W, const int64_t* __restrict__ cedge, const int32_t* __restrict__ next,
                                                          const int32_t* __restrict__ lead, const int32_t* __restrict__ dist, const int32_t* __restrict__ ring,
                                                          int64_t E, CclRing* rings) {
    const int64_t k = (int64_t)blockIdx.x * CCL_NT + threadIdx.x;
    if (k >= E) return;
    const int32_t l = lead[k], nk = next[k];
    CclRing* R = rings + ring[l];
    int64_t i0, j0, i1, j1;
    ccl_vertex(cedge[k], W, &i0, &j0);
    ccl_vertex(cedge[nk], W, &i1, &j1);
    atomicAdd(reinterpret_cast<u64*>(&R->area2), (u64)(j1 * i0 - j0 * i1));   // x0 y1 - x1 y0 (two's complement: exact in any order)
    if (l == (int32_t)k) {
        R->label = lab[cedge[k] >> 2];
        R->lead = (int32_t)k;
        R->len = dist[nk] + 1;
    }
}

__global__ __launch_bounds__(CCL_NT) void ccl_gather_kernel(int64_t W, const int64_t* __restrict__ cedge, const int32_t* __restrict__ lead,
                                                            const int32_t* __restrict__ dist, const int32_t* __restrict__ ring, const CclRing* __restrict__ rings,
                                                            const int64_t* __restrict__ base, int64_t E, double a, double c0, double e, double f,
                                                            double* __restrict__ xy) {
    const int64_t k = (int64_t)blockIdx.x * CCL_NT + threadIdx.x;
    if (k >= E) return;
    const int32_t l = lead[k], rg = ring[l];
    const int64_t pos = l == (int32_t)k ? 0 : (int64_t)rings[rg].len - dist[k];
    const int64_t at = base[rg] + pos;
    int64_t i, j;
    ccl_vertex(cedge[k], W, &i, &j);
    const double tx = a * (double)j, ty = e * (double)i;
    xy[at] = c0 + tx;
    xy[E + at] = f + ty;
}

struct CclEvents {
    static constexpr int N = 8;
    hipEvent_t ev[N] = {};
    bool ok = true;
    CclEvents() {
        for (auto& e : ev)
            if (hipEventCreate(&e) != hipSuccess) { e = nullptr; ok = false; (void)hipGetLastError(); }
    }
    ~CclEvents() {
        for (auto& e : ev)
            if (e) (void)hipEventDestroy(e);
    }
    void mark(int k, hipStream_t s) { if (ok) (void)hipEventRecord(ev[k], s); }
    void collect(float* ms, int n) {   // (after the stream was waited for)
        for (int k = 0; k < n; ++k) {
            ms[k] = 0.f;
            if (ok && hipEventElapsedTime(&ms[k], ev[k], ev[k + 1]) != hipSuccess) { (void)hipGetLastError(); ms[k] = 0.f; }
        }
    }
};

inline unsigned ccl_blocks(int64_t n, int per) { return (unsigned)((n + per - 1) / per); }

int ccl_fetch(xdemhip_ctx* ctx, void* dst, const void* src, size_t bytes) {
    XD_HIP_CHECK(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream));
    XD_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return XDEMHIP_OK;
}

// count, scan and place: `cnt` holds a word per chunk and one more for the total
template <typename F>
int ccl_scan_emit(xdemhip_ctx* ctx, const F& f, int64_t n, u64* cnt, bool emit_now) {
    const int64_t chunks = (n + CCL_CHUNK - 1) / CCL_CHUNK;
    CCL_LAUNCH(ctx, ccl_count_kernel<F>, dim3((unsigned)chunks), dim3(CCL_NT), 0, ctx->stream, f, n, cnt);
    CCL_LAUNCH(ctx, xd::rank_scan_kernel, dim3(1), dim3(1024), 0, ctx->stream, cnt, chunks, cnt + chunks);
    if (emit_now) CCL_LAUNCH(ctx, ccl_emit_kernel<F>, dim3((unsigned)chunks), dim3(CCL_NT), 0, ctx->stream, f, n, (const u64*)cnt);
    return launched(ctx, "ccl counting scan");
}

template <typename T>
int ccl_table(xdemhip_ctx* ctx, const T* d_cls, const int32_t* d_lab, int64_t H, int64_t W, int64_t K, long long* d_table) {
    if (K < 1) return XDEMHIP_OK;
    CCL_LAUNCH(ctx, ccl_table_init_kernel, dim3(ccl_blocks(K, CCL_NT)), dim3(CCL_NT), 0, ctx->stream, d_table, K);
    CCL_LAUNCH(ctx, ccl_table_kernel<T>, dim3(ccl_blocks(H * W, CCL_NT * CCL_RUN)), dim3(CCL_NT), 0, ctx->stream, d_cls, d_lab, H, W, K, d_table);
    return launched(ctx, "ccl table kernels");
}

template <typename T>
int ccl_label(xdemhip_ctx* ctx, const T* classes, int64_t H, int64_t W, int conn, int32_t* labels, int64_t* table, int64_t capacity, int memspace,
              int64_t* K_out) {
    const int64_t n = H * W;
    const CclPlan plan = ccl_plan(H, W, ctx->ccl_route);
    const int64_t chunks = (n + CCL_CHUNK - 1) / CCL_CHUNK;
    CclEvents events;
    XdBuffers buf(ctx, "xdemhip_label");
    const T* d_cls = buf.input(classes, (size_t)n * sizeof(T), memspace);
    int32_t* d_lab = buf.output(labels, (size_t)n * sizeof(int32_t), memspace);
    int32_t* d_parent = buf.alloc<int32_t>((size_t)n);
    u64* d_cnt = buf.alloc<u64>((size_t)chunks + 1);
    if (buf.rc) return buf.rc;
    ctx->ccl_launches = 0;
    XD_HIP_CHECK(ctx, hipEventRecord(ctx->ev_start, ctx->stream));
    events.mark(0, ctx->stream);
    CCL_LAUNCH(ctx, ccl_tile_kernel<T>, dim3((unsigned)(plan.tiles_r * plan.tiles_c)), dim3(CCL_NT), (size_t)plan.lds_bytes, ctx->stream, d_cls, d_parent, H, W,
               plan.tr, plan.tc, plan.tiles_c, conn);
    events.mark(1, ctx->stream);
    const int64_t n_hb = (plan.tiles_r - 1) * W, n_items = n_hb + (plan.tiles_c - 1) * H;
    if (n_items > 0)
        CCL_LAUNCH(ctx, ccl_border_kernel<T>, dim3(ccl_blocks(n_items, CCL_NT)), dim3(CCL_NT), 0, ctx->stream, d_cls, d_parent, H, W, plan.tr, plan.tc, n_hb,
                   n_items, conn);
    events.mark(2, ctx->stream);
    CCL_LAUNCH(ctx, ccl_flatten_kernel, dim3(ccl_blocks(n, CCL_NT)), dim3(CCL_NT), 0, ctx->stream, d_parent, d_lab, n);
    events.mark(3, ctx->stream);
    int rc = ccl_scan_emit(ctx, CclRoots{d_lab, d_parent}, n, d_cnt, true);
    if (rc) return rc;
    CCL_LAUNCH(ctx, ccl_relabel_kernel, dim3(ccl_blocks(n, CCL_NT)), dim3(CCL_NT), 0, ctx->stream, d_lab, (const int32_t*)d_parent, n);
    if ((rc = launched(ctx, "ccl label kernels")) != XDEMHIP_OK) return rc;
    events.mark(4, ctx->stream);
    u64 total = 0;
    if ((rc = ccl_fetch(ctx, &total, d_cnt + chunks, sizeof total)) != XDEMHIP_OK) return rc;
    const int64_t K = (int64_t)total;
    *K_out = K;
    bool short_table = false;
    if (table && K > 0) {
        if (capacity < K) short_table = true;
        else {
            long long* d_table = reinterpret_cast<long long*>(buf.output(table, (size_t)K * CCL_T_COLS * sizeof(int64_t), memspace));
            if (buf.rc) return buf.rc;
            if ((rc = ccl_table<T>(ctx, d_cls, d_lab, H, W, K, d_table)) != XDEMHIP_OK) return rc;
        }
    }
    events.mark(5, ctx->stream);
    (void)hipEventRecord(ctx->ev_stop, ctx->stream);
    ctx->timed = true;
    rc = buf.finish();
    if (rc == XDEMHIP_OK) rc = xd_sync(ctx);   // (device planes: the scope may have owned nothing that made it wait)
    if (rc != XDEMHIP_OK) return rc;
    events.collect(ctx->ccl_stage_ms, 5);
    ctx->ccl_stage_launches[0] = ctx->ccl_launches;
    if (short_table) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_label: capacity below the number of components (the labels and K are written)");
    return XDEMHIP_OK;
}

size_t ccl_class_size(int dtype) { return dtype == XDEMHIP_U8 ? 1 : (dtype == XDEMHIP_I32 ? 4 : 0); }

int ccl_check_plane(xdemhip_ctx* ctx, const char* who, int64_t H, int64_t W, int memspace) {
    if (H < 1 || W < 1 || H >= ((int64_t)1 << 31) || W >= ((int64_t)1 << 31) || H * W >= ((int64_t)1 << 31))
        return xd_fail(ctx, XDEMHIP_EINVAL, std::string(who) + ": H and W must be >= 1 and H * W below 2^31");
    if (memspace != XDEMHIP_HOST && memspace != XDEMHIP_DEVICE) return xd_fail(ctx, XDEMHIP_EINVAL, "memspace must be XDEMHIP_HOST or XDEMHIP_DEVICE");
    return XDEMHIP_OK;
}

int ccl_rounds(int64_t H, int64_t W) {   // 2^rounds >= 4 H W, a bound on the corners of one ring
    int r = 0;
    while (((int64_t)1 << r) < 4 * H * W) ++r;
    return r;
}

}  // namespace

extern "C" {

int xdemhip_label_plan(int64_t H, int64_t W, int route_switch, int* tile_rows, int* tile_cols, int64_t* tiles_r, int64_t* tiles_c, int* lds_bytes,
                       int* lds_budget) {
    if (H < 1 || W < 1 || H >= ((int64_t)1 << 31) || W >= ((int64_t)1 << 31) || H * W >= ((int64_t)1 << 31)) return XDEMHIP_EINVAL;
    if (route_switch != 0 && route_switch != 2) return XDEMHIP_EINVAL;
    const CclPlan p = ccl_plan(H, W, route_switch);
    if (tile_rows) *tile_rows = p.tr;
    if (tile_cols) *tile_cols = p.tc;
    if (tiles_r) *tiles_r = p.tiles_r;
    if (tiles_c) *tiles_c = p.tiles_c;
    if (lds_bytes) *lds_bytes = p.lds_bytes;
    if (lds_budget) *lds_budget = CCL_LDS_BUDGET;
    return XDEMHIP_OK;
}

int xdemhip_ccl_stage_ms(xdemhip_ctx* ctx, float* ms, int64_t* launches) {
    if (!ctx || !ms) return XDEMHIP_EINVAL;
    for (int k = 0; k < 11; ++k) ms[k] = ctx->ccl_stage_ms[k];
    if (launches) {
        launches[0] = ctx->ccl_stage_launches[0];
        launches[1] = ctx->ccl_stage_launches[1];
    }
    return XDEMHIP_OK;
}

int xdemhip_label(xdemhip_ctx* ctx, const void* classes, int dtype, int64_t H, int64_t W, int connectivity, int32_t* labels, int64_t* table,
                  int64_t capacity, int memspace, int64_t* K) {
    if (!ctx) return XDEMHIP_EINVAL;
    if (!classes || !labels || !K) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_label: null argument");
    if (connectivity != 4 && connectivity != 8) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_label: connectivity must be 4 or 8");
    if (!ccl_class_size(dtype)) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_label: dtype must be XDEMHIP_U8 or XDEMHIP_I32");
    int rc = ccl_check_plane(ctx, "xdemhip_label", H, W, memspace);
    if (rc) return rc;
    if (table && capacity < 0) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_label: capacity < 0");
    XD_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    return dtype == XDEMHIP_U8 ? ccl_label<unsigned char>(ctx, static_cast<const unsigned char*>(classes), H, W, connectivity, labels, table, capacity, memspace, K)
                               : ccl_label<int32_t>(ctx, static_cast<const int32_t*>(classes), H, W, connectivity, labels, table, capacity, memspace, K);
}

int xdemhip_label_table(xdemhip_ctx* ctx, const void* classes, int dtype, const int32_t* labels, int64_t H, int64_t W, int64_t K, int64_t* table,
                        int memspace) {
    if (!ctx) return XDEMHIP_EINVAL;
    if (!classes || !labels || (K > 0 && !table)) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_label_table: null argument");
    const size_t size = ccl_class_size(dtype);
    if (!size) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_label_table: dtype must be XDEMHIP_U8 or XDEMHIP_I32");
    int rc = ccl_check_plane(ctx, "xdemhip_label_table", H, W, memspace);
    if (rc) return rc;
    if (K < 0 || K > H * W) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_label_table: K must be 0 .. H * W");
    if (K == 0) return XDEMHIP_OK;
    XD_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    const size_t n = (size_t)H * (size_t)W;
    CclEvents events;
    XdBuffers buf(ctx, "xdemhip_label_table");
    const unsigned char* d_cls = buf.input(static_cast<const unsigned char*>(classes), n * size, memspace);
    const int32_t* d_lab = buf.input(labels, n * sizeof(int32_t), memspace);
    long long* d_table = reinterpret_cast<long long*>(buf.output(table, (size_t)K * CCL_T_COLS * sizeof(int64_t), memspace));
    if (buf.rc) return buf.rc;
    events.mark(0, ctx->stream);
    rc = dtype == XDEMHIP_U8 ? ccl_table<unsigned char>(ctx, d_cls, d_lab, H, W, K, d_table)
                             : ccl_table<int32_t>(ctx, reinterpret_cast<const int32_t*>(d_cls), d_lab, H, W, K, d_table);
    events.mark(1, ctx->stream);
    if (rc == XDEMHIP_OK) rc = buf.finish();
    if (rc == XDEMHIP_OK) rc = xd_sync(ctx);
    if (rc == XDEMHIP_OK) events.collect(ctx->ccl_stage_ms + 4, 1);
    return rc;
}

int xdemhip_outlines(xdemhip_ctx* ctx, const int32_t* labels, int64_t H, int64_t W, int64_t K, const double* transform6, double* xy, int64_t v_capacity,
                     int64_t* ring_off, int32_t* poly_of_ring, int64_t* ring_area, int64_t r_capacity, int memspace, int64_t* V, int64_t* R) {
    if (!ctx) return XDEMHIP_EINVAL;
    if (!labels || !transform6 || !V || !R) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_outlines: null argument");
    int rc = ccl_check_plane(ctx, "xdemhip_outlines", H, W, memspace);
    if (rc) return rc;
    if (!(transform6[1] == 0.0 && transform6[3] == 0.0 && transform6[0] > 0.0 && transform6[4] < 0.0))
        return xd_fail(ctx, XDEMHIP_EINVAL, "only north-up transforms (b = d = 0) are supported");
    for (int k = 0; k < 6; ++k)
        if (!std::isfinite(transform6[k])) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_outlines: the transform must be finite");
    if (K < 0 || K > H * W) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_outlines: K must be 0 .. H * W");
    const bool count_only = !xy && !ring_off && !poly_of_ring;
    if (!count_only && (!xy || !ring_off || !poly_of_ring)) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_outlines: xy, ring_off and poly_of_ring together, or none of them");
    if (!count_only && (v_capacity < 0 || r_capacity < 0)) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_outlines: capacity < 0");
    XD_HIP_CHECK(ctx, hipSetDevice(ctx->device));

    const int64_t n = H * W, chunks = (n + CCL_CHUNK - 1) / CCL_CHUNK;
    std::vector<CclRing> rings;          // (copies' destinations and sources: declared before the scope)
    std::vector<int64_t> base, off, area;
    std::vector<int32_t> owner;
    CclEvents events;
    XdBuffers buf(ctx, "xdemhip_outlines");
    const int32_t* d_lab = buf.input(labels, (size_t)n * sizeof(int32_t), memspace);
    u64* d_cnt = buf.alloc<u64>((size_t)chunks + 1);
    if (buf.rc) return buf.rc;
    ctx->ccl_launches = 0;
    XD_HIP_CHECK(ctx, hipEventRecord(ctx->ev_start, ctx->stream));
    events.mark(0, ctx->stream);
    CclCorners corners{d_lab, H, W, nullptr};
    if ((rc = ccl_scan_emit(ctx, corners, n, d_cnt, false)) != XDEMHIP_OK) return rc;
    u64 total = 0;
    if ((rc = ccl_fetch(ctx, &total, d_cnt + chunks, sizeof total)) != XDEMHIP_OK) return rc;
    if (total >= ((u64)1 << 31)) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_outlines: 2^31 corner vertices or more");
    const int64_t E = (int64_t)total;
    *V = E;
    *R = E / 4;   // (the counting call: a bound, every ring has at least four corners)
    if (count_only) return buf.finish();
    if (v_capacity < E || r_capacity < E / 4) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_outlines: capacity below the number of vertices, or r_capacity below V / 4");
    const int rounds = ccl_rounds(H, W);
    if (E == 0) {   // no component: nothing but the first ring offset
        *R = 0;
        const int64_t zero = 0;
        if (memspace == XDEMHIP_HOST) ring_off[0] = 0;
        else XD_HIP_CHECK(ctx, hipMemcpyAsync(ring_off, &zero, sizeof zero, hipMemcpyHostToDevice, ctx->stream));
        XD_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
        for (int k = 0; k < 6; ++k) ctx->ccl_stage_ms[5 + k] = 0.f;
        ctx->ccl_stage_launches[1] = ctx->ccl_launches;
        return buf.finish();
    }
    int64_t* d_cedge = buf.alloc<int64_t>((size_t)E);
    int32_t* d_next = buf.alloc<int32_t>((size_t)E);
    int32_t* d_lead = buf.alloc<int32_t>((size_t)E);
    int32_t* d_p[4];
    for (auto& p : d_p) p = buf.alloc<int32_t>((size_t)E);
    const int64_t echunks = (E + CCL_CHUNK - 1) / CCL_CHUNK;
    u64* d_ecnt = buf.alloc<u64>((size_t)echunks + 1);
    double* d_xy = buf.output(xy, (size_t)E * 2 * sizeof(double), memspace);
    if (buf.rc) return buf.rc;
    corners.cedge = d_cedge;
    const dim3 egrid(ccl_blocks(E, CCL_NT)), block(CCL_NT);
    CCL_LAUNCH(ctx, ccl_emit_kernel<CclCorners>, dim3((unsigned)chunks), block, 0, ctx->stream, corners, n, (const u64*)d_cnt);
    events.mark(1, ctx->stream);
    CCL_LAUNCH(ctx, ccl_walk_kernel, egrid, block, 0, ctx->stream, d_lab, H, W, (const int64_t*)d_cedge, E, d_next);
    events.mark(2, ctx->stream);
    // leader: after round r, m[k] is the smallest index among corner k and its 2^r - 1 successors
    CCL_LAUNCH(ctx, ccl_min_first_kernel, egrid, block, 0, ctx->stream, (const int32_t*)d_next, d_p[0], d_p[1], E);
    int cur = 0;
    for (int r = 1; r < rounds; ++r, cur ^= 2)
        CCL_LAUNCH(ctx, ccl_min_round_kernel, egrid, block, 0, ctx->stream, (const int32_t*)d_p[cur], (const int32_t*)d_p[cur + 1], d_p[cur ^ 2], d_p[(cur ^ 2) + 1], E);
    XD_HIP_CHECK(ctx, hipMemcpyAsync(d_lead, d_p[cur], (size_t)E * sizeof(int32_t), hipMemcpyDeviceToDevice, ctx->stream));
    events.mark(3, ctx->stream);
    // rank: after round r, w[k] is the distance from corner k to the leader, or 2^r where that is nearer
    CCL_LAUNCH(ctx, ccl_rank_first_kernel, egrid, block, 0, ctx->stream, (const int32_t*)d_next, (const int32_t*)d_lead, d_p[0], d_p[1], E);
    cur = 0;
    for (int r = 0; r < rounds; ++r, cur ^= 2)
        CCL_LAUNCH(ctx, ccl_rank_round_kernel, egrid, block, 0, ctx->stream, (const int32_t*)d_p[cur], (const int32_t*)d_p[cur + 1], d_p[cur ^ 2], d_p[(cur ^ 2) + 1], E);
    const int32_t* d_dist = d_p[cur];
    int32_t* d_ring = d_p[cur ^ 2];   // (the other pair is free again)
    events.mark(4, ctx->stream);
    if ((rc = launched(ctx, "ccl tracing kernels")) != XDEMHIP_OK) return rc;
    if ((rc = ccl_scan_emit(ctx, CclLeaders{d_lead, d_ring}, E, d_ecnt, true)) != XDEMHIP_OK) return rc;
    if ((rc = ccl_fetch(ctx, &total, d_ecnt + echunks, sizeof total)) != XDEMHIP_OK) return rc;
    const int64_t NR = (int64_t)total;
    if (NR < 1 || NR > E / 4) return xd_fail(ctx, XDEMHIP_EHIP, "xdemhip_outlines: ring count out of range (internal)");
    CclRing* d_rings = buf.alloc<CclRing>((size_t)NR);
    int64_t* d_base = buf.alloc<int64_t>((size_t)NR);
    if (buf.rc) return buf.rc;
    XD_HIP_CHECK(ctx, hipMemsetAsync(d_rings, 0, (size_t)NR * sizeof(CclRing), ctx->stream));
    CCL_LAUNCH(ctx, ccl_ring_kernel, egrid, block, 0, ctx->stream, d_lab, W, (const int64_t*)d_cedge, (const int32_t*)d_next, (const int32_t*)d_lead, d_dist,
               (const int32_t*)d_ring, E, d_rings);
    if ((rc = launched(ctx, "ccl ring kernel")) != XDEMHIP_OK) return rc;
    rings.resize((size_t)NR);
    if ((rc = ccl_fetch(ctx, rings.data(), d_rings, (size_t)NR * sizeof(CclRing))) != XDEMHIP_OK) return rc;
    // components in label order, the rings of a component in leader order (the order they are listed in): a stable counting sort
    std::vector<int64_t> first((size_t)K + 1, 0);
    int64_t sum_len = 0;
    for (const CclRing& g : rings) {
        if (g.label < 1 || g.label > K) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_outlines: a label outside 1 .. K");
        ++first[(size_t)g.label];
        sum_len += g.len;
    }
    if (sum_len != E) return xd_fail(ctx, XDEMHIP_EHIP, "xdemhip_outlines: ring lengths do not add up (internal)");
    for (int64_t l = 1, run = 0; l <= K; ++l) {
        const int64_t c = first[(size_t)l];
        first[(size_t)l] = run;
        run += c;
    }
    std::vector<int64_t> slot((size_t)NR);
    for (int64_t q = 0; q < NR; ++q) slot[(size_t)first[(size_t)rings[(size_t)q].label]++] = q;
    base.assign((size_t)NR, 0);
    off.assign((size_t)NR + 1, 0);
    owner.assign((size_t)NR, 0);
    area.assign((size_t)NR, 0);
    for (int64_t s = 0; s < NR; ++s) {
        const CclRing& g = rings[(size_t)slot[(size_t)s]];
        base[(size_t)slot[(size_t)s]] = off[(size_t)s];
        off[(size_t)s + 1] = off[(size_t)s] + g.len;
        owner[(size_t)s] = g.label - 1;
        area[(size_t)s] = (int64_t)(g.area2 / 2);
    }
    XD_HIP_CHECK(ctx, hipMemcpyAsync(d_base, base.data(), (size_t)NR * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream));
    if (memspace == XDEMHIP_HOST) {
        memcpy(ring_off, off.data(), ((size_t)NR + 1) * sizeof(int64_t));
        memcpy(poly_of_ring, owner.data(), (size_t)NR * sizeof(int32_t));
        if (ring_area) memcpy(ring_area, area.data(), (size_t)NR * sizeof(int64_t));
    } else {
        XD_HIP_CHECK(ctx, hipMemcpyAsync(ring_off, off.data(), ((size_t)NR + 1) * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream));
        XD_HIP_CHECK(ctx, hipMemcpyAsync(poly_of_ring, owner.data(), (size_t)NR * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
        if (ring_area) XD_HIP_CHECK(ctx, hipMemcpyAsync(ring_area, area.data(), (size_t)NR * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream));
    }
    events.mark(5, ctx->stream);
    CCL_LAUNCH(ctx, ccl_gather_kernel, egrid, block, 0, ctx->stream, W, (const int64_t*)d_cedge, (const int32_t*)d_lead, d_dist, (const int32_t*)d_ring,
               (const CclRing*)d_rings, (const int64_t*)d_base, E, transform6[0], transform6[2], transform6[4], transform6[5], d_xy);
    events.mark(6, ctx->stream);
    (void)hipEventRecord(ctx->ev_stop, ctx->stream);
    ctx->timed = true;
    rc = launched(ctx, "ccl gather kernel");
    if (rc == XDEMHIP_OK) rc = buf.finish();
    if (rc == XDEMHIP_OK) rc = xd_sync(ctx);
    if (rc != XDEMHIP_OK) return rc;
    events.collect(ctx->ccl_stage_ms + 5, 6);
    ctx->ccl_stage_launches[1] = ctx->ccl_launches;
    *R = NR;
    return XDEMHIP_OK;
}

}  // extern "C"
