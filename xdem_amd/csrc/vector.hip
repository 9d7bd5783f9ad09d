// vector.hip -- polygons burnt into a grid (include/xdemhip.h, "polygons burnt into a grid"): what geoutils' Vector.create_mask and
// Vector.rasterize do through GDAL's scanline fill, all_touched=False, in a number of launches that does not depend on the number of
// polygons.  THE RULE is stated in the header; every comparison and every operation of it appears here once, in vec_cy / vec_cx,
// vec_row_below / vec_col_ge and vec_cross_kernel, and the file is built with -ffp-contract=off.
//   1. vec_edge_kernel    per edge (= per vertex: the edge to the ring's next vertex, the last one back to the first): the rows it
//                         crosses, clipped to the grid, as [ra, ra + cnt); per polygon the extent of those rows (integer min / max).
//                         vec_scan: exclusive scan of the counts over the edges -> crossing k belongs to edge upper_bound(k) - 1, so a
//                         long edge is spread over as many lanes as it has crossings
//   2. vec_extent_kernel  per polygon its clipped row extent, scanned: segment id = rowbase[p] + (r - r0[p]), one segment per polygon
//                         and row of its extent.  vec_cross_kernel: per crossing its abscissa and segment, counted per segment;
//                         scan; vec_scatter_kernel: the abscissae into segment-contiguous order (a counting sort)
//   3. vec_sort_small_kernel / vec_sort_big_kernel: every segment ascending -- up to VEC_SEG_REG crossings in one lane's registers,
//                         up to VEC_SEG_LDS by one workgroup in LDS, longer ones in place in global memory (hyp_sort of volume.h).
//                         Equal abscissae are equal values: the scatter's order cannot reach a result
//   4. vec_fill_kernel    per pair (x_2k, x_2k+1) of a segment the columns c with x_2k <= cx(c) and not x_2k+1 <= cx(c): bytes of 1, or
//                         atomicMax(label, ordinal + 1) -- the polygon latest in the table wins, in any order of execution.  A span of
//                         up to VEC_WIDE columns is stored by its lane, a wider one by the whole wave (coalesced)
//   5. vec_finish_kernel  ordinal -> burn value / out_value, and the burnt pixels counted: one partial per workgroup, the reduce
//                         kernel of fixed_sums.h
// Every ring closes, so every row is crossed an even number of times by every ring and segments hold whole pairs; a pair that would
// straddle two segments (possible only with non-finite vertices, which the callers refuse) is skipped.
#include <math.h>
#include <string.h>

#include <string>
#include <vector>

#include "common.h"
#include "select.h"
#include "select_run.h"
#include "rank_select.h"
#include "volume.h"
#include "fixed_sums.h"
#include "../../include/xdemhip_test.h"

namespace xd {
namespace {

typedef unsigned long long u64;

constexpr int VEC_SEG_REG = 8;      // crossings of a segment sorted in one lane's registers
constexpr int VEC_SEG_LDS = 4096;   // crossings of a segment sorted by one workgroup in LDS (32 KiB)
constexpr int VEC_WIDE = 64;        // a span of more columns than this is stored by the whole wave
constexpr int VEC_TILE = 2048;      // elements per workgroup of the scans: 256 lanes x 8

struct VecGrid {
    int64_t H, W;
    double a, c0, e, f;
};

__device__ __forceinline__ double vec_cy(const VecGrid& g, int64_t r) {
    const double t = ((double)r + 0.5) * g.e;
    return g.f + t;
}
__device__ __forceinline__ double vec_cx(const VecGrid& g, int64_t c) {
    const double t = ((double)c + 0.5) * g.a;
    return g.c0 + t;
}
// the smallest r in [0, H] with cy(r) < y (H: none).  cy falls with r: a guess from the division, then the comparison itself decides.
__device__ __forceinline__ int64_t vec_row_below(const VecGrid& g, double y) {
    const double t = (y - g.f) / g.e - 0.5;
    int64_t r = !(t > 0.0) ? 0 : (t >= (double)g.H ? g.H : (int64_t)t);
    while (r > 0 && vec_cy(g, r - 1) < y) --r;
    while (r < g.H && !(vec_cy(g, r) < y)) ++r;
    return r;
}
// the smallest c in [0, W] with x <= cx(c) (W: none)
__device__ __forceinline__ int64_t vec_col_ge(const VecGrid& g, double x) {
    const double t = (x - g.c0) / g.a - 0.5;
    int64_t c = !(t > 0.0) ? 0 : (t >= (double)g.W ? g.W : (int64_t)t);
    while (c > 0 && x <= vec_cx(g, c - 1)) --c;
    while (c < g.W && !(x <= vec_cx(g, c))) ++c;
    return c;
}
// the number of a[0 .. n) that are <= x (a non-decreasing)
__device__ __forceinline__ int64_t vec_count_le(const u64* __restrict__ a, int64_t n, u64 x) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (a[mid] <= x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// ---- exclusive scan of a[0 .. n) in place, a[n] = the total: tile sums, rank_scan_kernel over the tiles, tile scans ---------------------
__global__ __launch_bounds__(256) void vec_tile_sum_kernel(const u64* __restrict__ a, int64_t n, int64_t n_tiles, u64* __restrict__ tile) {
    __shared__ u64 red[4];
    for (int64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const int64_t base = t * VEC_TILE;
        u64 s = 0ull;
        for (int i = threadIdx.x; i < VEC_TILE; i += 256)
            if (base + i < n) s += a[base + i];
        s = block_sum<u64>(s, red);
        if (threadIdx.x == 0) tile[t] = s;
    }
}
__global__ __launch_bounds__(256) void vec_tile_scan_kernel(u64* __restrict__ a, int64_t n, int64_t n_tiles, const u64* __restrict__ tile) {
    __shared__ u64 s[256];
    for (int64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const int64_t base = t * VEC_TILE + (int64_t)threadIdx.x * 8;
        u64 v[8], sum = 0ull;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            v[k] = base + k < n ? a[base + k] : 0ull;
            sum += v[k];
        }
        s[threadIdx.x] = sum;
        __syncthreads();
        for (int off = 1; off < 256; off <<= 1) {
            const u64 b = (int)threadIdx.x >= off ? s[threadIdx.x - off] : 0ull;
            __syncthreads();
            s[threadIdx.x] += b;
            __syncthreads();
        }
        u64 run = tile[t] + s[threadIdx.x] - sum;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            if (base + k < n) a[base + k] = run;
            run += v[k];
        }
        __syncthreads();
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) a[n] = tile[n_tiles];
}

// ---- 1. per edge ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void vec_edge_kernel(const double* __restrict__ xy, int64_t V, const int64_t* __restrict__ ring_off, int64_t R,
                                                       const int32_t* __restrict__ poly_of_ring, int32_t P, VecGrid g, int64_t* __restrict__ enext,
                                                       int32_t* __restrict__ era, int32_t* __restrict__ epoly, u64* __restrict__ ecnt, int32_t* r0, int32_t* r1) {
    for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < V; v += (int64_t)gridDim.x * 256) {
        // the ring of vertex v: the last k in [0, R) with ring_off[k] <= v
        int64_t lo = 0, hi = R;
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (ring_off[mid] <= v) lo = mid + 1;
            else hi = mid;
        }
        const int64_t k = lo - 1;
        int64_t nx = v, ra = 0, cnt = 0;
        int32_t p = -1;
        if (k >= 0) {
            const int64_t b = ring_off[k];
            int64_t e = ring_off[k + 1];
            e = e > V ? V : e;
            p = poly_of_ring[k];
            if (p >= 0 && p < P && b >= 0 && v < e && e - b >= 3) {
                nx = v + 1 < e ? v + 1 : b;
                const double y1 = xy[V + v], y2 = xy[V + nx];
                if (y1 != y2) {
                    const double ylo = y1 < y2 ? y1 : y2, yhi = y1 < y2 ? y2 : y1;
                    ra = vec_row_below(g, yhi);               // the first row with cy < max(y1, y2)
                    const int64_t rb = vec_row_below(g, ylo);  // the first row with cy < min(y1, y2): the rows before it have min <= cy
                    cnt = rb > ra ? rb - ra : 0;
                    if (cnt) {
                        atomicMin(&r0[p], (int32_t)ra);
                        atomicMax(&r1[p], (int32_t)rb);
                    }
                }
            } else {
                p = -1;
            }
        }
        enext[v] = nx;
        era[v] = (int32_t)ra;
        epoly[v] = p;
        ecnt[v] = (u64)cnt;
    }
}

// ---- 2. per polygon its row extent; per crossing its abscissa and segment ---------------------------------------------------------------
__global__ __launch_bounds__(256) void vec_extent_kernel(const int32_t* __restrict__ r0, const int32_t* __restrict__ r1, int32_t P, u64* __restrict__ ext) {
    for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < P; p += (int64_t)gridDim.x * 256) ext[p] = r1[p] > r0[p] ? (u64)(r1[p] - r0[p]) : 0ull;
}

__global__ __launch_bounds__(256) void vec_cross_kernel(const double* __restrict__ xy, int64_t V, const int64_t* __restrict__ enext, const int32_t* __restrict__ era,
                                                        const int32_t* __restrict__ epoly, const u64* __restrict__ eoff, const int32_t* __restrict__ r0,
                                                        const u64* __restrict__ rowbase, VecGrid g, int64_t C, int64_t S, double* __restrict__ tx,
                                                        int64_t* __restrict__ tseg, u64* scnt) {
    for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < C; k += (int64_t)gridDim.x * 256) {
        const int64_t v = vec_count_le(eoff, V, (u64)k) - 1;   // the last edge that starts at or before crossing k: it has crossings
        int64_t seg = -1;
        double x = 0.0;
        if (v >= 0) {
            const int32_t p = epoly[v];
            const int64_t r = (int64_t)era[v] + (k - (int64_t)eoff[v]);
            if (p >= 0 && r >= 0 && r < g.H) {
                const int64_t nx = enext[v];
                const double x1 = xy[v], y1 = xy[V + v], x2 = xy[nx], y2 = xy[V + nx];
                const double cy = vec_cy(g, r);
                const double dy = cy - y1, dx = x2 - x1, den = y2 - y1;
                const double num = dy * dx;
                const double q = num / den;
                x = x1 + q;
                seg = (int64_t)rowbase[p] + (r - (int64_t)r0[p]);
                if (seg < 0 || seg >= S) seg = -1;
            }
        }
        tx[k] = x;
        tseg[k] = seg;
        if (seg >= 0) atomicAdd(&scnt[seg], 1ull);
    }
}

__global__ __launch_bounds__(256) void vec_scatter_kernel(const double* __restrict__ tx, const int64_t* __restrict__ tseg, int64_t C, u64* cursor, double* __restrict__ xs) {
    for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < C; k += (int64_t)gridDim.x * 256) {
        const int64_t seg = tseg[k];
        if (seg < 0) continue;
        const u64 at = atomicAdd(&cursor[seg], 1ull);
        if (at < (u64)C) xs[at] = tx[k];
    }
}

// ---- 3. every segment ascending ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void vec_sort_small_kernel(double* __restrict__ xs, const u64* __restrict__ soff, int64_t S, int reg_cap) {
    for (int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x; s < S; s += (int64_t)gridDim.x * 256) {
        const int64_t b = (int64_t)soff[s], len = (int64_t)soff[s + 1] - b;
        if (len < 2 || len > reg_cap) continue;
        double a[VEC_SEG_REG];
#pragma unroll
        for (int i = 0; i < VEC_SEG_REG; ++i) a[i] = i < len ? xs[b + i] : (double)INFINITY;
        // odd-even transposition over 8 places: 8 rounds (the places beyond len hold +infinity and stay)
#pragma unroll
        for (int round = 0; round < VEC_SEG_REG; ++round) {
#pragma unroll
            for (int i = round & 1; i + 1 < VEC_SEG_REG; i += 2) {
                const double lo = a[i + 1] < a[i] ? a[i + 1] : a[i], hi = a[i + 1] < a[i] ? a[i] : a[i + 1];
                a[i] = lo;
                a[i + 1] = hi;
            }
        }
#pragma unroll
        for (int i = 0; i < VEC_SEG_REG; ++i)
            if (i < len) xs[b + i] = a[i];
    }
}

__global__ __launch_bounds__(256) void vec_sort_big_kernel(double* xs, const u64* __restrict__ soff, int64_t S, int reg_cap, int lds_cap) {
    __shared__ double s_x[VEC_SEG_LDS];
    for (int64_t s = blockIdx.x; s < S; s += gridDim.x) {
        const int64_t b = (int64_t)soff[s], len = (int64_t)soff[s + 1] - b;   // (the same for every lane: the branches below are uniform)
        if (len <= reg_cap) continue;
        if (len <= lds_cap) {
            for (int64_t i = threadIdx.x; i < len; i += HYP_THREADS) s_x[i] = xs[b + i];
            __syncthreads();
            hyp_sort(s_x, len, [](double x, double y) { return x < y; });
            for (int64_t i = threadIdx.x; i < len; i += HYP_THREADS) xs[b + i] = s_x[i];
            __syncthreads();
        } else {
            __syncthreads();
            hyp_sort(xs + b, len, [](double x, double y) { return x < y; });
        }
    }
}

// ---- 4. spans ---------------------------------------------------------------------------------------------------------------------------
template <int KIND> __device__ __forceinline__ void vec_store(void* plane, int64_t at, int32_t val) {
    if (KIND == 0) static_cast<unsigned char*>(plane)[at] = (unsigned char)1;
    else atomicMax(static_cast<int32_t*>(plane) + at, val);
}

template <int KIND>
__global__ __launch_bounds__(256) void vec_fill_kernel(const double* __restrict__ xs, const u64* __restrict__ soff, int64_t S, const u64* __restrict__ rowbase, int32_t P,
                                                       const int32_t* __restrict__ r0, VecGrid g, int64_t n_pairs, void* plane) {
    const int lane = threadIdx.x & 63;
    const int64_t n_pad = (n_pairs + 63) & ~(int64_t)63;   // whole waves walk the loop: the wave-wide operations see all lanes
    for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < n_pad; j += (int64_t)gridDim.x * 256) {
        int32_t row = 0, ca = 0, cb = 0, val = 0;
        if (j < n_pairs) {
            const u64 pos = (u64)j * 2ull;
            const int64_t s = vec_count_le(soff, S, pos) - 1;   // the last segment that starts at or before pos: it is not empty
            if (s >= 0 && pos + 1ull < soff[s + 1]) {
                const int64_t p = vec_count_le(rowbase, P, (u64)s) - 1;
                if (p >= 0) {
                    const int64_t r = (int64_t)r0[p] + (s - (int64_t)rowbase[p]);
                    if (r >= 0 && r < g.H) {
                        row = (int32_t)r;
                        ca = (int32_t)vec_col_ge(g, xs[pos]);
                        cb = (int32_t)vec_col_ge(g, xs[pos + 1ull]);
                        val = (int32_t)p + 1;
                    }
                }
            }
        }
        const bool wide = cb - ca > VEC_WIDE;
        if (!wide)
            for (int32_t c = ca; c < cb; ++c) vec_store<KIND>(plane, (int64_t)row * g.W + c, val);
        unsigned long long rem = __ballot(wide);
        while (rem) {
            const int src = __ffsll((unsigned long long)rem) - 1;
            const int32_t row_s = __shfl(row, src), ca_s = __shfl(ca, src), cb_s = __shfl(cb, src), val_s = __shfl(val, src);
            for (int32_t c = ca_s + lane; c < cb_s; c += 64) vec_store<KIND>(plane, (int64_t)row_s * g.W + c, val_s);
            rem &= rem - 1ull;
        }
    }
}

// ---- 5. finish --------------------------------------------------------------------------------------------------------------------------
// KIND 0: the bytes are final, counted only.  KIND 1: ordinal + 1 -> burn[ordinal] (null: ordinal + 1), 0 -> out_value, in place.
template <int KIND>
__global__ __launch_bounds__(256) void vec_finish_kernel(void* plane, int64_t n, const int32_t* __restrict__ burn, int32_t out_value, double* __restrict__ part) {
    __shared__ double red[4];
    double cnt = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        if (KIND == 0) {
            if (static_cast<const unsigned char*>(plane)[i]) cnt = cnt + 1.0;
        } else {
            int32_t* q = static_cast<int32_t*>(plane) + i;
            const int32_t v = *q;
            if (v > 0) cnt = cnt + 1.0;
            *q = v > 0 ? (burn ? burn[v - 1] : v) : out_value;
        }
    }
    const double total = block_sum<double>(cnt, red);
    if (threadIdx.x == 0) part[blockIdx.x] = total;
}

struct VecTable {
    const double* xy;
    int64_t V;
    const int64_t* ring_off;
    int64_t R;
    const int32_t* poly_of_ring;
    int32_t P;
};

int vec_check_table(xdemhip_ctx* ctx, const VecTable& t, int memspace, const char* who) {
    if (t.V < 0 || t.R < 0 || t.P < 0) return xd_fail(ctx, XDEMHIP_EINVAL, std::string(who) + ": negative size");
    if (t.V == 0) return XDEMHIP_OK;
    if (!t.xy || !t.ring_off || !t.poly_of_ring || t.R < 1 || t.P < 1) return xd_fail(ctx, XDEMHIP_EINVAL, "null argument");
    if (t.V >= ((int64_t)1 << 40)) return xd_fail(ctx, XDEMHIP_EINVAL, std::string(who) + ": too many vertices");
    if (memspace == XDEMHIP_HOST) {
        if (t.ring_off[0] != 0 || t.ring_off[t.R] != t.V) return xd_fail(ctx, XDEMHIP_EINVAL, std::string(who) + ": ring_off runs from 0 to V");
        for (int64_t r = 0; r < t.R; ++r) {
            if (t.ring_off[r + 1] < t.ring_off[r]) return xd_fail(ctx, XDEMHIP_EINVAL, std::string(who) + ": ring_off must not decrease");
            if (t.poly_of_ring[r] < 0 || t.poly_of_ring[r] >= t.P) return xd_fail(ctx, XDEMHIP_EINVAL, std::string(who) + ": a ring's polygon is an ordinal in [0, P)");
        }
    }
    return XDEMHIP_OK;
}

// test switch "vec_stage_times": an event where each stage starts, the times between them summed per stage once the call has synchronised
struct VecStages {
    xdemhip_ctx* ctx;
    std::vector<hipEvent_t> ev;
    std::vector<int> stage;
    explicit VecStages(xdemhip_ctx* c) : ctx(c) {
        for (float& m : ctx->vec_stage_ms) m = 0.0f;
    }
    void mark(int s) {   // stage s (0 .. 4) starts here; -1: the last stage ends
        if (!ctx->vec_stage_times) return;
        hipEvent_t e;
        if (hipEventCreate(&e) != hipSuccess) return;
        (void)hipEventRecord(e, ctx->stream);
        ev.push_back(e);
        stage.push_back(s);
    }
    void collect() {   // (after the stream has been waited for)
        for (size_t i = 0; i + 1 < ev.size(); ++i) {
            float ms = 0.0f;
            if (stage[i] >= 0 && hipEventElapsedTime(&ms, ev[i], ev[i + 1]) == hipSuccess) ctx->vec_stage_ms[stage[i]] += ms;
        }
    }
    ~VecStages() {
        for (hipEvent_t e : ev) (void)hipEventDestroy(e);
    }
    VecStages(const VecStages&) = delete;
    VecStages& operator=(const VecStages&) = delete;
};

#define VEC_LAUNCH(ctx, ...)              \
    do {                                  \
        hipLaunchKernelGGL(__VA_ARGS__);  \
        ++(ctx)->vec_launches;            \
    } while (0)

// exclusive scan of a[0 .. n) in place with the total in a[n]; tile: n_tiles + 1 words
int vec_scan(xdemhip_ctx* ctx, u64* a, int64_t n, u64* tile) {
    const int64_t n_tiles = (n + VEC_TILE - 1) / VEC_TILE;
    const int g = grid_for(ctx, n_tiles, 1, 8);
    VEC_LAUNCH(ctx, vec_tile_sum_kernel, dim3(g), dim3(256), 0, ctx->stream, a, n, n_tiles, tile);
    VEC_LAUNCH(ctx, rank_scan_kernel, dim3(1), dim3(1024), 0, ctx->stream, tile, n_tiles, tile + n_tiles);
    VEC_LAUNCH(ctx, vec_tile_scan_kernel, dim3(g), dim3(256), 0, ctx->stream, a, n, n_tiles, tile);
    return launched(ctx, "vec_scan");
}

// stages 1 to 4 of one table into `plane` (device; zeroed by the caller)
template <int KIND> int vec_burn(xdemhip_ctx* ctx, const VecTable& t, const VecGrid& g, int memspace, void* plane, VecStages& st) {
    if (t.V == 0) return XDEMHIP_OK;
    const int64_t V = t.V, R = t.R;
    const int32_t P = t.P;
    u64 totals[2] = {0ull, 0ull};   // (a copy's destination: declared before the buffers)
    XdBuffers buf(ctx, "xdemhip_rasterize");
    const double* xy = buf.input(t.xy, (size_t)V * 16, memspace);
    const int64_t* ring_off = buf.input(t.ring_off, (size_t)(R + 1) * 8, memspace);
    const int32_t* por = buf.input(t.poly_of_ring, (size_t)R * 4, memspace);
    int64_t* enext = buf.alloc<int64_t>((size_t)V);
    int32_t* era = buf.alloc<int32_t>((size_t)V);
    int32_t* epoly = buf.alloc<int32_t>((size_t)V);
    u64* eoff = buf.alloc<u64>((size_t)V + 1);
    int32_t* r0 = buf.alloc<int32_t>((size_t)P * 2);
    int32_t* r1 = r0 ? r0 + P : nullptr;
    u64* rowbase = buf.alloc<u64>((size_t)P + 1);
    const int64_t n_max = V > P ? V : P;
    u64* tile = buf.alloc<u64>((size_t)((n_max + VEC_TILE - 1) / VEC_TILE) + 2);
    if (buf.rc) return buf.rc;
    if (hipMemsetAsync(r0, 0x7f, (size_t)P * 4, ctx->stream) != hipSuccess || hipMemsetAsync(r1, 0, (size_t)P * 4, ctx->stream) != hipSuccess)
        return xd_fail(ctx, XDEMHIP_EHIP, "hipMemsetAsync failed");
    st.mark(0);
    VEC_LAUNCH(ctx, vec_edge_kernel, dim3(grid_for(ctx, V, 256, 16)), dim3(256), 0, ctx->stream, xy, V, ring_off, R, por, P, g, enext, era, epoly, eoff, r0, r1);
    int rc = vec_scan(ctx, eoff, V, tile);
    if (rc) return rc;
    st.mark(1);
    VEC_LAUNCH(ctx, vec_extent_kernel, dim3(grid_for(ctx, P, 256, 16)), dim3(256), 0, ctx->stream, r0, r1, P, rowbase);
    rc = vec_scan(ctx, rowbase, P, tile);
    if (rc == XDEMHIP_OK) rc = xd_d2h(ctx, &totals[0], eoff + V, 8);
    if (rc == XDEMHIP_OK) rc = xd_d2h(ctx, &totals[1], rowbase + P, 8);
    if (rc == XDEMHIP_OK) rc = xd_sync(ctx);
    if (rc) return rc;
    const int64_t C = (int64_t)totals[0], S = (int64_t)totals[1];
    if (C < 0 || S < 0 || C >= ((int64_t)1 << 40) || S > (int64_t)P * g.H) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_rasterize: 2^40 crossings or more");
    if (C < 2 || S < 1) {
        st.mark(-1);
        return buf.finish();
    }
    double* tx = buf.alloc<double>((size_t)C);
    int64_t* tseg = buf.alloc<int64_t>((size_t)C);
    double* xs = buf.alloc<double>((size_t)C);
    u64* soff = buf.alloc<u64>((size_t)S + 1);
    u64* cursor = buf.alloc<u64>((size_t)S + 1);
    u64* stile = buf.alloc<u64>((size_t)((S + VEC_TILE - 1) / VEC_TILE) + 2);
    if (buf.rc) return buf.rc;
    if (hipMemsetAsync(soff, 0, ((size_t)S + 1) * 8, ctx->stream) != hipSuccess) return xd_fail(ctx, XDEMHIP_EHIP, "hipMemsetAsync failed");
    const int gc = grid_for(ctx, C, 256, 16);
    VEC_LAUNCH(ctx, vec_cross_kernel, dim3(gc), dim3(256), 0, ctx->stream, xy, V, enext, era, epoly, eoff, r0, rowbase, g, C, S, tx, tseg, soff);
    rc = vec_scan(ctx, soff, S, stile);
    if (rc) return rc;
    if (hipMemcpyAsync(cursor, soff, (size_t)S * 8, hipMemcpyDeviceToDevice, ctx->stream) != hipSuccess) return xd_fail(ctx, XDEMHIP_EHIP, "device copy failed");
    VEC_LAUNCH(ctx, vec_scatter_kernel, dim3(gc), dim3(256), 0, ctx->stream, tx, tseg, C, cursor, xs);
    const int reg_cap = ctx->vec_seg_reg ? ctx->vec_seg_reg : VEC_SEG_REG;
    const int lds_cap = ctx->vec_seg_lds ? ctx->vec_seg_lds : VEC_SEG_LDS;
    st.mark(2);
    VEC_LAUNCH(ctx, vec_sort_small_kernel, dim3(grid_for(ctx, S, 256, 16)), dim3(256), 0, ctx->stream, xs, soff, S, reg_cap);
    VEC_LAUNCH(ctx, vec_sort_big_kernel, dim3(grid_for(ctx, S, 1, 8)), dim3(256), 0, ctx->stream, xs, soff, S, reg_cap, lds_cap);
    const int64_t n_pairs = C >> 1;
    st.mark(3);
    VEC_LAUNCH(ctx, (vec_fill_kernel<KIND>), dim3(grid_for(ctx, n_pairs, 256, 16)), dim3(256), 0, ctx->stream, xs, soff, S, rowbase, P, r0, g, n_pairs, plane);
    st.mark(-1);
    rc = launched(ctx, "vec_fill_kernel");
    if (rc) return rc;
    return buf.finish();
}

int vec_grid(xdemhip_ctx* ctx, int64_t H, int64_t W, const double* t6, VecGrid* g) {
    if (!t6) return xd_fail(ctx, XDEMHIP_EINVAL, "null argument");
    if (H < 1 || W < 1 || H >= ((int64_t)1 << 31) - 1 || W >= ((int64_t)1 << 31) - 1) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_rasterize: H and W are 1 to 2^31 - 2");
    if (!(t6[1] == 0.0 && t6[3] == 0.0 && t6[0] > 0.0 && t6[4] < 0.0)) return xd_fail(ctx, XDEMHIP_EINVAL, "only north-up transforms (b = d = 0) are supported");
    for (int k = 0; k < 6; ++k)
        if (!std::isfinite(t6[k])) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_rasterize: the transform must be finite");
    *g = VecGrid{H, W, t6[0], t6[2], t6[4], t6[5]};
    return XDEMHIP_OK;
}

// the shared body: one or two tables into one plane, then the finish pass
template <int KIND>
int vec_run(xdemhip_ctx* ctx, const VecTable* tabs, int n_tabs, const int32_t* burn, const VecGrid& g, void* out, int32_t out_value, int memspace, int64_t* n_burnt) {
    const int64_t n = g.H * g.W;
    const size_t es = KIND == 0 ? 1 : 4;
    double total = 0.0;   // (a copy's destination: declared before the buffers)
    VecStages st(ctx);
    XdBuffers buf(ctx, "xdemhip_rasterize");
    void* plane = buf.output(out, (size_t)n * es, memspace);
    const int32_t* d_burn = KIND == 1 && burn ? buf.input(burn, (size_t)tabs[0].P * 4, memspace) : nullptr;
    const int nb = fixed_sums_grid(ctx, (n + 255) / 256);
    double* part = buf.alloc<double>((size_t)nb + 1);
    if (buf.rc) return buf.rc;
    if (hipMemsetAsync(plane, 0, (size_t)n * es, ctx->stream) != hipSuccess) return xd_fail(ctx, XDEMHIP_EHIP, "hipMemsetAsync failed");
    (void)hipEventRecord(ctx->ev_start, ctx->stream);
    for (int k = 0; k < n_tabs; ++k) {
        const int rc = vec_burn<KIND>(ctx, tabs[k], g, memspace, plane, st);
        if (rc) return rc;
    }
    st.mark(4);
    VEC_LAUNCH(ctx, (vec_finish_kernel<KIND>), dim3(nb), dim3(256), 0, ctx->stream, plane, n, d_burn, out_value, part);
    int rc = launched(ctx, "vec_finish_kernel");
    if (rc == XDEMHIP_OK) { rc = fixed_sums_reduce(ctx, part, nb, 1, "vec_finish_kernel"); ++ctx->vec_launches; }
    st.mark(-1);
    (void)hipEventRecord(ctx->ev_stop, ctx->stream);
    ctx->timed = (rc == XDEMHIP_OK);
    if (rc == XDEMHIP_OK) rc = xd_d2h(ctx, &total, part + nb, 8);
    if (rc == XDEMHIP_OK) rc = xd_sync(ctx);
    if (rc) return rc;
    st.collect();
    if (n_burnt) *n_burnt = (int64_t)total;
    return buf.finish();
}

}  // namespace
}  // namespace xd

using namespace xd;

extern "C" {

int xdemhip_rasterize(xdemhip_ctx* ctx, const double* xy, int64_t V, const int64_t* ring_off, int64_t R, const int32_t* poly_of_ring,
                      const int32_t* burn_or_null, int32_t P, int64_t H, int64_t W, const double* transform6, void* out, int out_kind,
                      int32_t out_value, int memspace, int64_t* n_burnt) {
    XdFetchScope fetch_scope_(ctx);
    if (!ctx) return XDEMHIP_EINVAL;
    if (!out) return xd_fail(ctx, XDEMHIP_EINVAL, "null argument");
    if (memspace != XDEMHIP_HOST && memspace != XDEMHIP_DEVICE) return xd_fail(ctx, XDEMHIP_EINVAL, "bad memspace");
    if (out_kind != 0 && out_kind != 1) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_rasterize: out_kind is 0 (uint8 mask) or 1 (int32 labels)");
    VecGrid g;
    int rc = vec_grid(ctx, H, W, transform6, &g);
    if (rc) return rc;
    const VecTable t{xy, V, ring_off, R, poly_of_ring, P};
    rc = vec_check_table(ctx, t, memspace, "xdemhip_rasterize");
    if (rc) return rc;
    XD_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    ctx->vec_launches = 0;
    return out_kind == 0 ? vec_run<0>(ctx, &t, 1, nullptr, g, out, 0, memspace, n_burnt) : vec_run<1>(ctx, &t, 1, burn_or_null, g, out, out_value, memspace, n_burnt);
}

int xdemhip_rasterize_union(xdemhip_ctx* ctx, const double* xy_a, int64_t V_a, const int64_t* ring_off_a, int64_t R_a,
                            const int32_t* poly_of_ring_a, int32_t P_a, const double* xy_b, int64_t V_b, const int64_t* ring_off_b,
                            int64_t R_b, const int32_t* poly_of_ring_b, int32_t P_b, int64_t H, int64_t W, const double* transform6,
                            unsigned char* out, int memspace, int64_t* n_burnt) {
    XdFetchScope fetch_scope_(ctx);
    if (!ctx) return XDEMHIP_EINVAL;
    if (!out) return xd_fail(ctx, XDEMHIP_EINVAL, "null argument");
    if (memspace != XDEMHIP_HOST && memspace != XDEMHIP_DEVICE) return xd_fail(ctx, XDEMHIP_EINVAL, "bad memspace");
    VecGrid g;
    int rc = vec_grid(ctx, H, W, transform6, &g);
    if (rc) return rc;
    const VecTable tabs[2] = {{xy_a, V_a, ring_off_a, R_a, poly_of_ring_a, P_a}, {xy_b, V_b, ring_off_b, R_b, poly_of_ring_b, P_b}};
    for (int k = 0; k < 2; ++k) {
        rc = vec_check_table(ctx, tabs[k], memspace, "xdemhip_rasterize_union");
        if (rc) return rc;
    }
    XD_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    ctx->vec_launches = 0;
    return vec_run<0>(ctx, tabs, 2, nullptr, g, out, 0, memspace, n_burnt);
}

int xdemhip_rasterize_stage_ms(xdemhip_ctx* ctx, float* ms) {
    if (!ctx || !ms) return XDEMHIP_EINVAL;
    for (int k = 0; k < 5; ++k) ms[k] = ctx->vec_stage_ms[k];
    return XDEMHIP_OK;
}

int xdemhip_rasterize_launches(xdemhip_ctx* ctx, int64_t* n_launches) {
    if (!ctx || !n_launches) return XDEMHIP_EINVAL;
    *n_launches = ctx->vec_launches;
    return XDEMHIP_OK;
}

}  // extern "C"
