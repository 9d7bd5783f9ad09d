// edt.hip -- xdemhip_edt: the exact Euclidean distance transform of a target plane (geoutils' Raster.proximity, SciPy's
// distance_transform_edt; DESIGN.md 5p has the rule, include/xdemhip.h states it), and the two small kernels that make target planes:
// xdemhip_edt_targets (a raster's target pixels) and xdemhip_mask_boundary (the inner boundary of a mask).  All arithmetic of the rule
// is float64, one rounding per operation (the Makefile builds this file with -ffp-contract=off); tests/proximity_oracle.py restates it
// in NumPy and every value of the test switch "edt_route" returns its bits.
//
//   cost      c(y, x; ty, tx) = fl( cy(|y - ty|) + cx(|x - tx|) ),  cy(m) = fl(fl(m sy)^2),  cx(k) = fl(fl(k sx)^2)
//   result    d(y, x) = sqrt(min over targets of c); the winner among equal costs: smaller |x - tx|, then smaller tx, then the nearer
//             row of that column, the upper one on a tie
// Three facts make the pruning exact: cy and cx do not decrease with m and k (rounding is monotone), so the nearest target of a column
// is its only candidate; fl(A + B) >= A, so a scan outward from x ends at the first k whose cx(k) reaches the best cost; and a block of
// columns at least `gap` away whose nearest column candidate is m rows away costs at least fl(cx(gap) + cy(m)).  Nothing but these costs
// and their comparisons decides a winner.
//
// Passes (B = bytes per pixel for a float32 result with int16 offsets):
//   down      a thread per column and band of rows walks down: offset to the nearest target above within the band, the band's first and
//             last target row per column, the target count                                                            read 1, write 2
//   carry     a thread per column walks the bands: the nearest target row above and below every band                  (1 / band of the data)
//   up        a thread per column and band walks up: the signed offset to the nearest target of the column (above, below, or across
//             the band's edge through the carries), and the smallest |offset| of every block of columns per row       read 2, write 2
//   row       a workgroup owns a tile of rows x columns, stages the offsets of the tile and a halo in LDS; a lane scans outward from
//             its pixel there and, past the halo, block by block in global memory under the skip rule                 read 2+, write 4
#include "common.h"
#include "../../include/xdemhip_test.h"

#include <limits.h>
#include <math.h>

namespace {

constexpr int EDT_NT = 256;                                   // threads of every workgroup here
constexpr int EDT_NONE = INT_MIN;                             // "no target in this column" as the row pass sees it
constexpr int EDT_SLOTS = 1024, EDT_SLOT_STRIDE = 16;         // counters of the target count: 1024, 128 bytes apart
constexpr int EDT_MAX_VALUES = 64;

struct EdtPlan {
    int band, tw, halo, bc, off_bytes;   // halo < 0: no LDS window (the block search starts at the pixel's own column)
};

// The constants of a call.  Band: 128 rows keep a 40000-row column pass at 313 bands x 157 workgroups while the carries stay below
// 1 % of the plane.  Tile: 256 columns of one row, a halo of 64 on either side (1.5 KiB of LDS: occupancy is never LDS-bound; a
// dense outline is found within a few columns), blocks of 64 columns = one wave of the up pass.
inline EdtPlan edt_plan(int64_t H, int route_switch) {
    EdtPlan p;
    p.band = 128; p.tw = 256; p.halo = 64; p.bc = 64;
    if (route_switch == 1) p.halo = -1;
    if (route_switch == 2) { p.band = 4; p.tw = 64; p.halo = 2; p.bc = 4; }
    p.off_bytes = H <= 32767 ? 2 : 4;
    return p;
}

struct EdtGeom {
    int64_t H, W, nblk, tiles_x;
    double sy, sx;
    int band, tw, rows, halo, bc, keep_polarity;
};

template <typename OffT> struct EdtOff;
template <> struct EdtOff<int16_t> { static constexpr int16_t none = INT16_MIN; };
template <> struct EdtOff<int32_t> { static constexpr int32_t none = INT_MIN; };

// ---- down ---------------------------------------------------------------------------------------------------------------------------
template <typename OffT>
__global__ __launch_bounds__(EDT_NT) void edt_down_kernel(const unsigned char* __restrict__ tg, OffT* __restrict__ off, int* __restrict__ band_first,
                                                          int* __restrict__ band_last, EdtGeom g, unsigned long long* count) {
    __shared__ int wave_sums[EDT_NT / 64];
    const int tid = threadIdx.x;
    const int64_t x = (int64_t)blockIdx.x * EDT_NT + tid, b = blockIdx.y;
    const int64_t y0 = b * g.band, y1 = y0 + g.band < g.H ? y0 + g.band : g.H;
    int n = 0;
    if (x < g.W) {
        int first = -1, last = -1;
#pragma unroll 4
        for (int64_t y = y0; y < y1; ++y) {
            const size_t p = (size_t)y * (size_t)g.W + (size_t)x;
            if (tg[p]) {
                last = (int)y;
                if (first < 0) first = (int)y;
                ++n;
            }
            off[p] = last < 0 ? EdtOff<OffT>::none : (OffT)(last - (int)y);
        }
        band_first[(size_t)b * (size_t)g.W + (size_t)x] = first;
        band_last[(size_t)b * (size_t)g.W + (size_t)x] = last;
    }
    for (int o = 32; o > 0; o >>= 1) n += __shfl_down(n, o, 64);
    if ((tid & 63) == 0) wave_sums[tid >> 6] = n;
    __syncthreads();
    if (tid == 0) {
        int total = 0;
        for (int k = 0; k < EDT_NT / 64; ++k) total += wave_sums[k];
        if (total) atomicAdd(count + (size_t)((blockIdx.x + blockIdx.y * gridDim.x) % EDT_SLOTS) * EDT_SLOT_STRIDE, (unsigned long long)total);
    }
}

// ---- carry: band_last[b] becomes the nearest target row above band b, band_first[b] the nearest below (-1: none) ----------------------
__global__ __launch_bounds__(EDT_NT) void edt_carry_kernel(int* __restrict__ band_first, int* __restrict__ band_last, int64_t W, int64_t nbands) {
    const int64_t x = (int64_t)blockIdx.x * EDT_NT + threadIdx.x;
    if (x >= W) return;
    int above = -1, below = -1;
    for (int64_t b = 0; b < nbands; ++b) {
        const size_t p = (size_t)b * (size_t)W + (size_t)x;
        const int l = band_last[p];
        band_last[p] = above;
        if (l >= 0) above = l;
    }
    for (int64_t b = nbands - 1; b >= 0; --b) {
        const size_t p = (size_t)b * (size_t)W + (size_t)x;
        const int f = band_first[p];
        band_first[p] = below;
        if (f >= 0) below = f;
    }
}

// ---- up -----------------------------------------------------------------------------------------------------------------------------
template <typename OffT>
__global__ __launch_bounds__(EDT_NT) void edt_up_kernel(OffT* __restrict__ off, const int* __restrict__ carry_below, const int* __restrict__ carry_above,
                                                        int* __restrict__ bmin, EdtGeom g) {
    const int tid = threadIdx.x;
    const int64_t x = (int64_t)blockIdx.x * EDT_NT + tid, b = blockIdx.y;
    const int64_t y0 = b * g.band, y1 = y0 + g.band < g.H ? y0 + g.band : g.H;
    const bool live = x < g.W;
    int above = -1, next = -1;
    if (live) {
        above = carry_above[(size_t)b * (size_t)g.W + (size_t)x];
        next = carry_below[(size_t)b * (size_t)g.W + (size_t)x];
    }
    for (int64_t y = y1 - 1; y >= y0; --y) {   // (the same rows for every thread of the workgroup: the shuffles below are uniform)
        int a = INT_MAX;
        if (live) {
            const size_t p = (size_t)y * (size_t)g.W + (size_t)x;
            const OffT u = off[p];
            const int up_row = u == EdtOff<OffT>::none ? above : (int)y + (int)u;
            if (u == 0) next = (int)y;
            OffT out = EdtOff<OffT>::none;
            if (up_row >= 0 && (next < 0 || (int)y - up_row <= next - (int)y)) {   // the nearer row, the upper one on a tie
                out = (OffT)(up_row - (int)y);
                a = (int)y - up_row;
            } else if (next >= 0) {
                out = (OffT)(next - (int)y);
                a = next - (int)y;
            }
            off[p] = out;
        }
        for (int o = 1; o < g.bc; o <<= 1) {
            const int other = __shfl_xor(a, o, 64);
            a = other < a ? other : a;
        }
        if (live && (x % g.bc) == 0) bmin[(size_t)y * (size_t)g.nblk + (size_t)(x / g.bc)] = a;
    }
}

// ---- row ----------------------------------------------------------------------------------------------------------------------------
struct EdtBest {
    double cost;
    unsigned long long key;   // (|x - tx| << 32) | tx: the order among candidates of equal cost
    int off;
};

__device__ inline double edt_cost1(int m, double s) {
    const double a = (double)m * s;
    return a * a;
}

// the candidate of column tx (its nearest target `o` rows away) against the best so far: cost, then |x - tx|, then tx
__device__ inline void edt_consider(EdtBest& best, int64_t x, int64_t tx, int o, double sy, double sx) {
    const int k = (int)(tx > x ? tx - x : x - tx);
    const double c = edt_cost1(o < 0 ? -o : o, sy) + edt_cost1(k, sx);
    const unsigned long long key = ((unsigned long long)(unsigned)k << 32) | (unsigned long long)(unsigned)tx;
    const bool better = c < best.cost || (c == best.cost && key < best.key);
    best.cost = better ? c : best.cost;
    best.key = better ? key : best.key;
    best.off = better ? o : best.off;
}

// nothing at a column distance of `gap` or more, whose costs are at least `c`, can win any more
__device__ inline bool edt_beaten(const EdtBest& best, double c, int64_t gap) {
    return c > best.cost || (c == best.cost && (unsigned long long)gap > (best.key >> 32));
}

template <typename OffT, typename OutT>
__global__ __launch_bounds__(EDT_NT) void edt_row_kernel(const OffT* __restrict__ off, const int* __restrict__ bmin, OutT* __restrict__ dist,
                                                         int32_t* __restrict__ idx, const unsigned char* __restrict__ keep, EdtGeom g) {
    extern __shared__ int edt_win[];   // [rows][tw + 2 halo]
    const int tid = threadIdx.x;
    const int64_t by = (int64_t)blockIdx.x / g.tiles_x, bx = (int64_t)blockIdx.x - by * g.tiles_x;
    const int64_t x0 = bx * g.tw, yb = by * g.rows;
    const int halo = g.halo > 0 ? g.halo : 0, ww = g.tw + 2 * halo;
    if (g.halo >= 0) {
        for (int i = tid; i < g.rows * ww; i += EDT_NT) {
            const int r = i / ww, c = i - r * ww;
            const int64_t gy = yb + r, gx = x0 - halo + c;
            int v = EDT_NONE;
            if (gy < g.H && gx >= 0 && gx < g.W) {
                const OffT o = off[(size_t)gy * (size_t)g.W + (size_t)gx];
                if (o != EdtOff<OffT>::none) v = (int)o;
            }
            edt_win[i] = v;
        }
        __syncthreads();
    }
    const int ly = tid / g.tw, lx = tid - ly * g.tw;
    const int64_t x = x0 + lx, y = yb + ly;
    if (x >= g.W || y >= g.H) return;

    EdtBest best;
    best.cost = INFINITY;
    best.key = ~0ull;   // (no candidate yet: beyond every column distance)
    best.off = 0;
    bool done = false;
    if (g.halo >= 0) {
        const int* win = edt_win + ly * ww + halo + lx;   // win[d]: column x + d
        for (int k = 0; k <= halo; ++k) {
            if (edt_beaten(best, edt_cost1(k, g.sx), k)) { done = true; break; }
            const int l = win[-k];
            if (l != EDT_NONE) edt_consider(best, x, x - k, l, g.sy, g.sx);
            const int r = win[k];
            if (k > 0 && r != EDT_NONE) edt_consider(best, x, x + k, r, g.sy, g.sx);
        }
    }
    if (!done) {
        // beyond the window: the blocks of columns to the left (side 0) and to the right (side 1) in turn, each clipped to the
        // columns the window has not covered (without a window both sides start at the pixel's own column)
        const OffT* row = off + (size_t)y * (size_t)g.W;
        const int* brow = bmin + (size_t)y * (size_t)g.nblk;
        const int64_t lhi = x - g.halo - 1, rlo = x + g.halo + 1;
        bool ldone = lhi < 0, rdone = rlo >= g.W;
        int64_t lb = ldone ? 0 : lhi / g.bc, rb = rdone ? 0 : rlo / g.bc;
        for (int side = 0; !(ldone && rdone); side ^= 1) {
            if (side == 0 ? ldone : rdone) continue;
            const int64_t b = side == 0 ? lb : rb;
            int64_t lo = b * g.bc, hi = lo + g.bc - 1;
            if (side == 0) hi = hi < lhi ? hi : lhi;
            else {
                lo = lo > rlo ? lo : rlo;
                hi = hi < g.W - 1 ? hi : g.W - 1;
            }
            const int64_t gap = side == 0 ? x - hi : lo - x;
            const double ck = edt_cost1((int)gap, g.sx);
            bool stop = edt_beaten(best, ck, gap);
            if (!stop) {
                const int m = brow[b];
                if (m != INT_MAX && !edt_beaten(best, ck + edt_cost1(m, g.sy), gap))
                    for (int64_t tx = lo; tx <= hi; ++tx) {
                        const OffT o = row[tx];
                        if (o != EdtOff<OffT>::none) edt_consider(best, x, tx, (int)o, g.sy, g.sx);
                    }
                if (side == 0) stop = --lb < 0;
                else stop = ++rb >= g.nblk;
            }
            if (stop) {
                if (side == 0) ldone = true;
                else rdone = true;
            }
        }
    }
    const bool found = best.key != ~0ull;
    const int best_tx = (int)(unsigned)(best.key & 0xffffffffull);
    const size_t p = (size_t)y * (size_t)g.W + (size_t)x;
    if (dist) {
        double d = found ? sqrt(best.cost) : (double)INFINITY;
        if (keep && (keep[p] != 0) != (g.keep_polarity != 0)) d = 0.0;
        dist[p] = (OutT)d;
    }
    if (idx) {
        idx[p] = found ? (int32_t)((int)y + best.off) : -1;
        idx[(size_t)g.H * (size_t)g.W + p] = found ? best_tx : -1;
    }
}

// ---- target planes ------------------------------------------------------------------------------------------------------------------
struct EdtValues {
    double v[EDT_MAX_VALUES];
    int n;
};

template <typename T>
__global__ __launch_bounds__(EDT_NT) void edt_targets_kernel(const T* __restrict__ src, unsigned char* __restrict__ out, int64_t n, EdtValues vals) {
    const int64_t i = (int64_t)blockIdx.x * EDT_NT + threadIdx.x;
    if (i >= n) return;
    const double v = (double)src[i];
    bool t = false;
    if (vals.n == 0) t = fabs(v) < INFINITY && v != 0.0;
    for (int k = 0; k < vals.n; ++k) t = t || v == vals.v[k];   // (NaN equals nothing)
    out[i] = t ? 1 : 0;
}

__global__ __launch_bounds__(EDT_NT) void edt_boundary_kernel(const unsigned char* __restrict__ m, unsigned char* __restrict__ out, int64_t H, int64_t W,
                                                              int64_t tiles_x) {
    const int64_t by = (int64_t)blockIdx.x / tiles_x, bx = (int64_t)blockIdx.x - by * tiles_x;
    const int64_t x = bx * 64 + (threadIdx.x & 63), y = by * (EDT_NT / 64) + (threadIdx.x >> 6);
    if (x >= W || y >= H) return;
    const size_t p = (size_t)y * (size_t)W + (size_t)x;
    bool edge = false;
    if (m[p]) edge = (y > 0 && !m[p - (size_t)W]) || (y < H - 1 && !m[p + (size_t)W]) || (x > 0 && !m[p - 1]) || (x < W - 1 && !m[p + 1]);
    out[p] = edge ? 1 : 0;
}

template <typename OffT, typename OutT>
void edt_launch_row(xdemhip_ctx* ctx, const void* off, const int* bmin, void* dist, int32_t* idx, const unsigned char* keep, const EdtGeom& g,
                    int64_t blocks, size_t lds) {
    hipLaunchKernelGGL((edt_row_kernel<OffT, OutT>), dim3((unsigned)blocks), dim3(EDT_NT), lds, ctx->stream, static_cast<const OffT*>(off), bmin,
                       static_cast<OutT*>(dist), idx, keep, g);
}

struct EdtEvents {   // the five events around the four passes of one call
    hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    bool ok = true;
    EdtEvents() {
        for (auto& e : ev)
            if (hipEventCreate(&e) != hipSuccess) { e = nullptr; ok = false; (void)hipGetLastError(); }
    }
    ~EdtEvents() {
        for (auto& e : ev)
            if (e) (void)hipEventDestroy(e);
    }
    void mark(int k, hipStream_t s) { if (ok) (void)hipEventRecord(ev[k], s); }
};

}  // namespace

extern "C" {

int xdemhip_edt_plan(int64_t H, int64_t W, int route_switch, int* band_rows, int* tile_cols, int* halo, int* block_cols, int* offset_bytes) {
    if (H < 1 || W < 1 || route_switch < 0 || route_switch > 2) return XDEMHIP_EINVAL;
    const EdtPlan p = edt_plan(H, route_switch);
    if (band_rows) *band_rows = p.band;
    if (tile_cols) *tile_cols = p.tw;
    if (halo) *halo = p.halo > 0 ? p.halo : 0;
    if (block_cols) *block_cols = p.bc;
    if (offset_bytes) *offset_bytes = p.off_bytes;
    return XDEMHIP_OK;
}

int xdemhip_edt_stage_ms(xdemhip_ctx* ctx, float* ms) {
    if (!ctx || !ms) return XDEMHIP_EINVAL;
    for (int k = 0; k < 4; ++k) ms[k] = ctx->edt_stage_ms[k];
    return XDEMHIP_OK;
}

int xdemhip_edt(xdemhip_ctx* ctx, const unsigned char* targets, int64_t H, int64_t W, double sy, double sx, void* dist, int dist_dtype,
                int32_t* idx, const unsigned char* keep, int keep_polarity, int memspace, int64_t* n_targets) {
    if (!ctx) return XDEMHIP_EINVAL;
    if (!targets) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_edt: null target plane");
    const int64_t LIM = (int64_t)1 << 31;
    if (H < 1 || W < 1 || H >= LIM || W >= LIM) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_edt: raster sides must be 1 .. 2^31 - 1");
    if (!(sy > 0.0 && sx > 0.0 && sy < INFINITY && sx < INFINITY)) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_edt: the sampling must be finite and > 0");
    if (dist_dtype != XDEMHIP_F32 && dist_dtype != XDEMHIP_F64) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_edt: dist_dtype must be XDEMHIP_F32 or XDEMHIP_F64");
    if (memspace != XDEMHIP_HOST && memspace != XDEMHIP_DEVICE) return xd_fail(ctx, XDEMHIP_EINVAL, "memspace must be XDEMHIP_HOST or XDEMHIP_DEVICE");

    const EdtPlan plan = edt_plan(H, ctx->edt_route);
    EdtGeom g;
    g.H = H; g.W = W; g.sy = sy; g.sx = sx;
    g.band = plan.band; g.tw = plan.tw; g.rows = EDT_NT / plan.tw; g.halo = plan.halo; g.bc = plan.bc;
    g.keep_polarity = keep_polarity;
    g.nblk = (W + plan.bc - 1) / plan.bc;
    g.tiles_x = (W + plan.tw - 1) / plan.tw;
    const int64_t nbands = (H + plan.band - 1) / plan.band, cols_x = (W + EDT_NT - 1) / EDT_NT;
    const int64_t row_blocks = g.tiles_x * ((H + g.rows - 1) / g.rows);
    if (row_blocks >= LIM || nbands > 65535) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_edt: plane too large for one launch");

    XD_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    const size_t n = (size_t)H * (size_t)W, dist_size = dist_dtype == XDEMHIP_F32 ? 4 : 8;
    XdPrefault prefault;
    std::vector<unsigned long long> counted((size_t)EDT_SLOTS * EDT_SLOT_STRIDE, 0);   // (declared before the scope whose copies land in it)
    const size_t counted_bytes = counted.size() * sizeof(unsigned long long);
    EdtEvents events;
    XdBuffers buf(ctx, "xdemhip_edt");
    const unsigned char* d_targets = buf.input(targets, n, memspace);
    const unsigned char* d_keep = dist ? buf.input(keep, n, memspace) : nullptr;
    void* d_dist = buf.output(dist, n * dist_size, memspace);
    int32_t* d_idx = buf.output(idx, 2 * n * sizeof(int32_t), memspace);
    unsigned long long* d_count = buf.output(counted.data(), counted_bytes, XDEMHIP_HOST);
    void* d_off = buf.alloc(n * (size_t)plan.off_bytes);
    int* d_bmin = buf.alloc<int>((size_t)H * (size_t)g.nblk);
    int* d_first = buf.alloc<int>((size_t)nbands * (size_t)W);
    int* d_last = buf.alloc<int>((size_t)nbands * (size_t)W);
    if (buf.rc) return buf.rc;
    if (memspace == XDEMHIP_HOST) xd_prefault_start(prefault, dist, dist ? n * dist_size : 0, ctx->host_copy_threads);
    XD_HIP_CHECK(ctx, hipMemsetAsync(d_count, 0, counted_bytes, ctx->stream));
    XD_HIP_CHECK(ctx, hipEventRecord(ctx->ev_start, ctx->stream));
    const dim3 col_grid((unsigned)cols_x, (unsigned)nbands);
    events.mark(0, ctx->stream);
    if (plan.off_bytes == 2) hipLaunchKernelGGL(edt_down_kernel<int16_t>, col_grid, dim3(EDT_NT), 0, ctx->stream, d_targets, static_cast<int16_t*>(d_off), d_first, d_last, g, d_count);
    else hipLaunchKernelGGL(edt_down_kernel<int32_t>, col_grid, dim3(EDT_NT), 0, ctx->stream, d_targets, static_cast<int32_t*>(d_off), d_first, d_last, g, d_count);
    events.mark(1, ctx->stream);
    hipLaunchKernelGGL(edt_carry_kernel, dim3((unsigned)cols_x), dim3(EDT_NT), 0, ctx->stream, d_first, d_last, W, nbands);
    events.mark(2, ctx->stream);
    if (plan.off_bytes == 2) hipLaunchKernelGGL(edt_up_kernel<int16_t>, col_grid, dim3(EDT_NT), 0, ctx->stream, static_cast<int16_t*>(d_off), d_first, d_last, d_bmin, g);
    else hipLaunchKernelGGL(edt_up_kernel<int32_t>, col_grid, dim3(EDT_NT), 0, ctx->stream, static_cast<int32_t*>(d_off), d_first, d_last, d_bmin, g);
    events.mark(3, ctx->stream);
    if (dist || idx) {
        const size_t lds = plan.halo >= 0 ? (size_t)g.rows * (size_t)(plan.tw + 2 * plan.halo) * sizeof(int) : 0;
        if (plan.off_bytes == 2 && dist_dtype == XDEMHIP_F32) edt_launch_row<int16_t, float>(ctx, d_off, d_bmin, d_dist, d_idx, d_keep, g, row_blocks, lds);
        else if (plan.off_bytes == 2) edt_launch_row<int16_t, double>(ctx, d_off, d_bmin, d_dist, d_idx, d_keep, g, row_blocks, lds);
        else if (dist_dtype == XDEMHIP_F32) edt_launch_row<int32_t, float>(ctx, d_off, d_bmin, d_dist, d_idx, d_keep, g, row_blocks, lds);
        else edt_launch_row<int32_t, double>(ctx, d_off, d_bmin, d_dist, d_idx, d_keep, g, row_blocks, lds);
    }
    events.mark(4, ctx->stream);
    (void)hipEventRecord(ctx->ev_stop, ctx->stream);
    ctx->timed = true;
    int rc = launched(ctx, "edt kernels");
    prefault.join();
    if (rc == XDEMHIP_OK) rc = buf.finish();
    for (int k = 0; k < 4; ++k) {
        ctx->edt_stage_ms[k] = 0.f;
        if (rc == XDEMHIP_OK && events.ok && hipEventElapsedTime(&ctx->edt_stage_ms[k], events.ev[k], events.ev[k + 1]) != hipSuccess) {
            (void)hipGetLastError();
            ctx->edt_stage_ms[k] = 0.f;
        }
    }
    if (rc == XDEMHIP_OK && n_targets) {
        unsigned long long total = 0;
        for (int k = 0; k < EDT_SLOTS; ++k) total += counted[(size_t)k * EDT_SLOT_STRIDE];
        *n_targets = (int64_t)total;
    }
    return rc;
}

int xdemhip_edt_targets(xdemhip_ctx* ctx, const void* src, int src_dtype, int64_t n, const double* values, int n_values, unsigned char* out,
                        int memspace) {
    if (!ctx) return XDEMHIP_EINVAL;
    if (!src || !out || n < 1) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_edt_targets: null argument or n < 1");
    if (n_values < 0 || n_values > EDT_MAX_VALUES || (n_values > 0 && !values))
        return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_edt_targets: 0 to 64 target values");
    if (memspace != XDEMHIP_HOST && memspace != XDEMHIP_DEVICE) return xd_fail(ctx, XDEMHIP_EINVAL, "memspace must be XDEMHIP_HOST or XDEMHIP_DEVICE");
    size_t size = 0;
    if (src_dtype == XDEMHIP_F32 || src_dtype == XDEMHIP_I32) size = 4;
    else if (src_dtype == XDEMHIP_F64) size = 8;
    else if (src_dtype == XDEMHIP_U8) size = 1;
    else return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_edt_targets: src_dtype must be XDEMHIP_F32, _F64, _U8 or _I32");
    const int64_t blocks = (n + EDT_NT - 1) / EDT_NT;
    if (blocks >= ((int64_t)1 << 31)) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_edt_targets: raster too large for one launch");
    EdtValues vals;
    vals.n = n_values;
    for (int k = 0; k < EDT_MAX_VALUES; ++k) vals.v[k] = k < n_values ? values[k] : 0.0;
    XD_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    XdBuffers buf(ctx, "xdemhip_edt_targets");
    const void* d_src = buf.input(static_cast<const unsigned char*>(src), (size_t)n * size, memspace);
    unsigned char* d_out = buf.output(out, (size_t)n, memspace);
    if (buf.rc) return buf.rc;
    const dim3 grid((unsigned)blocks), block(EDT_NT);
    if (src_dtype == XDEMHIP_F32) hipLaunchKernelGGL(edt_targets_kernel<float>, grid, block, 0, ctx->stream, static_cast<const float*>(d_src), d_out, n, vals);
    else if (src_dtype == XDEMHIP_F64) hipLaunchKernelGGL(edt_targets_kernel<double>, grid, block, 0, ctx->stream, static_cast<const double*>(d_src), d_out, n, vals);
    else if (src_dtype == XDEMHIP_U8) hipLaunchKernelGGL(edt_targets_kernel<unsigned char>, grid, block, 0, ctx->stream, static_cast<const unsigned char*>(d_src), d_out, n, vals);
    else hipLaunchKernelGGL(edt_targets_kernel<int32_t>, grid, block, 0, ctx->stream, static_cast<const int32_t*>(d_src), d_out, n, vals);
    const int rc = launched(ctx, "edt targets kernel");
    return rc == XDEMHIP_OK ? buf.finish() : rc;
}

int xdemhip_mask_boundary(xdemhip_ctx* ctx, const unsigned char* mask, int64_t H, int64_t W, unsigned char* out, int memspace) {
    if (!ctx) return XDEMHIP_EINVAL;
    if (!mask || !out) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_mask_boundary: null argument");
    const int64_t LIM = (int64_t)1 << 31;
    if (H < 1 || W < 1 || H >= LIM || W >= LIM) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_mask_boundary: raster sides must be 1 .. 2^31 - 1");
    if (memspace != XDEMHIP_HOST && memspace != XDEMHIP_DEVICE) return xd_fail(ctx, XDEMHIP_EINVAL, "memspace must be XDEMHIP_HOST or XDEMHIP_DEVICE");
    const int64_t gx = (W + 63) / 64, gy = (H + EDT_NT / 64 - 1) / (EDT_NT / 64);
    if (gx * gy >= LIM) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_mask_boundary: raster too large for one launch");
    XD_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    XdBuffers buf(ctx, "xdemhip_mask_boundary");
    const unsigned char* d_mask = buf.input(mask, (size_t)H * (size_t)W, memspace);
    unsigned char* d_out = buf.output(out, (size_t)H * (size_t)W, memspace);
    if (buf.rc) return buf.rc;
    hipLaunchKernelGGL(edt_boundary_kernel, dim3((unsigned)(gx * gy)), dim3(EDT_NT), 0, ctx->stream, d_mask, d_out, H, W, gx);
    const int rc = launched(ctx, "mask boundary kernel");
    return rc == XDEMHIP_OK ? buf.finish() : rc;
}

}  // extern "C"
