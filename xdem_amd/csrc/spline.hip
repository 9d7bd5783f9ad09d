// spline.hip -- sampling a raster at points with SciPy's map_coordinates rule (geoutils' Raster.interp_points; DESIGN.md 5q has the
// rule, include/xdemhip.h states it), and a raster as a point cloud (Raster.to_pointcloud):
//   xdemhip_spline_prepare   a raster -> a uint8 `spread` plane (the 4-connected dilation of its non-finite pixels) and, for orders 3 and
//                            5, the float64 B-spline coefficients of the raster with its voids filled from the nearest finite pixel
//   xdemhip_spline_gather    points -> values: one thread per point does the coordinate, the outside test, the spread test, the weights,
//                            the taps and the one rounding
//   xdemhip_raster_points    a raster -> x, y, z columns in row-major order, finite pixels only on request (order-preserving compaction)
// All arithmetic of the rule is float64, one rounding per operation (the Makefile builds this file with -ffp-contract=off);
// tests/interp_oracle.py restates it in NumPy.
//
// The prefilter.  Per axis the samples take a gain, then per pole z a causal recursion c+[i] = s[i] + z c+[i-1] and an anticausal one
// c-[i] = z (c-[i+1] - c+[i]), both started by SciPy's mirror formulas at the raster's edges.  |z| <= 0.43, so a recursion started
// SP_HALO = 64 samples early from any value has forgotten it (0.43^64 = 3.5e-24): a band of rows or a segment of a row starts its
// causal recursion 64 samples before its first sample and takes its anticausal start from the 64 samples after its last one,
//   c-[y1] = -z sum_{j < m} z^j c+[y1 + j]  (+ z^m c-[n-1] when the m-th sample is the last of the line),
// which is summed forward while the causal recursion runs on: one walk down, one walk back.  A pass never works in place: the
// passes alternate between two float64 planes (the first reads the raster itself).
//
// Passes (bytes per pixel; T = 4 or 8 of the raster; band 256, tile 32 x 256, halo 64):
//   mask      finite flags and the count of non-finite pixels                                              read T, write 1
//   fill      (only with voids) xdemhip_edt's indices of the nearest finite pixel, then a gather           edt + read 1 + 8 + T, write T
//   dilate    diamond of radius <= 3 from an LDS tile with a halo (larger distances: repeated)             read ~1.6, write 1
//   column    a thread per column and band: walks down through band + halo, back up through the band       read 1.5 x (T or 8) + 8, write 16
//   row       a workgroup stages 32 x (256 + 128) samples in LDS (row stride 385 doubles: the 32 lanes of a group walk 32 rows in
//             32 different banks); a lane per row and 32-column segment; the tile leaves in full 64-lane runs   read 12, write 8
#include "common.h"
#include "../../include/xdemhip_test.h"
#include "spline_line.h"

#include <math.h>

namespace {

constexpr int SP_NT = 256;
constexpr int SP_BAND = 256;
constexpr int SP_TILE_ROWS = 32, SP_TILE_COLS = 256, SP_SEG = 32;
constexpr int SP_WIN = SP_TILE_COLS + 2 * SP_HALO;     // staged samples of a tile row
constexpr int SP_STRIDE = SP_WIN + 1;                  // doubles between tile rows in LDS (odd: no two rows of a lane group share a bank)
constexpr int SP_LDS_BYTES = SP_TILE_ROWS * SP_STRIDE * 8;
constexpr int SP_DIL_R = 3, SP_DIL_ROWS = 16;

struct SpPlan {
    int band, tile_rows, tile_cols, halo, lds_bytes;
    bool lds_rows;
};

// switch: 0 banded columns, LDS rows where a row is longer than its two halos; 1 one band per column; 2 the plain row route always;
// 3 the LDS row route always
inline SpPlan sp_plan(int64_t H, int64_t W, int route_switch) {
    SpPlan p;
    p.halo = SP_HALO;
    p.band = route_switch == 1 ? (int)H : SP_BAND;
    p.lds_rows = route_switch == 3 || (route_switch != 2 && W > 2 * SP_HALO);
    p.tile_rows = p.lds_rows ? SP_TILE_ROWS : 1;
    p.tile_cols = p.lds_rows ? SP_TILE_COLS : (int)W;
    p.lds_bytes = p.lds_rows ? SP_LDS_BYTES : 0;
    return p;
}

template <typename T> struct SpGlobalIn {
    const T* p;
    size_t stride;
    double gain;
    __device__ double operator()(int64_t i) const { return (double)p[(size_t)i * stride] * gain; }
};
struct SpGlobalOut {
    double* p;
    size_t stride;
    __device__ double get(int64_t i) const { return p[(size_t)i * stride]; }
    __device__ void put(int64_t i, double v) { p[(size_t)i * stride] = v; }
};

// ---- column pass: a thread per column and band of rows ---------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(SP_NT) void sp_col_kernel(const T* __restrict__ src, double* __restrict__ dst, int64_t H, int64_t W, int band, SpPole p) {
    const int64_t x = (int64_t)blockIdx.x * SP_NT + threadIdx.x;
    if (x >= W) return;
    const int64_t y0 = (int64_t)blockIdx.y * band, y1 = y0 + band < H ? y0 + band : H;
    const SpGlobalIn<T> in{src + x, (size_t)W, p.gain};
    SpGlobalOut out{dst + x, (size_t)W};
    SpWarm warm;
    double cm;
    bool last;
    sp_forward<true>(in, out, H, y0, y1, p, warm, cm, last);
    sp_backward(out, y0, y1, cm, last, p.z);
}

// ---- row pass, plain: a thread per row -----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SP_NT) void sp_row_plain_kernel(const double* __restrict__ src, double* __restrict__ dst, int64_t H, int64_t W, SpPole p) {
    const int64_t y = (int64_t)blockIdx.x * SP_NT + threadIdx.x;
    if (y >= H) return;
    const SpGlobalIn<double> in{src + (size_t)y * (size_t)W, 1, p.gain};
    SpGlobalOut out{dst + (size_t)y * (size_t)W, 1};
    SpWarm warm;
    double cm;
    bool last;
    sp_forward<true>(in, out, W, 0, W, p, warm, cm, last);
    sp_backward(out, 0, W, cm, last, p.z);
}

// ---- row pass, LDS: a workgroup per tile of 32 rows x 256 columns -------------------------------------------------------------------
struct SpLdsLine {      // sample i of the raster row lives at win[i - first]
    double* win;
    int64_t first;
    __device__ double operator()(int64_t i) const { return win[i - first]; }
    __device__ double get(int64_t i) const { return win[i - first]; }
    __device__ void put(int64_t i, double v) { win[i - first] = v; }
};

__global__ __launch_bounds__(SP_NT) void sp_row_lds_kernel(const double* __restrict__ src, double* __restrict__ dst, int64_t H, int64_t W,
                                                           int64_t tiles_x, SpPole p) {
    extern __shared__ double sp_tile[];   // [SP_TILE_ROWS][SP_STRIDE]
    const int tid = threadIdx.x;
    const int64_t by = (int64_t)blockIdx.x / tiles_x, bx = (int64_t)blockIdx.x - by * tiles_x;
    const int64_t x0 = bx * SP_TILE_COLS, yb = by * SP_TILE_ROWS, first = x0 - SP_HALO;
    for (int i = tid; i < SP_TILE_ROWS * SP_WIN; i += SP_NT) {
        const int r = i / SP_WIN, c = i - r * SP_WIN;
        const int64_t gy = yb + r, gx = first + c;
        double v = 0.0;
        if (gy < H && gx >= 0 && gx < W) v = src[(size_t)gy * (size_t)W + (size_t)gx] * p.gain;
        sp_tile[r * SP_STRIDE + c] = v;
    }
    __syncthreads();
    const int r = tid & (SP_TILE_ROWS - 1), s = tid / SP_TILE_ROWS;
    const int64_t y0 = x0 + (int64_t)s * SP_SEG, y1 = y0 + SP_SEG < W ? y0 + SP_SEG : W;
    const bool live = yb + r < H && y0 < W;
    SpLdsLine line{sp_tile + r * SP_STRIDE, first};
    SpWarm warm;
    double cm = 0.0;
    bool last = false;
    if (live) sp_forward<false>(line, line, W, y0, y1, p, warm, cm, last);   // (reads only: the neighbours' segments are still samples)
    __syncthreads();
    if (live) {
        sp_replay(line, line, y0, y1, p, warm);
        sp_backward(line, y0, y1, cm, last, p.z);
    }
    __syncthreads();
    for (int i = tid; i < SP_TILE_ROWS * SP_TILE_COLS; i += SP_NT) {
        const int rr = i / SP_TILE_COLS, c = i - rr * SP_TILE_COLS;
        const int64_t gy = yb + rr, gx = x0 + c;
        if (gy < H && gx < W) dst[(size_t)gy * (size_t)W + (size_t)gx] = sp_tile[rr * SP_STRIDE + SP_HALO + c];
    }
}

// ---- nodata: finite flags, fill, dilation ----------------------------------------------------------------------------------------------
__device__ inline void sp_block_count(int n, unsigned long long* count) {
    __shared__ int wave_sums[SP_NT / 64];
    for (int o = 32; o > 0; o >>= 1) n += __shfl_down(n, o, 64);
    if ((threadIdx.x & 63) == 0) wave_sums[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) {
        int total = 0;
        for (int k = 0; k < SP_NT / 64; ++k) total += wave_sums[k];
        if (total) atomicAdd(count, (unsigned long long)total);
    }
}

template <typename T>
__global__ __launch_bounds__(SP_NT) void sp_mask_kernel(const T* __restrict__ src, unsigned char* __restrict__ fin, int64_t n, unsigned long long* count) {
    const int64_t i = (int64_t)blockIdx.x * SP_NT + threadIdx.x;
    int bad = 0;
    if (i < n) {
        const bool f = fabs((double)src[i]) < INFINITY;
        fin[i] = f ? 1 : 0;
        bad = f ? 0 : 1;
    }
    sp_block_count(bad, count);
}

template <typename T>
__global__ __launch_bounds__(SP_NT) void sp_fill_kernel(const T* __restrict__ src, const unsigned char* __restrict__ fin, const int32_t* __restrict__ idx,
                                                        T* __restrict__ out, int64_t n, int64_t W) {
    const int64_t i = (int64_t)blockIdx.x * SP_NT + threadIdx.x;
    if (i >= n) return;
    T v = src[i];
    if (!fin[i]) {
        const int64_t ty = idx[i], tx = idx[(size_t)n + (size_t)i];
        v = src[(size_t)ty * (size_t)W + (size_t)tx];
    }
    out[i] = v;
}

// out = 1 where a pixel within city-block distance `radius` (<= SP_DIL_R) of (y, x) is set in `in` (set = non-zero, or zero if invert)
__global__ __launch_bounds__(SP_NT) void sp_dilate_kernel(const unsigned char* __restrict__ in, unsigned char* __restrict__ out, int64_t H, int64_t W,
                                                          int64_t tiles_x, int radius, int invert) {
    constexpr int TW = 64 + 2 * SP_DIL_R, TH = SP_DIL_ROWS + 2 * SP_DIL_R;
    __shared__ unsigned char tile[TH][TW + 2];
    const int tid = threadIdx.x;
    const int64_t by = (int64_t)blockIdx.x / tiles_x, bx = (int64_t)blockIdx.x - by * tiles_x;
    const int64_t x0 = bx * 64, y0 = by * SP_DIL_ROWS;
    for (int i = tid; i < TH * TW; i += SP_NT) {
        const int r = i / TW, c = i - r * TW;
        const int64_t gy = y0 - SP_DIL_R + r, gx = x0 - SP_DIL_R + c;
        unsigned char v = 0;
        if (gy >= 0 && gy < H && gx >= 0 && gx < W) v = (in[(size_t)gy * (size_t)W + (size_t)gx] != 0) != (invert != 0) ? 1 : 0;
        tile[r][c] = v;
    }
    __syncthreads();
    const int lx = tid & 63;
    const int64_t x = x0 + lx;
    if (x >= W) return;
    for (int ly = tid >> 6; ly < SP_DIL_ROWS; ly += SP_NT / 64) {
        const int64_t y = y0 + ly;
        if (y >= H) break;
        unsigned char any = 0;
        for (int dy = -radius; dy <= radius; ++dy) {
            const int w = radius - (dy < 0 ? -dy : dy);
            for (int dx = -w; dx <= w; ++dx) any |= tile[ly + SP_DIL_R + dy][lx + SP_DIL_R + dx];
        }
        out[(size_t)y * (size_t)W + (size_t)x] = any;
    }
}

// ---- gather -------------------------------------------------------------------------------------------------------------------------
struct SpGeom {
    int64_t H, W;
    double a, c, e, f, half;   // r = (y - f) / e - half, cc = (x - c) / a - half
    int all_nan;
};

template <int ORDER> __device__ inline void sp_weights(double t, double* w);
template <> __device__ inline void sp_weights<1>(double t, double* w) {
    w[0] = 1.0 - t;
    w[1] = 1.0 - w[0];
}
template <> __device__ inline void sp_weights<3>(double t, double* w) {
    const double y = t, z = 1.0 - t;
    w[0] = z * z * z / 6.0;
    w[1] = (y * y * (y - 2.0) * 3.0 + 4.0) / 6.0;
    w[2] = (z * z * (z - 2.0) * 3.0 + 4.0) / 6.0;
    w[3] = 1.0 - (w[0] + w[1] + w[2]);
}
template <> __device__ inline void sp_weights<5>(double t, double* w) {
    const double y = t, z = 1.0 - t, ty = y * y, tz = z * z, y1 = y + 1.0, z1 = z + 1.0;
    w[0] = tz * tz * z / 120.0;
    w[1] = (y1 * (y1 * (y1 * (y1 * (y1 * 5.0 - 45.0) + 150.0) - 210.0) + 75.0) + 51.0) / 120.0;
    w[2] = (ty * (ty * (y * -10.0 + 30.0) - 60.0) + 66.0) / 120.0;
    w[3] = (tz * (tz * (z * -10.0 + 30.0) - 60.0) + 66.0) / 120.0;
    w[4] = (z1 * (z1 * (z1 * (z1 * (z1 * 5.0 - 45.0) + 150.0) - 210.0) + 75.0) + 51.0) / 120.0;
    w[5] = 1.0 - ((((w[0] + w[1]) + w[2]) + w[3]) + w[4]);
}

__device__ inline int64_t sp_mirror(int64_t i, int64_t n) {
    const int64_t s2 = 2 * n - 2;
    int64_t m = i % s2;
    if (m < 0) m += s2;
    return m >= n ? s2 - m : m;
}

// T: the result's dtype; S: what the taps read (the raster for orders 0 and 1, the float64 coefficients above)
template <typename T, typename S, int ORDER>
__global__ __launch_bounds__(SP_NT) void sp_gather_kernel(const S* __restrict__ src, const unsigned char* __restrict__ spread, const double* __restrict__ xs,
                                                          const double* __restrict__ ys, T* __restrict__ out, int64_t n, SpGeom g, unsigned long long* count) {
    const int64_t i = (int64_t)blockIdx.x * SP_NT + threadIdx.x;
    int valid = 0;
    if (i < n) {
        const double r = (ys[i] - g.f) / g.e - g.half, cc = (xs[i] - g.c) / g.a - g.half;
        const size_t W = (size_t)g.W;
        bool ok = !g.all_nan && r >= 0.0 && r <= (double)(g.H - 1) && cc >= 0.0 && cc <= (double)(g.W - 1);   // (NaN fails every test)
        double v = NAN;
        if (ok) {
            const double fr = floor(r), fc = floor(cc);
            const int64_t ir = (int64_t)fr, ic = (int64_t)fc;
            const double tr = r - fr, tc = cc - fc;
            if (spread) {
                // the four bilinear corners; a corner past the last row or column has weight 0
                const double wr0 = 1.0 - tr, wc0 = 1.0 - tc, wr1 = 1.0 - wr0, wc1 = 1.0 - wc0;
                const size_t r0 = (size_t)ir * W, r1 = (size_t)(ir + 1 < g.H ? ir + 1 : g.H - 1) * W;
                const size_t c0 = (size_t)ic, c1 = (size_t)(ic + 1 < g.W ? ic + 1 : g.W - 1);
                const bool hit = spread[r0 + c0] || (wc1 != 0.0 && spread[r0 + c1]) || (wr1 != 0.0 && spread[r1 + c0]) ||
                                 (wr1 != 0.0 && wc1 != 0.0 && spread[r1 + c1]);
                ok = !hit;
            }
            if (ok) {
                if constexpr (ORDER == 0) {
                    const int64_t nr = (int64_t)floor(r + 0.5), nc = (int64_t)floor(cc + 0.5);
                    v = (double)src[(size_t)nr * W + (size_t)nc];
                } else {
                    double wr[ORDER + 1], wc[ORDER + 1];
                    sp_weights<ORDER>(tr, wr);
                    sp_weights<ORDER>(tc, wc);
                    size_t cols[ORDER + 1];
#pragma unroll
                    for (int k = 0; k <= ORDER; ++k) cols[k] = (size_t)sp_mirror(ic - ORDER / 2 + k, g.W);
                    double total = 0.0;
#pragma unroll
                    for (int a = 0; a <= ORDER; ++a) {
                        const size_t row = (size_t)sp_mirror(ir - ORDER / 2 + a, g.H) * W;
#pragma unroll
                        for (int b = 0; b <= ORDER; ++b) {
                            if (ORDER == 1 && (wr[a] == 0.0 || wc[b] == 0.0)) continue;   // (a tap of weight 0 is not read: it may be a void)
                            total = total + ((double)src[row + cols[b]] * wr[a]) * wc[b];
                        }
                    }
                    v = total;
                }
            }
        }
        const T res = (T)v;
        out[i] = res;
        valid = res == res ? 1 : 0;
    }
    sp_block_count(valid, count);
}

// ---- raster -> points -----------------------------------------------------------------------------------------------------------------
// a wave per row: the number of finite pixels of the row
template <typename T>
__global__ __launch_bounds__(64) void sp_row_count_kernel(const T* __restrict__ src, int64_t W, unsigned long long* __restrict__ counts) {
    const T* row = src + (size_t)blockIdx.x * (size_t)W;
    unsigned long long n = 0;
    for (int64_t x0 = 0; x0 < W; x0 += 64) {
        const int64_t x = x0 + threadIdx.x;
        const bool f = x < W && fabs((double)row[x]) < INFINITY;
        n += (unsigned long long)__popcll(__ballot(f));
    }
    if (threadIdx.x == 0) counts[blockIdx.x] = n;
}

// exclusive scan of a[0 .. n) in place by one workgroup, the total in a[n]: a chunk per lane, the chunk sums scanned in LDS
__global__ __launch_bounds__(SP_NT) void sp_scan_kernel(unsigned long long* __restrict__ a, int64_t n) {
    __shared__ unsigned long long s[SP_NT];
    const int tid = threadIdx.x;
    const int64_t per = (n + SP_NT - 1) / SP_NT, lo = per * tid, hi = lo + per < n ? lo + per : n;
    unsigned long long sum = 0;
    for (int64_t i = lo; i < hi; ++i) sum += a[i];
    s[tid] = sum;
    __syncthreads();
    for (int off = 1; off < SP_NT; off <<= 1) {
        const unsigned long long b = tid >= off ? s[tid - off] : 0ull;
        __syncthreads();
        s[tid] += b;
        __syncthreads();
    }
    unsigned long long run = s[tid] - sum;
    for (int64_t i = lo; i < hi; ++i) {
        const unsigned long long v = a[i];
        a[i] = run;
        run += v;
    }
    if (tid == SP_NT - 1) a[n] = s[tid];
}

// a wave per row writes its pixels from the row's offset on, in column order (offsets null: every pixel, offset = row W)
template <typename T>
__global__ __launch_bounds__(64) void sp_points_kernel(const T* __restrict__ src, int64_t W, const unsigned long long* __restrict__ offsets,
                                                       double ta, double tc, double te, double tf, double* __restrict__ xs, double* __restrict__ ys,
                                                       T* __restrict__ zs) {
    const int64_t y = blockIdx.x;
    const T* row = src + (size_t)y * (size_t)W;
    size_t base = offsets ? (size_t)offsets[y] : (size_t)y * (size_t)W;
    const double ty = ((double)y + 0.5) * te, py = tf + ty;
    const int lane = threadIdx.x;
    for (int64_t x0 = 0; x0 < W; x0 += 64) {
        const int64_t x = x0 + lane;
        T v = (T)0;
        bool take = x < W;
        if (take) {
            v = row[x];
            if (offsets) take = fabs((double)v) < INFINITY;
        }
        const unsigned long long m = __ballot(take);
        if (take) {
            const size_t at = base + (size_t)__popcll(m & ((1ull << lane) - 1ull));
            const double tx = ((double)x + 0.5) * ta;
            xs[at] = tc + tx;
            ys[at] = py;
            zs[at] = v;
        }
        base += (size_t)__popcll(m);
    }
}

struct SpEvents {   // the five events around the four stages of a prepare
    hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    bool ok = true;
    SpEvents() {
        for (auto& e : ev)
            if (hipEventCreate(&e) != hipSuccess) { e = nullptr; ok = false; (void)hipGetLastError(); }
    }
    ~SpEvents() {
        for (auto& e : ev)
            if (e) (void)hipEventDestroy(e);
    }
    void mark(int k, hipStream_t s) { if (ok) (void)hipEventRecord(ev[k], s); }
};

int sp_fetch_count(xdemhip_ctx* ctx, const unsigned long long* d, int64_t* out) {
    unsigned long long v = 0;
    XD_HIP_CHECK(ctx, hipMemcpyAsync(&v, d, sizeof v, hipMemcpyDeviceToHost, ctx->stream));
    XD_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    *out = (int64_t)v;
    return XDEMHIP_OK;
}

inline unsigned sp_blocks(int64_t n) { return (unsigned)((n + SP_NT - 1) / SP_NT); }

// One line through the functions the kernels run, on the CPU (host only, no context): every pole of the order over `in` (n >= 2
// samples), the line cut into bands of `band` samples; two_phase != 0 walks each band as the LDS route does (a first walk that stores
// nothing, then the causal loop again from its warm state).
struct SpHostIn {
    const double* p;
    double gain;
    SP_HD double operator()(int64_t i) const { return p[i] * gain; }
};
struct SpHostOut {
    double* p;
    SP_HD double get(int64_t i) const { return p[i]; }
    SP_HD void put(int64_t i, double v) { p[i] = v; }
};

}  // namespace

struct xdemhip_spline {
    xdemhip_ctx* ctx = nullptr;
    XdOwned mem;
    int64_t H = 0, W = 0, n_nonfinite = 0;
    int order = 0, dist = 0, dtype = XDEMHIP_F32;
    const void* raster = nullptr;            // orders 0 and 1: what the taps read (the caller's device array, or an owned copy)
    const unsigned char* spread = nullptr;   // null: no void in the raster (or nothing but voids)
    const double* coef = nullptr;            // orders 3 and 5
    float stage_ms[4] = {0, 0, 0, 0};        // mask and fill, dilation, column passes, row passes
};

namespace {

template <typename T>
int sp_prepare(xdemhip_spline* S, const T* raster, int route_switch) {
    xdemhip_ctx* ctx = S->ctx;
    XdOwned& mem = S->mem;
    const int64_t H = S->H, W = S->W;
    const size_t n = (size_t)H * (size_t)W;
    const SpPlan plan = sp_plan(H, W, route_switch);
    SpEvents events;
    unsigned char* fin = mem.take<unsigned char>(n, "spline mask");
    unsigned long long* d_count = mem.take<unsigned long long>(1, "spline mask");
    if (mem.rc) return mem.rc;
    XD_HIP_CHECK(ctx, hipMemsetAsync(d_count, 0, sizeof(unsigned long long), ctx->stream));
    events.mark(0, ctx->stream);
    hipLaunchKernelGGL(sp_mask_kernel<T>, dim3(sp_blocks((int64_t)n)), dim3(SP_NT), 0, ctx->stream, raster, fin, (int64_t)n, d_count);
    int rc = launched(ctx, "spline mask kernel");
    if (rc == XDEMHIP_OK) rc = sp_fetch_count(ctx, d_count, &S->n_nonfinite);
    if (rc != XDEMHIP_OK) return rc;
    const bool voids = S->n_nonfinite > 0, all_nan = S->n_nonfinite == (int64_t)n;
    const bool filter = S->order > 1 && !all_nan;
    const T* filled = raster;
    T* fill_buf = nullptr;
    if (voids && filter) {
        int32_t* idx = mem.take<int32_t>(2 * n, "spline fill");
        fill_buf = mem.take<T>(n, "spline fill");
        if (mem.rc) return mem.rc;
        rc = xdemhip_edt(ctx, fin, H, W, 1.0, 1.0, nullptr, XDEMHIP_F64, idx, nullptr, 1, XDEMHIP_DEVICE, nullptr);
        if (rc != XDEMHIP_OK) return rc;
        hipLaunchKernelGGL(sp_fill_kernel<T>, dim3(sp_blocks((int64_t)n)), dim3(SP_NT), 0, ctx->stream, raster, fin, idx, fill_buf, (int64_t)n, W);
        if ((rc = launched(ctx, "spline fill kernel")) != XDEMHIP_OK) return rc;
        mem.drop(idx);
        filled = fill_buf;
    }
    events.mark(1, ctx->stream);
    if (voids && !all_nan) {
        const int64_t tx = (W + 63) / 64, ty = (H + SP_DIL_ROWS - 1) / SP_DIL_ROWS;
        unsigned char* a = mem.take<unsigned char>(n, "spline spread");
        unsigned char* b = S->dist > SP_DIL_R ? mem.take<unsigned char>(n, "spline spread") : nullptr;
        if (mem.rc) return mem.rc;
        const unsigned char* from = fin;
        unsigned char* to = a;
        int left = S->dist, invert = 1;
        do {   // (a diamond of r1 dilated by one of r2 is the diamond of r1 + r2)
            const int r = left < SP_DIL_R ? left : SP_DIL_R;
            hipLaunchKernelGGL(sp_dilate_kernel, dim3((unsigned)(tx * ty)), dim3(SP_NT), 0, ctx->stream, from, to, H, W, tx, r, invert);
            left -= r;
            invert = 0;
            from = to;
            to = to == a ? b : a;
        } while (left > 0);
        if ((rc = launched(ctx, "spline dilation kernel")) != XDEMHIP_OK) return rc;
        S->spread = from;
        if (b) mem.drop(from == a ? b : a);
    }
    events.mark(2, ctx->stream);
    double *pa = nullptr, *pb = nullptr;
    if (filter) {
        pa = mem.take<double>(n, "spline coefficients");
        pb = mem.take<double>(n, "spline coefficients");
        if (mem.rc) return mem.rc;
        double zs[2];
        const int np = sp_poles(S->order, zs);
        // columns: raster -> pa (-> pb); rows: -> the other plane each time; the last pass writes pb
        const int64_t nbands = (H + plan.band - 1) / plan.band;
        const dim3 col_grid(sp_blocks(W), (unsigned)nbands);
        hipLaunchKernelGGL(sp_col_kernel<T>, col_grid, dim3(SP_NT), 0, ctx->stream, filled, pa, H, W, plan.band, sp_pole(S->order, 0, H));
        const double* cur = pa;
        if (np == 2) {
            hipLaunchKernelGGL(sp_col_kernel<double>, col_grid, dim3(SP_NT), 0, ctx->stream, (const double*)pa, pb, H, W, plan.band, sp_pole(S->order, 1, H));
            cur = pb;
        }
        if ((rc = launched(ctx, "spline column kernel")) != XDEMHIP_OK) return rc;
        events.mark(3, ctx->stream);
        const int64_t tiles_x = (W + SP_TILE_COLS - 1) / SP_TILE_COLS, tiles_y = (H + SP_TILE_ROWS - 1) / SP_TILE_ROWS;
        if (plan.lds_rows)
            XD_HIP_CHECK(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(&sp_row_lds_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, SP_LDS_BYTES));
        for (int k = 0; k < np; ++k) {
            double* to = cur == pa ? pb : pa;
            const SpPole pole = sp_pole(S->order, k, W);
            if (plan.lds_rows)
                hipLaunchKernelGGL(sp_row_lds_kernel, dim3((unsigned)(tiles_x * tiles_y)), dim3(SP_NT), SP_LDS_BYTES, ctx->stream, cur, to, H, W, tiles_x, pole);
            else
                hipLaunchKernelGGL(sp_row_plain_kernel, dim3(sp_blocks(H)), dim3(SP_NT), 0, ctx->stream, cur, to, H, W, pole);
            cur = to;
        }
        if ((rc = launched(ctx, "spline row kernel")) != XDEMHIP_OK) return rc;
        S->coef = cur;
    } else {
        events.mark(3, ctx->stream);
    }
    events.mark(4, ctx->stream);
    XD_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    for (int k = 0; k < 4; ++k) {
        S->stage_ms[k] = 0.f;
        if (events.ok && hipEventElapsedTime(&S->stage_ms[k], events.ev[k], events.ev[k + 1]) != hipSuccess) {
            (void)hipGetLastError();
            S->stage_ms[k] = 0.f;
        }
    }
    // what only the prepare needed goes back now
    mem.drop(fin);
    mem.drop(d_count);
    if (fill_buf) mem.drop(fill_buf);
    if (filter) mem.drop(S->coef == pa ? pb : pa);
    if (S->order > 1) {
        mem.drop(raster);   // (an owned upload; a caller's device array is not owned and stays)
        S->raster = nullptr;
    }
    return XDEMHIP_OK;
}

// R: the raster's dtype; O: the result's (R, or float64: the value before its one rounding)
template <typename R, typename O>
int sp_gather(xdemhip_spline* S, const double* d_x, const double* d_y, void* d_out, int64_t n, const SpGeom& g, unsigned long long* d_count) {
    xdemhip_ctx* ctx = S->ctx;
    const dim3 grid(sp_blocks(n)), block(SP_NT);
    O* out = static_cast<O*>(d_out);
    const R* raster = static_cast<const R*>(S->raster);
    if (S->order == 0) hipLaunchKernelGGL((sp_gather_kernel<O, R, 0>), grid, block, 0, ctx->stream, raster, S->spread, d_x, d_y, out, n, g, d_count);
    else if (S->order == 1) hipLaunchKernelGGL((sp_gather_kernel<O, R, 1>), grid, block, 0, ctx->stream, raster, S->spread, d_x, d_y, out, n, g, d_count);
    else if (S->order == 3) hipLaunchKernelGGL((sp_gather_kernel<O, double, 3>), grid, block, 0, ctx->stream, S->coef, S->spread, d_x, d_y, out, n, g, d_count);
    else hipLaunchKernelGGL((sp_gather_kernel<O, double, 5>), grid, block, 0, ctx->stream, S->coef, S->spread, d_x, d_y, out, n, g, d_count);
    return launched(ctx, "spline gather kernel");
}

// per-row counts of finite pixels scanned into per-row offsets, the total behind them
template <typename T>
int sp_row_offsets(xdemhip_ctx* ctx, const T* d_src, int64_t H, int64_t W, unsigned long long* d_counts) {
    hipLaunchKernelGGL(sp_row_count_kernel<T>, dim3((unsigned)H), dim3(64), 0, ctx->stream, d_src, W, d_counts);
    hipLaunchKernelGGL(sp_scan_kernel, dim3(1), dim3(SP_NT), 0, ctx->stream, d_counts, H);
    return launched(ctx, "raster points count kernels");
}

}  // namespace

extern "C" {

int xdemhip_spline_plan(int64_t H, int64_t W, int order, int route_switch, int* band_rows, int* tile_rows, int* tile_cols, int* halo, int* lds_bytes) {
    const int64_t LIM = (int64_t)1 << 31;
    if (H < 2 || W < 2 || H >= LIM || W >= LIM || route_switch < 0 || route_switch > 3) return XDEMHIP_EINVAL;
    if (order != 0 && order != 1 && order != 3 && order != 5) return XDEMHIP_EINVAL;
    const SpPlan p = sp_plan(H, W, route_switch);
    if (band_rows) *band_rows = p.band;
    if (tile_rows) *tile_rows = p.tile_rows;
    if (tile_cols) *tile_cols = p.tile_cols;
    if (halo) *halo = p.halo;
    if (lds_bytes) *lds_bytes = p.lds_bytes;
    return XDEMHIP_OK;
}

int xdemhip_spline_host_line(const double* in, int64_t n, int order, int64_t band, int two_phase, double* out) {
    if (!in || !out || n < 2 || band < 1 || (order != 3 && order != 5)) return XDEMHIP_EINVAL;
    std::vector<double> a(in, in + n), b((size_t)n);
    double zs[2];
    const int np = sp_poles(order, zs);
    for (int k = 0; k < np; ++k) {
        const SpPole p = sp_pole(order, k, n);
        const SpHostIn src{a.data(), p.gain};
        SpHostOut dst{b.data()};
        for (int64_t y0 = 0; y0 < n; y0 += band) {
            const int64_t y1 = y0 + band < n ? y0 + band : n;
            SpWarm warm;
            double cm;
            bool last;
            if (two_phase) {
                sp_forward<false>(src, dst, n, y0, y1, p, warm, cm, last);
                sp_replay(src, dst, y0, y1, p, warm);
            } else {
                sp_forward<true>(src, dst, n, y0, y1, p, warm, cm, last);
            }
            sp_backward(dst, y0, y1, cm, last, p.z);
        }
        a.swap(b);
    }
    for (int64_t i = 0; i < n; ++i) out[i] = a[(size_t)i];
    return XDEMHIP_OK;
}

void xdemhip_spline_destroy(xdemhip_spline* S) { delete S; }

int xdemhip_spline_prepare(xdemhip_ctx* ctx, const void* raster, int dtype, int64_t H, int64_t W, int order, int dist, int memspace,
                           xdemhip_spline** out, int64_t* n_nonfinite) {
    if (!ctx) return XDEMHIP_EINVAL;
    if (!raster || !out) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_spline_prepare: null argument");
    const int64_t LIM = (int64_t)1 << 31;
    if (H < 2 || W < 2 || H >= LIM || W >= LIM) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_spline_prepare: raster sides must be 2 .. 2^31 - 1 (axes of length 1 are refused)");
    if (order != 0 && order != 1 && order != 3 && order != 5) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_spline_prepare: order must be 0, 1, 3 or 5");
    if (dist < 0) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_spline_prepare: dist must be >= 0");
    if (dtype != XDEMHIP_F32 && dtype != XDEMHIP_F64) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_spline_prepare: dtype must be XDEMHIP_F32 or XDEMHIP_F64");
    if (memspace != XDEMHIP_HOST && memspace != XDEMHIP_DEVICE) return xd_fail(ctx, XDEMHIP_EINVAL, "memspace must be XDEMHIP_HOST or XDEMHIP_DEVICE");
    const int64_t dil_blocks = ((W + 63) / 64) * ((H + SP_DIL_ROWS - 1) / SP_DIL_ROWS);
    const int64_t row_blocks = ((W + SP_TILE_COLS - 1) / SP_TILE_COLS) * ((H + SP_TILE_ROWS - 1) / SP_TILE_ROWS);
    if (dil_blocks >= LIM || row_blocks >= LIM || (H * W + SP_NT - 1) / SP_NT >= LIM || (H + SP_BAND - 1) / SP_BAND > 65535)
        return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_spline_prepare: raster too large for one launch");
    XD_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    xdemhip_spline* S = new xdemhip_spline();
    S->ctx = S->mem.ctx = ctx;
    S->H = H; S->W = W; S->order = order; S->dist = dist; S->dtype = dtype;
    const size_t bytes = (size_t)H * (size_t)W * (dtype == XDEMHIP_F32 ? 4 : 8);
    S->raster = S->mem.keep(static_cast<const unsigned char*>(raster), bytes, memspace, "spline raster");
    int rc = S->mem.rc;
    if (rc == XDEMHIP_OK)
        rc = dtype == XDEMHIP_F32 ? sp_prepare<float>(S, static_cast<const float*>(S->raster), ctx->spline_route)
                                  : sp_prepare<double>(S, static_cast<const double*>(S->raster), ctx->spline_route);
    if (rc != XDEMHIP_OK) {
        delete S;
        return rc;
    }
    if (n_nonfinite) *n_nonfinite = S->n_nonfinite;
    *out = S;
    return XDEMHIP_OK;
}

int xdemhip_spline_stage_ms(xdemhip_spline* S, float* ms) {
    if (!S || !ms) return XDEMHIP_EINVAL;
    for (int k = 0; k < 4; ++k) ms[k] = S->stage_ms[k];
    return XDEMHIP_OK;
}

int xdemhip_spline_planes(xdemhip_spline* S, unsigned char* spread, double* coef, int memspace) {
    if (!S) return XDEMHIP_EINVAL;
    xdemhip_ctx* ctx = S->ctx;
    if ((spread && !S->spread) || (coef && !S->coef)) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_spline_planes: the plan holds no such plane");
    if (memspace != XDEMHIP_HOST && memspace != XDEMHIP_DEVICE) return xd_fail(ctx, XDEMHIP_EINVAL, "memspace must be XDEMHIP_HOST or XDEMHIP_DEVICE");
    XD_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    const size_t n = (size_t)S->H * (size_t)S->W;
    const hipMemcpyKind kind = memspace == XDEMHIP_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    if (spread) XD_HIP_CHECK(ctx, hipMemcpyAsync(spread, S->spread, n, kind, ctx->stream));
    if (coef) XD_HIP_CHECK(ctx, hipMemcpyAsync(coef, S->coef, n * sizeof(double), kind, ctx->stream));
    XD_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return XDEMHIP_OK;
}

int xdemhip_spline_gather(xdemhip_spline* S, const double* x, const double* y, int64_t n, const double* transform6, int shift, void* out,
                          int out_dtype, int memspace, int64_t* n_valid) {
    if (!S) return XDEMHIP_EINVAL;
    xdemhip_ctx* ctx = S->ctx;
    if (n < 0 || !transform6 || (n > 0 && (!x || !y || !out))) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_spline_gather: null argument or n < 0");
    if (transform6[1] != 0.0 || transform6[3] != 0.0 || transform6[0] == 0.0 || transform6[4] == 0.0)
        return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_spline_gather: only north-up transforms (b = d = 0, a and e non-zero)");
    if (out_dtype != XDEMHIP_F64 && out_dtype != S->dtype) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_spline_gather: out_dtype must be the raster's dtype or XDEMHIP_F64");
    if (memspace != XDEMHIP_HOST && memspace != XDEMHIP_DEVICE) return xd_fail(ctx, XDEMHIP_EINVAL, "memspace must be XDEMHIP_HOST or XDEMHIP_DEVICE");
    if ((n + SP_NT - 1) / SP_NT >= ((int64_t)1 << 31)) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_spline_gather: too many points for one launch");
    if (n_valid) *n_valid = 0;
    if (n == 0) return XDEMHIP_OK;
    SpGeom g;
    g.H = S->H; g.W = S->W;
    g.a = transform6[0]; g.c = transform6[2]; g.e = transform6[4]; g.f = transform6[5];
    g.half = shift ? 0.0 : 0.5;
    g.all_nan = S->n_nonfinite == S->H * S->W;
    XD_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    const size_t size = out_dtype == XDEMHIP_F32 ? 4 : 8;
    XdBuffers buf(ctx, "xdemhip_spline_gather");
    const double* d_x = buf.input(x, (size_t)n * 8, memspace);
    const double* d_y = buf.input(y, (size_t)n * 8, memspace);
    void* d_out = buf.output(out, (size_t)n * size, memspace);
    unsigned long long* d_count = buf.alloc<unsigned long long>(1);
    if (buf.rc) return buf.rc;
    XD_HIP_CHECK(ctx, hipMemsetAsync(d_count, 0, sizeof(unsigned long long), ctx->stream));
    XD_HIP_CHECK(ctx, hipEventRecord(ctx->ev_start, ctx->stream));
    int rc = out_dtype == XDEMHIP_F32 ? sp_gather<float, float>(S, d_x, d_y, d_out, n, g, d_count)
             : S->dtype == XDEMHIP_F32 ? sp_gather<float, double>(S, d_x, d_y, d_out, n, g, d_count)
                                       : sp_gather<double, double>(S, d_x, d_y, d_out, n, g, d_count);
    (void)hipEventRecord(ctx->ev_stop, ctx->stream);
    ctx->timed = true;
    int64_t valid = 0;
    if (rc == XDEMHIP_OK) rc = sp_fetch_count(ctx, d_count, &valid);
    if (rc == XDEMHIP_OK) rc = buf.finish();
    if (rc == XDEMHIP_OK && n_valid) *n_valid = valid;
    return rc;
}

int xdemhip_raster_points(xdemhip_ctx* ctx, const void* raster, int dtype, int64_t H, int64_t W, const double* transform6, int skip_nodata,
                          double* x, double* y, void* z, int64_t capacity, int memspace, int64_t* count) {
    if (!ctx) return XDEMHIP_EINVAL;
    if (!raster || !transform6 || !count) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_raster_points: null argument");
    const int64_t LIM = (int64_t)1 << 31;
    if (H < 1 || W < 1 || H >= LIM || W >= LIM) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_raster_points: raster sides must be 1 .. 2^31 - 1");
    if (dtype != XDEMHIP_F32 && dtype != XDEMHIP_F64) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_raster_points: dtype must be XDEMHIP_F32 or XDEMHIP_F64");
    if (transform6[1] != 0.0 || transform6[3] != 0.0) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_raster_points: only north-up transforms (b = d = 0)");
    if (memspace != XDEMHIP_HOST && memspace != XDEMHIP_DEVICE) return xd_fail(ctx, XDEMHIP_EINVAL, "memspace must be XDEMHIP_HOST or XDEMHIP_DEVICE");
    const bool count_only = !x && !y && !z;
    if (!count_only && (!x || !y || !z)) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_raster_points: x, y and z together, or none of them");
    if (!skip_nodata) {
        *count = H * W;
        if (count_only) return XDEMHIP_OK;
        if (capacity < H * W) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_raster_points: capacity below the number of pixels");
    }
    XD_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    const size_t size = dtype == XDEMHIP_F32 ? 4 : 8, n = (size_t)H * (size_t)W;
    XdBuffers buf(ctx, "xdemhip_raster_points");
    const void* d_src = buf.input(static_cast<const unsigned char*>(raster), n * size, memspace);
    unsigned long long* d_counts = skip_nodata ? buf.alloc<unsigned long long>((size_t)H + 1) : nullptr;
    if (buf.rc) return buf.rc;
    int rc = XDEMHIP_OK;
    int64_t total = H * W;
    if (skip_nodata) {
        rc = dtype == XDEMHIP_F32 ? sp_row_offsets<float>(ctx, static_cast<const float*>(d_src), H, W, d_counts)
                                  : sp_row_offsets<double>(ctx, static_cast<const double*>(d_src), H, W, d_counts);
        if (rc == XDEMHIP_OK) rc = sp_fetch_count(ctx, d_counts + H, &total);
        if (rc != XDEMHIP_OK) return rc;
        *count = total;
        if (count_only) return buf.finish();
        if (capacity < total) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_raster_points: capacity below the number of finite pixels");
    }
    if (total == 0) return buf.finish();
    double* d_x = buf.output(x, (size_t)total * 8, memspace);
    double* d_y = buf.output(y, (size_t)total * 8, memspace);
    void* d_z = buf.output(static_cast<unsigned char*>(z), (size_t)total * size, memspace);
    if (buf.rc) return buf.rc;
    // (the offsets are in place already: only the write pass runs)
    if (dtype == XDEMHIP_F32)
        hipLaunchKernelGGL(sp_points_kernel<float>, dim3((unsigned)H), dim3(64), 0, ctx->stream, static_cast<const float*>(d_src), W,
                           (const unsigned long long*)d_counts, transform6[0], transform6[2], transform6[4], transform6[5], d_x, d_y, static_cast<float*>(d_z));
    else
        hipLaunchKernelGGL(sp_points_kernel<double>, dim3((unsigned)H), dim3(64), 0, ctx->stream, static_cast<const double*>(d_src), W,
                           (const unsigned long long*)d_counts, transform6[0], transform6[2], transform6[4], transform6[5], d_x, d_y, static_cast<double*>(d_z));
    rc = launched(ctx, "raster points kernel");
    if (rc == XDEMHIP_OK) rc = buf.finish();
    if (rc == XDEMHIP_OK) rc = xd_sync(ctx);   // (device columns: the scope owned nothing and has not waited)
    return rc;
}

}  // extern "C"
