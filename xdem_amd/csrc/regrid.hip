// regrid.hip -- xdemhip_regrid: a raster resampled onto another north-up grid of the same CRS (geoutils' Raster.reproject for the
// same-CRS case; DESIGN.md "Regridding" has the rule, INTEGRATION.md what of it is pinned).  All arithmetic of the rule is float64 in
// the order the rule is written (the Makefile builds this file with -ffp-contract=off); tests/reproject_oracle.py restates it in NumPy
// and every route below returns its bits.
//
//   axis      r = a_d / a_s, t = (c_d - c_s) / a_s (the caller's map4); centre of destination pixel o in source pixels u = (o + 0.5) r + t
//   taps      s = min(1, 1 / r), Re = R / s, K = floor(2 Re) + 1, first tap i0 = ceil(u - 0.5 - Re), weight of tap i0 + m = k((i0 + m + 0.5 - u) s)
//   value     rows j, then columns i: a tap inside the source and finite adds ww = wy[j] wx[i] to den and ww v to num (both from +0.0);
//             the pixel is (dtype)(num / den) iff 0 <= ux < W, 0 <= uy < H and den > REGRID_MIN_DEN, else NaN.  (A tap whose wy[j] or wx[i]
//             is exactly zero adds +-0.0 to sums that are never -0.0: the kernels leave it out, which returns the same bits -- for scales
//             <= 1 that is one of the K = 2 R + 1 taps per axis, 5 of bilinear's 9.)
//   nearest   i = floor(u + 1e-10) per axis, the source value copied iff 0 <= i < n, else NaN (0 for uint8)
//
// Routes (the same bits from each):
//   tile      a workgroup of 256 threads owns REGRID_TW x REGRID_TH destination pixels, stages their source footprint (kernel radius
//             included, clipped to the source) and the per-column / per-row first taps and weights in LDS, and runs the double sum from
//             there.  Taken while the footprint and the tables fit REGRID_LDS_BUDGET bytes (regrid_tile_bytes): every upsampling, scales
//             near 1, moderate downsampling.
//   direct    one thread per destination pixel, taps from global memory, weights formed as they are used: strong downsampling.
//   nearest   a plain gather.
// The count of non-NaN destination pixels is summed in the same pass: a shuffle sum per wave and one integer atomic per workgroup,
// spread over REGRID_SLOTS counters a cache line apart (a single counter would serialise a million workgroups); the host adds them.
#include "common.h"
#include "../../include/xdemhip_test.h"

#include <math.h>

namespace {

constexpr double REGRID_MIN_DEN = 1e-5;    // the divisor threshold of the rule
constexpr double REGRID_NEAREST_EPS = 1e-10;
constexpr int REGRID_TW = 64, REGRID_TH = 16, REGRID_NT = 256;   // a tile: 64 lanes along a row, 4 waves, 4 rows per thread
constexpr int64_t REGRID_LDS_BUDGET = 63 * 1024;                 // bytes of dynamic LDS one workgroup of the tile route may ask for (64 KiB less its static words)
constexpr int64_t REGRID_MAX_TAPS = (int64_t)1 << 24;            // Kx * Ky of the direct route: beyond it the call is refused
constexpr int REGRID_KREG = 5;                                   // taps along x whose weights a thread of the tile route keeps in registers (2 R + 1 of the cubics)
constexpr int REGRID_SLOTS = 1024, REGRID_SLOT_STRIDE = 16;      // counters of the valid count: 1024, 128 bytes apart
constexpr double REGRID_FAR = 4e15;                              // first taps are clamped to +-this before they become integers

struct RegridAxis {
    double r, t, s, Re;
    int K;
};

struct RegridGeom {
    int64_t H, W, h, w;
    RegridAxis x, y;
    int kernel;
    int fw_cap, fh_cap;   // tile route: the footprint a workgroup may stage
};

__host__ __device__ inline double regrid_weight(int kernel, double d) {
    const double a = fabs(d);
    if (kernel == XDEMHIP_REGRID_BILINEAR) return a < 1.0 ? 1.0 - a : 0.0;
    if (kernel == XDEMHIP_REGRID_CUBIC) {
        if (a <= 1.0) return (1.5 * a - 2.5) * a * a + 1.0;
        if (a < 2.0) return ((-0.5 * a + 2.5) * a - 4.0) * a + 2.0;
        return 0.0;
    }
    if (a <= 1.0) return (0.5 * a - 1.0) * a * a + 2.0 / 3.0;
    if (a < 2.0) return ((2.0 - a) * (2.0 - a)) * (2.0 - a) / 6.0;
    return 0.0;
}

__host__ __device__ inline double regrid_centre(const RegridAxis& A, int64_t o) { return ((double)o + 0.5) * A.r + A.t; }

// the first tap of a pixel centred on u, as an integer that later sums cannot overflow
__host__ __device__ inline int64_t regrid_first_tap(const RegridAxis& A, double u) {
    double d = ceil(u - 0.5 - A.Re);
    d = d > -REGRID_FAR ? d : -REGRID_FAR;   // (NaN goes to -REGRID_FAR too)
    d = d < REGRID_FAR ? d : REGRID_FAR;
    return (int64_t)d;
}

__host__ __device__ inline bool regrid_inside(double u, int64_t n) { return u >= 0.0 && u < (double)n; }

inline RegridAxis regrid_axis(double r, double t, int kernel) {
    RegridAxis A;
    const double R = kernel == XDEMHIP_REGRID_BILINEAR ? 1.0 : 2.0;
    A.r = r;
    A.t = t;
    A.s = 1.0 / r < 1.0 ? 1.0 / r : 1.0;
    A.Re = R / A.s;
    const double k = floor(2.0 * A.Re) + 1.0;
    A.K = k < 2147483647.0 ? (int)k : 2147483647;
    return A;
}

// Source pixels along one axis that `n_tile` neighbouring destination pixels can touch: their first taps lie at most
// ceil((n_tile - 1) r) + 1 apart (the + 1: two ceilings), each has K taps, and one more pixel absorbs the rounding of u.
inline int64_t regrid_footprint(const RegridAxis& A, int n_tile) {
    const double span = ceil((double)(n_tile - 1) * A.r);
    if (!(span < 1e9)) return (int64_t)1 << 40;
    return (int64_t)span + A.K + 2;
}

// LDS bytes of a workgroup of the tile route: the footprint in the source dtype, the weights (float64) and the first taps and
// inside flags (int32) of its columns and rows.
inline int64_t regrid_tile_bytes(const RegridAxis& X, const RegridAxis& Y, int src_size, int64_t* fw, int64_t* fh) {
    *fw = regrid_footprint(X, REGRID_TW);
    *fh = regrid_footprint(Y, REGRID_TH);
    if (*fw > 1 << 20 || *fh > 1 << 20) return (int64_t)1 << 50;
    const int64_t tables = (int64_t)REGRID_TW * (X.K * 8 + 8) + (int64_t)REGRID_TH * (Y.K * 8 + 8);
    const int64_t tile = ((*fw * *fh * src_size + 15) / 16) * 16;
    return tables + tile;
}

template <typename T> __device__ inline T regrid_nan();
template <> __device__ inline float regrid_nan<float>() { return __builtin_nanf(""); }
template <> __device__ inline double regrid_nan<double>() { return __builtin_nan(""); }
template <> __device__ inline unsigned char regrid_nan<unsigned char>() { return 0; }

// `landed` of the calling thread's pixels summed over the workgroup into the workgroup's counter: one atomic per workgroup
__device__ inline void regrid_count(int landed, int* wave_sums, unsigned long long* count) {
    for (int off = 32; off > 0; off >>= 1) landed += __shfl_down(landed, off, 64);
    const int tid = threadIdx.x, wave = tid >> 6;
    if ((tid & 63) == 0) wave_sums[wave] = landed;
    __syncthreads();
    if (tid == 0) {
        int total = 0;
        for (int k = 0; k < REGRID_NT / 64; ++k) total += wave_sums[k];
        if (total) atomicAdd(count + (size_t)(blockIdx.x % REGRID_SLOTS) * REGRID_SLOT_STRIDE, (unsigned long long)total);
    }
}

// ---- tile route -------------------------------------------------------------------------------------------------------------------
// LDS layout (dynamic, 16-byte aligned): wx[Kx][TW] | wy[Ky][TH] (float64) | x0[TW] okx[TW] y0[TH] oky[TH] (int32) | tile[fh][fw] (Ts)
template <typename Ts, typename Td>
__global__ __launch_bounds__(REGRID_NT) void regrid_tile_kernel(const Ts* __restrict__ src, Td* __restrict__ dst, RegridGeom g, int64_t tiles_x,
                                                                unsigned long long* count) {
    extern __shared__ __attribute__((aligned(16))) unsigned char regrid_lds[];
    __shared__ int wave_sums[REGRID_NT / 64];
    const int Kx = g.x.K, Ky = g.y.K;
    double* wx = reinterpret_cast<double*>(regrid_lds);
    double* wy = wx + (size_t)Kx * REGRID_TW;
    int* x0 = reinterpret_cast<int*>(wy + (size_t)Ky * REGRID_TH);
    int* okx = x0 + REGRID_TW;
    int* y0 = okx + REGRID_TW;
    int* oky = y0 + REGRID_TH;
    Ts* tile = reinterpret_cast<Ts*>(oky + REGRID_TH);

    const int tid = threadIdx.x;
    const int64_t by = (int64_t)blockIdx.x / tiles_x, bx = (int64_t)blockIdx.x - by * tiles_x;
    const int64_t ox0 = bx * REGRID_TW, oy0 = by * REGRID_TH;
    const int64_t ox1 = ox0 + REGRID_TW - 1 < g.w - 1 ? ox0 + REGRID_TW - 1 : g.w - 1;
    const int64_t oy1 = oy0 + REGRID_TH - 1 < g.h - 1 ? oy0 + REGRID_TH - 1 : g.h - 1;
    // the footprint: from the first tap of the first pixel to the last tap of the last, clipped to the source and to what was asked for
    int64_t lo_x = regrid_first_tap(g.x, regrid_centre(g.x, ox0)), hi_x = regrid_first_tap(g.x, regrid_centre(g.x, ox1)) + Kx - 1;
    int64_t lo_y = regrid_first_tap(g.y, regrid_centre(g.y, oy0)), hi_y = regrid_first_tap(g.y, regrid_centre(g.y, oy1)) + Ky - 1;
    lo_x = lo_x > 0 ? lo_x : 0;
    lo_y = lo_y > 0 ? lo_y : 0;
    hi_x = hi_x < g.W - 1 ? hi_x : g.W - 1;
    hi_y = hi_y < g.H - 1 ? hi_y : g.H - 1;
    hi_x = hi_x < lo_x + g.fw_cap - 1 ? hi_x : lo_x + g.fw_cap - 1;
    hi_y = hi_y < lo_y + g.fh_cap - 1 ? hi_y : lo_y + g.fh_cap - 1;
    const int fw = hi_x >= lo_x ? (int)(hi_x - lo_x + 1) : 0, fh = hi_y >= lo_y ? (int)(hi_y - lo_y + 1) : 0;

    // the tables: one thread per column of the tile, one per row
    if (tid < REGRID_TW + REGRID_TH) {
        const bool col = tid < REGRID_TW;
        const int l = col ? tid : tid - REGRID_TW;
        const RegridAxis& A = col ? g.x : g.y;
        const int64_t o = (col ? ox0 : oy0) + l, n_dst = col ? g.w : g.h, n_src = col ? g.W : g.H, lo = col ? lo_x : lo_y;
        const int K = col ? Kx : Ky, stride = col ? REGRID_TW : REGRID_TH;
        double* wt = col ? wx : wy;
        int first = 0, ok = 0;
        if (o < n_dst) {
            const double u = regrid_centre(A, o);
            const int64_t i0 = regrid_first_tap(A, u);
            int64_t rel = i0 - lo;
            rel = rel > -(1 << 30) ? rel : -(1 << 30);
            rel = rel < (1 << 30) ? rel : (1 << 30);
            first = (int)rel;
            ok = regrid_inside(u, n_src);
            for (int m = 0; m < K; ++m) wt[(size_t)m * stride + l] = regrid_weight(g.kernel, ((double)(i0 + m) + 0.5 - u) * A.s);
        } else {
            for (int m = 0; m < K; ++m) wt[(size_t)m * stride + l] = 0.0;
        }
        (col ? x0 : y0)[l] = first;
        (col ? okx : oky)[l] = ok;
    }
    // the footprint: a wave per row, its lanes along the row
    if (fw > 0)
        for (int r = tid >> 6; r < fh; r += REGRID_NT / 64) {
            const Ts* row = src + (size_t)(lo_y + r) * (size_t)g.W + (size_t)lo_x;
            for (int c = tid & 63; c < fw; c += 64) tile[(size_t)r * fw + c] = row[c];
        }
    __syncthreads();

    const int lx = tid & 63, ly = tid >> 6;
    const int64_t ox = ox0 + lx;
    int landed = 0;
    if (ox < g.w) {
        const int cx0 = x0[lx], in_x = okx[lx];
        // A column's weights are the same for the thread's four rows.  With K <= REGRID_KREG taps along x (every scale <= 1) they are
        // held in registers with a mask of the taps that count (inside the staged rectangle, weight not zero), and the loop along x is
        // unrolled; longer rows of taps read their weights from LDS tap by tap.  The same sums in the same order.
        double wreg[REGRID_KREG];
        unsigned live = 0;
        const bool in_regs = Kx <= REGRID_KREG;
#pragma unroll
        for (int i = 0; i < REGRID_KREG; ++i) {
            wreg[i] = in_regs && i < Kx ? wx[i * REGRID_TW + lx] : 0.0;
            if (wreg[i] != 0.0 && (unsigned)(cx0 + i) < (unsigned)fw) live |= 1u << i;
        }
        for (int k = 0; k < REGRID_TH / (REGRID_NT / 64); ++k) {
            const int row_l = ly + k * (REGRID_NT / 64);
            const int64_t oy = oy0 + row_l;
            if (oy >= g.h) break;
            Td out = regrid_nan<Td>();
            if (in_x && oky[row_l]) {
                const int ry0 = y0[row_l];
                double num = 0.0, den = 0.0;
                for (int j = 0; j < Ky; ++j) {
                    const int ry = ry0 + j;
                    if ((unsigned)ry >= (unsigned)fh) continue;
                    const double wyj = wy[j * REGRID_TH + row_l];
                    if (wyj == 0.0) continue;   // (a tap of weight zero adds +-0 to both sums: leaving it out returns the same bits)
                    const Ts* trow = tile + (size_t)ry * fw;
                    if (in_regs) {
#pragma unroll
                        for (int i = 0; i < REGRID_KREG; ++i) {
                            if (!((live >> i) & 1u)) continue;
                            const double v = (double)trow[cx0 + i];
                            if (!(fabs(v) < INFINITY)) continue;
                            const double ww = wyj * wreg[i];
                            den += ww;
                            num += ww * v;
                        }
                        continue;
                    }
                    for (int i = 0; i < Kx; ++i) {
                        const int cx = cx0 + i;
                        if ((unsigned)cx >= (unsigned)fw) continue;
                        const double wxi = wx[i * REGRID_TW + lx];
                        if (wxi == 0.0) continue;
                        const double v = (double)trow[cx];
                        if (!(fabs(v) < INFINITY)) continue;
                        const double ww = wyj * wxi;
                        den += ww;
                        num += ww * v;
                    }
                }
                if (den > REGRID_MIN_DEN) out = (Td)(num / den);
            }
            dst[(size_t)oy * (size_t)g.w + (size_t)ox] = out;
            landed += out == out;
        }
    }
    regrid_count(landed, wave_sums, count);
}

// ---- direct route -----------------------------------------------------------------------------------------------------------------
template <typename Ts, typename Td>
__global__ __launch_bounds__(REGRID_NT) void regrid_direct_kernel(const Ts* __restrict__ src, Td* __restrict__ dst, RegridGeom g, int64_t tiles_x,
                                                                  unsigned long long* count) {
    __shared__ int wave_sums[REGRID_NT / 64];
    const int tid = threadIdx.x;
    const int64_t by = (int64_t)blockIdx.x / tiles_x, bx = (int64_t)blockIdx.x - by * tiles_x;
    const int64_t ox = bx * 64 + (tid & 63), oy = by * (REGRID_NT / 64) + (tid >> 6);
    int landed = 0;
    if (ox < g.w && oy < g.h) {
        const double ux = regrid_centre(g.x, ox), uy = regrid_centre(g.y, oy);
        Td out = regrid_nan<Td>();
        if (regrid_inside(ux, g.W) && regrid_inside(uy, g.H)) {
            const int64_t ix0 = regrid_first_tap(g.x, ux), iy0 = regrid_first_tap(g.y, uy);
            double num = 0.0, den = 0.0;
            for (int j = 0; j < g.y.K; ++j) {
                const int64_t ry = iy0 + j;
                if (ry < 0 || ry >= g.H) continue;
                const double wyj = regrid_weight(g.kernel, ((double)ry + 0.5 - uy) * g.y.s);
                if (wyj == 0.0) continue;   // (as in the tile route: a tap of weight zero changes neither sum)
                const Ts* row = src + (size_t)ry * (size_t)g.W;
                for (int i = 0; i < g.x.K; ++i) {
                    const int64_t cx = ix0 + i;
                    if (cx < 0 || cx >= g.W) continue;
                    const double wxi = regrid_weight(g.kernel, ((double)cx + 0.5 - ux) * g.x.s);
                    if (wxi == 0.0) continue;
                    const double v = (double)row[cx];
                    if (!(fabs(v) < INFINITY)) continue;
                    const double ww = wyj * wxi;
                    den += ww;
                    num += ww * v;
                }
            }
            if (den > REGRID_MIN_DEN) out = (Td)(num / den);
        }
        dst[(size_t)oy * (size_t)g.w + (size_t)ox] = out;
        landed = out == out;
    }
    regrid_count(landed, wave_sums, count);
}

// ---- nearest ----------------------------------------------------------------------------------------------------------------------
template <typename Ts, typename Td>
__global__ __launch_bounds__(REGRID_NT) void regrid_nearest_kernel(const Ts* __restrict__ src, Td* __restrict__ dst, RegridGeom g, int64_t tiles_x,
                                                                   unsigned long long* count) {
    __shared__ int wave_sums[REGRID_NT / 64];
    const int tid = threadIdx.x;
    const int64_t by = (int64_t)blockIdx.x / tiles_x, bx = (int64_t)blockIdx.x - by * tiles_x;
    const int64_t ox = bx * 64 + (tid & 63), oy = by * (REGRID_NT / 64) + (tid >> 6);
    int landed = 0;
    if (ox < g.w && oy < g.h) {
        const double fx = floor(regrid_centre(g.x, ox) + REGRID_NEAREST_EPS), fy = floor(regrid_centre(g.y, oy) + REGRID_NEAREST_EPS);
        Td out = regrid_nan<Td>();
        if (fx >= 0.0 && fx < (double)g.W && fy >= 0.0 && fy < (double)g.H) {
            out = (Td)src[(size_t)(int64_t)fy * (size_t)g.W + (size_t)(int64_t)fx];
            landed = sizeof(Td) == 1 ? 1 : out == out;   // (uint8 has no NaN: a pixel counts if it was taken from the source)
        }
        dst[(size_t)oy * (size_t)g.w + (size_t)ox] = out;
    }
    regrid_count(landed, wave_sums, count);
}

// The route a call takes: XDEMHIP_REGRID_ROUTE_* (nearest has one).  `route_switch`: the "regrid_route" test switch.
int regrid_choose(const RegridAxis& X, const RegridAxis& Y, int kernel, int src_size, int route_switch, int64_t* lds_bytes, int64_t* fw, int64_t* fh) {
    *lds_bytes = 0;
    *fw = *fh = 0;
    if (kernel == XDEMHIP_REGRID_NEAREST) return XDEMHIP_REGRID_ROUTE_NEAREST;
    *lds_bytes = regrid_tile_bytes(X, Y, src_size, fw, fh);
    if (route_switch == 2) return XDEMHIP_REGRID_ROUTE_DIRECT;
    return *lds_bytes <= REGRID_LDS_BUDGET ? XDEMHIP_REGRID_ROUTE_TILE : XDEMHIP_REGRID_ROUTE_DIRECT;
}

bool regrid_map_ok(const double* m) {
    for (int k = 0; k < 4; ++k)
        if (!(fabs(m[k]) < INFINITY)) return false;
    return m[0] > 0.0 && m[2] > 0.0;
}

template <typename Ts, typename Td>
void regrid_launch(xdemhip_ctx* ctx, int route, const void* src, void* dst, const RegridGeom& g, int64_t lds_bytes, unsigned long long* count) {
    const Ts* s = static_cast<const Ts*>(src);
    Td* d = static_cast<Td*>(dst);
    const int64_t tiles_x = (g.w + 63) / 64;
    const int64_t blocks = tiles_x * ((g.h + REGRID_NT / 64 - 1) / (REGRID_NT / 64));
    if constexpr (sizeof(Td) > 1) {   // (uint8 rasters reach the nearest kernel only)
        if (route == XDEMHIP_REGRID_ROUTE_TILE) {
            const int64_t tiles = tiles_x * ((g.h + REGRID_TH - 1) / REGRID_TH);
            hipLaunchKernelGGL((regrid_tile_kernel<Ts, Td>), dim3((unsigned)tiles), dim3(REGRID_NT), (size_t)lds_bytes, ctx->stream, s, d, g, tiles_x, count);
            return;
        }
        if (route == XDEMHIP_REGRID_ROUTE_DIRECT) {
            hipLaunchKernelGGL((regrid_direct_kernel<Ts, Td>), dim3((unsigned)blocks), dim3(REGRID_NT), 0, ctx->stream, s, d, g, tiles_x, count);
            return;
        }
    }
    hipLaunchKernelGGL((regrid_nearest_kernel<Ts, Td>), dim3((unsigned)blocks), dim3(REGRID_NT), 0, ctx->stream, s, d, g, tiles_x, count);
}

}  // namespace

extern "C" {

int xdemhip_regrid_route(const double* map4, int kernel, int src_dtype, int route_switch, int* route, int64_t* lds_bytes, int64_t* lds_budget) {
    if (!map4 || !route || !regrid_map_ok(map4)) return XDEMHIP_EINVAL;
    if (kernel < XDEMHIP_REGRID_NEAREST || kernel > XDEMHIP_REGRID_CUBIC_SPLINE || route_switch < 0 || route_switch > 2) return XDEMHIP_EINVAL;
    if (src_dtype != XDEMHIP_F32 && src_dtype != XDEMHIP_F64 && src_dtype != XDEMHIP_U8) return XDEMHIP_EINVAL;
    const RegridAxis X = regrid_axis(map4[0], map4[1], kernel), Y = regrid_axis(map4[2], map4[3], kernel);
    int64_t bytes = 0, fw = 0, fh = 0;
    *route = regrid_choose(X, Y, kernel, src_dtype == XDEMHIP_F32 ? 4 : (src_dtype == XDEMHIP_F64 ? 8 : 1), route_switch, &bytes, &fw, &fh);
    if (lds_bytes) *lds_bytes = bytes;
    if (lds_budget) *lds_budget = REGRID_LDS_BUDGET;
    return XDEMHIP_OK;
}

int xdemhip_regrid(xdemhip_ctx* ctx, const void* src, int src_dtype, int64_t H, int64_t W, void* dst, int dst_dtype, int64_t h, int64_t w,
                   const double* map4, int kernel, int memspace, int64_t* valid_count) {
    if (!ctx) return XDEMHIP_EINVAL;
    if (!src || !dst || !map4 || !valid_count) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_regrid: null argument");
    const int64_t LIM = (int64_t)1 << 31;
    if (H < 1 || W < 1 || h < 1 || w < 1 || H >= LIM || W >= LIM || h >= LIM || w >= LIM)
        return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_regrid: raster sides must be 1 .. 2^31 - 1");
    if (memspace != XDEMHIP_HOST && memspace != XDEMHIP_DEVICE) return xd_fail(ctx, XDEMHIP_EINVAL, "memspace must be XDEMHIP_HOST or XDEMHIP_DEVICE");
    if (kernel < XDEMHIP_REGRID_NEAREST || kernel > XDEMHIP_REGRID_CUBIC_SPLINE)
        return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_regrid: kernel must be XDEMHIP_REGRID_NEAREST, _BILINEAR, _CUBIC or _CUBIC_SPLINE");
    const bool src_f = src_dtype == XDEMHIP_F32 || src_dtype == XDEMHIP_F64, dst_f = dst_dtype == XDEMHIP_F32 || dst_dtype == XDEMHIP_F64;
    const bool bytes_only = src_dtype == XDEMHIP_U8 && dst_dtype == XDEMHIP_U8;
    if (!(src_f && dst_f) && !bytes_only)
        return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_regrid: dtypes must be float32 / float64 (any combination), or uint8 to uint8");
    if (bytes_only && kernel != XDEMHIP_REGRID_NEAREST) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_regrid: uint8 rasters take the nearest kernel only");
    if (!regrid_map_ok(map4)) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_regrid: map4 must be finite with positive scales (both grids north-up)");

    RegridGeom g;
    g.H = H; g.W = W; g.h = h; g.w = w;
    g.kernel = kernel;
    g.x = regrid_axis(map4[0], map4[1], kernel);
    g.y = regrid_axis(map4[2], map4[3], kernel);
    const int src_size = src_dtype == XDEMHIP_F32 ? 4 : (src_dtype == XDEMHIP_F64 ? 8 : 1);
    const int dst_size = dst_dtype == XDEMHIP_F32 ? 4 : (dst_dtype == XDEMHIP_F64 ? 8 : 1);
    int64_t lds_bytes = 0, fw = 0, fh = 0;
    const int route = regrid_choose(g.x, g.y, kernel, src_size, ctx->regrid_route, &lds_bytes, &fw, &fh);
    g.fw_cap = (int)fw;
    g.fh_cap = (int)fh;
    if (route == XDEMHIP_REGRID_ROUTE_DIRECT && (int64_t)g.x.K * (int64_t)g.y.K > REGRID_MAX_TAPS)
        return xd_fail(ctx, XDEMHIP_EUNSUPPORTED, "xdemhip_regrid: more than 2^24 taps per destination pixel (downsampling too strong)");
    const int64_t rows_per_block = route == XDEMHIP_REGRID_ROUTE_TILE ? REGRID_TH : REGRID_NT / 64;
    if (((w + 63) / 64) * ((h + rows_per_block - 1) / rows_per_block) >= LIM)
        return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_regrid: destination too large for one launch");

    XD_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    const size_t src_bytes = (size_t)H * (size_t)W * (size_t)src_size, dst_bytes = (size_t)h * (size_t)w * (size_t)dst_size;
    XdPrefault prefault;
    std::vector<unsigned long long> landed((size_t)REGRID_SLOTS * REGRID_SLOT_STRIDE, 0);   // (declared before the scope whose copies land in it)
    const size_t landed_bytes = landed.size() * sizeof(unsigned long long);
    XdBuffers buf(ctx, "xdemhip_regrid");
    const void* d_src = buf.input(src, src_bytes, memspace);
    void* d_dst = buf.output(dst, dst_bytes, memspace);
    unsigned long long* d_count = buf.output(landed.data(), landed_bytes, XDEMHIP_HOST);
    if (buf.rc) return buf.rc;
    if (memspace == XDEMHIP_HOST) xd_prefault_start(prefault, dst, dst_bytes, ctx->host_copy_threads);
    XD_HIP_CHECK(ctx, hipMemsetAsync(d_count, 0, landed_bytes, ctx->stream));
    XD_HIP_CHECK(ctx, hipEventRecord(ctx->ev_start, ctx->stream));
    if (bytes_only) regrid_launch<unsigned char, unsigned char>(ctx, route, d_src, d_dst, g, lds_bytes, d_count);
    else if (src_dtype == XDEMHIP_F32 && dst_dtype == XDEMHIP_F32) regrid_launch<float, float>(ctx, route, d_src, d_dst, g, lds_bytes, d_count);
    else if (src_dtype == XDEMHIP_F32) regrid_launch<float, double>(ctx, route, d_src, d_dst, g, lds_bytes, d_count);
    else if (dst_dtype == XDEMHIP_F32) regrid_launch<double, float>(ctx, route, d_src, d_dst, g, lds_bytes, d_count);
    else regrid_launch<double, double>(ctx, route, d_src, d_dst, g, lds_bytes, d_count);
    (void)hipEventRecord(ctx->ev_stop, ctx->stream);
    ctx->timed = true;
    int rc = launched(ctx, "regrid kernel");
    prefault.join();
    if (rc == XDEMHIP_OK) rc = buf.finish();
    if (rc == XDEMHIP_OK) {
        unsigned long long total = 0;
        for (int k = 0; k < REGRID_SLOTS; ++k) total += landed[(size_t)k * REGRID_SLOT_STRIDE];
        *valid_count = (int64_t)total;
    }
    return rc;
}

}  // extern "C"
