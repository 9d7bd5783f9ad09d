// filter.hip -- xdemhip_filter: Gaussian, median, mean, minimum, maximum and distance filters of a raster (scipy.ndimage.gaussian_filter
// and generic_filter with the nan-functions, xDEM's old xdem/filters.py; include/xdemhip.h has the rules, DESIGN.md 5s the routes).
// tests/filters_oracle.py restates every rule in NumPy and every route below returns its bits: all arithmetic is float64 in the order
// the rule is written, every rounding where the rule has one (the Makefile builds this file with -ffp-contract=off).
//
// One frame for all kinds.  A workgroup of 256 threads owns a tile of tr x tc destination pixels and stages tile + halo into LDS once,
// the edge rule applied while staging, then filters out of LDS: one read and one write of the raster per call.
//   window kinds   (median, minimum, maximum, mean, distance; halo = size / 2 or the disk's radius) stage ORDER-PRESERVING UNSIGNED KEYS
//                  of the values: sign bit flipped for positive values, all bits for negative ones, so that unsigned order is the order of
//                  the values with -0.0 below +0.0; NaN and everything outside the raster is the all-ones key, which no other value has.
//                  The footprint is walked dy outer, dx inner, both ascending; a disk's half width per row comes from a table of the call.
//   median         windows of 3 x 3 and 5 x 5 are sorted in registers by a merge-exchange network (the comparators are a compile-time
//                  table, so every index is a constant) with the missing keys at the top, and ranks (n - 1) / 2 and n / 2 are picked.
//                  Larger windows find rank (n - 1) / 2 by bisection on the key bits over the window (count the keys below a candidate,
//                  one bit per walk, starting below the bits the window's smallest and largest key share); for an even count one more
//                  walk finds rank n / 2: the same key if enough keys are <= it, else the smallest key above it.  Exact at every size.
//   Gaussian       stages the values (NaN -> 0 and a byte plane of "not NaN" when normalising) mirrored about the raster's edges, the
//                  mirror repeated when lw exceeds a side, and the first lw + 1 weights; the axis-0 pass writes a tr x (tc + 2 lw) plane
//                  ROUNDED TO THE DTYPE into LDS, the axis-1 pass, the division and the NaN restore follow from there.
// Global route: the same pixel functions with an accessor that reads global memory (window kinds: clipped to the raster, one launch;
// Gaussian: two launches through planes the call owns).  Taken where tile + halo exceed FILTER_LDS_BUDGET, or under "filter_route" = 2.
#include "common.h"
#include "../../include/xdemhip_test.h"

#include <math.h>

namespace {

constexpr int FILTER_NT = 256;
constexpr int64_t FILTER_LDS_BUDGET = 63 * 1024;   // bytes of dynamic LDS one workgroup of the tiled route may ask for
constexpr int FILTER_MAX_RADIUS = 16383;           // window kinds: (2 R + 1)^2 stays below 2^30 (int32 counts)
constexpr int FILTER_MAX_LW = 1 << 20;             // Gaussian: taps on one side
constexpr int FILTER_GB_W = 64, FILTER_GB_H = FILTER_NT / 64;   // pixels of a workgroup of the global route

enum { FW_MEAN = 0, FW_MIN, FW_MAX, FW_DIST, FW_MED3, FW_MED5, FW_MEDN };

template <typename T> struct FilterKey;
template <> struct FilterKey<float> {
    using K = uint32_t;
    static constexpr int BITS = 32;
    static constexpr K MISSING = 0xFFFFFFFFu;
    static __device__ inline K of(float v) {
        if (v != v) return MISSING;
        const K u = __float_as_uint(v);
        return (u >> 31) ? ~u : (u | 0x80000000u);
    }
    static __device__ inline float val(K k) { return __uint_as_float((k >> 31) ? (k & 0x7FFFFFFFu) : ~k); }
    static __device__ inline int clz(K k) { return __clz((int)k); }
    static __device__ inline float nan() { return __builtin_nanf(""); }
};
template <> struct FilterKey<double> {
    using K = uint64_t;
    static constexpr int BITS = 64;
    static constexpr K MISSING = 0xFFFFFFFFFFFFFFFFull;
    static __device__ inline K of(double v) {
        if (v != v) return MISSING;
        const K u = (K)__double_as_longlong(v);
        return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
    }
    static __device__ inline double val(K k) { return __longlong_as_double((long long)((k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k)); }
    static __device__ inline int clz(K k) { return __clzll((long long)k); }
    static __device__ inline double nan() { return __builtin_nan(""); }
};

struct FilterGeom {
    int64_t H, W, tiles_c;
    int tr, tc, halo;
    double thr;
};

// ---- the frame of a call ------------------------------------------------------------------------------------------------------------
struct FilterPlan {
    int tr, tc, halo, route;
    int64_t lds_bytes;
};

// LDS bytes of a workgroup of the tiled route.  Window kinds: the keys of tile + halo.  Gaussian: lw + 1 weights (float64), the staged
// values, the two axis-0 planes (values and counts) and the staged "not NaN" bytes: the normalising form, which the plain one stays below.
int64_t filter_lds_bytes(int kind, int halo, int sz, int tr, int tc) {
    const int64_t ph = (int64_t)tr + 2 * (int64_t)halo, pw = (int64_t)tc + 2 * (int64_t)halo;
    int64_t b = ph * pw * sz;
    if (kind == XDEMHIP_FILTER_GAUSSIAN) b += ((int64_t)halo + 1) * 8 + 2 * (int64_t)tr * pw * sz + ph * pw;
    return (b + 15) / 16 * 16;
}

FilterPlan filter_plan(int kind, int halo, int sz, int route_switch) {
    static const int full[2][2] = {{32, 64}, {16, 64}}, tiny[1][2] = {{4, 8}};
    const int (*cand)[2] = route_switch == 3 ? tiny : full;
    const int n = route_switch == 3 ? 1 : 2;
    FilterPlan p;
    p.halo = halo;
    p.route = XDEMHIP_FILTER_ROUTE_GLOBAL;
    for (int k = 0; k < n; ++k) {
        p.tr = cand[k][0];
        p.tc = cand[k][1];
        p.lds_bytes = filter_lds_bytes(kind, halo, sz, p.tr, p.tc);
        if (p.lds_bytes <= FILTER_LDS_BUDGET) {
            p.route = XDEMHIP_FILTER_ROUTE_TILE;
            break;
        }
    }
    if (route_switch == 2) p.route = XDEMHIP_FILTER_ROUTE_GLOBAL;
    return p;
}

// ---- accessors: the key at (dy, dx) from a pixel, and the offsets that can lie inside the raster --------------------------------------
template <typename T> struct FilterLdsAcc {
    using K = typename FilterKey<T>::K;
    const K* centre;
    int pitch, dy_lo, dy_hi, dx_lo, dx_hi;
    __device__ inline K key(int dy, int dx) const { return centre[dy * pitch + dx]; }
};
template <typename T> struct FilterGlobalAcc {
    using K = typename FilterKey<T>::K;
    const T* centre;
    int64_t W;
    int dy_lo, dy_hi, dx_lo, dx_hi;
    __device__ inline K key(int dy, int dx) const { return FilterKey<T>::of(centre[(int64_t)dy * W + dx]); }
};

template <typename A, typename F> __device__ inline void filter_walk(const A& a, int R, const int* __restrict__ hw, F f) {
    for (int dy = a.dy_lo; dy <= a.dy_hi; ++dy) {
        const int h = hw ? hw[dy + R] : R;
        const int lo = -h > a.dx_lo ? -h : a.dx_lo, hi = h < a.dx_hi ? h : a.dx_hi;
        for (int dx = lo; dx <= hi; ++dx) f(a.key(dy, dx));
    }
}

// Merge exchange (Knuth 5.2.2 M, Batcher): a sorting network for any N; the comparators as a compile-time table.
template <int N> struct FilterNet {
    unsigned char a[256], b[256];
    int n;
    constexpr FilterNet() : a{}, b{}, n(0) {
        for (int p = 1; p < N; p <<= 1)
            for (int k = p; k >= 1; k >>= 1)
                for (int j = k % p; j <= N - 1 - k; j += 2 * k)
                    for (int i = 0; i <= (k - 1 < N - j - k - 1 ? k - 1 : N - j - k - 1); ++i)
                        if ((i + j) / (2 * p) == (i + j + k) / (2 * p)) {
                            a[n] = (unsigned char)(i + j);
                            b[n] = (unsigned char)(i + j + k);
                            ++n;
                        }
    }
};

// ranks (n - 1) / 2 and n / 2 of the n non-missing keys of an S x S window, sorted in registers
template <typename T, int S, typename A>
__device__ inline void filter_median_small(const A& a, typename FilterKey<T>::K& klo, typename FilterKey<T>::K& khi, int& n) {
    using FK = FilterKey<T>;
    using K = typename FK::K;
    constexpr int N = S * S, R = S / 2;
    constexpr FilterNet<N> net{};
    static_assert(net.n <= 256, "comparator table too small");
    K v[N];
    n = 0;
#pragma unroll
    for (int q = 0; q < N; ++q) {
        const int dy = q / S - R, dx = q % S - R;
        K k = FK::MISSING;
        if (dy >= a.dy_lo && dy <= a.dy_hi && dx >= a.dx_lo && dx <= a.dx_hi) k = a.key(dy, dx);
        v[q] = k;
        n += k != FK::MISSING;
    }
#pragma unroll
    for (int c = 0; c < net.n; ++c) {
        const K x = v[net.a[c]], y = v[net.b[c]];
        v[net.a[c]] = x < y ? x : y;
        v[net.b[c]] = x < y ? y : x;
    }
    const int rl = (n - 1) / 2, rh = n / 2;
    klo = khi = v[0];
#pragma unroll
    for (int q = 1; q < N; ++q) {
        klo = q == rl ? v[q] : klo;
        khi = q == rh ? v[q] : khi;
    }
}

// the same two ranks of a window of any size, by bisection on the key bits
template <typename T, typename A>
__device__ inline void filter_median_bisect(const A& a, int R, const int* __restrict__ hw, typename FilterKey<T>::K& klo,
                                            typename FilterKey<T>::K& khi, int& n) {
    using FK = FilterKey<T>;
    using K = typename FK::K;
    K kmin = FK::MISSING, kmax = 0;
    int cnt = 0;
    filter_walk(a, R, hw, [&](K k) {
        if (k != FK::MISSING) {
            ++cnt;
            kmin = k < kmin ? k : kmin;
            kmax = k > kmax ? k : kmax;
        }
    });
    n = cnt;
    klo = khi = kmin;
    if (cnt == 0 || kmin == kmax) return;
    const int rl = (cnt - 1) / 2;
    const int top = FK::BITS - 1 - FK::clz(kmin ^ kmax);   // the highest bit in which two keys of the window differ
    K prefix = top == FK::BITS - 1 ? (K)0 : (kmin >> (top + 1)) << (top + 1);
    for (int b = top; b >= 0; --b) {
        const K cand = prefix | ((K)1 << b);
        int below = 0;
        filter_walk(a, R, hw, [&](K k) { below += k < cand; });
        if (below <= rl) prefix = cand;   // at most rl keys below cand: the key of rank rl is >= cand
    }
    klo = khi = prefix;
    if (cnt & 1) return;
    int le = 0;
    K next = FK::MISSING;
    filter_walk(a, R, hw, [&](K k) {
        le += k <= prefix;
        next = (k > prefix && k < next) ? k : next;
    });
    khi = le >= rl + 2 ? prefix : next;
}

template <typename T, int MODE, typename A> __device__ inline T filter_window_pixel(const A& a, int R, const int* __restrict__ hw, double thr) {
    using FK = FilterKey<T>;
    using K = typename FK::K;
    if constexpr (MODE == FW_MEAN || MODE == FW_DIST) {
        double sum = 0.0;
        int cnt = 0;
        filter_walk(a, R, hw, [&](K k) {
            if (k != FK::MISSING) {
                sum += (double)FK::val(k);
                ++cnt;
            }
        });
        if constexpr (MODE == FW_MEAN) {
            return cnt ? (T)(sum / (double)cnt) : FK::nan();
        } else {
            const K kc = a.key(0, 0);
            if (kc == FK::MISSING) return FK::nan();
            const T v = FK::val(kc);
            const double m = sum / (double)cnt;
            return fabs((double)v - m) > thr ? FK::nan() : v;
        }
    } else if constexpr (MODE == FW_MIN || MODE == FW_MAX) {
        K best = MODE == FW_MIN ? FK::MISSING : (K)0;
        int cnt = 0;
        filter_walk(a, R, hw, [&](K k) {
            if (k != FK::MISSING) {
                ++cnt;
                if (MODE == FW_MIN) best = k < best ? k : best;
                else best = k > best ? k : best;
            }
        });
        return cnt ? FK::val(best) : FK::nan();
    } else {
        K klo, khi;
        int n;
        if constexpr (MODE == FW_MED3) filter_median_small<T, 3>(a, klo, khi, n);
        else if constexpr (MODE == FW_MED5) filter_median_small<T, 5>(a, klo, khi, n);
        else filter_median_bisect<T>(a, R, hw, klo, khi, n);
        if (n == 0) return FK::nan();
        if (n & 1) return FK::val(klo);
        return (T)(((double)FK::val(klo) + (double)FK::val(khi)) / 2.0);
    }
}

// ---- window kinds: tiled route ----------------------------------------------------------------------------------------------------------
template <typename T, int MODE>
__global__ __launch_bounds__(FILTER_NT) void filter_window_tile_kernel(const T* __restrict__ in, T* __restrict__ out, FilterGeom g,
                                                                       const int* __restrict__ hw) {
    using FK = FilterKey<T>;
    using K = typename FK::K;
    extern __shared__ __attribute__((aligned(16))) unsigned char filter_lds[];
    K* tile = reinterpret_cast<K*>(filter_lds);
    const int tid = threadIdx.x, R = g.halo, pw = g.tc + 2 * R, ph = g.tr + 2 * R;
    const int64_t by = (int64_t)blockIdx.x / g.tiles_c, bx = (int64_t)blockIdx.x - by * g.tiles_c;
    const int64_t y0 = by * g.tr, x0 = bx * g.tc;
    // tile + halo: a wave per row, its lanes along the row; outside the raster = missing
    for (int r = tid >> 6; r < ph; r += FILTER_NT / 64) {
        const int64_t y = y0 - R + r;
        const bool row_in = y >= 0 && y < g.H;
        for (int c = tid & 63; c < pw; c += 64) {
            const int64_t x = x0 - R + c;
            K k = FK::MISSING;
            if (row_in && x >= 0 && x < g.W) k = FK::of(in[(size_t)y * (size_t)g.W + (size_t)x]);
            tile[r * pw + c] = k;
        }
    }
    __syncthreads();
    for (int q = tid; q < g.tr * g.tc; q += FILTER_NT) {
        const int ly = q / g.tc, lx = q - ly * g.tc;
        const int64_t y = y0 + ly, x = x0 + lx;
        if (y >= g.H || x >= g.W) continue;
        const FilterLdsAcc<T> a{tile + (ly + R) * pw + lx + R, pw, -R, R, -R, R};
        out[(size_t)y * (size_t)g.W + (size_t)x] = filter_window_pixel<T, MODE>(a, R, hw, g.thr);
    }
}

// ---- window kinds: global route ---------------------------------------------------------------------------------------------------------
template <typename T, int MODE>
__global__ __launch_bounds__(FILTER_NT) void filter_window_global_kernel(const T* __restrict__ in, T* __restrict__ out, FilterGeom g,
                                                                         const int* __restrict__ hw) {
    const int tid = threadIdx.x, R = g.halo;
    const int64_t by = (int64_t)blockIdx.x / g.tiles_c, bx = (int64_t)blockIdx.x - by * g.tiles_c;
    const int64_t y = by * FILTER_GB_H + (tid >> 6), x = bx * FILTER_GB_W + (tid & 63);
    if (y >= g.H || x >= g.W) return;
    FilterGlobalAcc<T> a;
    a.centre = in + (size_t)y * (size_t)g.W + (size_t)x;
    a.W = g.W;
    a.dy_lo = y < R ? -(int)y : -R;
    a.dy_hi = g.H - 1 - y < R ? (int)(g.H - 1 - y) : R;
    a.dx_lo = x < R ? -(int)x : -R;
    a.dx_hi = g.W - 1 - x < R ? (int)(g.W - 1 - x) : R;
    out[(size_t)y * (size_t)g.W + (size_t)x] = filter_window_pixel<T, MODE>(a, R, hw, g.thr);
}

// ---- Gaussian ---------------------------------------------------------------------------------------------------------------------------
// index i of a line of n samples mirrored about its edges (d c b a | a b c d | d c b a), any i
__device__ inline int64_t filter_reflect(int64_t i, int64_t n) {
    if (i >= 0 && i < n) return i;
    const int64_t period = 2 * n;
    int64_t m = i % period;
    if (m < 0) m += period;
    return m < n ? m : period - 1 - m;
}

// SciPy's symmetric correlate1d about `at`: tmp = c w[lw]; for i = -lw .. -1: tmp += (x[i] + x[-i]) w[i + lw]
template <typename X> __device__ inline double filter_gauss_line(const X& x, int lw, const double* __restrict__ w) {
    double tmp = x(0) * w[lw];
    for (int i = -lw; i < 0; ++i) tmp += (x(i) + x(-i)) * w[i + lw];
    return tmp;
}

// LDS layout (dynamic): w[lw + 1] (float64) | S[ph][pw] (T) | A[tr][pw] (T) | NORM: B[tr][pw] (T) | M[ph][pw] (uint8)
template <typename T, bool NORM>
__global__ __launch_bounds__(FILTER_NT) void filter_gauss_tile_kernel(const T* __restrict__ in, T* __restrict__ out, FilterGeom g,
                                                                      const double* __restrict__ weights) {
    extern __shared__ __attribute__((aligned(16))) unsigned char filter_lds[];
    const int tid = threadIdx.x, lw = g.halo, pw = g.tc + 2 * lw, ph = g.tr + 2 * lw;
    double* w = reinterpret_cast<double*>(filter_lds);
    T* S = reinterpret_cast<T*>(w + lw + 1);
    T* A = S + (size_t)ph * pw;
    T* B = A + (size_t)g.tr * pw;
    unsigned char* M = reinterpret_cast<unsigned char*>(B + (size_t)g.tr * pw);
    const int64_t by = (int64_t)blockIdx.x / g.tiles_c, bx = (int64_t)blockIdx.x - by * g.tiles_c;
    const int64_t y0 = by * g.tr, x0 = bx * g.tc;
    for (int i = tid; i <= lw; i += FILTER_NT) w[i] = weights[i];
    for (int r = tid >> 6; r < ph; r += FILTER_NT / 64) {
        const T* row = in + (size_t)filter_reflect(y0 - lw + r, g.H) * (size_t)g.W;
        for (int c = tid & 63; c < pw; c += 64) {
            T v = row[filter_reflect(x0 - lw + c, g.W)];
            if (NORM) {
                const bool ok = v == v;
                M[r * pw + c] = ok;
                v = ok ? v : (T)0;
            }
            S[r * pw + c] = v;
        }
    }
    __syncthreads();
    // axis 0, rounded to the dtype
    for (int q = tid; q < g.tr * pw; q += FILTER_NT) {
        const int ly = q / pw, c = q - ly * pw;
        const T* s = S + (ly + lw) * pw + c;
        A[q] = (T)filter_gauss_line([&](int i) { return (double)s[i * pw]; }, lw, w);
        if (NORM) {
            const unsigned char* m = M + (ly + lw) * pw + c;
            B[q] = (T)filter_gauss_line([&](int i) { return (double)m[i * pw]; }, lw, w);
        }
    }
    __syncthreads();
    // axis 1, the division, the NaN restore
    for (int q = tid; q < g.tr * g.tc; q += FILTER_NT) {
        const int ly = q / g.tc, lx = q - ly * g.tc;
        const int64_t y = y0 + ly, x = x0 + lx;
        if (y >= g.H || x >= g.W) continue;
        const T* s = A + ly * pw + lx + lw;
        T res = (T)filter_gauss_line([&](int i) { return (double)s[i]; }, lw, w);
        if (NORM) {
            const T* b = B + ly * pw + lx + lw;
            const T den = (T)filter_gauss_line([&](int i) { return (double)b[i]; }, lw, w);
            res = M[(ly + lw) * pw + lx + lw] ? res / den : FilterKey<T>::nan();
        }
        out[(size_t)y * (size_t)g.W + (size_t)x] = res;
    }
}

// global route, first launch: axis 0 of the values (and of the "not NaN" plane) into planes of the call, rounded to the dtype
template <typename T, bool NORM>
__global__ __launch_bounds__(FILTER_NT) void filter_gauss_rows_kernel(const T* __restrict__ in, T* __restrict__ A, T* __restrict__ B, FilterGeom g,
                                                                      const double* __restrict__ w) {
    const int tid = threadIdx.x, lw = g.halo;
    const int64_t by = (int64_t)blockIdx.x / g.tiles_c, bx = (int64_t)blockIdx.x - by * g.tiles_c;
    const int64_t y = by * FILTER_GB_H + (tid >> 6), x = bx * FILTER_GB_W + (tid & 63);
    if (y >= g.H || x >= g.W) return;
    const T* col = in + (size_t)x;
    const size_t at = (size_t)y * (size_t)g.W + (size_t)x;
    A[at] = (T)filter_gauss_line([&](int i) {
        const T v = col[(size_t)filter_reflect(y + i, g.H) * (size_t)g.W];
        return NORM ? (v == v ? (double)v : 0.0) : (double)v;
    }, lw, w);
    if (NORM)
        B[at] = (T)filter_gauss_line([&](int i) {
            const T v = col[(size_t)filter_reflect(y + i, g.H) * (size_t)g.W];
            return v == v ? 1.0 : 0.0;
        }, lw, w);
}

// second launch: axis 1 of those planes, the division, the NaN restore
template <typename T, bool NORM>
__global__ __launch_bounds__(FILTER_NT) void filter_gauss_cols_kernel(const T* __restrict__ in, const T* __restrict__ A, const T* __restrict__ B,
                                                                      T* __restrict__ out, FilterGeom g, const double* __restrict__ w) {
    const int tid = threadIdx.x, lw = g.halo;
    const int64_t by = (int64_t)blockIdx.x / g.tiles_c, bx = (int64_t)blockIdx.x - by * g.tiles_c;
    const int64_t y = by * FILTER_GB_H + (tid >> 6), x = bx * FILTER_GB_W + (tid & 63);
    if (y >= g.H || x >= g.W) return;
    const size_t row = (size_t)y * (size_t)g.W;
    T res = (T)filter_gauss_line([&](int i) { return (double)A[row + (size_t)filter_reflect(x + i, g.W)]; }, lw, w);
    if (NORM) {
        const T den = (T)filter_gauss_line([&](int i) { return (double)B[row + (size_t)filter_reflect(x + i, g.W)]; }, lw, w);
        const T v = in[row + (size_t)x];
        res = v == v ? res / den : FilterKey<T>::nan();
    }
    out[row + (size_t)x] = res;
}

template <typename T> __global__ __launch_bounds__(FILTER_NT) void filter_any_nan_kernel(const T* __restrict__ in, int64_t n, int* flag) {
    bool found = false;
    for (int64_t i = (int64_t)blockIdx.x * FILTER_NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * FILTER_NT) {
        const T v = in[i];
        found |= v != v;
    }
    if (found) atomicOr(flag, 1);
}

// ---- launches -----------------------------------------------------------------------------------------------------------------------------
template <typename T, int MODE>
void filter_window_launch(xdemhip_ctx* ctx, const FilterPlan& p, const T* in, T* out, FilterGeom g, const int* hw, unsigned blocks) {
    if (p.route == XDEMHIP_FILTER_ROUTE_TILE)
        hipLaunchKernelGGL((filter_window_tile_kernel<T, MODE>), dim3(blocks), dim3(FILTER_NT), (size_t)p.lds_bytes, ctx->stream, in, out, g, hw);
    else
        hipLaunchKernelGGL((filter_window_global_kernel<T, MODE>), dim3(blocks), dim3(FILTER_NT), 0, ctx->stream, in, out, g, hw);
}

template <typename T>
void filter_window_dispatch(xdemhip_ctx* ctx, int kind, int size, const FilterPlan& p, const T* in, T* out, const FilterGeom& g, const int* hw,
                            unsigned blocks) {
    switch (kind) {
        case XDEMHIP_FILTER_MEAN: filter_window_launch<T, FW_MEAN>(ctx, p, in, out, g, hw, blocks); break;
        case XDEMHIP_FILTER_MIN: filter_window_launch<T, FW_MIN>(ctx, p, in, out, g, hw, blocks); break;
        case XDEMHIP_FILTER_MAX: filter_window_launch<T, FW_MAX>(ctx, p, in, out, g, hw, blocks); break;
        case XDEMHIP_FILTER_DISTANCE: filter_window_launch<T, FW_DIST>(ctx, p, in, out, g, hw, blocks); break;
        default:
            if (size == 3) filter_window_launch<T, FW_MED3>(ctx, p, in, out, g, hw, blocks);
            else if (size == 5) filter_window_launch<T, FW_MED5>(ctx, p, in, out, g, hw, blocks);
            else filter_window_launch<T, FW_MEDN>(ctx, p, in, out, g, hw, blocks);
    }
}

template <typename T, bool NORM>
void filter_gauss_launch(xdemhip_ctx* ctx, const FilterPlan& p, const T* in, T* out, const FilterGeom& g, const double* w, T* A, T* B, unsigned blocks) {
    if (p.route == XDEMHIP_FILTER_ROUTE_TILE) {
        hipLaunchKernelGGL((filter_gauss_tile_kernel<T, NORM>), dim3(blocks), dim3(FILTER_NT), (size_t)p.lds_bytes, ctx->stream, in, out, g, w);
        return;
    }
    hipLaunchKernelGGL((filter_gauss_rows_kernel<T, NORM>), dim3(blocks), dim3(FILTER_NT), 0, ctx->stream, in, A, B, g, w);
    hipLaunchKernelGGL((filter_gauss_cols_kernel<T, NORM>), dim3(blocks), dim3(FILTER_NT), 0, ctx->stream, in, (const T*)A, (const T*)B, out, g, w);
}

// what a kind asks of size / radius: the halo, or a status
int filter_halo(int kind, int size, int radius, double sigma, double truncate, int* halo, bool* disk, const char** why) {
    *disk = false;
    if (kind == XDEMHIP_FILTER_GAUSSIAN) {
        if (!(sigma > 0.0) || !(sigma < INFINITY) || !(truncate >= 0.0) || !(truncate < INFINITY)) {
            *why = "xdemhip_filter: sigma must be finite and > 0, truncate finite and >= 0";
            return XDEMHIP_EINVAL;
        }
        const double t = truncate * sigma + 0.5;
        if (!(t < (double)FILTER_MAX_LW + 1.0)) {
            *why = "xdemhip_filter: more than 2^20 Gaussian taps on a side";
            return XDEMHIP_EUNSUPPORTED;
        }
        if (size != 0 || radius != (int)t) {
            *why = "xdemhip_filter: a Gaussian takes size = 0 and radius = int(truncate * sigma + 0.5)";
            return XDEMHIP_EINVAL;
        }
        *halo = radius;
        return XDEMHIP_OK;
    }
    const bool takes_size = kind == XDEMHIP_FILTER_MEDIAN || kind == XDEMHIP_FILTER_MIN || kind == XDEMHIP_FILTER_MAX ||
                            (kind == XDEMHIP_FILTER_MEAN && size != 0);
    if (takes_size) {
        if (size < 3 || size % 2 == 0 || radius != 0) {
            *why = "xdemhip_filter: size must be odd and >= 3 (and radius 0 next to it)";
            return XDEMHIP_EINVAL;
        }
        if (size / 2 > FILTER_MAX_RADIUS) {
            *why = "xdemhip_filter: size above 32767";
            return XDEMHIP_EUNSUPPORTED;
        }
        *halo = size / 2;
        return XDEMHIP_OK;
    }
    if (size != 0 || radius < 0) {
        *why = "xdemhip_filter: a disk takes size = 0 and radius >= 0";
        return XDEMHIP_EINVAL;
    }
    if (radius > FILTER_MAX_RADIUS) {
        *why = "xdemhip_filter: radius above 16383";
        return XDEMHIP_EUNSUPPORTED;
    }
    *halo = radius;
    *disk = true;
    return XDEMHIP_OK;
}

template <typename T>
int filter_run(xdemhip_ctx* ctx, const void* in_v, int64_t H, int64_t W, int kind, int size, int halo, bool disk, const double* weights, int normalise,
               double threshold, void* out_v, int memspace) {
    const int sz = (int)sizeof(T);
    const FilterPlan p = filter_plan(kind, halo, sz, ctx->filter_route);
    FilterGeom g;
    g.H = H; g.W = W; g.halo = halo; g.thr = threshold;
    const bool tiled = p.route == XDEMHIP_FILTER_ROUTE_TILE;
    g.tr = tiled ? p.tr : FILTER_GB_H;
    g.tc = tiled ? p.tc : FILTER_GB_W;
    g.tiles_c = (W + g.tc - 1) / g.tc;
    const int64_t blocks = g.tiles_c * ((H + g.tr - 1) / g.tr);
    if (blocks >= (int64_t)1 << 31) return xd_fail(ctx, XDEMHIP_EUNSUPPORTED, "xdemhip_filter: raster too large for one launch");

    XD_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    const size_t bytes = (size_t)H * (size_t)W * sizeof(T);
    std::vector<int> half;   // (host sources of queued copies: declared before the scope that waits for them)
    int any_nan = 0;
    XdPrefault prefault;
    XdBuffers buf(ctx, "xdemhip_filter");
    const T* d_in = buf.input(static_cast<const T*>(in_v), bytes, memspace);
    T* d_out = buf.output(static_cast<T*>(out_v), bytes, memspace);
    if (buf.rc) return buf.rc;
    if (memspace == XDEMHIP_HOST) xd_prefault_start(prefault, out_v, bytes, ctx->host_copy_threads);

    if (kind == XDEMHIP_FILTER_GAUSSIAN) {
        const double* d_w = buf.input(weights, ((size_t)halo + 1) * sizeof(double), XDEMHIP_HOST);
        if (normalise == 2) {
            int* d_flag = buf.alloc<int>(1);
            if (buf.rc) return buf.rc;
            XD_HIP_CHECK(ctx, hipMemsetAsync(d_flag, 0, sizeof(int), ctx->stream));
            const int64_t n = H * W, want = (n + FILTER_NT - 1) / FILTER_NT;
            hipLaunchKernelGGL((filter_any_nan_kernel<T>), dim3((unsigned)(want < 4096 ? want : 4096)), dim3(FILTER_NT), 0, ctx->stream, d_in, n, d_flag);
            XD_HIP_CHECK(ctx, hipMemcpyAsync(&any_nan, d_flag, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
            XD_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
            normalise = any_nan ? 1 : 0;
        }
        T *A = nullptr, *B = nullptr;
        if (!tiled) {
            A = buf.alloc<T>((size_t)H * (size_t)W);
            if (normalise) B = buf.alloc<T>((size_t)H * (size_t)W);
        }
        if (buf.rc) return buf.rc;
        XD_HIP_CHECK(ctx, hipEventRecord(ctx->ev_start, ctx->stream));
        if (normalise) filter_gauss_launch<T, true>(ctx, p, d_in, d_out, g, d_w, A, B, (unsigned)blocks);
        else filter_gauss_launch<T, false>(ctx, p, d_in, d_out, g, d_w, A, B, (unsigned)blocks);
    } else {
        const int* d_hw = nullptr;
        if (disk) {   // half width of the disk's row dy: the largest h with h^2 <= R^2 - dy^2, in integers
            half.resize(2 * (size_t)halo + 1);
            for (int dy = -halo; dy <= halo; ++dy) {
                const int64_t v = (int64_t)halo * halo - (int64_t)dy * dy;
                int64_t h = (int64_t)sqrt((double)v);
                while ((h + 1) * (h + 1) <= v) ++h;
                while (h * h > v) --h;
                half[(size_t)(dy + halo)] = (int)h;
            }
            d_hw = buf.input(half.data(), half.size() * sizeof(int), XDEMHIP_HOST);
            if (buf.rc) return buf.rc;
        }
        XD_HIP_CHECK(ctx, hipEventRecord(ctx->ev_start, ctx->stream));
        filter_window_dispatch<T>(ctx, kind, size, p, d_in, d_out, g, d_hw, (unsigned)blocks);
    }
    (void)hipEventRecord(ctx->ev_stop, ctx->stream);
    ctx->timed = true;
    int rc = launched(ctx, "filter kernel");
    prefault.join();
    if (rc == XDEMHIP_OK) rc = buf.finish();
    return rc;
}

}  // namespace

extern "C" {

int xdemhip_filter_plan(int64_t H, int64_t W, int kind, int radius, int dtype, int route_switch, int* tile_rows, int* tile_cols, int* halo,
                        int64_t* lds_bytes, int64_t* lds_budget, int* route) {
    if (H < 1 || W < 1 || kind < XDEMHIP_FILTER_GAUSSIAN || kind > XDEMHIP_FILTER_DISTANCE || route_switch < 0 || route_switch > 3)
        return XDEMHIP_EINVAL;
    if (dtype != XDEMHIP_F32 && dtype != XDEMHIP_F64) return XDEMHIP_EINVAL;
    if (radius < 0) return XDEMHIP_EINVAL;
    if (radius > (kind == XDEMHIP_FILTER_GAUSSIAN ? FILTER_MAX_LW : FILTER_MAX_RADIUS)) return XDEMHIP_EUNSUPPORTED;
    const FilterPlan p = filter_plan(kind, radius, dtype == XDEMHIP_F32 ? 4 : 8, route_switch);
    if (tile_rows) *tile_rows = p.tr;
    if (tile_cols) *tile_cols = p.tc;
    if (halo) *halo = p.halo;
    if (lds_bytes) *lds_bytes = p.lds_bytes;
    if (lds_budget) *lds_budget = FILTER_LDS_BUDGET;
    if (route) *route = p.route;
    return XDEMHIP_OK;
}

int xdemhip_filter(xdemhip_ctx* ctx, const void* in, int dtype, int64_t H, int64_t W, int kind, int size, int radius, double sigma,
                   double truncate, const double* weights, int normalise, double threshold, void* out, int memspace) {
    if (!ctx) return XDEMHIP_EINVAL;
    if (!in || !out) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_filter: null argument");
    const int64_t LIM = (int64_t)1 << 31;
    if (H < 1 || W < 1 || H >= LIM || W >= LIM) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_filter: raster sides must be 1 .. 2^31 - 1");
    if (dtype != XDEMHIP_F32 && dtype != XDEMHIP_F64) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_filter: dtype must be XDEMHIP_F32 or XDEMHIP_F64");
    if (memspace != XDEMHIP_HOST && memspace != XDEMHIP_DEVICE) return xd_fail(ctx, XDEMHIP_EINVAL, "memspace must be XDEMHIP_HOST or XDEMHIP_DEVICE");
    if (kind < XDEMHIP_FILTER_GAUSSIAN || kind > XDEMHIP_FILTER_DISTANCE) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_filter: unknown kind");
    const size_t bytes = (size_t)H * (size_t)W * (dtype == XDEMHIP_F32 ? 4 : 8);
    const char *a = static_cast<const char*>(in), *b = static_cast<const char*>(out);
    if (a < b + bytes && b < a + bytes) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_filter: out must not overlap in");
    int halo = 0;
    bool disk = false;
    const char* why = "";
    const int rc = filter_halo(kind, size, radius, sigma, truncate, &halo, &disk, &why);
    if (rc != XDEMHIP_OK) return xd_fail(ctx, rc, why);
    if (kind == XDEMHIP_FILTER_GAUSSIAN) {
        if (!weights) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_filter: a Gaussian needs its weights");
        if (normalise < 0 || normalise > 2) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_filter: normalise must be 0, 1 or 2");
    }
    if (dtype == XDEMHIP_F32) return filter_run<float>(ctx, in, H, W, kind, size, halo, disk, weights, normalise, threshold, out, memspace);
    return filter_run<double>(ctx, in, H, W, kind, size, halo, disk, weights, normalise, threshold, out, memspace);
}

}  // extern "C"
