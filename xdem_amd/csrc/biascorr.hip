// biascorr.hip -- Deramp / VerticalShift on gfx950: the passes of the two methods that touch the grids.
//
// Replaces, for raster-raster input (xdem/coreg):
//   valid = inlier & isfinite(ref) & isfinite(tba)                      base.py:652-663       -> dh_valid_kernel (counts once per plan)
//   random subsample of the valid pixels                                base.py:577-617       -> rank_select.h (ranks -> pixels)
//   curve_fit(polynomial_2d, (xx, yy), ref - tba) over the valid pixels biascorr.py:195, 621-745, base.py:978-985
//                                                                                             -> least-squares moments (dh_moments_*)
//   np.median(ref - tba) over the valid pixels                          affine.py:721-770     -> radix selection (select_run.h)
//   elev + polyval2d(xx, yy, c), cast to the input dtype                biascorr.py:262-311, base.py:491 -> poly2d_apply_kernel
//   nmad(ref - interp(tba)(shifted points)), DhMinimize's objective      affine.py:617-674     -> dh_shift_*_kernel + two selections
// The (order+1)^2 least-squares system is solved on the host (xdem_amd/biascorr.py).
//
// The moments are taken in normalised coordinates u = (x - cx) / sx, v = (y - cy) / sy with cx = sx = (W_global - 1) / 2 and
// cy = sy = (H_global - 1) / 2 (a half-width of 0 is taken as 1): x = column, y = row_offset + row, as np.meshgrid(arange(W),
// arange(H)) numbers them.  In raw pixel coordinates the normal equations of order 2 on a 2000 x 3000 grid are useless; in
// normalised ones their condition number is ~2e2 (order 2) to ~1e5 (order 4).  Everything is accumulated in float64 and
// combined in a fixed order (fixed_sums.h; its reduce kernel and host side live here and serve rigid.hip and icp.hip too): same bits every call.
#include <math.h>
#include <string.h>

#include <vector>

#include "common.h"
#include "select.h"
#include "select_run.h"
#include "rank_select.h"
#include "nk_geom.h"
#include "dh_plan.h"
#include "dh_eval.h"

namespace xd {
namespace {

constexpr int DH_MAX_ORDER = 5;

template <typename T> __device__ __forceinline__ bool dh_finite(T v) { return t_finite<T>(v); }

// count of the valid pixels per tile (+ the valid mask itself with WRITE_MASK).  Lane l of a tile handles pixels g * 1024 + 4 l .. + 3
// (g = 0..3): four-wide loads (VEC: 16-byte aligned rasters, 4-byte aligned mask), one 4-byte mask store, coalesced across the wave.
template <typename T> __device__ __forceinline__ void load4(const T* p, T v[4]) {
    if (sizeof(T) == 4) {
        const float4 f = *reinterpret_cast<const float4*>(p);
        v[0] = (T)f.x; v[1] = (T)f.y; v[2] = (T)f.z; v[3] = (T)f.w;
    } else {
        const double2 a = *reinterpret_cast<const double2*>(p), b = *reinterpret_cast<const double2*>(p + 2);
        v[0] = (T)a.x; v[1] = (T)a.y; v[2] = (T)b.x; v[3] = (T)b.y;
    }
}
template <typename T> __device__ __forceinline__ void store4(T* p, const T v[4]) {
    if (sizeof(T) == 4) {
        *reinterpret_cast<float4*>(p) = make_float4((float)v[0], (float)v[1], (float)v[2], (float)v[3]);
    } else {
        *reinterpret_cast<double2*>(p) = make_double2((double)v[0], (double)v[1]);
        *reinterpret_cast<double2*>(p + 2) = make_double2((double)v[2], (double)v[3]);
    }
}

template <typename T, bool WRITE_MASK, bool VEC>
__global__ __launch_bounds__(256) void dh_valid_kernel(const T* __restrict__ ref, const T* __restrict__ tba, const uint8_t* __restrict__ inl,
                                                       int64_t n, uint8_t* __restrict__ valid, unsigned long long* __restrict__ tile_cnt) {
    int c = 0;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const int64_t p0 = (int64_t)blockIdx.x * RANK_TILE + g * 1024 + (int64_t)threadIdx.x * 4;
        if (VEC && p0 + 4 <= n) {
            T a[4], b[4];
            load4<T>(ref + p0, a);
            load4<T>(tba + p0, b);
            const uint32_t m4 = inl ? *reinterpret_cast<const uint32_t*>(inl + p0) : 0x01010101u;
            uint32_t o = 0;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const bool ok = dh_finite<T>(a[q]) && dh_finite<T>(b[q]) && ((m4 >> (8 * q)) & 0xFFu) != 0;
                o |= (ok ? 1u : 0u) << (8 * q);
                c += ok ? 1 : 0;
            }
            if (WRITE_MASK) *reinterpret_cast<uint32_t*>(valid + p0) = o;
        } else {
            for (int64_t p = p0; p < n && p < p0 + 4; ++p) {
                const bool ok = dh_finite<T>(ref[p]) && dh_finite<T>(tba[p]) && (inl == nullptr || inl[p] != 0);
                if (WRITE_MASK) valid[p] = ok ? 1 : 0;
                c += ok ? 1 : 0;
            }
        }
    }
    __shared__ int s[256];
    s[threadIdx.x] = c;
    __syncthreads();
    for (int half = 128; half > 0; half >>= 1) {
        if ((int)threadIdx.x < half) s[threadIdx.x] += s[threadIdx.x + half];
        __syncthreads();
    }
    if (threadIdx.x == 0) tile_cnt[blockIdx.x] = (unsigned long long)s[0];
}

// ---- moments, dense route ----------------------------------------------------------------------------------------------------
// One row at a time per workgroup (rows blockIdx.x, + gridDim.x, ...).  v is constant along a row: a lane keeps only S_a = sum u^a
// (a <= 2K) and D_i = sum dh u^i (i <= K) over its columns; the row's sums are reduced over the workgroup (wave shuffles, then the
// four waves in order: wave_sum and block_sum's order, fixed_sums.h) and lane t < NT multiplies its row sum by the power of v of the term it owns.
template <int K> struct PolyTerms {
    static constexpr int NA = 2 * K + 1, NR = K + 1, NS = NA + NR, NT = NA * NA + NR * NR;
};

// term t of the output: (row-sum index, power of v)
template <int K> __device__ __forceinline__ void term_of(int t, int& s_idx, int& vpow) {
    constexpr int NA = PolyTerms<K>::NA, NR = PolyTerms<K>::NR;
    if (t < NA * NA) { s_idx = t / NA; vpow = t % NA; }
    else { const int j = t - NA * NA; s_idx = NA + j / NR; vpow = j % NR; }
}

template <typename T, int K>
__device__ __forceinline__ void moments_pixel(T a, T b, bool in, double u, double* s) {
    constexpr int NA = PolyTerms<K>::NA;
    if (in && dh_finite<T>(a) && dh_finite<T>(b)) {
        const double d = (double)(T)(a - b);   // dh rounded in the input dtype first, as the reference forms `diff`
        double p = 1.0;
#pragma unroll
        for (int e = 0; e < NA; ++e) {
            s[e] += p;
            if (e <= K) s[NA + e] += d * p;
            p *= u;
        }
    }
}

template <typename T, int K, bool VEC>
__global__ __launch_bounds__(256) void dh_moments_rows_kernel(const T* __restrict__ ref, const T* __restrict__ tba, const uint8_t* __restrict__ inl,
                                                              int64_t H, int64_t W, int64_t row_offset, double ax, double bx, double ay,
                                                              double by, double* __restrict__ part) {
    constexpr int NS = PolyTerms<K>::NS, NT = PolyTerms<K>::NT;
    __shared__ double red[4][NS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int s_idx = 0, vpow = 0;
    if ((int)threadIdx.x < NT) term_of<K>(threadIdx.x, s_idx, vpow);
    double acc = 0.0;
    for (int64_t r = blockIdx.x; r < H; r += gridDim.x) {
        double s[NS];
#pragma unroll
        for (int e = 0; e < NS; ++e) s[e] = 0.0;
        const T* rr = ref + r * W;
        const T* tr = tba + r * W;
        const uint8_t* ir = inl ? inl + r * W : nullptr;
        if (VEC) {
            // W % 4 == 0 and 16-byte aligned rows: four columns per lane and load
            for (int64_t c = (int64_t)threadIdx.x * 4; c < W; c += 1024) {
                T a4[4], b4[4];
                if (sizeof(T) == 4) {
                    const float4 fa = *reinterpret_cast<const float4*>(rr + c), fb = *reinterpret_cast<const float4*>(tr + c);
                    a4[0] = (T)fa.x; a4[1] = (T)fa.y; a4[2] = (T)fa.z; a4[3] = (T)fa.w;
                    b4[0] = (T)fb.x; b4[1] = (T)fb.y; b4[2] = (T)fb.z; b4[3] = (T)fb.w;
                } else {
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        const double2 da = *reinterpret_cast<const double2*>(rr + c + 2 * h), db = *reinterpret_cast<const double2*>(tr + c + 2 * h);
                        a4[2 * h] = (T)da.x; a4[2 * h + 1] = (T)da.y; b4[2 * h] = (T)db.x; b4[2 * h + 1] = (T)db.y;
                    }
                }
                uint32_t m4 = 0x01010101u;
                if (ir) m4 = *reinterpret_cast<const uint32_t*>(ir + c);
#pragma unroll
                for (int q = 0; q < 4; ++q) moments_pixel<T, K>(a4[q], b4[q], ((m4 >> (8 * q)) & 0xFFu) != 0, (double)(c + q) * ax + bx, s);
            }
        } else {
            for (int64_t c = threadIdx.x; c < W; c += 256) moments_pixel<T, K>(rr[c], tr[c], ir == nullptr || ir[c] != 0, (double)c * ax + bx, s);
        }
#pragma unroll
        for (int e = 0; e < NS; ++e) s[e] = wave_sum<double>(s[e]);
        if (lane == 0) {
#pragma unroll
            for (int e = 0; e < NS; ++e) red[wave][e] = s[e];
        }
        __syncthreads();
        if ((int)threadIdx.x < NT) {
            const double rs = ((red[0][s_idx] + red[1][s_idx]) + red[2][s_idx]) + red[3][s_idx];
            const double v = (double)(row_offset + r) * ay + by;
            double vp = 1.0;
            for (int e = 0; e < vpow; ++e) vp *= v;
            acc += rs * vp;
        }
        __syncthreads();
    }
    if ((int)threadIdx.x < NT) part[(int64_t)blockIdx.x * NT + threadIdx.x] = acc;
}

// ---- moments, subsample route: over the drawn pixel list (contiguous ranges of it per workgroup) --------------------------------
// 256 pixels at a time go to LDS as their powers of u and v and dh; lane t < NT then adds its term over them.
template <typename T, int K>
__global__ __launch_bounds__(256) void dh_moments_list_kernel(const T* __restrict__ ref, const T* __restrict__ tba, const int64_t* __restrict__ idx,
                                                              int64_t k, int64_t per_block, int64_t W, int64_t row_offset, double ax, double bx,
                                                              double ay, double by, double* __restrict__ part) {
    constexpr int NA = PolyTerms<K>::NA, NR = PolyTerms<K>::NR, NT = PolyTerms<K>::NT;
    __shared__ double pu[256][NA];
    __shared__ double pv[256][NA];
    __shared__ double sd[256];
    int s_idx = 0, vpow = 0;
    if ((int)threadIdx.x < NT) term_of<K>(threadIdx.x, s_idx, vpow);
    const bool is_r = s_idx >= NA;
    const int upow = is_r ? s_idx - NA : s_idx;
    double acc = 0.0;
    const int64_t p0 = (int64_t)blockIdx.x * per_block;
    const int64_t p1 = p0 + per_block < k ? p0 + per_block : k;
    for (int64_t base = p0; base < p1; base += 256) {
        const int64_t i = base + threadIdx.x;
        if (i < p1) {
            const int64_t q = idx[i], r = q / W, c = q - r * W;
            const T a = ref[q], b = tba[q];
            const double u = (double)c * ax + bx, v = (double)(row_offset + r) * ay + by;
            double x = 1.0, y = 1.0;
            for (int e = 0; e < NA; ++e) { pu[threadIdx.x][e] = x; pv[threadIdx.x][e] = y; x *= u; y *= v; }
            sd[threadIdx.x] = (double)(T)(a - b);
        } else {
            for (int e = 0; e < NA; ++e) { pu[threadIdx.x][e] = 0.0; pv[threadIdx.x][e] = 0.0; }
            sd[threadIdx.x] = 0.0;
        }
        __syncthreads();
        if ((int)threadIdx.x < NT) {
            if (is_r)
                for (int p = 0; p < 256; ++p) acc += (sd[p] * pu[p][upow]) * pv[p][vpow];
            else
                for (int p = 0; p < 256; ++p) acc += pu[p][upow] * pv[p][vpow];
        }
        __syncthreads();
    }
    (void)NR;
    if ((int)threadIdx.x < NT) part[(int64_t)blockIdx.x * NT + threadIdx.x] = acc;
}

// ---- dh for the median / values routes ---------------------------------------------------------------------------------------
// dh of every pixel, NaN where it is not valid (validity recomputed: the whole-raster routes need no stored mask)
template <typename T>
__global__ __launch_bounds__(256) void dh_dense_kernel(const T* __restrict__ ref, const T* __restrict__ tba, const uint8_t* __restrict__ inl, int64_t n,
                                                       T* __restrict__ dh) {
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (int64_t)gridDim.x * blockDim.x) {
        const T a = ref[p], b = tba[p];
        dh[p] = (dh_finite<T>(a) && dh_finite<T>(b) && (inl == nullptr || inl[p] != 0)) ? (T)(a - b) : (T)NAN;
    }
}

template <typename T>
__global__ __launch_bounds__(256) void dh_gather_kernel(const T* __restrict__ ref, const T* __restrict__ tba, const int64_t* __restrict__ idx, int64_t k,
                                                        int64_t W, T* __restrict__ dh, int64_t* __restrict__ col, int64_t* __restrict__ row) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < k; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t q = idx[i];
        if (dh) dh[i] = (T)(ref[q] - tba[q]);
        if (col) col[i] = q % W;
        if (row) row[i] = q / W;
    }
}

// ---- shifted dh and its NMAD: the objective of DhMinimize ---------------------------------------------------------------------
// dh = ref[r, c] - bilinear(tba)(r + g.dr, c + g.dc) with the taps and the nodata rule of the Nuth-Kaab step (nk_geom.h), NaN where
// the interpolated value is.  One pass writes dh of every selected pixel to the plan's staging buffer -- NaN for the others on the
// dense route -- and, with HIST, counts the leading key digit of the values for the median's selection; the later digit passes and the
// second selection (|dh - median|) read the staging buffer only.
template <typename T>
__device__ __forceinline__ T dh_shift_pixel(const T* __restrict__ tba, const NkGeom& g, int64_t r, int64_t c, T refv) {
    const BiTap t = bi_locate(g, r, c);
    const BiVals<T> tv = bi_load<T>(tba, t);
    T val;
    const bool ok = bi_value<T>(g, tba, t, tv.a00, tv.a01, tv.a10, tv.a11, val);
    return ok ? t_sub(refv, val) : (T)NAN;   // (a difference that overflows stays +-inf, as in NumPy: nanmedian keeps it)
}

// (the leading-digit counters of a workgroup, dh_hist_count / dh_hist_flush: dh_eval.h)

// dense route: the tiles of dh_valid_kernel (lane l of a tile: pixels g * 1024 + 4 l .. + 3, g = 0..3), 16-byte loads of ref and
// stores of dh and a 4-byte load of the mask where the rasters allow (VEC), one pixel at a time in the last, partial group
template <typename T, bool VEC, bool HIST>
__global__ __launch_bounds__(256) void dh_shift_dense_kernel(const T* __restrict__ ref, const T* __restrict__ tba, const uint8_t* __restrict__ valid,
                                                             NkGeom g, int64_t n, double invW, T* __restrict__ stage, uint64_t* __restrict__ hist) {
    __shared__ uint32_t h[HIST ? DH_HIST_COPIES * DH_HIST_STRIDE : 1];
    if (HIST) {
        for (int k = threadIdx.x; k < DH_HIST_COPIES * DH_HIST_STRIDE; k += blockDim.x) h[k] = 0;
        __syncthreads();
    }
    uint32_t* hc = h + (HIST ? (threadIdx.x % DH_HIST_COPIES) * DH_HIST_STRIDE : 0);
#pragma unroll
    for (int gq = 0; gq < 4; ++gq) {
        const int64_t p0 = (int64_t)blockIdx.x * RANK_TILE + gq * 1024 + (int64_t)threadIdx.x * 4;
        if (p0 >= n) continue;
        const bool full = p0 + 4 <= n;
        const int cnt = full ? 4 : (int)(n - p0);
        T a[4];
        uint32_t m4 = 0;
        if (VEC && full) {
            load4<T>(ref + p0, a);
            m4 = *reinterpret_cast<const uint32_t*>(valid + p0);
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                a[q] = q < cnt ? ref[p0 + q] : (T)NAN;
                m4 |= (q < cnt && valid[p0 + q]) ? (1u << (8 * q)) : 0u;
            }
        }
        int64_t r, c;
        row_col(p0, g.W, invW, r, c);
        T o[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            o[q] = (T)NAN;
            if (q < cnt) {
                if ((m4 >> (8 * q)) & 0xFFu) o[q] = dh_shift_pixel<T>(tba, g, r + g.roff, c, a[q]);
                if (HIST) dh_hist_count<T>(hc, o[q]);
                if (++c == g.W) { c = 0; ++r; }
            }
        }
        if (VEC && full) store4<T>(stage + p0, o);
        else
            for (int q = 0; q < cnt; ++q) stage[p0 + q] = o[q];
    }
    if (HIST) dh_hist_flush(h, hist);
}

// list route: dh of the listed pixels (the drawn ones, or all valid ones for xdemhip_dh_shift_values), in list order
template <typename T, bool HIST>
__global__ __launch_bounds__(256) void dh_shift_list_kernel(const T* __restrict__ ref, const T* __restrict__ tba, const int64_t* __restrict__ idx,
                                                            int64_t k, NkGeom g, double invW, T* __restrict__ out, uint64_t* __restrict__ hist) {
    __shared__ uint32_t h[HIST ? DH_HIST_COPIES * DH_HIST_STRIDE : 1];
    if (HIST) {
        for (int q = threadIdx.x; q < DH_HIST_COPIES * DH_HIST_STRIDE; q += blockDim.x) h[q] = 0;
        __syncthreads();
    }
    uint32_t* hc = h + (HIST ? (threadIdx.x % DH_HIST_COPIES) * DH_HIST_STRIDE : 0);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < k; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t q = idx[i];
        int64_t r, c;
        row_col(q, g.W, invW, r, c);
        const T d = dh_shift_pixel<T>(tba, g, r + g.roff, c, ref[q]);
        out[i] = d;
        if (HIST) dh_hist_count<T>(hc, d);
    }
    if (HIST) dh_hist_flush(h, hist);
}

// (|dh - median| as a source, the finish kernel of a selection and the block one evaluation hands back: dh_eval.h)

// ---- apply: out = cast(double(elev) + polyval2d(x, y, c)) ---------------------------------------------------------------------
// NumPy's evaluation order (numpy/polynomial/polynomial.py polyval / polyval2d), no contraction (-ffp-contract=off):
//   t_j = c[K-1, j] + x * 0;  t_j = c[K-2, j] + t_j * x; ... ; t_j = c[0, j] + t_j * x      (polyval(x, c), tensor form)
//   P   = t_{K-1} + y * 0;    P   = t_{K-2} + P * y;   ... ; P   = t_0 + P * y           (polyval(y, t, tensor=False))
struct PolyCoeffs { double c[(DH_MAX_ORDER + 1) * (DH_MAX_ORDER + 1)]; };

template <typename T, int K>
__global__ __launch_bounds__(256) void poly2d_apply_kernel(const T* __restrict__ elev, int64_t H, int64_t W, int64_t row_offset, PolyCoeffs cf,
                                                           T* __restrict__ out) {
    for (int64_t r = blockIdx.y; r < H; r += gridDim.y) {
        const double y = (double)(row_offset + r);
        for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < W; c += (int64_t)gridDim.x * blockDim.x) {
            const double x = (double)c;
            double t[K];
#pragma unroll
            for (int j = 0; j < K; ++j) {
                double a = __dadd_rn(cf.c[(K - 1) * K + j], __dmul_rn(x, 0.0));
#pragma unroll
                for (int i = K - 2; i >= 0; --i) a = __dadd_rn(cf.c[i * K + j], __dmul_rn(a, x));
                t[j] = a;
            }
            double p = __dadd_rn(t[K - 1], __dmul_rn(y, 0.0));
#pragma unroll
            for (int j = K - 2; j >= 0; --j) p = __dadd_rn(t[j], __dmul_rn(p, y));
            out[r * W + c] = (T)__dadd_rn((double)elev[r * W + c], p);
        }
    }
}

// Four columns per lane (W % 4 == 0, 16-byte aligned rows): the Horner terms t_j depend on x only, so a lane forms them once for its
// columns and walks rows blockIdx.y, + gridDim.y, ... (two rows per step, loads first); same operations in the same order as above.
template <typename T, int K>
__global__ __launch_bounds__(256) void poly2d_apply_vec_kernel(const T* __restrict__ elev, int64_t H, int64_t W, int64_t row_offset, PolyCoeffs cf,
                                                               T* __restrict__ out) {
    const int64_t c0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (c0 >= W) return;
    double t[4][K];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const double x = (double)(c0 + q);
#pragma unroll
        for (int j = 0; j < K; ++j) {
            double a = __dadd_rn(cf.c[(K - 1) * K + j], __dmul_rn(x, 0.0));
#pragma unroll
            for (int i = K - 2; i >= 0; --i) a = __dadd_rn(cf.c[i * K + j], __dmul_rn(a, x));
            t[q][j] = a;
        }
    }
    for (int64_t r = blockIdx.y; r < H; r += 2 * (int64_t)gridDim.y) {
        const int64_t r2 = r + gridDim.y;
        const bool two = r2 < H;
        T e[2][4];
        load4<T>(elev + r * W + c0, e[0]);
        if (two) load4<T>(elev + r2 * W + c0, e[1]);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            if (h == 1 && !two) break;
            const double y = (double)(row_offset + (h ? r2 : r));
            T o[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                double p = __dadd_rn(t[q][K - 1], __dmul_rn(y, 0.0));
#pragma unroll
                for (int j = K - 2; j >= 0; --j) p = __dadd_rn(t[q][j], __dmul_rn(p, y));
                o[q] = (T)__dadd_rn((double)e[h][q], p);
            }
            store4<T>(out + (h ? r2 : r) * W + c0, o);
        }
    }
}

template <typename T>
int launch_apply(xdemhip_ctx* ctx, const T* elev, int64_t H, int64_t W, int64_t row_offset, const PolyCoeffs& cf, int K, T* out) {
    const bool vec = W % 4 == 0 && (uintptr_t)elev % 16 == 0 && (uintptr_t)out % 16 == 0;
    int64_t gx = vec ? (W + 1023) / 1024 : (W + 255) / 256;
    if (!vec && gx > 64) gx = 64;
    int64_t gy = ((int64_t)ctx->num_cu * 8 + gx - 1) / gx;
    gy = gy < 1 ? 1 : (gy > H ? H : gy);
    if (gy > 65535) gy = 65535;
    if (gx > 0x7FFFFFFF) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_poly2d_apply: raster too wide");
    const dim3 g((unsigned)gx, (unsigned)gy);
#define XD_APPLY_CASE(KK)                                                                                                    \
    case KK:                                                                                                                 \
        if (vec) hipLaunchKernelGGL((poly2d_apply_vec_kernel<T, KK>), g, dim3(256), 0, ctx->stream, elev, H, W, row_offset, cf, out); \
        else hipLaunchKernelGGL((poly2d_apply_kernel<T, KK>), g, dim3(256), 0, ctx->stream, elev, H, W, row_offset, cf, out);         \
        break;
    switch (K) {
        XD_APPLY_CASE(1) XD_APPLY_CASE(2) XD_APPLY_CASE(3) XD_APPLY_CASE(4) XD_APPLY_CASE(5) XD_APPLY_CASE(6)
        default: return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_poly2d_apply: order must be 0..5");
    }
#undef XD_APPLY_CASE
    return launched(ctx, "poly2d_apply_kernel");
}

template <typename T, int K>
int launch_moments_t(xdemhip_dh_plan* P, int64_t row_offset, double ax, double bx, double ay, double by, double* d_part, int* nblocks) {
    xdemhip_ctx* ctx = P->ctx;
    if (P->drawn) {
        const int64_t k = P->n_idx;
        int64_t nb = (int64_t)ctx->num_cu * 4;
        int64_t per = (k + nb - 1) / nb;
        per = ((per + 255) / 256) * 256;
        if (per < 256) per = 256;
        nb = (k + per - 1) / per;
        if (nb < 1) nb = 1;
        *nblocks = (int)nb;
        hipLaunchKernelGGL((dh_moments_list_kernel<T, K>), dim3((unsigned)nb), dim3(256), 0, ctx->stream, static_cast<const T*>(P->ref),
                           static_cast<const T*>(P->tba), P->idx, k, per, P->W, row_offset, ax, bx, ay, by, d_part);
    } else {
        const int nb = fixed_sums_grid(ctx, P->H);
        *nblocks = nb;
        const bool vec = (P->W % 4 == 0) && ((uintptr_t)P->ref % 16 == 0) && ((uintptr_t)P->tba % 16 == 0) &&
                         (P->inlier == nullptr || (uintptr_t)P->inlier % 4 == 0);
        if (vec)
            hipLaunchKernelGGL((dh_moments_rows_kernel<T, K, true>), dim3((unsigned)nb), dim3(256), 0, ctx->stream, static_cast<const T*>(P->ref),
                               static_cast<const T*>(P->tba), P->inlier, P->H, P->W, row_offset, ax, bx, ay, by, d_part);
        else
            hipLaunchKernelGGL((dh_moments_rows_kernel<T, K, false>), dim3((unsigned)nb), dim3(256), 0, ctx->stream, static_cast<const T*>(P->ref),
                               static_cast<const T*>(P->tba), P->inlier, P->H, P->W, row_offset, ax, bx, ay, by, d_part);
    }
    return launched(ctx, "moments kernel");
}

template <typename T>
int launch_moments(xdemhip_dh_plan* P, int K, int64_t row_offset, double ax, double bx, double ay, double by, double* d_part, int* nblocks) {
    switch (K) {
        case 0: return launch_moments_t<T, 0>(P, row_offset, ax, bx, ay, by, d_part, nblocks);
        case 1: return launch_moments_t<T, 1>(P, row_offset, ax, bx, ay, by, d_part, nblocks);
        case 2: return launch_moments_t<T, 2>(P, row_offset, ax, bx, ay, by, d_part, nblocks);
        case 3: return launch_moments_t<T, 3>(P, row_offset, ax, bx, ay, by, d_part, nblocks);
        case 4: return launch_moments_t<T, 4>(P, row_offset, ax, bx, ay, by, d_part, nblocks);
        case 5: return launch_moments_t<T, 5>(P, row_offset, ax, bx, ay, by, d_part, nblocks);
        default: return xd_fail(P->ctx, XDEMHIP_EINVAL, "xdemhip_dh_poly_moments: order must be 0..5");
    }
}

template <typename T>
void launch_valid_t(xdemhip_dh_plan* P, bool write_mask) {
    xdemhip_ctx* ctx = P->ctx;
    const T* r = static_cast<const T*>(P->ref);
    const T* t = static_cast<const T*>(P->tba);
    const int64_t n = P->H * P->W;
    const bool vec = (uintptr_t)r % 16 == 0 && (uintptr_t)t % 16 == 0 && (P->inlier == nullptr || (uintptr_t)P->inlier % 4 == 0);
    const dim3 g((unsigned)P->n_tiles), b(256);
    if (write_mask) {
        if (vec) hipLaunchKernelGGL((dh_valid_kernel<T, true, true>), g, b, 0, ctx->stream, r, t, P->inlier, n, P->valid, P->tile_off);
        else hipLaunchKernelGGL((dh_valid_kernel<T, true, false>), g, b, 0, ctx->stream, r, t, P->inlier, n, P->valid, P->tile_off);
    } else {
        if (vec) hipLaunchKernelGGL((dh_valid_kernel<T, false, true>), g, b, 0, ctx->stream, r, t, P->inlier, n, (uint8_t*)nullptr, P->tile_off);
        else hipLaunchKernelGGL((dh_valid_kernel<T, false, false>), g, b, 0, ctx->stream, r, t, P->inlier, n, (uint8_t*)nullptr, P->tile_off);
    }
}
int launch_valid(xdemhip_dh_plan* P, bool write_mask) {
    if (P->dtype == XDEMHIP_F32) launch_valid_t<float>(P, write_mask);
    else launch_valid_t<double>(P, write_mask);
    return launched(P->ctx, "dh_valid_kernel");
}

// the valid mask, built on first need (the subsample and values routes; the whole-raster moments and median recompute validity).  The
// tile counts are written again: the same numbers as at creation, so the scanned offsets stay what they were.
int ensure_mask(xdemhip_dh_plan* P) {
    if (P->valid) return XDEMHIP_OK;
    xdemhip_ctx* ctx = P->ctx;
    const int64_t n = P->H * P->W;
    P->valid = P->mem.take<uint8_t>((size_t)n, "valid mask");
    { const int rc = P->mem.status(); if (rc) return rc; }
    const int rc = launch_valid(P, true);
    if (rc) return rc;
    hipLaunchKernelGGL(rank_scan_kernel, dim3(1), dim3(1024), 0, ctx->stream, P->tile_off, P->n_tiles, P->tile_off + P->n_tiles);
    return launched(ctx, "dh_scan_kernel");
}

// the list of all valid pixels (raster order), for the values route of a plan that was never subsampled
int ensure_valid_idx(xdemhip_dh_plan* P) {
    if (P->drawn || P->idx) return XDEMHIP_OK;
    xdemhip_ctx* ctx = P->ctx;
    { const int rc = ensure_mask(P); if (rc) return rc; }
    P->idx = P->mem.take<int64_t>((size_t)P->n_valid, "valid pixel list");
    { const int rc = P->mem.status(); if (rc) return rc; }
    hipLaunchKernelGGL((rank_select_kernel<RankOut::List>), dim3((unsigned)P->n_tiles), dim3(256), 0, ctx->stream, P->valid, P->H * P->W,
                       (const unsigned long long*)nullptr, (const uint8_t*)nullptr, P->tile_off, P->idx, (uint8_t*)nullptr);
    if (launched(ctx, "dh_sel_kernel")) return XDEMHIP_EHIP;
    P->n_idx = P->n_valid;
    return XDEMHIP_OK;
}

template <typename T>
int median_typed(xdemhip_dh_plan* P, double* median, int64_t* count) {
    typedef typename KeyT<T>::type K;
    xdemhip_ctx* ctx = P->ctx;
    const int64_t n = P->drawn ? P->n_idx : P->H * P->W;
    XdBuffers buf(ctx, "xdemhip_dh_median");
    T* d = buf.alloc<T>((size_t)n);
    unsigned char* scratch = buf.alloc<unsigned char>(scratch_size(1));
    if (buf.rc) return buf.rc;
    const dim3 g(grid_for(ctx, n, 256, 16));
    if (P->drawn)
        hipLaunchKernelGGL((dh_gather_kernel<T>), g, dim3(256), 0, ctx->stream, static_cast<const T*>(P->ref), static_cast<const T*>(P->tba), P->idx, n,
                           P->W, d, (int64_t*)nullptr, (int64_t*)nullptr);
    else
        hipLaunchKernelGGL((dh_dense_kernel<T>), g, dim3(256), 0, ctx->stream, static_cast<const T*>(P->ref), static_cast<const T*>(P->tba), P->inlier, n, d);
    if (launched(ctx, "dh kernel")) return XDEMHIP_EHIP;
    std::vector<SelResult<K>> r;
    XdLocalSelection local(ctx);   // (one process's pixels)
    SelWorkspaceLocal lws(ctx);
    if (n >= SEL_BRACKET_MIN_N) (void)sel_ws_create(lws.mem, n, sizeof(T), 1, lws.ws);  // (on failure: plain selection)
    const int rc = run_select<T>(ctx, d, nullptr, n, 1, scratch, r, &lws.ws);
    if (rc == XDEMHIP_OK) {
        *count = (int64_t)r[0].st.count;
        *median = median_from<T>(r[0]);
    }
    return rc;
}

// ---- shifted-dh evaluations: buffers the plan keeps, and the sequence of one evaluation ---------------------------------------------
int ensure_stage(xdemhip_dh_plan* P, int64_t n) {
    if (P->stage && P->stage_n == n) return XDEMHIP_OK;
    P->stage_n = P->mem.regrow(P->stage, (size_t)n * (P->dtype == XDEMHIP_F32 ? 4 : 8), "dh staging buffer") ? n : 0;
    return P->mem.status();
}
int ensure_selection(xdemhip_dh_plan* P, int64_t n) {
    if (!P->sel_scratch) P->sel_scratch = P->mem.take<unsigned char>(scratch_size(1) + sizeof(DhEvalOut), "dh selection scratch");
    { const int rc = P->mem.status(); if (rc) return rc; }
    if (P->sel_ws_n != n) {
        sel_ws_free(P->mem, P->sel_ws);
        if (n >= SEL_BRACKET_MIN_N) (void)sel_ws_create(P->mem, n, P->dtype == XDEMHIP_F32 ? 4 : 8, 1, P->sel_ws);  // (on failure: plain selection)
        P->sel_ws_n = n;
    }
    return XDEMHIP_OK;
}

NkGeom dh_geom(const xdemhip_dh_plan* P, double shift_x, double shift_y, double res_x, double res_y) {
    NkGeom g;
    g.H = P->H; g.W = P->W; g.roff = 0; g.dr = -shift_y / res_y; g.dc = shift_x / res_x; g.rule = P->ctx->nk_nan_rule;
    return g;
}

// dh of the plan's selection at a shift into the staging buffer (with_hist: + the leading digit's counts into `hist`)
template <typename T>
int launch_shift(xdemhip_dh_plan* P, const NkGeom& g, bool with_hist, uint64_t* hist) {
    xdemhip_ctx* ctx = P->ctx;
    const T* ref = static_cast<const T*>(P->ref);
    const T* tba = static_cast<const T*>(P->tba);
    T* stage = static_cast<T*>(P->stage);
    const double invW = 1.0 / (double)P->W;
    if (P->drawn) {
        const dim3 grid(grid_for(ctx, P->n_idx, 256, 16)), b(256);
        if (with_hist) hipLaunchKernelGGL((dh_shift_list_kernel<T, true>), grid, b, 0, ctx->stream, ref, tba, P->idx, P->n_idx, g, invW, stage, hist);
        else hipLaunchKernelGGL((dh_shift_list_kernel<T, false>), grid, b, 0, ctx->stream, ref, tba, P->idx, P->n_idx, g, invW, stage, hist);
    } else {
        const int64_t n = P->H * P->W;
        const bool vec = (uintptr_t)ref % 16 == 0 && (uintptr_t)stage % 16 == 0 && (uintptr_t)P->valid % 4 == 0;
        const dim3 grid((unsigned)P->n_tiles), b(256);
#define XD_DENSE(V, HH) hipLaunchKernelGGL((dh_shift_dense_kernel<T, V, HH>), grid, b, 0, ctx->stream, ref, tba, P->valid, g, n, invW, stage, hist)
        if (vec) { if (with_hist) XD_DENSE(true, true); else XD_DENSE(true, false); }
        else { if (with_hist) XD_DENSE(false, true); else XD_DENSE(false, false); }
#undef XD_DENSE
    }
    return launched(ctx, "dh_shift kernel");
}

// One evaluation (dh_eval.h: the data pass, two selections, one fetch) over the plan's selection; nothing is allocated here once the
// plan's buffers exist.
template <typename T>
int shift_nmad_typed(xdemhip_dh_plan* P, const NkGeom& g, double nfact, double* median, double* nmad, int64_t* count) {
    xdemhip_ctx* ctx = P->ctx;
    const int64_t n = P->drawn ? P->n_idx : P->H * P->W;
    int rc = ensure_stage(P, n);
    if (rc == XDEMHIP_OK) rc = ensure_selection(P, n);
    if (rc) return rc;
    return dh_eval_median_nmad<T>(ctx, static_cast<T*>(P->stage), n, P->sel_scratch, &P->sel_ws, nfact,
                                  [&](bool with_hist, uint64_t* hist) { return launch_shift<T>(P, g, with_hist, hist); }, median, nmad, count);
}

inline void norm_axis(int64_t n_global, double* a, double* b) {
    double half = 0.5 * (double)(n_global - 1);
    const double centre = half;
    if (!(half > 0)) half = 1.0;
    *a = 1.0 / half;
    *b = -centre / half;
}

}  // namespace

// what rigid.hip and icp.hip need of the plan's lazily built parts (dh_plan.h)
int dh_ensure_mask(xdemhip_dh_plan* P) { return ensure_mask(P); }
int dh_ensure_valid_idx(xdemhip_dh_plan* P) { return ensure_valid_idx(P); }
// ---- the reduce kernel and the host side of the fixed-order sums (fixed_sums.h) -----------------------------------------------------
// per-workgroup partials -> totals: one workgroup per term, lane l adds the partials of workgroups l, l + 256, ... in order, then a
// fixed tree over the lanes (the same bits every call)
static __global__ __launch_bounds__(256) void fixed_sums_reduce_kernel(const double* __restrict__ part, int nblocks, int nt, double* __restrict__ out) {
    __shared__ double s[256];
    const int t = blockIdx.x;
    double a = 0.0;
    for (int b = threadIdx.x; b < nblocks; b += 256) a += part[(int64_t)b * nt + t];
    s[threadIdx.x] = a;
    __syncthreads();
    for (int half = 128; half > 0; half >>= 1) {
        if ((int)threadIdx.x < half) s[threadIdx.x] += s[threadIdx.x + half];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[t] = s[0];
}
int FixedSums::reserve(XdOwned& mem, int nt, const char* who) {
    const int64_t need = ((int64_t)mem.ctx->num_cu * 8 + 1) * nt;
    if (cap >= need) return XDEMHIP_OK;
    cap = mem.regrow(part, (size_t)need * 8, who) ? need : 0;
    return mem.status();
}
int fixed_sums_reduce(xdemhip_ctx* ctx, double* part, int nblocks, int nt, const char* what) {
    hipLaunchKernelGGL(fixed_sums_reduce_kernel, dim3((unsigned)nt), dim3(256), 0, ctx->stream, part, nblocks, nt, part + (int64_t)nblocks * nt);
    return launched(ctx, what);
}
int fixed_sums_finish(xdemhip_ctx* ctx, const FixedSums& fs, int nblocks, int nt, const char* what, double* totals) {
    double* d_out = fs.part + (int64_t)nblocks * nt;
    int rc = fixed_sums_reduce(ctx, fs.part, nblocks, nt, what);
    (void)hipEventRecord(ctx->ev_stop, ctx->stream);
    ctx->timed = (rc == XDEMHIP_OK);
    if (rc == XDEMHIP_OK) rc = xd_d2h(ctx, totals, d_out, (size_t)nt * 8);   // the one fetch of the call
    return rc == XDEMHIP_OK ? xd_sync(ctx) : rc;
}
}  // namespace xd

using namespace xd;

extern "C" {

void xdemhip_dh_destroy(xdemhip_dh_plan* P) { delete P; }   // (its owner frees the device buffers)

int xdemhip_dh_create(xdemhip_ctx* ctx, const void* ref, const void* tba, const uint8_t* inlier, int dtype, int64_t H, int64_t W, int memspace,
                      xdemhip_dh_plan** out_plan, int64_t* n_valid) {
    XdFetchScope fetch_scope_(ctx);
    if (!ctx) return XDEMHIP_EINVAL;
    if (!ref || !tba || !out_plan) return xd_fail(ctx, XDEMHIP_EINVAL, "null argument");
    if (H < 1 || W < 1) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_dh_create: empty raster");
    if (dtype != XDEMHIP_F32 && dtype != XDEMHIP_F64) return xd_fail(ctx, XDEMHIP_EINVAL, "dtype must be float32 or float64");
    if (memspace != XDEMHIP_HOST && memspace != XDEMHIP_DEVICE) return xd_fail(ctx, XDEMHIP_EINVAL, "bad memspace");
    XD_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    const size_t es = dtype == XDEMHIP_F32 ? 4 : 8;
    const int64_t n = H * W;
    xdemhip_dh_plan* P = new xdemhip_dh_plan();
    P->ctx = P->mem.ctx = ctx; P->dtype = dtype; P->H = H; P->W = W;
    P->n_tiles = (n + RANK_TILE - 1) / RANK_TILE;
    auto fail = [&](int code) { delete P; return code; };
    if (P->n_tiles > 0x7FFFFFFF) return fail(xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_dh_create: raster too large"));
    P->ref = P->mem.keep(ref, (size_t)n * es, memspace, "xdemhip_dh_create");
    P->tba = P->mem.keep(tba, (size_t)n * es, memspace, "xdemhip_dh_create");
    P->inlier = P->mem.keep(inlier, (size_t)n, memspace, "xdemhip_dh_create");
    P->tile_off = P->mem.take<unsigned long long>((size_t)P->n_tiles + 1, "xdemhip_dh_create");
    if (P->mem.rc) return fail(P->mem.rc);
    // (counts only: the mask itself is built by the routes that read it)
    { const int rc_ = launch_valid(P, false); if (rc_) return fail(rc_); }
    hipLaunchKernelGGL(rank_scan_kernel, dim3(1), dim3(1024), 0, ctx->stream, P->tile_off, P->n_tiles, P->tile_off + P->n_tiles);
    if (launched(ctx, "xdemhip_dh_create: kernel")) return fail(XDEMHIP_EHIP);
    unsigned long long total = 0;
    { const int rc_ = xd_d2h(ctx, &total, P->tile_off + P->n_tiles, 8); if (rc_) return fail(rc_); }
    { const int rc_ = xd_sync(ctx); if (rc_) return fail(rc_); }
    P->n_valid = (int64_t)total;
    if (n_valid) *n_valid = P->n_valid;
    *out_plan = P;
    return XDEMHIP_OK;
}

int xdemhip_dh_subsample(xdemhip_dh_plan* P, const int64_t* ranks, int64_t k, int memspace, int64_t* n_drawn) {
    XdFetchScope fetch_scope_(P ? P->ctx : nullptr);
    if (!P) return XDEMHIP_EINVAL;
    xdemhip_ctx* ctx = P->ctx;
    if (!ranks || k < 1 || k > P->n_valid) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_dh_subsample: 1 <= k <= the plan's valid pixels");
    if (memspace != XDEMHIP_HOST && memspace != XDEMHIP_DEVICE) return xd_fail(ctx, XDEMHIP_EINVAL, "bad memspace");
    XD_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    { const int rc_ = ensure_mask(P); if (rc_) return rc_; }
    RankSelect rs(ctx, "xdemhip_dh_subsample");
    unsigned long long total = 0, bad = 0;
    { const int rc_ = rs.run(ranks, k, memspace, P->n_valid, P->valid, P->H * P->W, P->tile_off, &total, &bad); if (rc_) return rc_; }
    if (bad != 0) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_dh_subsample: a rank is outside [0, n_valid)");
    if ((int64_t)total > k) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_dh_subsample: more pixels than ranks");
    // (repeated ranks select one pixel: the list is as long as the distinct ranks)
    int64_t* idx = P->mem.take<int64_t>((size_t)k, "xdemhip_dh_subsample");
    { const int rc_ = P->mem.status(); if (rc_) return rc_; }
    hipLaunchKernelGGL((rank_select_kernel<RankOut::List>), dim3((unsigned)P->n_tiles), dim3(256), 0, ctx->stream, P->valid, P->H * P->W, P->tile_off,
                       rs.mark, rs.off, idx, (uint8_t*)nullptr);
    int rc = launched(ctx, "xdemhip_dh_subsample: kernel");
    if (rc == XDEMHIP_OK) rc = xd_sync(ctx);
    if (rc) { P->mem.drop(idx); return rc; }
    P->mem.drop(P->idx);
    P->idx = idx;
    P->n_idx = (int64_t)total;
    P->drawn = true;
    if (n_drawn) *n_drawn = P->n_idx;
    return XDEMHIP_OK;
}

int xdemhip_dh_poly_moments(xdemhip_dh_plan* P, int order, int64_t row_offset, int64_t H_global, int64_t W_global, double* m_out, double* r_out,
                            int64_t* count) {
    XdFetchScope fetch_scope_(P ? P->ctx : nullptr);
    if (!P) return XDEMHIP_EINVAL;
    xdemhip_ctx* ctx = P->ctx;
    if (order < 0 || order > DH_MAX_ORDER) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_dh_poly_moments: order must be 0..5");
    if (!m_out || !r_out) return xd_fail(ctx, XDEMHIP_EINVAL, "null argument");
    if (row_offset < 0 || H_global < row_offset + P->H || W_global != P->W)
        return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_dh_poly_moments: the plan's rows must lie inside the global grid (same width)");
    const int64_t cnt = P->drawn ? P->n_idx : P->n_valid;
    if (count) *count = cnt;
    if (cnt == 0) return xd_fail(ctx, XDEMHIP_EINVAL, "no valid points");
    XD_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    const int NA = 2 * order + 1, NR = order + 1, NT = NA * NA + NR * NR;
    double ax, bx, ay, by;
    norm_axis(W_global, &ax, &bx);
    norm_axis(H_global, &ay, &by);
    { const int rc_ = P->sums.reserve(P->mem, NT, "xdemhip_dh_poly_moments"); if (rc_) return rc_; }
    int nblocks = 0;
    (void)hipEventRecord(ctx->ev_start, ctx->stream);
    int rc = P->dtype == XDEMHIP_F32 ? launch_moments<float>(P, order, row_offset, ax, bx, ay, by, P->sums.part, &nblocks)
                                     : launch_moments<double>(P, order, row_offset, ax, bx, ay, by, P->sums.part, &nblocks);
    double h[PolyTerms<DH_MAX_ORDER>::NT];
    if (rc == XDEMHIP_OK) rc = fixed_sums_finish(ctx, P->sums, nblocks, NT, "dh_moments_reduce_kernel", h);
    if (rc) return rc;
    memcpy(m_out, h, (size_t)NA * NA * 8);
    memcpy(r_out, h + NA * NA, (size_t)NR * NR * 8);
    return XDEMHIP_OK;
}

int xdemhip_dh_median(xdemhip_dh_plan* P, double* median, int64_t* count) {
    XdFetchScope fetch_scope_(P ? P->ctx : nullptr);
    if (!P) return XDEMHIP_EINVAL;
    xdemhip_ctx* ctx = P->ctx;
    if (!median || !count) return xd_fail(ctx, XDEMHIP_EINVAL, "null argument");
    if ((P->drawn ? P->n_idx : P->n_valid) == 0) return xd_fail(ctx, XDEMHIP_EINVAL, "no valid points");
    XD_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    return P->dtype == XDEMHIP_F32 ? median_typed<float>(P, median, count) : median_typed<double>(P, median, count);
}

int xdemhip_dh_values(xdemhip_dh_plan* P, void* dh_out, int64_t* col_out, int64_t* row_out, int memspace, int64_t* count) {
    XdFetchScope fetch_scope_(P ? P->ctx : nullptr);
    if (!P) return XDEMHIP_EINVAL;
    xdemhip_ctx* ctx = P->ctx;
    if (memspace != XDEMHIP_HOST && memspace != XDEMHIP_DEVICE) return xd_fail(ctx, XDEMHIP_EINVAL, "bad memspace");
    XD_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    int rc = ensure_valid_idx(P);
    if (rc) return rc;
    const int64_t k = P->n_idx;
    if (count) *count = k;
    if (k == 0) return xd_fail(ctx, XDEMHIP_EINVAL, "no valid points");
    const size_t es = P->dtype == XDEMHIP_F32 ? 4 : 8;
    XdBuffers buf(ctx, "xdemhip_dh_values");
    void* d_dh = buf.output(dh_out, (size_t)k * es, memspace);
    int64_t* d_col = buf.output(col_out, (size_t)k * 8, memspace);
    int64_t* d_row = buf.output(row_out, (size_t)k * 8, memspace);
    if (buf.rc) return buf.rc;
    const dim3 g(grid_for(ctx, k, 256, 16));
    if (P->dtype == XDEMHIP_F32)
        hipLaunchKernelGGL((dh_gather_kernel<float>), g, dim3(256), 0, ctx->stream, static_cast<const float*>(P->ref), static_cast<const float*>(P->tba),
                           P->idx, k, P->W, static_cast<float*>(d_dh), d_col, d_row);
    else
        hipLaunchKernelGGL((dh_gather_kernel<double>), g, dim3(256), 0, ctx->stream, static_cast<const double*>(P->ref), static_cast<const double*>(P->tba),
                           P->idx, k, P->W, static_cast<double*>(d_dh), d_col, d_row);
    rc = launched(ctx, "dh_gather_kernel");
    return rc == XDEMHIP_OK ? buf.finish() : rc;
}

int xdemhip_dh_shift_nmad(xdemhip_dh_plan* P, double shift_x, double shift_y, double res_x, double res_y, double nfact, double* median, double* nmad,
                          int64_t* count) {
    XdFetchScope fetch_scope_(P ? P->ctx : nullptr);
    if (!P) return XDEMHIP_EINVAL;
    xdemhip_ctx* ctx = P->ctx;
    if (!median || !nmad || !count) return xd_fail(ctx, XDEMHIP_EINVAL, "null argument");
    if (!(res_x > 0) || !(res_y > 0) || !isfinite(shift_x) || !isfinite(shift_y))
        return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_dh_shift_nmad: finite shifts and positive resolutions");
    *count = 0;
    if ((P->drawn ? P->n_idx : P->n_valid) == 0) return xd_fail(ctx, XDEMHIP_EINVAL, "no valid points");
    XD_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    if (!P->drawn) { const int rc_ = ensure_mask(P); if (rc_) return rc_; }
    const NkGeom g = dh_geom(P, shift_x, shift_y, res_x, res_y);
    XdLocalSelection local(ctx);   // (one process's pixels, as in xdemhip_dh_median)
    return P->dtype == XDEMHIP_F32 ? shift_nmad_typed<float>(P, g, nfact, median, nmad, count)
                                   : shift_nmad_typed<double>(P, g, nfact, median, nmad, count);
}

int xdemhip_dh_shift_values(xdemhip_dh_plan* P, double shift_x, double shift_y, double res_x, double res_y, void* dh_out, int memspace, int64_t* count) {
    XdFetchScope fetch_scope_(P ? P->ctx : nullptr);
    if (!P) return XDEMHIP_EINVAL;
    xdemhip_ctx* ctx = P->ctx;
    if (!dh_out) return xd_fail(ctx, XDEMHIP_EINVAL, "null argument");
    if (memspace != XDEMHIP_HOST && memspace != XDEMHIP_DEVICE) return xd_fail(ctx, XDEMHIP_EINVAL, "bad memspace");
    if (!(res_x > 0) || !(res_y > 0) || !isfinite(shift_x) || !isfinite(shift_y))
        return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_dh_shift_values: finite shifts and positive resolutions");
    XD_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    int rc = ensure_valid_idx(P);
    if (rc) return rc;
    const int64_t k = P->n_idx;
    if (count) *count = k;
    if (k == 0) return xd_fail(ctx, XDEMHIP_EINVAL, "no valid points");
    const size_t es = P->dtype == XDEMHIP_F32 ? 4 : 8;
    void* d_dh = dh_out;
    if (memspace == XDEMHIP_HOST) {   // (through the staging buffer of the evaluations: it holds at least the selection)
        rc = ensure_stage(P, P->drawn ? P->n_idx : P->H * P->W);
        if (rc) return rc;
        d_dh = P->stage;
    }
    const NkGeom g = dh_geom(P, shift_x, shift_y, res_x, res_y);
    const double invW = 1.0 / (double)P->W;
    const dim3 grid(grid_for(ctx, k, 256, 16));
    if (P->dtype == XDEMHIP_F32)
        hipLaunchKernelGGL((dh_shift_list_kernel<float, false>), grid, dim3(256), 0, ctx->stream, static_cast<const float*>(P->ref),
                           static_cast<const float*>(P->tba), P->idx, k, g, invW, static_cast<float*>(d_dh), (uint64_t*)nullptr);
    else
        hipLaunchKernelGGL((dh_shift_list_kernel<double, false>), grid, dim3(256), 0, ctx->stream, static_cast<const double*>(P->ref),
                           static_cast<const double*>(P->tba), P->idx, k, g, invW, static_cast<double*>(d_dh), (uint64_t*)nullptr);
    if (launched(ctx, "dh_shift_list_kernel")) return XDEMHIP_EHIP;
    if (memspace == XDEMHIP_HOST) {
        if (hipMemcpyAsync(dh_out, d_dh, (size_t)k * es, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess) return xd_fail(ctx, XDEMHIP_EHIP, "D2H copy failed");
        rc = xd_sync(ctx);
    }
    return rc;
}

int xdemhip_poly2d_apply(xdemhip_ctx* ctx, const void* elev, int dtype, int64_t H, int64_t W, int64_t row_offset, const double* coeffs, int order,
                         void* out, int memspace) {
    XdFetchScope fetch_scope_(ctx);
    if (!ctx) return XDEMHIP_EINVAL;
    if (!elev || !out || !coeffs) return xd_fail(ctx, XDEMHIP_EINVAL, "null argument");
    if (H < 1 || W < 1 || row_offset < 0) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_poly2d_apply: bad raster size");
    if (order < 0 || order > DH_MAX_ORDER) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_poly2d_apply: order must be 0..5");
    if (dtype != XDEMHIP_F32 && dtype != XDEMHIP_F64) return xd_fail(ctx, XDEMHIP_EINVAL, "dtype must be float32 or float64");
    if (memspace != XDEMHIP_HOST && memspace != XDEMHIP_DEVICE) return xd_fail(ctx, XDEMHIP_EINVAL, "bad memspace");
    XD_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    const int K = order + 1;
    PolyCoeffs cf;
    memset(&cf, 0, sizeof cf);
    for (int i = 0; i < K * K; ++i) cf.c[i] = coeffs[i];
    const size_t bytes = (size_t)(H * W) * (dtype == XDEMHIP_F32 ? 4 : 8);
    XdBuffers buf(ctx, "xdemhip_poly2d_apply");
    const void* d_in = buf.input(elev, bytes, memspace);
    void* d_out = buf.output(out, bytes, memspace);
    if (buf.rc) return buf.rc;
    (void)hipEventRecord(ctx->ev_start, ctx->stream);
    int rc = dtype == XDEMHIP_F32 ? launch_apply<float>(ctx, static_cast<const float*>(d_in), H, W, row_offset, cf, K, static_cast<float*>(d_out))
                                  : launch_apply<double>(ctx, static_cast<const double*>(d_in), H, W, row_offset, cf, K, static_cast<double*>(d_out));
    (void)hipEventRecord(ctx->ev_stop, ctx->stream);
    ctx->timed = (rc == XDEMHIP_OK);
    return rc == XDEMHIP_OK ? buf.finish() : rc;
}

}  // extern "C"
