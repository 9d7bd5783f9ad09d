// biascorr.hip -- Deramp / VerticalShift on gfx950: the passes of the two methods that touch the grids.
//
// Replaces, for raster-raster input (xdem/coreg):
//   valid = inlier & isfinite(ref) & isfinite(tba)                      base.py:652-663       -> dh_valid_kernel (counts once per plan)
//   random subsample of the valid pixels                                base.py:577-617       -> rank_select.h (ranks -> pixels)
//   curve_fit(polynomial_2d, (xx, yy), ref - tba) over the valid pixels biascorr.py:195, 621-745, base.py:978-985
//                                                                                             -> least-squares moments (dh_moments_*)
//   np.median(ref - tba) over the valid pixels                          affine.py:721-770     -> radix selection (select_run.h)
//   elev + polyval2d(xx, yy, c), cast to the input dtype                biascorr.py:262-311, base.py:491 -> poly2d_apply_kernel
// The (order+1)^2 least-squares system is solved on the host (xdem_amd/biascorr.py).
//
// The moments are taken in normalised coordinates u = (x - cx) / sx, v = (y - cy) / sy with cx = sx = (W_global - 1) / 2 and
// cy = sy = (H_global - 1) / 2 (a half-width of 0 is taken as 1): x = column, y = row_offset + row, as np.meshgrid(arange(W),
// arange(H)) numbers them.  In raw pixel coordinates the normal equations of order 2 on a 2000 x 3000 grid are useless; in
// normalised ones their condition number is ~2e2 (order 2) to ~1e5 (order 4).  Everything is accumulated in float64 and
// combined in a fixed order: two calls return the same bits.
#include <math.h>
#include <string.h>

#include <vector>

#include "common.h"
#include "select.h"
#include "select_run.h"
#include "rank_select.h"

struct xdemhip_dh_plan {
    xdemhip_ctx* ctx = nullptr;
    int dtype = XDEMHIP_F32;
    int64_t H = 0, W = 0;
    bool own_inputs = false;
    void* ref = nullptr;
    void* tba = nullptr;
    uint8_t* inlier = nullptr;
    uint8_t* valid = nullptr;                 // n bytes: inlier & finite(ref) & finite(tba)
    unsigned long long* tile_off = nullptr;   // exclusive offsets of the valid pixels per tile (n_tiles + 1 words)
    int64_t n_tiles = 0;
    int64_t n_valid = 0;
    int64_t* idx = nullptr;                   // selected pixels (flat indexes, raster order): the drawn ones, or all valid ones on demand
    int64_t n_idx = 0;
    bool drawn = false;                       // xdemhip_dh_subsample was called: the drawn pixels are the selection
};

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
// four waves in order) and lane t < NT multiplies its row sum by the power of v of the term it owns.
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
        for (int e = 0; e < NS; ++e) {
            double x = s[e];
            for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off, 64);
            s[e] = x;
        }
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

// per-workgroup partials -> totals: one workgroup per term, lane l adds the partials of workgroups l, l + 256, ... in order, then a
// fixed tree over the lanes (the same bits every call)
__global__ __launch_bounds__(256) void dh_moments_reduce_kernel(const double* __restrict__ part, int nblocks, int nt, double* __restrict__ out) {
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
    if (hipGetLastError() != hipSuccess) return xd_fail(ctx, XDEMHIP_EHIP, "poly2d_apply_kernel launch failed");
    return XDEMHIP_OK;
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
        int64_t nb = (int64_t)ctx->num_cu * 8;
        if (nb > P->H) nb = P->H;
        *nblocks = (int)nb;
        const bool vec = (P->W % 4 == 0) && ((uintptr_t)P->ref % 16 == 0) && ((uintptr_t)P->tba % 16 == 0) &&
                         (P->inlier == nullptr || (uintptr_t)P->inlier % 4 == 0);
        if (vec)
            hipLaunchKernelGGL((dh_moments_rows_kernel<T, K, true>), dim3((unsigned)nb), dim3(256), 0, ctx->stream, static_cast<const T*>(P->ref),
                               static_cast<const T*>(P->tba), P->inlier, P->H, P->W, row_offset, ax, bx, ay, by, d_part);
        else
            hipLaunchKernelGGL((dh_moments_rows_kernel<T, K, false>), dim3((unsigned)nb), dim3(256), 0, ctx->stream, static_cast<const T*>(P->ref),
                               static_cast<const T*>(P->tba), P->inlier, P->H, P->W, row_offset, ax, bx, ay, by, d_part);
    }
    return hipGetLastError() == hipSuccess ? XDEMHIP_OK : xd_fail(ctx, XDEMHIP_EHIP, "moments kernel launch failed");
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
    return hipGetLastError() == hipSuccess ? XDEMHIP_OK : xd_fail(P->ctx, XDEMHIP_EHIP, "dh_valid_kernel launch failed");
}

// the valid mask, built on first need (the subsample and values routes; the whole-raster moments and median recompute validity).  The
// tile counts are written again: the same numbers as at creation, so the scanned offsets stay what they were.
int ensure_mask(xdemhip_dh_plan* P) {
    if (P->valid) return XDEMHIP_OK;
    xdemhip_ctx* ctx = P->ctx;
    const int64_t n = P->H * P->W;
    if (hipMalloc(reinterpret_cast<void**>(&P->valid), (size_t)n) != hipSuccess) {
        (void)hipGetLastError();
        P->valid = nullptr;
        return xd_fail(ctx, XDEMHIP_ENOMEM, "hipMalloc failed (valid mask)");
    }
    const int rc = launch_valid(P, true);
    if (rc) return rc;
    hipLaunchKernelGGL(rank_scan_kernel, dim3(1), dim3(1024), 0, ctx->stream, P->tile_off, P->n_tiles, P->tile_off + P->n_tiles);
    return hipGetLastError() == hipSuccess ? XDEMHIP_OK : xd_fail(ctx, XDEMHIP_EHIP, "dh_scan_kernel launch failed");
}

// the list of all valid pixels (raster order), for the values route of a plan that was never subsampled
int ensure_valid_idx(xdemhip_dh_plan* P) {
    if (P->drawn || P->idx) return XDEMHIP_OK;
    xdemhip_ctx* ctx = P->ctx;
    { const int rc = ensure_mask(P); if (rc) return rc; }
    if (hipMalloc(reinterpret_cast<void**>(&P->idx), (size_t)(P->n_valid > 0 ? P->n_valid : 1) * 8) != hipSuccess) {
        (void)hipGetLastError();
        P->idx = nullptr;
        return xd_fail(ctx, XDEMHIP_ENOMEM, "hipMalloc failed (valid pixel list)");
    }
    hipLaunchKernelGGL((rank_select_kernel<RankOut::List>), dim3((unsigned)P->n_tiles), dim3(256), 0, ctx->stream, P->valid, P->H * P->W,
                       (const unsigned long long*)nullptr, (const uint8_t*)nullptr, P->tile_off, P->idx, (uint8_t*)nullptr);
    if (hipGetLastError() != hipSuccess) return xd_fail(ctx, XDEMHIP_EHIP, "dh_sel_kernel launch failed");
    P->n_idx = P->n_valid;
    return XDEMHIP_OK;
}

template <typename T>
int median_typed(xdemhip_dh_plan* P, double* median, int64_t* count) {
    typedef typename KeyT<T>::type K;
    xdemhip_ctx* ctx = P->ctx;
    const int64_t n = P->drawn ? P->n_idx : P->H * P->W;
    T* d = nullptr;
    void* scratch = nullptr;
    auto cleanup = [&]() { if (d) (void)hipFree(d); if (scratch) (void)hipFree(scratch); };
    if (hipMalloc(reinterpret_cast<void**>(&d), (size_t)n * sizeof(T)) != hipSuccess || hipMalloc(&scratch, scratch_size(1)) != hipSuccess) {
        (void)hipGetLastError();
        cleanup();
        return xd_fail(ctx, XDEMHIP_ENOMEM, "hipMalloc failed (xdemhip_dh_median)");
    }
    const dim3 g(grid_for(ctx, n, 256, 16));
    if (P->drawn)
        hipLaunchKernelGGL((dh_gather_kernel<T>), g, dim3(256), 0, ctx->stream, static_cast<const T*>(P->ref), static_cast<const T*>(P->tba), P->idx, n,
                           P->W, d, (int64_t*)nullptr, (int64_t*)nullptr);
    else
        hipLaunchKernelGGL((dh_dense_kernel<T>), g, dim3(256), 0, ctx->stream, static_cast<const T*>(P->ref), static_cast<const T*>(P->tba), P->inlier, n, d);
    if (hipGetLastError() != hipSuccess) { cleanup(); return xd_fail(ctx, XDEMHIP_EHIP, "dh kernel launch failed"); }
    std::vector<SelResult<K>> r;
    const xdemhip_allreduce_fn hook = ctx->allreduce;   // (one process's pixels: a local selection)
    ctx->allreduce = nullptr;
    SelWorkspace ws;
    if (n >= SEL_BRACKET_MIN_N) (void)sel_ws_create(ctx, n, sizeof(T), 1, ws);  // (on failure: plain selection)
    int rc = run_select<T>(ctx, d, nullptr, n, 1, static_cast<unsigned char*>(scratch), r, &ws);
    ctx->allreduce = hook;
    if (rc == XDEMHIP_OK) {
        *count = (int64_t)r[0].st.count;
        *median = median_from<T>(r[0]);
    }
    (void)hipStreamSynchronize(ctx->stream);
    sel_ws_free(ws);
    cleanup();
    return rc;
}

int upload_or_use(xdemhip_ctx* ctx, const void* src, size_t bytes, int memspace, void** dptr, bool* own) {
    *own = false;
    if (memspace == XDEMHIP_DEVICE) { *dptr = const_cast<void*>(src); return XDEMHIP_OK; }
    if (hipMalloc(dptr, bytes) != hipSuccess) { (void)hipGetLastError(); *dptr = nullptr; return xd_fail(ctx, XDEMHIP_ENOMEM, "hipMalloc failed"); }
    *own = true;
    if (hipMemcpyAsync(*dptr, src, bytes, hipMemcpyHostToDevice, ctx->stream) != hipSuccess) return xd_fail(ctx, XDEMHIP_EHIP, "H2D copy failed");
    return XDEMHIP_OK;
}

inline void norm_axis(int64_t n_global, double* a, double* b) {
    double half = 0.5 * (double)(n_global - 1);
    const double centre = half;
    if (!(half > 0)) half = 1.0;
    *a = 1.0 / half;
    *b = -centre / half;
}

}  // namespace
}  // namespace xd

using namespace xd;

extern "C" {

void xdemhip_dh_destroy(xdemhip_dh_plan* P) {
    if (!P) return;
    (void)hipSetDevice(P->ctx->device);
    if (P->own_inputs) {
        if (P->ref) (void)hipFree(P->ref);
        if (P->tba) (void)hipFree(P->tba);
        if (P->inlier) (void)hipFree(P->inlier);
    }
    if (P->valid) (void)hipFree(P->valid);
    if (P->tile_off) (void)hipFree(P->tile_off);
    if (P->idx) (void)hipFree(P->idx);
    delete P;
}

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
    P->ctx = ctx; P->dtype = dtype; P->H = H; P->W = W;
    P->n_tiles = (n + RANK_TILE - 1) / RANK_TILE;
    auto fail = [&](int code) { xdemhip_dh_destroy(P); return code; };
    if (P->n_tiles > 0x7FFFFFFF) return fail(xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_dh_create: raster too large"));
    if (memspace == XDEMHIP_HOST) {
        P->own_inputs = true;
        bool own = false;
        int rc = upload_or_use(ctx, ref, (size_t)n * es, memspace, &P->ref, &own);
        if (rc == XDEMHIP_OK) rc = upload_or_use(ctx, tba, (size_t)n * es, memspace, &P->tba, &own);
        if (rc == XDEMHIP_OK && inlier) {
            void* d = nullptr;
            rc = upload_or_use(ctx, inlier, (size_t)n, memspace, &d, &own);
            P->inlier = static_cast<uint8_t*>(d);
        }
        if (rc) return fail(rc);
    } else {
        P->ref = const_cast<void*>(ref);
        P->tba = const_cast<void*>(tba);
        P->inlier = const_cast<uint8_t*>(inlier);
    }
    if (hipMalloc(reinterpret_cast<void**>(&P->tile_off), (size_t)(P->n_tiles + 1) * 8) != hipSuccess) {
        (void)hipGetLastError();
        return fail(xd_fail(ctx, XDEMHIP_ENOMEM, "hipMalloc failed (xdemhip_dh_create)"));
    }
    // (counts only: the mask itself is built by the routes that read it)
    { const int rc_ = launch_valid(P, false); if (rc_) return fail(rc_); }
    hipLaunchKernelGGL(rank_scan_kernel, dim3(1), dim3(1024), 0, ctx->stream, P->tile_off, P->n_tiles, P->tile_off + P->n_tiles);
    if (hipGetLastError() != hipSuccess) return fail(xd_fail(ctx, XDEMHIP_EHIP, "xdemhip_dh_create: kernel launch failed"));
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
    RankSelect rs;
    unsigned long long total = 0, bad = 0;
    { const int rc_ = rs.run(ctx, "xdemhip_dh_subsample", ranks, k, memspace, P->n_valid, P->valid, P->H * P->W, P->tile_off, &total, &bad); if (rc_) return rc_; }
    if (bad != 0) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_dh_subsample: a rank is outside [0, n_valid)");
    if ((int64_t)total > k) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_dh_subsample: more pixels than ranks");
    // (repeated ranks select one pixel: the list is as long as the distinct ranks)
    int64_t* idx = nullptr;
    if (hipMalloc(reinterpret_cast<void**>(&idx), (size_t)k * 8) != hipSuccess) {
        (void)hipGetLastError();
        return xd_fail(ctx, XDEMHIP_ENOMEM, "hipMalloc failed (xdemhip_dh_subsample)");
    }
    hipLaunchKernelGGL((rank_select_kernel<RankOut::List>), dim3((unsigned)P->n_tiles), dim3(256), 0, ctx->stream, P->valid, P->H * P->W, P->tile_off,
                       rs.mark, rs.off, idx, (uint8_t*)nullptr);
    int rc = hipGetLastError() == hipSuccess ? XDEMHIP_OK : xd_fail(ctx, XDEMHIP_EHIP, "xdemhip_dh_subsample: kernel launch failed");
    if (rc == XDEMHIP_OK) rc = xd_sync(ctx);
    if (rc) { (void)hipFree(idx); return rc; }
    if (P->idx) (void)hipFree(P->idx);
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
    const int64_t max_blocks = (int64_t)ctx->num_cu * 8;
    double* d_part = nullptr;
    if (hipMalloc(reinterpret_cast<void**>(&d_part), (size_t)(max_blocks * NT + NT) * 8) != hipSuccess) {
        (void)hipGetLastError();
        return xd_fail(ctx, XDEMHIP_ENOMEM, "hipMalloc failed (xdemhip_dh_poly_moments)");
    }
    int nblocks = 0;
    (void)hipEventRecord(ctx->ev_start, ctx->stream);
    int rc = P->dtype == XDEMHIP_F32 ? launch_moments<float>(P, order, row_offset, ax, bx, ay, by, d_part, &nblocks)
                                     : launch_moments<double>(P, order, row_offset, ax, bx, ay, by, d_part, &nblocks);
    if (rc == XDEMHIP_OK) {
        double* d_out = d_part + max_blocks * NT;
        hipLaunchKernelGGL(dh_moments_reduce_kernel, dim3((unsigned)NT), dim3(256), 0, ctx->stream, d_part, nblocks, NT, d_out);
        if (hipGetLastError() != hipSuccess) rc = xd_fail(ctx, XDEMHIP_EHIP, "dh_moments_reduce_kernel launch failed");
        (void)hipEventRecord(ctx->ev_stop, ctx->stream);
        ctx->timed = (rc == XDEMHIP_OK);
        std::vector<double> h(NT);
        if (rc == XDEMHIP_OK) rc = xd_d2h(ctx, h.data(), d_out, (size_t)NT * 8);
        if (rc == XDEMHIP_OK) rc = xd_sync(ctx);
        if (rc == XDEMHIP_OK) {
            memcpy(m_out, h.data(), (size_t)NA * NA * 8);
            memcpy(r_out, h.data() + NA * NA, (size_t)NR * NR * 8);
        }
    }
    (void)hipStreamSynchronize(ctx->stream);
    (void)hipFree(d_part);
    return rc;
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
    void* d_dh = nullptr;
    int64_t *d_col = nullptr, *d_row = nullptr;
    bool own = memspace == XDEMHIP_HOST;
    if (own) {
        if ((dh_out && hipMalloc(&d_dh, (size_t)k * es) != hipSuccess) || (col_out && hipMalloc(reinterpret_cast<void**>(&d_col), (size_t)k * 8) != hipSuccess) ||
            (row_out && hipMalloc(reinterpret_cast<void**>(&d_row), (size_t)k * 8) != hipSuccess)) {
            (void)hipGetLastError();
            rc = xd_fail(ctx, XDEMHIP_ENOMEM, "hipMalloc failed (xdemhip_dh_values)");
        }
    } else {
        d_dh = dh_out; d_col = col_out; d_row = row_out;
    }
    if (rc == XDEMHIP_OK) {
        const dim3 g(grid_for(ctx, k, 256, 16));
        if (P->dtype == XDEMHIP_F32)
            hipLaunchKernelGGL((dh_gather_kernel<float>), g, dim3(256), 0, ctx->stream, static_cast<const float*>(P->ref), static_cast<const float*>(P->tba),
                               P->idx, k, P->W, static_cast<float*>(d_dh), d_col, d_row);
        else
            hipLaunchKernelGGL((dh_gather_kernel<double>), g, dim3(256), 0, ctx->stream, static_cast<const double*>(P->ref), static_cast<const double*>(P->tba),
                               P->idx, k, P->W, static_cast<double*>(d_dh), d_col, d_row);
        if (hipGetLastError() != hipSuccess) rc = xd_fail(ctx, XDEMHIP_EHIP, "dh_gather_kernel launch failed");
    }
    if (rc == XDEMHIP_OK && own) {
        if (dh_out && hipMemcpyAsync(dh_out, d_dh, (size_t)k * es, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess) rc = xd_fail(ctx, XDEMHIP_EHIP, "D2H copy failed");
        if (rc == XDEMHIP_OK && col_out && hipMemcpyAsync(col_out, d_col, (size_t)k * 8, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess) rc = xd_fail(ctx, XDEMHIP_EHIP, "D2H copy failed");
        if (rc == XDEMHIP_OK && row_out && hipMemcpyAsync(row_out, d_row, (size_t)k * 8, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess) rc = xd_fail(ctx, XDEMHIP_EHIP, "D2H copy failed");
    }
    if (own) {
        (void)hipStreamSynchronize(ctx->stream);
        if (d_dh) (void)hipFree(d_dh);
        if (d_col) (void)hipFree(d_col);
        if (d_row) (void)hipFree(d_row);
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
    void *d_in = nullptr, *d_out = out;
    bool own = false;
    int rc = upload_or_use(ctx, elev, bytes, memspace, &d_in, &own);
    if (rc == XDEMHIP_OK && memspace == XDEMHIP_HOST && hipMalloc(&d_out, bytes) != hipSuccess) {
        (void)hipGetLastError();
        d_out = nullptr;
        rc = xd_fail(ctx, XDEMHIP_ENOMEM, "hipMalloc failed (xdemhip_poly2d_apply)");
    }
    if (rc == XDEMHIP_OK) {
        (void)hipEventRecord(ctx->ev_start, ctx->stream);
        rc = dtype == XDEMHIP_F32 ? launch_apply<float>(ctx, static_cast<const float*>(d_in), H, W, row_offset, cf, K, static_cast<float*>(d_out))
                                  : launch_apply<double>(ctx, static_cast<const double*>(d_in), H, W, row_offset, cf, K, static_cast<double*>(d_out));
        (void)hipEventRecord(ctx->ev_stop, ctx->stream);
        ctx->timed = (rc == XDEMHIP_OK);
    }
    if (rc == XDEMHIP_OK && memspace == XDEMHIP_HOST) {
        if (hipMemcpyAsync(out, d_out, bytes, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess) rc = xd_fail(ctx, XDEMHIP_EHIP, "D2H copy failed");
        if (rc == XDEMHIP_OK) rc = xd_sync(ctx);
    }
    if (memspace == XDEMHIP_HOST) {
        (void)hipStreamSynchronize(ctx->stream);
        if (own && d_in) (void)hipFree(d_in);
        if (d_out) (void)hipFree(d_out);
    }
    return rc;
}

}  // extern "C"
