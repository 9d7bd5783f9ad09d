// nk_aux.h -- what the Nuth-Kaab plan over two rasters (nuthkaab.hip) and the plan over a raster and a point cloud (ptsplan.hip)
// share: the auxiliary planes (slope tangent, aspect, valid mask), the min / max aspect record of a dh pass, SciPy's bin edges and
// its rule for samples on the last edge.  FOR TRANSLATION UNITS BUILT WITH -ffp-contract=off.
#pragma once
#include <math.h>

#include "common.h"
#include "select.h"
#include "select_run.h"
#include "nk_geom.h"

namespace xd {

// ---- aux: gradient -> slope tangent, aspect, valid mask --------------------------------------------------------
// One pixel (i, j) of an H x W raster held row-major in `ref`, the pixel at index p (rows W apart): slope tangent and aspect from np.gradient
// with unit spacing, and whether the pixel is valid.  `tv` is the to-be-aligned sample of the pixel, `inl` its inlier flag.
template <typename T>
__device__ __forceinline__ bool nk_aux_pixel(const T* __restrict__ ref, int64_t p, int64_t i, int64_t j, int64_t H, int64_t W, T tv, bool inl,
                                             T& st, T& as) {
    const T c = ref[p];
    T gy, gx;
    // np.gradient, unit spacing: central differences inside, one-sided on the borders of the RASTER
    if (i == 0) gy = t_sub(ref[p + W], c);
    else if (i == H - 1) gy = t_sub(c, ref[p - W]);
    else gy = t_div(t_sub(ref[p + W], ref[p - W]), (T)2);
    if (j == 0) gx = t_sub(ref[p + 1], c);
    else if (j == W - 1) gx = t_sub(c, ref[p - 1]);
    else gx = t_div(t_sub(ref[p + 1], ref[p - 1]), (T)2);
    st = t_sqrt(t_add(t_mul(gx, gx), t_mul(gy, gy)));
    // aspect = arctan2(-gx, gy) + pi: correctly rounded to the DEM dtype from the float64 arctangent
    as = (T)atan2(-(double)gx, (double)gy);
    as = t_add(as, (T)3.14159265358979323846);
    if (fabs((double)st) <= 1e-8) st = (T)NAN;  // np.isclose(slope_tan, 0) -> NaN (affine.py:578-579)
    return inl && t_finite(c) && t_finite(tv) && t_finite(st) && t_finite(as);
}

template <typename T>
__global__ __launch_bounds__(256) void nk_aux_kernel(const T* __restrict__ ref, const T* __restrict__ tba,
                                                     const uint8_t* __restrict__ inlier, NkGeom g,
                                                     T* __restrict__ slope_tan, T* __restrict__ aspect,
                                                     uint8_t* __restrict__ valid, unsigned long long* n_valid,
                                                     int64_t row0, int64_t row1) {
    // raster rows [row0, row1): blockIdx.x tiles the columns, blockIdx.y strides over the rows
    unsigned long long local = 0;
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t H = g.H, W = g.W;
    if (j < W)
    for (int64_t i = row0 + blockIdx.y; i < row1; i += gridDim.y) {
        const int64_t p = (i - g.roff) * W + j;
        T st, as;
        const bool ok = nk_aux_pixel<T>(ref, p, i, j, H, W, tba[p], inlier ? inlier[p] != 0 : true, st, as);
        slope_tan[p] = st;
        aspect[p] = as;
        valid[p] = ok ? 1 : 0;
        local += ok ? 1 : 0;
    }
    // wave reduction then one atomic per wave
    for (int off = 32; off > 0; off >>= 1) local += __shfl_down(local, off);
    if ((threadIdx.x & 63) == 0 && local) atomicAdd(n_valid, local);
}

// ---- min / max aspect over the finite dh of a pass -----------------------------------------------------------------
struct DhStats {
    uint64_t asp_min, asp_max;  // order-preserving keys (widened to 64 bit) of min / max aspect among finite dh
};

// np.linspace(smin, smax, nb + 1) in double (k * step + start, end point forced), cast to T -- SciPy's _bin_edges
template <typename T> __host__ __device__ inline void make_edges_into(double smin, double smax, int nb, T* e) {
    if (smin == smax) { smin -= 0.5; smax += 0.5; }
    const double step = (smax - smin) / nb;
    for (int k = 0; k <= nb; ++k) e[k] = (T)((double)k * step + smin);
    e[nb] = (T)smax;
}

// SciPy's rule for samples at or beyond the rightmost edge (_binned_statistic.py:_bin_numbers): such a sample joins the last
// bin iff np.around(x, decimal) == np.around(last_edge, decimal), decimal = int(-log10(min edge spacing)) + 6, evaluated in
// the sample dtype.  With the automatic edges the largest sample IS the last edge (decimal = NK_AUTO_EDGES: always true);
// explicit edges carry their decimal (computed by the caller exactly like SciPy).
constexpr int NK_AUTO_EDGES = -100000;
template <typename T> __device__ __forceinline__ bool on_last_edge(T x, T last, int decimal) {
    if (decimal == NK_AUTO_EDGES) return true;
    const T p10 = (T)pow(10.0, (double)(decimal < 0 ? -decimal : decimal));
    const T rx = decimal >= 0 ? rint(x * p10) / p10 : rint(x / p10) * p10;
    const T rl = decimal >= 0 ? rint(last * p10) / p10 : rint(last / p10) * p10;
    return rx == rl;
}

// np.digitize(x, e) - 1 = (number of edges <= x) - 1 against the nb + 1 dtype-rounded edges e (LDS or registers): an arithmetic guess
// on the uniform grid, then an exact walk (a step or two); a sample on the last edge joins the last bin by on_last_edge.  0xFFFF =
// outside every bin.
template <typename T> __device__ __forceinline__ uint16_t aspect_bin(T x, const T* e, int nb, double inv_width, int last_decimal) {
    int idx = (int)(((double)x - (double)e[0]) * inv_width);
    idx = idx < 0 ? 0 : (idx > nb ? nb : idx);
    while (idx > 0 && !(e[idx] <= x)) --idx;
    while (idx < nb && e[idx + 1] <= x) ++idx;
    if (!(e[0] <= x)) idx = -1;
    if (idx == nb && on_last_edge<T>(x, e[nb], last_decimal)) idx = nb - 1;
    return (idx >= 0 && idx < nb) ? (uint16_t)idx : (uint16_t)0xFFFF;
}

}  // namespace xd
