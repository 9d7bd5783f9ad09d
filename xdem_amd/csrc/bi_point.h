// bi_point.h -- the bilinear taps of nk_geom.h at an ARBITRARY float64 (row, col) instead of one shift for the whole grid (the LZD
// passes of rigid.hip move every pixel by a matrix), and the linear interpolation of SciPy's RegularGridInterpolator that upstream's
// rotation-capable regrid calls.
#pragma once
#include "nk_geom.h"

namespace xd {

// one axis of a point tap: bi_axis with the position given.  A position that is not a number or lies a pixel and more outside the raster
// is moved to -2 first (outside under every rule), so that no cast to an integer overflows.
__device__ __forceinline__ BiAxis bi_axis_at(double pos, int64_t extent, int rule) {
    BiAxis a;
    a.pos = (pos >= -1.0 && pos <= (double)extent) ? pos : -2.0;
    const double k0f = floor(a.pos);
    a.f = t_sub(a.pos, k0f);
    a.k0 = (int64_t)k0f;
    a.d1 = (a.f == 0.0 && (rule == 1 || a.k0 + 1 >= extent)) ? 0 : 1;
    a.in = a.k0 >= 0 && a.k0 + a.d1 < extent;
    return a;
}

// bilinear(img)(row, col): float64 weights, the arithmetic and the four nodata rules of bi_value, rounded to the raster dtype; false
// (and NaN) where the rule says nodata.  g.roff must be 0 (whole rasters).
template <typename T> __device__ __forceinline__ bool bi_point(const NkGeom& g, const T* __restrict__ img, double row, double col, T& out) {
    const BiTap t = bi_combine(g, bi_axis_at(row, g.H, g.rule), bi_axis_at(col, g.W, g.rule));
    const BiVals<T> v = bi_load<T>(img, t);
    const bool ok = bi_value<T>(g, img, t, v.a00, v.a01, v.a10, v.a11, out);
    if (!ok) out = (T)NAN;
    return ok;
}

// scipy.interpolate.RegularGridInterpolator(method="linear", bounds_error=False) on the pixel grid, in float64: NaN outside
// [0, n - 1], the cell index clipped to [0, n - 2], NaN if any of the cell's four nodes is non-finite (zero weights included).
// SciPy takes the cell [k, k + 1) along an ascending axis; upstream hands it the y axis, which ascends against the rows, so a position
// exactly on row k belongs to the cell of rows [k - 1, k] and one exactly on column k to the cell of columns [k, k + 1].  H, W >= 2.
template <typename T> __device__ __forceinline__ double rgi_linear(const T* __restrict__ img, int64_t H, int64_t W, double row, double col) {
    if (!(row >= 0.0 && row <= (double)(H - 1) && col >= 0.0 && col <= (double)(W - 1))) return NAN;
    int64_t i0 = (int64_t)ceil(row) - 1, j0 = (int64_t)floor(col);
    i0 = i0 < 0 ? 0 : i0;
    j0 = j0 > W - 2 ? W - 2 : j0;
    const double fr = row - (double)i0, fc = col - (double)j0;
    const T* q = img + i0 * W + j0;
    const T a00 = q[0], a01 = q[1], a10 = q[W], a11 = q[W + 1];
    if (!(t_finite(a00) && t_finite(a01) && t_finite(a10) && t_finite(a11))) return NAN;
    const double gr = 1.0 - fr, gc = 1.0 - fc;
    return (((double)a00 * gr) * gc + ((double)a01 * gr) * fc + ((double)a10 * fr) * gc) + ((double)a11 * fr) * fc;
}

}  // namespace xd
