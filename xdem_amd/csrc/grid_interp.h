// grid_interp.h -- the per-point arithmetic of the multilinear interpolant on a regular grid (scipy.interpolate.
// RegularGridInterpolator, method="linear", bounds_error=False, fill_value=None), shared by xdemhip_interp_grid_linear
// (binstats.hip) and the fused correction pass xdemhip_corr_apply (bincorr.hip): one source, the same float64 operations in the
// same order in both (their translation units are built without contraction).
#pragma once
#include "common.h"

namespace xd {

struct GridShape {
    int nd;
    int n[8], off[8], stride[8];   // points per axis, the axis' offset in the concatenated axes, C-order strides of the values
};

// `ax`: the concatenated axes (ascending), `V`: the grid values in C order, x_of(d): coordinate d of the point.  Linear
// extrapolation from the edge intervals outside the grid; *isnan_any: a coordinate is NaN (the callers write NaN then).
// MAXD >= S.nd bounds the per-dimension values: up to 4 the loops over the dimensions are unrolled with a guard, so that they
// stay in registers; the operations and their order are the same either way.
template <int MAXD, typename XF>
__device__ __forceinline__ double grid_linear_eval(const GridShape& S, const double* ax, const double* V, XF x_of, bool* isnan_any) {
    int base = 0;
    double y[MAXD];
    bool any = false;
    auto locate = [&](int d) {
        const double x = x_of(d);
        any |= (x != x);
        const double* g = ax + S.off[d];
        const int m = S.n[d];
        // interval i with g[i] <= x < g[i+1], clipped to [0, m-2] (x == g[m-1] belongs to the last interval)
        int lo = 0, hi = m - 1;
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (g[mid] <= x) lo = mid; else hi = mid;
        }
        y[d] = (x - g[lo]) / (g[lo + 1] - g[lo]);
        base += lo * S.stride[d];
    };
    if constexpr (MAXD <= 4) {
#pragma unroll
        for (int d = 0; d < MAXD; ++d)
            if (d < S.nd) locate(d);
    } else {
#pragma unroll 1
        for (int d = 0; d < S.nd; ++d) locate(d);
    }
    // hypercube corners in itertools.product order (first dimension slowest), weights multiplied left to right
    double value = 0.0;
    const int corners = 1 << S.nd;
    for (int c = 0; c < corners; ++c) {
        double wgt = 1.0;
        int idx = base;
        if constexpr (MAXD <= 4) {
#pragma unroll
            for (int d = 0; d < MAXD; ++d)
                if (d < S.nd) {
                    const int up = (c >> (S.nd - 1 - d)) & 1;
                    wgt = wgt * (up ? y[d] : (1.0 - y[d]));
                    idx += up * S.stride[d];
                }
        } else {
            for (int d = 0; d < S.nd; ++d) {
                const int up = (c >> (S.nd - 1 - d)) & 1;
                wgt = wgt * (up ? y[d] : (1.0 - y[d]));
                idx += up * S.stride[d];
            }
        }
        value = value + V[idx] * wgt;
    }
    *isnan_any = any;
    return value;
}

}  // namespace xd
