// rigid_geom.h -- what the rigid coregistrations (LZD in rigid.hip, ICP in icp.hip) share on the grid: np.gradient's stencil, the
// matrix applied to a point, the finiteness test of a float64 and the check of a call's transform.  No contraction (-ffp-contract=off).
#pragma once
#include <math.h>

#include "common.h"
#include "select_run.h"

namespace xd {

__device__ __forceinline__ bool d_finite(double v) { return fabs(v) <= 1.79769313486231570e308; }

// np.gradient(ref) at pixel (r, c) in the raster dtype: central differences, one-sided at the borders; gx along the columns, gy along
// the rows.  H, W >= 2.
template <typename T>
__device__ __forceinline__ void np_gradient_at(const T* __restrict__ ref, int64_t H, int64_t W, int64_t r, int64_t c, T& gx, T& gy) {
    const int64_t p = r * W + c;
    if (c == 0) gx = t_sub(ref[p + 1], ref[p]);
    else if (c == W - 1) gx = t_sub(ref[p], ref[p - 1]);
    else gx = t_div(t_sub(ref[p + 1], ref[p - 1]), (T)2);
    if (r == 0) gy = t_sub(ref[p + W], ref[p]);
    else if (r == H - 1) gy = t_sub(ref[p], ref[p - W]);
    else gy = t_div(t_sub(ref[p + W], ref[p - W]), (T)2);
}

// rows 0..2 of a 4 x 4 matrix, and M p with the products as explicit sums in the order ((m0 x + m1 y) + m2 z) + m3
struct Mat12 { double m[12]; };
__device__ __forceinline__ void mat12_apply(const double* m, double x, double y, double z, double& ox, double& oy, double& oz) {
    ox = ((m[0] * x + m[1] * y) + m[2] * z) + m[3];
    oy = ((m[4] * x + m[5] * y) + m[6] * z) + m[7];
    oz = ((m[8] * x + m[9] * y) + m[10] * z) + m[11];
}

// the 6-tuple geotransform of a call: (a, 0, c, 0, e, f), north-up
inline int check_transform(xdemhip_ctx* ctx, const double* t, const char* who) {
    if (!t) return xd_fail(ctx, XDEMHIP_EINVAL, "null argument");
    if (t[1] != 0.0 || t[3] != 0.0 || !(fabs(t[0]) > 0) || !(fabs(t[4]) > 0) || !isfinite(t[0]) || !isfinite(t[4]) || !isfinite(t[2]) || !isfinite(t[5]))
        return xd_fail(ctx, XDEMHIP_EINVAL, std::string(who) + ": transform6 = (a, 0, c, 0, e, f) with finite entries and a, e != 0");
    return XDEMHIP_OK;
}

}  // namespace xd
