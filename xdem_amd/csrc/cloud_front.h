// cloud_front.h -- the front that the point-cloud coregistrations (ICP in icp.hip, CPD in cpd.hip) share: the two clouds of a dh plan's
// selected pixels gathered into float64 structure-of-arrays form, and _standardize_epc (xdem/coreg/affine.py:296-328) on them with
// exact medians -- nine selections (select_run.h).  No contraction (-ffp-contract=off).
#pragma once
#include <math.h>

#include <string>
#include <vector>

#include "common.h"
#include "select.h"
#include "select_run.h"
#include "dh_plan.h"

namespace xd {

template <typename T>
__global__ __launch_bounds__(256) void icp_gather_kernel(const T* __restrict__ ref, const T* __restrict__ tba, const T* __restrict__ pnx,
                                                         const T* __restrict__ pny, const T* __restrict__ pnz, const int64_t* __restrict__ idx, int64_t n,
                                                         int64_t W, double ta, double tc, double te, double tf, double* __restrict__ x,
                                                         double* __restrict__ y, double* __restrict__ zr, double* __restrict__ zt, double* __restrict__ nx,
                                                         double* __restrict__ ny, double* __restrict__ nz) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t q = idx[i], r = q / W, c = q - r * W;
        x[i] = tc + ((double)c + 0.5) * ta;
        y[i] = tf + ((double)r + 0.5) * te;
        zr[i] = (double)ref[q];
        zt[i] = (double)tba[q];
        if (pnx) { nx[i] = (double)pnx[q]; ny[i] = (double)pny[q]; nz[i] = (double)pnz[q]; }
    }
}
static __global__ __launch_bounds__(256) void icp_sub_kernel(double* __restrict__ v, int64_t n, double c) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) v[i] = v[i] - c;
}
static __global__ __launch_bounds__(256) void icp_div_kernel(double* __restrict__ v, int64_t n, double f) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) v[i] = v[i] / f;
}
static __global__ __launch_bounds__(256) void icp_absdev_kernel(const double* __restrict__ v, int64_t n, double c, double* __restrict__ out) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) out[i] = fabs(v[i] - c);
}

// exact np.median of d[0..n) (one local selection; a reduction hook on the context is suspended)
inline int icp_median(xdemhip_ctx* ctx, const double* d, int64_t n, unsigned char* scratch, SelWorkspace* ws, double* out) {
    std::vector<SelResult<uint64_t>> r;
    XdLocalSelection local(ctx);
    const int rc = run_select<double>(ctx, d, nullptr, n, 1, scratch, r, ws);
    if (rc) return rc;
    *out = median_from<double>(r[0]);
    return XDEMHIP_OK;
}

// the clouds of a plan, on the device: x, y (shared by both), the reference and the to-be-aligned heights, the normals (or null)
struct CloudFront {
    double *x = nullptr, *y = nullptr, *zr = nullptr, *zt = nullptr;
    double *nx = nullptr, *ny = nullptr, *nz = nullptr;
};

// Gather the n = P->n_idx selected pixels (dh_ensure_valid_idx was called, n > 0) and standardise them.  `mem` is the owner of the
// caller's object: the clouds live as long as it does (it frees them, also after a failure here).  `who`: "ICP" or "CPD", for messages.
inline int cloud_front_build(xdemhip_dh_plan* P, const double* transform6, bool with_normals, bool standardize, const char* who, XdOwned& mem, CloudFront& C,
                             double* centroid3, double* std_fac) {
    xdemhip_ctx* ctx = P->ctx;
    const int64_t n = P->n_idx;
    const std::string w(who);
    double* base = mem.take<double>((size_t)n * (with_normals ? 7 : 4), (w + " clouds").c_str());
    unsigned char* scratch = mem.take<unsigned char>(scratch_size(1), (w + " selection").c_str());
    double* tmp = mem.take<double>((size_t)n, (w + " selection").c_str());
    if (mem.rc) return mem.rc;
    C.x = base; C.y = base + n; C.zr = base + 2 * n; C.zt = base + 3 * n;
    if (with_normals) { C.nx = base + 4 * n; C.ny = base + 5 * n; C.nz = base + 6 * n; }
    const dim3 grid(grid_for(ctx, n, 256, 16));
    if (P->dtype == XDEMHIP_F32)
        hipLaunchKernelGGL((icp_gather_kernel<float>), grid, dim3(256), 0, ctx->stream, static_cast<const float*>(P->ref), static_cast<const float*>(P->tba),
                           with_normals ? static_cast<const float*>(P->icp_n[0]) : nullptr, static_cast<const float*>(P->icp_n[1]),
                           static_cast<const float*>(P->icp_n[2]), P->idx, n, P->W, transform6[0], transform6[2], transform6[4], transform6[5], C.x, C.y,
                           C.zr, C.zt, C.nx, C.ny, C.nz);
    else
        hipLaunchKernelGGL((icp_gather_kernel<double>), grid, dim3(256), 0, ctx->stream, static_cast<const double*>(P->ref), static_cast<const double*>(P->tba),
                           with_normals ? static_cast<const double*>(P->icp_n[0]) : nullptr, static_cast<const double*>(P->icp_n[1]),
                           static_cast<const double*>(P->icp_n[2]), P->idx, n, P->W, transform6[0], transform6[2], transform6[4], transform6[5], C.x, C.y,
                           C.zr, C.zt, C.nx, C.ny, C.nz);
    { const int rc_ = launched(ctx, "icp_gather_kernel"); if (rc_) return rc_; }
    // standardisation: three medians for the centroid, three more (of the centred values, as np.median sees them) and three of the
    // absolute deviations for the NMADs
    double* axis[3] = {C.x, C.y, C.zr};
    double nmads[3] = {0.0, 0.0, 0.0};
    int rc = XDEMHIP_OK;
    {   // (the workspace goes when the medians are done)
        SelWorkspaceLocal lws(ctx);
        SelWorkspace& ws = lws.ws;
        if (n >= SEL_BRACKET_MIN_N) (void)sel_ws_create(lws.mem, n, 8, 1, ws);
        for (int a = 0; a < 3 && rc == XDEMHIP_OK; ++a) {
            double med = 0.0, med2 = 0.0, mad = 0.0;
            rc = icp_median(ctx, axis[a], n, scratch, &ws, &med);
            if (rc) break;
            centroid3[a] = med;
            hipLaunchKernelGGL(icp_sub_kernel, grid, dim3(256), 0, ctx->stream, axis[a], n, med);
            if (a == 2) hipLaunchKernelGGL(icp_sub_kernel, grid, dim3(256), 0, ctx->stream, C.zt, n, med);
            if (!standardize) continue;
            rc = icp_median(ctx, axis[a], n, scratch, &ws, &med2);
            if (rc) break;
            hipLaunchKernelGGL(icp_absdev_kernel, grid, dim3(256), 0, ctx->stream, axis[a], n, med2, tmp);
            rc = icp_median(ctx, tmp, n, scratch, &ws, &mad);
            nmads[a] = 1.4826 * mad;
        }
    }
    if (rc) return rc;
    double f = 1.0;
    if (standardize) {
        f = ((nmads[0] + nmads[1]) + nmads[2]) / 3.0;
        if (!(f > 0.0) || !isfinite(f)) return xd_fail(ctx, XDEMHIP_EINVAL, w + ": the standardisation factor (mean NMAD of the reference cloud) is not positive");
        double* all[4] = {C.x, C.y, C.zr, C.zt};
        for (int a = 0; a < 4; ++a) hipLaunchKernelGGL(icp_div_kernel, grid, dim3(256), 0, ctx->stream, all[a], n, f);
    }
    *std_fac = f;
    return launched(ctx, (w + " standardisation").c_str());
}

}  // namespace xd
