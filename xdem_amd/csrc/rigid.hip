// rigid.hip -- LZD coregistration and the rotation-capable raster apply on gfx950: the passes that touch the grids.
//
// Replaces, for raster-raster input (xdem/coreg):
//   np.gradient(ref) scaled by the resolution                            affine.py:1440, 1455-1456 -> lzd_gradient_kernel (once per plan)
//   nanmean of the sampled coordinates and elevations                    affine.py:1744-1746       -> lzd_centroid_kernel
//   one LZD iteration: move the sampled pixels by the matrix, interpolate ref and its gradients there, least squares of the
//   linearised rigid model (Rosenholm & Torlegard 1988)                  affine.py:1461-1677       -> lzd_normal_kernel: the 6 x 6
//                                                                                                   normal equations (solved on the host)
//   _iterate_affine_regrid_small_rotations(resampling="linear")          base.py:1389-1519         -> apply_matrix_kernel
// The model is linear in its six parameters, so what upstream's least_squares converges to is the solution of the normal equations
// (the precedent: Deramp's moments).  Everything is float64 without contraction (-ffp-contract=off) and summed in a fixed order: two
// calls return the same bits, and the per-pixel values are bit for bit those of tests/rigid_oracle.py.  The order of the sums and the
// host sequence around them are those of fixed_sums.h; the gradient stencil, the matrix product and the transform check are shared with
// icp.hip (rigid_geom.h).
#include <math.h>
#include <string.h>

#include <vector>

#include "common.h"
#include "select.h"
#include "select_run.h"
#include "rank_select.h"
#include "nk_geom.h"
#include "bi_point.h"
#include "rigid_geom.h"
#include "dh_plan.h"

namespace xd {
namespace {

constexpr int LZD_NS = 29;   // 21 upper-triangle terms of a a^T, 6 of a dh, dh^2, sum dh

// 6-tuple geotransform (a, b, c, d, e, f), b = d = 0: x = c + (col + 0.5) a, y = f + (row + 0.5) e (pixel centres)
struct Rigid {
    double ta, tc, te, tf;
    double m[12];        // rows 0..2 of the 4 x 4 matrix
    double inv[12];      // rows 0..2 of its inverse (apply only)
    double cx, cy, cz;
    int has_centroid;
};

// p' = M (p - centroid) + centroid (mat12_apply, rigid_geom.h)
__device__ __forceinline__ void rigid_apply(const double* m, const Rigid& R, double x, double y, double z, double& ox, double& oy, double& oz) {
    if (R.has_centroid) { x = x - R.cx; y = y - R.cy; z = z - R.cz; }
    mat12_apply(m, x, y, z, ox, oy, oz);
    if (R.has_centroid) { ox = ox + R.cx; oy = oy + R.cy; oz = oz + R.cz; }
}

// ---- gradient planes -----------------------------------------------------------------------------------------------------------
// np.gradient(ref) in the raster dtype (np_gradient_at, rigid_geom.h), gradx = gx / res_x, grady = -gy / res_y with
// the resolution taken to the raster dtype first (NumPy 2: a Python float next to a float32 array is a float32).  H, W >= 2.
template <typename T>
__global__ __launch_bounds__(256) void lzd_gradient_kernel(const T* __restrict__ ref, int64_t H, int64_t W, T res_x, T res_y, T* __restrict__ gradx,
                                                           T* __restrict__ grady) {
    const int64_t n = H * W;
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = p / W, c = p - r * W;
        T gx, gy;
        np_gradient_at<T>(ref, H, W, r, c, gx, gy);
        gradx[p] = t_div(gx, res_x);
        grady[p] = t_div(-gy, res_y);
    }
}

// ---- one selected pixel of an LZD iteration ------------------------------------------------------------------------------------
struct LzdPixel { double x, y, z, dh, gx, gy; };   // x, y, z with the centroid removed
template <typename T>
__device__ __forceinline__ bool lzd_pixel(const T* __restrict__ ref, const T* __restrict__ gradx, const T* __restrict__ grady, const NkGeom& g,
                                          const Rigid& R, int64_t row, int64_t col, T tbav, LzdPixel& o) {
    const double x = R.tc + ((double)col + 0.5) * R.ta, y = R.tf + ((double)row + 0.5) * R.te;
    double xt, yt, zt;
    rigid_apply(R.m, R, x, y, (double)tbav, xt, yt, zt);
    const double rowp = (yt - R.tf) / R.te - 0.5, colp = (xt - R.tc) / R.ta - 0.5;
    T vr, vx, vy;
    bi_point<T>(g, ref, rowp, colp, vr);
    bi_point<T>(g, gradx, rowp, colp, vx);
    bi_point<T>(g, grady, rowp, colp, vy);
    o.dh = (double)vr - zt;
    o.gx = (double)vx;
    o.gy = (double)vy;
    o.x = xt - R.cx;
    o.y = yt - R.cy;
    o.z = zt - R.cz;
    return d_finite(o.dh) && d_finite(o.z) && d_finite(o.gx) && d_finite(o.gy);
}

__device__ __forceinline__ void lzd_accumulate(const LzdPixel& p, double* s) {
    const double a[6] = {-p.gx, -p.gy, 1.0, p.y + p.gy * p.z, -p.x - p.gx * p.z, p.gx * p.y - p.gy * p.x};
    int k = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = i; j < 6; ++j) s[k++] += a[i] * a[j];
#pragma unroll
    for (int i = 0; i < 6; ++i) s[21 + i] += a[i] * p.dh;
    s[27] += p.dh * p.dh;
    s[28] += p.dh;
}

// The hot kernel.  Dense route (idx == nullptr): workgroup b takes the tiles b, b + gridDim.x, ... of the valid mask (RANK_TILE pixels
// each, a lane strides through a tile so that a wave reads consecutive pixels).  List route: the drawn pixels, grid-strided.  Per-lane
// float64 accumulators, one partial per workgroup (block_sums_store, fixed_sums.h): part[b * (LZD_NS + 1) + k], slot LZD_NS = the count
// (exact in float64).
template <typename T>
__global__ __launch_bounds__(256) void lzd_normal_kernel(const T* __restrict__ ref, const T* __restrict__ tba, const T* __restrict__ gradx,
                                                         const T* __restrict__ grady, const uint8_t* __restrict__ valid,
                                                         const int64_t* __restrict__ idx, int64_t n, NkGeom g, Rigid R, double* __restrict__ part) {
    __shared__ double red[4];
    double s[LZD_NS];
#pragma unroll
    for (int k = 0; k < LZD_NS; ++k) s[k] = 0.0;
    double cnt = 0.0;
    LzdPixel px;
    if (idx) {
        for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
            const int64_t q = idx[i], r = q / g.W, c = q - r * g.W;
            if (lzd_pixel<T>(ref, gradx, grady, g, R, r, c, tba[q], px)) { lzd_accumulate(px, s); cnt += 1.0; }
        }
    } else {
        const int64_t n_tiles = (n + RANK_TILE - 1) / RANK_TILE;
        for (int64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
            const int64_t q0 = t * RANK_TILE;
            for (int k = threadIdx.x; k < RANK_TILE; k += 256) {
                const int64_t q = q0 + k;
                if (q < n && valid[q]) {
                    const int64_t r = q / g.W, c = q - r * g.W;
                    if (lzd_pixel<T>(ref, gradx, grady, g, R, r, c, tba[q], px)) { lzd_accumulate(px, s); cnt += 1.0; }
                }
            }
        }
    }
    block_sums_store<LZD_NS>(s, cnt, red, part);
}

// centroid sums over the listed pixels: integer sums of row and column, the float64 sum of tba in a fixed order.  ipart[b * 2 + 0 / 1],
// dpart[b].
template <typename T>
__global__ __launch_bounds__(256) void lzd_centroid_kernel(const T* __restrict__ tba, const int64_t* __restrict__ idx, int64_t n, int64_t W,
                                                           unsigned long long* __restrict__ ipart, double* __restrict__ dpart) {
    __shared__ double red[4];
    __shared__ unsigned long long ired[4];
    unsigned long long sr = 0, sc = 0;
    double sz = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t q = idx[i], r = q / W;
        sr += (unsigned long long)r;
        sc += (unsigned long long)(q - r * W);
        sz += (double)tba[q];
    }
    const unsigned long long tr = block_sum<unsigned long long>(sr, ired), tcn = block_sum<unsigned long long>(sc, ired);
    const double tz = block_sum<double>(sz, red);
    if (threadIdx.x == 0) { ipart[2 * blockIdx.x] = tr; ipart[2 * blockIdx.x + 1] = tcn; dpart[blockIdx.x] = tz; }
}
__global__ void lzd_centroid_reduce_kernel(const unsigned long long* __restrict__ ipart, const double* __restrict__ dpart, int nblocks,
                                           unsigned long long* __restrict__ iout, double* __restrict__ dout) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    unsigned long long sr = 0, sc = 0;
    double sz = 0.0;
    for (int b = 0; b < nblocks; ++b) { sr += ipart[2 * b]; sc += ipart[2 * b + 1]; sz += dpart[b]; }
    iout[0] = sr; iout[1] = sc; dout[0] = sz;
}

// the six arrays of every listed pixel, in list order, and whether the pixel is kept (the host drops the others)
template <typename T>
__global__ __launch_bounds__(256) void lzd_values_kernel(const T* __restrict__ ref, const T* __restrict__ tba, const T* __restrict__ gradx,
                                                         const T* __restrict__ grady, const int64_t* __restrict__ idx, int64_t n, NkGeom g, Rigid R,
                                                         double* __restrict__ out, uint8_t* __restrict__ keep) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t q = idx[i], r = q / g.W, c = q - r * g.W;
        LzdPixel p;
        keep[i] = lzd_pixel<T>(ref, gradx, grady, g, R, r, c, tba[q], p) ? 1 : 0;
        out[i] = p.x; out[n + i] = p.y; out[2 * n + i] = p.z; out[3 * n + i] = p.dh; out[4 * n + i] = p.gx; out[5 * n + i] = p.gy;
    }
}

// ---- the rotation-capable apply ------------------------------------------------------------------------------------------------
// One thread per output pixel: upstream's fixed-point iteration, which checks convergence after iterations 1 and 5 only and stores
// nothing after 5 -- a pixel keeps z0 of iteration 1 if it has converged (or is nodata) there, else z0 of iteration 5.
template <typename T>
__global__ __launch_bounds__(256) void apply_matrix_kernel(const T* __restrict__ dem, int64_t H, int64_t W, Rigid R, double tol_x, double tol_y,
                                                           T* __restrict__ out) {
    const int64_t n = H * W;
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = p / W, c = p - r * W;
        const double x = R.tc + ((double)c + 0.5) * R.ta, y = R.tf + ((double)r + 0.5) * R.te;
        double ux, uy, guess;
        rigid_apply(R.m, R, x, y, (double)dem[p], ux, uy, guess);
        double z0 = guess;
        for (int it = 1; it <= 5; ++it) {
            double tx, ty, tz, x0, y0;
            rigid_apply(R.inv, R, x, y, guess, tx, ty, tz);
            const double v = rgi_linear<T>(dem, H, W, (ty - R.tf) / R.te - 0.5, (tx - R.tc) / R.ta - 0.5);
            rigid_apply(R.m, R, tx, ty, v, x0, y0, z0);
            if (it == 1) {
                const double dx = x0 - x, dy = y0 - y;
                if ((fabs(dx) < tol_x || !d_finite(dx)) && (fabs(dy) < tol_y || !d_finite(dy))) break;
            }
            guess = z0;
        }
        out[p] = (T)z0;
    }
}

// (the inverse of the rigid matrix: R^T and -(R^T t), the products as explicit sums)
Rigid make_rigid(const double* t, const double* m16, const double* centroid) {
    Rigid R;
    memset(&R, 0, sizeof R);
    R.ta = t[0]; R.tc = t[2]; R.te = t[4]; R.tf = t[5];
    memcpy(R.m, m16, sizeof R.m);
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) R.inv[4 * i + j] = m16[4 * j + i];
        R.inv[4 * i + 3] = -((m16[i] * m16[3] + m16[4 + i] * m16[7]) + m16[8 + i] * m16[11]);
    }
    R.has_centroid = centroid != nullptr;
    if (centroid) { R.cx = centroid[0]; R.cy = centroid[1]; R.cz = centroid[2]; }
    return R;
}

NkGeom lzd_geom(const xdemhip_dh_plan* P) {
    NkGeom g;
    g.H = P->H; g.W = P->W; g.roff = 0; g.dr = 0.0; g.dc = 0.0; g.rule = P->ctx->nk_nan_rule;
    return g;
}

// the gradient planes of the plan for this resolution (made once; made again should the resolution change)
template <typename T>
int ensure_gradients_t(xdemhip_dh_plan* P, double res_x, double res_y) {
    xdemhip_ctx* ctx = P->ctx;
    if (P->gradx && P->grad_res_x == res_x && P->grad_res_y == res_y) return XDEMHIP_OK;
    const int64_t n = P->H * P->W;
    if (!P->gradx) {
        P->mem.optional();   // (both planes or neither: a plan without them can be asked again)
        P->gradx = P->mem.take((size_t)n * sizeof(T), "LZD gradient planes");
        P->grady = P->mem.take((size_t)n * sizeof(T), "LZD gradient planes");
        if (!P->mem.all_or_none(P->gradx, P->grady)) return xd_fail(ctx, XDEMHIP_ENOMEM, "hipMalloc failed (LZD gradient planes)");
    }
    hipLaunchKernelGGL((lzd_gradient_kernel<T>), dim3(grid_for(ctx, n, 256, 16)), dim3(256), 0, ctx->stream, static_cast<const T*>(P->ref), P->H, P->W,
                       (T)res_x, (T)res_y, static_cast<T*>(P->gradx), static_cast<T*>(P->grady));
    if (launched(ctx, "lzd_gradient_kernel")) return XDEMHIP_EHIP;
    P->grad_res_x = res_x; P->grad_res_y = res_y;
    return XDEMHIP_OK;
}
int ensure_gradients(xdemhip_dh_plan* P, const double* t) {
    if (P->H < 2 || P->W < 2) return xd_fail(P->ctx, XDEMHIP_EINVAL, "LZD needs a raster of at least 2 x 2 pixels (np.gradient)");
    return P->dtype == XDEMHIP_F32 ? ensure_gradients_t<float>(P, fabs(t[0]), fabs(t[4])) : ensure_gradients_t<double>(P, fabs(t[0]), fabs(t[4]));
}

template <typename T>
void launch_normal(xdemhip_dh_plan* P, const NkGeom& g, const Rigid& R, int nblocks, double* d_part) {
    const bool list = P->drawn;
    hipLaunchKernelGGL((lzd_normal_kernel<T>), dim3((unsigned)nblocks), dim3(256), 0, P->ctx->stream, static_cast<const T*>(P->ref),
                       static_cast<const T*>(P->tba), static_cast<const T*>(P->gradx), static_cast<const T*>(P->grady), P->valid,
                       list ? P->idx : (const int64_t*)nullptr, list ? P->n_idx : P->H * P->W, g, R, d_part);
}
template <typename T>
void launch_values(xdemhip_dh_plan* P, const NkGeom& g, const Rigid& R, double* d_out, uint8_t* d_keep) {
    hipLaunchKernelGGL((lzd_values_kernel<T>), dim3(grid_for(P->ctx, P->n_idx, 256, 16)), dim3(256), 0, P->ctx->stream, static_cast<const T*>(P->ref),
                       static_cast<const T*>(P->tba), static_cast<const T*>(P->gradx), static_cast<const T*>(P->grady), P->idx, P->n_idx, g, R, d_out, d_keep);
}
template <typename T>
void launch_centroid(xdemhip_dh_plan* P, int nblocks, unsigned long long* d_ip, double* d_dp) {
    hipLaunchKernelGGL((lzd_centroid_kernel<T>), dim3((unsigned)nblocks), dim3(256), 0, P->ctx->stream, static_cast<const T*>(P->tba), P->idx, P->n_idx, P->W,
                       d_ip, d_dp);
}

}  // namespace
}  // namespace xd

using namespace xd;

extern "C" {

int xdemhip_dh_lzd_gradients(xdemhip_dh_plan* P, const double* transform6, void* gradx_out, void* grady_out, int memspace) {
    XdFetchScope fetch_scope_(P ? P->ctx : nullptr);
    if (!P) return XDEMHIP_EINVAL;
    xdemhip_ctx* ctx = P->ctx;
    if (!gradx_out || !grady_out) return xd_fail(ctx, XDEMHIP_EINVAL, "null argument");
    if (memspace != XDEMHIP_HOST && memspace != XDEMHIP_DEVICE) return xd_fail(ctx, XDEMHIP_EINVAL, "bad memspace");
    { const int rc_ = check_transform(ctx, transform6, "xdemhip_dh_lzd_gradients"); if (rc_) return rc_; }
    XD_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    { const int rc_ = ensure_gradients(P, transform6); if (rc_) return rc_; }
    const size_t bytes = (size_t)(P->H * P->W) * (P->dtype == XDEMHIP_F32 ? 4 : 8);
    const hipMemcpyKind kind = memspace == XDEMHIP_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    XD_HIP_CHECK(ctx, hipMemcpyAsync(gradx_out, P->gradx, bytes, kind, ctx->stream));
    XD_HIP_CHECK(ctx, hipMemcpyAsync(grady_out, P->grady, bytes, kind, ctx->stream));
    return xd_sync(ctx);
}

int xdemhip_dh_lzd_centroid(xdemhip_dh_plan* P, const double* transform6, double* centroid_out, int64_t* count) {
    XdFetchScope fetch_scope_(P ? P->ctx : nullptr);
    if (!P) return XDEMHIP_EINVAL;
    xdemhip_ctx* ctx = P->ctx;
    if (!centroid_out) return xd_fail(ctx, XDEMHIP_EINVAL, "null argument");
    { const int rc_ = check_transform(ctx, transform6, "xdemhip_dh_lzd_centroid"); if (rc_) return rc_; }
    XD_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    { const int rc_ = dh_ensure_valid_idx(P); if (rc_) return rc_; }
    const int64_t k = P->n_idx;
    if (count) *count = k;
    if (k == 0) return xd_fail(ctx, XDEMHIP_EINVAL, "no valid points");
    const int nblocks = grid_for(ctx, k, 256, 4);
    unsigned long long hi[2] = {0, 0};   // (the fetches' destinations: declared first, they outlive the buffer's synchronisation)
    double hz = 0.0;
    XdBuffers buf(ctx, "xdemhip_dh_lzd_centroid");
    // layout: integer partials (2 per workgroup) and totals (2), then the float64 partials and total
    unsigned long long* d_ip = buf.alloc<unsigned long long>((size_t)(nblocks + 1) * 3);
    if (buf.rc) return buf.rc;
    unsigned long long* d_iout = d_ip + 2 * (size_t)nblocks;
    double* d_dp = reinterpret_cast<double*>(d_iout + 2);
    double* d_dout = d_dp + nblocks;
    if (P->dtype == XDEMHIP_F32) launch_centroid<float>(P, nblocks, d_ip, d_dp);
    else launch_centroid<double>(P, nblocks, d_ip, d_dp);
    hipLaunchKernelGGL(lzd_centroid_reduce_kernel, dim3(1), dim3(64), 0, ctx->stream, d_ip, d_dp, nblocks, d_iout, d_dout);
    int rc = launched(ctx, "lzd_centroid_kernel");
    if (rc == XDEMHIP_OK) rc = xd_d2h(ctx, hi, d_iout, 16);
    if (rc == XDEMHIP_OK) rc = xd_d2h(ctx, &hz, d_dout, 8);
    if (rc == XDEMHIP_OK) rc = xd_sync(ctx);
    if (rc) return rc;
    const double nk = (double)k;
    centroid_out[0] = transform6[2] + ((double)hi[1] / nk + 0.5) * transform6[0];
    centroid_out[1] = transform6[5] + ((double)hi[0] / nk + 0.5) * transform6[4];
    centroid_out[2] = hz / nk;
    return XDEMHIP_OK;
}

int xdemhip_dh_lzd_normal(xdemhip_dh_plan* P, const double* transform6, const double* matrix16, const double* centroid3, double* sums_out,
                          int64_t* count) {
    XdFetchScope fetch_scope_(P ? P->ctx : nullptr);
    if (!P) return XDEMHIP_EINVAL;
    xdemhip_ctx* ctx = P->ctx;
    if (!matrix16 || !centroid3 || !sums_out || !count) return xd_fail(ctx, XDEMHIP_EINVAL, "null argument");
    { const int rc_ = check_transform(ctx, transform6, "xdemhip_dh_lzd_normal"); if (rc_) return rc_; }
    *count = 0;
    if ((P->drawn ? P->n_idx : P->n_valid) == 0) return xd_fail(ctx, XDEMHIP_EINVAL, "no valid points");
    XD_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    if (!P->drawn) { const int rc_ = dh_ensure_mask(P); if (rc_) return rc_; }
    { const int rc_ = ensure_gradients(P, transform6); if (rc_) return rc_; }
    const int nb = fixed_sums_grid(ctx, P->drawn ? (P->n_idx + 255) / 256 : P->n_tiles);
    const int NT = LZD_NS + 1;
    { const int rc_ = P->sums.reserve(P->mem, NT, "xdemhip_dh_lzd_normal"); if (rc_) return rc_; }
    const NkGeom g = lzd_geom(P);
    const Rigid R = make_rigid(transform6, matrix16, centroid3);
    (void)hipEventRecord(ctx->ev_start, ctx->stream);
    if (P->dtype == XDEMHIP_F32) launch_normal<float>(P, g, R, nb, P->sums.part);
    else launch_normal<double>(P, g, R, nb, P->sums.part);
    double h[LZD_NS + 1];
    { const int rc_ = fixed_sums_finish(ctx, P->sums, nb, NT, "lzd_normal_kernel", h); if (rc_) return rc_; }
    memcpy(sums_out, h, LZD_NS * 8);
    *count = (int64_t)h[LZD_NS];
    return XDEMHIP_OK;
}

int xdemhip_dh_lzd_values(xdemhip_dh_plan* P, const double* transform6, const double* matrix16, const double* centroid3, double* out,
                          int64_t* count) {
    XdFetchScope fetch_scope_(P ? P->ctx : nullptr);
    if (!P) return XDEMHIP_EINVAL;
    xdemhip_ctx* ctx = P->ctx;
    if (!matrix16 || !centroid3 || !out || !count) return xd_fail(ctx, XDEMHIP_EINVAL, "null argument");
    { const int rc_ = check_transform(ctx, transform6, "xdemhip_dh_lzd_values"); if (rc_) return rc_; }
    *count = 0;
    XD_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    { const int rc_ = dh_ensure_valid_idx(P); if (rc_) return rc_; }
    const int64_t n = P->n_idx;
    if (n == 0) return xd_fail(ctx, XDEMHIP_EINVAL, "no valid points");
    { const int rc_ = ensure_gradients(P, transform6); if (rc_) return rc_; }
    std::vector<double> h;          // (the copies' destinations: declared first, so that they outlive the buffer's synchronisation)
    std::vector<uint8_t> keep;
    XdBuffers buf(ctx, "xdemhip_dh_lzd_values");
    double* d_out = static_cast<double*>(buf.alloc((size_t)n * 49));   // six float64 rows, then the keep bytes
    if (buf.rc) return buf.rc;
    uint8_t* d_keep = reinterpret_cast<uint8_t*>(d_out + 6 * n);
    const NkGeom g = lzd_geom(P);
    const Rigid R = make_rigid(transform6, matrix16, centroid3);
    if (P->dtype == XDEMHIP_F32) launch_values<float>(P, g, R, d_out, d_keep);
    else launch_values<double>(P, g, R, d_out, d_keep);
    int rc = launched(ctx, "lzd_values_kernel");
    if (rc == XDEMHIP_OK) {
        h.resize((size_t)6 * n);
        keep.resize((size_t)n);
        if (hipMemcpyAsync(h.data(), d_out, (size_t)n * 48, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
            hipMemcpyAsync(keep.data(), d_keep, (size_t)n, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess)
            rc = xd_fail(ctx, XDEMHIP_EHIP, "D2H copy failed");
    }
    if (rc == XDEMHIP_OK) rc = xd_sync(ctx);
    if (rc) return rc;
    // the pixels left, in raster order: row a of the result starts at out[a * n] (n = the selection's size), *count entries are filled
    int64_t m = 0;
    for (int64_t i = 0; i < n; ++i)
        if (keep[i]) {
            for (int a = 0; a < 6; ++a) out[(size_t)a * n + m] = h[(size_t)a * n + i];
            ++m;
        }
    *count = m;
    return XDEMHIP_OK;
}

int xdemhip_apply_matrix_rst(xdemhip_ctx* ctx, const void* dem, int dtype, int64_t H, int64_t W, const double* transform6, const double* matrix16,
                             const double* centroid3_or_null, void* out, int memspace) {
    XdFetchScope fetch_scope_(ctx);
    if (!ctx) return XDEMHIP_EINVAL;
    if (!dem || !out || !matrix16) return xd_fail(ctx, XDEMHIP_EINVAL, "null argument");
    if (H < 2 || W < 2) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_apply_matrix_rst: the raster must be at least 2 x 2 pixels");
    if (dtype != XDEMHIP_F32 && dtype != XDEMHIP_F64) return xd_fail(ctx, XDEMHIP_EINVAL, "dtype must be float32 or float64");
    if (memspace != XDEMHIP_HOST && memspace != XDEMHIP_DEVICE) return xd_fail(ctx, XDEMHIP_EINVAL, "bad memspace");
    { const int rc_ = check_transform(ctx, transform6, "xdemhip_apply_matrix_rst"); if (rc_) return rc_; }
    XD_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    const int64_t n = H * W;
    const size_t bytes = (size_t)n * (dtype == XDEMHIP_F32 ? 4 : 8);
    XdBuffers buf(ctx, "xdemhip_apply_matrix_rst");
    const void* d_in = buf.input(dem, bytes, memspace);
    void* d_out = buf.output(out, bytes, memspace);
    if (buf.rc) return buf.rc;
    const Rigid R = make_rigid(transform6, matrix16, centroid3_or_null);
    const double tol_x = 1e-4 * fabs(transform6[0]), tol_y = 1e-4 * fabs(transform6[4]);
    const dim3 grid(grid_for(ctx, n, 256, 16));
    (void)hipEventRecord(ctx->ev_start, ctx->stream);
    if (dtype == XDEMHIP_F32)
        hipLaunchKernelGGL((apply_matrix_kernel<float>), grid, dim3(256), 0, ctx->stream, static_cast<const float*>(d_in), H, W, R, tol_x, tol_y,
                           static_cast<float*>(d_out));
    else
        hipLaunchKernelGGL((apply_matrix_kernel<double>), grid, dim3(256), 0, ctx->stream, static_cast<const double*>(d_in), H, W, R, tol_x, tol_y,
                           static_cast<double*>(d_out));
    int rc = launched(ctx, "apply_matrix_kernel");
    (void)hipEventRecord(ctx->ev_stop, ctx->stream);
    ctx->timed = (rc == XDEMHIP_OK);
    return rc == XDEMHIP_OK ? buf.finish() : rc;
}

}  // extern "C"
