// cpd.hip -- Coherent Point Drift coregistration on gfx950: the E-step over every (reference, to-be-aligned) pair of two clouds and the
// sums of the M-step.
//
// Replaces, for raster-raster input (xdem/coreg/affine.py):
//   _standardize_epc (np.median, nmad)                                   affine.py:296-328   -> exact selections (cloud_front.h, shared with icp.hip)
//   _cpd_fit: diff2 (M, N, 3), P (M, N), Pden, Pt1, P1, Np, PX           affine.py:1215-1236 -> two streaming pair passes with O(N + M) state
//   _cpd_fit: muX, muY, X_hat, Y_hat, YPY, A, xPx                        affine.py:1241-1283 -> two stages of fixed-order sums (fixed_sums.h)
// The 3 x 3 SVD and the update of (matrix, sigma2, q) stay on the host (xdem_amd/cpd.py).
//
// Everything is float64 without contraction (-ffp-contract=off).  Nothing of size N M exists.  The passes share one tiling: a workgroup
// of 256 lanes owns 256 points of one cloud (one per lane, coordinates in registers) and walks one SLICE of the other cloud, staged
// through LDS in chunks of 256 points of four doubles; every lane reads the same LDS address (a broadcast), 128 bits at a time.
//   pass A   lane = reference point n, slice of the moved cloud ty:  den_part[slice][n] = sum_m p_mn          (first call: sum_m |x_n - ty_m|^2)
//   finish A den_n = the slices added in ascending order, inv_n = 1 / (max(den_n, 2^-52) + c), Pt1_n = den_n inv_n
//   pass B   lane = moved point m, slice of (x_n, inv_n):            P1_m = sum_n p_mn inv_n, PX_m = sum_n p_mn inv_n x_n, per slice
//   finish B the slices added in ascending order
// p_mn = exp(-((dx dx + dy dy) + dz dz) / (2 sigma2)) with d = x_n - ty_m is ONE expression (cpd_affinity): the same bits in A and B.
//
// The order contract: a lane adds the points of its slice in ascending index; slices are added in ascending order; the slice length
// depends on N, M and the device's number of compute units only -- never on how the pass is cut into launches; the sums of the
// M-step follow fixed_sums.h.  No float atomics: two calls return the same bits.
#include <math.h>
#include <string.h>

#include <vector>

#include "common.h"
#include "select.h"
#include "select_run.h"
#include "rigid_geom.h"
#include "dh_plan.h"
#include "cloud_front.h"

struct xdemhip_cpd {
    xdemhip_ctx* ctx = nullptr;
    int64_t n = 0, m = 0;            // reference points, to-be-aligned points
    XdOwned mem;                     // every device allocation of the object
    double *rx = nullptr, *ry = nullptr, *rz = nullptr;   // reference cloud
    double *qx = nullptr, *qy = nullptr, *qz = nullptr;   // to-be-aligned cloud (qx, qy = rx, ry for a cloud made from a plan)
    double4* x4 = nullptr;           // n x (x, y, z, inv): what pass B stages
    double4* t4 = nullptr;           // m x (tx, ty, tz, 0): the moved cloud, what pass A stages
    double *den = nullptr, *pt1 = nullptr;   // n
    double *p1 = nullptr, *px = nullptr;     // m, 3 m (rows x, y, z)
    double* part = nullptr;          // slice partials: max(slices_a * n, 4 * slices_b * m)
    int64_t len_a = 0, len_b = 0;    // points per slice: of the moved cloud (pass A), of the reference cloud (pass B)
    int64_t slices_a = 0, slices_b = 0;
    double* dpar = nullptr;          // [0] sigma2, [1] 2 sigma2, [2] c; [8 .. 27) the results of an E-step
    bool stepped = false;
    xd::FixedSums sums;              // per-workgroup partials and totals of the M-step sums (fixed_sums.h)
};

namespace xd {
namespace {

constexpr int CPD_NT1 = 8;    // stage 1: Np, sum PX (3), sum P1 y (3), the count
constexpr int CPD_NT2 = 12;   // stage 2: A (9, row by row), xPx, YPY, the count
constexpr int CPD_NOUT = 19;  // Np, muX (3), muY (3), A (9), xPx, YPY, sigma2
constexpr int64_t CPD_MIN_SLICE = 16;
constexpr int64_t CPD_PAIRS_PER_LAUNCH = (int64_t)1 << 32;

__device__ __forceinline__ double cpd_d2(double xx, double xy, double xz, double tx, double ty, double tz) {
    const double dx = xx - tx, dy = xy - ty, dz = xz - tz;
    return (dx * dx + dy * dy) + dz * dz;
}
// p_mn: the one expression of both passes
__device__ __forceinline__ double cpd_affinity(double xx, double xy, double xz, double tx, double ty, double tz, double two_s2) {
    return exp(-cpd_d2(xx, xy, xz, tx, ty, tz) / two_s2);
}

__global__ __launch_bounds__(256) void cpd_pack_kernel(const double* __restrict__ x, const double* __restrict__ y, const double* __restrict__ z, int64_t n,
                                                       double4* __restrict__ out) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) out[i] = make_double4(x[i], y[i], z[i], 0.0);
}
__global__ __launch_bounds__(256) void cpd_move_kernel(const double* __restrict__ qx, const double* __restrict__ qy, const double* __restrict__ qz, int64_t m,
                                                       Mat12 M, double4* __restrict__ t4) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (int64_t)gridDim.x * blockDim.x) {
        double px, py, pz;
        mat12_apply(M.m, qx[i], qy[i], qz[i], px, py, pz);
        t4[i] = make_double4(px, py, pz, 0.0);
    }
}

// ---- the pair passes ---------------------------------------------------------------------------------------------------------------
// Workgroup `unit` = block * slices + slice.  A lane beyond its cloud's end computes on zeros and writes nothing; every lane takes
// part in the staging and its barriers.
template <bool EXP>
__global__ __launch_bounds__(256) void cpd_pass_a_kernel(const double* __restrict__ rx, const double* __restrict__ ry, const double* __restrict__ rz, int64_t n,
                                                         const double4* __restrict__ t4, int64_t m, int64_t len, int64_t slices, int64_t unit0,
                                                         const double* __restrict__ dpar, double* __restrict__ part) {
    __shared__ double4 s[256];
    const int64_t unit = unit0 + blockIdx.x, block = unit / slices, slice = unit - block * slices;
    const int64_t i = block * 256 + threadIdx.x;
    const bool live = i < n;
    const double xx = live ? rx[i] : 0.0, xy = live ? ry[i] : 0.0, xz = live ? rz[i] : 0.0;
    const double two_s2 = EXP ? dpar[1] : 1.0;
    const int64_t j0 = slice * len, j1 = (j0 + len < m) ? j0 + len : m;
    double acc = 0.0;
    for (int64_t c0 = j0; c0 < j1; c0 += 256) {
        const int cnt = (int)((j1 - c0 < 256) ? j1 - c0 : 256);
        if ((int)threadIdx.x < cnt) s[threadIdx.x] = t4[c0 + threadIdx.x];
        __syncthreads();
#pragma unroll 4
        for (int j = 0; j < cnt; ++j) {
            const double4 t = s[j];
            acc += EXP ? cpd_affinity(xx, xy, xz, t.x, t.y, t.z, two_s2) : cpd_d2(xx, xy, xz, t.x, t.y, t.z);
        }
        __syncthreads();
    }
    if (live) part[slice * n + i] = acc;
}

// out[i] = the slices of part[.][i] in ascending order
__global__ __launch_bounds__(256) void cpd_slices_kernel(const double* __restrict__ part, int64_t n, int64_t slices, double* __restrict__ out) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        double a = 0.0;
        for (int64_t sl = 0; sl < slices; ++sl) a += part[sl * n + i];
        out[i] = a;
    }
}
// the first call's sum of squared distances over n: one partial per workgroup, part[b * 2 + 0], the count in slot 1
__global__ __launch_bounds__(256) void cpd_total_kernel(const double* __restrict__ v, int64_t n, double* __restrict__ part) {
    __shared__ double red[4];
    double s[1] = {0.0}, cnt = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) { s[0] += v[i]; cnt += 1.0; }
    block_sums_store<1>(s, cnt, red, part);
}
// sigma2 (given, or total / (3 N M)), 2 sigma2 and c = (2 pi sigma2)^(3/2) w / (1 - w) M / N, left to right as upstream writes it
__global__ void cpd_params_kernel(double sigma2, const double* __restrict__ total, double n, double m, double weight, double* __restrict__ dpar) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    if (total) sigma2 = total[0] / ((3.0 * n) * m);
    dpar[0] = sigma2;
    dpar[1] = 2.0 * sigma2;
    dpar[2] = pow((2.0 * 3.141592653589793) * sigma2, 1.5) * weight / (1.0 - weight) * m / n;
}
__global__ __launch_bounds__(256) void cpd_finish_a_kernel(const double* __restrict__ part, int64_t n, int64_t slices, const double* __restrict__ dpar,
                                                           double* __restrict__ den, double4* __restrict__ x4, double* __restrict__ pt1) {
    const double c = dpar[2];
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        double a = 0.0;
        for (int64_t sl = 0; sl < slices; ++sl) a += part[sl * n + i];
        const double inv = 1.0 / (fmax(a, 2.220446049250313e-16) + c);
        den[i] = a;
        x4[i].w = inv;
        pt1[i] = a * inv;
    }
}

__global__ __launch_bounds__(256) void cpd_pass_b_kernel(const double4* __restrict__ t4, int64_t m, const double4* __restrict__ x4, int64_t n, int64_t len,
                                                         int64_t slices, int64_t unit0, const double* __restrict__ dpar, double* __restrict__ part) {
    __shared__ double4 s[256];
    const int64_t unit = unit0 + blockIdx.x, block = unit / slices, slice = unit - block * slices;
    const int64_t i = block * 256 + threadIdx.x;
    const bool live = i < m;
    const double4 t = live ? t4[i] : make_double4(0.0, 0.0, 0.0, 0.0);
    const double two_s2 = dpar[1];
    const int64_t j0 = slice * len, j1 = (j0 + len < n) ? j0 + len : n;
    double a1 = 0.0, ax = 0.0, ay = 0.0, az = 0.0;
    for (int64_t c0 = j0; c0 < j1; c0 += 256) {
        const int cnt = (int)((j1 - c0 < 256) ? j1 - c0 : 256);
        if ((int)threadIdx.x < cnt) s[threadIdx.x] = x4[c0 + threadIdx.x];
        __syncthreads();
#pragma unroll 4
        for (int j = 0; j < cnt; ++j) {
            const double4 x = s[j];
            const double P = cpd_affinity(x.x, x.y, x.z, t.x, t.y, t.z, two_s2) * x.w;
            a1 += P;
            ax += P * x.x; ay += P * x.y; az += P * x.z;
        }
        __syncthreads();
    }
    if (live) {
        double* o = part + slice * 4 * m + i;
        o[0] = a1; o[m] = ax; o[2 * m] = ay; o[3 * m] = az;
    }
}
__global__ __launch_bounds__(256) void cpd_finish_b_kernel(const double* __restrict__ part, int64_t m, int64_t slices, double* __restrict__ p1,
                                                           double* __restrict__ px) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (int64_t)gridDim.x * blockDim.x) {
        double a[4] = {0.0, 0.0, 0.0, 0.0};
        for (int64_t sl = 0; sl < slices; ++sl)
#pragma unroll
            for (int k = 0; k < 4; ++k) a[k] += part[(sl * 4 + k) * m + i];
        p1[i] = a[0];
        px[i] = a[1]; px[m + i] = a[2]; px[2 * m + i] = a[3];
    }
}

// ---- the sums of the M-step (fixed_sums.h) -----------------------------------------------------------------------------------------
// stage 1 over the to-be-aligned points (the ORIGINAL ones, as upstream's muY): Np, sum PX, sum P1 y
__global__ __launch_bounds__(256) void cpd_stage1_kernel(const double* __restrict__ p1, const double* __restrict__ px, const double* __restrict__ qx,
                                                         const double* __restrict__ qy, const double* __restrict__ qz, int64_t m, double* __restrict__ part) {
    __shared__ double red[4];
    double s[CPD_NT1 - 1];
#pragma unroll
    for (int t = 0; t < CPD_NT1 - 1; ++t) s[t] = 0.0;
    double cnt = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (int64_t)gridDim.x * blockDim.x) {
        const double w = p1[i];
        s[0] += w;
        s[1] += px[i]; s[2] += px[m + i]; s[3] += px[2 * m + i];
        s[4] += w * qx[i]; s[5] += w * qy[i]; s[6] += w * qz[i];
        cnt += 1.0;
    }
    block_sums_store<CPD_NT1 - 1>(s, cnt, red, part);
}
// stage 2 with muX = sum PX / Np and muY = sum P1 y / Np from stage 1's totals: A = sum_m (PX_m - P1_m muX) yhat_m^T,
// YPY = sum_m P1_m |yhat_m|^2 (index < m) and xPx = sum_n Pt1_n |xhat_n|^2 (index < n)
__global__ __launch_bounds__(256) void cpd_stage2_kernel(const double* __restrict__ tot1, const double* __restrict__ p1, const double* __restrict__ px,
                                                         const double* __restrict__ qx, const double* __restrict__ qy, const double* __restrict__ qz, int64_t m,
                                                         const double* __restrict__ pt1, const double* __restrict__ rx, const double* __restrict__ ry,
                                                         const double* __restrict__ rz, int64_t n, double* __restrict__ part) {
    __shared__ double red[4];
    const double np_ = tot1[0];
    const double mux[3] = {tot1[1] / np_, tot1[2] / np_, tot1[3] / np_}, muy[3] = {tot1[4] / np_, tot1[5] / np_, tot1[6] / np_};
    double s[CPD_NT2 - 1];
#pragma unroll
    for (int t = 0; t < CPD_NT2 - 1; ++t) s[t] = 0.0;
    double cnt = 0.0;
    const int64_t top = m > n ? m : n;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < top; i += (int64_t)gridDim.x * blockDim.x) {
        if (i < m) {
            const double w = p1[i];
            const double yh[3] = {qx[i] - muy[0], qy[i] - muy[1], qz[i] - muy[2]};
            const double g[3] = {px[i] - w * mux[0], px[m + i] - w * mux[1], px[2 * m + i] - w * mux[2]};
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = 0; c < 3; ++c) s[3 * r + c] += g[r] * yh[c];
            s[10] += w * ((yh[0] * yh[0] + yh[1] * yh[1]) + yh[2] * yh[2]);
        }
        if (i < n) {
            const double xh[3] = {rx[i] - mux[0], ry[i] - mux[1], rz[i] - mux[2]};
            s[9] += pt1[i] * ((xh[0] * xh[0] + xh[1] * xh[1]) + xh[2] * xh[2]);
        }
        cnt += 1.0;
    }
    block_sums_store<CPD_NT2 - 1>(s, cnt, red, part);
}
// the results of an E-step in one block: Np, muX, muY, A, xPx, YPY, sigma2
__global__ void cpd_results_kernel(const double* __restrict__ tot1, const double* __restrict__ tot2, const double* __restrict__ dpar, double* __restrict__ out) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const double np_ = tot1[0];
    out[0] = np_;
    for (int k = 0; k < 3; ++k) { out[1 + k] = tot1[1 + k] / np_; out[4 + k] = tot1[4 + k] / np_; }
    for (int k = 0; k < 11; ++k) out[7 + k] = tot2[k];
    out[18] = dpar[0];
}

// ---- host side -------------------------------------------------------------------------------------------------------------------
// Points per slice of a cloud of `other` points walked by the blocks of a cloud of `own` points: enough slices that blocks x slices
// reaches num_cu * 8 workgroups and no more, at least CPD_MIN_SLICE points each.  A function of N, M and the device only.
void cpd_slicing(const xdemhip_ctx* ctx, int64_t own, int64_t other, int64_t* len, int64_t* slices) {
    const int64_t blocks = (own + 255) / 256, target = (int64_t)ctx->num_cu * 8;
    int64_t s = (target + blocks - 1) / blocks;
    const int64_t most = (other + CPD_MIN_SLICE - 1) / CPD_MIN_SLICE;
    if (s > most) s = most;
    if (s < 1) s = 1;
    *len = (other + s - 1) / s;
    *slices = (other + *len - 1) / *len;
}

// the buffers of the E-step, sized once the clouds are known, and the packed reference cloud
int cpd_alloc_work(xdemhip_cpd* C) {
    xdemhip_ctx* ctx = C->ctx;
    const int64_t n = C->n, m = C->m;
    cpd_slicing(ctx, n, m, &C->len_a, &C->slices_a);
    cpd_slicing(ctx, m, n, &C->len_b, &C->slices_b);
    const int64_t pa = C->slices_a * n, pb = 4 * C->slices_b * m;
    XdOwned& mem = C->mem;
    C->x4 = mem.take<double4>((size_t)n, "CPD clouds");
    C->t4 = mem.take<double4>((size_t)m, "CPD clouds");
    C->den = mem.take<double>((size_t)n, "CPD E-step");
    C->pt1 = mem.take<double>((size_t)n, "CPD E-step");
    C->p1 = mem.take<double>((size_t)m, "CPD E-step");
    C->px = mem.take<double>((size_t)m * 3, "CPD E-step");
    C->part = mem.take<double>((size_t)(pa > pb ? pa : pb), "CPD slice partials");
    C->dpar = mem.take<double>(32, "CPD E-step");
    if (mem.rc) return mem.rc;
    { const int rc = C->sums.reserve(mem, CPD_NT1 + CPD_NT2, "CPD partial sums"); if (rc) return rc; }
    hipLaunchKernelGGL(cpd_pack_kernel, dim3(grid_for(ctx, n, 256, 16)), dim3(256), 0, ctx->stream, C->rx, C->ry, C->rz, n, C->x4);
    return launched(ctx, "cpd_pack_kernel");
}

// A pair pass of `units` workgroups of `pairs_per_wg` pair evaluations each, in launches of at most 2^32 evaluations -- or of
// "pairs_launch_cap" workgroups where that option is set.  launch(first unit, workgroups).
template <typename L> int cpd_pair_launches(xdemhip_ctx* ctx, int64_t units, int64_t pairs_per_wg, const char* what, L launch) {
    int64_t per = ctx->pairs_launch_cap > 0 ? (int64_t)ctx->pairs_launch_cap : CPD_PAIRS_PER_LAUNCH / (pairs_per_wg > 0 ? pairs_per_wg : 1);
    const int64_t most = ((int64_t)1 << 31) / 256;   // a HIP dispatch carries the total work-item count of a dimension in 32 bits
    if (per > most) per = most;
    if (per < 1) per = 1;
    for (int64_t u0 = 0; u0 < units; u0 += per) launch(u0, (unsigned)((units - u0) < per ? (units - u0) : per));
    return launched(ctx, what);
}

}  // namespace
}  // namespace xd

using namespace xd;

extern "C" {

void xdemhip_cpd_destroy(xdemhip_cpd* C) { delete C; }

int xdemhip_cpd_create_plan(xdemhip_dh_plan* P, const double* transform6, int standardize, xdemhip_cpd** out, double* centroid3, double* std_fac,
                            int64_t* count) {
    XdFetchScope fetch_scope_(P ? P->ctx : nullptr);
    if (!P) return XDEMHIP_EINVAL;
    xdemhip_ctx* ctx = P->ctx;
    if (!out || !centroid3 || !std_fac) return xd_fail(ctx, XDEMHIP_EINVAL, "null argument");
    { const int rc_ = check_transform(ctx, transform6, "xdemhip_cpd_create_plan"); if (rc_) return rc_; }
    XD_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    { const int rc_ = dh_ensure_valid_idx(P); if (rc_) return rc_; }
    const int64_t n = P->n_idx;
    if (count) *count = n;
    if (n == 0) return xd_fail(ctx, XDEMHIP_EINVAL, "no valid points");
    xdemhip_cpd* C = new xdemhip_cpd();
    C->ctx = C->mem.ctx = ctx; C->n = n; C->m = n;
    auto fail = [&](int code) { delete C; return code; };
    CloudFront F;
    int rc = cloud_front_build(P, transform6, false, standardize != 0, "CPD", C->mem, F, centroid3, std_fac);
    if (rc) return fail(rc);
    C->rx = C->qx = F.x; C->ry = C->qy = F.y; C->rz = F.zr; C->qz = F.zt;
    rc = cpd_alloc_work(C);
    if (rc == XDEMHIP_OK) rc = xd_sync(ctx);
    if (rc) return fail(rc);
    *out = C;
    return XDEMHIP_OK;
}

int xdemhip_cpd_create_points(xdemhip_ctx* ctx, const double* ref3n, int64_t n, const double* tba3m, int64_t m, xdemhip_cpd** out) {
    XdFetchScope fetch_scope_(ctx);
    if (!ctx) return XDEMHIP_EINVAL;
    if (!ref3n || !tba3m || !out) return xd_fail(ctx, XDEMHIP_EINVAL, "null argument");
    if (n < 1 || m < 1) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_cpd_create_points: both clouds need at least one point");
    XD_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    xdemhip_cpd* C = new xdemhip_cpd();
    C->ctx = C->mem.ctx = ctx; C->n = n; C->m = m;
    auto fail = [&](int code) { delete C; return code; };
    double* r = C->mem.keep(ref3n, (size_t)n * 24, XDEMHIP_HOST, "CPD clouds");
    double* q = C->mem.keep(tba3m, (size_t)m * 24, XDEMHIP_HOST, "CPD clouds");
    int rc = C->mem.rc;
    if (rc) return fail(rc);
    C->rx = r; C->ry = r + n; C->rz = r + 2 * n;
    C->qx = q; C->qy = q + m; C->qz = q + 2 * m;
    rc = cpd_alloc_work(C);
    if (rc == XDEMHIP_OK) rc = xd_sync(ctx);
    if (rc) return fail(rc);
    *out = C;
    return XDEMHIP_OK;
}

int xdemhip_cpd_estep(xdemhip_cpd* C, const double* matrix16_or_null, double sigma2_or_nan, double weight, double* sums_out, double* sigma2_used) {
    XdFetchScope fetch_scope_(C ? C->ctx : nullptr);
    if (!C) return XDEMHIP_EINVAL;
    xdemhip_ctx* ctx = C->ctx;
    if (!sums_out || !sigma2_used) return xd_fail(ctx, XDEMHIP_EINVAL, "null argument");
    if (!(weight >= 0.0 && weight < 1.0)) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_cpd_estep: 0 <= weight < 1");
    XD_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    const int64_t n = C->n, m = C->m;
    const int64_t blocks_n = (n + 255) / 256, blocks_m = (m + 255) / 256;
    Mat12 M;
    const double eye[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    memcpy(M.m, matrix16_or_null ? matrix16_or_null : eye, sizeof M.m);
    const int G = ctx->num_cu * 8 + 1;   // rows of a FixedSums region
    double* part1 = C->sums.part;
    double* part2 = C->sums.part + (int64_t)G * CPD_NT1;
    const dim3 gn(grid_for(ctx, n, 256, 16)), gm(grid_for(ctx, m, 256, 16));
    (void)hipEventRecord(ctx->ev_start, ctx->stream);
    hipLaunchKernelGGL(cpd_move_kernel, gm, dim3(256), 0, ctx->stream, C->qx, C->qy, C->qz, m, M, C->t4);
    { const int rc_ = launched(ctx, "cpd_move_kernel"); if (rc_) return rc_; }
    if (sigma2_or_nan != sigma2_or_nan) {   // the first call: sigma2 = sum |x_n - ty_m|^2 / (3 N M), summed pair by pair
        int rc = cpd_pair_launches(ctx, blocks_n * C->slices_a, 256 * C->len_a, "cpd_pass_a_kernel", [&](int64_t u0, unsigned nw) {
            hipLaunchKernelGGL((cpd_pass_a_kernel<false>), dim3(nw), dim3(256), 0, ctx->stream, C->rx, C->ry, C->rz, n, C->t4, m, C->len_a, C->slices_a, u0,
                               C->dpar, C->part);
        });
        if (rc) return rc;
        const int nb = fixed_sums_grid(ctx, blocks_n);
        hipLaunchKernelGGL(cpd_slices_kernel, gn, dim3(256), 0, ctx->stream, C->part, n, C->slices_a, C->den);
        hipLaunchKernelGGL(cpd_total_kernel, dim3((unsigned)nb), dim3(256), 0, ctx->stream, C->den, n, part2);
        rc = fixed_sums_reduce(ctx, part2, nb, 2, "cpd_total_kernel");
        if (rc) return rc;
        hipLaunchKernelGGL(cpd_params_kernel, dim3(1), dim3(64), 0, ctx->stream, 0.0, part2 + (int64_t)nb * 2, (double)n, (double)m, weight, C->dpar);
    } else {
        hipLaunchKernelGGL(cpd_params_kernel, dim3(1), dim3(64), 0, ctx->stream, sigma2_or_nan, (const double*)nullptr, (double)n, (double)m, weight, C->dpar);
    }
    { const int rc_ = launched(ctx, "cpd_params_kernel"); if (rc_) return rc_; }
    int rc = cpd_pair_launches(ctx, blocks_n * C->slices_a, 256 * C->len_a, "cpd_pass_a_kernel", [&](int64_t u0, unsigned nw) {
        hipLaunchKernelGGL((cpd_pass_a_kernel<true>), dim3(nw), dim3(256), 0, ctx->stream, C->rx, C->ry, C->rz, n, C->t4, m, C->len_a, C->slices_a, u0, C->dpar,
                           C->part);
    });
    if (rc) return rc;
    hipLaunchKernelGGL(cpd_finish_a_kernel, gn, dim3(256), 0, ctx->stream, C->part, n, C->slices_a, C->dpar, C->den, C->x4, C->pt1);
    { const int rc_ = launched(ctx, "cpd_finish_a_kernel"); if (rc_) return rc_; }
    rc = cpd_pair_launches(ctx, blocks_m * C->slices_b, 256 * C->len_b, "cpd_pass_b_kernel", [&](int64_t u0, unsigned nw) {
        hipLaunchKernelGGL(cpd_pass_b_kernel, dim3(nw), dim3(256), 0, ctx->stream, C->t4, m, C->x4, n, C->len_b, C->slices_b, u0, C->dpar, C->part);
    });
    if (rc) return rc;
    hipLaunchKernelGGL(cpd_finish_b_kernel, gm, dim3(256), 0, ctx->stream, C->part, m, C->slices_b, C->p1, C->px);
    { const int rc_ = launched(ctx, "cpd_finish_b_kernel"); if (rc_) return rc_; }
    // the sums of the M-step
    const int nb1 = fixed_sums_grid(ctx, blocks_m), nb2 = fixed_sums_grid(ctx, blocks_m > blocks_n ? blocks_m : blocks_n);
    hipLaunchKernelGGL(cpd_stage1_kernel, dim3((unsigned)nb1), dim3(256), 0, ctx->stream, C->p1, C->px, C->qx, C->qy, C->qz, m, part1);
    rc = fixed_sums_reduce(ctx, part1, nb1, CPD_NT1, "cpd_stage1_kernel");
    if (rc) return rc;
    const double* tot1 = part1 + (int64_t)nb1 * CPD_NT1;
    hipLaunchKernelGGL(cpd_stage2_kernel, dim3((unsigned)nb2), dim3(256), 0, ctx->stream, tot1, C->p1, C->px, C->qx, C->qy, C->qz, m, C->pt1, C->rx, C->ry, C->rz, n,
                       part2);
    rc = fixed_sums_reduce(ctx, part2, nb2, CPD_NT2, "cpd_stage2_kernel");
    if (rc) return rc;
    double* d_out = C->dpar + 8;
    hipLaunchKernelGGL(cpd_results_kernel, dim3(1), dim3(64), 0, ctx->stream, tot1, part2 + (int64_t)nb2 * CPD_NT2, C->dpar, d_out);
    rc = launched(ctx, "cpd_results_kernel");
    (void)hipEventRecord(ctx->ev_stop, ctx->stream);
    ctx->timed = (rc == XDEMHIP_OK);
    if (rc) return rc;
    double h[CPD_NOUT];
    rc = xd_d2h(ctx, h, d_out, sizeof h);   // the one fetch of the call
    if (rc == XDEMHIP_OK) rc = xd_sync(ctx);
    if (rc) return rc;
    memcpy(sums_out, h, 18 * 8);
    *sigma2_used = h[18];
    C->stepped = true;
    return XDEMHIP_OK;
}

int xdemhip_cpd_terms(xdemhip_cpd* C, double* p1_out, double* pt1_out, double* px_out) {
    XdFetchScope fetch_scope_(C ? C->ctx : nullptr);
    if (!C) return XDEMHIP_EINVAL;
    xdemhip_ctx* ctx = C->ctx;
    if (!C->stepped) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_cpd_terms: no E-step was made");
    XD_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    if (p1_out) XD_HIP_CHECK(ctx, hipMemcpyAsync(p1_out, C->p1, (size_t)C->m * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (pt1_out) XD_HIP_CHECK(ctx, hipMemcpyAsync(pt1_out, C->pt1, (size_t)C->n * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (px_out) XD_HIP_CHECK(ctx, hipMemcpyAsync(px_out, C->px, (size_t)C->m * 24, hipMemcpyDeviceToHost, ctx->stream));
    return xd_sync(ctx);
}

}  // extern "C"
