// icp.hip -- ICP coregistration on gfx950: normal planes, the point clouds, the exact nearest-neighbour search, picky removal and the
// sums of the fit.
//
// Replaces, for raster-raster input (xdem/coreg/affine.py):
//   _icp_norms                                                           affine.py:1062-1081 -> icp_normals_kernel (once per plan)
//   _standardize_epc (np.median, nmad)                                   affine.py:296-328   -> exact selections (cloud_front.h)
//   scipy.spatial.KDTree(ref_epc.T).query(trans.T, k=1)                  affine.py:1013,1155 -> a uniform cell grid built by a counting
//                                                                                              sort, icp_query_kernel walking rings
//   picky duplicate removal (pandas groupby().idxmin())                  affine.py:1017-1021 -> three atomicMin passes, rank_select.h
//   _icp_fit_func and its least squares                                  affine.py:773-974   -> icp_sums_kernel: J^T J, J^T r
// Everything is float64 without contraction (-ffp-contract=off).  The search is exact: the squared distance is dx dx + dy dy + dz dz
// in that order, ties go to the lowest reference index, and a ring walk stops only when no unvisited cell can hold a point as near.
// The sums are added in a fixed order: two calls return the same bits (fixed_sums.h, shared with biascorr.hip and rigid.hip; the
// gradient stencil, the matrix product and the transform check are those of rigid.hip: rigid_geom.h).
#include <math.h>
#include <string.h>

#include <vector>

#include "common.h"
#include "select.h"
#include "select_run.h"
#include "rank_select.h"
#include "rigid_geom.h"
#include "dh_plan.h"
#include "cloud_front.h"

struct xdemhip_icp {
    xdemhip_ctx* ctx = nullptr;
    int64_t n = 0, m = 0;            // reference points, query points
    XdOwned mem;                     // every device allocation of the object
    double *rx = nullptr, *ry = nullptr, *rz = nullptr;   // reference cloud
    double *qx = nullptr, *qy = nullptr, *qz = nullptr;   // query cloud (qx, qy = rx, ry for a cloud made from a plan)
    double *nx = nullptr, *ny = nullptr, *nz = nullptr;   // normals at the reference points (null: none)
    // the cell grid over (rx, ry)
    double x0 = 0.0, y0 = 0.0, h = 1.0;
    int gx = 1, gy = 1;
    unsigned long long* cell_start = nullptr;   // gx * gy + 1 offsets into the sorted arrays
    double *sx = nullptr, *sy = nullptr, *sz = nullptr;
    int64_t* sidx = nullptr;
    // the last query
    double *tx = nullptr, *ty = nullptr, *tz = nullptr;   // the query cloud under the matrix
    int64_t* ind = nullptr;
    double* dist = nullptr;
    bool queried = false;
    // the pairs kept
    unsigned long long* best = nullptr;         // per reference point: smallest distance bits, then smallest query index
    unsigned long long* bestq = nullptr;
    uint8_t* has = nullptr;
    unsigned long long* tile_off = nullptr;
    int64_t* pair_r = nullptr;
    int64_t k = -1;
    bool picky = false;
    xd::FixedSums sums;                         // per-workgroup partials and totals of the fit's sums (fixed_sums.h)
};

namespace xd {
namespace {

constexpr int ICP_NS = 37;   // 21 upper-triangle terms of J J^T, 6 of J r, r^2, 9 moments of p' (squares, products, sums)
constexpr double ICP_OCCUPANCY = 3.0;

// ---- normal planes ---------------------------------------------------------------------------------------------------------------
// sin(arctan(g)) = g / sqrt(1 + g^2), evaluated in float64 and rounded once to the raster dtype (|g| = inf and beyond 1e150: +-1)
template <typename T> __device__ __forceinline__ T sin_atan(T g) {
    const double d = (double)g;
    if (d != d) return g;
    if (fabs(d) > 1e150) return (T)copysign(1.0, d);
    return (T)(d / sqrt(1.0 + d * d));
}

// np.gradient(ref) in the raster dtype (np_gradient_at, rigid_geom.h); nx = -sin(arctan(d/dcol / res_y)), ny = sin(arctan(d/drow / res_x)) -- upstream's pairing --
// nz = 1 - sqrt(nx^2 + ny^2) in the dtype.  valid[p] loses the pixels where a plane is not finite.  H, W >= 2.
template <typename T>
__global__ __launch_bounds__(256) void icp_normals_kernel(const T* __restrict__ ref, int64_t H, int64_t W, T res_x, T res_y, T* __restrict__ pnx,
                                                          T* __restrict__ pny, T* __restrict__ pnz, uint8_t* __restrict__ valid) {
    const int64_t n = H * W;
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = p / W, c = p - r * W;
        T gc, gr;
        np_gradient_at<T>(ref, H, W, r, c, gc, gr);
        const T vx = -sin_atan<T>(t_div(gc, res_y));
        const T vy = sin_atan<T>(t_div(gr, res_x));
        const T vz = t_sub((T)1, (T)sqrt(t_add(t_mul(vx, vx), t_mul(vy, vy))));
        pnx[p] = vx; pny[p] = vy; pnz[p] = vz;
        if (!(t_finite<T>(vx) && t_finite<T>(vy) && t_finite<T>(vz))) valid[p] = 0;
    }
}

// ---- the cell grid ---------------------------------------------------------------------------------------------------------------
struct Grid {
    double x0, y0, h;
    int gx, gy;
};
// the column / row of cells a coordinate falls in, clamped to the grid (the one rule of the build and of the query)
__device__ __forceinline__ int cell_of(double v, double v0, double h, int g) {
    double f = floor((v - v0) / h);
    if (!(f >= 0.0)) f = 0.0;
    if (f > (double)(g - 1)) f = (double)(g - 1);
    return (int)f;
}

// per-workgroup bounding box of (x, y): part[4 b + 0..3] = min x, max x, min y, max y
__global__ __launch_bounds__(256) void icp_bbox_kernel(const double* __restrict__ x, const double* __restrict__ y, int64_t n, double* __restrict__ part) {
    __shared__ double s[4][256];
    double a = INFINITY, b = -INFINITY, c = INFINITY, d = -INFINITY;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        a = fmin(a, x[i]); b = fmax(b, x[i]); c = fmin(c, y[i]); d = fmax(d, y[i]);
    }
    s[0][threadIdx.x] = a; s[1][threadIdx.x] = b; s[2][threadIdx.x] = c; s[3][threadIdx.x] = d;
    __syncthreads();
    for (int half = 128; half > 0; half >>= 1) {
        if ((int)threadIdx.x < half) {
            s[0][threadIdx.x] = fmin(s[0][threadIdx.x], s[0][threadIdx.x + half]);
            s[1][threadIdx.x] = fmax(s[1][threadIdx.x], s[1][threadIdx.x + half]);
            s[2][threadIdx.x] = fmin(s[2][threadIdx.x], s[2][threadIdx.x + half]);
            s[3][threadIdx.x] = fmax(s[3][threadIdx.x], s[3][threadIdx.x + half]);
        }
        __syncthreads();
    }
    if (threadIdx.x < 4) part[4 * (int64_t)blockIdx.x + threadIdx.x] = s[threadIdx.x][0];
}

// counting sort by cell: histogram, (rank_scan_kernel), scatter.  The order inside a cell is whatever the atomics give; the query
// breaks ties by the original index, so it does not show.
__global__ __launch_bounds__(256) void icp_cell_count_kernel(const double* __restrict__ x, const double* __restrict__ y, int64_t n, Grid g,
                                                             unsigned long long* __restrict__ cnt) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t c = (int64_t)cell_of(y[i], g.y0, g.h, g.gy) * g.gx + cell_of(x[i], g.x0, g.h, g.gx);
        atomicAdd(&cnt[c], 1ull);
    }
}
__global__ __launch_bounds__(256) void icp_cell_scatter_kernel(const double* __restrict__ x, const double* __restrict__ y, const double* __restrict__ z,
                                                               int64_t n, Grid g, const unsigned long long* __restrict__ start,
                                                               unsigned long long* __restrict__ cursor, double* __restrict__ sx, double* __restrict__ sy,
                                                               double* __restrict__ sz, int64_t* __restrict__ sidx) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t c = (int64_t)cell_of(y[i], g.y0, g.h, g.gy) * g.gx + cell_of(x[i], g.x0, g.h, g.gx);
        const unsigned long long o = start[c] + atomicAdd(&cursor[c], 1ull);
        if (o < (unsigned long long)n) { sx[o] = x[i]; sy[o] = y[i]; sz[o] = z[i]; sidx[o] = i; }
    }
}

// ---- the query -------------------------------------------------------------------------------------------------------------------
// One thread per query point: the point under the matrix, then rings of cells (Chebyshev distance 0, 1, 2, ... around the cell the
// point falls in, clamped to the grid).  A row of a ring's cells is one contiguous run of the sorted arrays.  After ring k every cell
// not yet seen lies beyond column cx -+ k or row cy -+ k: its points are at least `d` away in x or y, d taken from the point's own
// position (also outside the grid) less a rounding allowance; the walk ends once best < d^2 strictly, so no equal distance is missed.
__global__ __launch_bounds__(256) void icp_query_kernel(Grid g, const unsigned long long* __restrict__ start, const double* __restrict__ sx,
                                                        const double* __restrict__ sy, const double* __restrict__ sz, const int64_t* __restrict__ sidx,
                                                        const double* __restrict__ qx, const double* __restrict__ qy, const double* __restrict__ qz, int64_t m,
                                                        Mat12 M, double* __restrict__ tx, double* __restrict__ ty, double* __restrict__ tz,
                                                        int64_t* __restrict__ ind, double* __restrict__ dist) {
    const double EPS = 2.220446049250313e-16;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (int64_t)gridDim.x * blockDim.x) {
        double px, py, pz;
        mat12_apply(M.m, qx[i], qy[i], qz[i], px, py, pz);
        tx[i] = px; ty[i] = py; tz[i] = pz;
        const int cx = cell_of(px, g.x0, g.h, g.gx), cy = cell_of(py, g.y0, g.h, g.gy);
        int last = cx;
        if (g.gx - 1 - cx > last) last = g.gx - 1 - cx;
        if (cy > last) last = cy;
        if (g.gy - 1 - cy > last) last = g.gy - 1 - cy;
        double best = INFINITY;
        int64_t bi = -1;
        for (int ring = 0; ring <= last; ++ring) {
            const int ya = cy - ring, yb = cy + ring, xa = cx - ring, xb = cx + ring;
            const int xlo = xa < 0 ? 0 : xa, xhi = xb > g.gx - 1 ? g.gx - 1 : xb;
            for (int yy = (ya < 0 ? 0 : ya); yy <= (yb > g.gy - 1 ? g.gy - 1 : yb); ++yy) {
                const bool edge = yy == ya || yy == yb;
                // a full row of the ring, or its two end cells
                for (int part = 0; part < (edge ? 1 : 2); ++part) {
                    int c0, c1;
                    if (edge) { c0 = xlo; c1 = xhi; }
                    else if (part == 0) { if (xa < 0) continue; c0 = c1 = xa; }
                    else { if (xb > g.gx - 1 || ring == 0) continue; c0 = c1 = xb; }
                    const int64_t row = (int64_t)yy * g.gx;
                    const unsigned long long e = start[row + c1 + 1];
                    for (unsigned long long o = start[row + c0]; o < e; ++o) {
                        const double dx = px - sx[o], dy = py - sy[o], dz = pz - sz[o];
                        const double d2 = (dx * dx + dy * dy) + dz * dz;
                        const int64_t id = sidx[o];
                        if (d2 < best || (d2 == best && id < bi)) { best = d2; bi = id; }
                    }
                }
            }
            if (ring == last) break;
            double d = INFINITY;
            if (xa > 0) { const double b = g.x0 + (double)xa * g.h; d = fmin(d, (px - b) - 8.0 * EPS * ((fabs(g.x0) + fabs(b)) + fabs(px))); }
            if (xb < g.gx - 1) { const double b = g.x0 + (double)(xb + 1) * g.h; d = fmin(d, (b - px) - 8.0 * EPS * ((fabs(g.x0) + fabs(b)) + fabs(px))); }
            if (ya > 0) { const double b = g.y0 + (double)ya * g.h; d = fmin(d, (py - b) - 8.0 * EPS * ((fabs(g.y0) + fabs(b)) + fabs(py))); }
            if (yb < g.gy - 1) { const double b = g.y0 + (double)(yb + 1) * g.h; d = fmin(d, (b - py) - 8.0 * EPS * ((fabs(g.y0) + fabs(b)) + fabs(py))); }
            if (d > 0.0) {
                double lim = d * d;
                lim = lim - lim * (16.0 * EPS);
                if (best < lim) break;
            }
        }
        ind[i] = bi;
        dist[i] = sqrt(best);
    }
}

// ---- picky removal ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned long long bits_of(double v) { unsigned long long b; __builtin_memcpy(&b, &v, 8); return b; }

__global__ __launch_bounds__(256) void icp_fill_kernel(unsigned long long* __restrict__ a, unsigned long long* __restrict__ b, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) { a[i] = ~0ull; b[i] = ~0ull; }
}
// pass 1: per reference index the smallest distance (non-negative doubles order as their bits)
__global__ __launch_bounds__(256) void icp_picky1_kernel(const int64_t* __restrict__ ind, const double* __restrict__ dist, int64_t m, int64_t n,
                                                         unsigned long long* __restrict__ best) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t j = ind[i];
        if (j >= 0 && j < n) atomicMin(&best[j], bits_of(dist[i]));
    }
}
// pass 2: among the queries at that distance, the smallest query index (pandas idxmin: the first occurrence)
__global__ __launch_bounds__(256) void icp_picky2_kernel(const int64_t* __restrict__ ind, const double* __restrict__ dist, int64_t m, int64_t n,
                                                         const unsigned long long* __restrict__ best, unsigned long long* __restrict__ bestq) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t j = ind[i];
        if (j >= 0 && j < n && bits_of(dist[i]) == best[j]) atomicMin(&bestq[j], (unsigned long long)i);
    }
}
// pass 3: the keep flag, per reference index (one pair each: compacting the flags gives the pairs in reference-index order)
__global__ __launch_bounds__(256) void icp_picky3_kernel(const unsigned long long* __restrict__ bestq, int64_t n, uint8_t* __restrict__ has) {
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += (int64_t)gridDim.x * blockDim.x) has[j] = bestq[j] != ~0ull ? 1 : 0;
}

// ---- the sums of the fit ---------------------------------------------------------------------------------------------------------
struct PairSrc {
    const int64_t* pair_r;              // picky: the reference indexes kept, ascending; else null
    const unsigned long long* bestq;    // picky: the query index of each reference index
    const int64_t* ind;                 // not picky: pair p = (query p, ind[p])
};
__device__ __forceinline__ void pair_of(const PairSrc& s, int64_t p, int64_t& qi, int64_t& ri) {
    if (s.pair_r) { ri = s.pair_r[p]; qi = (int64_t)s.bestq[ri]; }
    else { qi = p; ri = s.ind[p]; }
}

// For every kept pair: p' = S t, the residual r and its row J = [p' x n, n] (point-to-plane, r = (p' - q) . n) or [p' x u, u]
// (point-to-point, r = |p' - q|, u = (p' - q) / r, a zero row where r = 0) about p', and the nine moments of p' from which the host
// forms the normal matrix of the vector residual p' - q (point-to-point: the rows of the scalar distance leave out r grad^2 r =
// I - u u^T, which is not small).  Per-lane accumulators, one partial per workgroup (block_sums_store, fixed_sums.h):
// part[b * (ICP_NS + 1) + k], slot ICP_NS = the count.
__global__ __launch_bounds__(256) void icp_sums_kernel(PairSrc src, int64_t k, const double* __restrict__ tx, const double* __restrict__ ty,
                                                       const double* __restrict__ tz, const double* __restrict__ rx, const double* __restrict__ ry,
                                                       const double* __restrict__ rz, const double* __restrict__ nx, const double* __restrict__ ny,
                                                       const double* __restrict__ nz, Mat12 S, int plane, double* __restrict__ part) {
    __shared__ double red[4];
    double s[ICP_NS];
#pragma unroll
    for (int t = 0; t < ICP_NS; ++t) s[t] = 0.0;
    double cnt = 0.0;
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < k; p += (int64_t)gridDim.x * blockDim.x) {
        int64_t qi, ri;
        pair_of(src, p, qi, ri);
        if (ri < 0 || qi < 0) continue;   // (a query that found nothing: a non-finite point)
        double px, py, pz;
        mat12_apply(S.m, tx[qi], ty[qi], tz[qi], px, py, pz);
        const double dx = px - rx[ri], dy = py - ry[ri], dz = pz - rz[ri];
        double ux, uy, uz, r;
        if (plane) {
            ux = nx[ri]; uy = ny[ri]; uz = nz[ri];
            r = (dx * ux + dy * uy) + dz * uz;
        } else {
            r = sqrt((dx * dx + dy * dy) + dz * dz);
            if (r > 0.0) { ux = dx / r; uy = dy / r; uz = dz / r; }
            else { ux = uy = uz = 0.0; }
        }
        const double a[6] = {py * uz - pz * uy, pz * ux - px * uz, px * uy - py * ux, ux, uy, uz};
        int t = 0;
#pragma unroll
        for (int i = 0; i < 6; ++i)
#pragma unroll
            for (int j = i; j < 6; ++j) s[t++] += a[i] * a[j];
#pragma unroll
        for (int i = 0; i < 6; ++i) s[21 + i] += a[i] * r;
        s[27] += r * r;
        s[28] += px * px; s[29] += py * py; s[30] += pz * pz;
        s[31] += px * py; s[32] += px * pz; s[33] += py * pz;
        s[34] += px; s[35] += py; s[36] += pz;
        cnt += 1.0;
    }
    block_sums_store<ICP_NS>(s, cnt, red, part);
}

// the kept pairs as upstream hands them to _icp_fit: out rows 0-2 = ref, 3-5 = the moved query points, 6-8 = the normals (k each)
__global__ __launch_bounds__(256) void icp_values_kernel(PairSrc src, int64_t k, const double* __restrict__ tx, const double* __restrict__ ty,
                                                         const double* __restrict__ tz, const double* __restrict__ rx, const double* __restrict__ ry,
                                                         const double* __restrict__ rz, const double* __restrict__ nx, const double* __restrict__ ny,
                                                         const double* __restrict__ nz, double* __restrict__ out, int64_t* __restrict__ pq,
                                                         int64_t* __restrict__ pr) {
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < k; p += (int64_t)gridDim.x * blockDim.x) {
        int64_t qi, ri;
        pair_of(src, p, qi, ri);
        if (ri < 0 || qi < 0) { ri = 0; qi = 0; }
        if (out) {
            out[p] = rx[ri]; out[k + p] = ry[ri]; out[2 * k + p] = rz[ri];
            out[3 * k + p] = tx[qi]; out[4 * k + p] = ty[qi]; out[5 * k + p] = tz[qi];
            out[6 * k + p] = nx ? nx[ri] : 0.0; out[7 * k + p] = nx ? ny[ri] : 0.0; out[8 * k + p] = nx ? nz[ri] : 0.0;
        }
        if (pq) { pq[p] = qi; pr[p] = ri; }
    }
}

// ---- host side -------------------------------------------------------------------------------------------------------------------
// The grid over the reference cloud: cells of side h with about ICP_OCCUPANCY points each, from the bounding box and n; an axis of
// zero extent gets one row of cells, and h is never below what a one-dimensional cloud needs (so the cells number at most ~ n).
int icp_build_grid(xdemhip_icp* I) {
    xdemhip_ctx* ctx = I->ctx;
    const int64_t n = I->n;
    const int nb = grid_for(ctx, n, 256, 4);
    double* d_box = I->mem.take<double>((size_t)nb * 4, "ICP bounding box");
    if (I->mem.rc) return I->mem.rc;
    hipLaunchKernelGGL(icp_bbox_kernel, dim3((unsigned)nb), dim3(256), 0, ctx->stream, I->rx, I->ry, n, d_box);
    { const int rc_ = launched(ctx, "icp_bbox_kernel"); if (rc_) return rc_; }
    std::vector<double> hb((size_t)nb * 4);
    XD_HIP_CHECK(ctx, hipMemcpyAsync(hb.data(), d_box, (size_t)nb * 32, hipMemcpyDeviceToHost, ctx->stream));
    { const int rc_ = xd_sync(ctx); if (rc_) return rc_; }
    double x0 = INFINITY, x1 = -INFINITY, y0 = INFINITY, y1 = -INFINITY;
    for (int b = 0; b < nb; ++b) {
        x0 = fmin(x0, hb[4 * b]); x1 = fmax(x1, hb[4 * b + 1]); y0 = fmin(y0, hb[4 * b + 2]); y1 = fmax(y1, hb[4 * b + 3]);
    }
    if (!isfinite(x0) || !isfinite(x1) || !isfinite(y0) || !isfinite(y1)) return xd_fail(ctx, XDEMHIP_EINVAL, "ICP: the reference cloud must be finite");
    const double wx = x1 - x0, wy = y1 - y0, wl = wx > wy ? wx : wy;
    double h = sqrt(wx * wy * ICP_OCCUPANCY / (double)n);
    const double h1 = wl * ICP_OCCUPANCY / (double)n;
    if (!(h > h1)) h = h1;
    if (!(h > 0.0) || !isfinite(h)) h = 1.0;
    const double limit = 2.0 * (double)n + 16.0;
    double fx = floor(wx / h) + 1.0, fy = floor(wy / h) + 1.0;
    if (!(fx >= 1.0)) fx = 1.0;
    if (!(fy >= 1.0)) fy = 1.0;
    if (fx > limit) fx = limit;
    if (fy > limit) fy = limit;
    while (fx * fy > 4.0 * limit) { if (fx > fy) fx = ceil(fx / 2); else fy = ceil(fy / 2); }   // (cannot happen for h >= h1; a guard)
    I->x0 = x0; I->y0 = y0; I->h = h; I->gx = (int)fx; I->gy = (int)fy;
    const int64_t ncell = (int64_t)I->gx * I->gy;
    XdOwned& mem = I->mem;
    I->cell_start = mem.take<unsigned long long>((size_t)ncell + 1, "ICP cells");
    unsigned long long* cursor = mem.take<unsigned long long>((size_t)ncell, "ICP cells");
    I->sx = mem.take<double>((size_t)n, "ICP sorted cloud");
    I->sy = mem.take<double>((size_t)n, "ICP sorted cloud");
    I->sz = mem.take<double>((size_t)n, "ICP sorted cloud");
    I->sidx = mem.take<int64_t>((size_t)n, "ICP sorted cloud");
    if (mem.rc) return mem.rc;
    XD_HIP_CHECK(ctx, hipMemsetAsync(I->cell_start, 0, (size_t)(ncell + 1) * 8, ctx->stream));
    XD_HIP_CHECK(ctx, hipMemsetAsync(cursor, 0, (size_t)ncell * 8, ctx->stream));
    const Grid g = {I->x0, I->y0, I->h, I->gx, I->gy};
    const dim3 grid(grid_for(ctx, n, 256, 16));
    hipLaunchKernelGGL(icp_cell_count_kernel, grid, dim3(256), 0, ctx->stream, I->rx, I->ry, n, g, I->cell_start);
    hipLaunchKernelGGL(rank_scan_kernel, dim3(1), dim3(1024), 0, ctx->stream, I->cell_start, ncell, I->cell_start + ncell);
    hipLaunchKernelGGL(icp_cell_scatter_kernel, grid, dim3(256), 0, ctx->stream, I->rx, I->ry, I->rz, n, g, I->cell_start, cursor, I->sx, I->sy, I->sz,
                       I->sidx);
    return launched(ctx, "ICP grid build");
}

// the arrays of the query and of the pairs, sized once the clouds are known
int icp_alloc_work(xdemhip_icp* I) {
    const size_t n = (size_t)I->n, m = (size_t)I->m;
    XdOwned& mem = I->mem;
    I->tx = mem.take<double>(m, "ICP query");
    I->ty = mem.take<double>(m, "ICP query");
    I->tz = mem.take<double>(m, "ICP query");
    I->ind = mem.take<int64_t>(m, "ICP query");
    I->dist = mem.take<double>(m, "ICP query");
    I->best = mem.take<unsigned long long>(n, "ICP pairs");
    I->bestq = mem.take<unsigned long long>(n, "ICP pairs");
    I->has = mem.take<uint8_t>(n + 16, "ICP pairs");
    I->tile_off = mem.take<unsigned long long>((n + RANK_TILE - 1) / RANK_TILE + 2, "ICP pairs");
    I->pair_r = mem.take<int64_t>(n, "ICP pairs");
    return mem.rc;
}

PairSrc pair_src(const xdemhip_icp* I) {
    PairSrc s;
    s.pair_r = I->picky ? I->pair_r : nullptr;
    s.bestq = I->bestq;
    s.ind = I->ind;
    return s;
}

template <typename T>
int normals_typed(xdemhip_dh_plan* P, double res_x, double res_y) {
    xdemhip_ctx* ctx = P->ctx;
    const int64_t n = P->H * P->W;
    P->mem.optional();   // (three planes or none: a plan without them can be asked again)
    for (int a = 0; a < 3; ++a) P->icp_n[a] = P->mem.take((size_t)n * sizeof(T), "ICP normal planes");
    if (!P->mem.all_or_none(P->icp_n[0], P->icp_n[1], P->icp_n[2])) return xd_fail(ctx, XDEMHIP_ENOMEM, "hipMalloc failed (ICP normal planes)");
    hipLaunchKernelGGL((icp_normals_kernel<T>), dim3(grid_for(ctx, n, 256, 16)), dim3(256), 0, ctx->stream, static_cast<const T*>(P->ref), P->H, P->W, (T)res_x,
                       (T)res_y, static_cast<T*>(P->icp_n[0]), static_cast<T*>(P->icp_n[1]), static_cast<T*>(P->icp_n[2]), P->valid);
    // the tiles' counts of the narrowed mask, scanned: the subsample ranks and the pixel list follow the new mask
    hipLaunchKernelGGL((rank_select_kernel<RankOut::Count>), dim3((unsigned)P->n_tiles), dim3(256), 0, ctx->stream, P->valid, n,
                       (const unsigned long long*)nullptr, (const uint8_t*)nullptr, P->tile_off, (int64_t*)nullptr, (uint8_t*)nullptr);
    hipLaunchKernelGGL(rank_scan_kernel, dim3(1), dim3(1024), 0, ctx->stream, P->tile_off, P->n_tiles, P->tile_off + P->n_tiles);
    return launched(ctx, "icp_normals_kernel");
}

}  // namespace
}  // namespace xd

using namespace xd;

extern "C" {

int xdemhip_dh_icp_normals(xdemhip_dh_plan* P, const double* transform6, void* nx_out, void* ny_out, void* nz_out, int memspace, int64_t* n_valid) {
    XdFetchScope fetch_scope_(P ? P->ctx : nullptr);
    if (!P) return XDEMHIP_EINVAL;
    xdemhip_ctx* ctx = P->ctx;
    if (memspace != XDEMHIP_HOST && memspace != XDEMHIP_DEVICE) return xd_fail(ctx, XDEMHIP_EINVAL, "bad memspace");
    { const int rc_ = check_transform(ctx, transform6, "xdemhip_dh_icp_normals"); if (rc_) return rc_; }
    if (P->H < 2 || P->W < 2) return xd_fail(ctx, XDEMHIP_EINVAL, "ICP normals need a raster of at least 2 x 2 pixels (np.gradient)");
    XD_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    const double res_x = fabs(transform6[0]), res_y = fabs(transform6[4]);
    if (!P->icp_n[0]) {
        if (P->drawn || P->idx) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_dh_icp_normals: the normal planes narrow the valid mask and must be made before the draw");
        { const int rc_ = dh_ensure_mask(P); if (rc_) return rc_; }
        const int rc = P->dtype == XDEMHIP_F32 ? normals_typed<float>(P, res_x, res_y) : normals_typed<double>(P, res_x, res_y);
        if (rc) return rc;
        unsigned long long total = 0;
        { const int rc_ = xd_d2h(ctx, &total, P->tile_off + P->n_tiles, 8); if (rc_) return rc_; }
        { const int rc_ = xd_sync(ctx); if (rc_) return rc_; }
        P->n_valid = (int64_t)total;
        P->icp_res_x = res_x; P->icp_res_y = res_y;
    } else if (P->icp_res_x != res_x || P->icp_res_y != res_y) {
        return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_dh_icp_normals: the plan's normal planes were made for another resolution");
    }
    if (n_valid) *n_valid = P->n_valid;
    const size_t bytes = (size_t)(P->H * P->W) * (P->dtype == XDEMHIP_F32 ? 4 : 8);
    const hipMemcpyKind kind = memspace == XDEMHIP_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    void* outs[3] = {nx_out, ny_out, nz_out};
    for (int a = 0; a < 3; ++a)
        if (outs[a]) XD_HIP_CHECK(ctx, hipMemcpyAsync(outs[a], P->icp_n[a], bytes, kind, ctx->stream));
    return xd_sync(ctx);
}

void xdemhip_icp_destroy(xdemhip_icp* I) { delete I; }

int xdemhip_icp_create_plan(xdemhip_dh_plan* P, const double* transform6, int with_normals, int standardize, xdemhip_icp** out, double* centroid3,
                            double* std_fac, int64_t* count) {
    XdFetchScope fetch_scope_(P ? P->ctx : nullptr);
    if (!P) return XDEMHIP_EINVAL;
    xdemhip_ctx* ctx = P->ctx;
    if (!out || !centroid3 || !std_fac) return xd_fail(ctx, XDEMHIP_EINVAL, "null argument");
    { const int rc_ = check_transform(ctx, transform6, "xdemhip_icp_create_plan"); if (rc_) return rc_; }
    if (with_normals && !P->icp_n[0]) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_icp_create_plan: call xdemhip_dh_icp_normals first");
    XD_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    { const int rc_ = dh_ensure_valid_idx(P); if (rc_) return rc_; }
    const int64_t n = P->n_idx;
    if (count) *count = n;
    if (n == 0) return xd_fail(ctx, XDEMHIP_EINVAL, "no valid points");
    xdemhip_icp* I = new xdemhip_icp();
    I->ctx = I->mem.ctx = ctx; I->n = n; I->m = n;
    auto fail = [&](int code) { delete I; return code; };
    CloudFront C;   // the gather and the standardisation: cloud_front.h, shared with cpd.hip
    int rc = cloud_front_build(P, transform6, with_normals != 0, standardize != 0, "ICP", I->mem, C, centroid3, std_fac);
    if (rc) return fail(rc);
    I->rx = I->qx = C.x; I->ry = I->qy = C.y; I->rz = C.zr; I->qz = C.zt;
    I->nx = C.nx; I->ny = C.ny; I->nz = C.nz;
    rc = icp_build_grid(I);
    if (rc == XDEMHIP_OK) rc = icp_alloc_work(I);
    if (rc == XDEMHIP_OK) rc = xd_sync(ctx);
    if (rc) return fail(rc);
    *out = I;
    return XDEMHIP_OK;
}

int xdemhip_icp_create_points(xdemhip_ctx* ctx, const double* ref3n, int64_t n, const double* query3m, int64_t m, const double* norms3n_or_null,
                              xdemhip_icp** out) {
    XdFetchScope fetch_scope_(ctx);
    if (!ctx) return XDEMHIP_EINVAL;
    if (!ref3n || !query3m || !out) return xd_fail(ctx, XDEMHIP_EINVAL, "null argument");
    if (n < 1 || m < 1) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_icp_create_points: both clouds need at least one point");
    XD_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    xdemhip_icp* I = new xdemhip_icp();
    I->ctx = I->mem.ctx = ctx; I->n = n; I->m = m;
    auto fail = [&](int code) { delete I; return code; };
    double* r = I->mem.keep(ref3n, (size_t)n * 24, XDEMHIP_HOST, "ICP clouds");
    double* q = I->mem.keep(query3m, (size_t)m * 24, XDEMHIP_HOST, "ICP clouds");
    double* nn = I->mem.keep(norms3n_or_null, (size_t)n * 24, XDEMHIP_HOST, "ICP clouds");
    int rc = I->mem.rc;
    if (rc) return fail(rc);
    I->rx = r; I->ry = r + n; I->rz = r + 2 * n;
    I->qx = q; I->qy = q + m; I->qz = q + 2 * m;
    if (nn) { I->nx = nn; I->ny = nn + n; I->nz = nn + 2 * n; }
    rc = icp_build_grid(I);
    if (rc == XDEMHIP_OK) rc = icp_alloc_work(I);
    if (rc == XDEMHIP_OK) rc = xd_sync(ctx);
    if (rc) return fail(rc);
    *out = I;
    return XDEMHIP_OK;
}

int xdemhip_icp_cloud(xdemhip_icp* I, double* out7n) {
    XdFetchScope fetch_scope_(I ? I->ctx : nullptr);
    if (!I) return XDEMHIP_EINVAL;
    xdemhip_ctx* ctx = I->ctx;
    if (!out7n) return xd_fail(ctx, XDEMHIP_EINVAL, "null argument");
    if (I->n != I->m) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_icp_cloud: for clouds made from a plan");
    XD_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    const size_t row = (size_t)I->n * 8;
    const double* rows[7] = {I->rx, I->ry, I->rz, I->qz, I->nx, I->ny, I->nz};
    for (int a = 0; a < 7; ++a) {
        if (rows[a]) XD_HIP_CHECK(ctx, hipMemcpyAsync(out7n + (size_t)a * I->n, rows[a], row, hipMemcpyDeviceToHost, ctx->stream));
        else memset(out7n + (size_t)a * I->n, 0, row);
    }
    return xd_sync(ctx);
}

int xdemhip_icp_grid(xdemhip_icp* I, double* x0_y0_h, int64_t* gx_gy) {
    if (!I) return XDEMHIP_EINVAL;
    if (!x0_y0_h || !gx_gy) return xd_fail(I->ctx, XDEMHIP_EINVAL, "null argument");
    x0_y0_h[0] = I->x0; x0_y0_h[1] = I->y0; x0_y0_h[2] = I->h;
    gx_gy[0] = I->gx; gx_gy[1] = I->gy;
    return XDEMHIP_OK;
}

int xdemhip_icp_query(xdemhip_icp* I, const double* matrix16_or_null, int64_t* ind_out, double* dist_out) {
    XdFetchScope fetch_scope_(I ? I->ctx : nullptr);
    if (!I) return XDEMHIP_EINVAL;
    xdemhip_ctx* ctx = I->ctx;
    XD_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    Mat12 M;
    const double eye[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    memcpy(M.m, matrix16_or_null ? matrix16_or_null : eye, sizeof M.m);
    const Grid g = {I->x0, I->y0, I->h, I->gx, I->gy};
    (void)hipEventRecord(ctx->ev_start, ctx->stream);
    hipLaunchKernelGGL(icp_query_kernel, dim3(grid_for(ctx, I->m, 256, 64)), dim3(256), 0, ctx->stream, g, I->cell_start, I->sx, I->sy, I->sz, I->sidx, I->qx,
                       I->qy, I->qz, I->m, M, I->tx, I->ty, I->tz, I->ind, I->dist);
    const int rc = launched(ctx, "icp_query_kernel");
    (void)hipEventRecord(ctx->ev_stop, ctx->stream);
    ctx->timed = (rc == XDEMHIP_OK);
    if (rc) return rc;
    I->queried = true;
    I->k = -1;
    if (ind_out) XD_HIP_CHECK(ctx, hipMemcpyAsync(ind_out, I->ind, (size_t)I->m * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (dist_out) XD_HIP_CHECK(ctx, hipMemcpyAsync(dist_out, I->dist, (size_t)I->m * 8, hipMemcpyDeviceToHost, ctx->stream));
    return (ind_out || dist_out) ? xd_sync(ctx) : XDEMHIP_OK;
}

int xdemhip_icp_set_pairs(xdemhip_icp* I, const int64_t* ind, const double* dist) {
    XdFetchScope fetch_scope_(I ? I->ctx : nullptr);
    if (!I) return XDEMHIP_EINVAL;
    xdemhip_ctx* ctx = I->ctx;
    if (!ind || !dist) return xd_fail(ctx, XDEMHIP_EINVAL, "null argument");
    for (int64_t i = 0; i < I->m; ++i)
        if (ind[i] < 0 || ind[i] >= I->n || !(dist[i] >= 0.0)) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_icp_set_pairs: 0 <= ind < n and dist >= 0");
    XD_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    XD_HIP_CHECK(ctx, hipMemcpyAsync(I->ind, ind, (size_t)I->m * 8, hipMemcpyHostToDevice, ctx->stream));
    XD_HIP_CHECK(ctx, hipMemcpyAsync(I->dist, dist, (size_t)I->m * 8, hipMemcpyHostToDevice, ctx->stream));
    XD_HIP_CHECK(ctx, hipMemcpyAsync(I->tx, I->qx, (size_t)I->m * 8, hipMemcpyDeviceToDevice, ctx->stream));
    XD_HIP_CHECK(ctx, hipMemcpyAsync(I->ty, I->qy, (size_t)I->m * 8, hipMemcpyDeviceToDevice, ctx->stream));
    XD_HIP_CHECK(ctx, hipMemcpyAsync(I->tz, I->qz, (size_t)I->m * 8, hipMemcpyDeviceToDevice, ctx->stream));
    I->queried = true;
    I->k = -1;
    return xd_sync(ctx);
}

int xdemhip_icp_pairs(xdemhip_icp* I, int picky, int64_t* n_kept, int64_t* query_idx_out, int64_t* ref_idx_out) {
    XdFetchScope fetch_scope_(I ? I->ctx : nullptr);
    if (!I) return XDEMHIP_EINVAL;
    xdemhip_ctx* ctx = I->ctx;
    if (!n_kept) return xd_fail(ctx, XDEMHIP_EINVAL, "null argument");
    if (!I->queried) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_icp_pairs: no query was made");
    XD_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    const int64_t n = I->n, m = I->m;
    I->picky = picky != 0;
    if (picky) {
        const int64_t n_tiles = (n + RANK_TILE - 1) / RANK_TILE;
        const dim3 gn(grid_for(ctx, n, 256, 16)), gm(grid_for(ctx, m, 256, 16));
        hipLaunchKernelGGL(icp_fill_kernel, gn, dim3(256), 0, ctx->stream, I->best, I->bestq, n);
        hipLaunchKernelGGL(icp_picky1_kernel, gm, dim3(256), 0, ctx->stream, I->ind, I->dist, m, n, I->best);
        hipLaunchKernelGGL(icp_picky2_kernel, gm, dim3(256), 0, ctx->stream, I->ind, I->dist, m, n, I->best, I->bestq);
        hipLaunchKernelGGL(icp_picky3_kernel, gn, dim3(256), 0, ctx->stream, I->bestq, n, I->has);
        hipLaunchKernelGGL((rank_select_kernel<RankOut::Count>), dim3((unsigned)n_tiles), dim3(256), 0, ctx->stream, I->has, n, (const unsigned long long*)nullptr,
                           (const uint8_t*)nullptr, I->tile_off, (int64_t*)nullptr, (uint8_t*)nullptr);
        hipLaunchKernelGGL(rank_scan_kernel, dim3(1), dim3(1024), 0, ctx->stream, I->tile_off, n_tiles, I->tile_off + n_tiles);
        hipLaunchKernelGGL((rank_select_kernel<RankOut::List>), dim3((unsigned)n_tiles), dim3(256), 0, ctx->stream, I->has, n, (const unsigned long long*)nullptr,
                           (const uint8_t*)nullptr, I->tile_off, I->pair_r, (uint8_t*)nullptr);
        { const int rc_ = launched(ctx, "ICP picky removal"); if (rc_) return rc_; }
        unsigned long long total = 0;
        { const int rc_ = xd_d2h(ctx, &total, I->tile_off + n_tiles, 8); if (rc_) return rc_; }
        { const int rc_ = xd_sync(ctx); if (rc_) return rc_; }
        I->k = (int64_t)total;
    } else {
        I->k = m;
    }
    *n_kept = I->k;
    if ((query_idx_out || ref_idx_out) && I->k > 0) {
        if (!query_idx_out || !ref_idx_out) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_icp_pairs: both index outputs or none");
        XdBuffers buf(ctx, "xdemhip_icp_pairs");
        int64_t* d = buf.alloc<int64_t>((size_t)I->k * 2);
        if (buf.rc) return buf.rc;
        hipLaunchKernelGGL(icp_values_kernel, dim3(grid_for(ctx, I->k, 256, 16)), dim3(256), 0, ctx->stream, pair_src(I), I->k, I->tx, I->ty, I->tz, I->rx, I->ry,
                           I->rz, I->nx, I->ny, I->nz, (double*)nullptr, d, d + I->k);
        int rc = launched(ctx, "icp_values_kernel");
        if (rc == XDEMHIP_OK && (hipMemcpyAsync(query_idx_out, d, (size_t)I->k * 8, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
                                 hipMemcpyAsync(ref_idx_out, d + I->k, (size_t)I->k * 8, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess))
            rc = xd_fail(ctx, XDEMHIP_EHIP, "D2H copy failed");
        return rc == XDEMHIP_OK ? xd_sync(ctx) : rc;
    }
    return XDEMHIP_OK;
}

int xdemhip_icp_sums(xdemhip_icp* I, const double* step16, int method, double* sums_out, int64_t* count) {
    XdFetchScope fetch_scope_(I ? I->ctx : nullptr);
    if (!I) return XDEMHIP_EINVAL;
    xdemhip_ctx* ctx = I->ctx;
    if (!step16 || !sums_out || !count) return xd_fail(ctx, XDEMHIP_EINVAL, "null argument");
    if (method != 0 && method != 1) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_icp_sums: method 0 (point-to-point) or 1 (point-to-plane)");
    if (method == 1 && !I->nx) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_icp_sums: point-to-plane needs normals");
    if (I->k < 0) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_icp_sums: call xdemhip_icp_pairs first");
    *count = 0;
    if (I->k == 0) return xd_fail(ctx, XDEMHIP_EINVAL, "no valid points");
    XD_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    const int NT = ICP_NS + 1;
    const int nb = fixed_sums_grid(ctx, (I->k + 255) / 256);
    { const int rc_ = I->sums.reserve(I->mem, NT, "ICP partial sums"); if (rc_) return rc_; }
    Mat12 S;
    memcpy(S.m, step16, sizeof S.m);
    (void)hipEventRecord(ctx->ev_start, ctx->stream);
    hipLaunchKernelGGL(icp_sums_kernel, dim3((unsigned)nb), dim3(256), 0, ctx->stream, pair_src(I), I->k, I->tx, I->ty, I->tz, I->rx, I->ry, I->rz, I->nx, I->ny,
                       I->nz, S, method, I->sums.part);
    double h[ICP_NS + 1];
    { const int rc_ = fixed_sums_finish(ctx, I->sums, nb, NT, "icp_sums_kernel", h); if (rc_) return rc_; }
    memcpy(sums_out, h, ICP_NS * 8);
    *count = (int64_t)h[ICP_NS];
    return XDEMHIP_OK;
}

int xdemhip_icp_values(xdemhip_icp* I, double* out9k) {
    XdFetchScope fetch_scope_(I ? I->ctx : nullptr);
    if (!I) return XDEMHIP_EINVAL;
    xdemhip_ctx* ctx = I->ctx;
    if (!out9k) return xd_fail(ctx, XDEMHIP_EINVAL, "null argument");
    if (I->k < 0) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_icp_values: call xdemhip_icp_pairs first");
    if (I->k == 0) return xd_fail(ctx, XDEMHIP_EINVAL, "no valid points");
    XD_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    XdBuffers buf(ctx, "xdemhip_icp_values");
    double* d = buf.alloc<double>((size_t)I->k * 9);
    if (buf.rc) return buf.rc;
    hipLaunchKernelGGL(icp_values_kernel, dim3(grid_for(ctx, I->k, 256, 16)), dim3(256), 0, ctx->stream, pair_src(I), I->k, I->tx, I->ty, I->tz, I->rx, I->ry, I->rz,
                       I->nx, I->ny, I->nz, d, (int64_t*)nullptr, (int64_t*)nullptr);
    int rc = launched(ctx, "icp_values_kernel");
    if (rc == XDEMHIP_OK && hipMemcpyAsync(out9k, d, (size_t)I->k * 72, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess) rc = xd_fail(ctx, XDEMHIP_EHIP, "D2H copy failed");
    return rc == XDEMHIP_OK ? xd_sync(ctx) : rc;
}

}  // extern "C"
