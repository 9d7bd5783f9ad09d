// ptsplan.hip -- raster-point coregistration on gfx950: everything of NuthKaab, DhMinimize and VerticalShift that touches the raster or
// the cloud when one of the two elevation datasets is a point cloud (xdem/coreg/affine.py:150-243 with base.py:624-706), and the
// matrix applied to a cloud (base.py: _apply_matrix_pts_arr).
//
//   _get_subsample_mask_pts_rst (base.py:674-704)        -> pts_valid_plane_kernel + pts_valid_kernel (once), rank_select.h
//   _interp_points of slope tangent / aspect              -> pts_valid_kernel (once, at zero shift)
//   sub_dh_interpolator (affine.py:217-231)               -> pts_dh_kernel: one 4-tap gather per point and evaluation
//   _nuth_kaab_iteration_step (affine.py:477-536)         -> xdemhip_pts_nk_step: the gather, two exact selections, one fetch
//   _dh_minimize_fit's objective (affine.py:636-674)      -> xdemhip_pts_shift_nmad (dh_eval.h)
//
// A point's position on the raster is (row, col) = ((y - f) / e - 0.5, (x - c) / a - 0.5), every float64 operation rounded on its
// own (-ffp-contract=off); the tap is bi_point under the option "nk_nan_rule".  Every pass after the gather reads its columns in cloud
// order, so two runs return the same bits whatever order the gather walked the points in (test switch "pts_tile_order").
#include <math.h>
#include <string.h>

#include <string>
#include <vector>

#include "common.h"
#include "select.h"
#include "select_run.h"
#include "rank_select.h"
#include "nk_geom.h"
#include "nk_aux.h"
#include "bi_point.h"
#include "rigid_geom.h"
#include "fixed_sums.h"
#include "dh_eval.h"
#include "pts_plan.h"

namespace xd {
namespace {

constexpr int PTS_MAX_BINS = 1024;
constexpr int PTS_TILE_LOG2 = 5;   // the gather's buckets: raster tiles of 32 x 32 pixels (one tile row of float32 = one 128-byte line)

// where a point lies on the raster: the geotransform and the shift of one evaluation (already signed: + for a point reference, - for a
// raster reference)
struct PtsGeo { double a, c, e, f, sx, sy; };
__device__ __forceinline__ void pts_row_col(const PtsGeo& q, double x, double y, double& row, double& col) {
    const double xs = x + q.sx, ys = y + q.sy;
    row = (ys - q.f) / q.e - 0.5;
    col = (xs - q.c) / q.a - 0.5;
}

// ---- creation ---------------------------------------------------------------------------------------------------------------------
// the validity plane as upstream interpolates it: 1 where the raster pixel is usable, NaN elsewhere (float32 whatever the raster is)
template <typename T>
__global__ __launch_bounds__(256) void pts_valid_plane_kernel(const T* __restrict__ raster, const uint8_t* __restrict__ inlier,
                                                              const uint8_t* __restrict__ valid, int64_t n, float* __restrict__ plane) {
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (int64_t)gridDim.x * blockDim.x) {
        const bool ok = valid ? valid[p] != 0 : ((inlier == nullptr || inlier[p] != 0) && t_finite(raster[p]));
        plane[p] = ok ? 1.0f : NAN;
    }
}

// per point: valid iff (x, y, z) are finite and the tap rule accepts the validity plane at the unshifted position; with the aux
// planes, slope tangent and aspect interpolated there (raster dtype)
template <typename T>
__global__ __launch_bounds__(256) void pts_valid_kernel(const float* __restrict__ plane, NkGeom g, PtsGeo q, const double* __restrict__ x,
                                                        const double* __restrict__ y, const T* __restrict__ z, int64_t n,
                                                        const T* __restrict__ st_plane, const T* __restrict__ asp_plane,
                                                        uint8_t* __restrict__ pvalid, T* __restrict__ a_st, T* __restrict__ a_asp) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const double px = x[i], py = y[i];
        double row, col;
        pts_row_col(q, px, py, row, col);
        float v;
        const bool ok = d_finite(px) && d_finite(py) && t_finite(z[i]) && bi_point<float>(g, plane, row, col, v);
        pvalid[i] = ok ? 1 : 0;
        if (st_plane) {
            T s, a;
            bi_point<T>(g, st_plane, row, col, s);
            bi_point<T>(g, asp_plane, row, col, a);
            a_st[i] = s;
            a_asp[i] = a;
        }
    }
}

// the selected points' columns in cloud order
template <typename T>
__global__ __launch_bounds__(256) void pts_gather_kernel(const int64_t* __restrict__ idx, int64_t m, const double* __restrict__ x,
                                                         const double* __restrict__ y, const T* __restrict__ z, const T* __restrict__ a_st,
                                                         const T* __restrict__ a_asp, double* __restrict__ sx, double* __restrict__ sy,
                                                         T* __restrict__ sz, T* __restrict__ sst, T* __restrict__ sasp) {
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < m; k += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = idx[k];
        sx[k] = x[i];
        sy[k] = y[i];
        sz[k] = z[i];
        if (a_st) { sst[k] = a_st[i]; sasp[k] = a_asp[i]; }
    }
}

// counting sort of the selection by raster tile of the unshifted position: histogram, (rank_scan_kernel), scatter.  The order inside
// a tile is whatever the atomics give; the gather writes dh[original index], so no result depends on it.
__device__ __forceinline__ int64_t pts_tile_of(const PtsGeo& q, double x, double y, int64_t H, int64_t W, int64_t tw) {
    double row, col;
    pts_row_col(q, x, y, row, col);
    int64_t r = (row >= 0.0) ? (row < (double)H ? (int64_t)row : H - 1) : 0;   // (NaN: 0)
    int64_t c = (col >= 0.0) ? (col < (double)W ? (int64_t)col : W - 1) : 0;
    return (r >> PTS_TILE_LOG2) * tw + (c >> PTS_TILE_LOG2);
}
__global__ __launch_bounds__(256) void pts_tile_count_kernel(PtsGeo q, const double* __restrict__ sx, const double* __restrict__ sy, int64_t m,
                                                             int64_t H, int64_t W, int64_t tw, uint32_t* __restrict__ tile,
                                                             unsigned long long* __restrict__ cnt) {
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < m; k += (int64_t)gridDim.x * blockDim.x) {
        const int64_t t = pts_tile_of(q, sx[k], sy[k], H, W, tw);
        tile[k] = (uint32_t)t;
        atomicAdd(&cnt[t], 1ull);
    }
}
__global__ __launch_bounds__(256) void pts_tile_scatter_kernel(const uint32_t* __restrict__ tile, int64_t m, unsigned long long* __restrict__ cursor,
                                                               int64_t* __restrict__ order) {
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < m; k += (int64_t)gridDim.x * blockDim.x) {
        const unsigned long long pos = atomicAdd(&cursor[tile[k]], 1ull);
        if ((int64_t)pos < m) order[pos] = k;
    }
}

// ---- one evaluation ---------------------------------------------------------------------------------------------------------------
// dh of every selected point at the shifted position, written at the point's own index whatever order the points are walked in; with
// `asp`, min / max aspect over the points that still have a dh (SciPy's automatic edges); with HIST, the leading digit's counts.
template <typename T, bool HIST>
__global__ __launch_bounds__(256) void pts_dh_kernel(const T* __restrict__ raster, NkGeom g, PtsGeo q, const double* __restrict__ sx,
                                                     const double* __restrict__ sy, const T* __restrict__ sz, const T* __restrict__ asp,
                                                     const int64_t* __restrict__ order, int64_t m, int pts_is_ref, T* __restrict__ dh,
                                                     DhStats* stats, uint64_t* __restrict__ hist) {
    typedef typename KeyT<T>::type K;
    __shared__ uint32_t h[HIST ? DH_HIST_COPIES * DH_HIST_STRIDE : 1];
    if (HIST) {
        for (int k = threadIdx.x; k < DH_HIST_COPIES * DH_HIST_STRIDE; k += blockDim.x) h[k] = 0;
        __syncthreads();
    }
    uint32_t* hc = h + (HIST ? (threadIdx.x % DH_HIST_COPIES) * DH_HIST_STRIDE : 0);
    K kmin = ~(K)0, kmax = 0;
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < m; k += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = order ? order[k] : k;
        double row, col;
        pts_row_col(q, sx[i], sy[i], row, col);
        T val;
        const bool ok = bi_point<T>(g, raster, row, col, val);
        const T zv = sz[i];
        T out = pts_is_ref ? t_sub(zv, val) : t_sub(val, zv);
        if (ok && t_finite(out)) {
            if (asp) {
                const K ka = key_of(asp[i]);
                kmin = ka < kmin ? ka : kmin;
                kmax = ka > kmax ? ka : kmax;
            }
        } else {
            out = (T)NAN;
        }
        dh[i] = out;
        if (HIST) dh_hist_count<T>(hc, out);
    }
    if (asp) {
        for (int off = 32; off > 0; off >>= 1) {
            const K a = k_shfl_down(kmin, off), b = k_shfl_down(kmax, off);
            kmin = a < kmin ? a : kmin;
            kmax = b > kmax ? b : kmax;
        }
        if ((threadIdx.x & 63) == 0) {
            if (kmin != ~(K)0) k_atomic_min(&stats->asp_min, (uint64_t)kmin);
            if (kmax != 0) k_atomic_max(&stats->asp_max, (uint64_t)kmax);
        }
    }
    if (HIST) dh_hist_flush(h, hist);
}

static __global__ void pts_stats_init_kernel(DhStats* s) {
    if (threadIdx.x == 0) { s->asp_min = ~(uint64_t)0; s->asp_max = 0; }
}

// the bin edges of a step: SciPy's automatic ones from min / max aspect, or the caller's
template <typename T>
__global__ void pts_edges_kernel(const DhStats* stats, const T* __restrict__ custom, int nb, T* __restrict__ edges) {
    typedef typename KeyT<T>::type K;
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    if (custom) {
        for (int k = 0; k <= nb; ++k) edges[k] = custom[k];
        return;
    }
    if (stats->asp_min == ~(uint64_t)0) {   // no point has a dh: the step fails on its count
        for (int k = 0; k <= nb; ++k) edges[k] = (T)k;
        return;
    }
    make_edges_into<T>((double)val_of((K)stats->asp_min), (double)val_of((K)stats->asp_max), nb, edges);
}

// y = (dh - vshift) / slope_tan and its aspect bin for every selected point (cloud order); sum y, sum y^2 and the count as one partial
// per workgroup (fixed_sums.h)
template <typename T>
__global__ __launch_bounds__(256) void pts_y_kernel(const T* __restrict__ dh, const T* __restrict__ slope_tan, const T* __restrict__ aspect,
                                                    int64_t m, const T* __restrict__ vshift_p, const T* __restrict__ edges, int nb,
                                                    T* __restrict__ y, uint16_t* __restrict__ bins, double* __restrict__ part, int last_decimal) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ double red[4];
    T* e = reinterpret_cast<T*>(smem);
    for (int k = threadIdx.x; k <= nb; k += blockDim.x) e[k] = edges[k];
    __syncthreads();
    const T vshift = *vshift_p;
    const double inv_width = (double)nb / ((double)e[nb] - (double)e[0]);
    double s[2] = {0.0, 0.0}, cnt = 0.0;
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < m; p += (int64_t)gridDim.x * blockDim.x) {
        const T d = dh[p];
        T yv = (T)NAN;
        uint16_t b = 0xFFFF;
        if (d == d) {
            yv = t_div(t_sub(d, vshift), slope_tan[p]);
            b = aspect_bin<T>(aspect[p], e, nb, inv_width, last_decimal);
            s[0] += (double)yv;
            s[1] += (double)yv * (double)yv;
            cnt += 1.0;
        }
        y[p] = yv;
        bins[p] = b;
    }
    block_sums_store<2>(s, cnt, red, part);
}

__global__ __launch_bounds__(256) void pts_apply_matrix_kernel(Mat12 M, int has_c, double cx, double cy, double cz, const double* __restrict__ x,
                                                               const double* __restrict__ y, const double* __restrict__ z, int64_t n,
                                                               double* __restrict__ xo, double* __restrict__ yo, double* __restrict__ zo) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        double px = x[i], py = y[i], pz = z[i];
        if (has_c) { px = px - cx; py = py - cy; pz = pz - cz; }
        double ox, oy, oz;
        mat12_apply(M.m, px, py, pz, ox, oy, oz);
        if (has_c) { ox = ox + cx; oy = oy + cy; oz = oz + cz; }
        xo[i] = ox; yo[i] = oy; zo[i] = oz;
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------
inline size_t es_of(const xdemhip_pts_plan* P) { return P->dtype == XDEMHIP_F32 ? 4 : 8; }
// scratch: T edges[PTS_MAX_BINS + 1] at 0 | DhStats at OFF_STATS | selection scratch from OFF_STATE | DhEvalOut behind scratch_size(PTS_MAX_BINS)
inline size_t pts_scratch_bytes() { return scratch_size(PTS_MAX_BINS) + sizeof(DhEvalOut) + 64; }

NkGeom pts_geom(const xdemhip_pts_plan* P) {
    NkGeom g;
    g.H = P->H; g.W = P->W; g.roff = 0; g.dr = 0.0; g.dc = 0.0; g.rule = P->nan_rule;
    return g;
}
PtsGeo pts_geo(const xdemhip_pts_plan* P, double shift_x, double shift_y) {
    PtsGeo q;
    q.a = P->t6[0]; q.c = P->t6[2]; q.e = P->t6[4]; q.f = P->t6[5];
    q.sx = P->pts_is_ref ? shift_x : -shift_x;
    q.sy = P->pts_is_ref ? shift_y : -shift_y;
    return q;
}

void free_selection(xdemhip_pts_plan* P) {
    const void* b[] = {P->idx, P->sx, P->sy, P->sz, P->sst, P->sasp, P->order};
    for (const void* p : b) P->mem.drop(p);
    P->idx = nullptr; P->sx = P->sy = nullptr; P->sz = P->sst = P->sasp = nullptr; P->order = nullptr;
    P->m = 0;
    P->y_n = -1;
}

// The selection's columns from its list of cloud indexes (P->idx, P->m set by the caller), and its tile order if the switch asks.
template <typename T> int build_selection(xdemhip_pts_plan* P) {
    xdemhip_ctx* ctx = P->ctx;
    const int64_t m = P->m;
    P->sx = P->mem.take<double>((size_t)m, "selected points");
    P->sy = P->mem.take<double>((size_t)m, "selected points");
    P->sz = P->mem.take<T>((size_t)m, "selected points");
    if (P->with_aux) {
        P->sst = P->mem.take<T>((size_t)m, "selected points");
        P->sasp = P->mem.take<T>((size_t)m, "selected points");
    }
    { const int rc = P->mem.status(); if (rc) return rc; }
    if (m == 0) return XDEMHIP_OK;
    hipLaunchKernelGGL((pts_gather_kernel<T>), dim3(grid_for(ctx, m, 256, 16)), dim3(256), 0, ctx->stream, P->idx, m, P->x, P->y,
                       static_cast<const T*>(P->z), static_cast<const T*>(P->a_st), static_cast<const T*>(P->a_asp), P->sx, P->sy,
                       static_cast<T*>(P->sz), static_cast<T*>(P->sst), static_cast<T*>(P->sasp));
    if (launched(ctx, "pts_gather_kernel")) return XDEMHIP_EHIP;
    if (ctx->pts_tile_order == 0) return XDEMHIP_OK;
    const int64_t tw = (P->W + (1 << PTS_TILE_LOG2) - 1) >> PTS_TILE_LOG2, th = (P->H + (1 << PTS_TILE_LOG2) - 1) >> PTS_TILE_LOG2;
    const int64_t nt = tw * th;
    if (nt > 0xFFFFFFFFll) return XDEMHIP_OK;   // (tile ids are 32-bit: such a raster keeps the cloud order)
    XdBuffers buf(ctx, "raster-point plan: tile order");
    uint32_t* tile = buf.alloc<uint32_t>((size_t)m);
    unsigned long long* cnt = buf.alloc<unsigned long long>((size_t)nt + 2);
    if (buf.rc) return buf.rc;
    P->order = P->mem.take<int64_t>((size_t)m, "tile order");
    { const int rc = P->mem.status(); if (rc) return rc; }
    XD_HIP_CHECK(ctx, hipMemsetAsync(cnt, 0, (size_t)(nt + 2) * 8, ctx->stream));
    const PtsGeo q = pts_geo(P, 0.0, 0.0);
    const dim3 grid(grid_for(ctx, m, 256, 16));
    hipLaunchKernelGGL(pts_tile_count_kernel, grid, dim3(256), 0, ctx->stream, q, P->sx, P->sy, m, P->H, P->W, tw, tile, cnt);
    hipLaunchKernelGGL(rank_scan_kernel, dim3(1), dim3(1024), 0, ctx->stream, cnt, nt, cnt + nt);
    hipLaunchKernelGGL(pts_tile_scatter_kernel, grid, dim3(256), 0, ctx->stream, tile, m, cnt, P->order);
    if (launched(ctx, "tile order kernels")) return XDEMHIP_EHIP;
    return XDEMHIP_OK;   // (the scope waits for the stream before it frees its buffers)
}

int ensure_step(xdemhip_pts_plan* P, bool with_y) {
    xdemhip_ctx* ctx = P->ctx;
    const size_t es = es_of(P);
    const size_t mm = (size_t)P->m;
    XdOwned& mem = P->mem;
    if (!P->scratch) P->scratch = mem.take<unsigned char>(pts_scratch_bytes(), "raster-point plan: selection scratch");
    if (P->step_n != P->m) {
        mem.drop(P->yv);
        mem.drop(P->bins);
        P->yv = nullptr; P->bins = nullptr;
        P->y_n = -1;
        P->step_n = mem.regrow(P->dh, mm * es, "raster-point plan: dh column") ? P->m : -1;
    }
    { const int rc = mem.status(); if (rc) return rc; }
    if (with_y && !P->yv) {   // (both or neither: a later step asks again)
        mem.optional();
        P->yv = mem.take(mm * es, "raster-point plan: y column");
        P->bins = mem.take<uint16_t>(mm, "raster-point plan: y column");
        if (!mem.all_or_none(P->yv, P->bins)) return xd_fail(ctx, XDEMHIP_ENOMEM, "hipMalloc failed (raster-point plan: y column)");
    }
    if (P->ws_n != P->m) {
        sel_ws_free(mem, P->ws);
        if (P->m >= SEL_BRACKET_MIN_N) (void)sel_ws_create(mem, P->m, es, MAX_BINS_PER_SWEEP, P->ws);   // (on failure: plain selection)
        P->ws_n = P->m;
    }
    return XDEMHIP_OK;
}

template <typename T>
int launch_dh(xdemhip_pts_plan* P, const PtsGeo& q, bool with_asp, DhStats* stats, bool with_hist, uint64_t* hist) {
    xdemhip_ctx* ctx = P->ctx;
    const dim3 grid(grid_for(ctx, P->m, 256, 16)), b(256);
    const T* asp = with_asp ? static_cast<const T*>(P->sasp) : (const T*)nullptr;
    if (with_hist)
        hipLaunchKernelGGL((pts_dh_kernel<T, true>), grid, b, 0, ctx->stream, static_cast<const T*>(P->raster), pts_geom(P), q, P->sx, P->sy,
                           static_cast<const T*>(P->sz), asp, P->order, P->m, (int)P->pts_is_ref, static_cast<T*>(P->dh), stats, hist);
    else
        hipLaunchKernelGGL((pts_dh_kernel<T, false>), grid, b, 0, ctx->stream, static_cast<const T*>(P->raster), pts_geom(P), q, P->sx, P->sy,
                           static_cast<const T*>(P->sz), asp, P->order, P->m, (int)P->pts_is_ref, static_cast<T*>(P->dh), stats, hist);
    return launched(ctx, "pts_dh_kernel");
}

// One Nuth-Kaab step over the selected points: the gather with the median's selection, vshift and the edges decoded on the device,
// y and its bins, the fixed-order sums, the per-bin selection -- whose own synchronisation delivers every result (one fetch).  A missed
// bracket of the first selection (clouds of SEL_BRACKET_MIN_N points and more only) runs the step again with the plain digit passes.
template <typename T>
int nk_step_typed(xdemhip_pts_plan* P, double shift_x, double shift_y, int nb, double* vshift, int64_t* n_valid, double* y_mean, double* y_std,
                  double* edges_out, int64_t* counts, double* medians) {
    typedef typename KeyT<T>::type K;
    xdemhip_ctx* ctx = P->ctx;
    int rc = ensure_step(P, true);
    if (rc) return rc;
    rc = P->sums.reserve(P->mem, 3, "xdemhip_pts_nk_step");
    if (rc) return rc;
    const int64_t m = P->m;
    unsigned char* base = P->scratch;
    T* d_edges = reinterpret_cast<T*>(base);
    DhStats* d_stats = reinterpret_cast<DhStats*>(base + OFF_STATS);
    DhEvalOut* d_out = reinterpret_cast<DhEvalOut*>(base + scratch_size(PTS_MAX_BINS));
    const PtsGeo q = pts_geo(P, shift_x, shift_y);
    const int decimal = P->d_custom ? P->custom_decimal : NK_AUTO_EDGES;
    const int nblocks = fixed_sums_grid(ctx, (m + 255) / 256);
    double* d_tot = P->sums.part + (int64_t)nblocks * 3;
    std::vector<SelResult<K>> hs;
    std::vector<T> edges(nb + 1);
    DhEvalOut h;
    double tot[3] = {0.0, 0.0, 0.0};
    for (int attempt = 0; attempt < 2; ++attempt) {
        const bool plain = attempt == 1 || m < SEL_BRACKET_MIN_N;
        hipLaunchKernelGGL(pts_stats_init_kernel, dim3(1), dim3(64), 0, ctx->stream, d_stats);
        rc = dh_median_enqueue<T>(ctx, static_cast<T*>(P->dh), m, base, &P->ws, plain,
                                  [&](bool with_hist, uint64_t* hist) { return launch_dh<T>(P, q, true, d_stats, with_hist, hist); }, d_out);
        if (rc) return rc;
        hipLaunchKernelGGL((pts_edges_kernel<T>), dim3(1), dim3(64), 0, ctx->stream, d_stats, static_cast<const T*>(P->d_custom), nb, d_edges);
        hipLaunchKernelGGL((pts_y_kernel<T>), dim3(nblocks), dim3(256), sizeof(T) * (nb + 1), ctx->stream, static_cast<const T*>(P->dh),
                           static_cast<const T*>(P->sst), static_cast<const T*>(P->sasp), m, reinterpret_cast<const T*>(&d_out->slot), d_edges, nb,
                           static_cast<T*>(P->yv), P->bins, P->sums.part, decimal);
        if (launched(ctx, "raster-point step kernels")) return XDEMHIP_EHIP;
        rc = fixed_sums_reduce(ctx, P->sums.part, nblocks, 3, "raster-point step sums");
        if (rc == XDEMHIP_OK) rc = xd_d2h(ctx, &h, d_out, sizeof h);
        if (rc == XDEMHIP_OK) rc = xd_d2h(ctx, edges.data(), d_edges, sizeof(T) * (nb + 1));
        if (rc == XDEMHIP_OK) rc = xd_d2h(ctx, tot, d_tot, 24);
        // (the selection's own synchronisation delivers the three blocks above)
        if (rc == XDEMHIP_OK) rc = plain ? run_select_core<T>(ctx, static_cast<const T*>(P->yv), P->bins, m, nb, base, hs, SEL_MEDIAN, nullptr)
                                         : run_select<T>(ctx, static_cast<const T*>(P->yv), P->bins, m, nb, base, hs, &P->ws);
        if (rc) return rc;
        if (!h.fail) break;
    }
    *n_valid = (int64_t)h.count;
    if (h.count == 0) return xd_fail(ctx, XDEMHIP_EINVAL, "The subsample contains no more valid values.");
    P->y_n = m;
    *vshift = h.median;
    const double cnt = tot[2];
    const double mean = tot[0] / cnt;
    const double var = tot[1] / cnt - mean * mean;
    *y_mean = mean;
    *y_std = var > 0 ? sqrt(var) : 0.0;
    for (int k = 0; k < nb; ++k) {
        counts[k] = (int64_t)hs[k].st.count;
        medians[k] = median_from<T>(hs[k]);
    }
    for (int k = 0; k <= nb; ++k) edges_out[k] = (double)edges[k];
    return XDEMHIP_OK;
}

template <typename T>
int create_typed(xdemhip_pts_plan* P, const uint8_t* inlier_host_or_dev, int memspace) {
    xdemhip_ctx* ctx = P->ctx;
    const int64_t n = P->H * P->W;
    XdBuffers buf(ctx, "xdemhip_pts_create");
    const uint8_t* d_inl = buf.input(inlier_host_or_dev, (size_t)n, memspace);
    float* plane = buf.alloc<float>((size_t)n);
    T* st_plane = nullptr;
    T* asp_plane = nullptr;
    uint8_t* valid = nullptr;
    if (P->with_aux) {
        st_plane = buf.alloc<T>((size_t)n);
        asp_plane = buf.alloc<T>((size_t)n);
        valid = buf.alloc<uint8_t>((size_t)n);
    }
    unsigned long long* d_cnt = buf.alloc<unsigned long long>(1);
    if (buf.rc) return buf.rc;
    const T* raster = static_cast<const T*>(P->raster);
    if (P->with_aux) {
        // slope tangent, aspect and the valid mask as xdemhip_nk_create builds them (the raster in both places: finite(raster) once)
        const int64_t gx = (P->W + 255) / 256;
        int64_t gy = ((int64_t)ctx->num_cu * 16 + gx - 1) / gx;
        gy = gy < 1 ? 1 : (gy > P->H ? P->H : gy);
        XD_HIP_CHECK(ctx, hipMemsetAsync(d_cnt, 0, 8, ctx->stream));
        hipLaunchKernelGGL((nk_aux_kernel<T>), dim3((unsigned)gx, (unsigned)gy), dim3(256), 0, ctx->stream, raster, raster, d_inl, pts_geom(P),
                           st_plane, asp_plane, valid, d_cnt, (int64_t)0, P->H);
    }
    hipLaunchKernelGGL((pts_valid_plane_kernel<T>), dim3(grid_for(ctx, n, 256, 16)), dim3(256), 0, ctx->stream, raster, d_inl, valid, n, plane);
    hipLaunchKernelGGL((pts_valid_kernel<T>), dim3(grid_for(ctx, P->n_pts, 256, 16)), dim3(256), 0, ctx->stream, plane, pts_geom(P),
                       pts_geo(P, 0.0, 0.0), P->x, P->y, static_cast<const T*>(P->z), P->n_pts, st_plane, asp_plane, P->pvalid,
                       static_cast<T*>(P->a_st), static_cast<T*>(P->a_asp));
    // the valid points counted per tile of RANK_TILE points and scanned: ranks in cloud order (rank_select.h)
    hipLaunchKernelGGL((rank_select_kernel<RankOut::Count>), dim3((unsigned)P->n_tiles), dim3(256), 0, ctx->stream, P->pvalid, P->n_pts,
                       (const unsigned long long*)nullptr, (const uint8_t*)nullptr, P->tile_off, (int64_t*)nullptr, (uint8_t*)nullptr);
    hipLaunchKernelGGL(rank_scan_kernel, dim3(1), dim3(1024), 0, ctx->stream, P->tile_off, P->n_tiles, P->tile_off + P->n_tiles);
    if (launched(ctx, "xdemhip_pts_create: kernel")) return XDEMHIP_EHIP;
    unsigned long long total = 0;
    { const int rc_ = xd_d2h(ctx, &total, P->tile_off + P->n_tiles, 8); if (rc_) return rc_; }
    { const int rc_ = xd_sync(ctx); if (rc_) return rc_; }
    P->n_valid = (int64_t)total;
    // the selection: every valid point
    P->m = P->n_valid;
    P->idx = P->mem.take<int64_t>((size_t)P->m, "valid point list");
    if (P->mem.rc) return P->mem.rc;
    hipLaunchKernelGGL((rank_select_kernel<RankOut::List>), dim3((unsigned)P->n_tiles), dim3(256), 0, ctx->stream, P->pvalid, P->n_pts,
                       (const unsigned long long*)nullptr, (const uint8_t*)nullptr, P->tile_off, P->idx, (uint8_t*)nullptr);
    if (launched(ctx, "xdemhip_pts_create: list kernel")) return XDEMHIP_EHIP;
    return build_selection<T>(P);
}

}  // namespace
}  // namespace xd

using namespace xd;

extern "C" {

void xdemhip_pts_destroy(xdemhip_pts_plan* P) { delete P; }   // (its owner frees the device buffers)

int xdemhip_pts_create(xdemhip_ctx* ctx, const void* raster, const uint8_t* inlier, int dtype, int64_t H, int64_t W, const double* transform6,
                       const double* x, const double* y, const void* z, int64_t n_pts, int pts_is_ref, int with_nk_aux, int memspace,
                       xdemhip_pts_plan** out_plan, int64_t* n_valid) {
    XdFetchScope fetch_scope_(ctx);
    if (!ctx) return XDEMHIP_EINVAL;
    if (!raster || !x || !y || !z || !out_plan) return xd_fail(ctx, XDEMHIP_EINVAL, "null argument");
    if (H < 1 || W < 1 || n_pts < 1) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_pts_create: empty raster or cloud");
    if (with_nk_aux && (H < 2 || W < 2)) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_pts_create: the raster must be at least 2 x 2 pixels for the gradient");
    if (dtype != XDEMHIP_F32 && dtype != XDEMHIP_F64) return xd_fail(ctx, XDEMHIP_EINVAL, "dtype must be float32 or float64");
    if (memspace != XDEMHIP_HOST && memspace != XDEMHIP_DEVICE) return xd_fail(ctx, XDEMHIP_EINVAL, "bad memspace");
    { const int rc_ = check_transform(ctx, transform6, "xdemhip_pts_create"); if (rc_) return rc_; }
    XD_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    const size_t es = dtype == XDEMHIP_F32 ? 4 : 8;
    xdemhip_pts_plan* P = new xdemhip_pts_plan();
    P->ctx = P->mem.ctx = ctx; P->dtype = dtype; P->H = H; P->W = W; P->n_pts = n_pts;
    memcpy(P->t6, transform6, sizeof P->t6);
    P->pts_is_ref = pts_is_ref != 0;
    P->with_aux = with_nk_aux != 0;
    P->nan_rule = ctx->nk_nan_rule;
    P->n_tiles = (n_pts + RANK_TILE - 1) / RANK_TILE;
    auto fail = [&](int code) { delete P; return code; };
    if (P->n_tiles > 0x7FFFFFFF) return fail(xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_pts_create: cloud too large"));
    XdOwned& mem = P->mem;
    P->raster = mem.keep(raster, (size_t)(H * W) * es, memspace, "xdemhip_pts_create");
    P->x = mem.keep(x, (size_t)n_pts * 8, memspace, "xdemhip_pts_create");
    P->y = mem.keep(y, (size_t)n_pts * 8, memspace, "xdemhip_pts_create");
    P->z = mem.keep(z, (size_t)n_pts * es, memspace, "xdemhip_pts_create");
    P->pvalid = mem.take<uint8_t>((size_t)P->n_tiles * RANK_TILE, "xdemhip_pts_create");
    P->tile_off = mem.take<unsigned long long>((size_t)P->n_tiles + 1, "xdemhip_pts_create");
    if (P->with_aux) {
        P->a_st = mem.take((size_t)n_pts * es, "xdemhip_pts_create");
        P->a_asp = mem.take((size_t)n_pts * es, "xdemhip_pts_create");
    }
    if (mem.rc) return fail(mem.rc);
    int rc = dtype == XDEMHIP_F32 ? create_typed<float>(P, inlier, memspace) : create_typed<double>(P, inlier, memspace);
    if (rc == XDEMHIP_OK) rc = xd_sync(ctx);
    if (rc) return fail(rc);
    if (n_valid) *n_valid = P->n_valid;
    *out_plan = P;
    return XDEMHIP_OK;
}

int xdemhip_pts_subsample(xdemhip_pts_plan* P, const int64_t* ranks, int64_t k, int memspace, int64_t* n_selected) {
    XdFetchScope fetch_scope_(P ? P->ctx : nullptr);
    if (!P) return XDEMHIP_EINVAL;
    xdemhip_ctx* ctx = P->ctx;
    if (!ranks || k < 1 || k > P->n_valid) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_pts_subsample: 1 <= k <= the plan's valid points");
    if (memspace != XDEMHIP_HOST && memspace != XDEMHIP_DEVICE) return xd_fail(ctx, XDEMHIP_EINVAL, "bad memspace");
    XD_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    RankSelect rs(ctx, "xdemhip_pts_subsample");
    unsigned long long total = 0, bad = 0;
    { const int rc_ = rs.run(ranks, k, memspace, P->n_valid, P->pvalid, P->n_pts, P->tile_off, &total, &bad); if (rc_) return rc_; }
    if (bad != 0) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_pts_subsample: a rank is outside [0, n_valid)");
    if ((int64_t)total > k) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_pts_subsample: more points than ranks");
    int64_t* idx = P->mem.take<int64_t>((size_t)k, "xdemhip_pts_subsample");
    { const int rc_ = P->mem.status(); if (rc_) return rc_; }
    hipLaunchKernelGGL((rank_select_kernel<RankOut::List>), dim3((unsigned)P->n_tiles), dim3(256), 0, ctx->stream, P->pvalid, P->n_pts, P->tile_off,
                       rs.mark, rs.off, idx, (uint8_t*)nullptr);
    int rc = launched(ctx, "xdemhip_pts_subsample: kernel");
    if (rc == XDEMHIP_OK) rc = xd_sync(ctx);
    if (rc) { P->mem.drop(idx); return rc; }
    free_selection(P);
    P->idx = idx;
    P->m = (int64_t)total;
    rc = P->dtype == XDEMHIP_F32 ? build_selection<float>(P) : build_selection<double>(P);
    if (rc == XDEMHIP_OK) rc = xd_sync(ctx);
    if (rc) return rc;
    if (n_selected) *n_selected = P->m;
    return XDEMHIP_OK;
}

int xdemhip_pts_selection(xdemhip_pts_plan* P, int64_t* idx_out, int64_t* count) {
    XdFetchScope fetch_scope_(P ? P->ctx : nullptr);
    if (!P) return XDEMHIP_EINVAL;
    xdemhip_ctx* ctx = P->ctx;
    if (!count) return xd_fail(ctx, XDEMHIP_EINVAL, "null argument");
    *count = P->m;
    if (!idx_out || P->m == 0) return XDEMHIP_OK;
    XD_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    XD_HIP_CHECK(ctx, hipMemcpyAsync(idx_out, P->idx, (size_t)P->m * 8, hipMemcpyDeviceToHost, ctx->stream));
    return xd_sync(ctx);
}

int xdemhip_pts_set_bin_edges(xdemhip_pts_plan* P, const double* edges, int n_edges, int decimal) {
    if (!P) return XDEMHIP_EINVAL;
    xdemhip_ctx* ctx = P->ctx;
    XD_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    P->mem.drop(P->d_custom);
    P->d_custom = nullptr; P->n_custom = 0;
    if (!edges) return XDEMHIP_OK;
    if (n_edges < 2 || n_edges > PTS_MAX_BINS + 1) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_pts_set_bin_edges: 2 to 1025 edges");
    for (int k = 1; k < n_edges; ++k)
        if (!(edges[k] > edges[k - 1])) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_pts_set_bin_edges: edges must increase");
    const size_t es = es_of(P);
    std::vector<unsigned char> h((size_t)n_edges * es);
    for (int k = 0; k < n_edges; ++k) {
        if (P->dtype == XDEMHIP_F32) reinterpret_cast<float*>(h.data())[k] = (float)edges[k];
        else reinterpret_cast<double*>(h.data())[k] = edges[k];
    }
    P->d_custom = P->mem.take(h.size(), "xdemhip_pts_set_bin_edges");
    { const int rc = P->mem.status(); if (rc) return rc; }
    XD_HIP_CHECK(ctx, hipMemcpyAsync(P->d_custom, h.data(), h.size(), hipMemcpyHostToDevice, ctx->stream));
    XD_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    P->n_custom = n_edges - 1;
    P->custom_decimal = decimal;
    return XDEMHIP_OK;
}

int xdemhip_pts_nk_step(xdemhip_pts_plan* P, double shift_x, double shift_y, int n_bins, double* vshift, int64_t* n_valid, double* y_mean,
                        double* y_std, double* edges, int64_t* counts, double* medians) {
    XdFetchScope fetch_scope_(P ? P->ctx : nullptr);
    if (!P) return XDEMHIP_EINVAL;
    xdemhip_ctx* ctx = P->ctx;
    if (!vshift || !n_valid || !y_mean || !y_std || !edges || !counts || !medians) return xd_fail(ctx, XDEMHIP_EINVAL, "null argument");
    if (!P->with_aux) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_pts_nk_step: the plan was created without slope tangent and aspect");
    if (!isfinite(shift_x) || !isfinite(shift_y)) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_pts_nk_step: finite shifts");
    const int nb = P->d_custom ? P->n_custom : n_bins;
    if (nb < 1 || nb > PTS_MAX_BINS) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_pts_nk_step: 1 to 1024 bins");
    *n_valid = 0;
    if (P->m == 0) return xd_fail(ctx, XDEMHIP_EINVAL, "The subsample contains no more valid values.");
    XD_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    XdLocalSelection local(ctx);   // (one process's points)
    return P->dtype == XDEMHIP_F32 ? nk_step_typed<float>(P, shift_x, shift_y, nb, vshift, n_valid, y_mean, y_std, edges, counts, medians)
                                   : nk_step_typed<double>(P, shift_x, shift_y, nb, vshift, n_valid, y_mean, y_std, edges, counts, medians);
}

int xdemhip_pts_step_y(xdemhip_pts_plan* P, void* y_out, int memspace, int64_t* count) {
    XdFetchScope fetch_scope_(P ? P->ctx : nullptr);
    if (!P) return XDEMHIP_EINVAL;
    xdemhip_ctx* ctx = P->ctx;
    if (!y_out || !count) return xd_fail(ctx, XDEMHIP_EINVAL, "null argument");
    if (memspace != XDEMHIP_HOST && memspace != XDEMHIP_DEVICE) return xd_fail(ctx, XDEMHIP_EINVAL, "bad memspace");
    if (!P->yv || P->y_n != P->m || P->m < 1) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_pts_step_y: no step has run on the current selection");
    XD_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    *count = P->m;
    XD_HIP_CHECK(ctx, hipMemcpyAsync(y_out, P->yv, (size_t)P->m * es_of(P), memspace == XDEMHIP_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice,
                                     ctx->stream));
    return xd_sync(ctx);
}

int xdemhip_pts_shift_nmad(xdemhip_pts_plan* P, double shift_x, double shift_y, double nfact, double* median, double* nmad, int64_t* count) {
    XdFetchScope fetch_scope_(P ? P->ctx : nullptr);
    if (!P) return XDEMHIP_EINVAL;
    xdemhip_ctx* ctx = P->ctx;
    if (!median || !nmad || !count) return xd_fail(ctx, XDEMHIP_EINVAL, "null argument");
    if (!isfinite(shift_x) || !isfinite(shift_y)) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_pts_shift_nmad: finite shifts");
    *count = 0;
    if (P->m == 0) return xd_fail(ctx, XDEMHIP_EINVAL, "no valid points");
    XD_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    { const int rc_ = ensure_step(P, false); if (rc_) return rc_; }
    XdLocalSelection local(ctx);
    const PtsGeo q = pts_geo(P, shift_x, shift_y);
    if (P->dtype == XDEMHIP_F32)
        return dh_eval_median_nmad<float>(ctx, static_cast<float*>(P->dh), P->m, P->scratch, &P->ws, nfact,
                                          [&](bool wh, uint64_t* hist) { return launch_dh<float>(P, q, false, nullptr, wh, hist); }, median, nmad, count);
    return dh_eval_median_nmad<double>(ctx, static_cast<double*>(P->dh), P->m, P->scratch, &P->ws, nfact,
                                       [&](bool wh, uint64_t* hist) { return launch_dh<double>(P, q, false, nullptr, wh, hist); }, median, nmad, count);
}

int xdemhip_pts_shift_values(xdemhip_pts_plan* P, double shift_x, double shift_y, void* dh_out, void* slope_out, void* aspect_out, int memspace,
                             int64_t* count) {
    XdFetchScope fetch_scope_(P ? P->ctx : nullptr);
    if (!P) return XDEMHIP_EINVAL;
    xdemhip_ctx* ctx = P->ctx;
    if (!dh_out) return xd_fail(ctx, XDEMHIP_EINVAL, "null argument");
    if (memspace != XDEMHIP_HOST && memspace != XDEMHIP_DEVICE) return xd_fail(ctx, XDEMHIP_EINVAL, "bad memspace");
    if (!isfinite(shift_x) || !isfinite(shift_y)) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_pts_shift_values: finite shifts");
    if ((slope_out || aspect_out) && !P->with_aux) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_pts_shift_values: the plan was created without slope tangent and aspect");
    if (count) *count = P->m;
    if (P->m == 0) return xd_fail(ctx, XDEMHIP_EINVAL, "no valid points");
    XD_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    { const int rc_ = ensure_step(P, false); if (rc_) return rc_; }
    const PtsGeo q = pts_geo(P, shift_x, shift_y);
    int rc = P->dtype == XDEMHIP_F32 ? launch_dh<float>(P, q, false, nullptr, false, nullptr) : launch_dh<double>(P, q, false, nullptr, false, nullptr);
    if (rc) return rc;
    const size_t bytes = (size_t)P->m * es_of(P);
    const hipMemcpyKind kind = memspace == XDEMHIP_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    XD_HIP_CHECK(ctx, hipMemcpyAsync(dh_out, P->dh, bytes, kind, ctx->stream));
    if (slope_out) XD_HIP_CHECK(ctx, hipMemcpyAsync(slope_out, P->sst, bytes, kind, ctx->stream));
    if (aspect_out) XD_HIP_CHECK(ctx, hipMemcpyAsync(aspect_out, P->sasp, bytes, kind, ctx->stream));
    return xd_sync(ctx);
}

int xdemhip_apply_matrix_pts(xdemhip_ctx* ctx, const double* x, const double* y, const double* z, int64_t n, const double* matrix16,
                             const double* centroid3_or_null, int invert, double* x_out, double* y_out, double* z_out, int memspace) {
    XdFetchScope fetch_scope_(ctx);
    if (!ctx) return XDEMHIP_EINVAL;
    if (!x || !y || !z || !matrix16 || !x_out || !y_out || !z_out) return xd_fail(ctx, XDEMHIP_EINVAL, "null argument");
    if (n < 1) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_apply_matrix_pts: empty cloud");
    if (memspace != XDEMHIP_HOST && memspace != XDEMHIP_DEVICE) return xd_fail(ctx, XDEMHIP_EINVAL, "bad memspace");
    XD_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    Mat12 M;
    if (invert) {   // R^T and -(R^T t), the products as explicit sums (as xdemhip_apply_matrix_rst forms its inverse)
        const double* m = matrix16;
        for (int i = 0; i < 3; ++i) {
            for (int j = 0; j < 3; ++j) M.m[4 * i + j] = m[4 * j + i];
            M.m[4 * i + 3] = -((m[0 + i] * m[3] + m[4 + i] * m[7]) + m[8 + i] * m[11]);
        }
    } else {
        memcpy(M.m, matrix16, sizeof M.m);
    }
    const size_t bytes = (size_t)n * 8;
    XdBuffers buf(ctx, "xdemhip_apply_matrix_pts");
    const double* dx = buf.input(x, bytes, memspace);
    const double* dy = buf.input(y, bytes, memspace);
    const double* dz = buf.input(z, bytes, memspace);
    double* ox = buf.output(x_out, bytes, memspace);
    double* oy = buf.output(y_out, bytes, memspace);
    double* oz = buf.output(z_out, bytes, memspace);
    if (buf.rc) return buf.rc;
    const double* c = centroid3_or_null;
    hipLaunchKernelGGL(pts_apply_matrix_kernel, dim3(grid_for(ctx, n, 256, 16)), dim3(256), 0, ctx->stream, M, c ? 1 : 0, c ? c[0] : 0.0, c ? c[1] : 0.0,
                       c ? c[2] : 0.0, dx, dy, dz, n, ox, oy, oz);
    const int rc = launched(ctx, "pts_apply_matrix_kernel");
    return rc == XDEMHIP_OK ? buf.finish() : rc;
}

}  // extern "C"
