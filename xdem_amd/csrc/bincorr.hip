// bincorr.hip -- the raster passes of the bias corrections with variables (include/xdemhip.h, "bias corrections with variables"):
//   xdem.coreg.BiasCorr / DirectionalBias / TerrainBias                              xdem/coreg/biascorr.py:40-618
//     valid = inlier & finite(ref) & finite(tba) & finite(every variable)             base.py:653-661   -> restrict_kernel
//     dh and the variables at the valid (drawn) pixels, handed to nd_binning / a fit  base.py:663-700   -> var_columns_kernel
//     elev + corr(variables), cast to the raster dtype                                biascorr.py:261-311, base.py:491 -> corr_apply_kernel
// Upstream materialises every variable as a whole-raster plane -- also the rotated coordinate of DirectionalBias (float64) and the
// elevation of TerrainBias("elevation") -- then a float64 correction plane, then their sum.  Here a variable is described by its
// source and formed per pixel, the correction never leaves the registers: the float32 DirectionalBias apply reads 4 B and writes
// 4 B per pixel.  The small tables (axes and grid values, left interval ends and bin statistics, model parameters) are staged in LDS;
// the interpolation and the interval search are the code of xdemhip_interp_grid_linear and xdemhip_perbin_lookup
// (grid_interp.h, perbin_locate.h).  No contraction in this file: the Makefile builds it with -ffp-contract=off.
#include <math.h>
#include <string.h>

#include <string>

#include "common.h"
#include "select.h"
#include "select_run.h"
#include "rank_select.h"
#include "dh_plan.h"
#include "grid_interp.h"
#include "perbin_locate.h"

namespace xd {
namespace {

constexpr int BC_MAXVAR = 3;         // variables of the fused apply
constexpr int VC_MAXVAR = 8;         // variables of the column gather (what xdemhip_binstats takes)
constexpr int BC_MAX_TABLE = 3072;   // table entries (bins / grid points) held in LDS: the bin limit of xdemhip_binstats_run
constexpr int BC_MAX_POLY = 64, BC_MAX_SIN = 192;
constexpr int BC_U = 4;              // consecutive pixels per thread and trip: one 16-byte access per float32 plane

struct BcVar {
    int kind, f32;
    const void* plane;
    double c, s, rx, ry, off;
};

// x = (col * res_x) * cos + ((H - 1 - row) * res_y) * sin - offset, every operation rounded on its own (bincorr.rotated_x on the host)
__device__ __forceinline__ double bc_rotated(const BcVar& v, int64_t row, int64_t col, int64_t H) {
    const double xx = (double)col * v.rx;
    const double yy = (double)(H - 1 - row) * v.ry;
    const double a = xx * v.c;
    const double b = yy * v.s;
    return (a + b) - v.off;
}

// ---- valid &= isfinite(var) ----------------------------------------------------------------------------------------------------------
template <typename V>
__global__ __launch_bounds__(256) void restrict_kernel(const V* __restrict__ var, int64_t n, uint8_t* __restrict__ valid) {
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (int64_t)gridDim.x * blockDim.x)
        if (valid[p] && !t_finite<V>(var[p])) valid[p] = 0;
}

// ---- dh and the variables of the selected pixels as columns ------------------------------------------------------------------------------
struct VcArgs {
    BcVar var[VC_MAXVAR];
    void* out[VC_MAXVAR];
    int n_var;
    int64_t H, W, k;
    const int64_t* idx;
};

template <typename T>
__global__ __launch_bounds__(256) void var_columns_kernel(VcArgs A, const T* __restrict__ ref, const T* __restrict__ tba, T* __restrict__ dh) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < A.k; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t q = A.idx[i];
        if (dh) dh[i] = (T)(ref[q] - tba[q]);
#pragma unroll
        for (int v = 0; v < VC_MAXVAR; ++v) {   // (unrolled with a guard: the argument block is indexed statically)
            if (v < A.n_var) {
                const BcVar& s = A.var[v];
                if (s.kind == XDEMHIP_VAR_PLANE) {
                    if (s.f32) static_cast<float*>(A.out[v])[i] = static_cast<const float*>(s.plane)[q];
                    else static_cast<double*>(A.out[v])[i] = static_cast<const double*>(s.plane)[q];
                } else if (s.kind == XDEMHIP_VAR_ROTATED) {
                    const int64_t row = q / A.W;
                    static_cast<double*>(A.out[v])[i] = bc_rotated(s, row, q - row * A.W, A.H);
                } else {
                    static_cast<T*>(A.out[v])[i] = s.kind == XDEMHIP_VAR_REF ? ref[q] : tba[q];
                }
            }
        }
    }
}

// ---- the fused apply ----------------------------------------------------------------------------------------------------------------------
struct BcArgs {
    BcVar var[BC_MAXVAR];
    int n_var, vec, any_rotated;
    int64_t H, W, n;
    GridShape g;            // GRID: the grid; PERBIN: n[] = intervals per variable, off[] = their offsets in a / b
    int n_a, n_b, n_table, n_pass;
    const double *a, *b, *table;
    const unsigned char* pass;
    unsigned long long* missing;
};

template <typename P>
__device__ __forceinline__ void bc_load4(const P* __restrict__ p, int64_t i0, bool whole, int64_t n, double* out);
template <>
__device__ __forceinline__ void bc_load4<float>(const float* __restrict__ p, int64_t i0, bool whole, int64_t n, double* out) {
    if (whole) {
        const float4 t = *reinterpret_cast<const float4*>(p + i0);
        out[0] = (double)t.x; out[1] = (double)t.y; out[2] = (double)t.z; out[3] = (double)t.w;
    } else {
#pragma unroll
        for (int u = 0; u < BC_U; ++u) out[u] = i0 + u < n ? (double)p[i0 + u] : (double)NAN;
    }
}
template <>
__device__ __forceinline__ void bc_load4<double>(const double* __restrict__ p, int64_t i0, bool whole, int64_t n, double* out) {
    if (whole) {
        const double2 t0 = *reinterpret_cast<const double2*>(p + i0);
        const double2 t1 = *reinterpret_cast<const double2*>(p + i0 + 2);
        out[0] = t0.x; out[1] = t0.y; out[2] = t1.x; out[3] = t1.y;
    } else {
#pragma unroll
        for (int u = 0; u < BC_U; ++u) out[u] = i0 + u < n ? p[i0 + u] : (double)NAN;
    }
}

__device__ __forceinline__ void bc_store4(float* __restrict__ p, int64_t i0, bool whole, int64_t n, const double* e, const double* corr) {
    float r[BC_U];
#pragma unroll
    for (int u = 0; u < BC_U; ++u) r[u] = (float)(e[u] + corr[u]);
    if (whole) {
        *reinterpret_cast<float4*>(p + i0) = make_float4(r[0], r[1], r[2], r[3]);
    } else {
#pragma unroll
        for (int u = 0; u < BC_U; ++u)
            if (i0 + u < n) p[i0 + u] = r[u];
    }
}
__device__ __forceinline__ void bc_store4(double* __restrict__ p, int64_t i0, bool whole, int64_t n, const double* e, const double* corr) {
    double r[BC_U];
#pragma unroll
    for (int u = 0; u < BC_U; ++u) r[u] = e[u] + corr[u];
    if (whole) {
        *reinterpret_cast<double2*>(p + i0) = make_double2(r[0], r[1]);
        *reinterpret_cast<double2*>(p + i0 + 2) = make_double2(r[2], r[3]);
    } else {
#pragma unroll
        for (int u = 0; u < BC_U; ++u)
            if (i0 + u < n) p[i0 + u] = r[u];
    }
}

// LDS: [a | table | pass] -- at the table limit 24 + 24 + 3 KiB, under the 64 KiB every workgroup may ask for.  The right ends `b`
// of the per-bin intervals stay in global memory: one read per variable and pixel, of a table the caches hold.
template <int KIND, typename T>
__global__ __launch_bounds__(256) void corr_apply_kernel(BcArgs A, const T* __restrict__ elev, T* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char bc_smem[];
    double* s_a = reinterpret_cast<double*>(bc_smem);
    double* s_table = s_a + A.n_a;
    unsigned char* s_pass = reinterpret_cast<unsigned char*>(s_table + A.n_table);
    for (int e = threadIdx.x; e < A.n_a; e += 256) s_a[e] = A.a[e];
    for (int e = threadIdx.x; e < A.n_table; e += 256) s_table[e] = A.table[e];
    for (int e = threadIdx.x; e < A.n_pass; e += 256) s_pass[e] = A.pass[e];
    __syncthreads();
    auto lo_of = [&](int e) { return s_a[e]; };
    const double* __restrict__ g_b = A.b;
    auto hi_of = [&](int e) { return g_b[e]; };
    const int64_t stride = (int64_t)gridDim.x * blockDim.x * BC_U;
    unsigned long long miss = 0;
    for (int64_t i0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * BC_U; i0 < A.n; i0 += stride) {
        const bool whole = A.vec && i0 + BC_U <= A.n;
        double e[BC_U];
        bc_load4<T>(elev, i0, whole, A.n, e);
        // the pixels' row and column, for the rotated coordinate (one 64-bit division per trip, only where a variable needs it)
        int64_t row[BC_U], col[BC_U];
#pragma unroll
        for (int u = 0; u < BC_U; ++u) { row[u] = 0; col[u] = 0; }
        if (A.any_rotated) {
            row[0] = i0 / A.W;
            col[0] = i0 - row[0] * A.W;
#pragma unroll
            for (int u = 1; u < BC_U; ++u) {
                const bool wrap = col[u - 1] + 1 == A.W;
                col[u] = wrap ? 0 : col[u - 1] + 1;
                row[u] = wrap ? row[u - 1] + 1 : row[u - 1];
            }
        }
        double x[BC_MAXVAR][BC_U];
#pragma unroll
        for (int k = 0; k < BC_MAXVAR; ++k) {
            const BcVar& s = A.var[k];
            if (k < A.n_var && s.kind == XDEMHIP_VAR_PLANE) {
                if (s.f32) bc_load4<float>(static_cast<const float*>(s.plane), i0, whole, A.n, x[k]);
                else bc_load4<double>(static_cast<const double*>(s.plane), i0, whole, A.n, x[k]);
            } else {
                // the rotated coordinate or the raster itself: a select, both are a few operations (beyond n_var: never read)
                const bool rotated = s.kind == XDEMHIP_VAR_ROTATED;
#pragma unroll
                for (int u = 0; u < BC_U; ++u) {
                    const double r = bc_rotated(s, row[u], col[u], A.H);
                    x[k][u] = rotated ? r : e[u];
                }
            }
        }
        double corr[BC_U];
        if (KIND == XDEMHIP_CORR_GRID) {
#pragma unroll
            for (int u = 0; u < BC_U; ++u) {
                bool isnan_any = false;
                const double v = grid_linear_eval<BC_MAXVAR>(A.g, s_a, s_table, [&](int d) { return d == 0 ? x[0][u] : (d == 1 ? x[1][u] : x[2][u]); },
                                                             &isnan_any);
                corr[u] = isnan_any ? (double)NAN : v;
            }
        } else if (KIND == XDEMHIP_CORR_PERBIN) {
            int64_t idx[BC_U];
            bool in[BC_U];
#pragma unroll
            for (int u = 0; u < BC_U; ++u) { idx[u] = 0; in[u] = true; }
#pragma unroll
            for (int k = 0; k < BC_MAXVAR; ++k)
                if (k < A.n_var) pb_locate<BC_U>([&](int u) { return x[k][u]; }, A.g.off[k], A.g.n[k], lo_of, hi_of, in, idx);
#pragma unroll
            for (int u = 0; u < BC_U; ++u) {
                corr[u] = (double)NAN;
                if (in[u] && i0 + u < A.n) {   // (idx < n_table: every position is below its variable's interval count)
                    const unsigned char p = s_pass[idx[u]];
                    if (p == 1) corr[u] = s_table[idx[u]];
                    miss += p == 2;
                }
            }
        } else if (KIND == XDEMHIP_CORR_POLY) {
            // np.polynomial.polynomial.polyval: c0 = c[-1] + x * 0; for i in 2..n: c0 = c[-i] + c0 * x
#pragma unroll
            for (int u = 0; u < BC_U; ++u) {
                double c0 = s_table[A.n_table - 1] + x[0][u] * 0.0;
                for (int i = 2; i <= A.n_table; ++i) c0 = s_table[A.n_table - i] + c0 * x[0][u];
                corr[u] = c0;
            }
        } else {
            // xdem.fit.sumsin_1d: np.sum(a * np.sin(2 pi / b * x + c), axis=0) -- table holds (a, 2 pi / b, c) per term
#pragma unroll
            for (int u = 0; u < BC_U; ++u) {
                double acc = s_table[0] * sin(s_table[1] * x[0][u] + s_table[2]);
                for (int t = 3; t < A.n_table; t += 3) acc = acc + s_table[t] * sin(s_table[t + 1] * x[0][u] + s_table[t + 2]);
                corr[u] = acc;
            }
        }
        bc_store4(out, i0, whole, A.n, e, corr);
    }
    if (KIND == XDEMHIP_CORR_PERBIN && miss) atomicAdd(A.missing, miss);
}

int bc_var_from(xdemhip_ctx* ctx, const xdemhip_varsrc& s, bool plan_sources, const char* who, BcVar* v) {
    memset(v, 0, sizeof *v);
    v->kind = s.kind;
    if (s.kind == XDEMHIP_VAR_PLANE) {
        if (!s.plane) return xd_fail(ctx, XDEMHIP_EINVAL, std::string(who) + ": a plane variable needs its plane");
        if (s.dtype != XDEMHIP_F32 && s.dtype != XDEMHIP_F64) return xd_fail(ctx, XDEMHIP_EINVAL, std::string(who) + ": variables must be float32 or float64");
        v->f32 = s.dtype == XDEMHIP_F32;
    } else if (s.kind == XDEMHIP_VAR_ROTATED) {
        if (!isfinite(s.cos_t) || !isfinite(s.sin_t) || !(s.res_x > 0) || !(s.res_y > 0) || !isfinite(s.offset))
            return xd_fail(ctx, XDEMHIP_EINVAL, std::string(who) + ": the rotated coordinate needs finite cos / sin / offset and positive resolutions");
        v->c = s.cos_t; v->s = s.sin_t; v->rx = s.res_x; v->ry = s.res_y; v->off = s.offset;
    } else if (!(s.kind == XDEMHIP_VAR_REF || (plan_sources && s.kind == XDEMHIP_VAR_TBA))) {
        return xd_fail(ctx, XDEMHIP_EINVAL, std::string(who) + ": unknown variable source");
    }
    return XDEMHIP_OK;
}

}  // namespace
}  // namespace xd

using namespace xd;

extern "C" {

int xdemhip_dh_restrict_finite(xdemhip_dh_plan* P, const void* var, int dtype, int memspace, int64_t* n_valid) {
    XdFetchScope fetch_scope_(P ? P->ctx : nullptr);
    if (!P) return XDEMHIP_EINVAL;
    xdemhip_ctx* ctx = P->ctx;
    if (!var) return xd_fail(ctx, XDEMHIP_EINVAL, "null argument");
    if (dtype != XDEMHIP_F32 && dtype != XDEMHIP_F64) return xd_fail(ctx, XDEMHIP_EINVAL, "dtype must be float32 or float64");
    if (memspace != XDEMHIP_HOST && memspace != XDEMHIP_DEVICE) return xd_fail(ctx, XDEMHIP_EINVAL, "bad memspace");
    if (P->drawn || P->idx)
        return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_dh_restrict_finite: a variable narrows the valid mask and must be given before the draw");
    XD_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    { const int rc_ = dh_ensure_mask(P); if (rc_) return rc_; }
    const int64_t n = P->H * P->W;
    unsigned long long total = 0;   // (the copy's destination: declared first, it outlives the buffers' synchronisation)
    XdBuffers buf(ctx, "xdemhip_dh_restrict_finite");
    const void* d_var = buf.input(var, (size_t)n * (dtype == XDEMHIP_F32 ? 4 : 8), memspace);
    if (buf.rc) return buf.rc;
    const dim3 g(grid_for(ctx, n, 256, 16));
    if (dtype == XDEMHIP_F32) hipLaunchKernelGGL((restrict_kernel<float>), g, dim3(256), 0, ctx->stream, static_cast<const float*>(d_var), n, P->valid);
    else hipLaunchKernelGGL((restrict_kernel<double>), g, dim3(256), 0, ctx->stream, static_cast<const double*>(d_var), n, P->valid);
    // the tiles' counts of the narrowed mask, scanned: the subsample ranks and the pixel list follow the new mask
    hipLaunchKernelGGL((rank_select_kernel<RankOut::Count>), dim3((unsigned)P->n_tiles), dim3(256), 0, ctx->stream, P->valid, n,
                       (const unsigned long long*)nullptr, (const uint8_t*)nullptr, P->tile_off, (int64_t*)nullptr, (uint8_t*)nullptr);
    hipLaunchKernelGGL(rank_scan_kernel, dim3(1), dim3(1024), 0, ctx->stream, P->tile_off, P->n_tiles, P->tile_off + P->n_tiles);
    int rc = launched(ctx, "restrict_kernel");
    if (rc == XDEMHIP_OK) rc = xd_d2h(ctx, &total, P->tile_off + P->n_tiles, 8);
    if (rc == XDEMHIP_OK) rc = xd_sync(ctx);
    if (rc) return rc;
    P->n_valid = (int64_t)total;
    if (n_valid) *n_valid = P->n_valid;
    return buf.finish();
}

int xdemhip_dh_var_columns(xdemhip_dh_plan* P, int n_var, const xdemhip_varsrc* vars, void* dh_out, void* const* var_out, int memspace,
                           int64_t* count) {
    XdFetchScope fetch_scope_(P ? P->ctx : nullptr);
    if (!P) return XDEMHIP_EINVAL;
    xdemhip_ctx* ctx = P->ctx;
    if (n_var < 0 || n_var > VC_MAXVAR) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_dh_var_columns: 0 to 8 variables");
    if (n_var > 0 && (!vars || !var_out)) return xd_fail(ctx, XDEMHIP_EINVAL, "null argument");
    if (memspace != XDEMHIP_HOST && memspace != XDEMHIP_DEVICE) return xd_fail(ctx, XDEMHIP_EINVAL, "bad memspace");
    VcArgs A;
    memset(&A, 0, sizeof A);
    for (int v = 0; v < n_var; ++v) {
        if (!var_out[v]) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_dh_var_columns: every variable needs an output column");
        const int rc_ = bc_var_from(ctx, vars[v], true, "xdemhip_dh_var_columns", &A.var[v]);
        if (rc_) return rc_;
    }
    XD_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    int rc = dh_ensure_valid_idx(P);
    if (rc) return rc;
    const int64_t k = P->n_idx;
    if (count) *count = k;
    if (k == 0) return xd_fail(ctx, XDEMHIP_EINVAL, "no valid points");
    const int64_t n = P->H * P->W;
    const size_t es = P->dtype == XDEMHIP_F32 ? 4 : 8;
    XdBuffers buf(ctx, "xdemhip_dh_var_columns");
    void* d_dh = buf.output(dh_out, (size_t)k * es, memspace);
    for (int v = 0; v < n_var; ++v) {
        const xdemhip_varsrc& s = vars[v];
        size_t col_es = es;
        if (s.kind == XDEMHIP_VAR_PLANE) {
            col_es = s.dtype == XDEMHIP_F32 ? 4 : 8;
            A.var[v].plane = buf.input(s.plane, (size_t)n * col_es, memspace);
        } else if (s.kind == XDEMHIP_VAR_ROTATED) {
            col_es = 8;
        }
        A.out[v] = buf.output(var_out[v], (size_t)k * col_es, memspace);
    }
    if (buf.rc) return buf.rc;
    A.n_var = n_var; A.H = P->H; A.W = P->W; A.k = k; A.idx = P->idx;
    const dim3 g(grid_for(ctx, k, 256, 16));
    if (P->dtype == XDEMHIP_F32)
        hipLaunchKernelGGL((var_columns_kernel<float>), g, dim3(256), 0, ctx->stream, A, static_cast<const float*>(P->ref), static_cast<const float*>(P->tba),
                           static_cast<float*>(d_dh));
    else
        hipLaunchKernelGGL((var_columns_kernel<double>), g, dim3(256), 0, ctx->stream, A, static_cast<const double*>(P->ref),
                           static_cast<const double*>(P->tba), static_cast<double*>(d_dh));
    rc = launched(ctx, "var_columns_kernel");
    if (rc == XDEMHIP_OK) rc = buf.finish();
    // (device columns: complete when the call returns, whichever stream the caller reads them on)
    if (rc == XDEMHIP_OK && memspace == XDEMHIP_DEVICE) rc = xd_sync(ctx);
    return rc;
}

int xdemhip_corr_apply(xdemhip_ctx* ctx, const void* elev, int dtype, int64_t H, int64_t W, int kind, int n_var, const xdemhip_varsrc* vars,
                       const int* n_tab, const double* a, const double* b, const double* table, const unsigned char* pass, void* out,
                       int64_t* n_missing, int memspace) {
    XdFetchScope fetch_scope_(ctx);
    if (!ctx) return XDEMHIP_EINVAL;
    if (!elev || !out || !vars || !n_tab || !table) return xd_fail(ctx, XDEMHIP_EINVAL, "null argument");
    if (H < 1 || W < 1) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_corr_apply: bad raster size");
    if (dtype != XDEMHIP_F32 && dtype != XDEMHIP_F64) return xd_fail(ctx, XDEMHIP_EINVAL, "dtype must be float32 or float64");
    if (memspace != XDEMHIP_HOST && memspace != XDEMHIP_DEVICE) return xd_fail(ctx, XDEMHIP_EINVAL, "bad memspace");
    if (kind < XDEMHIP_CORR_GRID || kind > XDEMHIP_CORR_SUMSIN) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_corr_apply: unknown kind of correction");
    const bool tabled = kind == XDEMHIP_CORR_GRID || kind == XDEMHIP_CORR_PERBIN;
    if (n_var < 1 || n_var > (tabled ? BC_MAXVAR : 1))
        return xd_fail(ctx, XDEMHIP_EINVAL, tabled ? "xdemhip_corr_apply: 1 to 3 variables" : "xdemhip_corr_apply: the 1-D models take one variable");
    if (n_missing) *n_missing = 0;
    BcArgs A;
    memset(&A, 0, sizeof A);
    for (int v = 0; v < n_var; ++v) {
        const int rc_ = bc_var_from(ctx, vars[v], false, "xdemhip_corr_apply", &A.var[v]);
        if (rc_) return rc_;
    }
    int64_t n_entries = 1, n_ends = 0;
    if (tabled) {
        if (!a || (kind == XDEMHIP_CORR_PERBIN && (!b || !pass))) return xd_fail(ctx, XDEMHIP_EINVAL, "null argument");
        A.g.nd = n_var;
        for (int d = 0; d < n_var; ++d) {
            if (n_tab[d] < (kind == XDEMHIP_CORR_GRID ? 2 : 1))
                return xd_fail(ctx, XDEMHIP_EINVAL, kind == XDEMHIP_CORR_GRID ? "every grid axis needs at least 2 points" : "every variable needs at least one interval");
            A.g.n[d] = n_tab[d]; A.g.off[d] = (int)n_ends;
            n_ends += n_tab[d];
            n_entries *= n_tab[d];
            if (n_entries > BC_MAX_TABLE) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_corr_apply: more than 3072 table entries");
        }
        for (int d = n_var - 1, st = 1; d >= 0; --d) { A.g.stride[d] = st; st *= n_tab[d]; }
    } else {
        n_entries = n_tab[0];
        if (kind == XDEMHIP_CORR_POLY && (n_entries < 1 || n_entries > BC_MAX_POLY)) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_corr_apply: 1 to 64 polynomial coefficients");
        if (kind == XDEMHIP_CORR_SUMSIN && (n_entries < 3 || n_entries > BC_MAX_SIN || n_entries % 3 != 0))
            return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_corr_apply: 3 K sinusoid parameters, K = 1..64");
    }
    XD_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    // host copies of the tables, each padded to an even number of doubles (16-byte parts in LDS); sumsin: (a, 2 pi / b, c)
    auto even = [](int64_t c) { return (int)((c + 1) & ~(int64_t)1); };
    A.n_a = tabled ? even(n_ends) : 0;
    A.n_b = kind == XDEMHIP_CORR_PERBIN ? even(n_ends) : 0;
    A.n_table = (int)n_entries;
    A.n_pass = kind == XDEMHIP_CORR_PERBIN ? (int)n_entries : 0;
    const int table_pad = even(n_entries);
    std::vector<double> h((size_t)A.n_a + A.n_b + table_pad, 0.0);
    if (tabled) memcpy(h.data(), a, (size_t)n_ends * 8);
    if (A.n_b) memcpy(h.data() + A.n_a, b, (size_t)n_ends * 8);
    double* h_table = h.data() + A.n_a + A.n_b;
    memcpy(h_table, table, (size_t)n_entries * 8);
    if (kind == XDEMHIP_CORR_SUMSIN)
        for (int t = 1; t < n_entries; t += 3) h_table[t] = (2.0 * 3.141592653589793) / table[t];   // 2 * np.pi / b
    unsigned long long miss = 0;   // (the counter's destination: declared first, it outlives the buffers' synchronisation)
    const int64_t n = H * W;
    const size_t es = dtype == XDEMHIP_F32 ? 4 : 8;
    XdBuffers buf(ctx, "xdemhip_corr_apply");
    const double* d_tabs = buf.input(h.data(), h.size() * 8, XDEMHIP_HOST);
    const unsigned char* d_pass = A.n_pass ? buf.input(pass, (size_t)A.n_pass, XDEMHIP_HOST) : nullptr;
    A.missing = buf.alloc<unsigned long long>(1);
    const void* d_elev = buf.input(elev, (size_t)n * es, memspace);
    void* d_out = buf.output(out, (size_t)n * es, memspace);
    for (int v = 0; v < n_var; ++v)
        if (vars[v].kind == XDEMHIP_VAR_PLANE) A.var[v].plane = buf.input(vars[v].plane, (size_t)n * (vars[v].dtype == XDEMHIP_F32 ? 4 : 8), memspace);
    if (buf.rc) return buf.rc;
    if (hipMemsetAsync(A.missing, 0, 8, ctx->stream) != hipSuccess) return xd_fail(ctx, XDEMHIP_EHIP, "upload failed");
    A.a = d_tabs; A.b = d_tabs + A.n_a; A.table = d_tabs + A.n_a + A.n_b; A.pass = d_pass;
    A.n_table = (int)n_entries;
    A.n_var = n_var; A.H = H; A.W = W; A.n = n;
    A.vec = ((uintptr_t)d_elev & 15) == 0 && ((uintptr_t)d_out & 15) == 0;
    for (int v = 0; v < n_var; ++v) {
        if (A.var[v].kind == XDEMHIP_VAR_PLANE) A.vec = A.vec && ((uintptr_t)A.var[v].plane & 15) == 0;
        if (A.var[v].kind == XDEMHIP_VAR_ROTATED) A.any_rotated = 1;
    }
    // LDS: the parts in the kernel's order; the table part is addressed with n_table, the pass bytes follow it directly
    const size_t smem = ((size_t)(A.n_a + A.n_table) * 8 + (size_t)A.n_pass + 15) & ~(size_t)15;
    const int64_t want = (n + 256 * BC_U - 1) / (256 * BC_U);
    const unsigned blocks = (unsigned)(want < (int64_t)ctx->num_cu * 16 ? want : (int64_t)ctx->num_cu * 16);
    (void)hipEventRecord(ctx->ev_start, ctx->stream);
    int rc = XDEMHIP_OK;
#define XD_BC_GO(K)                                                                                                                                   \
    do {                                                                                                                                              \
        if (dtype == XDEMHIP_F32) {                                                                                                                   \
            rc = set_big_lds(ctx, corr_apply_kernel<K, float>, smem);                                                                                 \
            if (rc == XDEMHIP_OK)                                                                                                                     \
                hipLaunchKernelGGL((corr_apply_kernel<K, float>), dim3(blocks), dim3(256), smem, ctx->stream, A, static_cast<const float*>(d_elev),   \
                                   static_cast<float*>(d_out));                                                                                       \
        } else {                                                                                                                                      \
            rc = set_big_lds(ctx, corr_apply_kernel<K, double>, smem);                                                                                \
            if (rc == XDEMHIP_OK)                                                                                                                     \
                hipLaunchKernelGGL((corr_apply_kernel<K, double>), dim3(blocks), dim3(256), smem, ctx->stream, A, static_cast<const double*>(d_elev), \
                                   static_cast<double*>(d_out));                                                                                      \
        }                                                                                                                                             \
    } while (0)
    if (kind == XDEMHIP_CORR_GRID) XD_BC_GO(XDEMHIP_CORR_GRID);
    else if (kind == XDEMHIP_CORR_PERBIN) XD_BC_GO(XDEMHIP_CORR_PERBIN);
    else if (kind == XDEMHIP_CORR_POLY) XD_BC_GO(XDEMHIP_CORR_POLY);
    else XD_BC_GO(XDEMHIP_CORR_SUMSIN);
#undef XD_BC_GO
    if (rc) return rc;
    (void)hipEventRecord(ctx->ev_stop, ctx->stream);
    ctx->timed = true;
    if (hipGetLastError() != hipSuccess) rc = xd_fail(ctx, XDEMHIP_EHIP, "correction kernel launch failed");
    if (rc == XDEMHIP_OK && hipMemcpyAsync(&miss, A.missing, 8, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess)
        rc = xd_fail(ctx, XDEMHIP_EHIP, "correction kernel failed");
    if (rc == XDEMHIP_OK) rc = buf.finish();
    if (n_missing) *n_missing = (int64_t)miss;
    return rc;
}

}  // extern "C"
