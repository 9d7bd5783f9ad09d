// volume.hip -- the raster passes of xdem/volume.py (include/xdemhip.h, "hypsometric binning and gap filling"):
//   hypsometric_binning                       volume.py:43-128    label statistics, grouping, per-segment median
//   calculate_hypsometry_area                 volume.py:239-299   -> hyp_area_kernel
//   hypsometric_interpolation                 volume.py:353-404   the one-label case + fill
//   get_regional_hypsometric_signal           volume.py:568-665   labelled statistics, grouping, per-segment median
//   norm_regional_hypsometric_interpolation   volume.py:668-808   the same with standard deviations + fill with a model per label
// Upstream loops over the glaciers of the index map and builds full-raster masks for each: O(G N).  Here the rasters are read a
// constant number of times whatever G is:
//   1. hyp_stats_kernel    per label: pixels, inliers (finite dDEM and reference), min / max of the reference over both sets
//   2. hyp_group_kernel    per inlier of a kept label: its bin by binary search in that label's edges (np.digitize), group =
//                          rank(label) * nb + bin; a count per group.  rank_scan_kernel, then hyp_scatter_kernel: the values in
//                          group-contiguous segments (the counting sort of icp.hip)
//   3. hyp_segment_kernel  per segment: count, exact median, on request the standard deviation (volume.h)
//   4. hyp_fill_kernel     out = fill ? model[rank(label)](ref) : ddem
// Counts are integers and extremes atomic min / max on orderable keys: no result depends on the order the atomics run in.  The
// order INSIDE a segment does, so everything taken from a segment is either an order statistic or a sum over the sorted segment.
#include <math.h>
#include <string.h>

#include <string>
#include <vector>

#include "common.h"
#include "select.h"
#include "select_run.h"
#include "rank_select.h"
#include "volume.h"

struct xdemhip_hypso {
    xdemhip_ctx* ctx = nullptr;
    int t_f32 = 1, r_f32 = 1;
    int64_t n = 0, L = 2;   // L: size of the label tables (2^20 with labels, 2 without: "label 1")
    XdOwned mem;            // every device buffer of the plan but the caller's own device arrays
    void *ddem = nullptr, *ref = nullptr, *labels = nullptr, *mask = nullptr;   // the caller's device arrays, or owned copies of its host arrays
    int32_t* rank_of = nullptr;   // [L] rank of a kept label, -1 otherwise (rebuilt by every call that takes a list of labels)
    int32_t* grp = nullptr;       // [n] group of every pixel in the last xdemhip_hypso_segments call, -1: in none
    bool grouped = false;
};

namespace xd {
namespace {

constexpr int64_t HYP_LABEL_LIMIT = (int64_t)1 << 20;
constexpr int HYP_LDS_GROUPS = 4096;   // group counters of one workgroup in LDS (16 KiB); more groups count in global memory
constexpr int HYP_AREA_LDS_BINS = 8192;

__device__ __forceinline__ int32_t hyp_label(const int32_t* __restrict__ labels, const uint8_t* __restrict__ mask, int64_t p) {
    return labels ? labels[p] : (mask ? (int32_t)(mask[p] != 0) : 1);
}

__device__ __forceinline__ unsigned long long wave_min(unsigned long long v) {
    for (int off = 32; off > 0; off >>= 1) { const unsigned long long o = __shfl_xor(v, off); v = o < v ? o : v; }
    return v;
}
__device__ __forceinline__ unsigned long long wave_max(unsigned long long v) {
    for (int off = 32; off > 0; off >>= 1) { const unsigned long long o = __shfl_xor(v, off); v = o > v ? o : v; }
    return v;
}
__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// ---- 1. label statistics --------------------------------------------------------------------------------------------------------------
// tab: six planes of L words: pixels | inliers | min key, max key of ref over the label's pixels | the same over its inliers.
// Every wave walks whole groups of 64 pixels (the loop runs to n rounded up), so the wave-wide operations see all lanes.
__global__ __launch_bounds__(256) void hyp_stats_init_kernel(unsigned long long* tab, int64_t L) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < 6 * L; i += (int64_t)gridDim.x * blockDim.x) {
        const int plane = (int)(i / L);
        tab[i] = (plane == 2 || plane == 4) ? ~0ull : 0ull;
    }
}

template <typename T, typename R>
__global__ __launch_bounds__(256) void hyp_stats_kernel(const T* __restrict__ ddem, const R* __restrict__ ref, const int32_t* __restrict__ labels,
                                                        const uint8_t* __restrict__ mask, int64_t n, int64_t L, unsigned long long* tab,
                                                        unsigned long long* misc) {
    const int64_t n_pad = (n + 63) & ~(int64_t)63;
    const int lane = threadIdx.x & 63;
    unsigned long long bad = 0, ref_bad = 0;
    // a run of trips in which the whole wave saw one label is kept in registers and flushed when the label changes: a raster with one
    // label (or large outlines) would otherwise send every wave's atomics of every trip to the same six words
    int32_t run_lab = 0;
    unsigned long long run_pix = 0, run_inl = 0, run_amin = ~0ull, run_amax = 0, run_imin = ~0ull, run_imax = 0;
    auto flush = [&]() {
        if (run_lab != 0 && lane == 0) {
            atomicAdd(&tab[run_lab], run_pix);
            if (run_inl) atomicAdd(&tab[L + run_lab], run_inl);
            if (run_amin != ~0ull) { atomicMin(&tab[2 * L + run_lab], run_amin); atomicMax(&tab[3 * L + run_lab], run_amax); }
            if (run_imin != ~0ull) { atomicMin(&tab[4 * L + run_lab], run_imin); atomicMax(&tab[5 * L + run_lab], run_imax); }
        }
        run_pix = 0; run_inl = 0; run_amin = ~0ull; run_amax = 0; run_imin = ~0ull; run_imax = 0;
    };
    for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < n_pad; p += (int64_t)gridDim.x * 256) {
        int32_t lab = 0;
        bool rf = false, df = false;
        unsigned long long key = 0;
        if (p < n) {
            lab = hyp_label(labels, mask, p);
            const R r = ref[p];
            rf = t_finite<R>(r);
            ref_bad += !rf;
            if (lab < 0 || lab >= L) { ++bad; lab = 0; }
            if (lab != 0 && rf) {
                df = t_finite<T>(ddem[p]);
                key = (unsigned long long)key_of((double)r);
            }
        }
        const int32_t lab0 = __builtin_amdgcn_readfirstlane(lab);
        if (__all(lab == lab0)) {
            if (lab0 != 0) {   // one label across the wave (so all 64 pixels are inside the raster): joins the run
                if (lab0 != run_lab) { flush(); run_lab = lab0; }
                const unsigned long long a_min = wave_min(rf ? key : ~0ull), a_max = wave_max(rf ? key : 0ull);
                const unsigned long long i_min = wave_min(df ? key : ~0ull), i_max = wave_max(df ? key : 0ull);
                run_pix += 64ull;
                run_inl += (unsigned long long)__popcll(__ballot(df));
                run_amin = a_min < run_amin ? a_min : run_amin; run_amax = a_max > run_amax ? a_max : run_amax;
                run_imin = i_min < run_imin ? i_min : run_imin; run_imax = i_max > run_imax ? i_max : run_imax;
            }
        } else {
            // a wave on an outline's border: the labels of its first lanes are reduced by ballot, one set of atomics each (three
            // rounds: the background and two outlines), what is left goes lane by lane
            unsigned long long rem = __ballot(lab != 0);
            for (int round = 0; round < 3 && rem; ++round) {
                const int src = __ffsll((unsigned long long)rem) - 1;
                const int32_t l0 = __shfl(lab, src);
                const bool mine = lab == l0;
                const unsigned long long same = __ballot(mine);
                const unsigned long long inl = (unsigned long long)__popcll(__ballot(mine && df));
                const unsigned long long a_min = wave_min(mine && rf ? key : ~0ull), a_max = wave_max(mine && rf ? key : 0ull);
                const unsigned long long i_min = wave_min(mine && df ? key : ~0ull), i_max = wave_max(mine && df ? key : 0ull);
                if (lane == src) {
                    atomicAdd(&tab[l0], (unsigned long long)__popcll(same));
                    if (inl) atomicAdd(&tab[L + l0], inl);
                    if (a_min != ~0ull) { atomicMin(&tab[2 * L + l0], a_min); atomicMax(&tab[3 * L + l0], a_max); }
                    if (i_min != ~0ull) { atomicMin(&tab[4 * L + l0], i_min); atomicMax(&tab[5 * L + l0], i_max); }
                }
                rem &= ~same;
            }
            if ((rem >> lane) & 1ull) {
                atomicAdd(&tab[lab], 1ull);
                if (rf) { atomicMin(&tab[2 * L + lab], key); atomicMax(&tab[3 * L + lab], key); }
                if (df) { atomicAdd(&tab[L + lab], 1ull); atomicMin(&tab[4 * L + lab], key); atomicMax(&tab[5 * L + lab], key); }
            }
        }
    }
    flush();
    bad = wave_sum(bad);
    ref_bad = wave_sum(ref_bad);
    if (lane == 0) {
        if (bad) atomicAdd(&misc[1], bad);
        if (ref_bad) atomicAdd(&misc[2], ref_bad);
    }
}

// the labels that occur, in whatever order the atomics give (the host sorts them): misc[0] counts them
__global__ __launch_bounds__(256) void hyp_stats_compact_kernel(const unsigned long long* __restrict__ tab, int64_t L, int64_t cap, unsigned long long* misc,
                                                                int32_t* __restrict__ ids, int64_t* __restrict__ cnt, double* __restrict__ ext) {
    for (int64_t l = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; l < L; l += (int64_t)gridDim.x * blockDim.x) {
        if (l == 0 || tab[l] == 0ull) continue;
        const unsigned long long at = atomicAdd(&misc[0], 1ull);
        if ((int64_t)at >= cap) continue;
        ids[at] = (int32_t)l;
        cnt[2 * at] = (int64_t)tab[l];
        cnt[2 * at + 1] = (int64_t)tab[L + l];
        for (int k = 0; k < 4; ++k) {
            const unsigned long long key = tab[(2 + k) * L + l];
            const bool none = (k & 1) ? (key == 0ull) : (key == ~0ull);   // (no finite double has the key 0 or all ones)
            ext[4 * at + k] = none ? (double)NAN : val_of((uint64_t)key);
        }
    }
}

__global__ __launch_bounds__(256) void hyp_rank_fill_kernel(int32_t* rank_of, int64_t L) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < L; i += (int64_t)gridDim.x * blockDim.x) rank_of[i] = -1;
}
__global__ __launch_bounds__(256) void hyp_rank_set_kernel(int32_t* rank_of, int64_t L, const int32_t* __restrict__ ids, int n_kept) {
    for (int r = blockIdx.x * blockDim.x + threadIdx.x; r < n_kept; r += gridDim.x * blockDim.x) {
        const int32_t l = ids[r];
        if (l > 0 && l < L) rank_of[l] = r;
    }
}

// ---- 2. grouping ----------------------------------------------------------------------------------------------------------------------
template <typename T, typename R>
__global__ __launch_bounds__(256) void hyp_group_kernel(const T* __restrict__ ddem, const R* __restrict__ ref, const int32_t* __restrict__ labels,
                                                        const uint8_t* __restrict__ mask, int64_t n, int64_t L, const int32_t* __restrict__ rank_of, int nb,
                                                        const double* __restrict__ edges, int n_groups, int use_lds, unsigned long long* cnt,
                                                        int32_t* __restrict__ grp) {
    extern __shared__ unsigned int hyp_s_cnt[];
    if (use_lds) {
        for (int g = threadIdx.x; g < n_groups; g += 256) hyp_s_cnt[g] = 0u;
        __syncthreads();
    }
    const int64_t n_pad = (n + 63) & ~(int64_t)63;
    const int lane = threadIdx.x & 63;
    for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < n_pad; p += (int64_t)gridDim.x * 256) {
        int32_t g = -1;
        if (p < n) {
            const int32_t lab = hyp_label(labels, mask, p);
            const int32_t r = (lab > 0 && lab < L) ? rank_of[lab] : -1;
            if (r >= 0) {
                const T d = ddem[p];
                const R e = ref[p];
                if (t_finite<T>(d) && t_finite<R>(e)) {
                    const int i = hyp_count_le(edges + (int64_t)r * (nb + 1), nb + 1, (double)e);
                    if (i >= 1 && i <= nb) g = r * nb + (i - 1);
                }
            }
            grp[p] = g;
        }
        if (use_lds) {
            if (g >= 0) atomicAdd(&hyp_s_cnt[g], 1u);
        } else {
            const int32_t g0 = __builtin_amdgcn_readfirstlane(g);
            if (__all(g == g0)) {
                if (g0 >= 0 && lane == 0) atomicAdd(&cnt[g0], 64ull);
            } else if (g >= 0) {
                atomicAdd(&cnt[g], 1ull);
            }
        }
    }
    if (use_lds) {
        __syncthreads();
        for (int g = threadIdx.x; g < n_groups; g += 256)
            if (hyp_s_cnt[g]) atomicAdd(&cnt[g], (unsigned long long)hyp_s_cnt[g]);
    }
}

// ---- 3. per-segment statistics: hyp_scatter_kernel and hyp_segment_kernel of volume.h (demstack.hip runs the same two) ----------------

// ---- 4. fused fill ------------------------------------------------------------------------------------------------------------------------
// mode 0: fill where the label is kept and the dDEM is not finite; 1: wherever the label is kept.  round_ref: the model's value is
// written into a plane of the reference's dtype first (volume.py:394-395), as hypsometric_interpolation does.
template <typename T, typename R>
__global__ __launch_bounds__(256) void hyp_fill_kernel(const T* __restrict__ ddem, const R* __restrict__ ref, const int32_t* __restrict__ labels,
                                                       const uint8_t* __restrict__ mask, int64_t n, int64_t L, const int32_t* __restrict__ rank_of, int mode,
                                                       int m, const double* __restrict__ xs, const double* __restrict__ ys, int round_ref, void* __restrict__ out,
                                                       int out_f64) {
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (int64_t)gridDim.x * blockDim.x) {
        const T d = ddem[p];
        const int32_t lab = hyp_label(labels, mask, p);
        const int32_t r = (lab > 0 && lab < L) ? rank_of[lab] : -1;
        double v = (double)d;
        if (r >= 0 && (mode == 1 || !t_finite<T>(d))) {
            v = hyp_interp1d(xs + (int64_t)r * m, ys + (int64_t)r * m, m, (double)ref[p]);
            if (round_ref) v = (double)(R)v;
        }
        if (out_f64) static_cast<double*>(out)[p] = v;
        else static_cast<float*>(out)[p] = (float)v;
    }
}

// ---- calculate_hypsometry_area ------------------------------------------------------------------------------------------------------------
// timeframe 0 "reference": e = ref; 1 "nonreference": e = ref - f(ref); 2 "mean": e = ref - f(ref) / 2, in float64 (the reference
// raster widened exactly).  np.histogram(e, edges): [edges[i], edges[i + 1]), the last bin closed on the right; NaN in none.
template <typename R>
__global__ __launch_bounds__(256) void hyp_area_kernel(const R* __restrict__ ref, int64_t n, int timeframe, int m, const double* __restrict__ xs,
                                                       const double* __restrict__ ys, int nb, const double* __restrict__ edges, int use_lds,
                                                       unsigned long long* cnt) {
    extern __shared__ unsigned int hyp_s_cnt[];
    if (use_lds) {
        for (int g = threadIdx.x; g < nb; g += 256) hyp_s_cnt[g] = 0u;
        __syncthreads();
    }
    const double last = edges[nb];
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (int64_t)gridDim.x * blockDim.x) {
        const double x = (double)ref[p];
        double e = x;
        if (timeframe == 1) e = x - hyp_interp1d(xs, ys, m, x);
        else if (timeframe == 2) e = x - hyp_interp1d(xs, ys, m, x) / 2.0;
        int i = hyp_count_le(edges, nb + 1, e) - 1;
        if (e == last) i = nb - 1;
        if (i >= 0 && i < nb) {
            if (use_lds) atomicAdd(&hyp_s_cnt[i], 1u);
            else atomicAdd(&cnt[i], 1ull);
        }
    }
    if (use_lds) {
        __syncthreads();
        for (int g = threadIdx.x; g < nb; g += 256)
            if (hyp_s_cnt[g]) atomicAdd(&cnt[g], (unsigned long long)hyp_s_cnt[g]);
    }
}

int hyp_set_ranks(xdemhip_hypso* P, XdBuffers& buf, int n_kept, const int32_t* ids) {
    xdemhip_ctx* ctx = P->ctx;
    for (int r = 0; r < n_kept; ++r)
        if (ids[r] <= 0 || ids[r] >= P->L) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_hypso: a kept label must lie in [1, 2^20)");
    const int32_t* d_ids = buf.input(ids, (size_t)n_kept * 4, XDEMHIP_HOST);
    if (buf.rc) return buf.rc;
    hipLaunchKernelGGL(hyp_rank_fill_kernel, dim3(grid_for(ctx, P->L, 256, 8)), dim3(256), 0, ctx->stream, P->rank_of, P->L);
    hipLaunchKernelGGL(hyp_rank_set_kernel, dim3(grid_for(ctx, n_kept, 256, 8)), dim3(256), 0, ctx->stream, P->rank_of, P->L, d_ids, n_kept);
    return launched(ctx, "hyp_rank_set_kernel");
}

}  // namespace
}  // namespace xd

using namespace xd;

#define XD_HYP_DISPATCH(P, CALL)                          \
    do {                                                  \
        if ((P)->t_f32 && (P)->r_f32) { CALL(float, float); }      \
        else if ((P)->t_f32) { CALL(float, double); }             \
        else if ((P)->r_f32) { CALL(double, float); }             \
        else { CALL(double, double); }                            \
    } while (0)

extern "C" {

int xdemhip_hypso_create(xdemhip_ctx* ctx, const void* ddem, int ddem_dtype, const void* ref, int ref_dtype, const int32_t* labels,
                         const unsigned char* mask, int64_t n, int memspace, xdemhip_hypso** out) {
    if (!ctx || !out) return XDEMHIP_EINVAL;
    *out = nullptr;
    if (!ddem || !ref) return xd_fail(ctx, XDEMHIP_EINVAL, "null argument");
    if (labels && mask) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_hypso_create: labels or a mask, not both");
    if ((ddem_dtype != XDEMHIP_F32 && ddem_dtype != XDEMHIP_F64) || (ref_dtype != XDEMHIP_F32 && ref_dtype != XDEMHIP_F64))
        return xd_fail(ctx, XDEMHIP_EINVAL, "dtype must be float32 or float64");
    if (memspace != XDEMHIP_HOST && memspace != XDEMHIP_DEVICE) return xd_fail(ctx, XDEMHIP_EINVAL, "bad memspace");
    if (n < 1 || n >= ((int64_t)1 << 32)) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_hypso_create: 1 to 2^32 - 1 pixels");
    XD_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    xdemhip_hypso* P = new xdemhip_hypso;
    P->ctx = P->mem.ctx = ctx; P->n = n;
    P->t_f32 = ddem_dtype == XDEMHIP_F32; P->r_f32 = ref_dtype == XDEMHIP_F32;
    P->L = labels ? HYP_LABEL_LIMIT : 2;
    P->ddem = P->mem.keep(ddem, (size_t)n * (P->t_f32 ? 4 : 8), memspace, "xdemhip_hypso_create");
    P->ref = P->mem.keep(ref, (size_t)n * (P->r_f32 ? 4 : 8), memspace, "xdemhip_hypso_create");
    P->labels = P->mem.keep(labels, (size_t)n * 4, memspace, "xdemhip_hypso_create");
    P->mask = P->mem.keep(mask, (size_t)n, memspace, "xdemhip_hypso_create");
    P->rank_of = P->mem.take<int32_t>((size_t)P->L, "xdemhip_hypso_create");
    int rc = P->mem.rc;
    if (rc == XDEMHIP_OK) rc = xd_sync(ctx);   // (the caller's host arrays may go once this returns)
    if (rc) { xdemhip_hypso_destroy(P); return rc; }
    *out = P;
    return XDEMHIP_OK;
}

void xdemhip_hypso_destroy(xdemhip_hypso* P) { delete P; }   // (its owner frees the device buffers)

int xdemhip_hypso_label_stats(xdemhip_hypso* P, int64_t cap, int32_t* ids, int64_t* counts, double* extremes, int64_t* n_found,
                              int64_t* n_bad_labels, int64_t* n_ref_invalid) {
    XdFetchScope fetch_scope_(P ? P->ctx : nullptr);
    if (!P) return XDEMHIP_EINVAL;
    xdemhip_ctx* ctx = P->ctx;
    if (!ids || !counts || !extremes || !n_found || cap < 1) return xd_fail(ctx, XDEMHIP_EINVAL, "null argument");
    XD_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    const int64_t L = P->L, n = P->n;
    unsigned long long misc[3] = {0, 0, 0};   // (a copy's destination: declared before the buffers)
    XdBuffers buf(ctx, "xdemhip_hypso_label_stats");
    unsigned long long* tab = buf.alloc<unsigned long long>((size_t)6 * L);
    unsigned long long* d_misc = buf.alloc<unsigned long long>(3);
    int32_t* d_ids = buf.alloc<int32_t>((size_t)cap);
    int64_t* d_cnt = buf.alloc<int64_t>((size_t)2 * cap);
    double* d_ext = buf.alloc<double>((size_t)4 * cap);
    if (buf.rc) return buf.rc;
    if (hipMemsetAsync(d_misc, 0, 24, ctx->stream) != hipSuccess) return xd_fail(ctx, XDEMHIP_EHIP, "hipMemsetAsync failed");
    hipLaunchKernelGGL(hyp_stats_init_kernel, dim3(grid_for(ctx, 6 * L, 256, 8)), dim3(256), 0, ctx->stream, tab, L);
    const dim3 g(grid_for(ctx, n, 256, 16));
#define XD_HYP_STATS(T, R)                                                                                                                       \
    hipLaunchKernelGGL((hyp_stats_kernel<T, R>), g, dim3(256), 0, ctx->stream, static_cast<const T*>(P->ddem), static_cast<const R*>(P->ref),  \
                       static_cast<const int32_t*>(P->labels), static_cast<const uint8_t*>(P->mask), n, L, tab, d_misc)
    XD_HYP_DISPATCH(P, XD_HYP_STATS);
#undef XD_HYP_STATS
    hipLaunchKernelGGL(hyp_stats_compact_kernel, dim3(grid_for(ctx, L, 256, 8)), dim3(256), 0, ctx->stream, tab, L, cap, d_misc, d_ids, d_cnt, d_ext);
    int rc = launched(ctx, "hyp_stats_kernel");
    if (rc == XDEMHIP_OK && hipMemcpyAsync(misc, d_misc, 24, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess) rc = xd_fail(ctx, XDEMHIP_EHIP, "D2H copy failed");
    if (rc == XDEMHIP_OK) rc = xd_sync(ctx);
    if (rc) return rc;
    const int64_t found = (int64_t)misc[0] < cap ? (int64_t)misc[0] : cap;
    *n_found = (int64_t)misc[0];
    if (n_bad_labels) *n_bad_labels = (int64_t)misc[1];
    if (n_ref_invalid) *n_ref_invalid = (int64_t)misc[2];
    if (found > 0) {
        if (hipMemcpyAsync(ids, d_ids, (size_t)found * 4, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
            hipMemcpyAsync(counts, d_cnt, (size_t)found * 16, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
            hipMemcpyAsync(extremes, d_ext, (size_t)found * 32, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess)
            return xd_fail(ctx, XDEMHIP_EHIP, "D2H copy failed (xdemhip_hypso_label_stats)");
    }
    return buf.finish();
}

int xdemhip_hypso_segments(xdemhip_hypso* P, int n_kept, const int32_t* ids, int nb, const double* edges, int want_std, int64_t* counts,
                           double* medians, double* stds) {
    XdFetchScope fetch_scope_(P ? P->ctx : nullptr);
    if (!P) return XDEMHIP_EINVAL;
    xdemhip_ctx* ctx = P->ctx;
    if (!ids || !edges || !counts || !medians || (want_std && !stds)) return xd_fail(ctx, XDEMHIP_EINVAL, "null argument");
    if (n_kept < 1 || nb < 1 || (int64_t)n_kept * (nb + 1) >= ((int64_t)1 << 31))
        return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_hypso_segments: at least one label and one bin, fewer than 2^31 groups");
    XD_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    const int64_t n = P->n;
    const int n_groups = n_kept * nb;
    P->grouped = false;
    if (!P->grp) P->grp = P->mem.take<int32_t>((size_t)n, "xdemhip_hypso_segments");
    { const int rc_ = P->mem.status(); if (rc_) return rc_; }
    const size_t es = P->t_f32 ? 4 : 8;
    unsigned long long total = 0;   // (a copy's destination: declared before the buffers)
    XdBuffers buf(ctx, "xdemhip_hypso_segments");
    int rc = hyp_set_ranks(P, buf, n_kept, ids);
    if (rc) return rc;
    const double* d_edges = buf.input(edges, (size_t)n_kept * (nb + 1) * 8, XDEMHIP_HOST);
    unsigned long long* off = buf.alloc<unsigned long long>((size_t)n_groups + 1);
    unsigned long long* cursor = buf.alloc<unsigned long long>((size_t)n_groups);
    int64_t* d_counts = buf.output(counts, (size_t)n_groups * 8, XDEMHIP_HOST);
    double* d_med = buf.output(medians, (size_t)n_groups * 8, XDEMHIP_HOST);
    double* d_sd = want_std ? buf.output(stds, (size_t)n_groups * 8, XDEMHIP_HOST) : nullptr;
    if (buf.rc) return buf.rc;
    if (hipMemsetAsync(off, 0, ((size_t)n_groups + 1) * 8, ctx->stream) != hipSuccess) return xd_fail(ctx, XDEMHIP_EHIP, "hipMemsetAsync failed");
    const dim3 g(grid_for(ctx, n, 256, 16));
    const int use_lds = n_groups <= HYP_LDS_GROUPS;
    const size_t lds_cnt = use_lds ? (size_t)n_groups * 4 : 0;
#define XD_HYP_GROUP(T, R)                                                                                                                             \
    hipLaunchKernelGGL((hyp_group_kernel<T, R>), g, dim3(256), lds_cnt, ctx->stream, static_cast<const T*>(P->ddem), static_cast<const R*>(P->ref),  \
                       static_cast<const int32_t*>(P->labels), static_cast<const uint8_t*>(P->mask), n, P->L, P->rank_of, nb, d_edges, n_groups,     \
                       use_lds, off, P->grp)
    XD_HYP_DISPATCH(P, XD_HYP_GROUP);
#undef XD_HYP_GROUP
    hipLaunchKernelGGL(rank_scan_kernel, dim3(1), dim3(1024), 0, ctx->stream, off, (int64_t)n_groups, off + n_groups);
    rc = launched(ctx, "hyp_group_kernel");
    if (rc == XDEMHIP_OK && hipMemcpyAsync(cursor, off, (size_t)n_groups * 8, hipMemcpyDeviceToDevice, ctx->stream) != hipSuccess)
        rc = xd_fail(ctx, XDEMHIP_EHIP, "device copy failed");
    if (rc == XDEMHIP_OK && hipMemcpyAsync(&total, off + n_groups, 8, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess) rc = xd_fail(ctx, XDEMHIP_EHIP, "D2H copy failed");
    if (rc == XDEMHIP_OK) rc = xd_sync(ctx);
    if (rc) return rc;
    P->grouped = true;
    void* seg = buf.alloc((size_t)(total ? total : 1) * es);
    if (buf.rc) return buf.rc;
    // segments longer than the switch's value leave the LDS route (include/xdemhip_test.h: "hypso_seg_lds")
    const int cap = ctx->hypso_seg_lds ? ctx->hypso_seg_lds : HYP_SEG_LDS;
    const size_t lds_seg = (size_t)cap * (P->t_f32 ? 4 : 8);
    const int seg_blocks = n_groups < ctx->num_cu * 8 ? n_groups : ctx->num_cu * 8;
    if (P->t_f32) {
        if (total) hipLaunchKernelGGL((hyp_scatter_kernel<float>), g, dim3(256), 0, ctx->stream, static_cast<const float*>(P->ddem), P->grp, n, cursor, static_cast<float*>(seg));
        rc = set_big_lds(ctx, hyp_segment_kernel<float>, lds_seg);
        if (rc == XDEMHIP_OK)
            hipLaunchKernelGGL((hyp_segment_kernel<float>), dim3(seg_blocks), dim3(256), lds_seg, ctx->stream, static_cast<float*>(seg), off, n_groups, cap, want_std,
                               d_counts, d_med, d_sd);
    } else {
        if (total) hipLaunchKernelGGL((hyp_scatter_kernel<double>), g, dim3(256), 0, ctx->stream, static_cast<const double*>(P->ddem), P->grp, n, cursor, static_cast<double*>(seg));
        rc = set_big_lds(ctx, hyp_segment_kernel<double>, lds_seg);
        if (rc == XDEMHIP_OK)
            hipLaunchKernelGGL((hyp_segment_kernel<double>), dim3(seg_blocks), dim3(256), lds_seg, ctx->stream, static_cast<double*>(seg), off, n_groups, cap, want_std,
                               d_counts, d_med, d_sd);
    }
    if (rc == XDEMHIP_OK) rc = launched(ctx, "hyp_segment_kernel");
    if (rc) return rc;
    return buf.finish();
}

int xdemhip_hypso_groups(xdemhip_hypso* P, int32_t* groups_out, int memspace) {
    if (!P) return XDEMHIP_EINVAL;
    xdemhip_ctx* ctx = P->ctx;
    if (!groups_out) return xd_fail(ctx, XDEMHIP_EINVAL, "null argument");
    if (memspace != XDEMHIP_HOST && memspace != XDEMHIP_DEVICE) return xd_fail(ctx, XDEMHIP_EINVAL, "bad memspace");
    if (!P->grouped) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_hypso_groups: no xdemhip_hypso_segments call yet");
    XD_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    XD_HIP_CHECK(ctx, hipMemcpyAsync(groups_out, P->grp, (size_t)P->n * 4, memspace == XDEMHIP_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, ctx->stream));
    return xd_sync(ctx);
}

int xdemhip_hypso_fill(xdemhip_hypso* P, int mode, int n_kept, const int32_t* ids, int m, const double* xs, const double* ys, int round_to_ref,
                       void* out, int out_dtype, int memspace) {
    XdFetchScope fetch_scope_(P ? P->ctx : nullptr);
    if (!P) return XDEMHIP_EINVAL;
    xdemhip_ctx* ctx = P->ctx;
    if (!out || (n_kept > 0 && (!ids || !xs || !ys))) return xd_fail(ctx, XDEMHIP_EINVAL, "null argument");
    if (mode != 0 && mode != 1) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_hypso_fill: mode 0 (voids of kept labels) or 1 (kept labels)");
    if (n_kept < 0 || (n_kept > 0 && m < 2) || (int64_t)n_kept * m >= ((int64_t)1 << 31)) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_hypso_fill: a model needs at least 2 points");
    if (out_dtype != XDEMHIP_F32 && out_dtype != XDEMHIP_F64) return xd_fail(ctx, XDEMHIP_EINVAL, "dtype must be float32 or float64");
    if (!P->t_f32 && out_dtype == XDEMHIP_F32) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_hypso_fill: a float64 dDEM needs a float64 output");
    if (memspace != XDEMHIP_HOST && memspace != XDEMHIP_DEVICE) return xd_fail(ctx, XDEMHIP_EINVAL, "bad memspace");
    XD_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    const int64_t n = P->n;
    XdBuffers buf(ctx, "xdemhip_hypso_fill");
    int rc = hyp_set_ranks(P, buf, n_kept, ids);
    if (rc) return rc;
    const double* d_xs = n_kept ? buf.input(xs, (size_t)n_kept * m * 8, XDEMHIP_HOST) : nullptr;
    const double* d_ys = n_kept ? buf.input(ys, (size_t)n_kept * m * 8, XDEMHIP_HOST) : nullptr;
    void* d_out = buf.output(out, (size_t)n * (out_dtype == XDEMHIP_F32 ? 4 : 8), memspace);
    if (buf.rc) return buf.rc;
    const dim3 g(grid_for(ctx, n, 256, 16));
    const int out_f64 = out_dtype == XDEMHIP_F64;
    (void)hipEventRecord(ctx->ev_start, ctx->stream);
#define XD_HYP_FILL(T, R)                                                                                                                         \
    hipLaunchKernelGGL((hyp_fill_kernel<T, R>), g, dim3(256), 0, ctx->stream, static_cast<const T*>(P->ddem), static_cast<const R*>(P->ref),    \
                       static_cast<const int32_t*>(P->labels), static_cast<const uint8_t*>(P->mask), n, P->L, P->rank_of, mode, m, d_xs, d_ys,  \
                       round_to_ref, d_out, out_f64)
    XD_HYP_DISPATCH(P, XD_HYP_FILL);
#undef XD_HYP_FILL
    (void)hipEventRecord(ctx->ev_stop, ctx->stream);
    ctx->timed = true;
    rc = launched(ctx, "hyp_fill_kernel");
    if (rc == XDEMHIP_OK) rc = buf.finish();
    // (a device plane is complete when the call returns, whichever stream the caller reads it on)
    if (rc == XDEMHIP_OK && memspace == XDEMHIP_DEVICE) rc = xd_sync(ctx);
    return rc;
}

int xdemhip_hypso_area(xdemhip_ctx* ctx, const void* ref, int dtype, int64_t n, int timeframe, int m, const double* xs, const double* ys, int nb,
                       const double* edges, int64_t* counts, int memspace) {
    XdFetchScope fetch_scope_(ctx);
    if (!ctx) return XDEMHIP_EINVAL;
    if (!ref || !edges || !counts) return xd_fail(ctx, XDEMHIP_EINVAL, "null argument");
    if (dtype != XDEMHIP_F32 && dtype != XDEMHIP_F64) return xd_fail(ctx, XDEMHIP_EINVAL, "dtype must be float32 or float64");
    if (memspace != XDEMHIP_HOST && memspace != XDEMHIP_DEVICE) return xd_fail(ctx, XDEMHIP_EINVAL, "bad memspace");
    if (timeframe < 0 || timeframe > 2) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_hypso_area: timeframe 0 reference, 1 nonreference, 2 mean");
    if (timeframe != 0 && (m < 2 || !xs || !ys)) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_hypso_area: the model needs at least 2 points");
    if (n < 1 || nb < 1) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_hypso_area: at least one pixel and one bin");
    XD_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    XdBuffers buf(ctx, "xdemhip_hypso_area");
    const void* d_ref = buf.input(ref, (size_t)n * (dtype == XDEMHIP_F32 ? 4 : 8), memspace);
    const double* d_xs = timeframe ? buf.input(xs, (size_t)m * 8, XDEMHIP_HOST) : nullptr;
    const double* d_ys = timeframe ? buf.input(ys, (size_t)m * 8, XDEMHIP_HOST) : nullptr;
    const double* d_edges = buf.input(edges, ((size_t)nb + 1) * 8, XDEMHIP_HOST);
    unsigned long long* d_cnt = buf.alloc<unsigned long long>((size_t)nb);
    if (buf.rc) return buf.rc;
    if (hipMemsetAsync(d_cnt, 0, (size_t)nb * 8, ctx->stream) != hipSuccess) return xd_fail(ctx, XDEMHIP_EHIP, "hipMemsetAsync failed");
    const int use_lds = nb <= HYP_AREA_LDS_BINS;
    const size_t lds = use_lds ? (size_t)nb * 4 : 0;
    const dim3 g(grid_for(ctx, n, 256, 16));
    if (dtype == XDEMHIP_F32)
        hipLaunchKernelGGL((hyp_area_kernel<float>), g, dim3(256), lds, ctx->stream, static_cast<const float*>(d_ref), n, timeframe, m, d_xs, d_ys, nb, d_edges, use_lds, d_cnt);
    else
        hipLaunchKernelGGL((hyp_area_kernel<double>), g, dim3(256), lds, ctx->stream, static_cast<const double*>(d_ref), n, timeframe, m, d_xs, d_ys, nb, d_edges, use_lds, d_cnt);
    int rc = launched(ctx, "hyp_area_kernel");
    if (rc == XDEMHIP_OK && hipMemcpyAsync(counts, d_cnt, (size_t)nb * 8, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess) rc = xd_fail(ctx, XDEMHIP_EHIP, "D2H copy failed");
    if (rc == XDEMHIP_OK) rc = buf.finish();
    return rc;
}

}  // extern "C"
