// demstack.hip -- a time series of T DEMs on one grid in batched passes (include/xdemhip.h, "a stack of DEMs"): what
// xdem/demcollection.py and xdem/ddem.py do one DEM at a time,
//   DEMCollection.subtract_dems      demcollection.py:104-136   one full-raster subtraction per DEM
//   dDEM.interpolate                 ddem.py:256-264            one hypsometric_interpolation per dDEM
//   DEMCollection.get_dh_series      demcollection.py:193-229   one masked np.nanmean per dDEM
// in a number of launches that does not depend on T:
//   1. stk_subtract_kernel   ddem_t = ref - dem_t for every plane, the reference loaded once per STK_CHUNK planes; per plane the
//                            pixels that differ from the reference and the non-finite differences.  stk_zero_kernel: the planes
//                            that equal the reference become 0
//   2. stk_stats_kernel      per plane: inliers (mask_t, finite dDEM_t and reference), min / max of the reference over them
//   3. stk_group_kernel      per inlier its 50 m bin in ITS plane's edges, group = t * nb_max + bin; then rank_scan_kernel and the
//                            hyp_scatter_kernel / hyp_segment_kernel of volume.h over the T * n values: exact medians per segment
//   4. stk_fill_kernel       filled_t = void inside mask_t ? (V)model_t(ref) : ddem_t, and in the same pass per plane over the series
//                            mask: its pixels, the finite values among them and their float64 sum.  Without models: the sums alone
// A thread keeps the counters of STK_CHUNK planes in registers and walks the pixels once per chunk.  Counts are integer atomics,
// extremes atomic min / max on orderable keys, the sums go the fixed order of fixed_sums.h (one partial per workgroup and plane, the
// reduce kernel of biascorr.hip, a grid that depends on the device and n only): no result depends on the order atomics run in.
#include <math.h>
#include <string.h>

#include <string>
#include <vector>

#include "common.h"
#include "select.h"
#include "select_run.h"
#include "rank_select.h"
#include "volume.h"
#include "fixed_sums.h"

struct xdemhip_stack {
    xdemhip_ctx* ctx = nullptr;
    int f32 = 1, T = 0, K = 0, ref_index = 0;
    int64_t n = 0;
    XdOwned mem;                        // every device buffer of the stack but the caller's own device arrays
    void* upload = nullptr;             // [T * n] the planes of host inputs (device inputs are used in place)
    const void* ref = nullptr;          // the reference's input plane
    void *ddem = nullptr, *filled = nullptr;   // [T * n] each: the caller's device array, or the stack's own buffer behind a host array
    void* out_buf[2] = {nullptr, nullptr};     // those own buffers of the two slots (null: none)
    const void** tabs = nullptr;        // [3 * T] device pointers: the input planes | the dDEM planes | the filled planes
    unsigned char* mask_upload = nullptr;      // [K * n] the masks of host inputs
    const unsigned char** mask_tab = nullptr;  // [T] device pointers: the mask of every plane (null: every pixel)
    int32_t* grp = nullptr;             // [T * n] group of every value in the last xdemhip_stack_segments call
    bool subtracted = false, has_filled = false;
    xd::FixedSums sums;
};

namespace xd {
namespace {

constexpr int STK_CHUNK = 8;          // planes whose counters one thread keeps in registers
constexpr int STK_MAX_PLANES = 1024;
constexpr int STK_LDS_BINS = 4096;    // bin counters of one workgroup in LDS (16 KiB); more bins count in global memory

__device__ __forceinline__ bool stk_same(float a, float b) { return __float_as_uint(a) == __float_as_uint(b) || (a != a && b != b); }
__device__ __forceinline__ bool stk_same(double a, double b) { return __double_as_longlong(a) == __double_as_longlong(b) || (a != a && b != b); }

__device__ __forceinline__ unsigned long long stk_block_min(unsigned long long v, unsigned long long* red) {
    for (int off = 32; off > 0; off >>= 1) { const unsigned long long o = __shfl_xor(v, off, 64); v = o < v ? o : v; }
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    unsigned long long r = red[0];
    for (int w = 1; w < 4; ++w) r = red[w] < r ? red[w] : r;
    __syncthreads();
    return r;
}
__device__ __forceinline__ unsigned long long stk_block_max(unsigned long long v, unsigned long long* red) {
    for (int off = 32; off > 0; off >>= 1) { const unsigned long long o = __shfl_xor(v, off, 64); v = o > v ? o : v; }
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    unsigned long long r = red[0];
    for (int w = 1; w < 4; ++w) r = red[w] > r ? red[w] : r;
    __syncthreads();
    return r;
}

// ---- 1. subtraction ---------------------------------------------------------------------------------------------------------------------
// cnt: [T] pixels that differ from the reference (other bits, and not both NaN) | [T] non-finite differences
template <typename V>
__global__ __launch_bounds__(256) void stk_subtract_kernel(const V* const* __restrict__ planes, int ref_index, int T, int64_t n, V* __restrict__ ddem,
                                                           unsigned long long* cnt) {
    __shared__ unsigned long long red[4];
    const V* __restrict__ ref = planes[ref_index];
    for (int c0 = 0; c0 < T; c0 += STK_CHUNK) {
        const int nc = T - c0 < STK_CHUNK ? T - c0 : STK_CHUNK;
        const V* pl[STK_CHUNK];
        unsigned long long dif[STK_CHUNK], bad[STK_CHUNK];
#pragma unroll
        for (int k = 0; k < STK_CHUNK; ++k) { pl[k] = planes[c0 + (k < nc ? k : 0)]; dif[k] = 0ull; bad[k] = 0ull; }
        for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < n; p += (int64_t)gridDim.x * 256) {
            const V r = ref[p];
#pragma unroll
            for (int k = 0; k < STK_CHUNK; ++k) {
                if (k < nc) {
                    const V d = pl[k][p];
                    const V v = r - d;
                    ddem[(int64_t)(c0 + k) * n + p] = v;
                    dif[k] += !stk_same(r, d);
                    bad[k] += !t_finite<V>(v);
                }
            }
        }
#pragma unroll
        for (int k = 0; k < STK_CHUNK; ++k) {
            if (k < nc) {   // (nc is the same in every lane)
                const unsigned long long a = block_sum<unsigned long long>(dif[k], red), b = block_sum<unsigned long long>(bad[k], red);
                if (threadIdx.x == 0) {
                    if (a) atomicAdd(&cnt[c0 + k], a);
                    if (b) atomicAdd(&cnt[T + c0 + k], b);
                }
            }
        }
    }
}

// the planes that equal the reference (no pixel differs, and the caller does not rule it out) become 0; blockIdx.y: the plane
template <typename V>
__global__ __launch_bounds__(256) void stk_zero_kernel(V* __restrict__ ddem, const unsigned long long* __restrict__ cnt, const int32_t* __restrict__ can_equal,
                                                       int64_t n) {
    const int t = blockIdx.y;
    if (cnt[t] != 0ull || (can_equal && !can_equal[t])) return;
    V* out = ddem + (int64_t)t * n;
    for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < n; p += (int64_t)gridDim.x * 256) out[p] = (V)0;
}

// ---- 2. inlier statistics ---------------------------------------------------------------------------------------------------------------
// tab: [T] inliers | [T] smallest key of the reference over them (all ones: none) | [T] largest key (0: none)
template <typename V>
__global__ __launch_bounds__(256) void stk_stats_kernel(const V* __restrict__ ddem, const V* __restrict__ ref, const unsigned char* const* __restrict__ mask_tab,
                                                        int T, int64_t n, unsigned long long* tab) {
    __shared__ unsigned long long red[4];
    for (int c0 = 0; c0 < T; c0 += STK_CHUNK) {
        const int nc = T - c0 < STK_CHUNK ? T - c0 : STK_CHUNK;
        const unsigned char* mk[STK_CHUNK];
        unsigned long long inl[STK_CHUNK], lo[STK_CHUNK], hi[STK_CHUNK];
#pragma unroll
        for (int k = 0; k < STK_CHUNK; ++k) { mk[k] = mask_tab[c0 + (k < nc ? k : 0)]; inl[k] = 0ull; lo[k] = ~0ull; hi[k] = 0ull; }
        for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < n; p += (int64_t)gridDim.x * 256) {
            const V r = ref[p];
            if (!t_finite<V>(r)) continue;
            const unsigned long long key = (unsigned long long)key_of((double)r);
#pragma unroll
            for (int k = 0; k < STK_CHUNK; ++k) {
                if (k < nc && (!mk[k] || mk[k][p] != 0) && t_finite<V>(ddem[(int64_t)(c0 + k) * n + p])) {
                    ++inl[k];
                    lo[k] = key < lo[k] ? key : lo[k];
                    hi[k] = key > hi[k] ? key : hi[k];
                }
            }
        }
#pragma unroll
        for (int k = 0; k < STK_CHUNK; ++k) {
            if (k < nc) {
                const unsigned long long a = block_sum<unsigned long long>(inl[k], red), b = stk_block_min(lo[k], red), c = stk_block_max(hi[k], red);
                if (threadIdx.x == 0 && a) {
                    atomicAdd(&tab[c0 + k], a);
                    atomicMin(&tab[T + c0 + k], b);
                    atomicMax(&tab[2 * T + c0 + k], c);
                }
            }
        }
    }
}

// ---- 3. grouping --------------------------------------------------------------------------------------------------------------------------
// blockIdx.y: the plane.  edges: T rows of nb_max + 1, of which plane t uses nbs[t] + 1 (nbs[t] = 0: the plane is in no group).
template <typename V>
__global__ __launch_bounds__(256) void stk_group_kernel(const V* __restrict__ ddem, const V* __restrict__ ref, const unsigned char* const* __restrict__ mask_tab,
                                                        int64_t n, int nb_max, const int32_t* __restrict__ nbs, const double* __restrict__ edges, int use_lds,
                                                        unsigned long long* cnt, int32_t* __restrict__ grp) {
    extern __shared__ unsigned int stk_s_cnt[];
    const int t = blockIdx.y;
    const int nb = nbs[t];
    const double* __restrict__ e = edges + (int64_t)t * (nb_max + 1);
    const unsigned char* __restrict__ mk = mask_tab[t];
    const V* __restrict__ dd = ddem + (int64_t)t * n;
    int32_t* __restrict__ gp = grp + (int64_t)t * n;
    if (use_lds) {
        for (int g = threadIdx.x; g < nb_max; g += 256) stk_s_cnt[g] = 0u;
        __syncthreads();
    }
    for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < n; p += (int64_t)gridDim.x * 256) {
        int b = -1;
        if (nb > 0 && (!mk || mk[p] != 0)) {
            const V d = dd[p];
            const V r = ref[p];
            if (t_finite<V>(d) && t_finite<V>(r)) {
                const int i = hyp_count_le(e, nb + 1, (double)r);
                if (i >= 1 && i <= nb) b = i - 1;
            }
        }
        gp[p] = b < 0 ? -1 : t * nb_max + b;
        if (b >= 0) {
            if (use_lds) atomicAdd(&stk_s_cnt[b], 1u);
            else atomicAdd(&cnt[(int64_t)t * nb_max + b], 1ull);
        }
    }
    if (use_lds) {
        __syncthreads();
        for (int g = threadIdx.x; g < nb_max; g += 256)
            if (stk_s_cnt[g]) atomicAdd(&cnt[(int64_t)t * nb_max + g], (unsigned long long)stk_s_cnt[g]);
    }
}

// ---- 4. fused fill and series sums ------------------------------------------------------------------------------------------------------
// src: T plane pointers.  out (null: nothing is written, the values are those of src): T * n.  ms[t] >= 2: plane t has the model
// xs / ys[t * m_max ..] and its non-finite pixels inside its mask take (V)model(ref) -- mode 0 of hyp_fill_kernel with the value
// rounded to the reference's dtype, which is V.  series (null: the plane's own mask): the mask of the sums.
// part: one row of T sums per workgroup; cnt: [T] pixels of the series mask | [T] finite values among them.
template <typename V>
__global__ __launch_bounds__(256) void stk_fill_kernel(const V* const* __restrict__ src, const V* __restrict__ ref, const unsigned char* const* __restrict__ mask_tab,
                                                       const unsigned char* __restrict__ series, int T, int64_t n, int m_max, const int32_t* __restrict__ ms,
                                                       const double* __restrict__ xs, const double* __restrict__ ys, V* __restrict__ out,
                                                       double* __restrict__ part, unsigned long long* cnt) {
    __shared__ unsigned long long red[4];
    __shared__ double red_d[4];
    for (int c0 = 0; c0 < T; c0 += STK_CHUNK) {
        const int nc = T - c0 < STK_CHUNK ? T - c0 : STK_CHUNK;
        const V* pl[STK_CHUNK];
        const unsigned char* mk[STK_CHUNK];
        int mm[STK_CHUNK];
        double acc[STK_CHUNK];
        unsigned long long in_mask[STK_CHUNK], fin[STK_CHUNK];
#pragma unroll
        for (int k = 0; k < STK_CHUNK; ++k) {
            const int t = c0 + (k < nc ? k : 0);
            pl[k] = src[t]; mk[k] = mask_tab[t]; mm[k] = (out && ms) ? ms[t] : 0;
            acc[k] = 0.0; in_mask[k] = 0ull; fin[k] = 0ull;
        }
        for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < n; p += (int64_t)gridDim.x * 256) {
            const bool sm = series ? series[p] != 0 : true;
#pragma unroll
            for (int k = 0; k < STK_CHUNK; ++k) {
                if (k < nc) {
                    const bool own = !mk[k] || mk[k][p] != 0;
                    V v = pl[k][p];
                    if (out) {
                        if (own && mm[k] >= 2 && !t_finite<V>(v))
                            v = (V)hyp_interp1d(xs + (int64_t)(c0 + k) * m_max, ys + (int64_t)(c0 + k) * m_max, mm[k], (double)ref[p]);
                        out[(int64_t)(c0 + k) * n + p] = v;
                    }
                    if (series ? sm : own) {
                        ++in_mask[k];
                        if (t_finite<V>(v)) { ++fin[k]; acc[k] = acc[k] + (double)v; }
                    }
                }
            }
        }
#pragma unroll
        for (int k = 0; k < STK_CHUNK; ++k) {
            if (k < nc) {
                const double s = block_sum<double>(acc[k], red_d);
                const unsigned long long a = block_sum<unsigned long long>(in_mask[k], red), b = block_sum<unsigned long long>(fin[k], red);
                if (threadIdx.x == 0) {
                    part[(int64_t)blockIdx.x * T + c0 + k] = s;
                    if (a) atomicAdd(&cnt[c0 + k], a);
                    if (b) atomicAdd(&cnt[T + c0 + k], b);
                }
            }
        }
    }
}

// Where a pass writes its T planes: the caller's device array itself, or a buffer of the stack's behind a host array (copied out when the
// pass ends).  slot 1: the dDEMs, 2: the filled dDEMs; the slot's T entries of the pointer table follow.
int stk_place(xdemhip_stack* S, int slot, void* out, int memspace) {
    xdemhip_ctx* ctx = S->ctx;
    void*& buf = slot == 1 ? S->ddem : S->filled;
    void*& mine = S->out_buf[slot - 1];
    const size_t plane = (size_t)S->n * (S->f32 ? 4 : 8);
    XD_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    if (memspace == XDEMHIP_DEVICE) {
        S->mem.drop(mine);
        mine = nullptr;
        buf = out;
    } else {
        if (!mine) mine = S->mem.take(plane * S->T, "xdemhip_stack");
        buf = mine;
        { const int rc = S->mem.status(); if (rc) return rc; }
    }
    std::vector<const void*> tab((size_t)S->T);
    for (int t = 0; t < S->T; ++t) tab[t] = static_cast<const char*>(buf) + plane * t;
    XD_HIP_CHECK(ctx, hipMemcpyAsync(S->tabs + (size_t)slot * S->T, tab.data(), (size_t)S->T * sizeof(void*), hipMemcpyHostToDevice, ctx->stream));
    XD_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));   // (`tab` goes)
    return XDEMHIP_OK;
}
// the end of such a pass: a host array gets its copy; a device array is complete when the call returns
int stk_deliver(xdemhip_stack* S, int slot, void* out, int memspace) {
    xdemhip_ctx* ctx = S->ctx;
    if (memspace == XDEMHIP_HOST)
        XD_HIP_CHECK(ctx, hipMemcpyAsync(out, slot == 1 ? S->ddem : S->filled, (size_t)S->T * S->n * (S->f32 ? 4 : 8), hipMemcpyDeviceToHost, ctx->stream));
    return xd_sync(ctx);
}

int stk_series(xdemhip_stack* S, const void** src_tab, void* out, int m_max, const int32_t* d_ms, const double* d_xs, const double* d_ys,
               const unsigned char* d_series, XdBuffers& buf, int64_t* n_mask, int64_t* n_finite, double* sums) {
    xdemhip_ctx* ctx = S->ctx;
    const int T = S->T;
    const int64_t n = S->n;
    int rc = S->sums.reserve(S->mem, T, "xdemhip_stack");
    if (rc) return rc;
    unsigned long long* d_cnt = buf.alloc<unsigned long long>((size_t)2 * T);
    if (buf.rc) return buf.rc;
    if (hipMemsetAsync(d_cnt, 0, (size_t)2 * T * 8, ctx->stream) != hipSuccess) return xd_fail(ctx, XDEMHIP_EHIP, "hipMemsetAsync failed");
    const int nblocks = fixed_sums_grid(ctx, (n + 255) / 256);
    (void)hipEventRecord(ctx->ev_start, ctx->stream);
    if (S->f32)
        hipLaunchKernelGGL((stk_fill_kernel<float>), dim3(nblocks), dim3(256), 0, ctx->stream, reinterpret_cast<const float* const*>(src_tab),
                           static_cast<const float*>(S->ref), S->mask_tab, d_series, T, n, m_max, d_ms, d_xs, d_ys, static_cast<float*>(out), S->sums.part, d_cnt);
    else
        hipLaunchKernelGGL((stk_fill_kernel<double>), dim3(nblocks), dim3(256), 0, ctx->stream, reinterpret_cast<const double* const*>(src_tab),
                           static_cast<const double*>(S->ref), S->mask_tab, d_series, T, n, m_max, d_ms, d_xs, d_ys, static_cast<double*>(out), S->sums.part, d_cnt);
    rc = fixed_sums_reduce(ctx, S->sums.part, nblocks, T, "stk_fill_kernel");
    (void)hipEventRecord(ctx->ev_stop, ctx->stream);
    ctx->timed = rc == XDEMHIP_OK;
    if (rc) return rc;
    // the one fetch of the pass
    rc = xd_d2h(ctx, n_mask, d_cnt, (size_t)T * 8);
    if (rc == XDEMHIP_OK) rc = xd_d2h(ctx, n_finite, d_cnt + T, (size_t)T * 8);
    if (rc == XDEMHIP_OK) rc = xd_d2h(ctx, sums, S->sums.part + (int64_t)nblocks * T, (size_t)T * 8);
    return rc == XDEMHIP_OK ? xd_sync(ctx) : rc;
}

}  // namespace
}  // namespace xd

using namespace xd;

extern "C" {

int xdemhip_stack_create(xdemhip_ctx* ctx, const void* const* planes, int n_planes, int dtype, int64_t n, int ref_index, int memspace,
                         xdemhip_stack** out) {
    if (!ctx || !out) return XDEMHIP_EINVAL;
    *out = nullptr;
    if (!planes) return xd_fail(ctx, XDEMHIP_EINVAL, "null argument");
    if (n_planes < 1 || n_planes > STK_MAX_PLANES) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_stack_create: 1 to 1024 planes");
    if (ref_index < 0 || ref_index >= n_planes) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_stack_create: the reference must be one of the planes");
    if (dtype != XDEMHIP_F32 && dtype != XDEMHIP_F64) return xd_fail(ctx, XDEMHIP_EINVAL, "dtype must be float32 or float64");
    if (memspace != XDEMHIP_HOST && memspace != XDEMHIP_DEVICE) return xd_fail(ctx, XDEMHIP_EINVAL, "bad memspace");
    if (n < 1 || n >= ((int64_t)1 << 32)) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_stack_create: 1 to 2^32 - 1 pixels");
    for (int t = 0; t < n_planes; ++t)
        if (!planes[t]) return xd_fail(ctx, XDEMHIP_EINVAL, "null argument");
    XD_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    const int T = n_planes;
    const size_t es = dtype == XDEMHIP_F32 ? 4 : 8, plane = (size_t)n * es;
    xdemhip_stack* S = new xdemhip_stack;
    S->ctx = S->mem.ctx = ctx; S->f32 = dtype == XDEMHIP_F32; S->T = T; S->n = n; S->ref_index = ref_index;
    std::vector<const void*> tabs((size_t)3 * T, nullptr);
    std::vector<const unsigned char*> no_masks((size_t)T, nullptr);
    S->tabs = S->mem.take<const void*>((size_t)3 * T, "xdemhip_stack_create");
    S->mask_tab = S->mem.take<const unsigned char*>((size_t)T, "xdemhip_stack_create");
    if (memspace == XDEMHIP_HOST) S->upload = S->mem.take(plane * T, "xdemhip_stack_create");
    int rc = S->mem.rc;
    for (int t = 0; t < T && rc == XDEMHIP_OK; ++t) {
        if (memspace == XDEMHIP_DEVICE) tabs[t] = planes[t];
        else {
            tabs[t] = static_cast<const char*>(S->upload) + plane * t;
            if (hipMemcpyAsync(const_cast<void*>(tabs[t]), planes[t], plane, hipMemcpyHostToDevice, ctx->stream) != hipSuccess) rc = xd_fail(ctx, XDEMHIP_EHIP, "H2D copy failed");
        }
    }
    S->ref = tabs[ref_index];
    if (rc == XDEMHIP_OK && (hipMemcpyAsync(S->tabs, tabs.data(), (size_t)3 * T * sizeof(void*), hipMemcpyHostToDevice, ctx->stream) != hipSuccess ||
                             hipMemcpyAsync(S->mask_tab, no_masks.data(), (size_t)T * sizeof(void*), hipMemcpyHostToDevice, ctx->stream) != hipSuccess))
        rc = xd_fail(ctx, XDEMHIP_EHIP, "H2D copy failed");
    if (rc == XDEMHIP_OK) rc = xd_sync(ctx);   // (the caller's host arrays and the tables above may go once this returns)
    if (rc) { xdemhip_stack_destroy(S); return rc; }
    *out = S;
    return XDEMHIP_OK;
}

void xdemhip_stack_destroy(xdemhip_stack* S) { delete S; }   // (its owner frees the device buffers)

int xdemhip_stack_set_masks(xdemhip_stack* S, const unsigned char* const* masks, int n_masks, const int32_t* mask_id, int memspace) {
    if (!S) return XDEMHIP_EINVAL;
    xdemhip_ctx* ctx = S->ctx;
    if (n_masks < 0 || (n_masks > 0 && (!masks || !mask_id))) return xd_fail(ctx, XDEMHIP_EINVAL, "null argument");
    if (memspace != XDEMHIP_HOST && memspace != XDEMHIP_DEVICE) return xd_fail(ctx, XDEMHIP_EINVAL, "bad memspace");
    const int T = S->T;
    for (int t = 0; t < T && n_masks > 0; ++t)
        if (mask_id[t] < -1 || mask_id[t] >= n_masks) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_stack_set_masks: a mask id is -1 (every pixel) or the index of a mask");
    for (int k = 0; k < n_masks; ++k)
        if (!masks[k]) return xd_fail(ctx, XDEMHIP_EINVAL, "null argument");
    XD_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    XD_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    S->mem.drop(S->mask_upload);
    S->mask_upload = nullptr;
    if (memspace == XDEMHIP_HOST && n_masks > 0) {
        S->mask_upload = S->mem.take<unsigned char>((size_t)n_masks * S->n, "xdemhip_stack_set_masks");
        { const int rc = S->mem.status(); if (rc) return rc; }
        for (int k = 0; k < n_masks; ++k)
            XD_HIP_CHECK(ctx, hipMemcpyAsync(S->mask_upload + (size_t)k * S->n, masks[k], (size_t)S->n, hipMemcpyHostToDevice, ctx->stream));
    }
    std::vector<const unsigned char*> tab((size_t)T, nullptr);
    for (int t = 0; t < T && n_masks > 0; ++t)
        if (mask_id[t] >= 0) tab[t] = memspace == XDEMHIP_HOST ? S->mask_upload + (size_t)mask_id[t] * S->n : masks[mask_id[t]];
    XD_HIP_CHECK(ctx, hipMemcpyAsync(S->mask_tab, tab.data(), (size_t)T * sizeof(void*), hipMemcpyHostToDevice, ctx->stream));
    S->K = n_masks;
    return xd_sync(ctx);
}

int xdemhip_stack_subtract(xdemhip_stack* S, const int32_t* can_equal, void* out, int memspace, int64_t* n_differ, int64_t* n_nonfinite) {
    XdFetchScope fetch_scope_(S ? S->ctx : nullptr);
    if (!S) return XDEMHIP_EINVAL;
    xdemhip_ctx* ctx = S->ctx;
    if (!out || !n_differ || !n_nonfinite) return xd_fail(ctx, XDEMHIP_EINVAL, "null argument");
    if (memspace != XDEMHIP_HOST && memspace != XDEMHIP_DEVICE) return xd_fail(ctx, XDEMHIP_EINVAL, "bad memspace");
    XD_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    const int T = S->T;
    const int64_t n = S->n;
    S->subtracted = false;
    S->has_filled = false;
    { const int rc_ = stk_place(S, 1, out, memspace); if (rc_) return rc_; }
    XdBuffers buf(ctx, "xdemhip_stack_subtract");
    unsigned long long* d_cnt = buf.alloc<unsigned long long>((size_t)2 * T);
    const int32_t* d_can = buf.input(can_equal, (size_t)T * 4, XDEMHIP_HOST);
    if (buf.rc) return buf.rc;
    if (hipMemsetAsync(d_cnt, 0, (size_t)2 * T * 8, ctx->stream) != hipSuccess) return xd_fail(ctx, XDEMHIP_EHIP, "hipMemsetAsync failed");
    const int g = grid_for(ctx, n, 256, 16);
    (void)hipEventRecord(ctx->ev_start, ctx->stream);
    if (S->f32) {
        hipLaunchKernelGGL((stk_subtract_kernel<float>), dim3(g), dim3(256), 0, ctx->stream, reinterpret_cast<const float* const*>(S->tabs), S->ref_index, T, n,
                           static_cast<float*>(S->ddem), d_cnt);
        hipLaunchKernelGGL((stk_zero_kernel<float>), dim3(g, T), dim3(256), 0, ctx->stream, static_cast<float*>(S->ddem), d_cnt, d_can, n);
    } else {
        hipLaunchKernelGGL((stk_subtract_kernel<double>), dim3(g), dim3(256), 0, ctx->stream, reinterpret_cast<const double* const*>(S->tabs), S->ref_index, T, n,
                           static_cast<double*>(S->ddem), d_cnt);
        hipLaunchKernelGGL((stk_zero_kernel<double>), dim3(g, T), dim3(256), 0, ctx->stream, static_cast<double*>(S->ddem), d_cnt, d_can, n);
    }
    (void)hipEventRecord(ctx->ev_stop, ctx->stream);
    ctx->timed = true;
    int rc = launched(ctx, "stk_subtract_kernel");
    if (rc == XDEMHIP_OK) rc = xd_d2h(ctx, n_differ, d_cnt, (size_t)T * 8);
    if (rc == XDEMHIP_OK) rc = xd_d2h(ctx, n_nonfinite, d_cnt + T, (size_t)T * 8);
    if (rc == XDEMHIP_OK) rc = xd_sync(ctx);
    if (rc) return rc;
    for (int t = 0; t < T; ++t)
        if (n_differ[t] == 0 && (!can_equal || can_equal[t])) n_nonfinite[t] = 0;   // (zeroed)
    rc = stk_deliver(S, 1, out, memspace);
    if (rc) return rc;
    S->subtracted = true;
    return buf.finish();
}

int xdemhip_stack_stats(xdemhip_stack* S, int64_t* inliers, double* ref_min, double* ref_max) {
    XdFetchScope fetch_scope_(S ? S->ctx : nullptr);
    if (!S) return XDEMHIP_EINVAL;
    xdemhip_ctx* ctx = S->ctx;
    if (!inliers || !ref_min || !ref_max) return xd_fail(ctx, XDEMHIP_EINVAL, "null argument");
    if (!S->subtracted) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_stack: no xdemhip_stack_subtract call yet");
    XD_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    const int T = S->T;
    const int64_t n = S->n;
    std::vector<unsigned long long> tab((size_t)3 * T);   // (a copy's destination: declared before the buffers)
    XdBuffers buf(ctx, "xdemhip_stack_stats");
    unsigned long long* d_tab = buf.alloc<unsigned long long>((size_t)3 * T);
    if (buf.rc) return buf.rc;
    if (hipMemsetAsync(d_tab, 0, (size_t)3 * T * 8, ctx->stream) != hipSuccess || hipMemsetAsync(d_tab + T, 0xFF, (size_t)T * 8, ctx->stream) != hipSuccess)
        return xd_fail(ctx, XDEMHIP_EHIP, "hipMemsetAsync failed");
    const int g = grid_for(ctx, n, 256, 16);
    if (S->f32)
        hipLaunchKernelGGL((stk_stats_kernel<float>), dim3(g), dim3(256), 0, ctx->stream, static_cast<const float*>(S->ddem), static_cast<const float*>(S->ref), S->mask_tab, T, n, d_tab);
    else
        hipLaunchKernelGGL((stk_stats_kernel<double>), dim3(g), dim3(256), 0, ctx->stream, static_cast<const double*>(S->ddem), static_cast<const double*>(S->ref), S->mask_tab, T, n, d_tab);
    int rc = launched(ctx, "stk_stats_kernel");
    if (rc == XDEMHIP_OK) rc = xd_d2h(ctx, tab.data(), d_tab, (size_t)3 * T * 8);
    if (rc == XDEMHIP_OK) rc = xd_sync(ctx);
    if (rc) return rc;
    for (int t = 0; t < T; ++t) {
        inliers[t] = (int64_t)tab[t];
        ref_min[t] = tab[t] ? val_of((uint64_t)tab[T + t]) : (double)NAN;
        ref_max[t] = tab[t] ? val_of((uint64_t)tab[2 * T + t]) : (double)NAN;
    }
    return buf.finish();
}

int xdemhip_stack_segments(xdemhip_stack* S, int nb_max, const int32_t* nbs, const double* edges, int64_t* counts, double* medians) {
    XdFetchScope fetch_scope_(S ? S->ctx : nullptr);
    if (!S) return XDEMHIP_EINVAL;
    xdemhip_ctx* ctx = S->ctx;
    if (!nbs || !edges || !counts || !medians) return xd_fail(ctx, XDEMHIP_EINVAL, "null argument");
    if (!S->subtracted) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_stack: no xdemhip_stack_subtract call yet");
    const int T = S->T;
    const int64_t n = S->n;
    if (nb_max < 1 || (int64_t)T * (nb_max + 1) >= ((int64_t)1 << 31)) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_stack_segments: at least one bin, fewer than 2^31 groups");
    for (int t = 0; t < T; ++t)
        if (nbs[t] < 0 || nbs[t] > nb_max) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_stack_segments: a plane has 0 to nb_max bins");
    XD_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    const int n_groups = T * nb_max;
    const size_t es = S->f32 ? 4 : 8;
    if (!S->grp) S->grp = S->mem.take<int32_t>((size_t)T * n, "xdemhip_stack_segments");
    { const int rc_ = S->mem.status(); if (rc_) return rc_; }
    unsigned long long total = 0;   // (a copy's destination: declared before the buffers)
    XdBuffers buf(ctx, "xdemhip_stack_segments");
    const int32_t* d_nbs = buf.input(nbs, (size_t)T * 4, XDEMHIP_HOST);
    const double* d_edges = buf.input(edges, (size_t)T * (nb_max + 1) * 8, XDEMHIP_HOST);
    unsigned long long* off = buf.alloc<unsigned long long>((size_t)n_groups + 1);
    unsigned long long* cursor = buf.alloc<unsigned long long>((size_t)n_groups);
    int64_t* d_counts = buf.output(counts, (size_t)n_groups * 8, XDEMHIP_HOST);
    double* d_med = buf.output(medians, (size_t)n_groups * 8, XDEMHIP_HOST);
    if (buf.rc) return buf.rc;
    if (hipMemsetAsync(off, 0, ((size_t)n_groups + 1) * 8, ctx->stream) != hipSuccess) return xd_fail(ctx, XDEMHIP_EHIP, "hipMemsetAsync failed");
    const dim3 g2(grid_for(ctx, n, 256, 16), T);
    const int use_lds = nb_max <= STK_LDS_BINS;
    const size_t lds_cnt = use_lds ? (size_t)nb_max * 4 : 0;
    if (S->f32)
        hipLaunchKernelGGL((stk_group_kernel<float>), g2, dim3(256), lds_cnt, ctx->stream, static_cast<const float*>(S->ddem), static_cast<const float*>(S->ref), S->mask_tab, n,
                           nb_max, d_nbs, d_edges, use_lds, off, S->grp);
    else
        hipLaunchKernelGGL((stk_group_kernel<double>), g2, dim3(256), lds_cnt, ctx->stream, static_cast<const double*>(S->ddem), static_cast<const double*>(S->ref), S->mask_tab, n,
                           nb_max, d_nbs, d_edges, use_lds, off, S->grp);
    hipLaunchKernelGGL(rank_scan_kernel, dim3(1), dim3(1024), 0, ctx->stream, off, (int64_t)n_groups, off + n_groups);
    int rc = launched(ctx, "stk_group_kernel");
    if (rc == XDEMHIP_OK && hipMemcpyAsync(cursor, off, (size_t)n_groups * 8, hipMemcpyDeviceToDevice, ctx->stream) != hipSuccess)
        rc = xd_fail(ctx, XDEMHIP_EHIP, "device copy failed");
    if (rc == XDEMHIP_OK && hipMemcpyAsync(&total, off + n_groups, 8, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess) rc = xd_fail(ctx, XDEMHIP_EHIP, "D2H copy failed");
    if (rc == XDEMHIP_OK) rc = xd_sync(ctx);
    if (rc) return rc;
    if ((int64_t)total > (int64_t)T * n) return xd_fail(ctx, XDEMHIP_EHIP, "xdemhip_stack_segments: more grouped values than pixels");
    void* seg = buf.alloc((size_t)(total ? total : 1) * es);
    if (buf.rc) return buf.rc;
    // the T * n values of the stack are one long raster to the counting sort and the segment statistics of volume.h; segments
    // longer than the switch's value leave the LDS route (include/xdemhip_test.h: "hypso_seg_lds")
    const int64_t n_all = (int64_t)T * n;
    const dim3 g(grid_for(ctx, n_all, 256, 16));
    const int cap = ctx->hypso_seg_lds ? ctx->hypso_seg_lds : HYP_SEG_LDS;
    const size_t lds_seg = (size_t)cap * es;
    const int seg_blocks = n_groups < ctx->num_cu * 8 ? n_groups : ctx->num_cu * 8;
    if (S->f32) {
        if (total) hipLaunchKernelGGL((hyp_scatter_kernel<float>), g, dim3(256), 0, ctx->stream, static_cast<const float*>(S->ddem), S->grp, n_all, cursor, static_cast<float*>(seg));
        rc = set_big_lds(ctx, hyp_segment_kernel<float>, lds_seg);
        if (rc == XDEMHIP_OK)
            hipLaunchKernelGGL((hyp_segment_kernel<float>), dim3(seg_blocks), dim3(256), lds_seg, ctx->stream, static_cast<float*>(seg), off, n_groups, cap, 0, d_counts, d_med,
                               static_cast<double*>(nullptr));
    } else {
        if (total) hipLaunchKernelGGL((hyp_scatter_kernel<double>), g, dim3(256), 0, ctx->stream, static_cast<const double*>(S->ddem), S->grp, n_all, cursor, static_cast<double*>(seg));
        rc = set_big_lds(ctx, hyp_segment_kernel<double>, lds_seg);
        if (rc == XDEMHIP_OK)
            hipLaunchKernelGGL((hyp_segment_kernel<double>), dim3(seg_blocks), dim3(256), lds_seg, ctx->stream, static_cast<double*>(seg), off, n_groups, cap, 0, d_counts, d_med,
                               static_cast<double*>(nullptr));
    }
    if (rc == XDEMHIP_OK) rc = launched(ctx, "hyp_segment_kernel");
    if (rc) return rc;
    return buf.finish();
}

int xdemhip_stack_fill(xdemhip_stack* S, int m_max, const int32_t* ms, const double* xs, const double* ys, void* out, int memspace, int64_t* n_mask,
                       int64_t* n_finite, double* sums) {
    XdFetchScope fetch_scope_(S ? S->ctx : nullptr);
    if (!S) return XDEMHIP_EINVAL;
    xdemhip_ctx* ctx = S->ctx;
    if (!ms || !xs || !ys || !out || !n_mask || !n_finite || !sums) return xd_fail(ctx, XDEMHIP_EINVAL, "null argument");
    if (memspace != XDEMHIP_HOST && memspace != XDEMHIP_DEVICE) return xd_fail(ctx, XDEMHIP_EINVAL, "bad memspace");
    if (!S->subtracted) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_stack: no xdemhip_stack_subtract call yet");
    const int T = S->T;
    if (m_max < 2 || (int64_t)T * m_max >= ((int64_t)1 << 31)) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_stack_fill: a model needs at least 2 points");
    for (int t = 0; t < T; ++t)
        if (ms[t] != 0 && (ms[t] < 2 || ms[t] > m_max)) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_stack_fill: a plane has no model (0) or one of 2 to m_max points");
    XD_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    S->has_filled = false;
    { const int rc_ = stk_place(S, 2, out, memspace); if (rc_) return rc_; }
    XdBuffers buf(ctx, "xdemhip_stack_fill");
    const int32_t* d_ms = buf.input(ms, (size_t)T * 4, XDEMHIP_HOST);
    const double* d_xs = buf.input(xs, (size_t)T * m_max * 8, XDEMHIP_HOST);
    const double* d_ys = buf.input(ys, (size_t)T * m_max * 8, XDEMHIP_HOST);
    if (buf.rc) return buf.rc;
    int rc = stk_series(S, S->tabs + T, S->filled, m_max, d_ms, d_xs, d_ys, nullptr, buf, n_mask, n_finite, sums);
    if (rc == XDEMHIP_OK) rc = stk_deliver(S, 2, out, memspace);
    if (rc) return rc;
    S->has_filled = true;
    return buf.finish();
}

int xdemhip_stack_series(xdemhip_stack* S, int which, const unsigned char* mask, int memspace, int64_t* n_mask, int64_t* n_finite, double* sums) {
    XdFetchScope fetch_scope_(S ? S->ctx : nullptr);
    if (!S) return XDEMHIP_EINVAL;
    xdemhip_ctx* ctx = S->ctx;
    if (!n_mask || !n_finite || !sums) return xd_fail(ctx, XDEMHIP_EINVAL, "null argument");
    if (memspace != XDEMHIP_HOST && memspace != XDEMHIP_DEVICE) return xd_fail(ctx, XDEMHIP_EINVAL, "bad memspace");
    if (which < 0 || which > 2) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_stack_series: 0 the input planes, 1 the dDEMs, 2 the filled dDEMs");
    if ((which == 1 && !S->subtracted) || (which == 2 && !S->has_filled)) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_stack_series: these planes have not been computed");
    XD_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    XdBuffers buf(ctx, "xdemhip_stack_series");
    const unsigned char* d_mask = buf.input(mask, (size_t)S->n, memspace);
    if (buf.rc) return buf.rc;
    int rc = stk_series(S, S->tabs + (size_t)which * S->T, nullptr, 0, nullptr, nullptr, nullptr, d_mask, buf, n_mask, n_finite, sums);
    if (rc) return rc;
    return buf.finish();
}

}  // extern "C"
