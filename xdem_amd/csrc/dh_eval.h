// dh_eval.h -- median and NMAD of one dh column on the device with ONE fetch: what the shifted-dh evaluations of the dh plan
// (biascorr.hip: xdemhip_dh_shift_nmad) and of the raster-point plan (ptsplan.hip) share.  The caller's own kernel writes dh into a
// staging buffer -- and, on the plain route, counts the leading key digit on the side (dh_hist_count / dh_hist_flush) -- the selections
// of select_run.h read that buffer, and their results are decoded by a kernel, so that the second selection (|dh - median|) can
// depend on the first without a host round trip.
#pragma once
#include "common.h"
#include "select.h"
#include "select_run.h"

namespace xd {

// leading-digit counters of a workgroup: DH_HIST_COPIES privatised tables (copy = lane % copies, an odd stride apart: float keys
// share their sign and exponent bits, every lane of a wave would otherwise hit one counter), flushed with one global add per
// non-empty counter
constexpr int DH_HIST_COPIES = 16, DH_HIST_STRIDE = SEL_RADIX + 1;
template <typename T> __device__ __forceinline__ void dh_hist_count(uint32_t* hc, T v) {
    if (v == v) atomicAdd(&hc[(int)(key_of(v) >> (8 * (KeyT<T>::passes - 1)))], 1u);
}
__device__ __forceinline__ void dh_hist_flush(const uint32_t* h, uint64_t* __restrict__ hist) {
    __syncthreads();
    for (int k = threadIdx.x; k < SEL_RADIX; k += blockDim.x) {
        unsigned long long c = 0;
        for (int q = 0; q < DH_HIST_COPIES; ++q) c += h[q * DH_HIST_STRIDE + k];
        if (c) atomicAdd(reinterpret_cast<unsigned long long*>(&hist[k]), c);
    }
}

__device__ __forceinline__ float dh_abs(float v) { return fabsf(v); }
__device__ __forceinline__ double dh_abs(double v) { return fabs(v); }

// |dh - median| of the staging buffer as an element source of the bracketed selection (select_run.h): nothing is materialised
template <typename T> struct AbsDevSource {
    const T* vals;
    const T* med;    // device slot the first selection's finish kernel wrote
    T m;
    struct Raw { T v; };
    struct Acc {};
    static size_t lds_bytes(int) { return 0; }
    __device__ __forceinline__ void setup(unsigned char*, int) { m = *med; }
    __device__ __forceinline__ void fetch(int64_t p, Raw& r) const { r.v = vals[p]; }
    __device__ __forceinline__ void blank(Raw& r) const { r.v = (T)NAN; }
    template <bool ACC> __device__ __forceinline__ bool eval(const Raw& r, int, T& v, uint16_t& b, Acc&) const {
        v = dh_abs(t_sub(r.v, m));
        b = 0;
        return v == v;
    }
    __device__ __forceinline__ void finish(Acc&) const {}
    static constexpr bool HAS_LEAN = false;
};
// the same in place, for the plain digit passes (they read an array)
template <typename T>
__global__ __launch_bounds__(256) void dh_absdev_kernel(T* __restrict__ stage, int64_t n, const T* __restrict__ med) {
    const T m = *med;
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (int64_t)gridDim.x * blockDim.x) stage[p] = dh_abs(t_sub(stage[p], m));
}

// What one evaluation hands back (a block behind the selection scratch): filled by the two finish kernels, fetched once.
struct DhEvalOut {
    double median, mad;             // in the value dtype, widened
    unsigned long long count, fail; // values that are not NaN; a bracket of either selection missed or a candidate buffer overflowed
    double slot;                    // the median in the value dtype: what the second selection subtracts
};
// np.nanmedian from a finished selection, on the device (median_from's rule).  `small` = the workspace block of a bracketed selection
// (select_bracketed_enqueue: flags, rebase shift, low key, counters), nullptr after the plain passes.
template <typename T>
__global__ void dh_sel_finish_kernel(const SelState<typename KeyT<T>::type>* st, const uint64_t* succ, const uint64_t* small, int nb_max, int which,
                                     DhEvalOut* out) {
    typedef typename KeyT<T>::type K;
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    SelState<K> s = st[0];
    uint64_t sc = succ[0];
    if (small) {
        if (small[2] != 0 || small[3] != 0) out->fail = 1ull;
        const int rbs = (int)(uint32_t)small[4];
        const K klo = reinterpret_cast<const K*>(small + 8)[0];
        const uint64_t* cnt = small + 8 + 3 * nb_max;
        s.count = cnt[0];
        s.n_le += cnt[1];
        s.prefix = (K)((K)(s.prefix >> rbs) + klo);
        if (sc != ~(uint64_t)0) sc = (uint64_t)(K)((K)((K)sc >> rbs) + klo);
    }
    T m = (T)NAN;
    if (s.count) {
        const T lo = val_of(s.prefix);
        if (s.count & 1) m = lo;
        else {
            const T hi = (s.n_le > s.count / 2) ? lo : val_of((K)sc);
            m = (T)((T)(lo + hi) / (T)2);
        }
    }
    if (which == 0) {
        out->median = (double)m;
        out->count = s.count;
        *reinterpret_cast<T*>(&out->slot) = m;
    } else {
        out->mad = (double)m;
    }
}

// The data pass and the median's selection of one evaluation, queued without a host synchronisation.  `launch(with_hist, hist)` is the
// caller's pass: it writes dh of the n selected elements into `stage` (NaN where there is none) and, with_hist, adds the leading
// digit's counts to `hist`.  `plain`: the digit passes; otherwise the bracketed route where it applies (n >= SEL_BRACKET_MIN_N and a
// workspace).  On return d_out holds the median, the count and the slot (and `fail` if a bracket missed).  `scratch`: scratch_size(1)
// bytes and more; `ws`: the owner's workspace (may be empty).
template <typename T, typename Launch>
int dh_median_enqueue(xdemhip_ctx* ctx, T* stage, int64_t n, unsigned char* scratch, SelWorkspace* ws, bool plain, Launch&& launch,
                      DhEvalOut* d_out) {
    typedef typename KeyT<T>::type K;
    const SelState<K>* d_st = reinterpret_cast<const SelState<K>*>(scratch + OFF_STATE);
    const uint64_t* d_succ = reinterpret_cast<const uint64_t*>(scratch + off_succ(1));
    XD_HIP_CHECK(ctx, hipMemsetAsync(d_out, 0, sizeof(DhEvalOut), ctx->stream));
    bool queued = false;
    int rc;
    if (plain) {
        uint64_t* hist = select_reset<K>(ctx, scratch, 1);
        rc = launch(true, hist);
        if (rc == XDEMHIP_OK) rc = select_enqueue<T>(ctx, stage, nullptr, n, n, nullptr, 1, scratch, SEL_MEDIAN, nullptr, 0, true, nullptr, nullptr, true);
    } else {
        rc = launch(false, (uint64_t*)nullptr);
        if (rc == XDEMHIP_OK) rc = select_bracketed_enqueue<T, ArraySource<T>>(ctx, ArraySource<T>{stage, nullptr}, n, 1, scratch, ws, &queued);
        if (rc == XDEMHIP_OK && !queued) rc = select_enqueue<T>(ctx, stage, nullptr, n, n, nullptr, 1, scratch, SEL_MEDIAN, nullptr);
    }
    if (rc) return rc;
    hipLaunchKernelGGL((dh_sel_finish_kernel<T>), dim3(1), dim3(1), 0, ctx->stream, d_st, d_succ, queued ? ws->d_small : (const uint64_t*)nullptr,
                       ws->nb_max, 0, d_out);
    return launched(ctx, "dh selection kernel");
}

// One evaluation: the data pass, the median's selection, |dh - median|'s selection, ONE fetch.  Inputs of SEL_BRACKET_MIN_N values
// and more take the bracketed route of select_run.h for both selections (a sample, one counting pass, the candidates) with the
// decoding done by dh_sel_finish_kernel; should a bracket miss -- the integer counts of the counting pass tell -- the evaluation is
// run again with the plain digit passes, which cannot miss.  Nothing is allocated here.  `scratch` holds scratch_size(1) bytes and a
// DhEvalOut behind them.
template <typename T, typename Launch>
int dh_eval_median_nmad(xdemhip_ctx* ctx, T* stage, int64_t n, unsigned char* scratch, SelWorkspace* ws, double nfact, Launch&& launch,
                        double* median, double* nmad, int64_t* count) {
    typedef typename KeyT<T>::type K;
    DhEvalOut* d_out = reinterpret_cast<DhEvalOut*>(scratch + scratch_size(1));
    const SelState<K>* d_st = reinterpret_cast<const SelState<K>*>(scratch + OFF_STATE);
    const uint64_t* d_succ = reinterpret_cast<const uint64_t*>(scratch + off_succ(1));
    const T* d_med = reinterpret_cast<const T*>(&d_out->slot);
    DhEvalOut h;
    for (int attempt = 0; attempt < 2; ++attempt) {
        const bool plain = attempt == 1 || n < SEL_BRACKET_MIN_N;
        int rc = dh_median_enqueue<T>(ctx, stage, n, scratch, ws, plain, launch, d_out);
        if (rc) return rc;
        bool queued2 = false;
        if (!plain) rc = select_bracketed_enqueue<T, AbsDevSource<T>>(ctx, AbsDevSource<T>{stage, d_med, (T)0}, n, 1, scratch, ws, &queued2);
        if (rc == XDEMHIP_OK && !queued2) {
            hipLaunchKernelGGL((dh_absdev_kernel<T>), dim3(grid_for(ctx, n, 256, 16)), dim3(256), 0, ctx->stream, stage, n, d_med);
            rc = select_enqueue<T>(ctx, stage, nullptr, n, n, nullptr, 1, scratch, SEL_MEDIAN, nullptr);
        }
        if (rc) return rc;
        hipLaunchKernelGGL((dh_sel_finish_kernel<T>), dim3(1), dim3(1), 0, ctx->stream, d_st, d_succ, queued2 ? ws->d_small : (const uint64_t*)nullptr,
                           ws->nb_max, 1, d_out);
        if (launched(ctx, "dh selection kernel")) return XDEMHIP_EHIP;
        rc = xd_d2h(ctx, &h, d_out, sizeof h);
        if (rc == XDEMHIP_OK) rc = xd_sync(ctx);
        if (rc) return rc;
        if (!h.fail) break;
    }
    *count = (int64_t)h.count;
    if (h.count == 0) return xd_fail(ctx, XDEMHIP_EINVAL, "no valid points");
    *median = h.median;
    *nmad = (double)(T)((T)nfact * (T)h.mad);   // nfact * np.nanmedian(...): the Python float is a weak scalar (xdemhip_nmad's rule)
    return XDEMHIP_OK;
}

}  // namespace xd
