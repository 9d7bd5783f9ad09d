// rasterstats.hip -- the statistics of one raster in a handful of passes (xdemhip_raster_stats): what geoutils' Raster.get_stats
// computes on the host with several full sorts -- count, min, max, sum, sum of squares, sum of squared deviations, the median, up to
// four percentiles and the NMAD -- from fused passes and the multi-rank exact selection of multi_select.h.
//
// A pixel is VALID when its value is finite, differs from `nodata` (when given; rounded to the value dtype first) and both byte masks
// (when given) are non-zero.
// Round 1 selects the two median ranks and two ranks per quantile of the valid values v; round 2 the two median ranks of
// |v - median| (formed in the value dtype).  Routes, by the context's "selection" option:
//   plain (1; and what the others fall back to): the first digit's histogram comes out of the statistics pass itself (round 1: count,
//     min, max, sum v, sum v^2; round 2: sum (v - mean)^2), the other digits take one pass over the raster each: 4 + 4 reads of a
//     float32 raster, 8 + 8 of a float64 one.  Nothing is materialised: round 2 forms |v - median| on the fly in every pass.
//   bracketed (0 for n >= SEL_BRACKET_MIN_N; 2, 3 at every size): per round a 1/64 line sample (sample_lines_kernel), the ends of one
//     bracket per wanted pair of ranks selected from it (both ends of every bracket in ONE multi-rank selection, 3 leading digits),
//     then ONE pass over the raster -- the same statistics pass -- that counts per bracket the elements below and inside it and
//     compacts the union of the brackets; the wanted ranks, moved by the counted offsets, are selected among the candidates.  A rank
//     outside its bracket or a full candidate buffer -> the plain route for that round (2: brackets collapsed to one key, so that
//     this happens).
// The sums are float64 added in one fixed order -- a lane its own elements in loop order, xor shuffles over the wave, the 16 waves of
// the workgroup in order, one partial per workgroup, lane l of the reduce kernel the partials l, l + 256, ..., a halving tree -- on a
// grid that depends on the device and n only; the statistics pass is one kernel body for both routes: same bits from every route.
// The ranks are fixed on the device (ms_rank, from the count the first histogram gives); the host synchronises once at the end on the
// plain route, once per round on the bracketed one (to learn whether the brackets held).
#include <math.h>
#include <stddef.h>
#include <string.h>

#include "common.h"
#include "fixed_sums.h"
#include "multi_select.h"

namespace xd {

constexpr int RS_MAXB = 5;   // brackets of a round: the median's and one per quantile
constexpr int RS_NT = 2;     // float64 sums of a round

template <typename T> struct RsParams { double mean; T med; T pad; };

template <typename T> __device__ __forceinline__ T t_abs(T d) { return d < (T)0 ? -d : d; }

// The valid values of the raster as an element source (select_run.h).  round 2: |v - median| with the median read from the device.
template <typename T> struct RsSource {
    const T* vals;
    const uint8_t* tmask;
    const uint8_t* inl;
    const RsParams<T>* par;
    T nodata;
    int has_nodata, round;
    T med;   // (setup)
    struct Raw { T v; uint8_t m; };
    struct Acc {};
    static size_t lds_bytes(int) { return 0; }
    __device__ __forceinline__ void setup(unsigned char*, int) { med = round == 2 ? par->med : (T)0; }
    __device__ __forceinline__ void fetch(int64_t p, Raw& r) const {
        r.v = vals[p];
        r.m = (uint8_t)(((!tmask || tmask[p]) ? 1 : 0) | ((!inl || inl[p]) ? 2 : 0));
    }
    __device__ __forceinline__ void blank(Raw& r) const { r.v = (T)NAN; r.m = 0; }
    __device__ __forceinline__ bool value_ok(const Raw& r) const { return (r.m & 1) && t_finite<T>(r.v) && !(has_nodata && r.v == nodata); }
    template <bool ACC> __device__ __forceinline__ bool eval(const Raw& r, int, T& v, uint16_t& b, Acc&) const {
        b = 0;
        if (!(r.m & 2) || !value_ok(r)) return false;
        v = round == 2 ? t_abs<T>(t_sub<T>(r.v, med)) : r.v;
        return true;
    }
    __device__ __forceinline__ void finish(Acc&) const {}
    static constexpr bool HAS_LEAN = false;
};

// what one round leaves on the device
template <typename K> struct RsRound {
    uint64_t icnt[4];             // valid (and inlier) pixels, valid pixels whatever the inlier mask, inlier pixels
    K kext[2];                    // max of ~key (= ~min key), max key
    K kpad[2];
    double totals[RS_NT];
    unsigned long long ctr[4];    // sample count, candidate count, overflow, a rank outside its bracket
    K klo[RS_MAXB + 1], khi[RS_MAXB + 1];
    uint64_t bcnt[3][RS_MAXB];    // per bracket: elements below it, elements inside it, CANDIDATES (elements of any bracket) below it
    uint64_t given[MS_MAX];
    MsTable<K> tab_s, tab;        // the sample's selection (bracket ends), the final one
};
template <typename T> struct RsCtrl {
    RsRound<typename KeyT<T>::type> r[2];
    RsParams<T> par;
    uint64_t hist[8 * MS_MAX * SEL_RADIX];   // (fetched up to here)
};

template <typename V> __device__ __forceinline__ V wave_max_u(V x);
template <> __device__ __forceinline__ uint32_t wave_max_u<uint32_t>(uint32_t x) {
    for (int off = 32; off > 0; off >>= 1) { const uint32_t o = (uint32_t)__shfl_xor((int)x, off, 64); x = o > x ? o : x; }
    return x;
}
template <> __device__ __forceinline__ uint64_t wave_max_u<uint64_t>(uint64_t x) {
    for (int off = 32; off > 0; off >>= 1) { const uint64_t o = (uint64_t)__shfl_xor((unsigned long long)x, off, 64); x = o > x ? o : x; }
    return x;
}
__device__ __forceinline__ uint32_t wave_add_u32(uint32_t x) {
    for (int off = 32; off > 0; off >>= 1) x += (uint32_t)__shfl_xor((int)x, off, 64);
    return x;
}

// The statistics pass of a round.  BR = false: + the first digit's histogram (32 privatised tables).  BR = true: + the counters of NBR
// brackets (1: round 2's; RS_MAXB: unused ones are empty) and the compaction of the candidates (BlockStage, select_run.h).  The float64
// sums do not depend on BR.
template <typename T, bool BR, int NBR>
__global__ __launch_bounds__(HIST_THREADS) void rs_data_pass_kernel(RsSource<T> src, int64_t n, RsRound<typename KeyT<T>::type>* R, double* __restrict__ part,
                                                                    uint64_t* hist, int nbr, T* out_v, uint16_t* out_b, int64_t cap) {
    typedef typename KeyT<T>::type K;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ double s_red[RS_NT][HIST_THREADS / 64];
    __shared__ uint32_t s_cnt[3 + 3 * RS_MAXB];
    __shared__ K s_ext[2];
    constexpr int COPIES = 32, CSTRIDE = SEL_RADIX + 1;
    uint32_t* h = reinterpret_cast<uint32_t*>(smem);
    BlockStage<T> st;
    K lo[NBR], hi[NBR];
    if (BR) {
        st.v = reinterpret_cast<T*>(smem);
        st.b = reinterpret_cast<uint16_t*>(st.v + SEL_STAGE_CAP);
        st.base = reinterpret_cast<unsigned long long*>(st.b + SEL_STAGE_CAP);
        st.held = reinterpret_cast<int*>(st.base + 1);
        if (threadIdx.x == 0) *st.held = 0;
#pragma unroll
        for (int b = 0; b < NBR; ++b) { lo[b] = b < nbr ? R->klo[b] : (K)1; hi[b] = b < nbr ? R->khi[b] : (K)0; }   // (unused: empty)
    } else {
        for (int k = threadIdx.x; k < CSTRIDE * COPIES; k += blockDim.x) h[k] = 0;
    }
    if (threadIdx.x < 3 + 3 * RS_MAXB) s_cnt[threadIdx.x] = 0;
    if (threadIdx.x < 2) s_ext[threadIdx.x] = 0;
    src.setup(nullptr, 1);
    const double mean = src.round == 2 ? src.par->mean : 0.0;
    __syncthreads();
    uint32_t* hc = h + (threadIdx.x % COPIES) * CSTRIDE;
    const int top = 8 * (KeyT<T>::passes - 1);
    double s0 = 0.0, s1 = 0.0;
    uint32_t c_n = 0, c_all = 0, c_inl = 0;
    uint32_t cb[3][NBR];
#pragma unroll
    for (int b = 0; b < NBR; ++b) cb[0][b] = cb[1][b] = cb[2][b] = 0;
    K e_min = 0, e_max = 0;
    int it = 0;
    const int64_t step = (int64_t)blockDim.x * SEL_TILE;
    for (int64_t base = (int64_t)blockIdx.x * step; base < n; base += (int64_t)gridDim.x * step) {
        typename RsSource<T>::Raw raw[SEL_TILE];
#pragma unroll
        for (int q = 0; q < SEL_TILE; ++q) {
            const int64_t p = base + (int64_t)q * blockDim.x + threadIdx.x;
            if (p < n) src.fetch(p, raw[q]);
            else src.blank(raw[q]);
        }
#pragma unroll
        for (int q = 0; q < SEL_TILE; ++q) {
            const bool vok = src.value_ok(raw[q]);
            const bool ok = vok && (raw[q].m & 2);
            c_all += vok ? 1u : 0u;
            c_inl += (raw[q].m & 2) ? 1u : 0u;   // (lanes past the end hold m = 0)
            bool cand = false;
            T x = (T)0;
            if (ok) {
                ++c_n;
                const double v64 = (double)raw[q].v;
                if (src.round == 2) {
                    const double d = v64 - mean;
                    s0 += d * d;
                    x = t_abs<T>(t_sub<T>(raw[q].v, src.med));
                } else {
                    s0 += v64;
                    s1 += v64 * v64;
                    x = raw[q].v;
                }
                const K key = key_of(x);
                e_min = (K)~key > e_min ? (K)~key : e_min;
                e_max = key > e_max ? key : e_max;
                if (BR) {
                    // nearly every element is in no bracket: for those, one count and two compares per bracket; the candidates (a few
                    // percent) then say which brackets hold them and which they lie below
#pragma unroll
                    for (int b = 0; b < NBR; ++b) {
                        const bool below = key < lo[b];
                        cb[0][b] += below ? 1u : 0u;
                        cand = cand || (!below && key <= hi[b]);
                    }
                    if (cand) {
#pragma unroll
                        for (int b = 0; b < NBR; ++b) {
                            cb[1][b] += (key >= lo[b] && key <= hi[b]) ? 1u : 0u;
                            cb[2][b] += key < lo[b] ? 1u : 0u;
                        }
                    }
                } else {
                    atomicAdd(&hc[(int)((key >> top) & 0xFF)], 1u);
                }
            }
            if (BR) st.append_bounded(cand, x, (uint16_t)0, &R->ctr[2]);
        }
        if (BR) {
            if ((++it % SEL_FLUSH_EVERY) == 0) st.sync_and_flush_at(0, out_v, out_b, &R->ctr[1], cap, &R->ctr[2]);
        }
    }
    if (BR) st.sync_and_flush_at(0, out_v, out_b, &R->ctr[1], cap, &R->ctr[2]);
    // the sums: fixed order
    const int wv = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
    s0 = wave_sum<double>(s0);
    s1 = wave_sum<double>(s1);
    if (lane == 0) { s_red[0][wv] = s0; s_red[1][wv] = s1; }
    // the integers: any order
    c_n = wave_add_u32(c_n); c_all = wave_add_u32(c_all); c_inl = wave_add_u32(c_inl);
    e_min = wave_max_u<K>(e_min); e_max = wave_max_u<K>(e_max);
    if (lane == 0) {
        atomicAdd(&s_cnt[0], c_n); atomicAdd(&s_cnt[1], c_all); atomicAdd(&s_cnt[2], c_inl);
        k_atomic_max(&s_ext[0], e_min); k_atomic_max(&s_ext[1], e_max);
    }
    if (BR) {
#pragma unroll
        for (int j = 0; j < 3; ++j)
#pragma unroll
            for (int b = 0; b < NBR; ++b) {
                const uint32_t t = wave_add_u32(cb[j][b]);
                if (lane == 0 && t) atomicAdd(&s_cnt[3 + j * RS_MAXB + b], t);
            }
    }
    __syncthreads();
    if (threadIdx.x < RS_NT) {
        double t = 0.0;
        for (int k = 0; k < HIST_THREADS / 64; ++k) t += s_red[threadIdx.x][k];
        part[(int64_t)blockIdx.x * RS_NT + threadIdx.x] = t;
    }
    if (threadIdx.x < 3 && s_cnt[threadIdx.x]) atomicAdd(reinterpret_cast<unsigned long long*>(&R->icnt[threadIdx.x]), (unsigned long long)s_cnt[threadIdx.x]);
    if (threadIdx.x < 2 && s_cnt[0]) k_atomic_max(&R->kext[threadIdx.x], s_ext[threadIdx.x]);
    if (BR) {   // (rows of RS_MAXB counters in LDS and in bcnt alike; the counters of unused brackets are never read)
        if (threadIdx.x < 3 * RS_MAXB && s_cnt[3 + threadIdx.x])
            atomicAdd(reinterpret_cast<unsigned long long*>(&R->bcnt[0][0] + threadIdx.x), (unsigned long long)s_cnt[3 + threadIdx.x]);
    } else {
        for (int k = threadIdx.x; k < SEL_RADIX; k += blockDim.x) {
            unsigned long long c = 0;
            for (int q = 0; q < COPIES; ++q) c += h[q * CSTRIDE + k];
            if (c) atomicAdd(reinterpret_cast<unsigned long long*>(&hist[k]), c);
        }
    }
}

// totals[t] = the partials of term t: lane l adds l, l + 256, ... in order, then a halving tree over the 256 lanes
static __global__ __launch_bounds__(256) void rs_reduce_kernel(const double* __restrict__ part, int nblocks, double* totals) {
    __shared__ double s[256];
    const int t = blockIdx.x;
    double a = 0.0;
    for (int k = threadIdx.x; k < nblocks; k += 256) a += part[(int64_t)k * RS_NT + t];
    s[threadIdx.x] = a;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) s[threadIdx.x] += s[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) totals[t] = s[0];
}

// after round 1: the median rounded in the value dtype (np.median: the mean of the two middle values in T) and the float64 mean
template <typename T>
__global__ void rs_params_kernel(const RsRound<typename KeyT<T>::type>* R, RsParams<T>* par) {
    if (threadIdx.x || blockIdx.x) return;
    const uint64_t n = R->icnt[0];
    T med = (T)NAN;
    if (n && R->tab.st[0].active && R->tab.st[1].active) {
        const T lo = val_of(R->tab.st[0].prefix), hi = val_of(R->tab.st[1].prefix);
        med = (n & 1) ? lo : t_div<T>(t_add<T>(lo, hi), (T)2);
    }
    par->med = med;
    par->pad = (T)0;
    par->mean = n ? R->totals[0] / (double)n : (double)NAN;
}

// bracket b from the sample's states 2b (low end) and 2b + 1 (high end): only the leading digits are fixed, `low_mask` = the open ones
template <typename K>
__global__ void rs_brackets_kernel(RsRound<K>* R, int nbr, int degenerate, K low_mask) {
    const int b = threadIdx.x;
    if (b >= nbr) return;
    const MsState<K> a = R->tab_s.st[2 * b], z = R->tab_s.st[2 * b + 1];
    const bool have = a.active && z.active;   // (an empty sample: everything is a candidate)
    R->klo[b] = have ? a.prefix : (K)0;
    R->khi[b] = have ? (degenerate ? a.prefix : (K)(z.prefix | low_mask)) : (K)~(K)0;
}

// the wanted ranks among the candidates: rank - (elements below the rank's bracket that are in no bracket = all below it - the candidates
// below it); raises ctr[3] when a rank lies outside its bracket
template <typename K>
__global__ void rs_given_kernel(RsRound<K>* R, MsSpecs want) {
    const int r = threadIdx.x;
    if (r >= want.n) return;
    const uint64_t n = R->icnt[0];
    uint64_t g = ~(uint64_t)0;
    if (n) {
        const uint64_t k = ms_rank(want.s[r], n, 0);
        const int b = want.s[r].bracket;
        const uint64_t lt = R->bcnt[0][b], in = R->bcnt[1][b], nc = lt - R->bcnt[2][b];
        if (k < lt || k >= lt + in) R->ctr[3] = 1ull;
        else g = k - nc;
    }
    R->given[r] = g;
}

template <typename T>
static int raster_stats_typed(xdemhip_ctx* ctx, const void* values, int64_t n, const uint8_t* total_mask, const uint8_t* inlier, int has_nodata, double nodata,
                              const double* quantiles, int nq, double nfact, int memspace, xdemhip_raster_stats_out* out) {
    typedef typename KeyT<T>::type K;
    const int passes = KeyT<T>::passes;
    XdBuffers buf(ctx, "xdemhip_raster_stats");
    RsSource<T> src;
    src.vals = buf.input(static_cast<const T*>(values), (size_t)n * sizeof(T), memspace);
    src.tmask = buf.input(total_mask, (size_t)n, memspace);
    src.inl = buf.input(inlier, (size_t)n, memspace);
    RsCtrl<T>* ctrl = buf.alloc<RsCtrl<T>>(1);
    const int grid = grid_for(ctx, n, HIST_THREADS * SEL_TILE, 2);
    double* part = buf.alloc<double>((size_t)grid * RS_NT);
    if (buf.rc) return buf.rc;
    src.par = &ctrl->par;
    src.nodata = (T)nodata;
    src.has_nodata = has_nodata && nodata == nodata;   // (rounded to T before it is compared, as NumPy's `v == nodata` does)
    src.round = 1;
    src.med = (T)0;
    XD_HIP_CHECK(ctx, hipMemsetAsync(ctrl, 0, offsetof(RsCtrl<T>, hist), ctx->stream));

    // the wanted ranks of the two rounds, and for the bracketed route the ends of their brackets in a sample
    MsSpecs want[2], ends[2];
    memset(want, 0, sizeof want);
    memset(ends, 0, sizeof ends);
    for (int b = 0; b <= nq; ++b)
        for (int e = 0; e < 2; ++e) {
            MsSpec s = {b == 0 ? MS_MEDIAN : MS_QUANTILE, e, b, 0, b == 0 ? 0.5 : quantiles[b - 1]};
            want[0].s[2 * b + e] = s;
            s.end = MS_BR_LO + e;
            ends[0].s[2 * b + e] = s;
        }
    want[0].n = ends[0].n = 2 * (nq + 1);
    want[1].n = ends[1].n = 2;
    for (int e = 0; e < 2; ++e) { want[1].s[e] = want[0].s[e]; ends[1].s[e] = ends[0].s[e]; }

    const int mode = ctx->selection_mode;
    const bool try_brackets = mode != 1 && (mode == 2 || mode == 3 || n >= SEL_BRACKET_MIN_N);
    SelWorkspaceLocal lws(ctx);
    if (try_brackets) (void)sel_ws_create(lws.mem, n, sizeof(T), 1, lws.ws);   // (on failure: the plain route)
    const size_t lds_hist = (size_t)(SEL_RADIX + 1) * 32 * 4;
    const size_t lds_stage = (size_t)SEL_STAGE_CAP * (sizeof(T) + 2) + 16;
    double reads = 0.0;

    for (int round = 0; round < 2; ++round) {
        RsRound<K>* R = &ctrl->r[round];
        src.round = round + 1;
        const int nbr = round == 0 ? nq + 1 : 1;
        bool done = false;
        out->route[round] = 1;
        if (try_brackets && lws.ws.d_small) {
            // sample -> bracket ends -> the one pass -> the ranks among the candidates
            int rc = set_big_lds(ctx, sample_lines_kernel<T, RsSource<T>>, lds_stage);
            if (rc) return rc;
            hipLaunchKernelGGL((sample_lines_kernel<T, RsSource<T>>), dim3(grid_for(ctx, n / 64 + 1, HIST_THREADS, 2)), dim3(HIST_THREADS), lds_stage, ctx->stream,
                               src, n, 1, static_cast<T*>(lws.ws.s_vals), lws.ws.s_bins, R->ctr, lws.ws.s_cap);
            XD_HIP_CHECK(ctx, hipGetLastError());
            constexpr int BR_PASSES = 3;
            const K low_mask = (K)(((K)1 << (8 * (passes - BR_PASSES))) - 1);
            ArraySource<T> sample{static_cast<const T*>(lws.ws.s_vals), nullptr};
            rc = ms_enqueue<T, ArraySource<T>>(ctx, sample, lws.ws.s_cap, n / 48 + 1, R->ctr + 0, &R->tab_s, ctrl->hist, ends[round], nullptr, BR_PASSES, false);
            if (rc) return rc;
            hipLaunchKernelGGL((rs_brackets_kernel<K>), dim3(1), dim3(64), 0, ctx->stream, R, nbr, (int)(mode == 2), low_mask);
            XD_HIP_CHECK(ctx, hipGetLastError());
            auto pass = nbr == 1 ? rs_data_pass_kernel<T, true, 1> : rs_data_pass_kernel<T, true, RS_MAXB>;
            rc = set_big_lds(ctx, pass, lds_stage);
            if (rc) return rc;
            hipLaunchKernelGGL(pass, dim3(grid), dim3(HIST_THREADS), lds_stage, ctx->stream, src, n, R, part, ctrl->hist, nbr,
                               static_cast<T*>(lws.ws.c_vals), lws.ws.c_bins, lws.ws.c_cap);
            hipLaunchKernelGGL(rs_reduce_kernel, dim3(RS_NT), dim3(256), 0, ctx->stream, part, grid, R->totals);
            hipLaunchKernelGGL((rs_given_kernel<K>), dim3(1), dim3(64), 0, ctx->stream, R, want[round]);
            XD_HIP_CHECK(ctx, hipGetLastError());
            MsSpecs giv = want[round];
            for (int i = 0; i < giv.n; ++i) giv.s[i].end = MS_GIVEN;
            ArraySource<T> cands{static_cast<const T*>(lws.ws.c_vals), nullptr};
            rc = ms_enqueue<T, ArraySource<T>>(ctx, cands, lws.ws.c_cap, n / 32 + 1, R->ctr + 1, &R->tab, ctrl->hist, giv, R->given, 0, false);
            if (rc) return rc;
            reads += 1.0 + 1.0 / 64.0;
            unsigned long long flags[4];
            XD_HIP_CHECK(ctx, hipMemcpyAsync(flags, R->ctr, sizeof flags, hipMemcpyDeviceToHost, ctx->stream));
            XD_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
            done = flags[2] == 0 && flags[3] == 0;
            out->route[round] = done ? 0 : 2;
        }
        if (!done) {
            XD_HIP_CHECK(ctx, hipMemsetAsync(R, 0, sizeof(RsRound<K>), ctx->stream));
            XD_HIP_CHECK(ctx, hipMemsetAsync(ctrl->hist, 0, (size_t)MS_MAX * SEL_RADIX * 8, ctx->stream));
            hipLaunchKernelGGL((rs_data_pass_kernel<T, false, 1>), dim3(grid), dim3(HIST_THREADS), lds_hist, ctx->stream, src, n, R, part, ctrl->hist, 0,
                               static_cast<T*>(nullptr), static_cast<uint16_t*>(nullptr), (int64_t)0);
            hipLaunchKernelGGL(rs_reduce_kernel, dim3(RS_NT), dim3(256), 0, ctx->stream, part, grid, R->totals);
            XD_HIP_CHECK(ctx, hipGetLastError());
            const int rc = ms_enqueue<T, RsSource<T>>(ctx, src, n, n, nullptr, &R->tab, ctrl->hist, want[round], nullptr, 0, true);
            if (rc) return rc;
            reads += (double)passes;
        }
        if (round == 0) {
            hipLaunchKernelGGL((rs_params_kernel<T>), dim3(1), dim3(64), 0, ctx->stream, R, &ctrl->par);
            XD_HIP_CHECK(ctx, hipGetLastError());
        }
    }

    // one fetch of everything but the histograms
    std::vector<unsigned char> hb(offsetof(RsCtrl<T>, hist));
    XD_HIP_CHECK(ctx, hipMemcpyAsync(hb.data(), ctrl, hb.size(), hipMemcpyDeviceToHost, ctx->stream));
    XD_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    const RsCtrl<T>* H = reinterpret_cast<const RsCtrl<T>*>(hb.data());
    const RsRound<K>& A = H->r[0];
    const RsRound<K>& B = H->r[1];
    out->n = (int64_t)A.icnt[0];
    out->n_valid = (int64_t)A.icnt[1];
    out->n_inlier = inlier ? (int64_t)A.icnt[2] : n;
    out->reads = reads;
    if (A.icnt[0] == 0) return buf.finish();   // (every value stays NaN)
    auto stat = [](const MsTable<K>& t, int i) { return t.st[i].active ? (double)val_of(t.st[i].prefix) : (double)NAN; };
    out->min = (double)val_of((K)~A.kext[0]);
    out->max = (double)val_of(A.kext[1]);
    out->sum = A.totals[0];
    out->sumsq = A.totals[1];
    out->sumdev2 = B.totals[0];
    out->med_lo = stat(A.tab, 0);
    out->med_hi = stat(A.tab, 1);
    out->median = (double)H->par.med;
    for (int i = 0; i < nq; ++i) { out->q_lo[i] = stat(A.tab, 2 + 2 * i); out->q_hi[i] = stat(A.tab, 3 + 2 * i); }
    out->mad_lo = stat(B.tab, 0);
    out->mad_hi = stat(B.tab, 1);
    const T ml = (T)out->mad_lo, mh = (T)out->mad_hi;
    const T mad = (A.icnt[0] & 1) ? ml : (T)((T)(ml + mh) / (T)2);
    out->nmad = (double)(T)((T)nfact * mad);   // (xdemhip_nmad's rounding: the Python float is a weak scalar)
    return buf.finish();
}

}  // namespace xd

using namespace xd;

extern "C" int xdemhip_raster_stats(xdemhip_ctx* ctx, const void* values, int dtype, int64_t n, const uint8_t* total_mask, const uint8_t* inlier, int has_nodata,
                                    double nodata, const double* quantiles, int nq, double nfact, int memspace, xdemhip_raster_stats_out* out) {
    if (!ctx) return XDEMHIP_EINVAL;
    if (n < 0 || (n > 0 && !values) || !out || nq < 0 || nq > XDEMHIP_STATS_MAXQ || (nq > 0 && !quantiles)) return xd_fail(ctx, XDEMHIP_EINVAL, "bad argument");
    if (dtype != XDEMHIP_F32 && dtype != XDEMHIP_F64) return xd_fail(ctx, XDEMHIP_EINVAL, "dtype must be float32 or float64");
    if (memspace != XDEMHIP_HOST && memspace != XDEMHIP_DEVICE) return xd_fail(ctx, XDEMHIP_EINVAL, "bad memspace");
    for (int i = 0; i < nq; ++i)
        if (!(quantiles[i] >= 0.0 && quantiles[i] <= 1.0)) return xd_fail(ctx, XDEMHIP_EINVAL, "quantiles must lie in [0, 1]");
    if (ctx->allreduce) return xd_fail(ctx, XDEMHIP_EUNSUPPORTED, "xdemhip_raster_stats: statistics of a partitioned raster are not supported");
    memset(out, 0, sizeof *out);
    out->min = out->max = out->sum = out->sumsq = out->sumdev2 = out->med_lo = out->med_hi = out->median = out->mad_lo = out->mad_hi = out->nmad = (double)NAN;
    for (int i = 0; i < XDEMHIP_STATS_MAXQ; ++i) out->q_lo[i] = out->q_hi[i] = (double)NAN;
    out->route[0] = out->route[1] = 1;
    if (n == 0) return XDEMHIP_OK;
    XD_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    if (dtype == XDEMHIP_F32) return raster_stats_typed<float>(ctx, values, n, total_mask, inlier, has_nodata, nodata, quantiles, nq, nfact, memspace, out);
    return raster_stats_typed<double>(ctx, values, n, total_mask, inlier, has_nodata, nodata, quantiles, nq, nfact, memspace, out);
}
