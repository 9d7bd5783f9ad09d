// multi_select.h -- several arbitrary ranks of ONE array selected in the same digit passes (exact order statistics).
//
// select.h / select_run.h select one rank per bin (two with SEL_BRACKET_DUAL); the raster statistics (rasterstats.hip) want the two
// medians and up to four pairs of percentile ranks of one array at once.  Up to MS_MAX target ranks advance together through the
// 8-bit radix passes of select.h (ordered keys, most significant digit first: 4 passes for float32, 8 for float64):
//   * a pass keeps one 256-counter LDS histogram per DISTINCT ACTIVE PREFIX (a "group"): ranks that still agree on the digits fixed
//     so far share a table, an element is counted in the one group whose prefix it matches (prefixes are distinct: at most one);
//   * the tables are privatised over lanes (copy = lane % copies, odd stride -- hist_pass_kernel's layout): the leading digit of
//     float keys, sign and exponent, is the same for nearly every element;
//   * ms_advance_kernel: one wave per state locates its rank's digit in its group's table (the scan of select_advance_body), then
//     one lane regroups the states by their new prefixes.
// After the last pass every active state's prefix IS its order statistic; upper medians / upper percentile neighbours are states of
// their own, so no successor pass is needed.  All counting is integer: exact and independent of the order of the atomics.
// The target ranks are fixed ON THE DEVICE by the first advance, from the element count its histogram gives (MsSpec): no fetch of n.
#pragma once
#include "select_run.h"

namespace xd {

constexpr int MS_MAX = 10;                  // states (target ranks) of one selection
constexpr int MS_LDS_WORDS = 16 * 1024;     // 64 KiB of histogram counters per workgroup: 2 workgroups of 1024 lanes per CU

template <typename K> struct MsState {
    K prefix;          // key digits fixed so far
    uint64_t rank;     // remaining 0-based rank inside the prefix group
    uint32_t active;   // 0: no such rank (empty input, rank beyond the count, a skipped given rank)
    uint32_t group;    // the histogram table of the NEXT pass this state reads
};
// the device-resident state of one selection
template <typename K> struct MsTable {
    MsState<K> st[MS_MAX];
    K gprefix[MS_MAX];   // the distinct prefixes of the active states
    uint32_t ngroups, nstates;
    uint64_t count;      // elements the first pass counted
};

// What rank a state selects, as a function of the element count c the first pass finds:
//   what = MS_MEDIAN: the pair (c - 1) / 2, c / 2;  MS_QUANTILE: lo = floor((c - 1) * q) -- one float64 multiply -- and min(lo + 1, c - 1)
//   end  = MS_LO / MS_HI: the lower / upper rank of the pair;  MS_BR_LO / MS_BR_HI: the pair of a SAMPLE moved down / up by
//          sel_bracket_halfwidth(c) and clipped (bracket ends);  MS_GIVEN: given[state] (all-ones: skip)
enum { MS_MEDIAN = 0, MS_QUANTILE = 1 };
enum { MS_LO = 0, MS_HI = 1, MS_BR_LO = 2, MS_BR_HI = 3, MS_GIVEN = 4 };
struct MsSpec { int what, end; int bracket /* rasterstats.hip: the bracket that holds this rank */, pad; double q; };
struct MsSpecs { int n; int pad; MsSpec s[MS_MAX]; };

#pragma clang fp contract(off)
__host__ __device__ inline uint64_t ms_rank(const MsSpec& sp, uint64_t c, uint64_t given) {
    if (sp.end == MS_GIVEN) return given;
    if (c == 0) return ~(uint64_t)0;
    uint64_t lo, hi;
    if (sp.what == MS_MEDIAN) { lo = (c - 1) / 2; hi = c / 2; }
    else {
        const double vi = (double)(c - 1) * sp.q;
        lo = (uint64_t)floor(vi);
        if (lo > c - 1) lo = c - 1;
        hi = lo + 1 < c ? lo + 1 : c - 1;
    }
    if (sp.end == MS_LO) return lo;
    if (sp.end == MS_HI) return hi;
    const uint64_t h = sel_bracket_halfwidth(c);
    if (sp.end == MS_BR_LO) return lo > h ? lo - h : 0;
    return hi + h < c ? hi + h : c - 1;
}

// One digit pass over a source's elements (select_run.h: ArraySource and its kin).  LDS: MS_LDS_WORDS counters shared out over
// `copies` privatised sets of G tables, G = the number of groups (1 at the first digit).
template <typename T, typename Src>
__global__ __launch_bounds__(HIST_THREADS) void ms_hist_kernel(Src src, int64_t n, const unsigned long long* n_dev, const MsTable<typename KeyT<T>::type>* tab,
                                                               int shift, int first, uint64_t* hist /* [MS_MAX][256] of this pass, zero */) {
    typedef typename KeyT<T>::type K;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint32_t* h = reinterpret_cast<uint32_t*>(smem);
    if (n_dev) {
        const unsigned long long m = *n_dev;
        n = m < (unsigned long long)n ? (int64_t)m : n;
    }
    const int G = first ? 1 : (int)tab->ngroups;
    if (G < 1 || G > MS_MAX) return;   // (uniform) no active state
    const int table = G * SEL_RADIX, cstride = table + 1;
    int copies = MS_LDS_WORDS / cstride;
    copies = copies > 32 ? 32 : copies;
    for (int k = threadIdx.x; k < cstride * copies; k += blockDim.x) h[k] = 0;
    // the groups' prefixes in registers (uniform loads): an element is compared with all of them, and in the late passes matches none
    K gp[MS_MAX];
#pragma unroll
    for (int g = 0; g < MS_MAX; ++g) gp[g] = (!first && g < G) ? tab->gprefix[g] : (K)0;
    src.setup(nullptr, 1);
    __syncthreads();
    uint32_t* hc = h + (threadIdx.x % copies) * cstride;
    const K himask = first ? (K)0 : (K)(~(K)0 << (shift + 8));
    typename Src::Acc acc;
    const int64_t step = (int64_t)blockDim.x * SEL_UNROLL;
    for (int64_t base = (int64_t)blockIdx.x * step; base < n; base += (int64_t)gridDim.x * step) {
        typename Src::Raw raw[SEL_UNROLL];
#pragma unroll
        for (int q = 0; q < SEL_UNROLL; ++q) {
            const int64_t p = base + (int64_t)q * blockDim.x + threadIdx.x;
            if (p < n) src.fetch(p, raw[q]);
            else src.blank(raw[q]);
        }
#pragma unroll
        for (int q = 0; q < SEL_UNROLL; ++q) {
            T v;
            uint16_t b;
            if (!src.template eval<false>(raw[q], 1, v, b, acc)) continue;
            const K key = key_of(v);
            const K hi = (K)(key & himask);
            const int digit = (int)((key >> shift) & 0xFF);
            int g = -1;
#pragma unroll
            for (int j = 0; j < MS_MAX; ++j) g = (j < G && hi == gp[j]) ? j : g;
            if (g >= 0) atomicAdd(&hc[g * SEL_RADIX + digit], 1u);
        }
    }
    __syncthreads();
    const int flush_0 = (int)(((unsigned)blockIdx.x * 37u) % (unsigned)G) * SEL_RADIX;   // (each workgroup starts at its own row: hist_pass_kernel)
    for (int kk = threadIdx.x; kk < table; kk += blockDim.x) {
        const int k = kk + flush_0 < table ? kk + flush_0 : kk + flush_0 - table;
        unsigned long long c = 0;
        for (int q = 0; q < copies; ++q) c += h[q * cstride + k];
        if (c) atomicAdd(reinterpret_cast<unsigned long long*>(&hist[k]), c);
    }
}

// Advance every state by one digit -- one wave per state, lane l owns buckets 4l .. 4l+3 of the state's group table -- then regroup.
// First digit: the one table's total is the element count, from which every state's rank is fixed (ms_rank).
template <typename K>
__global__ __launch_bounds__(64 * MS_MAX) void ms_advance_kernel(MsTable<K>* tab, const uint64_t* hist, MsSpecs sp, int shift, int first, const uint64_t* given) {
    __shared__ MsState<K> s_st[MS_MAX];
    const int w = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
    const int ns = sp.n < MS_MAX ? sp.n : MS_MAX;
    if (w < ns) {
        MsState<K> s;
        if (first) { s.prefix = 0; s.rank = 0; s.active = 1u; s.group = 0u; }
        else s = tab->st[w];
        if (s.active) {
            const uint64_t* h = hist + (size_t)s.group * SEL_RADIX;
            unsigned long long c[4], mine = 0;
#pragma unroll
            for (int q = 0; q < 4; ++q) { c[q] = (unsigned long long)h[4 * lane + q]; mine += c[q]; }
            unsigned long long incl = mine;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const unsigned long long t = __shfl_up(incl, off);
                if (lane >= off) incl += t;
            }
            const unsigned long long total = __shfl(incl, 63);
            if (first) {
                const uint64_t r = ms_rank(sp.s[w], (uint64_t)total, given ? given[w] : ~(uint64_t)0);
                s.active = (total > 0 && r != ~(uint64_t)0 && r < total) ? 1u : 0u;
                s.rank = s.active ? r : 0;
                if (w == 0 && lane == 0) tab->count = total;
            }
            if (s.active) {   // (uniform over the wave)
                const unsigned long long excl = incl - mine;
                const bool here = (s.rank >= excl) && (s.rank < incl);
                const unsigned long long vote = __ballot(here);
                const int src = vote ? (int)__ffsll((long long)vote) - 1 : 63;
                unsigned long long cum = excl;
                int q = 0;
                if (cum + c[0] <= s.rank) { cum += c[0]; q = 1;
                    if (cum + c[1] <= s.rank) { cum += c[1]; q = 2;
                        if (cum + c[2] <= s.rank) { cum += c[2]; q = 3; } } }
                const int dsel = __shfl(4 * lane + q, src);
                const unsigned long long cumsel = __shfl(cum, src);
                s.prefix |= (K)dsel << shift;
                s.rank -= cumsel;
            }
        }
        if (lane == 0) s_st[w] = s;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t ng = 0;
        for (int i = 0; i < ns; ++i) {
            MsState<K> s = s_st[i];
            if (s.active) {
                uint32_t g = 0;
                while (g < ng && tab->gprefix[g] != s.prefix) ++g;
                if (g == ng) tab->gprefix[ng++] = s.prefix;
                s.group = g;
            }
            tab->st[i] = s;
        }
        tab->ngroups = ng;
        tab->nstates = (uint32_t)ns;
    }
}

// Queue a selection of sp.n ranks over `src` on the context's stream: `run` leading digits (0 = all).  `hist`: KeyT<T>::passes tables of
// [MS_MAX][256] counters; first_hist_done: the caller's own pass filled the first digit's table (row 0) -- everything else is zeroed here.
// d_n (optional): the element count lives on the device, `n` is the capacity and `n_grid` what the grids are sized for.
template <typename T, typename Src>
int ms_enqueue(xdemhip_ctx* ctx, const Src& src, int64_t n, int64_t n_grid, const unsigned long long* d_n, MsTable<typename KeyT<T>::type>* tab, uint64_t* hist,
               const MsSpecs& sp, const uint64_t* d_given, int run, bool first_hist_done) {
    typedef typename KeyT<T>::type K;
    const int passes = KeyT<T>::passes;
    const size_t pass_words = (size_t)MS_MAX * SEL_RADIX;
    if (run <= 0 || run > passes) run = passes;
    const int z0 = first_hist_done ? 1 : 0;
    XD_HIP_CHECK(ctx, hipMemsetAsync(hist + z0 * pass_words, 0, (size_t)(passes - z0) * pass_words * 8, ctx->stream));
    const size_t lds = (size_t)MS_LDS_WORDS * 4;
    const int rc = set_big_lds(ctx, ms_hist_kernel<T, Src>, lds);
    if (rc) return rc;
    const int grid = grid_for(ctx, n_grid, HIST_THREADS * SEL_UNROLL, n_grid < ((int64_t)1 << 24) ? 1 : 2);
    for (int p = 0; p < run; ++p) {
        const int shift = 8 * (passes - 1 - p);
        uint64_t* hp = hist + (size_t)p * pass_words;
        if (n > 0 && !(p == 0 && first_hist_done)) {
            hipLaunchKernelGGL((ms_hist_kernel<T, Src>), dim3(grid), dim3(HIST_THREADS), lds, ctx->stream, src, n, d_n, tab, shift, (int)(p == 0), hp);
            XD_HIP_CHECK(ctx, hipGetLastError());
        }
        hipLaunchKernelGGL((ms_advance_kernel<K>), dim3(1), dim3(64 * MS_MAX), 0, ctx->stream, tab, hp, sp, shift, (int)(p == 0), d_given);
        XD_HIP_CHECK(ctx, hipGetLastError());
    }
    return XDEMHIP_OK;
}

}  // namespace xd
