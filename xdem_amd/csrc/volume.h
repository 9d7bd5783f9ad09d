// volume.h -- device helpers of volume.hip and demstack.hip (xdem/volume.py on the GPU): the two interval searches, SciPy's linear interp1d, and
// what one workgroup does to one segment of values: a sort (in LDS or in place in global memory), an exact radix selection over a
// slice of global memory, and a sum in a fixed order.  Everything here runs with 256 threads per workgroup and without contraction
// (the Makefile builds volume.hip with -ffp-contract=off).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "select.h"

namespace xd {

constexpr int HYP_THREADS = 256;

// np.digitize(x, edges) for increasing edges, right=False: the number of edges <= x (np.searchsorted(edges, x, side="right")).
// NaN compares false everywhere: 0, "below the first edge".
__device__ __forceinline__ int hyp_count_le(const double* __restrict__ e, int n, double x) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (e[mid] <= x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// np.searchsorted(xs, x) (side="left"): the number of entries < x
__device__ __forceinline__ int hyp_count_lt(const double* __restrict__ xs, int n, double x) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (xs[mid] < x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// scipy.interpolate.interp1d(xs, ys, kind="linear", fill_value="extrapolate")(x), as _call_linear writes it: the interval from
// searchsorted clipped to [1, n - 1], slope = (y_hi - y_lo) / (x_hi - x_lo), slope * (x - x_lo) + y_lo -- every operation rounded
// on its own.  A NaN x gives NaN from any interval.
__device__ __forceinline__ double hyp_interp1d(const double* __restrict__ xs, const double* __restrict__ ys, int n, double x) {
    int hi = hyp_count_lt(xs, n, x);
    hi = hi < 1 ? 1 : (hi > n - 1 ? n - 1 : hi);
    const int lo = hi - 1;
    const double x_lo = xs[lo], x_hi = xs[hi], y_lo = ys[lo], y_hi = ys[hi];
    const double slope = (y_hi - y_lo) / (x_hi - x_lo);
    const double t = slope * (x - x_lo);
    return t + y_lo;
}

// Ascending sort of a[0 .. n) by one workgroup, any n: the bitonic network with every comparator pointing up (first step of a
// merge: partner i ^ (k - 1), then i ^ j).  Positions at or beyond n stand for +infinity, which such a network never moves, so
// their comparators are skipped.  `a` is LDS or global memory: __syncthreads orders both inside a workgroup.
template <typename E, typename Less>
__device__ __forceinline__ void hyp_sort(E* a, int64_t n, Less less) {
    for (int64_t k = 2; (k >> 1) < n; k <<= 1) {
        for (int64_t i = threadIdx.x; i < n; i += HYP_THREADS) {
            const int64_t l = i ^ (k - 1);
            if (l > i && l < n) {
                const E x = a[i], y = a[l];
                if (less(y, x)) { a[i] = y; a[l] = x; }
            }
        }
        __syncthreads();
        for (int64_t j = k >> 2; j > 0; j >>= 1) {
            for (int64_t i = threadIdx.x; i < n; i += HYP_THREADS) {
                const int64_t l = i ^ j;
                if (l > i && l < n) {
                    const E x = a[i], y = a[l];
                    if (less(y, x)) { a[i] = y; a[l] = x; }
                }
            }
            __syncthreads();
        }
    }
}

struct HypSelectShared {
    unsigned int hist[256];
    unsigned long long prefix, rank;
};

// The key of 0-based rank `rank` among the n finite values v[0 .. n) (n < 2^32), by one workgroup: most significant digit first,
// 8 bits per pass, a 256-counter LDS histogram of the values that still match the digits fixed so far.  All counting is integer.
template <typename T>
__device__ __forceinline__ typename KeyT<T>::type hyp_radix_select(const T* v, int64_t n, uint64_t rank, HypSelectShared* s) {
    typedef typename KeyT<T>::type K;
    K prefix = 0, mask = 0;
    if (threadIdx.x == 0) s->rank = rank;
    for (int shift = (int)sizeof(K) * 8 - 8; shift >= 0; shift -= 8) {
        s->hist[threadIdx.x] = 0u;
        __syncthreads();
        // The leading digits of a segment's values are nearly all equal, and 64 lanes adding to one counter take 64 turns: the
        // digits of the wave's first lanes are counted by ballot (two rounds), what is left lane by lane.  Every wave walks whole
        // groups of 64 values (the loop runs to n rounded up), so the wave-wide operations see all lanes.
        const int lane = threadIdx.x & 63;
        const int64_t n_pad = (n + HYP_THREADS - 1) / HYP_THREADS * HYP_THREADS;
        for (int64_t i = threadIdx.x; i < n_pad; i += HYP_THREADS) {
            int d = -1;
            if (i < n) {
                const K key = key_of(v[i]);
                if ((key & mask) == prefix) d = (int)((unsigned)(key >> shift) & 255u);
            }
            unsigned long long rem = __ballot(d >= 0);
            for (int round = 0; round < 2 && rem; ++round) {
                const int src = __ffsll((unsigned long long)rem) - 1;
                const int d0 = __shfl(d, src);
                const unsigned long long same = __ballot(d == d0) & rem;
                if (lane == src) atomicAdd(&s->hist[d0], (unsigned int)__popcll(same));
                rem &= ~same;
            }
            if ((rem >> lane) & 1ull) atomicAdd(&s->hist[d], 1u);
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            uint64_t r = s->rank, cum = 0;
            int b = 0;
            for (; b < 255; ++b) {
                if (r < cum + s->hist[b]) break;
                cum += s->hist[b];
            }
            s->prefix = (unsigned long long)(prefix | ((K)b << shift));
            s->rank = r - cum;
        }
        __syncthreads();
        prefix = (K)s->prefix;
        mask |= (K)255 << shift;
        __syncthreads();
    }
    return prefix;
}

// sum of get(0) .. get(n - 1) in float64 in one fixed order: lane t adds its elements t, t + 256, ... in turn, then the 256 partial
// sums fold pairwise.  `red`: 256 doubles of LDS, free again on return.
template <typename F>
__device__ __forceinline__ double hyp_fixed_sum(F get, int64_t n, double* red) {
    double acc = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += HYP_THREADS) acc = acc + get(i);
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int off = HYP_THREADS / 2; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) red[threadIdx.x] = red[threadIdx.x] + red[threadIdx.x + off];
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

constexpr int HYP_SEG_LDS = 8192;       // values of a segment sorted in LDS: 32 KiB of float32 keys, 64 KiB of float64 keys

// ---- the counting sort's second half and the per-segment statistics: shared by volume.hip and demstack.hip ------------------------------
// grp: the group of every value (-1: in none), cursor: the exclusive scan of the group counts; seg: the values in group-contiguous
// segments.
template <typename T>
__global__ __launch_bounds__(256) void hyp_scatter_kernel(const T* __restrict__ ddem, const int32_t* __restrict__ grp, int64_t n, unsigned long long* cursor,
                                                          T* __restrict__ seg) {
    const int64_t n_pad = (n + 63) & ~(int64_t)63;
    const int lane = threadIdx.x & 63;
    for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < n_pad; p += (int64_t)gridDim.x * 256) {
        const int32_t g = p < n ? grp[p] : -1;
        const int32_t g0 = __builtin_amdgcn_readfirstlane(g);
        if (__all(g == g0)) {
            if (g0 >= 0) {   // a wave inside one group takes its 64 places with one atomic
                unsigned long long base = 0ull;
                if (lane == 0) base = atomicAdd(&cursor[g0], 64ull);
                base = __shfl(base, 0);
                seg[base + lane] = ddem[p];
            }
        } else {
            // voids and bin borders split most waves: the groups of the wave's first lanes take their places with one atomic each
            // (three rounds), what is left goes lane by lane
            unsigned long long rem = __ballot(g >= 0);
            const unsigned long long below = (1ull << lane) - 1ull;
            for (int round = 0; round < 3 && rem; ++round) {
                const int src = __ffsll((unsigned long long)rem) - 1;
                const int32_t g1 = __shfl(g, src);
                const unsigned long long same = __ballot(g == g1);
                unsigned long long base = 0ull;
                if (lane == src) base = atomicAdd(&cursor[g1], (unsigned long long)__popcll(same));
                base = __shfl(base, src);
                if (g == g1) seg[base + (unsigned long long)__popcll(same & below)] = ddem[p];
                rem &= ~same;
            }
            if ((rem >> lane) & 1ull) {
                const unsigned long long at = atomicAdd(&cursor[g], 1ull);
                seg[at] = ddem[p];
            }
        }
    }
}

// ---- 3. per-segment statistics ----------------------------------------------------------------------------------------------------------
// off: the exclusive scan of the group counts, off[n_groups] = their total.  A segment of at most `cap` values is sorted in LDS (as
// keys); a longer one takes the radix selection over its slice and, only where the standard deviation is wanted, is sorted in place.
// np.median: the mean of the two middle values in the value dtype for an even count.  np.nanstd (ddof 0) in float64: the mean, then
// the squared deviations, both summed in one fixed order over the sorted segment.
template <typename T>
__global__ __launch_bounds__(256) void hyp_segment_kernel(T* seg, const unsigned long long* __restrict__ off, int n_groups, int cap, int want_std,
                                                          int64_t* __restrict__ counts, double* __restrict__ med, double* __restrict__ sd) {
    typedef typename KeyT<T>::type K;
    extern __shared__ __attribute__((aligned(16))) unsigned char hyp_smem[];
    K* s_keys = reinterpret_cast<K*>(hyp_smem);
    __shared__ HypSelectShared s_sel;
    __shared__ double s_red[HYP_THREADS];
    for (int g = blockIdx.x; g < n_groups; g += gridDim.x) {
        const int64_t b = (int64_t)off[g], c = (int64_t)off[g + 1] - b;
        if (c == 0) {
            if (threadIdx.x == 0) {
                counts[g] = 0;
                med[g] = (double)NAN;
                if (sd) sd[g] = (double)NAN;
            }
            continue;
        }
        T* v = seg + b;
        const int64_t k0 = (c - 1) / 2, k1 = c / 2;
        const bool in_lds = c <= cap;
        T lo, hi;
        if (in_lds) {
            for (int64_t i = threadIdx.x; i < c; i += HYP_THREADS) s_keys[i] = key_of(v[i]);
            __syncthreads();
            hyp_sort(s_keys, c, [](K x, K y) { return x < y; });
            lo = val_of(s_keys[k0]);
            hi = val_of(s_keys[k1]);
        } else {
            const K klo = hyp_radix_select<T>(v, c, (uint64_t)k0, &s_sel);
            const K khi = k1 == k0 ? klo : hyp_radix_select<T>(v, c, (uint64_t)k1, &s_sel);
            lo = val_of(klo);
            hi = val_of(khi);
            if (want_std) hyp_sort(v, c, [](T x, T y) { return key_of(x) < key_of(y); });
        }
        const T m = k0 == k1 ? lo : (T)((T)(lo + hi) / (T)2);
        double s = (double)NAN;
        if (want_std) {
            auto at = [&](int64_t i) { return in_lds ? (double)val_of(s_keys[i]) : (double)v[i]; };
            const double mean = hyp_fixed_sum(at, c, s_red) / (double)c;
            const double ss = hyp_fixed_sum([&](int64_t i) { const double d = at(i) - mean; return d * d; }, c, s_red);
            s = sqrt(ss / (double)c);
        }
        if (threadIdx.x == 0) {
            counts[g] = c;
            med[g] = (double)m;
            if (sd) sd[g] = s;
        }
        __syncthreads();   // (the keys in LDS are read until here)
    }
}

}  // namespace xd
