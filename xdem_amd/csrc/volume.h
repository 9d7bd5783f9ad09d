// volume.h -- device helpers of volume.hip (xdem/volume.py on the GPU): the two interval searches, SciPy's linear interp1d, and
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

}  // namespace xd
