// perbin_locate.h -- the interval search of the per-bin lookup for sorted disjoint intervals (what nd_binning produces), shared by
// xdemhip_perbin_lookup (perbin.hip) and the fused correction pass xdemhip_corr_apply (bincorr.hip).
#pragma once
#include "common.h"

namespace xd {

// One variable's step for U pixels at once (U independent search chains in flight): the only candidate interval is the last one
// whose left end is <= v -- branch-free binary search with a wave-uniform trip count (a NaN compares false everywhere and finds
// none) -- then in[u] &&= v < its right end and idx[u] = idx[u] * n + its position (itertools.product order: the last variable
// runs fastest).  val(u): the variable's value at pixel u; lo_of(e) / hi_of(e): the ends of interval e of the concatenated
// tables; base, n: this variable's offset and number of intervals.
template <int U, typename ValF, typename LoF, typename HiF>
__device__ __forceinline__ void pb_locate(ValF val, int base, int n, LoF lo_of, HiF hi_of, bool* in, int64_t* idx) {
    int top = 1;
    while (top <= n) top <<= 1;   // (uniform)
    int pos[U];
#pragma unroll
    for (int u = 0; u < U; ++u) pos[u] = 0;
    for (int len = top >> 1; len > 0; len >>= 1) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int cand = pos[u] + len;
            const int at = cand <= n ? cand : n;   // (stay inside the table; the result is discarded when cand > n)
            pos[u] = (cand <= n && lo_of(base + at - 1) <= val(u)) ? cand : pos[u];
        }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int j = pos[u] - 1;
        in[u] = in[u] && j >= 0 && val(u) < hi_of(base + (j < 0 ? 0 : j));
        idx[u] = idx[u] * n + (j < 0 ? 0 : j);
    }
}

}  // namespace xd
