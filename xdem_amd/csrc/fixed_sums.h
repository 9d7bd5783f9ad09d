// fixed_sums.h -- float64 sums added in a fixed order, so that two calls return the same bits: the one home of what the moments of
// Deramp (biascorr.hip), the normal equations of LZD (rigid.hip), the sums of ICP (icp.hip) and the M-step of CPD (cpd.hip) share.
//
// FOR TRANSLATION UNITS BUILT WITH -ffp-contract=off: the terms reproduce NumPy's arithmetic only without contraction.
//
// The order, which is the contract:
//   1. a lane adds its own elements in the order its kernel visits them;
//   2. wave_sum: xor shuffles over the 64 lanes, offsets 32 down to 1;
//   3. block_sum: the four waves of a 256-lane workgroup as ((w0 + w1) + w2) + w3;
//   4. one partial per workgroup and term, part[b * nt + t] (the count, where there is one, in the last slot);
//   5. the reduce kernel (biascorr.hip): one workgroup per term, lane l adds the partials l, l + 256, ... in order, then a halving tree
//      over the 256 lanes.
// The grid is min(num_cu * 8, units), at least 1: it depends on the device and the input only, never on the call.
#pragma once
#include "common.h"

namespace xd {

template <typename V> __device__ __forceinline__ V wave_sum(V x) {
    for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off, 64);
    return x;
}

// sum over the workgroup (256 lanes = 4 waves): wave shuffles, then the four waves in order.  `red`: 4 values of LDS.
template <typename V> __device__ __forceinline__ V block_sum(V x, V* red) {
    x = wave_sum<V>(x);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = x;
    __syncthreads();
    const V r = ((red[0] + red[1]) + red[2]) + red[3];
    __syncthreads();
    return r;
}

// the end of a sums kernel: the N per-lane sums and the count, each summed over the workgroup, into the workgroup's row of `part`
template <int N> __device__ __forceinline__ void block_sums_store(const double* s, double cnt, double* red, double* __restrict__ part) {
    double* out = part + (int64_t)blockIdx.x * (N + 1);
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const double v = block_sum<double>(s[k], red);
        if (threadIdx.x == 0) out[k] = v;
    }
    const double v = block_sum<double>(cnt, red);
    if (threadIdx.x == 0) out[N] = v;
}

// ---- host side (defined in biascorr.hip) -----------------------------------------------------------------------------------------
// The partials of one owner (a dh plan, an ICP or CPD object) and the totals behind them: num_cu * 8 + 1 rows of nt doubles, made at the
// first call and kept (nothing is allocated per iteration); grows when a call has more terms.
struct FixedSums {
    double* part = nullptr;
    int64_t cap = 0;   // doubles
    int reserve(XdOwned& mem, int nt, const char* who);   // from the owner of whoever holds the sums; XDEMHIP_ENOMEM: "hipMalloc failed (who)"
};
// the workgroups of a sums kernel over `units` units of work (tiles, rows, runs of 256 elements)
inline int fixed_sums_grid(const xdemhip_ctx* ctx, int64_t units) {
    int64_t nb = (int64_t)ctx->num_cu * 8;
    if (nb > units) nb = units;
    return nb < 1 ? 1 : (int)nb;
}
// The reduce kernel alone, for sums whose totals the next kernel reads (the two stages of CPD's M-step): `part` holds `nblocks` rows of
// `nt` partials, the totals land behind them at part + nblocks * nt; the check of both launches ("`what` launch failed").
int fixed_sums_reduce(xdemhip_ctx* ctx, double* part, int nblocks, int nt, const char* what);
// What follows a sums kernel that wrote `nblocks` rows of `nt` partials: the reduce kernel, the check of both launches ("`what` launch
// failed"), ev_stop, ctx->timed, the one fetch of the nt totals, xd_sync.
int fixed_sums_finish(xdemhip_ctx* ctx, const FixedSums& fs, int nblocks, int nt, const char* what, double* totals);

}  // namespace xd
