// variogram.hip -- pairwise lag binning of the empirical variogram on gfx950.
//
// Replaces the pairwise work the reference hands to scikit-gstat from sample_empirical_variogram
// (xdem/spatialstats.py:1091 pdist, 1247-1255 cdist): for every pair of a "pair block" (every point of set A with
// every point of set B, or all i < j inside A) take the Euclidean distance d and the absolute value difference,
// assign the lag class k with e_{k-1} <= d < e_k from explicit right edges, and reduce per class:
//   sums   -> count and sum(diff^2) (Matheron) or sum(sqrt diff) (Cressie-Hawkins)
//   hist   -> one 8-bit digit histogram of the diff keys per class (exact median for Dowd, select.h)
//   succ   -> smallest key above the selected one (upper median of an even-sized class)
// This is O(N^2) arithmetic over O(N) bytes: points are staged in LDS and re-used 256x, HBM traffic is negligible
// and the bound is VALU + LDS-atomic throughput (no MFMA: there is no contraction, every pair ends in a scatter).
//
// One workgroup = 256 points of A (one per lane, in registers) x a chunk of B streamed through LDS in tiles of 256
// (all lanes read the same B element: LDS broadcast, conflict-free).  Class lookup is a binary search over
// thresholds on the SQUARED distance that are exact images of the edges under sqrt (computed on the host), so the
// class is bit-identical to comparing the rounded float64 distance with the edges.  Accumulators live in LDS
// (ds_add_u32 / ds_add_f64 / ds_min) and are flushed once per workgroup with global atomics; counts and histograms
// are integers, hence exact and all-reducible across GPUs.
//
// This file: the pair set (xdemhip_pairs), the launch, the C entry points and the selection driver.  The kernel is pairs_kernel.h;
// the host arithmetic behind every pair's class pairs_classes.h, the kernel's LDS block pairs_layout.h, the decisions of the
// bracketed selection pairs_policy.h -- those three are plain C++ and tested on the CPU (tests/test_pairs_host.py).
#include <math.h>
#include <type_traits>
#include <string.h>
#include <vector>
#include <stdio.h>
#include <time.h>
#include <stdlib.h>

#include "common.h"
#include "select.h"
#include "select_run.h"
#include "pairs_kernel.h"
#include "pairs_policy.h"

using namespace xd;

struct xdemhip_pairs {
    xdemhip_ctx* ctx = nullptr;
    int val_dtype = XDEMHIP_F32, nblk = 0, nb = 0, pdist = 0;
    XdOwned mem;   // every device buffer of the set but the caller's own device arrays
    double *ax = nullptr, *ay = nullptr, *bx = nullptr, *by = nullptr;   // the caller's device arrays, or owned copies of its host arrays
    void *av = nullptr, *bv = nullptr;
    int64_t *a_off = nullptr, *b_off = nullptr, *wg_off = nullptr, *wg_off_big = nullptr;
    double *thr = nullptr, *sums = nullptr;
    uint8_t* lut = nullptr;  // null when the edges are too dense for the binade table
    int lut_emin = 0;
    // integer-lattice path (make_grid): packed int16 lattice indexes, integer thresholds, class table over float(d2)
    uint32_t *a_xy = nullptr, *b_xy = nullptr, *thr_i = nullptr;
    uint8_t* lut_i = nullptr;
    bool grid = false;
    unsigned long long *counts = nullptr, *hist = nullptr;
    void *prefix = nullptr, *succ = nullptr;
    int64_t n_wg = 0, n_wg_big = 0, n_pairs = 0;
    // bracketed selection state (xdemhip_pairs_medians)
    int sample = 0, has_nan = 1, dual = 0;
    void* prefix2 = nullptr;             // (points into the caller's scratch while a dual pass runs)
    unsigned long long* hist2 = nullptr;
    void* khi = nullptr;
    unsigned long long *cnt3 = nullptr, *cand_ctr = nullptr;
    void* cand_v = nullptr;
    uint16_t* cand_b = nullptr;
    long long cand_cap = 0;
    // the same pair set with the points of every block in Morton order (xdemhip_pairs_link_sorted; not owned): the counting pass
    // of the bracketed selection reads its points
    xdemhip_pairs* sorted = nullptr;
    // a float32 copy of a float64 set whose values are all exactly float32 numbers (xdemhip_pairs_link_shadow; not owned): the
    // bracketed exact-median route runs its passes there and takes float64 candidates (WIDE kernels)
    xdemhip_pairs* shadow = nullptr;
    // small device blocks of xdemhip_pairs_medians, kept between calls (their hipMalloc / hipFree cost ~1 ms per call)
    unsigned char* sel_small = nullptr;
    size_t sel_small_bytes = 0;
    void* sel_scratch = nullptr;
    size_t sel_scratch_bytes = 0;
    std::vector<int64_t> h_a_off, h_b_off;   // host copies of the block offsets (link check)
};

namespace {

template <typename T, int OP, bool WIDE = false> int launch_pairs(xdemhip_pairs* P, int shift, int first, int bin0, int nbs) {
    xdemhip_ctx* ctx = P->ctx;
    constexpr int NT = (OP == OP_HIST || OP == OP_BRACKET) ? 1024 : 256;  // histograms: 16 waves share one 51 KB LDS table -> full occupancy
    PairArgs<T> a;
    a.ax = P->ax; a.ay = P->ay; a.bx = P->bx; a.by = P->by;
    a.av = static_cast<const T*>(P->av); a.bv = static_cast<const T*>(P->bv);
    a.a_off = P->a_off; a.b_off = P->b_off; a.wg_off = (NT == 1024) ? P->wg_off_big : P->wg_off;
    a.nblk = P->nblk; a.nb = P->nb; a.pdist = P->pdist; a.thr = P->thr; a.lut = P->lut; a.lut_emin = P->lut_emin;
    a.a_xy = P->a_xy; a.b_xy = P->b_xy; a.thr_i = P->thr_i; a.lut_i = P->lut_i;
    a.sums = P->sums; a.counts = P->counts; a.hist = P->hist;
    a.prefix = static_cast<const typename KeyT<T>::type*>(P->prefix);
    a.succ = static_cast<unsigned long long*>(P->succ);
    a.shift = shift; a.first = first; a.bin0 = bin0; a.nbs = nbs;
    a.sample = P->sample;
    a.dual = (OP == OP_HIST) ? P->dual : 0;
    a.prefix2 = static_cast<const typename KeyT<T>::type*>(P->prefix2);
    a.hist2 = P->hist2;
    a.has_nan = P->has_nan;
    a.khi = static_cast<const typename KeyT<T>::type*>(P->khi);
    a.cnt3 = P->cnt3; a.cand_v = P->cand_v; a.cand_b = P->cand_b; a.cand_ctr = P->cand_ctr; a.cand_cap = P->cand_cap;
    a.runs = 0;
    if (OP == OP_BRACKET && P->sorted && ctx->vario_runs != 0) {
        // same blocks, same offsets, other slot order: counts and candidates are the same multiset
        const xdemhip_pairs* S = P->sorted;
        a.ax = S->ax; a.ay = S->ay; a.bx = S->bx; a.by = S->by;
        a.av = static_cast<const T*>(S->av); a.bv = static_cast<const T*>(S->bv);
        a.a_xy = S->a_xy; a.b_xy = S->b_xy;
        a.runs = 1;
    }
    const size_t lds = pairs_lds_bytes<T, OP, WIDE>(P->nb, (OP == OP_HIST && P->dual) ? 2 * nbs : nbs);
    const int64_t n_wg = (NT == 1024) ? P->n_wg_big : P->n_wg;
    // HIP dispatches carry the TOTAL work-item count of a dimension in 32 bits (a larger grid x block product is silently
    // truncated): a pass over more workgroups than 2^31 / NT goes out as several launches, each told where it starts.
    const int64_t per_launch = ctx->pairs_launch_cap > 0 ? (int64_t)ctx->pairs_launch_cap : ((int64_t)1 << 31) / NT;
    // the route of the class lookup: integer lattice, binade table over d^2, or binary search
    const bool grid = P->grid && ctx->vario_grid != 0;
    void (*const kernel)(PairArgs<T>) = grid     ? pairs_kernel<T, OP, true, NT, true, WIDE>
                                        : P->lut ? pairs_kernel<T, OP, true, NT, false, WIDE>
                                                 : pairs_kernel<T, OP, false, NT, false, WIDE>;
    if (int rc = set_big_lds(ctx, kernel, lds)) return rc;
    for (int64_t w0 = 0; w0 < n_wg; w0 += per_launch) {
        const int64_t nw = (n_wg - w0) < per_launch ? (n_wg - w0) : per_launch;
        a.wg_base = w0;
        a.wg_end = w0 + nw;
        // sampled digit passes: resident workgroups walking over the units (see the kernel); everything else one unit each
        const int64_t resident = (int64_t)ctx->num_cu * (lds > 80 * 1024 ? 1 : 2);
        const unsigned nlaunch = (unsigned)((OP == OP_HIST && P->sample && nw > resident) ? resident : nw);
        hipLaunchKernelGGL(kernel, dim3(nlaunch), dim3(NT), lds, ctx->stream, a);
        XD_HIP_CHECK(ctx, hipGetLastError());
    }
    return XDEMHIP_OK;
}

// the caller's 64-bit keys (one per class) into P->prefix, narrowed to the key width of the set's values
int upload_keys(xdemhip_pairs* P, const uint64_t* keys) {
    xdemhip_ctx* ctx = P->ctx;
    if (P->val_dtype == XDEMHIP_F32) {
        std::vector<uint32_t> k32(P->nb);
        for (int k = 0; k < P->nb; ++k) k32[k] = (uint32_t)keys[k];
        XD_HIP_CHECK(ctx, hipMemcpy(P->prefix, k32.data(), 4 * P->nb, hipMemcpyHostToDevice));
    } else {
        XD_HIP_CHECK(ctx, hipMemcpy(P->prefix, keys, 8 * P->nb, hipMemcpyHostToDevice));
    }
    return XDEMHIP_OK;
}

template <int OP> int launch_any(xdemhip_pairs* P, int shift = 0, int first = 0, int bin0 = 0, int nbs = 0) {
    return P->val_dtype == XDEMHIP_F32 ? launch_pairs<float, OP>(P, shift, first, bin0, nbs)
                                       : launch_pairs<double, OP>(P, shift, first, bin0, nbs);
}

}  // namespace

extern "C" {

void xdemhip_pairs_destroy(xdemhip_pairs* P) { delete P; }   // (its owner frees the device buffers)

int xdemhip_pairs_create(xdemhip_ctx* ctx, int n_blocks, const int64_t* a_off, const double* ax, const double* ay, const void* av,
                         const int64_t* b_off, const double* bx, const double* by, const void* bv, int val_dtype,
                         const double* right_edges, int n_bins, int memspace, xdemhip_pairs** out, int64_t* n_pairs) {
    if (!ctx) return XDEMHIP_EINVAL;
    if (!out || n_blocks <= 0 || !a_off || !ax || !ay || !av || !right_edges) return xd_fail(ctx, XDEMHIP_EINVAL, "bad argument");
    if (n_bins < 1 || n_bins > 1024) return xd_fail(ctx, XDEMHIP_EINVAL, "n_bins out of range (1..1024)");
    if (val_dtype != XDEMHIP_F32 && val_dtype != XDEMHIP_F64) return xd_fail(ctx, XDEMHIP_EINVAL, "values must be float32 or float64");
    const bool pd = (b_off == nullptr);
    if (!pd && (!bx || !by || !bv)) return xd_fail(ctx, XDEMHIP_EINVAL, "null B arrays");
    for (int k = 1; k < n_bins; ++k)
        if (!(right_edges[k] > right_edges[k - 1])) return xd_fail(ctx, XDEMHIP_EINVAL, "right_edges must be strictly increasing");
    XD_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    // context option "vario_diff" = 1: |dv| in float64 whatever the value dtype (SciPy's pdist / cdist, which scikit-gstat builds
    // on, widen to float64 first): float32 values are widened here, every pass then runs the float64 instantiation
    std::vector<double> wide_a, wide_b;
    if (ctx->vario_diff && val_dtype == XDEMHIP_F32 && memspace == XDEMHIP_HOST) {
        const int64_t na0 = a_off[n_blocks], nb0 = pd ? 0 : b_off[n_blocks];
        wide_a.resize((size_t)na0);
        for (int64_t i = 0; i < na0; ++i) wide_a[(size_t)i] = (double)static_cast<const float*>(av)[i];
        av = wide_a.data();
        if (!pd) {
            wide_b.resize((size_t)nb0);
            for (int64_t i = 0; i < nb0; ++i) wide_b[(size_t)i] = (double)static_cast<const float*>(bv)[i];
            bv = wide_b.data();
        }
        val_dtype = XDEMHIP_F64;
    }
    xdemhip_pairs* P = new xdemhip_pairs();
    P->ctx = P->mem.ctx = ctx; P->val_dtype = val_dtype; P->nblk = n_blocks; P->nb = n_bins; P->pdist = pd;
    const size_t es = val_dtype == XDEMHIP_F32 ? 4 : 8;
    const int64_t na = a_off[n_blocks], nbt = pd ? 0 : b_off[n_blocks];
    std::vector<int64_t> wg(n_blocks + 1, 0), wgb(n_blocks + 1, 0);
    int64_t pairs = 0;
    for (int r = 0; r < n_blocks; ++r) {
        const int64_t a = a_off[r + 1] - a_off[r], b = pd ? a : b_off[r + 1] - b_off[r];
        if (a < 0 || b < 0) { delete P; return xd_fail(ctx, XDEMHIP_EINVAL, "offsets must be non-decreasing"); }
        wg[r + 1] = wg[r] + ((a + 255) / 256) * ((b + BCHUNK - 1) / BCHUNK);
        wgb[r + 1] = wgb[r] + ((a + 1023) / 1024) * ((b + BCHUNK - 1) / BCHUNK);
        pairs += pd ? a * (a - 1) / 2 : a * b;
    }
    P->n_wg = wg[n_blocks];
    P->n_wg_big = wgb[n_blocks];
    P->n_pairs = pairs;
    P->h_a_off.assign(a_off, a_off + n_blocks + 1);
    if (!pd) P->h_b_off.assign(b_off, b_off + n_blocks + 1);
    std::vector<double> thr(n_bins);
    // context option "vario_edge": 0 = classes [e_{k-1}, e_k) (default), 1 = (e_{k-1}, e_k]
    for (int k = 0; k < n_bins; ++k) thr[k] = ctx->vario_edge ? sq_threshold_strict(right_edges[k]) : sq_threshold(right_edges[k]);
    // class lookup table over the 1/8 binades of d^2 (pairs_classes.h); edges too dense for it: binary search
    std::vector<uint8_t> lut;
    const bool lut_ok = build_binade_lut(thr, lut, P->lut_emin);
    // (every host array read below outlives the synchronisation that ends the uploads)
    const char* who = "xdemhip_pairs_create";
    const size_t offs = sizeof(int64_t) * (size_t)(n_blocks + 1), nbin = (size_t)n_bins;
    XdOwned& mem = P->mem;
    GridInfo gi;
    P->a_off = mem.keep(a_off, offs, XDEMHIP_HOST, who);
    P->wg_off = mem.keep(wg.data(), offs, XDEMHIP_HOST, who);
    P->wg_off_big = mem.keep(wgb.data(), offs, XDEMHIP_HOST, who);
    P->thr = mem.keep(thr.data(), 8 * nbin, XDEMHIP_HOST, who);
    P->sums = mem.take<double>(nbin, who);
    P->counts = mem.take<unsigned long long>(nbin, who);
    P->hist = mem.take<unsigned long long>(nbin * SEL_RADIX, who);
    P->hist2 = mem.take<unsigned long long>(nbin * SEL_RADIX, who);
    P->prefix = mem.take(8 * nbin, who);
    P->succ = mem.take(8 * nbin, who);
    P->b_off = mem.keep(b_off, offs, XDEMHIP_HOST, who);   // (null for a pdist set)
    if (lut_ok) P->lut = mem.keep(lut.data(), LUT_N, XDEMHIP_HOST, who);
    P->ax = mem.keep(ax, 8 * (size_t)na, memspace, who);
    P->ay = mem.keep(ay, 8 * (size_t)na, memspace, who);
    P->av = mem.keep(av, es * (size_t)na, memspace, who);
    if (!pd || memspace == XDEMHIP_DEVICE) {
        P->bx = mem.keep(bx, 8 * (size_t)nbt, memspace, who);
        P->by = mem.keep(by, 8 * (size_t)nbt, memspace, who);
        P->bv = mem.keep(bv, es * (size_t)nbt, memspace, who);
    }
    if (memspace == XDEMHIP_HOST) {
        // NaN values never pair (the kernel tests for them); knowing that there are none lets full tiles skip the test
        auto any_nan = [&](const void* v, int64_t n) {
            if (val_dtype == XDEMHIP_F32) { const float* f = static_cast<const float*>(v); for (int64_t i = 0; i < n; ++i) if (f[i] != f[i]) return true; }
            else { const double* f = static_cast<const double*>(v); for (int64_t i = 0; i < n; ++i) if (f[i] != f[i]) return true; }
            return false;
        };
        P->has_nan = (any_nan(av, na) || (!pd && any_nan(bv, nbt))) ? 1 : 0;
        // raster-sampled points (the reference's samplers draw pixels): integer-lattice kernels
        if (lut_ok && ctx->vario_grid != 0 && make_grid(ax, ay, na, pd ? nullptr : bx, pd ? nullptr : by, nbt, thr, gi)) {
            P->a_xy = mem.keep(gi.a_xy.data(), 4 * (size_t)na, XDEMHIP_HOST, who);
            P->thr_i = mem.keep(gi.thr_i.data(), 4 * nbin, XDEMHIP_HOST, who);
            P->lut_i = mem.keep(gi.lut.data(), LUT_G, XDEMHIP_HOST, who);
            if (!pd) P->b_xy = mem.keep(gi.b_xy.data(), 4 * (size_t)nbt, XDEMHIP_HOST, who);
            P->grid = true;
        }
    }
    int rc = mem.rc;
    if (rc == XDEMHIP_OK && hipStreamSynchronize(ctx->stream) != hipSuccess) rc = xd_fail(ctx, XDEMHIP_EHIP, "upload failed");
    if (rc) { delete P; return rc; }
    if (n_pairs) *n_pairs = pairs;
    *out = P;
    return XDEMHIP_OK;
}

int xdemhip_pairs_link_sorted(xdemhip_pairs* P, xdemhip_pairs* sorted) {
    if (!P) return XDEMHIP_EINVAL;
    xdemhip_ctx* ctx = P->ctx;
    if (sorted == P) sorted = nullptr;
    if (sorted) {
        if (sorted->ctx != ctx || sorted->val_dtype != P->val_dtype || sorted->nblk != P->nblk || sorted->nb != P->nb ||
            sorted->pdist != P->pdist || sorted->grid != P->grid || sorted->h_a_off != P->h_a_off || sorted->h_b_off != P->h_b_off ||
            sorted->has_nan != P->has_nan)
            return xd_fail(ctx, XDEMHIP_EINVAL, "pairs_link_sorted: the two sets must hold the same blocks (sizes, dtype, edges, context)");
        std::vector<double> t0(P->nb), t1(P->nb);
        XD_HIP_CHECK(ctx, hipSetDevice(ctx->device));
        XD_HIP_CHECK(ctx, hipMemcpy(t0.data(), P->thr, 8 * (size_t)P->nb, hipMemcpyDeviceToHost));
        XD_HIP_CHECK(ctx, hipMemcpy(t1.data(), sorted->thr, 8 * (size_t)P->nb, hipMemcpyDeviceToHost));
        if (memcmp(t0.data(), t1.data(), 8 * (size_t)P->nb) != 0)
            return xd_fail(ctx, XDEMHIP_EINVAL, "pairs_link_sorted: the two sets must hold the same lag edges");
    }
    P->sorted = sorted;
    return XDEMHIP_OK;
}

int xdemhip_pairs_sums(xdemhip_pairs* P, int kind, double* sums, int64_t* counts) {
    if (!P) return XDEMHIP_EINVAL;
    xdemhip_ctx* ctx = P->ctx;
    if (!sums || !counts || (kind != 0 && kind != 1)) return xd_fail(ctx, XDEMHIP_EINVAL, "bad argument");
    XD_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    XD_HIP_CHECK(ctx, hipMemsetAsync(P->sums, 0, 8 * P->nb, ctx->stream));
    XD_HIP_CHECK(ctx, hipMemsetAsync(P->counts, 0, 8 * P->nb, ctx->stream));
    int rc = XDEMHIP_OK;
    if (P->n_wg > 0) {
        XD_HIP_CHECK(ctx, hipEventRecord(ctx->ev_start, ctx->stream));
        rc = kind == 0 ? launch_any<OP_SUMS_SQ>(P) : launch_any<OP_SUMS_SQRT>(P);
        (void)hipEventRecord(ctx->ev_stop, ctx->stream);
        ctx->timed = rc == XDEMHIP_OK;
        if (rc) return rc;
    }
    XD_HIP_CHECK(ctx, hipMemcpyAsync(sums, P->sums, 8 * P->nb, hipMemcpyDeviceToHost, ctx->stream));
    XD_HIP_CHECK(ctx, hipMemcpyAsync(counts, P->counts, 8 * P->nb, hipMemcpyDeviceToHost, ctx->stream));
    XD_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return XDEMHIP_OK;
}

int xdemhip_pairs_hist(xdemhip_pairs* P, int shift, int first, const uint64_t* prefix, uint64_t* hist) {
    if (!P) return XDEMHIP_EINVAL;
    xdemhip_ctx* ctx = P->ctx;
    const int key_bits = P->val_dtype == XDEMHIP_F32 ? 32 : 64;
    if (!hist || shift < 0 || shift > key_bits - 8 || (shift & 7) || (!first && !prefix)) return xd_fail(ctx, XDEMHIP_EINVAL, "bad argument");
    XD_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    XD_HIP_CHECK(ctx, hipMemsetAsync(P->hist, 0, 8 * (size_t)P->nb * SEL_RADIX, ctx->stream));
    if (!first)
        if (int rc = upload_keys(P, prefix)) return rc;
    if (P->n_wg > 0) {
        XD_HIP_CHECK(ctx, hipEventRecord(ctx->ev_start, ctx->stream));
        for (int b0 = 0; b0 < P->nb; b0 += HIST_BINS_PER_SWEEP) {
            const int nbs = (P->nb - b0) < HIST_BINS_PER_SWEEP ? (P->nb - b0) : HIST_BINS_PER_SWEEP;
            int rc = launch_any<OP_HIST>(P, shift, first, b0, nbs);
            if (rc) return rc;
        }
        (void)hipEventRecord(ctx->ev_stop, ctx->stream);
        ctx->timed = true;
    }
    XD_HIP_CHECK(ctx, hipMemcpyAsync(hist, P->hist, 8 * (size_t)P->nb * SEL_RADIX, hipMemcpyDeviceToHost, ctx->stream));
    XD_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return XDEMHIP_OK;
}

int xdemhip_pairs_succ(xdemhip_pairs* P, const uint64_t* key, uint64_t* succ) {
    if (!P) return XDEMHIP_EINVAL;
    xdemhip_ctx* ctx = P->ctx;
    if (!key || !succ) return xd_fail(ctx, XDEMHIP_EINVAL, "bad argument");
    XD_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    XD_HIP_CHECK(ctx, hipMemsetAsync(P->succ, 0xFF, 8 * P->nb, ctx->stream));
    if (int rc = upload_keys(P, key)) return rc;
    if (P->n_wg > 0) {
        int rc = launch_any<OP_SUCC>(P);
        if (rc) return rc;
    }
    XD_HIP_CHECK(ctx, hipMemcpyAsync(succ, P->succ, 8 * P->nb, hipMemcpyDeviceToHost, ctx->stream));  // all-ones = none
    XD_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return XDEMHIP_OK;
}

}  // extern "C"

namespace {

template <typename K> __global__ void extract_prefix_kernel(const SelState<K>* st, K* out, int nb) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < nb) out[k] = st[k].prefix;
}

template <typename T> __host__ inline T abs_key_value(typename KeyT<T>::type key) {  // inverse of key_abs
    typename KeyT<T>::type bits = key >> 1;
    T v;
    memcpy(&v, &bits, sizeof(T));
    return v;
}

// What one digit pass is made of, for the plain passes and the dual sampled ones alike: the histogram sweeps over the classes
// (`sweep` classes per launch: what one LDS table holds), the advance of nb selection states by the digit, and their prefixes for
// the next pass's kernels.  The callers keep the order of these pieces, and what lies between them (all-reduces, the dual passes'
// histogram copy), as it was.
template <typename T> int digit_pass_sweeps(xdemhip_pairs* P, int shift, int first, int sweep) {
    if (P->n_wg_big > 0)
        for (int b0 = 0; b0 < P->nb; b0 += sweep) {
            const int nbs = (P->nb - b0) < sweep ? (P->nb - b0) : sweep;
            if (int rc = launch_pairs<T, OP_HIST>(P, shift, first, b0, nbs)) return rc;
        }
    return XDEMHIP_OK;
}
template <typename K> void digit_pass_advance(xdemhip_ctx* ctx, SelState<K>* st, unsigned long long* hist, int nb, int shift, int p, int passes, int mode, uint32_t deff) {
    hipLaunchKernelGGL((select_advance_kernel<K>), dim3(nb), dim3(64), 0, ctx->stream, st, reinterpret_cast<uint64_t*>(hist), nb, shift, (int)(p == 0),
                       (int)(p == passes - 1), mode, (const uint64_t*)nullptr, (const uint32_t*)nullptr, deff);
}
template <typename K> void digit_pass_prefixes(xdemhip_ctx* ctx, const SelState<K>* st, K* out, int nb) {
    hipLaunchKernelGGL((extract_prefix_kernel<K>), dim3((nb + 63) / 64), dim3(64), 0, ctx->stream, st, out, nb);
}

// 8-bit digit passes over all the pairs towards every class's lower median, with the selection state kept on the device;
// histograms go through the all-reduce hook, so sharded pair sets select the same global order statistics.
template <typename T>
int pairs_digit_passes(xdemhip_pairs* P, SelState<typename KeyT<T>::type>* d_st, std::vector<SelState<typename KeyT<T>::type>>& out) {
    typedef typename KeyT<T>::type K;
    xdemhip_ctx* ctx = P->ctx;
    const int nb = P->nb, passes = KeyT<T>::passes;
    XD_HIP_CHECK(ctx, hipMemsetAsync(d_st, 0, sizeof(SelState<K>) * nb, ctx->stream));
    XD_HIP_CHECK(ctx, hipMemsetAsync(P->hist, 0, 8 * (size_t)nb * SEL_RADIX, ctx->stream));
    P->sample = 0;
    for (int p = 0; p < passes; ++p) {
        const int shift = 8 * (passes - 1 - p);
        int rc = digit_pass_sweeps<T>(P, shift, (int)(p == 0), HIST_BINS_PER_SWEEP);
        if (rc == XDEMHIP_OK) rc = xd_allreduce_device(ctx, P->hist, (int64_t)nb * SEL_RADIX, XDEMHIP_RED_SUM_U64);
        if (rc) return rc;
        digit_pass_advance<K>(ctx, d_st, P->hist, nb, shift, p, passes, SEL_MEDIAN, PAIR_DEFF_WIDE);
        digit_pass_prefixes<K>(ctx, d_st, static_cast<K*>(P->prefix), nb);
        XD_HIP_CHECK(ctx, hipGetLastError());
    }
    out.resize(nb);
    XD_HIP_CHECK(ctx, hipMemcpyAsync(out.data(), d_st, sizeof(SelState<K>) * nb, hipMemcpyDeviceToHost, ctx->stream));
    XD_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return XDEMHIP_OK;
}

// Both ends of every class's bracket from ONE set of sampled digit passes: states [0, nb) select the low ends (d_st), states
// [nb, 2 nb) the high ends; the pair kernel counts every sampled pair under each of the two prefixes of its class it matches
// (PairArgs::dual).  `d_pref2` = nb key slots for the second prefix array.
template <typename T>
int pairs_digit_passes_dual(xdemhip_pairs* P, SelState<typename KeyT<T>::type>* d_st, typename KeyT<T>::type* d_pref2, uint32_t wide_deff,
                            std::vector<SelState<typename KeyT<T>::type>>& lo, std::vector<SelState<typename KeyT<T>::type>>& hi, int n_passes) {
    typedef typename KeyT<T>::type K;
    xdemhip_ctx* ctx = P->ctx;
    const int nb = P->nb, passes = KeyT<T>::passes;
    const int run = (n_passes > 0 && n_passes < passes) ? n_passes : passes;
    constexpr int SWEEP = HIST_BINS_PER_SWEEP / 2;   // two [classes][256] tables per sweep in LDS
    XD_HIP_CHECK(ctx, hipMemsetAsync(d_st, 0, sizeof(SelState<K>) * 2 * nb, ctx->stream));
    XD_HIP_CHECK(ctx, hipMemsetAsync(P->hist, 0, 8 * (size_t)nb * SEL_RADIX, ctx->stream));
    XD_HIP_CHECK(ctx, hipMemsetAsync(P->hist2, 0, 8 * (size_t)nb * SEL_RADIX, ctx->stream));
    P->sample = 1; P->dual = 1; P->prefix2 = d_pref2;
    auto leave = [&](int rc) { P->sample = 0; P->dual = 0; P->prefix2 = nullptr; return rc; };
    for (int p = 0; p < run; ++p) {
        const int shift = 8 * (passes - 1 - p);
        int rc = digit_pass_sweeps<T>(P, shift, (int)(p == 0), SWEEP);
        if (rc == XDEMHIP_OK) rc = xd_allreduce_device(ctx, P->hist, (int64_t)nb * SEL_RADIX, XDEMHIP_RED_SUM_U64);
        if (rc == XDEMHIP_OK && p > 0) rc = xd_allreduce_device(ctx, P->hist2, (int64_t)nb * SEL_RADIX, XDEMHIP_RED_SUM_U64);
        if (rc) return leave(rc);
        if (p == 0)   // the first digit's histogram serves both states
            if (hipMemcpyAsync(P->hist2, P->hist, 8 * (size_t)nb * SEL_RADIX, hipMemcpyDeviceToDevice, ctx->stream) != hipSuccess)
                return leave(xd_fail(ctx, XDEMHIP_EHIP, "histogram copy failed"));
        digit_pass_advance<K>(ctx, d_st, P->hist, nb, shift, p, passes, SEL_BRACKET_LO_WIDE, wide_deff);
        digit_pass_advance<K>(ctx, d_st + nb, P->hist2, nb, shift, p, passes, SEL_BRACKET_HI_WIDE, wide_deff);
        digit_pass_prefixes<K>(ctx, d_st, static_cast<K*>(P->prefix), nb);
        digit_pass_prefixes<K>(ctx, d_st + nb, d_pref2, nb);
        if (hipGetLastError() != hipSuccess) return leave(xd_fail(ctx, XDEMHIP_EHIP, "sampled digit pass failed"));
    }
    leave(0);
    lo.resize(nb); hi.resize(nb);
    XD_HIP_CHECK(ctx, hipMemcpyAsync(lo.data(), d_st, sizeof(SelState<K>) * nb, hipMemcpyDeviceToHost, ctx->stream));
    XD_HIP_CHECK(ctx, hipMemcpyAsync(hi.data(), d_st + nb, sizeof(SelState<K>) * nb, hipMemcpyDeviceToHost, ctx->stream));
    XD_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return XDEMHIP_OK;
}

template <typename T>
int pairs_medians_plain(xdemhip_pairs* P, SelState<typename KeyT<T>::type>* d_st, int64_t* counts, double* medians) {
    typedef typename KeyT<T>::type K;
    xdemhip_ctx* ctx = P->ctx;
    const int nb = P->nb;
    std::vector<SelState<K>> st;
    int rc = pairs_digit_passes<T>(P, d_st, st);
    if (rc) return rc;
    // successor of the selected key per class (upper median of even classes); P->prefix holds the selected keys
    XD_HIP_CHECK(ctx, hipMemsetAsync(P->succ, 0xFF, 8 * (size_t)nb, ctx->stream));
    if (P->n_wg > 0) {
        rc = launch_pairs<T, OP_SUCC>(P, 0, 0, 0, 0);
        if (rc) return rc;
    }
    rc = xd_allreduce_device(ctx, P->succ, nb, XDEMHIP_RED_MIN_U64);
    if (rc) return rc;
    std::vector<uint64_t> succ(nb);
    XD_HIP_CHECK(ctx, hipMemcpyAsync(succ.data(), P->succ, 8 * (size_t)nb, hipMemcpyDeviceToHost, ctx->stream));
    XD_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    for (int k = 0; k < nb; ++k) {
        counts[k] = (int64_t)st[k].count;
        if (st[k].count == 0) { medians[k] = NAN; continue; }
        const T lo = abs_key_value<T>(st[k].prefix);
        if (st[k].count & 1) { medians[k] = (double)lo; continue; }
        const uint64_t k2 = st[k].count / 2;
        const T hi = (st[k].n_le > k2) ? lo : abs_key_value<T>((K)succ[k]);
        medians[k] = (double)(T)((T)(lo + hi) / (T)2);
    }
    return XDEMHIP_OK;
}

// XDEMHIP_DEBUG: the time of every phase of a selection on stderr (each line costs a stream synchronisation)
struct PhaseTimer {
    xdemhip_ctx* ctx;
    bool on;
    double t = 0.0;
    explicit PhaseTimer(xdemhip_ctx* c) : ctx(c), on(getenv("XDEMHIP_DEBUG") != nullptr) { if (on) t = now_ms(); }
    double now_ms() const { (void)hipStreamSynchronize(ctx->stream); timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); return ts.tv_sec * 1e3 + ts.tv_nsec * 1e-6; }
    void phase(const char* what) { if (on) { const double n = now_ms(); fprintf(stderr, "[xdemhip] pair medians: %-28s %8.2f ms\n", what, n - t); t = n; } }
};

// One exact-median selection over a pair set: the stages of the bracketed route (every decision: pairs_policy.h) and what they
// share.  WIDE (T = float): `P` is the float32 shadow of a float64 set (xdemhip_pairs_link_shadow) -- sampled passes and the
// counting pass in float32, candidates and their selection in float64 (see pairs_kernel).
template <typename T, bool WIDE> struct PairsSelection {
    typedef typename KeyT<T>::type K;
    typedef typename CandT<T, WIDE>::type TC;      // candidate values ...
    typedef typename KeyT<TC>::type KC;            // ... and their keys
    static constexpr int BR_PASSES = 3;            // 24 leading key bits place the bracket ends finely enough
    xdemhip_pairs* P;
    xdemhip_ctx* ctx;
    int nb;
    PhaseTimer timer;
    // small device block: selection states | klo | khi | given | counters[3 nb] | candidate counter, overflow | rebase shift | second prefixes
    unsigned char* d_small = nullptr;
    size_t off_klo, off_khi, off_given, off_cnt, off_ctr, off_rbs, off_pref2, small_bytes;
    void* scratch = nullptr;
    std::vector<K> klo, khi;                 // the brackets, as keys of the pair passes
    std::vector<uint64_t> lo_count;          // sampled pairs per class
    std::vector<KC> rb_lo;                   // rebase origins of the candidate keys
    uint32_t rbs = 0;                        // ... and their common shift
    std::vector<uint64_t> cnt, given;        // [3][nb] total, below, inside; rank among the candidates per class
    uint64_t ctr[2] = {0, 0};                // candidates, overflow flag

    explicit PairsSelection(xdemhip_pairs* P_) : P(P_), ctx(P_->ctx), nb(P_->nb), timer(P_->ctx), klo(nb), khi(nb), lo_count(nb, 0), cnt(3 * (size_t)nb), given(nb) {
        off_klo = 2 * (size_t)nb * sizeof(SelState<K>); off_khi = off_klo + 8 * (size_t)nb; off_given = off_khi + 8 * (size_t)nb;
        off_cnt = off_given + 8 * (size_t)nb; off_ctr = off_cnt + 24 * (size_t)nb; off_rbs = off_ctr + 16; off_pref2 = off_rbs + 8;
        small_bytes = off_pref2 + 8 * (size_t)nb;
    }
    SelState<K>* d_st() const { return reinterpret_cast<SelState<K>*>(d_small); }
    KC* d_klo() const { return reinterpret_cast<KC*>(d_small + off_klo); }   // (8-byte slots: rebase origins of the CANDIDATE keys)
    uint32_t* d_rbs() const { return reinterpret_cast<uint32_t*>(d_small + off_rbs); }
    uint64_t* d_given() const { return reinterpret_cast<uint64_t*>(d_small + off_given); }
    void cleanup() {
        // (the candidate buffers and the small blocks stay with the pair set -- tens of GB whose hipMalloc and first touch cost a
        // second: a second selection on the same set, e.g. after a warm-up call, reuses them; xdemhip_pairs_destroy frees them)
        P->khi = nullptr; P->cnt3 = nullptr; P->cand_ctr = nullptr;
    }

    // stage: the small block every route needs
    int workspace() {
        if (P->sel_small_bytes < small_bytes) {
            P->sel_small_bytes = P->mem.regrow(P->sel_small, small_bytes, "xdemhip_pairs_medians") ? small_bytes : 0;
            { const int rc_ = P->mem.status(); if (rc_) return rc_; }
        }
        d_small = P->sel_small;
        return XDEMHIP_OK;
    }
    // stage: does this set take the bracketed route -- by the policy, with its scratch block, and on every rank alike
    int route(bool& bracket) {
        bracket = pairs_route_brackets(ctx->selection_mode, nb, P->n_pairs, P->n_wg_big);
        if (bracket) {
            const size_t need = scratch_size(nb);
            if (P->sel_scratch_bytes < need) {
                P->mem.drop(P->sel_scratch);
                P->mem.optional();   // (too little memory: plain passes)
                P->sel_scratch = P->mem.take(need, "xdemhip_pairs_medians");
                bracket = P->mem.all_or_none(P->sel_scratch);
                P->sel_scratch_bytes = bracket ? need : 0;
            }
            scratch = P->sel_scratch;
        }
        if (ctx->allreduce) {  // sharded pair sets: every rank must take the same route
            uint64_t can = bracket ? 1 : 0;
            if (ctx->allreduce(&can, 1, XDEMHIP_RED_MIN_U64, ctx->allreduce_user) != 0) return xd_fail(ctx, XDEMHIP_EHIP, "all-reduce hook failed");
            bracket = can != 0;
        }
        return XDEMHIP_OK;
    }
    // stage: both ends of every class's bracket from one set of sampled digit passes; `expected` = candidates the brackets should hold
    int sampled_ends(uint32_t deff, double& expected) {
        std::vector<SelState<K>> lo, hi;
        const K low_mask = (K)(((K)1 << (8 * (KeyT<T>::passes - BR_PASSES))) - 1);
        const int rc = pairs_digit_passes_dual<T>(P, d_st(), reinterpret_cast<K*>(d_small + off_pref2), deff, lo, hi, BR_PASSES);
        if (rc) return rc;
        timer.phase("sampled digit passes");
        expected = 0.0;
        for (int k = 0; k < nb; ++k) {
            lo_count[k] = lo[k].count;
            pairs_bracket_ends<K>(lo[k].count, lo[k].prefix, hi[k].prefix, low_mask, ctx->selection_mode, klo[k], khi[k]);
            expected += pairs_expected_candidates(lo[k].count, sel_bracket_halfwidth_wide(lo[k].count, deff), P->pdist ? 64.0 : (double)(PT / SPREAD_SLOTS));
        }
        return XDEMHIP_OK;
    }
    // stage: candidate buffers sized from the brackets, not from the pair count.  Too little memory (on any rank): *have = false, plain passes.
    int candidate_buffers(double expected, bool& have) {
        const long long need = pairs_candidate_capacity(expected, P->n_pairs);
        uint64_t got = 1;
        if (P->cand_cap < need) {
            P->mem.drop(P->cand_v);
            P->mem.drop(P->cand_b);
            P->mem.optional();
            P->cand_v = P->mem.take((size_t)need * sizeof(TC), "xdemhip_pairs_medians");
            P->cand_b = P->mem.take<uint16_t>((size_t)need, "xdemhip_pairs_medians");
            got = P->mem.all_or_none(P->cand_v, P->cand_b) ? 1 : 0;
            P->cand_cap = got ? need : 0;
        }
        if (ctx->allreduce && ctx->allreduce(&got, 1, XDEMHIP_RED_MIN_U64, ctx->allreduce_user) != 0) return xd_fail(ctx, XDEMHIP_EHIP, "all-reduce hook failed");
        if (!got) {   // (another rank's shortage: this rank's buffers go too)
            P->mem.drop(P->cand_v);
            P->mem.drop(P->cand_b);
            P->cand_v = nullptr; P->cand_b = nullptr; P->cand_cap = 0;
        }
        have = got != 0;
        return XDEMHIP_OK;
    }
    // stage: the ONE pass over all pairs -- counts per class against the brackets, candidates compacted; the counters come back summed over the ranks
    int counting_pass() {
        K* d_khi = reinterpret_cast<K*>(d_small + off_khi);
        P->cnt3 = reinterpret_cast<unsigned long long*>(d_small + off_cnt);
        P->cand_ctr = reinterpret_cast<unsigned long long*>(d_small + off_ctr);
        P->khi = d_khi;
        hipError_t e = hipMemcpyAsync(P->prefix, klo.data(), sizeof(K) * nb, hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(d_khi, khi.data(), sizeof(K) * nb, hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) e = hipMemsetAsync(d_small + off_cnt, 0, 24 * (size_t)nb + 16, ctx->stream);
        // candidate keys are rebased for their selection (select_run.h, hist_pass_kernel): origins and the common shift
        rbs = rebase_shift_of(pairs_rebase_origins<WIDE, K, KC>(klo, khi, rb_lo));
        if (e == hipSuccess) e = hipMemcpyAsync(d_klo(), rb_lo.data(), sizeof(KC) * nb, hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(d_rbs(), &rbs, 4, hipMemcpyHostToDevice, ctx->stream);
        if (e != hipSuccess) return xd_fail(ctx, XDEMHIP_EHIP, "bracket setup failed");
        int rc = XDEMHIP_OK;
        if (P->n_wg_big > 0) {
            XD_HIP_CHECK(ctx, hipEventRecord(ctx->ev_start, ctx->stream));
            rc = launch_pairs<T, OP_BRACKET, WIDE>(P, 0, 0, 0, 0);
            (void)hipEventRecord(ctx->ev_stop, ctx->stream);
            ctx->timed = rc == XDEMHIP_OK;
        }
        if (rc == XDEMHIP_OK) rc = xd_allreduce_device(ctx, P->cnt3, 3 * (int64_t)nb, XDEMHIP_RED_SUM_U64);
        if (rc == XDEMHIP_OK) rc = xd_allreduce_device(ctx, P->cand_ctr + 1, 1, XDEMHIP_RED_SUM_U64);
        if (rc) return rc;
        e = hipMemcpyAsync(cnt.data(), P->cnt3, 24 * (size_t)nb, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(ctr, P->cand_ctr, 16, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) return xd_fail(ctx, XDEMHIP_EHIP, std::string("bracket pass failed: ") + hipGetErrorString(e));
        timer.phase("counting + compaction pass");
        if (timer.on) fprintf(stderr, "[xdemhip] pair medians: %llu candidates (%.2f %% of the pairs)\n", (unsigned long long)ctr[0], 100.0 * (double)ctr[0] / (double)P->n_pairs);
        for (int k = 0; k < nb; ++k) cnt[k] += cnt[nb + k];  // class total = (keys >= low end) + (keys below it)
        return XDEMHIP_OK;
    }
    // stage: the rank of every class's median among its candidates; false: a bracket missed its rank or the candidates overflowed
    bool ranks() {
        if (timer.on) {  // how far from the bracket's centre the wanted rank lies, in half widths (1 = the bracket just missed)
            double worst = 0.0, sum2 = 0.0;
            int nn = 0, kw = -1;
            for (int k = 0; k < nb; ++k) {
                const double total = (double)cnt[k], lt = (double)cnt[nb + k], in = (double)cnt[2 * nb + k];
                if (total < 1.0 || in < 1.0 || lo_count[k] == 0) continue;
                if (in >= total) continue;  // the bracket holds the whole class
                const double off = fabs(((total - 1.0) * 0.5 - lt) - 0.5 * in) / (0.5 * in);
                sum2 += off * off; ++nn;
                if (off > worst) { worst = off; kw = k; }
            }
            fprintf(stderr, "[xdemhip] pair medians: wanted rank off the bracket centre by %.3f half widths at worst (class %d), rms %.3f over %d classes\n",
                    worst, kw, nn ? sqrt(sum2 / nn) : 0.0, nn);
        }
        const int missed = pairs_ranks_from_counts(&cnt[0], &cnt[nb], &cnt[2 * nb], nb, ctr[1] != 0, given.data());
        if (missed >= 0 && timer.on)
            fprintf(stderr, "[xdemhip] pair medians: bracket of class %d missed (total %llu, below %llu, inside %llu, rank %llu, sample %llu)\n",
                    missed, (unsigned long long)cnt[missed], (unsigned long long)cnt[nb + missed], (unsigned long long)cnt[2 * nb + missed],
                    (unsigned long long)((cnt[missed] - 1) / 2), (unsigned long long)lo_count[missed]);
        if (missed != -1 && timer.on) fprintf(stderr, "[xdemhip] pair medians: candidate overflow flag %llu, candidates %llu of %lld\n",
                                              (unsigned long long)ctr[1], (unsigned long long)ctr[0], (long long)P->cand_cap);
        return missed == -1;
    }
    // stage: the order statistics among the candidates (select_run.h), and from them counts and medians
    int select_and_results(int64_t* counts, double* medians) {
        if (hipMemcpyAsync(d_given(), given.data(), 8 * (size_t)nb, hipMemcpyHostToDevice, ctx->stream) != hipSuccess)
            return xd_fail(ctx, XDEMHIP_EHIP, "bracket ranks upload failed");
        std::vector<SelResult<KC>> res;
        int rc = select_enqueue<TC>(ctx, static_cast<const TC*>(P->cand_v), P->cand_b, (int64_t)ctr[0], (int64_t)ctr[0], nullptr, nb,
                                    static_cast<unsigned char*>(scratch), SEL_GIVEN, d_given(), 0, true, d_klo(), d_rbs());
        if (rc == XDEMHIP_OK) rc = select_fetch<TC>(ctx, static_cast<unsigned char*>(scratch), nb, res);
        if (rc) return rc;
        timer.phase("selection among candidates");
        for (int k = 0; k < nb; ++k) {
            counts[k] = (int64_t)cnt[k];
            if (cnt[k] == 0) { medians[k] = NAN; continue; }
            res[k].st.count = cnt[k];
            res[k].st.n_le += cnt[nb + k];
            res[k].st.prefix = (KC)((KC)(res[k].st.prefix >> rbs) + rb_lo[k]);  // back from the rebased keys
            if (res[k].succ != ~(uint64_t)0) res[k].succ = (uint64_t)(KC)((KC)((KC)res[k].succ >> rbs) + rb_lo[k]);
            medians[k] = median_from<TC>(res[k]);
        }
        return XDEMHIP_OK;
    }
};

// The driver: up to three attempts at the bracketed route, each with the design effect the policy names for it (a bracket that
// missed its rank -- the integer counts tell -- costs one more attempt; with a reduction hook the counts are global, so every rank
// retries alike), then the plain digit passes.  WIDE: returns with *answered = false instead of taking the plain passes when the
// bracketed route does not apply or fails (the caller then runs the float64 set's own route).
template <typename T, bool WIDE = false>
int pairs_medians_typed(xdemhip_pairs* P, int64_t* counts, double* medians, bool* answered = nullptr) {
    if (answered) *answered = false;
    PairsSelection<T, WIDE> s(P);
    int rc = s.workspace();
    if (rc) return rc;
    bool bracket = false, done = false;
    rc = s.route(bracket);
    uint32_t deff = 0;
    for (int attempt = 0; attempt < 3 && rc == XDEMHIP_OK && bracket && !done; ++attempt) {
        deff = pairs_attempt_deff(attempt, deff, P->pdist != 0, PAIR_DEFF_WIDE, PAIR_DEFF_SPREAD);
        if (!deff) break;
        if (attempt >= 1 && s.timer.on) fprintf(stderr, "[xdemhip] pair medians: attempt %d with design effect %u\n", attempt + 1, deff);
        double expected = 0.0;
        rc = s.sampled_ends(deff, expected);
        if (rc == XDEMHIP_OK) rc = s.candidate_buffers(expected, bracket);
        if (rc) break;
        s.timer.phase("candidate buffers");
        if (!bracket) break;
        rc = s.counting_pass();
        if (rc == XDEMHIP_OK && s.ranks()) {
            rc = s.select_and_results(counts, medians);
            done = rc == XDEMHIP_OK;
        }
    }
    if (rc) { s.cleanup(); return rc; }
    if (WIDE) {   // (the shadow answers through the bracketed route or not at all)
        s.cleanup();
        if (answered) *answered = done;
        return rc;
    }
    if (!done) { rc = pairs_medians_plain<T>(P, s.d_st(), counts, medians); s.timer.phase("plain digit passes"); }
    s.cleanup();
    s.timer.phase("cleanup");
    if (answered) *answered = true;
    return rc;
}

}  // namespace

extern "C" {

int xdemhip_pairs_medians(xdemhip_pairs* P, int64_t* counts, double* medians) {
    XdFetchScope fetch_scope_(P ? P->ctx : nullptr);  // (select_fetch queues deferred result copies)
    if (!P) return XDEMHIP_EINVAL;
    xdemhip_ctx* ctx = P->ctx;
    if (!counts || !medians) return xd_fail(ctx, XDEMHIP_EINVAL, "bad argument");
    XD_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    if (P->val_dtype == XDEMHIP_F64 && P->shadow && P->shadow->val_dtype == XDEMHIP_F32 && !ctx->allreduce) {
        // float64 differences of float32 values (option "vario_diff" = 1 on float32 inputs): the float32 shadow's passes, float64 candidates
        bool answered = false;
        const int rc = pairs_medians_typed<float, true>(P->shadow, counts, medians, &answered);
        if (rc != XDEMHIP_OK || answered) return rc;
    }
    return P->val_dtype == XDEMHIP_F32 ? pairs_medians_typed<float>(P, counts, medians) : pairs_medians_typed<double>(P, counts, medians);
}

int xdemhip_pairs_takes_brackets(xdemhip_pairs* P, int* yes) {
    if (!P || !yes) return XDEMHIP_EINVAL;
    const xdemhip_ctx* ctx = P->ctx;
    // (the conditions of the bracketed route in pairs_medians_typed, plus: a float32 shadow is only read on hook-less contexts)
    *yes = (pairs_route_brackets(ctx->selection_mode, P->nb, P->n_pairs, P->n_wg_big) && !ctx->allreduce) ? 1 : 0;
    return XDEMHIP_OK;
}

int xdemhip_pairs_link_shadow(xdemhip_pairs* P, xdemhip_pairs* shadow) {
    if (!P) return XDEMHIP_EINVAL;
    xdemhip_ctx* ctx = P->ctx;
    if (shadow) {
        if (shadow->ctx != ctx || P->val_dtype != XDEMHIP_F64 || shadow->val_dtype != XDEMHIP_F32 || shadow->nblk != P->nblk || shadow->nb != P->nb ||
            shadow->pdist != P->pdist || shadow->h_a_off != P->h_a_off || shadow->h_b_off != P->h_b_off)
            return xd_fail(ctx, XDEMHIP_EINVAL, "pairs_link_shadow: a float64 set and a float32 set of the same blocks and edges are required");
    }
    P->shadow = shadow;
    return XDEMHIP_OK;
}

}  // extern "C"
