// nuthkaab.hip -- Nuth & Kaab (2011) inner loop on gfx950: everything of one iteration that touches the grids.
//
// Replaces, for raster-raster input (xdem/coreg/affine.py):
//   _nuth_kaab_aux_vars 412-474 (+ zero-slope removal 578-579, valid mask base.py:650-661)   -> nk_aux_kernel (once)
//   _nuth_kaab_iteration_step 477-536:  dh = ref - tba(shifted)                                  -> nk_dh_kernel
//                                       vshift = nanmedian(dh)                                  -> radix select (select.h)
//   _nuth_kaab_bin_fit 358-409:         y = dh / slope_tan, nanmean / nanstd                     -> nk_y_kernel
//                                       binned_statistic(aspect, y, np.nanmedian, 72)            -> bin ids + radix select
// The 72-point curve_fit stays on the host (scipy), exactly as in the reference.
//
// All kernels are streaming passes over row-major grids (coalesced 4-byte lanes, grid-stride), i.e. HBM-bound;
// the per-bin histograms live in LDS (ds_add_u32) and are flushed once per workgroup.  Float arithmetic that the
// reference does in the DEM dtype uses the non-contracting *_rn intrinsics so results are bit-identical to NumPy.
#include <math.h>
#include <string.h>

#include <optional>
#include <vector>

#include "common.h"
#include "select.h"
#include "select_run.h"
#include "nk_geom.h"
#include "nk_aux.h"
#include "nk_layout.h"
#include "nk_policy.h"
#include "rank_select.h"

namespace xd {

// ---- dh at a shifted position + min / max aspect over its finite pixels -------------------------------------------
// (DhStats: nk_aux.h)
static __global__ void nk_stats_init_kernel(DhStats* s) {
    if (threadIdx.x == 0) { s->asp_min = ~(uint64_t)0; s->asp_max = 0; }
}
// ... and, for the one-pass step, the zeroing of its device block and of the EXT survivor counters in the same launch (two memsets less)
static __global__ void nk_step_init_kernel(DhStats* s, uint64_t* fz, int64_t fz_words, unsigned long long* ext_survivors /* [2] */) {
    for (int64_t w = threadIdx.x; w < fz_words; w += blockDim.x) fz[w] = 0;
    if (threadIdx.x == 0) { s->asp_min = ~(uint64_t)0; s->asp_max = 0; ext_survivors[0] = 0; ext_survivors[1] = 0; }
}

template <typename T>
__global__ __launch_bounds__(256) void nk_dh_kernel(const T* __restrict__ ref, const T* __restrict__ tba,
                                                    const uint8_t* __restrict__ valid, const T* __restrict__ aspect,
                                                    NkGeom g, T* __restrict__ dh, DhStats* stats, int64_t row0, int64_t row1) {
    typedef typename KeyT<T>::type K;
    K kmin = ~(K)0, kmax = 0;
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const BiAxis col = bi_axis(j, g.dc, g.W, g.rule);
    if (j < g.W)
    for (int64_t i = row0 + blockIdx.y; i < row1; i += gridDim.y) {
        const int64_t p = (i - g.roff) * g.W + j;
        const BiTap t = bi_combine(g, bi_axis(i, g.dr, g.H, g.rule), col);
        // all loads issued unconditionally (clamped taps) so they overlap; validity is applied afterwards
        const BiVals<T> tv = bi_load<T>(tba, t);
            const T a00 = tv.a00, a01 = tv.a01, a10 = tv.a10, a11 = tv.a11;
        const T rv = ref[p];
        const T av = aspect[p];
        const uint8_t vd = valid[p];  // (every load of the pixel is issued before the first use)
        T val;
        const bool ok = bi_value<T>(g, tba, t, a00, a01, a10, a11, val) & (vd != 0);
        T out = t_sub(rv, val);
        if (ok && t_finite(out)) {
            const K ka = key_of(av);
            kmin = ka < kmin ? ka : kmin;
            kmax = ka > kmax ? ka : kmax;
        } else {
            out = (T)NAN;
        }
        dh[p] = out;
    }
    for (int off = 32; off > 0; off >>= 1) {
        const K a = k_shfl_down(kmin, off), b = k_shfl_down(kmax, off);
        kmin = a < kmin ? a : kmin;
        kmax = b > kmax ? b : kmax;
    }
    if ((threadIdx.x & 63) == 0) {
        if (kmin != ~(K)0) k_atomic_min(&stats->asp_min, (uint64_t)kmin);
        if (kmax != 0) k_atomic_max(&stats->asp_max, (uint64_t)kmax);
    }
}

// ---- min / max aspect without reading the aspect raster every step (round 3) -----------------------------------------------
// The dh pass needs min / max of the aspect over the pixels whose dh is finite (SciPy's bin edges) -- two numbers, each set by
// ONE pixel -- and used to read the 4-byte aspect of every pixel for them.  At plan creation the valid pixels whose aspect lies
// in the lowest / highest ~16 K of the raster are listed (EXT lists); a step evaluates dh at those few pixels only: the minimum
// over the listed pixels with a finite dh IS the minimum over all of them as long as one listed pixel survives (every unlisted
// pixel has a larger aspect); if none survives, or a list came out empty / overfull, the step falls back to the plain route, whose
// kernel reads the aspect (counter [6] of the one-pass step: the plan then stops using its lists).  The same kernel folds the valid mask into a plan-owned copy of
// the reference DEM (NaN where a pixel is not valid): dh = ref - bilinear(tba) is then non-finite by itself and the dh pass
// reads neither the mask nor the aspect: 12 instead of 17 B/pixel.
constexpr int EXT_TARGET = 16384, EXT_CAP = 4 * EXT_TARGET;
template <typename T>
__global__ __launch_bounds__(256) void nk_ext_build_kernel(const T* __restrict__ ref, const uint8_t* __restrict__ valid,
                                                           const T* __restrict__ aspect, int64_t q0, int64_t n, T thr_lo, T thr_hi,
                                                           T* __restrict__ ref_m, int64_t* __restrict__ ext_idx,
                                                           unsigned long long* __restrict__ ext_cnt /* [2] */) {
    const int lane = threadIdx.x & 63;
    for (int64_t base = (int64_t)blockIdx.x * blockDim.x; base < n; base += (int64_t)gridDim.x * blockDim.x) {
        const int64_t p = base + threadIdx.x;
        bool lo = false, hi = false;
        if (p < n) {
            const int64_t q = q0 + p;
            const bool v = valid[q] != 0;
            ref_m[q] = v ? ref[q] : (T)NAN;
            const T a = aspect[q];
            lo = v && a < thr_lo;
            hi = v && a > thr_hi;
        }
#pragma unroll
        for (int w = 0; w < 2; ++w) {
            const bool mine = w ? hi : lo;
            const unsigned long long m = __builtin_amdgcn_ballot_w64(mine);
            if (m) {
                const int leader = __ffsll((long long)m) - 1;
                unsigned long long b = 0;
                if (lane == leader) b = atomicAdd(&ext_cnt[w], (unsigned long long)__popcll(m));
                b = ((unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)(b >> 32), leader) << 32) |
                    (unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)b, leader);
                const unsigned long long pos = b + (unsigned long long)__popcll(m & ((1ull << lane) - 1ull));
                if (mine && pos < (unsigned long long)EXT_CAP) ext_idx[(int64_t)w * EXT_CAP + (int64_t)pos] = q0 + p;
            }
        }
    }
}
// one thread per listed pixel: is its dh finite at this step's shift?  -> min / max aspect keys, survivors per list
template <typename T>
__global__ __launch_bounds__(256) void nk_ext_eval_kernel(const T* __restrict__ ref_m, const T* __restrict__ tba, const T* __restrict__ aspect,
                                                          NkGeom g, const int64_t* __restrict__ ext_idx, const unsigned long long* __restrict__ ext_cnt,
                                                          DhStats* stats, unsigned long long* survivors /* [2] */) {
    typedef typename KeyT<T>::type K;
    const int w = blockIdx.y;
    const unsigned long long cnt = ext_cnt[w] < (unsigned long long)EXT_CAP ? ext_cnt[w] : (unsigned long long)EXT_CAP;
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool ok = false;
    K key = 0;
    if ((unsigned long long)k < cnt) {
        const int64_t q = ext_idx[(int64_t)w * EXT_CAP + k];
        const int64_t li = q / g.W, j = q - li * g.W;
        const BiTap t = bi_locate(g, li + g.roff, j);
        const BiVals<T> tv = bi_load<T>(tba, t);
        T val;
        const bool in = bi_value<T>(g, tba, t, tv.a00, tv.a01, tv.a10, tv.a11, val);
        const T out = t_sub(ref_m[q], val);
        ok = in && t_finite(out);
        key = key_of(aspect[q]);
    }
    const unsigned long long m = __builtin_amdgcn_ballot_w64(ok);
    if (!m) return;
    K best = ok ? key : (w ? (K)0 : ~(K)0);
    for (int off = 32; off > 0; off >>= 1) {
        const K o = k_shfl_down(best, off);
        best = w ? (o > best ? o : best) : (o < best ? o : best);
    }
    if ((threadIdx.x & 63) == 0) {
        if (w) k_atomic_max(&stats->asp_max, (uint64_t)best);
        else k_atomic_min(&stats->asp_min, (uint64_t)best);
        atomicAdd(&survivors[w], (unsigned long long)__popcll(m));
    }
}

// Row-tap table of a chunk of rows (one entry per row, computed once per workgroup into LDS by the one-pass kernel below).
struct NkRowTab { double fr; int k0l; int flags; int rnl; int pad_; };  // upper tap row (buffer-local, clamped), bit 0 = taps inside the raster, bit 1 = d1; rnl: buffer row of the NEAREST pixel (rules 2 / 3), -1 = its neighbourhood leaves the raster

// ---- rules 2 / 3 ("dilate3x3" / "dilate_cross") without a neighbourhood read per pixel (round 5) -------------------------------
// Under these rules a sample is valid iff its four taps are finite AND the 3 x 3 / cross neighbourhood of the pixel NEAREST to the
// tap position holds no non-finite value and stays inside the raster (bi_value above).  The second condition depends on tba alone:
// it is evaluated ONCE per plan into a bit per pixel ("bad" = neighbourhood not clean; border pixels, the columns beyond W in a
// row's last word and one all-ones pad word on either side of every row are bad too), and the streaming kernels then test the bit
// of the nearest pixel -- the same floor(pos + 0.5) per row and per lane as bi_combine -- next to their rule-0 arithmetic: one 8-byte
// word per lane and row, two distinct words per wave.  Results are those of the generic kernel bit for bit (GPU tests per rule).
template <typename T>
__global__ __launch_bounds__(256) void nk_badbits_kernel(const T* __restrict__ tba /* the plan's buffer: rows roff .. roff + nbuf of the raster */,
                                                         int64_t H, int64_t W, int64_t roff, int64_t nbuf, int rule, int64_t wpr,
                                                         uint64_t* __restrict__ out /* [nbuf][wpr] */) {
    const int lane = threadIdx.x & 63;
    const int64_t word = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);   // data word of the row (pad words: below)
    const int64_t nwords = wpr - 2;
    for (int64_t r = blockIdx.y; r < nbuf; r += gridDim.y) {
        if (word < nwords) {
            const int64_t c = word * 64 + lane;
            // bad: on the raster's border -- or, in a row block, in the first / last row of the buffer where that is not the raster's:
            // the halo rule of the step (HaloTooSmall) keeps every nearest pixel off those rows, so the bit is never consulted
            bool bad = !(roff + r >= 1 && c >= 1 && roff + r + 1 < H && c + 1 < W) || r < 1 || r + 1 >= nbuf;
            if (!bad) {
                for (int dy = -1; dy <= 1; ++dy)
                    for (int dx = -1; dx <= 1; ++dx)
                        if (rule == 2 || dy == 0 || dx == 0) bad = bad || !t_finite(tba[(r + dy) * W + (c + dx)]);
            }
            const unsigned long long m = __builtin_amdgcn_ballot_w64(bad);
            if (lane == 0) out[r * wpr + 1 + word] = (uint64_t)m;
        }
        if (blockIdx.x == 0 && threadIdx.x < 2) out[r * wpr + (threadIdx.x ? wpr - 1 : 0)] = ~(uint64_t)0;
    }
}
// nearest pixel of a row / column position as bi_combine computes it
__device__ __forceinline__ int64_t nk_nearest(double pos) { return (int64_t)floor(pos + 0.5); }
// ---- full-grid translation resample (Coreg.apply for a pure shift) --------------------------------
// out(r, c) = bilinear(src)(r + dr, c + dc) + dz with the same tap convention / NaN rule as the Nuth-Kaab step.
template <typename T>
__global__ __launch_bounds__(256) void shift_bilinear_kernel(const T* __restrict__ src, NkGeom g, T dz, T* __restrict__ out) {
    const int64_t n = g.H * g.W;
    const double invW = 1.0 / (double)g.W;
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (int64_t)gridDim.x * blockDim.x) {
        int64_t i, j;
        row_col(p, g.W, invW, i, j);
        const BiTap t = bi_locate(g, i, j);
        T val;
        const BiVals<T> tv = bi_load<T>(src, t);
        const bool ok = bi_value<T>(g, src, t, tv.a00, tv.a01, tv.a10, tv.a11, val);
        out[p] = ok ? t_add(val, dz) : (T)NAN;
    }
}

// (SciPy's rule for samples on the last edge, on_last_edge, and the digitize step aspect_bin: nk_aux.h)
// ---- y = (dh - vshift) / slope_tan, aspect bin id, sums for nanmean / nanstd --------------------------------
template <typename T>
__global__ __launch_bounds__(256) void nk_y_kernel(const T* __restrict__ dh, const T* __restrict__ slope_tan,
                                                   const T* __restrict__ aspect, int64_t n, T vshift,
                                                   const T* __restrict__ edges, int nb, T* __restrict__ y,
                                                   uint16_t* __restrict__ bins, double* sums /* [sum, sumsq] */,
                                                   int last_decimal = NK_AUTO_EDGES,
                                                   double* part = nullptr /* [workgroups][2]: the sums leave per workgroup, for nk_y_sums_kernel */) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ double wave_part[2][4];
    T* e = reinterpret_cast<T*>(smem);
    for (int k = threadIdx.x; k <= nb; k += blockDim.x) e[k] = edges[k];
    __syncthreads();
    const double inv_width = (double)nb / ((double)e[nb] - (double)e[0]);
    double s1 = 0.0, s2 = 0.0;
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (int64_t)gridDim.x * blockDim.x) {
        const T d = dh[p];
        const T st = slope_tan[p];
        const T x = aspect[p];
        T yv = (T)NAN;
        uint16_t b = 0xFFFF;
        if (d == d) {  // dh is NaN wherever the pixel is unusable
            yv = t_div(t_sub(d, vshift), st);
            b = aspect_bin<T>(x, e, nb, inv_width, last_decimal);
            s1 += (double)yv;
            s2 += (double)yv * (double)yv;
        }
        y[p] = yv;
        bins[p] = b;
    }
    for (int off = 32; off > 0; off >>= 1) { s1 += __shfl_down(s1, off); s2 += __shfl_down(s2, off); }
    if (!part) {
        if ((threadIdx.x & 63) == 0) { atomicAdd(&sums[0], s1); atomicAdd(&sums[1], s2); }
        return;
    }
    // a fixed order instead of atomics, whose order of arrival changes the last bits from launch to launch: the four waves in order
    // here, the workgroups in order in nk_y_sums_kernel
    if ((threadIdx.x & 63) == 0) { wave_part[0][threadIdx.x >> 6] = s1; wave_part[1][threadIdx.x >> 6] = s2; }
    __syncthreads();
    if (threadIdx.x < 2) {
        const double* w = wave_part[threadIdx.x];
        part[2 * (size_t)blockIdx.x + threadIdx.x] = ((w[0] + w[1]) + w[2]) + w[3];
    }
}

// sums[t] = the workgroups' partials of nk_y_kernel added in a fixed order: lane l takes the partials l, l + 256, ... in order, then a
// halving tree over the 256 lanes.  One workgroup.
__global__ __launch_bounds__(256) void nk_y_sums_kernel(const double* __restrict__ part, int n_wg, double* __restrict__ sums) {
    __shared__ double red[256];
    for (int t = 0; t < 2; ++t) {
        double s = 0.0;
        for (int b = threadIdx.x; b < n_wg; b += 256) s += part[2 * (size_t)b + t];
        red[threadIdx.x] = s;
        __syncthreads();
        for (int half = 128; half > 0; half >>= 1) {
            if ((int)threadIdx.x < half) red[threadIdx.x] += red[threadIdx.x + half];
            __syncthreads();
        }
        if (threadIdx.x == 0) sums[t] = red[0];
        __syncthreads();
    }
}

// The same y / bin id computed on the fly for the bracketed selection (select_run.h): its sample and counting passes read
// dh, slope_tan and aspect directly, so the y and bin-id arrays are neither written nor re-read (nk_y_kernel + plain
// selection remain the fallback).  The counting pass, which sees every element once, also accumulates the two sums.
// Aspect-bin cache: the bin of a pixel depends only on its aspect and on the edges, and the edges (SciPy's linspace between the
// min and max aspect of the valid pixels, or the caller's explicit edges) hardly ever change between the steps of a fit.  The
// first pass under a given set of edges stores every pixel's bin id (uint16, 0xFFFF = outside) and later passes read 2 bytes
// instead of digitizing a 4-byte aspect again; a one-thread kernel compares the edges with the record of what the cache holds.
// The aspect-bin cache holds ONE BYTE per pixel (round 6; two until then): every route that reads it takes at most MAX_BINS_PER_SWEEP
// = 128 bins, 0xFF = "no bin" -- the one-pass step touches 13 instead of 14 bytes per pixel, the bin pass of the plain route 9
// instead of 10.  Candidates and samples keep 16-bit bin ids (the selection code is shared with nd_binning).
typedef uint8_t nk_bin_t;
constexpr nk_bin_t NK_NOBIN = 0xFF;
constexpr int NK_BINCACHE_MAX_BINS = 254;
__host__ __device__ inline uint16_t nk_bin16(nk_bin_t b) { return b == NK_NOBIN ? (uint16_t)0xFFFF : (uint16_t)b; }
__host__ __device__ inline nk_bin_t nk_bin8(uint16_t b) { return b == (uint16_t)0xFFFF ? NK_NOBIN : (nk_bin_t)b; }
struct BinCacheRec { double e0, eN; int nb; int fresh; };
template <typename T> __global__ void nk_bin_cache_check_kernel(const T* edges, int nb, BinCacheRec* rec, int force) {
    if (threadIdx.x == 0) {
        const double e0 = (double)edges[0], eN = (double)edges[nb];
        rec->fresh = (!force && rec->nb == nb && rec->e0 == e0 && rec->eN == eN) ? 1 : 0;
    }
}
// (launched once a pass over ALL own pixels has been queued under these edges; nb = 0 invalidates)
template <typename T> __global__ void nk_bin_cache_commit_kernel(const T* edges, int nb, BinCacheRec* rec) {
    if (threadIdx.x == 0) {
        rec->e0 = nb > 0 ? (double)edges[0] : 0.0;
        rec->eN = nb > 0 ? (double)edges[nb] : 0.0;
        rec->nb = nb;
    }
}

template <typename T> struct NkYSource {
    const T* dh;
    const T* slope_tan;
    const T* aspect;
    const T* vshift_p;  // device scalar (uploaded by the host on the plain route)
    const T* edges;  // [nb + 1], device
    double* sums;    // [sum, sumsq], device
    T* e;            // LDS copy of the edges (setup)
    double inv_width;
    T vshift;
    int last_decimal;  // rounding precision of SciPy's rightmost-edge rule (NK_AUTO_EDGES for the automatic edges)
    nk_bin_t* bcache = nullptr;          // per-pixel bin ids (null: no cache)
    const BinCacheRec* rec = nullptr;
    int fresh = -1;                      // 1: read the cache, 0: digitize and fill it, -1: digitize only
    struct Raw { T d, st, x; int64_t p; uint16_t b; };
    struct Acc { double s1 = 0.0, s2 = 0.0; };
    static size_t lds_bytes(int nb) { return sizeof(T) * (size_t)(nb + 1) + 8; }
    __device__ __forceinline__ void setup(unsigned char* lds, int nb) {
        e = reinterpret_cast<T*>((reinterpret_cast<uintptr_t>(lds) + 7) & ~(uintptr_t)7);
        for (int k = threadIdx.x; k <= nb; k += blockDim.x) e[k] = edges[k];
        inv_width = (double)nb / ((double)edges[nb] - (double)edges[0]);
        vshift = *vshift_p;
        fresh = bcache ? __builtin_amdgcn_readfirstlane(rec->fresh) : -1;
    }
    __device__ __forceinline__ void fetch(int64_t p, Raw& r) const {
        r.d = dh[p]; r.st = slope_tan[p]; r.p = p;
        if (fresh == 1) { r.b = nk_bin16(bcache[p]); r.x = (T)0; }
        else { r.x = aspect[p]; r.b = 0xFFFF; }
    }
    __device__ __forceinline__ void blank(Raw& r) const { r.d = (T)NAN; r.st = (T)1; r.x = (T)0; r.p = -1; r.b = 0xFFFF; }
    __device__ __forceinline__ uint16_t digitize(T x, int nb) const {
        int idx = (int)(((double)x - (double)e[0]) * inv_width);  // (same digitize as nk_y_kernel)
        idx = idx < 0 ? 0 : (idx > nb ? nb : idx);
        while (idx > 0 && !(e[idx] <= x)) --idx;
        while (idx < nb && e[idx + 1] <= x) ++idx;
        if (!(e[0] <= x)) idx = -1;
        if (idx == nb && on_last_edge<T>(x, e[nb], last_decimal)) idx = nb - 1;
        return (idx >= 0 && idx < nb) ? (uint16_t)idx : (uint16_t)0xFFFF;
    }
    template <bool ACC> __device__ __forceinline__ bool eval(const Raw& r, int nb, T& v, uint16_t& b, Acc& acc) const {
        v = (T)NAN;
        b = 0xFFFF;
        uint16_t bin = r.b;
        if (fresh != 1) {
            if (fresh == 0) {  // filling pass: every pixel, whatever its dh is this step
                if (r.p >= 0) { bin = digitize(r.x, nb); bcache[r.p] = nk_bin8(bin); }
            } else if (r.d == r.d) {
                bin = digitize(r.x, nb);
            }
        }
        if (!(r.d == r.d)) return false;
        const T yv = t_div(t_sub(r.d, vshift), r.st);
        if (ACC) { acc.s1 += (double)yv; acc.s2 += (double)yv * (double)yv; }
        v = yv;
        if (bin == 0xFFFF) return false;
        b = bin;
        return yv == yv;
    }
    __device__ __forceinline__ void finish(Acc& acc) const {
        double s1 = acc.s1, s2 = acc.s2;
        for (int off = 32; off > 0; off >>= 1) { s1 += __shfl_down(s1, off); s2 += __shfl_down(s2, off); }
        if ((threadIdx.x & 63) == 0) { atomicAdd(&sums[0], s1); atomicAdd(&sums[1], s2); }
    }
    // the counting pass has a dedicated kernel for cached bins (nk_bins_lean_kernel below): the generic one steps aside then
    static constexpr bool HAS_LEAN = true;
    __device__ __forceinline__ bool skip_counting_pass() const { return fresh == 1; }
    int launch_lean(xdemhip_ctx* ctx, int64_t n, int nb, const typename KeyT<T>::type* d_klo, const typename KeyT<T>::type* d_khi,
                    uint64_t* d_cnt, T* c_vals, uint16_t* c_bins, unsigned long long* d_flags, int64_t c_cap) const;
};

// ---- lean form of the per-bin counting pass (select_run.h: bracket_pass_kernel over NkYSource) for steps whose aspect bins are
// cached: 10 bytes per pixel (dh, slope tangent, bin id), one LDS read for the bin's bracket, one LDS atomic for its class,
// candidates compacted through per-wave staging (no workgroup barrier in the loop).  The generic kernel -- measured VALU-bound at
// about 145 vector instructions per element -- stays in charge of the steps that (re)fill the cache; both are queued, each
// leaves at once when the device-side `fresh` flag says it is the other one's turn.
constexpr int NKB_TILE = 8;
template <typename T>
__global__ __launch_bounds__(HIST_THREADS) void nk_bins_lean_kernel(const T* __restrict__ dh, const T* __restrict__ slope_tan,
                                                                    const nk_bin_t* __restrict__ bcache, const BinCacheRec* rec,
                                                                    const T* vshift_p, int64_t n, int nb, int copies,
                                                                    const typename KeyT<T>::type* __restrict__ klo,
                                                                    const typename KeyT<T>::type* __restrict__ khi,
                                                                    uint64_t* counters /* [3][nb] */, T* out_v, uint16_t* out_b,
                                                                    unsigned long long* ctr, int64_t cap, double* sums) {
    typedef typename KeyT<T>::type K;
    if (rec->fresh != 1) return;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    // workgroup staging exactly as in bracket_pass_kernel (one global atomic per burst of thousands of candidates)
    BlockStage<T> st;
    st.v = reinterpret_cast<T*>(smem);
    st.b = reinterpret_cast<uint16_t*>(st.v + SEL_STAGE_CAP);
    st.base = reinterpret_cast<unsigned long long*>(st.b + SEL_STAGE_CAP);
    st.held = reinterpret_cast<int*>(st.base + 1);
    K* lohi = reinterpret_cast<K*>(st.base + 2);               // [nb][2]
    uint32_t* c = reinterpret_cast<uint32_t*>(lohi + 2 * nb);  // [copies][cs]: 3 counters per bin
    const int cs = (3 * nb) | 1;  // odd copy stride: the copies of one counter fall into different LDS banks
    for (int k = threadIdx.x; k < nb; k += blockDim.x) { lohi[2 * k] = klo[k]; lohi[2 * k + 1] = khi[k]; }
    for (int k = threadIdx.x; k < cs * copies; k += blockDim.x) c[k] = 0;
    if (threadIdx.x == 0) *st.held = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    uint32_t* cc = c + (threadIdx.x % copies) * cs;
    const T vshift = *vshift_p;
    double s1 = 0.0, s2 = 0.0;
    int it = 0;
    const int64_t step = (int64_t)blockDim.x * NKB_TILE;
    for (int64_t base = (int64_t)blockIdx.x * step; base < n; base += (int64_t)gridDim.x * step) {
        T d[NKB_TILE], sl[NKB_TILE];
        uint16_t b[NKB_TILE];
        if (base + step <= n) {  // (uniform) whole tile inside: no per-element bounds logic
#pragma unroll
            for (int q = 0; q < NKB_TILE; ++q) {
                const int64_t p = base + (int64_t)q * blockDim.x + threadIdx.x;
                d[q] = __builtin_nontemporal_load(dh + p); sl[q] = __builtin_nontemporal_load(slope_tan + p);
                b[q] = nk_bin16(__builtin_nontemporal_load(bcache + p));
            }
        } else {
#pragma unroll
            for (int q = 0; q < NKB_TILE; ++q) {
                const int64_t p = base + (int64_t)q * blockDim.x + threadIdx.x;
                const bool in = p < n;
                const int64_t pc = in ? p : n - 1;
                d[q] = dh[pc]; sl[q] = slope_tan[pc]; b[q] = nk_bin16(bcache[pc]);
                if (!in) d[q] = (T)NAN;
            }
        }
#pragma unroll
        for (int q = 0; q < NKB_TILE; ++q) {
            const T yv = t_div(t_sub(d[q], vshift), sl[q]);
            const bool has = d[q] == d[q];
            if (has) { s1 += (double)yv; s2 += (double)yv * (double)yv; }
            const bool ok = has & (b[q] != 0xFFFF) & (yv == yv);
            bool cand = false;
            if (ok) {
                const K key = key_of(yv);
                const K l = lohi[2 * b[q]], h = lohi[2 * b[q] + 1];
                cand = (key >= l) & (key <= h);
                const int cls = key < l ? 1 : (cand ? 2 : 0);
                atomicAdd(&cc[__umul24((unsigned)cls, (unsigned)nb) + b[q]], 1u);
            }
            st.append_bounded(cand, yv, b[q], &ctr[2]);
        }
        // (same exposure to candidate bursts as the generic kernel: 16384 elements between two looks at the staging buffer)
        if ((++it % (SEL_FLUSH_EVERY * SEL_TILE / NKB_TILE)) == 0) st.sync_and_flush_at(0, out_v, out_b, &ctr[1], cap, &ctr[2]);
    }
    st.sync_and_flush_at(0, out_v, out_b, &ctr[1], cap, &ctr[2]);
    for (int off = 32; off > 0; off >>= 1) { s1 += __shfl_down(s1, off); s2 += __shfl_down(s2, off); }
    if (lane == 0) { atomicAdd(&sums[0], s1); atomicAdd(&sums[1], s2); }
    for (int k = threadIdx.x; k < nb; k += blockDim.x) {
        unsigned long long above = 0, below = 0, inside = 0;
        for (int q = 0; q < copies; ++q) {
            above += c[q * cs + k]; below += c[q * cs + nb + k]; inside += c[q * cs + 2 * nb + k];
        }
        if (above + below + inside) atomicAdd(reinterpret_cast<unsigned long long*>(&counters[k]), above + below + inside);
        if (below) atomicAdd(reinterpret_cast<unsigned long long*>(&counters[nb + k]), below);
        if (inside) atomicAdd(reinterpret_cast<unsigned long long*>(&counters[2 * nb + k]), inside);
    }
}

template <typename T>
int NkYSource<T>::launch_lean(xdemhip_ctx* ctx, int64_t n, int nb, const typename KeyT<T>::type* d_klo, const typename KeyT<T>::type* d_khi,
                              uint64_t* d_cnt, T* c_vals, uint16_t* c_bins, unsigned long long* d_flags, int64_t c_cap) const {
    typedef typename KeyT<T>::type K;
    if (!bcache || n <= 0) return XDEMHIP_OK;
    int copies = (28 * 1024) / (nb * 12);
    copies = copies < 1 ? 1 : (copies > 32 ? 32 : copies);
    const size_t lds = (size_t)SEL_STAGE_CAP * (sizeof(T) + 2) + 16 + (size_t)nb * 2 * sizeof(K) + (size_t)((3 * nb) | 1) * 4 * (size_t)copies;
    int rc = set_big_lds(ctx, nk_bins_lean_kernel<T>, lds);
    if (rc) return rc;
    // (grid-stride: two 1024-thread workgroups per CU are resident -- LDS -- and that is the grid)
    hipLaunchKernelGGL((nk_bins_lean_kernel<T>), dim3(grid_for(ctx, n, HIST_THREADS * NKB_TILE, 2)), dim3(HIST_THREADS), lds, ctx->stream, dh,
                       slope_tan, bcache, rec, vshift_p, n, nb, copies, d_klo, d_khi, d_cnt, c_vals, c_bins, d_flags, c_cap, sums);
    XD_HIP_CHECK(ctx, hipGetLastError());
    return XDEMHIP_OK;
}


}  // namespace xd

#include "nk_onepass.h"


// ================================================================================================================
using namespace xd;

struct xdemhip_nk_plan {
    xdemhip_ctx* ctx = nullptr;
    int dtype = XDEMHIP_F32;
    int64_t H = 0, W = 0;                 // raster shape (global)
    int64_t roff = 0, nbuf = 0;           // the buffers hold raster rows [roff, roff + nbuf)
    int64_t row0 = 0, row1 = 0;           // this rank's own rows [row0, row1) (whole raster unless sharded)
    XdOwned mem;                          // every device buffer of the plan but the caller's own device arrays
    void *ref = nullptr, *tba = nullptr;  // device: the caller's arrays, or owned copies of its host arrays
    uint8_t* inlier = nullptr;            // ... likewise, kept for re-partitioning
    uint8_t* sub_inlier = nullptr;        // xdemhip_nk_subsample: the inlier mask in force after it (owned; `inlier` then points here)
    void *slope_tan = nullptr, *aspect = nullptr, *dh = nullptr, *y = nullptr;
    uint8_t* valid = nullptr;
    uint16_t* bins = nullptr;
    nk_bin_t* bcache = nullptr;   // aspect-bin cache (NkYSource), one BYTE per buffer pixel
    bool bcache_force = true;     // the cache does not hold the bins of the current own rows / edges: refill at the next step
    void* ref_m = nullptr;        // reference DEM with NaN where a pixel is not valid (EXT route of the dh pass)
    int64_t* ext_idx = nullptr;   // [2][EXT_CAP] pixels with the lowest / highest aspects
    unsigned long long* ext_cnt = nullptr;  // [0..1] list lengths, [2..3] survivors of the current step
    bool ext_ok = false;
    uint64_t* fz = nullptr;       // device block of the one-pass step (nk_layout.h: NkFzLayout): counters, bracket keys, v^, sums
    void* cd_vals = nullptr;      // ... candidates of the median of dh
    int64_t cd_cap = 0;
    void* c_st = nullptr;         // ... slope tangents of the bin candidates (next to ws.c_vals / ws.c_bins)
    double* wg_sums = nullptr;    // ... the pass's five float64 sums per workgroup (added up in a fixed order: nk_sums_reduce)
    size_t wg_sums_cap = 0;
    unsigned char* fz_pack = nullptr;   // ... the step's small results, gathered for one device-to-host copy
    size_t fz_pack_bytes = 0;
    std::vector<unsigned char> fz_host;
    int64_t n_onepass = 0, n_plain = 0;   // steps answered by each route (xdemhip_nk_route_counts)
    // one-pass route, the two host policies (nk_policy.h): how narrow the sample brackets of the NEXT step may be, and the record
    // of the previous step from which THIS step's brackets are predicted instead of sampled
    NkNarrowing narrowing;
    NkPrediction pred;
    // one-pass step on PARTITIONED plans (reduction hook + xdemhip_set_rank): the two exchange buffers, this rank's own classes and the
    // counters rewritten for the gathered bucket values (nk_mr_* kernels); the ranks' agreement on the route, renewed when what it rests
    // on changes
    uint64_t *mr_a = nullptr, *mr_b = nullptr, *mr_small = nullptr;
    size_t mr_a_words = 0, mr_b_words = 0;
    int64_t mr_key[8] = {-1, -1, -1, -1, -1, -1, -1, -1};
    bool mr_can = false;
    int64_t mr_nglob = 0;
    void* scratch = nullptr;  // edges, stats, sums, selection states, successor keys, histograms
    size_t scratch_bytes = 0;
    int max_bins = 0;
    long long n_valid0 = 0;
    xd::SelWorkspace ws;  // bracketed selection (select_run.h): sample + candidate buffers
    uint64_t* badbits = nullptr;   // rules 2 / 3: one bit per buffer pixel, "the neighbourhood of this pixel of tba is not clean" (nk_badbits_kernel)
    int64_t bad_wpr = 0;           // ... 64-bit words per row, one all-ones pad word on either side
    int bin_stat = XDEMHIP_BINSTAT_MEDIAN;
    int nan_rule = 0;
    int custom_decimal = 0;            // ... and the decimal of SciPy's rightmost-edge rule for them
    std::vector<double> custom_edges;  // explicit bin edges (xdemhip_nk_set_bin_edges); empty: SciPy's linspace(min, max, n + 1)
};

namespace {

// scratch (first 16 KiB): bin edges [0, 8208) | device-side step results at OFF_INFO
constexpr size_t OFF_INFO = 12288;  // T vshift (8 B slot) | uint64 n_valid | uint64 flags | double vshift

// column tiles of 256 x enough row-strided workgroups to fill the chip (~16 workgroups per CU)
dim3 grid2d(const xdemhip_ctx* ctx, int64_t W, int64_t rows) {
    const int64_t gx = (W + 255) / 256;
    int64_t gy = ((int64_t)ctx->num_cu * 16 + gx - 1) / gx;
    gy = gy < 1 ? 1 : (gy > rows ? (rows > 0 ? rows : 1) : gy);
    return dim3((unsigned)gx, (unsigned)gy);
}

template <typename T> void make_edges(double smin, double smax, int nb, std::vector<T>& e) {
    e.resize(nb + 1);
    make_edges_into<T>(smin, smax, nb, e.data());
}

NkGeom geom_of(const xdemhip_nk_plan* P, double dr, double dc) {
    NkGeom g;
    g.H = P->H; g.W = P->W; g.roff = P->roff; g.dr = dr; g.dc = dc; g.rule = P->nan_rule;
    return g;
}

// aux variables + valid mask for this rank's rows; global valid count through the hook
template <typename T> int nk_aux_typed(xdemhip_nk_plan* P) {
    xdemhip_ctx* ctx = P->ctx;
    const int64_t rows = P->row1 - P->row0;
    unsigned long long* d_cnt = reinterpret_cast<unsigned long long*>(static_cast<unsigned char*>(P->scratch) + OFF_STATS);
    XD_HIP_CHECK(ctx, hipMemsetAsync(d_cnt, 0, 8, ctx->stream));
    if (rows > 0) {
        hipLaunchKernelGGL((nk_aux_kernel<T>), grid2d(ctx, P->W, rows), dim3(256), 0, ctx->stream,
                           static_cast<const T*>(P->ref), static_cast<const T*>(P->tba), P->inlier, geom_of(P, 0.0, 0.0),
                           static_cast<T*>(P->slope_tan), static_cast<T*>(P->aspect), P->valid, d_cnt, P->row0, P->row1);
        XD_HIP_CHECK(ctx, hipGetLastError());
    }
    int rc = xd_allreduce_device(ctx, d_cnt, 1, XDEMHIP_RED_SUM_U64);
    if (rc) return rc;
    unsigned long long c = 0;
    { const int rc_ = xd_d2h(ctx, &c, d_cnt, 8); if (rc_) return rc_; }
    { const int rc_ = xd_sync(ctx); if (rc_) return rc_; }
    P->n_valid0 = (long long)c;
    // EXT route (see nk_ext_build_kernel): single-GPU plans only -- with a reduction hook every rank would have to agree on
    // the route at every step; the sharded plans keep reading mask and aspect
    // Partitioned plans (round 5, second half): every rank lists ITS extreme-aspect pixels against the same thresholds (the valid
    // count is the global one), min / max aspect of a step are the min / max over the ranks' survivors, and the lists are usable if
    // no rank's overflowed and each kind has a pixel on SOME rank -- agreed once, here.
    P->ext_ok = false;
    const bool mr = ctx->allreduce != nullptr;
    if (mr && !(ctx->nk_fused_dist != 0 && ctx->world >= 1 && ctx->world <= MR_WORLD_MAX)) return XDEMHIP_OK;
    if (P->n_valid0 >= 8 * (long long)EXT_TARGET) {   // (the same decision on every rank)
        const bool local_ok = P->ref_m != nullptr && rows > 0;
        unsigned long long ec[2] = {0, 0};
        if (local_ok) {
            const double frac = (double)EXT_TARGET / (double)P->n_valid0;
            const T thr_lo = (T)(6.283185307179586 * frac), thr_hi = (T)(6.283185307179586 * (1.0 - frac));
            const int64_t q0 = (P->row0 - P->roff) * P->W, nown = rows * P->W;
            XD_HIP_CHECK(ctx, hipMemsetAsync(P->ext_cnt, 0, 32, ctx->stream));
            hipLaunchKernelGGL((nk_ext_build_kernel<T>), dim3(grid_for(ctx, nown, 256, 16)), dim3(256), 0, ctx->stream, static_cast<const T*>(P->ref),
                               P->valid, static_cast<const T*>(P->aspect), q0, nown, thr_lo, thr_hi, static_cast<T*>(P->ref_m), P->ext_idx, P->ext_cnt);
            XD_HIP_CHECK(ctx, hipGetLastError());
            { const int rc_ = xd_d2h(ctx, ec, P->ext_cnt, 16); if (rc_) return rc_; }
            { const int rc_ = xd_sync(ctx); if (rc_) return rc_; }
        }
        // (aspects far from uniform -- a tilted plane, a raster of one slope direction -- leave a list empty or overfull)
        const bool over = ec[0] > (unsigned long long)EXT_CAP || ec[1] > (unsigned long long)EXT_CAP;
        if (mr) {
            uint64_t v[3] = {ec[0], ec[1], (uint64_t)((!local_ok || over) ? 1 : 0)};
            const int rc_ = xd_allreduce_host(ctx, v, 3, XDEMHIP_RED_SUM_U64);
            if (rc_) return rc_;
            P->ext_ok = v[2] == 0 && v[0] >= 1 && v[1] >= 1;
        } else {
            P->ext_ok = local_ok && !over && ec[0] >= 1 && ec[1] >= 1;
        }
    }
    return XDEMHIP_OK;
}

// Least-squares sums of the un-binned fit (NuthKaab(bin_before_fit=False): curve_fit of a cos(b - x) + c on every point,
// xdem/coreg/base.py:975-989).  The model is linear in (A, B, c) = (a cos b, a sin b, c): y = A cos x + B sin x + c, so the
// optimum curve_fit converges to follows from nine float64 sums; x = aspect and y = (dh - vshift) / slope_tan are widened
// to float64 first, as curve_fit does with its inputs.  sums: n, Sc, Ss, Scc, Sss, Scs, Sy, Syc, Sys, Syy.
template <typename T>
__global__ __launch_bounds__(256) void nk_fit_sums_kernel(const T* __restrict__ dh, const T* __restrict__ slope_tan,
                                                          const T* __restrict__ aspect, int64_t n, const T* __restrict__ vshift_p,
                                                          double* sums /* [10] */) {
    const T vshift = *vshift_p;
    double a[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (int64_t)gridDim.x * blockDim.x) {
        const T d = dh[p];
        const T st = slope_tan[p];
        const T x = aspect[p];
        if (d == d) {
            const double y = (double)t_div(t_sub(d, vshift), st);
            const double c = cos((double)x), sn = sin((double)x);
            a[0] += 1.0; a[1] += c; a[2] += sn; a[3] += c * c; a[4] += sn * sn; a[5] += c * sn;
            a[6] += y; a[7] += y * c; a[8] += y * sn; a[9] += y * y;
        }
    }
    __shared__ double blk[10];
    if (threadIdx.x < 10) blk[threadIdx.x] = 0.0;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 10; ++k) {
        double v = a[k];
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
        if ((threadIdx.x & 63) == 0) atomicAdd(&blk[k], v);
    }
    __syncthreads();
    if (threadIdx.x < 10) atomicAdd(&sums[threadIdx.x], blk[threadIdx.x]);
}

// Stages 1 + 2 of a step on the PLAIN route (the fall-back of the one-pass step, and the route of the mean statistic, of the un-binned
// fit and of small rasters): dh at the shifted position (written), min / max aspect over its finite pixels, the exact nanmedian of
// dh.  On return the device holds dh, the vertical shift (OFF_INFO), the bin edges (scratch start; the plan's custom edges if set)
// and, at OFF_INFO + 8, the valid count.
template <typename T>
int nk_stage_a(xdemhip_nk_plan* P, const NkGeom& g, int64_t q0, int64_t n, int nb) {
    typedef typename KeyT<T>::type K;
    xdemhip_ctx* ctx = P->ctx;
    unsigned char* base = static_cast<unsigned char*>(P->scratch);
    DhStats* d_stats = reinterpret_cast<DhStats*>(base + OFF_STATS);
    T* d_edges = reinterpret_cast<T*>(base);
    DhStats hs0;
    hipLaunchKernelGGL(nk_stats_init_kernel, dim3(1), dim3(64), 0, ctx->stream, d_stats);
    XD_HIP_CHECK(ctx, hipGetLastError());
    int rc = XDEMHIP_OK;
    {
        if (n > 0) {
            hipLaunchKernelGGL((nk_dh_kernel<T>), grid2d(ctx, P->W, P->row1 - P->row0), dim3(256), 0, ctx->stream,
                               static_cast<const T*>(P->ref), static_cast<const T*>(P->tba), P->valid, static_cast<const T*>(P->aspect),
                               g, static_cast<T*>(P->dh), d_stats, P->row0, P->row1);
            XD_HIP_CHECK(ctx, hipGetLastError());
        }
        rc = xd_allreduce_device(ctx, &d_stats->asp_min, 1, XDEMHIP_RED_MIN_U64);
        if (rc) return rc;
        rc = xd_allreduce_device(ctx, &d_stats->asp_max, 1, XDEMHIP_RED_MAX_U64);
        if (rc) return rc;
        std::vector<SelResult<K>> g0;
        rc = run_select<T>(ctx, static_cast<const T*>(P->dh) + q0, nullptr, n, 1, base, g0, &P->ws);
        if (rc) return rc;
        { const int rc_ = xd_d2h(ctx, &hs0, d_stats, sizeof hs0); if (rc_) return rc_; }
        { const int rc_ = xd_sync(ctx); if (rc_) return rc_; }
        unsigned char info[32] = {0};
        const T vs_t = (T)median_from<T>(g0[0]);
        const uint64_t total = g0[0].st.count, flags = 0;
        const double vs = g0[0].st.count ? (double)vs_t : (double)NAN;
        memcpy(info, &vs_t, sizeof(T));
        memcpy(info + 8, &total, 8);
        memcpy(info + 16, &flags, 8);
        memcpy(info + 24, &vs, 8);
        std::vector<T> edges;
        make_edges<T>((double)val_of((K)hs0.asp_min), (double)val_of((K)hs0.asp_max), nb, edges);
        XD_HIP_CHECK(ctx, hipMemcpyAsync(base + OFF_INFO, info, 32, hipMemcpyHostToDevice, ctx->stream));
        XD_HIP_CHECK(ctx, hipMemcpyAsync(d_edges, edges.data(), sizeof(T) * (nb + 1), hipMemcpyHostToDevice, ctx->stream));
        { const int rc_ = xd_sync(ctx); if (rc_) return rc_; }  // (info / edges are stack / local buffers)
    }
    if (!P->custom_edges.empty()) {  // explicit bin edges (NuthKaab(bin_sizes=<edges>)): SciPy casts them to the sample dtype
        std::vector<T> e(P->custom_edges.size());
        for (size_t k = 0; k < e.size(); ++k) e[k] = (T)P->custom_edges[k];
        XD_HIP_CHECK(ctx, hipMemcpyAsync(d_edges, e.data(), sizeof(T) * e.size(), hipMemcpyHostToDevice, ctx->stream));
        { const int rc_ = xd_sync(ctx); if (rc_) return rc_; }
    }
    return XDEMHIP_OK;
}


// exchange buffers of the one-pass step on partitioned plans, sized for `nb` bins and `world` ranks (see the nk_mr_* kernels)
int nk_mr_alloc(xdemhip_nk_plan* P, int nb, int world, size_t es) {
    auto mx = [](size_t a, size_t b) { return a > b ? a : b; };
    const size_t wa = mx(mx(4, 3 + 3 * (size_t)nb + 5 * (size_t)world + (size_t)world * (DSEL_BUCKETS / 2)), 2 + 2 * (size_t)nb + (size_t)world * nb * (SEL_RADIX / 2));
    const size_t wb = mx((size_t)world * DSEL_HDR_WORDS + (size_t)DSEL_CAP * es / 8, (size_t)nb * MR_GSEG * es / 8);
    const char* who = "exchange buffers of the one-pass step";
    if (!P->mr_small) P->mr_small = P->mem.take<uint64_t>((size_t)NkMrSmallLayout::total_words(P->ws.nb_max), who);
    if (P->mr_a_words < wa) P->mr_a_words = P->mem.regrow(P->mr_a, wa * 8, who) ? wa : 0;
    if (P->mr_b_words < wb) P->mr_b_words = P->mem.regrow(P->mr_b, wb * 8, who) ? wb : 0;
    return P->mem.status();
}

// ---- host side of the one-pass step (device code: nk_onepass.h; the two policies: nk_policy.h; the device blocks: nk_layout.h) ----
// where a step's results go
struct NkStepOut { double* vshift; int64_t* n_valid; double *y_mean, *y_std, *edges; int64_t* counts; double* medians; };

// (the step's small results and the ONE table that says where each comes from -- NkStepResults, nk_fetch_bytes: nk_layout.h)
static_assert(NK_FETCH_MAX <= (int)(sizeof(FzPack::bytes) / sizeof(uint32_t)), "the pack kernel's argument holds every item");

// what became of a step on this route
enum NkOutcome { NK_STEP_DONE, NK_STEP_PLAIN /* the plain route takes the step */, NK_STEP_AGAIN /* once more, with sampled brackets */ };

// One step on the one-pass route: the context every stage works in, and the stages in the order nk_step_onepass queues them.
template <typename T> struct NkOnepass {
    typedef typename KeyT<T>::type K;
    static constexpr int BR_PASSES = 3;
    xdemhip_nk_plan* const P;
    xdemhip_ctx* const ctx;
    SelWorkspace* const ws;
    const NkGeom& g;
    const int64_t q0, n;
    const int nb;
    const int64_t rows, n_slots;
    const bool mr;   // a partitioned plan: this rank's rows, every count and order statistic over all ranks
    const int world, rank;
    const NkFzLayout<T> fz;
    NkMrSmallLayout mrs;     // (partitioned plans, once the ranks have agreed on the route -- eligible; null members otherwise)
    unsigned char* const scratch;
    T* const d_edges;
    DhStats* const d_stats;
    BinCacheRec* const d_rec;
    const SelState<K>* const d_st;
    uint64_t* const ext_slots;   // partitioned plans: per-rank slots of min / max aspect and the EXT survivors, behind the two histograms of the dh sample's selection
    const T *const ref_m, *const tba, *const st_all;
    T* const s_v;
    const bool custom;
    const int last_decimal;
    const K low_mask;
    const int narrow;        // the code this step's sample brackets are taken with
    NkStepBrackets br;       // sampled or predicted brackets (NkPrediction::plan)
    int n_wg = 0;            // workgroups of the pass
    int dsel_grid = 0;
    NkStepResults<T, K, SelState<K>> h;   // (sized by stage_fetch: a step that takes the plain route allocates nothing here)

    NkOnepass(xdemhip_nk_plan* P_, const NkGeom& g_, int64_t q0_, int64_t n_, int nb_)
        : P(P_), ctx(P_->ctx), ws(&P_->ws), g(g_), q0(q0_), n(n_), nb(nb_), rows(P_->row1 - P_->row0),
          n_slots(((((n_ + SEL_LINE - 1) >> SEL_LINE_LOG2) + 63) >> 6) << SEL_LINE_LOG2), mr(P_->ctx->allreduce != nullptr), world(P_->ctx->world),
          rank(P_->ctx->rank), fz(P_->fz, P_->ws.nb_max), mrs(nullptr, P_->ws.nb_max), scratch(static_cast<unsigned char*>(P_->scratch)),
          d_edges(reinterpret_cast<T*>(scratch)), d_stats(reinterpret_cast<DhStats*>(scratch + OFF_STATS)),
          d_rec(reinterpret_cast<BinCacheRec*>(scratch + OFF_INFO + 64)), d_st(reinterpret_cast<const SelState<K>*>(scratch + OFF_STATE)),
          ext_slots(reinterpret_cast<uint64_t*>(scratch + off_hist(2)) + 2 * SEL_RADIX), ref_m(static_cast<const T*>(P_->ref_m)),
          tba(static_cast<const T*>(P_->tba)), st_all(static_cast<const T*>(P_->slope_tan)), s_v(static_cast<T*>(P_->ws.s_vals)),
          custom(!P_->custom_edges.empty()), last_decimal(custom ? P_->custom_decimal : NK_AUTO_EDGES),
          low_mask((K)(((K)1 << (8 * (KeyT<T>::passes - BR_PASSES))) - 1)), narrow(P_->narrowing.narrow) {}

    // ---- does the route apply?  (*go stays false: the caller runs the plain route, which needs nothing from here) ----------------
    int eligible(bool* go) {
        *go = false;
        bool cannot = !ctx->nk_fused || !P->fz || !P->cd_vals || !P->c_st || !P->bcache || !P->ext_ok || (g.rule > 1 && !P->badbits) || rows <= 0 ||
                      P->bin_stat != XDEMHIP_BINSTAT_MEDIAN || !(ctx->selection_mode == 0 || ctx->selection_mode == 3) || !ws->d_small ||
                      (int64_t)P->nbuf * P->W < ws->c_cap ||   // (the kept bin candidates go into per-bin segments of the y raster)
                      ws->es != sizeof(T) || nb > ws->nb_max || nb > MAX_BINS_PER_SWEEP || n_slots > ws->s_cap ||
                      (int64_t)(NKZ_CHUNK_MAX + 2) * P->W * (int64_t)sizeof(T) >= ((int64_t)1 << 32);   // (32-bit byte offsets inside a chunk of rows)
        int64_t n_all = n;   // pixels of all ranks
        if (mr && (world < 1 || !ctx->nk_fused_dist || !ctx->nk_fused)) return XDEMHIP_OK;   // (not told the ranks / switched off: context-level, the same on every rank)
        if (mr) {
            // Every rank must take the same route.  What the decision rests on is either fixed for the plan and its options or derives
            // from reduced data (ext_ok), so the ranks agree ONCE -- a host all-reduce of (own pixels, "I cannot") -- and again whenever
            // any of it changes, which it does on all ranks at the same step.
            const int64_t key[8] = {nb, P->row0, P->row1, (int64_t)P->ext_ok, (int64_t)P->bin_stat, (int64_t)ctx->selection_mode,
                                    (int64_t)(ctx->nk_fused * 4 + ctx->nk_fused_dist * 2), (int64_t)world * 64 + rank};
            if (memcmp(key, P->mr_key, sizeof key) != 0) {
                cannot = cannot || !ctx->nk_fused_dist || world < 1 || world > MR_WORLD_MAX || rank < 0 || rank >= world ||
                         (int64_t)P->nbuf * P->W < ws->c_cap;
                if (!cannot && nk_mr_alloc(P, nb, world, sizeof(T)) != XDEMHIP_OK) cannot = true;
                uint64_t v[2] = {(uint64_t)n, (uint64_t)(cannot ? 1 : 0)};
                const int rc_ = xd_allreduce_host(ctx, v, 2, XDEMHIP_RED_SUM_U64);
                if (rc_) return rc_;
                P->mr_nglob = (int64_t)v[0];
                P->mr_can = v[1] == 0;
                memcpy(P->mr_key, key, sizeof key);
            }
            if (!P->mr_can) return XDEMHIP_OK;
            n_all = P->mr_nglob;
            mrs = NkMrSmallLayout(P->mr_small, ws->nb_max);   // (allocated with the agreement: nk_mr_alloc)
        } else if (cannot) {
            return XDEMHIP_OK;
        }
        if (n_all < SEL_BRACKET_MIN_N || (ctx->selection_mode == 0 && n_all < SEL_BRACKET_MIN_PER_BIN * nb)) return XDEMHIP_OK;
        *go = true;
        return XDEMHIP_OK;
    }

    // edges from the min / max aspect in d_stats, freshness of the bin cache, (re)fill of the cache
    int edges_and_bins() {
        hipLaunchKernelGGL((nk_fz_prep_kernel<T>), dim3(1), dim3(64), 0, ctx->stream, d_stats, P->ext_cnt + 2, nb, (int)custom, d_edges, d_rec,
                           (int)P->bcache_force, fz.ctr);
        hipLaunchKernelGGL((nk_bin_fill_kernel<T>), dim3(grid_for(ctx, n, 256, 16)), dim3(256), sizeof(T) * (nb + 1), ctx->stream,
                           static_cast<const T*>(P->aspect) + q0, n, d_edges, nb, last_decimal, d_rec, P->bcache + q0);
        hipLaunchKernelGGL((nk_bin_cache_commit_kernel<T>), dim3(1), dim3(64), 0, ctx->stream, d_edges, nb, d_rec);
        XD_HIP_CHECK(ctx, hipGetLastError());
        P->bcache_force = false;
        return XDEMHIP_OK;
    }
    // partitioned plans: min / max aspect and the EXT survivors of all ranks, once their slots are reduced -> edges and bin cache
    int edges_and_bins_of_all_ranks() {
        hipLaunchKernelGGL(nk_mr_ext_unpack_kernel, dim3(1), dim3(64), 0, ctx->stream, ext_slots, world, d_stats, P->ext_cnt + 2);
        return edges_and_bins();
    }

    // ---- 1. min / max aspect of this step from the EXT lists -> edges, freshness of the bin cache; (re)fill of the cache ---------
    int stage_edges() {
        if (custom) {  // explicit bin edges: SciPy casts them to the sample dtype (rare path: a blocking copy)
            std::vector<T> e(P->custom_edges.size());
            for (size_t k = 0; k < e.size(); ++k) e[k] = (T)P->custom_edges[k];
            XD_HIP_CHECK(ctx, hipMemcpyAsync(d_edges, e.data(), sizeof(T) * e.size(), hipMemcpyHostToDevice, ctx->stream));
            { const int rc_ = xd_sync(ctx); if (rc_) return rc_; }
        }
        static_assert(MAX_BINS_PER_SWEEP <= NK_BINCACHE_MAX_BINS, "the one-pass step's bins fit the byte-wide cache");
        hipLaunchKernelGGL(nk_step_init_kernel, dim3(1), dim3(1024), 0, ctx->stream, d_stats, fz.base, fz.zeroed_words(fz.nbm), P->ext_cnt + 2);
        hipLaunchKernelGGL((nk_ext_eval_kernel<T>), dim3(EXT_CAP / 256, 2), dim3(256), 0, ctx->stream, ref_m, tba, static_cast<const T*>(P->aspect), g,
                           P->ext_idx, P->ext_cnt, d_stats, P->ext_cnt + 2);
        // (partitioned plans: min / max aspect and the survivors of all ranks arrive with the first histogram all-reduce of the dh sample's
        //  selection -- per-rank slots behind its two histograms -- so the edges and the bin cache, which only the y^ sample and the
        //  pass need, follow that selection: edges_and_bins_of_all_ranks in the bracket stages)
        if (mr) hipLaunchKernelGGL(nk_mr_ext_pack_kernel, dim3(1), dim3(64), 0, ctx->stream, d_stats, P->ext_cnt + 2, rank, world, ext_slots);
        if (!mr) return edges_and_bins();
        return XDEMHIP_OK;
    }

    // ---- 2 + 3, predicted: every bracket from the previous step's medians (NkPrediction::plan) -------------------------------------
    int launch_predicted(int nb_pred) {
        NkPredicted<T> pr;
        pr.dlo = (T)(P->pred.v - br.hd);
        pr.dhi = (T)(P->pred.v + br.hd);
        for (int b = 0; b < nb_pred; ++b) { pr.lo[b] = (T)br.lo[b]; pr.hi[b] = (T)br.hi[b]; }
        hipLaunchKernelGGL((nk_predict_kernel<T>), dim3(1), dim3(64), 0, ctx->stream, pr, nb_pred, fz.klo_d, fz.khi_d, fz.rbs_d, fz.vhat, fz.delta, fz.klo_y,
                           fz.khi_y, fz.rbs_y, fz.ctr);
        XD_HIP_CHECK(ctx, hipGetLastError());
        return XDEMHIP_OK;
    }
    int stage_brackets_predicted() {
        if (mr) {   // min / max aspect and the EXT survivors of all ranks: their own small exchange (they ride on the dh sample's first histogram otherwise)
            { const int rc_ = xd_allreduce_device(ctx, ext_slots, 4 * (int64_t)world, XDEMHIP_RED_SUM_U64); if (rc_) return rc_; }
            { const int rc_ = edges_and_bins_of_all_ranks(); if (rc_) return rc_; }
        }
        return launch_predicted(nb);
    }

    // ---- 2 + 3, sampled: sample of dh -> bracket of its median, v^, delta; then the bins' ----------------------------------------
    // (the sample kernels also reset the selection that runs on their sample -- select_reset_slice; the passes advance their own
    //  states and the last one writes the bracket ends -- hist_pass_kernel<T, true>; `fused` tells whether that form ran)
    int stage_brackets_sampled() {
        hipLaunchKernelGGL((nk_sample_dh_kernel<T>), dim3(grid_for(ctx, n_slots, 256, 8)), dim3(256), 0, ctx->stream, ref_m, tba, g, q0, n,
                           1.0 / (double)P->W, n_slots, s_v, select_reset_plan<K>(scratch, 1, SEL_BRACKET_DUAL));
        XD_HIP_CHECK(ctx, hipGetLastError());
        bool fused = false;
        const int rc = select_enqueue<T>(ctx, s_v, nullptr, n_slots, n_slots, nullptr, 1, scratch, SEL_BRACKET_DUAL, nullptr, BR_PASSES, false, nullptr, nullptr,
                                         false, narrow, fz.klo_d, fz.khi_d, fz.rbs_d, low_mask, &fused, true, mr ? 0 : -1, mr ? 4 * (int64_t)world : 0);
        if (rc) return rc;
        if (!fused) hipLaunchKernelGGL((bracket_finish_kernel<K>), dim3(1), dim3(64), 0, ctx->stream, d_st, 1, 0, low_mask, fz.klo_d, fz.khi_d, fz.rbs_d);
        return bin_brackets_sampled(false);
    }

    // ---- 3. sample of y^ per aspect bin -> brackets of the bin medians (v^ and delta formed by the sample kernel itself) ---------
    // `from_rasters`: no dh sample in memory -- the y^ sample is formed straight from the rasters
    int bin_brackets_sampled(bool from_rasters) {
        if (mr) { const int rc_ = edges_and_bins_of_all_ranks(); if (rc_) return rc_; }
        if (from_rasters)
            hipLaunchKernelGGL((nk_sample_dy_kernel<T>), dim3(grid_for(ctx, n_slots, 256, 8)), dim3(256), 0, ctx->stream, ref_m, tba, g, q0, n,
                               1.0 / (double)P->W, n_slots, s_v, ws->s_bins, st_all + q0, P->bcache + q0, fz.klo_d, fz.khi_d, fz.vhat, fz.delta, fz.ctr,
                               select_reset_plan<K>(scratch, nb, SEL_BRACKET_DUAL));
        else
            hipLaunchKernelGGL((nk_sample_y_kernel<T>), dim3(grid_for(ctx, n_slots, 256, 8)), dim3(256), 0, ctx->stream, s_v, ws->s_bins, st_all + q0,
                               P->bcache + q0, n, n_slots, fz.vhat, fz.klo_d, fz.khi_d, fz.vhat, fz.delta, fz.ctr, select_reset_plan<K>(scratch, nb, SEL_BRACKET_DUAL));
        XD_HIP_CHECK(ctx, hipGetLastError());
        bool fused = false;
        const int rc = select_enqueue<T>(ctx, s_v, nb == 1 ? nullptr : ws->s_bins, n_slots, n_slots, nullptr, nb, scratch, SEL_BRACKET_DUAL, nullptr, BR_PASSES,
                                         false, nullptr, nullptr, false, narrow, fz.klo_y, fz.khi_y, fz.rbs_y, low_mask, &fused, true);
        if (rc) return rc;
        if (!fused) hipLaunchKernelGGL((bracket_finish_kernel<K>), dim3(1), dim3(64), 0, ctx->stream, d_st, nb, 0, low_mask, fz.klo_y, fz.khi_y, fz.rbs_y);
        XD_HIP_CHECK(ctx, hipGetLastError());
        return XDEMHIP_OK;
    }

    // ---- 2 + 3, the bracket of the median of dh predicted: no dh sample and no selection on it; the bins' brackets sampled -------
    int stage_brackets_dh_predicted() {
        if (mr) { const int rc_ = xd_allreduce_device(ctx, ext_slots, 4 * (int64_t)world, XDEMHIP_RED_SUM_U64); if (rc_) return rc_; }
        { const int rc_ = launch_predicted(0); if (rc_) return rc_; }
        return bin_brackets_sampled(true);
    }

    // ---- 4. the one pass --------------------------------------------------------------------------------------------------------
    int stage_pass() {
        dim3 grid = grid2d(ctx, P->W, rows);
        if ((rows + grid.y - 1) / grid.y > NKZ_CHUNK_MAX) grid.y = (unsigned)((rows + NKZ_CHUNK_MAX - 1) / NKZ_CHUNK_MAX);
        n_wg = (int)(grid.x * grid.y);
        if ((size_t)n_wg > P->wg_sums_cap) {   // (per-workgroup slots of the pass's five float64 sums: nk_sums_reduce)
            P->wg_sums_cap = P->mem.regrow(P->wg_sums, (size_t)n_wg * 5 * sizeof(double), "per-workgroup sums of the one-pass step") ? (size_t)n_wg : 0;
            { const int rc_ = P->mem.status(); if (rc_) return rc_; }
        }
        int copies = (4608) / (nb * 12);   // (static 26 KB + this: five workgroups of 256 threads per CU)
        copies = copies < 1 ? 1 : (copies > 16 ? 16 : copies);
        const size_t lds = (size_t)nb * sizeof(FzPair<T>) + (size_t)((3 * nb) | 1) * 4 * (size_t)copies + 64 * 4;
        T* cy_d = static_cast<T*>(ws->c_vals);
#define XD_NK_FZ(RULE)                                                                                                                     \
    hipLaunchKernelGGL((nk_fused_kernel<T, RULE>), grid, dim3(256), lds, ctx->stream, ref_m, tba, st_all, P->bcache, g, P->row0, P->row1,        \
                       P->nbuf, nb, copies, fz.klo_d, fz.khi_d, fz.vhat, fz.delta, fz.klo_y, fz.khi_y, fz.cnt_d, fz.cls_y,                       \
                       static_cast<T*>(P->cd_vals), P->cd_cap, cy_d, static_cast<T*>(P->c_st), ws->c_bins, ws->c_cap, fz.ctr, P->wg_sums,        \
                       P->badbits, P->bad_wpr)
        if (g.rule == 0) XD_NK_FZ(0);
        else if (g.rule == 1) XD_NK_FZ(1);
        else XD_NK_FZ(2);
#undef XD_NK_FZ
        XD_HIP_CHECK(ctx, hipGetLastError());
        // (few workgroups for the histogram / gather of the dh candidates: every one of them ends with an atomic on ONE word, which
        //  serialise -- 256 workgroups with an atomic per wave spent 80 us there)
        dsel_grid = grid_for(ctx, n / 32 + 1, HIST_THREADS * 8, 1);
        dsel_grid = dsel_grid > 64 ? 64 : dsel_grid;
        return XDEMHIP_OK;
    }

    // ---- 5. exact median of dh among its candidates -> vshift: value buckets of the bracket, three launches (nk_dhsel_*) ---------
    static size_t dhsel_final_lds() {
        return (size_t)DSEL_CAP * sizeof(K) + (size_t)(BINSEL_COPIES * (SEL_RADIX + 1) + 1) * 4 + (size_t)(SEL_RADIX + 4 + 16 + 2) * 8;
    }
    int stage_median_dh() {
        const T* cd = static_cast<const T*>(P->cd_vals);
        const size_t lds = dhsel_final_lds();
        { const int rc_ = set_big_lds(ctx, nk_dhsel_final_kernel<T>, lds); if (rc_) return rc_; }
        hipLaunchKernelGGL((nk_dhsel_hist_kernel<T>), dim3(dsel_grid), dim3(HIST_THREADS), 0, ctx->stream, cd, P->cd_cap, fz.ctr + 1, fz.klo_d, fz.khi_d,
                           fz.dsel_hist(), P->wg_sums, n_wg, fz.sums);
        hipLaunchKernelGGL((nk_dhsel_gather_kernel<T>), dim3(dsel_grid), dim3(HIST_THREADS), 0, ctx->stream, cd, P->cd_cap, fz.ctr + 1, fz.cnt_d, fz.klo_d,
                           fz.khi_d, fz.dsel, fz.dsel_keys, fz.ctr);
        hipLaunchKernelGGL((nk_dhsel_final_kernel<T>), dim3(1), dim3(HIST_THREADS), lds, ctx->stream, P->cd_cap, fz.ctr + 1, fz.cnt_d, fz.klo_d, fz.khi_d, fz.dsel,
                           fz.dsel_keys, fz.ctr, scratch + OFF_INFO);
        XD_HIP_CHECK(ctx, hipGetLastError());
        return XDEMHIP_OK;
    }
    // ... on partitioned plans, behind the exchange of the pass's counters
    int stage_median_dh_partitioned() {
        const T* cd = static_cast<const T*>(P->cd_vals);
        // exchange 7: the pass's counters summed, the five float64 sums of every rank gathered and added in rank order -- and, in the
        // same all-reduce, the 4096-bucket histogram of this rank's dh candidates in its own row (the candidates and the bracket
        // are there once the pass is through; only the choice of the bucket needs the summed counters)
        const int64_t words7 = 3 + 3 * (int64_t)nb + 5 * (int64_t)world;
        uint32_t* mr_rows = reinterpret_cast<uint32_t*>(P->mr_a + words7);   // [world][DSEL_BUCKETS]
        XD_HIP_CHECK(ctx, hipMemsetAsync(mr_rows, 0, (size_t)world * DSEL_BUCKETS * 4, ctx->stream));
        hipLaunchKernelGGL(nk_mr_counts_pack_kernel, dim3(1), dim3(256), 0, ctx->stream, fz.cnt_d, fz.cls_y, P->wg_sums, n_wg, nb, rank, world, P->mr_a,
                           mrs.cls_loc);
        hipLaunchKernelGGL((nk_dhsel_hist_kernel<T>), dim3(dsel_grid), dim3(HIST_THREADS), 0, ctx->stream, cd, P->cd_cap, fz.ctr + 1, fz.klo_d, fz.khi_d,
                           mr_rows + (size_t)rank * DSEL_BUCKETS);
        XD_HIP_CHECK(ctx, hipGetLastError());
        { const int rc_ = xd_allreduce_device(ctx, P->mr_a, words7 + (int64_t)world * (DSEL_BUCKETS / 2), XDEMHIP_RED_SUM_U64); if (rc_) return rc_; }
        hipLaunchKernelGGL(nk_mr_counts_unpack_kernel, dim3(1), dim3(256), 0, ctx->stream, P->mr_a, nb, world, fz.cnt_d, fz.cls_y, fz.sums);
        XD_HIP_CHECK(ctx, hipGetLastError());
        const size_t lds = dhsel_final_lds();
        { const int rc_ = set_big_lds(ctx, nk_dhsel_final_kernel<T>, lds); if (rc_) return rc_; }
        // (the rows of exchange 7) -> the global histogram, the bucket, this rank's offset in the bucket's key list
        hipLaunchKernelGGL((nk_mr_dh_base_kernel<T>), dim3(1), dim3(HIST_THREADS), 0, ctx->stream, mr_rows, world, rank, fz.cnt_d, fz.klo_d, fz.khi_d, fz.dsel,
                           fz.ctr);
        // exchange 8: the bucket's keys of all ranks, each at its offset, + every rank's header words
        uint64_t* slots = P->mr_b;
        K* gk = reinterpret_cast<K*>(P->mr_b + (size_t)world * DSEL_HDR_WORDS);
        const int64_t words8 = (int64_t)world * DSEL_HDR_WORDS + (int64_t)DSEL_CAP * (int64_t)sizeof(K) / 8;
        XD_HIP_CHECK(ctx, hipMemsetAsync(P->mr_b, 0, (size_t)words8 * 8, ctx->stream));
        hipLaunchKernelGGL((nk_dhsel_gather_kernel<T>), dim3(dsel_grid), dim3(HIST_THREADS), 0, ctx->stream, cd, P->cd_cap, fz.ctr + 1, fz.cnt_d, fz.klo_d,
                           fz.khi_d, fz.dsel, gk, fz.ctr, 0);
        hipLaunchKernelGGL(nk_mr_dh_hdr_pack_kernel, dim3(1), dim3(64), 0, ctx->stream, fz.dsel, rank, slots);
        XD_HIP_CHECK(ctx, hipGetLastError());
        { const int rc_ = xd_allreduce_device(ctx, P->mr_b, words8, XDEMHIP_RED_SUM_U64); if (rc_) return rc_; }
        hipLaunchKernelGGL(nk_mr_dh_hdr_merge_kernel, dim3(1), dim3(64), 0, ctx->stream, slots, world, fz.dsel);
        hipLaunchKernelGGL((nk_dhsel_final_kernel<T>), dim3(1), dim3(HIST_THREADS), lds, ctx->stream, P->cd_cap, fz.ctr + 1, fz.cnt_d, fz.klo_d, fz.khi_d, fz.dsel, gk,
                           fz.ctr, scratch + OFF_INFO, 0);
        XD_HIP_CHECK(ctx, hipGetLastError());
        return XDEMHIP_OK;
    }

    // ---- 6. the bin candidates with the exact vshift -> counts, exact medians among those inside the brackets --------------------
    // kept values into per-bin segments (in the y raster, which this route does not use), one workgroup per bin selects
    void resolve_scatter() {
        const size_t lds = (size_t)nb * (3 * 8 + 2 * sizeof(K) + 3 * 4) + 16;
        hipLaunchKernelGGL((nk_resolve_scatter_kernel<T>), dim3(grid_for(ctx, n / 16 + 1, HIST_THREADS * BINSEG_U, 2)), dim3(HIST_THREADS), lds, ctx->stream,
                           static_cast<const T*>(ws->c_vals), static_cast<const T*>(P->c_st), ws->c_bins, ws->c_cap, fz.ctr + 5,
                           reinterpret_cast<const T*>(scratch + OFF_INFO), nb, fz.klo_y, fz.khi_y, fz.cls_y, fz.res_y, fz.seg_ctr, static_cast<T*>(P->y),
                           (int64_t)P->nbuf * P->W, fz.ctr, mrs.cls_loc);
    }
    static size_t bin_select_lds() { return (size_t)BINSEL_KEY_BYTES + (size_t)(BINSEL_COPIES * (SEL_RADIX + 1) + 1) * 4 + (size_t)(SEL_RADIX + 8) * 8; }
    int stage_bin_medians() {
        resolve_scatter();
        const size_t lds2 = bin_select_lds();
        { const int rc_ = set_big_lds(ctx, nk_bin_select_kernel<T>, lds2); if (rc_) return rc_; }
        hipLaunchKernelGGL((nk_bin_select_kernel<T>), dim3(nb), dim3(HIST_THREADS), lds2, ctx->stream, static_cast<const T*>(P->y), fz.cls_y, fz.res_y, fz.seg_ctr, nb,
                           fz.klo_y, fz.khi_y, fz.rbs_y, reinterpret_cast<SelState<K>*>(scratch + OFF_STATE), reinterpret_cast<uint64_t*>(scratch + off_succ(nb)),
                           fz.cnt_y, fz.ctr);
        XD_HIP_CHECK(ctx, hipGetLastError());
        return XDEMHIP_OK;
    }
    int stage_bin_medians_partitioned() {
        resolve_scatter();
        const size_t lds2 = bin_select_lds();
        { const int rc_ = set_big_lds(ctx, nk_bin_select_kernel<T>, lds2); if (rc_) return rc_; }
        // exchange 9: per bin the value-bucket histogram of this rank's segment, one row per rank; the resolved counters; local flags
        const int64_t words9 = 2 + 2 * (int64_t)nb + (int64_t)world * nb * (SEL_RADIX / 2);
        XD_HIP_CHECK(ctx, hipMemsetAsync(P->mr_a, 0, (size_t)words9 * 8, ctx->stream));
        hipLaunchKernelGGL((nk_mr_bin_hist_kernel<T>), dim3(nb), dim3(HIST_THREADS), 0, ctx->stream, static_cast<const T*>(P->y), mrs.cls_loc, fz.res_y, fz.seg_ctr, nb,
                           fz.klo_y, fz.khi_y, rank, world, P->mr_a, fz.ctr);
        XD_HIP_CHECK(ctx, hipGetLastError());
        { const int rc_ = xd_allreduce_device(ctx, P->mr_a, words9, XDEMHIP_RED_SUM_U64); if (rc_) return rc_; }
        // exchange 10: per bin the chosen bucket's values of all ranks (+ each rank's smallest value above it)
        const int64_t words10 = (int64_t)nb * MR_GSEG * (int64_t)sizeof(T) / 8;
        XD_HIP_CHECK(ctx, hipMemsetAsync(P->mr_b, 0, (size_t)words10 * 8, ctx->stream));
        hipLaunchKernelGGL((nk_mr_bin_gather_kernel<T>), dim3(nb), dim3(HIST_THREADS), 0, ctx->stream, static_cast<const T*>(P->y), mrs.cls_loc, fz.cls_y, P->mr_a,
                           fz.seg_ctr, nb, fz.klo_y, fz.khi_y, rank, world, reinterpret_cast<T*>(P->mr_b), mrs.cls_f, mrs.res_f, mrs.segf_ctr, mrs.cnt_true, fz.ctr);
        XD_HIP_CHECK(ctx, hipGetLastError());
        { const int rc_ = xd_allreduce_device(ctx, P->mr_b, words10, XDEMHIP_RED_SUM_U64); if (rc_) return rc_; }
        hipLaunchKernelGGL((nk_bin_select_kernel<T>), dim3(nb), dim3(HIST_THREADS), lds2, ctx->stream, reinterpret_cast<const T*>(P->mr_b), mrs.cls_f, mrs.res_f,
                           mrs.segf_ctr, nb, fz.klo_y, fz.khi_y, fz.rbs_y, reinterpret_cast<SelState<K>*>(scratch + OFF_STATE),
                           reinterpret_cast<uint64_t*>(scratch + off_succ(nb)), fz.cnt_y, fz.ctr, (int64_t)MR_GSEG);
        XD_HIP_CHECK(ctx, hipGetLastError());
        return XDEMHIP_OK;
    }

    // ---- 7. everything the step hands back: packed into one block on the device, one copy, one synchronisation -------------------
    int stage_fetch() {
        NkFetchItem t[NK_FETCH_MAX];
        FzPack pk;
        h.resize(nb, mr);
        pk.n = h.table(fz, mrs, NkScratchSrc{scratch + OFF_INFO, d_edges, scratch + OFF_STATE, scratch + off_succ(nb)}, nb, mr, t);
        const uint32_t total = (uint32_t)nk_fetch_offsets(t, pk.n, pk.off);
        for (int k = 0; k < pk.n; ++k) {
            pk.src[k] = static_cast<const unsigned char*>(t[k].src);
            pk.bytes[k] = (uint32_t)t[k].bytes;
        }
        if (total > P->fz_pack_bytes) return xd_fail(ctx, XDEMHIP_EINVAL, "one-pass step: result block too small");
        P->fz_host.resize(total);
        // (the block is written straight into the pinned staging buffer where there is room -- no copy behind the kernel)
        unsigned char* pin = xd_pin_claim(ctx, P->fz_host.data(), total);
        pk.dst = pin ? pin : P->fz_pack;
        hipLaunchKernelGGL(nk_fz_pack_kernel, dim3(1), dim3(256), 0, ctx->stream, pk);
        XD_HIP_CHECK(ctx, hipGetLastError());
        if (!pin) { const int rc_ = xd_d2h(ctx, P->fz_host.data(), P->fz_pack, total); if (rc_) return rc_; }
        { const int rc_ = xd_sync(ctx); if (rc_) return rc_; }
        for (int k = 0; k < pk.n; ++k) memcpy(t[k].dst, P->fz_host.data() + pk.off[k], t[k].bytes);
        return XDEMHIP_OK;
    }

    // ---- 8. what the fetched integers say: a miss, or the step's numbers; the two policies learn from them -----------------------
    int stage_interpret(const NkStepOut& out, NkOutcome* outcome) {
        const unsigned long long* h_ctr = h.ctr();
        const bool fell = h_ctr[2] != 0 || h_ctr[3] != 0;   // overflow / a bracket missed / no extreme-aspect survivor
        if (fell && getenv("XDEMHIP_DEBUG"))
            fprintf(stderr, "[xdemhip] one-pass step falls through: overflow flag %llu, miss flag %llu, dh candidates %llu, bin candidates %llu\n", h_ctr[2], h_ctr[3],
                    h_ctr[1], h_ctr[5]);
        if (fell && (br.predict || br.predict_d)) {
            P->pred.on_miss();
            *outcome = NK_STEP_AGAIN;
            return XDEMHIP_OK;
        }
        if (fell) {
            if (h_ctr[6] != 0) P->ext_ok = false;   // (no listed extreme-aspect pixel kept a finite dh: this plan reads the aspect from now on -- identical on every rank, the flag derives from reduced counts)
            P->narrowing.on_miss(narrow);
            P->pred.forget();
            *outcome = NK_STEP_PLAIN;
            return XDEMHIP_OK;
        }
        if (!br.predict) {   // (offsets are measured in half widths of the bracket that was used)
            const double unit = sel_narrow_unit((uint32_t)narrow);
            const std::vector<uint64_t>& c = mr ? h.cnt_t : h.cnt;
            if (!br.predict_d) P->narrowing.observe(h.cnt_d()[0], h.cnt_d()[1], h.cnt_d()[2], unit);   // (a predicted bracket says nothing about the centring of sample brackets)
            for (int b = 0; b < nb; ++b) P->narrowing.observe(c[b], c[nb + b], c[2 * nb + b], unit);
            P->narrowing.choose_next(ctx->nk_narrow);
        }
        uint64_t total;
        double vs;
        memcpy(&total, h.info + 8, 8);
        memcpy(&vs, h.info + 24, 8);
        *out.n_valid = (int64_t)total;
        if (total == 0) return xd_fail(ctx, XDEMHIP_EINVAL, "The subsample contains no more valid values.");
        *out.vshift = vs;
        const int rbs = (int)(uint32_t)h.rbs;
        for (int b = 0; b < nb; ++b) {
            const uint64_t tot = h.cnt[b], lt = h.cnt[nb + b];
            if (tot == 0) { out.counts[b] = 0; out.medians[b] = NAN; continue; }
            SelResult<K> r;
            r.st = h.st[b];
            r.succ = h.succ[b];
            r.st.count = tot;
            r.st.n_le += lt;
            r.st.prefix = (K)((K)(r.st.prefix >> rbs) + h.klo[b]);  // back from the rebased candidate keys
            if (r.succ != ~(uint64_t)0) r.succ = (uint64_t)(K)((K)((K)r.succ >> rbs) + h.klo[b]);
            out.counts[b] = (int64_t)tot;
            out.medians[b] = median_from<T>(r);
        }
        for (int k = 0; k <= nb; ++k) out.edges[k] = (double)h.edges[k];
        // nanmean / nanstd of y from the sums of y^ and the first-order correction in (v^ - vshift)
        const double dlt = (double)h.vhat - vs, cntd = (double)total;
        const double s1 = h.sums[0] + dlt * h.sums[2];
        const double s2 = h.sums[1] + 2.0 * dlt * h.sums[3] + dlt * dlt * h.sums[4];
        const double mean = s1 / cntd, var = s2 / cntd - mean * mean;
        *out.y_mean = mean;
        *out.y_std = var > 0 ? sqrt(var) : 0.0;
        std::vector<double> lo(nb), hi(nb);   // (keys are order preserving: the brackets' ends as values)
        for (int b = 0; b < nb; ++b) { lo[b] = (double)val_of(h.klo[b]); hi[b] = (double)val_of(h.khi[b]); }
        P->pred.record(br, g.dc, g.dr, nb, vs, out.medians, out.counts, out.edges, lo.data(), hi.data(), (double)val_of(h.kd[0]), (double)val_of(h.kd[1]), narrow);
        *outcome = NK_STEP_DONE;
        return XDEMHIP_OK;
    }
};

// *done = false (nothing returned) when the route does not apply or when a bracket missed / a buffer overflowed: the caller
// then runs the plain route, which needs nothing from here.  A PREDICTED bracket that missed sends the step round once more with
// sampled brackets.
template <typename T>
int nk_step_onepass(xdemhip_nk_plan* P, const NkGeom& g, int64_t q0, int64_t n, int nb, bool* done, const NkStepOut& out) {
    *done = false;
    for (int trip = 0; trip < 2; ++trip) {
        NkOnepass<T> s(P, g, q0, n, nb);
        bool go = false;
        { const int rc_ = s.eligible(&go); if (rc_ || !go) return rc_; }
        { const int rc_ = s.stage_edges(); if (rc_) return rc_; }
        // (the prediction's record holds the previous tap offsets in pixels)
        s.br = P->pred.plan(g.dc - P->pred.sx, -(g.dr - P->pred.sy), nb, trip == 0, P->ctx->nk_predict);
        // (the three forms are named in the order the step used to hold them: the compiler then emits their kernels in the same order,
        //  and the device code of this file stays what it was byte for byte)
        { const int rc_ = s.br.predict ? s.stage_brackets_predicted() : (!s.br.predict_d ? s.stage_brackets_sampled() : s.stage_brackets_dh_predicted()); if (rc_) return rc_; }
        { const int rc_ = s.stage_pass(); if (rc_) return rc_; }
        { const int rc_ = s.mr ? s.stage_median_dh_partitioned() : s.stage_median_dh(); if (rc_) return rc_; }
        { const int rc_ = s.mr ? s.stage_bin_medians_partitioned() : s.stage_bin_medians(); if (rc_) return rc_; }
        { const int rc_ = s.stage_fetch(); if (rc_) return rc_; }
        NkOutcome outcome = NK_STEP_PLAIN;
        { const int rc_ = s.stage_interpret(out, &outcome); if (rc_) return rc_; }
        if (outcome != NK_STEP_AGAIN) { *done = outcome == NK_STEP_DONE; return XDEMHIP_OK; }
    }
    return XDEMHIP_OK;   // (not reached: the second trip predicts nothing)
}

template <typename T>
int nk_step_typed(xdemhip_nk_plan* P, double shift_x, double shift_y, double res_x, double res_y, int nb, double* vshift,
                  int64_t* n_valid, double* y_mean, double* y_std, double* edges_out, int64_t* counts, double* medians,
                  double* fit_sums /* non-null: the un-binned least-squares sums instead of the binning */) {
    typedef typename KeyT<T>::type K;
    xdemhip_ctx* ctx = P->ctx;
    const int64_t q0 = (P->row0 - P->roff) * P->W;
    const int64_t n = (P->row1 - P->row0) * P->W;
    unsigned char* base = static_cast<unsigned char*>(P->scratch);
    double* d_sums = reinterpret_cast<double*>(base + OFF_SUMS);
    const T* dh = static_cast<const T*>(P->dh) + q0;
    const T* st = static_cast<const T*>(P->slope_tan) + q0;
    const T* asp = static_cast<const T*>(P->aspect) + q0;
    T* y = static_cast<T*>(P->y) + q0;
    uint16_t* bins = P->bins + q0;
    T* d_edges = reinterpret_cast<T*>(base);
    T* d_vshift = reinterpret_cast<T*>(base + OFF_INFO);
    if (!P->custom_edges.empty()) nb = (int)P->custom_edges.size() - 1;

    // tba is sampled at (row - shift_y / res_y, col + shift_x / res_x); the taps of this rank's rows must lie in its buffers
    const double dr = -shift_y / res_y, dc = shift_x / res_x;
    const NkGeom g = geom_of(P, dr, dc);
    {
        // Direction-agnostic on purpose: every rank of a partitioned fit must take the same decision (a rank that raised
        // while its neighbours entered the next all-reduce would dead-lock the group), and all interior block borders
        // carry the same halo depth.
        // rules 0 / 1 read the four bilinear taps (rows floor(r + dr), + 1); rules 2 / 3 look one row around the NEAREST pixel,
        // i.e. round(r + dr) +- 1: one more row once the fractional part of |dr| reaches one half
        const int64_t need = (int64_t)floor(fabs(dr)) + (P->nan_rule >= 2 ? 2 : 1);
        const bool top_ok = P->row0 == 0 || P->row0 - P->roff >= need;
        const bool bottom_ok = P->row1 == P->H || P->roff + P->nbuf - P->row1 >= need;
        if (!top_ok || !bottom_ok)
            return xd_fail(ctx, XDEMHIP_EINVAL, "halo too small: the vertical shift moves the bilinear taps outside this rank's row block + halo");
    }
    if (!fit_sums) {   // round 4: one data pass (14 B/pixel) where the plan and the step qualify; anything it cannot prove falls through
        bool done = false;
        const int rc1 = nk_step_onepass<T>(P, g, q0, n, nb, &done, NkStepOut{vshift, n_valid, y_mean, y_std, edges_out, counts, medians});
        if (rc1) return rc1;
        if (done) { ++P->n_onepass; return XDEMHIP_OK; }
    }
    int rc = nk_stage_a<T>(P, g, q0, n, nb);
    if (rc) return rc;
    // stages 3 + 4: y = (dh - vshift) / slope_tan, its bins, the per-bin statistic (vshift and the edges are read from the device)
    std::vector<SelResult<K>> hs;
    bool bins_done = false, bins_passed = false, tail_queued = false, committed = false;
    unsigned char info[32];
    std::vector<T> edges_early(nb + 1);
    double sums_early[2] = {0.0, 0.0};
    double* d_bsum = reinterpret_cast<double*>(base + off_hist(nb));
    unsigned long long* d_bcnt = reinterpret_cast<unsigned long long*>(d_bsum + nb);
    double* d_fit = reinterpret_cast<double*>(base + off_hist(1));
    NkYSource<T> src{dh, st, asp, d_vshift, d_edges, d_sums, nullptr, 0.0, (T)0,
                     P->custom_edges.empty() ? NK_AUTO_EDGES : P->custom_decimal};
    BinCacheRec* d_rec = reinterpret_cast<BinCacheRec*>(base + OFF_INFO + 64);
    if (!fit_sums && P->bcache && nb <= NK_BINCACHE_MAX_BINS) {   // (one byte per cached bin id)
        src.bcache = P->bcache + q0;
        src.rec = d_rec;
        hipLaunchKernelGGL((nk_bin_cache_check_kernel<T>), dim3(1), dim3(64), 0, ctx->stream, d_edges, nb, d_rec, (int)P->bcache_force);
        XD_HIP_CHECK(ctx, hipGetLastError());
    }
    XD_HIP_CHECK(ctx, hipMemsetAsync(d_sums, 0, 16, ctx->stream));
    if (fit_sums) {
        XD_HIP_CHECK(ctx, hipMemsetAsync(d_fit, 0, 80, ctx->stream));
        if (n > 0) {
            hipLaunchKernelGGL((nk_fit_sums_kernel<T>), dim3(grid_for(ctx, n, 256, 16)), dim3(256), 0, ctx->stream, dh, st, asp, n, d_vshift,
                               d_fit);
            XD_HIP_CHECK(ctx, hipGetLastError());
        }
        rc = xd_allreduce_device(ctx, d_fit, 10, XDEMHIP_RED_SUM_F64);
        if (rc) return rc;
    } else if (P->bin_stat == XDEMHIP_BINSTAT_MEAN) {
        // bin_statistic = np.nanmean: one pass, per-bin float64 sums and counts (and the two global sums)
        if (nb > 3072) return xd_fail(ctx, XDEMHIP_EINVAL, "n_bins too large for the mean statistic");
        rc = run_bin_sums<T, NkYSource<T>>(ctx, src, n, nb, d_bsum, d_bcnt);
        if (rc) return rc;
        if (src.bcache) {  // the pass visited every own pixel: the cache now holds the bins of these edges
            hipLaunchKernelGGL((nk_bin_cache_commit_kernel<T>), dim3(1), dim3(64), 0, ctx->stream, d_edges, nb, d_rec);
            P->bcache_force = false;
        }
    } else {
        // per-bin exact medians, bracketed route: y and the bin ids are computed on the fly by the sample / counting
        // passes (NkYSource), the counting pass accumulates the sums
        // On a single GPU everything this step still has to hand back -- the cache commit, vshift / counts / flags, the edges
        // and the two sums -- is queued behind the route BEFORE its one synchronisation (three host round trips of ~50 us
        // otherwise).  With an all-reduce hook the sums need their reduction first: the separate copies below remain.
        const std::function<int()> tail = [&]() -> int {
            if (ctx->allreduce) return XDEMHIP_OK;
            if (src.bcache) {
                hipLaunchKernelGGL((nk_bin_cache_commit_kernel<T>), dim3(1), dim3(64), 0, ctx->stream, d_edges, nb, d_rec);
                XD_HIP_CHECK(ctx, hipGetLastError());
                P->bcache_force = false;
                committed = true;
            }
            { const int rc_ = xd_d2h(ctx, info, base + OFF_INFO, 32); if (rc_) return rc_; }
            { const int rc_ = xd_d2h(ctx, edges_early.data(), d_edges, sizeof(T) * (nb + 1)); if (rc_) return rc_; }
            { const int rc_ = xd_d2h(ctx, sums_early, d_sums, 16); if (rc_) return rc_; }
            tail_queued = true;
            return XDEMHIP_OK;
        };
        rc = run_select_bracketed<T, NkYSource<T>>(ctx, src, n, nb, base, hs, &P->ws, &bins_done, &bins_passed, &tail);
        if (rc) return rc;
        if (src.bcache && !committed) {
            // the counting pass ran over every own pixel (whether or not its brackets held): the cache is filled; a route
            // that never launched it leaves the record untouched and the cache marked stale
            if (bins_passed) {
                hipLaunchKernelGGL((nk_bin_cache_commit_kernel<T>), dim3(1), dim3(64), 0, ctx->stream, d_edges, nb, d_rec);
                P->bcache_force = false;
            } else {
                P->bcache_force = true;
            }
        }
    }
    if (!tail_queued) {
        { const int rc_ = xd_d2h(ctx, info, base + OFF_INFO, 32); if (rc_) return rc_; }
        { const int rc_ = xd_sync(ctx); if (rc_) return rc_; }
    }
    uint64_t total;
    double vs;
    memcpy(&total, info + 8, 8);
    memcpy(&vs, info + 24, 8);
    ++P->n_plain;
    *n_valid = (int64_t)total;
    if (total == 0) return xd_fail(ctx, XDEMHIP_EINVAL, "The subsample contains no more valid values.");
    *vshift = vs;
    if (!fit_sums && P->bin_stat == XDEMHIP_BINSTAT_MEDIAN && !bins_done) {
        // small grids, plain mode, a missed bracket: y and bin-id arrays + plain digit passes
        XD_HIP_CHECK(ctx, hipMemsetAsync(d_sums, 0, 16, ctx->stream));
        if (n > 0) {
            // (the two sums seed curve_fit: added in a fixed order, so that a fit repeats its bits -- per-workgroup partials in the slots
            //  of the one-pass step, which this route never runs beside)
            const int n_wg = grid_for(ctx, n, 256, 16);
            const size_t slots = ((size_t)n_wg * 2 + 4) / 5;   // (the capacity counts rows of five doubles)
            if (slots > P->wg_sums_cap) {
                P->wg_sums_cap = P->mem.regrow(P->wg_sums, slots * 5 * sizeof(double), "per-workgroup sums of the y pass") ? slots : 0;
                { const int rc_ = P->mem.status(); if (rc_) return rc_; }
            }
            hipLaunchKernelGGL((nk_y_kernel<T>), dim3(n_wg), dim3(256), sizeof(T) * (nb + 1), ctx->stream, dh, st, asp, n,
                               (T)vs, d_edges, nb, y, bins, d_sums, P->custom_edges.empty() ? NK_AUTO_EDGES : P->custom_decimal, P->wg_sums);
            hipLaunchKernelGGL(nk_y_sums_kernel, dim3(1), dim3(256), 0, ctx->stream, P->wg_sums, n_wg, d_sums);
            XD_HIP_CHECK(ctx, hipGetLastError());
        }
        rc = run_select_core<T>(ctx, y, bins, n, nb, base, hs, SEL_MEDIAN, nullptr);
        if (rc) return rc;
    }
    const double cnt = (double)total;
    if (tail_queued && bins_done) {
        // everything arrived with the route's own synchronisation
        const double mean = sums_early[0] / cnt;
        const double var = sums_early[1] / cnt - mean * mean;
        *y_mean = mean;
        *y_std = var > 0 ? sqrt(var) : 0.0;
        for (int k = 0; k < nb; ++k) {
            counts[k] = (int64_t)hs[k].st.count;
            medians[k] = median_from<T>(hs[k]);
        }
        for (int k = 0; k <= nb; ++k) edges_out[k] = (double)edges_early[k];
        return XDEMHIP_OK;
    }
    std::vector<T> edges(nb + 1);
    { const int rc_ = xd_d2h(ctx, edges.data(), d_edges, sizeof(T) * (nb + 1)); if (rc_) return rc_; }
    if (fit_sums) {
        { const int rc_ = xd_d2h(ctx, fit_sums, d_fit, 80); if (rc_) return rc_; }
        { const int rc_ = xd_sync(ctx); if (rc_) return rc_; }
        const double mean = fit_sums[6] / cnt;
        const double var = fit_sums[9] / cnt - mean * mean;
        *y_mean = mean;
        *y_std = var > 0 ? sqrt(var) : 0.0;
        return XDEMHIP_OK;
    }
    rc = xd_allreduce_device(ctx, d_sums, 2, XDEMHIP_RED_SUM_F64);
    if (rc) return rc;
    double sums[2];
    { const int rc_ = xd_d2h(ctx, sums, d_sums, 16); if (rc_) return rc_; }
    std::vector<double> bs(nb);
    std::vector<unsigned long long> bc(nb);
    if (P->bin_stat == XDEMHIP_BINSTAT_MEAN) {
        { const int rc_ = xd_d2h(ctx, bs.data(), d_bsum, 8 * (size_t)nb); if (rc_) return rc_; }
        { const int rc_ = xd_d2h(ctx, bc.data(), d_bcnt, 8 * (size_t)nb); if (rc_) return rc_; }
    }
    { const int rc_ = xd_sync(ctx); if (rc_) return rc_; }
    const double mean = sums[0] / cnt;
    const double var = sums[1] / cnt - mean * mean;
    *y_mean = mean;
    *y_std = var > 0 ? sqrt(var) : 0.0;
    for (int k = 0; k < nb; ++k) {
        if (P->bin_stat == XDEMHIP_BINSTAT_MEAN) {
            counts[k] = (int64_t)bc[k];
            medians[k] = bc[k] ? (double)(T)(bs[k] / (double)bc[k]) : NAN;  // np.nanmean returns the sample dtype
        } else {
            counts[k] = (int64_t)hs[k].st.count;
            medians[k] = median_from<T>(hs[k]);
        }
    }
    for (int k = 0; k <= nb; ++k) edges_out[k] = (double)edges[k];
    return XDEMHIP_OK;
}

// NuthKaab(bin_statistic=<any callable>) (xdem/coreg/affine.py:2404 -> nd_binning -> scipy.stats.binned_statistic with the callable):
// a Python callable cannot run here, so the step hands back what it would be called on -- y = (dh - vshift) / slope_tan and the aspect-bin
// id of every pixel of the plan's rows, in raster order (NaN / 0xFFFF where the pixel has no dh) -- next to vshift, the valid count, the
// moments of y and the bin edges.  Plain route (stored dh); whole-raster plans only: a callable needs all of a bin's values in one place.
template <typename T>
int nk_step_values(xdemhip_nk_plan* P, double shift_x, double shift_y, double res_x, double res_y, int nb, double* vshift, int64_t* n_valid,
                   double* y_mean, double* y_std, double* edges_out, void* y_out, uint16_t* bins_out, int memspace) {
    xdemhip_ctx* ctx = P->ctx;
    if (ctx->allreduce) return xd_fail(ctx, XDEMHIP_EINVAL, "per-pixel values of a step: whole-raster plans only (a partitioned plan holds a part of every bin)");
    if (P->row0 != 0 || P->row1 != P->H || P->roff != 0) return xd_fail(ctx, XDEMHIP_EINVAL, "per-pixel values of a step: the plan must cover the whole raster");
    const int64_t n = P->H * P->W;
    unsigned char* base = static_cast<unsigned char*>(P->scratch);
    double* d_sums = reinterpret_cast<double*>(base + OFF_SUMS);
    T* d_edges = reinterpret_cast<T*>(base);
    if (!P->custom_edges.empty()) nb = (int)P->custom_edges.size() - 1;
    const NkGeom g = geom_of(P, -shift_y / res_y, shift_x / res_x);
    int rc = nk_stage_a<T>(P, g, 0, n, nb);
    if (rc) return rc;
    unsigned char info[32];
    { const int rc_ = xd_d2h(ctx, info, base + OFF_INFO, 32); if (rc_) return rc_; }
    { const int rc_ = xd_sync(ctx); if (rc_) return rc_; }
    uint64_t total;
    double vs;
    memcpy(&total, info + 8, 8);
    memcpy(&vs, info + 24, 8);
    ++P->n_plain;
    *n_valid = (int64_t)total;
    if (total == 0) return xd_fail(ctx, XDEMHIP_EINVAL, "The subsample contains no more valid values.");
    *vshift = vs;
    XD_HIP_CHECK(ctx, hipMemsetAsync(d_sums, 0, 16, ctx->stream));
    hipLaunchKernelGGL((nk_y_kernel<T>), dim3(grid_for(ctx, n, 256, 16)), dim3(256), sizeof(T) * (nb + 1), ctx->stream, static_cast<const T*>(P->dh),
                       static_cast<const T*>(P->slope_tan), static_cast<const T*>(P->aspect), n, (T)vs, d_edges, nb, static_cast<T*>(P->y), P->bins,
                       d_sums, P->custom_edges.empty() ? NK_AUTO_EDGES : P->custom_decimal);
    XD_HIP_CHECK(ctx, hipGetLastError());
    P->bcache_force = true;   // (nothing here maintains the bin cache of the other routes)
    std::vector<T> edges(nb + 1);
    double sums[2];
    { const int rc_ = xd_d2h(ctx, edges.data(), d_edges, sizeof(T) * (nb + 1)); if (rc_) return rc_; }
    { const int rc_ = xd_d2h(ctx, sums, d_sums, 16); if (rc_) return rc_; }
    const hipMemcpyKind kind = memspace == XDEMHIP_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    XD_HIP_CHECK(ctx, hipMemcpyAsync(y_out, P->y, (size_t)n * sizeof(T), kind, ctx->stream));
    XD_HIP_CHECK(ctx, hipMemcpyAsync(bins_out, P->bins, (size_t)n * 2, kind, ctx->stream));
    { const int rc_ = xd_sync(ctx); if (rc_) return rc_; }
    const double cnt = (double)total, mean = sums[0] / cnt, var = sums[1] / cnt - mean * mean;
    *y_mean = mean;
    *y_std = var > 0 ? sqrt(var) : 0.0;
    for (int k = 0; k <= nb; ++k) edges_out[k] = (double)edges[k];
    return XDEMHIP_OK;
}

// The device side of xdemhip_binned_median: the m finite (x, y) pairs binned on SciPy's edges over [smin, smax], one median per bin.
template <typename T>
int binned_median_typed(xdemhip_ctx* ctx, const void* xs, const void* ys, int64_t m, double smin, double smax, int n_bins, double* edges,
                        int64_t* counts, double* medians) {
    std::vector<T> e;   // (sources of copies queued on the stream: declared before the buffers)
    make_edges<T>(smin, smax, n_bins, e);
    const std::vector<T> ones((size_t)m, (T)1);
    XdBuffers buf(ctx, "xdemhip_binned_median");
    const T* d_x = static_cast<const T*>(buf.input(xs, (size_t)m * sizeof(T), XDEMHIP_HOST));
    const T* d_y = static_cast<const T*>(buf.input(ys, (size_t)m * sizeof(T), XDEMHIP_HOST));
    const T* d_one = buf.input(ones.data(), (size_t)m * sizeof(T), XDEMHIP_HOST);
    T* d_yb = buf.alloc<T>((size_t)m);
    uint16_t* d_bins = buf.alloc<uint16_t>((size_t)m);
    unsigned char* base = buf.alloc<unsigned char>(scratch_size(n_bins));
    if (buf.rc) return buf.rc;
    double* d_sums = reinterpret_cast<double*>(base + OFF_SUMS);
    XD_HIP_CHECK(ctx, hipMemsetAsync(d_sums, 0, 16, ctx->stream));
    XD_HIP_CHECK(ctx, hipMemcpyAsync(base, e.data(), sizeof(T) * (n_bins + 1), hipMemcpyHostToDevice, ctx->stream));
    // reuse nk_y_kernel with vshift = 0 and slope_tan = 1: y passes through unchanged ((y - 0) / 1 is exact)
    hipLaunchKernelGGL((nk_y_kernel<T>), dim3(grid_for(ctx, m, 256, 16)), dim3(256), sizeof(T) * (n_bins + 1), ctx->stream, d_y, d_one, d_x, m, (T)0,
                       reinterpret_cast<const T*>(base), n_bins, d_yb, d_bins, d_sums);
    std::vector<SelResult<typename KeyT<T>::type>> hs;
    XdLocalSelection local(ctx);   // (a purely local helper)
    const int rc = run_select<T>(ctx, d_yb, d_bins, m, n_bins, base, hs);
    if (rc) return rc;
    for (int k = 0; k < n_bins; ++k) { counts[k] = (int64_t)hs[k].st.count; medians[k] = median_from<T>(hs[k]); }
    for (int k = 0; k <= n_bins; ++k) edges[k] = (double)e[k];
    return buf.finish();
}

// Shared by the two creation entry points.  Buffers hold raster rows [roff, roff + nbuf); own rows [row0, row1).
int nk_create_impl(xdemhip_ctx* ctx, const void* ref, const void* tba, const uint8_t* inlier, int dtype, int64_t H, int64_t W,
                   int64_t roff, int64_t nbuf, int64_t row0, int64_t row1, int memspace, bool global_count,
                   xdemhip_nk_plan** out_plan, int64_t* n_valid) {
    if (!ctx) return XDEMHIP_EINVAL;
    if (!ref || !tba || !out_plan) return xd_fail(ctx, XDEMHIP_EINVAL, "null argument");
    if (H < 2 || W < 2) return xd_fail(ctx, XDEMHIP_EINVAL, "Shape of array too small to calculate a numerical gradient, at least 2 elements are required.");
    if (dtype != XDEMHIP_F32 && dtype != XDEMHIP_F64) return xd_fail(ctx, XDEMHIP_EINVAL, "dtype must be float32 or float64");
    XD_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    const size_t es = dtype == XDEMHIP_F32 ? 4 : 8;
    const size_t n = (size_t)nbuf * (size_t)W;
    xdemhip_nk_plan* P = new xdemhip_nk_plan();
    P->ctx = P->mem.ctx = ctx; P->dtype = dtype; P->H = H; P->W = W; P->roff = roff; P->nbuf = nbuf; P->row0 = row0; P->row1 = row1;
    P->nan_rule = ctx->nk_nan_rule;
    auto fail = [&](int code) { delete P; return code; };
    const char* who = "xdemhip_nk_create";
    XdOwned& mem = P->mem;
    P->ref = mem.keep(ref, n * es, memspace, who);
    P->tba = mem.keep(tba, n * es, memspace, who);
    P->inlier = mem.keep(inlier, n, memspace, who);
    P->max_bins = 1024;
    P->scratch_bytes = scratch_size(P->max_bins);
    P->slope_tan = mem.take(n * es, who);
    P->aspect = mem.take(n * es, who);
    P->dh = mem.take(n * es, who);
    P->y = mem.take(n * es, who);
    P->valid = mem.take<uint8_t>(n, who);
    P->bins = mem.take<uint16_t>(n, who);
    P->bcache = mem.take<nk_bin_t>(n, who);
    P->scratch = mem.take(P->scratch_bytes, who);
    if (mem.rc) return fail(mem.rc);
    if ((int64_t)n >= SEL_BRACKET_MIN_N && sel_ws_create(mem, (int64_t)n, es, MAX_BINS_PER_SWEEP, P->ws) != XDEMHIP_OK) return fail(XDEMHIP_ENOMEM);
    // EXT buffers of the one-pass step (large plans): masked copy of the reference DEM + the lists of extreme-aspect pixels;
    // without the memory for them the plan simply keeps the plain route, which reads mask and aspect
    if ((int64_t)n >= SEL_BRACKET_MIN_N && ctx->nk_fused != 0) {
        mem.optional();
        P->ref_m = mem.take(n * es, who);
        P->ext_idx = mem.take<int64_t>((size_t)2 * EXT_CAP, who);
        P->ext_cnt = mem.take<unsigned long long>(4, who);
        (void)mem.all_or_none(P->ref_m, P->ext_idx, P->ext_cnt);
    }
    // one-pass step (large single-GPU plans with the EXT buffers): its device block and candidate buffers; without the memory the
    // plan keeps the plain route
    if (P->ref_m && P->ws.d_small && ctx->nk_fused != 0) {
        // (the device block and the packed results: sized by what the step indexes them with -- nk_layout.h, NkStepResults::table)
        P->cd_cap = (int64_t)n / 8 + 4096;
        P->fz_pack_bytes = dtype == XDEMHIP_F32 ? nk_fetch_bytes<float, uint32_t, SelState<uint32_t>>(P->ws.nb_max)
                                                : nk_fetch_bytes<double, uint64_t, SelState<uint64_t>>(P->ws.nb_max);
        mem.optional();
        P->fz = static_cast<uint64_t*>(mem.take(NkFzWords::total_bytes(P->ws.nb_max), who));
        P->cd_vals = mem.take((size_t)P->cd_cap * es, who);
        P->c_st = mem.take((size_t)P->ws.c_cap * es, who);
        P->fz_pack = mem.take<unsigned char>(P->fz_pack_bytes, who);
        (void)mem.all_or_none(P->fz, P->cd_vals, P->c_st, P->fz_pack);
    }
    // rules 2 / 3 on plans large enough for the streaming kernels (whole rasters and row blocks alike): the per-pixel neighbourhood
    // flags of the tba buffer, once
    if (P->nan_rule >= 2 && (int64_t)n >= SEL_BRACKET_MIN_N) {
        P->bad_wpr = (W + 63) / 64 + 2;
        mem.optional();
        P->badbits = mem.take<uint64_t>((size_t)P->bad_wpr * (size_t)nbuf, who);
        if (mem.all_or_none(P->badbits)) {   // (without them the plan keeps the generic kernels)
            const dim3 bgrid((unsigned)((P->bad_wpr - 2 + 3) / 4), (unsigned)(nbuf < 4096 ? nbuf : 4096));
            if (dtype == XDEMHIP_F32)
                hipLaunchKernelGGL((nk_badbits_kernel<float>), bgrid, dim3(256), 0, ctx->stream, static_cast<const float*>(P->tba), H, W, roff, nbuf, P->nan_rule, P->bad_wpr, P->badbits);
            else
                hipLaunchKernelGGL((nk_badbits_kernel<double>), bgrid, dim3(256), 0, ctx->stream, static_cast<const double*>(P->tba), H, W, roff, nbuf, P->nan_rule, P->bad_wpr, P->badbits);
            if (launched(ctx, "nk_badbits_kernel")) return fail(XDEMHIP_EHIP);
        }
    }
    int rc;
    {
        std::optional<XdLocalSelection> local;   // whole-raster plan: local pass; xdemhip_nk_set_rows re-partitions with the hook
        if (!global_count) local.emplace(ctx);
        rc = dtype == XDEMHIP_F32 ? nk_aux_typed<float>(P) : nk_aux_typed<double>(P);
    }
    if (rc != XDEMHIP_OK) return fail(rc);
    if (n_valid) *n_valid = P->n_valid0;
    *out_plan = P;
    return XDEMHIP_OK;
}

// What the three step entry points share.  The message texts and the order in which each entry point checks its arguments are part
// of the interface.
static int nk_check_bins(xdemhip_nk_plan* P, int n_bins) {
    if (n_bins < 1 || n_bins > P->max_bins) return xd_fail(P->ctx, XDEMHIP_EINVAL, "n_bins out of range (1..1024)");
    // explicit edges fix the number of bins: the caller's output arrays are sized by ITS n_bins, so the two must agree
    if (!P->custom_edges.empty() && n_bins != (int)P->custom_edges.size() - 1)
        return xd_fail(P->ctx, XDEMHIP_EINVAL, "n_bins must equal the number of explicit bin edges - 1 (xdemhip_nk_set_bin_edges)");
    return XDEMHIP_OK;
}
static int nk_check_resolution(xdemhip_ctx* ctx, double res_x, double res_y) {
    if (!(res_x > 0) || !(res_y > 0)) return xd_fail(ctx, XDEMHIP_EINVAL, "resolution must be > 0");
    return XDEMHIP_OK;
}
// the step itself between the context's two timing events; `typed(tag)` runs it for the sample type of `tag`
template <typename F> static int nk_timed_step(xdemhip_nk_plan* P, F&& typed) {
    xdemhip_ctx* ctx = P->ctx;
    XD_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    XD_HIP_CHECK(ctx, hipEventRecord(ctx->ev_start, ctx->stream));
    const int rc = P->dtype == XDEMHIP_F32 ? typed(float()) : typed(double());
    (void)hipEventRecord(ctx->ev_stop, ctx->stream);
    ctx->timed = (rc == XDEMHIP_OK);
    return rc;
}

}  // namespace

extern "C" {

void xdemhip_nk_destroy(xdemhip_nk_plan* P) { delete P; }   // (its owner frees the device buffers)

int xdemhip_nk_create(xdemhip_ctx* ctx, const void* ref, const void* tba, const uint8_t* inlier, int dtype, int64_t H, int64_t W,
                      int memspace, xdemhip_nk_plan** out_plan, int64_t* n_valid) {
    XdFetchScope fetch_scope_(ctx);
    return nk_create_impl(ctx, ref, tba, inlier, dtype, H, W, 0, H, 0, H, memspace, false, out_plan, n_valid);
}

int xdemhip_nk_create_block(xdemhip_ctx* ctx, const void* ref_block, const void* tba_block, const uint8_t* inlier_block, int dtype,
                            int64_t H, int64_t W, int64_t row_begin, int64_t row_end, int64_t halo_top, int64_t halo_bottom,
                            int memspace, xdemhip_nk_plan** out_plan, int64_t* n_valid) {
    XdFetchScope fetch_scope_(ctx);
    if (!ctx) return XDEMHIP_EINVAL;
    if (row_begin < 0 || row_end < row_begin || row_end > H || halo_top < 0 || halo_bottom < 0 || halo_top > row_begin ||
        row_end + halo_bottom > H)
        return xd_fail(ctx, XDEMHIP_EINVAL, "bad row block");
    // np.gradient reads one neighbour row on each side of an own row: a block that does not start / end at the raster's
    // border needs at least one halo row there
    if ((row_begin > 0 && halo_top < 1) || (row_end < H && halo_bottom < 1))
        return xd_fail(ctx, XDEMHIP_EINVAL, "a row block inside the raster needs >= 1 halo row towards each neighbour");
    return nk_create_impl(ctx, ref_block, tba_block, inlier_block, dtype, H, W, row_begin - halo_top, (row_end - row_begin) + halo_top + halo_bottom,
                          row_begin, row_end, memspace, true, out_plan, n_valid);
}

int xdemhip_nk_set_rows(xdemhip_nk_plan* P, int64_t row_begin, int64_t row_end, int64_t* n_valid) {
    XdFetchScope fetch_scope_(P ? P->ctx : nullptr);
    if (!P) return XDEMHIP_EINVAL;
    xdemhip_ctx* ctx = P->ctx;
    if (row_begin < P->roff || row_end < row_begin || row_end > P->roff + P->nbuf) return xd_fail(ctx, XDEMHIP_EINVAL, "bad row range");
    XD_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    P->row0 = row_begin;
    P->row1 = row_end;
    P->bcache_force = true;  // other own rows: their bins were never cached
    P->pred.forget();        // ... and their medians are not the previous step's
    // valid mask / aux rasters outside the range are never read by this rank; recount the global number of valid pixels
    int rc = P->dtype == XDEMHIP_F32 ? nk_aux_typed<float>(P) : nk_aux_typed<double>(P);
    if (rc) return rc;
    if (n_valid) *n_valid = P->n_valid0;
    return XDEMHIP_OK;
}

int xdemhip_nk_subsample(xdemhip_nk_plan* P, const int64_t* ranks, int64_t k, int memspace, int64_t* n_valid) {
    XdFetchScope fetch_scope_(P ? P->ctx : nullptr);
    if (!P) return XDEMHIP_EINVAL;
    xdemhip_ctx* ctx = P->ctx;
    if (ctx->allreduce || P->row0 != 0 || P->row1 != P->H || P->roff != 0 || P->nbuf != P->H)
        return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_nk_subsample: whole-raster plans of one process only (partitioned plans: pass the drawn mask as inlier mask)");
    if (!ranks || k < 1 || k > P->n_valid0) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_nk_subsample: 1 <= k <= the plan's valid pixels");
    XD_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    const int64_t n = P->H * P->W, n_tiles = (n + RANK_TILE - 1) / RANK_TILE;
    if (n_tiles > 0x7FFFFFFF) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_nk_subsample: raster too large");
    if (!P->sub_inlier) P->sub_inlier = P->mem.take<uint8_t>((size_t)n, "xdemhip_nk_subsample");
    { const int rc_ = P->mem.status(); if (rc_) return rc_; }
    RankSelect rs(ctx, "xdemhip_nk_subsample");
    unsigned long long total = 0, bad = 0;
    { const int rc_ = rs.run(ranks, k, memspace, P->n_valid0, P->valid, n, nullptr, &total, &bad); if (rc_) return rc_; }
    if ((long long)total != P->n_valid0) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_nk_subsample: the valid mask changed under the call");
    if (bad != 0) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_nk_subsample: a rank is outside [0, n_valid)");
    hipLaunchKernelGGL((rank_select_kernel<RankOut::Mask>), dim3((unsigned)n_tiles), dim3(256), 0, ctx->stream, P->valid, n, rs.off, rs.mark,
                       (unsigned long long*)nullptr, (int64_t*)nullptr, P->sub_inlier);
    if (hipGetLastError() != hipSuccess) return xd_fail(ctx, XDEMHIP_EHIP, "xdemhip_nk_subsample: kernel launch failed");
    P->inlier = P->sub_inlier;   // (an owned copy of the mask the plan was created with stays with the owner)
    // (as after xdemhip_nk_set_rows: other valid pixels -- no cached bins, no previous medians, no measured sample offsets)
    P->bcache_force = true;
    P->pred.forget();
    P->narrowing.reset();
    const int rc = P->dtype == XDEMHIP_F32 ? nk_aux_typed<float>(P) : nk_aux_typed<double>(P);
    if (rc) return rc;
    if (n_valid) *n_valid = P->n_valid0;
    return XDEMHIP_OK;
}

int xdemhip_nk_predict_counts(xdemhip_nk_plan* P, int64_t* predicted, int64_t* predicted_dh_only, int64_t* missed) {
    if (!P) return XDEMHIP_EINVAL;
    if (predicted) *predicted = P->pred.n_predicted;
    if (predicted_dh_only) *predicted_dh_only = P->pred.n_predicted_d;
    if (missed) *missed = P->pred.n_predict_miss;
    return XDEMHIP_OK;
}

int xdemhip_nk_route_counts(xdemhip_nk_plan* P, int64_t* onepass, int64_t* plain) {
    if (!P) return XDEMHIP_EINVAL;
    if (onepass) *onepass = P->n_onepass;
    if (plain) *plain = P->n_plain;
    return XDEMHIP_OK;
}

int xdemhip_nk_set_statistic(xdemhip_nk_plan* P, int bin_stat) {
    if (!P) return XDEMHIP_EINVAL;
    if (bin_stat != XDEMHIP_BINSTAT_MEDIAN && bin_stat != XDEMHIP_BINSTAT_MEAN) return xd_fail(P->ctx, XDEMHIP_EINVAL, "bin statistic: 0 median, 1 mean");
    P->bin_stat = bin_stat;
    return XDEMHIP_OK;
}

int xdemhip_nk_get_aux(xdemhip_nk_plan* P, void* slope_tan, void* aspect, uint8_t* valid) {
    if (!P) return XDEMHIP_EINVAL;
    xdemhip_ctx* ctx = P->ctx;
    XD_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    { const int rc_ = xd_sync(ctx); if (rc_) return rc_; }
    const size_t es = P->dtype == XDEMHIP_F32 ? 4 : 8, n = (size_t)P->nbuf * (size_t)P->W;  // (the plan's buffer rows)
    if (slope_tan) XD_HIP_CHECK(ctx, hipMemcpy(slope_tan, P->slope_tan, n * es, hipMemcpyDeviceToHost));
    if (aspect) XD_HIP_CHECK(ctx, hipMemcpy(aspect, P->aspect, n * es, hipMemcpyDeviceToHost));
    if (valid) XD_HIP_CHECK(ctx, hipMemcpy(valid, P->valid, n, hipMemcpyDeviceToHost));
    return XDEMHIP_OK;
}

int xdemhip_nk_step(xdemhip_nk_plan* P, double shift_x, double shift_y, double res_x, double res_y, int n_bins, double* vshift,
                    int64_t* n_valid, double* y_mean, double* y_std, double* edges, int64_t* counts, double* medians) {
    XdFetchScope fetch_scope_(P ? P->ctx : nullptr);
    if (!P) return XDEMHIP_EINVAL;
    xdemhip_ctx* ctx = P->ctx;
    if (!vshift || !n_valid || !y_mean || !y_std || !edges || !counts || !medians) return xd_fail(ctx, XDEMHIP_EINVAL, "null output");
    { const int rc_ = nk_check_bins(P, n_bins); if (rc_) return rc_; }
    { const int rc_ = nk_check_resolution(ctx, res_x, res_y); if (rc_) return rc_; }
    return nk_timed_step(P, [&](auto tag) {
        return nk_step_typed<decltype(tag)>(P, shift_x, shift_y, res_x, res_y, n_bins, vshift, n_valid, y_mean, y_std, edges, counts, medians, nullptr);
    });
}

int xdemhip_nk_step_fit(xdemhip_nk_plan* P, double shift_x, double shift_y, double res_x, double res_y, double* vshift, int64_t* n_valid,
                        double* y_mean, double* y_std, double* sums) {
    XdFetchScope fetch_scope_(P ? P->ctx : nullptr);
    if (!P) return XDEMHIP_EINVAL;
    xdemhip_ctx* ctx = P->ctx;
    if (!vshift || !n_valid || !y_mean || !y_std || !sums) return xd_fail(ctx, XDEMHIP_EINVAL, "null output");
    { const int rc_ = nk_check_resolution(ctx, res_x, res_y); if (rc_) return rc_; }
    return nk_timed_step(P, [&](auto tag) {
        return nk_step_typed<decltype(tag)>(P, shift_x, shift_y, res_x, res_y, 72, vshift, n_valid, y_mean, y_std, nullptr, nullptr, nullptr, sums);
    });
}

int xdemhip_nk_step_values(xdemhip_nk_plan* P, double shift_x, double shift_y, double res_x, double res_y, int n_bins, double* vshift,
                           int64_t* n_valid, double* y_mean, double* y_std, double* edges, void* y_out, uint16_t* bins_out, int memspace) {
    XdFetchScope fetch_scope_(P ? P->ctx : nullptr);
    if (!P) return XDEMHIP_EINVAL;
    xdemhip_ctx* ctx = P->ctx;
    if (!vshift || !n_valid || !y_mean || !y_std || !edges || !y_out || !bins_out) return xd_fail(ctx, XDEMHIP_EINVAL, "null output");
    { const int rc_ = nk_check_resolution(ctx, res_x, res_y); if (rc_) return rc_; }
    if (memspace != XDEMHIP_HOST && memspace != XDEMHIP_DEVICE) return xd_fail(ctx, XDEMHIP_EINVAL, "memspace must be XDEMHIP_HOST or XDEMHIP_DEVICE");
    { const int rc_ = nk_check_bins(P, n_bins); if (rc_) return rc_; }
    return nk_timed_step(P, [&](auto tag) {
        return nk_step_values<decltype(tag)>(P, shift_x, shift_y, res_x, res_y, n_bins, vshift, n_valid, y_mean, y_std, edges, y_out, bins_out, memspace);
    });
}

int xdemhip_nk_set_bin_edges(xdemhip_nk_plan* P, const double* edges, int n_edges, int decimal) {
    if (!P) return XDEMHIP_EINVAL;
    P->bcache_force = true;
    P->pred.forget();
    if (n_edges == 0) { P->custom_edges.clear(); return XDEMHIP_OK; }
    if (!edges || n_edges < 2 || n_edges - 1 > MAX_BINS_PER_SWEEP) return xd_fail(P->ctx, XDEMHIP_EINVAL, "bin edges: 2 .. 129 increasing values");
    for (int k = 1; k < n_edges; ++k)
        if (!(edges[k] > edges[k - 1])) return xd_fail(P->ctx, XDEMHIP_EINVAL, "bin edges must increase strictly");
    P->custom_edges.assign(edges, edges + n_edges);
    P->custom_decimal = decimal;
    return XDEMHIP_OK;
}

// resample a raster shifted by (shift_col, shift_row) pixels (+ dz) back onto its own grid -- the
// translation case of Coreg.apply(resample=True): _reproject_horizontal_shift_samecrs, xdem/coreg/base.py:1615-1655.
int xdemhip_shift_bilinear(xdemhip_ctx* ctx, const void* src, int dtype, int64_t H, int64_t W, double shift_row_px,
                           double shift_col_px, double dz, void* out, int memspace) {
    if (!ctx) return XDEMHIP_EINVAL;
    if (!src || !out || H < 1 || W < 1) return xd_fail(ctx, XDEMHIP_EINVAL, "bad argument");
    if (dtype != XDEMHIP_F32 && dtype != XDEMHIP_F64) return xd_fail(ctx, XDEMHIP_EINVAL, "dtype must be float32 or float64");
    XD_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    const size_t es = dtype == XDEMHIP_F32 ? 4 : 8, bytes = (size_t)H * (size_t)W * es;
    XdPrefault prefault;
    XdBuffers buf(ctx, "xdemhip_shift_bilinear");
    const void* d_src = buf.input(src, bytes, memspace);
    void* d_out = buf.output(out, bytes, memspace);
    if (buf.rc) return buf.rc;
    if (memspace == XDEMHIP_HOST) xd_prefault_start(prefault, out, bytes, ctx->host_copy_threads);   // (the caller's output pages, while the raster travels and the kernel runs)
    const int64_t n = H * W;
    XD_HIP_CHECK(ctx, hipEventRecord(ctx->ev_start, ctx->stream));
    NkGeom g;
    g.H = H; g.W = W; g.roff = 0; g.dr = shift_row_px; g.dc = shift_col_px; g.rule = ctx->nk_nan_rule;
    if (dtype == XDEMHIP_F32)
        hipLaunchKernelGGL((shift_bilinear_kernel<float>), dim3(grid_for(ctx, n, 256, 16)), dim3(256), 0, ctx->stream,
                           static_cast<const float*>(d_src), g, (float)dz, static_cast<float*>(d_out));
    else
        hipLaunchKernelGGL((shift_bilinear_kernel<double>), dim3(grid_for(ctx, n, 256, 16)), dim3(256), 0, ctx->stream,
                           static_cast<const double*>(d_src), g, dz, static_cast<double*>(d_out));
    (void)hipEventRecord(ctx->ev_stop, ctx->stream);
    ctx->timed = true;
    const int rc = launched(ctx, "shift kernel");
    prefault.join();
    return rc ? rc : buf.finish();
}

// Stand-alone binned nanmedian: binned_statistic(x, y, np.nanmedian, n_bins) + counts on SciPy's edges.
// (xdem/spatialstats.py:143-157 for one explanatory variable).  Non-finite (x, y) pairs are dropped like nd_binning does.
int xdemhip_binned_median(xdemhip_ctx* ctx, const void* x, const void* y, int dtype, int64_t n, int n_bins, double* edges,
                          int64_t* counts, double* medians) {
    XdFetchScope fetch_scope_(ctx);
    if (!ctx) return XDEMHIP_EINVAL;
    if (!x || !y || !edges || !counts || !medians || n <= 0) return xd_fail(ctx, XDEMHIP_EINVAL, "bad argument");
    if (n_bins < 1 || n_bins > 1024) return xd_fail(ctx, XDEMHIP_EINVAL, "n_bins out of range (1..1024)");
    if (dtype != XDEMHIP_F32 && dtype != XDEMHIP_F64) return xd_fail(ctx, XDEMHIP_EINVAL, "dtype must be float32 or float64");
    XD_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    const size_t es = dtype == XDEMHIP_F32 ? 4 : 8;
    // finite filter + min / max on the host, like nd_binning (O(n); this helper is not a hot path)
    double smin = INFINITY, smax = -INFINITY;
    std::vector<unsigned char> xs((size_t)n * es), ys((size_t)n * es);
    int64_t m = 0;
    for (int64_t i = 0; i < n; ++i) {
        double xv, yv;
        if (dtype == XDEMHIP_F32) { xv = static_cast<const float*>(x)[i]; yv = static_cast<const float*>(y)[i]; }
        else { xv = static_cast<const double*>(x)[i]; yv = static_cast<const double*>(y)[i]; }
        if (!std::isfinite(xv) || !std::isfinite(yv)) continue;
        memcpy(&xs[(size_t)m * es], static_cast<const unsigned char*>(x) + (size_t)i * es, es);
        memcpy(&ys[(size_t)m * es], static_cast<const unsigned char*>(y) + (size_t)i * es, es);
        smin = xv < smin ? xv : smin;
        smax = xv > smax ? xv : smax;
        ++m;
    }
    if (m == 0) { for (int k = 0; k < n_bins; ++k) { counts[k] = 0; medians[k] = NAN; } return XDEMHIP_OK; }
    return dtype == XDEMHIP_F32 ? binned_median_typed<float>(ctx, xs.data(), ys.data(), m, smin, smax, n_bins, edges, counts, medians)
                                : binned_median_typed<double>(ctx, xs.data(), ys.data(), m, smin, smax, n_bins, edges, counts, medians);
}

}  // extern "C"
