// blockwise.hip -- xdem.coreg.BlockwiseCoreg (xdem/coreg/blockwise.py) on gfx950: the Nuth-Kaab step of EVERY tile of a tiling in a fixed
// number of launches, and the warp of `apply` in one pass.
//
// A plan copies the two rasters into TILE-MAJOR buffers: tile t is a contiguous h x w raster at tiles[t].off.  Every tile is then an
// independent raster to the device functions the whole-raster plan uses (nk_aux_pixel, NkGeom / bi_locate / bi_value, aspect_bin,
// make_edges_into): the gradient is one-sided on the tile's borders and no tap or neighbourhood leaves the tile, by construction.
// One step (xdemhip_bw_nk_step), seven launches whatever the number of tiles; a phase that reads what other workgroups wrote is a
// launch of its own:
//   1 bw_init_kernel     per active tile: min / max aspect keys, counts
//   2 bw_dh_kernel       dh = ref - bilinear(tba) at the tile's own shift; min / max aspect key and count of the finite dh (integer atomics)
//   3 bw_vshift_kernel   one workgroup per tile: exact nanmedian of dh (radix selection over the tile's slice), SciPy's bin edges
//   4 bw_y_kernel        y = (dh - vshift) / slope_tan, aspect bin, (tile, bin) counts
//   5 bw_scan_kernel     one workgroup per tile: segment offsets; mean and standard deviation of y, summed in a fixed order
//   6 bw_scatter_kernel  y into (tile, bin) segments (the order inside a segment depends on scheduling; only order statistics are taken)
//   7 bw_segment_kernel  one workgroup per (tile, bin): exact median by a sort in LDS, or by radix selection for a long segment
// and one device-to-host copy of the results.  FOR -ffp-contract=off (the Makefile lists this file).
#include <math.h>
#include <string.h>

#include <vector>

#include "common.h"
#include "select.h"
#include "select_run.h"
#include "nk_aux.h"
#include "nk_geom.h"
#include "bi_point.h"
#include "volume.h"

namespace xd {
namespace {

constexpr int BW_MAX_BINS = 128;     // one byte per bin id, one LDS counter per bin
constexpr int BW_SEG_LDS = 4096;     // keys of a segment sorted in LDS (32 KiB of float64 keys)
constexpr uint8_t BW_NOBIN = 0xFF;

struct BwTile {
    int64_t off;       // first sample of the tile in the tile-major buffers
    int32_t h, w;      // the tile's shape
    int32_t r0, c0;    // its first row / column in the raster
};

// Every per-pixel kernel runs on a grid (blocks, tiles): blockIdx.y is the tile, the workgroups of a row stride over its h * w samples
// (fewer than 2^31).  All lanes of a wave belong to one tile.

template <typename T>
__global__ __launch_bounds__(256) void bw_gather_kernel(const T* __restrict__ ref, const T* __restrict__ tba, int64_t W,
                                                        const BwTile* __restrict__ tiles, T* __restrict__ t_ref, T* __restrict__ t_tba) {
    const BwTile t = tiles[blockIdx.y];
    const uint32_t n = (uint32_t)t.h * (uint32_t)t.w, w = (uint32_t)t.w;
    for (uint32_t p = blockIdx.x * 256u + threadIdx.x; p < n; p += gridDim.x * 256u) {
        const uint32_t i = p / w, j = p - i * w;
        const int64_t src = ((int64_t)t.r0 + i) * W + t.c0 + j;
        t_ref[t.off + p] = ref[src];
        t_tba[t.off + p] = tba[src];
    }
}

template <typename T>
__global__ __launch_bounds__(256) void bw_aux_kernel(const T* __restrict__ t_ref, const T* __restrict__ t_tba, const uint8_t* __restrict__ inlier,
                                                     int64_t W, const BwTile* __restrict__ tiles, T* __restrict__ slope_tan, T* __restrict__ aspect,
                                                     uint8_t* __restrict__ valid, unsigned long long* __restrict__ n_valid) {
    const BwTile t = tiles[blockIdx.y];
    const uint32_t n = (uint32_t)t.h * (uint32_t)t.w, w = (uint32_t)t.w;
    unsigned long long local = 0;
    for (uint32_t p = blockIdx.x * 256u + threadIdx.x; p < n; p += gridDim.x * 256u) {
        const uint32_t i = p / w, j = p - i * w;
        const bool inl = inlier ? inlier[((int64_t)t.r0 + i) * W + t.c0 + j] != 0 : true;
        T st, as;
        const bool ok = nk_aux_pixel<T>(t_ref + t.off, (int64_t)p, (int64_t)i, (int64_t)j, t.h, t.w, t_tba[t.off + p], inl, st, as);
        slope_tan[t.off + p] = st;
        aspect[t.off + p] = as;
        valid[t.off + p] = ok ? 1 : 0;
        local += ok ? 1 : 0;
    }
    for (int off = 32; off > 0; off >>= 1) local += __shfl_down(local, off);
    if ((threadIdx.x & 63) == 0 && local) atomicAdd(&n_valid[blockIdx.y], local);
}

// per active tile: keys[2 t] = all ones (min), keys[2 t + 1] = 0 (max), n_fin[t] = 0, cnt[t][0 .. nb) = 0
__global__ __launch_bounds__(256) void bw_init_kernel(int n_tiles, int nb, const uint8_t* __restrict__ active, unsigned long long* __restrict__ keys,
                                                      unsigned long long* __restrict__ n_fin, unsigned long long* __restrict__ cnt) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= (int64_t)n_tiles * BW_MAX_BINS) return;
    const int t = (int)(k / BW_MAX_BINS), b = (int)(k % BW_MAX_BINS);
    if (!active[t]) return;
    if (b < nb) cnt[k] = 0ull;
    if (b == 0) { keys[2 * t] = ~0ull; keys[2 * t + 1] = 0ull; n_fin[t] = 0ull; }
}

template <typename T>
__global__ __launch_bounds__(256) void bw_dh_kernel(const BwTile* __restrict__ tiles, const uint8_t* __restrict__ active, const double* __restrict__ dr,
                                                    const double* __restrict__ dc, int rule, const T* __restrict__ ref, const T* __restrict__ tba,
                                                    const uint8_t* __restrict__ valid, const T* __restrict__ aspect, T* __restrict__ dh,
                                                    unsigned long long* __restrict__ keys, unsigned long long* __restrict__ n_fin) {
    typedef typename KeyT<T>::type K;
    if (!active[blockIdx.y]) return;
    const BwTile t = tiles[blockIdx.y];
    NkGeom g;
    g.H = t.h; g.W = t.w; g.roff = 0; g.dr = dr[blockIdx.y]; g.dc = dc[blockIdx.y]; g.rule = rule;
    const T* img = tba + t.off;
    const uint32_t n = (uint32_t)t.h * (uint32_t)t.w, w = (uint32_t)t.w;
    K kmin = ~(K)0, kmax = 0;
    unsigned long long fin = 0;
    for (uint32_t p = blockIdx.x * 256u + threadIdx.x; p < n; p += gridDim.x * 256u) {
        const uint32_t i = p / w, j = p - i * w;
        const BiTap tp = bi_locate(g, (int64_t)i, (int64_t)j);
        const BiVals<T> tv = bi_load<T>(img, tp);
        T val;
        const bool ok = bi_value<T>(g, img, tp, tv.a00, tv.a01, tv.a10, tv.a11, val) & (valid[t.off + p] != 0);
        T out = t_sub(ref[t.off + p], val);
        if (ok && t_finite(out)) {
            const K ka = key_of(aspect[t.off + p]);
            kmin = ka < kmin ? ka : kmin;
            kmax = ka > kmax ? ka : kmax;
            ++fin;
        } else {
            out = (T)NAN;   // THE positive quiet NaN: its key lies above every finite value's (bw_vshift_kernel relies on it)
        }
        dh[t.off + p] = out;
    }
    for (int off = 32; off > 0; off >>= 1) {
        const K a = k_shfl_down(kmin, off), b = k_shfl_down(kmax, off);
        kmin = a < kmin ? a : kmin;
        kmax = b > kmax ? b : kmax;
        fin += __shfl_down(fin, off);
    }
    if ((threadIdx.x & 63) == 0 && fin) {
        atomicMin(&keys[2 * blockIdx.y], (unsigned long long)kmin);
        atomicMax(&keys[2 * blockIdx.y + 1], (unsigned long long)kmax);
        atomicAdd(&n_fin[blockIdx.y], fin);
    }
}

// np.nanmedian of the tile's dh.  The selection runs over ALL h * w samples of the tile: the non-finite ones are the one NaN that
// bw_dh_kernel writes, whose order-preserving key is larger than the key of +infinity, so the ranks below the finite count are the
// ranks among the finite values.  Then SciPy's automatic bin edges from the tile's own min / max aspect.
template <typename T>
__global__ __launch_bounds__(HYP_THREADS) void bw_vshift_kernel(const BwTile* __restrict__ tiles, const uint8_t* __restrict__ active, int nb,
                                                                const T* __restrict__ dh, const unsigned long long* __restrict__ keys,
                                                                const unsigned long long* __restrict__ n_fin, T* __restrict__ vshift_t,
                                                                T* __restrict__ edges_t, double* __restrict__ r_vshift, int64_t* __restrict__ r_nvalid,
                                                                double* __restrict__ r_edges) {
    typedef typename KeyT<T>::type K;
    __shared__ HypSelectShared s_sel;
    const int ti = blockIdx.x;
    if (!active[ti]) return;
    const BwTile t = tiles[ti];
    const uint64_t nf = n_fin[ti];
    T* e = edges_t + (size_t)ti * (BW_MAX_BINS + 1);
    if (nf == 0) {   // (uniform over the workgroup)
        if (threadIdx.x == 0) { r_vshift[ti] = (double)NAN; r_nvalid[ti] = 0; vshift_t[ti] = (T)NAN; }
        for (int k = threadIdx.x; k <= nb; k += HYP_THREADS) { e[k] = (T)NAN; r_edges[(size_t)ti * (nb + 1) + k] = (double)NAN; }
        return;
    }
    const int64_t n = (int64_t)t.h * t.w;
    const uint64_t k0 = (nf - 1) / 2, k1 = nf / 2;
    const K klo = hyp_radix_select<T>(dh + t.off, n, k0, &s_sel);
    const K khi = k1 == k0 ? klo : hyp_radix_select<T>(dh + t.off, n, k1, &s_sel);
    const T lo = val_of(klo), hi = val_of(khi);
    const T vs = k0 == k1 ? lo : (T)((T)(lo + hi) / (T)2);   // np.nanmedian: the mean of the two middle values in the raster dtype
    if (threadIdx.x == 0) {
        vshift_t[ti] = vs;
        r_vshift[ti] = (double)vs;
        r_nvalid[ti] = (int64_t)nf;
        make_edges_into<T>((double)val_of((K)keys[2 * ti]), (double)val_of((K)keys[2 * ti + 1]), nb, e);
        for (int k = 0; k <= nb; ++k) r_edges[(size_t)ti * (nb + 1) + k] = (double)e[k];
    }
}

template <typename T>
__global__ __launch_bounds__(256) void bw_y_kernel(const BwTile* __restrict__ tiles, const uint8_t* __restrict__ active, int nb, const T* __restrict__ dh,
                                                   const T* __restrict__ slope_tan, const T* __restrict__ aspect, const unsigned long long* __restrict__ n_fin,
                                                   const T* __restrict__ vshift_t, const T* __restrict__ edges_t, T* __restrict__ y,
                                                   uint8_t* __restrict__ bin, unsigned long long* __restrict__ cnt) {
    __shared__ T e[BW_MAX_BINS + 1];
    __shared__ unsigned int hist[BW_MAX_BINS];
    const int ti = blockIdx.y;
    if (!active[ti] || n_fin[ti] == 0) return;
    const BwTile t = tiles[ti];
    for (int k = threadIdx.x; k <= nb; k += 256) e[k] = edges_t[(size_t)ti * (BW_MAX_BINS + 1) + k];
    for (int k = threadIdx.x; k < nb; k += 256) hist[k] = 0u;
    __syncthreads();
    const T vs = vshift_t[ti];
    const double inv_width = (double)nb / ((double)e[nb] - (double)e[0]);
    const uint32_t n = (uint32_t)t.h * (uint32_t)t.w;
    for (uint32_t p = blockIdx.x * 256u + threadIdx.x; p < n; p += gridDim.x * 256u) {
        const T d = dh[t.off + p];
        T yv = (T)NAN;
        uint8_t b = BW_NOBIN;
        if (d == d) {   // dh is NaN wherever the pixel is unusable
            yv = t_div(t_sub(d, vs), slope_tan[t.off + p]);
            const uint16_t b16 = aspect_bin<T>(aspect[t.off + p], e, nb, inv_width, NK_AUTO_EDGES);
            if (b16 != (uint16_t)0xFFFF && t_finite(yv)) {   // (nd_binning drops non-finite values before it bins)
                b = (uint8_t)b16;
                atomicAdd(&hist[b], 1u);
            }
        }
        y[t.off + p] = yv;
        bin[t.off + p] = b;
    }
    __syncthreads();
    for (int k = threadIdx.x; k < nb; k += 256)
        if (hist[k]) atomicAdd(&cnt[(size_t)ti * BW_MAX_BINS + k], (unsigned long long)hist[k]);
}

// one workgroup per tile: where each bin's segment starts inside the tile's slice of `seg`, and the moments of y.  np.nanmean /
// np.nanstd (ddof 0) in float64: the mean, then the squared deviations, both summed in one fixed order (volume.h: hyp_fixed_sum).
template <typename T>
__global__ __launch_bounds__(HYP_THREADS) void bw_scan_kernel(const BwTile* __restrict__ tiles, const uint8_t* __restrict__ active, int nb,
                                                              const T* __restrict__ dh, const T* __restrict__ y, const unsigned long long* __restrict__ n_fin,
                                                              const unsigned long long* __restrict__ cnt, unsigned long long* __restrict__ seg_off,
                                                              unsigned long long* __restrict__ cursor, double* __restrict__ r_ymean, double* __restrict__ r_ystd) {
    __shared__ double s_red[HYP_THREADS];
    const int ti = blockIdx.x;
    if (!active[ti]) return;
    const uint64_t nf = n_fin[ti];
    if (nf == 0) {
        if (threadIdx.x == 0) { r_ymean[ti] = (double)NAN; r_ystd[ti] = (double)NAN; }
        return;
    }
    const BwTile t = tiles[ti];
    if (threadIdx.x == 0) {
        unsigned long long run = 0;
        for (int b = 0; b < nb; ++b) {
            seg_off[(size_t)ti * BW_MAX_BINS + b] = run;
            cursor[(size_t)ti * BW_MAX_BINS + b] = run;
            run += cnt[(size_t)ti * BW_MAX_BINS + b];
        }
    }
    const int64_t n = (int64_t)t.h * t.w;
    const T* dv = dh + t.off;
    const T* yv = y + t.off;
    const double mean = hyp_fixed_sum([&](int64_t i) { return dv[i] == dv[i] ? (double)yv[i] : 0.0; }, n, s_red) / (double)nf;
    const double ss = hyp_fixed_sum([&](int64_t i) { const double d = (double)yv[i] - mean; return dv[i] == dv[i] ? d * d : 0.0; }, n, s_red);
    if (threadIdx.x == 0) { r_ymean[ti] = mean; r_ystd[ti] = sqrt(ss / (double)nf); }
}

// A workgroup counts its samples per bin in LDS, takes its places in every bin's segment with one atomic per bin, then hands them out
// in LDS: two reads of a byte per sample instead of one global atomic per sample.
template <typename T>
__global__ __launch_bounds__(256) void bw_scatter_kernel(const BwTile* __restrict__ tiles, const uint8_t* __restrict__ active, int nb,
                                                         const T* __restrict__ y, const uint8_t* __restrict__ bin, const unsigned long long* __restrict__ n_fin,
                                                         unsigned long long* __restrict__ cursor, T* __restrict__ seg) {
    __shared__ unsigned int s_cnt[BW_MAX_BINS];
    __shared__ unsigned long long s_base[BW_MAX_BINS];
    const int ti = blockIdx.y;
    if (!active[ti] || n_fin[ti] == 0) return;
    const BwTile t = tiles[ti];
    for (int k = threadIdx.x; k < BW_MAX_BINS; k += 256) s_cnt[k] = 0u;
    __syncthreads();
    const uint32_t n = (uint32_t)t.h * (uint32_t)t.w;
    for (uint32_t p = blockIdx.x * 256u + threadIdx.x; p < n; p += gridDim.x * 256u) {
        const uint8_t b = bin[t.off + p];
        if (b < nb) atomicAdd(&s_cnt[b], 1u);
    }
    __syncthreads();
    for (int k = threadIdx.x; k < nb; k += 256) {
        s_base[k] = s_cnt[k] ? atomicAdd(&cursor[(size_t)ti * BW_MAX_BINS + k], (unsigned long long)s_cnt[k]) : 0ull;
        s_cnt[k] = 0u;
    }
    __syncthreads();
    for (uint32_t p = blockIdx.x * 256u + threadIdx.x; p < n; p += gridDim.x * 256u) {
        const uint8_t b = bin[t.off + p];
        if (b < nb) {
            const unsigned int k = atomicAdd(&s_cnt[b], 1u);
            seg[t.off + (int64_t)(s_base[b] + k)] = y[t.off + p];   // (the bin counts of a tile add up to at most h * w: inside its slice)
        }
    }
}

// one workgroup per (tile, bin): count and exact median.  np.nanmedian: the mean of the two middle values in the raster dtype for an
// even count.  A segment of at most `cap` values is sorted in LDS as keys, a longer one takes the radix selection over its slice.
template <typename T>
__global__ __launch_bounds__(HYP_THREADS) void bw_segment_kernel(const BwTile* __restrict__ tiles, const uint8_t* __restrict__ active, int nb, int cap,
                                                                 const T* __restrict__ seg, const unsigned long long* __restrict__ n_fin,
                                                                 const unsigned long long* __restrict__ cnt, const unsigned long long* __restrict__ seg_off,
                                                                 int64_t* __restrict__ r_counts, double* __restrict__ r_med) {
    typedef typename KeyT<T>::type K;
    __shared__ K s_keys[BW_SEG_LDS];
    __shared__ HypSelectShared s_sel;
    const int ti = blockIdx.x / nb, b = blockIdx.x % nb;
    if (!active[ti]) return;
    const int64_t c = n_fin[ti] ? (int64_t)cnt[(size_t)ti * BW_MAX_BINS + b] : 0;
    if (c == 0) {
        if (threadIdx.x == 0) { r_counts[(size_t)ti * nb + b] = 0; r_med[(size_t)ti * nb + b] = (double)NAN; }
        return;
    }
    const T* v = seg + tiles[ti].off + (int64_t)seg_off[(size_t)ti * BW_MAX_BINS + b];
    const int64_t k0 = (c - 1) / 2, k1 = c / 2;
    T lo, hi;
    if (c <= cap) {
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
    }
    const T m = k0 == k1 ? lo : (T)((T)(lo + hi) / (T)2);
    if (threadIdx.x == 0) { r_counts[(size_t)ti * nb + b] = c; r_med[(size_t)ti * nb + b] = (double)m; }
}

// ---- the warp of BlockwiseCoreg.apply ------------------------------------------------------------------------------------------------
// The shift field s(x, y) = (a_x x + b_x y + d_x, a_y x + b_y y + d_y) moves a point p to (I + A) p + d; an output pixel centre p' takes
// its value from p = (I + A)^-1 (p' - d): out = (T)(bilinear(dem)(row(p), col(p)) + s_z(p)).  Float64, every operation rounded on its
// own, in the order tests/blockwise_oracle.py writes them.
struct BwWarp {
    double a, c, e, f;            // x = a (col + 0.5) + c, y = e (row + 0.5) + f
    double i00, i01, i10, i11;    // (I + A)^-1
    double dx, dy;
    double az, bz, dz;
};
template <typename T>
__global__ __launch_bounds__(256) void bw_apply_kernel(const T* __restrict__ dem, NkGeom g, BwWarp w, T* __restrict__ out) {
    const int64_t n = g.H * g.W;
    const double invW = 1.0 / (double)g.W;
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < n; q += (int64_t)gridDim.x * blockDim.x) {
        int64_t i, j;
        row_col(q, g.W, invW, i, j);
        const double xo = w.a * ((double)j + 0.5) + w.c, yo = w.e * ((double)i + 0.5) + w.f;
        const double ux = xo - w.dx, uy = yo - w.dy;
        const double px = w.i00 * ux + w.i01 * uy, py = w.i10 * ux + w.i11 * uy;
        const double sz = (w.az * px + w.bz * py) + w.dz;
        const double col = (px - w.c) / w.a - 0.5, row = (py - w.f) / w.e - 0.5;
        T v;
        const bool ok = bi_point<T>(g, dem, row, col, v);
        out[q] = ok ? (T)((double)v + sz) : (T)NAN;
    }
}

}  // namespace
}  // namespace xd

using namespace xd;

struct xdemhip_bw_plan {
    xdemhip_ctx* ctx = nullptr;
    int dtype = XDEMHIP_F32;
    int n_tiles = 0;
    int nan_rule = 0;
    int64_t total = 0, max_px = 0;   // samples of all tiles; of the largest tile
    XdOwned mem;
    BwTile* tiles = nullptr;
    void *ref = nullptr, *tba = nullptr, *slope_tan = nullptr, *aspect = nullptr, *dh = nullptr, *y = nullptr, *seg = nullptr;
    uint8_t *valid = nullptr, *bin = nullptr;
    unsigned char* step_in = nullptr;    // dr[n] | dc[n] | active[n]
    unsigned long long *keys = nullptr, *n_fin = nullptr, *cnt = nullptr, *seg_off = nullptr, *cursor = nullptr;
    void *vshift_t = nullptr, *edges_t = nullptr;
    unsigned char* res = nullptr;        // the results of a step, one block (layout: bw_step_typed)
    std::vector<unsigned char> host_in, host_res;
};

namespace {

size_t bw_res_bytes(int n, int nb) { return (size_t)n * 8 * (4 + (size_t)(nb + 1) + 2 * (size_t)nb); }

unsigned bw_blocks(int64_t max_px) {
    const int64_t b = (max_px + 2047) / 2048;   // eight samples per thread
    return (unsigned)(b < 1 ? 1 : (b > 1024 ? 1024 : b));
}

template <typename T>
int bw_create_typed(xdemhip_bw_plan* P, const void* ref, const void* tba, const uint8_t* inlier, int64_t H, int64_t W, int memspace, int64_t* n_valid) {
    xdemhip_ctx* ctx = P->ctx;
    const int n = P->n_tiles;
    std::vector<unsigned long long> nv((size_t)n, 0ull);   // (a copy's destination: declared before the buffers)
    XdBuffers buf(ctx, "xdemhip_bw_create");
    const T* d_ref = static_cast<const T*>(buf.input(ref, (size_t)H * W * sizeof(T), memspace));
    const T* d_tba = static_cast<const T*>(buf.input(tba, (size_t)H * W * sizeof(T), memspace));
    const uint8_t* d_inl = buf.input(inlier, (size_t)H * W, memspace);
    if (buf.rc) return buf.rc;
    const dim3 grid(bw_blocks(P->max_px), (unsigned)n);
    hipLaunchKernelGGL((bw_gather_kernel<T>), grid, dim3(256), 0, ctx->stream, d_ref, d_tba, W, P->tiles, static_cast<T*>(P->ref), static_cast<T*>(P->tba));
    XD_HIP_CHECK(ctx, hipMemsetAsync(P->n_fin, 0, (size_t)n * 8, ctx->stream));
    hipLaunchKernelGGL((bw_aux_kernel<T>), grid, dim3(256), 0, ctx->stream, static_cast<const T*>(P->ref), static_cast<const T*>(P->tba), d_inl, W, P->tiles,
                       static_cast<T*>(P->slope_tan), static_cast<T*>(P->aspect), P->valid, P->n_fin);
    int rc = launched(ctx, "bw_aux_kernel");
    if (rc) return rc;
    XD_HIP_CHECK(ctx, hipMemcpyAsync(nv.data(), P->n_fin, (size_t)n * 8, hipMemcpyDeviceToHost, ctx->stream));
    rc = xd_sync(ctx);
    if (rc) return rc;
    for (int t = 0; t < n; ++t) n_valid[t] = (int64_t)nv[t];
    return buf.finish();
}

template <typename T>
int bw_step_typed(xdemhip_bw_plan* P, const uint8_t* active, const double* shift_x, const double* shift_y, double res_x, double res_y, int nb,
                  double* vshift, int64_t* n_valid, double* y_mean, double* y_std, double* edges, int64_t* counts, double* medians) {
    xdemhip_ctx* ctx = P->ctx;
    const int n = P->n_tiles;
    // tba is sampled at (row - shift_y / res_y, col + shift_x / res_x), as the whole-raster plan does
    P->host_in.resize((size_t)n * 17);
    double* h_dr = reinterpret_cast<double*>(P->host_in.data());
    double* h_dc = h_dr + n;
    for (int t = 0; t < n; ++t) { h_dr[t] = -shift_y[t] / res_y; h_dc[t] = shift_x[t] / res_x; }
    memcpy(P->host_in.data() + (size_t)n * 16, active, (size_t)n);
    XD_HIP_CHECK(ctx, hipMemcpyAsync(P->step_in, P->host_in.data(), P->host_in.size(), hipMemcpyHostToDevice, ctx->stream));
    const double* d_dr = reinterpret_cast<const double*>(P->step_in);
    const double* d_dc = d_dr + n;
    const uint8_t* d_act = P->step_in + (size_t)n * 16;
    // the results of the step, one block: vshift[n] | n_valid[n] | y_mean[n] | y_std[n] | edges[n][nb + 1] | counts[n][nb] | medians[n][nb]
    double* r_vshift = reinterpret_cast<double*>(P->res);
    int64_t* r_nvalid = reinterpret_cast<int64_t*>(r_vshift + n);
    double* r_ymean = reinterpret_cast<double*>(r_nvalid + n);
    double* r_ystd = r_ymean + n;
    double* r_edges = r_ystd + n;
    int64_t* r_counts = reinterpret_cast<int64_t*>(r_edges + (size_t)n * (nb + 1));
    double* r_med = reinterpret_cast<double*>(r_counts + (size_t)n * nb);
    const dim3 grid(bw_blocks(P->max_px), (unsigned)n);
    const int cap = ctx->bw_seg_lds ? ctx->bw_seg_lds : BW_SEG_LDS;
    const T *ref = static_cast<const T*>(P->ref), *tba = static_cast<const T*>(P->tba), *st = static_cast<const T*>(P->slope_tan),
            *asp = static_cast<const T*>(P->aspect);
    T *dh = static_cast<T*>(P->dh), *y = static_cast<T*>(P->y), *seg = static_cast<T*>(P->seg), *vs_t = static_cast<T*>(P->vshift_t),
      *e_t = static_cast<T*>(P->edges_t);
    hipLaunchKernelGGL(bw_init_kernel, dim3((unsigned)(((int64_t)n * BW_MAX_BINS + 255) / 256)), dim3(256), 0, ctx->stream, n, nb, d_act, P->keys, P->n_fin, P->cnt);
    hipLaunchKernelGGL((bw_dh_kernel<T>), grid, dim3(256), 0, ctx->stream, P->tiles, d_act, d_dr, d_dc, P->nan_rule, ref, tba, P->valid, asp, dh, P->keys, P->n_fin);
    hipLaunchKernelGGL((bw_vshift_kernel<T>), dim3((unsigned)n), dim3(HYP_THREADS), 0, ctx->stream, P->tiles, d_act, nb, dh, P->keys, P->n_fin, vs_t, e_t, r_vshift,
                       r_nvalid, r_edges);
    hipLaunchKernelGGL((bw_y_kernel<T>), grid, dim3(256), 0, ctx->stream, P->tiles, d_act, nb, dh, st, asp, P->n_fin, vs_t, e_t, y, P->bin, P->cnt);
    hipLaunchKernelGGL((bw_scan_kernel<T>), dim3((unsigned)n), dim3(HYP_THREADS), 0, ctx->stream, P->tiles, d_act, nb, dh, y, P->n_fin, P->cnt, P->seg_off, P->cursor,
                       r_ymean, r_ystd);
    hipLaunchKernelGGL((bw_scatter_kernel<T>), grid, dim3(256), 0, ctx->stream, P->tiles, d_act, nb, y, P->bin, P->n_fin, P->cursor, seg);
    hipLaunchKernelGGL((bw_segment_kernel<T>), dim3((unsigned)((int64_t)n * nb)), dim3(HYP_THREADS), 0, ctx->stream, P->tiles, d_act, nb, cap, seg, P->n_fin, P->cnt,
                       P->seg_off, r_counts, r_med);
    int rc = launched(ctx, "blockwise step");
    if (rc) return rc;
    P->host_res.resize(bw_res_bytes(n, nb));
    XD_HIP_CHECK(ctx, hipMemcpyAsync(P->host_res.data(), P->res, P->host_res.size(), hipMemcpyDeviceToHost, ctx->stream));
    rc = xd_sync(ctx);
    if (rc) return rc;
    const unsigned char* h = P->host_res.data();
    const size_t N = (size_t)n;
    for (int t = 0; t < n; ++t) {
        if (!active[t]) continue;   // a frozen tile's entries stay as the caller has them
        memcpy(&vshift[t], h + 8 * (size_t)t, 8);
        memcpy(&n_valid[t], h + 8 * (N + t), 8);
        memcpy(&y_mean[t], h + 8 * (2 * N + t), 8);
        memcpy(&y_std[t], h + 8 * (3 * N + t), 8);
        memcpy(edges + (size_t)t * (nb + 1), h + 8 * (4 * N + (size_t)t * (nb + 1)), 8 * (size_t)(nb + 1));
        memcpy(counts + (size_t)t * nb, h + 8 * (4 * N + N * (nb + 1) + (size_t)t * nb), 8 * (size_t)nb);
        memcpy(medians + (size_t)t * nb, h + 8 * (4 * N + N * (nb + 1) + N * nb + (size_t)t * nb), 8 * (size_t)nb);
    }
    return XDEMHIP_OK;
}

}  // namespace

extern "C" {

void xdemhip_bw_destroy(xdemhip_bw_plan* P) {
    delete P;   // (its owner frees the device buffers)
}

int xdemhip_bw_create(xdemhip_ctx* ctx, const void* ref, const void* tba, const unsigned char* inlier, int dtype, int64_t H, int64_t W, int n_tiles,
                      const int64_t* tiles4, int memspace, xdemhip_bw_plan** out, int64_t* n_valid) {
    if (!ctx) return XDEMHIP_EINVAL;
    if (!ref || !tba || !tiles4 || !out || !n_valid) return xd_fail(ctx, XDEMHIP_EINVAL, "null argument");
    if (dtype != XDEMHIP_F32 && dtype != XDEMHIP_F64) return xd_fail(ctx, XDEMHIP_EINVAL, "dtype must be float32 or float64");
    if (memspace != XDEMHIP_HOST && memspace != XDEMHIP_DEVICE) return xd_fail(ctx, XDEMHIP_EINVAL, "bad memspace");
    if (H < 2 || W < 2 || W > ((int64_t)1 << 31)) return xd_fail(ctx, XDEMHIP_EINVAL, "raster shape");
    if (n_tiles < 1 || n_tiles > 65535) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_bw_create: 1 to 65535 tiles");
    if (ctx->allreduce) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_bw_create: single-process plans only (a reduction hook is installed)");
    std::vector<BwTile> tiles((size_t)n_tiles);
    int64_t total = 0, max_px = 0;
    for (int t = 0; t < n_tiles; ++t) {
        const int64_t r0 = tiles4[4 * t], r1 = tiles4[4 * t + 1], c0 = tiles4[4 * t + 2], c1 = tiles4[4 * t + 3];
        // (np.gradient needs two samples along each axis; a tile's samples are indexed with 32 bits)
        if (r0 < 0 || c0 < 0 || r1 > H || c1 > W || r1 - r0 < 2 || c1 - c0 < 2 || (r1 - r0) * (c1 - c0) >= ((int64_t)1 << 31))
            return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_bw_create: a tile must lie inside the raster, hold at least 2 x 2 and fewer than 2^31 pixels");
        tiles[t].off = total;
        tiles[t].h = (int32_t)(r1 - r0); tiles[t].w = (int32_t)(c1 - c0);
        tiles[t].r0 = (int32_t)r0; tiles[t].c0 = (int32_t)c0;
        const int64_t px = (r1 - r0) * (c1 - c0);
        total += px;
        max_px = px > max_px ? px : max_px;
    }
    XD_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    xdemhip_bw_plan* P = new xdemhip_bw_plan;
    P->ctx = P->mem.ctx = ctx; P->dtype = dtype; P->n_tiles = n_tiles; P->nan_rule = ctx->nk_nan_rule; P->total = total; P->max_px = max_px;
    const size_t es = dtype == XDEMHIP_F32 ? 4 : 8, N = (size_t)n_tiles;
    auto take = [&](size_t bytes) { return P->mem.take(bytes, "xdemhip_bw_create"); };
    P->tiles = static_cast<BwTile*>(take(N * sizeof(BwTile)));
    P->ref = take(total * es); P->tba = take(total * es); P->slope_tan = take(total * es); P->aspect = take(total * es);
    P->dh = take(total * es); P->y = take(total * es); P->seg = take(total * es);
    P->valid = static_cast<uint8_t*>(take(total)); P->bin = static_cast<uint8_t*>(take(total));
    P->step_in = static_cast<unsigned char*>(take(N * 17));
    P->keys = static_cast<unsigned long long*>(take(N * 16));
    P->n_fin = static_cast<unsigned long long*>(take(N * 8));
    P->cnt = static_cast<unsigned long long*>(take(N * BW_MAX_BINS * 8));
    P->seg_off = static_cast<unsigned long long*>(take(N * BW_MAX_BINS * 8));
    P->cursor = static_cast<unsigned long long*>(take(N * BW_MAX_BINS * 8));
    P->vshift_t = take(N * es);
    P->edges_t = take(N * (BW_MAX_BINS + 1) * es);
    P->res = static_cast<unsigned char*>(take(bw_res_bytes(n_tiles, BW_MAX_BINS)));
    int rc = P->mem.rc;
    if (rc == XDEMHIP_OK && hipMemcpyAsync(P->tiles, tiles.data(), N * sizeof(BwTile), hipMemcpyHostToDevice, ctx->stream) != hipSuccess)
        rc = xd_fail(ctx, XDEMHIP_EHIP, "H2D copy failed (xdemhip_bw_create)");
    if (rc == XDEMHIP_OK)   // (`tiles` outlives the copy: both typed functions synchronise the stream before they return)
        rc = dtype == XDEMHIP_F32 ? bw_create_typed<float>(P, ref, tba, inlier, H, W, memspace, n_valid)
                                  : bw_create_typed<double>(P, ref, tba, inlier, H, W, memspace, n_valid);
    if (rc) { xdemhip_bw_destroy(P); return rc; }
    *out = P;
    return XDEMHIP_OK;
}

int xdemhip_bw_nk_step(xdemhip_bw_plan* P, const unsigned char* active, const double* shift_x, const double* shift_y, double res_x, double res_y, int n_bins,
                       double* vshift, int64_t* n_valid, double* y_mean, double* y_std, double* edges, int64_t* counts, double* medians) {
    if (!P) return XDEMHIP_EINVAL;
    xdemhip_ctx* ctx = P->ctx;
    if (!active || !shift_x || !shift_y || !vshift || !n_valid || !y_mean || !y_std || !edges || !counts || !medians)
        return xd_fail(ctx, XDEMHIP_EINVAL, "null argument");
    if (n_bins < 1 || n_bins > BW_MAX_BINS) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_bw_nk_step: 1 to 128 aspect bins");
    if (!(res_x > 0) || !(res_y > 0)) return xd_fail(ctx, XDEMHIP_EINVAL, "resolution must be positive");
    XD_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    return P->dtype == XDEMHIP_F32 ? bw_step_typed<float>(P, active, shift_x, shift_y, res_x, res_y, n_bins, vshift, n_valid, y_mean, y_std, edges, counts, medians)
                                   : bw_step_typed<double>(P, active, shift_x, shift_y, res_x, res_y, n_bins, vshift, n_valid, y_mean, y_std, edges, counts, medians);
}

int xdemhip_bw_get_aux(xdemhip_bw_plan* P, void* slope_tan, void* aspect, unsigned char* valid) {
    if (!P) return XDEMHIP_EINVAL;
    xdemhip_ctx* ctx = P->ctx;
    if (!slope_tan || !aspect || !valid) return xd_fail(ctx, XDEMHIP_EINVAL, "null argument");
    XD_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    const size_t es = P->dtype == XDEMHIP_F32 ? 4 : 8;
    XD_HIP_CHECK(ctx, hipMemcpyAsync(slope_tan, P->slope_tan, (size_t)P->total * es, hipMemcpyDeviceToHost, ctx->stream));
    XD_HIP_CHECK(ctx, hipMemcpyAsync(aspect, P->aspect, (size_t)P->total * es, hipMemcpyDeviceToHost, ctx->stream));
    XD_HIP_CHECK(ctx, hipMemcpyAsync(valid, P->valid, (size_t)P->total, hipMemcpyDeviceToHost, ctx->stream));
    return xd_sync(ctx);
}

int xdemhip_bw_apply(xdemhip_ctx* ctx, const void* dem, int dtype, int64_t H, int64_t W, const double* transform6, const double* coeff_x3,
                     const double* coeff_y3, const double* coeff_z3, void* out, int memspace) {
    if (!ctx) return XDEMHIP_EINVAL;
    if (!dem || !transform6 || !coeff_x3 || !coeff_y3 || !coeff_z3 || !out) return xd_fail(ctx, XDEMHIP_EINVAL, "null argument");
    if (dtype != XDEMHIP_F32 && dtype != XDEMHIP_F64) return xd_fail(ctx, XDEMHIP_EINVAL, "dtype must be float32 or float64");
    if (memspace != XDEMHIP_HOST && memspace != XDEMHIP_DEVICE) return xd_fail(ctx, XDEMHIP_EINVAL, "bad memspace");
    if (H < 1 || W < 1 || W > ((int64_t)1 << 31)) return xd_fail(ctx, XDEMHIP_EINVAL, "raster shape");
    // transform6 = (a, b, c, d, e, f) of x = a col + b row + c, y = d col + e row + f at pixel CORNERS; centres are half a pixel in
    if (transform6[1] != 0.0 || transform6[3] != 0.0 || !(transform6[0] != 0.0) || !(transform6[4] != 0.0))
        return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_bw_apply: the transform must be axis-aligned (b = d = 0, a and e non-zero)");
    for (int k = 0; k < 3; ++k)
        if (!isfinite(coeff_x3[k]) || !isfinite(coeff_y3[k]) || !isfinite(coeff_z3[k])) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_bw_apply: non-finite coefficient");
    BwWarp w;
    w.a = transform6[0]; w.c = transform6[2]; w.e = transform6[4]; w.f = transform6[5];
    const double m00 = 1.0 + coeff_x3[0], m01 = coeff_x3[1], m10 = coeff_y3[0], m11 = 1.0 + coeff_y3[1];
    const double det = m00 * m11 - m01 * m10;
    if (!(det != 0.0) || !isfinite(det)) return xd_fail(ctx, XDEMHIP_EINVAL, "xdemhip_bw_apply: singular shift field (I + A has no inverse)");
    w.i00 = m11 / det; w.i01 = -m01 / det; w.i10 = -m10 / det; w.i11 = m00 / det;
    w.dx = coeff_x3[2]; w.dy = coeff_y3[2];
    w.az = coeff_z3[0]; w.bz = coeff_z3[1]; w.dz = coeff_z3[2];
    XD_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    const size_t bytes = (size_t)H * W * (dtype == XDEMHIP_F32 ? 4 : 8);
    XdBuffers buf(ctx, "xdemhip_bw_apply");
    const void* d_dem = buf.input(dem, bytes, memspace);
    void* d_out = buf.output(out, bytes, memspace);
    if (buf.rc) return buf.rc;
    NkGeom g;
    g.H = H; g.W = W; g.roff = 0; g.dr = 0.0; g.dc = 0.0; g.rule = ctx->nk_nan_rule;
    const dim3 grid((unsigned)grid_for(ctx, H * W, 256, 16));
    if (dtype == XDEMHIP_F32) hipLaunchKernelGGL((bw_apply_kernel<float>), grid, dim3(256), 0, ctx->stream, static_cast<const float*>(d_dem), g, w, static_cast<float*>(d_out));
    else hipLaunchKernelGGL((bw_apply_kernel<double>), grid, dim3(256), 0, ctx->stream, static_cast<const double*>(d_dem), g, w, static_cast<double*>(d_out));
    const int rc = launched(ctx, "bw_apply_kernel");
    if (rc) return rc;
    return buf.finish();
}

}  // extern "C"
