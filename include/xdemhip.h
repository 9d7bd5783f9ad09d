/* xdemhip.h -- C-ABI of libxdemhip.so: MI355X (gfx950) kernels for xDEM's three dense-array hot paths.
 *
 * The reference (GlacioHack/xdem) has no FFI: its operator boundary for these paths is a set of private
 * Python engine functions that take plain ndarrays.  Every entry point below cites
 * the reference function it stands in for; the ctypes binding a maintainer would add is in INTEGRATION.md
 * and is what xdem_amd/_lib.py implements.
 *
 * Conventions
 *  - every function returns 0 on success or a negative XDEMHIP_E* code; nothing throws; the text of the
 *    last error of a context is available through xdemhip_last_error();
 *  - the caller owns every buffer; the library owns only the opaque context (one per GPU / per process);
 *  - `memspace` says where the caller's buffers live: XDEMHIP_HOST (the library stages H2D/D2H itself) or
 *    XDEMHIP_DEVICE (raw device pointers, e.g. torch tensors' data_ptr(); work is enqueued on the context
 *    stream and the call returns without synchronising);
 *  - rasters are row-major, element (row, col) at base[row * row_stride + col]; all sizes are 64-bit.
 */
#ifndef XDEMHIP_H
#define XDEMHIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Threading contract: the library is re-entrant PER CONTEXT.  A context owns one stream, one scratch state and one queue of
 * deferred result copies; calls on the same context (and on plans / pair sets created from it) must not overlap in time --
 * drive a context from one thread at a time.  Different contexts may be used from different threads concurrently. */
typedef struct xdemhip_ctx xdemhip_ctx;

enum { XDEMHIP_OK = 0, XDEMHIP_EINVAL = -1, XDEMHIP_ENODEV = -2, XDEMHIP_EHIP = -3, XDEMHIP_ENOMEM = -4,
       XDEMHIP_EUNSUPPORTED = -5 };
enum { XDEMHIP_F32 = 0, XDEMHIP_F64 = 1 };
enum { XDEMHIP_HOST = 0, XDEMHIP_DEVICE = 1 };

/* surface_fit ids: xdem/terrain/surfit.py:1240 ; curvature method ids: surfit.py:1244 ; TRI: window.py:964 */
enum { XDEMHIP_FIT_HORN = 0, XDEMHIP_FIT_ZEVENBERGTHORNE = 1, XDEMHIP_FIT_FLORINSKY = 2 };
enum { XDEMHIP_CURV_GEOMETRIC = 0, XDEMHIP_CURV_DIRECTIONAL = 1 };
enum { XDEMHIP_TRI_RILEY = 0, XDEMHIP_TRI_WILSON = 1 };

/* Attribute bits.  Bits 0-9 follow the reference's fixed attribute order (surfit.py:407-418), bits 10-11
 * are the two windowed indexes of window.py:752-758 that are on the hot path, bit 12 the first "next" one. */
enum {
    XDEMHIP_ATTR_SLOPE = 1u << 0,
    XDEMHIP_ATTR_ASPECT = 1u << 1,
    XDEMHIP_ATTR_HILLSHADE = 1u << 2,
    XDEMHIP_ATTR_CURVATURE = 1u << 3,
    XDEMHIP_ATTR_PROFILE_CURVATURE = 1u << 4,
    XDEMHIP_ATTR_TANGENTIAL_CURVATURE = 1u << 5,
    XDEMHIP_ATTR_PLANFORM_CURVATURE = 1u << 6,
    XDEMHIP_ATTR_FLOWLINE_CURVATURE = 1u << 7,
    XDEMHIP_ATTR_MAX_CURVATURE = 1u << 8,
    XDEMHIP_ATTR_MIN_CURVATURE = 1u << 9,
    XDEMHIP_ATTR_TPI = 1u << 10,
    XDEMHIP_ATTR_TRI = 1u << 11,
    XDEMHIP_ATTR_ROUGHNESS = 1u << 12, /* max - min of the window (window.py:261-308) */
    XDEMHIP_ATTR_RUGOSITY = 1u << 13,  /* 8f-2: Jenness surface-area ratio, always 3x3, needs resolution (window.py:466-563) */
    XDEMHIP_ATTR_FRACTAL_ROUGHNESS = 1u << 14, /* 8f-2: box-counting dimension over window_size (window.py:316-401);
                                                   the reference runs it in a second engine call with its own
                                                   window_size_fractal (terrain.py:619-630): do the same here */
    XDEMHIP_ATTR_COUNT = 15
};

/* ---- context ------------------------------------------------------------------------------------- */
int xdemhip_version(void);
/* One context per process and GPU (the multi-GPU layer is one process per GPU, torch.distributed/RCCL). */
int xdemhip_create(int device_id, xdemhip_ctx** out_ctx);
void xdemhip_destroy(xdemhip_ctx* ctx);
const char* xdemhip_last_error(const xdemhip_ctx* ctx);
/* Enqueue on the caller's hipStream_t, e.g. torch.cuda.current_stream().cuda_stream -- NULL (0) is HIP's default stream,
 * which is what torch reports for its default stream: device-resident calls are then ordered with the caller's own kernels.
 * XDEMHIP_OWN_STREAM returns to the context's private non-blocking stream (the initial setting; host-buffer calls synchronise
 * it themselves). */
#define XDEMHIP_OWN_STREAM ((void*)(intptr_t)-1)
int xdemhip_set_stream(xdemhip_ctx* ctx, void* hip_stream);
int xdemhip_synchronize(xdemhip_ctx* ctx);
/* Device memory with a chosen PHYSICAL backing, for resident planes.  The streaming terrain kernel keeps
 * ~55 row streams going at once; in physically contiguous memory -- XDEMHIP_ALLOC_CONTIGUOUS, or an ordinary allocation on a box
 * whose free memory is one block -- they collide in the memory channels (14.4-15.6 ms for the 40000^2 set), in memory whose
 * pieces are scattered they do not (12.7-13.3 ms).  XDEMHIP_ALLOC_SCATTERED is the form to use: one virtual range over 32 MiB
 * physical pieces mapped in a fixed pseudo-random order (HIP virtual memory management).  `flags` = 0: hipMalloc.
 * XDEMHIP_ALLOC_CONTIGUOUS (hipExtMallocWithFlags / hipDeviceMallocContiguous; *got_contiguous -- optional -- tells whether the
 * driver had one piece), XDEMHIP_ALLOC_RECYCLED (allocate, touch, free, allocate again), XDEMHIP_ALLOC_CHUNKED (64 MiB pieces in
 * order) exist for measurements.  xdemhip_device_free takes all of them. */
enum { XDEMHIP_ALLOC_CONTIGUOUS = 1, XDEMHIP_ALLOC_RECYCLED = 2, XDEMHIP_ALLOC_CHUNKED = 4, XDEMHIP_ALLOC_SCATTERED = 8 };
int xdemhip_device_alloc(xdemhip_ctx* ctx, size_t bytes, int flags, void** ptr, int* got_contiguous);
int xdemhip_device_free(xdemhip_ctx* ctx, void* ptr);
/* Timing of the work enqueued by the last call on the context stream, measured with hipEvents recorded on
 * that stream around the kernel launch(es); returns milliseconds in *ms (synchronises the stop event). */
int xdemhip_last_kernel_ms(xdemhip_ctx* ctx, float* ms);
/* Diagnostics: the shader clock WHILE other work runs.  Enqueues on `hip_stream` (a stream of the caller's, not the context's: the
 * point is to run next to the context's kernels) one wave that sleeps `sleeps` x 8128 shader clocks (about 3.4 us each at 2.4 GHz)
 * and writes to out_device[0..1] (device memory, 16 bytes) the ticks of the shader-clock counter and of the constant 100 MHz
 * counter it saw go by: clock in MHz = 100 x out[0] / out[1].  No profiler, no SMI, nothing synchronises.  (bench.py launches one
 * per timed step: the same binary runs the terrain launch at 12.7 ms on one box and 13.9 ms on the next, and only the clock under
 * load tells a power-managed part from a slow placement of the planes.) */
int xdemhip_clock_probe(xdemhip_ctx* ctx, void* hip_stream, int sleeps, uint64_t* out_device);
/* OPTIONS of a context (fourteen names; every one of them has a GPU test).  Switches that only choose between internal routes
 * which must agree -- for the route-agreement tests and for measurements -- are not options: include/xdemhip_test.h.
 *  Host-buffer terrain calls
 *   "host_chunk_mb"     device-memory budget (MiB) of one row chunk (0 = default 288): host rasters of any size stream through the
 *                       GPU in row chunks with the overlap the attributes need.
 *   "host_chunk_rows"   rows per chunk where that is FEWER than the budget gives (0 = from the budget; at least 64 are taken) -- what
 *                       the reference's tiled call takes from `mp_config.chunk_size` (xdem/terrain/terrain.py:412-466); chunked and
 *                       one-pass results are bit-identical.
 *   "host_copy_threads" threads (one HIP stream each) that move host-buffer rasters over PCIe, rows split among them (0 = default 8,
 *                       at most 16).
 *   "host_release"      (any value) frees the pinned staging buffers the context keeps between such calls.
 *  Terrain
 *   "terrain_math"      precision recipe of float32 -> float32 launches: 2 (default) lean tail -- float64 where terms cancel, float32
 *                       scale factors; 0 mixed tail -- float64 everywhere but the arcsines; 1 float64 attribute math (what every other
 *                       dtype pair always runs).  All three meet the 1e-6 bar of the reference fixtures.
 *   "terrain_nonfinite" which of the reference's two rules decides what +-Inf pixels do to the surface-fit attributes -- 0 (default) the
 *                       SciPy engine's: an output is NaN iff its full window holds a non-finite value (surfit.py:1185-1192); 1 the
 *                       Numba engine's (surfit.py:948-1088, 1270-1303): no mask, the float64 loop over every tap and the formulas decide
 *                       (0 x Inf and Inf - Inf give NaN, other infinite windows give slope 90 deg etc.).  NaN pixels and raster edges
 *                       behave alike under both.
 *  Conventions of the third-party packages that nothing readable offline pins (oracle/pin_thirdparty.py decides them where the
 *  packages are importable; xdem_amd/thirdparty_decision.json then sets every context's defaults)
 *   "nk_nan_rule"       how nodata spreads through the bilinear taps of the Nuth-Kaab step / translation resample (geoutils'
 *                       _interp_points): 0 "4tap" (default; NaN if any of the four taps is non-finite or outside, zero weights included --
 *                       except a zero-weight tap beyond the last row / column, so a node exactly on the upper edge keeps its value), 1
 *                       "weighted" (zero-weight taps ignored everywhere), 2 "dilate3x3" (NaN if the 3 x 3 neighbourhood of the nearest
 *                       pixel holds a non-finite value), 3 "dilate_cross" (the same with the 4-connected cross: SciPy's default
 *                       binary-dilation structure).  Read when a plan is created / a resample is launched.
 *   "vario_edge"        lag classes of the pair kernels, 0 = [e_{k-1}, e_k) (default), 1 = (e_{k-1}, e_k].
 *   "vario_diff"        |dv| formed 0 = in the value dtype (default), 1 = in float64 (float32 values widened at xdemhip_pairs_create).
 *  Exact order statistics and the Nuth-Kaab step (results are identical under every value; tests hold the routes against each other)
 *   "selection"         how the exact medians (nanmedian of dh, aspect-bin and nd_binning medians, NMAD, Dowd) are selected -- 0 (default)
 *                       bracketed for large inputs: brackets from a ~1/64 sample, one counting + compaction pass, exact selection among
 *                       the candidates, plain radix passes if a bracket misses or the input is too small per bin; 1 plain 8-bit radix
 *                       passes only (the fall-back, and the check of the other); 2 degenerate brackets (exercises the fall-back); 3
 *                       bracketed even where the per-bin sample is small.
 *   "nk_fused"          1 (default) the Nuth-Kaab step of large plans is ONE data pass (13 B/pixel), 0 the plain route (stored dh and selections
 *                       over it: what a one-pass step hands over to when a bracket misses or a buffer overflows).
 *   "nk_fused_dist"     1 (default) partitioned plans (reduction hook + xdemhip_set_rank) take the one-pass step too, 0 the plain route.
 *   "nk_predict"        1 (default) a settled one-pass step takes its brackets from the previous step's exact medians (see
 *                       xdemhip_nk_predict_counts), 0 every step samples.
 *   "pairs_launch_cap"  workgroups per launch of the variogram pair passes (0 = default 2^31 / workgroup size, the most a HIP dispatch
 *                       holds; a pass over more tiles goes out as several launches -- a small value exercises that path) and of the
 *                       pair passes of CPD's E-step (0 = default: launches of at most 2^32 pair evaluations, 2^24 / slice length
 *                       workgroups); the cut changes neither the layout of the partials nor a bit of the results. */
int xdemhip_set_option(xdemhip_ctx* ctx, const char* name, int value);

/* Multi-GPU hook for the accumulator-style paths (Nuth-Kaab reductions): one process per GPU, every rank works on its
 * share and calls the same entry points; wherever a global reduction is needed the library hands a small HOST array of
 * `count` 8-byte elements to `fn`, which must combine it in place over all ranks (e.g. torch.distributed.all_reduce over
 * RCCL) and return 0.  kind: 0 = sum of uint64, 1 = sum of float64, 2 = min of uint64, 3 = max of uint64.  Integer
 * histograms / counts make the reductions exact and order-independent.  fn == NULL restores single-process behaviour. */
enum { XDEMHIP_RED_SUM_U64 = 0, XDEMHIP_RED_SUM_F64 = 1, XDEMHIP_RED_MIN_U64 = 2, XDEMHIP_RED_MAX_U64 = 3 };
typedef int (*xdemhip_allreduce_fn)(void* host_array, int64_t count, int kind, void* user);
int xdemhip_set_allreduce(xdemhip_ctx* ctx, xdemhip_allreduce_fn fn, void* user);
/* Device-side form of the same hook (round 3): the library's per-pass reductions (integer histograms, counters, min / max
 * keys) live in DEVICE memory; with this hook installed next to the host one they are handed over as they are -- `fn` gets
 * the device pointer and the hipStream_t (as void*) the library's work is queued on, must ENQUEUE the in-place all-reduce so
 * that it is ordered after the work already on that stream and before whatever is queued next (RCCL: ncclAllReduce on that
 * stream, or on another one bracketed by events), and returns without waiting: no D2H / H2D staging, no host
 * synchronisation per reduction.  The host hook stays in use for the few host-side scalars (route agreements).  NULL
 * removes it (every reduction is then staged through the host hook).  xdemhip_reduction_calls reports how many reductions
 * went through each hook since the context was created. */
typedef int (*xdemhip_allreduce_device_fn)(void* device_array, int64_t count, int kind, void* hip_stream, void* user);
int xdemhip_set_allreduce_device(xdemhip_ctx* ctx, xdemhip_allreduce_device_fn fn, void* user);
int xdemhip_reduction_calls(xdemhip_ctx* ctx, int64_t* host_calls, int64_t* device_calls);
/* ---- host-side preparation of the variogram path in native code (no context, no GPU: plain C++ on `threads` host threads) ----------
 * xdem's default sampler of raster variograms is scikit-gstat's RasterEquidistantMetricSpace (xdem/spatialstats.py:1185-1260; un-vendored):
 * per run a random centre, a centre disk and rings whose radii grow by sqrt(2), up to `samples` pixels of each, every centre-disk pixel
 * paired with every ring pixel.  xdemhip_host_ring_sample draws, for `runs` centres (cx, cy: pixel column / row) and `n_rings` rings
 * ring_lo[k] <= d < ring_hi[k] (distances in units of gsd x pixels, float64 arithmetic as NumPy forms them), up to `samples` distinct
 * pixels of every ring uniformly without replacement -- valid[iy * nx + ix] != 0 only, if `valid` is given -- as flat indexes iy * nx + ix
 * into out_idx[run][ring][0 .. out_count[run][ring]) (padded with -1; a ring that holds no more than `samples` pixels is returned whole,
 * in raster order, any other in random order).  Every (run, ring) has its own random stream derived from `seed`: the result does not
 * depend on `threads`.  Returns XDEMHIP_OK / XDEMHIP_EINVAL. */
int xdemhip_host_ring_sample(const uint8_t* valid, int64_t ny, int64_t nx, double gsd, int64_t runs, const int64_t* cx, const int64_t* cy,
                             int n_rings, const double* ring_lo, const double* ring_hi, int64_t samples, uint64_t seed, int threads,
                             int64_t* out_idx, int64_t* out_count);
/* Coordinates (x = ix gsd, y = iy gsd, float64) and values (`dtype` XDEMHIP_F32 / XDEMHIP_F64, gathered from the row-major raster
 * `values` with `nx` columns) of `n_blocks` point sets given as flat pixel indexes idx[off[b] .. off[b + 1]), in the order given (x_out,
 * y_out, v_out) and -- if sx_out is not NULL -- once more with every set permuted into Z-order over its own bounding box (sx_out, sy_out,
 * sv_out: the slot order the pair kernels' run-length accumulation wants). */
int xdemhip_host_gather_points(const void* values, int dtype, int64_t nx, double gsd, int n_blocks, const int64_t* off, const int64_t* idx,
                               int threads, double* x_out, double* y_out, void* v_out, double* sx_out, double* sy_out, void* sv_out);
/* np.isfinite(values) over a host array of gigabytes on `threads` threads (the first thing sample_empirical_variogram does with its
 * raster, xdem/spatialstats.py:1404-1410: the NaN filter of its values): the number of finite elements, and -- if valid_out is not
 * NULL -- the 0 / 1 mask itself (a caller whose raster turns out to be all finite never needs one). */
int xdemhip_host_count_finite(const void* values, int dtype, int64_t n, int threads, int64_t* n_finite, uint8_t* valid_out);
/* This process's place among the ranks the hooks reduce over (round 5).  The hooks only combine; a few exchanges of the one-pass
 * Nuth-Kaab step on partitioned plans need every rank's contribution SEPARATELY (per-rank histogram rows, per-rank slices of a small
 * key list): they travel as sum all-reduces in which every rank fills its own slot and adds zeros to the others', for which the
 * library must know `rank` in [0, `world`).  world = 0 (default) = not told: partitioned plans keep the plain route.  Ranks
 * must be numbered the same way on every process of the group (torch.distributed's group rank does). */
int xdemhip_set_rank(xdemhip_ctx* ctx, int rank, int world);

/* ---- path 1: terrain stencil engine --------------------------------------------------------------
 * Replaces  _get_surface_attributes(dem, resolution, surface_attributes, out_dtype, surface_fit,
 *           curv_method, engine, hillshade_*)                       xdem/terrain/surfit.py:1197-1305
 *      and  _get_windowed_indexes(dem, window_size, windowed_indexes, resolution, out_dtype, tri_method,
 *           engine) for TPI / TRI                                   xdem/terrain/window.py:926-1002
 *      plus the unit conversion / clip of _get_terrain_attribute     xdem/terrain/terrain.py:586-596
 * in ONE fused pass: one DEM read, one write per requested attribute.
 *
 *  dem          first row of the buffer.  Output row r (0 <= r < H) is buffer row (halo_top + r); the
 *               buffer holds halo_top + H + halo_bottom rows.  Halo rows are neighbour data of a
 *               row-block partition (multi-GPU); rows beyond them count as outside the raster (NaN), as
 *               do columns outside [0, W).  Single raster: halo_top = halo_bottom = 0.
 *  attr_mask    OR of XDEMHIP_ATTR_*; out_planes[k] receives the k-th SET bit in ascending bit order,
 *               each an (H, W) plane with row stride W in out_dtype.
 *  degrees      bit 0: slope / aspect in degrees (terrain.py:586-591), else radians.  Bit 1 (value 2, or 3 with degrees): the
 *               hillshade plane as the reference's ENGINE returns it (surfit.py:609-622), WITHOUT the caller's clip to [0, 255]
 *               (terrain.py:594-596) that every other call fuses -- for bindings at the engine boundary
 *               (_get_surface_attributes); such a launch takes the float64 attribute tail.
 *  window_size  odd window of TPI / TRI / roughness (reference default 3) and of fractal roughness (reference default
 *               13 through its own window_size_fractal: request that attribute in a call of its own); rugosity is 3x3.
 * NaN / +-Inf in the DEM are nodata: an output pixel is NaN iff its full window (3x3 Horn/ZT, 5x5
 * Florinsky; window_size for TPI/TRI) holds a non-finite value or leaves the raster (surfit.py:1185-1192).
 */
int xdemhip_terrain(xdemhip_ctx* ctx, const void* dem, int dem_dtype, int64_t H, int64_t W, int64_t row_stride,
                    int64_t halo_top, int64_t halo_bottom, double resolution, int surface_fit, int curv_method,
                    uint32_t attr_mask, int tri_method, int window_size, double hillshade_altitude_deg,
                    double hillshade_azimuth_deg, double hillshade_z_factor, int degrees, int out_dtype,
                    void* const* out_planes, int memspace);

/* Host-only helper (no GPU needed): the regression abscissae of fractal roughness for a window size, with NumPy's
 * float16 arithmetic reproduced (xdem/terrain/window.py:362-393: the divisors q of window_size//2 are a uint8 array, so
 * np.log / np.mean / SS_xx are float16).  Fills q[], log_q[] (float16 values as double) and returns the number of
 * divisors (<= max_q), or a negative status. */
int xdemhip_fractal_constants(int window_size, int max_q, int* q, double* log_q, double* mean_log_q, double* ss_xx);

/* Texture shading, the frequency-domain attribute of get_terrain_attribute: replaces
 *   _texture_shading_fft(dem, alpha)   xdem/terrain/freq.py:63-148   (called at xdem/terrain/terrain.py:637-644)
 * non-finite pixels are filled with the NaN-ignoring mean, the raster is padded symmetrically to the next 2/3/5/7-smooth
 * size, multiplied by |f|^alpha in the frequency domain (DC zeroed when alpha > 0) and cropped; invalid pixels -> NaN.
 * 0 <= alpha <= 2.  The FFT itself is hipFFT's (loaded on first use), in the DEM's precision like scipy.fft. */
int xdemhip_texture_shading(xdemhip_ctx* ctx, const void* dem, int dem_dtype, int64_t H, int64_t W, double alpha, int out_dtype,
                            void* out, int memspace);

/* ---- path 2: Nuth & Kaab (2011) inner loop ------------------------------------------------------------
 * Replaces the array work of  nuth_kaab(ref_elev, tba_elev, inlier_mask, transform, ...)   xdem/coreg/affine.py:539-609
 * for two rasters on the same grid, i.e. what NuthKaab._fit_rst_rst reaches (affine.py:2458-2522):
 *
 *  xdemhip_nk_create   once per fit: slope tangent / aspect from np.gradient (affine.py:433-438), zero slopes -> NaN
 *                      (affine.py:578-579), valid = inlier & finite(ref, tba, slope_tan, aspect) (base.py:650-661);
 *                      *n_valid = number of valid pixels (the reference's `subsample_final` for subsample == 1).
 *  xdemhip_nk_step     one _nuth_kaab_iteration_step (affine.py:477-536) up to, not including, the 72-point curve
 *                      fit: for the current offsets (georeferenced units, east / north)
 *                        dh      = ref - bilinear(tba)(row - shift_y/res_y, col + shift_x/res_x)     [convention: DESIGN.md]
 *                        vshift  = np.nanmedian(dh)                          (exact, radix selection)
 *                        y       = (dh - vshift) / slope_tan,  y_mean / y_std = np.nanmean / np.nanstd (for p0)
 *                        edges[n_bins+1], counts[n_bins], medians[n_bins] = scipy.stats.binned_statistic(aspect, y,
 *                                  np.nanmedian, bins=n_bins) with 'count'      (xdem/spatialstats.py:143-157)
 *                      Empty bins give NaN medians.  Returns XDEMHIP_EINVAL ("The subsample contains no more valid
 *                      values.") when no pixel survives, like affine.py:510-515.
 *  xdemhip_binned_median  the binning alone on caller-supplied 1-D (x, y) host arrays (nd_binning, 1 variable).
 * Host code fits a*cos(b - x) + c to (bin mids, medians) with scipy.optimize.curve_fit exactly as base.py:1038-1045.
 */
typedef struct xdemhip_nk_plan xdemhip_nk_plan;
int xdemhip_nk_create(xdemhip_ctx* ctx, const void* ref, const void* tba, const uint8_t* inlier_mask_or_null, int dtype,
                      int64_t H, int64_t W, int memspace, xdemhip_nk_plan** out_plan, int64_t* n_valid);
int xdemhip_nk_step(xdemhip_nk_plan* plan, double shift_x, double shift_y, double res_x, double res_y, int n_bins,
                    double* vshift, int64_t* n_valid, double* y_mean, double* y_std, double* edges, int64_t* counts,
                    double* medians);
/* Multi-GPU, partitioned (the production layout; structural ancestor: xdem/coreg/blockwise.py:174): this rank holds only
 * raster rows [row_begin - halo_top, row_end + halo_bottom) of ref / tba / inlier mask -- its own row block plus halo rows
 * copied from the neighbours (xdem_amd.dist.RowBlock exchanges them over RCCL send / recv).  The gradient needs ONE halo
 * row; the bilinear taps of a step need floor(|shift_y / res_y|) + 1 more, so the halo bounds the vertical shift a fit may
 * reach: xdemhip_nk_step returns XDEMHIP_EINVAL ("halo too small ...") when a step would leave it, and the caller
 * re-creates the plan with a deeper halo.  Install the all-reduce hook (and xdemhip_set_rank) BEFORE this call: n_valid is the
 * global count, and every reduction of a step (histograms, counters, min / max keys, successor keys) goes through the hook. */
int xdemhip_nk_create_block(xdemhip_ctx* ctx, const void* ref_block, const void* tba_block, const uint8_t* inlier_block_or_null,
                            int dtype, int64_t H, int64_t W, int64_t row_begin, int64_t row_end, int64_t halo_top,
                            int64_t halo_bottom, int memspace, xdemhip_nk_plan** out_plan, int64_t* n_valid);
/* Multi-GPU, replicated (every rank holds the full ref / tba): restrict this rank's work to raster rows
 * [row_begin, row_end); the streaming passes and their histograms are sharded by row block and combined through the
 * all-reduce hook.  Call right after xdemhip_nk_create on every rank; n_valid then returns the global count. */
int xdemhip_nk_set_rows(xdemhip_nk_plan* plan, int64_t row_begin, int64_t row_end, int64_t* n_valid);
/* Debug / test access: copy the auxiliary rasters back to host buffers (any pointer may be NULL). */
/* Statistic of the aspect bins (NuthKaab(bin_statistic=...), xdem/coreg/affine.py:2404): XDEMHIP_BINSTAT_MEDIAN (default,
 * np.nanmedian -- exact selection) or XDEMHIP_BINSTAT_MEAN (np.nanmean: per-bin float64 sums and counts in one pass, sum-
 * reducible across GPUs; equals NumPy's float32 pairwise mean to rounding, not bit for bit).  xdemhip_nk_step then returns
 * the bin means in `medians`. */
/* NuthKaab(bin_before_fit=False) (the mode of the reference's own synthetic tests, tests/test_coreg/test_affine.py:163-239):
 * the step without binning.  curve_fit then runs on every valid point (xdem/coreg/base.py:975-989); the model
 * a cos(b - x) + c is linear in (a cos b, a sin b, c), so its optimum follows from ten float64 sums over the points --
 * sums = [n, S cos x, S sin x, S cos^2, S sin^2, S cos sin, S y, S y cos, S y sin, S y^2] with x = aspect, y = (dh - vshift) /
 * slope_tan widened to float64 like curve_fit widens its inputs -- which is what this entry returns next to vshift,
 * n_valid and the p0 ingredients (np.nanmean / np.nanstd of y). */
int xdemhip_nk_step_fit(xdemhip_nk_plan* plan, double shift_x, double shift_y, double res_x, double res_y, double* vshift,
                        int64_t* n_valid, double* y_mean, double* y_std, double* sums /* [10] */);
/* NuthKaab(bin_statistic=<a callable other than np.nanmedian / np.nanmean>) (xdem/coreg/affine.py:2404; nd_binning hands the callable to
 * scipy.stats.binned_statistic, xdem/spatialstats.py:143-157): host code cannot run on the GPU, so this entry returns what the callable is
 * applied to -- y = (dh - vshift) / slope_tan in the DEM dtype and the aspect-bin id (uint16; 0xFFFF = no bin) of every pixel of the raster
 * in raster order, NaN / 0xFFFF where the pixel has no dh at this shift -- next to vshift, the valid count, np.nanmean / np.nanstd of y and
 * the n_bins + 1 bin edges.  `y_out` holds H x W values of the plan's dtype, `bins_out` H x W uint16, both in `memspace`.  Whole-raster
 * plans without a reduction hook only (a partitioned plan holds a part of every bin: XDEMHIP_EINVAL); the step takes the plain route. */
int xdemhip_nk_step_values(xdemhip_nk_plan* plan, double shift_x, double shift_y, double res_x, double res_y, int n_bins, double* vshift,
                           int64_t* n_valid, double* y_mean, double* y_std, double* edges /* [n_bins + 1] */, void* y_out,
                           uint16_t* bins_out, int memspace);
/* Explicit aspect-bin edges (NuthKaab(bin_sizes={"aspect": edges}), the array form of scipy.stats.binned_statistic's `bins`):
 * n_edges increasing values (2 .. 129: at most 128 bins, one histogram sweep); xdemhip_nk_step must then be called with
 * n_bins = n_edges - 1 (its output arrays are sized by n_bins; any other value is XDEMHIP_EINVAL).  `decimal` = SciPy's
 * `int(-log10(min edge spacing)) + 6` for these edges in the sample dtype (its rule for samples at or beyond the rightmost
 * edge, _binned_statistic.py:_bin_numbers).  n_edges = 0 restores SciPy's automatic edges. */
int xdemhip_nk_set_bin_edges(xdemhip_nk_plan* plan, const double* edges, int n_edges, int decimal);
#define XDEMHIP_BINSTAT_MEDIAN 0
#define XDEMHIP_BINSTAT_MEAN 1
int xdemhip_nk_set_statistic(xdemhip_nk_plan* plan, int bin_stat);
int xdemhip_nk_get_aux(xdemhip_nk_plan* plan, void* slope_tan, void* aspect, uint8_t* valid);
/* The random subsample of the valid pixels (replaces the host round trip of _get_subsample_on_valid_mask, xdem/coreg/base.py:577-617,
 * whose draw is `rng.choice(np.flatnonzero(valid), k, replace=False)` = flatnonzero(valid)[rng.choice(n_valid, k, replace=False)]): the
 * caller draws `k` distinct RANKS in [0, n_valid) -- positions among the plan's valid pixels in raster order -- and the plan keeps
 * exactly those pixels as inliers (the valid mask never travels to the host; rasters and aux variables stay where they are; a second
 * call draws again among the pixels still valid).  `ranks`: int64, host or device (`memspace`).  Whole-raster plans of one process
 * only (XDEMHIP_EINVAL otherwise: partitioned plans pass the drawn mask as their inlier mask).  n_valid returns the new count (= k). */
int xdemhip_nk_subsample(xdemhip_nk_plan* plan, const int64_t* ranks, int64_t k, int memspace, int64_t* n_valid);
/* How the steps of this plan were answered so far (either pointer may be NULL).  Two routes since round 6:
 *   ONE-PASS  one data pass of 13 B/pixel -- the shifted elevation difference, the counting for its exact median and the
 *             aspect-bin counting against brackets with per-pixel margins (large plans, median statistic, context option
 *             "nk_fused" = 1, the default); around it per-bin candidate segments with one workgroup per bin, a value-bucket
 *             selection of the median of dh, sample passes that advance their own selection states: 24 launches per step with
 *             sampled brackets, 14 with predicted ones (option "nk_predict");
 *   PLAIN     dh written by a generic kernel that reads mask and aspect, then the selections of select_run.h over the stored
 *             arrays (bracketed where the size pays, plain digit passes otherwise): small rasters, the mean statistic, the
 *             un-binned fit, "nk_fused" = 0, and the fall-back of a one-pass step whose brackets missed or overflowed.
 * (The queued two-pass route of rounds 2-5 is retired: no plan needed it.)  Results are identical on both routes (integer
 * counts, exact selections); nanmean / nanstd of y -- the p0 of the curve fit -- agree to 2e-6 of the spread on the one-pass
 * route (float32 partial sums, the accuracy class of the reference's own float32 np.nanmean).
 * PARTITIONED plans (reduction hook installed, xdemhip_set_rank told, context option "nk_fused_dist" = 1, the default) take the
 * one-pass step as well: one data pass over the rank's own rows and ten all-reduces per sampled step, five per predicted one
 * (nuthkaab.hip: "the ONE-PASS step on PARTITIONED plans"), all of them enqueued through the device hook where it is installed;
 * every rank returns the same integers as a single-GPU fit of the whole rasters. */
int xdemhip_nk_route_counts(xdemhip_nk_plan* plan, int64_t* onepass, int64_t* plain);
/* Round 6: how many of the one-pass steps took PREDICTED brackets -- the previous step's exact medians moved by the Nuth-Kaab
 * model for the change of the shift, instead of brackets from a fresh 1/64 sample: no sample kernels and no digit passes over
 * samples on a settled fit (context option "nk_predict", default 1; 0 = every step samples) --, how many predicted only the bracket
 * of the median of dh (steps that still move too far for the bins: the dh sample's three digit passes are skipped, the bins'
 * brackets are sampled), and how many predictions missed (such a step is run again with sampled brackets: the integers returned
 * are the same either way). */
int xdemhip_nk_predict_counts(xdemhip_nk_plan* plan, int64_t* predicted, int64_t* predicted_dh_only, int64_t* missed);
void xdemhip_nk_destroy(xdemhip_nk_plan* plan);
int xdemhip_binned_median(xdemhip_ctx* ctx, const void* x, const void* y, int dtype, int64_t n, int n_bins, double* edges,
                          int64_t* counts, double* medians);

/* ---- bias corrections: Deramp and VerticalShift (elevation difference of two rasters on one grid) ----------------------------
 * Replaces the array work of
 *   Deramp._fit_rst_rst -> _bin_or_and_fit_nd("fit")   xdem/coreg/biascorr.py:195, 621-745; base.py:978-985
 *       curve_fit(polynomial_2d, (xx, yy), ref - tba, p0=ones((order+1)^2)) over the valid pixels: here the least-squares moments
 *   Deramp._apply_rst                                    biascorr.py:262-311 (+ the cast of base.py:491): xdemhip_poly2d_apply
 *   vertical_shift(..., vshift_reduc_func=np.median)     xdem/coreg/affine.py:721-770: xdemhip_dh_median
 * A dh plan holds ref, tba (H x W, `dtype`) and an optional inlier mask (0 / 1 bytes), in `memspace` like xdemhip_nk_create:
 *
 *  xdemhip_dh_create        valid = inlier & isfinite(ref) & isfinite(tba) (base.py:652-663); *n_valid = its count.
 *  xdemhip_dh_subsample     the random subsample (base.py:577-617): the caller draws `k` distinct RANKS among the valid pixels in
 *                           raster order (xdem_amd.coreg.subsample_ranks), the plan keeps those pixels -- flatnonzero(valid)[ranks] --
 *                           as its selection for every later call; *n_drawn = their number.  The same tile count -> scan -> rank
 *                           selection as xdemhip_nk_subsample (one implementation: xdem_amd/csrc/rank_select.h).
 *  xdemhip_dh_poly_moments  least-squares sums of the tensor-product polynomial sum c[i, j] x^i y^j (xdem/fit.py:127-149; x = column,
 *                           y = row_offset + row) over the selected pixels, in normalised coordinates u = (x - cx) / sx, v = (y - cy) / sy,
 *                           cx = sx = (W_global - 1) / 2, cy = sy = (H_global - 1) / 2 (a half-width of 0 counts as 1):
 *                             m_out[a * (2 order + 1) + b] = sum u^a v^b      (a, b <= 2 order)
 *                             r_out[i * (order + 1) + j]   = sum dh u^i v^j   (i, j <= order)
 *                           dh = ref - tba rounded in the input dtype, all sums float64, partials added in a fixed order (the same bits
 *                           every call); *count = the number of selected pixels.  order 0..5.  A plan over raster rows
 *                           [row_offset, row_offset + H) of an H_global x W grid returns sums that add up over row blocks.
 *  xdemhip_dh_median        np.median(dh) over the selected pixels, exact, in the value dtype (radix selection; mean of the two middle
 *                           values in the value dtype for an even count), and the count.
 *  xdemhip_dh_values        dh (plan dtype) and the column / row index (int64) of every selected pixel, in raster order (any output may
 *                           be NULL; each holds *count elements -- n_valid, or n_drawn after a subsample): what a host callable receives.
 *  xdemhip_dh_shift_nmad    the objective of DhMinimize (xdem/coreg/affine.py:617-674) at one trial shift: for every selected pixel (r, c)
 *                           dh = ref[r, c] - bilinear(tba)(r - shift_y / res_y, c + shift_x / res_x), with the taps and the nodata rule of
 *                           the Nuth-Kaab step (option "nk_nan_rule"; float64 weights, the interpolated value rounded to the raster
 *                           dtype, the difference taken in it); pixels whose interpolated value is NaN drop out.  *count = the number
 *                           left, *median = np.nanmedian(dh) (exact; mean of the two middle values in the value dtype for an even
 *                           count), *nmad = (T)nfact * np.nanmedian(|dh - median|) rounded as xdemhip_nmad rounds it.  One pass over the
 *                           rasters per call; both selections read the plan's staging copy of dh, and their results come back in one
 *                           fetch.  The plan keeps the buffers from the first call on.  Single-process plans: a reduction hook on the
 *                           context is suspended for the call.
 *  xdemhip_dh_shift_values  the same dh of every selected pixel in raster order (plan dtype, NaN kept where the interpolation is NaN):
 *                           what any other loss function receives; *count = the number of selected pixels, as xdemhip_dh_values.
 * Every entry returns XDEMHIP_EINVAL ("no valid points") where nothing is selected (xdemhip_dh_shift_nmad: where nothing is left). */
typedef struct xdemhip_dh_plan xdemhip_dh_plan;
int xdemhip_dh_create(xdemhip_ctx* ctx, const void* ref, const void* tba, const uint8_t* inlier_mask_or_null, int dtype, int64_t H, int64_t W,
                      int memspace, xdemhip_dh_plan** out_plan, int64_t* n_valid);
int xdemhip_dh_subsample(xdemhip_dh_plan* plan, const int64_t* ranks, int64_t k, int memspace, int64_t* n_drawn);
int xdemhip_dh_poly_moments(xdemhip_dh_plan* plan, int order, int64_t row_offset, int64_t H_global, int64_t W_global, double* m_out,
                            double* r_out, int64_t* count);
int xdemhip_dh_median(xdemhip_dh_plan* plan, double* median, int64_t* count);
int xdemhip_dh_values(xdemhip_dh_plan* plan, void* dh_out, int64_t* col_out, int64_t* row_out, int memspace, int64_t* count);
int xdemhip_dh_shift_nmad(xdemhip_dh_plan* plan, double shift_x, double shift_y, double res_x, double res_y, double nfact, double* median,
                          double* nmad, int64_t* count);
int xdemhip_dh_shift_values(xdemhip_dh_plan* plan, double shift_x, double shift_y, double res_x, double res_y, void* dh_out, int memspace,
                            int64_t* count);
void xdemhip_dh_destroy(xdemhip_dh_plan* plan);

/* ---- bias corrections with variables: BiasCorr, DirectionalBias, TerrainBias (csrc/bincorr.hip) --------------------------------
 * The raster passes of xdem.coreg.BiasCorr / DirectionalBias / TerrainBias (xdem/coreg/biascorr.py:40-618) for two rasters on one
 * grid.  A variable of a correction is described by its SOURCE, so that the two variables upstream materialises as whole-raster
 * planes -- the rotated coordinate of DirectionalBias, the elevation of TerrainBias("elevation") -- are formed per pixel instead:
 *   XDEMHIP_VAR_PLANE    `plane`: H x W values (`dtype` float32 / float64) in the call's memspace;
 *   XDEMHIP_VAR_ROTATED  the along-track coordinate of a north-up grid, float64, every operation rounded on its own:
 *                          x = (col * res_x) * cos_t + ((H - 1 - row) * res_y) * sin_t - offset
 *                        (xdem_amd.bincorr.rotated_x is the same arithmetic on the host);
 *   XDEMHIP_VAR_REF      the reference raster of the plan (xdemhip_corr_apply: the raster `elev` itself), in the raster dtype;
 *   XDEMHIP_VAR_TBA      the to-be-aligned raster of the plan (xdemhip_dh_var_columns only).
 *
 *  xdemhip_dh_restrict_finite  narrows the plan's valid mask by isfinite(var) for a plane on the plan's grid -- upstream's valid mask
 *                              of a bias correction is inlier & finite(ref) & finite(tba) & finite(every variable) (base.py:653-661),
 *                              and the subsample ranks are drawn among exactly those pixels; *n_valid = the new count.  Only before
 *                              xdemhip_dh_subsample or any call that lists the valid pixels: XDEMHIP_EINVAL afterwards.
 *  xdemhip_dh_var_columns      for the selected pixels in raster order: dh (plan dtype) and the value of each of the n_var (<= 8)
 *                              variables as columns of *count elements -- a plane's values in the plane's dtype, the rotated
 *                              coordinate in float64, ref / tba in the plan dtype.  With XDEMHIP_DEVICE the columns are what
 *                              xdemhip_binstats_create / _add_var take, without a host round trip (planes are then device planes too).
 *  xdemhip_corr_apply          out = (raster dtype)((double)elev + corr(variables)) in one pass over the raster, corr being
 *     XDEMHIP_CORR_GRID    the multilinear interpolant of xdemhip_interp_grid_linear (same code, same bits): n_tab[d] = points of
 *                          axis d, `a` = the axes concatenated, `table` = the grid values in C order; 1 to 3 variables;
 *     XDEMHIP_CORR_PERBIN  the lookup of xdemhip_perbin_lookup for disjoint intervals (same code): n_tab[d] = intervals of variable
 *                          d, `a` / `b` = their left / right ends concatenated, `table` / `pass` over their product;
 *                          *n_missing = pixels in a bin of kind 2; 1 to 3 variables;
 *     XDEMHIP_CORR_POLY    sum c_i x^i by Horner's rule in float64 as np.polynomial.polynomial.polyval evaluates it
 *                          (c0 = c[n-1] + x * 0, then c0 = c[n-i] + c0 * x); n_tab[0] = n <= 64, `table` = c; one variable;
 *     XDEMHIP_CORR_SUMSIN  sum_k a_k sin(2 pi / b_k x + c_k), float64, terms added in index order (xdem/fit.py:87-112);
 *                          n_tab[0] = 3 K <= 192, `table` = (a_0, b_0, c_0, a_1, ...); one variable.
 *                          The tables are small and live in LDS: more than 3072 table entries (bins, or grid points) are refused
 *                          with XDEMHIP_EINVAL.  float32 variables are widened to float64 first, as NumPy does. */
enum { XDEMHIP_VAR_PLANE = 0, XDEMHIP_VAR_ROTATED = 1, XDEMHIP_VAR_REF = 2, XDEMHIP_VAR_TBA = 3 };
enum { XDEMHIP_CORR_GRID = 0, XDEMHIP_CORR_PERBIN = 1, XDEMHIP_CORR_POLY = 2, XDEMHIP_CORR_SUMSIN = 3 };
typedef struct xdemhip_varsrc {
    int kind;           /* XDEMHIP_VAR_* */
    int dtype;          /* XDEMHIP_VAR_PLANE: XDEMHIP_F32 / XDEMHIP_F64 */
    const void* plane;  /* XDEMHIP_VAR_PLANE */
    double cos_t, sin_t, res_x, res_y, offset;   /* XDEMHIP_VAR_ROTATED */
} xdemhip_varsrc;
int xdemhip_dh_restrict_finite(xdemhip_dh_plan* plan, const void* var, int dtype, int memspace, int64_t* n_valid);
int xdemhip_dh_var_columns(xdemhip_dh_plan* plan, int n_var, const xdemhip_varsrc* vars, void* dh_out, void* const* var_out, int memspace,
                           int64_t* count);
int xdemhip_corr_apply(xdemhip_ctx* ctx, const void* elev, int dtype, int64_t H, int64_t W, int kind, int n_var, const xdemhip_varsrc* vars,
                       const int* n_tab, const double* a, const double* b, const double* table, const unsigned char* pass, void* out,
                       int64_t* n_missing, int memspace);

/* ---- rigid coregistration: LZD and the rotation-capable raster apply (csrc/rigid.hip) ------------------------------------------
 * The grid passes of xdem.coreg.LZD (Rosenholm & Torlegard 1988; xdem/coreg/affine.py:1417-1776) on a dh plan, and
 * _iterate_affine_regrid_small_rotations (xdem/coreg/base.py:1389-1519) for resampling="linear".
 * `transform6` = the north-up geotransform (a, b, c, d, e, f) with b = d = 0: pixel (row, col) has its centre at
 * x = c + (col + 0.5) a, y = f + (row + 0.5) e.  `matrix16` = a 4 x 4 rigid matrix, row-major, last row (0, 0, 0, 1);
 * p' = M (p - centroid) + centroid, the products as explicit float64 sums m0 x + m1 y + m2 z + m3 without contraction.
 *  xdemhip_dh_lzd_gradients  gradx = gradient_x / res_x, grady = -gradient_y / res_y of np.gradient(ref) (affine.py:1440, 1455-1456) in the
 *                            raster dtype, the resolution taken to that dtype first; made at the first LZD call and kept by the plan.
 *                            Copies the two planes out (H * W values each).  The raster must be at least 2 x 2.
 *  xdemhip_dh_lzd_centroid   (mean x, mean y, mean tba) over the selected pixels (affine.py:1744-1746): integer sums of row and column,
 *                            the float64 sum of tba in a fixed order; *count = the selected pixels.
 *  xdemhip_dh_lzd_normal     one LZD iteration's normal equations.  Every selected pixel p = (x, y, tba) is moved by the matrix, ref, gradx
 *                            and grady are interpolated at its new position (row', col') = ((y' - f) / e - 0.5, (x' - c) / a - 0.5) with the
 *                            bilinear taps and the nodata rule of the Nuth-Kaab step (option "nk_nan_rule"), each rounded to the raster dtype;
 *                            dh = ref' - z'.  Pixels with a non-finite dh, z', gx or gy are dropped (affine.py:1640).  With (x, y, z) the moved
 *                            point minus the centroid, a = (-gx, -gy, 1, y + gy z, -x - gx z, gx y - gy x) (the derivatives of
 *                            affine.py:1496-1503 by t1, t2, t3, alpha1, alpha2, alpha3).  sums_out[29] = the 21 upper-triangle terms of
 *                            a a^T (row by row), the 6 of a dh, sum dh^2, sum dh, in float64: per-lane accumulators, one partial per
 *                            workgroup (in a buffer the plan keeps), partials added in a fixed order (two calls return the same bits), one
 *                            fetch.  *count = pixels kept.
 *  xdemhip_dh_lzd_values     what upstream hands _lzd_fit: x, y, z (centroid removed), dh, gradx, grady of the pixels kept, float64, raster
 *                            order.  `out` holds 6 rows of n values, n = the selected pixels (row k starts at out[k * n]); the first *count
 *                            entries of each row are filled.  `out` is host memory.
 *  xdemhip_apply_matrix_rst  the DEM seen after the rigid transform, resampled on its own grid: one thread per pixel runs upstream's
 *                            fixed-point iteration (first guess z of the pixel's own transformed point; inverse transform of (x, y, z_guess),
 *                            interpolation of dem there, forward transform to (x0, y0, z0); after iteration 1 the pixel keeps z0 if
 *                            |x0 - x| < 1e-4 res_x or is non-finite, and the same in y; otherwise it keeps z0 of iteration 5).  The
 *                            interpolation is SciPy's RegularGridInterpolator(method="linear", bounds_error=False): NaN outside the pixel
 *                            centres' extent and where any node of the cell is non-finite (a position exactly on row k lies in SciPy's cell of
 *                            rows [k - 1, k], one exactly on column k in the cell of columns [k, k + 1]).  The inverse is formed here as
 *                            R^T and -(R^T t); `centroid3_or_null`: no centroid is subtracted when null.  All float64,
 *                            result cast to `dtype`.  The raster must be at least 2 x 2. */
int xdemhip_dh_lzd_gradients(xdemhip_dh_plan* plan, const double* transform6, void* gradx_out, void* grady_out, int memspace);
int xdemhip_dh_lzd_centroid(xdemhip_dh_plan* plan, const double* transform6, double* centroid_out, int64_t* count);
int xdemhip_dh_lzd_normal(xdemhip_dh_plan* plan, const double* transform6, const double* matrix16, const double* centroid3, double* sums_out,
                          int64_t* count);
int xdemhip_dh_lzd_values(xdemhip_dh_plan* plan, const double* transform6, const double* matrix16, const double* centroid3, double* out,
                          int64_t* count);
int xdemhip_apply_matrix_rst(xdemhip_ctx* ctx, const void* dem, int dtype, int64_t H, int64_t W, const double* transform6, const double* matrix16,
                             const double* centroid3_or_null, void* out, int memspace);

/* ---- raster-point coregistration (csrc/ptsplan.hip) -------------------------------------------------------------------------------
 * NuthKaab, DhMinimize and VerticalShift when one elevation dataset is a point cloud (xdem/coreg/affine.py:150-243 with
 * base.py:624-706).  A raster-point plan holds one raster (H x W, `dtype`), an optional inlier mask (0 / 1 bytes), the north-up
 * `transform6` and the cloud's columns x, y (float64) and z (`dtype`), n_pts values each, all in `memspace`; `pts_is_ref` says which side
 * is the reference.  A point lies at (row, col) = ((y - f) / e - 0.5, (x - c) / a - 0.5), every float64 operation rounded on its own;
 * the raster is sampled there with the bilinear taps and the nodata rule of the Nuth-Kaab step (option "nk_nan_rule": float64 weights,
 * the value rounded to the raster dtype).
 *
 *  xdemhip_pts_create        the validity plane of the raster is inlier & isfinite(raster), with `with_nk_aux` also isfinite of the slope
 *                            tangent and the aspect, built as xdemhip_nk_create builds them.  A point is valid iff x, y, z are finite and
 *                            the tap rule accepts the validity plane -- 1 / NaN as float32 -- at its unshifted position
 *                            (base.py:679, 697-701).  *n_valid = their number; the selection is every valid point, in cloud order.  With
 *                            `with_nk_aux` slope tangent and aspect are interpolated at every point, once, at zero shift
 *                            (affine.py:234-239: the aspect plane as it is, its 0 / 2 pi jump included).
 *  xdemhip_pts_subsample     as xdemhip_dh_subsample: `k` distinct ranks among the valid points in cloud order; the selection becomes
 *                            flatnonzero(valid)[ranks], kept in cloud order.
 *  xdemhip_pts_selection     the cloud indexes of the selected points (host array of *count values; may be NULL for the count alone).
 *  xdemhip_pts_nk_step       one iteration of Nuth & Kaab at the offsets (shift_x, shift_y), in georeferenced units, over the selected
 *                            points: dh = z - raster(x + shift_x, y + shift_y) for a point reference, raster(x - shift_x, y - shift_y) - z
 *                            for a raster reference (affine.py:217-231), the difference taken in the raster dtype, non-finite values
 *                            dropped.  Outputs as xdemhip_nk_step: *vshift = np.nanmedian(dh) (exact), *n_valid = the points that have a dh,
 *                            y = (dh - vshift) / slope_tan, SciPy's automatic bin edges from the aspect of those points (or the explicit
 *                            ones), per-bin counts and exact medians, *y_mean / *y_std = np.nanmean / np.nanstd of y from float64 sums
 *                            added in a fixed order (the same bits every call).  One fetch per step.  XDEMHIP_EINVAL ("The subsample
 *                            contains no more valid values.") where no point is left.
 *  xdemhip_pts_step_y        the y column of the last xdemhip_pts_nk_step: one value per selected point in cloud order (raster dtype), NaN where
 *                            the point had no dh.  Upstream forms the start of its curve fit from np.nanmean(y) and np.nanstd(y) in y's own
 *                            dtype (affine.py:381-384), NumPy's pairwise sums, which no sum in another order reproduces to the bit; the
 *                            host takes them from this column.  XDEMHIP_EINVAL before a step or after the selection changed.
 *  xdemhip_pts_set_bin_edges as xdemhip_nk_set_bin_edges (NULL: automatic edges again); at most 1024 bins.
 *  xdemhip_pts_shift_nmad    as xdemhip_dh_shift_nmad with the dh above: median and NMAD at a trial shift, two exact selections, one fetch.
 *  xdemhip_pts_shift_values  the dh column of the selected points in cloud order, NaN kept, and (non-NULL outputs, `with_nk_aux` plans) their
 *                            slope tangent and aspect columns: what a host loss function or bin statistic receives.
 *  xdemhip_apply_matrix_pts  p' = M (p - centroid) + centroid for n points (float64 columns), the products as explicit sums
 *                            ((m0 x + m1 y) + m2 z) + m3 without contraction; no centroid is subtracted when it is NULL; `invert`: the
 *                            inverse R^T, -(R^T t) is formed first, as xdemhip_apply_matrix_rst forms it.
 * The gather of one evaluation walks the selected points in cloud order, or by raster tile of their unshifted position (test switch
 * "pts_tile_order", include/xdemhip_test.h); it writes dh at the point's own index and every later pass reads cloud order, so both
 * orders and every run return the same bits.  Single-process plans: a reduction hook on the context is suspended for the calls. */
typedef struct xdemhip_pts_plan xdemhip_pts_plan;
int xdemhip_pts_create(xdemhip_ctx* ctx, const void* raster, const uint8_t* inlier_mask_or_null, int dtype, int64_t H, int64_t W,
                       const double* transform6, const double* x, const double* y, const void* z, int64_t n_pts, int pts_is_ref, int with_nk_aux,
                       int memspace, xdemhip_pts_plan** out_plan, int64_t* n_valid);
int xdemhip_pts_subsample(xdemhip_pts_plan* plan, const int64_t* ranks, int64_t k, int memspace, int64_t* n_selected);
int xdemhip_pts_selection(xdemhip_pts_plan* plan, int64_t* idx_out_or_null, int64_t* count);
int xdemhip_pts_set_bin_edges(xdemhip_pts_plan* plan, const double* edges_or_null, int n_edges, int decimal);
int xdemhip_pts_nk_step(xdemhip_pts_plan* plan, double shift_x, double shift_y, int n_bins, double* vshift, int64_t* n_valid, double* y_mean,
                        double* y_std, double* edges, int64_t* counts, double* medians);
int xdemhip_pts_step_y(xdemhip_pts_plan* plan, void* y_out, int memspace, int64_t* count);
int xdemhip_pts_shift_nmad(xdemhip_pts_plan* plan, double shift_x, double shift_y, double nfact, double* median, double* nmad, int64_t* count);
int xdemhip_pts_shift_values(xdemhip_pts_plan* plan, double shift_x, double shift_y, void* dh_out, void* slope_out_or_null,
                             void* aspect_out_or_null, int memspace, int64_t* count);
void xdemhip_pts_destroy(xdemhip_pts_plan* plan);
int xdemhip_apply_matrix_pts(xdemhip_ctx* ctx, const double* x, const double* y, const double* z, int64_t n, const double* matrix16,
                             const double* centroid3_or_null, int invert, double* x_out, double* y_out, double* z_out, int memspace);

/* ---- ICP coregistration (csrc/icp.hip) -----------------------------------------------------------------------------------------
 * The device passes of xdem.coreg.ICP (Besl & McKay 1992, Chen & Medioni 1992; xdem/coreg/affine.py:296-328, 773-1182) for two rasters
 * on one grid, and an exact 3-D nearest-neighbour search for any two clouds.  Everything is float64 without contraction.
 *  xdemhip_dh_icp_normals    _icp_norms (affine.py:1062-1081) on a dh plan: np.gradient(ref) in the raster dtype,
 *                            nx = -sin(arctan(d/dcol / res_y)), ny = sin(arctan(d/drow / res_x)) -- upstream's pairing of derivative and
 *                            resolution -- with the quotient taken in the dtype, g / sqrt(1 + g^2) (= sin(arctan g)) in float64 and rounded
 *                            once to the dtype, nz = 1 - sqrt(nx^2 + ny^2) in the dtype.  The planes are kept by the plan; the call NARROWS
 *                            the plan's valid mask to the pixels where all three are finite (*n_valid = the new count), so it must come
 *                            before xdemhip_dh_subsample or any call that lists the valid pixels: XDEMHIP_EINVAL afterwards.  Outputs
 *                            (H * W values each, any may be NULL) are copied out; a second call only copies.  At least 2 x 2 pixels.
 *  xdemhip_icp_create_plan   the clouds of the plan's selected pixels, device-resident, structure of arrays: x, y (pixel centres), ref, tba
 *                            and -- with_normals -- nx, ny, nz, in raster order.  centroid3 = the per-axis np.median of (x, y, ref), exact
 *                            (radix selection; an even count averages the two middle values), subtracted from both clouds; std_fac = the
 *                            mean of the three 1.4826 * median|v - median v| of the centred reference cloud (standardize = 0: 1), both
 *                            clouds divided by it.  Then the search grid of the reference cloud is built.  *count = the points.
 *  xdemhip_icp_create_points the same object for arbitrary clouds: ref3n (3 x n, rows x, y, z), query3m (3 x m), optional normals at the
 *                            reference points; host memory; nothing is centred or scaled.
 *  xdemhip_icp_cloud         the rows x, y, ref, tba, nx, ny, nz (7 x n, host) of a cloud made from a plan, as standardised.
 *  xdemhip_icp_grid          the search grid: (x0, y0, h) -- cell (i, j) covers [x0 + i h, x0 + (i + 1) h) x [y0 + j h, y0 + (j + 1) h), the
 *                            last column and row also what lies beyond -- and its (columns, rows).
 *  xdemhip_icp_query         nearest reference point of every query point under the 4 x 4 matrix (rows 0..2 used; NULL = identity;
 *                            p' = (m0 x + m1 y) + m2 z + m3): a uniform grid of square cells over the reference (x, y), sized from the
 *                            bounding box and n for about three points per cell (an axis of zero extent gets one row of cells), built by
 *                            a counting sort; one thread per query walks Chebyshev rings of cells around its own cell (clamped to the
 *                            grid) and keeps the smallest dx dx + dy dy + dz dz, ties to the LOWEST reference index; it stops after a
 *                            ring once the best is strictly below the squared distance from the query's real position to the nearest
 *                            unvisited cell (less a rounding allowance).  ind (int64) and dist (the square root) stay on the device for
 *                            the next calls and are copied to the host outputs that are not NULL.  Two runs return the same bits.
 *  xdemhip_icp_set_pairs     put ind / dist (m each, host) in the place of a query's result (the moved cloud = the query cloud).
 *  xdemhip_icp_pairs         the pairs of the fit.  picky (Zinsser et al. 2003; affine.py:1017-1021): per reference index the pair of
 *                            smallest distance -- atomicMin over the distance bits, then over the query indexes at that distance (pandas
 *                            idxmin: first occurrence), then the keep flags compacted -- in reference-index order; else every pair in
 *                            query order.  *n_kept, and optionally the kept (query index, reference index) lists on the host.
 *  xdemhip_icp_sums          for every kept pair p' = S t (S = step16, t = the query point as moved by the last query), q its reference
 *                            point: method 1 point-to-plane r = (p' - q) . n, J = [p' x n, n]; method 0 point-to-point r = |p' - q|,
 *                            u = (p' - q) / r, J = [p' x u, u], a zero row where r = 0.  sums_out[37] = the 21 upper-triangle terms of
 *                            J J^T (row by row; parameters: rotation vector, then translation), the 6 of J r, sum r^2, and nine moments
 *                            of p': sums of x^2, y^2, z^2, xy, xz, yz, x, y, z -- with the count they give the normal matrix of the VECTOR
 *                            residual p' - q, sum D^T D with D = [-[p']x, I], which the point-to-point Gauss-Newton uses (same gradient
 *                            J^T r; the scalar rows drop r grad^2 r = I - u u^T and do not converge).  Per-lane accumulators, one
 *                            partial per workgroup, partials added in a fixed order (the same bits every call), one fetch.
 *  xdemhip_icp_values        what upstream hands _icp_fit: rows ref x, y, z, moved query x, y, z, normals x, y, z of the kept pairs
 *                            (9 x n_kept, host; the normals' rows are zero without normals). */
typedef struct xdemhip_icp xdemhip_icp;
int xdemhip_dh_icp_normals(xdemhip_dh_plan* plan, const double* transform6, void* nx_out, void* ny_out, void* nz_out, int memspace, int64_t* n_valid);
int xdemhip_icp_create_plan(xdemhip_dh_plan* plan, const double* transform6, int with_normals, int standardize, xdemhip_icp** out, double* centroid3,
                            double* std_fac, int64_t* count);
int xdemhip_icp_create_points(xdemhip_ctx* ctx, const double* ref3n, int64_t n, const double* query3m, int64_t m, const double* norms3n_or_null,
                              xdemhip_icp** out);
int xdemhip_icp_cloud(xdemhip_icp* icp, double* out7n);
int xdemhip_icp_grid(xdemhip_icp* icp, double* x0_y0_h, int64_t* gx_gy);
int xdemhip_icp_query(xdemhip_icp* icp, const double* matrix16_or_null, int64_t* ind_out, double* dist_out);
int xdemhip_icp_set_pairs(xdemhip_icp* icp, const int64_t* ind, const double* dist);
int xdemhip_icp_pairs(xdemhip_icp* icp, int picky, int64_t* n_kept, int64_t* query_idx_out, int64_t* ref_idx_out);
int xdemhip_icp_sums(xdemhip_icp* icp, const double* step16, int method, double* sums_out, int64_t* count);
int xdemhip_icp_values(xdemhip_icp* icp, double* out9k);
void xdemhip_icp_destroy(xdemhip_icp* icp);

/* ---- CPD coregistration (csrc/cpd.hip) -----------------------------------------------------------------------------------------
 * The device passes of xdem.coreg.CPD (Myronenko & Song 2010; xdem/coreg/affine.py:1190-1409): the E-step over EVERY pair of a
 * reference cloud x (N points) and a to-be-aligned cloud y (M points), and the sums of the M-step.  Float64 without contraction;
 * nothing of size N M is stored; no float atomics, two calls return the same bits.
 *  xdemhip_cpd_create_plan   the clouds (x, y, ref) and (x, y, tba) of the plan's selected pixels, centred and scaled exactly as
 *                            xdemhip_icp_create_plan does without normals (the same code); no search grid.  *count = N = M.
 *  xdemhip_cpd_create_points arbitrary clouds: ref3n (3 x n, rows x, y, z), tba3m (3 x m), host memory; N != M allowed; nothing is centred.
 *  xdemhip_cpd_estep         ty_m = matrix y_m (rows 0..2 of the 4 x 4; NULL = identity).  sigma2 = the argument, or -- NaN -- the sum
 *                            over all pairs of |x_n - ty_m|^2, added pair by pair, / (3 N M).  p_mn = exp(-((dx dx + dy dy) + dz dz) /
 *                            (2 sigma2)), den_n = sum_m p_mn, c = (2 pi sigma2)^(3/2) weight / (1 - weight) M / N, inv_n = 1 /
 *                            (max(den_n, 2^-52) + c), P_mn = p_mn inv_n; Pt1_n = den_n inv_n, P1_m = sum_n P_mn, PX_m = sum_n P_mn x_n.
 *                            A workgroup of 256 lanes owns 256 points of one cloud and walks one slice of the other through LDS; a lane
 *                            adds its slice in ascending index, slices are added in ascending order, and the slice length depends on N,
 *                            M and the device only.  Then, in fixed-order sums: Np = sum P1, muX = sum PX / Np, muY = sum P1 y / Np,
 *                            A = sum_m (PX_m - P1_m muX)(y_m - muY)^T, xPx = sum_n Pt1_n |x_n - muX|^2, YPY = sum_m P1_m |y_m - muY|^2.
 *                            sums_out[18] = Np, muX (3), muY (3), A (9, row by row), xPx, YPY; *sigma2_used.  One fetch.  0 <= weight < 1.
 *  xdemhip_cpd_terms         host copies of the last E-step's P1 (M), Pt1 (N) and PX (3 x M, rows x, y, z); any may be NULL. */
typedef struct xdemhip_cpd xdemhip_cpd;
int xdemhip_cpd_create_plan(xdemhip_dh_plan* plan, const double* transform6, int standardize, xdemhip_cpd** out, double* centroid3, double* std_fac,
                            int64_t* count);
int xdemhip_cpd_create_points(xdemhip_ctx* ctx, const double* ref3n, int64_t n, const double* tba3m, int64_t m, xdemhip_cpd** out);
int xdemhip_cpd_estep(xdemhip_cpd* cpd, const double* matrix16_or_null, double sigma2_or_nan, double weight, double* sums_out, double* sigma2_used);
int xdemhip_cpd_terms(xdemhip_cpd* cpd, double* p1_out, double* pt1_out, double* px_out);
void xdemhip_cpd_destroy(xdemhip_cpd* cpd);

/* out = cast(double(elev) + P(x, y)), P = np.polynomial.polynomial.polyval2d(x, y, c) with c[i, j] = coeffs[i * (order + 1) + j]
 * (the reference's fit_params reshaped), x = column, y = row_offset + row, evaluated in NumPy's order bit for bit: Horner in x for
 * every j (polyval, tensor form), then Horner in y (polyval, tensor=False), no fused multiply-add.  out has the dtype of elev: float32
 * elev -> float32(elev + P) (the reference's final cast), float64 -> elev + P.  Non-finite elev stays non-finite.  order 0..5. */
int xdemhip_poly2d_apply(xdemhip_ctx* ctx, const void* elev, int dtype, int64_t H, int64_t W, int64_t row_offset, const double* coeffs,
                         int order, void* out, int memspace);

/* "Next" row f4: the dense step of the patches method -- mean_filter_nan(img, kernel_size, kernel_shape)
 * (xdem/spatialstats.py:2597-2655: two scipy.ndimage.convolve calls with a ones / circular uint8 kernel, mode="constant",
 * cval=nan).  kernel_shape 0 = square, 1 = circular (_create_circular_mask, spatialstats.py:880-904).  Outputs are float64
 * (H, W) like the reference's: mean of the finite pixels under the kernel and their number; a window with a kernel pixel
 * outside the raster gives (NaN, 0) as SciPy's NaN border value does.  *n_kernel_px = np.count_nonzero(kernel).  Kernels of
 * more than 127 pixels (kernel_size > 11 square, > 13 circular) return XDEMHIP_EUNSUPPORTED: the reference counts in int8,
 * which wraps there. */
int xdemhip_mean_filter_nan(xdemhip_ctx* ctx, const void* img, int dtype, int64_t H, int64_t W, int kernel_size, int kernel_shape,
                            double* mean_out, double* nvalid_out, int* n_kernel_px, int memspace);

/* Row a5 as the PUBLIC function: xdem.spatialstats.convolution(imgs, filters, method)
 * (xdem/spatialstats.py:2558-2594; called by the reference's surface fit, surfit.py:1107, and by its tests,
 * tests/test_terrain/test_surfit.py:542-563, 612): `n_img` images (H x W, `dtype` float32 / float64, contiguous) against
 * `n_f` filters (M1 x M2, float64, HOST memory whatever `memspace` says) -> out float64 (n_img, n_f, H, W).
 * method 0 = "scipy": scipy.ndimage.convolve(img, filter, mode="constant", cval=nan) per pair (_scipy_convolution,
 * spatialstats.py:2512-2525) -- true convolution, weights with |w| <= DBL_EPSILON skipped, NaN beyond the border, double
 * accumulation in SciPy's tap order, rounded to the image dtype; method 1 = "numba": the loop of _numba_convolution
 * (spatialstats.py:2528-2555) on the NaN-padded images of 2582-2585 -- correlation over every tap, unrounded float64, last
 * row / column left 0 for an even filter size.  Bit for bit in both (tests/test_convolution_gpu.py). */
int xdemhip_convolution(xdemhip_ctx* ctx, const void* imgs, int dtype, int64_t n_img, int64_t H, int64_t W, const double* filters,
                        int n_f, int M1, int M2, int method, double* out, int memspace);

/* "Next" row f3, consumer side: xdem.spatialstats.get_perbin_nd_binning(df, list_var, list_var_names,
 * statistic, min_count) (xdem/spatialstats.py:425-527; used by the bias corrections, xdem/coreg/biascorr.py:302) as ONE
 * lookup per pixel instead of a mask per bin.  `vars[k]` = variable k (n values, `var_dtypes[k]` float32 / float64, in
 * `memspace`); host tables: variable k's `n_intervals[k]` sorted unique intervals [left, right) concatenated in `left` /
 * `right` (float64, already rounded to the dtype NumPy compares in), `table` / `pass` over the Cartesian product of the
 * intervals in itertools.product order (last variable fastest): the bin's statistic and 1 = write it (count > min_count),
 * 0 = leave NaN, 2 = the DataFrame has no such row.  `disjoint` != 0: the intervals of every variable are pairwise disjoint
 * (nd_binning's output) -- one containing interval per variable; 0: overlapping intervals, the product is walked per pixel in
 * upstream's order and the last bin that writes wins.  out float64 (n); *n_missing = pixels lying in a bin of kind 2 (upstream
 * raises IndexError there, and so does the Python side). */
int xdemhip_perbin_lookup(xdemhip_ctx* ctx, const void* const* vars, const int* var_dtypes, int n_var, int64_t n,
                          const int* n_intervals, const double* left, const double* right, const double* table,
                          const unsigned char* pass, int disjoint, double* out, int64_t* n_missing, int memspace);

/* "Next" row f1: the step right after a Nuth-Kaab fit -- resampling the translated DEM back onto
 * its own grid, i.e. _reproject_horizontal_shift_samecrs(raster_arr, src_transform, dst_transform)
 * (xdem/coreg/base.py:1615-1655) as used by Coreg.apply for pure translations:
 *     out(r, c) = bilinear(src)(r + shift_row_px, c + shift_col_px) + dz      (same tap convention as xdemhip_nk_step) */
int xdemhip_shift_bilinear(xdemhip_ctx* ctx, const void* src, int dtype, int64_t H, int64_t W, double shift_row_px,
                           double shift_col_px, double dz, void* out, int memspace);

/* ---- geoutils' Raster.reproject, same CRS: a raster resampled onto another north-up grid ----------------------------------------
 * What the reference's entry points do first to put two rasters on one grid (xdem/coreg/base.py:146-156, demcollection.py:128,
 * dem.py:724, ddem.py:198).  The reference runs GDAL's warper through rasterio; the rule here is written down in DESIGN.md
 * ("Regridding") and restated in NumPy by tests/reproject_oracle.py, whose bits every route returns -- parity with GDAL is unpinned.
 * src: H x W, float32 / float64 (uint8 with XDEMHIP_REGRID_NEAREST only, then dst is uint8 too); dst: h x w, float32 / float64 in any
 * combination with src.  map4 = (rx, tx, ry, ty): the centre of destination pixel (row o_y, column o_x) lies at
 * (u_y, u_x) = ((o_y + 0.5) ry + ty, (o_x + 0.5) rx + tx) in source pixel units (pixel i covers [i, i + 1)); rx, ry > 0, i.e.
 * r = a_d / a_s and t = (c_d - c_s) / a_s per axis of two north-up transforms.  Kernels: bilinear (radius 1), cubic (Catmull-Rom,
 * radius 2), cubic spline (B-spline, radius 2), stretched by max(1, r) when downsampling; taps outside the source and non-finite taps
 * are dropped and the rest renormalised; a pixel whose centre lies outside the source, or whose remaining weight is <= 1e-5, is NaN.
 * Nearest copies source pixel floor(u + 1e-10) per axis, NaN (uint8: 0) outside.  float64 arithmetic throughout, in one fixed order.
 * *valid_count = destination pixels that are not NaN (uint8: pixels taken from inside the source), counted in the same pass.
 * Nothing outlives the call: it returns synchronised in both memory spaces.  XDEMHIP_EUNSUPPORTED: a downsampling that needs more
 * than 2^24 taps per destination pixel. */
enum { XDEMHIP_U8 = 2 };
enum { XDEMHIP_REGRID_NEAREST = 0, XDEMHIP_REGRID_BILINEAR = 1, XDEMHIP_REGRID_CUBIC = 2, XDEMHIP_REGRID_CUBIC_SPLINE = 3 };
int xdemhip_regrid(xdemhip_ctx* ctx, const void* src, int src_dtype, int64_t H, int64_t W, void* dst, int dst_dtype, int64_t h, int64_t w,
                   const double* map4, int kernel, int memspace, int64_t* valid_count);

/* ---- xdem.coreg.BlockwiseCoreg (xdem/coreg/blockwise.py): one Nuth-Kaab fit per tile of a tiling, all tiles together --------------
 * A plan copies the two rasters into tile-major buffers (tiles4: row0, row1, col0, col1 of each of the n_tiles <= 65535 tiles, every tile
 * inside the raster, at least 2 x 2 and fewer than 2^31 pixels); every tile is then an independent raster: np.gradient is one-sided
 * on ITS borders and no bilinear tap or nodata neighbourhood ("nk_nan_rule", read at creation) leaves it.  n_valid_per_tile[t] = the
 * valid pixels of tile t (the valid mask of xdemhip_nk_create, per tile).  The caller's arrays are not referenced after the call.
 * xdemhip_bw_nk_step runs ONE iteration step of every tile whose active[t] is non-zero, at that tile's own (shift_x[t], shift_y[t]), in
 * a number of launches that does not depend on n_tiles, with one copy back.  Per active tile: what xdemhip_nk_step returns for the
 * tile as a raster of its own -- vshift, n_valid (finite dh; 0: the tile has no valid value left, every other entry of it is NaN / 0),
 * y_mean / y_std (float64, summed in a fixed order), edges[t][n_bins + 1], counts[t][n_bins], medians[t][n_bins], n_bins <= 128.  The
 * entries of inactive tiles are left as they are.  Automatic edges and the median statistic only.
 * xdemhip_bw_apply is the warp of BlockwiseCoreg.apply for shift fields affine in (x, y): coeff_* = (a, b, d) of shift = a x + b y + d in
 * the georeferenced coordinates of transform6 = (a, b, c, d, e, f) (x = a col + c, y = e row + f at pixel corners; b = d = 0).  With
 * M = I + [[a_x, b_x], [a_y, b_y]]: out(p') = (dtype)(bilinear(dem)(row(p), col(p)) + a_z x + b_z y + d_z) at p = M^-1 (p' - (d_x, d_y)),
 * p' the output pixel's centre; float64, nodata by "nk_nan_rule".  XDEMHIP_EINVAL if M is singular. */
typedef struct xdemhip_bw_plan xdemhip_bw_plan;
int xdemhip_bw_create(xdemhip_ctx* ctx, const void* ref, const void* tba, const unsigned char* inlier_or_null, int dtype, int64_t H, int64_t W,
                      int n_tiles, const int64_t* tiles4, int memspace, xdemhip_bw_plan** plan, int64_t* n_valid_per_tile);
int xdemhip_bw_nk_step(xdemhip_bw_plan* plan, const unsigned char* active, const double* shift_x, const double* shift_y, double res_x,
                       double res_y, int n_bins, double* vshift, int64_t* n_valid, double* y_mean, double* y_std, double* edges,
                       int64_t* counts, double* medians);
/* (slope tangent, aspect, valid mask) of every tile copied to the host, tile after tile, each tile row-major (tests / debugging) */
int xdemhip_bw_get_aux(xdemhip_bw_plan* plan, void* slope_tan, void* aspect, unsigned char* valid);
void xdemhip_bw_destroy(xdemhip_bw_plan* plan);
int xdemhip_bw_apply(xdemhip_ctx* ctx, const void* dem, int dtype, int64_t H, int64_t W, const double* transform6, const double* coeff_x3,
                     const double* coeff_y3, const double* coeff_z3, void* out, int memspace);

/* ---- path 3: empirical variogram, pairwise lag binning -----------------------------------------------
 * Replaces the pairwise work sample_empirical_variogram delegates to scikit-gstat:
 *   skg.Variogram(coordinates, values, bin_func=<right edges>, maxlag=, estimator=)      xdem/spatialstats.py:1091  (pdist)
 *   skg.Variogram(RasterEquidistantMetricSpace / ProbabalisticMetricSpace, values, ...)  xdem/spatialstats.py:1247-1255 (cdist)
 *   -> V.get_empirical(bin_center=False), V.bin_count
 * A "pair set" is a list of blocks; block r pairs every point A_r[i] with every point B_r[j] (b_off != NULL), or
 * all i < j inside A_r (b_off == NULL).  Points are SoA (x, y float64; value float32/float64), blocks concatenated,
 * a_off / b_off hold n_blocks + 1 offsets.  Lag class k: right_edges[k-1] <= d < right_edges[k] (edges[-1] := 0);
 * d >= right_edges[n_bins-1] is dropped.  Pairs with a NaN value difference are dropped.
 *
 *  xdemhip_pairs_sums   kind 0: sums[k] = sum |dv|^2 (Matheron), kind 1: sum sqrt|dv| (Cressie-Hawkins); counts[k]
 *  xdemhip_pairs_hist   one radix-select pass for the exact per-class median of |dv| (Dowd): histogram (n_bins x 256,
 *                       uint64) of key bits [shift, shift+8) among pairs whose higher key bits equal prefix[k]
 *                       (first != 0: all pairs).  Keys are order-preserving integer images of |dv|: its IEEE bits
 *                       shifted left by one (the sign bit of |dv| is always 0), 32 bit for float32 values, 64 bit for
 *                       float64.  The host advances the selection; integer
 *                       histograms / counts can be summed over GPUs (all-reduce) before doing so.
 *  xdemhip_pairs_succ   succ[k] = smallest key > key[k] in class k (all-ones if none): upper median of even classes.
 */
typedef struct xdemhip_pairs xdemhip_pairs;
int xdemhip_pairs_create(xdemhip_ctx* ctx, int n_blocks, const int64_t* a_off, const double* ax, const double* ay,
                         const void* av, const int64_t* b_off, const double* bx, const double* by, const void* bv,
                         int val_dtype, const double* right_edges, int n_bins, int memspace, xdemhip_pairs** out,
                         int64_t* n_pairs);
int xdemhip_pairs_sums(xdemhip_pairs* pairs, int kind, double* sums, int64_t* counts);
int xdemhip_pairs_hist(xdemhip_pairs* pairs, int shift, int first, const uint64_t* prefix, uint64_t* hist);
int xdemhip_pairs_succ(xdemhip_pairs* pairs, const uint64_t* key, uint64_t* succ);
/* Exact per-class median of |dv| (np.median semantics: mean of the two middle values in the value dtype for even classes,
 * NaN for empty ones) and the class counts, selection state kept on the device: Dowd's estimator is
 * 2.198 * median^2 / 2.  Large pair sets (>= 4e9 pairs) are bracketed first -- digit passes over a 1/64 sample of the
 * (A tile x B tile) units, ONE pass over all pairs that counts and compacts the candidates, exact selection among them --
 * with the plain 4 (float32) / 8 (float64) digit passes + successor pass as the fall-back and for small sets.  Histograms,
 * counters and successor keys go through the xdemhip_set_allreduce hook when the pair blocks are sharded over GPUs. */
int xdemhip_pairs_medians(xdemhip_pairs* pairs, int64_t* counts, double* medians);
/* Tell `pairs` that `sorted` holds THE SAME blocks (same sizes, value dtype, edges, context) with the points of every block
 * in an order in which neighbouring slots are neighbouring points (Morton order): the one pass of xdemhip_pairs_medians that
 * visits every pair -- counting against the brackets and compacting the candidates -- then reads `sorted`'s points and
 * counts run-length (a lane touches its LDS counters once per run of equal lag class instead of once per pair).  Counts,
 * candidates and medians do not depend on the slot order.  The sampled digit passes keep `pairs`' own order (their
 * statistics assume unsorted tiles).  `sorted` is not owned and must outlive the calls; NULL (or `pairs` itself) unlinks.
 * (Test switch "vario_runs" = 0 ignores the link: include/xdemhip_test.h.) */
int xdemhip_pairs_link_sorted(xdemhip_pairs* pairs, xdemhip_pairs* sorted);
/* Round 5: float64 differences of float32 values (option "vario_diff" = 1 -- SciPy's pdist widens -- on float32 inputs) at the speed
 * of the float32 kernels.  `shadow` is a float32 set of the same blocks and edges as the float64 set `pairs` (whose values are all
 * exactly float32 numbers, widened): xdemhip_pairs_medians(pairs) then classifies every pair by its float32 difference on the
 * shadow (rounding is monotone, so the integer counts hold for the exact differences too), stages the candidates as exact float64
 * differences and selects among them in float64 -- the float64 medians bit for bit, the counting pass in 38 instead of 60 ms on
 * BASELINE's C5.  NULL removes the link; the shadow must outlive it (not owned). */
int xdemhip_pairs_link_shadow(xdemhip_pairs* pairs, xdemhip_pairs* shadow);
/* Whether exact medians on this pair set take the bracketed route (one counting pass against sample brackets: large sets, few
 * enough lag classes, the selection mode that allows it, no reduction hook) -- the only route that reads a float32 shadow, so a
 * caller builds one (two more uploads and their device memory) exactly when this says 1. */
int xdemhip_pairs_takes_brackets(xdemhip_pairs* pairs, int* yes);
void xdemhip_pairs_destroy(xdemhip_pairs* pairs);

/* ---- next row 8f-3: N-dimensional binned statistics ---------------------------------------------------------------
 * Replaces the array work of  nd_binning(values, list_var, list_var_names, list_var_bins, statistics, list_ranges)
 * xdem/spatialstats.py:91-216, i.e. scipy.stats.binned_statistic / binned_statistic_2d / binned_statistic_dd with the
 * statistics "count", np.nanmedian and nmad (1.4826 * nanmedian(|x - nanmedian(x)|), geoutils.stats.nmad) -- the binning
 * behind the heteroscedasticity inference (spatialstats.py:576-631).
 *
 *  create / add_var   values and explanatory variables, all of length n (float32 or float64 each).
 *  finalize           joint finiteness filter (spatialstats.py:140-143) -> n_valid, and every variable's min / max over
 *                     the kept rows (what SciPy's _bin_edges takes its range from).
 *  run                one binning over n_dims of the variables.  edges = the dimensions' bin edges concatenated
 *                     (n_edges[d] each, float64 numbers already rounded to SciPy's edge dtype); decimals[d] = SciPy's
 *                     `int(-log10(min edge spacing)) + 6` and sample_dtype = dtype of its sample matrix (both only matter
 *                     for samples at or beyond the rightmost edge, _binned_statistic.py:_bin_numbers).  Outputs are in C
 *                     order over the dimensions: counts (exact), medians (exact order statistics, mean of the two
 *                     middle values in the value dtype for even counts, NaN for empty bins), nmads (want_nmad != 0).
 */
typedef struct xdemhip_binstats xdemhip_binstats;
int xdemhip_binstats_create(xdemhip_ctx* ctx, const void* values, int dtype, int64_t n, int memspace, xdemhip_binstats** out);
int xdemhip_binstats_add_var(xdemhip_binstats* plan, const void* var, int dtype, int memspace); /* returns the variable id */
int xdemhip_binstats_finalize(xdemhip_binstats* plan, int64_t* n_valid, double* var_min, double* var_max);
int xdemhip_binstats_run(xdemhip_binstats* plan, int n_dims, const int* var_ids, const double* edges, const int* n_edges,
                         const int* decimals, int sample_dtype, int want_nmad, double nfact, int64_t* counts,
                         double* medians, double* nmads);
/* The flat bin number (C order over the dimensions of the LAST xdemhip_binstats_run) of each of the n samples, 0xFFFF for a sample
 * the joint finiteness filter dropped or that lies in no bin: what a binding needs to evaluate a statistic the device does not know
 * -- any Python callable nd_binning is given (xdem/spatialstats.py:143-157 hands it to scipy.stats.binned_statistic, which applies
 * it to the values of every bin in sample order) -- on the host.  bins_out: host array of n uint16. */
int xdemhip_binstats_bin_numbers(xdemhip_binstats* plan, uint16_t* bins_out);
void xdemhip_binstats_destroy(xdemhip_binstats* plan);

/* Global NMAD of an array, NaN-skipping: median = np.nanmedian(v), nmad = nfact * np.nanmedian(|v - median|) in the value
 * dtype; values with |v| > abs_limit are dropped first (two_step_standardization's outlier filter, spatialstats.py:556-561;
 * pass +inf to keep everything). */
int xdemhip_nmad(xdemhip_ctx* ctx, const void* values, int dtype, int64_t n, double nfact, double abs_limit, int memspace,
                 double* median, double* nmad, int64_t* count);

/* The statistics of one raster (geoutils' Raster.get_stats, which xdem's DEM inherits: xdem/workflows/topo.py:291,
 * accuracy.py:243-381) from fused passes and a multi-rank exact selection (csrc/rasterstats.hip, csrc/multi_select.h).
 * A pixel is VALID when its value is finite (+-Inf is not), differs from `nodata` (has_nodata != 0) and total_mask (uint8, or NULL:
 * all ones) is non-zero there; the value statistics are over the valid pixels whose `inlier` byte (uint8, or NULL) is non-zero too.
 * `nodata` is rounded to `dtype` before it is compared (NumPy's `v == nodata`): for a float32 raster 0.1 matches the pixels that hold
 * (float)0.1; a NaN `nodata` matches nothing, and neither does one that rounds to +-Inf (such pixels are not valid anyway).
 *   n, n_valid, n_inlier   pixels behind the value statistics; valid pixels whatever `inlier` says; non-zero bytes of `inlier`
 *                          (n_values without one)
 *   min, max               exact
 *   sum, sumsq, sumdev2    float64 sums of v, v^2 and (v - sum / n)^2, the squares formed in float64 from the widened value, added in
 *                          one fixed order: two calls return the same bits
 *   med_lo, med_hi         the order statistics of ranks (n - 1) / 2 and n / 2;  median = their mean in the value dtype (np.median)
 *   q_lo[i], q_hi[i]       the order statistics of ranks lo = floor((n - 1) * quantiles[i]) (one float64 multiply) and
 *                          min(lo + 1, n - 1): what np.percentile(..., method="linear") interpolates between; nq <= XDEMHIP_STATS_MAXQ
 *                          quantiles in [0, 1]
 *   mad_lo, mad_hi         the same two ranks of |v - median|, formed in the value dtype;  nmad = nfact * their mean, rounded as
 *                          xdemhip_nmad rounds it
 *   reads                  full reads of the raster the call made;  route[r] of round r (0: v, 1: |v - median|): 1 plain digit
 *                          passes, 0 bracketed, 2 bracketed first and then plain (a bracket missed or the candidates overflowed)
 * The route follows the "selection" option -- 0: bracketed from 2^22 pixels on, 1: plain, 2: collapsed brackets (the fall-back), 3:
 * bracketed at every size -- and never changes a bit of the result.  n == 0 or no valid pixel: counts 0, every value NaN, XDEMHIP_OK.
 * With a reduction hook installed: XDEMHIP_EUNSUPPORTED (the statistics of a partitioned raster are not provided).
 * XDEMHIP_DEVICE: values and both masks are device arrays; the call returns synchronised on the context's stream. */
#define XDEMHIP_STATS_MAXQ 4
typedef struct xdemhip_raster_stats_out {
    int64_t n, n_valid, n_inlier;
    double min, max, sum, sumsq, sumdev2, med_lo, med_hi, median, mad_lo, mad_hi, nmad;
    double q_lo[XDEMHIP_STATS_MAXQ], q_hi[XDEMHIP_STATS_MAXQ];
    double reads;
    int32_t route[2];
} xdemhip_raster_stats_out;
int xdemhip_raster_stats(xdemhip_ctx* ctx, const void* values, int dtype, int64_t n_values, const uint8_t* total_mask,
                         const uint8_t* inlier, int has_nodata, double nodata, const double* quantiles, int nq, double nfact,
                         int memspace, xdemhip_raster_stats_out* out);

/* out[p] = scale * f(vars[0][p], ..., vars[n_dims-1][p]) for the multilinear interpolant f on a regular grid: the evaluation
 * scipy.interpolate.RegularGridInterpolator(axes, grid_values, method="linear", bounds_error=False, fill_value=None) performs
 * for the error function returned by interp_nd_binning (xdem/spatialstats.py:417-421) and applied to whole rasters by
 * infer_heteroscedasticity_from_stable (spatialstats.py:866-868).  axes = grid axes concatenated (n_axis[d] points each,
 * ascending), grid_values in C order, NaN in any coordinate -> NaN, coordinates outside the grid extrapolate linearly. */
int xdemhip_interp_grid_linear(xdemhip_ctx* ctx, int n_dims, const double* axes, const int* n_axis, const double* grid_values,
                               const void* const* vars, const int* var_dtypes, int64_t n, double scale, double* out, int memspace);

/* ---- caller of path 3: double sum of spatially correlated errors ------------------------------------------------------
 * out = sum_i sum_j  ae[i] * be[j] * rho(|a_i - b_j|),  rho(h) = 1 - sum_m gamma_m(h) / sum_m psill_m: the O(N^2) part of
 *   neff_exact(coords, errors, params_variogram_model)            xdem/spatialstats.py:2175-2236  (bx = NULL: B = A, every ordered
 *                                                                  pair including i = j)
 *   neff_hugonnet_approx(coords, errors, params, subsample, ...)  xdem/spatialstats.py:2239-2308  (B = the random subset)
 * model_type: 0 spherical, 1 exponential, 2 gaussian, 3 cubic, 4 stable (smooth[m] used); scikit-gstat's effective-range forms.
 * Coordinates and errors float64. */
int xdemhip_cov_double_sum(xdemhip_ctx* ctx, const double* ax, const double* ay, const double* ae, int64_t na, const double* bx,
                           const double* by, const double* be, int64_t nb, int n_models, const int* model_type, const double* range,
                           const double* psill, const double* smooth, double* out_sum, int memspace);

/* ---- hypsometric binning and gap filling (xdem/volume.py) -----------------------------------------------------------
 * A plan over one (dDEM, reference DEM) pair of n pixels, float32 or float64 each, with an optional int32 label map (a glacier
 * index map: label 0 = no glacier, labels in [1, 2^20)) OR an optional byte mask (non-zero = "label 1"); neither: every pixel has
 * label 1.  Host arrays are uploaded once and kept; device arrays are used in place and must outlive the plan.  An INLIER is a
 * pixel of a non-zero label with a finite dDEM and a finite reference.
 *  label_stats  one pass: for every label that occurs (at most `cap`, in no particular order) its id, counts[2] = (pixels, inliers)
 *               and extremes[4] = min, max of the reference over its pixels with a finite reference, min, max over its inliers
 *               (NaN where there is none).  n_bad_labels: pixels whose label lies outside [0, 2^20); n_ref_invalid: pixels of the
 *               whole raster with a non-finite reference.
 *  segments     for the n_kept labels `ids` (rank r = position in the list), each with its own nb + 1 increasing bin edges
 *               (edges[r * (nb + 1) ..]): every inlier's bin i = np.digitize(ref, edges) (right=False, the comparison in float64
 *               on the exactly widened values), kept for 1 <= i <= nb; group = r * nb + (i - 1).  Per group: the count, the exact
 *               median of the dDEM (np.median: the mean of the two middle values in the dDEM's dtype for an even count; NaN for an
 *               empty group) and, with want_std, np.nanstd (ddof 0) in float64 -- the mean, then the squared deviations, both summed
 *               in one fixed order over the segment sorted by value: the same bits from every run.
 *  groups       the group of every pixel in the last segments call (-1: in none), for statistics the device does not evaluate.
 *  fill         out[p] = fill(p) ? model_r(ref[p]) : ddem[p], r = rank of the pixel's label in `ids`; model_r = SciPy's
 *               interp1d(xs[r * m ..], ys[r * m ..], kind="linear", fill_value="extrapolate") in float64.  mode 0: fill = label
 *               kept and dDEM not finite; mode 1: fill = label kept.  round_to_ref: the model's value is rounded to the reference's
 *               dtype before it is stored (hypsometric_interpolation writes it into such a plane).  out_dtype: the dDEM's dtype, or
 *               float64.  `out` in `memspace`.
 * A context serialises these calls like all others. */
typedef struct xdemhip_hypso xdemhip_hypso;
int xdemhip_hypso_create(xdemhip_ctx* ctx, const void* ddem, int ddem_dtype, const void* ref, int ref_dtype, const int32_t* labels,
                         const unsigned char* mask, int64_t n, int memspace, xdemhip_hypso** out);
int xdemhip_hypso_label_stats(xdemhip_hypso* plan, int64_t cap, int32_t* ids, int64_t* counts, double* extremes, int64_t* n_found,
                              int64_t* n_bad_labels, int64_t* n_ref_invalid);
int xdemhip_hypso_segments(xdemhip_hypso* plan, int n_kept, const int32_t* ids, int nb, const double* edges, int want_std,
                           int64_t* counts, double* medians, double* stds);
int xdemhip_hypso_groups(xdemhip_hypso* plan, int32_t* groups_out, int memspace);
int xdemhip_hypso_fill(xdemhip_hypso* plan, int mode, int n_kept, const int32_t* ids, int m, const double* xs, const double* ys,
                       int round_to_ref, void* out, int out_dtype, int memspace);
void xdemhip_hypso_destroy(xdemhip_hypso* plan);
/* calculate_hypsometry_area (volume.py:239-299): counts[i] = pixels whose elevation e lies in [edges[i], edges[i + 1]) -- the last
 * bin closed on the right, np.histogram -- with e = ref (timeframe 0), ref - f(ref) (1) or ref - f(ref) / 2 (2) in float64,
 * f = interp1d(xs, ys, fill_value="extrapolate") of m points. */
int xdemhip_hypso_area(xdemhip_ctx* ctx, const void* ref, int dtype, int64_t n, int timeframe, int m, const double* xs,
                       const double* ys, int nb, const double* edges, int64_t* counts, int memspace);

/* ---- a stack of DEMs (xdem/demcollection.py, xdem/ddem.py) ----------------------------------------------------------------
 * T planes (1 .. 1024) of n pixels on one grid, all float32 or all float64, one of them the reference.  Host planes are uploaded
 * once and kept, device planes are used in place and must outlive the stack.  subtract and fill write T contiguous planes to `out`
 * in `memspace`: a device array is written in place and read again by the later passes (it must outlive the stack, or the next call
 * that replaces it); behind a host array the stack owns the device planes and copies them out.  Every pass is a number of launches
 * that does not depend on T and ends in one fetch.
 *  subtract     ddem_t = ref - dem_t, one IEEE subtraction in the planes' dtype.  n_differ[t]: pixels of plane t that differ from the
 *               reference (other bits, and not both NaN); a plane with none EQUALS the reference and its dDEM is set to 0 -- unless
 *               can_equal[t] is 0 (T host ints, null: all 1; the caller knows of a difference outside the pixels, a nodata value).
 *               n_nonfinite[t]: non-finite pixels of the dDEM as left.
 *  set_masks    n_masks distinct byte masks of n pixels (non-zero = inside) and one mask id per plane (-1: every pixel).  Masks in
 *               `memspace`; device masks must outlive the stack.  Without a call every plane has every pixel.
 *  stats        per plane over its INLIERS -- inside its mask, dDEM and reference finite: their number, min and max of the
 *               reference over them (NaN without an inlier).
 *  segments     the grouping pass of xdemhip_hypso_segments for all planes at once: plane t has nbs[t] bins (0: the plane is left
 *               out) whose nbs[t] + 1 edges start row t of `edges`, rows of nb_max + 1.  counts / medians: T rows of nb_max, the
 *               entries beyond a plane's bins 0 / NaN.  Medians are np.median's, exact.  (Test switch "hypso_seg_lds".)
 *  fill         filled_t[p] = (p inside mask_t, ddem_t[p] not finite, ms[t] >= 2) ? model_t(ref[p]) rounded to the planes' dtype
 *               : ddem_t[p]; model_t = interp1d(xs[t * m_max ..], ys[t * m_max ..], fill_value="extrapolate") of ms[t] points
 *               (ms[t] = 0: plane t is copied).  Fused into the pass, per plane over its own mask: n_mask[t] pixels of the mask,
 *               n_finite[t] finite filled values among them, sums[t] their float64 sum in the fixed order of the library's
 *               repeatable sums (one partial per workgroup, a grid that depends on the device and n only): the same bits every run.
 *  series       the same three figures without filling, over `which` planes: 0 the inputs, 1 the dDEMs, 2 the filled dDEMs;
 *               mask (n bytes in `memspace`; null: every plane's own mask) is the mask of all planes.
 * A context serialises these calls like all others. */
typedef struct xdemhip_stack xdemhip_stack;
int xdemhip_stack_create(xdemhip_ctx* ctx, const void* const* planes, int n_planes, int dtype, int64_t n, int ref_index, int memspace,
                         xdemhip_stack** out);
int xdemhip_stack_set_masks(xdemhip_stack* stack, const unsigned char* const* masks, int n_masks, const int32_t* mask_id, int memspace);
int xdemhip_stack_subtract(xdemhip_stack* stack, const int32_t* can_equal, void* out, int memspace, int64_t* n_differ, int64_t* n_nonfinite);
int xdemhip_stack_stats(xdemhip_stack* stack, int64_t* inliers, double* ref_min, double* ref_max);
int xdemhip_stack_segments(xdemhip_stack* stack, int nb_max, const int32_t* nbs, const double* edges, int64_t* counts, double* medians);
int xdemhip_stack_fill(xdemhip_stack* stack, int m_max, const int32_t* ms, const double* xs, const double* ys, void* out, int memspace,
                       int64_t* n_mask, int64_t* n_finite, double* sums);
int xdemhip_stack_series(xdemhip_stack* stack, int which, const unsigned char* mask, int memspace, int64_t* n_mask, int64_t* n_finite,
                         double* sums);
void xdemhip_stack_destroy(xdemhip_stack* stack);

/* ---- polygons burnt into a grid (geoutils' Vector.create_mask / Vector.rasterize with all_touched=False) -------------------
 * A table of P polygons as R rings over V vertices: xy = the V abscissae, then the V ordinates (float64); ring r is the vertices
 * ring_off[r] .. ring_off[r + 1] (ring_off[0] = 0, ring_off[R] = V, non-decreasing) and belongs to polygon poly_of_ring[r] in
 * [0, P) -- the rings of a multipolygon and its holes share one ordinal.  The grid is H x W under the north-up transform6
 * (a, 0, c0, 0, e, f) with a > 0 > e; anything else is XDEMHIP_EINVAL.
 * THE RULE: a pixel belongs to a polygon iff its centre is inside, every operation below rounded on its own in float64
 * (the file is built without contraction):
 *   centre of pixel (r, c):   cy(r) = f + (r + 0.5) * e,   cx(c) = c0 + (c + 0.5) * a
 *   an edge (x1, y1) -> (x2, y2) with y1 != y2 crosses row r iff min(y1, y2) <= cy(r) < max(y1, y2) (half open: a vertex on a centre
 *   line counts once, a horizontal edge never), at x = x1 + (cy(r) - y1) * (x2 - x1) / (y2 - y1), evaluated in that order
 *   (r, c) is inside iff the number of crossings of row r by the edges of ALL rings of the polygon with x <= cx(c) is odd: even-odd,
 *   so interior rings are holes.
 * Rings are closed implicitly (the edge from the last vertex back to the first; a repeated first vertex adds a horizontal edge of
 * length 0); a ring of fewer than three vertices contributes nothing.  Vertices must be finite (the callers check; an edge with a
 * NaN ordinate crosses no row).  Row ranges of edges and column ranges of spans start from a division and are corrected with the
 * very comparisons above, so membership is decided by those comparisons alone.
 *   out_kind 0   `out` = H * W bytes: 1 inside any polygon, 0 elsewhere (burn and out_value are not read)
 *   out_kind 1   `out` = H * W int32: burn[p] of the LAST polygon p in table order that holds the pixel (burn null: p + 1), out_value
 *                where none does
 * n_burnt (may be null): the pixels inside at least one polygon.  All arrays and `out` in `memspace`; n_burnt is a host word.  The
 * number of kernel launches does not depend on P, R or V (xdemhip_rasterize_launches: those of the last call).  Overlaps resolve
 * through an integer maximum, the count through the fixed order of the library's repeatable sums: the same bits every run.
 * (Test switches "vec_seg_reg", "vec_seg_lds".)
 * xdemhip_rasterize_union: the byte mask of the pixels inside a polygon of table A OR of table B (either table may have V = 0). */
int xdemhip_rasterize(xdemhip_ctx* ctx, const double* xy, int64_t V, const int64_t* ring_off, int64_t R, const int32_t* poly_of_ring,
                      const int32_t* burn_or_null, int32_t P, int64_t H, int64_t W, const double* transform6, void* out, int out_kind,
                      int32_t out_value, int memspace, int64_t* n_burnt);
int xdemhip_rasterize_union(xdemhip_ctx* ctx, const double* xy_a, int64_t V_a, const int64_t* ring_off_a, int64_t R_a,
                            const int32_t* poly_of_ring_a, int32_t P_a, const double* xy_b, int64_t V_b, const int64_t* ring_off_b,
                            int64_t R_b, const int32_t* poly_of_ring_b, int32_t P_b, int64_t H, int64_t W, const double* transform6,
                            unsigned char* out, int memspace, int64_t* n_burnt);
int xdemhip_rasterize_launches(xdemhip_ctx* ctx, int64_t* n_launches);

/* ---- exact Euclidean distance transform (edt.hip; geoutils' Raster.proximity) ---------------------------------------
 * xdemhip_edt: for every pixel of an H x W plane the distance to the nearest target (targets[y * W + x] != 0) under the sampling
 * (sy of rows, sx of columns; finite, > 0).  THE RULE, float64, every fl one rounding (the file is built without contraction):
 *   d(y, x) = sqrt( min over targets (ty, tx) of  fl( fl(fl((y - ty) sy)^2) + fl(fl((x - tx) sx)^2) ) )
 * the true float64 minimum of that expression over all targets (SciPy's expression, axis 0 first).  No target: +inf everywhere,
 * indices -1.  `dist` (may be null): H * W of dist_dtype (XDEMHIP_F32: the float64 result rounded once).  `idx` (may be null):
 * int32 [2][H][W], row and column of the target that attains the minimum; among targets of equal cost the smaller |x - tx| wins,
 * then the smaller tx, then within that column the nearer row, the upper row on a tie.  `keep` (may be null): H * W bytes, the
 * distance is 0 wherever (keep != 0) != (keep_polarity != 0) (indices are not touched).  n_targets (may be null; a host word):
 * the targets counted.  Planes in `memspace`; the call returns synchronised and holds no memory afterwards.  Sides 1 .. 2^31 - 1.
 * Only sums, products and comparisons of the costs above decide which target wins (no divisions, no parabola intersections): the
 * column pass keeps the nearest target of each column as an integer row offset, the row pass scans outward from each pixel and
 * stops at the first column distance whose own cost reaches the best so far, skipping blocks of columns whose lower bound does.
 * (Test switch "edt_route"; xdemhip_edt_plan of include/xdemhip_test.h has the tile constants.)
 * xdemhip_edt_targets: out[i] = 1 where src[i] is a target, else 0: with n_values = 0 finite and != 0, else equal to one of
 * values[0 .. n_values) (at most 64, host doubles; NaN never is a target).  src of XDEMHIP_F32 / _F64 / _U8 / _I32, n >= 1 elements.
 * xdemhip_mask_boundary: out = 1 on the inner boundary of a byte mask: a mask pixel with a 4-neighbour INSIDE the raster that is not
 * in the mask (the raster's edge makes no boundary), else 0. */
enum { XDEMHIP_I32 = 3 };
int xdemhip_edt(xdemhip_ctx* ctx, const unsigned char* targets, int64_t H, int64_t W, double sy, double sx, void* dist, int dist_dtype,
                int32_t* idx, const unsigned char* keep, int keep_polarity, int memspace, int64_t* n_targets);
int xdemhip_edt_targets(xdemhip_ctx* ctx, const void* src, int src_dtype, int64_t n, const double* values, int n_values,
                        unsigned char* out, int memspace);
int xdemhip_mask_boundary(xdemhip_ctx* ctx, const unsigned char* mask, int64_t H, int64_t W, unsigned char* out, int memspace);

/* ---- sampling a raster at points, a raster as points (spline.hip; geoutils' Raster.interp_points / to_pointcloud) -----
 * THE RULE, float64, every operation one rounding (the file is built without contraction); transform6 = (a, b, c, d, e, f), b = d = 0:
 *   r = (y - f) / e - 0.5, cc = (x - c) / a - 0.5 (without the 0.5 when shift != 0); a point with r outside [0, H - 1] or cc outside
 *   [0, W - 1], or a non-finite coordinate, gives NaN.
 *   spread = the non-finite pixels grown by `dist` in city-block distance; a point is NaN if one of its four bilinear corner pixels
 *   with non-zero weight (w0 = 1 - t, w1 = 1 - w0) is in it.  A raster without a finite pixel gives NaN everywhere.
 *   order 0: the pixel floor(r + 0.5), floor(cc + 0.5).  order 1: the four taps of the raster itself.  orders 3 and 5: the
 *   (order + 1)^2 B-spline taps (SciPy's weight polynomials, mirror index mapping) of the coefficient plane: the mirror spline
 *   prefilter (per axis a gain, per pole a causal and an anticausal recursion; columns first) of the raster whose non-finite pixels
 *   took the value of their nearest finite pixel (xdemhip_edt's winner on unit sampling).  value = sum of ((c wr) wc) from 0.0, rows
 *   outer and columns inner, rounded once to the raster's dtype.
 * xdemhip_spline_prepare: makes the plan of an H x W raster (sides >= 2; XDEMHIP_F32 / _F64; host or device memory) for an order
 *   (0, 1, 3, 5) and a spreading distance: the spread plane and, for orders 3 and 5, the coefficients, in device memory the plan
 *   owns.  For orders 0 and 1 the plan reads the raster at every gather: a device raster must outlive the plan (a host raster is
 *   copied).  *n_nonfinite = the number of non-finite pixels.  Returns synchronised.  (Test switch "spline_route".)
 * xdemhip_spline_gather: out[i] = the value at (x[i], y[i]), i < n (float64 columns; host or device memory, the result where the
 *   points are) in out_dtype: the raster's dtype, or XDEMHIP_F64 for the value before its one rounding; *n_valid = the number of
 *   results that are not NaN.  Returns synchronised.
 * xdemhip_raster_points: the pixels of a raster in row-major order as x = c + (col + 0.5) a, y = f + (row + 0.5) e (float64) and z
 *   (the raster's dtype); skip_nodata != 0 keeps the finite pixels only (per-row counts, an exclusive scan, a write in column order).
 *   *count = the number of points; with x = y = z = null only the count is made, else `capacity` (elements) must hold it.
 *   Returns synchronised. */
typedef struct xdemhip_spline xdemhip_spline;
int xdemhip_spline_prepare(xdemhip_ctx* ctx, const void* raster, int dtype, int64_t H, int64_t W, int order, int dist, int memspace,
                           xdemhip_spline** out, int64_t* n_nonfinite);
int xdemhip_spline_gather(xdemhip_spline* plan, const double* x, const double* y, int64_t n, const double* transform6, int shift, void* out,
                          int out_dtype, int memspace, int64_t* n_valid);
void xdemhip_spline_destroy(xdemhip_spline* plan);
int xdemhip_raster_points(xdemhip_ctx* ctx, const void* raster, int dtype, int64_t H, int64_t W, const double* transform6, int skip_nodata,
                          double* x, double* y, void* z, int64_t capacity, int memspace, int64_t* count);

/* ---- connected components and outline rings (ccl.hip; scipy.ndimage.label, geoutils' Raster.polygonize) -------------------
 * THE RULE of xdemhip_label.  `classes`: an H x W plane of XDEMHIP_U8 or XDEMHIP_I32, 0 = background; H * W < 2^31 (else XDEMHIP_EINVAL).
 *   Two pixels are joined iff they are neighbours under `connectivity` (4: sharing an edge; 8: or a corner) and hold the same non-zero
 *   class; a component is a class of the transitive closure.  `labels` (int32, H x W): 0 on background; the components are numbered
 *   1 .. K in raster order of their first pixel, the one with the smallest row * W + col.  On a 0/1 plane that is scipy.ndimage.label's
 *   numbering with generate_binary_structure(2, 1) for 4 and (2, 2) for 8.  *K (a host word): the number of components.
 *   `table` (may be null): K x 7 int64, COLUMN by column (table[col * K + l - 1] for label l): class, pixel count, row_min, row_max,
 *   col_min, col_max (inclusive), linear index of the first pixel.  It is written when `capacity` (components) holds K; a smaller
 *   capacity returns XDEMHIP_EINVAL with the labels and *K written, so a caller without a bound passes table = null, reads K and calls
 *   xdemhip_label_table on the label plane it has (the way xdemhip_raster_points is called twice).
 *   Union-find on a parent plane whose roots are the smallest linear index of their set, split over launches at every inter-workgroup
 *   hand-off (no flags, no spin-waiting); counts, minima and maxima are integer atomics: the same bits every run.
 *   (Test switch "ccl_route"; xdemhip_label_plan of include/xdemhip_test.h has the tile.)
 * xdemhip_label_table: the same table from a label plane and the class plane it was made of (labels outside 1 .. K are skipped).
 * THE RULE of xdemhip_outlines.  `labels`: an int32 H x W plane, 0 = background, a component = the pixels of one value in 1 .. K (any
 *   other value: XDEMHIP_EINVAL), as xdemhip_label makes them under either connectivity.  Vertices are pixel corners (i, j), i in [0, H],
 *   j in [0, W].  A component owns one unit EDGE for each side of each of its pixels whose neighbour across that side is not in the
 *   component (another component, background, or outside the raster).  Sides: 0 top, 1 left, 2 bottom, 3 right; edge number =
 *   4 * (row * W + col) + side.  An edge is directed with its pixel on the left in map coordinates (x east, y north): the top side
 *   runs west, the left side south, the bottom side east, the right side north.  The SUCCESSOR of an edge is the edge of the same
 *   component that starts at its end vertex; with `ahead` the pixel across the end vertex on the edge's own side and `across` the one on
 *   the other side: if `across` is in the component the ring turns right onto its previous side (so at a PINCH vertex, where two
 *   diagonally opposite pixels belong to the component and two edges start, the ring keeps hugging the non-member pixel on its right);
 *   else if `ahead` is in the component it goes straight on along the same side of `ahead`; else it turns left onto the next side of
 *   its own pixel.  The successor is a permutation of the edges; its cycles are the RINGS.  Every component has exactly one ring of
 *   positive signed area, its exterior, counter-clockwise in map coordinates, and any number of rings of negative area, its holes,
 *   clockwise; the signed areas of a component's rings add up to its pixel count.  Under connectivity 4 no ring visits a vertex twice;
 *   under connectivity 8 a ring may touch itself at a pinch vertex (inherent; GDAL's polygonize does the same).
 *   Only CORNER edges, those whose successor turns, give a vertex: their end vertex.  A ring starts at the end vertex of its
 *   lowest-numbered corner edge and follows the successors.  The lowest edge of a component is the top side of its first pixel, a corner
 *   edge of its exterior, so with the rings of a component in increasing number of that edge the exterior comes first; components
 *   follow in label order.  x = c + a * j, y = f + e * i in float64, one multiply and one add each (built without contraction), for the
 *   north-up transform6 (a, 0, c, 0, e, f), a > 0 > e (else XDEMHIP_EINVAL).
 *   Outputs, the table layout xdemhip_rasterize reads: xy = the V abscissae, then the V ordinates, packed for the V the call returns;
 *   ring_off (R + 1 int64), poly_of_ring (R int32: label - 1), ring_area (may be null; R int64: the signed area in pixels).  *V and *R
 *   are host words.  With xy = ring_off = poly_of_ring = null only the counting pass runs: *V is exact and *R is the bound V / 4 (a
 *   ring has at least four corners); the full call needs v_capacity >= V and r_capacity >= V / 4 (ring_off one more) and returns the
 *   exact *R.  V must stay below 2^31.  The number of kernel launches depends on H and W only.
 * All planes and arrays in `memspace`; every call returns synchronised and holds no memory afterwards. */
int xdemhip_label(xdemhip_ctx* ctx, const void* classes, int dtype, int64_t H, int64_t W, int connectivity, int32_t* labels, int64_t* table,
                  int64_t capacity, int memspace, int64_t* K);
int xdemhip_label_table(xdemhip_ctx* ctx, const void* classes, int dtype, const int32_t* labels, int64_t H, int64_t W, int64_t K, int64_t* table,
                        int memspace);
int xdemhip_outlines(xdemhip_ctx* ctx, const int32_t* labels, int64_t H, int64_t W, int64_t K, const double* transform6, double* xy, int64_t v_capacity,
                     int64_t* ring_off, int32_t* poly_of_ring, int64_t* ring_area, int64_t r_capacity, int memspace, int64_t* V, int64_t* R);

/* ---- raster filters (filter.hip; scipy.ndimage.gaussian_filter / generic_filter, xDEM's old xdem/filters.py) -----------
 * xdemhip_filter: out = the filter `kind` of the H x W plane `in` (XDEMHIP_F32 / _F64, row-major; sides 1 .. 2^31 - 1), in the same
 * dtype and memspace.  NaN = missing; +-Inf are ordinary values.  tests/filters_oracle.py restates every rule in NumPy and every route
 * returns its bits (the file is built without contraction).  `out` must not overlap `in` (XDEMHIP_EINVAL).
 *   XDEMHIP_FILTER_GAUSSIAN  scipy.ndimage.gaussian_filter(mode="reflect"): `radius` = lw = int(truncate * sigma + 0.5) and `weights` =
 *     the 2 lw + 1 normalised float64 weights, both made by the caller on the host (the library has no exp; it checks sigma > 0,
 *     truncate > 0 and that radius is that lw).  Axis 0 first, then axis 1; one pass, float64, in SciPy's order:
 *     tmp = c w[lw]; for i = -lw .. -1: tmp += (x[i] + x[-i]) w[i + lw]; x mirrored about the raster's edges (d c b a | a b c d | d c b a,
 *     repeated when lw exceeds the side); the axis-0 result is rounded to the dtype before the axis-1 pass, the axis-1 result after it.
 *     `normalise` 0: that, NaN spreading as in SciPy.  1: g = G(in with NaN -> 0), n = G(1 where not NaN else 0, in the dtype),
 *     out = g / n in the dtype (IEEE division), NaN where in is NaN.  2: 1 if the plane holds a NaN (one counting pass), else 0.
 *   XDEMHIP_FILTER_MEDIAN / _MIN / _MAX  the window size x size (odd, >= 3) about the pixel, clipped at the raster's edge: the median /
 *     minimum / maximum of its non-NaN values, NaN if it has none, whether or not the centre is NaN.  An even count gives (a + b) / 2
 *     of the two middle values in float64, rounded once.  Values are compared as order-preserving unsigned keys: -0.0 < +0.0.
 *   XDEMHIP_FILTER_MEAN  footprint = the square size x size (size odd >= 3, radius = 0) or the disk dy^2 + dx^2 <= radius^2 (size = 0,
 *     radius >= 0), clipped at the edge: the float64 sum of its non-NaN values from +0.0, dy outer and dx inner, both ascending, divided
 *     by their count and rounded once; NaN for an empty window.
 *   XDEMHIP_FILTER_DISTANCE  out = in, but NaN where |in - m| > threshold, m the unrounded float64 disk mean (radius; the centre
 *     included), the comparison in float64 (false for a NaN on either side).  One pass; no mean plane is stored.
 * A workgroup stages its tile and halo in LDS once, the edge rule applied while staging, and filters from there; halos beyond the LDS
 * budget read their taps from global memory (the Gaussian in two launches through a plane of the call's own): no upper limit on sigma,
 * size or radius but XDEMHIP_EUNSUPPORTED above lw = 2^20 and above radius 16383 / size 32767 (int32 window counts).
 * Returns synchronised whenever the call held a buffer of its own (host memory, a Gaussian's weights, a disk's table); a square
 * window on device memory is queued on the context's stream.  The call holds no memory afterwards.
 * (Test switch "filter_route"; xdemhip_filter_plan of include/xdemhip_test.h has the tile.) */
enum { XDEMHIP_FILTER_GAUSSIAN = 0, XDEMHIP_FILTER_MEDIAN = 1, XDEMHIP_FILTER_MEAN = 2, XDEMHIP_FILTER_MIN = 3, XDEMHIP_FILTER_MAX = 4,
       XDEMHIP_FILTER_DISTANCE = 5 };
int xdemhip_filter(xdemhip_ctx* ctx, const void* in, int dtype, int64_t H, int64_t W, int kind, int size, int radius, double sigma,
                   double truncate, const double* weights, int normalise, double threshold, void* out, int memspace);

#ifdef __cplusplus
}
#endif
#endif /* XDEMHIP_H */
