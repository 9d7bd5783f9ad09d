/* xdemhip_test.h -- switches between internal routes of libxdemhip.so that must AGREE (round 6: split from the options of
 * include/xdemhip.h).  Not part of the drop-in boundary: nothing a caller of the library needs; the route-agreement tests
 * (tests/test_*_gpu.py) and the measurement tools (tools/) set them.  Every value of every switch returns the same planes /
 * integers / medians -- that is what the tests assert.
 *   "terrain_stream"     1 (default) streaming strips over the raster interior + tiles over its frame where the raster qualifies,
 *                        0 tiles only; 2 / 3 = one of the two launches only (debug); 128 / 256 / 512 = band height.
 *   "terrain_order"      0 (default) one band of strip groups per XCD, 1 natural order, 2 permuted, 3 column-major (measurement forms).
 *   "terrain_ring_wait"  0 (default) counted s_waitcnt for the LDS-DMA ring of the streaming kernels, 1 vmcnt(0): the check of the count.
 *   "terrain_window_lds" 1 (default) LDS-tiled kernel for windowed indexes of window sizes other than 3, 0 the per-pixel kernel.
 *   "nk_narrow"          -1 (default) sample brackets of the one-pass step narrowed by the measured rank offsets, 0 / 1 / 2 fixed.
 *   "vario_grid"         1 (default) raster-sampled points run the integer-lattice pair kernels, 0 always the float64-coordinate ones.
 *   "vario_runs"         1 (default) run-length counting pass of the exact-Dowd route on the Morton-ordered copy, 0 per-pair counters.
 *   "vario_sort"         1 (default) the host side uploads a Morton-ordered copy of every pair block, 0 one copy in the caller's order.
 *   "hypso_seg_lds"      0 (default: 8192) the longest segment of xdemhip_hypso_segments that one workgroup sorts in LDS; a longer one takes
 *                        the radix selection over its slice of global memory (1 .. 16384: a test sends a 40-value segment down it).
 *   "bw_seg_lds"         0 (default: 4096) the longest (tile, bin) segment of xdemhip_bw_nk_step that one workgroup sorts in LDS; a longer one
 *                        takes the radix selection over its slice of global memory (1 .. 4096: a test sends 20-value segments down it).
 *   "pts_tile_order"     0 (default) the 4-tap gather of a raster-point plan walks the selected points in cloud order, 1 ordered by raster
 *                        tile (32 x 32 pixels) of their unshifted position; read when a selection is made (create / subsample).
 *   "vec_seg_reg"        0 (default: 8) the longest crossing segment (one polygon, one pixel row) of xdemhip_rasterize that a single lane sorts
 *                        in registers; a longer one goes to a workgroup (1 .. 8; 1 sends every segment to the workgroup routes).
 *   "vec_seg_lds"        0 (default: 4096) the longest crossing segment that one workgroup sorts in LDS; a longer one is sorted in place in
 *                        global memory (1 .. 4096; with "vec_seg_reg" = 1 the value 1 sends every segment down the global route).
 *   "vec_stage_times"    0 (default) / 1: xdemhip_rasterize records an event where each of its five stages starts and
 *                        xdemhip_rasterize_stage_ms returns the device time between them (a measurement form: the same planes).
 *   "regrid_route"       0 (default) xdemhip_regrid takes the LDS-tiled route while a workgroup's source footprint fits its LDS budget and
 *                        the per-pixel route that reads its taps from global memory beyond it; 1 = the tiled route wherever the footprint
 *                        fits (today the automatic choice, pinned against a later change of policy); 2 = the per-pixel route always.
 *   "edt_route"          0 (default) the row pass of xdemhip_edt scans a window of column offsets staged in LDS and goes on block by block
 *                        in global memory beyond its halo; 1 = no window: every pixel takes the block search in global memory; 2 = band
 *                        height, tile, halo and block shrunk to their minima, so that small planes cross bands, tiles and blocks.
 *   "spline_route"       0 (default) the prefilter of xdemhip_spline_prepare runs its column passes in bands of rows and its row passes
 *                        out of LDS tiles where a row is longer than its two warm-up halos, else one thread per row; 1 = one band per
 *                        column (no warm-up halo along rows); 2 = the one-thread-per-row route always; 3 = the LDS tiles always.
 *   "ccl_route"          0 (default) xdemhip_label labels tiles of 64 x 64 pixels in LDS before the border unions; 2 = minimal tiles of 2 x 2
 *                        pixels, so that small planes cross tile borders and four-tile corners everywhere (no value 1).
 *   "filter_route"       0 (default) xdemhip_filter takes the LDS-tiled route while tile and halo fit its LDS budget and reads its taps from
 *                        global memory beyond it; 1 = the tiled route wherever the halo fits (today the automatic choice, pinned against a
 *                        later change of policy); 2 = the global route always; 3 = tiles shrunk to their minimum (4 x 8 pixels), so that
 *                        small planes cross tile borders and corners everywhere. */
#pragma once
#include "xdemhip.h"
#ifdef __cplusplus
extern "C" {
#endif
int xdemhip_set_test_switch(xdemhip_ctx* ctx, const char* name, int value);
/* ms[5]: edges, crossings into segments (with the call's one fetch of two totals), sorts, spans, finish -- of the last
 * xdemhip_rasterize / xdemhip_rasterize_union call made with "vec_stage_times" = 1 (two tables: summed per stage); zeros otherwise. */
int xdemhip_rasterize_stage_ms(xdemhip_ctx* ctx, float* ms);
/* Device bytes that the plans of this context hold between calls: what their creates and steps asked for and have not yet freed
 * (0 once every plan is destroyed; the memory tests read it). */
int xdemhip_plan_bytes(xdemhip_ctx* ctx, int64_t* bytes);
/* The route xdemhip_regrid takes for a map4 / kernel / source dtype under a value of "regrid_route" (host only, no context):
 * *route = XDEMHIP_REGRID_ROUTE_*, *lds_bytes = what a workgroup of the tiled route would ask for, *lds_budget = the most it may. */
enum { XDEMHIP_REGRID_ROUTE_NEAREST = 0, XDEMHIP_REGRID_ROUTE_TILE = 1, XDEMHIP_REGRID_ROUTE_DIRECT = 2 };
int xdemhip_regrid_route(const double* map4, int kernel, int src_dtype, int route_switch, int* route, int64_t* lds_bytes, int64_t* lds_budget);
/* ms[4]: device time of the four passes (down, carry, up, row) of the last xdemhip_edt call on this context. */
int xdemhip_edt_stage_ms(xdemhip_ctx* ctx, float* ms);
/* The constants xdemhip_edt works with on an H x W plane under a value of "edt_route" (host only, no context): rows of a band of the
 * column pass, columns of a tile of the row pass, its halo on either side (0: no window), columns of a block of the block minima,
 * bytes of a stored row offset (2 while H <= 32767, else 4).  Any output may be null. */
int xdemhip_edt_plan(int64_t H, int64_t W, int route_switch, int* band_rows, int* tile_cols, int* halo, int* block_cols, int* offset_bytes);
/* The constants the prefilter of xdemhip_spline_prepare works with on an H x W raster (sides >= 2) for an order (0, 1, 3, 5) under a
 * value of "spline_route" (host only, no context): rows of a band of the column passes, rows and columns of a tile of the row passes
 * (1 x W: the one-thread-per-row route), the warm-up halo in samples, LDS bytes of a workgroup of the row passes.  Any output may be null. */
int xdemhip_spline_plan(int64_t H, int64_t W, int order, int route_switch, int* band_rows, int* tile_rows, int* tile_cols, int* halo, int* lds_bytes);
/* One line of the prefilter on the CPU through the functions the kernels run (host only, no context): every pole of the order (3, 5)
 * over in[0 .. n), n >= 2, cut into bands of `band` samples; two_phase != 0: each band walked as the LDS row route walks a segment. */
int xdemhip_spline_host_line(const double* in, int64_t n, int order, int64_t band, int two_phase, double* out);
/* ms[4]: device time of the stages of the prepare that made this plan: mask and fill, dilation, column passes, row passes. */
int xdemhip_spline_stage_ms(xdemhip_spline* plan, float* ms);
/* The planes a plan holds, copied out (either may be null; asking for one the plan does not hold is XDEMHIP_EINVAL): the uint8 spread
 * plane (held while the raster has some but not only non-finite pixels) and the float64 coefficients (orders 3 and 5). */
int xdemhip_spline_planes(xdemhip_spline* plan, unsigned char* spread, double* coef, int memspace);
/* The tile xdemhip_label works with on an H x W plane (H * W < 2^31) under a value of "ccl_route" (host only, no context): rows and
 * columns of a tile, the tiles down and across, the LDS bytes of a workgroup and the budget they must stay within.  Any output may be null. */
int xdemhip_label_plan(int64_t H, int64_t W, int route_switch, int* tile_rows, int* tile_cols, int64_t* tiles_r, int64_t* tiles_c, int* lds_bytes,
                       int* lds_budget);
/* ms[11]: device time of the stages of the last xdemhip_label call on this context (tile, border, flatten, number, table; the table
 * stage also after xdemhip_label_table) and of the last full xdemhip_outlines call (corners, walk, leader, rank, rings with their fetch
 * and host ordering, gather).  launches (may be null) [2]: the kernels those two calls launched. */
int xdemhip_ccl_stage_ms(xdemhip_ctx* ctx, float* ms, int64_t* launches);
/* The frame xdemhip_filter works with on an H x W plane for a kind (XDEMHIP_FILTER_*), a halo `radius` (the Gaussian's lw, size / 2
 * of a window, the radius of a disk) and a dtype under a value of "filter_route" (host only, no context): rows and columns of a tile,
 * its halo on every side, the LDS bytes of a workgroup of the tiled route (the Gaussian's counted with its normalising planes), the
 * budget they must stay within, and *route = XDEMHIP_FILTER_ROUTE_*.  Any output may be null. */
enum { XDEMHIP_FILTER_ROUTE_TILE = 1, XDEMHIP_FILTER_ROUTE_GLOBAL = 2 };
int xdemhip_filter_plan(int64_t H, int64_t W, int kind, int radius, int dtype, int route_switch, int* tile_rows, int* tile_cols, int* halo,
                        int64_t* lds_bytes, int64_t* lds_budget, int* route);
#ifdef __cplusplus
}
#endif
