// terrain_route.h -- the host side of the terrain path as data: which kernel a call gets (terrain_route), how the streaming route
// cuts a raster into strips and frame tiles (plan_strips), which window kernel runs on which grid (plan_window) and how a
// host-buffer call is cut into row chunks (plan_host_chunks).  Plain C++17, no HIP: terrain_tile.h, terrain_host.hip and capi.hip
// act on these plans; tests/test_terrain_route_host.py restates every rule and compares on the CPU.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../../include/xdemhip.h"

namespace xd {

// ---- attribute groups ---------------------------------------------------------------------------------------------------------
constexpr uint32_t ATTRS_CURVATURE = XDEMHIP_ATTR_CURVATURE | XDEMHIP_ATTR_PROFILE_CURVATURE | XDEMHIP_ATTR_TANGENTIAL_CURVATURE |
                                     XDEMHIP_ATTR_PLANFORM_CURVATURE | XDEMHIP_ATTR_FLOWLINE_CURVATURE | XDEMHIP_ATTR_MAX_CURVATURE |
                                     XDEMHIP_ATTR_MIN_CURVATURE;
constexpr uint32_t ATTRS_SURFACE = XDEMHIP_ATTR_SLOPE | XDEMHIP_ATTR_ASPECT | XDEMHIP_ATTR_HILLSHADE | ATTRS_CURVATURE;   // need a surface fit
constexpr uint32_t ATTRS_FUSED_WINDOW = XDEMHIP_ATTR_TPI | XDEMHIP_ATTR_TRI | XDEMHIP_ATTR_ROUGHNESS;   // windowed indexes the fused kernels know (window 3)
constexpr uint32_t ATTRS_WINDOWED = ATTRS_FUSED_WINDOW | XDEMHIP_ATTR_FRACTAL_ROUGHNESS;              // every index over window_size
constexpr uint32_t ATTRS_NEED_RESOLUTION = ATTRS_SURFACE | XDEMHIP_ATTR_RUGOSITY;                     // (terrain.py:352-367)
constexpr uint32_t ATTRS_FULL11 = (ATTRS_SURFACE & ~(uint32_t)XDEMHIP_ATTR_CURVATURE) | XDEMHIP_ATTR_TPI | XDEMHIP_ATTR_TRI;
constexpr uint32_t ATTRS_SAH = XDEMHIP_ATTR_SLOPE | XDEMHIP_ATTR_ASPECT | XDEMHIP_ATTR_HILLSHADE;
constexpr uint32_t ATTRS_SAH_WIN = ATTRS_SAH | XDEMHIP_ATTR_TPI | XDEMHIP_ATTR_TRI;

// ---- argument checks of xdemhip_terrain, in the order the entry point has always made them -------------------------------------
struct TerrainCheck { int code; const char* msg; };
inline TerrainCheck terrain_validate(const void* dem, const void* out_planes, int dem_dtype, int64_t H, int64_t W, int64_t row_stride,
                                     int64_t halo_top, int64_t halo_bottom, double resolution, int surface_fit, int curv_method,
                                     uint32_t attr_mask, int tri_method, int window_size, int out_dtype, int memspace) {
    const auto bad = [](const char* msg) { return TerrainCheck{XDEMHIP_EINVAL, msg}; };
    if (!dem || !out_planes) return bad("null buffer");
    if (H <= 0 || W <= 0 || row_stride < W || halo_top < 0 || halo_bottom < 0) return bad("bad raster geometry");
    if ((dem_dtype != XDEMHIP_F32 && dem_dtype != XDEMHIP_F64) || (out_dtype != XDEMHIP_F32 && out_dtype != XDEMHIP_F64))
        return bad("dtype must be XDEMHIP_F32 or XDEMHIP_F64");
    if (surface_fit < 0 || surface_fit > 2) return bad("unknown surface_fit");
    if (curv_method < 0 || curv_method > 1) return bad("unknown curv_method");
    if (tri_method < 0 || tri_method > 1) return bad("unknown tri_method");
    if (attr_mask == 0 || (attr_mask >> XDEMHIP_ATTR_COUNT)) return bad("bad attr_mask");
    if (surface_fit == XDEMHIP_FIT_HORN && (attr_mask & ATTRS_CURVATURE))
        return bad("'Horn' surface fit cannot be used to calculate curvatures");
    if ((attr_mask & ATTRS_WINDOWED) && (window_size < 3 || (window_size & 1) == 0 || window_size > 1023))
        return bad("window_size must be odd and >= 3");
    if ((attr_mask & ATTRS_NEED_RESOLUTION) && !(resolution > 0.0)) return bad("resolution must be > 0");
    if (memspace != XDEMHIP_HOST && memspace != XDEMHIP_DEVICE) return bad("bad memspace");
    return TerrainCheck{XDEMHIP_OK, ""};
}

// ---- which kernel ---------------------------------------------------------------------------------------------------------------
// The fused kernels come in families: compile-time attribute sets for the calls users make most (all with the reference's defaults:
// degrees, Riley TRI, z_factor 1, clipped hillshade) and the runtime-mask kernels for everything else.
enum TerrainFamily {
    TF_NONE = 0,         // no fused launch: only windowed indexes of a window size other than 3
    TF_FULL11_GEO,       // the eleven planes, geometric curvatures (Florinsky / Zevenbergen-Thorne)
    TF_FULL11_DIR,       // the eleven planes, directional curvatures
    TF_SAH_WIN,          // slope, aspect, hillshade, TPI, TRI (Horn)
    TF_SLOPE, TF_SLOPE_ASPECT, TF_HILLSHADE, TF_SAH,   // the small sets (every fit, lean tail only)
    TF_RUNTIME,          // runtime attribute mask, mixed tail
    TF_RUNTIME_F64       // runtime attribute mask, float64 attribute math (float32 -> float32 only)
};

struct TerrainCall {     // what of a call the choice looks at
    int dem_dtype, out_dtype;
    uint32_t attr_mask;  // the fused and window kernels' attributes (bits below XDEMHIP_ATTR_RUGOSITY)
    int surface_fit, curv_method, tri_method, degrees;
    double hs_z;
    int hs_unclipped, window_size;
};
struct TerrainOptions { int terrain_math, terrain_stream; };

struct TerrainRoute {
    int family = TF_NONE;
    int fit = XDEMHIP_FIT_ZEVENBERGTHORNE;   // template argument FIT of the fused kernel
    bool curv = false, fuse_win = false;     // template arguments CURV and WIN
    int tail = 0;             // Spec's F64TAIL: 0 mixed, 1 float64, 2 lean
    bool try_stream = false;  // strips for the interior where plan_strips lets the raster through
    uint32_t mask = 0;        // attributes of the fused launch
    uint32_t window_mask = 0; // attributes of the separate window launch that follows (0: none)
};

inline TerrainRoute terrain_route(const TerrainCall& c, const TerrainOptions& o) {
    TerrainRoute r;
    const uint32_t surf = c.attr_mask & ~ATTRS_FUSED_WINDOW, win = c.attr_mask & ATTRS_FUSED_WINDOW;
    r.fuse_win = win && c.window_size == 3;
    r.mask = surf | (r.fuse_win ? win : 0u);
    r.window_mask = r.fuse_win ? 0u : win;
    if (!r.mask) return r;
    r.fit = surf ? c.surface_fit : XDEMHIP_FIT_ZEVENBERGTHORNE;   // window-only: cheapest 3x3 march
    r.curv = r.fit != XDEMHIP_FIT_HORN && (surf & ATTRS_CURVATURE) != 0;
    const bool ff = c.dem_dtype == XDEMHIP_F32 && c.out_dtype == XDEMHIP_F32;
    // option "terrain_math" counts for float32 -> float32 only; an unclipped hillshade (the engine-boundary call) is known to the
    // float64 tail of the runtime-mask kernels alone
    const bool lean = ff && o.terrain_math == 2, mixed = !ff || o.terrain_math == 0;
    const bool f64tail = ff && (o.terrain_math == 1 || c.hs_unclipped);
    const bool hs_default = c.degrees && c.hs_z == 1.0 && !c.hs_unclipped;
    const bool defaults_dir = hs_default && c.tri_method == XDEMHIP_TRI_RILEY;   // ... with either curvature method
    const bool geometric = c.curv_method == XDEMHIP_CURV_GEOMETRIC, directional = c.curv_method == XDEMHIP_CURV_DIRECTIONAL;
    const bool fit_fl = r.fit == XDEMHIP_FIT_FLORINSKY, fit_zt = r.fit == XDEMHIP_FIT_ZEVENBERGTHORNE, fit_horn = r.fit == XDEMHIP_FIT_HORN;
    const auto specialised = [&](int family, int tail, bool stream) {
        r.family = family;
        r.tail = tail;
        r.curv = family == TF_FULL11_GEO || family == TF_FULL11_DIR;
        r.try_stream = stream && o.terrain_stream != 0;
        return r;
    };
    if (defaults_dir && (lean || mixed)) {
        const int tail = lean ? 2 : 0;
        if (r.mask == ATTRS_FULL11 && (fit_fl || fit_zt) && geometric) return specialised(TF_FULL11_GEO, tail, ff);
        if (r.mask == ATTRS_SAH_WIN && fit_horn && geometric) return specialised(TF_SAH_WIN, tail, ff);
        if (r.mask == ATTRS_FULL11 && (fit_fl || fit_zt) && directional && ff) return specialised(TF_FULL11_DIR, tail, true);
    }
    // the small sets: compile-time masks + lean tail + strips, like the full set.  (win == 0: a windowed index of another window
    // size keeps the runtime-mask kernel for its surface attributes and has its own launch)
    if (lean && hs_default && win == 0) {
        if (r.mask == XDEMHIP_ATTR_SLOPE) return specialised(TF_SLOPE, 2, true);
        if (r.mask == (XDEMHIP_ATTR_SLOPE | XDEMHIP_ATTR_ASPECT)) return specialised(TF_SLOPE_ASPECT, 2, true);
        if (r.mask == XDEMHIP_ATTR_HILLSHADE) return specialised(TF_HILLSHADE, 2, true);
        if (r.mask == ATTRS_SAH) return specialised(TF_SAH, 2, true);
    }
    if (f64tail && defaults_dir && geometric && r.mask == ATTRS_FULL11 && fit_fl) return specialised(TF_FULL11_GEO, 1, false);
    r.family = f64tail ? TF_RUNTIME_F64 : TF_RUNTIME;
    r.tail = f64tail ? 1 : 0;
    return r;
}

// ---- streaming strips: which part of the raster they take ------------------------------------------------------------------------
constexpr int TILE_W = 256;
constexpr int STRIP_TILE_H = 32;   // tile height of float32 rasters, the only ones that stream
struct RasterGeom { int64_t H, W, row_stride, halo_top, halo_bottom; };
struct FrameRect { int tx0 = 0, tx1 = 0, ty0 = 0, ty1 = 0; };  // interior tile rectangle left out in frame mode (empty: all tiles)

struct StripPlan {
    bool ok = false;           // false: the raster does not qualify, the tile kernel takes all of it
    FrameRect fr;              // the interior in tiles: strips inside, frame launch of the tile kernel outside
    int64_t xi0 = 0, yi0 = 0, yi1 = 0;   // the interior in pixels: columns from xi0 (groups of 256), rows [yi0, yi1)
    int band_height = 128;
    int groups_x = 0, nbands = 0, ngroups = 0, grid8 = 0;
    uint32_t perm_mul = 1;     // order 2: workgroup b takes strip group (b * perm_mul) mod (grid8 * 8)
    bool strips = true, frame = true;   // option "terrain_stream" = 3 / 2 (debug): one of the two launches only
};

// `halo`: rows a window reaches beyond its pixel (Halo<FIT>); `terrain_stream`: the option's value, 1 or a band height or 2 / 3
inline StripPlan plan_strips(const RasterGeom& g, bool dem_aligned16, int halo, int terrain_stream) {
    StripPlan p;
    if (!dem_aligned16 || (g.row_stride & 3)) return p;              // 16-byte quads of the LDS-DMA
    if (g.row_stride >= ((int64_t)1 << 24) - 64) return p;           // 24-bit row offsets inside a ring block
    p.fr.tx0 = 1;
    p.fr.tx1 = (int)((g.W - 4) / TILE_W);
    p.fr.ty0 = g.halo_top >= halo ? 0 : 1;
    const int64_t ylim = (g.H + g.halo_bottom - halo) < g.H ? (g.H + g.halo_bottom - halo) : g.H;
    p.fr.ty1 = (int)(ylim / STRIP_TILE_H);
    if (p.fr.tx1 - p.fr.tx0 < 1 || p.fr.ty1 - p.fr.ty0 < 2) return p;
    if ((int64_t)(p.fr.tx1 - p.fr.tx0) * (p.fr.ty1 - p.fr.ty0) < 64) return p;   // small rasters: one launch of the tile kernel
    p.xi0 = (int64_t)p.fr.tx0 * TILE_W; p.yi0 = (int64_t)p.fr.ty0 * STRIP_TILE_H; p.yi1 = (int64_t)p.fr.ty1 * STRIP_TILE_H;
    p.groups_x = p.fr.tx1 - p.fr.tx0;
    p.band_height = terrain_stream >= 64 ? terrain_stream : 128;
    p.strips = terrain_stream != 3;
    p.frame = terrain_stream != 2;
    const int64_t bands = (p.yi1 - p.yi0 + p.band_height - 1) / p.band_height;
    if (bands * p.groups_x > (int64_t)0xfffff0) return p;             // (a dispatch carries its work-item count in 32 bits)
    p.ngroups = (int)(bands * p.groups_x);
    p.grid8 = (p.ngroups + 7) / 8;
    p.nbands = (int)bands;
    // multiplier of order 2: near the golden section of the grid, coprime to it
    const uint32_t n = (uint32_t)p.grid8 * 8u;
    uint32_t m = (uint32_t)(0.6180339887 * (double)n) | 1u;
    const auto gcd = [](uint32_t x, uint32_t y) { while (y) { const uint32_t t = x % y; x = y; y = t; } return x; };
    while (m > 1 && gcd(m, n) != 1) m += 2;
    p.perm_mul = m;
    p.ok = true;
    return p;
}

// ---- windowed indexes of a window size other than 3 -----------------------------------------------------------------------------
constexpr int WIN_TW = 64, WIN_TH = 16;
constexpr size_t WIN_LDS_BYTES = 64 * 1024;
struct WindowPlan {
    bool lds = false;         // window_lds_kernel (a workgroup stages its patch in LDS) or window_generic_kernel (one thread per pixel)
    bool too_tall = false;    // generic kernel: more rows than one launch holds
    size_t lds_bytes = 0;
    unsigned grid_x = 0, grid_y = 0;
};
inline WindowPlan plan_window(int64_t H, int64_t W, int window_size, size_t in_elem, int terrain_window_lds) {
    WindowPlan p;
    p.lds_bytes = (size_t)(WIN_TH + window_size - 1) * (size_t)(WIN_TW + window_size - 1) * in_elem;
    const int64_t gy_lds = (H + WIN_TH - 1) / WIN_TH, gy_gen = (H + 3) / 4;
    p.lds = terrain_window_lds != 0 && p.lds_bytes <= WIN_LDS_BYTES && gy_lds <= 65535;
    p.too_tall = !p.lds && gy_gen > 65535;
    p.grid_x = (unsigned)(p.lds ? (W + WIN_TW - 1) / WIN_TW : (W + 63) / 64);
    p.grid_y = (unsigned)(p.lds ? gy_lds : gy_gen);
    return p;
}

// ---- host-buffer calls: row chunks ----------------------------------------------------------------------------------------------
// Overlap rows a chunk (or a rank's row block: xdem_amd/dist.py, halo_depth) needs on each side
inline int terrain_halo_depth(uint32_t attr_mask, int surface_fit, int window_size) {
    int depth = 0;
    if (attr_mask & ATTRS_SURFACE) depth = surface_fit == XDEMHIP_FIT_FLORINSKY ? 2 : 1;
    if ((attr_mask & ATTRS_WINDOWED) && window_size / 2 > depth) depth = window_size / 2;
    if ((attr_mask & XDEMHIP_ATTR_RUGOSITY) && depth < 1) depth = 1;
    return depth;
}

struct HostChunk { int64_t r0, r1, top, bot; };   // output rows [r0, r1) with `top` / `bot` rows of the caller's buffer above / below
struct HostChunks {
    static constexpr int64_t MIN_ROWS = 64;
    static constexpr int DEFAULT_BUDGET_MB = 288;   // ~256 MiB of planes per chunk: deep enough to hide latencies, small enough to pipeline
    int64_t H = 0, W = 0, halo_top = 0, halo_bottom = 0;
    size_t in_es = 4, out_es = 4;
    int n_planes = 0, depth = 0;
    int64_t rows = 0;          // output rows per chunk
    size_t in_bytes() const { return (size_t)(rows + 2 * depth) * (size_t)W * in_es; }
    size_t plane_bytes() const { return (size_t)rows * (size_t)W * out_es; }
    size_t out_bytes() const { return plane_bytes() * (size_t)n_planes; }
    // the pinning fallback: half the rows, down to MIN_ROWS; false when there is nothing left to halve
    bool halved() {
        if (rows <= MIN_ROWS) return false;
        rows = rows / 2 < MIN_ROWS ? MIN_ROWS : rows / 2;
        return true;
    }
    std::vector<HostChunk> list() const {
        std::vector<HostChunk> chunks;
        for (int64_t r0 = 0; r0 < H; r0 += rows) {
            HostChunk g;
            g.r0 = r0; g.r1 = (r0 + rows < H) ? r0 + rows : H;
            // rows of the caller's buffer (which itself may carry halo rows) available above / below this chunk
            g.top = (r0 + halo_top < depth) ? r0 + halo_top : depth;
            g.bot = (H + halo_bottom - g.r1 < depth) ? H + halo_bottom - g.r1 : depth;
            chunks.push_back(g);
        }
        return chunks;
    }
};
// `host_chunk_mb`: the device / pinned budget of one chunk, input + planes (0: the default); `host_chunk_rows`: the caller's tile
// size (mp_config.chunk_size of the reference's tiled call), which can only SHRINK the chunks: a tile of the whole raster's height --
// or a moderate one on a very wide raster -- would otherwise put input + all planes of the raster on the device and fail with ENOMEM
// where the untiled call streams
inline HostChunks plan_host_chunks(int64_t H, int64_t W, int64_t halo_top, int64_t halo_bottom, int depth, int n_planes, size_t in_es,
                                   size_t out_es, int host_chunk_mb, int host_chunk_rows) {
    HostChunks p;
    p.H = H; p.W = W; p.halo_top = halo_top; p.halo_bottom = halo_bottom;
    p.in_es = in_es; p.out_es = out_es; p.n_planes = n_planes; p.depth = depth;
    const size_t row_bytes = (size_t)W * (in_es + out_es * (size_t)n_planes);
    const size_t budget = (size_t)(host_chunk_mb > 0 ? host_chunk_mb : HostChunks::DEFAULT_BUDGET_MB) << 20;
    p.rows = (int64_t)(budget / (row_bytes ? row_bytes : 1)) - 2 * depth;
    if (host_chunk_rows > 0 && host_chunk_rows < p.rows) p.rows = host_chunk_rows;
    if (p.rows < HostChunks::MIN_ROWS) p.rows = HostChunks::MIN_ROWS;  // (a few rows of a very wide raster may exceed the budget; still correct)
    if (p.rows > H) p.rows = H;
    return p;
}

}  // namespace xd
