// Host harness of the terrain path's host side (xdem_amd/csrc/terrain_route.h, host_copy.h) -- test tool only, driven through
// ctypes by tests/test_terrain_route_host.py.  Compiled with -DTR_COPY_MAIN it is a stand-alone program instead: the span-copy
// checks with their own main, for a build under -fsanitize=address,undefined.
#include <stdio.h>
#include <stdlib.h>

#include "../../xdem_amd/csrc/host_copy.h"
#include "../../xdem_amd/csrc/terrain_route.h"

using namespace xd;

// the literals the named masks replaced
static_assert(ATTRS_SURFACE == 0x3ffu && ATTRS_CURVATURE == 0x3f8u && ATTRS_WINDOWED == 0x5c00u, "attribute groups");
static_assert(ATTRS_NEED_RESOLUTION == (0x3ffu | XDEMHIP_ATTR_RUGOSITY) && ATTRS_FULL11 == (0xFFFu & ~8u) && ATTRS_SAH_WIN == 0xC07u, "attribute groups");

namespace {

// One copy of random-looking bytes through xd_parallel_copy into destinations with guard bytes either side; 0 if every destination
// equals its source and every guard byte is intact, else the 1-based index of the first span that is wrong.
int copy_case(const int64_t* sizes, int n, int nthreads, uint32_t seed) {
    const size_t G = 64;
    std::vector<std::vector<unsigned char>> src(n), dst(n);
    std::vector<XdSpan> spans;
    for (int i = 0; i < n; ++i) {
        src[i].resize((size_t)sizes[i] + 1);
        dst[i].assign((size_t)sizes[i] + 2 * G, 0xA5);
        for (size_t b = 0; b < (size_t)sizes[i]; ++b) { seed = seed * 1664525u + 1013904223u; src[i][b] = (unsigned char)(seed >> 24); }
        spans.push_back({reinterpret_cast<char*>(dst[i].data() + G), reinterpret_cast<const char*>(src[i].data()), (size_t)sizes[i]});
    }
    xd_parallel_copy(spans, nthreads);
    for (int i = 0; i < n; ++i) {
        if (memcmp(dst[i].data() + G, src[i].data(), (size_t)sizes[i]) != 0) return i + 1;
        for (size_t b = 0; b < G; ++b)
            if (dst[i][b] != 0xA5 || dst[i][G + (size_t)sizes[i] + b] != 0xA5) return i + 1;
    }
    return 0;
}

}  // namespace

#ifdef TR_COPY_MAIN
// argv: seed.  Span lists with empty spans, totals on both sides of the threaded path's threshold, 1 to 17 threads.
int main(int argc, char** argv) {
    uint32_t s = argc > 1 ? (uint32_t)atoi(argv[1]) : 1u;
    const auto rnd = [&](uint32_t n) { s = s * 1664525u + 1013904223u; return (s >> 8) % n; };
    int cases = 0;
    for (int nthreads = 1; nthreads <= 17; ++nthreads)
        for (int big = 0; big < 2; ++big) {
            std::vector<int64_t> sizes;
            const int n = 1 + (int)rnd(12);
            for (int i = 0; i < n; ++i) sizes.push_back(rnd(4) == 0 ? 0 : (int64_t)rnd(big ? 1500000 : 200000));
            if (big) sizes.push_back((int64_t)XD_COPY_THREADED_FROM);   // certainly threaded
            const int bad = copy_case(sizes.data(), (int)sizes.size(), nthreads, s);
            if (bad) { printf("span %d wrong (%d threads, case %d)\n", bad, nthreads, cases); return 1; }
            ++cases;
        }
    printf("span copy: %d cases OK\n", cases);
    return 0;
}
#else

extern "C" {

int64_t tr_copy_threshold() { return (int64_t)XD_COPY_THREADED_FROM; }
int tr_copy_case(const int64_t* sizes, int n, int nthreads, uint32_t seed) { return copy_case(sizes, n, nthreads, seed); }

// args: dem_ok, planes_ok, dem_dtype, H, W, row_stride, halo_top, halo_bottom, fit, curv, mask, tri, window, out_dtype, memspace
int tr_validate(const int64_t* a, double resolution, char* msg, int msg_cap) {
    static const int one = 1;
    const TerrainCheck c = terrain_validate(a[0] ? &one : nullptr, a[1] ? &one : nullptr, (int)a[2], a[3], a[4], a[5], a[6], a[7], resolution,
                                            (int)a[8], (int)a[9], (uint32_t)a[10], (int)a[11], (int)a[12], (int)a[13], (int)a[14]);
    snprintf(msg, (size_t)msg_cap, "%s", c.msg);
    return c.code;
}

// rows of 12 inputs: dem_dtype, out_dtype, mask, fit, curv, tri, degrees, hs_z (as an integer), unclipped, window, terrain_math,
// terrain_stream -> rows of 8 outputs: family, fit, curv, fuse_win, tail, try_stream, mask, window_mask
void tr_route_bulk(const int32_t* in, int64_t n, int32_t* out) {
    for (int64_t i = 0; i < n; ++i) {
        const int32_t* a = in + 12 * i;
        const TerrainCall c = {a[0], a[1], (uint32_t)a[2], a[3], a[4], a[5], a[6], (double)a[7], a[8], a[9]};
        const TerrainRoute r = terrain_route(c, TerrainOptions{a[10], a[11]});
        int32_t* o = out + 8 * i;
        o[0] = r.family; o[1] = r.fit; o[2] = r.curv; o[3] = r.fuse_win; o[4] = r.tail; o[5] = r.try_stream; o[6] = (int32_t)r.mask;
        o[7] = (int32_t)r.window_mask;
    }
}
void tr_families(int32_t* out) {
    const int f[10] = {TF_NONE, TF_FULL11_GEO, TF_FULL11_DIR, TF_SAH_WIN, TF_SLOPE, TF_SLOPE_ASPECT, TF_HILLSHADE, TF_SAH, TF_RUNTIME, TF_RUNTIME_F64};
    for (int i = 0; i < 10; ++i) out[i] = f[i];
}

// geom: H, W, row_stride, halo_top, halo_bottom -> out: ok, tx0, tx1, ty0, ty1, xi0, yi0, yi1, band_height, groups_x, nbands, ngroups,
// grid8, perm_mul, strips, frame
void tr_plan_strips(const int64_t* geom, int aligned, int halo, int terrain_stream, int64_t* out) {
    const RasterGeom g = {geom[0], geom[1], geom[2], geom[3], geom[4]};
    const StripPlan p = plan_strips(g, aligned != 0, halo, terrain_stream);
    const int64_t v[16] = {p.ok, p.fr.tx0, p.fr.tx1, p.fr.ty0, p.fr.ty1, p.xi0, p.yi0, p.yi1, p.band_height, p.groups_x, p.nbands, p.ngroups,
                           p.grid8, p.perm_mul, p.strips, p.frame};
    for (int i = 0; i < 16; ++i) out[i] = v[i];
}

// out: lds, too_tall, lds_bytes, grid_x, grid_y
void tr_plan_window(int64_t H, int64_t W, int w, int in_elem, int opt_lds, int64_t* out) {
    const WindowPlan p = plan_window(H, W, w, (size_t)in_elem, opt_lds);
    out[0] = p.lds; out[1] = p.too_tall; out[2] = (int64_t)p.lds_bytes; out[3] = p.grid_x; out[4] = p.grid_y;
}

int tr_halo_depth(uint32_t mask, int fit, int w) { return terrain_halo_depth(mask, fit, w); }

// args: H, W, halo_top, halo_bottom, depth, n_planes, in_es, out_es, host_chunk_mb, host_chunk_rows; `halvings` calls of halved()
// first.  head: rows, in_bytes, plane_bytes, out_bytes, halvings that took; chunks: rows of r0, r1, top, bot; returns their count (or
// -count if there are more than `cap`)
int64_t tr_host_chunks(const int64_t* a, int halvings, int64_t* head, int64_t* chunks, int64_t cap) {
    HostChunks p = plan_host_chunks(a[0], a[1], a[2], a[3], (int)a[4], (int)a[5], (size_t)a[6], (size_t)a[7], (int)a[8], (int)a[9]);
    int took = 0;
    for (int i = 0; i < halvings; ++i) took += p.halved() ? 1 : 0;
    head[0] = p.rows; head[1] = (int64_t)p.in_bytes(); head[2] = (int64_t)p.plane_bytes(); head[3] = (int64_t)p.out_bytes(); head[4] = took;
    const std::vector<HostChunk> l = p.list();
    if ((int64_t)l.size() > cap) return -(int64_t)l.size();
    for (size_t i = 0; i < l.size(); ++i) { chunks[4 * i] = l[i].r0; chunks[4 * i + 1] = l[i].r1; chunks[4 * i + 2] = l[i].top; chunks[4 * i + 3] = l[i].bot; }
    return (int64_t)l.size();
}

}  // extern "C"
#endif
