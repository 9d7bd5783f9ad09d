// terrain_host.hip -- xdemhip_terrain for HOST buffers: the raster streams through the device in ROW CHUNKS with the overlap the
// requested attributes need (the GPU analogue of the reference's map_overlap tiles, xdem/terrain/terrain.py:412-466): device memory
// stays bounded however large the host raster is, and a chunk is computed exactly as the same rows of the whole raster (halo_top /
// halo_bottom of the kernels).  A double-buffered pipeline over PINNED staging buffers owned by the context --
//   copy threads: caller's rows -> pinned in[k & 1]      |  H2D (copy stream 0)  |  kernels (context stream)
//   D2H (copy stream 1) -> pinned out[k & 1]             |  copy threads: pinned out -> caller's planes
// with chunk k's transfers and kernels running while the threads move chunk k - 1's planes into the caller's (pageable, often
// never-touched) arrays: the PCIe link stays busy in both directions instead of idling behind a pageable copy.
// The chunk plan is terrain_route.h's (plan_host_chunks); this file holds the stages that act on it and their driver.
#include "common.h"
#include "host_copy.h"
#include "terrain_route.h"

namespace xd {
namespace {

struct XdEvents {   // the events of one call, destroyed with the scope
    std::vector<hipEvent_t> owned;
    hipEvent_t create() {
        hipEvent_t e = nullptr;
        if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return nullptr;
        owned.push_back(e);
        return e;
    }
    ~XdEvents() { for (hipEvent_t e : owned) (void)hipEventDestroy(e); }
    XdEvents() = default;
    XdEvents(const XdEvents&) = delete;
    XdEvents& operator=(const XdEvents&) = delete;
};

struct HostRun {   // what the stages share; buffers and events by pipeline slot q = k & 1
    xdemhip_ctx* ctx;
    TerrainLaunch L;              // the call; dem / planes / H / halos are set per chunk
    const char* dem;              // caller's buffer and its geometry
    int64_t row_stride, halo_top;
    void* const* out_planes;
    int n_planes;
    HostChunks plan;
    std::vector<HostChunk> chunks;
    void* d_in[2];
    void* d_out[2];
    hipEvent_t ev_in[2], ev_comp[2], ev_out[2];
    hipStream_t s_h2d, s_d2h;
    size_t rows_bytes(const HostChunk& g) const { return (size_t)(g.r1 - g.r0) * (size_t)plan.W * plan.out_es; }   // one plane's rows of a chunk
};

void drop_staging(xdemhip_ctx* ctx) {
    for (int q = 0; q < 2; ++q) {
        if (ctx->stage_in[q]) (void)hipHostFree(ctx->stage_in[q]);
        if (ctx->stage_out[q]) (void)hipHostFree(ctx->stage_out[q]);
        ctx->stage_in[q] = ctx->stage_out[q] = nullptr;
    }
    ctx->stage_in_bytes = ctx->stage_out_bytes = 0;
}

// Pinned staging, kept by the context between calls (pinning hundreds of MiB costs more than moving them).  The budget sizes
// 2 x (input + planes) of pinned host memory AND the same of device memory; where the host cannot pin that much the chunk is
// halved until it can (down to 64 rows) instead of failing the call.  Option "host_release" frees the staging buffers.
int ensure_staging(xdemhip_ctx* ctx, HostChunks& plan) {
    if (ctx->stage_in_bytes >= plan.in_bytes() && ctx->stage_out_bytes >= plan.out_bytes()) return XDEMHIP_OK;
    for (;;) {
        drop_staging(ctx);
        bool ok = true;
        for (int q = 0; q < 2 && ok; ++q)
            ok = hipHostMalloc(&ctx->stage_in[q], plan.in_bytes(), hipHostMallocDefault) == hipSuccess &&
                 hipHostMalloc(&ctx->stage_out[q], plan.out_bytes(), hipHostMallocDefault) == hipSuccess;
        if (ok) break;
        (void)hipGetLastError();
        drop_staging(ctx);
        if (!plan.halved()) return xd_fail(ctx, XDEMHIP_ENOMEM, "hipHostMalloc(staging) failed even for 64-row chunks");
    }
    ctx->stage_in_bytes = plan.in_bytes();
    ctx->stage_out_bytes = plan.out_bytes();
    return XDEMHIP_OK;
}

// device buffers and events of the two pipeline slots, owned by the caller's scopes
int acquire_device(HostRun& R, XdBuffers& buf, XdEvents& events) {
    for (int q = 0; q < 2; ++q) {
        R.d_in[q] = buf.alloc(R.plan.in_bytes());
        R.d_out[q] = buf.alloc(R.plan.out_bytes());
        R.ev_in[q] = events.create();
        R.ev_comp[q] = events.create();
        R.ev_out[q] = events.create();
        if (!R.d_in[q] || !R.d_out[q] || !R.ev_in[q] || !R.ev_comp[q] || !R.ev_out[q])
            return xd_fail(R.ctx, XDEMHIP_ENOMEM, "hipMalloc / hipEventCreate (host path) failed");
    }
    return XDEMHIP_OK;
}

// caller's rows of chunk k -> pinned in[q] (row stride squeezed out), then H2D; the context's stream waits for it
int stage_in(HostRun& R, int k) {
    const HostChunk& g = R.chunks[k];
    const int q = k & 1;
    const int64_t in_rows = g.top + (g.r1 - g.r0) + g.bot;
    const size_t row = (size_t)R.plan.W * R.plan.in_es, src_row = (size_t)R.row_stride * R.plan.in_es;
    const char* src = R.dem + (size_t)(g.r0 + R.halo_top - g.top) * src_row;
    char* dst = static_cast<char*>(R.ctx->stage_in[q]);
    std::vector<XdSpan> spans;
    if (R.row_stride == R.plan.W) spans.push_back({dst, src, (size_t)in_rows * row});
    else
        for (int64_t r = 0; r < in_rows; ++r) spans.push_back({dst + (size_t)r * row, src + (size_t)r * src_row, row});
    xd_parallel_copy(spans, R.ctx->host_copy_threads);
    if (hipMemcpyAsync(R.d_in[q], R.ctx->stage_in[q], (size_t)in_rows * row, hipMemcpyHostToDevice, R.s_h2d) != hipSuccess ||
        hipEventRecord(R.ev_in[q], R.s_h2d) != hipSuccess || hipStreamWaitEvent(R.ctx->stream, R.ev_in[q], 0) != hipSuccess)
        return xd_fail(R.ctx, XDEMHIP_EHIP, "H2D copy failed");
    return XDEMHIP_OK;
}

// the kernels of chunk k on the context's stream (the first and the last chunk carry the timing events)
int launch_chunk(HostRun& R, int k) {
    const HostChunk& g = R.chunks[k];
    const int q = k & 1;
    R.L.dem = R.d_in[q];
    for (int bit = 0, i = 0; bit < XDEMHIP_ATTR_COUNT; ++bit)
        if (R.L.attr_mask & (1u << bit)) R.L.planes[bit] = static_cast<char*>(R.d_out[q]) + (size_t)(i++) * R.plan.plane_bytes();
    R.L.H = g.r1 - g.r0; R.L.halo_top = g.top; R.L.halo_bottom = g.bot;
    if (k == 0) (void)hipEventRecord(R.ctx->ev_start, R.ctx->stream);
    const int rc = launch_terrain(R.ctx, R.L);
    if (rc != XDEMHIP_OK) return rc;
    if (k == (int)R.chunks.size() - 1) (void)hipEventRecord(R.ctx->ev_stop, R.ctx->stream);
    return XDEMHIP_OK;
}

// chunk k's planes: device -> pinned out[q] on the D2H stream, after its kernels
int fetch_planes(HostRun& R, int k) {
    const int q = k & 1;
    const size_t nb = R.rows_bytes(R.chunks[k]), plane = R.plan.plane_bytes();
    hipError_t e = hipEventRecord(R.ev_comp[q], R.ctx->stream);
    if (e == hipSuccess) e = hipStreamWaitEvent(R.s_d2h, R.ev_comp[q], 0);
    for (int i = 0; i < R.n_planes && e == hipSuccess; ++i)   // (a short last chunk leaves gaps between its planes: one copy per plane)
        e = hipMemcpyAsync(static_cast<char*>(R.ctx->stage_out[q]) + (size_t)i * plane,
                           static_cast<const char*>(R.d_out[q]) + (size_t)i * plane, nb, hipMemcpyDeviceToHost, R.s_d2h);
    if (e == hipSuccess) e = hipEventRecord(R.ev_out[q], R.s_d2h);
    return e == hipSuccess ? XDEMHIP_OK : xd_fail(R.ctx, XDEMHIP_EHIP, "D2H copy failed");
}

// chunk k's planes: pinned staging -> caller's arrays (after its D2H has landed)
int drain(HostRun& R, int k) {
    const HostChunk& g = R.chunks[k];
    const int q = k & 1;
    if (hipEventSynchronize(R.ev_out[q]) != hipSuccess) return xd_fail(R.ctx, XDEMHIP_EHIP, "D2H copy failed");
    std::vector<XdSpan> spans;
    for (int i = 0; i < R.n_planes; ++i)
        spans.push_back({static_cast<char*>(R.out_planes[i]) + (size_t)g.r0 * (size_t)R.plan.W * R.plan.out_es,
                         static_cast<const char*>(R.ctx->stage_out[q]) + (size_t)i * R.plan.plane_bytes(), R.rows_bytes(g)});
    xd_parallel_copy(spans, R.ctx->host_copy_threads);
    return XDEMHIP_OK;
}

}  // namespace

// `L`: the call as xdemhip_terrain filled it (the caller's geometry, no pointers); `dem`, `out_planes`: the caller's host arrays
int terrain_host(xdemhip_ctx* ctx, const TerrainLaunch& L, const void* dem, void* const* out_planes) {
    HostRun R = {};
    R.ctx = ctx; R.L = L;
    R.dem = static_cast<const char*>(dem); R.row_stride = L.row_stride; R.halo_top = L.halo_top;
    R.out_planes = out_planes; R.n_planes = __builtin_popcount(L.attr_mask);
    R.s_h2d = ctx->copy_streams[0]; R.s_d2h = ctx->copy_streams[1];
    R.plan = plan_host_chunks(L.H, L.W, L.halo_top, L.halo_bottom, terrain_halo_depth(L.attr_mask, L.surface_fit, L.window_size), R.n_planes,
                              L.dem_dtype == XDEMHIP_F32 ? 4 : 8, L.out_dtype == XDEMHIP_F32 ? 4 : 8, ctx->host_chunk_mb, ctx->host_chunk_rows);
    int rc = ensure_staging(ctx, R.plan);
    if (rc != XDEMHIP_OK) return rc;
    XdBuffers buf(ctx, "xdemhip_terrain");
    XdEvents events;
    rc = acquire_device(R, buf, events);
    if (rc != XDEMHIP_OK) return rc;
    R.chunks = R.plan.list();
    R.L.row_stride = L.W;   // (staging squeezes the caller's stride out)
    const int nchunks = (int)R.chunks.size();
    for (int k = 0; k < nchunks && rc == XDEMHIP_OK; ++k) {
        // (buffers k & 1 are free: chunk k - 2 was drained two iterations ago, which followed its kernels and copies)
        rc = stage_in(R, k);
        if (rc == XDEMHIP_OK) rc = launch_chunk(R, k);
        if (rc == XDEMHIP_OK) rc = fetch_planes(R, k);
        // while the device works on chunk k, move chunk k - 1's planes into the caller's arrays
        if (rc == XDEMHIP_OK && k > 0) rc = drain(R, k - 1);
    }
    if (rc == XDEMHIP_OK) rc = drain(R, nchunks - 1);
    if (rc != XDEMHIP_OK) { (void)hipStreamSynchronize(R.s_h2d); (void)hipStreamSynchronize(R.s_d2h); }
    ctx->timed = (rc == XDEMHIP_OK);
    const hipError_t e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess && rc == XDEMHIP_OK) rc = xd_fail(ctx, XDEMHIP_EHIP, std::string("kernel failed: ") + hipGetErrorString(e));
    return rc;
}

}  // namespace xd
