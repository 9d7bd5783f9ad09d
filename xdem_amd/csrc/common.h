// common.h -- context object and helpers shared by the C-ABI translation units of libxdemhip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <string>
#include <thread>
#include <vector>

#include "../../include/xdemhip.h"

struct xdemhip_ctx {
    int device = 0;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;  // stream work is enqueued on (own_stream or the caller's)
    hipEvent_t ev_start = nullptr, ev_stop = nullptr, ev_copy = nullptr;
    static constexpr int MAX_COPY_THREADS = 16;
    hipStream_t copy_streams[MAX_COPY_THREADS] = {};  // one per copy thread of the host-buffer path
    int host_copy_threads = 8;                        // option "host_copy_threads"
    void* stage_in[2] = {nullptr, nullptr};            // pinned staging of the host-buffer terrain path (double-buffered), kept between calls
    void* stage_out[2] = {nullptr, nullptr};
    size_t stage_in_bytes = 0, stage_out_bytes = 0;
    int pairs_launch_cap = 0;                         // option "pairs_launch_cap": workgroups per pair-kernel launch (0 = 2^31 / NT; CPD: 2^32 pair evaluations)
    bool timed = false;
    int num_cu = 256;
    xdemhip_allreduce_fn allreduce = nullptr;  // multi-GPU hook (null: single process)
    void* allreduce_user = nullptr;
    xdemhip_allreduce_device_fn allreduce_dev = nullptr;  // device-side form of the hook (device arrays stay on the device)
    void* allreduce_dev_user = nullptr;
    int64_t n_red_host = 0, n_red_dev = 0;     // reductions that went through the host / the device hook
    int rank = 0, world = 0;                   // xdemhip_set_rank: this process's place among the ranks the hooks reduce over (world 0: not told)
    int nk_fused_dist = 1;   // option "nk_fused_dist": 1 partitioned Nuth-Kaab plans (reduction hook + xdemhip_set_rank) take the one-pass step too: 5-10 all-reduces per step (default), 0 the plain route
    int host_chunk_rows = 0; // option "host_chunk_rows": rows per chunk of host-buffer terrain calls (0 = from the budget); the mp_config tile size
    int host_chunk_mb = 0;   // device budget (MiB) of one row chunk of host-buffer terrain calls; 0 = default
    int nk_narrow = -1;      // option "nk_narrow": sample brackets of the one-pass Nuth-Kaab step 2^-k as wide as the rule (-1 = adaptive: from the offsets measured in earlier steps)
    int vario_runs = 1;      // option "vario_runs": run-length counting pass of the bracketed Dowd selection when a Morton-ordered copy is linked (0 = per-pair counters)
    int vario_sort = 1;      // option "vario_sort": the Python side uploads the points of a pair block in Morton order (run-length accumulation of the pair kernels)
    int nk_predict = 1;      // option "nk_predict": 1 a settled one-pass Nuth-Kaab step takes its brackets from the previous step's exact medians moved by the model (no sample kernels, no digit passes over samples; default), 0 every step samples
    int nk_fused = 1;        // option "nk_fused": 1 the Nuth-Kaab step of large single-GPU plans is ONE data pass (14 B/pixel: dh, its median's counting and the aspect-bin counting against sample brackets with per-pixel margins; default), 0 the two passes of round 3
    int terrain_stream = 1;  // option "terrain_stream": 1 streaming strips for the raster interior where they apply (default), 0 tiles only; 128 / 256 / 512 = band height
    int terrain_order = 0;   // option "terrain_order": 0 one band of tiles per XCD (default), 1 natural order (XCDs interleave along a tile row); strips only: 2 permuted, 3 column-major (measurement)
    int terrain_window_lds = 1;  // option "terrain_window_lds": 1 LDS-tiled window kernel for window sizes != 3 (default), 0 the per-pixel form (its check)
    int terrain_ring_wait = 0;  // option "terrain_ring_wait": 1 = the streaming strips drain every VMEM operation before reading a refilled ring block (test switch for the counted wait)
    int terrain_nonfinite = 0;  // option "terrain_nonfinite": 0 an output is NaN iff its full window holds a non-finite value (SciPy engine, default), 1 the Numba engine's rule: +-Inf pixels go through the arithmetic (terrain_nonfinite.hip)
    int* nf_flag = nullptr;  // device word of that path: "the rows at hand hold an infinite pixel"
    int terrain_math = 2;    // option "terrain_math": float32 rasters: 2 lean tail for the specialised attribute sets (default), 0 mixed-precision tail of round 2, 1 float64 tail everywhere
    int vario_grid = 1;      // option "vario_grid": 1 = integer-lattice pair kernels for raster-sampled points (default), 0 = always float64 coordinates
    int vario_edge = 0;      // option "vario_edge": lag classes 0 = [e_{k-1}, e_k) (default), 1 = (e_{k-1}, e_k]
    int vario_diff = 0;      // option "vario_diff": |dv| formed 0 = in the value dtype (default), 1 = in float64 (float32 values are widened)
    int nk_nan_rule = 0;     // option "nk_nan_rule": nodata spreading of the bilinear taps (nuthkaab.hip): 0 4tap, 1 weighted, 2 dilate3x3, 3 dilate_cross
    int pts_tile_order = 0;  // test switch "pts_tile_order": 1 the gather of a raster-point plan walks its points by raster tile, 0 in cloud order (ptsplan.hip)
    int hypso_seg_lds = 0;   // test switch "hypso_seg_lds": longest segment of xdemhip_hypso_segments sorted in LDS (values; 0 = 8192), longer ones take the radix selection
    int bw_seg_lds = 0;      // test switch "bw_seg_lds": longest (tile, bin) segment of xdemhip_bw_nk_step sorted in LDS (values; 0 = 4096), longer ones take the radix selection
    int vec_seg_reg = 0;     // test switch "vec_seg_reg": longest crossing segment of xdemhip_rasterize sorted in one lane's registers (0 = 8), longer ones go to a workgroup
    int vec_seg_lds = 0;     // test switch "vec_seg_lds": longest crossing segment of xdemhip_rasterize one workgroup sorts in LDS (0 = 4096), longer ones are sorted in place in global memory
    int vec_stage_times = 0; // test switch "vec_stage_times": 1 xdemhip_rasterize records an event at every stage's start (measurement: xdemhip_rasterize_stage_ms)
    int regrid_route = 0;    // test switch "regrid_route": 0 xdemhip_regrid picks its route by the LDS budget, 1 the tiled route wherever the footprint fits, 2 the per-pixel route always
    int edt_route = 0;       // test switch "edt_route": 0 the row pass of xdemhip_edt scans an LDS window first, 1 global block search only, 2 minimal band / tile / halo / block
    int spline_route = 0;    // test switch "spline_route": prefilter of xdemhip_spline_prepare: 0 banded columns and LDS rows where a row is longer than its halos, 1 one band per column, 2 plain rows always, 3 LDS rows always
    int ccl_route = 0;       // test switch "ccl_route": tiles of xdemhip_label: 0 automatic (64 x 64), 2 minimal (2 x 2): small planes cross every tile border
    int filter_route = 0;    // test switch "filter_route": xdemhip_filter: 0 tiled while tile and halo fit the LDS budget, 1 the same pinned, 2 taps from global memory always, 3 minimal tiles (4 x 8)
    float ccl_stage_ms[11] = {};              // device time of the stages of the last xdemhip_label (5) and xdemhip_outlines (6) calls (xdemhip_ccl_stage_ms)
    int64_t ccl_launches = 0, ccl_stage_launches[2] = {0, 0};   // kernels launched by the call at hand; by the last xdemhip_label / xdemhip_outlines call
    float edt_stage_ms[4] = {0, 0, 0, 0};      // device time of the four passes (down, carry, up, row) of the last xdemhip_edt call
    float vec_stage_ms[5] = {0, 0, 0, 0, 0};   // device time of the five stages of the last xdemhip_rasterize call made under that switch
    int64_t vec_launches = 0;   // kernels launched by the last xdemhip_rasterize / xdemhip_rasterize_union call (xdemhip_rasterize_launches)
    int selection_mode = 0;  // 0 auto (bracketed for large inputs), 1 plain digit passes only, 2 degenerate brackets (tests the
                             // fallback), 3 bracketed whatever the per-bin sample size (2 and 3: test switches)
    // Deferred device-to-host results (xd_d2h / xd_sync below): small result blocks land in one pinned staging buffer with
    // truly asynchronous copies and are handed to their destinations at the next xd_sync -- a copy into pageable memory
    // would stall the host once per block (tens of microseconds each, a dozen blocks per Nuth-Kaab step).
    unsigned char* pin = nullptr;
    size_t pin_cap = 0, pin_used = 0;
    struct Pending { void* dst; size_t off, bytes; };
    std::vector<Pending> pending;
    int64_t plan_bytes = 0;  // device bytes the plans of this context hold (XdOwned below; read by xdemhip_plan_bytes only)
    std::string err;
};

#define XD_HIP_CHECK(ctx, expr)                                                                   \
    do {                                                                                          \
        hipError_t _e = (expr);                                                                   \
        if (_e != hipSuccess) {                                                                   \
            char _b[512];                                                                         \
            snprintf(_b, sizeof _b, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
            (ctx)->err = _b;                                                                      \
            return XDEMHIP_EHIP;                                                                  \
        }                                                                                         \
    } while (0)

inline int xd_fail(xdemhip_ctx* ctx, int code, const std::string& msg) {
    if (ctx) ctx->err = msg;
    return code;
}

// after one or more kernel launches: XDEMHIP_OK, or XDEMHIP_EHIP with "`what` launch failed"
inline int launched(xdemhip_ctx* ctx, const char* what) {
    return hipGetLastError() == hipSuccess ? XDEMHIP_OK : xd_fail(ctx, XDEMHIP_EHIP, std::string(what) + " launch failed");
}

inline int xd_sync(xdemhip_ctx* ctx);

// The device buffers of one call.  alloc() gives a buffer for the length of the scope.  input() and output() give the device side of a
// caller's array (sizes in bytes, the pointer's type kept): the array itself where it is on the device (XDEMHIP_DEVICE), else a
// buffer of the scope, the upload queued on the context's stream at once and the download by finish().  A null array stays null.  A
// failure returns nullptr and sets `rc`: XDEMHIP_ENOMEM with "hipMalloc failed (`who`)" and HIP's last error cleared, XDEMHIP_EHIP
// for a copy; after a failure every further request returns nullptr, so a call site asks for all it needs and looks at `rc` once.
// finish() ends a call that went well: the downloads are queued and, if the scope owns anything, the stream is waited for (xd_sync,
// its status returned) and the buffers freed.  On every other path the end of the scope does the same without a status.  A scope
// that owns nothing does nothing, which keeps device routes asynchronous.  Host destinations of copies queued on the stream, other
// than the caller's own arrays, are declared BEFORE it, so that they outlive that synchronisation on every return path.
struct XdBuffers {
    xdemhip_ctx* ctx;
    const char* who;
    int rc = XDEMHIP_OK;
    struct Out { void* host; const void* dev; size_t bytes; };
    std::vector<void*> owned;
    std::vector<Out> outs;
    XdBuffers(xdemhip_ctx* c, const char* w) : ctx(c), who(w) {}
    void* alloc(size_t bytes) {
        void* p = nullptr;
        if (rc != XDEMHIP_OK) return nullptr;
        if (hipMalloc(&p, bytes) != hipSuccess) {
            (void)hipGetLastError();
            rc = xd_fail(ctx, XDEMHIP_ENOMEM, std::string("hipMalloc failed (") + who + ")");
            return nullptr;
        }
        if (p) owned.push_back(p);
        return p;
    }
    template <typename T> T* alloc(size_t count) { return static_cast<T*>(alloc(count * sizeof(T))); }
    template <typename T> const T* input(const T* src, size_t bytes, int memspace) {
        if (memspace == XDEMHIP_DEVICE || !src) return src;
        T* d = static_cast<T*>(alloc(bytes));
        if (d && hipMemcpyAsync(d, src, bytes, hipMemcpyHostToDevice, ctx->stream) != hipSuccess) {
            rc = xd_fail(ctx, XDEMHIP_EHIP, std::string("H2D copy failed (") + who + ")");
            return nullptr;
        }
        return d;
    }
    template <typename T> T* output(T* dst, size_t bytes, int memspace) {
        if (memspace == XDEMHIP_DEVICE || !dst) return dst;
        T* d = static_cast<T*>(alloc(bytes));
        if (d) outs.push_back({dst, d, bytes});
        return d;
    }
    int finish() {
        for (const Out& o : outs)
            if (rc == XDEMHIP_OK && hipMemcpyAsync(o.host, o.dev, o.bytes, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess)
                rc = xd_fail(ctx, XDEMHIP_EHIP, std::string("D2H copy failed (") + who + ")");
        if (owned.empty()) return rc;
        const int synced = xd_sync(ctx);
        if (rc == XDEMHIP_OK) rc = synced;
        free_all();
        return rc;
    }
    // free one buffer of the scope now (the queued work that uses it is waited for); a pointer the scope does not own is left alone
    void release(const void* p) {
        for (size_t i = 0; i < owned.size(); ++i)
            if (owned[i] == p) {
                (void)hipStreamSynchronize(ctx->stream);
                (void)hipFree(owned[i]);
                owned.erase(owned.begin() + (ptrdiff_t)i);
                return;
            }
    }
    ~XdBuffers() {
        if (owned.empty()) return;
        (void)hipStreamSynchronize(ctx->stream);
        free_all();
    }
    void free_all() {
        for (void* p : owned) (void)hipFree(p);
        owned.clear();
    }
    XdBuffers(const XdBuffers&) = delete;
    XdBuffers& operator=(const XdBuffers&) = delete;
};

// The device buffers a plan keeps from create to destroy; the plan struct holds one by value.  take() gives a buffer for the life of
// the owner (a zero-byte request still a valid pointer).  keep() gives the device side of an array the plan goes on reading: the
// caller's array itself where it is on the device (XDEMHIP_DEVICE; not owned), else an owned copy with the upload queued on the
// context's stream.  A failure returns nullptr, clears HIP's last error and sets `rc` (XDEMHIP_ENOMEM "hipMalloc failed (`who`)",
// XDEMHIP_EHIP "H2D copy failed (`who`)"); after it every further request returns nullptr, so a call site asks for all it needs
// and looks once: at `rc` in a constructor, whose plan dies with the failure, at status() in a step, which hands the owner back
// ready for the next call.  Buffers a plan can do without are taken between optional() and all_or_none(): if one of them fails,
// all of them are freed, the pointers named are nulled and `rc` stays clear.  drop() frees one buffer now and regrow() replaces
// it, both after waiting for the stream; a pointer the owner does not own is left alone.  release(), and the end of the owner,
// free everything after that wait.  ctx->plan_bytes counts the bytes asked for that are still held.
struct XdOwned {
    struct Buf { void* p; size_t bytes; };
    xdemhip_ctx* ctx = nullptr;
    int rc = XDEMHIP_OK;
    std::vector<Buf> owned;
    size_t opt_from = 0;
    bool in_opt = false, opt_failed = false;
    void* take(size_t bytes, const char* who) {
        void* p = nullptr;
        if (rc != XDEMHIP_OK || (in_opt && opt_failed)) return nullptr;
        if (hipMalloc(&p, bytes ? bytes : 8) != hipSuccess) {
            (void)hipGetLastError();
            if (in_opt) opt_failed = true;
            else rc = xd_fail(ctx, XDEMHIP_ENOMEM, std::string("hipMalloc failed (") + who + ")");
            return nullptr;
        }
        owned.push_back({p, bytes});
        ctx->plan_bytes += (int64_t)bytes;
        return p;
    }
    template <typename T> T* take(size_t count, const char* who) { return static_cast<T*>(take(count * sizeof(T), who)); }
    template <typename T> T* keep(const T* src, size_t bytes, int memspace, const char* who) {
        if (memspace == XDEMHIP_DEVICE || !src) return const_cast<T*>(src);
        T* d = static_cast<T*>(take(bytes, who));
        if (d && hipMemcpyAsync(d, src, bytes, hipMemcpyHostToDevice, ctx->stream) != hipSuccess) {
            (void)hipGetLastError();
            drop(d);
            rc = xd_fail(ctx, XDEMHIP_EHIP, std::string("H2D copy failed (") + who + ")");
            return nullptr;
        }
        return d;
    }
    void optional() { opt_from = owned.size(); in_opt = true; opt_failed = rc != XDEMHIP_OK; }
    template <typename... T> bool all_or_none(T*&... ptrs) {
        in_opt = false;
        if (!opt_failed) return true;
        if (owned.size() > opt_from) (void)hipStreamSynchronize(ctx->stream);
        while (owned.size() > opt_from) free_last();
        ((ptrs = nullptr), ...);
        return false;
    }
    void drop(const void* p) {
        for (size_t i = 0; p && i < owned.size(); ++i)
            if (owned[i].p == p) {
                (void)hipStreamSynchronize(ctx->stream);
                std::swap(owned[i], owned.back());
                free_last();
                return;
            }
    }
    template <typename T> bool regrow(T*& p, size_t bytes, const char* who) {
        drop(p);
        p = static_cast<T*>(take(bytes, who));
        return p != nullptr;
    }
    int status() { const int r = rc; rc = XDEMHIP_OK; return r; }
    void release() {
        if (owned.empty()) return;
        (void)hipSetDevice(ctx->device);
        (void)hipStreamSynchronize(ctx->stream);
        while (!owned.empty()) free_last();
    }
    void free_last() {
        (void)hipFree(owned.back().p);
        ctx->plan_bytes -= (int64_t)owned.back().bytes;
        owned.pop_back();
    }
    XdOwned() = default;
    explicit XdOwned(xdemhip_ctx* c) : ctx(c) {}
    ~XdOwned() { release(); }
    XdOwned(const XdOwned&) = delete;
    XdOwned& operator=(const XdOwned&) = delete;
};

// "This selection is local": the reduction hook is off for the length of the scope (one process's values, a single-device helper).
struct XdLocalSelection {
    xdemhip_ctx* ctx;
    xdemhip_allreduce_fn hook;
    explicit XdLocalSelection(xdemhip_ctx* c) : ctx(c), hook(c->allreduce) { ctx->allreduce = nullptr; }
    ~XdLocalSelection() { ctx->allreduce = hook; }
    XdLocalSelection(const XdLocalSelection&) = delete;
    XdLocalSelection& operator=(const XdLocalSelection&) = delete;
};

// Queue a small device-to-host copy whose destination is filled by the next xd_sync(ctx) (falls back to a plain copy when
// the staging buffer is full).  `dst` must stay alive until that xd_sync; xd_drop_pending forgets undelivered blocks (entry
// points call it on their way in and out, so an error return never leaves a dangling destination behind).
inline void xd_drop_pending(xdemhip_ctx* ctx) {
    ctx->pending.clear();
    ctx->pin_used = 0;
}
inline int xd_d2h(xdemhip_ctx* ctx, void* dst, const void* dsrc, size_t bytes) {
    if (!ctx->pin) {
        if (hipHostMalloc(reinterpret_cast<void**>(&ctx->pin), 256 * 1024, hipHostMallocDefault) == hipSuccess) ctx->pin_cap = 256 * 1024;
        else ctx->pin = nullptr;
    }
    const size_t need = (bytes + 15) & ~(size_t)15;
    if (!ctx->pin || ctx->pin_used + need > ctx->pin_cap) {
        XD_HIP_CHECK(ctx, hipMemcpyAsync(dst, dsrc, bytes, hipMemcpyDeviceToHost, ctx->stream));
        return XDEMHIP_OK;
    }
    if (hipMemcpyAsync(ctx->pin + ctx->pin_used, dsrc, bytes, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess) {
        xd_drop_pending(ctx);  // the operation is abandoned: nothing queued before may be delivered into dead destinations later
        return xd_fail(ctx, XDEMHIP_EHIP, "hipMemcpyAsync (deferred device-to-host copy) failed");
    }
    ctx->pending.push_back({dst, ctx->pin_used, bytes});
    ctx->pin_used += need;
    return XDEMHIP_OK;
}
// The same for results a KERNEL writes itself: a region of the pinned staging buffer (device-writable: pinned host memory is mapped)
// that the next xd_sync hands to `dst` -- saves the copy engine's launch behind the kernel.  nullptr: no room, use xd_d2h.
inline unsigned char* xd_pin_claim(xdemhip_ctx* ctx, void* dst, size_t bytes) {
    if (!ctx->pin) {
        if (hipHostMalloc(reinterpret_cast<void**>(&ctx->pin), 256 * 1024, hipHostMallocDefault) == hipSuccess) ctx->pin_cap = 256 * 1024;
        else { ctx->pin = nullptr; (void)hipGetLastError(); }
    }
    const size_t need = (bytes + 15) & ~(size_t)15;
    if (!ctx->pin || ctx->pin_used + need > ctx->pin_cap) return nullptr;
    unsigned char* at = ctx->pin + ctx->pin_used;
    ctx->pending.push_back({dst, ctx->pin_used, bytes});
    ctx->pin_used += need;
    return at;
}
// Pages of a caller's HOST output buffer made resident before a large device-to-host copy lands in them: a fresh np.empty is
// untouched virtual memory, and a copy that faults its pages in one by one runs at ~10 GB/s instead of the link's ~55.  `threads`
// threads write every page's first byte back to itself (contents kept); returns the threads for the caller to join -- the faults
// overlap whatever the device is still doing for this call.
struct XdPrefault {
    std::vector<std::thread> workers;
    void join() { for (auto& w : workers) if (w.joinable()) w.join(); workers.clear(); }
    ~XdPrefault() { join(); }
};
inline void xd_prefault_start(XdPrefault& pf, void* dst, size_t bytes, int threads) {
    if (!dst || bytes < ((size_t)64 << 20)) return;
    threads = threads < 1 ? 1 : (threads > 16 ? 16 : threads);
    const size_t per = (bytes + (size_t)threads - 1) / (size_t)threads;
    for (int t = 0; t < threads; ++t)
        pf.workers.emplace_back([=]() {
            volatile unsigned char* p = static_cast<volatile unsigned char*>(dst);
            const size_t lo = per * (size_t)t, hi = lo + per < bytes ? lo + per : bytes;
            for (size_t o = lo; o < hi; o += 4096) p[o] = p[o];
        });
}
inline int xd_sync(xdemhip_ctx* ctx) {
    const hipError_t e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) {
        xd_drop_pending(ctx);
        return xd_fail(ctx, XDEMHIP_EHIP, std::string("hipStreamSynchronize failed: ") + hipGetErrorString(e));
    }
    for (const auto& p : ctx->pending) memcpy(p.dst, ctx->pin + p.off, p.bytes);
    xd_drop_pending(ctx);
    return XDEMHIP_OK;
}
struct XdFetchScope {  // RAII for C entry points that queue deferred copies
    xdemhip_ctx* c;
    explicit XdFetchScope(xdemhip_ctx* ctx) : c(ctx) { if (c) xd_drop_pending(c); }
    ~XdFetchScope() { if (c) xd_drop_pending(c); }
};

// All-reduce a small device array over the ranks through the caller's hook (no-op without a hook): the array is
// staged to the host, combined by the hook (torch.distributed / RCCL or gloo on the Python side) and copied back.
inline int xd_allreduce_device(xdemhip_ctx* ctx, void* dptr, int64_t count, int kind) {
    if (!ctx->allreduce || count <= 0) return XDEMHIP_OK;
    if (ctx->allreduce_dev) {  // enqueued on the context's stream by the caller's hook: no staging, no host synchronisation
        ++ctx->n_red_dev;
        if (ctx->allreduce_dev(dptr, count, kind, static_cast<void*>(ctx->stream), ctx->allreduce_dev_user) != 0)
            return xd_fail(ctx, XDEMHIP_EHIP, "device all-reduce hook failed");
        return XDEMHIP_OK;
    }
    ++ctx->n_red_host;
    std::string buf((size_t)count * 8, '\0');
    hipError_t e = hipMemcpyAsync(&buf[0], dptr, buf.size(), hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return xd_fail(ctx, XDEMHIP_EHIP, "all-reduce staging (D2H) failed");
    if (ctx->allreduce(&buf[0], count, kind, ctx->allreduce_user) != 0) return xd_fail(ctx, XDEMHIP_EHIP, "all-reduce hook failed");
    e = hipMemcpyAsync(dptr, &buf[0], buf.size(), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return xd_fail(ctx, XDEMHIP_EHIP, "all-reduce staging (H2D) failed");
    return XDEMHIP_OK;
}

// A small HOST array through the host hook: the route agreements, made once per plan (like the per-step agreements of the selection
// routes they are not counted by xdemhip_reduction_calls, which counts the data reductions of the steps).
inline int xd_allreduce_host(xdemhip_ctx* ctx, void* hptr, int64_t count, int kind) {
    if (!ctx->allreduce || count <= 0) return XDEMHIP_OK;
    if (ctx->allreduce(hptr, count, kind, ctx->allreduce_user) != 0) return xd_fail(ctx, XDEMHIP_EHIP, "all-reduce hook failed");
    return XDEMHIP_OK;
}

// Launchers implemented in the kernel translation units.
namespace xd {
struct TerrainLaunch {
    const void* dem;     // device pointer to buffer row 0
    int dem_dtype, out_dtype;
    int64_t H, W, row_stride, halo_top, halo_bottom;
    double resolution;
    int surface_fit, curv_method, tri_method, window_size, degrees;
    int hs_unclipped;    // bit 1 of xdemhip_terrain's `degrees`: hillshade as the reference's ENGINE returns it (no clip to [0, 255])
    uint32_t attr_mask;
    double hs_alt, hs_az, hs_z;
    void* planes[XDEMHIP_ATTR_COUNT];  // device pointers by attribute bit (null when not requested)
};
int launch_terrain(xdemhip_ctx* ctx, const TerrainLaunch& L);
int terrain_host(xdemhip_ctx* ctx, const TerrainLaunch& L, const void* dem, void* const* out_planes);  // terrain_host.hip: host buffers, in row chunks
int launch_terrain_nonfinite(xdemhip_ctx* ctx, const TerrainLaunch& L);  // terrain_nonfinite.hip
// rugosity / fractal roughness (window_extra.hip); plane indexes of the two attributes
constexpr int P_RUGOSITY_IDX = 13, P_FRACTAL_IDX = 14;
int launch_window_extra(xdemhip_ctx* ctx, const TerrainLaunch& L);
int fractal_constants(int w, int* qs, double* x, double* m_x, double* ss_xx);
}  // namespace xd
