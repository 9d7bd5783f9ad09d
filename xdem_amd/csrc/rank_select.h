// rank_select.h -- the random subsample of the valid pixels, shared by xdemhip_nk_subsample and xdemhip_dh_subsample.
//
// What the caller's `rng.choice(np.flatnonzero(valid), k, replace=False)` selects, without the mask travelling to the host and back:
// the host draws RANKS (positions among the valid pixels in raster order), the device turns them into pixels.  The raster is cut
// into tiles of 4096 pixels; the pixels of a tile are counted, the counts scanned over the tiles, then every tile ranks its own
// valid pixels and looks their ranks up in the byte array of marked ranks.  A repeated rank marks one pixel.
#pragma once

#include <string>

#include "common.h"
#include "select_run.h"

namespace xd {
namespace {

constexpr int RANK_TILE = 4096;   // pixels per tile: 256 lanes x 16

// exclusive scan over the tile counts, in place; total in *total (one workgroup walks them in pieces of 1024 with a carry)
__global__ __launch_bounds__(1024) void rank_scan_kernel(unsigned long long* tile_cnt, int64_t n_tiles, unsigned long long* total) {
    __shared__ unsigned long long s[1024];
    __shared__ unsigned long long carry;
    if (threadIdx.x == 0) carry = 0ull;
    __syncthreads();
    for (int64_t b0 = 0; b0 < n_tiles; b0 += 1024) {
        const int64_t k = b0 + threadIdx.x;
        const unsigned long long v = k < n_tiles ? tile_cnt[k] : 0ull;
        s[threadIdx.x] = v;
        __syncthreads();
        for (int off = 1; off < 1024; off <<= 1) {
            const unsigned long long a = (int)threadIdx.x >= off ? s[threadIdx.x - off] : 0ull;
            __syncthreads();
            s[threadIdx.x] += a;
            __syncthreads();
        }
        if (k < n_tiles) tile_cnt[k] = carry + s[threadIdx.x] - v;
        __syncthreads();
        if (threadIdx.x == 1023) carry += s[1023];
        __syncthreads();
    }
    if (threadIdx.x == 0) *total = carry;
}

// mark[r] = 1 for every listed rank r in [0, n_ranks); the others are counted in *bad
__global__ __launch_bounds__(256) void rank_mark_kernel(const int64_t* __restrict__ ranks, int64_t k, int64_t n_ranks, uint8_t* __restrict__ mark,
                                                        unsigned long long* bad) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < k; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = ranks[i];
        if (r < 0 || r >= n_ranks) atomicAdd(bad, 1ull);
        else mark[r] = 1;
    }
}

// inclusive prefix sum of v over the 256 lanes of the workgroup (s: 256 ints of LDS, free again on return)
__device__ __forceinline__ int rank_block_scan(int v, int* s) {
    s[threadIdx.x] = v;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {
        const int a = (int)threadIdx.x >= off ? s[threadIdx.x - off] : 0;
        __syncthreads();
        s[threadIdx.x] += a;
        __syncthreads();
    }
    const int r = s[threadIdx.x];
    __syncthreads();
    return r;
}

enum class RankOut { Count, List, Mask };

// Selection of a tile's pixels: valid (a nonzero byte of `valid`), and -- with `mark` -- whose rank among the valid pixels is marked
// (valid_off: exclusive offsets of the valid pixels per tile).  Lane l of a tile holds pixels 16 l .. 16 l + 15.  What it writes:
//   Count: the number selected per tile into sel[tile];
//   List:  sel[] holds the scanned offsets of the selected pixels, their flat indexes go to idx[] in raster order;
//   Mask:  mask[p] = 1 for the selected pixels, 0 for the others (needs `mark`).
template <RankOut OUT>
__global__ __launch_bounds__(256) void rank_select_kernel(const uint8_t* __restrict__ valid, int64_t n, const unsigned long long* __restrict__ valid_off,
                                                          const uint8_t* __restrict__ mark, unsigned long long* __restrict__ sel,
                                                          int64_t* __restrict__ idx, uint8_t* __restrict__ mask) {
    const int64_t t0 = (int64_t)blockIdx.x * RANK_TILE + (int64_t)threadIdx.x * 16;
    const bool full = t0 + 16 <= n;
    uint8_t v[16];
    if (full) {
        const uint4 q = *reinterpret_cast<const uint4*>(valid + t0);   // (tiles start at multiples of 4096 bytes: aligned)
        const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int k = 0; k < 16; ++k) v[k] = ((w[k >> 2] >> (8 * (k & 3))) & 0xFFu) ? 1 : 0;
    } else {
#pragma unroll
        for (int k = 0; k < 16; ++k) v[k] = (t0 + k < n && valid[t0 + k]) ? 1 : 0;
    }
    __shared__ int s[256];
    if (mark) {
        int cv = 0;
#pragma unroll
        for (int k = 0; k < 16; ++k) cv += v[k];
        unsigned long long r = valid_off[blockIdx.x] + (unsigned long long)(rank_block_scan(cv, s) - cv);
#pragma unroll
        for (int k = 0; k < 16; ++k)
            if (v[k]) { v[k] = mark[r] ? 1 : 0; ++r; }
    }
    if (OUT == RankOut::Mask) {
        if (full) {
            uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
            for (int k = 0; k < 16; ++k) w[k >> 2] |= (uint32_t)v[k] << (8 * (k & 3));
            *reinterpret_cast<uint4*>(mask + t0) = make_uint4(w[0], w[1], w[2], w[3]);
        } else {
            for (int k = 0; k < 16 && t0 + k < n; ++k) mask[t0 + k] = v[k];
        }
        return;
    }
    int cs = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) cs += v[k];
    const int incl = rank_block_scan(cs, s);
    if (OUT == RankOut::Count) {
        if (threadIdx.x == 255) sel[blockIdx.x] = (unsigned long long)incl;
        return;
    }
    unsigned long long o = sel[blockIdx.x] + (unsigned long long)(incl - cs);
#pragma unroll
    for (int k = 0; k < 16; ++k)
        if (v[k]) idx[o++] = t0 + k;
}

// The steps both subsample entry points share: the ranks to the device (if they are on the host), the marks cleared, the ranks
// marked, the pixels of every tile counted and the counts scanned; then *total (pixels counted) and *bad (ranks outside
// [0, n_ranks)) read back.  Counted are the valid pixels (valid_off == nullptr) or the valid pixels whose rank is marked.  The
// temporaries live as long as the object (the queued work that reads them is waited for when it goes): `mark` and `off` are what
// the caller's selection launch reads after run().
struct RankSelect {
    XdBuffers buf;                        // `who`: the entry point, named in the error texts
    uint8_t* mark = nullptr;              // [n_ranks] 1 where a rank is listed
    unsigned long long* off = nullptr;    // [n_tiles] exclusive offsets of the counted pixels, [n_tiles] total, [n_tiles + 1] ranks out of range
    RankSelect(xdemhip_ctx* ctx, const char* who) : buf(ctx, who) {}

    int run(const int64_t* ranks, int64_t k, int memspace, int64_t n_ranks, const uint8_t* valid, int64_t n, const unsigned long long* valid_off,
            unsigned long long* total, unsigned long long* bad) {
        xdemhip_ctx* ctx = buf.ctx;
        const char* who = buf.who;
        const int64_t n_tiles = (n + RANK_TILE - 1) / RANK_TILE;
        mark = buf.alloc<uint8_t>((size_t)n_ranks);
        off = buf.alloc<unsigned long long>((size_t)n_tiles + 2);
        const int64_t* rk = buf.input(ranks, (size_t)k * 8, memspace);
        if (buf.rc) return buf.rc;
        if (hipMemsetAsync(mark, 0, (size_t)n_ranks, ctx->stream) != hipSuccess || hipMemsetAsync(off + n_tiles, 0, 16, ctx->stream) != hipSuccess)
            return xd_fail(ctx, XDEMHIP_EHIP, "hipMemsetAsync failed");
        hipLaunchKernelGGL(rank_mark_kernel, dim3(grid_for(ctx, k, 256, 8)), dim3(256), 0, ctx->stream, rk, k, n_ranks, mark, off + n_tiles + 1);
        hipLaunchKernelGGL((rank_select_kernel<RankOut::Count>), dim3((unsigned)n_tiles), dim3(256), 0, ctx->stream, valid, n, valid_off,
                           valid_off ? mark : (const uint8_t*)nullptr, off, (int64_t*)nullptr, (uint8_t*)nullptr);
        hipLaunchKernelGGL(rank_scan_kernel, dim3(1), dim3(1024), 0, ctx->stream, off, n_tiles, off + n_tiles);
        if (hipGetLastError() != hipSuccess) return xd_fail(ctx, XDEMHIP_EHIP, std::string(who) + ": kernel launch failed");
        unsigned long long chk[2] = {0, 0};
        { const int rc_ = xd_d2h(ctx, chk, off + n_tiles, 16); if (rc_) return rc_; }
        { const int rc_ = xd_sync(ctx); if (rc_) return rc_; }
        *total = chk[0];
        *bad = chk[1];
        return XDEMHIP_OK;
    }
};

}  // namespace
}  // namespace xd
