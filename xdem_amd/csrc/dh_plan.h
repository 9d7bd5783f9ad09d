// dh_plan.h -- the dh plan (elevation difference of two rasters on one grid) as the translation units that work on it see it:
// biascorr.hip creates and destroys it, rigid.hip adds the LZD passes, icp.hip the normal planes of ICP.  The fixed-order sums of
// the moments and of the LZD normal equations go through the plan's one partials buffer (fixed_sums.h); ICP's through its own.
#pragma once
#include "common.h"
#include "select.h"
#include "select_run.h"
#include "fixed_sums.h"

struct xdemhip_dh_plan {
    xdemhip_ctx* ctx = nullptr;
    int dtype = XDEMHIP_F32;
    int64_t H = 0, W = 0;
    XdOwned mem;                              // every device buffer of the plan but the caller's own device arrays
    void* ref = nullptr;                      // the caller's device arrays, or owned copies of its host arrays
    void* tba = nullptr;
    uint8_t* inlier = nullptr;
    uint8_t* valid = nullptr;                 // n bytes: inlier & finite(ref) & finite(tba)
    unsigned long long* tile_off = nullptr;   // exclusive offsets of the valid pixels per tile (n_tiles + 1 words)
    int64_t n_tiles = 0;
    int64_t n_valid = 0;
    int64_t* idx = nullptr;                   // selected pixels (flat indexes, raster order): the drawn ones, or all valid ones on demand
    int64_t n_idx = 0;
    bool drawn = false;                       // xdemhip_dh_subsample was called: the drawn pixels are the selection
    // shifted-dh evaluations (xdemhip_dh_shift_nmad / _values): made at the first evaluation, kept until the plan goes
    void* stage = nullptr;                    // dh of one evaluation: H * W values (dense route) or n_idx (list route)
    int64_t stage_n = 0;
    unsigned char* sel_scratch = nullptr;     // selection states, successor keys, histograms (scratch_size(1)), then the DhEvalOut block
    xd::SelWorkspace sel_ws;                  // sample / candidate buffers of the bracketed selection (stage_n >= SEL_BRACKET_MIN_N)
    int64_t sel_ws_n = 0;
    xd::FixedSums sums;                       // per-workgroup partials and totals of the moments (biascorr.hip) and of the LZD normal equations
    // LZD (rigid.hip): gradient planes of ref in the raster dtype, made at the first LZD call, kept until the plan goes
    void* gradx = nullptr;                    // gradient_x / res_x
    void* grady = nullptr;                    // -gradient_y / res_y
    double grad_res_x = 0.0, grad_res_y = 0.0;  // the resolutions the planes were formed with
    // ICP (icp.hip): the normal planes nx, ny, nz of ref in the raster dtype; making them narrows `valid` by their finiteness
    void* icp_n[3] = {nullptr, nullptr, nullptr};
    double icp_res_x = 0.0, icp_res_y = 0.0;
};

namespace xd {
int dh_ensure_mask(xdemhip_dh_plan* P);        // the valid mask and the scanned tile offsets, built on first need
int dh_ensure_valid_idx(xdemhip_dh_plan* P);   // P->idx = the drawn pixels, or the list of all valid pixels (raster order)
}  // namespace xd
