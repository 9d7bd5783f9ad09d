// pts_plan.h -- the raster-point plan: one raster, one elevation point cloud and which of the two is the reference
// (ptsplan.hip creates, steps and destroys it).
#pragma once
#include <vector>

#include "common.h"
#include "select.h"
#include "select_run.h"
#include "fixed_sums.h"

struct xdemhip_pts_plan {
    xdemhip_ctx* ctx = nullptr;
    int dtype = XDEMHIP_F32;
    int64_t H = 0, W = 0;
    double t6[6] = {1, 0, 0, 0, -1, 0};       // north-up geotransform (a, 0, c, 0, e, f)
    bool pts_is_ref = false;                  // dh = z - raster(x + sx, y + sy); otherwise raster(x - sx, y - sy) - z
    bool with_aux = false;
    int nan_rule = 0;                         // the tap rule the plan was created under (option "nk_nan_rule")
    XdOwned mem;                              // every device buffer of the plan but the caller's own device arrays
    void* raster = nullptr;                   // the raster and the cloud: the caller's device arrays, or owned copies of its host arrays
    double* x = nullptr;                      // the cloud's columns, n_pts values each, cloud order
    double* y = nullptr;
    void* z = nullptr;                        // raster dtype
    int64_t n_pts = 0;
    uint8_t* pvalid = nullptr;                // n_pts bytes: finite (x, y, z) and the tap rule accepts the validity plane at the point
    unsigned long long* tile_off = nullptr;   // exclusive offsets of the valid points per tile of RANK_TILE points (n_tiles + 1 words)
    int64_t n_tiles = 0;
    int64_t n_valid = 0;
    void* a_st = nullptr;                     // slope tangent / aspect interpolated at every point at zero shift (with_aux), raster dtype
    void* a_asp = nullptr;
    // the selection: all valid points, or the drawn ones; columns of m values in cloud order
    int64_t m = 0;
    int64_t* idx = nullptr;                   // cloud indexes
    double* sx = nullptr;
    double* sy = nullptr;
    void* sz = nullptr;
    void* sst = nullptr;
    void* sasp = nullptr;
    int64_t* order = nullptr;                 // test switch "pts_tile_order": the selection ordered by raster tile of the unshifted position
    // buffers of the evaluations, made at the first one and kept
    void* dh = nullptr;
    void* yv = nullptr;
    uint16_t* bins = nullptr;
    int64_t step_n = -1;
    int64_t y_n = -1;                         // values of yv the last Nuth-Kaab step filled (-1: none yet)
    unsigned char* scratch = nullptr;         // bin edges | min / max aspect | selection scratch | the blocks an evaluation hands back
    xd::SelWorkspace ws;
    int64_t ws_n = -1;
    xd::FixedSums sums;
    void* d_custom = nullptr;                 // explicit bin edges in the raster dtype (n_custom + 1 values)
    int n_custom = 0, custom_decimal = 0;
};
