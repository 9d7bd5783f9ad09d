"""Measurement of interp_points (csrc/spline.hip); prints one JSON line per case and writes them, with a summary, to --out (default
profiles/interp_bench.json).

A device-resident N x N float32 raster, once without gaps and once with 20 % of its pixels NaN at random; cubic and quintic; 10^6
and 10^7 random points inside the hull (device tensors), so that the calls time device work and not the transfers.

Per case: the device time of each stage of the prepare (``xdemhip_spline_stage_ms``: mask and fill -- with gaps that includes the
distance transform --, dilation, column passes, row passes) and of the gather (``xdemhip_last_kernel_ms``), medians of --reps runs
after --warmup with the smallest and the largest; for the streaming passes the algorithmic bytes per pixel, derived from the code
below, and the fraction of the HBM peak (8 TB/s) they make at the median.  For scale, ``scipy.ndimage.map_coordinates`` on the CPU
at --scipy-n (default 4096) with 10^6 points: what upstream pays on every call.

    python tools/interp_probe.py [--n 16384] [--reps 10] [--warmup 2] [--scipy-n 4096] [--out profiles/interp_bench.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12   # bytes / s (spec)
STAGES = ("mask_fill", "dilation", "column", "row")
ORDERS = {"cubic": 3, "quintic": 5}


def bytes_per_pixel(plan: dict, order: int, itemsize: int, dist: int, gaps: bool) -> dict:
    """Algorithmic bytes per pixel of the streaming passes of a prepare (interior bands and tiles).
    mask: the raster read, a flag written.  dilation: a 16 x 64 tile with a halo of 3 read, a byte written, per round of radius <= 3.
    column, per pole: the band and its two halos read (the raster's dtype for the first pole, float64 after), c+ written, read back
    and c- written.  row, per pole: the tile and its two halos read in float64, the tile written."""
    band, halo, tc = plan["band_rows"], plan["halo"], plan["tile_cols"]
    poles = 1 if order == 3 else 2
    col = sum((itemsize if k == 0 else 8) * (band + 2 * halo) / band + 24 for k in range(poles))
    row = poles * (8 * (tc + 2 * halo) / tc + 8)
    out = {"column": col, "row": row}
    if gaps:
        out["dilation"] = max(1, -(-dist // 3)) * ((16 + 6) * (64 + 6) / (16 * 64) + 1)
    else:
        out["mask_fill"] = itemsize + 1
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=16384)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--scipy-n", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "interp_bench.json"))
    a = ap.parse_args()

    import torch

    from xdem_amd import _lib, interp

    ctx = _lib.default_context()
    N = a.n
    transform = (2.0, 0.0, 100.0, 0.0, -2.0, 5000.0)
    g = torch.Generator(device="cuda").manual_seed(0)
    yy = torch.arange(N, device="cuda", dtype=torch.float32).reshape(-1, 1)
    xx = torch.arange(N, device="cuda", dtype=torch.float32).reshape(1, -1)
    base = 1000.0 + 40.0 * torch.sin(yy / 70.0) * torch.cos(xx / 50.0) + torch.randn((N, N), device="cuda", generator=g)
    del yy, xx
    points = {}
    for n_pts in (10**6, 10**7):
        px = transform[2] + (torch.rand(n_pts, device="cuda", dtype=torch.float64, generator=g) * (N - 1) + 0.5) * transform[0]
        py = transform[5] + (torch.rand(n_pts, device="cuda", dtype=torch.float64, generator=g) * (N - 1) + 0.5) * transform[4]
        points[n_pts] = (px, py)

    def med(v):
        v = np.asarray(v, dtype=np.float64)
        return {"ms": round(float(np.median(v)), 4), "ms_min_max": [round(float(v.min()), 4), round(float(v.max()), 4)]}

    lines = []
    for gaps in (False, True):
        raster = base.clone()
        if gaps:
            raster[torch.rand((N, N), device="cuda", generator=g) < 0.2] = float("nan")
        torch.cuda.synchronize()
        for method, order in ORDERS.items():
            plan_c = interp.plan_constants(N, N, order, 0)
            dist = interp.spread_distance(order)
            bpp = bytes_per_pixel(plan_c, order, 4, dist, gaps)
            stages, gathers, valid = [], {n: [] for n in points}, {}
            for i in range(a.warmup + a.reps):
                with interp.InterpPlan(raster, transform, order, ctx=ctx) as plan:
                    if i >= a.warmup:
                        stages.append(plan.stage_ms())
                    for n_pts, pts in points.items():
                        plan.at(pts)
                        valid[n_pts] = plan.n_valid
                        if i >= a.warmup:
                            gathers[n_pts].append(ctx.last_kernel_ms())
            stages = np.asarray(stages)
            line = {"case": f"{method}_{'gaps20' if gaps else 'nogaps'}", "shape": [N, N], "dtype": "float32", "order": order, "dist": dist,
                    "prepare_ms": med(stages.sum(axis=1)), "stages": {}, "gather": {}}
            for k, s in enumerate(STAGES):
                entry = med(stages[:, k])
                if s in bpp:
                    entry["bytes_per_pixel"] = round(bpp[s], 3)
                    entry["hbm_peak_fraction"] = round(bpp[s] * N * N / (max(entry["ms"], 1e-6) * 1e-3) / HBM_PEAK, 4)
                line["stages"][s] = entry
            for n_pts, ms in gathers.items():
                entry = med(ms)
                entry["points_per_s"] = round(n_pts / (entry["ms"] * 1e-3), 0)
                entry["n_valid"] = valid[n_pts]
                line["gather"][str(n_pts)] = entry
            print(json.dumps(line), flush=True)
            lines.append(line)
        del raster
        torch.cuda.empty_cache()

    from scipy import ndimage

    n = a.scipy_n
    host = base[:n, :n].cpu().numpy()
    rng = np.random.default_rng(0)
    r, c = rng.uniform(0, n - 1, 10**6), rng.uniform(0, n - 1, 10**6)
    scipy_s = {}
    for method, order in ORDERS.items():
        t0 = time.perf_counter()
        ndimage.map_coordinates(host, [r, c], order=order)
        scipy_s[method] = round(time.perf_counter() - t0, 3)
    summary = {"n": N, "reps": a.reps, "warmup": a.warmup, "hbm_peak_Bps": HBM_PEAK, "plan": interp.plan_constants(N, N, 5, 0),
               "scipy_n": n, "scipy_points": 10**6, "scipy_cpu_seconds": scipy_s, "cases": lines}
    print(json.dumps({k: v for k, v in summary.items() if k != "cases"}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(summary, f)
        f.write("\n")


if __name__ == "__main__":
    main()
