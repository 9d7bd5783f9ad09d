"""Measurement of the raster filters (csrc/filter.hip); prints one JSON line per case and writes them, with a summary, to --out
(default profiles/filters_bench.json).

A device-resident float32 raster of N x N elevation-like pixels with 10 % voids, so that the calls time device work and not the
transfers.  Per case: the device time between the events the library records around its kernels (``xdemhip_last_kernel_ms``), median
of --reps launches after --warmup; the algorithmic bytes (the raster read once plus written once: the 2-plane roofline), bytes per
pixel, TB/s and the fraction of the HBM peak (8 TB/s) they make at that time; the route the call took.

  * Gaussian sigma = 1 and sigma = 5 (normalised: the raster has voids);
  * median 3, 5 and 11;
  * disk mean, radius 5;
  * distance filter, radius 5.

    python tools/bench_filters.py [--n 16384] [--reps 11] [--warmup 3] [--out profiles/filters_bench.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12   # bytes / s (spec)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=16384)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "filters_bench.json"))
    a = ap.parse_args()
    if a.reps < 10:
        ap.error("--reps must be at least 10")

    import torch

    from xdem_amd import _lib, filters

    ctx = _lib.default_context()
    N = a.n
    gen = torch.Generator(device="cuda").manual_seed(0)
    dem = 1500.0 + 100.0 * torch.randn((N, N), device="cuda", dtype=torch.float32, generator=gen)
    dem[torch.rand((N, N), device="cuda", generator=gen) < 0.10] = float("nan")
    torch.cuda.synchronize()

    cases = [("gaussian", {"sigma": 1.0, "normalise": True}), ("gaussian", {"sigma": 5.0, "normalise": True}), ("median", {"size": 3}), ("median", {"size": 5}),
             ("median", {"size": 11}), ("mean", {"radius": 5}), ("distance", {"radius": 5, "outlier_threshold": 120.0})]
    lines = []
    for method, kw in cases:
        ms = []
        for i in range(a.warmup + a.reps):
            out = filters.filter_array(dem, method, ctx=ctx, **kw)
            ctx.synchronize()
            if i >= a.warmup:
                ms.append(ctx.last_kernel_ms())
            del out
        med = float(np.median(ms))
        halo = filters.gaussian_radius(kw["sigma"]) if method == "gaussian" else kw.get("radius", kw.get("size", 0) // 2)
        nbytes = 2 * 4 * N * N
        line = {"method": method, **kw, "n": N, "halo": halo, "route": filters.filter_plan(N, N, method, halo, np.float32)["route"],
                "device_ms": round(med, 4), "device_ms_min_max": [round(float(min(ms)), 4), round(float(max(ms)), 4)],
                "algorithmic_bytes": nbytes, "bytes_per_pixel": 8, "TBps": round(nbytes / (med * 1e-3) / 1e12, 4),
                "roofline_fraction": round(nbytes / (med * 1e-3) / HBM_PEAK, 4)}
        print(json.dumps(line), flush=True)
        lines.append(line)
    summary = {"n": N, "dtype": "float32", "void_fraction": 0.10, "reps": a.reps, "warmup": a.warmup, "hbm_peak_Bps": HBM_PEAK, "cases": lines}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(summary, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
