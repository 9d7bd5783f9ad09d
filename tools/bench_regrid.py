"""Measurement of the regridding pass (csrc/regrid.hip); prints one JSON line per case and writes them, with a summary, to --out
(default profiles/regrid_bench.json).

Device-resident float32 rasters, so that the calls time device work and not the transfers.  Per case: the device time between the
events the library records around its kernel (``xdemhip_last_kernel_ms``), median of --reps launches after --warmup; the algorithmic
bytes (source read once plus destination written once) and the fraction of the HBM peak (8 TB/s) they make at that time; the route.

  * N x N onto the same-size grid moved by (0.5, 0.25) pixels, with each of the four kernels;
  * N x N -> (N / 2.5)^2 with bilinear;
  * (N / 2.5)^2 -> N x N with cubic;
  * for the half-pixel bilinear case, in the same process on the same raster: ``xdemhip_shift_bilinear``, the translation resampler
    behind ``apply_translation``, which moves the same bytes -- and the ratio of the two times.

    python tools/bench_regrid.py [--n 20000] [--reps 11] [--warmup 3] [--out profiles/regrid_bench.json]
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12   # bytes / s (spec)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=20000)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "regrid_bench.json"))
    a = ap.parse_args()
    if a.reps < 10:
        ap.error("--reps must be at least 10")

    import torch

    from xdem_amd import _args, _lib, reproject

    ctx = _lib.default_context()
    N, M = a.n, int(a.n / 2.5)
    gen = torch.Generator(device="cuda").manual_seed(0)

    def raster(n):
        t = 1500.0 + 400.0 * torch.randn((n, n), device="cuda", dtype=torch.float32, generator=gen)
        t[torch.rand((n, n), device="cuda", generator=gen) < 0.01] = float("nan")
        return t

    big, small = raster(N), raster(M)
    out_big = torch.empty((N, N), device="cuda", dtype=torch.float32)
    out_small = torch.empty((M, M), device="cuda", dtype=torch.float32)
    torch.cuda.synchronize()

    def timed(launch):
        ms = []
        for i in range(a.warmup + a.reps):
            launch()
            if i >= a.warmup:
                ms.append(ctx.last_kernel_ms())
        return float(np.median(ms)), [float(min(ms)), float(max(ms))]

    def regrid_case(name, src, dst, map4, kernel):
        count = ctypes.c_int64()
        m = _args.c_doubles(map4)

        def launch():
            ctx.check(ctx._L.xdemhip_regrid(ctx.handle, _args.ptr(src), _lib.F32, src.shape[0], src.shape[1], _args.ptr(dst), _lib.F32,
                                            dst.shape[0], dst.shape[1], m, reproject.RESAMPLINGS[kernel], _lib.DEVICE, ctypes.byref(count)))

        med, spread = timed(launch)
        nbytes = 4 * (src.numel() + dst.numel())
        t = (1.0, 0.0, 0.0, 0.0, -1.0, 0.0)
        line = {"case": name, "kernel": kernel, "src": list(src.shape), "dst": list(dst.shape), "map4": list(map4),
                "route": reproject.route(t, (map4[0], 0.0, map4[1], 0.0, -map4[2], -map4[3]), kernel)[0],
                "device_ms": round(med, 4), "device_ms_min_max": [round(v, 4) for v in spread], "algorithmic_bytes": nbytes,
                "TBps": round(nbytes / (med * 1e-3) / 1e12, 3), "hbm_peak_fraction": round(nbytes / (med * 1e-3) / HBM_PEAK, 3),
                "valid_count": int(count.value)}
        print(json.dumps(line), flush=True)
        return line

    lines = [regrid_case("half_pixel", big, out_big, (1.0, 0.5, 1.0, 0.25), k) for k in ("nearest", "bilinear", "cubic", "cubic_spline")]
    lines.append(regrid_case("down2.5", big, out_small, (2.5, 0.0, 2.5, 0.0), "bilinear"))
    lines.append(regrid_case("up2.5", small, out_big, (M / N, 0.0, M / N, 0.0), "cubic"))

    def shift_launch():
        ctx.check(ctx._L.xdemhip_shift_bilinear(ctx.handle, _args.ptr(big), _lib.F32, N, N, 0.25, 0.5, 0.0, _args.ptr(out_big), _lib.DEVICE))
        ctx.synchronize()

    med, spread = timed(shift_launch)
    bil = next(v for v in lines if v["case"] == "half_pixel" and v["kernel"] == "bilinear")
    summary = {"n": N, "reps": a.reps, "warmup": a.warmup, "hbm_peak_Bps": HBM_PEAK,
               "shift_bilinear_ms": round(med, 4), "shift_bilinear_ms_min_max": [round(v, 4) for v in spread],
               "shift_bilinear_hbm_peak_fraction": round(bil["algorithmic_bytes"] / (med * 1e-3) / HBM_PEAK, 3),
               "regrid_bilinear_over_shift_bilinear": round(bil["device_ms"] / med, 3), "cases": lines}
    print(json.dumps({k: v for k, v in summary.items() if k != "cases"}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(summary, f)
        f.write("\n")


if __name__ == "__main__":
    main()
