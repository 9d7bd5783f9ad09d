"""Measurement of the bias corrections with variables (csrc/bincorr.hip); prints one JSON line and writes it to --out (default
profiles/bincorr_bench.json).  Nothing here asserts a time.

One synthetic N x N float32 pair, device-resident (an fBm surface; ``tba`` = the surface minus an along-track sine and an
elevation-proportional term, noise).  For ``DirectionalBias(angle=20, fit_or_bin="bin")`` and ``TerrainBias("elevation")``
(100 bins, linear apply):

  * ``fit`` and ``apply`` on the device tensors: wall clock of the second of two calls each, stream synchronised, and the
    apply's effective traffic at 8 B per pixel (4 B read, 4 B written);
  * the fused pass alone (``bincorr.corr_apply`` with the fitted grid), median of --reps calls;
  * the composed route of the entries that existed before the fused pass, for the same correction: the variable as a host plane
    (the float64 rotated coordinate / the elevation), ``GridInterpolant`` on it (host in, float64 host out), a host add and cast;
  * the CPU route of the reference's calls on a --cpu-n x --cpu-n crop (``scipy.stats.binned_statistic`` with ``np.nanmedian``
    for the fit, ``scipy.interpolate.RegularGridInterpolator`` and the add for the apply), scaled per pixel -- skipped with
    --skip-cpu.

    python tools/bench_bincorr.py [--n 20000] [--reps 5] [--cpu-n 3000] [--skip-cpu] [--out profiles/bincorr_bench.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=20000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cpu-n", type=int, default=3000)
    ap.add_argument("--skip-cpu", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bincorr_bench.json"))
    a = ap.parse_args()

    import torch

    from xdem_amd import _lib, bincorr, coreg, synth
    from xdem_amd.spatialstats import GridInterpolant, interp_nd_binning

    N, res = a.n, (10.0, 10.0)
    dev = torch.device("cuda:0")
    ref = synth.fbm_torch(N, N, dev)
    cols = torch.arange(N, device=dev, dtype=torch.float32)[None, :] * res[0]
    rows = (N - 1 - torch.arange(N, device=dev, dtype=torch.float32))[:, None] * res[1]
    along = cols * float(np.cos(np.deg2rad(20.0))) + rows * float(np.sin(np.deg2rad(20.0)))
    tba = ref - 3.0 * torch.sin(along * (2 * np.pi / (N * res[0] / 3.0))) - 0.01 * (ref - 1000.0)
    tba += 0.2 * (torch.rand((N, N), device=dev, generator=torch.Generator(device=dev).manual_seed(1)) - 0.5)
    del cols, rows, along
    torch.cuda.synchronize()
    out = {"n": N, "dtype": "float32", "bins": 100, "device": torch.cuda.get_device_name(0)}

    def timed(fn, reps=2):
        ts = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = fn()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        return r, ts

    steps = {"directional": lambda: coreg.DirectionalBias(angle=20.0, fit_or_bin="bin"), "terrain_elevation": lambda: coreg.TerrainBias("elevation")}
    for tag, make in steps.items():
        step = make()
        _, ts = timed(lambda: step.fit(ref, tba, resolution=res))
        rec = {"fit_s": ts[-1], "fit_first_s": ts[0]}
        _, ts = timed(lambda: step.apply(tba, resolution=res))
        rec.update(apply_s=ts[-1], apply_first_s=ts[0])
        name = step.meta["inputs"]["fitorbin"]["bias_var_names"][0]
        interp = interp_nd_binning(step.meta["outputs"]["fitorbin"]["bin_dataframe"], [name], statistic=np.nanmedian, min_count=0)
        var = bincorr._Var("rotated", rot=bincorr._rotation((N, N), res, 20.0)) if tag == "directional" else bincorr._Var("raster")
        fused, ts = timed(lambda: bincorr.corr_apply(tba, _lib.CORR_GRID, [var], [len(interp.grid[0])], a=interp.grid[0], table=interp.values)[0], a.reps)
        rec["fused_pass_s"] = float(np.median(ts))
        rec["fused_pass_GBps_at_8B_per_pixel"] = 8.0 * N * N / rec["fused_pass_s"] / 1e9
        # the composed route: host plane -> GridInterpolant -> host add (what the parent commit's entries allow)
        h_tba = tba.cpu().numpy()
        t0 = time.perf_counter()
        plane = bincorr.rotated_x((N, N), res, 20.0) if tag == "directional" else h_tba
        t1 = time.perf_counter()
        corr = GridInterpolant(list(interp.grid), interp.values)((plane,))
        t2 = time.perf_counter()
        composed = (h_tba + corr).astype(np.float32)
        t3 = time.perf_counter()
        rec["composed"] = {"plane_s": t1 - t0, "interpolant_s": t2 - t1, "add_cast_s": t3 - t2, "total_s": t3 - t0,
                           "equal_to_fused": bool(np.array_equal(composed, fused.cpu().numpy(), equal_nan=True))}
        del plane, corr, composed, fused
        if not a.skip_cpu:
            import scipy.stats
            from scipy.interpolate import RegularGridInterpolator

            n = min(a.cpu_n, N)
            c_ref, c_tba = ref[:n, :n].cpu().numpy(), h_tba[:n, :n]
            t0 = time.perf_counter()
            x = bincorr.rotated_x((n, n), res, 20.0) if tag == "directional" else c_ref
            dh = c_ref - c_tba
            scipy.stats.binned_statistic(x.ravel(), dh.ravel(), statistic=np.nanmedian, bins=100)
            t1 = time.perf_counter()
            xa = bincorr.rotated_x((n, n), res, 20.0) if tag == "directional" else c_tba
            f = RegularGridInterpolator(interp.grid, interp.values, method="linear", bounds_error=False, fill_value=None)
            (c_tba + f((xa.ravel(),)).reshape(n, n)).astype(np.float32)
            t2 = time.perf_counter()
            scale = (N / n) ** 2
            rec["cpu"] = {"n": n, "fit_s": t1 - t0, "apply_s": t2 - t1, "fit_s_scaled_to_n": (t1 - t0) * scale, "apply_s_scaled_to_n": (t2 - t1) * scale}
        del h_tba
        out[tag] = rec
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
