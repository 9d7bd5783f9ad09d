"""Measurement of xdem_amd.DEMCollection (csrc/demstack.hip); prints one JSON line and writes it to --out (default
profiles/demcollection_bench.json).  Nothing here asserts a time; a run without a GPU fails.

--t device-resident float32 DEMs of --n x --n: an fBm reference, the others the reference minus a trend, noise and 20 % voids; one
outline mask.  Two routes over the same inputs, ALTERNATING in one process (--repeats rounds after one warm-up round of each), wall
clock around work that ends in a device synchronise:

  * batched: ``DEMCollection.subtract_dems``, ``interpolate_ddems("regional_hypsometric")``, ``get_dh_series`` -- the stack's passes;
  * per pair: what upstream's loop does with this library's per-pair functions -- per DEM one ``ref - dem`` (torch), one
    ``volume.hypsometric_interpolation`` and one masked mean (``stats.get_stats``).

Reported per route: the times of every round per step and their medians; for the batched route also the bytes its passes need, from the
shapes (values per pixel: subtract 1 + 2 T, statistics 1 + T, grouping 3 T, scatter 2 T + inliers, fill 1 + 2 T, masks one byte per
plane and pass), and that figure over the median time -- a whole-route rate, not a kernel's share of peak.  The two routes' filled
planes are compared bit for bit before anything is timed.

    python tools/bench_demcollection.py [--n 20000] [--t 8] [--repeats 3] [--out ...]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]


def inputs(N: int, T: int, dev):
    import torch

    from xdem_amd import synth

    ref = synth.fbm_torch(N, N, dev)
    gen = torch.Generator(device=dev).manual_seed(5)
    dems = []
    for t in range(T):
        if t == 0:
            dems.append(ref)
            continue
        ddem = -0.01 * t * (ref - 1000.0) + 0.5 * (torch.rand((N, N), device=dev, generator=gen) - 0.5)
        ddem[torch.rand((N, N), device=dev, generator=gen) < 0.2] = float("nan")
        dems.append(ref - ddem)
        del ddem
    r = torch.arange(N, device=dev)
    inside = (r > N // 8) & (r < N - N // 8)
    return dems, inside[:, None] & inside[None, :]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=20000)
    ap.add_argument("--t", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "demcollection_bench.json"))
    a = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench_demcollection.py measures the GPU: no device found")
    from xdem_amd import DEMCollection, ddem as ddem_mod, stats, volume

    dev = torch.device("cuda:0")
    N, T = a.n, a.t
    planes, mask = inputs(N, T, dev)
    torch.cuda.synchronize()
    transform = (30.0, 0.0, 0.0, 0.0, -30.0, 0.0)
    stamps = [np.datetime64(f"{2000 + t}-01-01") for t in range(T)]
    dems = [ddem_mod.raster_of(p, transform) for p in planes]

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return r, time.perf_counter() - t0

    def batched():
        col = DEMCollection(dems, timestamps=stamps, outlines=mask, reference_dem=0)
        _, t_sub = timed(col.subtract_dems)
        filled, t_fill = timed(lambda: col.interpolate_ddems("regional_hypsometric"))
        dh, t_series = timed(lambda: col.get_dh_series())
        return {"subtract": t_sub, "fill": t_fill, "series": t_series, "total": t_sub + t_fill + t_series}, filled, dh

    def per_pair():
        steps = {"subtract": 0.0, "fill": 0.0, "series": 0.0}
        filled, means = [], []
        for t in range(1, T):
            d, dt = timed(lambda: planes[0] - planes[t])
            steps["subtract"] += dt
            f, dt = timed(lambda: volume.hypsometric_interpolation(d, planes[0], mask))
            steps["fill"] += dt
            m, dt = timed(lambda: stats.get_stats(f, "mean", inlier_mask=mask))
            steps["series"] += dt
            filled.append(f)
            means.append(m)
        steps["total"] = sum(steps.values())
        return steps, filled, means

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        _, f_b, dh = batched()       # warm-up of both routes, and the comparison
        _, f_p, means = per_pair()
        same = all(bool(torch.equal(torch.nan_to_num(f_b[t], nan=0.0), torch.nan_to_num(f_p[t - 1], nan=0.0))) and
                   bool(torch.equal(f_b[t].isnan(), f_p[t - 1].isnan())) for t in range(1, T))
        del f_b, f_p
        rounds = {"batched": [], "per_pair": []}
        for _ in range(a.repeats):
            for name, fn in (("batched", batched), ("per_pair", per_pair)):
                steps, f, _ = fn()
                del f
                rounds[name].append(steps)
    n = N * N
    inl = float(mask.sum().item()) * 0.8 * (T - 1)
    values = (1 + 2 * T) + (1 + T) + 3 * T + 2 * T + (1 + 2 * T)
    bytes_batched = 4.0 * (values * n + inl * 2) + 4.0 * T * n
    out = {"n": N, "t": T, "dtype": "float32", "device": torch.cuda.get_device_name(0), "repeats": a.repeats, "filled_planes_equal": same,
           "dh": [float(v) for v in dh["dh"].values], "per_pair_mean": [float(v) for v in means], "rounds": rounds,
           "median_s": {name: {k: statistics.median(r[k] for r in rs) for k in rs[0]} for name, rs in rounds.items()},
           "batched_bytes_from_shapes": bytes_batched}
    out["batched_route_rate_GBps"] = bytes_batched / out["median_s"]["batched"]["total"] / 1e9
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
