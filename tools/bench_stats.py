"""Measurement of the raster statistics (csrc/rasterstats.hip); prints one JSON line and writes it to --out (default
profiles/stats_bench.json).

One N x N float32 raster (default 16384^2, Gaussian elevations, 20 % NaN gaps), resident on the device so that the calls time device
work and not the upload:

  * ``stats.get_stats`` (all keys) under "selection" 0 (the default route: bracketed at this size) and 1 (plain digit passes): wall
    clock of a call, which returns synchronised -- median of --reps calls after --warmup; the route each round took, the full reads of the
    raster the call made and the bandwidth they imply; whether the two routes returned the same bits;
  * ``xdemhip_nmad`` on the same device array: the closest call before this one (median and NMAD only), same clock;
  * on a 4096^2 crop, on this host: the NumPy expressions the statistics restate (np.median, three np.percentile, the two medians of the
    NMAD, the sums), skipped with --skip-cpu.

    python tools/bench_stats.py [--n 16384] [--reps 7] [--warmup 2] [--skip-cpu] [--out profiles/stats_bench.json]
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import struct
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=16384)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--skip-cpu", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stats_bench.json"))
    a = ap.parse_args()

    import torch

    from xdem_amd import _lib, stats

    ctx = _lib.default_context()
    N = a.n
    gen = torch.Generator(device="cuda").manual_seed(0)
    dem = 1500.0 + 400.0 * torch.randn((N, N), device="cuda", dtype=torch.float32, generator=gen)
    dem[torch.rand((N, N), device="cuda", generator=gen) < 0.2] = float("nan")
    torch.cuda.synchronize()
    out = {"n": N, "dtype": "float32", "gaps": 0.2, "reps": a.reps, "warmup": a.warmup}
    nbytes = N * N * 4

    blocks = {}
    for mode in (0, 1):
        ctx.set_option("selection", mode)
        inp = stats._Input(dem, None, None)
        ms = []
        for i in range(a.warmup + a.reps):
            t0 = time.perf_counter()
            s = stats.get_stats(dem, ctx=ctx)
            ms.append((time.perf_counter() - t0) * 1e3)
        blk = stats._device_stats(inp, (0.9, 0.95, 0.05), ctx)
        blocks[mode] = blk
        t = float(np.median(ms[a.warmup:]))
        out[f"get_stats_selection{mode}_ms"] = round(t, 3)
        out[f"get_stats_selection{mode}_ms_min_max"] = [round(min(ms[a.warmup:]), 3), round(max(ms[a.warmup:]), 3)]
        out[f"selection{mode}_route"] = list(blk["route"])
        out[f"selection{mode}_raster_reads"] = round(blk["reads"], 3)
        out[f"selection{mode}_implied_TBps"] = round(blk["reads"] * nbytes / (t * 1e-3) / 1e12, 3)
        if mode == 0:
            out["median"], out["nmad"], out["valid"] = s["Median"], s["NMAD"], s["Valid count"]
    ctx.set_option("selection", 0)
    flat = lambda b: [struct.pack("d", float(x)) for k, x in sorted(b.items()) if k not in ("route", "reads", "q_lo", "q_hi")] + \
        [struct.pack("d", x) for x in b["q_lo"] + b["q_hi"]]  # noqa: E731
    out["routes_bit_identical"] = flat(blocks[0]) == flat(blocks[1])

    med, nm, cnt = ctypes.c_double(), ctypes.c_double(), ctypes.c_int64()
    ms = []
    with ctx.call_lock:
        ctx.set_stream(torch.cuda.current_stream(dem.device).cuda_stream)
        for i in range(a.warmup + a.reps):
            t0 = time.perf_counter()
            ctx.check(ctx._L.xdemhip_nmad(ctx.handle, dem.data_ptr(), _lib.F32, N * N, 1.4826, float("inf"), _lib.DEVICE, ctypes.byref(med),
                                          ctypes.byref(nm), ctypes.byref(cnt)))
            ms.append((time.perf_counter() - t0) * 1e3)
        ctx.set_stream(None)
    out["nmad_device_ms"] = round(float(np.median(ms[a.warmup:])), 3)
    out["nmad_agrees"] = bool(med.value == out["median"] and nm.value == out["nmad"] and cnt.value == out["valid"])

    if not a.skip_cpu:
        c = min(N, 4096)
        v = dem[:c, :c].cpu().numpy()
        t0 = time.perf_counter()
        v = v[np.isfinite(v)]
        v64 = v.astype(np.float64)
        m = np.median(v)
        host = [float(m), float(np.percentile(v64, 90)), float(np.percentile(v64, 95) - np.percentile(v64, 5)),
                float(1.4826 * np.median(np.abs(v - m))), float(v64.sum()), float((v64 * v64).sum()), float(v64.std()), float(v.min()), float(v.max())]
        out["cpu_numpy_crop"] = c
        out["cpu_numpy_crop_s"] = round(time.perf_counter() - t0, 4)
        ctx.set_option("selection", 1)
        t0 = time.perf_counter()
        s = stats.get_stats(dem[:c, :c].contiguous(), ctx=ctx)
        out["get_stats_crop_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
        ctx.set_option("selection", 0)
        out["crop_order_statistics_agree"] = bool([s["Median"], s["90th percentile"], s["LE90"], s["NMAD"]] == host[:4] and [s["Min"], s["Max"]] == host[7:])
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
