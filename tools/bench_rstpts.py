"""Measurement of the raster-point plan on the MI355X (no test asserts a time): one NuthKaab step, one ``shift_nmad`` and a whole
default fit over a device-resident float32 raster and a cloud, per order of the cloud (random, along-track) and per value of the test
switch "pts_tile_order"; the same step on the CPU through NumPy / SciPy on a crop, for scale.

The two values of the switch alternate inside one process, every shape is warmed first, a timed window holds ``--reps`` calls that each
end in the call's own fetch (a host clock around synchronous calls), and the spread over ``--rounds`` windows is recorded next to the
median.  Launches are counted by the profiler in a run of its own; here they are "not measured".

    python tools/bench_rstpts.py [--size 20000] [--points 10000000] [--reps 5] [--rounds 5]   [--out FILE]   ->  one line in profiles/rstpts_bench.json
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]


def make(size: int, n: int):
    """A device raster of ``synth.cloud_surface`` and a cloud of it displaced by ``CLOUD_SHIFT`` (hashed positions, no noise planes kept)."""
    import torch
    from xdem_amd import synth

    t6 = (10.0, 0.0, 500000.0, 0.0, -10.0, 4200000.0 + 10.0 * size)
    ax = torch.arange(size, dtype=torch.float64, device="cuda")
    px = (t6[2] + (ax + 0.5) * t6[0])[None, :]
    py = (t6[5] + (ax + 0.5) * t6[4])[:, None]
    raster = synth.cloud_surface(px, py, t6, (size, size)).to(torch.float32).contiguous()
    x = t6[2] + synth._hash01(n, 31) * size * t6[0]
    y = t6[5] + synth._hash01(n, 5031) * size * t6[4]
    sx, sy, sz = synth.CLOUD_SHIFT
    z = synth.cloud_surface(x + sx, y + sy, t6, (size, size)) + sz + 0.3 * (synth._hash01(n, 10031) * 2.0 - 1.0)
    return raster, t6, x, y, z


def timed(fn, reps: int, rounds: int):
    fn()
    fn()
    w = []
    for _ in range(rounds):
        t = time.perf_counter()
        for _ in range(reps):
            fn()
        w.append((time.perf_counter() - t) / reps * 1e3)
    return {"ms_median": float(np.median(w)), "ms_min": float(min(w)), "ms_max": float(max(w))}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=20000)
    ap.add_argument("--points", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--cpu-crop", type=int, default=2000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rstpts_bench.json"))
    a = ap.parse_args()
    import torch
    from xdem_amd import EPC, _lib, coreg, epc

    if not torch.cuda.is_available():
        raise SystemExit("bench_rstpts.py measures on the GPU: no device found")
    ctx = _lib.default_context()
    raster, t6, x, y, z = make(a.size, a.points)
    rec = {"size": a.size, "points": a.points, "reps": a.reps, "rounds": a.rounds, "launches": "not measured", "orders": {}}
    for order_name in ("random", "along_track"):
        if order_name == "along_track":   # sorted by a track coordinate: northing first, easting within a 100 m swath
            k = np.lexsort((x, np.floor(y / 100.0)))
            x, y, z = x[k], y[k], z[k]
        cols = [torch.from_numpy(v).cuda() for v in (x, y, z)]
        plans = {}
        for sw in (0, 1):
            ctx.set_option("pts_tile_order", sw)
            plans[sw] = epc.PtsPlan(raster, *cols, t6, True, None, with_nk_aux=True, ctx=ctx)
        ctx.set_option("pts_tile_order", 0)
        out = {"n_valid": plans[0].n_valid}
        for name, call in (("nk_step", lambda p: p.step(7.0, -3.5)), ("shift_nmad", lambda p: p.shift_nmad(7.0, -3.5))):
            res = {0: [], 1: []}
            for _ in range(2):   # the two values alternate
                for sw in (0, 1):
                    res[sw].append(timed(lambda: call(plans[sw]), a.reps, a.rounds))
            out[name] = {f"tile_order_{sw}": res[sw] for sw in (0, 1)}
        assert plans[0].shift_nmad(7.0, -3.5) == plans[1].shift_nmad(7.0, -3.5)   # (faster and different is not faster)
        for p in plans.values():
            p.close()
        fit = {}
        for sw in (0, 1):
            ctx.set_option("pts_tile_order", sw)
            fit[f"tile_order_{sw}"] = timed(lambda: coreg.NuthKaab().fit(EPC(*cols), raster, transform=t6, random_state=1), 1, 3)
        ctx.set_option("pts_tile_order", 0)
        out["default_fit"] = fit
        rec["orders"][order_name] = out
    # the same step on the CPU (NumPy / SciPy through the oracle's statement of it) on a crop
    import rstpts_oracle

    c = a.cpu_crop
    crop = raster[:c, :c].cpu().numpy()
    tc = (t6[0], 0.0, t6[2], 0.0, t6[4], t6[5])
    inside = (x < t6[2] + c * t6[0]) & (y > t6[5] + c * t6[4])
    t0 = time.perf_counter()
    o = rstpts_oracle.OraclePlan(crop, x[inside], y[inside], z[inside], tc, True, None, with_nk_aux=True)
    t1 = time.perf_counter()
    o.step(7.0, -3.5)
    rec["cpu_crop"] = {"size": c, "points": int(inside.sum()), "create_ms": (t1 - t0) * 1e3, "nk_step_ms": (time.perf_counter() - t1) * 1e3}
    line = json.dumps(rec)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
