"""Measurement of connected-component labelling and outline tracing (csrc/ccl.hip); prints one JSON line per case and writes them, with
a summary, to --out (default profiles/polygonize_bench.json).

Device-resident planes, so that the calls time device work and not the transfers.  Three uint8 masks on an N x N plane, connectivity 4:

  * ``sparse_blobs``      -- many small blobs, a few per cent of the plane;
  * ``large_with_holes``  -- one disc of radius 0.45 N with the blobs cut out of it as holes;
  * ``random_0.59``       -- independent pixels at density 0.59, next to the percolation threshold of the square lattice: the
                             components span many tiles and the union chains of the border pass are at their longest.

Per case: K, the corner vertices V and the rings R; wall time of the label call, the table call and the outline route (its counting call and its full call; medians of
--reps after --warmup, with the smallest and largest), and per stage (``xdemhip_ccl_stage_ms``) the median device time, the algorithmic
bytes per pixel it moves and the fraction of the HBM peak (8 TB/s) that makes.  The tracing stages work on the V corners, not on the
pixels: their bytes are per corner times V / N^2.  The span of the ``corners`` stage also holds the fetch of the corner count and the
allocation of the corner buffers (not pure kernel time); the ``rings`` stage includes a fetch of the ring table and its ordering on the
host.  For the record, ``scipy.ndimage.label`` on the CPU on the same three masks at --scipy-n (default 4000).

    python tools/bench_polygonize.py [--n 20000] [--reps 5] [--warmup 1] [--scipy-n 4000] [--out profiles/polygonize_bench.json]
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
CASES = ("sparse_blobs", "large_with_holes", "random_0.59")
TRANSFORM = (30.0, 0.0, 412345.0, 0.0, -30.0, 5267890.0)


def blobs(n: int, xp, level: float):
    """A mask of many blobs on an n x n plane (``xp``: numpy or torch, the same expression)."""
    y = xp.arange(n).reshape(-1, 1)
    x = xp.arange(n).reshape(1, -1)
    return (xp.sin(y * 0.043) * xp.sin(x * 0.031) + 0.5 * xp.sin((x + y) * 0.0071)) > level


def disc(n: int, xp):
    y = xp.arange(n).reshape(-1, 1) - n // 2
    x = xp.arange(n).reshape(1, -1) - n // 2
    return (y * y + x * x) <= (0.45 * n) ** 2


def stage_bytes(plan: dict, n_pixels: int, V: int, rounds: int) -> dict:
    """Algorithmic bytes per PIXEL of every stage (uint8 classes, int32 parents and labels, int64 edge numbers, int32 corner links)."""
    per_corner = V / n_pixels
    tr, tc = plan["tile_rows"], plan["tile_cols"]
    return {"tile": 1 + 4, "border": (1.0 / tr + 1.0 / tc) * (2 * 1 + 2 * 4), "flatten": 4 + 4, "number": 4 + 4 + (4 + 4 + 4), "table": 1 + 4,
            "corners": 4 + 4 + 8 * per_corner, "walk": (8 + 4 + 8) * per_corner, "leader": rounds * 24 * per_corner, "rank": (rounds + 1) * 24 * per_corner,
            "rings": (4 + 4 + 40) * per_corner, "gather": (28 + 16) * per_corner}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=20000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--scipy-n", type=int, default=4000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "polygonize_bench.json"))
    a = ap.parse_args()
    if a.reps < 3:
        ap.error("--reps must be at least 3")

    import torch

    from xdem_amd import _lib, polygonize

    ctx = _lib.default_context()
    N = a.n
    plan = polygonize.label_plan(N, N, 0)
    rounds = int(np.ceil(np.log2(4 * N * N)))

    class _TorchXp:   # (the calls the generators make, on the device)
        sin = staticmethod(torch.sin)

        @staticmethod
        def arange(n):
            return torch.arange(n, device="cuda", dtype=torch.float32)

    def mask(name, n, device):
        xp = _TorchXp if device else np
        if name == "sparse_blobs":
            m = blobs(n, xp, 1.2)
        elif name == "large_with_holes":
            m = disc(n, xp) & ~blobs(n, xp, 1.2)
        elif device:
            g = torch.Generator(device="cuda")
            g.manual_seed(59)
            m = torch.rand((n, n), device="cuda", generator=g) < 0.59
        else:
            m = np.random.default_rng(59).random((n, n), dtype=np.float32) < 0.59
        return m.to(torch.uint8).contiguous() if device else np.ascontiguousarray(m)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return out, (time.perf_counter() - t0) * 1e3

    def spread(v):
        return [round(float(np.median(v)), 3), round(float(min(v)), 3), round(float(max(v)), 3)]

    lines = []
    for name in CASES:
        m = mask(name, N, True)
        torch.cuda.synchronize()
        wall = {"label": [], "table": [], "outlines": []}
        stages = []
        for i in range(a.warmup + a.reps):
            (labels, K), t_label = timed(lambda: polygonize._ENGINE.label(m, 4, ctx=ctx))
            _, t_table = timed(lambda: polygonize._ENGINE.table(m, labels, K, ctx=ctx))
            rings, t_out = timed(lambda: polygonize._ENGINE.outlines(labels, K, TRANSFORM, ctx=ctx))
            V, R = int(rings.xy.shape[1]), int(rings.poly_of_ring.shape[0])
            if i >= a.warmup:
                for k, v in zip(("label", "table", "outlines"), (t_label, t_table, t_out)):
                    wall[k].append(v)
                stages.append(polygonize.DeviceEngine.stage_ms(ctx)[0])
            del labels, rings
        bpp = stage_bytes(plan, N * N, V, rounds)
        med = {s: float(np.median([st[s] for st in stages])) for s in polygonize.STAGES}
        line = {"case": name, "shape": [N, N], "foreground": round(float(m.float().mean()), 4), "K": K, "V": V, "R": R, "jumping_rounds": rounds,
                "wall_ms_median_min_max": {k: spread(v) for k, v in wall.items()},
                "stages": {s: {"ms": round(med[s], 4), "bytes_per_pixel": round(bpp[s], 4),
                               "hbm_peak_fraction": round(bpp[s] * N * N / (max(med[s], 1e-6) * 1e-3) / HBM_PEAK, 4)} for s in polygonize.STAGES},
                "dominant_stage": max(med, key=med.get)}
        print(json.dumps(line), flush=True)
        lines.append(line)
        del m
        torch.cuda.empty_cache()

    from scipy import ndimage

    scipy_s = {}
    for name in CASES:
        m = mask(name, a.scipy_n, False)
        t0 = time.perf_counter()
        _, k = ndimage.label(m)
        scipy_s[name] = {"seconds": round(time.perf_counter() - t0, 3), "K": int(k)}
    summary = {"n": N, "reps": a.reps, "warmup": a.warmup, "hbm_peak_Bps": HBM_PEAK, "plan": plan, "scipy_n": a.scipy_n,
               "scipy_label_cpu": scipy_s, "cases": lines}
    print(json.dumps({k: v for k, v in summary.items() if k != "cases"}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(summary, f)
        f.write("\n")


if __name__ == "__main__":
    main()
