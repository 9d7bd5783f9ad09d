"""Measurement of the distance transform (csrc/edt.hip); prints one JSON line per case and writes them, with a summary, to --out
(default profiles/proximity_bench.json).

Device-resident planes, so that the calls time device work and not the transfers.  Three target sets on an N x N plane, float32
distances, sampling (30, 20):

  * ``dense_outlines`` -- the inner boundary of a mask of many blobs (a target within tens of pixels of every pixel);
  * ``one_polygon``    -- the pixels of one disc of radius N / 8 in the centre (the far corners are 0.58 N away);
  * ``single_target``  -- one target pixel in a corner: the worst case of the block search.

Per case: the device time of the whole call (``xdemhip_last_kernel_ms``) and of each of its four passes (``xdemhip_edt_stage_ms``),
medians of --reps calls after --warmup, with the smallest and the largest; the algorithmic bytes per pixel that each pass moves and the
fraction of the HBM peak (8 TB/s) they make at the pass's median time.  For the record, ``scipy.ndimage.distance_transform_edt`` on
the CPU on the same three target sets at --scipy-n (default 4000).

    python tools/bench_proximity.py [--n 20000] [--reps 11] [--warmup 2] [--scipy-n 4000] [--out profiles/proximity_bench.json]
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
SAMPLING = (30.0, 20.0)
PASSES = ("down", "carry", "up", "row")


def blobs(n: int, xp):
    """A mask of many blobs on an n x n plane (``xp``: numpy or torch, the same expression)."""
    y = xp.arange(n).reshape(-1, 1)
    x = xp.arange(n).reshape(1, -1)
    return (xp.sin(y * 0.043) * xp.sin(x * 0.031) + 0.5 * xp.sin((x + y) * 0.0071)) > 0.35


def disc(n: int, xp):
    y = xp.arange(n).reshape(-1, 1) - n // 2
    x = xp.arange(n).reshape(1, -1) - n // 2
    return (y * y + x * x) <= (n // 8) ** 2


def bytes_per_pixel(plan: dict, H: int) -> dict:
    """Algorithmic bytes per pixel of each pass: targets are bytes, offsets ``offset_bytes``, distances float32."""
    ob, band, tile, halo, block = (plan[k] for k in ("offset_bytes", "band_rows", "tile_cols", "halo", "block_cols"))
    nbands = -(-H // band)
    return {"down": 1 + ob + 8.0 / band, "carry": 16.0 * nbands / H, "up": 2 * ob + 8.0 / band + 4.0 / block,
            "row": ob * (tile + 2 * halo) / tile + 4}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=20000)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--scipy-n", type=int, default=4000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "proximity_bench.json"))
    a = ap.parse_args()
    if a.reps < 10:
        ap.error("--reps must be at least 10")

    import torch

    from xdem_amd import _lib, proximity

    ctx = _lib.default_context()
    N = a.n
    plan = proximity.edt_plan(N, N, 0)
    bpp = bytes_per_pixel(plan, N)

    def targets(name, n, xp, device):
        if name == "dense_outlines":
            m = blobs(n, xp)
            if device:
                return proximity.inner_boundary(m.contiguous(), ctx=ctx)
            b = np.zeros_like(m)
            b[1:] |= m[1:] & ~m[:-1]
            b[:-1] |= m[:-1] & ~m[1:]
            b[:, 1:] |= m[:, 1:] & ~m[:, :-1]
            b[:, :-1] |= m[:, :-1] & ~m[:, 1:]
            return b
        if name == "one_polygon":
            m = disc(n, xp)
            return m.to(torch.uint8).contiguous() if device else m
        m = xp.zeros((n, n), dtype=xp.uint8)
        m[0, 0] = 1
        return m

    class _TorchXp:   # (the three calls the generators make, on the device)
        uint8 = torch.uint8
        sin = staticmethod(torch.sin)

        @staticmethod
        def arange(n):
            return torch.arange(n, device="cuda", dtype=torch.float32)

        @staticmethod
        def zeros(shape, dtype):
            return torch.zeros(shape, device="cuda", dtype=dtype)

    lines = []
    for name in ("dense_outlines", "one_polygon", "single_target"):
        t = targets(name, N, _TorchXp, True)
        torch.cuda.synchronize()
        total, stages, n_targets = [], [], 0
        for i in range(a.warmup + a.reps):
            _, _, n_targets = proximity.edt(t, SAMPLING, np.float32, ctx=ctx)
            if i >= a.warmup:
                total.append(ctx.last_kernel_ms())
                stages.append(proximity.DeviceEngine.stage_ms(ctx))
        stages = np.asarray(stages)
        med = np.median(stages, axis=0)
        line = {"case": name, "shape": [N, N], "sampling": list(SAMPLING), "n_targets": n_targets,
                "device_ms": round(float(np.median(total)), 4), "device_ms_min_max": [round(float(min(total)), 4), round(float(max(total)), 4)],
                "passes": {p: {"ms": round(float(med[k]), 4), "ms_min_max": [round(float(stages[:, k].min()), 4), round(float(stages[:, k].max()), 4)],
                               "bytes_per_pixel": round(bpp[p], 4),
                               "hbm_peak_fraction": round(bpp[p] * N * N / (max(float(med[k]), 1e-6) * 1e-3) / HBM_PEAK, 4)}
                           for k, p in enumerate(PASSES)},
                "bytes_per_pixel": round(sum(bpp.values()), 3),
                "hbm_peak_fraction": round(sum(bpp.values()) * N * N / (float(np.median(total)) * 1e-3) / HBM_PEAK, 4)}
        print(json.dumps(line), flush=True)
        lines.append(line)
        del t
        torch.cuda.empty_cache()

    from scipy import ndimage

    scipy_s = {}
    for name in ("dense_outlines", "one_polygon", "single_target"):
        t = np.asarray(targets(name, a.scipy_n, np, False)) != 0
        t0 = time.perf_counter()
        ndimage.distance_transform_edt(~t, sampling=SAMPLING)
        scipy_s[name] = round(time.perf_counter() - t0, 3)
    summary = {"n": N, "reps": a.reps, "warmup": a.warmup, "hbm_peak_Bps": HBM_PEAK, "plan": plan, "scipy_n": a.scipy_n,
               "scipy_cpu_seconds": scipy_s, "cases": lines}
    print(json.dumps({k: v for k, v in summary.items() if k != "cases"}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(summary, f)
        f.write("\n")


if __name__ == "__main__":
    main()
