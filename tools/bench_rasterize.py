"""Measurement of polygon rasterisation (csrc/vector.hip behind xdem_amd.vector.DeviceRasterizer); prints one JSON line and writes it
to --out (default profiles/vector_bench.json).  Nothing here asserts a time; a run without a GPU fails.

Three tables on an --n x --n grid at 10 m, built as vertex tables in NumPy (a million polygons through ``Vector``'s parser would time
the parser), burnt into device planes:

  * rgi_like     --polygons (default 10^4) random 32-vertex stars of 40 to 300 pixels radius, hashed centres: an inventory of outlines
  * giant        one 1000-vertex star over most of the grid: 2 to 6 crossings per row, every span thousands of columns wide
  * pixel_sized  --small (default 10^6) quadrilaterals of one to three pixels on a lattice

Each case runs in a child process of its own under a time limit (--limit seconds), --repeats times after one warm-up, mask and label
route: wall clock around a call that returns synchronised, the device time between the call's first and last kernel (the library's
events; it contains the call's one mid-way fetch of two totals), the kernels launched, and from one more round under the test switch
"vec_stage_times" the device time of each of the five stages ("segments" contains that fetch).

CPU stand-in: the only comparator at hand offline is matplotlib's point-in-polygon test, run for the first --cpu-polygons stars of
rgi_like over the pixel centres of their bounding boxes and scaled linearly to the table.  Upstream's path is GDAL's scanline fill
through rasterio, which is not installed and could not be run.

    python tools/bench_rasterize.py [--n 20000] [--polygons 10000] [--small 1000000] [--repeats 3] [--limit 300] [--out ...]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

CASES = ("rgi_like", "giant", "pixel_sized")


def transform(n: int) -> tuple:
    return (10.0, 0.0, 500000.0, 0.0, -10.0, 4200000.0 + 10.0 * n)


def stars(n: int, count: int, vertices: int, r_lo: float, r_hi: float, salt: int) -> tuple:
    """`count` stars of `vertices` vertices as a vertex table (xy, ring_off, poly_of_ring, P)."""
    from xdem_amd.synth import _hash01

    t6 = transform(n)
    cu, cv = _hash01(count, salt) * n, _hash01(count, salt + 1) * n
    rad = r_lo + (r_hi - r_lo) * _hash01(count, salt + 2) ** 2
    k = np.arange(vertices)
    jitter = _hash01(count * vertices, salt + 3).reshape(count, vertices)
    ang = 2 * np.pi * (k[None, :] + 0.3 * jitter) / vertices
    r = rad[:, None] * np.where(k % 2 == 0, 1.0, 0.55)[None, :] * (0.85 + 0.3 * _hash01(count * vertices, salt + 4).reshape(count, vertices))
    u, v = cu[:, None] + r * np.cos(ang), cv[:, None] + r * np.sin(ang)
    xy = np.ascontiguousarray(np.stack([t6[2] + u.ravel() * t6[0], t6[5] + v.ravel() * t6[4]]))
    return xy, np.arange(count + 1, dtype=np.int64) * vertices, np.arange(count, dtype=np.int32), count


def lattice(n: int, count: int) -> tuple:
    from xdem_amd.synth import _hash01

    t6 = transform(n)
    per_row = int(np.ceil(np.sqrt(count)))
    k = np.arange(count)
    cu, cv = (k % per_row + 0.5) * n / per_row, (k // per_row + 0.5) * n / per_row
    h = _hash01(count * 8, 7000).reshape(count, 8)
    du = np.stack([-0.4 - 1.2 * h[:, 0], 0.4 + 1.2 * h[:, 2], 0.4 + 1.2 * h[:, 4], -0.4 - 1.2 * h[:, 6]], axis=1)
    dv = np.stack([-0.4 - 1.2 * h[:, 1], -0.4 - 1.2 * h[:, 3], 0.4 + 1.2 * h[:, 5], 0.4 + 1.2 * h[:, 7]], axis=1)
    u, v = cu[:, None] + du, cv[:, None] + dv
    xy = np.ascontiguousarray(np.stack([t6[2] + u.ravel() * t6[0], t6[5] + v.ravel() * t6[4]]))
    return xy, np.arange(count + 1, dtype=np.int64) * 4, np.arange(count, dtype=np.int32), count


def table_of(case: str, a) -> tuple:
    if case == "rgi_like":
        return stars(a.n, a.polygons, 32, 40.0, 300.0, 11)
    if case == "giant":
        xy, off, por, _ = stars(a.n, 1, 1000, 0.47 * a.n, 0.47 * a.n, 23)
        t6 = transform(a.n)
        xy[0] += t6[2] + 0.5 * a.n * t6[0] - xy[0].mean()   # about the grid's centre
        xy[1] += t6[5] + 0.5 * a.n * t6[4] - xy[1].mean()
        return xy, off, por, 1
    return lattice(a.n, a.small)


def child(a) -> None:
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench_rasterize.py measures the GPU: no device found")
    from xdem_amd import _lib, vector

    table = table_of(a.case, a)
    shape, t6 = (a.n, a.n), transform(a.n)
    ctx = _lib.default_context()
    dev = vector.DeviceRasterizer()
    burn = np.arange(1, table[3] + 1, dtype=np.int32)
    out = {"case": a.case, "polygons": int(table[3]), "vertices": int(table[0].shape[1])}
    if a.case == "giant":   # (a plausibility figure next to burnt_pixels: the star's area by the shoelace formula, in pixels)
        x, y = table[0][0] / t6[0], table[0][1] / t6[4]
        x, y = x - x.mean(), y - y.mean()
        out["shoelace_area_px"] = float(abs(np.sum(x * np.roll(y, -1) - np.roll(x, -1) * y)) / 2.0)
    for route in ("mask", "labels"):
        wall, device_ms = [], []
        for k in range(a.repeats + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            plane = dev.mask([table], shape, t6, device=True) if route == "mask" else dev.labels(table, burn, 0, shape, t6, device=True)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            if k:   # (the first round warms up)
                wall.append(dt)
                device_ms.append(ctx.last_kernel_ms())
            del plane
        ctx.set_option("vec_stage_times", 1)   # one more round under the stage events (kept out of the timed rounds)
        try:
            plane = dev.mask([table], shape, t6, device=True) if route == "mask" else dev.labels(table, burn, 0, shape, t6, device=True)
            del plane
            stages = dict(zip(("edges", "segments", "sorts", "spans", "finish"), dev.stage_ms()))
        finally:
            ctx.set_option("vec_stage_times", 0)
        out[route] = {"stage_ms": stages, "wall_s": wall, "wall_median_s": statistics.median(wall), "device_ms": device_ms,
                      "device_median_ms": statistics.median(device_ms), "launches": dev.launches(), "burnt_pixels": dev.last_count}
    if a.case == "rgi_like" and a.cpu_polygons > 0:
        from matplotlib.path import Path

        xy, off, _, count = table
        m = min(a.cpu_polygons, count)
        t0 = time.perf_counter()
        inside = 0
        for p in range(m):
            ring = xy[:, off[p]:off[p + 1]].T
            c0 = max(0, int((ring[:, 0].min() - t6[2]) / t6[0]))
            c1 = min(a.n, int((ring[:, 0].max() - t6[2]) / t6[0]) + 1)
            r0 = max(0, int((ring[:, 1].max() - t6[5]) / t6[4]))
            r1 = min(a.n, int((ring[:, 1].min() - t6[5]) / t6[4]) + 1)
            if c1 <= c0 or r1 <= r0:
                continue
            cx, cy = t6[2] + (np.arange(c0, c1) + 0.5) * t6[0], t6[5] + (np.arange(r0, r1) + 0.5) * t6[4]
            pts = np.stack([np.tile(cx, r1 - r0), np.repeat(cy, c1 - c0)], axis=1)
            inside += int(Path(ring).contains_points(pts).sum())
        dt = time.perf_counter() - t0
        out["cpu_standin"] = {"what": "matplotlib.path.Path.contains_points over the bounding-box pixel centres of each polygon, one thread",
                              "polygons": m, "seconds": dt, "scaled_to_table_s": dt * count / m, "pixels_inside": inside,
                              "note": "a stand-in: upstream's GDAL scanline fill is not installed and could not be run"}
    print("RESULT " + json.dumps(out))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=20000)
    ap.add_argument("--polygons", type=int, default=10000)
    ap.add_argument("--small", type=int, default=1000000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--limit", type=int, default=300, help="seconds per case")
    ap.add_argument("--cpu-polygons", type=int, default=100)
    ap.add_argument("--case", choices=CASES, default=None, help="(internal) run one case in this process")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vector_bench.json"))
    a = ap.parse_args()
    if a.case:
        child(a)
        return
    out = {"n": a.n, "repeats": a.repeats, "cases": {}}
    for case in CASES:
        cmd = [sys.executable, os.path.abspath(__file__), "--case", case, "--n", str(a.n), "--polygons", str(a.polygons), "--small", str(a.small),
               "--repeats", str(a.repeats), "--cpu-polygons", str(a.cpu_polygons)]
        try:
            done = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
        except subprocess.TimeoutExpired:
            out["cases"][case] = {"error": f"no result within {a.limit} s"}
            break   # (nothing more is started on a device that did not answer)
        lines = [ln for ln in done.stdout.splitlines() if ln.startswith("RESULT ")]
        if done.returncode != 0 or not lines:
            out["cases"][case] = {"error": f"exit status {done.returncode}", "stderr": done.stderr[-2000:]}
            break
        out["cases"][case] = json.loads(lines[-1][len("RESULT "):])
    try:
        import torch

        out["device"] = torch.cuda.get_device_name(0) if torch.cuda.is_available() else None
    except Exception:  # noqa: BLE001
        out["device"] = None
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
