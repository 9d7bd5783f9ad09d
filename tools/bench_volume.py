"""Measurement of xdem_amd.volume (csrc/volume.hip); prints one JSON line and writes it to --out (default
profiles/volume_bench.json).  Nothing here asserts a time.

One synthetic N x N float32 pair, device-resident: an fBm reference DEM, a dDEM with an elevation trend, noise and 20 % voids, and
--glaciers square outlines on a grid (labels 1 .. G, label 0 between them).  Wall clock, stream synchronised, of one call each of

  * hypsometric_binning (50 m bins), hypsometric_interpolation (mask = every outline), get_regional_hypsometric_signal and
    norm_regional_hypsometric_interpolation, end to end (the per-glacier host work -- pandas interval arithmetic and one
    scipy.optimize.curve_fit each -- is inside the last two);
  * the device calls of the regional interpolation alone: label statistics, segments (with standard deviations), fill;
  * the CPU route in upstream's shape on a --cpu-n x --cpu-n crop: per glacier a full-raster mask, the inlier extraction,
    np.digitize and a median per bin (what volume.py:604-650 does around hypsometric_binning), for --cpu-glaciers outlines; the
    time per glacier scales with the raster's pixels, so the full figure is per-glacier time x (N / n)^2 x G -- skipped with
    --skip-cpu.

--launches DIR: summarise a ``rocprofv3 --kernel-trace --output-format csv -d DIR`` trace of this command (run with
--only-regional) into --out instead: launches and device time per kernel.  Two such runs with different --glaciers show that the
number of raster passes does not depend on the number of glaciers.

    python tools/bench_volume.py [--n 20000] [--glaciers 3025] [--cpu-n 2000] [--cpu-glaciers 8] [--skip-cpu] [--out ...]
"""
from __future__ import annotations

import argparse
import csv
import glob
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]


def summarise_launches(src: str) -> dict:
    per: dict = {}
    for path in glob.glob(os.path.join(src, "**", "*kernel_trace.csv"), recursive=True):
        with open(path, newline="") as f:
            for r in csv.DictReader(f):
                name = r["Kernel_Name"].replace("(anonymous namespace)::", "").replace("void ", "")
                name = name.split("(")[0].split("<")[0]
                if not name.startswith("xd::"):
                    continue   # (torch's kernels of the input synthesis)
                name = name[4:]
                rec = per.setdefault(name, {"launches": 0, "ms": 0.0})
                rec["launches"] += 1
                rec["ms"] += (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6
    return dict(sorted(per.items()))


def inputs(N: int, G: int, dev):
    import torch

    from xdem_amd import synth

    ref = synth.fbm_torch(N, N, dev)
    gen = torch.Generator(device=dev).manual_seed(3)
    ddem = -0.01 * (ref - 1000.0) + 0.5 * (torch.rand((N, N), device=dev, generator=gen) - 0.5)
    ddem[torch.rand((N, N), device=dev, generator=gen) < 0.2] = float("nan")
    side = max(1, int(np.sqrt(G)))
    cell = N // side
    r = torch.arange(N, device=dev)
    inside = ((r % cell) >= cell // 8) & ((r // cell) < side)
    labels = ((r // cell)[:, None] * side + (r // cell)[None, :] + 1).to(torch.int32)
    labels *= (inside[:, None] & inside[None, :]).to(torch.int32)
    return ddem, ref, labels, side * side


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=20000)
    ap.add_argument("--glaciers", type=int, default=3025)
    ap.add_argument("--cpu-n", type=int, default=2000)
    ap.add_argument("--cpu-glaciers", type=int, default=8)
    ap.add_argument("--skip-cpu", action="store_true")
    ap.add_argument("--only-regional", action="store_true")
    ap.add_argument("--launches", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "volume_bench.json"))
    a = ap.parse_args()

    if a.launches:
        out = {"n": a.n, "glaciers": a.glaciers, "kernels": summarise_launches(a.launches)}
    else:
        import torch

        from xdem_amd import volume

        dev = torch.device("cuda:0")
        N = a.n
        ddem, ref, labels, G = inputs(N, a.glaciers, dev)
        torch.cuda.synchronize()
        out = {"n": N, "dtype": "float32", "glaciers": G, "device": torch.cuda.get_device_name(0)}

        def timed(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = fn()
            torch.cuda.synchronize()
            return r, time.perf_counter() - t0

        if not a.only_regional:
            _, out["hypsometric_binning_s"] = timed(lambda: volume.hypsometric_binning(ddem, ref))
            _, out["hypsometric_interpolation_s"] = timed(lambda: volume.hypsometric_interpolation(ddem, ref, labels > 0))
            _, out["get_regional_hypsometric_signal_s"] = timed(lambda: volume.get_regional_hypsometric_signal(ddem, ref, labels))
        signal = volume.get_regional_hypsometric_signal(ddem, ref, labels) if a.only_regional else _
        _, out["norm_regional_hypsometric_interpolation_s"] = timed(
            lambda: volume.norm_regional_hypsometric_interpolation(ddem, ref, labels, regional_signal=signal))
        if not a.only_regional:
            with volume.HypsoPlan(ddem, ref, labels=labels) as plan:
                st, t_stats = timed(plan.label_stats)
                keep = st["inliers"] > 0
                edges = np.linspace(st["ref_min"][keep], st["ref_max"][keep], 21).T
                (counts, med, _sd), t_seg = timed(lambda: plan.segments(st["ids"][keep], edges, want_std=True))
                xs = np.ascontiguousarray(0.5 * (edges[:, 1:] + edges[:, :-1]))
                _, t_fill = timed(lambda: plan.fill(0, st["ids"][keep], xs, np.nan_to_num(med), False, np.float32))
            out["device_calls_s"] = {"label_stats": t_stats, "segments_with_std": t_seg, "fill": t_fill}
            out["longest_segment"] = int(counts.max())
        if not a.skip_cpu and not a.only_regional:
            n = min(a.cpu_n, N)
            c_ddem, c_ref, c_lab = ddem[:n, :n].cpu().numpy(), ref[:n, :n].cpu().numpy(), labels[:n, :n].cpu().numpy()
            ids = [i for i in np.unique(c_lab) if i != 0][: a.cpu_glaciers]
            nans = ~np.isfinite(c_ddem)
            t0 = time.perf_counter()
            for i in ids:
                glacier = c_lab == i
                inlier = glacier & ~nans
                if np.count_nonzero(inlier) / np.count_nonzero(glacier) < 0.05:
                    continue
                d, e = c_ddem[inlier], c_ref[inlier]
                z = np.linspace(e.min(), e.max() + 1e-6 / 20, 21)
                idx = np.digitize(e, z)
                for b in range(20):
                    v = d[idx == b + 1]
                    if v.shape[0]:
                        np.median(v)
            per = (time.perf_counter() - t0) / max(len(ids), 1)
            out["cpu"] = {"n": n, "glaciers_timed": len(ids), "signal_s_per_glacier": per, "signal_s_scaled_to_n_and_G": per * (N / n) ** 2 * G}
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
