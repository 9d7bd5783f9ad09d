"""Measurement of the CPD path (csrc/cpd.hip); prints one JSON line and writes it to --out (default profiles/cpd_bench.json).

One synthetic N x N float32 pair, device-resident (a smooth surface, ``tba`` = the surface moved by about a pixel and tilted, noise,
NaN holes).  At ``subsample`` 5e3 (upstream's default) and 5e4 (which upstream cannot run: 80 GB):

  * the preparation alone (plan, draw, gather, nine exact selections, the buffers of the E-step);
  * one ``estep`` on the clouds it leaves: wall clock with its one fetch, median of --reps calls, and the pair rate, N M pair
    evaluations per pass and two passes per E-step, in pair evaluations per second;
  * a whole default ``CPD().fit`` at that subsample: wall clock of the second of two fits and its iteration count.

And upstream's CPU E-step on clouds of the same size, on this host: the dense NumPy evaluation (tests/cpd_oracle.py's
``estep_dense`` in float64: the ``(3, M, N)`` differences and the ``(M, N)`` matrix, as ``_cpd_fit`` holds them) -- skipped with --skip-cpu.

    python tools/bench_cpd.py [--n 4096] [--reps 7] [--skip-cpu] [--out profiles/cpd_bench.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--skip-cpu", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cpd_bench.json"))
    a = ap.parse_args()

    import torch

    from xdem_amd import _lib, coreg, cpd

    ctx = _lib.default_context()
    N = a.n
    out = {"n": N}
    t6 = (10.0, 0.0, 0.0, 0.0, -10.0, 10.0 * N)
    rng = np.random.default_rng(0)
    yy = np.arange(N, dtype=np.float32)[:, None]
    xx = np.arange(N, dtype=np.float32)[None, :]
    ref = (1000 + 120 * np.sin(xx / 90.0) * np.cos(yy / 70.0) + 40 * np.sin((xx + yy) / 50.0)).astype(np.float32)
    tba = (1000 + 120 * np.sin((xx + 1.2) / 90.0) * np.cos((yy - 0.8) / 70.0) + 40 * np.sin((xx + yy + 0.4) / 50.0) + 1.5 + 0.0004 * (xx - N / 2)
           + rng.normal(scale=0.02, size=(N, N))).astype(np.float32)
    ref[rng.random((N, N)) < 0.02] = np.nan
    tba[rng.random((N, N)) < 0.02] = np.nan
    d_ref, d_tba = torch.from_numpy(ref).cuda(), torch.from_numpy(tba).cuda()
    torch.cuda.synchronize()

    for sub, tag in ((5e3, "5e3"), (5e4, "5e4")):
        t0 = time.perf_counter()
        plan = coreg.DhPlan(d_ref, d_tba, ctx=ctx)
        n = coreg.draw(plan, sub, 0)
        cloud = cpd.CpdCloud.from_plan(plan, t6)
        ctx.synchronize()
        out[f"prepare_{tag}_s"] = round(time.perf_counter() - t0, 4)
        out[f"points_{tag}"] = n
        _, sigma2 = cloud.estep(None, None, 0.0)
        e_ms = []
        for i in range(a.reps + 1):
            t0 = time.perf_counter()
            cloud.estep(None, sigma2 * (1.0 + 0.01 * (i % 2)), 0.0)
            e_ms.append((time.perf_counter() - t0) * 1e3)
        ms = float(np.median(e_ms[1:]))
        out[f"estep_{tag}_ms"] = round(ms, 4)
        out[f"pair_rate_{tag}_per_s"] = float(f"{2.0 * n * n / (ms * 1e-3):.4g}")
        if tag == "5e3" and not a.skip_cpu:
            import cpd_oracle
            import icp_oracle

            flat = np.flatnonzero(np.isfinite(ref) & np.isfinite(tba))
            pick = np.sort(np.random.default_rng(0).choice(flat, size=n, replace=False))
            rows, cols = np.divmod(pick, N)
            x, y = t6[2] + (cols + 0.5) * t6[0], t6[5] + (rows + 0.5) * t6[4]
            X, TY = icp_oracle.standardize(np.vstack((x, y, ref.ravel()[pick])), np.vstack((x, y, tba.ravel()[pick])))[:2]
            t0 = time.perf_counter()
            cpd_oracle.estep_dense(X, TY, sigma2, 0.0, dtype=np.float64)
            out["cpu_dense_estep_5e3_s"] = round(time.perf_counter() - t0, 4)
        cloud.close()
        plan.close()
        for _ in range(2):
            t0 = time.perf_counter()
            c = coreg.CPD(subsample=sub).fit(d_ref, d_tba, transform=t6, random_state=0)
            wall = time.perf_counter() - t0
        out[f"fit_{tag}_s"] = round(wall, 4)
        out[f"fit_{tag}_iterations"] = c.meta["outputs"]["iterative"]["last_iteration"]
        out[f"fit_{tag}_translations"] = [round(float(v), 4) for v in c.to_translations()]
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
