"""Measurement of the ICP path (csrc/icp.hip); prints one JSON line and writes it to --out (default profiles/icp_bench.json).

One synthetic N x N float32 pair (a smooth surface, ``tba`` = the surface moved by about a pixel and tilted, noise, NaN holes) with the
default ``subsample = 5e5``:

  * a whole ``ICP().fit`` for the three routes -- point-to-plane with the default minimiser (Gauss-Newton on device sums),
    point-to-plane with "lsq_approx", point-to-point with the default minimiser: wall clock of the second of two fits, its iteration
    count, and the time per iteration;
  * the preparation alone (plan, normal planes, draw, gather, nine exact selections, grid build) and, on the clouds it leaves, the query
    kernel alone (device time between two events, median of --reps calls at alternating matrices), one picky selection and one
    evaluation of the sums (wall clock, each ends with its one synchronisation);
  * upstream's CPU path on the same clouds, on this host: ``scipy.spatial.KDTree`` build and one ``query(k=1)``, pandas'
    ``groupby().idxmin()`` and one ``scipy.optimize.least_squares`` on ``_icp_fit_func`` restated (``xdem_amd.icp.fit_func``) for
    point-to-plane (skipped with --skip-cpu; pandas only if it is installed).

    python tools/bench_icp.py [--n 4096] [--reps 7] [--skip-cpu] [--out profiles/icp_bench.json]
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


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--skip-cpu", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "icp_bench.json"))
    a = ap.parse_args()

    from xdem_amd import _lib, coreg, icp

    ctx = _lib.default_context()
    N = a.n
    out = {"n": N, "subsample": 5e5}
    t6 = (10.0, 0.0, 0.0, 0.0, -10.0, 10.0 * N)
    rng = np.random.default_rng(0)
    yy = np.arange(N, dtype=np.float32)[:, None]
    xx = np.arange(N, dtype=np.float32)[None, :]
    ref = (1000 + 120 * np.sin(xx / 90.0) * np.cos(yy / 70.0) + 40 * np.sin((xx + yy) / 50.0)).astype(np.float32)
    tba = (1000 + 120 * np.sin((xx + 1.2) / 90.0) * np.cos((yy - 0.8) / 70.0) + 40 * np.sin((xx + yy + 0.4) / 50.0) + 1.5 + 0.0004 * (xx - N / 2)
           + rng.normal(scale=0.02, size=(N, N))).astype(np.float32)
    ref[rng.random((N, N)) < 0.02] = np.nan
    tba[rng.random((N, N)) < 0.02] = np.nan

    routes = {"plane_default": {}, "plane_lsq_approx": {"fit_minimizer": "lsq_approx"}, "point_default": {"method": "point-to-point"}}
    for name, kw in routes.items():
        for _ in range(2):
            t0 = time.perf_counter()
            c = coreg.ICP(**kw).fit(ref, tba, transform=t6, random_state=0)
            wall = time.perf_counter() - t0
        its = c.meta["outputs"]["iterative"]["last_iteration"]
        out[f"fit_{name}_s"] = round(wall, 4)
        out[f"fit_{name}_iterations"] = its
        out[f"fit_{name}_translations"] = [round(float(v), 4) for v in c.to_translations()]

    # the pieces, on the clouds of the point-to-plane fit
    t0 = time.perf_counter()
    plan = coreg.DhPlan(ref, tba, ctx=ctx)
    icp.icp_normals(plan, t6, fetch=False)
    n = coreg.draw(plan, 5e5, 0)
    cloud = icp.IcpCloud.from_plan(plan, t6, True)
    ctx.synchronize()
    out["prepare_s"] = round(time.perf_counter() - t0, 4)
    out["points"] = n
    out["grid"] = list(cloud.grid()[3:])
    mats = [coreg.matrix_from_translations_rotations(0.03, -0.02, 0.005, 0.02, -0.01, 0.03), np.eye(4)]
    q_ms, p_ms, s_ms = [], [], []
    for i in range(a.reps + 1):
        cloud.query(mats[i % 2], fetch=False)
        ctx.synchronize()
        q_ms.append(ctx.last_kernel_ms())
        t0 = time.perf_counter()
        k = cloud.pairs(True)
        p_ms.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        cloud.sums(np.eye(4), "point-to-plane")
        s_ms.append((time.perf_counter() - t0) * 1e3)
    out["query_kernel_ms"] = round(float(np.median(q_ms[1:])), 4)
    out["picky_ms"] = round(float(np.median(p_ms[1:])), 4)
    out["sums_evaluation_ms"] = round(float(np.median(s_ms[1:])), 4)
    out["pairs_kept"] = k
    for name in routes:
        out[f"fit_{name}_per_iteration_ms"] = round(1e3 * (out[f"fit_{name}_s"] - out["prepare_s"]) / out[f"fit_{name}_iterations"], 3)

    if not a.skip_cpu:
        import scipy.optimize
        import scipy.spatial

        arr = cloud.cloud()
        ref_epc, tba_epc, norms = arr[:3], np.vstack((arr[:2], arr[3:4])), arr[4:]
        t0 = time.perf_counter()
        tree = scipy.spatial.KDTree(ref_epc.T)
        out["cpu_kdtree_build_s"] = round(time.perf_counter() - t0, 4)
        t0 = time.perf_counter()
        dists, ind = tree.query(tba_epc.T, k=1)
        out["cpu_kdtree_query_s"] = round(time.perf_counter() - t0, 4)
        try:
            import pandas as pd

            t0 = time.perf_counter()
            kept = pd.DataFrame(data={"ind": ind, "dists": dists}).groupby(["ind"]).idxmin()["dists"].values
            out["cpu_pandas_picky_s"] = round(time.perf_counter() - t0, 4)
        except ImportError:
            order = np.lexsort((np.arange(ind.size), dists, ind))
            kept = order[np.concatenate(([True], ind[order][1:] != ind[order][:-1]))]
        inputs = (ref_epc[:, ind[kept]], tba_epc[:, kept], norms[:, ind[kept]])
        t0 = time.perf_counter()
        res = scipy.optimize.least_squares(lambda p: icp.fit_func(inputs, p, "point-to-plane"), np.zeros(6), loss="linear")
        out["cpu_least_squares_s"] = round(time.perf_counter() - t0, 4)
        out["cpu_least_squares_nfev"] = int(res.nfev)
        out["cpu_iteration_s"] = round(out["cpu_kdtree_query_s"] + out.get("cpu_pandas_picky_s", 0.0) + out["cpu_least_squares_s"], 4)
    cloud.close()
    plan.close()
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
