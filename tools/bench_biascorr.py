"""Measurement of the Deramp / VerticalShift path (csrc/biascorr.hip); prints one JSON line.

  * the moments pass (xdemhip_dh_poly_moments, order 2, whole raster) and the apply pass (xdemhip_poly2d_apply) at N x N float32,
    device-resident (torch tensors): milliseconds (median of --reps, hipEvents around the launches) and the fraction of 8 TB/s at the
    algorithmic bytes -- 8 B/px read for the moments (ref + tba; 9 with an inlier mask), 4 + 4 B/px for the apply;
  * end to end: NuthKaab() + Deramp() fit_and_apply on M x M host arrays (wall clock, one warm-up run first);
  * a CPU baseline: scipy.optimize.curve_fit of a local order-2 polynomial on the same draw of 5e5 points.

    python tools/bench_biascorr.py [--n 40000] [--m 20000] [--reps 5] [--skip-e2e]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK = 8.0e12


def _poly2(xx, *p):
    c = np.array(p).reshape(3, 3)
    return np.polynomial.polynomial.polyval2d(xx[0], xx[1], c)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=40000)
    ap.add_argument("--m", type=int, default=20000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-e2e", action="store_true")
    a = ap.parse_args()
    import scipy.optimize
    import torch

    from xdem_amd import _lib, coreg
    from xdem_amd.biascorr import DhPlan, poly2d_apply

    ctx = _lib.default_context()
    out = {"n": a.n}
    N = a.n
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev)
    g.manual_seed(0)
    ref = torch.randn((N, N), device=dev, dtype=torch.float32, generator=g)
    tba = ref - 0.5
    torch.cuda.synchronize()
    with DhPlan(ref, tba, ctx=ctx) as plan:
        ms = []
        for _ in range(a.reps + 1):
            plan.poly_moments(2)
            ms.append(ctx.last_kernel_ms())
        t = float(np.median(ms[1:]))
        out["moments_ms"] = round(t, 3)
        out["moments_frac_8tbs"] = round(8.0 * N * N / (t * 1e-3) / PEAK, 3)
    res = torch.empty_like(ref)
    params = np.array([1.0, 1e-4, 1e-9, -2e-4, 1e-9, 0.0, 1e-9, 0.0, 0.0])
    ms = []
    for _ in range(a.reps + 1):
        poly2d_apply(ref, params, ctx=ctx, out=res)
        ms.append(ctx.last_kernel_ms())
    t = float(np.median(ms[1:]))
    out["apply_ms"] = round(t, 3)
    out["apply_frac_8tbs"] = round(8.0 * N * N / (t * 1e-3) / PEAK, 3)
    del ref, tba, res
    torch.cuda.empty_cache()

    M = a.m
    rng = np.random.default_rng(1)
    yy = np.arange(M, dtype=np.float32)[:, None]
    xx = np.arange(M, dtype=np.float32)[None, :]
    href = (1000 + 40 * np.sin(xx / 50.0) * np.cos(yy / 70.0)).astype(np.float32)
    htba = (1000 + 40 * np.sin((xx + 1.5) / 50.0) * np.cos((yy - 0.5) / 70.0) + 1.0 + 1e-4 * xx - 2e-4 * yy).astype(np.float32)
    if not a.skip_e2e:
        walls = []
        for _ in range(2):
            t0 = time.perf_counter()
            pipe = coreg.NuthKaab() + coreg.Deramp()
            pipe.fit_and_apply(href, htba, fit_kwargs={"resolution": 1.0}, random_state=0)
            walls.append(time.perf_counter() - t0)
        out["e2e_nk_deramp_s"] = round(walls[-1], 3)
        out["e2e_m"] = M
    # CPU baseline: the same draw of 5e5 valid points, scipy curve_fit of an order-2 polynomial
    valid = np.isfinite(href) & np.isfinite(htba)
    n_valid = int(valid.sum())
    ranks = coreg.subsample_ranks(n_valid, 5e5, 0)
    flat = np.flatnonzero(valid.ravel())[np.sort(ranks)]
    y, x = np.divmod(flat, M)
    dh = href.ravel()[flat] - htba.ravel()[flat]
    t0 = time.perf_counter()
    scipy.optimize.curve_fit(_poly2, np.array([x, y]), dh, p0=np.ones(9), absolute_sigma=True)
    out["cpu_curve_fit_5e5_s"] = round(time.perf_counter() - t0, 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
