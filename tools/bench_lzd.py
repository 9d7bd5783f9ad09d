"""Measurement of the LZD path (csrc/rigid.hip); prints one JSON line.

  * the normal-equation pass (``xdemhip_dh_lzd_normal``) at N x N float32, device-resident (torch tensors), with every valid pixel (dense
    route) and with 5e5 drawn pixels (list route): milliseconds, median of --reps calls at alternating matrices, wall clock around the
    call (each call ends with its one synchronisation);
  * the regrid pass (``xdemhip_apply_matrix_rst``) at N x N float32, device to device, for a rotation of 0.5 degrees: milliseconds
    (synchronised around the call);
  * end to end: a whole default ``LZD().fit`` on N x N host arrays (wall clock, one warm-up run first) and its iteration count.

    python tools/bench_lzd.py [--n 20000] [--reps 7] [--skip-e2e]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=20000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--skip-e2e", action="store_true")
    a = ap.parse_args()
    import torch

    from xdem_amd import _args, _lib, coreg, rigid

    ctx = _lib.default_context()
    N = a.n
    out = {"n": N}
    t6 = (10.0, 0.0, 0.0, 0.0, -10.0, 10.0 * N)
    yy = np.arange(N, dtype=np.float32)[:, None]
    xx = np.arange(N, dtype=np.float32)[None, :]
    href = (1000 + 40 * np.sin(xx / 50.0) * np.cos(yy / 70.0) + 25 * np.sin((xx + yy) / 31.0)).astype(np.float32)
    htba = (1000 + 40 * np.sin((xx + 0.4) / 50.0) * np.cos((yy - 0.3) / 70.0) + 25 * np.sin((xx + yy + 0.1) / 31.0) + 1.0).astype(np.float32)
    dev = torch.device("cuda", 0)
    ref, tba = torch.from_numpy(href).to(dev), torch.from_numpy(htba).to(dev)
    torch.cuda.synchronize()
    mats = [coreg.matrix_from_translations_rotations(3.0, -2.0, 1.0, 0.002, -0.001, 0.003), np.eye(4)]
    for name, sub in (("dense", 1), ("list_5e5", 5e5)):
        with coreg.DhPlan(ref, tba, ctx=ctx) as plan:
            coreg.draw(plan, sub, 0)
            cen, _ = rigid.lzd_centroid(plan, t6)
            ms = []
            for i in range(a.reps + 2):
                t0 = time.perf_counter()
                rigid.lzd_normal(plan, t6, mats[i % 2], cen)
                ms.append((time.perf_counter() - t0) * 1e3)
            out[f"normal_{name}_ms"] = round(float(np.median(ms[2:])), 3)   # (the first call makes the plan's buffers)
    del ref
    res = torch.empty_like(tba)
    m = coreg.matrix_from_translations_rotations(3.0, -2.0, 1.0, 0.5, -0.3, 0.4)
    cen = (5.0 * N, 5.0 * N, 1000.0)
    ms = []
    for i in range(a.reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ctx.check(ctx._L.xdemhip_apply_matrix_rst(ctx.handle, tba.data_ptr(), _lib.F32, N, N, _args.c_doubles(t6), _args.c_doubles(m.ravel()),
                                                  _args.c_doubles(cen), res.data_ptr(), _lib.DEVICE))
        ctx.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    out["regrid_ms"] = round(float(np.median(ms[1:])), 3)
    del tba, res
    torch.cuda.empty_cache()
    if not a.skip_e2e:
        for _ in range(2):
            t0 = time.perf_counter()
            c = coreg.LZD().fit(href, htba, transform=t6, random_state=0)
            wall = time.perf_counter() - t0
        out["e2e_fit_s"] = round(wall, 3)
        out["e2e_iterations"] = c.meta["outputs"]["iterative"]["last_iteration"]
        out["e2e_translations"] = [round(float(v), 4) for v in c.to_translations()]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
