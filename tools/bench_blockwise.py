"""Measurement of xdem_amd.coreg.BlockwiseCoreg (csrc/blockwise.hip); prints one JSON line and writes it to --out (default
profiles/blockwise_bench.json, one line per run appended with --append).  Nothing here asserts a time.

One synthetic N x N float32 pair, device-resident: an fBm reference DEM, the same surface moved by a fraction of a pixel, lifted and
with noise as the DEM to be aligned, 20 % gaps in it.  Wall clock, stream synchronised, of

  * the creation of the batched plan (tile-major copies + the aux pass) and ONE batched iteration of every tile;
  * a whole ``fit`` on the batched route, with the time spent inside the host's ``curve_fit`` calls (one per tile and iteration)
    counted by a wrapper: its share is what is left to gain on the host once the kernels are not the bound;
  * a whole ``fit`` on the loop route -- one ``NKPlan`` per tile, what the package could do per tile before the batched plan -- over
    the first --loop-tiles tiles, scaled to all tiles;
  * the warp of ``apply``.

--launches DIR: summarise a ``rocprofv3 --kernel-trace --output-format csv -d DIR`` trace of this command (run with --only step,
--only fit or --only warp) into the output instead: launches and device time per kernel.

    python tools/bench_blockwise.py [--n 20000] [--block 500] [--loop-tiles 100] [--only step|fit|loop|warp] [--out ...] [--append]
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
                rec = per.setdefault(name[4:], {"launches": 0, "ms": 0.0})
                rec["launches"] += 1
                rec["ms"] += (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6
    return dict(sorted(per.items()))


def inputs(N: int, dev):
    import torch

    from xdem_amd import synth

    ref = synth.fbm_torch(N, N, dev)
    gen = torch.Generator(device=dev).manual_seed(5)
    # the surface 0.3 pixel to the east and 0.2 pixel to the south of itself (linear blends of neighbours), 1 m up, 5 cm of noise
    tba = 0.7 * ref + 0.3 * torch.roll(ref, 1, dims=1)
    tba = 0.8 * tba + 0.2 * torch.roll(tba, -1, dims=0)
    tba += 1.0 + 0.05 * torch.randn((N, N), device=dev, generator=gen)
    tba[torch.rand((N, N), device=dev, generator=gen) < 0.2] = float("nan")
    return ref.contiguous(), tba.contiguous()


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=20000)
    ap.add_argument("--block", type=int, default=500)
    ap.add_argument("--loop-tiles", type=int, default=100)
    ap.add_argument("--only", choices=("step", "fit", "loop", "warp"), default=None)
    ap.add_argument("--launches", default=None)
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "blockwise_bench.json"))
    a = ap.parse_args()

    if a.launches:
        out = {"n": a.n, "block": a.block, "only": a.only, "kernels": summarise_launches(a.launches)}
    else:
        import scipy.optimize
        import torch

        from xdem_amd import blockwise, coreg

        dev = torch.device("cuda:0")
        N, res = a.n, 10.0
        ref, tba = inputs(N, dev)
        tiles = blockwise.tiling_grid((N, N), a.block).reshape(-1, 4)
        n = int(tiles.shape[0])
        out = {"n": N, "dtype": "float32", "block": a.block, "tiles": n, "device": torch.cuda.get_device_name(0)}

        def timed(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = fn()
            torch.cuda.synchronize()
            return r, time.perf_counter() - t0

        want = lambda k: a.only in (None, k)   # noqa: E731
        if want("step"):
            plan, out["plan_create_s"] = timed(lambda: blockwise.BWPlan(ref, tba, None, tiles))
            with plan:
                act, z = np.ones(n, dtype=np.uint8), np.zeros(n)
                res_out = plan.new_results(72)
                _, out["batched_step_first_s"] = timed(lambda: plan.step(act, z, z, (res, res), 72, res_out))
                _, out["batched_step_s"] = timed(lambda: plan.step(act, z + 1.0, z - 1.0, (res, res), 72, res_out))
                out["valid_per_tile_mean"] = float(plan.n_valid.mean())
        if want("fit"):
            spent = {"s": 0.0, "calls": 0}

            def counted_curve_fit(*args, **kwargs):
                t0 = time.perf_counter()
                try:
                    return scipy.optimize.curve_fit(*args, **kwargs)
                finally:
                    spent["s"] += time.perf_counter() - t0
                    spent["calls"] += 1

            b = coreg.BlockwiseCoreg(coreg.NuthKaab(fit_optimizer=counted_curve_fit), block_size_fit=a.block)
            _, out["fit_batched_s"] = timed(lambda: b.fit(ref, tba, resolution=res))
            assert b.fit_route == "batched"
            out["fit_batched_curve_fit_s"], out["fit_batched_curve_fit_calls"] = spent["s"], spent["calls"]
            out["fit_batched_curve_fit_share"] = spent["s"] / out["fit_batched_s"]
            out["fit_batched_iterations_max"] = int(b.n_iterations.max())
            out["fit_batched_tiles_without_fit"] = int(np.isnan(b.shifts_x).sum())
            out["fit_batched_median_shift"] = [float(np.nanmedian(v)) for v in (b.shifts_x, b.shifts_y, b.shifts_z)]
        if want("loop"):
            k = min(a.loop_tiles, n)
            b = coreg.BlockwiseCoreg(coreg.NuthKaab(), block_size_fit=a.block)
            t6 = blockwise._transform6(None, res)
            rows = int(tiles[:k, 1].max())   # host arrays, as NuthKaab.fit takes them: the rows that hold the timed tiles
            h_ref, h_tba = ref[:rows].cpu().numpy(), tba[:rows].cpu().numpy()
            b._fit_loop(h_ref, h_tba, None, tiles[:1], t6)   # (first call: the code objects load)
            shifts, t = timed(lambda: b._fit_loop(h_ref, h_tba, None, tiles[:k], t6))
            out["fit_loop_tiles_timed"], out["fit_loop_s_timed"], out["fit_loop_s_scaled_to_all_tiles"] = k, t, t * n / k
            out["fit_loop_median_shift"] = [float(np.nanmedian(v)) for v in shifts]
        if want("warp"):
            t6 = blockwise._transform6(None, res)
            cx, cy, cz = (2e-6, -1e-6, 3.0), (1e-6, 2e-6, -2.0), (0.0, 0.0, 1.0)
            blockwise.warp_affine_field(tba[:64].contiguous(), t6, cx, cy, cz)   # (first call: the code object loads)
            _, out["warp_s"] = timed(lambda: blockwise.warp_affine_field(tba, t6, cx, cy, cz))
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a" if a.append else "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
