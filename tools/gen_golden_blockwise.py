"""Golden vectors for BlockwiseCoreg, recorded from the REFERENCE's own ``BlockwiseCoreg._ransac`` (needs the reference source tree, so it
runs only where that tree is present; the fixtures it writes are what the tests read).

xdem/coreg/blockwise.py imports geopandas, geoutils and rasterio, which are absent: oracle/_refimport.py installs its stub modules in
``sys.modules`` first, then the reference module is imported as it is -- ``_ransac`` itself needs NumPy and scikit-learn only.

tests/golden/blockwise_golden.npz holds, per case ``c``: ``c_x``, ``c_y``, ``c_shifts`` (the inputs) and ``c_coeff`` = the returned
``(a, b, c)`` as float64, with ``threshold=0.01, max_iterations=2000`` under ``np.random.seed(0)``:

* ``planar``   a 4 x 6 grid of tile centres at absolute UTM-sized coordinates, exactly planar shifts with 4 gross outliers (RANSAC branch;
               the fit of the 20 inliers does not depend on which minimal samples were drawn: ``planar_seed_spread`` records the largest
               difference of a coefficient over 8 global seeds, 0.0)
* ``allnan``   the same centres, an all-NaN field (becomes zeros)
* ``onerow``   a single row of tiles (``np.polyfit`` along x)
* ``onecol``   a single column of tiles (``np.polyfit`` along y)
* ``onetile``  one tile

Also records tests/golden/signatures_blockwise.json: the signatures of ``__init__``, ``fit``, ``apply`` and ``_ransac``.

    python tools/gen_golden_blockwise.py
"""
from __future__ import annotations

import importlib
import inspect
import json
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import _refimport  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")


def _literal(v):
    if v is inspect.Parameter.empty:
        return "<required>"
    if v is None or isinstance(v, (bool, int, float, str)):
        return v
    return "<object>"


def _record(fn) -> list:
    return [{"name": n, "kind": p.kind.name, "default": _literal(p.default)} for n, p in inspect.signature(fn).parameters.items()]


def cases() -> dict:
    block, res, x0, y0 = 500, 10.0, 412000.0, 5178000.0
    cols, rows = np.meshgrid(np.arange(6) * block + block / 2, np.arange(4) * block + block / 2)
    x, y = (x0 + res * cols).ravel(), (y0 - res * rows).ravel()
    planar = 2.5e-4 * (x - x0) - 1.25e-4 * (y - y0) + 3.0
    planar[[3, 8, 14, 21]] += np.array([7.0, -5.5, 12.0, -9.25])
    return {
        "planar": (x, y, planar),
        "allnan": (x, y, np.full(x.size, np.nan)),
        "onerow": (x[:6], y[:6], 1.5e-4 * (x[:6] - x0) - 2.0 + np.array([0.0, 0.01, -0.02, 0.005, 0.0, -0.01])),
        "onecol": (x[::6], y[::6], -3.0e-4 * (y[::6] - y0) + 0.75 + np.array([0.02, 0.0, -0.01, 0.015])),
        "onetile": (x[:1], y[:1], np.array([1.25])),
    }


def main() -> None:
    _refimport.install()
    bw = importlib.import_module("xdem.coreg.blockwise").BlockwiseCoreg
    rec = {}
    for name, (x, y, s) in cases().items():
        np.random.seed(0)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")   # (np.polyfit on one point: RankWarning)
            coeff = np.array([float(v) for v in bw._ransac(x, y, s, 0.01, 2000)], dtype=np.float64)
        rec[f"{name}_x"], rec[f"{name}_y"], rec[f"{name}_shifts"], rec[f"{name}_coeff"] = x, y, s, coeff
        print(name, coeff)
    x, y, s = cases()["planar"]
    runs = []
    for seed in range(8):
        np.random.seed(seed)
        runs.append([float(v) for v in bw._ransac(x, y, s, 0.01, 2000)])
    rec["planar_seed_spread"] = np.array(np.ptp(np.array(runs), axis=0).max())
    print("spread over 8 seeds:", rec["planar_seed_spread"])
    out = os.path.join(GOLDEN, "blockwise_golden.npz")
    np.savez_compressed(out, **rec)
    print(out, os.path.getsize(out), "bytes")
    sig = {"coreg": {f"BlockwiseCoreg.{m}": _record(getattr(bw, m)) for m in ("__init__", "fit", "apply", "_ransac")}}
    with open(os.path.join(GOLDEN, "signatures_blockwise.json"), "w") as f:
        json.dump(sig, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
