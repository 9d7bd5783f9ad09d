"""Golden vectors for Deramp / VerticalShift, recorded from the REFERENCE's own functions (needs the reference source tree, so it
runs only where that tree is present; the fixtures it writes are what the tests read).

For float32 DEM pairs of 129 x 193 with NaNs and an inlier mask, at poly_order 1, 2 and 3:
  * fit_params / fit_perr of the reference's ``_bin_or_and_fit_nd("fit", ..., p0=ones)`` (xdem/coreg/base.py:906-1000) on the valid
    pixels with ``xdem.fit.polynomial_2d`` and ``scipy.optimize.curve_fit`` -- the call Deramp._fit_rst_rst makes
    (xdem/coreg/biascorr.py:663-695) after ``_preprocess_pts_rst_subsample``;
  * the reference's applied output ``(elev + polynomial_2d((xx, yy), *params)).astype("float32")`` (biascorr.py:262-311, 740-745 and
    the cast of base.py:491);
  * ``float(np.median(dh))`` for VerticalShift (affine.py:721-770), on float32 and float64 dh.
The valid mask (inlier & finite ref & finite tba, base.py:652-663) is restated here: ``_preprocess_pts_rst_subsample`` draws the
subsample through geoutils, which is absent; the fixtures use subsample = 1 (every valid pixel), where no draw takes place.

Also records tests/golden/signatures_biascorr.json: the signatures of Deramp.__init__, VerticalShift.__init__ and
CoregPipeline.__init__ / fit / apply (parameter names, order, plain-literal defaults).

    python tools/gen_golden_biascorr.py
"""
from __future__ import annotations

import inspect
import json
import os
import sys

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
    if isinstance(v, (tuple, list)) and all(x is None or isinstance(x, (bool, int, float, str)) for x in v):
        return list(v)
    return "<object>"


def _record(fn) -> list:
    return [{"name": n, "kind": p.kind.name, "default": _literal(p.default)} for n, p in inspect.signature(fn).parameters.items()]


def pair(rng, H, W, dtype):
    """A DEM pair whose difference is a smooth 2-D surface plus noise, with NaNs in both and a patchy inlier mask."""
    yy, xx = np.mgrid[0:H, 0:W]
    ref = 800 + 30 * np.sin(xx / 17.0) + 20 * np.cos(yy / 11.0) + np.cumsum(rng.normal(scale=0.2, size=(H, W)), 1)
    ramp = 1.5 + 0.02 * xx - 0.03 * yy + 1e-4 * xx * yy - 8e-5 * xx ** 2 + 5e-5 * yy ** 2
    tba = ref - ramp + rng.normal(scale=0.3, size=(H, W))
    ref, tba = ref.astype(dtype), tba.astype(dtype)
    ref[rng.random((H, W)) < 0.03] = np.nan
    tba[rng.random((H, W)) < 0.03] = np.nan
    tba[5:9, 20:31] = np.nan
    inlier = np.ones((H, W), dtype=bool)
    inlier[60:80, 100:140] = False
    inlier[rng.random((H, W)) < 0.02] = False
    return ref, tba, inlier


def main() -> None:
    import scipy.optimize

    ref_mods = _refimport.load()
    import importlib

    base = ref_mods.base
    fit = importlib.import_module("xdem.fit")
    biascorr = importlib.import_module("xdem.coreg.biascorr")
    affine = ref_mods.affine

    rng = np.random.default_rng(2024)
    H, W = 129, 193
    rec = {"H": H, "W": W}
    ref32, tba32, inlier = pair(rng, H, W, np.float32)
    rec["ref"], rec["tba"], rec["inlier"] = ref32, tba32, inlier
    valid = inlier & np.isfinite(ref32) & np.isfinite(tba32)
    xx, yy = np.meshgrid(np.arange(0, W), np.arange(0, H))
    dh = ref32[valid] - tba32[valid]
    for order in (1, 2, 3):
        params_fit_or_bin = {"fit_or_bin": "fit", "fit_func": fit.polynomial_2d, "fit_optimizer": scipy.optimize.curve_fit,
                             "bin_sizes": 10, "bin_statistic": np.nanmedian, "bias_var_names": ["xx", "yy"], "nd": 2}
        p0 = np.ones(shape=((order + 1) ** 2))
        _, results = base._bin_or_and_fit_nd(fit_or_bin="fit", params_fit_or_bin=params_fit_or_bin, values=dh,
                                             bias_vars={"xx": xx[valid], "yy": yy[valid]}, weights=None, p0=p0)
        params = results[0]
        perr = np.sqrt(np.diag(results[1]))
        applied = (tba32 + fit.polynomial_2d((xx, yy), *params)).astype("float32")
        rec[f"o{order}_fit_params"] = params
        rec[f"o{order}_fit_perr"] = perr
        rec[f"o{order}_applied"] = applied
        sse = float(np.sum((dh.astype(np.float64) - fit.polynomial_2d((xx[valid], yy[valid]), *params)) ** 2))
        rec[f"o{order}_sse"] = sse
    # VerticalShift: float(np.median(dh)) on the valid pixels, float32 and float64 pairs
    rec["vshift_f32"] = float(np.median(dh))
    ref64, tba64 = ref32.astype(np.float64) + 0.1, tba32.astype(np.float64)
    rec["vshift_f64"] = float(np.median(ref64[valid] - tba64[valid]))
    out = os.path.join(GOLDEN, "biascorr_golden.npz")
    np.savez_compressed(out, **rec)
    print(out, os.path.getsize(out), "bytes")

    sig = {"coreg": {"Deramp.__init__": _record(biascorr.Deramp.__init__),
                     "VerticalShift.__init__": _record(affine.VerticalShift.__init__),
                     "CoregPipeline.__init__": _record(base.CoregPipeline.__init__),
                     "CoregPipeline.fit": _record(base.CoregPipeline.fit),
                     "CoregPipeline.apply": _record(base.CoregPipeline.apply)}}
    with open(os.path.join(GOLDEN, "signatures_biascorr.json"), "w") as f:
        json.dump(sig, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
