"""Golden vectors for DhMinimize, recorded from the REFERENCE's own driver (needs the reference source tree, so it runs only where that
tree is present; the fixtures it writes are what the tests read).

For one float32 and one float64 DEM pair of 96 x 128 with NaN holes and an inlier mask, the reference's ``_dh_minimize_fit``
(xdem/coreg/affine.py:636-674) is run with ``fit_minimizer = scipy.optimize.minimize`` (so: Nelder-Mead from (1, 1)) and
``fit_loss_func = binning_oracle.nmad``.  Its ``dh_interpolator`` is built from ``nuthkaab_oracle.shifted_dh`` restricted to the sample
mask (inlier & finite ref & finite tba, base.py:652-663; subsample = 1): geoutils' interpolator is absent here, so the interpolation
is the stated convention of oracle/nuthkaab_oracle.py -- parity unpinned -- and only the DRIVER is pinned by the reference.  The nodata
rule of that convention is switchable (``nk_nan_rule``), so every case is recorded once per rule 0..3.

tests/golden/dhminimize_golden.npz holds, per case ``c`` in (f32, f64): ``c_ref``, ``c_tba``, ``c_inlier``, ``c_mask``, ``c_res`` and, per rule
``r``, ``c_r{r}_traj`` -- every (x, y, loss) the reference's minimiser evaluated, in order, as float64 rows -- and ``c_r{r}_offsets``, the
three returned offsets (easting, northing, vertical).

Also records tests/golden/signatures_dhminimize.json: the signatures of DhMinimize.__init__ and of the ``fit`` / ``apply`` it inherits.

    python tools/gen_golden_dhminimize.py
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
import binning_oracle  # noqa: E402
import nuthkaab_oracle  # noqa: E402

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


def surface(xx, yy):
    return 800.0 + 40.0 * np.sin(xx / 9.0) * np.cos(yy / 7.0) + 15.0 * np.sin((xx + yy) / 5.0)


def pair(rng, H, W, dtype, dx, dy, dz):
    """tba = the surface of ref sampled (dx, dy) pixels away, minus dz, plus noise; NaNs in both, a patchy inlier mask."""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    ref = surface(xx, yy).astype(dtype)
    tba = (surface(xx + dx, yy + dy) - dz + rng.normal(scale=0.05, size=(H, W))).astype(dtype)
    ref[rng.random((H, W)) < 0.03] = np.nan
    tba[rng.random((H, W)) < 0.03] = np.nan
    tba[30:34, 50:61] = np.nan
    inlier = np.ones((H, W), dtype=bool)
    inlier[60:75, 20:45] = False
    inlier[rng.random((H, W)) < 0.02] = False
    return ref, tba, inlier


def main() -> None:
    import scipy.optimize

    ref_mods = _refimport.load()
    affine = ref_mods.affine
    base = ref_mods.base

    rng = np.random.default_rng(617)
    H, W = 96, 128
    rec = {}
    for name, dtype, res, (dx, dy, dz) in (("f32", np.float32, (10.0, 10.0), (1.3, -0.8, 2.5)),
                                           ("f64", np.float64, (5.0, 7.5), (-0.6, 1.7, -1.25))):
        ref, tba, inlier = pair(rng, H, W, dtype, dx, dy, dz)
        mask = inlier & np.isfinite(ref) & np.isfinite(tba)
        rec[f"{name}_ref"], rec[f"{name}_tba"], rec[f"{name}_inlier"], rec[f"{name}_mask"] = ref, tba, inlier, mask
        rec[f"{name}_res"] = np.array(res, dtype=np.float64)
        for rule in range(4):
            calls = []

            def dh_interpolator(x, y):
                d = nuthkaab_oracle.shifted_dh(ref, tba, float(x), float(y), res, rule)[mask]
                calls.append((float(x), float(y), float(binning_oracle.nmad(d))))
                return d

            params = {"fit_or_bin": "fit", "fit_minimizer": scipy.optimize.minimize, "fit_loss_func": binning_oracle.nmad}
            offsets = affine._dh_minimize_fit(dh_interpolator=dh_interpolator, params_fit_or_bin=params)
            # (the last call is the driver's own: dh at the optimum for the vertical offset, not an evaluation of the minimiser)
            rec[f"{name}_r{rule}_traj"] = np.array(calls[:-1], dtype=np.float64)
            rec[f"{name}_r{rule}_offsets"] = np.array([float(v) for v in offsets], dtype=np.float64)
            print(name, "rule", rule, "evaluations", len(calls) - 1, "offsets", offsets)
    out = os.path.join(GOLDEN, "dhminimize_golden.npz")
    np.savez_compressed(out, **rec)
    print(out, os.path.getsize(out), "bytes")

    sig = {"coreg": {"DhMinimize.__init__": _record(affine.DhMinimize.__init__),
                     "DhMinimize.fit": _record(affine.DhMinimize.fit),
                     "DhMinimize.apply": _record(affine.DhMinimize.apply)}}
    assert affine.DhMinimize.fit is base.Coreg.fit
    with open(os.path.join(GOLDEN, "signatures_dhminimize.json"), "w") as f:
        json.dump(sig, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
