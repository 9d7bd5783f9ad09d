"""Golden vectors for BiasCorr / DirectionalBias / TerrainBias, recorded from the REFERENCE's own methods (needs the reference
source tree, so it runs only where that tree is present; the fixtures it writes are what the tests read).

Inputs: ``xdem_amd.synth.bias_case(H, W, dtype)`` -- float32 and float64 DEM pairs of 61 x 83 and 129 x 193 with NaNs in both
rasters, NaNs in a variable plane and a patchy inlier mask, built from exactly rounded arithmetic on hashed integers, so the tests
rebuild them bit for bit and nothing of them is stored.  The valid mask (inlier & finite ref & finite tba & finite every variable,
base.py:653-661) is restated here: upstream draws it through geoutils, which is absent; the fixtures use subsample = 1.

Per binning case -- 1 variable with bin_sizes 1, 10, 100; 2 variables with bin_sizes 6 and with a dict of edge arrays; 3 variables
4 x 3 x 5 -- the reference's ``BiasCorr(fit_or_bin="bin", ...)._bin_or_and_fit_nd(values, bias_vars)`` (biascorr.py:40-165,
base.py:906-1050, 2749-2807) gives the DataFrame: recorded as its columns (``nd``, ``nanmedian``, ``count`` and the interval ends
of every variable, NaN where a row has none), for both shapes and dtypes.  For the 61 x 83 inputs the reference's ``_apply_rst``
(biascorr.py:261-311) gives the correction: with ``elev = 0`` (float64) its result IS ``corr`` (``0 + corr``), recorded in float64
for ``bin_apply_method`` "linear" (min_count 0 and 5) and "per_bin"; the applied array is then ``elev + corr`` cast to the raster
dtype (base.py:491), one NumPy addition the tests repeat -- a few cases record the applied array too, to show it is that.  The
apply planes carry values exactly on inner edges, on the rightmost edge, outside the grid, NaN, and in empty bins.

The two named workflows are recorded on a binned table: ``fit_or_bin="bin_and_fit"`` with ``fit_func="norder_polynomial"`` and
``"nfreq_sumsin"`` (``random_state=42, niter=3`` for basinhopping): the table's (x, y), ``fit_params``, the ``specific`` outputs,
and ``corr`` of ``_apply_rst`` on the 61 x 83 planes.

Also: what upstream does with a dict of INTEGER bin sizes for two variables (a TypeError out of SciPy), the constructors'
TypeError / ValueError messages (tests/golden/bincorr_errors.json) and the signatures of the three constructors
(tests/golden/signatures_bincorr.json).

    python tools/gen_golden_bincorr.py
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
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

GOLDEN = os.path.join(ROOT, "tests", "golden")

# (name, variables of the fit, bin_sizes): shared with tests/test_bincorr_gpu.py through the fixture's "cases" entry
BINNINGS = [
    ("v1_b1", ["v1"], 1),
    ("v1_b10", ["v1"], 10),
    ("v3_b100", ["v3"], 100),
    ("v12_b6", ["v1", "v2"], 6),
    ("v12_edges", ["v1", "v2"], {"v1": [0.0, 2.5, 5.0, 7.5, 10.0], "v2": [-1.0, -1.0 / 3.0, 1.0 / 3.0, 1.0]}),
    ("v123_435", ["v1", "v2", "v3"], {"v1": [0.0, 2.5, 5.0, 7.5, 10.0], "v2": [-1.0, -1.0 / 3.0, 1.0 / 3.0, 1.0],
                                      "v3": [0.0, 6.0, 12.0, 18.0, 24.0, 30.0]}),
]
APPLY_PLANE = {"v1": "a1", "v2": "a2", "v3": "a3"}
# apply cases on the 61 x 83 inputs: (binning, dtype, bin_apply_method, min_count)
APPLIES = [(b, "float32", m, mc) for b in ("v1_b10", "v12_b6", "v123_435") for (m, mc) in (("linear", 0), ("linear", 5), ("per_bin", 0))]
APPLIES += [(b, "float32", m, 0) for b in ("v1_b1", "v3_b100", "v12_edges") for m in ("linear", "per_bin")]
APPLIES += [("v3_b100", "float32", "linear", 5)]   # (bins of 1 to 4 pixels at the thin end of v3: the count filter bites)
APPLIES += [("v1_b10", "float64", "linear", 0), ("v1_b10", "float64", "per_bin", 0), ("v12_b6", "float64", "linear", 0),
            ("v123_435", "float64", "per_bin", 0)]
WITH_APPLIED = [("v1_b10", "float32", "linear", 0), ("v12_b6", "float32", "per_bin", 0), ("v1_b10", "float64", "linear", 0)]


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


def valid_mask(case: dict, names: list) -> np.ndarray:
    valid = case["inlier"] & np.isfinite(case["ref"]) & np.isfinite(case["tba"])
    for n in names:
        valid &= np.isfinite(case[n])
    return valid


def frame_columns(df, names: list, stat: str = "nanmedian") -> dict:
    """The DataFrame as arrays: nd, the statistic, count, and left / right ends of every variable's interval (NaN: no interval)."""
    import pandas as pd

    out = {"nd": df["nd"].values.astype(np.int64), stat: df[stat].values.astype(np.float64), "count": df["count"].values.astype(np.float64)}
    for n in names:
        cells = df[n].values
        out[n + "_left"] = np.array([c.left if isinstance(c, pd.Interval) else np.nan for c in cells], dtype=np.float64)
        out[n + "_right"] = np.array([c.right if isinstance(c, pd.Interval) else np.nan for c in cells], dtype=np.float64)
    return out


def main() -> None:
    import _refimport

    _refimport.load()
    from xdem_amd import synth

    bc = importlib.import_module("xdem.coreg.biascorr")
    rec: dict = {}
    fitted = {}
    for (H, W) in ((61, 83), (129, 193)):
        for dtype in ("float32", "float64"):
            case = synth.bias_case(H, W, np.dtype(dtype))
            for name, names, bins in BINNINGS:
                valid = valid_mask(case, names)
                dh = case["ref"][valid] - case["tba"][valid]
                for method in ("linear", "per_bin"):
                    b = bc.BiasCorr(fit_or_bin="bin", bin_sizes=bins, bin_statistic=np.nanmedian, bin_apply_method=method, bias_var_names=names)
                    b._bin_or_and_fit_nd(values=dh, bias_vars={n: case[n][valid] for n in names})
                    fitted[(name, H, dtype, method)] = b
                df = b.meta["outputs"]["fitorbin"]["bin_dataframe"]
                for k, v in frame_columns(df, names).items():
                    rec[f"df|{H}x{W}|{dtype}|{name}|{k}"] = v
    H, W = 61, 83
    for name, dtype, method, mc in APPLIES:
        case = synth.bias_case(H, W, np.dtype(dtype))
        names = dict((b[0], b[1]) for b in BINNINGS)[name]
        b = fitted[(name, H, dtype, method)]
        planes = {n: case[APPLY_PLANE[n]] for n in names}
        kw = {"min_count": mc} if method == "linear" else {}
        corr, _ = b._apply_rst(elev=np.zeros((H, W)), transform=None, crs=None, bias_vars=planes, **kw)
        rec[f"corr|{dtype}|{name}|{method}|{mc}"] = np.asarray(corr, dtype=np.float64)
        if (name, dtype, method, mc) in WITH_APPLIED:
            applied, _ = b._apply_rst(elev=case["tba"], transform=None, crs=None, bias_vars=planes, **kw)
            rec[f"applied|{dtype}|{name}|{method}|{mc}"] = np.asarray(applied).astype(dtype)   # (the cast of base.py:491)

    # the named workflows on a binned table (bin_and_fit), float32 inputs
    case = synth.bias_case(H, W, np.float32)
    from xdem_amd.bincorr import rotated_x

    angle_plane = rotated_x((H, W), (5.0, 5.0), 20.0)
    valid = valid_mask(case, ["v1"])
    dh = case["ref"][valid] - case["tba"][valid]
    import pandas as pd

    for tag, func, var, plane_fit, plane_apply, bins, kwargs in (
            ("poly", "norder_polynomial", "v1", case["v1"], case["a1"], 30, {}),
            ("sumsin", "nfreq_sumsin", "angle", angle_plane, angle_plane, 40, {"random_state": 42, "niter": 3})):
        b = bc.BiasCorr(fit_or_bin="bin_and_fit", fit_func=func, bin_sizes=bins, bin_statistic=np.nanmedian, bias_var_names=[var])
        # (sumsin: a clean along-track sine -- on the noisy dh the reference's basinhopping steps out of its own bounds and SciPy raises)
        values = dh if tag == "poly" else 3.0 * np.sin(2 * np.pi / 200.0 * plane_fit[valid] + 1.0) + 0.05 * (synth._hash01(int(valid.sum()), 5) - 0.5)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            b._bin_or_and_fit_nd(values=values, bias_vars={var: plane_fit[valid]}, **kwargs)
        # (upstream keeps only the fit's results for bin_and_fit: the table the optimiser saw is formed again here)
        sp = importlib.import_module("xdem.spatialstats")
        df = sp.nd_binning(values=values, list_var=[plane_fit[valid]], list_var_names=[var], list_var_bins=bins, statistics=(np.nanmedian, "count"))
        df_nd = df[df.nd == 1]
        x, y = pd.IntervalIndex(df_nd[var]).mid.values, df_nd["nanmedian"].values
        ok = np.isfinite(x) & np.isfinite(y)
        rec[f"{tag}|x"], rec[f"{tag}|y"] = x[ok], y[ok]
        rec[f"{tag}|fit_params"] = np.asarray(b.meta["outputs"]["fitorbin"]["fit_params"], dtype=np.float64)
        rec[f"{tag}|order"] = np.int64(list(b.meta["outputs"]["specific"].values())[0])
        corr, _ = b._apply_rst(elev=np.zeros((H, W)), transform=None, crs=None, bias_vars={var: plane_apply})
        rec[f"{tag}|corr"] = np.asarray(corr, dtype=np.float64).reshape(H, W)
        print(tag, rec[f"{tag}|fit_params"], rec[f"{tag}|order"])
    out = os.path.join(GOLDEN, "bincorr_golden.npz")
    np.savez_compressed(out, **rec)
    print(out, os.path.getsize(out), "bytes")

    # messages
    errors = {}

    def message(key, fn):
        try:
            fn()
            errors[key] = None
        except Exception as e:  # noqa: BLE001
            errors[key] = {"type": type(e).__name__, "message": str(e)}

    message("fit_or_bin", lambda: bc.BiasCorr(fit_or_bin=True))
    message("fit_func", lambda: bc.BiasCorr(fit_func="yay"))
    message("fit_optimizer", lambda: bc.BiasCorr(fit_optimizer=3))
    message("bin_sizes", lambda: bc.BiasCorr(fit_or_bin="bin", bin_sizes={"a": 1.5}))
    message("bin_statistic", lambda: bc.BiasCorr(fit_or_bin="bin", bin_statistic="count"))
    message("bin_apply_method", lambda: bc.BiasCorr(fit_or_bin="bin", bin_apply_method=1))
    case = synth.bias_case(61, 83, np.float32)
    valid = valid_mask(case, ["v1", "v2"])
    dh = case["ref"][valid] - case["tba"][valid]
    b = bc.BiasCorr(fit_or_bin="bin", bin_sizes={"v1": 4, "v2": 3}, bias_var_names=["v1", "v2"])
    message("integer_dict_two_variables", lambda: b._bin_or_and_fit_nd(values=dh, bias_vars={"v1": case["v1"][valid], "v2": case["v2"][valid]}))
    b1 = bc.BiasCorr(fit_or_bin="bin", bias_var_names=["v1"])
    message("wrong_number", lambda: b1._bin_or_and_fit_nd(values=dh, bias_vars={"v1": case["v1"][valid], "v2": case["v2"][valid]}))
    message("wrong_keys", lambda: b1._bin_or_and_fit_nd(values=dh, bias_vars={"v2": case["v2"][valid]}))
    message("fit_none", lambda: b1._bin_or_and_fit_nd(values=dh, bias_vars=None))
    b1._bin_or_and_fit_nd(values=dh, bias_vars={"v1": case["v1"][valid]})
    message("apply_none", lambda: b1._apply_rst(elev=case["tba"], transform=None, crs=None, bias_vars=None))
    message("apply_keys", lambda: b1._apply_rst(elev=case["tba"], transform=None, crs=None, bias_vars={"v2": case["v2"]}))
    with open(os.path.join(GOLDEN, "bincorr_errors.json"), "w") as f:
        json.dump(errors, f, indent=1)
        f.write("\n")

    sig = {"coreg": {"BiasCorr.__init__": _record(bc.BiasCorr.__init__), "DirectionalBias.__init__": _record(bc.DirectionalBias.__init__),
                     "TerrainBias.__init__": _record(bc.TerrainBias.__init__)}}
    with open(os.path.join(GOLDEN, "signatures_bincorr.json"), "w") as f:
        json.dump(sig, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
