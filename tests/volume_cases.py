"""The cases of the xdem_amd.volume fixtures (tools/gen_golden_volume.py), run on a given ``volume`` module -- the device's, or the
NumPy restatement's (volume_oracle.patched) -- and compared with a fixture: shared by test_volume_host.py and test_volume_gpu.py."""
from __future__ import annotations

import os
import warnings

import numpy as np

from xdem_amd import synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SHAPES = ((61, 83), (129, 193))
DTYPES = ("float32", "float64")
CUSTOM_EDGES = np.arange(900.0, 1800.0, 100.0)
PIXEL_SIZE = 30.0
COUNT_THRESHOLD = 40

_golden: dict = {}
_cases: dict = {}


def golden(H: int, W: int, dtype: str) -> dict:
    key = (H, W, dtype)
    if key not in _golden:
        with np.load(os.path.join(GOLDEN, f"volume_{H}x{W}_{dtype}.npz")) as z:
            _golden[key] = {k: z[k] for k in z.files}
    return _golden[key]


def case(H: int, W: int, dtype: str) -> dict:
    """synth.volume_case, built once per shape and dtype and never written to."""
    key = (H, W, dtype)
    if key not in _cases:
        c = synth.volume_case(H, W, np.dtype(dtype))
        for v in c.values():
            v.setflags(write=False)
        _cases[key] = c
    return _cases[key]


def binning_cases(c: dict) -> dict:
    ref = c["ref_voids"]
    return {"fixed": (50.0, "fixed"), "count": (12, "count"), "quantile": (8, "quantile"), "custom": (CUSTOM_EDGES, "custom"),
            "array": (np.linspace(float(np.nanmin(ref)), float(np.nanmax(ref)), 12), "fixed")}


def frame_columns(prefix: str, df, out: dict) -> None:
    out[prefix + "_left"] = np.asarray(df.index.left)
    out[prefix + "_right"] = np.asarray(df.index.right)
    for col in df.columns:
        out[prefix + "_" + col.replace("-", "_")] = np.asarray(df[col].values)


def to_host(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def run_binning(vol, c: dict, put=lambda a: a) -> dict:
    out: dict = {}
    for name, (bins, kind) in binning_cases(c).items():
        frame_columns("bin_" + name, vol.hypsometric_binning(put(c["ddem"]), put(c["ref_voids"]), bins=bins, kind=kind), out)
    return out


def run_tables(vol, fixed) -> dict:
    out: dict = {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        frame_columns("interp", vol.interpolate_hypsometric_bins(fixed), out)
        frame_columns("interp_ct", vol.interpolate_hypsometric_bins(fixed, count_threshold=COUNT_THRESHOLD), out)
        frame_columns("poly", vol.fit_hypsometric_bins_poly(fixed), out)
        frame_columns("poly_ct", vol.fit_hypsometric_bins_poly(fixed, count_threshold=COUNT_THRESHOLD, iterations=3), out)
    return out


def fixed_frame(g: dict):
    """The recorded "fixed" DataFrame of hypsometric_binning, rebuilt from its columns."""
    import pandas as pd

    return pd.DataFrame(index=pd.IntervalIndex.from_arrays(g["bin_fixed_left"], g["bin_fixed_right"]),
                        data={"value": g["bin_fixed_value"], "count": g["bin_fixed_count"]})


def run_area(vol, c: dict, g: dict, put=lambda a: a) -> dict:
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        filled = vol.interpolate_hypsometric_bins(fixed_frame(g), method="linear")
    return {"area_" + t: np.asarray(vol.calculate_hypsometry_area(filled, put(c["ref"]), PIXEL_SIZE, timeframe=t).values)
            for t in ("reference", "nonreference", "mean")}


def run_hypso_interp(vol, c: dict, put=lambda a: a) -> dict:
    hi = vol.hypsometric_interpolation(put(c["ddem"]), put(c["ref_voids"]), put(c["mask"]))
    data = to_host(hi.data if isinstance(hi, np.ma.MaskedArray) else hi)
    mask = np.ma.getmaskarray(hi) if isinstance(hi, np.ma.MaskedArray) else ~np.isfinite(data)
    return {"hypso_interp_data": data, "hypso_interp_mask": mask}


def run_signal(vol, c: dict, put=lambda a: a) -> dict:
    out: dict = {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        frame_columns("signal", vol.get_regional_hypsometric_signal(put(c["ddem"]), put(c["ref"]), put(c["labels"])), out)
    return out


def signal_frame(g: dict):
    import pandas as pd

    cols = ("w_mean", "median", "std", "sigma-1-lower", "sigma-1-upper", "sigma-2-lower", "sigma-2-upper", "count")
    return pd.DataFrame(index=pd.IntervalIndex.from_arrays(g["signal_left"], g["signal_right"]),
                        data={col: g["signal_" + col.replace("-", "_")] for col in cols})


def run_regional(vol, c: dict, g: dict, put=lambda a: a) -> dict:
    """norm_regional_hypsometric_interpolation (both forms) and its per-glacier records, fed the RECORDED regional signal, so that
    this comparison does not hang on the signal's own."""
    out: dict = {}
    sig = signal_frame(g)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        for name, idealized in (("filled", False), ("idealized", True)):
            out["regional_" + name] = to_host(vol.norm_regional_hypsometric_interpolation(
                put(c["ddem"]), put(c["ref"]), put(c["labels"]), regional_signal=sig, idealized_ddem=idealized))
        with vol.HypsoPlan(put(c["ddem"]), put(c["ref"]), labels=put(c["labels"])) as plan:
            records = vol.regional_glacier_models(plan, plan.label_stats(), sig, 0.1, 0.33)
    out["glacier_ids"] = np.asarray([r["id"] for r in records], dtype=np.int64)
    out["glacier_skipped"] = np.asarray([r["skipped"] for r in records], dtype=bool)
    for r in records:
        for key in ("value", "count", "std", "coeffs", "x", "y"):
            if key in r:
                out[f"glacier_{r['id']}_{key}"] = np.asarray(r[key])
    return out


def assert_same_bits(got: dict, g: dict, keys=None) -> None:
    for k in (keys if keys is not None else got):
        a, b = np.asarray(got[k]), np.asarray(g[k])
        assert a.dtype == b.dtype, f"{k}: dtype {a.dtype}, recorded {b.dtype}"
        assert a.shape == b.shape, f"{k}: shape {a.shape}, recorded {b.shape}"
        assert np.array_equal(a, b, equal_nan=True), f"{k}: {np.count_nonzero(~((a == b) | (np.isnan(a) & np.isnan(b))))} of {a.size} entries differ"


def regional_deviations(got: dict, g: dict, c: dict) -> tuple[float, float]:
    """Asserts everything of the regional interpolation that is exact (every glacier's skip decision, counts, medians, the model's
    abscissae, the pixels no model touches, the NaN pattern) and returns the two measured deviations: the largest |std - recorded| /
    recorded over all bins of all glaciers, and the largest deviation of a model quantity -- coefficients, model table, filled
    pixels -- relative to its glacier's largest recorded |model value|."""
    assert_same_bits(got, g, ["glacier_ids", "glacier_skipped"])
    assert sorted(k for k in got if k.startswith("glacier_")) == sorted(k for k in g if k.startswith("glacier_")), "glacier records differ"
    std_dev, model_dev = 0.0, 0.0
    labels = c["labels"].reshape(g["regional_filled"].shape)   # (the functions squeeze, as get_array_and_mask does)
    scale = np.zeros(labels.shape)
    for i, skipped in zip(g["glacier_ids"], g["glacier_skipped"]):
        if f"glacier_{i}_value" not in g:
            continue
        assert_same_bits(got, g, [f"glacier_{i}_value", f"glacier_{i}_count"])
        s, s0 = got[f"glacier_{i}_std"], g[f"glacier_{i}_std"]
        assert s.dtype == s0.dtype and np.array_equal(np.isnan(s), np.isnan(s0)) and np.array_equal(s == 0, s0 == 0), f"glacier {i}: std pattern"
        pos = s0 > 0
        if pos.any():
            std_dev = max(std_dev, float(np.max(np.abs(s[pos].astype(np.float64) - s0[pos]) / s0[pos])))
        if skipped:
            continue
        assert_same_bits(got, g, [f"glacier_{i}_x"])
        top = float(np.max(np.abs(g[f"glacier_{i}_y"])))
        scale[labels == i] = top
        for key in ("coeffs", "y"):
            model_dev = max(model_dev, float(np.max(np.abs(got[f"glacier_{i}_{key}"] - g[f"glacier_{i}_{key}"])) / top))
    for name in ("regional_filled", "regional_idealized"):
        a, b = got[name], g[name]
        assert a.dtype == b.dtype and a.shape == b.shape, name
        assert np.array_equal(np.isnan(a), np.isnan(b)), f"{name}: NaN pattern"
        untouched = scale == 0
        assert np.array_equal(a[untouched], b[untouched], equal_nan=True), f"{name}: pixels outside the fitted glaciers"
        fin = np.isfinite(b) & ~untouched
        assert np.array_equal(a[~fin & ~untouched], b[~fin & ~untouched], equal_nan=True), f"{name}: non-finite pixels"
        if fin.any():
            model_dev = max(model_dev, float(np.max(np.abs(a[fin].astype(np.float64) - b[fin]) / scale[fin])))
    return std_dev, model_dev


# The largest deviations from the fixtures measured on an MI355X, per dtype: (per-bin standard deviation relative to the bin's
# standard deviation, model quantities relative to the glacier's largest model value).  Upstream sums float32 pairwise in sample
# order; the device sums float64 over the sorted bin.  The bars of the tests are 4 x these figures.
MEASURED = {"float32": (1.2e-7, 1.5e-6), "float64": (2.2e-16, 9.6e-8)}
