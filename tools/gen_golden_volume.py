"""Golden vectors for xdem_amd.volume, recorded from the REFERENCE's own functions in xdem/volume.py (needs the reference source
tree, so it runs only where that tree is present; the fixtures it writes are what the tests read).

Inputs: ``xdem_amd.synth.volume_case(H, W, dtype)`` for 61 x 83 and 129 x 193, float32 and float64 -- built from exactly rounded
arithmetic on hashed integers, so the tests rebuild them bit for bit and nothing of them is stored.

The reference is imported through oracle/_refimport.py as it stands; this tool adds the one shim volume.py needs on top,
``geoutils.raster.array.get_mask_from_array`` (masked or non-finite), and sets ``xdem.volume`` on the package object, because
``hypsometric_interpolation`` calls ``xdem.volume.hypsometric_binning``.  rasterio is a stub: ``idw_interpolation`` and
``local_hypsometric_interpolation`` cannot run here and nothing of them is recorded.

61 x 83 is also recorded for the two mixed pairs -- the dDEM of the case of one dtype with ``ref`` / ``ref_voids`` of the case of the other,
labels and mask shared -- as tests/golden/volume_61x83_<ddem dtype>_<ref dtype>.npz.

Recorded per shape and dtype (tests/golden/volume_<H>x<W>_<dtype>.npz):
  * hypsometric_binning for kind "fixed", "count", "quantile", "custom" and a plain edge array (on the reference with voids): the
    value and count columns and the interval ends;
  * interpolate_hypsometric_bins and fit_hypsometric_bins_poly on the "fixed" table, with and without count_threshold;
  * calculate_hypsometry_area for the three timeframes;
  * hypsometric_interpolation: data and mask;
  * get_regional_hypsometric_signal: every column;
  * norm_regional_hypsometric_interpolation, idealized_ddem False and True, and per glacier what it decided and fitted (a restatement
    of the loop body of volume.py:715-797 around the reference's own hypsometric_binning, since the function keeps none of it):
    the bins' value, count and std, the skip decision, the coefficients and the model table.
No skip decision may lie within 1e-3 of its threshold: asserted below.

Also: the signatures (tests/golden/signatures_volume.json) and the messages of upstream's errors, assertions and warnings
(tests/golden/volume_errors.json).

    python tools/gen_golden_volume.py
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
SHAPES = ((61, 83), (129, 193))
MIXED_SHAPE = (61, 83)
MIXED_PAIRS = (("float32", "float64"), ("float64", "float32"))   # (dDEM, reference)
FUNCTIONS = ("hypsometric_binning", "interpolate_hypsometric_bins", "fit_hypsometric_bins_poly", "calculate_hypsometry_area",
             "hypsometric_interpolation", "get_regional_hypsometric_signal", "norm_regional_hypsometric_interpolation")
CUSTOM_EDGES = np.arange(900.0, 1800.0, 100.0)
PIXEL_SIZE = 30.0
COUNT_THRESHOLD = 40


def load_reference():
    import _refimport

    _refimport.install()
    import geoutils.raster.array

    def get_mask_from_array(array):
        """geoutils.raster.array.get_mask_from_array: masked or non-finite."""
        invalid = ~np.isfinite(np.asarray(np.ma.getdata(array), dtype=np.float64))
        return invalid | np.ma.getmaskarray(array)

    geoutils.raster.array.get_mask_from_array = get_mask_from_array
    volume = importlib.import_module("xdem.volume")
    sys.modules["xdem"].volume = volume
    return volume


def _literal(v):
    if v is inspect.Parameter.empty:
        return "<required>"
    if v is None or isinstance(v, (bool, int, float, str)):
        return v
    return getattr(v, "__name__", repr(v))


def signature_of(fn) -> list:
    return [{"name": n, "kind": p.kind.name, "default": _literal(p.default)} for n, p in inspect.signature(fn).parameters.items()]


def frame_columns(prefix: str, df, out: dict) -> None:
    out[prefix + "_left"] = np.asarray(df.index.left)
    out[prefix + "_right"] = np.asarray(df.index.right)
    for c in df.columns:
        out[prefix + "_" + c.replace("-", "_")] = np.asarray(df[c].values)


def binning_cases(case: dict) -> dict:
    """name -> (bins, kind) of the hypsometric_binning fixtures (shared with the tests)."""
    ref = case["ref_voids"]
    return {"fixed": (50.0, "fixed"), "count": (12, "count"), "quantile": (8, "quantile"), "custom": (CUSTOM_EDGES, "custom"),
            "array": (np.linspace(float(np.nanmin(ref)), float(np.nanmax(ref)), 12), "fixed")}


def glacier_records(volume, ddem, ref, index_map, regional_signal, min_coverage=0.1, min_elevation_range=0.33):
    """What norm_regional_hypsometric_interpolation decides and fits per glacier (the function itself keeps none of it): the steps of
    its loop body (volume.py:715-797) around the reference's own hypsometric_binning.  Asserts that no decision sits on its threshold.
    The filled rasters recorded next to these come from the reference's function itself; the fill-pass test ties the two together."""
    import pandas as pd
    import scipy.optimize

    voids = ~np.isfinite(ddem)
    records = []
    for label in np.unique(index_map):
        if label == 0:
            continue
        outline = index_map == label
        valid = outline & ~voids
        coverage = np.count_nonzero(valid) / np.count_nonzero(outline)
        assert abs(coverage - min_coverage) > 1e-3 and abs(coverage - 0.05) > 1e-3, f"glacier {label}: coverage {coverage} on a threshold"
        rec = {"id": int(label), "skipped": True}
        records.append(rec)
        if coverage < min_coverage:
            continue
        low, high = ref[outline].min(), ref[outline].max()
        scaled = regional_signal["w_mean"].copy()
        mids = scaled.index.mid
        mids *= high - low
        mids += low
        width = mids[1] - mids[0]
        scaled.index = pd.IntervalIndex.from_arrays(left=mids - width / 2, right=mids + width / 2)
        edges = np.r_[[scaled.index.left[0]], scaled.index.right]
        medians = volume.hypsometric_binning(ddem=ddem[valid], ref_dem=ref[valid], bins=edges, kind="custom")
        spreads = volume.hypsometric_binning(ddem=ddem[valid], ref_dem=ref[valid], bins=edges, kind="custom", aggregation_function=np.nanstd)
        rec.update(value=medians["value"].values, count=medians["count"].values, std=spreads["value"].values)
        filled = np.isfinite(medians["value"])
        with np.errstate(invalid="ignore", divide="ignore"):
            covered = np.sum(filled[filled].index.length) / np.sum(medians.index.length)
        assert not abs(covered - min_elevation_range) <= 1e-3, f"glacier {label}: elevation range ratio {covered} on the threshold"
        if covered < min_elevation_range or np.count_nonzero(filled) < 2:
            continue
        sigma = spreads["value"].values[filled] / np.sqrt(medians["count"].values[filled])
        sigma[sigma == 0.0] = 1e-8
        with warnings.catch_warnings():
            warnings.filterwarnings("ignore", message="covariance")
            coeffs = scipy.optimize.curve_fit(f=lambda x, a, b: a * x + b, xdata=scaled.values[filled], ydata=medians["value"].values[filled],
                                              p0=[1, 0], sigma=sigma)[0]
        rec.update(skipped=False, coeffs=coeffs, x=np.asarray(scaled.index.mid, dtype=np.float64), y=np.poly1d(coeffs)(scaled.values))
    return records


def mixed_case(H: int, W: int, ddem_dtype, ref_dtype) -> dict:
    """The dDEM of the case of one dtype with the reference rasters of the case of the other; labels and mask are the same in both."""
    from xdem_amd import synth

    case = dict(synth.volume_case(H, W, np.dtype(ddem_dtype)))
    if np.dtype(ref_dtype) != np.dtype(ddem_dtype):
        other = synth.volume_case(H, W, np.dtype(ref_dtype))
        assert np.array_equal(other["labels"], case["labels"]) and np.array_equal(other["mask"], case["mask"])
        case["ref"], case["ref_voids"] = other["ref"], other["ref_voids"]
    return case


def record_case(volume, H: int, W: int, dtype, ref_dtype=None) -> dict:
    case = mixed_case(H, W, dtype, dtype if ref_dtype is None else ref_dtype)
    ddem, ref, ref_voids, labels, mask = (case[k] for k in ("ddem", "ref", "ref_voids", "labels", "mask"))
    out: dict = {}
    frames = {}
    for name, (bins, kind) in binning_cases(case).items():
        frames[name] = volume.hypsometric_binning(ddem, ref_voids, bins=bins, kind=kind)
        frame_columns("bin_" + name, frames[name], out)
    fixed = frames["fixed"]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        frame_columns("interp", volume.interpolate_hypsometric_bins(fixed), out)
        frame_columns("interp_ct", volume.interpolate_hypsometric_bins(fixed, count_threshold=COUNT_THRESHOLD), out)
        frame_columns("poly", volume.fit_hypsometric_bins_poly(fixed), out)
        frame_columns("poly_ct", volume.fit_hypsometric_bins_poly(fixed, count_threshold=COUNT_THRESHOLD, iterations=3), out)
        filled_bins = volume.interpolate_hypsometric_bins(fixed, method="linear")
    assert not np.any(np.isnan(filled_bins["value"].values))
    for timeframe in ("reference", "nonreference", "mean"):
        out["area_" + timeframe] = np.asarray(volume.calculate_hypsometry_area(filled_bins, ref, PIXEL_SIZE, timeframe=timeframe).values)
    hi = volume.hypsometric_interpolation(ddem, ref_voids, mask)
    out["hypso_interp_data"], out["hypso_interp_mask"] = np.asarray(hi.data), np.ma.getmaskarray(hi)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        signal = volume.get_regional_hypsometric_signal(ddem, ref, labels)
        frame_columns("signal", signal, out)
        for name, idealized in (("filled", False), ("idealized", True)):
            out["regional_" + name] = volume.norm_regional_hypsometric_interpolation(ddem, ref, labels, idealized_ddem=idealized)
        records = glacier_records(volume, ddem, ref, labels, signal)
    out["glacier_ids"] = np.asarray([r["id"] for r in records], dtype=np.int64)
    out["glacier_skipped"] = np.asarray([r["skipped"] for r in records], dtype=bool)
    for r in records:
        for key in ("value", "count", "std", "coeffs", "x", "y"):
            if key in r:
                out[f"glacier_{r['id']}_{key}"] = np.asarray(r[key])
    return out


def record_errors(volume) -> dict:
    from xdem_amd import synth

    case = synth.volume_case(61, 83, np.float32)
    ddem, ref, labels = case["ddem"], case["ref"], case["labels"]
    errors = {}

    def catch(name, fn):
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            try:
                fn()
                errors[name] = {"type": None, "message": None}
            except BaseException as e:   # noqa: BLE001 (assertions included)
                errors[name] = {"type": type(e).__name__, "message": str(e)}
            errors[name]["warnings"] = [[w.category.__name__, str(w.message)] for w in caught if issubclass(w.category, UserWarning)]

    fixed = volume.hypsometric_binning(ddem, ref)
    catch("shape_mismatch", lambda: volume.hypsometric_binning(ddem[:, :-1], ref))
    catch("invalid_kind", lambda: volume.hypsometric_binning(ddem, ref, kind="nope"))
    catch("invalid_timeframe", lambda: volume.calculate_hypsometry_area(fixed, ref, 30.0, timeframe="nope"))
    catch("area_ref_nans", lambda: volume.calculate_hypsometry_area(fixed, case["ref_voids"], 30.0))
    catch("area_bins_nans", lambda: volume.calculate_hypsometry_area(fixed, ref, 30.0, timeframe="mean"))
    catch("signal_ref_voids", lambda: volume.get_regional_hypsometric_signal(ddem, case["ref_voids"], labels))
    catch("regional_ref_voids", lambda: volume.norm_regional_hypsometric_interpolation(ddem, case["ref_voids"], labels))
    catch("interp_too_few_bins", lambda: volume.interpolate_hypsometric_bins(fixed.iloc[:3]))
    catch("hypso_interp_empty_mask", lambda: volume.hypsometric_interpolation(ddem, ref, np.zeros(ddem.shape, dtype=bool)))
    return errors


def main() -> None:
    volume = load_reference()
    os.makedirs(GOLDEN, exist_ok=True)
    for H, W in SHAPES:
        for dtype in (np.float32, np.float64):
            out = record_case(volume, H, W, dtype)
            path = os.path.join(GOLDEN, f"volume_{H}x{W}_{np.dtype(dtype).name}.npz")
            np.savez_compressed(path, **out)
            print(path, os.path.getsize(path), "bytes;", int((~out["glacier_skipped"]).sum()), "of", len(out["glacier_ids"]), "glaciers fitted")
    for ddem_dtype, ref_dtype in MIXED_PAIRS:
        out = record_case(volume, *MIXED_SHAPE, ddem_dtype, ref_dtype)
        path = os.path.join(GOLDEN, f"volume_{MIXED_SHAPE[0]}x{MIXED_SHAPE[1]}_{ddem_dtype}_{ref_dtype}.npz")
        np.savez_compressed(path, **out)
        print(path, os.path.getsize(path), "bytes;", int((~out["glacier_skipped"]).sum()), "of", len(out["glacier_ids"]), "glaciers fitted")
    with open(os.path.join(GOLDEN, "signatures_volume.json"), "w") as f:
        json.dump({name: signature_of(getattr(volume, name)) for name in FUNCTIONS}, f, indent=1)
        f.write("\n")
    with open(os.path.join(GOLDEN, "volume_errors.json"), "w") as f:
        json.dump(record_errors(volume), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
