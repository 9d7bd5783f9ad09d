"""The cases of the dDEM / DEMCollection fixtures (tools/gen_golden_demcollection.py) and what the tests need to compare a collection
with them: shared by test_demcollection_host.py and test_demstack_gpu.py."""
from __future__ import annotations

import math
import os
import warnings

import numpy as np

import volume_cases as vc

GOLDEN = vc.GOLDEN
SHAPES = vc.SHAPES
DTYPES = vc.DTYPES
YEARS = (2000, 2005, 2010, 2015)
REFERENCE = 1                       # the DEM of 2005
FACTORS = (1.0, None, -1.0 / 3.0, 2.0)    # dem_t = ref - factor * ddem, rounded to the dtype (the third: full mantissas); None: the reference itself
RES = (30.0, 30.0)
TRANSFORM = (30.0, 0.0, 500000.0, 0.0, -30.0, 7000000.0)
VARIANTS = ("raw_full", "raw_mask", "filled_full", "filled_mask")   # dDEMs with their voids / filled inside the mask; every pixel / the mask

_stacks: dict = {}
_golden: dict = {}


def stamps(years=YEARS) -> list:
    return [np.datetime64(f"{y}-01-01") for y in years]


def stack(H: int, W: int, dtype: str) -> dict:
    """Four DEMs made from volume_cases.case: the reference (with voids) and three DEMs that differ from it by a multiple of the case's
    dDEM, whose +-inf become voids (upstream's np.nanmean takes an infinity along; the series here are over finite values).  Built
    once, never written to."""
    key = (H, W, dtype)
    if key not in _stacks:
        c = vc.case(H, W, dtype)
        dt = np.dtype(dtype)
        ref = c["ref_voids"]
        dd = np.where(np.isfinite(c["ddem"]), c["ddem"], np.nan).astype(dt)
        dems = [ref if f is None else (ref - dt.type(f) * dd).astype(dt) for f in FACTORS]
        for d in dems:
            d.setflags(write=False)
        _stacks[key] = {"dems": dems, "mask": c["mask"], "ref": ref}
    return _stacks[key]


def golden() -> dict:
    if not _golden:
        with np.load(os.path.join(GOLDEN, "demcollection_golden.npz")) as z:
            _golden.update({k: z[k] for k in z.files})
    return _golden


def series_columns(prefix: str, dh, dv, cum_dh, cum_dv, out: dict) -> None:
    """A dh frame, the dv series and the two cumulative series as arrays: interval and timestamp indexes as int64 nanoseconds."""
    out[prefix + "_left"] = np.asarray([i.left.value for i in dh.index], dtype=np.int64)
    out[prefix + "_right"] = np.asarray([i.right.value for i in dh.index], dtype=np.int64)
    out[prefix + "_dh"] = np.asarray(dh["dh"].values, dtype=np.float64)
    out[prefix + "_area"] = np.asarray(dh["area"].values, dtype=np.float64)
    out[prefix + "_dv"] = np.asarray(dv.values, dtype=np.float64)
    for name, s in (("cumdh", cum_dh), ("cumdv", cum_dv)):
        out[f"{prefix}_{name}_index"] = np.asarray(s.index.values.astype("datetime64[ns]").astype(np.int64))
        out[f"{prefix}_{name}"] = np.asarray(s.values, dtype=np.float64)


# ---- bounds ------------------------------------------------------------------------------------------------------------------------------
def moments(values: np.ndarray) -> tuple:
    """(count, exactly rounded mean, mean |x|) of the finite values."""
    v = np.asarray(values, dtype=np.float64)
    v = v[np.isfinite(v)]
    n = v.shape[0]
    if n == 0:
        return 0, math.nan, math.nan
    return n, math.fsum(v) / n, math.fsum(np.abs(v)) / n


def any_order_bound(n: int, mean: float, mean_abs: float, u: float) -> float:
    """|computed mean - exact mean| for a sum of n terms added in ANY order with unit roundoff u, then one division:
    (n - 1) u mean|x| + u |mean| (Higham, Accuracy and Stability of Numerical Algorithms, 4.2: |E_n| <= (n - 1) u sum|x_i|
    to first order, whatever the order; the division adds a relative u)."""
    return (n - 1) * u * mean_abs + u * abs(mean)


U = {"float32": 2.0 ** -24, "float64": 2.0 ** -53}

# The largest |dh - recorded dh| / mean|x| over every recorded series, per dtype: the collection's float64 fixed-order mean against the
# reference's np.nanmean in the raster's own dtype (pairwise).  (NumPy restatement on the CPU, MI355X with ROCm 7.2.0), rounded up to
# two digits: 1.110e-07 and 1.110e-07 for float32 (float32 terms sum exactly in float64, so both are the reference's own float32
# rounding), 2.364e-16 and 2.586e-16 for float64.  The bar of the tests is min(any_order_bound with the dtype's unit roundoff,
# 4 x the larger of the two x mean|x|).
MEASURED = {"float32": (1.2e-7, 1.2e-7), "float64": (2.4e-16, 2.6e-16)}


def recorded_bar(dtype: str, n: int, mean: float, mean_abs: float) -> float:
    cap = any_order_bound(n, mean, mean_abs, U[dtype])
    figures = [f for f in MEASURED[dtype] if f is not None]
    return min(cap, 4.0 * max(figures) * mean_abs) if figures else cap


# ---- a collection's series against the recorded ones -----------------------------------------------------------------------------------------
def series_of(col, **kw) -> dict:
    out: dict = {}
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        dh = col.get_dh_series(**kw)
    texts = [str(w.message) for w in caught]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        series_columns("s", dh, col.get_dv_series(nans_ok=True, **kw), col.get_cumulative_series(kind="dh", nans_ok=True, **kw),
                          col.get_cumulative_series(kind="dv", nans_ok=True, **kw), out)
    return {"texts": texts, **out}


def assert_series(got: dict, g: dict, prefix: str, dtype: str, sources: list, mask: np.ndarray, texts: list) -> float:
    """Indexes, areas and warnings exact; every dh within its bar of the reference's np.nanmean; dv and the cumulative series within the
    bars their dh imply.  Returns the largest |dh - recorded| / mean|x|."""
    for k in ("left", "right", "cumdh_index", "cumdv_index"):
        assert np.array_equal(got["s_" + k], g[f"{prefix}_{k}"]) and got["s_" + k].dtype == np.int64, k
    assert np.array_equal(got["s_area"], g[prefix + "_area"])
    assert got["texts"] == texts
    worst, bars = 0.0, []
    for j, src in enumerate(sources):
        n, mean, mean_abs = moments(src[mask])
        dev = abs(got["s_dh"][j] - g[prefix + "_dh"][j])
        bar = recorded_bar(dtype, n, mean, mean_abs)
        print(f"{prefix} dDEM {j}: n {n} dh {got['s_dh'][j]!r} recorded {g[prefix + '_dh'][j]!r} |dev| {dev:.3e} / mean|x| {dev / mean_abs:.3e} bar {bar:.3e}")
        assert dev <= bar, (prefix, j, dev, bar)
        # against the exactly rounded mean: the any-order bound in float64 (the restatement sums with math.fsum: one rounding)
        assert abs(got["s_dh"][j] - mean) <= any_order_bound(n, mean, mean_abs, 2.0 ** -53), (prefix, j)
        worst = max(worst, dev / mean_abs)
        bars.append(bar)
    # dv = area * dh: the dh's bar times the area, and one rounding of the product on either side.  The cumulative series: -value per
    # timestamp minus the first entry: two of the bars, and one rounding of the difference on either side.
    area, eps = g[prefix + "_area"], 2.0 ** -52
    assert np.all(np.abs(got["s_dv"] - g[prefix + "_dv"]) <= np.array(bars) * area + eps * np.abs(g[prefix + "_dv"]))
    for kind, scale in (("cumdh", 1.0), ("cumdv", float(area.max()))):
        want = g[f"{prefix}_{kind}"]
        assert np.all(np.abs(got["s_" + kind] - want) <= 2 * max(bars) * scale + 2 * eps * np.abs(want).max()), kind
    return worst
