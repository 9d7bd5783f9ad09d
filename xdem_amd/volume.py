"""xdem.volume on the GPU: hypsometric binning of a dDEM and the gap-filling methods built on it (xdem/volume.py).

The raster work runs in csrc/volume.hip, a constant number of passes whatever the number of glaciers: per-label statistics, a
grouping pass with a counting sort into (label, elevation bin) segments, exact medians (and standard deviations) per segment,
and one fused fill pass.  Tables of tens of rows stay in pandas / NumPy / SciPy, written as upstream writes them, so that the
DataFrames come out bit for bit -- including upstream's storing of bin ``i``'s statistic at row ``i - 1`` (volume.py:115-116: the
first bin's result lands in the last row), which everything downstream inherits.

Inputs are host arrays, masked arrays or device tensors; device inputs give device outputs wherever upstream returns an array.
``idw_interpolation`` and ``local_hypsometric_interpolation`` (GDAL's fillnodata) are not part of this module;
the ``dDEM`` / ``DEMCollection`` classes built on it are xdem_amd/ddem.py and xdem_amd/demcollection.py.
"""
from __future__ import annotations

import ctypes
import warnings
from typing import Any, Callable

import numpy as np
import pandas as pd
import scipy.interpolate
import scipy.optimize

from . import _args, _lib
from ._args import code, dp, i32p, i64p, is_tensor, np_dtype, ptr, same_space
from ._args import flat_float as _float_plane  # (under these names tests/volume_oracle.py builds its plan's inputs too)
from ._args import flat_mask as _mask_plane

LABEL_LIMIT = 1 << 20


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
def _labels_plane(x, like):
    """A glacier index map as flat int32 in the memspace of `like`; integral values in [0, 2^20) only."""
    def bad(lo, hi):
        return ValueError(f"glacier_index_map: labels must lie in [0, 2^20 = {LABEL_LIMIT}); found {lo} .. {hi}")

    if is_tensor(x):
        import torch

        x = x.contiguous().reshape(-1)
        if x.is_floating_point():
            if not bool(torch.all(x == torch.floor(x))):
                raise ValueError("glacier_index_map: labels must be integers")
        lo, hi = x.min().item(), x.max().item()
        if lo < 0 or hi >= LABEL_LIMIT:
            raise bad(lo, hi)
        x = x.to(torch.int32)
    else:
        if isinstance(x, np.ma.MaskedArray):
            x = np.where(np.ma.getmaskarray(x), 0, x.data)
        x = np.asarray(x).reshape(-1)
        if x.dtype == bool:
            x = x.astype(np.int32)
        if not np.issubdtype(x.dtype, np.integer):
            if not np.all(x == np.floor(x)):
                raise ValueError("glacier_index_map: labels must be integers")
        lo, hi = x.min(), x.max()
        if lo < 0 or hi >= LABEL_LIMIT:
            raise bad(lo, hi)
        x = np.ascontiguousarray(x.astype(np.int32, copy=False))
    return same_space(x, like)


# ---- the labelled engine ---------------------------------------------------------------------------------------------------------------
class HypsoPlan(_lib._Plan):
    """One (dDEM, reference) pair on the device with its optional label map or mask: ``xdemhip_hypso`` of include/xdemhip.h."""

    _DESTROY = "xdemhip_hypso_destroy"

    def __init__(self, ddem, ref, labels=None, mask=None, ctx: _lib.Context | None = None):
        self.ddem = _float_plane(ddem, "ddem")
        self.ref = same_space(_float_plane(ref, "ref_dem"), self.ddem)
        if self.ddem.shape != self.ref.shape:
            raise ValueError("the dDEM and the reference DEM must have the same number of pixels")
        self.labels = None if labels is None else _labels_plane(labels, self.ddem)
        self.mask = None if mask is None else _mask_plane(mask, self.ddem)
        for extra in (self.labels, self.mask):
            if extra is not None and extra.shape != self.ddem.shape:
                raise ValueError("the label map / mask must have the same number of pixels as the rasters")
        self.n = int(self.ddem.shape[0])
        self.on_device = is_tensor(self.ddem)
        self.ctx = ctx or _lib.default_context(self.ddem.device.index if self.on_device else None)
        self.space = _args.space(self.ddem)
        if self.on_device:
            _args.synchronize_torch(self.ddem)   # (the inputs are complete; the calls return synchronised)
        h = ctypes.c_void_p()
        with self.ctx.call_lock:
            self.ctx.check(self.ctx._L.xdemhip_hypso_create(
                self.ctx.handle, ptr(self.ddem), code(self.ddem), ptr(self.ref), code(self.ref), ptr(self.labels), ptr(self.mask),
                self.n, self.space, ctypes.byref(h)))
        self.handle = h
        self.ctx.adopt(self)

    def label_stats(self) -> dict:
        """Per label that occurs (ascending): pixels, inliers, min / max of the reference over its pixels and over its inliers; and
        the number of pixels with a non-finite reference in the whole raster."""
        cap = max(1, min(self.n, LABEL_LIMIT - 1 if self.labels is not None else 1))
        ids = np.empty(cap, np.int32)
        cnt = np.empty((cap, 2), np.int64)
        ext = np.empty((cap, 4), np.float64)
        found, bad, ref_bad = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
        with self.ctx.call_lock:
            self.ctx.check(self.ctx._L.xdemhip_hypso_label_stats(
                self.handle, cap, i32p(ids), i64p(cnt), dp(ext), ctypes.byref(found), ctypes.byref(bad), ctypes.byref(ref_bad)))
        if bad.value:
            raise ValueError(f"glacier_index_map: {bad.value} labels outside [0, 2^20 = {LABEL_LIMIT})")
        k = int(found.value)
        order = np.argsort(ids[:k], kind="stable")
        return {"ids": ids[:k][order], "pixels": cnt[:k, 0][order], "inliers": cnt[:k, 1][order], "ref_min": ext[:k, 0][order],
                "ref_max": ext[:k, 1][order], "inlier_ref_min": ext[:k, 2][order], "inlier_ref_max": ext[:k, 3][order],
                "ref_invalid": int(ref_bad.value)}

    def segments(self, ids, edges: np.ndarray, want_std: bool = False):
        """(counts, medians, stds | None), each (len(ids), nb): the bins 1 .. nb of np.digitize(ref, edges[r]) per kept label."""
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        edges = np.ascontiguousarray(edges, dtype=np.float64).reshape(len(ids), -1)
        nb = edges.shape[1] - 1
        counts = np.empty((len(ids), nb), np.int64)
        med = np.empty((len(ids), nb), np.float64)
        sd = np.empty((len(ids), nb), np.float64) if want_std else None
        with self.ctx.call_lock:
            self.ctx.check(self.ctx._L.xdemhip_hypso_segments(
                self.handle, len(ids), i32p(ids), nb, dp(edges), int(want_std), i64p(counts), dp(med), dp(sd)))
        return counts, med, sd

    def groups(self) -> np.ndarray:
        """The group (rank * nb + bin - 1, or -1) of every pixel in the last ``segments`` call, on the host."""
        out = np.empty(self.n, np.int32)
        with self.ctx.call_lock:
            self.ctx.check(self.ctx._L.xdemhip_hypso_groups(self.handle, ptr(out), _lib.HOST))
        return out

    def fill(self, mode: int, ids, xs: np.ndarray, ys: np.ndarray, round_to_ref: bool, out_dtype: np.dtype):
        """The fused fill pass: a flat array / tensor of `out_dtype` in the inputs' memspace."""
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        m = np.size(xs) // len(ids) if len(ids) else 0
        xs = np.ascontiguousarray(xs, dtype=np.float64).reshape(len(ids), m)
        ys = np.ascontiguousarray(ys, dtype=np.float64).reshape(len(ids), m)
        out_dtype = np.dtype(out_dtype)
        if self.on_device:
            import torch

            out = torch.empty(self.n, dtype=getattr(torch, out_dtype.name), device=self.ddem.device)
        else:
            out = np.empty(self.n, out_dtype)
        with self.ctx.call_lock:
            self.ctx.check(self.ctx._L.xdemhip_hypso_fill(
                self.handle, int(mode), len(ids), i32p(ids), m, dp(xs), dp(ys), int(round_to_ref), ptr(out), code(out_dtype), self.space))
        return out


def _host(x) -> np.ndarray:
    return x.cpu().numpy() if is_tensor(x) else x


_DEVICE_MEDIANS = (np.median, np.nanmedian)


def _rotated(nb: int, counts: np.ndarray, stat: np.ndarray, dtype: np.dtype):
    """Upstream's loop over the bins (volume.py:101-121): the statistic of bin i + 1 is stored at row i - 1."""
    values = np.full(shape=nb, fill_value=np.nan, dtype=dtype)
    out_counts = np.zeros_like(values, dtype=int)
    filled = counts > 0
    values[filled] = stat[filled]
    out_counts[filled] = counts[filled]
    return np.roll(values, -1), np.roll(out_counts, -1)


def _host_statistic(plan: HypsoPlan, nb: int, rank: int, fn: Callable) -> tuple[np.ndarray, np.ndarray]:
    """`fn` applied per bin on the host, to the finite values of each bin in sample order (the bin numbers come from the device)."""
    groups = plan.groups()
    ddem = _host(plan.ddem)
    stat = np.full(nb, np.nan, dtype=np.float64)
    counts = np.zeros(nb, np.int64)
    for b in range(nb):
        v = ddem[groups == rank * nb + b]
        counts[b] = v.shape[0]
        if v.shape[0]:
            stat[b] = fn(v)
    return counts, stat


def _zbins(kind: str, bins, ref_min, ref_max, ref_valid: Callable[[], np.ndarray]):
    """The bin edges of hypsometric_binning (volume.py:75-92), the expressions as upstream writes them on scalars of the raster's
    dtype (so what NumPy does to float32 scalars -- float32 edges, an increment that vanishes -- happens here too)."""
    if isinstance(bins, np.ndarray):
        return bins
    if kind == "fixed":
        return np.arange(ref_min, ref_max + bins + 1e-6, step=bins)
    if kind == "count":
        return np.linspace(ref_min, ref_max + 1e-6 / bins, num=int(bins + 1))
    if kind == "quantile":
        steps = np.linspace(0, 100, num=int(bins) + 1)
        ref = ref_valid()
        zbins = np.fromiter((np.percentile(ref, step) for step in steps), dtype=float)
        zbins[-1] += 1e-6
        return zbins
    if kind == "custom":
        return bins
    raise ValueError(f"Invalid bin kind: {kind}. Choices: ['fixed', 'count', 'quantile', 'custom'].")


def _binning_frame(zbins, values, counts) -> pd.DataFrame:
    return pd.DataFrame(index=pd.IntervalIndex.from_breaks(zbins), data=np.vstack([values, counts]).T, columns=["value", "count"])



def hypsometric_binning(
    ddem,
    ref_dem,
    bins: float | np.ndarray[Any, np.dtype[np.floating[Any] | np.integer[Any]]] = 50.0,
    kind: str = "fixed",
    aggregation_function: Callable[[np.ndarray], float] = np.median,
) -> pd.DataFrame:
    """One statistic of the dDEM per elevation bin of the reference DEM (``xdem.volume.hypsometric_binning``).

    The bins span the valid pixels of `ref_dem`; non-finite or masked dDEM pixels are left out of the statistic.  `bins` is the bin
    height ("fixed"), the number of bins ("count", "quantile") or the edges ("custom", or any ndarray).  Returns the DataFrame of
    upstream: an IntervalIndex of the edges, columns "value" and "count" -- rows rotated by one as upstream stores them.
    """
    assert tuple(ddem.shape) == tuple(ref_dem.shape)
    with HypsoPlan(ddem, ref_dem) as plan:
        return _binning_of(plan, bins, kind, aggregation_function, over_inliers=False)


def _binning_of(plan: HypsoPlan, bins, kind, aggregation_function, over_inliers: bool) -> pd.DataFrame:
    """hypsometric_binning on the one label of `plan`.  over_inliers: the caller handed upstream only the inlier pixels (so the edges
    come from their extremes); otherwise from every pixel with a valid reference."""
    st = plan.label_stats()
    dt = np_dtype(plan.ref)
    key = ("inlier_ref_min", "inlier_ref_max") if over_inliers else ("ref_min", "ref_max")
    empty = len(st["ids"]) == 0 or np.isnan(st[key[0]][0])
    if empty and not isinstance(bins, np.ndarray) and kind in ("fixed", "count", "quantile"):
        raise ValueError("zero-size array to reduction operation minimum which has no identity")   # (what ref_dem.min() raises)
    ref_min, ref_max = (dt.type(st[key[0]][0]), dt.type(st[key[1]][0])) if not empty else (dt.type(np.nan),) * 2

    def ref_valid():
        ref = _host(plan.ref)
        keep = np.isfinite(ref)
        if over_inliers:
            keep &= np.isfinite(_host(plan.ddem))
            if plan.mask is not None:
                keep &= _host(plan.mask).astype(bool)
        return ref[keep]

    zbins = _zbins(kind, bins, ref_min, ref_max, ref_valid)
    nb = zbins.shape[0] - 1
    vdt = np_dtype(plan.ddem)
    if nb < 1 or empty:
        return _binning_frame(zbins, np.full(max(nb, 0), np.nan, dtype=vdt), np.zeros(max(nb, 0), dtype=int))
    if np.any(np.diff(np.asarray(zbins, dtype=np.float64)) < 0):
        raise ValueError("bins must be monotonically increasing or decreasing")   # np.digitize's own message; decreasing: not here
    counts, med, _ = plan.segments([1], np.asarray(zbins, dtype=np.float64)[None, :])
    if aggregation_function in _DEVICE_MEDIANS:
        stat = med[0]
    else:
        _, stat = _host_statistic(plan, nb, 0, aggregation_function)
    values, out_counts = _rotated(nb, counts[0], stat, vdt)
    return _binning_frame(zbins, values, out_counts)


def _below_threshold(table: pd.DataFrame, source: pd.DataFrame, value_column: str, count_threshold):
    """The rows whose pixel count lies under `count_threshold`, their value set to NaN in `table`; None without a threshold."""
    if count_threshold is None:
        return None
    assert "count" in source.columns, "'count' not a column in the dataframe"
    low = table["count"] < count_threshold
    table.loc[low, value_column] = np.nan
    return low


def interpolate_hypsometric_bins(
    hypsometric_bins: pd.DataFrame,
    value_column: str = "value",
    method: str = "polynomial",
    order: int = 3,
    count_threshold: int | None = None,
) -> pd.DataFrame:
    """NaN bins filled by pandas' ``Series.interpolate`` over the bin midpoints, no extrapolation
    (``xdem.volume.interpolate_hypsometric_bins``; host only).

    `method` / `order` go to pandas; bins with fewer than `count_threshold` pixels are kept out of the interpolation and get their
    own value back.  With `order + 1` valid bins or fewer a copy is returned, with upstream's warning.
    """
    table = hypsometric_bins.copy()
    table.index = table.index.mid
    low = _below_threshold(table, hypsometric_bins, value_column, count_threshold)
    if np.count_nonzero(np.isfinite(table[value_column])) <= order + 1:
        warnings.warn("Not enough valid bins for interpolation -> returning copy", UserWarning)
        return hypsometric_bins.copy()
    table[value_column] = table[value_column].interpolate(method=method, order=order, limit_direction="both")
    if low is not None:
        table.loc[low, value_column] = hypsometric_bins.loc[low.values, value_column]
    table.index = hypsometric_bins.index
    return table


def fit_hypsometric_bins_poly(
    hypsometric_bins: pd.DataFrame,
    value_column: str = "value",
    degree: int = 3,
    iterations: int = 1,
    count_threshold: int | None = None,
) -> pd.Series:
    """The bins replaced by a polynomial of `degree` fitted over their midpoints (``xdem.volume.fit_hypsometric_bins_poly``; host
    only): up to `iterations` rounds of ``np.polyfit``, each dropping the bins whose residual exceeds three standard deviations
    of the residuals; bins with fewer than `count_threshold` pixels never take part.
    """
    table = hypsometric_bins.copy()
    table.index = table.index.mid
    _below_threshold(table, hypsometric_bins, value_column, count_threshold)
    used = np.isfinite(np.asarray(table[value_column]))
    for _ in range(iterations):
        coefficients = np.polyfit(table.index[used], table[value_column][used], deg=degree)
        fitted = np.polyval(coefficients, table.index)
        residuals = (fitted - table[value_column]).values
        before = used.copy()
        used[np.abs(residuals) > 3 * np.nanstd(residuals)] = False
        if np.array_equal(used, before):
            break
    return pd.DataFrame(index=hypsometric_bins.index, data=np.vstack([fitted, table["count"]]).T, columns=["value", "count"])


_TIMEFRAMES = {"reference": 0, "nonreference": 1, "mean": 2}


def _area_counts(ref, timeframe: int, xs: np.ndarray, ys: np.ndarray, bins: np.ndarray) -> np.ndarray:
    """np.histogram(elevations, bins)[0] of calculate_hypsometry_area for the flat raster `ref` (``xdemhip_hypso_area``)."""
    nb = bins.shape[0] - 1
    counts = np.zeros(nb, np.int64)
    xs, ys, bins = np.ascontiguousarray(xs), np.ascontiguousarray(ys), np.ascontiguousarray(bins)
    ctx = _lib.default_context(ref.device.index if is_tensor(ref) else None)
    if is_tensor(ref):
        _args.synchronize_torch(ref)
    with ctx.call_lock:
        ctx.check(ctx._L.xdemhip_hypso_area(ctx.handle, ptr(ref), code(ref), int(ref.shape[0]), timeframe, int(xs.shape[0]), dp(xs), dp(ys),
                                           nb, dp(bins), i64p(counts), _args.space(ref)))
    return counts


def calculate_hypsometry_area(
    ddem_bins: pd.Series | pd.DataFrame,
    ref_dem,
    pixel_size: float | tuple[float, float],
    timeframe: str = "reference",
) -> pd.Series:
    """The area of the reference DEM that falls into each bin of `ddem_bins` (``xdem.volume.calculate_hypsometry_area``).

    The elevations are those of `ref_dem` ("reference"), of the other DEM, ``ref - f(ref)`` ("nonreference"), or of the time in
    between, ``ref - f(ref) / 2`` ("mean"), `f` being the linear interpolant of the bins' values over their midpoints.  `ref_dem`
    must hold no NaN; `pixel_size` is one length or an (x, y) pair.  Returns a Series over the bins' index.
    """
    ref = _float_plane(ref_dem.data if isinstance(ref_dem, np.ma.MaskedArray) else ref_dem, "ref_dem")   # (upstream reads `.data`)
    nan_count = int(ref.isnan().sum().item()) if is_tensor(ref) else int(np.count_nonzero(np.isnan(ref)))
    assert not nan_count, "The given reference DEM has NaNs. No NaNs are allowed to calculate area!"
    if timeframe not in _TIMEFRAMES:
        raise ValueError(f"Argument 'timeframe={timeframe}' is invalid. Choices: ['reference', 'nonreference', 'mean'].")
    series = ddem_bins["value"] if isinstance(ddem_bins, pd.DataFrame) else ddem_bins
    xs = ys = np.zeros(2)
    if timeframe != "reference":
        assert not np.any(np.isnan(series.values)), "The dDEM bins cannot contain NaNs. Remove or fill them first."
        # (interp1d's own checks and its sorting of x run here; the device evaluates the table it holds)
        model = scipy.interpolate.interp1d(series.index.mid, series.values, kind="linear", fill_value="extrapolate")
        xs, ys = np.asarray(model.x, dtype=np.float64), np.asarray(model.y, dtype=np.float64)
    edges = np.asarray(np.r_[[series.index.left[0]], series.index.right], dtype=np.float64)
    if np.any(edges[:-1] > edges[1:]):
        raise ValueError("`bins` must increase monotonically, when an array")   # (np.histogram's message)
    pixels = _area_counts(ref, _TIMEFRAMES[timeframe], xs, ys, edges).astype(np.intp)
    pixel_area = pixel_size[0] * pixel_size[1] if isinstance(pixel_size, tuple) else pixel_size**2
    return pd.Series(index=series.index, data=pixels * pixel_area)


def hypsometric_interpolation(voided_ddem, ref_dem, mask):
    """The voids of a dDEM inside `mask` filled from the dDEM's median per 50 m elevation bin
    (``xdem.volume.hypsometric_interpolation``).

    The bins are taken over the pixels of `mask` where both rasters are valid, empty bins are interpolated, and the linear model
    over the bin midpoints (extrapolating) is evaluated at the reference elevation of every void inside the mask.  Returns a masked
    array (host inputs) or a tensor (device inputs).
    """
    shape = tuple(int(d) for d in voided_ddem.shape if d != 1)   # (get_array_and_mask squeezes)
    with HypsoPlan(voided_ddem, ref_dem, mask=mask) as plan:
        st = plan.label_stats()
        if len(st["ids"]) == 0 or st["inliers"][0] == 0:
            warnings.warn("No valid data found within mask, returning copy", UserWarning)
            return voided_ddem.clone() if is_tensor(voided_ddem) else np.ma.masked_array(data=voided_ddem)
        gradient = interpolate_hypsometric_bins(_binning_of(plan, 50.0, "fixed", np.median, over_inliers=True))
        model = scipy.interpolate.interp1d(gradient.index.mid, gradient["value"].values, fill_value="extrapolate")
        out_dtype = np.promote_types(np_dtype(plan.ddem), np_dtype(plan.ref))
        out = plan.fill(0, [1], np.asarray(model.x, np.float64), np.asarray(model.y, np.float64), True, out_dtype)
    out = out.reshape(shape)
    if is_tensor(out):
        return out
    return np.ma.masked_array(out, mask=~np.isfinite(out))


def _assert_void_free(stats: dict) -> None:
    assert stats["ref_invalid"] == 0, "Reference DEM has voids"


_SIGNAL_PERCENTILES = (("sigma-1-lower", 16), ("sigma-1-upper", 84), ("sigma-2-lower", 2.5), ("sigma-2-upper", 97.5))


def _regional_signal(plan: HypsoPlan, st: dict, n_bins: int, min_coverage: float) -> pd.DataFrame:
    ids, pix, inl = st["ids"], st["pixels"], st["inliers"]
    n_unique = len(ids) + (1 if int(pix.sum()) < plan.n else 0)   # (np.unique sees label 0 too where it occurs)
    values = np.full((n_bins, n_unique), fill_value=np.nan, dtype=float)
    counts = np.full((n_bins, n_unique), fill_value=np.nan, dtype=float)
    # upstream's decisions (volume.py:609-635): outlines of fewer than 10 pixels, coverage under the threshold, no inlier at all
    keep = (pix >= 10) & ~((inl / pix) < min_coverage) & (inl > 0)
    kept = ids[keep]
    dt, vdt = np_dtype(plan.ref), np_dtype(plan.ddem)
    if len(kept):
        edges = [_zbins("count", n_bins, dt.type(lo), dt.type(hi), None) for lo, hi in zip(st["inlier_ref_min"][keep], st["inlier_ref_max"][keep])]
        g_counts, g_med, _ = plan.segments(kept, np.asarray(edges, dtype=np.float64))
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)   # (a glacier whose bins hold one value divides 0 by 0, as upstream)
            for column, zbins in enumerate(edges):
                v, c = _rotated(n_bins, g_counts[column], g_med[column], vdt)
                frame = _binning_frame(zbins, v, c)
                lowest, highest = np.nanmin(frame["value"]), np.nanmax(frame["value"])
                values[:, column] = (frame["value"] - lowest) / (highest - lowest)
                counts[:, column] = frame["count"]
    columns = {"w_mean": np.nansum(values * counts, axis=1) / np.nansum(counts, axis=1), "median": np.nanmedian(values, axis=1),
               "std": np.nanstd(values, axis=1)}
    for name, q in _SIGNAL_PERCENTILES:
        columns[name] = np.nanpercentile(values, q, axis=1)
    columns["count"] = np.nansum(counts, axis=1).astype(int)
    return pd.DataFrame(data=columns, index=pd.IntervalIndex.from_breaks(np.linspace(0, 1, n_bins + 1, dtype="float64")))


def get_regional_hypsometric_signal(ddem, ref_dem, glacier_index_map, n_bins: int = 20, min_coverage: float = 0.05) -> pd.DataFrame:
    """The normalised shape of elevation change against elevation over all glaciers of an index map
    (``xdem.volume.get_regional_hypsometric_signal``).

    Every glacier of at least 10 pixels and `min_coverage` valid dDEM is cut into `n_bins` elevation bins, its bin medians are
    scaled to [0, 1], and the glaciers are combined per bin: count-weighted mean, median, standard deviation, four percentiles, the
    pixel count.  `ref_dem` must be void free; label 0 is no glacier.
    """
    with HypsoPlan(ddem, ref_dem, labels=glacier_index_map) as plan:
        st = plan.label_stats()
        _assert_void_free(st)
        return _regional_signal(plan, st, n_bins, min_coverage)


def _line(x, a, b):
    return a * x + b


def regional_glacier_models(plan: HypsoPlan, st: dict, regional_signal: pd.DataFrame, min_coverage: float, min_elevation_range: float) -> list:
    """Per glacier of the index map (ascending), what norm_regional_hypsometric_interpolation decides and fits (volume.py:715-797):
    dicts with "id", "skipped" and, where the glacier passed the coverage threshold, "value", "count", "std" (its bins) and, where a
    fit was made, "coeffs" and the model table "x" = signal.index.mid, "y" = np.poly1d(coeffs)(signal.values).  One grouping pass
    serves all glaciers."""
    ids, pix, inl = st["ids"], st["pixels"], st["inliers"]
    dt, vdt = np_dtype(plan.ref), np_dtype(plan.ddem)
    records = [{"id": int(i), "skipped": True} for i in ids]
    passing = [k for k in range(len(ids)) if not (inl[k] / pix[k]) < min_coverage]
    signals = []
    for k in passing:
        if inl[k] == 0:
            raise ValueError("zero-size array to reduction operation minimum which has no identity")   # (upstream's binning call)
        low, high = dt.type(st["ref_min"][k]), dt.type(st["ref_max"][k])
        # the signal's unit interval stretched over the glacier's elevations, as upstream does it: in place on the midpoints' Index
        scaled = regional_signal["w_mean"].copy()
        mids = scaled.index.mid
        mids *= high - low
        mids += low
        width = mids[1] - mids[0]
        scaled.index = pd.IntervalIndex.from_arrays(left=mids - width / 2, right=mids + width / 2)
        signals.append(scaled)
    if not passing:
        return records
    edges = np.asarray([np.r_[[s.index.left[0]], s.index.right] for s in signals], dtype=np.float64)
    n_bins = edges.shape[1] - 1
    g_counts, g_med, g_std = plan.segments(ids[passing], edges, want_std=True)
    for j, k in enumerate(passing):
        scaled, rec = signals[j], records[k]
        v, c = _rotated(n_bins, g_counts[j], g_med[j], vdt)
        s, _ = _rotated(n_bins, g_counts[j], g_std[j], vdt)
        medians, spreads = _binning_frame(edges[j], v, c), _binning_frame(edges[j], s, c)
        rec.update(value=medians["value"].values, count=medians["count"].values, std=spreads["value"].values)
        filled = np.isfinite(medians["value"])
        with np.errstate(invalid="ignore", divide="ignore"):
            covered = np.sum(filled[filled].index.length) / np.sum(medians.index.length)
        if covered < min_elevation_range or np.count_nonzero(filled) < 2:
            continue
        sigma = spreads["value"].values[filled] / np.sqrt(medians["count"].values[filled])
        sigma[sigma == 0.0] = 1e-8
        with warnings.catch_warnings():
            warnings.filterwarnings("ignore", message="covariance")
            coeffs = scipy.optimize.curve_fit(f=_line, xdata=scaled.values[filled], ydata=medians["value"].values[filled], p0=[1, 0], sigma=sigma)[0]
        model = scipy.interpolate.interp1d(scaled.index.mid, np.poly1d(coeffs)(scaled.values), bounds_error=False, fill_value="extrapolate")
        rec.update(skipped=False, coeffs=coeffs, x=np.asarray(model.x, np.float64), y=np.asarray(model.y, np.float64))
    return records


def norm_regional_hypsometric_interpolation(
    voided_ddem,
    ref_dem,
    glacier_index_map,
    min_coverage: float = 0.1,
    regional_signal: pd.DataFrame | None = None,
    min_elevation_range: float = 0.33,
    idealized_ddem: bool = False,
):
    """The voids of every glacier filled with the regional signal scaled to that glacier
    (``xdem.volume.norm_regional_hypsometric_interpolation``).

    Per glacier with at least `min_coverage` valid dDEM whose non-empty bins span `min_elevation_range` of its elevations, a line
    ``a * signal + b`` is fitted to its bin medians (weights from the bins' standard deviation and count) and evaluated at the
    reference elevation of its voids -- of all its pixels with `idealized_ddem`.  `regional_signal` defaults to
    ``get_regional_hypsometric_signal`` of the same inputs; `ref_dem` must be void free (AssertionError).  Returns the filled
    dDEM in the input's dtype and memspace.
    """
    shape = tuple(int(d) for d in voided_ddem.shape if d != 1)   # (get_array_and_mask squeezes)
    with HypsoPlan(voided_ddem, ref_dem, labels=glacier_index_map) as plan:
        st = plan.label_stats()
        _assert_void_free(st)
        if regional_signal is None:
            regional_signal = _regional_signal(plan, st, 20, 0.05)
        fitted = [r for r in regional_glacier_models(plan, st, regional_signal, min_coverage, min_elevation_range) if not r["skipped"]]
        ids = [r["id"] for r in fitted]
        xs = np.asarray([r["x"] for r in fitted], dtype=np.float64)
        ys = np.asarray([r["y"] for r in fitted], dtype=np.float64)
        out = plan.fill(1 if idealized_ddem else 0, ids, xs, ys, False, np_dtype(plan.ddem))
    return out.reshape(shape)
