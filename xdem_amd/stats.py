"""Raster statistics on the GPU: ``get_stats`` (geoutils' ``Raster.get_stats``, which ``xdem.DEM`` inherits and the reference's
workflows call on every DEM and every elevation difference: xdem/workflows/topo.py:291, accuracy.py:243-381), an exact
``percentile`` and ``linear_error``.

One device call (``xdemhip_raster_stats``: csrc/rasterstats.hip over csrc/multi_select.h) returns the count, the extremes, the
float64 sums and the ORDER STATISTICS next to every wanted rank; what is left to the host is a handful of float64 operations:
the interpolation between two neighbouring order statistics with NumPy's own formula (``_lerp``), divisions and square roots.

The keys and their definitions are this project's restatement of geoutils' published ``get_stats`` (geoutils is not
installed where this project is developed and nothing offline pins it).  With ``v`` the valid values in their dtype ``T`` and
``v64 = v.astype(float64)``: Mean = sum(v64) / n; Median = np.median(v) (the mean of the two middle values taken in T); Max, Min;
Sum, Sum of squares (float64); 90th percentile = np.percentile(v64, 90); LE90 = np.percentile(v64, 95) - np.percentile(v64, 5);
NMAD = spatialstats.nmad(v); RMSE = sqrt(sum(v64^2) / n); Standard deviation = sqrt(sum((v64 - mean)^2) / n); Valid count,
Total count, Percentage valid points.  A pixel is valid when it is finite, is not ``nodata`` and is not masked.  ``nodata`` is rounded
to the dtype of the values before it is compared (``v == nodata`` in NumPy, and what ``DEM`` does when it is built): for a float32
raster ``nodata=0.1`` drops the pixels that hold ``np.float32(0.1)``.
"""
from __future__ import annotations

import ctypes
import math

import numpy as np

from . import _args, _lib
from ._args import is_tensor

STAT_KEYS = ("Mean", "Median", "Max", "Min", "Sum", "Sum of squares", "90th percentile", "LE90", "NMAD", "RMSE", "Standard deviation",
             "Valid count", "Total count", "Percentage valid points")
INLIER_KEYS = ("Valid inlier count", "Total inlier count", "Percentage inlier points", "Percentage valid inlier points")
NFACT = 1.4826
MAX_Q = 4   # XDEMHIP_STATS_MAXQ: quantiles of one device call


def _norm(name: str) -> str:
    return "".join(name.split()).lower()


# every key by its normalised spelling, the configuration names of the reference's workflows (xdem/workflows/schemas.py:
# STATS_METHODS -- the normalised keys but for "std") and the report labels its _ALIAS gives "max" and "min"
_NAMES = {_norm(k): k for k in STAT_KEYS + INLIER_KEYS}
_NAMES.update({"std": "Standard deviation", "maximum": "Max", "minimum": "Min"})


def resolve_name(name: str) -> str:
    """The key of the statistic called `name` (case and spaces do not matter); ``ValueError`` listing the choices otherwise."""
    if not isinstance(name, str) or _norm(name) not in _NAMES:
        raise ValueError(f"Statistic name '{name}' is not recognized; choose from {sorted(_NAMES)} or pass a callable.")
    return _NAMES[_norm(name)]


def _lerp(a: float, b: float, n: int, q: float) -> float:
    """NumPy's ``method="linear"`` interpolation between the order statistics `a`, `b` of ranks floor((n - 1) q) and the next, in
    float64 (numpy/lib/_function_base_impl.py: _lerp)."""
    a, b = np.float64(a), np.float64(b)
    vi = np.float64(n - 1) * np.float64(q)
    t = vi - np.floor(vi)
    d = b - a
    r = a + d * t
    if t >= 0.5:
        r = b - d * (1 - t)
    if b == a:
        r = a
    return float(r)


class _Input:
    """What the device call reads: values (NumPy float32 / float64 array or CUDA tensor), the byte masks, nodata, the sizes."""

    def __init__(self, values, inlier_mask, nodata):
        self.tensor = is_tensor(values)
        self.total_mask = None
        if self.tensor:
            self.values = _args.device_float(values, "a tensor input must be a contiguous float32 or float64 CUDA tensor", ndim=None)
            self.size = int(values.numel())
            self.shape = tuple(values.shape)
        else:
            if isinstance(values, np.ma.MaskedArray):
                m = np.ma.getmaskarray(values)
                if m.any():
                    self.total_mask = np.ascontiguousarray(~m, dtype=np.uint8)
                values = values.data
            v = np.asarray(getattr(values, "data", values) if not isinstance(values, np.ndarray) else values)
            self.values = _args.host_float(v, np.float64)
            self.size = int(v.size)
            self.shape = v.shape
        self.inlier = None
        if inlier_mask is not None:
            inl = getattr(inlier_mask, "data", inlier_mask) if not is_tensor(inlier_mask) else inlier_mask
            inl = _args.mask_u8(inl, self.values, nonzero=True)
            if tuple(inl.shape) != tuple(self.shape):
                raise ValueError(f"inlier_mask has shape {tuple(inl.shape)}, the values {tuple(self.shape)}")
            self.inlier = inl
        self.nodata = None if nodata is None or (isinstance(nodata, float) and math.isnan(nodata)) else float(nodata)

    def host_valid_values(self) -> np.ndarray:
        """The valid (and inlier) values on the host, in raster order: what a callable statistic is applied to."""
        v = self.values.cpu().numpy() if self.tensor else self.values
        ok = np.isfinite(v)
        if self.nodata is not None:
            with np.errstate(over="ignore"):
                ok &= v != v.dtype.type(self.nodata)   # (rounded to the dtype first: NumPy's `v == nodata`, and DEM's)
        if self.total_mask is not None:
            ok &= self.total_mask.astype(bool)
        if self.inlier is not None:
            ok &= (self.inlier.cpu().numpy() if self.tensor else self.inlier).astype(bool)
        return v[ok]


def _device_stats(inp: _Input, quantiles, ctx: _lib.Context | None = None) -> dict:
    """``xdemhip_raster_stats`` on the prepared input: its output block as a dict (q_lo / q_hi: one entry per quantile)."""
    ctx = ctx or (_lib.default_context(inp.values.device.index) if inp.tensor else _lib.default_context())
    qs = [float(q) for q in quantiles]
    if len(qs) > MAX_Q:
        raise ValueError(f"at most {MAX_Q} quantiles per device call")
    out = _lib.RasterStatsOut()
    qa = (ctypes.c_double * max(len(qs), 1))(*qs)
    has_nd, nd = (1, inp.nodata) if inp.nodata is not None else (0, 0.0)
    v = inp.values
    with _args.torch_stream_scope(ctx, v, reset=True):
        ctx.check(ctx._L.xdemhip_raster_stats(ctx.handle, _args.ptr(v) if inp.size else None, _args.code(v), inp.size, _args.ptr(inp.total_mask),
                                              _args.ptr(inp.inlier), has_nd, nd, qa, len(qs), NFACT, _args.space(v), ctypes.byref(out)))
    d = {k: getattr(out, k) for k in ("n", "n_valid", "n_inlier", "min", "max", "sum", "sumsq", "sumdev2", "med_lo", "med_hi", "median", "mad_lo",
                                      "mad_hi", "nmad", "reads")}
    d["q_lo"], d["q_hi"] = list(out.q_lo)[:len(qs)], list(out.q_hi)[:len(qs)]
    d["route"] = tuple(out.route)
    return d


def _all_stats(inp: _Input, ctx) -> dict:
    r = _device_stats(inp, (0.9, 0.95, 0.05), ctx)
    n, total = int(r["n"]), inp.size
    nan = float("nan")
    s = dict.fromkeys(STAT_KEYS, nan)
    if n > 0:
        p = [_lerp(r["q_lo"][i], r["q_hi"][i], n, q) for i, q in enumerate((0.9, 0.95, 0.05))]
        s.update({"Mean": r["sum"] / n, "Median": float(r["median"]), "Max": float(r["max"]), "Min": float(r["min"]), "Sum": float(r["sum"]),
                  "Sum of squares": float(r["sumsq"]), "90th percentile": p[0], "LE90": p[1] - p[2], "NMAD": float(r["nmad"]),
                  "RMSE": math.sqrt(r["sumsq"] / n), "Standard deviation": math.sqrt(r["sumdev2"] / n)})
    valid = int(r["n_valid"])
    s.update({"Valid count": valid, "Total count": total, "Percentage valid points": (valid / total * 100) if total else nan})
    if inp.inlier is not None:
        n_inl = int(r["n_inlier"])
        s.update({"Valid inlier count": n, "Total inlier count": n_inl, "Percentage inlier points": (n / valid * 100) if valid else 0.0,
                  "Percentage valid inlier points": (n / n_inl * 100) if n_inl else 0.0})
    return s


def get_stats(values, stats_name=None, inlier_mask=None, nodata=None, ctx: _lib.Context | None = None):
    """Statistics of a raster: a dict of all of them (``stats_name=None``), of the listed ones (keyed as given; a callable by its
    ``__name__``), or the bare value for a single name or callable.

    `values`: N-D NumPy array, masked array, or a contiguous float32 / float64 CUDA tensor (read in place, on the current torch
    stream); other dtypes are widened to float64.  `inlier_mask` (True = keep) restricts the value statistics; the three count keys
    keep describing the whole raster and four inlier keys are added.  `nodata` is rounded to the dtype of the values before it is
    compared with them, on the device and for a callable alike.  A callable is applied on the host to the valid values in raster
    order."""
    single = stats_name is not None and (isinstance(stats_name, str) or callable(stats_name))
    names = None if stats_name is None else ([stats_name] if single else list(stats_name))
    keys = None if names is None else [n if callable(n) else resolve_name(n) for n in names]   # (errors before any work)
    inp = _Input(values, inlier_mask, nodata)
    if keys is not None:
        for k in keys:
            if not callable(k) and k in INLIER_KEYS and inp.inlier is None:
                raise ValueError(f"'{k}' needs an inlier_mask")
    s = _all_stats(inp, ctx) if keys is None or any(not callable(k) for k in keys) else {}
    if keys is None:
        return s
    host = inp.host_valid_values() if any(callable(k) for k in keys) else None
    vals = [k(host) if callable(k) else s[k] for k in keys]
    if single:
        return vals[0]
    return {(n.__name__ if callable(n) else n): v for n, v in zip(names, vals)}


def percentile(values, q, inlier_mask=None, nodata=None, ctx: _lib.Context | None = None):
    """Exact ``np.nanpercentile(valid values as float64, q, method="linear")``: a float64 scalar for a scalar `q`, else an array of
    the shape of `q`.  The device selects the two order statistics next to every wanted rank (at most 4 values of `q` per call,
    longer lists in chunks); NaN when nothing is valid."""
    qa = np.asarray(q, dtype=np.float64)
    if qa.size and not (np.all(qa >= 0) and np.all(qa <= 100)):
        raise ValueError("Percentiles must be in the range [0, 100]")
    quant = np.true_divide(qa, 100).ravel()
    inp = _Input(values, inlier_mask, nodata)
    res = np.full(quant.size, np.nan)
    for c0 in range(0, quant.size, MAX_Q):
        chunk = quant[c0:c0 + MAX_Q]
        r = _device_stats(inp, chunk, ctx)
        n = int(r["n"])
        if n > 0:
            for i, qq in enumerate(chunk):
                res[c0 + i] = _lerp(r["q_lo"][i], r["q_hi"][i], n, qq)
    return np.float64(res[0]) if qa.ndim == 0 else res.reshape(qa.shape)


def linear_error(values, interval: float = 90, inlier_mask=None, nodata=None, ctx: _lib.Context | None = None) -> float:
    """The width of the central `interval` percent of the valid values: percentile(50 + interval / 2) - percentile(50 - interval / 2)
    (LE90 for the default)."""
    if not isinstance(interval, (int, float)) or isinstance(interval, bool) or not 0 < interval <= 100:
        raise ValueError("Interval must be a number greater than 0 and lesser than 100.")
    hi, lo = percentile(values, [50 + interval / 2, 50 - interval / 2], inlier_mask=inlier_mask, nodata=nodata, ctx=ctx)
    return float(hi - lo)
