"""NumPy restatement of xdem_amd.stats: the table of keys (``table``), and the block ``xdemhip_raster_stats`` returns
(``device_block``; ``patched()`` puts it in the device call's place for the host tests).  The sums are exact: ``math.fsum``."""
from __future__ import annotations

import contextlib
import math

import numpy as np

from xdem_amd import spatialstats, stats


def valid_values(values, inlier_mask=None, nodata=None):
    """(valid-and-inlier values in their dtype, raster order; valid pixels whatever the inlier mask; inlier pixels; all pixels).
    Valid: finite, not nodata, not masked.  Dtypes other than float32 / float64 are widened to float64."""
    total_mask = None
    if isinstance(values, np.ma.MaskedArray):
        total_mask = ~np.ma.getmaskarray(values)
        values = values.data
    v = np.asarray(values)
    if v.dtype not in (np.dtype(np.float32), np.dtype(np.float64)):
        v = v.astype(np.float64)
    ok = np.isfinite(v)
    if nodata is not None and not (isinstance(nodata, float) and math.isnan(nodata)):
        ok &= v != nodata
    if total_mask is not None:
        ok &= total_mask
    n_valid = int(ok.sum())
    n_inlier = v.size
    if inlier_mask is not None:
        inl = np.asarray(inlier_mask, dtype=bool)
        n_inlier = int(inl.sum())
        ok = ok & inl
    return v[ok], n_valid, n_inlier, int(v.size)


def table(values, inlier_mask=None, nodata=None) -> dict:
    """Every key of ``stats.get_stats`` from NumPy's own functions."""
    v, n_valid, n_inlier, total = valid_values(values, inlier_mask, nodata)
    n = v.size
    s = dict.fromkeys(stats.STAT_KEYS, float("nan"))
    if n:
        v64 = v.astype(np.float64)
        fs, fs2 = math.fsum(v64), math.fsum(v64 * v64)
        mean = fs / n
        s.update({"Mean": mean, "Median": float(np.median(v)), "Max": float(v.max()), "Min": float(v.min()), "Sum": fs, "Sum of squares": fs2,
                  "90th percentile": float(np.percentile(v64, 90)), "LE90": float(np.percentile(v64, 95) - np.percentile(v64, 5)),
                  "NMAD": float(spatialstats.nmad(v)), "RMSE": math.sqrt(fs2 / n), "Standard deviation": math.sqrt(math.fsum((v64 - mean) ** 2) / n)})
    s.update({"Valid count": n_valid, "Total count": total, "Percentage valid points": n_valid / total * 100 if total else float("nan")})
    if inlier_mask is not None:
        s.update({"Valid inlier count": int(n), "Total inlier count": n_inlier, "Percentage inlier points": n / n_valid * 100 if n_valid else 0.0,
                  "Percentage valid inlier points": n / n_inlier * 100 if n_inlier else 0.0})
    return s


def device_block(inp, quantiles, ctx=None) -> dict:
    """What ``stats._device_stats`` returns, from a sort."""
    if inp.tensor:
        raise NotImplementedError("host oracle: NumPy inputs only")
    vals = inp.values if inp.total_mask is None else np.ma.MaskedArray(inp.values, mask=~inp.total_mask.astype(bool))
    v, n_valid, n_inlier, _ = valid_values(vals, None if inp.inlier is None else inp.inlier.astype(bool), inp.nodata)
    n = int(v.size)
    nan = float("nan")
    qs = [float(q) for q in quantiles]
    d = {"n": n, "n_valid": n_valid, "n_inlier": n_inlier, "reads": 0.0, "route": (1, 1), "q_lo": [nan] * len(qs), "q_hi": [nan] * len(qs)}
    d.update(dict.fromkeys(("min", "max", "sum", "sumsq", "sumdev2", "med_lo", "med_hi", "median", "mad_lo", "mad_hi", "nmad"), nan))
    if n == 0:
        return d
    T = v.dtype.type
    srt = np.sort(v)
    v64 = v.astype(np.float64)
    mean = math.fsum(v64) / n
    med = T((srt[(n - 1) // 2] + srt[n // 2]) / T(2)) if n % 2 == 0 else srt[n // 2]
    dev = np.sort(np.abs(v - med))
    mad = T((dev[(n - 1) // 2] + dev[n // 2]) / T(2)) if n % 2 == 0 else dev[n // 2]
    d.update({"min": float(srt[0]), "max": float(srt[-1]), "sum": math.fsum(v64), "sumsq": math.fsum(v64 * v64), "sumdev2": math.fsum((v64 - mean) ** 2),
              "med_lo": float(srt[(n - 1) // 2]), "med_hi": float(srt[n // 2]), "median": float(med), "mad_lo": float(dev[(n - 1) // 2]),
              "mad_hi": float(dev[n // 2]), "nmad": float(T(T(stats.NFACT) * mad))})
    for i, q in enumerate(qs):
        lo = min(int(math.floor(np.float64(n - 1) * np.float64(q))), n - 1)
        d["q_lo"][i], d["q_hi"][i] = float(srt[lo]), float(srt[min(lo + 1, n - 1)])
    return d


@contextlib.contextmanager
def patched():
    """xdem_amd.stats with its device call replaced by the restatement above."""
    saved = stats._device_stats
    stats._device_stats = device_block
    try:
        yield stats
    finally:
        stats._device_stats = saved
