"""NumPy restatement of xdem_amd.stats: the table of keys (``table``), and the block ``xdemhip_raster_stats`` returns
(``device_block``; ``patched()`` puts it in the device call's place for the host tests).  The sums are exact: ``math.fsum``."""
from __future__ import annotations

import contextlib
import math

import numpy as np

from xdem_amd import spatialstats, stats


def valid_mask(values, inlier_mask=None, nodata=None):
    """(values as float32 / float64; valid-and-inlier pixels; valid pixels whatever the inlier mask; inlier pixels or None).
    Valid: finite, not nodata (`v != nodata` as NumPy decides it: nodata rounded to the dtype of v), not masked.  Dtypes other than
    float32 / float64 are widened to float64."""
    total_mask = None
    if isinstance(values, np.ma.MaskedArray):
        total_mask = ~np.ma.getmaskarray(values)
        values = values.data
    v = np.asarray(values)
    if v.dtype not in (np.dtype(np.float32), np.dtype(np.float64)):
        v = v.astype(np.float64)
    valid = np.isfinite(v)
    if nodata is not None and not (isinstance(nodata, float) and math.isnan(nodata)):
        with np.errstate(over="ignore"):
            valid &= v != v.dtype.type(nodata)
    if total_mask is not None:
        valid &= total_mask
    inl = None if inlier_mask is None else np.asarray(inlier_mask, dtype=bool)
    return v, (valid if inl is None else valid & inl), valid, inl


def valid_values(values, inlier_mask=None, nodata=None):
    """(valid-and-inlier values in their dtype, raster order; valid pixels whatever the inlier mask; inlier pixels; all pixels)."""
    v, ok, valid, inl = valid_mask(values, inlier_mask, nodata)
    return v[ok], int(valid.sum()), int(v.size if inl is None else inl.sum()), int(v.size)


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


# ---- the sample and the brackets of the bracketed route (csrc/select.h, select_run.h, rasterstats.hip), restated ----------------
# Used to BUILD inputs and to assert that a built input has the property its test is about (the brackets hold, a named one misses,
# a workgroup's staging buffer fills) -- never to produce an expected value: those stay with `device_block` / `table` above.
LINE = 8                 # elements of a sampled line (SEL_LINE)
TILE = 4096              # elements a workgroup takes per step (HIST_THREADS x SEL_TILE)
FLUSH_EVERY = 4          # steps between two flushes of the staging buffer (SEL_FLUSH_EVERY)
STAGE_CAP = 8192         # slots of the staging buffer (SEL_STAGE_CAP)
BRACKET_DIGITS = 3       # leading key bytes the sample's selection fixes
PASSES = {np.dtype(np.float32): 4, np.dtype(np.float64): 8}


def sampled_positions(n: int) -> np.ndarray:
    """The elements of the 1/64 line sample of an n-element raster, ascending: one LINE-element line per group of 64 lines, picked by
    the top 6 bits of a multiplicative hash of the group's number (sel_sampled_line / sample_lines_kernel)."""
    groups = -(-(-(-n // LINE)) // 64)
    g = np.arange(groups, dtype=np.uint64)
    line = g * np.uint64(64) + ((g * np.uint64(0x9E3779B97F4A7C15)) >> np.uint64(58))   # (uint64 arrays wrap: mod 2^64)
    pos = (line[:, None] * np.uint64(LINE) + np.arange(LINE, dtype=np.uint64)[None, :]).reshape(-1).astype(np.int64)
    return pos[pos < n]


def ordered_keys(v: np.ndarray) -> np.ndarray:
    """key_of: unsigned integers that order as the floats do (negative: every bit flipped; else the sign bit set)."""
    K = np.uint32 if v.dtype == np.float32 else np.uint64
    b = np.ascontiguousarray(v).view(K)
    top = K(1) << K(8 * v.dtype.itemsize - 1)
    return np.where(b & top, ~b, b | top).astype(K)


def rank_pair(c: int, q=None):
    """ms_rank: the two ranks wanted of c elements -- the medians (q None), or floor((c - 1) q) and the next, clipped."""
    if q is None:
        return (c - 1) // 2, c // 2
    lo = min(int(math.floor(np.float64(c - 1) * np.float64(q))), c - 1)
    return lo, min(lo + 1, c - 1)


def halfwidth(m: int) -> int:
    """sel_bracket_halfwidth: sample ranks a bracket end is moved by."""
    return int(3.0 * math.sqrt(8.0 * m)) + 32


def predict_round(values_flat, valid_flat, qs, dtype, n_cu: int, flush_every: int = FLUSH_EVERY) -> dict:
    """One round of the bracketed route on `values_flat` (raster order) of which `valid_flat` are used, for the median and the
    quantiles `qs`: "holds" -- per bracket, whether both wanted ranks lie in it; "candidates" -- the elements of the union of the
    brackets; "capacity" of the candidate buffer; "peak" -- the most candidates one workgroup stages between two flushes (the staging
    buffer holds STAGE_CAP; `flush_every`: steps between two flushes, for asking what another rhythm would stage); "sample" -- the
    valid sampled elements."""
    v = np.ascontiguousarray(np.asarray(values_flat).reshape(-1), dtype=dtype)
    ok = np.asarray(valid_flat).reshape(-1).astype(bool)
    n = v.size
    keys = ordered_keys(v)
    K = keys.dtype.type
    pos = sampled_positions(n)
    sk = np.sort(keys[pos][ok[pos]])
    pk = np.sort(keys[ok])
    m, c = int(sk.size), int(pk.size)
    low = K((1 << (8 * (v.dtype.itemsize - BRACKET_DIGITS))) - 1)   # the open bits: zeros at the low end, ones at the high end
    cand = np.zeros(n, dtype=bool)
    holds = []
    for q in [None] + [float(x) for x in qs]:
        if m:
            lo, hi = rank_pair(m, q)
            h = halfwidth(m)
            klo, khi = K(sk[max(lo - h, 0)] & ~low), K(sk[min(hi + h, m - 1)] | low)
        else:
            klo, khi = K(0), ~K(0)   # (an empty sample: everything is a candidate)
        below, upto = int(np.searchsorted(pk, klo, "left")), int(np.searchsorted(pk, khi, "right"))
        r0, r1 = rank_pair(c, q) if c else (0, -1)
        holds.append(bool(below <= r0 and r1 < upto))
        cand |= ok & (keys >= klo) & (keys <= khi)
    G = min(-(-n // TILE), 2 * n_cu)
    tile = np.flatnonzero(cand) // TILE
    slot = (tile // G // flush_every) * G + tile % G   # (workgroup, group of `flush_every` steps)
    peak = int(np.bincount(slot).max()) if tile.size else 0
    return {"holds": holds, "candidates": int(cand.sum()), "capacity": n // 2 + 4096, "peak": peak, "sample": m}


def predict_rounds(values, inlier_mask, nodata, qs, n_cu: int, flush_every: int = FLUSH_EVERY):
    """predict_round for both rounds of one call: the valid values with `qs`, then |v - median| (formed in the value dtype) alone."""
    v, ok, _, _ = valid_mask(values, inlier_mask, nodata)
    v, ok = v.reshape(-1), ok.reshape(-1)
    first = predict_round(v, ok, qs, v.dtype, n_cu, flush_every)
    if not ok.any():
        return first, predict_round(v, ok, (), v.dtype, n_cu, flush_every)
    T = v.dtype.type
    srt = np.sort(v[ok])
    n = srt.size
    med = T((srt[(n - 1) // 2] + srt[n // 2]) / T(2)) if n % 2 == 0 else srt[n // 2]
    with np.errstate(invalid="ignore", over="ignore"):
        dev = np.abs(v - med)
    return first, predict_round(dev, ok, (), v.dtype, n_cu, flush_every)
