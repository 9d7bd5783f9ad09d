"""What csrc/volume.hip computes, restated in NumPy: label statistics, np.digitize grouping, per-segment median and standard
deviation, SciPy's linear interp1d in the fill pass and the histogram of calculate_hypsometry_area.  ``OraclePlan`` has the
interface of ``xdem_amd.volume.HypsoPlan``, so the public functions of xdem_amd.volume run on it unchanged (``patched``): pinned
to the reference's fixtures by tests/test_volume_host.py, and the yardstick of the device at shapes without fixtures."""
from __future__ import annotations

import contextlib

import numpy as np

from xdem_amd import volume

LABEL_LIMIT = 1 << 20


def interp1d_linear(xs: np.ndarray, ys: np.ndarray, x: np.ndarray) -> np.ndarray:
    """scipy.interpolate.interp1d(xs, ys, fill_value="extrapolate")._call_linear, in float64."""
    x = np.asarray(x, dtype=np.float64)
    hi = np.clip(np.searchsorted(xs, x), 1, len(xs) - 1)
    lo = hi - 1
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        slope = (ys[hi] - ys[lo]) / (xs[hi] - xs[lo])
        return slope * (x - xs[lo]) + ys[lo]


class OraclePlan:
    def __init__(self, ddem, ref, labels=None, mask=None, ctx=None):
        self.ddem = volume._float_plane(ddem, "ddem")
        self.ref = volume._float_plane(ref, "ref_dem")
        self.labels = None if labels is None else volume._labels_plane(labels, self.ddem)
        self.mask = None if mask is None else volume._mask_plane(mask, self.ddem)
        self.n = self.ddem.shape[0]
        if self.labels is not None:
            self.lab = self.labels
        elif self.mask is not None:
            self.lab = (self.mask != 0).astype(np.int32)
        else:
            self.lab = np.ones(self.n, np.int32)
        self.inlier = (self.lab != 0) & np.isfinite(self.ddem) & np.isfinite(self.ref)
        self._groups = None

    def close(self):
        pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False

    def label_stats(self) -> dict:
        bad = int(np.count_nonzero((self.lab < 0) | (self.lab >= LABEL_LIMIT)))
        if bad:
            raise ValueError(f"glacier_index_map: {bad} labels outside [0, 2^20 = {LABEL_LIMIT})")
        ids = np.unique(self.lab[self.lab != 0]).astype(np.int32)
        ref64, ref_ok = self.ref.astype(np.float64), np.isfinite(self.ref)
        cols = {k: [] for k in ("pixels", "inliers", "ref_min", "ref_max", "inlier_ref_min", "inlier_ref_max")}
        for i in ids:
            sel = self.lab == i
            cols["pixels"].append(np.count_nonzero(sel))
            cols["inliers"].append(np.count_nonzero(sel & self.inlier))
            for name, m in (("ref", sel & ref_ok), ("inlier_ref", sel & self.inlier)):
                cols[name + "_min"].append(ref64[m].min() if m.any() else np.nan)
                cols[name + "_max"].append(ref64[m].max() if m.any() else np.nan)
        out = {k: np.asarray(v, dtype=np.int64 if k in ("pixels", "inliers") else np.float64) for k, v in cols.items()}
        out.update(ids=ids, ref_invalid=int(np.count_nonzero(~ref_ok)))
        return out

    def segments(self, ids, edges, want_std=False):
        ids = np.asarray(ids, dtype=np.int32)
        edges = np.asarray(edges, dtype=np.float64).reshape(len(ids), -1)
        nb = edges.shape[1] - 1
        counts = np.zeros((len(ids), nb), np.int64)
        med = np.full((len(ids), nb), np.nan)
        sd = np.full((len(ids), nb), np.nan) if want_std else None
        self._groups = np.full(self.n, -1, np.int32)
        ref64 = self.ref.astype(np.float64)
        for r, i in enumerate(ids):
            sel = np.flatnonzero((self.lab == i) & self.inlier)
            b = np.digitize(ref64[sel], edges[r])
            keep = (b >= 1) & (b <= nb)
            self._groups[sel[keep]] = r * nb + b[keep] - 1
            for k in range(nb):
                v = self.ddem[sel[b == k + 1]]
                counts[r, k] = v.shape[0]
                if v.shape[0]:
                    med[r, k] = np.median(v)
                    if want_std:
                        v64 = np.sort(v).astype(np.float64)
                        sd[r, k] = np.sqrt(np.mean((v64 - v64.mean()) ** 2))
        return counts, med, sd

    def groups(self):
        return self._groups

    def fill(self, mode, ids, xs, ys, round_to_ref, out_dtype):
        ids = np.asarray(ids, dtype=np.int32)
        out = self.ddem.astype(out_dtype)
        if not len(ids):
            return out
        xs = np.asarray(xs, dtype=np.float64).reshape(len(ids), -1)
        ys = np.asarray(ys, dtype=np.float64).reshape(len(ids), -1)
        for r, i in enumerate(ids):
            sel = self.lab == i
            if mode == 0:
                sel = sel & ~np.isfinite(self.ddem)
            with np.errstate(over="ignore", invalid="ignore"):
                v = interp1d_linear(xs[r], ys[r], self.ref[sel])
                if round_to_ref:
                    v = v.astype(self.ref.dtype)
                out[sel] = v
        return out


def area_counts(ref, timeframe, xs, ys, bins):
    x = ref.astype(np.float64)
    e = x if timeframe == 0 else (x - interp1d_linear(xs, ys, x) if timeframe == 1 else x - interp1d_linear(xs, ys, x) / 2)
    return np.histogram(e, bins=bins)[0].astype(np.int64)


@contextlib.contextmanager
def patched():
    """xdem_amd.volume with its device plan and its area pass replaced by the restatements above."""
    saved = volume.HypsoPlan, volume._area_counts
    volume.HypsoPlan, volume._area_counts = OraclePlan, area_counts
    try:
        yield volume
    finally:
        volume.HypsoPlan, volume._area_counts = saved
