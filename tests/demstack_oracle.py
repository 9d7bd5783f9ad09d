"""CPU oracle of the DEM stack -- TEST INFRASTRUCTURE, NOT PRODUCT CODE (NumPy, own code).

``OracleStack`` restates the passes of ``csrc/demstack.hip`` behind the interface of ``xdem_amd.demcollection.StackPlan``, so that the
product's own host code (the collection, the dDEMs, the per-plane tables, the series) runs on it without a GPU (``patched``), and is
the yardstick of the device.  The subtraction is NumPy's, the equality test compares bits, the medians are ``np.median`` per
(plane, bin), the model is ``volume_oracle.interp1d_linear`` rounded to the dtype, the sums are ``math.fsum`` (exactly rounded)."""
from __future__ import annotations

import contextlib
import math

import numpy as np

import volume_oracle
from xdem_amd import demcollection
from xdem_amd.demcollection import DDEMS, FILLED, INPUTS


class OracleStack(demcollection.StackPlan):
    """``StackPlan`` with NumPy in place of the device: same constructor, same methods."""

    def _start(self, ctx) -> None:
        self.handle, self.ctx = None, None
        self.mask_ids = np.full(self.T, -1, np.int32)
        self._planes: dict = {INPUTS: np.stack(self.inputs)}

    def close(self) -> None:
        pass

    def _set_masks(self) -> None:
        pass

    def mask_of(self, t: int) -> np.ndarray:
        return np.ones(self.n, bool) if self.mask_ids[t] < 0 else self.masks[self.mask_ids[t]].astype(bool)

    def subtract(self, can_equal=None):
        bits = np.uint32 if self.dtype == np.float32 else np.uint64
        ref = self.inputs[self.ref_index]
        differ, bad = self._counts()
        out = np.empty((self.T, self.n), self.dtype)
        for t, d in enumerate(self.inputs):
            with np.errstate(invalid="ignore", over="ignore"):
                out[t] = ref - d
            differ[t] = np.count_nonzero(~((ref.view(bits) == d.view(bits)) | (np.isnan(ref) & np.isnan(d))))
            if differ[t] == 0 and (can_equal is None or can_equal[t]):
                out[t] = 0
            bad[t] = np.count_nonzero(~np.isfinite(out[t]))
        self._planes[DDEMS] = out
        self._planes.pop(FILLED, None)
        return differ, bad

    def inliers(self, t: int) -> np.ndarray:
        return self.mask_of(t) & np.isfinite(self._planes[DDEMS][t]) & np.isfinite(self.inputs[self.ref_index])

    def inlier_stats(self):
        ref64 = self.inputs[self.ref_index].astype(np.float64)
        inl = np.zeros(self.T, np.int64)
        lo, hi = np.full(self.T, np.nan), np.full(self.T, np.nan)
        for t in range(self.T):
            sel = self.inliers(t)
            inl[t] = np.count_nonzero(sel)
            if inl[t]:
                lo[t], hi[t] = ref64[sel].min(), ref64[sel].max()
        return inl, lo, hi

    def segments(self, nbs, edges):
        edges = np.asarray(edges, dtype=np.float64).reshape(self.T, -1)
        nb_max = edges.shape[1] - 1
        counts = np.zeros((self.T, nb_max), np.int64)
        med = np.full((self.T, nb_max), np.nan)
        ref64 = self.inputs[self.ref_index].astype(np.float64)
        for t in range(self.T):
            if nbs[t] == 0:
                continue
            sel = np.flatnonzero(self.inliers(t))
            b = np.digitize(ref64[sel], edges[t, :nbs[t] + 1])
            for k in range(nbs[t]):
                v = self._planes[DDEMS][t][sel[b == k + 1]]
                counts[t, k] = v.shape[0]
                if v.shape[0]:
                    med[t, k] = np.median(v)
        return counts, med

    def fill(self, ms, xs, ys):
        xs = np.asarray(xs, dtype=np.float64).reshape(self.T, -1)
        ys = np.asarray(ys, dtype=np.float64).reshape(self.T, -1)
        out = self._planes[DDEMS].copy()
        ref = self.inputs[self.ref_index]
        for t in range(self.T):
            if ms[t] >= 2:
                sel = self.mask_of(t) & ~np.isfinite(out[t])
                with np.errstate(over="ignore", invalid="ignore"):
                    out[t][sel] = volume_oracle.interp1d_linear(xs[t, :ms[t]], ys[t, :ms[t]], ref[sel]).astype(self.dtype)
        self._planes[FILLED] = out
        return self.series(FILLED)

    def series(self, which: int, mask=None):
        n_mask, n_fin = self._counts()
        sums = np.zeros(self.T, np.float64)
        for t in range(self.T):
            m = self.mask_of(t) if mask is None else np.asarray(mask).reshape(-1).astype(bool)
            v = self._planes[which][t][m]
            v = v[np.isfinite(v)].astype(np.float64)
            n_mask[t], n_fin[t], sums[t] = np.count_nonzero(m), v.shape[0], math.fsum(v)
        return n_mask, n_fin, sums

    def planes(self, which: int):
        return self._planes[which]


@contextlib.contextmanager
def patched():
    """xdem_amd.demcollection with its device stack, and xdem_amd.volume with its device plan, replaced by the restatements."""
    saved = demcollection.StackPlan
    demcollection.StackPlan = OracleStack
    try:
        with volume_oracle.patched():
            yield demcollection
    finally:
        demcollection.StackPlan = saved
