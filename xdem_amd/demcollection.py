"""``xdem.DEMCollection``: a time series of DEMs on one grid -- their differences to a reference DEM, the gap filling of those dDEMs
and the series of mean elevation and volume change (xdem/demcollection.py:34-287).

Upstream loops over the DEMs: one subtraction, one ``hypsometric_interpolation`` of about ten raster passes and one masked
``np.nanmean`` per DEM.  Here the T DEMs are one device-resident stack (``StackPlan``: ``xdemhip_stack`` of include/xdemhip.h,
csrc/demstack.hip) and every step is a constant number of launches whatever T is: one subtraction pass, a batched hypsometric fill
(inlier statistics, one counting sort into (plane, elevation bin) segments with exact medians, one fused fill) and the series sums,
fused into the fill.  The tables of tens of rows per plane stay in pandas / SciPy, through the functions of ``xdem_amd.volume``, so a
filled plane has the bits ``volume.hypsometric_interpolation`` gives for it.

Outlines are ``xdem_amd.Vector`` tables, as upstream takes them, or boolean arrays on the DEMs' grid (or a dict of either by
timestamp).  A Vector is burnt into the grid on the GPU when a mask is first asked for and the mask is kept per (vector, filter, grid);
the union of a start and an end outline is one call (``xdemhip_rasterize_union``).  DEMs on different grids are refused by the
constructor's route (reprojection is geoutils' job); ``DEMCollection.on_reference_grid`` regrids them onto the reference's grid first
(same CRS, ``xdem_amd.reproject``).  A stack of mixed dtypes is float64 throughout.

One quirk of upstream is reproduced on purpose: the constructor sorts ``dems`` by time but leaves ``timestamps`` in the caller's order
(demcollection.py:70-78), so ``reference_timestamp`` and the intervals of the dDEMs index the UNSORTED stamps with SORTED positions.
With stamps in ascending order there is no difference.
"""
from __future__ import annotations

import ctypes
import warnings

import numpy as np
import pandas as pd
import scipy.interpolate

from . import _args, _lib, volume
from ._args import dp, i32p, i64p, is_tensor, ptr
from .ddem import dDEM
from .dem import DEM
from .vector import Vector, union_mask

MAX_PLANES = 1024   # (STK_MAX_PLANES of csrc/demstack.hip)
INPUTS, DDEMS, FILLED = 0, 1, 2


class StackPlan(_lib._Plan):
    """T planes of one grid on the device with the dDEM and filled planes made from them: ``xdemhip_stack`` of include/xdemhip.h."""

    _DESTROY = "xdemhip_stack_destroy"

    def __init__(self, planes, ref_index: int, ctx: _lib.Context | None = None):
        if not 1 <= len(planes) <= MAX_PLANES:
            raise ValueError(f"a stack holds 1 to {MAX_PLANES} DEMs; got {len(planes)}")
        flat = [_args.flat_float(p, "dems") for p in planes]
        self.on_device = is_tensor(flat[0])
        if any(is_tensor(p) != self.on_device for p in flat):
            raise ValueError("the DEMs of a stack must all be host arrays or all be device tensors")
        if any(p.shape != flat[0].shape for p in flat):
            raise ValueError("the DEMs of a stack must have the same number of pixels")
        self.dtype = np.result_type(*[_args.np_dtype(p) for p in flat])   # (what NumPy makes of ref - dem; mixed: float64 throughout)
        if self.on_device:
            import torch

            flat = [p.to(getattr(torch, self.dtype.name)) for p in flat]
        else:
            flat = [p.astype(self.dtype, copy=False) for p in flat]
        self.inputs = flat   # (device planes are used in place: kept alive here)
        self.T, self.n, self.ref_index = len(flat), int(flat[0].shape[0]), int(ref_index)
        self.masks: list = []
        self._start(ctx)

    def _start(self, ctx) -> None:
        self.ctx = ctx or _lib.default_context(self.inputs[0].device.index if self.on_device else None)
        self.space = _args.space(self.inputs[0])
        self._after_torch()
        h = ctypes.c_void_p()
        table = (ctypes.c_void_p * self.T)(*[ptr(p) for p in self.inputs])
        with self.ctx.call_lock:
            self.ctx.check(self.ctx._L.xdemhip_stack_create(self.ctx.handle, table, self.T, _args.code(self.dtype), self.n, self.ref_index,
                                                            self.space, ctypes.byref(h)))
        self.handle = h
        self.ctx.adopt(self)

    def _after_torch(self) -> None:
        """Every pass begins here.  The library launches on its own stream, which does not order against torch's, and what a pass reads
        -- the inputs, the masks, and the dDEM and filled planes, which on the device are the caller's own tensors and may have been
        written to since the last pass -- is made on torch's: wait for it.  The calls themselves return synchronised."""
        if self.on_device:
            _args.synchronize_torch(self.inputs[0])

    def _counts(self):
        return np.empty(self.T, np.int64), np.empty(self.T, np.int64)

    def set_masks(self, masks, mask_ids) -> None:
        """`masks`: distinct boolean arrays / tensors of n pixels; `mask_ids`: per plane the index of its mask, -1 for every pixel."""
        self.masks = [_args.flat_mask(m, self.inputs[0]) for m in masks]   # (device masks are used in place: kept alive here)
        if any(m.shape[0] != self.n for m in self.masks):
            raise ValueError("a mask must have the same number of pixels as the DEMs")
        self.mask_ids = np.ascontiguousarray(mask_ids, dtype=np.int32)
        self._after_torch()   # (the masks' unions, conversions and uploads)
        self._set_masks()

    def _set_masks(self) -> None:
        table = (ctypes.c_void_p * max(1, len(self.masks)))(*[ptr(m) for m in self.masks])
        with self.ctx.call_lock:
            self.ctx.check(self.ctx._L.xdemhip_stack_set_masks(self.handle, table, len(self.masks), i32p(self.mask_ids), self.space))

    def subtract(self, can_equal=None):
        """(pixels that differ from the reference, non-finite dDEM pixels) per plane; planes without a differing pixel are zeroed,
        unless `can_equal` (per plane) rules it out."""
        differ, bad = self._counts()
        flags = np.ones(self.T, np.int32) if can_equal is None else np.ascontiguousarray(can_equal, dtype=np.int32)
        out = self._empty()
        self._after_torch()
        with self.ctx.call_lock:
            self.ctx.check(self.ctx._L.xdemhip_stack_subtract(self.handle, i32p(flags), ptr(out), self.space, i64p(differ), i64p(bad)))
        self._out = {DDEMS: self._frozen(out)}
        return differ, bad

    def inlier_stats(self):
        """(inliers, min, max of the reference over them) per plane; an inlier: inside the plane's mask, dDEM and reference finite."""
        inl = np.empty(self.T, np.int64)
        lo, hi = np.empty(self.T, np.float64), np.empty(self.T, np.float64)
        self._after_torch()
        with self.ctx.call_lock:
            self.ctx.check(self.ctx._L.xdemhip_stack_stats(self.handle, i64p(inl), dp(lo), dp(hi)))
        return inl, lo, hi

    def segments(self, nbs, edges):
        """(counts, medians), each (T, nb_max): plane t's bins 1 .. nbs[t] of np.digitize(ref, edges[t, :nbs[t] + 1])."""
        nbs = np.ascontiguousarray(nbs, dtype=np.int32)
        edges = np.ascontiguousarray(edges, dtype=np.float64).reshape(self.T, -1)
        nb_max = edges.shape[1] - 1
        counts, med = np.empty((self.T, nb_max), np.int64), np.empty((self.T, nb_max), np.float64)
        self._after_torch()
        with self.ctx.call_lock:
            self.ctx.check(self.ctx._L.xdemhip_stack_segments(self.handle, nb_max, i32p(nbs), dp(edges), i64p(counts), dp(med)))
        return counts, med

    def fill(self, ms, xs, ys):
        """The fused fill: plane t's voids inside its mask take its model (ms[t] points of xs[t], ys[t]; 0: none).  Returns the series
        figures of the filled planes over their own masks: (pixels of the mask, finite values, their float64 sum) per plane."""
        ms = np.ascontiguousarray(ms, dtype=np.int32)
        xs = np.ascontiguousarray(xs, dtype=np.float64).reshape(self.T, -1)
        ys = np.ascontiguousarray(ys, dtype=np.float64).reshape(self.T, -1)
        n_mask, n_fin = self._counts()
        sums = np.empty(self.T, np.float64)
        out = self._empty()
        self._after_torch()
        with self.ctx.call_lock:
            self.ctx.check(self.ctx._L.xdemhip_stack_fill(self.handle, xs.shape[1], i32p(ms), dp(xs), dp(ys), ptr(out), self.space, i64p(n_mask),
                                                          i64p(n_fin), dp(sums)))
        self._out[FILLED] = self._frozen(out)
        return n_mask, n_fin, sums

    def series(self, which: int, mask=None):
        """The series figures of the INPUTS, DDEMS or FILLED planes over `mask` (one for all planes), or over every plane's own mask."""
        n_mask, n_fin = self._counts()
        sums = np.empty(self.T, np.float64)
        m = None if mask is None else _args.flat_mask(mask, self.inputs[0])
        if m is not None and m.shape[0] != self.n:
            raise ValueError("a mask must have the same number of pixels as the DEMs")
        self._after_torch()   # (the mask's conversion, and whatever the caller wrote into the planes)
        with self.ctx.call_lock:
            self.ctx.check(self.ctx._L.xdemhip_stack_series(self.handle, int(which), ptr(m), self.space, i64p(n_mask), i64p(n_fin), dp(sums)))
        return n_mask, n_fin, sums

    def _empty(self):
        if self.on_device:
            import torch

            return torch.empty((self.T, self.n), dtype=getattr(torch, self.dtype.name), device=self.inputs[0].device)
        return np.empty((self.T, self.n), self.dtype)

    @staticmethod
    def _frozen(out):
        """A host copy of the stack's planes is read-only: the device keeps computing on its own planes, so a pixel written into the
        copy would be lost on it (a device array IS the stack's plane; to change a dDEM on the host, give it a new array)."""
        if not is_tensor(out):
            out.setflags(write=False)
        return out

    def planes(self, which: int):
        """The T DDEMS or FILLED planes, one (T, n) array / tensor in the inputs' memspace: what ``subtract`` / ``fill`` wrote.  On the
        device these ARE the planes the later passes read (no copy is made)."""
        return self._out[which]


def _raster_like(data, like: DEM) -> DEM:
    """A DEM around `data` as it is (array or tensor, no copy, no nodata pass) on the grid of `like`."""
    dem = DEM.__new__(DEM)
    dem.data, dem.transform, dem.crs, dem.nodata = data, like.transform, like.crs, like.nodata
    return dem


def _address(x) -> tuple:
    return (ptr(x), tuple(x.shape), str(x.dtype))


def _is_outline(x) -> bool:
    return is_tensor(x) or isinstance(x, (np.ndarray, Vector))


def plane_model(counts: np.ndarray, medians: np.ndarray, zbins: np.ndarray, dtype: np.dtype):
    """The model of one plane as ``volume.hypsometric_interpolation`` makes it from the bins' counts and medians: upstream's rotated
    table, ``interpolate_hypsometric_bins``, SciPy's interp1d over the midpoints.  Returns the interpolant's (x, y)."""
    nb = zbins.shape[0] - 1
    values, out_counts = volume._rotated(nb, counts[:nb], medians[:nb], dtype)
    gradient = volume.interpolate_hypsometric_bins(volume._binning_frame(zbins, values, out_counts))
    model = scipy.interpolate.interp1d(gradient.index.mid, gradient["value"].values, fill_value="extrapolate")
    return np.asarray(model.x, np.float64), np.asarray(model.y, np.float64)


class DEMCollection:
    """A temporal collection of DEMs."""

    def __init__(self, dems, timestamps=None, outlines=None, reference_dem=0):
        """`dems`: ``xdem_amd.DEM`` objects on one grid; `timestamps`: one per DEM (default: every DEM's ``datetime`` attribute);
        `outlines`: a Vector or a boolean array on the grid, or a dict of them by timestamp; `reference_dem`: an index into `dems` or one of them."""
        if timestamps is None:
            timestamp_attributes = [getattr(dem, "datetime", None) for dem in dems]
            if any(stamp is None for stamp in timestamp_attributes):
                raise ValueError("Argument `timestamps` not provided and the given DEMs do not all have datetime attributes")
            timestamps = timestamp_attributes
        given = list(dems)
        if not all(isinstance(dem, DEM) for dem in dems):   # (other rasters become DEMs, as upstream makes them: demcollection.py:64-65)
            dems = [DEM.from_array(dem.data, dem.transform, dem.crs, dem.nodata) for dem in dems]
        assert len(dems) == len(timestamps), "The 'dem' and 'timestamps' len differ."
        self.timestamps = np.array(timestamps).astype("datetime64[ns]")
        # the DEMs are sorted by time, the stamps are not (upstream's quirk, see the module's docstring)
        indices = np.argsort(self.timestamps.astype("int64"))
        self.dems = [dems[i] for i in indices]
        self.ddems: list[dDEM] = []
        if isinstance(reference_dem, (int, np.integer)):
            self.reference_index = np.argwhere(indices == reference_dem)[0][0]
        else:
            # one of the rasters as the caller gave them (a raster that was rebuilt as a DEM above is found by what it was)
            found = [k for k, i in enumerate(indices) if given[i] is reference_dem]
            if not found:
                raise ValueError("Argument `reference_dem` must be an index into `dems` or one of the `dems` themselves.")
            self.reference_index = found[0]
        if outlines is None:
            self.outlines: dict = {}
        elif _is_outline(outlines):
            self.outlines = {self.timestamps[self.reference_index]: outlines}
        elif isinstance(outlines, dict) and all(_is_outline(value) for value in outlines.values()):
            self.outlines = dict(zip(np.array(list(outlines.keys())).astype("datetime64[ns]"), outlines.values()))
        else:
            raise ValueError(f"Invalid format on 'outlines': {type(outlines)}, expected one of ['gu.Vector', 'dict[datetime.datetime, gu.Vector']")
        self._plan: StackPlan | None = None
        self._views: dict = {}     # DDEMS / FILLED: the (T, n) planes the dDEMs' arrays are views of
        self._fused = None         # (mask keys, figures) of the last batched fill
        self._burnt: dict = {}     # masks made from Vector outlines, by (vectors, filter, grid, memspace)

    @classmethod
    def on_reference_grid(cls, dems, timestamps=None, outlines=None, reference_dem=0, resampling="cubic_spline") -> "DEMCollection":
        """The collection of `dems` with every DEM that is not on the reference's grid regridded onto it first (``DEM.reproject``, same
        CRS; a ``datetime`` attribute is carried over).  Upstream's ``subtract_dems`` calls ``dem.reproject(resampling=...)`` with no
        target for this; the reference's grid is the evident intent.  ``subtract_dems()`` of the result is the batched pass."""
        dems = list(dems)
        ref = dems[reference_dem] if isinstance(reference_dem, (int, np.integer)) else reference_dem
        ref_grid = (tuple(ref.shape), tuple(float(v) for v in ref.transform))
        on_grid = []
        for dem in dems:
            if dem is not ref and (tuple(dem.shape), tuple(float(v) for v in dem.transform)) != ref_grid:
                if not isinstance(dem, DEM):
                    dem = DEM.from_array(dem.data, dem.transform, dem.crs, dem.nodata)
                moved = dem.reproject(ref, resampling=resampling, silent=True)
                if hasattr(dem, "datetime"):
                    moved.datetime = dem.datetime
                dem = moved
            on_grid.append(dem)
        return cls(on_grid, timestamps=timestamps, outlines=outlines, reference_dem=reference_dem)

    @property
    def reference_dem(self) -> DEM:
        return self.dems[self.reference_index]

    @property
    def reference_timestamp(self) -> np.datetime64:
        return self.timestamps[self.reference_index]

    # ---- subtraction ---------------------------------------------------------------------------------------------------------------
    def subtract_dems(self, resampling_method: str = "cubic_spline") -> list[dDEM]:
        """One dDEM per DEM: ``reference - dem`` in the rasters' dtype, over ``min / max(reference_timestamp, timestamps[i])``.  A DEM
        that equals the reference (the same bits or both NaN at every pixel, the same transform and nodata) gives the all-zero dDEM
        with ``error=0``.  One pass over the stack; `resampling_method` is never used: the DEMs share one grid."""
        ref = self.reference_dem
        shape = tuple(ref.data.shape)
        for dem in self.dems:
            if tuple(dem.data.shape) != shape or dem.transform != ref.transform:
                raise NotImplementedError("all DEMs of a collection must share one grid (reprojection is geoutils' job); "
                                          "DEMCollection.on_reference_grid(...) regrids them within one CRS first.")
        can_equal = [dem.nodata == ref.nodata or (dem.nodata is None and ref.nodata is None) for dem in self.dems]
        if self._plan is not None:
            self._plan.close()
        self._plan = StackPlan([dem.data for dem in self.dems], int(self.reference_index))
        differ, bad = self._plan.subtract(can_equal)
        planes = self._plan.planes(DDEMS)
        self._views, self._fused = {DDEMS: planes}, None
        ddems = []
        for i in range(len(self.dems)):
            raster = _raster_like(planes[i].reshape(shape), ref)
            if differ[i] == 0 and can_equal[i]:
                ddem = dDEM(raster, start_time=self.reference_timestamp, end_time=self.reference_timestamp, error=0)
            else:
                ddem = dDEM(raster, start_time=min(self.reference_timestamp, self.timestamps[i]),
                            end_time=max(self.reference_timestamp, self.timestamps[i]), error=None)
            ddem._known_voids = (ddem.data, bool(bad[i] > 0), getattr(ddem.data, "_version", 0))
            ddems.append(ddem)
        self.ddems = ddems
        return self.ddems

    # ---- masks -----------------------------------------------------------------------------------------------------------------------
    def _mask_parts(self, ddem: dDEM, outlines_filter=None) -> tuple:
        """The outlines whose union is the dDEM's mask, by upstream's four rules; () for the full mask."""
        if not any(ddem is ddem_in_list for ddem_in_list in self.ddems):
            raise ValueError("Given dDEM must be a part of the DEMCollection object.")
        outlines = self.outlines
        all_vectors = bool(outlines) and all(isinstance(value, Vector) for value in outlines.values())
        if outlines_filter is not None and not all_vectors:
            raise NotImplementedError("outlines_filter is a pandas query on a vector's table; the outlines of this class are boolean arrays.")
        if ddem.start_time in outlines and ddem.end_time in outlines:
            if outlines[ddem.start_time] is outlines[ddem.end_time]:   # (the union of an outline with itself)
                parts = (outlines[ddem.start_time],)
            else:
                parts = (outlines[ddem.start_time], outlines[ddem.end_time])
        elif ddem.start_time in outlines:
            parts = (outlines[ddem.start_time],)
        elif len(outlines) == 1:
            parts = (list(outlines.values())[0],)
        else:
            return ()
        if any(isinstance(part, Vector) for part in parts):
            return self._burn_parts(parts, outlines_filter, ddem)
        return parts

    def _burn_parts(self, parts: tuple, outlines_filter, ddem: dDEM) -> tuple:
        """`parts` with their Vectors burnt into the dDEM's grid, in the memspace of its data: two Vectors in one union call.  The masks
        are kept, so a part is the same array every time it is asked for (the plans tell masks apart by address)."""
        grid = (tuple(ddem.data.shape), tuple(self.reference_dem.transform))
        device = is_tensor(ddem.data)
        key = (tuple(id(part) for part in parts), outlines_filter, grid, device)
        if key not in self._burnt:
            chosen = tuple(part.query(outlines_filter) if outlines_filter is not None else part for part in parts)
            if len(chosen) == 2 and all(isinstance(part, Vector) for part in chosen):
                burnt = (union_mask(chosen[0], chosen[1], grid, device=device),)
            else:
                burnt = tuple(part.create_mask(grid, device=device) if isinstance(part, Vector) else part for part in chosen)
            self._burnt[key] = (burnt, parts)   # (the parts are kept alive: their ids are the key)
        return self._burnt[key][0]

    @staticmethod
    def _mask_of(parts: tuple, shape: tuple):
        if len(parts) == 2:
            a, b = parts
            mask = (a.bool() | b.bool()) if is_tensor(a) else np.logical_or(a, b)
        elif len(parts) == 1:
            mask = parts[0]
        else:
            return np.ones(shape=shape, dtype=bool)
        return mask.reshape(shape)

    def get_ddem_mask(self, ddem: dDEM, outlines_filter: str | None = None):
        """The mask of a dDEM of this collection.  In order: outlines for its start and its end time: their union; for its start time
        only: that one; a single outline in all: that one; else every pixel."""
        return self._mask_of(self._mask_parts(ddem, outlines_filter), tuple(ddem.data.shape))

    def _set_plan_masks(self, plan: StackPlan, ddems, outlines_filter=None) -> tuple:
        """The distinct masks of `ddems` handed to `plan`; returns their keys (one per dDEM)."""
        keys = tuple(tuple(_address(p) for p in self._mask_parts(d, outlines_filter)) for d in ddems)
        if getattr(plan, "_mask_keys", None) != keys:
            distinct: dict = {}
            ids = []
            for d, key in zip(ddems, keys):
                if not key:
                    ids.append(-1)
                    continue
                if key not in distinct:
                    distinct[key] = (len(distinct), self._mask_of(self._mask_parts(d, outlines_filter), (plan.n,)))
                ids.append(distinct[key][0])
            plan.set_masks([m for _, m in distinct.values()], ids)
            plan._mask_keys = keys
        return keys

    # ---- gap filling -------------------------------------------------------------------------------------------------------------------
    def _stack_holds(self, which: int, arrays) -> bool:
        planes = self._views.get(which)
        if self._plan is None or planes is None or len(arrays) != planes.shape[0]:
            return False
        return all(a is not None and _address(a.reshape(-1)) == _address(planes[i]) for i, a in enumerate(arrays))

    def interpolate_ddems(self, method: str = "linear") -> list:
        """Fill the voids of every dDEM with `method` (``dDEM.interpolate``; upstream's default is a method it refuses) and return
        the filled arrays.  "regional_hypsometric" fills all dDEMs of ``subtract_dems`` in one batched pass."""
        if method == "regional_hypsometric" and self.ddems and self._stack_holds(DDEMS, [d.data for d in self.ddems]):
            self._fill_stack()
        else:
            for ddem in self.ddems:
                ddem.interpolate(method=method, reference_elevation=self.reference_dem, mask=self.get_ddem_mask(ddem))
        return [ddem.filled_data for ddem in self.ddems]

    @staticmethod
    def _version(planes):
        """What tells that device planes were written to in place: torch's version counter, which a tensor shares with its views (the
        dDEMs' ``filled_data``).  Host planes are read-only.  Sums made before such a write are not reused: the next series reads
        the planes as they are."""
        return planes._version if is_tensor(planes) else 0

    def _fill_stack(self) -> None:
        plan = self._plan
        keys = self._set_plan_masks(plan, self.ddems)
        inliers, lo, hi = plan.inlier_stats()
        dt = plan.dtype
        zbins: list = [None] * plan.T
        for t in range(plan.T):
            if inliers[t] == 0:
                warnings.warn("No valid data found within mask, returning copy", UserWarning)
                continue
            zbins[t] = volume._zbins("fixed", 50.0, dt.type(lo[t]), dt.type(hi[t]), None)
        nbs = np.array([0 if z is None else z.shape[0] - 1 for z in zbins], dtype=np.int32)
        ms = np.zeros(plan.T, np.int32)
        models: list = [None] * plan.T
        if nbs.max() > 0:
            edges = np.full((plan.T, int(nbs.max()) + 1), np.inf)   # (the planes differ in their number of bins: rows padded)
            for t, z in enumerate(zbins):
                if z is not None:
                    edges[t, :z.shape[0]] = np.asarray(z, dtype=np.float64)
            counts, med = plan.segments(nbs, edges)
            for t, z in enumerate(zbins):
                if z is not None:
                    models[t] = plane_model(counts[t], med[t], z, dt)
                    if models[t][0].shape[0] == 1:
                        # inliers within one bin: SciPy's interpolant of one point returns NaN everywhere (a slope of 0 / 0).  The
                        # point twice gives the device the same 0 / 0, and the plane's voids inside the mask become NaN
                        models[t] = tuple(np.repeat(v, 2) for v in models[t])
                    ms[t] = models[t][0].shape[0]
        m_max = max(2, int(ms.max()))
        xs, ys = np.zeros((plan.T, m_max)), np.zeros((plan.T, m_max))
        for t, model in enumerate(models):
            if model is not None:
                xs[t, :ms[t]], ys[t, :ms[t]] = model
        figures = plan.fill(ms, xs, ys)
        filled = plan.planes(FILLED)
        self._views[FILLED] = filled
        self._fused = (keys, figures, self._version(filled))
        for t, ddem in enumerate(self.ddems):
            ddem.filled_data = filled[t]

    # ---- series ------------------------------------------------------------------------------------------------------------------------
    def _series_figures(self, mask, outlines_filter):
        """Per dDEM: (pixels of the mask, finite values inside it, their float64 sum), of its filled data where it has some."""
        if mask is None:
            for ddem in self.ddems:
                self._mask_parts(ddem, outlines_filter)   # (upstream's errors, before anything runs)
        sources = [ddem.data if ddem.filled_data is None else ddem.filled_data for ddem in self.ddems]
        for which in (FILLED, DDEMS):
            if self._stack_holds(which, sources):
                plan = self._plan
                if mask is not None:
                    return plan.series(which, mask)
                keys = self._set_plan_masks(plan, self.ddems, outlines_filter)
                if which == FILLED and self._fused is not None and self._fused[0] == keys and self._fused[2] == self._version(self._views[FILLED]):
                    return self._fused[1]   # (summed in the fill pass, and nothing has written to the filled planes since)
                return plan.series(which)
        # arrays the stack does not hold (dDEMs filled one by one, or set by the caller): a stack of their own
        with StackPlan(sources, 0) as plan:
            if mask is None:
                self._set_plan_masks(plan, self.ddems, outlines_filter)
            return plan.series(INPUTS, mask)

    def get_dh_series(self, outlines_filter: str | None = None, mask=None, nans_ok: bool = False) -> pd.DataFrame:
        """The mean dDEM value ("dh", float64 sum / count in a fixed order) and the mask's area per dDEM other than the reference's own,
        indexed by the dDEMs' intervals.  `mask` overrides the outlines; `nans_ok`: no warning for a dDEM that still has voids."""
        if len(self.ddems) == 0:
            raise ValueError("dDEMs have not yet been calculated.")
        dh_values = pd.DataFrame(columns=["dh", "area"], dtype=float)
        n_mask, n_finite, sums = self._series_figures(mask, outlines_filter)
        res = self.reference_dem.res
        for i, ddem in enumerate(self.ddems):
            if float(ddem.time) == 0:
                continue
            if ddem.filled_data is None and not nans_ok:
                warnings.warn(f"NaNs found in dDEM ({ddem.start_time} - {ddem.end_time}).")
            mean_dh = sums[i] / n_finite[i] if n_finite[i] else np.nan
            area = int(n_mask[i]) * res[0] * res[1]
            dh_values.loc[pd.Interval(pd.Timestamp(ddem.start_time), pd.Timestamp(ddem.end_time))] = mean_dh, area
        return dh_values

    def get_dv_series(self, outlines_filter: str | None = None, mask=None, nans_ok: bool = False) -> pd.Series:
        """The volume change per dDEM: area times mean elevation change."""
        dh_values = self.get_dh_series(outlines_filter=outlines_filter, mask=mask, nans_ok=nans_ok)
        return dh_values["area"] * dh_values["dh"]

    def get_cumulative_series(self, kind: str = "dh", outlines_filter: str | None = None, mask=None, nans_ok: bool = False) -> pd.Series:
        """The cumulative "dh" or "dv" since the first timestamp, indexed by timestamp."""
        if kind.lower() == "dh":
            d_series = self.get_dh_series(mask=mask, outlines_filter=outlines_filter, nans_ok=nans_ok)["dh"]
        elif kind.lower() == "dv":
            d_series = self.get_dv_series(mask=mask, outlines_filter=outlines_filter, nans_ok=nans_ok)
        else:
            raise ValueError("Invalid argument: '{dh=}'. Choices: ['dh', 'dv'].")
        cumulative_dh = pd.Series(dtype=d_series.dtype)
        cumulative_dh[self.reference_timestamp] = 0.0
        for i, value in zip(d_series.index, d_series.values):
            non_reference_year = [date for date in [i.left, i.right] if date != self.reference_timestamp][0]
            cumulative_dh.loc[non_reference_year] = -value
        cumulative_dh.sort_index(inplace=True)
        cumulative_dh -= cumulative_dh.iloc[0]
        return cumulative_dh
