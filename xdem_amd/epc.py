"""Elevation point clouds as inputs of the coregistrations: the container ``EPC`` and the device plan over one raster and one cloud.

Upstream takes a cloud as a GeoDataFrame and asks four things of it (``xdem/coreg/base.py:674-704, 750-764``,
``xdem/coreg/affine.py:198-231``): ``cloud.geometry.x.values``, ``cloud.geometry.y.values``, ``cloud[z_name].values`` and
``cloud.columns``.  ``EPC`` answers exactly those; anything else that does is accepted as a cloud too (duck typing -- geopandas is
never imported).  A plain 1-D array is not a cloud.

``PtsPlan`` is the device side (``xdemhip_pts_plan``, ``csrc/ptsplan.hip``): the validity of every point under the tap rule, the
random subsample by ranks, slope tangent and aspect interpolated at the points, and the evaluations of the three methods that run on
a raster and a cloud -- NuthKaab (``step``), DhMinimize (``shift_nmad``) and VerticalShift (``shift_values`` at zero shift).

Conventions: a point lies at ``(row, col) = ((y - f) / e - 0.5, (x - c) / a - 0.5)`` under the north-up 6-tuple transform (the one of
``xdem_amd.rigid``); ``area_or_point`` is accepted by the callers and not used -- geoutils' ``_interp_points`` is absent, **parity
unpinned**.  Not built: returning a GeoDataFrame, reprojection of the cloud, ``weights``."""
from __future__ import annotations

import ctypes
from typing import Any

import numpy as np

from . import _args, _lib
from ._args import is_tensor
from ._lib import _Plan

NK_NO_MORE_VALID = ("The subsample contains no more valid values. This can happen is the horizontal shift to "
                    "correct is very large, or if the algorithm diverged. To ensure all possible points can "
                    "be used at any iteration step, use subsample=1.")


class _Values:
    """A column as upstream reads it: ``.values``."""

    def __init__(self, values):
        self.values = values


class _Geometry:
    def __init__(self, x, y):
        self.x, self.y = _Values(x), _Values(y)


def _column(v, name: str):
    if is_tensor(v):
        if v.dim() != 1:
            raise ValueError(f"EPC: column '{name}' must be 1-D")
        return v
    v = np.asarray(v)
    if v.ndim != 1:
        raise ValueError(f"EPC: column '{name}' must be 1-D")
    return v


class EPC:
    """An elevation point cloud: three 1-D columns of one length, NumPy arrays or device tensors -- coordinates ``x`` and ``y``
    (float64) and elevations (float64 or a raster's dtype) under the name ``data_column``."""

    def __init__(self, x, y, z, data_column: str = "z") -> None:
        x, y, z = _column(x, "x"), _column(y, "y"), _column(z, data_column)
        if not (len(x) == len(y) == len(z)):
            raise ValueError("EPC: x, y and z must have the same length")
        self.geometry = _Geometry(x, y)
        self.data_column = data_column
        self._data = {data_column: _Values(z)}

    @property
    def columns(self) -> list[str]:
        return [*self._data, "geometry"]

    def __getitem__(self, name: str) -> _Values:
        return self._data[name]

    def __len__(self) -> int:
        return len(self.geometry.x.values)

    @property
    def x(self):
        return self.geometry.x.values

    @property
    def y(self):
        return self.geometry.y.values

    @property
    def z(self):
        return self._data[self.data_column].values

    def __repr__(self) -> str:
        return f"EPC({len(self)} points, data_column={self.data_column!r})"


def is_cloud(obj) -> bool:
    """Whether ``obj`` answers what upstream asks of a GeoDataFrame of points."""
    return hasattr(obj, "geometry") and hasattr(obj, "columns") and hasattr(obj, "__getitem__") and not isinstance(obj, np.ndarray)


def cloud_columns(cloud, z_name: str | None):
    """(x, y, z) of a cloud; ``z_name`` as upstream's ``fit(z_name=...)``: the cloud's own data column when it has one and none is
    named, else ``"z"`` (base.py:2280-2284, same message)."""
    name = z_name if z_name is not None else getattr(cloud, "data_column", "z")
    if name not in cloud.columns:
        raise ValueError(f"Elevation point cloud is missing the column name '{name}' passed to 'z_name'.")   # (base.py:228-232)
    return cloud.geometry.x.values, cloud.geometry.y.values, cloud[name].values


def transform6(transform) -> tuple[float, ...]:
    """The north-up 6-tuple of a raster-point call; ``transform`` is required, as upstream requires it (base.py:204)."""
    if transform is None:
        raise ValueError("'transform' must be given if both DEMs are array-like.")
    t = (transform.a, transform.b, transform.c, transform.d, transform.e, transform.f) if hasattr(transform, "a") else tuple(transform)[:6]
    t = tuple(float(v) for v in t)
    if t[1] != 0.0 or t[3] != 0.0:
        raise NotImplementedError("only north-up transforms (b = d = 0) are supported")
    return t


def split_pair(reference_elev, to_be_aligned_elev):
    """(raster, cloud, pts_is_ref) of a pair of which exactly one is a cloud."""
    return (to_be_aligned_elev, reference_elev, True) if is_cloud(reference_elev) else (reference_elev, to_be_aligned_elev, False)


def _host_raster(raster):
    arr = _args.host_float(raster)
    if arr.ndim != 2:
        raise ValueError("the raster of a raster-point pair must be a 2D array")
    return arr


class PtsPlan(_Plan):
    """Device-resident state of one raster-point fit (``xdemhip_pts_plan``).  ``raster``: a 2-D NumPy array or a contiguous CUDA tensor
    (float32 / float64, kept alive by the plan, never copied); the cloud's columns go where the raster is.  ``with_nk_aux``: slope tangent
    and aspect of the raster take part in the validity and are interpolated at the points (NuthKaab)."""

    _DESTROY = "xdemhip_pts_destroy"

    def __init__(self, raster, x, y, z, transform, pts_is_ref: bool, inlier_mask=None, with_nk_aux: bool = False,
                 ctx: _lib.Context | None = None):
        self.handle = None
        t6 = transform6(transform)
        if is_tensor(raster):
            import torch

            _args.device_float(raster, "a device raster must be a contiguous 2D float32 / float64 CUDA tensor")

            def col(v, dt):
                v = v if is_tensor(v) else torch.from_numpy(np.ascontiguousarray(v))
                return v.to(device=raster.device, dtype=dt).contiguous()

            cols = (col(x, torch.float64), col(y, torch.float64), col(z, raster.dtype))
        else:
            raster = _host_raster(raster)
            host = lambda v: v.cpu().numpy() if is_tensor(v) else v   # noqa: E731
            cols = (np.ascontiguousarray(host(x), dtype=np.float64), np.ascontiguousarray(host(y), dtype=np.float64),
                    np.ascontiguousarray(host(z), dtype=raster.dtype))
        inl = None if inlier_mask is None else _args.mask_u8(inlier_mask, raster)
        if inl is not None and tuple(inl.shape) != tuple(raster.shape):
            raise ValueError("inlier_mask must have the shape of the raster")
        if is_tensor(raster):
            _args.synchronize_torch(raster)
        self._keep = (raster, cols, inl)
        self.dtype = _args.np_dtype(raster)
        space, n_pts, shape = _args.space(raster), int(cols[0].numel() if is_tensor(raster) else cols[0].size), tuple(raster.shape)
        if not (len(cols[0]) == len(cols[1]) == len(cols[2])):
            raise ValueError("the cloud's columns must have one length")
        self.shape, self.n_points, self.pts_is_ref, self.transform6 = shape, n_pts, bool(pts_is_ref), t6
        self.res = (abs(t6[0]), abs(t6[4]))
        self.n_valid = self.n_selected = 0
        self._n_custom_bins = None
        self._bin_callable = None
        if n_pts == 0:   # (an empty cloud has no valid point: the callers raise upstream's message)
            self.ctx = None
            return
        self.ctx = ctx or _lib.default_context()
        self.ctx.adopt(self)
        h, nv = ctypes.c_void_p(), ctypes.c_int64()
        t = np.asarray(t6, dtype=np.float64)
        self.ctx.check(self.ctx._L.xdemhip_pts_create(self.ctx.handle, _args.ptr(raster), _args.ptr(inl), _args.code(raster), shape[0], shape[1],
                                                      _args.dp(t), *(_args.ptr(c) for c in cols), n_pts, int(self.pts_is_ref),
                                                      int(bool(with_nk_aux)), space, ctypes.byref(h), ctypes.byref(nv)))
        self.handle = h
        self.n_valid = self.n_selected = int(nv.value)

    def close(self) -> None:
        if getattr(self, "ctx", None) is not None:
            super().close()

    # ---- selection ----
    def subsample(self, ranks: np.ndarray) -> int:
        """Keep the valid points whose rank (position among the valid points in cloud order) is listed: ``flatnonzero(valid)[ranks]``,
        kept in cloud order (``xdemhip_pts_subsample``).  Returns their number."""
        ranks = np.ascontiguousarray(ranks, dtype=np.int64)
        k = ctypes.c_int64()
        self.ctx.check(self.ctx._L.xdemhip_pts_subsample(self.handle, _args.ptr(ranks), int(ranks.size), _lib.HOST, ctypes.byref(k)))
        self.n_selected = int(k.value)
        return self.n_selected

    def selection(self) -> np.ndarray:
        """Cloud indexes of the selected points, ascending (``xdemhip_pts_selection``)."""
        idx = np.empty(self.n_selected, dtype=np.int64)
        if self.n_selected:
            cnt = ctypes.c_int64()
            self.ctx.check(self.ctx._L.xdemhip_pts_selection(self.handle, _args.ptr(idx), ctypes.byref(cnt)))
        return idx

    # ---- evaluations ----
    def shift_values(self, shift_x: float, shift_y: float, res=None, aux: bool = False):
        """dh of every selected point at the offsets (raster dtype, cloud order, NaN where the point has none); with ``aux`` also
        the slope tangent and aspect columns (``xdemhip_pts_shift_values``).  ``res`` is the raster's own and not read: the signature
        is ``DhPlan.shift_values``'s."""
        k = self.n_selected
        if k == 0:
            raise _lib.XdemHipError("no valid points")
        outs = [np.empty(k, dtype=self.dtype) for _ in range(3 if aux else 1)]
        cnt = ctypes.c_int64()
        ptrs = [_args.ptr(o) for o in outs] + [None] * (3 - len(outs))
        self.ctx.check(self.ctx._L.xdemhip_pts_shift_values(self.handle, float(shift_x), float(shift_y), *ptrs, _lib.HOST, ctypes.byref(cnt)))
        if int(cnt.value) != k:
            raise _lib.XdemHipError(f"xdemhip_pts_shift_values returned {cnt.value} values, expected {k}")
        return tuple(outs) if aux else outs[0]

    def shift_nmad(self, shift_x: float, shift_y: float, res=None, nfact: float = 1.4826) -> tuple[float, float, int]:
        """(median, nmad, count) of dh at the offsets over the selected points, exact (``xdemhip_pts_shift_nmad``: one gather, two
        selections, one fetch).  Raises "no valid points" where no point is left."""
        if self.n_selected == 0:
            raise _lib.XdemHipError("no valid points")
        med, nm, cnt = ctypes.c_double(), ctypes.c_double(), ctypes.c_int64()
        self.ctx.check(self.ctx._L.xdemhip_pts_shift_nmad(self.handle, float(shift_x), float(shift_y), float(nfact), ctypes.byref(med),
                                                          ctypes.byref(nm), ctypes.byref(cnt)))
        return med.value, nm.value, int(cnt.value)

    def set_bin_edges(self, edges) -> None:
        """Explicit aspect-bin edges (``bin_sizes={"aspect": edges}`` upstream); ``None`` restores SciPy's automatic edges."""
        if edges is None:
            self._custom_edges, self._n_custom_bins = None, None
            if self.handle:
                self.ctx.check(self.ctx._L.xdemhip_pts_set_bin_edges(self.handle, None, 0, 0))
            return
        e = np.ascontiguousarray(edges, dtype=np.float64).ravel()
        decimal = int(-np.log10(np.diff(e.astype(self.dtype)).min())) + 6   # SciPy's rightmost-edge rule, from the dtype-cast edges
        self._custom_edges, self._n_custom_bins = e.astype(self.dtype), int(e.size) - 1
        if self.handle:
            self.ctx.check(self.ctx._L.xdemhip_pts_set_bin_edges(self.handle, _args.dp(e), int(e.size), decimal))

    def set_statistic(self, bin_statistic) -> None:
        """Statistic of the aspect bins: ``np.nanmedian`` / ``np.median`` are exact selections on the device; any other callable
        (``np.nanmean`` included) runs on the host per bin over the y column the device hands back, with upstream's arithmetic."""
        is_median = any(bin_statistic is f for f in (np.nanmedian, np.median)) or bin_statistic in ("median", "nanmedian")
        if not is_median and isinstance(bin_statistic, str):
            bin_statistic = {"mean": np.nanmean, "nanmean": np.nanmean}[bin_statistic]
        self._bin_callable = None if is_median else bin_statistic

    def step(self, shift_x: float, shift_y: float, res=None, n_bins: int = 72) -> dict[str, Any]:
        """One Nuth-Kaab iteration at the offsets (georeferenced units; ``res`` is the raster's own and not read): the outputs of
        ``NKPlan.step`` (``xdemhip_pts_nk_step``)."""
        n_bins = self._n_custom_bins or int(n_bins)
        if self._bin_callable is not None:
            return self._step_host(shift_x, shift_y, n_bins, self._bin_callable)
        if self.n_selected == 0:
            raise ValueError(NK_NO_MORE_VALID)
        det = self._device_step(shift_x, shift_y, n_bins)
        # The start of upstream's curve fit is (3 np.nanstd(y) / 2**0.5, 0, np.nanmean(y)) in y's own dtype (affine.py:381-384), and near
        # convergence Levenberg-Marquardt's stopping rule lets a change of one unit in its last place move the fit by 3e-4 pixel
        # (DESIGN.md 5j): the two numbers are NumPy's, over the step's y column, and the arithmetic of `_bin_fit_from_step` on scalars of
        # that dtype is then upstream's.  The float64 sums of the device stay what `_device_step` returns.
        y = self.step_y()
        y = y[~np.isnan(y)]
        det["y_mean"], det["y_std"] = np.nanmean(y), np.nanstd(y)
        return det

    def step_y(self) -> np.ndarray:
        """y = (dh - vshift) / slope_tan of the last step for every selected point (raster dtype, cloud order, NaN where the point had
        no dh): ``xdemhip_pts_step_y``."""
        y = np.empty(self.n_selected, dtype=self.dtype)
        cnt = ctypes.c_int64()
        self.ctx.check(self.ctx._L.xdemhip_pts_step_y(self.handle, _args.ptr(y), _lib.HOST, ctypes.byref(cnt)))
        if int(cnt.value) != y.size:
            raise _lib.XdemHipError(f"xdemhip_pts_step_y returned {cnt.value} values, expected {y.size}")
        return y

    def _device_step(self, shift_x: float, shift_y: float, n_bins: int) -> dict[str, Any]:
        edges = np.empty(n_bins + 1, dtype=np.float64)
        counts = np.empty(n_bins, dtype=np.int64)
        med = np.empty(n_bins, dtype=np.float64)
        vshift, ymean, ystd = ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
        nv = ctypes.c_int64()
        rc = self.ctx._L.xdemhip_pts_nk_step(self.handle, float(shift_x), float(shift_y), n_bins, ctypes.byref(vshift), ctypes.byref(nv),
                                             ctypes.byref(ymean), ctypes.byref(ystd), _args.dp(edges), _args.i64p(counts), _args.dp(med))
        if rc != _lib.OK:
            msg = self.ctx._L.xdemhip_last_error(self.ctx.handle).decode()
            if "no more valid values" in msg:
                raise ValueError(NK_NO_MORE_VALID)
            raise _lib.XdemHipError(f"libxdemhip status {rc}: {msg}")
        return {"vshift": vshift.value, "n_valid": int(nv.value), "y_mean": ymean.value, "y_std": ystd.value,
                "edges": edges, "counts": counts, "medians": med}

    def _y_columns(self, shift_x: float, shift_y: float):
        """(vshift, y, aspect) of the points that have a dh at the offsets, as ``_nuth_kaab_iteration_step`` forms them
        (affine.py:500-518, 381): NumPy in the raster dtype over the columns of ``shift_values``."""
        dh, st, asp = self.shift_values(shift_x, shift_y, aux=True)
        ok = np.isfinite(dh)
        if not ok.any():
            raise ValueError(NK_NO_MORE_VALID)
        vshift = np.nanmedian(dh)
        with np.errstate(divide="ignore", invalid="ignore"):
            y = (dh[ok] - vshift) / st[ok]
        return float(vshift), y, asp[ok]

    def _step_host(self, shift_x: float, shift_y: float, n_bins: int, stat) -> dict[str, Any]:
        """The step under a ``bin_statistic`` other than the median: the callable per bin exactly as ``scipy.stats.binned_statistic``
        calls it upstream (``NKPlan._step_callable``'s host half), over the columns the device hands back."""
        from ._binstat_host import binned_statistic_host

        vshift, y, x = self._y_columns(shift_x, shift_y)
        if self._n_custom_bins:
            edges = self._custom_edges
        else:
            smin, smax = float(x.min()), float(x.max())
            if smin == smax:
                smin, smax = smin - 0.5, smax + 0.5
            edges = np.linspace(smin, smax, n_bins + 1, dtype=x.dtype)
        b = np.digitize(x, edges)
        decimal = int(-np.log10(np.diff(edges).min())) + 6
        b = b - ((x >= edges[-1]) & (np.around(x, decimal) == np.around(edges[-1], decimal))).astype(b.dtype) - 1
        ok = (b >= 0) & (b < n_bins) & np.isfinite(y)
        counts = np.bincount(b[ok], minlength=n_bins).astype(np.int64)
        med = binned_statistic_host(stat, b[ok], y[ok], n_bins)
        return {"vshift": vshift, "n_valid": int(y.size), "y_mean": float(np.nanmean(y)), "y_std": float(np.nanstd(y)),
                "edges": edges.astype(np.float64), "counts": counts, "medians": med}

    def step_fit(self, shift_x: float, shift_y: float, res=None) -> dict[str, Any]:
        """One iteration without binning (``bin_before_fit=False``): the ten least-squares sums of ``NKPlan.step_fit``, formed on the
        host in float64 over the columns the device hands back."""
        vshift, y, x = self._y_columns(shift_x, shift_y)
        y, x = y.astype(np.float64), x.astype(np.float64)
        c, s = np.cos(x), np.sin(x)
        sums = np.array([y.size, c.sum(), s.sum(), (c * c).sum(), (s * s).sum(), (c * s).sum(), y.sum(), (y * c).sum(), (y * s).sum(),
                         (y * y).sum()], dtype=np.float64)
        mean = sums[6] / y.size
        var = sums[9] / y.size - mean * mean
        return {"vshift": vshift, "n_valid": int(y.size), "y_mean": float(mean), "y_std": float(np.sqrt(var)) if var > 0 else 0.0, "sums": sums}


def apply_matrix_pts(x, y, z, matrix, invert: bool = False, centroid=None, ctx: _lib.Context | None = None):
    """``p' = M (p - centroid) + centroid`` for the points of three columns (``_apply_matrix_pts_arr``; ``xdemhip_apply_matrix_pts``):
    float64 NumPy columns out."""
    host = lambda v: v.cpu().numpy() if is_tensor(v) else v   # noqa: E731
    x, y, z = (np.ascontiguousarray(host(v), dtype=np.float64) for v in (x, y, z))
    m = np.ascontiguousarray(matrix, dtype=np.float64)
    if m.shape != (4, 4):
        raise ValueError("matrix must be 4 x 4")
    out = [np.empty_like(x) for _ in range(3)]
    if x.size == 0:
        return tuple(out)
    ctx = ctx or _lib.default_context()
    cen = None if centroid is None else np.ascontiguousarray([float(v) for v in centroid], dtype=np.float64)
    ctx.check(ctx._L.xdemhip_apply_matrix_pts(ctx.handle, *(_args.ptr(v) for v in (x, y, z)), int(x.size), _args.dp(m), _args.dp(cen),
                                              int(bool(invert)), *(_args.ptr(o) for o in out), _lib.HOST))
    return tuple(out)


def apply_matrix_cloud(cloud, matrix, invert: bool = False, centroid=None, z_name: str | None = None) -> EPC:
    """A cloud moved by a 4 x 4 matrix, as an ``EPC`` with the same data column (``_apply_matrix_pts``, base.py:1290-1325)."""
    name = z_name if z_name is not None else getattr(cloud, "data_column", "z")
    x, y, z = cloud_columns(cloud, name)
    return EPC(*apply_matrix_pts(x, y, z, matrix, invert, centroid), data_column=name)
