"""Sampling a raster at points on MI355X: ``geoutils.Raster.interp_points`` (``_interp_points``, which calls
``scipy.ndimage.map_coordinates`` on the CPU and refilters the whole raster on every call) and ``Raster.to_pointcloud``
(``xdemhip_spline_prepare`` / ``xdemhip_spline_gather`` / ``xdemhip_raster_points``, csrc/spline.hip; DESIGN.md 5q has the rule).

* ``interp_points`` -- values at ``(x, y)`` for "nearest", "linear", "cubic", "quintic": host arrays or device tensors, the result
  where the points live.
* ``InterpPlan`` -- the prepared raster (nodata spread plane and, for cubic and quintic, the B-spline coefficients) kept on the device:
  ``.at(points)`` as often as an iterative caller needs it, the prefilter paid once.
* ``raster_points`` -- a raster as ``x``, ``y``, ``z`` columns in row-major order (``to_pointcloud``).
* ``plan_constants`` -- the constants of the prefilter (for tests).

The rule is SciPy's: pixel coordinates in float64, order 0 / 1 / 3 / 5 of ``map_coordinates`` on the mirror-extended raster (equal to
its default ``mode="constant"`` for points inside the hull of the pixel centres), NaN outside that hull, nodata spread by the
4-connected ``binary_dilation`` of the non-finite pixels and tested on the bilinear corners.  **Parity unpinned** in three places
(INTEGRATION.md): geoutils is not installed, so its ``_interp_points`` is restated from its source, not run; the voids are filled
from the nearest finite pixel by this project's EDT, whose winner among equally near pixels is not SciPy's (it matters only through
the spline's decaying tail beyond the spreading distance); and points outside the hull are NaN here whatever upstream's edge
handling returns."""
from __future__ import annotations

import ctypes

import numpy as np

from . import _args, _lib

METHODS = {"nearest": 0, "linear": 1, "cubic": 3, "quintic": 5}
ORDERS = (0, 1, 3, 5)


def plan_constants(H: int, W: int, order: int, switch: int = 0) -> dict:
    """The constants the prefilter works with on an ``H x W`` raster under the test switch ``"spline_route" = switch``
    (``xdemhip_spline_plan``, host only): ``band_rows``, ``tile_rows``, ``tile_cols``, ``halo``, ``lds_bytes``."""
    v = [ctypes.c_int() for _ in range(5)]
    rc = _lib.lib().xdemhip_spline_plan(int(H), int(W), int(order), int(switch), *(ctypes.byref(c) for c in v))
    if rc != _lib.OK:
        raise ValueError(f"xdemhip_spline_plan refused its arguments (status {rc})")
    return dict(zip(("band_rows", "tile_rows", "tile_cols", "halo", "lds_bytes"), (int(c.value) for c in v)))


def order_of(method: str) -> int:
    if method not in METHODS:
        raise NotImplementedError(f"method {method!r} is not implemented: one of {tuple(METHODS)} (the interpn-only methods "
                                  "'slinear', 'pchip' and 'splinef2d' stay out)")
    return METHODS[method]


def spread_distance(order: int, dist_nodata_spread="half_order_up") -> int:
    """Pixels of city-block distance the nodata spreads by: ``ceil(order / 2)``, ``floor(order / 2)`` or a non-negative int."""
    if isinstance(dist_nodata_spread, str):
        if dist_nodata_spread == "half_order_up":
            return -(-order // 2)
        if dist_nodata_spread == "half_order_down":
            return order // 2
        raise ValueError("dist_nodata_spread must be 'half_order_up', 'half_order_down' or a non-negative integer")
    if isinstance(dist_nodata_spread, (bool, float)) or int(dist_nodata_spread) != dist_nodata_spread or int(dist_nodata_spread) < 0:
        raise ValueError("dist_nodata_spread must be 'half_order_up', 'half_order_down' or a non-negative integer")
    return int(dist_nodata_spread)


def transform6(transform) -> tuple:
    """``(a, b, c, d, e, f)`` of an affine object or a 6-tuple; only north-up transforms (b = d = 0, a and e non-zero)."""
    t = (transform.a, transform.b, transform.c, transform.d, transform.e, transform.f) if hasattr(transform, "a") else tuple(transform)[:6]
    t = tuple(float(v) for v in t)
    if len(t) != 6:
        raise ValueError("a transform has six coefficients (a, b, c, d, e, f)")
    if t[1] != 0.0 or t[3] != 0.0 or t[0] == 0.0 or t[4] == 0.0:
        raise ValueError("only north-up transforms (b = d = 0, a and e non-zero) are taken: rotated grids stay out")
    return t


def _raster(array):
    """A 2-D float32 / float64 raster where it lives: a contiguous CUDA tensor or a C-contiguous host array (masked cells NaN, other
    dtypes through float32)."""
    if _args.is_tensor(array):
        import torch

        if not array.is_cuda or array.dim() != 2:
            raise ValueError("a tensor raster must be a 2-D CUDA tensor")
        t = array if array.dtype in (torch.float32, torch.float64) else array.to(torch.float32)
        return t.contiguous()
    a = _args.host_float(array)
    if a.ndim == 3 and a.shape[0] == 1:
        a = a[0]
    if a.ndim != 2:
        raise ValueError("the raster must be 2-D")
    return a


def _column(v):
    """A coordinate column as contiguous 1-D float64 where it lives."""
    if _args.is_tensor(v):
        import torch

        if not v.is_cuda or v.dim() != 1:
            raise ValueError("a tensor of coordinates must be a 1-D CUDA tensor")
        return v.to(torch.float64).contiguous()
    a = np.ascontiguousarray(np.asarray(v, dtype=np.float64))
    if a.ndim != 1:
        raise ValueError("coordinates must be 1-D")
    return a


def _points(points):
    from .epc import is_cloud

    if is_cloud(points):
        x, y = points.geometry.x.values, points.geometry.y.values
    else:
        x, y = points
    x = _column(x)
    y = _column(_args.same_space(y, x) if _args.is_tensor(x) != _args.is_tensor(y) else y)
    if len(x) != len(y):
        raise ValueError("x and y must have the same length")
    return x, y


def _empty(n: int, dtype: np.dtype, like):
    if _args.is_tensor(like):
        import torch

        return torch.empty(n, dtype=getattr(torch, dtype.name), device=like.device)
    return np.empty(n, dtype=dtype)


class InterpPlan(_lib._Plan):
    """A raster prepared for sampling (``xdemhip_spline_prepare``): the nodata spread plane and, for orders 3 and 5, the float64
    B-spline coefficients, in device memory the plan owns until ``close``.  For orders 0 and 1 the plan reads the raster itself: a
    device tensor is kept alive by the plan, a host array is copied to the device.  ``n_nonfinite``: the raster's non-finite pixels."""

    _DESTROY = "xdemhip_spline_destroy"

    def __init__(self, array, transform, order: int = 1, dist_nodata_spread="half_order_up", ctx=None) -> None:
        self.handle = None
        if order not in ORDERS:
            raise NotImplementedError(f"order {order!r} is not implemented: one of {ORDERS}")
        self.order = int(order)
        self.dist = spread_distance(self.order, dist_nodata_spread)
        self.transform = transform6(transform)
        raster = _raster(array)
        H, W = (int(v) for v in raster.shape)
        if H < 2 or W < 2:
            raise ValueError(f"axes of length 1 are refused (the raster is {H} x {W})")
        self.shape, self.dtype = (H, W), _args.np_dtype(raster)
        self.ctx = ctx or _lib.default_context(raster.device.index if _args.is_tensor(raster) else None)
        if _args.is_tensor(raster):
            _args.synchronize_torch(raster)
        handle, n = ctypes.c_void_p(), ctypes.c_int64()
        with self.ctx.call_lock:
            self.ctx.check(self.ctx._L.xdemhip_spline_prepare(self.ctx.handle, _args.ptr(raster), _args.code(raster), H, W, self.order, self.dist,
                                                              _args.space(raster), ctypes.byref(handle), ctypes.byref(n)))
        self.handle = handle
        self.n_nonfinite = int(n.value)
        self._raster = raster if _args.is_tensor(raster) and self.order <= 1 else None   # (what the device plan goes on reading)
        self.n_valid = 0
        self.ctx.adopt(self)

    def at(self, points, shift: bool = False, dtype=None):
        """The values at ``points`` = ``(x, y)`` or a cloud, where the points live (``n_valid``: how many are not NaN), in the
        raster's dtype, or with ``dtype=np.float64`` as they are before that one rounding.  ``shift``: the coordinates are on the
        "Point" lattice (``shift_area_or_point``): no half pixel."""
        if not self.handle:
            raise RuntimeError("the plan is closed")
        dt = self.dtype if dtype is None else np.dtype(dtype)
        if dt not in (self.dtype, np.dtype(np.float64)):
            raise ValueError("dtype must be the raster's dtype or float64")
        x, y = _points(points)
        n = len(x)
        out = _empty(n, dt, x)
        if _args.is_tensor(x):
            _args.synchronize_torch(x)
        valid = ctypes.c_int64()
        with self.ctx.call_lock:
            self.ctx.check(self.ctx._L.xdemhip_spline_gather(self.handle, _args.ptr(x), _args.ptr(y), n, _args.c_doubles(self.transform), int(bool(shift)),
                                                             _args.ptr(out), _args.code(dt), _args.space(x), ctypes.byref(valid)))
        self.n_valid = int(valid.value)
        return out

    def planes(self):
        """``(spread, coefficients)`` as host arrays (uint8, float64); None for a plane the plan does not hold."""
        H, W = self.shape
        voids = 0 < self.n_nonfinite < H * W
        spread = np.empty((H, W), np.uint8) if voids else None
        coef = np.empty((H, W), np.float64) if self.order > 1 and self.n_nonfinite < H * W else None
        with self.ctx.call_lock:
            self.ctx.check(self.ctx._L.xdemhip_spline_planes(self.handle, _args.ptr(spread), _args.ptr(coef), _lib.HOST))
        return spread, coef

    def stage_ms(self) -> list:
        """Device time of the stages of the prepare: mask and fill, dilation, column passes, row passes."""
        ms = (ctypes.c_float * 4)()
        self.ctx.check(self.ctx._L.xdemhip_spline_stage_ms(self.handle, ms))
        return [float(v) for v in ms]


def interp_points(array, transform, points, method: str = "linear", area_or_point=None, dist_nodata_spread="half_order_up",
                  shift_area_or_point: bool = False, force_scipy_function=None, ctx=None):
    """geoutils' ``_interp_points``: the raster ``array`` (host array or 2-D CUDA tensor) on the north-up grid ``transform`` sampled
    at ``points`` = ``(x, y)`` (arrays or device tensors; or a cloud).  ``method``: "nearest", "linear", "cubic", "quintic" (orders 0,
    1, 3, 5 of ``map_coordinates``); ``dist_nodata_spread``: "half_order_up", "half_order_down" or pixels; ``shift_area_or_point`` with
    ``area_or_point="Point"`` drops the half-pixel shift; ``force_scipy_function``: None or "map_coordinates".  The values, in the
    raster's floating dtype (integers through float32), where the points live; NaN outside the hull of the pixel centres and
    within the spread of a void."""
    order = order_of(method)
    if force_scipy_function not in (None, "map_coordinates"):
        raise ValueError("force_scipy_function must be None or 'map_coordinates' (scipy.interpolate.interpn is not restated)")
    if area_or_point not in (None, "Area", "Point"):
        raise ValueError("area_or_point must be None, 'Area' or 'Point'")
    shift = bool(shift_area_or_point) and area_or_point == "Point"
    with InterpPlan(array, transform, order, dist_nodata_spread, ctx=ctx) as plan:
        return plan.at(points, shift)


def raster_points(array, transform, skip_nodata: bool = True, ctx=None):
    """``(x, y, z)`` of a raster in row-major order: float64 pixel-centre coordinates and the values in the raster's floating
    dtype, finite pixels only with ``skip_nodata``; host arrays, or device tensors for a CUDA tensor."""
    t6 = transform6(transform)
    raster = _raster(array)
    H, W = (int(v) for v in raster.shape)
    dt = _args.np_dtype(raster)
    ctx = ctx or _lib.default_context(raster.device.index if _args.is_tensor(raster) else None)
    if _args.is_tensor(raster):
        _args.synchronize_torch(raster)
    count = ctypes.c_int64()
    args = (ctx.handle, _args.ptr(raster), _args.code(raster), H, W, _args.c_doubles(t6), int(bool(skip_nodata)))
    with ctx.call_lock:
        ctx.check(ctx._L.xdemhip_raster_points(*args, None, None, None, 0, _args.space(raster), ctypes.byref(count)))
        n = int(count.value)
        x, y, z = _empty(n, np.dtype(np.float64), raster), _empty(n, np.dtype(np.float64), raster), _empty(n, dt, raster)
        if n:
            ctx.check(ctx._L.xdemhip_raster_points(*args, _args.ptr(x), _args.ptr(y), _args.ptr(z), n, _args.space(raster), ctypes.byref(count)))
    return x, y, z


def dem_interp_points(dem, points, method="linear", dist_nodata_spread="half_order_up", band=1, input_latlon=False,
                      shift_area_or_point=False, force_scipy_function=None):
    """``DEM.interp_points``."""
    if band != 1:
        raise ValueError(f"band must be 1: a DEM has a single band (got {band!r})")
    if input_latlon:
        raise NotImplementedError("input_latlon=True needs a transformation between CRSs, which stays out: pass the points in the DEM's CRS")
    return interp_points(dem.data, dem.transform, points, method=method, area_or_point=getattr(dem, "area_or_point", None),
                         dist_nodata_spread=dist_nodata_spread, shift_area_or_point=shift_area_or_point,
                         force_scipy_function=force_scipy_function)


def dem_to_pointcloud(dem, data_column_name="b1", data_band=1, auxiliary_data_bands=None, auxiliary_column_names=None, subsample=1,
                      skip_nodata=True, as_array=False, random_state=None, force_pixel_offset="center"):
    """``DEM.to_pointcloud``."""
    from .epc import EPC

    if data_band != 1:
        raise ValueError(f"data_band must be 1: a DEM has a single band (got {data_band!r})")
    if auxiliary_data_bands is not None:
        raise NotImplementedError("auxiliary_data_bands: a DEM has a single band")
    if auxiliary_column_names is not None:
        raise NotImplementedError("auxiliary_column_names: a DEM has a single band")
    if subsample != 1:
        raise NotImplementedError("subsample other than 1 stays out: subsample the cloud that comes back")
    if force_pixel_offset != "center":
        raise NotImplementedError("force_pixel_offset other than 'center' stays out")
    x, y, z = raster_points(dem.data, dem.transform, skip_nodata=skip_nodata)
    if as_array:
        return np.column_stack([np.asarray(_args.same_space(v, np.empty(0)), dtype=np.float64) for v in (x, y, z)])
    return EPC(x, y, z, data_column=data_column_name)
