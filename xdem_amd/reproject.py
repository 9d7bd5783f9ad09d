"""Same-CRS regridding on MI355X: the step upstream's entry points begin with, ``geoutils.Raster.reproject`` onto another raster's grid
(``xdem/coreg/base.py:146-156``, ``demcollection.py:128``, ``dem.py:724``, ``ddem.py:198``), for two north-up grids of one CRS.

* ``target_grid`` -- the destination grid of a call: from a reference, a resolution, a grid size and / or bounds.
* ``regrid`` -- the array-level pass (``xdemhip_regrid``, csrc/regrid.hip): host arrays or torch device tensors.
* ``reproject_mask`` -- a boolean mask onto a reference's grid with nearest neighbour (``base.py:146``).
* ``reproject_dem`` -- what ``DEM.reproject`` runs.

The reference's implementation is GDAL's warper through rasterio, which nothing here can run: the resampling rule is written down in
DESIGN.md ("Regridding"), restated in NumPy by tests/reproject_oracle.py and returned bit for bit by the device -- **parity with GDAL
unpinned** (INTEGRATION.md lists the points).  A change of CRS, rotated grids, other resamplings and ``crop`` are not built."""
from __future__ import annotations

import contextlib
import ctypes
import math
import warnings

import numpy as np

from . import _args, _lib

RESAMPLINGS = {"nearest": 0, "bilinear": 1, "cubic": 2, "cubic_spline": 3}   # XDEMHIP_REGRID_* of include/xdemhip.h
ROUTES = {0: "nearest", 1: "tile", 2: "direct"}                              # XDEMHIP_REGRID_ROUTE_* of include/xdemhip_test.h
SAME_GRID = "Output projection, bounds and grid size are identical -> returning self (not a copy!)"


def transform6(transform) -> tuple[float, ...]:
    """``(a, b, c, d, e, f)`` of an affine object or a 6-tuple; only north-up grids (b = d = 0)."""
    t = (transform.a, transform.b, transform.c, transform.d, transform.e, transform.f) if hasattr(transform, "a") else tuple(transform)[:6]
    t = tuple(float(v) for v in t)
    if len(t) != 6:
        raise ValueError("a transform has six coefficients (a, b, c, d, e, f)")
    if t[1] != 0.0 or t[3] != 0.0:
        raise NotImplementedError("only north-up transforms (b = d = 0) are supported: rotated grids are not regridded")
    return t


def resampling_code(resampling) -> int:
    """The kernel of a resampling given by name or by an object with a ``.name`` (rasterio's ``Resampling`` enum)."""
    name = resampling if isinstance(resampling, str) else getattr(resampling, "name", None)
    if not isinstance(name, str):
        raise ValueError(f"resampling must be a name or an object with a .name, got {resampling!r}")
    if name.lower() not in RESAMPLINGS:
        raise NotImplementedError(f"resampling={name!r}: implemented are {sorted(RESAMPLINGS)}")
    return RESAMPLINGS[name.lower()]


def _grid_of(ref) -> tuple[tuple[int, int], tuple[float, ...]]:
    """(shape, transform6) of a reference: an object with ``.shape`` and ``.transform``, or a ``(shape, transform)`` pair."""
    if hasattr(ref, "shape") and hasattr(ref, "transform"):
        shape, transform = ref.shape, ref.transform
    else:
        shape, transform = ref
    shape = tuple(int(v) for v in shape)
    if len(shape) != 2 or min(shape) < 1:
        raise ValueError(f"a grid has a 2-D shape of at least 1 x 1, got {shape}")
    return shape, transform6(transform)


def _bounds4(bounds) -> tuple[float, float, float, float]:
    if hasattr(bounds, "left"):
        return float(bounds.left), float(bounds.bottom), float(bounds.right), float(bounds.top)
    left, bottom, right, top = (float(v) for v in bounds)
    return left, bottom, right, top


def _count(extent: float, res: float) -> int:
    return max(1, int(math.floor(extent / res + 0.5)))


def target_grid(src_shape, src_transform, ref=None, res=None, grid_size=None, bounds=None) -> tuple[tuple[int, int], tuple[float, ...]]:
    """``(shape, transform6)`` of the grid a raster of ``src_shape`` / ``src_transform`` is resampled onto.

    ``ref``: that grid (``.shape`` and ``.transform``, or a ``(shape, transform)`` pair).  ``res`` (scalar or ``(rx, ry)``): the
    upper-left corner is kept and the counts are ``max(1, floor(extent / res + 0.5))``; with ``bounds`` (``left, bottom, right, top``:
    a tuple or an object with those attributes) the extent is the bounds'.  ``grid_size = (w, h)``: the resolution is extent / size.
    ``bounds`` alone keeps the source's resolution."""
    H, W = (int(v) for v in src_shape)
    a, _, c, _, e, f = transform6(src_transform)
    if ref is None and res is None and grid_size is None and bounds is None:
        raise ValueError("one of ref, res, grid_size and bounds must be given")
    if ref is not None:
        if res is not None or grid_size is not None or bounds is not None:
            raise ValueError("ref fixes the whole grid: res, grid_size and bounds cannot be given with it")
        return _grid_of(ref)
    if res is not None and grid_size is not None:
        raise ValueError("res and grid_size cannot both be given")
    if bounds is not None:
        left, bottom, right, top = _bounds4(bounds)
        if not (right > left and top > bottom):
            raise ValueError("bounds must have right > left and top > bottom")
        extent_x, extent_y = right - left, top - bottom
        c, f = (left if a > 0 else right), (top if e < 0 else bottom)
    else:
        extent_x, extent_y = W * abs(a), H * abs(e)
    if grid_size is not None:
        w, h = (int(v) for v in grid_size)
        if w < 1 or h < 1:
            raise ValueError("grid_size must be at least (1, 1)")
        rx, ry = extent_x / w, extent_y / h
    else:
        if res is None:
            rx, ry = abs(a), abs(e)
        else:
            rx, ry = (float(res), float(res)) if np.isscalar(res) else (float(res[0]), float(res[1]))
        if not (rx > 0 and ry > 0):
            raise ValueError("res must be positive")
        w, h = _count(extent_x, rx), _count(extent_y, ry)
    return (h, w), (math.copysign(rx, a), 0.0, c, 0.0, math.copysign(ry, e), f)


def grid_map(src_transform, transform) -> tuple[float, float, float, float]:
    """``(rx, tx, ry, ty)`` of ``xdemhip_regrid``: per axis r = a_d / a_s, t = (c_d - c_s) / a_s, so that the centre of destination
    pixel o lies at u = (o + 0.5) r + t in source pixel units."""
    a_s, _, c_s, _, e_s, f_s = transform6(src_transform)
    a_d, _, c_d, _, e_d, f_d = transform6(transform)
    if a_s == 0 or e_s == 0 or a_d == 0 or e_d == 0:
        raise ValueError("a transform with a zero pixel size")
    m = (a_d / a_s, (c_d - c_s) / a_s, e_d / e_s, (f_d - f_s) / e_s)
    if not (m[0] > 0 and m[2] > 0):
        raise NotImplementedError("the two grids must have the same orientation (pixel sizes of the same sign)")
    return m


def route(src_transform, transform, resampling="bilinear", dtype=np.float32, switch: int = 0) -> tuple[str, int, int]:
    """``(route, LDS bytes of a tile, LDS budget)`` of a call: what ``xdemhip_regrid`` would take under the test switch
    ``"regrid_route" = switch`` -- "nearest", "tile" or "direct" (``xdemhip_regrid_route``, host only)."""
    L = _lib.lib()
    r, nbytes, budget = ctypes.c_int(), ctypes.c_int64(), ctypes.c_int64()
    rc = L.xdemhip_regrid_route(_args.c_doubles(grid_map(src_transform, transform)), resampling_code(resampling), _dtype_code(np.dtype(dtype)),
                                int(switch), ctypes.byref(r), ctypes.byref(nbytes), ctypes.byref(budget))
    if rc != _lib.OK:
        raise ValueError(f"xdemhip_regrid_route refused its arguments (status {rc})")
    return ROUTES[r.value], int(nbytes.value), int(budget.value)


def _dtype_code(dt: np.dtype) -> int:
    return {np.dtype(np.float32): _lib.F32, np.dtype(np.float64): _lib.F64, np.dtype(np.uint8): _lib.U8}[dt]


def regrid(array, src_transform, shape, transform, resampling="bilinear", dtype=None, *, ctx: _lib.Context | None = None,
           return_count: bool = False):
    """``array`` (2-D, on the grid ``src_transform``) resampled onto the grid ``shape`` / ``transform``: one device pass.

    ``array``: a host array (masked cells are NaN; integer rasters other than ``uint8`` / ``bool`` become float32) or a contiguous CUDA
    tensor of float32 / float64 / uint8 / bool; the result is of the same kind, NaN where nothing lands (0 / False for ``uint8`` / ``bool``,
    which take ``"nearest"`` only).  ``resampling``: "nearest", "bilinear", "cubic", "cubic_spline", or an object whose ``.name`` is one
    of them.  ``dtype``: float32 / float64 of the result (default: the input's).  ``return_count``: also the number of pixels that are
    not NaN (``uint8`` / ``bool``: that were taken from inside the source)."""
    kernel = resampling_code(resampling)
    h, w = (int(v) for v in shape)
    if h < 1 or w < 1:
        raise ValueError("the destination grid must be at least 1 x 1")
    m = grid_map(src_transform, transform)
    on_device = _args.is_tensor(array)
    if on_device:
        import torch

        if not (array.is_cuda and array.is_contiguous() and array.dim() == 2 and
                array.dtype in (torch.float32, torch.float64, torch.uint8, torch.bool)):
            raise ValueError("a tensor input must be a contiguous 2-D CUDA tensor of float32, float64, uint8 or bool")
        was_bool = array.dtype == torch.bool
        src = array.view(torch.uint8) if was_bool else array
    else:
        src = _args.nan_filled(array)
        was_bool = src.dtype == np.bool_
        if was_bool:
            src = np.ascontiguousarray(src).view(np.uint8)
        elif src.dtype != np.uint8:
            src = _args.host_float(src)
        src = np.ascontiguousarray(src)
        if src.ndim != 2:
            raise ValueError("array must be 2-D")
    src_dt = _args.np_dtype(src)
    if src_dt == np.uint8:
        if kernel != RESAMPLINGS["nearest"]:
            raise ValueError("uint8 / bool rasters are regridded with resampling=\"nearest\" only")
        if dtype is not None and np.dtype(dtype) not in (np.dtype(np.uint8), np.dtype(np.bool_)):
            raise ValueError("uint8 / bool rasters keep their dtype")
        dst_dt = np.dtype(np.uint8)
    else:
        dst_dt = src_dt if dtype is None else np.dtype(dtype)
        if dst_dt not in _args.FLOATS:
            raise ValueError("dtype must be float32 or float64")
    ctx = ctx or _lib.default_context(array.device.index if on_device else None)
    if on_device:
        dst = torch.empty((h, w), dtype=getattr(torch, dst_dt.name), device=array.device)
    else:
        dst = np.empty((h, w), dtype=dst_dt)
    count = ctypes.c_int64()
    with (_args.torch_stream_scope(ctx, src, reset=True) if on_device else contextlib.nullcontext()):
        ctx.check(ctx._L.xdemhip_regrid(ctx.handle, _args.ptr(src), _dtype_code(src_dt), src.shape[0], src.shape[1], _args.ptr(dst),
                                        _dtype_code(dst_dt), h, w, _args.c_doubles(m), kernel, _args.space(src), ctypes.byref(count)))
    if was_bool:
        dst = dst.view(torch.bool) if on_device else dst.view(np.bool_)
    return (dst, int(count.value)) if return_count else dst


def reproject_mask(mask, src_transform, ref):
    """A boolean mask on the grid ``src_transform`` onto the grid of ``ref`` (``.shape`` / ``.transform`` or a ``(shape, transform)`` pair)
    with nearest neighbour, False where the reference leaves the mask's extent: what upstream does to an inlier mask that is a raster
    (``base.py:146``)."""
    shape, transform = _grid_of(ref)
    data = mask if _args.is_tensor(mask) or isinstance(mask, np.ndarray) else getattr(mask, "data", mask)   # (a raster: its array)
    if _args.is_tensor(data):
        import torch

        data = data if data.dtype == torch.bool else data != 0
        return regrid(data.contiguous(), src_transform, shape, transform, "nearest")
    return regrid(np.asarray(data, dtype=bool), src_transform, shape, transform, "nearest")


def reproject_dem(dem, ref=None, crs=None, res=None, grid_size=None, bounds=None, nodata=None, dtype=None, resampling="bilinear",
                  force_source_nodata=None, silent: bool = False):
    """``DEM.reproject`` (see there)."""
    if crs is not None and crs != dem.crs:
        raise NotImplementedError("a change of CRS is not implemented (it needs pyproj): only same-CRS regridding onto another grid")
    kernel = resampling_code(resampling)   # (refused before anything runs)
    shape, transform = target_grid(dem.shape, dem.transform, ref=ref, res=res, grid_size=grid_size, bounds=bounds)
    src_transform = transform6(dem.transform)
    out_nodata = dem.nodata if nodata is None else nodata
    same_dtype = dtype is None or np.dtype(dtype) == _args.np_dtype(dem.data)
    if tuple(dem.shape) == shape and src_transform == transform and out_nodata == dem.nodata and same_dtype and force_source_nodata is None:
        if not silent:
            warnings.warn(SAME_GRID, UserWarning, stacklevel=3)
        return dem
    data = dem.data
    if force_source_nodata is not None:
        if _args.is_tensor(data):
            import torch

            data = torch.where(data == force_source_nodata, torch.full_like(data, float("nan")), data)
        else:
            data = _args.host_float(data)
            data = np.where(data == force_source_nodata, data.dtype.type(np.nan), data)
    if not _args.is_tensor(data) and kernel != RESAMPLINGS["nearest"]:
        data = _args.host_float(data)   # (an integer DEM is interpolated as float32)
    out = regrid(data, src_transform, shape, transform, resampling, dtype)
    new = type(dem).__new__(type(dem))   # (the array as the pass left it: voids are NaN already, no nodata pass)
    new.data, new.transform, new.crs, new.nodata = out, transform, dem.crs, out_nodata
    return new
