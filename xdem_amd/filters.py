"""Raster filters on MI355X: Gaussian, median, mean, minimum, maximum and distance filters of a 2-D raster with voids
(``geoutils.filters`` / ``Raster.filter``, which xDEM shipped as ``xdem/filters.py`` before; on the CPU they are
``scipy.ndimage.gaussian_filter`` and ``generic_filter`` with NumPy's nan-functions) as one LDS-tiled pass of ``xdemhip_filter``
(csrc/filter.hip; include/xdemhip.h has the rules, DESIGN.md 5s the routes, tests/filters_oracle.py their NumPy restatement).

* ``gaussian_filter`` -- SciPy's ``gaussian_filter(mode="reflect")`` bit for bit on a raster without NaN; with NaNs xDEM's normalised
  convolution ``G(a, NaN -> 0) / G(not NaN)``, NaN where the input is.
* ``median_filter`` / ``min_filter`` / ``max_filter`` -- ``generic_filter(np.nanmedian / nanmin / nanmax, size, mode="constant",
  cval=nan)``: the window clipped at the edge, its non-NaN values only, exact at every size.
* ``mean_filter`` -- a square or a disk of integer offsets; the float64 sum in row-major footprint order (NumPy's ``nanmean`` adds
  pairwise and may differ in the last bit).
* ``distance_filter`` -- xDEM's old filter: NaN wherever a pixel is further than ``outlier_threshold`` from the disk mean around it.
* ``filter_array`` / ``filter_dem`` -- the dispatch behind ``DEM.filter``; ``filter_plan`` -- the frame of a call (for tests).

Arrays are 2-D float32 / float64 (other host dtypes and masked arrays become float with NaN), host arrays or contiguous CUDA tensors;
the result has the input's dtype and lives where the input lives.  NaN means missing, +-Inf are ordinary values.  Minimum, maximum and
median order -0.0 below +0.0, which NumPy does not promise.  ``radius`` is in pixels.  **Parity with geoutils unpinned**: geoutils is
not installed next to this project, so the names and defaults of ``geoutils.filters`` / ``Raster.filter`` could not be read; the
names here are xDEM's old ones and SciPy's."""
from __future__ import annotations

import contextlib
import ctypes

import numpy as np

from . import _args, _lib

GAUSSIAN, MEDIAN, MEAN, MIN, MAX, DISTANCE = range(6)
KINDS = {"gaussian": GAUSSIAN, "median": MEDIAN, "mean": MEAN, "min": MIN, "max": MAX, "distance": DISTANCE}
ROUTES = {1: "tile", 2: "global"}
MAX_RADIUS, MAX_LW = 16383, 1 << 20


def filter_plan(H: int, W: int, kind, radius: int, dtype=np.float32, switch: int = 0) -> dict:
    """The frame ``xdemhip_filter`` works with under the test switch ``"filter_route" = switch`` (``xdemhip_filter_plan``, host only):
    ``tile_rows``, ``tile_cols``, ``halo``, ``lds_bytes``, ``lds_budget``, ``route`` ("tile" / "global").  ``radius``: the Gaussian's
    ``lw``, ``size // 2`` of a window, the radius of a disk."""
    i = [ctypes.c_int() for _ in range(3)]
    b = [ctypes.c_int64() for _ in range(2)]
    r = ctypes.c_int()
    rc = _lib.lib().xdemhip_filter_plan(int(H), int(W), KINDS.get(kind, kind), int(radius), _args.code(np.dtype(dtype)), int(switch),
                                        *(ctypes.byref(c) for c in i), *(ctypes.byref(c) for c in b), ctypes.byref(r))
    if rc != _lib.OK:
        raise ValueError(f"xdemhip_filter_plan refused its arguments (status {rc})")
    return {"tile_rows": i[0].value, "tile_cols": i[1].value, "halo": i[2].value, "lds_bytes": b[0].value, "lds_budget": b[1].value,
            "route": ROUTES[r.value]}


def gaussian_radius(sigma: float, truncate: float = 4.0) -> int:
    """SciPy's ``lw = int(truncate * sigma + 0.5)``."""
    return int(float(truncate) * float(sigma) + 0.5)


def gaussian_weights(sigma: float, radius: int) -> np.ndarray:
    """The ``2 radius + 1`` normalised float64 weights, formed as SciPy's ``_gaussian_kernel1d`` forms them (on the host: NumPy's ``exp``
    and NumPy's sum, whose bits the device could not promise)."""
    x = np.arange(-radius, radius + 1)
    phi = np.exp(-0.5 / (float(sigma) * float(sigma)) * x ** 2)
    return phi / phi.sum()


def _plane(array):
    """The raster as the library reads it, where it lives: a contiguous 2-D float32 / float64 host array or CUDA tensor."""
    if _args.is_tensor(array):
        return _args.device_float(array, "a tensor input must be a contiguous 2-D CUDA tensor of float32 or float64")
    a = _args.host_float(array)
    if a.ndim != 2 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError("array must be 2-D and not empty")
    return a


def _odd_size(size) -> int:
    if isinstance(size, bool) or int(size) != size or size < 3 or size % 2 == 0:
        raise ValueError(f"size must be an odd integer >= 3, got {size!r}")
    if size // 2 > MAX_RADIUS:
        raise NotImplementedError(f"size above {2 * MAX_RADIUS + 1} is not supported")
    return int(size)


def _disk_radius(radius) -> int:
    if isinstance(radius, bool) or int(radius) != radius or radius < 0:
        raise ValueError(f"radius must be an integer >= 0 (pixels), got {radius!r}")
    if radius > MAX_RADIUS:
        raise NotImplementedError(f"radius above {MAX_RADIUS} pixels is not supported")
    return int(radius)


def _run(array, kind: int, size: int = 0, radius: int = 0, sigma: float = 0.0, truncate: float = 0.0, weights=None, normalise: int = 0,
         threshold: float = 0.0, ctx: _lib.Context | None = None):
    src = _plane(array)
    on_device = _args.is_tensor(src)
    ctx = ctx or _lib.default_context(src.device.index if on_device else None)
    if on_device:
        import torch

        dst = torch.empty_like(src)
    else:
        dst = np.empty_like(src)
    w = None if weights is None else _args.c_doubles(weights)
    with (_args.torch_stream_scope(ctx, src, reset=True) if on_device else contextlib.nullcontext()):
        ctx.check(ctx._L.xdemhip_filter(ctx.handle, _args.ptr(src), _args.code(src), int(src.shape[0]), int(src.shape[1]), kind, size, radius,
                                        float(sigma), float(truncate), w, normalise, float(threshold), _args.ptr(dst), _args.space(src)))
    return dst


def gaussian_filter(array, sigma, truncate=4.0, normalise="auto", ctx=None):
    """``scipy.ndimage.gaussian_filter(array, sigma, truncate=truncate, mode="reflect")``, axis 0 then axis 1, the axis-0 result
    rounded to the dtype.  ``normalise``: True = the normalised convolution that ignores NaNs (``G(array, NaN -> 0) / G(not NaN)``, NaN
    where the input is NaN); False = SciPy's plain form, in which a NaN spreads over its window; "auto" = True iff the array holds a NaN
    (one counting pass on the device), so that a raster without voids gets SciPy's bits."""
    sigma, truncate = float(sigma), float(truncate)
    if not (np.isfinite(sigma) and sigma > 0):
        raise ValueError(f"sigma must be finite and > 0, got {sigma!r}")
    if not (np.isfinite(truncate) and truncate >= 0):
        raise ValueError(f"truncate must be finite and >= 0, got {truncate!r}")
    if not (normalise == "auto" or isinstance(normalise, (bool, np.bool_))):
        raise ValueError(f"normalise must be True, False or \"auto\", got {normalise!r}")
    if truncate * sigma + 0.5 >= MAX_LW + 1:
        raise NotImplementedError(f"more than {MAX_LW} taps on a side (truncate * sigma) are not supported")
    lw = gaussian_radius(sigma, truncate)
    return _run(array, GAUSSIAN, radius=lw, sigma=sigma, truncate=truncate, weights=gaussian_weights(sigma, lw),
                normalise=2 if isinstance(normalise, str) else int(bool(normalise)), ctx=ctx)


def median_filter(array, size, ctx=None):
    """The median of the non-NaN values of the ``size x size`` window (odd, >= 3) clipped at the raster's edge, whether or not the
    centre is NaN; an even count gives the float64 mean of the two middle values rounded once; NaN for a window without a value."""
    return _run(array, MEDIAN, size=_odd_size(size), ctx=ctx)


def min_filter(array, size, ctx=None):
    """The smallest non-NaN value of the ``size x size`` window clipped at the edge; NaN for a window without a value."""
    return _run(array, MIN, size=_odd_size(size), ctx=ctx)


def max_filter(array, size, ctx=None):
    """The largest non-NaN value of the ``size x size`` window clipped at the edge; NaN for a window without a value."""
    return _run(array, MAX, size=_odd_size(size), ctx=ctx)


def mean_filter(array, size=None, radius=None, ctx=None):
    """The mean of the non-NaN values of a footprint clipped at the edge: the square ``size x size`` (odd, >= 3) or the disk
    ``dy^2 + dx^2 <= radius^2`` of integer pixel offsets; the float64 sum in row-major footprint order divided by the count, rounded once."""
    if (size is None) == (radius is None):
        raise ValueError("mean_filter takes exactly one of size and radius")
    if size is not None:
        return _run(array, MEAN, size=_odd_size(size), ctx=ctx)
    return _run(array, MEAN, radius=_disk_radius(radius), ctx=ctx)


def distance_filter(array, radius, outlier_threshold, ctx=None):
    """``array`` with NaN wherever ``|array - m| > outlier_threshold``, ``m`` the unrounded float64 mean of the disk of ``radius``
    pixels around the pixel, the pixel included (xDEM's old ``distance_filter``); one fused pass."""
    thr = float(outlier_threshold)
    if np.isnan(thr):
        raise ValueError("outlier_threshold must not be NaN")
    return _run(array, DISTANCE, radius=_disk_radius(radius), threshold=thr, ctx=ctx)


_FUNCTIONS = {"gaussian": gaussian_filter, "median": median_filter, "mean": mean_filter, "min": min_filter, "max": max_filter,
              "distance": distance_filter}


def filter_array(array, method, **kwargs):
    """``array`` through the filter ``method``: one of "gaussian", "median", "mean", "min", "max", "distance" with that function's
    keywords, or a callable that takes and returns an array of the same shape."""
    if callable(method):
        out = method(array, **kwargs)
        if tuple(getattr(out, "shape", ())) != tuple(array.shape):
            raise ValueError("a filter callable must return an array of the input's shape")
        return out
    if method not in _FUNCTIONS:
        raise ValueError(f"method must be one of {tuple(_FUNCTIONS)} or a callable, got {method!r}")
    return _FUNCTIONS[method](array, **kwargs)


def filter_dem(dem, method, inplace: bool = False, **kwargs):
    """``DEM.filter`` (see there)."""
    data = dem.data
    if not _args.is_tensor(data):
        data = _args.host_float(data)   # (an integer DEM is filtered as float32; voids are NaN already)
    out = filter_array(data, method, **kwargs)
    if inplace:
        new = dem
    else:
        new = type(dem).__new__(type(dem))   # (the array as the pass left it: voids are NaN already, no nodata pass)
        new.__dict__ = dict(dem.__dict__)
    new.data = out
    for name, cleared in (("_filled_data", None), ("_fill_method", ""), ("_known_voids", None)):   # (a dDEM's caches describe the old data)
        if name in new.__dict__:
            new.__dict__[name] = cleared
    return None if inplace else new
