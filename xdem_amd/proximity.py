"""Proximity on MI355X: the distance of every pixel to the nearest target pixel or outline (``geoutils.Raster.proximity``, which
computes it with ``scipy.ndimage.distance_transform_edt`` on the CPU) as an exact Euclidean distance transform on the GPU
(``xdemhip_edt``, csrc/edt.hip; DESIGN.md 5p has the rule).

* ``distance_transform_edt`` -- SciPy's call for 2-D inputs: host arrays or torch device tensors, the result where the input lives.
* ``proximity`` -- ``Raster.proximity``: targets from the raster's own pixels, or from a ``Vector`` burnt on the GPU.
* ``edt`` / ``target_plane`` / ``inner_boundary`` -- the array-level passes; ``edt_plan`` -- the constants of a call (for tests).

The distance is the true float64 minimum of SciPy's own expression ``(dy * sy)**2 + (dx * sx)**2`` over all targets; where SciPy's
parabola intersections leave that minimum (inexact samplings) the two differ and SciPy is the larger.  Ties between targets are
broken by a rule of this project's own (smaller column distance, then smaller column, then nearer and upper row), not SciPy's.
**Parity with geoutils unpinned** in two places: geoutils burns the boundary as GDAL lines and buffers a geometry
with shapely; here the boundary is the inner boundary of the burnt mask and a buffer is a distance between pixel centres."""
from __future__ import annotations

import contextlib
import ctypes

import numpy as np

from . import _args, _lib

GEOMETRY_TYPES = ("boundary", "polygon")
IN_OR_OUT = ("in", "out", "both")
DISTANCE_UNITS = ("pixel", "georeferenced")
MAX_TARGET_VALUES = 64


def edt_plan(H: int, W: int, switch: int = 0) -> dict:
    """The constants ``xdemhip_edt`` works with on an ``H x W`` plane under the test switch ``"edt_route" = switch``
    (``xdemhip_edt_plan``, host only): ``band_rows``, ``tile_cols``, ``halo``, ``block_cols``, ``offset_bytes``."""
    v = [ctypes.c_int() for _ in range(5)]
    rc = _lib.lib().xdemhip_edt_plan(int(H), int(W), int(switch), *(ctypes.byref(c) for c in v))
    if rc != _lib.OK:
        raise ValueError(f"xdemhip_edt_plan refused its arguments (status {rc})")
    return dict(zip(("band_rows", "tile_cols", "halo", "block_cols", "offset_bytes"), (int(c.value) for c in v)))


def sampling_pair(sampling) -> tuple[float, float]:
    """``(sy, sx)`` of a scalar, a pair or None (1, 1): finite and positive."""
    if sampling is None:
        sy = sx = 1.0
    elif np.ndim(sampling) == 0:
        sy = sx = float(sampling)
    else:
        s = tuple(float(v) for v in sampling)
        if len(s) != 2:
            raise ValueError("sampling is a scalar or a pair (rows, columns)")
        sy, sx = s
    if not (np.isfinite(sy) and np.isfinite(sx) and sy > 0 and sx > 0):
        raise ValueError("sampling must be finite and positive")
    return sy, sx


def sampling_of(transform, distance_unit: str = "georeferenced") -> tuple[float, float]:
    """``(sy, sx)`` of a grid: (1, 1) for "pixel", ``(|e|, |a|)`` of its north-up transform for "georeferenced"."""
    if distance_unit not in DISTANCE_UNITS:
        raise ValueError(f"distance_unit must be one of {DISTANCE_UNITS}, got {distance_unit!r}")
    if distance_unit == "pixel":
        return 1.0, 1.0
    from .reproject import transform6

    a, _, _, _, e, _ = transform6(transform)
    return sampling_pair((abs(e), abs(a)))


def _dist_code(dtype) -> tuple[np.dtype, int]:
    dt = np.dtype(dtype)
    if dt not in _args.FLOATS:
        raise ValueError("dtype must be float32 or float64")
    return dt, _args.code(dt)


def _u8(plane, what: str):
    """A 2-D mask or byte plane as contiguous uint8 where it lives (bool is viewed, not copied)."""
    if _args.is_tensor(plane):
        import torch

        if not (plane.is_cuda and plane.dim() == 2 and plane.dtype in (torch.uint8, torch.bool)):
            raise ValueError(f"{what}: a tensor must be a 2-D CUDA tensor of uint8 or bool")
        plane = plane.contiguous()
        return plane.view(torch.uint8) if plane.dtype == torch.bool else plane
    a = np.asarray(plane)
    if a.ndim != 2 or a.dtype not in (np.dtype(np.uint8), np.dtype(np.bool_)):
        raise ValueError(f"{what}: an array must be 2-D of uint8 or bool")
    a = np.ascontiguousarray(a)
    return a.view(np.uint8) if a.dtype == np.bool_ else a


def _empty(shape, dtype: np.dtype, like, ctx):
    if _args.is_tensor(like):
        import torch

        return torch.empty(shape, dtype=getattr(torch, dtype.name), device=like.device)
    return np.empty(shape, dtype=dtype)


def _scope(ctx, x):
    return _args.torch_stream_scope(ctx, x, reset=True) if _args.is_tensor(x) else contextlib.nullcontext()


class DeviceEngine:
    """The binding of ``xdemhip_edt``, ``xdemhip_edt_targets`` and ``xdemhip_mask_boundary``.  ``tests/proximity_oracle.OracleEngine`` has
    the same methods and stands in for it where no GPU is at hand.  ``on_device``: outlines are burnt into device memory."""

    on_device = True

    def edt(self, targets, sampling, dtype=np.float64, return_distances=True, return_indices=False, keep=None, keep_polarity=1, ctx=None):
        """``(distances or None, indices or None, number of targets)`` of a uint8 / bool target plane."""
        tg = _u8(targets, "targets")
        sy, sx = sampling_pair(sampling)
        dt, code = _dist_code(dtype)
        kp = None if keep is None else _u8(_args.same_space(keep, tg), "keep")
        if kp is not None and tuple(kp.shape) != tuple(tg.shape):
            raise ValueError("keep must have the shape of the target plane")
        H, W = (int(v) for v in tg.shape)
        ctx = ctx or _lib.default_context(tg.device.index if _args.is_tensor(tg) else None)
        dist = _empty((H, W), dt, tg, ctx) if return_distances else None
        idx = _empty((2, H, W), np.dtype(np.int32), tg, ctx) if return_indices else None
        n = ctypes.c_int64()
        with _scope(ctx, tg):
            ctx.check(ctx._L.xdemhip_edt(ctx.handle, _args.ptr(tg), H, W, sy, sx, _args.ptr(dist), code, _args.ptr(idx), _args.ptr(kp),
                                         int(bool(keep_polarity)), _args.space(tg), ctypes.byref(n)))
        return dist, idx, int(n.value)

    def targets(self, raster, values=None, ctx=None):
        """The uint8 target plane of a raster: finite and non-zero pixels, or those equal to one of ``values`` (NaN never)."""
        vals = np.zeros(0) if values is None else np.atleast_1d(np.asarray(values, dtype=np.float64)).ravel()
        if vals.size > MAX_TARGET_VALUES:
            raise ValueError(f"at most {MAX_TARGET_VALUES} target values, got {vals.size}")
        if values is not None and vals.size == 0:
            raise ValueError("target_values is empty")
        if _args.is_tensor(raster):
            import torch

            if not raster.is_cuda or raster.dim() != 2:
                raise ValueError("a tensor raster must be a 2-D CUDA tensor")
            src = raster.contiguous()
            if src.dtype == torch.bool:
                src = src.view(torch.uint8)
            elif src.dtype not in (torch.float32, torch.float64, torch.uint8, torch.int32):
                src = src.to(torch.float64)
        else:
            src = _args.nan_filled(raster)
            if src.ndim != 2:
                raise ValueError("the raster must be 2-D")
            if src.dtype == np.bool_:
                src = np.ascontiguousarray(src).view(np.uint8)
            elif src.dtype not in (np.dtype(np.float32), np.dtype(np.float64), np.dtype(np.uint8), np.dtype(np.int32)):
                src = src.astype(np.float32 if src.dtype == np.float16 else np.float64)
            src = np.ascontiguousarray(src)
        code = {"float32": _lib.F32, "float64": _lib.F64, "uint8": _lib.U8, "int32": _lib.I32}[_args.np_dtype(src).name]
        ctx = ctx or _lib.default_context(src.device.index if _args.is_tensor(src) else None)
        out = _empty(tuple(src.shape), np.dtype(np.uint8), src, ctx)
        with _scope(ctx, src):
            ctx.check(ctx._L.xdemhip_edt_targets(ctx.handle, _args.ptr(src), code, int(np.prod(src.shape)), _args.c_doubles(vals) if vals.size else None,
                                                 int(vals.size), _args.ptr(out), _args.space(src)))
        return out

    def boundary(self, mask, ctx=None):
        """The inner boundary of a mask as a uint8 plane: mask pixels with a 4-neighbour inside the raster that is not in the mask."""
        m = _u8(mask, "mask")
        ctx = ctx or _lib.default_context(m.device.index if _args.is_tensor(m) else None)
        out = _empty(tuple(m.shape), np.dtype(np.uint8), m, ctx)
        with _scope(ctx, m):
            ctx.check(ctx._L.xdemhip_mask_boundary(ctx.handle, _args.ptr(m), int(m.shape[0]), int(m.shape[1]), _args.ptr(out), _args.space(m)))
        return out

    @staticmethod
    def stage_ms(ctx=None) -> list:
        """Device time of the four passes (down, carry, up, row) of the last ``xdemhip_edt`` call on the context."""
        ctx = ctx or _lib.default_context()
        ms = (ctypes.c_float * 4)()
        ctx.check(ctx._L.xdemhip_edt_stage_ms(ctx.handle, ms))
        return [float(v) for v in ms]


_ENGINE = DeviceEngine()   # (a test puts its oracle here)


def edt(targets, sampling=None, dtype=np.float64, return_distances=True, return_indices=False, keep=None, keep_polarity=1, ctx=None):
    """Distances to, and indices of, the nearest non-zero pixel of the uint8 / bool plane ``targets``: ``(distances or None, int32
    [2, H, W] indices or None, number of targets)``.  ``keep`` (a mask): the distance is 0 where ``bool(keep) != bool(keep_polarity)``."""
    kw = {} if ctx is None else {"ctx": ctx}
    return _ENGINE.edt(targets, sampling, dtype, return_distances, return_indices, keep, keep_polarity, **kw)


def target_plane(raster, target_values=None, ctx=None):
    kw = {} if ctx is None else {"ctx": ctx}
    return _ENGINE.targets(raster, target_values, **kw)


def inner_boundary(mask, ctx=None):
    kw = {} if ctx is None else {"ctx": ctx}
    return _ENGINE.boundary(mask, **kw)


def distance_transform_edt(input, sampling=None, return_distances=True, return_indices=False, dtype=np.float64, ctx=None):
    """``scipy.ndimage.distance_transform_edt`` for 2-D inputs: non-zero pixels (NaN among them) get the distance to the nearest zero
    pixel, zero pixels 0; ``return_indices``: the int32 ``[2, H, W]`` row and column of that pixel.  A plane without a zero is
    ``+inf`` with indices -1 (SciPy returns garbage there).  ``input``: a host array or a 2-D CUDA tensor; the result lives where it
    does.  ``dtype``: float32 / float64 of the distances."""
    if not return_distances and not return_indices:
        raise RuntimeError("at least one of return_distances/return_indices must be True")
    zeros = target_plane(input, [0.0], ctx=ctx)
    dist, idx, _ = edt(zeros, sampling, dtype, return_distances, return_indices, ctx=ctx)
    if return_distances and return_indices:
        return dist, idx
    return dist if return_distances else idx


def check_keywords(geometry_type="boundary", in_or_out="both", distance_unit="georeferenced") -> None:
    if geometry_type not in GEOMETRY_TYPES:
        raise ValueError(f"geometry_type must be one of {GEOMETRY_TYPES}, got {geometry_type!r}")
    if in_or_out not in IN_OR_OUT:
        raise ValueError(f"in_or_out must be one of {IN_OR_OUT}, got {in_or_out!r}")
    if distance_unit not in DISTANCE_UNITS:
        raise ValueError(f"distance_unit must be one of {DISTANCE_UNITS}, got {distance_unit!r}")


def proximity_array(data, transform, vector=None, target_values=None, geometry_type="boundary", in_or_out="both",
                    distance_unit="georeferenced", dtype=np.float32):
    """The plane ``proximity`` returns, for the raster ``data`` (host array or device tensor; only its shape is read when a vector is
    given) on the grid ``transform``.  With a vector the plane is a device tensor when ``data`` is one, else a host array."""
    check_keywords(geometry_type, in_or_out, distance_unit)
    from .vector import grid_of

    shape, t6 = grid_of((tuple(data.shape), transform))   # (rotated grids: the north-up NotImplementedError)
    sampling = sampling_of(t6, distance_unit)
    _dist_code(dtype)
    if vector is None:
        return edt(target_plane(data, target_values), sampling, dtype)[0]
    mask = vector.create_mask((shape, t6), device=_ENGINE.on_device)
    targets = mask if geometry_type == "polygon" else inner_boundary(mask)
    keep = None if in_or_out == "both" else mask
    out = edt(targets, sampling, dtype, keep=keep, keep_polarity=1 if in_or_out == "in" else 0)[0]
    return _args.same_space(out, data) if _args.is_tensor(data) or isinstance(data, np.ndarray) else out


def proximity(raster, vector=None, target_values=None, geometry_type="boundary", in_or_out="both", distance_unit="georeferenced",
              dtype=np.float32):
    """``geoutils.Raster.proximity``: a raster on the grid and CRS of ``raster`` (no nodata) with every pixel's distance to the nearest
    target.  Without ``vector`` the targets are the non-zero finite pixels of ``raster``, or those equal to one of up to 64
    ``target_values``; ``geometry_type`` and ``in_or_out`` are ignored then.  With an ``xdem_amd.Vector`` its outlines are burnt on the
    GPU: ``geometry_type="polygon"`` makes the mask pixels the targets, ``"boundary"`` the inner boundary of the mask; ``in_or_out``
    = "in" / "out" / "both" keeps the distances inside the mask / outside it / everywhere, the rest is 0.  ``distance_unit``: "pixel"
    (sampling 1) or "georeferenced" (the pixel sizes of the north-up transform).  ``dtype``: float32 / float64."""
    from .ddem import raster_of

    out = proximity_array(raster.data, raster.transform, vector, target_values, geometry_type, in_or_out, distance_unit, dtype)
    return raster_of(out, raster.transform, getattr(raster, "crs", None), None)


def buffered_mask(mask, sampling, buffer: float):
    """``mask`` grown by ``buffer`` > 0 (the pixels whose distance to the nearest mask pixel is <= buffer join it) or shrunk by
    ``buffer`` < 0 (the mask pixels whose distance to the nearest pixel outside it is > |buffer| stay); distances between pixel
    centres under ``sampling``.  A bool array or tensor where ``mask`` lives."""
    buffer = float(buffer)
    if not np.isfinite(buffer):
        raise ValueError("buffer must be finite")
    if buffer == 0.0:
        return mask
    if buffer > 0:
        dist = edt(mask, sampling, np.float64)[0]
        return dist <= buffer
    dist = edt(target_plane(mask, [0.0]), sampling, np.float64)[0]
    return dist > -buffer
