"""Polygonize on MI355X: a raster's target pixels as a ``Vector`` of outline polygons (``geoutils.Raster.polygonize``, which runs
GDAL's polygonize on the CPU), and underneath it connected-component labelling (``scipy.ndimage.label``) -- ``xdemhip_label``,
``xdemhip_label_table`` and ``xdemhip_outlines`` of csrc/ccl.hip; DESIGN.md 5r and include/xdemhip.h have the rule.

* ``label`` -- components of a class plane numbered ``1..K`` in raster order of their first pixel (SciPy's numbering on a 0/1 mask),
  with a table of class, pixel count and bounding box per component.
* ``outlines`` -- the outline rings of every component as the vertex table ``Vector.tables()`` holds and ``xdemhip_rasterize`` reads.
* ``polygonize`` -- ``Raster.polygonize``: one row per component, exterior ring first, holes after.

Vertices are pixel corners; only corners of the outline are kept; a ring starts at the end of its lowest-numbered corner edge; the
exterior runs counter-clockwise in map coordinates and holes clockwise.  Under ``connectivity=8`` a ring may touch itself where two
pixels of a component meet only diagonally (GDAL does the same).  **Parity unpinned**: geoutils, rasterio and GDAL cannot be run
offline, and GDAL's start vertex, ring order and orientation may differ; what is pinned is the set of pixels every polygon covers
(``Vector.rasterize`` of the result gives the label plane back bit for bit) and SciPy's numbering of the components."""
from __future__ import annotations

import collections
import contextlib
import ctypes

import numpy as np
import pandas as pd

from . import _args, _lib

RingTable = collections.namedtuple("RingTable", ["xy", "ring_off", "poly_of_ring", "ring_area", "K"])
TABLE_COLUMNS = ("class", "count", "row_min", "row_max", "col_min", "col_max", "first")
STAGES = ("tile", "border", "flatten", "number", "table", "corners", "walk", "leader", "rank", "rings", "gather")


def label_plan(H: int, W: int, switch: int = 0) -> dict:
    """The tile ``xdemhip_label`` works with on an ``H x W`` plane under the test switch ``"ccl_route" = switch``
    (``xdemhip_label_plan``, host only): ``tile_rows``, ``tile_cols``, ``tiles_r``, ``tiles_c``, ``lds_bytes``, ``lds_budget``."""
    ints = [ctypes.c_int() for _ in range(4)]
    tiles = [ctypes.c_int64(), ctypes.c_int64()]
    rc = _lib.lib().xdemhip_label_plan(int(H), int(W), int(switch), ctypes.byref(ints[0]), ctypes.byref(ints[1]), ctypes.byref(tiles[0]),
                                       ctypes.byref(tiles[1]), ctypes.byref(ints[2]), ctypes.byref(ints[3]))
    if rc != _lib.OK:
        raise ValueError(f"xdemhip_label_plan refused its arguments (status {rc})")
    return {"tile_rows": ints[0].value, "tile_cols": ints[1].value, "tiles_r": tiles[0].value, "tiles_c": tiles[1].value,
            "lds_bytes": ints[2].value, "lds_budget": ints[3].value}


def class_plane(plane, what: str = "classes"):
    """A 2-D class plane as contiguous uint8 or int32 where it lives: bool is viewed as uint8, other integers that fit become int32."""
    if _args.is_tensor(plane):
        import torch

        if not (plane.is_cuda and plane.dim() == 2):
            raise ValueError(f"{what}: a tensor must be a 2-D CUDA tensor")
        plane = plane.contiguous()
        if plane.dtype == torch.bool:
            return plane.view(torch.uint8)
        if plane.dtype in (torch.uint8, torch.int32):
            return plane
        if plane.dtype in (torch.int8, torch.int16, torch.int64):
            if plane.dtype == torch.int64 and plane.numel() and int(plane.abs().max()) >= 2 ** 31:
                raise ValueError(f"{what}: integer classes must fit int32")
            return plane.to(torch.int32)
        raise ValueError(f"{what}: a class plane is of bool or an integer dtype, got {plane.dtype}")
    a = np.asarray(plane)
    if a.ndim != 2:
        raise ValueError(f"{what}: a class plane is 2-D, got shape {a.shape}")
    if a.dtype == np.bool_:
        return np.ascontiguousarray(a).view(np.uint8)
    if a.dtype in (np.dtype(np.uint8), np.dtype(np.int32)):
        return np.ascontiguousarray(a)
    if np.issubdtype(a.dtype, np.integer):
        if a.size and (int(a.max()) >= 2 ** 31 or int(a.min()) < -2 ** 31):
            raise ValueError(f"{what}: integer classes must fit int32")
        return np.ascontiguousarray(a, dtype=np.int32)
    raise ValueError(f"{what}: a class plane is of bool or an integer dtype, got {a.dtype}")


def _empty(shape, dtype, like):
    if _args.is_tensor(like):
        import torch

        return torch.empty(shape, dtype=getattr(torch, np.dtype(dtype).name), device=like.device)
    return np.empty(shape, dtype=dtype)


def _scope(ctx, x):
    return _args.torch_stream_scope(ctx, x, reset=True) if _args.is_tensor(x) else contextlib.nullcontext()


def _ctx_of(ctx, x):
    return ctx or _lib.default_context(x.device.index if _args.is_tensor(x) else None)


def _check_connectivity(connectivity) -> int:
    if connectivity not in (4, 8):
        raise ValueError(f"connectivity must be 4 or 8, got {connectivity!r}")
    return int(connectivity)


class DeviceEngine:
    """The binding of ``xdemhip_label``, ``xdemhip_label_table`` and ``xdemhip_outlines``.  ``tests/polygonize_oracle.OracleEngine`` has
    the same methods and stands in for it where no GPU is at hand."""

    def label(self, classes, connectivity=4, ctx=None):
        """``(int32 label plane where the classes live, K)``."""
        cls = class_plane(classes)
        H, W = (int(v) for v in cls.shape)
        ctx = _ctx_of(ctx, cls)
        labels = _empty((H, W), np.int32, cls)
        K = ctypes.c_int64()
        code = _lib.U8 if _args.np_dtype(cls) == np.uint8 else _lib.I32
        with _scope(ctx, cls):
            ctx.check(ctx._L.xdemhip_label(ctx.handle, _args.ptr(cls), code, H, W, _check_connectivity(connectivity), _args.ptr(labels), None, 0,
                                           _args.space(cls), ctypes.byref(K)))
        return labels, int(K.value)

    def table(self, classes, labels, K, ctx=None):
        """The ``(7, K)`` int64 host array of ``TABLE_COLUMNS`` of a label plane and the class plane it was made of."""
        cls = class_plane(classes)
        lab = _args.same_space(labels, cls)
        H, W = (int(v) for v in cls.shape)
        if tuple(lab.shape) != (H, W) or _args.np_dtype(lab) != np.int32:
            raise ValueError("labels must be an int32 plane of the shape of the classes")
        ctx = _ctx_of(ctx, cls)
        out = _empty((len(TABLE_COLUMNS), int(K)), np.int64, cls)
        code = _lib.U8 if _args.np_dtype(cls) == np.uint8 else _lib.I32
        with _scope(ctx, cls):
            ctx.check(ctx._L.xdemhip_label_table(ctx.handle, _args.ptr(cls), code, _args.ptr(lab.contiguous() if _args.is_tensor(lab) else np.ascontiguousarray(lab)),
                                                 H, W, int(K), _args.ptr(out), _args.space(cls)))
        return out.cpu().numpy() if _args.is_tensor(out) else out

    def outlines(self, labels, K, t6, ctx=None) -> RingTable:
        """The ring table of an int32 label plane with components ``1..K``, where the plane lives.  Two library calls, as the count-
        dependent results of ``xdemhip_raster_points`` are fetched: the first counts the corners so that the arrays can be sized, the
        second counts again and places them -- three reads of the label plane's 3 x 3 neighbourhoods in all, and for a host plane two
        uploads (a bound of 4 H W vertices would be the alternative to the first call)."""
        lab = labels.contiguous() if _args.is_tensor(labels) else np.ascontiguousarray(labels)
        if _args.np_dtype(lab) != np.int32 or len(lab.shape) != 2:
            raise ValueError("labels must be a 2-D int32 plane")
        H, W = (int(v) for v in lab.shape)
        ctx = _ctx_of(ctx, lab)
        tr = (ctypes.c_double * 6)(*t6)
        V, R = ctypes.c_int64(), ctypes.c_int64()
        space = _args.space(lab)
        with _scope(ctx, lab):
            ctx.check(ctx._L.xdemhip_outlines(ctx.handle, _args.ptr(lab), H, W, int(K), tr, None, 0, None, None, None, 0, space, ctypes.byref(V), ctypes.byref(R)))
            v, r_cap = int(V.value), int(R.value)
            xy = _empty((2, v), np.float64, lab)
            ring_off = _empty((r_cap + 1,), np.int64, lab)
            owner = _empty((r_cap,), np.int32, lab)
            area = _empty((r_cap,), np.int64, lab)
            if v == 0:   # (no component: nothing to trace, and an empty tensor has no address to hand over)
                ring_off[0] = 0
                return RingTable(xy, ring_off, owner, area, int(K))
            ctx.check(ctx._L.xdemhip_outlines(ctx.handle, _args.ptr(lab), H, W, int(K), tr, _args.ptr(xy), v, _args.ptr(ring_off), _args.ptr(owner),
                                              _args.ptr(area), r_cap, space, ctypes.byref(V), ctypes.byref(R)))
        r = int(R.value)
        return RingTable(xy, ring_off[:r + 1], owner[:r], area[:r], int(K))

    @staticmethod
    def stage_ms(ctx=None) -> tuple[dict, tuple[int, int]]:
        """Device time per stage (``STAGES``) of the last label and outline calls on the context, and the kernels each launched."""
        ctx = ctx or _lib.default_context()
        ms = (ctypes.c_float * len(STAGES))()
        launches = (ctypes.c_int64 * 2)()
        ctx.check(ctx._L.xdemhip_ccl_stage_ms(ctx.handle, ms, launches))
        return dict(zip(STAGES, (float(v) for v in ms))), (int(launches[0]), int(launches[1]))


_ENGINE = DeviceEngine()   # (a test puts its oracle here)


def _kw(ctx):
    return {} if ctx is None else {"ctx": ctx}


def _to_device(a, ctx):
    import torch

    return torch.from_numpy(a).to(torch.device("cuda", (ctx or _lib.default_context()).device))


def label(classes, connectivity=4, device=False, ctx=None):
    """The connected components of a class plane (bool or integer; 0 is background): pixels are joined iff they are neighbours under
    `connectivity` (4: edges, 8: and diagonals) and hold the same non-zero class.  Returns ``(labels, K, table)``: the int32 label
    plane (0 on background, ``1..K`` in raster order of each component's first pixel: ``scipy.ndimage.label``'s numbering on a mask),
    the number of components, and a DataFrame with one row per component (index = label) and the columns ``class``, ``count``,
    ``row_min``, ``row_max``, ``col_min``, ``col_max`` (inclusive) and ``first`` (linear index of the first pixel).  A host array
    gives a host plane; a CUDA tensor, or `device`, a tensor on the GPU."""
    _check_connectivity(connectivity)
    cls = class_plane(classes)
    if device and not _args.is_tensor(cls):
        cls = _to_device(cls, ctx)
    labels, K = _ENGINE.label(cls, connectivity, **_kw(ctx))
    t = _ENGINE.table(cls, labels, K, **_kw(ctx)) if K else np.zeros((len(TABLE_COLUMNS), 0), np.int64)
    table = pd.DataFrame({name: t[k] for k, name in enumerate(TABLE_COLUMNS)}, index=pd.RangeIndex(1, K + 1, name="label"))
    return labels, K, table


def outlines(labels_or_classes, transform, connectivity=4, K=None, ctx=None) -> RingTable:
    """The outline rings of the components of a plane on the north-up grid `transform`: with `K` the plane is an int32 label plane
    holding ``1..K`` (as ``label`` returns it), without it a class plane that is labelled first under `connectivity`.  Returns
    ``RingTable(xy, ring_off, poly_of_ring, ring_area, K)`` where the plane lives: float64 ``(2, V)`` map coordinates, int64
    ``(R + 1)`` ring offsets, int32 ``(R)`` component ordinal (label - 1) and int64 ``(R)`` signed area in pixels (positive: the
    exterior, first among its component's rings; negative: a hole)."""
    from .vector import grid_of

    shape, t6 = grid_of((tuple(labels_or_classes.shape), transform))   # (rotated grids: the north-up NotImplementedError)
    plane = labels_or_classes
    if K is None:
        plane, K = _ENGINE.label(class_plane(plane), _check_connectivity(connectivity), **_kw(ctx))
    return _ENGINE.outlines(plane, K, t6, **_kw(ctx))


def vector_of(rings: RingTable, table=None, crs=None):
    """A ``Vector`` with one row per component of a ring table (its arrays fetched to the host if need be)."""
    from .vector import Rings, Vector

    xy, ring_off, owner = (np.ascontiguousarray(a.cpu().numpy() if _args.is_tensor(a) else a) for a in rings[:3])
    rows = [Rings() for _ in range(rings.K)]
    pts = xy.T
    for r, k in enumerate(owner):
        rows[k].append(pts[ring_off[r]:ring_off[r + 1]])
    v = Vector(rows, table=table, crs=crs)
    v._tables = (xy, ring_off, owner, rings.K)   # (the layout xdemhip_rasterize reads, as it came)
    return v


def target_mask(data, target_values="all", nodata=None):
    """The bool mask of the pixels geoutils' ``polygonize`` targets, where `data` lives: a number (equal to it), a ``(min, max)`` tuple
    (strictly between), a list or array (equal to one of up to 64 values), or "all" (finite and not `nodata`).  NaN never is a target."""
    from . import proximity as _prox

    if isinstance(target_values, str):
        if target_values != "all":
            raise ValueError(f"target_values must be a number, a (min, max) tuple, a list or 'all', got {target_values!r}")
        if _args.is_tensor(data):
            import torch

            m = torch.isfinite(data) if data.is_floating_point() else torch.ones_like(data, dtype=torch.bool)
        else:
            data = _args.nan_filled(data)
            m = np.isfinite(data) if np.issubdtype(data.dtype, np.floating) else np.ones(data.shape, bool)
        return m if nodata is None else m & (data != nodata)
    if isinstance(target_values, tuple):
        if len(target_values) != 2:
            raise ValueError("a tuple of target_values is (min, max)")
        if not _args.is_tensor(data):
            data = _args.nan_filled(data)
        return (data > target_values[0]) & (data < target_values[1])
    if np.ndim(target_values) == 0 and not isinstance(target_values, (int, float, np.integer, np.floating)):
        raise ValueError(f"target_values must be a number, a (min, max) tuple, a list or 'all', got {target_values!r}")
    plane = _prox.target_plane(data, np.atleast_1d(np.asarray(target_values, dtype=np.float64)))
    return plane.bool() if _args.is_tensor(plane) else plane.view(np.bool_)


def polygonize(raster, target_values="all", data_column_name="id", connectivity=4, by_value=False):
    """``geoutils.Raster.polygonize``: the target pixels of `raster` (a DEM, or anything with ``.data`` and ``.transform``) as a
    ``Vector`` with one polygon per connected component, exterior ring first and holes after.  `target_values`: a number, a ``(min,
    max)`` tuple (strictly between), a list, or "all" (every finite pixel that is not nodata).  The table holds `data_column_name` =
    ``0..K-1`` in raster order of each component's first pixel and ``raster_value`` = 1; with `by_value` (integer rasters only)
    pixels are joined only where their values are equal and ``raster_value`` is that value; the class plane of that route is made
    on the HOST (``numpy.unique`` ranks the distinct values, so a device raster is fetched and the classes sent back) before the GPU
    labels and traces it.  `connectivity`: 4 (GDAL's default) or 8.
    North-up grids only.  **Parity unpinned**: GDAL's start vertex, ring order and orientation cannot be read offline; the set of
    pixels each polygon covers is what is pinned."""
    from .vector import grid_of

    _check_connectivity(connectivity)
    data = raster.data
    grid_of((tuple(data.shape), raster.transform))
    mask = target_mask(data, target_values, getattr(raster, "nodata", None))
    values = None
    if by_value:
        host = data.cpu().numpy() if _args.is_tensor(data) else np.asarray(data)
        if not np.issubdtype(host.dtype, np.integer):
            raise NotImplementedError("by_value needs an integer raster")
        hmask = mask.cpu().numpy() if _args.is_tensor(mask) else mask
        values, inverse = np.unique(host[hmask], return_inverse=True)
        classes = np.zeros(host.shape, np.int32)
        classes[hmask] = inverse.astype(np.int32) + 1   # (a class is the rank of the value: the value 0 can be a target too)
        if _args.is_tensor(data):
            classes = _args.same_space(classes, data)
    else:
        classes = mask
    cls = class_plane(classes)
    labels, K = _ENGINE.label(cls, connectivity)
    rings = _ENGINE.outlines(labels, K, grid_of((tuple(data.shape), raster.transform))[1])
    table = {data_column_name: np.arange(K, dtype=np.int64)}
    if values is None:
        table["raster_value"] = np.ones(K, np.int64)
    else:
        ranks = _ENGINE.table(cls, labels, K)[TABLE_COLUMNS.index("class")] if K else np.zeros(0, np.int64)
        table["raster_value"] = values[ranks - 1] if K else values[:0]
    return vector_of(rings, pd.DataFrame(table), getattr(raster, "crs", None))
