"""``geoutils.Vector`` for polygon outlines: a table of (multi)polygons that is burnt into a raster's grid on the GPU
(``xdemhip_rasterize`` of include/xdemhip.h, csrc/vector.hip) -- ``create_mask`` and ``rasterize`` as upstream's callers use them.

The rule is upstream's default ``all_touched=False``: a pixel belongs to a polygon iff its centre is inside, even-odd over all rings
of the polygon (interior rings are holes), with a half-open edge rule stated in include/xdemhip.h and restated in NumPy by
``tests/vector_oracle.py``; the device and that oracle agree bit for bit.  Away from edges the result is geometry alone and is held to
matplotlib's point-in-polygon test.  PARITY UNPINNED: geoutils, rasterio and GDAL cannot be run offline, and GDAL's treatment of a
pixel centre that lies EXACTLY on an edge may differ from the half-open rule used here.

Geometries are taken by duck typing (shapely and geopandas are never imported): an ``(N, 2)`` array (one exterior ring), ``(exterior,
[holes...])``, a list of those (a multipolygon), a GeoJSON-like mapping (``Polygon``, ``MultiPolygon``, ``Feature``; a
``FeatureCollection`` as the whole argument, its properties becoming the table), or any object that answers shapely's calls
(``.geom_type``, ``.exterior.coords``, ``.interiors``, ``.geoms``).  Out of scope: lines and points, ``all_touched=True``, buffering a
geometry (``create_mask(buffer=)`` buffers the burnt mask), reprojection of a vector, file formats other than GeoJSON.
"""
from __future__ import annotations

import collections
import ctypes
import json
import os
from collections.abc import Mapping
from typing import Any

import numpy as np
import pandas as pd

from . import _args, _lib

Bounds = collections.namedtuple("Bounds", ["left", "bottom", "right", "top"])
NORTH_UP = "only north-up transforms (b = d = 0) are supported"


class Rings(list):
    """The rings of one table row: ``(N, 2)`` float64 arrays, not closed explicitly, each with at least three distinct vertices."""

    def __repr__(self) -> str:
        return f"Rings({len(self)} rings, {sum(len(r) for r in self)} vertices)"


def _ring(coords) -> np.ndarray | None:
    a = np.asarray(coords, dtype=np.float64)
    if a.ndim != 2 or a.shape[1] < 2:
        raise ValueError(f"a ring is an (N, 2) array of x, y; got shape {a.shape}")
    a = np.ascontiguousarray(a[:, :2])
    if not np.all(np.isfinite(a)):
        raise ValueError("the vertices of a geometry must be finite")
    if a.shape[0] == 0 or np.unique(a, axis=0).shape[0] < 3:
        return None   # (fewer than three distinct vertices: the ring contributes nothing)
    return a


def _is_ring_like(x) -> bool:
    if isinstance(x, (Mapping, str)) or hasattr(x, "geom_type"):
        return False
    try:
        a = np.asarray(x, dtype=np.float64)
    except (ValueError, TypeError):
        return False
    return a.ndim == 2 and a.shape[1] >= 2


def parse_geometry(geom) -> Rings:
    """The rings of one geometry in any of the accepted forms (the module's docstring)."""
    if isinstance(geom, Rings):
        return geom
    out = Rings()

    def add(ring) -> None:
        r = _ring(ring)
        if r is not None:
            out.append(r)

    kind = getattr(geom, "geom_type", None)
    if kind is not None:   # shapely's calls
        if kind == "Polygon":
            add(geom.exterior.coords)
            for hole in geom.interiors:
                add(hole.coords)
        elif kind == "MultiPolygon":
            for part in geom.geoms:
                out.extend(parse_geometry(part))
        else:
            raise NotImplementedError(f"geometry type '{kind}' is not supported: only Polygon and MultiPolygon")
        return out
    if isinstance(geom, Mapping):
        kind = geom.get("type")
        if kind == "Feature":
            return parse_geometry(geom["geometry"])
        if kind == "Polygon":
            for ring in geom["coordinates"]:
                add(ring)
        elif kind == "MultiPolygon":
            for part in geom["coordinates"]:
                for ring in part:
                    add(ring)
        else:
            raise NotImplementedError(f"geometry type '{kind}' is not supported: only Polygon and MultiPolygon")
        return out
    if _is_ring_like(geom):
        add(geom)
        return out
    if isinstance(geom, tuple) and len(geom) == 2 and _is_ring_like(geom[0]) and isinstance(geom[1], (list, tuple)) \
            and all(_is_ring_like(h) for h in geom[1]):
        add(geom[0])
        for hole in geom[1]:
            add(hole)
        return out
    if isinstance(geom, (list, tuple)):
        for part in geom:
            out.extend(parse_geometry(part))
        return out
    raise NotImplementedError(f"geometry type '{type(geom).__name__}' is not supported: only Polygon and MultiPolygon")


def grid_of(raster) -> tuple:
    """``((H, W), transform6)`` of a DEM, a dDEM, any object with ``.shape`` and ``.transform``, or ``(shape, transform)``."""
    if isinstance(raster, tuple) and len(raster) == 2 and not hasattr(raster, "transform"):
        shape, t = raster
    else:
        shape, t = raster.shape, raster.transform
    t6 = tuple(float(v) for v in ((t.a, t.b, t.c, t.d, t.e, t.f) if hasattr(t, "a") else t))[:6]
    shape = tuple(int(v) for v in shape)[-2:]
    if len(t6) != 6 or len(shape) != 2:
        raise ValueError("a grid is ((H, W), (a, b, c, d, e, f))")
    if not (t6[1] == 0.0 and t6[3] == 0.0 and t6[0] > 0.0 and t6[4] < 0.0):
        raise NotImplementedError(NORTH_UP)
    return shape, t6


class DeviceRasterizer:
    """The binding of ``xdemhip_rasterize`` / ``xdemhip_rasterize_union``.  ``tests/vector_oracle.OracleRasterizer`` has the same two
    methods and stands in for it where no GPU is at hand.  ``last_count``: the burnt pixels of the last call."""

    last_count = 0

    @staticmethod
    def _table_args(table, where=None):
        """The five arguments a vertex table is to the library, read from the arrays or tensors `where` (default: the table's own)."""
        xy, ring_off, poly_of_ring, n_poly = table
        t = (xy, ring_off, poly_of_ring) if where is None else where
        return (_args.dp(t[0]), xy.shape[1], _args.i64p(t[1]), poly_of_ring.shape[0], _args.i32p(t[2]))

    def _out(self, ctx, shape, dtype, device):
        if device:
            import torch

            out = torch.empty(shape, dtype=getattr(torch, dtype), device=torch.device("cuda", ctx.device))
        else:
            out = np.empty(shape, dtype)
        return out, ctypes.c_void_p(_args.ptr(out))

    def _run(self, call, tables, device, ctx):
        """Host tables with a host plane; for a device plane the tables are uploaded through torch and everything stays there."""
        keep = []
        if device:
            import torch

            dev = torch.device("cuda", ctx.device)
            args = []
            for table in tables:
                t = [torch.from_numpy(a).to(dev) for a in table[:3]]
                keep.append(t)
                args.append(self._table_args(table, t))
            torch.cuda.current_stream(dev).synchronize()   # (the library launches on its own stream)
        else:
            args = [self._table_args(t) for t in tables]
        count = ctypes.c_int64()
        with ctx.call_lock:
            ctx.check(call(args, keep, ctypes.byref(count)))
        self.last_count = int(count.value)
        DeviceRasterizer.last_count = self.last_count

    def mask(self, tables, shape, t6, device: bool = False, ctx: _lib.Context | None = None):
        """The OR of the masks of one or two tables: a bool array, or a bool tensor on the GPU with `device`."""
        ctx = ctx or _lib.default_context()
        L = ctx._L
        out, ptr = self._out(ctx, shape, "uint8", device)
        space = _lib.DEVICE if device else _lib.HOST
        tr = (ctypes.c_double * 6)(*t6)
        if len(tables) == 1:
            def call(args, keep, count):
                return L.xdemhip_rasterize(ctx.handle, *args[0], None, tables[0][3], shape[0], shape[1], tr, ptr, 0, 0, space, count)
        else:
            def call(args, keep, count):
                return L.xdemhip_rasterize_union(ctx.handle, *args[0], tables[0][3], *args[1], tables[1][3], shape[0], shape[1], tr, ptr, space, count)
        self._run(call, tables, device, ctx)
        return out.bool() if device else out.view(np.bool_)

    def labels(self, table, burn, out_value, shape, t6, device: bool = False, ctx: _lib.Context | None = None):
        """The int32 label plane of one table: ``burn[p]`` of the last polygon that holds the pixel, `out_value` elsewhere."""
        ctx = ctx or _lib.default_context()
        L = ctx._L
        out, ptr = self._out(ctx, shape, "int32", device)
        space = _lib.DEVICE if device else _lib.HOST
        tr = (ctypes.c_double * 6)(*t6)
        burn = np.ascontiguousarray(burn, dtype=np.int32)

        def call(args, keep, count):
            b = burn
            if device:
                import torch

                b = torch.from_numpy(burn).to(torch.device("cuda", ctx.device))
                keep.append(b)
                _args.synchronize_torch(b)
            return L.xdemhip_rasterize(ctx.handle, *args[0], _args.i32p(b), table[3], shape[0], shape[1], tr, ptr, 1, int(out_value), space, count)

        self._run(call, [table], device, ctx)
        return out

    @staticmethod
    def stage_ms(ctx: _lib.Context | None = None) -> list:
        """Device time of the five stages (edges, crossings into segments, sorts, spans, finish) of the last call made under the test
        switch ``"vec_stage_times"``."""
        ctx = ctx or _lib.default_context()
        ms = (ctypes.c_float * 5)()
        ctx.check(ctx._L.xdemhip_rasterize_stage_ms(ctx.handle, ms))
        return [float(v) for v in ms]

    @staticmethod
    def launches(ctx: _lib.Context | None = None) -> int:
        ctx = ctx or _lib.default_context()
        n = ctypes.c_int64()
        ctx.check(ctx._L.xdemhip_rasterize_launches(ctx.handle, ctypes.byref(n)))
        return int(n.value)


class _SizedGrid:
    """A grid without data: what ``Vector.proximity(raster=None)`` hands on (``.data`` is only asked for its shape)."""

    def __init__(self, shape, transform, crs):
        self.shape, self.transform, self.crs = shape, transform, crs
        self.data = np.broadcast_to(np.uint8(0), shape)


_RASTERIZER: Any = DeviceRasterizer()   # (a test puts its oracle here)


class Vector:
    """A table of polygons: ``geometries`` in any accepted form, ``table`` their attributes (a DataFrame or a mapping of columns), ``crs``
    opaque.  ``Vector(dataframe)`` takes a DataFrame with a ``geometry`` column, such as ``v.ds.query(...)``."""

    def __init__(self, geometries, table=None, crs=None):
        if isinstance(geometries, Vector):
            geometries, table, crs = geometries.ds, None, geometries.crs if crs is None else crs
        if isinstance(geometries, Mapping) and geometries.get("type") == "FeatureCollection":
            features = list(geometries["features"])
            if table is None:
                table = pd.DataFrame([dict(f.get("properties") or {}) for f in features])
            geometries = [f["geometry"] for f in features]
        elif isinstance(geometries, Mapping) or hasattr(geometries, "geom_type") or _is_ring_like(geometries):
            geometries = [geometries]   # (a single geometry)
        if isinstance(geometries, pd.DataFrame):   # (also what a GeoDataFrame is)
            if "geometry" not in geometries.columns:
                raise ValueError("a DataFrame given as geometries needs a 'geometry' column")
            if table is None:
                table = pd.DataFrame(geometries.drop(columns="geometry"))
            if crs is None:
                crs = getattr(geometries, "crs", None)
            geometries = list(geometries["geometry"])
        rows = [parse_geometry(g) for g in geometries]
        if table is None:
            ds = pd.DataFrame(index=pd.RangeIndex(len(rows)))
        else:
            ds = pd.DataFrame(table).copy()
            if "geometry" in ds.columns:
                ds = ds.drop(columns="geometry")
            if len(ds) != len(rows):
                raise ValueError(f"the table has {len(ds)} rows for {len(rows)} geometries")
        col = pd.Series([None] * len(rows), index=ds.index, dtype=object)
        for k, r in enumerate(rows):
            col.iloc[k] = r
        ds["geometry"] = col
        self.ds = ds
        self.crs = crs
        self._tables = None
        self._cache: dict = {}

    @classmethod
    def from_geojson(cls, path_or_dict, crs=None) -> "Vector":
        """A Vector from GeoJSON: a path, a JSON string or the decoded mapping (``FeatureCollection``, ``Feature`` or a geometry)."""
        obj = path_or_dict
        if isinstance(obj, (str, os.PathLike)):
            if isinstance(obj, str) and obj.lstrip().startswith("{"):
                obj = json.loads(obj)
            else:
                with open(obj) as fh:
                    obj = json.load(fh)
        if obj.get("type") == "Feature":
            obj = {"type": "FeatureCollection", "features": [obj]}
        return cls(obj, crs=crs)

    @classmethod
    def from_mask(cls, mask, raster, connectivity=4, crs=None) -> "Vector":
        """The outlines of a boolean mask on the grid of `raster` (a DEM, a dDEM or ``(shape, transform)``): one polygon per connected
        component, labelled and traced on the GPU (``xdem_amd.polygonize``); the column ``id`` numbers them ``0..K-1``."""
        from .ddem import raster_of
        from .polygonize import polygonize

        shape, t6 = grid_of(raster)
        m = mask if hasattr(mask, "is_cuda") else np.asarray(mask)
        if tuple(m.shape) != shape or str(m.dtype).split(".")[-1] != "bool":
            raise ValueError(f"from_mask takes a boolean mask of the grid's shape {shape}")
        grid = raster_of(m, t6, crs if crs is not None else getattr(raster, "crs", None), None)
        return polygonize(grid, 1, "id", connectivity)

    # ---- the table -------------------------------------------------------------------------------------------------------------------
    def __len__(self) -> int:
        return len(self.ds)

    def __str__(self) -> str:
        return str(self.ds)

    def copy(self) -> "Vector":
        return Vector(self.ds.copy(), crs=self.crs)

    def query(self, expression: str, inplace: bool = False) -> "Vector":
        """``ds.query(expression)`` as a Vector (geoutils' ``Vector.query``)."""
        if inplace:
            self.ds = self.ds.query(expression)
            self._tables, self._cache = None, {}
            return self
        return Vector(self.ds.query(expression), crs=self.crs)

    def __getitem__(self, key) -> "Vector":
        key = np.asarray(key)
        if key.dtype != bool or key.shape != (len(self),):
            raise TypeError("a Vector is indexed by a boolean mask over its rows")
        return Vector(self.ds[key], crs=self.crs)

    @property
    def bounds(self) -> Bounds:
        """(left, bottom, right, top) over every vertex."""
        xy = self.tables()[0]
        if xy.shape[1] == 0:
            return Bounds(np.nan, np.nan, np.nan, np.nan)
        return Bounds(float(xy[0].min()), float(xy[1].min()), float(xy[0].max()), float(xy[1].max()))

    def tables(self) -> tuple:
        """``(xy, ring_off, poly_of_ring, P)`` of ``xdemhip_rasterize``: float64 (2, V), int64 (R + 1), int32 (R), rows of the table."""
        if self._tables is None:
            rings, owner = [], []
            for k, geom in enumerate(self.ds["geometry"]):
                for r in geom:
                    rings.append(r)
                    owner.append(k)
            ring_off = np.zeros(len(rings) + 1, np.int64)
            if rings:
                ring_off[1:] = np.cumsum([len(r) for r in rings])
            xy = np.ascontiguousarray(np.concatenate(rings, axis=0).T) if rings else np.zeros((2, 0))
            self._tables = (xy.astype(np.float64, copy=False), ring_off, np.asarray(owner, dtype=np.int32), len(self.ds))
        return self._tables

    # ---- rasterisation -----------------------------------------------------------------------------------------------------------------
    def _grid(self, raster, res, bounds) -> tuple:
        if raster is not None:
            return grid_of(raster)
        if res is None:
            raise ValueError("create_mask needs a raster, or a resolution `res`")
        rx, ry = (float(res), float(res)) if np.ndim(res) == 0 else (float(res[0]), float(res[1]))
        if not (rx > 0 and ry > 0):
            raise ValueError("the resolution must be positive")
        b = self.bounds if bounds is None else Bounds(*bounds)
        if not all(np.isfinite(v) for v in b):
            raise ValueError("a grid from `res` needs bounds: the vector has no vertex")
        shape = (max(1, int(np.ceil((b.top - b.bottom) / ry))), max(1, int(np.ceil((b.right - b.left) / rx))))
        return shape, (rx, 0.0, float(b.left), 0.0, -ry, float(b.top))

    def create_mask(self, raster=None, res=None, bounds=None, as_array: bool = True, device: bool = False, buffer: float = 0):
        """True where a pixel's centre is inside a polygon of the table.  `raster`: a DEM, a dDEM or ``(shape, transform)``.  With `res`
        alone the grid runs from ``(left, top)`` of `bounds` (default: the vector's) with ``ceil(extent / res)`` pixels each way, at
        least one -- UNPINNED: geoutils' own choice of that grid cannot be read offline.  Returns a NumPy bool array, with `device` a
        torch bool tensor on the GPU (nothing is fetched), with ``as_array=False`` a DEM around either.  The mask is kept per grid and
        memspace and returned again by the next call (the host array is read-only).  `buffer` (upstream's keyword, georeferenced units
        between pixel centres): > 0 adds the pixels whose distance to the nearest mask pixel is <= buffer, < 0 keeps the mask pixels
        whose distance to the nearest pixel outside the mask is > |buffer| (``xdem_amd.proximity``; UNPINNED: geoutils buffers the
        geometry with shapely before burning it)."""
        shape, t6 = self._grid(raster, res, bounds)
        key = ("mask", shape, t6, bool(device))
        if key not in self._cache:
            mask = _RASTERIZER.mask([self.tables()], shape, t6, device=bool(device))
            if isinstance(mask, np.ndarray):
                mask.setflags(write=False)   # (kept per (shape, transform, memspace) and handed out again: copy it to change it)
            self._cache[key] = mask
        mask = self._cache[key]
        if buffer != 0:
            from . import proximity as _prox

            bkey = key + (float(buffer),)
            if bkey not in self._cache:
                grown = _prox.buffered_mask(mask, (abs(t6[4]), abs(t6[0])), buffer)
                if isinstance(grown, np.ndarray):
                    grown.setflags(write=False)
                self._cache[bkey] = grown
            mask = self._cache[bkey]
        if as_array:
            return mask
        from .ddem import raster_of

        return raster_of(mask, t6, self.crs, None)

    def proximity(self, raster=None, size=(1000, 1000), geometry_type="boundary", in_or_out="both", distance_unit="georeferenced",
                  dtype=np.float32):
        """``geoutils.Vector.proximity``: the distance of every pixel of `raster`'s grid to this vector's outlines
        (``xdem_amd.proximity.proximity``; a DEM on that grid, a device plane when `raster`'s data is one).  With ``raster=None`` the
        grid has `size` = (columns, rows) pixels over the vector's bounds and the plane is a host array."""
        from . import proximity as _prox

        if raster is None:
            raster = _SizedGrid(*self.size_grid(size), self.crs)
        return _prox.proximity(raster, self, None, geometry_type, in_or_out, distance_unit, dtype)

    def size_grid(self, size) -> tuple:
        """``((rows, columns), transform6)`` of a grid of `size` = (columns, rows) pixels over the vector's bounds."""
        w, h = (int(v) for v in size)
        if w < 1 or h < 1:
            raise ValueError("size must be at least (1, 1)")
        b = self.bounds
        if not all(np.isfinite(v) for v in b) or not (b.right > b.left and b.top > b.bottom):
            raise ValueError("a grid from `size` needs bounds with an extent: the vector has none")
        return (h, w), ((b.right - b.left) / w, 0.0, float(b.left), 0.0, -(b.top - b.bottom) / h, float(b.top))

    def rasterize(self, raster, in_value=None, out_value=0, device: bool = False):
        """An int32 plane on the grid of `raster`: `in_value` of the polygon that holds the pixel's centre, the LATER polygon of the
        table where several do (GDAL's burn order), `out_value` elsewhere.  `in_value`: default ``index + 1`` per row of the table, a
        scalar for all rows, or one value per row."""
        shape, t6 = grid_of(raster)
        n = len(self)
        if in_value is None:
            burn = np.asarray(self.ds.index, dtype=np.int64) + 1 if n else np.zeros(0, np.int64)
        elif np.ndim(in_value) == 0:
            burn = np.full(n, in_value)
        else:
            burn = np.asarray(in_value)
            if burn.shape != (n,):
                raise ValueError(f"in_value has {burn.size} values for {n} polygons")
        if n and (np.any(burn != np.round(burn)) or np.any(np.abs(burn) >= 2 ** 31)) or abs(out_value) >= 2 ** 31 or out_value != round(out_value):
            raise ValueError("in_value and out_value must be integers that fit int32")
        return _RASTERIZER.labels(self.tables(), burn.astype(np.int32), int(out_value), shape, t6, device=bool(device))


def union_mask(a: Vector, b: Vector, raster, device: bool = False):
    """The mask of the pixels inside a polygon of `a` or of `b`, in one call (``xdemhip_rasterize_union``)."""
    shape, t6 = grid_of(raster)
    return _RASTERIZER.mask([a.tables(), b.tables()], shape, t6, device=bool(device))
