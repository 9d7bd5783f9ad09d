"""Terrain attributes on MI355X -- host-side mirror of ``xdem.terrain`` for the stencil hot path.

Same call signatures, argument meaning, return-type rules and error messages as the reference
(``xdem/terrain/terrain.py:176-485`` ``get_terrain_attribute`` and its thin wrappers 693-1571), but the
engines behind it are the fused HIP kernel of ``csrc/terrain.hip`` reached through the C-ABI
(``include/xdemhip.h``: ``xdemhip_terrain``).  There is no CPU engine in this package.

Covered attributes (the hot path named in BASELINE.json): slope, aspect, hillshade, curvature
(deprecated), profile / tangential / planform / flowline / max / min curvature, topographic position
index, terrain ruggedness index, plus the remaining windowed indexes: ``roughness``, ``rugosity``
and ``fractal_roughness`` (``csrc/window_extra.hip``) and the frequency-domain ``texture_shading`` (8f-4,
``csrc/texture.hip``) -- i.e. every attribute ``xdem.terrain.get_terrain_attribute`` offers.
"""
from __future__ import annotations

import ctypes
import warnings
from collections.abc import Sized
from typing import Any

import numpy as np

from . import _args, _lib

# Attribute families as in xdem/terrain/terrain.py:40-84
available_attributes = [
    "slope", "aspect", "hillshade", "profile_curvature", "tangential_curvature", "planform_curvature",
    "flowline_curvature", "max_curvature", "min_curvature", "topographic_position_index",
    "terrain_ruggedness_index", "roughness", "rugosity", "fractal_roughness", "texture_shading",
]
list_requiring_surface_fit = [
    "slope", "aspect", "hillshade", "curvature", "profile_curvature", "tangential_curvature",
    "planform_curvature", "flowline_curvature", "max_curvature", "min_curvature",
]
list_requiring_windowed_index = ["terrain_ruggedness_index", "topographic_position_index", "roughness", "rugosity"]
list_requiring_windowed_fractal_index = ["fractal_roughness"]
list_requiring_frequency_domain = ["texture_shading"]

# attribute -> bit of the C-ABI mask (include/xdemhip.h)
ATTR_BIT = {
    "slope": 0, "aspect": 1, "hillshade": 2, "curvature": 3, "profile_curvature": 4, "tangential_curvature": 5,
    "planform_curvature": 6, "flowline_curvature": 7, "max_curvature": 8, "min_curvature": 9,
    "topographic_position_index": 10, "terrain_ruggedness_index": 11, "roughness": 12, "rugosity": 13,
    "fractal_roughness": 14,
}
_NOT_ON_HOT_PATH = ()
_FIT_ID = {"horn": 0, "zevenbergthorne": 1, "florinsky": 2}
_CURV_ID = {"geometric": 0, "directional": 1}
_TRI_ID = {"riley": 0, "wilson": 1}


def _is_raster(obj: Any) -> bool:
    """Duck-typed geoutils.Raster (the package is not a dependency): has .data, .res, .transform, .crs."""
    return all(hasattr(obj, a) for a in ("data", "res", "transform", "crs")) and not isinstance(obj, np.ndarray)


def _array_with_nan(dem: Any) -> np.ndarray:
    """Equivalent of ``gu.raster.get_array_and_mask(dem)[0]`` (terrain.py:558): masked / nodata -> NaN."""
    if _is_raster(dem):
        dem = dem.data
    if isinstance(dem, np.ma.MaskedArray):
        arr = np.array(dem.data, copy=True)
        mask = np.ma.getmaskarray(dem)
        if np.issubdtype(arr.dtype, np.integer):
            arr = arr.astype(np.float32)
        if mask.any():
            arr[mask] = np.nan
        return arr
    return np.asarray(dem)


def _validate(dem, attribute, resolution, hillshade_altitude, hillshade_azimuth, hillshade_z_factor, surface_fit,
              curv_method, tri_method, window_size_fractal):
    """Input checks of xdem/terrain/terrain.py:293-409 with the reference's messages."""
    if surface_fit == "Horn":
        curvature_list = ["curvature", "profile_curvature", "tangential_curvature", "planform_curvature",
                          "flowline_curvature", "max_curvature", "min_curvature"]
        found = attribute in curvature_list if isinstance(attribute, str) else any(a in curvature_list for a in attribute)
        if found:
            raise ValueError(
                "'Horn' surface fit method cannot be used for to calculate curvatures. "
                "Use 'ZevenbergThorne' or 'Florinsky' instead."
            )
    if _is_raster(dem) and resolution is None:
        resolution = dem.res
    if isinstance(attribute, str):
        attribute = [attribute]
    attributes_requiring_surface_fit = [a for a in attribute if a in list_requiring_surface_fit]
    if "fractal_roughness" in attribute:
        if window_size_fractal < 5:
            warnings.warn(category=UserWarning, stacklevel=3,
                          message="Fractal roughness can only be computed on window sizes larger or equal to 5.")
        elif window_size_fractal < 13:
            warnings.warn(category=UserWarning, stacklevel=3,
                          message="Fractal roughness results with window size of less than 13 can be inaccurate.")
    attributes_requiring_resolution = attributes_requiring_surface_fit + (["rugosity"] if "rugosity" in attribute else [])
    if len(attributes_requiring_resolution) > 0:
        if resolution is None:
            raise ValueError(
                f"'resolution' must be provided as an argument for attributes: {attributes_requiring_resolution}"
            )
        if not isinstance(resolution, Sized):
            resolution = (float(resolution), float(resolution))
        if resolution[0] != resolution[1]:
            raise ValueError(
                f"Surface fit and rugosity require the same X and Y resolution ({resolution} was given). "
                f"This was required by: {attributes_requiring_resolution}."
            )
    if resolution is None:
        resolution = 1
    elif isinstance(resolution, Sized):
        resolution = resolution[0]
    choices = (list_requiring_surface_fit + list_requiring_windowed_index + list_requiring_windowed_fractal_index
               + list_requiring_frequency_domain)
    for attr in attribute:
        if attr not in choices:
            raise ValueError(f"Attribute '{attr}' is not supported. Choices: {choices}")
    list_surface_fit = ["Horn", "ZevenbergThorne", "Florinsky"]
    if surface_fit.lower() not in [sm.lower() for sm in list_surface_fit]:
        raise ValueError(f"Surface fit '{surface_fit}' is not supported. Must be one of: {list_surface_fit}")
    list_curv_methods = ["geometric", "directional"]
    if curv_method.lower() not in [cm.lower() for cm in list_curv_methods]:
        raise ValueError(f"Curvature method '{curv_method}' is not supported. Must be one of: {list_curv_methods}")
    list_tri_methods = ["Riley", "Wilson"]
    if tri_method.lower() not in [tm.lower() for tm in list_tri_methods]:
        raise ValueError(f"TRI method '{tri_method}' is not supported. Must be one of: {list_tri_methods}")
    if (hillshade_azimuth < 0.0) or (hillshade_azimuth > 360.0):
        raise ValueError(f"Azimuth must be a value between 0 and 360 degrees (given value: {hillshade_azimuth})")
    if (hillshade_altitude < 0.0) or (hillshade_altitude > 90):
        raise ValueError("Altitude must be a value between 0 and 90 degrees (given value: {altitude})")
    if (hillshade_z_factor < 0.0) or not np.isfinite(hillshade_z_factor):
        raise ValueError(f"z_factor must be a non-negative finite value (given value: {hillshade_z_factor})")
    if _is_raster(dem) and len(attributes_requiring_surface_fit) > 0:
        crs = getattr(dem, "crs", None)
        if crs is not None and not getattr(crs, "is_projected", True):
            warnings.warn(
                category=UserWarning,
                message=f"DEM is not in a projected CRS, the following surface fit attributes might be "
                f"wrong: {list_requiring_surface_fit}."
                f"Use DEM.reproject(crs=DEM.get_metric_crs()) to reproject in a projected CRS.",
            )
    for attr in attribute:
        if attr in _NOT_ON_HOT_PATH:
            raise NotImplementedError(
                f"Attribute '{attr}' is not on the MI355X hot path of xdem_amd (surface-fit attributes and windowed "
                "indexes); see SURVEY.md section 8f."
            )
    return attribute, resolution


def launch_terrain(ctx: _lib.Context, dem_ptr: int, dem_dtype, H: int, W: int, row_stride: int, halo_top: int,
                   halo_bottom: int, resolution: float, surface_fit: str, curv_method: str, attribute: list[str],
                   tri_method: str, window_size: int, hillshade_altitude: float, hillshade_azimuth: float,
                   hillshade_z_factor: float, degrees: bool, out_dtype, plane_ptrs: dict[str, int], memspace: int,
                   window_size_fractal: int = 13) -> None:
    """Thin marshalling of ``xdemhip_terrain`` (planes are passed in ascending attribute-bit order).  Fractal
    roughness has its own window size and, like upstream (terrain.py:619-630), its own engine call.  ``degrees`` is a bool, or the
    library's integer form: bit 0 degrees, bit 1 hillshade without the clip (the engine-boundary call of ``xdem_amd.surfit``)."""
    frac = [a for a in attribute if a in list_requiring_windowed_fractal_index]
    if frac and len(frac) < len(set(attribute)):
        rest = [a for a in attribute if a not in list_requiring_windowed_fractal_index]
        launch_terrain(ctx, dem_ptr, dem_dtype, H, W, row_stride, halo_top, halo_bottom, resolution, surface_fit,
                       curv_method, rest, tri_method, window_size, hillshade_altitude, hillshade_azimuth,
                       hillshade_z_factor, degrees, out_dtype, plane_ptrs, memspace)
        attribute = frac
    if frac:
        window_size = window_size_fractal
    mask = 0
    for a in attribute:
        mask |= 1 << ATTR_BIT[a]
    ordered = sorted(set(attribute), key=lambda a: ATTR_BIT[a])
    planes = (ctypes.c_void_p * len(ordered))(*[plane_ptrs[a] for a in ordered])
    args = (ctx.handle, ctypes.c_void_p(dem_ptr), _args.code(dem_dtype), H, W,
            row_stride, halo_top, halo_bottom, float(resolution), _FIT_ID[surface_fit.lower()],
            _CURV_ID[curv_method.lower()], mask, _TRI_ID[tri_method.lower()], int(window_size), float(hillshade_altitude),
            float(hillshade_azimuth), float(hillshade_z_factor), (int(degrees) & 3) if isinstance(degrees, int) and not isinstance(degrees, bool) else int(bool(degrees)),
            _args.code(out_dtype), planes, memspace)
    with ctx.call_lock:   # (a launch reads the context's options: not while another thread has one changed for its own call)
        rc = ctx._L.xdemhip_terrain(*args)
    ctx.check(rc)


def get_terrain_attribute(
    dem,
    attribute,
    resolution=None,
    degrees: bool = True,
    hillshade_altitude: float = 45.0,
    hillshade_azimuth: float = 315.0,
    hillshade_z_factor: float = 1.0,
    slope_method=None,
    surface_fit: str = "Florinsky",
    curv_method: str = "geometric",
    tri_method: str = "Riley",
    window_size: int = 3,
    window_size_fractal: int = 13,
    engine: str = "hip",
    texture_alpha: float = 0.8,
    out_dtype=None,
    mp_config=None,
):
    """Derive one or multiple terrain attributes from a DEM on the GPU.

    Drop-in for ``xdem.terrain.get_terrain_attribute`` (xdem/terrain/terrain.py:176-485): ``str`` attribute
    -> one array, ``list`` -> list of arrays (a one-element list also yields a single array, as upstream,
    terrain.py:666); ndarray / masked-array in -> ndarray out; Raster-like in -> ``type(dem).from_array(...,
    nodata=-99999)`` out.

    Every ``engine`` value runs the HIP kernels; the name only selects upstream's precision recipe for the surface
    fit: ``"hip"`` / ``"scipy"`` (upstream's default engine, the one parity is pinned on) round the fitted derivatives
    to the DEM dtype before the float64 attribute formulas (``scipy.ndimage.convolve`` returns the input dtype,
    spatialstats.py:2512-2594); ``"numba"`` keeps them in float64 as upstream's Numba engine does (surfit.py:1044)
    and, like that engine, has no dilated non-finite mask: pixels next to a +-Inf value come out of the arithmetic (slope
    90 deg, ...) instead of NaN (surfit.py:1270-1303 against 1185-1192).  On finite / NaN data the two differ only for a
    float32 / integer DEM, at the 1e-7 .. 1e-6 relative level upstream itself tolerates (tests/test_terrain/test_surfit.py:452).
    Pinned by outputs of upstream's own numba-engine code (tests/golden/terrain_T11_numba_engine.npz).  Windowed indexes are
    evaluated on a float64 window under every engine name (upstream's Numba engine sums them in the DEM dtype, window.py:851:
    a noisier evaluation of the same quantity).
    """
    if slope_method is not None:
        warnings.warn("'slope_method' is deprecated, use 'surface_fit' instead.", DeprecationWarning, stacklevel=2)
        surface_fit = slope_method
    if engine not in ("hip", "scipy", "numba"):
        raise ValueError(f"engine must be 'hip', 'scipy' or 'numba' (got '{engine}'); all of them run on the GPU.")
    attribute, resolution = _validate(dem, attribute, resolution, hillshade_altitude, hillshade_azimuth,
                                      hillshade_z_factor, surface_fit, curv_method, tri_method, window_size_fractal)
    tile_rows = _tile_rows_of(mp_config, dem)   # (refusals of the tiled call come right after the validation, as upstream)
    if "texture_shading" in attribute:
        texture_alpha = 0.8 if texture_alpha is None else texture_alpha
        if not 0 <= texture_alpha <= 2:
            raise ValueError(f"Alpha must be between 0 and 2, got {texture_alpha}")  # freq.py:80-83
    if out_dtype is None:
        in_dt = np.asarray(dem.data if _is_raster(dem) else dem).dtype
        out_dtype = np.float32 if np.issubdtype(in_dt, np.integer) else np.dtype(in_dt)
    out_dtype = np.dtype(out_dtype)
    if out_dtype not in (np.dtype(np.float32), np.dtype(np.float64)):
        raise ValueError(f"out_dtype must be float32 or float64 on the HIP engine (got {out_dtype}).")

    dem_arr = _array_with_nan(dem)
    if dem_arr.ndim != 2:
        raise ValueError("The DEM must be a 2D array.")
    if np.issubdtype(dem_arr.dtype, np.integer):
        dem_arr = dem_arr.astype(np.float32)
    if dem_arr.dtype not in (np.dtype(np.float32), np.dtype(np.float64)):
        dem_arr = dem_arr.astype(np.float64 if dem_arr.dtype.itemsize > 4 else np.float32)
    dem_arr = np.ascontiguousarray(dem_arr)
    H, W = dem_arr.shape

    outs = {a: np.empty((H, W), dtype=out_dtype) for a in set(attribute)}
    ctx = _lib.default_context()
    with (ctx.option_scope("host_chunk_rows", tile_rows) if tile_rows else ctx.call_lock):
        return _run_and_wrap(ctx, dem, dem_arr, attribute, outs, H, W, resolution, degrees, hillshade_altitude, hillshade_azimuth,
                             hillshade_z_factor, surface_fit, curv_method, tri_method, window_size, window_size_fractal, engine,
                             texture_alpha, out_dtype, mp_config)


def _tile_rows_of(mp_config, dem) -> int:
    """Upstream's tiled call (terrain.py:412-466: `mp_config` = geoutils' MultiprocConfig(chunk_size, outfile, cluster)) mapped
    onto the library's chunked host path: the raster streams through the GPU in chunks of `chunk_size` ROWS with the overlap
    the attributes need (the library derives the same depth as terrain.py:417-432) -- results are bit-identical to the one-pass
    call, as upstream's tiles are to its untiled call.  `outfile` is honoured through the Raster's own `save`; a `cluster` of
    worker processes has no counterpart (the tiles run on one GPU, one after the other) and is ignored with a warning."""
    if mp_config is None:
        return 0
    if not _is_raster(dem):
        raise TypeError("The DEM must be a Raster to use multiprocessing.")   # terrain.py:436-437
    chunk = int(getattr(mp_config, "chunk_size", 0) or 0)
    if chunk <= 0:
        raise ValueError("mp_config.chunk_size must be a positive number of pixels.")
    cluster = getattr(mp_config, "cluster", None)
    if cluster is not None and "basic" not in type(cluster).__name__.lower():
        warnings.warn("mp_config.cluster is ignored: the tiles are row chunks streamed through one GPU, not tasks of worker "
                      "processes (multi-GPU: xdem_amd.dist).", UserWarning, stacklevel=3)
    return chunk


def _run_and_wrap(ctx, dem, dem_arr, attribute, outs, H, W, resolution, degrees, hillshade_altitude, hillshade_azimuth,
                  hillshade_z_factor, surface_fit, curv_method, tri_method, window_size, window_size_fractal, engine,
                  texture_alpha, out_dtype, mp_config):
    stencil = [a for a in attribute if a not in list_requiring_frequency_domain]
    groups = [(dem_arr, stencil, 0)]
    if engine == "numba" and any(a in list_requiring_surface_fit for a in stencil):
        # upstream's Numba recipe for the surface fit (surfit.py:948-1088, 1270-1303): unrounded float64 derivatives -- the
        # float64-input kernel on the (exactly) widened DEM -- and no dilated non-finite mask: +-Inf pixels go through the
        # arithmetic (library option "terrain_nonfinite" = 1).  Windowed indexes on the DEM as is.
        wide = dem_arr if dem_arr.dtype == np.float64 else dem_arr.astype(np.float64)
        groups = [(wide, [a for a in stencil if a in list_requiring_surface_fit], 1),
                  (dem_arr, [a for a in stencil if a not in list_requiring_surface_fit], 0)]
    for arr, names, nonfinite in groups:
        if names:
            with ctx.option_scope("terrain_nonfinite", nonfinite):
                launch_terrain(ctx, _args.ptr(arr), arr.dtype, H, W, W, 0, 0, resolution, surface_fit, curv_method,
                               names, tri_method, window_size, hillshade_altitude, hillshade_azimuth, hillshade_z_factor,
                               degrees, out_dtype, {a: _args.ptr(outs[a]) for a in set(names)}, _lib.HOST, window_size_fractal)
    if "texture_shading" in attribute:  # frequency-domain attribute: its own engine (terrain.py:637-644)
        alpha = texture_alpha
        ctx.check(ctx._L.xdemhip_texture_shading(ctx.handle, _args.ptr(dem_arr), _args.code(dem_arr), H, W, float(alpha), _args.code(out_dtype),
                                                 _args.ptr(outs["texture_shading"]), _lib.HOST))
    output_attributes = [outs[a] for a in attribute]
    if _is_raster(dem):
        output_attributes = [
            type(dem).from_array(attr, transform=dem.transform, crs=dem.crs, nodata=-99999) for attr in output_attributes
        ]
    outfile = getattr(mp_config, "outfile", None) if mp_config is not None else None
    if outfile is not None:   # one file per attribute, named as upstream names them (terrain.py:441-443)
        for name, raster in zip(attribute, output_attributes):
            raster.save(outfile if len(attribute) == 1 else outfile.split(".")[0] + "_" + name + ".tif")
    return output_attributes if len(output_attributes) > 1 else output_attributes[0]


def _calibrated_planes(n_attr: int, H: int, W: int, dtype, ctx: _lib.Context, probe, candidates=("scattered", "torch") * 4):
    """Several placements of a plane set, the caller's launch timed on each, the fastest kept (see ``alloc_planes``).  A candidate is
    allocated WHILE the best one so far is still held -- so that it lands on other physical memory -- probed (two untimed + three
    timed launches), and either replaces the incumbent (more than 1 % faster) or is released; never more than two sets are alive.
    None when not even two sets fit (the caller then takes the uncalibrated default)."""
    import gc
    import time

    import torch

    dev = torch.device("cuda", ctx.device)
    np_dt = {torch.float32: "float32", torch.float64: "float64"}[dtype]
    need = n_attr * H * W * torch.empty((), dtype=dtype).element_size()
    best, best_kind, best_ms, log = None, None, float("inf"), []
    t_start = time.perf_counter()
    for kind in candidates:
        gc.collect()
        torch.cuda.empty_cache()   # (a released ordinary block goes back to the driver, not into torch's cache)
        if torch.cuda.mem_get_info(dev)[0] < need + (2 << 30):
            break
        try:
            t = ctx.device_tensor((n_attr, H, W), np_dt, scattered=True) if kind == "scattered" else torch.empty((n_attr, H, W), dtype=dtype, device=dev)
        except (_lib.XdemHipError, RuntimeError, MemoryError):
            continue
        probe(t)   # (first touch of the pages, code objects)
        probe(t)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(3):
            probe(t)
        e1.record()
        torch.cuda.synchronize(dev)
        ms = e0.elapsed_time(e1) / 3.0
        log.append([kind, round(ms, 4)])
        if best is None or ms < 0.99 * best_ms:
            best, best_kind, best_ms = t, kind, ms
        del t
        # good draws cluster at the fast end, slow ones scatter (12.6-12.9 against 13-16 ms for the 40000^2 set): once a second
        # candidate has come within 3 % of the fastest, the fastest is a good draw and not merely the least bad one -- stop there
        # (at least three candidates, at most eight)
        times = sorted(m for _, m in log)
        if len(times) >= 3 and times[1] <= 1.03 * times[0]:
            break
    if best is None or len(log) < 2:
        return None
    gc.collect()
    torch.cuda.empty_cache()
    best._xdem_backing = best_kind
    best._xdem_calibration_ms = log
    best._xdem_calibration_launches = 5
    best._xdem_calibration_s = round(time.perf_counter() - t_start, 3)
    return best


def alloc_planes(n_attr: int, H: int, W: int, dtype=None, ctx: _lib.Context | None = None, device=None, backing: str = "auto", probe=None):
    """(n_attr, H, W) device tensor for resident attribute planes.

    How the planes are backed PHYSICALLY decides the speed of the streaming kernel: it writes ~55 row
    streams at once (11 planes x the row bands in flight), and when the planes sit in one physically contiguous block -- what an
    ordinary hipMalloc returns on a box whose free device memory is still one piece -- those streams collide in the memory
    channels: 14.4-15.6 ms for the 40000^2 set instead of 12.7-13.3 ms.  ``backing``:
    "auto" (default) = "scattered" for sets of 256 MiB and more (an ordinary allocation if the driver cannot provide the pieces),
    torch's allocator below; "scattered" = one virtual range over
    32 MiB physical pieces (8 MiB until round 6) mapped in a fixed pseudo-random order (``xdemhip_device_alloc``, HIP virtual memory management): 13.3 ms
    on a box where ordinary and contiguous planes ran at 15.0-15.6 / 14.8 ms in the same process; "torch" = torch's allocator
    (ordinary hipMalloc); "contiguous", "chunked" (64 MiB pieces in order), "recycled" = the other forms, kept for measurements.
    The memory of the library's forms is released when the tensor (and every view of it) is gone.  The scattered pieces are mapped
    for THIS device only (``hipMemSetAccess`` of the owning device): planes another GPU reads directly (peer access, IPC handles)
    must come from ``backing="torch"``; RCCL send / recv of their rows is fine (the local GPU reads them).

    ``probe`` (with ``backing="auto"``, large sets): a callable ``probe(planes)`` that enqueues the caller's own launch on the
    current stream.  Neither placement wins on every box -- on most the scattered pieces run 12.7-12.9 ms where an ordinary
    allocation runs 12.7-15 ms, but a process whose free device memory is already in pieces can see the opposite (session
    r06zzzz: scattered 14.3 ms, ordinary 12.7 ms in the same process), and two allocations of the same kind differ as well
    (session r06av) -- so with a probe several candidates are tried in turn (scattered, ordinary, scattered, ... -- each
    allocated while the best so far is still held, so that it lands elsewhere; at least three, at most eight, until a second
    one has come within 3 % of the fastest), the probe is timed on each (two untimed + three timed launches), and the fastest is
    returned; the others are released.  The tensor carries ``_xdem_backing``,
    ``_xdem_calibration_ms`` (the candidates in order) and ``_xdem_calibration_s`` (what the calibration cost)."""
    import torch

    dtype = dtype or torch.float32
    ctx = ctx or _lib.default_context(None if device is None else torch.device(device).index)
    auto = backing == "auto"
    if auto:
        backing = "scattered" if n_attr * H * W * torch.empty((), dtype=dtype).element_size() >= (1 << 28) else "torch"
    if auto and probe is not None and backing == "scattered":
        planes = _calibrated_planes(n_attr, H, W, dtype, ctx, probe)
        if planes is not None:
            return planes
    if backing == "torch":
        return torch.empty((n_attr, H, W), dtype=dtype, device=torch.device("cuda", ctx.device))
    if backing not in ("contiguous", "chunked", "recycled", "scattered"):
        raise ValueError("backing must be 'auto', 'torch', 'scattered', 'contiguous', 'chunked' or 'recycled'")
    kw = dict(contiguous=backing in ("contiguous", "recycled"), recycled=backing == "recycled", chunked=backing == "chunked",
              scattered=backing == "scattered")
    np_dt = {torch.float32: "float32", torch.float64: "float64"}[dtype]
    soft = (_lib.XdemHipError, RuntimeError, MemoryError)   # allocator refusals (library / torch); anything else is a bug and propagates
    try:
        return ctx.device_tensor((n_attr, H, W), np_dt, **kw)
    except soft:
        if not auto:
            raise
    # "auto": the library's pieces do not come out of torch's cache -- hand the cached blocks back to the driver and try again,
    # and rather take an ordinary allocation than fail (said aloud: the backing decides the speed of the streaming kernel)
    torch.cuda.empty_cache()
    try:
        return ctx.device_tensor((n_attr, H, W), np_dt, **kw)
    except soft as e:
        warnings.warn(f"xdem_amd: scattered plane backing unavailable ({e}); falling back to torch's allocator", RuntimeWarning,
                      stacklevel=2)
    ctx.release_pool()   # memory torch cannot see: give it back before asking torch for the planes
    return torch.empty((n_attr, H, W), dtype=dtype, device=torch.device("cuda", ctx.device))


def terrain_attributes_device(dem, attribute: list[str], resolution: float = 1.0, degrees: bool = True,
                              hillshade_altitude: float = 45.0, hillshade_azimuth: float = 315.0,
                              hillshade_z_factor: float = 1.0, surface_fit: str = "Florinsky",
                              curv_method: str = "geometric", tri_method: str = "Riley", window_size: int = 3,
                              out=None, halo_top: int = 0, halo_bottom: int = 0, ctx: _lib.Context | None = None,
                              window_size_fractal: int = 13):
    """Device-resident variant: ``dem`` is a CUDA(HIP) torch tensor (rows = halo_top + H + halo_bottom), result is
    one (n_attr, H, W) tensor (or ``out``) filled on the current torch stream.  No host copies, no sync."""
    import torch

    assert dem.is_cuda and dem.dim() == 2 and dem.stride(1) == 1
    Hbuf, W = dem.shape
    H = Hbuf - halo_top - halo_bottom
    dt = {torch.float32: np.float32, torch.float64: np.float64}[dem.dtype]
    ctx = ctx or _lib.default_context(dem.device.index)
    if out is None:
        # the callee allocates the outputs, as upstream's engines do (terrain.py:528-666): plane sets of 256 MiB and more come
        # from the library's scattered backing, the form the streaming kernel writes fastest on every box (alloc_planes)
        out = alloc_planes(len(attribute), H, W, dem.dtype, ctx, dem.device)
    ctx.set_stream(torch.cuda.current_stream(dem.device).cuda_stream)
    assert out.shape == (len(attribute), H, W) and out.stride(2) == 1 and out.stride(1) == W and out.is_cuda
    ptrs = {a: _args.ptr(out[i]) for i, a in enumerate(attribute)}  # planes may be row windows of a larger tensor
    launch_terrain(ctx, _args.ptr(dem), dt, H, W, dem.stride(0), halo_top, halo_bottom, resolution, surface_fit,
                   curv_method, list(attribute), tri_method, window_size, hillshade_altitude, hillshade_azimuth,
                   hillshade_z_factor, degrees, {torch.float32: np.float32, torch.float64: np.float64}[out.dtype],
                   ptrs, _lib.DEVICE, window_size_fractal)
    return out


def _deprecated_method(method, surface_fit):
    if method is not None:
        warnings.warn("'method' is deprecated, use 'surface_fit' instead.", DeprecationWarning, stacklevel=3)
        return method
    return surface_fit


# ---- thin wrappers, same signatures as xdem/terrain/terrain.py:693-1571 --------------------------------
def slope(dem, method=None, surface_fit="Florinsky", degrees=True, resolution=None, mp_config=None, engine="hip"):
    """Slope map (terrain.py:694-747)."""
    surface_fit = _deprecated_method(method, surface_fit)
    return get_terrain_attribute(dem, attribute="slope", surface_fit=surface_fit, resolution=resolution,
                                 degrees=degrees, mp_config=mp_config, engine=engine)


def aspect(dem, method=None, surface_fit="Florinsky", degrees=True, mp_config=None, engine="hip"):
    """Aspect map; always computed with resolution=1.0 like the reference (terrain.py:773-836)."""
    surface_fit = _deprecated_method(method, surface_fit)
    return get_terrain_attribute(dem, attribute="aspect", surface_fit=surface_fit, resolution=1.0, degrees=degrees,
                                 mp_config=mp_config, engine=engine)


def hillshade(dem, method=None, surface_fit="Florinsky", azimuth=315.0, altitude=45.0, z_factor=1.0, resolution=None,
              mp_config=None, engine="hip"):
    """Hillshade (terrain.py:867-919)."""
    surface_fit = _deprecated_method(method, surface_fit)
    return get_terrain_attribute(dem, attribute="hillshade", resolution=resolution, surface_fit=surface_fit,
                                 hillshade_azimuth=azimuth, hillshade_altitude=altitude, hillshade_z_factor=z_factor,
                                 mp_config=mp_config, engine=engine)


def curvature(dem, resolution=None, surface_fit="Florinsky", mp_config=None, engine="hip"):
    """Deprecated total curvature (terrain.py:944-991)."""
    warnings.warn("The curvature attribute is deprecated, refer to docs for specific curvature functions.",
                  DeprecationWarning, stacklevel=2)
    return get_terrain_attribute(dem=dem, attribute="curvature", resolution=resolution, surface_fit=surface_fit,
                                 mp_config=mp_config, engine=engine)


def _curv_wrapper(name):
    def f(dem, resolution=None, surface_fit="Florinsky", curv_method="geometric", mp_config=None, engine="hip"):
        return get_terrain_attribute(dem=dem, attribute=name, resolution=resolution, surface_fit=surface_fit,
                                     curv_method=curv_method, mp_config=mp_config, engine=engine)

    f.__name__ = name
    f.__doc__ = f"{name} (xdem/terrain/terrain.py:1016-1447), multiplied by 100."
    return f


profile_curvature = _curv_wrapper("profile_curvature")
tangential_curvature = _curv_wrapper("tangential_curvature")
planform_curvature = _curv_wrapper("planform_curvature")
flowline_curvature = _curv_wrapper("flowline_curvature")
max_curvature = _curv_wrapper("max_curvature")
min_curvature = _curv_wrapper("min_curvature")


def topographic_position_index(dem, window_size=3, mp_config=None, engine="hip"):
    """TPI (terrain.py:1468-1508)."""
    return get_terrain_attribute(dem=dem, attribute="topographic_position_index", window_size=window_size,
                                 mp_config=mp_config, engine=engine)


def roughness(dem, window_size=3, mp_config=None, engine="hip"):
    """Roughness: largest elevation difference inside the window (terrain.py:1600-1640)."""
    return get_terrain_attribute(dem=dem, attribute="roughness", window_size=window_size, mp_config=mp_config, engine=engine)


def rugosity(dem, resolution=None, mp_config=None, engine="hip"):
    """Rugosity: real over planimetric surface area on a 3x3 window, Jenness (2004) (terrain.py:1660-1700)."""
    return get_terrain_attribute(dem=dem, attribute="rugosity", resolution=resolution, mp_config=mp_config, engine=engine)


def fractal_roughness(dem, window_size_fractal=13, mp_config=None, engine="hip"):
    """Fractal roughness: box-counting estimate of the local fractal dimension (1..3), Taud & Parrot (2005)
    (terrain.py:1721-1765)."""
    return get_terrain_attribute(dem=dem, attribute="fractal_roughness", window_size_fractal=window_size_fractal,
                                 mp_config=mp_config, engine=engine)


def texture_shading(dem, alpha: float = 0.8, mp_config=None, engine="hip"):
    """Texture shading, the fractional Laplacian ``|f|^alpha`` of the DEM (Brown 2010) (terrain.py:1783-1840, freq.py:63-148)."""
    return get_terrain_attribute(dem=dem, attribute="texture_shading", texture_alpha=alpha, mp_config=mp_config, engine=engine)


def terrain_ruggedness_index(dem, method="Riley", window_size=3, mp_config=None, engine="hip"):
    """TRI, Riley (topography) or Wilson (bathymetry) (terrain.py:1531-1579)."""
    return get_terrain_attribute(dem=dem, attribute="terrain_ruggedness_index", tri_method=method,
                                 window_size=window_size, mp_config=mp_config, engine=engine)
