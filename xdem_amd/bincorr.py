"""BiasCorr, DirectionalBias and TerrainBias on MI355X -- mirrors of ``xdem.coreg.BiasCorr`` / ``DirectionalBias`` / ``TerrainBias``
(``xdem/coreg/biascorr.py:40-618``; ``_bin_or_and_fit_nd``, ``base.py:906-1050, 2749-2807``) for two rasters on one grid.
Re-exported by ``xdem_amd.coreg``.  ``Deramp`` stays in ``xdem_amd.biascorr``.

``fit``: a dh plan holds the rasters; every variable plane narrows its valid mask (``inlier & finite(ref) & finite(tba) &
finite(every variable)``, base.py:653-661), the subsample is drawn among those pixels, and dh with the variables' values at the
selected pixels is gathered as columns (``csrc/bincorr.hip``).  ``"bin"`` hands the columns to ``nd_binning`` -- for CUDA tensors
without a host round trip --, ``"bin_and_fit"`` runs the optimiser on the binned table, ``"fit"`` on the columns themselves, both on
the host as upstream calls them.

``apply``: the small table of the correction is built on the host -- ``interp_nd_binning``'s grid, the interval table of
``get_perbin_nd_binning``, or the parameters of ``polynomial_1d`` / ``sumsin_1d`` -- and ONE launch computes
``(raster dtype)(elev + corr(variables))`` (``xdemhip_corr_apply``).  A variable is described by its source: a plane, the rotated
coordinate of ``DirectionalBias`` (formed per pixel, never a plane on the device path) or the raster itself
(``TerrainBias("elevation")``).  Any other ``fit_func`` is evaluated on the host, as ``Deramp``'s custom route is.

Not implemented (``NotImplementedError``): ``weights``, point-cloud inputs, more than 3 variables in the fused apply,
row-partitioned (multi-rank) plans.
``rotated_x`` restates geoutils' ``get_xy_rotated`` (geoutils is not vendored): **parity unpinned**, like ``subsample_array``."""
from __future__ import annotations

import ctypes
import inspect
import logging
from collections.abc import Iterable
from typing import Any, Callable

import numpy as np
import scipy.optimize

from . import _args, _lib
from ._args import is_tensor, nan_filled
from ._coregbase import _Step, _with_transform, draw
from .biascorr import DhPlan, _check_weights
from .fit import fit_workflows, polynomial_1d, robust_norder_polynomial_fit, sumsin_1d

MAX_FUSED_VARS = 3


# ---- the rotated coordinate of DirectionalBias ----------------------------------------------------------------------------------
def _resolution(res) -> tuple[float, float]:
    if res is None:
        return 1.0, 1.0
    return (float(res), float(res)) if np.isscalar(res) else (float(res[0]), float(res[1]))


def _rotation(shape, res, angle) -> tuple[float, float, float, float, float]:
    """(cos, sin, res_x, res_y, offset) of ``rotated_x``: the offset is the minimum of the unshifted coordinate, which a
    coordinate that is monotone along both axes takes at one of the four corners (same float64 operations)."""
    H, W = int(shape[0]), int(shape[1])
    rx, ry = _resolution(res)
    theta = np.deg2rad(float(angle))
    c, s = float(np.cos(theta)), float(np.sin(theta))
    corners = [(float(col) * rx) * c + (float(H - 1 - row) * ry) * s for row in (0, H - 1) for col in (0, W - 1)]
    return c, s, rx, ry, float(min(corners))


def rotated_x(shape, res, angle) -> np.ndarray:
    """Along-track coordinate of the pixels of a north-up grid of ``shape`` = (H, W) and ``res`` = (res_x, res_y), for a track at
    ``angle`` degrees: ``xx = col res_x``, ``yy = (H - 1 - row) res_y``, ``xr = xx cos + yy sin``, ``x = xr - min(xr)`` in float64 --
    a restatement of ``geoutils.raster.get_xy_rotated`` (parity unpinned).  The device forms the same value per pixel with the
    same operations (``xdemhip_varsrc``, kind ``XDEMHIP_VAR_ROTATED``), bit for bit."""
    H, W = int(shape[0]), int(shape[1])
    c, s, rx, ry, off = _rotation(shape, res, angle)
    xx = np.arange(W, dtype=np.float64) * rx
    yy = (H - 1 - np.arange(H)).astype(np.float64) * ry
    return ((xx * c)[None, :] + (yy * s)[:, None]) - off


# ---- variables and their sources -------------------------------------------------------------------------------------------------
class _Var:
    """One variable of a correction: ``kind`` "plane" (``plane``: H x W array or CUDA tensor), "rotated" (``rot``: the tuple of
    ``_rotation``) or "raster" (the reference raster in ``fit``, the raster itself in ``apply``)."""

    def __init__(self, kind: str, plane=None, rot=None):
        self.kind, self.plane, self.rot = kind, plane, rot


def _source(var: _Var, plane_ptr=None, plane_code=None) -> _lib.VarSrc:
    if var.kind == "plane":
        return _lib.VarSrc(_lib.VAR_PLANE, plane_code, plane_ptr, 0.0, 0.0, 0.0, 0.0, 0.0)
    if var.kind == "rotated":
        c, s, rx, ry, off = var.rot
        return _lib.VarSrc(_lib.VAR_ROTATED, 0, None, c, s, rx, ry, off)
    return _lib.VarSrc(_lib.VAR_REF, 0, None, 0.0, 0.0, 0.0, 0.0, 0.0)


def _host_plane(var: _Var, elev: np.ndarray) -> np.ndarray:
    """The variable as a host plane (the host routes of ``apply``)."""
    if var.kind == "plane":
        return var.plane.cpu().numpy() if is_tensor(var.plane) else nan_filled(var.plane)
    if var.kind == "rotated":
        c, s, rx, ry, off = var.rot
        H, W = elev.shape
        return ((np.arange(W, dtype=np.float64) * rx * c)[None, :] + ((H - 1 - np.arange(H)).astype(np.float64) * ry * s)[:, None]) - off
    return elev


# ---- the fused apply ----------------------------------------------------------------------------------------------------------------
def corr_apply(elev, kind: int, variables: list, n_tab, a=None, b=None, table=None, decided=None, ctx: _lib.Context | None = None):
    """``(elev dtype)(elev + corr(variables))`` in one launch (``xdemhip_corr_apply``).  ``elev``: a 2-D NumPy array or a
    contiguous 2-D float32 / float64 CUDA tensor (then the planes of ``variables`` are moved to its device and the result is a
    tensor).  ``kind``: ``_lib.CORR_GRID`` (``n_tab`` points per axis, ``a`` the axes concatenated, ``table`` the grid values),
    ``_lib.CORR_PERBIN`` (``n_tab`` intervals per variable, ``a`` / ``b`` their ends, ``table`` / ``decided`` per bin),
    ``_lib.CORR_POLY`` / ``_lib.CORR_SUMSIN`` (``table`` = the parameters).  Returns (out, pixels in a bin without a row)."""
    if len(variables) > MAX_FUSED_VARS:
        raise NotImplementedError(f"the fused apply takes at most {MAX_FUSED_VARS} variables, got {len(variables)}")
    device = is_tensor(elev)
    if device:
        import torch

        _args.device_float(elev, "device elev must be a contiguous 2D float32 / float64 CUDA tensor")
        out = torch.empty_like(elev, memory_format=torch.contiguous_format)
        ctx = ctx or _lib.default_context(elev.device.index)
    else:
        elev = _args.host_float(elev)
        if elev.ndim != 2:
            raise ValueError("elev must be a 2D array")
        out = np.empty_like(elev)
        ctx = ctx or _lib.default_context()
    shape = tuple(elev.shape)
    keep, srcs = [], []
    for v in variables:
        if v.kind != "plane":
            srcs.append(_source(v))
            continue
        p_ptr, p_code, p_shape, t = _args.plane_in_space(v.plane, elev.device if device else None)
        if p_shape != shape:
            raise ValueError(f"a bias variable has shape {p_shape}, the raster {shape}")
        keep.append(t)
        srcs.append(_source(v, p_ptr, p_code))
    n_var = len(srcs)
    arr_src = (_lib.VarSrc * n_var)(*srcs)
    n_tab = [int(n) for n in n_tab]
    nt = (ctypes.c_int * len(n_tab))(*n_tab)
    as_d = lambda x: None if x is None else np.ascontiguousarray(x, dtype=np.float64)  # noqa: E731
    a, b, table = as_d(a), as_d(b), as_d(table)
    decided = None if decided is None else np.ascontiguousarray(decided, dtype=np.uint8)
    missing = ctypes.c_int64()
    with ctx.call_lock:
        if device:
            _args.synchronize_torch(elev)   # (the inputs are complete; the call itself returns synchronised)
        rc = ctx._L.xdemhip_corr_apply(ctx.handle, _args.ptr(elev), _args.code(elev), shape[0], shape[1], int(kind), n_var, arr_src, nt,
                                       _args.dp(a), _args.dp(b), _args.dp(table), _args.chars(decided), _args.ptr(out), ctypes.byref(missing),
                                       _args.space(elev))
    ctx.check(rc)
    del keep
    return out, int(missing.value)


# ---- the fit on columns (base.py:906-1050) ---------------------------------------------------------------------------------------
def _check_bias_vars(params: dict, names: list) -> None:
    nd = params["nd"]
    if nd is not None and len(names) != nd:
        raise ValueError("A number of {} variable(s) has to be provided through the argument 'bias_vars', got {}.".format(nd, len(names)))
    if params["bias_var_names"] is not None and not sorted(names) == sorted(params["bias_var_names"]):
        raise ValueError("The keys of `bias_vars` do not match the `bias_var_names` defined during instantiation: {}."
                         .format(params["bias_var_names"]))


def _bin_sizes_in_order(params: dict, names: list):
    """``bin_sizes`` as ``nd_binning`` takes it: a dict is ordered like the variables, every entry made an array (base.py:959-968 --
    an INTEGER entry becomes a 0-d array, which SciPy refuses for two variables and more with its own TypeError: reproduced)."""
    bs = params["bin_sizes"]
    return tuple(np.array(bs[name]) for name in names) if isinstance(bs, dict) else bs


def _bin_or_and_fit_nd(fit_or_bin: str, params: dict, values, columns: dict, weights=None, ctx=None, **kwargs: Any):
    """``_bin_or_and_fit_nd`` (base.py:906-1050) on the gathered columns: ``values`` = dh, ``columns`` = {name: values of the
    variable}, both NumPy arrays or 1-D CUDA tensors of one length.  Returns (DataFrame | None, optimiser results | None)."""
    import pandas as pd

    from .spatialstats import nd_binning

    _check_weights(weights)
    if columns is None:
        raise ValueError("At least one `bias_var` should be passed to the fitting function, got None.")
    names = list(columns.keys())
    _check_bias_vars(params, names)
    if fit_or_bin in ["fit", "bin_and_fit"]:
        if "random_state" not in inspect.getfullargspec(params["fit_optimizer"]).args and "random_state" in kwargs:
            kwargs.pop("random_state")
    to_host = lambda c: c.cpu().numpy() if is_tensor(c) else np.asarray(c)  # noqa: E731
    df, results = None, None
    if fit_or_bin == "fit":
        logging.debug("Estimating alignment along variables %s by fitting with function %s.", ", ".join(names), params["fit_func"].__name__)
        results = params["fit_optimizer"](f=params["fit_func"], xdata=np.array([to_host(c).flatten() for c in columns.values()]).squeeze(),
                                          ydata=to_host(values).flatten(), sigma=None, absolute_sigma=True, **kwargs)
        return df, results
    bin_sizes = _bin_sizes_in_order(params, names)
    logging.debug("Estimating alignment along variables %s by binning with statistic %s.", ", ".join(names), params["bin_statistic"].__name__)
    df = nd_binning(values=values, list_var=list(columns.values()), list_var_names=names, list_var_bins=bin_sizes,
                    statistics=(params["bin_statistic"], "count"), ctx=ctx)
    if fit_or_bin == "bin":
        return df, results
    # the fit sees the N-D block only: the mid points of its bins and their statistic
    df_nd = df[df.nd == len(names)]
    new_vars = [pd.IntervalIndex(df_nd[name]).mid.values for name in names]
    new_diff = df_nd[params["bin_statistic"].__name__].values
    ok = np.logical_and.reduce((np.isfinite(new_diff), *(np.isfinite(v) for v in new_vars)))
    if np.all(~ok):
        raise ValueError("Only NaN values after binning, did you pass the right bin edges?")
    results = params["fit_optimizer"](f=params["fit_func"], xdata=np.array([v[ok].flatten() for v in new_vars]).squeeze(),
                                      ydata=new_diff[ok].flatten(), sigma=None, absolute_sigma=True, **kwargs)
    return df, results


# ---- BiasCorr ----------------------------------------------------------------------------------------------------------------------
class BiasCorr(_Step):
    """Bias correction along any number and type of variables by binning, fitting or both (``xdem.coreg.BiasCorr``,
    biascorr.py:40-311).  The results are in ``meta["outputs"]["fitorbin"]``: ``bin_dataframe`` for ``"bin"``, ``fit_params`` (and
    ``fit_perr`` with ``curve_fit``) for ``"fit"`` / ``"bin_and_fit"``; a named workflow adds
    ``meta["outputs"]["specific"]["best_poly_order" | "best_nb_sin_freq"]``."""

    _is_affine = False

    def __init__(self, fit_or_bin: str = "fit", fit_func: Callable[..., Any] | str = "norder_polynomial",
                 fit_optimizer: Callable[..., Any] = scipy.optimize.curve_fit, bin_sizes: int | dict = 10,
                 bin_statistic: Callable[..., Any] = np.nanmedian, bin_apply_method: str = "linear", bias_var_names: Iterable[str] = None,
                 subsample: float | int = 1.0):
        if fit_or_bin not in ["fit", "bin", "bin_and_fit"]:
            raise ValueError(f"Argument `fit_or_bin` must be 'bin_and_fit', 'fit' or 'bin', got {fit_or_bin}.")
        if fit_or_bin in ["fit", "bin_and_fit"]:
            if not (callable(fit_func) or (isinstance(fit_func, str) and fit_func in fit_workflows.keys())):
                raise TypeError("Argument `fit_func` must be a function (callable) or the string '{}', got {}."
                                .format("', '".join(fit_workflows.keys()), type(fit_func)))
            if not callable(fit_optimizer):
                raise TypeError("Argument `fit_optimizer` must be a function (callable), got {}.".format(type(fit_optimizer)))
            if isinstance(fit_func, str):   # a named workflow brings its optimiser
                fit_optimizer = fit_workflows[fit_func]["optimizer"]
                fit_func = fit_workflows[fit_func]["func"]
        if fit_or_bin in ["bin", "bin_and_fit"]:
            if not (isinstance(bin_sizes, int) or (isinstance(bin_sizes, dict) and all(isinstance(v, (int, Iterable)) for v in bin_sizes.values()))):
                raise TypeError("Argument `bin_sizes` must be an integer, or a dictionary of integers or iterables, got {}."
                                .format(type(bin_sizes)))
            if not callable(bin_statistic):
                raise TypeError("Argument `bin_statistic` must be a function (callable), got {}.".format(type(bin_statistic)))
            if not isinstance(bin_apply_method, str):
                raise TypeError("Argument `bin_apply_method` must be the string 'linear' or 'per_bin', got {}.".format(type(bin_apply_method)))
        names = list(bias_var_names) if bias_var_names is not None else None
        if fit_or_bin == "fit":
            fitorbin = {"fit_func": fit_func, "fit_optimizer": fit_optimizer, "bias_var_names": names}
        elif fit_or_bin == "bin":
            fitorbin = {"bin_sizes": bin_sizes, "bin_statistic": bin_statistic, "bin_apply_method": bin_apply_method, "bias_var_names": names}
        else:
            fitorbin = {"fit_func": fit_func, "fit_optimizer": fit_optimizer, "bin_sizes": bin_sizes, "bin_statistic": bin_statistic,
                        "bias_var_names": names}
        fitorbin["fit_or_bin"] = fit_or_bin
        fitorbin["nd"] = len(names) if names is not None else None
        self.meta: dict[str, Any] = {
            "inputs": {"random": {"subsample": subsample}, "fitorbin": fitorbin, "iterative": {}, "specific": {}, "affine": {}},
            "outputs": {},
        }
        self._needs_vars = True

    # -- what the subclasses change: where the variables come from --
    def _fit_vars(self, ref, bias_vars, resolution) -> dict:
        if bias_vars is None:
            raise ValueError("At least one `bias_var` should be passed to the fitting function, got None.")
        return {name: _Var("plane", plane) for name, plane in bias_vars.items()}

    def _apply_vars(self, elev, bias_vars, resolution) -> dict:
        if bias_vars is None:
            raise ValueError("At least one `bias_var` should be passed to the `apply` function, got None.")
        return {name: _Var("plane", plane) for name, plane in bias_vars.items()}

    def fit(self, reference_elev, to_be_aligned_elev, inlier_mask=None, bias_vars=None, weights=None, subsample=None, transform=None,
            crs=None, area_or_point=None, z_name=None, random_state=None, resolution=None, **kwargs: Any):
        """Estimate the correction of dh = reference - to_be_aligned along the variables (``Coreg.fit`` with ``_fit_rst_rst``,
        biascorr.py:167-231).  Rasters: 2-D NumPy arrays, or contiguous CUDA tensors of one dtype (then the columns stay on the
        device).  ``resolution`` = (res_x, res_y) is what the rotated coordinate and the terrain attributes read of a transform."""
        _check_weights(weights)
        for e in (reference_elev, to_be_aligned_elev):
            if hasattr(e, "columns") or hasattr(e, "geometry"):
                raise NotImplementedError("Point-cloud inputs are not implemented for the bias corrections here: two rasters on one grid.")
        if subsample is not None:
            self.meta["inputs"]["random"]["subsample"] = subsample
        if self.meta["inputs"]["random"]["subsample"] != 1:
            self.meta["inputs"]["random"]["random_state"] = random_state
        fb = self.meta["inputs"]["fitorbin"]
        variables = self._fit_vars(reference_elev, bias_vars, resolution)
        names = list(variables.keys())
        _check_bias_vars(fb, names)
        if fb["bias_var_names"] is None:
            fb["bias_var_names"] = names
        with DhPlan(reference_elev, to_be_aligned_elev, inlier_mask) as plan:
            if getattr(plan.ctx, "_hook", None) is not None:   # (reduction hooks installed: the rasters are one rank's rows)
                raise NotImplementedError("Row-partitioned (multi-rank) plans are not implemented for the bias corrections.")
            keep, srcs = [], []
            for v in variables.values():
                if v.kind == "plane":
                    ptr, code, arr = plan._plane(v.plane)
                    keep.append(arr)
                    v.plane = arr
                    plan.restrict_finite(arr)
                    srcs.append(_source(v, ptr, code))
                else:
                    srcs.append(_source(v))
            n = draw(plan, self.meta["inputs"]["random"]["subsample"], self.meta["inputs"]["random"].get("random_state"))
            dh, cols = plan.var_columns(srcs)
            del keep
            df, results = _bin_or_and_fit_nd(fb["fit_or_bin"], fb, dh, dict(zip(names, cols)), None, plan.ctx, **kwargs)
        self.meta["outputs"]["fitorbin"] = {}
        if fb["fit_or_bin"] in ["fit", "bin_and_fit"] and results is not None:
            params = results[0]
            if fb["fit_optimizer"] in (w["optimizer"] for w in fit_workflows.values()):
                key = "best_poly_order" if fb["fit_optimizer"] == robust_norder_polynomial_fit else "best_nb_sin_freq"
                self.meta["outputs"]["specific"] = {key: results[1]}
            elif fb["fit_optimizer"] == scipy.optimize.curve_fit:
                self.meta["outputs"]["fitorbin"].update({"fit_perr": np.sqrt(np.diag(results[1]))})
            self.meta["outputs"]["fitorbin"].update({"fit_params": params})
        elif fb["fit_or_bin"] in ["bin", "bin_and_fit"] and df is not None:
            self.meta["outputs"]["fitorbin"].update({"bin_dataframe": df})
        self.meta["outputs"]["random"] = {"subsample_final": int(n)}
        return self

    def apply(self, elev, resolution=None, resample: bool = True, *, bias_vars=None, resampling: str = "bilinear", transform=None, crs=None,
              z_name: str = "z", **kwargs: Any):
        """``elev + corr(variables)`` in the input dtype, shape (H, W) (biascorr.py:261-311 and the cast of base.py:491); with
        ``transform=`` the call returns ``(array, transform)``.  ``min_count=`` (keyword) reaches ``interp_nd_binning`` as upstream."""
        if "fitorbin" not in self.meta["outputs"]:
            raise AssertionError(".fit() does not seem to have been called yet")
        if hasattr(elev, "columns") or hasattr(elev, "geometry"):
            raise NotImplementedError("Point-cloud inputs are not implemented for the bias corrections here.")
        fb = self.meta["inputs"]["fitorbin"]
        variables = self._apply_vars(elev, bias_vars, resolution)
        names = list(variables.keys())
        if not sorted(names) == sorted(fb["bias_var_names"]):
            raise ValueError("The keys of `bias_vars` do not match the `bias_var_names` defined during instantiation or fitting: {}."
                             .format(fb["bias_var_names"]))
        out = self._corrected(elev, variables, names, kwargs.get("min_count", 0))
        return _with_transform(out, transform)

    def _corrected(self, elev, variables: dict, names: list, min_count):
        from .spatialstats import _perbin_tables, interp_nd_binning

        fb = self.meta["inputs"]["fitorbin"]
        outputs = self.meta["outputs"]["fitorbin"]
        var_list = list(variables.values())
        if fb["fit_or_bin"] in ["fit", "bin_and_fit"]:
            params = np.asarray(outputs["fit_params"], dtype=np.float64)
            if fb["fit_func"] is polynomial_1d and len(var_list) == 1 and 1 <= params.size <= 64:
                return corr_apply(elev, _lib.CORR_POLY, var_list, [params.size], table=params)[0]
            if fb["fit_func"] is sumsin_1d and len(var_list) == 1 and params.size % 3 == 0 and 3 <= params.size <= 192:
                return corr_apply(elev, _lib.CORR_SUMSIN, var_list, [params.size], table=params)[0]
            # any other function: evaluated on the host, as upstream does (slow; exists for compatibility)
            arr = _elev_host(elev)
            corr = fb["fit_func"](tuple(_host_plane(v, arr) for v in var_list), *outputs["fit_params"])
            return _like(elev, (arr + np.asarray(corr).reshape(arr.shape)).astype(arr.dtype))
        if len(var_list) > MAX_FUSED_VARS:
            raise NotImplementedError(f"the fused apply takes at most {MAX_FUSED_VARS} variables, got {len(var_list)}")
        df = outputs["bin_dataframe"]
        if fb["bin_apply_method"] == "linear":
            interp = interp_nd_binning(df=df, list_var_names=names, statistic=fb["bin_statistic"], min_count=min_count)
            return corr_apply(elev, _lib.CORR_GRID, var_list, [len(g) for g in interp.grid], a=np.concatenate(interp.grid), table=interp.values)[0]
        # per bin: the lookup of get_perbin_nd_binning (upstream calls it with its default min_count = 0 here, biascorr.py:302-307)
        elev_dtype = np.dtype(np.float32 if "float32" in str(elev.dtype) else np.float64) if is_tensor(elev) else _elev_host(elev).dtype
        dts = [_var_dtype(v, elev_dtype) for v in var_list]
        stat_name = fb["bin_statistic"] if isinstance(fb["bin_statistic"], str) else fb["bin_statistic"].__name__
        if stat_name not in df.columns:
            raise ValueError('Statistic "' + stat_name + '" does not exist in the provided dataframe.')
        counts, left, right, table, decided, disjoint, _ = _perbin_tables(df, dts, names, stat_name, 0)
        if table is None:
            raise ValueError("Dataframe is empty.")
        if not disjoint:
            raise NotImplementedError("the fused apply needs pairwise disjoint bin intervals (what nd_binning writes)")
        out, missing = corr_apply(elev, _lib.CORR_PERBIN, var_list, counts, a=left, b=right, table=table, decided=decided)
        if missing:
            raise IndexError("index 0 is out of bounds for axis 0 with size 0")   # upstream's `.values[0]` of a bin without a row
        return out

    @property
    def is_affine(self) -> bool:
        return False

    def to_matrix(self):
        raise NotImplementedError("A bias correction is not an affine transformation: it has no matrix.")


def _elev_host(elev) -> np.ndarray:
    arr = elev.cpu().numpy() if is_tensor(elev) else nan_filled(elev)
    return arr if arr.dtype in _args.FLOATS else arr.astype(np.float32)


def _like(elev, out: np.ndarray):
    return _args.same_space(out, elev)


def _var_dtype(v: _Var, elev_dtype: np.dtype) -> np.dtype:
    """The dtype NumPy would compare the variable in (what the interval ends of the per-bin lookup are rounded to)."""
    if v.kind == "rotated":
        return np.dtype(np.float64)
    if v.kind == "raster":
        return elev_dtype
    dt = _args.np_dtype(v.plane)
    return dt if dt in _args.FLOATS else np.dtype(np.float64)


# ---- DirectionalBias ---------------------------------------------------------------------------------------------------------------
class DirectionalBias(BiasCorr):
    """Bias correction along a direction, for example along- or across-track of a satellite (``xdem.coreg.DirectionalBias``,
    biascorr.py:314-446).  The variable ``"angle"`` is ``rotated_x(shape, resolution, angle)``, formed per pixel on the device."""

    def __init__(self, angle: float = 0, fit_or_bin: str = "bin_and_fit", fit_func: Callable[..., Any] | str = "nfreq_sumsin",
                 fit_optimizer: Callable[..., Any] = scipy.optimize.curve_fit, bin_sizes: int | dict = 100,
                 bin_statistic: Callable[..., Any] = np.nanmedian, bin_apply_method: str = "linear", subsample: float | int = 1.0):
        super().__init__(fit_or_bin, fit_func, fit_optimizer, bin_sizes, bin_statistic, bin_apply_method, ["angle"], subsample)
        self.meta["inputs"]["specific"]["angle"] = angle
        self._needs_vars = False

    def _rotated(self, raster, resolution) -> dict:
        logging.info("Estimating rotated coordinates.")
        return {"angle": _Var("rotated", rot=_rotation(tuple(raster.shape), resolution, self.meta["inputs"]["specific"]["angle"]))}

    def _fit_vars(self, ref, bias_vars, resolution) -> dict:
        return self._rotated(ref, resolution)

    def _apply_vars(self, elev, bias_vars, resolution) -> dict:
        return self._rotated(elev, resolution)


# ---- TerrainBias -------------------------------------------------------------------------------------------------------------------
class TerrainBias(BiasCorr):
    """Bias correction along a terrain attribute, such as elevation or curvature (``xdem.coreg.TerrainBias``, biascorr.py:449-618).
    ``"elevation"`` reads the raster itself; any other attribute comes from ``xdem_amd.terrain`` at ``resolution``; a plane passed
    in ``bias_vars`` under the attribute's name wins."""

    def __init__(self, terrain_attribute: str = "max_curvature", fit_or_bin: str = "bin", fit_func: Callable[..., Any] | str = "norder_polynomial",
                 fit_optimizer: Callable[..., Any] = scipy.optimize.curve_fit, bin_sizes: int | dict = 100,
                 bin_statistic: Callable[..., Any] = np.nanmedian, bin_apply_method: str = "linear", subsample: float | int = 1.0):
        super().__init__(fit_or_bin, fit_func, fit_optimizer, bin_sizes, bin_statistic, bin_apply_method, [terrain_attribute], subsample)
        self.meta["inputs"]["specific"]["terrain_attribute"] = terrain_attribute
        self._needs_vars = False

    def _attribute(self, raster, resolution) -> _Var:
        attr = self.meta["inputs"]["specific"]["terrain_attribute"]
        if attr == "elevation":
            return _Var("raster")
        from . import terrain

        res = _resolution(resolution)
        if is_tensor(raster):
            if res[0] != res[1]:
                raise ValueError(f"The terrain attributes on the device take one resolution for X and Y ({res} was given).")
            return _Var("plane", terrain.terrain_attributes_device(raster, [attr], resolution=res[0])[0])
        return _Var("plane", terrain.get_terrain_attribute(nan_filled(raster), attr, resolution=res))

    def _fit_vars(self, ref, bias_vars, resolution) -> dict:
        attr = self.meta["inputs"]["specific"]["terrain_attribute"]
        if bias_vars is not None and attr in bias_vars:
            return {attr: _Var("plane", bias_vars[attr])}
        return {attr: self._attribute(ref, resolution)}

    def _apply_vars(self, elev, bias_vars, resolution) -> dict:
        if bias_vars is not None:
            return {name: _Var("plane", plane) for name, plane in bias_vars.items()}
        return {self.meta["inputs"]["specific"]["terrain_attribute"]: self._attribute(elev, resolution)}
