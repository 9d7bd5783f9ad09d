"""What ``xdem_amd.coreg`` (NuthKaab) and ``xdem_amd.biascorr`` (Deramp, VerticalShift) share: the random subsample of the valid
pixels, ``apply_translation``, and the steps' common base with the pipeline they form (``xdem.coreg.CoregPipeline``, base.py:2008-2019,
2880-3190).  The raster-pair front of their device plans (``_args.raster_pair``) and the plans' lifetime (``_lib._Plan``) are
re-exported here.  Both modules re-export what their users import."""
from __future__ import annotations

import copy as _copy
import inspect
import logging
import warnings
from typing import Any

import numpy as np

from . import _args, _lib
from ._args import RasterPair, raster_pair  # noqa: F401  (the plans' front; imported from here by the modules that build plans)
from ._lib import _Plan  # noqa: F401  (and their lifetime)

NO_VALID = ("There is no valid points common to the input and auxiliary data (bias variables, or "
            "derivatives required for this method, for example slope, aspect, etc).")


# ---- the random subsample ---------------------------------------------------------------------------------------------------------
def subsample_valid_mask(valid_mask: np.ndarray, subsample: float | int, random_state=None) -> np.ndarray:
    """Boolean mask of a random subsample of the valid pixels (``_get_subsample_on_valid_mask``, xdem/coreg/base.py:577-617).
    The draw itself is geoutils' ``subsample_array`` (un-vendored, absent here); its published rule is restated --
    ``rng = default_rng(random_state)``, ``n = int(subsample * n_valid)`` for 0 < subsample <= 1 else ``int(subsample)``,
    capped at n_valid, ``rng.choice(flat valid indices, n, replace=False)`` -- **parity unpinned**."""
    n_valid = int(np.count_nonzero(valid_mask))
    if subsample == 1 and n_valid > 0:
        return valid_mask
    ranks = subsample_ranks(n_valid, subsample, random_state)
    valids = np.flatnonzero(valid_mask.ravel())
    out = np.zeros(valid_mask.size, dtype=bool)
    out[valids[ranks]] = True
    return out.reshape(valid_mask.shape)


def subsample_ranks(n_valid: int, subsample: float | int, random_state=None) -> np.ndarray:
    """The draw of ``subsample_valid_mask`` as RANKS among the valid pixels: ``rng.choice(valids, n, replace=False)`` is
    ``valids[rng.choice(len(valids), n, replace=False)]`` -- NumPy draws the positions from the population SIZE and indexes the array
    with them (same generator stream, same order; CPU test) -- so the ranks need only the count of valid pixels, not the mask:
    the device turns them into pixels (``NKPlan.subsample``) and the mask stays where it is."""
    if n_valid == 0:
        raise ValueError(NO_VALID)
    if subsample <= 0:
        raise ValueError("`subsample` must be > 0")
    npoints = int(subsample * n_valid) if subsample <= 1 else int(subsample)
    npoints = min(npoints, n_valid)
    rng = np.random.default_rng(random_state)
    return rng.choice(n_valid, npoints, replace=False)


def draw(plan, subsample, random_state) -> int:
    """The random subsample of upstream's ``_get_subsample_on_valid_mask`` (base.py:577-617; geoutils' draw restated by
    ``subsample_ranks``) applied to a device plan (``NKPlan`` / ``DhPlan``); returns the number of pixels the fit uses."""
    if plan.n_valid == 0:
        raise ValueError(NO_VALID)
    if subsample == 1:
        return plan.n_valid
    ranks = subsample_ranks(plan.n_valid, subsample, random_state)
    if ranks.size == plan.n_valid:   # every valid pixel drawn: the whole-raster route covers the same set
        return plan.n_valid
    return plan.subsample(ranks)


def apply_translation(elev: np.ndarray, shift_x: float, shift_y: float, shift_z: float, resolution, resample: bool = True,
                      ctx: _lib.Context | None = None) -> np.ndarray:
    """Apply a pure translation to a DEM array (``Coreg.apply`` for ``shift_x / shift_y / shift_z``): with
    ``resample=True`` the shifted DEM is bilinearly resampled onto its original grid
    (``_apply_matrix_rst`` case 2 + ``_reproject_horizontal_shift_samecrs``, xdem/coreg/base.py:1522-1570, 1615-1655):
    ``out(r, c) = elev(r + shift_y / res_y, c - shift_x / res_x) + shift_z``.  Without resampling only ``shift_z`` is
    added (the reference then just moves the geotransform)."""
    arr = _args.host_float(elev)
    from .spatialstats import _count_finite   # (np.isfinite over the raster on the library's host threads: 7 ms against 0.1 s at 20000^2)

    if _count_finite(arr)[0] == 0:
        raise ValueError("Input DEM has all nans.")
    if not resample:
        return arr + arr.dtype.type(shift_z)
    res = (float(resolution), float(resolution)) if np.isscalar(resolution) else (float(resolution[0]), float(resolution[1]))
    ctx = ctx or _lib.default_context()
    out = np.empty_like(arr)
    ctx.check(ctx._L.xdemhip_shift_bilinear(ctx.handle, _args.ptr(arr), _args.code(arr), arr.shape[0], arr.shape[1], float(shift_y) / res[1],
                                            -float(shift_x) / res[0], float(shift_z), _args.ptr(out), _lib.HOST))
    return out


# ---- the coregistration steps --------------------------------------------------------------------------------------------------
class _Step:
    """What NuthKaab, Deramp, VerticalShift and CoregPipeline share with ``xdem.coreg.Coreg``: copy, ``+``, fit_and_apply."""

    def copy(self):
        """Identical, independent copy (base.py:1999-2006)."""
        new = self.__new__(type(self))
        new.__dict__ = {k: _copy.deepcopy(v) for k, v in self.__dict__.items()}
        return new

    def __add__(self, other) -> "CoregPipeline":
        """``Coreg.__add__`` (base.py:2008-2019): a two-step pipeline; an ``initial_shift`` of either step is dropped."""
        if not isinstance(other, _Step):
            raise ValueError(f"Incompatible add type: {type(other)}. Expected 'Coreg' subclass")
        for m in (self, other):
            if "affine" in m.meta["inputs"] and "initial_shift" in m.meta["inputs"]["affine"]:
                del m.meta["inputs"]["affine"]["initial_shift"]
        return CoregPipeline([self, other])

    def fit_and_apply(self, reference_elev, to_be_aligned_elev, inlier_mask=None, bias_vars=None, weights=None, subsample=None,
                      transform=None, crs=None, area_or_point=None, z_name: str = "z", resample: bool = True,
                      resampling: str = "bilinear", random_state=None, fit_kwargs=None, apply_kwargs=None):
        """``Coreg.fit_and_apply`` (base.py:2482-2590): fit, then apply to the to-be-aligned elevations."""
        fit_kwargs = dict(fit_kwargs or {})
        apply_kwargs = dict(apply_kwargs or {})
        self.fit(reference_elev, to_be_aligned_elev, inlier_mask=inlier_mask, bias_vars=bias_vars, weights=weights, subsample=subsample,
                 transform=transform, crs=crs, area_or_point=area_or_point, z_name=z_name, random_state=random_state, **fit_kwargs)
        if "resolution" in fit_kwargs:
            apply_kwargs.setdefault("resolution", fit_kwargs["resolution"])
        return self.apply(to_be_aligned_elev, bias_vars=bias_vars, resample=resample, resampling=resampling, transform=transform, crs=crs,
                          z_name=z_name, **apply_kwargs)


def _with_transform(out, transform):
    return out if transform is None else (out, transform)


# ---- CoregPipeline --------------------------------------------------------------------------------------------------------------
class CoregPipeline(_Step):
    """A sequential set of co-registration steps (``xdem.coreg.CoregPipeline``, base.py:2880-3190)."""

    def __init__(self, pipeline: list) -> None:
        self.pipeline = list(pipeline)
        self.meta: dict[str, Any] = {"inputs": {}, "outputs": {}}
        self._fit_called = False
        self._needs_vars = any(getattr(c, "_needs_vars", False) for c in self.pipeline)

    def __repr__(self) -> str:
        return f"Pipeline: {self.pipeline}"

    def __iter__(self):
        yield from self.pipeline

    def copy(self) -> "CoregPipeline":
        """Identical, independent copy: every step copied (base.py:2916-2923)."""
        new = self.__new__(type(self))
        new.__dict__ = {k: _copy.deepcopy(v) for k, v in self.__dict__.items() if k != "pipeline"}
        new.pipeline = [step.copy() for step in self.pipeline]
        return new

    def __add__(self, other) -> "CoregPipeline":
        """Append a step or the steps of a list / pipeline (base.py:3166-3180); an ``initial_shift`` of any step is dropped."""
        other = [other] if isinstance(other, _Step) else list(other)
        steps = self.pipeline + other
        for m in steps:
            if "affine" in m.meta["inputs"] and "initial_shift" in m.meta["inputs"]["affine"]:
                del m.meta["inputs"]["affine"]["initial_shift"]
        return CoregPipeline(steps)

    def _parse_bias_vars(self, step: int, bias_vars: dict | None) -> dict:
        """The bias variables of one step that needs them, picked from the pipeline's (base.py:2930-2969, same messages)."""
        nb_needs_vars = sum(bool(getattr(c, "_needs_vars", False)) for c in self.pipeline)
        coreg = self.pipeline[step]
        var_names = coreg.meta["inputs"]["fitorbin"]["bias_var_names"]
        if bias_vars is None:
            msg = f"No `bias_vars` passed to .fit() for bias correction step {coreg.__class__} of the pipeline."
            if nb_needs_vars > 1:
                msg += (" As you are using several bias correction steps requiring `bias_vars`, don't forget to "
                        "explicitly define their `bias_var_names` during "
                        "instantiation, e.g. {}(bias_var_names=['slope']).".format(coreg.__class__.__name__))
            raise ValueError(msg)
        if var_names is None and nb_needs_vars > 1:
            raise ValueError("When using several bias correction steps requiring `bias_vars` in a pipeline,"
                             "the `bias_var_names` need to be explicitly defined at each step's "
                             "instantiation, e.g. {}(bias_var_names=['slope']).".format(coreg.__class__.__name__))
        if var_names is None:   # (one step, names left open: it takes every variable and records their names at its fit)
            return dict(bias_vars)
        if not all(n in bias_vars.keys() for n in var_names):
            raise ValueError("Not all keys of `bias_vars` in .fit() match the `bias_var_names` defined during "
                             "instantiation of the bias correction step {}: {}.".format(coreg.__class__, var_names))
        return {n: bias_vars[n] for n in var_names}

    def fit(self, reference_elev, to_be_aligned_elev, inlier_mask=None, bias_vars=None, weights=None, subsample=None, transform=None,
            crs=None, area_or_point=None, z_name=None, random_state=None, **kwargs: Any) -> "CoregPipeline":
        """Fit every step on the output of the previous step's ``apply`` (base.py:2967-3050); the last step is not applied.
        ``resolution=`` (keyword) reaches every step's fit and apply, like ``transform``.  ``bias_vars`` go to the steps that need
        them (``BiasCorr``), to their fit and to their apply; the other steps never see them."""
        argspec = [inspect.getfullargspec(c.__class__) for c in self.pipeline]
        sub_meta = [c.meta["inputs"]["random"]["subsample"] for c in self.pipeline]
        sub_is_default = [argspec[i].defaults[argspec[i].args.index("subsample") - 1] == sub_meta[i] for i in range(len(argspec))]
        if subsample is not None and not all(sub_is_default):
            warnings.warn(
                "Subsample argument passed to fit() will override non-default subsample values defined for"
                " individual steps of the pipeline. To silence this warning: only define 'subsample' in "
                "either fit(subsample=...) or instantiation e.g., VerticalShift(subsample=...)."
            )
            warnings.filterwarnings("ignore", message="Subsample argument passed to*", category=UserWarning)
        extra = {"resolution": kwargs.pop("resolution")} if "resolution" in kwargs else {}
        tba_mod = to_be_aligned_elev
        out_transform = transform
        for i, step in enumerate(self.pipeline):
            logging.debug("Running pipeline step: %d / %d", i + 1, len(self.pipeline))
            step_vars = {"bias_vars": self._parse_bias_vars(i, bias_vars)} if getattr(step, "_needs_vars", False) else {}
            step.fit(reference_elev=reference_elev, to_be_aligned_elev=tba_mod, inlier_mask=inlier_mask, transform=out_transform, crs=crs,
                     z_name=z_name, weights=weights, subsample=subsample, random_state=random_state, **step_vars, **extra, **kwargs)
            if i != len(self.pipeline) - 1:
                res = step.apply(elev=tba_mod, transform=out_transform, crs=crs, z_name=z_name, **step_vars, **extra)
                if hasattr(tba_mod, "geometry"):   # (a cloud on the to-be-aligned side is moved by the step's matrix and has no transform)
                    tba_mod = res
                elif out_transform is None:
                    tba_mod = res
                else:
                    tba_mod, out_transform = res
        self._fit_called = True
        return self

    def apply(self, elev, bias_vars=None, resample: bool = True, resampling: str = "bilinear", transform=None, crs=None, z_name=None,
              **kwargs: Any):
        """Apply the steps in order (base.py:3106-3150).  With ``transform=`` returns ``(array, transform)``, else the array."""
        if not self._fit_called:
            raise AssertionError(".fit() does not seem to have been called yet")
        elev_mod = elev
        out_transform = transform
        for i, step in enumerate(self.pipeline):
            step_vars = {"bias_vars": self._parse_bias_vars(i, bias_vars)} if getattr(step, "_needs_vars", False) else {}
            res = step.apply(elev=elev_mod, transform=out_transform, crs=crs, z_name=z_name, resample=resample, resampling=resampling,
                             **step_vars, **kwargs)
            if hasattr(elev_mod, "geometry"):
                elev_mod = res
            elif out_transform is None:
                elev_mod = res
            else:
                elev_mod, out_transform = res
        return elev_mod if hasattr(elev_mod, "geometry") else _with_transform(elev_mod, out_transform)

    @property
    def is_affine(self) -> bool:
        return all(c.is_affine for c in self.pipeline)

    def to_matrix(self) -> np.ndarray:
        """Product of the steps' 4x4 matrices (base.py:3187-3199); a non-affine step raises."""
        total = np.eye(4)
        for c in self.pipeline:
            total = c.to_matrix() @ total
        return total

    def to_translations(self) -> tuple[float, float, float]:
        m = self.to_matrix()
        return (float(m[0, 3]), float(m[1, 3]), float(m[2, 3]))
