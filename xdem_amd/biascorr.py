"""Deramp, VerticalShift and coregistration pipelines on MI355X -- host-side mirrors of ``xdem.coreg.Deramp``
(``xdem/coreg/biascorr.py:621-745``), ``xdem.coreg.VerticalShift`` (``affine.py:721-770, 2013-2075``) and
``xdem.coreg.CoregPipeline`` (``base.py:2008-2019, 2880-3190``) for two rasters on one grid.  Re-exported by ``xdem_amd.coreg``.

Every pass over the grids runs in ``csrc/biascorr.hip`` through a dh plan (``xdemhip_dh_*``):

* ``Deramp`` with the defaults ``fit_func=polynomial_2d`` and ``fit_optimizer=scipy.optimize.curve_fit`` takes the least-squares
  moments of the polynomial over the valid (or drawn) pixels on the device, in normalised coordinates, and solves the
  (order+1)^2 system in float64 here: the optimum ``curve_fit`` converges to from upstream's ``p0 = ones`` (the model is linear in
  its parameters).  The coefficients are mapped back to raw pixel monomials, so ``fit_params`` has the reference's layout, and
  ``fit_perr`` is curve_fit's ``absolute_sigma=True`` error.  Any other ``fit_func`` / ``fit_optimizer`` receives dh and the pixel
  coordinates from the device and runs on the host exactly as upstream calls it (``base.py:978-985``); ``apply`` with a custom
  ``fit_func`` evaluates it on the host too -- that route is slow and exists for compatibility.
* ``VerticalShift`` with ``np.median`` / ``np.nanmedian`` selects the exact median of dh on the device; any other callable gets dh.
* ``CoregPipeline`` (``xdem_amd._coregbase``, shared with NuthKaab) chains the steps' public ``fit`` / ``apply`` as upstream does; rasters
  go back to the host between steps.

Output dtype of ``apply`` = input dtype (float32 in, float32 out -- upstream's final cast; float64 in: ``elev + corr`` in float64).
"""
from __future__ import annotations

import ctypes
import logging
import math
import warnings
from typing import Any, Callable

import numpy as np
import scipy.optimize

from . import _args, _lib
from ._args import nan_filled as _host_array  # noqa: F401  (the name bincorr, rigid and the test helpers know it by)
from ._args import plane_in_space  # noqa: F401
from ._coregbase import NO_VALID, CoregPipeline, _Plan, _Step, _with_transform, apply_translation, draw, raster_pair  # noqa: F401

MAX_DEVICE_ORDER = 5


def polynomial_2d(xx, *params):
    """N-order 2-D polynomial ``np.polynomial.polynomial.polyval2d(xx[0], xx[1], c)`` with ``c`` the (order+1)^2 params reshaped to
    a square (xdem/fit.py:127-149)."""
    poly_order = np.sqrt(len(params))
    if not poly_order.is_integer():
        raise ValueError("The parameters of the 2D polynomial should have a length equal to order^2, "
                         "see np.polyval2d for more details.")
    c = np.array(params).reshape((int(poly_order), int(poly_order)))
    return np.polynomial.polynomial.polyval2d(xx[0], xx[1], c)


# ---- the device plan --------------------------------------------------------------------------------------------------------
class DhPlan(_Plan):
    """Device-resident elevation difference of two rasters (``xdemhip_dh_plan``): valid mask, optional random subsample, and the
    reductions Deramp / VerticalShift need.  ``ref`` / ``tba``: 2-D NumPy arrays, or contiguous CUDA tensors of one dtype (kept alive by
    the plan, never copied)."""

    _DESTROY = "xdemhip_dh_destroy"

    def __init__(self, ref, tba, inlier_mask=None, ctx: _lib.Context | None = None):
        self.handle = None
        self.drawn = False
        if not _args.is_tensor(ref):
            ref, tba, inlier_mask = _host_array(ref), _host_array(tba), _host_array(inlier_mask)
        p = raster_pair(ref, tba, inlier_mask)   # (checked before a device is asked for: what is no raster pair is refused anywhere)
        if p.memspace == _lib.HOST and p.keep[2] is not None and p.keep[2].shape != p.shape:
            raise ValueError("inlier_mask must have the shape of the rasters")
        self.ctx = ctx or _lib.default_context()
        self.ctx.adopt(self)
        h, nv = ctypes.c_void_p(), ctypes.c_int64()
        self.dtype, self.shape = p.dtype, p.shape
        if p.memspace == _lib.DEVICE:
            self._keep = p.keep
        self.ctx.check(self.ctx._L.xdemhip_dh_create(self.ctx.handle, p.ref, p.tba, p.inlier, p.code, p.shape[0], p.shape[1], p.memspace,
                                                     ctypes.byref(h), ctypes.byref(nv)))
        self.handle = h
        self.n_valid = int(nv.value)
        self.n_selected = self.n_valid

    def subsample(self, ranks: np.ndarray) -> int:
        """Keep the valid pixels whose rank (position among the valid pixels in raster order) is listed: ``flatnonzero(valid)[ranks]``,
        formed on the device (``xdemhip_dh_subsample``).  Returns their number."""
        ranks = np.ascontiguousarray(ranks, dtype=np.int64)
        k = ctypes.c_int64()
        self.ctx.check(self.ctx._L.xdemhip_dh_subsample(self.handle, _args.ptr(ranks), int(ranks.size), _lib.HOST, ctypes.byref(k)))
        self.drawn = True
        self.n_selected = int(k.value)
        return self.n_selected

    def poly_moments(self, order: int, row_offset: int = 0, H_global: int | None = None, W_global: int | None = None):
        """(M, R, count): M[a, b] = sum u^a v^b (a, b <= 2 order), R[i, j] = sum dh u^i v^j (i, j <= order) over the selected pixels, in
        the normalised coordinates of ``poly_norm`` (``xdemhip_dh_poly_moments``)."""
        order = int(order)
        H_global = self.shape[0] if H_global is None else int(H_global)
        W_global = self.shape[1] if W_global is None else int(W_global)
        m = np.empty((2 * order + 1, 2 * order + 1), dtype=np.float64)
        r = np.empty((order + 1, order + 1), dtype=np.float64)
        cnt = ctypes.c_int64()
        self.ctx.check(self.ctx._L.xdemhip_dh_poly_moments(self.handle, order, int(row_offset), H_global, W_global, _args.dp(m), _args.dp(r),
                                                           ctypes.byref(cnt)))
        return m, r, int(cnt.value)

    def median(self) -> tuple[float, int]:
        """Exact ``np.median(dh)`` over the selected pixels in the value dtype, and their number (``xdemhip_dh_median``)."""
        med, cnt = ctypes.c_double(), ctypes.c_int64()
        self.ctx.check(self.ctx._L.xdemhip_dh_median(self.handle, ctypes.byref(med), ctypes.byref(cnt)))
        return med.value, int(cnt.value)

    def values(self, coords: bool = True):
        """dh of the selected pixels (plan dtype, raster order) and -- with ``coords`` -- their column and row indexes (int64)."""
        k = self.n_selected
        dh = np.empty(k, dtype=self.dtype)
        col = np.empty(k, dtype=np.int64) if coords else None
        row = np.empty(k, dtype=np.int64) if coords else None
        cnt = ctypes.c_int64()
        self.ctx.check(self.ctx._L.xdemhip_dh_values(self.handle, _args.ptr(dh), _args.ptr(col), _args.ptr(row), _lib.HOST, ctypes.byref(cnt)))
        if int(cnt.value) != k:
            raise _lib.XdemHipError(f"xdemhip_dh_values returned {cnt.value} values, expected {k}")
        return (dh, col, row) if coords else dh

    # ---- variables of the bias corrections (csrc/bincorr.hip; the sources are made by xdem_amd.bincorr) ----
    def _on_device(self) -> bool:
        return getattr(self, "_keep", None) is not None

    def _plane(self, plane):
        """A variable plane on the plan's grid, in the plan's memory space: (pointer, dtype code, the array kept alive)."""
        ptr, code, shape, t = plane_in_space(plane, self._keep[0].device if self._on_device() else None)
        if shape != tuple(self.shape):
            raise ValueError(f"a bias variable has shape {shape}, the rasters {tuple(self.shape)}")
        return ptr, code, t

    def restrict_finite(self, plane) -> int:
        """Narrow the valid pixels to those where ``plane`` (H x W) is finite -- upstream's valid mask of a bias correction is
        ``inlier & finite(ref) & finite(tba) & finite(every variable)`` (base.py:653-661).  Before ``subsample`` / ``values`` only
        (``xdemhip_dh_restrict_finite``).  Returns the new count."""
        ptr, code, keep = self._plane(plane)
        nv = ctypes.c_int64()
        self.ctx.check(self.ctx._L.xdemhip_dh_restrict_finite(self.handle, ptr, code, _lib.DEVICE if self._on_device() else _lib.HOST,
                                                              ctypes.byref(nv)))
        del keep
        self.n_valid = self.n_selected = int(nv.value)
        return self.n_valid

    def var_columns(self, sources: list):
        """dh (plan dtype) and the value of every variable of ``sources`` (``_lib.VarSrc`` descriptions, their planes made by
        ``_plane``) at the selected pixels in raster order (``xdemhip_dh_var_columns``): NumPy columns for a plan made of NumPy
        rasters, 1-D CUDA tensors for a plan made of CUDA tensors -- those go into ``nd_binning`` without a host round trip.  A
        plane's column has the plane's dtype, the rotated coordinate is float64, ref / tba have the plan's dtype."""
        k = self.n_selected
        if k == 0:
            raise ValueError(NO_VALID)
        n_var = len(sources)
        dts = []
        for s in sources:
            if s.kind == _lib.VAR_PLANE:
                dts.append(np.dtype(np.float32 if s.dtype == _lib.F32 else np.float64))
            else:
                dts.append(np.dtype(np.float64) if s.kind == _lib.VAR_ROTATED else np.dtype(self.dtype))
        if self._on_device():
            import torch

            dev = self._keep[0].device
            tdt = {np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64}
            dh = torch.empty(k, dtype=tdt[np.dtype(self.dtype)], device=dev)
            cols = [torch.empty(k, dtype=tdt[d], device=dev) for d in dts]
        else:
            dh = np.empty(k, dtype=self.dtype)
            cols = [np.empty(k, dtype=d) for d in dts]
        arr = (_lib.VarSrc * max(n_var, 1))(*sources)
        outs = (ctypes.c_void_p * max(n_var, 1))(*[_args.ptr(c) for c in cols])
        cnt = ctypes.c_int64()
        self.ctx.check(self.ctx._L.xdemhip_dh_var_columns(self.handle, n_var, arr, _args.ptr(dh), outs, _args.space(dh), ctypes.byref(cnt)))
        if int(cnt.value) != k:
            raise _lib.XdemHipError(f"xdemhip_dh_var_columns returned {cnt.value} values, expected {k}")
        return dh, cols

    def shift_nmad(self, shift_x: float, shift_y: float, res, nfact: float = 1.4826) -> tuple[float, float, int]:
        """(median, nmad, count) of dh = ref - bilinear(tba)(row - shift_y / res_y, col + shift_x / res_x) over the selected pixels, the
        ones whose interpolated value is NaN dropped: ``np.nanmedian(dh)``, ``nfact * np.nanmedian(|dh - median|)`` in the value dtype
        and ``np.isfinite(dh).sum()``, all exact (``xdemhip_dh_shift_nmad``: one pass over the rasters, two selections, one fetch).
        Raises "no valid points" where no pixel is left."""
        res = (float(res), float(res)) if np.isscalar(res) else (float(res[0]), float(res[1]))
        med, nm, cnt = ctypes.c_double(), ctypes.c_double(), ctypes.c_int64()
        self.ctx.check(self.ctx._L.xdemhip_dh_shift_nmad(self.handle, float(shift_x), float(shift_y), res[0], res[1], float(nfact),
                                                         ctypes.byref(med), ctypes.byref(nm), ctypes.byref(cnt)))
        return med.value, nm.value, int(cnt.value)

    def shift_values(self, shift_x: float, shift_y: float, res) -> np.ndarray:
        """The same dh of every selected pixel (plan dtype, raster order, NaN where the interpolated value is): what a host loss function
        receives (``xdemhip_dh_shift_values``)."""
        res = (float(res), float(res)) if np.isscalar(res) else (float(res[0]), float(res[1]))
        k = self.n_selected
        dh = np.empty(k, dtype=self.dtype)
        cnt = ctypes.c_int64()
        self.ctx.check(self.ctx._L.xdemhip_dh_shift_values(self.handle, float(shift_x), float(shift_y), res[0], res[1], _args.ptr(dh),
                                                           _lib.HOST, ctypes.byref(cnt)))
        if int(cnt.value) != k:
            raise _lib.XdemHipError(f"xdemhip_dh_shift_values returned {cnt.value} values, expected {k}")
        return dh


# ---- polynomial algebra on the host --------------------------------------------------------------------------------------------
def poly_norm(n_global: int) -> tuple[float, float]:
    """(centre, half-width) of the normalised coordinate of an axis of n_global pixels: u = (x - centre) / half-width (include/xdemhip.h)."""
    half = 0.5 * (n_global - 1)
    return half, (half if half > 0 else 1.0)


def _axis_transform(K: int, centre: float, scale: float) -> np.ndarray:
    """T[m, i] = C(i, m) (-centre)^(i - m) / scale^i: raw-monomial coefficients of u^i, u = (x - centre) / scale."""
    T = np.zeros((K, K), dtype=np.float64)
    for i in range(K):
        for m in range(i + 1):
            T[m, i] = math.comb(i, m) * (-centre) ** (i - m) / scale ** i
    return T


def coeff_transform(order: int, shape: tuple[int, int]) -> np.ndarray:
    """The (K^2 x K^2) map from coefficients b[i, j] of u^i v^j to coefficients c[m, n] of x^m y^n (K = order + 1, both raveled in C
    order, the layout of polynomial_2d's params), for a grid of ``shape`` = (H, W)."""
    K = order + 1
    cx, sx = poly_norm(shape[1])
    cy, sy = poly_norm(shape[0])
    return np.kron(_axis_transform(K, cx, sx), _axis_transform(K, cy, sy))


def solve_moments(M: np.ndarray, R: np.ndarray, order: int, shape: tuple[int, int]):
    """Least-squares polynomial from the device moments: the Gram matrix G[(i,j),(k,l)] = M[i+k, j+l] and right-hand side R[i, j] in
    normalised coordinates, solved in float64 (minimum-norm where G is rank-deficient, e.g. all points on one row), mapped back to raw
    pixel monomials.  Returns (fit_params, fit_perr): perr = sqrt(diag(T G^-1 T^T)), curve_fit's ``absolute_sigma=True`` error."""
    K = order + 1
    idx = [(i, j) for i in range(K) for j in range(K)]
    G = np.array([[M[i + k, j + l] for (k, l) in idx] for (i, j) in idx], dtype=np.float64)
    rhs = np.array([R[i, j] for (i, j) in idx], dtype=np.float64)
    if np.linalg.matrix_rank(G) == G.shape[0]:
        b = np.linalg.solve(G, rhs)
        Ginv = np.linalg.inv(G)
    else:
        b = np.linalg.lstsq(G, rhs, rcond=None)[0]
        Ginv = np.linalg.pinv(G)
    T = coeff_transform(order, shape)
    params = T @ b
    cov = T @ Ginv @ T.T
    return params, np.sqrt(np.abs(np.diag(cov)))


def poly2d_apply(elev, params, row_offset: int = 0, ctx: _lib.Context | None = None, out=None):
    """``elev + polyval2d(xx, yy, c)`` on the device, NumPy's evaluation order bit for bit (``xdemhip_poly2d_apply``); float32 elev gives
    the float32 cast of the float64 sum, float64 elev the float64 sum.  ``elev``: a 2-D NumPy array, or a contiguous 2-D float32 /
    float64 CUDA tensor -- then the result (``out`` if given: a contiguous CUDA tensor of the same shape, dtype and device) is written on
    the current torch stream, ordered after the work that produced ``elev`` and before whatever the caller queues next, without a host
    synchronisation (the context's stream is set to that stream, as ``terrain_attributes_device`` does)."""
    params = np.ascontiguousarray(params, dtype=np.float64).ravel()
    K = int(round(math.sqrt(params.size)))
    if K * K != params.size:
        raise ValueError("The parameters of the 2D polynomial should have a length equal to order^2, see np.polyval2d for more details.")
    if K - 1 > MAX_DEVICE_ORDER:
        raise NotImplementedError(f"poly_order > {MAX_DEVICE_ORDER} is not supported on the device")
    if _args.is_tensor(elev):
        import torch

        _args.device_float(elev, "device elev must be a contiguous 2D float32 / float64 CUDA tensor")
        if out is None:
            out = torch.empty_like(elev, memory_format=torch.contiguous_format)
        elif not (_args.is_tensor(out) and out.is_cuda and out.is_contiguous() and out.shape == elev.shape and out.dtype == elev.dtype
                  and out.device == elev.device):
            raise ValueError("out must be a contiguous CUDA tensor of elev's shape, dtype and device")
        ctx = ctx or _lib.default_context(elev.device.index)
    else:
        ctx = ctx or _lib.default_context()
        elev = _args.host_float(elev)
        out = np.empty_like(elev)
    with _args.torch_stream_scope(ctx, elev):
        ctx.check(ctx._L.xdemhip_poly2d_apply(ctx.handle, _args.ptr(elev), _args.code(elev), elev.shape[0], elev.shape[1], int(row_offset),
                                              _args.dp(params), K - 1, _args.ptr(out), _args.space(elev)))
    return out


def _check_weights(weights) -> None:
    if weights is not None:
        raise NotImplementedError("Weights have not yet been implemented")


# ---- Deramp ---------------------------------------------------------------------------------------------------------------------
class Deramp(_Step):
    """Correct a 2-D polynomial along the pixel coordinates (tilts, domes).  Constructor of ``xdem.coreg.Deramp``
    (biascorr.py:630-640); only ``fit_or_bin="fit"`` is implemented here.  The parameters land in
    ``meta["outputs"]["fitorbin"]["fit_params"]`` in the reference's layout: ``fit_func((xx, yy), *fit_params)`` is the surface."""

    def __init__(self, poly_order: int = 2, fit_or_bin: str = "fit", fit_func: Callable[..., Any] = polynomial_2d,
                 fit_optimizer: Callable[..., Any] = scipy.optimize.curve_fit, bin_sizes=10, bin_statistic=np.nanmedian,
                 bin_apply_method: str = "linear", subsample: float | int = 5e5) -> None:
        if fit_or_bin not in ["fit", "bin", "bin_and_fit"]:
            raise ValueError(f"Argument `fit_or_bin` must be 'bin_and_fit', 'fit' or 'bin', got {fit_or_bin}.")
        if fit_or_bin != "fit":
            raise NotImplementedError(f"fit_or_bin={fit_or_bin!r}: only \"fit\" is implemented for Deramp here.")
        if not callable(fit_func):
            raise TypeError(f"Argument `fit_func` must be a function (callable), got {type(fit_func)}.")
        if not callable(fit_optimizer):
            raise TypeError(f"Argument `fit_optimizer` must be a function (callable), got {type(fit_optimizer)}.")
        self.meta: dict[str, Any] = {
            "inputs": {
                "fitorbin": {"fit_or_bin": fit_or_bin, "fit_func": fit_func, "fit_optimizer": fit_optimizer, "bin_sizes": bin_sizes,
                             "bin_statistic": bin_statistic, "bin_apply_method": bin_apply_method, "bias_var_names": ["xx", "yy"]},
                "random": {"subsample": subsample, "random_state": None},
                "specific": {"poly_order": int(poly_order)},
            },
            "outputs": {},
        }
        self._needs_vars = False

    def _device_route(self) -> bool:
        fb = self.meta["inputs"]["fitorbin"]
        return fb["fit_func"] is polynomial_2d and fb["fit_optimizer"] is scipy.optimize.curve_fit

    def fit(self, reference_elev, to_be_aligned_elev, inlier_mask=None, bias_vars=None, weights=None, subsample=None, transform=None,
            crs=None, area_or_point=None, z_name=None, random_state=None, resolution=None, **kwargs: Any) -> "Deramp":
        """Estimate the polynomial of dh = reference - to_be_aligned over the valid (and drawn) pixels (``Coreg.fit`` with
        ``_fit_rst_rst``, biascorr.py:663-695).  ``transform`` / ``resolution`` are accepted for call compatibility (pixel
        coordinates need neither)."""
        _check_weights(weights)
        if bias_vars is not None:
            raise NotImplementedError("bias_vars is not used by Deramp (its variables are the pixel coordinates).")
        if subsample is not None:
            self.meta["inputs"]["random"]["subsample"] = subsample
        if random_state is not None:
            self.meta["inputs"]["random"]["random_state"] = random_state
        order = self.meta["inputs"]["specific"]["poly_order"]
        n_params = (order + 1) ** 2
        if self._device_route() and order > MAX_DEVICE_ORDER:
            raise NotImplementedError(f"Deramp: poly_order 0..{MAX_DEVICE_ORDER} on the device, got {order}")
        with DhPlan(reference_elev, to_be_aligned_elev, inlier_mask) as plan:
            n = draw(plan, self.meta["inputs"]["random"]["subsample"], self.meta["inputs"]["random"]["random_state"])
            if n < n_params:   # (what curve_fit raises for fewer points than parameters)
                raise TypeError(f"Improper input: func input vector length N={n_params} must not exceed func output vector length M={n}")
            logging.debug("Estimating a 2D polynomial of order %d on %d points.", order, n)
            if self._device_route():
                M, R, _ = plan.poly_moments(order)
                params, perr = solve_moments(M, R, order, plan.shape)
            else:
                dh, col, row = plan.values()
                fb = self.meta["inputs"]["fitorbin"]
                results = fb["fit_optimizer"](f=fb["fit_func"], xdata=np.array([col, row]).squeeze(), ydata=dh, sigma=None,
                                              absolute_sigma=True, p0=np.ones(n_params), **kwargs)
                params = results[0]
                perr = np.sqrt(np.diag(results[1])) if fb["fit_optimizer"] is scipy.optimize.curve_fit else None
        self.meta["outputs"]["fitorbin"] = {"fit_params": np.asarray(params)}
        if perr is not None:
            self.meta["outputs"]["fitorbin"]["fit_perr"] = perr
        self.meta["outputs"]["random"] = {"subsample_final": int(n)}
        return self

    def apply(self, elev, resolution=None, resample: bool = True, *, bias_vars=None, resampling: str = "bilinear", transform=None, crs=None,
              z_name: str = "z"):
        """``elev + fit_func((xx, yy), *fit_params)`` (biascorr.py:262-311, 740-745) in the input dtype; with ``transform=`` the call
        returns ``(array, transform)`` like upstream's array interface."""
        if "fitorbin" not in self.meta["outputs"]:
            raise AssertionError(".fit() does not seem to have been called yet")
        if bias_vars is not None:
            raise NotImplementedError("bias_vars is not used by Deramp (its variables are the pixel coordinates).")
        params = self.meta["outputs"]["fitorbin"]["fit_params"]
        fit_func = self.meta["inputs"]["fitorbin"]["fit_func"]
        if fit_func is polynomial_2d:
            out = poly2d_apply(elev, params)
        else:   # a custom surface: evaluated on the host, as upstream does
            arr = _host_array(elev)
            if arr.dtype not in _args.FLOATS:
                arr = arr.astype(np.float32)
            xx, yy = np.meshgrid(np.arange(0, arr.shape[1]), np.arange(0, arr.shape[0]))
            out = (arr + fit_func((xx, yy), *params)).astype(arr.dtype)
        return _with_transform(out, transform)

    @property
    def is_affine(self) -> bool:
        return False

    def to_matrix(self):
        raise NotImplementedError("Deramp is not an affine transformation: it has no matrix.")


# ---- VerticalShift --------------------------------------------------------------------------------------------------------------
class VerticalShift(_Step):
    """Shift the to-be-aligned DEM by a central tendency of dh (``xdem.coreg.VerticalShift``, affine.py:2013-2075).
    ``np.median`` / ``np.nanmedian`` are exact selections on the device; any other callable receives dh (value dtype, raster order)."""

    def __init__(self, vshift_reduc_func: Callable[[np.ndarray], Any] = np.median, subsample: float | int = 1.0, initial_shift=None) -> None:
        if initial_shift is not None:
            raise NotImplementedError("VerticalShift(initial_shift=...) is not implemented here.")
        if not callable(vshift_reduc_func):
            raise TypeError("vshift_reduc_func must be a callable")
        self.meta: dict[str, Any] = {
            "inputs": {"affine": {"vshift_reduc_func": vshift_reduc_func}, "random": {"subsample": subsample, "random_state": None}},
            "outputs": {},
        }
        self._needs_vars = False

    def fit(self, reference_elev, to_be_aligned_elev, inlier_mask=None, bias_vars=None, weights=None, subsample=None, transform=None,
            crs=None, area_or_point=None, z_name=None, random_state=None, resolution=None, **kwargs: Any) -> "VerticalShift":
        """``vertical_shift`` (affine.py:721-770): ``float(vshift_reduc_func(ref - tba))`` over the valid (and drawn) pixels."""
        _check_weights(weights)
        if bias_vars is not None:
            raise NotImplementedError("bias_vars is not used by VerticalShift.")
        if subsample is not None:
            self.meta["inputs"]["random"]["subsample"] = subsample
        if random_state is not None:
            self.meta["inputs"]["random"]["random_state"] = random_state
        func = self.meta["inputs"]["affine"]["vshift_reduc_func"]
        logging.info("Running vertical shift coregistration")
        from . import epc as _epc

        if _epc.is_cloud(reference_elev) or _epc.is_cloud(to_be_aligned_elev):
            # one raster and one cloud (base.py:747-772): dh at the points at zero shift, reference minus to-be-aligned
            if _epc.is_cloud(reference_elev) and _epc.is_cloud(to_be_aligned_elev):
                raise TypeError("This pre-processing function is only intended for raster-point or raster-raster methods, "
                                "not point-point methods.")
            raster, cloud, pts_is_ref = _epc.split_pair(reference_elev, to_be_aligned_elev)
            with _epc.PtsPlan(raster, *_epc.cloud_columns(cloud, z_name), transform, pts_is_ref, inlier_mask) as plan:
                n = draw(plan, self.meta["inputs"]["random"]["subsample"], self.meta["inputs"]["random"]["random_state"])
                if func is np.median or func is np.nanmedian:
                    vshift = float(plan.shift_nmad(0.0, 0.0)[0])
                else:
                    vshift = float(func(plan.shift_values(0.0, 0.0)))
            self.meta["outputs"]["affine"] = {"shift_z": vshift}
            self.meta["outputs"]["random"] = {"subsample_final": int(n)}
            return self
        with DhPlan(reference_elev, to_be_aligned_elev, inlier_mask) as plan:
            n = draw(plan, self.meta["inputs"]["random"]["subsample"], self.meta["inputs"]["random"]["random_state"])
            if func is np.median or func is np.nanmedian:
                vshift = float(plan.median()[0])
            else:
                vshift = float(func(plan.values(coords=False)))
        self.meta["outputs"]["affine"] = {"shift_z": vshift}
        self.meta["outputs"]["random"] = {"subsample_final": int(n)}
        return self

    def apply(self, elev, resolution=None, resample: bool = True, *, bias_vars=None, resampling: str = "bilinear", transform=None, crs=None,
              z_name: str = "z"):
        """``elev + shift_z`` in the input dtype (``apply_translation(..., resample=False)``); with ``transform=`` the call returns
        ``(array, transform)``: a vertical shift leaves the geotransform as it is."""
        if "affine" not in self.meta["outputs"]:
            raise AssertionError(".fit() does not seem to have been called yet")
        if bias_vars is not None:
            raise NotImplementedError("bias_vars is not used by VerticalShift.")
        from . import epc as _epc

        if _epc.is_cloud(elev):
            return _epc.apply_matrix_cloud(elev, self.to_matrix(), z_name=z_name)
        res = resolution if resolution is not None else 1.0
        out = apply_translation(elev, 0.0, 0.0, self.meta["outputs"]["affine"]["shift_z"], res, resample=False)
        return _with_transform(out, transform)

    @property
    def is_affine(self) -> bool:
        return True

    def to_translations(self) -> tuple[float, float, float]:
        m = self.to_matrix()
        return (float(m[0, 3]), float(m[1, 3]), float(m[2, 3]))

    def to_rotations(self) -> tuple[float, float, float]:
        return (0.0, 0.0, 0.0)

    def to_matrix(self) -> np.ndarray:
        """4x4 matrix of the vertical shift (affine.py:2098-2104)."""
        m = np.diag(np.ones(4, dtype=float))
        m[2, 3] += self.meta["outputs"]["affine"]["shift_z"]
        return m
