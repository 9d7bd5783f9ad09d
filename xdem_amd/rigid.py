"""LZD coregistration and the rotation-capable raster apply on MI355X -- host-side mirrors of ``xdem.coreg.LZD``
(``xdem/coreg/affine.py:1417-1776, 2544-2664``; Rosenholm & Torlegard 1988), ``xdem.coreg.apply_matrix`` for arrays
(``xdem/coreg/base.py:1389-1590, 1686-1760``) and the matrix helpers of ``base.py:1056-1287``.  Re-exported by ``xdem_amd.coreg``.

Every pass over the grids runs in ``csrc/rigid.hip``:

* ``LZD.fit`` builds a dh plan, draws the subsample, takes the centroid and iterates as upstream's ``_iterate_method`` does.  With the
  defaults ``fit_minimizer=scipy.optimize.least_squares`` and ``fit_loss_func="linear"`` one iteration is ONE device call
  (``xdemhip_dh_lzd_normal``: the 6 x 6 normal equations of the model, which is linear in its parameters) and a float64 solve here --
  the optimum ``least_squares`` converges to from zeros, as Deramp's moments replace ``curve_fit``.  Any other minimiser / loss gets
  the six arrays ``x, y, z, dh, gradx, grady`` from the device (``xdemhip_dh_lzd_values``) and runs on the host exactly as ``_lzd_fit``
  calls it.
* ``apply_matrix`` moves a point cloud by any 4 x 4 matrix (``xdemhip_apply_matrix_pts``, returns an ``EPC``) and regrids a DEM after a rigid transform with rotations below 20 degrees (``xdemhip_apply_matrix_rst``); pure
  translations go through ``apply_translation``.  Larger rotations (Delaunay ``griddata`` upstream) and resamplings other than linear
  are not implemented.

The grid's coordinates are pixel centres under the 6-tuple transform ``(a, b, c, d, e, f)``: ``x = c + (col + 0.5) a``,
``y = f + (row + 0.5) e`` -- geoutils' ``_coords`` / ``_interp_points`` / ``to_pointcloud`` are un-vendored and absent, **parity unpinned**;
the convention is self-consistent (an identity matrix samples pixel (r, c) at (r, c)).

``_RigidStep`` carries what LZD, ``xdem_amd.icp.ICP`` and ``xdem_amd.cpd.CPD`` share: the front of ``fit``, the iteration loop, the outputs, ``apply`` and the accessors."""
from __future__ import annotations

import contextlib
import ctypes
import logging
from typing import Any, Callable

import numpy as np
import scipy.optimize

from . import _args, _lib
from ._args import c_doubles
from ._coregbase import _Step, _with_transform, apply_translation, draw
from .biascorr import DhPlan, _check_weights

LZD_NO_VALID = ("The subsample contains no more valid values. This can happen if the affine transformation to "
                "correct is larger than the data extent, or if the algorithm diverged. To ensure all possible points can "
                "be used at any iteration step, use subsample=1.")


# ---- matrix helpers: upstream's names, signatures and messages (base.py:1056-1287), written from the formulas ----------------------
_RIGID_ATOL = 10e-8


def _rotation(ax: float, ay: float, az: float) -> np.ndarray:
    """Rotation by extrinsic Euler angles (radians): first about X, then Y, then Z, i.e. Rz(az) Ry(ay) Rx(ax) in closed form."""
    (sx, sy, sz), (cx, cy, cz) = np.sin([ax, ay, az]), np.cos([ax, ay, az])
    return np.array([[cy * cz, sx * sy * cz - cx * sz, cx * sy * cz + sx * sz],
                     [cy * sz, sx * sy * sz + cx * cz, cx * sy * sz - sx * cz],
                     [-sy, sx * cy, cx * cy]], dtype=np.float64)


def _is_rotation(rot: np.ndarray, atol: float) -> bool:
    return bool(np.allclose(rot.T @ rot, np.eye(3), atol=atol))


def _euler_angles(rot: np.ndarray, atol: float = _RIGID_ATOL) -> tuple[float, float, float]:
    """The angles (radians, about X, Y, Z) of ``_rotation``: row 2 of the closed form is (-sin ay, sin ax cos ay, cos ax cos ay) and
    column 0 is (cos ay cos az, cos ay sin az, -sin ay); cos ay > 0 drops out of the two arctangents.  At cos ay = 0 only ax -+ az is
    determined: ax is set to 0."""
    if not _is_rotation(rot, atol):
        raise ValueError("Matrix is not orthogonal")
    if abs(rot[2, 0]) >= 1 - atol:
        return 0.0, float(np.copysign(np.pi / 2, -rot[2, 0])), float(np.arctan2(-rot[0, 1], rot[1, 1]))
    return float(np.arctan2(rot[2, 1], rot[2, 2])), float(np.arcsin(-rot[2, 0])), float(np.arctan2(rot[1, 0], rot[0, 0]))


def _make_matrix_valid(matrix: np.ndarray) -> np.ndarray:
    """The nearest rigid matrix: bottom row (0, 0, 0, 1) and the rotation block replaced by the orthogonal factor of its polar
    decomposition (from the SVD), its determinant forced to +1."""
    out = np.array(matrix, dtype=np.float64)
    out[3] = (0.0, 0.0, 0.0, 1.0)
    left, _, right = np.linalg.svd(out[:3, :3])
    handed = 1.0 if np.linalg.det(left @ right) >= 0 else -1.0
    out[:3, :3] = left @ np.diag([1.0, 1.0, handed]) @ right
    return out


def matrix_from_translations_rotations(t1: float = 0.0, t2: float = 0.0, t3: float = 0.0, alpha1: float = 0.0, alpha2: float = 0.0,
                                       alpha3: float = 0.0, use_degrees: bool = True) -> np.ndarray:
    """Rigid 4 x 4 matrix from three translations (unit of the coordinates) and three extrinsic Euler rotations about X, Y and Z
    (degrees, or radians with ``use_degrees=False``)."""
    angles = np.deg2rad([alpha1, alpha2, alpha3]) if use_degrees else (alpha1, alpha2, alpha3)
    out = np.eye(4)
    out[:3, :3] = _rotation(*angles)
    out[:3, 3] = (t1, t2, t3)
    return out


def translations_rotations_from_matrix(matrix: np.ndarray, return_degrees: bool = True) -> tuple[float, float, float, float, float, float]:
    """``(t1, t2, t3, alpha1, alpha2, alpha3)`` of a rigid matrix: the inverse of ``matrix_from_translations_rotations``."""
    angles = _euler_angles(np.asarray(matrix)[:3, :3])
    if return_degrees:
        angles = tuple(np.rad2deg(angles))
    return (*np.asarray(matrix)[:3, 3], *angles)


def invert_matrix(matrix: np.ndarray, atol: float = _RIGID_ATOL) -> np.ndarray:
    """The inverse of a rigid matrix (made valid first): rotation R^T, translation -R^T t."""
    matrix = np.asarray(matrix)
    if not np.allclose(matrix[3], (0, 0, 0, 1), atol=atol):
        raise ValueError("Not affine")
    if not _is_rotation(matrix[:3, :3], atol):
        raise ValueError("Not a rigid transform")
    rigid = _make_matrix_valid(matrix)
    out = np.eye(4)
    out[:3, :3] = rigid[:3, :3].T
    out[:3, 3] = -(out[:3, :3] @ rigid[:3, 3])
    return out


# ---- transforms -------------------------------------------------------------------------------------------------------------------
def _transform6(transform, resolution, shape) -> tuple[float, ...]:
    """The 6-tuple ``(a, b, c, d, e, f)`` of a call: from ``transform`` (an object with ``.a`` .. ``.f`` or a 6-tuple), else from
    ``resolution`` alone, which means the grid ``(rx, 0, 0, 0, -ry, H * ry)``.  Only north-up grids (b = d = 0)."""
    if transform is not None:
        t = (transform.a, transform.b, transform.c, transform.d, transform.e, transform.f) if hasattr(transform, "a") else tuple(transform)[:6]
        t = tuple(float(v) for v in t)
    elif resolution is not None:
        rx, ry = (float(resolution), float(resolution)) if np.isscalar(resolution) else (float(resolution[0]), float(resolution[1]))
        t = (rx, 0.0, 0.0, 0.0, -ry, shape[0] * ry)
    else:
        raise ValueError("'transform' must be given if both DEMs are array-like.")
    if t[1] != 0.0 or t[3] != 0.0:
        raise NotImplementedError("only north-up transforms (b = d = 0) are supported")
    return t


# ---- apply_matrix -------------------------------------------------------------------------------------------------------------------
def apply_matrix(elev, matrix, invert: bool = False, centroid=None, resample: bool = True, resampling: str = "linear", transform=None,
                 z_name: str = "z", *, ctx: _lib.Context | None = None):
    """Apply a 3D affine transformation matrix to a 2.5D DEM given as a 2-D array with its ``transform`` (``xdem.coreg.apply_matrix``,
    array case; returns ``(array, transform)``): a z-only matrix adds the shift, a translation goes through ``apply_translation``
    (``resample=False`` moves the transform instead), rotations below 20 degrees about every axis are regridded on the device by
    upstream's fixed-point iteration with SciPy's linear ``RegularGridInterpolator``.  Output dtype = input dtype."""
    if hasattr(elev, "geometry"):   # a cloud: every point moved by the matrix, any rotation (_apply_matrix_pts, base.py:1290-1325)
        from . import epc as _epc

        if invert:
            invert_matrix(np.asarray(matrix, dtype=np.float64))   # (its checks; the device forms R^T and -(R^T t) itself)
        return _epc.apply_matrix_cloud(elev, matrix, invert, centroid, z_name)
    matrix = np.asarray(matrix, dtype=np.float64)
    if invert:
        matrix = invert_matrix(matrix)
    arr = _args.host_float(elev)
    if arr.ndim != 2:
        raise ValueError("elev must be a 2D array")
    if np.count_nonzero(np.isfinite(arr)) == 0:
        raise ValueError("Input DEM has all nans.")
    dx, dy, dz = (float(v) for v in matrix[:3, 3])
    no_rotation = np.array_equal(matrix[:3, :3], np.eye(3)) and np.array_equal(matrix[3], (0, 0, 0, 1))
    if no_rotation and dx == 0 and dy == 0:   # a vertical shift: no grid is needed
        return arr + arr.dtype.type(dz), transform
    t6 = _transform6(transform, None, arr.shape)
    if no_rotation:
        out = apply_translation(arr, dx, dy, dz, (abs(t6[0]), abs(t6[4])), resample, ctx=ctx)
        if resample:
            return out, transform
        moved = (t6[0], t6[1], t6[2] + dx, t6[3], t6[4], t6[5] + dy)
        return out, (type(transform)(*moved) if hasattr(transform, "a") else moved)
    if resampling != "linear":
        raise NotImplementedError(f"resampling={resampling!r}: only \"linear\" is implemented for matrices with a rotation.")
    if max(abs(angle) for angle in translations_rotations_from_matrix(matrix)[3:]) >= 20:
        raise NotImplementedError("rotations of 20 degrees and more (upstream's Delaunay griddata route) are not implemented.")
    if arr.shape[0] < 2 or arr.shape[1] < 2:
        raise ValueError("the DEM must be at least 2 x 2 pixels for a regrid")
    ctx = ctx or _lib.default_context()
    out = np.empty_like(arr)
    cen = None if centroid is None else c_doubles([float(v) for v in centroid])
    ctx.check(ctx._L.xdemhip_apply_matrix_rst(ctx.handle, _args.ptr(arr), _args.code(arr), arr.shape[0], arr.shape[1], c_doubles(t6),
                                              c_doubles(matrix.ravel()), cen, _args.ptr(out), _lib.HOST))
    return out, transform


# ---- the LZD passes of a dh plan ----------------------------------------------------------------------------------------------------
def lzd_gradients(plan: DhPlan, t6) -> tuple[np.ndarray, np.ndarray]:
    """(gradx, grady) = (gradient_x / res_x, -gradient_y / res_y) of ``np.gradient(ref)`` in the plan's dtype (``xdemhip_dh_lzd_gradients``)."""
    gx, gy = np.empty(plan.shape, dtype=plan.dtype), np.empty(plan.shape, dtype=plan.dtype)
    plan.ctx.check(plan.ctx._L.xdemhip_dh_lzd_gradients(plan.handle, c_doubles(t6), _args.ptr(gx), _args.ptr(gy), _lib.HOST))
    return gx, gy


def lzd_centroid(plan: DhPlan, t6) -> tuple[tuple[float, float, float], int]:
    """((mean x, mean y, mean tba), count) over the plan's selected pixels (``xdemhip_dh_lzd_centroid``)."""
    c = np.empty(3, dtype=np.float64)
    cnt = ctypes.c_int64()
    plan.ctx.check(plan.ctx._L.xdemhip_dh_lzd_centroid(plan.handle, c_doubles(t6), _args.dp(c), ctypes.byref(cnt)))
    return (float(c[0]), float(c[1]), float(c[2])), int(cnt.value)


def lzd_normal(plan: DhPlan, t6, matrix, centroid) -> tuple[np.ndarray, int]:
    """(29 sums, count) of one LZD iteration (``xdemhip_dh_lzd_normal``): the 21 upper-triangle terms of a a^T, the 6 of a dh, sum dh^2
    and sum dh over the pixels that stay valid under ``matrix``."""
    s = np.empty(29, dtype=np.float64)
    cnt = ctypes.c_int64()
    plan.ctx.check(plan.ctx._L.xdemhip_dh_lzd_normal(plan.handle, c_doubles(t6), c_doubles(np.asarray(matrix, dtype=np.float64).ravel()), c_doubles(centroid),
                                                     _args.dp(s), ctypes.byref(cnt)))
    return s, int(cnt.value)


def lzd_values(plan: DhPlan, t6, matrix, centroid) -> np.ndarray:
    """The six arrays ``x, y, z, dh, gradx, grady`` (rows of a (6, k) float64 array, raster order) of the pixels that stay valid under
    ``matrix``: what upstream hands ``_lzd_fit`` (``xdemhip_dh_lzd_values``)."""
    n = plan.n_selected
    out = np.empty((6, max(n, 1)), dtype=np.float64)
    cnt = ctypes.c_int64()
    plan.ctx.check(plan.ctx._L.xdemhip_dh_lzd_values(plan.handle, c_doubles(t6), c_doubles(np.asarray(matrix, dtype=np.float64).ravel()), c_doubles(centroid),
                                                     _args.dp(out), ctypes.byref(cnt)))
    return np.ascontiguousarray(out[:, : int(cnt.value)])


def solve_scaled(N: np.ndarray, b: np.ndarray) -> np.ndarray:
    """N x = b in float64 after scaling by N's diagonal, minimum-norm where N is singular (e.g. a flat reference)."""
    d = np.sqrt(np.diag(N))
    d = np.where(d > 0, 1.0 / np.where(d > 0, d, 1.0), 1.0)
    Ns, bs = N * d[:, None] * d[None, :], b * d
    try:
        q = np.linalg.solve(Ns, bs)
        if not np.all(np.isfinite(q)):
            raise np.linalg.LinAlgError
    except np.linalg.LinAlgError:
        q = np.linalg.lstsq(Ns, bs, rcond=None)[0]
    return q * d


def solve_normal(sums: np.ndarray, only_translation: bool = False) -> np.ndarray:
    """The least-squares parameters ``(t1, t2, t3[, alpha1, alpha2, alpha3])`` from the 29 sums: N p = b with N the (leading 3 x 3 of the)
    6 x 6 normal matrix (``solve_scaled``)."""
    N = np.zeros((6, 6), dtype=np.float64)
    N[np.triu_indices(6)] = sums[:21]
    k = 3 if only_translation else 6
    return solve_scaled((N + np.triu(N, 1).T)[:k, :k], np.array(sums[21:27], dtype=np.float64)[:k])


def design_rows(arrays) -> np.ndarray:
    """(6, k): the model's derivatives by (t1, t2, t3, alpha1, alpha2, alpha3) per pixel -- the rows the kernel accumulates:
    (-gx, -gy, 1, y + gy z, -x - gx z, gx y - gy x).  The model is linear: its residual is ``p @ rows - dh``."""
    x, y, z, _, gx, gy = arrays
    return np.array([-gx, -gy, np.ones_like(x), y + gy * z, -x - gx * z, gx * y - gy * x])


# ---- what LZD and ICP share ---------------------------------------------------------------------------------------------------------
def _iterate_method(method: Callable[[Any], tuple[Any, float]], iterating_input: Any, tolerance: float, max_iterations: int) -> tuple[Any, list]:
    """Upstream's ``_iterate_method`` (affine.py:102-147) in general: ``method(input)`` returns ``(new input, statistic)``; the loop stops
    after an iteration with ``i > 1 and statistic < tolerance``.  (The constant inputs are the method's own, by closure.)  Returns the
    last input and the ``(input, statistic)`` of every iteration."""
    new_inputs, history = iterating_input, []
    for i in range(int(max_iterations)):
        new_inputs, new_statistic = method(new_inputs)
        history.append((new_inputs, new_statistic))
        if i > 1 and new_statistic < tolerance:
            break
    return new_inputs, history


def _iterate(step_matrix: Callable[[np.ndarray], np.ndarray], max_iterations: int, tolerance: float) -> tuple[np.ndarray, list]:
    """``_iterate_method`` for the methods that compose step matrices (LZD, ICP): ``step_matrix(matrix)`` makes an iteration's step from
    the transform so far.  Returns the transform and the ``(transform, statistic)`` of every iteration; the statistic is upstream's,
    |t1 + t2 + t3|."""

    def method(matrix: np.ndarray) -> tuple[np.ndarray, float]:
        step = step_matrix(matrix)
        return step @ matrix, float(np.sqrt(np.sum(step[:3, 3]) ** 2))

    matrix, history = _iterate_method(method, np.eye(4), tolerance, max_iterations)
    return matrix, [(m.copy(), stat) for m, stat in history]


class _RigidStep(_Step):
    """What the steps that estimate a rotation and a translation (LZD, ICP, CPD) share -- the counterpart of ``coreg._TranslationStep``: the
    front of ``fit``, the writing of its outputs, ``apply`` through ``apply_matrix`` and the accessors of the stored transform."""

    def _check(self) -> None:   # (a step's own checks of its inputs, made before anything of the call is stored)
        pass

    @contextlib.contextmanager
    def _open(self, reference_elev, to_be_aligned_elev, inlier_mask, bias_vars, weights, subsample, random_state, transform, resolution):
        """The front of ``fit``: the refusals, ``subsample`` / ``random_state`` into ``meta``, the dh plan (at least 2 x 2), the transform."""
        name = type(self).__name__
        _check_weights(weights)
        if bias_vars is not None:
            raise NotImplementedError(f"bias_vars is not used by {name}.")
        if hasattr(reference_elev, "geometry") or hasattr(to_be_aligned_elev, "geometry"):
            raise NotImplementedError("point-cloud inputs are not supported: both elevation datasets must be arrays on one grid")
        self._check()
        if subsample is not None:
            self.meta["inputs"]["random"]["subsample"] = subsample
        if random_state is not None:
            self.meta["inputs"]["random"]["random_state"] = random_state
        logging.info(f"Running {name} coregistration")
        with DhPlan(reference_elev, to_be_aligned_elev, inlier_mask) as plan:
            if plan.shape[0] < 2 or plan.shape[1] < 2:
                raise ValueError("Shape of array too small for calculating a numerical gradient, at least (edge_order + 1) elements are required.")
            yield plan, _transform6(transform, resolution, plan.shape)

    def _store(self, centroid, matrix: np.ndarray, n: int, history: list) -> None:
        """``meta["outputs"]`` of a fit: "affine", "random", "iterative"."""
        self.meta["outputs"]["affine"] = {"centroid": centroid, "matrix": matrix, "shift_x": matrix[0, 3], "shift_y": matrix[1, 3],
                                          "shift_z": matrix[2, 3]}
        self.meta["outputs"]["random"] = {"subsample_final": int(n)}
        self.meta["outputs"]["iterative"] = {"last_iteration": len(history), "last_tolerance": history[-1][1] if history else None,
                                             "matrices": [h[0] for h in history], "statistics": [h[1] for h in history]}

    def apply(self, elev, bias_vars=None, resample: bool = True, resampling: str = "bilinear", transform=None, crs=None, z_name=None,
              resolution=None):
        """``Coreg.apply`` for an affine method that is no translation (base.py:2701-2725): ``apply_matrix`` with the stored matrix
        around the stored centroid.  With ``transform=`` the call returns ``(array, transform)``, with ``resolution=`` the array."""
        if "affine" not in self.meta["outputs"]:
            raise AssertionError(".fit() does not seem to have been called yet")
        if bias_vars is not None:
            raise NotImplementedError(f"bias_vars is not used by {type(self).__name__}.")
        if not resample:
            raise NotImplementedError(f"Option `resample=False` not supported by {self.__class__},"
                                      f" only available for translation coregistrations such as NuthKaab.")
        if resampling not in ("bilinear", "linear"):
            raise NotImplementedError(f"resampling={resampling!r}: only \"linear\" is implemented for matrices with a rotation.")
        arr = _args.nan_filled(elev)
        t6 = _transform6(transform, resolution, np.shape(arr))
        out, _ = apply_matrix(arr, self.to_matrix(), centroid=self.meta["outputs"]["affine"]["centroid"], resample=True, resampling="linear",
                              transform=t6)
        return _with_transform(out, transform)

    @property
    def is_affine(self) -> bool:
        return True

    def to_matrix(self) -> np.ndarray:
        return np.array(self.meta["outputs"]["affine"]["matrix"], dtype=np.float64)

    def centroid(self) -> tuple[float, float, float] | None:
        """The centroid the rotation is centred on (``AffineCoreg.centroid``); None before ``fit``."""
        return self.meta["outputs"].get("affine", {}).get("centroid")

    def to_translations(self) -> tuple[float, float, float]:
        return tuple(float(v) for v in self.to_matrix()[:3, 3])

    def to_rotations(self, return_degrees: bool = True) -> tuple[float, float, float]:
        """Extrinsic Euler rotations about X, Y and Z of the estimated transform."""
        return tuple(float(v) for v in translations_rotations_from_matrix(self.to_matrix(), return_degrees=return_degrees)[3:])


# ---- LZD ----------------------------------------------------------------------------------------------------------------------------
class LZD(_RigidStep):
    """Least Z-difference coregistration (Rosenholm & Torlegard 1988): a rigid transform (rotation + translation) between two DEMs on
    one grid.  Constructor of ``xdem.coreg.LZD`` (affine.py:2559-2589).  The estimated transform lands in
    ``meta["outputs"]["affine"]``: "matrix", rotation centred on "centroid", and the translations "shift_x", "shift_y", "shift_z"."""

    def __init__(self, only_translation: bool = False, fit_minimizer: Callable[..., Any] = scipy.optimize.least_squares,
                 fit_loss_func: Callable[[np.ndarray], Any] | str = "linear", max_iterations: int = 200, tolerance: float = 0.01,
                 subsample: float | int = 5e5, initial_shift=None) -> None:
        if initial_shift is not None:
            raise NotImplementedError("LZD(initial_shift=...) is not implemented here.")
        if not callable(fit_minimizer):
            raise TypeError(f"Argument `fit_minimizer` must be a function (callable), got {type(fit_minimizer)}.")
        self.meta: dict[str, Any] = {
            "inputs": {
                "fitorbin": {"fit_or_bin": "fit", "fit_minimizer": fit_minimizer, "fit_loss_func": fit_loss_func},
                "iterative": {"max_iterations": max_iterations, "tolerance": tolerance},
                "random": {"subsample": subsample, "random_state": None},
                "affine": {"only_translation": bool(only_translation)},
            },
            "outputs": {},
        }
        self._needs_vars = False
        self._needs_transform = True   # (DEM.coregister_3d: the rotation is about a centroid in the grid's coordinates)

    def _device_route(self) -> bool:
        fb = self.meta["inputs"]["fitorbin"]
        return fb["fit_minimizer"] is scipy.optimize.least_squares and isinstance(fb["fit_loss_func"], str) and fb["fit_loss_func"] == "linear"

    def _step_matrix(self, plan: DhPlan, t6, matrix, centroid, **kwargs: Any) -> np.ndarray:
        """The step transform of one iteration (``_lzd_fit``, affine.py:1511-1586)."""
        only_t = self.meta["inputs"]["affine"]["only_translation"]
        if self._device_route() and not kwargs:
            sums, cnt = lzd_normal(plan, t6, matrix, centroid)
            if cnt == 0:
                raise ValueError(LZD_NO_VALID)
            p = solve_normal(sums, only_t)
        else:
            inputs = tuple(lzd_values(plan, t6, matrix, centroid))
            if inputs[0].size == 0:
                raise ValueError(LZD_NO_VALID)
            fb = self.meta["inputs"]["fitorbin"]
            n_par = 3 if only_t else 6
            rows, dh = design_rows(inputs)[:n_par], inputs[3]
            results = fb["fit_minimizer"](lambda p: np.asarray(p) @ rows - dh, np.zeros(n_par), loss=fb["fit_loss_func"], **kwargs)
            p = results.x
        return matrix_from_translations_rotations(*p, use_degrees=False)

    def fit(self, reference_elev, to_be_aligned_elev, inlier_mask=None, bias_vars=None, weights=None, subsample=None, transform=None,
            crs=None, area_or_point=None, z_name=None, random_state=None, resolution=None, **kwargs: Any) -> "LZD":
        """Estimate the rigid transform from the to-be-aligned DEM to the reference, both arrays on one grid (``Coreg.fit`` with
        ``_fit_rst_rst``, affine.py:1680-1776).  The grid comes from ``transform``, or from ``resolution`` alone (then its origin is
        the lower-left corner).  ``kwargs`` go to ``fit_minimizer`` (and select the host route); the iterations' matrices and
        statistics land in ``meta["outputs"]["iterative"]``."""
        with self._open(reference_elev, to_be_aligned_elev, inlier_mask, bias_vars, weights, subsample, random_state, transform, resolution) as (plan, t6):
            n = draw(plan, self.meta["inputs"]["random"]["subsample"], self.meta["inputs"]["random"]["random_state"])
            centroid, _ = lzd_centroid(plan, t6)
            it = self.meta["inputs"]["iterative"]
            matrix, history = _iterate(lambda m: self._step_matrix(plan, t6, m, centroid, **kwargs), it["max_iterations"], it["tolerance"])
        self._store(centroid, matrix, n, history)
        return self
