"""CPD coregistration on MI355X -- host-side mirror of ``xdem.coreg.CPD`` (``xdem/coreg/affine.py:296-328, 1190-1409, 2262-2383``; Myronenko &
Song 2010) for two rasters on one grid, and ``cpd_expectation``: the E-step alone between any two clouds.  Re-exported by ``xdem_amd.coreg``.

One iteration of Coherent Point Drift weighs EVERY reference point against EVERY to-be-aligned point by a Gaussian affinity; upstream
materialises the ``(M, N, 3)`` differences and the ``(M, N)`` matrix ``P``.  Here ``csrc/cpd.hip`` streams over the pairs twice with
O(N + M) state and returns the eighteen sums of the M-step in one fetch (``xdemhip_cpd_estep``); what is left of an iteration
(``cpd_update``: a 3 x 3 SVD, the objective, the variance) is O(1) float64 NumPy in upstream's order of operations.

* ``CPD.fit`` builds a dh plan, draws the subsample, gathers the two clouds and standardises them with exact medians -- the front of
  ``xdem_amd.icp`` without normals and without a search grid -- and iterates as upstream's ``_iterate_method`` does on
  ``(matrix, sigma2, q)`` from ``(eye(4), None, inf)``: CPD recomputes the whole transform from the original cloud every step, nothing
  is composed, and the statistic is ``|q - q'|``.
* The clouds' coordinates are pixel centres under the 6-tuple transform, as in ``xdem_amd.rigid``; NMAD is
  ``1.4826 * median|v - median v|`` (geoutils' ``nmad`` is absent: **parity unpinned**).  Point-cloud inputs, ``initial_shift`` and
  ``scale=True`` (which upstream never passes) are not implemented.

The front of ``fit``, ``apply`` and the accessors are ``rigid._RigidStep``'s; the loop is ``rigid._iterate_method``."""
from __future__ import annotations

import ctypes
from typing import Any

import numpy as np

from . import _args, _lib
from ._args import c_doubles
from ._coregbase import _Plan, draw
from .biascorr import DhPlan
from .icp import _points
from .rigid import _iterate_method, _RigidStep, invert_matrix

N_SUMS = 18
BAD_WEIGHT = "CPD weight must be in [0, 1)."
SVD_FAILED = "CPD coregistration numerics during np.linalg.svd(), try setting standardize=True."


class CpdCloud(_Plan):
    """Two device-resident clouds and the state of an E-step between them (``xdemhip_cpd``)."""

    _DESTROY = "xdemhip_cpd_destroy"

    def __init__(self, ctx: _lib.Context, handle, n: int, m: int):
        self.ctx, self.handle, self.n, self.m = ctx, handle, int(n), int(m)
        self.centroid: tuple[float, float, float] | None = None
        self.std_fac = 1.0
        ctx.adopt(self)

    @classmethod
    def from_plan(cls, plan: DhPlan, t6, standardize: bool = True) -> "CpdCloud":
        """The clouds of the plan's selected pixels, centred on the reference cloud's per-axis median and divided by the mean NMAD of
        its axes (``_standardize_epc``, affine.py:296-328): ``.centroid``, ``.std_fac``.  What ``IcpCloud.from_plan`` yields without
        normals, by the same device code."""
        h, cnt = ctypes.c_void_p(), ctypes.c_int64()
        cen, fac = np.empty(3, dtype=np.float64), ctypes.c_double()
        plan.ctx.check(plan.ctx._L.xdemhip_cpd_create_plan(plan.handle, c_doubles(t6), int(bool(standardize)), ctypes.byref(h), _args.dp(cen),
                                                           ctypes.byref(fac), ctypes.byref(cnt)))
        out = cls(plan.ctx, h, cnt.value, cnt.value)
        out.centroid, out.std_fac = (float(cen[0]), float(cen[1]), float(cen[2])), float(fac.value)
        return out

    @classmethod
    def from_points(cls, ref_points, tba_points, ctx: _lib.Context | None = None) -> "CpdCloud":
        """Arbitrary (3, N) reference and (3, M) to-be-aligned clouds (float64, finite); nothing is centred or scaled."""
        ref, tba = _points(ref_points, "ref_points"), _points(tba_points, "tba_points")
        ctx = ctx or _lib.default_context()
        h = ctypes.c_void_p()
        ctx.check(ctx._L.xdemhip_cpd_create_points(ctx.handle, _args.dp(ref), ref.shape[1], _args.dp(tba), tba.shape[1], ctypes.byref(h)))
        return cls(ctx, h, ref.shape[1], tba.shape[1])

    def estep(self, matrix=None, sigma2: float | None = None, weight: float = 0.0) -> tuple[np.ndarray, float]:
        """One E-step with the to-be-aligned cloud moved by the 4 x 4 ``matrix`` (``xdemhip_cpd_estep``): ``(sums, sigma2)`` -- the 18
        sums ``Np, muX (3), muY (3), A (9, row by row), xPx, YPY`` of the M-step, and the variance used: ``sigma2``, or with ``None`` the
        mean squared coordinate difference over all pairs."""
        m16 = None if matrix is None else c_doubles(np.asarray(matrix, dtype=np.float64).ravel())
        s, used = np.empty(N_SUMS, dtype=np.float64), ctypes.c_double()
        self.ctx.check(self.ctx._L.xdemhip_cpd_estep(self.handle, m16, float("nan") if sigma2 is None else float(sigma2), float(weight),
                                                     _args.dp(s), ctypes.byref(used)))
        return s, float(used.value)

    def terms(self) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
        """``(P1 (M), Pt1 (N), PX (3, M))`` of the last E-step (``xdemhip_cpd_terms``)."""
        p1, pt1, px = np.empty(self.m, dtype=np.float64), np.empty(self.n, dtype=np.float64), np.empty((3, self.m), dtype=np.float64)
        self.ctx.check(self.ctx._L.xdemhip_cpd_terms(self.handle, _args.dp(p1), _args.dp(pt1), _args.dp(px)))
        return p1, pt1, px


def _check_weight(weight) -> None:
    if not 0.0 <= weight < 1.0:
        raise ValueError(BAD_WEIGHT)


def cpd_expectation(ref_points, tba_points, matrix=None, sigma2: float | None = None, weight: float = 0.0,
                    ctx: _lib.Context | None = None) -> dict[str, Any]:
    """The E-step of rigid CPD between ``ref_points`` (3, N) and ``tba_points`` (3, M) -- moved by the 4 x 4 ``matrix`` if one is given
    -- over all N M pairs, float64, on the device: ``P1`` (M), ``Pt1`` (N), ``PX`` (3, M; upstream's ``PX`` transposed), ``Np`` and the
    ``sigma2`` used (``None``: the mean squared coordinate difference over all pairs, upstream's start).  ``weight`` in [0, 1) is the
    share of the uniform outlier distribution.  What ``_cpd_fit`` (affine.py:1215-1236) forms from its dense ``P``."""
    _check_weight(weight)
    with CpdCloud.from_points(ref_points, tba_points, ctx=ctx) as cloud:
        sums, used = cloud.estep(matrix, sigma2, weight)
        p1, pt1, px = cloud.terms()
    return {"P1": p1, "Pt1": pt1, "PX": px, "Np": float(sums[0]), "sigma2": used}


def cpd_update(sums, sigma2: float, sigma2_min: float, only_translation: bool = False) -> tuple[np.ndarray, float, float]:
    """The M-step of rigid CPD (Myronenko & Song 2010, Fig. 2; what ``_cpd_fit``, affine.py:1253-1293, computes after its sums, in its
    order of operations) from the 18 sums of an E-step made with ``sigma2``: ``(matrix, sigma2', q)``.  The rotation is
    ``(U diag(1, 1, det(U V)) V)^T`` of ``U, _, V = svd(A)`` -- ``eye(3)`` with ``only_translation`` --, the scale is 1 (upstream never
    passes ``scale``), the matrix carries ``-t`` with ``t = muX - R^T muY``; a variance that comes out non-positive is replaced by
    ``sigma2_min``.  A failing SVD raises upstream's ``ValueError``; NaN sums give the NaNs they give upstream."""
    sums = np.asarray(sums, dtype=np.float64)
    Np, muX, muY, A, xPx, YPY = sums[0], sums[1:4], sums[4:7], sums[7:16].reshape(3, 3), sums[16], sums[17]
    if only_translation:
        R = np.eye(3)
    else:
        try:
            U, _, V = np.linalg.svd(A, full_matrices=True)
        except np.linalg.LinAlgError:
            raise ValueError(SVD_FAILED)
        handed = np.ones(3)
        handed[2] = np.linalg.det(U @ V)
        R = (U @ np.diag(handed) @ V).T
    matrix = np.eye(4)
    matrix[:3, :3] = R
    matrix[:3, 3] = -(muX - R.T @ muY)
    trAR = np.trace(A @ R)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = (xPx - 2 * trAR + YPY) / (2 * sigma2) + 3 * Np / 2 * np.log(sigma2)
        new_sigma2 = (xPx - trAR) / (Np * 3)
    if new_sigma2 <= 0:
        new_sigma2 = sigma2_min
    return matrix, float(new_sigma2), float(q)


class CPD(_RigidStep):
    """Coherent Point Drift registration (Myronenko & Song 2010): a rigid transform (rotation + translation) between two DEMs on one
    grid.  Constructor of ``xdem.coreg.CPD`` (affine.py:2274-2308).  The estimated transform lands in ``meta["outputs"]["affine"]``:
    "matrix", rotation centred on "centroid", and the translations "shift_x", "shift_y", "shift_z".

    ``weight`` -- the share of the uniform distribution that accounts for outliers -- must lie in [0, 1): ``ValueError`` otherwise.
    Upstream does not check it and divides by zero at 1."""

    def __init__(self, weight: float = 0, only_translation: bool = False, max_iterations: int = 100, tolerance: float = 0.01,
                 standardize: bool = True, subsample: int | float = 5e3, initial_shift=None) -> None:
        if initial_shift is not None:
            raise NotImplementedError("CPD(initial_shift=...) is not implemented here.")
        _check_weight(weight)
        self.meta: dict[str, Any] = {
            "inputs": {
                "random": {"subsample": subsample, "random_state": None},
                "iterative": {"max_iterations": max_iterations, "tolerance": tolerance},
                "affine": {"only_translation": only_translation, "standardize": standardize},
                "specific": {"cpd_weight": weight},
            },
            "outputs": {},
        }
        self._needs_vars = False
        self._needs_transform = True   # (DEM.coregister_3d: the clouds live in the grid's coordinates)

    def fit(self, reference_elev, to_be_aligned_elev, inlier_mask=None, bias_vars=None, weights=None, subsample=None, transform=None,
            crs=None, area_or_point=None, z_name=None, random_state=None, resolution=None, **kwargs: Any) -> "CPD":
        """Estimate the rigid transform from the to-be-aligned DEM to the reference, both arrays on one grid (``Coreg.fit`` with
        ``cpd``, affine.py:1340-1409).  The grid comes from ``transform``, or from ``resolution`` alone (then its origin is the
        lower-left corner).  The iterations' matrices (standardised coordinates, as ``_cpd_fit`` returns them), statistics, ``sigma2``
        and ``q`` land in ``meta["outputs"]["iterative"]``."""
        with self._open(reference_elev, to_be_aligned_elev, inlier_mask, bias_vars, weights, subsample, random_state, transform, resolution) as (plan, t6):
            it, aff = self.meta["inputs"]["iterative"], self.meta["inputs"]["affine"]
            weight, only_t = self.meta["inputs"]["specific"]["cpd_weight"], bool(aff["only_translation"])
            n = draw(plan, self.meta["inputs"]["random"]["subsample"], self.meta["inputs"]["random"]["random_state"])
            with CpdCloud.from_plan(plan, t6, bool(aff["standardize"])) as cloud:
                tolerance = it["tolerance"] / cloud.std_fac
                sigma2_min = tolerance / 10

                def step(iterating_input):   # _cpd_iteration_step: the cloud under the inverse of the matrix so far, the fit
                    matrix, sigma2, q = iterating_input
                    sums, used = cloud.estep(invert_matrix(matrix), sigma2, weight)
                    new_matrix, new_sigma2, new_q = cpd_update(sums, used, sigma2_min, only_t)
                    return (new_matrix, new_sigma2, new_q), np.abs(q - new_q)

                (final, _, _), trail = _iterate_method(step, (np.eye(4), None, np.inf), tolerance, it["max_iterations"])
                matrix = invert_matrix(final)
                matrix[:3, 3] *= cloud.std_fac
                centroid = cloud.centroid
        self._store(centroid, matrix, n, [(inp[0], float(stat)) for inp, stat in trail])
        self.meta["outputs"]["iterative"]["sigma2"] = [inp[1] for inp, _ in trail]
        self.meta["outputs"]["iterative"]["q"] = [inp[2] for inp, _ in trail]
        return self
