"""ICP coregistration on MI355X -- host-side mirror of ``xdem.coreg.ICP`` (``xdem/coreg/affine.py:296-328, 773-1182, 2107-2259``; Besl &
McKay 1992, Chen & Medioni 1992, Low 2004, Zinsser et al. 2003) for two rasters on one grid, and ``nearest``: an exact 3-D
nearest-neighbour search between two clouds.  Re-exported by ``xdem_amd.coreg``.

Every pass over the rasters and the clouds runs in ``csrc/icp.hip``:

* ``ICP.fit`` builds a dh plan, makes the normal planes (point-to-plane; they narrow the valid mask), draws the subsample, gathers the
  two clouds and standardises them with exact medians, builds the search grid once, and iterates as upstream's ``_iterate_method``
  does: one query (``scipy.spatial.KDTree.query`` upstream), the picky removal (pandas ``groupby().idxmin()`` upstream), the fit.
* The fit has three routes.  With the defaults ``fit_minimizer=scipy.optimize.least_squares`` and ``fit_loss_func="linear"`` it is a
  Gauss-Newton loop on device sums (``xdemhip_icp_sums``: one small fetch per evaluation) -- the optimum ``least_squares`` truncates
  at its ``ftol``.  ``"lsq_approx"`` is one evaluation at the identity (Low 2004).  Any other minimiser or loss gets the kept pairs
  from the device and runs on the host exactly as ``_icp_fit`` calls it.

The clouds' coordinates are pixel centres under the 6-tuple transform, as in ``xdem_amd.rigid``; NMAD is ``1.4826 * median|v - median v|``
(geoutils' ``nmad`` is absent: **parity unpinned**).  Point-cloud inputs and ``initial_shift`` are not implemented (``CPD`` is ``xdem_amd.cpd``).  The front
of ``fit``, the iteration loop, ``apply`` and the accessors are ``rigid._RigidStep``'s; ``solve_scaled`` is ``rigid``'s."""
from __future__ import annotations

import ctypes
from typing import Any, Callable

import numpy as np
import scipy.optimize

from . import _args, _lib
from ._args import c_doubles
from ._coregbase import _Plan, draw
from .biascorr import DhPlan
from .rigid import _iterate, _RigidStep, matrix_from_translations_rotations, solve_scaled, translations_rotations_from_matrix

METHODS = ("point-to-point", "point-to-plane")
BAD_METHOD = "ICP method must be 'point-to-point' or 'point-to-plane'."
BAD_LSQ_APPROX = "Fit optimizer 'lst_approx' of ICP is only available for point-to-plane method."   # (upstream's spelling)
N_SUMS = 37
GN_MAX_EVALUATIONS = 50
GN_UPDATE_TOLERANCE = 1e-14


# ---- the device passes -------------------------------------------------------------------------------------------------------------
def icp_normals(plan: DhPlan, t6, fetch: bool = True):
    """The normal planes ``(nx, ny, nz)`` of the plan's reference raster in its dtype (``xdemhip_dh_icp_normals``; ``_icp_norms``,
    affine.py:1062-1081).  The call narrows the plan's valid mask to the pixels where the three are finite -- before any draw."""
    outs = [np.empty(plan.shape, dtype=plan.dtype) if fetch else None for _ in range(3)]
    nv = ctypes.c_int64()
    plan.ctx.check(plan.ctx._L.xdemhip_dh_icp_normals(plan.handle, c_doubles(t6), *(_args.ptr(o) for o in outs), _lib.HOST,
                                                      ctypes.byref(nv)))
    plan.n_valid = int(nv.value)
    if not plan.drawn:
        plan.n_selected = plan.n_valid
    return tuple(outs) if fetch else None


class IcpCloud(_Plan):
    """Two device-resident clouds with the search grid of the first (``xdemhip_icp``): the query, the pairs and the sums of a fit."""

    _DESTROY = "xdemhip_icp_destroy"

    def __init__(self, ctx: _lib.Context, handle, n: int, m: int, has_normals: bool):
        self.ctx, self.handle, self.n, self.m, self.has_normals = ctx, handle, int(n), int(m), bool(has_normals)
        self.centroid: tuple[float, float, float] | None = None
        self.std_fac = 1.0
        ctx.adopt(self)

    @classmethod
    def from_plan(cls, plan: DhPlan, t6, with_normals: bool, standardize: bool = True) -> "IcpCloud":
        """The clouds of the plan's selected pixels, centred on the reference cloud's per-axis median and divided by the mean NMAD of
        its axes (``_standardize_epc``, affine.py:296-328): ``.centroid``, ``.std_fac``."""
        h, cnt = ctypes.c_void_p(), ctypes.c_int64()
        cen, fac = np.empty(3, dtype=np.float64), ctypes.c_double()
        plan.ctx.check(plan.ctx._L.xdemhip_icp_create_plan(plan.handle, c_doubles(t6), int(bool(with_normals)), int(bool(standardize)), ctypes.byref(h),
                                                           _args.dp(cen), ctypes.byref(fac), ctypes.byref(cnt)))
        out = cls(plan.ctx, h, cnt.value, cnt.value, with_normals)
        out.centroid, out.std_fac = (float(cen[0]), float(cen[1]), float(cen[2])), float(fac.value)
        return out

    @classmethod
    def from_points(cls, ref_points, query_points, normals=None, ctx: _lib.Context | None = None) -> "IcpCloud":
        """Arbitrary (3, N) reference and (3, M) query clouds (float64, finite), optional (3, N) normals at the reference points."""
        ref, qry = _points(ref_points, "ref_points"), _points(query_points, "query_points")
        nrm = None if normals is None else _points(normals, "normals")
        if nrm is not None and nrm.shape != ref.shape:
            raise ValueError("normals must have the shape of ref_points")
        ctx = ctx or _lib.default_context()
        h = ctypes.c_void_p()
        ctx.check(ctx._L.xdemhip_icp_create_points(ctx.handle, _args.dp(ref), ref.shape[1], _args.dp(qry), qry.shape[1], _args.dp(nrm),
                                                   ctypes.byref(h)))
        return cls(ctx, h, ref.shape[1], qry.shape[1], nrm is not None)

    def cloud(self) -> np.ndarray:
        """(7, n): x, y, ref, tba, nx, ny, nz as standardised (clouds made from a plan)."""
        out = np.empty((7, self.n), dtype=np.float64)
        self.ctx.check(self.ctx._L.xdemhip_icp_cloud(self.handle, _args.dp(out)))
        return out

    def grid(self) -> tuple[float, float, float, int, int]:
        """(x0, y0, h, columns, rows) of the search grid over the reference cloud (``xdemhip_icp_grid``)."""
        f, n = np.empty(3, dtype=np.float64), np.empty(2, dtype=np.int64)
        self.ctx.check(self.ctx._L.xdemhip_icp_grid(self.handle, _args.dp(f), _args.i64p(n)))
        return float(f[0]), float(f[1]), float(f[2]), int(n[0]), int(n[1])

    def query(self, matrix=None, fetch: bool = True):
        """Nearest reference point of every query point moved by ``matrix``: ``(dist, ind)`` as ``KDTree.query(k=1)`` returns them
        (``xdemhip_icp_query``); with ``fetch=False`` the result stays on the device for ``pairs``."""
        m16 = None if matrix is None else c_doubles(np.asarray(matrix, dtype=np.float64).ravel())
        dist = np.empty(self.m, dtype=np.float64) if fetch else None
        ind = np.empty(self.m, dtype=np.int64) if fetch else None
        self.ctx.check(self.ctx._L.xdemhip_icp_query(self.handle, m16, _args.i64p(ind), _args.dp(dist)))
        return (dist, ind) if fetch else None

    def set_pairs(self, ind, dist) -> None:
        """Put ``ind`` / ``dist`` in the place of a query's result (``xdemhip_icp_set_pairs``)."""
        ind, dist = np.ascontiguousarray(ind, dtype=np.int64), np.ascontiguousarray(dist, dtype=np.float64)
        if ind.shape != (self.m,) or dist.shape != (self.m,):
            raise ValueError("ind and dist must hold one entry per query point")
        self.ctx.check(self.ctx._L.xdemhip_icp_set_pairs(self.handle, _args.i64p(ind), _args.dp(dist)))

    def pairs(self, picky: bool, fetch: bool = False):
        """Select the pairs of the fit (``xdemhip_icp_pairs``): their number, and with ``fetch`` the kept (query, reference) indexes."""
        k = ctypes.c_int64()
        if not fetch:
            self.ctx.check(self.ctx._L.xdemhip_icp_pairs(self.handle, int(bool(picky)), ctypes.byref(k), None, None))
            return int(k.value)
        q, r = np.empty(self.m, dtype=np.int64), np.empty(self.m, dtype=np.int64)
        self.ctx.check(self.ctx._L.xdemhip_icp_pairs(self.handle, int(bool(picky)), ctypes.byref(k), _args.i64p(q), _args.i64p(r)))
        return int(k.value), q[: k.value].copy(), r[: k.value].copy()

    def sums(self, step, method: str) -> tuple[np.ndarray, int]:
        """(37 sums, count) of the kept pairs under the step transform (``xdemhip_icp_sums``): J J^T (21), J r (6), sum r^2, and the
        nine moments of the moved points (x^2, y^2, z^2, xy, xz, yz, x, y, z)."""
        s = np.empty(N_SUMS, dtype=np.float64)
        cnt = ctypes.c_int64()
        self.ctx.check(self.ctx._L.xdemhip_icp_sums(self.handle, c_doubles(np.asarray(step, dtype=np.float64).ravel()), METHODS.index(method),
                                                    _args.dp(s), ctypes.byref(cnt)))
        return s, int(cnt.value)

    def values(self, k: int) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
        """``(ref, trans, norms)``, each (3, k) float64: the kept pairs as upstream hands them to ``_icp_fit`` (``xdemhip_icp_values``)."""
        out = np.empty((9, k), dtype=np.float64)
        self.ctx.check(self.ctx._L.xdemhip_icp_values(self.handle, _args.dp(out)))
        return out[:3], out[3:6], out[6:]


def _points(a, name: str) -> np.ndarray:
    a = np.ascontiguousarray(a, dtype=np.float64)
    if a.ndim != 2 or a.shape[0] != 3 or a.shape[1] < 1:
        raise ValueError(f"{name} must be a (3, N) array with N >= 1")
    if not np.isfinite(a).all():
        raise ValueError(f"{name} must be finite")
    return a


def nearest(ref_points, query_points, matrix=None, ctx: _lib.Context | None = None) -> tuple[np.ndarray, np.ndarray]:
    """``(dist, ind)``: for every point of ``query_points`` (3, M) -- moved by the 4 x 4 ``matrix`` if one is given -- the Euclidean
    distance to and the index of its nearest point of ``ref_points`` (3, N), float64, exact; ties go to the lowest index.  What
    ``scipy.spatial.KDTree(ref_points.T).query(query_points.T, k=1)`` returns, computed on the device."""
    with IcpCloud.from_points(ref_points, query_points, ctx=ctx) as cloud:
        return cloud.query(matrix)


# ---- the solves ---------------------------------------------------------------------------------------------------------------------
def normal_system(sums: np.ndarray, count: int = 0, vector: bool = False) -> tuple[np.ndarray, np.ndarray]:
    """(normal matrix, J^T r) from the sums; parameters (rotation vector, translation).  The matrix is J^T J of the scalar rows, or
    -- ``vector``, point-to-point -- sum D^T D of the vector residual p' - q, D = [-[p']x, I], from the moments of p' and the count:
    [[sum(|p|^2 I - p p^T), sum [p]x], [sum [p]x^T, count I]].  Both have the gradient J^T r, hence the same stationary point; the scalar
    rows leave out r grad^2 r = I - u u^T, which is of the size of J^T J itself, and a Gauss-Newton loop on them does not converge."""
    b = np.array(sums[21:27], dtype=np.float64)
    if not vector:
        N = np.zeros((6, 6), dtype=np.float64)
        N[np.triu_indices(6)] = sums[:21]
        return N + np.triu(N, 1).T, b
    xx, yy, zz, xy, xz, yz, sx, sy, sz = sums[28:37]
    N = np.zeros((6, 6), dtype=np.float64)
    N[:3, :3] = [[yy + zz, -xy, -xz], [-xy, xx + zz, -yz], [-xz, -yz, xx + yy]]
    N[:3, 3:] = [[0.0, -sz, sy], [sz, 0.0, -sx], [-sy, sx, 0.0]]
    N[3:, :3] = N[:3, 3:].T
    N[3:, 3:] = float(count) * np.eye(3)
    return N, b


def gn_update(sums: np.ndarray, count: int = 0, only_translation: bool = False, vector: bool = False) -> np.ndarray:
    """The Gauss-Newton update (omega, dt) -- 6 numbers, omega = 0 with ``only_translation`` -- from the sums."""
    N, b = normal_system(sums, count, vector)
    x = np.zeros(6)
    if only_translation:
        x[3:] = solve_scaled(N[3:, 3:], -b[3:])
    else:
        x[:] = solve_scaled(N, -b)
    return x


def update_matrix(x: np.ndarray) -> np.ndarray:
    """T(omega, dt): the exact rotation by the vector omega (Rodrigues) and the translation dt."""
    w, out = np.asarray(x[:3], dtype=np.float64), np.eye(4)
    theta = float(np.sqrt(w @ w))
    K = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    if theta > 0:
        a = np.sin(theta) / theta if theta > 1e-8 else 1.0 - theta * theta / 6.0
        b = (1.0 - np.cos(theta)) / (theta * theta) if theta > 1e-4 else 0.5 - theta * theta / 24.0
        out[:3, :3] = np.eye(3) + a * K + b * (K @ K)
    out[:3, 3] = x[3:]
    return out


def gauss_newton(evaluate: Callable[[np.ndarray], tuple[np.ndarray, int]], only_translation: bool = False,
                 vector: bool = False) -> tuple[np.ndarray, int]:
    """Minimise sum r^2 over the rigid step S from the identity: ``evaluate(S)`` returns (sums, count) at S; S <- T(omega, dt) S until
    every component of the update is below 1e-14 or 50 evaluations have run.  ``vector``: the point-to-point normal matrix of
    ``normal_system``.  Returns (S, evaluations)."""
    S = np.eye(4)
    n_eval = 0
    while n_eval < GN_MAX_EVALUATIONS:
        x = gn_update(*evaluate(S), only_translation=only_translation, vector=vector)
        n_eval += 1
        S = update_matrix(x) @ S
        if np.abs(x).max() < GN_UPDATE_TOLERANCE:
            break
    return S, n_eval


def step_from(S: np.ndarray) -> np.ndarray:
    """The step matrix as upstream forms it from its parameters: translations and Euler angles of S, back into a matrix."""
    return matrix_from_translations_rotations(*translations_rotations_from_matrix(S, return_degrees=False), use_degrees=False)


def fit_func(inputs, params, method: str) -> np.ndarray:
    """``_icp_fit_func`` (affine.py:773-832) restated: the residuals of the pairs under the rigid transform of ``params``
    (t1, t2, t3[, alpha1, alpha2, alpha3], radians)."""
    ref, tba, norm = inputs
    p = tuple(params) + (0.0,) * (6 - len(params))
    matrix = matrix_from_translations_rotations(*p, use_degrees=False)
    trans = matrix[:3, :3] @ tba + matrix[:3, 3:4]
    if method == "point-to-point":
        return np.sqrt(np.sum((trans - ref) ** 2, axis=0))
    if method == "point-to-plane":
        return np.sum((trans - ref) * norm, axis=0)
    raise ValueError(BAD_METHOD)


# ---- ICP ----------------------------------------------------------------------------------------------------------------------------
class ICP(_RigidStep):
    """Iterative closest point registration: a rigid transform (rotation + translation) between two DEMs on one grid.  Constructor of
    ``xdem.coreg.ICP`` (affine.py:2137-2181).  The estimated transform lands in ``meta["outputs"]["affine"]``: "matrix", rotation
    centred on "centroid", and the translations "shift_x", "shift_y", "shift_z"."""

    def __init__(self, method: str = "point-to-plane", picky: bool = True, only_translation: bool = False,
                 fit_minimizer: Callable[..., Any] | str = scipy.optimize.least_squares, fit_loss_func: Callable[[np.ndarray], Any] | str = "linear",
                 max_iterations: int = 20, tolerance: float = 0.01, standardize: bool = True, subsample: float | int = 5e5,
                 initial_shift=None) -> None:
        if initial_shift is not None:
            raise NotImplementedError("ICP(initial_shift=...) is not implemented here.")
        self.meta: dict[str, Any] = {
            "inputs": {
                "random": {"subsample": subsample, "random_state": None},
                "fitorbin": {"fit_minimizer": fit_minimizer, "fit_loss_func": fit_loss_func},
                "iterative": {"max_iterations": max_iterations, "tolerance": tolerance},
                "affine": {"only_translation": only_translation, "standardize": standardize},
                "specific": {"icp_method": method, "icp_picky": picky},
            },
            "outputs": {},
        }
        self._needs_vars = False
        self._needs_transform = True   # (DEM.coregister_3d: the clouds live in the grid's coordinates)

    # -- the routes of _icp_fit (affine.py:888-974)
    def _route(self) -> str:
        fb = self.meta["inputs"]["fitorbin"]
        if isinstance(fb["fit_minimizer"], str) and fb["fit_minimizer"] == "lsq_approx":
            return "lsq_approx"
        if fb["fit_minimizer"] is scipy.optimize.least_squares and isinstance(fb["fit_loss_func"], str) and fb["fit_loss_func"] == "linear":
            return "device"
        return "host"

    def _check(self) -> None:
        method = self.meta["inputs"]["specific"]["icp_method"]
        if method not in METHODS:
            raise ValueError(BAD_METHOD)
        fm = self.meta["inputs"]["fitorbin"]["fit_minimizer"]
        if self._route() == "lsq_approx":
            if method != "point-to-plane":
                raise ValueError(BAD_LSQ_APPROX)
        elif not callable(fm):
            raise TypeError(f"Argument `fit_minimizer` must be a function (callable) or \"lsq_approx\", got {type(fm)}.")

    def _step_matrix(self, cloud: IcpCloud, k: int, method: str, **kwargs: Any) -> np.ndarray:
        """The step transform of one iteration from the pairs the cloud holds (``_icp_fit``)."""
        only_t = bool(self.meta["inputs"]["affine"]["only_translation"])
        route = self._route()
        if route == "lsq_approx":   # Low (2004): A = [tba x n, n], B = (ref - tba) . n = -r, x = inv(A^T A) A^T B = (alpha, t)
            N, b = normal_system(cloud.sums(np.eye(4), method)[0])
            x = solve_scaled(N, -b)
            return matrix_from_translations_rotations(alpha1=x[0], alpha2=x[1], alpha3=x[2], t1=x[3], t2=x[4], t3=x[5], use_degrees=False)
        if route == "device" and not kwargs:
            S, _ = gauss_newton(lambda S: cloud.sums(S, method), only_t, vector=method == "point-to-point")
            return step_from(S)
        inputs = cloud.values(k)
        fb = self.meta["inputs"]["fitorbin"]
        results = fb["fit_minimizer"](lambda p: fit_func(inputs, p, method), np.zeros(3 if only_t else 6), **kwargs, loss=fb["fit_loss_func"])
        return matrix_from_translations_rotations(*results.x, *((0.0,) * 3 if only_t else ()), use_degrees=False)

    def fit(self, reference_elev, to_be_aligned_elev, inlier_mask=None, bias_vars=None, weights=None, subsample=None, transform=None,
            crs=None, area_or_point=None, z_name=None, random_state=None, resolution=None, **kwargs: Any) -> "ICP":
        """Estimate the rigid transform from the to-be-aligned DEM to the reference, both arrays on one grid (``Coreg.fit`` with
        ``icp``, affine.py:1084-1182).  The grid comes from ``transform``, or from ``resolution`` alone (then its origin is the
        lower-left corner).  ``kwargs`` go to ``fit_minimizer`` (and select the host route); the iterations' matrices (standardised
        coordinates) and statistics land in ``meta["outputs"]["iterative"]``."""
        with self._open(reference_elev, to_be_aligned_elev, inlier_mask, bias_vars, weights, subsample, random_state, transform, resolution) as (plan, t6):
            it, spec = self.meta["inputs"]["iterative"], self.meta["inputs"]["specific"]
            method = spec["icp_method"]
            plane = method == "point-to-plane"
            if plane:
                icp_normals(plan, t6, fetch=False)
            n = draw(plan, self.meta["inputs"]["random"]["subsample"], self.meta["inputs"]["random"]["random_state"])
            with IcpCloud.from_plan(plan, t6, plane, bool(self.meta["inputs"]["affine"]["standardize"])) as cloud:

                def step_matrix(matrix: np.ndarray) -> np.ndarray:   # _icp_iteration_step: query, picky removal, fit
                    cloud.query(matrix, fetch=False)
                    return self._step_matrix(cloud, cloud.pairs(bool(spec["icp_picky"])), method, **kwargs)

                matrix, history = _iterate(step_matrix, it["max_iterations"], it["tolerance"] / cloud.std_fac)
                matrix[:3, 3] *= cloud.std_fac
                centroid = cloud.centroid
        self._store(centroid, matrix, n, history)
        return self
