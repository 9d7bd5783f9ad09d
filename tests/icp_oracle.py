"""CPU oracle for ICP -- TEST INFRASTRUCTURE, NOT PRODUCT CODE (NumPy / SciPy, float64, own code).

What csrc/icp.hip and xdem_amd/icp.py compute, restated from ``xdem/coreg/affine.py:296-328, 773-1182``:

* ``normals`` / ``valid_mask``: ``_icp_norms`` with the gradient quotient in the raster dtype, ``g / sqrt(1 + g^2)`` (= sin(arctan g)) in
  float64 rounded once to the dtype, ``nz`` in the dtype; validity = inlier & finite rasters & finite normals.
* ``clouds`` / ``standardize``: pixel-centre coordinates, the per-axis median as centroid, the mean of the three NMADs
  (``1.4826 * median|v - median v|``) as scale.
* ``apply`` (explicit sums, the device's order) and ``apply_blas`` (NumPy's product, as upstream's ``_apply_matrix_pts_mat``).
* ``nearest_brute`` (every pair, ``(dx dx + dy dy) + dz dz``, lowest index on ties) and ``nearest_tree`` (``scipy.spatial.KDTree``).
* ``picky``: per reference index the query of smallest distance, first occurrence on ties, ordered by reference index (NumPy only).
* ``pair_terms`` / ``fit_sums`` (``math.fsum``) / ``gauss_newton`` (lstsq on the rows, independent of the product's normal equations;
  point-to-point on the rows of the vector residual p' - q, since the rows of the scalar distance leave out r grad^2 r = I - u u^T
  and a Gauss-Newton loop on them does not converge) / ``lsq_approx``: the fit.
* ``iteration`` / ``drive``: ``_icp_iteration_step`` under ``_iterate_method``."""
from __future__ import annotations

import math

import numpy as np

NMAD_FACTOR = 1.4826
GN_MAX_EVALUATIONS = 50
GN_UPDATE_TOLERANCE = 1e-14


# ---- rasters to clouds ----------------------------------------------------------------------------------------------------------
def sin_atan(g: np.ndarray) -> np.ndarray:
    d = g.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        v = d / np.sqrt(1.0 + d * d)
        v = np.where(np.abs(d) > 1e150, np.copysign(1.0, d), v)
    return v.astype(g.dtype)


def normals(ref: np.ndarray, res_x: float, res_y: float):
    """(nx, ny, nz) in ref's dtype: nx = -sin(arctan(d/dcol / res_y)), ny = sin(arctan(d/drow / res_x)), nz = 1 - sqrt(nx^2 + ny^2)."""
    dt = ref.dtype.type
    with np.errstate(invalid="ignore", over="ignore"):
        g_row, g_col = np.gradient(ref)
        nx = -sin_atan(g_col / dt(res_y))
        ny = sin_atan(g_row / dt(res_x))
        nz = dt(1) - np.sqrt(nx * nx + ny * ny)
    return nx, ny, nz


def valid_mask(ref, tba, inlier=None, norms=None) -> np.ndarray:
    m = np.isfinite(ref) & np.isfinite(tba)
    if inlier is not None:
        m &= np.asarray(inlier, dtype=bool)
    if norms is not None:
        m &= np.isfinite(norms[0]) & np.isfinite(norms[1]) & np.isfinite(norms[2])
    return m


def clouds(ref, tba, mask, t6, norms=None):
    """(ref_epc, tba_epc, norms): (3, n) float64 arrays of the masked pixels in raster order, pixel-centre x and y."""
    a, _, c, _, e, f = (float(v) for v in t6)
    rows, cols = np.nonzero(mask)
    x, y = c + (cols.astype(np.float64) + 0.5) * a, f + (rows.astype(np.float64) + 0.5) * e
    ref_epc = np.vstack((x, y, ref[mask].astype(np.float64)))
    tba_epc = np.vstack((x, y, tba[mask].astype(np.float64)))
    n3 = None if norms is None else np.vstack([p[mask].astype(np.float64) for p in norms])
    return ref_epc, tba_epc, n3


def nmad(v: np.ndarray) -> float:
    return float(NMAD_FACTOR * np.median(np.abs(v - np.median(v))))


def standardize(ref_epc, tba_epc, scale_std: bool = True):
    """``_standardize_epc``: (ref_epc, tba_epc, centroid, std_fac)."""
    centroid = np.median(ref_epc, axis=1)
    ref_epc = ref_epc - centroid[:, None]
    tba_epc = tba_epc - centroid[:, None]
    std_fac = 1.0
    if scale_std:
        std_fac = float(np.mean([nmad(ref_epc[0]), nmad(ref_epc[1]), nmad(ref_epc[2])]))
        ref_epc, tba_epc = ref_epc / std_fac, tba_epc / std_fac
    return ref_epc, tba_epc, (float(centroid[0]), float(centroid[1]), float(centroid[2])), std_fac


# ---- the transform ----------------------------------------------------------------------------------------------------------------
def apply(matrix, pts: np.ndarray) -> np.ndarray:
    """M p with the products as explicit sums ((m0 x + m1 y) + m2 z) + m3: the device's order."""
    m = np.asarray(matrix, dtype=np.float64)
    x, y, z = pts
    return np.array([((m[i, 0] * x + m[i, 1] * y) + m[i, 2] * z) + m[i, 3] for i in range(3)])


def apply_blas(matrix, pts: np.ndarray) -> np.ndarray:
    """``_apply_matrix_pts_mat`` without a centroid: NumPy's own matrix product on the 4 x N array."""
    return (np.asarray(matrix, dtype=np.float64) @ np.concatenate((pts, np.ones((1, pts.shape[1])))))[:3, :]


# ---- nearest neighbour ------------------------------------------------------------------------------------------------------------
def nearest_brute(ref: np.ndarray, qry: np.ndarray, chunk: int = 256):
    """(dist, ind) over every pair; np.argmin returns the first (lowest) index of the minimum."""
    m = qry.shape[1]
    dist, ind = np.empty(m), np.empty(m, dtype=np.int64)
    for s in range(0, m, chunk):
        q = qry[:, s: s + chunk]
        dx, dy, dz = (q[a][:, None] - ref[a][None, :] for a in range(3))
        d2 = (dx * dx + dy * dy) + dz * dz
        j = np.argmin(d2, axis=1)
        ind[s: s + chunk] = j
        dist[s: s + chunk] = np.sqrt(d2[np.arange(q.shape[1]), j])
    return dist, ind


def nearest_tree(ref: np.ndarray, qry: np.ndarray, tree=None):
    import scipy.spatial

    tree = tree if tree is not None else scipy.spatial.KDTree(ref.T)
    dist, ind = tree.query(qry.T, k=1)
    return dist, ind.astype(np.int64)


def picky(ind: np.ndarray, dist: np.ndarray):
    """(query indexes, reference indexes) of the pairs kept, ordered by reference index: per reference index the smallest distance,
    the lowest query index among equals (pandas ``groupby(ind).idxmin()``)."""
    order = np.lexsort((np.arange(ind.size), dist, ind))
    first = np.ones(ind.size, dtype=bool)
    first[1:] = ind[order][1:] != ind[order][:-1]
    q = order[first]
    return q, ind[q]


def pairs(ind, dist, use_picky: bool):
    if use_picky:
        return picky(ind, dist)
    return np.arange(ind.size), ind


# ---- the fit ----------------------------------------------------------------------------------------------------------------------
def pair_terms(ref, trans, norms, S, method: str):
    """(J (6, k), r (k)) at the step transform S: p' = S trans; point-to-plane r = (p' - q) . n, J = [p' x n, n]; point-to-point
    r = |p' - q|, u = (p' - q) / r, J = [p' x u, u], a zero row where r = 0."""
    p = apply(S, trans)
    d = p - ref
    if method == "point-to-plane":
        u = norms
        r = (d[0] * u[0] + d[1] * u[1]) + d[2] * u[2]
    elif method == "point-to-point":
        r = np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
        with np.errstate(invalid="ignore", divide="ignore"):
            u = np.where(r > 0, d / r, 0.0)
    else:
        raise ValueError("ICP method must be 'point-to-point' or 'point-to-plane'.")
    J = np.array([p[1] * u[2] - p[2] * u[1], p[2] * u[0] - p[0] * u[2], p[0] * u[1] - p[1] * u[0], u[0], u[1], u[2]])
    return J, r


def fit_sums(J: np.ndarray, r: np.ndarray, p: np.ndarray | None = None):
    """(28 sums, 28 sums of magnitudes): the upper triangle of J J^T row by row, J r, sum r^2, each through math.fsum.  With the
    moved points ``p`` (3, k) nine more: the sums of x^2, y^2, z^2, xy, xz, yz, x, y, z."""
    terms = [J[i] * J[j] for i in range(6) for j in range(i, 6)] + [J[i] * r for i in range(6)] + [r * r]
    if p is not None:
        terms += [p[0] * p[0], p[1] * p[1], p[2] * p[2], p[0] * p[1], p[0] * p[2], p[1] * p[2], p[0], p[1], p[2]]
    return np.array([math.fsum(t) for t in terms]), np.array([math.fsum(np.abs(t)) for t in terms])


def rodrigues(x) -> np.ndarray:
    w, out = np.asarray(x[:3], dtype=np.float64), np.eye(4)
    theta = float(np.linalg.norm(w))
    K = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    if theta > 0:
        a = math.sin(theta) / theta if theta > 1e-8 else 1.0 - theta * theta / 6.0
        b = (1.0 - math.cos(theta)) / (theta * theta) if theta > 1e-4 else 0.5 - theta * theta / 24.0
        out[:3, :3] = np.eye(3) + a * K + b * (K @ K)
    out[:3, 3] = x[3:]
    return out


def _helpers():
    from xdem_amd import rigid   # (the matrix helpers are pinned against the reference by tests/test_lzd_host.py)

    return rigid.matrix_from_translations_rotations, rigid.translations_rotations_from_matrix


def gauss_newton(ref, trans, norms, method: str, only_translation: bool = False):
    """(step matrix, S, evaluations): Gauss-Newton from the identity, each update the least-squares solution of J^T x = -r by lstsq on
    the rows (columns scaled to unit norm), S <- T(omega, dt) S, until every component of the update is below 1e-14 or 50 evaluations."""
    from_params, to_params = _helpers()
    S, n_eval = np.eye(4), 0
    while n_eval < GN_MAX_EVALUATIONS:
        if method == "point-to-plane":
            J, r = pair_terms(ref, trans, norms, S, method)
            A, b = (J[3:] if only_translation else J), -r
        else:   # the vector residual d = p' - q: three rows per pair, d(omega, dt) = d + omega x p' + dt
            p = apply(S, trans)
            z, o = np.zeros(p.shape[1]), np.ones(p.shape[1])
            A = np.hstack([np.array([z, p[2], -p[1], o, z, z]), np.array([-p[2], z, p[0], z, o, z]), np.array([p[1], -p[0], z, z, z, o])])
            A, b = (A[3:] if only_translation else A), -(p - ref).ravel()
        scale = np.sqrt(np.sum(A * A, axis=1))
        scale = np.where(scale > 0, scale, 1.0)
        sol = np.linalg.lstsq((A / scale[:, None]).T, b, rcond=None)[0] / scale
        x = np.concatenate((np.zeros(3), sol)) if only_translation else sol
        n_eval += 1
        S = rodrigues(x) @ S
        if np.abs(x).max() < GN_UPDATE_TOLERANCE:
            break
    return from_params(*to_params(S, return_degrees=False), use_degrees=False), S, n_eval


def lsq_approx(ref, trans, norms):
    """Low (2004) as ``_icp_fit_approx_lsq`` writes it: A = [tba x n, n], B = (ref - tba) . n, x = lstsq(A, B) = (alpha, t)."""
    from_params, _ = _helpers()
    A = np.hstack((np.cross(trans.T, norms.T), norms.T))
    B = np.sum(ref.T * norms.T, axis=1) - np.sum(trans.T * norms.T, axis=1)
    x = np.linalg.lstsq(A, B, rcond=None)[0]
    return from_params(alpha1=x[0], alpha2=x[1], alpha3=x[2], t1=x[3], t2=x[4], t3=x[5], use_degrees=False), x, A


def fit_func(inputs, params, method: str):
    """``_icp_fit_func`` restated for a host minimiser (params: t1, t2, t3[, alpha1, alpha2, alpha3] in radians)."""
    from_params, _ = _helpers()
    ref, tba, norm = inputs
    m = from_params(*tuple(params), *((0.0,) * (6 - len(params))), use_degrees=False)
    trans = apply_blas(m, tba)
    if method == "point-to-point":
        return np.sqrt(np.sum((trans - ref) ** 2, axis=0))
    return np.sum((trans - ref) * norm, axis=0)


def solve(ref, trans, norms, method, route, only_translation, minimizer=None, loss="linear"):
    """The step matrix of one iteration by route: "device" (Gauss-Newton), "lsq_approx", or "host" (a SciPy-style minimiser)."""
    if route == "lsq_approx":
        return lsq_approx(ref, trans, norms)[0]
    if route == "device":
        return gauss_newton(ref, trans, norms, method, only_translation)[0]
    from_params, _ = _helpers()
    res = minimizer(lambda p: fit_func((ref, trans, norms), p, method), np.zeros(3 if only_translation else 6), loss=loss)
    return from_params(*res.x, *((0.0,) * 3 if only_translation else ()), use_degrees=False)


# ---- the driver -------------------------------------------------------------------------------------------------------------------
def iteration(matrix, ref_epc, tba_epc, norms, method, use_picky, only_translation, route="device", tree=None, blas=False, brute=False,
              minimizer=None, loss="linear"):
    """One ``_icp_iteration_step``: dict with trans, ind, dists, kept_q, kept_r, step, matrix (new), stat."""
    trans = apply_blas(matrix, tba_epc) if blas else apply(matrix, tba_epc)
    dists, ind = nearest_brute(ref_epc, trans) if brute else nearest_tree(ref_epc, trans, tree)
    kq, kr = pairs(ind, dists, use_picky)
    step = solve(ref_epc[:, kr], trans[:, kq], None if norms is None else norms[:, kr], method, route, only_translation, minimizer, loss)
    return {"trans": trans, "ind": ind, "dists": dists, "kept_q": kq, "kept_r": kr, "step": step, "matrix": step @ matrix,
            "stat": float(np.sqrt(np.sum(step[:3, 3]) ** 2))}


def drive(ref_epc, tba_epc, norms, method, use_picky, only_translation, tolerance, max_iterations, route="device", **kw):
    """``_iterate_method`` over ``iteration`` on standardised clouds: (final matrix in standardised coordinates, list of iterations)."""
    import scipy.spatial

    tree = scipy.spatial.KDTree(ref_epc.T)
    matrix, trail = np.eye(4), []
    for i in range(int(max_iterations)):
        it = iteration(matrix, ref_epc, tba_epc, norms, method, use_picky, only_translation, route, tree, **kw)
        matrix = it["matrix"]
        trail.append(it)
        if i > 1 and it["stat"] < tolerance:
            break
    return matrix, trail
