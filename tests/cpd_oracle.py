"""CPU oracle for CPD -- TEST INFRASTRUCTURE, NOT PRODUCT CODE (NumPy, float64 and longdouble, own code).

What csrc/cpd.hip and xdem_amd/cpd.py compute, restated from ``xdem/coreg/affine.py:1190-1409``:

* ``estep``: the E-step streamed over chunks of the to-be-aligned cloud (``chunk`` points at a time, two passes, never an ``(M, N)``
  array kept): ``den``, ``P1``, ``Pt1``, ``PX``, ``Np`` and the ``sigma2`` used.  Its summation order differs from upstream's dense
  one and changes with ``chunk``.  ``perturb`` (a ``numpy.random.Generator``) multiplies every exponential by ``1 + delta``, delta
  uniform in +-2 * 2^-52: a stand-in for another ``exp`` and another order.
* ``estep_dense``: the same in ``np.longdouble`` on the dense arrays, for small clouds; also the sums of magnitudes and the largest
  exponent among the terms that do not underflow, which bound a float64 evaluation.
* ``sums``: the 18 sums of the M-step from the E-step's vectors, centred as upstream centres them.
* ``update``: ``_cpd_fit``'s lines after the sums (the 3 x 3 SVD, the matrix, q, sigma2').
* ``iteration`` / ``drive``: ``_cpd_iteration_step`` under ``_iterate_method``; ``cpd``: the whole of ``cpd()`` on two rasters.

Cloud building and standardisation are tests/icp_oracle.py's."""
from __future__ import annotations

import numpy as np

from icp_oracle import apply, clouds, standardize, valid_mask  # noqa: F401

EPS = float(np.finfo(np.float64).eps)
SVD_FAILED = "CPD coregistration numerics during np.linalg.svd(), try setting standardize=True."


def _helpers():
    from xdem_amd import rigid   # (the matrix helpers are pinned against the reference by tests/test_lzd_host.py)

    return rigid.invert_matrix


def outlier_constant(sigma2: float, weight: float, n: int, m: int) -> float:
    return (2 * np.pi * sigma2) ** (3 / 2) * weight / (1.0 - weight) * m / n


def mean_sq_distance(X: np.ndarray, TY: np.ndarray, chunk: int = 256) -> float:
    """sum |x_n - ty_m|^2 / (3 N M), pair by pair (no closed form: it cancels for clouds that are not centred)."""
    n, m, total = X.shape[1], TY.shape[1], 0.0
    for s in range(0, m, chunk):
        d = X[:, None, :] - TY[:, s: s + chunk, None]
        total += float(np.sum((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]))
    return total / (3 * n * m)


def estep(X: np.ndarray, TY: np.ndarray, sigma2: float | None, weight: float, chunk: int = 256, perturb=None, magnitudes: bool = False) -> dict:
    """X (3, N) reference, TY (3, M) moved cloud.  Two passes over chunks of M: the denominators, then P's row and column sums.
    ``magnitudes``: also ``PX_abs``."""
    n, m = X.shape[1], TY.shape[1]
    if sigma2 is None:
        sigma2 = mean_sq_distance(X, TY, chunk)

    def affinity(s):
        d = X[:, None, :] - TY[:, s: s + chunk, None]
        with np.errstate(under="ignore", divide="ignore", invalid="ignore"):
            p = np.exp(-((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]) / (2 * sigma2))
        return p

    noise = []
    den = np.zeros(n)
    for s in range(0, m, chunk):
        p = affinity(s)
        if perturb is not None:
            noise.append(1.0 + perturb.uniform(-2 * EPS, 2 * EPS, size=p.shape))
            p = p * noise[-1]
        den += p.sum(axis=0)
    c = outlier_constant(sigma2, weight, n, m)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = 1.0 / (np.clip(den, EPS, None) + c)
    P1, PX, PX_abs = np.empty(m), np.empty((3, m)), np.empty((3, m))
    for k, s in enumerate(range(0, m, chunk)):
        p = affinity(s)
        if perturb is not None:
            p = p * noise[k]
        P = p * inv[None, :]
        P1[s: s + chunk] = P.sum(axis=1)
        PX[:, s: s + chunk] = (P @ X.T).T
        if magnitudes:
            PX_abs[:, s: s + chunk] = (P @ np.abs(X).T).T
    return {"den": den, "P1": P1, "Pt1": den * inv, "PX": PX, "PX_abs": PX_abs if magnitudes else None, "Np": float(P1.sum()), "sigma2": float(sigma2)}


def largest_exponent(X: np.ndarray, TY: np.ndarray, sigma2: float, chunk: int = 256) -> float:
    """The largest |x_n - ty_m|^2 / (2 sigma2) among the pairs whose exponential does not underflow to zero (below 745)."""
    a_max = 0.0
    for s in range(0, TY.shape[1], chunk):
        d = X[:, None, :] - TY[:, s: s + chunk, None]
        a = ((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]) / (2 * sigma2)
        a = a[a < 745.0]
        if a.size:
            a_max = max(a_max, float(a.max()))
    return a_max


def estep_dense(X: np.ndarray, TY: np.ndarray, sigma2: float | None, weight: float, dtype=np.longdouble) -> dict:
    """The E-step in longdouble (or ``dtype``) on dense arrays (small clouds).  Besides the terms: ``PX_abs`` (the sums of magnitudes behind ``PX``; the
    terms of ``P1`` and ``Pt1`` are positive) and ``a_max`` (the largest exponent magnitude among the terms whose exponential is not
    zero in float64)."""
    L = dtype
    Xl, Tl = X.astype(L), TY.astype(L)
    n, m = X.shape[1], TY.shape[1]
    d = Xl[:, None, :] - Tl[:, :, None]            # (3, M, N)
    d2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
    s2 = d2.sum() / L(3 * n * m) if sigma2 is None else L(sigma2)
    a = d2 / (2 * s2)
    with np.errstate(under="ignore"):
        p = np.exp(-a)
    alive = a < 745.0
    a_max = float(a[alive].max()) if alive.any() else 0.0
    den = p.sum(axis=0)
    c = (2 * L(np.pi) * s2) ** L(1.5) * L(weight) / (1 - L(weight)) * L(m) / L(n)
    Pden = np.clip(den, L(EPS), None) + c
    P = p / Pden[None, :]
    PX = np.array([(P * Xl[k][None, :]).sum(axis=1) for k in range(3)])
    PX_abs = np.array([(P * np.abs(Xl[k])[None, :]).sum(axis=1) for k in range(3)])
    return {"den": den, "P1": P.sum(axis=1), "Pt1": P.sum(axis=0), "PX": PX, "PX_abs": PX_abs, "Np": P.sum(), "sigma2": s2, "a_max": a_max}


def sums(X: np.ndarray, Y: np.ndarray, e: dict) -> np.ndarray:
    """The 18 sums of the M-step: Np, muX, muY, A (row by row), xPx, YPY -- from the E-step ``e`` and the ORIGINAL cloud Y (3, M)."""
    P1, Pt1, PX = e["P1"], e["Pt1"], e["PX"]
    Np = np.sum(P1)
    muX = np.sum(PX, axis=1) / Np
    muY = np.sum(P1[None, :] * Y, axis=1) / Np
    X_hat, Y_hat = X - muX[:, None], Y - muY[:, None]
    YPY = np.dot(P1, np.sum(Y_hat * Y_hat, axis=0))
    xPx = np.dot(Pt1, np.sum(X_hat * X_hat, axis=0))
    A = (PX - P1[None, :] * muX[:, None]) @ Y_hat.T
    return np.concatenate(([Np], muX, muY, A.ravel(), [xPx, YPY]))


def update(s: np.ndarray, sigma2: float, sigma2_min: float, only_translation: bool = False):
    """``_cpd_fit`` after the sums: (matrix, sigma2', q)."""
    Np, muX, muY, A, xPx, YPY = s[0], s[1:4], s[4:7], s[7:16].reshape(3, 3), s[16], s[17]
    if not only_translation:
        try:
            U, _, V = np.linalg.svd(A, full_matrices=True)
        except np.linalg.LinAlgError:
            raise ValueError(SVD_FAILED)
        C = np.ones(3)
        C[2] = np.linalg.det(U @ V)
        R = (U @ np.diag(C) @ V).T
    else:
        R = np.eye(3)
    t = muX - R.T @ muY
    matrix = np.eye(4)
    matrix[:3, :3] = R
    matrix[:3, 3] = -t
    trAR = np.trace(A @ R)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = (xPx - 2 * trAR + YPY) / (2 * sigma2) + 3 * Np / 2 * np.log(sigma2)
        new = (xPx - trAR) / (Np * 3)
    if new <= 0:
        new = sigma2_min
    return matrix, float(new), float(q)


def iteration(inp, X, Y, weight, sigma2_min, only_translation, chunk: int = 256, perturb=None):
    """One ``_cpd_iteration_step``: ((matrix, sigma2, q), statistic, E-step)."""
    matrix, sigma2, q = inp
    TY = apply(_helpers()(matrix), Y)
    e = estep(X, TY, sigma2, weight, chunk, perturb)
    new_matrix, new_sigma2, new_q = update(sums(X, Y, e), e["sigma2"], sigma2_min, only_translation)
    return (new_matrix, new_sigma2, new_q), float(np.abs(q - new_q)), e


def drive(X, Y, weight, only_translation, tolerance, max_iterations, chunk: int = 256, perturb=None):
    """``_iterate_method`` over ``iteration`` on standardised clouds (``tolerance`` already divided by std_fac): (final iterating
    matrix -- NOT yet inverted --, list of dicts with matrix_in, sigma2_in, matrix, sigma2, q, stat, estep)."""
    inp, trail = (np.eye(4), None, np.inf), []
    for i in range(int(max_iterations)):
        new, stat, e = iteration(inp, X, Y, weight, tolerance / 10, only_translation, chunk, perturb)
        trail.append({"matrix_in": inp[0], "sigma2_in": inp[1], "matrix": new[0], "sigma2": new[1], "q": new[2], "stat": stat, "estep": e})
        inp = new
        if i > 1 and stat < tolerance:
            break
    return inp[0], trail


def cpd(ref, tba, inlier, t6, weight=0.0, only_translation=False, max_iterations=100, tolerance=0.01, scale_std=True, chunk: int = 256):
    """``cpd()`` on two rasters with ``subsample=1``: (final de-standardised matrix, centroid, count, trail)."""
    mask = valid_mask(ref, tba, inlier)
    X, Y, _ = clouds(ref, tba, mask, t6)
    X, Y, centroid, std_fac = standardize(X, Y, scale_std)
    final, trail = drive(X, Y, weight, only_translation, tolerance / std_fac, max_iterations, chunk)
    matrix = _helpers()(final)
    matrix[:3, 3] *= std_fac
    return matrix, centroid, X.shape[1], trail
