"""CPU oracle for LZD and the rotation-capable raster apply -- TEST INFRASTRUCTURE, NOT PRODUCT CODE (NumPy, own code).

What csrc/rigid.hip computes, restated so that the per-pixel values agree bit for bit: float64 throughout, matrix products as explicit
sums in the order ``m0 x + m1 y + m2 z + m3`` (upstream multiplies with BLAS, whose summation order is nobody's to pin), interpolated
values rounded to the raster dtype.  The grid's coordinates are pixel centres under the 6-tuple transform ``(a, b, c, d, e, f)``,
``b = d = 0``: ``x = c + (col + 0.5) a``, ``y = f + (row + 0.5) e``.

* ``point_taps``: ``nuthkaab_oracle.bilinear_shifted``'s arithmetic and four nodata rules at arbitrary float64 (row, col).
* ``gradient_planes``: ``gradient_x / res_x`` and ``-gradient_y / res_y`` of ``np.gradient(ref)`` (affine.py:1440, 1455-1456).
* ``lzd_arrays``: the six arrays ``x, y, z, dh, gradx, grady`` upstream's ``_lzd_iteration_step`` hands ``_lzd_fit`` (affine.py:1622-1652).
* ``normal_sums``: the 29 sums of the normal equations through ``math.fsum``, and the sums of the terms' magnitudes (error bounds).
* ``regrid``: ``_iterate_affine_regrid_small_rotations`` (base.py:1389-1519) with SciPy's linear ``RegularGridInterpolator`` restated
  on the pixel grid (``rgi_linear``)."""
from __future__ import annotations

import math

import numpy as np


def pixel_xy(t6, rows, cols):
    a, _, c, _, e, f = (float(v) for v in t6)
    return c + (np.asarray(cols, dtype=np.float64) + 0.5) * a, f + (np.asarray(rows, dtype=np.float64) + 0.5) * e


def xy_to_pixel(t6, x, y):
    a, _, c, _, e, f = (float(v) for v in t6)
    return (y - f) / e - 0.5, (x - c) / a - 0.5


def apply_pts(matrix, centroid, x, y, z):
    """p' = M (p - centroid) + centroid with the products as explicit sums (no centroid: nothing subtracted)."""
    m = np.asarray(matrix, dtype=np.float64)
    x, y, z = (np.asarray(v, dtype=np.float64) for v in (x, y, z))
    with np.errstate(invalid="ignore", over="ignore"):
        if centroid is not None:
            x, y, z = x - centroid[0], y - centroid[1], z - centroid[2]
        out = [((m[i, 0] * x + m[i, 1] * y) + m[i, 2] * z) + m[i, 3] for i in range(3)]
        if centroid is not None:
            out = [o + c for o, c in zip(out, centroid)]
    return out


def point_taps(img: np.ndarray, rows, cols, nan_rule: int) -> np.ndarray:
    """bilinear(img)(rows, cols): float64 weights, ``top = v00 + fc (v01 - v00)``, ``bot = v10 + fc (v11 - v10)``,
    ``val = top + fr (bot - top)``, rounded to img's dtype; NaN by the nodata rule 0..3 of ``nuthkaab_oracle.bilinear_shifted``."""
    H, W = img.shape
    rr = np.asarray(rows, dtype=np.float64)
    cc = np.asarray(cols, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        rr = np.where((rr >= -1.0) & (rr <= H), rr, -2.0)   # not a number or a pixel and more outside: outside under every rule
        cc = np.where((cc >= -1.0) & (cc <= W), cc, -2.0)
    r0 = np.floor(rr)
    c0 = np.floor(cc)
    fr = rr - r0
    fc = cc - c0
    r0 = r0.astype(np.int64)
    c0 = c0.astype(np.int64)
    need_r1 = (fr != 0) if nan_rule == 1 else ((fr != 0) | (r0 + 1 < H))
    need_c1 = (fc != 0) if nan_rule == 1 else ((fc != 0) | (c0 + 1 < W))
    r1 = np.where(need_r1, r0 + 1, r0)
    c1 = np.where(need_c1, c0 + 1, c0)
    ok = (r0 >= 0) & (r1 < H) & (c0 >= 0) & (c1 < W)
    r0c, r1c = np.clip(r0, 0, H - 1), np.clip(r1, 0, H - 1)
    c0c, c1c = np.clip(c0, 0, W - 1), np.clip(c1, 0, W - 1)
    t = img.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        v00, v01, v10, v11 = t[r0c, c0c], t[r0c, c1c], t[r1c, c0c], t[r1c, c1c]
        top = v00 + fc * (v01 - v00)
        bot = v10 + fc * (v11 - v10)
        val = top + fr * (bot - top)
        good = ok & np.isfinite(v00) & np.isfinite(v01) & np.isfinite(v10) & np.isfinite(v11)
        if nan_rule >= 2:
            pad = np.ones((H + 2, W + 2), dtype=bool)
            pad[1:-1, 1:-1] = ~np.isfinite(img)
            dil = np.zeros((H, W), dtype=bool)
            for a in range(3):
                for b in range(3):
                    if nan_rule == 2 or a == 1 or b == 1:
                        dil |= pad[a: a + H, b: b + W]
            rn = np.floor(rr + 0.5).astype(np.int64)
            cn = np.floor(cc + 0.5).astype(np.int64)
            inside = (rn >= 0) & (rn < H) & (cn >= 0) & (cn < W)
            good = good & ~np.where(inside, dil[np.clip(rn, 0, H - 1), np.clip(cn, 0, W - 1)], True)
        return np.where(good, val, np.nan).astype(img.dtype)


def gradient_planes(ref: np.ndarray, res_x: float, res_y: float):
    """(gradx, grady) in ref's dtype: central differences with one-sided borders (``nuthkaab_oracle.gradient_unit``), divided by the
    resolution as NumPy 2 divides a float32 array by a Python float."""
    import nuthkaab_oracle

    gy, gx = nuthkaab_oracle.gradient_unit(ref)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        return gx / float(res_x), -gy / float(res_y)


def centroid(tba: np.ndarray, sel_mask: np.ndarray, t6):
    """(mean x, mean y, mean tba) over the selected pixels: integer sums of row / column; the mean of tba through fsum."""
    rows, cols = np.nonzero(sel_mask)
    n = rows.size
    a, _, c, _, e, f = (float(v) for v in t6)
    return (c + (float(int(cols.sum())) / n + 0.5) * a, f + (float(int(rows.sum())) / n + 0.5) * e,
            math.fsum(tba[sel_mask].astype(np.float64)) / n)


def lzd_arrays(ref, tba, gradx, grady, sel_mask, t6, matrix, cen, nan_rule: int):
    """(6, k) float64: x, y, z (centroid removed), dh, gradx, grady of the selected pixels left valid under ``matrix``, raster order."""
    rows, cols = np.nonzero(sel_mask)
    x, y = pixel_xy(t6, rows, cols)
    xt, yt, zt = apply_pts(matrix, cen, x, y, tba[rows, cols].astype(np.float64))
    with np.errstate(invalid="ignore", over="ignore"):
        rp, cp = xy_to_pixel(t6, xt, yt)
        dh = point_taps(ref, rp, cp, nan_rule).astype(np.float64) - zt
        gx = point_taps(gradx, rp, cp, nan_rule).astype(np.float64)
        gy = point_taps(grady, rp, cp, nan_rule).astype(np.float64)
        xo, yo, zo = xt - cen[0], yt - cen[1], zt - cen[2]
    keep = np.isfinite(dh) & np.isfinite(zo) & np.isfinite(gx) & np.isfinite(gy)
    return np.array([v[keep] for v in (xo, yo, zo, dh, gx, gy)], dtype=np.float64)


def design_rows(arr6):
    """The rows a = (-gx, -gy, 1, y + gy z, -x - gx z, gx y - gy x): derivatives of upstream's model (affine.py:1496-1503) by
    t1, t2, t3, alpha1, alpha2, alpha3."""
    x, y, z, _, gx, gy = arr6
    return np.array([-gx, -gy, np.ones_like(x), y + gy * z, -x - gx * z, gx * y - gy * x])


def normal_sums(arr6):
    """(sums[29], abs_sums[29]): the 21 upper-triangle terms of a a^T (row by row), the 6 of a dh, sum dh^2, sum dh -- each term formed
    in float64 as the kernel forms it, summed with math.fsum; abs_sums = the sums of the terms' magnitudes (plain sums: they only scale a bound)."""
    a = design_rows(arr6)
    dh = arr6[3]
    terms = [a[i] * a[j] for i in range(6) for j in range(i, 6)] + [a[i] * dh for i in range(6)] + [dh * dh, dh]
    return np.array([math.fsum(t) for t in terms]), np.array([float(np.abs(t).sum()) for t in terms])


def lstsq_step(arr6, only_translation: bool = False):
    """The least-squares parameters of one iteration by a float64 ``lstsq`` on the design matrix itself."""
    a = design_rows(arr6)
    k = 3 if only_translation else 6
    return np.linalg.lstsq(a[:k].T, arr6[3], rcond=None)[0]


def rgi_linear(dem: np.ndarray, rows, cols) -> np.ndarray:
    """scipy.interpolate.RegularGridInterpolator(method="linear", bounds_error=False) on the pixel grid, float64: NaN outside
    [0, n - 1], cell index clipped to [0, n - 2], NaN if any node of the cell is non-finite.  SciPy's cell is [k, k + 1) along an ascending
    axis; upstream's y axis ascends against the rows, so a position exactly on row k lies in the cell of rows [k - 1, k]."""
    H, W = dem.shape
    rr = np.asarray(rows, dtype=np.float64)
    cc = np.asarray(cols, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        inside = (rr >= 0) & (rr <= H - 1) & (cc >= 0) & (cc <= W - 1)
        rs, cs = np.where(inside, rr, 0.0), np.where(inside, cc, 0.0)
        i0 = np.maximum(np.ceil(rs).astype(np.int64) - 1, 0)   # (SciPy's cell along y, which ascends against the rows: (k - 1, k])
        j0 = np.minimum(np.floor(cs).astype(np.int64), W - 2)
        fr, fc = rs - i0, cs - j0
        t = dem.astype(np.float64)
        v00, v01, v10, v11 = t[i0, j0], t[i0, j0 + 1], t[i0 + 1, j0], t[i0 + 1, j0 + 1]
        gr, gc = 1.0 - fr, 1.0 - fc
        val = ((v00 * gr) * gc + (v01 * gr) * fc + (v10 * fr) * gc) + (v11 * fr) * fc
        ok = inside & np.isfinite(v00) & np.isfinite(v01) & np.isfinite(v10) & np.isfinite(v11)
    return np.where(ok, val, np.nan)


NEAR_THRESHOLD = 1e-6   # relative distance of |x0 - x| from the tolerance below which another summation order may decide otherwise


def rigid_inverse(matrix) -> np.ndarray:
    """The inverse of a rigid 4 x 4 matrix as the kernel's entry forms it: R^T and -(R^T t), the products as explicit sums."""
    m = np.asarray(matrix, dtype=np.float64)
    inv = np.eye(4)
    inv[:3, :3] = m[:3, :3].T
    for i in range(3):
        inv[i, 3] = -((m[0, i] * m[0, 3] + m[1, i] * m[1, 3]) + m[2, i] * m[2, 3])
    return inv


def regrid(dem: np.ndarray, t6, matrix, cen=None, details: bool = False):
    """(regridded DEM in dem's dtype, number of pixels that kept the value of iteration 1): upstream's fixed-point iteration, which
    checks after iterations 1 and 5 only and stores nothing after 5.  With ``details`` also the mask of the pixels whose residual at
    iteration 1 lies within NEAR_THRESHOLD (relative) of the tolerance in x or y: the ones a product summed in another order (BLAS) may
    switch between the value of iteration 1 and that of iteration 5."""
    H, W = dem.shape
    rows, cols = np.divmod(np.arange(H * W, dtype=np.int64), W)
    x, y = pixel_xy(t6, rows, cols)
    tol_x, tol_y = 1e-4 * abs(float(t6[0])), 1e-4 * abs(float(t6[4]))
    inv_matrix = rigid_inverse(matrix)
    guess = apply_pts(matrix, cen, x, y, dem.ravel().astype(np.float64))[2]
    out = np.empty(H * W, dtype=np.float64)
    active = np.arange(H * W)
    n_first = 0
    with np.errstate(invalid="ignore", over="ignore"):
        for it in range(1, 6):
            tx, ty, _ = apply_pts(inv_matrix, cen, x, y, guess)
            rp, cp = xy_to_pixel(t6, tx, ty)
            x0, y0, z0 = apply_pts(matrix, cen, tx, ty, rgi_linear(dem, rp, cp))
            out[active] = z0
            if it == 1:
                dx, dy = x0 - x, y0 - y
                conv = ((np.abs(dx) < tol_x) | ~np.isfinite(dx)) & ((np.abs(dy) < tol_y) | ~np.isfinite(dy))
                n_first = int(conv.sum())
                near = (np.abs(np.abs(dx) - tol_x) <= NEAR_THRESHOLD * tol_x) | (np.abs(np.abs(dy) - tol_y) <= NEAR_THRESHOLD * tol_y)
                active, x, y, z0 = active[~conv], x[~conv], y[~conv], z0[~conv]
                if active.size == 0:
                    break
            guess = z0
    res = out.astype(dem.dtype).reshape(H, W)
    return (res, n_first, near.reshape(H, W)) if details else (res, n_first)
