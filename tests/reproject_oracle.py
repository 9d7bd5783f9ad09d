"""The regridding rule of DESIGN.md ("Regridding") restated in NumPy: what ``xdemhip_regrid`` returns bit for bit.

All arithmetic is float64 in the order written.  Per axis: ``u = (o + 0.5) * r + t`` is the centre of destination pixel ``o`` in source
pixel units; ``s = min(1, 1 / r)``, ``Re = R / s``, ``K = floor(2 * Re) + 1`` taps from ``i0 = ceil(u - 0.5 - Re)``, tap ``i0 + m`` weighing
``k((i0 + m + 0.5 - u) * s)``.  The loops run over the ``Ky x Kx`` taps, rows then columns, with whole-image array operations."""
import math

import numpy as np

MIN_DEN = 1e-5          # the divisor threshold of the rule
NEAREST_EPS = 1e-10
RADIUS = {"bilinear": 1.0, "cubic": 2.0, "cubic_spline": 2.0}


def kernel(name: str, d: np.ndarray) -> np.ndarray:
    a = np.abs(d)
    if name == "bilinear":
        return np.where(a < 1.0, 1.0 - a, 0.0)
    if name == "cubic":
        return np.where(a <= 1.0, (1.5 * a - 2.5) * a * a + 1.0, np.where(a < 2.0, ((-0.5 * a + 2.5) * a - 4.0) * a + 2.0, 0.0))
    if name == "cubic_spline":
        return np.where(a <= 1.0, (0.5 * a - 1.0) * a * a + 2.0 / 3.0, np.where(a < 2.0, ((2.0 - a) * (2.0 - a)) * (2.0 - a) / 6.0, 0.0))
    raise NotImplementedError(name)


def grid_map(src_transform, transform):
    """(rx, tx, ry, ty): r = a_d / a_s, t = (c_d - c_s) / a_s per axis; the y axis uses e and f."""
    a_s, b_s, c_s, d_s, e_s, f_s = (float(v) for v in src_transform)
    a_d, b_d, c_d, d_d, e_d, f_d = (float(v) for v in transform)
    assert b_s == d_s == b_d == d_d == 0.0
    return a_d / a_s, (c_d - c_s) / a_s, e_d / e_s, (f_d - f_s) / e_s


def centres(n: int, r: float, t: float) -> np.ndarray:
    return (np.arange(n, dtype=np.float64) + 0.5) * r + t


def taps(name: str, n: int, r: float, t: float):
    """(u, i0, [weights of tap m for every destination pixel of the axis])."""
    u = centres(n, r, t)
    s = min(1.0, 1.0 / r)
    Re = RADIUS[name] / s
    K = int(math.floor(2.0 * Re)) + 1
    i0 = np.ceil(u - 0.5 - Re)
    return u, i0, [kernel(name, (i0 + m + 0.5 - u) * s) for m in range(K)]


def tap_count(name: str, r: float) -> int:
    return int(math.floor(2.0 * (RADIUS[name] / min(1.0, 1.0 / r)))) + 1


def _gather(src, rows, cols):
    """src[rows, cols] for float index vectors, with the mask of the (row, column) pairs that lie inside the source."""
    H, W = src.shape
    in_r, in_c = (rows >= 0) & (rows < H), (cols >= 0) & (cols < W)
    rr = np.where(in_r, rows, 0).astype(np.int64)
    cc = np.where(in_c, cols, 0).astype(np.int64)
    return src[rr[:, None], cc[None, :]], in_r[:, None] & in_c[None, :]


def regrid(src: np.ndarray, shape, map4, resampling: str = "bilinear", dtype=None, return_den: bool = False):
    """``src`` (H x W) onto a grid of ``shape`` = (h, w) under ``map4`` = (rx, tx, ry, ty).  Returns (array, valid_count): the count of
    pixels that are not NaN, or for uint8 of pixels taken from inside the source.  ``return_den``: also the ``den`` plane."""
    H, W = src.shape
    h, w = shape
    rx, tx, ry, ty = (float(v) for v in map4)
    if resampling == "nearest":
        fx, fy = np.floor(centres(w, rx, tx) + NEAREST_EPS), np.floor(centres(h, ry, ty) + NEAREST_EPS)
        v, inside = _gather(src, fy, fx)
        if src.dtype == np.uint8:
            out = np.where(inside, v, np.uint8(0))
            return out, int(np.count_nonzero(inside))
        dt = np.dtype(src.dtype if dtype is None else dtype)
        out = np.where(inside, v.astype(dt), dt.type(np.nan))
        return out, int(np.count_nonzero(~np.isnan(out)))
    assert src.dtype in (np.float32, np.float64)
    dt = np.dtype(src.dtype if dtype is None else dtype)
    ux, ix0, wx = taps(resampling, w, rx, tx)
    uy, iy0, wy = taps(resampling, h, ry, ty)
    num, den = np.zeros((h, w), np.float64), np.zeros((h, w), np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(len(wy)):
            for i in range(len(wx)):
                v, inside = _gather(src, iy0 + j, ix0 + i)
                v = v.astype(np.float64)
                ok = inside & np.isfinite(v)
                ww = wy[j][:, None] * wx[i][None, :]
                den = np.where(ok, den + ww, den)
                num = np.where(ok, num + ww * v, num)
        landed = ((uy >= 0) & (uy < H))[:, None] & ((ux >= 0) & (ux < W))[None, :] & (den > MIN_DEN)
        out = np.where(landed, (num / np.where(landed, den, 1.0)).astype(dt), dt.type(np.nan))
    count = int(np.count_nonzero(~np.isnan(out)))
    return (out, count, den) if return_den else (out, count)


def regrid_between(src, src_transform, shape, transform, resampling="bilinear", dtype=None):
    return regrid(src, shape, grid_map(src_transform, transform), resampling, dtype)


def target_grid(src_shape, src_transform, ref=None, res=None, grid_size=None, bounds=None):
    """The destination grid ``(shape, transform6)``: ``ref``'s; or from ``res`` (upper-left corner kept, counts
    ``max(1, floor(extent / res + 0.5))``), ``grid_size = (w, h)`` (resolution = extent / size) and ``bounds`` (left, bottom, right, top:
    the extent)."""
    H, W = src_shape
    a, _, c, _, e, f = (float(v) for v in src_transform)
    if ref is not None:
        shape, t = (ref.shape, ref.transform) if hasattr(ref, "transform") else ref
        return tuple(shape), tuple(float(v) for v in t)
    extent_x, extent_y = W * abs(a), H * abs(e)
    if bounds is not None:
        left, bottom, right, top = bounds
        extent_x, extent_y, c, f = right - left, top - bottom, left, top
    if grid_size is not None:
        w, h = grid_size
        rx, ry = extent_x / w, extent_y / h
    else:
        rx, ry = (abs(a), abs(e)) if res is None else ((res, res) if np.isscalar(res) else res)
        w, h = max(1, int(math.floor(extent_x / rx + 0.5))), max(1, int(math.floor(extent_y / ry + 0.5)))
    return (h, w), (math.copysign(rx, a), 0.0, c, 0.0, math.copysign(ry, e), f)
