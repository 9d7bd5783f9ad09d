"""The rule of ``interp_points`` and ``to_pointcloud`` restated in NumPy: what ``xdemhip_spline_prepare``,
``xdemhip_spline_gather`` and ``xdemhip_raster_points`` return.  No SciPy in the filter, the weights, the dilation or the spread
rule; tests/test_interp_host.py pins each of them to SciPy.

    r = (y - f) / e - 0.5, cc = (x - c) / a - 0.5          float64 (no - 0.5 with shift_area_or_point and "Point")
    outside: r not in [0, H - 1] or cc not in [0, W - 1] (non-finite coordinates too) -> NaN
    spread = 4-connected dilation of ~isfinite(raster) by dist; a point is NaN if a bilinear corner pixel with non-zero weight is in it
    filled = every non-finite pixel takes its nearest finite pixel (the project's EDT winner on unit sampling)
    order 0: the pixel floor(r + 0.5), floor(cc + 0.5); order 1: the 4 taps of the raster itself, zero-weight taps skipped
    orders 3, 5: coefficients = the mirror spline prefilter of `filled` in float64 (columns first, then rows; per pole a gain, a
    causal and an anticausal recursion), value = the (order + 1)^2 B-spline taps, ((c wr) wc) summed from 0.0, rows outer, columns inner
    one rounding of the float64 value to the raster's dtype"""
import functools

import numpy as np

ORDERS = {"nearest": 0, "linear": 1, "cubic": 3, "quintic": 5}


def poles(order: int) -> tuple:
    if order == 3:
        return (-0.267949192431122706472553658494127633,)                                             # sqrt(3) - 2
    if order == 5:
        return (-0.430575347099973791851434783493520110, -0.043096288203264653822712376822550182)   # the closed forms lose digits
    raise ValueError(order)


def spread_distance(order: int, dist_nodata_spread="half_order_up") -> int:
    if dist_nodata_spread == "half_order_up":
        return -(-order // 2)
    if dist_nodata_spread == "half_order_down":
        return order // 2
    d = int(dist_nodata_spread)
    if d < 0:
        raise ValueError("dist_nodata_spread must be >= 0")
    return d


# ---- the prefilter ------------------------------------------------------------------------------------------------------------------
def filter_axis0(c: np.ndarray, order: int) -> np.ndarray:
    """The mirror spline prefilter along axis 0 of a float64 array (every column at once), in place on a copy."""
    c = np.array(c, dtype=np.float64)
    n = c.shape[0]
    zs = poles(order)
    gain = 1.0
    for z in zs:
        gain *= (1.0 - z) * (1.0 - 1.0 / z)
    c *= gain
    for z in zs:
        z_n_1 = z ** (n - 1)
        c0 = c[0] + z_n_1 * c[n - 1]
        z_i = z
        for i in range(1, n - 1):
            c0 = c0 + z_i * (c[i] + z_n_1 * c[n - 1 - i])
            z_i *= z
        c[0] = c0 / (1.0 - z_n_1 * z_n_1)
        for i in range(1, n):
            c[i] += z * c[i - 1]
        c[n - 1] = (z * c[n - 2] + c[n - 1]) * z / (z * z - 1.0)
        for i in range(n - 2, -1, -1):
            c[i] = z * (c[i + 1] - c[i])
    return c


def coefficients(filled: np.ndarray, order: int) -> np.ndarray:
    """float64 B-spline coefficients of a finite raster: axis 0, then axis 1."""
    if min(filled.shape) < 2:
        raise ValueError("axes of length 1 are refused")
    c = filter_axis0(np.asarray(filled, dtype=np.float64), order)
    return np.ascontiguousarray(filter_axis0(c.T, order).T)


# ---- weights and taps ---------------------------------------------------------------------------------------------------------------
def weights(t: np.ndarray, order: int) -> np.ndarray:
    """[order + 1, n] B-spline weights at the fractions ``t`` in [0, 1) past the lower middle knot; the last is 1 - the others."""
    y, z = t, 1.0 - t
    if order == 1:
        w = [1.0 - t]
    elif order == 3:
        w = [z * z * z / 6.0, (y * y * (y - 2.0) * 3.0 + 4.0) / 6.0, (z * z * (z - 2.0) * 3.0 + 4.0) / 6.0]
    elif order == 5:
        ty, tz = y * y, z * z
        w2 = (ty * (ty * (y * -10.0 + 30.0) - 60.0) + 66.0) / 120.0
        w3 = (tz * (tz * (z * -10.0 + 30.0) - 60.0) + 66.0) / 120.0
        y1, z1 = y + 1.0, z + 1.0
        w1 = (y1 * (y1 * (y1 * (y1 * (y1 * 5.0 - 45.0) + 150.0) - 210.0) + 75.0) + 51.0) / 120.0
        w4 = (z1 * (z1 * (z1 * (z1 * (z1 * 5.0 - 45.0) + 150.0) - 210.0) + 75.0) + 51.0) / 120.0
        w0 = tz * tz * z / 120.0
        w = [w0, w1, w2, w3, w4]
    else:
        raise ValueError(order)
    s = w[0]
    for k in w[1:]:
        s = s + k
    return np.stack(w + [1.0 - s])


def mirror(i: np.ndarray, n: int) -> np.ndarray:
    s2 = 2 * n - 2
    m = np.mod(i, s2)
    return np.where(m >= n, s2 - m, m)


def pixel_coordinates(x, y, transform, shift: bool = False):
    """(r, cc) in float64."""
    a, b, c, d, e, f = (float(v) for v in transform)
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        r, cc = (y - f) / e, (x - c) / a
        if not shift:
            r, cc = r - 0.5, cc - 0.5
    return r, cc


def inside(r, cc, shape):
    H, W = shape
    with np.errstate(invalid="ignore"):
        return (r >= 0) & (r <= H - 1) & (cc >= 0) & (cc <= W - 1)


# ---- nodata -------------------------------------------------------------------------------------------------------------------------
def dilate(mask: np.ndarray, dist: int) -> np.ndarray:
    """The 4-connected dilation: pixels within city-block distance ``dist`` of a mask pixel (outside the raster there is none)."""
    m = np.asarray(mask, dtype=bool).copy()
    for _ in range(int(dist)):
        g = m.copy()
        g[1:] |= m[:-1]
        g[:-1] |= m[1:]
        g[:, 1:] |= m[:, :-1]
        g[:, :-1] |= m[:, 1:]
        m = g
    return m


def spread_hit(spread: np.ndarray, r: np.ndarray, cc: np.ndarray) -> np.ndarray:
    """The integer rule: a bilinear corner pixel with non-zero weight is in ``spread`` (points inside the hull)."""
    H, W = spread.shape
    ir, ic = np.floor(r).astype(np.int64), np.floor(cc).astype(np.int64)
    wr0, wc0 = 1.0 - (r - ir), 1.0 - (cc - ic)
    wr1, wc1 = 1.0 - wr0, 1.0 - wc0
    hit = np.zeros(r.shape, bool)
    for dr, wr in ((0, wr0), (1, wr1)):
        for dc, wc in ((0, wc0), (1, wc1)):
            on = (wr != 0) & (wc != 0)
            rr, cq = np.minimum(ir + dr, H - 1), np.minimum(ic + dc, W - 1)   # (a tap past the edge has weight 0)
            hit |= on & spread[rr, cq]
    return hit


@functools.lru_cache(maxsize=None)
def _offsets(radius: int):
    """Offsets (dy, dx) within ``radius`` in the order the project's EDT prefers them from a pixel on unit sampling: the cost, then
    the smaller |dx|, then the smaller column, then the upper row."""
    d = np.arange(-radius, radius + 1)
    dy, dx = (v.ravel() for v in np.meshgrid(d, d, indexing="ij"))
    cost = dy * dy + dx * dx
    keep = cost <= radius * radius
    dy, dx, cost = dy[keep], dx[keep], cost[keep]
    o = np.lexsort((dy, dx, np.abs(dx), cost))
    return dy[o], dx[o]


def fill(raster: np.ndarray) -> np.ndarray:
    """Every non-finite pixel takes the value of its nearest finite pixel, the EDT's winner among equals (a raster with a finite pixel)."""
    a = np.array(raster)
    fin = np.isfinite(a)
    H, W = a.shape
    py, px = np.nonzero(~fin)
    radius = 4
    while py.size:
        dys, dxs = _offsets(radius)
        for dy, dx in zip(dys, dxs):
            if not py.size:
                break
            qy, qx = py + dy, px + dx
            ok = (qy >= 0) & (qy < H) & (qx >= 0) & (qx < W)
            ok[ok] = fin[qy[ok], qx[ok]]
            a[py[ok], px[ok]] = raster[qy[ok], qx[ok]]
            py, px = py[~ok], px[~ok]
        radius *= 2   # (what is left has nothing within the radius: the order restarts, a pixel's first hit is still its winner)
    return a


# ---- the calls ----------------------------------------------------------------------------------------------------------------------
class Prepared:
    """What ``xdemhip_spline_prepare`` makes of a float raster: ``spread`` (bool plane or None), ``coef`` (float64 plane or None)."""

    def __init__(self, raster, order: int, dist: int):
        self.raster = np.asarray(raster)
        if self.raster.dtype not in (np.dtype(np.float32), np.dtype(np.float64)):
            self.raster = self.raster.astype(np.float32)
        if min(self.raster.shape) < 2:
            raise ValueError("axes of length 1 are refused")
        self.order, self.dist = order, dist
        mask = ~np.isfinite(self.raster)
        self.n_nonfinite = int(mask.sum())
        self.all_nan = self.n_nonfinite == mask.size
        self.spread = dilate(mask, dist) if self.n_nonfinite and not self.all_nan else None
        self.coef = None
        if order > 1 and not self.all_nan:
            self.coef = coefficients(fill(self.raster) if self.n_nonfinite else self.raster, order)

    def values64(self, r, cc):
        """float64 values at pixel coordinates (NaN outside and in the spread)."""
        H, W = self.raster.shape
        r, cc = np.asarray(r, dtype=np.float64), np.asarray(cc, dtype=np.float64)
        out = np.full(r.shape, np.nan)
        ok = inside(r, cc, (H, W))
        if self.all_nan:
            return out
        if self.spread is not None:
            ok[ok] = ~spread_hit(self.spread, r[ok], cc[ok])
        r, cc = r[ok], cc[ok]
        if self.order == 0:
            out[ok] = self.raster[np.floor(r + 0.5).astype(np.int64), np.floor(cc + 0.5).astype(np.int64)]
            return out
        ir, ic = np.floor(r).astype(np.int64), np.floor(cc).astype(np.int64)
        wr, wc = weights(r - ir, self.order), weights(cc - ic, self.order)
        src = self.raster if self.order == 1 else self.coef
        total = np.zeros(r.shape)
        half = self.order // 2
        for i in range(self.order + 1):
            rr = mirror(ir - half + i, H)
            for j in range(self.order + 1):
                cq = mirror(ic - half + j, W)
                term = (src[rr, cq].astype(np.float64) * wr[i]) * wc[j]
                if self.order == 1:
                    term = np.where((wr[i] != 0) & (wc[j] != 0), term, 0.0)
                total = total + term
        out[ok] = total
        return out

    def at(self, x, y, transform, shift: bool = False):
        r, cc = pixel_coordinates(x, y, transform, shift)
        return self.values64(r, cc).astype(self.raster.dtype)


def interp_points(raster, transform, points, method="linear", dist_nodata_spread="half_order_up", shift: bool = False):
    order = ORDERS[method]
    return Prepared(raster, order, spread_distance(order, dist_nodata_spread)).at(points[0], points[1], transform, shift)


def raster_points(raster, transform, skip_nodata: bool = True):
    """(x, y, z): pixel-centre coordinates (float64) and values in row-major order; finite pixels only with ``skip_nodata``."""
    a = np.asarray(raster)
    if a.dtype not in (np.dtype(np.float32), np.dtype(np.float64)):
        a = a.astype(np.float32)
    ta, _, tc, _, te, tf = (float(v) for v in transform)
    rows, cols = np.nonzero(np.isfinite(a) if skip_nodata else np.ones(a.shape, bool))
    x = tc + (cols.astype(np.float64) + 0.5) * ta
    y = tf + (rows.astype(np.float64) + 0.5) * te
    return x, y, a[rows, cols]
