"""The rules of ``xdemhip_filter`` (include/xdemhip.h) restated in NumPy: this file is their definition and the device
returns its bits.  NaN means missing, +-Inf are ordinary IEEE values; 2-D float32 / float64 arrays in, the same dtype out.

* ``gaussian_filter`` -- ``scipy.ndimage.gaussian_filter(mode="reflect")`` operation for operation (``gaussian_weights``,
  ``reflect_index``, ``correlate_axis``) and, with NaNs, xDEM's normalised convolution on top of it.
* ``median_filter`` / ``min_filter`` / ``max_filter`` -- ``generic_filter(np.nanmedian / nanmin / nanmax, size, mode="constant",
  cval=nan)``: the window clipped at the raster's edge, its non-NaN values only.
* ``mean_filter`` -- square or disk footprint, the float64 sum in row-major footprint order; ``window_sum`` is that sum.
* ``distance_filter`` -- NaN wherever a pixel is further than a threshold from the unrounded disk mean around it.

**Zeros**: the device orders values by unsigned keys in which -0.0 < +0.0; NumPy's minimum, maximum and partition do not promise which
zero they return, so the planes compared bit for bit hold no zero of either sign."""
from __future__ import annotations

import numpy as np


# ---- Gaussian ---------------------------------------------------------------------------------------------------------------------------
def gaussian_radius(sigma: float, truncate: float = 4.0) -> int:
    return int(truncate * float(sigma) + 0.5)


def gaussian_weights(sigma: float, radius: int) -> np.ndarray:
    """SciPy's ``_gaussian_kernel1d(sigma, 0, radius)``: float64, normalised by NumPy's own sum."""
    sigma2 = float(sigma) * float(sigma)
    x = np.arange(-radius, radius + 1)
    phi = np.exp(-0.5 / sigma2 * x ** 2)
    return phi / phi.sum()


def reflect_index(i, n: int):
    """Index into a line of ``n`` samples mirrored about its edges (d c b a | a b c d | d c b a), repeated for any ``i``."""
    m = np.mod(np.asarray(i, dtype=np.int64), 2 * n)
    return np.where(m < n, m, 2 * n - 1 - m)


def correlate_axis(a: np.ndarray, w: np.ndarray, axis: int) -> np.ndarray:
    """SciPy's symmetric ``correlate1d`` along ``axis`` in float64, the result rounded to ``a``'s dtype."""
    lw = (w.size - 1) // 2
    n = a.shape[axis]
    x = np.moveaxis(a, axis, 0).astype(np.float64)
    at = np.arange(n)
    with np.errstate(all="ignore"):
        tmp = x * w[lw]
        for i in range(-lw, 0):
            tmp = tmp + (x[reflect_index(at + i, n)] + x[reflect_index(at - i, n)]) * w[i + lw]
        out = tmp.astype(a.dtype)
    return np.ascontiguousarray(np.moveaxis(out, 0, axis))


def _gauss(a: np.ndarray, sigma: float, truncate: float) -> np.ndarray:
    w = gaussian_weights(sigma, gaussian_radius(sigma, truncate))
    return correlate_axis(correlate_axis(a, w, 0), w, 1)


def gaussian_filter(array, sigma, truncate=4.0, normalise="auto") -> np.ndarray:
    a = np.asarray(array)
    nan = np.isnan(a)
    if normalise == "auto":
        normalise = bool(nan.any())
    if not normalise:
        return _gauss(a, sigma, truncate)
    g = _gauss(np.where(nan, a.dtype.type(0), a), sigma, truncate)
    n = _gauss((~nan).astype(a.dtype), sigma, truncate)
    with np.errstate(all="ignore"):
        out = g / n
    assert out.dtype == a.dtype
    out[nan] = np.nan
    return out


# ---- windows ----------------------------------------------------------------------------------------------------------------------------
def square_offsets(size: int):
    r = size // 2
    return [(dy, dx) for dy in range(-r, r + 1) for dx in range(-r, r + 1)]


def disk_offsets(radius: int):
    r = int(radius)
    return [(dy, dx) for dy in range(-r, r + 1) for dx in range(-r, r + 1) if dy * dy + dx * dx <= r * r]


def disk_footprint(radius: int) -> np.ndarray:
    r = int(radius)
    f = np.zeros((2 * r + 1, 2 * r + 1), dtype=bool)
    for dy, dx in disk_offsets(r):
        f[dy + r, dx + r] = True
    return f


def shifted(a: np.ndarray, dy: int, dx: int) -> np.ndarray:
    """``a[y + dy, x + dx]`` with NaN outside the raster."""
    H, W = a.shape
    out = np.full(a.shape, np.nan, dtype=a.dtype)
    ys, xs = slice(max(0, -dy), min(H, H - dy)), slice(max(0, -dx), min(W, W - dx))
    if ys.start < ys.stop and xs.start < xs.stop:
        out[ys, xs] = a[ys.start + dy:ys.stop + dy, xs.start + dx:xs.stop + dx]
    return out


def window_stack(a: np.ndarray, offsets) -> np.ndarray:
    return np.stack([shifted(a, dy, dx) for dy, dx in offsets])


def window_sum(a: np.ndarray, offsets):
    """(float64 sum of the window's non-NaN values in the order of ``offsets``, from +0.0; their count)."""
    s, n = np.zeros(a.shape, dtype=np.float64), np.zeros(a.shape, dtype=np.int64)
    with np.errstate(all="ignore"):
        for dy, dx in offsets:
            v = shifted(a, dy, dx)
            ok = ~np.isnan(v)
            s = np.where(ok, s + v.astype(np.float64), s)
            n += ok
    return s, n


def _check_size(size) -> int:
    if int(size) != size or size < 3 or size % 2 == 0:
        raise ValueError("size must be odd and >= 3")
    return int(size)


def median_filter(array, size) -> np.ndarray:
    a = np.asarray(array)
    st = np.sort(window_stack(a, square_offsets(_check_size(size))).astype(np.float64), axis=0)   # (NaN sorts last)
    n = (~np.isnan(st)).sum(axis=0)
    lo, hi = np.maximum(n - 1, 0) // 2, n // 2
    vlo, vhi = (np.take_along_axis(st, r[None], axis=0)[0] for r in (lo, hi))
    with np.errstate(all="ignore"):
        out = np.where(n % 2 == 1, vlo, (vlo + vhi) / 2.0)
    out[n == 0] = np.nan
    return out.astype(a.dtype)


def _extreme(array, size, fn, fill) -> np.ndarray:
    a = np.asarray(array)
    st = window_stack(a, square_offsets(_check_size(size)))
    nan = np.isnan(st)
    out = fn(np.where(nan, a.dtype.type(fill), st), axis=0)
    out[nan.all(axis=0)] = np.nan
    return out


def min_filter(array, size) -> np.ndarray:
    return _extreme(array, size, np.min, np.inf)


def max_filter(array, size) -> np.ndarray:
    return _extreme(array, size, np.max, -np.inf)


def mean_offsets(size=None, radius=None):
    if (size is None) == (radius is None):
        raise ValueError("exactly one of size and radius")
    if size is not None:
        return square_offsets(_check_size(size))
    if int(radius) != radius or radius < 0:
        raise ValueError("radius must be an integer >= 0")
    return disk_offsets(radius)


def mean_filter(array, size=None, radius=None) -> np.ndarray:
    a = np.asarray(array)
    s, n = window_sum(a, mean_offsets(size, radius))
    with np.errstate(all="ignore"):
        out = s / n
    out[n == 0] = np.nan
    return out.astype(a.dtype)


def distance_filter(array, radius, outlier_threshold) -> np.ndarray:
    a = np.asarray(array)
    s, n = window_sum(a, mean_offsets(None, radius))
    with np.errstate(all="ignore"):
        far = np.abs(a.astype(np.float64) - s / n) > float(outlier_threshold)
    out = a.copy()
    out[far] = np.nan
    return out


FILTERS = {"gaussian": gaussian_filter, "median": median_filter, "mean": mean_filter, "min": min_filter, "max": max_filter,
           "distance": distance_filter}
