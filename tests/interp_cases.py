"""Shapes, rasters and points of the interp_points tests.  The shapes come from ``xdemhip_spline_plan``: the smallest at which a
stage of the prefilter can go wrong -- one band of rows or one tile of rows / columns minus one, exactly one, plus one; sides shorter
than the warm-up halo; and one raster of three bands by three tiles, whose middle band and tile start from halos on both sides."""
import functools

import numpy as np

SWITCHES = (0, 1, 2, 3)     # "spline_route": automatic, one band per column, plain rows, LDS rows
EXACT = (2.0, 0.0, 100.0, 0.0, -2.0, 5000.0)        # node and edge coordinates are exact in float64
INEXACT = (0.3, 0.0, -17.1, 0.0, -0.7, 311.3)
SOUTH_UP = (1.5, 0.0, 3.0, 0.0, 1.5, -40.0)


@functools.lru_cache(maxsize=None)
def plan():
    """The automatic constants (those of a raster large enough for every route)."""
    from xdem_amd import interp

    return interp.plan_constants(4096, 4096, 5, 0)


@functools.lru_cache(maxsize=None)
def shapes() -> dict:
    p = plan()
    band, tr, tc = p["band_rows"], p["tile_rows"], p["tile_cols"]
    out = {"tiny_5x7": (5, 7), "two_rows": (2, 97), "two_cols": (97, 2), "two_by_two": (2, 2)}
    for d in (-1, 0, 1):
        out[f"band{d:+d}"] = (band + d, 9)
        out[f"tile_rows{d:+d}"] = (tr + d, 2 * p["halo"] + 3)
        out[f"tile_cols{d:+d}"] = (5, tc + d)
    out["three_by_three"] = (2 * band + 7, 2 * tc + 9)
    return out


def surface(shape, dtype, seed: int = 0) -> np.ndarray:
    """A rough finite raster around 1000."""
    rng = np.random.default_rng([seed, *shape])
    H, W = shape
    yy, xx = np.mgrid[0:H, 0:W]
    a = 1000.0 + 40.0 * np.sin(yy / 7.0) * np.cos(xx / 5.0) + 0.3 * xx - 0.2 * yy + rng.normal(scale=5.0, size=shape)
    return np.ascontiguousarray(a.astype(dtype))


def with_voids(a: np.ndarray, kind: str, seed: int = 0) -> np.ndarray:
    """``a`` with non-finite pixels: "single", "frame", "random" (20 %), "blobs" (on tile and band corners and on the raster's edges;
    one of them +inf), "none", "all"."""
    a = a.copy()
    H, W = a.shape
    rng = np.random.default_rng([seed, H, W, len(kind)])
    if kind == "none":
        return a
    if kind == "all":
        a[:] = np.nan
    elif kind == "single":
        a[H // 2, W // 2] = np.nan
    elif kind == "frame":
        a[0], a[-1], a[:, 0], a[:, -1] = np.nan, np.nan, np.nan, np.nan
        if H <= 2 or W <= 2:   # (nothing finite would be left)
            a[0, 0] = 1000.0
    elif kind == "random":
        a[rng.random(a.shape) < 0.2] = np.nan
        a[0, 0] = 1000.0
    elif kind == "blobs":
        p = plan()
        corners = [(0, 0), (H - 1, W - 1), (0, W // 2), (H // 2, 0), (p["band_rows"], p["tile_cols"]), (p["tile_rows"], p["tile_cols"]),
                   (2 * p["band_rows"], 2 * p["tile_cols"]), (p["tile_rows"], 64), (H // 3, W // 3)]
        for k, (y, x) in enumerate(corners):
            if y < H and x < W:
                r = 1 + k % 3
                a[max(0, y - r):y + r, max(0, x - r):x + r] = np.inf if k == 4 else np.nan
        if not np.isfinite(a).any():
            a[-1, 0] = 1000.0
    else:
        raise ValueError(kind)
    return a


def pixel_points(shape, n_random: int = 1500, seed: int = 0):
    """(r, cc) pixel coordinates: random in the hull, nodes, pixel edges (half-integers), the four corners."""
    H, W = shape
    rng = np.random.default_rng([seed, H, W])
    r, c = [rng.uniform(0, H - 1, n_random)], [rng.uniform(0, W - 1, n_random)]
    k = 300
    r.append(rng.integers(0, H, k).astype(np.float64)), c.append(rng.integers(0, W, k).astype(np.float64))            # nodes
    r.append(rng.integers(0, H - 1, k) + 0.5), c.append(rng.integers(0, W - 1, k) + 0.5)                               # edges, both axes
    r.append(rng.integers(0, H, k).astype(np.float64)), c.append(rng.integers(0, W - 1, k) + 0.5)                      # node rows, edge columns
    r.append(rng.uniform(0, H - 1, k)), c.append(rng.integers(0, W, k).astype(np.float64))                            # node columns only
    r.append(np.array([0.0, 0.0, H - 1.0, H - 1.0])), c.append(np.array([0.0, W - 1.0, 0.0, W - 1.0]))               # corners
    return np.concatenate(r), np.concatenate(c)


def world_points(shape, transform, n_random: int = 1500, seed: int = 0, outside: bool = True):
    """(x, y) of ``pixel_points`` under a transform, then points outside the hull and non-finite coordinates."""
    a, _, c, _, e, f = transform
    r, cc = pixel_points(shape, n_random, seed)
    x, y = c + (cc + 0.5) * a, f + (r + 0.5) * e
    if outside:
        H, W = shape
        ro = np.array([-0.25, H - 0.75, 1.0, 1.0, -3.0, H + 5.0, np.nan, 1.0, np.inf, 1.0, -np.inf])
        co = np.array([1.0, 1.0, -0.25, W - 0.75, -3.0, W + 5.0, 1.0, np.nan, 1.0, np.inf, np.nan])
        x, y = np.concatenate([x, c + (co + 0.5) * a]), np.concatenate([y, f + (ro + 0.5) * e])
    return x, y
