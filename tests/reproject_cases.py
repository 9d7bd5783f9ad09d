"""Inputs of the regridding tests (tests/test_reproject_host.py, tests/test_reproject_gpu.py): small sources, their voids, and the
destination grids as ``(shape, map4)`` with ``map4 = (rx, tx, ry, ty)`` (tests/reproject_oracle.py)."""
import numpy as np

TW, TH = 64, 16          # the tile of the LDS route (REGRID_TW, REGRID_TH of csrc/regrid.hip)
BIG = (61, 83)
KERNELS = ("nearest", "bilinear", "cubic", "cubic_spline")
NEAR = 1e-12             # distance of a pixel centre from an integer in the near-integer cases


def terrain(shape=BIG, dtype=np.float32, seed=0) -> np.ndarray:
    rng = np.random.default_rng(seed)
    return (1000 + np.cumsum(np.cumsum(rng.normal(scale=0.2, size=shape), 0), 1)).astype(dtype)


def plane(shape, dtype=np.float32) -> np.ndarray:
    """The integer-valued plane 3x - 5y + 7 at pixel indexes (x = column, y = row)."""
    yy, xx = np.mgrid[0:shape[0], 0:shape[1]]
    return (3 * xx - 5 * yy + 7).astype(dtype)


def plane_at(ux, uy) -> np.ndarray:
    """The same plane at pixel-unit coordinates (pixel i has its centre at i + 0.5), float64."""
    return 3 * (np.asarray(ux)[None, :] - 0.5) - 5 * (np.asarray(uy)[:, None] - 0.5) + 7


def voids(kind: str, dtype=np.float32) -> np.ndarray:
    a = terrain(BIG, dtype)
    yy, xx = np.mgrid[0:BIG[0], 0:BIG[1]]
    if kind == "single":
        a[30, 41] = np.nan
    elif kind == "border_rows":
        a[0, :] = a[-1, :] = np.nan
        a[:, 0] = a[:, -1] = np.nan
    elif kind == "hole":            # wider than 2 * Re of every case it is used with (Re <= 7.4)
        a[15:45, 25:60] = np.nan
    elif kind == "checkerboard":
        a[(yy + xx) % 2 == 0] = np.nan
    elif kind == "inf":
        a[10, 10], a[10, 11], a[40, 70] = np.inf, -np.inf, np.inf
        a[20:23, 30] = -np.inf
    else:
        raise KeyError(kind)
    return a


# the checkerboard under "cubic" on this grid has pixels whose summed weight lies on both sides of the 1e-5 threshold (asserted where used)
CHECKERBOARD_MAP = (1.0002, -0.001, 1.0002, -0.001)

SMALL_SOURCES = {"1x1": (1, 1), "1x7": (1, 7), "7x1": (7, 1)}


def offsets_scale_one():
    """(name, shape, map4) on the 61 x 83 source at scale 1."""
    return [
        ("same", BIG, (1.0, 0.0, 1.0, 0.0)),
        ("whole_pixels", BIG, (1.0, 3.0, 1.0, -2.0)),
        ("fraction", BIG, (1.0, 0.5, 1.0, 0.25)),
        ("just_above_integer", BIG, (1.0, NEAR, 1.0, NEAR)),
        ("just_below_integer", BIG, (1.0, -NEAR, 1.0, -NEAR)),
        ("half_plus", BIG, (1.0, 0.5 + NEAR, 1.0, -0.5 - NEAR)),
    ]


def tile_edges():
    """Destination sizes one less than, equal to and one more than the tile, and 1 x 1, at a fractional offset."""
    out = [(f"{h}x{w}", (h, w), (1.0, 0.3, 1.0, 0.6)) for h in (TH - 1, TH, TH + 1) for w in (TW - 1, TW, TW + 1)]
    return out + [("1x1", (1, 1), (1.0, 20.25, 1.0, 30.5))]


def scales():
    return [
        ("up2.5", (150, 205), (0.4, 0.1, 0.4, 0.2)),
        ("aniso", (36, 205), (0.4, 0.3, 1.7, -0.2)),
        ("aniso_t", (150, 49), (1.7, 0.3, 0.4, -0.2)),
        ("down3.7", (17, 23), (3.7, -0.5, 3.7, 0.25)),
        ("down2", (31, 42), (2.0, 0.0, 2.0, 0.0)),
    ]


def placements():
    """Destinations that overhang each side of the source, lie wholly outside it, or wholly inside one source pixel."""
    return [
        ("over_left", (20, 70), (1.0, -10.5, 1.0, 5.25)),
        ("over_right", (20, 70), (1.0, 40.5, 1.0, 5.25)),
        ("over_top", (20, 70), (1.0, 5.5, 1.0, -9.75)),
        ("over_bottom", (20, 70), (1.0, 5.5, 1.0, 50.25)),
        ("over_all", (40, 50), (2.0, -8.0, 2.0, -9.0)),
        ("outside_right", (18, 66), (1.0, 200.0, 1.0, 3.0)),
        ("outside_above", (18, 66), (1.3, 2.0, 1.3, -500.0)),
        ("far_outside", (5, 5), (1.0, 1e17, 1.0, -1e17)),
        ("inside_one_pixel", (17, 65), (0.001, 40.2, 0.001, 30.3)),
    ]
