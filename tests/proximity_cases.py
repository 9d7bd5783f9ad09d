"""Inputs of the proximity tests (tests/test_proximity_host.py, tests/test_proximity_gpu.py): target planes sized from the constants
``xdemhip_edt_plan`` returns for a value of the test switch ``"edt_route"``, so that each is the smallest plane on which a stage of
``xdemhip_edt`` can go wrong; the samplings; a vector of two polygons and its grid."""
import numpy as np

EXACT = ((1.0, 1.0), (10.0, 10.0), (30.0, 20.0), (2.5, 0.5))     # products and squares exact: SciPy is the float minimum
INEXACT = ((0.1, 0.3), (1.0 / 3.0, 1.0 / 7.0))                  # SciPy's parabola intersections leave the float minimum
ANISOTROPIC = (1.0, 50.0)
SWITCHES = (0, 1, 2)


def plan(switch: int, H: int = 1, W: int = 1) -> dict:
    from xdem_amd import proximity

    return proximity.edt_plan(H, W, switch)


def empty(H, W):
    return np.zeros((H, W), np.uint8)


def with_targets(H, W, cells):
    t = empty(H, W)
    for y, x in cells:
        t[y % H, x % W] = 1
    return t


def far_width(p) -> int:
    """tile + halo + 2 blocks + 1: a corner target lies beyond the window and two blocks of the opposite corner's pixel."""
    return p["tile_cols"] + p["halo"] + 2 * p["block_cols"] + 1


def cases(switch: int) -> list:
    """``[(name, uint8 target plane)]`` for a value of the switch."""
    p = plan(switch)
    band, block = p["band_rows"], p["block_cols"]
    rng = np.random.default_rng(20 + switch)
    out = []
    # carries from above and below across an empty band: targets in the first and the last band only
    H, W = 2 * band + 3, 2 * block + 7
    t = empty(H, W)
    t[rng.integers(0, band, 9), rng.integers(0, W, 9)] = 1
    t[rng.integers(H - 3, H, 4), rng.integers(0, W, 4)] = 1
    t[:, block + 1] = 0                     # (a column without any target)
    out.append(("bands", t))
    # a single target in each corner: halo overflow, block skip, far search
    Wf, Hf = far_width(p), 5
    for name, cell in (("corner_tl", (0, 0)), ("corner_tr", (0, -1)), ("corner_bl", (-1, 0)), ("corner_br", (-1, -1))):
        out.append((name, with_targets(Hf, Wf, [cell])))
    # ties: left / right of a pixel, above / below it, and diagonal pairs of equal cost
    out.append(("ties", with_targets(9, 3 * block + 11, [(4, 3), (4, 7), (4, 8), (4, 12), (1, 20), (7, 20), (0, 30), (8, 30), (2, 2 * block + 1),
                                                          (6, 2 * block + 9), (6, 2 * block + 1), (2, 2 * block + 9)])))
    out.append(("one_pixel_target", with_targets(1, 1, [(0, 0)])))
    out.append(("one_row", with_targets(1, Wf, [(0, 2), (0, Wf - 3)])))
    out.append(("one_column", with_targets(H, 1, [(1, 0), (H - 2, 0)])))
    out.append(("all_targets", np.ones((band + 2, block + 3), np.uint8)))
    out.append(("no_target", empty(3, far_width(p))))
    out.append(("no_target_tall", empty(band + 2, 5)))
    out.append(("one_pixel_no_target", empty(1, 1)))
    out.append(("dense", (rng.random((band + 5, p["tile_cols"] + p["halo"] + 3)) < 0.02).astype(np.uint8)))
    return out


def tall() -> np.ndarray:
    """H = 32768: the first height whose row offsets need 32 bits."""
    return with_targets(32768, 3, [(0, 0), (20000, 1), (32767, 2), (5, 2)])


def tiny(seed: int, shape) -> np.ndarray:
    rng = np.random.default_rng(seed)
    return (rng.random(shape) < 0.08).astype(np.uint8)


# ---- a vector of two polygons, one with a hole, and a grid it covers partly ---------------------------------------------------------
GRID_SHAPE = (57, 83)
GRID_TRANSFORM = (20.0, 0.0, 1000.0, 0.0, -30.0, 5000.0)
POLYGONS = [
    (np.array([[1100.0, 4800.0], [1700.0, 4850.0], [1750.0, 4100.0], [1150.0, 4000.0]]),
     [np.array([[1300.0, 4600.0], [1500.0, 4600.0], [1500.0, 4350.0], [1300.0, 4350.0]])]),
    np.array([[1900.0, 3900.0], [2500.0, 3950.0], [2400.0, 3400.0]]),
]


def raster_values(shape=GRID_SHAPE, seed=5):
    """A float32 raster with zeros, NaN, an infinity and a few repeated values."""
    rng = np.random.default_rng(seed)
    a = np.zeros(shape, np.float32)
    pick = rng.random(shape)
    a[pick < 0.03] = 1.0
    a[(pick >= 0.03) & (pick < 0.05)] = 7.0
    a[(pick >= 0.05) & (pick < 0.06)] = -2.5
    a[(pick >= 0.06) & (pick < 0.08)] = np.nan
    a[3, 4] = np.inf
    return a
