"""Inputs and measured figures of the block-wise coregistration tests (shared by the host and the GPU file)."""
import numpy as np

RES = 10.0

# Largest deviation of a whole batched fit's final offsets from tests/blockwise_oracle.py::fit_tiles over cases A and B, both dtypes, in
# PIXELS for the horizontal offsets (the unit of Nuth-Kaab's stopping threshold, 1e-3 pixel) and in metres for the vertical one.  The
# batched route seeds every tile's 72-point curve_fit with float64 moments of y, the oracle with NumPy's nanmean / nanstd in the raster
# dtype: on the host float64 rasters coincide (0.0), float32 ones start the optimiser a few 1e-8 apart, it stops up to 7e-5 pixel away,
# and the vertical offset -- a median of float32 differences of elevations near 800 m -- moves by one of their steps, 2^-14 m.  "cpu":
# the product's host code over blockwise_oracle.OraclePlan (float64 moments like the device); "mi355x": over the device plan -- float32
# as on the host to the digit, float64 differs through the last bit of the device's arctangent (the aspect decides the bins: 1.05e-4
# pixel on case B; the loop route on the device differs from the batched one by as much, 9.3e-5, for the same reason: its NKPlan's own
# moments).  The bar of the tests is 4 x the larger: 4.2e-4 pixel, below the method's own stopping threshold of 1e-3.
MEASURED = {"cpu": {"horizontal_px": 7.382e-5, "vertical": 6.104e-5}, "mi355x": {"horizontal_px": 1.051e-4, "vertical": 6.104e-5}}


def _bar(key: str) -> float:
    return 4 * max(v[key] for v in MEASURED.values())


BAR_PX, BAR_Z = _bar("horizontal_px"), _bar("vertical")

# the shift fields of the warp tests: (coeff_x, coeff_y, coeff_z) of shift = a x + b y + d; gradients up to 3e-4, offsets up to 25 m
WARP_SHAPES = ((61, 83), (96, 128))
WARP_FIELDS = (
    ((3e-4, -1e-4, 12.0), (-2e-4, 2.5e-4, -25.0), (1e-4, -3e-4, 1.5)),
    ((-1.5e-4, 3e-4, -18.5), (1e-4, -3e-4, 7.25), (0.0, 0.0, 0.0)),
    ((0.0, 0.0, 20.0), (0.0, 0.0, -10.0), (-2e-4, 1e-4, -0.75)),
)


def surface(x, y):
    return 800.0 + 120.0 * np.sin(x / 90.0) * np.cos(y / 70.0) + 40.0 * np.sin((x + y) / 50.0)


def transform6(H: int):
    """North-up grid of RES metres with its lower left corner at the origin: (a, b, c, d, e, f)."""
    return (RES, 0.0, 0.0, 0.0, -RES, RES * H)


def grid_xy(H: int, W: int):
    rows, cols = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    t = transform6(H)
    return t[0] * (cols + 0.5) + t[2], t[4] * (rows + 0.5) + t[5]


def fit_case(H: int, W: int, dtype):
    """(ref, tba): ref is the surface, tba the surface at positions moved by a shift field affine in (x, y), plus 1.5 m, plus noise;
    2 % NaN in each raster."""
    rng = np.random.default_rng(7)
    x, y = grid_xy(H, W)
    xm, ym = x.mean(), y.mean()
    sx = 4.0 + 6e-3 * (x - xm) - 2e-3 * (y - ym)
    sy = -3.0 + 1e-3 * (x - xm) + 5e-3 * (y - ym)
    ref = surface(x, y)
    tba = surface(x + sx, y + sy) + 1.5 + rng.normal(scale=0.05, size=(H, W))
    ref[rng.random((H, W)) < 0.02] = np.nan
    tba[rng.random((H, W)) < 0.02] = np.nan
    return ref.astype(dtype), tba.astype(dtype)


CASES = {"A": (70, 100, 32), "B": (150, 200, 64)}   # H, W, block_size_fit


def warp_dem(H: int, W: int, dtype, nans: bool):
    x, y = grid_xy(H, W)
    dem = surface(x, y)
    if nans:
        rng = np.random.default_rng(11)
        dem[rng.random((H, W)) < 0.02] = np.nan
        dem[H // 3: H // 3 + 3, W // 2: W // 2 + 4] = np.nan
    return dem.astype(dtype)
