"""Plain high-precision restatement of the two grid passes behind Deramp (csrc/biascorr.hip): the least-squares moments in
``np.longdouble`` with the magnitudes a bound needs, the derived bound itself, and the polynomial apply as NumPy forms it.  No GPU, no
import of the package under test.  Used by tests/test_deramp_routes_gpu.py and checked by tests/test_biascorr_host.py.

THE BOUND of a moment (``moments_bound``), in units of EPS = 2^-52, for M[a, b] = sum u^a v^b (weight w = 1) and
R[i, j] = sum dh u^i v^j (weight w = |dh|; dh is exact: both sides form it in the raster dtype and widen it).

  1. The coordinate.  The device forms u = c * ax + bx with ax = fl(1 / half) and bx = -1 exactly (or ax = 1, bx = -0 for a half-width
     of 0).  ax is off by 1/2 unit relative, which c * ax (at most 2) turns into 1 unit absolute; the product is rounded at a
     magnitude of at most 2 (1 unit), the sum at a magnitude of at most 1 (1/2 unit): |u^ - u| <= 5/2.  v likewise.
  2. A power.  p_1 = 1 * u^ is exact, p_e = fl(p_(e-1) * u^) adds 1/2 unit relative per step.  With |u| <= 1,
     |u^^e - u^e| <= e |u|^(e-1) 5/2 <= 5/2 e absolute, and the e - 1 roundings add at most (e - 1) / 2 of |u^e| <= 1:
     |p_e - u^e| <= 3 e, absolute -- not relative to u^e, which may be as small as it likes.
  3. A term.  w u^a v^b is off by w (3 a |v^b| + 3 b |u^a|) <= 3 (a + b) w from the two powers, and by 1/2 unit of itself for each
     of its products (one for M, two for R: dh * p first): at most (3 (a + b) + 1) w.  On the rows route the power of v multiplies the
     sum of a row, not each term; the same figure bounds it, the map being linear and |row sum| <= sum of the row's w |u^a|.
     Summed over the pixels: (3 (a + b) + 1) * sum w, where sum w is the count for M and sum |dh| for R.
  4. The additions.  Every term passes through at most L additions on its way to the total, each of which rounds a partial sum of
     magnitude at most mag = sum |term|: L / 2 units of mag, doubled for the second-order terms (as tests/test_cpd_gpu.py does):
     L * mag.  L counts the route (``additions_rows`` / ``additions_list``):
       rows: the pixels a lane adds in a row (ceil(W / 256), or 4 ceil(W / 1024) four-wide), 6 shuffle steps, 3 additions over the
             four waves, the product with the power of v (counted as one), the rows of a workgroup (ceil(H / nblocks)),
             ceil(nblocks / 256) partials per reduce lane, 8 tree steps;
       list: 256 per tile (the padding included), tiles per workgroup (together ``per``), then the same reduce.

  bound[a, b] = EPS * ((3 (a + b) + 1) * sum w + L * mag[a, b])

The oracle's own error -- pairwise longdouble sums, 2^-64 per operation -- is three orders of magnitude below EPS and is not counted."""
import math
from typing import NamedTuple

import numpy as np

EPS = 2.0 ** -52
LD = np.longdouble
MAX_ORDER = 5
LONGDOUBLE_REASON = ("np.longdouble has fewer than 63 mantissa bits here: the moments oracle would be no more precise than the "
                     "float64 sums it is meant to judge")


def require_longdouble() -> None:
    """Skips the calling test where np.longdouble is not the 80-bit extended format (or wider)."""
    if np.finfo(np.longdouble).nmant < 63:
        import pytest

        pytest.skip(LONGDOUBLE_REASON)
    assert np.finfo(np.longdouble).nmant >= 63


class Moments(NamedTuple):
    M: np.ndarray      # (2 order + 1)^2, longdouble
    R: np.ndarray      # (order + 1)^2, longdouble
    count: int
    magM: np.ndarray   # sums of |term|
    magR: np.ndarray


def _norm(n_global: int):
    """(centre, half-width) of an axis of n_global pixels; a half-width of 0 counts as 1."""
    half = LD(n_global - 1) / LD(2)
    return half, (half if half > 0 else LD(1))


def valid_mask(ref, tba, inlier=None) -> np.ndarray:
    """inlier & finite(ref) & finite(tba): the inputs are tested, never their difference."""
    valid = np.isfinite(ref) & np.isfinite(tba)
    if inlier is not None:
        valid &= np.asarray(inlier) != 0
    return valid


def moments(ref, tba, inlier, order, row_offset=0, H_global=None, ranks=None) -> Moments:
    """M[a, b] = sum u^a v^b (a, b <= 2 order) and R[i, j] = sum dh u^i v^j (i, j <= order) over the valid pixels -- with ``ranks``
    over ``flatnonzero(valid)[unique ranks]`` -- in longdouble, with u = (col - (W - 1) / 2) / halfW and
    v = (row_offset + row - (H_global - 1) / 2) / halfH.  dh = ref - tba is formed in the raster dtype and then widened; a pair of
    finite values whose difference overflows is a valid pixel with an infinite dh, as on the device."""
    require_longdouble()
    ref, tba = np.asarray(ref), np.asarray(tba)
    assert ref.shape == tba.shape and ref.ndim == 2 and ref.dtype == tba.dtype and ref.dtype in (np.float32, np.float64)
    H, W = ref.shape
    H_global = H if H_global is None else int(H_global)
    assert 0 <= row_offset and row_offset + H <= H_global
    flat = np.flatnonzero(valid_mask(ref, tba, inlier))
    if ranks is not None:
        flat = flat[np.unique(np.asarray(ranks, dtype=np.int64))]
    with np.errstate(over="ignore", invalid="ignore"):
        dh = (ref.ravel()[flat] - tba.ravel()[flat]).astype(LD)   # (the raster dtype's difference, then widened)
    row, col = np.divmod(flat, W)
    cx, sx = _norm(W)
    cy, sy = _norm(H_global)
    u = (col.astype(LD) - cx) / sx
    v = ((row + int(row_offset)).astype(LD) - cy) / sy
    NA, NR = 2 * order + 1, order + 1
    U, V = [np.ones(flat.size, dtype=LD)], [np.ones(flat.size, dtype=LD)]
    for _ in range(NA - 1):
        U.append(U[-1] * u)
        V.append(V[-1] * v)
    M, magM = np.zeros((NA, NA), dtype=LD), np.zeros((NA, NA), dtype=LD)
    R, magR = np.zeros((NR, NR), dtype=LD), np.zeros((NR, NR), dtype=LD)
    with np.errstate(over="ignore", invalid="ignore"):
        for a in range(NA):
            for b in range(NA):
                t = U[a] * V[b]
                M[a, b], magM[a, b] = np.sum(t), np.sum(np.abs(t))   # (pairwise sums over a contiguous vector)
                if a < NR and b < NR:
                    t = dh * t
                    R[a, b], magR[a, b] = np.sum(t), np.sum(np.abs(t))
    return Moments(M, R, int(flat.size), magM, magR)


def sub(want: Moments, order: int) -> Moments:
    """The moments of a lower order are the leading blocks of a higher order's."""
    NA, NR = 2 * order + 1, order + 1
    return Moments(want.M[:NA, :NA], want.R[:NR, :NR], want.count, want.magM[:NA, :NA], want.magR[:NR, :NR])


def rows_grid(H: int, num_cu: int) -> int:
    """Workgroups of the rows route: min(8 CUs, rows), at least one."""
    return max(1, min(8 * num_cu, H))


def additions_rows(H: int, W: int, vec: bool, num_cu: int) -> int:
    nb = rows_grid(H, num_cu)
    lane = 4 * math.ceil(W / 1024) if vec else math.ceil(W / 256)
    return lane + 6 + 3 + 1 + math.ceil(H / nb) + math.ceil(nb / 256) + 8


def list_grid(k: int, num_cu: int):
    """(pixels per workgroup, workgroups) of the list route, as the launch computes them."""
    nb = 4 * num_cu
    per = max(256, 256 * math.ceil(math.ceil(k / nb) / 256))
    return per, max(1, math.ceil(k / per))


def additions_list(k: int, num_cu: int) -> int:
    per, nb = list_grid(k, num_cu)
    return per + math.ceil(nb / 256) + 8


def moments_bound(want: Moments, additions: int):
    """(bound of M, bound of R) as float64 arrays: the module docstring's derivation.  sum w is magM[0, 0] (the count) for M and
    magR[0, 0] (sum |dh|) for R."""
    out = []
    for mag in (want.magM, want.magR):
        n = mag.shape[0]
        powers = np.add.outer(np.arange(n), np.arange(n)).astype(np.float64)
        out.append(EPS * ((3.0 * powers + 1.0) * float(mag[0, 0]) + float(additions) * mag.astype(np.float64)))
    return out[0], out[1]


def count_bound(n: int, additions: int) -> float:
    """The bound of M[0, 0] over n pixels: below 0.5 means the device's count moment is the integer itself."""
    return EPS * (1.0 + additions) * n


def moments_shapes(num_cu: int):
    """(H, W, four-wide route when aligned) of every rows-route case of tests/test_deramp_routes_gpu.py."""
    tall = 8 * num_cu + 37
    return [(37, 61, False), (40, 64, True), (5, 259, False), (3, 515, False), (6, 1028, True), (tall, 8, True), (tall, 7, False),
            (1, 64, True), (64, 1, False), (1, 1, False)]


LIST_SMALL_K = (1, 255, 256, 257, 1000)


def list_large_case(num_cu: int):
    """(side, k) of the large list-route case: k > 1024 CUs, so that a workgroup walks more than one 256-pixel tile; a 520 x 520
    raster where that fits (up to 259 CUs), the next multiple of 4 that holds k valid pixels otherwise."""
    k = 1024 * num_cu + 1000
    side = max(520, 4 * math.ceil(math.sqrt((k + 1000) / 0.99) / 4))
    return side, k


def make_pair(H: int, W: int, dtype, seed: int, nan_frac: float = 0.03, masked: bool = False, outliers: float = 0.1):
    """(ref, tba, inlier or None): elevations around 1000 m, dh a low-order surface of a few metres plus noise, ``nan_frac`` of ref and of
    tba NaN, ``masked``: about a tenth of the pixels excluded.  A share ``outliers`` of tba is scaled to a third: there ref and tba lie
    in different binades, so their float32 difference is a rounded one (between neighbours of 1000 m it is exact, and a kernel that
    subtracted in float64 would go unnoticed).  Pixel (0, 0) stays valid, so that a 1 x 1 raster has a point."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    un, vn = xx / max(W - 1, 1), yy / max(H - 1, 1)
    ref = 1000.0 + 50.0 * rng.normal(size=(H, W))
    dh = 1.5 - 2.0 * un + 3.0 * vn + 4.0 * un * vn - 2.5 * un ** 2 + 1.5 * vn ** 3 + 0.1 * rng.normal(size=(H, W))
    tba = ref - dh
    tba[rng.random((H, W)) < outliers] *= 0.37
    ref[rng.random((H, W)) < nan_frac] = np.nan
    tba[rng.random((H, W)) < nan_frac] = np.nan
    ref, tba = ref.astype(dtype), tba.astype(dtype)
    inlier = None
    if masked:
        inlier = rng.random((H, W)) >= 0.1
        inlier[0, 0] = True
    ref[0, 0], tba[0, 0] = 1003.25, 1001.5
    return ref, tba, inlier


def apply(elev, params, row_offset=0):
    """``elev + polyval2d(xx, yy, c)`` in float64, cast to the dtype of elev: NumPy's own evaluation, the bits the device must give."""
    elev = np.asarray(elev)
    params = np.asarray(params, dtype=np.float64).ravel()
    K = int(round(math.sqrt(params.size)))
    assert K * K == params.size
    yy, xx = np.meshgrid(np.arange(elev.shape[0]) + int(row_offset), np.arange(elev.shape[1]), indexing="ij")
    with np.errstate(invalid="ignore", over="ignore"):
        return (elev.astype(np.float64) + np.polynomial.polynomial.polyval2d(xx, yy, params.reshape(K, K))).astype(elev.dtype)
