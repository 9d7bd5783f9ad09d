"""The distance-transform rule of DESIGN.md 5p restated in NumPy: what ``xdemhip_edt`` returns bit for bit.

    cost(y, x; ty, tx) = fl( fl(fl((y - ty) sy)^2) + fl(fl((x - tx) sx)^2) )          float64, one rounding per fl
    d(y, x) = sqrt(min over targets of cost)       no target: +inf, indices -1
    winner among equal costs: the smaller |x - tx|, then the smaller tx, then within that column the nearer row, the upper on a tie

Two forms: ``brute`` takes the minimum over all targets (tiny shapes), ``separable`` the nearest target of every column and then the
minimum of the W x W cost matrix of every row (it carries the tie rule as the device does).  Then the small restatements: the target
plane of a raster, the inner boundary of a mask, the compositions of ``proximity`` and of ``create_mask(buffer=)``, and an engine
that stands in for the device one in host tests."""
import contextlib

import numpy as np

BIG = np.iinfo(np.int64).max


def axis_cost(n: int, s: float) -> np.ndarray:
    """fl(fl(k s)^2) for k = 0 .. n - 1."""
    a = np.arange(n, dtype=np.float64) * np.float64(s)
    return a * a


def _pair(sampling):
    if sampling is None:
        return 1.0, 1.0
    if np.ndim(sampling) == 0:
        return float(sampling), float(sampling)
    return float(sampling[0]), float(sampling[1])


def brute(targets, sampling=None):
    """(float64 distances, int32 [2, H, W] indices, number of targets) by the minimum over ALL targets."""
    t = np.asarray(targets) != 0
    H, W = t.shape
    sy, sx = _pair(sampling)
    cy, cx = axis_cost(H, sy), axis_cost(W, sx)
    ty, tx = np.nonzero(t)
    dist = np.full((H, W), np.inf)
    idx = np.full((2, H, W), -1, np.int32)
    if ty.size == 0:
        return dist, idx, 0
    yy, xx = np.mgrid[0:H, 0:W]
    yy, xx = yy.reshape(-1, 1), xx.reshape(-1, 1)
    dy, dx = np.abs(yy - ty[None, :]), np.abs(xx - tx[None, :])
    cost = cy[dy] + cx[dx]
    tie = cost == cost.min(axis=1, keepdims=True)
    for key in (dx, np.broadcast_to(tx[None, :], dx.shape), dy, np.broadcast_to(ty[None, :], dx.shape)):
        k = np.where(tie, key, BIG)
        tie &= k == k.min(axis=1, keepdims=True)
    win = tie.argmax(axis=1)
    dist = np.sqrt(cost[np.arange(cost.shape[0]), win]).reshape(H, W)
    idx[0], idx[1] = ty[win].reshape(H, W), tx[win].reshape(H, W)
    return dist, idx, int(ty.size)


def column_offsets(targets):
    """(signed row offset to the nearest target of the pixel's column -- the upper one on a tie --, True where the column has one)."""
    t = np.asarray(targets) != 0
    H, W = t.shape
    rows = np.arange(H, dtype=np.int64)[:, None]
    up = np.maximum.accumulate(np.where(t, rows, -1), axis=0)
    down = np.minimum.accumulate(np.where(t, rows, BIG)[::-1], axis=0)[::-1]
    has_up, has_down = up >= 0, down < BIG
    take_up = has_up & (~has_down | (rows - up <= down - rows))
    off = np.where(take_up, up - rows, np.where(has_down, down - rows, 0))
    return off, has_up | has_down


def separable(targets, sampling=None, chunk_elems: int = 1 << 22):
    """The same three results from the nearest target per column and the W x W cost matrix of every row."""
    t = np.asarray(targets) != 0
    H, W = t.shape
    sy, sx = _pair(sampling)
    cy, cx = axis_cost(H, sy), axis_cost(W, sx)
    off, has = column_offsets(t)
    colcost = np.where(has, cy[np.abs(off)], np.inf)                  # [H, tx]
    K = np.abs(np.arange(W)[:, None] - np.arange(W)[None, :])         # [x, tx]
    cxm = cx[K]
    dist = np.empty((H, W))
    idx = np.full((2, H, W), -1, np.int32)
    step = max(1, chunk_elems // (W * W))
    for y0 in range(0, H, step):
        y1 = min(H, y0 + step)
        cost = colcost[y0:y1, None, :] + cxm[None, :, :]              # [y, x, tx]
        tie = (cost == cost.min(axis=2, keepdims=True)) & has[y0:y1, None, :]
        k = np.where(tie, K[None], BIG)
        tie &= k == k.min(axis=2, keepdims=True)
        win = tie.argmax(axis=2)                                      # (the first True: the smallest tx)
        found = tie.any(axis=2)
        c = np.take_along_axis(cost, win[:, :, None], axis=2)[:, :, 0]
        dist[y0:y1] = np.where(found, np.sqrt(c), np.inf)
        rows = np.arange(y0, y1)[:, None]
        idx[0, y0:y1] = np.where(found, rows + off[rows, win], -1)
        idx[1, y0:y1] = np.where(found, win, -1)
    return dist, idx, int(t.sum())


def reproduces(targets, sampling, dist, idx) -> bool:
    """Every index points at a target and gives back its own distance under the rule's expression."""
    t = np.asarray(targets) != 0
    H, W = t.shape
    sy, sx = _pair(sampling)
    yy, xx = np.mgrid[0:H, 0:W]
    iy, ix = np.asarray(idx[0], dtype=np.int64), np.asarray(idx[1], dtype=np.int64)
    if not (np.all((iy >= 0) & (iy < H) & (ix >= 0) & (ix < W)) and np.all(t[iy, ix])):
        return False
    a, b = (yy - iy) * np.float64(sy), (xx - ix) * np.float64(sx)
    return np.array_equal(np.sqrt(a * a + b * b), np.asarray(dist, dtype=np.float64))


def kept(dist, keep, polarity):
    """``keep`` of xdemhip_edt: the distance is 0 wherever bool(keep) != bool(polarity)."""
    return np.where((np.asarray(keep) != 0) == bool(polarity), dist, dist.dtype.type(0))


def target_plane(raster, values=None):
    a = np.asarray(raster)
    v = a.astype(np.float64)
    if values is None:
        return (np.isfinite(v) & (v != 0)).astype(np.uint8)
    out = np.zeros(a.shape, bool)
    for t in np.atleast_1d(np.asarray(values, dtype=np.float64)):
        out |= v == t
    return out.astype(np.uint8)


def inner_boundary(mask):
    m = np.asarray(mask) != 0
    out = np.zeros_like(m)
    out[1:] |= m[1:] & ~m[:-1]
    out[:-1] |= m[:-1] & ~m[1:]
    out[:, 1:] |= m[:, 1:] & ~m[:, :-1]
    out[:, :-1] |= m[:, :-1] & ~m[:, 1:]
    return out.astype(np.uint8)


def edt_zeros(a, sampling=None):
    """distance_transform_edt's meaning: distances to the nearest zero pixel (NaN counts as non-zero)."""
    return separable(target_plane(a, [0.0]), sampling)


def proximity(mask, sampling, geometry_type="boundary", in_or_out="both", dtype=np.float32, edt=None):
    """``proximity`` with a vector, composed on its burnt mask.  ``edt(targets, sampling) -> float64 distances`` (default: the
    separable oracle; the host tests pass SciPy's)."""
    edt = edt or (lambda t, s: separable(t, s)[0])
    m = np.asarray(mask) != 0
    targets = m if geometry_type == "polygon" else inner_boundary(m) != 0
    d = edt(targets, sampling).astype(dtype)
    if in_or_out == "in":
        d = np.where(m, d, dtype(0))
    elif in_or_out == "out":
        d = np.where(~m, d, dtype(0))
    return d


def buffered(mask, sampling, buffer, edt=None):
    edt = edt or (lambda t, s: separable(t, s)[0])
    m = np.asarray(mask) != 0
    if buffer == 0:
        return m
    if buffer > 0:
        return edt(m, sampling) <= buffer
    return edt(~m, sampling) > -buffer


class OracleEngine:
    """Stands in for ``xdem_amd.proximity.DeviceEngine`` (``proximity._ENGINE``) where no GPU is at hand: host arrays only."""

    on_device = False

    def edt(self, targets, sampling, dtype=np.float64, return_distances=True, return_indices=False, keep=None, keep_polarity=1, ctx=None):
        dist, idx, n = separable(np.asarray(targets), sampling)
        dist = dist.astype(dtype)
        if keep is not None:
            dist = kept(dist, keep, keep_polarity)
        return (dist if return_distances else None), (idx if return_indices else None), n

    def targets(self, raster, values=None, ctx=None):
        return target_plane(np.asarray(raster), values)

    def boundary(self, mask, ctx=None):
        return inner_boundary(mask)


@contextlib.contextmanager
def oracle_engine():
    """xdem_amd.proximity with its device engine replaced by the restatement above."""
    from xdem_amd import proximity

    saved = proximity._ENGINE
    proximity._ENGINE = OracleEngine()
    try:
        yield proximity
    finally:
        proximity._ENGINE = saved
