"""CPU oracle for block-wise coregistration -- TEST INFRASTRUCTURE, NOT PRODUCT CODE (NumPy / SciPy, own code).

* ``tiling_grid``: the tiles of a raster, restated on its own (geoutils' ``compute_tiling`` is absent: unpinned).
* ``fit_tiles``: ``nuthkaab_oracle.nuth_kaab`` on the slices of every tile, as ``BlockwiseCoreg._coreg_wrapper`` runs the step on a tile
  cropped out of the rasters (blockwise.py:118-154): a tile whose reference or to-be-aligned part is entirely invalid, or whose fit
  raises ``ValueError`` / ``TypeError``, has NaN shifts.
* ``step_tiles``: one ``nuthkaab_oracle.iteration_step`` per tile, each at its own offsets.
* ``OraclePlan``: ``fit_tiles``' ingredients behind the interface of ``xdem_amd.blockwise.BWPlan`` (host tests put it in its place).
* ``apply``: the inverse-map warp of ``xdemhip_bw_apply`` in float64, every operation on its own.
* ``apply_forward_griddata``: upstream's formulation (blockwise.py:291-349): every pixel a point, moved by the shift field, gridded back
  by linear interpolation on a Delaunay triangulation (``scipy.interpolate.griddata``, which is what geoutils' ``_grid_pointcloud`` calls).
"""
from __future__ import annotations

import math

import numpy as np

import nuthkaab_oracle
import rigid_oracle


def tiling_grid(shape, block_size: int) -> np.ndarray:
    def axis(n, b):
        k = -(-n // b)
        r = n % b
        if r != 0 and 2 * r <= b:
            k = max(k - 1, 1)
        return [(i * b, n if i == k - 1 else (i + 1) * b) for i in range(k)]

    rows, cols = axis(int(shape[0]), int(block_size)), axis(int(shape[1]), int(block_size))
    return np.array([[(r0, r1, c0, c1) for (c0, c1) in cols] for (r0, r1) in rows], dtype=np.int64)


def tile_valid(ref, tba, inlier):
    st, asp = nuthkaab_oracle.aux_vars(ref)
    inl = np.ones(ref.shape, dtype=bool) if inlier is None else inlier.astype(bool)
    return st, asp, inl & np.isfinite(ref) & np.isfinite(tba) & np.isfinite(st) & np.isfinite(asp)


def fit_tiles(ref, tba, inlier, block_size: int, res, nan_rule=None, tolerance: float = 0.001, max_iterations: int = 10, n_bins: int = 72,
              vertical_shift: bool = True):
    """{"shift_x", "shift_y", "shift_z": float64 arrays over the tiles (row-major), "n_iterations": int array (0: no fit)}."""
    tiles = tiling_grid(ref.shape, block_size).reshape(-1, 4)
    n = tiles.shape[0]
    out = {k: np.full(n, np.nan) for k in ("shift_x", "shift_y", "shift_z")}
    out["n_iterations"] = np.zeros(n, dtype=np.int64)
    for t, (r0, r1, c0, c1) in enumerate(tiles):
        r, b = ref[r0:r1, c0:c1], tba[r0:r1, c0:c1]
        if not np.isfinite(r).any() or not np.isfinite(b).any():
            continue
        m = None if inlier is None else inlier[r0:r1, c0:c1].astype(bool)
        try:
            (east, north, vert), _, trace = nuthkaab_oracle.nuth_kaab(r, b, m, res, tolerance, max_iterations, n_bins, nan_rule)
        except (ValueError, TypeError):
            continue
        out["shift_x"][t], out["shift_y"][t], out["shift_z"][t] = -east, -north, vert * vertical_shift
        out["n_iterations"][t] = len(trace)
    return out


def step_tiles(ref, tba, inlier, tiles, active, shift_x, shift_y, res, n_bins: int = 72, nan_rule=None, aspects=None):
    """Per active tile the details of ``nuthkaab_oracle.iteration_step`` at (shift_x[t], shift_y[t]) plus "y" (the values binned), or
    ``None`` for a tile with no finite dh left; inactive tiles: ``None`` too.  ``aspects``: per tile an aspect plane to hand
    ``iteration_step`` instead of the oracle's own (float64: the device's arctangent may differ from libm's in the last bit)."""
    out = []
    for t, (r0, r1, c0, c1) in enumerate(np.asarray(tiles).reshape(-1, 4)):
        if not active[t]:
            out.append(None)
            continue
        r, b = ref[r0:r1, c0:c1], tba[r0:r1, c0:c1]
        st, asp, valid = tile_valid(r, b, None if inlier is None else inlier[r0:r1, c0:c1])
        if aspects is not None:
            asp = aspects[t]
        if not valid.any():
            out.append(None)
            continue
        try:
            _, _, det = nuthkaab_oracle.iteration_step((shift_x[t], shift_y[t], 0.0), r, b, valid, st, asp, res, n_bins, nan_rule)
        except ValueError:
            out.append(None)
            continue
        dh = nuthkaab_oracle.shifted_dh(r, b, shift_x[t], shift_y[t], res, nan_rule)[valid]
        dh = dh - np.nanmedian(dh)
        ok = np.isfinite(dh)
        with np.errstate(divide="ignore", invalid="ignore"):
            det["y"] = (dh[ok] / st[valid][ok]).astype(np.float64)
        out.append(det)
    return out


class OraclePlan:
    """``xdem_amd.blockwise.BWPlan`` answered by ``step_tiles`` (host arrays only)."""

    nan_rule = None

    def __init__(self, ref, tba, inlier_mask, tiles, ctx=None):
        self.ref, self.tba = np.ascontiguousarray(ref), np.ascontiguousarray(tba)
        self.inlier = None if inlier_mask is None else np.asarray(inlier_mask).astype(bool)
        self.dtype = self.ref.dtype
        self.tiles = np.asarray(tiles, dtype=np.int64).reshape(-1, 4)
        self.n_tiles = self.tiles.shape[0]
        self.n_valid = np.array([int(tile_valid(self.ref[r0:r1, c0:c1], self.tba[r0:r1, c0:c1],
                                                None if self.inlier is None else self.inlier[r0:r1, c0:c1])[2].sum())
                                 for (r0, r1, c0, c1) in self.tiles], dtype=np.int64)

    def new_results(self, n_bins):
        n = self.n_tiles
        return {"vshift": np.full(n, np.nan), "n_valid": np.zeros(n, dtype=np.int64), "y_mean": np.full(n, np.nan), "y_std": np.full(n, np.nan),
                "edges": np.full((n, n_bins + 1), np.nan), "counts": np.zeros((n, n_bins), dtype=np.int64), "medians": np.full((n, n_bins), np.nan)}

    def step(self, active, shift_x, shift_y, res, n_bins=72, out=None):
        out = out if out is not None else self.new_results(n_bins)
        dets = step_tiles(self.ref, self.tba, self.inlier, self.tiles, active, shift_x, shift_y, res, n_bins, self.nan_rule)
        for t, det in enumerate(dets):
            if not active[t]:
                continue
            if det is None:
                out["n_valid"][t] = 0
                continue
            out["vshift"][t], out["n_valid"][t] = det["vshift"], det["n_valid"]
            out["y_mean"][t], out["y_std"][t] = det["y"].mean(), det["y"].std()   # (float64 moments, as the device plan forms them)
            out["edges"][t], out["counts"][t], out["medians"][t] = det["edges"].astype(np.float64), det["counts"], det["medians"]
        return out

    def close(self):
        pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


def inverse_field(coeff_x, coeff_y):
    """(i00, i01, i10, i11) of (I + A)^-1, A = [[a_x, b_x], [a_y, b_y]]; ValueError if singular."""
    m00, m01, m10, m11 = 1.0 + float(coeff_x[0]), float(coeff_x[1]), float(coeff_y[0]), 1.0 + float(coeff_y[1])
    det = m00 * m11 - m01 * m10
    if det == 0.0 or not math.isfinite(det):
        raise ValueError("singular shift field")
    return m11 / det, -m01 / det, -m10 / det, m00 / det


def apply(dem: np.ndarray, t6, coeff_x, coeff_y, coeff_z, nan_rule: int) -> np.ndarray:
    """out(p') = dtype(bilinear(dem)(row(p), col(p)) + s_z(p)), p = (I + A)^-1 (p' - d), p' the pixel centres under ``t6``."""
    H, W = dem.shape
    i00, i01, i10, i11 = inverse_field(coeff_x, coeff_y)
    rows, cols = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    a, _, c, _, e, f = (float(v) for v in t6)
    xo = a * (cols + 0.5) + c
    yo = e * (rows + 0.5) + f
    ux, uy = xo - float(coeff_x[2]), yo - float(coeff_y[2])
    px = i00 * ux + i01 * uy
    py = i10 * ux + i11 * uy
    sz = (float(coeff_z[0]) * px + float(coeff_z[1]) * py) + float(coeff_z[2])
    col = (px - c) / a - 0.5
    row = (py - f) / e - 0.5
    v = rigid_oracle.point_taps(dem, row, col, nan_rule)
    with np.errstate(invalid="ignore"):
        return (v.astype(np.float64) + sz).astype(dem.dtype)


def apply_forward_griddata(dem: np.ndarray, t6, coeff_x, coeff_y, coeff_z) -> np.ndarray:
    """Upstream's arithmetic: the finite pixels as points, moved, ``griddata(method="linear")`` at the pixel centres (float64)."""
    from scipy.interpolate import griddata

    H, W = dem.shape
    rows, cols = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    x, y = rigid_oracle.pixel_xy(t6, rows, cols)
    z = dem.astype(np.float64)
    ok = np.isfinite(z)
    xs, ys, zs = x[ok], y[ok], z[ok]
    xn = xs + (coeff_x[0] * xs + coeff_x[1] * ys + coeff_x[2])
    yn = ys + (coeff_y[0] * xs + coeff_y[1] * ys + coeff_y[2])
    zn = zs + (coeff_z[0] * xs + coeff_z[1] * ys + coeff_z[2])
    return griddata((xn, yn), zn, (x, y), method="linear")


def twist_bound(dem: np.ndarray, t6, coeff_x, coeff_y) -> np.ndarray:
    """|a00 - a01 - a10 + a11| / 4 of the cell each output pixel's pre-image falls in (NaN where it falls in none): how far bilinear
    interpolation can lie from a linear interpolant on either diagonal of that cell."""
    H, W = dem.shape
    i00, i01, i10, i11 = inverse_field(coeff_x, coeff_y)
    rows, cols = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    x, y = rigid_oracle.pixel_xy(t6, rows, cols)
    ux, uy = x - coeff_x[2], y - coeff_y[2]
    row, col = rigid_oracle.xy_to_pixel(t6, i00 * ux + i01 * uy, i10 * ux + i11 * uy)
    r0, c0 = np.floor(row).astype(np.int64), np.floor(col).astype(np.int64)
    inside = (r0 >= 0) & (r0 + 1 < H) & (c0 >= 0) & (c0 + 1 < W)
    r0, c0 = np.clip(r0, 0, H - 2), np.clip(c0, 0, W - 2)
    z = dem.astype(np.float64)
    tw = np.abs(z[r0, c0] - z[r0, c0 + 1] - z[r0 + 1, c0] + z[r0 + 1, c0 + 1]) / 4
    return np.where(inside, tw, np.nan)
