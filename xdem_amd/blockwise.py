"""Block-wise co-registration on MI355X -- host-side mirror of ``xdem.coreg.BlockwiseCoreg`` (xdem/coreg/blockwise.py).

``fit`` cuts the two rasters into tiles (``tiling_grid``), fits a copy of the step on every tile as a raster of its own and records the
tiles' shifts; ``apply`` fits a plane to each of the three shift fields with upstream's ``_ransac`` and warps the raster by them.

Two fit routes that agree (tests/test_blockwise_gpu.py):

* the **loop route** serves any affine step: ``step.copy().fit`` on the slices of each tile with the tile's own transform;
* the **batched route** serves ``NuthKaab`` in its default form (binned, exact medians, every valid pixel of a tile in the fit): one
  device plan over all tiles (``BWPlan``: csrc/blockwise.hip) runs one iteration of every tile that is still iterating per call -- a
  fixed number of launches and one copy back whatever the number of tiles -- and the 72-point ``curve_fit`` of every tile runs on the
  host, as upstream.  A tile stops on its own by ``_iterate``'s rule and is frozen afterwards.

``apply`` is ONE pass on the device (``xdemhip_bw_apply``): the shift field is affine in (x, y), so the forward map of upstream's point
cloud has a closed-form inverse and every output pixel samples the raster bilinearly at its pre-image.  Upstream grids the moved
points by linear interpolation on a Delaunay triangulation instead; the two differ by at most a quarter of the cell's twist.

Differences from upstream, stated: no raster I/O -- nothing is written to disk, ``mp_config`` is kept and not executed, neither of
``mp_config`` / ``parent_path`` is required, ``block_size_apply`` is kept and not used.  Arrays on one grid only (no clouds).
"""
from __future__ import annotations

import ctypes
import logging
import math
from typing import Any

import numpy as np

from . import _args, _lib
from ._args import is_tensor, nan_filled, raster_pair
from ._lib import _Plan

BATCHED_DEFAULT = True   # tests: False sends an eligible step down the loop route


def _axis_tiles(n: int, b: int) -> list[tuple[int, int]]:
    k = math.ceil(n / b)
    if 0 < n % b <= b / 2:   # a remainder of at most half a block joins the last tile
        k = max(k - 1, 1)
    return [(i * b, (i + 1) * b if i < k - 1 else n) for i in range(k)]


def tiling_grid(shape: tuple[int, int], block_size: int) -> np.ndarray:
    """The tiles of a raster of ``shape`` for ``block_size``: an int64 array ``(rows, cols, 4)`` of ``(row0, row1, col0, col1)``.  A
    restatement of geoutils' ``compute_tiling`` (absent here, **parity unpinned**): per axis ``ceil(n / b)`` tiles, one fewer where the
    remainder is at most half a block; tile i is ``[i b, (i + 1) b)`` and the last one ends at n."""
    block_size = int(block_size)
    if block_size < 1:
        raise ValueError("block size must be a positive integer")
    rows, cols = _axis_tiles(int(shape[0]), block_size), _axis_tiles(int(shape[1]), block_size)
    out = np.empty((len(rows), len(cols), 4), dtype=np.int64)
    for i, (r0, r1) in enumerate(rows):
        for j, (c0, c1) in enumerate(cols):
            out[i, j] = (r0, r1, c0, c1)
    return out


def _transform6(transform, resolution) -> tuple[float, ...]:
    """(a, b, c, d, e, f) of x = a col + b row + c, y = d col + e row + f from an affine ``transform`` (an object with ``.a`` .. ``.f`` or a
    6-tuple), or from ``resolution`` alone: a north-up grid with its upper left corner at the origin."""
    if transform is not None:
        t = tuple(float(getattr(transform, k)) for k in "abcdef") if hasattr(transform, "a") else tuple(float(v) for v in tuple(transform)[:6])
        if len(t) != 6:
            raise ValueError("transform must be an affine transform: an object with a .. f or six numbers")
        return t
    if resolution is None:
        raise ValueError("'transform' must be given if both DEMs are array-like.")   # (base.py:204; or pass resolution=)
    rx, ry = (float(resolution), float(resolution)) if np.isscalar(resolution) else (float(resolution[0]), float(resolution[1]))
    return (rx, 0.0, 0.0, 0.0, -ry, 0.0)


class BWPlan(_Plan):
    """Device-resident state of the Nuth-Kaab fits of all tiles of a tiling (``xdemhip_bw_plan``).  ``n_valid``: valid pixels per tile."""

    _DESTROY = "xdemhip_bw_destroy"

    def __init__(self, ref, tba, inlier_mask, tiles: np.ndarray, ctx: _lib.Context | None = None):
        self.ctx = ctx or _lib.default_context()
        self.handle = None
        self.ctx.adopt(self)
        p = raster_pair(ref, tba, inlier_mask)
        self.dtype, self.shape = p.dtype, p.shape
        self.tiles = np.ascontiguousarray(tiles, dtype=np.int64).reshape(-1, 4)
        self.n_tiles = int(self.tiles.shape[0])
        h = ctypes.c_void_p()
        nv = np.zeros(self.n_tiles, dtype=np.int64)
        self.ctx.check(self.ctx._L.xdemhip_bw_create(self.ctx.handle, p.ref, p.tba, p.inlier, p.code, p.shape[0], p.shape[1], self.n_tiles,
                                                     _args.i64p(self.tiles), p.memspace, ctypes.byref(h), _args.i64p(nv)))
        self.handle = h
        self.n_valid = nv

    def aux(self) -> list[tuple[np.ndarray, np.ndarray, np.ndarray]]:
        """Per tile (slope_tan, aspect, valid) copied back to the host (tests / debugging)."""
        sizes = (self.tiles[:, 1] - self.tiles[:, 0]) * (self.tiles[:, 3] - self.tiles[:, 2])
        total = int(sizes.sum())
        st, asp, valid = np.empty(total, dtype=self.dtype), np.empty(total, dtype=self.dtype), np.empty(total, dtype=np.uint8)
        self.ctx.check(self.ctx._L.xdemhip_bw_get_aux(self.handle, _args.ptr(st), _args.ptr(asp), _args.ptr(valid)))
        out, off = [], 0
        for (r0, r1, c0, c1), n in zip(self.tiles, sizes):
            shape = (int(r1 - r0), int(c1 - c0))
            out.append(tuple(a[off:off + n].reshape(shape) for a in (st, asp, valid.astype(bool))))
            off += int(n)
        return out

    def new_results(self, n_bins: int) -> dict[str, np.ndarray]:
        n = self.n_tiles
        return {"vshift": np.full(n, np.nan), "n_valid": np.zeros(n, dtype=np.int64), "y_mean": np.full(n, np.nan), "y_std": np.full(n, np.nan),
                "edges": np.full((n, n_bins + 1), np.nan), "counts": np.zeros((n, n_bins), dtype=np.int64), "medians": np.full((n, n_bins), np.nan)}

    def step(self, active, shift_x, shift_y, res: tuple[float, float], n_bins: int = 72, out: dict[str, np.ndarray] | None = None):
        """One iteration step of every tile with ``active[t]`` set, at its own ``(shift_x[t], shift_y[t])``: per tile what ``NKPlan.step``
        returns for the tile as a raster of its own, as arrays over the tiles.  ``out`` (from ``new_results`` or an earlier step)
        receives the results; the entries of inactive tiles are left as they are."""
        n_bins = int(n_bins)
        out = out if out is not None else self.new_results(n_bins)
        act = np.ascontiguousarray(active, dtype=np.uint8)
        sx, sy = np.ascontiguousarray(shift_x, dtype=np.float64), np.ascontiguousarray(shift_y, dtype=np.float64)
        if not (act.size == sx.size == sy.size == self.n_tiles) or out["edges"].shape != (self.n_tiles, n_bins + 1):
            raise ValueError("one entry per tile expected")
        dp, ip = _args.dp, _args.i64p
        self.ctx.check(self.ctx._L.xdemhip_bw_nk_step(self.handle, _args.ptr(act), dp(sx), dp(sy), float(res[0]), float(res[1]), n_bins,
                                                      dp(out["vshift"]), ip(out["n_valid"]), dp(out["y_mean"]), dp(out["y_std"]),
                                                      dp(out["edges"]), ip(out["counts"]), dp(out["medians"])))
        return out


def warp_affine_field(dem, transform6, coeff_x, coeff_y, coeff_z, ctx: _lib.Context | None = None):
    """``xdemhip_bw_apply``: the raster warped by the shift field ``s(x, y) = a x + b y + d`` per axis (module docstring).  ``dem``: a 2-D
    array (returns an array) or a contiguous float32 / float64 CUDA tensor (returns a tensor).  A singular ``I + A`` raises ValueError."""
    ctx = ctx or _lib.default_context()
    cx, cy, cz = (np.array([float(v) for v in c], dtype=np.float64) for c in (coeff_x, coeff_y, coeff_z))
    if (1.0 + cx[0]) * (1.0 + cy[1]) - cx[1] * cy[0] == 0.0:
        raise ValueError("The shift field is singular: I + [[a_x, b_x], [a_y, b_y]] has no inverse.")
    t6 = np.array(transform6, dtype=np.float64)
    device = is_tensor(dem)
    if device:
        import torch

        _args.device_float(dem, "a device input must be a contiguous 2D float32 / float64 CUDA tensor")
        _args.synchronize_torch(dem)
        out = torch.empty_like(dem)
    else:
        dem = _args.host_float(dem)
        if dem.ndim != 2:
            raise ValueError("the elevation array must be 2D")
        out = np.empty_like(dem)
    ctx.check(ctx._L.xdemhip_bw_apply(ctx.handle, _args.ptr(dem), _args.code(dem), dem.shape[0], dem.shape[1], _args.dp(t6), _args.dp(cx),
                                      _args.dp(cy), _args.dp(cz), _args.ptr(out), _args.space(dem)))
    if device:
        ctx.synchronize()
    return out


class BlockwiseCoreg:
    """A coregistration step run on the tiles of a subdivision of the raster; ``apply`` warps by planes fitted through the tiles' shifts
    (``xdem.coreg.BlockwiseCoreg``, blockwise.py:51-407; the module docstring lists the differences)."""

    def __init__(self, step, mp_config=None, block_size_fit: int = 500, block_size_apply: int = 500, parent_path: str = None) -> None:
        if (mp_config is not None) and (parent_path is not None):
            raise ValueError("Only one of the parameters 'mp_config' or 'parent_path' may be specified.")
        # (upstream requires one of the two for its output file; nothing is written here, so neither is accepted too)
        if isinstance(step, type):
            raise ValueError(
                "The 'step' argument must be an instantiated Coreg subclass. " "Hint: write e.g. ICP() instead of ICP"
            )
        if not step.is_affine:
            raise ValueError("The blockwise coregistration only supports affine coregistration methods.")
        if not step.meta["inputs"].get("affine", {}).get("only_translation", True):
            raise ValueError(
                "The provided coregistration method is configured to only estimate translation. "
                "Consider setting 'only_translation' to True to allow for more complex transformations."
            )
        from .coreg import NuthKaab

        self.procstep = step
        self.block_size_fit = block_size_fit
        self.block_size_apply = block_size_apply   # (kept; the warp is one pass over the raster)
        self.apply_z_correction = step.vertical_shift if isinstance(step, NuthKaab) else True
        self.mp_config = mp_config                 # (kept; nothing is executed through it)
        self.parent_path = parent_path
        self.meta: dict[str, Any] = {"inputs": {}, "outputs": {}}
        self.shape_tiling_grid = (0, 0, 0)
        self.fit_route: str | None = None          # "batched" or "loop" after a fit

    # ---- fit ------------------------------------------------------------------------------------------------------------------------
    def _batched_candidate(self) -> bool:
        """What of the batched route's conditions can be told from the step alone (the subsample needs the tiles' valid counts)."""
        from .coreg import NuthKaab, _bin_statistic_id

        step = self.procstep
        if not (BATCHED_DEFAULT and type(step) is NuthKaab):
            return False
        fb, aff, sub = step.meta["inputs"]["fitorbin"], step.meta["inputs"]["affine"], step.meta["inputs"]["random"]["subsample"]
        return (fb["fit_or_bin"] == "bin_and_fit" and _bin_statistic_id(fb["bin_statistic"]) == 0
                and isinstance(fb["bin_sizes"], (int, np.integer)) and 1 <= fb["bin_sizes"] <= 128 and "initial_shift" not in aff
                and (sub == 1 or (sub > 1 and float(sub) == int(sub))))

    def _fit_batched(self, ref, tba, inlier_mask, tiles, res):
        """The tiles' (shift_x, shift_y, shift_z), NaN where a tile has no fit; ``None`` if the subsample would leave pixels of a tile out
        (the loop route then draws them)."""
        from .coreg import _bin_fit_from_step

        step = self.procstep
        it, fb = step.meta["inputs"]["iterative"], step.meta["inputs"]["fitorbin"]
        sub = step.meta["inputs"]["random"]["subsample"]
        n_bins = int(fb["bin_sizes"])
        with BWPlan(ref, tba, inlier_mask, tiles) as plan:
            n = plan.n_tiles
            if sub != 1 and int(sub) < int(plan.n_valid.max(initial=0)):
                return None
            ox, oy, vs = np.zeros(n), np.zeros(n), np.zeros(n)
            failed = plan.n_valid == 0            # (upstream: a tile that is entirely invalid, or whose fit raises "no valid points")
            active = (~failed).astype(np.uint8)
            out = plan.new_results(n_bins)
            self.n_iterations = np.zeros(n, dtype=np.int64)
            for i in range(it["max_iterations"]):
                if not active.any():
                    break
                plan.step(active, ox, oy, res, n_bins, out)
                for t in np.flatnonzero(active):
                    self.n_iterations[t] += 1
                    if out["n_valid"][t] == 0:    # ("The subsample contains no more valid values": a ValueError of the tile's fit)
                        failed[t], active[t] = True, 0
                        continue
                    det = {k: out[k][t] for k in ("vshift", "n_valid", "y_mean", "y_std", "edges", "counts", "medians")}
                    try:
                        east, north, _ = _bin_fit_from_step(det, fb["fit_optimizer"], plan.dtype)
                    except (ValueError, TypeError) as e:
                        logging.error(f"Failed to fit coregistration. Reason: {e}")
                        failed[t], active[t] = True, 0
                        continue
                    ox[t], oy[t], vs[t] = ox[t] + east * res[0], oy[t] + north * res[1], float(det["vshift"])
                    if i > 1 and float(np.sqrt(east**2 + north**2)) < it["tolerance"]:
                        active[t] = 0
        sx, sy, sz = -ox, -oy, vs * step.vertical_shift
        for a in (sx, sy, sz):
            a[failed] = np.nan
        return sx, sy, sz

    def _fit_loop(self, ref, tba, inlier_mask, tiles, t6):
        n = tiles.shape[0]
        sx, sy, sz = np.full(n, np.nan), np.full(n, np.nan), np.full(n, np.nan)

        def cut(a, r0, r1, c0, c1):   # (the steps' fit takes host arrays: a tile of a device raster is fetched)
            return a[r0:r1, c0:c1].cpu().numpy() if is_tensor(a) else np.ascontiguousarray(a[r0:r1, c0:c1])

        def all_invalid(a) -> bool:
            return not bool(np.isfinite(a).any())

        for t, (r0, r1, c0, c1) in enumerate(tiles):
            ref_t, tba_t = cut(ref, r0, r1, c0, c1), cut(tba, r0, r1, c0, c1)
            if all_invalid(ref_t) or all_invalid(tba_t):
                continue
            inl_t = None if inlier_mask is None else cut(inlier_mask, r0, r1, c0, c1)
            tile_t6 = (t6[0], t6[1], t6[2] + t6[0] * c0 + t6[1] * r0, t6[3], t6[4], t6[5] + t6[3] * c0 + t6[4] * r0)
            step = self.procstep.copy()
            try:
                step.fit(ref_t, tba_t, inl_t, transform=tile_t6)
            except (ValueError, TypeError) as e:
                logging.error(f"Failed to fit coregistration. Reason: {e}")
                continue
            aff = step.meta["outputs"]["affine"]
            sx[t], sy[t], sz[t] = aff.get("shift_x", np.nan), aff.get("shift_y", np.nan), aff.get("shift_z", np.nan)
        return sx, sy, sz

    def fit(self, reference_elev, to_be_aligned_elev, inlier_mask=None, *, transform=None, resolution=None) -> None:
        """Fit a copy of the step on every tile of ``tiling_grid(shape, block_size_fit)`` (blockwise.py:156-223).  Two 2-D arrays on one
        grid -- NumPy, or contiguous CUDA tensors of one dtype -- whose georeferencing comes from ``transform`` or from ``resolution``."""
        t6 = _transform6(transform, resolution)
        res = (abs(t6[0]), abs(t6[4]))
        ref, tba = reference_elev, to_be_aligned_elev
        if not is_tensor(ref):
            ref, tba = nan_filled(ref), nan_filled(tba)
        if tuple(ref.shape) != tuple(tba.shape) or len(ref.shape) != 2:
            raise ValueError("ref and tba must be 2D arrays of the same shape")
        self.meta["inputs"] = self.procstep.meta["inputs"]
        grid = tiling_grid(tuple(ref.shape), self.block_size_fit)
        tiles = grid.reshape(-1, 4)
        shifts = self._fit_batched(ref, tba, inlier_mask, tiles, res) if self._batched_candidate() else None
        self.fit_route = "batched" if shifts is not None else "loop"
        if shifts is None:
            shifts = self._fit_loop(ref, tba, inlier_mask, tiles, t6)
        self.shape_tiling_grid = grid.shape
        # the tile centres: (col0 + block / 2, row0 + block / 2) * transform -- the BLOCK size, also for the larger merged tiles
        col, row = tiles[:, 2] + self.block_size_fit / 2, tiles[:, 0] + self.block_size_fit / 2
        self.x_coords = np.array(t6[0] * col + t6[1] * row + t6[2])
        self.y_coords = np.array(t6[3] * col + t6[4] * row + t6[5])
        self.shifts_x, self.shifts_y, self.shifts_z = (np.array(s) for s in shifts)
        n_cols = grid.shape[1]
        for t in range(tiles.shape[0]):
            self.meta["outputs"][f"{t // n_cols}_{t % n_cols}"] = {"shift_x": self.shifts_x[t], "shift_y": self.shifts_y[t],
                                                                    "shift_z": self.shifts_z[t]}

    # ---- apply ----------------------------------------------------------------------------------------------------------------------
    @staticmethod
    def _ransac(x_coords, y_coords, shifts, threshold: float = 0.01, max_iterations: int = 2000) -> tuple[float, float, float]:
        """Estimate ``(a, b, c)`` of ``shift = a x + b y + c`` with RANSAC (blockwise.py:225-289, statement for statement)."""
        from sklearn.linear_model import LinearRegression, RANSACRegressor

        if np.isnan(shifts).all():
            shifts = np.zeros_like(shifts)
        points = np.dstack([x_coords, y_coords, shifts])
        points = np.squeeze(points)
        if points.ndim == 1:   # one point: squeeze() gives (3,)
            if points.shape[0] != 3:
                raise ValueError(f"Unexpected point shape: {points.shape}")
            points = points.reshape(1, 3)
        points = points[~np.isnan(points).any(axis=1)]
        if points.size == 0:
            raise ValueError("No valid points after removing NaNs.")
        if np.allclose(points[:, 1], points[0, 1]):      # variation along x only
            a, c = np.polyfit(points[:, 0], points[:, 2], 1)
            b = 0.0
        elif np.allclose(points[:, 0], points[0, 0]):    # variation along y only
            b, c = np.polyfit(points[:, 1], points[:, 2], 1)
            a = 0.0
        else:
            X = points[:, :2]
            y = points[:, 2]
            ransac = RANSACRegressor(estimator=LinearRegression(), residual_threshold=threshold, max_trials=max_iterations)
            ransac.fit(X, y)
            a, b = ransac.estimator_.coef_
            c = ransac.estimator_.intercept_
        return a, b, c

    def coefficients(self, threshold_ransac: float = 0.01, max_iterations_ransac: int = 2000):
        """The three ``_ransac`` fits of ``apply`` (blockwise.py:365-388): ``(coeff_x, coeff_y, coeff_z)``."""
        if not hasattr(self, "shifts_x"):
            raise AssertionError(".fit() does not seem to have been called yet")
        cx = self._ransac(self.x_coords, self.y_coords, self.shifts_x, threshold_ransac, max_iterations_ransac)
        cy = self._ransac(self.x_coords, self.y_coords, self.shifts_y, threshold_ransac, max_iterations_ransac)
        cz = (self._ransac(self.x_coords, self.y_coords, self.shifts_z, threshold_ransac, max_iterations_ransac)
              if self.apply_z_correction else (0, 0, 0))
        return cx, cy, cz

    def apply(self, to_be_aligned_elev, threshold_ransac: float = 0.01, max_iterations_ransac: int = 2000, *, transform=None, resolution=None):
        """Warp the raster by the planes fitted through the tiles' shifts (blockwise.py:351-407).  Returns the aligned array, or
        ``(array, transform)`` when ``transform=`` is given."""
        cx, cy, cz = self.coefficients(threshold_ransac, max_iterations_ransac)
        out = warp_affine_field(to_be_aligned_elev, _transform6(transform, resolution), cx, cy, cz)
        return out if transform is None else (out, transform)
