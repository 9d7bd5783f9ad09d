"""Golden vectors for LZD and the rotation-capable raster apply, recorded from the REFERENCE's own functions (needs the reference source
tree, so it runs only where that tree is present; the fixtures it writes are what the tests read).

On one float32 and one float64 pair of 96 x 128 (NaN holes, an inlier mask, a known small rigid misalignment) it records:

1. helper matrices for a list of parameter sets: ``matrix_from_translations_rotations``, ``invert_matrix``, ``_apply_matrix_pts_arr``;
2. ``_iterate_method(_lzd_iteration_step, ...)`` (affine.py:102-147, 1589-1677) per nodata rule 0..3 and for both ``only_translation``
   values, driven with interpolator callables built from tests/rigid_oracle.py (geoutils' interpolator is absent: the taps are the
   stated convention, parity unpinned; the DRIVER and ``_lzd_fit`` with ``scipy.optimize.least_squares`` are the reference's): every
   iteration's matrix and statistic, at the default tolerance 0.01 (three iterations, the fewest the stop rule allows) and at 1e-5
   (keys ``*_tight``: more iterations), and ``solve_gap`` = the largest matrix-element gap, over all iterations of all runs, between
   ``_lzd_fit`` and a float64 ``lstsq`` on the same six arrays (least_squares stops on ftol = 1e-8: the gap is its truncation);
3. ``_iterate_affine_regrid_small_rotations`` (base.py:1389-1519) for matrices with rotations of about 0.01, 0.5, 5 and 15 degrees on
   DEMs with and without NaN blocks, run with a small ``Raster`` shim (pixel-centre coordinates) and SciPy's real
   ``RegularGridInterpolator``; per case the oracle's count of pixels that converge at iteration 1, and overall
   ``regrid_flip_share`` (share of pixels within rounding of the 1e-4 res threshold, which BLAS's summation order may switch) and
   ``regrid_gap`` (largest |reference - oracle| on the other pixels);
4. tests/golden/signatures_lzd.json: the signatures of ``LZD.__init__``, ``LZD.fit``, ``LZD.apply`` and ``apply_matrix``.

    python tools/gen_golden_lzd.py
"""
from __future__ import annotations

import inspect
import json
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]
import _refimport  # noqa: E402
import rigid_oracle  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
TIGHT_TOLERANCE = 1e-5

PARAM_SETS = [(0.0, 0.0, 0.0, 0.0, 0.0, 0.0), (3.0, -2.0, 1.5, 0.0, 0.0, 0.0), (20.0, 5.0, 0.1, 0.1, 0.05, 0.01),
              (-4.5, 12.25, -3.0, -1.5, 2.5, 7.0), (0.5, 0.25, -0.125, 15.0, -12.0, 19.0)]
# (t1, t2, t3, alpha1, alpha2, alpha3 in degrees; with the centroid; on the DEM with NaN blocks)
REGRID_SETS = [((0.7, -0.4, 0.3, 0.01, -0.008, 0.012), True, False), ((3.0, -2.0, 1.5, 0.5, -0.3, 0.4), True, True),
               ((0.0, 0.0, 0.0, 0.0, 0.0, 0.6), True, False), ((-6.0, 4.0, 2.0, 5.0, -4.0, 3.0), False, True),
               ((10.0, -8.0, -1.0, -15.0, 12.0, 14.0), True, False)]


def _literal(v):
    if v is inspect.Parameter.empty:
        return "<required>"
    if v is None or isinstance(v, (bool, int, float, str)):
        return v
    if isinstance(v, (tuple, list)) and all(x is None or isinstance(x, (bool, int, float, str)) for x in v):
        return list(v)
    return "<object>"


def _record(fn) -> list:
    return [{"name": n, "kind": p.kind.name, "default": _literal(p.default)} for n, p in inspect.signature(fn).parameters.items()]


def surface(x, y):
    return 800.0 + 40.0 * np.sin(x / 90.0) * np.cos(y / 70.0) + 15.0 * np.sin((x + y) / 50.0) + 0.02 * x - 0.015 * y


def pair(rng, H, W, dtype, t6, misalign, base_mod):
    """ref = a smooth surface on the grid; tba = ref seen through the inverse of ``misalign`` (the oracle's regrid: an input, not a
    recorded result) plus noise; NaN holes in both, a patchy inlier mask."""
    rows, cols = np.mgrid[0:H, 0:W]
    x, y = rigid_oracle.pixel_xy(t6, rows, cols)
    ref = surface(x - t6[2], y - t6[5]).astype(dtype)
    M = base_mod.matrix_from_translations_rotations(*misalign)
    Minv = base_mod.invert_matrix(M)
    cen = (float(x.mean()), float(y.mean()), float(ref.mean()))
    tba = rigid_oracle.regrid(ref.astype(np.float64), t6, Minv, cen)[0]
    tba = (tba + rng.normal(scale=0.02, size=(H, W))).astype(dtype)
    ref[rng.random((H, W)) < 0.02] = np.nan
    tba[rng.random((H, W)) < 0.02] = np.nan
    tba[30:34, 50:61] = np.nan
    inlier = np.ones((H, W), dtype=bool)
    inlier[60:75, 20:45] = False
    inlier[rng.random((H, W)) < 0.02] = False
    return ref, tba, inlier


class _Cloud:
    def __init__(self, x, y, z):
        self.geometry = types.SimpleNamespace(x=types.SimpleNamespace(values=x), y=types.SimpleNamespace(values=y))
        self.z = types.SimpleNamespace(values=z)


class RasterShim:
    """What ``_iterate_affine_regrid_small_rotations`` asks of ``gu.Raster``: pixel-centre coordinates, every pixel in the point cloud
    (NaN elevations kept), raster order."""

    def __init__(self, arr, t6):
        self.arr, self.t6 = arr, tuple(float(v) for v in t6)
        self.res = (abs(self.t6[0]), abs(self.t6[4]))

    @classmethod
    def from_array(cls, data, transform, crs=None, nodata=None):
        return cls(np.asarray(data), transform)

    def to_pointcloud(self, data_column_name="z", skip_nodata=False):
        H, W = self.arr.shape
        rows, cols = np.divmod(np.arange(H * W), W)
        x, y = rigid_oracle.pixel_xy(self.t6, rows, cols)
        return types.SimpleNamespace(ds=_Cloud(x, y, self.arr.ravel().astype(np.float64)))

    def coords(self, grid=False):
        H, W = self.arr.shape
        x = rigid_oracle.pixel_xy(self.t6, np.zeros(W), np.arange(W))[0]
        y = rigid_oracle.pixel_xy(self.t6, np.arange(H), np.zeros(H))[1]
        return x, np.flip(y)   # both ascending

    def from_pointcloud_regular(self, epc, transform, shape, data_column_name="z", nodata=None):
        return types.SimpleNamespace(data=np.ma.masked_invalid(np.asarray(epc.z).reshape(shape)))


def main() -> None:
    import scipy.optimize

    mods = _refimport.load()
    affine, base = mods.affine, mods.base
    rng = np.random.default_rng(1988)
    H, W = 96, 128
    rec = {}

    # 1. helper matrices
    pts = rng.uniform(-500.0, 500.0, size=(3, 40))
    cen = (12.5, -40.0, 300.0)
    rec["helper_params"] = np.array(PARAM_SETS, dtype=np.float64)
    rec["helper_points"], rec["helper_centroid"] = pts, np.array(cen)
    rec["helper_matrix"] = np.array([base.matrix_from_translations_rotations(*p) for p in PARAM_SETS])
    rec["helper_matrix_rad"] = np.array([base.matrix_from_translations_rotations(*p[:3], *np.deg2rad(p[3:]), use_degrees=False) for p in PARAM_SETS])
    rec["helper_inverse"] = np.array([base.invert_matrix(m) for m in rec["helper_matrix"]])
    rec["helper_params_back"] = np.array([base.translations_rotations_from_matrix(m) for m in rec["helper_matrix"]], dtype=np.float64)
    rec["helper_applied"] = np.array([np.array(base._apply_matrix_pts_arr(pts[0], pts[1], pts[2], m, centroid=cen)) for m in rec["helper_matrix"]])
    rec["helper_applied_inv"] = np.array([np.array(base._apply_matrix_pts_arr(pts[0], pts[1], pts[2], m, centroid=cen, invert=True))
                                          for m in rec["helper_matrix"]])

    # 2. the LZD driver
    solve_gap = 0.0
    orig_fit = affine._lzd_fit

    def fit_and_compare(x, y, z, dh, gradx, grady, params_fit_or_bin, only_translation, **kwargs):
        nonlocal solve_gap
        m = orig_fit(x=x, y=y, z=z, dh=dh, gradx=gradx, grady=grady, params_fit_or_bin=params_fit_or_bin, only_translation=only_translation, **kwargs)
        p = rigid_oracle.lstsq_step(np.array([x, y, z, dh, gradx, grady], dtype=np.float64), only_translation)
        solve_gap = max(solve_gap, float(np.abs(m - base.matrix_from_translations_rotations(*p, use_degrees=False)).max()))
        return m

    affine._lzd_fit = fit_and_compare
    params = {"fit_or_bin": "fit", "fit_minimizer": scipy.optimize.least_squares, "fit_loss_func": "linear"}
    cases = (("f32", np.float32, (10.0, 0.0, 1000.0, 0.0, -10.0, 5000.0), (3.0, -2.0, 1.5, 0.05, -0.03, 0.1)),
             ("f64", np.float64, (5.0, 0.0, -200.0, 0.0, -7.5, 900.0), (-1.5, 2.5, -0.75, -0.04, 0.06, -0.08)))
    dems = {}
    for name, dtype, t6, misalign in cases:
        ref, tba, inlier = pair(rng, H, W, dtype, t6, misalign, base)
        mask = inlier & np.isfinite(ref) & np.isfinite(tba)
        dems[name] = (ref, tba, t6)
        rec[f"{name}_filled"] = np.where(np.isfinite(ref), ref, np.nanmean(ref)).astype(ref.dtype)
        rec[f"{name}_ref"], rec[f"{name}_tba"], rec[f"{name}_inlier"], rec[f"{name}_mask"] = ref, tba, inlier, mask
        rec[f"{name}_transform"], rec[f"{name}_misalign"] = np.array(t6), np.array(misalign)
        gradx, grady = rigid_oracle.gradient_planes(ref, abs(t6[0]), abs(t6[4]))
        rows, cols = np.nonzero(mask)
        sub_coords = rigid_oracle.pixel_xy(t6, rows, cols)
        sub_pts = tba[mask]
        centroid = (float(np.nanmean(sub_coords[0])), float(np.nanmean(sub_coords[1])), float(np.nanmean(sub_pts)))
        rec[f"{name}_centroid"] = np.array(centroid)
        for rule in range(4):
            def interp(img):
                return lambda yx, img=img: rigid_oracle.point_taps(img, *rigid_oracle.xy_to_pixel(t6, yx[1], yx[0]), rule)

            # (tolerance 0.01 is the default: the driver settles in its minimum of three iterations; 1e-5 makes it go on, so that the
            #  recorded statistics say something about the stop rule)
            for only_t, tolerance, tag in ((False, 0.01, ""), (True, 0.01, ""), (False, TIGHT_TOLERANCE, "_tight"), (True, TIGHT_TOLERANCE, "_tight")):
                trail = []

                def method(matrix, *const):
                    new, stat = affine._lzd_iteration_step(matrix, *const)
                    trail.append((new.copy(), float(stat)))
                    return new, stat

                const = (interp(ref), sub_pts, (sub_coords[0].copy(), sub_coords[1].copy()), centroid, interp(gradx), interp(grady), params, only_t)
                final = affine._iterate_method(method=method, iterating_input=np.eye(4), constant_inputs=const, tolerance=tolerance,
                                               max_iterations=200)
                key = f"{name}_r{rule}_t{int(only_t)}{tag}"
                rec[f"{key}_matrices"] = np.array([t[0] for t in trail])
                rec[f"{key}_stats"] = np.array([t[1] for t in trail])
                rec[f"{key}_final"] = np.array(final)
                assert tag == "" or len(trail) > 3, key
                print(key, "iterations", len(trail), "statistics", [f"{t[1]:.3g}" for t in trail])
    affine._lzd_fit = orig_fit
    rec["solve_gap"], rec["tight_tolerance"] = np.array(solve_gap), np.array(TIGHT_TOLERANCE)
    print("solve_gap", solve_gap)

    # 3. the regrid
    import geoutils

    saved = geoutils.Raster
    geoutils.Raster = RasterShim
    flip = total = 0
    gap = 0.0
    partial = False
    try:
        for k, (p, with_centroid, holes) in enumerate(REGRID_SETS):
            name = "f32" if k % 2 == 0 else "f64"
            ref, tba, t6 = dems[name]
            dem_key = f"{name}_tba" if holes else f"{name}_filled"   # (the DEMs are stored once)
            dem = rec[dem_key]
            matrix = base.matrix_from_translations_rotations(*p)
            x, y = rigid_oracle.pixel_xy(t6, *np.mgrid[0:H, 0:W])
            cen3 = (float(x.mean()), float(y.mean()), float(np.nanmean(dem))) if with_centroid else None
            got = base._iterate_affine_regrid_small_rotations(dem=dem, transform=t6, matrix=matrix, centroid=cen3, resampling="linear")[0]
            mine, n_first, near = rigid_oracle.regrid(dem, t6, matrix, cen3, details=True)
            assert np.array_equal(np.isnan(got[~near]), np.isnan(mine[~near])), k
            d = np.abs(got.astype(np.float64) - mine.astype(np.float64))[~near]
            gap = max(gap, float(np.nanmax(d)) if np.isfinite(d).any() else 0.0)
            flip += int(near.sum())
            total += near.size
            partial = partial or 0 < n_first < dem.size
            rec[f"regrid{k}_dem_key"], rec[f"regrid{k}_params"], rec[f"regrid{k}_matrix"] = np.array(dem_key), np.array(p), matrix
            rec[f"regrid{k}_centroid"] = np.array(cen3 if cen3 is not None else (np.nan,) * 3)
            rec[f"regrid{k}_transform"], rec[f"regrid{k}_out"], rec[f"regrid{k}_n_first"] = np.array(t6), got, np.array(n_first)
            print("regrid", k, name, p, "converged at iteration 1:", n_first, "of", dem.size, "near threshold:", int(near.sum()),
                  "finite out:", int(np.isfinite(got).sum()), "gap", float(np.nanmax(d)) if np.isfinite(d).any() else 0.0)
    finally:
        geoutils.Raster = saved
    assert partial, "no matrix for which some but not all pixels converge at iteration 1"
    rec["regrid_n"] = np.array(len(REGRID_SETS))
    rec["regrid_flip_share"], rec["regrid_gap"] = np.array(flip / total), np.array(gap)
    print("regrid_flip_share", flip / total, "regrid_gap", gap)
    assert flip / total < 0.01

    out = os.path.join(GOLDEN, "lzd_golden.npz")
    np.savez_compressed(out, **rec)
    print(out, os.path.getsize(out), "bytes")

    sig = {"coreg": {"LZD.__init__": _record(affine.LZD.__init__), "LZD.fit": _record(affine.LZD.fit), "LZD.apply": _record(affine.LZD.apply),
                     "apply_matrix": _record(base.apply_matrix)}}
    with open(os.path.join(GOLDEN, "signatures_lzd.json"), "w") as f:
        json.dump(sig, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
