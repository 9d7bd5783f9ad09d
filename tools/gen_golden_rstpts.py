"""Golden vectors for raster-point coregistration, recorded from the REFERENCE's own functions (needs the reference source tree, so it
runs only where that tree is present; the fixtures it writes are what the tests read).

Inputs are ``xdem_amd.synth.cloud_case`` (rebuilt by the tests, not stored): 61 x 83 with 700 points and 96 x 128 with 3000, float32 and
float64 (one file per dtype).  Per shape, nodata rule 0..3 and direction (``p``: the cloud is the reference, ``r``: the raster is) it
records

1. every iteration's offsets and statistic of ``_iterate_method(_nuth_kaab_iteration_step, ...)`` (affine.py:102-147, 477-536) at the
   defaults (tolerance 0.001, 10 iterations, 72 bins, ``np.nanmedian``, ``curve_fit``);
2. the evaluations (x0, x1, loss) and the result of ``_dh_minimize_fit`` (affine.py:636-674) with the default Nelder-Mead and
   ``fit_loss_func = binning_oracle.nmad``;
3. ``vertical_shift`` (affine.py:721-765) with ``np.median``;

all driven with the dh interpolator, the valid points and the slope tangent / aspect columns of tests/rstpts_oracle.py (geoutils'
``_interp_points`` is absent: the taps are the stated convention, parity unpinned; the drivers, the binning, the curve fit and the
minimiser are the reference's).  And, once per file, ``_apply_matrix_pts_arr`` (base.py) for the parameter sets of
tools/gen_golden_lzd.py on the first 40 points of the larger cloud, with and without a centroid, forward and inverted.

    python tools/gen_golden_rstpts.py
"""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]
import _refimport  # noqa: E402
import binning_oracle  # noqa: E402
import rstpts_oracle  # noqa: E402
from rstpts_cases import SHAPES  # noqa: E402
from xdem_amd import synth  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
PARAM_SETS = [(0.0, 0.0, 0.0, 0.0, 0.0, 0.0), (3.0, -2.0, 1.5, 0.0, 0.0, 0.0), (20.0, 5.0, 0.1, 0.1, 0.05, 0.01),
              (-4.5, 12.25, -3.0, -1.5, 2.5, 7.0), (0.5, 0.25, -0.125, 15.0, -12.0, 19.0)]   # (tools/gen_golden_lzd.py)


def main() -> None:
    import scipy.optimize

    mods = _refimport.load()
    affine, base = mods.affine, mods.base
    for tag, dtype in (("f32", np.float32), ("f64", np.float64)):
        rec = {}
        for H, W, n in SHAPES:
            case = synth.cloud_case(H, W, n, dtype)
            for rule in range(4):
                rstpts_oracle.OraclePlan.nan_rule = rule
                for direction, pts_is_ref in (("p", True), ("r", False)):
                    key = f"{H}x{W}_r{rule}_{direction}"
                    plan = rstpts_oracle.OraclePlan(case["raster"], case["x"], case["y"], case["z"], case["transform"], pts_is_ref,
                                                    case["inlier"], with_nk_aux=True)
                    _, st, asp = plan.shift_values(0.0, 0.0, aux=True)
                    trail = []

                    def method(offsets, *const):
                        new, stat = affine._nuth_kaab_iteration_step(offsets, *const)
                        trail.append((*new, float(stat)))
                        return new, stat

                    params = {"fit_or_bin": "bin_and_fit", "fit_optimizer": scipy.optimize.curve_fit, "bin_sizes": 72,
                              "bin_statistic": np.nanmedian, "nd": 1, "bias_var_names": ["aspect"]}
                    const = (lambda sx, sy, plan=plan: plan.shift_values(sx, sy).copy(), st, asp, case["res"], params)
                    final = affine._iterate_method(method=method, iterating_input=(0.0, 0.0, 0.0), constant_inputs=const, tolerance=0.001,
                                                   max_iterations=10)
                    rec[f"{key}_nk_trail"] = np.array(trail, dtype=np.float64)
                    rec[f"{key}_nk_final"] = np.array(final, dtype=np.float64)
                    rec[f"{key}_n_valid"] = np.array(plan.n_valid)
                    # DhMinimize and VerticalShift: valid points by the raster and the mask alone
                    plan = rstpts_oracle.OraclePlan(case["raster"], case["x"], case["y"], case["z"], case["transform"], pts_is_ref,
                                                    case["inlier"])
                    calls = []

                    def loss(dh):
                        v = binning_oracle.nmad(dh)
                        calls.append(float(v))
                        return v

                    pos = []

                    def interp(sx, sy, plan=plan):
                        pos.append((float(sx), float(sy)))
                        return plan.shift_values(sx, sy)

                    dparams = {"fit_or_bin": "fit", "fit_minimizer": scipy.optimize.minimize, "fit_loss_func": loss}
                    off = affine._dh_minimize_fit(dh_interpolator=interp, params_fit_or_bin=dparams)
                    rec[f"{key}_dhmin_traj"] = np.array([(*p, c) for p, c in zip(pos, calls)], dtype=np.float64)   # (the last position has no loss: the median's)
                    rec[f"{key}_dhmin_offsets"] = np.array(off, dtype=np.float64)
                    rec[f"{key}_n_valid_plain"] = np.array(plan.n_valid)
                    dh0 = plan.shift_values(0.0, 0.0)
                    saved = affine._preprocess_pts_rst_subsample
                    # (dh = sub_ref - sub_tba: the oracle's dh column stands for the pair the absent interpolator would return)
                    affine._preprocess_pts_rst_subsample = lambda **kw: (dh0, np.zeros_like(dh0), None, None)
                    try:
                        v, nsub = affine.vertical_shift(ref_elev=None, tba_elev=None, inlier_mask=None, transform=None, crs=None, area_or_point=None,
                                                        params_random={"subsample": 1, "random_state": None}, vshift_reduc_func=np.median,
                                                        z_name="z")
                    finally:
                        affine._preprocess_pts_rst_subsample = saved
                    rec[f"{key}_vshift"] = np.array([v, nsub], dtype=np.float64)
                    print(tag, key, "nk iterations", len(trail), "final", final, "dhmin", off, "evaluations", len(calls), "vshift", v)
        rstpts_oracle.OraclePlan.nan_rule = None
        H, W, n = SHAPES[-1]
        case = synth.cloud_case(H, W, n, dtype)
        x, y, z = case["x"][:40], case["y"][:40], case["z"][:40]
        cen = (float(x.mean()), float(y.mean()), float(z.mean()))
        rec["apply_params"], rec["apply_cen"] = np.array(PARAM_SETS), np.array(cen)
        mats = [base.matrix_from_translations_rotations(*p) for p in PARAM_SETS]
        rec["apply_matrix"] = np.array(mats)
        for name, kw in (("plain", {}), ("centroid", {"centroid": cen}), ("inverted", {"centroid": cen, "invert": True})):
            rec[f"apply_{name}"] = np.array([np.array(base._apply_matrix_pts_arr(x, y, z, m, **kw)) for m in mats])
        out = os.path.join(GOLDEN, f"rstpts_golden_{tag}.npz")
        np.savez_compressed(out, **rec)
        print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
