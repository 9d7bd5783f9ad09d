"""Golden vectors for CPD, recorded from the REFERENCE's own functions (needs the reference source tree, so it runs only where that tree
is present; the fixtures it writes are what the tests read).

Inputs: one float32 and one float64 pair of 32 x 40 at 10 m -- gen_golden_icp.py's surface, misalignment (12, -8, 1.5; 0.3, -0.2, 0.5
degrees), noise, 2 % NaN in each raster and 2 % outliers in the inlier mask -- ``subsample = 1``: about 1100 points, four full blocks
of 256 and a tail.

The reference's ``_standardize_epc``, ``_cpd_iteration_step`` (hence ``_cpd_fit``) and ``_iterate_method`` are driven as ``cpd()``
drives them.  geoutils' ``nmad`` is a stub where the reference imports it, so the generator sets ``affine.nmad`` to the stated
convention (``1.4826 * median|v - median v|``, parity unpinned).

Runs per dtype: ``rigid`` (w = 0, tolerance 0.01), ``tight`` (w = 0, tolerance 1e-5), ``weight`` (w = 0.3), ``trans``
(only_translation), ``nostd`` (standardize=False).

Recorded per dtype (one file each, tests/golden/cpd_golden_<dtype>.npz: the float64 vectors of both would exceed what one committed
file may hold): the rasters, the inlier bits, the transform, centroid and std_fac (with and without scaling).  Per run and iteration:
the input ``(matrix, sigma2)`` (NaN for upstream's None), the output ``(matrix, sigma2, q)`` and the statistic; ``P1``, ``Pt1`` and
``PX`` (3, M) in full -- the locals of ``_cpd_fit`` when it returns -- for iterations 0, 1 and the last; the final de-standardised
matrix; ``subsample_final``.  The clouds are not stored: the oracle rebuilds them, and the generator asserts that they equal the
reference's bit for bit.

Recorded gaps.  tests/cpd_oracle.py's driver runs on the same clouds with chunk lengths 64, 256 and 1000, and with chunk 256 and
every exponential multiplied by ``1 + delta``, delta uniform in +-2 * 2^-52 (seeded) -- a stand-in for another ``exp`` and another
order.  ``<run>_perturb_gap`` = the largest deviation of any variant from the reference's trajectory over all iterations: matrix
elements (absolute), sigma2 (relative), q (relative).  The generator ASSERTS that every variant stops at the reference's iteration
and that at every iteration ``|stat - tol| / tol > 1e-6``: no stop decision sits on a rounding.

tests/golden/signatures_cpd.json: ``CPD.__init__``, ``fit``, ``apply``.

    python tools/gen_golden_cpd.py
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
import _refimport  # noqa: E402
import cpd_oracle  # noqa: E402
import gen_golden_icp  # noqa: E402
import icp_oracle  # noqa: E402
import rigid_oracle  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
H, W = 32, 40
#        weight, only_translation, standardize, tolerance
RUNS = {"rigid": (0.0, False, True, 0.01), "tight": (0.0, False, True, 1e-5), "weight": (0.3, False, True, 0.01),
        "trans": (0.0, True, True, 0.01), "nostd": (0.0, False, False, 0.01)}
MAX_ITERATIONS = 100
CHUNKS = (64, 256, 1000)
PERTURB_SEED = 2010
MARGIN = 1e-6


def main() -> None:
    mods = _refimport.load()
    affine, base = mods.affine, mods.base
    affine.nmad = icp_oracle.nmad
    rng = np.random.default_rng(2010)
    captured: dict = {}

    def profiler(frame, event, arg):   # the locals of _cpd_fit as it returns
        if event == "return" and frame.f_code.co_name == "_cpd_fit":
            loc = frame.f_locals
            captured.update(P1=np.array(loc["P1"]), Pt1=np.array(loc["Pt1"]), PX=np.array(loc["PX"]).T.copy())

    for name, dtype, t6 in (("f32", np.float32, (10.0, 0.0, 1000.0, 0.0, -10.0, 5000.0)), ("f64", np.float64, (10.0, 0.0, -300.0, 0.0, -10.0, 2000.0))):
        ref, tba, inlier = gen_golden_icp.pair(rng, H, W, dtype, t6, base)
        rec = {"ref": ref, "tba": tba, "inlier": np.packbits(inlier), "transform": np.array(t6), "misalign": np.array(gen_golden_icp.MISALIGN)}
        mask = inlier & np.isfinite(ref) & np.isfinite(tba)
        rows, cols = np.nonzero(mask)
        x, y = rigid_oracle.pixel_xy(t6, rows, cols)
        raw_ref, raw_tba = np.vstack((x, y, ref[mask])), np.vstack((x, y, tba[mask]))
        rec["subsample_final"] = np.array(raw_ref.shape[1])
        for run, (weight, only_t, scale_std, tol) in RUNS.items():
            ref_epc, tba_epc, centroid, std_fac = affine._standardize_epc(raw_ref, raw_tba, scale_std=scale_std)
            o_ref, o_tba, _ = icp_oracle.clouds(ref, tba, mask, t6)
            o_ref, o_tba, o_cen, o_fac = icp_oracle.standardize(o_ref, o_tba, scale_std)
            assert np.array_equal(o_ref, ref_epc) and np.array_equal(o_tba, tba_epc) and o_cen == tuple(centroid) and o_fac == std_fac
            rec[f"{run}_centroid"], rec[f"{run}_std_fac"] = np.array(centroid), np.array(std_fac)
            tol_std = tol / std_fac
            trail = []

            def method(inp, *const):
                new, stat = affine._cpd_iteration_step(inp, *const)
                trail.append({"matrix_in": np.array(inp[0]), "sigma2_in": np.nan if inp[1] is None else float(inp[1]), "matrix": np.array(new[0]),
                              "sigma2": float(new[1]), "q": float(new[2]), "stat": float(stat), **captured})
                return new, stat

            sys.setprofile(profiler)
            try:
                final, _, _ = affine._iterate_method(method=method, iterating_input=(np.eye(4), None, np.inf),
                                                     constant_inputs=(ref_epc, tba_epc, weight, tol_std / 10, only_t), tolerance=tol_std,
                                                     max_iterations=MAX_ITERATIONS)
            finally:
                sys.setprofile(None)
            final = base.invert_matrix(final)
            final[:3, 3] *= std_fac
            n_it = len(trail)
            assert 3 < n_it < MAX_ITERATIONS, (name, run, n_it)
            for t in trail:
                assert abs(t["stat"] - tol_std) / tol_std > MARGIN, (name, run, "a stop decision sits on a rounding")
            # the oracle's variants: other chunk lengths (other orders), and perturbed exponentials
            gap = np.zeros(3)
            variants = [(c, None) for c in CHUNKS] + [(256, np.random.default_rng(PERTURB_SEED))]
            for chunk, perturb in variants:
                o_final, o_trail = cpd_oracle.drive(ref_epc, tba_epc, weight, only_t, tol_std, MAX_ITERATIONS, chunk, perturb)
                assert len(o_trail) == n_it, (name, run, chunk, len(o_trail), n_it)
                for a, b in zip(trail, o_trail):
                    assert abs(b["stat"] - tol_std) / tol_std > MARGIN
                    gap = np.maximum(gap, [np.abs(a["matrix"] - b["matrix"]).max(), abs(a["sigma2"] - b["sigma2"]) / abs(a["sigma2"]),
                                           abs(a["q"] - b["q"]) / abs(a["q"])])
            rec[f"{run}_perturb_gap"] = gap
            for k in ("matrix_in", "sigma2_in", "matrix", "sigma2", "q", "stat"):
                rec[f"{run}_{k}"] = np.array([t[k] for t in trail])
            full = sorted({0, 1, n_it - 1})
            rec[f"{run}_full_iterations"] = np.array(full)
            for i in full:
                for k in ("P1", "Pt1", "PX"):
                    rec[f"{run}_it{i}_{k}"] = trail[i][k]
            rec[f"{run}_final"] = np.array(final)
            rec[f"{run}_settings"] = np.array([weight, float(only_t), float(scale_std), tol])
            print(name, run, "points", ref_epc.shape[1], "iterations", n_it, "gap", gap, "final t", final[:3, 3], "stat", trail[-1]["stat"], "tol", tol_std)
        out = os.path.join(GOLDEN, f"cpd_golden_{name}.npz")
        np.savez_compressed(out, **rec)
        print(out, os.path.getsize(out), "bytes")
        assert os.path.getsize(out) < 2 ** 20

    sig = {"coreg": {"CPD.__init__": gen_golden_icp._record(affine.CPD.__init__), "CPD.fit": gen_golden_icp._record(affine.CPD.fit),
                     "CPD.apply": gen_golden_icp._record(affine.CPD.apply)}}
    with open(os.path.join(GOLDEN, "signatures_cpd.json"), "w") as f:
        json.dump(sig, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
