"""Golden vectors for ICP, recorded from the REFERENCE's own functions (needs the reference source tree, so it runs only where that tree
is present; the fixtures it writes are what the tests read).

Inputs: one float32 and one float64 pair of 96 x 128 at 10 m -- the surface of gen_golden_lzd.py with amplitudes 120 and 40, ``tba`` =
``ref`` seen through the inverse of ``matrix_from_translations_rotations(12, -8, 1.5, 0.3, -0.2, 0.5)`` plus N(0, 0.02) noise, 2 % NaN
in each raster, a patchy inlier mask -- ``subsample = 1``, tolerance 1e-5.  The misalignment is large on purpose: the generator
asserts that more than 30 % of the points match a pixel other than their own at iteration 0, that picky removes more than 5 % of the
pairs, and that the smallest relative margin between nearest and second-nearest distance stays above 1e-9.

The reference's ``_icp_norms``, ``_standardize_epc``, ``_icp_iteration_step``, ``_icp_fit`` and ``_iterate_method`` are driven with a
real ``scipy.spatial.KDTree`` and pandas.  Two geoutils names are stubs where the reference imports them, so the generator sets
``affine.nmad`` to the stated convention (``1.4826 * median|v - median v|``, parity unpinned) and ``affine._res`` to ``(|a|, |e|)``.

Runs per dtype: ``plane`` (point-to-plane, default minimiser, picky), ``lsq`` (point-to-plane, "lsq_approx", not picky), ``point``
(point-to-point, default minimiser, picky), ``trans`` (point-to-plane, only_translation, picky).

Recorded per dtype: the rasters, the inlier mask, the reference's normal planes, the validity mask, centroid and std_fac.  Per run
and iteration: the input matrix, the step matrix, the statistic, cond(J^T J), the number of kept pairs and CRC-32 digests of ``ind``
(int64) and of the kept query indexes (int64); the final matrix.  ``ind`` as int16 offsets from the query's own index, the kept flags
and every sixteenth ``dists`` value are stored in full for iterations 0, 1 and the last of every run only: a committed file may not
exceed 1 MiB, and the float64 distances of all iterations are 24 MB.  The clouds are not stored: the oracle rebuilds them from the
rasters and the mask, and the generator asserts that they equal the reference's bit for bit after ``_standardize_epc``.

Recorded gaps: ``norms_gap`` (reference planes against the oracle's, ulps of the dtype, per dtype), ``solve_gap`` (largest element
gap between ``_icp_fit`` with least_squares and the oracle's Gauss-Newton on the same pairs), ``lsq_gap`` (the same for "lsq_approx"
against the oracle's lstsq), ``trajectory_gap`` (largest element gap between the final matrices of the reference driver run with
``_icp_fit`` as it is and with the oracle's solve in its place, de-standardised); the solve and trajectory gaps also per run.  tests/golden/signatures_icp.json: ``ICP.__init__``, ``fit``, ``apply``.

    python tools/gen_golden_icp.py
"""
from __future__ import annotations

import inspect
import json
import os
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]
import _refimport  # noqa: E402
import icp_oracle  # noqa: E402
import rigid_oracle  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
TOLERANCE = 1e-5
MISALIGN = (12.0, -8.0, 1.5, 0.3, -0.2, 0.5)
DIST_STRIDE = 16
RUNS = {"plane": ("point-to-plane", "default", True, False), "lsq": ("point-to-plane", "lsq_approx", False, False),
        "point": ("point-to-point", "default", True, False), "trans": ("point-to-plane", "default", True, True)}


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
    return 800.0 + 120.0 * np.sin(x / 90.0) * np.cos(y / 70.0) + 40.0 * np.sin((x + y) / 50.0) + 0.02 * x - 0.015 * y


def pair(rng, H, W, dtype, t6, base_mod):
    rows, cols = np.mgrid[0:H, 0:W]
    x, y = rigid_oracle.pixel_xy(t6, rows, cols)
    ref = surface(x - t6[2], y - t6[5]).astype(dtype)
    Minv = base_mod.invert_matrix(base_mod.matrix_from_translations_rotations(*MISALIGN))
    cen = (float(x.mean()), float(y.mean()), float(ref.mean()))
    tba = rigid_oracle.regrid(ref.astype(np.float64), t6, Minv, cen)[0]
    tba = (tba + rng.normal(scale=0.02, size=(H, W))).astype(dtype)
    ref[rng.random((H, W)) < 0.02] = np.nan
    tba[rng.random((H, W)) < 0.02] = np.nan
    inlier = np.ones((H, W), dtype=bool)
    inlier[60:75, 20:45] = False
    inlier[rng.random((H, W)) < 0.02] = False
    return ref, tba, inlier


def ulp_gap(a: np.ndarray, b: np.ndarray) -> int:
    it = np.int32 if a.dtype == np.float32 else np.int64
    ok = np.isfinite(a) & np.isfinite(b)
    assert np.array_equal(np.isfinite(a), np.isfinite(b))

    def key(v):
        k = v.view(it).astype(np.int64)
        return np.where(k < 0, np.iinfo(it).min - k, k)

    return int(np.abs(key(a[ok]) - key(b[ok])).max())


def crc(a: np.ndarray) -> int:
    return zlib.crc32(np.ascontiguousarray(a, dtype=np.int64).tobytes())


def main() -> None:
    import pandas as pd
    import scipy.optimize
    import scipy.spatial

    mods = _refimport.load()
    affine, base = mods.affine, mods.base
    affine.nmad = icp_oracle.nmad
    affine._res = lambda t: (abs(t[0]), abs(t[4]))
    rng = np.random.default_rng(1992)
    H, W = 96, 128
    rec = {"tolerance": np.array(TOLERANCE), "misalign": np.array(MISALIGN), "dist_stride": np.array(DIST_STRIDE)}
    gaps = {"solve_gap": 0.0, "lsq_gap": 0.0, "trajectory_gap": 0.0}
    margin_min, moved0, dup_share = np.inf, [], []
    orig_fit = affine._icp_fit

    for name, dtype, t6 in (("f32", np.float32, (10.0, 0.0, 1000.0, 0.0, -10.0, 5000.0)), ("f64", np.float64, (10.0, 0.0, -300.0, 0.0, -10.0, 2000.0))):
        ref, tba, inlier = pair(rng, H, W, dtype, t6, base)
        nx, ny, nz = affine._icp_norms(ref, t6)
        assert nx.dtype == ny.dtype == nz.dtype == dtype
        mine = icp_oracle.normals(ref, abs(t6[0]), abs(t6[4]))
        rec[f"{name}_norms_gap"] = np.array([ulp_gap(a, b) for a, b in zip((nx, ny, nz), mine)])
        print(name, "norms_gap (ulps)", rec[f"{name}_norms_gap"])
        rec[f"{name}_ref"], rec[f"{name}_tba"], rec[f"{name}_inlier"] = ref, tba, np.packbits(inlier)
        rec[f"{name}_transform"] = np.array(t6)
        rec[f"{name}_nx"], rec[f"{name}_ny"], rec[f"{name}_nz"] = nx, ny, nz
        for run, (method, minimizer, picky, only_t) in RUNS.items():
            plane = method == "point-to-plane"
            mask = inlier & np.isfinite(ref) & np.isfinite(tba)
            if plane:
                mask &= np.isfinite(nx) & np.isfinite(ny) & np.isfinite(nz)
            rows, cols = np.nonzero(mask)
            x, y = rigid_oracle.pixel_xy(t6, rows, cols)
            ref_epc = np.vstack((x, y, ref[mask]))
            tba_epc = np.vstack((x, y, tba[mask]))
            norms = np.vstack((nx[mask], ny[mask], nz[mask])) if plane else None
            ref_epc, tba_epc, centroid, std_fac = affine._standardize_epc(ref_epc, tba_epc, scale_std=True)
            norms64 = None if norms is None else norms.astype(np.float64)
            # the oracle's clouds are the reference's, bit for bit (that is why they need not be stored)
            o_ref, o_tba, o_n = icp_oracle.clouds(ref, tba, mask, t6, (nx, ny, nz) if plane else None)
            o_ref, o_tba, o_cen, o_fac = icp_oracle.standardize(o_ref, o_tba)
            assert np.array_equal(o_ref, ref_epc) and np.array_equal(o_tba, tba_epc) and o_cen == tuple(centroid) and o_fac == std_fac
            assert norms is None or np.array_equal(o_n, norms64)
            key = f"{name}_{run}"
            rec[f"{key}_mask"] = np.packbits(mask)
            rec[f"{key}_centroid"], rec[f"{key}_std_fac"] = np.array(centroid), np.array(std_fac)
            tree = scipy.spatial.KDTree(ref_epc.T)
            params = {"fit_or_bin": "fit", "fit_minimizer": scipy.optimize.least_squares if minimizer == "default" else "lsq_approx",
                      "fit_loss_func": "linear"}
            own = np.arange(ref_epc.shape[1])
            trail, run_gap = [], [0.0]

            def fit_and_compare(ref, tba, norms, method, params_fit_or_bin, only_translation, **kwargs):
                m = orig_fit(ref=ref, tba=tba, norms=norms, method=method, params_fit_or_bin=params_fit_or_bin, only_translation=only_translation,
                             **kwargs)
                if isinstance(params_fit_or_bin["fit_minimizer"], str):
                    gap, which = float(np.abs(m - icp_oracle.lsq_approx(ref, tba, norms)[0]).max()), "lsq_gap"
                else:
                    gap, which = float(np.abs(m - icp_oracle.gauss_newton(ref, tba, norms, method, only_translation)[0]).max()), "solve_gap"
                gaps[which] = max(gaps[which], gap)
                run_gap[0] = max(run_gap[0], gap)
                trail[-1]["fit_in"] = (ref, tba, norms)
                trail[-1]["step"] = m
                return m

            def oracle_fit(ref, tba, norms, method, params_fit_or_bin, only_translation, **kwargs):
                return icp_oracle.solve(ref, tba, norms, method, "lsq_approx" if minimizer == "lsq_approx" else "device", only_translation)

            def method_fn(matrix, *const):
                trail.append({"matrix_in": matrix.copy()})
                new, stat = affine._icp_iteration_step(matrix, *const)
                trail[-1]["stat"] = float(stat)
                return new, stat

            const = (ref_epc, tba_epc, norms64, tree, params, method, picky, only_t)
            affine._icp_fit = fit_and_compare
            final = affine._iterate_method(method=method_fn, iterating_input=np.eye(4), constant_inputs=const, tolerance=TOLERANCE / std_fac,
                                           max_iterations=20)
            affine._icp_fit = oracle_fit
            final_oracle = affine._iterate_method(method=affine._icp_iteration_step, iterating_input=np.eye(4), constant_inputs=const,
                                                  tolerance=TOLERANCE / std_fac, max_iterations=20)
            affine._icp_fit = orig_fit
            final[:3, 3] *= std_fac          # de-standardise, as icp() does (affine.py:1177)
            final_oracle[:3, 3] *= std_fac
            tgap = float(np.abs(final - final_oracle).max())
            gaps["trajectory_gap"] = max(gaps["trajectory_gap"], tgap)
            n_it = len(trail)
            full = sorted({0, 1, n_it - 1})
            rec[f"{key}_full_iterations"] = np.array(full)
            arrs = {k: [] for k in ("matrix_in", "step", "stat", "cond", "n_kept", "crc_ind", "crc_kept")}
            for i, t in enumerate(trail):
                trans = base._apply_matrix_pts_mat(tba_epc, matrix=t["matrix_in"])
                d2, i2 = tree.query(trans.T, k=2)
                dists, ind = tree.query(trans.T, k=1)
                assert np.array_equal(ind, i2[:, 0]) and np.array_equal(dists, d2[:, 0])
                margin_min = min(margin_min, float(((d2[:, 1] - d2[:, 0]) / d2[:, 1]).min()))
                if picky:
                    kept = pd.DataFrame(data={"ind": ind, "dists": dists}).groupby(["ind"]).idxmin()["dists"].values
                    dup_share.append(1.0 - kept.size / ind.size)
                else:
                    kept = own
                # what _icp_fit received is what these indexes select
                f_ref, f_tba, f_n = t["fit_in"]
                assert np.array_equal(f_ref, ref_epc[:, ind[kept]]) and np.array_equal(f_tba, trans[:, kept])
                assert f_n is None or np.array_equal(f_n, norms64[:, ind[kept]])
                # the oracle's removal is pandas'
                kq, kr = icp_oracle.pairs(ind, dists, picky)
                assert np.array_equal(kq, kept) and np.array_equal(kr, ind[kept])
                if i == 0:
                    moved0.append(float(np.mean(ind != own)))
                J, _ = icp_oracle.pair_terms(f_ref, f_tba, f_n, np.eye(4), method)
                A = J[3:] if only_t else J
                for k, v in (("matrix_in", t["matrix_in"]), ("step", t["step"]), ("stat", t["stat"]), ("cond", float(np.linalg.cond(A @ A.T))),
                             ("n_kept", kept.size), ("crc_ind", crc(ind)), ("crc_kept", crc(kept))):
                    arrs[k].append(v)
                if i in full:
                    off = ind - own
                    assert np.abs(off).max() < 2 ** 15
                    flags = np.zeros(ind.size, dtype=bool)
                    flags[kept] = True
                    rec[f"{key}_it{i}_ind_offset"] = off.astype(np.int16)
                    rec[f"{key}_it{i}_kept"] = np.packbits(flags)
                    rec[f"{key}_it{i}_dists"] = dists[::DIST_STRIDE].copy()
            for k, v in arrs.items():
                rec[f"{key}_{k}"] = np.array(v)
            rec[f"{key}_final"] = np.array(final)
            rec[f"{key}_trajectory_gap"], rec[f"{key}_solve_gap"] = np.array(tgap), np.array(run_gap[0])
            print(key, "points", ref_epc.shape[1], "iterations", n_it, "moved at 0:", f"{moved0[-1]:.3f}", "kept", arrs["n_kept"][0], "..", arrs["n_kept"][-1],
                  "cond", f"{max(arrs['cond']):.3g}", "trajectory gap", f"{tgap:.3g}", "solve gap", f"{run_gap[0]:.3g}", "stat", f"{arrs['stat'][-1]:.3g}")
            assert n_it >= 4, key
    for k, v in gaps.items():
        rec[k] = np.array(v)
    rec["margin_min"] = np.array(margin_min)
    print(gaps, "margin_min", margin_min, "moved at iteration 0", min(moved0), "duplicates", min(dup_share), max(dup_share))
    assert min(moved0) > 0.30, "the misalignment leaves the points on their own pixel"
    assert min(dup_share) > 0.05, "picky removes too few pairs"
    assert margin_min > 1e-9, "a nearest / second-nearest tie"

    out = os.path.join(GOLDEN, "icp_golden.npz")
    np.savez_compressed(out, **rec)
    print(out, os.path.getsize(out), "bytes")
    assert os.path.getsize(out) < 2 ** 20

    sig = {"coreg": {"ICP.__init__": _record(affine.ICP.__init__), "ICP.fit": _record(affine.ICP.fit), "ICP.apply": _record(affine.ICP.apply)}}
    with open(os.path.join(GOLDEN, "signatures_icp.json"), "w") as f:
        json.dump(sig, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
