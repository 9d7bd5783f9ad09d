"""Raster-point coregistration on the MI355X: the device plan (``xdem_amd.epc.PtsPlan``, csrc/ptsplan.hip) bit for bit against
``tests/rstpts_oracle.OraclePlan``, the agreement of its routes, and whole fits against the reference runs recorded by
tools/gen_golden_rstpts.py."""
import math
import os

import numpy as np
import pytest

from conftest import GOLDEN, decided
from rstpts_cases import NK_BAR_PX, NK_BAR_Z, SHAPES

pytestmark = pytest.mark.gpu
DTYPES = {"f32": np.float32, "f64": np.float64}
SHIFTS = ((0.0, 0.0), (7.5, -4.0), (30.0, -20.0), (5000.0, 0.0))   # zero, the case's own, whole pixels, one that leaves nothing


@pytest.fixture(scope="module")
def ctx():
    from xdem_amd import _lib

    c = _lib.default_context()
    yield c
    c.set_option("nk_nan_rule", decided("nk_nan_rule"))
    c.set_option("selection", 0)
    c.set_option("pts_tile_order", 0)


@pytest.fixture(scope="module")
def cases():
    from xdem_amd import synth

    return {(tag, H, W): synth.cloud_case(H, W, n, dt) for tag, dt in DTYPES.items() for H, W, n in SHAPES}


def _plans(ctx, c, rule, pts_is_ref, aux=True, raster=None):
    """(device plan, oracle plan) of a case under a tap rule."""
    import rstpts_oracle
    from xdem_amd import epc

    ctx.set_option("nk_nan_rule", rule)
    rstpts_oracle.OraclePlan.nan_rule = rule
    try:
        o = rstpts_oracle.OraclePlan(c["raster"], c["x"], c["y"], c["z"], c["transform"], pts_is_ref, c["inlier"], with_nk_aux=aux)
    finally:
        rstpts_oracle.OraclePlan.nan_rule = None
    p = epc.PtsPlan(c["raster"] if raster is None else raster, c["x"], c["y"], c["z"], c["transform"], pts_is_ref, c["inlier"], with_nk_aux=aux, ctx=ctx)
    return p, o


def _align_aspect(p, o):
    """float64 only: the device's arctangent (ocml) and NumPy's (libm) may differ in the last bit, as tests/test_nuthkaab_gpu.py states
    for the raster plan; the interpolated aspect column must agree within 4 ulp of 2 pi and the oracle goes on with the device's own,
    so that edges, bins and medians compare bit for bit.  Call with every valid point selected."""
    if o.dtype != np.float64:
        return
    asp = p.shift_values(0.0, 0.0, aux=True)[2]
    assert np.abs(asp - o.asp[o.sel]).max() <= 4 * np.spacing(2 * np.pi)
    o.asp = o.asp.copy()
    o.asp[o.sel] = asp


def _same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def _check_step(got, want, n_terms_bound=True):
    """Integers, edges and medians bit for bit; y_mean / y_std within n * 2^-52 * sum|terms| of the fsum values, carried through
    mean = S1 / n and std = sqrt(S2 / n - mean^2): |d var| <= (e2 + 2 |mean| e1) / n + 4 * 2^-52 * (S2 / n), d std = d var / (2 std)."""
    assert got["n_valid"] == want["n_valid"] and got["vshift"] == want["vshift"]
    assert _same(got["edges"], want["edges"]) and _same(got["counts"], want["counts"]) and _same(got["medians"], want["medians"])
    n, eps = want["n_valid"], 2.0**-52
    e1, e2 = n * eps * want["abs1"], n * eps * want["abs2"]
    assert abs(got["y_mean"] - want["y_mean"]) <= e1 / n + 2 * eps * abs(want["y_mean"])
    dvar = (e2 + 2 * abs(want["y_mean"]) * e1) / n + 4 * eps * want["abs2"] / n
    if want["y_std"] > 0:
        assert abs(got["y_std"] - want["y_std"]) <= dvar / (2 * want["y_std"]) + 2 * eps * want["y_std"]
    else:
        assert got["y_std"] <= math.sqrt(dvar)


@pytest.mark.parametrize("tag", sorted(DTYPES))
@pytest.mark.parametrize("rule", range(4))
@pytest.mark.parametrize("pts_is_ref", (True, False))
def test_validity_selection_dh_columns_step_and_nmad_match_the_oracle(ctx, cases, tag, rule, pts_is_ref):
    import rstpts_oracle
    from xdem_amd import _lib
    from xdem_amd._coregbase import subsample_ranks

    c = cases[(tag, 61, 83)]
    p, o = _plans(ctx, c, rule, pts_is_ref)
    with p:
        assert p.n_valid == o.n_valid and _same(p.selection(), o.selection())
        _align_aspect(p, o)
        for draw in (None, subsample_ranks(o.n_valid, 300, 11)):
            if draw is not None:
                assert p.subsample(draw) == o.subsample(draw) == 300
                assert _same(p.selection(), np.sort(np.flatnonzero(o.valid)[draw]))
            for sx, sy in SHIFTS:
                want = o.shift_values(sx, sy, aux=True)
                if not np.isfinite(want[0]).any():
                    with pytest.raises(ValueError, match="The subsample contains no more valid values"):
                        p.step(sx, sy)
                    with pytest.raises(_lib.XdemHipError, match="no valid points"):
                        p.shift_nmad(sx, sy)
                    assert _same(p.shift_values(sx, sy), want[0])
                    continue
                got = p.shift_values(sx, sy, aux=True)
                for name, g, w in zip(("dh", "slope_tan", "aspect"), got, want):
                    assert g.dtype == w.dtype and _same(g, w), (name, sx, sy)
                want_step = rstpts_oracle.step_details(o, sx, sy, 72)
                _check_step(p._device_step(sx, sy, 72), want_step)
                # the public step: the same, with NumPy's nanmean / nanstd of the y column in its own dtype (upstream's p0 ingredients)
                got_step = p.step(sx, sy)
                ycol = p.step_y()
                assert _same(ycol[~np.isnan(ycol)], want_step["y"]) and _same(np.isnan(ycol), ~np.isfinite(want[0]))
                assert got_step["y_mean"] == np.nanmean(want_step["y"]) and got_step["y_std"] == np.nanstd(want_step["y"])
                assert got_step["y_mean"].dtype == o.dtype and _same(got_step["medians"], want_step["medians"])
                assert p.shift_nmad(sx, sy) == o.shift_nmad(sx, sy)
        # explicit edges, and fewer bins
        edges = np.linspace(0.0, 2 * np.pi, 25)
        p.set_bin_edges(edges)
        o.set_bin_edges(edges)
        _check_step(p._device_step(7.5, -4.0, 24), rstpts_oracle.step_details(o, 7.5, -4.0, 24))
        p.set_bin_edges(None)
        o.set_bin_edges(None)
        _check_step(p._device_step(7.5, -4.0, 9), rstpts_oracle.step_details(o, 7.5, -4.0, 9))


@pytest.fixture(scope="module")
def big(ctx):
    """One case with more than 8193 valid points, its device and oracle plans (float32, the decided rule)."""
    from xdem_amd import synth

    c = synth.cloud_case(96, 128, 9400, np.float32)
    p, o = _plans(ctx, c, decided("nk_nan_rule"), True)
    yield c, p, o
    p.close()


@pytest.mark.parametrize("k", (1, 63, 64, 65, 255, 256, 257, 8191, 8192, 8193))
def test_point_counts_at_wave_workgroup_and_staging_edges(ctx, big, k):
    import rstpts_oracle

    c, p, o = big
    ctx.set_option("nk_nan_rule", decided("nk_nan_rule"))
    assert o.n_valid >= 8193
    ranks = np.random.default_rng(k).choice(o.n_valid, k, replace=False)
    assert p.subsample(ranks) == o.subsample(ranks) == k
    want = rstpts_oracle.step_details(o, 7.5, -4.0, 72)
    _check_step(p._device_step(7.5, -4.0, 72), want)
    assert p.step(7.5, -4.0)["y_mean"] == np.nanmean(want["y"])
    assert p.shift_nmad(7.5, -4.0) == o.shift_nmad(7.5, -4.0)
    if k in (63, 64, 65):
        assert {0, 1, 2} <= set(want["counts"].tolist())   # bins with no, one and two members


def test_bracketed_selection_agrees_with_the_digit_passes(ctx):
    """2^22 + 4097 points on a 512 x 512 raster: both selections of the step take the bracketed route (SEL_BRACKET_MIN_N) under
    "selection" 0 and the plain digit passes under 1; integers and medians must be identical (sums: fixed order, the same bits)."""
    from xdem_amd import epc, synth

    c = synth.cloud_case(512, 512, (1 << 22) + 4097 + 600000, np.float32)
    ctx.set_option("nk_nan_rule", decided("nk_nan_rule"))
    with epc.PtsPlan(c["raster"], c["x"], c["y"], c["z"], c["transform"], True, c["inlier"], with_nk_aux=True, ctx=ctx) as p:
        assert p.n_valid >= (1 << 22) + 4097
        assert p.subsample(np.arange((1 << 22) + 4097)) == (1 << 22) + 4097
        out = {}
        for mode in (0, 1):
            ctx.set_option("selection", mode)
            out[mode] = (p.step(7.5, -4.0), p.shift_nmad(7.5, -4.0))
        ctx.set_option("selection", 0)
    a, b = out[0], out[1]
    assert a[1] == b[1] and a[0]["n_valid"] == b[0]["n_valid"] > (1 << 22) - 100000
    assert all(_same(a[0][k], b[0][k]) for k in ("vshift", "edges", "counts", "medians", "y_mean", "y_std"))


@pytest.mark.parametrize("tag", sorted(DTYPES))
def test_tile_order_device_tensors_and_repeated_fits_return_the_same_bits(ctx, cases, tag):
    import torch
    from xdem_amd import EPC, coreg

    c = cases[(tag, 96, 128)]
    rule = decided("nk_nan_rule")
    ctx.set_option("nk_nan_rule", rule)
    outs = []
    for order in (0, 1):
        ctx.set_option("pts_tile_order", order)
        for raster in (None, torch.from_numpy(c["raster"]).cuda()):
            p, _ = _plans(ctx, c, rule, False, raster=raster)
            with p:
                p.subsample(np.random.default_rng(3).choice(p.n_valid, 2000, replace=False))
                outs.append((p.selection(), p.step(7.5, -4.0), p.shift_nmad(-3.0, 2.0), p.shift_values(1.0, 1.0)))
    ctx.set_option("pts_tile_order", 0)
    first = outs[0]
    for o in outs[1:]:
        assert _same(o[0], first[0]) and o[2] == first[2] and _same(o[3], first[3])
        assert all(_same(o[1][k], first[1][k]) for k in first[1])
    cloud = EPC(c["x"], c["y"], c["z"])
    dev = EPC(torch.from_numpy(c["x"]).cuda(), torch.from_numpy(c["y"]).cuda(), torch.from_numpy(c["z"]).cuda())
    fits = [coreg.NuthKaab().fit(cl, r, c["inlier"], transform=c["transform"]).meta["outputs"]
            for cl, r in ((cloud, c["raster"]), (cloud, c["raster"]), (dev, torch.from_numpy(c["raster"]).cuda()))]
    assert fits[0] == fits[1] == fits[2]


@pytest.mark.parametrize("tag", sorted(DTYPES))
def test_apply_matrix_on_a_cloud_matches_the_oracle(ctx, cases, tag):
    import rigid_oracle
    from xdem_amd import EPC, coreg

    c = cases[(tag, 61, 83)]
    cloud = EPC(c["x"], c["y"], c["z"].astype(DTYPES[tag]))
    z64 = cloud.z.astype(np.float64)
    cen = (500400.0, 4200300.0, 1000.0)
    for params in ((3.0, -2.0, 1.5, 0.0, 0.0, 0.0), (-4.5, 12.25, -3.0, -1.5, 2.5, 7.0), (0.5, 0.25, -0.125, 75.0, -40.0, 160.0)):
        m = coreg.matrix_from_translations_rotations(*params)
        for invert, centroid in ((False, None), (False, cen), (True, cen), (True, None)):
            got = coreg.apply_matrix(cloud, m, invert=invert, centroid=centroid)
            want = rigid_oracle.apply_pts(rigid_oracle.rigid_inverse(m) if invert else m, centroid, c["x"], c["y"], z64)
            assert isinstance(got, EPC) and all(_same(a, b) for a, b in zip((got.x, got.y, got.z), want))
    step = coreg.NuthKaab()
    step.meta["outputs"]["affine"] = {"shift_x": 1.5, "shift_y": -2.25, "shift_z": 0.5}
    moved = step.apply(cloud)
    assert all(_same(a, b) for a, b in zip((moved.x, moved.y, moved.z), rigid_oracle.apply_pts(step.to_matrix(), None, c["x"], c["y"], z64)))


@pytest.fixture(scope="module")
def golden():
    return {tag: np.load(os.path.join(GOLDEN, f"rstpts_golden_{tag}.npz")) for tag in DTYPES}


@pytest.mark.parametrize("tag", sorted(DTYPES))
@pytest.mark.parametrize("rule", range(4))
def test_whole_fits_follow_the_recorded_reference_runs(ctx, cases, golden, monkeypatch, tag, rule):
    """Both shapes and both directions per case: NuthKaab takes the reference's number of iterations and ends within the measured bar
    (tests/rstpts_cases.py); DhMinimize sees the reference's losses bit for bit and ends where it ended; VerticalShift is its median."""
    from xdem_amd import EPC, coreg, epc

    ctx.set_option("nk_nan_rule", rule)
    steps = {"n": 0}
    orig = epc.PtsPlan._device_step

    def counted(self, *a):
        steps["n"] += 1
        return orig(self, *a)

    monkeypatch.setattr(epc.PtsPlan, "_device_step", counted)
    g = golden[tag]
    for H, W, _ in SHAPES:
        c = cases[(tag, H, W)]
        cloud = EPC(c["x"], c["y"], c["z"])
        for direction in ("p", "r"):
            key = f"{H}x{W}_r{rule}_{direction}"
            pair = (cloud, c["raster"]) if direction == "p" else (c["raster"], cloud)
            steps["n"] = 0
            out = coreg.NuthKaab().fit(*pair, c["inlier"], transform=c["transform"]).meta["outputs"]
            final = g[f"{key}_nk_final"]
            dev = (abs(-out["affine"]["shift_x"] - final[0]) / c["res"][0], abs(-out["affine"]["shift_y"] - final[1]) / c["res"][1],
                   abs(out["affine"]["shift_z"] - final[2]))
            print(f"{tag} {key}: iterations {steps['n']} / {len(g[f'{key}_nk_trail'])}, deviation px {max(dev[:2]):.3e}, vertical {dev[2]:.3e}")
            assert steps["n"] == len(g[f"{key}_nk_trail"]) and out["random"]["subsample_final"] == int(g[f"{key}_n_valid"])
            assert max(dev[:2]) <= NK_BAR_PX and dev[2] <= NK_BAR_Z
            fit = coreg.DhMinimize().fit(*pair, c["inlier"], transform=c["transform"])
            off, a = g[f"{key}_dhmin_offsets"], fit.meta["outputs"]["affine"]
            assert (a["shift_x"], a["shift_y"], a["shift_z"]) == (off[0], off[1], off[2])
            assert fit.meta["outputs"]["specific"]["n_evaluations"] == len(g[f"{key}_dhmin_traj"])
            v = coreg.VerticalShift().fit(*pair, c["inlier"], transform=c["transform"]).meta["outputs"]
            assert v["affine"]["shift_z"] == g[f"{key}_vshift"][0] and v["random"]["subsample_final"] == int(g[f"{key}_vshift"][1])
    ctx.set_option("nk_nan_rule", decided("nk_nan_rule"))


def test_dem_coregister_3d_takes_a_cloud_as_reference(ctx, cases):
    from xdem_amd import DEM, EPC, coreg

    ctx.set_option("nk_nan_rule", decided("nk_nan_rule"))
    c = cases[("f32", 96, 128)]
    cloud = EPC(c["x"], c["y"], c["z"])
    dem = DEM(c["raster"], c["transform"])
    method = coreg.NuthKaab()
    out = dem.coregister_3d(cloud, method, inlier_mask=c["inlier"])
    a = method.meta["outputs"]["affine"]
    assert isinstance(out, DEM) and out.shape == dem.shape
    assert abs(-a["shift_x"] - c["shift"][0]) < 1.0 and abs(-a["shift_y"] - c["shift"][1]) < 1.0 and abs(a["shift_z"] - c["shift"][2]) < 0.1
