"""Raster-point coregistration without a GPU: the product's host code (``xdem_amd.coreg`` / ``biascorr`` / ``epc``: routing, the
Nuth-Kaab iteration and curve fit, the minimiser, the host bin statistics, the pipeline) over ``tests/rstpts_oracle.OraclePlan`` in
``PtsPlan``'s place, against the reference runs recorded by tools/gen_golden_rstpts.py."""
import os

import numpy as np
import pytest

from conftest import GOLDEN
from rstpts_cases import NK_BAR_PX, NK_BAR_Z, SHAPES

DTYPES = {"f32": np.float32, "f64": np.float64}
KEYS = [(tag, H, W, n, rule, d) for tag in DTYPES for H, W, n in SHAPES for rule in range(4) for d in ("p", "r")]


@pytest.fixture(scope="module")
def golden():
    return {tag: np.load(os.path.join(GOLDEN, f"rstpts_golden_{tag}.npz")) for tag in DTYPES}


@pytest.fixture()
def oracle_plan(monkeypatch):
    """``PtsPlan`` and ``apply_matrix_pts`` replaced by the CPU oracle for the test; yields the oracle class (its ``nan_rule`` is reset)."""
    import rstpts_oracle
    from xdem_amd import epc

    monkeypatch.setattr(epc, "PtsPlan", rstpts_oracle.OraclePlan)
    monkeypatch.setattr(epc, "apply_matrix_pts", rstpts_oracle.apply_matrix_pts)
    calls = {"steps": 0}
    orig = rstpts_oracle.OraclePlan._device_step

    def counted(self, *a):
        calls["steps"] += 1
        return orig(self, *a)

    monkeypatch.setattr(rstpts_oracle.OraclePlan, "_device_step", counted)
    rstpts_oracle.OraclePlan.calls = calls
    yield rstpts_oracle.OraclePlan
    rstpts_oracle.OraclePlan.nan_rule = None


def _case(tag, H, W, n):
    from xdem_amd import EPC, synth

    c = synth.cloud_case(H, W, n, DTYPES[tag])
    return c, EPC(c["x"], c["y"], c["z"])


def _pair(c, cloud, direction):
    return (cloud, c["raster"]) if direction == "p" else (c["raster"], cloud)


def test_the_bar_stays_below_the_methods_stopping_threshold():
    """The bar of the whole-fit tests -- 4 x the largest measured deviation of a fit's final offsets from the recorded reference run
    (tests/rstpts_cases.py) -- stays below NuthKaab's own stopping threshold, 1e-3 pixel.  (With p0 taken from float64 sums instead of
    NumPy's nanmean / nanstd in y's dtype it did not: 2.844e-4 pixel in one case)"""
    assert 0 <= NK_BAR_PX < 1e-3


@pytest.mark.parametrize("tag,H,W,n,rule,direction", KEYS)
def test_nuth_kaab_fit_follows_the_recorded_reference_run(golden, oracle_plan, tag, H, W, n, rule, direction):
    """Same number of iterations as ``_iterate_method(_nuth_kaab_iteration_step, ...)``; final offsets within the measured bar (p0 is
    formed as the reference forms it, from NumPy's nanmean / nanstd of y in its own dtype: over the oracle plan the runs coincide)."""
    from xdem_amd import coreg

    oracle_plan.nan_rule = rule
    c, cloud = _case(tag, H, W, n)
    g, key = golden[tag], f"{H}x{W}_r{rule}_{direction}"
    fit = coreg.NuthKaab().fit(*_pair(c, cloud, direction), c["inlier"], transform=c["transform"])
    trail, final = g[f"{key}_nk_trail"], g[f"{key}_nk_final"]
    out = fit.meta["outputs"]
    dev = (abs(-out["affine"]["shift_x"] - final[0]) / c["res"][0], abs(-out["affine"]["shift_y"] - final[1]) / c["res"][1],
           abs(out["affine"]["shift_z"] - final[2]))
    print(f"{tag} {key}: iterations {oracle_plan.calls['steps']} / {len(trail)}, deviation px {max(dev[:2]):.3e}, vertical {dev[2]:.3e}")
    assert oracle_plan.calls["steps"] == len(trail)
    assert out["random"]["subsample_final"] == int(g[f"{key}_n_valid"])
    assert max(dev[:2]) <= NK_BAR_PX and dev[2] <= NK_BAR_Z


@pytest.mark.parametrize("tag,H,W,n,rule,direction", [k for k in KEYS if k[4] in (0, 3)])
def test_dhminimize_and_vertical_shift_reproduce_the_recorded_runs(golden, oracle_plan, tag, H, W, n, rule, direction):
    """The minimiser sees the same losses, bit for bit, so it evaluates the recorded points and ends where the reference ended; the
    vertical shift is the recorded median."""
    from xdem_amd import coreg

    oracle_plan.nan_rule = rule
    c, cloud = _case(tag, H, W, n)
    g, key = golden[tag], f"{H}x{W}_r{rule}_{direction}"
    fit = coreg.DhMinimize().fit(*_pair(c, cloud, direction), c["inlier"], transform=c["transform"])
    off = g[f"{key}_dhmin_offsets"]
    a = fit.meta["outputs"]["affine"]
    assert (a["shift_x"], a["shift_y"], a["shift_z"]) == (off[0], off[1], off[2])
    assert fit.meta["outputs"]["specific"]["n_evaluations"] == len(g[f"{key}_dhmin_traj"])
    assert fit.meta["outputs"]["random"]["subsample_final"] == int(g[f"{key}_n_valid_plain"])
    v = coreg.VerticalShift().fit(*_pair(c, cloud, direction), c["inlier"], transform=c["transform"])
    assert v.meta["outputs"]["affine"]["shift_z"] == g[f"{key}_vshift"][0]
    assert v.meta["outputs"]["random"]["subsample_final"] == int(g[f"{key}_vshift"][1])


def test_fit_recovers_the_shift_of_the_case_in_both_directions(oracle_plan):
    """0.3 m of noise over slopes of a few metres per pixel and ~2700 points leave the estimate a few hundredths of a pixel from the
    truth (the binned medians' scatter): within a tenth of a pixel horizontally and 0.1 m vertically, mirrored for a raster reference."""
    from xdem_amd import coreg, synth

    c, cloud = _case("f32", 96, 128, 3000)
    sx, sy, sz = synth.CLOUD_SHIFT
    a = coreg.NuthKaab().fit(cloud, c["raster"], c["inlier"], transform=c["transform"]).meta["outputs"]["affine"]
    b = coreg.NuthKaab().fit(c["raster"], cloud, c["inlier"], transform=c["transform"]).meta["outputs"]["affine"]
    assert abs(-a["shift_x"] - sx) < 1.0 and abs(-a["shift_y"] - sy) < 1.0 and abs(a["shift_z"] - sz) < 0.1
    assert abs(b["shift_x"] - sx) < 1.0 and abs(b["shift_y"] - sy) < 1.0 and abs(b["shift_z"] + sz) < 0.1


def test_routing_and_refusals(oracle_plan):
    from xdem_amd import EPC, coreg

    c, cloud = _case("f32", 61, 83, 700)
    with pytest.raises(TypeError, match="does not support two point clouds"):
        coreg.NuthKaab().fit(cloud, cloud, transform=c["transform"])
    for step in (coreg.DhMinimize(), coreg.VerticalShift()):
        with pytest.raises(TypeError, match="not point-point methods"):
            step.fit(cloud, cloud, transform=c["transform"])
    for step in (coreg.NuthKaab(), coreg.DhMinimize(), coreg.VerticalShift()):
        with pytest.raises(ValueError, match="'transform' must be given"):
            step.fit(cloud, c["raster"])
        with pytest.raises(ValueError, match="missing the column name 'h'"):
            step.fit(cloud, c["raster"], transform=c["transform"], z_name="h")
    # a plain 1-D array is still not a cloud
    with pytest.raises(ValueError, match="ref and tba must be 2D arrays of the same shape"):
        coreg.DhMinimize().fit(c["raster"], c["z"].astype(np.float32), resolution=10.0)
    # a cloud without a valid point: every z NaN, and every point off the raster
    for bad in (EPC(c["x"], c["y"], np.full_like(c["z"], np.nan)), EPC(c["x"] + 1e6, c["y"], c["z"])):
        for step in (coreg.NuthKaab(), coreg.DhMinimize(), coreg.VerticalShift()):
            with pytest.raises(ValueError, match="no valid points"):
                step.fit(bad, c["raster"], transform=c["transform"])
    with pytest.raises(NotImplementedError, match="Weights have not yet been implemented"):
        coreg.DhMinimize().fit(cloud, c["raster"], weights=np.ones(3), transform=c["transform"])


def test_the_other_methods_keep_refusing_clouds_with_their_messages():
    from xdem_amd import coreg

    c, cloud = _case("f32", 61, 83, 700)
    for step in (coreg.LZD(), coreg.ICP(), coreg.CPD()):
        with pytest.raises(NotImplementedError, match="point-cloud inputs are not supported: both elevation datasets must be arrays on one grid"):
            step.fit(cloud, c["raster"], transform=c["transform"])
    for step in (coreg.DirectionalBias(), coreg.TerrainBias(), coreg.BiasCorr()):
        with pytest.raises(NotImplementedError, match="Point-cloud inputs are not implemented for the bias corrections here"):
            step.fit(c["raster"], cloud, transform=c["transform"], bias_vars={"a": c["raster"]})


def test_meta_outputs_subsample_and_options(oracle_plan):
    from xdem_amd import coreg

    c, cloud = _case("f64", 61, 83, 700)
    t = c["transform"]
    fit = coreg.NuthKaab(subsample=300, vertical_shift=False).fit(cloud, c["raster"], c["inlier"], transform=t, random_state=7)
    assert fit.meta["outputs"]["random"] == {"subsample_final": 300} and fit.meta["outputs"]["affine"]["shift_z"] == 0.0
    again = coreg.NuthKaab(subsample=300, vertical_shift=False).fit(cloud, c["raster"], c["inlier"], transform=t, random_state=7)
    assert again.meta["outputs"] == fit.meta["outputs"]
    assert coreg.NuthKaab(subsample=0.5).fit(cloud, c["raster"], transform=t, random_state=1).meta["outputs"]["random"]["subsample_final"] > 250
    # the other statistics and the un-binned fit run on the host over the plan's columns and land near the median's answer
    ref = coreg.NuthKaab().fit(cloud, c["raster"], c["inlier"], transform=t).meta["outputs"]["affine"]
    for kw in ({"bin_statistic": np.nanmean}, {"bin_before_fit": False}, {"bin_sizes": 36}, {"bin_sizes": {"aspect": np.linspace(0, 2 * np.pi, 41)}},
               {"bin_statistic": lambda v: np.nanpercentile(v, 50)}):
        got = coreg.NuthKaab(**kw).fit(cloud, c["raster"], c["inlier"], transform=t).meta["outputs"]["affine"]
        assert abs(got["shift_x"] - ref["shift_x"]) < 3.0 and abs(got["shift_y"] - ref["shift_y"]) < 3.0, kw
    # np.nanpercentile(50) IS the median wherever a bin's count is odd or its middle values agree: same iteration, nearly the same fit
    start = coreg.NuthKaab(initial_shift=(-7.0, 3.0)).fit(cloud, c["raster"], c["inlier"], transform=t).meta["outputs"]["affine"]
    assert abs(start["shift_x"] - ref["shift_x"]) < 0.05 and abs(start["shift_y"] - ref["shift_y"]) < 0.05
    m = fit.to_matrix()
    assert m[0, 3] == fit.meta["outputs"]["affine"]["shift_x"] and m[2, 3] == 0.0


def test_apply_moves_a_cloud_and_the_pipeline_equals_its_steps_by_hand(oracle_plan):
    import rigid_oracle
    from xdem_amd import EPC, coreg

    c, cloud = _case("f32", 61, 83, 700)
    t = c["transform"]
    # the cloud as the to-be-aligned side: moved between the steps by each step's matrix
    pipe = (coreg.VerticalShift() + coreg.NuthKaab()).fit(c["raster"], cloud, c["inlier"], transform=t)
    v = coreg.VerticalShift().fit(c["raster"], cloud, c["inlier"], transform=t)
    moved = v.apply(cloud, transform=t)
    # (explicit sums: 0 * NaN is NaN, so a point with a non-finite z loses its coordinates too, as under upstream's matrix product)
    assert isinstance(moved, EPC) and all(np.array_equal(a, b, equal_nan=True) for a, b in
                                          zip((moved.x, moved.y, moved.z), rigid_oracle.apply_pts(v.to_matrix(), None, c["x"], c["y"], c["z"])))
    nk = coreg.NuthKaab().fit(c["raster"], moved, c["inlier"], transform=t)
    assert pipe.pipeline[0].meta["outputs"] == v.meta["outputs"] and pipe.pipeline[1].meta["outputs"] == nk.meta["outputs"]
    out = pipe.apply(cloud, transform=t)
    by_hand = nk.apply(moved)
    assert isinstance(out, EPC) and all(np.array_equal(getattr(out, k), getattr(by_hand, k), equal_nan=True) for k in "xyz")
    # apply_matrix on a cloud: any rotation, the inverse, a centroid
    m = coreg.matrix_from_translations_rotations(3.0, -2.0, 1.5, 25.0, -40.0, 60.0)
    cen = (500400.0, 4200300.0, 1000.0)
    got = coreg.apply_matrix(cloud, m, invert=True, centroid=cen)
    want = rigid_oracle.apply_pts(rigid_oracle.rigid_inverse(m), cen, c["x"], c["y"], c["z"])
    assert isinstance(got, EPC) and all(np.array_equal(a, b, equal_nan=True) for a, b in zip((got.x, got.y, got.z), want))


def test_epc_answers_what_upstream_asks_and_any_such_object_is_a_cloud(oracle_plan):
    import types

    from xdem_amd import EPC, coreg, epc

    c, cloud = _case("f32", 61, 83, 700)
    assert cloud.columns == ["z", "geometry"] and len(cloud) == 700
    assert cloud.geometry.x.values is cloud.x and cloud.geometry.y.values is cloud.y and cloud["z"].values is cloud.z
    named = EPC(c["x"], c["y"], c["z"], data_column="h")
    assert named.columns == ["h", "geometry"] and named["h"].values is named.z
    with pytest.raises(ValueError, match="must be 1-D"):
        EPC(np.zeros((2, 2)), np.zeros(4), np.zeros(4))
    with pytest.raises(ValueError, match="same length"):
        EPC(np.zeros(3), np.zeros(4), np.zeros(4))

    class Frame:   # a stand-in for a GeoDataFrame: the four calls and nothing else
        columns = ["geometry", "z"]
        geometry = types.SimpleNamespace(x=types.SimpleNamespace(values=c["x"]), y=types.SimpleNamespace(values=c["y"]))

        def __getitem__(self, name):
            return types.SimpleNamespace(values={"z": c["z"]}[name])

    assert epc.is_cloud(Frame()) and epc.is_cloud(cloud) and not epc.is_cloud(c["z"]) and not epc.is_cloud(c["raster"])
    a = coreg.VerticalShift().fit(Frame(), c["raster"], c["inlier"], transform=c["transform"]).meta["outputs"]
    b = coreg.VerticalShift().fit(cloud, c["raster"], c["inlier"], transform=c["transform"]).meta["outputs"]
    assert a == b
    # the data column of an EPC is found without naming it; a frame's is "z" unless named
    assert coreg.VerticalShift().fit(named, c["raster"], c["inlier"], transform=c["transform"]).meta["outputs"] == b


@pytest.mark.parametrize("tag", sorted(DTYPES))
def test_recorded_apply_matrix_is_the_oracles_up_to_the_order_of_its_sums(golden, tag):
    """``_apply_matrix_pts_arr`` multiplies with BLAS, the oracle adds ``((m0 x + m1 y) + m2 z) + m3``: three products and three sums of
    terms no larger than the largest coordinate (4.2e6), so the two differ by at most 8 * 2^-52 * 3 * 4.3e6."""
    import rstpts_oracle
    from xdem_amd import synth

    g = golden[tag]
    H, W, n = SHAPES[-1]
    c = synth.cloud_case(H, W, n, DTYPES[tag])
    x, y, z = c["x"][:40], c["y"][:40], c["z"][:40]
    cen = tuple(g["apply_cen"])
    bound = 8 * 2.0**-52 * 3 * 4.3e6
    for k, m in enumerate(g["apply_matrix"]):
        for name, kw in (("plain", {}), ("centroid", {"centroid": cen}), ("inverted", {"centroid": cen, "invert": True})):
            got = np.array(rstpts_oracle.apply_matrix_pts(x, y, z, m, **kw))
            assert np.abs(got - g[f"apply_{name}"][k]).max() <= bound, (k, name)
