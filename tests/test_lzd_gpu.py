"""LZD and the rotation-capable raster apply on the GPU (csrc/rigid.hip) against the CPU oracle tests/rigid_oracle.py: gradient planes,
the six arrays of an iteration and the regrid bit for bit; the 29 float64 sums within the worst-case bound of recursive summation,
repeatable to the byte; the recorded runs of the reference's driver (tests/golden/lzd_golden.npz, tools/gen_golden_lzd.py); the step
alone, in a pipeline and through ``DEM.coregister_3d``."""
import functools
import os
import warnings

import numpy as np
import pytest

import rigid_oracle
from conftest import GOLDEN, decided

pytestmark = pytest.mark.gpu

SHAPES = [(2, 2), (3, 130), (67, 129), (257, 64)]
BIG = (1500, 1700)   # many workgroups on the dense route: the second reduction kernel adds more partials than it has lanes
LZD_NO_VALID = "The subsample contains no more valid values"


@functools.lru_cache(maxsize=None)
def golden():
    return dict(np.load(os.path.join(GOLDEN, "lzd_golden.npz")))


def _surface(x, y):
    return 800.0 + 40.0 * np.sin(x / 90.0) * np.cos(y / 70.0) + 15.0 * np.sin((x + y) / 50.0) + 0.02 * x - 0.015 * y


def _t6(H, dtype_name):
    return (10.0, 0.0, 1000.0, 0.0, -10.0, 5000.0) if dtype_name == "float32" else (5.0, 0.0, -200.0, 0.0, -7.5, 900.0)


@functools.lru_cache(maxsize=None)
def _pair(H, W, dtype_name):
    """(ref, tba, inlier, t6): tba = ref's surface a fraction of a pixel away; a few NaNs and masked pixels in all but the smallest."""
    rng = np.random.default_rng(H * 1000 + W)
    dt = np.dtype(dtype_name)
    t6 = _t6(H, dtype_name)
    x, y = rigid_oracle.pixel_xy(t6, *np.mgrid[0:H, 0:W])
    ref = _surface(x - t6[2], y - t6[5]).astype(dt)
    tba = (_surface(x - t6[2] + 2.0, y - t6[5] - 1.5) - 0.7 + rng.normal(scale=0.02, size=(H, W))).astype(dt)
    inlier = None
    if H * W > 16:
        ref[rng.random((H, W)) < 0.03] = np.nan
        tba[rng.random((H, W)) < 0.03] = np.nan
        inlier = rng.random((H, W)) >= 0.03
    for a in (ref, tba) + (() if inlier is None else (inlier,)):
        a.setflags(write=False)
    return ref, tba, inlier, t6


def _matrices(H, W, t6):
    from xdem_amd import coreg

    mk = coreg.matrix_from_translations_rotations
    return [np.eye(4), mk(3.0, -2.0, 1.5), mk(0.7, -0.4, 0.3, 0.05, -0.03, 0.1), mk(-2.0, 1.0, 0.5, -0.4, 0.3, 1.2),
            mk(abs(t6[0]) * W / 3.0, 0.0, 0.0, 0.01, 0.0, 0.0)]   # the last one moves a third of the points off the grid


def _plan(ref, tba, inlier, route):
    """(plan, selection mask): every valid pixel (dense route) or the pixels of ``subsample_ranks(n_valid, 3000, 42)`` (list route)."""
    from xdem_amd import coreg

    plan = coreg.DhPlan(ref, tba, inlier)
    mask = np.isfinite(ref) & np.isfinite(tba) & (True if inlier is None else inlier)
    assert plan.n_valid == int(mask.sum())
    if route == "list":
        ranks = coreg.subsample_ranks(plan.n_valid, 3000, 42)
        sel = np.zeros(mask.size, dtype=bool)
        sel[np.flatnonzero(mask.ravel())[ranks]] = True
        mask = sel.reshape(mask.shape)
        assert plan.subsample(ranks) == int(mask.sum())
    return plan, mask


def _check_iteration(plan, ref, tba, gradx, grady, mask, t6, matrix, cen, rule, values=True):
    """One matrix: the six arrays bit for bit, the sums within n 2^-53 sum|term| of fsum, the count exact, two calls the same bytes."""
    from xdem_amd import rigid

    want = rigid_oracle.lzd_arrays(ref, tba, gradx, grady, mask, t6, matrix, cen, rule)
    if values:
        got = rigid.lzd_values(plan, t6, matrix, cen)
        assert got.dtype == np.float64 and got.shape == want.shape and np.array_equal(got, want), (plan.shape, rule)
    n = want.shape[1]
    if n == 0:
        with pytest.raises(ValueError, match=LZD_NO_VALID):
            rigid.LZD()._step_matrix(plan, t6, matrix, cen)
        return 0
    sums, cnt = rigid.lzd_normal(plan, t6, matrix, cen)
    sums2, cnt2 = rigid.lzd_normal(plan, t6, matrix, cen)
    assert cnt == cnt2 == n and sums.tobytes() == sums2.tobytes()
    fs, fabs = rigid_oracle.normal_sums(want)
    bound = n * 2.0 ** -53 * fabs
    print("LZD sums", plan.shape, ref.dtype, "n", n, "worst |got - fsum| / bound", float(np.max(np.abs(sums - fs) / np.maximum(bound, 1e-300))))
    assert np.all(np.abs(sums - fs) <= bound), (np.abs(sums - fs) / np.maximum(bound, 1e-300))
    return n


@pytest.mark.parametrize("route", ["dense", "list"])
@pytest.mark.parametrize("dtype_name", ["float32", "float64"])
@pytest.mark.parametrize("shape", SHAPES)
def test_iteration_against_oracle(shape, dtype_name, route):
    from xdem_amd import rigid

    ref, tba, inlier, t6 = _pair(*shape, dtype_name)
    rule = decided("nk_nan_rule")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        plan, mask = _plan(ref, tba, inlier, route)
        with plan:
            gradx, grady = rigid_oracle.gradient_planes(ref, abs(t6[0]), abs(t6[4]))
            gx, gy = rigid.lzd_gradients(plan, t6)
            assert gx.dtype == ref.dtype and np.array_equal(gx, gradx, equal_nan=True) and np.array_equal(gy, grady, equal_nan=True)
            cen, n_sel = rigid.lzd_centroid(plan, t6)
            want_cen = rigid_oracle.centroid(tba, mask, t6)
            assert n_sel == int(mask.sum()) and cen[:2] == want_cen[:2]
            assert abs(cen[2] - want_cen[2]) <= n_sel * 2.0 ** -53 * float(np.abs(tba[mask].astype(np.float64)).sum())
            assert rigid.lzd_centroid(plan, t6)[0] == cen
            kept = [_check_iteration(plan, ref, tba, gradx, grady, mask, t6, m, cen, rule) for m in _matrices(*shape, t6)]
            assert kept[0] > 0
            if shape[1] >= 64:
                assert 0 < kept[-1] < 0.8 * kept[0]


@pytest.mark.parametrize("rule", [0, 1, 2, 3])
def test_every_nodata_rule(rule):
    from xdem_amd import _lib, rigid

    ref, tba, inlier, t6 = _pair(67, 129, "float32")
    ctx = _lib.default_context()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        gradx, grady = rigid_oracle.gradient_planes(ref, abs(t6[0]), abs(t6[4]))
        with ctx.option_scope("nk_nan_rule", rule):
            for route in ("dense", "list"):
                plan, mask = _plan(ref, tba, inlier, route)
                with plan:
                    cen, _ = rigid.lzd_centroid(plan, t6)
                    for m in _matrices(67, 129, t6)[:4]:
                        assert _check_iteration(plan, ref, tba, gradx, grady, mask, t6, m, cen, rule) > 0
    assert ctx.options.get("nk_nan_rule", 0) == decided("nk_nan_rule")


@pytest.mark.parametrize("route", ["dense", "list"])
def test_multi_workgroup_reduction(route):
    from xdem_amd import rigid

    ref, tba, inlier, t6 = _pair(*BIG, "float32")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        gradx, grady = rigid_oracle.gradient_planes(ref, abs(t6[0]), abs(t6[4]))
        plan, mask = _plan(ref, tba, inlier, route)
        with plan:
            cen, _ = rigid.lzd_centroid(plan, t6)
            m = _matrices(*BIG, t6)[2]
            assert _check_iteration(plan, ref, tba, gradx, grady, mask, t6, m, cen, decided("nk_nan_rule"), values=route == "list") > 0


def test_empty_selection_raises_upstreams_error():
    from xdem_amd import coreg

    ref, tba, inlier, t6 = _pair(67, 129, "float32")
    far = coreg.matrix_from_translations_rotations(1e5, 0.0, 0.0)
    with _plan(ref, tba, inlier, "dense")[0] as plan:
        with pytest.raises(ValueError, match=LZD_NO_VALID):
            coreg.LZD()._step_matrix(plan, t6, far, (0.0, 0.0, 0.0))
    with pytest.raises(ValueError, match=LZD_NO_VALID):   # a first step that throws every point off the grid
        coreg.LZD(fit_minimizer=lambda f, x0, **kw: type("R", (), {"x": np.array([1e6, 0, 0, 0, 0, 0.0])})(), max_iterations=3).fit(
            ref, tba, inlier, transform=t6)


# ---- the recorded runs of the reference --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["f32", "f64"])
def test_iterations_follow_the_reference(case):
    """Device sums + host solve, iterated as ``_iterate_method`` iterates from the recorded centroid, against every matrix and statistic
    the reference's driver went through with ``least_squares``: within 10 x the recorded ``solve_gap``."""
    from xdem_amd import _lib, coreg, rigid

    g = golden()
    ref, tba, inlier, t6 = g[f"{case}_ref"], g[f"{case}_tba"], g[f"{case}_inlier"], tuple(g[f"{case}_transform"])
    cen = tuple(g[f"{case}_centroid"])
    tol = 10 * float(g["solve_gap"])
    ctx = _lib.default_context()
    for rule in range(4):
        with ctx.option_scope("nk_nan_rule", rule), coreg.DhPlan(ref, tba, inlier) as plan:
            assert plan.n_valid == int(g[f"{case}_mask"].sum())
            for only_t, tag in ((False, ""), (True, ""), (False, "_tight"), (True, "_tight")):
                key = f"{case}_r{rule}_t{int(only_t)}{tag}"
                matrix = np.eye(4)
                for i, want in enumerate(g[f"{key}_matrices"]):
                    sums, cnt = rigid.lzd_normal(plan, t6, matrix, cen)
                    step = coreg.matrix_from_translations_rotations(*rigid.solve_normal(sums, only_t), use_degrees=False)
                    matrix = step @ matrix
                    print(key, i, "matrix gap", float(np.abs(matrix - want).max()), "allowed", tol)
                    assert np.abs(matrix - want).max() <= tol, (key, i)
                    assert abs(abs(step[:3, 3].sum()) - g[f"{key}_stats"][i]) <= 3 * tol


def test_fit_stops_where_the_reference_stops():
    """``LZD.fit`` on the recorded pair (every valid pixel): as many iterations as the reference's driver, its final matrix within the
    effect of the centroid's elevation (ours a float64 mean, upstream's a float32 nanmean: the rotation times their difference)."""
    from xdem_amd import coreg

    g = golden()
    for case in ("f32", "f64"):
        for tag, kw in (("", {}), ("_tight", {"tolerance": float(g["tight_tolerance"])})):
            key = f"{case}_r{decided('nk_nan_rule')}_t0{tag}"
            c = coreg.LZD(subsample=1, **kw).fit(g[f"{case}_ref"], g[f"{case}_tba"], g[f"{case}_inlier"], transform=tuple(g[f"{case}_transform"]))
            out = c.meta["outputs"]
            assert out["iterative"]["last_iteration"] == len(g[f"{key}_stats"]) >= (4 if tag else 3)
            assert out["random"]["subsample_final"] == int(g[f"{case}_mask"].sum())
            dz = abs(out["affine"]["centroid"][2] - g[f"{case}_centroid"][2])
            rot = np.abs(c.to_matrix()[:3, :3] - np.eye(3)).max()
            assert np.abs(c.to_matrix() - g[f"{key}_final"]).max() <= 10 * float(g["solve_gap"]) + 3 * rot * dz
            assert out["affine"]["shift_x"] == c.to_matrix()[0, 3] and c.centroid() == out["affine"]["centroid"]


def test_host_route_gets_the_six_arrays():
    """A minimiser that is not ``scipy.optimize.least_squares`` itself runs on the host over the six arrays, as ``_lzd_fit`` calls it.  Here
    it is least_squares behind a wrapper -- the same objective -- so every matrix of the run agrees with the device route's within 10 x
    the recorded ``solve_gap`` (least_squares' truncation)."""
    import scipy.optimize

    from xdem_amd import coreg

    g = golden()
    args = (g["f64_ref"], g["f64_tba"], g["f64_inlier"])
    seen = []

    def wrapped(fun, x0, **kw):
        seen.append(kw)
        return scipy.optimize.least_squares(fun, x0, **kw)

    for only_t in (False, True):
        a = coreg.LZD(only_translation=only_t, subsample=1).fit(*args, transform=tuple(g["f64_transform"]))
        b = coreg.LZD(only_translation=only_t, subsample=1, fit_minimizer=wrapped).fit(*args, transform=tuple(g["f64_transform"]))
        assert a._device_route() and not b._device_route() and seen[-1] == {"loss": "linear"}
        ma, mb = a.meta["outputs"]["iterative"]["matrices"], b.meta["outputs"]["iterative"]["matrices"]
        assert len(ma) == len(mb)
        for x, y in zip(ma, mb):
            assert np.abs(x - y).max() <= 10 * float(g["solve_gap"])


# ---- the regrid ---------------------------------------------------------------------------------------------------------------------
def test_regrid_golden_matrices_bit_for_bit():
    from xdem_amd import coreg

    g = golden()
    for k in range(int(g["regrid_n"])):
        dem, matrix, t6 = g[str(g[f"regrid{k}_dem_key"])], g[f"regrid{k}_matrix"], tuple(g[f"regrid{k}_transform"])
        cen = None if np.isnan(g[f"regrid{k}_centroid"][0]) else tuple(g[f"regrid{k}_centroid"])
        got, t = coreg.apply_matrix(dem, matrix, centroid=cen, transform=t6)
        want, n_first = rigid_oracle.regrid(dem, t6, matrix, cen)
        assert t == t6 and got.dtype == dem.dtype and np.array_equal(got, want, equal_nan=True), k
        inv, _ = coreg.apply_matrix(dem, matrix, invert=True, centroid=cen, transform=t6)
        assert np.array_equal(inv, rigid_oracle.regrid(dem, t6, coreg.invert_matrix(matrix), cen)[0],
                              equal_nan=True), k


@pytest.mark.parametrize("shape,dtype_name", [(s, d) for s in SHAPES for d in ("float32", "float64")] + [(BIG, "float32")])
def test_regrid_shapes_bit_for_bit(shape, dtype_name):
    from xdem_amd import coreg

    g = golden()
    _, tba, _, t6 = _pair(*shape, dtype_name)
    x, y = rigid_oracle.pixel_xy(t6, *np.mgrid[0:shape[0], 0:shape[1]])
    cen = (float(x.mean()), float(y.mean()), float(np.nanmean(tba)))
    ks = range(int(g["regrid_n"])) if shape != BIG else [1]
    for k in ks:
        matrix = g[f"regrid{k}_matrix"]
        got, _ = coreg.apply_matrix(tba, matrix, centroid=cen, transform=t6)
        want, _ = rigid_oracle.regrid(tba, t6, matrix, cen)
        assert np.array_equal(got, want, equal_nan=True), (shape, k)


def test_apply_matrix_translation_cases():
    from xdem_amd import coreg

    _, tba, _, t6 = _pair(67, 129, "float32")
    m = coreg.matrix_from_translations_rotations(12.0, -7.0, 2.0)
    got, t = coreg.apply_matrix(tba, m, transform=t6)
    assert t == t6 and np.array_equal(got, coreg.apply_translation(tba, 12.0, -7.0, 2.0, (10.0, 10.0)), equal_nan=True)
    got, t = coreg.apply_matrix(tba, m, resample=False, transform=t6)
    assert t == (10.0, 0.0, 1012.0, 0.0, -10.0, 4993.0) and np.array_equal(got, tba + np.float32(2.0), equal_nan=True)


# ---- the step ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _synthetic():
    """A 400 x 500 terrain at 20 m and the same terrain seen through upstream's synthetic misalignment (20, 5, 0.1 | 0.1, 0.05, 0.01
    degrees) about the lower-left corner (test_coreg_rigid__synthetic, tests/test_coreg/test_affine.py:355-415)."""
    from xdem_amd import coreg

    H, W, res = 400, 500, 20.0
    t6 = (res, 0.0, 440000.0, 0.0, -res, 8670000.0)
    x, y = rigid_oracle.pixel_xy(t6, *np.mgrid[0:H, 0:W])
    u, v = x - t6[2], y - (t6[5] - H * res)
    ref = (600.0 + 250.0 * np.sin(u / 1700.0) * np.cos(v / 1300.0) + 120.0 * np.sin((u + 2 * v) / 900.0) + 40.0 * np.cos((2 * u - v) / 350.0)
           + 0.01 * u).astype(np.float32)
    params = (20, 5, 0.1, 0.1, 0.05, 0.01)
    matrix = coreg.matrix_from_translations_rotations(*params)
    cen = (t6[2], t6[5] - H * res, float(np.nanmean(ref)))
    tba, _ = coreg.apply_matrix(ref, matrix, centroid=cen, transform=t6)
    return ref, tba, t6, params, matrix, cen


def _about(matrix, c_from, c_to):
    """The matrix of the same transform written about another centroid: T(-c_to) T(c_from) M T(-c_from) T(c_to)."""
    out = np.array(matrix, dtype=np.float64)
    d = np.asarray(c_to, dtype=np.float64) - np.asarray(c_from, dtype=np.float64)
    out[:3, 3] = matrix[:3, 3] + (matrix[:3, :3] - np.eye(3)) @ d
    return out


def test_recovers_a_synthetic_rigid_misalignment():
    """``LZD().fit_and_apply`` recovers the inverse of upstream's synthetic misalignment within 0.5 pixel and 0.02 degrees and removes
    more than 95 % of the variance of dh (the reference's tolerances).  The fit's matrix is about the fit's centroid and the synthetic
    one about the lower-left corner: both are written about the same centroid before their translations are compared."""
    from xdem_amd import coreg

    ref, tba, t6, params, matrix, cen = _synthetic()
    c = coreg.LZD()
    aligned, _ = c.fit_and_apply(ref, tba, subsample=50000, random_state=42, transform=t6)
    fit = _about(c.to_matrix(), c.centroid(), cen)
    back = coreg.translations_rotations_from_matrix(coreg.invert_matrix(fit))
    print("recovered", back, "iterations", c.meta["outputs"]["iterative"]["last_iteration"])
    assert np.allclose(params[:3], back[:3], atol=0.5 * 20.0)
    assert np.allclose(params[3:], back[3:], atol=2 * 10e-3)
    init_dh, dh = (ref - tba).astype(np.float64), (ref - aligned).astype(np.float64)
    print("variance of dh before", np.nanvar(init_dh), "after", np.nanvar(dh))
    assert np.nanvar(dh) < 0.05 * np.nanvar(init_dh)
    assert c.meta["outputs"]["random"]["subsample_final"] == 50000
    only_t = coreg.LZD(only_translation=True).fit(ref, tba, subsample=50000, random_state=42, transform=t6)
    assert np.array_equal(only_t.to_matrix()[:3, :3], np.eye(3)) and only_t.to_rotations() == (0.0, 0.0, 0.0)


def test_pipeline_and_coregister_3d():
    from xdem_amd import coreg
    from xdem_amd.dem import DEM

    ref, tba, t6, params, matrix, cen = _synthetic()
    pipe = coreg.NuthKaab() + coreg.LZD()
    out, t = pipe.fit_and_apply(ref, tba, subsample=50000, random_state=42, transform=t6)
    assert t == t6 and pipe.is_affine
    assert np.array_equal(pipe.to_matrix(), pipe.pipeline[1].to_matrix() @ pipe.pipeline[0].to_matrix())
    assert np.any(pipe.pipeline[1].to_matrix()[:3, :3] != np.eye(3))
    assert np.nanvar((ref - out).astype(np.float64)) < 0.05 * np.nanvar((ref - tba).astype(np.float64))
    again, _ = pipe.apply(tba, transform=t6)
    assert np.array_equal(again, out, equal_nan=True)
    aligned = DEM(tba, t6).coregister_3d(DEM(ref, t6), coreg.LZD(subsample=50000), random_state=42)
    assert aligned.transform == t6 and aligned.data.dtype == np.float32
    assert np.nanvar((ref - aligned.data).astype(np.float64)) < 0.05 * np.nanvar((ref - tba).astype(np.float64))
