"""Host-side contract of ``xdem_amd.coreg.LZD`` / ``apply_matrix`` and the CPU oracle (no GPU), against what
tools/gen_golden_lzd.py recorded from the reference's own functions (tests/golden/lzd_golden.npz, signatures_lzd.json):
the matrix helpers, the signatures, the errors raised before a device is asked for, and tests/rigid_oracle.py -- its point transform, its
LZD iterations and its regrid -- against the reference's ``_apply_matrix_pts_arr``, ``_iterate_method(_lzd_iteration_step)`` and
``_iterate_affine_regrid_small_rotations``."""
import functools
import inspect
import json
import os

import numpy as np
import pytest

import rigid_oracle
from conftest import GOLDEN

SIG = json.load(open(os.path.join(GOLDEN, "signatures_lzd.json")))["coreg"]
EPS = 2.0 ** -52


@functools.lru_cache(maxsize=None)
def golden():
    return dict(np.load(os.path.join(GOLDEN, "lzd_golden.npz")))


# ---- signatures -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SIG))
def test_reference_parameters_are_mirrored(name):
    from xdem_amd import coreg

    obj = coreg
    for part in name.split("."):
        obj = getattr(obj, part)
    mine = list(inspect.signature(obj).parameters.items())
    names = [n for n, _ in mine]
    pos = -1
    for rec in SIG[name]:
        if rec["kind"] in ("VAR_KEYWORD", "VAR_POSITIONAL"):
            continue
        assert rec["name"] in names, f"{name}: parameter '{rec['name']}' of the reference is missing"
        p = dict(mine)[rec["name"]]
        assert names.index(rec["name"]) > pos, f"{name}: '{rec['name']}' is out of the reference's order"
        pos = names.index(rec["name"])
        if rec["default"] == "<required>":
            assert p.default is inspect.Parameter.empty, f"{name}: '{rec['name']}' must stay required"
        elif rec["default"] == "<object>":
            assert p.default is not inspect.Parameter.empty
        else:
            assert p.default == rec["default"], f"{name}: default of '{rec['name']}' is {p.default!r}, reference {rec['default']!r}"


def test_constructor_meta_and_defaults():
    import scipy.optimize

    from xdem_amd import coreg

    c = coreg.LZD()
    assert c.meta["inputs"]["fitorbin"]["fit_minimizer"] is scipy.optimize.least_squares
    assert c.meta["inputs"]["fitorbin"]["fit_loss_func"] == "linear"
    assert c.meta["inputs"]["iterative"] == {"max_iterations": 200, "tolerance": 0.01}
    assert c.meta["inputs"]["random"]["subsample"] == 5e5
    assert c.meta["inputs"]["affine"]["only_translation"] is False
    assert c.is_affine and c.centroid() is None
    assert isinstance(c + coreg.NuthKaab(), coreg.CoregPipeline)


# ---- matrix helpers -----------------------------------------------------------------------------------------------------------------
def test_helper_matrices_match_the_reference():
    from xdem_amd import coreg

    g = golden()
    for k, p in enumerate(g["helper_params"]):
        m = coreg.matrix_from_translations_rotations(*p)
        want = g["helper_matrix"][k]
        # computed elementwise by the reference: the translations, the last row
        assert np.array_equal(m[:, 3], want[:, 3]) and np.array_equal(m[3], want[3])
        # Rz @ Ry @ Rx: entries are sums of at most 9 products of sines and cosines, |entry| <= 1
        assert np.abs(m[:3, :3] - want[:3, :3]).max() <= 16 * EPS
        mr = coreg.matrix_from_translations_rotations(*p[:3], *np.deg2rad(p[3:]), use_degrees=False)
        assert np.abs(mr - g["helper_matrix_rad"][k]).max() <= 16 * EPS
        tmax = max(1.0, np.abs(p[:3]).max())
        assert np.abs(coreg.invert_matrix(want) - g["helper_inverse"][k]).max() <= 64 * EPS * tmax   # SVD, then R^T t
        back = coreg.translations_rotations_from_matrix(want)
        assert np.array_equal(back[:3], g["helper_params_back"][k][:3])
        assert np.abs(np.array(back[3:]) - g["helper_params_back"][k][3:]).max() <= 1e-12   # degrees, through arcsin / arctan2
        assert np.allclose(back[3:], p[3:], atol=1e-10)
        v = coreg._make_matrix_valid(want + 1e-9)
        assert np.array_equal(v[3], [0, 0, 0, 1]) and np.allclose(v[:3, :3].T @ v[:3, :3], np.eye(3), atol=1e-14)


def test_helper_errors():
    from xdem_amd import coreg

    bad = np.eye(4)
    bad[3, 0] = 1.0
    with pytest.raises(ValueError, match="Not affine"):
        coreg.invert_matrix(bad)
    bad = np.eye(4)
    bad[0, 0] = 2.0
    with pytest.raises(ValueError, match="Not a rigid transform"):
        coreg.invert_matrix(bad)
    with pytest.raises(ValueError, match="Matrix is not orthogonal"):
        coreg.translations_rotations_from_matrix(bad)


def test_oracle_point_transform_matches_the_reference():
    g = golden()
    pts, cen = g["helper_points"], tuple(g["helper_centroid"])
    from xdem_amd import coreg

    for k, m in enumerate(g["helper_matrix"]):
        for mat, want in ((m, g["helper_applied"][k]), (coreg.invert_matrix(m), g["helper_applied_inv"][k])):
            got = np.array(rigid_oracle.apply_pts(mat, cen, *pts))
            # four products of magnitude <= |coordinate| + |translation| summed in another order than BLAS's, then the centroid added
            scale = np.abs(pts).max() + np.abs(cen).max() + np.abs(m[:3, 3]).max()
            assert np.abs(got - want).max() <= 16 * EPS * scale


# ---- errors raised without a device ------------------------------------------------------------------------------------------------
def test_errors_without_a_device():
    from xdem_amd import coreg

    dem = np.zeros((8, 9), dtype=np.float32)
    with pytest.raises(NotImplementedError, match="initial_shift"):
        coreg.LZD(initial_shift=(1, 2))
    with pytest.raises(TypeError, match="fit_minimizer"):
        coreg.LZD(fit_minimizer=3)
    with pytest.raises(NotImplementedError, match="Weights have not yet been implemented"):
        coreg.LZD().fit(dem, dem, weights=dem, resolution=1.0)
    with pytest.raises(NotImplementedError, match="bias_vars"):
        coreg.LZD().fit(dem, dem, bias_vars={"a": dem}, resolution=1.0)
    with pytest.raises(AssertionError, match="fit"):
        coreg.LZD().apply(dem, resolution=1.0)
    fitted = coreg.LZD()
    fitted.meta["outputs"]["affine"] = {"matrix": coreg.matrix_from_translations_rotations(1, 2, 3, 0.1, 0.2, 0.3), "centroid": (0.0, 0.0, 0.0)}
    with pytest.raises(NotImplementedError, match="Option `resample=False` not supported by"):
        fitted.apply(dem, resample=False, resolution=1.0)
    with pytest.raises(NotImplementedError, match="resampling"):
        fitted.apply(dem, resampling="cubic", resolution=1.0)
    assert np.allclose(fitted.to_rotations(), (0.1, 0.2, 0.3)) and fitted.to_translations() == (1.0, 2.0, 3.0)
    assert np.allclose(fitted.to_rotations(return_degrees=False), np.deg2rad((0.1, 0.2, 0.3)))
    t6 = (1.0, 0.0, 0.0, 0.0, -1.0, 8.0)
    with pytest.raises(ValueError, match="Input DEM has all nans."):
        coreg.apply_matrix(np.full((4, 4), np.nan), np.eye(4), transform=t6)
    with pytest.raises(NotImplementedError, match="20 degrees"):
        coreg.apply_matrix(dem + 1, coreg.matrix_from_translations_rotations(alpha3=25.0), transform=t6)
    with pytest.raises(NotImplementedError, match="resampling"):
        coreg.apply_matrix(dem + 1, coreg.matrix_from_translations_rotations(alpha3=2.0), resampling="cubic", transform=t6)
    out, t = coreg.apply_matrix(dem + 1, coreg.matrix_from_translations_rotations(t3=2.5), transform=t6)   # z only: no device needed
    assert out.dtype == np.float32 and np.array_equal(out, dem + np.float32(3.5)) and t == t6


# ---- the oracle against the reference's recorded runs ------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["f32", "f64"])
@pytest.mark.parametrize("only_t", [False, True])
def test_oracle_iterations_follow_the_reference(case, only_t):
    """The oracle's six arrays with a float64 lstsq, iterated as ``_iterate_method`` iterates, against the recorded matrices and
    statistics of the reference's driver with ``least_squares``: within 10 x ``solve_gap`` (least_squares stops on ftol = 1e-8: the
    recorded gap is its truncation)."""
    from xdem_amd import coreg

    g = golden()
    ref, tba, mask, t6 = g[f"{case}_ref"], g[f"{case}_tba"], g[f"{case}_mask"], tuple(g[f"{case}_transform"])
    gradx, grady = rigid_oracle.gradient_planes(ref, abs(t6[0]), abs(t6[4]))
    # the recorded centroid is upstream's: nanmean in the raster dtype (pairwise float32 sums for float32 rasters), ours sums in float64
    cen = rigid_oracle.centroid(tba, mask, t6)
    assert np.allclose(cen[:2], g[f"{case}_centroid"][:2], rtol=1e-13, atol=0)
    assert abs(cen[2] - g[f"{case}_centroid"][2]) <= (2.0 ** -24 * np.log2(mask.sum()) if case == "f32" else 1e-13) * abs(cen[2])
    cen = tuple(g[f"{case}_centroid"])   # (the iterations are compared on the centroid the reference's run used)
    tol = 10 * float(g["solve_gap"])
    for rule in range(4):
        for tag, stop in (("", 0.01), ("_tight", float(g["tight_tolerance"]))):
            key = f"{case}_r{rule}_t{int(only_t)}{tag}"
            matrix = np.eye(4)
            for i, want in enumerate(g[f"{key}_matrices"]):
                arr = rigid_oracle.lzd_arrays(ref, tba, gradx, grady, mask, t6, matrix, cen, rule)
                step = coreg.matrix_from_translations_rotations(*rigid_oracle.lstsq_step(arr, only_t), use_degrees=False)
                matrix = step @ matrix
                assert np.abs(matrix - want).max() <= tol, (key, i, np.abs(matrix - want).max())
                assert abs(abs(step[:3, 3].sum()) - g[f"{key}_stats"][i]) <= 3 * tol
            assert np.array_equal(g[f"{key}_final"], g[f"{key}_matrices"][-1])
            # the recorded run stopped by upstream's rule: i > 1 and stat < tolerance (the tight runs go past iteration 3, so the
            # statistics before the last one are there to be at or above the tolerance)
            stats = g[f"{key}_stats"]
            assert len(stats) >= (4 if tag else 3) and stats[-1] < stop and all(s >= stop for s in stats[2:-1])


def test_normal_equations_give_the_lstsq_step():
    """The 29 sums solved after diagonal scaling (the product's host solve) against lstsq on the design matrix."""
    from xdem_amd import rigid

    g = golden()
    ref, tba, mask, t6 = g["f64_ref"], g["f64_tba"], g["f64_mask"], tuple(g["f64_transform"])
    gradx, grady = rigid_oracle.gradient_planes(ref, abs(t6[0]), abs(t6[4]))
    cen = rigid_oracle.centroid(tba, mask, t6)
    arr = rigid_oracle.lzd_arrays(ref, tba, gradx, grady, mask, t6, np.eye(4), cen, 0)
    sums, _ = rigid_oracle.normal_sums(arr)
    for only_t in (False, True):
        p, q = rigid.solve_normal(sums, only_t), rigid_oracle.lstsq_step(arr, only_t)
        assert np.abs(p - q).max() <= 1e-9 * np.abs(q).max()


def test_oracle_regrid_follows_the_reference():
    """Oracle regrid against the recorded ``_iterate_affine_regrid_small_rotations``: the pixels within rounding of the 1e-4 res
    threshold (which BLAS's summation order may switch between the value of iteration 1 and of iteration 5) stay below 1 %; on the others
    the NaN pattern is the reference's and the values lie within 4 x the gap recorded at generation."""
    from xdem_amd import coreg

    g = golden()
    assert float(g["regrid_flip_share"]) < 0.01
    flipped = total = 0
    partial = False
    for k in range(int(g["regrid_n"])):
        dem, matrix, t6 = g[str(g[f"regrid{k}_dem_key"])], g[f"regrid{k}_matrix"], tuple(g[f"regrid{k}_transform"])
        cen = None if np.isnan(g[f"regrid{k}_centroid"][0]) else tuple(g[f"regrid{k}_centroid"])
        got, n_first, near = rigid_oracle.regrid(dem, t6, matrix, cen, details=True)
        want = g[f"regrid{k}_out"]
        assert got.dtype == want.dtype == dem.dtype and n_first == int(g[f"regrid{k}_n_first"])
        partial = partial or 0 < n_first < dem.size
        flipped += int(near.sum())
        total += near.size
        assert np.array_equal(np.isnan(got[~near]), np.isnan(want[~near]))
        d = np.abs(got.astype(np.float64) - want.astype(np.float64))[~near]
        assert not np.isfinite(d).any() or np.nanmax(d) <= 4 * float(g["regrid_gap"]), (k, np.nanmax(d))
        assert np.isfinite(want).sum() > 0.6 * want.size
    assert partial and flipped / total < 0.01


def test_oracle_point_taps_are_the_shifted_taps():
    """At the positions of a whole-grid shift the point taps are ``nuthkaab_oracle.bilinear_shifted``, rule by rule."""
    import nuthkaab_oracle

    g = golden()
    img = g["f32_tba"]
    H, W = img.shape
    rows, cols = np.mgrid[0:H, 0:W].astype(np.float64)
    for rule in range(4):
        for dr, dc in ((0.0, 0.0), (0.37, -1.6), (-2.0, 3.0), (1.5, 0.25)):
            want = nuthkaab_oracle.bilinear_shifted(img, dr, dc, rule)
            assert np.array_equal(rigid_oracle.point_taps(img, rows + dr, cols + dc, rule), want, equal_nan=True), (rule, dr, dc)
    assert np.isnan(rigid_oracle.point_taps(img, np.array([np.nan, 1e300, -1e300, 3.0]), np.array([2.0, 2.0, 2.0, np.inf]), 0)).all()


def test_oracle_interpolation_is_scipys_as_upstream_calls_it():
    """``rigid_oracle.rgi_linear`` against SciPy's ``RegularGridInterpolator`` built as upstream builds it (the flipped y axis, the DEM as it
    is): the NaN pattern -- also exactly on nodes, where the cell SciPy picks decides which neighbour's nodata spreads -- and the values."""
    import scipy.interpolate

    rng = np.random.default_rng(5)
    H, W = 9, 11
    dem = rng.normal(size=(H, W))
    dem[rng.random((H, W)) < 0.15] = np.nan
    t6 = (2.0, 0.0, 100.0, 0.0, -3.0, 50.0)
    xs = rigid_oracle.pixel_xy(t6, np.zeros(W), np.arange(W))[0]
    ys = np.flip(rigid_oracle.pixel_xy(t6, np.arange(H), np.zeros(H))[1])   # ascending, as upstream's coords(grid=False) hands them over
    interp = scipy.interpolate.RegularGridInterpolator(points=(np.flip(ys, axis=0), xs), values=dem, method="linear", bounds_error=False)
    rows = np.concatenate([np.repeat(np.arange(H, dtype=np.float64), W), rng.uniform(-0.5, H - 0.5, 400), np.repeat(np.arange(H) + 0.5, W)[: W * (H - 1)]])
    cols = np.concatenate([np.tile(np.arange(W, dtype=np.float64), H), rng.uniform(-0.5, W - 0.5, 400), np.tile(np.arange(W, dtype=np.float64), H - 1)])
    x, y = rigid_oracle.pixel_xy(t6, rows, cols)
    want = interp((y, x))
    got = rigid_oracle.rgi_linear(dem, *rigid_oracle.xy_to_pixel(t6, x, y))
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert np.isfinite(want).sum() > 100 and np.nanmax(np.abs(got - want)) <= 64 * EPS * np.nanmax(np.abs(dem))
