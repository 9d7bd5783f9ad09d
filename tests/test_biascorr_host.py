"""Host logic of Deramp / VerticalShift / CoregPipeline (xdem_amd/biascorr.py) without the GPU: signatures against the reference's
(tests/golden/signatures_biascorr.json, written by tools/gen_golden_biascorr.py), the float64 solve of the polynomial moments and its
map back to raw pixel monomials, the pipeline's composition rules, and the errors upstream raises."""
import inspect
import json
import os
import warnings

import numpy as np
import pytest
import scipy.optimize

from conftest import GOLDEN

SIG = json.load(open(os.path.join(GOLDEN, "signatures_biascorr.json")))["coreg"]


@pytest.mark.parametrize("name", sorted(SIG))
def test_reference_parameters_are_mirrored(name):
    from xdem_amd import coreg

    cls, meth = name.split(".")
    fn = getattr(getattr(coreg, cls), meth)
    mine = list(inspect.signature(fn).parameters.items())
    names = [n for n, _ in mine]
    catch_all = any(p.kind is inspect.Parameter.VAR_KEYWORD for _, p in mine)
    pos = -1
    for rec in SIG[name]:
        if rec["kind"] in ("VAR_KEYWORD", "VAR_POSITIONAL"):
            continue
        if rec["name"] not in names:
            assert catch_all, f"{name}: parameter '{rec['name']}' of the reference is missing"
            continue
        i = names.index(rec["name"])
        assert i > pos, f"{name}: parameter '{rec['name']}' is out of order"
        pos = i
        p = mine[i][1]
        if rec["default"] == "<required>":
            assert p.default is inspect.Parameter.empty, f"{name}: '{rec['name']}' must stay required"
        elif rec["default"] == "<object>":
            assert p.default is not inspect.Parameter.empty
        else:
            assert p.default == rec["default"], f"{name}: default of '{rec['name']}' is {p.default!r}, reference {rec['default']!r}"


def _moments(x, y, dh, order, shape):
    """What xdemhip_dh_poly_moments returns, computed with NumPy."""
    from xdem_amd.biascorr import poly_norm

    cx, sx = poly_norm(shape[1])
    cy, sy = poly_norm(shape[0])
    u, v = (x - cx) / sx, (y - cy) / sy
    NA = 2 * order + 1
    M = np.array([[np.sum(u ** a * v ** b) for b in range(NA)] for a in range(NA)])
    R = np.array([[np.sum(dh * u ** i * v ** j) for j in range(order + 1)] for i in range(order + 1)])
    return M, R


@pytest.mark.parametrize("order", [0, 1, 2, 3, 4])
def test_back_transform_and_perr_match_lstsq_and_curve_fit(order):
    from xdem_amd.biascorr import polynomial_2d, solve_moments

    rng = np.random.default_rng(order)
    H, W = 40, 57
    n = 600
    flat = rng.choice(H * W, n, replace=False)
    y, x = np.divmod(flat, W)
    true = rng.normal(size=(order + 1) ** 2) * np.array([10.0 ** -(i + j) for i in range(order + 1) for j in range(order + 1)])
    dh = polynomial_2d((x, y), *true) + rng.normal(scale=0.1, size=n)
    M, R = _moments(x.astype(float), y.astype(float), dh, order, (H, W))
    params, perr = solve_moments(M, R, order, (H, W))
    # the surface: same as curve_fit from upstream's p0 = ones, and as a raw least-squares solve
    popt, pcov = scipy.optimize.curve_fit(polynomial_2d, np.array([x, y]), dh, p0=np.ones((order + 1) ** 2), absolute_sigma=True)
    A = np.stack([x.astype(float) ** i * y.astype(float) ** j for i in range(order + 1) for j in range(order + 1)], 1)
    scale = np.linalg.norm(A, axis=0)   # (columns scaled to unit norm: the raw monomials alone are too ill-conditioned from order 3 on)
    lst = np.linalg.lstsq(A / scale, dh, rcond=None)[0] / scale
    mine = polynomial_2d((x, y), *params)
    sse = lambda p: float(np.sum((dh - polynomial_2d((x, y), *p)) ** 2))
    assert sse(params) <= sse(popt) * (1 + 1e-9)
    assert np.max(np.abs(mine - polynomial_2d((x, y), *lst))) <= 1e-8 * (1 + np.max(np.abs(mine)))
    assert np.max(np.abs(mine - polynomial_2d((x, y), *popt))) <= 1e-4 * (1 + np.max(np.abs(mine)))
    # curve_fit's absolute_sigma covariance inv(A^T A); curve_fit forms it from raw monomials, which loses digits from order 3 on, so
    # the higher orders are held against the same matrix formed from unit-norm columns
    As = A / scale
    cov = np.linalg.inv(As.T @ As) / np.outer(scale, scale)
    np.testing.assert_allclose(perr, np.sqrt(np.diag(cov)), rtol=1e-6)
    if order <= 2:
        np.testing.assert_allclose(perr, np.sqrt(np.diag(pcov)), rtol=1e-5)


def test_rank_deficient_moments_take_the_minimum_norm_solution():
    """All points on one row: the Gram matrix is singular; the surface still fits the data points like curve_fit's."""
    from xdem_amd.biascorr import polynomial_2d, solve_moments

    rng = np.random.default_rng(3)
    H, W, order = 20, 60, 2
    x = np.arange(W, dtype=float)
    y = np.full(W, 7.0)
    dh = 0.3 + 0.01 * x - 2e-4 * x ** 2 + rng.normal(scale=0.01, size=W)
    M, R = _moments(x, y, dh, order, (H, W))
    params, perr = solve_moments(M, R, order, (H, W))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        popt, _ = scipy.optimize.curve_fit(polynomial_2d, np.array([x, y]), dh, p0=np.ones(9), absolute_sigma=True)
    assert np.all(np.isfinite(params))
    np.testing.assert_allclose(polynomial_2d((x, y), *params), polynomial_2d((x, y), *popt), atol=1e-5)


class _FakePlan:
    """Stand-in for DhPlan: a fixed number of valid pixels, records what the fit asks of it."""
    n_valid = 50
    log = []

    def __init__(self, ref, tba, inlier_mask=None, ctx=None):
        self.shape = np.shape(ref)
        self.n_selected = self.n_valid
        _FakePlan.log.append(("create", inlier_mask is not None))

    def subsample(self, ranks):
        self.n_selected = len(ranks)
        _FakePlan.log.append(("subsample", len(ranks)))
        return self.n_selected

    def median(self):
        return 2.5, self.n_selected

    def values(self, coords=True):
        dh = np.arange(self.n_selected, dtype=np.float32)
        if not coords:
            return dh
        return dh, np.arange(self.n_selected) % 10, np.arange(self.n_selected) // 10

    def close(self):
        pass

    __enter__ = lambda self: self
    __exit__ = lambda self, *a: False


def test_errors_mirror_upstream(monkeypatch):
    from xdem_amd import biascorr, coreg

    z = np.zeros((10, 10), dtype=np.float32)
    with pytest.raises(NotImplementedError, match="Weights have not yet been implemented"):
        coreg.Deramp().fit(z, z, weights=np.ones((10, 10)))
    with pytest.raises(NotImplementedError, match="Weights have not yet been implemented"):
        coreg.VerticalShift().fit(z, z, weights=np.ones((10, 10)))
    with pytest.raises(NotImplementedError, match='only "fit"'):
        coreg.Deramp(fit_or_bin="bin")
    with pytest.raises(NotImplementedError, match='only "fit"'):
        coreg.Deramp(fit_or_bin="bin_and_fit")
    with pytest.raises(ValueError, match="fit_or_bin"):
        coreg.Deramp(fit_or_bin="nope")
    with pytest.raises(NotImplementedError, match="initial_shift"):
        coreg.VerticalShift(initial_shift=(1.0, 2.0))
    with pytest.raises(AssertionError, match=r"\.fit\(\) does not seem to have been called yet"):
        coreg.CoregPipeline([coreg.VerticalShift()]).apply(z, resolution=1.0)
    with pytest.raises(ValueError, match="Incompatible add type: <class 'int'>. Expected 'Coreg' subclass"):
        coreg.NuthKaab() + 3
    with pytest.raises(ValueError, match="Incompatible add type"):
        coreg.Deramp() + object()
    monkeypatch.setattr(biascorr, "DhPlan", _FakePlan)
    # fewer valid points than parameters: the TypeError curve_fit raises
    monkeypatch.setattr(_FakePlan, "n_valid", 8)
    with pytest.raises(TypeError, match="N=9 must not exceed func output vector length M=8"):
        coreg.Deramp(subsample=1).fit(z, z)
    monkeypatch.setattr(_FakePlan, "n_valid", 0)
    for m in (coreg.Deramp(), coreg.VerticalShift()):
        with pytest.raises(ValueError, match="There is no valid points common to the input"):
            m.fit(z, z)
    with pytest.raises(NotImplementedError, match="poly_order 0..5"):
        coreg.Deramp(poly_order=6).fit(z, z)


def test_host_routes_call_the_callables_as_upstream(monkeypatch):
    """A custom vshift_reduc_func gets dh; a custom fit_optimizer gets xdata = [cols, rows] (int64), ydata = dh, p0 = ones."""
    from xdem_amd import biascorr, coreg

    monkeypatch.setattr(biascorr, "DhPlan", _FakePlan)
    monkeypatch.setattr(_FakePlan, "n_valid", 50)
    seen = {}

    def reduc(dh):
        seen["dh"] = dh
        return np.float32(4.25)

    vs = coreg.VerticalShift(vshift_reduc_func=reduc).fit(np.zeros((5, 10)), np.zeros((5, 10)))
    assert vs.meta["outputs"]["affine"] == {"shift_z": 4.25}
    assert seen["dh"].dtype == np.float32 and seen["dh"].shape == (50,)   # (dh in the plan's value dtype, one value per pixel)
    assert coreg.VerticalShift().fit(np.zeros((5, 10)), np.zeros((5, 10))).meta["outputs"]["affine"]["shift_z"] == 2.5

    def opt(f, xdata, ydata, sigma, absolute_sigma, p0, **kw):
        seen.update(xdata=xdata, ydata=ydata, p0=p0, sigma=sigma, absolute_sigma=absolute_sigma)
        return (np.arange(4.0), np.eye(4))

    d = coreg.Deramp(poly_order=1, fit_optimizer=opt, subsample=20).fit(np.zeros((5, 10)), np.zeros((5, 10)), random_state=1)
    assert seen["xdata"].shape == (2, 20) and seen["xdata"].dtype == np.int64 and seen["p0"].tolist() == [1.0] * 4
    assert seen["sigma"] is None and seen["absolute_sigma"] is True
    assert d.meta["outputs"]["fitorbin"]["fit_params"].tolist() == [0.0, 1.0, 2.0, 3.0]
    assert d.meta["outputs"]["random"]["subsample_final"] == 20 and ("subsample", 20) in _FakePlan.log


def test_pipeline_composition(monkeypatch):
    """fit: every step on the previous step's apply output, the last step not applied, transform / subsample / random_state / inlier
    mask handed on; apply: the steps' applies in order; to_matrix: product of affine steps, a non-affine step raises."""
    from xdem_amd import coreg

    calls = []

    def make(cls, tag, dz):
        def fit(self, reference_elev, to_be_aligned_elev, inlier_mask=None, bias_vars=None, weights=None, subsample=None, transform=None,
                crs=None, area_or_point=None, z_name=None, random_state=None, resolution=None, **kw):
            calls.append(("fit", tag, float(to_be_aligned_elev[0, 0]), transform, subsample, random_state, inlier_mask is not None,
                          resolution))
            self.meta["outputs"]["affine"] = {"shift_x": 0.0, "shift_y": 0.0, "shift_z": dz}
            self.meta["outputs"]["fitorbin"] = {"fit_params": np.zeros(9)}
            return self

        def apply(self, elev, resolution=None, resample=True, *, bias_vars=None, resampling="bilinear", transform=None, crs=None,
                  z_name="z"):
            calls.append(("apply", tag, float(elev[0, 0]), transform, resolution))
            out = elev + dz
            return out if transform is None else (out, transform)

        monkeypatch.setattr(cls, "fit", fit)
        monkeypatch.setattr(cls, "apply", apply)

    make(coreg.VerticalShift, "vs", 1.0)
    make(coreg.NuthKaab, "nk", 10.0)
    make(coreg.Deramp, "dr", 100.0)
    ref = np.zeros((3, 4))
    tba = np.zeros((3, 4))
    pipe = coreg.VerticalShift() + coreg.NuthKaab() + coreg.Deramp()
    assert isinstance(pipe, coreg.CoregPipeline) and len(list(pipe)) == 3 and repr(pipe).startswith("Pipeline: [")
    tr = (2.0, 0.0, 0.0, 0.0, -2.0, 10.0)
    mask = np.ones((3, 4), dtype=bool)
    pipe.fit(ref, tba, inlier_mask=mask, transform=tr, random_state=5)
    assert calls == [("fit", "vs", 0.0, tr, None, 5, True, None), ("apply", "vs", 0.0, tr, None),
                     ("fit", "nk", 1.0, tr, None, 5, True, None), ("apply", "nk", 1.0, tr, None),
                     ("fit", "dr", 11.0, tr, None, 5, True, None)]
    calls.clear()
    out, t = pipe.apply(tba, transform=tr)
    assert t == tr and out[0, 0] == 111.0 and [c[1] for c in calls] == ["vs", "nk", "dr"]
    calls.clear()
    # resolution= instead of a transform: arrays only
    out = pipe.fit_and_apply(ref, tba, fit_kwargs={"resolution": 2.0})
    assert out[0, 0] == 111.0 and calls[0][-1] == 2.0 and calls[-1][-1] == 2.0
    # to_matrix
    aff = coreg.VerticalShift() + coreg.NuthKaab()
    aff.fit(ref, tba, resolution=1.0)
    assert aff.is_affine and aff.to_matrix()[2, 3] == 11.0
    assert not pipe.is_affine
    with pytest.raises(NotImplementedError):
        pipe.to_matrix()
    # copy is deep
    cp = pipe.copy()
    assert cp.pipeline[0] is not pipe.pipeline[0] and cp.pipeline[0].meta.keys() == pipe.pipeline[0].meta.keys()


def test_pipeline_subsample_warning_and_initial_shift():
    from xdem_amd import coreg

    nk = coreg.NuthKaab(initial_shift=(1.0, 2.0))
    pipe = nk + coreg.VerticalShift()
    assert "initial_shift" not in nk.meta["inputs"]["affine"]
    def stubbed(steps):
        calls = []
        for step in steps:   # (no GPU: the steps only record that they ran)
            step.fit = lambda *a, _c=calls, **k: _c.append(k.get("subsample"))
            step.apply = lambda *a, **k: np.zeros((2, 2))
        return coreg.CoregPipeline(steps), calls

    pipe2, calls = stubbed([coreg.NuthKaab(subsample=1000), coreg.Deramp()])
    with pytest.warns(UserWarning, match="Subsample argument passed to fit\\(\\) will override non-default"):
        pipe2.fit(np.zeros((2, 2)), np.zeros((2, 2)), subsample=0.5, resolution=1.0)
    assert calls == [0.5, 0.5]
    # every step at its default subsample: fit(subsample=...) overrides nothing, no warning
    pipe3, calls = stubbed([coreg.NuthKaab(), coreg.Deramp(), coreg.VerticalShift()])
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        pipe3.fit(np.zeros((2, 2)), np.zeros((2, 2)), subsample=0.5, resolution=1.0)
    assert calls == [0.5, 0.5, 0.5]


def test_coregister_3d_accepts_the_new_methods(monkeypatch):
    import xdem_amd
    from xdem_amd import coreg

    seen = []

    def fit(self, ref, tba, inlier_mask=None, resolution=None, **kw):
        seen.append(("fit", type(self).__name__, resolution))
        self.meta["outputs"]["affine"] = {"shift_z": 1.0}
        self.meta["outputs"]["fitorbin"] = {"fit_params": np.zeros(9)}
        return self

    def apply(self, elev, resolution=None, resample=True, *, transform=None, **kw):
        seen.append(("apply", type(self).__name__, resample))
        return (elev + 1, transform)

    for cls in (coreg.Deramp, coreg.VerticalShift, coreg.CoregPipeline):
        monkeypatch.setattr(cls, "fit", fit)
        monkeypatch.setattr(cls, "apply", apply)
    a = xdem_amd.DEM(np.zeros((5, 6), dtype=np.float32), transform=(2.0, 0.0, 0.0, 0.0, -2.0, 10.0))
    b = xdem_amd.DEM(np.ones((5, 6), dtype=np.float32), transform=(2.0, 0.0, 0.0, 0.0, -2.0, 10.0))
    for m in (coreg.Deramp(), coreg.VerticalShift(), coreg.CoregPipeline([coreg.Deramp()])):
        out = a.coregister_3d(b, m, resample=False)
        assert np.all(out.data == 1.0) and seen[-2] == ("fit", type(m).__name__, (2.0, 2.0)) and seen[-1][2] is False


@pytest.mark.parametrize("first", ["biascorr", "coreg"])
def test_coreg_and_biascorr_import_in_either_order(first):
    """coreg and biascorr share xdem_amd._coregbase and import each other nowhere lazily: either may be imported first."""
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    second = "coreg" if first == "biascorr" else "biascorr"
    code = (f"import xdem_amd.{first}, xdem_amd.{second}\n"
            "from xdem_amd import biascorr, coreg\n"
            "assert coreg.CoregPipeline is biascorr.CoregPipeline and coreg.Deramp is biascorr.Deramp\n"
            "assert isinstance(coreg.NuthKaab() + coreg.VerticalShift(), biascorr.CoregPipeline)\n")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join(p for p in (root, os.environ.get("PYTHONPATH")) if p))
    subprocess.run([sys.executable, "-c", code], cwd=root, env=env, check=True, timeout=300)


def test_nuthkaab_is_a_step(monkeypatch):
    """NuthKaab shares _Step with the other methods: ``+`` gives a two-step pipeline, and fit_and_apply hands
    ``fit_kwargs={"resolution": ...}`` on to apply."""
    from xdem_amd import coreg
    from xdem_amd._coregbase import _Step

    assert isinstance(coreg.NuthKaab(), _Step)
    pipe = coreg.NuthKaab() + coreg.Deramp()
    assert isinstance(pipe, coreg.CoregPipeline) and [type(s) for s in pipe] == [coreg.NuthKaab, coreg.Deramp]
    with pytest.raises(ValueError, match="Incompatible add type"):
        coreg.NuthKaab() + 1
    seen = {}
    monkeypatch.setattr(coreg, "nuth_kaab", lambda ref, tba, inlier, res, **kw: ((1.0, 2.0, 3.0), 7))

    def fake_translation(elev, sx, sy, sz, res, resample=True, ctx=None):
        seen["apply"] = (sx, sy, sz, res, resample)
        return elev + sz

    monkeypatch.setattr(coreg, "apply_translation", fake_translation)
    out = coreg.NuthKaab().fit_and_apply(np.zeros((3, 4), np.float32), np.ones((3, 4), np.float32), fit_kwargs={"resolution": (2.0, 4.0)})
    assert seen["apply"] == (-1.0, -2.0, 3.0, (2.0, 4.0), True) and np.all(out == 4.0)


def test_nuth_kaab_closes_the_plan_when_the_draw_fails(monkeypatch):
    from xdem_amd import coreg

    closed = []

    class _NKPlan:
        n_valid = 100

        def __init__(self, *args, **kwargs):
            pass

        def subsample(self, ranks):
            raise RuntimeError("draw failed")

        def close(self):
            closed.append(True)

    monkeypatch.setattr(coreg, "NKPlan", _NKPlan)
    with pytest.raises(RuntimeError, match="draw failed"):
        coreg.nuth_kaab(np.zeros((10, 10)), np.zeros((10, 10)), None, (1.0, 1.0), subsample=0.5, random_state=0)
    assert closed == [True]


# ---- the moments oracle of the device tests (tests/deramp_oracle.py) ---------------------------------------------------------------
def _pairwise_additions(n):
    """Additions a term passes through in np.sum over n contiguous values: 16 in one of the 8 accumulators of a 128-value block, 3 to
    combine them, one per level of the pairwise tree above the blocks; + 1 for the product that forms the term."""
    import math

    return 16 + 3 + max(0, math.ceil(math.log2(max(n / 128.0, 1.0)))) + 1


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("masked", [False, True])
def test_deramp_oracle_matches_numpy_moments_within_the_bound(dtype, masked):
    """The longdouble oracle against this module's float64 ``_moments`` (whose error the same bound covers: its coordinate is one
    division, its powers are correctly rounded ones), and the oracle's row-block and rank forms against its own whole-raster form."""
    import deramp_oracle as do

    H, W, order = 37, 61, 5
    ref, tba, inl = do.make_pair(H, W, dtype, seed=7, masked=masked)
    want = do.moments(ref, tba, inl, order)
    valid = do.valid_mask(ref, tba, inl)
    assert want.count == int(valid.sum()) and want.M[0, 0] == want.count and 0 < want.count < H * W
    y, x = np.nonzero(valid)
    M, R = _moments(x.astype(float), y.astype(float), (ref[valid] - tba[valid]).astype(np.float64), order, (H, W))
    bM, bR = do.moments_bound(want, _pairwise_additions(want.count))
    assert np.all(np.abs(M - want.M) <= bM) and np.all(np.abs(R - want.R) <= bR)
    # lower orders are the leading blocks
    low = do.moments(ref, tba, inl, 2)
    assert np.array_equal(low.M, do.sub(want, 2).M) and np.array_equal(low.R, do.sub(want, 2).R)
    # rows [r0, r1) with their offset = the whole raster with the other rows masked out
    r0, r1 = 11, 29
    rows_only = np.zeros((H, W), dtype=bool)
    rows_only[r0:r1] = True if inl is None else inl[r0:r1]
    a = do.moments(ref[r0:r1], tba[r0:r1], None if inl is None else inl[r0:r1], order, row_offset=r0, H_global=H)
    b = do.moments(ref, tba, rows_only, order)
    tiny = np.longdouble(2.0 ** -58)
    assert a.count == b.count and np.all(np.abs(a.M - b.M) <= tiny * b.magM) and np.all(np.abs(a.R - b.R) <= tiny * b.magR)
    # ranks: flatnonzero(valid)[unique ranks]
    ranks = np.array([5, 0, want.count - 1, 5, 17, 17, 400])
    picked = np.zeros(H * W, dtype=bool)
    picked[np.flatnonzero(valid)[np.unique(ranks)]] = True
    a = do.moments(ref, tba, inl, order, ranks=ranks)
    b = do.moments(ref, tba, picked.reshape(H, W), order)
    assert a.count == b.count == 5 and np.array_equal(a.M, b.M) and np.array_equal(a.R, b.R)


@pytest.mark.parametrize("num_cu", [64, 256, 304])
def test_deramp_count_moment_is_exact_on_every_tested_shape(num_cu):
    """The bound of M[0, 0] is below 0.5 on every moments shape of tests/test_deramp_routes_gpu.py, on either route a shape can take
    and for every device size: the device tests may ask for M[0, 0] == count exactly."""
    import deramp_oracle as do

    for H, W, vec in do.moments_shapes(num_cu):
        for route in {vec, False}:
            assert do.count_bound(H * W, do.additions_rows(H, W, route, num_cu)) < 0.5, (H, W, route)
    side, k_large = do.list_large_case(num_cu)
    assert k_large + 1000 <= 0.99 * side * side and do.list_grid(k_large, num_cu)[0] > 256
    for k in do.LIST_SMALL_K + (k_large,):
        assert do.count_bound(k, do.additions_list(k, num_cu)) < 0.5, k
    assert do.count_bound(side * side, do.additions_rows(side, side, True, num_cu)) < 0.5


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_deramp_oracle_bound_notices_one_dropped_pixel(dtype):
    """Dropping one valid pixel -- a corner, the centre, the last pixel of a row -- moves at least one entry of (M, R) by more than
    its bound: a kernel that loses a pixel cannot pass the device tests."""
    import deramp_oracle as do

    H, W, order = 40, 64, 5
    ref, tba, _ = do.make_pair(H, W, dtype, seed=11, nan_frac=0.0)
    want = do.moments(ref, tba, None, order)
    assert want.count == H * W
    bM, bR = do.moments_bound(want, do.additions_rows(H, W, True, 256))
    for r, c in ((0, 0), (H // 2, W // 2), (17, W - 1)):
        inl = np.ones((H, W), dtype=bool)
        inl[r, c] = False
        less = do.moments(ref, tba, inl, order)
        moved_m, moved_r = np.abs(less.M - want.M) > bM, np.abs(less.R - want.R) > bR
        assert less.count == want.count - 1 and (moved_m.any() or moved_r.any())
        # not the count alone: the right-hand side feels it too
        assert moved_m[0, 0] and moved_r[0, 0], (r, c)
