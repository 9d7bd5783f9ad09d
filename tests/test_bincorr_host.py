"""Host logic of BiasCorr / DirectionalBias / TerrainBias (xdem_amd/bincorr.py) without the GPU: constructor signatures and error
messages against the reference's (tests/golden/signatures_bincorr.json, bincorr_errors.json, written by
tools/gen_golden_bincorr.py), the meta layout, the pipeline's parsing of bias variables, the rotated coordinate, and the
refusals."""
import inspect
import json
import os

import numpy as np
import pytest
import scipy.optimize

from conftest import GOLDEN

SIG = json.load(open(os.path.join(GOLDEN, "signatures_bincorr.json")))["coreg"]
ERR = json.load(open(os.path.join(GOLDEN, "bincorr_errors.json")))


@pytest.mark.parametrize("name", sorted(SIG))
def test_reference_parameters_are_mirrored(name):
    from xdem_amd import coreg

    cls, meth = name.split(".")
    mine = list(inspect.signature(getattr(getattr(coreg, cls), meth)).parameters.items())
    theirs = SIG[name]
    assert [n for n, _ in mine] == [r["name"] for r in theirs]
    for (n, p), rec in zip(mine, theirs):
        if rec["default"] == "<required>":
            assert p.default is inspect.Parameter.empty, f"{name}: '{n}' must stay required"
        elif rec["default"] == "<object>":
            assert p.default is not inspect.Parameter.empty
        else:
            assert p.default == rec["default"] and type(p.default) is type(rec["default"]), f"{name}: default of '{n}' is {p.default!r}"


def _raises(key, fn):
    want = ERR[key]
    exc = {"ValueError": ValueError, "TypeError": TypeError}[want["type"]]
    with pytest.raises(exc) as info:
        fn()
    assert str(info.value) == want["message"]


def test_constructor_errors_are_the_references():
    from xdem_amd import coreg

    _raises("fit_or_bin", lambda: coreg.BiasCorr(fit_or_bin=True))
    _raises("fit_func", lambda: coreg.BiasCorr(fit_func="yay"))
    _raises("fit_optimizer", lambda: coreg.BiasCorr(fit_optimizer=3))
    _raises("bin_sizes", lambda: coreg.BiasCorr(fit_or_bin="bin", bin_sizes={"a": 1.5}))
    _raises("bin_statistic", lambda: coreg.BiasCorr(fit_or_bin="bin", bin_statistic="count"))
    _raises("bin_apply_method", lambda: coreg.BiasCorr(fit_or_bin="bin", bin_apply_method=1))


def test_variable_checks_are_the_references():
    from xdem_amd import bincorr, coreg

    z = np.zeros((4, 5), dtype=np.float32)
    b1 = coreg.BiasCorr(fit_or_bin="bin", bias_var_names=["v1"])
    _raises("wrong_number", lambda: b1.fit(z, z, bias_vars={"v1": z, "v2": z}))
    _raises("wrong_keys", lambda: b1.fit(z, z, bias_vars={"v2": z}))
    _raises("fit_none", lambda: b1.fit(z, z))
    _raises("fit_none", lambda: bincorr._bin_or_and_fit_nd("bin", b1.meta["inputs"]["fitorbin"], z, None))
    with pytest.raises(AssertionError, match="fit"):
        b1.apply(z, bias_vars={"v1": z})
    b1.meta["outputs"]["fitorbin"] = {"bin_dataframe": None}   # (as after a fit: the checks of apply come before any device work)
    _raises("apply_none", lambda: b1.apply(z))
    _raises("apply_keys", lambda: b1.apply(z, bias_vars={"v2": z}))


def test_meta_layout_of_the_three_classes():
    from xdem_amd import coreg, fit

    b = coreg.BiasCorr()
    assert b.meta["inputs"]["fitorbin"] == {"fit_func": fit.polynomial_1d, "fit_optimizer": fit.robust_norder_polynomial_fit,
                                            "bias_var_names": None, "fit_or_bin": "fit", "nd": None}
    assert b.meta["inputs"]["random"] == {"subsample": 1.0} and b.meta["inputs"]["specific"] == {} and b.meta["outputs"] == {}
    assert b._needs_vars is True and b._is_affine is False and b.is_affine is False
    b = coreg.BiasCorr(fit_or_bin="bin", bin_sizes={"a": 3, "b": [0, 1, 2]}, bin_apply_method="per_bin", bias_var_names=("a", "b"), subsample=0.5)
    assert b.meta["inputs"]["fitorbin"] == {"bin_sizes": {"a": 3, "b": [0, 1, 2]}, "bin_statistic": np.nanmedian, "bin_apply_method": "per_bin",
                                            "bias_var_names": ["a", "b"], "fit_or_bin": "bin", "nd": 2}
    assert b.meta["inputs"]["random"]["subsample"] == 0.5
    b = coreg.BiasCorr(fit_or_bin="bin_and_fit", fit_func=fit.polynomial_2d)
    assert set(b.meta["inputs"]["fitorbin"]) == {"fit_func", "fit_optimizer", "bin_sizes", "bin_statistic", "bias_var_names", "fit_or_bin", "nd"}
    assert b.meta["inputs"]["fitorbin"]["fit_optimizer"] is scipy.optimize.curve_fit
    d = coreg.DirectionalBias(angle=20)
    assert d.meta["inputs"]["specific"] == {"angle": 20} and d.meta["inputs"]["fitorbin"]["bias_var_names"] == ["angle"]
    assert d.meta["inputs"]["fitorbin"]["fit_or_bin"] == "bin_and_fit" and d.meta["inputs"]["fitorbin"]["fit_func"] is fit.sumsin_1d
    assert d.meta["inputs"]["fitorbin"]["fit_optimizer"] is fit.robust_nfreq_sumsin_fit and d.meta["inputs"]["fitorbin"]["bin_sizes"] == 100
    assert d._needs_vars is False and d.meta["inputs"]["fitorbin"]["nd"] == 1
    t = coreg.TerrainBias()
    assert t.meta["inputs"]["specific"] == {"terrain_attribute": "max_curvature"} and t._needs_vars is False
    assert t.meta["inputs"]["fitorbin"]["bias_var_names"] == ["max_curvature"] and t.meta["inputs"]["fitorbin"]["fit_or_bin"] == "bin"
    with pytest.raises(NotImplementedError, match="no matrix"):
        t.to_matrix()
    c = d.copy()
    c.meta["inputs"]["specific"]["angle"] = 5
    assert d.meta["inputs"]["specific"]["angle"] == 20


def test_deramp_stays_where_and_what_it_is():
    from xdem_amd import biascorr, bincorr, coreg

    assert coreg.Deramp is biascorr.Deramp and not issubclass(coreg.Deramp, bincorr.BiasCorr)
    assert coreg.BiasCorr is bincorr.BiasCorr and issubclass(coreg.DirectionalBias, coreg.BiasCorr) and issubclass(coreg.TerrainBias, coreg.BiasCorr)


def test_refusals():
    from xdem_amd import bincorr, coreg

    z = np.zeros((4, 5), dtype=np.float32)
    with pytest.raises(NotImplementedError, match="Weights have not yet been implemented"):
        coreg.BiasCorr(fit_or_bin="bin").fit(z, z, bias_vars={"a": z}, weights=z)
    with pytest.raises(NotImplementedError, match="Weights have not yet been implemented"):
        coreg.TerrainBias("elevation").fit(z, z, weights=z)

    class Cloud:   # (what a GeoDataFrame looks like from here)
        columns, geometry = ["z"], None

    with pytest.raises(NotImplementedError, match="Point-cloud"):
        coreg.DirectionalBias().fit(Cloud(), z)
    with pytest.raises(NotImplementedError, match="Point-cloud"):
        coreg.DirectionalBias().fit(z, Cloud())
    with pytest.raises(NotImplementedError, match="at most 3 variables"):
        bincorr.corr_apply(z, 0, [bincorr._Var("raster")] * 4, [2, 2, 2, 2])
    b = coreg.BiasCorr(fit_or_bin="bin", bias_var_names=list("abcd"))
    b.meta["outputs"]["fitorbin"] = {"bin_dataframe": None}
    with pytest.raises(NotImplementedError, match="at most 3 variables"):
        b.apply(z, bias_vars={k: z for k in "abcd"})


@pytest.mark.parametrize("shape,res", [((5, 7), (2.0, 3.0)), ((1, 200), (1.0, 1.0)), ((200, 1), (0.5, 4.0)), ((61, 83), (5.0, 5.0))])
def test_rotated_x_properties(shape, res):
    from xdem_amd.bincorr import rotated_x

    H, W = shape
    col = np.arange(W, dtype=np.float64)[None, :] * np.ones((H, 1))
    up = (H - 1 - np.arange(H, dtype=np.float64))[:, None] * np.ones((1, W))
    assert np.array_equal(rotated_x(shape, res, 0), col * res[0])                      # angle 0: the column coordinate
    x90 = rotated_x(shape, res, 90)                                                    # angle 90: the row coordinate, counted from the south
    extent = W * res[0] + H * res[1]
    assert np.allclose(x90, up * res[1], rtol=0, atol=1e-15 * extent)                  # (cos(pi / 2) is 6e-17, not 0)
    for angle in (0, 20, 90, 135, 200, -45, 359.5):
        x = rotated_x(shape, res, angle)
        assert x.dtype == np.float64 and x.shape == shape and x.min() == 0.0           # the minimum is exactly 0, taken at a corner
        c, s = np.cos(np.deg2rad(angle)), np.sin(np.deg2rad(angle))
        want = col * res[0] * c + up * res[1] * s
        assert np.allclose(x, want - want.min(), rtol=0, atol=1e-12 * extent)
    assert np.array_equal(rotated_x(shape, res[0], 20), rotated_x(shape, (res[0], res[0]), 20))


class _Recorder:
    """A step that records what the pipeline hands it."""

    def __init__(self, needs_vars=False, names=None, subsample=1.0):
        self.meta = {"inputs": {"random": {"subsample": subsample}, "fitorbin": {"bias_var_names": names}}, "outputs": {}}
        self._needs_vars = needs_vars
        self.seen = []

    def fit(self, reference_elev, to_be_aligned_elev, inlier_mask=None, bias_vars=None, weights=None, subsample=1.0, **kw):
        self.seen.append(("fit", None if bias_vars is None else sorted(bias_vars)))
        return self

    def apply(self, elev, bias_vars=None, **kw):
        self.seen.append(("apply", None if bias_vars is None else sorted(bias_vars)))
        return elev


def _pipeline(steps):
    from xdem_amd._coregbase import CoregPipeline, _Step

    class Step(_Recorder, _Step):
        pass

    made = [Step(*s) for s in steps]
    return CoregPipeline(made), made


def test_pipeline_hands_bias_vars_to_the_steps_that_need_them():
    z = np.zeros((3, 4), dtype=np.float32)
    pipe, (affine, a, b) = _pipeline([(False,), (True, ["slope"]), (True, ["aspect", "slope"])])
    assert pipe._needs_vars
    planes = {"slope": z, "aspect": z, "unused": z}
    pipe.fit(z, z, bias_vars=planes)
    assert affine.seen == [("fit", None), ("apply", None)]
    assert a.seen == [("fit", ["slope"]), ("apply", ["slope"])]
    assert b.seen == [("fit", ["aspect", "slope"])]
    pipe.apply(z, bias_vars=planes)
    assert affine.seen[-1] == ("apply", None) and a.seen[-1] == ("apply", ["slope"]) and b.seen[-1] == ("apply", ["aspect", "slope"])


def test_parse_bias_vars_messages():
    z = np.zeros((3, 4), dtype=np.float32)
    pipe, (a,) = _pipeline([(True, ["slope"])])
    with pytest.raises(ValueError) as info:
        pipe.fit(z, z)
    assert str(info.value) == f"No `bias_vars` passed to .fit() for bias correction step {a.__class__} of the pipeline."
    with pytest.raises(ValueError) as info:
        pipe.fit(z, z, bias_vars={"aspect": z})
    assert str(info.value) == ("Not all keys of `bias_vars` in .fit() match the `bias_var_names` defined during "
                               f"instantiation of the bias correction step {a.__class__}: ['slope'].")
    pipe, (a, b) = _pipeline([(True, ["slope"]), (True, None)])
    with pytest.raises(ValueError) as info:
        pipe.fit(z, z)
    assert str(info.value) == (f"No `bias_vars` passed to .fit() for bias correction step {a.__class__} of the pipeline."
                               " As you are using several bias correction steps requiring `bias_vars`, don't forget to "
                               "explicitly define their `bias_var_names` during instantiation, e.g. Step(bias_var_names=['slope']).")
    with pytest.raises(ValueError) as info:
        pipe._parse_bias_vars(1, {"slope": z})
    assert str(info.value) == ("When using several bias correction steps requiring `bias_vars` in a pipeline,"
                               "the `bias_var_names` need to be explicitly defined at each step's "
                               "instantiation, e.g. Step(bias_var_names=['slope']).")


def test_coregister_3d_forwards_or_refuses_bias_vars(monkeypatch):
    import xdem_amd
    from xdem_amd import coreg

    seen = {}

    def fake_fit(self, ref, tba, inlier_mask=None, bias_vars=None, resolution=None, **kw):
        seen["fit"] = (sorted(bias_vars), resolution)
        return self

    def fake_apply(self, elev, resolution=None, resample=True, *, bias_vars=None, transform=None, **kw):
        seen["apply"] = (sorted(bias_vars), resolution)
        return elev + 1, transform

    tf = (2.0, 0.0, 0.0, 0.0, -2.0, 10.0)
    a = xdem_amd.DEM(np.zeros((5, 6), dtype=np.float32), transform=tf)
    b = xdem_amd.DEM(np.ones((5, 6), dtype=np.float32), transform=tf)
    planes = {"x": np.zeros((5, 6))}
    # a method without variable steps still refuses them, before anything runs
    for method in (None, coreg.NuthKaab(), coreg.Deramp(), coreg.TerrainBias("elevation"), coreg.NuthKaab() + coreg.DirectionalBias()):
        with pytest.raises(NotImplementedError, match="bias_vars"):
            a.coregister_3d(b, method, bias_vars=planes)
    monkeypatch.setattr(coreg.BiasCorr, "fit", fake_fit)
    monkeypatch.setattr(coreg.BiasCorr, "apply", fake_apply)
    out = a.coregister_3d(b, coreg.BiasCorr(fit_or_bin="bin", bias_var_names=["x"]), bias_vars=planes)
    assert seen == {"fit": (["x"], (2.0, 2.0)), "apply": (["x"], (2.0, 2.0))} and np.all(out.data == 1.0) and out.transform == tf


def test_recorded_applied_arrays_are_the_raster_plus_the_recorded_correction():
    """The fixture stores the reference's correction (its ``_apply_rst`` on a zero raster) for every apply case and its applied
    array for a few: the applied array is ``elev + corr`` cast to the raster dtype, the one addition the GPU tests repeat."""
    from xdem_amd import synth

    golden = np.load(os.path.join(GOLDEN, "bincorr_golden.npz"))
    keys = [k for k in golden.files if k.startswith("applied|")]
    assert len(keys) == 3
    for key in keys:
        _, dtype, name, method, mc = key.split("|")
        elev = synth.bias_case(61, 83, np.dtype(dtype))["tba"]
        corr = golden[f"corr|{dtype}|{name}|{method}|{mc}"]
        assert golden[key].dtype == np.dtype(dtype) and np.array_equal(golden[key], (elev.astype(np.float64) + corr).astype(dtype), equal_nan=True)


def test_bias_case_is_reproducible_arithmetic():
    from xdem_amd import synth

    a, b = synth.bias_case(61, 83, np.float32), synth.bias_case(61, 83, np.float32)
    assert all(np.array_equal(a[k], b[k], equal_nan=True) for k in a)
    assert synth._hash01(3, 17).tolist() == [0.7990333654529804, 0.3187677329830695, 0.9891303072316078]   # (the integer mix is exact everywhere)
    c = synth.bias_case(1, 200, np.float64)
    assert c["ref"].shape == (1, 200) and c["ref"].dtype == np.float64 and c["v1"].dtype == np.float32 and c["v2"].dtype == np.float64
