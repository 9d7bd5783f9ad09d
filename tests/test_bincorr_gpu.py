"""BiasCorr / DirectionalBias / TerrainBias on the GPU (xdem_amd/bincorr.py, csrc/bincorr.hip) against what the reference's own
``BiasCorr._bin_or_and_fit_nd`` / ``_apply_rst`` returned (tests/golden/bincorr_golden.npz, tools/gen_golden_bincorr.py) on the
inputs of ``xdem_amd.synth.bias_case``, and against the composed routes of the entries that existed before the fused pass.

Bars: the DataFrame, the per-bin apply and the polynomial apply are bit for bit (exact medians, an exact lookup / Horner in
NumPy's order, one float64 add, one rounding).  The linear apply carries the project's bar for xdemhip_interp_grid_linear against
SciPy (1e-12 relative to the correction) plus the rounding of the sum.  The sum-of-sinusoids apply differs from NumPy
by the device's ``sin``: bar below."""
import functools
import os

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

BINNINGS = {
    "v1_b1": (["v1"], 1),
    "v1_b10": (["v1"], 10),
    "v3_b100": (["v3"], 100),
    "v12_b6": (["v1", "v2"], 6),
    "v12_edges": (["v1", "v2"], {"v1": [0.0, 2.5, 5.0, 7.5, 10.0], "v2": [-1.0, -1.0 / 3.0, 1.0 / 3.0, 1.0]}),
    "v123_435": (["v1", "v2", "v3"], {"v1": [0.0, 2.5, 5.0, 7.5, 10.0], "v2": [-1.0, -1.0 / 3.0, 1.0 / 3.0, 1.0],
                                      "v3": [0.0, 6.0, 12.0, 18.0, 24.0, 30.0]}),
}
APPLY_PLANE = {"v1": "a1", "v2": "a2", "v3": "a3"}
AWKWARD = [(1, 200), (200, 1), (61, 83), (129, 193)]   # no multiple of 64 anywhere

# Worst |corr_got - corr_ref| / sum|a_k| of the sum-of-sinusoids apply on the fixture, MEASURED on an MI355X (gfx950): 1.483e-16.
# The raster of the measurement is 0 in float64, so that the result IS the device's corr (0 + corr) and the figure holds nothing
# but ocml's double sin against NumPy's, at arguments up to 2 pi / 200 * 490 + 1 (one term, sum|a_k| = 2.99): two thirds of an ulp
# of the largest correction.  The bar is 4 x the measured value, since ROCm releases change ocml's sin.
SUMSIN_MEASURED = 1.483e-16
SUMSIN_BAR = 4 * SUMSIN_MEASURED


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "bincorr_golden.npz"))


@functools.lru_cache(maxsize=None)
def _case(H, W, dtype):
    from xdem_amd import synth

    c = synth.bias_case(H, W, np.dtype(dtype))
    for v in c.values():
        v.setflags(write=False)
    return c


def _cuda(a):
    import torch

    return torch.from_numpy(np.array(a)).cuda()   # (a copy: the cached inputs are read-only)


def _np(a):
    return a.cpu().numpy() if hasattr(a, "is_cuda") else np.asarray(a)


def _frame_columns(df, names, stat="nanmedian"):
    import pandas as pd

    out = {"nd": df["nd"].values.astype(np.int64), stat: df[stat].values.astype(np.float64), "count": df["count"].values.astype(np.float64)}
    for n in names:
        cells = df[n].values
        out[n + "_left"] = np.array([c.left if isinstance(c, pd.Interval) else np.nan for c in cells], dtype=np.float64)
        out[n + "_right"] = np.array([c.right if isinstance(c, pd.Interval) else np.nan for c in cells], dtype=np.float64)
    return out


def _ulp(x, mant_bits):
    """Spacing of the floats with `mant_bits` mantissa bits in the binade of |x| (2^(e - mant_bits) for |x| in [2^(e-1), 2^e))."""
    _, e = np.frexp(np.abs(x))
    return np.ldexp(1.0, e - mant_bits)


def _fit_bin(name, case, method="linear", space="host", **kw):
    from xdem_amd import coreg

    names, bins = BINNINGS[name]
    conv = _cuda if space == "device" else (lambda a: a)
    b = coreg.BiasCorr(fit_or_bin="bin", bin_sizes=bins, bin_statistic=np.nanmedian, bin_apply_method=method, bias_var_names=names)
    b.fit(conv(case["ref"]), conv(case["tba"]), conv(case["inlier"]), bias_vars={n: conv(case[n]) for n in names}, **kw)
    return b


# ---- fit: the DataFrame ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(BINNINGS))
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("shape,space", [((61, 83), "host"), ((61, 83), "device"), ((129, 193), "device")])
def test_bin_dataframe_equals_the_reference(golden, name, dtype, shape, space):
    H, W = shape
    b = _fit_bin(name, _case(H, W, dtype), space=space)
    names = BINNINGS[name][0]
    df = b.meta["outputs"]["fitorbin"]["bin_dataframe"]
    assert list(df.columns) == ["nd", "nanmedian", "count"] + names
    got = _frame_columns(df, names)
    for k, v in got.items():
        assert np.array_equal(v, golden[f"df|{H}x{W}|{dtype}|{name}|{k}"], equal_nan=True), k
    assert set(b.meta["outputs"]["fitorbin"]) == {"bin_dataframe"} and b.meta["inputs"]["fitorbin"]["bias_var_names"] == names


# ---- apply against the reference's recorded correction -----------------------------------------------------------------------------
def _recorded(golden, kind):
    return sorted(tuple(k.split("|")[1:]) for k in golden.files if k.startswith("corr|") and k.split("|")[3] == kind)


def _apply_case(golden, dtype, name, method, mc, space="host"):
    case = _case(61, 83, dtype)
    b = _fit_bin(name, case, method)
    conv = _cuda if space == "device" else (lambda a: a)
    planes = {n: conv(case[APPLY_PLANE[n]]) for n in BINNINGS[name][0]}
    kw = {"min_count": int(mc)} if method == "linear" else {}
    got = _np(b.apply(conv(case["tba"]), bias_vars=planes, **kw))
    corr = golden[f"corr|{dtype}|{name}|{method}|{mc}"]
    assert got.dtype == np.dtype(dtype) and got.shape == (61, 83)
    return got, case["tba"].astype(np.float64) + corr, corr


def test_the_fixture_has_every_kind_of_apply(golden):
    per_bin, linear = _recorded(golden, "per_bin"), _recorded(golden, "linear")
    assert len(per_bin) == 8 and len(linear) == 12
    assert {c[0] for c in per_bin} == {"float32", "float64"} == {c[0] for c in linear} and {c[3] for c in linear} == {"0", "5"}
    # the planted values do their work: pixels outside every bin (NaN per bin, extrapolated linearly), and a count filter that bites
    a = golden["corr|float32|v3_b100|linear|0"], golden["corr|float32|v3_b100|linear|5"]
    assert not np.array_equal(a[0], a[1], equal_nan=True)
    assert np.isnan(golden["corr|float32|v1_b10|per_bin|0"]).sum() > np.isnan(golden["corr|float32|v1_b10|linear|0"]).sum() > 0


@pytest.mark.parametrize("space", ["host", "device"])
def test_per_bin_apply_is_bit_exact(golden, space):
    for dtype, name, method, mc in _recorded(golden, "per_bin"):
        got, expected64, _ = _apply_case(golden, dtype, name, method, mc, space)
        assert np.array_equal(got, expected64.astype(dtype), equal_nan=True), (dtype, name)


@pytest.mark.parametrize("space", ["host", "device"])
def test_linear_apply_within_the_interpolation_bar(golden, space):
    for dtype, name, method, mc in _recorded(golden, "linear"):
        got, expected64, corr = _apply_case(golden, dtype, name, method, mc, space)
        assert np.array_equal(np.isnan(got), np.isnan(expected64)), (dtype, name, mc)
        ok = np.isfinite(expected64)
        err = np.abs(got.astype(np.float64)[ok] - expected64[ok])
        if dtype == "float64":
            bar = 1e-12 * np.abs(corr[ok]) + _ulp(expected64[ok], 53)
        else:
            bar = 0.5 * _ulp(expected64[ok], 24) + 1e-12 * np.abs(corr[ok])
        worst = float(np.max(err / bar))
        print(f"linear {dtype} {name} min_count={mc}: worst error / bar = {worst:.3g}")
        assert np.all(err <= bar), (dtype, name, mc, worst)


def _poly_step(case, space="host"):
    from xdem_amd import coreg

    conv = _cuda if space == "device" else (lambda a: a)
    b = coreg.BiasCorr(fit_or_bin="bin_and_fit", fit_func="norder_polynomial", bin_sizes=30, bin_statistic=np.nanmedian, bias_var_names=["v1"])
    import warnings

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")   # (scikit-learn's convergence warnings for the high orders, as in the reference's run)
        b.fit(conv(case["ref"]), conv(case["tba"]), conv(case["inlier"]), bias_vars={"v1": conv(case["v1"])})
    return b


@pytest.mark.parametrize("space", ["host", "device"])
def test_polynomial_workflow_fit_and_apply_are_bit_exact(golden, space):
    from xdem_amd import fit

    case = _case(61, 83, "float32")
    b = _poly_step(case, space)
    assert b.meta["inputs"]["fitorbin"]["fit_func"] is fit.polynomial_1d
    assert np.array_equal(b.meta["outputs"]["fitorbin"]["fit_params"], golden["poly|fit_params"])
    assert b.meta["outputs"]["specific"] == {"best_poly_order": int(golden["poly|order"])}
    assert "bin_dataframe" not in b.meta["outputs"]["fitorbin"] and "fit_perr" not in b.meta["outputs"]["fitorbin"]
    conv = _cuda if space == "device" else (lambda a: a)
    corr = golden["poly|corr"]
    got = _np(b.apply(conv(case["tba"]), bias_vars={"v1": conv(case["a1"])}))
    assert got.dtype == np.float32 and got.shape == (61, 83)   # (the reference's internal result is (1, H, W); the public one 2-D)
    assert np.array_equal(got, (case["tba"].astype(np.float64) + corr).astype(np.float32), equal_nan=True)
    elev64 = case["tba"].astype(np.float64) * 1.000000123
    got = _np(b.apply(conv(elev64), bias_vars={"v1": conv(case["a1"])}))
    assert got.dtype == np.float64 and np.array_equal(got, elev64 + corr, equal_nan=True)


def test_sumsin_apply_within_the_measured_bar(golden):
    from xdem_amd import coreg
    from xdem_amd.bincorr import rotated_x

    params = golden["sumsin|fit_params"]
    corr = golden["sumsin|corr"]
    plane = rotated_x((61, 83), (5.0, 5.0), 20.0)
    scale = float(np.sum(np.abs(params[0::3])))
    b = coreg.BiasCorr(fit_or_bin="bin_and_fit", fit_func="nfreq_sumsin", bin_sizes=40, bias_var_names=["angle"])
    b.meta["outputs"]["fitorbin"] = {"fit_params": params}
    # elev = 0 in float64: the result IS the device's corr (0 + corr), as the fixture's corr is the reference's
    got = b.apply(np.zeros((61, 83)), bias_vars={"angle": plane})
    worst = float(np.max(np.abs(got - corr))) / scale
    print(f"sumsin apply: worst |corr_got - corr_ref| / sum|a_k| = {worst:.3e} (bar {SUMSIN_BAR:.3e})")
    assert worst <= SUMSIN_BAR
    # three frequencies, a float32 raster, the rotated coordinate formed on the device: against NumPy's own evaluation
    from xdem_amd import fit

    p3 = np.array([2.0, 150.0, 0.5, 0.7, 41.0, 3.0, 0.1, 7.0, 6.0])
    d = coreg.DirectionalBias(angle=20.0)
    d.meta["outputs"]["fitorbin"] = {"fit_params": p3}
    case = _case(61, 83, "float32")
    got = d.apply(case["tba"], resolution=(5.0, 5.0))
    want64 = case["tba"].astype(np.float64) + fit.sumsin_1d((plane,), *p3)
    ok = np.isfinite(want64)
    assert np.array_equal(np.isnan(got), ~ok)
    assert np.all(np.abs(got.astype(np.float64)[ok] - want64[ok]) <= 0.5 * _ulp(want64[ok], 24) + SUMSIN_BAR * np.sum(np.abs(p3[0::3])))


# ---- the fused pass against the composed routes of the entries that existed before it ------------------------------------------------
def _grid(n_var):
    """A small interpolation grid over the apply planes' ranges (uneven axes), values from a hash: no fit needed."""
    from xdem_amd.synth import _hash01

    axes = [np.array([-1.0, 0.5, 2.0, 4.5, 7.0, 9.5, 11.0]), np.array([-2.0, -0.5, 0.1, 0.8, 2.0]), np.array([-1.0, 3.0, 9.0, 15.0, 21.0, 27.0, 31.0])][:n_var]
    shape = tuple(len(a) for a in axes)
    return axes, (4.0 * _hash01(int(np.prod(shape)), 77) - 2.0).reshape(shape)


@pytest.mark.parametrize("shape", AWKWARD)
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("n_var", [1, 2, 3])
def test_fused_grid_apply_equals_the_composed_route(shape, dtype, n_var):
    from xdem_amd import _lib, bincorr
    from xdem_amd.spatialstats import GridInterpolant

    case = _case(shape[0], shape[1], dtype)
    axes, values = _grid(n_var)
    planes = [case[k] for k in ("a1", "a2", "a3")[:n_var]]
    composed = (case["tba"].astype(np.float64) + GridInterpolant(axes, values)(tuple(planes))).astype(dtype)
    variables = [bincorr._Var("plane", p) for p in planes]
    for conv in (lambda a: a, _cuda):
        got, missing = bincorr.corr_apply(conv(case["tba"]), _lib.CORR_GRID, variables, [len(a) for a in axes], a=np.concatenate(axes), table=values)
        assert missing == 0 and np.array_equal(_np(got), composed, equal_nan=True)


@pytest.mark.parametrize("shape", AWKWARD)
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_fused_per_bin_apply_equals_get_perbin_nd_binning(shape, dtype):
    from xdem_amd.spatialstats import get_perbin_nd_binning

    case = _case(shape[0], shape[1], dtype)
    for name in ("v1_b10", "v123_435"):
        b = _fit_bin(name, case, "per_bin")
        names = BINNINGS[name][0]
        planes = {n: case[APPLY_PLANE[n]] for n in names}
        corr = get_perbin_nd_binning(b.meta["outputs"]["fitorbin"]["bin_dataframe"], list(planes.values()), names, np.nanmedian)
        want = (case["tba"].astype(np.float64) + corr).astype(dtype)
        assert np.array_equal(b.apply(case["tba"], bias_vars=planes), want, equal_nan=True)
        assert np.array_equal(_np(b.apply(_cuda(case["tba"]), bias_vars={n: _cuda(p) for n, p in planes.items()})), want, equal_nan=True)


def test_raster_and_rotated_sources_equal_their_planes():
    """"The raster itself" and the rotated coordinate, formed per pixel, against the same values handed over as planes."""
    from xdem_amd import _lib, bincorr

    for shape in AWKWARD:
        for dtype in ("float32", "float64"):
            case = _case(shape[0], shape[1], dtype)
            elev = case["tba"]
            axes = [np.array([700.0, 790.0, 801.5, 820.0, 900.0]), np.array([-5.0, 0.0, 40.0, 300.0, 1200.0])]
            values = np.arange(25, dtype=np.float64).reshape(5, 5) ** 0.5
            rot = bincorr._rotation(shape, (5.0, 3.0), 20.0)
            x = bincorr.rotated_x(shape, (5.0, 3.0), 20.0)
            args = dict(n_tab=[5, 5], a=np.concatenate(axes), table=values)
            fused = bincorr.corr_apply(elev, _lib.CORR_GRID, [bincorr._Var("raster"), bincorr._Var("rotated", rot=rot)], **args)[0]
            planes = bincorr.corr_apply(elev, _lib.CORR_GRID, [bincorr._Var("plane", elev), bincorr._Var("plane", x)], **args)[0]
            assert np.array_equal(fused, planes, equal_nan=True), (shape, dtype)
            assert np.isfinite(fused).sum() == np.isfinite(elev).sum() > 0
            # the same two sources through the per-bin lookup, and each of them through the 1-D models
            left, right = np.array([700.0, 800.0, 0.0, 100.0, 500.0]), np.array([800.0, 1000.0, 100.0, 500.0, 5000.0])
            args = dict(n_tab=[2, 3], a=left, b=right, table=np.arange(6.0) - 2.5, decided=np.array([1, 1, 0, 1, 1, 1], np.uint8))
            fused = bincorr.corr_apply(elev, _lib.CORR_PERBIN, [bincorr._Var("raster"), bincorr._Var("rotated", rot=rot)], **args)[0]
            planes = bincorr.corr_apply(elev, _lib.CORR_PERBIN, [bincorr._Var("plane", elev), bincorr._Var("plane", x)], **args)[0]
            assert np.array_equal(fused, planes, equal_nan=True), (shape, dtype)
            for kind, table in ((_lib.CORR_POLY, [1.0, -2e-3, 1e-6]), (_lib.CORR_SUMSIN, [2.0, 300.0, 0.5, 0.25, 41.0, 3.0])):
                for source, plane in ((bincorr._Var("raster"), elev), (bincorr._Var("rotated", rot=rot), x)):
                    fused = bincorr.corr_apply(elev, kind, [source], [len(table)], table=table)[0]
                    planes = bincorr.corr_apply(elev, kind, [bincorr._Var("plane", plane)], [len(table)], table=table)[0]
                    assert np.array_equal(fused, planes, equal_nan=True), (shape, dtype, kind, source.kind)


# ---- the plan's new entries -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", AWKWARD)
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("space", ["host", "device"])
def test_restrict_finite_and_var_columns_equal_numpy(shape, dtype, space):
    from xdem_amd import _lib, bincorr
    from xdem_amd._coregbase import subsample_ranks
    from xdem_amd.biascorr import DhPlan

    case = _case(shape[0], shape[1], dtype)
    conv = _cuda if space == "device" else (lambda a: a)
    ref, tba, v1, v2 = case["ref"], case["tba"], case["v1"], case["a2"]
    valid = case["inlier"] & np.isfinite(ref) & np.isfinite(tba)
    rot = bincorr._rotation(shape, (2.0, 3.0), 33.0)
    x = bincorr.rotated_x(shape, (2.0, 3.0), 33.0)
    for drawn in (False, True):
        with DhPlan(conv(ref), conv(tba), conv(case["inlier"])) as plan:
            assert plan.n_valid == valid.sum()
            dh0 = plan.values(coords=False) if not drawn else None   # (listing the pixels ends the narrowing: checked below)
            if dh0 is not None:
                with pytest.raises(_lib.XdemHipError, match="before the draw"):
                    plan.restrict_finite(conv(v1))
                continue
            p1, c1, k1 = plan._plane(conv(v1))
            assert plan.restrict_finite(k1) == (valid & np.isfinite(v1)).sum()
            p2, c2, k2 = plan._plane(conv(v2))
            assert plan.restrict_finite(k2) == (valid & np.isfinite(v1) & np.isfinite(v2)).sum() == plan.n_valid
            sel = np.flatnonzero((valid & np.isfinite(v1) & np.isfinite(v2)).ravel())
            ranks = np.sort(subsample_ranks(sel.size, 0.3, 7))
            assert plan.subsample(ranks) == ranks.size
            sel = sel[ranks]
            with pytest.raises(_lib.XdemHipError, match="before the draw"):
                plan.restrict_finite(k1)
            srcs = [bincorr._source(bincorr._Var("plane"), p1, c1), bincorr._source(bincorr._Var("plane"), p2, c2),
                    bincorr._source(bincorr._Var("rotated", rot=rot)), bincorr._source(bincorr._Var("raster")),
                    _lib.VarSrc(_lib.VAR_TBA, 0, None, 0.0, 0.0, 0.0, 0.0, 0.0)]
            dh, cols = plan.var_columns(srcs)
            want_dh, col, row = plan.values()
            assert np.array_equal(row * shape[1] + col, sel)
            assert np.array_equal(_np(dh), want_dh) and np.array_equal(want_dh, (ref.ravel()[sel] - tba.ravel()[sel]).astype(dtype))
            for got, want in zip(cols, (v1.ravel()[sel], v2.ravel()[sel], x.ravel()[sel], ref.ravel()[sel], tba.ravel()[sel])):
                got = _np(got)
                assert got.dtype == want.dtype and np.array_equal(got, want)
    # without a draw: every valid pixel, in raster order
    with DhPlan(conv(ref), conv(tba), conv(case["inlier"])) as plan:
        p1, c1, k1 = plan._plane(conv(v1))
        plan.restrict_finite(k1)
        dh, (c,) = plan.var_columns([bincorr._source(bincorr._Var("plane"), p1, c1)])
        sel = np.flatnonzero((valid & np.isfinite(v1)).ravel())
        assert np.array_equal(_np(dh), (ref.ravel()[sel] - tba.ravel()[sel]).astype(dtype)) and np.array_equal(_np(c), v1.ravel()[sel])


def test_subsampled_fit_bins_the_drawn_pixels():
    from xdem_amd import coreg
    from xdem_amd._coregbase import subsample_ranks
    from xdem_amd.spatialstats import nd_binning

    case = _case(129, 193, "float32")
    b = coreg.BiasCorr(fit_or_bin="bin", bin_sizes=8, bias_var_names=["v1", "v2"], subsample=0.25)
    b.fit(case["ref"], case["tba"], case["inlier"], bias_vars={"v1": case["v1"], "v2": case["v2"]}, random_state=11)
    valid = case["inlier"] & np.isfinite(case["ref"]) & np.isfinite(case["tba"]) & np.isfinite(case["v1"]) & np.isfinite(case["v2"])
    sel = np.sort(np.flatnonzero(valid.ravel())[subsample_ranks(int(valid.sum()), 0.25, 11)])
    assert b.meta["outputs"]["random"]["subsample_final"] == sel.size and b.meta["inputs"]["random"]["random_state"] == 11
    want = nd_binning(case["ref"].ravel()[sel] - case["tba"].ravel()[sel], [case["v1"].ravel()[sel], case["v2"].ravel()[sel]], ["v1", "v2"], 8,
                      statistics=(np.nanmedian, "count"))
    got = b.meta["outputs"]["fitorbin"]["bin_dataframe"]
    for k, v in _frame_columns(got, ["v1", "v2"]).items():
        assert np.array_equal(v, _frame_columns(want, ["v1", "v2"])[k], equal_nan=True), k


# ---- the subclasses are BiasCorr with their variable -----------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("method", ["linear", "per_bin"])
def test_directional_bias_equals_biascorr_with_the_rotated_plane(dtype, method):
    from xdem_amd import coreg
    from xdem_amd.bincorr import rotated_x

    case = _case(129, 193, dtype)
    res = (5.0, 4.0)
    x = rotated_x((129, 193), res, 20.0)
    d = coreg.DirectionalBias(angle=20.0, fit_or_bin="bin", bin_sizes=25, bin_apply_method=method)
    d.fit(case["ref"], case["tba"], case["inlier"], resolution=res)
    b = coreg.BiasCorr(fit_or_bin="bin", bin_sizes=25, bin_apply_method=method, bias_var_names=["angle"])
    b.fit(case["ref"], case["tba"], case["inlier"], bias_vars={"angle": x})
    got, want = (_frame_columns(s.meta["outputs"]["fitorbin"]["bin_dataframe"], ["angle"]) for s in (d, b))
    for k in want:
        assert np.array_equal(got[k], want[k], equal_nan=True), k
    out_d = d.apply(case["tba"], resolution=res)
    assert out_d.dtype == np.dtype(dtype) and np.array_equal(out_d, b.apply(case["tba"], bias_vars={"angle": x}), equal_nan=True)
    assert np.array_equal(_np(d.apply(_cuda(case["tba"]), resolution=res)), out_d, equal_nan=True)
    out, tf = d.apply(case["tba"], resolution=res, transform=(5.0, 0.0, 0.0, 0.0, -4.0, 0.0))
    assert tf == (5.0, 0.0, 0.0, 0.0, -4.0, 0.0) and np.array_equal(out, out_d, equal_nan=True)


@pytest.mark.parametrize("attribute", ["slope", "elevation"])
def test_terrain_bias_equals_biascorr_with_the_terrain_plane(attribute):
    from xdem_amd import coreg, terrain

    case = _case(129, 193, "float32")
    res = (5.0, 5.0)
    plane_of = (lambda dem: dem) if attribute == "elevation" else (lambda dem: terrain.get_terrain_attribute(dem, "slope", resolution=res))
    t = coreg.TerrainBias(attribute, bin_sizes=20)
    t.fit(case["ref"], case["tba"], case["inlier"], resolution=res)
    b = coreg.BiasCorr(fit_or_bin="bin", bin_sizes=20, bias_var_names=[attribute])
    b.fit(case["ref"], case["tba"], case["inlier"], bias_vars={attribute: plane_of(case["ref"])})
    got, want = (_frame_columns(s.meta["outputs"]["fitorbin"]["bin_dataframe"], [attribute]) for s in (t, b))
    for k in want:
        assert np.array_equal(got[k], want[k], equal_nan=True), k
    out = t.apply(case["tba"], resolution=res)
    assert np.array_equal(out, b.apply(case["tba"], bias_vars={attribute: plane_of(case["tba"])}), equal_nan=True)
    assert np.array_equal(_np(t.apply(_cuda(case["tba"]), resolution=res)), out, equal_nan=True)
    # a plane passed under the attribute's name wins
    t2 = coreg.TerrainBias(attribute, bin_sizes=20)
    t2.fit(case["ref"], case["tba"], case["inlier"], bias_vars={attribute: case["v3"]}, resolution=res)
    b2 = coreg.BiasCorr(fit_or_bin="bin", bin_sizes=20, bias_var_names=[attribute])
    b2.fit(case["ref"], case["tba"], case["inlier"], bias_vars={attribute: case["v3"]})
    assert np.array_equal(t2.meta["outputs"]["fitorbin"]["bin_dataframe"]["nanmedian"].values, b2.meta["outputs"]["fitorbin"]["bin_dataframe"]["nanmedian"].values,
                          equal_nan=True)
    assert np.array_equal(t2.apply(case["tba"], bias_vars={attribute: case["a3"]}), b2.apply(case["tba"], bias_vars={attribute: case["a3"]}), equal_nan=True)


def test_fit_mode_hands_the_columns_to_the_optimiser():
    from xdem_amd import coreg, fit

    case = _case(61, 83, "float32")
    seen = {}

    def optimiser(f, xdata, ydata, sigma=None, absolute_sigma=None, **kw):
        seen.update(f=f, x=xdata, y=ydata, sigma=sigma, absolute_sigma=absolute_sigma, kw=kw)
        return np.array([0.25, 0.5]), None

    b = coreg.BiasCorr(fit_or_bin="fit", fit_func=fit.polynomial_1d, fit_optimizer=optimiser)
    b.fit(case["ref"], case["tba"], case["inlier"], bias_vars={"v1": case["v1"]}, maxfev=7)
    valid = case["inlier"] & np.isfinite(case["ref"]) & np.isfinite(case["tba"]) & np.isfinite(case["v1"])
    assert seen["f"] is fit.polynomial_1d and seen["sigma"] is None and seen["absolute_sigma"] is True and seen["kw"] == {"maxfev": 7}
    assert np.array_equal(seen["x"], case["v1"][valid]) and np.array_equal(seen["y"], case["ref"][valid] - case["tba"][valid])
    assert b.meta["outputs"]["fitorbin"] == {"fit_params": pytest.approx(np.array([0.25, 0.5]))} and b.meta["inputs"]["fitorbin"]["bias_var_names"] == ["v1"]
    got = b.apply(case["tba"], bias_vars={"v1": case["a1"]})
    assert np.array_equal(got, (case["tba"] + (0.25 + 0.5 * case["a1"].astype(np.float64))).astype(np.float32), equal_nan=True)
    # any other function: the host route
    b.meta["inputs"]["fitorbin"]["fit_func"] = lambda xx, a, c: a + c * xx[0]
    assert np.array_equal(b.apply(case["tba"], bias_vars={"v1": case["a1"]}), got, equal_nan=True)


# ---- limits and refusals ---------------------------------------------------------------------------------------------------------------
def test_table_limits_one_bin_and_missing_bins():
    import pandas as pd

    from xdem_amd import _lib, bincorr, coreg

    elev = _case(61, 83, "float32")["tba"]
    x = _case(61, 83, "float32")["a1"]
    var = [bincorr._Var("plane", x)]
    # per bin: one bin; 3072 bins; one past the limit
    out, missing = bincorr.corr_apply(elev, _lib.CORR_PERBIN, var, [1], a=[0.0], b=[10.0], table=[1.5], decided=[1])
    inside = (x >= 0) & (x < 10)
    assert missing == 0 and np.array_equal(out, np.where(inside, (elev.astype(np.float64) + 1.5).astype(np.float32), np.float32(np.nan)), equal_nan=True)
    for n, ok in ((3072, True), (3073, False)):
        edges = np.linspace(0.0, 10.0, n + 1)
        table = np.arange(n, dtype=np.float64)
        if not ok:
            with pytest.raises(_lib.XdemHipError, match="more than 3072 table entries"):
                bincorr.corr_apply(elev, _lib.CORR_PERBIN, var, [n], a=edges[:-1], b=edges[1:], table=table, decided=np.ones(n, np.uint8))
            continue
        out, missing = bincorr.corr_apply(elev, _lib.CORR_PERBIN, var, [n], a=edges[:-1], b=edges[1:], table=table, decided=np.ones(n, np.uint8))
        idx = np.searchsorted(edges, x.astype(np.float64), side="right") - 1
        want = np.where(inside, (elev.astype(np.float64) + table[np.clip(idx, 0, n - 1)]).astype(np.float32), np.float32(np.nan))
        assert missing == 0 and np.array_equal(out, want, equal_nan=True)
    # linear: 3072 grid points; one past the limit
    from xdem_amd.spatialstats import GridInterpolant

    for n, ok in ((3072, True), (3073, False)):
        axis, values = np.linspace(-1.0, 11.0, n), np.sin(np.arange(n))
        if not ok:
            with pytest.raises(_lib.XdemHipError, match="more than 3072 table entries"):
                bincorr.corr_apply(elev, _lib.CORR_GRID, var, [n], a=axis, table=values)
            continue
        out, _ = bincorr.corr_apply(elev, _lib.CORR_GRID, var, [n], a=axis, table=values)
        assert np.array_equal(out, (elev.astype(np.float64) + GridInterpolant([axis], values)((x,))).astype(np.float32), equal_nan=True)
    with pytest.raises(_lib.XdemHipError, match="3072"):
        bincorr.corr_apply(elev, _lib.CORR_GRID, var * 3, [16, 16, 13], a=np.concatenate([np.arange(16.0), np.arange(16.0), np.arange(13.0)]),
                           table=np.zeros(16 * 16 * 13))
    # a DataFrame without the row of a bin that pixels fall into: upstream's IndexError
    b = coreg.BiasCorr(fit_or_bin="bin", bin_apply_method="per_bin", bias_var_names=["v1"])
    ii = pd.IntervalIndex.from_breaks([0.0, 5.0, 10.0], closed="left")
    b.meta["outputs"]["fitorbin"] = {"bin_dataframe": pd.DataFrame({"nd": [1, 2, 2], "nanmedian": [1.0, 2.0, 3.0], "count": [5.0, 5.0, 5.0],
                                                                   "v1": [ii[0], ii[0], ii[1]], "v2": [np.nan, ii[0], ii[1]]})}
    out = b.apply(elev, bias_vars={"v1": x})
    assert np.array_equal(out, np.where((x >= 0) & (x < 5), (elev.astype(np.float64) + 1.0).astype(np.float32), np.float32(np.nan)), equal_nan=True)
    b2 = coreg.BiasCorr(fit_or_bin="bin", bin_apply_method="per_bin", bias_var_names=["v1", "v2"])
    df = pd.DataFrame({"nd": [2, 2, 2], "nanmedian": [1.0, 2.0, 3.0], "count": [5.0, 5.0, 5.0], "v1": [ii[0], ii[0], ii[1]], "v2": [ii[0], ii[1], ii[1]]})
    b2.meta["outputs"]["fitorbin"] = {"bin_dataframe": df}
    with pytest.raises(IndexError, match="index 0 is out of bounds for axis 0 with size 0"):
        b2.apply(elev, bias_vars={"v1": x, "v2": np.full_like(x, 2.0)})   # v1 in [5, 10), v2 in [0, 5): no such row


def test_every_selected_pixel_in_one_bin_and_nothing_valid():
    from xdem_amd import coreg
    from xdem_amd._coregbase import NO_VALID

    case = _case(61, 83, "float32")
    const = np.full((61, 83), 3.0, dtype=np.float32)
    b = coreg.BiasCorr(fit_or_bin="bin", bin_sizes=4, bias_var_names=["c"])
    b.fit(case["ref"], case["tba"], case["inlier"], bias_vars={"c": const})
    df = b.meta["outputs"]["fitorbin"]["bin_dataframe"]
    valid = case["inlier"] & np.isfinite(case["ref"]) & np.isfinite(case["tba"])
    # SciPy's edges for a constant sample: [c - 0.5, c + 0.5] cut in four; the value sits on the edge between bins 1 and 2
    assert df["count"].values.tolist() == [0.0, 0.0, float(valid.sum()), 0.0]
    assert df["nanmedian"].values[2] == np.median(case["ref"][valid] - case["tba"][valid])
    out = b.apply(case["tba"], bias_vars={"c": const})
    assert np.array_equal(out, (case["tba"].astype(np.float64) + float(df["nanmedian"].values[2])).astype(np.float32), equal_nan=True)
    for step, kw in ((coreg.BiasCorr(fit_or_bin="bin"), {"bias_vars": {"c": np.full((61, 83), np.nan, dtype=np.float32)}}),
                     (coreg.DirectionalBias(fit_or_bin="bin"), {"inlier_mask": np.zeros((61, 83), dtype=bool)})):
        with pytest.raises(ValueError) as info:
            step.fit(case["ref"], case["tba"], **kw)
        assert str(info.value) == NO_VALID


def test_row_partitioned_contexts_are_refused(monkeypatch):
    from xdem_amd import _lib, coreg

    case = _case(61, 83, "float32")
    monkeypatch.setattr(_lib.default_context(), "_hook", object(), raising=False)   # (what Context.set_allreduce leaves behind)
    with pytest.raises(NotImplementedError, match="multi-rank"):
        coreg.TerrainBias("elevation").fit(case["ref"], case["tba"], case["inlier"])


def test_integer_dict_of_bin_sizes_fails_as_upstream():
    import json

    want = json.load(open(os.path.join(GOLDEN, "bincorr_errors.json")))["integer_dict_two_variables"]
    case = _case(61, 83, "float32")
    from xdem_amd import coreg

    b = coreg.BiasCorr(fit_or_bin="bin", bin_sizes={"v1": 4, "v2": 3}, bias_var_names=["v1", "v2"])
    with pytest.raises(TypeError) as info:
        b.fit(case["ref"], case["tba"], case["inlier"], bias_vars={"v1": case["v1"], "v2": case["v2"]})
    assert want["type"] == "TypeError" and str(info.value) == want["message"]


# ---- end to end --------------------------------------------------------------------------------------------------------------------
def _nmad(x):
    x = x[np.isfinite(x)]
    return 1.4826 * np.median(np.abs(x - np.median(x)))


def _terrain_pair():
    from xdem_amd import synth

    ref = synth.fbm_numpy((160, 200), seed=3, mean=1000.0, std=200.0)
    noise = (0.2 * (synth._hash01(ref.size, 4) - 0.5)).reshape(ref.shape).astype(np.float32)
    return ref, noise


def test_directional_bias_lowers_the_nmad_of_an_along_track_sine():
    from xdem_amd import coreg
    from xdem_amd.bincorr import rotated_x

    ref, noise = _terrain_pair()
    res = (10.0, 10.0)
    x = rotated_x(ref.shape, res, 20.0)
    tba = (ref - 3.0 * np.sin(2 * np.pi / 700.0 * x) + noise).astype(np.float32)
    out = coreg.DirectionalBias(angle=20, fit_or_bin="bin").fit_and_apply(ref, tba, fit_kwargs={"resolution": res})
    assert out.shape == ref.shape and out.dtype == np.float32
    assert _nmad(ref - out) < _nmad(ref - tba)


def test_terrain_bias_lowers_the_nmad_of_an_elevation_proportional_bias():
    from xdem_amd import coreg

    ref, noise = _terrain_pair()
    tba = (ref - 0.01 * (ref - 1000.0) + noise).astype(np.float32)
    out = coreg.TerrainBias("elevation").fit_and_apply(ref, tba)
    assert _nmad(ref - out) < _nmad(ref - tba)


def test_bias_corrections_in_a_pipeline_and_through_coregister_3d():
    import xdem_amd
    from xdem_amd import coreg

    ref, noise = _terrain_pair()
    tba = (ref - 0.01 * (ref - 1000.0) + noise).astype(np.float32)
    tf = (10.0, 0.0, 0.0, 0.0, -10.0, 1600.0)
    pipe = coreg.NuthKaab() + coreg.TerrainBias("elevation")
    out = pipe.fit_and_apply(ref, tba, fit_kwargs={"resolution": 10.0})
    assert out.shape == ref.shape and _nmad(ref - out) < _nmad(ref - tba)
    a, b = xdem_amd.DEM(tba, transform=tf), xdem_amd.DEM(ref, transform=tf)
    for method in (coreg.TerrainBias("elevation"), coreg.DirectionalBias(angle=20, fit_or_bin="bin"), coreg.NuthKaab() + coreg.TerrainBias("slope")):
        aligned = a.coregister_3d(b, method)
        assert isinstance(aligned, xdem_amd.DEM) and aligned.shape == ref.shape and np.isfinite(aligned.data).any()
    slope = b.get_terrain_attribute("slope")
    step = coreg.BiasCorr(fit_or_bin="bin", bin_sizes=15, bias_var_names=["slope"])
    aligned = a.coregister_3d(b, coreg.NuthKaab() + step, bias_vars={"slope": slope})
    assert isinstance(aligned, xdem_amd.DEM) and "bin_dataframe" in step.meta["outputs"]["fitorbin"]
