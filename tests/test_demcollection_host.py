"""xdem_amd.dDEM and xdem_amd.DEMCollection without a GPU: the product's host code over the NumPy restatement of the stack
(demstack_oracle.OracleStack), against what the reference's own classes returned (tools/gen_golden_demcollection.py)."""
import inspect
import json
import os
import warnings

import numpy as np
import pytest

import demcollection_cases as dc
import demstack_oracle
from xdem_amd import DEM, DEMCollection, dDEM, demcollection, volume


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(dc.GOLDEN, "signatures_ddem.json")) as f:
        return json.load(f)


def dems_of(s: dict) -> list:
    return [DEM.from_array(d, dc.TRANSFORM, None) for d in s["dems"]]


def message_of(fn) -> str:
    try:
        fn()
    except Exception as e:  # noqa: BLE001
        return f"{type(e).__name__}: {e}"
    raise AssertionError("no error raised")


def test_signatures_match_the_reference(recorded):
    classes = {"dDEM": dDEM, "DEMCollection": DEMCollection}
    assert len(recorded["signatures"]) == 11
    for name, params in recorded["signatures"].items():
        cls, method = name.split(".")
        sig = inspect.signature(getattr(classes[cls], method))
        assert [p["name"] for p in params] == list(sig.parameters), name
        for p in params:
            q = sig.parameters[p["name"]]
            assert q.kind.name == p["kind"], (name, p["name"])
            if p["default"] == "<required>":
                assert q.default is inspect.Parameter.empty, (name, p["name"])
            else:
                assert q.default == p["default"], (name, p["name"])
    for cls, names in recorded["properties"].items():
        for prop in names:
            assert isinstance(vars(classes[cls])[prop], property), (cls, prop)
    assert vars(dDEM)["filled_data"].fset is not None


@pytest.mark.parametrize("name", ["sorted_first", "sorted_third", "unsorted_first", "unsorted_object"])
def test_constructor_matches_the_reference(name):
    """Upstream sorts the DEMs by time and leaves the stamps unsorted: with stamps 2010, 1990, 2020, 2000 and reference_dem=0 the
    reference index is 2 and the reference timestamp 2020 (the third of the UNSORTED stamps)."""
    g = dc.golden()
    years, reference = {"sorted_first": ((1990, 2000, 2010, 2020), 0), "sorted_third": ((1990, 2000, 2010, 2020), 2),
                        "unsorted_first": ((2010, 1990, 2020, 2000), 0), "unsorted_object": ((2010, 1990, 2020, 2000), 1)}[name]
    dems = [DEM(np.full((3, 4), float(i), np.float32), dc.TRANSFORM) for i in range(4)]
    col = DEMCollection(dems, timestamps=dc.stamps(years), reference_dem=dems[reference] if name.endswith("object") else reference)
    assert col.reference_index == g[f"ctor_{name}_index"]
    assert np.array_equal(col.timestamps.astype(np.int64), g[f"ctor_{name}_timestamps"]) and col.timestamps.dtype == np.dtype("datetime64[ns]")
    assert col.reference_timestamp.astype(np.int64) == g[f"ctor_{name}_reference_timestamp"]
    assert [int(d.data[0, 0]) for d in col.dems] == list(g[f"ctor_{name}_order"])
    assert col.reference_dem is col.dems[col.reference_index] and col.ddems == [] and col.outlines == {}
    if name == "unsorted_first":
        assert col.reference_index == 2 and col.reference_timestamp == np.datetime64("2020-01-01")


def test_timestamps_from_the_dems():
    dems = [DEM(np.zeros((3, 4), np.float32), dc.TRANSFORM) for _ in range(2)]
    for d, stamp in zip(dems, dc.stamps((2001, 2002))):
        d.datetime = stamp
    assert np.array_equal(DEMCollection(dems).timestamps, np.array(dc.stamps((2001, 2002))).astype("datetime64[ns]"))


@pytest.mark.parametrize("dtype", dc.DTYPES)
@pytest.mark.parametrize("H,W", dc.SHAPES)
def test_series_match_the_reference(H, W, dtype, recorded):
    g, s = dc.golden(), dc.stack(H, W, dtype)
    full = np.ones((H, W), bool)
    worst = 0.0
    with demstack_oracle.patched():
        col = DEMCollection(dems_of(s), timestamps=dc.stamps(), outlines=s["mask"], reference_dem=dc.REFERENCE)
        ddems = col.subtract_dems()
        ref = s["dems"][dc.REFERENCE]
        for t, d in enumerate(ddems):
            with np.errstate(invalid="ignore"):
                want = np.zeros_like(ref) if t == dc.REFERENCE else ref - s["dems"][t]
            assert d.data.dtype == want.dtype and np.array_equal(d.data, want, equal_nan=True)
            assert (d.error == 0) if t == dc.REFERENCE else (d.error is None)
            assert (d.filled_data is None) == (t != dc.REFERENCE) and d.fill_method == ""
        assert ddems[0].time == np.datetime64("2005-01-01") - np.datetime64("2000-01-01") and float(ddems[dc.REFERENCE].time) == 0
        others = [d for t, d in enumerate(ddems) if t != dc.REFERENCE]
        for variant, kw in (("raw_full", {"mask": full}), ("raw_mask", {})):
            prefix = f"{H}x{W}_{dtype}_{variant}"
            worst = max(worst, dc.assert_series(dc.series_of(col, **kw), g, prefix, dtype, [d.data for d in others], kw.get("mask", s["mask"]),
                                             recorded["warnings"][prefix]))
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            filled = col.interpolate_ddems(method="regional_hypsometric")
        for t, d in enumerate(ddems):
            per_pair = volume.hypsometric_interpolation(d.data, ref, s["mask"])
            assert np.array_equal(filled[t], per_pair.data, equal_nan=True) and filled[t].dtype == per_pair.dtype and d.fill_method == ""
            assert d.filled_data is filled[t] or np.shares_memory(d.filled_data, filled[t])
        for variant, kw in (("filled_full", {"mask": full}), ("filled_mask", {})):
            prefix = f"{H}x{W}_{dtype}_{variant}"
            worst = max(worst, dc.assert_series(dc.series_of(col, **kw), g, prefix, dtype, [d.filled_data for d in others], kw.get("mask", s["mask"]),
                                             recorded["warnings"][prefix]))
    print(f"{H}x{W} {dtype}: largest |dh - recorded| / mean|x| {worst:.3e}")


def small_collection(outlines=None, years=dc.YEARS):
    s = dc.stack(61, 83, "float32")
    col = DEMCollection(dems_of(s), timestamps=dc.stamps(years), outlines=outlines, reference_dem=dc.REFERENCE)
    col.subtract_dems()
    return s, col


def test_mask_rules():
    """get_ddem_mask: start and end -> union; start only; one outline in all; no fitting key -> every pixel."""
    s = dc.stack(61, 83, "float32")
    a, b, c = s["mask"], np.roll(s["mask"], 7, axis=1), np.roll(s["mask"], -5, axis=0)
    t = np.array(dc.stamps()).astype("datetime64[ns]")
    with demstack_oracle.patched():
        _, col = small_collection(a)
        assert list(col.outlines) == [t[dc.REFERENCE]]
        for d in col.ddems:
            assert np.array_equal(col.get_ddem_mask(d), a)            # a single outline
        _, col = small_collection({dc.stamps()[0]: a, dc.stamps()[1]: b, dc.stamps()[3]: c})
        m = [col.get_ddem_mask(d) for d in col.ddems]
        assert np.array_equal(m[0], a | b)                            # 2000 - 2005: both keys
        assert np.array_equal(m[1], b)                                # 2005 - 2005
        assert np.array_equal(m[2], b)                                # 2005 - 2010: the start only
        assert np.array_equal(m[3], b | c)
        _, col = small_collection({np.datetime64("1980-01-01"): a, np.datetime64("1981-01-01"): b})
        assert all(col.get_ddem_mask(d).all() and col.get_ddem_mask(d).shape == (61, 83) for d in col.ddems)   # no fitting key
        # K = T masks with a union reach the stack as distinct masks: the series over them are the per-dDEM figures
        _, col = small_collection({dc.stamps()[0]: a, dc.stamps()[1]: b, dc.stamps()[3]: c})
        dh = col.get_dh_series(nans_ok=True)
        for row, (j, want) in enumerate(zip((0, 2, 3), (a | b, b, b | c))):
            n, mean, _ = dc.moments(col.ddems[j].data[want])
            assert dh["area"].iloc[row] == np.count_nonzero(want) * 900.0
            assert dh["dh"].iloc[row] == mean


def test_errors_and_warnings(recorded):
    msg = recorded["messages"]
    dems = [DEM(np.zeros((3, 4), np.float32), dc.TRANSFORM) for _ in range(2)]
    two = dc.stamps((2000, 2010))
    assert message_of(lambda: DEMCollection(dems)) == msg["no_timestamps"]
    assert message_of(lambda: DEMCollection(dems, timestamps=two, outlines={two[0]: 3})) == msg["bad_outlines"]
    assert message_of(lambda: DEMCollection(dems, timestamps=two).get_dh_series()) == msg["not_calculated"]
    one = dDEM.from_array(np.zeros((3, 4), np.float32), dc.TRANSFORM, None, two[0], two[1])
    assert message_of(lambda: setattr(one, "filled_data", np.zeros(5))) == msg["filled_size"]
    assert message_of(lambda: one.interpolate(method="linear")) == msg["bad_method"]
    assert message_of(lambda: one.interpolate(method="regional_hypsometric", reference_elevation=np.zeros((2, 2)), mask=np.ones((3, 4), bool))) == msg["reference_shape"]
    with demstack_oracle.patched():
        _, col = small_collection()
        assert message_of(lambda: col.get_ddem_mask(one)) == msg["foreign_ddem"]
        assert message_of(lambda: col.get_cumulative_series(kind="dz")) == msg["bad_kind"]
        with pytest.warns(UserWarning, match=r"NaNs found in dDEM \(2000-01-01T00:00:00.000000000 - 2005-01-01T00:00:00.000000000\)\."):
            col.get_dh_series()
        # a mask without an inlier: the warning of hypsometric_interpolation, the plane copied, dh = NaN
        _, col = small_collection(np.zeros((61, 83), bool))
        with pytest.warns(UserWarning, match="No valid data found within mask, returning copy"):
            filled = col.interpolate_ddems("regional_hypsometric")
        assert all(np.array_equal(f, d.data, equal_nan=True) for f, d in zip(filled, col.ddems))
        assert np.isnan(col.get_dh_series(nans_ok=True)["dh"]).all() and (col.get_dh_series(nans_ok=True)["area"] == 0).all()


def test_refusals():
    s = dc.stack(61, 83, "float32")
    two = dc.stamps((2000, 2010))
    one = dDEM.from_array(np.zeros((3, 4), np.float32), dc.TRANSFORM, None, two[0], two[1])
    for method in ("idw", "local_hypsometric"):
        with pytest.raises(NotImplementedError, match="fillnodata"):
            one.interpolate(method=method)
    with pytest.raises(NotImplementedError, match="fillnodata"):
        one.interpolate()   # (upstream's default)
    with demstack_oracle.patched():
        _, col = small_collection(s["mask"])
        with pytest.raises(NotImplementedError, match="Interpolation method 'linear' not supported"):
            col.interpolate_ddems()   # (upstream's default is a method dDEM.interpolate refuses)
        with pytest.raises(NotImplementedError, match="pandas query"):
            col.get_ddem_mask(col.ddems[0], outlines_filter="name == 'x'")
        with pytest.raises(NotImplementedError, match="pandas query"):
            col.get_dh_series(outlines_filter="name == 'x'")
    other = DEM(np.zeros((61, 83), np.float32), (10.0, 0.0, 0.0, 0.0, -10.0, 0.0))
    col = DEMCollection([dems_of(s)[0], other], timestamps=two)
    with pytest.raises(NotImplementedError, match="reprojection is geoutils' job"):
        col.subtract_dems()
    with pytest.raises(ValueError, match=f"1 to {demcollection.MAX_PLANES} DEMs"):
        demstack_oracle.OracleStack([np.zeros(4, np.float32)] * (demcollection.MAX_PLANES + 1), 0)
    assert not hasattr(volume, "idw_interpolation") and not hasattr(volume, "local_hypsometric_interpolation")


def test_ddem_state():
    s = dc.stack(61, 83, "float32")
    two = dc.stamps((2000, 2010))
    raster = DEM.from_array(s["dems"][0], dc.TRANSFORM, None)
    d = dDEM(raster, two[0], two[1], error=1.5)
    assert d.data is raster.data and d.transform == raster.transform and d.res == (30.0, 30.0)   # (the raster's state, taken over)
    assert d.time == two[1] - two[0] and d.error == 1.5 and d.fill_method == "" and d.filled_data is None
    assert str(d).startswith("dDEM from 2000-01-01 to 2010-01-01.\n\n")
    c = d.copy()
    assert c.data is not d.data and np.array_equal(c.data, d.data, equal_nan=True) and (c.start_time, c.end_time) == (two[0], two[1])
    full = dDEM.from_array(np.ones((3, 4), np.float32), dc.TRANSFORM, None, two[0], two[1])
    assert np.array_equal(full.filled_data, full.data)
    full.filled_data = np.arange(12.0)
    assert full.filled_data.shape == (3, 4) and full.fill_method == ""
    # a DEM of a mask: the true value is the maximum, unless that is 0
    with demstack_oracle.patched():
        ref = s["dems"][dc.REFERENCE]
        with np.errstate(invalid="ignore"):
            dd = dDEM.from_array(ref - s["dems"][0], dc.TRANSFORM, None, two[0], two[1])
        want = volume.hypsometric_interpolation(dd.data, ref, s["mask"]).data
        got = dd.interpolate("regional_hypsometric", reference_elevation=DEM.from_array(ref, dc.TRANSFORM), mask=DEM.from_array(s["mask"].astype(np.uint8) * 7, dc.TRANSFORM))
        assert np.array_equal(got, want, equal_nan=True) and dd.filled_data is got and dd.fill_method == ""


def test_every_plane_its_own_mask():
    """K = T: an outline for every stamp, so that every dDEM has a mask of its own (three of them unions)."""
    s = dc.stack(61, 83, "float32")
    a = s["mask"]
    outlines = dict(zip(dc.stamps(), (np.roll(a, 7, axis=1), a, np.roll(a, -5, axis=0), np.roll(a, 3, axis=0))))
    with demstack_oracle.patched():
        _, col = small_collection(outlines)
        dh = col.get_dh_series(nans_ok=True)
        assert len(col._plan.masks) == len(col.ddems) == 4 and col._plan.mask_ids.tolist() == [0, 1, 2, 3]
        for row, j in enumerate((0, 2, 3)):
            want = a | outlines[dc.stamps()[j]]
            assert np.array_equal(col.get_ddem_mask(col.ddems[j]), want)
            assert dh["dh"].iloc[row] == dc.moments(col.ddems[j].data[want])[1] and dh["area"].iloc[row] == np.count_nonzero(want) * 900.0


def test_reference_dem_given_as_an_object():
    """A raster that is no xdem_amd.DEM is rebuilt as one, as upstream does, and is still found as the reference; an object that is
    none of the rasters is refused with a message."""
    import types

    rasters = [types.SimpleNamespace(data=np.full((3, 4), float(i), np.float32), transform=dc.TRANSFORM, crs=None, nodata=None) for i in range(3)]
    col = DEMCollection(rasters, timestamps=dc.stamps((2010, 1990, 2000)), reference_dem=rasters[0])
    assert all(isinstance(d, DEM) for d in col.dems) and col.reference_index == 2 and col.reference_dem.data[0, 0] == 0.0
    stranger = DEM(np.zeros((3, 4), np.float32), dc.TRANSFORM)
    with pytest.raises(ValueError, match="`reference_dem` must be an index into `dems` or one of the `dems`"):
        DEMCollection(rasters, timestamps=dc.stamps((2010, 1990, 2000)), reference_dem=stranger)


def test_an_infinity_is_a_void_on_both_routes():
    """filled_data is None for a dDEM with an infinity and no NaN, whether the dDEM stands alone or comes from a collection."""
    ref = np.full((5, 6), 1000.0, np.float32)
    dem = ref - 1.0
    dem[2, 3] = np.inf
    two = dc.stamps((2000, 2010))
    alone = dDEM.from_array(ref - dem, dc.TRANSFORM, None, two[0], two[1])
    assert not np.isnan(alone.data).any() and alone.filled_data is None
    with demstack_oracle.patched():
        col = DEMCollection([DEM(ref, dc.TRANSFORM), DEM(dem, dc.TRANSFORM)], timestamps=two)
        assert col.subtract_dems()[1].filled_data is None and col.ddems[0].filled_data is not None


def test_inliers_within_one_bin():
    """A reference whose inliers span less than one 50 m bin: SciPy's interpolant of one point returns NaN, and so does the batched fill
    for that plane's voids inside the mask -- the other planes are filled as ever."""
    s = dc.stack(61, 83, "float32")
    ref = np.full((61, 83), 1000.0, np.float32)
    ref[:, :40] += 20.0
    with np.errstate(invalid="ignore"):
        dem = (ref - (s["dems"][dc.REFERENCE] - s["dems"][0])).astype(np.float32)
    with demstack_oracle.patched():
        col = DEMCollection([DEM.from_array(ref, dc.TRANSFORM), DEM.from_array(dem, dc.TRANSFORM)], timestamps=dc.stamps((2000, 2010)), outlines=s["mask"])
        d = col.subtract_dems()[1]
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            filled = col.interpolate_ddems("regional_hypsometric")[1]
    voids = ~np.isfinite(d.data)
    assert (voids & s["mask"]).any() and np.isnan(filled[voids]).all() and np.array_equal(filled[~voids], d.data[~voids])
