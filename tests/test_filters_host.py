"""The rules of ``xdemhip_filter`` on the CPU (tests/filters_oracle.py): the restatements equal SciPy bit for bit for the Gaussian (plain
and normalised), the median, the minimum and the maximum on every case of tests/filters_cases.py; the mean in footprint order stays
within the bound of two summation orders of ``generic_filter(np.nanmean)``; the host-only ``xdemhip_filter_plan`` is consistent; the
kernel weights are SciPy's; and ``filters.py`` / ``DEM.filter`` refuse bad arguments without a GPU."""
import warnings

import numpy as np
import pytest
import scipy.ndimage
from scipy.ndimage._filters import _gaussian_kernel1d

import filters_cases as fc
import filters_oracle as fo
from xdem_amd import DEM, filters

PLANES = [(s, name, dt) for s in (1, 3) for name in fc.NAMES for dt in fc.DTYPES]


def same_bits(a, b) -> bool:
    """Equal dtype, shape, NaN positions and, elsewhere, bits."""
    if a.dtype != b.dtype or a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    u = np.uint32 if a.dtype == np.float32 else np.uint64
    ok = ~np.isnan(a)
    return np.array_equal(np.ascontiguousarray(a).view(u)[ok], np.ascontiguousarray(b).view(u)[ok])


def generic(a, fn, **kw):
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")   # (an all-NaN window, inf - inf)
        return scipy.ndimage.generic_filter(a, fn, mode="constant", cval=np.nan, **kw)


def test_gaussian_equals_scipy_bit_for_bit():
    for s, name, dt in PLANES:
        a = fc.case(s, name, dt)
        nan = np.isnan(a)
        for sigma in fc.SIGMAS:
            with np.errstate(all="ignore"):
                plain = scipy.ndimage.gaussian_filter(a, sigma, mode="reflect", truncate=4.0)
                g = scipy.ndimage.gaussian_filter(np.where(nan, dt(0), a), sigma, mode="reflect", truncate=4.0)
                n = scipy.ndimage.gaussian_filter((~nan).astype(dt), sigma, mode="reflect", truncate=4.0)
                norm = g / n
            norm[nan] = np.nan
            what = (s, name, dt.__name__, sigma)
            assert same_bits(fo.gaussian_filter(a, sigma, normalise=False), plain), what
            assert same_bits(fo.gaussian_filter(a, sigma, normalise=True), norm), what
            assert same_bits(fo.gaussian_filter(a, sigma), norm if nan.any() else plain), what
    assert fo.gaussian_radius(2.5) > max(fc.case(1, "small", np.float32).shape)   # (the mirror repeats there)


def test_median_min_max_equal_scipy_bit_for_bit():
    for s, name, dt in PLANES:
        a = fc.case(s, name, dt)
        for size in fc.SIZES:
            for ours, fn in ((fo.median_filter, np.nanmedian), (fo.min_filter, np.nanmin), (fo.max_filter, np.nanmax)):
                assert same_bits(ours(a, size), generic(a, fn, size=size)), (s, name, dt.__name__, size, fn.__name__)


def test_mean_in_footprint_order_is_within_the_bound_of_two_summation_orders():
    for s, name, dt in PLANES:
        a = fc.case(s, name, dt)
        for kw in ({"size": 3}, {"size": 7}, {"radius": 1}, {"radius": 4}):
            got = fo.mean_filter(a, **kw)
            want = generic(a, np.nanmean, **({"size": kw["size"]} if "size" in kw else {"footprint": fo.disk_footprint(kw["radius"])}))
            assert got.dtype == want.dtype == dt and np.array_equal(np.isnan(got), np.isnan(want)), (s, name, kw)
            fin = np.isfinite(want) & np.isfinite(got)
            assert np.array_equal(got[~fin], want[~fin], equal_nan=True)
            err = np.abs(got[fin].astype(np.float64) - want[fin].astype(np.float64))
            if dt == np.float32:
                assert np.all(err <= np.spacing(np.abs(want[fin]))), (s, name, kw)   # 1 ulp of float32
            else:
                total, n = fo.window_sum(np.abs(a), fo.mean_offsets(**kw))
                bound = 2.0 * (n[fin] - 1) * 2.0 ** -53 * total[fin] / n[fin]
                assert np.all(err <= bound), (s, name, kw)


def test_distance_filter_follows_its_mean_and_removes_some_pixels():
    for s in (1, 3):
        for name in ("elev", "ddem"):
            a = fc.case(s, name, np.float32)
            kw = fc.kwargs_for("distance", {"radius": 3}, name)
            out = fo.distance_filter(a, **kw)
            removed = np.isnan(out) & ~np.isnan(a)
            assert 0 < removed.sum() < (~np.isnan(a)).sum()
            total, n = fo.window_sum(a, fo.disk_offsets(3))
            assert np.array_equal(removed, np.abs(a.astype(np.float64) - total / np.maximum(n, 1)) > kw["outlier_threshold"])
            assert same_bits(out[~removed], a[~removed])


def test_weights_are_scipys():
    for sigma in (0.3, 0.6, 1.0, 2.5, 5.0, 40.0):
        lw = filters.gaussian_radius(sigma)
        assert lw == fo.gaussian_radius(sigma) == int(4.0 * sigma + 0.5)
        want = _gaussian_kernel1d(sigma, 0, lw)
        for got in (filters.gaussian_weights(sigma, lw), fo.gaussian_weights(sigma, lw)):
            assert got.dtype == np.float64 and np.array_equal(got.view(np.uint64), want.view(np.uint64))


def test_plan_is_consistent_and_flips_to_global_exactly_where_the_halo_does_not_fit():
    for kind in filters.KINDS:
        for dt in fc.DTYPES:
            for switch in fc.SWITCHES:
                fits = []
                for radius in range(0, 120):
                    p = filters.filter_plan(100, 100, kind, radius, dt, switch)
                    assert p["halo"] == radius and p["lds_budget"] <= 64 * 1024
                    assert (p["tile_rows"], p["tile_cols"]) == (4, 8) if switch == 3 else p["tile_cols"] == 64 and p["tile_rows"] in (16, 32)
                    fit = p["lds_bytes"] <= p["lds_budget"]
                    assert p["route"] == ("tile" if fit and switch != 2 else "global"), (kind, dt, switch, radius)
                    item = 4 if dt == np.float32 else 8
                    assert p["lds_bytes"] >= (p["tile_rows"] + 2 * radius) * (p["tile_cols"] + 2 * radius) * item
                    fits.append(fit)
                assert fits[0] and not fits[-1] and fits == sorted(fits, reverse=True), (kind, dt, switch)   # (one flip, from fitting to not)
    assert fc.big_shape(1) == (2 * 32 + 3, 2 * 64 + 5) and fc.big_shape(3) == (2 * 4 + 3, 2 * 8 + 5)
    for bad in ((0, 5, "median", 1, np.float32, 0), (5, 5, 9, 1, np.float32, 0), (5, 5, "median", -1, np.float32, 0),
                (5, 5, "median", 1, np.float32, 4)):
        with pytest.raises(ValueError):
            filters.filter_plan(*bad)


def test_filters_refuse_bad_arguments_on_the_host():
    a = fc.case(3, "elev", np.float32)
    for call in (lambda: filters.gaussian_filter(a, 0.0), lambda: filters.gaussian_filter(a, -1.0), lambda: filters.gaussian_filter(a, np.nan),
                 lambda: filters.gaussian_filter(a, 1.0, truncate=-1.0), lambda: filters.gaussian_filter(a, 1.0, normalise="yes"),
                 lambda: filters.median_filter(a, 4), lambda: filters.median_filter(a, 1), lambda: filters.min_filter(a, 2.5),
                 lambda: filters.max_filter(a, -3), lambda: filters.mean_filter(a), lambda: filters.mean_filter(a, size=3, radius=1),
                 lambda: filters.mean_filter(a, size=6), lambda: filters.mean_filter(a, radius=-1), lambda: filters.mean_filter(a, radius=1.5),
                 lambda: filters.distance_filter(a, -1, 1.0), lambda: filters.distance_filter(a, 2, np.nan),
                 lambda: filters.median_filter(a[0], 3), lambda: filters.median_filter(np.zeros((2, 3, 4), np.float32), 3),
                 lambda: filters.filter_array(a, "bilateral"), lambda: filters.filter_array(a, lambda x: x[1:])):
        with pytest.raises(ValueError):
            call()
    for call in (lambda: filters.median_filter(a, 2 * 16384 + 1), lambda: filters.mean_filter(a, radius=16384),
                 lambda: filters.gaussian_filter(a, 1e6)):
        with pytest.raises(NotImplementedError):
            call()


def test_dem_filter_dispatch_on_the_host():
    dem = DEM(fc.case(3, "elev", np.float32).copy(), (2.0, 0.0, 10.0, 0.0, -2.0, 50.0), crs="EPSG:32633", nodata=-9999)
    with pytest.raises(ValueError):
        dem.filter("bilateral")
    with pytest.raises(ValueError):
        dem.filter("median", size=4)
    with pytest.raises(TypeError):
        dem.filter("median", sigma=1.0)
    out = dem.filter(lambda x: x + 1)
    assert isinstance(out, DEM) and out is not dem and np.array_equal(out.data, dem.data + 1, equal_nan=True)
    assert (out.transform, out.crs, out.nodata) == (dem.transform, dem.crs, dem.nodata)
    before = dem.data.copy()
    assert dem.filter(lambda x: x * 2, inplace=True) is None and np.array_equal(dem.data, before * 2, equal_nan=True)
