"""``xdemhip_filter`` on the GPU against the restatement of its rules (tests/filters_oracle.py): every filter and parameter set of
tests/filters_cases.py on every case, under every value of the test switch ``"filter_route"`` (0 automatic, 1 tiled, 2 global taps,
3 minimal tiles), for float32 and float64, from host and from device memory -- bit for bit, NaN positions included, from two runs, the
result where the input lives.  Then halos beyond the LDS budget (the automatic switch to the global route), the status codes of refused
arguments, ``distance_filter``'s removed pixels, and ``DEM.filter`` end to end.  The planes are sized from ``xdemhip_filter_plan``:
(2 T_r + 3) x (2 T_c + 5), the smallest that has nine partial tiles."""
import functools

import numpy as np
import pytest

import filters_cases as fc
import filters_oracle as fo
from gpu_helpers import _dev
from xdem_amd import DEM, _args, _lib, dDEM, filters
from xdem_amd.ddem import raster_of

pytestmark = pytest.mark.gpu

EINVAL, EUNSUPPORTED = -1, -5


@pytest.fixture(scope="module")
def ctx():
    return _lib.default_context()


@functools.lru_cache(maxsize=None)
def oracle(plan_switch, name, dtype, method, kw_items):
    """What the rule gives on a case: computed once, read-only, shared among the switches."""
    out = fo.FILTERS[method](fc.case(plan_switch, name, dtype), **dict(kw_items))
    out.setflags(write=False)
    return out


def host(x):
    return x.cpu().numpy() if _args.is_tensor(x) else x


def same_bits(a, b) -> bool:
    """Equal dtype, shape, NaN positions and, elsewhere, bits."""
    if a.dtype != b.dtype or a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    u = np.uint32 if a.dtype == np.float32 else np.uint64
    ok = ~np.isnan(a)
    return np.array_equal(np.ascontiguousarray(a).view(u)[ok], np.ascontiguousarray(b).view(u)[ok])


@pytest.mark.parametrize("switch", fc.SWITCHES)
@pytest.mark.parametrize("method,kw", fc.FILTERS, ids=[fc.label(m, k) for m, k in fc.FILTERS])
def test_every_route_returns_the_oracles_bits(ctx, method, kw, switch):
    with ctx.option_scope("filter_route", switch):
        for name in fc.NAMES:
            for dt in fc.DTYPES:
                a = fc.case(switch, name, dt)
                kwargs = fc.kwargs_for(method, kw, name)
                want = oracle(fc.plan_switch(switch), name, dt, method, tuple(sorted(kwargs.items())))
                what = (name, dt.__name__)
                first = filters.filter_array(a, method, ctx=ctx, **kwargs)
                assert isinstance(first, np.ndarray) and same_bits(first, want), what + ("host",)
                on_device = filters.filter_array(_dev(np.array(a)), method, ctx=ctx, **kwargs)
                assert _args.is_tensor(on_device) and on_device.is_cuda, what   # (the result keeps the caller's memory space)
                assert same_bits(host(on_device), want), what + ("device",)
                again = filters.filter_array(a, method, ctx=ctx, **kwargs)
                assert np.array_equal(first.view(np.uint8), again.view(np.uint8)), what + ("second run",)


def test_planes_cross_tiles_and_routes_are_what_the_cases_say():
    for switch, tile in ((1, (32, 64)), (3, (4, 8))):
        H, W = fc.big_shape(switch)
        assert (H, W) == (2 * tile[0] + 3, 2 * tile[1] + 5)
        for method, kw in fc.FILTERS:
            for dt in fc.DTYPES:
                p = filters.filter_plan(H, W, method, fc.halo_of(method, kw), dt, switch)
                assert p["route"] == "tile" and p["lds_bytes"] <= p["lds_budget"]
                # (the largest tile sizes the plane; a parameter set whose halo leaves room for the smaller tile only crosses more borders)
                assert p["tile_rows"] <= tile[0] and p["tile_cols"] <= tile[1] and H % p["tile_rows"] and W % p["tile_cols"]
                assert filters.filter_plan(H, W, method, fc.halo_of(method, kw), dt, 2)["route"] == "global"


BEYOND = [("gaussian", {"sigma": 6.0}, np.float64), ("gaussian", {"sigma": 12.0, "normalise": True}, np.float32),
          ("median", {"size": 61}, np.float64), ("mean", {"radius": 30}, np.float64), ("max", {"size": 91}, np.float32),
          ("distance", {"radius": 45, "outlier_threshold": 110.0}, np.float32)]


@pytest.mark.parametrize("method,kw,dt", BEYOND, ids=[fc.label(m, k) for m, k, _ in BEYOND])
def test_halo_beyond_the_lds_budget_takes_the_global_route_by_itself(ctx, method, kw, dt):
    rng = np.random.default_rng(23)
    a = (1500.0 + 100.0 * rng.standard_normal((23, 38))).astype(dt)   # (smaller than the window: the mirror repeats, every window is clipped)
    a[rng.random(a.shape) < 0.1] = np.nan
    halo = fc.halo_of(method, kw)
    assert filters.filter_plan(*a.shape, method, halo, dt, 0)["route"] == "global"
    assert filters.filter_plan(*a.shape, method, 8 if dt == np.float32 else 5, dt, 0)["route"] == "tile"
    want = fo.FILTERS[method](a, **kw)
    for switch in (0, 1):
        with ctx.option_scope("filter_route", switch):
            assert same_bits(filters.filter_array(a, method, ctx=ctx, **kw), want)
            assert same_bits(host(filters.filter_array(_dev(a), method, ctx=ctx, **kw)), want)


def test_refused_arguments_return_status_codes(ctx):
    L = ctx._L
    a = np.ascontiguousarray(fc.case(3, "elev", np.float32))
    out = np.empty_like(a)
    H, W = a.shape
    w = filters.gaussian_weights(1.0, 4)

    def call(kind, size=0, radius=0, sigma=0.0, truncate=0.0, weights=None, normalise=0, src=a, dst=out, dtype=_lib.F32, h=H, w_=W, space=_lib.HOST):
        return L.xdemhip_filter(ctx.handle, _args.ptr(src), dtype, h, w_, kind, size, radius, sigma, truncate,
                                None if weights is None else _args.c_doubles(weights), normalise, 1.0, _args.ptr(dst), space)

    assert call(filters.MEDIAN, size=3) == _lib.OK
    assert call(filters.GAUSSIAN, radius=4, sigma=1.0, truncate=4.0, weights=w, normalise=2) == _lib.OK
    for kind in (filters.MEDIAN, filters.MIN, filters.MAX, filters.MEAN):
        for size in (4, 2, 1, -3):
            assert call(kind, size=size) == EINVAL
    assert call(filters.MEDIAN, size=0) == EINVAL and call(filters.MEDIAN, size=3, radius=1) == EINVAL
    assert call(filters.MEAN, size=3, radius=1) == EINVAL and call(filters.MEAN, radius=-1) == EINVAL
    assert call(filters.DISTANCE, radius=-1) == EINVAL and call(filters.DISTANCE, size=3) == EINVAL
    for sigma in (0.0, -1.0, float("nan"), float("inf")):
        assert call(filters.GAUSSIAN, radius=4, sigma=sigma, truncate=4.0, weights=w) == EINVAL
    assert call(filters.GAUSSIAN, radius=4, sigma=1.0, truncate=-1.0, weights=w) == EINVAL
    assert call(filters.GAUSSIAN, radius=3, sigma=1.0, truncate=4.0, weights=w) == EINVAL        # (radius is not int(truncate * sigma + 0.5))
    assert call(filters.GAUSSIAN, radius=4, sigma=1.0, truncate=4.0) == EINVAL                   # (no weights)
    assert call(filters.GAUSSIAN, radius=4, sigma=1.0, truncate=4.0, weights=w, normalise=3) == EINVAL
    assert call(6, size=3) == EINVAL and call(-1, size=3) == EINVAL
    assert call(filters.MEDIAN, size=3, h=0) == EINVAL and call(filters.MEDIAN, size=3, w_=0) == EINVAL and call(filters.MEDIAN, size=3, h=-2) == EINVAL
    assert call(filters.MEDIAN, size=3, dtype=2) == EINVAL and call(filters.MEDIAN, size=3, dtype=7) == EINVAL
    assert call(filters.MEDIAN, size=3, space=5) == EINVAL
    assert call(filters.MEDIAN, size=3, dst=a) == EINVAL                                           # (out aliases in)
    assert call(filters.MEDIAN, size=3, src=a.reshape(-1)[W:], dst=a, h=H - 1) == EINVAL           # (out overlaps in)
    assert L.xdemhip_filter(ctx.handle, None, _lib.F32, H, W, filters.MEDIAN, 3, 0, 0.0, 0.0, None, 0, 0.0, _args.ptr(out), _lib.HOST) == EINVAL
    assert L.xdemhip_filter(ctx.handle, _args.ptr(a), _lib.F32, H, W, filters.MEDIAN, 3, 0, 0.0, 0.0, None, 0, 0.0, None, _lib.HOST) == EINVAL
    assert call(filters.MEDIAN, size=2 * 16384 + 1) == EUNSUPPORTED and call(filters.MEAN, radius=16384) == EUNSUPPORTED
    assert call(filters.GAUSSIAN, radius=1 << 21, sigma=float(1 << 19), truncate=4.0, weights=w) == EUNSUPPORTED
    d = _dev(np.array(a))
    assert call(filters.MEDIAN, size=3, src=d, dst=d, space=_lib.DEVICE) == EINVAL
    with pytest.raises(_lib.XdemHipError):
        ctx.set_option("filter_route", 4)
    assert call(filters.MEDIAN, size=3) == _lib.OK                         # (the context still works)
    assert same_bits(out, fo.median_filter(a, 3))


def test_sides_of_one_pixel_and_a_single_pixel(ctx):
    for shape in ((1, 1), (1, 2), (3, 1)):
        a = np.full(shape, 7.5, dtype=np.float32)
        for method, kw in fc.FILTERS:
            kwargs = fc.kwargs_for(method, kw, "elev")
            assert same_bits(filters.filter_array(a, method, ctx=ctx, **kwargs), fo.FILTERS[method](a, **kwargs)), (shape, method, kw)


def test_distance_filter_removes_exactly_the_oracles_pixels(ctx):
    for switch in (1, 3):
        with ctx.option_scope("filter_route", switch):
            for name in ("elev", "ddem"):
                for dt in fc.DTYPES:
                    a = fc.case(switch, name, dt)
                    kw = fc.kwargs_for("distance", {"radius": 3}, name)
                    got = filters.distance_filter(a, ctx=ctx, **kw)
                    want = fo.distance_filter(a, **kw)
                    removed = np.isnan(got) & ~np.isnan(a)
                    assert np.array_equal(removed, np.isnan(want) & ~np.isnan(a)) and 0 < removed.sum() < (~np.isnan(a)).sum()
                    assert same_bits(got[~removed], a[~removed])   # (every other pixel is the input's)


def test_dem_filter_end_to_end(ctx):
    a = fc.case(1, "ddem", np.float32).copy()
    raw = np.where(np.isnan(a), np.float32(-9999), a)
    t = (2.0, 0.0, 10.0, 0.0, -2.0, 50.0)
    dem = DEM(raw, t, crs="EPSG:32633", nodata=-9999)
    assert np.array_equal(np.isnan(dem.data), np.isnan(a))   # (nodata became NaN when the DEM was made)
    out = dem.filter("median", size=5)
    assert isinstance(out, DEM) and out is not dem and (out.transform, out.crs, out.nodata) == (dem.transform, "EPSG:32633", -9999)
    assert same_bits(out.data, fo.median_filter(a, 5)) and same_bits(dem.data, a)
    assert same_bits(dem.filter("gaussian", sigma=2.5).data, fo.gaussian_filter(a, 2.5))
    assert same_bits(dem.filter("mean", radius=4).data, fo.mean_filter(a, radius=4))
    assert same_bits(dem.filter("distance", radius=3, outlier_threshold=6.0).data, fo.distance_filter(a, 3, 6.0))
    assert same_bits(dem.filter(lambda x: filters.max_filter(x, 3)).data, fo.max_filter(a, 3))
    twin = dem.copy()
    assert twin.filter("min", size=3, inplace=True) is None and same_bits(twin.data, fo.min_filter(a, 3))
    # an integer DEM is filtered as float32
    ints = DEM(np.arange(1, 36, dtype=np.int16).reshape(5, 7), t)
    assert same_bits(ints.filter("mean", size=3).data, fo.mean_filter(np.arange(1, 36, dtype=np.float32).reshape(5, 7), size=3))
    # a DEM around a device tensor stays on the device
    on_device = raster_of(_dev(np.array(a)), t, "EPSG:32633", -9999).filter("median", size=9)
    assert _args.is_tensor(on_device.data) and same_bits(host(on_device.data), fo.median_filter(a, 9))
    # dDEM inherits the method and keeps its times
    dd = dDEM(DEM(a.copy(), t), np.datetime64("2000-01-01"), np.datetime64("2010-01-01"))
    smooth = dd.filter("gaussian", sigma=0.6)
    assert isinstance(smooth, dDEM) and smooth.start_time == dd.start_time and smooth.end_time == dd.end_time
    assert same_bits(smooth.data, fo.gaussian_filter(a, 0.6)) and same_bits(dd.data, a)
