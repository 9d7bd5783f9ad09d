"""xdemhip_spline_prepare / _gather / xdemhip_raster_points on the GPU against the NumPy restatement of their rule
(tests/interp_oracle.py): the coefficient plane within 1e-12 x max |raster| of the oracle under every value of the test switch
``"spline_route"`` (0 automatic, 1 one band per column, 2 plain rows, 3 LDS rows), the values of the four methods (orders 0 and 1 bit
for bit, 3 and 5 within the bound, the NaN set and the count identical), every form of ``dist_nodata_spread``, the fast paths, plan
reuse, the round trip through ``to_pointcloud`` and the ``DEM`` methods.  float32 and float64, host and device memory.  The shapes
come from ``xdemhip_spline_plan`` (tests/interp_cases.py)."""
import functools

import numpy as np
import pytest

import interp_cases as ic
import interp_oracle as io
from gpu_helpers import _dev
from xdem_amd import DEM, EPC, _lib, interp

pytestmark = pytest.mark.gpu

BOUND = 1e-12   # x max |finite raster value|
METHODS = ("nearest", "linear", "cubic", "quintic")


@pytest.fixture(scope="module")
def ctx():
    return _lib.default_context()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


def host(a):
    return a.cpu().numpy() if hasattr(a, "is_cuda") else a


@functools.lru_cache(maxsize=None)
def raster(name, dtype, kind):
    a = ic.with_voids(ic.surface(ic.shapes()[name], np.dtype(dtype)), kind)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def prepared(name, dtype, kind, order, dist):
    """The oracle's plan of a case (shared among the tests that need it)."""
    return io.Prepared(raster(name, dtype, kind), order, dist)


def scale(a):
    return np.abs(a[np.isfinite(a)]).max()


def close(got, want, a, order):
    """Orders 0 and 1 bit for bit; 3 and 5 within the bound; the NaN set identical."""
    if got.dtype != want.dtype or not np.array_equal(np.isnan(got), np.isnan(want)):
        return False
    if order <= 1:
        return np.array_equal(bits(got), bits(want))
    ok = ~np.isnan(want)
    return bool(np.all(np.abs(got[ok].astype(np.float64) - want[ok].astype(np.float64)) <= BOUND * scale(a)))


def sampled(plan, want, a, x, y, transform, device=False, shift=False):
    """One gather of a plan against the oracle's plan ``want``.  The bound is on the float64 value: for a float32 raster at orders 3
    and 5 it is asked before the one rounding (two float64 values within the bound may round to neighbouring float32 values), and the
    float32 result must be that float64 result rounded once."""
    pts = (_dev(x), _dev(y)) if device else (x, y)
    got = plan.at(pts, shift)
    if hasattr(got, "is_cuda") != device:
        return False
    got = host(got)
    w64 = want.values64(*io.pixel_coordinates(x, y, transform, shift))
    if plan.n_valid != int((~np.isnan(w64)).sum()) or got.dtype != a.dtype:
        return False
    if plan.order <= 1 or a.dtype == np.float64:
        return close(got, w64.astype(a.dtype), a, plan.order)
    g64 = host(plan.at(pts, shift, dtype=np.float64))
    return close(g64, w64, a, plan.order) and np.array_equal(bits(got), bits(g64.astype(np.float32)))


@pytest.mark.parametrize("switch", ic.SWITCHES)
@pytest.mark.parametrize("order", (3, 5))
def test_coefficients_every_case(ctx, switch, order):
    with ctx.option_scope("spline_route", switch):
        for k, name in enumerate(ic.shapes()):
            for dtype, kind in (("float32", "none"), ("float64", "blobs")):
                a = raster(name, dtype, kind)
                want = prepared(name, dtype, kind, order, io.spread_distance(order))
                with interp.InterpPlan(_dev(a) if (k + switch) % 2 else a, ic.EXACT, order, ctx=ctx) as plan:
                    spread, coef = plan.planes()
                    assert plan.n_nonfinite == want.n_nonfinite, (name, kind)
                err = np.abs(coef - want.coef).max() / scale(a)
                print(f"switch {switch} order {order} {name} {dtype} {kind}: coefficient error / max |a| = {err:.3e}")
                assert err <= BOUND, (name, dtype, kind)
                if want.spread is None:
                    assert spread is None
                else:
                    assert np.array_equal(spread != 0, want.spread), (name, kind)


@pytest.mark.parametrize("order", (3, 5))
def test_routes_agree(ctx, order):
    """All four routes on the three-by-three raster: within the bound of each other (printed: whether bit for bit)."""
    a = raster("three_by_three", "float32", "blobs")
    planes = []
    for switch in ic.SWITCHES:
        with ctx.option_scope("spline_route", switch), interp.InterpPlan(a, ic.EXACT, order, ctx=ctx) as plan:
            planes.append(plan.planes()[1])
    for switch, c in zip(ic.SWITCHES[1:], planes[1:]):
        err = np.abs(c - planes[0]).max() / scale(a)
        print(f"order {order}: route {switch} against route 0: error / max |a| = {err:.3e}, identical bits: {np.array_equal(bits(c), bits(planes[0]))}")
        assert err <= BOUND


@pytest.mark.parametrize("switch", ic.SWITCHES)
@pytest.mark.parametrize("dtype", ("float32", "float64"))
def test_values_all_methods(ctx, switch, dtype):
    with ctx.option_scope("spline_route", switch):
        for k, name in enumerate(ic.shapes()):
            kind = ("blobs", "none", "random")[k % 3]
            a = raster(name, dtype, kind)
            transform = (ic.EXACT, ic.INEXACT, ic.SOUTH_UP)[k % 3]
            x, y = ic.world_points(a.shape, transform, 800, seed=k)
            device = (k + switch) % 2 == 1
            for method in METHODS:
                order = io.ORDERS[method]
                want = prepared(name, dtype, kind, order, io.spread_distance(order))
                with interp.InterpPlan(_dev(a) if device else a, transform, order, ctx=ctx) as plan:
                    assert sampled(plan, want, a, x, y, transform, device), (name, method, kind, "device" if device else "host")
                    assert np.isnan(host(plan.at((x[-11:], y[-11:])))).all()   # (outside the hull, non-finite coordinates)


@pytest.mark.parametrize("spread", ("half_order_up", "half_order_down", 0, 1, 2, 3, 5, 7))
def test_dist_nodata_spread_forms(ctx, spread):
    """NaN blobs on tile and band corners and on the raster's edge, every form of the spreading distance (5 and 7: repeated dilations)."""
    name, dtype = "three_by_three", "float32"
    a = raster(name, dtype, "blobs")
    x, y = ic.world_points(a.shape, ic.EXACT, 4000, seed=5)
    # (points around the blobs on the tile corners)
    p = ic.plan()
    rng = np.random.default_rng(9)
    ry = np.concatenate([c + rng.uniform(-9, 9, 400) for c in (p["band_rows"], 2 * p["band_rows"], p["tile_rows"])])
    rx = np.concatenate([c + rng.uniform(-9, 9, 400) for c in (p["tile_cols"], 2 * p["tile_cols"], p["tile_cols"])])
    x, y = np.concatenate([x, ic.EXACT[2] + (rx + 0.5) * ic.EXACT[0]]), np.concatenate([y, ic.EXACT[5] + (ry + 0.5) * ic.EXACT[4]])
    for method in METHODS:
        order = io.ORDERS[method]
        want = prepared(name, dtype, "blobs", order, io.spread_distance(order, spread))
        with interp.InterpPlan(a, ic.EXACT, order, spread, ctx=ctx) as plan:
            assert plan.dist == want.dist and sampled(plan, want, a, x, y, ic.EXACT), (method, spread)
            assert 0 < plan.n_valid < x.size


def test_fast_paths(ctx):
    for dtype in ("float32", "float64"):
        a = raster("tile_rows+1", dtype, "none")
        x, y = ic.world_points(a.shape, ic.EXACT, 500)
        with interp.InterpPlan(a, ic.EXACT, 3, ctx=ctx) as plan:
            assert plan.n_nonfinite == 0 and plan.planes()[0] is None
        nothing = raster("tile_rows+1", dtype, "all")
        for method in METHODS:
            with interp.InterpPlan(_dev(nothing), ic.EXACT, io.ORDERS[method], ctx=ctx) as plan:
                assert plan.n_nonfinite == nothing.size and plan.planes() == (None, None)
                got = plan.at((x, y))
                assert got.dtype == nothing.dtype and np.isnan(got).all() and plan.n_valid == 0
        assert interp.interp_points(a, ic.EXACT, (x[:0], y[:0]), ctx=ctx).shape == (0,)


def test_area_or_point_shift(ctx):
    a = raster("tile_cols+1", "float64", "none")
    r, cc = ic.pixel_points(a.shape, 300)
    t = ic.EXACT
    x, y = t[2] + cc * t[0], t[5] + r * t[4]   # (no half pixel: the "Point" lattice)
    for method in METHODS:
        want = prepared("tile_cols+1", "float64", "none", io.ORDERS[method], 0).at(x, y, t, True)
        got = interp.interp_points(a, t, (x, y), method=method, area_or_point="Point", shift_area_or_point=True, ctx=ctx)
        assert close(got, want, a, io.ORDERS[method]) and not np.isnan(got).any()
        unshifted = interp.interp_points(a, t, (x, y), method=method, area_or_point="Area", shift_area_or_point=True, ctx=ctx)
        assert close(unshifted, prepared("tile_cols+1", "float64", "none", io.ORDERS[method], 0).at(x, y, t, False), a, io.ORDERS[method])


@pytest.mark.parametrize("method", METHODS)
def test_plan_reuse(ctx, method):
    a = raster("three_by_three", "float32", "random")
    x, y = ic.world_points(a.shape, ic.INEXACT, 2000, seed=2)
    x2, y2 = ic.world_points(a.shape, ic.INEXACT, 2000, seed=3)
    d = _dev(a)
    with interp.InterpPlan(d, ic.INEXACT, io.ORDERS[method], ctx=ctx) as plan:
        first, other, again = host(plan.at((x, y))), host(plan.at((_dev(x2), _dev(y2)))), host(plan.at((x, y)))
    assert np.array_equal(bits(first), bits(again))
    assert np.array_equal(bits(first), bits(interp.interp_points(a, ic.INEXACT, (x, y), method=method, ctx=ctx)))
    assert np.array_equal(bits(other), bits(interp.interp_points(a, ic.INEXACT, (x2, y2), method=method, ctx=ctx)))
    assert ctx.synchronize() is None


@pytest.mark.parametrize("dtype", ("float32", "float64"))
def test_to_pointcloud(ctx, dtype):
    """skip_nodata both ways, rows that alternate between empty and full, W no multiple of 64: bit for bit the oracle, order included."""
    for shape, transform in (((37, 131), ic.INEXACT), ((6, 64), ic.EXACT), ((3, 200), ic.SOUTH_UP)):
        a = ic.with_voids(ic.surface(shape, np.dtype(dtype)), "random")
        a[::2] = np.nan
        a[1, :70] = 7.0
        for skip in (True, False):
            want = io.raster_points(a, transform, skip)
            for src in (a, _dev(a)):
                got = interp.raster_points(src, transform, skip, ctx=ctx)
                assert all(hasattr(g, "is_cuda") == hasattr(src, "is_cuda") for g in got)
                for g, w in zip(got, want):
                    g = host(g)
                    assert g.dtype == w.dtype and np.array_equal(bits(g), bits(w)), (shape, skip)
        dem = DEM(a, transform)
        cloud = dem.to_pointcloud()
        assert isinstance(cloud, EPC) and cloud.data_column == "b1" and len(cloud) == int(np.isfinite(a).sum())
        assert np.array_equal(cloud["b1"].values, io.raster_points(a, transform)[2])
        arr = dem.to_pointcloud(as_array=True, skip_nodata=False)
        assert arr.shape == (a.size, 3) and np.array_equal(arr[:, 2], a.ravel().astype(np.float64), equal_nan=True)
    empty = DEM(np.full((4, 5), np.nan, np.dtype(dtype)), ic.EXACT).to_pointcloud()
    assert len(empty) == 0


@pytest.mark.parametrize("method", METHODS)
def test_round_trip(ctx, method):
    """interp_points(to_pointcloud()) returns z: exactly for orders 0 and 1, within the bound for 3 and 5."""
    for dtype, transform in (("float32", ic.EXACT), ("float64", ic.SOUTH_UP)):   # (transforms whose pixel centres are exact in float64)
        a = raster("tile_cols+1", dtype, "none")
        dem = DEM(a, transform)
        cloud = dem.to_pointcloud()
        got = dem.interp_points(cloud, method=method)
        z = cloud.z
        assert got.dtype == z.dtype and got.shape == z.shape and z.size == a.size
        if io.ORDERS[method] <= 1:
            assert np.array_equal(bits(got), bits(z))
        else:
            assert np.all(np.abs(got.astype(np.float64) - z.astype(np.float64)) <= BOUND * scale(a))


def test_dem_interp_points_with_an_epc(ctx):
    a = raster("tile_rows+1", "float64", "single")
    dem = DEM(a, ic.EXACT)
    x, y = ic.world_points(a.shape, ic.EXACT, 500, seed=4)
    cloud = EPC(x, y, np.zeros_like(x))
    for method in METHODS:
        order = io.ORDERS[method]
        want = prepared("tile_rows+1", "float64", "single", order, io.spread_distance(order)).at(x, y, ic.EXACT)
        assert close(dem.interp_points(cloud, method=method), want, a, order)
        assert close(dem.interp_points((x, y), method=method), want, a, order)
        got = dem.interp_points(EPC(_dev(x), _dev(y), _dev(x)), method=method)
        assert got.is_cuda and close(host(got), want, a, order)
    masked = DEM(np.ma.masked_invalid(a.astype(np.float32)), ic.EXACT)
    assert close(masked.interp_points((x, y)), io.interp_points(a.astype(np.float32), ic.EXACT, (x, y)), a, 1)
    ints = DEM(np.arange(48, dtype=np.int16).reshape(6, 8), ic.EXACT)
    got = ints.interp_points((np.array([103.0, 104.0]), np.array([4997.0, 4996.0])), method="linear")
    assert got.dtype == np.float32 and np.array_equal(got, io.interp_points(ints.data, ic.EXACT, (np.array([103.0, 104.0]), np.array([4997.0, 4996.0]))))
