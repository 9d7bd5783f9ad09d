"""Regridding without a GPU: the NumPy oracle (tests/reproject_oracle.py) against the properties its rule must have, so that the
yardstick is checked before anything is measured with it; ``xdem_amd.reproject.target_grid``; and the parts of ``DEM.reproject``,
``reproject_mask`` and ``DEMCollection.on_reference_grid`` that decide or refuse before any device pass."""
import types
import warnings

import numpy as np
import pytest

import reproject_cases as rc
import reproject_oracle as ro
from xdem_amd import DEM, DEMCollection, reproject

T0 = (10.0, 0.0, 500.0, 0.0, -10.0, 9000.0)


@pytest.fixture(scope="module")
def src():
    return rc.terrain((37, 53))


# ---- the oracle against its own rule ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", ["bilinear", "cubic", "nearest"])
def test_oracle_identity_and_whole_pixel_shift_are_bit_exact(src, kernel):
    out, count = ro.regrid(src, src.shape, (1.0, 0.0, 1.0, 0.0), kernel)
    assert out.dtype == src.dtype and np.array_equal(out, src) and count == src.size
    out, count = ro.regrid(src, src.shape, (1.0, 3.0, 1.0, -2.0), kernel)
    expect = np.full_like(src, np.nan)
    expect[2:, :-3] = src[:-2, 3:]
    assert np.array_equal(out, expect, equal_nan=True) and count == np.count_nonzero(~np.isnan(expect))


@pytest.mark.parametrize("kernel", ["bilinear", "cubic", "cubic_spline"])
def test_oracle_returns_the_integer_plane_under_upsampling(kernel):
    """x2 upsampling with quarter-pixel offsets.  bilinear and cubic: exact in float32 and float64.  cubic_spline: its weights sum to
    1 within an ulp, so the plane comes back within a few ulp of its largest value (1e-16 where the plane crosses zero)."""
    shape, m = (60, 90), (0.5, 2.25, 0.5, 3.25)
    expect = rc.plane_at(ro.centres(shape[1], m[0], m[1]), ro.centres(shape[0], m[2], m[3]))
    inner = (slice(8, -8), slice(8, -8))
    for dtype in (np.float32, np.float64):
        out, _ = ro.regrid(rc.plane((37, 53), dtype), shape, m, kernel)
        assert out.dtype == dtype
        if kernel == "cubic_spline":
            assert np.max(np.abs(out[inner] - expect[inner].astype(dtype))) <= 4 * np.finfo(dtype).eps * 256
        else:
            assert np.array_equal(out[inner], expect[inner].astype(dtype))


def test_oracle_returns_the_integer_plane_under_bilinear_downsampling():
    shape, m = (15, 22), (2.0, 2.0, 2.0, 3.0)
    out, _ = ro.regrid(rc.plane((37, 53)), shape, m, "bilinear")
    expect = rc.plane_at(ro.centres(shape[1], m[0], m[1]), ro.centres(shape[0], m[2], m[3])).astype(np.float32)
    assert np.array_equal(out[2:-2, 2:-2], expect[2:-2, 2:-2])
    assert ro.tap_count("bilinear", 2.0) == 5 and ro.tap_count("bilinear", 3.7) == 8 and ro.tap_count("cubic", 3.7) == 15
    assert ro.tap_count("bilinear", 0.4) == 3 and ro.tap_count("cubic", 1.0) == 5


@pytest.mark.parametrize("kernel", rc.KERNELS)
def test_oracle_outside_and_holes(src, kernel):
    out, count = ro.regrid(src, (9, 11), (1.0, 200.0, 1.0, 3.0), kernel)
    assert np.all(np.isnan(out)) and count == 0
    holed = src.copy()
    holed[10:25, 20:40] = np.nan
    out, _ = ro.regrid(holed, src.shape, (1.0, 0.5, 1.0, 0.25), kernel)
    assert np.all(np.isnan(out[13:22, 23:36])) and np.all(np.isfinite(out[2:8, 2:18]))
    holed[5, 5] = np.inf
    out2, _ = ro.regrid(holed, src.shape, (1.0, 0.5, 1.0, 0.25), kernel)
    nan5 = src.copy()
    nan5[10:25, 20:40] = np.nan
    nan5[5, 5] = np.nan
    if kernel == "nearest":   # (copies the source's bits, an infinite one too)
        assert np.count_nonzero(np.isinf(out2)) == 1
        return
    assert np.array_equal(out2, ro.regrid(nan5, src.shape, (1.0, 0.5, 1.0, 0.25), kernel)[0], equal_nan=True)   # (Inf is skipped like NaN)


def test_oracle_nearest_epsilon_and_uint8():
    a = np.arange(12, dtype=np.float32).reshape(3, 4)
    below, _ = ro.regrid(a, a.shape, (1.0, -0.5 - 1e-12, 1.0, -0.5 - 1e-12), "nearest")   # u = o - 1e-12: still pixel o
    assert np.array_equal(below, a)
    mask = (a % 2 == 0).view(np.uint8)
    out, count = ro.regrid(mask, (3, 6), (1.0, -1.0, 1.0, 0.0), "nearest")
    assert out.dtype == np.uint8 and np.array_equal(out[:, 1:5], mask) and not out[:, 0].any() and not out[:, 5].any() and count == 12


def test_checkerboard_case_straddles_the_threshold():
    out, _, den = ro.regrid(rc.voids("checkerboard"), rc.BIG, rc.CHECKERBOARD_MAP, "cubic", return_den=True)
    assert np.count_nonzero((den > 0) & (den <= ro.MIN_DEN)) >= 1 and np.count_nonzero((den > ro.MIN_DEN) & (den < 4 * ro.MIN_DEN)) >= 1
    assert np.all(np.isnan(out[(den > 0) & (den <= ro.MIN_DEN)])) and np.all(np.isfinite(out[(den > ro.MIN_DEN) & (den < 4 * ro.MIN_DEN)]))


# ---- target_grid --------------------------------------------------------------------------------------------------------------------
def test_target_grid_forms():
    shape = (40, 60)
    ref = types.SimpleNamespace(shape=(7, 9), transform=(20.0, 0.0, 510.0, 0.0, -20.0, 8990.0))
    assert reproject.target_grid(shape, T0, ref=ref) == ((7, 9), ref.transform)
    assert reproject.target_grid(shape, T0, ref=((7, 9), ref.transform)) == ((7, 9), ref.transform)
    assert reproject.target_grid(shape, T0, ref=DEM(np.zeros((7, 9), np.float32), ref.transform)) == ((7, 9), ref.transform)
    cases = [dict(res=25.0), dict(res=(4.0, 7.0)), dict(grid_size=(13, 11)), dict(bounds=(505.0, 8700.0, 1000.0, 8995.0)),
             dict(bounds=(505.0, 8700.0, 1000.0, 8995.0), res=30.0), dict(bounds=(505.0, 8700.0, 1000.0, 8995.0), grid_size=(5, 3)),
             dict(res=1e6)]
    for kw in cases:
        assert reproject.target_grid(shape, T0, **kw) == ro.target_grid(shape, T0, **kw), kw
    assert reproject.target_grid(shape, T0, res=25.0) == ((16, 24), (25.0, 0.0, 500.0, 0.0, -25.0, 9000.0))
    assert reproject.target_grid(shape, T0, res=1e6)[0] == (1, 1)
    box = types.SimpleNamespace(left=505.0, bottom=8700.0, right=1000.0, top=8995.0)
    assert reproject.target_grid(shape, T0, bounds=box) == ((30, 50), (10.0, 0.0, 505.0, 0.0, -10.0, 8995.0))
    assert reproject.target_grid(shape, T0, grid_size=(13, 11)) == ((11, 13), (600.0 / 13, 0.0, 500.0, 0.0, -400.0 / 11, 9000.0))


def test_target_grid_errors():
    with pytest.raises(ValueError, match="res and grid_size"):
        reproject.target_grid((4, 5), T0, res=2.0, grid_size=(3, 3))
    with pytest.raises(ValueError, match="one of ref, res, grid_size and bounds"):
        reproject.target_grid((4, 5), T0)
    with pytest.raises(ValueError):
        reproject.target_grid((4, 5), T0, ref=((4, 5), T0), res=2.0)
    with pytest.raises(NotImplementedError, match="north-up"):
        reproject.target_grid((4, 5), (10.0, 0.1, 0.0, 0.0, -10.0, 0.0), res=2.0)
    with pytest.raises(NotImplementedError, match="north-up"):
        reproject.target_grid((4, 5), T0, ref=((4, 5), (10.0, 0.0, 0.0, 0.2, -10.0, 0.0)))


# ---- the route policy (a host function of the library) ------------------------------------------------------------------------------
def test_route_policy():
    """Tiled while a workgroup's footprint and tables fit the LDS budget, per-pixel beyond; the switch values 1 and 2; nearest has one."""
    t = (1.0, 0.0, 0.0, 0.0, -1.0, 0.0)
    grid = lambda r: (r, 0.0, 0.0, 0.0, -r, 0.0)
    for kernel in ("bilinear", "cubic", "cubic_spline"):
        for dtype in (np.float32, np.float64):
            previous = 0
            for r in (0.1, 0.4, 1.0, 1.7, 2.0, 2.2, 3.0, 5.0, 40.0):
                name, nbytes, budget = reproject.route(t, grid(r), kernel, dtype)
                assert budget == 63 * 1024 and nbytes >= previous and name == ("tile" if nbytes <= budget else "direct"), (kernel, r)
                assert reproject.route(t, grid(r), kernel, dtype, switch=1)[0] == name
                assert reproject.route(t, grid(r), kernel, dtype, switch=2)[0] == "direct"
                previous = nbytes
            assert reproject.route(t, grid(1.0), kernel, dtype)[0] == "tile" and reproject.route(t, grid(40.0), kernel, dtype)[0] == "direct"
    assert reproject.route(t, grid(7.0), "nearest", np.uint8)[0] == "nearest"
    # at scale 1 from float32: room for 68 x 20 (bilinear, K = 3) and 70 x 22 (cubic, K = 5) source pixels, and the tables
    assert reproject.route(t, grid(1.0), "bilinear")[1] == 4 * 68 * 20 + 64 * (3 * 8 + 8) + 16 * (3 * 8 + 8)
    assert reproject.route(t, grid(1.0), "cubic")[1] == 4 * 70 * 22 + 64 * (5 * 8 + 8) + 16 * (5 * 8 + 8)


# ---- DEM.reproject, before the device -----------------------------------------------------------------------------------------------
def test_reproject_onto_the_same_grid_returns_self(src):
    dem = DEM(src, T0, crs="EPSG:32633", nodata=-9999)
    with pytest.warns(UserWarning, match="Output projection, bounds and grid size are identical -> returning self"):
        assert dem.reproject(dem) is dem
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert dem.reproject(DEM(src * 0, T0), silent=True) is dem
        assert dem.reproject(res=10.0, silent=True) is dem
        assert dem.reproject(crs="EPSG:32633", grid_size=(53, 37), silent=True) is dem


def test_reproject_refusals(src):
    dem = DEM(src, T0, crs="EPSG:32633")
    other = ((20, 20), (10.0, 0.0, 505.0, 0.0, -10.0, 8995.0))
    with pytest.raises(NotImplementedError, match="CRS"):
        dem.reproject(other, crs="EPSG:4326")
    with pytest.raises(NotImplementedError, match="north-up"):
        dem.reproject(((20, 20), (10.0, 1.0, 505.0, 0.0, -10.0, 8995.0)))
    with pytest.raises(NotImplementedError, match="north-up"):
        DEM(src, (10.0, 0.0, 500.0, 0.5, -10.0, 9000.0)).reproject(other)
    for name in ("average", "lanczos", "mode", types.SimpleNamespace(name="max")):
        with pytest.raises(NotImplementedError, match="resampling"):
            dem.reproject(other, resampling=name)
    with pytest.raises(NotImplementedError, match="resampling"):
        reproject.regrid(src, T0, *other, resampling="gauss")
    with pytest.raises(ValueError):
        dem.reproject()


def test_resampling_names_and_enum_like_objects():
    for name, code in (("nearest", 0), ("bilinear", 1), ("cubic", 2), ("cubic_spline", 3)):
        assert reproject.resampling_code(name) == code
        assert reproject.resampling_code(types.SimpleNamespace(name=name, value=code)) == code
    assert reproject.grid_map(T0, (20.0, 0.0, 510.0, 0.0, -20.0, 8990.0)) == ro.grid_map(T0, (20.0, 0.0, 510.0, 0.0, -20.0, 8990.0)) == (2.0, 1.0, 2.0, 1.0)


def test_refusals_on_differing_grids_point_to_reproject(src):
    ref, tba = DEM(src, T0), DEM(src, (10.0, 0.0, 505.0, 0.0, -10.0, 9000.0))
    with pytest.raises(NotImplementedError, match=r"share one grid \(reprojection is geoutils' job\).*DEM\.reproject"):
        tba.coregister_3d(ref)
    with pytest.raises(NotImplementedError, match=r"share one grid \(reprojection is geoutils' job\).*DEM\.reproject"):
        tba.estimate_uncertainty(ref)
    col = DEMCollection([ref, tba], timestamps=[np.datetime64("2000-01-01"), np.datetime64("2010-01-01")])
    with pytest.raises(NotImplementedError, match=r"share one grid \(reprojection is geoutils' job\).*on_reference_grid"):
        col.subtract_dems()


def test_on_reference_grid_keeps_dems_already_on_the_grid(src):
    stamps = [np.datetime64("2000-01-01"), np.datetime64("2010-01-01")]
    a, b = DEM(src, T0), DEM(src + 1, T0)
    col = DEMCollection.on_reference_grid([a, b], timestamps=stamps, reference_dem=b)
    assert col.dems[0] is a and col.dems[1] is b and col.reference_dem is b
