"""The NumPy restatement of the interp_points rule (tests/interp_oracle.py) pinned to SciPy on the CPU: coefficients against
``spline_filter``, values against ``map_coordinates`` (default mode and mirror), the spread rule against ``binary_dilation`` +
``map_coordinates(order=1) > 0``, the fill against ``distance_transform_edt`` where the nearest finite pixel is unique.  Then what the
library answers without a GPU: the plan constants, one line of the prefilter through the functions the kernels run, and the argument
errors of the Python layer."""
import numpy as np
import pytest
import scipy.ndimage as ndi

import interp_cases as ic
import interp_oracle as io
import proximity_oracle as po
from xdem_amd import DEM, _args, _lib, interp

BOUND = 1e-12   # x max |finite raster value|: DESIGN.md section 7 (f3), float64 kernels against SciPy


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


@pytest.mark.parametrize("order", (3, 5))
@pytest.mark.parametrize("dtype", (np.float32, np.float64))
@pytest.mark.parametrize("shape", ((2, 2), (2, 97), (97, 2), (5, 7), (131, 200)))
def test_coefficients_against_spline_filter(shape, dtype, order):
    a = ic.surface(shape, dtype)
    want = ndi.spline_filter(a, order, output=np.float64, mode="mirror")
    got = io.coefficients(a, order)
    err = np.abs(got - want).max()
    print(shape, np.dtype(dtype).name, order, "max error / max |a| =", err / np.abs(a).max())
    assert err <= BOUND * np.abs(a).max()


@pytest.mark.parametrize("order", (0, 1, 3, 5))
@pytest.mark.parametrize("dtype", (np.float32, np.float64))
def test_values_against_map_coordinates(dtype, order):
    for shape in ((131, 200), (5, 7), (2, 2)):
        a = ic.surface(shape, dtype)
        r, cc = ic.pixel_points(shape, 3000)
        got = io.Prepared(a, order, 0).values64(r, cc)
        for kw in ({}, {"mode": "mirror"}):
            want = ndi.map_coordinates(a, [r, cc], order=order, output=np.float64, **kw)
            if order <= 1:
                assert np.array_equal(bits(got), bits(want)), (shape, kw)
            else:
                err = np.abs(got - want).max()
                print(shape, np.dtype(dtype).name, order, kw, "max error / max |a| =", err / np.abs(a).max())
                assert err <= BOUND * np.abs(a).max(), (shape, kw)
        # the one rounding to the raster's dtype is SciPy's too
        if order <= 1:
            assert np.array_equal(bits(io.Prepared(a, order, 0).values64(r, cc).astype(dtype)), bits(ndi.map_coordinates(a, [r, cc], order=order)))


@pytest.mark.parametrize("order", (0, 1, 3, 5))
def test_nodes_return_the_raster(order):
    a = ic.surface((37, 53), np.float64)
    rr, cq = np.mgrid[0:37, 0:53]
    got = io.Prepared(a, order, 0).values64(rr.ravel().astype(np.float64), cq.ravel().astype(np.float64)).reshape(a.shape)
    assert np.abs(got - a).max() <= BOUND * np.abs(a).max()
    if order <= 1:
        assert np.array_equal(got, a)


@pytest.mark.parametrize("kind", ("single", "frame", "random", "none", "all"))
def test_spread_rule_against_scipy(kind):
    shape = (23, 31)
    a = ic.with_voids(ic.surface(shape, np.float64), kind)
    mask = ~np.isfinite(a)
    r, cc = ic.pixel_points(shape, 2000)
    for d in range(4):
        spread = ndi.binary_dilation(mask, iterations=d) if d else mask
        assert np.array_equal(io.dilate(mask, d), spread), d
        want = ndi.map_coordinates(spread.astype(np.float64), [r, cc], order=1) > 0
        assert np.array_equal(io.spread_hit(spread, r, cc), want), d
    # the spreading distances by name
    assert [io.spread_distance(o) for o in (0, 1, 3, 5)] == [0, 1, 2, 3]
    assert [io.spread_distance(o, "half_order_down") for o in (0, 1, 3, 5)] == [0, 0, 1, 2]
    assert [interp.spread_distance(o) for o in (0, 1, 3, 5)] == [0, 1, 2, 3] and interp.spread_distance(3, 7) == 7
    # and through the whole call: the NaN set of every order is outside | spread
    for order in (0, 1, 3, 5):
        p = io.Prepared(a, order, io.spread_distance(order))
        got = np.isnan(p.values64(r, cc))
        if kind == "all":
            assert got.all()
        else:
            sp = ndi.binary_dilation(mask, iterations=p.dist) if p.dist else mask
            assert np.array_equal(got, ndi.map_coordinates(sp.astype(np.float64), [r, cc], order=1) > 0)


@pytest.mark.parametrize("kind", ("single", "frame", "random", "blobs"))
def test_fill_rule(kind):
    shape = (40, 47)
    a = ic.with_voids(ic.surface(shape, np.float32), kind)
    a[~np.isfinite(a)] = np.nan
    fin = np.isfinite(a)
    got = io.fill(a)
    # the project's EDT, tie-break included
    _, idx, _ = po.separable(fin.astype(np.uint8), None)
    assert np.array_equal(got, a[idx[0], idx[1]])
    # SciPy's, where the nearest finite pixel is unique
    dist, sidx = ndi.distance_transform_edt(~fin, return_indices=True)
    yy, xx = np.nonzero(fin)
    unique = np.zeros(shape, bool)
    for y, x in zip(*np.nonzero(~fin)):
        d2 = (yy - y) ** 2 + (xx - x) ** 2
        unique[y, x] = (d2 == d2.min()).sum() == 1
    assert unique.any() or kind == "single"   # (a lone void has four nearest pixels)
    assert np.array_equal(got[unique], a[sidx[0], sidx[1]][unique])
    assert np.array_equal(got[fin], a[fin])


def test_plan_constants():
    L = _lib.lib()
    for switch in ic.SWITCHES:
        for name, (H, W) in ic.shapes().items():
            for order in (0, 1, 3, 5):
                p = interp.plan_constants(H, W, order, switch)
                assert p["halo"] == 64
                assert 0 <= p["lds_bytes"] <= 160 * 1024
                assert p["band_rows"] >= 1 and p["tile_rows"] >= 1 and p["tile_cols"] >= 1
                tiles = -(-H // p["tile_rows"]) * -(-W // p["tile_cols"])
                assert tiles * p["tile_rows"] * p["tile_cols"] >= H * W and -(-H // p["band_rows"]) * p["band_rows"] >= H
                if p["lds_bytes"]:
                    assert p["lds_bytes"] == p["tile_rows"] * (p["tile_cols"] + 2 * p["halo"] + 1) * 8
                else:
                    assert (p["tile_rows"], p["tile_cols"]) == (1, W)
                if switch == 1:
                    assert p["band_rows"] == H
                assert (p["lds_bytes"] > 0) == (switch == 3 or (switch != 2 and W > 2 * p["halo"]))
    none = [None] * 5
    for args in ((1, 9, 3, 0), (9, 1, 3, 0), (9, 9, 2, 0), (9, 9, 3, 4), (9, 9, 3, -1), (1 << 31, 9, 3, 0)):
        assert L.xdemhip_spline_plan(*args, *none) == -1, args
        with pytest.raises(ValueError):
            interp.plan_constants(*args)
    assert L.xdemhip_spline_plan(9, 9, 3, 0, *none) == 0


@pytest.mark.parametrize("order", (3, 5))
def test_banded_line_on_the_cpu(order):
    """The functions the kernels run, on one line cut into bands: within the bound of the whole-line recursion for every length
    around the halo and every band length, stored at once or in the two walks of the LDS route."""
    L = _lib.lib()
    rng = np.random.default_rng(order)
    worst = 0.0
    for n in (2, 3, 5, 31, 33, 63, 64, 65, 66, 97, 127, 128, 129, 130, 257, 769):
        a = 1000.0 + 100.0 * rng.normal(size=n)
        want = io.filter_axis0(a[:, None], order)[:, 0]
        for band in (1, 7, 32, 64, 100, 256, n):
            for two_phase in (0, 1):
                out = np.empty(n)
                assert L.xdemhip_spline_host_line(_args.dp(a), n, order, band, two_phase, _args.dp(out)) == 0
                worst = max(worst, np.abs(out - want).max() / np.abs(a).max())
    print("order", order, "worst error / max |a| =", worst)
    assert worst <= BOUND
    assert L.xdemhip_spline_host_line(_args.dp(a), 1, order, 4, 0, _args.dp(out)) == -1
    assert L.xdemhip_spline_host_line(_args.dp(a), 5, 2, 4, 0, _args.dp(out)) == -1


def test_argument_errors():
    a = ic.surface((6, 8), np.float32)
    pts = (np.array([101.0]), np.array([4999.0]))
    for method in ("slinear", "pchip", "splinef2d", "bicubic", None):
        with pytest.raises(NotImplementedError, match=repr(method) if method else "None"):
            interp.interp_points(a, ic.EXACT, pts, method=method)
    with pytest.raises(ValueError, match="north-up"):
        interp.interp_points(a, (2.0, 0.1, 100.0, 0.0, -2.0, 5000.0), pts)
    with pytest.raises(ValueError, match="north-up"):
        interp.raster_points(a, (2.0, 0.0, 100.0, 0.3, -2.0, 5000.0))
    for shape in ((1, 8), (8, 1)):
        with pytest.raises(ValueError, match="length 1"):
            interp.interp_points(np.ones(shape, np.float32), ic.EXACT, pts)
    with pytest.raises(ValueError, match="force_scipy_function"):
        interp.interp_points(a, ic.EXACT, pts, force_scipy_function="interpn")
    for bad in ("half", -1, 1.5):
        with pytest.raises(ValueError, match="dist_nodata_spread"):
            interp.interp_points(a, ic.EXACT, pts, dist_nodata_spread=bad)
    dem = DEM(a, ic.EXACT)
    with pytest.raises(ValueError, match="band"):
        dem.interp_points(pts, band=2)
    with pytest.raises(NotImplementedError, match="input_latlon"):
        dem.interp_points(pts, input_latlon=True)
    with pytest.raises(NotImplementedError, match="subsample"):
        dem.to_pointcloud(subsample=100)
    with pytest.raises(NotImplementedError, match="auxiliary_data_bands"):
        dem.to_pointcloud(auxiliary_data_bands=[2])
    with pytest.raises(NotImplementedError, match="force_pixel_offset"):
        dem.to_pointcloud(force_pixel_offset="ul")


def test_raster_points_oracle():
    """Row-major order and pixel-centre coordinates against np.nonzero."""
    for transform in (ic.EXACT, ic.INEXACT):
        a = ic.with_voids(ic.surface((9, 13), np.float32), "random")
        a[3] = np.nan
        x, y, z = io.raster_points(a, transform, True)
        rows, cols = np.nonzero(np.isfinite(a))
        assert np.array_equal(z, a[rows, cols]) and z.dtype == a.dtype
        assert np.array_equal(x, transform[2] + (cols + 0.5) * transform[0]) and np.array_equal(y, transform[5] + (rows + 0.5) * transform[4])
        r, cc = io.pixel_coordinates(x, y, transform)
        assert np.allclose(r, rows, atol=1e-9) and np.allclose(cc, cols, atol=1e-9)
        x, y, z = io.raster_points(a, transform, False)
        assert z.size == a.size and np.array_equal(z, a.ravel(), equal_nan=True)
        assert np.array_equal(x.reshape(a.shape)[0], transform[2] + (np.arange(13) + 0.5) * transform[0])
