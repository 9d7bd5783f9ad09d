"""CPU-side tests of the proximity feature: the NumPy oracle of the distance-transform rule (tests/proximity_oracle.py) against its own
brute-force form and against ``scipy.ndimage.distance_transform_edt``, and the host logic of ``xdem_amd.proximity``, ``DEM.proximity``,
``Vector.proximity`` and ``Vector.create_mask(buffer=)`` with the oracle engine in the device engine's place."""
import numpy as np
import pytest
from scipy import ndimage

import proximity_cases as pc
import proximity_oracle as po
import vector_oracle as vo
from xdem_amd import DEM, Vector, proximity


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


@pytest.fixture(scope="module")
def case_list():
    return [(f"{name}/{s}", t) for s in (0, 2) for name, t in pc.cases(s)]


# ---- the oracle ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sampling", pc.EXACT + pc.INEXACT + (pc.ANISOTROPIC,))
def test_separable_oracle_equals_brute_force(sampling):
    for seed, shape in enumerate([(1, 1), (1, 17), (13, 1), (7, 9), (23, 31), (40, 60)]):
        t = pc.tiny(seed, shape)
        if shape == (7, 9):
            t[:] = 0   # (no target)
        a, b = po.brute(t, sampling), po.separable(t, sampling)
        assert np.array_equal(bits(a[0]), bits(b[0])), (shape, sampling)
        assert np.array_equal(a[1], b[1]) and a[2] == b[2] == int(t.sum()), (shape, sampling)
    ties = dict(pc.cases(2))["ties"]
    a, b = po.brute(ties, sampling), po.separable(ties, sampling)
    assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(a[1], b[1])


def test_tie_rule_of_the_indices():
    t = pc.with_targets(5, 9, [(2, 2), (2, 6), (0, 4), (4, 4)])
    _, idx, _ = po.separable(t, (1.0, 1.0))
    assert tuple(idx[:, 2, 4]) == (0, 4)      # four targets at distance 2: the smaller |x - tx| is the pixel's own column, its upper row
    t[0, 4] = 0
    assert tuple(po.separable(t, (1.0, 1.0))[1][:, 2, 4]) == (4, 4)   # (still the own column)
    t[4, 4] = 0
    assert tuple(po.separable(t, (1.0, 1.0))[1][:, 2, 4]) == (2, 2)   # left and right at the same distance: the smaller tx
    t = pc.with_targets(1, 9, [(0, 2), (0, 6)])
    assert tuple(po.separable(t, (1.0, 1.0))[1][:, 0, 4]) == (0, 2)   # left and right at the same distance: the smaller tx


@pytest.mark.parametrize("sampling", pc.EXACT)
def test_oracle_equals_scipy_on_exact_samplings(case_list, sampling):
    for name, t in case_list:
        if not t.any():
            continue   # (SciPy returns garbage without a target: the +inf there is this project's own rule)
        want = ndimage.distance_transform_edt(t == 0, sampling=sampling)
        got = po.separable(t, sampling)[0]
        assert np.array_equal(bits(got), bits(want)), (name, sampling, int((got != want).sum()))


@pytest.mark.parametrize("sampling", pc.INEXACT)
def test_oracle_never_exceeds_scipy_on_inexact_samplings(case_list, sampling):
    """On inexact samplings SciPy's parabola intersections can leave the float minimum; a SciPy value is still the cost of a real
    target, so the oracle is never the larger.  The count of differing pixels is printed, a recorded figure and not a criterion: 0 of
    100772 pixels for (0.1, 0.3) and for (1/3, 1/7) on this case list (SciPy 1.15)."""
    differing = total = 0
    for name, t in case_list:
        if not t.any():
            continue
        want = ndimage.distance_transform_edt(t == 0, sampling=sampling)
        got = po.separable(t, sampling)[0]
        assert np.all(got <= want), (name, sampling)   # (a SciPy value is the cost of a real target: never below the minimum)
        differing += int((got != want).sum())
        total += got.size
    print(f"sampling {sampling}: SciPy differs from the float minimum on {differing} of {total} pixels")


@pytest.mark.parametrize("sampling", (pc.EXACT[0], pc.EXACT[3], pc.INEXACT[0]))
def test_indices_point_at_targets_and_reproduce_their_distance(case_list, sampling):
    for name, t in case_list:
        if not t.any():
            dist, idx, n = po.separable(t, sampling)
            assert np.all(np.isinf(dist)) and np.all(idx == -1) and n == 0
            continue
        dist, idx, _ = po.separable(t, sampling)
        assert po.reproduces(t, sampling, dist, idx), name
        sd, si = ndimage.distance_transform_edt(t == 0, sampling=sampling, return_indices=True)
        assert po.reproduces(t, sampling, sd, si), name


def test_small_restatements():
    a = pc.raster_values()
    t = po.target_plane(a)
    assert t.dtype == np.uint8 and not t[np.isnan(a)].any() and not t[3, 4] and t[a == 7].all() and not t[a == 0].any()
    assert np.array_equal(po.target_plane(a, [7.0, -2.5]), ((a == 7) | (a == -2.5)).astype(np.uint8))
    assert not po.target_plane(a, [np.nan]).any()
    m = np.zeros((6, 7), bool)
    m[0:3, 0:3] = True      # touches the raster's edge: the edge makes no boundary
    m[4, 1:6] = True        # one pixel wide: all boundary
    b = po.inner_boundary(m)
    assert b[4, 1:6].all() and not b[0, 0] and not b[1, 1] and b[2, 0] and b[0, 2] and b[2, 2] and b.sum() == 5 + 5
    zeros = po.edt_zeros(np.array([[0.0, 3.0, np.nan]]))[0]
    assert np.array_equal(zeros, [[0.0, 1.0, 2.0]])


# ---- host logic ---------------------------------------------------------------------------------------------------------------------
def test_keyword_validation_and_messages():
    dem = DEM(np.zeros(pc.GRID_SHAPE, np.float32), pc.GRID_TRANSFORM)
    for kw, names in (("geometry_type", proximity.GEOMETRY_TYPES), ("in_or_out", proximity.IN_OR_OUT), ("distance_unit", proximity.DISTANCE_UNITS)):
        with pytest.raises(ValueError) as e:
            dem.proximity(**{kw: "nearby"})
        assert kw in str(e.value) and all(n in str(e.value) for n in names)
    with pytest.raises(NotImplementedError, match="north-up"):
        DEM(np.zeros((4, 5), np.float32), (1.0, 0.1, 0.0, 0.0, -1.0, 0.0)).proximity()
    with pytest.raises(ValueError, match="float32 or float64"):
        dem.proximity(dtype=np.int32)
    for bad in (0.0, -1.0, np.inf, np.nan, (1.0, 0.0), (1.0, 2.0, 3.0)):
        with pytest.raises(ValueError, match="sampling"):
            proximity.sampling_pair(bad)
    with po.oracle_engine():
        with pytest.raises(RuntimeError):
            proximity.distance_transform_edt(np.ones((2, 2)), return_distances=False)
    with pytest.raises(ValueError, match="at most 64"):
        proximity.DeviceEngine().targets(np.zeros((2, 2), np.float32), np.arange(65.0))


def test_sampling_from_transform_and_unit():
    assert proximity.sampling_of(pc.GRID_TRANSFORM, "georeferenced") == (30.0, 20.0)
    assert proximity.sampling_of(pc.GRID_TRANSFORM, "pixel") == (1.0, 1.0)
    assert proximity.sampling_pair(None) == (1.0, 1.0) and proximity.sampling_pair(2) == (2.0, 2.0) and proximity.sampling_pair((2, 3)) == (2.0, 3.0)


def test_proximity_without_a_vector_on_the_oracle_engine():
    a = pc.raster_values()
    dem = DEM(a, pc.GRID_TRANSFORM, crs="EPSG:32645")
    with po.oracle_engine():
        out = dem.proximity(geometry_type="polygon", in_or_out="in")   # (both ignored without a vector)
        assert isinstance(out, DEM) and out.transform == dem.transform and out.crs == dem.crs and out.nodata is None
        want = ndimage.distance_transform_edt(po.target_plane(a) == 0, sampling=(30.0, 20.0)).astype(np.float32)
        assert out.data.dtype == np.float32 and np.array_equal(bits(out.data), bits(want))
        out = dem.proximity(target_values=[7.0, -2.5], distance_unit="pixel", dtype=np.float64)
        want = ndimage.distance_transform_edt(~((a == 7) | (a == -2.5)))
        assert np.array_equal(bits(out.data), bits(want))
        d = proximity.distance_transform_edt(a, sampling=(30, 20))
        assert np.array_equal(bits(d), bits(ndimage.distance_transform_edt(a, sampling=(30, 20))))


def test_compositions_with_a_vector_equal_scipy_on_the_oracle_mask():
    scipy_edt = lambda t, s: ndimage.distance_transform_edt(~t, sampling=s)
    grid = (pc.GRID_SHAPE, pc.GRID_TRANSFORM)
    dem = DEM(np.zeros(pc.GRID_SHAPE, np.float32), pc.GRID_TRANSFORM)
    with vo.patched(), po.oracle_engine():
        v = Vector(pc.POLYGONS)
        mask = v.create_mask(grid)
        assert v.create_mask(grid, buffer=0) is mask
        assert mask.any() and not mask.all()
        for geometry_type in proximity.GEOMETRY_TYPES:
            for in_or_out in proximity.IN_OR_OUT:
                for unit, sampling in (("georeferenced", (30.0, 20.0)), ("pixel", (1.0, 1.0))):
                    got = dem.proximity(v, geometry_type=geometry_type, in_or_out=in_or_out, distance_unit=unit).data
                    want = po.proximity(mask, sampling, geometry_type, in_or_out, np.float32, edt=scipy_edt)
                    assert got.dtype == np.float32 and np.array_equal(bits(got), bits(want)), (geometry_type, in_or_out, unit)
        inside = dem.proximity(v, in_or_out="in").data
        assert np.all(inside[~mask] == 0) and inside[mask].max() > 0
        for r in (45.0, -45.0, 20.0, -20.0):
            got = v.create_mask(grid, buffer=r)
            assert got.dtype == np.bool_ and np.array_equal(got, po.buffered(mask, (30.0, 20.0), r, edt=scipy_edt)), r
            assert v.create_mask(grid, buffer=r) is got
        assert v.create_mask(grid, buffer=45.0).sum() > mask.sum() > v.create_mask(grid, buffer=-45.0).sum() > 0


def test_size_grid_of_vector_proximity():
    with vo.patched(), po.oracle_engine():
        v = Vector(pc.POLYGONS, crs="EPSG:32645")
        shape, t6 = v.size_grid((40, 25))
        b = v.bounds
        assert shape == (25, 40) and t6 == ((b.right - b.left) / 40, 0.0, b.left, 0.0, -(b.top - b.bottom) / 25, b.top)
        out = v.proximity(size=(40, 25), geometry_type="polygon")
        assert isinstance(out, DEM) and out.shape == (25, 40) and out.transform == t6 and out.crs == "EPSG:32645"
        want = po.proximity(v.create_mask((shape, t6)), proximity.sampling_of(t6), "polygon", "both")
        assert np.array_equal(bits(out.data), bits(want))
        with pytest.raises(ValueError, match="size"):
            v.proximity(size=(0, 5))
        on_dem = v.proximity(DEM(np.zeros(pc.GRID_SHAPE, np.float32), pc.GRID_TRANSFORM))
        assert on_dem.shape == pc.GRID_SHAPE


def test_edt_plan_constants():
    for switch in pc.SWITCHES:
        p = proximity.edt_plan(1000, 1000, switch)
        assert p["band_rows"] > 0 and p["block_cols"] > 0 and 0 <= p["halo"] < p["tile_cols"] and 256 % p["tile_cols"] == 0
        assert p["block_cols"] & (p["block_cols"] - 1) == 0 and 64 % p["block_cols"] == 0
        assert proximity.edt_plan(32767, 3, switch)["offset_bytes"] == 2 and proximity.edt_plan(32768, 3, switch)["offset_bytes"] == 4
    assert proximity.edt_plan(1, 1, 1)["halo"] == 0 and proximity.edt_plan(1, 1, 0)["halo"] > 0
    small, auto = proximity.edt_plan(1, 1, 2), proximity.edt_plan(1, 1, 0)
    assert all(small[k] < auto[k] for k in ("band_rows", "tile_cols", "halo", "block_cols"))
    for bad in ((0, 5, 0), (5, 0, 0), (5, 5, 3), (5, 5, -1)):
        with pytest.raises(ValueError):
            proximity.edt_plan(*bad)
