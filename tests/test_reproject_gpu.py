"""xdemhip_regrid on the GPU against the NumPy restatement of its rule (tests/reproject_oracle.py): the destination array bit for bit
(NaN where the oracle has NaN) and ``valid_count`` equal -- from host and device memory, from two runs, and under every value of the
test switch ``"regrid_route"`` (0 automatic, 1 tiled where the footprint fits, 2 per-pixel).  Then ``DEM.reproject``, ``reproject_mask``
and ``DEMCollection.on_reference_grid`` end to end.  The shapes are the smallest at which a stage can go wrong."""
import ctypes

import numpy as np
import pytest

import reproject_cases as rc
import reproject_oracle as ro
from gpu_helpers import _back, _dev
from xdem_amd import DEM, DEMCollection, _args, _lib, coreg, reproject

pytestmark = pytest.mark.gpu

CODES = {np.dtype(np.float32): _lib.F32, np.dtype(np.float64): _lib.F64, np.dtype(np.uint8): _lib.U8}
FLOAT_KERNELS = ("bilinear", "cubic", "cubic_spline")


@pytest.fixture(scope="module")
def ctx():
    return _lib.default_context()


@pytest.fixture(scope="module")
def big():
    return rc.terrain()


def call(ctx, src, shape, map4, kernel, dst_dtype=None, device=False):
    """xdemhip_regrid through the C ABI with the map as it stands: (array, valid_count), or the status of a refusal."""
    import torch

    dst_dtype = np.dtype(src.dtype if dst_dtype is None else dst_dtype)
    count = ctypes.c_int64(-1)
    if device:
        s = _dev(src)
        d = torch.full(tuple(shape), 77, dtype=getattr(torch, dst_dtype.name), device="cuda")
        torch.cuda.synchronize()
    else:
        s, d = np.ascontiguousarray(src), np.full(shape, 77, dtype=dst_dtype)
    rc_ = ctx._L.xdemhip_regrid(ctx.handle, _args.ptr(s), CODES[np.dtype(src.dtype)], src.shape[0], src.shape[1], _args.ptr(d), CODES[dst_dtype],
                                shape[0], shape[1], _args.c_doubles(map4), reproject.RESAMPLINGS[kernel], _args.space(s), ctypes.byref(count))
    if rc_ != _lib.OK:
        return rc_
    return (_back(ctx, d) if device else d), int(count.value)


def same(got, expect) -> bool:
    """Bit for bit where the oracle is a number, NaN where it is NaN."""
    arr, exp = got[0], expect[0]
    if arr.dtype != exp.dtype or arr.shape != exp.shape or got[1] != expect[1]:
        return False
    if arr.dtype == np.uint8:
        return np.array_equal(arr, exp)
    nan = np.isnan(exp)
    view = np.uint32 if arr.dtype == np.float32 else np.uint64
    return np.array_equal(np.isnan(arr), nan) and np.array_equal(arr.view(view)[~nan], exp.view(view)[~nan])


def check(ctx, src, shape, map4, kernel, dst_dtype=None, expect_route=None):
    expect = ro.regrid(src, shape, map4, kernel, dst_dtype)
    if expect_route is not None:
        assert route_of(map4, kernel, src.dtype)[0] == expect_route
    try:
        for switch in (0, 1, 2):
            ctx.set_option("regrid_route", switch)
            assert same(call(ctx, src, shape, map4, kernel, dst_dtype), expect), (kernel, shape, map4, switch, "host")
            if switch != 1:
                assert same(call(ctx, src, shape, map4, kernel, dst_dtype, device=True), expect), (kernel, shape, map4, switch, "device")
            if switch == 0:
                assert same(call(ctx, src, shape, map4, kernel, dst_dtype), expect), (kernel, shape, map4, "second run")
    finally:
        ctx.set_option("regrid_route", 0)
    return expect


def route_of(map4, kernel, dtype, switch=0):
    """(route, LDS bytes of a tile, budget) from the library's own policy function."""
    r, nbytes, budget = ctypes.c_int(), ctypes.c_int64(), ctypes.c_int64()
    assert _lib.lib().xdemhip_regrid_route(_args.c_doubles(map4), reproject.RESAMPLINGS[kernel], CODES[np.dtype(dtype)], switch, ctypes.byref(r),
                                           ctypes.byref(nbytes), ctypes.byref(budget)) == _lib.OK
    return reproject.ROUTES[r.value], int(nbytes.value), int(budget.value)


# ---- the kernel routes --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", rc.KERNELS)
@pytest.mark.parametrize("name,shape,map4", rc.offsets_scale_one() + rc.scales() + rc.placements(), ids=lambda v: v if isinstance(v, str) else None)
def test_grids_on_the_big_source(ctx, big, kernel, name, shape, map4):
    out, count = check(ctx, big, shape, map4, kernel)
    if name == "same" and kernel != "cubic_spline":
        assert np.array_equal(out, big) and count == big.size
    if name.startswith("outside") or name == "far_outside":
        assert count == 0
    if name == "inside_one_pixel":
        assert count == shape[0] * shape[1]


@pytest.mark.parametrize("kernel", rc.KERNELS)
def test_destination_sizes_around_the_tile(ctx, big, kernel):
    for _, shape, map4 in rc.tile_edges():
        check(ctx, big, shape, map4, kernel)


@pytest.mark.parametrize("kernel", rc.KERNELS)
@pytest.mark.parametrize("source", sorted(rc.SMALL_SOURCES))
def test_small_sources(ctx, kernel, source):
    src = rc.terrain(rc.SMALL_SOURCES[source], seed=3)
    H, W = src.shape
    for shape, map4 in [((H, W), (1.0, 0.0, 1.0, 0.0)), ((3 * H, 3 * W), (1 / 3, 0.0, 1 / 3, 0.0)), ((H + 2, W + 2), (1.0, -1.25, 1.0, -0.75)),
                        ((1, 1), (float(W), 0.0, float(H), 0.0)), ((rc.TH + 1, rc.TW + 1), (W / (rc.TW + 1), 0.0, H / (rc.TH + 1), 0.0))]:
        check(ctx, src, shape, map4, kernel)


@pytest.mark.parametrize("kernel", FLOAT_KERNELS)
def test_tap_counts_of_the_downsampling_case(ctx, big, kernel):
    assert ro.tap_count("bilinear", 3.7) == 8 and ro.tap_count("cubic", 3.7) == 15
    check(ctx, big.astype(np.float64), (17, 23), (3.7, -0.5, 3.7, 0.25), kernel)


@pytest.mark.parametrize("kernel,dtype", [("bilinear", np.float32), ("cubic", np.float32), ("cubic_spline", np.float64)])
def test_both_sides_of_the_route_threshold(ctx, big, kernel, dtype):
    """The automatic choice takes the tiled route while a workgroup's footprint and tables fit REGRID_LDS_BUDGET (63 KiB) and the
    per-pixel route beyond: the downsampling factors just below and just above it, each under every switch."""
    factors = [1.0 + 0.02 * k for k in range(1, 700)]
    routes = [route_of((r, 0.1, r, 0.2), kernel, dtype) for r in factors]
    flip = next(k for k in range(1, len(routes)) if routes[k][0] == "direct")
    assert routes[flip - 1][0] == "tile" and routes[flip - 1][1] <= routes[flip][2] < routes[flip][1]
    assert all(r[0] == "tile" for r in routes[:flip]) and all(r[0] == "direct" for r in routes[flip:])
    src = big.astype(dtype)
    for k, expect_route in ((flip - 1, "tile"), (flip, "direct")):
        r = factors[k]
        assert route_of((r, 0.1, r, 0.2), kernel, dtype, switch=1)[0] == expect_route and route_of((r, 0.1, r, 0.2), kernel, dtype, switch=2)[0] == "direct"
        check(ctx, src, (max(1, int(61 / r)) + 1, max(1, int(83 / r)) + 1), (r, 0.1, r, 0.2), kernel, expect_route=expect_route)


@pytest.mark.parametrize("kernel", rc.KERNELS)
@pytest.mark.parametrize("kind", ["single", "border_rows", "hole", "checkerboard", "inf"])
def test_voids_and_non_finite_values(ctx, kernel, kind):
    src = rc.voids(kind)
    for shape, map4 in [(rc.BIG, (1.0, 0.5, 1.0, 0.25)), (rc.BIG, (1.0, 0.0, 1.0, 0.0)), ((150, 205), (0.4, 0.1, 0.4, 0.2)), ((17, 23), (3.7, -0.5, 3.7, 0.25))]:
        out, _ = check(ctx, src, shape, map4, kernel)
        if kind == "hole" and kernel != "nearest":
            assert np.any(np.isnan(out)) and np.any(np.isfinite(out))


def test_checkerboard_on_both_sides_of_the_divisor_threshold(ctx):
    src = rc.voids("checkerboard")
    _, _, den = ro.regrid(src, rc.BIG, rc.CHECKERBOARD_MAP, "cubic", return_den=True)
    assert np.count_nonzero((den > 0) & (den <= ro.MIN_DEN)) >= 1 and np.count_nonzero((den > ro.MIN_DEN) & (den < 4 * ro.MIN_DEN)) >= 1
    assert np.count_nonzero(den < 0) >= 1
    check(ctx, src, rc.BIG, rc.CHECKERBOARD_MAP, "cubic")
    check(ctx, src.astype(np.float64), rc.BIG, rc.CHECKERBOARD_MAP, "cubic", np.float32)


@pytest.mark.parametrize("kernel", rc.KERNELS)
@pytest.mark.parametrize("src_dtype", [np.float32, np.float64])
@pytest.mark.parametrize("dst_dtype", [np.float32, np.float64])
def test_dtype_combinations(ctx, kernel, src_dtype, dst_dtype):
    src = rc.voids("single", src_dtype)
    if src_dtype == np.float64:
        src = src + 1e-9 * rc.terrain(seed=5, dtype=np.float64)   # (bits a float32 cannot hold)
    for shape, map4 in [(rc.BIG, (1.0, 0.5, 1.0, 0.25)), ((40, 70), (1.3, -2.0, 0.7, 3.0)), ((9, 12), (7.1, -0.5, 7.1, 0.0))]:
        out, _ = check(ctx, src, shape, map4, kernel, dst_dtype)
        assert out.dtype == dst_dtype


def test_uint8_takes_nearest_only(ctx):
    mask = (rc.terrain() > 1000).view(np.uint8)
    for shape, map4 in [(rc.BIG, (1.0, 0.0, 1.0, 0.0)), ((70, 90), (1.0, -3.5, 1.0, -4.25)), ((150, 205), (0.4, 0.1, 0.4, 0.2)), ((17, 23), (3.7, -0.5, 3.7, 0.25))]:
        out, count = check(ctx, mask, shape, map4, "nearest")
        assert out.dtype == np.uint8
    assert call(ctx, mask, rc.BIG, (1.0, 0.0, 1.0, 0.0), "bilinear") == -1          # XDEMHIP_EINVAL
    assert call(ctx, mask, rc.BIG, (1.0, 0.0, 1.0, 0.0), "nearest", np.float32) == -1
    assert call(ctx, rc.terrain(), rc.BIG, (-1.0, 0.0, 1.0, 0.0), "bilinear") == -1
    assert call(ctx, rc.terrain(), rc.BIG, (1.0, np.nan, 1.0, 0.0), "bilinear") == -1
    assert call(ctx, rc.terrain(), (2, 2), (5000.0, 0.0, 5000.0, 0.0), "cubic") == -5   # XDEMHIP_EUNSUPPORTED: 20001^2 taps per pixel
    with pytest.raises(ValueError, match="nearest"):
        reproject.regrid(mask.view(bool), (1, 0, 0, 0, -1, 61), rc.BIG, (1, 0, 0.5, 0, -1, 61), "bilinear")


# ---- end to end on 61 x 83 grids ----------------------------------------------------------------------------------------------------
T_REF = (10.0, 0.0, 500.0, 0.0, -10.0, 9000.0)
T_HALF = (10.0, 0.0, 505.0, 0.0, -10.0, 9005.0)        # moved by half a pixel
T_COARSE = (15.0, 0.0, 495.0, 0.0, -15.0, 9010.0)      # 1.5 x the resolution


def test_dem_reproject_matches_the_oracle(big):
    tba = DEM(rc.voids("hole"), T_HALF, crs="EPSG:32633", nodata=-9999)
    ref = DEM(big, T_REF, crs="EPSG:32633")
    for kernel in rc.KERNELS:
        out = tba.reproject(ref, resampling=kernel)
        expect, _ = ro.regrid_between(tba.data, T_HALF, rc.BIG, T_REF, kernel)
        assert out is not tba and out.transform == T_REF and out.crs == tba.crs and out.nodata == -9999 and out.shape == ref.shape
        assert same((out.data, 0), (expect, 0))
    out64 = tba.reproject(res=15.0, dtype=np.float64, resampling="cubic")
    shape, t = ro.target_grid(rc.BIG, T_HALF, res=15.0)
    assert out64.shape == shape == (41, 55) and out64.transform == t and out64.dtype == np.float64
    assert same((out64.data, 0), (ro.regrid_between(tba.data, T_HALF, shape, t, "cubic", np.float64)[0], 0))
    forced = DEM(np.where(np.isnan(tba.data), np.float32(-7), tba.data), T_HALF).reproject(ref, force_source_nodata=-7, nodata=-7)
    assert forced.nodata == -7 and same((forced.data, 0), (ro.regrid_between(tba.data, T_HALF, rc.BIG, T_REF, "bilinear")[0], 0))


def test_regrid_takes_device_tensors_and_counts(big):
    import torch

    t = torch.from_numpy(rc.voids("single")).cuda()
    out, count = reproject.regrid(t, T_HALF, rc.BIG, T_REF, "cubic_spline", return_count=True)
    expect = ro.regrid_between(rc.voids("single"), T_HALF, rc.BIG, T_REF, "cubic_spline")
    assert out.is_cuda and same((out.cpu().numpy(), count), expect)
    host, count = reproject.regrid(rc.voids("single"), T_HALF, rc.BIG, T_REF, "cubic_spline", return_count=True)
    assert same((host, count), expect)


def test_reproject_mask_matches_the_oracle_nearest(big):
    mask = big > np.median(big)
    ref = DEM(big, T_COARSE)
    out = reproject.reproject_mask(mask, T_HALF, ref)
    expect, _ = ro.regrid_between(mask.view(np.uint8), T_HALF, rc.BIG, T_COARSE, "nearest")
    assert out.dtype == np.bool_ and np.array_equal(out, expect.astype(bool)) and out.any() and not out.all()


def test_coregistration_takes_the_reprojected_dem(big):
    """What ``coregister_3d`` reads of ``tba.reproject(ref)`` -- the array's bits, dtype and layout, the transform, the CRS and nodata --
    is what it reads of a DEM built around the oracle-regridded array, and the call runs."""
    ref = DEM(big, T_REF, crs="EPSG:32633")
    tba = DEM(rc.terrain(seed=0) + np.float32(2.0), T_HALF, crs="EPSG:32633")
    with pytest.raises(NotImplementedError, match="share one grid"):
        tba.coregister_3d(ref, coreg.NuthKaab(subsample=1))
    moved = tba.reproject(ref)
    on_grid = DEM(ro.regrid_between(tba.data, T_HALF, rc.BIG, T_REF, "bilinear")[0], T_REF, crs="EPSG:32633")
    assert same((moved.data, 0), (on_grid.data, 0)) and moved.data.flags["C_CONTIGUOUS"] and moved.data.dtype == on_grid.data.dtype
    assert (moved.transform, moved.crs, moved.nodata, moved.shape) == (on_grid.transform, on_grid.crs, on_grid.nodata, on_grid.shape)
    aligned = moved.coregister_3d(ref, coreg.NuthKaab(subsample=1))
    assert aligned.transform == T_REF and aligned.shape == rc.BIG and np.count_nonzero(np.isfinite(aligned.data)) > 1000


def test_coregistration_after_reproject_returns_the_same_bits(big):
    """``tba.reproject(ref).coregister_3d(ref, NuthKaab(subsample=1))`` against ``coregister_3d`` of the oracle-regridded array, bit for
    bit.  The two inputs are bit-identical (the test above), so this asks that a ``NuthKaab`` fit on a grid of this size repeats its own
    bits: the y pass of the plain route adds its two sums, which seed ``curve_fit``, in a fixed order (``nk_y_sums_kernel``).  With
    float64 atomics there, eight fits of this pair gave 4 distinct outputs (shift_x between -5.236862 and -5.236307)."""
    ref = DEM(big, T_REF)
    tba = DEM(rc.terrain(seed=0) + np.float32(2.0), T_HALF)
    aligned = tba.reproject(ref).coregister_3d(ref, coreg.NuthKaab(subsample=1))
    on_grid = DEM(ro.regrid_between(tba.data, T_HALF, rc.BIG, T_REF, "bilinear")[0], T_REF)
    expect = on_grid.coregister_3d(ref, coreg.NuthKaab(subsample=1))
    assert aligned.transform == expect.transform and same((aligned.data, 0), (expect.data, 0))


def test_collection_on_the_reference_grid(big):
    stamps = [np.datetime64(f"{y}-01-01") for y in (2000, 2010, 2020)]
    ref = DEM(big, T_REF)
    half = DEM(rc.terrain(seed=1), T_HALF)
    coarse = DEM(rc.terrain(seed=2), T_COARSE)
    with pytest.raises(NotImplementedError, match="reprojection is geoutils' job"):
        DEMCollection([ref, half, coarse], timestamps=stamps).subtract_dems()
    col = DEMCollection.on_reference_grid([ref, half, coarse], timestamps=stamps, reference_dem=0)
    assert col.dems[0] is ref and all(d.shape == ref.shape and d.transform == ref.transform for d in col.dems)
    ddems = col.subtract_dems()
    planes = [big, ro.regrid_between(half.data, T_HALF, rc.BIG, T_REF, "cubic_spline")[0], ro.regrid_between(coarse.data, T_COARSE, rc.BIG, T_REF, "cubic_spline")[0]]
    assert np.array_equal(np.asarray(ddems[0].data), np.zeros(rc.BIG, np.float32))
    for ddem, plane in zip(ddems[1:], planes[1:]):
        with np.errstate(invalid="ignore"):
            assert same((np.asarray(ddem.data), 0), (big - plane, 0))
        assert np.count_nonzero(np.isfinite(np.asarray(ddem.data))) > 1000
