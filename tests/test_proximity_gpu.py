"""xdemhip_edt on the GPU against the NumPy restatement of its rule (tests/proximity_oracle.py): distances in float64 and float32,
indices and the target count bit for bit -- from host and device memory, from two runs, and under every value of the test switch
``"edt_route"`` (0 automatic, 1 block search in global memory only, 2 minimal band / tile / halo / block).  Then the two small kernels
(target plane, inner boundary), the status codes of refused arguments, and ``DEM.proximity`` / ``Vector.proximity`` /
``create_mask(buffer=)`` end to end.  The shapes come from ``xdemhip_edt_plan`` (tests/proximity_cases.py): the smallest at which a
stage can go wrong."""
import ctypes
import functools

import numpy as np
import pytest

import proximity_cases as pc
import proximity_oracle as po
from gpu_helpers import _dev
from xdem_amd import DEM, Vector, _args, _lib, coreg, proximity

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    return _lib.default_context()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


@functools.lru_cache(maxsize=None)
def _oracle(switch, name, sampling):
    t = dict(pc.cases(switch))[name]
    dist, idx, n = po.separable(t, sampling)
    for a in (dist, idx):   # (shared among the tests that need them)
        a.setflags(write=False)
    return t, dist, idx, n


def run(ctx, targets, sampling, dtype, device, keep=None, polarity=1, indices=True):
    """proximity.edt on host arrays or on device copies: (distances, indices, count) as host arrays."""
    t = _dev(targets) if device else targets
    k = None if keep is None else (_dev(keep) if device else keep)
    dist, idx, n = proximity.edt(t, sampling, dtype, True, indices, k, polarity, ctx=ctx)
    if device:
        assert dist.is_cuda and (idx is None or idx.is_cuda)
        dist, idx = dist.cpu().numpy(), None if idx is None else idx.cpu().numpy()
    return dist, idx, n


def same(got, dist, idx, n, dtype) -> bool:
    want = dist.astype(dtype)
    return got[0].dtype == want.dtype and np.array_equal(bits(got[0]), bits(want)) and got[1].dtype == np.int32 and \
        np.array_equal(got[1], idx) and got[2] == n


@pytest.mark.parametrize("switch", pc.SWITCHES)
@pytest.mark.parametrize("sampling", (pc.EXACT[0], pc.INEXACT[0]))
def test_every_case_bit_for_bit(ctx, switch, sampling):
    with ctx.option_scope("edt_route", switch):
        for name, _ in pc.cases(switch):
            t, dist, idx, n = _oracle(switch, name, sampling)
            host = run(ctx, t, sampling, np.float64, False)
            assert same(host, dist, idx, n, np.float64), (name, "host float64")
            dev = run(ctx, t, sampling, np.float32, True)
            assert same(dev, dist, idx, n, np.float32), (name, "device float32")
            again = run(ctx, t, sampling, np.float64, False)
            assert np.array_equal(bits(again[0]), bits(host[0])) and np.array_equal(again[1], host[1]), (name, "second run")
    if sampling == pc.EXACT[0]:
        t, dist, idx, n = _oracle(switch, "no_target", sampling)
        assert n == 0 and np.all(np.isinf(dist)) and np.all(idx == -1)


@pytest.mark.parametrize("switch", pc.SWITCHES)
def test_dense_samplings_and_dtypes(ctx, switch):
    with ctx.option_scope("edt_route", switch):
        for sampling in (pc.EXACT[2], pc.INEXACT[1], pc.ANISOTROPIC):
            t, dist, idx, n = _oracle(switch, "dense", sampling)
            assert same(run(ctx, t, sampling, np.float32, False), dist, idx, n, np.float32), (sampling, "host float32")
            assert same(run(ctx, t, sampling, np.float64, True), dist, idx, n, np.float64), (sampling, "device float64")
            t, dist, idx, n = _oracle(switch, "ties", sampling)
            assert same(run(ctx, t, sampling, np.float64, True), dist, idx, n, np.float64), (sampling, "ties")


def test_switch_values_return_the_same_bits(ctx):
    """One plane large enough for the automatic constants, under each value of the switch."""
    p = pc.plan(0)
    rng = np.random.default_rng(3)
    t = (rng.random((2 * p["band_rows"] + 3, pc.far_width(p))) < 0.0005).astype(np.uint8)
    t[0, 0] = 1
    outs = []
    for switch in pc.SWITCHES:
        with ctx.option_scope("edt_route", switch):
            outs.append(run(ctx, t, (0.1, 0.3), np.float64, True))
    for o in outs[1:]:
        assert np.array_equal(bits(o[0]), bits(outs[0][0])) and np.array_equal(o[1], outs[0][1]) and o[2] == outs[0][2] == int(t.sum())
    dist, idx, n = po.separable(t, (0.1, 0.3))
    assert same(outs[0], dist, idx, n, np.float64)


@pytest.mark.parametrize("switch", (0, 2))
def test_int32_offsets_at_32768_rows(ctx, switch):
    t = pc.tall()
    assert pc.plan(switch, *t.shape)["offset_bytes"] == 4 and pc.plan(switch, t.shape[0] - 1, 3)["offset_bytes"] == 2
    dist, idx, n = po.separable(t, (1.0, 1.0))
    with ctx.option_scope("edt_route", switch):
        assert same(run(ctx, t, (1.0, 1.0), np.float64, True), dist, idx, n, np.float64)
        short = np.ascontiguousarray(t[:32767])
        d2, i2, n2 = po.separable(short, (1.0, 1.0))
        assert same(run(ctx, short, (1.0, 1.0), np.float64, False), d2, i2, n2, np.float64)


@pytest.mark.parametrize("device", (False, True))
def test_keep_with_both_polarities(ctx, device):
    t, dist, idx, n = _oracle(2, "dense", pc.EXACT[0])
    keep = (np.random.default_rng(8).random(t.shape) < 0.5).astype(np.uint8)
    with ctx.option_scope("edt_route", 2):
        for pol in (0, 1):
            got = run(ctx, t, pc.EXACT[0], np.float32, device, keep=keep, polarity=pol)
            want = po.kept(dist.astype(np.float32), keep, pol)
            assert np.array_equal(bits(got[0]), bits(want)) and np.array_equal(got[1], idx) and got[2] == n, pol
            assert np.any(want[keep != pol] == 0) and np.any(want[keep == pol] > 0)
    only_idx = proximity.edt(t, None, np.float64, False, True, ctx=ctx)
    assert only_idx[0] is None and np.array_equal(only_idx[1], idx)


def test_target_plane_kernel(ctx):
    a = pc.raster_values()
    for device in (False, True):
        back = (lambda x: x.cpu().numpy()) if device else (lambda x: x)
        src = (lambda x: _dev(x)) if device else (lambda x: x)
        assert np.array_equal(back(proximity.target_plane(src(a), ctx=ctx)), po.target_plane(a))
        assert np.array_equal(back(proximity.target_plane(src(a.astype(np.float64)), [7.0, -2.5, np.nan], ctx=ctx)), po.target_plane(a, [7.0, -2.5]))
        u8 = (np.arange(a.size, dtype=np.uint8) % 5).reshape(a.shape)
        assert np.array_equal(back(proximity.target_plane(src(u8), ctx=ctx)), po.target_plane(u8))
        i32 = (np.arange(a.size, dtype=np.int32).reshape(a.shape) % 11) - 5
        values = list(range(-5, 6)) + [100 + k for k in range(53)]   # 64 values
        assert np.array_equal(back(proximity.target_plane(src(i32), values, ctx=ctx)), po.target_plane(i32, values))
        assert np.array_equal(back(proximity.target_plane(src(i32), [-5, 3], ctx=ctx)), po.target_plane(i32, [-5, 3]))
    got = proximity.distance_transform_edt(a, sampling=(2.5, 0.5), return_indices=True, ctx=ctx)
    want = po.edt_zeros(a, (2.5, 0.5))
    assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(got[1], want[1])


def test_boundary_kernel(ctx):
    m = np.zeros((37, 70), np.uint8)
    m[0:9, 0:12] = 1          # touches the raster's edge
    m[20, 3:66] = 1           # one pixel wide, across a 64-column tile
    m[25:36, 60:70] = 1
    m[30, 64] = 0             # a hole
    for device in (False, True):
        got = proximity.inner_boundary(_dev(m) if device else m, ctx=ctx)
        got = got.cpu().numpy() if device else got
        assert got.dtype == np.uint8 and np.array_equal(got, po.inner_boundary(m)), device
    assert np.array_equal(proximity.inner_boundary(np.ones((1, 1), bool), ctx=ctx), [[0]])


def test_refused_arguments_return_status_codes(ctx):
    L = ctx._L
    t = np.ones((4, 5), np.uint8)
    d = np.zeros((4, 5), np.float64)
    n = ctypes.c_int64()

    def edt(H=4, W=5, sy=1.0, sx=1.0, dtype=_lib.F64, targets=t, memspace=_lib.HOST):
        return L.xdemhip_edt(ctx.handle, _args.ptr(targets), H, W, sy, sx, _args.ptr(d), dtype, None, None, 1, memspace, ctypes.byref(n))

    assert edt() == _lib.OK and n.value == 20 and not d.any()
    for kw in (dict(H=0), dict(W=0), dict(H=-3), dict(W=1 << 31), dict(sy=0.0), dict(sx=-1.0), dict(sy=float("inf")), dict(sx=float("nan")),
               dict(dtype=_lib.U8), dict(dtype=7), dict(targets=None), dict(memspace=5)):
        assert edt(**kw) == -1, kw
    out = np.zeros(20, np.uint8)
    src = np.zeros(20, np.float32)
    vals = np.arange(65.0)
    targets = lambda n_values=0, code=_lib.F32, count=20: L.xdemhip_edt_targets(ctx.handle, _args.ptr(src), code, count, _args.dp(vals), n_values,
                                                                               _args.ptr(out), _lib.HOST)
    assert targets() == _lib.OK and targets(64) == _lib.OK
    assert targets(65) == -1 and targets(-1) == -1 and targets(code=9) == -1 and targets(count=0) == -1
    assert L.xdemhip_mask_boundary(ctx.handle, _args.ptr(t), 0, 5, _args.ptr(out), _lib.HOST) == -1
    with pytest.raises(_lib.XdemHipError):
        ctx.set_option("edt_route", 3)
    ms = proximity.DeviceEngine.stage_ms(ctx)
    assert len(ms) == 4 and all(v >= 0 for v in ms)


# ---- end to end ---------------------------------------------------------------------------------------------------------------------
def test_dem_proximity_without_a_vector(ctx):
    a = pc.raster_values()
    dem = DEM(a, pc.GRID_TRANSFORM, crs="EPSG:32645")
    out = dem.proximity()
    want = po.separable(po.target_plane(a), (30.0, 20.0))[0].astype(np.float32)
    assert isinstance(out, DEM) and out.transform == dem.transform and out.crs == dem.crs and out.nodata is None
    assert np.array_equal(bits(out.data), bits(want))
    out = dem.proximity(target_values=[7.0, -2.5], distance_unit="pixel", dtype=np.float64)
    assert np.array_equal(bits(out.data), bits(po.separable(po.target_plane(a, [7.0, -2.5]), None)[0]))


def test_proximity_with_a_vector_end_to_end(ctx):
    import torch

    import vector_oracle as vo

    v = Vector(pc.POLYGONS, crs="EPSG:32645")
    grid = (pc.GRID_SHAPE, pc.GRID_TRANSFORM)
    mask = vo.mask([v.tables()], *grid)
    assert np.array_equal(v.create_mask(grid), mask)
    host_dem = DEM(np.zeros(pc.GRID_SHAPE, np.float32), pc.GRID_TRANSFORM)
    from xdem_amd.ddem import raster_of

    dev_dem = raster_of(torch.zeros(pc.GRID_SHAPE, device="cuda"), pc.GRID_TRANSFORM)
    for geometry_type in proximity.GEOMETRY_TYPES:
        for in_or_out in proximity.IN_OR_OUT:
            want = po.proximity(mask, (30.0, 20.0), geometry_type, in_or_out, np.float32)
            got = host_dem.proximity(v, geometry_type=geometry_type, in_or_out=in_or_out)
            assert isinstance(got.data, np.ndarray) and np.array_equal(bits(got.data), bits(want)), (geometry_type, in_or_out)
            got = dev_dem.proximity(v, geometry_type=geometry_type, in_or_out=in_or_out)
            assert got.data.is_cuda and np.array_equal(bits(got.data.cpu().numpy()), bits(want)), (geometry_type, in_or_out, "device")
    out = v.proximity(size=(40, 25), distance_unit="pixel", dtype=np.float64)
    shape, t6 = v.size_grid((40, 25))
    assert out.shape == shape and out.transform == t6
    assert np.array_equal(bits(out.data), bits(po.proximity(vo.mask([v.tables()], shape, t6), None, dtype=np.float64)))
    for r in (45.0, -45.0):
        want = po.buffered(mask, (30.0, 20.0), r)
        assert np.array_equal(v.create_mask(grid, buffer=r), want), r
        got = v.create_mask(grid, buffer=r, device=True)
        assert got.is_cuda and got.dtype == torch.bool and np.array_equal(got.cpu().numpy(), want), r
    assert v.create_mask(grid, buffer=0) is v.create_mask(grid)


def test_proximity_plane_as_a_bias_variable_on_the_device(ctx):
    """The float32 plane of DEM.proximity, still on the device, as the variable of BiasCorr: the same fit as from its host copy."""
    import torch

    from xdem_amd.ddem import raster_of

    rng = np.random.default_rng(11)
    shape = pc.GRID_SHAPE
    v = Vector(pc.POLYGONS)
    prox = raster_of(torch.zeros(shape, device="cuda"), pc.GRID_TRANSFORM).proximity(v, geometry_type="polygon")
    assert prox.data.is_cuda and prox.data.dtype == torch.float32
    plane = prox.data.cpu().numpy()
    assert np.array_equal(bits(plane), bits(po.proximity(v.create_mask((shape, pc.GRID_TRANSFORM)), (30.0, 20.0), "polygon")))
    ref = rng.normal(size=shape).astype(np.float32)
    tba = ref + (0.01 * plane / max(1.0, float(plane.max()))).astype(np.float32) + rng.normal(scale=0.01, size=shape).astype(np.float32)
    fits = []
    for device in (True, False):
        conv = _dev if device else (lambda x: x)
        var = prox.data if device else plane   # (the device plane itself: nothing is fetched)
        step = coreg.BiasCorr(fit_or_bin="bin", bin_sizes=8, bias_var_names=["proximity"])
        step.fit(conv(ref), conv(tba), bias_vars={"proximity": var})
        out = step.apply(conv(tba), bias_vars={"proximity": var})
        assert _args.is_tensor(out) == device
        fits.append((step.meta["outputs"]["fitorbin"]["bin_dataframe"]["nanmedian"].values, out.cpu().numpy() if device else np.asarray(out)))
    assert np.array_equal(fits[0][0], fits[1][0], equal_nan=True) and np.isfinite(fits[0][0]).sum() >= 4
    assert np.array_equal(fits[0][1], fits[1][1], equal_nan=True)
