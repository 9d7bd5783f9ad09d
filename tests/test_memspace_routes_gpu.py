"""Both memory routes of the one-shot entry points give the same bits.

Every entry point below is called through the C ABI twice on the same inputs: with NumPy arrays (``XDEMHIP_HOST``: the library
uploads, runs and downloads) and with torch device tensors (``XDEMHIP_DEVICE``: it uses the caller's memory as it is, on its own
stream).  The host results are pinned to the oracles elsewhere; these tests only tie the device route to the host route, at the
smallest shapes that reach them.  ``xdemhip_convolution`` and ``xdemhip_poly2d_apply`` are not repeated here: their device routes
are compared with the host form in test_convolution_gpu.py and test_biascorr_gpu.py."""
import ctypes

import numpy as np
import pytest

from gpu_helpers import DP, _back, _dev, _dev_empty, _with_nans

pytestmark = pytest.mark.gpu

EINVAL = -1


@pytest.fixture(scope="module")
def ctx():
    from xdem_amd import _lib

    c = _lib.Context(0)
    yield c
    c.close()


def _code(dtype):
    from xdem_amd import _lib

    return _lib.F32 if np.dtype(dtype) == np.float32 else _lib.F64


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("size", [3, 5])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_mean_filter_nan_device_route_equals_the_host_route(ctx, dtype, size):
    from xdem_amd import _lib

    rng = np.random.default_rng(1)
    img = _with_nans(rng, rng.normal(size=(7, 9)).astype(dtype), 5)
    H, W = img.shape

    def call(src, mean, nvalid, memspace):
        npx = ctypes.c_int(-1)
        assert ctx._L.xdemhip_mean_filter_nan(ctx.handle, src, _code(dtype), H, W, size, 1, mean, nvalid, ctypes.byref(npx), memspace) == _lib.OK
        return npx.value

    mean_h, nv_h = np.empty((H, W)), np.empty((H, W))
    npx_h = call(img.ctypes.data, mean_h.ctypes.data, nv_h.ctypes.data, _lib.HOST)
    t, mean_d, nv_d = _dev(img), _dev_empty((H, W), np.float64), _dev_empty((H, W), np.float64)
    npx_d = call(t.data_ptr(), mean_d.data_ptr(), nv_d.data_ptr(), _lib.DEVICE)
    assert npx_h == npx_d == {3: 1, 5: 9}[size]   # (the circular mask keeps the pixels nearer than size // 2 to the centre)
    assert np.isnan(mean_h).any() and np.isfinite(mean_h).any()
    assert _same(_back(ctx, mean_d), mean_h) and _same(_back(ctx, nv_d), nv_h)


@pytest.mark.parametrize("disjoint", [1, 0])
def test_perbin_lookup_device_route_equals_the_host_route(ctx, disjoint):
    """Two variables with 3 and 4 intervals; n = 1000, and n = 5 on views offset by one element, where the device route takes the
    unaligned (scalar) loads and stores while the host route's own buffers are aligned."""
    from xdem_amd import _lib

    rng = np.random.default_rng(2)
    left = np.array([0.0, 1.0, 2.0, 0.0, 0.25, 0.5, 0.75])
    right = np.array([1.0, 2.0, 3.0, 0.25, 0.5, 0.75, 1.0])
    table = rng.normal(size=12)
    decided = np.array([1, 1, 0, 1, 2, 1, 1, 0, 1, 1, 2, 1], dtype=np.uint8)   # 1 passes, 0 stays NaN, 2 counts as missing
    nint = (ctypes.c_int * 2)(3, 4)
    dts = (ctypes.c_int * 2)(_lib.F32, _lib.F64)

    def call(p0, p1, n, out, memspace):
        ptrs = (ctypes.c_void_p * 2)(p0, p1)
        missing = ctypes.c_int64(-1)
        rc = ctx._L.xdemhip_perbin_lookup(ctx.handle, ptrs, dts, 2, n, nint, left.ctypes.data_as(DP), right.ctypes.data_as(DP),
                                          table.ctypes.data_as(DP), decided.ctypes.data_as(ctypes.c_char_p), disjoint, out, ctypes.byref(missing),
                                          memspace)
        assert rc == _lib.OK
        return missing.value

    for n, off in ((1000, 0), (5, 1)):
        v0 = _with_nans(rng, rng.uniform(-0.3, 3.3, n + off).astype(np.float32), 1)
        v1 = _with_nans(rng, rng.uniform(-0.1, 1.1, n + off), 1)
        a0, a1 = np.ascontiguousarray(v0[off:]), np.ascontiguousarray(v1[off:])
        out_h = np.full(n, -7.0)
        miss_h = call(a0.ctypes.data, a1.ctypes.data, n, out_h.ctypes.data, _lib.HOST)
        t0, t1, out_d = _dev(v0), _dev(v1), _dev_empty(n + off, np.float64)
        if off:
            assert t1[off:].data_ptr() % 16 != 0
        miss_d = call(t0[off:].data_ptr(), t1[off:].data_ptr(), n, out_d[off:].data_ptr(), _lib.DEVICE)
        assert miss_h == miss_d
        if n == 1000:
            assert miss_h > 0 and np.isnan(out_h).any() and np.isfinite(out_h).any()
        assert _same(_back(ctx, out_d)[off:], out_h)


@pytest.mark.parametrize("shape", [(5, 7), (1, 7)])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_texture_shading_device_route_equals_the_host_route(ctx, shape, dtype):
    from xdem_amd import _lib

    rng = np.random.default_rng(3)
    dem = _with_nans(rng, (100 + rng.normal(size=shape)).astype(dtype), 1)
    H, W = shape

    def call(src, out, memspace):
        assert ctx._L.xdemhip_texture_shading(ctx.handle, src, _code(dtype), H, W, 0.8, _code(dtype), out, memspace) == _lib.OK

    out_h = np.empty(shape, dtype=dtype)
    call(dem.ctypes.data, out_h.ctypes.data, _lib.HOST)
    t, out_d = _dev(dem), _dev_empty(shape, dtype)
    call(t.data_ptr(), out_d.data_ptr(), _lib.DEVICE)
    assert np.isnan(out_h).sum() == 1
    assert _same(_back(ctx, out_d), out_h)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_apply_matrix_rst_device_route_equals_the_host_route(ctx, dtype):
    from xdem_amd import _lib

    rng = np.random.default_rng(4)
    dem = _with_nans(rng, (50 + np.cumsum(rng.normal(size=(6, 5)), axis=1)).astype(dtype), 1)
    H, W = dem.shape
    t6 = (ctypes.c_double * 6)(10.0, 0.0, 100.0, 0.0, -10.0, 200.0)
    a = np.deg2rad(0.5)
    m = np.eye(4)
    m[:3, :3] = [[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]]
    m[:3, 3] = (3.0, -2.0, 0.25)
    m16 = (ctypes.c_double * 16)(*m.ravel())

    def call(src, out, memspace):
        assert ctx._L.xdemhip_apply_matrix_rst(ctx.handle, src, _code(dtype), H, W, t6, m16, None, out, memspace) == _lib.OK

    out_h = np.empty_like(dem)
    call(dem.ctypes.data, out_h.ctypes.data, _lib.HOST)
    t, out_d = _dev(dem), _dev_empty(dem.shape, dtype)
    call(t.data_ptr(), out_d.data_ptr(), _lib.DEVICE)
    assert np.isfinite(out_h).any()
    assert _same(_back(ctx, out_d), out_h)


def test_interp_grid_linear_device_route_equals_the_host_route(ctx):
    from xdem_amd import _lib

    rng = np.random.default_rng(5)
    n = 300
    axes = np.array([0.0, 1.0, 2.5, -1.0, 0.0, 0.5, 2.0])   # a 3 x 4 grid
    n_axis = (ctypes.c_int * 2)(3, 4)
    grid = rng.normal(size=12)
    v0 = _with_nans(rng, rng.uniform(-0.5, 3.0, n).astype(np.float32), 3)   # (points outside the grid extrapolate)
    v1 = _with_nans(rng, rng.uniform(-1.5, 2.5, n), 3)
    dts = (ctypes.c_int * 2)(_lib.F32, _lib.F64)

    def call(p0, p1, out, memspace):
        ptrs = (ctypes.c_void_p * 2)(p0, p1)
        rc = ctx._L.xdemhip_interp_grid_linear(ctx.handle, 2, axes.ctypes.data_as(DP), n_axis, grid.ctypes.data_as(DP), ptrs, dts, n, 1.5,
                                               ctypes.cast(out, DP), memspace)
        assert rc == _lib.OK

    out_h = np.empty(n)
    call(v0.ctypes.data, v1.ctypes.data, out_h.ctypes.data, _lib.HOST)
    t0, t1, out_d = _dev(v0), _dev(v1), _dev_empty(n, np.float64)
    call(t0.data_ptr(), t1.data_ptr(), out_d.data_ptr(), _lib.DEVICE)
    assert 0 < np.isnan(out_h).sum() <= 6
    assert _same(_back(ctx, out_d), out_h)


@pytest.mark.parametrize("abs_limit", [np.inf, 1.0])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_nmad_device_route_equals_the_host_route(ctx, dtype, abs_limit):
    from xdem_amd import _lib

    rng = np.random.default_rng(6)
    n = 1000
    v = _with_nans(rng, rng.normal(size=n).astype(dtype), 10)
    assert (np.abs(v) > 1.0).any()   # (the finite limit removes some values)

    def call(src, memspace):
        med, nm, cnt = ctypes.c_double(), ctypes.c_double(), ctypes.c_int64(-1)
        rc = ctx._L.xdemhip_nmad(ctx.handle, src, _code(dtype), n, 1.4826, float(abs_limit), memspace, ctypes.byref(med), ctypes.byref(nm),
                                 ctypes.byref(cnt))
        assert rc == _lib.OK
        return np.array([med.value, nm.value]).tobytes(), cnt.value

    host = call(v.ctypes.data, _lib.HOST)
    t = _dev(v)
    dev = call(t.data_ptr(), _lib.DEVICE)
    assert host == dev
    assert host[1] == np.count_nonzero(np.abs(v) <= abs_limit)
    assert np.array_equal(_back(ctx, t), v, equal_nan=True)   # (the caller's device array is left as it was)


@pytest.mark.parametrize("self_sum", [True, False])
def test_cov_double_sum_device_route_equals_the_host_route(ctx, self_sum):
    """na = 70, nb = 130 is one workgroup: its sum has one order.  (Larger sets combine their workgroups' sums with float64 atomic
    additions, whose order, and so the last bits, differ from run to run on either route.)"""
    from xdem_amd import _lib

    rng = np.random.default_rng(7)
    na, nb = 70, 130
    a = [rng.uniform(0, 500, na), rng.uniform(0, 500, na), rng.uniform(0.5, 2.0, na)]
    b = [rng.uniform(0, 500, nb), rng.uniform(0, 500, nb), rng.uniform(0.5, 2.0, nb)]
    types = (ctypes.c_int * 2)(0, 2)   # spherical + gaussian
    ranges, psills, smooth = np.array([120.0, 400.0]), np.array([0.7, 0.3]), np.ones(2)

    def call(pa, pb, memspace):
        out = ctypes.c_double(-1.0)
        pa = [ctypes.cast(p, DP) for p in pa]
        pb = [None, None, None] if self_sum else [ctypes.cast(p, DP) for p in pb]
        rc = ctx._L.xdemhip_cov_double_sum(ctx.handle, pa[0], pa[1], pa[2], na, pb[0], pb[1], pb[2], 0 if self_sum else nb, 2, types,
                                           ranges.ctypes.data_as(DP), psills.ctypes.data_as(DP), smooth.ctypes.data_as(DP), ctypes.byref(out), memspace)
        assert rc == _lib.OK
        return out.value

    host = call([x.ctypes.data for x in a], [x.ctypes.data for x in b], _lib.HOST)
    ta, tb = [_dev(x) for x in a], [_dev(x) for x in b]
    dev = call([t.data_ptr() for t in ta], [t.data_ptr() for t in tb], _lib.DEVICE)
    assert host > 0.0
    assert np.float64(host).tobytes() == np.float64(dev).tobytes()


def test_a_refused_call_leaves_the_context_usable(ctx):
    """After a call that returns XDEMHIP_EINVAL, a valid call on the same context returns XDEMHIP_OK."""
    from xdem_amd import _lib

    v = np.arange(8, dtype=np.float32)
    med, nm, cnt = ctypes.c_double(), ctypes.c_double(), ctypes.c_int64()

    def call(n, memspace):
        return ctx._L.xdemhip_nmad(ctx.handle, v.ctypes.data, _lib.F32, n, 1.4826, float("inf"), memspace, ctypes.byref(med), ctypes.byref(nm),
                                   ctypes.byref(cnt))

    assert call(0, _lib.HOST) == EINVAL
    assert call(v.size, 7) == EINVAL
    assert call(v.size, _lib.HOST) == _lib.OK
    assert (med.value, cnt.value) == (3.5, 8)
