"""xdem_amd.stats on the GPU: xdemhip_raster_stats (csrc/rasterstats.hip, csrc/multi_select.h) against the NumPy restatement of
tests/stats_oracle.py, under every value of the "selection" option (the comparison itself: tests/stats_cases.py, shared with
test_stats_routes_gpu.py).

Order-statistic keys (Median, Max, Min, 90th percentile, LE90, NMAD) and the counts: bit for bit (by value: +-0.0 compare equal).
Summed keys: bounds that hold for ANY order of a float64 summation of n terms (u = 2^-53), so derived, not measured:
  |Sum - fsum(v64)| <= n u sum|v64|, Mean that / n;  Sum of squares, sum of squared deviations: relative 2 n u (one rounding per square --
  three for a squared deviation -- and n - 1 per sum);  RMSE, Standard deviation: relative n u + 2 ulp (the square root halves the
  relative error; a division and the root round once each).
A dropped or doubled pixel moves a sum by about 1 / n of sum|v|: orders of magnitude outside these bounds at the sizes used here.
Every route returns the same bits: asserted on the whole output block."""
import ctypes

import numpy as np
import pytest

import stats_oracle
from stats_cases import EXACT, bits, check, check_block, mixed, run, same
from xdem_amd import DEM, _lib, stats

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = _lib.default_context()
    c.set_option("selection", 0)
    yield c
    c.set_option("selection", 0)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_tiny_inputs(ctx, dtype):
    check(np.array([[3.5]], dtype=dtype), ctx)
    for nvalid in (1, 2, 3):   # rank clipping, lo == hi
        a = np.full((7, 9), np.nan, dtype=dtype)
        a.reshape(-1)[[11, 40, 62][:nvalid]] = [2.5, -7.0, 11.25][:nvalid]
        check(a, ctx)
    blocks = check(np.full((7, 9), np.nan, dtype=dtype), ctx)
    assert all(b["n"] == 0 and b["n_valid"] == 0 for b in blocks.values())


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_mixed_raster(ctx, dtype):
    a, inl = mixed(dtype)
    check(a, ctx, None, -9999.0)
    check(a, ctx, inl, -9999.0)
    check(np.ma.MaskedArray(a, mask=~inl), ctx, None, -9999.0)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_constant_raster(ctx, dtype):
    """Every rank shares one prefix at every digit.  Bracketed, every element is a candidate: more than the candidate buffer (half the
    raster + 4096) holds at this size -- the fall-back."""
    a = np.full((129, 193), 5.25, dtype=dtype)
    check(a, ctx, routes={0: (1, 1), 2: (2, 2), 3: (2, 2)})


def digit_raster(dtype, d):
    """Values whose ordered keys (select.h: key_of) differ ONLY in digit d (0 = the most significant byte): every digit value once,
    shuffled, 16 x 16 -- for d = 0, sign and leading exponent bits, the 128 digit values 0x40 .. 0xBF (|v| < 2, both signs: the squares
    of the others overflow float64 or are no numbers), 8 x 16."""
    nbytes = np.dtype(dtype).itemsize
    K = np.uint32 if nbytes == 4 else np.uint64
    base = K(0xC2123456) if nbytes == 4 else K(0xC012345612345678)
    shift = K(8 * (nbytes - 1 - d))
    digits = np.arange(0x40, 0xC0, dtype=K) if d == 0 else np.arange(256, dtype=K)
    keys = (base & ~(K(0xFF) << shift)) | (digits << shift)
    top = K(1) << K(8 * nbytes - 1)
    vals = np.where(keys & top, keys ^ top, ~keys).astype(K).view(dtype)
    assert np.isfinite(vals.astype(np.float64) ** 2).all() and np.unique(vals).size == digits.size
    return np.random.default_rng(d).permutation(vals).reshape(-1, 16)


@pytest.mark.parametrize("dtype,d", [(np.float32, d) for d in range(4)] + [(np.float64, d) for d in range(8)])
def test_ranks_that_separate_at_one_digit(ctx, dtype, d):
    blocks = check(digit_raster(dtype, d), ctx)
    b = blocks[1]
    picked = [b["med_lo"], b["med_hi"]] + b["q_lo"] + b["q_hi"]
    assert len(set(picked)) == 8   # ranks 127 128 | 229 230 | 242 243 | 12 13 of 256 distinct values (d = 0: 63 64 | 114 115 | 120 121 | 6 7 of 128)
    # four quantiles: all ten states, + ranks 76 77 (d = 0: 38 39); below the last digit ten distinct prefixes, so ten tables a pass
    b = check_block(digit_raster(dtype, d), (0.9, 0.95, 0.05, 0.3), ctx)[1]
    assert len(set([b["med_lo"], b["med_hi"]] + b["q_lo"] + b["q_hi"])) == 10


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("shape", [(257, 513), (1031, 2053)])
def test_shapes(ctx, dtype, shape):
    rng = np.random.default_rng(shape[0])
    a = (1500.0 + 400.0 * rng.standard_normal(shape)).astype(dtype)
    a[rng.random(shape) < 0.2] = np.nan
    inl = rng.random(shape) < 0.9
    # at 1031 x 2053 the brackets hold (6 sigma of the sample ranks) and their union is about a third of the raster
    routes = {0: (1, 1), 2: (2, 2), 3: (0, 0)} if shape[0] > 1000 else {0: (1, 1)}
    check(a, ctx, inl, None, routes)


def test_tensor_input_equals_host_input(ctx):
    import torch

    a, inl = mixed(np.float32)
    for mask in (None, inl):
        _, host = run(a, mask, -9999.0, ctx)
        t = torch.from_numpy(a).cuda()
        _, dev = run(t, mask, -9999.0, ctx)
        _, dev2 = run(t, None if mask is None else torch.from_numpy(mask).cuda(), -9999.0, ctx)
        assert bits(dev) == bits(host) and bits(dev2) == bits(host)
    check(torch.from_numpy(a.astype(np.float64)).cuda(), ctx, inl, -9999.0)
    assert stats.percentile(torch.from_numpy(a).cuda(), 90, nodata=-9999.0) == stats.percentile(a, 90, nodata=-9999.0)


def test_two_calls_return_identical_bits(ctx):
    rng = np.random.default_rng(2)
    a = rng.standard_normal((700, 900)).astype(np.float32) * 1e3   # (sums that round: the order of the additions shows)
    first, second = run(a, None, None, ctx)[1], run(a, None, None, ctx)[1]
    assert bits(first) == bits(second)


def test_percentile_and_linear_error(ctx):
    a, inl = mixed(np.float64)
    qs = [0, 2.5, 10, 50, 66.6, 99, 100]   # (two device calls)
    with np.errstate(invalid="ignore"):
        clean = np.where(np.isfinite(a) & (a != -9999.0) & inl, a, np.nan)
    assert np.array_equal(stats.percentile(a, qs, inlier_mask=inl, nodata=-9999.0, ctx=ctx), np.nanpercentile(clean, qs))
    assert stats.linear_error(a, 68, inlier_mask=inl, nodata=-9999.0, ctx=ctx) == np.nanpercentile(clean, 84) - np.nanpercentile(clean, 16)
    top = a[np.isfinite(a) & (a != -9999.0)].max()   # a callable next to a key: applied on the host to the valid values
    assert stats.get_stats(a, [np.nanmax, "max"], nodata=-9999.0, ctx=ctx) == {"nanmax": top, "max": float(top)}


def test_int16_dem_with_nodata(ctx):
    rng = np.random.default_rng(4)
    z = rng.integers(-300, 3000, size=(61, 83)).astype(np.int16)
    z[rng.random(z.shape) < 0.1] = -32768
    got = DEM(z, nodata=-32768).get_stats()
    want = stats_oracle.table(np.where(z == -32768, np.float32(np.nan), z.astype(np.float32)))
    for k in EXACT:
        if k in want:
            assert same(got[k], want[k]), (k, got[k], want[k])
    assert got["Valid count"] == int((z != -32768).sum()) and got["Total count"] == z.size
    assert got["Sum"] == want["Sum"] and got["Sum of squares"] == want["Sum of squares"]   # (integers: every partial sum is exact)


def test_unsupported_with_a_reduction_hook(ctx):
    CB = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_void_p)
    cb = CB(lambda ptr, count, kind, user: 0)
    a = np.ones((4, 4), np.float32)
    ctx.check(ctx._L.xdemhip_set_allreduce(ctx.handle, ctypes.cast(cb, ctypes.c_void_p), None))
    try:
        out = _lib.RasterStatsOut()
        rc = ctx._L.xdemhip_raster_stats(ctx.handle, a.ctypes.data, _lib.F32, a.size, None, None, 0, 0.0, None, 0, 1.4826, _lib.HOST, ctypes.byref(out))
        assert rc == -5   # XDEMHIP_EUNSUPPORTED
        with pytest.raises(_lib.XdemHipError, match="partitioned"):
            stats.get_stats(a, ctx=ctx)
    finally:
        ctx.check(ctx._L.xdemhip_set_allreduce(ctx.handle, None, None))
    assert stats.get_stats(a, "mean", ctx=ctx) == 1.0
