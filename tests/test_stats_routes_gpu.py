"""xdemhip_raster_stats on the route it takes at production sizes -- the 1/64 sample, the brackets, ONE fused pass that counts per
bracket and compacts their union, the ranks moved among the candidates (rs_data_pass_kernel<T, true, *>, rs_given_kernel) -- on inputs
built so that the brackets HOLD, or so that a named one does not (tests/stats_cases.py: CASES).

Before a route is asserted, stats_cases.build derives from the sample and the bracket ends (stats_oracle.predict_rounds, with this
device's compute units) that the input has the property that sends the device there, and asserts it: nothing is skipped.  Expected
values are stats_oracle.table / device_block: a sort, math.fsum, NumPy's percentile.  Counts and order statistics compare exactly, the
sums within the bounds derived in stats_cases, every mode returns mode 1's bits, `reads` is exact for the route."""
import numpy as np
import pytest

import stats_cases
import stats_oracle
from stats_cases import CASES, QS, bits, check, check_block, run, same
from xdem_amd import DEM, _lib, stats

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = _lib.default_context()
    c.set_option("selection", 0)
    yield c
    c.set_option("selection", 0)


@pytest.fixture(scope="module")
def n_cu():
    import torch

    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def params(*names):
    return pytest.mark.parametrize("name,dtype", [(n, d) for n in names for d in CASES[n][3]],
                                   ids=[f"{n}-{np.dtype(d).name}" for n in names for d in CASES[n][3]])


@params("mixed", "mixed-inlier", "mixed-masked", "ramp")
def test_get_stats_where_the_brackets_hold(ctx, n_cu, name, dtype):
    """Every key of get_stats with both rounds bracketed.  mixed: values quantised to 0.25 (long runs of ties across the bracket ends),
    20 % NaN, +-Inf, +-0, a subnormal, nodata; alone, with an inlier mask, as a MaskedArray.  ramp: sorted in space, so a workgroup's
    steps are all candidates or none and the staging buffer of the workgroups that take two steps is filled to its last slot."""
    values, mask, qs, nodata, route, _ = stats_cases.build(name, dtype, n_cu)
    assert qs == QS
    check(values, ctx, mask, nodata, routes={0: (1, 1), 3: route})


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_device_tensor_and_device_mask_on_the_holding_route(ctx, n_cu, dtype):
    import torch

    a, inl, _, nodata, route, _ = stats_cases.build("mixed-inlier", dtype, n_cu)
    ctx.set_option("selection", 3)
    try:
        _, host = run(a, inl, nodata, ctx)
        t = torch.from_numpy(a).cuda()
        _, dev = run(t, torch.from_numpy(inl).cuda(), nodata, ctx)
        _, dev_host_mask = run(t, inl, nodata, ctx)
    finally:
        ctx.set_option("selection", 0)
    assert host["route"] == dev["route"] == dev_host_mask["route"] == route
    assert bits(dev) == bits(host) and bits(dev_host_mask) == bits(host)
    want = stats_oracle.device_block(stats._Input(a, inl, nodata), QS)
    for k in stats_cases.BLOCK_EXACT:
        assert same(dev[k], want[k]), (k, dev[k], want[k])


@params("close-quantiles", "repeated-quantiles", "both-ends")
def test_five_brackets_and_clipped_ends(ctx, n_cu, name, dtype):
    """Ten states in five brackets -- overlapping in part (candidates of OTHER brackets lie below a bracket: nc = lt - bcnt[2][b] of
    rs_given_kernel), or five times the same one -- and the brackets of ranks 0 and n - 1, clipped at the sample's extremes."""
    values, mask, qs, nodata, route, _ = stats_cases.build(name, dtype, n_cu)
    check_block(values, qs, ctx, mask, nodata, routes={3: route})


@params("median-only", "offset-sample")
def test_no_quantile(ctx, n_cu, name, dtype):
    """nq = 0: round 1 runs the one-bracket pass as well (rs_data_pass_kernel<T, true, 1>).  offset-sample: the wanted ranks lie
    three quarters of the half width away from the sample's own."""
    values, mask, qs, nodata, route, _ = stats_cases.build(name, dtype, n_cu)
    check_block(values, qs, ctx, mask, nodata, routes={3: route, 2: (2, 2)})


@params("low-outlier", "high-outlier", "split", "dense-block")
def test_one_round_falls_back_and_the_other_holds(ctx, n_cu, name, dtype):
    """(2, 0): the bracket of rank 0 (n - 1) ends at the sample's extreme and the raster holds one value beyond it; or one workgroup
    stages more candidates between two flushes than its buffer holds while the candidate buffer has room (append_bounded).
    (0, 2): round 2's bracket of |v - median| lies below its wanted ranks.  The round that misses is cleared and run again mid-call."""
    values, mask, qs, nodata, route, _ = stats_cases.build(name, dtype, n_cu)
    assert route in ((2, 0), (0, 2))
    check_block(values, qs, ctx, mask, nodata, routes={3: route})


@params("five-trips")
def test_flush_inside_the_loop(ctx, n_cu, name, dtype):
    """The first workgroups take 5 steps: the flush after the 4th, more appends, the final flush.  The one large case: two modes."""
    values, mask, qs, nodata, route, _ = stats_cases.build(name, dtype, n_cu)
    assert values.size >= stats_cases.BRACKET_MIN_N
    check_block(values, qs, ctx, mask, nodata, routes={3: route}, modes=(1, 3))


# ---- nodata: rounded to the raster's dtype before it is compared ----------------------------------------------------------------------
def nodata_raster(dtype, nodata, shape=(61, 83)):
    rng = np.random.default_rng(9)
    a = rng.normal(scale=30.0, size=shape).astype(dtype)
    a[rng.random(shape) < 0.1] = dtype(nodata)
    a[rng.random(shape) < 0.1] = np.nan
    return a


@pytest.mark.parametrize("dtype,nodata", [(np.float32, -3.4e38), (np.float32, 0.1), (np.float64, 0.1)])
def test_nodata_is_rounded_to_the_dtype(ctx, dtype, nodata):
    a = nodata_raster(dtype, nodata)
    keep = np.isfinite(a) & (a != dtype(nodata))
    assert 0.7 * a.size < keep.sum() < 0.9 * a.size and (a == dtype(nodata)).sum() > 0.05 * a.size
    blocks = check(a, ctx, None, nodata)   # (the oracle: NumPy's own `v != nodata`)
    assert all(b["n"] == keep.sum() for b in blocks.values())
    assert stats.get_stats(a, np.size, nodata=nodata, ctx=ctx) == keep.sum()
    assert stats.get_stats(a, [np.size, "Valid count"], nodata=nodata, ctx=ctx) == {"size": keep.sum(), "Valid count": keep.sum()}
    dem, direct = DEM(a, nodata=nodata).get_stats(), stats.get_stats(a, nodata=nodata, ctx=ctx)
    assert list(dem) == list(direct)
    for k in direct:
        assert same(dem[k], direct[k]), (k, dem[k], direct[k])
    # the same values widened: float32(nodata) as a float64 is not `nodata` unless it was exact
    if dtype is np.float32:
        wide = stats.get_stats(a.astype(np.float64), "Valid count", nodata=nodata, ctx=ctx)
        assert wide == int(np.isfinite(a).sum())
