"""Without a GPU: the inputs test_stats_routes_gpu.py asserts a route on have the property that sends xdemhip_raster_stats there
(tests/stats_cases.py: CASES, derived for the 256 compute units of an MI355X); the restatement those derivations rest on
(stats_oracle.predict_round) against a count made element by element; and the nodata rule of get_stats on the host path."""
import math
import struct

import numpy as np
import pytest

import stats_cases
import stats_oracle
from stats_cases import HOST_N_CU
from xdem_amd import DEM, stats


def test_sampled_positions():
    """One 8-element line of every 64: the hash written out with Python integers."""
    for n in (1, 8, 511, 512, 513, 4096, 300000, 1031 * 2053):
        lines = -(-n // 8)
        want = []
        for g in range(-(-lines // 64)):
            line = 64 * g + (((g * 0x9E3779B97F4A7C15) % (1 << 64)) >> 58)
            want += [p for p in range(8 * line, 8 * line + 8) if p < n]
        got = stats_oracle.sampled_positions(n)
        assert got.tolist() == want, n
        assert n < 512 or abs(len(want) - n / 64) <= 8
    assert stats_oracle.sampled_positions(512).tolist() == list(range(8))   # (group 0: the hash of 0 is line 0)


def brute_round(v, ok, qs, n_cu):
    """predict_round element by element, on Python integers: keys from struct, the brackets from sorted lists, every count a loop."""
    fmt, nbits = ("<f", 32) if v.dtype == np.float32 else ("<d", 64)
    full = (1 << nbits) - 1

    def key(x):
        b = int.from_bytes(struct.pack(fmt, x), "little")
        return b ^ full if b >> (nbits - 1) else b | (1 << (nbits - 1))

    n = v.size
    keys = [key(x) for x in v.tolist()]
    sample = sorted(keys[p] for p in stats_oracle.sampled_positions(n).tolist() if ok[p])
    pop = sorted(k for k, o in zip(keys, ok.tolist()) if o)
    m, c = len(sample), len(pop)
    low = (1 << (nbits - 24)) - 1
    h = int(3.0 * math.sqrt(8.0 * m)) + 32
    ends = []
    for q in [None] + list(qs):
        lo, hi = ((m - 1) // 2, m // 2) if q is None else (int(math.floor((m - 1) * q)), min(int(math.floor((m - 1) * q)) + 1, m - 1))
        ends.append((sample[max(lo - h, 0)] & ~low & full, sample[min(hi + h, m - 1)] | low))
    holds = []
    for (klo, khi), q in zip(ends, [None] + list(qs)):
        r0, r1 = ((c - 1) // 2, c // 2) if q is None else (int(math.floor((c - 1) * q)), min(int(math.floor((c - 1) * q)) + 1, c - 1))
        holds.append(klo <= pop[r0] <= khi and klo <= pop[r1] <= khi)
    G = min(-(-n // 4096), 2 * n_cu)
    staged, cands = {}, 0
    for p in range(n):
        if ok[p] and any(klo <= keys[p] <= khi for klo, khi in ends):
            cands += 1
            slot = ((p // 4096) % G, (p // (4096 * G)) // 4)
            staged[slot] = staged.get(slot, 0) + 1
    return {"holds": holds, "candidates": cands, "capacity": n // 2 + 4096, "peak": max(staged.values()), "sample": m}


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_predict_round_against_a_brute_force_count(dtype):
    """18 steps over 2 and over 4 workgroups (9 and 5 steps: three and two groups of steps between flushes), gaps, ties, both signs;
    a shuffled and a spatially sorted input, and an outlier the sample does not see: brackets hold, overlap and miss."""
    n = 70001
    rng = np.random.default_rng(7)
    ok = rng.random(n) > 0.3
    smooth = np.round(rng.normal(scale=40.0, size=n), 1).astype(dtype)
    sorted_in_space = np.sort(smooth)
    outlier = smooth.copy()
    outlier[stats_cases.unsampled_position(n)] = -1e6
    ok[stats_cases.unsampled_position(n)] = True
    seen = set()
    for v, qs in ((smooth, (0.9, 0.95, 0.05)), (sorted_in_space, (0.45, 0.55, 0.4, 0.6)), (outlier, (0.0, 1.0)), (smooth, ())):
        for n_cu in (1, 2):
            got = stats_oracle.predict_round(v, ok, qs, dtype, n_cu)
            assert got == brute_round(v, ok, qs, n_cu), (qs, n_cu)
            seen.update(got["holds"])
    assert seen == {True, False}
    # where the rank pair of a value with no exact float64 product is decided: one float64 multiply, floored
    assert stats_oracle.rank_pair(1000003, 0.95) == (950001, 950002) and stats_oracle.rank_pair(1, 0.3) == (0, 0)
    assert stats_oracle.rank_pair(10, None) == (4, 5) and stats_oracle.rank_pair(11, None) == (5, 5) and stats_oracle.rank_pair(7, 1.0) == (6, 6)


@pytest.mark.parametrize("name,dtype", stats_cases.PARAMS, ids=[f"{n}-{np.dtype(d).name}" for n, d in stats_cases.PARAMS])
def test_case_has_the_property_its_route_needs(name, dtype):
    """stats_cases.build asserts it: held rounds with every rank in its bracket, the candidates within 0.8 of the buffer and the staging
    peak within 8192; missed rounds with the named bracket missing and the others holding; the ramp's peak exactly 8192, the dense
    block's above."""
    values, mask, qs, nodata, route, pred = stats_cases.build(name, dtype, HOST_N_CU)
    n = int(np.asarray(values).size)
    if name in ("mixed", "mixed-inlier", "mixed-masked", "close-quantiles", "repeated-quantiles", "both-ends", "ramp"):
        assert n == 1031 * 2053
    if name == "dense-block":
        assert n == (4 * HOST_N_CU + 3) * 4096 and pred[0]["peak"] == 3 * 4096 and pred[0]["candidates"] < 0.2 * pred[0]["capacity"]
    if name == "five-trips":
        assert n == (8 * HOST_N_CU + 2) * 4096 + 1   # workgroups 0, 1, 2 take a 5th step
        late = stats_oracle.predict_rounds(values, mask, nodata, qs, HOST_N_CU, flush_every=5)[0]   # (one flush, at the end)
        assert 4096 < pred[0]["peak"] <= stats_oracle.STAGE_CAP < late["peak"]
    if name == "offset-sample":   # held by the full half width of the rule only
        full = stats_oracle.halfwidth
        stats_oracle.halfwidth = lambda m: (full(m) - 32) // 2 + 32
        try:
            assert stats_oracle.predict_rounds(values, mask, nodata, qs, HOST_N_CU)[0]["holds"] == [False]
        finally:
            stats_oracle.halfwidth = full
    if name == "close-quantiles":   # the brackets overlap in part: their union is smaller than their sum, larger than any one of them
        one = stats_oracle.predict_rounds(values, mask, nodata, (), HOST_N_CU)[0]["candidates"]
        assert one < pred[0]["candidates"] < 5 * one
    if name == "repeated-quantiles":   # five identical brackets: the union is the median's own
        assert pred[0]["candidates"] == stats_oracle.predict_rounds(values, mask, nodata, (), HOST_N_CU)[0]["candidates"]


def test_smaller_shapes_would_not_hold():
    """Why the four-bracket cases are as large as they are: at 257 x 513 and at 300 000 the union of get_stats' four brackets is larger
    than the candidate buffer; one bracket alone fits at 300 000 with room to spare."""
    for n in (257 * 513, 300000):
        p = stats_oracle.predict_round(stats_cases.gaussian(np.float32, n, 3), np.ones(n, bool), stats_cases.QS, np.float32, HOST_N_CU)
        assert all(p["holds"]) and p["candidates"] > p["capacity"], (n, p)
    p = stats_oracle.predict_round(stats_cases.gaussian(np.float32, 257 * 513, 3), np.ones(257 * 513, bool), (), np.float32, HOST_N_CU)
    assert stats_cases.FILL * p["capacity"] * 0.9 < p["candidates"] <= p["capacity"]   # (fits, but too near the cap to assert a route on)


# ---- nodata: rounded to the raster's dtype before it is compared, as NumPy's `v == nodata` and DEM.__init__ do -----------------------
NODATA_CASES = [(np.float32, -3.4e38), (np.float32, 0.1), (np.float64, 0.1), (np.float64, -9999.0)]


def nodata_raster(dtype, nodata, shape=(4, 5)):
    rng = np.random.default_rng(5)
    a = rng.normal(scale=30.0, size=shape).astype(dtype)
    with np.errstate(over="ignore"):
        a[0, 0] = a[2, 3] = dtype(nodata)
    a[1, 1] = np.nan
    return a


@pytest.mark.parametrize("dtype,nodata", NODATA_CASES)
def test_nodata_is_rounded_to_the_dtype_on_the_host_path(dtype, nodata):
    a = nodata_raster(dtype, nodata)
    with np.errstate(over="ignore"):
        keep = np.isfinite(a) & (a != dtype(nodata))
    assert keep.sum() == a.size - 3
    # a callable statistic needs no device
    assert stats.get_stats(a, np.size, nodata=nodata) == a.size - 3
    assert np.array_equal(stats.get_stats(a, lambda v: v, nodata=nodata), a[keep])
    assert np.array_equal(stats_oracle.valid_values(a, None, nodata)[0], a[keep])
    with stats_oracle.patched():
        s = stats.get_stats(a, nodata=nodata)
        assert s["Valid count"] == a.size - 3 and s["Min"] == float(a[keep].min()) and s["Max"] == float(a[keep].max())
        d = DEM(a, nodata=nodata).get_stats()
    assert list(d) == list(s) and all(stats_cases.same(d[k], s[k]) for k in s)


def test_nodata_that_differs_from_every_pixel_drops_nothing():
    a = nodata_raster(np.float32, 0.1)
    assert stats.get_stats(a, np.size, nodata=0.2) == a.size - 1
    assert stats.get_stats(a, np.size, nodata=float("nan")) == a.size - 1
    assert stats.get_stats(a, np.size, nodata=1e39) == a.size - 1   # (rounds to +Inf: no finite pixel equals it)
    assert stats.get_stats(a.astype(np.float64), np.size, nodata=0.1) == a.size - 1   # (float32(0.1) widened is not 0.1)
