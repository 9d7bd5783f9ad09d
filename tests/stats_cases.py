"""What test_stats_gpu.py and test_stats_routes_gpu.py share, and test_stats_routes_host.py checks without a device: the comparison of
``get_stats`` (``check``) and of one device call (``check_block``) with tests/stats_oracle.py under every value of the "selection"
option, and the inputs built to send the bracketed route of xdemhip_raster_stats down each of its branches (``CASES``).

Order statistics and counts: exact.  Sums: bounds that hold for ANY order of a float64 summation of n terms (u = 2^-53), derived, not
measured:  |Sum - fsum(v64)| <= n u sum|v64|, Mean that / n;  Sum of squares, sum of squared deviations: relative 2 n u (one rounding
per square -- three for a squared deviation -- and n - 1 per sum);  RMSE, Standard deviation: relative n u + 2 ulp (the square root
halves the relative error; a division and the root round once each).

A case names the route it is about; ``build`` derives from stats_oracle.predict_rounds -- a restatement of the sample and
of the bracket ends, never of a result -- that the input has the property that sends the device there.  A round stays bracketed when
every wanted rank lies in its bracket, the union of the brackets fits the candidate buffer and no workgroup stages more than its
staging buffer holds between two flushes.  HELD rounds are asserted with the candidates at most 0.8 of the capacity: any nearer and
a case could drift onto the fall-back without a test noticing why."""
from __future__ import annotations

import math
import struct

import numpy as np

import stats_oracle
from xdem_amd import stats

U = 2.0 ** -53
EXACT = ("Median", "Max", "Min", "90th percentile", "LE90", "NMAD", "Valid count", "Total count", "Percentage valid points") + stats.INLIER_KEYS
QS = (0.9, 0.95, 0.05)      # get_stats' own quantiles
BIG = (1031, 2053)          # the smallest shape at which the four brackets of QS fit the candidate buffer with room to spare
MID = 300000                # ... and one bracket alone (qs = ())
BRACKET_MIN_N = 1 << 22     # SEL_BRACKET_MIN_N: from here on "selection" 0 brackets too
HOST_N_CU = 256             # the compute units of an MI355X: what the host tests derive the preconditions for
FILL = 0.8                  # of the candidate buffer, at most, in a round asserted as bracketed
BLOCK_EXACT = ("n", "n_valid", "n_inlier", "min", "max", "med_lo", "med_hi", "median", "q_lo", "q_hi", "mad_lo", "mad_hi", "nmad")


def run(values, mask, nodata, ctx):
    """get_stats (all keys) and the device block behind it."""
    blocks = []
    orig = stats._device_stats

    def recording(inp, q, c=None):
        blocks.append(orig(inp, q, c))
        return blocks[-1]

    stats._device_stats = recording
    try:
        s = stats.get_stats(values, None, mask, nodata, ctx)
    finally:
        stats._device_stats = orig
    assert len(blocks) == 1
    return s, blocks[0]


def bits(block):
    flat = [block[k] for k in ("n", "n_valid", "n_inlier")] + [block[k] for k in ("min", "max", "sum", "sumsq", "sumdev2", "med_lo", "med_hi", "median",
                                                                                  "mad_lo", "mad_hi", "nmad")] + list(block["q_lo"]) + list(block["q_hi"])
    return [struct.pack("d", float(x)) for x in flat]


def same(a, b):
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    return a == b or (isinstance(a, float) and isinstance(b, float) and math.isnan(a) and math.isnan(b))


def sum_bounds(v64):
    """(exact Sum, Sum of squares, sum of squared deviations of the float64 values; the bound of each for any order of summation)."""
    n = int(v64.size)
    fs, sabs, s2 = math.fsum(v64), math.fsum(np.abs(v64)), math.fsum(v64 * v64)
    dev2 = math.fsum((v64 - fs / n) ** 2)
    return {"sum": (fs, n * U * sabs), "sumsq": (s2, 2 * n * U * s2), "sumdev2": (dev2, 2 * n * U * dev2)}, sabs


def check(values, ctx, mask=None, nodata=None, routes=None):
    """get_stats under every mode against the oracle and against each other; `routes`: {mode: expected route pair}.  Returns the
    blocks by mode."""
    host = values.cpu().numpy() if hasattr(values, "is_cuda") else values
    want = stats_oracle.table(host, mask, nodata)
    v, _, _, _ = stats_oracle.valid_values(host, mask, nodata)
    v64 = v.astype(np.float64)
    n = int(v.size)
    if n:
        exact, sabs = sum_bounds(v64)
    blocks = {}
    try:
        for mode in (0, 1, 2, 3):
            ctx.set_option("selection", mode)
            got, blk = run(values, mask, nodata, ctx)
            blocks[mode] = blk
            assert list(got) == list(want)
            for k in EXACT:
                if k in want:
                    assert same(got[k], want[k]), (mode, k, got[k], want[k])
            if n == 0:
                assert all(math.isnan(got[k]) for k in stats.STAT_KEYS[:11]), (mode, got)
                continue
            s2, dev2 = exact["sumsq"][0], exact["sumdev2"][0]
            fig = {"Sum": (abs(got["Sum"] - want["Sum"]), n * U * sabs), "Mean": (abs(got["Mean"] - want["Mean"]), U * sabs),
                   "Sum of squares": (abs(got["Sum of squares"] - s2), 2 * n * U * s2), "sumdev2": (abs(blk["sumdev2"] - dev2), 2 * n * U * dev2),
                   "RMSE": (abs(got["RMSE"] - want["RMSE"]), want["RMSE"] * (n * U + 4 * U)),
                   "Standard deviation": (abs(got["Standard deviation"] - want["Standard deviation"]), want["Standard deviation"] * (n * U + 4 * U))}
            print(f"mode {mode} n {n} route {blk['route']} reads {blk['reads']:.3f}: " + ", ".join(f"{k} {e:.3e} <= {b:.3e}" for k, (e, b) in fig.items()))
            for k, (e, b) in fig.items():
                assert e <= b, (mode, k, e, b)
            assert blk["route"] == (1, 1) if mode == 1 else True, blk["route"]
            if routes and mode in routes:
                assert blk["route"] == routes[mode], (mode, blk["route"])
    finally:
        ctx.set_option("selection", 0)
    for mode in (0, 2, 3):
        assert bits(blocks[mode]) == bits(blocks[1]), (mode, blocks[mode], blocks[1])
    return blocks


def expected_reads(route, dtype) -> float:
    """Full reads of the raster: per round 1 + 1/64 bracketed (the pass and the sample), one per key byte plain, both after a fall-back."""
    passes = stats_oracle.PASSES[np.dtype(dtype)]
    return float(sum({0: 1 + 1 / 64, 1: passes, 2: 1 + 1 / 64 + passes}[r] for r in route))


def check_block(values, qs, ctx, mask=None, nodata=None, routes=None, modes=(0, 1, 2, 3)):
    """ONE device call (any quantiles) under each of `modes` against stats_oracle.device_block: counts and order statistics exactly,
    the three sums within their bounds, the route named by `routes` ({mode: pair}; mode 1 is (1, 1) always, mode 0 is what mode 3 is
    from BRACKET_MIN_N elements on and (1, 1) below), the reads that route makes, and the same bits from every mode.  Returns the blocks."""
    routes = dict(routes or {})
    inp = stats._Input(values, mask, nodata)
    want = stats_oracle.device_block(inp, qs)
    v, _, _, _ = stats_oracle.valid_values(values, mask, nodata)
    n = int(v.size)
    assert n == want["n"] and n > 0
    exact, _ = sum_bounds(v.astype(np.float64))
    routes[1] = (1, 1)
    if 0 not in routes and (inp.size < BRACKET_MIN_N or 3 in routes):
        routes[0] = (1, 1) if inp.size < BRACKET_MIN_N else routes[3]
    blocks = {}
    try:
        for mode in modes:
            ctx.set_option("selection", mode)
            blk = blocks[mode] = stats._device_stats(inp, qs, ctx)
            for k in BLOCK_EXACT:
                assert same(blk[k], want[k]), (mode, k, blk[k], want[k])
            fig = {k: (abs(blk[k] - x), b) for k, (x, b) in exact.items()}
            print(f"mode {mode} n {n} qs {tuple(qs)} route {blk['route']} reads {blk['reads']:.4f}: " + ", ".join(f"{k} {e:.3e} <= {b:.3e}" for k, (e, b) in fig.items()))
            for k, (e, b) in fig.items():
                assert e <= b, (mode, k, e, b)
            if mode in routes:
                assert blk["route"] == routes[mode], (mode, blk["route"], routes[mode])
            assert blk["reads"] == expected_reads(blk["route"], inp.values.dtype), (mode, blk["route"], blk["reads"])
    finally:
        ctx.set_option("selection", 0)
    for mode in modes:
        assert bits(blocks[mode]) == bits(blocks[1]), (mode, blocks[mode], blocks[1])
    return blocks


def mixed(dtype, shape=(61, 83), seed=1):
    """~20 % NaN, a nodata value, +-Inf, values quantised to 0.25 (ties), both signs, +-0.0, a subnormal; and an inlier mask."""
    rng = np.random.default_rng(seed)
    a = (np.round(rng.normal(scale=300.0, size=shape) * 4) / 4).astype(dtype)
    a[rng.random(shape) < 0.2] = np.nan
    flat = a.reshape(-1)
    flat[5], flat[17], flat[29], flat[31] = np.inf, -np.inf, 0.0, -0.0
    flat[43] = np.finfo(dtype).smallest_subnormal
    flat[rng.choice(flat.size, 40, replace=False)] = -9999.0
    inl = rng.random(shape) < 0.8
    return a, inl


# ---- inputs that send the bracketed route down each of its branches ------------------------------------------------------------------
def gaussian(dtype, n, seed):
    return (1500.0 + 400.0 * np.random.default_rng(seed).standard_normal(n)).astype(dtype)


def unsampled_position(n, after=1000):
    taken = set(stats_oracle.sampled_positions(n).tolist())
    return next(p for p in range(after, n) if p not in taken)


def _mixed_big(dtype, n_cu, variant):
    a, inl = mixed(dtype, BIG)
    if variant == "masked":
        return np.ma.MaskedArray(a, mask=~inl), None
    return a, (inl if variant == "inlier" else None)


def _lattice(dtype, n_cu):
    """Distinct values of both signs, shuffled: multiples of 0.25, exact in float32."""
    n = BIG[0] * BIG[1]
    a = ((np.random.default_rng(21).permutation(n) - n // 2) * 0.25).astype(dtype).reshape(BIG)
    assert np.unique(a).size == n
    return a, None


def _median_only(dtype, n_cu):
    return gaussian(dtype, MID, 31), None


def open_bits_set(x) -> bool:
    """The key bits a bracket end leaves open (all but the leading 24) are not all zero: the high end needs them set to hold x."""
    k = stats_oracle.ordered_keys(np.asarray([x]))[0]
    return bool(int(k) & ((1 << (8 * (k.dtype.itemsize - stats_oracle.BRACKET_DIGITS))) - 1))


def _both_ends(dtype, n_cu):
    """The raster's minimum and maximum are sampled: the brackets of ranks 0 and n - 1, clipped at the sample's extremes, hold them --
    the maximum only through the open low bits of the high end, which are all ones."""
    a = gaussian(dtype, BIG[0] * BIG[1], 41)
    pos = stats_oracle.sampled_positions(a.size)
    a[pos[1234]], a[pos[-4321]] = -5000.123, 9000.123
    assert a.min() == dtype(-5000.123) and a.max() == dtype(9000.123) and open_bits_set(a.max())
    return a.reshape(BIG), None


def _outlier(sign):
    def build(dtype, n_cu):
        """The wanted extreme is ONE outlier the sample does not see, and the next value inwards is sampled: the bracket of rank 0
        (n - 1) ends at the sample's own extreme, and the wanted rank is the first element outside it -- k = lt - 1 (k = lt + in)."""
        a = gaussian(dtype, MID, 43)
        a[stats_oracle.sampled_positions(a.size)[777]] = sign * 9000.123
        a[unsampled_position(a.size)] = sign * 1e6
        srt = np.sort(a)
        assert (srt[0], srt[1]) == (dtype(-1e6), dtype(-9000.123)) if sign < 0 else (srt[-1], srt[-2]) == (dtype(1e6), dtype(9000.123))
        return a, None
    return build


def _offset_sample(dtype, n_cu):
    """The sample sits off centre by three quarters of the half width of a bracket: of its m values only (m - 1) / 2 - 3 h / 4 lie
    below the raster's median.  The median's bracket reaches h sample ranks down and holds the wanted ranks by h / 4 of them; a
    bracket of half that width would miss (test_stats_routes_host.py asserts that too)."""
    rng = np.random.default_rng(61)
    a = gaussian(np.float64, MID, 62)
    pos = stats_oracle.sampled_positions(MID)
    m = pos.size
    below = (m - 1) // 2 - 3 * stats_oracle.halfwidth(m) // 4
    side = rng.permutation(np.repeat([-1.0, 1.0], [below, m - below]))
    a[pos] = np.median(a) + side * np.abs(400.0 * rng.standard_normal(m))
    return a.astype(dtype), None


def _split(dtype, n_cu):
    """+-(1000 + u), the signs exactly balanced; the sampled positions hold +-t, |t| < 1, balanced too.  The two middle values of the
    raster are the sample's own: round 1's bracket holds.  |v - median| is below 1.5 on the sample and above 999 on everything else:
    round 2's bracket ends at the sample's largest and the wanted ranks, near n / 2, lie far above it."""
    n = MID
    rng = np.random.default_rng(47)
    pos = stats_oracle.sampled_positions(n)
    assert pos.size % 2 == 0 and n % 2 == 0

    def signs(k):
        return rng.permutation(np.repeat([1.0, -1.0], k // 2))

    a = np.empty(n)
    rest = np.ones(n, dtype=bool)
    rest[pos] = False
    a[rest] = signs(n - pos.size) * (1000.0 + rng.uniform(0.0, 500.0, n - pos.size))
    a[pos] = signs(pos.size) * rng.uniform(0.001, 1.0, pos.size)
    return a.astype(dtype), None


def _ramp(dtype, n_cu):
    """Sorted in space: every step of a workgroup is all candidates or none."""
    return (0.25 * np.arange(BIG[0] * BIG[1])).astype(dtype).reshape(BIG), None


def _dense(dtype, n_cu):
    """Three whole steps of workgroup 0 lie inside the median's bracket: 3 x 4096 candidates staged between two flushes, in 8192 slots,
    while the candidate buffer is far from full -- the local overflow of BlockStage::append_bounded."""
    G, T = 2 * n_cu, stats_oracle.TILE
    a = gaussian(dtype, 2 * G * T + 3 * T, 53)
    rng = np.random.default_rng(54)
    for s in range(3):
        a[s * G * T:s * G * T + T] = (1500.0 + 1e-3 * rng.standard_normal(T)).astype(dtype)
    return a, None


def _five_trips(dtype, n_cu):
    """The first workgroups take 5 steps: a flush after the 4th, more appends, the final flush.  Workgroup 0's first and fifth steps lie
    whole inside the median's bracket: 4096 + the usual share of three steps before the flush, 4096 after it -- more than 8192 together,
    so the flush inside the loop is what keeps this round bracketed (test_stats_routes_host.py asserts that too)."""
    G, T = 2 * n_cu, stats_oracle.TILE
    a = gaussian(dtype, 4 * G * T + 2 * T + 1, 59)
    rng = np.random.default_rng(60)
    for s in (0, 4):
        a[s * G * T:s * G * T + T] = (1500.0 + 1e-3 * rng.standard_normal(T)).astype(dtype)
    return a, None


F32, F64 = np.float32, np.float64
HELD, FULL, OVER = "held", "held, staging full", "staging overflow"
# name: (builder, quantiles, nodata, dtypes, route under "selection" 3, what sends each round there)
#   HELD: every rank in its bracket, candidates <= FILL x capacity, staging peak <= 8192;  a tuple: the brackets that miss (0 = the
#   median's, 1 + i = quantile i's) while the others hold;  FULL: held, with the staging peak exactly 8192 (every slot written, none
#   refused; at 256 compute units, where 5 of the 512 workgroups take two steps);  OVER: all hold, the candidates fit, one workgroup
#   stages more than 8192
CASES = {
    "mixed": (lambda d, c: _mixed_big(d, c, "plain"), QS, -9999.0, (F32, F64), (0, 0), (HELD, HELD)),
    "mixed-inlier": (lambda d, c: _mixed_big(d, c, "inlier"), QS, -9999.0, (F32, F64), (0, 0), (HELD, HELD)),
    "mixed-masked": (lambda d, c: _mixed_big(d, c, "masked"), QS, -9999.0, (F32, F64), (0, 0), (HELD, HELD)),
    "close-quantiles": (_lattice, (0.45, 0.55, 0.4, 0.6), None, (F32, F64), (0, 0), (HELD, HELD)),
    "repeated-quantiles": (_lattice, (0.5,) * 4, None, (F32, F64), (0, 0), (HELD, HELD)),
    "median-only": (_median_only, (), None, (F32, F64), (0, 0), (HELD, HELD)),
    "both-ends": (_both_ends, (0.0, 1.0), None, (F32, F64), (0, 0), (HELD, HELD)),
    "low-outlier": (_outlier(-1.0), (0.0,), None, (F32, F64), (2, 0), ((1,), HELD)),
    "high-outlier": (_outlier(1.0), (1.0,), None, (F32, F64), (2, 0), ((1,), HELD)),
    "offset-sample": (_offset_sample, (), None, (F32, F64), (0, 0), (HELD, HELD)),
    "split": (_split, (), None, (F32, F64), (0, 2), (HELD, (0,))),
    "ramp": (_ramp, QS, None, (F32, F64), (0, 0), (FULL, HELD)),
    "dense-block": (_dense, (), None, (F32,), (2, 0), (OVER, HELD)),
    "five-trips": (_five_trips, QS, None, (F32,), (0, 0), (HELD, HELD)),
}
PARAMS = [(name, dtype) for name, c in CASES.items() for dtype in c[3]]


def build(name, dtype, n_cu):
    """(values, inlier mask, quantiles, nodata, the route under "selection" 3) of a case, with its precondition asserted for a device
    of `n_cu` compute units; also returns the two predictions."""
    builder, qs, nodata, _, route, why = CASES[name]
    values, mask = builder(dtype, n_cu)
    pred = stats_oracle.predict_rounds(values, mask, nodata, qs, n_cu)
    for r, (p, w) in enumerate(zip(pred, why)):
        fill = p["candidates"] / p["capacity"]
        print(f"{name} {np.dtype(dtype).name} round {r + 1}: holds {p['holds']} candidates {p['candidates']} / {p['capacity']} = {fill:.3f} "
              f"staging peak {p['peak']} sample {p['sample']} -> route {route[r]}")
        missed = w if isinstance(w, tuple) else ()
        assert p["holds"] == [b not in missed for b in range(len(p["holds"]))], (name, r, p)
        assert fill <= FILL, (name, r, p)
        assert (p["peak"] > stats_oracle.STAGE_CAP) == (w == OVER), (name, r, p)
        assert w != FULL or p["peak"] == stats_oracle.STAGE_CAP, (name, r, p)
        assert route[r] == (0 if w in (HELD, FULL) else 2)
    return values, mask, qs, nodata, route, pred
