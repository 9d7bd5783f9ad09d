"""Cases and measured figures of the route tests of xdemhip_perbin_lookup, xdemhip_interp_grid_linear and xdemhip_cov_double_sum
(shared by tests/test_lookup_routes_host.py, which asserts what each case is built for on the oracles alone, and
tests/test_lookup_routes_gpu.py).  Every case is built from a seed; no expected value is stored.

The limits restated here are the host dispatch code's: csrc/perbin.hip (PB_LDS_EDGES, PB_LDS_BINS, PB_U, 16 workgroups per compute
unit), csrc/binstats.hip (40 KB of axes and grid values in LDS, 48 KB of axes, 2^24 grid values), csrc/covsum.hip (CV_NT, CV_CHUNK)."""
import functools
import itertools
import math

import numpy as np

import lookup_oracle as lo

# ---- measured figures ----------------------------------------------------------------------------------------------------------------
# K of the covariance sum's bound (cov_bound below), per model kind ("mixed": several kinds in one sum), in units of 2^-52.
# "cpu": the largest |rho_float64 - rho_longdouble| / 2^-52 over the pairs of every case below, NumPy / libm on x86-64 (cubic's
# polynomial cancels near h = r).  "mi355x": the largest (|S_device - S_ref| - summation part) / (2^-52 A) over the same cases,
# 0 where the difference stays inside the summation part; "mi355x_whole": |S_device - S_ref| / (2^-52 A) without that subtraction, for
# the record; "mi355x_pair": the largest |rho_device - rho_longdouble| / 2^-52 over the single pairs of cov_pair_separations, where the
# device's sum IS rho -- the direct measurement of what K stands for.  The bar of the tests is 4 x the largest of "cpu", "mi355x" and
# "mi355x_pair" (the convention for bars that depend on ocml's exp / pow).
MEASURED_ON = "ROCm 7.2.0"
MEASURED = {
    "cpu": {"spherical": 1.29, "exponential": 1.07, "gaussian": 1.24, "cubic": 11.65, "stable": 1.32, "mixed": 1.67},
    "mi355x": {"spherical": 0.0, "exponential": 0.0, "gaussian": 0.0, "cubic": 0.0, "stable": 0.0, "mixed": 0.0},
    "mi355x_whole": {"spherical": 0.0641, "exponential": 0.1982, "gaussian": 0.0685, "cubic": 0.1014, "stable": 0.0645, "mixed": 0.2973},
    "mi355x_pair": {"spherical": 0.94, "exponential": 0.76, "gaussian": 0.75, "cubic": 10.71, "stable": 0.91},
}


def case_id(p) -> str:
    """The id of a parametrised case: the builder's name, then its arguments."""
    return p.__name__ if callable(p) else "-".join(map(str, p)) if isinstance(p, tuple) else str(p)


def cov_k_bar(key: str) -> float:
    return 4 * max(MEASURED[k].get(key, 0.0) for k in ("cpu", "mi355x", "mi355x_pair"))


# ---- per-bin lookup ------------------------------------------------------------------------------------------------------------------
PB_LDS_EDGES = PB_LDS_BINS = 2048
PB_BLOCK_PIXELS = 256 * 4       # one workgroup and trip
PB_BLOCKS_PER_CU = 16
F32, F64 = np.float32, np.float64


def perbin_route(n_int, disjoint) -> tuple:
    """(DISJOINT, LDS, NV) of perbin_kernel for a table, as xdemhip_perbin_lookup chooses them."""
    n_var = len(n_int)
    lds = sum(n_int) <= PB_LDS_EDGES and math.prod(n_int) <= PB_LDS_BINS
    return bool(disjoint), lds, n_var if n_var <= 4 else 8


def _disjoint_ends(m: int, gaps: bool, start: float):
    """m sorted disjoint intervals [start + j, ...): every third one ends 3/8 short of the next (a gap), the others touch it.  Every
    end is a multiple of 1/8 below 2^12, exact in float32."""
    left = start + np.arange(m, dtype=np.float64)
    right = left + np.where(gaps & (np.arange(m) % 3 == 1), 0.625, 1.0)
    return left, right


def _pass_bytes(rng, n_bins: int, p):
    """1 = write, 0 = the count fails, 2 = no such row, in the proportions p = (p0, p1, p2) and in random places; at least one bin
    of kind 2 from 2 bins on, one of kind 0 from 4 bins on, and the rest -- never none -- write."""
    n2 = max(1, round(p[2] * n_bins)) if n_bins >= 2 else 0
    n0 = max(1, round(p[0] * n_bins)) if n_bins >= 4 else 0
    passb = np.ones(n_bins, dtype=np.uint8)
    where = rng.permutation(n_bins)
    passb[where[:n2]], passb[where[n2:n2 + n0]] = 2, 0
    return passb


def _values(rng, n, left, right, dtype, pad, plant):
    """n values of one variable: uniform over the intervals' hull widened by `pad` of its length on both sides; then, where n allows
    it, planted in random places: n/64 * plant values exactly on left ends and as many on right ends, n/256 * plant each below the hull,
    above it, +inf, -inf and NaN."""
    lo_, hi_ = float(left.min()), float(right.max())
    span = hi_ - lo_
    v = rng.uniform(lo_ - pad * span, hi_ + pad * span, n).astype(dtype)
    if n >= 64:
        k, q = max(1, int(n * plant) // 64), max(1, int(n * plant) // 256)
        pos = rng.permutation(n)
        v[pos[:k]] = rng.choice(left, k)
        v[pos[k:2 * k]] = rng.choice(right, k)
        at = 2 * k
        for special in (lo_ - 1.0, hi_ + 1.0, np.inf, -np.inf, np.nan):
            v[pos[at:at + q]] = special
            at += q
    return v


def _perbin_case(name, seed, dtypes, ends, n, pad, plant, p_pass, disjoint, edges=True):
    """ends: (left, right) per variable."""
    rng = np.random.default_rng(seed)
    n_int = [int(e[0].size) for e in ends]
    left, right = np.concatenate([e[0] for e in ends]), np.concatenate([e[1] for e in ends])
    n_bins = math.prod(n_int)
    return {"name": name, "n_int": n_int, "left": left, "right": right, "table": rng.normal(size=n_bins), "passb": _pass_bytes(rng, n_bins, p_pass),
            "vars": [_values(rng, n, e[0], e[1], dt, pad, plant) for dt, e in zip(dtypes, ends)], "disjoint": disjoint, "edges": edges and n >= 64}


def _disjoint_case(name, seed, dtypes, n_int, n=4099):
    """A table nd_binning could have produced.  The more variables, the less of each may fall outside (a pixel needs all of them inside
    an interval for a finite output): gaps in the first variable only from 4 variables on, hull padding and plants divided by n_var."""
    n_var = len(n_int)
    ends = [_disjoint_ends(m, n_var < 4 or k == 0, start=(-3.0, 0.0, 100.0, -40.0)[k % 4]) for k, m in enumerate(n_int)]
    return _perbin_case(name, seed, dtypes, ends, n, pad=0.1 / n_var, plant=1.0 / n_var, p_pass=(0.15, 0.7, 0.15), disjoint=True)


PERBIN_NV = {1: ((F32,), (3,)), 2: ((F32, F64), (3, 4)), 3: ((F64, F32, F64), (2, 5, 3)), 4: ((F32, F64, F32, F64), (3, 2, 4, 2)),
             5: ((F64, F32, F32, F64, F32), (2, 3, 2, 3, 2)), 8: ((F32, F64) * 4, (2,) * 8)}
PERBIN_INTERVAL_COUNTS = (1, 2, 3, 4, 5, 7, 8, 9, 2048, 2049)
# tables beyond LDS through their bins with few interval ends; the last two are there for NV = 4 and NV = 8 without LDS
PERBIN_BEYOND_LDS = {"46x45": ((F32, F64), (46, 45)), "13x13x13": ((F64, F32, F64), (13, 13, 13)), "7x7x7x7": ((F32, F64, F64, F32), (7, 7, 7, 7)),
                     "3^6x2^2": ((F32, F64) * 4, (3, 3, 3, 3, 3, 3, 2, 2))}
PERBIN_WALK_N = 1027   # pixels of the disjoint = 0 runs on those tables (the walk costs n_bins per pixel)
PERBIN_PIXEL_COUNTS = (1, 2, 3, 4, 5, 1023, 1024, 1025)
PERBIN_ALIGN_N = (4099, 4100)
PERBIN_ALIGN_VARIANTS = {"aligned": (0, 0, 0), "out": (0, 0, 1), "float32_variable": (1, 0, 0), "all": (1, 1, 1)}   # offsets of (v0, v1, out)


@functools.lru_cache(maxsize=None)
def perbin_variables_case(n_var: int):
    dtypes, n_int = PERBIN_NV[n_var]
    return _disjoint_case(f"{n_var}var", 100 + n_var, dtypes, n_int)


@functools.lru_cache(maxsize=None)
def perbin_interval_count_case(m: int):
    return _disjoint_case(f"1var_{m}", 200 + m, (F32 if m % 2 else F64,), (m,))


@functools.lru_cache(maxsize=None)
def perbin_beyond_lds_case(key: str):
    dtypes, n_int = PERBIN_BEYOND_LDS[key]
    return _disjoint_case(key, 300 + len(n_int), dtypes, n_int)


@functools.lru_cache(maxsize=None)
def perbin_pixel_count_family():
    """One two-variable table and 1025 pixels; the cases are its first n pixels.  The first five alternate inside / outside."""
    c = _disjoint_case("pixel_counts", 400, *PERBIN_NV[2], n=1025)
    c["vars"][0][:5] = (-2.5, 9.0, -1.0, np.nan, -0.5)
    c["vars"][1][:5] = (0.5, 0.5, 2.25, 1.0, 3.5)
    c["passb"][:] = 1
    c["passb"][[5, 7]] = (0, 2)
    return c


@functools.lru_cache(maxsize=None)
def perbin_alignment_case(n: int):
    """n + 1 values per variable: the tests pass the arrays from element 0 (aligned) or from element 1 (4 or 8 bytes off)."""
    return _disjoint_case(f"align_{n}", 500 + n, *PERBIN_NV[2], n=n + 1)


def prefix(case, n):
    return {**case, "vars": [v[:n] for v in case["vars"]], "edges": False}


def _iv(*pairs):
    a = np.array(pairs, dtype=np.float64)
    return a[:, 0], a[:, 1]


def _random_overlaps(rng, m):
    left = rng.integers(0, 32, m) * 0.25
    return left, left + rng.integers(2, 17, m) * 0.25


@functools.lru_cache(maxsize=None)
def perbin_overlap_case(key: str):
    """Hand-made intervals: nested, partly overlapping, unsorted (the C entry point takes them in any order with disjoint = 0)."""
    v0 = _iv((0.0, 5.0), (3.0, 8.0), (2.0, 4.0), (-1.0, 9.0), (6.0, 7.0))
    v1 = _iv((1.0, 6.0), (0.0, 2.0), (4.0, 10.0), (1.5, 1.75))
    v2 = _iv((0.0, 3.0), (2.0, 5.0), (1.0, 4.0))
    rng = np.random.default_rng(600)
    ends, dtypes, n = {"2var": ([v0, v1], (F32, F64), 4099), "3var": ([v1, v0, v2], (F64, F32, F32), 4099),
                       "3var_2197_bins": ([_random_overlaps(rng, 13) for _ in range(3)], (F32, F64, F32), PERBIN_WALK_N)}[key]
    return _perbin_case("overlap_" + key, 601 + len(key), dtypes, ends, n, pad=0.05, plant=0.5, p_pass=(0.3, 0.5, 0.2), disjoint=False)


PERBIN_OVERLAPS = ("2var", "3var", "3var_2197_bins")


def perbin_second_trip_n(num_cu: int) -> int:
    return PB_BLOCKS_PER_CU * num_cu * PB_BLOCK_PIXELS + 1027


@functools.lru_cache(maxsize=None)
def perbin_second_trip_case(num_cu: int):
    return _disjoint_case("second_trip", 700, (F32,), (7,), n=perbin_second_trip_n(num_cu))


@functools.lru_cache(maxsize=None)
def perbin_want(case_fn, *args):
    """(out, n_missing) of the oracle for a cached case, computed once."""
    c = case_fn(*args)
    return lo.perbin_tables(c["vars"], c["n_int"], c["left"], c["right"], c["table"], c["passb"])


def perbin_memberships(c):
    """Per pixel: in how many writing bins and in how many pass-2 bins it lies (the oracle's masks, counted)."""
    var = [v.astype(np.float64) for v in c["vars"]]
    off = np.cumsum([0] + c["n_int"])
    writes, misses = np.zeros(var[0].size, int), np.zeros(var[0].size, int)
    for b, combo in enumerate(itertools.product(*[range(m) for m in c["n_int"]])):
        m = np.ones(var[0].size, bool)
        for k, j in enumerate(combo):
            m &= (var[k] >= c["left"][off[k] + j]) & (var[k] < c["right"][off[k] + j])
        writes += m & (c["passb"][b] == 1)
        misses += m & (c["passb"][b] == 2)
    return writes, misses


# ---- multilinear interpolation -------------------------------------------------------------------------------------------------------
IG_LDS_VALUES = 40 * 1024 // 8      # axis and grid values together that still go to LDS
IG_AXIS_VALUES = 48 * 1024 // 8     # axis values a call may have when the grid stays in global memory
IG_MAX_GRID = 1 << 24
IG_BLOCKS_PER_CU, IG_BLOCK = 16, 256
IG_N = 1031
IG_SCALES = (1.0, 1.5, -0.0)

# node values exact in float32, except the fifth axis' (its coordinate arrays are float64)
_AXES = ([0.0, 1.0, 2.5], [-1.0, 0.5], [499998.0, 499999.5, 500000.0, 500004.0], [-7.25, -3.0, -2.875], [0.1, 0.7, 2.3, 2.4], [2.0, 4.0],
         [-8.0, -6.0, -4.0], [10.0, 10.125])
_AXES_2 = ([0.0, 1.0], [-1.0, 0.5], [500000.0, 500002.0], [-3.0, -2.875], [0.1, 0.7], [2.0, 4.0], [-8.0, -4.0], [10.0, 10.125])
_AXIS_DTYPES = (F32, F64, F32, F64, F64, F32, F64, F32)
IG_DIMS = (1, 2, 3, 4, 5, 8)


def grid_in_lds(axes) -> bool:
    return sum(len(g) for g in axes) + math.prod(len(g) for g in axes) <= IG_LDS_VALUES


def _interp_points(rng, axes, dtypes, n):
    """X (one array per dimension) and the rows that hold a NaN.  Random points reach 1.5 axis lengths beyond both ends; the first rows
    are, per axis: a point on every node; one ulp (of the coordinate's dtype) below and above the first and the last node; then one
    point on the last node of every axis at once, one on the first; then one row per axis with NaN in that coordinate alone."""
    nd = len(axes)
    X = []
    for g, dt in zip(axes, dtypes):
        span = g[-1] - g[0]
        X.append(rng.uniform(g[0] - 1.5 * span, g[-1] + 1.5 * span, n).astype(dt))
    row = 0
    for d, (g, dt) in enumerate(zip(axes, dtypes)):
        nodes = np.asarray(g, dtype=dt)
        assert np.array_equal(nodes.astype(np.float64), g)   # (the planted points are exactly on the nodes)
        near = [np.nextafter(nodes[e], dt(s)) for e in (0, -1) for s in (-np.inf, np.inf)]
        for x in list(nodes) + near:
            X[d][row] = x
            row += 1
    for d, g in enumerate(axes):
        X[d][row], X[d][row + 1] = g[-1], g[0]
    row += 2
    nan_rows = np.arange(row, row + nd)
    for d in range(nd):
        X[d][row + d] = np.nan
    assert row + nd <= n
    return X, nan_rows


def _interp_case(name, seed, axes, dtypes, n=IG_N):
    rng = np.random.default_rng(seed)
    axes = [np.asarray(g, dtype=np.float64) for g in axes]
    X, nan_rows = _interp_points(rng, axes, dtypes, n)
    V = 50.0 + 3.0 * rng.normal(size=math.prod(g.size for g in axes))
    return {"name": name, "axes": axes, "V": V, "X": X, "nan_rows": nan_rows}


@functools.lru_cache(maxsize=None)
def interp_dims_case(nd: int):
    """Axes of 2 to 4 nodes: one of exactly 2, uneven spacing, negative nodes, nodes around 5e5; the 8-D grid is 2^8."""
    axes = _AXES_2 if nd == 8 else _AXES[:nd] if nd > 1 else _AXES[4:5]
    dtypes = _AXIS_DTYPES[:nd] if nd > 1 else (F64,)
    return _interp_case(f"{nd}d", 800 + nd, axes, dtypes)


IG_STAGING = {"80x80": (80, 80), "72x71": (72, 71), "71x70": (71, 70)}


@functools.lru_cache(maxsize=None)
def interp_staging_case(key: str):
    rng = np.random.default_rng(820)
    axes = [np.cumsum(rng.integers(1, 9, m)) * 0.125 - 3.0 for m in IG_STAGING[key]]   # uneven, exact in float32
    return _interp_case(key, 821 + IG_STAGING[key][0], axes, (F32, F64))


def interp_second_trip_n(num_cu: int) -> int:
    return IG_BLOCKS_PER_CU * num_cu * IG_BLOCK + 77


@functools.lru_cache(maxsize=None)
def interp_second_trip_case(num_cu: int):
    return _interp_case("second_trip", 830, _AXES[:2], (F32, F64), n=interp_second_trip_n(num_cu))


@functools.lru_cache(maxsize=None)
def interp_want(case_fn, arg, scale):
    c = case_fn(arg)
    return lo.grid_linear(c["axes"], c["V"], c["X"], scale)


# ---- covariance double sum -----------------------------------------------------------------------------------------------------------
CV_NT, CV_CHUNK, CV_MAXM = 256, 4096, 8
SPH, EXP, GAU, CUB, STA = lo.SPHERICAL, lo.EXPONENTIAL, lo.GAUSSIAN, lo.CUBIC, lo.STABLE

COV_MODEL_SETS = {
    "spherical": [(SPH, 150.0, 1.0, 1.0)],
    "exponential": [(EXP, 200.0, 0.8, 1.0)],
    "gaussian": [(GAU, 180.0, 1.2, 1.0)],
    "cubic": [(CUB, 160.0, 0.9, 1.0)],
    "stable_0.5": [(STA, 170.0, 1.0, 0.5)],
    "stable_1.0": [(STA, 170.0, 1.0, 1.0)],
    "stable_2.0": [(STA, 170.0, 1.0, 2.0)],
    "spherical+gaussian": [(SPH, 120.0, 0.7, 1.0), (GAU, 400.0, 0.3, 1.0)],
    "eight": [(SPH, 100.0, 0.2, 1.0), (EXP, 150.0, 0.1, 1.0), (GAU, 250.0, 0.15, 1.0), (CUB, 300.0, 0.05, 1.0), (STA, 120.0, 0.1, 0.7),
              (SPH, 400.0, 0.2, 1.0), (STA, 200.0, 0.1, 1.5), (EXP, 50.0, 0.1, 1.0)],
}
# (the last is there because a swapped (ta, cb) permutes the 3 x 3 workgroups of (513, 8193) among themselves: 2 x 3 are not symmetric)
COV_SHAPES = ((1, 1), (1, 257), (255, 255), (256, 256), (257, 4095), (256, 4096), (257, 4097), (513, 8193), (257, 8193))
COV_SELF = (1, 257, 4097)
COV_MODEL_SHAPE = (300, 700)            # the shape of the model sweep: two A tiles, three B tiles, the last of both partial
COV_LATTICE_RANGES = (30.0, 50.0)       # spacing 10: pairs 30 apart along an axis, and 30 by 40 apart (a 3-4-5 triangle), are exactly on them
COV_OFFSETS = (0.0, 5e5)


def cov_key(models) -> str:
    kinds = {m[0] for m in models}
    return lo.KIND_NAMES[kinds.pop()] if len(kinds) == 1 else "mixed"


def cov_n_wg(na: int, nb: int) -> int:
    return -(-na // CV_NT) * -(-nb // CV_CHUNK)


def cov_summation_part(na, nb, T) -> float:
    """What the order of the additions can change: the longest chain a term goes through is CV_CHUNK additions in its thread, 6
    shuffles, 4 wave partials and the atomics of the n_wg workgroups, in any order -- so this also covers the run-to-run order of the
    atomics."""
    return (CV_CHUNK + 10 + cov_n_wg(na, nb)) * 2.0 ** -53 * T


def cov_bound(na, nb, ref, key) -> float:
    """The issue's bound, plus what the reference itself may be off by (0 up to lookup_oracle.COV_EXACT_PAIRS pairs)."""
    return cov_summation_part(na, nb, ref["T"]) + cov_k_bar(key) * 2.0 ** -52 * ref["A"] + ref["S_err"]


def _cov_points(rng, n, offset=0.0, signed=False):
    e = rng.normal(size=n) if signed else rng.uniform(0.5, 2.0, n)
    return [offset + rng.uniform(0.0, 500.0, n), offset + rng.uniform(0.0, 500.0, n), e]


@functools.lru_cache(maxsize=None)
def cov_shape_case(na: int, nb: int):
    """Two sets of random points (nb = 0: one set, for the self sum) whose coordinates are offset by 5e5; errors of both signs.  The
    first min(na, nb, 7) points of B coincide with A's: h = 0.  Spherical + gaussian; the self sum of 4097 points, 16.8 M pairs, takes
    the spherical model alone, whose long-double reference needs no exponential, and the block-wise reference of lookup_oracle."""
    rng = np.random.default_rng(900 + na + nb)
    a = _cov_points(rng, na, 5e5, signed=True)
    if nb == 0:
        return {"a": a, "b": None, "models": COV_MODEL_SETS["spherical" if na > 1000 else "spherical+gaussian"], "smooth_null": False}
    b = _cov_points(rng, nb, 5e5, signed=True)
    k = min(na, nb, 7)
    b[0][:k], b[1][:k] = a[0][:k], a[1][:k]
    return {"a": a, "b": b, "models": COV_MODEL_SETS["spherical+gaussian"], "smooth_null": False}


@functools.lru_cache(maxsize=None)
def cov_model_case(name: str):
    """name: a key of COV_MODEL_SETS, or "smooth_null" -- a stable model called with smooth = NULL, which stands for s = 1."""
    rng = np.random.default_rng(950)
    na, nb = COV_MODEL_SHAPE
    a, b = _cov_points(rng, na), _cov_points(rng, nb)
    b[0][:5], b[1][:5] = a[0][:5], a[1][:5]
    null = name == "smooth_null"
    return {"a": a, "b": b, "models": COV_MODEL_SETS["stable_1.0" if null else name], "smooth_null": null}


COV_MODEL_CASES = tuple(COV_MODEL_SETS) + ("smooth_null",)


@functools.lru_cache(maxsize=None)
def cov_lattice_case(kind: int, r: float, offset: float):
    """A: a 12 x 11 lattice of spacing 10; B: a 13 x 12 lattice of the same spacing shifted by (20, 30), so that points coincide; one
    model of range exactly r."""
    rng = np.random.default_rng(970 + kind)

    def lattice(nx, ny, x0, y0):
        gx, gy = np.meshgrid(np.arange(nx) * 10.0 + x0 + offset, np.arange(ny) * 10.0 + y0 + offset, indexing="ij")
        return [gx.ravel(), gy.ravel(), rng.uniform(0.5, 2.0, nx * ny)]

    return {"a": lattice(12, 11, 0.0, 0.0), "b": lattice(13, 12, 20.0, 30.0), "models": [(kind, r, 1.0, 1.5)], "smooth_null": False}


COV_PAIR_SETS = ("spherical", "exponential", "gaussian", "cubic", "stable_0.5", "stable_1.0", "stable_2.0")


@functools.lru_cache(maxsize=None)
def cov_pair_separations(name: str):
    """Distances for sums over ONE pair of unit errors, which are rho(h) itself: 0, the range and its two neighbours, half and twice
    the range, 64 distances within 1e-3 of the range below it (where the cubic model's polynomial cancels) and 192 spread over
    [0, 1.5 r]."""
    r = COV_MODEL_SETS[name][0][1]
    rng = np.random.default_rng(990)
    return np.concatenate([[0.0, r, np.nextafter(r, 0.0), np.nextafter(r, np.inf), 0.5 * r, 2.0 * r], r * (1.0 - rng.uniform(0.0, 1e-3, 64)),
                           rng.uniform(0.0, 1.5 * r, 192)])


def cov_pair_want(name: str):
    """(rho in float64 with the kernel's operations, rho in long double) at cov_pair_separations(name); h = sqrt(dx dx + 0 0)."""
    dx = cov_pair_separations(name)
    models = COV_MODEL_SETS[name]
    ldx = dx.astype(np.longdouble)
    return lo.cov_rho(models, np.sqrt(dx * dx + 0.0 * 0.0)), lo.cov_rho(models, np.sqrt(ldx * ldx))


def cov_sizes(c):
    na = c["a"][0].size
    return na, (na if c["b"] is None else c["b"][0].size)


@functools.lru_cache(maxsize=None)
def cov_want(case_fn, *args):
    c = case_fn(*args)
    return lo.cov_reference(c["a"], c["b"], c["models"])
