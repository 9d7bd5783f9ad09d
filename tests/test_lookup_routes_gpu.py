"""The routes of xdemhip_perbin_lookup (csrc/perbin.hip, perbin_locate.h), xdemhip_interp_grid_linear (csrc/binstats.hip, grid_interp.h)
and xdemhip_cov_double_sum (csrc/covsum.hip) that table sizes, pointer alignment and n choose -- none of which the pandas front end can
steer -- through the C ABI, on the cases of tests/lookup_cases.py and against the NumPy oracles of tests/lookup_oracle.py:

  * per-bin lookup: all 20 instantiations of perbin_kernel<DISJOINT, LDS, NV>, both values of a.vec with the mixed tail, a second trip
    of the grid-stride loop; the outputs bit for bit and the count of pixels in bins without a row exactly;
  * interpolation: 1 to 8 dimensions, the grid in LDS and in global memory on both sides of the threshold, a second trip, the refusals;
    bit for bit (binstats.hip is built without contraction and grid_interp.h fixes the order of the operations);
  * covariance sum: the tile edges of the 256 x 4096 decomposition, every model branch with pairs exactly at h = 0 and h = r, within
    ``lookup_cases.cov_bound`` of the long-double sum -- a derived summation part and a measured function part (MEASURED there).

What each case is built for is asserted without a GPU by tests/test_lookup_routes_host.py.

Case against route, read off the host dispatch code (every disjoint table runs with disjoint = 1 and with disjoint = 0):

    perbin_kernel<1|0, LDS, 1>      1 variable of 1, 2, 3, 4, 5, 7, 8, 9, 2048 intervals; the second trip (disjoint = 1)
    perbin_kernel<1|0, global, 1>   2049 intervals
    perbin_kernel<1|0, LDS, 2>      2 variables 3 x 4; the pixel counts; the alignment variants
    perbin_kernel<1|0, global, 2>   46 x 45 = 2070 bins
    perbin_kernel<1|0, LDS, 3>      3 variables 2 x 5 x 3
    perbin_kernel<1|0, global, 3>   13^3 = 2197 bins
    perbin_kernel<1|0, LDS, 4>      4 variables 3 x 2 x 4 x 2
    perbin_kernel<1|0, global, 4>   7^4 = 2401 bins
    perbin_kernel<1|0, LDS, 8>      5 variables (72 bins); 8 variables (2^8 bins)
    perbin_kernel<1|0, global, 8>   8 variables, 3^6 x 2^2 = 2916 bins
    perbin_kernel<0, LDS, 2|3>      overlapping intervals, 20 and 48 bins;  <0, global, 3>: 13^3 overlapping
    a.vec = 1                       every host-memspace call and every device call but the three below (_run asserts each pointer's
                                    alignment, the output's included), so also the second trip; whole == false: the tail of 3 at
                                    n = 4099 and at the end of the second trip
    a.vec = 0                       device calls with only the output / only the float32 variable / all arrays off a 16-byte boundary
    grid_in_lds = 1                 1, 2, 3, 4, 5, 8 dimensions; 71 x 70.     grid_in_lds = 0: 80 x 80; 72 x 71
    cov_rho                         each CV_* kind alone, in sums and as single pairs, with h == r and h == 0 (both sides of
                                    ``h <= r`` and ``h < r``: the lattices, and one ulp either side of r in the single pairs);
                                    stable at s = 0.5, 1, 2 and with smooth = NULL; 2 and 8 (CV_MAXM) models"""
import ctypes
import functools

import numpy as np
import pytest

import lookup_cases as lc
import lookup_oracle as lo
from gpu_helpers import DP, _back, _dev

pytestmark = pytest.mark.gpu

EINVAL, EUNSUPPORTED = -1, -5
GUARD = -7.0   # what the output buffers hold before a call, and around the part a call may write


@pytest.fixture(scope="module")
def ctx():
    from xdem_amd import _lib

    c = _lib.Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def _num_cu() -> int:
    import torch

    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _codes(arrays):
    from xdem_amd import _lib

    return (ctypes.c_int * len(arrays))(*[_lib.F32 if a.dtype == np.float32 else _lib.F64 for a in arrays])


def _run(ctx, call, arrays, n, memspace, offsets=None):
    """call(pointers of the input arrays, pointer of the float64 output) on host arrays, or on device tensors of which array k starts
    offsets[k] elements into its (aligned) allocation; the last offset is the output's.  With offset 0 a pointer is 16-byte aligned,
    with offset 1 it is 4 or 8 bytes off: asserted for every pointer, the output's included.  The output buffer has guard elements
    on both sides and is pre-filled: returns the n values written, after checking that nothing else was."""
    from xdem_amd import _lib

    offsets = offsets or (0,) * (len(arrays) + 1)
    if memspace == _lib.HOST:
        assert not any(offsets)
        out = np.full(n + 2, GUARD)
        call([a.ctypes.data for a in arrays], out[1:].ctypes.data)
    else:
        pads = [np.concatenate([np.zeros(o, a.dtype), a]) for a, o in zip(arrays, offsets)]
        tens = [_dev(p) for p in pads]
        o_out = offsets[-1] + 2     # two guard elements (16 bytes) in front: the written part is aligned when its offset is 0
        t_out = _dev(np.full(o_out + n + 1, GUARD))
        ptrs = [t[o:].data_ptr() for t, o in zip(tens, offsets)] + [t_out[o_out:].data_ptr()]
        for p, o in zip(ptrs, offsets):
            assert o in (0, 1) and (p % 16 == 0) == (o == 0)
        call(ptrs[:-1], ptrs[-1])
        out = _back(ctx, t_out)[o_out - 1:]
        assert (_back(ctx, t_out)[:o_out] == GUARD).all()
    assert out[0] == GUARD and out[n + 1] == GUARD
    return out[1:n + 1].copy()


# ---- per-bin lookup ------------------------------------------------------------------------------------------------------------------
def _perbin(ctx, c, disjoint, memspace, offsets=None):
    from xdem_amd import _lib

    arrays = [np.ascontiguousarray(v) for v in c["vars"]]
    n, n_var = arrays[0].size, len(arrays)
    nint, dts = (ctypes.c_int * n_var)(*c["n_int"]), _codes(arrays)
    missing = ctypes.c_int64(-1)

    def call(ptrs, out):
        rc = ctx._L.xdemhip_perbin_lookup(ctx.handle, (ctypes.c_void_p * n_var)(*ptrs), dts, n_var, n, nint, c["left"].ctypes.data_as(DP),
                                          c["right"].ctypes.data_as(DP), c["table"].ctypes.data_as(DP), c["passb"].ctypes.data_as(ctypes.c_char_p),
                                          disjoint, out, ctypes.byref(missing), memspace)
        assert rc == _lib.OK

    out = _run(ctx, call, arrays, n, memspace, offsets)
    return out, missing.value


def _assert_perbin(ctx, c, want, modes, memspaces=None, offsets=None):
    from xdem_amd import _lib

    for memspace in memspaces or (_lib.HOST, _lib.DEVICE):
        for disjoint in modes:
            out, missing = _perbin(ctx, c, disjoint, memspace, offsets)
            assert np.array_equal(out, want[0], equal_nan=True), (c["name"], disjoint, memspace, int((~((out == want[0]) | (np.isnan(out) & np.isnan(want[0])))).sum()))
            assert missing == want[1], (c["name"], disjoint, memspace)


@pytest.mark.parametrize("n_var", lc.PERBIN_NV)
def test_perbin_one_to_eight_variables_both_lookups(ctx, n_var):
    """NV = 1, 2, 3, 4, 8, 8 with float32 and float64 variables in one call, tables in LDS; the search and the walk of the product agree."""
    c = lc.perbin_variables_case(n_var)
    assert lc.perbin_route(c["n_int"], 1) == (True, True, n_var if n_var <= 4 else 8)
    _assert_perbin(ctx, c, lc.perbin_want(lc.perbin_variables_case, n_var), (1, 0))


@pytest.mark.parametrize("m", lc.PERBIN_INTERVAL_COUNTS)
def test_perbin_interval_counts_around_powers_of_two(ctx, m):
    """The branch-free search of pb_locate at 1 to 9 intervals and at 2048 (the last table in LDS) and 2049 (the first in global memory):
    gaps, values on left ends (inside) and right ends (outside), below, above, infinite, NaN."""
    c = lc.perbin_interval_count_case(m)
    assert lc.perbin_route(c["n_int"], 1)[1] == (m <= 2048)
    _assert_perbin(ctx, c, lc.perbin_want(lc.perbin_interval_count_case, m), (1, 0))


@functools.lru_cache(maxsize=None)
def _walk_prefix(key):
    c = lc.prefix(lc.perbin_beyond_lds_case(key), lc.PERBIN_WALK_N)
    return c, lo.perbin_tables(c["vars"], c["n_int"], c["left"], c["right"], c["table"], c["passb"])


@pytest.mark.parametrize("key", lc.PERBIN_BEYOND_LDS)
def test_perbin_more_bins_than_lds_holds_with_few_interval_ends(ctx, key):
    """2070, 2197, 2401 and 2916 bins from 91 interval ends at the most (NV = 2, 3, 4, 8 without LDS): the search on 4099 pixels, the
    walk on the first 1027."""
    c = lc.perbin_beyond_lds_case(key)
    assert not lc.perbin_route(c["n_int"], 1)[1] and sum(c["n_int"]) <= 91
    _assert_perbin(ctx, c, lc.perbin_want(lc.perbin_beyond_lds_case, key), (1,))
    short, want = _walk_prefix(key)
    _assert_perbin(ctx, short, want, (0, 1))


@pytest.mark.parametrize("key", lc.PERBIN_OVERLAPS)
def test_perbin_overlapping_intervals_last_writer_wins(ctx, key):
    """Nested and partly overlapping intervals in unsorted order over 2 and 3 variables, pass bytes 0, 1 and 2 mixed: a pixel lies in
    several writing bins and in several bins without a row (each counts); in LDS and with 2197 bins."""
    c = lc.perbin_overlap_case(key)
    assert lc.perbin_route(c["n_int"], 0)[1] == (key != "3var_2197_bins")
    _assert_perbin(ctx, c, lc.perbin_want(lc.perbin_overlap_case, key), (0,))


@pytest.mark.parametrize("n", lc.PERBIN_PIXEL_COUNTS)
def test_perbin_pixel_counts_around_a_thread_and_a_workgroup(ctx, n):
    want = lc.perbin_want(lc.perbin_pixel_count_family)
    c = lc.prefix(lc.perbin_pixel_count_family(), n)
    short = lo.perbin_tables(c["vars"], c["n_int"], c["left"], c["right"], c["table"], c["passb"])
    assert np.array_equal(short[0], want[0][:n], equal_nan=True)
    _assert_perbin(ctx, c, short, (1, 0))


@pytest.mark.parametrize("variant", lc.PERBIN_ALIGN_VARIANTS)
@pytest.mark.parametrize("n", lc.PERBIN_ALIGN_N)
def test_perbin_alignment_of_the_callers_device_arrays(ctx, n, variant):
    """a.vec: 16-byte loads and stores need every array aligned.  The same pixels with all arrays aligned, with only the output 8 bytes
    off, with only the float32 variable 4 bytes off, and with all off; n = 4099 leaves a tail of 3 for the element-wise route inside
    a vector launch (whole == false), n = 4100 none.  The aligned host-memspace call gives the same.  (_run asserts that each
    pointer, the output's included, is on a 16-byte boundary exactly when its offset is 0: a.vec = 1 for "aligned" alone.)"""
    from xdem_amd import _lib

    c = lc.perbin_alignment_case(n)
    c = {**c, "vars": [v[1:] for v in c["vars"]]}
    want = lo.perbin_tables(c["vars"], c["n_int"], c["left"], c["right"], c["table"], c["passb"])
    assert np.isfinite(want[0]).mean() > 0.25 and want[1] > 0
    _assert_perbin(ctx, c, want, (1, 0), memspaces=(_lib.DEVICE,), offsets=lc.PERBIN_ALIGN_VARIANTS[variant])
    if variant == "aligned":
        _assert_perbin(ctx, c, want, (1, 0), memspaces=(_lib.HOST,))


def test_perbin_second_trip_of_the_grid_stride_loop(ctx):
    """n = 16 CU x 1024 + 1027 on aligned device arrays (a.vec = 1): one workgroup takes a second trip of 16-byte loads and stores in
    full, the next a partial one whose last thread goes element by element over a tail of 3."""
    from xdem_amd import _lib

    cu = _num_cu()
    c = lc.perbin_second_trip_case(cu)
    assert c["vars"][0].size == lc.perbin_second_trip_n(cu) > lc.PB_BLOCKS_PER_CU * cu * lc.PB_BLOCK_PIXELS
    want = lc.perbin_want(lc.perbin_second_trip_case, cu)
    assert np.isfinite(want[0][-1027:]).mean() > 0.25 and np.isnan(want[0][-1027:]).any()
    _assert_perbin(ctx, c, want, (1,), memspaces=(_lib.DEVICE,))


# ---- interpolation -------------------------------------------------------------------------------------------------------------------
def _interp_rc(ctx, axes, V, X, n, scale, out, memspace, ptrs):
    nd = len(axes)
    flat = np.ascontiguousarray(np.concatenate(axes), dtype=np.float64)
    n_axis = (ctypes.c_int * nd)(*[len(g) for g in axes])
    return ctx._L.xdemhip_interp_grid_linear(ctx.handle, nd, flat.ctypes.data_as(DP), n_axis, V.ctypes.data_as(DP), (ctypes.c_void_p * nd)(*ptrs),
                                             _codes(X), n, scale, ctypes.cast(out, DP), memspace)


def _interp(ctx, c, scale, memspace):
    from xdem_amd import _lib

    X = [np.ascontiguousarray(x) for x in c["X"]]

    def call(ptrs, out):
        assert _interp_rc(ctx, c["axes"], c["V"], X, X[0].size, scale, out, memspace, ptrs) == _lib.OK

    return _run(ctx, call, X, X[0].size, memspace)


def _same_bits(got, want):
    """Equal as float64 values including the sign of zero; NaN where NaN is wanted (whatever its payload)."""
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and got[~nan].tobytes() == want[~nan].tobytes()


def _assert_interp(ctx, case_fn, arg, memspaces=None, scales=lc.IG_SCALES):
    from xdem_amd import _lib

    c = case_fn(arg)
    for memspace in memspaces or (_lib.HOST, _lib.DEVICE):
        for scale in scales:
            got, want = _interp(ctx, c, scale, memspace), lc.interp_want(case_fn, arg, scale)
            assert _same_bits(got, want), (c["name"], scale, memspace, float(np.nanmax(np.abs(got - want))))


@pytest.mark.parametrize("nd", lc.IG_DIMS)
def test_interp_one_to_eight_dimensions(ctx, nd):
    """2 to 256 corners; axes of 2 to 4 nodes, uneven, negative, around 5e5; float32 and float64 coordinates in one call; points on
    every node, one ulp on either side of the end nodes, beyond both ends, NaN in each coordinate alone; scale 1, 1.5 and -0."""
    assert lc.grid_in_lds(lc.interp_dims_case(nd)["axes"])
    _assert_interp(ctx, lc.interp_dims_case, nd)


@pytest.mark.parametrize("key", lc.IG_STAGING)
def test_interp_grid_in_global_memory_and_at_the_threshold(ctx, key):
    """80 x 80: the grid read from global memory beside axes in LDS; 72 x 71: the grid alone would fit the 40 KB, with its axes it does
    not; 71 x 70: stays in LDS."""
    assert lc.grid_in_lds(lc.interp_staging_case(key)["axes"]) == (key == "71x70")
    _assert_interp(ctx, lc.interp_staging_case, key, scales=(1.5,))


def test_interp_second_trip_of_the_grid_stride_loop(ctx):
    from xdem_amd import _lib

    cu = _num_cu()
    assert lc.interp_second_trip_case(cu)["X"][0].size == lc.interp_second_trip_n(cu) > lc.IG_BLOCKS_PER_CU * cu * lc.IG_BLOCK
    _assert_interp(ctx, lc.interp_second_trip_case, cu, memspaces=(_lib.DEVICE,), scales=(1.5,))


def test_interp_refusals_leave_the_context_usable(ctx):
    """Return codes only: no kernel runs for the refused calls."""
    from xdem_amd import _lib

    x = [np.zeros(4, np.float32), np.zeros(4)]
    out = np.full(4, GUARD)

    def rc(sizes):
        axes = [np.arange(m, dtype=np.float64) for m in sizes]
        return _interp_rc(ctx, axes, np.zeros(int(np.prod(sizes))), x, 4, 1.0, out.ctypes.data, _lib.HOST, [v.ctypes.data for v in x])

    assert rc((3100, 3100)) == EUNSUPPORTED      # 6200 axis values: more than 48 KB of LDS beside a grid in global memory
    assert rc((4097, 4097)) == EUNSUPPORTED      # more than 2^24 grid values
    assert rc((1, 5)) == EINVAL and rc((5, 1)) == EINVAL
    assert (out == GUARD).all()
    assert rc((3, 4)) == _lib.OK and (out == 0.0).all()


# ---- covariance double sum -----------------------------------------------------------------------------------------------------------
def _cov_rc(ctx, pa, na, pb, nb, models, smooth_null, memspace, out):
    nm = len(models)
    types = (ctypes.c_int * max(nm, 1))(*[m[0] for m in models])
    ranges, psills, smooth = (np.array([m[i] for m in models] + [0.0] * (nm == 0), dtype=np.float64) for i in (1, 2, 3))
    pa = [ctypes.cast(p, DP) for p in pa]
    pb = [None] * 3 if pb is None else [ctypes.cast(p, DP) for p in pb]
    return ctx._L.xdemhip_cov_double_sum(ctx.handle, pa[0], pa[1], pa[2], na, pb[0], pb[1], pb[2], nb, nm, types, ranges.ctypes.data_as(DP),
                                         psills.ctypes.data_as(DP), None if smooth_null else smooth.ctypes.data_as(DP), ctypes.byref(out), memspace)


def _cov(ctx, c, memspace, b="own"):
    """The device's sum for a case; b: "own" -- the case's second set (None: the self route), "a" -- the first set passed twice."""
    from xdem_amd import _lib

    a = [np.ascontiguousarray(v) for v in c["a"]]
    second = a if b == "a" else None if c["b"] is None else [np.ascontiguousarray(v) for v in c["b"]]
    if memspace == _lib.HOST:
        pa, pb = [v.ctypes.data for v in a], (None if second is None else [v.ctypes.data for v in second])
    else:
        keep = [_dev(v) for v in a], (None if second is None else [_dev(v) for v in second])
        pa, pb = [t.data_ptr() for t in keep[0]], (None if keep[1] is None else [t.data_ptr() for t in keep[1]])
    out = ctypes.c_double(np.nan)
    rc = _cov_rc(ctx, pa, a[0].size, pb, 0 if second is None else second[0].size, c["models"], c["smooth_null"], memspace, out)
    assert rc == _lib.OK
    ctx.synchronize()
    return out.value


def _assert_cov(ctx, case_fn, *args):
    from xdem_amd import _lib

    c, ref = case_fn(*args), lc.cov_want(case_fn, *args)
    na, nb = lc.cov_sizes(c)
    key = lc.cov_key(c["models"])
    part, unit = lc.cov_summation_part(na, nb, ref["T"]), 2.0 ** -52 * ref["A"]
    for memspace in (_lib.HOST, _lib.DEVICE):
        got = _cov(ctx, c, memspace)
        err = abs(got - ref["S_ref"])
        print(f"K {key} {case_fn.__name__}{args} memspace {memspace}: |S_dev - S_ref| = {err:.3e}, summation part {part:.3e}, "
              f"K_dev = {max(0.0, err - part) / unit:.3f}, whole = {err / unit:.4f}, bound {lc.cov_bound(na, nb, ref, key):.3e}")
        assert err <= lc.cov_bound(na, nb, ref, key)


@pytest.mark.parametrize("shape", lc.COV_SHAPES, ids=lc.case_id)
def test_cov_two_sets_at_the_tile_edges(ctx, shape):
    """One point; one short of, exactly, and one past the 256 A points of a workgroup, its 4096-point chunk of B and the 256-point
    LDS tiles; (513, 8193): 3 A tiles x 3 chunks, where a swapped (ta, cb) reads other points.  Spherical + gaussian, coordinates
    around 5e5, errors of both signs, coincident points."""
    _assert_cov(ctx, lc.cov_shape_case, *shape)


@pytest.mark.parametrize("na", lc.COV_SELF)
def test_cov_self_sum_and_the_same_set_passed_twice(ctx, na):
    """S(A, A) by the self route (bx = NULL) and with A passed as both sets: the same terms, so the two differ by no more than the
    order of the additions allows."""
    from xdem_amd import _lib

    _assert_cov(ctx, lc.cov_shape_case, na, 0)
    c, ref = lc.cov_shape_case(na, 0), lc.cov_want(lc.cov_shape_case, na, 0)
    for memspace in (_lib.HOST, _lib.DEVICE):
        own, twice = _cov(ctx, c, memspace), _cov(ctx, c, memspace, b="a")
        print(f"self {na} memspace {memspace}: |S_self - S_twice| = {abs(own - twice):.3e}, summation part {lc.cov_summation_part(na, na, ref['T']):.3e}")
        assert abs(own - twice) <= lc.cov_summation_part(na, na, ref["T"])


@pytest.mark.parametrize("name", lc.COV_MODEL_CASES)
def test_cov_every_model_kind(ctx, name):
    """Each kind alone, stable at s = 0.5, 1 and 2, spherical + gaussian, eight models with every kind among them, smooth = NULL."""
    _assert_cov(ctx, lc.cov_model_case, name)


@pytest.mark.parametrize("offset", lc.COV_OFFSETS)
@pytest.mark.parametrize("r", lc.COV_LATTICE_RANGES)
@pytest.mark.parametrize("kind", range(5), ids=lo.KIND_NAMES)
def test_cov_lattice_pairs_exactly_at_zero_and_at_the_range(ctx, kind, r, offset):
    """Lattices of spacing 10 and a range of exactly 30 or 50: hundreds of pairs sit on h == r (``h <= r`` of the spherical model,
    ``h < r`` of the cubic one) and 80 on h == 0 (``pow(0, s)`` of the stable one)."""
    _assert_cov(ctx, lc.cov_lattice_case, kind, r, offset)


@pytest.mark.parametrize("name", lc.COV_PAIR_SETS)
def test_cov_single_pairs_are_rho_itself(ctx, name):
    """na = nb = 1 with unit errors: the sum is ``1 * (1 * rho(h))`` with nothing added, so the device's rho is seen directly, at h = 0,
    h = r, one ulp on either side of r, near r and across the range.  The spherical and cubic models are +, -, *, / and a correctly
    rounded sqrt without contraction: the device's value equals NumPy's bit for bit.  The others go through ocml's exp and pow: within
    the bar K of the long-double value (their figures are printed: MEASURED["mi355x_pair"])."""
    from xdem_amd import _lib

    dx = lc.cov_pair_separations(name)
    rho64, rho_ld = lc.cov_pair_want(name)
    models = lc.COV_MODEL_SETS[name]
    key = lc.cov_key(models)
    zero, one, x, out = np.zeros(1), np.ones(1), np.zeros(1), ctypes.c_double(np.nan)
    got = np.empty(dx.size)
    for i, h in enumerate(dx):
        x[0] = h
        rc = _cov_rc(ctx, [zero.ctypes.data, zero.ctypes.data, one.ctypes.data], 1, [x.ctypes.data, zero.ctypes.data, one.ctypes.data], 1, models, False,
                     _lib.HOST, out)
        assert rc == _lib.OK
        got[i] = out.value
    assert got[0] == 1.0   # h = 0: every model gives gamma = 0, also through pow(0, s)
    k_dev = float(np.abs(got.astype(np.longdouble) - rho_ld).max()) / 2.0 ** -52
    k_cpu = float(np.abs(rho64.astype(np.longdouble) - rho_ld).max()) / 2.0 ** -52
    print(f"K pair {key} {name}: device {k_dev:.3f}, NumPy {k_cpu:.3f}, device values that differ from NumPy's: {np.count_nonzero(got != rho64)} of {dx.size}")
    if key in ("spherical", "cubic"):
        assert got.tobytes() == rho64.tobytes()
    assert k_dev <= lc.cov_k_bar(key)


def test_cov_refusals_leave_the_context_usable(ctx):
    from xdem_amd import _lib

    c = lc.cov_model_case("spherical")
    a = [np.ascontiguousarray(v) for v in c["a"]]
    pa = [v.ctypes.data for v in a]
    out = ctypes.c_double(GUARD)

    def rc(models):
        return _cov_rc(ctx, pa, a[0].size, None, 0, models, False, _lib.HOST, out)

    ok = (lc.SPH, 100.0, 1.0, 1.0)
    assert rc([]) == EINVAL and rc([ok] * 9) == EINVAL
    assert rc([(lc.SPH, 0.0, 1.0, 1.0)]) == EINVAL and rc([(lc.SPH, -5.0, 1.0, 1.0)]) == EINVAL
    assert rc([(lc.GAU, 100.0, 0.0, 1.0)]) == EINVAL and rc([ok, (lc.EXP, 100.0, -1.0, 1.0)]) == EINVAL
    assert rc([(lc.STA, 100.0, 1.0, 0.0)]) == EINVAL and rc([(lc.STA, 100.0, 1.0, -1.0)]) == EINVAL
    assert rc([(5, 100.0, 1.0, 1.0)]) == EUNSUPPORTED
    assert out.value == GUARD
    assert rc([ok] * 8) == _lib.OK and out.value > 0.0
