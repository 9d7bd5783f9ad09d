"""Without a GPU: the oracles of tests/lookup_oracle.py against independent references, and what the cases of tests/lookup_cases.py
are built for, asserted on the oracles alone -- so that no case of tests/test_lookup_routes_gpu.py can pass by returning NaN
everywhere, by never meeting an interval end, or by summing pairs that all lie beyond the range.

  * per-bin lookup: the oracle on the tables the product's ``_perbin_tables`` makes equals the reference's recorded outputs;
  * interpolation: the oracle equals SciPy's RegularGridInterpolator bit for bit except in 2-D, where SciPy's compiled fast path
    orders the operations differently: there within the bound B of lookup_oracle.grid_linear;
  * covariance sum: the float64 terms stay within the recorded per-pair figures of the long-double evaluation."""
import itertools

import numpy as np
import pandas as pd
import pytest

import lookup_cases as lc
import lookup_oracle as lo
from test_oracle_conv_golden import PERBIN_RUNS, Z, perbin_frame, perbin_vars

CU = 256   # compute units of an MI355X: the second-trip cases are built for the device at hand, checked here for this count


# ---- per-bin lookup ------------------------------------------------------------------------------------------------------------------
def _oracle_on_product_tables(df, list_var, names, stat, min_count):
    from xdem_amd import spatialstats as ss

    names = [names] if isinstance(names, str) else names
    arrays = [np.ascontiguousarray(v) for v in list_var]
    arrays = [(a if a.dtype in (np.float32, np.float64) else a.astype(np.float64)).reshape(-1) for a in arrays]
    counts, left, right, table, decided, disjoint, _ = ss._perbin_tables(df, [a.dtype for a in arrays], names, stat, min_count)
    out, n_missing = lo.perbin_tables(arrays, counts, left, right, table, decided)
    return out.reshape(np.shape(list_var[0])), n_missing, disjoint


@pytest.mark.parametrize("key", sorted(PERBIN_RUNS))
def test_perbin_oracle_on_the_products_tables_equals_the_reference(key):
    d, vkeys, names, stat, mc = PERBIN_RUNS[key]
    out, n_missing, disjoint = _oracle_on_product_tables(perbin_frame(d), perbin_vars(vkeys), names, stat, mc)
    assert np.array_equal(out, Z[f"perbin|{key}|out"], equal_nan=True)
    assert n_missing == 0 and disjoint


def test_perbin_oracle_on_the_overlap_frame_equals_the_reference():
    hand = pd.DataFrame({"x": [pd.Interval(0.0, 5.0, closed="left"), pd.Interval(3.0, 8.0, closed="left"), pd.Interval(2.0, 4.0, closed="left")],
                         "count": [10.0, 1.0, 7.0], "val": [1.5, 2.5, 3.5]})
    for mc in (0, 5):
        out, n_missing, disjoint = _oracle_on_product_tables(hand, [Z["perbin|overlap|x"]], ["x"], "val", mc)
        assert np.array_equal(out, Z[f"perbin|overlap|out_min{mc}"], equal_nan=True)
        assert n_missing == 0 and not disjoint


def _perbin_cases():
    yield from ((lc.perbin_variables_case, (v,)) for v in lc.PERBIN_NV)
    yield from ((lc.perbin_interval_count_case, (m,)) for m in lc.PERBIN_INTERVAL_COUNTS)
    yield from ((lc.perbin_beyond_lds_case, (k,)) for k in lc.PERBIN_BEYOND_LDS)
    yield from ((lc.perbin_overlap_case, (k,)) for k in lc.PERBIN_OVERLAPS)
    yield from ((lc.perbin_alignment_case, (n,)) for n in lc.PERBIN_ALIGN_N)
    yield (lc.perbin_pixel_count_family, ())
    yield (lc.perbin_second_trip_case, (CU,))


def _assert_perbin_conditions(c, out, n_missing):
    """At least 25 % finite and 5 % NaN outputs; pass-2 bins are met; pixels exactly on a left end (inside) and on a right end."""
    assert np.isfinite(out).mean() >= 0.25 and np.isnan(out).mean() >= 0.05, (c["name"], np.isfinite(out).mean())
    if (c["passb"] == 2).any():
        assert n_missing > 0, c["name"]
    if c["edges"]:
        off = np.cumsum([0] + c["n_int"])
        assert any(np.isin(v.astype(np.float64), c["left"][off[k]:off[k + 1]]).any() for k, v in enumerate(c["vars"])), c["name"]
        assert any(np.isin(v.astype(np.float64), c["right"][off[k]:off[k + 1]]).any() for k, v in enumerate(c["vars"])), c["name"]
        assert all(np.isnan(v).any() and np.isposinf(v).any() and np.isneginf(v).any() for v in c["vars"]), c["name"]


@pytest.mark.parametrize("case_fn, args", list(_perbin_cases()), ids=lc.case_id)
def test_perbin_cases_meet_their_conditions(case_fn, args):
    c = case_fn(*args)
    assert c["edges"]
    out, n_missing = lc.perbin_want(case_fn, *args)
    _assert_perbin_conditions(c, out, n_missing)
    if c["disjoint"]:   # what the disjoint route relies on: sorted, not overlapping, per variable
        off = np.cumsum([0] + c["n_int"])
        for k in range(len(c["n_int"])):
            le, ri = c["left"][off[k]:off[k + 1]], c["right"][off[k]:off[k + 1]]
            assert (le < ri).all() and (ri[:-1] <= le[1:]).all()
            if k == 0 and le.size >= 3:
                assert (ri[:-1] < le[1:]).any() and (ri[:-1] == le[1:]).any()   # a gap, and two intervals that touch


def test_perbin_walk_prefixes_and_pixel_counts_meet_their_conditions():
    """The disjoint = 0 runs on the tables beyond LDS use the first 1027 pixels: the same fractions hold there.  The pixel-count cases
    are the first n pixels of one family: the fractions cannot hold at n < 20 (5 % of them is less than a pixel); there a finite and a
    NaN output from n = 2 on, both kinds from n = 1023 on."""
    for key in lc.PERBIN_BEYOND_LDS:
        c = lc.prefix(lc.perbin_beyond_lds_case(key), lc.PERBIN_WALK_N)
        _assert_perbin_conditions(c, *lo.perbin_tables(c["vars"], c["n_int"], c["left"], c["right"], c["table"], c["passb"]))
    out, _ = lc.perbin_want(lc.perbin_pixel_count_family)
    for n in lc.PERBIN_PIXEL_COUNTS:
        assert np.isfinite(out[0]) and (n < 2 or (np.isnan(out[:n]).any() and np.isfinite(out[:n]).any()))
        if n >= 1023:
            c = lc.prefix(lc.perbin_pixel_count_family(), n)
            _assert_perbin_conditions(c, *lo.perbin_tables(c["vars"], c["n_int"], c["left"], c["right"], c["table"], c["passb"]))


@pytest.mark.parametrize("key", lc.PERBIN_OVERLAPS)
def test_perbin_overlap_cases_have_pixels_in_several_bins_of_each_kind(key):
    c = lc.perbin_overlap_case(key)
    writes, misses = lc.perbin_memberships(c)
    assert (writes >= 2).mean() > 0.1 and (misses >= 2).mean() > 0.02 and ((writes >= 1) & (misses >= 1)).mean() > 0.1
    off = np.cumsum([0] + c["n_int"])
    nested = False
    for k in range(len(c["n_int"])):
        le, ri = c["left"][off[k]:off[k + 1]], c["right"][off[k]:off[k + 1]]
        assert (np.diff(le) < 0).any()                                                                           # unsorted
        assert ((le[:, None] < le[None, :]) & (le[None, :] < ri[:, None]) & (ri[:, None] < ri[None, :])).any()   # partly overlapping
        nested |= bool(((le[:, None] < le[None, :]) & (ri[None, :] < ri[:, None])).any())
    assert nested


def test_perbin_cases_reach_all_twenty_instantiations():
    """perbin_kernel<DISJOINT, LDS, NV>, read off the host dispatch (lookup_cases.perbin_route); every disjoint table runs both ways."""
    tables = [lc.perbin_variables_case(v)["n_int"] for v in lc.PERBIN_NV] + [[m] for m in lc.PERBIN_INTERVAL_COUNTS]
    tables += [list(t[1]) for t in lc.PERBIN_BEYOND_LDS.values()]
    seen = {lc.perbin_route(t, d) for t in tables for d in (0, 1)}
    assert seen == set(itertools.product((False, True), (False, True), (1, 2, 3, 4, 8)))
    assert {lc.perbin_route(lc.perbin_overlap_case(k)["n_int"], 0) for k in lc.PERBIN_OVERLAPS} == {(False, True, 2), (False, True, 3), (False, False, 3)}
    assert lc.perbin_route([2048], 1)[1] and not lc.perbin_route([2049], 1)[1]
    n = lc.perbin_second_trip_n(CU)
    assert lc.PB_BLOCKS_PER_CU * CU * lc.PB_BLOCK_PIXELS < n and n % 4 == 3   # a second trip of one workgroup and a bit, a tail of 3


# ---- interpolation -------------------------------------------------------------------------------------------------------------------
def _interp_cases():
    yield from ((lc.interp_dims_case, nd) for nd in lc.IG_DIMS)
    yield from ((lc.interp_staging_case, k) for k in lc.IG_STAGING)
    yield (lc.interp_second_trip_case, CU)


@pytest.mark.parametrize("case_fn, arg", list(_interp_cases()), ids=lc.case_id)
def test_interp_oracle_equals_scipy_and_the_cases_meet_their_conditions(case_fn, arg):
    from scipy.interpolate import RegularGridInterpolator

    c = case_fn(arg)
    nd = len(c["axes"])
    pts = np.stack([x.astype(np.float64) for x in c["X"]], axis=1)
    ref = RegularGridInterpolator(tuple(c["axes"]), c["V"].reshape([g.size for g in c["axes"]]), method="linear", bounds_error=False, fill_value=None)(pts)
    for scale in lc.IG_SCALES:
        got, bound = lo.grid_linear(c["axes"], c["V"], c["X"], scale, with_bound=True)
        assert np.array_equal(got, lc.interp_want(case_fn, arg, scale), equal_nan=True)
        want = np.float64(scale) * ref
        assert np.array_equal(np.isnan(got), np.isnan(want))
        ok = ~np.isnan(got)
        if nd != 2:
            assert np.array_equal(got[ok], want[ok]) and np.array_equal(np.signbit(got[ok]), np.signbit(want[ok]))
        else:
            diff = np.abs(got[ok] - want[ok])
            print(f"{c['name']} scale {scale}: largest |oracle - scipy| / B = {float((diff[diff > 0] / bound[ok][diff > 0]).max(initial=0.0)):.3f}")
            assert (diff <= bound[ok]).all()
    # conditions, on the oracle alone
    out = lc.interp_want(case_fn, arg, 1.0)
    nan_in = np.zeros(out.size, bool)
    for d, (g, x) in enumerate(zip(c["axes"], c["X"])):
        x64 = x.astype(np.float64)
        assert (x64 < g[0]).any() and (x64 > g[-1]).any()                      # extrapolated below and above
        assert all((x64 == node).any() for node in g)                           # exactly on every node
        assert (x64 == np.nextafter(x.dtype.type(g[-1]), x.dtype.type(-np.inf))).any()
        assert np.isnan(x[c["nan_rows"][d]]) and sum(np.isnan(xx[c["nan_rows"][d]]) for xx in c["X"]) == 1   # NaN in this coordinate alone
        nan_in |= np.isnan(x)
    assert (np.stack([x.astype(np.float64) == g[-1] for g, x in zip(c["axes"], c["X"])]).all(axis=0)).any()   # on the last node of every axis
    assert nan_in.sum() == nd and np.isnan(out[nan_in]).all()
    assert np.isfinite(out[~nan_in]).mean() >= 0.9


def test_interp_cases_reach_both_stagings_and_the_refusals():
    """grid_in_lds as xdemhip_interp_grid_linear decides it: axes and grid values together within 40 KB."""
    assert all(lc.grid_in_lds(lc.interp_dims_case(nd)["axes"]) for nd in lc.IG_DIMS)
    assert [lc.grid_in_lds(lc.interp_staging_case(k)["axes"]) for k in ("80x80", "72x71", "71x70")] == [False, False, True]
    assert 72 * 71 <= lc.IG_LDS_VALUES < 72 * 71 + 143          # the grid alone would fit: the threshold counts the axes
    assert 3100 + 3100 > lc.IG_AXIS_VALUES and 3100 * 3100 <= lc.IG_MAX_GRID < 4097 * 4097
    assert [len(g) for g in lc.interp_dims_case(8)["axes"]] == [2] * 8
    n = lc.interp_second_trip_n(CU)
    assert n > lc.IG_BLOCKS_PER_CU * CU * lc.IG_BLOCK


# ---- covariance double sum -----------------------------------------------------------------------------------------------------------
def _cov_cases():
    yield from ((lc.cov_shape_case, s) for s in lc.COV_SHAPES)
    yield from ((lc.cov_shape_case, (na, 0)) for na in lc.COV_SELF)
    yield from ((lc.cov_model_case, (name,)) for name in lc.COV_MODEL_CASES)
    yield from ((lc.cov_lattice_case, (kind, r, off)) for kind in range(5) for r in lc.COV_LATTICE_RANGES for off in lc.COV_OFFSETS)


@pytest.mark.parametrize("case_fn, args", list(_cov_cases()), ids=lc.case_id)
def test_cov_oracle_stays_within_the_cpu_figures_and_the_cases_meet_their_conditions(case_fn, args):
    c, ref = case_fn(*args), lc.cov_want(case_fn, *args)
    key = lc.cov_key(c["models"])
    print(f"{case_fn.__name__}{args} [{key}]: k_pair = {ref['k_pair']:.3f}, |S64 - S_ref| / (2^-52 A) = {abs(ref['S64'] - ref['S_ref']) / (2.0 ** -52 * ref['A']):.3f}, "
          f"T / A = {ref['T'] / ref['A']:.4f}, pairs at h = 0: {ref['h_zero']}, at h = r: {ref['h_on_range']}")
    assert ref["k_pair"] <= lc.MEASURED["cpu"][key]
    # every float64 term is off by at most k_pair 2^-52 |e_i e_j| through rho and by two roundings of 2^-53 |term| through its products
    assert abs(ref["S64"] - ref["S_ref"]) <= lc.MEASURED["cpu"][key] * 2.0 ** -52 * ref["A"] + 2.0 ** -52 * ref["T"] + 2 * ref["S_err"]
    assert (ref["S_err"] == 0.0) == (np.prod(lc.cov_sizes(c)) <= lo.COV_EXACT_PAIRS) and ref["S_err"] <= 0.2 * lc.cov_summation_part(*lc.cov_sizes(c), ref["T"])
    assert ref["T"] / ref["A"] >= 0.01
    na, nb = lc.cov_sizes(c)
    if case_fn is lc.cov_lattice_case:
        assert ref["h_on_range"] > 0 and ref["h_zero"] > 0
    elif min(na, nb) > 1 or c["b"] is None:
        assert ref["h_zero"] > 0


@pytest.mark.parametrize("name", lc.COV_PAIR_SETS)
def test_cov_single_pair_separations_meet_their_conditions(name):
    """The distances of the one-pair sums hold 0, the range, its two neighbours and both sides; rho there stays within the CPU figure."""
    dx, r = lc.cov_pair_separations(name), lc.COV_MODEL_SETS[name][0][1]
    rho64, rho_ld = lc.cov_pair_want(name)
    assert dx[0] == 0.0 and dx[1] == r and dx[2] < r < dx[3] and dx[3] - dx[2] < 1e-13 * r and (dx > 1.2 * r).any() and (dx < 0.2 * r).any()
    assert rho64[0] == 1.0 and np.isfinite(rho64).all() and np.unique(rho64).size > 150
    assert float(np.abs(rho64.astype(np.longdouble) - rho_ld).max()) / 2.0 ** -52 <= lc.MEASURED["cpu"][lc.cov_key(lc.COV_MODEL_SETS[name])]


def test_cov_cases_reach_the_tile_edges_and_every_model():
    assert {lc.cov_n_wg(*s) for s in lc.COV_SHAPES} == {1, 2, 4, 6, 9} and lc.cov_n_wg(513, 8193) == 9 and lc.cov_n_wg(257, 8193) == 6
    assert lc.cov_n_wg(256, 4096) == 1 and lc.cov_n_wg(257, 4097) == 4
    assert len(lc.COV_MODEL_SETS["eight"]) == lc.CV_MAXM and {m[0] for m in lc.COV_MODEL_SETS["eight"]} == set(range(5))
    assert {m[3] for k, v in lc.COV_MODEL_SETS.items() if k.startswith("stable") for m in v} == {0.5, 1.0, 2.0}
    assert set(lc.MEASURED["cpu"]) == set(lc.MEASURED["mi355x"]) == set(lo.KIND_NAMES) | {"mixed"}
