"""The routes of csrc/volume.hip that the fixtures' rasters are too small or too regular to reach, each on a case of
tests/volume_cases.py built for it and against the NumPy restatement (volume_oracle.OraclePlan):

  * more than one trip of the grid-stride loops: the register run of hyp_stats_kernel carried from trip to trip and flushed on a label
    change, the LDS counters of hyp_group_kernel and hyp_area_kernel filled over several trips, the scatter cursor taken again;
  * the counters in global memory: more than 4096 groups, more than 8192 area bins;
  * segments at the lengths the segment kernel is built for: on both sides of the LDS limit of 8192 values without the test switch, the
    LDS sort full, the in-place global sort and the fixed-order sum over tens of thousands of values;
  * a grouping that keeps nothing.

Integers, extremes, groups and medians compare bit for bit; a standard deviation with the exactly summed one within the derived bound
of volume_cases.std_bound.  The conditions under which each case reaches its route are asserted without a GPU by
tests/test_volume_host.py, and again here for the device's own number of compute units."""
import functools

import numpy as np
import pytest

import volume_cases as vc
import volume_oracle as vo

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def vol():
    from xdem_amd import volume

    return volume


@functools.lru_cache(maxsize=None)
def _num_cu() -> int:
    import torch

    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _want(oracle, ids, edges):
    return oracle.label_stats(), oracle.segments(ids, edges, want_std=True), oracle.groups()


@functools.lru_cache(maxsize=None)
def _trip_oracle(dtype: str, how: str):
    """(oracle plan, ids, edges, (stats, segments, groups)) of the multi-trip raster: with its labels, without any, with its mask."""
    c = vc.multi_trip_case(_num_cu(), dtype)
    extra = {"labels": {"labels": c["labels"]}, "none": {}, "mask": {"mask": c["mask"]}}[how]
    oracle = vo.OraclePlan(c["ddem"], c["ref_voids"], **extra)
    ids, edges = vc.count_edges(oracle.label_stats(), vc.TRIP_BINS)
    return oracle, extra, ids, edges, _want(oracle, ids, edges)


def _device_plan_matches(vol, ddem, ref, extra, oracle, ids, edges, want=None):
    with vol.HypsoPlan(ddem, ref, **extra) as plan:
        stats = plan.label_stats()
        segments = plan.segments(ids, edges, want_std=True)
        groups = plan.groups()
        median_only = plan.segments(ids, edges)
    want = vc.assert_plan_matches(stats, segments, groups, oracle, ids, edges, want)
    assert np.array_equal(median_only[0], segments[0]) and np.array_equal(median_only[1], segments[1], equal_nan=True) and median_only[2] is None
    return segments


@pytest.mark.parametrize("dtype", vc.DTYPES)
def test_second_and_third_trips_with_a_label_change_on_each(vol, dtype):
    """2.25 trips of every grid-stride loop; the label a trip further on is another non-zero one almost everywhere, so the register run
    of hyp_stats_kernel is flushed between trips; 70 segments of 26 to 31 thousand values: the radix selection, the in-place global
    sort and the fixed-order sum at more than a hundred terms per lane."""
    c = vc.multi_trip_case(_num_cu(), dtype)
    oracle, extra, ids, edges, want = _trip_oracle(dtype, "labels")
    figures = vc.multi_trip_conditions(c, vc.trip_pixels(_num_cu()), want[2], want[1][0])
    print(figures)
    vc.assert_multi_trip_conditions(figures)
    counts, _, _ = _device_plan_matches(vol, c["ddem"], c["ref_voids"], extra, oracle, ids, edges, want)
    assert counts.shape == (7, vc.TRIP_BINS) and counts.min() > 8192


@pytest.mark.parametrize("how", ["none", "mask"])
@pytest.mark.parametrize("dtype", vc.DTYPES)
def test_one_label_across_all_trips(vol, dtype, how):
    """Without a label map (tables of 2 entries) every whole wave of every trip joins one register run of label 1, flushed once at the
    end; under the mask the run is interrupted and taken up again."""
    c = vc.multi_trip_case(_num_cu(), dtype)
    oracle, extra, ids, edges, want = _trip_oracle(dtype, how)
    assert ids.tolist() == [1] and want[0]["pixels"][0] == (c["ddem"].size if how == "none" else np.count_nonzero(c["mask"]))
    _device_plan_matches(vol, c["ddem"], c["ref_voids"], extra, oracle, ids, edges, want)


@pytest.mark.parametrize("dtype", vc.DTYPES)
def test_public_functions_on_the_multi_trip_raster(vol, dtype):
    c = vc.multi_trip_case(_num_cu(), dtype)

    def run(v):
        out: dict = {}
        for name, (bins, kind) in (("fixed", (50.0, "fixed")), ("count", (12, "count"))):
            vc.frame_columns("bin_" + name, v.hypsometric_binning(c["ddem"], c["ref_voids"], bins=bins, kind=kind), out)
        out.update(vc.run_signal(v, c))
        return out

    with vo.patched() as ovol:
        want = run(ovol)
    vc.assert_same_bits(run(vol), want)
    assert want["signal_count"].sum() > vc.trip_pixels(_num_cu()) and np.isfinite(want["bin_fixed_value"]).sum() >= 10
    # the LDS histogram of hyp_area_kernel over several trips (timeframe 1: the model evaluated per pixel)
    flat = np.ascontiguousarray(c["ref"]).reshape(-1)
    xs = np.linspace(1000.0, 1600.0, 13)
    ys = -(xs - 1000.0) / 64.0 + (np.arange(13) % 3) / 4.0
    bins = np.linspace(990.0, 1610.0, 63)
    counts = vol._area_counts(flat, 1, xs, ys, bins)
    assert counts.dtype == np.int64 and np.array_equal(counts, vo.area_counts(flat, 1, xs, ys, bins)) and counts.sum() > 0.9 * flat.size


@pytest.mark.parametrize("noise", [False, True])
@pytest.mark.parametrize("dtype", vc.DTYPES)
def test_more_groups_than_lds_counters(vol, dtype, noise):
    """5000 groups > HYP_LDS_GROUPS = 4096: hyp_group_kernel counts in global memory, a whole wave inside one group with one atomic of 64
    (noise False: every row is two such waves), a split wave lane by lane (noise True)."""
    c = vc.many_groups_case(noise, dtype)
    oracle = vo.OraclePlan(c["ddem"], c["ref"], labels=c["labels"])
    counts, _, _ = _device_plan_matches(vol, c["ddem"], c["ref"], {"labels": c["labels"]}, oracle, c["ids"], c["edges"])
    assert counts.size == 5000 and (not noise) == (np.count_nonzero(counts) == 40 and counts.max() == 128)


@pytest.mark.parametrize("nb", [8192, 8193])
@pytest.mark.parametrize("dtype", vc.DTYPES)
def test_area_histogram_at_and_beyond_the_lds_bins(vol, dtype, nb):
    """8192 bins still count in LDS, 8193 in global memory; values on interior edges, on the last edge, outside and NaN."""
    import torch

    c = vc.area_case(nb, dtype)
    for timeframe in (0, 1, 2):
        want = vo.area_counts(c["ref"], timeframe, c["xs"], c["ys"], c["bins"])
        got = vol._area_counts(c["ref"], timeframe, c["xs"], c["ys"], c["bins"])
        assert got.dtype == want.dtype and np.array_equal(got, want), (timeframe, int(np.abs(got - want).sum()))
        assert want.sum() > 4500
    on_device = vol._area_counts(torch.from_numpy(np.array(c["ref"])).cuda(), 0, c["xs"], c["ys"], c["bins"])
    assert np.array_equal(on_device, vo.area_counts(c["ref"], 0, c["xs"], c["ys"], c["bins"]))


@pytest.mark.parametrize("dtype", vc.DTYPES)
def test_segments_of_8191_8192_and_8193_values(vol, dtype):
    """At the default limit the first two segments are sorted in LDS (the second fills it) and the third takes the radix selection and,
    for its standard deviation, the in-place global sort; with the switch at 16384 all three are sorted in LDS.  The same arrays."""
    from xdem_amd import _lib

    c = vc.threshold_case(dtype)
    ctx = _lib.default_context()
    assert ctx.options.get("hypso_seg_lds", 0) == 0
    oracle = vo.OraclePlan(c["ddem"], c["ref"])
    with vol.HypsoPlan(c["ddem"], c["ref"]) as plan:
        stats = plan.label_stats()
        default = plan.segments([1], vc.THRESHOLD_EDGES, want_std=True)
        groups = plan.groups()
        default_median_only = plan.segments([1], vc.THRESHOLD_EDGES)
        with ctx.option_scope("hypso_seg_lds", 16384):
            in_lds = plan.segments([1], vc.THRESHOLD_EDGES, want_std=True)
            in_lds_median_only = plan.segments([1], vc.THRESHOLD_EDGES)
    vc.assert_plan_matches(stats, default, groups, oracle, [1], vc.THRESHOLD_EDGES)
    assert default[0].tolist() == [list(vc.THRESHOLD_COUNTS)]
    for a, b in zip(default, in_lds):
        assert np.array_equal(a, b)
    for other in (default_median_only, in_lds_median_only):
        assert np.array_equal(other[0], default[0]) and np.array_equal(other[1], default[1]) and other[2] is None
    for b in range(3):
        v = c["ddem"][c["bin"] == b]
        assert v.dtype == np.dtype(dtype) and default[1][0, b] == np.median(v)


@pytest.mark.parametrize("dtype", vc.DTYPES)
def test_edges_that_keep_no_inlier(vol, dtype):
    """No pixel in any group: nothing is scattered and the segment kernel sees only empty segments; the plan serves the next call."""
    c = vc.case(61, 83, dtype)
    oracle = vo.OraclePlan(c["ddem"], c["ref"], labels=c["labels"])
    ids = np.array([3, 7, 1000], dtype=np.int32)
    nowhere = np.tile(np.array([5000.0, 6000.0, 7000.0, 8000.0]), (3, 1))
    edges = np.tile(np.linspace(1000.0, 1700.0, 8), (3, 1))
    with vol.HypsoPlan(c["ddem"], c["ref"], labels=c["labels"]) as plan:
        counts, med, sd = plan.segments(ids, nowhere, want_std=True)
        assert counts.shape == (3, 3) and not counts.any() and np.isnan(med).all() and np.isnan(sd).all()
        assert np.array_equal(plan.groups(), np.full(61 * 83, -1, np.int32))
        counts, med, _ = plan.segments(ids, nowhere)
        assert not counts.any() and np.isnan(med).all()
        stats = plan.label_stats()
        segments = plan.segments(ids, edges, want_std=True)
        groups = plan.groups()
    vc.assert_plan_matches(stats, segments, groups, oracle, ids, edges)
    assert segments[0].sum() > 1500 and (segments[0] == 0).any()
