"""xdem_amd.volume without a GPU: the NumPy restatement of the device's work (volume_oracle.py) under the module's own host code
against every fixture recorded from the reference (tools/gen_golden_volume.py), the signatures, and the errors and warnings of
the functions that need no device."""
import inspect
import json
import os
import warnings

import numpy as np
import pytest

import volume_cases as vc
import volume_oracle as vo

CASES = [(H, W, dt) for (H, W) in vc.SHAPES for dt in vc.DTYPES] + [(61, 83, dt) for dt in vc.MIXED]


@pytest.fixture(scope="module")
def errors():
    with open(os.path.join(vc.GOLDEN, "volume_errors.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("H,W,dtype", CASES)
def test_restatement_matches_every_fixture(H, W, dtype):
    c, g = vc.case(H, W, dtype), vc.golden(H, W, dtype)
    with vo.patched() as vol:
        got = vc.run_binning(vol, c)
        got.update(vc.run_tables(vol, vc.fixed_frame(g)))
        got.update(vc.run_area(vol, c, g))
        got.update(vc.run_hypso_interp(vol, c))
        got.update(vc.run_signal(vol, c))
        regional = vc.run_regional(vol, c, g)
    vc.assert_same_bits(got, g)
    assert set(got) | set(regional) == set(g), "a recorded entry is not compared"
    std_dev, model_dev = vc.regional_deviations(regional, g, c)
    std_bar, model_bar = vc.regional_bars(dtype, g)
    print(f"{dtype}: std deviation {std_dev:.3e}, model deviation {model_dev:.3e}")
    assert std_dev <= std_bar and model_dev <= model_bar, (std_dev, model_dev)


def test_rotation_by_one_is_reproduced():
    """volume.py:115-116 stores bin i's statistic at row i - 1: with a dDEM that falls with elevation the LAST row carries the lowest
    bin's (largest) median."""
    g = vc.golden(61, 83, "float32")
    v = g["bin_fixed_value"]
    assert v[-1] > v[0] > v[-2]


def test_signatures_match_the_reference():
    from xdem_amd import volume

    with open(os.path.join(vc.GOLDEN, "signatures_volume.json")) as f:
        recorded = json.load(f)
    assert len(recorded) == 7
    for name, params in recorded.items():
        sig = inspect.signature(getattr(volume, name))
        assert [p["name"] for p in params] == list(sig.parameters), name
        for p in params:
            q = sig.parameters[p["name"]]
            assert q.kind.name == p["kind"], (name, p["name"])
            if p["default"] == "<required>":
                assert q.default is inspect.Parameter.empty, (name, p["name"])
            else:
                d = q.default
                assert (d if d is None or isinstance(d, (bool, int, float, str)) else getattr(d, "__name__", repr(d))) == p["default"], (name, p["name"])
    for absent in ("idw_interpolation", "local_hypsometric_interpolation"):
        assert not hasattr(volume, absent)


def _raised(fn):
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        try:
            fn()
            out = {"type": None, "message": None}
        except BaseException as e:   # noqa: BLE001 (assertions included)
            out = {"type": type(e).__name__, "message": str(e)}
    out["warnings"] = [[w.category.__name__, str(w.message)] for w in caught if issubclass(w.category, UserWarning)]
    return out


def test_errors_and_warnings_match_the_reference(errors):
    c = vc.case(61, 83, "float32")
    ddem, ref, labels = c["ddem"], c["ref"], c["labels"]
    with vo.patched() as vol:
        fixed = vol.hypsometric_binning(ddem, ref)
        got = {
            "shape_mismatch": _raised(lambda: vol.hypsometric_binning(ddem[:, :-1], ref)),
            "invalid_kind": _raised(lambda: vol.hypsometric_binning(ddem, ref, kind="nope")),
            "invalid_timeframe": _raised(lambda: vol.calculate_hypsometry_area(fixed, ref, 30.0, timeframe="nope")),
            "area_ref_nans": _raised(lambda: vol.calculate_hypsometry_area(fixed, c["ref_voids"], 30.0)),
            "area_bins_nans": _raised(lambda: vol.calculate_hypsometry_area(fixed, ref, 30.0, timeframe="mean")),
            "signal_ref_voids": _raised(lambda: vol.get_regional_hypsometric_signal(ddem, c["ref_voids"], labels)),
            "regional_ref_voids": _raised(lambda: vol.norm_regional_hypsometric_interpolation(ddem, c["ref_voids"], labels)),
            "interp_too_few_bins": _raised(lambda: vol.interpolate_hypsometric_bins(fixed.iloc[:3])),
            "hypso_interp_empty_mask": _raised(lambda: vol.hypsometric_interpolation(ddem, ref, np.zeros(ddem.shape, dtype=bool))),
        }
    assert got == errors


def test_labels_outside_the_limit_are_refused_before_any_device_work():
    from xdem_amd import volume

    lab = np.zeros(16, np.int64)
    for value in (1 << 20, -1, 1 << 40):
        lab[3] = value
        with pytest.raises(ValueError, match=r"\[0, 2\^20"):
            volume._labels_plane(lab, np.zeros(16, np.float32))
    with pytest.raises(ValueError, match="integers"):
        volume._labels_plane(np.array([0.0, 1.5]), np.zeros(2, np.float32))
    assert volume._labels_plane(np.array([0.0, 7.0]), np.zeros(2, np.float32)).dtype == np.int32


# ---- the conditions under which the cases of tests/test_volume_routes_gpu.py reach their routes, from the inputs and the oracle alone ----
@pytest.mark.parametrize("dtype", vc.DTYPES)
@pytest.mark.parametrize("num_cu", [256])
def test_multi_trip_case_makes_every_thread_change_label_between_trips(num_cu, dtype):
    """With 256 compute units a trip is 1,048,576 pixels = 512 rows = 64 label bands, 64 = 1 (mod 7): the label 512 rows on is the next of
    the cycle, so a wave's register run of hyp_stats_kernel is flushed on a change between two non-zero labels on every trip."""
    c = vc.multi_trip_case(num_cu, dtype)
    n_trip = vc.trip_pixels(num_cu)
    assert c["ddem"].shape == (-(-9 * n_trip // (4 * 2048)), 2048) == (1152, 2048)
    oracle = vo.OraclePlan(c["ddem"], c["ref_voids"], labels=c["labels"])
    st = oracle.label_stats()
    ids, edges = vc.count_edges(st, vc.TRIP_BINS)
    assert st["ref_invalid"] > 0 and ids.tolist() == sorted(vc.TRIP_IDS)
    counts, _, _ = oracle.segments(ids, edges)
    figures = vc.multi_trip_conditions(c, n_trip, oracle.groups(), counts)
    print(figures)
    vc.assert_multi_trip_conditions(figures)
    assert figures["label_changes"] > 0.99 and figures["empty_segments"] == 0 and counts.shape == (7, 10)
    # without labels: one run of label 1 across all trips; the mask: runs that end and begin again
    assert np.count_nonzero(c["mask"]) > n_trip // 2 and not c["mask"].all()
    assert np.isfinite(c["ref"]).all()


@pytest.mark.parametrize("dtype", vc.DTYPES)
def test_many_groups_case_leaves_the_lds_counters(dtype):
    for noise in (False, True):
        c = vc.many_groups_case(noise, dtype)
        assert c["edges"].shape == (5, 1001) and c["edges"].shape[0] * (c["edges"].shape[1] - 1) > 4096   # HYP_LDS_GROUPS
        oracle = vo.OraclePlan(c["ddem"], c["ref"], labels=c["labels"])
        counts, _, _ = oracle.segments(c["ids"], c["edges"])
        one, several = vc.run_groups(oracle.groups())
        if not noise:
            assert np.count_nonzero(counts) == 40 and set(counts[counts > 0]) == {128} and (one, several) == (80, 0)
        else:
            assert one == 0 and several == 80 and np.count_nonzero(counts) > 100 and np.count_nonzero(oracle.groups() < 0) > 0


@pytest.mark.parametrize("dtype", vc.DTYPES)
def test_threshold_case_has_segments_on_both_sides_of_8192(dtype):
    c = vc.threshold_case(dtype)
    oracle = vo.OraclePlan(c["ddem"], c["ref"])
    counts, med, _ = oracle.segments([1], vc.THRESHOLD_EDGES)
    assert counts.tolist() == [list(vc.THRESHOLD_COUNTS)] and c["ddem"].shape == (24576,)
    for b in range(3):
        v = c["ddem"][c["bin"] == b]
        assert med[0, b] == np.median(v) and v.min() < 0 < v.max() and np.unique(v).shape[0] < v.shape[0]


@pytest.mark.parametrize("dtype", vc.DTYPES)
def test_area_case_has_pixels_on_interior_edges_the_last_edge_and_outside(dtype):
    for nb in (8192, 8193):   # HYP_AREA_LDS_BINS and one more
        c = vc.area_case(nb, dtype)
        ref, bins = c["ref"].astype(np.float64), c["bins"]
        assert bins.shape == (nb + 1,) and np.isnan(ref).sum() > 0
        assert np.count_nonzero(ref == bins[-1]) > 0 and np.count_nonzero(ref > bins[-1]) > 0 and np.count_nonzero(ref < bins[0]) > 0
        assert np.count_nonzero(np.isin(ref, bins[1:-1])) > 4000
        counts = vo.area_counts(c["ref"], 0, c["xs"], c["ys"], bins)
        assert counts[-1] == np.count_nonzero((ref == bins[-1]) | (ref == bins[-2]))
