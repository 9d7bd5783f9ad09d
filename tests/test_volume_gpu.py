"""xdem_amd.volume on the device against the reference's fixtures (tools/gen_golden_volume.py), against the NumPy restatement at
shapes without fixtures, and its internal routes against each other.

Bit for bit: every DataFrame of hypsometric_binning, calculate_hypsometry_area, hypsometric_interpolation, the regional signal, every
glacier's skip decision, counts and medians, and the fill pass fed the recorded model tables.  The per-bin standard deviation is
float64 on the device and float32, summed pairwise in sample order, upstream: its largest deviation from the fixtures, relative to
the bin's standard deviation, and through it the largest deviation of the fitted coefficients, the model tables and the filled
pixels, relative to the glacier's largest model value, were measured on an MI355X (volume_cases.MEASURED: float32 1.2e-7 and
1.5e-6, float64 2.2e-16 and 9.6e-8); each bar is 4 x its figure.  The figures of the two mixed pairs (float32 dDEM with a float64
reference and the reverse, 61 x 83) are those of the NumPy restatement against the pairs' fixtures, computed on the CPU
(volume_cases.regional_bars)."""
import numpy as np
import pytest

import volume_cases as vc
import volume_oracle as vo

pytestmark = pytest.mark.gpu

CASES = [(H, W, dt) for (H, W) in vc.SHAPES for dt in vc.DTYPES] + [(61, 83, dt) for dt in vc.MIXED]


@pytest.fixture(scope="module")
def vol():
    from xdem_amd import volume

    return volume


def _put(a):
    import torch

    return torch.from_numpy(np.array(a)).cuda()


def _check_regional(got, ref, c, dtype):
    std_dev, model_dev = vc.regional_deviations(got, ref, c)
    std_bar, model_bar = vc.regional_bars(dtype, ref)
    print(f"std deviation {std_dev:.3e} (bar {std_bar:.3e}), model deviation {model_dev:.3e} (bar {model_bar:.3e})")
    assert std_dev <= std_bar and model_dev <= model_bar


@pytest.mark.parametrize("H,W,dtype", CASES)
def test_binning_area_interpolation_signal_fixtures(vol, H, W, dtype):
    c, g = vc.case(H, W, dtype), vc.golden(H, W, dtype)
    got = vc.run_binning(vol, c)
    got.update(vc.run_area(vol, c, g))
    got.update(vc.run_hypso_interp(vol, c))
    got.update(vc.run_signal(vol, c))
    vc.assert_same_bits(got, g)


@pytest.mark.parametrize("H,W,dtype", CASES)
def test_regional_interpolation_fixtures(vol, H, W, dtype):
    c, g = vc.case(H, W, dtype), vc.golden(H, W, dtype)
    _check_regional(vc.run_regional(vol, c, g), g, c, dtype)


@pytest.mark.parametrize("H,W,dtype", CASES)
def test_fill_pass_fed_the_recorded_tables(vol, H, W, dtype):
    c, g = vc.case(H, W, dtype), vc.golden(H, W, dtype)
    ids = [int(i) for i, s in zip(g["glacier_ids"], g["glacier_skipped"]) if not s]
    xs, ys = [g[f"glacier_{i}_x"] for i in ids], [g[f"glacier_{i}_y"] for i in ids]
    with vol.HypsoPlan(c["ddem"], c["ref"], labels=c["labels"]) as plan:
        for mode, name in ((0, "regional_filled"), (1, "regional_idealized")):
            out = plan.fill(mode, ids, xs, ys, False, vc.ddem_dtype(dtype)).reshape(H, W)
            vc.assert_same_bits({name: out}, g)


@pytest.mark.parametrize("H,W", [(1, 200), (200, 1)])
@pytest.mark.parametrize("dtype", vc.DTYPES)
def test_against_the_restatement_on_thin_rasters(vol, H, W, dtype):
    c = vc.case(H, W, dtype)
    with vo.patched() as ovol:
        want = vc.run_binning(ovol, c)
        want.update(vc.run_hypso_interp(ovol, c))
        want.update(vc.run_signal(ovol, c))
        want.update(vc.run_area(ovol, c, vc.golden(61, 83, dtype)))
        want_reg = vc.run_regional(ovol, c, want)
    got = vc.run_binning(vol, c)
    got.update(vc.run_hypso_interp(vol, c))
    got.update(vc.run_signal(vol, c))
    got.update(vc.run_area(vol, c, vc.golden(61, 83, dtype)))
    vc.assert_same_bits(got, want)
    _check_regional(vc.run_regional(vol, c, want), want_reg, c, dtype)


@pytest.mark.parametrize("dtype", vc.DTYPES)
def test_device_input_gives_the_host_input_bits_on_the_device(vol, dtype):
    import torch

    c, g = vc.case(61, 83, dtype), vc.golden(61, 83, dtype)
    host = vc.run_binning(vol, c)
    host.update(vc.run_hypso_interp(vol, c))
    host.update(vc.run_area(vol, c, g))
    host_reg = vc.run_regional(vol, c, g)
    dev = vc.run_binning(vol, c, _put)
    dev.update(vc.run_hypso_interp(vol, c, _put))
    dev.update(vc.run_area(vol, c, g, _put))
    vc.assert_same_bits(dev, host)
    vc.assert_same_bits(vc.run_regional(vol, c, g, _put), host_reg)
    out = vol.norm_regional_hypsometric_interpolation(_put(c["ddem"]), _put(c["ref"]), _put(c["labels"]), regional_signal=vc.signal_frame(g))
    assert isinstance(out, torch.Tensor) and out.is_cuda and tuple(out.shape) == (61, 83)
    assert isinstance(vol.hypsometric_interpolation(_put(c["ddem"]), _put(c["ref_voids"]), _put(c["mask"])), torch.Tensor)
    # other label dtypes: converted on the device
    for lab in (_put(c["labels"].astype(np.int64)), _put(c["labels"].astype(np.float64))):
        again = vol.norm_regional_hypsometric_interpolation(_put(c["ddem"]), _put(c["ref"]), lab, regional_signal=vc.signal_frame(g))
        assert torch.equal(torch.nan_to_num(again, nan=1e30), torch.nan_to_num(out, nan=1e30))


@pytest.mark.parametrize("dtype", vc.MIXED)
def test_mixed_dtype_pairs_on_device_tensors(vol, dtype):
    """A float32 dDEM with a float64 reference and the reverse, as device tensors, against the fixtures of the pair: the
    (float, double) and (double, float) instances of the statistics, grouping and fill kernels.  hypsometric_interpolation promotes
    its output to float64 for both pairs (the model's value rounded to the reference's dtype first); the regional fill keeps the
    dDEM's dtype."""
    import torch

    c, g = vc.case(61, 83, dtype), vc.golden(61, 83, dtype)
    assert (c["ddem"].dtype, c["ref"].dtype, c["ref_voids"].dtype) == (vc.ddem_dtype(dtype), vc.ref_dtype(dtype), vc.ref_dtype(dtype))
    hi = vol.hypsometric_interpolation(_put(c["ddem"]), _put(c["ref_voids"]), _put(c["mask"]))
    assert isinstance(hi, torch.Tensor) and hi.is_cuda and hi.dtype == torch.float64 and tuple(hi.shape) == (61, 83)
    data = hi.cpu().numpy()
    vc.assert_same_bits({"hypso_interp_data": data, "hypso_interp_mask": ~np.isfinite(data)}, g)
    masked = vol.hypsometric_interpolation(c["ddem"], c["ref_voids"], c["mask"])
    assert isinstance(masked, np.ma.MaskedArray) and masked.dtype == np.float64
    vc.assert_same_bits({"hypso_interp_data": np.asarray(masked.data), "hypso_interp_mask": np.ma.getmaskarray(masked)}, g)
    dev = vc.run_binning(vol, c, _put)
    dev.update(vc.run_area(vol, c, g, _put))
    dev.update(vc.run_signal(vol, c, _put))
    vc.assert_same_bits(dev, g)
    reg = vc.run_regional(vol, c, g, _put)
    assert reg["regional_filled"].dtype == vc.ddem_dtype(dtype)
    _check_regional(reg, g, c, dtype)
    vc.assert_same_bits(reg, vc.run_regional(vol, c, g))


def test_two_runs_return_the_same_bits(vol):
    c, g = vc.case(129, 193, "float32"), vc.golden(129, 193, "float32")
    first = vc.run_regional(vol, c, g, _put)
    vc.assert_same_bits(vc.run_regional(vol, c, g, _put), first)


def _segments_both_routes(vol, plan, ids, edges, long_above):
    from xdem_amd import _lib

    lds = plan.segments(ids, edges, want_std=True)
    with _lib.default_context().option_scope("hypso_seg_lds", long_above):
        long = plan.segments(ids, edges, want_std=True)
        long_median_only = plan.segments(ids, edges)
    for a, b in zip(lds, long):
        assert np.array_equal(a, b, equal_nan=True)
    assert np.array_equal(lds[0], long_median_only[0]) and np.array_equal(lds[1], long_median_only[1], equal_nan=True)
    return lds


@pytest.mark.parametrize("dtype", vc.DTYPES)
def test_long_segment_route_returns_the_lds_route_bits(vol, dtype):
    # one segment of 40 values (ties, both signs, an even count) and one of 41, with the threshold at 32
    k = np.arange(81)
    ddem = (((k * 37) % 23) - 11.0).astype(dtype) / 4
    ref = np.where(k < 40, 10.0, 20.0).astype(dtype)
    edges = np.array([[0.0, 15.0, 25.0]])
    with vol.HypsoPlan(ddem, ref) as plan:
        counts, med, sd = _segments_both_routes(vol, plan, [1], edges, 32)
    assert counts.tolist() == [[40, 41]]
    assert med[0, 0] == np.median(ddem[:40]) and med[0, 1] == np.median(ddem[40:])
    want = [np.sqrt(np.mean((np.sort(v).astype(np.float64) - np.sort(v).astype(np.float64).mean()) ** 2)) for v in (ddem[:40], ddem[40:])]
    assert np.allclose(sd[0], want, rtol=1e-14, atol=0)
    # every glacier's bins of the fixture case: segments of 1 to a few hundred values on either side of a threshold of 8
    c = vc.case(129, 193, dtype)
    with vol.HypsoPlan(c["ddem"], c["ref"], labels=c["labels"]) as plan:
        st = plan.label_stats()
        keep = st["inliers"] > 0
        edges = np.linspace(st["ref_min"][keep], st["ref_max"][keep], 21).T
        counts, _, _ = _segments_both_routes(vol, plan, st["ids"][keep], edges, 8)
    assert counts.max() > 8 and 0 < counts[counts > 0].min() <= 8


def test_label_at_the_limit_is_refused(vol):
    c = vc.case(61, 83, "float32")
    lab = c["labels"].copy()
    lab[0, 0] = 1 << 20
    with pytest.raises(ValueError, match=r"2\^20"):
        vol.get_regional_hypsometric_signal(c["ddem"], c["ref"], lab)
    with pytest.raises(ValueError, match=r"2\^20"):
        vol.norm_regional_hypsometric_interpolation(_put(c["ddem"]), _put(c["ref"]), _put(lab.astype(np.int64)))
    lab[0, 0] = (1 << 20) - 1
    vol.get_regional_hypsometric_signal(c["ddem"], c["ref"], lab)


def test_callable_statistics_run_on_the_host_from_device_bin_numbers(vol):
    c = vc.case(61, 83, "float32")
    with vo.patched() as ovol:
        want = ovol.hypsometric_binning(c["ddem"], c["ref_voids"], aggregation_function=np.nanstd)
    got = vol.hypsometric_binning(c["ddem"], c["ref_voids"], aggregation_function=np.nanstd)
    assert got.equals(want)
    ref = vc.golden(61, 83, "float32")
    mean = vol.hypsometric_binning(c["ddem"], c["ref_voids"], aggregation_function=np.mean)
    assert np.array_equal(mean["count"].values, ref["bin_fixed_count"])
