"""The device stack (csrc/demstack.hip behind xdem_amd.demcollection.StackPlan) against its NumPy restatement
(demstack_oracle.OracleStack), through the public DEMCollection: dDEM planes, equal-to-reference decisions and counts bit for bit, the
filled planes bit for bit against both the restatement and per-pair ``volume.hypsometric_interpolation`` on the same device, the series
counts exact and the means within the derived any-order bound of the exactly rounded mean; the same bits from two runs and from host
and tensor inputs; device inputs give device outputs.

Shapes 61 x 83 and 129 x 193 (neither a multiple of the workgroup's 256 pixels), stacks of 1, 2 and 5 DEMs, of STK_CHUNK = 8 and 9 (a
thread keeps the counters of 8 planes and walks the pixels once per chunk), one raster of 2.25 trips of the grid-stride loops, and a
lowered "hypso_seg_lds" that puts (plane, bin) segments on both sides of the LDS-sort switch."""
import functools
import warnings

import numpy as np
import pytest

import demcollection_cases as dc
import demstack_oracle
import volume_cases as vc

pytestmark = pytest.mark.gpu

CHUNK = 8   # STK_CHUNK of csrc/demstack.hip


@functools.lru_cache(maxsize=None)
def _num_cu() -> int:
    import torch

    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def make_dems(ref: np.ndarray, dd: np.ndarray, T: int, ref_index: int, special: dict | None = None) -> list:
    """T planes: the reference at ref_index, the others ref - (t - ref_index) / 3 * dd rounded to the dtype (full mantissas: the float64 sums round); special: {plane: "copy" | "nan"}."""
    dt = ref.dtype
    out = []
    for t in range(T):
        kind = (special or {}).get(t)
        if t == ref_index:
            out.append(ref)
        elif kind == "copy":
            out.append(ref.copy())
        elif kind == "nan":
            out.append(np.full_like(ref, np.nan))
        else:
            with np.errstate(invalid="ignore"):
                out.append((ref - dt.type((t - ref_index) / 3.0) * dd).astype(dt))
    return out


def years(T: int) -> tuple:
    return tuple(2000 + 3 * t for t in range(T))


def finite_ddem(c: dict) -> np.ndarray:
    return np.where(np.isfinite(c["ddem"]), c["ddem"], np.nan).astype(c["ddem"].dtype)


def to_device(a):
    import torch

    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return t


def run(planes, ref_index, outlines, tensors: bool = False, patched: bool = False) -> dict:
    """The whole pipeline of a collection: what it leaves, as host arrays."""
    from xdem_amd import DEMCollection, ddem as ddem_mod

    put = to_device if tensors else (lambda a: a)
    dems = [ddem_mod.raster_of(put(p), dc.TRANSFORM) for p in planes]
    if isinstance(outlines, dict):
        outlines = {k: put(v) for k, v in outlines.items()}
    elif outlines is not None:
        outlines = put(outlines)
    out: dict = {}

    def body():
        col = DEMCollection(dems, timestamps=dc.stamps(years(len(planes))), outlines=outlines, reference_dem=ref_index)
        ddems = col.subtract_dems()
        out["is_tensor"] = [hasattr(d.data, "data_ptr") for d in ddems]
        out["ddem"] = [vc.to_host(d.data) for d in ddems]
        out["equal"] = [d.error == 0 and float(d.time) == 0 for d in ddems]
        out["has_voids"] = [d.filled_data is None for d in ddems]
        out["raw"] = col._series_figures(None, None)
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            filled = col.interpolate_ddems("regional_hypsometric")
        out["warnings"] = sorted(str(w.message) for w in caught)
        out["filled_is_tensor"] = [hasattr(f, "data_ptr") for f in filled]
        out["filled"] = [vc.to_host(f) for f in filled]
        out["fused"] = col._series_figures(None, None)
        out["reduced"] = col._plan.series(demstack_oracle.FILLED)
        full = np.ones(planes[0].shape, bool)
        out["full"] = col._series_figures(put(full), None)
        out["masks"] = [vc.to_host(col.get_ddem_mask(d)) for d in ddems]
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            out["dh"] = col.get_dh_series(nans_ok=True)
        out["col"] = col

    if patched:
        with demstack_oracle.patched():
            body()
    else:
        body()
    return out


def assert_same_run(a: dict, b: dict) -> None:
    """Two runs: the same bits everywhere, sums included."""
    for k in ("ddem", "filled"):
        for x, y in zip(a[k], b[k]):
            assert x.dtype == y.dtype and np.array_equal(x, y, equal_nan=True), k
    for k in ("raw", "fused", "reduced", "full"):
        for x, y in zip(a[k], b[k]):
            assert np.array_equal(x.view(np.int64), y.view(np.int64)), k
    assert a["equal"] == b["equal"] and a["has_voids"] == b["has_voids"] and a["warnings"] == b["warnings"]


def assert_matches_oracle(got: dict, want: dict, planes, ref_index: int) -> None:
    from xdem_amd import volume

    ref = planes[ref_index]
    for t in range(len(planes)):
        assert got["ddem"][t].dtype == want["ddem"][t].dtype == ref.dtype
        assert np.array_equal(got["ddem"][t], want["ddem"][t], equal_nan=True), f"dDEM {t}: {np.count_nonzero(~((got['ddem'][t] == want['ddem'][t]) | np.isnan(want['ddem'][t])))} pixels differ"
        assert np.array_equal(got["filled"][t], want["filled"][t], equal_nan=True), f"filled {t}"
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            per_pair = volume.hypsometric_interpolation(got["ddem"][t], ref, got["masks"][t])   # (the device's own per-pair route)
        assert np.array_equal(got["filled"][t], np.asarray(per_pair.data), equal_nan=True) and got["filled"][t].dtype == per_pair.dtype, f"per pair {t}"
    assert got["equal"] == want["equal"] and got["has_voids"] == want["has_voids"] and got["warnings"] == want["warnings"]
    for m_got, m_want in zip(got["masks"], want["masks"]):
        assert np.array_equal(m_got, m_want)
    # the fused sums of the fill pass are those of the reduce-only pass over the filled planes
    for x, y in zip(got["fused"], got["reduced"]):
        assert np.array_equal(x.view(np.int64), y.view(np.int64))
    for k, source in (("raw", "ddem"), ("fused", "filled"), ("full", "filled")):
        n_mask, n_fin, sums = got[k]
        w_mask, w_fin, w_sums = want[k]
        assert np.array_equal(n_mask, w_mask) and np.array_equal(n_fin, w_fin), k
        for t in range(len(planes)):
            m = np.ones(ref.shape, bool) if k == "full" else got["masks"][t]
            n, mean, mean_abs = dc.moments(got[source][t][m])
            assert n == n_fin[t] and np.count_nonzero(m) == n_mask[t], (k, t)
            if n == 0:
                assert sums[t] == 0.0
                continue
            dev, bound = abs(sums[t] / n - mean), dc.any_order_bound(n, mean, mean_abs, 2.0 ** -53)
            assert dev <= bound, (k, t, dev, bound)
            assert abs(w_sums[t] / n - mean) <= 2.0 ** -53 * abs(mean)   # (the restatement: math.fsum, one rounding, one division)
    assert np.array_equal(got["dh"].index, want["dh"].index) and np.array_equal(got["dh"]["area"].values, want["dh"]["area"].values)
    assert np.array_equal(np.isnan(got["dh"]["dh"].values), np.isnan(want["dh"]["dh"].values))


def case_planes(H, W, dtype, T, ref_index, special=None):
    c = vc.case(H, W, dtype)
    return make_dems(c["ref_voids"], finite_ddem(c), T, ref_index, special), c["mask"]


@pytest.mark.parametrize("T,ref_index", [(1, 0), (2, 0), (5, 2), (CHUNK, 3), (CHUNK + 1, CHUNK)])
@pytest.mark.parametrize("dtype", dc.DTYPES)
@pytest.mark.parametrize("H,W", dc.SHAPES)
def test_stack_matches_the_restatement(H, W, dtype, T, ref_index):
    """The reference alone; ordinary stacks with the reference first and in the middle; a full chunk of planes and one plane more (the
    reference in the second chunk)."""
    planes, mask = case_planes(H, W, dtype, T, ref_index)
    got = run(planes, ref_index, mask)
    want = run(planes, ref_index, mask, patched=True)
    assert_matches_oracle(got, want, planes, ref_index)
    assert got["equal"] == [t == ref_index for t in range(T)]
    assert not any(got["is_tensor"]) and not any(got["filled_is_tensor"])


@pytest.mark.parametrize("H,W,dtype", [(61, 83, "float32"), (129, 193, "float64")])
def test_two_runs_and_both_memspaces_give_the_same_bits(H, W, dtype):
    planes, mask = case_planes(H, W, dtype, 5, 2)
    first = run(planes, 2, mask)
    assert_same_run(first, run(planes, 2, mask))
    on_device = run(planes, 2, mask, tensors=True)
    assert all(on_device["is_tensor"]) and all(on_device["filled_is_tensor"])   # device inputs give device outputs
    assert_same_run(first, on_device)
    assert_same_run(on_device, run(planes, 2, mask, tensors=True))


@pytest.mark.parametrize("dtype", dc.DTYPES)
def test_equal_copy_all_nan_plane_and_mask_without_inlier(dtype):
    """Plane 1 equals the reference but is another object: the all-zero dDEM, error 0.  Plane 3 is all NaN: no inlier, the warning, the
    plane copied, dh NaN.  Plane 4's outline covers only voids of the reference: no inlier either."""
    H, W = 61, 83
    planes, mask = case_planes(H, W, dtype, 5, 0, {1: "copy", 3: "nan"})
    ref_voids = ~np.isfinite(planes[0])
    assert ref_voids.any()
    got = run(planes, 0, mask)
    want = run(planes, 0, mask, patched=True)
    assert_matches_oracle(got, want, planes, 0)
    assert got["equal"] == [True, True, False, False, False] and not got["ddem"][1].any() and got["ddem"][1].dtype == planes[0].dtype
    assert np.isnan(got["ddem"][3]).all() and np.isnan(got["filled"][3]).all()
    assert got["warnings"].count("No valid data found within mask, returning copy") == 1
    assert np.isnan(got["dh"]["dh"].iloc[1]) and got["fused"][1][3] == 0 and got["fused"][0][3] == np.count_nonzero(mask)
    only_voids = run(planes[:1] + planes[4:], 0, ref_voids)
    assert_matches_oracle(only_voids, run(planes[:1] + planes[4:], 0, ref_voids, patched=True), planes[:1] + planes[4:], 0)
    assert only_voids["warnings"] == ["No valid data found within mask, returning copy"] * 2   # (the reference's own zero dDEM too)
    assert np.array_equal(only_voids["filled"][1], only_voids["ddem"][1], equal_nan=True) and np.isnan(only_voids["dh"]["dh"].iloc[0])


@pytest.mark.parametrize("dtype", dc.DTYPES)
def test_voids_only_outside_the_mask(dtype):
    c = vc.case(129, 193, dtype)
    dd = finite_ddem(c)
    dd = np.where(c["mask"] & ~np.isfinite(dd), dd.dtype.type(0.25), dd)
    ref = np.where(c["mask"] & ~np.isfinite(c["ref_voids"]), c["ref"], c["ref_voids"])
    planes = make_dems(ref, dd, 3, 1)
    got = run(planes, 1, c["mask"])
    assert_matches_oracle(got, run(planes, 1, c["mask"], patched=True), planes, 1)
    for t in (0, 2):
        assert np.isnan(got["ddem"][t]).any() and np.array_equal(got["filled"][t], got["ddem"][t], equal_nan=True)   # nothing is filled


@pytest.mark.parametrize("tensors", [False, True])
def test_one_shared_mask_and_one_mask_per_plane_with_a_union(tensors):
    H, W, dtype, T = 129, 193, "float32", 4
    planes, mask = case_planes(H, W, dtype, T, 0)
    shared = run(planes, 0, mask, tensors=tensors)
    assert len(shared["col"]._plan.masks) == 1
    stamps = dc.stamps(years(T))
    outlines = {stamps[0]: mask, stamps[2]: np.roll(mask, 9, axis=1), stamps[3]: np.roll(mask, -11, axis=0)}
    got = run(planes, 0, outlines, tensors=tensors)
    want = run(planes, 0, outlines, patched=True)
    assert_matches_oracle(got, want, planes, 0)
    # plane 1: the start key only; planes 2 and 3: the union of two outlines; plane 0 (the reference): its own key twice
    assert len(got["col"]._plan.masks) == 3 and got["col"]._plan.mask_ids.tolist() == [0, 0, 1, 2]
    assert np.array_equal(got["masks"][1], mask) and np.array_equal(got["masks"][2], mask | outlines[stamps[2]])
    assert np.array_equal(got["masks"][3], mask | outlines[stamps[3]])
    assert not np.array_equal(got["filled"][2], shared["filled"][2], equal_nan=True)


@pytest.mark.parametrize("tensors", [False, True])
def test_every_plane_its_own_mask(tensors):
    """K = T: an outline for every stamp, so every plane has a mask of its own (three of them unions of two outlines)."""
    H, W, dtype, T = 129, 193, "float32", 4
    planes, mask = case_planes(H, W, dtype, T, 0)
    stamps = dc.stamps(years(T))
    outlines = {stamps[0]: mask, stamps[1]: np.roll(mask, 5, axis=0), stamps[2]: np.roll(mask, 9, axis=1), stamps[3]: np.roll(mask, 23, axis=1)}
    got = run(planes, 0, outlines, tensors=tensors)
    assert_matches_oracle(got, run(planes, 0, outlines, patched=True), planes, 0)
    assert len(got["col"]._plan.masks) == T and got["col"]._plan.mask_ids.tolist() == [0, 1, 2, 3]
    for t in range(1, T):
        assert np.array_equal(got["masks"][t], mask | outlines[stamps[t]])
    assert len({m.tobytes() for m in got["masks"]}) == T


def test_a_write_into_device_filled_data_is_seen_by_the_series():
    """A device array IS the stack's plane: after an in-place write into a dDEM's filled_data the sums of the fill pass are not reused,
    and dh is that of the planes as they are.  The write is queued on torch's stream BEHIND tens of milliseconds of other work (three
    8192^2 matrix products) and the series is asked for at once: the library's stream does not order against torch's, so the pass
    reads the written plane only because it waits for torch's stream first."""
    import torch

    planes, mask = case_planes(61, 83, "float32", 3, 0)
    got = run(planes, 0, mask, tensors=True)
    col = got["col"]
    before = col.get_dh_series()["dh"].values.copy()
    assert mask[10].any()
    a = torch.ones((8192, 8192), device="cuda")
    torch.cuda.synchronize()
    for _ in range(3):
        a = torch.mm(a, a) * 1e-4
    col.ddems[1].filled_data[10] += 64.0
    after = col.get_dh_series()["dh"].values
    n, mean, mean_abs = dc.moments(vc.to_host(col.ddems[1].filled_data)[mask])
    assert after[0] != before[0] and abs(after[0] - mean) <= dc.any_order_bound(n, mean, mean_abs, 2.0 ** -53)
    assert after[1].tobytes() == before[1].tobytes()
    # the same for a write into a dDEM's data before the fill: the batched fill computes over the plane as written
    got = run(planes, 0, mask, tensors=True)
    col = got["col"]
    col.subtract_dems()
    for _ in range(3):
        a = torch.mm(a, a) * 1e-4
    col.ddems[2].data[10] += 64.0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        filled = vc.to_host(col.interpolate_ddems("regional_hypsometric")[2])
        edited = vc.to_host(col.ddems[2].data)
        from xdem_amd import volume

        per_pair = volume.hypsometric_interpolation(edited, planes[0], mask)
    assert np.array_equal(filled, np.asarray(per_pair.data), equal_nan=True)
    assert not np.array_equal(filled, got["filled"][2], equal_nan=True)


def test_inliers_within_one_bin():
    """Inliers that span less than one 50 m bin: a one-point table, SciPy's NaN for the plane's voids inside the mask."""
    planes, mask = case_planes(61, 83, "float32", 2, 0)
    ref = np.full((61, 83), 1000.0, np.float32)
    ref[:, :40] += 20.0
    with np.errstate(invalid="ignore"):
        dems = [ref, (ref - (planes[0] - planes[1])).astype(np.float32)]
    from xdem_amd import DEM, DEMCollection

    def fill():
        col = DEMCollection([DEM.from_array(d, dc.TRANSFORM) for d in dems], timestamps=dc.stamps(years(2)), outlines=mask)
        data = col.subtract_dems()[1].data
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            return data, col.interpolate_ddems("regional_hypsometric")[1]

    data, filled = fill()
    with demstack_oracle.patched():
        w_data, w_filled = fill()
    voids = ~np.isfinite(data)
    assert np.array_equal(data, w_data, equal_nan=True) and np.array_equal(filled, w_filled, equal_nan=True)
    assert (voids & mask).any() and np.isnan(filled[voids]).all() and np.array_equal(filled[~voids], data[~voids])


@pytest.mark.parametrize("dtype", dc.DTYPES)
def test_workgroups_that_make_more_than_one_trip(dtype):
    """T = 2 on the raster of volume_cases.multi_trip_case: 2.25 trips of grid_for(ctx, n, 256, 16), and (n / 256) / (num_cu * 8) = 4.5
    trips of the fixed-order grid of the fill pass."""
    c = vc.multi_trip_case(_num_cu(), dtype)
    assert c["ddem"].size > 2 * vc.trip_pixels(_num_cu())
    planes = make_dems(c["ref_voids"], finite_ddem(c), 2, 0)
    got = run(planes, 0, c["mask"])
    assert_matches_oracle(got, run(planes, 0, c["mask"], patched=True), planes, 0)


@pytest.mark.parametrize("dtype", dc.DTYPES)
def test_segments_on_both_sides_of_the_lds_switch(dtype):
    from xdem_amd import _lib

    H, W, limit = 61, 83, 40
    planes, mask = case_planes(H, W, dtype, 3, 1)
    want = run(planes, 1, mask, patched=True)
    oracle = want["col"]._plan
    inl, lo, hi = oracle.inlier_stats()
    from xdem_amd import volume

    sizes = []
    for t in (0, 2):
        z = np.asarray(volume._zbins("fixed", 50.0, planes[0].dtype.type(lo[t]), planes[0].dtype.type(hi[t]), None), dtype=np.float64)
        nbs = np.zeros(3, np.int32)
        nbs[t] = z.shape[0] - 1
        edges = np.full((3, z.shape[0]), np.inf)
        edges[t] = z
        sizes.extend(oracle.segments(nbs, edges)[0][t].tolist())
    assert any(0 < s <= limit for s in sizes) and any(s > limit for s in sizes), sizes
    ctx = _lib.default_context()
    with ctx.option_scope("hypso_seg_lds", limit):
        got = run(planes, 1, mask)
    assert_matches_oracle(got, want, planes, 1)
    assert_same_run(got, run(planes, 1, mask))


@pytest.mark.parametrize("dtype", dc.DTYPES)
@pytest.mark.parametrize("H,W", dc.SHAPES)
def test_series_match_the_reference_on_the_device(H, W, dtype):
    """The device's series against the reference's recorded ones (tests/test_demcollection_host.py does the same over the restatement);
    prints the largest |dh - recorded| / mean|x|, the figure of demcollection_cases.MEASURED."""
    import json
    import os

    from xdem_amd import DEM, DEMCollection

    with open(os.path.join(dc.GOLDEN, "signatures_ddem.json")) as f:
        texts = json.load(f)["warnings"]
    g, s = dc.golden(), dc.stack(H, W, dtype)
    full = np.ones((H, W), bool)
    col = DEMCollection([DEM.from_array(d, dc.TRANSFORM, None) for d in s["dems"]], timestamps=dc.stamps(), outlines=s["mask"], reference_dem=dc.REFERENCE)
    others = [d for t, d in enumerate(col.subtract_dems()) if t != dc.REFERENCE]
    worst = 0.0
    for state in ("raw", "filled"):
        if state == "filled":
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                col.interpolate_ddems("regional_hypsometric")
        for region, kw in (("full", {"mask": full}), ("mask", {})):
            prefix = f"{H}x{W}_{dtype}_{state}_{region}"
            sources = [d.data if state == "raw" else d.filled_data for d in others]
            worst = max(worst, dc.assert_series(dc.series_of(col, **kw), g, prefix, dtype, sources, kw.get("mask", s["mask"]), texts[prefix]))
    print(f"MEASURED {H}x{W} {dtype}: largest |dh - recorded| / mean|x| {worst:.3e}")
