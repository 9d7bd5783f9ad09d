"""The cases of the xdem_amd.volume fixtures (tools/gen_golden_volume.py), run on a given ``volume`` module -- the device's, or the
NumPy restatement's (volume_oracle.patched) -- and compared with a fixture: shared by test_volume_host.py and test_volume_gpu.py."""
from __future__ import annotations

import os
import warnings

import numpy as np

from xdem_amd import synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SHAPES = ((61, 83), (129, 193))
DTYPES = ("float32", "float64")
MIXED = ("float32_float64", "float64_float32")   # "<dDEM dtype>_<reference dtype>": recorded at 61 x 83 only
CUSTOM_EDGES = np.arange(900.0, 1800.0, 100.0)
PIXEL_SIZE = 30.0
COUNT_THRESHOLD = 40

_golden: dict = {}
_cases: dict = {}


def golden(H: int, W: int, dtype: str) -> dict:
    key = (H, W, dtype)
    if key not in _golden:
        with np.load(os.path.join(GOLDEN, f"volume_{H}x{W}_{dtype}.npz")) as z:
            _golden[key] = {k: z[k] for k in z.files}
    return _golden[key]


def ddem_dtype(dtype: str) -> np.dtype:
    return np.dtype(dtype.split("_")[0])


def ref_dtype(dtype: str) -> np.dtype:
    return np.dtype(dtype.split("_")[-1])


def case(H: int, W: int, dtype: str) -> dict:
    """synth.volume_case, built once per shape and dtype and never written to.  A mixed pair takes the dDEM of the case of its first
    dtype and ``ref`` / ``ref_voids`` of the case of its second; labels and mask are the same in both."""
    key = (H, W, dtype)
    if key not in _cases and "_" in dtype:
        d, r = case(H, W, ddem_dtype(dtype).name), case(H, W, ref_dtype(dtype).name)
        assert np.array_equal(d["labels"], r["labels"]) and np.array_equal(d["mask"], r["mask"])
        _cases[key] = {"ddem": d["ddem"], "ref": r["ref"], "ref_voids": r["ref_voids"], "labels": d["labels"], "mask": d["mask"]}
    if key not in _cases:
        c = synth.volume_case(H, W, np.dtype(dtype))
        for v in c.values():
            v.setflags(write=False)
        _cases[key] = c
    return _cases[key]


def binning_cases(c: dict) -> dict:
    ref = c["ref_voids"]
    return {"fixed": (50.0, "fixed"), "count": (12, "count"), "quantile": (8, "quantile"), "custom": (CUSTOM_EDGES, "custom"),
            "array": (np.linspace(float(np.nanmin(ref)), float(np.nanmax(ref)), 12), "fixed")}


def frame_columns(prefix: str, df, out: dict) -> None:
    out[prefix + "_left"] = np.asarray(df.index.left)
    out[prefix + "_right"] = np.asarray(df.index.right)
    for col in df.columns:
        out[prefix + "_" + col.replace("-", "_")] = np.asarray(df[col].values)


def to_host(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def run_binning(vol, c: dict, put=lambda a: a) -> dict:
    out: dict = {}
    for name, (bins, kind) in binning_cases(c).items():
        frame_columns("bin_" + name, vol.hypsometric_binning(put(c["ddem"]), put(c["ref_voids"]), bins=bins, kind=kind), out)
    return out


def run_tables(vol, fixed) -> dict:
    out: dict = {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        frame_columns("interp", vol.interpolate_hypsometric_bins(fixed), out)
        frame_columns("interp_ct", vol.interpolate_hypsometric_bins(fixed, count_threshold=COUNT_THRESHOLD), out)
        frame_columns("poly", vol.fit_hypsometric_bins_poly(fixed), out)
        frame_columns("poly_ct", vol.fit_hypsometric_bins_poly(fixed, count_threshold=COUNT_THRESHOLD, iterations=3), out)
    return out


def fixed_frame(g: dict):
    """The recorded "fixed" DataFrame of hypsometric_binning, rebuilt from its columns."""
    import pandas as pd

    return pd.DataFrame(index=pd.IntervalIndex.from_arrays(g["bin_fixed_left"], g["bin_fixed_right"]),
                        data={"value": g["bin_fixed_value"], "count": g["bin_fixed_count"]})


def run_area(vol, c: dict, g: dict, put=lambda a: a) -> dict:
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        filled = vol.interpolate_hypsometric_bins(fixed_frame(g), method="linear")
    return {"area_" + t: np.asarray(vol.calculate_hypsometry_area(filled, put(c["ref"]), PIXEL_SIZE, timeframe=t).values)
            for t in ("reference", "nonreference", "mean")}


def run_hypso_interp(vol, c: dict, put=lambda a: a) -> dict:
    hi = vol.hypsometric_interpolation(put(c["ddem"]), put(c["ref_voids"]), put(c["mask"]))
    data = to_host(hi.data if isinstance(hi, np.ma.MaskedArray) else hi)
    mask = np.ma.getmaskarray(hi) if isinstance(hi, np.ma.MaskedArray) else ~np.isfinite(data)
    return {"hypso_interp_data": data, "hypso_interp_mask": mask}


def run_signal(vol, c: dict, put=lambda a: a) -> dict:
    out: dict = {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        frame_columns("signal", vol.get_regional_hypsometric_signal(put(c["ddem"]), put(c["ref"]), put(c["labels"])), out)
    return out


def signal_frame(g: dict):
    import pandas as pd

    cols = ("w_mean", "median", "std", "sigma-1-lower", "sigma-1-upper", "sigma-2-lower", "sigma-2-upper", "count")
    return pd.DataFrame(index=pd.IntervalIndex.from_arrays(g["signal_left"], g["signal_right"]),
                        data={col: g["signal_" + col.replace("-", "_")] for col in cols})


def run_regional(vol, c: dict, g: dict, put=lambda a: a) -> dict:
    """norm_regional_hypsometric_interpolation (both forms) and its per-glacier records, fed the RECORDED regional signal, so that
    this comparison does not hang on the signal's own."""
    out: dict = {}
    sig = signal_frame(g)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        for name, idealized in (("filled", False), ("idealized", True)):
            out["regional_" + name] = to_host(vol.norm_regional_hypsometric_interpolation(
                put(c["ddem"]), put(c["ref"]), put(c["labels"]), regional_signal=sig, idealized_ddem=idealized))
        with vol.HypsoPlan(put(c["ddem"]), put(c["ref"]), labels=put(c["labels"])) as plan:
            records = vol.regional_glacier_models(plan, plan.label_stats(), sig, 0.1, 0.33)
    out["glacier_ids"] = np.asarray([r["id"] for r in records], dtype=np.int64)
    out["glacier_skipped"] = np.asarray([r["skipped"] for r in records], dtype=bool)
    for r in records:
        for key in ("value", "count", "std", "coeffs", "x", "y"):
            if key in r:
                out[f"glacier_{r['id']}_{key}"] = np.asarray(r[key])
    return out


def assert_same_bits(got: dict, g: dict, keys=None) -> None:
    for k in (keys if keys is not None else got):
        a, b = np.asarray(got[k]), np.asarray(g[k])
        assert a.dtype == b.dtype, f"{k}: dtype {a.dtype}, recorded {b.dtype}"
        assert a.shape == b.shape, f"{k}: shape {a.shape}, recorded {b.shape}"
        assert np.array_equal(a, b, equal_nan=True), f"{k}: {np.count_nonzero(~((a == b) | (np.isnan(a) & np.isnan(b))))} of {a.size} entries differ"


def regional_deviations(got: dict, g: dict, c: dict) -> tuple[float, float]:
    """Asserts everything of the regional interpolation that is exact (every glacier's skip decision, counts, medians, the model's
    abscissae, the pixels no model touches, the NaN pattern) and returns the two measured deviations: the largest |std - recorded| /
    recorded over all bins of all glaciers, and the largest deviation of a model quantity -- coefficients, model table, filled
    pixels -- relative to its glacier's largest recorded |model value|."""
    assert_same_bits(got, g, ["glacier_ids", "glacier_skipped"])
    assert sorted(k for k in got if k.startswith("glacier_")) == sorted(k for k in g if k.startswith("glacier_")), "glacier records differ"
    std_dev, model_dev = 0.0, 0.0
    labels = c["labels"].reshape(g["regional_filled"].shape)   # (the functions squeeze, as get_array_and_mask does)
    scale = np.zeros(labels.shape)
    for i, skipped in zip(g["glacier_ids"], g["glacier_skipped"]):
        if f"glacier_{i}_value" not in g:
            continue
        assert_same_bits(got, g, [f"glacier_{i}_value", f"glacier_{i}_count"])
        s, s0 = got[f"glacier_{i}_std"], g[f"glacier_{i}_std"]
        assert s.dtype == s0.dtype and np.array_equal(np.isnan(s), np.isnan(s0)) and np.array_equal(s == 0, s0 == 0), f"glacier {i}: std pattern"
        pos = s0 > 0
        if pos.any():
            std_dev = max(std_dev, float(np.max(np.abs(s[pos].astype(np.float64) - s0[pos]) / s0[pos])))
        if skipped:
            continue
        assert_same_bits(got, g, [f"glacier_{i}_x"])
        top = float(np.max(np.abs(g[f"glacier_{i}_y"])))
        scale[labels == i] = top
        for key in ("coeffs", "y"):
            model_dev = max(model_dev, float(np.max(np.abs(got[f"glacier_{i}_{key}"] - g[f"glacier_{i}_{key}"])) / top))
    for name in ("regional_filled", "regional_idealized"):
        a, b = got[name], g[name]
        assert a.dtype == b.dtype and a.shape == b.shape, name
        assert np.array_equal(np.isnan(a), np.isnan(b)), f"{name}: NaN pattern"
        untouched = scale == 0
        assert np.array_equal(a[untouched], b[untouched], equal_nan=True), f"{name}: pixels outside the fitted glaciers"
        fin = np.isfinite(b) & ~untouched
        assert np.array_equal(a[~fin & ~untouched], b[~fin & ~untouched], equal_nan=True), f"{name}: non-finite pixels"
        if fin.any():
            model_dev = max(model_dev, float(np.max(np.abs(a[fin].astype(np.float64) - b[fin]) / scale[fin])))
    return std_dev, model_dev


# The largest deviations from the fixtures measured on an MI355X, per dtype: (per-bin standard deviation relative to the bin's
# standard deviation, model quantities relative to the glacier's largest model value).  Upstream sums float32 pairwise in sample
# order; the device sums float64 over the sorted bin.  The bars of the tests are 4 x these figures.
MEASURED = {"float32": (1.2e-7, 1.5e-6), "float64": (2.2e-16, 9.6e-8)}
# The mixed pairs (61 x 83 only): the deviation of the NumPy restatement (volume_oracle.py) from the two mixed fixtures, computed on the
# CPU by tests/test_volume_host.py::test_restatement_matches_every_fixture (which prints them) and rounded up to two digits -- not device
# measurements.  float32 dDEM / float64 reference: 1.19e-7 and 1.47e-7; float64 dDEM / float32 reference: 2.18e-16 and 4.52e-7.
MEASURED.update({"float32_float64": (1.2e-7, 1.5e-7), "float64_float32": (2.2e-16, 4.6e-7)})


def std_bound(c) -> np.ndarray:
    """The derived relative bound of a segment's standard deviation over c values.  hyp_fixed_sum (csrc/volume.h) adds at most
    ceil(c / 256) terms per lane and folds 8 levels: gamma = (ceil(c / 256) + 8) 2^-53.  To first order the mean's error cancels in
    sum (v - mean)^2, whose relative error is at most gamma + 3 2^-53; the division and the square root add 2^-53 each, so the
    standard deviation is off by at most gamma / 2 + 4 2^-53 = (ceil(c / 256) + 16) 2^-54.  The bar is (ceil(c / 256) + 16) 2^-52,
    four times that, twice the first-order bound on the squared sum: room for the second-order terms."""
    return (np.ceil(np.asarray(c, dtype=np.float64) / 256.0) + 16.0) * 2.0 ** -52


def regional_bars(dtype: str, g: dict) -> tuple[float, float]:
    """4 x MEASURED.  A mixed pair with a float64 dDEM: upstream's std is float64 too and the restatement's deviation from it is an ulp,
    so the std bar is the larger of that and the derived summation bound for the fixture's longest bin."""
    std_bar, model_bar = (4 * f for f in MEASURED[dtype])
    if dtype in MIXED and ddem_dtype(dtype) == np.float64:
        longest = max(int(g[k].max()) for k in g if k.startswith("glacier_") and k.endswith("_count"))
        std_bar = max(std_bar, float(std_bound(longest)))
    return std_bar, model_bar


# ---- cases that reach the routes no fixture reaches (tests/test_volume_routes_gpu.py; their conditions: tests/test_volume_host.py) ----
_route_cases: dict = {}


def _frozen(key, build) -> dict:
    if key not in _route_cases:
        c = build()
        for v in c.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _route_cases[key] = c
    return _route_cases[key]


def _hash01(n: int, salt: int) -> np.ndarray:
    return synth._hash01(n, salt)


TRIP_IDS = (3, 7, 77, 1000, 5, (1 << 20) - 1, 19)
TRIP_W = 2048
TRIP_BINS = 10


def trip_pixels(num_cu: int) -> int:
    """Pixels one trip of a grid-stride loop of grid_for(ctx, n, 256, 16) covers: the grid is capped at num_cu * 16 workgroups."""
    return num_cu * 16 * 256


def multi_trip_case(num_cu: int, dtype: str) -> dict:
    """A raster of 2.25 trips (every thread makes a second full trip, some a third): ceil(2.25 n_trip / 2048) x 2048.

    ref: 1000 + row / 2, a function of the row only (so whole waves share a bin) except in 1 row of 97, where it climbs 2 m per column
    inside every run of 64, from -64 m (waves there hold several bins); float64 adds (row % 8) / 1024.  ref_voids: the same with a NaN every
    100003 pixels.  labels: bands of 8 rows cycling through TRIP_IDS, the last 8 columns 0.  ddem: the elevation trend plus hashed
    ties (float64: plus multiples of 2^-12); NaN in a fifth of the pixels of columns >= 1024 and in a tenth of their whole 64-pixel
    runs, a few +-inf; columns < 1024 carry voids only in 1 row of 32.  mask: the labels 3, 77 and 19."""
    def build():
        n_trip = trip_pixels(num_cu)
        W = TRIP_W
        H = -(-9 * n_trip // (4 * W))
        n = H * W
        k = np.arange(n)
        row, col = np.divmod(k, W)
        f64 = np.dtype(dtype) == np.float64
        ref = 1000.0 + row / 2.0
        climb = (row % 97 == 13) & (row >= 200) & (row < H - 200)   # (away from every label's lowest and highest band)
        ref[climb] += 2.0 * (col[climb] % 64) - 64.0
        if f64:
            ref = ref + (row % 8) / 1024.0
        u = [_hash01(n, 3000 * j + 17) for j in range(3)]
        ddem = -(ref - 1000.0) / 64.0 + (np.floor(64.0 * u[0]) - 32.0) / 16.0
        if f64:
            ddem = ddem + np.floor(8.0 * u[2]) / 4096.0
        right = col >= 1024
        run_void = _hash01(n // 64, 9001)[k // 64] < 0.1
        ddem[right & ((u[1] < 0.2) | run_void)] = np.nan
        ddem[~right & (row % 32 == 5) & (u[1] < 0.2)] = np.nan
        ddem[k % 99991 == 3] = np.inf
        ddem[k % 99991 == 5] = -np.inf
        lab = np.asarray(TRIP_IDS, dtype=np.int32)[(row // 8) % len(TRIP_IDS)]
        lab[col >= W - 8] = 0
        ref_voids = ref.copy()
        ref_voids[k % 100003 == 17] = np.nan
        dt = np.dtype(dtype)
        return {"ddem": ddem.astype(dt).reshape(H, W), "ref": ref.astype(dt).reshape(H, W), "ref_voids": ref_voids.astype(dt).reshape(H, W),
                "labels": lab.reshape(H, W), "mask": np.isin(lab, (3, 77, 19)).reshape(H, W)}

    return _frozen(("trip", num_cu, dtype), build)


def count_edges(st: dict, n_bins: int) -> np.ndarray:
    """Per label of `st` with an inlier: n_bins bins over its inliers' elevations, the last edge moved up as hypsometric_binning's
    kind "count" does; (labels, edges)."""
    keep = st["inliers"] > 0
    lo, hi = st["inlier_ref_min"][keep], st["inlier_ref_max"][keep]
    return st["ids"][keep], np.linspace(lo, hi + 1e-6 / n_bins, n_bins + 1).T


def run_groups(groups: np.ndarray) -> tuple[int, int]:
    """Of the whole 64-aligned runs of `groups`: how many lie in one group >= 0, how many hold several values."""
    g = groups[: groups.shape[0] // 64 * 64].reshape(-1, 64)
    one = (g == g[:, :1]).all(axis=1)
    return int(np.count_nonzero(one & (g[:, 0] >= 0))), int(np.count_nonzero(~one))


def multi_trip_conditions(c: dict, n_trip: int, groups: np.ndarray, counts: np.ndarray) -> dict:
    """What makes multi_trip_case reach its routes, from the inputs and the oracle alone."""
    lab = c["labels"].reshape(-1)
    a, b = lab[:-n_trip], lab[n_trip:]
    one, several = run_groups(groups)
    return {"trips": lab.shape[0] / n_trip, "label_changes": float(np.mean((a != 0) & (b != 0) & (a != b))), "runs_one_group": one,
            "runs_several_groups": several, "shortest_segment": int(counts[counts > 0].min()), "empty_segments": int(np.count_nonzero(counts == 0))}


def assert_multi_trip_conditions(f: dict) -> None:
    assert 2.25 <= f["trips"] < 2.26, f
    assert f["label_changes"] > 0.5, f
    assert f["runs_one_group"] > 0 and f["runs_several_groups"] > 0, f
    assert f["shortest_segment"] > 8192, f


MANY_EDGES = np.linspace(1000.0, 2000.0, 1001)


def many_groups_case(noise: bool, dtype: str) -> dict:
    """40 x 128: ref = 1000 + 25 row, labels 1 + row // 8 (5 labels); with MANY_EDGES per label 5000 groups, each row one group of two
    whole waves.  noise: the reference moves by 0 to 3 m per pixel (a wave holds four groups) and the dDEM has voids."""
    def build():
        n = 40 * 128
        k = np.arange(n)
        row = k // 128
        u = [_hash01(n, 4000 * j + 29) for j in range(3)]
        ref = 1000.0 + 25.0 * row
        ddem = (np.floor(64.0 * u[0]) - 32.0) / 16.0 - row / 8.0
        if np.dtype(dtype) == np.float64:
            ddem = ddem + np.floor(8.0 * u[2]) / 4096.0
        if noise:
            ref = ref + np.floor(4.0 * u[1])
            ddem[u[2] < 0.15] = np.nan
        dt = np.dtype(dtype)
        return {"ddem": ddem.astype(dt).reshape(40, 128), "ref": ref.astype(dt).reshape(40, 128), "labels": (1 + row // 8).astype(np.int32).reshape(40, 128),
                "ids": np.arange(1, 6, dtype=np.int32), "edges": np.tile(MANY_EDGES, (5, 1))}

    return _frozen(("many", noise, dtype), build)


def area_case(nb: int, dtype: str) -> dict:
    """A 61 x 83 reference (multiples of 1/8 m from 1000 m: every value an interior edge of `bins` = 1000 + j / 8, j = 0 .. nb) with
    pixels on the last edge, just beyond it, below the first edge and NaN; and a model table for the timeframes 1 and 2."""
    def build():
        n = 61 * 83
        k = np.arange(n)
        row, col = np.divmod(k, 83)
        ref = (8000.0 + 64.0 * row + 16.0 * col + np.floor(240.0 * _hash01(n, 5031))) / 8.0
        last = 1000.0 + nb / 8.0
        ref[k % 101 == 7] = last
        ref[k % 103 == 9] = last + 0.125
        ref[k % 107 == 11] = 999.875
        ref[k % 109 == 13] = np.nan
        ref[k % 113 == 15] = last - 0.125
        xs = np.linspace(1000.0, 1700.0, 15)
        ys = -(xs - 1000.0) / 64.0 + (np.arange(15) % 3) / 4.0
        return {"ref": ref.astype(np.dtype(dtype)), "bins": 1000.0 + np.arange(nb + 1) / 8.0, "xs": xs, "ys": ys}

    return _frozen(("area", nb, dtype), build)


THRESHOLD_COUNTS = (8191, 8192, 8193)
THRESHOLD_EDGES = np.array([[5.0, 15.0, 25.0, 35.0]])


def threshold_case(dtype: str) -> dict:
    """24576 pixels of one label in three bins of 8191, 8192 and 8193 values (the bins interleaved pixel by pixel): an odd and an even count
    on the LDS side of HYP_SEG_LDS = 8192 and an odd one beyond; dDEM with ties and both signs, all finite."""
    def build():
        k = np.arange(24576)
        b = k % 3
        b[0] = 2
        ddem = ((k * 37) % 1009 - 504.0) / 4.0
        if np.dtype(dtype) == np.float64:
            ddem = ddem + ((k * 7) % 8) / 4096.0
        return {"ddem": ddem.astype(np.dtype(dtype)), "ref": (10.0 * (b + 1)).astype(np.dtype(dtype)), "bin": b}

    return _frozen(("threshold", dtype), build)


def exact_stds(ddem: np.ndarray, groups: np.ndarray, n_groups: int) -> np.ndarray:
    """The standard deviation (ddof 0) of every group's values, summed in extended precision; NaN for an empty group."""
    flat = np.asarray(ddem).reshape(-1)
    order = np.argsort(groups, kind="stable")
    order = order[np.searchsorted(groups[order], 0):]
    bounds = np.searchsorted(groups[order], np.arange(n_groups + 1))
    out = np.full(n_groups, np.nan)
    for g in range(n_groups):
        if bounds[g + 1] > bounds[g]:
            v = flat[order[bounds[g]:bounds[g + 1]]].astype(np.longdouble)
            d = v - v.sum() / v.shape[0]
            out[g] = float(np.sqrt((d * d).sum() / v.shape[0]))
    return out


def assert_plan_matches(got_stats: dict, got_segments: tuple, got_groups: np.ndarray, oracle, ids, edges, want=None) -> tuple:
    """label_stats, segments(want_std=True) and groups of a device plan against the OraclePlan `oracle`: integers, extremes, groups and
    medians bit for bit, standard deviations within std_bound of the exactly summed one.  `want`: the oracle's (stats, segments, groups)
    where the caller has them already.  Returns them."""
    if want is None:
        want = (oracle.label_stats(), oracle.segments(ids, edges, want_std=True), oracle.groups())
    w_stats, (w_counts, w_med, _), w_groups = want
    assert sorted(got_stats) == sorted(w_stats)
    for k in w_stats:
        a, b = np.asarray(got_stats[k]), np.asarray(w_stats[k])
        assert a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True), k
    counts, med, sd = got_segments
    assert np.array_equal(got_groups, w_groups), f"{np.count_nonzero(got_groups != w_groups)} groups differ"
    assert np.array_equal(counts, w_counts)
    assert np.array_equal(med, w_med, equal_nan=True), f"{np.count_nonzero(~((med == w_med) | np.isnan(w_med)))} medians differ"
    exact = exact_stds(oracle.ddem, w_groups, counts.size).reshape(counts.shape)
    assert np.array_equal(np.isnan(sd), counts == 0) and np.array_equal(np.isnan(exact), counts == 0)
    filled = counts > 0
    excess = np.abs(sd[filled] - exact[filled]) - exact[filled] * std_bound(counts[filled])
    print(f"std: largest |sd - exact| / exact {np.max(np.abs(sd[filled] - exact[filled]) / np.maximum(exact[filled], 1e-300)):.3e}, "
          f"smallest bound {std_bound(counts[filled]).min():.3e}")
    assert np.all(excess <= 0), f"{np.count_nonzero(excess > 0)} standard deviations beyond the bound"
    return want
