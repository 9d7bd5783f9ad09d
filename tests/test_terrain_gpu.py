"""GPU parity tests of the terrain path: HIP kernel (through the C-ABI) vs the CPU oracle and the golden
vectors recorded from the reference.  Run on the MI355X box with:  pytest -m gpu"""
import os

import numpy as np
import pytest

import terrain_oracle as to
from conftest import GOLDEN
from parity import assert_parity, assert_parity_true, check_attribute, compare_true, noise_floor

pytestmark = pytest.mark.gpu

FULL = ["slope", "aspect", "hillshade", "profile_curvature", "tangential_curvature", "planform_curvature",
        "flowline_curvature", "max_curvature", "min_curvature", "topographic_position_index",
        "terrain_ruggedness_index"]
SAH_WIN = ["slope", "aspect", "hillshade", "topographic_position_index", "terrain_ruggedness_index"]


@pytest.fixture(scope="module")
def terrain():
    from xdem_amd import terrain as t

    return t


def _dem(shape, seed, dtype=np.float32):
    from xdem_amd.synth import fbm_numpy

    dem = fbm_numpy(shape, seed=seed, dtype=dtype)
    dem[5, 7] = np.nan
    dem[shape[0] // 2, 30:33] = np.nan
    dem[-1, -1] = np.nan
    return dem


@pytest.mark.parametrize("fit,cm", [("Florinsky", "geometric"), ("Florinsky", "directional"),
                                    ("ZevenbergThorne", "geometric"), ("ZevenbergThorne", "directional"),
                                    ("Horn", "geometric")])
@pytest.mark.parametrize("shape", [(301, 517), (64, 1000), (1, 1), (2, 3), (33, 256), (700, 800)])
def test_fbm_f32_all_attributes(terrain, fit, cm, shape):
    dem = _dem(shape, seed=11) if min(shape) > 8 else np.arange(shape[0] * shape[1], dtype=np.float32).reshape(shape)
    attrs = FULL if fit != "Horn" else SAH_WIN
    got = terrain.get_terrain_attribute(dem, attrs, resolution=10.0, surface_fit=fit, curv_method=cm)
    ref = to.terrain_attributes(dem, attrs, resolution=10.0, surface_fit=fit, curv_method=cm)
    for a, g, r in zip(attrs, got, ref):
        check_attribute(g, r, a, dem, 10.0, f"{fit}/{cm}/{shape}/{a}")


@pytest.mark.parametrize("kw", [
    dict(resolution=1.0, degrees=False, hillshade_altitude=10.0, hillshade_azimuth=90.0, hillshade_z_factor=10.0,
         tri_method="Wilson"),
    dict(resolution=0.25, degrees=True, hillshade_altitude=80.0, hillshade_azimuth=0.0, hillshade_z_factor=0.5),
    dict(resolution=30.0, degrees=True, hillshade_altitude=0.0, hillshade_azimuth=360.0, hillshade_z_factor=0.0),
])
def test_options(terrain, kw):
    dem = _dem((257, 300), seed=5)
    got = terrain.get_terrain_attribute(dem, FULL, **kw)
    ref = to.terrain_attributes(dem, FULL, **kw)
    for a, g, r in zip(FULL, got, ref):
        check_attribute(g, r, a, dem, kw["resolution"], f"{kw}/{a}")


def test_f64_in_out_and_mixed(terrain):
    dem = _dem((130, 140), seed=9, dtype=np.float64)
    for out_dtype in (None, np.float32):
        got = terrain.get_terrain_attribute(dem, FULL, resolution=5.0, out_dtype=out_dtype)
        ref = to.terrain_attributes(dem, FULL, resolution=5.0, out_dtype=out_dtype)
        for a, g, r in zip(FULL, got, ref):
            assert g.dtype == (np.float64 if out_dtype is None else np.float32)
            assert_parity(g, r, f"f64->{g.dtype}/{a}")
    dem32 = dem.astype(np.float32)
    got = terrain.get_terrain_attribute(dem32, FULL, resolution=5.0, out_dtype=np.float64)
    ref = to.terrain_attributes(dem32, FULL, resolution=5.0, out_dtype=np.float64)
    for a, g, r in zip(FULL, got, ref):
        assert_parity(g, r, f"f32->f64/{a}")


def test_engine_names_select_the_precision_recipe(terrain):
    """'scipy' = the default recipe (derivatives rounded to the DEM dtype); 'numba' = float64 derivatives
    (surfit.py:1044), i.e. what the float64-input path computes on the widened DEM.  Checked here against the oracle's
    float64 path on a larger raster; the reference's own numba-engine outputs are test_T11_numba_engine_... below."""
    dem = _dem((150, 300), seed=13)
    attrs = FULL + ["roughness"]
    base = terrain.get_terrain_attribute(dem, attrs, resolution=10.0)
    for g, b in zip(terrain.get_terrain_attribute(dem, attrs, resolution=10.0, engine="scipy"), base):
        assert np.array_equal(g, b, equal_nan=True)
    got = terrain.get_terrain_attribute(dem, attrs, resolution=10.0, engine="numba")
    ref = to.terrain_attributes(dem.astype(np.float64), FULL, resolution=10.0, out_dtype=np.float32)
    for a, g, r in zip(FULL, got, ref):
        assert g.dtype == np.float32
        assert_parity(g, r, f"numba-recipe/{a}")
    for i in (9, 10, 11):  # windowed indexes: unchanged
        assert np.array_equal(got[i], base[i], equal_nan=True)
    assert not np.array_equal(got[0], base[0], equal_nan=True)  # and the recipes do differ in the last digits


def test_inf_and_nan_propagation_bit_exact_mask(terrain):
    rng = np.random.default_rng(42)
    dem = rng.normal(size=(40, 300)).astype(np.float32)
    dem[4, 4:6] = np.nan
    dem[17, 16] = np.inf
    dem[10, 2] = -np.inf
    dem[20, 255:258] = np.nan  # straddles a tile boundary
    for fit in ("Florinsky", "ZevenbergThorne", "Horn"):
        attrs = FULL if fit != "Horn" else SAH_WIN
        got = terrain.get_terrain_attribute(dem, attrs, resolution=2.0, surface_fit=fit)
        ref = to.terrain_attributes(dem, attrs, resolution=2.0, surface_fit=fit)
        for a, g, r in zip(attrs, got, ref):
            assert np.array_equal(np.isnan(g), np.isnan(r)), (fit, a)
            assert np.array_equal(np.isinf(g), np.isinf(r)), (fit, a)


@pytest.mark.parametrize("w", [5, 7, 11])
def test_generic_window_sizes(terrain, w):
    dem = _dem((60, 333), seed=3)
    for tri in ("Riley", "Wilson"):
        got = terrain.get_terrain_attribute(dem, ["topographic_position_index", "terrain_ruggedness_index", "slope"],
                                            window_size=w, tri_method=tri, resolution=1.0)
        ref = to.terrain_attributes(dem, ["topographic_position_index", "terrain_ruggedness_index", "slope"],
                                    window_size=w, tri_method=tri, resolution=1.0)
        for g, r in zip(got, ref):
            assert_parity(g, r, f"w{w}/{tri}")


def test_window_lds_kernel_equals_per_pixel_kernel(terrain):
    """Round 4: windows other than 3 x 3 run the LDS-tiled kernel (window_lds_kernel: the patch of a 64 x 16 output tile staged
    once, taps from LDS, same row-major float64 accumulation).  Every plane must be BIT-IDENTICAL to the per-pixel kernel of
    rounds 1-3 (option "terrain_window_lds" = 0): all seven subsets of {TPI, TRI, roughness}, Riley and Wilson, float32 and
    float64, NaN / Inf holes, ragged shapes, row blocks with halo rows, windows up to the LDS limit and beyond it."""
    import torch

    from xdem_amd import _lib

    ctx = _lib.default_context()
    names = ["topographic_position_index", "terrain_ruggedness_index", "roughness"]
    rng = np.random.default_rng(11)
    for dtype in (np.float32, np.float64):
        dem = _dem((203, 517), seed=5).astype(dtype)
        for _ in range(25):
            dem[rng.integers(0, dem.shape[0]), rng.integers(0, dem.shape[1])] = np.nan
        dem[40:44, 100:103] = np.inf
        dem[150, 300] = -np.inf
        d = torch.from_numpy(dem).cuda()
        for w in (5, 7, 13, 31, 89, 95):          # 89: the largest window whose patch fits the LDS budget; 95: the fall-back
            for tri in ("Riley", "Wilson"):
                for sub in range(1, 8):
                    if (w > 13 or dtype == np.float64) and sub not in (1, 7):
                        continue
                    attrs = [n_ for i, n_ in enumerate(names) if sub >> i & 1]
                    res = {}
                    for lds in (1, 0):
                        try:
                            ctx.set_option("terrain_window_lds", lds)
                            full = terrain.terrain_attributes_device(d, attrs, window_size=w, tri_method=tri)
                            blk = terrain.terrain_attributes_device(d[20:190], attrs, window_size=w, tri_method=tri,
                                                                    halo_top=min(w // 2, 10), halo_bottom=min(w // 2, 3))
                            torch.cuda.synchronize()
                        finally:
                            ctx.set_option("terrain_window_lds", 1)
                        res[lds] = (full.cpu().numpy(), blk.cpu().numpy())
                    it = np.int32 if dtype == np.float32 else np.int64
                    for k in (0, 1):
                        assert np.array_equal(res[1][k].view(it), res[0][k].view(it)), (dtype, w, tri, attrs, k)


def test_golden_reference_vectors(terrain):
    """Directly against outputs recorded from the reference itself (not via the oracle)."""
    z = np.load(os.path.join(GOLDEN, "terrain_T2_f32.npz"))
    dem = z["dem"]
    groups = {}
    for key in z.files:
        if key != "dem":
            *cfg, attr = key.split("|")
            groups.setdefault(tuple(cfg), []).append(attr)
    for cfg, attrs in groups.items():
        fit, cm, deg, az, alt, zf, tri = cfg
        got = terrain.get_terrain_attribute(dem, attrs, resolution=10.0, degrees=bool(int(deg)),
                                            hillshade_azimuth=float(az), hillshade_altitude=float(alt),
                                            hillshade_z_factor=float(zf), surface_fit=fit, curv_method=cm,
                                            tri_method=tri)
        got = got if isinstance(got, list) else [got]
        for a, g in zip(attrs, got):
            check_attribute(g, z["|".join(cfg) + "|" + a], a, dem, 10.0, f"{cfg}/{a}")
    z = np.load(os.path.join(GOLDEN, "terrain_T4_int32.npz"))
    attrs = [k for k in z.files if k != "dem"]
    got = terrain.get_terrain_attribute(z["dem"], attrs, resolution=5.0)
    for a, g in zip(attrs, got):
        assert g.dtype == np.float32
        check_attribute(g, z[a], a, z["dem"].astype(np.float32), 5.0, f"int32/{a}")


def _ulp_line(c):
    return ("hist(0,1,2,3-4,5-8,>8)=" + "/".join(f"{h:.3f}" for h in c["hist"]) + f" max_ulp={c['max_ulp']} max_rel={c['max_rel']:.2e}"
            + f" excused_by_noise_floor={c['excused']:.5f}")


@pytest.mark.parametrize("fname", ["terrain_T1_float32_nan.npz", "terrain_T1_float32_inf.npz",
                                   "terrain_T1_float64_nan.npz", "terrain_T1_float64_inf.npz"])
def test_T1_reference_fixtures_on_the_hip_path(terrain, fname, record_property):
    """Every T1 array recorded from the reference (normal noise with NaN / Inf holes x 3 fits x 2 curvature methods x 3
    resolutions, float32 and float64, deprecated `curvature` included) through get_terrain_attribute on the HIP path:
    masks bit-exact, TRUE relative error <= 1e-6.  (Zero-mean noise is the worst case for bit-identity: derivative sums of
    full-width float32 values land on exact rounding ties, which the reference breaks by its float64 rounding noise.)"""
    z = np.load(os.path.join(GOLDEN, fname))
    dem = z["dem"]
    n = 0
    worst, excused = {}, {}
    for key in z.files:
        if key == "dem":
            continue
        fit, cm, res, attr = key.split("|")
        got = terrain.get_terrain_attribute(dem, attr, resolution=float(res), surface_fit=fit, curv_method=cm)
        # (T1 is noise with relief everywhere: the float64 noise floor may excuse 5 % of the differing pixels at most)
        c = assert_parity_true(got, z[key], f"{fname}:{key}", floor=noise_floor(attr, dem, float(res)), max_excused=0.05)
        w = worst.setdefault(attr, c)
        if c["max_rel"] >= w["max_rel"]:
            worst[attr] = c
        excused[attr] = max(excused.get(attr, 0.0), c["excused"])
        n += 1
    assert n > 100
    for attr, c in worst.items():
        record_property(f"T1/{fname}/{attr}", _ulp_line(c) + f" worst_excused_share_over_configs={excused[attr]:.5f}")
        print(f"T1 {fname} {attr:28s} {_ulp_line(c)} worst excused share {excused[attr]:.5f}")


def test_T3_reference_known_answers_on_the_hip_path(terrain, record_property):
    """The reference's data-free known-answer DEMs (tests/test_terrain/test_surfit.py:228-411: flat, ramps, V shapes,
    saddle, ridge, trough) with the outputs the reference itself produced, through the HIP path.  Includes the exactly
    flat Florinsky window, where the reference returns its cancellation residue (slope 2.5e-15, aspect 198.43494 deg):
    reproduced by the kernel's reference-order recomputation of exactly cancelling derivative sums."""
    z = np.load(os.path.join(GOLDEN, "terrain_T3_known_answers.npz"))
    n = 0
    exc, signal, fixtures_with_signal = {}, {}, {}
    for key in z.files:
        if key.startswith("dem|"):
            continue
        name, fit, res, attr = key.split("|")
        dem = z["dem|" + name]
        got = terrain.get_terrain_attribute(dem, attr, resolution=float(res), surface_fit=fit)
        demf = dem.astype(np.float32) if dem.dtype.kind in "iu" else dem
        # (known-answer DEMs are planar / flat by construction: their curvatures and TPI are exact zeros, so the reference's
        # float64 residues -- the noise floor's whole purpose -- can be every pixel of a fixture; the share is recorded)
        c = assert_parity_true(got, z[key], key, floor=noise_floor(attr, demf, float(res)))
        exc[attr] = max(exc.get(attr, 0.0), c["excused"])
        signal[attr] = signal.get(attr, 0) + c["n_signal"]
        fixtures_with_signal[attr] = fixtures_with_signal.get(attr, 0) + (c["n_signal"] > 0)
        n += 1
    assert n > 900
    for attr, e in exc.items():
        record_property(f"T3/{attr}/max_share_excused_by_noise_floor", f"{e:.5f}")
        record_property(f"T3/{attr}/pixels_judged_above_the_floor", f"{signal[attr]} in {fixtures_with_signal[attr]} fixtures")
        print(f"T3 {attr:28s} max share excused by the noise floor {e:.5f}; {signal[attr]} pixels in "
              f"{fixtures_with_signal[attr]} fixtures carry a reference value above the floor (judged at 1e-6)")
        # the complement of the excusal: every attribute has fixtures (V shapes, saddle, ridge, trough, ramps for the first
        # derivatives) whose reference values stand ABOVE the floor -- there a kernel that returned 0 would fail the 1e-6 bar
        assert signal[attr] >= 40 and fixtures_with_signal[attr] >= 9, (attr, signal[attr], fixtures_with_signal[attr])
    flat = terrain.get_terrain_attribute(z["dem|flat"], ["slope", "aspect"], resolution=1.0, surface_fit="Florinsky")
    assert flat[1][2, 2] == z["flat|Florinsky|1.0|aspect"][2, 2] == np.float32(198.43494)
    assert flat[0][2, 2] == z["flat|Florinsky|1.0|slope"][2, 2] and 0 < flat[0][2, 2] < 1e-12


def test_T11_numba_engine_reference_fixtures_on_the_hip_path(terrain, record_property):
    """Row a8 of SURVEY section 8.  Outputs of the reference's OWN numba-engine code (surfit.py:948-1088, 1270-1303, run through
    the identity-njit shim of oracle/_refimport.py; oracle/gen_golden.py: terrain_T11_numba) against `engine="numba"` on the HIP
    path: float64 derivatives (the float64-input kernels on the widened DEM) and the Numba engine's rule for +-Inf pixels
    (terrain_nonfinite.hip).  Masks bit-exact -- including the pixels next to an Inf value that the SciPy engine blanks and this
    engine does not (slope 90 deg, hillshade 1.5 / 181.1, `curvature` -+Inf) --, TRUE relative error <= 1e-6 elsewhere."""
    z = np.load(os.path.join(GOLDEN, "terrain_T11_numba_engine.npz"))
    n = n_inf_window_values = 0
    worst = {}
    for key in z.files:
        parts = key.split("|")
        if parts[0] in ("dem", "boundary") or len(parts) != 5 or parts[1] == "win":
            continue
        name, fit, cm, res, attr = parts
        dem = z["dem|" + name]
        got = terrain.get_terrain_attribute(dem, attr, resolution=float(res), surface_fit=fit, curv_method=cm, engine="numba")
        ref = z[key]
        c = assert_parity_true(got, ref, key, floor=noise_floor(attr, dem, float(res)), max_excused=0.05)
        if name.endswith("_inf"):
            blanked_by_scipy = to._window_invalid(dem, 5 if fit == "Florinsky" else 3)
            sel = blanked_by_scipy & ~np.isnan(ref)
            n_inf_window_values += int(sel.sum())
            if ref.dtype == np.float32:   # special values (90, 45 k, 1.5, 181.10512, 0, +-Inf): bit for bit
                assert np.array_equal(got[sel], ref[sel]), (key, got[sel], ref[sel])
        w = worst.setdefault(attr, c)
        if c["max_rel"] >= w["max_rel"]:
            worst[attr] = c
        n += 1
    assert n > 500 and n_inf_window_values > 100
    for attr, c in worst.items():
        record_property(f"T11/{attr}", _ulp_line(c))
        print(f"T11 numba engine {attr:28s} {_ulp_line(c)}")
    # ... and the option does not leak: the default engine after a numba call still blanks the Inf windows
    dem = z["dem|T1_float32_inf"]
    s = terrain.get_terrain_attribute(dem, "slope", resolution=1.0)
    assert np.array_equal(np.isnan(s), to._window_invalid(dem, 5))
    # windowed indexes under engine="numba": the float64-window evaluation, within the float32 rounding noise of the recorded one
    for key in z.files:
        parts = key.split("|")
        if len(parts) == 5 and parts[1] == "win" and parts[0] == "terrainlike_float32":
            name, _, w, tri, attr = parts
            dem = z["dem|" + name]
            got = terrain.get_terrain_attribute(dem, attr, window_size=int(w), tri_method=tri, engine="numba")
            ref = z[key]
            assert np.array_equal(np.isnan(got), np.isnan(ref)), key
            fin = np.isfinite(ref)
            tol = int(w) ** 2 * 2.0**-24 * float(np.nanmax(np.abs(dem)))
            assert np.all(np.abs(got[fin].astype(np.float64) - ref[fin]) <= tol), key


def test_numba_engine_nonfinite_rule_at_scale_and_in_row_blocks(terrain):
    """The +-Inf fix-up of engine="numba" against the oracle's numba recipe on a raster large enough for the streaming strips
    and the chunked host path (several row chunks: Inf pixels next to chunk borders), float32 and float64 outputs."""
    from xdem_amd import _lib

    rng = np.random.default_rng(5)
    dem = _dem((1500, 1100), seed=21)
    rows = rng.integers(0, 1500, 40)
    cols = rng.integers(0, 1100, 40)
    dem[rows, cols] = np.where(rng.random(40) < 0.5, np.inf, -np.inf).astype(np.float32)
    dem[0, 0] = np.inf
    dem[-1, 5] = -np.inf
    dem[700, 3:6] = np.inf   # two infinite taps of equal sign in one window
    attrs = ["slope", "aspect", "hillshade", "curvature", "profile_curvature", "max_curvature", "min_curvature"]
    ctx = _lib.default_context()
    for chunk_mb in (0, 8):
        ctx.set_option("host_chunk_mb", chunk_mb)
        try:
            for fit, cm in (("Florinsky", "geometric"), ("ZevenbergThorne", "directional")):
                for od in (np.float32, np.float64):
                    got = terrain.get_terrain_attribute(dem, attrs, resolution=10.0, surface_fit=fit, curv_method=cm,
                                                        engine="numba", out_dtype=od)
                    ref = to.terrain_attributes(dem, attrs, resolution=10.0, surface_fit=fit, curv_method=cm, engine="numba",
                                                out_dtype=od)
                    for a, g, r in zip(attrs, got, ref):
                        assert_parity_true(g, r, f"{fit}/{cm}/{od.__name__}/{a}/chunk{chunk_mb}", floor=noise_floor(a, dem, 10.0))
        finally:
            ctx.set_option("host_chunk_mb", 0)


class _FakeRaster:
    """Duck-typed geoutils.Raster (the package is absent): what xdem_amd.terrain needs of one."""
    saved = {}

    def __init__(self, data, transform=(10.0, 0, 0, 0, -10.0, 0), crs=None, nodata=None):
        self.data, self.transform, self.crs, self.nodata, self.res = data, transform, crs, nodata, (10.0, 10.0)

    @classmethod
    def from_array(cls, data, transform, crs, nodata=None):
        return cls(data, transform, crs, nodata)

    def save(self, filename):
        _FakeRaster.saved[filename] = self.data.copy()


def test_mp_config_is_the_row_chunked_host_path(terrain):
    """`mp_config` (upstream: geoutils MultiprocConfig -> tiles with overlap, terrain.py:412-466) maps onto the library's
    row-chunked host path: chunk_size rows per chunk, overlap derived from the attributes, planes bit-identical to the one-pass
    call; `outfile` goes through the Raster's own save, one file per attribute named as upstream names them; a worker cluster is
    ignored with a warning; the option does not outlive the call."""
    from types import SimpleNamespace

    from xdem_amd import _lib

    dem = _dem((700, 800), seed=17)
    ras = _FakeRaster(dem)
    attrs = ["slope", "max_curvature", "topographic_position_index", "fractal_roughness"]
    one = terrain.get_terrain_attribute(ras, attrs)
    _FakeRaster.saved.clear()
    cfg = SimpleNamespace(chunk_size=96, outfile="out/attr.tif", cluster=None)
    tiled = terrain.get_terrain_attribute(ras, attrs, mp_config=cfg)
    assert all(isinstance(t, _FakeRaster) and t.nodata == -99999 for t in tiled)
    for a, o, t in zip(attrs, one, tiled):
        assert np.array_equal(o.data, t.data, equal_nan=True), a
        assert np.array_equal(_FakeRaster.saved[f"out/attr_{a}.tif"], t.data, equal_nan=True)
    assert _lib.default_context().options.get("host_chunk_rows", 0) == 0
    # (a single attribute takes the small-set kernel, whose lean tail may differ from the 4-attribute launch in the last ulp:
    # the tiled call is held against the one-pass call of the SAME attribute set)
    single = terrain.slope(ras, mp_config=SimpleNamespace(chunk_size=64, outfile="s.tif", cluster=None))
    assert np.array_equal(single.data, terrain.slope(ras).data, equal_nan=True) and "s.tif" in _FakeRaster.saved

    class MultiprocessingCluster:
        pass

    with pytest.warns(UserWarning, match="cluster is ignored"):
        w = terrain.get_terrain_attribute(ras, "slope", mp_config=SimpleNamespace(chunk_size=128, outfile=None,
                                                                                   cluster=MultiprocessingCluster()))
    assert np.array_equal(w.data, terrain.slope(ras).data, equal_nan=True)


def test_ulp_histogram_per_attribute(terrain, record_property):
    """Per-attribute ulp histogram of the float32 kernels against the oracle on a terrain-like raster (what
    tools/ulp_report.py prints), for both tails of the specialised kernels: the lean tail (option "terrain_math" = 2, default:
    float32 scale factors, every plane within 1e-6 TRUE relative error) and the mixed tail of round 2 (0: eight planes
    bit-identical).  The raster is large enough for the streaming-strip route (interior) and the tile kernel (frame)."""
    from parity import EXACT_ATTRS_MIXED

    from xdem_amd import _lib

    ctx = _lib.default_context()
    dem = _dem((1500, 1532), seed=42)
    try:
        for tail in (2, 0):
            ctx.set_option("terrain_math", tail)
            for fit, attrs in (("Florinsky", FULL), ("ZevenbergThorne", FULL), ("Horn", SAH_WIN)):
                got = terrain.get_terrain_attribute(dem, attrs, resolution=10.0, surface_fit=fit)
                ref = to.terrain_attributes(dem, attrs, resolution=10.0, surface_fit=fit)
                for a, g, r in zip(attrs, got, ref):
                    c = check_attribute(g, r, a, dem, 10.0, f"tail {tail} {fit}/{a}", exact_attrs=EXACT_ATTRS_MIXED if tail == 0 else None)
                    record_property(f"tail{tail}/{fit}/{a}", _ulp_line(c))
                    print(f"tail {tail} {fit:16s} {a:28s} {_ulp_line(c)}")
    finally:
        ctx.set_option("terrain_math", 2)


def test_halo_rows_equal_full_raster(terrain):
    """Row-block call with halo rows reproduces the corresponding rows of the full-raster result (multi-GPU contract)."""
    import torch

    dem = _dem((200, 300), seed=21)
    full = terrain.get_terrain_attribute(dem, FULL, resolution=10.0)
    d = torch.from_numpy(dem).cuda()
    r0, r1, depth = 64, 150, 2
    out = terrain.terrain_attributes_device(d[r0 - depth:r1 + depth], FULL, resolution=10.0, halo_top=depth,
                                            halo_bottom=depth)
    torch.cuda.synchronize()
    for i, f in enumerate(full):
        assert np.array_equal(out[i].cpu().numpy(), f[r0:r1], equal_nan=True)


def test_fresh_scattered_ranges_hold_what_the_kernel_wrote(terrain):
    """Round 4: plane ranges that are allocated, freed (not pooled) and allocated again, with other ranges and torch blocks coming
    and going in between.  A range that was re-reserved at the address of a freed one used to be read and written through
    translations of the previous mapping (profiles/r04_vmm_stale_probe.txt: tens of MiB of other memory's contents in 6 of 14
    repeats at 46400^2); the library keeps freed ranges reserved since.  Every pixel of every repeat against the same launch
    into torch planes."""
    import gc

    import torch

    from xdem_amd import _lib
    from xdem_amd.synth import fbm_torch

    ctx = _lib.default_context()
    n = 23000
    attrs, kw = ["roughness", "topographic_position_index"], {"window_size": 5}
    dem = fbm_torch(n, n, "cuda", seed=9)
    ref = torch.empty((2, n, n), device="cuda")
    terrain.terrain_attributes_device(dem, attrs, resolution=10.0, out=ref, **kw)
    torch.cuda.synchronize()
    rng = np.random.default_rng(4)
    seen = set()
    for it in range(10):
        junk = [terrain.alloc_planes(int(k), 6144, 6144, backing="scattered") for k in rng.integers(1, 10, 3)]
        tj = [torch.empty(int(m) << 20, device="cuda") for m in rng.integers(64, 1024, 3)]
        for j in junk:
            j.fill_(float(it))
        del junk, tj
        gc.collect()
        ctx.release_pool()          # (the ranges really go back: the next allocation maps new pieces)
        if it % 3 == 2:
            torch.cuda.empty_cache()
        out = terrain.alloc_planes(2, n, n, backing="scattered")
        terrain.terrain_attributes_device(dem, attrs, resolution=10.0, out=out, **kw)
        torch.cuda.synchronize()
        bad = int((out.view(torch.int32) != ref.view(torch.int32)).sum())
        assert bad == 0, (it, bad, hex(out.data_ptr()), out.data_ptr() in seen)
        seen.add(out.data_ptr())
        del out
        gc.collect()
        ctx.release_pool()


@pytest.mark.parametrize("backing", ["contiguous", "chunked", "scattered", "recycled"])
def test_library_allocated_planes(terrain, backing):
    """xdemhip_device_alloc / terrain.alloc_planes(backing=...): resident planes on the library's own allocations (physically
    contiguous, chunked virtual range, recycled).  Same results as on torch's own memory, the memory goes back when the tensor
    dies, and a size nobody can provide fails loudly."""
    import gc

    import torch

    from xdem_amd import _lib
    from xdem_amd.synth import fbm_torch

    ctx = _lib.default_context()
    attrs = ["slope", "aspect", "hillshade", "profile_curvature", "topographic_position_index", "terrain_ruggedness_index"]
    n = 4608
    dem = fbm_torch(n, n, "cuda", seed=3)
    torch.cuda.synchronize()
    gc.collect()
    ctx.release_pool()
    torch.cuda.empty_cache()   # (blocks cached by earlier tests would be handed back later and blur the accounting below)
    free0 = torch.cuda.mem_get_info()[0]
    planes = terrain.alloc_planes(len(attrs), n, n, torch.float32, ctx, backing=backing)
    assert planes.shape == (len(attrs), n, n) and planes.is_cuda and hasattr(planes, "xdem_contiguous")
    assert torch.cuda.mem_get_info()[0] <= free0 - planes.numel() * 4 + (64 << 20)
    got = terrain.terrain_attributes_device(dem, attrs, resolution=10.0, out=planes, ctx=ctx)
    ref = terrain.terrain_attributes_device(dem, attrs, resolution=10.0, out=torch.empty_like(planes), ctx=ctx)
    torch.cuda.synchronize()
    assert got.data_ptr() == planes.data_ptr()
    assert torch.equal(got.view(torch.int32), ref.view(torch.int32))
    view = planes[2, 100:200]          # a view keeps the allocation alive
    del planes, got
    gc.collect()
    assert torch.equal(view.view(torch.int32), ref[2, 100:200].view(torch.int32))
    del view, ref
    gc.collect()
    torch.cuda.empty_cache()
    if backing == "scattered":
        # a released scattered range waits in the context's pool for the next request of its size ...
        assert torch.cuda.mem_get_info()[0] < free0 - (400 << 20)
        again = terrain.alloc_planes(len(attrs), n, n, torch.float32, ctx, backing=backing)
        assert torch.cuda.mem_get_info()[0] <= free0 - again.numel() * 4 + (64 << 20)   # ... which takes it instead of a new one
        del again
        gc.collect()
        ctx.release_pool()   # ... and goes back to the driver on request
    assert torch.cuda.mem_get_info()[0] >= free0 - (64 << 20)
    assert not hasattr(terrain.alloc_planes(2, 64, 64, torch.float32, ctx), "xdem_contiguous")   # small sets: torch's allocator
    assert hasattr(terrain.alloc_planes(4, n, n, torch.float32, ctx), "xdem_contiguous")          # 340 MB: the library's scattered backing
    assert hasattr(terrain.terrain_attributes_device(dem, attrs[:4], resolution=10.0, ctx=ctx), "xdem_contiguous")   # out=None: the same
    gc.collect()
    ctx.release_pool()
    with pytest.raises(_lib.XdemHipError):
        ctx.device_tensor((1 << 40,), "float32")   # 4 TiB


# the small sets and the directional full set: one kernel family each, at the smallest raster that streams (8 x 8 interior tiles)
# and one column narrower, where the plan falls back to tiles
STREAM_SMALL = {"FULL_DIR": FULL, "SLOPE": ["slope"], "SLOPE_ASPECT": ["slope", "aspect"], "HILLSHADE": ["hillshade"],
                "SAH": ["slope", "aspect", "hillshade"]}


@pytest.mark.parametrize("fit,attrs", [("Florinsky", "FULL"), ("ZevenbergThorne", "FULL"), ("Horn", "SAH_WIN"),
                                       ("Florinsky", "FULL_DIR"), ("ZevenbergThorne", "FULL_DIR"), ("Horn", "SLOPE"),
                                       ("ZevenbergThorne", "SLOPE_ASPECT"), ("Florinsky", "HILLSHADE"), ("Florinsky", "SAH")])
def test_streaming_strips_equal_tile_kernel_and_oracle(terrain, fit, attrs):
    """The streaming route of the specialised kernels (raster interior by wave-autonomous 64-column strips fed by LDS-DMA,
    frame of edge tiles by the tile kernel; context option "terrain_stream") runs the very same per-pixel code as the tile
    kernel: planes must be BIT-IDENTICAL with the route switched off, for every band height, with NaN / Inf holes straddling
    strip, band and ring-block boundaries, for row blocks with halo rows (the multi-GPU call) and for shapes whose last band
    and frame are ragged; and equal to the oracle like every other configuration.  Every kernel family that has strips is
    here: the full sets with either curvature method, Horn's five planes and the four small sets."""
    import torch

    from xdem_amd import _lib

    kw = dict(resolution=10.0, surface_fit=fit, curv_method="directional" if attrs == "FULL_DIR" else "geometric")
    shapes = ((9 * 32 + 2, 9 * 256 + 4), (9 * 32 + 2, 9 * 256 + 3)) if attrs in STREAM_SMALL else ((1400, 2600), (2309, 1801), (1153, 4100))
    attrs = STREAM_SMALL.get(attrs) or (FULL if attrs == "FULL" else SAH_WIN)
    ctx = _lib.default_context()
    rng = np.random.default_rng(7)
    for shape in shapes:
        dem = _dem(shape, seed=shape[0])
        # holes: single pixels, a block across a 64-column strip border and a 128-row band border, +-Inf, a whole row piece
        for _ in range(40):
            dem[rng.integers(0, shape[0]), rng.integers(0, shape[1])] = np.nan
        dem[30:36, 310:330] = np.nan
        dem[158:163, 572:580] = np.nan
        dem[287:290, 255:258] = np.inf
        dem[min(600, shape[0] - 90), 700:900] = np.nan
        dem[shape[0] - 40, shape[1] - 300] = -np.inf
        d = torch.from_numpy(dem).cuda()
        ref_planes = None
        try:
            for stream in (0, 1, 128, 256, 512):
                ctx.set_option("terrain_stream", stream)
                out = terrain.terrain_attributes_device(d, attrs, **kw)
                torch.cuda.synchronize()
                got = out.cpu().numpy()
                if stream == 0:
                    ref_planes = got
                else:
                    for i, a in enumerate(attrs):
                        assert np.array_equal(got[i], ref_planes[i], equal_nan=True), (shape, stream, a)
            # strip-to-workgroup orders (0 XCD bands, 1 natural, 2 permuted, 3 column-major) and the conservative form of the
            # ring wait (vmcnt(0) instead of the counted wait: the counted form may never read a stale ring row)
            ctx.set_option("terrain_stream", 1)
            for order, wait in ((1, 0), (2, 0), (3, 0), (0, 1)):
                try:
                    ctx.set_option("terrain_order", order)
                    ctx.set_option("terrain_ring_wait", wait)
                    got = terrain.terrain_attributes_device(d, attrs, **kw)
                    torch.cuda.synchronize()
                    got = got.cpu().numpy()
                finally:
                    ctx.set_option("terrain_order", 0)
                    ctx.set_option("terrain_ring_wait", 0)
                for i, a in enumerate(attrs):
                    assert np.array_equal(got[i], ref_planes[i], equal_nan=True), (shape, "order", order, "wait", wait, a)
            # row block with halo rows: rows [r0, r1) of the raster from a buffer holding depth rows either side
            r0, r1, depth = 96, shape[0] - 70, 2
            blk = terrain.terrain_attributes_device(d[r0 - depth:r1 + depth], attrs, **kw,
                                                    halo_top=depth, halo_bottom=depth)
            top = terrain.terrain_attributes_device(d[:r1 + depth], attrs, **kw, halo_bottom=depth)
            torch.cuda.synchronize()
            for i, a in enumerate(attrs):
                assert np.array_equal(blk[i].cpu().numpy(), ref_planes[i][r0:r1], equal_nan=True), (shape, "block", a)
                assert np.array_equal(top[i].cpu().numpy(), ref_planes[i][:r1], equal_nan=True), (shape, "top block", a)
        finally:
            ctx.set_option("terrain_stream", 1)
        if shape == shapes[0]:
            ref = to.terrain_attributes(dem, attrs, **kw)
            for a, g, r in zip(attrs, ref_planes, ref):
                check_attribute(g, r, a, dem, 10.0, f"{fit}/{a}")


def test_large_properties_16384(terrain):
    """BASELINE config[1] size: size-independent properties instead of an oracle run."""
    import torch

    from xdem_amd.synth import fbm_torch

    n = 16384
    dem = fbm_torch(n, n, "cuda", seed=42)
    out = terrain.terrain_attributes_device(dem, FULL, resolution=10.0)
    torch.cuda.synchronize()
    # (1) NaN only on the 2-pixel Florinsky border (no nodata in the synthetic DEM); TPI/TRI: 1-pixel border
    inner = out[:9, 2:-2, 2:-2]
    assert bool(torch.isfinite(inner).all())
    assert bool(torch.isnan(out[:9, :2, :]).all()) and bool(torch.isnan(out[:9, :, -2:]).all())
    assert bool(torch.isfinite(out[9:, 1:-1, 1:-1]).all()) and bool(torch.isnan(out[9:, 0, :]).all())
    # (2) ranges: slope in [0,90), aspect in [0,360], hillshade in [0,255], TRI >= 0, max >= min curvature
    assert float(inner[0].min()) >= 0 and float(inner[0].max()) < 90
    assert float(inner[1].min()) >= 0 and float(inner[1].max()) <= 360
    assert float(inner[2].min()) >= 0 and float(inner[2].max()) <= 255
    assert float(out[10, 1:-1, 1:-1].min()) >= 0
    assert bool((inner[7] >= inner[8]).all())
    # (3) translation equivariance: a shifted crop gives bit-identical interior values
    crop = dem[4096:4096 + 1024, 8192:8192 + 1536].contiguous()
    out_c = terrain.terrain_attributes_device(crop, FULL, resolution=10.0)
    torch.cuda.synchronize()
    a_, b_ = out_c[:, 2:-2, 2:-2], out[:, 4098:4096 + 1022, 8194:8192 + 1534]
    neq = (a_.view(torch.int32) != b_.view(torch.int32))
    assert not bool(neq.any()), (int(neq.sum()), neq.sum(dim=(1, 2)).tolist(), neq.nonzero()[:8].tolist())
    # (4) a random sample of rows agrees with the oracle
    sub = dem[5000:5064, 3000:3400].cpu().numpy()
    ref = to.terrain_attributes(sub, FULL, resolution=10.0)
    for i, r in enumerate(ref):
        g = out[i, 5002:5062, 3002:3398].cpu().numpy()
        check_attribute(g, r[2:-2, 2:-2], FULL[i], sub, 10.0, FULL[i])


def test_raster_beyond_2g_pixels(terrain):
    """46400^2 = 2.15e9 pixels: element offsets of the lower tiles exceed 2^31 (a sign-extended 32-bit half of the
    tile origin once sent those stores out of bounds).  Crops from the bottom rows must match the whole-raster planes."""
    import torch

    from xdem_amd.synth import fbm_torch

    n = 46400
    attrs = ["slope", "max_curvature", "terrain_ruggedness_index"]
    dem = fbm_torch(n, n, "cuda", seed=7)
    out = terrain.terrain_attributes_device(dem, attrs, resolution=10.0)
    torch.cuda.synchronize()
    for (r, c) in ((n - 700, n - 1000), (n - 300, 5), (46341, 20000), (23170, 23000)):
        r1, c1 = min(r + 300, n), min(c + 700, n)
        oc = terrain.terrain_attributes_device(dem[r:r1, c:c1].contiguous(), attrs, resolution=10.0)
        torch.cuda.synchronize()
        a_ = oc[:, 2:-2, 2:-2].view(torch.int32)
        b_ = out[:, r + 2:r1 - 2, c + 2:c1 - 2].view(torch.int32)
        assert torch.equal(a_, b_), (r, c)
    assert bool(torch.isfinite(out[0, 2:-2, 2:-2]).all())
    del out
    # the other window kernels (rugosity, fractal roughness w=13, generic 5x5 roughness) address pixels the same way
    for attrs, kw, m in ((["rugosity", "fractal_roughness"], {}, 6), (["roughness", "topographic_position_index"], {"window_size": 5}, 2)):
        out = terrain.terrain_attributes_device(dem, attrs, resolution=10.0, **kw)
        for (r, c) in ((n - 300, n - 700), (46341, 20000)):
            r1, c1 = min(r + 300, n), min(c + 700, n)
            oc = terrain.terrain_attributes_device(dem[r:r1, c:c1].contiguous(), attrs, resolution=10.0, **kw)
            torch.cuda.synchronize()
            a_ = oc[:, m:-m, m:-m].view(torch.int32)
            b_ = out[:, r + m:r1 - m, c + m:c1 - m].view(torch.int32)
            neq = a_ != b_
            if bool(neq.any()):   # which side is off?  a second whole-raster launch and the context's state go into the message
                from xdem_amd import _lib
                ctx = _lib.default_context()
                out2 = terrain.terrain_attributes_device(dem, attrs, resolution=10.0, **kw)
                torch.cuda.synchronize()
                b2 = out2[:, r + m:r1 - m, c + m:c1 - m].view(torch.int32)
                info = {"whole2 == whole": bool(torch.equal(b2, b_)), "whole2 == crop": bool(torch.equal(b2, a_)),
                        "pool": [(b, f) for b, f, _ in ctx._pool], "options": dict(ctx.options), "ptr whole": out.data_ptr(), "ptr whole2": out2.data_ptr()}
                raise AssertionError((attrs, r, c, int(neq.sum()), neq.sum(dim=(1, 2)).tolist(), neq.nonzero()[:3].tolist(), neq.nonzero()[-3:].tolist(), info))
        del out


@pytest.mark.parametrize("w", [3, 5])
def test_roughness_next_row_f2(terrain, w):
    """SURVEY 8f-2 (first windowed index beyond TPI/TRI): max - min of the window, NaN if any NaN."""
    dem = _dem((90, 300), seed=13)
    dem[40, 100] = np.inf
    attrs = ["roughness", "topographic_position_index", "slope"]
    got = terrain.get_terrain_attribute(dem, attrs, window_size=w, resolution=2.0)
    ref = to.terrain_attributes(dem, attrs, window_size=w, resolution=2.0)
    assert np.array_equal(got[0], ref[0], equal_nan=True)  # pure selection: bit-exact
    for g, r in zip(got[1:], ref[1:]):
        assert_parity(g, r, f"w{w}")
    assert np.array_equal(terrain.roughness(dem, window_size=w), ref[0], equal_nan=True)
    z = np.load(os.path.join(GOLDEN, "terrain_T5_windows.npz"))
    key = f"dem|{w}|Riley|roughness"
    assert np.array_equal(terrain.roughness(z["dem"], window_size=w), z[key], equal_nan=True)  # reference's own output


def test_C1_dem_slope_plumbing_horn():
    """BASELINE config[0]: ~700x800 float32 DEM, slope + aspect (Horn) through the DEM object API (the Longyearbyen
    file itself needs network access; a synthetic raster of that size stands in)."""
    import xdem_amd
    from xdem_amd.synth import fbm_numpy

    arr = fbm_numpy((700, 800), seed=1, mean=400.0, std=150.0)
    arr[:20, :30] = -9999.0
    dem = xdem_amd.DEM.from_array(arr, transform=(20.0, 0.0, 502810.0, 0.0, -20.0, 8674030.0), crs="EPSG:25833", nodata=-9999.0)
    assert dem.res == (20.0, 20.0) and np.isnan(dem.data[0, 0])
    slope = dem.slope(surface_fit="Horn")
    aspect = dem.aspect(surface_fit="Horn", degrees=False)
    assert isinstance(slope, xdem_amd.DEM) and slope.transform == dem.transform and slope.crs == dem.crs and slope.nodata == -99999
    ref_s, = to.terrain_attributes(dem.data, ["slope"], resolution=20.0, surface_fit="Horn")
    ref_a, = to.terrain_attributes(dem.data, ["aspect"], resolution=1.0, surface_fit="Horn", degrees=False)
    check_attribute(slope.data, ref_s, "slope", dem.data, 20.0, "DEM.slope")
    check_attribute(aspect.data, ref_a, "aspect", dem.data, 1.0, "DEM.aspect")
    both = dem.get_terrain_attribute(["slope", "aspect"], surface_fit="Horn")
    assert np.array_equal(both[0].data, slope.data, equal_nan=True) and len(both) == 2
    aligned = dem.coregister_3d(xdem_amd.DEM.from_array(arr + 1.0, dem.transform, dem.crs, nodata=-9998.0))
    assert isinstance(aligned, xdem_amd.DEM) and abs(np.nanmedian(aligned.data - dem.data) - 1.0) < 0.05


# ---- rugosity and fractal roughness (csrc/window_extra.hip) -------------------------------------------
def _ulp_f(a, b):
    return np.abs(a.astype(np.float64) - b.astype(np.float64)) / np.spacing(np.abs(b)).astype(np.float64)


def test_T9_golden_rugosity_fractal():
    """Fixtures recorded from the reference (oracle/gen_golden.py: terrain_T9).  Rugosity bit-exact (same float32 /
    float64 operations in the same order); fractal roughness within 1e-6 relative (float32 log, see window_extra.hip)."""
    from xdem_amd import terrain as t

    z = np.load(os.path.join(GOLDEN, "terrain_T9_rugosity_fractal.npz"))
    n = 0
    for key in z.files:
        if key.startswith("dem|"):
            continue
        parts = key.split("|")
        if parts[0] == "pyramid":
            dem, (attr, par) = z[f"dem|pyramid|{parts[1]}"], parts[2:]
        else:
            dem, (attr, par) = z[f"dem|{parts[0]}"], parts[1:]
        ref = z[key]
        if attr == "rugosity":
            got = t.rugosity(dem, resolution=float(par))
            assert got.dtype == ref.dtype and np.array_equal(got, ref, equal_nan=True), key
        else:
            import warnings

            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                got = t.fractal_roughness(dem, window_size_fractal=int(par))
            assert got.dtype == ref.dtype and np.array_equal(np.isnan(got), np.isnan(ref)), key
            assert np.array_equal(np.isinf(got), np.isinf(ref)), key
            ok = np.isfinite(ref)
            assert np.all(np.abs(got[ok] - ref[ok]) <= 1e-6 * np.abs(ref[ok])), key
        n += 1
    assert n >= 25
    # known answers of tests/test_terrain/test_window.py:21-89 through the product path
    jen = np.array([[190, 170, 155], [183, 165, 145], [175, 160, 122]], dtype="float32")
    assert t.rugosity(jen, resolution=100.0)[1, 1] == pytest.approx(10280.48 / 10000.0, rel=1e-4)
    for dem, d in ((z["dem|line"], 1.0), (z["dem|plane"], 2.0), (z["dem|cube"], 3.0)):
        assert np.round(t.fractal_roughness(dem)[6, 6], 3) == d


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_rugosity_fractal_vs_oracle_larger(dtype):
    """300 x 517 terrain-like DEM with NaN / Inf holes, all windowed indexes in one call (two engine launches)."""
    from xdem_amd import terrain as t

    rng = np.random.default_rng(21)
    dem = (500.0 + np.cumsum(np.cumsum(rng.normal(scale=0.4, size=(300, 517)), axis=0), axis=1)).astype(dtype)
    dem[40, 100:104] = np.nan
    dem[200, 300] = np.inf
    dem[299, 0] = -np.inf
    attrs = ["fractal_roughness", "rugosity", "roughness", "slope"]
    got = t.get_terrain_attribute(dem, attrs, resolution=5.0)
    ref = to.terrain_attributes(dem, attrs, resolution=5.0)
    assert np.array_equal(got[1], ref[1], equal_nan=True)          # rugosity: bit-exact
    assert np.array_equal(got[2], ref[2], equal_nan=True)
    # fractal roughness: the shared 1e-6 scaled metric (NumPy's float32 log is not correctly rounded and the
    # regression amplifies its last-bit differences ~5x); most pixels are still bit-identical
    assert np.isfinite(ref[0]).sum() > 100000
    assert_parity(got[0], ref[0], "fractal_roughness", min_exact=0.85 if dtype == np.float32 else 0.5)
    for w in (5, 7, 21, 49):
        import warnings

        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            g = t.fractal_roughness(dem[:120, :150], window_size_fractal=w)
        r = to.terrain_attributes(dem[:120, :150], ["fractal_roughness"], window_size_fractal=w)[0]
        assert_parity(g, r, f"fractal_roughness w={w}")


def test_rugosity_fractal_device_row_blocks():
    """Device-resident entry with halo rows: a split raster reproduces the single-launch result bit for bit."""
    import torch
    from xdem_amd.terrain import terrain_attributes_device

    rng = np.random.default_rng(5)
    dem = torch.from_numpy(rng.uniform(0, 30, size=(200, 333)).astype(np.float32)).cuda()
    attrs = ["rugosity", "fractal_roughness"]
    full = terrain_attributes_device(dem, attrs, resolution=2.0)
    top = terrain_attributes_device(dem[:106], attrs, resolution=2.0, halo_bottom=6)
    bot = terrain_attributes_device(dem[94:], attrs, resolution=2.0, halo_top=6)
    torch.cuda.synchronize()
    assert torch.equal(torch.cat([top, bot], dim=1).view(torch.int32), full.view(torch.int32))


# ---- texture shading (csrc/texture.hip: hipFFT + pad / filter / crop kernels) ----------------------------------
def _tex_err(got, ref):
    ok = np.isfinite(ref)
    assert np.array_equal(np.isnan(got), np.isnan(ref)) and got.dtype == ref.dtype
    if not ok.any():
        return 0.0
    return float(np.abs(got[ok].astype(np.float64) - ref[ok]).max() / max(np.abs(ref[ok]).max(), 1e-30))


def test_T10_texture_shading_vs_reference():
    """Reference outputs (tests/golden/terrain_T10_texture.npz).  Two different FFT libraries in the DEM's own precision:
    float32 transforms carry the rounding noise of the ~1e3 m input, i.e. ~1e-6 of the output scale (the reference's own
    result has that noise): tolerance 1e-5 of the output maximum for float32, 1e-12 for float64."""
    from xdem_amd import terrain as t

    z = np.load(os.path.join(GOLDEN, "terrain_T10_texture.npz"))
    worst = {}
    for key in z.files:
        if key.startswith("dem|"):
            continue
        name, alpha = key.split("|")
        got = t.texture_shading(z[f"dem|{name}"], alpha=float(alpha))
        e = _tex_err(got, z[key])
        worst[key] = e
        tol = 1e-12 if z[key].dtype == np.float64 else 1e-5  # measured: 1e-14 / 2.5e-6 of the output maximum
        assert e <= tol, (key, e)
    assert np.all(t.texture_shading(z["dem|flat"]) == 0)
    with pytest.raises(ValueError, match="Alpha must be between 0 and 2"):
        t.texture_shading(z["dem|flat"], alpha=2.1)
    print(worst)


def test_texture_shading_properties_large():
    """2000 x 3000 float32 DEM (FFT lengths 2000 x 3000 are 7-smooth): oracle comparison + the reference's invariants
    (tests/test_terrain/test_freq.py:84-160): offset invariance for alpha > 0, linear scaling, all-attribute call."""
    from xdem_amd import terrain as t
    from xdem_amd.synth import fbm_numpy

    dem = fbm_numpy((2000, 3000), seed=12)
    dem[100:110, 200:260] = np.nan
    got = t.texture_shading(dem, alpha=0.8)
    ref = to.terrain_attributes(dem, ["texture_shading"])[0]
    e32 = _tex_err(got, ref)
    assert e32 <= 5e-5, e32
    got64 = t.texture_shading(dem.astype(np.float64), alpha=0.8)
    ref64 = to.terrain_attributes(dem.astype(np.float64), ["texture_shading"])[0]
    assert _tex_err(got64, ref64) <= 1e-12
    ok = np.isfinite(got64)
    off = t.texture_shading(dem.astype(np.float64) + 1234.5, alpha=0.8)
    assert np.abs(off[ok] - got64[ok]).max() <= 1e-8 * np.abs(got64[ok]).max()
    sc = t.texture_shading(dem.astype(np.float64) * 3.0, alpha=0.8)
    assert np.abs(sc[ok] - 3.0 * got64[ok]).max() <= 1e-9 * np.abs(got64[ok]).max()
    both = t.get_terrain_attribute(dem, ["texture_shading", "slope", "fractal_roughness"], resolution=10.0)
    assert np.array_equal(both[0], got, equal_nan=True) and both[1].shape == dem.shape


def test_randomised_configurations_vs_oracle():
    """Seeded sweep over what the fixed grids above do not enumerate: random attribute subsets in random order (runtime-mask
    kernels, plane ordering), odd raster shapes down to 1 x N, both dtypes, all fits / curvature methods, random resolutions,
    hillshade settings, TRI methods, window sizes, NaN / Inf holes -- every output against the oracle with the shared metric."""
    from xdem_amd import terrain as t

    rng = np.random.default_rng(20260926)
    surf = ["slope", "aspect", "hillshade", "curvature", "profile_curvature", "tangential_curvature", "planform_curvature",
            "flowline_curvature", "max_curvature", "min_curvature"]
    win = ["topographic_position_index", "terrain_ruggedness_index", "roughness", "rugosity"]
    n_checked = 0
    for trial in range(160):
        H, W = int(rng.integers(1, 90)), int(rng.integers(1, 300))
        dtype = rng.choice([np.float32, np.float64])
        kind = rng.integers(0, 3)
        if kind == 0:
            dem = rng.normal(1500, 200, (H, W))
        elif kind == 1:
            dem = 300 + np.cumsum(np.cumsum(rng.normal(0, 0.3, (H, W)), 0), 1)
        else:
            dem = np.round(rng.uniform(0, 40, (H, W)))  # ties, flats
        dem = dem.astype(dtype)
        for _ in range(int(rng.integers(0, 4))):
            dem[rng.integers(0, H), rng.integers(0, W)] = rng.choice([np.nan, np.inf, -np.inf])
        fit = str(rng.choice(["Horn", "ZevenbergThorne", "Florinsky"]))
        pool = (surf[:3] if fit == "Horn" else surf) + win
        k = int(rng.integers(1, len(pool) + 1))
        attrs = [str(a) for a in rng.choice(pool, size=k, replace=False)]
        kw = dict(resolution=float(rng.choice([0.25, 1.0, 7.5, 30.0])), surface_fit=fit,
                  curv_method=str(rng.choice(["geometric", "directional"])), degrees=bool(rng.integers(0, 2)),
                  hillshade_altitude=float(rng.uniform(0, 90)), hillshade_azimuth=float(rng.uniform(0, 360)),
                  hillshade_z_factor=float(rng.choice([1.0, 0.5, 3.0])), tri_method=str(rng.choice(["Riley", "Wilson"])),
                  window_size=int(rng.choice([3, 3, 5, 7])))
        import warnings

        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            got = t.get_terrain_attribute(dem, attrs, **kw)
            ref = to.terrain_attributes(dem, attrs, **kw)
        got = got if isinstance(got, list) else [got]
        # (Round 1 excluded pixels whose derivative sums cancel exactly -- integer-valued DEMs -- because the reference returns
        # its ~1e-15 rounding residue there and hence an arbitrary aspect; the kernel now recomputes such sums in the
        # reference's own order, so they are compared like everything else: TRUE relative error.)
        for a, g, r in zip(attrs, got, ref):
            if a in ("rugosity", "roughness"):
                assert np.array_equal(g, r, equal_nan=True), (trial, a, kw, dem.shape, dtype)
            else:
                assert_parity_true(g, r, f"trial {trial} {a} {fit} {dem.shape} {np.dtype(dtype).name} {kw}",
                                   floor=noise_floor(a, dem, kw["resolution"]))
            n_checked += 1
    assert n_checked > 800


def test_device_views_strided_and_misaligned():
    """Device entry on tensor VIEWS: a column window of a wider tensor (row stride > width, base pointer not 16-byte aligned:
    the scalar tile-load path instead of the float4 one) and a row window; results equal those of the contiguous copy."""
    import torch
    from xdem_amd.terrain import terrain_attributes_device

    g = torch.Generator(device="cuda").manual_seed(3)
    big = (1000 + 50 * torch.randn((700, 1500), generator=g, device="cuda")).cumsum(0).cumsum(1) * 1e-3 + 500
    big[100, 333] = float("nan")
    for (r0, r1, c0, c1) in ((0, 700, 0, 1500), (5, 650, 3, 1290), (17, 400, 64, 1001), (1, 3, 1, 9)):
        view = big[r0:r1, c0:c1]
        assert view.stride(1) == 1 and (view.stride(0) != view.shape[1] or (r0, c0) == (0, 0))
        a = terrain_attributes_device(view, FULL, resolution=10.0)
        b = terrain_attributes_device(view.contiguous(), FULL, resolution=10.0)
        torch.cuda.synchronize()
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (r0, r1, c0, c1)


def test_host_path_row_chunks_equal_single_pass():
    """Host-buffer calls stream the raster through the GPU in row chunks with overlap (bounded device memory for rasters of any
    size): with a chunk budget of 1 MiB (dozens of chunks) every attribute family gives bit-identical results to one pass."""
    from xdem_amd import _lib
    from xdem_amd import terrain as t

    rng = np.random.default_rng(77)
    dem = (800 + np.cumsum(np.cumsum(rng.normal(0, 0.3, (700, 900)), 0), 1)).astype(np.float32)
    dem[300:303, 500] = np.nan
    ctx = _lib.default_context()
    configs = [
        (FULL + ["roughness", "rugosity"], dict(resolution=10.0)),
        (["slope", "max_curvature", "topographic_position_index", "terrain_ruggedness_index", "roughness"],
         dict(resolution=5.0, surface_fit="ZevenbergThorne", window_size=7)),
        (["slope", "aspect", "hillshade"], dict(resolution=2.0, surface_fit="Horn")),
        (["fractal_roughness", "texture_shading", "slope"], dict(resolution=10.0)),
    ]
    import warnings

    for attrs, kw in configs:
        ctx.set_option("host_chunk_mb", 0)
        want = t.get_terrain_attribute(dem, attrs, **kw)
        try:
            ctx.set_option("host_chunk_mb", 1)
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                got = t.get_terrain_attribute(dem, attrs, **kw)
        finally:
            ctx.set_option("host_chunk_mb", 0)
        for a, g, w in zip(attrs, got, want):
            assert np.array_equal(g.view(np.int32), w.view(np.int32)), (a, kw)
    # options "host_copy_threads" (copy threads / streams of the PCIe legs: 1, 3, the default 8) and "host_release" (the pinned
    # staging buffers are freed and come back with the next call): neither may change a bit of the result
    attrs, kw = configs[0]
    want = t.get_terrain_attribute(dem, attrs, **kw)
    try:
        for nthreads in (1, 3, 0):
            ctx.set_option("host_copy_threads", nthreads)
            ctx.set_option("host_chunk_mb", 1 if nthreads == 3 else 0)
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                got = t.get_terrain_attribute(dem, attrs, **kw)
            for a, g, w in zip(attrs, got, want):
                assert np.array_equal(g.view(np.int32), w.view(np.int32)), (a, nthreads)
            ctx.set_option("host_release", 1)
        with pytest.raises(_lib.XdemHipError):
            ctx.set_option("host_copy_threads", 17)
    finally:
        ctx.set_option("host_copy_threads", 0)
        ctx.set_option("host_chunk_mb", 0)


def test_c4_size_on_one_gpu_crops_equal_full():
    """BASELINE.json configs[3]'s raster size (65536^2: 4.3e9 pixels > 2^32, 17 GB in, 189 GB out) through the fused kernel on
    ONE GPU, so that the size the 8-GPU configuration partitions is exercised by the suite: crops computed separately must
    be bit-identical to the same windows of the whole-raster planes (translation equivariance of every attribute), including
    windows beyond pixel offset 2^32 and at the raster's far corner."""
    import torch

    from xdem_amd.terrain import terrain_attributes_device

    n = 65536
    dev = torch.device("cuda", 0)
    torch.cuda.empty_cache()  # (blocks cached by earlier tests of the session count as used otherwise)
    free, _ = torch.cuda.mem_get_info(dev)
    if free < 225 * 2**30:
        pytest.skip(f"needs 225 GiB of free device memory, {free / 2**30:.0f} GiB free")
    attrs = ["slope", "aspect", "hillshade", "profile_curvature", "tangential_curvature", "planform_curvature",
             "flowline_curvature", "max_curvature", "min_curvature", "topographic_position_index", "terrain_ruggedness_index"]
    r = torch.arange(n, device=dev, dtype=torch.float32)[:, None]
    c = torch.arange(n, device=dev, dtype=torch.float32)[None, :]
    dem = torch.empty((n, n), device=dev, dtype=torch.float32)
    for i in range(0, n, 4096):
        rr = r[i:i + 4096]
        dem[i:i + 4096] = 1000.0 + 30.0 * torch.sin(rr * 0.013) * torch.cos(c * 0.011) + 0.002 * rr + 5.0 * torch.sin(c * 0.21 + rr * 0.17)
    dem[50000:50003, 60000:60010] = float("nan")
    out = terrain_attributes_device(dem, attrs, resolution=10.0)
    torch.cuda.synchronize()
    assert out.shape == (11, n, n)
    for (r0, c0) in ((0, 0), (n - 600, n - 900), (n // 2 + 13, 7), (49800, 59500), (65536 - 601, 123)):
        r1, c1 = min(r0 + 600, n), min(c0 + 900, n)
        crop = terrain_attributes_device(dem[r0:r1, c0:c1].contiguous(), attrs, resolution=10.0)
        torch.cuda.synchronize()
        # the crop's own 2-pixel rim sees the raster edge rule instead of neighbours: compare interiors, NaN patterns included
        a = crop[:, 2:-2, 2:-2].contiguous().view(torch.int32)
        b = out[:, r0 + 2:r1 - 2, c0 + 2:c1 - 2].contiguous().view(torch.int32)
        assert torch.equal(a, b), (r0, c0)
    assert bool(torch.isnan(out[0, 50001, 60005])) and bool(torch.isfinite(out[0, 40000, 61000]))
    del out, dem
    torch.cuda.empty_cache()


def test_alloc_planes_with_a_probe_keeps_one_of_the_candidates(terrain):
    """terrain.alloc_planes(backing="auto", probe=...): the candidates (scattered, ordinary, in turn: three to eight) are probed with the caller's own
    launch and the fastest is returned -- whichever it is, the planes it holds after a launch are the ordinary call's bit for bit, the
    calibration log names every candidate, and without a probe nothing is calibrated."""
    import torch

    from xdem_amd import _lib

    ctx = _lib.default_context()
    n = 4608
    attrs = ["slope", "aspect", "hillshade", "max_curvature"]
    dem = torch.from_numpy((1000 + np.cumsum(np.cumsum(np.random.default_rng(3).normal(scale=0.2, size=(n, n)), 0), 1)).astype(np.float32)).cuda()
    calls = []

    def probe(planes):
        calls.append(planes.data_ptr())
        terrain.terrain_attributes_device(dem, attrs, out=planes, resolution=10.0)

    planes = terrain.alloc_planes(len(attrs), n, n, torch.float32, ctx, backing="auto", probe=probe)
    log = planes._xdem_calibration_ms
    assert planes._xdem_backing in ("scattered", "torch") and 3 <= len(log) <= 8 and [k for k, _ in log] == (["scattered", "torch"] * 4)[:len(log)]
    assert len(calls) == 5 * len(log) and planes.data_ptr() in calls and all(ms > 0 for _, ms in log)
    ordered = sorted(ms for _, ms in log)
    assert len(log) == 8 or ordered[1] <= 1.03 * ordered[0]          # stopped because a second candidate confirmed the fastest, or ran out
    kept = [ms for k, ms in log if k == planes._xdem_backing]
    assert min(kept) <= 1.0101 * min(ms for _, ms in log)          # the fastest candidate, up to the 1 % that favours the incumbent
    terrain.terrain_attributes_device(dem, attrs, out=planes, resolution=10.0)
    want = terrain.terrain_attributes_device(dem, attrs, resolution=10.0)
    torch.cuda.synchronize()
    assert torch.equal(torch.nan_to_num(planes, nan=-1e30), torch.nan_to_num(want, nan=-1e30))
    plain = terrain.alloc_planes(len(attrs), n, n, torch.float32, ctx, backing="auto")
    assert not hasattr(plain, "_xdem_calibration_ms")


def test_retired_measurement_switches_are_refused_and_leave_the_context_usable(terrain):
    """The four switches of the retired measurement builds ("terrain_store", "terrain_rows", "terrain_sync", "vario_deff") are
    names the library no longer knows: the binding's set_option (which now routes them to xdemhip_set_option) raises, the
    test-switch entry point refuses them too, and the refusals leave the context as it was -- the slope plane of a 64 x 96
    float32 raster is the same before and after, bit for bit."""
    from xdem_amd import _lib

    ctx = _lib.default_context()
    dem = _dem((64, 96), seed=3)
    before = terrain.get_terrain_attribute(dem, "slope", resolution=10.0)
    for name in ("terrain_store", "terrain_rows", "terrain_sync", "vario_deff"):
        assert name not in ctx.TEST_SWITCHES
        with pytest.raises(_lib.XdemHipError):
            ctx.set_option(name, 1)
        assert name not in ctx.options
        assert ctx._L.xdemhip_set_test_switch(ctx.handle, name.encode(), 1) != 0
    after = terrain.get_terrain_attribute(dem, "slope", resolution=10.0)
    assert np.isfinite(after).any() and np.array_equal(before, after, equal_nan=True)
