"""Host-side contract of ``xdem_amd.coreg.BlockwiseCoreg`` (no GPU): the constructor's checks, the tiling, ``_ransac`` against the values
recorded from the reference's own (tests/golden/blockwise_golden.npz, tools/gen_golden_blockwise.py), the reference's signatures, the
oracle's warp against upstream's formulation, and the attributes / ``meta`` of a fit with the CPU oracle in the device plan's place."""
import inspect
import json
import os
import warnings

import numpy as np
import pytest

import blockwise_cases as bc
import blockwise_oracle as bo
from conftest import GOLDEN

SIG = json.load(open(os.path.join(GOLDEN, "signatures_blockwise.json")))["coreg"]


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "blockwise_golden.npz"))


class _Cfg:
    outfile = "aligned_dem.tif"
    chunk_size = 500


def test_constructor_checks_and_messages():
    from xdem_amd import coreg

    with pytest.raises(ValueError, match="Only one of the parameters 'mp_config' or 'parent_path' may be specified."):
        coreg.BlockwiseCoreg(coreg.NuthKaab(), mp_config=_Cfg(), parent_path="out")
    # neither: accepted here (no raster I/O), and each alone
    assert coreg.BlockwiseCoreg(coreg.NuthKaab()).mp_config is None
    cfg = _Cfg()
    assert coreg.BlockwiseCoreg(coreg.NuthKaab(), mp_config=cfg).mp_config is cfg
    b = coreg.BlockwiseCoreg(coreg.NuthKaab(vertical_shift=False), parent_path="out", block_size_fit=64, block_size_apply=128)
    assert (b.parent_path, b.block_size_fit, b.block_size_apply, b.apply_z_correction) == ("out", 64, 128, False)
    assert not os.path.exists("out")   # nothing is written
    assert b.meta == {"inputs": {}, "outputs": {}} and b.shape_tiling_grid == (0, 0, 0)
    assert coreg.BlockwiseCoreg(coreg.VerticalShift()).apply_z_correction is True
    with pytest.raises(ValueError, match=r"The 'step' argument must be an instantiated Coreg subclass. Hint: write e.g. ICP\(\) instead of ICP"):
        coreg.BlockwiseCoreg(coreg.ICP)
    with pytest.raises(ValueError, match="The blockwise coregistration only supports affine coregistration methods."):
        coreg.BlockwiseCoreg(coreg.Deramp())
    # the oddly worded check of blockwise.py:87-91: a step whose only_translation is False is the one refused
    with pytest.raises(ValueError, match="The provided coregistration method is configured to only estimate translation. "
                                         "Consider setting 'only_translation' to True to allow for more complex transformations."):
        coreg.BlockwiseCoreg(coreg.ICP())
    coreg.BlockwiseCoreg(coreg.ICP(only_translation=True))
    with pytest.raises(AssertionError, match="fit"):
        coreg.BlockwiseCoreg(coreg.NuthKaab()).apply(np.zeros((4, 4), dtype=np.float32), resolution=10.0)


@pytest.mark.parametrize("shape,block,rows,cols", [
    ((70, 100), 32, [(0, 32), (32, 70)], [(0, 32), (32, 64), (64, 100)]),
    ((64, 64), 64, [(0, 64)], [(0, 64)]),
    ((10, 200), 32, [(0, 10)], [(0, 32), (32, 64), (64, 96), (96, 128), (128, 160), (160, 200)]),
    ((33, 33), 32, [(0, 33)], [(0, 33)]),
    ((48, 49), 32, [(0, 48)], [(0, 32), (32, 49)]),   # a remainder of exactly half a block merges, one above it does not
])
def test_tiling_grid(shape, block, rows, cols):
    from xdem_amd import coreg

    g = coreg.tiling_grid(shape, block)
    assert g.shape == (len(rows), len(cols), 4) and g.dtype == np.int64
    for i, (r0, r1) in enumerate(rows):
        for j, (c0, c1) in enumerate(cols):
            assert tuple(g[i, j]) == (r0, r1, c0, c1)
    assert np.array_equal(g, bo.tiling_grid(shape, block))


@pytest.mark.parametrize("case", ["planar", "allnan", "onerow", "onecol", "onetile"])
def test_ransac_returns_what_the_reference_returned(golden, case):
    """Bit for bit: the polyfit branches are deterministic, and with exactly planar inliers the RANSAC fit does not depend on the draws
    (``planar_seed_spread`` is 0 over 8 seeds of the reference run); the global seed is set as the generator set it."""
    from xdem_amd import coreg

    assert float(golden["planar_seed_spread"]) == 0.0
    np.random.seed(0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = coreg.BlockwiseCoreg._ransac(golden[f"{case}_x"], golden[f"{case}_y"], golden[f"{case}_shifts"], 0.01, 2000)
    assert np.array_equal(np.array([float(v) for v in got]), golden[f"{case}_coeff"])


def test_ransac_refuses_an_empty_set():
    from xdem_amd import coreg

    with pytest.raises(ValueError, match="No valid points after removing NaNs."):
        coreg.BlockwiseCoreg._ransac(np.array([1.0, np.nan]), np.array([np.nan, 2.0]), np.array([0.5, 0.25]))


@pytest.mark.parametrize("name", sorted(SIG))
def test_reference_parameters_are_mirrored(name):
    """Every parameter of the reference, in its order, with its default (``fit`` / ``apply`` add keyword-only ``transform`` / ``resolution``)."""
    from xdem_amd import coreg

    cls, meth = name.split(".")
    mine = inspect.signature(getattr(getattr(coreg, cls), meth)).parameters
    names = list(mine)
    pos = -1
    for rec in SIG[name]:
        assert rec["name"] in names, f"{name}: parameter '{rec['name']}' of the reference is missing"
        assert mine[rec["name"]].kind.name == rec["kind"]
        assert names.index(rec["name"]) > pos, f"{name}: '{rec['name']}' is out of the reference's order"
        pos = names.index(rec["name"])
        mine_default = "<required>" if mine[rec["name"]].default is inspect.Parameter.empty else mine[rec["name"]].default
        assert mine_default == rec["default"], (name, rec["name"])
    extra = [n for n in names if n not in [r["name"] for r in SIG[name]]]
    assert all(mine[n].kind is inspect.Parameter.KEYWORD_ONLY for n in extra), extra


@pytest.mark.parametrize("H,W", bc.WARP_SHAPES)
@pytest.mark.parametrize("field", range(len(bc.WARP_FIELDS)))
def test_inverse_map_warp_stays_within_the_twist_of_upstreams_gridding(H, W, field):
    """Bilinear interpolation differs from a linear interpolant on either diagonal of the cell by at most a quarter of the cell's twist
    |a00 - a01 - a10 + a11|: on every pixel farther than ceil(max |shift| / res) + 2 from the border both are finite and the oracle's
    warp lies within twist / 4 + 1e-9 |z| of forward map + griddata."""
    cx, cy, cz = bc.WARP_FIELDS[field]
    dem = bc.warp_dem(H, W, np.float64, nans=False)
    t6 = bc.transform6(H)
    mine = bo.apply(dem, t6, cx, cy, cz, 0)
    theirs = bo.apply_forward_griddata(dem, t6, cx, cy, cz)
    x, y = bc.grid_xy(H, W)
    shift = max(np.abs(cx[0] * x + cx[1] * y + cx[2]).max(), np.abs(cy[0] * x + cy[1] * y + cy[2]).max())
    m = int(np.ceil(shift / bc.RES)) + 2
    inner = np.zeros((H, W), dtype=bool)
    inner[m:H - m, m:W - m] = True
    assert inner.sum() > 0.2 * H * W
    assert np.isfinite(mine[inner]).all() and np.isfinite(theirs[inner]).all()
    bound = bo.twist_bound(dem, t6, cx, cy) + 1e-9 * np.abs(theirs)
    excess = (np.abs(mine - theirs) - bound)[inner]
    print(f"{H}x{W} field {field}: margin {m}, largest excess over the bound {excess.max():.3e}, largest difference {np.abs(mine - theirs)[inner].max():.3e}")
    assert excess.max() <= 0.0


@pytest.fixture
def oracle_plan(monkeypatch):
    """``BWPlan`` replaced by the CPU oracle for the test."""
    from xdem_amd import blockwise

    bo.OraclePlan.nan_rule = None
    monkeypatch.setattr(blockwise, "BWPlan", bo.OraclePlan)
    return bo.OraclePlan


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_fit_records_upstreams_attributes_and_meta(oracle_plan, dtype):
    from xdem_amd import coreg

    H, W, block = bc.CASES["A"]
    ref, tba = bc.fit_case(H, W, dtype)
    ref[:32, :32] = np.nan                       # a tile whose reference is entirely invalid
    inlier = np.ones((H, W), dtype=bool)
    inlier[32:, 64:] = False                     # a tile emptied by the mask
    step = coreg.NuthKaab()
    b = coreg.BlockwiseCoreg(step, block_size_fit=block)
    t6 = bc.transform6(H)
    assert b.fit(ref, tba, inlier, transform=t6) is None
    assert b.fit_route == "batched"
    assert b.shape_tiling_grid == (2, 3, 4)
    assert b.meta["inputs"] is step.meta["inputs"]
    assert list(b.meta["outputs"]) == ["0_0", "0_1", "0_2", "1_0", "1_1", "1_2"]
    # centres: (col0 + block / 2, row0 + block / 2) * transform, the BLOCK size also for the merged tiles
    assert np.array_equal(b.x_coords, bc.RES * (np.array([0, 32, 64, 0, 32, 64]) + 16.0))
    assert np.array_equal(b.y_coords, bc.RES * H - bc.RES * (np.array([0, 0, 0, 32, 32, 32]) + 16.0))
    want = bo.fit_tiles(ref, tba, inlier, block, (bc.RES, bc.RES))
    nan = np.isnan(want["shift_x"])
    assert list(nan) == [True, False, False, False, False, True]
    for k, arr in (("shift_x", b.shifts_x), ("shift_y", b.shifts_y), ("shift_z", b.shifts_z)):
        assert arr.shape == (6,) and np.array_equal(np.isnan(arr), nan)
        bar = bc.BAR_Z if k == "shift_z" else bc.BAR_PX * bc.RES
        dev = np.nanmax(np.abs(arr - want[k]))
        print(f"{np.dtype(dtype).name} {k}: deviation from the oracle {dev:.3e}")
        assert dev <= bar
        for t, key in enumerate(b.meta["outputs"]):
            assert set(b.meta["outputs"][key]) == {"shift_x", "shift_y", "shift_z"}
            assert np.array_equal(b.meta["outputs"][key][k], arr[t], equal_nan=True)
    assert np.array_equal(b.n_iterations, want["n_iterations"])
    # the planes of apply: finite coefficients from the four tiles that fit
    np.random.seed(0)
    cx, cy, cz = b.coefficients()
    assert np.isfinite([*cx, *cy, *cz]).all()
    b2 = coreg.BlockwiseCoreg(coreg.NuthKaab(vertical_shift=False), block_size_fit=block)
    b2.fit(ref, tba, inlier, resolution=bc.RES)
    assert b2.coefficients()[2] == (0, 0, 0) and np.all(b2.shifts_z[~nan] == 0.0)
    assert np.array_equal(b2.y_coords, -bc.RES * (np.array([0, 0, 0, 32, 32, 32]) + 16.0))   # resolution alone: the upper left corner is the origin


def test_route_eligibility_is_decided_from_the_step():
    from xdem_amd import coreg

    def cand(step):
        return coreg.BlockwiseCoreg(step)._batched_candidate()

    assert cand(coreg.NuthKaab()) and cand(coreg.NuthKaab(subsample=1)) and cand(coreg.NuthKaab(bin_sizes=128, bin_statistic=np.median))
    assert not cand(coreg.NuthKaab(bin_before_fit=False))
    assert not cand(coreg.NuthKaab(bin_statistic=np.nanmean))
    assert not cand(coreg.NuthKaab(bin_sizes=129))
    assert not cand(coreg.NuthKaab(bin_sizes=np.linspace(0, 6.3, 10)))
    assert not cand(coreg.NuthKaab(subsample=0.5))
    assert not cand(coreg.NuthKaab(initial_shift=(1.0, 2.0)))
    assert not cand(coreg.VerticalShift()) and not cand(coreg.DhMinimize())


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_single_tile_case_crosses_the_lds_limit_of_the_segment_sort(dtype):
    """tests/test_blockwise_gpu.py::test_segments_on_both_sides_of_the_default_lds_limit: 150 x 200 as one tile in 6 aspect bins has
    segments on both sides of BW_SEG_LDS = 4096 (csrc/blockwise.hip), all past half of it."""
    ref, tba = bc.fit_case(150, 200, np.dtype(dtype).type)
    tiles = bo.tiling_grid(ref.shape, 256).reshape(-1, 4)
    assert tiles.tolist() == [[0, 150, 0, 200]]
    (w,) = bo.step_tiles(ref, tba, None, tiles, np.ones(1, dtype=np.uint8), np.zeros(1), np.zeros(1), (bc.RES, bc.RES), 6)
    counts = w["counts"]
    assert counts.tolist() == [4640, 3828, 3919, 4902, 3795, 3927]   # (at zero offsets under the decided NaN rule, either dtype)
    assert counts.max() > 4096 >= counts.min() > 2048
