"""Block-wise coregistration on the MI355X: the batched per-tile Nuth-Kaab step (csrc/blockwise.hip) against the CPU oracle run on
each tile's slices, whole fits against the oracle and against the loop route, the warp of ``apply`` bit for bit, and the chain end to
end.  Shapes: case A = 70 x 100 in blocks of 32 (2 x 3 tiles, merged remainders, one tile that runs all 10 iterations, one with an
empty aspect bin), case B = 150 x 200 in blocks of 64 (several workgroups per tile); references are computed once per module."""
import ctypes
import functools

import numpy as np
import pytest

import blockwise_cases as bc
import blockwise_oracle as bo
from conftest import decided

pytestmark = pytest.mark.gpu

RES2 = (bc.RES, bc.RES)
KEYS = ("vshift", "n_valid", "y_mean", "y_std", "edges", "counts", "medians")


@pytest.fixture(scope="module")
def mods():
    from xdem_amd import _lib, blockwise, coreg

    return _lib, blockwise, coreg


@functools.lru_cache(maxsize=None)
def _case(name: str, dtype_name: str):
    H, W, block = bc.CASES[name]
    ref, tba = bc.fit_case(H, W, np.dtype(dtype_name).type)
    for a in (ref, tba):
        a.setflags(write=False)
    return ref, tba, block


@functools.lru_cache(maxsize=None)
def _variant(kind: str, dtype_name: str):
    """Case A with a tile whose reference is all NaN ("refnan"), a tile emptied by the inlier mask ("masked"); a single-tile raster."""
    ref, tba, block = _case("A", dtype_name)
    ref, tba, inlier = ref.copy(), tba.copy(), None
    if kind == "refnan":
        ref[:32, 32:64] = np.nan
    elif kind == "masked":
        inlier = np.ones(ref.shape, dtype=bool)
        inlier[32:, :32] = False
        inlier[5:9, 70:80] = False
    elif kind == "single":
        ref, tba = np.ascontiguousarray(ref[:20, :25]), np.ascontiguousarray(tba[:20, :25])
    return ref, tba, inlier, block


@functools.lru_cache(maxsize=None)
def _oracle_fit(kind: str, dtype_name: str):
    if kind in bc.CASES:
        ref, tba, block = _case(kind, dtype_name)
        inlier = None
    else:
        ref, tba, inlier, block = _variant(kind, dtype_name)
    return bo.fit_tiles(ref, tba, inlier, block, RES2)   # (nan_rule None: the decided convention, as the product's default)


def _moments_close(a_mean, a_std, y):
    """The bar of tests/test_nuthkaab_gpu.py::_moments_close for the plain route, against float64 mean / std of the oracle's y."""
    m, s = y.mean(), y.std()
    tol = 1e-10 * abs(s) + 1e-11 * abs(m) + 1e-13
    return abs(a_mean - m) <= tol and abs(a_std - s) <= tol


def _offsets(n):
    """Per-tile offsets that differ between tiles: zero, whole pixels, fractions, both signs."""
    sx = np.array([0.0, 10.0, 3.7, -12.5, 20.0, -4.2, 6.6, -10.0])[:n]
    sy = np.array([0.0, -10.0, 1.3, 5.0, 0.0, -7.7, 20.0, 2.5])[:n]
    return sx, sy


def _check_step(blockwise, ref, tba, inlier, block, rule, active, n_bins=72, at_zero=False):
    tiles = bo.tiling_grid(ref.shape, block).reshape(-1, 4)
    n = tiles.shape[0]
    sx, sy = (np.zeros(n), np.zeros(n)) if at_zero else _offsets(n)
    with blockwise.BWPlan(ref, tba, inlier, tiles) as plan:
        assert np.array_equal(plan.n_valid, bo.OraclePlan(ref, tba, inlier, tiles).n_valid)
        aspects = None
        if ref.dtype == np.float64:
            # the device's float64 arctangent may differ from libm's in the last bit (tests/test_nuthkaab_gpu.py::test_step_matches_oracle):
            # the aspect planes agree within 4 ulp and the oracle's step goes on, bit for bit, with the device's own
            aspects = []
            for (r0, r1, c0, c1), (st_d, asp_d, valid_d) in zip(tiles, plan.aux()):
                st_o, asp_o, valid_o = bo.tile_valid(ref[r0:r1, c0:c1], tba[r0:r1, c0:c1], None if inlier is None else inlier[r0:r1, c0:c1])
                assert np.array_equal(st_d, st_o, equal_nan=True) and np.array_equal(valid_d, valid_o)
                assert np.array_equal(np.isnan(asp_d), np.isnan(asp_o))
                assert np.all(np.abs(asp_d - asp_o)[np.isfinite(asp_o)] <= 4 * np.spacing(6.3))
                aspects.append(asp_d)
        out = plan.new_results(n_bins)
        sentinel = {"vshift": -7.0, "n_valid": -3, "y_mean": -5.0, "y_std": -6.0, "edges": -1.0, "counts": -2, "medians": -4.0}
        for k in KEYS:
            out[k][...] = sentinel[k]
        plan.step(active, sx, sy, RES2, n_bins, out)
    want = bo.step_tiles(ref, tba, inlier, tiles, active, sx, sy, RES2, n_bins, rule, aspects)
    for t in range(n):
        if not active[t]:   # untouched
            assert all(np.all(out[k][t] == sentinel[k]) for k in KEYS), t
            continue
        w = want[t]
        if w is None:       # no finite dh left: a count of 0
            assert out["n_valid"][t] == 0 and np.isnan(out["vshift"][t]) and not out["counts"][t].any() and np.isnan(out["medians"][t]).all(), t
            continue
        assert out["n_valid"][t] == w["n_valid"], t
        assert out["vshift"][t] == w["vshift"], (t, out["vshift"][t], w["vshift"])
        assert np.array_equal(out["edges"][t], w["edges"].astype(np.float64)), t
        assert np.array_equal(out["counts"][t], w["counts"]), t
        assert np.array_equal(out["medians"][t], w["medians"], equal_nan=True), t
        assert _moments_close(out["y_mean"][t], out["y_std"][t], w["y"]), (t, out["y_mean"][t], w["y"].mean(), out["y_std"][t], w["y"].std())
    return out, want


@pytest.mark.parametrize("rule", [0, 1, 2, 3])
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("name", ["A", "B"])
def test_one_batched_step_is_the_oracles_step_of_every_tile(mods, name, dtype, rule):
    _lib, blockwise, _ = mods
    ref, tba, block = _case(name, dtype)
    active = np.array([1, 1, 1, 1, 0, 1], dtype=np.uint8)
    with _lib.default_context().option_scope("nk_nan_rule", rule):
        _check_step(blockwise, ref, tba, None, block, rule, active)
        if name == "A" and rule != 1:   # the first step of a fit: at zero offsets a tile of the case has an empty aspect bin (rule 1 keeps the last row / column: none)
            _, want = _check_step(blockwise, ref, tba, None, block, rule, np.ones(6, dtype=np.uint8), at_zero=True)
            assert any((w["counts"] == 0).any() for w in want)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("kind", ["refnan", "masked", "single"])
def test_batched_step_on_empty_masked_and_single_tiles(mods, kind, dtype):
    _lib, blockwise, _ = mods
    ref, tba, inlier, block = _variant(kind, dtype)
    n = bo.tiling_grid(ref.shape, block).reshape(-1, 4).shape[0]
    assert n == (1 if kind == "single" else 6)
    rule = decided("nk_nan_rule")
    _check_step(blockwise, ref, tba, inlier, block, rule, np.ones(n, dtype=np.uint8))
    _check_step(blockwise, ref, tba, inlier, block, rule, np.ones(n, dtype=np.uint8), n_bins=5)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_long_segments_take_the_radix_selection(mods, dtype):
    """With the LDS limit lowered to 20 values most (tile, bin) segments of case B (16 to 144 values) are selected by radix passes over
    their slice of global memory: the same medians."""
    _lib, blockwise, _ = mods
    ref, tba, block = _case("B", dtype)
    ctx = _lib.default_context()
    with ctx.option_scope("bw_seg_lds", 20):
        out, want = _check_step(blockwise, ref, tba, None, block, decided("nk_nan_rule"), np.ones(6, dtype=np.uint8))
    assert max(int(w["counts"].max()) for w in want) > 20 > min(int(w["counts"].min()) for w in want)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_segments_on_both_sides_of_the_default_lds_limit(mods, dtype):
    """150 x 200 as ONE tile in 6 aspect bins, no switch set: segments of 3795 to 4902 values, so some are sorted in LDS filled past half
    of BW_SEG_LDS = 4096 keys and some are longer than it and take the radix selection over global memory at the limit the product
    runs with (tests/test_blockwise_host.py checks the counts without a GPU)."""
    _lib, blockwise, _ = mods
    ref, tba, _ = _case("B", dtype)
    assert bo.tiling_grid(ref.shape, 256).reshape(-1, 4).shape[0] == 1
    assert _lib.default_context().options.get("bw_seg_lds", 0) == 0
    _, want = _check_step(blockwise, ref, tba, None, 256, decided("nk_nan_rule"), np.ones(1, dtype=np.uint8), n_bins=6)
    counts = want[0]["counts"]
    assert counts.max() > 4096 >= counts.min() > 2048


def _deviation(b, want):
    h = max(np.nanmax(np.abs(b.shifts_x - want["shift_x"])), np.nanmax(np.abs(b.shifts_y - want["shift_y"]))) / bc.RES
    return h, np.nanmax(np.abs(b.shifts_z - want["shift_z"]))


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("kind", ["A", "B", "refnan", "masked", "single"])
def test_whole_fit_follows_the_oracle_tile_by_tile(mods, kind, dtype):
    """Per tile the same number of iterations, the oracle's NaN tiles, final offsets within 4 x the measured deviation
    (tests/blockwise_cases.py: MEASURED)."""
    _, blockwise, coreg = mods
    if kind in bc.CASES:
        ref, tba, block = _case(kind, dtype)
        inlier = None
    else:
        ref, tba, inlier, block = _variant(kind, dtype)
    want = _oracle_fit(kind, dtype)
    b = coreg.BlockwiseCoreg(coreg.NuthKaab(), block_size_fit=block)
    b.fit(ref, tba, inlier, transform=bc.transform6(ref.shape[0]))
    assert b.fit_route == "batched"
    nan = np.isnan(want["shift_x"])
    assert nan.sum() == (1 if kind in ("refnan", "masked") else 0)
    for arr in (b.shifts_x, b.shifts_y, b.shifts_z):
        assert np.array_equal(np.isnan(arr), nan)
    h, z = _deviation(b, want)
    print(f"{kind} {dtype}: iterations {list(b.n_iterations)} / {list(want['n_iterations'])}, deviation px {h:.3e}, vertical {z:.3e}")
    assert np.array_equal(b.n_iterations, want["n_iterations"])
    if kind == "A":
        assert want["n_iterations"].max() == 10   # one tile runs out of iterations while the others are frozen
    assert h <= bc.BAR_PX and z <= bc.BAR_Z


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("name", ["A", "B"])
def test_batched_route_agrees_with_the_loop_route(mods, monkeypatch, name, dtype):
    """Both on the GPU: the same keys, the same NaN tiles, offsets within the bar; host and device inputs give the same bits, and so do
    two runs."""
    import torch

    _, blockwise, coreg = mods
    ref, tba, block = _case(name, dtype)
    ref = ref.copy()
    ref[:block, :block] = np.nan   # one tile without a fit
    t6 = bc.transform6(ref.shape[0])

    def run(r, t):
        b = coreg.BlockwiseCoreg(coreg.NuthKaab(), block_size_fit=block)
        b.fit(r, t, transform=t6)
        return b

    batched = run(ref, tba)
    again = run(ref, tba)
    device = run(torch.from_numpy(ref).cuda(), torch.from_numpy(np.array(tba)).cuda())
    monkeypatch.setattr(blockwise, "BATCHED_DEFAULT", False)
    loop = run(ref, tba)
    loop_device = run(torch.from_numpy(ref).cuda(), torch.from_numpy(np.array(tba)).cuda())
    assert (batched.fit_route, device.fit_route, loop.fit_route, loop_device.fit_route) == ("batched", "batched", "loop", "loop")
    # (the loop route's NKPlan sums its moments of y with float64 atomics, whose last bits depend on the order of the additions: two loop
    #  runs agree within the bar, not to the bit)
    assert np.array_equal(np.isnan(loop.shifts_x), np.isnan(loop_device.shifts_x))
    h, z = _deviation(loop_device, {"shift_x": loop.shifts_x, "shift_y": loop.shifts_y, "shift_z": loop.shifts_z})
    assert h <= bc.BAR_PX and z <= bc.BAR_Z
    assert list(batched.meta["outputs"]) == list(loop.meta["outputs"])
    for k in ("shifts_x", "shifts_y", "shifts_z", "x_coords", "y_coords"):
        assert np.array_equal(getattr(batched, k), getattr(again, k), equal_nan=True), k
        assert np.array_equal(getattr(batched, k), getattr(device, k), equal_nan=True), k
    assert np.array_equal(np.isnan(batched.shifts_x), np.isnan(loop.shifts_x)) and np.isnan(loop.shifts_x).sum() == 1
    h, z = _deviation(batched, {"shift_x": loop.shifts_x, "shift_y": loop.shifts_y, "shift_z": loop.shifts_z})
    print(f"{name} {dtype}: batched against loop, deviation px {h:.3e}, vertical {z:.3e}")
    assert h <= bc.BAR_PX and z <= bc.BAR_Z


@pytest.mark.parametrize("rule", [0, 2])
@pytest.mark.parametrize("nans", [False, True])
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("H,W", bc.WARP_SHAPES)
def test_warp_is_the_oracles_inverse_map_bit_for_bit(mods, H, W, dtype, nans, rule):
    _lib, blockwise, _ = mods
    dem = bc.warp_dem(H, W, np.dtype(dtype).type, nans)
    t6 = bc.transform6(H)
    with _lib.default_context().option_scope("nk_nan_rule", rule):
        for cx, cy, cz in bc.WARP_FIELDS:      # (the second has coeff_z zero, the third no gradients in x / y)
            got = blockwise.warp_affine_field(dem, t6, cx, cy, cz)
            want = bo.apply(dem, t6, cx, cy, cz, rule)
            assert got.dtype == dem.dtype and np.array_equal(got, want, equal_nan=True), (cx, cy, cz, np.nanmax(np.abs(got - want)))
            assert np.isfinite(want).sum() > 0.5 * H * W


def test_warp_accepts_device_tensors_and_refuses_a_singular_field(mods):
    import torch

    _lib, blockwise, _ = mods
    dem = bc.warp_dem(61, 83, np.float32, True)
    t6 = bc.transform6(61)
    cx, cy, cz = bc.WARP_FIELDS[0]
    host = blockwise.warp_affine_field(dem, t6, cx, cy, cz)
    dev = blockwise.warp_affine_field(torch.from_numpy(dem).cuda(), t6, cx, cy, cz)
    assert np.array_equal(dev.cpu().numpy(), host, equal_nan=True)
    with pytest.raises(ValueError, match="singular"):
        blockwise.warp_affine_field(dem, t6, (-1.0, 0.0, 3.0), cy, cz)
    with pytest.raises(ValueError, match="singular"):
        blockwise.warp_affine_field(dem, t6, (1.0, 2.0, 0.0), (1.0, 0.0, 0.0), cz)   # I + A = [[2, 2], [1, 1]]
    # the library's own check, reached without the Python one
    ctx = _lib.default_context()
    dp = ctypes.POINTER(ctypes.c_double)
    out = np.empty_like(dem)
    arrs = [np.array(v, dtype=np.float64) for v in (t6, (-1.0, 0.0, 3.0), cy, cz)]
    rc = ctx._L.xdemhip_bw_apply(ctx.handle, dem.ctypes.data, _lib.F32, 61, 83, *(a.ctypes.data_as(dp) for a in arrs), out.ctypes.data, _lib.HOST)
    assert rc != _lib.OK and b"singular" in ctx._L.xdemhip_last_error(ctx.handle)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_fit_then_apply_follows_the_oracle_chain(mods, dtype):
    """Case B under ``np.random.seed(0)``: device fit -> ``_ransac`` -> device warp against ``fit_tiles`` -> the same ``_ransac`` (pinned to
    the reference's by tests/test_blockwise_host.py) -> the oracle's warp.

    Propagation of the offsets' bar.  Both chains draw the same minimal samples (same seed); where they end with the same inlier set S
    (asserted, from scikit-learn's own ``inlier_mask_``) each plane is the least-squares fit of S, which is LINEAR in the shifts: the
    plane's value at (x, y) is ``w(x, y) . s`` with ``w = [x y 1] pinv([X_S 1])``, so two shift vectors at most eps apart give planes at
    most ``g eps`` apart, ``g = max sum |w|`` over the raster.  A pre-image solves ``p + s(p) = p'``: it moves by ``M^-1`` times the
    change of the field, at most ``dp = |M^-1|_inf g eps_h`` per axis.  The bilinear interpolant changes by at most the cell's largest
    first difference per pixel of movement along each axis, s_z by ``g eps_z`` plus its gradient times dp, and the rounding of the two
    outputs to the raster dtype adds an ulp of the largest elevation each.  NaN may differ only where a pre-image lies within dp of a
    cell border."""
    from sklearn.linear_model import LinearRegression, RANSACRegressor

    _, blockwise, coreg = mods
    ref, tba, block = _case("B", dtype)
    H, W = ref.shape
    t6 = bc.transform6(H)
    b = coreg.BlockwiseCoreg(coreg.NuthKaab(), block_size_fit=block)
    b.fit(ref, tba, transform=t6)
    np.random.seed(0)
    got, t_out = b.apply(tba, transform=t6)
    assert t_out is t6 and got.dtype == tba.dtype and got.shape == tba.shape
    np.random.seed(0)
    dev_coeff = b.coefficients()
    want_fit = _oracle_fit("B", dtype)
    np.random.seed(0)
    coeff = [coreg.BlockwiseCoreg._ransac(b.x_coords, b.y_coords, want_fit[k]) for k in ("shift_x", "shift_y", "shift_z")]
    want = bo.apply(np.array(tba), t6, *coeff, decided("nk_nan_rule"))

    X = np.column_stack([b.x_coords, b.y_coords])
    x, y = bc.grid_xy(H, W)
    def inlier_sets(shifts):   # (the three fits in the order and from the seed of `coefficients`)
        np.random.seed(0)
        return [RANSACRegressor(estimator=LinearRegression(), residual_threshold=0.01, max_trials=2000).fit(X, s).inlier_mask_ for s in shifts]

    sets_dev = inlier_sets((b.shifts_x, b.shifts_y, b.shifts_z))
    sets_orc = inlier_sets([want_fit[k] for k in ("shift_x", "shift_y", "shift_z")])
    g = 0.0
    for m_dev, m_orc in zip(sets_dev, sets_orc):
        assert np.array_equal(m_dev, m_orc)
        A = np.column_stack([X[m_orc], np.ones(m_orc.sum())])
        w = np.stack([x.ravel(), y.ravel(), np.ones(x.size)], axis=1) @ np.linalg.pinv(A)
        g = max(g, np.abs(w).sum(axis=1).max())
    eps_h, eps_z = bc.BAR_PX * bc.RES, bc.BAR_Z
    inv = np.array(bo.inverse_field(coeff[0], coeff[1])).reshape(2, 2)
    dp = np.abs(inv).sum(axis=1).max() * g * eps_h + 1e-9
    z = np.array(tba, dtype=np.float64)
    step = max(np.nanmax(np.abs(np.diff(z, axis=0))), np.nanmax(np.abs(np.diff(z, axis=1))))
    bound = 2 * step * dp / bc.RES + g * eps_z + (abs(coeff[2][0]) + abs(coeff[2][1])) * dp + 2 * np.finfo(tba.dtype).eps * np.nanmax(np.abs(z))
    both = np.isfinite(got) & np.isfinite(want)
    dev = np.abs(got.astype(np.float64) - want)[both].max()
    print(f"{dtype}: amplification g {g:.3f}, pre-image bound {dp:.3e} m, value bound {bound:.3e}, largest difference {dev:.3e}; "
          f"coefficients {dev_coeff[0]} {dev_coeff[1]} {dev_coeff[2]}")
    assert both.sum() > 0.5 * H * W and dev <= bound
    ux, uy = x - coeff[0][2], y - coeff[1][2]
    col = ((inv[0, 0] * ux + inv[0, 1] * uy) - t6[2]) / t6[0] - 0.5
    row = ((inv[1, 0] * ux + inv[1, 1] * uy) - t6[5]) / t6[4] - 0.5
    near = (np.abs(col - np.round(col)) <= dp / bc.RES) | (np.abs(row - np.round(row)) <= dp / bc.RES) | (np.abs(col - np.floor(col) - 0.5) <= dp / bc.RES) \
        | (np.abs(row - np.floor(row) - 0.5) <= dp / bc.RES)   # (cell borders; rules 2 / 3 switch their nearest pixel at the half)
    assert not ((np.isfinite(got) != np.isfinite(want)) & ~near).any()


def test_steps_outside_the_batched_form_take_the_loop_route(mods):
    _, blockwise, coreg = mods
    ref, tba, block = _case("A", "float32")
    t6 = bc.transform6(ref.shape[0])
    for step in (coreg.NuthKaab(bin_before_fit=False), coreg.NuthKaab(subsample=0.5), coreg.VerticalShift()):
        b = coreg.BlockwiseCoreg(step, block_size_fit=block)
        b.fit(ref, tba, transform=t6)
        assert b.fit_route == "loop"
        assert np.isfinite(b.shifts_z).all() and b.shifts_z.shape == (6,)
        if isinstance(step, coreg.NuthKaab):
            assert np.isfinite(b.shifts_x).all() and np.isfinite(b.shifts_y).all()   # (every tile fits; a fractional subsample draws without a seed, so no value is compared)
        else:
            assert np.isnan(b.shifts_x).all()              # VerticalShift records no horizontal shift: upstream's .get(..., nan)
            np.random.seed(0)
            out = b.apply(tba, transform=t6)[0]
            np.random.seed(0)
            cx, cy, cz = b.coefficients()
            assert tuple(cx) == (0.0, 0.0, 0.0) and tuple(cy) == (0.0, 0.0, 0.0)   # all-NaN shifts count as zeros (blockwise.py:248-249)
            assert np.array_equal(out, bo.apply(np.array(tba), t6, cx, cy, cz, decided("nk_nan_rule")), equal_nan=True)
    # an integer subsample below a tile's valid count leaves pixels out: the loop route draws them
    b = coreg.BlockwiseCoreg(coreg.NuthKaab(subsample=500), block_size_fit=block)
    b.fit(ref, tba, transform=t6)
    assert b.fit_route == "loop" and np.isfinite(b.shifts_x).all()
    with pytest.raises(ValueError, match="The blockwise coregistration only supports affine coregistration methods."):
        coreg.BlockwiseCoreg(coreg.Deramp(), block_size_fit=block)
