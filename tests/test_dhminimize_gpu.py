"""DhMinimize on the GPU: the shifted-dh objective (``DhPlan.shift_nmad`` / ``shift_values``) against the CPU oracle, bit for bit, on
the dense and the list route, at awkward shapes, shifts, tie-heavy and large inputs; the recorded trajectories of the reference's
driver (tests/golden/dhminimize_golden.npz, tools/gen_golden_dhminimize.py); the fitted step alone and in pipelines.

Oracle of one evaluation: ``d = nuthkaab_oracle.shifted_dh(ref, tba, sx, sy, res)[mask]``, then ``np.nanmedian(d)``,
``binning_oracle.nmad(d)`` and ``np.isfinite(d).sum()`` -- under whichever third-party decision the suite runs with."""
import functools
import os
import warnings

import numpy as np
import pytest

from conftest import GOLDEN, decided

pytestmark = pytest.mark.gpu

NO_POINTS = "no valid points"


def _surface(xx, yy):
    return 800.0 + 40.0 * np.sin(xx / 9.0) * np.cos(yy / 7.0) + 15.0 * np.sin((xx + yy) / 5.0)


@functools.lru_cache(maxsize=None)
def _pair(H, W, dtype_name, seed=0, noise=0.05, nan_frac=0.05, shift=(1.3, -0.8, 2.5)):
    """(ref, tba, inlier): tba = ref's surface sampled `shift` pixels away minus a vertical offset; ~5 % NaN in each, a patchy mask."""
    rng = np.random.default_rng(seed)
    dt = np.dtype(dtype_name)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    ref = _surface(xx, yy).astype(dt)
    tba = (_surface(xx + shift[0], yy + shift[1]) - shift[2] + rng.normal(scale=noise, size=(H, W))).astype(dt)
    ref[rng.random((H, W)) < nan_frac] = np.nan
    tba[rng.random((H, W)) < nan_frac] = np.nan
    inlier = rng.random((H, W)) >= 0.03
    if H > 20 and W > 20:
        inlier[H // 2:H // 2 + 6, W // 3:W // 3 + 9] = False
    for a in (ref, tba, inlier):
        a.setflags(write=False)
    return ref, tba, inlier


def _valid(ref, tba, inlier):
    ok = np.isfinite(ref) & np.isfinite(tba)
    return ok if inlier is None else ok & inlier


def _oracle(ref, tba, mask, sx, sy, res):
    import binning_oracle
    import nuthkaab_oracle

    d = nuthkaab_oracle.shifted_dh(ref, tba, sx, sy, res)[mask]
    cnt = int(np.isfinite(d).sum())
    if cnt == 0:
        return d, None, None, 0
    return d, np.nanmedian(d), binning_oracle.nmad(d), cnt


def _same_bits(got: float, want, dtype) -> bool:
    return np.dtype(dtype).type(got).tobytes() == np.dtype(dtype).type(want).tobytes()


def _plan(ref, tba, inlier, route):
    """(plan, sample mask): every valid pixel (dense route) or the pixels of ``subsample_ranks(n_valid, 3000, 42)`` (list route)."""
    from xdem_amd import coreg

    plan = coreg.DhPlan(ref, tba, inlier)
    mask = _valid(ref, tba, inlier)
    assert plan.n_valid == int(mask.sum())
    if route == "list":
        ranks = coreg.subsample_ranks(plan.n_valid, 3000, 42)
        sel = np.zeros(mask.size, dtype=bool)
        sel[np.flatnonzero(mask.ravel())[ranks]] = True
        mask = sel.reshape(mask.shape)
        assert plan.subsample(ranks) == int(mask.sum())
    return plan, mask


def _check(plan, ref, tba, mask, sx, sy, res):
    from xdem_amd import _lib

    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        d, med, nm, cnt = _oracle(ref, tba, mask, sx, sy, res)
    vals = plan.shift_values(sx, sy, res)
    assert vals.dtype == ref.dtype and np.array_equal(vals, d, equal_nan=True), (sx, sy)
    if cnt == 0:
        with pytest.raises(_lib.XdemHipError, match=NO_POINTS):
            plan.shift_nmad(sx, sy, res)
        return 0
    g_med, g_nm, g_cnt = plan.shift_nmad(sx, sy, res)
    assert g_cnt == cnt, (sx, sy, g_cnt, cnt)
    assert _same_bits(g_med, med, ref.dtype), (sx, sy, g_med, med)
    assert _same_bits(g_nm, nm, ref.dtype), (sx, sy, g_nm, nm)
    return cnt


def _shifts(res):
    rx, ry = res
    return [(0.0, 0.0), (rx, 0.0), (-rx, 0.0), (0.0, ry), (0.0, -ry), (rx, -ry), (0.37 * rx, -1.62 * ry), (-2.5 * rx, 0.25 * ry)]


SHAPES = [(67, 131, "float32"), (50, 70, "float64"), (1, 40, "float32"), (40, 1, "float64")]


@pytest.mark.parametrize("route", ["dense", "list"])
@pytest.mark.parametrize("res", [(10.0, 10.0), (10.0, 20.0)])
@pytest.mark.parametrize("H,W,dtype", SHAPES)
def test_shift_nmad_matches_the_oracle(H, W, dtype, res, route):
    """Widths that are no multiple of 4 or 64 (scalar tail, unaligned rows), one-row and one-column rasters, whole-pixel and
    fractional shifts of both signs, square and non-square pixels; a shift beyond the raster leaves no point."""
    from xdem_amd import _lib

    ref, tba, inlier = _pair(H, W, dtype)
    plan, mask = _plan(ref, tba, inlier, route)
    with plan:
        counts = [_check(plan, ref, tba, mask, sx, sy, res) for sx, sy in _shifts(res)]
        assert 0 < counts[0] <= int(mask.sum())   # (zero shift: the "4tap" rule still drops pixels next to a NaN, zero weights count)
        if min(H, W) > 1:
            assert all(c > 0 for c in counts)
        for sx, sy in (((W + 1) * res[0], 0.0), (0.0, -(H + 1) * res[1])):
            with pytest.raises(_lib.XdemHipError, match=NO_POINTS):
                plan.shift_nmad(sx, sy, res)
            assert np.isnan(plan.shift_values(sx, sy, res)).all()


@pytest.mark.parametrize("route", ["dense", "list"])
def test_odd_and_even_counts(route):
    """Both parities of the count after the NaN drop-outs: the second configuration leaves out one pixel that survived in the first
    (dense: masked as an outlier; list: its rank is not drawn)."""
    import nuthkaab_oracle
    from xdem_amd import coreg

    res = (10.0, 20.0)
    ref, tba, inlier = _pair(67, 131, "float32")
    sx, sy = 0.37 * res[0], -1.62 * res[1]
    alive = np.isfinite(nuthkaab_oracle.shifted_dh(ref, tba, sx, sy, res))
    valid = _valid(ref, tba, inlier)
    seen = set()
    if route == "dense":
        for drop in (False, True):
            inl = inlier.copy()
            if drop:
                inl.flat[np.flatnonzero((valid & alive).ravel())[7]] = False
            plan, mask = _plan(ref, tba, inl, "dense")
            with plan:
                seen.add(_check(plan, ref, tba, mask, sx, sy, res) % 2)
    else:
        pixels = np.flatnonzero(valid.ravel())
        ranks = coreg.subsample_ranks(pixels.size, 3000, 42)
        first_alive = next(i for i, r in enumerate(ranks) if alive.flat[pixels[r]])
        for rk in (ranks, np.delete(ranks, first_alive)):
            mask = np.zeros(valid.size, dtype=bool)
            mask[pixels[rk]] = True
            mask = mask.reshape(valid.shape)
            with coreg.DhPlan(ref, tba, inlier) as plan:
                assert plan.subsample(rk) == rk.size
                seen.add(_check(plan, ref, tba, mask, sx, sy, res) % 2)
    assert seen == {0, 1}


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_ties(dtype):
    """ref and tba on a 0.25 lattice, whole-pixel shift: dh has at most 16 distinct values, every digit pass meets ties."""
    rng = np.random.default_rng(5)
    H, W = 67, 131
    ref = (np.round(rng.uniform(0, 1.75, (H, W)) * 4) / 4).astype(dtype)
    tba = (np.round(rng.uniform(0, 1.75, (H, W)) * 4) / 4).astype(dtype)
    tba[rng.random((H, W)) < 0.05] = np.nan
    res = (10.0, 10.0)
    for route in ("dense", "list"):
        plan, mask = _plan(ref, tba, None if route == "dense" else np.ones((H, W), bool), route)
        with plan:
            for sx, sy in ((10.0, -20.0), (0.0, 0.0)):
                d = _oracle(ref, tba, mask, sx, sy, res)[0]
                assert np.unique(d[np.isfinite(d)]).size <= 16
                _check(plan, ref, tba, mask, sx, sy, res)


@functools.lru_cache(maxsize=None)
def _large(H, W):
    return _pair(H, W, "float32", seed=11, nan_frac=0.02)


@pytest.mark.parametrize("H,W", [(1500, 1000), (2100, 2000)])
def test_large_counts(H, W):
    """1500 x 1000, and 2100 x 2000 = 4.2e6 >= SEL_BRACKET_MIN_N (2^22) values, where both selections take the bracketed route; there also
    with the plain digit passes forced (selection 1) and with degenerate brackets, which miss and fall back (selection 2)."""
    from xdem_amd import _lib

    ref, tba, inlier = _large(H, W)
    res = (10.0, 10.0)
    sx, sy = 3.7, -16.2
    plan, mask = _plan(ref, tba, inlier, "dense")
    with plan:
        cnt = _check(plan, ref, tba, mask, sx, sy, res)
        first = plan.shift_nmad(sx, sy, res)
        if H * W >= 1 << 22:
            assert cnt < H * W   # (the staging buffer decides the route: H * W values)
            ctx = _lib.default_context()
            for mode in (1, 2):
                with ctx.option_scope("selection", mode):
                    assert plan.shift_nmad(sx, sy, res) == first
        other = plan.shift_nmad(-12.5, 2.5, res)
        assert other != first
        assert plan.shift_nmad(sx, sy, res) == first


@pytest.mark.parametrize("route", ["dense", "list"])
def test_repeated_evaluations_return_the_same_bits(route):
    """20 evaluations at alternating shifts on one plan, then the first again: no stale staging or histogram state between calls."""
    ref, tba, inlier = _pair(67, 131, "float32")
    res = (10.0, 20.0)
    plan, mask = _plan(ref, tba, inlier, route)
    a, b = (3.7, -32.4), (-25.0, 5.0)
    with plan:
        first_a, first_b = plan.shift_nmad(*a, res), plan.shift_nmad(*b, res)
        assert first_a != first_b
        for i in range(18):
            got = plan.shift_nmad(*(a if i % 2 == 0 else b), res)
            assert got == (first_a if i % 2 == 0 else first_b)
        assert plan.shift_nmad(*a, res) == first_a
        v = plan.shift_values(*a, res)
        assert plan.shift_nmad(*b, res) == first_b   # (shift_values shares the staging buffer)
        assert np.array_equal(plan.shift_values(*a, res), v, equal_nan=True)


# ---- the reference's driver -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _golden():
    return dict(np.load(os.path.join(GOLDEN, "dhminimize_golden.npz")))


@pytest.mark.parametrize("case", ["f32", "f64"])
def test_recorded_trajectory_and_offsets(case):
    """Every (x, y) the reference's Nelder-Mead evaluated gives the recorded loss bit for bit, so the fit takes the recorded path and
    returns the recorded offsets exactly."""
    from xdem_amd import coreg

    g = _golden()
    rule = decided("nk_nan_rule")
    ref, tba, inlier, mask = (g[f"{case}_{k}"] for k in ("ref", "tba", "inlier", "mask"))
    res = tuple(float(v) for v in g[f"{case}_res"])
    traj, offsets = g[f"{case}_r{rule}_traj"], g[f"{case}_r{rule}_offsets"]
    assert traj.shape[0] > 50
    with coreg.DhPlan(ref, tba, inlier) as plan:
        assert plan.n_valid == int(mask.sum())
        for x, y, loss in traj:
            assert plan.shift_nmad(x, y, res)[1] == loss, (x, y)
    c = coreg.DhMinimize(subsample=1).fit(ref, tba, inlier, resolution=res)
    a = c.meta["outputs"]["affine"]
    assert (a["shift_x"], a["shift_y"], a["shift_z"]) == tuple(offsets)
    assert c.meta["outputs"]["random"]["subsample_final"] == int(mask.sum())
    assert c.meta["outputs"]["specific"]["n_evaluations"] == traj.shape[0]


def _cpu_minimize(ref, tba, mask, res, loss):
    import nuthkaab_oracle
    import scipy.optimize

    r = scipy.optimize.minimize(lambda x: loss(nuthkaab_oracle.shifted_dh(ref, tba, float(x[0]), float(x[1]), res)[mask]), (1, 1),
                                method="Nelder-Mead")
    return -r.x[0], -r.x[1]


def test_host_callable_route_equals_cpu_minimisation():
    """fit_loss_func = np.nanstd: the callable gets the flattened dh of the selected pixels, equal to the oracle's at every point, so
    the minimiser ends where the CPU run over the oracle interpolator ends."""
    from xdem_amd import coreg

    g = _golden()
    ref, tba, inlier, mask = (g[f"f32_{k}"] for k in ("ref", "tba", "inlier", "mask"))
    res = (10.0, 10.0)
    c = coreg.DhMinimize(fit_loss_func=np.nanstd, subsample=1).fit(ref, tba, inlier, resolution=res)
    east, north = _cpu_minimize(ref, tba, mask, res, np.nanstd)
    assert (c.meta["outputs"]["affine"]["shift_x"], c.meta["outputs"]["affine"]["shift_y"]) == (east, north)


def test_known_answer_and_apply():
    """An analytic surface sampled (1.3, -0.8) px away plus a vertical offset: the CPU oracle minimisation lands within 0.05 px of the
    truth, the GPU fit lands where it does; apply is apply_translation with the fitted numbers."""
    import binning_oracle
    from xdem_amd import coreg

    res = (10.0, 20.0)
    ref, tba, inlier = _pair(80, 100, "float32", seed=3, noise=0.0, nan_frac=0.01)
    mask = _valid(ref, tba, inlier)
    truth = (1.3 * res[0], 0.8 * res[1])
    east, north = _cpu_minimize(ref, tba, mask, res, binning_oracle.nmad)
    dist = float(np.hypot((east - truth[0]) / res[0], (north - truth[1]) / res[1]))
    print(f"CPU oracle minimisation: {dist:.4f} px from the truth")
    assert dist < 0.05
    c = coreg.DhMinimize(subsample=1).fit(ref, tba, inlier, resolution=res)
    a = c.meta["outputs"]["affine"]
    assert (a["shift_x"], a["shift_y"]) == (east, north)
    assert float(np.hypot((a["shift_x"] - truth[0]) / res[0], (a["shift_y"] - truth[1]) / res[1])) < 0.05
    assert abs(a["shift_z"] - 2.5) < 0.05
    assert c.is_affine and c.to_translations() == (a["shift_x"], a["shift_y"], a["shift_z"])
    out = c.apply(tba, resolution=res)
    want = coreg.apply_translation(tba, a["shift_x"], a["shift_y"], a["shift_z"], res)
    assert out.dtype == tba.dtype and np.array_equal(out, want, equal_nan=True)


def test_pipeline_and_coregister_3d():
    import xdem_amd
    from xdem_amd import coreg

    res = (10.0, 10.0)
    ref, tba, inlier = _pair(67, 131, "float32")
    alone = coreg.DhMinimize(subsample=1).fit(ref, tba, inlier, resolution=res)
    pipe = (coreg.DhMinimize(subsample=1) + coreg.Deramp(subsample=1)).fit(ref, tba, inlier, resolution=res)
    assert pipe.pipeline[0].meta["outputs"] == alone.meta["outputs"]
    assert "fit_params" in pipe.pipeline[1].meta["outputs"]["fitorbin"]
    like = coreg.NuthKaab(subsample=1) + coreg.Deramp(subsample=1)
    assert pipe.is_affine == like.is_affine is False
    with pytest.raises(NotImplementedError, match="not an affine transformation"):
        pipe.to_matrix()
    both = (coreg.DhMinimize(subsample=1) + coreg.VerticalShift()).fit(ref, tba, inlier, resolution=res)
    assert both.is_affine and np.array_equal(both.to_matrix(), both.pipeline[1].to_matrix() @ both.pipeline[0].to_matrix())
    tr = (10.0, 0.0, 0.0, 0.0, -10.0, 0.0)
    dem = xdem_amd.DEM(tba, tr).coregister_3d(xdem_amd.DEM(ref, tr), coreg.DhMinimize(subsample=1), inlier_mask=inlier)
    assert np.array_equal(dem.data, alone.apply(tba, resolution=res), equal_nan=True)


def test_default_subsample_draws_once():
    """subsample below the valid count: the drawn pixels are the selection of every evaluation (list route), and the fit equals the CPU
    minimisation over the same pixels."""
    import binning_oracle
    from xdem_amd import coreg

    res = (10.0, 10.0)
    ref, tba, inlier = _pair(67, 131, "float32")
    valid = _valid(ref, tba, inlier)
    ranks = coreg.subsample_ranks(int(valid.sum()), 3000, 42)
    sel = np.zeros(valid.size, dtype=bool)
    sel[np.flatnonzero(valid.ravel())[ranks]] = True
    c = coreg.DhMinimize(subsample=3000).fit(ref, tba, inlier, resolution=res, random_state=42)
    assert c.meta["outputs"]["random"]["subsample_final"] == 3000
    east, north = _cpu_minimize(ref, tba, sel.reshape(valid.shape), res, binning_oracle.nmad)
    assert (c.meta["outputs"]["affine"]["shift_x"], c.meta["outputs"]["affine"]["shift_y"]) == (east, north)
