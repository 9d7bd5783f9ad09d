"""Deramp / VerticalShift / CoregPipeline on the MI355X (csrc/biascorr.hip) against the reference's fixtures
(tests/golden/biascorr_golden.npz, tools/gen_golden_biascorr.py) and known answers."""
import os

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

G = np.load(os.path.join(GOLDEN, "biascorr_golden.npz"))


def _valid():
    return G["inlier"] & np.isfinite(G["ref"]) & np.isfinite(G["tba"])


@pytest.mark.parametrize("order", [1, 2, 3])
def test_deramp_fit_matches_curve_fit(order):
    from xdem_amd import coreg
    from xdem_amd.biascorr import polynomial_2d

    d = coreg.Deramp(poly_order=order, subsample=1).fit(G["ref"], G["tba"], inlier_mask=G["inlier"], resolution=1.0)
    p = d.meta["outputs"]["fitorbin"]["fit_params"]
    v = _valid()
    y, x = np.nonzero(v)
    dh = (G["ref"][v] - G["tba"][v]).astype(np.float64)
    mine, theirs = polynomial_2d((x, y), *p), polynomial_2d((x, y), *G[f"o{order}_fit_params"])
    assert float(np.sum((dh - mine) ** 2)) <= float(G[f"o{order}_sse"]) * (1 + 1e-9)
    yy, xx = np.mgrid[0:G["ref"].shape[0], 0:G["ref"].shape[1]]
    P = polynomial_2d((xx, yy), *p)
    assert np.max(np.abs(P - polynomial_2d((xx, yy), *G[f"o{order}_fit_params"]))) <= 1e-4 * (1 + np.max(np.abs(P)))
    np.testing.assert_allclose(d.meta["outputs"]["fitorbin"]["fit_perr"], G[f"o{order}_fit_perr"], rtol=1e-5)
    assert d.meta["outputs"]["random"]["subsample_final"] == int(v.sum()) and np.max(np.abs(mine - theirs)) < 1e-3


@pytest.mark.parametrize("order", [1, 2, 3])
def test_deramp_apply_bit_for_bit(order):
    from xdem_amd import coreg

    d = coreg.Deramp(poly_order=order)
    d.meta["outputs"]["fitorbin"] = {"fit_params": G[f"o{order}_fit_params"]}
    out = d.apply(G["tba"])
    assert out.dtype == np.float32
    assert np.array_equal(out, G[f"o{order}_applied"], equal_nan=True)
    # float64 input: the float64 sum, before the reference's final cast
    from xdem_amd.biascorr import polynomial_2d

    t64 = G["tba"].astype(np.float64)
    yy, xx = np.meshgrid(np.arange(t64.shape[0]), np.arange(t64.shape[1]), indexing="ij")
    assert np.array_equal(d.apply(t64), t64 + polynomial_2d((xx, yy), *G[f"o{order}_fit_params"]), equal_nan=True)


def test_vertical_shift_median_bit_for_bit():
    from xdem_amd import coreg

    vs = coreg.VerticalShift().fit(G["ref"], G["tba"], inlier_mask=G["inlier"], resolution=1.0)
    assert vs.meta["outputs"]["affine"]["shift_z"] == G["vshift_f32"]
    assert vs.meta["outputs"]["random"]["subsample_final"] == int(_valid().sum())
    vs64 = coreg.VerticalShift(vshift_reduc_func=np.nanmedian).fit(G["ref"].astype(np.float64) + 0.1, G["tba"].astype(np.float64),
                                                                    inlier_mask=G["inlier"])
    assert vs64.meta["outputs"]["affine"]["shift_z"] == G["vshift_f64"]
    # any other callable gets dh through the values route: the same number as on the host
    v = _valid()
    dh = G["ref"][v] - G["tba"][v]
    vsm = coreg.VerticalShift(vshift_reduc_func=np.mean).fit(G["ref"], G["tba"], inlier_mask=G["inlier"])
    assert vsm.meta["outputs"]["affine"]["shift_z"] == float(np.mean(dh))
    out = vs.apply(G["tba"], resolution=1.0)
    assert np.array_equal(out, G["tba"] + np.float32(G["vshift_f32"]), equal_nan=True)


def test_subsample_route_uses_the_same_pixels():
    """The device draw selects exactly subsample_valid_mask's pixels: the values route returns their dh / coordinates, and the median
    and the moments over them equal NumPy's over the host-drawn mask."""
    from xdem_amd import coreg
    from xdem_amd.biascorr import DhPlan, polynomial_2d

    v = _valid()
    mask = coreg.subsample_valid_mask(v, 3000, random_state=42)
    with DhPlan(G["ref"], G["tba"], G["inlier"]) as plan:
        assert plan.n_valid == int(v.sum())
        plan.subsample(coreg.subsample_ranks(plan.n_valid, 3000, 42))
        dh, col, row = plan.values()
        y, x = np.nonzero(mask)
        assert np.array_equal(col, x) and np.array_equal(row, y) and np.array_equal(dh, G["ref"][mask] - G["tba"][mask])
        assert plan.median() == (float(np.median(G["ref"][mask] - G["tba"][mask])), 3000)
    d = coreg.Deramp(poly_order=2, subsample=3000).fit(G["ref"], G["tba"], inlier_mask=G["inlier"], random_state=42)
    import scipy.optimize

    popt, _ = scipy.optimize.curve_fit(polynomial_2d, np.array([x, y]), (G["ref"][mask] - G["tba"][mask]), p0=np.ones(9), absolute_sigma=True)
    p = d.meta["outputs"]["fitorbin"]["fit_params"]
    assert np.max(np.abs(polynomial_2d((x, y), *p) - polynomial_2d((x, y), *popt))) < 1e-4 * (1 + np.max(np.abs(polynomial_2d((x, y), *p))))
    assert d.meta["outputs"]["random"]["subsample_final"] == 3000


def test_fit_is_deterministic_and_row_blocks_add_up():
    from xdem_amd import coreg
    from xdem_amd.biascorr import DhPlan

    rng = np.random.default_rng(1)
    H, W = 1500, 1000
    ref = rng.normal(size=(H, W)).astype(np.float32)
    tba = (ref - 0.5 + 1e-3 * np.arange(W)[None, :] + rng.normal(scale=0.1, size=(H, W))).astype(np.float32)
    ref[rng.random((H, W)) < 0.05] = np.nan
    a = coreg.Deramp(subsample=1).fit(ref, tba).meta["outputs"]["fitorbin"]
    b = coreg.Deramp(subsample=1).fit(ref, tba).meta["outputs"]["fitorbin"]
    assert a["fit_params"].tobytes() == b["fit_params"].tobytes() and a["fit_perr"].tobytes() == b["fit_perr"].tobytes()
    for order in (0, 2, 5):
        with DhPlan(ref, tba) as whole, DhPlan(ref[:700], tba[:700]) as top, DhPlan(ref[700:], tba[700:]) as bot:
            Mw, Rw, nw = whole.poly_moments(order)
            Mt, Rt, nt = top.poly_moments(order, 0, H, W)
            Mb, Rb, nb = bot.poly_moments(order, 700, H, W)
            assert nw == nt + nb
            np.testing.assert_allclose(Mt + Mb, Mw, rtol=1e-12, atol=1e-12 * np.abs(Mw).max())
            np.testing.assert_allclose(Rt + Rb, Rw, rtol=1e-12, atol=1e-12 * np.abs(Rw).max())


def _shifted_pair(H, W, dx, dy, seed=0):
    """tba = ref translated by (dx, dy) pixels (an analytic surface evaluated at shifted coordinates) + a ramp."""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)

    def surf(x, y):
        return 500 + 40 * np.sin(x / 23.0) * np.cos(y / 31.0) + 25 * np.sin((x + 2 * y) / 47.0) + 0.05 * x

    ref = surf(xx, yy)
    ramp = 2.0 + 3e-3 * xx - 4e-3 * yy
    tba = surf(xx + dx, yy + dy) + ramp
    return ref.astype(np.float32), tba.astype(np.float32), ramp


def test_known_answers_pipelines():
    from xdem_amd import coreg

    ref, tba, ramp = _shifted_pair(600, 700, 2.5, -1.5)
    pipe = coreg.NuthKaab() + coreg.Deramp(poly_order=1)
    out = pipe.fit_and_apply(ref, tba, fit_kwargs={"resolution": 1.0}, random_state=0)
    nk, dr = pipe.pipeline
    sx, sy = nk.meta["outputs"]["affine"]["shift_x"], nk.meta["outputs"]["affine"]["shift_y"]
    # the translation (shift_x = -easting; rows grow southwards) and the ramp (its slopes) are recovered
    # tba(x, y) = ref(x + 2.5, y - 1.5), so ref(c, r) = tba(c - 2.5, r + 1.5) = apply's elev(r + shift_y, c - shift_x): +2.5, +1.5
    assert abs(sx - 2.5) < 0.1 and abs(sy - 1.5) < 0.1, (sx, sy)
    p = dr.meta["outputs"]["fitorbin"]["fit_params"]
    assert abs(p[2] + 3e-3) < 3e-4 and abs(p[1] - 4e-3) < 3e-4   # (dh = ref - tba carries minus the ramp)
    res = (out - ref)[20:-20, 20:-20]
    assert np.nanmedian(np.abs(res)) < 0.2
    # VerticalShift() + NuthKaab(): the pipeline equals the steps run by hand
    p2 = coreg.VerticalShift() + coreg.NuthKaab(subsample=1)
    p2.fit(ref, tba, resolution=1.0)
    o2 = p2.apply(tba, resolution=1.0)
    vs = coreg.VerticalShift().fit(ref, tba, resolution=1.0)
    t1 = vs.apply(tba, resolution=1.0)
    nk2 = coreg.NuthKaab(subsample=1).fit(ref, t1, resolution=1.0)
    assert p2.pipeline[0].meta["outputs"]["affine"] == vs.meta["outputs"]["affine"]   # (exact median: the same bits)
    a, b = p2.pipeline[1].meta["outputs"]["affine"], nk2.meta["outputs"]["affine"]
    # (two Nuth-Kaab fits of the same rasters need not agree to the last bit: its curve_fit starts from float32 partial sums)
    assert all(abs(a[k] - b[k]) <= 1e-3 for k in ("shift_x", "shift_y", "shift_z")), (a, b)
    # the pipeline's apply is its steps' applies chained, bit for bit
    o_hand = p2.pipeline[1].apply(p2.pipeline[0].apply(tba, resolution=1.0), resolution=1.0)
    assert np.array_equal(o2, o_hand, equal_nan=True)
    m = p2.to_matrix()
    assert m[2, 3] == vs.meta["outputs"]["affine"]["shift_z"] + a["shift_z"]


def test_scale_20000_through_coregister_3d():
    import xdem_amd
    from xdem_amd import coreg

    H = W = 20000
    rng = np.random.default_rng(5)
    yy = np.arange(H, dtype=np.float32)[:, None]
    xx = np.arange(W, dtype=np.float32)[None, :]
    ref = (1000 + 0.01 * xx + 0.02 * yy).astype(np.float32) + rng.normal(scale=0.5, size=(H, W)).astype(np.float32)
    tba = ref - (1.0 + 1e-4 * xx - 2e-4 * yy)
    tr = (1.0, 0.0, 0.0, 0.0, -1.0, float(H))
    out = xdem_amd.DEM(tba, tr).coregister_3d(xdem_amd.DEM(ref, tr), coreg.Deramp(poly_order=1), random_state=0)
    assert out.data.dtype == np.float32 and out.data.shape == (H, W)
    err = (out.data - ref)[::97, ::89]
    assert np.max(np.abs(err)) < 1e-2


def test_poly2d_apply_device_tensors():
    """Device path of poly2d_apply: the host path's bits, on the current torch stream (elev produced by torch right before the call,
    out consumed by torch right after, no explicit synchronisation); anything but a contiguous 2-D float32 / float64 CUDA tensor, or an
    `out` that does not match it, is refused before any launch."""
    import torch

    from xdem_amd.biascorr import poly2d_apply

    params = G["o2_fit_params"]
    want = poly2d_apply(G["tba"], params)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        base = torch.from_numpy(np.nan_to_num(G["tba"], nan=-1.0)).cuda()
        elev = base * 1.0            # (queued on s, just before the apply)
        got = poly2d_apply(elev, params)
        got = got * 1.0              # (consumed on s right after)
    s.synchronize()
    assert np.array_equal(got.cpu().numpy(), poly2d_apply(np.nan_to_num(G["tba"], nan=-1.0), params))
    t = torch.from_numpy(G["tba"]).cuda()
    assert np.array_equal(poly2d_apply(t, params).cpu().numpy(), want, equal_nan=True)
    out = torch.empty_like(t)
    assert poly2d_apply(t, params, out=out) is out and np.array_equal(out.cpu().numpy(), want, equal_nan=True)
    # 192 columns (W % 4 == 0) take the four-wide kernel on both sides: the device path against the host path, the same bits.  Both
    # kernels against NumPy: tests/test_deramp_routes_gpu.py
    assert np.array_equal(poly2d_apply(t[:, :-1].contiguous(), params).cpu().numpy(), poly2d_apply(G["tba"][:, :-1], params), equal_nan=True)
    for bad in (t.half(), t.to(torch.bfloat16), t.to(torch.int32), t.t(), t[:, ::2], t.reshape(-1), t.cpu()):
        with pytest.raises(ValueError):
            poly2d_apply(bad, params)
    for bad_out in (torch.empty_like(t, dtype=torch.float64), torch.empty((t.shape[0], t.shape[1] - 1), device=t.device),
                    torch.empty_like(t).t().contiguous().t(), np.empty(t.shape, dtype=np.float32)):
        with pytest.raises(ValueError):
            poly2d_apply(t, params, out=bad_out)


@pytest.mark.parametrize("shape", [(333, 517), (2101, 2011)])
def test_nk_and_dh_plans_select_the_same_pixels(shape):
    """The two subsample entry points share one rank selection: given the same ranks over the same valid pixels, the NK plan's inlier
    mask and the dh plan's pixel list name the same pixels -- flatnonzero(valid)[ranks], a repeated rank counted once.  333 x 517 is
    not a multiple of 16 or 4096 pixels; 2101 x 2011 has more than 1024 tiles of 4096, so the tile scan carries over pieces."""
    from xdem_amd import coreg
    from xdem_amd.biascorr import DhPlan

    rng = np.random.default_rng(3)
    ref = (100 + np.cumsum(rng.normal(size=shape), axis=1)).astype(np.float32)
    tba = (ref + rng.normal(scale=0.1, size=shape)).astype(np.float32)
    ref[rng.random(shape) < 0.05] = np.nan
    with coreg.NKPlan(ref, tba, None) as nk0:
        valid = nk0.aux()[2]   # (the NK rule is the stricter one: as inlier mask it makes both plans' valid pixels the same)
    ranks = coreg.subsample_ranks(int(valid.sum()), 0.3, 11)
    ranks = np.concatenate([ranks, ranks[:50], ranks[-7:]])
    want = np.zeros(valid.size, dtype=bool)
    want[np.flatnonzero(valid)[ranks]] = True
    want = want.reshape(shape)
    with coreg.NKPlan(ref, tba, valid) as nk, DhPlan(ref, tba, valid) as dh:
        assert nk.n_valid == dh.n_valid == int(valid.sum())
        assert nk.subsample(ranks) == dh.subsample(ranks) == int(want.sum())
        _, col, row = dh.values()
        got = np.zeros(shape, dtype=bool)
        got[row, col] = True
        assert np.array_equal(nk.aux()[2], want) and np.array_equal(got, want)
        assert np.all(np.diff(row * shape[1] + col) > 0)   # (raster order)


def test_nk_plan_takes_any_device_mask_and_refuses_other_dtypes():
    """NKPlan and DhPlan share one input front: a device inlier mask of any integer / bool dtype is converted to uint8, and a CUDA
    dtype other than float32 / float64 is a ValueError."""
    import torch

    from xdem_amd import coreg

    rng = np.random.default_rng(5)
    ref = torch.from_numpy((100 + np.cumsum(rng.normal(size=(64, 80)), axis=1)).astype(np.float32)).cuda()
    tba = ref + 0.5
    mask = np.ones((64, 80), dtype=bool)
    mask[10:20, 30:50] = False
    with coreg.NKPlan(ref.cpu().numpy(), tba.cpu().numpy(), mask.astype(np.uint8)) as host:
        want = host.aux()[2]
    for m in (torch.from_numpy(mask).cuda(), torch.from_numpy(mask.astype(np.int32)).cuda()):
        with coreg.NKPlan(ref, tba, m) as plan:
            assert np.array_equal(plan.aux()[2], want)
    with pytest.raises(ValueError, match="float32 / float64"):
        coreg.NKPlan(ref.half(), tba.half(), None)
