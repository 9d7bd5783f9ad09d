"""csrc/vector.hip behind ``xdem_amd.Vector`` against the rule's NumPy restatement (vector_oracle.py) BIT FOR BIT: mask, labels and the
count of burnt pixels, from host and device tables and planes, from two runs, and from every sort route forced by its test switch.

The inputs are the smallest at which a stage can go wrong: a triangle inside one pixel; polygons outside, over and across each side
of the grid; combs whose rows are crossed 2, SEG_REG, SEG_REG + 2, SEG_LDS and SEG_LDS + 2 times (the register, LDS and global sort
routes and their borders); spans of 0, 1, 63, 64, 65, 255, 256, 257 and W columns and one that ends on column W - 1 (the lane and the
wave store routes); vertices on centre lines and edges through centres on a unit grid with origin 0, where the abscissae are exact and
the half-open rule itself decides; shared edges, holes, a hole's hole, multipolygons, both orientations, unclosed and degenerate
rings; overlaps in both table orders; 3000 polygons with the same number of launches as 3; 1 x 1 and 1 x W grids; and the consumers
end to end."""
import functools
import warnings

import numpy as np
import pytest

import vector_cases as vcs
import vector_oracle as vo

pytestmark = pytest.mark.gpu


def _ctx():
    from xdem_amd import _lib

    return _lib.default_context()


def check(geoms, shape, t6, burn=None, out_value=0, device=False):
    """Mask, labels and both counts of a table against the oracle; returns (vector, mask, labels)."""
    from xdem_amd import Vector, vector

    v = geoms if isinstance(geoms, Vector) else Vector(geoms)
    table = v.tables()
    want_mask = vo.mask([table], shape, t6)
    burn_arr = np.arange(1, len(v) + 1) if burn is None else (np.full(len(v), burn) if np.ndim(burn) == 0 else np.asarray(burn))
    want_lab, want_count = vo.labels(table, burn_arr, out_value, shape, t6)
    v._cache.clear()
    got_mask = v.create_mask((shape, t6), device=device)
    count_mask = vector.DeviceRasterizer.last_count
    got_lab = v.rasterize((shape, t6), in_value=burn, out_value=out_value, device=device)
    count_lab = vector.DeviceRasterizer.last_count
    if device:
        import torch

        assert got_mask.is_cuda and got_mask.dtype == torch.bool and got_lab.is_cuda and got_lab.dtype == torch.int32
        got_mask, got_lab = got_mask.cpu().numpy(), got_lab.cpu().numpy()
    assert got_mask.dtype == np.bool_ and got_lab.dtype == np.int32
    assert got_mask.shape == tuple(shape) and got_lab.shape == tuple(shape)
    assert np.array_equal(got_mask, want_mask), f"{int((got_mask != want_mask).sum())} mask pixels differ"
    assert np.array_equal(got_lab, want_lab), f"{int((got_lab != want_lab).sum())} label pixels differ"
    assert count_mask == int(want_mask.sum()) == want_count == count_lab
    return v, got_mask, got_lab


@pytest.mark.parametrize("shape", vcs.SHAPES)
def test_star_with_hole_host_device_and_two_runs(shape):
    shape, t6 = vcs.grid(*shape)
    geom = vcs.star_with_hole(shape, t6)
    _, m_host, l_host = check([geom], shape, t6)
    _, m_dev, l_dev = check([geom], shape, t6, device=True)
    _, m_again, l_again = check([geom], shape, t6, device=True)
    assert np.array_equal(m_host, m_dev) and np.array_equal(l_host, l_dev)
    assert np.array_equal(m_dev, m_again) and np.array_equal(l_dev, l_again)
    assert 0 < m_host.sum() < m_host.size


def test_triangle_inside_one_pixel_burns_one_pixel_or_none():
    shape, t6 = vcs.grid(61, 83)
    around = vcs.world(t6, [(20.3, 30.2), (20.8, 30.4), (20.4, 30.9)])    # holds the centre (20.5, 30.5)
    beside = vcs.world(t6, [(20.05, 30.1), (20.4, 30.1), (20.1, 30.45)])  # does not
    _, m, _ = check([around], shape, t6)
    assert m.sum() == 1 and m[30, 20]
    _, m, _ = check([beside], shape, t6)
    assert m.sum() == 0
    check([beside, around], shape, t6, device=True)


def test_outside_covering_and_across_each_side():
    shape, t6 = vcs.grid(61, 83)
    H, W = shape
    _, m, _ = check([vcs.rect(t6, W + 3.0, W + 20.0, 5.0, 30.0)], shape, t6)
    assert m.sum() == 0
    _, m, _ = check([vcs.rect(t6, -4.0, W + 4.0, -4.0, H + 4.0)], shape, t6)
    assert m.all()
    sides = [vcs.star(shape, t6, n=11, salt=20 + k, centre=c, r_out=14.0, r_in=6.0)
             for k, c in enumerate([(-2.0, 0.4 * H), (W + 1.5, 0.6 * H), (0.3 * W, -3.0), (0.7 * W, H + 2.0)])]
    for s in sides:
        _, m, _ = check([s], shape, t6)
        assert 0 < m.sum()
    check(sides, shape, t6, device=True)


@functools.lru_cache(maxsize=None)
def _comb(n_teeth: int):
    shape, t6 = vcs.grid(96, 128)
    return shape, t6, vcs.comb(t6, n_teeth, 5.3, 10.2, 40.6, 50.4, 100.0 / max(n_teeth, 8), salt=n_teeth)


@pytest.mark.parametrize("n_teeth", [1, vcs.SEG_REG // 2, vcs.SEG_REG // 2 + 1, vcs.SEG_LDS // 2, vcs.SEG_LDS // 2 + 1])
def test_comb_segments_at_the_route_capacities_and_every_route_forced(n_teeth):
    shape, t6, ring = _comb(n_teeth)
    ctx = _ctx()
    _, m0, l0 = check([ring], shape, t6)
    assert m0.sum() > 0
    try:
        for reg, lds in ((1, 0), (1, 1), (0, 1), (vcs.SEG_REG // 2, 16)):
            ctx.set_option("vec_seg_reg", reg)
            ctx.set_option("vec_seg_lds", lds)
            _, m, lab = check([ring], shape, t6)
            assert np.array_equal(m, m0) and np.array_equal(lab, l0), (reg, lds)
    finally:
        ctx.set_option("vec_seg_reg", 0)
        ctx.set_option("vec_seg_lds", 0)


def test_span_widths_on_both_store_routes():
    shape, t6 = vcs.unit_grid(11, 301)
    rects, want = vcs.span_rects(t6, shape[1])
    assert {0, 1, vcs.WIDE - 1, vcs.WIDE, vcs.WIDE + 1, 255, 256, 257, shape[1]} <= {w for _, w in want}
    for device in (False, True):
        _, m, lab = check(rects, shape, t6, device=device)
        for row, (first, n) in enumerate(want):
            assert m[row].sum() == n and (n == 0 or (m[row, first:first + n].all() and lab[row, first] == row + 1)), (row, first, n)
        assert not m[len(want):].any()
    assert m[len(want) - 1, shape[1] - 1]   # (the last column is written, nothing beyond it)


def test_half_open_rule_on_exact_coordinates():
    """Origin 0, resolution 1: centres at half-integers, the abscissae exact.  A vertex on a centre line counts once, an edge through a
    centre holds it on its left end only: [lo, hi) both ways."""
    shape, t6 = vcs.unit_grid(8, 9)   # cy(r) = 8 - (r + 0.5)
    H = shape[0]
    square = np.array([(0.5, 0.5), (2.5, 0.5), (2.5, 2.5), (0.5, 2.5)])   # world coordinates: corners ON centres
    _, m, _ = check([square], shape, t6)
    want = np.zeros(shape, dtype=bool)
    for y in (0.5, 1.5):
        for x in (0.5, 1.5):
            want[int(H - y - 0.5), int(x - 0.5)] = True
    assert np.array_equal(m, want)
    # a triangle whose hypotenuse runs through the centres (1.5, 1.5) .. (5.5, 5.5), its other vertex on a centre line
    tri = np.array([(1.5, 1.5), (6.5, 6.5), (1.5, 6.5)])
    _, m, _ = check([tri], shape, t6)
    want = np.zeros(shape, dtype=bool)
    for r in range(H):
        cy = H - (r + 0.5)
        for c in range(shape[1]):
            cx = c + 0.5
            want[r, c] = 1.5 <= cy < 6.5 and 1.5 <= cx and not cy <= cx   # left edge x = 1.5, hypotenuse x = y
    assert np.array_equal(m, want) and m.sum() == 10
    # a diamond with all four vertices on centres: every row's vertex counts once
    diamond = np.array([(4.5, 0.5), (7.5, 3.5), (4.5, 6.5), (1.5, 3.5)])
    check([diamond, tri, square], shape, t6, device=True)
    # horizontal and vertical edges on centre lines and between them
    check([np.array([(0.5, 3.5), (8.5, 3.5), (8.5, 4.0), (0.5, 4.0)]), np.array([(3.0, 0.0), (3.5, 0.0), (3.5, 8.0), (3.0, 8.0)])], shape, t6)


def test_polygons_sharing_an_edge_take_every_pixel_once():
    shape, t6 = vcs.grid(61, 83)
    a, b, c, d = (10.3, 5.2), (60.7, 12.9), (55.1, 50.6), (14.8, 44.4)
    left = vcs.world(t6, [a, b, d])
    right = vcs.world(t6, [b, c, d])
    both = vcs.world(t6, [a, b, c, d])
    _, m_l, _ = check([left], shape, t6)
    _, m_r, _ = check([right], shape, t6)
    _, m_b, lab = check([left, right], shape, t6)
    _, m_q, _ = check([both], shape, t6)
    assert not (m_l & m_r).any() and np.array_equal(m_l | m_r, m_q) and np.array_equal(m_b, m_q)
    assert np.array_equal(lab == 1, m_l) and np.array_equal(lab == 2, m_r)
    for H, W in vcs.SHAPES:   # the seven strips: every pixel exactly once, so each pixel gets its strip's value in any table order
        shape, t6 = vcs.grid(H, W)
        strips = vcs.strips(shape, t6)
        _, m, lab = check(strips, shape, t6, device=True)
        assert m.all()
        order = [4, 0, 6, 2, 5, 1, 3]
        _, _, lab2 = check([strips[k] for k in order], shape, t6, burn=[k + 1 for k in order])
        assert np.array_equal(lab, lab2)


def test_holes_multipolygons_orientations_unclosed_and_degenerate_rings():
    shape, t6 = vcs.grid(61, 83)
    outer = vcs.rect(t6, 8.4, 70.3, 6.7, 52.2)
    hole = vcs.rect(t6, 20.6, 50.2, 15.3, 40.9, ccw=False)
    island = vcs.rect(t6, 28.1, 41.8, 21.4, 33.3)   # a hole's hole: a polygon of its own
    far = vcs.star(shape, t6, n=7, salt=5, centre=(76.0, 55.0), r_out=6.0, r_in=3.0)
    _, m, lab = check([(outer, [hole]), island], shape, t6)
    assert not m[25, 22] and m[25, 35] and m[10, 10] and lab[25, 35] == 2
    _, m_multi, _ = check([[(outer, [hole]), island, far]], shape, t6)   # one multipolygon row
    assert m_multi.sum() > m.sum()
    _, m_cw, _ = check([(outer[::-1], [hole[::-1]]), island[::-1]], shape, t6)
    assert np.array_equal(m, m_cw)
    closed = np.concatenate([outer, outer[:1]])
    _, m_closed, _ = check([(closed, [np.concatenate([hole, hole[:1]])]), island], shape, t6, device=True)
    assert np.array_equal(m, m_closed)
    line = vcs.world(t6, [(5.0, 5.0), (40.0, 40.0), (5.0, 5.0), (40.0, 40.0)])   # two distinct vertices: contributes nothing
    _, m_deg, _ = check([(outer, [hole, line]), island, line], shape, t6)
    assert np.array_equal(m, m_deg)


def test_overlaps_in_both_orders_in_values_and_out_value():
    shape, t6 = vcs.grid(96, 128)
    a = vcs.star(shape, t6, n=13, salt=11, centre=(50.0, 40.0), r_out=45.0, r_in=20.0)
    b = vcs.star(shape, t6, n=9, salt=12, centre=(75.0, 55.0), r_out=40.0, r_in=25.0)
    _, m_ab, l_ab = check([a, b], shape, t6)
    _, m_ba, l_ba = check([b, a], shape, t6)
    both = vo.rings_mask([a], shape, t6) & vo.rings_mask([b], shape, t6)
    assert both.sum() > 100 and np.array_equal(m_ab, m_ba)
    assert (l_ab[both] == 2).all() and (l_ba[both] == 2).all()   # the later row wins, whichever polygon it is
    check([a, b], shape, t6, burn=7, out_value=-3, device=True)
    _, _, lab = check([a, b], shape, t6, burn=[-5, 2 ** 31 - 1], out_value=255)
    assert set(np.unique(lab)) == {-5, 255, 2 ** 31 - 1}


def test_three_thousand_polygons_take_the_launches_of_three():
    from xdem_amd import vector

    shape, t6 = vcs.grid(96, 128)
    polys = vcs.many_small(shape, t6, 3000)
    check(polys, shape, t6, device=True)
    check(polys, shape, t6)
    many = vector.DeviceRasterizer.launches()
    check(polys[1000:1003], shape, t6)
    few = vector.DeviceRasterizer.launches()
    assert many == few > 0


@pytest.mark.parametrize("shape", [(1, 1), (1, 131), (67, 1)])
def test_smallest_grids(shape):
    shape, t6 = vcs.grid(*shape)
    H, W = shape
    check([vcs.rect(t6, -1.0, W + 1.0, -1.0, H + 1.0)], shape, t6)
    check([vcs.world(t6, [(0.2, 0.1), (W - 0.3, 0.3), (0.6 * W, H - 0.2)])], shape, t6, device=True)
    check([vcs.rect(t6, 0.6, 0.9, 0.6, 0.9)], shape, t6)


def test_labels_on_the_device_pass_as_a_glacier_index_map():
    import torch

    from xdem_amd import Vector, volume

    shape, t6 = vcs.grid(61, 83)
    v = Vector(vcs.strips(shape, t6))
    lab = v.rasterize((shape, t6), device=True)
    plane = volume._labels_plane(lab, torch.zeros(shape, device="cuda"))
    assert plane.is_cuda and plane.dtype == torch.int32 and torch.equal(plane.reshape(shape), lab)


# ---- the consumers, end to end ---------------------------------------------------------------------------------------------------------------
def _outlines(shape, t6):
    a = vcs.star(shape, t6, n=13, salt=31, centre=(0.4 * shape[1], 0.45 * shape[0]), r_out=0.45 * shape[0], r_in=0.25 * shape[0])
    b = vcs.star(shape, t6, n=11, salt=32, centre=(0.6 * shape[1], 0.55 * shape[0]), r_out=0.4 * shape[0], r_in=0.2 * shape[0])
    return a, b


@pytest.mark.parametrize("tensors", [False, True])
def test_collection_with_vector_outlines_equals_the_oracles_masks(tensors):
    import demcollection_cases as dc
    from xdem_amd import DEMCollection, Vector, ddem as ddem_mod

    H, W = dc.SHAPES[0]
    s = dc.stack(H, W, "float32")
    shape = (H, W)
    a, b = _outlines(shape, dc.TRANSFORM)
    stamps = dc.stamps()
    va, vb = Vector([a]), Vector([b])
    ma, mb = vo.mask([va.tables()], shape, dc.TRANSFORM), vo.mask([vb.tables()], shape, dc.TRANSFORM)
    assert 0 < (ma & mb).sum() < min(ma.sum(), mb.sum())

    def put(x):
        if not tensors:
            return x
        import torch

        t = torch.from_numpy(np.array(x)).cuda()
        torch.cuda.synchronize()
        return t

    def run(outlines):
        dems = [ddem_mod.raster_of(put(p), dc.TRANSFORM) for p in s["dems"]]
        col = DEMCollection(dems, timestamps=stamps, outlines=outlines, reference_dem=dc.REFERENCE)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            ddems = col.subtract_dems()
            masks = [col.get_ddem_mask(d) for d in ddems]
            col.interpolate_ddems(method="regional_hypsometric")
            dh, dv = col.get_dh_series(nans_ok=True), col.get_dv_series(nans_ok=True)
        host = [m.cpu().numpy() if hasattr(m, "cpu") else np.asarray(m) for m in masks]   # (a dDEM without a fitting outline: np.ones)
        filled = [d.filled_data.cpu().numpy() if tensors else np.asarray(d.filled_data) for d in ddems]
        return host, filled, dh, dv

    # outlines for the reference's stamp and one other: the dDEM between them takes the union, the others the start outline's rule
    got = run({stamps[dc.REFERENCE]: va, stamps[3]: vb})
    want = run({stamps[dc.REFERENCE]: put(ma), stamps[3]: put(mb)})
    assert any(np.array_equal(m, ma | mb) for m in got[0])
    for g, w in zip(got[0], want[0]):
        assert g.dtype == np.bool_ and np.array_equal(g, w)
    for g, w in zip(got[1], want[1]):
        assert np.array_equal(g, w, equal_nan=True)
    assert got[2].equals(want[2]) and got[3].equals(want[3])


def test_outlines_filter_selects_rows_of_the_table():
    import demcollection_cases as dc
    from xdem_amd import DEMCollection, Vector, ddem as ddem_mod

    H, W = dc.SHAPES[0]
    s = dc.stack(H, W, "float32")
    a, b = _outlines((H, W), dc.TRANSFORM)
    v = Vector([a, b], table={"name": ["north", "south"], "area_km2": [3.5, 0.7]})
    col = DEMCollection([ddem_mod.raster_of(p, dc.TRANSFORM) for p in s["dems"]], timestamps=dc.stamps(), outlines=v, reference_dem=dc.REFERENCE)
    ddems = col.subtract_dems()
    only_b = vo.mask([Vector([b]).tables()], (H, W), dc.TRANSFORM)
    assert np.array_equal(col.get_ddem_mask(ddems[0], outlines_filter="area_km2 < 1"), only_b)
    assert np.array_equal(col.get_ddem_mask(ddems[0], outlines_filter="name == 'south'"), only_b)
    assert np.array_equal(col.get_ddem_mask(ddems[0]), vo.mask([v.tables()], (H, W), dc.TRANSFORM))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = col.get_dh_series(outlines_filter="area_km2 < 1", nans_ok=True)
        want = col.get_dh_series(mask=only_b, nans_ok=True)
    assert got.equals(want)


def test_number_effective_samples_with_a_vector_equals_the_call_with_its_mask():
    import pandas as pd

    from xdem_amd import DEM, Vector, spatialstats

    shape, t6 = vcs.grid(61, 83)
    a, _ = _outlines(shape, t6)
    v = Vector([a])
    params = pd.DataFrame({"model": ["spherical", "gaussian"], "range": [120.0, 900.0], "psill": [0.7, 0.3]})
    res_mask = v.create_mask(res=10.0)
    assert np.array_equal(res_mask, vo.mask([v.tables()], res_mask.shape, (10.0, 0.0, v.bounds.left, 0.0, -10.0, v.bounds.top)))
    got = spatialstats.number_effective_samples(v, params, rasterize_resolution=10.0, subsample=200, random_state=3)
    want = spatialstats.number_effective_samples(res_mask, params, rasterize_resolution=10.0, subsample=200, random_state=3)
    assert got == want and np.isfinite(got) and got >= 1
    # a raster gives its own grid; distances are the same as the relative ones of the mask route on that grid
    raster = DEM(np.ones(shape, np.float32), t6)
    on_grid = vo.mask([v.tables()], shape, t6)
    got = spatialstats.number_effective_samples(v, params, rasterize_resolution=raster, subsample=200, random_state=3)
    want = spatialstats.number_effective_samples(on_grid, params, rasterize_resolution=10.0, subsample=200, random_state=3)
    assert np.isclose(got, want, rtol=1e-9)
    errors = DEM(np.full(shape, 2.0, np.float32), t6)
    se_v = spatialstats.spatial_error_propagation([v], errors, params, subsample=200, random_state=3)
    se_m = spatialstats.spatial_error_propagation([on_grid], errors, params, subsample=200, random_state=3)
    assert np.isclose(se_v[0], se_m[0], rtol=1e-9)


def test_stage_events_leave_the_planes_alone():
    from xdem_amd import vector

    shape, t6 = vcs.grid(96, 128)
    geom = vcs.star_with_hole(shape, t6)
    ctx = _ctx()
    _, m0, l0 = check([geom], shape, t6)
    assert vector.DeviceRasterizer.stage_ms() == [0.0] * 5   # (no events without the switch)
    ctx.set_option("vec_stage_times", 1)
    try:
        _, m1, l1 = check([geom], shape, t6, device=True)
        ms = vector.DeviceRasterizer.stage_ms()
    finally:
        ctx.set_option("vec_stage_times", 0)
    assert np.array_equal(m0, m1) and np.array_equal(l0, l1)
    assert len(ms) == 5 and all(v >= 0.0 for v in ms) and sum(ms) > 0.0
