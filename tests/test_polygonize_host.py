"""The rule of xdemhip_label and xdemhip_outlines on the CPU (tests/polygonize_oracle.py): the flood fill equals
``scipy.ndimage.label`` bit for bit on 0/1 masks, the rings satisfy the invariants the header states and an even-odd fill of them gives
every component's pixels back; the host-only ``xdemhip_label_plan``; the arguments refused without a GPU; and ``polygonize`` with the
oracle standing in for the device calls."""
import functools

import numpy as np
import pytest
import scipy.ndimage

import polygonize_cases as pc
import polygonize_oracle as po
from xdem_amd import DEM, Vector, _lib, polygonize, vector

STRUCTURE = {4: scipy.ndimage.generate_binary_structure(2, 1), 8: scipy.ndimage.generate_binary_structure(2, 2)}


@functools.lru_cache(maxsize=None)
def oracle(switch, name, connectivity):
    cls = pc.case(switch, name)
    lab, K = po.label(cls, connectivity)
    lab.setflags(write=False)
    return cls, lab, K, po.rings_of(lab)


ALL = [(s, name, c) for s in pc.SWITCHES for name, _ in pc.cases(s) for c in pc.CONNECTIVITIES]


def test_flood_fill_equals_scipy_on_masks():
    for s, name, c in ALL:
        cls, _, _, _ = oracle(s, name, c)
        mask = (cls != 0).astype(np.int32)
        lab, K = po.label(mask, c)
        want, n = scipy.ndimage.label(mask, structure=STRUCTURE[c])
        assert K == n and lab.dtype == np.int32 and np.array_equal(lab, want), (s, name, c)
    rng = np.random.default_rng(5)
    for _ in range(60):   # (and on small random masks of every density)
        mask = (rng.random((rng.integers(1, 14), rng.integers(1, 14))) < rng.random()).astype(np.uint8)
        for c in pc.CONNECTIVITIES:
            want, n = scipy.ndimage.label(mask, structure=STRUCTURE[c])
            lab, K = po.label(mask, c)
            assert K == n and np.array_equal(lab, want)


def test_components_join_equal_classes_only_and_the_table_describes_them():
    for s in pc.SWITCHES:
        for name in ("two_classes", "random_classes", "diagonals", "tile_corner_pairs"):
            for c in pc.CONNECTIVITIES:
                cls, lab, K, _ = oracle(s, name, c)
                assert np.array_equal(lab != 0, cls != 0)
                t = po.table(cls, lab, K)
                want = 0
                for v in np.unique(cls[cls != 0]):   # (per class the components are SciPy's, numbered together in raster order)
                    want += scipy.ndimage.label(cls == v, structure=STRUCTURE[c])[1]
                assert K == want and t[1].sum() == np.count_nonzero(cls)
                first = t[6]
                assert np.all(np.diff(first) > 0) and np.array_equal(lab.reshape(-1)[first], np.arange(1, K + 1))
                assert np.array_equal(cls.reshape(-1)[first], t[0])
    cls, lab, K, _ = oracle(0, "tile_corner_pairs", 4)
    assert K == 6 and oracle(0, "tile_corner_pairs", 8)[2] == 3


def test_ring_invariants():
    for s, name, c in ALL:
        cls, lab, K, rings = oracle(s, name, c)
        W = lab.shape[1]
        counts = np.bincount(lab.reshape(-1), minlength=K + 1)
        by_label = {}
        for label, leader, verts in rings:
            by_label.setdefault(label, []).append((leader, verts))
        assert sorted(by_label) == list(range(1, K + 1)), (s, name, c)
        order = [(label, leader) for label, leader, _ in rings]
        assert order == sorted(order)
        for label, group in by_label.items():
            areas = [po.signed_area(v) for _, v in group]
            assert areas[0] > 0 and all(a < 0 for a in areas[1:]), (s, name, c, label)   # one exterior, placed first; holes after
            assert sum(areas) == counts[label], (s, name, c, label)
            first = int(np.flatnonzero(lab.reshape(-1) == label)[0])
            assert group[0][0] == 4 * first and group[0][1][0] == divmod(first, W)   # the top side of the first pixel ends at its corner
            for leader, verts in group:
                v = np.asarray(verts)
                assert len(verts) >= 4 and len(verts) % 2 == 0
                if c == 4:
                    assert len(set(verts)) == len(verts), (s, name, label)   # no vertex twice
                step = np.roll(v, -1, axis=0) - v
                assert np.all((step[:, 0] == 0) != (step[:, 1] == 0))   # axis-parallel edges of non-zero length
                assert np.all((step[:, 0] == 0) != (np.roll(step, -1, axis=0)[:, 0] == 0))   # and never two collinear in a row
                assert verts[0] == po.end_vertex(*divmod(leader // 4, W), leader % 4)   # the stated start vertex
    assert any(len(set(v)) < len(v) for _, _, v in oracle(0, "tile_corner_pairs", 8)[3]), "a ring that touches itself under connectivity 8"


def test_even_odd_fill_of_the_rings_gives_the_pixels_back():
    for s, name, c in ALL:
        cls, lab, K, rings = oracle(s, name, c)
        for label in range(1, K + 1):
            verts = [v for lb, _, v in rings if lb == label]
            assert np.array_equal(po.even_odd_fill(verts, lab.shape), lab == label), (s, name, c, label)
            if K > 40 and label >= 12:
                break   # (planes of many small components: a dozen of them)


def test_ring_table_layout():
    cls, lab, K, rings = oracle(2, "nested", 4)
    t = po.outlines(lab, K, pc.TRANSFORM)
    a, _, c0, _, e, f = pc.TRANSFORM
    assert t.xy.shape == (2, t.ring_off[-1]) and t.ring_off[0] == 0 and len(t.poly_of_ring) == len(rings) == len(t.ring_area)
    i, j = rings[0][2][0]
    assert t.xy[0, 0] == c0 + a * j and t.xy[1, 0] == f + e * i
    assert np.all(np.diff(t.poly_of_ring) >= 0) and t.ring_area[0] > 0


def test_label_plan_and_its_refusals():
    L = _lib.lib()
    for switch in pc.SWITCHES:
        for H, W in ((1, 1), (7, 9), (131, 133), (20000, 20000), (1, 2 ** 31 - 1)):
            p = polygonize.label_plan(H, W, switch)
            tr, tc = p["tile_rows"], p["tile_cols"]
            assert (tr, tc) == ((2, 2) if switch == 2 else (64, 64))
            assert p["tiles_r"] == -(-H // tr) and p["tiles_c"] == -(-W // tc)
            assert p["lds_bytes"] == tr * tc * 8 and p["lds_bytes"] <= p["lds_budget"] == 160 * 1024
    for H, W, switch in ((0, 5, 0), (5, 0, 0), (-1, 5, 0), (1 << 16, 1 << 15, 0), (1 << 31, 1, 0), (46341, 46341, 0), (5, 5, 1), (5, 5, 3), (5, 5, -1)):
        assert L.xdemhip_label_plan(H, W, switch, None, None, None, None, None, None) == -1, (H, W, switch)
    assert L.xdemhip_label_plan(46340, 46340, 0, None, None, None, None, None, None) == 0
    # without a context every call is refused before it reads an argument
    assert L.xdemhip_label(None, None, _lib.U8, 4, 4, 4, None, None, 0, _lib.HOST, None) == -1
    assert L.xdemhip_outlines(None, None, 4, 4, 0, None, None, 0, None, None, None, 0, _lib.HOST, None, None) == -1


def test_python_refusals():
    with pytest.raises(ValueError, match="connectivity must be 4 or 8"):
        polygonize.label(np.ones((3, 3), np.uint8), connectivity=6)
    with pytest.raises(ValueError, match="bool or an integer dtype"):
        polygonize.label(np.ones((3, 3), np.float32))
    with pytest.raises(ValueError, match="2-D"):
        polygonize.label(np.ones(3, np.uint8))
    with pytest.raises(ValueError, match="fit int32"):
        polygonize.class_plane(np.full((2, 2), 2 ** 40))
    with pytest.raises(NotImplementedError, match="north-up"):
        polygonize.outlines(np.ones((3, 3), np.int32), (1.0, 0.1, 0.0, 0.0, -1.0, 0.0), K=1)
    with pytest.raises(ValueError, match="target_values"):
        polygonize.target_mask(np.ones((3, 3)), "some")
    assert polygonize.class_plane(np.ones((2, 2), bool)).dtype == np.uint8 and polygonize.class_plane(np.ones((2, 2), np.int64)).dtype == np.int32


@pytest.fixture
def oracle_engine(monkeypatch):
    monkeypatch.setattr(polygonize, "_ENGINE", po.OracleEngine())


class HostTargets:
    """``xdemhip_edt_targets``' rule in NumPy, for the proximity engine that ``target_mask`` asks."""

    def targets(self, raster, values=None, ctx=None):
        a = np.asarray(raster, dtype=np.float64)
        return np.isin(a, np.asarray(values, dtype=np.float64)).astype(np.uint8)


def test_target_values_and_the_vector_on_the_oracle_engine(oracle_engine, monkeypatch):
    from xdem_amd import proximity

    monkeypatch.setattr(proximity, "_ENGINE", HostTargets())
    data = np.array([[1.0, 1.0, 0.0, 5.0, 5.0],
                     [1.0, np.nan, 0.0, 5.0, -9999.0],
                     [2.0, 2.0, 0.0, 0.0, 3.0],
                     [2.0, 7.0, 7.0, 0.0, 3.0]], np.float32)
    dem = DEM(data, pc.ROUND_TRIP_TRANSFORM, crs="EPSG:32633", nodata=-9999.0)
    assert np.isnan(dem.data[1, 4])
    tm = polygonize.target_mask
    assert np.array_equal(tm(dem.data, "all", dem.nodata), np.isfinite(dem.data))
    assert np.array_equal(tm(np.array([[1, -9999]]), "all", -9999), [[True, False]])
    assert np.array_equal(tm(dem.data, 5), data == 5) and np.array_equal(tm(dem.data, 5.0), data == 5)
    assert np.array_equal(tm(dem.data, (1, 5)), (data > 1) & (data < 5))
    assert np.array_equal(tm(dem.data, [1, 7, 3]), np.isin(data, [1, 7, 3]))
    assert np.array_equal(tm(dem.data, np.array([2.0])), data == 2)

    v = dem.polygonize()
    assert isinstance(v, Vector) and v.crs == "EPSG:32633"
    assert len(v) == 1 and list(v.ds.columns) == ["id", "raster_value", "geometry"] and v.ds["id"].tolist() == [0] and v.ds["raster_value"].tolist() == [1]
    assert len(v.ds["geometry"][0]) == 2   # the exterior, notched at the nodata pixel on the raster's edge, and the hole at the NaN
    v = dem.polygonize(target_values=[1, 7, 3], data_column_name="glacier")
    assert v.ds["glacier"].tolist() == [0, 1, 2] and all(len(g) == 1 for g in v.ds["geometry"])
    a, _, c0, _, e, f = pc.ROUND_TRIP_TRANSFORM
    assert np.array_equal(v.ds["geometry"][0][0], [[c0, f], [c0, f + 2 * e], [c0 + a, f + 2 * e], [c0 + a, f + e], [c0 + 2 * a, f + e], [c0 + 2 * a, f]])
    xy, ring_off, owner, P = v.tables()
    assert P == 3 and xy.shape == (2, ring_off[-1]) and owner.tolist() == [0, 1, 2]
    assert len(dem.polygonize(target_values=(100, 200))) == 0
    assert len(dem.polygonize(target_values=0, connectivity=8)) == 1 and len(dem.polygonize(target_values=0)) == 1
    with pytest.raises(NotImplementedError, match="integer raster"):
        dem.polygonize(by_value=True)
    idem = DEM(np.array([[4, 4, 0], [0, 4, 9], [9, 0, 9]], np.int32), pc.ROUND_TRIP_TRANSFORM)
    v = idem.polygonize(by_value=True)
    assert v.ds["raster_value"].tolist() == [4, 0, 0, 9, 9, 0] and v.ds["id"].tolist() == list(range(6))
    assert idem.polygonize(by_value=True, connectivity=8).ds["raster_value"].tolist() == [4, 0, 0, 9, 9]
    assert idem.polygonize(target_values=[4, 9], by_value=True).ds["raster_value"].tolist() == [4, 9, 9]
    with pytest.raises(NotImplementedError, match="north-up"):
        DEM(data, (30.0, 1.0, 0.0, 0.0, -30.0, 0.0)).polygonize()

    mask = np.isin(data, [1, 7])
    vm = Vector.from_mask(mask, dem)
    assert len(vm) == 2 and vm.ds["id"].tolist() == [0, 1] and vm.crs == "EPSG:32633"
    with pytest.raises(ValueError, match="boolean mask"):
        Vector.from_mask(mask.astype(np.uint8), dem)
    labels, K, table = polygonize.label(mask)
    assert K == 2 and list(table.columns) == list(polygonize.TABLE_COLUMNS) and table.index.tolist() == [1, 2]
    assert table.loc[1].tolist() == [1, 3, 0, 1, 0, 1, 0] and table.loc[2].tolist() == [1, 2, 3, 3, 1, 2, 16]
    rings = polygonize.outlines(mask, dem.transform)
    assert rings.K == 2 and rings.ring_area.tolist() == [3, 2]
