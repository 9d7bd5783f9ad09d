"""xdem_amd.Vector without a GPU: every accepted geometry form, the table and its queries, the messages, the grid made from ``res``,
and the added Vector branch of every consumer with the rule's NumPy restatement (vector_oracle.OracleRasterizer) in the rasteriser's
place.  The restatement itself is held to an independent implementation: matplotlib's point-in-polygon test on the pixel centres,
XOR-ed over the rings of a polygon, on EVERY pixel (the generators keep every centre at least 1e-6 pixel from every edge)."""
import json
import warnings

import numpy as np
import pandas as pd
import pytest

import demcollection_cases as dc
import demstack_oracle
import vector_cases as vcs
import vector_oracle as vo
from xdem_amd import DEM, DEMCollection, Vector, dDEM, spatialstats, vector


# ---- the oracle against matplotlib ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", vcs.SHAPES)
def test_oracle_agrees_with_matplotlib_on_every_pixel(shape):
    shape, t6 = vcs.grid(*shape)
    ext, holes = vcs.star_with_hole(shape, t6)
    polygons = [[ext] + holes] + [[s] for s in vcs.strips(shape, t6)] + [[vcs.comb(t6, 5, 5.3, 10.2, 40.6, 50.4, 12.5, salt=5)]]
    for rings in polygons:
        assert vcs.min_centre_to_edge(rings, shape, t6) >= 1e-6
        got, want = vo.rings_mask(rings, shape, t6), vcs.mpl_mask(rings, shape, t6)
        assert np.array_equal(got, want), int((got != want).sum())
    assert 0 < vo.rings_mask(polygons[0], shape, t6).sum() < shape[0] * shape[1]


@pytest.mark.parametrize("shape", vcs.SHAPES)
def test_seven_strips_cover_every_pixel_exactly_once(shape):
    shape, t6 = vcs.grid(*shape)
    strips = vcs.strips(shape, t6)
    cover = sum(vo.rings_mask([s], shape, t6).astype(np.int32) for s in strips)
    assert cover.min() == cover.max() == 1
    with vo.patched():
        lab = Vector(strips).rasterize((shape, t6))
        order = [4, 0, 6, 2, 5, 1, 3]
        lab2 = Vector([strips[k] for k in order]).rasterize((shape, t6), in_value=[k + 1 for k in order])
    assert np.array_equal(lab, lab2) and set(np.unique(lab)) == set(range(1, 8))


# ---- parsing ----------------------------------------------------------------------------------------------------------------------------
class _Coords:
    def __init__(self, ring):
        self.coords = [tuple(p) for p in ring]


class _Polygon:
    geom_type = "Polygon"

    def __init__(self, ext, holes=()):
        self.exterior, self.interiors = _Coords(ext), [_Coords(h) for h in holes]


class _Multi:
    geom_type = "MultiPolygon"

    def __init__(self, parts):
        self.geoms = parts


class _Line:
    geom_type = "LineString"


def _shapes():
    shape, t6 = vcs.grid(61, 83)
    outer, hole = vcs.rect(t6, 8.4, 70.3, 6.7, 52.2), vcs.rect(t6, 20.6, 50.2, 15.3, 40.9, ccw=False)
    other = vcs.rect(t6, 72.2, 80.1, 3.3, 9.9)
    return shape, t6, outer, hole, other


def test_every_geometry_form_gives_the_same_table():
    shape, t6, outer, hole, other = _shapes()
    closed = lambda r: np.concatenate([r, r[:1]]).tolist()   # noqa: E731  (GeoJSON closes its rings)
    forms = {
        "arrays": [(outer, [hole]), other],
        "lists": [(outer.tolist(), [hole.tolist()]), other.tolist()],
        "geojson": [{"type": "Polygon", "coordinates": [closed(outer), closed(hole)]}, {"type": "Polygon", "coordinates": [closed(other)]}],
        "features": [{"type": "Feature", "properties": {}, "geometry": {"type": "Polygon", "coordinates": [closed(outer), closed(hole)]}},
                     {"type": "Feature", "properties": {}, "geometry": {"type": "Polygon", "coordinates": [closed(other)]}}],
        "shapely": [_Polygon(outer, [hole]), _Polygon(other)],
    }
    want = vo.rings_mask([outer, hole], shape, t6) | vo.rings_mask([other], shape, t6)
    with vo.patched():
        for name, geoms in forms.items():
            v = Vector(geoms)
            assert len(v) == 2 and v.tables()[3] == 2 and list(v.tables()[2]) == [0, 0, 1], name
            assert np.array_equal(v.create_mask((shape, t6)), want), name
        multi = {
            "list": [[(outer, [hole]), other]],
            "geojson": [{"type": "MultiPolygon", "coordinates": [[closed(outer), closed(hole)], [closed(other)]]}],
            "shapely": [_Multi([_Polygon(outer, [hole]), _Polygon(other)])],
            "single geometry": _Multi([_Polygon(outer, [hole]), _Polygon(other)]),
        }
        for name, geoms in multi.items():
            v = Vector(geoms)
            assert len(v) == 1 and list(v.tables()[2]) == [0, 0, 0], name
            assert np.array_equal(v.create_mask((shape, t6)), want), name
            assert set(np.unique(v.rasterize((shape, t6)))) == {0, 1}
    assert Vector(outer).tables()[0].shape == (2, 4) and Vector(outer).tables()[0].dtype == np.float64
    assert Vector([np.concatenate([outer, outer[:1]])]).tables()[0].shape == (2, 5)   # (a closing vertex stays: its edge has length 0)
    # degenerate rings (fewer than three DISTINCT vertices) contribute nothing
    line = np.array([(0.0, 0.0), (5.0, 5.0), (0.0, 0.0), (5.0, 5.0)])
    assert Vector([line]).tables()[0].shape == (2, 0) and len(Vector([line])) == 1
    assert list(Vector([(outer, [line])]).tables()[1]) == [0, 4]


def test_feature_collections_tables_and_queries(tmp_path):
    shape, t6, outer, hole, other = _shapes()
    closed = lambda r: np.concatenate([r, r[:1]]).tolist()   # noqa: E731
    fc = {"type": "FeatureCollection", "features": [
        {"type": "Feature", "properties": {"name": "north", "area_km2": 3.5}, "geometry": {"type": "Polygon", "coordinates": [closed(outer), closed(hole)]}},
        {"type": "Feature", "properties": {"name": "south", "area_km2": 0.7}, "geometry": {"type": "Polygon", "coordinates": [closed(other)]}}]}
    path = tmp_path / "outlines.geojson"
    path.write_text(json.dumps(fc))
    for v in (Vector(fc), Vector.from_geojson(fc), Vector.from_geojson(str(path)), Vector.from_geojson(path), Vector.from_geojson(json.dumps(fc))):
        assert list(v.ds.columns) == ["name", "area_km2", "geometry"] and list(v.ds["name"]) == ["north", "south"]
        assert isinstance(v.ds, pd.DataFrame) and len(v.ds["geometry"].iloc[0]) == 2
    v = Vector(fc, crs="EPSG:32633")
    small = v.query("area_km2 < 1")
    assert len(small) == 1 and small.crs == "EPSG:32633" and list(small.ds["name"]) == ["south"]
    again = Vector(v.ds.query("name == 'north'"))   # (as upstream's DEMCollection filters outlines)
    ring = lambda r: np.concatenate([r, r[:1]])   # noqa: E731  (the closing vertex of a GeoJSON ring stays in the table)
    assert len(again) == 1 and np.array_equal(again.tables()[0], Vector([(ring(outer), [ring(hole)])]).tables()[0])
    picked = v[np.array([False, True])]
    assert np.array_equal(picked.tables()[0], small.tables()[0])
    with pytest.raises(TypeError, match="boolean mask"):
        v[0]
    c = v.copy()
    assert c is not v and c.ds is not v.ds and list(c.ds["name"]) == ["north", "south"] and np.array_equal(c.tables()[0], v.tables()[0])
    b = v.bounds
    allxy = np.concatenate([outer, hole, other])
    assert (b.left, b.bottom, b.right, b.top) == (allxy[:, 0].min(), allxy[:, 1].min(), allxy[:, 0].max(), allxy[:, 1].max())
    assert tuple(b) == (b.left, b.bottom, b.right, b.top)
    t = Vector([outer, other], table={"id": [10, 20]})
    assert list(t.ds["id"]) == [10, 20]
    with vo.patched():   # in_value defaults to index + 1 of the TABLE, which a query keeps
        assert set(np.unique(small.rasterize((shape, t6)))) == {0, 2}


def test_messages():
    shape, t6, outer, hole, other = _shapes()
    with pytest.raises(NotImplementedError, match="geometry type 'LineString' is not supported"):
        Vector([_Line()])
    with pytest.raises(NotImplementedError, match="geometry type 'Point' is not supported"):
        Vector([{"type": "Point", "coordinates": [1.0, 2.0]}])
    bad = outer.copy()
    bad[1, 0] = np.nan
    with pytest.raises(ValueError, match="must be finite"):
        Vector([bad])
    bad[1, 0] = np.inf
    with pytest.raises(ValueError, match="must be finite"):
        Vector([(outer, [bad])])
    with pytest.raises(ValueError, match="2 rows for 1 geometries"):
        Vector([outer], table={"id": [1, 2]})
    v = Vector([outer])
    for t in ((10.0, 0.5, 0.0, 0.0, -10.0, 0.0), (10.0, 0.0, 0.0, 0.5, -10.0, 0.0), (10.0, 0.0, 0.0, 0.0, 10.0, 0.0), (-10.0, 0.0, 0.0, 0.0, -10.0, 0.0)):
        with pytest.raises(NotImplementedError, match=r"only north-up transforms \(b = d = 0\) are supported"):
            v.create_mask((shape, t))
        with pytest.raises(NotImplementedError, match=r"only north-up transforms \(b = d = 0\) are supported"):
            v.rasterize(DEM(np.zeros(shape, np.float32), t))
    with pytest.raises(ValueError, match="needs a raster, or a resolution"):
        v.create_mask()
    with vo.patched():
        with pytest.raises(ValueError, match="in_value has 3 values for 1 polygons"):
            v.rasterize((shape, t6), in_value=[1, 2, 3])
        with pytest.raises(ValueError, match="integers that fit int32"):
            v.rasterize((shape, t6), in_value=1.5)
        with pytest.raises(ValueError, match="integers that fit int32"):
            v.rasterize((shape, t6), out_value=2 ** 31)


def test_grid_from_res_and_the_kinds_of_raster():
    shape, t6, outer, hole, other = _shapes()
    v = Vector([(outer, [hole]), other])
    b = v.bounds
    with vo.patched():
        for res in (10.0, 7.0, (13.0, 4.0)):
            rx, ry = (res, res) if np.ndim(res) == 0 else res
            m = v.create_mask(res=res)
            want_shape = (int(np.ceil((b.top - b.bottom) / ry)), int(np.ceil((b.right - b.left) / rx)))
            assert m.shape == want_shape and m.dtype == np.bool_
            assert np.array_equal(m, vo.mask([v.tables()], want_shape, (rx, 0.0, b.left, 0.0, -ry, b.top)))
        box = (b.left - 35.0, b.bottom - 5.0, b.right + 1.0, b.top + 20.0)
        m = v.create_mask(res=10.0, bounds=box)
        assert m.shape == (int(np.ceil((box[3] - box[1]) / 10.0)), int(np.ceil((box[2] - box[0]) / 10.0)))
        assert np.array_equal(m, vo.mask([v.tables()], m.shape, (10.0, 0.0, box[0], 0.0, -10.0, box[3])))
        want = vo.mask([v.tables()], shape, t6)
        dem = DEM(np.zeros(shape, np.float32), t6)
        dd = dDEM.from_array(np.zeros(shape, np.float32), t6, None, np.datetime64("2000-01-01"), np.datetime64("2001-01-01"))
        for raster in (dem, dd, (shape, t6)):
            assert np.array_equal(v.create_mask(raster), want)
        as_dem = v.create_mask(dem, as_array=False)
        assert isinstance(as_dem, DEM) and as_dem.transform == t6 and np.array_equal(as_dem.data, want)
        n = vo.OracleRasterizer.calls
        assert v.create_mask(dem) is v.create_mask((shape, t6))   # kept per (vector, shape, transform)
        assert vo.OracleRasterizer.calls == n
        lab = v.rasterize(dem, in_value=[5, 9], out_value=-1)
        assert lab.dtype == np.int32 and set(np.unique(lab)) == {-1, 5, 9} and np.array_equal(lab != -1, want)
        assert set(np.unique(v.rasterize(dem, in_value=4))) == {0, 4}


# ---- the consumers ------------------------------------------------------------------------------------------------------------------------
def _outlines():
    shape = dc.SHAPES[0]
    a = vcs.star(shape, dc.TRANSFORM, n=13, salt=31, centre=(0.4 * shape[1], 0.45 * shape[0]), r_out=0.45 * shape[0], r_in=0.25 * shape[0])
    b = vcs.star(shape, dc.TRANSFORM, n=11, salt=32, centre=(0.6 * shape[1], 0.55 * shape[0]), r_out=0.4 * shape[0], r_in=0.2 * shape[0])
    return shape, a, b


def _collection(outlines):
    H, W = dc.SHAPES[0]
    s = dc.stack(H, W, "float32")
    col = DEMCollection([DEM.from_array(d, dc.TRANSFORM, None) for d in s["dems"]], timestamps=dc.stamps(), outlines=outlines, reference_dem=dc.REFERENCE)
    col.subtract_dems()
    return col


def test_collection_takes_vectors_for_every_mask():
    shape, a, b = _outlines()
    va, vb = Vector([a]), Vector([b])
    ma, mb = vo.mask([va.tables()], shape, dc.TRANSFORM), vo.mask([vb.tables()], shape, dc.TRANSFORM)
    stamps = dc.stamps()
    with demstack_oracle.patched(), vo.patched(), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        col = _collection(va)
        assert all(np.array_equal(col.get_ddem_mask(d), ma) for d in col.ddems)
        col_v = _collection({stamps[0]: va, stamps[1]: vb})
        col_m = _collection({stamps[0]: ma, stamps[1]: mb})
        masks = [col_v.get_ddem_mask(d) for d in col_v.ddems]
        assert np.array_equal(masks[0], ma | mb) and np.array_equal(masks[1], mb) and np.array_equal(masks[2], mb)
        n = vo.OracleRasterizer.calls
        assert np.shares_memory(col_v.get_ddem_mask(col_v.ddems[0]), masks[0]) and vo.OracleRasterizer.calls == n   # burnt once, kept
        filled_v, filled_m = col_v.interpolate_ddems("regional_hypsometric"), col_m.interpolate_ddems("regional_hypsometric")
        assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(filled_v, filled_m))
        assert col_v.get_dh_series(nans_ok=True).equals(col_m.get_dh_series(nans_ok=True))
        assert col_v.get_dv_series(nans_ok=True).equals(col_m.get_dv_series(nans_ok=True))
        assert col_v.get_cumulative_series("dv", nans_ok=True).equals(col_m.get_cumulative_series("dv", nans_ok=True))
        # a Vector next to a boolean array: each as it is
        col_x = _collection({stamps[0]: va, stamps[1]: mb})
        assert np.array_equal(col_x.get_ddem_mask(col_x.ddems[0]), ma | mb)


def test_outlines_filter_queries_vectors_and_keeps_refusing_arrays():
    shape, a, b = _outlines()
    v = Vector([a, b], table={"name": ["north", "south"], "area_km2": [3.5, 0.7]})
    mb = vo.mask([Vector([b]).tables()], shape, dc.TRANSFORM)
    stamps = dc.stamps()
    with demstack_oracle.patched(), vo.patched(), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        col = _collection(v)
        assert np.array_equal(col.get_ddem_mask(col.ddems[0], outlines_filter="area_km2 < 1"), mb)
        assert col.get_dh_series(outlines_filter="name == 'south'", nans_ok=True).equals(col.get_dh_series(mask=mb, nans_ok=True))
        assert col.get_cumulative_series("dh", outlines_filter="name == 'south'", nans_ok=True).equals(col.get_cumulative_series("dh", mask=mb, nans_ok=True))
        for outlines in (mb, {stamps[0]: v, stamps[1]: mb}, None):
            col = _collection(outlines)
            with pytest.raises(NotImplementedError, match="pandas query"):
                col.get_ddem_mask(col.ddems[0], outlines_filter="area_km2 < 1")
            with pytest.raises(NotImplementedError, match="pandas query"):
                col.get_dh_series(outlines_filter="area_km2 < 1")


def test_ddem_interpolate_takes_a_vector_mask():
    import volume_oracle
    from xdem_amd import ddem as ddem_mod

    shape, a, _ = _outlines()
    s = dc.stack(*shape, "float32")
    v = Vector([a])
    ma = vo.mask([v.tables()], shape, dc.TRANSFORM)
    two = dc.stamps((2000, 2010))
    with np.errstate(invalid="ignore"):
        dd = (s["dems"][1] - s["dems"][0]).astype(np.float32)

    def filled(mask):
        one = dDEM.from_array(dd.copy(), dc.TRANSFORM, None, two[0], two[1])
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            return one.interpolate(method="regional_hypsometric", reference_elevation=s["ref"], mask=mask)

    with volume_oracle.patched(), vo.patched():
        assert np.array_equal(filled(v), filled(ma), equal_nan=True)
        one = dDEM.from_array(dd.copy(), dc.TRANSFORM, None, two[0], two[1])
        assert np.array_equal(ddem_mod.mask_as_array(v, one), ma)
        with pytest.raises(ValueError, match="needs the raster it is burnt into"):
            ddem_mod.mask_as_array(v)
    with pytest.raises(TypeError, match="Raster has invalid type"):
        ddem_mod.mask_as_array([1, 2])


def test_spatialstats_burns_vector_masks_and_keeps_its_refusals():
    shape, t6 = vcs.grid(61, 83)
    a = vcs.star(shape, t6, n=13, salt=31, centre=(30.0, 28.0), r_out=27.0, r_in=15.0)
    v = Vector([a])
    want = vo.mask([v.tables()], shape, t6)
    dem = DEM(np.ones(shape, np.float32), t6)
    with vo.patched():
        got = spatialstats._burn_vector_masks((v, None), dem)
        assert np.array_equal(got[0], want) and got[1] is None
        arr = np.ones(shape, bool)
        assert spatialstats._burn_vector_masks((arr, "x"), None) == [arr, "x"]   # (anything else as it came, for the callers' checks)
        for fn, kw in ((spatialstats.infer_heteroscedasticity_from_stable, {"dvalues": dem.data, "list_var": [dem.data]}),
                       (spatialstats.infer_spatial_correlation_from_stable, {"dvalues": dem.data, "list_models": ["spherical"], "gsd": 10.0}),
                       (spatialstats.patches_method, {"values": dem.data, "areas": [100.0], "gsd": 10.0})):
            with pytest.raises(ValueError, match="a Vector mask needs the grid"):
                fn(stable_mask=v, **kw)
            with pytest.raises(ValueError, match="a Vector mask needs the grid"):
                fn(unstable_mask=v, **kw)
    # the refusals of everything that is neither an array nor a Vector stand
    with pytest.raises(ValueError, match="boolean arrays"):
        spatialstats.infer_heteroscedasticity_from_stable(dem.data, [dem.data], stable_mask="outlines.shp")
    with pytest.raises(ValueError, match="boolean arrays"):
        spatialstats.infer_spatial_correlation_from_stable(dem.data, ["spherical"], unstable_mask="outlines.shp", gsd=10.0)
    with pytest.raises(NotImplementedError, match="must be boolean arrays here"):
        spatialstats.patches_method(dem.data, [100.0], gsd=10.0, stable_mask="outlines.shp")


def test_number_effective_samples_builds_upstreams_coordinates(monkeypatch):
    shape, t6 = vcs.grid(61, 83)
    a = vcs.star(shape, t6, n=13, salt=31, centre=(30.0, 28.0), r_out=27.0, r_in=15.0)
    v = Vector([a])
    params = pd.DataFrame({"model": ["spherical"], "range": [100.0], "psill": [1.0]})
    seen = {}

    def capture(coords, errors, params_variogram_model, **kw):
        seen["coords"], seen["errors"], seen["kw"] = np.asarray(coords), np.asarray(errors), kw
        return 42.0

    monkeypatch.setattr(spatialstats, "neff_hugonnet_approx", capture)
    with vo.patched():
        assert spatialstats.number_effective_samples(v, params, rasterize_resolution=10.0, subsample=50) == 42.0
        mask = v.create_mask(res=10.0)
        x, y = 10.0 * np.arange(mask.shape[0]), 10.0 * np.arange(mask.shape[1])
        assert np.array_equal(seen["coords"], np.array(np.meshgrid(y, x))[:, mask].T) and seen["kw"] == {"subsample": 50}
        assert np.array_equal(seen["errors"], np.ones(mask.sum()))
        via_mask = dict(seen)
        spatialstats.number_effective_samples(mask, params, rasterize_resolution=10.0, subsample=50)
        assert np.array_equal(seen["coords"], via_mask["coords"])
        dem = DEM(np.ones(shape, np.float32), t6)
        spatialstats.number_effective_samples(v, params, rasterize_resolution=dem)
        on_grid = vo.mask([v.tables()], shape, t6)
        rows, cols = np.nonzero(on_grid)
        assert np.array_equal(seen["coords"], np.stack([t6[2] + (cols + 0.5) * 10.0, t6[5] - (rows + 0.5) * 10.0], axis=1))
        with pytest.warns(UserWarning, match="20% of the shortest correlation range"):
            spatialstats.number_effective_samples(v, params)
        assert seen["coords"].shape[0] == v.create_mask(res=20.0).sum()
        with pytest.raises(ValueError, match="The rasterize resolution must be a float, integer or Raster subclass."):
            spatialstats.number_effective_samples(v, params, rasterize_resolution="10 m")
        errors = DEM(np.where(on_grid, 2.0, 8.0).astype(np.float32), t6)
        se = spatialstats.spatial_error_propagation([v, on_grid], errors, params, subsample=50)
        assert se[0] == se[1] == 2.0 / np.sqrt(42.0)
        with pytest.raises(ValueError, match="a Vector area needs the errors' grid"):
            spatialstats.spatial_error_propagation([v], errors.data, params)
    for area in ("glacier.shp", [1.0, 2.0], None):
        with pytest.raises(ValueError, match="Area must be a float, integer, Vector subclass or geopandas dataframe."):
            spatialstats.number_effective_samples(area, params)


def test_estimate_uncertainty_takes_a_vector_for_stable_terrain(monkeypatch):
    from xdem_amd import dem as dem_mod

    shape, t6 = vcs.grid(61, 83)
    a = vcs.star(shape, t6, n=13, salt=31, centre=(30.0, 28.0), r_out=27.0, r_in=15.0)
    v = Vector([a])
    want = vo.mask([v.tables()], shape, t6)
    seen = {}

    def capture(**kw):
        seen.update(kw)
        return None, None, "corr"

    monkeypatch.setattr(dem_mod._ss, "infer_spatial_correlation_from_stable", capture)
    rng = np.random.default_rng(0)
    one, other = DEM(rng.normal(size=shape).astype(np.float32), t6), DEM(rng.normal(size=shape).astype(np.float32), t6)
    with vo.patched():
        sig, corr = one.estimate_uncertainty(other, stable_terrain=v, approach="Basic", spread_estimator=np.std, list_vario_models="spherical")
    assert corr == "corr" and np.array_equal(seen["stable_mask"], want) and seen["stable_mask"].dtype == np.bool_
    assert np.all(sig.data == np.std((other.data - one.data)[want]))
