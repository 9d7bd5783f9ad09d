"""xdemhip_label, xdemhip_label_table and xdemhip_outlines on the GPU against the restatement of their rule (tests/polygonize_oracle.py):
label plane, K, component table and ring arrays bit for bit -- from host and device memory, for uint8 and int32 classes, from two runs,
under both connectivities and both values of the test switch ``"ccl_route"`` (0 automatic tiles, 2 minimal tiles).  Then the launch
counts, the round trip through ``xdemhip_rasterize`` (the polygons burnt again give the label plane back), the status codes of refused
arguments, and ``DEM.polygonize`` / ``Vector.from_mask`` end to end.  The planes come from tests/polygonize_cases.py, sized from
``xdemhip_label_plan``: (2 T_r + 3) x (2 T_c + 5), the smallest that has nine partial tiles."""
import ctypes
import functools

import numpy as np
import pytest

import polygonize_cases as pc
import polygonize_oracle as po
from gpu_helpers import _dev
from xdem_amd import DEM, Vector, _args, _lib, polygonize

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    return _lib.default_context()


@functools.lru_cache(maxsize=None)
def oracle(switch, name, connectivity):
    """(classes, labels, K, table, ring table) of a case: computed once, read-only, shared among the tests."""
    cls = pc.case(switch, name)
    lab, K = po.label(cls, connectivity)
    t = po.table(cls, lab, K)
    rings = po.outlines(lab, K, pc.TRANSFORM)
    for a in (lab, t) + tuple(rings[:4]):
        a.setflags(write=False)
    return cls, lab, K, t, rings


def host(x):
    return x.cpu().numpy() if _args.is_tensor(x) else x


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def same_rings(got, want) -> bool:
    got = [host(a) for a in got[:4]]
    return got[0].dtype == np.float64 and got[0].shape == want.xy.shape and np.array_equal(bits(got[0]), bits(want.xy)) and \
        got[1].dtype == np.int64 and np.array_equal(got[1], want.ring_off) and got[2].dtype == np.int32 and \
        np.array_equal(got[2], want.poly_of_ring) and np.array_equal(got[3], want.ring_area)


@pytest.mark.parametrize("connectivity", pc.CONNECTIVITIES)
@pytest.mark.parametrize("switch", pc.SWITCHES)
def test_labels_and_table_bit_for_bit(ctx, switch, connectivity):
    with ctx.option_scope("ccl_route", switch):
        for name, _ in pc.cases(switch):
            cls, lab, K, t, _ = oracle(switch, name, connectivity)
            first = None
            for dtype in (np.int32, np.uint8):
                for device in (False, True):
                    plane = cls.astype(dtype)
                    got, k, table = polygonize.label(_dev(plane) if device else plane, connectivity, ctx=ctx)
                    assert _args.is_tensor(got) == device
                    got = host(got)
                    what = (name, dtype.__name__, "device" if device else "host")
                    assert k == K and got.dtype == np.int32 and np.array_equal(got, lab), what
                    assert table.shape == (K, 7) and np.array_equal(table.to_numpy().T, t), what
                    if first is None:
                        first = got
            again = host(polygonize.label(cls, connectivity, ctx=ctx)[0])
            assert np.array_equal(again, first), (name, "second run")
    assert oracle(switch, "all_background", connectivity)[2] == 0
    assert oracle(switch, "all_foreground", connectivity)[2] == 1
    assert oracle(switch, "checkerboard", connectivity)[2] == (1 if connectivity == 8 else (pc.case(switch, "checkerboard") != 0).sum())
    assert oracle(switch, "serpentine", connectivity)[2] == 1 and oracle(switch, "spiral", connectivity)[2] == 1


@pytest.mark.parametrize("connectivity", pc.CONNECTIVITIES)
@pytest.mark.parametrize("switch", pc.SWITCHES)
def test_rings_bit_for_bit(ctx, switch, connectivity):
    for name, _ in pc.cases(switch):
        cls, lab, K, _, want = oracle(switch, name, connectivity)
        got = polygonize.outlines(lab, pc.TRANSFORM, K=K, ctx=ctx)
        assert same_rings(got, want), (name, "host labels")
        dev = polygonize.outlines(_dev(lab), pc.TRANSFORM, K=K, ctx=ctx)
        assert all(_args.is_tensor(a) for a in dev[:4]) and same_rings(dev, want), (name, "device labels")
        assert same_rings(polygonize.outlines(lab, pc.TRANSFORM, K=K, ctx=ctx), want), (name, "second run")
        with ctx.option_scope("ccl_route", switch):   # (a class plane: labelled first, under the switch)
            assert same_rings(polygonize.outlines(cls, pc.TRANSFORM, connectivity, ctx=ctx), want), (name, "from classes")
    empty = oracle(switch, "all_background", connectivity)[4]
    assert empty.xy.shape == (2, 0) and empty.ring_off.tolist() == [0] and empty.poly_of_ring.size == 0
    stairs = oracle(switch, "staircase", connectivity)[4]
    assert stairs.ring_off.tolist() == [0, 2 * pc.case(switch, "staircase").shape[0] + 2] and stairs.ring_off[1] > 256


def test_launch_count_does_not_depend_on_the_components(ctx):
    counts = {}
    for name in ("all_foreground", "checkerboard", "random_0.59"):
        cls = pc.case(0, name)
        labels, K, _ = polygonize.label(cls, 4, ctx=ctx)
        rings = polygonize.outlines(labels, pc.TRANSFORM, K=K, ctx=ctx)
        ms, launches = polygonize.DeviceEngine.stage_ms(ctx)
        counts[name] = (K, len(rings.poly_of_ring), launches)
        assert set(ms) == set(polygonize.STAGES) and all(v >= 0.0 for v in ms.values()) and ms["tile"] > 0.0 and ms["walk"] > 0.0
    assert counts["all_foreground"][:2] == (1, 1) and counts["checkerboard"][0] > 4000
    assert counts["all_foreground"][2] == counts["checkerboard"][2] == counts["random_0.59"][2]
    H, W = pc.case(0, "checkerboard").shape
    rounds = int(np.ceil(np.log2(4 * H * W)))
    assert counts["checkerboard"][2] == (7, 2 * rounds + 10)   # (a jumping round is one launch: log2 of the shape, not of K)


@pytest.mark.parametrize("switch", pc.SWITCHES)
def test_round_trip_through_rasterize(ctx, switch):
    t6 = pc.ROUND_TRIP_TRANSFORM
    for name, _ in pc.cases(switch):
        cls, lab, K, _, _ = oracle(switch, name, 4)
        rings = polygonize.outlines(lab, t6, K=K, ctx=ctx)
        v = polygonize.vector_of(rings, {"id": np.arange(K)})
        assert len(v) == K
        grid = (lab.shape, t6)
        burnt = v.rasterize(grid, in_value=v.ds["id"].to_numpy() + 1)
        assert burnt.dtype == np.int32 and np.array_equal(burnt, lab), name
        assert np.array_equal(v.create_mask(grid), cls != 0), name
        # pixel centres never lie on an edge: the edges run along pixel borders, half a pixel from every centre
        a, _, c0, _, e, f = t6
        assert not np.isin(rings.xy[0], c0 + (np.arange(lab.shape[1]) + 0.5) * a).any() and not np.isin(rings.xy[1], f + (np.arange(lab.shape[0]) + 0.5) * e).any()


def test_refused_arguments_return_status_codes(ctx):
    L = ctx._L
    cls = np.ones((4, 5), np.uint8)
    lab = np.zeros((4, 5), np.int32)
    table = np.zeros((7, 4), np.int64)
    K = ctypes.c_int64()

    def label(classes=cls, dtype=_lib.U8, H=4, W=5, connectivity=4, labels=lab, table=None, capacity=0, memspace=_lib.HOST, k=K):
        return L.xdemhip_label(ctx.handle, _args.ptr(classes), dtype, H, W, connectivity, _args.ptr(labels), _args.ptr(table), capacity, memspace,
                               ctypes.byref(k) if k is not None else None)

    assert label() == _lib.OK and K.value == 1 and np.all(lab == 1)
    assert label(table=table, capacity=4) == _lib.OK and table.reshape(-1)[:7].tolist() == [1, 20, 0, 3, 0, 4, 0]
    for kw in (dict(connectivity=6), dict(connectivity=0), dict(dtype=_lib.F32), dict(dtype=_lib.F64), dict(dtype=9), dict(classes=None), dict(labels=None),
               dict(k=None), dict(H=0), dict(W=-1), dict(H=1 << 16, W=1 << 15), dict(H=46341, W=46341), dict(memspace=3), dict(table=table, capacity=-1)):
        assert label(**kw) == -1, kw
    two = np.array([[1, 0, 1, 0, 1]] * 4, np.uint8)
    assert label(classes=two, table=table, capacity=2) == -1 and K.value == 3 and b"capacity" in L.xdemhip_last_error(ctx.handle)
    assert lab[0].tolist() == [1, 0, 2, 0, 3]   # (the labels and K are written all the same)
    assert L.xdemhip_label_table(ctx.handle, _args.ptr(two), _lib.U8, _args.ptr(lab), 4, 5, 3, _args.ptr(table), _lib.HOST) == _lib.OK
    assert table.reshape(-1)[:3 * 7].reshape(7, 3)[1].tolist() == [4, 4, 4]
    assert L.xdemhip_label_table(ctx.handle, None, _lib.U8, _args.ptr(lab), 4, 5, 3, _args.ptr(table), _lib.HOST) == -1
    assert L.xdemhip_label_table(ctx.handle, _args.ptr(two), _lib.F32, _args.ptr(lab), 4, 5, 3, _args.ptr(table), _lib.HOST) == -1
    assert L.xdemhip_label_table(ctx.handle, _args.ptr(two), _lib.U8, _args.ptr(lab), 4, 5, 21, _args.ptr(table), _lib.HOST) == -1

    V, R = ctypes.c_int64(), ctypes.c_int64()
    xy, off, owner = np.zeros((2, 12)), np.zeros(4, np.int64), np.zeros(3, np.int32)

    def outlines(labels=lab, H=4, W=5, k=3, t6=pc.TRANSFORM, xy=xy, vcap=12, off=off, owner=owner, rcap=3, memspace=_lib.HOST):
        return L.xdemhip_outlines(ctx.handle, _args.ptr(labels), H, W, k, (ctypes.c_double * 6)(*t6) if t6 else None, _args.ptr(xy), vcap, _args.ptr(off),
                                  _args.ptr(owner), None, rcap, memspace, ctypes.byref(V), ctypes.byref(R))

    assert outlines(xy=None, off=None, owner=None) == _lib.OK and (V.value, R.value) == (12, 3)
    assert outlines() == _lib.OK and (V.value, R.value) == (12, 3) and off.tolist() == [0, 4, 8, 12] and owner.tolist() == [0, 1, 2]
    for kw in (dict(labels=None), dict(t6=None), dict(H=0), dict(H=46341, W=46341), dict(t6=(1.0, 0.5, 0.0, 0.0, -1.0, 0.0)), dict(t6=(1.0, 0.0, 0.0, 0.0, 1.0, 0.0)),
               dict(t6=(float("nan"), 0.0, 0.0, 0.0, -1.0, 0.0)), dict(k=-1), dict(k=2), dict(xy=None), dict(vcap=11), dict(rcap=2), dict(memspace=7)):
        assert outlines(**kw) == -1, kw
    assert b"outside 1 .. K" in (outlines(k=2), L.xdemhip_last_error(ctx.handle))[1]
    for value in (1, 3, -1):
        with pytest.raises(_lib.XdemHipError):
            ctx.set_option("ccl_route", value)


def test_polygonize_end_to_end(ctx):
    rng = np.random.default_rng(11)
    H, W = 150, 170
    t6 = pc.ROUND_TRIP_TRANSFORM
    data = rng.integers(0, 5, (H, W)).astype(np.float32)
    data[20:60, 30:90] = 7.0
    data[30:40, 40:60] = 2.0          # a hole of another value in the block of sevens
    data[rng.random((H, W)) < 0.02] = np.nan
    data[100:104, 5:9] = -9999.0
    dem = DEM(data, t6, crs="EPSG:32633", nodata=-9999.0)
    filled = np.nan_to_num(dem.data, nan=-1.0)

    def check(v, mask, connectivity=4):
        lab, K = po.label(mask, connectivity)
        assert isinstance(v, Vector) and len(v) == K and v.crs == "EPSG:32633" and v.ds["id"].tolist() == list(range(K))
        if connectivity == 4:
            assert np.array_equal(v.rasterize(dem, in_value=v.ds["id"].to_numpy() + 1), lab)
        assert np.array_equal(v.create_mask(dem), mask != 0)
        return v

    v = check(dem.polygonize(), np.isfinite(dem.data))
    assert v.ds["raster_value"].tolist() == [1] * len(v)
    check(dem.polygonize(target_values=7), filled == 7)
    check(dem.polygonize(target_values=7.0, connectivity=8), filled == 7, 8)
    check(dem.polygonize(target_values=(1, 4)), (filled > 1) & (filled < 4))
    check(dem.polygonize(target_values=[0, 7, 3]), np.isin(filled, [0, 7, 3]))
    got = dem.polygonize(target_values=[0, 7, 3], data_column_name="glacier")
    assert list(got.ds.columns) == ["glacier", "raster_value", "geometry"]
    sevens = dem.polygonize(target_values=7).ds["geometry"]
    assert max(len(g) for g in sevens) >= 2 and all(len(r) >= 4 for g in sevens for r in g)

    idem = DEM(np.where(np.isfinite(dem.data), dem.data, 9).astype(np.int32), t6, crs="EPSG:32633")
    v = idem.polygonize(by_value=True)
    lab, K = po.label(idem.data + 1, 4)   # (the value 0 is a class as well)
    assert len(v) == K and np.array_equal(v.rasterize(idem, in_value=v.ds["id"].to_numpy() + 1), lab)
    assert np.array_equal(v.ds["raster_value"].to_numpy(), idem.data.reshape(-1)[po.table(idem.data + 1, lab, K)[6]])

    mask = filled == 7
    check(Vector.from_mask(mask, dem), mask)
    check(Vector.from_mask(_dev(mask), dem), mask)
    labels, K, table = polygonize.label(_dev(mask), 4)
    assert labels.is_cuda and K == po.label(mask, 4)[1] and table["count"].sum() == mask.sum() and set(table["class"]) == {1}
    labels, K, _ = polygonize.label(mask, 4, device=True)
    assert labels.is_cuda and np.array_equal(labels.cpu().numpy(), po.label(mask, 4)[0])
