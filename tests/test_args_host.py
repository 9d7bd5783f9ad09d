"""How an array becomes a library argument, and how long a plan holds its handle: the rules of every entry point that prepares a raster
for ``libxdemhip`` -- output dtype per input dtype, masked cells, zero copy, the array kept alive, the refusals with their messages --
pinned on 3 x 5 arrays.  No GPU and no library: nothing here reaches a library call.

The assertions on the entry points and on the plan base were written against the functions as each module spelled them out before
``xdem_amd._args`` existed and passed there; moving the functions changed the import lines below and nothing else.  The tests of the
``_args`` primitives themselves (``ptr``, ``code``, the typed pointers, ``is_tensor``, ``host_float``, ``device_float``) and
``test_every_stateful_object_is_a_plan`` had no counterpart to run against."""
import ctypes

import numpy as np
import pytest
import torch

from xdem_amd import _args, _lib
from xdem_amd._args import flat_float as _float_plane
from xdem_amd._args import flat_mask as _mask_plane
from xdem_amd._args import nan_filled as _host_array
from xdem_amd._args import plane_in_space, raster_pair
from xdem_amd._lib import _Plan
from xdem_amd.biascorr import DhPlan, poly2d_apply
from xdem_amd.bincorr import corr_apply
from xdem_amd.blockwise import warp_affine_field
from xdem_amd.epc import PtsPlan, _host_raster
from xdem_amd.spatialstats import _DeviceColumn, convolution
from xdem_amd.stats import _Input
from xdem_amd.terrain import _array_with_nan
from xdem_amd.volume import HypsoPlan

F32, F64 = np.dtype(np.float32), np.dtype(np.float64)
IN_DTYPES = (np.float32, np.float64, np.float16, np.int16, np.uint8, np.bool_)
T6 = (1.0, 0.0, 0.0, 0.0, -1.0, 3.0)


def grid(dtype=np.float32) -> np.ndarray:
    return (np.arange(15).reshape(3, 5) % 7).astype(dtype)


# what each entry point returns, reduced to the array the library would read
ENTRY = {
    "host_array": lambda a: _host_array(a),
    "host_raster": lambda a: _host_raster(a),
    "float_plane": lambda a: _float_plane(a, "ddem"),
    "plane_in_space": lambda a: plane_in_space(a, None)[3],
    "stats_input": lambda a: _Input(a, None, None).values,
    "array_with_nan": lambda a: _array_with_nan(a),
}
# float32 / float64 are kept everywhere; what the other dtypes become (None: left as they are)
PROMOTES_TO = {"host_array": None, "host_raster": F32, "float_plane": F32, "plane_in_space": F64, "stats_input": F64, "array_with_nan": None}
CONTIGUOUS = ("host_raster", "float_plane", "plane_in_space", "stats_input")   # the others hand the array on as it is


# ---- promotion ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ENTRY))
@pytest.mark.parametrize("dtype", IN_DTYPES)
def test_promotion_table(name, dtype):
    a = grid(dtype)
    out = ENTRY[name](a)
    want = a.dtype if a.dtype in (F32, F64) or PROMOTES_TO[name] is None else PROMOTES_TO[name]
    assert out.dtype == want
    assert np.array_equal(out.reshape(a.shape).astype(np.float64), a.astype(np.float64))


def test_array_with_nan_promotes_masked_integers_only():
    assert _array_with_nan(np.ma.masked_array(grid(np.int16), mask=grid() == 1)).dtype == F32
    assert _array_with_nan(np.ma.masked_array(grid(np.float16), mask=grid() == 1)).dtype == np.float16
    assert _array_with_nan(np.ma.masked_array(grid(np.float64), mask=grid() == 1)).dtype == F64


@pytest.mark.parametrize("dt_ref", (np.float32, np.float64, np.int32))
@pytest.mark.parametrize("dt_tba", (np.float32, np.float64, np.int32))
def test_raster_pair_promotion(dt_ref, dt_tba):
    ref, tba = grid(dt_ref), grid(dt_tba) + 1
    p = raster_pair(ref, tba, None)
    want = F64 if np.float64 in (dt_ref, dt_tba) else F32
    assert p.dtype == want and p.keep[0].dtype == want and p.keep[1].dtype == want
    assert p.code == (_lib.F64 if want == F64 else _lib.F32) and p.memspace == _lib.HOST and p.shape == (3, 5) and p.inlier is None
    assert np.array_equal(p.keep[0], ref.astype(want)) and np.array_equal(p.keep[1], tba.astype(want))


# ---- masked input -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["host_array", "host_raster", "float_plane", "plane_in_space", "array_with_nan"])
@pytest.mark.parametrize("dtype", (np.float32, np.float64))
def test_masked_cells_become_nan(name, dtype):
    data, mask = grid(dtype), grid() == 3
    before = data.copy()
    out = ENTRY[name](np.ma.masked_array(data, mask=mask)).reshape(3, 5)
    assert out.dtype == dtype
    assert np.all(np.isnan(out[mask])) and np.array_equal(out[~mask], before[~mask])
    assert np.array_equal(data, before)   # the caller's array is not written to


def test_stats_input_keeps_masked_values_and_carries_the_mask():
    data, mask = grid(np.float32), grid() == 3
    inp = _Input(np.ma.masked_array(data, mask=mask), None, None)
    assert np.array_equal(inp.values, data) and inp.values.ctypes.data == data.ctypes.data
    assert inp.total_mask.dtype == np.uint8 and np.array_equal(inp.total_mask, (~mask).astype(np.uint8))
    assert _Input(np.ma.masked_array(data, mask=False), None, None).total_mask is None
    assert (inp.size, inp.shape, inp.tensor) == (15, (3, 5), False)


# ---- zero copy and the array kept alive ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ENTRY))
@pytest.mark.parametrize("dtype", (np.float32, np.float64))
def test_contiguous_float_input_is_not_copied(name, dtype):
    a = grid(dtype)
    assert ENTRY[name](a).ctypes.data == a.ctypes.data


@pytest.mark.parametrize("name", list(ENTRY))
@pytest.mark.parametrize("view", ("fortran", "strided"))
def test_views_come_out_contiguous_where_the_library_reads_them(name, view):
    a = np.asfortranarray(grid()) if view == "fortran" else np.tile(grid(), (1, 2))[:, ::2]
    assert not a.flags.c_contiguous
    out = ENTRY[name](a)
    assert np.array_equal(out.reshape(a.shape), a)
    if name in CONTIGUOUS:
        assert out.flags.c_contiguous and out.ctypes.data != a.ctypes.data
    else:
        assert out is a


def test_plane_in_space_returns_what_it_points_into():
    for a in (grid(np.float64), np.asfortranarray(grid()), grid(np.int16)):
        ptr, code, shape, keep = plane_in_space(a, None)
        assert ptr == keep.ctypes.data and shape == (3, 5) and keep.flags.c_contiguous
        assert code == (_lib.F32 if keep.dtype == F32 else _lib.F64)
    t = torch.arange(15, dtype=torch.float32).reshape(3, 5)   # a host tensor is read where it is
    ptr, code, shape, keep = plane_in_space(t, None)
    assert ptr == t.data_ptr() == keep.ctypes.data and code == _lib.F32 and shape == (3, 5)


def test_raster_pair_returns_what_it_points_into():
    ref, tba, mask = grid(), grid() + 1, grid() > 2
    p = raster_pair(ref, tba, mask)
    assert (p.ref, p.tba) == (ref.ctypes.data, tba.ctypes.data) and p.keep[0] is ref and p.keep[1] is tba
    assert p.inlier == p.keep[2].ctypes.data and p.keep[2].dtype == np.uint8 and np.array_equal(p.keep[2], mask)
    u8 = mask.astype(np.uint8)
    assert raster_pair(ref, tba, u8).inlier == u8.ctypes.data   # a uint8 mask goes as it is
    p = raster_pair(np.asfortranarray(ref), tba[:, ::-1], None)
    assert p.ref == p.keep[0].ctypes.data and p.tba == p.keep[1].ctypes.data
    assert all(k.flags.c_contiguous for k in p.keep[:2]) and np.array_equal(p.keep[1], tba[:, ::-1])


# ---- masks: cast as they are next to a raster pair, non-zero = set for the statistics and the volumes ----------------------------------
def test_mask_rules():
    ref, two = grid(), np.where(grid() > 2, 2, 0)
    assert np.array_equal(raster_pair(ref, ref, two).keep[2], two.astype(np.uint8))
    inl = _Input(ref, two, None).inlier
    assert inl.dtype == np.uint8 and np.array_equal(inl, (two != 0).astype(np.uint8)) and inl.shape == (3, 5)
    m = _mask_plane(two, np.zeros(15, np.float32))
    assert m.dtype == np.uint8 and m.shape == (15,) and np.array_equal(m, (two != 0).astype(np.uint8).ravel())
    t = _mask_plane(torch.from_numpy(two), np.zeros(15, np.float32))   # a tensor mask next to host rasters comes to the host
    assert isinstance(t, np.ndarray) and np.array_equal(t, m)


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
DEVICE_PAIR = "device inputs must be contiguous 2D float32 / float64 CUDA tensors of the same shape and dtype"


def cpu_tensor():
    return torch.arange(15, dtype=torch.float32).reshape(3, 5)


def test_convolution_refuses_a_host_tensor():
    with pytest.raises(TypeError) as e:
        convolution(cpu_tensor()[None], np.ones((1, 3, 3)), ctx=object())
    assert str(e.value) == "convolution: a device tensor must be a float32 / float64 CUDA tensor of shape (n_N, N1, N2)"
    with pytest.raises(TypeError, match="^convolution: images must be float32 or float64, got int16 "):
        convolution(grid(np.int16)[None], np.ones((1, 3, 3)), ctx=object())
    with pytest.raises(ValueError, match=r"^imgs must have three dimensions \(n_N, N1, N2\), got shape \(3, 5\)$"):
        convolution(grid(), np.ones((1, 3, 3)), ctx=object())


@pytest.mark.parametrize("call, message", [
    (lambda t: raster_pair(t, t, None), DEVICE_PAIR),
    (lambda t: DhPlan(t, t), DEVICE_PAIR),
    (lambda t: _float_plane(t, "ddem"), "ddem: a tensor input must live on the GPU (pass host data as a NumPy array)"),
    (lambda t: HypsoPlan(t, t), "ddem: a tensor input must live on the GPU (pass host data as a NumPy array)"),
    (lambda t: _Input(t, None, None), "a tensor input must be a contiguous float32 or float64 CUDA tensor"),
    (lambda t: poly2d_apply(t, np.ones(4)), "device elev must be a contiguous 2D float32 / float64 CUDA tensor"),
    (lambda t: corr_apply(t, _lib.CORR_POLY, [], [2], table=np.ones(2)), "device elev must be a contiguous 2D float32 / float64 CUDA tensor"),
    (lambda t: warp_affine_field(t, T6, (0, 0, 0), (0, 0, 0), (0, 0, 0), ctx=object()),
     "a device input must be a contiguous 2D float32 / float64 CUDA tensor"),
    (lambda t: PtsPlan(t, np.zeros(2), np.zeros(2), np.zeros(2), T6, False), "a device raster must be a contiguous 2D float32 / float64 CUDA tensor"),
    (lambda t: _DeviceColumn(t.reshape(-1)), "device columns must be contiguous 1-D float32 / float64 CUDA tensors"),
])
def test_host_tensors_are_refused(call, message):
    with pytest.raises(ValueError) as e:
        call(cpu_tensor())
    assert str(e.value) == message


@pytest.mark.parametrize("call, message", [
    (lambda a: raster_pair(a, a[:, :4], None), "ref and tba must be 2D arrays of the same shape"),
    (lambda a: raster_pair(a[0], a[0], None), "ref and tba must be 2D arrays of the same shape"),
    (lambda a: DhPlan(a, a, np.ones((3, 4), bool)), "inlier_mask must have the shape of the rasters"),
    (lambda a: PtsPlan(a, np.zeros(2), np.zeros(2), np.zeros(2), T6, False, np.ones((3, 4), bool)), "inlier_mask must have the shape of the raster"),
    (lambda a: _Input(a, np.ones((3, 4), bool), None), "inlier_mask has shape (3, 4), the values (3, 5)"),
    (lambda a: _host_raster(a[0]), "the raster of a raster-point pair must be a 2D array"),
    (lambda a: HypsoPlan(a, a[:, :4]), "the dDEM and the reference DEM must have the same number of pixels"),
    (lambda a: HypsoPlan(a, a, mask=np.ones((3, 4), bool)), "the label map / mask must have the same number of pixels as the rasters"),
])
def test_shape_mismatches(call, message):
    with pytest.raises(ValueError) as e:
        call(grid())
    assert str(e.value) == message


# ---- the primitives -----------------------------------------------------------------------------------------------------------------
def test_primitives_ptr_code_space():
    assert _args.ptr(None) is None
    a, t = grid(np.float64), cpu_tensor()
    assert _args.ptr(a) == a.ctypes.data and _args.ptr(t) == t.data_ptr()
    for np_dt, torch_dt, want in ((np.float32, torch.float32, _lib.F32), (np.float64, torch.float64, _lib.F64)):
        forms = (np_dt, np.dtype(np_dt), grid(np_dt), torch.zeros(2, dtype=torch_dt), torch_dt)
        assert [_args.code(f) for f in forms] == [want] * len(forms)
        assert all(_args.np_dtype(f) == np.dtype(np_dt) for f in forms)
    assert _args.np_dtype(torch.zeros(1, dtype=torch.int32)) == np.int32
    assert _args.space(a) == _lib.HOST
    assert _args.same_space(a, a) is a and _args.same_space(t, t) is t
    assert isinstance(_args.same_space(t, a), np.ndarray)


def test_primitives_typed_pointers():
    a = np.array([1.5, 2.5])
    p = _args.dp(a)
    assert isinstance(p, _args.DP) and ctypes.cast(p, ctypes.c_void_p).value == a.ctypes.data and p[1] == 2.5
    assert _args.dp(None) is None and _args.i64p(None) is None
    i = np.array([7, 8], dtype=np.int64)
    assert isinstance(_args.i64p(i), _args.I64P) and _args.i64p(i)[1] == 8
    assert _args.i32p(i.astype(np.int32))[0] == 7 and _args.u64p(i.astype(np.uint64))[0] == 7
    t = torch.tensor([3.0, 4.0], dtype=torch.float64)
    assert _args.dp(t)[1] == 4.0   # a tensor's address under the same type
    c = _args.c_doubles((1, 2, 3))   # (the pointer keeps the temporary array alive)
    assert isinstance(c, _args.DP) and [c[k] for k in range(3)] == [1.0, 2.0, 3.0]


def test_is_tensor_forms_agree():
    from xdem_amd import DEM

    by_module = lambda x: type(x).__module__.startswith("torch") and hasattr(x, "data_ptr")   # noqa: E731
    inputs = [grid(), np.ma.masked_array(grid()), [1.0, 2.0], (1, 2), None, 3.0, cpu_tensor(), torch.nn.Parameter(cpu_tensor()),
              cpu_tensor().bool(), torch.float32, torch.Size((3, 5)), DEM.from_array(grid(), T6, None, None)]
    for x in inputs:
        assert _args.is_tensor(x) == hasattr(x, "is_cuda") == by_module(x), type(x)


def test_host_float():
    a = grid()
    assert _args.host_float(a) is a
    assert _args.host_float(grid(np.int16)).dtype == F32 and _args.host_float(grid(np.int16), np.float64).dtype == F64
    out = _args.host_float(np.ma.masked_array(grid(np.float64), mask=grid() == 3))
    assert out.dtype == F64 and np.isnan(out[grid() == 3]).all()
    assert _args.host_float(np.asfortranarray(a)).flags.c_contiguous


def test_device_float_refuses_with_the_callers_text():
    with pytest.raises(ValueError, match="^my own words$"):
        _args.device_float(cpu_tensor(), "my own words")


# ---- the plan base ------------------------------------------------------------------------------------------------------------------
class _StubLib:
    def __init__(self):
        self.destroyed = []

    def stub_destroy(self, handle):
        self.destroyed.append(handle)


class _StubContext:
    def __init__(self):
        self.handle, self._L, self.adopted = 1, _StubLib(), []

    def adopt(self, obj):
        self.adopted.append(obj)


class _StubPlan(_Plan):
    _DESTROY = "stub_destroy"

    def __init__(self, ctx):
        self.ctx, self.handle = ctx, 42
        ctx.adopt(self)


def test_plan_destroys_once():
    ctx = _StubContext()
    plan = _StubPlan(ctx)
    plan.close()
    assert ctx._L.destroyed == [42] and plan.handle is None
    plan.close()
    plan.__del__()
    assert ctx._L.destroyed == [42]
    with _StubPlan(ctx) as inside:
        assert inside.handle == 42
    assert ctx._L.destroyed == [42, 42] and inside.handle is None


def test_plan_of_a_closed_context_makes_no_call():
    ctx = _StubContext()
    plan = _StubPlan(ctx)
    ctx.handle = None
    plan.close()
    plan.__del__()
    assert ctx._L.destroyed == [] and plan.handle is None


@pytest.mark.parametrize("cls, module", [("HypsoPlan", "volume"), ("StackPlan", "demcollection"), ("BinStatsPlan", "spatialstats"),
                                         ("PairSet", "spatialstats"), ("NKPlan", "coreg"), ("DhPlan", "biascorr"), ("PtsPlan", "epc"),
                                         ("IcpCloud", "icp"), ("CpdCloud", "cpd"), ("BWPlan", "blockwise")])
def test_every_stateful_object_is_a_plan(cls, module):
    import importlib

    assert issubclass(getattr(importlib.import_module("xdem_amd." + module), cls), _Plan)
