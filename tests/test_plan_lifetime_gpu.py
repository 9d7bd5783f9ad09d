"""The lifetime of the ten objects that hold a library handle, on the host and the device route, and the one-call wrappers whose
two routes share one library call.  One private context (not the process default), 8 x 12 rasters, 16-point clouds.

``PairSet`` takes host blocks only (one case, no device route), ``BWPlan`` keeps no tensor, and the clouds of ICP / CPD are made from
a dh plan of either route: their "device route" is that plan's, and the tensors compared are the ones that plan keeps.  ``apply_matrix`` has a host route only; it is compared with the library's device route called
directly with arguments made by the same helpers."""
import numpy as np
import pytest
import torch

from xdem_amd import _args, _lib, stats
from xdem_amd.biascorr import DhPlan, poly2d_apply
from xdem_amd.blockwise import BWPlan, tiling_grid, warp_affine_field
from xdem_amd.coreg import NKPlan
from xdem_amd.cpd import CpdCloud
from xdem_amd.demcollection import StackPlan
from xdem_amd.epc import PtsPlan
from xdem_amd.icp import IcpCloud
from xdem_amd.rigid import apply_matrix, matrix_from_translations_rotations
from xdem_amd.spatialstats import BinStatsPlan, PairSet, convolution
from xdem_amd.volume import HypsoPlan

pytestmark = pytest.mark.gpu

H, W, N_PTS = 8, 12, 16
T6 = (1.0, 0.0, 0.0, 0.0, -1.0, float(H))


def rasters():
    rng = np.random.default_rng(7)
    yy, xx = np.mgrid[0:H, 0:W]
    ref = (100 + 3 * np.sin(xx / 3.0) + 2 * np.cos(yy / 2.0) + 0.05 * rng.normal(size=(H, W))).astype(np.float32)
    tba = (ref + 0.3 + 0.02 * xx + 0.05 * rng.normal(size=(H, W))).astype(np.float32)
    return ref, tba


def cloud():
    rng = np.random.default_rng(8)
    return rng.uniform(1.5, W - 1.5, N_PTS), rng.uniform(1.5, H - 1.5, N_PTS), rng.normal(100, 2, N_PTS).astype(np.float32)


def place(a, device: bool):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda() if device else a


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


# ---- one builder per class: (plan, [(tensor the plan keeps, tensor that was passed in)]) ----------------------------------------------------
def build_nk(ctx, device):
    ref, tba = (place(a, device) for a in rasters())
    plan = NKPlan(ref, tba, None, ctx)
    return plan, ([(plan._keep[0], ref), (plan._keep[1], tba)] if device else [])


def build_dh(ctx, device):
    ref, tba = (place(a, device) for a in rasters())
    plan = DhPlan(ref, tba, None, ctx)
    return plan, ([(plan._keep[0], ref), (plan._keep[1], tba)] if device else [])


def build_pts(ctx, device):
    raster = place(rasters()[0], device)
    x, y, z = (place(c, device) for c in cloud())
    plan = PtsPlan(raster, x, y, z, T6, False, None, ctx=ctx)
    return plan, ([(plan._keep[0], raster), (plan._keep[1][0], x), (plan._keep[1][1], y), (plan._keep[1][2], z)] if device else [])


def build_bw(ctx, device):
    ref, tba = (place(a, device) for a in rasters())
    plan = BWPlan(ref, tba, None, tiling_grid((H, W), 4), ctx)
    plan._inputs = (ref, tba)   # (the plan keeps no tensor itself: they live as long as it does here)
    return plan, []


def build_hypso(ctx, device):
    ref, tba = (place(a, device) for a in rasters())
    plan = HypsoPlan(tba, ref, ctx=ctx)
    return plan, ([(plan.ddem, tba), (plan.ref, ref)] if device else [])


def build_stack(ctx, device):
    ref, tba = (place(a, device) for a in rasters())
    plan = StackPlan([ref, tba], 0, ctx)
    return plan, ([(plan.inputs[0], ref), (plan.inputs[1], tba)] if device else [])


def build_binstats(ctx, device):
    ref, tba = (place(a.ravel(), device) for a in rasters())
    plan = BinStatsPlan(tba, [ref], ctx)
    return plan, ([(plan._dev_values.tensor, tba), (plan.vars[0].tensor, ref)] if device else [])


def build_pairs(ctx, device):
    assert not device   # (pair blocks are host arrays)
    x, y, z = cloud()
    return PairSet([(x, y, z)], np.array([2.0, 5.0, 20.0]), ctx), []


class _WithParent:
    """A cloud made from a dh plan, which has to outlive it: both closed together, the cloud first."""

    def __init__(self, make, ctx, device):
        self.parent, self.kept = build_dh(ctx, device)
        self.plan = make(self.parent)

    def __getattr__(self, name):
        return getattr(self.plan, name)

    def close(self):
        self.plan.close()
        self.parent.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


def build_icp(ctx, device):
    both = _WithParent(lambda dh: IcpCloud.from_plan(dh, T6, False), ctx, device)
    return both, both.kept


def build_cpd(ctx, device):
    both = _WithParent(lambda dh: CpdCloud.from_plan(dh, T6), ctx, device)
    return both, both.kept


BUILDERS = {"NKPlan": build_nk, "DhPlan": build_dh, "PtsPlan": build_pts, "IcpCloud": build_icp, "CpdCloud": build_cpd, "BWPlan": build_bw,
            "HypsoPlan": build_hypso, "StackPlan": build_stack, "BinStatsPlan": build_binstats, "PairSet": build_pairs}


ROUTES = [(name, device) for name in BUILDERS for device in (False, True) if not (device and name == "PairSet")]
DEVICE_KEEPERS = {"NKPlan", "DhPlan", "PtsPlan", "IcpCloud", "CpdCloud", "HypsoPlan", "StackPlan", "BinStatsPlan"}


@pytest.mark.parametrize("name, device", ROUTES, ids=[f"{name}-{'device' if device else 'host'}" for name, device in ROUTES])
def test_with_block_closes_and_device_inputs_are_the_callers(ctx, name, device):
    plan, kept = BUILDERS[name](ctx, device)
    assert bool(kept) == (device and name in DEVICE_KEEPERS)   # (no comparison is skipped silently)
    with plan:
        assert plan.handle
        for mine, given in kept:
            assert mine.data_ptr() == given.data_ptr()
    assert plan.handle is None
    plan.close()   # (nothing left to do)
    assert plan.handle is None
    assert ctx.handle   # (the context is untouched)


class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"library call {name} after the context was closed")


def test_closing_the_context_closes_its_plans():
    own = _lib.Context(0)
    plans = {name: build(own, False)[0] for name, build in BUILDERS.items()}
    assert all(p.handle for p in plans.values())
    own.close()
    assert own.handle is None
    own._L = _NoLibrary()
    for name, plan in plans.items():
        assert plan.handle is None, name
        plan.close()
        if isinstance(plan, _WithParent):
            assert plan.parent.handle is None


# ---- one call site, two routes: the same arguments give the same bits --------------------------------------------------------------------
def same_bits(host, dev) -> bool:
    return np.array_equal(host, dev.cpu().numpy(), equal_nan=True) and host.dtype == dev.cpu().numpy().dtype


@pytest.mark.parametrize("dtype", (np.float32, np.float64))
def test_one_call_wrappers_agree_between_routes(ctx, dtype):
    dem = rasters()[1].astype(dtype)
    dem[2, 3] = np.nan
    dev = torch.from_numpy(dem).cuda()
    params = np.array([0.5, 0.01, -0.02, 0.001])
    assert same_bits(poly2d_apply(dem, params, ctx=ctx), poly2d_apply(dev, params, ctx=ctx))
    coeffs = ((0.01, 0.002, 0.3), (-0.003, 0.02, -0.2), (0.001, 0.0, 0.5))
    assert same_bits(warp_affine_field(dem, T6, *coeffs, ctx=ctx), warp_affine_field(dev, T6, *coeffs, ctx=ctx))
    filt = np.ones((1, 3, 3)) / 9.0
    assert same_bits(convolution(dem[None], filt, ctx=ctx), convolution(dev[None], filt, ctx=ctx))
    on_host, on_device = stats.get_stats(dem, ctx=ctx), stats.get_stats(dev, ctx=ctx)
    assert list(on_host) == list(on_device)
    for key in on_host:
        assert np.array_equal(np.float64(on_host[key]), np.float64(on_device[key]), equal_nan=True), key
    mask = rasters()[0] > 100
    assert stats.get_stats(dem, inlier_mask=mask, ctx=ctx) == pytest.approx(stats.get_stats(dev, inlier_mask=torch.from_numpy(mask).cuda(), ctx=ctx),
                                                                             rel=0, abs=0, nan_ok=True)


@pytest.mark.parametrize("dtype", (np.float32, np.float64))
def test_apply_matrix_feeds_the_library_what_its_device_route_gets(ctx, dtype):
    dem = rasters()[1].astype(dtype)
    matrix = matrix_from_translations_rotations(0.7, -0.4, 0.2, 1.0, -0.5, 0.8)
    centroid = (6.0, 4.0, 100.0)
    host, _ = apply_matrix(dem, matrix, centroid=centroid, transform=T6, ctx=ctx)
    dev, out = torch.from_numpy(dem).cuda(), torch.empty((H, W), dtype=getattr(torch, np.dtype(dtype).name), device="cuda")
    torch.cuda.synchronize()
    ctx.check(ctx._L.xdemhip_apply_matrix_rst(ctx.handle, _args.ptr(dev), _args.code(dev), H, W, _args.c_doubles(T6),
                                              _args.c_doubles(matrix.ravel()), _args.c_doubles(centroid), _args.ptr(out), _args.space(dev)))
    ctx.synchronize()
    assert host.dtype == dtype and same_bits(host, out)
