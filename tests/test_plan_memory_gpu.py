"""Device memory that plans keep between calls: every stateful object of the C ABI gives back what it took.

xdemhip_plan_bytes (include/xdemhip_test.h) counts the bytes that the plans of a context have asked for and not yet freed.  Every kind
of plan is created once from NumPy arrays and once from torch device tensors, through the C ABI, on the smallest input its create
accepts; the count is 0 before, positive after, 0 again after destroy, the two routes return the same bytes from their first step, and
where a kind keeps the caller's device arrays the host route holds exactly the uploaded bytes more.

Creates that fail after allocation has begun: the ICP object of a non-finite reference cloud ("the reference cloud must be finite",
found after the clouds are on the device) and the ICP / CPD objects of a one-pixel dh plan with standardisation (the factor, the mean
NMAD of the cloud, is 0).  The raster plans (Nuth-Kaab, dh, raster-point, blockwise), the pair set, the stack, the binning and the
hypsometric plans check their arguments before they allocate and have no argument that is rejected later: an entirely NaN raster makes
a valid plan with no valid pixel (its first STEP reports that), which is created and destroyed here all the same.
"""
import ctypes

import numpy as np
import pytest
import torch

from xdem_amd import _lib
from xdem_amd._lib import DEVICE, F32, HOST

pytestmark = pytest.mark.gpu

c_i64, c_dbl, c_vp = ctypes.c_int64, ctypes.c_double, ctypes.c_void_p
EINVAL = -1   # XDEMHIP_EINVAL
H, W = 6, 7
N = H * W
T6 = np.array([1.0, 0.0, 0.0, 0.0, -1.0, float(H)])   # north-up, 1 m pixels


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context()
    yield c
    c.close()


def held(ctx) -> int:
    b = c_i64(-1)
    ctx.check(ctx._L.xdemhip_plan_bytes(ctx.handle, ctypes.byref(b)))
    return b.value


def dp(a):
    return a.ctypes.data_as(ctypes.POINTER(c_dbl))


def ip(a):
    return a.ctypes.data_as(ctypes.POINTER(c_i64))


class Arrays:
    """The same arrays for one route: NumPy on the host route, torch tensors on the device route (kept alive by the object)."""

    def __init__(self, memspace, **arrays):
        self.memspace = memspace
        self.host = {k: np.ascontiguousarray(v) for k, v in arrays.items()}
        self.dev = {k: torch.from_numpy(v).cuda() for k, v in self.host.items()} if memspace == DEVICE else {}
        torch.cuda.synchronize()
        self.nbytes = sum(v.nbytes for v in self.host.values())

    def __call__(self, name):
        return c_vp(self.dev[name].data_ptr()) if self.memspace == DEVICE else c_vp(self.host[name].ctypes.data)


def rasters():
    rng = np.random.default_rng(7)
    yy, xx = np.mgrid[0:H, 0:W]
    ref = (100 + 3 * np.sin(xx / 2.0) + 2 * np.cos(yy / 1.5) + rng.normal(scale=0.05, size=(H, W))).astype(np.float32)
    tba = (ref + 0.3 + rng.normal(scale=0.05, size=(H, W))).astype(np.float32)
    ref[1, 2] = np.nan
    tba[4, 5] = np.nan
    inlier = np.ones((H, W), np.uint8)
    inlier[0, 0] = 0
    return ref, tba, inlier


def cloud(n=40, seed=3):
    rng = np.random.default_rng(seed)
    x = rng.uniform(0.6, W - 1.6, n)
    y = rng.uniform(1.6, H - 0.6, n)
    z = (100 + 3 * np.sin(x / 2.0) + rng.normal(scale=0.05, size=n)).astype(np.float32)
    return x, y, z


def nk_step_bytes(ctx, step, plan, nb, *lead):
    vs, nv, ym, ys = c_dbl(), c_i64(), c_dbl(), c_dbl()
    edges, counts, med = np.zeros(nb + 1), np.zeros(nb, np.int64), np.zeros(nb)
    ctx.check(step(plan, *lead, nb, ctypes.byref(vs), ctypes.byref(nv), ctypes.byref(ym), ctypes.byref(ys), dp(edges), ip(counts), dp(med)))
    return np.array([vs.value, ym.value, ys.value]).tobytes() + bytes(c_i64(nv.value)) + edges.tobytes() + counts.tobytes() + med.tobytes()


# ---- one class per kind: create(ctx, memspace) -> object with .step() -> bytes, .destroy(), .uploaded (bytes the host route uploads and keeps)
class Kind:
    keeps_device_arrays = False
    uploaded = 0

    def destroy(self):
        self.free(self.plan)


class NuthKaab(Kind):
    keeps_device_arrays = True

    def __init__(self, ctx, memspace, ref=None, tba=None, inlier=None):
        r, t, i = rasters()
        self.ctx, L = ctx, ctx._L
        self.a = Arrays(memspace, ref=r if ref is None else ref, tba=t if tba is None else tba, inlier=i if inlier is None else inlier)
        h, w = self.a.host["ref"].shape
        self.plan, nv = c_vp(), c_i64()
        self.rc = L.xdemhip_nk_create(ctx.handle, self.a("ref"), self.a("tba"), self.a("inlier"), F32, h, w, memspace, ctypes.byref(self.plan), ctypes.byref(nv))
        self.free, self.uploaded = L.xdemhip_nk_destroy, self.a.nbytes

    def step(self, nb=8):
        return nk_step_bytes(self.ctx, self.ctx._L.xdemhip_nk_step, self.plan, nb, 0.1, -0.2, 1.0, 1.0)

    def regrow(self):
        self.step(8)
        self.step(16)

    def direct(self):
        self.step(16)


class Dh(Kind):
    keeps_device_arrays = True

    def __init__(self, ctx, memspace, inlier=None):
        r, t, i = rasters()
        self.ctx, L = ctx, ctx._L
        self.a = Arrays(memspace, ref=r, tba=t, inlier=i if inlier is None else inlier)
        self.plan, nv = c_vp(), c_i64()
        ctx.check(L.xdemhip_dh_create(ctx.handle, self.a("ref"), self.a("tba"), self.a("inlier"), F32, H, W, memspace, ctypes.byref(self.plan), ctypes.byref(nv)))
        self.n_valid, self.free, self.uploaded = nv.value, L.xdemhip_dh_destroy, self.a.nbytes

    def step(self):
        med, cnt = c_dbl(), c_i64()
        self.ctx.check(self.ctx._L.xdemhip_dh_median(self.plan, ctypes.byref(med), ctypes.byref(cnt)))
        return bytes(med) + bytes(cnt)

    def draw(self, k):
        ranks, nd = np.arange(k, dtype=np.int64) * 2, c_i64()
        med, nmad, cnt = c_dbl(), c_dbl(), c_i64()
        self.ctx.check(self.ctx._L.xdemhip_dh_subsample(self.plan, c_vp(ranks.ctypes.data), k, HOST, ctypes.byref(nd)))
        assert nd.value == k
        self.ctx.check(self.ctx._L.xdemhip_dh_shift_nmad(self.plan, 0.1, 0.1, 1.0, 1.0, 1.4826, ctypes.byref(med), ctypes.byref(nmad), ctypes.byref(cnt)))

    def regrow(self):
        self.draw(5)
        self.draw(11)

    def direct(self):
        self.draw(11)


class RasterPoint(Kind):
    keeps_device_arrays = True

    def __init__(self, ctx, memspace):
        r, _, i = rasters()
        x, y, z = cloud()
        self.ctx, L = ctx, ctx._L
        self.a = Arrays(memspace, raster=r, x=x, y=y, z=z)
        self.inl = Arrays(memspace, inlier=i)   # (read by create only, not kept)
        self.plan, nv = c_vp(), c_i64()
        ctx.check(L.xdemhip_pts_create(ctx.handle, self.a("raster"), self.inl("inlier"), F32, H, W, dp(T6), self.a("x"), self.a("y"), self.a("z"), x.size, 0, 1,
                                       memspace, ctypes.byref(self.plan), ctypes.byref(nv)))
        self.n_valid, self.free, self.uploaded = nv.value, L.xdemhip_pts_destroy, self.a.nbytes

    def step(self, nb=6):
        return nk_step_bytes(self.ctx, self.ctx._L.xdemhip_pts_nk_step, self.plan, nb, 0.1, -0.1)

    def draw(self, k):
        ranks, ns = np.arange(k, dtype=np.int64), c_i64()
        self.ctx.check(self.ctx._L.xdemhip_pts_subsample(self.plan, c_vp(ranks.ctypes.data), k, HOST, ctypes.byref(ns)))
        assert ns.value == k
        self.step()

    def regrow(self):
        self.draw(9)
        self.draw(17)

    def direct(self):
        self.draw(17)


class PairSet(Kind):
    def __init__(self, ctx, memspace):
        x, y, z = cloud(30)
        self.ctx, L, self.nb = ctx, ctx._L, 4
        self.off = np.array([0, 30], np.int64)
        self.edges = np.array([1.0, 2.0, 4.0, 8.0])
        self.a = Arrays(memspace, x=x, y=y, v=z)
        self.plan, npairs = c_vp(), c_i64()
        ctx.check(L.xdemhip_pairs_create(ctx.handle, 1, c_vp(self.off.ctypes.data), self.a("x"), self.a("y"), self.a("v"), None, None, None, None, F32,
                                         c_vp(self.edges.ctypes.data), self.nb, memspace, ctypes.byref(self.plan), ctypes.byref(npairs)))
        assert npairs.value == 30 * 29 // 2
        self.free = L.xdemhip_pairs_destroy

    def step(self):
        sums, counts = np.zeros(self.nb), np.zeros(self.nb, np.int64)
        self.ctx.check(self.ctx._L.xdemhip_pairs_sums(self.plan, 0, dp(sums), ip(counts)))
        return sums.tobytes() + counts.tobytes()


class Blockwise(Kind):
    def __init__(self, ctx, memspace):
        r, t, i = rasters()
        self.ctx, L = ctx, ctx._L
        self.a = Arrays(memspace, ref=r, tba=t, inlier=i)
        self.tiles = np.array([0, 3, 0, 3, 3, 6, 3, 6], np.int64)   # two 3 x 3 tiles: (r0, r1, c0, c1) each
        self.plan, nv = c_vp(), np.zeros(2, np.int64)
        ctx.check(L.xdemhip_bw_create(ctx.handle, self.a("ref"), self.a("tba"), self.a("inlier"), F32, H, W, 2, ip(self.tiles), memspace, ctypes.byref(self.plan), ip(nv)))
        self.free = L.xdemhip_bw_destroy

    def step(self, nb=4):
        active, sx, sy = np.ones(2, np.uint8), np.array([0.1, -0.1]), np.array([0.05, 0.2])
        vs, nv, ym, ys = np.zeros(2), np.zeros(2, np.int64), np.zeros(2), np.zeros(2)
        edges, counts, med = np.zeros((2, nb + 1)), np.zeros((2, nb), np.int64), np.zeros((2, nb))
        self.ctx.check(self.ctx._L.xdemhip_bw_nk_step(self.plan, c_vp(active.ctypes.data), dp(sx), dp(sy), 1.0, 1.0, nb, dp(vs), ip(nv), dp(ym), dp(ys), dp(edges),
                                                      ip(counts), dp(med)))
        return b"".join(a.tobytes() for a in (vs, nv, ym, ys, edges, counts, med))


class Icp(Kind):
    """From a dh plan of the route (the clouds of its valid pixels); xdemhip_icp_create_points takes host arrays only."""

    create, free_name, flags = "xdemhip_icp_create_plan", "xdemhip_icp_destroy", (0, 1)   # without normals, standardised

    def __init__(self, ctx, memspace, inlier=None):
        self.ctx, L = ctx, ctx._L
        self.dh = Dh(ctx, memspace, inlier)
        self.free = getattr(L, self.free_name)
        self.make()   # (the first create also builds the dh plan's list of valid pixels, which stays with the dh plan)
        if self.rc == 0:
            self.free(self.plan)
        self.before = held(ctx)
        self.make()

    def make(self):
        self.plan, cen, fac, cnt = c_vp(), np.zeros(3), c_dbl(), c_i64()
        self.rc = getattr(self.ctx._L, self.create)(self.dh.plan, dp(T6), *self.flags, ctypes.byref(self.plan), dp(cen), ctypes.byref(fac), ctypes.byref(cnt))
        self.n = cnt.value

    def step(self):
        ind, dist = np.zeros(self.n, np.int64), np.zeros(self.n)
        self.ctx.check(self.ctx._L.xdemhip_icp_query(self.plan, None, ip(ind), dp(dist)))
        return ind.tobytes() + dist.tobytes()

    def destroy(self):
        if self.rc == 0:
            self.free(self.plan)
        self.dh.destroy()


class Cpd(Icp):
    create, free_name, flags = "xdemhip_cpd_create_plan", "xdemhip_cpd_destroy", (1,)   # standardised

    def step(self):
        sums, s2 = np.zeros(18), c_dbl()
        self.ctx.check(self.ctx._L.xdemhip_cpd_estep(self.plan, None, float("nan"), 0.1, dp(sums), ctypes.byref(s2)))
        return sums.tobytes() + bytes(s2)


class Stack(Kind):
    keeps_device_arrays = True
    T = 3

    def __init__(self, ctx, memspace):
        r, t, _ = rasters()
        self.ctx, L, self.memspace = ctx, ctx._L, memspace
        self.a = Arrays(memspace, p0=r.ravel(), p1=t.ravel(), p2=(t + 1).ravel())
        masks = [np.zeros(N, np.uint8), np.ones(N, np.uint8)]
        masks[0][: N // 2] = 1
        self.masks = Arrays(memspace, m0=masks[0], m1=masks[1])
        self.out = Arrays(memspace, out=np.zeros(self.T * N, np.float32))
        planes = (c_vp * self.T)(*(self.a(k) for k in ("p0", "p1", "p2")))
        self.plan = c_vp()
        ctx.check(L.xdemhip_stack_create(ctx.handle, planes, self.T, F32, N, 0, memspace, ctypes.byref(self.plan)))
        self.free, self.uploaded = L.xdemhip_stack_destroy, self.a.nbytes

    def step(self):
        nd, nn = np.zeros(self.T, np.int64), np.zeros(self.T, np.int64)
        self.ctx.check(self.ctx._L.xdemhip_stack_subtract(self.plan, None, self.out("out"), self.memspace, ip(nd), ip(nn)))
        torch.cuda.synchronize()
        out = self.out.dev["out"].cpu().numpy() if self.memspace == DEVICE else self.out.host["out"]
        return nd.tobytes() + nn.tobytes() + out.tobytes()

    def set_masks(self, k):
        ptrs = (c_vp * k)(*(self.masks(n) for n in ("m0", "m1")[:k]))
        ids = np.array([0, k - 1, -1], np.int32)
        self.ctx.check(self.ctx._L.xdemhip_stack_set_masks(self.plan, ptrs, k, ids.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), self.memspace))

    def regrow(self):
        self.set_masks(1)
        self.set_masks(2)

    def direct(self):
        self.set_masks(2)


class Binning(Kind):
    keeps_device_arrays = True

    def __init__(self, ctx, memspace):
        r, t, _ = rasters()
        self.ctx, L, self.memspace = ctx, ctx._L, memspace
        self.a = Arrays(memspace, values=(t - r).ravel())
        self.var = Arrays(memspace, var=r.ravel())
        self.plan = c_vp()
        ctx.check(L.xdemhip_binstats_create(ctx.handle, self.a("values"), F32, N, memspace, ctypes.byref(self.plan)))
        self.free, self.uploaded = L.xdemhip_binstats_destroy, self.a.nbytes

    def step(self):
        L = self.ctx._L
        assert L.xdemhip_binstats_add_var(self.plan, self.var("var"), F32, self.memspace) == 0
        nv, lo, hi = c_i64(), np.zeros(1), np.zeros(1)
        self.ctx.check(L.xdemhip_binstats_finalize(self.plan, ctypes.byref(nv), dp(lo), dp(hi)))
        return bytes(nv) + lo.tobytes() + hi.tobytes()


class Hypso(Kind):
    keeps_device_arrays = True

    def __init__(self, ctx, memspace):
        r, t, i = rasters()
        self.ctx, L = ctx, ctx._L
        self.a = Arrays(memspace, ddem=(t - r).ravel(), ref=r.ravel(), mask=i.ravel())
        self.plan = c_vp()
        ctx.check(L.xdemhip_hypso_create(ctx.handle, self.a("ddem"), F32, self.a("ref"), F32, None, self.a("mask"), N, memspace, ctypes.byref(self.plan)))
        self.free, self.uploaded = L.xdemhip_hypso_destroy, self.a.nbytes

    def step(self):
        cap = 4
        ids, counts, ext = np.zeros(cap, np.int32), np.zeros(2 * cap, np.int64), np.zeros(4 * cap)
        nf, nb, nr = c_i64(), c_i64(), c_i64()
        self.ctx.check(self.ctx._L.xdemhip_hypso_label_stats(self.plan, cap, ids.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), ip(counts), dp(ext),
                                                             ctypes.byref(nf), ctypes.byref(nb), ctypes.byref(nr)))
        order = np.argsort(ids[: nf.value])   # (the labels come in no particular order)
        return bytes(nf) + bytes(nb) + bytes(nr) + ids[: nf.value][order].tobytes() + counts.reshape(cap, 2)[: nf.value][order].tobytes() + \
            ext.reshape(cap, 4)[: nf.value][order].tobytes()


KINDS = [NuthKaab, Dh, RasterPoint, PairSet, Blockwise, Icp, Cpd, Stack, Binning, Hypso]


@pytest.mark.parametrize("kind", KINDS, ids=lambda k: k.__name__)
def test_plan_gives_back_what_it_took(ctx, kind):
    got, count = {}, {}
    for memspace in (HOST, DEVICE):
        assert held(ctx) == 0                                   # a.
        p = kind(ctx, memspace)
        assert getattr(p, "rc", 0) == 0
        count[memspace] = held(ctx)
        assert count[memspace] > getattr(p, "before", 0)        # b.
        got[memspace] = p.step()
        p.destroy()
        assert held(ctx) == 0                                   # c.
    assert got[HOST] == got[DEVICE]                             # f.
    if kind.keeps_device_arrays:                                # d.
        assert count[HOST] - count[DEVICE] == p.uploaded > 0


@pytest.mark.parametrize("kind", [NuthKaab, Dh, RasterPoint, Stack], ids=lambda k: k.__name__)
@pytest.mark.parametrize("memspace", [HOST, DEVICE], ids=["host", "device"])
def test_regrown_plan_holds_what_a_fresh_one_does(ctx, kind, memspace):
    assert held(ctx) == 0
    p = kind(ctx, memspace)
    p.regrow()
    regrown = held(ctx)
    p.destroy()
    assert held(ctx) == 0
    q = kind(ctx, memspace)
    q.direct()
    assert held(ctx) == regrown > 0                             # e.
    q.destroy()
    assert held(ctx) == 0


def test_failed_creates_leave_nothing(ctx):
    """Creates rejected after allocation has begun: ICP from a non-finite cloud, ICP / CPD from a one-pixel dh plan.  The Nuth-Kaab,
    dh, raster-point, blockwise, pair-set, stack, binning and hypsometric creates have no such late-rejecting argument (module
    docstring); the all-NaN raster of a Nuth-Kaab plan is run all the same."""
    L = ctx._L
    assert held(ctx) == 0
    # an entirely NaN raster: a valid Nuth-Kaab plan without a valid pixel (module docstring), or an error -- nothing is left either way
    nan = np.full((H, W), np.nan, np.float32)
    for memspace in (HOST, DEVICE):
        p = NuthKaab(ctx, memspace, ref=nan, tba=nan)
        if p.rc == 0:
            p.destroy()
        assert held(ctx) == 0
    # ICP from points: the bounding box of a non-finite reference cloud is found after the clouds are uploaded
    ref = np.ascontiguousarray(np.stack(cloud(20)).astype(np.float64))
    qry = ref.copy()
    ref[0, 3] = np.inf
    icp = c_vp()
    assert L.xdemhip_icp_create_points(ctx.handle, dp(ref), 20, dp(qry), 20, None, ctypes.byref(icp)) == EINVAL
    assert b"finite" in L.xdemhip_last_error(ctx.handle)
    assert held(ctx) == 0
    # ICP / CPD from a dh plan of one valid pixel: the standardisation factor is 0, found after the clouds are gathered
    one = np.zeros((H, W), np.uint8)
    one[2, 3] = 1
    for kind in (Icp, Cpd):
        for memspace in (HOST, DEVICE):
            p = kind(ctx, memspace, inlier=one)
            assert p.rc == EINVAL and p.n == 1
            assert b"standardisation" in L.xdemhip_last_error(ctx.handle)
            assert held(ctx) == p.before > 0    # (the dh plan's own buffers; the failed object left none)
            p.destroy()
            assert held(ctx) == 0


def large_rasters(n=2048):
    rng = np.random.default_rng(11)
    yy, xx = np.mgrid[0:n, 0:n].astype(np.float32)
    ref = (500 + 40 * np.sin(xx / 97) * np.cos(yy / 131) + 15 * np.sin((xx + yy) / 41) + rng.normal(scale=0.5, size=(n, n))).astype(np.float32)
    tba = (ref + 1.5 + rng.normal(scale=0.3, size=(n, n))).astype(np.float32)
    return ref, tba, np.ones((n, n), np.uint8)


def test_large_plan_takes_and_returns_its_optional_groups(ctx):
    """2048 x 2048 float32 = SEL_BRACKET_MIN_N pixels: the smallest Nuth-Kaab plan that takes the selection workspace and the EXT and
    one-pass groups.  Its first step takes the route it took before the plans had an owner: (one-pass, plain) = ROUTE."""
    ROUTE = (0, 1)
    n = 2048
    ref, tba, inlier = large_rasters(n)
    assert held(ctx) == 0
    p = NuthKaab(ctx, HOST, ref=ref, tba=tba, inlier=inlier)
    assert p.rc == 0
    # per pixel: 9 B of inputs, 20 B of planes (four float32, mask, bins, bin cache); 3.25 B of selection workspace, 4 B of masked reference
    # and 2.5 B of one-pass candidates are the optional groups: 38.75 B with all of them
    assert held(ctx) > 38 * n * n
    p.step(72)
    a, c = c_i64(), c_i64()
    ctx.check(ctx._L.xdemhip_nk_route_counts(p.plan, ctypes.byref(a), ctypes.byref(c)))
    assert (a.value, c.value) == ROUTE
    p.destroy()
    assert held(ctx) == 0
