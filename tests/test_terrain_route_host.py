"""The host side of the terrain path on the CPU: which kernel a call gets, how the streaming route cuts a raster into strips and frame
tiles, which window kernel runs on which grid, how a host-buffer call is cut into row chunks (xdem_amd/csrc/terrain_route.h) and the
threaded span copy (host_copy.h).  The headers are compiled with g++ into a small harness (tests/hostsim/terrain_route_hostsim.cpp);
every rule is restated here in plain Python and compared exactly.
"""
import ctypes
import itertools
import math
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostsim", "terrain_route_hostsim.cpp")
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "xdem_amd", "csrc")
HDRS = [os.path.join(CSRC, "terrain_route.h"), os.path.join(CSRC, "host_copy.h"), os.path.join(ROOT, "include", "xdemhip.h")]
SO = os.path.join(HERE, "hostsim", "_terrain_route_hostsim.so")
COPY_CHECK = os.path.join(HERE, "hostsim", "_host_copy_check")

# include/xdemhip.h
F32, F64 = 0, 1
HORN, ZT, FL = 0, 1, 2
GEOMETRIC, DIRECTIONAL = 0, 1
RILEY, WILSON = 0, 1
SLOPE, ASPECT, HILLSHADE, CURVATURE = 1, 2, 4, 8
TPI, TRI, ROUGH, RUGOSITY, FRACTAL = 1 << 10, 1 << 11, 1 << 12, 1 << 13, 1 << 14
CURV_BITS = 0x3F8
SURFACE = 0x3FF
FUSED_WIN = TPI | TRI | ROUGH
FULL11 = 0xFFF & ~CURVATURE
SAH = SLOPE | ASPECT | HILLSHADE
SAH_WIN = SAH | TPI | TRI
EINVAL = -1
TILE_W, TILE_H = 256, 32


def p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(q) for q in [SRC] + HDRS):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-pthread", "-shared", "-fPIC", "-o", SO, SRC])
    L = ctypes.CDLL(SO)
    L.tr_copy_threshold.restype = ctypes.c_int64
    L.tr_copy_case.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_uint32]
    L.tr_validate.argtypes = [ctypes.c_void_p, ctypes.c_double, ctypes.c_char_p, ctypes.c_int]
    L.tr_route_bulk.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]
    L.tr_families.argtypes = [ctypes.c_void_p]
    L.tr_plan_strips.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    L.tr_plan_window.argtypes = [ctypes.c_int64, ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    L.tr_halo_depth.argtypes = [ctypes.c_uint32, ctypes.c_int, ctypes.c_int]
    L.tr_host_chunks.restype = ctypes.c_int64
    L.tr_host_chunks.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64]
    fam = np.zeros(10, np.int32)
    L.tr_families(p(fam))
    assert len(set(fam.tolist())) == 10
    L.fam = dict(zip(["none", "full11_geo", "full11_dir", "sah_win", "slope", "slope_aspect", "hillshade", "sah", "runtime", "runtime_f64"],
                     fam.tolist()))
    return L


# ---- argument checks ------------------------------------------------------------------------------------------------------------
def validate(lib, resolution=10.0, **kw):
    a = dict(dem_ok=1, planes_ok=1, dem_dtype=F32, H=100, W=200, row_stride=200, halo_top=0, halo_bottom=0, fit=FL, curv=0, mask=FULL11,
             tri=0, window=3, out_dtype=F32, memspace=1)
    a.update(kw)
    msg = ctypes.create_string_buffer(128)
    code = lib.tr_validate(p(np.array(list(a.values()), np.int64)), resolution, msg, 128)
    return code, msg.value.decode()


def test_validate_messages_and_their_order(lib):
    assert validate(lib) == (0, "")
    # each bad argument alone, then every bad argument from that one on: the first check that fails speaks
    bad = [(dict(dem_ok=0), "null buffer"), (dict(W=0), "bad raster geometry"), (dict(dem_dtype=2), "dtype must be XDEMHIP_F32 or XDEMHIP_F64"),
           (dict(fit=3), "unknown surface_fit"), (dict(curv=2), "unknown curv_method"), (dict(tri=-1), "unknown tri_method"),
           (dict(mask=1 << 15), "bad attr_mask"), (dict(window=4), "window_size must be odd and >= 3"),
           (dict(resolution=0.0), "resolution must be > 0"), (dict(memspace=2), "bad memspace")]
    for i, (kw, msg) in enumerate(bad):
        assert validate(lib, **kw) == (EINVAL, msg)
        later = {}
        for kw2, _ in bad[i:]:
            later.update(kw2)
        assert validate(lib, **later) == (EINVAL, msg)
    for kw in (dict(planes_ok=0), dict(H=0), dict(row_stride=199), dict(halo_top=-1), dict(halo_bottom=-1), dict(out_dtype=-1), dict(mask=0),
               dict(window=1), dict(window=1025), dict(resolution=float("nan")), dict(mask=RUGOSITY, resolution=-1.0)):
        assert validate(lib, **kw)[0] == EINVAL, kw
    # the window size counts for the windowed indexes only, the resolution for the surface fits and rugosity only
    assert validate(lib, mask=SLOPE, window=4)[0] == 0 and validate(lib, mask=FRACTAL, window=4)[0] == EINVAL
    assert validate(lib, mask=RUGOSITY, window=4)[0] == 0
    assert validate(lib, mask=TPI | ROUGH | FRACTAL, resolution=0.0)[0] == 0


def test_horn_with_any_curvature_is_refused(lib):
    for bit in range(3, 10):
        assert validate(lib, fit=HORN, mask=SLOPE | (1 << bit)) == (EINVAL, "'Horn' surface fit cannot be used to calculate curvatures")
        assert validate(lib, fit=ZT, mask=SLOPE | (1 << bit))[0] == 0
    assert validate(lib, fit=HORN, mask=SAH_WIN | ROUGH | RUGOSITY | FRACTAL)[0] == 0


# ---- which kernel ---------------------------------------------------------------------------------------------------------------
COLS = ["dem_dtype", "out_dtype", "mask", "fit", "curv", "tri", "degrees", "hs_z", "unclipped", "window", "math", "stream"]
OUT = ["family", "fit", "curv", "fuse_win", "tail", "try_stream", "mask", "window_mask"]


def py_route(fam, ddt, odt, mask, fit, curvm, tri, deg, hsz, uncl, w, tmath, stream):
    """The decision as the dispatcher has always made it, one call at a time."""
    surf, win = mask & ~FUSED_WIN, mask & FUSED_WIN
    fuse = bool(win) and w == 3
    m = surf | (win if fuse else 0)
    wmask = 0 if fuse else win
    if m == 0:
        return (fam["none"], ZT, 0, int(fuse), 0, 0, 0, wmask)
    f = fit if surf else ZT
    curv = int(bool(surf & CURV_BITS) and f != HORN)
    ff = ddt == F32 and odt == F32
    defaults_dir = bool(deg) and tri == RILEY and hsz == 1 and not uncl
    defaults = defaults_dir and curvm == GEOMETRIC
    f64tail = ff and (tmath == 1 or bool(uncl))
    small = {SLOPE: "slope", SLOPE | ASPECT: "slope_aspect", HILLSHADE: "hillshade", SAH: "sah"}
    if ff:
        if tmath in (0, 2):
            name = None
            if defaults and m == FULL11 and f in (FL, ZT):
                name = "full11_geo"
            elif defaults and m == SAH_WIN and f == HORN:
                name = "sah_win"
            elif defaults_dir and curvm == DIRECTIONAL and m == FULL11 and f in (FL, ZT):
                name = "full11_dir"
            if name:
                return (fam[name], f, int(name != "sah_win"), 1, tmath, int(stream != 0), m, wmask)
        if win == 0 and tmath == 2 and deg and not uncl and hsz == 1 and m in small:
            return (fam[small[m]], f, 0, 0, 2, int(stream != 0), m, wmask)
        if f64tail and defaults and m == FULL11 and f == FL:
            return (fam["full11_geo"], f, 1, 1, 1, 0, m, wmask)
        return (fam["runtime_f64" if f64tail else "runtime"], f, curv, int(fuse), int(f64tail), 0, m, wmask)
    if defaults and m == FULL11 and f in (FL, ZT):
        return (fam["full11_geo"], f, 1, 1, 0, 0, m, wmask)
    if defaults and m == SAH_WIN and f == HORN:
        return (fam["sah_win"], f, 0, 1, 0, 0, m, wmask)
    return (fam["runtime"], f, curv, int(fuse), 0, 0, m, wmask)


def routes(lib, rows):
    a = np.ascontiguousarray(rows, np.int32)
    out = np.zeros((a.shape[0], 8), np.int32)
    lib.tr_route_bulk(p(a), a.shape[0], p(out))
    return out


def named_masks():
    base = {"full11": FULL11, "sah_win": SAH_WIN, "slope": SLOPE, "slope_aspect": SLOPE | ASPECT, "hillshade": HILLSHADE, "sah": SAH}
    masks = dict(base)
    for name, m in base.items():
        for bit in range(13):
            if m ^ (1 << bit):
                masks[f"{name}^{bit}"] = m ^ (1 << bit)
    masks.update({"window_only": TPI | TRI | ROUGH, "tri_only": TRI, "curvature": CURVATURE, "tpi": TPI})
    return masks


def test_route_equals_the_restated_decision_over_the_cross_product(lib):
    pairs = [(F32, F32), (F64, F64), (F32, F64), (F64, F32)]
    options = list(itertools.product(pairs, (HORN, ZT, FL), (GEOMETRIC, DIRECTIONAL), (RILEY, WILSON), (0, 1), (1, 2), (0, 1), (0, 1, 2), (3, 5)))
    rows = [(ddt, odt, m, fit, cm, tri, deg, hsz, uncl, w, tmath, 1)
            for m in named_masks().values() for (ddt, odt), fit, cm, tri, deg, hsz, uncl, tmath, w in options]
    rng = np.random.default_rng(11)
    rows += [(F32, F32, int(m), int(fit), GEOMETRIC, RILEY, 1, 1, 0, 3, 2, 1) for m, fit in zip(rng.integers(1, 1 << 13, 2000), rng.integers(0, 3, 2000))]
    rows += [r[:11] + (0,) for r in rows[::7]]   # option "terrain_stream" = 0
    got = routes(lib, rows)
    want = np.array([py_route(lib.fam, *r) for r in rows], np.int32)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, [(dict(zip(COLS, rows[i])), dict(zip(OUT, got[i].tolist())), dict(zip(OUT, want[i].tolist()))) for i in bad[:5]]
    # whatever the route: every requested plane is written by exactly one of the two launches
    a = np.array(rows, np.int64)
    assert np.all((got[:, 6] | got[:, 7]) == a[:, 2]) and np.all((got[:, 6] & got[:, 7]) == 0)
    assert np.all((got[:, 0] == lib.fam["none"]) == (got[:, 6] == 0))
    # kernels that exist for float32 -> float32 alone
    ff = (a[:, 0] == F32) & (a[:, 1] == F32)
    ff_only = np.isin(got[:, 0], [lib.fam[k] for k in ("full11_dir", "slope", "slope_aspect", "hillshade", "sah", "runtime_f64")])
    assert not np.any(ff_only & ~ff) and not np.any((got[:, 4] != 0) & ~ff) and not np.any((got[:, 5] != 0) & ~ff)
    # strips: compile-time sets at the lean or mixed tail only; the float64 tail of a compile-time set: the Florinsky full set only
    runtime = np.isin(got[:, 0], [lib.fam["runtime"], lib.fam["runtime_f64"], lib.fam["none"]])
    assert not np.any((got[:, 5] != 0) & (runtime | (got[:, 4] == 1)))
    assert np.all(got[~runtime & (got[:, 4] == 1), 0] == lib.fam["full11_geo"]) and np.all(got[~runtime & (got[:, 4] == 1), 1] == FL)
    assert len(set(got[:, 0].tolist())) == 10    # every family is reached


def test_route_named_cases(lib):
    fam = lib.fam
    # the recorded bug: ["slope", "tpi"] with window_size = 5 needs BOTH launches -- a fused one for the
    # slope and the window launch for the TPI.  Since that fix a windowed index of another window size keeps the call off the
    # small-set kernels: the slope comes from the runtime-mask kernel, as before this header existed.
    r = dict(zip(OUT, routes(lib, [(F32, F32, SLOPE | TPI, FL, GEOMETRIC, RILEY, 1, 1, 0, 5, 2, 1)])[0].tolist()))
    assert r["family"] == fam["runtime"] and r["mask"] == SLOPE and r["window_mask"] == TPI and not r["fuse_win"]
    r = dict(zip(OUT, routes(lib, [(F32, F32, SLOPE, FL, GEOMETRIC, RILEY, 1, 1, 0, 5, 2, 1)])[0].tolist()))
    assert r["family"] == fam["slope"] and r["tail"] == 2 and r["try_stream"] and r["window_mask"] == 0
    r = dict(zip(OUT, routes(lib, [(F32, F32, SLOPE | TPI, FL, GEOMETRIC, RILEY, 1, 1, 0, 3, 2, 1)])[0].tolist()))
    assert r["family"] == fam["runtime"] and r["mask"] == SLOPE | TPI and r["window_mask"] == 0 and r["fuse_win"]
    # an unclipped hillshade never gets a lean-tail (or any compile-time) kernel
    rows = [(ddt, odt, m, fit, cm, RILEY, 1, 1, 1, 3, tmath, 1) for (ddt, odt) in ((F32, F32), (F64, F64), (F32, F64), (F64, F32))
            for m in named_masks().values() for fit in (HORN, ZT, FL) for cm in (0, 1) for tmath in (0, 1, 2)]
    got = routes(lib, rows)
    assert np.all(np.isin(got[:, 0], [fam["runtime"], fam["runtime_f64"], fam["none"]])) and not np.any(got[:, 4] == 2) and not np.any(got[:, 5])
    ff = np.array([r[0] == F32 and r[1] == F32 for r in rows])
    assert np.all(got[ff & (got[:, 0] != fam["none"]), 0] == fam["runtime_f64"])
    # window-only calls march with the cheapest fit whatever was asked for
    got = routes(lib, [(F32, F32, TPI | TRI, fit, 0, 0, 1, 1, 0, 3, 2, 1) for fit in (HORN, ZT, FL)])
    assert np.all(got[:, 1] == ZT) and np.all(got[:, 0] == fam["runtime"]) and np.all(got[:, 2] == 0)


# ---- strips -----------------------------------------------------------------------------------------------------------------------
SP = ["ok", "tx0", "tx1", "ty0", "ty1", "xi0", "yi0", "yi1", "band_height", "groups_x", "nbands", "ngroups", "grid8", "perm_mul", "strips", "frame"]


def strips(lib, H, W, stride=None, halo_top=0, halo_bottom=0, aligned=1, halo=2, stream=1):
    out = np.zeros(16, np.int64)
    lib.tr_plan_strips(p(np.array([H, W, W if stride is None else stride, halo_top, halo_bottom], np.int64)), aligned, halo, stream, p(out))
    return dict(zip(SP, out.tolist()))


def py_strips(H, W, stride, halo_top, halo_bottom, aligned, halo, stream):
    """The arithmetic of the streaming launcher as it stood; None where the raster does not qualify."""
    if not aligned or stride & 3 or stride >= (1 << 24) - 64:
        return None
    tx0, tx1 = 1, (W - 4) // TILE_W
    ty0 = 0 if halo_top >= halo else 1
    ty1 = min(H + halo_bottom - halo, H) // TILE_H
    if tx1 - tx0 < 1 or ty1 - ty0 < 2 or (tx1 - tx0) * (ty1 - ty0) < 64:
        return None
    bh = stream if stream >= 64 else 128
    yi0, yi1 = ty0 * TILE_H, ty1 * TILE_H
    bands = (yi1 - yi0 + bh - 1) // bh
    if bands * (tx1 - tx0) > 0xFFFFF0:
        return None
    ngroups = bands * (tx1 - tx0)
    grid8 = (ngroups + 7) // 8
    n = grid8 * 8
    m = int(0.6180339887 * n) | 1
    while m > 1 and math.gcd(m, n) != 1:
        m += 2
    return dict(ok=1, tx0=tx0, tx1=tx1, ty0=ty0, ty1=ty1, xi0=tx0 * TILE_W, yi0=yi0, yi1=yi1, band_height=bh, groups_x=tx1 - tx0, nbands=bands,
                ngroups=ngroups, grid8=grid8, perm_mul=m, strips=int(stream != 3), frame=int(stream != 2))


def frame_tiles(tiles_x, tiles_y, s):
    """Tiles of the frame launch, by the tile kernel's own enumeration (terrain_tile_kernel, frame mode)."""
    n = tiles_x * tiles_y - (s["tx1"] - s["tx0"]) * (s["ty1"] - s["ty0"])
    top, midw = tiles_x * s["ty0"], s["tx0"] + (tiles_x - s["tx1"])
    mid = midw * (s["ty1"] - s["ty0"])
    out = []
    for f in range(n):
        ty, tx = divmod(f, tiles_x)
        if f >= top:
            g = f - top
            if g < mid:
                ty, j = s["ty0"] + g // midw, g % midw
                tx = j if j < s["tx0"] else s["tx1"] + (j - s["tx0"])
            else:
                ty, tx = s["ty1"] + (g - mid) // tiles_x, (g - mid) % tiles_x
        out.append((tx, ty))
    return out


def strip_cases():
    cases = []
    for H, W in ((1400, 2600), (2309, 1801), (1153, 4100)):       # the shapes of the GPU test of the streaming route
        for stream in (1, 128, 256, 512, 2, 3):
            cases.append(dict(H=H, W=W, stream=stream))
        cases.append(dict(H=H - 166, W=W, halo_top=2, halo_bottom=2))   # its row block with halo rows
    for W in (515, 516, 771, 772, 20 * 256 + 3, 20 * 256 + 4, 66 * 256 + 4):   # interiors of 0, 1, 1, 2, 18, 19 and 65 tile columns
        for H in (2 * 32 + 1, 2 * 32 + 2, 3 * 32 + 2, 4 * 32 + 2, 66 * 32 + 2):   # ... and 0, 1, 2, 3 and 65 tile rows (halo 2, no halo rows)
            cases.append(dict(H=H, W=W))
    for W, H in ((10 * 256 + 4, 8 * 32 + 2), (9 * 256 + 4, 9 * 32 + 2), (9 * 256 + 3, 9 * 32 + 2), (9 * 256 + 4, 9 * 32 + 1)):   # 63, 64, 56, 56 tiles
        cases.append(dict(H=H, W=W))
    for halo, ht, hb in itertools.product((1, 2), (0, 1, 2), (0, 1, 2)):
        for H in (1400, 44 * 32, 44 * 32 + 1):
            cases.append(dict(H=H, W=2600, halo=halo, halo_top=ht, halo_bottom=hb))
    for stride in (2601, 2602, 2604, (1 << 24) - 64, (1 << 24) - 68, 1 << 24):
        cases.append(dict(H=1400, W=2600, stride=stride))
    cases.append(dict(H=1400, W=2600, aligned=0))
    for bh in (128, 256, 512):
        cases.append(dict(H=70000, W=5000, stream=bh))
    cases.append(dict(H=32 * 0xFFFFF0 // 64 * 4 + 40000, W=65 * 256 + 4, stream=128))   # more strip groups than one launch holds
    return cases


def test_strip_plan_equals_the_restated_arithmetic_and_covers_every_tile_once(lib):
    seen = {"ok": 0, "refused": 0}
    for c in strip_cases():
        a = dict(H=c["H"], W=c["W"], stride=c.get("stride", c["W"]), halo_top=c.get("halo_top", 0), halo_bottom=c.get("halo_bottom", 0),
                 aligned=c.get("aligned", 1), halo=c.get("halo", 2), stream=c.get("stream", 1))
        s, want = strips(lib, **a), py_strips(**a)
        assert bool(s["ok"]) == (want is not None), c
        if want is None:
            seen["refused"] += 1
            continue
        seen["ok"] += 1
        assert s == want, c
        H, W, halo, bh = a["H"], a["W"], a["halo"], s["band_height"]
        assert s["ngroups"] == s["nbands"] * s["groups_x"] and s["grid8"] * 8 >= s["ngroups"] > (s["grid8"] - 1) * 8
        assert s["perm_mul"] & 1 and math.gcd(s["perm_mul"], s["grid8"] * 8) == 1 and s["perm_mul"] < s["grid8"] * 8 + 2
        # rows and columns a strip reads (with its halo rows and the 4 columns either side) lie inside the buffer
        assert s["yi0"] - halo >= -a["halo_top"] and s["yi1"] + halo <= H + a["halo_bottom"]
        assert s["xi0"] - 4 >= 0 and s["xi0"] + s["groups_x"] * TILE_W + 4 <= W
        # bands tile [yi0, yi1) and the interior is whole tiles: the plan's tile rectangle
        assert (s["nbands"] - 1) * bh < s["yi1"] - s["yi0"] <= s["nbands"] * bh
        assert (s["xi0"], s["yi0"], s["yi1"]) == (s["tx0"] * TILE_W, s["ty0"] * TILE_H, s["ty1"] * TILE_H) and s["groups_x"] == s["tx1"] - s["tx0"]
        tiles_x, tiles_y = -(-W // TILE_W), -(-H // TILE_H)
        if tiles_x * tiles_y <= 20000:
            interior = {(tx, ty) for tx in range(s["tx0"], s["tx1"]) for ty in range(s["ty0"], s["ty1"])}
            frame = frame_tiles(tiles_x, tiles_y, s)
            assert len(set(frame)) == len(frame) and not (set(frame) & interior)
            assert set(frame) | interior == {(tx, ty) for tx in range(tiles_x) for ty in range(tiles_y)}
    assert seen["ok"] >= 40 and seen["refused"] >= 25
    # the named edges
    assert strips(lib, 9 * 32 + 2, 9 * 256 + 4)["ngroups"] == 8 * 2 and not strips(lib, 9 * 32 + 2, 9 * 256 + 3)["ok"]
    assert not strips(lib, 8 * 32 + 2, 10 * 256 + 4)["ok"]                                    # 63 interior tiles
    assert strips(lib, 1400, 2600, stride=(1 << 24) - 68)["ok"] and not strips(lib, 1400, 2600, stride=(1 << 24) - 64)["ok"]
    assert not strips(lib, 1400, 2600, stride=2602)["ok"] and not strips(lib, 1400, 2600, aligned=0)["ok"]
    assert strips(lib, 1400, 2600, stream=2)["frame"] == 0 and strips(lib, 1400, 2600, stream=3)["strips"] == 0
    assert strips(lib, 1400, 2600, halo_top=1)["ty0"] == 1 and strips(lib, 1400, 2600, halo_top=2)["ty0"] == 0
    assert strips(lib, 1400, 2600, halo=1, halo_top=1)["ty0"] == 0
    assert strips(lib, 44 * 32, 2600)["ty1"] == 43 and strips(lib, 44 * 32, 2600, halo_bottom=2)["ty1"] == 44


# ---- window kernels ---------------------------------------------------------------------------------------------------------------
def test_window_plan_choice_and_grids(lib):
    out = np.zeros(5, np.int64)
    for w, es, opt, W in itertools.product((3, 5, 7, 33, 1023), (4, 8), (0, 1), (1, 64, 65, 5000)):
        for H in (1, 100, 65535 * 4 - 1, 65535 * 4, 65535 * 4 + 1, 65535 * 16 - 1, 65535 * 16, 65535 * 16 + 1):
            lib.tr_plan_window(H, W, w, es, opt, p(out))
            lds_bytes = (16 + w - 1) * (64 + w - 1) * es
            gy_lds, gy_gen = -(-H // 16), -(-H // 4)
            lds = bool(opt) and lds_bytes <= 64 * 1024 and gy_lds <= 65535
            want = [int(lds), int(not lds and gy_gen > 65535), lds_bytes, -(-W // 64), gy_lds if lds else gy_gen % (1 << 32)]
            assert out.tolist() == want, (w, es, opt, W, H)
    lib.tr_plan_window(1000, 1000, 33, 4, 1, p(out))
    assert out[0] == 1 and out[2] == 48 * 96 * 4
    lib.tr_plan_window(1000, 1000, 1023, 4, 1, p(out))
    assert out[0] == 0 and out[1] == 0 and out[4] == 250
    lib.tr_plan_window(65535 * 16 + 1, 1000, 5, 4, 1, p(out))      # too tall for the LDS form's grid and for the per-pixel form's
    assert out[0] == 0 and out[1] == 1


# ---- host-buffer chunks -------------------------------------------------------------------------------------------------------------
def host_chunks(lib, H, W, halo_top, halo_bottom, depth, n_planes, in_es, out_es, mb, rows, halvings=0):
    head, chunks = np.zeros(5, np.int64), np.zeros((4096, 4), np.int64)
    n = lib.tr_host_chunks(p(np.array([H, W, halo_top, halo_bottom, depth, n_planes, in_es, out_es, mb, rows], np.int64)), halvings, p(head),
                           p(chunks), 4096)
    assert n > 0
    return dict(zip(["rows", "in_bytes", "plane_bytes", "out_bytes", "halved"], head.tolist())), chunks[:n]


def test_host_chunks_tile_the_raster_within_the_budget(lib):
    n_cases = 0
    for (H, W), (ht, hb), depth, n_planes, (in_es, out_es), mb in itertools.product(
            ((1, 1), (63, 10), (64, 4097), (1000, 300), (5000, 20000), (40000, 40000)), ((0, 0), (1, 0), (0, 2), (5, 5)), (0, 1, 2, 6),
            (1, 11, 15), ((4, 4), (8, 8), (4, 8)), (0, 1, 8)):
        free, _ = host_chunks(lib, H, W, ht, hb, depth, n_planes, in_es, out_es, mb, 0)
        for rows_opt in (0, 1, 100, H, 10 * H):
            head, ch = host_chunks(lib, H, W, ht, hb, depth, n_planes, in_es, out_es, mb, rows_opt)
            n_cases += 1
            case = (H, W, ht, hb, depth, n_planes, in_es, out_es, mb, rows_opt)
            # the restated rule
            budget = (mb if mb > 0 else 288) << 20
            rows = budget // (W * (in_es + out_es * n_planes)) - 2 * depth
            if 0 < rows_opt < rows:
                rows = rows_opt
            rows = min(max(rows, 64), H)
            assert head["rows"] == rows, case
            assert head["rows"] <= free["rows"], case                                # option "host_chunk_rows" never enlarges a chunk
            assert head["in_bytes"] == (rows + 2 * depth) * W * in_es and head["plane_bytes"] == rows * W * out_es, case
            assert head["out_bytes"] == head["plane_bytes"] * n_planes, case
            if rows > 64:
                assert 2 * (head["in_bytes"] + head["out_bytes"]) <= 2 * budget, case    # two pipeline slots of one chunk's budget each
            # chunks tile [0, H) in order, without gap, each of `rows` rows but the last
            assert ch[0, 0] == 0 and ch[-1, 1] == H and np.array_equal(ch[1:, 0], ch[:-1, 1]), case
            assert np.all(ch[:-1, 1] - ch[:-1, 0] == rows) and 0 < ch[-1, 1] - ch[-1, 0] <= rows, case
            # overlap: as deep as the attributes need, or as many rows as the caller's buffer has
            assert np.array_equal(ch[:, 2], np.minimum(depth, ch[:, 0] + ht)) and np.array_equal(ch[:, 3], np.minimum(depth, H + hb - ch[:, 1])), case
            # rows read from the caller's buffer, which holds rows [-halo_top, H + halo_bottom), and rows staged per chunk
            assert np.all(ch[:, 0] - ch[:, 2] >= -ht) and np.all(ch[:, 1] + ch[:, 3] <= H + hb), case
            assert np.all((ch[:, 1] - ch[:, 0] + ch[:, 2] + ch[:, 3]) * W * in_es <= head["in_bytes"]), case
    assert n_cases > 10000


def test_halving_reaches_the_floor_and_stops(lib):
    for H in (1, 63, 64, 65, 127, 128, 129, 1000, 5000, 100000):
        head, _ = host_chunks(lib, H, 3000, 0, 0, 2, 11, 4, 4, 0, 0)
        rows, expect = head["rows"], []
        while rows > 64:
            rows = max(rows // 2, 64)
            expect.append(rows)
        for k in range(len(expect) + 3):
            got, ch = host_chunks(lib, H, 3000, 0, 0, 2, 11, 4, 4, 0, 0, halvings=k)
            assert got["halved"] == min(k, len(expect)) and got["rows"] == ([head["rows"]] + expect)[min(k, len(expect))], (H, k)
            assert ch[-1, 1] == H and np.all(ch[:-1, 1] - ch[:-1, 0] == got["rows"])
        assert (min(H, 64) if expect else head["rows"]) == ([head["rows"]] + expect)[-1]


def test_halo_depth_of_the_library_and_of_dist(lib):
    """One rule, two places: the chunk overlap of host-buffer calls (terrain_halo_depth) and xdem_amd.dist.halo_depth, which sizes
    the halo rows of a rank's row block.  They agree on every surface-fit attribute and on TPI / TRI / roughness.  They differ on
    rugosity: the library knows it is always 3 x 3 (depth 1), dist follows the reference's list of windowed indexes and takes
    window_size // 2 -- deeper than needed where rugosity is the only reason for it, never shallower.  Both sides are left as they
    are; this test pins the two rules and the difference."""
    from xdem_amd import dist
    from xdem_amd.terrain import ATTR_BIT, list_requiring_surface_fit, list_requiring_windowed_index

    names = list_requiring_surface_fit + list_requiring_windowed_index
    rng = np.random.default_rng(3)
    sets = [[n] for n in names] + [names, list_requiring_surface_fit, list_requiring_windowed_index]
    sets += [[n for n in names if rng.random() < 0.3] or ["slope"] for _ in range(300)]
    differ = 0
    for attrs, (fit_name, fit), w in itertools.product(sets, (("Horn", HORN), ("ZevenbergThorne", ZT), ("Florinsky", FL)), (3, 5, 7, 9, 33)):
        mask = sum(1 << ATTR_BIT[a] for a in set(attrs))
        got, py = lib.tr_halo_depth(mask, fit, w), dist.halo_depth(attrs, fit_name, w)
        surf = (2 if fit == FL else 1) if mask & SURFACE else 0
        assert got == max(surf, w // 2 if mask & FUSED_WIN else 0, 1 if mask & RUGOSITY else 0), (attrs, fit_name, w)
        if mask & RUGOSITY and not mask & FUSED_WIN:
            assert py == max(got, w // 2), (attrs, fit_name, w)
            differ += py != got
        else:
            assert py == got, (attrs, fit_name, w)
    assert differ > 0
    # fractal roughness has a window size of its own, which dist.halo_depth has no argument for
    assert lib.tr_halo_depth(FRACTAL, FL, 13) == 6 and lib.tr_halo_depth(FRACTAL | SLOPE, FL, 3) == 2


# ---- span copy ----------------------------------------------------------------------------------------------------------------------
def test_span_copy_equals_a_plain_copy_and_keeps_its_bounds(lib):
    thr = lib.tr_copy_threshold()
    assert thr == 4 << 20
    rng = np.random.default_rng(17)
    lists = [[0], [0, 0, 0], [1], [thr - 1], [thr], [thr + 1], [thr // 2, 0, thr // 2 - 1], [thr // 2, 0, thr // 2], [0, thr + 5, 0, 3]]
    for _ in range(12):
        n = int(rng.integers(1, 14))
        sizes = rng.integers(0, int(rng.choice([2000, 300000, 1200000])), n)
        sizes[rng.random(n) < 0.25] = 0
        lists.append(sizes.tolist())
    threaded = 0
    for i, sizes in enumerate(lists):
        for nthreads in ((1, 2, 3, 8, 16, 17) if i % 2 else (1, 4, 5, 7, 9, 13)):
            a = np.array(sizes, np.int64)
            assert lib.tr_copy_case(p(a), a.size, nthreads, 100 + i) == 0, (sizes, nthreads)
            threaded += sum(sizes) >= thr and nthreads > 1
    assert threaded >= 20
    for nthreads in range(1, 18):
        a = np.array([5, 0, thr // 3, 7, thr // 3, 0, thr // 3 + 11], np.int64)
        assert lib.tr_copy_case(p(a), a.size, nthreads, nthreads) == 0


def test_span_copy_under_address_and_undefined_behaviour_sanitizers():
    """The same checks as a stand-alone program (its own main, nothing preloaded) built with -fsanitize=address,undefined."""
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
           "-static-libubsan", "-DTR_COPY_MAIN", "-o", COPY_CHECK, SRC]
    built = subprocess.run(cmd, capture_output=True, text=True)
    if built.returncode != 0:
        pytest.skip("g++ cannot link the sanitizer runtimes here: " + (built.stderr.strip().splitlines() or ["?"])[-1])
    for seed in (1, 2):
        run = subprocess.run([COPY_CHECK, str(seed)], capture_output=True, text=True)
        assert run.returncode == 0 and "cases OK" in run.stdout, (run.stdout, run.stderr[-2000:])
