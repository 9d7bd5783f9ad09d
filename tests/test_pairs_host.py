"""The host side of the variogram pair kernel on the CPU: the arithmetic that decides every pair's lag class
(xdem_amd/csrc/pairs_classes.h), the description of the kernel's LDS block (pairs_layout.h) and the decisions of the bracketed
exact-median selection (pairs_policy.h).  The headers are compiled with g++ into a small harness (tests/hostsim/pairs_hostsim.cpp);
every rule is restated here in NumPy / plain Python and compared exactly.
"""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostsim", "pairs_hostsim.cpp")
CSRC = os.path.join(os.path.dirname(HERE), "xdem_amd", "csrc")
HDRS = [os.path.join(CSRC, h) for h in ("pairs_classes.h", "pairs_layout.h", "pairs_policy.h", "sel_narrow.h")]
SO = os.path.join(HERE, "hostsim", "_pairs_hostsim.so")

OPS = {"sums_sq": 0, "sums_sqrt": 1, "hist": 2, "succ": 3, "bracket": 4}
PT, LUT_N, LUT_G, LUT_G0, NCOPY, SWEEP, STAGE_CAP = 256, 512, 256, 1016, 32, 128, 8192
DEFF_WIDE, DEFF_SPREAD = 4096, 4   # (select.h: PAIR_DEFF_WIDE, PAIR_DEFF_SPREAD)


def p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(q) for q in [SRC] + HDRS):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-pthread", "-shared", "-fPIC", "-o", SO, SRC])
    L = ctypes.CDLL(SO)
    L.ph_expected.restype = ctypes.c_double
    L.ph_expected.argtypes = [ctypes.c_uint64, ctypes.c_uint64, ctypes.c_double]
    L.ph_capacity.restype = ctypes.c_longlong
    L.ph_capacity.argtypes = [ctypes.c_double, ctypes.c_int64]
    L.ph_route.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int64, ctypes.c_int64]
    L.ph_bracket_min.restype = ctypes.c_int64
    L.ph_attempt_deff.restype = ctypes.c_uint32
    L.ph_attempt_deff.argtypes = [ctypes.c_int, ctypes.c_uint32, ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32]
    L.ph_bracket_ends32.argtypes = [ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int, ctypes.c_void_p]
    L.ph_bracket_ends64.argtypes = [ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int, ctypes.c_void_p]
    L.ph_rebase32.restype = ctypes.c_uint32
    L.ph_rebase64.restype = L.ph_rebase_wide.restype = ctypes.c_uint64
    for f in (L.ph_rebase32, L.ph_rebase64, L.ph_rebase_wide):
        f.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    L.ph_ranks.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    L.ph_thresholds.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    L.ph_binade_lut.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    L.ph_binade_classes.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]
    L.ph_cell_of_u32.argtypes = [ctypes.c_uint32]
    L.ph_make_grid.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                               ctypes.c_int] + [ctypes.c_void_p] * 4
    L.ph_lds_table.argtypes = [ctypes.c_int] * 5 + [ctypes.c_void_p, ctypes.c_void_p]
    L.ph_lds_pointers.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    c = np.zeros(10, np.int32)
    L.ph_constants(p(c))
    assert list(c[:7]) == [PT, 4096, LUT_N, LUT_G, LUT_G0, NCOPY, SWEEP] and c[8] == STAGE_CAP and c[9] == 12 * NCOPY
    L.acc_first = int(c[7])
    return L


# ---- thresholds on the squared distance ---------------------------------------------------------------------------------------
def edge_cases():
    tiny = np.nextafter(0.0, 1.0)
    return np.concatenate([np.geomspace(math.sqrt(2.0), 28283.0, 50), np.linspace(0.1, 1000.0, 97), np.sqrt(np.arange(1.0, 40.0)),
                           np.arange(1.0, 40.0), [0.0, tiny, 3 * tiny, 1.5e-154, 2.2250738585072014e-308, 1e-160, 1e150]])


def thresholds(lib, edges, strict=False):
    edges = np.ascontiguousarray(edges, np.float64)
    thr = np.zeros_like(edges)
    lib.ph_thresholds(p(edges), edges.size, int(strict), p(thr))
    return thr


def test_threshold_is_the_smallest_square_whose_root_reaches_the_edge(lib):
    e = edge_cases()
    t = thresholds(lib, e)
    below = np.nextafter(t, 0.0)
    assert np.all(np.sqrt(t) >= e)
    assert np.all((np.sqrt(below) < e) | (t == 0.0))       # (nothing lies below 0: every distance reaches an edge of 0)
    assert np.all(t[e == 0.0] == 0.0)


def test_strict_threshold_is_the_smallest_square_whose_root_exceeds_the_edge(lib):
    e = edge_cases()
    t = thresholds(lib, e, strict=True)
    assert np.all(np.sqrt(t) > e)
    assert np.all(np.sqrt(np.nextafter(t, 0.0)) <= e)
    assert np.all(t > 0.0)


# ---- binade table over d^2 ----------------------------------------------------------------------------------------------------
def binade_lut(lib, thr):
    lut, emin = np.zeros(LUT_N, np.uint8), ctypes.c_int(0)
    ok = lib.ph_binade_lut(p(thr), thr.size, p(lut), ctypes.byref(emin))
    return bool(ok), lut, emin.value


def test_binade_table_and_one_compare_give_the_searchsorted_class(lib):
    thr = thresholds(lib, np.geomspace(math.sqrt(2.0), 28283.0, 50))
    ok, lut, emin = binade_lut(lib, thr)
    assert ok
    rng = np.random.default_rng(5)
    s2 = np.concatenate([thr, np.nextafter(thr, 0.0), np.nextafter(thr, np.inf), [0.0, 1e-300, 1e-12, 0.5, 1.0, thr[0] / 4, thr[-1] * 2, 1e30, 1e300],
                         np.exp(rng.uniform(math.log(1e-3), math.log(4.0 * thr[-1]), 100000))])
    cls = np.zeros(s2.size, np.int32)
    lib.ph_binade_classes(p(thr), thr.size, p(lut), emin, p(s2), s2.size, p(cls))
    assert np.array_equal(cls, np.searchsorted(thr, s2, "right"))


def test_binade_table_is_refused_for_dense_edges_and_many_classes(lib):
    assert not binade_lut(lib, thresholds(lib, np.linspace(100.0, 1000.0, 40)))[0]        # several thresholds in one 1/8 binade
    # (distances over 30 binades = d^2 over 60 of the table's 64, a factor 1.39 between thresholds: never two in a cell)
    assert not binade_lut(lib, thresholds(lib, np.geomspace(1.0, 2.0**30, 128)))[0]       # 128 classes do not fit the entry
    assert not binade_lut(lib, thresholds(lib, np.geomspace(1.0, 2.0**30, 200)))[0]
    assert binade_lut(lib, thresholds(lib, np.geomspace(1.0, 2.0**30, 127)))[0]
    # a first threshold below the lowest cell the table can start at (exponent field 1: the cell index is clamped there) would be
    # missed by every d^2 that clamps onto cell 0: refused; a small but normal one is taken
    assert thresholds(lib, np.array([1e-160]))[0] < 2.0**-1022
    assert not binade_lut(lib, thresholds(lib, np.array([1e-160])))[0]
    assert binade_lut(lib, thresholds(lib, np.array([1e-150])))[0]


# ---- integer lattice --------------------------------------------------------------------------------------------------------
def make_grid(lib, a, b, thr):
    ax, ay = (np.ascontiguousarray(v, np.float64) for v in a)
    na = ax.size
    if b is None:
        bx = by = None
        nbt = 0
    else:
        bx, by = (np.ascontiguousarray(v, np.float64) for v in b)
        nbt = bx.size
    a_xy, b_xy, thr_i, lut = np.zeros(max(na, 1), np.uint32), np.zeros(max(nbt, 1), np.uint32), np.zeros(max(thr.size, 1), np.uint32), np.zeros(LUT_G, np.uint8)
    ok = lib.ph_make_grid(p(ax), p(ay), na, None if b is None else p(bx), None if b is None else p(by), nbt, p(thr), thr.size, p(a_xy), p(b_xy),
                          p(thr_i), p(lut))
    return bool(ok), a_xy[:na], b_xy[:nbt], thr_i, lut


def lattice_points(rng, n, spacing, origin, span=40):
    ix, iy = rng.integers(0, span, n), rng.integers(0, span, n)
    ix[:2], iy[:2] = [0, span - 1], [0, span - 1]
    return origin[0] + spacing * ix, origin[1] + spacing * iy


def classes_from_lattice(lib, a_xy, b_xy, thr_i, lut):
    ax, ay = (a_xy & 0xFFFF).astype(np.int64), (a_xy >> 16).astype(np.int64)
    bx, by = (b_xy & 0xFFFF).astype(np.int64), (b_xy >> 16).astype(np.int64)
    d2 = ((ax[:, None] - bx[None, :]) ** 2 + (ay[:, None] - by[None, :]) ** 2).astype(np.uint32)
    cell = (d2.astype(np.float32).view(np.uint32) >> 20).astype(np.int64)   # 1/8-binade cell of float(d2), as the kernel computes it
    low = lut[np.maximum(cell, LUT_G0) - LUT_G0].astype(np.int64)
    nxt = np.concatenate([thr_i, [0xFFFFFFFF]])[np.minimum(low, thr_i.size)]
    return low + (nxt <= d2)


@pytest.mark.parametrize("spacing,origin", [(1.0, (0.0, 0.0)), (0.5, (1000.25, -37.5)), (30.0, (432000.0, 5141000.0)), (2.5, (-7.5, 12.5))])
@pytest.mark.parametrize("pdist", [False, True])
def test_lattice_classes_equal_the_float64_classes_pair_by_pair(lib, spacing, origin, pdist):
    rng = np.random.default_rng(int(spacing * 10) + pdist)
    a = lattice_points(rng, 300, spacing, origin)
    b = a if pdist else lattice_points(rng, 280, spacing, origin)
    thr = thresholds(lib, np.geomspace(spacing * math.sqrt(2.0), spacing * 39 * math.sqrt(2.0), 14))
    ok, a_xy, b_xy, thr_i, lut = make_grid(lib, a, None if pdist else b, thr)
    assert ok
    if pdist:
        b_xy = a_xy
    dx, dy = a[0][:, None] - b[0][None, :], a[1][:, None] - b[1][None, :]
    want = np.searchsorted(thr, dx * dx + dy * dy, "right")
    assert np.array_equal(classes_from_lattice(lib, a_xy, b_xy, thr_i, lut), want)
    # the packed indexes reproduce the coordinates
    x0, y0 = min(a[0].min(), b[0].min()), min(a[1].min(), b[1].min())
    for xy, (x, y) in ((a_xy, a), (b_xy, b)):
        assert np.array_equal(x0 + spacing * (xy & 0xFFFF), x) and np.array_equal(y0 + spacing * (xy >> 16), y)


def test_lattice_route_is_refused(lib):
    rng = np.random.default_rng(11)
    thr = thresholds(lib, np.geomspace(math.sqrt(2.0), 60.0, 12))
    x, y = lattice_points(rng, 200, 1.0, (5.0, 7.0))
    assert make_grid(lib, (x, y), None, thr)[0]
    off = x.copy(); off[17] += 1e-3 / 3.0
    assert not make_grid(lib, (off, y), None, thr)[0]                       # an off-lattice point
    nan = y.copy(); nan[3] = np.nan
    assert not make_grid(lib, (x, nan), None, thr)[0]                       # a NaN coordinate
    far = x.copy(); far[5] = x.min() + 32768.0
    assert not make_grid(lib, (far, y), None, thr)[0]                       # index span above 32767
    assert make_grid(lib, (np.where(np.arange(200) == 5, x.min() + 32767.0, x), y), None, thresholds(lib, np.geomspace(2.0, 4e4, 12)))[0]
    # G * imax >= 2^26: lattice constant 4096, thresholds scaled to it (integer thresholds 2 .. 2e8, a factor 5 apart: one per cell
    # at most), so that nothing but the size of the coordinates refuses the set; one index less is taken
    thr_g = thresholds(lib, np.geomspace(4096.0 * math.sqrt(2.0), 4096.0 * 2.0e4, 12))
    assert not make_grid(lib, (np.array([0.0, 4096.0 * 16384.0]), np.array([0.0, 4096.0])), None, thr_g)[0]    # G * imax = 2^26
    assert make_grid(lib, (np.array([0.0, 4096.0 * 16383.0]), np.array([0.0, 4096.0])), None, thr_g)[0]        # 2^26 - 4096
    # more than 255 classes: twelve edges among the distances, the others beyond every distance (their integer thresholds saturate
    # at all-ones and lie in no cell), so that nothing but the class count refuses the set; 255 classes are taken
    def many(n):
        return thresholds(lib, np.concatenate([np.geomspace(math.sqrt(2.0), 60.0, 12), np.linspace(1.0e5, 2.0e5, n - 12)]))
    assert not make_grid(lib, (x, y), None, many(256))[0]
    ok255, _, _, thr_i255, lut255 = make_grid(lib, (x, y), None, many(255))
    assert ok255 and np.all(thr_i255[12:] == 0xFFFFFFFF) and lut255.max() == 12
    assert not make_grid(lib, (x, y), None, thresholds(lib, np.array([30.0, 30.01, 60.0])))[0]   # two integer thresholds in one cell
    assert not make_grid(lib, (np.zeros(0), np.zeros(0)), None, thr)[0]     # an empty set


def test_lattice_scan_does_not_depend_on_the_host_threads(lib):
    rng = np.random.default_rng(3)
    n = 3 * 65536 + 1234                                                     # longer than two 64 K pieces
    a = lattice_points(rng, n, 0.5, (100.0, -50.0), span=2000)
    b = lattice_points(rng, 70000, 0.5, (100.0, -50.0), span=2000)
    thr = thresholds(lib, np.geomspace(1.0, 1500.0, 20))
    got = []
    old = os.environ.get("XDEM_HOST_THREADS")
    try:
        for t in ("1", "4"):
            os.environ["XDEM_HOST_THREADS"] = t
            assert lib.ph_host_threads() == int(t)
            got.append(make_grid(lib, a, b, thr))
    finally:
        if old is None:
            os.environ.pop("XDEM_HOST_THREADS", None)
        else:
            os.environ["XDEM_HOST_THREADS"] = old
    assert got[0][0] and got[1][0]
    for u, v in zip(got[0][1:], got[1][1:]):
        assert np.array_equal(u, v)


# ---- LDS layout ---------------------------------------------------------------------------------------------------------------
def lds_table(lib, f64, op, wide, nb, nbs):
    out, total = np.zeros(5 * 32, np.int64), ctypes.c_uint64(0)
    n = lib.ph_lds_table(int(f64), op, int(wide), nb, nbs, p(out), ctypes.byref(total))
    assert n > 0
    return out[:5 * n].reshape(n, 5), int(total.value)


def parent_lds_bytes(es, nb, op, nbs, wide):
    """The hand formula the launch used before the layout had one description (with its slack terms), as a literal expression."""
    base = 8 * (2 * 256 + nb + 1 + 1) + 16 * nb + es * 256 + 8 + 4 * (256 + nb + 4)
    if op == OPS["hist"]:
        return base + nbs * 256 * 4
    if op == OPS["bracket"]:
        return base + (nb + 1) * 32 * 8 + 4 * (nb + 1) * es + 4 * (nb + 2) + 8 + (4096 if wide else 8192) * ((8 if wide else es) + 2) + 16
    if op == OPS["succ"]:
        return base + nb * es
    return base + (nb + 1) * 32 * 12


@pytest.mark.parametrize("nb", [1, 2, 50, 127, 128, 255, 1024])
def test_lds_regions_follow_each_other_aligned_and_within_the_old_bound(lib, nb):
    for nbs in (1, 64, 128):
        for f64, es in ((0, 4), (1, 8)):
            acc = set()
            for name, op in OPS.items():
                for wide in ((0, 1) if (op == OPS["bracket"] and not f64) else (0,)):
                    t, total = lds_table(lib, f64, op, wide, nb, nbs)
                    ids, offs, elem, cnt, align = t.T
                    assert np.all(np.diff(ids) > 0)                                      # each region once, in the order of the enumeration
                    assert offs[0] == 0 and np.all(offs[1:] >= offs[:-1] + elem[:-1] * cnt[:-1])   # no overlap
                    assert np.all(offs % align == 0) and np.all(elem > 0) and np.all(cnt >= 0)
                    hand = int(np.sum(elem * cnt))
                    assert hand <= total <= parent_lds_bytes(es, nb, op, nbs, wide)
                    assert total == offs[-1] + elem[-1] * cnt[-1]
                    # the declared alias: every operation's accumulators start at the same place, 8-byte aligned, right behind the class tables
                    first = int(np.argmax(ids >= lib.acc_first))
                    assert ids[first] >= lib.acc_first and np.all(ids[:first] < lib.acc_first) and first == 9
                    acc.add(int(offs[first]))
                    assert offs[first] % 8 == 0
                    # what the kernel relies on
                    by = dict(zip(ids.tolist(), zip(offs.tolist(), elem.tolist(), cnt.tolist())))
                    assert by[0][2] == by[1][2] == PT and by[2][2] == nb and by[3][2] == 2 and by[8][2] >= nb + 2
                    if op == OPS["hist"]:
                        assert cnt[first] == nbs * 256
            assert len(acc) == 1


def test_bracket_block_lets_two_workgroups_share_a_cu(lib):
    # Two workgroups share a CU's 160 KB of LDS while each takes at most 80 KB (the launch's own rule).  The bound at the most
    # classes the bracketed route takes (128) is what the old formula gave there; wherever the old formula stayed within 80 KB --
    # the benchmark's 50 classes among them -- the block must stay within it too.
    for f64, es, wide in ((0, 4, 0), (0, 4, 1), (1, 8, 0)):
        assert lds_table(lib, f64, OPS["bracket"], wide, 128, 0)[1] <= parent_lds_bytes(es, 128, OPS["bracket"], 0, wide)
        for nb in range(1, 129):
            if parent_lds_bytes(es, nb, OPS["bracket"], 0, wide) <= 80 * 1024:
                assert lds_table(lib, f64, OPS["bracket"], wide, nb, 0)[1] <= 80 * 1024
    assert parent_lds_bytes(4, 50, OPS["bracket"], 0, 0) <= 80 * 1024 and parent_lds_bytes(4, 50, OPS["bracket"], 0, 1) <= 80 * 1024


def test_kernel_pointers_are_the_table_offsets(lib):
    for nb in (1, 50, 128):
        t, total = lds_table(lib, 0, OPS["bracket"], 0, nb, 0)
        buf = np.zeros(total + 64, np.uint8)
        off = np.full(32, -2, np.int64)
        lib.ph_lds_pointers(nb, p(buf), p(off))
        for rid, o in zip(t[:, 0], t[:, 1]):
            assert off[rid] == o
        assert sorted(np.flatnonzero(off[:19] == -1).tolist()) == [9, 10, 11]       # rec, hist, min: other operations' regions


# ---- policy of the bracketed selection ----------------------------------------------------------------------------------------
def ranks(lib, total, below, inside, overflow=False):
    a = [np.ascontiguousarray(v, np.uint64) for v in (total, below, inside)]
    given = np.full(len(total), 12345, np.uint64)
    rc = lib.ph_ranks(p(a[0]), p(a[1]), p(a[2]), len(total), int(overflow), p(given))
    return rc, given


def test_ranks_from_counts(lib):
    NONE = np.uint64(2**64 - 1)
    # odd total 101: rank 50; 40 below, 20 inside -> candidate 10
    rc, g = ranks(lib, [101], [40], [20])
    assert rc == -1 and g[0] == 10
    # even total 100: ranks 49 and 50 must both be inside
    rc, g = ranks(lib, [100], [40], [11])
    assert rc == -1 and g[0] == 9                      # candidates 40 .. 50 hold ranks 49 and 50
    assert ranks(lib, [100], [40], [10])[0] == 0       # rank 50 lies just above the bracket
    assert ranks(lib, [100], [50], [30])[0] == 0       # rank 49 lies just below the bracket
    assert ranks(lib, [101], [51], [30])[0] == 0
    assert ranks(lib, [101], [50], [1])[0] == -1 and ranks(lib, [101], [50], [0])[0] == 0
    # an empty class is skipped; the bracket may hold the whole class
    rc, g = ranks(lib, [0, 7, 8], [0, 0, 0], [0, 7, 8])
    assert rc == -1 and g[0] == NONE and g[1] == 3 and g[2] == 3
    # the first missed class is reported, classes before it have their ranks
    rc, g = ranks(lib, [101, 101, 101], [40, 60, 40], [20, 20, 20])
    assert rc == 1 and g[0] == 10
    # overflow of the candidate buffer: nothing is ranked
    rc, g = ranks(lib, [101], [40], [20], overflow=True)
    assert rc == -2 and g[0] == 12345


def key32(v):
    return (np.asarray(v, np.float32).view(np.uint32).astype(np.uint64) << np.uint64(1)).astype(np.uint32)


def test_rebase_origins_plain(lib):
    rng = np.random.default_rng(9)
    lo = np.abs(rng.normal(size=64)).astype(np.float32)
    hi = (lo + np.abs(rng.normal(size=64)).astype(np.float32) * 0.01).astype(np.float32)
    klo, khi = key32(lo), key32(hi) | np.uint32(1)
    khi[5], klo[5] = klo[5] - np.uint32(2), klo[5]     # an empty bracket
    origin = np.zeros(64, np.uint32)
    widest = lib.ph_rebase32(p(klo), p(khi), 64, p(origin))
    top = np.uint32(1 << 31)
    want_r = np.where(khi >= klo, (khi >> 1).astype(np.int64) - (klo >> 1).astype(np.int64), 0)
    assert np.array_equal(origin, (klo >> 1) | top) and widest == want_r.max() and want_r[5] == 0
    # every candidate value in [lo, hi] has its key (bits | top) at or above the origin and within the range
    for k in range(64):
        if k == 5:
            continue
        for v in (lo[k], hi[k], np.nextafter(lo[k], np.float32(np.inf)), np.nextafter(hi[k], np.float32(0))):
            key = int(np.float32(v).view(np.uint32)) | (1 << 31)
            assert int(origin[k]) <= key <= int(origin[k]) + int(widest)
    klo64 = (np.abs(rng.normal(size=8)).view(np.uint64) << np.uint64(1))
    khi64 = klo64 + np.uint64(1000)
    o64 = np.zeros(8, np.uint64)
    assert lib.ph_rebase64(p(klo64), p(khi64), 8, p(o64)) == 500 and np.array_equal(o64, (klo64 >> np.uint64(1)) | np.uint64(1 << 63))
    empty = np.array([key32(2.0)], np.uint32), np.array([key32(1.0)], np.uint32)
    assert lib.ph_rebase32(p(empty[0]), p(empty[1]), 1, p(origin)) == 0


def test_rebase_origins_wide(lib):
    rng = np.random.default_rng(10)
    n = 200
    lo = np.abs(rng.normal(size=n)).astype(np.float32)
    lo[:3] = [0.0, np.float32(1e-45), np.float32(3.0)]
    hi = (lo * np.float32(1.001) + np.float32(1e-6)).astype(np.float32)
    klo, khi = key32(lo), key32(hi)
    origin = np.zeros(n, np.uint64)
    widest = int(lib.ph_rebase_wide(p(klo), p(khi), n, p(origin)))
    top = 1 << 63
    for k in range(n):
        L, H = float(lo[k]), float(hi[k])
        # float64 neighbours of the ends, inside and outside: those whose float32 rounding lies in [L, H] are candidates
        cands = [L, H, np.nextafter(L, -np.inf), np.nextafter(L, np.inf), np.nextafter(H, np.inf), np.nextafter(H, -np.inf),
                 0.5 * (L + float(np.nextafter(lo[k], np.float32(-np.inf)))), 0.5 * (H + float(np.nextafter(hi[k], np.float32(np.inf))))]
        for d in cands:
            if d < 0 or not (L <= float(np.float32(d)) <= H):
                continue
            key = int(np.float64(d).view(np.uint64)) | top
            assert int(origin[k]) <= key <= int(origin[k]) + widest, (k, d)
    e = np.array([key32(2.0)], np.uint32), np.array([key32(1.0)], np.uint32)
    assert lib.ph_rebase_wide(p(e[0]), p(e[1]), 1, p(origin)) == 0      # empty brackets give range 0


def test_design_effect_retry_sequence(lib):
    def sequence(pdist):
        seq, deff = [], 0
        for attempt in range(5):
            deff = lib.ph_attempt_deff(attempt, deff, int(pdist), DEFF_WIDE, DEFF_SPREAD)
            if not deff:
                break
            seq.append(deff)
        return seq

    assert sequence(True) == [4096]                  # i < j blocks start with the wide rule: nothing wider to retry with
    assert sequence(False) == [4, 64, 4096]          # spread samples: 16 x the design effect, then the wide rule
    assert lib.ph_attempt_deff(1, 512, 0, DEFF_WIDE, DEFF_SPREAD) == 4096 and lib.ph_attempt_deff(3, 64, 0, DEFF_WIDE, DEFF_SPREAD) == 0


def test_route_predicate_at_its_boundaries(lib):
    m = lib.ph_bracket_min()
    assert m == 4_000_000_000
    assert lib.ph_route(0, 128, m, 256) == 1 and lib.ph_route(2, 128, m, 256) == 1
    assert lib.ph_route(1, 128, m, 256) == 0         # switched off
    assert lib.ph_route(0, 129, m, 256) == 0         # more classes than one histogram sweep
    assert lib.ph_route(0, 128, m - 1, 256) == 0     # too few pairs
    assert lib.ph_route(0, 128, m, 255) == 0         # too few units


def test_bracket_ends_and_capacity(lib):
    out = np.zeros(2, np.uint32)
    lib.ph_bracket_ends32(10, 0x40001200, 0x40003400, 0xFF, 0, p(out))
    assert list(out) == [0x40001200, 0x400034FF]
    lib.ph_bracket_ends32(0, 0x40001200, 0x40003400, 0xFF, 0, p(out))
    assert list(out) == [0, 0xFFFFFFFF]              # no sampled pair: the bracket holds everything
    lib.ph_bracket_ends32(10, 0x40001200, 0x40003400, 0xFF, 2, p(out))
    assert list(out) == [0x40001200, 0x40001200]     # test mode: collapsed
    lib.ph_bracket_ends32(0, 0x40001200, 0x40003400, 0xFF, 2, p(out))
    assert list(out) == [0, 0xFFFFFFFF]
    o64 = np.zeros(2, np.uint64)
    lib.ph_bracket_ends64(3, 1 << 62, (1 << 62) + (1 << 41), (1 << 40) - 1, 0, p(o64))
    assert [int(v) for v in o64] == [1 << 62, (1 << 62) + (1 << 41) + (1 << 40) - 1]
    assert lib.ph_expected(10**6, 500, 64.0) == 64.0 * 1002.0 and lib.ph_expected(100, 500, 128.0) == 128.0 * 100.0
    assert lib.ph_capacity(1e6, 10**12) == int(1.5e6 + 2**20) and lib.ph_capacity(1e12, 10**9) == 10**9 + 1024
