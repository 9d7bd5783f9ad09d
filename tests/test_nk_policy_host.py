"""The two host policies of the one-pass Nuth-Kaab step (xdem_amd/csrc/nk_policy.h) and the sizes of its device blocks
(nk_layout.h), on the CPU: the headers are compiled with g++ into a small harness (tests/hostsim/nk_policy_hostsim.cpp) and every
decision is compared with the rule restated here in float64.

Decisions and codes must be equal.  Float outputs must be equal to the last bit -- sqrt, min, max, + - * / are correctly rounded
on both sides -- except the three that go through sin / cos: the predicted bin brackets (lo, hi) and the measured error of the
bins' centres (err).  The model takes math.sin / math.cos, which are the C library's like the harness's, so they agree in
practice too; should the two come from different libraries they may differ by 1 ulp there, and those three outputs are given 1 ulp
(the sines are multiplied by shift changes of a thousandth and added to medians of order one: their last bit hardly ever shows).

The step's packed result block is sized from the step's own table of items, evaluated here with a selection state of select.h's
members; the parent's hand formula (160 bytes per bin + 1024) was an upper bound of that sum, so the size is checked against the
hand sum of the items and against that bound, not for equality with it.
"""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

from hostsim_util import ulp_diff

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostsim", "nk_policy_hostsim.cpp")
CSRC = os.path.join(os.path.dirname(HERE), "xdem_amd", "csrc")
HDRS = [os.path.join(CSRC, h) for h in ("nk_policy.h", "nk_layout.h", "sel_narrow.h")]
SO = os.path.join(HERE, "hostsim", "_nk_policy_hostsim.so")

c_dp = ctypes.POINTER(ctypes.c_double)
c_ip = ctypes.POINTER(ctypes.c_int64)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(p) for p in [SRC] + HDRS):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-o", SO, SRC])
    L = ctypes.CDLL(SO)
    for name in ("nkp_narrow_new", "nkp_pred_new"):
        getattr(L, name).restype = ctypes.c_void_p
    L.nkp_narrow_free.argtypes = L.nkp_narrow_reset.argtypes = [ctypes.c_void_p]
    L.nkp_narrow_observe.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_double]
    L.nkp_narrow_choose_next.argtypes = L.nkp_narrow_on_miss.argtypes = [ctypes.c_void_p, ctypes.c_int]
    L.nkp_narrow_get.argtypes = [ctypes.c_void_p, c_dp, c_ip]
    L.nkp_narrow_unit.argtypes = [ctypes.c_uint32]
    L.nkp_narrow_unit.restype = ctypes.c_double
    L.nkp_narrowed.argtypes = [ctypes.c_uint64, ctypes.c_uint32]
    L.nkp_narrowed.restype = ctypes.c_uint64
    L.nkp_pred_free.argtypes = L.nkp_pred_on_miss.argtypes = L.nkp_pred_forget.argtypes = [ctypes.c_void_p]
    L.nkp_pred_set.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 5
    L.nkp_pred_get.argtypes = [ctypes.c_void_p] * 7
    L.nkp_pred_plan.argtypes = [ctypes.c_void_p, ctypes.c_double, ctypes.c_double, ctypes.c_int, ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 4
    L.nkp_pred_record.argtypes = [ctypes.c_void_p, ctypes.c_double, ctypes.c_double, ctypes.c_int, ctypes.c_double] + [ctypes.c_void_p] * 5 + [
        ctypes.c_double, ctypes.c_double, ctypes.c_int]
    for name in ("nkp_fz_zeroed_words", "nkp_mr_small_words"):
        getattr(L, name).argtypes = [ctypes.c_int64]
        getattr(L, name).restype = ctypes.c_int64
    L.nkp_fz_total_bytes.argtypes = [ctypes.c_int64]
    L.nkp_fz_total_bytes.restype = ctypes.c_uint64
    L.nkp_fz_offsets.argtypes = [ctypes.c_int64, ctypes.c_void_p]
    L.nkp_fetch_bytes.argtypes = [ctypes.c_int, ctypes.c_int]
    L.nkp_fetch_bytes.restype = ctypes.c_uint64
    return L


def same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float64).view(np.uint64), np.asarray(b, np.float64).view(np.uint64))


# ---- bracket narrowing -------------------------------------------------------------------------------------------------------
def unit_of(code):
    """Fraction of the full bracket rule a narrow code stands for: below 16 a right shift, 16 + q = q sixteenths."""
    return 1.0 / float(1 << code) if code < 16 else float(code - 16) / 16.0


class NarrowModel:
    def __init__(self):
        self.narrow, self.unit_min, self.worst, self.off2, self.offn = 0, 0.25, 0.0, 0.0, 0

    def observe(self, tot, lt, inside, unit):
        if tot < 4096 or inside < 64 or inside >= tot:
            return
        o = abs((float(tot - 1) * 0.5 - float(lt)) - 0.5 * float(inside)) / (0.5 * float(inside)) * unit
        self.worst = max(self.worst, o)
        self.off2 += o * o
        self.offn += 1

    def choose_next(self, option):
        nxt = 0
        if self.offn >= 24:
            sigma = math.sqrt(self.off2 / float(self.offn))
            for q in (4, 5, 6, 7, 8, 10, 12):
                u = q / 16.0
                if 4.8 * sigma <= u and 1.5 * self.worst <= u and u >= self.unit_min:
                    nxt = {8: 1, 4: 2}.get(q, 16 + q)
                    break
        if option >= 0:
            nxt = option
        self.narrow = nxt
        return nxt

    def on_miss(self, used):
        if used > 0:
            self.unit_min = min(1.0, 1.5 * unit_of(used))
            self.narrow = 0


class Narrow:
    """The harness's object next to the model: every call goes to both, the states are compared after each."""

    def __init__(self, lib):
        self.lib, self.p, self.m = lib, ctypes.c_void_p(lib.nkp_narrow_new()), NarrowModel()

    def close(self):
        self.lib.nkp_narrow_free(self.p)

    def check(self):
        out = np.zeros(3)
        n = np.zeros(1, np.int64)
        code = self.lib.nkp_narrow_get(self.p, out.ctypes.data_as(c_dp), n.ctypes.data_as(c_ip))
        assert code == self.m.narrow and int(n[0]) == self.m.offn
        assert same_bits(out, [self.m.unit_min, self.m.worst, self.m.off2])

    def observe(self, tot, lt, inside, unit=1.0):
        self.lib.nkp_narrow_observe(self.p, tot, lt, inside, unit)
        self.m.observe(tot, lt, inside, unit)
        self.check()

    def offsets(self, thousandths, unit=1.0):
        """Observations whose wanted rank lies d / 1000 half widths off the centre: total 100001, 2000 inside the bracket."""
        for d in thousandths:
            self.observe(100001, 50000 - 1000 - d, 2000, unit)

    def choose_next(self, option=-1):
        got = self.lib.nkp_narrow_choose_next(self.p, option)
        assert got == self.m.choose_next(option)
        self.check()
        return got

    def on_miss(self, used):
        self.lib.nkp_narrow_on_miss(self.p, used)
        self.m.on_miss(used)
        self.check()


@pytest.fixture
def narrow(lib):
    s = Narrow(lib)
    yield s
    s.close()


def test_narrow_codes(lib):
    for code, unit in ((0, 1.0), (1, 0.5), (2, 0.25), (16 + 5, 5 / 16), (16 + 12, 0.75), (16 + 16, 1.0)):
        assert lib.nkp_narrow_unit(code) == unit == unit_of(code)
    for h in (32, 33, 1000, 123457):
        w = h - 32
        assert [lib.nkp_narrowed(h, c) for c in (0, 1, 2, 21, 28)] == [w + 32, (w >> 1) + 32, (w >> 2) + 32, ((w * 5) >> 4) + 32, ((w * 12) >> 4) + 32]


def test_narrowing_needs_24_observations(narrow):
    narrow.offsets([40] * 23)
    assert narrow.choose_next() == 0
    narrow.offsets([40])
    assert narrow.choose_next() == 2   # (rms 0.04, worst 0.04: a quarter of the rule holds 4.8 sigma and 1.5 x the worst)


def test_narrowing_rms_one_seventeenth_worst_a_fifth_gives_five_sixteenths(narrow):
    narrow.offsets([200] + [52] * 49)
    assert abs(math.sqrt(narrow.m.off2 / narrow.m.offn) - 1 / 17) < 2e-4 and narrow.m.worst == 0.2
    assert narrow.choose_next() == 16 + 5


def test_narrowing_rows_of_a_half_and_a_quarter(narrow):
    narrow.offsets([300] + [40] * 49)   # 1.5 x 0.3 = 0.45: above seven sixteenths, within eight
    assert narrow.choose_next() == 1
    narrow.lib.nkp_narrow_reset(narrow.p)
    narrow.m = NarrowModel()
    narrow.check()
    narrow.offsets([40] * 50)
    assert narrow.choose_next() == 2


def test_narrowing_miss_raises_the_floor(narrow):
    narrow.offsets([40] * 50)
    assert narrow.choose_next() == 2
    narrow.on_miss(1)   # brackets of one half missed: nothing below 1.5 x 0.5 again
    assert narrow.m.unit_min == 0.75 and narrow.m.narrow == 0
    assert narrow.choose_next() == 16 + 12
    narrow.on_miss(0)   # (full brackets missed: nothing to learn about narrowing)
    assert narrow.m.unit_min == 0.75
    narrow.on_miss(2)
    assert narrow.m.unit_min == 0.375
    assert narrow.choose_next() == 16 + 6


def test_narrowing_option_overrides_the_rule(narrow):
    narrow.offsets([40] * 50)
    for option in (0, 1, 2):
        assert narrow.choose_next(option) == option
    assert narrow.choose_next(-1) == 2


def test_narrowing_ignores_small_or_degenerate_brackets(narrow):
    narrow.observe(4095, 1000, 2000)     # fewer than 4096 values
    narrow.observe(100001, 49000, 63)    # fewer than 64 inside
    narrow.observe(5000, 0, 5000)        # everything inside
    narrow.observe(5000, 0, 6000)
    assert narrow.m.offn == 0
    narrow.observe(4096, 1000, 64)
    assert narrow.m.offn == 1
    narrow.offsets([100], unit=0.5)      # (offsets are kept in units of the FULL rule)
    assert narrow.m.worst == max(0.1 * 0.5, narrow.m.worst)


# ---- predicted brackets ------------------------------------------------------------------------------------------------------
MAX_BINS = 128


class Brackets:
    pass


class PredModel:
    def __init__(self):
        self.have, self.nb, self.cooldown = False, 0, 0
        self.sx = self.sy = self.v = self.wd = 0.0
        self.err = self.err_d = self.dpx = 1e30
        self.med, self.w, self.mid, self.ok = [], [], [], []
        self.n_predicted = self.n_predicted_d = self.n_predict_miss = 0

    def plan(self, dE, dN, nb, allow, option):
        s = Brackets()
        s.dE, s.dN = dE, dN
        s.dpx = math.sqrt(dE * dE + dN * dN)
        scaled = 0 < self.dpx < 1e29
        # the miss to expect: the last measured one scaled by the ratio of the shift changes, floor 0.02
        expect = max(0.02, self.err * (s.dpx / self.dpx)) if scaled else 1e30
        expect_d = max(0.02, self.err_d * (s.dpx / self.dpx)) if scaled else 1e30
        ready = allow and option != 0 and self.have and self.nb == nb and self.cooldown == 0 and self.wd > 0
        s.predict = bool(ready and nb <= MAX_BINS and expect <= 0.20 and expect_d <= 0.20 and s.dpx <= 0.05)
        s.predict_d = bool(ready and not s.predict and expect_d <= 0.35 and s.dpx <= 0.6)
        if self.cooldown > 0 and allow:
            self.cooldown -= 1
        s.h, s.hd, s.lo, s.hi = 1.0, 0.0, [], []
        if s.predict or s.predict_d:
            s.hd = min(1.0, max(0.25, 2.0 * expect_d + 0.15)) * self.wd
        if s.predict:
            s.h = min(1.0, max(0.25, 2.0 * expect + 0.15))
            for b in range(nb):
                if not self.ok[b]:
                    s.lo.append(1.0)
                    s.hi.append(0.0)
                    continue
                c = self.med[b] - (dE * math.sin(self.mid[b]) + dN * math.cos(self.mid[b]))
                hw = s.h * self.w[b] + 0.05 * s.dpx
                s.lo.append(c - hw)
                s.hi.append(c + hw)
        return s

    def on_miss(self):
        self.n_predict_miss += 1
        self.cooldown = 1
        self.err = self.err_d = 1e30

    def record(self, s, dc, dr, nb, vs, med, counts, edges, lo, hi, dlo, dhi, narrow):
        if self.have and self.nb == nb:
            worst = 0.0
            for b in range(nb):
                if self.ok[b] and counts[b] != 0 and self.w[b] > 0:
                    moved = self.med[b] - (s.dE * math.sin(self.mid[b]) + s.dN * math.cos(self.mid[b]))
                    worst = max(worst, abs(med[b] - moved) / self.w[b])
            self.err = worst
            self.err_d = abs(vs - self.v) / self.wd if self.wd > 0 else 1e30
            self.dpx = max(s.dpx, 1e-5)
        else:
            self.err = self.err_d = self.dpx = 1e30
        if not s.predict or len(self.w) != nb:   # widths of SAMPLED brackets only, in units of half the rule
            norm = 0.5 / unit_of(narrow) if narrow >= 16 else 1.0
            self.w = [norm * 0.5 * (hi[b] - lo[b]) if counts[b] > 0 and hi[b] >= lo[b] else 0.0 for b in range(nb)]
            if not s.predict_d:
                self.wd = norm * 0.5 * (dhi - dlo) if dhi >= dlo else 0.0
        self.med = list(med)
        self.mid = [0.5 * (edges[b] + edges[b + 1]) for b in range(nb)]
        self.ok = [int(counts[b] > 0 and self.w[b] > 0 and math.isfinite(self.w[b]) and math.isfinite(med[b])) for b in range(nb)]
        self.v, self.sx, self.sy, self.nb, self.have = vs, dc, dr, nb, True
        self.n_predicted += int(s.predict)
        self.n_predicted_d += int(s.predict_d)


def f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


class Pred:
    def __init__(self, lib):
        self.lib, self.p, self.m, self.last = lib, ctypes.c_void_p(lib.nkp_pred_new()), PredModel(), None

    def close(self):
        self.lib.nkp_pred_free(self.p)

    def set(self, nb, err=0.05, err_d=0.05, dpx=0.002, wd=0.01, cooldown=0, ok=None, seed=0):
        """The record of a settled fit: medians of order one on a cosine, sampled half widths of a few hundredths."""
        rng = np.random.default_rng(seed)
        m = self.m
        m.have, m.nb, m.cooldown = True, nb, cooldown
        m.sx, m.sy, m.v, m.wd, m.err, m.err_d, m.dpx = 0.25, -0.5, 1.75, wd, err, err_d, dpx
        m.mid = list((np.arange(nb) + 0.5) * (2 * np.pi / nb))
        m.med = list(1.5 + np.cos(0.7 - np.array(m.mid)) + 0.01 * rng.normal(size=nb))
        m.w = list(rng.uniform(0.02, 0.05, nb))
        m.ok = list(np.ones(nb, np.uint8) if ok is None else np.asarray(ok, np.uint8))
        sc = f64([m.sx, m.sy, m.v, m.wd, m.err, m.err_d, m.dpx])
        med, w, mid, okb = f64(m.med), f64(m.w), f64(m.mid), np.ascontiguousarray(m.ok, dtype=np.uint8)
        self.lib.nkp_pred_set(self.p, 1, nb, cooldown, sc.ctypes.data, med.ctypes.data, w.ctypes.data, mid.ctypes.data, okb.ctypes.data)
        self.check()

    def check(self):
        ints, sc = np.zeros(7, np.int64), np.zeros(7)
        med, w, mid, ok = np.zeros(256), np.zeros(256), np.zeros(256), np.zeros(256, np.uint8)
        self.lib.nkp_pred_get(self.p, ints.ctypes.data, sc.ctypes.data, med.ctypes.data, w.ctypes.data, mid.ctypes.data, ok.ctypes.data)
        m = self.m
        assert list(ints) == [int(m.have), m.nb, m.cooldown, m.n_predicted, m.n_predicted_d, m.n_predict_miss, len(m.w)]
        if not m.have:
            return
        got = dict(zip(("sx", "sy", "v", "wd", "err", "err_d", "dpx"), sc))
        for k in ("sx", "sy", "v", "wd", "err_d", "dpx"):
            assert same_bits(got[k], getattr(m, k)), k
        assert ulp_diff(f64([got["err"]]), f64([m.err]))[0] <= 1   # (through sin / cos)
        nb = m.nb
        assert same_bits(med[:nb], m.med) and same_bits(w[:nb], m.w) and same_bits(mid[:nb], m.mid) and list(ok[:nb]) == list(m.ok)

    def plan(self, dE, dN, nb, allow=True, option=1):
        flags, sc = np.zeros(2, np.int32), np.zeros(3)
        lo, hi = np.zeros(256), np.zeros(256)
        self.lib.nkp_pred_plan(self.p, dE, dN, nb, int(allow), option, flags.ctypes.data, sc.ctypes.data, lo.ctypes.data, hi.ctypes.data)
        s = self.m.plan(dE, dN, nb, allow, option)
        assert (bool(flags[0]), bool(flags[1])) == (s.predict, s.predict_d)
        assert same_bits(sc, [s.dpx, s.h, s.hd])
        if s.predict:
            assert ulp_diff(lo[:nb], f64(s.lo)).max() <= 1 and ulp_diff(hi[:nb], f64(s.hi)).max() <= 1   # (through sin / cos)
        self.check()
        self.last = s
        return s

    def record(self, dc, dr, nb, vs, med, counts, edges, lo, hi, dlo, dhi, narrow):
        a = [f64(med), np.ascontiguousarray(counts, dtype=np.int64), f64(edges), f64(lo), f64(hi)]
        self.lib.nkp_pred_record(self.p, dc, dr, nb, vs, *[x.ctypes.data for x in a], dlo, dhi, narrow)
        self.m.record(self.last, dc, dr, nb, vs, list(a[0]), list(a[1]), list(a[2]), list(a[3]), list(a[4]), dlo, dhi, narrow)
        self.check()


@pytest.fixture
def pred(lib):
    s = Pred(lib)
    yield s
    s.close()


def test_no_previous_step_no_prediction(pred):
    s = pred.plan(0.001, 0.0, 36)
    assert not s.predict and not s.predict_d
    pred.set(36)
    pred.lib.nkp_pred_forget(pred.p)
    pred.m.have = False
    s = pred.plan(0.001, 0.0, 36)
    assert not s.predict and not s.predict_d


def test_small_shift_change_predicts_every_bracket(pred):
    pred.set(36, err=0.05, dpx=0.002)
    s = pred.plan(0.001, 0.0, 36)
    expect = max(0.02, 0.05 * (0.001 / 0.002))
    assert s.predict and not s.predict_d and s.h == max(0.25, 2 * expect + 0.15) and s.hd == s.h * 0.01
    pred.set(36, err=0.15, err_d=0.15, dpx=0.002)
    s = pred.plan(0.0, 0.002, 36)   # as far as the last step: 2 x 0.15 + 0.15 sampled half widths
    assert s.predict and s.h == 2.0 * 0.15 + 0.15
    assert not pred.plan(0.0, 0.001, 36, option=0).predict
    assert not pred.plan(0.0, 0.001, 36, allow=False).predict


def test_larger_shift_change_predicts_the_dh_bracket_only(pred):
    pred.set(36, err=0.05, err_d=0.002, dpx=0.002)
    s = pred.plan(0.0, -0.3, 36)
    assert not s.predict and s.predict_d and s.h == 1.0 and s.hd == min(1.0, 2.0 * (0.002 * (0.3 / 0.002)) + 0.15) * 0.01
    s = pred.plan(0.5, -0.4, 36)   # 0.64 px
    assert not s.predict and not s.predict_d
    pred.set(36, err=0.05, err_d=0.05, dpx=0.002)
    s = pred.plan(0.0, -0.3, 36)   # (the median of dh is expected 7.5 half widths off)
    assert not s.predict and not s.predict_d


def test_cooldown_holds_one_step_then_runs_out(pred):
    pred.set(36, cooldown=1)
    s = pred.plan(0.001, 0.0, 36, allow=False)   # (the rerun of a step does not count)
    assert not s.predict and not s.predict_d and pred.m.cooldown == 1
    s = pred.plan(0.001, 0.0, 36)
    assert not s.predict and not s.predict_d and pred.m.cooldown == 0
    assert pred.plan(0.001, 0.0, 36).predict


def test_other_bin_count_and_too_many_bins(pred):
    pred.set(36)
    s = pred.plan(0.001, 0.0, 72)
    assert not s.predict and not s.predict_d
    pred.set(129)
    s = pred.plan(0.001, 0.0, 129)
    assert not s.predict and s.predict_d
    pred.set(128)
    assert pred.plan(0.001, 0.0, 128).predict


def test_bin_without_a_median_gets_the_empty_bracket(lib, pred):
    ok = np.ones(36, np.uint8)
    ok[[3, 35]] = 0
    pred.set(36, ok=ok)
    flags, sc, lo, hi = np.zeros(2, np.int32), np.zeros(3), np.zeros(256), np.zeros(256)
    lib.nkp_pred_plan(pred.p, 0.001, -0.0005, 36, 1, 1, flags.ctypes.data, sc.ctypes.data, lo.ctypes.data, hi.ctypes.data)
    assert flags[0] == 1
    assert (lo[3], hi[3]) == (1.0, 0.0) and (lo[35], hi[35]) == (1.0, 0.0)
    assert np.all(lo[:36][ok == 1] < hi[:36][ok == 1])


def step_results(m, nb, dE, dN, seed=1):
    """What a step some (dE, dN) further returns: the previous medians moved as the model says, up to a hundredth; brackets around them."""
    rng = np.random.default_rng(seed)
    mid = (np.arange(nb) + 0.5) * (2 * np.pi / nb)
    before = f64(m.med) if m.have else 1.5 + np.cos(0.7 - mid)
    med = before - (dE * np.sin(mid) + dN * np.cos(mid)) + rng.uniform(0.005, 0.01, nb)
    counts = np.full(nb, 5000, np.int64)
    edges = np.arange(nb + 1) * (2 * np.pi / nb)
    half = rng.uniform(0.02, 0.05, nb)
    return med, counts, edges, med - half, med + half


def test_record_after_a_predicted_step_keeps_the_sampled_widths(pred):
    pred.set(36)
    w0, wd0 = list(pred.m.w), pred.m.wd
    assert pred.plan(0.001, 0.0005, 36).predict
    med, counts, edges, lo, hi = step_results(pred.m, 36, 0.001, 0.0005)
    pred.record(0.251, -0.5005, 36, 1.7501, med, counts, edges, lo, hi, 1.74, 1.76, 16 + 5)
    m = pred.m
    assert m.w == w0 and m.wd == wd0 and m.n_predicted == 1 and m.n_predicted_d == 0
    assert 0 < m.err < 1 and m.dpx == math.sqrt(0.001 * 0.001 + 0.0005 * 0.0005) and (m.sx, m.sy, m.v) == (0.251, -0.5005, 1.7501)
    # the bracket of the median of dh predicted alone: the bins' widths are those of this step's samples, that one's is kept
    pred.set(36, err_d=0.002)
    assert pred.plan(0.0, -0.3, 36).predict_d
    pred.record(0.25, -0.2, 36, 1.7501, med, counts, edges, lo, hi, 1.74, 1.76, 0)
    assert pred.m.w == list(0.5 * (f64(hi) - f64(lo))) and pred.m.wd == 0.01 and pred.m.n_predicted_d == 1


def test_record_scales_the_widths_of_sixteenth_brackets(pred):
    s = pred.plan(0.25, 0.5, 36)   # the first step of a plan
    assert not s.predict and not s.predict_d
    med, counts, edges, lo, hi = step_results(pred.m, 36, 0.0, 0.0)
    counts[7] = 0
    med[7] = np.nan
    lo[9], hi[9] = hi[9], lo[9]   # (a bracket whose ends crossed)
    pred.record(0.25, -0.5, 36, 1.75, med, counts, edges, lo, hi, 1.74, 1.76, 16 + 5)
    m = pred.m
    scale = 0.5 / (5 / 16)
    assert scale == 1.6
    for b in (0, 1, 35):
        assert m.w[b] == scale * 0.5 * (hi[b] - lo[b]) and m.ok[b] == 1
    assert m.wd == scale * 0.5 * (1.76 - 1.74)
    assert m.w[7] == 0.0 and m.ok[7] == 0 and m.w[9] == 0.0 and m.ok[9] == 0
    assert m.have and (m.err, m.err_d, m.dpx) == (1e30, 1e30, 1e30)   # (nothing to measure a first step against)
    # codes 1 and 2 -- a half, a quarter -- are not rescaled
    s = pred.plan(0.0, 0.0, 36)
    pred.record(0.25, -0.5, 36, 1.75, med, counts, edges, lo, hi, 1.74, 1.76, 2)
    assert pred.m.w[0] == 0.5 * (hi[0] - lo[0]) and pred.m.dpx == 1e-5   # (a repeated step: the floor of the shift change)


def test_miss_and_forget(pred):
    pred.set(36)
    assert pred.plan(0.001, 0.0, 36).predict
    pred.lib.nkp_pred_on_miss(pred.p)
    pred.m.on_miss()
    pred.check()
    assert pred.m.cooldown == 1 and pred.m.err == 1e30 and pred.m.n_predict_miss == 1
    s = pred.plan(0.001, 0.0, 36, allow=False)   # the rerun
    assert not s.predict and not s.predict_d and pred.m.cooldown == 1


# ---- sizes of the device blocks ----------------------------------------------------------------------------------------------
def test_block_sizes_are_those_of_the_hand_written_formulas(lib):
    stride, hdr, buckets, cap = 16, 4, 4096, 8192
    for nbm in (1, 72, 128):
        zeroed = 24 + (11 + stride) * nbm + hdr + buckets // 2
        assert lib.nkp_fz_zeroed_words(nbm) == zeroed
        assert lib.nkp_fz_total_bytes(nbm) == zeroed * 8 + cap * 8
        assert lib.nkp_mr_small_words(nbm) == (11 + stride) * nbm
        off = np.zeros(8, np.int64)
        lib.nkp_fz_offsets(nbm, off.ctypes.data)
        assert list(off) == [24, 24 + nbm, 24 + 3 * nbm, 24 + 6 * nbm, 24 + 8 * nbm, 24 + 11 * nbm, 24 + (11 + stride) * nbm, zeroed]


def test_packed_result_block_is_the_sum_of_its_items(lib):
    def a16(n):
        return (n + 15) // 16 * 16

    for f64, es in ((0, 4), (1, 8)):
        ks, state = es, 40   # key of the sample type; a selection state: the key (padded to 8) + four 64-bit counters
        for nb in (1, 72, 128):
            items = [8 * 3 * nb, ks * nb, 16 * 8, 8, 32, 5 * 8, es, es * (nb + 1), state * nb, 8 * nb, ks * nb, ks, ks, 8 * 3 * nb]
            assert lib.nkp_fetch_bytes(f64, nb) == sum(a16(b) for b in items)
            assert lib.nkp_fetch_bytes(f64, nb) <= nb * (8 * 3 + 8 + 16 + 64 + 8 + 8 * 3 + 16) + 1024   # (what plans used to allocate)
    assert lib.nkp_fetch_bytes(0, 128) == 14112 and lib.nkp_fetch_bytes(1, 128) == 15648
