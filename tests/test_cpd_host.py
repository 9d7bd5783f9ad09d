"""Host-side contract of ``xdem_amd.coreg.CPD`` / ``cpd_update`` and the CPU oracle tests/cpd_oracle.py (no GPU), against what
tools/gen_golden_cpd.py recorded from the reference's own functions (tests/golden/cpd_golden_f32.npz, cpd_golden_f64.npz,
signatures_cpd.json): signatures and constructor meta, the errors raised before a device is asked for, the M-step on the host, and
the oracle driven over every recorded run.

Tolerances are the fixture's: ``<run>_perturb_gap`` holds the largest deviation from the reference's trajectory -- matrix elements
(absolute), sigma2 (relative), q (relative) -- that the generator saw when it ran the oracle with three chunk lengths (three summation
orders) and with every exponential perturbed by +-2 * 2^-52.  Everything here is held within 10 x that gap."""
import functools
import inspect
import json
import os

import numpy as np
import pytest

import cpd_oracle
import icp_oracle
from conftest import GOLDEN

SIG = json.load(open(os.path.join(GOLDEN, "signatures_cpd.json")))["coreg"]
RUNS = ("rigid", "tight", "weight", "trans", "nostd")


@functools.lru_cache(maxsize=None)
def golden(case):
    return dict(np.load(os.path.join(GOLDEN, f"cpd_golden_{case}.npz")))


def unpack(bits, shape):
    return np.unpackbits(bits)[: int(np.prod(shape))].reshape(shape).astype(bool)


def settings(g, run):
    weight, only_t, scale_std, tol = g[f"{run}_settings"]
    return float(weight), bool(only_t), bool(scale_std), float(tol)


@functools.lru_cache(maxsize=None)
def case_clouds(case, scale_std):
    """(ref_epc, tba_epc, centroid, std_fac) of a recorded pair, rebuilt by the oracle from the rasters and the inlier bits."""
    g = golden(case)
    ref, tba, t6 = g["ref"], g["tba"], tuple(g["transform"])
    mask = icp_oracle.valid_mask(ref, tba, unpack(g["inlier"], ref.shape))
    r, t, _ = icp_oracle.clouds(ref, tba, mask, t6)
    r, t, cen, fac = icp_oracle.standardize(r, t, scale_std)
    r.setflags(write=False)
    t.setflags(write=False)
    return r, t, cen, fac


def within(g, run, got, i):
    """(matrix, sigma2, q) against the recorded output of iteration i, within 10 x the run's perturb_gap."""
    gm, gs, gq = 10 * g[f"{run}_perturb_gap"]
    matrix, sigma2, q = got
    want_m, want_s, want_q = g[f"{run}_matrix"][i], float(g[f"{run}_sigma2"][i]), float(g[f"{run}_q"][i])
    assert np.abs(matrix - want_m).max() <= gm, (run, i, np.abs(matrix - want_m).max(), gm)
    assert abs(sigma2 - want_s) <= gs * abs(want_s), (run, i, abs(sigma2 - want_s) / abs(want_s), gs)
    assert abs(q - want_q) <= gq * abs(want_q), (run, i, abs(q - want_q) / abs(want_q), gq)


# ---- signatures, meta, errors ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SIG))
def test_reference_parameters_are_mirrored(name):
    from xdem_amd import coreg

    obj = coreg
    for part in name.split("."):
        obj = getattr(obj, part)
    mine = list(inspect.signature(obj).parameters.items())
    names = [n for n, _ in mine]
    pos = -1
    for rec in SIG[name]:
        if rec["kind"] in ("VAR_KEYWORD", "VAR_POSITIONAL"):
            continue
        assert rec["name"] in names, f"{name}: parameter '{rec['name']}' of the reference is missing"
        p = dict(mine)[rec["name"]]
        assert names.index(rec["name"]) > pos, f"{name}: '{rec['name']}' is out of the reference's order"
        pos = names.index(rec["name"])
        if rec["default"] == "<required>":
            assert p.default is inspect.Parameter.empty, f"{name}: '{rec['name']}' must stay required"
        elif rec["default"] == "<object>":
            assert p.default is not inspect.Parameter.empty
        else:
            assert p.default == rec["default"], f"{name}: default of '{rec['name']}' is {p.default!r}, reference {rec['default']!r}"


def test_constructor_meta_and_defaults():
    from xdem_amd import coreg, cpd

    c = coreg.CPD()
    assert c.meta["inputs"]["specific"] == {"cpd_weight": 0}
    assert c.meta["inputs"]["affine"] == {"only_translation": False, "standardize": True}
    assert c.meta["inputs"]["iterative"] == {"max_iterations": 100, "tolerance": 0.01}
    assert c.meta["inputs"]["random"] == {"subsample": 5e3, "random_state": None}
    assert set(c.meta["inputs"]) == {"specific", "affine", "iterative", "random"} and c.meta["outputs"] == {}
    assert c.is_affine and c.centroid() is None and c._needs_transform and not c._needs_vars
    assert isinstance(coreg.NuthKaab() + c, coreg.CoregPipeline)
    assert coreg.CPD is cpd.CPD and coreg.cpd_expectation is cpd.cpd_expectation
    d = coreg.CPD(weight=0.3, only_translation=True, max_iterations=7, tolerance=1e-4, standardize=False, subsample=123)
    assert d.meta["inputs"]["specific"]["cpd_weight"] == 0.3 and d.meta["inputs"]["affine"] == {"only_translation": True, "standardize": False}
    assert d.meta["inputs"]["iterative"] == {"max_iterations": 7, "tolerance": 1e-4} and d.meta["inputs"]["random"]["subsample"] == 123


def test_errors_without_a_device():
    from xdem_amd import coreg

    dem = np.zeros((8, 9), dtype=np.float32)
    with pytest.raises(NotImplementedError, match="initial_shift"):
        coreg.CPD(initial_shift=(1, 2))
    for bad in (1, 1.0, -0.1, 2.5, float("nan")):
        with pytest.raises(ValueError, match=r"CPD weight must be in \[0, 1\)"):
            coreg.CPD(weight=bad)
        with pytest.raises(ValueError, match=r"CPD weight must be in \[0, 1\)"):
            coreg.cpd_expectation(np.zeros((3, 2)), np.zeros((3, 2)), weight=bad)
    with pytest.raises(NotImplementedError, match="Weights have not yet been implemented"):
        coreg.CPD().fit(dem, dem, weights=dem, resolution=1.0)
    with pytest.raises(NotImplementedError, match="bias_vars"):
        coreg.CPD().fit(dem, dem, bias_vars={"a": dem}, resolution=1.0)

    class Cloud:
        geometry = None

    with pytest.raises(NotImplementedError, match="point-cloud inputs are not supported"):
        coreg.CPD().fit(Cloud(), dem, resolution=1.0)
    with pytest.raises(NotImplementedError, match="point-cloud inputs are not supported"):
        coreg.CPD().fit(dem, Cloud(), resolution=1.0)
    with pytest.raises(AssertionError, match="fit"):
        coreg.CPD().apply(dem, resolution=1.0)


# ---- the M-step on the host -----------------------------------------------------------------------------------------------------------
def _sums(Np, muX, muY, A, xPx, YPY):
    return np.concatenate(([Np], muX, muY, np.asarray(A, dtype=np.float64).ravel(), [xPx, YPY]))


def test_cpd_update_branches_on_hand_made_sums():
    from xdem_amd import cpd

    muX, muY = np.array([1.0, 2.0, 3.0]), np.array([0.5, -1.0, 0.25])
    # A = I: U = V = I, R = I, tr(A R) = 3; xPx = 1 -> sigma2' = (1 - 3) / 6 < 0 -> sigma2_min
    matrix, sigma2, q = cpd.cpd_update(_sums(2.0, muX, muY, np.eye(3), 1.0, 4.0), 0.5, 1e-3)
    assert np.array_equal(matrix[:3, :3], np.eye(3)) and np.array_equal(matrix[:3, 3], -(muX - muY)) and np.array_equal(matrix[3], [0, 0, 0, 1])
    assert sigma2 == 1e-3
    assert q == (1.0 - 2 * 3.0 + 4.0) / (2 * 0.5) + 3 * 2.0 / 2 * np.log(0.5)
    # a positive variance is kept: xPx = 9 -> (9 - 3) / 6 = 1
    assert cpd.cpd_update(_sums(2.0, muX, muY, np.eye(3), 9.0, 4.0), 0.5, 1e-3)[1] == 1.0
    # a rotation about z by 90 degrees: A = R0^T maximises tr(A R) at R = R0
    R0 = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    matrix, _, _ = cpd.cpd_update(_sums(1.0, muX, muY, R0.T, 9.0, 4.0), 0.5, 1e-3)
    assert np.abs(matrix[:3, :3] - R0).max() <= 4 * 2.0 ** -52 and np.abs(matrix[:3, 3] + (muX - R0.T @ muY)).max() <= 8 * 2.0 ** -52
    # a reflection is refused: A = diag(1, 1, -1) gives det(U V) = -1 and a proper rotation
    matrix, _, _ = cpd.cpd_update(_sums(1.0, muX, muY, np.diag([1.0, 1.0, -1.0]), 9.0, 4.0), 0.5, 1e-3)
    assert abs(np.linalg.det(matrix[:3, :3]) - 1.0) <= 4 * 2.0 ** -52
    # only_translation: R = I whatever A is, tr(A R) = tr(A)
    A = np.array([[0.0, -2.0, 0.0], [2.0, 0.0, 0.0], [0.0, 0.0, 0.5]])
    matrix, sigma2, q = cpd.cpd_update(_sums(2.0, muX, muY, A, 9.0, 4.0), 0.5, 1e-3, only_translation=True)
    assert np.array_equal(matrix[:3, :3], np.eye(3)) and np.array_equal(matrix[:3, 3], -(muX - muY))
    assert sigma2 == (9.0 - 0.5) / 6.0 and q == (9.0 - 2 * 0.5 + 4.0) / (2 * 0.5) + 3 * 2.0 / 2 * np.log(0.5)


def test_cpd_update_svd_error_message(monkeypatch):
    from xdem_amd import cpd

    def fail(*a, **k):
        raise np.linalg.LinAlgError("SVD did not converge")

    monkeypatch.setattr(np.linalg, "svd", fail)
    s = _sums(1.0, np.zeros(3), np.zeros(3), np.eye(3), 1.0, 1.0)
    with pytest.raises(ValueError, match=r"CPD coregistration numerics during np.linalg.svd\(\), try setting standardize=True."):
        cpd.cpd_update(s, 0.5, 1e-3)
    cpd.cpd_update(s, 0.5, 1e-3, only_translation=True)   # (no SVD on that branch)


@pytest.mark.parametrize("case", ["f32", "f64"])
@pytest.mark.parametrize("run", RUNS)
def test_cpd_update_on_oracle_sums_gives_the_recorded_step(case, run):
    """``cpd_update`` on the sums the oracle forms from a recorded input lands on the recorded output (iterations 0, 1, the last),
    and the E-step's vectors on the recorded ``P1`` / ``Pt1`` / ``PX`` within the same relative gap as sigma2."""
    from xdem_amd import cpd, rigid

    g = golden(case)
    weight, only_t, scale_std, tol = settings(g, run)
    X, Y, _, fac = case_clouds(case, scale_std)
    for i in (int(v) for v in g[f"{run}_full_iterations"]):
        s_in = g[f"{run}_sigma2_in"][i]
        TY = icp_oracle.apply(rigid.invert_matrix(g[f"{run}_matrix_in"][i]), Y)
        e = cpd_oracle.estep(X, TY, None if np.isnan(s_in) else float(s_in), weight)
        within(g, run, cpd.cpd_update(cpd_oracle.sums(X, Y, e), e["sigma2"], tol / fac / 10, only_t), i)
        rel = 10 * float(g[f"{run}_perturb_gap"][1])
        for k in ("P1", "Pt1"):
            want = g[f"{run}_it{i}_{k}"]
            assert np.all(np.abs(e[k] - want) <= rel * np.abs(want)), (run, i, k)
        want = g[f"{run}_it{i}_PX"]
        assert np.all(np.abs(e["PX"] - want) <= rel * np.abs(want).max(axis=0)), (run, i, "PX")


# ---- the oracle against the reference's recorded runs -------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["f32", "f64"])
@pytest.mark.parametrize("run", RUNS)
def test_oracle_follows_the_reference(case, run):
    from xdem_amd import rigid

    g = golden(case)
    weight, only_t, scale_std, tol = settings(g, run)
    X, Y, cen, fac = case_clouds(case, scale_std)
    assert cen == tuple(g[f"{run}_centroid"]) and fac == float(g[f"{run}_std_fac"]) and X.shape[1] == int(g["subsample_final"])
    n_it = len(g[f"{run}_stat"])
    final, trail = cpd_oracle.drive(X, Y, weight, only_t, tol / fac, 100)
    assert len(trail) == n_it
    for i, t in enumerate(trail):
        within(g, run, (t["matrix"], t["sigma2"], t["q"]), i)
        if i + 1 < n_it:   # the recorded driver went on from its own output
            assert np.array_equal(g[f"{run}_matrix"][i], g[f"{run}_matrix_in"][i + 1]) and g[f"{run}_sigma2"][i] == g[f"{run}_sigma2_in"][i + 1]
    # the recorded run stopped by upstream's rule, with a margin on every decision
    stats, stop = g[f"{run}_stat"], tol / fac
    assert 3 < n_it < 100 and stats[-1] < stop and all(s >= stop for s in stats[2:-1]) and np.all(np.abs(stats - stop) > 1e-6 * stop)
    assert np.isnan(g[f"{run}_sigma2_in"][0]) and np.array_equal(g[f"{run}_matrix_in"][0], np.eye(4))
    out = rigid.invert_matrix(final)
    out[:3, 3] *= fac
    gm = 10 * float(g[f"{run}_perturb_gap"][0])
    assert np.abs(out[:3, :3] - g[f"{run}_final"][:3, :3]).max() <= gm and np.abs(out[:3, 3] - g[f"{run}_final"][:3, 3]).max() <= gm * fac


def test_fixture_is_not_trivial():
    """Four full blocks of 256 and a tail; runs of different lengths; an E-step whose rows differ."""
    for case in ("f32", "f64"):
        g = golden(case)
        n = int(g["subsample_final"])
        assert 4 * 256 < n < 5 * 256
        lengths = {run: len(g[f"{run}_stat"]) for run in RUNS}
        assert lengths["tight"] > lengths["rigid"] and len(set(lengths.values())) >= 4
        assert g["rigid_it0_P1"].shape == (n,) and g["rigid_it0_PX"].shape == (3, n) and g["rigid_it0_P1"].std() > 0
        assert np.all(g["rigid_perturb_gap"] < 1e-9) and np.all(g["nostd_perturb_gap"] < 1e-9)
        assert np.array_equal(g["trans_matrix"][:, :3, :3], np.broadcast_to(np.eye(3), (lengths["trans"], 3, 3)))
        assert np.all(g["weight_it0_Pt1"] < 1.0) and np.abs(g["rigid_it0_Pt1"] - 1.0).max() < 1e-12


# ---- the iteration loop ---------------------------------------------------------------------------------------------------------------
def test_iterate_through_iterate_method_returns_what_it_returned():
    """``rigid._iterate`` expressed through the general ``_iterate_method`` against the loop it was, on a scripted step function."""
    from xdem_amd import rigid

    def scripted(shifts):
        calls = []

        def step_matrix(matrix):
            calls.append(matrix.copy())
            t = shifts[len(calls) - 1]
            return rigid.matrix_from_translations_rotations(t, -0.5 * t, 0.25 * t, 0.1 * t, -0.2 * t, 0.3 * t)

        return step_matrix, calls

    def before(step_matrix, max_iterations, tolerance):   # (the loop as it stood)
        matrix, history = np.eye(4), []
        for i in range(int(max_iterations)):
            step = step_matrix(matrix)
            matrix = step @ matrix
            stat = float(np.sqrt(np.sum(step[:3, 3]) ** 2))
            history.append((matrix.copy(), stat))
            if i > 1 and stat < tolerance:
                break
        return matrix, history

    shifts = [4.0, 0.001, 2.0, 1.0, 0.5, 0.01, 3.0, 0.001]
    for max_it, tol in ((8, 0.1), (8, 1e-9), (1, 0.1), (3, 100.0), (2, 100.0), (0, 0.1), (5, 0.0075)):
        f0, c0 = scripted(shifts)
        f1, c1 = scripted(shifts)
        m0, h0 = before(f0, max_it, tol)
        m1, h1 = rigid._iterate(f1, max_it, tol)
        assert np.array_equal(m0, m1) and len(h0) == len(h1) == len(c0) == len(c1)
        for (a, sa), (b, sb), ca, cb in zip(h0, h1, c0, c1):
            assert np.array_equal(a, b) and sa == sb and isinstance(sb, float) and np.array_equal(ca, cb)
    # the general loop: any iterating input, the statistic compared as upstream compares it
    seen = []

    def method(inp):
        seen.append(inp)
        return (inp[0] + 1, inp[1] / 2), inp[1] / 2

    out, trail = rigid._iterate_method(method, (0, 8.0), 1.5, 10)
    assert out == (3, 1.0) and [s for _, s in trail] == [4.0, 2.0, 1.0] and seen == [(0, 8.0), (1, 4.0), (2, 2.0)]
    out, trail = rigid._iterate_method(method, (0, 0.5), 1.5, 10)   # never before the third iteration
    assert len(trail) == 3
