"""CPD on the GPU (csrc/cpd.hip, xdem_amd/cpd.py): the E-step over all pairs against a dense longdouble evaluation
(tests/cpd_oracle.py) within a derived bound and repeatable to the byte, under every cut into launches; the clouds' standardisation
against the oracle's bits; single steps from every recorded input of the reference's runs (tests/golden/cpd_golden_*.npz,
tools/gen_golden_cpd.py) and whole fits, alone, in a pipeline and through ``DEM.coregister_3d``; the edge cases.

THE BOUND of a term of the E-step (``bound``).  P1_m = sum_n p_mn inv_n, PX_m = sum_n p_mn inv_n x_n and den_n = sum_m p_mn (behind
Pt1_n) are sums of K products of exponentials, p = exp(-a), a = ((dx dx + dy dy) + dz dz) / (2 sigma2).  In units of 2^-52 and
relative to sum |term|:
  * K    recursive summation of K terms in any order (a lane's slice, the slices, whatever the order: at most K - 1 additions touch a
         term, half a unit each, doubled for second-order terms);
  * 3 a  the exponent is rounded before it is exponentiated: each difference 1/2, each square 1/2 more on twice that (3/2), the two
         additions 1/2 each (5/2), the division 1/2: 3 units relative on a, which exp turns into 3 a relative on p; a is at most
         a_max, the largest exponent among the terms that do not underflow to zero, and never above 745;
  * 16   exp itself (the device library's, within 2), the product with inv_n and with x_n, the division and the additions behind
         inv_n = 1 / (max(den_n, 2^-52) + c), c (a power and four operations, scaled by c / (den + c) <= 1).
inv_n also carries the error of its own sum den_n, in the worst case another (M + 3 a_max); the asserted bound leaves that out on
purpose -- it is the tighter one, recursive sums of positive terms err far below their worst case, and every measured figure is printed."""
import functools
import os

import numpy as np
import pytest

import cpd_oracle
import icp_oracle
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
RUNS = ("rigid", "tight", "weight", "trans", "nostd")
SCALE_REF, SCALE_TBA = np.array([[5.0], [3.0], [0.5]]), np.array([[6.0], [4.0], [0.7]])


@functools.lru_cache(maxsize=None)
def golden(case):
    return dict(np.load(os.path.join(GOLDEN, f"cpd_golden_{case}.npz")))


def unpack(bits, shape):
    return np.unpackbits(bits)[: int(np.prod(shape))].reshape(shape).astype(bool)


def rasters(case):
    g = golden(case)
    return g["ref"], g["tba"], unpack(g["inlier"], g["ref"].shape), tuple(g["transform"])


def settings(g, run):
    weight, only_t, scale_std, tol = g[f"{run}_settings"]
    return float(weight), bool(only_t), bool(scale_std), float(tol)


@functools.lru_cache(maxsize=None)
def oracle_clouds(case, scale_std=True, flip=False):
    """(ref_epc, tba_epc, centroid, std_fac, inlier): the reference's clouds bit for bit (the generator asserts it); ``flip`` masks
    one more pixel (the other parity of the count)."""
    ref, tba, inlier, t6 = rasters(case)
    if flip:
        rows, cols = np.nonzero(icp_oracle.valid_mask(ref, tba, inlier))
        inlier = inlier.copy()
        inlier[rows[0], cols[0]] = False
    r, t, _ = icp_oracle.clouds(ref, tba, icp_oracle.valid_mask(ref, tba, inlier), t6)
    r, t, cen, fac = icp_oracle.standardize(r, t, scale_std)
    r.setflags(write=False)
    t.setflags(write=False)
    return r, t, cen, fac, inlier


def bound(k, a_max, magnitude):
    return (k + 3.0 * min(a_max, 745.0) + 16.0) * EPS * np.asarray(magnitude, dtype=np.float64)


def check_terms(got, want, n, m, a_max, label):
    """P1, PX (K = N terms each), Pt1 (K = M) and Np against ``want`` (values and magnitudes); prints the largest error / bound."""
    worst = {}
    for key, k, mag in (("P1", n, want["P1"]), ("PX", n, want["PX_abs"]), ("Pt1", m, want["Pt1"])):
        err, lim = np.abs(got[key] - np.asarray(want[key], dtype=np.float64)), bound(k, a_max, mag)
        worst[key] = float(np.max(err / np.maximum(lim, 1e-300)))
        assert np.all(np.isfinite(got[key])) and np.all(err <= lim), (label, key, worst[key])
    # Np adds the M values of P1, each a sum of N terms
    assert abs(got["Np"] - float(want["Np"])) <= bound(n + m, a_max, float(want["Np"])), (label, "Np")
    print(label, "a_max", round(a_max, 1), "error / bound", {k: round(v, 4) for k, v in worst.items()})


def check_expectation(ref, tba, matrix, sigma2, weight, label):
    from xdem_amd import coreg

    got = coreg.cpd_expectation(ref, tba, matrix, sigma2, weight)
    n, m = ref.shape[1], tba.shape[1]
    assert got["P1"].shape == (m,) and got["Pt1"].shape == (n,) and got["PX"].shape == (3, m)
    moved = tba if matrix is None else icp_oracle.apply(matrix, tba)   # (the device's order of the product: the same bits)
    if sigma2 is None:
        # The direct sum: every term (three rounded squares of rounded differences, two additions: 5/2 units) passes through at
        # most len + slices <= M + 1 additions over its slices, N over the reference points, 26 in the shuffles and trees, and the
        # division by 3 N M: (N + M + 32) units.
        first = cpd_oracle.estep_dense(ref, moved, None, weight)
        assert abs(got["sigma2"] - float(first["sigma2"])) <= (n + m + 32) * EPS * float(first["sigma2"]), (label, got["sigma2"], first["sigma2"])
    else:
        assert got["sigma2"] == sigma2
    want = cpd_oracle.estep_dense(ref, moved, got["sigma2"], weight)   # the terms at the variance the device used
    check_terms(got, want, n, m, want["a_max"], label)
    return got


# ---- the E-step on small clouds -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 257, 600])
@pytest.mark.parametrize("m", [1, 65, 300])
def test_expectation_small_clouds(n, m):
    from xdem_amd import coreg

    rng = np.random.default_rng(100 * n + m)
    ref, tba = rng.normal(size=(3, n)) * SCALE_REF, rng.normal(size=(3, m)) * SCALE_TBA
    m4 = coreg.matrix_from_translations_rotations(0.4, -0.3, 0.1, 2.0, -3.0, 5.0)
    for matrix in (None, m4):
        for sigma2 in (4.0, None):
            for weight in (0.0, 0.3):
                label = f"n={n} m={m} matrix={matrix is not None} sigma2={sigma2} w={weight}"
                a = check_expectation(ref, tba, matrix, sigma2, weight, label)
                if matrix is None:
                    b = coreg.cpd_expectation(ref, tba, matrix, sigma2, weight)
                    assert all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in a), label
                if weight == 0.0 and sigma2 is None:   # without the uniform component every reference point is fully explained
                    assert np.abs(a["Pt1"] - 1.0).max() <= 4 * EPS


def test_expectation_clip_path():
    """One reference point 1e3 extents from every moved point, weight 0: its den underflows to exactly 0, the clip keeps inv finite
    (2^52), so its Pt1 is exactly 0 and it adds exactly 0 to every P1 and PX; the others are within the bound."""
    rng = np.random.default_rng(21)
    ref, tba = rng.normal(size=(3, 65)) * SCALE_REF, rng.normal(size=(3, 70)) * SCALE_TBA
    ref[:, 17] = (5.0e3, -3.0e3, 0.5e3)
    got = check_expectation(ref, tba, None, 4.0, 0.0, "clip")
    assert got["Pt1"][17] == 0.0 and np.all(np.delete(got["Pt1"], 17) > 0.5)
    assert all(np.all(np.isfinite(got[k])) for k in ("P1", "Pt1", "PX")) and np.isfinite(got["Np"])
    want = cpd_oracle.estep_dense(np.delete(ref, 17, axis=1), tba, 4.0, 0.0)   # the other points do not see it
    check_terms({"P1": got["P1"], "PX": got["PX"], "Pt1": np.delete(got["Pt1"], 17), "Np": got["Np"]}, want, 64, 70, want["a_max"], "clip, without the point")


def test_expectation_not_centred():
    """Both clouds offset by 1e6 on every axis: the start variance is summed pair by pair, so it stays within the direct sum's bound
    (the closed form M sum|x|^2 + N sum|ty|^2 - 2 sum x . sum ty would keep no digit: 1e12-sized squares against a 50-sized result)."""
    rng = np.random.default_rng(22)
    ref, tba = rng.normal(size=(3, 257)) * SCALE_REF + 1.0e6, rng.normal(size=(3, 300)) * SCALE_TBA + 1.0e6
    got = check_expectation(ref, tba, None, None, 0.0, "offset 1e6")
    closed = (300 * np.sum(ref * ref) + 257 * np.sum(tba * tba) - 2 * np.sum(ref.sum(axis=1) * tba.sum(axis=1))) / (3 * 257 * 300)
    print("sigma2", got["sigma2"], "closed form in float64", closed)
    assert 10.0 < got["sigma2"] < 100.0


def test_slices_and_launches_return_the_same_bytes():
    """600 x 300 runs several slices per block; cut into launches of 1 and of 3 workgroups, then whole again: the bytes of the default."""
    from xdem_amd import _lib, coreg

    rng = np.random.default_rng(23)
    ref, tba = rng.normal(size=(3, 600)) * SCALE_REF, rng.normal(size=(3, 300)) * SCALE_TBA
    ctx = _lib.default_context()
    want = {s: coreg.cpd_expectation(ref, tba, None, s, 0.3) for s in (4.0, None)}
    try:
        for cap in (1, 3, 0):
            ctx.set_option("pairs_launch_cap", cap)
            for s, w in want.items():
                got = coreg.cpd_expectation(ref, tba, None, s, 0.3)
                assert all(np.asarray(got[k]).tobytes() == np.asarray(w[k]).tobytes() for k in w), (cap, s)
    finally:
        ctx.set_option("pairs_launch_cap", 0)


def test_more_than_two_to_the_32_pairs():
    """65 600 x 65 600 points: 4.3e9 pair evaluations per pass, more than one launch holds (2^32), so the default goes out as two
    launches over ranges of workgroups; as ONE launch (``pairs_launch_cap`` above the 2 056 workgroups) it returns the same bytes.
    ``Pt1_n = den_n / (den_n + c)`` of a few reference points -- the first, those around index 2^16, the last -- against their own sum
    over all moved points in longdouble, within ``bound`` (K = M)."""
    from xdem_amd import _lib, coreg

    n = m = 65_600
    rng = np.random.default_rng(24)
    ref, tba = rng.normal(size=(3, n)) * SCALE_REF, rng.normal(size=(3, m)) * SCALE_TBA
    ctx = _lib.default_context()
    got = coreg.cpd_expectation(ref, tba, None, 4.0, 0.3)
    try:
        ctx.set_option("pairs_launch_cap", 4096)
        one = coreg.cpd_expectation(ref, tba, None, 4.0, 0.3)
    finally:
        ctx.set_option("pairs_launch_cap", 0)
    assert all(np.asarray(got[k]).tobytes() == np.asarray(one[k]).tobytes() for k in got)
    assert np.all(np.isfinite(got["P1"])) and np.all(np.isfinite(got["PX"])) and 0.0 < got["Np"] < n
    L = np.longdouble
    c = (2 * L(np.pi) * L(4.0)) ** L(1.5) * L(0.3) / (1 - L(0.3)) * L(m) / L(n)
    for i in (0, 255, 256, 65_535, 65_536, 65_537, n - 1):
        d = ref[:, i].astype(L)[:, None] - tba.astype(L)
        a = ((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]) / L(8.0)
        den = np.exp(-a).sum()
        want = den / (max(den, L(EPS)) + c)
        assert abs(got["Pt1"][i] - float(want)) <= bound(m, float(a[a < 745.0].max()), float(want)), i


# ---- the clouds ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["f32", "f64"])
@pytest.mark.parametrize("flip", [False, True])
def test_clouds_centroid_and_std_fac_are_the_oracles_bits(case, flip):
    from xdem_amd import cpd
    from xdem_amd.biascorr import DhPlan

    ref, tba, _, t6 = rasters(case)
    r, t, cen, fac, inlier = oracle_clouds(case, True, flip)
    with DhPlan(ref, tba, inlier) as plan:
        with cpd.CpdCloud.from_plan(plan, t6) as cloud:
            assert cloud.n == cloud.m == r.shape[1] and cloud.centroid == cen and cloud.std_fac == fac
            # the clouds themselves: an E-step on them returns the bytes of the same E-step on the oracle's clouds
            sums, used = cloud.estep(None, None, 0.1)
            terms = cloud.terms()
        with cpd.CpdCloud.from_plan(plan, t6, standardize=False) as cloud:
            assert cloud.std_fac == 1.0 and cloud.centroid == cen
    with cpd.CpdCloud.from_points(r, t) as cloud:
        sums2, used2 = cloud.estep(None, None, 0.1)
        terms2 = cloud.terms()
    assert sums.tobytes() == sums2.tobytes() and used == used2 and all(a.tobytes() == b.tobytes() for a, b in zip(terms, terms2))


def test_counts_of_both_parities_are_covered():
    for case in ("f32", "f64"):
        assert {oracle_clouds(case, True, f)[0].shape[1] % 2 for f in (False, True)} == {0, 1}


# ---- single steps from the recorded inputs ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["f32", "f64"])
@pytest.mark.parametrize("run", RUNS)
def test_steps_from_the_recorded_inputs(case, run):
    """From every recorded input ``(matrix, sigma2)``, on the reference's own clouds: one ``estep`` + ``cpd_update`` lands on the
    recorded output within 10 x the run's ``perturb_gap`` (matrix elements absolute, sigma2 and q relative); ``P1`` / ``Pt1`` / ``PX`` of
    iterations 0, 1 and the last within ``bound``."""
    from xdem_amd import cpd, rigid

    g = golden(case)
    weight, only_t, scale_std, tol = settings(g, run)
    X, Y, _, fac, _ = oracle_clouds(case, scale_std)
    gm, gs, gq = 10 * g[f"{run}_perturb_gap"]
    full = set(int(i) for i in g[f"{run}_full_iterations"])
    n = X.shape[1]
    worst = np.zeros(3)
    with cpd.CpdCloud.from_points(X, Y) as cloud:
        for i, matrix_in in enumerate(g[f"{run}_matrix_in"]):
            s_in = g[f"{run}_sigma2_in"][i]
            inv = rigid.invert_matrix(matrix_in)
            sums, used = cloud.estep(inv, None if np.isnan(s_in) else float(s_in), weight)
            matrix, sigma2, q = cpd.cpd_update(sums, used, tol / fac / 10, only_t)
            want_m, want_s, want_q = g[f"{run}_matrix"][i], float(g[f"{run}_sigma2"][i]), float(g[f"{run}_q"][i])
            gaps = np.array([np.abs(matrix - want_m).max(), abs(sigma2 - want_s) / abs(want_s), abs(q - want_q) / abs(want_q)])
            worst = np.maximum(worst, gaps)
            assert gaps[0] <= gm and gaps[1] <= gs and gaps[2] <= gq, (case, run, i, gaps, (gm, gs, gq))
            if only_t:
                assert np.array_equal(matrix[:3, :3], np.eye(3))
            if i in full:
                p1, pt1, px = cloud.terms()
                moved = icp_oracle.apply(inv, Y)
                e = cpd_oracle.estep(X, moved, used, weight, magnitudes=True)
                want = {"P1": g[f"{run}_it{i}_P1"], "Pt1": g[f"{run}_it{i}_Pt1"], "PX": g[f"{run}_it{i}_PX"], "PX_abs": e["PX_abs"],
                        "Np": g[f"{run}_it{i}_P1"].sum()}
                check_terms({"P1": p1, "Pt1": pt1, "PX": px, "Np": float(sums[0])}, want, n, n, cpd_oracle.largest_exponent(X, moved, used),
                            f"{case} {run} iteration {i}")
    print(case, run, "largest gaps (matrix, sigma2, q)", worst, "bounds", (gm, gs, gq))


# ---- whole fits ---------------------------------------------------------------------------------------------------------------------------
def _fit(case, run, **kw):
    from xdem_amd import coreg

    g = golden(case)
    weight, only_t, scale_std, tol = settings(g, run)
    ref, tba, inlier, t6 = rasters(case)
    args = dict(weight=weight, only_translation=only_t, standardize=scale_std, tolerance=tol, subsample=1)
    args.update(kw)
    return coreg.CPD(**args).fit(ref, tba, inlier, transform=t6)


@pytest.mark.parametrize("case", ["f32", "f64"])
@pytest.mark.parametrize("run", RUNS)
def test_whole_fits_land_on_the_reference(case, run):
    """The fit stops at the recorded iteration and ends within 10 x the run's ``perturb_gap`` of the recorded final matrix (the
    translation de-standardised: x std_fac); each dtype has its own fixture and gap.  Two fits return the same bytes."""
    g = golden(case)
    c, again = _fit(case, run), _fit(case, run)
    got, want = c.to_matrix(), g[f"{run}_final"]
    fac, gm = float(g[f"{run}_std_fac"]), 10 * float(g[f"{run}_perturb_gap"][0])
    out = c.meta["outputs"]
    gap_r, gap_t = float(np.abs(got[:3, :3] - want[:3, :3]).max()), float(np.abs(got[:3, 3] - want[:3, 3]).max())
    print(case, run, "iterations", out["iterative"]["last_iteration"], "recorded", len(g[f"{run}_stat"]), "rotation gap", gap_r, "bound", gm,
          "translation gap", gap_t, "bound", gm * fac)
    assert out["iterative"]["last_iteration"] == len(g[f"{run}_stat"])
    assert gap_r <= gm and gap_t <= gm * fac and np.array_equal(got[3], [0, 0, 0, 1])
    assert c.centroid() == tuple(g[f"{run}_centroid"]) and out["random"]["subsample_final"] == int(g["subsample_final"])
    assert out["affine"]["shift_x"] == got[0, 3] and out["affine"]["shift_y"] == got[1, 3] and out["affine"]["shift_z"] == got[2, 3]
    it = out["iterative"]
    assert it["last_iteration"] == len(it["matrices"]) == len(it["statistics"]) == len(it["sigma2"]) == len(it["q"])
    assert it["last_tolerance"] == it["statistics"][-1] and np.isinf(it["statistics"][0])
    gs, gq = 10 * float(g[f"{run}_perturb_gap"][1]), 10 * float(g[f"{run}_perturb_gap"][2])
    assert np.all(np.abs(np.array(it["sigma2"]) - g[f"{run}_sigma2"]) <= gs * np.abs(g[f"{run}_sigma2"]))
    assert np.all(np.abs(np.array(it["q"]) - g[f"{run}_q"]) <= gq * np.abs(g[f"{run}_q"]))
    assert np.abs(np.array(it["matrices"]) - g[f"{run}_matrix"]).max() <= gm
    if settings(g, run)[1]:
        assert np.array_equal(got[:3, :3], np.eye(3)) and c.to_rotations() == (0.0, 0.0, 0.0)
    assert again.to_matrix().tobytes() == got.tobytes()
    assert np.array(again.meta["outputs"]["iterative"]["q"]).tobytes() == np.array(it["q"]).tobytes()


# ---- integration ------------------------------------------------------------------------------------------------------------------------
def test_pipeline_coregister_3d_and_apply():
    from xdem_amd import coreg
    from xdem_amd.dem import DEM

    ref, tba, inlier, t6 = rasters("f32")
    c = coreg.CPD(subsample=1).fit(ref, tba, inlier, transform=t6)
    out, t = c.apply(tba, transform=t6)
    want, _ = coreg.apply_matrix(tba, c.to_matrix(), centroid=c.centroid(), transform=t6)
    assert t == t6 and out.dtype == tba.dtype and np.array_equal(out, want, equal_nan=True) and np.isfinite(out).any()
    pipe = coreg.NuthKaab(subsample=1) + coreg.CPD(subsample=1)
    piped, t = pipe.fit_and_apply(ref, tba, inlier, transform=t6)
    assert t == t6 and pipe.is_affine and np.isfinite(piped).any() and np.all(np.isfinite(pipe.to_matrix()))
    assert np.array_equal(pipe.to_matrix(), pipe.pipeline[1].to_matrix() @ pipe.pipeline[0].to_matrix())
    aligned = DEM(tba, t6).coregister_3d(DEM(ref, t6), coreg.CPD(subsample=1), inlier_mask=inlier)
    assert aligned.transform == t6 and aligned.data.dtype == np.float32 and np.array_equal(aligned.data, out, equal_nan=True)


def test_default_subsample_on_a_larger_pair():
    """``CPD()`` as it comes -- 5 000 points, 100 iterations at most -- on a 96 x 128 pair: a finite result, nothing more."""
    from xdem_amd import coreg

    rows, cols = np.mgrid[0:96, 0:128]
    x, y = 10.0 * cols, 10.0 * rows
    ref = (800.0 + 120.0 * np.sin(x / 90.0) * np.cos(y / 70.0) + 40.0 * np.sin((x + y) / 50.0)).astype(np.float32)
    tba = (ref + 1.5 + 0.002 * x + np.random.default_rng(24).normal(scale=0.02, size=ref.shape)).astype(np.float32)
    c = coreg.CPD().fit(ref, tba, transform=(10.0, 0.0, 0.0, 0.0, -10.0, 960.0), random_state=42)
    out = c.meta["outputs"]
    assert out["random"]["subsample_final"] == 5000 and 3 <= out["iterative"]["last_iteration"] <= 100
    assert np.all(np.isfinite(c.to_matrix())) and np.all(np.isfinite(out["iterative"]["q"][1:]))


# ---- edge cases -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_iterations", [1, 3])
def test_few_iterations_follow_the_oracle(max_iterations):
    """Stopped by ``max_iterations`` (the stop rule never fires before the third iteration): the oracle's matrix within 10 x the
    ``rigid`` run's gap, whose first iterations these are."""
    g = golden("f64")
    c = _fit("f64", "rigid", max_iterations=max_iterations)
    ref, tba, inlier, t6 = rasters("f64")
    want, cen, n, trail = cpd_oracle.cpd(ref, tba, inlier, t6, max_iterations=max_iterations)
    fac, gm = float(g["rigid_std_fac"]), 10 * float(g["rigid_perturb_gap"][0])
    got = c.to_matrix()
    assert c.meta["outputs"]["iterative"]["last_iteration"] == len(trail) == max_iterations and c.centroid() == cen
    assert np.abs(got[:3, :3] - want[:3, :3]).max() <= gm and np.abs(got[:3, 3] - want[:3, 3]).max() <= gm * fac
    assert np.abs(np.array(c.meta["outputs"]["iterative"]["matrices"]) - g["rigid_matrix"][:max_iterations]).max() <= gm


# Four points, or one: every sum has at most four terms and the oracle's run ends on an exact fixed point (its last statistic is 0.0)
# after six, or three, iterations.  A few hundred roundings of numbers no larger than 10 (metres, or standardised units):
SMALL_BOUND = 1000 * EPS * 10.0


@pytest.mark.parametrize("standardize", [True, False])
def test_two_by_two_raster(standardize):
    from xdem_amd import coreg

    t6 = (10.0, 0.0, 100.0, 0.0, -10.0, 200.0)
    ref = np.array([[100.0, 101.5], [99.0, 102.0]])
    tba = ref + 0.75
    want, cen, n, trail = cpd_oracle.cpd(ref, tba, None, t6, scale_std=standardize)
    assert trail[-1]["stat"] == 0.0 and n == 4
    c = coreg.CPD(standardize=standardize, subsample=1).fit(ref, tba, transform=t6)
    assert c.meta["outputs"]["iterative"]["last_iteration"] == len(trail) and c.centroid() == cen
    assert c.meta["outputs"]["random"]["subsample_final"] == 4
    assert np.abs(c.to_matrix() - want).max() <= SMALL_BOUND, np.abs(c.to_matrix() - want).max()


def test_single_valid_pixel():
    """One valid pixel: A = 0, the SVD of zeros gives R = I, the variance falls to sigma2_min and the fit ends on the vertical
    difference -- the oracle's host lines, the same matrix.  With ``standardize`` the factor (a NMAD of one value) is 0: upstream
    divides by it; the cloud front refuses, as it does for ICP."""
    from xdem_amd import _lib, coreg

    t6 = (10.0, 0.0, 100.0, 0.0, -10.0, 200.0)
    ref = np.full((2, 2), np.nan)
    ref[1, 0] = 5.0
    tba = ref + 0.75
    want, cen, n, trail = cpd_oracle.cpd(ref, tba, None, t6, scale_std=False)
    assert n == 1 and np.all(np.isfinite(want))
    c = coreg.CPD(standardize=False, subsample=1).fit(ref, tba, transform=t6)
    assert c.meta["outputs"]["iterative"]["last_iteration"] == len(trail) and c.centroid() == cen
    assert np.abs(c.to_matrix() - want).max() <= SMALL_BOUND and c.meta["outputs"]["random"]["subsample_final"] == 1
    with pytest.raises(_lib.XdemHipError, match="standardisation factor"):
        coreg.CPD(subsample=1).fit(ref, tba, transform=t6)
