"""Host-side contract of ``xdem_amd.coreg.ICP`` / ``nearest`` and the CPU oracle tests/icp_oracle.py (no GPU), against what
tools/gen_golden_icp.py recorded from the reference's own functions (tests/golden/icp_golden.npz, signatures_icp.json): signatures and
constructor meta, the errors raised before a device is asked for, the host solves, and the oracle followed step by step from every
recorded input matrix -- ``ind`` and the kept pairs exactly, ``dists`` within 4 * 2^-52 relative (three rounded products and two sums),
the step matrix within 10 x the run's ``solve_gap``.

The fixture holds ``ind``, the kept flags and every sixteenth ``dists`` value in full for iterations 0, 1 and the last of each run, and
CRC-32 digests of ``ind`` and of the kept indexes for every iteration (a committed file may not exceed 1 MiB): exactness is checked
on all iterations through the digests, the distances where they are stored."""
import functools
import inspect
import json
import os
import zlib

import numpy as np
import pytest

import icp_oracle
from conftest import GOLDEN

SIG = json.load(open(os.path.join(GOLDEN, "signatures_icp.json")))["coreg"]
EPS = 2.0 ** -52
RUNS = {"plane": ("point-to-plane", "device", True, False), "lsq": ("point-to-plane", "lsq_approx", False, False),
        "point": ("point-to-point", "device", True, False), "trans": ("point-to-plane", "device", True, True)}


@functools.lru_cache(maxsize=None)
def golden():
    return dict(np.load(os.path.join(GOLDEN, "icp_golden.npz")))


def crc(a) -> int:
    return zlib.crc32(np.ascontiguousarray(a, dtype=np.int64).tobytes())


def unpack(bits, shape):
    return np.unpackbits(bits)[: int(np.prod(shape))].reshape(shape).astype(bool)


@functools.lru_cache(maxsize=None)
def case_clouds(case, run):
    """(ref_epc, tba_epc, norms, centroid, std_fac, mask) of a recorded run, rebuilt by the oracle from the rasters and the recorded
    normal planes (the reference's own: the oracle's differ from them by up to ``norms_gap`` ulps, which is checked on its own)."""
    g = golden()
    method = RUNS[run][0]
    ref, tba, t6 = g[f"{case}_ref"], g[f"{case}_tba"], tuple(g[f"{case}_transform"])
    inlier = unpack(g[f"{case}_inlier"], ref.shape)
    norms = (g[f"{case}_nx"], g[f"{case}_ny"], g[f"{case}_nz"]) if method == "point-to-plane" else None
    mask = icp_oracle.valid_mask(ref, tba, inlier, norms)
    r, t, n = icp_oracle.clouds(ref, tba, mask, t6, norms)
    r, t, cen, fac = icp_oracle.standardize(r, t)
    for a in (r, t) + (() if n is None else (n,)):
        a.setflags(write=False)
    return r, t, n, cen, fac, mask


def ulp_gap(a, b) -> int:
    it = np.int32 if a.dtype == np.float32 else np.int64

    def key(v):
        k = v.view(it).astype(np.int64)
        return np.where(k < 0, np.iinfo(it).min - k, k)

    ok = np.isfinite(a) & np.isfinite(b)
    return int(np.abs(key(a[ok]) - key(b[ok])).max())


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
    import scipy.optimize

    from xdem_amd import coreg, icp

    c = coreg.ICP()
    assert c.meta["inputs"]["specific"] == {"icp_method": "point-to-plane", "icp_picky": True}
    assert c.meta["inputs"]["fitorbin"]["fit_minimizer"] is scipy.optimize.least_squares
    assert c.meta["inputs"]["fitorbin"]["fit_loss_func"] == "linear"
    assert c.meta["inputs"]["iterative"] == {"max_iterations": 20, "tolerance": 0.01}
    assert c.meta["inputs"]["random"]["subsample"] == 5e5
    assert c.meta["inputs"]["affine"] == {"only_translation": False, "standardize": True}
    assert c.is_affine and c.centroid() is None and c._needs_transform
    assert isinstance(coreg.NuthKaab() + c, coreg.CoregPipeline)
    assert coreg.ICP is icp.ICP and coreg.nearest is icp.nearest
    assert coreg.ICP(fit_minimizer="lsq_approx")._route() == "lsq_approx" and c._route() == "device"
    assert coreg.ICP(fit_loss_func="soft_l1")._route() == "host" and coreg.ICP(fit_minimizer=scipy.optimize.minimize)._route() == "host"
    d = c.copy()
    d.meta["inputs"]["specific"]["icp_picky"] = False
    assert c.meta["inputs"]["specific"]["icp_picky"] is True


def test_errors_without_a_device():
    from xdem_amd import coreg

    dem = np.zeros((8, 9), dtype=np.float32)
    with pytest.raises(NotImplementedError, match="initial_shift"):
        coreg.ICP(initial_shift=(1, 2))
    with pytest.raises(ValueError, match="ICP method must be 'point-to-point' or 'point-to-plane'."):
        coreg.ICP(method="point-to-line").fit(dem, dem, resolution=1.0)
    with pytest.raises(ValueError, match="Fit optimizer 'lst_approx' of ICP is only available for point-to-plane method."):
        coreg.ICP(method="point-to-point", fit_minimizer="lsq_approx").fit(dem, dem, resolution=1.0)
    with pytest.raises(TypeError, match="fit_minimizer"):
        coreg.ICP(fit_minimizer=3).fit(dem, dem, resolution=1.0)
    with pytest.raises(NotImplementedError, match="Weights have not yet been implemented"):
        coreg.ICP().fit(dem, dem, weights=dem, resolution=1.0)
    with pytest.raises(NotImplementedError, match="bias_vars"):
        coreg.ICP().fit(dem, dem, bias_vars={"a": dem}, resolution=1.0)

    class Cloud:
        geometry = None

    with pytest.raises(NotImplementedError, match="point-cloud inputs are not supported"):
        coreg.ICP().fit(Cloud(), dem, resolution=1.0)
    with pytest.raises(AssertionError, match="fit"):
        coreg.ICP().apply(dem, resolution=1.0)
    fitted = coreg.ICP()
    fitted.meta["outputs"]["affine"] = {"matrix": coreg.matrix_from_translations_rotations(1, 2, 3, 0.1, 0.2, 0.3), "centroid": (0.0, 0.0, 0.0)}
    with pytest.raises(NotImplementedError, match="Option `resample=False` not supported by"):
        fitted.apply(dem, resample=False, resolution=1.0)
    with pytest.raises(NotImplementedError, match="resampling"):
        fitted.apply(dem, resampling="cubic", resolution=1.0)
    assert np.allclose(fitted.to_rotations(), (0.1, 0.2, 0.3)) and fitted.to_translations() == (1.0, 2.0, 3.0)
    assert fitted.centroid() == (0.0, 0.0, 0.0)
    for bad in (np.zeros((2, 5)), np.zeros((3, 0)), np.full((3, 4), np.nan)):
        with pytest.raises(ValueError, match="ref_points"):
            coreg.nearest(bad, np.zeros((3, 2)))
    with pytest.raises(ValueError, match="query_points"):
        coreg.nearest(np.zeros((3, 2)), np.zeros((4, 2)))


# ---- the host solves ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("run", ["plane", "point", "trans"])
def test_gauss_newton_on_sums_gives_the_oracle_step(run):
    """The product's Gauss-Newton on the 37 sums (formed here by the oracle's fsum) against the oracle's lstsq on the rows, on the
    pairs of the recorded iterations 0 and 1: both stop at updates below 1e-14, so the steps agree to rounding amplified by cond."""
    from xdem_amd import icp

    g = golden()
    method, _, use_picky, only_t = RUNS[run]
    r, t, n, _, _, _ = case_clouds("f64", run)
    for i in (0, 1):
        it = icp_oracle.iteration(g[f"f64_{run}_matrix_in"][i], r, t, n, method, use_picky, only_t, blas=True)
        kq, kr = it["kept_q"], it["kept_r"]
        pr, pt, pn = r[:, kr], it["trans"][:, kq], None if n is None else n[:, kr]

        def evaluate(S):
            J, res = icp_oracle.pair_terms(pr, pt, pn, S, method)
            return icp_oracle.fit_sums(J, res, icp_oracle.apply(S, pt))[0], pt.shape[1]

        S, n_eval = icp.gauss_newton(evaluate, only_t, vector=method == "point-to-point")
        assert n_eval < icp.GN_MAX_EVALUATIONS
        assert np.abs(icp.step_from(S) - it["step"]).max() <= 1e-12
        if only_t:
            assert np.array_equal(icp.step_from(S)[:3, :3], np.eye(3))


def test_scalar_rows_do_not_converge_for_point_to_point():
    """Why point-to-point takes the normal matrix of the vector residual: on the recorded pairs a Gauss-Newton loop on J^T J of the
    scalar distance rows ends its 50 evaluations at a HIGHER cost than the reference's least_squares reached, the loop on the vector
    residual at a lower one (both have the gradient J^T r)."""
    from xdem_amd import icp

    g = golden()
    r, t, n, _, _, _ = case_clouds("f64", "point")
    it = icp_oracle.iteration(g["f64_point_matrix_in"][0], r, t, n, "point-to-point", True, False, blas=True)
    pr, pt = r[:, it["kept_r"]], it["trans"][:, it["kept_q"]]

    def evaluate(S):
        J, res = icp_oracle.pair_terms(pr, pt, None, S, "point-to-point")
        return icp_oracle.fit_sums(J, res, icp_oracle.apply(S, pt))[0], pt.shape[1]

    def cost(S):
        return evaluate(S)[0][27]

    reference = cost(g["f64_point_step"][0])
    S_scalar, n_scalar = icp.gauss_newton(evaluate, False, vector=False)
    S_vector, n_vector = icp.gauss_newton(evaluate, False, vector=True)
    assert n_scalar == icp.GN_MAX_EVALUATIONS and cost(S_scalar) > 1.1 * reference
    assert n_vector < 10 and cost(S_vector) <= reference


def test_update_matrix_is_a_rotation():
    from xdem_amd import icp

    for x in ([0, 0, 0, 1, 2, 3], [1e-9, -2e-9, 3e-9, 0, 0, 0], [1e-5, 2e-5, -1e-5, 0.5, 0, 0], [0.3, -0.2, 0.5, 1, 1, 1]):
        T = icp.update_matrix(np.array(x, dtype=np.float64))
        assert np.abs(T[:3, :3].T @ T[:3, :3] - np.eye(3)).max() <= 8 * EPS and abs(np.linalg.det(T[:3, :3]) - 1) <= 8 * EPS
        assert np.array_equal(T[:3, 3], x[3:]) and np.array_equal(T[3], [0, 0, 0, 1])
        assert np.abs(T - icp_oracle.rodrigues(np.array(x, dtype=np.float64))).max() <= 4 * EPS
    w = np.array([0.3, -0.2, 0.5])
    v = np.array([0.7, 0.1, -0.4])
    first_order = v + 1e-7 * np.cross(w, v)
    assert np.abs(icp.update_matrix(np.concatenate((1e-7 * w, np.zeros(3))))[:3, :3] @ v - first_order).max() <= 1e-13


def test_fit_func_is_the_reference_residual():
    """``fit_func`` at the recorded step of a recorded iteration gives the residuals whose squares sum to the cost the oracle computes."""
    from xdem_amd import icp

    g = golden()
    for run in ("plane", "point"):
        method = RUNS[run][0]
        r, t, n, _, _, _ = case_clouds("f64", run)
        it = icp_oracle.iteration(g[f"f64_{run}_matrix_in"][0], r, t, n, method, True, False, blas=True)
        inputs = (r[:, it["kept_r"]], it["trans"][:, it["kept_q"]], None if n is None else n[:, it["kept_r"]])
        from xdem_amd import rigid

        p = rigid.translations_rotations_from_matrix(it["step"], return_degrees=False)
        mine, theirs = icp.fit_func(inputs, p, method), icp_oracle.fit_func(inputs, p, method)
        assert mine.shape == (inputs[0].shape[1],) and np.abs(mine - theirs).max() <= 64 * EPS
        assert np.abs(icp.fit_func(inputs, p[:3], method) - icp_oracle.fit_func(inputs, p[:3], method)).max() <= 64 * EPS


# ---- the oracle against the reference's recorded runs -------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["f32", "f64"])
def test_oracle_normals_follow_the_reference(case):
    g = golden()
    ref, t6 = g[f"{case}_ref"], tuple(g[f"{case}_transform"])
    mine = icp_oracle.normals(ref, abs(t6[0]), abs(t6[4]))
    for k, name in enumerate(("nx", "ny", "nz")):
        want = g[f"{case}_{name}"]
        assert mine[k].dtype == want.dtype == ref.dtype
        assert np.array_equal(np.isfinite(mine[k]), np.isfinite(want))
        assert ulp_gap(mine[k], want) <= int(g[f"{case}_norms_gap"][k]), name
    assert int(g[f"{case}_norms_gap"][0]) <= 2 and int(g[f"{case}_norms_gap"][1]) <= 2   # (sin(arctan) against g / sqrt(1 + g^2))
    # nz = 1 - sqrt(nx^2 + ny^2) cancels: its gap in ulps of nz is a few ulps of 1
    eps = float(np.finfo(ref.dtype).eps)
    ok = np.isfinite(mine[2])
    assert np.abs(mine[2][ok].astype(np.float64) - g[f"{case}_nz"][ok]).max() <= 4 * eps
    # NaN exactly where the pixel or a neighbour np.gradient reads is NaN
    bad = ~np.isfinite(ref)
    near = bad.copy()
    near[1:, :] |= bad[:-1, :]; near[:-1, :] |= bad[1:, :]; near[:, 1:] |= bad[:, :-1]; near[:, :-1] |= bad[:, 1:]
    interior = np.zeros_like(bad)
    interior[1:-1, 1:-1] = True
    assert not np.isfinite(mine[2][near & interior & ~bad]).any() and np.isfinite(mine[2][~near]).all()


@pytest.mark.parametrize("case", ["f32", "f64"])
@pytest.mark.parametrize("run", sorted(RUNS))
def test_oracle_follows_the_reference_step_by_step(case, run):
    g = golden()
    key = f"{case}_{run}"
    method, route, use_picky, only_t = RUNS[run]
    r, t, n, cen, fac, mask = case_clouds(case, run)
    assert np.array_equal(mask, unpack(g[f"{key}_mask"], mask.shape))
    assert cen == tuple(g[f"{key}_centroid"]) and fac == float(g[f"{key}_std_fac"])
    import scipy.spatial

    tree = scipy.spatial.KDTree(r.T)
    own = np.arange(r.shape[1])
    tol = 10 * float(g[f"{key}_solve_gap"] if route == "device" else g["lsq_gap"])
    full = set(int(i) for i in g[f"{key}_full_iterations"])
    stride = int(g["dist_stride"])
    n_it = len(g[f"{key}_stat"])
    assert full == {0, 1, n_it - 1}
    for i in range(n_it):
        it = icp_oracle.iteration(g[f"{key}_matrix_in"][i], r, t, n, method, use_picky, only_t, route, tree, blas=True)
        assert crc(it["ind"]) == int(g[f"{key}_crc_ind"][i]), (key, i)
        assert crc(it["kept_q"]) == int(g[f"{key}_crc_kept"][i]) and it["kept_q"].size == int(g[f"{key}_n_kept"][i]), (key, i)
        assert np.all(np.diff(it["kept_r"]) > 0) if use_picky else np.array_equal(it["kept_q"], own)
        if i in full:
            assert np.array_equal(it["ind"], own + g[f"{key}_it{i}_ind_offset"])
            flags = np.zeros(own.size, dtype=bool)
            flags[it["kept_q"]] = True
            assert np.array_equal(flags, unpack(g[f"{key}_it{i}_kept"], own.shape))
            want = g[f"{key}_it{i}_dists"]
            assert np.all(np.abs(it["dists"][::stride] - want) <= 4 * EPS * want), (key, i)
        gap = np.abs(it["step"] - g[f"{key}_step"][i]).max()
        if route == "lsq_approx":   # the oracle's lstsq against the reference's explicit inverse: rounding amplified by cond
            x = np.abs(icp_oracle.lsq_approx(r[:, it["kept_r"]], it["trans"][:, it["kept_q"]], n[:, it["kept_r"]])[1]).max()
            assert gap <= it["kept_q"].size * EPS * float(g[f"{key}_cond"][i]) * x + tol, (key, i, gap)
        else:
            assert gap <= tol, (key, i, gap, tol)
        assert abs(it["stat"] - g[f"{key}_stat"][i]) <= 3 * max(tol, 1e-15)
        if i + 1 < n_it:   # the recorded driver went on from step @ matrix
            assert np.array_equal(g[f"{key}_step"][i] @ g[f"{key}_matrix_in"][i], g[f"{key}_matrix_in"][i + 1])
    # the recorded run stopped by upstream's rule, or at max_iterations
    stats, stop = g[f"{key}_stat"], float(g["tolerance"]) / fac
    assert (n_it == 20 or stats[-1] < stop) and all(s >= stop for s in stats[2:-1])
    assert np.array_equal(g[f"{key}_final"][:3, :3], (g[f"{key}_step"][-1] @ g[f"{key}_matrix_in"][-1])[:3, :3])
    assert np.array_equal(g[f"{key}_final"][:3, 3], (g[f"{key}_step"][-1] @ g[f"{key}_matrix_in"][-1])[:3, 3] * fac)   # de-standardised


def test_fixture_is_not_trivial():
    """What makes the fixture a test of the search: points leave their own pixel, picky removes pairs, no near-tie."""
    g = golden()
    assert float(g["margin_min"]) > 1e-9
    for case in ("f32", "f64"):
        for run, (_, _, use_picky, _) in RUNS.items():
            key = f"{case}_{run}"
            n = g[f"{key}_it0_ind_offset"].size
            assert np.count_nonzero(g[f"{key}_it0_ind_offset"]) > 0.30 * n
            last = int(g[f"{key}_full_iterations"][-1])
            assert np.count_nonzero(g[f"{key}_it{last}_ind_offset"]) > 0.90 * n
            if use_picky:
                assert np.all(g[f"{key}_n_kept"] < 0.95 * n)


def test_oracle_picky_and_brute_force():
    """The NumPy picky removal on constructed ties, and brute force against the tree on a recorded iteration."""
    ind = np.array([3, 1, 3, 1, 0, 3, 7])
    dist = np.array([0.5, 0.25, 0.5, 0.25, 1.0, 0.75, 0.0])
    q, r = icp_oracle.picky(ind, dist)
    assert q.tolist() == [4, 1, 0, 6] and r.tolist() == [0, 1, 3, 7]
    g = golden()
    ref, t, n, _, _, _ = case_clouds("f64", "plane")
    trans = icp_oracle.apply(g["f64_plane_matrix_in"][1], t)[:, :1500]
    d0, i0 = icp_oracle.nearest_brute(ref, trans)
    d1, i1 = icp_oracle.nearest_tree(ref, trans)
    assert np.array_equal(i0, i1) and np.all(np.abs(d0 - d1) <= 4 * EPS * d1)
