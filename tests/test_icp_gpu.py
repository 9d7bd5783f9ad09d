"""ICP on the GPU (csrc/icp.hip, xdem_amd/icp.py): the exact nearest-neighbour search against ``scipy.spatial.KDTree``, the picky
removal against tests/icp_oracle.py on constructed ties, the sums of the fit within the worst-case bound of recursive summation and
repeatable to the byte, normal planes and standardisation against the oracle, single steps from the recorded input matrices of the
reference's runs (tests/golden/icp_golden.npz, tools/gen_golden_icp.py) and whole fits, alone, in a pipeline and through
``DEM.coregister_3d``."""
import functools
import os
import zlib

import numpy as np
import pytest
import scipy.spatial

import icp_oracle
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

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


def rasters(case):
    g = golden()
    ref = g[f"{case}_ref"]
    return ref, g[f"{case}_tba"], unpack(g[f"{case}_inlier"], ref.shape), tuple(g[f"{case}_transform"])


@functools.lru_cache(maxsize=None)
def reference_clouds(case, run):
    """The standardised clouds of a recorded run with the REFERENCE's normal planes (the inputs of the recorded iterations)."""
    g = golden()
    ref, tba, inlier, t6 = rasters(case)
    norms = (g[f"{case}_nx"], g[f"{case}_ny"], g[f"{case}_nz"]) if RUNS[run][0] == "point-to-plane" else None
    mask = icp_oracle.valid_mask(ref, tba, inlier, norms)
    r, t, n = icp_oracle.clouds(ref, tba, mask, t6, norms)
    r, t, cen, fac = icp_oracle.standardize(r, t)
    return r, t, n, cen, fac


@functools.lru_cache(maxsize=None)
def oracle_clouds(case, plane: bool, flip: bool = False):
    """The same with the ORACLE's planes (what the device forms itself); ``flip`` masks one more pixel (the other parity of the count)."""
    ref, tba, inlier, t6 = rasters(case)
    norms = icp_oracle.normals(ref, abs(t6[0]), abs(t6[4])) if plane else None
    if flip:
        rows, cols = np.nonzero(icp_oracle.valid_mask(ref, tba, inlier, norms))
        inlier = inlier.copy()
        inlier[rows[0], cols[0]] = False
    mask = icp_oracle.valid_mask(ref, tba, inlier, norms)
    r, t, n = icp_oracle.clouds(ref, tba, mask, t6, norms)
    return icp_oracle.standardize(r, t) + (n, mask, inlier, norms)


def ulp_gap(a, b) -> int:
    it = np.int32 if a.dtype == np.float32 else np.int64

    def key(v):
        k = v.view(it).astype(np.int64)
        return np.where(k < 0, np.iinfo(it).min - k, k)

    ok = np.isfinite(a) & np.isfinite(b)
    return int(np.abs(key(a[ok]) - key(b[ok])).max()) if ok.any() else 0


# ---- nearest --------------------------------------------------------------------------------------------------------------------------
def check_nearest(ref, qry, matrix=None, excuse=0):
    """``nearest`` against the tree: dist within 4 * 2^-52 relative; ind equal wherever the tree's k = 2 margin exceeds 1e-12; at most
    ``excuse`` queries (a count) may be excused that way."""
    from xdem_amd import coreg

    dist, ind = coreg.nearest(ref, qry, matrix)
    moved = qry if matrix is None else icp_oracle.apply(matrix, qry)
    tree = scipy.spatial.KDTree(ref.T)
    if ref.shape[1] > 1:
        d2, i2 = tree.query(moved.T, k=2)
        with np.errstate(invalid="ignore", divide="ignore"):
            margin = np.where(d2[:, 1] > 0, (d2[:, 1] - d2[:, 0]) / d2[:, 1], 0.0)
        d, i = d2[:, 0], i2[:, 0]
    else:
        d, i = tree.query(moved.T, k=1)
        margin = np.ones(d.shape)
    assert dist.dtype == np.float64 and ind.dtype == np.int64 and dist.shape == ind.shape == (qry.shape[1],)
    assert np.all(np.abs(dist - d) <= 4 * EPS * d), np.abs(dist - d).max()
    clear = margin > 1e-12
    assert np.count_nonzero(~clear) <= excuse, np.count_nonzero(~clear)
    assert np.array_equal(ind[clear], i[clear])
    # the excused ones still hold a point at the smallest distance
    far = np.sqrt(((moved[:, ~clear] - ref[:, ind[~clear]]) ** 2).sum(axis=0))
    assert np.all(np.abs(far - d[~clear]) <= 4 * EPS * d[~clear])
    return dist, ind


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 257])
@pytest.mark.parametrize("m", [1, 65])
def test_nearest_small_clouds(n, m):
    rng = np.random.default_rng(100 * n + m)
    ref = rng.normal(size=(3, n)) * np.array([[5.0], [3.0], [0.5]])
    qry = rng.normal(size=(3, m)) * np.array([[6.0], [4.0], [0.7]])
    d0, i0 = check_nearest(ref, qry)
    d1, i1 = check_nearest(ref, qry)
    assert d0.tobytes() == d1.tobytes() and i0.tobytes() == i1.tobytes()
    from xdem_amd import coreg

    m4 = coreg.matrix_from_translations_rotations(0.4, -0.3, 0.1, 2.0, -3.0, 5.0)
    check_nearest(ref, qry, m4)


def test_nearest_zero_extent_axis():
    rng = np.random.default_rng(7)
    for axis in (0, 1):
        ref = rng.normal(size=(3, 257))
        ref[axis] = 1.25
        qry = rng.normal(size=(3, 65))
        check_nearest(ref, qry)
    ref = np.tile(np.array([[1.0], [2.0], [3.0]]), (1, 5)) + np.array([[0.0], [0.0], [1.0]]) * np.arange(5)   # both extents zero
    check_nearest(ref, rng.normal(size=(3, 9)) + np.array([[1.0], [2.0], [5.0]]))


def test_nearest_two_far_clusters():
    """Two clusters 1 000 extents apart: almost every cell is empty, queries in between walk many rings."""
    rng = np.random.default_rng(8)
    a = rng.uniform(0.0, 1.0, size=(3, 130))
    b = rng.uniform(0.0, 1.0, size=(3, 127)) + np.array([[1000.0], [1000.0], [0.0]])
    ref = np.hstack((a, b))
    qry = np.hstack((rng.uniform(0.0, 1.0, size=(3, 20)), rng.uniform(0.0, 1.0, size=(3, 20)) + np.array([[1000.0], [1000.0], [0.0]]),
                     rng.uniform(0.0, 1000.0, size=(3, 25)) * np.array([[1.0], [1.0], [0.001]])))
    check_nearest(ref, qry)


def test_nearest_on_cell_edges_reference_points_and_outside():
    from xdem_amd import icp

    rng = np.random.default_rng(9)
    ref = rng.uniform(-1.0, 1.0, size=(3, 257)) * np.array([[40.0], [25.0], [2.0]])
    with icp.IcpCloud.from_points(ref, ref[:, :1]) as cloud:
        x0, y0, h, gx, gy = cloud.grid()
    assert gx > 3 and gy > 3 and 257 / 6.0 < gx * gy < 2 * 257 + 16 and x0 == ref[0].min() and y0 == ref[1].min()
    ex, ey = x0 + np.arange(gx + 1) * h, y0 + np.arange(gy + 1) * h
    on_edges = np.array([[x, y, z] for x in ex for y in ey[::2] for z in (0.0,)]).T
    on_x_only = np.vstack((np.repeat(ex, 3), rng.uniform(y0, ey[-1], 3 * ex.size), rng.normal(size=3 * ex.size)))
    on_y_only = np.vstack((rng.uniform(x0, ex[-1], 3 * ey.size), np.repeat(ey, 3), rng.normal(size=3 * ey.size)))
    wx, wy = ref[0].max() - x0, ref[1].max() - y0
    cx, cy = x0 + wx / 2, y0 + wy / 2
    outside = np.array([[x0 - 10 * wx, cy, 0.0], [x0 + 11 * wx, cy, 0.3], [cx, y0 - 10 * wy, -0.2], [cx, y0 + 11 * wy, 0.1],
                        [x0 - 10 * wx, y0 - 10 * wy, 0.0], [x0 + 11 * wx, y0 + 11 * wy, 50.0]]).T
    qry = np.hstack((on_edges, on_x_only, on_y_only, ref[:, ::3], outside))
    dist, ind = check_nearest(ref, qry)
    k = on_edges.shape[1] + on_x_only.shape[1] + on_y_only.shape[1]
    assert np.array_equal(ind[k: k + ref[:, ::3].shape[1]], np.arange(0, 257, 3)) and not dist[k: k + ref[:, ::3].shape[1]].any()


def test_nearest_exact_duplicates_take_the_lowest_index():
    rng = np.random.default_rng(10)
    base = rng.normal(size=(3, 65))
    ref = np.hstack((base, base[:, ::2], base[:, :10]))   # every other point twice, the first ten (some) three times
    qry = np.hstack((rng.normal(size=(3, 130)), base[:, 5:25]))
    from xdem_amd import coreg

    dist, ind = coreg.nearest(ref, qry)
    d, i = icp_oracle.nearest_brute(ref, qry)   # np.argmin: the first index of the minimum
    assert np.all(np.abs(dist - d) <= 4 * EPS * d) and np.array_equal(ind, i) and np.all(ind < 65)
    tree_d = scipy.spatial.KDTree(ref.T).query(qry.T, k=1)[0]
    assert np.all(np.abs(dist - tree_d) <= 4 * EPS * tree_d)


def test_nearest_large_random():
    rng = np.random.default_rng(11)
    n = 200_000
    ref = rng.uniform(0.0, 1.0, size=(3, n)) * np.array([[100.0], [80.0], [3.0]])
    qry = rng.uniform(-0.02, 1.02, size=(3, n)) * np.array([[100.0], [80.0], [3.0]])
    check_nearest(ref, qry, excuse=n // 1000)


# ---- picky ----------------------------------------------------------------------------------------------------------------------------
def _picky_case(ind, dist, n):
    from xdem_amd import icp

    rng = np.random.default_rng(12)
    ind, dist = np.asarray(ind, dtype=np.int64), np.asarray(dist, dtype=np.float64)
    with icp.IcpCloud.from_points(rng.normal(size=(3, n)), rng.normal(size=(3, ind.size))) as cloud:
        cloud.set_pairs(ind, dist)
        k, q, r = cloud.pairs(True, fetch=True)
        k2, q2, r2 = cloud.pairs(True, fetch=True)
        k0, q0, r0 = cloud.pairs(False, fetch=True)
    wq, wr = icp_oracle.picky(ind, dist)
    assert k == wq.size and np.array_equal(q, wq) and np.array_equal(r, wr) and np.all(np.diff(r) > 0)
    assert k2 == k and np.array_equal(q2, q) and np.array_equal(r2, r)
    assert k0 == ind.size and np.array_equal(q0, np.arange(ind.size)) and np.array_equal(r0, ind)   # without picky: every pair, query order
    return q, r


def test_picky_ties_group_sizes_and_order():
    # groups of 1, 2 and 70 queries, ties in distance inside the groups: the lowest query index wins
    ind = np.concatenate(([5], [2, 2], np.full(70, 9), [0]))
    dist = np.concatenate(([0.5], [0.25, 0.25], np.tile([0.75, 0.5, 0.5, 1.0, 0.5], 14), [0.0]))
    perm = np.random.default_rng(13).permutation(ind.size)
    q, r = _picky_case(ind[perm], dist[perm], 12)
    assert r.tolist() == [0, 2, 5, 9]
    assert dist[perm][q].tolist() == [0.0, 0.25, 0.5, 0.5]
    first_of_9 = min(i for i in range(ind.size) if ind[perm][i] == 9 and dist[perm][i] == 0.5)
    first_of_2 = min(i for i in range(ind.size) if ind[perm][i] == 2)
    assert q[3] == first_of_9 and q[1] == first_of_2
    # a distance of zero and its neighbours in bit order
    _picky_case([1, 1, 1, 1], [5e-324, 0.0, 0.0, 1.0], 3)


def test_picky_all_collide_and_none_collide():
    rng = np.random.default_rng(14)
    q, r = _picky_case(np.full(300, 4), rng.uniform(1.0, 2.0, 300), 9)
    assert q.size == 1 and r.tolist() == [4]
    q, r = _picky_case(rng.permutation(5000)[:4500], rng.uniform(0.0, 1.0, 4500), 5000)   # more than one tile of reference indexes
    assert q.size == 4500


# ---- the sums of the fit --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 63, 64, 65, 4097])
@pytest.mark.parametrize("method", ["point-to-plane", "point-to-point"])
def test_fit_sums_against_the_oracle(k, method):
    """Pairs (i, i) by construction -- reference points on a jittered lattice of spacing 1, queries within 0.02 of them, some exactly on
    them (r = 0) -- so the sums come from the public path query -> pairs -> sums.  Each sum lies within k * 2^-52 * sum|terms| of the
    oracle's fsum (recursive summation of k terms, in any order), and two calls return the same bytes."""
    from xdem_amd import coreg, icp

    rng = np.random.default_rng(15 + k)
    i = np.arange(k)
    ref = np.vstack((i % 17, (i // 17) % 17, i // 289)).astype(np.float64) + rng.uniform(-0.1, 0.1, size=(3, k))
    qry = ref + rng.uniform(-0.02, 0.02, size=(3, k))
    qry[:, ::7] = ref[:, ::7]
    nrm = rng.normal(size=(3, k))
    nrm /= np.linalg.norm(nrm, axis=0)
    S = coreg.matrix_from_translations_rotations(0.01, -0.02, 0.005, 0.2, -0.1, 0.3)
    with icp.IcpCloud.from_points(ref, qry, nrm) as cloud:
        dist, ind = cloud.query()
        assert np.array_equal(ind, i)
        outs = []
        for use_picky in (False, True, False):
            assert cloud.pairs(use_picky) == k
            outs.append(cloud.sums(S, method))
        ref_v, trans_v, nrm_v = cloud.values(k)
    assert np.array_equal(ref_v, ref) and np.array_equal(trans_v, qry) and np.array_equal(nrm_v, nrm)
    J, r = icp_oracle.pair_terms(ref, qry, nrm, S, method)
    if method == "point-to-point":
        assert np.count_nonzero(r == 0) == 0   # (under S the coincident pairs have moved apart; at the identity they have not)
    want, mag = icp_oracle.fit_sums(J, r, icp_oracle.apply(S, qry))
    for sums, cnt in outs:
        assert cnt == k and sums.shape == (37,)
        assert np.all(np.abs(sums - want) <= k * EPS * mag), np.max(np.abs(sums - want) / np.maximum(mag, 1e-300))
        assert sums.tobytes() == outs[0][0].tobytes()
    # at the identity the coincident pairs have r = 0: a zero row in point-to-point, no NaN
    with icp.IcpCloud.from_points(ref, qry, nrm) as cloud:
        cloud.query(fetch=False)
        cloud.pairs(False)
        sums, cnt = cloud.sums(np.eye(4), method)
    J, r = icp_oracle.pair_terms(ref, qry, nrm, np.eye(4), method)
    if method == "point-to-point":
        assert np.count_nonzero(r == 0) == len(range(0, k, 7)) and not J[:, ::7].any()
    want, mag = icp_oracle.fit_sums(J, r, qry)
    assert cnt == k and np.all(np.isfinite(sums)) and np.all(np.abs(sums - want) <= k * EPS * mag)


# ---- normal planes and standardisation --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["f32", "f64"])
def test_normal_planes_and_mask_narrowing(case):
    from xdem_amd import _lib, icp
    from xdem_amd.biascorr import DhPlan

    ref, tba, inlier, t6 = rasters(case)
    want = icp_oracle.normals(ref, abs(t6[0]), abs(t6[4]))
    with DhPlan(ref, tba, inlier) as plan:
        before = plan.n_valid
        got = icp.icp_normals(plan, t6)
        after = plan.n_valid
        again = icp.icp_normals(plan, t6)   # a second call only copies
        assert plan.n_valid == after and all(np.array_equal(a, b, equal_nan=True) for a, b in zip(got, again))
        plan.subsample(np.arange(0, after, 3))
    assert before == np.count_nonzero(icp_oracle.valid_mask(ref, tba, inlier))
    assert after == np.count_nonzero(icp_oracle.valid_mask(ref, tba, inlier, want)) and after < before
    for k in range(3):
        assert got[k].dtype == ref.dtype and np.array_equal(np.isnan(got[k]), np.isnan(want[k]))
    assert ulp_gap(got[0], want[0]) <= 1 and ulp_gap(got[1], want[1]) <= 1
    # nz = 1 - sqrt(nx^2 + ny^2): within 1 ulp where nx and ny are the oracle's bits, else within the few ulps of 1 that one ulp of
    # nx, ny moves the root by
    same = (got[0] == want[0]) & (got[1] == want[1])
    assert ulp_gap(np.where(same, got[2], np.nan), np.where(same, want[2], np.nan)) <= 1
    ok = np.isfinite(want[2])
    assert np.abs(got[2][ok].astype(np.float64) - want[2][ok]).max() <= 4 * float(np.finfo(ref.dtype).eps)
    # NaN exactly where a pixel that np.gradient reads is NaN: the two neighbours along each axis, at a border the pixel and its inner
    # neighbour (a NaN pixel between finite neighbours has finite planes; the mask drops it through ref)
    bad = ~np.isfinite(ref)
    reads = np.zeros_like(bad)
    reads[:, 1:-1] |= bad[:, :-2] | bad[:, 2:]
    reads[1:-1, :] |= bad[:-2, :] | bad[2:, :]
    reads[:, 0] |= bad[:, 0] | bad[:, 1]; reads[:, -1] |= bad[:, -1] | bad[:, -2]
    reads[0, :] |= bad[0, :] | bad[1, :]; reads[-1, :] |= bad[-1, :] | bad[-2, :]
    assert np.array_equal(np.isnan(got[2]), reads) and reads.any() and (bad & ~reads).any()
    # after a draw the planes can no longer narrow the mask
    with DhPlan(ref, tba, inlier) as plan:
        plan.subsample(np.arange(0, plan.n_valid, 2))
        with pytest.raises(_lib.XdemHipError, match="before the draw"):
            icp.icp_normals(plan, t6)


@pytest.mark.parametrize("shape", [(2, 2), (3, 130), (67, 129)])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_normal_planes_awkward_shapes(shape, dtype):
    from xdem_amd import icp
    from xdem_amd.biascorr import DhPlan

    rng = np.random.default_rng(shape[0] * 1000 + shape[1])
    ref = (800.0 + 50.0 * rng.normal(size=shape).cumsum(axis=1)).astype(dtype)
    if ref.size > 4:
        ref[rng.random(shape) < 0.05] = np.nan
        ref.flat[1] = np.inf
    t6 = (3.0, 0.0, 10.0, 0.0, -7.0, 400.0)
    want = icp_oracle.normals(ref, 3.0, 7.0)
    with DhPlan(ref, ref, None) as plan:
        got = icp.icp_normals(plan, t6)
        assert plan.n_valid == np.count_nonzero(icp_oracle.valid_mask(ref, ref, None, want))
    for k in range(3):
        assert np.array_equal(np.isfinite(got[k]), np.isfinite(want[k])) and (k == 2 or ulp_gap(got[k], want[k]) <= 1)
        ok = np.isfinite(want[k])
        assert not ok.any() or np.abs(got[k][ok].astype(np.float64) - want[k][ok]).max() <= 4 * float(np.finfo(dtype).eps)


@pytest.mark.parametrize("case", ["f32", "f64"])
@pytest.mark.parametrize("plane", [True, False])
@pytest.mark.parametrize("flip", [False, True])
def test_clouds_centroid_and_std_fac_are_the_oracles_bits(case, plane, flip):
    from xdem_amd import icp
    from xdem_amd.biascorr import DhPlan

    ref, tba, _, t6 = rasters(case)
    r, t, cen, fac, n, mask, inlier, _ = oracle_clouds(case, plane, flip)
    with DhPlan(ref, tba, inlier) as plan:
        if plane:
            icp.icp_normals(plan, t6, fetch=False)
        with icp.IcpCloud.from_plan(plan, t6, plane) as cloud:
            got = cloud.cloud()
            assert cloud.n == cloud.m == r.shape[1] and cloud.centroid == cen and cloud.std_fac == fac
        with icp.IcpCloud.from_plan(plan, t6, plane, standardize=False) as cloud:
            raw = cloud.cloud()
            assert cloud.std_fac == 1.0 and cloud.centroid == cen
    assert np.array_equal(got[:3], r) and np.array_equal(got[3], t[2])
    assert np.array_equal(got[4:], n if plane else np.zeros((3, r.shape[1])))
    r1, t1, _, _ = icp_oracle.standardize(*icp_oracle.clouds(ref, tba, mask, t6)[:2], scale_std=False)
    assert np.array_equal(raw[:3], r1) and np.array_equal(raw[3], t1[2])


def test_counts_of_both_parities_are_covered():
    for case in ("f32", "f64"):
        assert {oracle_clouds(case, True, f)[0].shape[1] % 2 for f in (False, True)} == {0, 1}


# ---- single steps from the recorded input matrices ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["f32", "f64"])
@pytest.mark.parametrize("run", sorted(RUNS))
def test_steps_from_the_recorded_matrices(case, run):
    """From every recorded input matrix, on the recorded run's own inputs (the oracle's clouds, bit for bit the reference's, with the
    reference's normal planes): ``ind`` and the kept pairs are the fixture's (CRC-32 on every iteration, element by element where the
    fixture holds them), the step matrix lies within 10 x the run's ``solve_gap`` -- for "lsq_approx" within
    k * 2^-52 * cond * |x|_inf + 10 x ``lsq_gap``."""
    from xdem_amd import coreg, icp

    g = golden()
    key = f"{case}_{run}"
    method, route, use_picky, only_t = RUNS[run]
    r, t, n, cen, fac = reference_clouds(case, run)
    step_of = coreg.ICP(method=method, picky=use_picky, only_translation=only_t, **({"fit_minimizer": "lsq_approx"} if route == "lsq_approx" else {}))
    own = np.arange(r.shape[1])
    tol = 10 * float(g[f"{key}_solve_gap"] if route == "device" else g["lsq_gap"])
    full = set(int(i) for i in g[f"{key}_full_iterations"])
    worst = 0.0
    with icp.IcpCloud.from_points(r, t, n) as cloud:
        for i, matrix in enumerate(g[f"{key}_matrix_in"]):
            dist, ind = cloud.query(matrix)
            k, q, kr = cloud.pairs(use_picky, fetch=True)
            assert crc(ind) == int(g[f"{key}_crc_ind"][i]) and crc(q) == int(g[f"{key}_crc_kept"][i]) and k == int(g[f"{key}_n_kept"][i]), (key, i)
            assert np.array_equal(kr, ind[q])
            if i in full:
                assert np.array_equal(ind, own + g[f"{key}_it{i}_ind_offset"])
                flags = np.zeros(own.size, dtype=bool)
                flags[q] = True
                assert np.array_equal(flags, unpack(g[f"{key}_it{i}_kept"], own.shape))
                want = g[f"{key}_it{i}_dists"]
                # (the device moves the cloud with explicit sums, the reference with BLAS: the coordinates differ in the last bit, the
                #  distances by that over the distance)
                assert np.all(np.abs(dist[:: int(g["dist_stride"])] - want) <= 64 * EPS * np.maximum(want, 1.0))
            step = step_of._step_matrix(cloud, k, method)
            gap = float(np.abs(step - g[f"{key}_step"][i]).max())
            worst = max(worst, gap)
            if route == "lsq_approx":
                x = np.abs(icp_oracle.lsq_approx(r[:, kr], icp_oracle.apply(matrix, t)[:, q], n[:, kr])[1]).max()
                assert gap <= k * EPS * float(g[f"{key}_cond"][i]) * x + tol, (key, i, gap)
            else:
                assert gap <= tol, (key, i, gap, tol)
            if only_t:
                assert np.array_equal(step[:3, :3], np.eye(3))
    print(key, "largest step gap", worst, "bound", tol)


@pytest.mark.parametrize("case", ["f32", "f64"])
def test_plan_route_finds_the_recorded_pairs(case):
    """The same through the plan: the device's own planes, mask, gather and standardisation, then the recorded matrices."""
    from xdem_amd import icp
    from xdem_amd.biascorr import DhPlan

    g = golden()
    ref, tba, inlier, t6 = rasters(case)
    for run, plane in (("plane", True), ("point", False)):
        key = f"{case}_{run}"
        with DhPlan(ref, tba, inlier) as plan:
            if plane:
                icp.icp_normals(plan, t6, fetch=False)
            with icp.IcpCloud.from_plan(plan, t6, plane) as cloud:
                assert cloud.centroid == tuple(g[f"{key}_centroid"]) and cloud.std_fac == float(g[f"{key}_std_fac"])
                for i in sorted(int(v) for v in g[f"{key}_full_iterations"]):
                    _, ind = cloud.query(g[f"{key}_matrix_in"][i])
                    k, q, _ = cloud.pairs(True, fetch=True)
                    assert crc(ind) == int(g[f"{key}_crc_ind"][i]) and crc(q) == int(g[f"{key}_crc_kept"][i]), (key, i)


# ---- whole fits ---------------------------------------------------------------------------------------------------------------------------
def _fit(case, run, **kw):
    from xdem_amd import coreg

    g = golden()
    method, route, use_picky, only_t = RUNS[run]
    ref, tba, inlier, t6 = rasters(case)
    extra = {"fit_minimizer": "lsq_approx"} if route == "lsq_approx" else {}
    c = coreg.ICP(method=method, picky=use_picky, only_translation=only_t, tolerance=float(g["tolerance"]), subsample=1, **extra, **kw)
    return c.fit(ref, tba, inlier, transform=t6)


@pytest.mark.parametrize("case", ["f32", "f64"])
@pytest.mark.parametrize("run", sorted(RUNS))
def test_whole_fits_land_on_the_reference(case, run):
    """The final matrix (de-standardised) against the reference driver's: within 10 x ``trajectory_gap`` with a floor of 10 x
    ``solve_gap``, the two figures the generator recorded over all runs.  Where the run's own figures are tighter and the device's normal
    planes are the reference's to within float64 rounding (the float64 rasters) they are asserted too, the solve gap taken to the
    units of the de-standardised translation (x std_fac)."""
    g = golden()
    key = f"{case}_{run}"
    c = _fit(case, run)
    got, want = c.to_matrix(), g[f"{key}_final"]
    gap = float(np.abs(got - want).max())
    fac = float(g[f"{key}_std_fac"])
    own = 10 * max(float(g[f"{key}_trajectory_gap"]), fac * float(g[f"{key}_solve_gap"] if RUNS[run][1] == "device" else g["lsq_gap"]), 1e-9)
    print(key, "final gap", gap, "bound", 10 * max(float(g["trajectory_gap"]), float(g["solve_gap"])), "run's own", own,
          "iterations", c.meta["outputs"]["iterative"]["last_iteration"], "recorded", len(g[f"{key}_stat"]))
    assert gap <= 10 * max(float(g["trajectory_gap"]), float(g["solve_gap"]))
    if case == "f64":
        assert gap <= own
    assert c.centroid() == tuple(g[f"{key}_centroid"])
    assert c.meta["outputs"]["random"]["subsample_final"] == reference_clouds(case, run)[0].shape[1]
    out = c.meta["outputs"]
    assert out["affine"]["shift_x"] == got[0, 3] and out["affine"]["shift_y"] == got[1, 3] and out["affine"]["shift_z"] == got[2, 3]
    assert out["iterative"]["last_iteration"] == len(out["iterative"]["matrices"]) == len(out["iterative"]["statistics"]) <= 20
    if RUNS[run][3]:
        assert np.array_equal(got[:3, :3], np.eye(3)) and c.to_rotations() == (0.0, 0.0, 0.0)


def test_host_route_follows_the_oracle_driven_with_scipy():
    """``fit_loss_func="soft_l1"`` takes the host route: the pairs come from the device, ``least_squares`` runs on ``fit_func``.  Against
    the oracle's driver with the same SciPy call on its own planes, five iterations: the same bound as the whole fits."""
    import scipy.optimize

    g = golden()
    c = _fit("f64", "plane", fit_loss_func="soft_l1", max_iterations=5)
    assert c._route() == "host" and c.meta["outputs"]["iterative"]["last_iteration"] == 5
    r, t, cen, fac, n, _, _, _ = oracle_clouds("f64", True)
    final, trail = icp_oracle.drive(r, t, n, "point-to-plane", True, False, float(g["tolerance"]) / fac, 5, route="host",
                                    minimizer=scipy.optimize.least_squares, loss="soft_l1")
    final[:3, 3] *= fac
    gap = float(np.abs(c.to_matrix() - final).max())
    print("host route: final gap", gap)
    assert gap <= 10 * max(float(g["trajectory_gap"]), float(g["solve_gap"]))
    # a minimiser's keyword selects the host route too
    from xdem_amd import coreg

    ref, tba, inlier, t6 = rasters("f64")
    c2 = coreg.ICP(only_translation=True, max_iterations=3, subsample=1).fit(ref, tba, inlier, transform=t6, ftol=1e-10)
    assert np.array_equal(c2.to_matrix()[:3, :3], np.eye(3)) and np.abs(c2.to_matrix()[:3, 3]).max() > 1.0


def test_pipeline_coregister_3d_and_apply():
    from xdem_amd import coreg
    from xdem_amd.dem import DEM

    ref, tba, inlier, t6 = rasters("f32")

    def spread(a):
        d = (ref - a).astype(np.float64)
        return icp_oracle.nmad(d[np.isfinite(d)])

    before = spread(tba)
    c = coreg.ICP().fit(ref, tba, inlier, transform=t6)
    out, t = c.apply(tba, transform=t6)
    want, _ = coreg.apply_matrix(tba, c.to_matrix(), centroid=c.centroid(), transform=t6)
    assert t == t6 and out.dtype == tba.dtype and np.array_equal(out, want, equal_nan=True)
    assert spread(out) < 0.1 * before
    both, _ = coreg.ICP().fit_and_apply(ref, tba, inlier, transform=t6)
    assert np.array_equal(both, out, equal_nan=True)
    pipe = coreg.NuthKaab() + coreg.ICP()
    piped, t = pipe.fit_and_apply(ref, tba, inlier, transform=t6)
    assert t == t6 and pipe.is_affine and np.array_equal(pipe.to_matrix(), pipe.pipeline[1].to_matrix() @ pipe.pipeline[0].to_matrix())
    print("NMAD of dh before", before, "ICP", spread(out), "NuthKaab + ICP", spread(piped))
    assert spread(piped) < before   # (two resamplings and upstream's stop rule on |t1 + t2 + t3|: the pipeline need only improve)
    aligned = DEM(tba, t6).coregister_3d(DEM(ref, t6), coreg.ICP(), inlier_mask=inlier)
    assert aligned.transform == t6 and aligned.data.dtype == np.float32
    assert np.array_equal(aligned.data, out, equal_nan=True)
    sub = coreg.ICP(subsample=3000).fit(ref, tba, inlier, transform=t6, random_state=42)
    assert sub.meta["outputs"]["random"]["subsample_final"] == 3000
    assert spread(sub.apply(tba, transform=t6)[0]) < before
