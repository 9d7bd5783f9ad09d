"""Every route of the two grid passes behind Deramp (csrc/biascorr.hip) against tests/deramp_oracle.py:

  * the least-squares moments -- dh_moments_rows_kernel<T, K, VEC> and dh_moments_list_kernel<T, K>, then fixed_sums_reduce_kernel --
    against longdouble sums within the derived bound of deramp_oracle.moments_bound, the count moment exactly;
  * the polynomial apply -- poly2d_apply_kernel<T, K> and poly2d_apply_vec_kernel<T, K> -- against NumPy's polyval2d bit for bit;
  * the valid counts and the values route -- dh_valid_kernel<T, WRITE_MASK, VEC> -- at the edges of its 4096-pixel tiles, bit for bit.

Which shape reaches which route (W % 4 == 0 and 16-byte aligned rasters take the four-wide "VEC" forms; CU = the device's compute
units, every threshold asserted where it is used):
  moments  37 x 61 scalar, 40 x 64 VEC: one trip of every loop; 5 x 259, 3 x 515: the scalar column loop wraps once / twice (W > 256);
           6 x 1028: the VEC column loop wraps for lane 0 alone (W > 1024); (8 CU + 37) x 8 VEC and x 7 scalar: 37 workgroups own two
           rows, and the reduce lanes add ceil(8 CU / 256) > 1 partials; 1 x 64, 64 x 1, 1 x 1: a half-width of 0;
           a contiguous CUDA view one element (mask: one byte) into its buffer: 40 x 64 on the scalar forms;
           list route: k = 1, 255, 256, 257, 1000 drawn pixels (a partial tile, a full one, a second workgroup), and k > 1024 CU, where a
           workgroup walks two 256-pixel tiles.
  apply    33 x 61 scalar, 33 x 64 VEC; (G + 5) x 8 and (2 G + 3) x 8 with G = ceil(8 CU / gx) rows of workgroups: the two-rows-per-step
           body with some rows paired and some not, then a second trip; the same heights x 7: the scalar row loop; 3 x (64 * 256 + 9):
           the scalar column loop (gx capped at 64); 2 x 1028: VEC with gx = 2; misaligned elev or out: 33 x 64 on the scalar kernel.
Every case prints its largest error / bound; on an MI355X (256 CUs) the largest of all was 0.044 (list route, k = 256), the rows route
stayed below 0.04.  The rasters carry a tenth of pixels whose float32 difference is a rounded one (deramp_oracle.make_pair): dh formed in
float64 instead of the raster dtype fails these tests."""
import functools
import math

import numpy as np
import pytest

import deramp_oracle as do

pytestmark = pytest.mark.gpu

LD = np.longdouble
DTYPES = ("float32", "float64")
ALL_ORDERS = (0, 1, 2, 3, 4, 5)
SOME_ORDERS = (0, 2, 5)


@functools.lru_cache(maxsize=None)
def _num_cu() -> int:
    import torch

    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _frozen(*arrays):
    for a in arrays:
        if a is not None:
            a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def _rasters(H, W, dtype, masked, nan_frac=0.03):
    """(ref, tba, inlier or None) of a case, made once and read-only."""
    return _frozen(*do.make_pair(H, W, np.dtype(dtype), seed=H * 7919 + W, nan_frac=nan_frac, masked=masked))


@functools.lru_cache(maxsize=None)
def _pair(H, W, dtype, masked, nan_frac=0.03):
    """(ref, tba, inlier or None, the oracle's moments of order 5 over all valid pixels), computed once."""
    ref, tba, inl = _rasters(H, W, dtype, masked, nan_frac)
    return ref, tba, inl, do.moments(ref, tba, inl, do.MAX_ORDER)


def _check(got, want, additions, label):
    """count, the count moment and every entry of (M, R) against the oracle; returns and prints the largest error / bound."""
    M, R, cnt = got
    assert cnt == want.count, (label, cnt, want.count)
    assert M[0, 0] == cnt, (label, M[0, 0], cnt)
    assert M.shape == want.M.shape and R.shape == want.R.shape
    bM, bR = do.moments_bound(want, additions)
    assert bM[0, 0] < 0.5
    eM, eR = np.abs(M.astype(LD) - want.M).astype(np.float64), np.abs(R.astype(LD) - want.R).astype(np.float64)
    ratio = max(float(np.max(eM / bM)), float(np.max(eR / bR)))
    print(f"{label}: additions {additions}, largest error / bound {ratio:.4f}")
    assert np.all(np.isfinite(M)) and np.all(np.isfinite(R)) and np.all(eM <= bM) and np.all(eR <= bR), (label, ratio)
    return ratio


def _orders_of(H, W):
    return ALL_ORDERS if (H, W) in ((37, 61), (40, 64)) else SOME_ORDERS


def _shape_params():
    """The rows-route shapes by name: the tall ones depend on the device, so they are resolved inside the test."""
    return ["37x61", "40x64", "5x259", "3x515", "6x1028", "tallx8", "tallx7", "1x64", "64x1", "1x1"]


def _resolve(name):
    shapes = dict(zip(_shape_params(), do.moments_shapes(_num_cu())))
    return shapes[name]


# ---- 2. moments ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", _shape_params())
def test_moments_rows_route(name, dtype, masked):
    """dh_moments_rows_kernel on every shape of deramp_oracle.moments_shapes, from host arrays (aligned uploads): VEC where W % 4 == 0."""
    from xdem_amd.biascorr import DhPlan

    cu = _num_cu()
    H, W, vec = _resolve(name)
    assert vec == (W % 4 == 0)
    nb = do.rows_grid(H, cu)
    # the conditions under which the shape reaches its route
    if name in ("5x259", "3x515"):
        assert not vec and math.ceil(W / 256) == {"5x259": 2, "3x515": 3}[name]
    if name == "6x1028":
        assert vec and 1024 < W <= 1024 + 4          # (a second trip for lane 0 alone)
    if name.startswith("tall"):
        assert 8 * cu < H < 16 * cu and nb == 8 * cu and nb > 256 and math.ceil(nb / 256) > 1
    if name in ("37x61", "40x64"):
        assert H <= 8 * cu and W <= 256
    ref, tba, inl, want5 = _pair(H, W, dtype, masked)
    if dtype == "float32" and H * W >= 64:   # (the data tells a float32 difference from a float64 one)
        v = do.valid_mask(ref, tba, inl)
        assert np.any(ref[v].astype(np.float64) - tba[v].astype(np.float64) != (ref[v] - tba[v]).astype(np.float64))
    with DhPlan(ref, tba, inl) as plan:
        assert plan.n_valid == want5.count
        for order in _orders_of(H, W):
            _check(plan.poly_moments(order), do.sub(want5, order), do.additions_rows(H, W, vec, cu),
                   f"rows {name} {dtype} mask={masked} order {order}")


def _poisoned(H, W, dtype, which, masked):
    """A pair with NaN, +inf and -inf in ``which`` alone: one in each of the four positions of a four-wide group, in the first and the last
    group of a row, and at the last pixel of the raster."""
    ref, tba, inl = do.make_pair(H, W, np.dtype(dtype), seed=31 + H, nan_frac=0.0, masked=masked)
    if inl is not None:
        inl[:] = True
        inl[4, :] = False
        inl[20, 1::2] = False
    target = ref if which == "ref" else tba
    bad = (np.nan, np.inf, -np.inf)
    spots = [(3, 8), (5, 13), (7, 18), (9, 23), (6, 0), (8, 1), (10, 2), (12, 3),
             (11, W - 4), (13, W - 3), (15, W - 2), (17, W - 1), (H - 1, W - 1), (H - 1, W - 2), (20, 4), (20, 5)]
    assert sorted({c % 4 for _, c in spots[:8]}) == [0, 1, 2, 3]
    for i, (r, c) in enumerate(spots):
        target[r, c] = bad[i % 3]
    return ref, tba, inl, spots


@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("which", ["ref", "tba"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(37, 61), (40, 64)], ids=["scalar", "vec"])
def test_moments_skip_non_finite_pixels(shape, dtype, which, masked):
    """NaN, +inf and -inf in one raster alone, at every position of a four-wide group, in the last group of a row and at the last pixel."""
    from xdem_amd.biascorr import DhPlan

    H, W = shape
    ref, tba, inl, spots = _poisoned(H, W, dtype, which, masked)
    want5 = do.moments(ref, tba, inl, do.MAX_ORDER)
    valid = do.valid_mask(ref, tba, inl)
    other = tba if which == "ref" else ref
    assert want5.count == int(valid.sum()) and not any(valid[r, c] for r, c in spots) and np.all(np.isfinite(other))
    if inl is None:
        assert want5.count == H * W - len(spots)
    with DhPlan(ref, tba, inl) as plan:
        assert plan.n_valid == want5.count
        for order in SOME_ORDERS:
            _check(plan.poly_moments(order), do.sub(want5, order), do.additions_rows(H, W, W % 4 == 0, _num_cu()),
                   f"non-finite in {which} {H}x{W} {dtype} mask={masked} order {order}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(37, 61), (40, 64)], ids=["scalar", "vec"])
def test_moments_keep_a_pixel_whose_difference_overflows(shape, dtype):
    """ref = 0.9 max and tba = -0.9 max are both finite: moments_pixel tests the inputs, not the difference, so the pixel counts, its
    dh is +inf and every R[i, j] is the infinity of the sign of u^i v^j there (the pixel is off both centre lines: no 0 * inf).  The
    oracle does the same.  M is untouched and stays within its bound."""
    from xdem_amd.biascorr import DhPlan

    H, W = shape
    ref, tba, _ = do.make_pair(H, W, np.dtype(dtype), seed=5, nan_frac=0.0)
    big = 0.9 * np.finfo(np.dtype(dtype)).max
    ref[2, 5], tba[2, 5] = big, -big
    with np.errstate(over="ignore"):
        assert np.isposinf(ref[2, 5] - tba[2, 5])
    order = 3
    want = do.moments(ref, tba, None, order)
    assert want.count == H * W and np.all(np.isinf(want.R))
    with DhPlan(ref, tba) as plan:
        M, R, cnt = plan.poly_moments(order)
    assert cnt == plan.n_valid == H * W and M[0, 0] == cnt
    bM, _ = do.moments_bound(want, do.additions_rows(H, W, W % 4 == 0, _num_cu()))
    eM = np.abs(M.astype(LD) - want.M).astype(np.float64)
    print(f"overflow {H}x{W} {dtype}: largest error / bound of M {float(np.max(eM / bM)):.4f}")
    assert np.all(eM <= bM)
    assert np.array_equal(R, want.R.astype(np.float64))     # (+-inf, the same signs)
    signs = np.sign(np.array([[(-1.0) ** (i + j) for j in range(order + 1)] for i in range(order + 1)]))
    assert np.array_equal(np.sign(R), signs)                # (u < 0 and v < 0 at (2, 5))


@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(37, 61), (40, 64)], ids=["scalar", "vec"])
def test_moments_of_a_row_block_in_global_coordinates(shape, dtype, masked):
    """A plan of rows [r0, r1) with row_offset = r0 and H_global = H against the oracle over the whole raster with the other rows masked
    out: the oracle never sees an offset."""
    from xdem_amd.biascorr import DhPlan

    H, W = shape
    r0, r1 = 11, 29
    assert 0 < r0 < r1 < H
    ref, tba, inl, _ = _pair(H, W, dtype, masked)
    rows_only = np.zeros((H, W), dtype=bool)
    rows_only[r0:r1] = True if inl is None else inl[r0:r1]
    want5 = do.moments(ref, tba, rows_only, do.MAX_ORDER)
    with DhPlan(ref[r0:r1], tba[r0:r1], None if inl is None else inl[r0:r1]) as plan:
        for order in SOME_ORDERS:
            _check(plan.poly_moments(order, row_offset=r0, H_global=H), do.sub(want5, order),
                   do.additions_rows(r1 - r0, W, W % 4 == 0, _num_cu()), f"rows [{r0}, {r1}) of {H}x{W} {dtype} mask={masked} order {order}")


def _offset_view(a, torch):
    """A contiguous CUDA copy of ``a`` that starts one element into its buffer: 4 or 8 bytes off a 16-byte boundary, a mask 1 byte."""
    buf = torch.empty(a.size + 1, dtype=torch.from_numpy(np.empty(0, a.dtype)).dtype, device="cuda")
    view = buf[1:].view(*a.shape)
    view.copy_(torch.from_numpy(np.array(a)))
    assert view.is_contiguous() and view.data_ptr() % 16 == a.itemsize % 16 and view.data_ptr() == buf.data_ptr() + a.itemsize
    return view


def _device_inputs(ref, tba, inl, how, torch):
    """CUDA tensors of a case: ``how`` names what is misaligned ("all", "mask", "tba", or "none")."""
    def put(a, off):
        return _offset_view(a, torch) if off else torch.from_numpy(np.array(a)).cuda()

    m = None if inl is None else put(inl.astype(np.uint8), how in ("all", "mask"))
    return put(ref, how == "all"), put(tba, how in ("all", "tba")), m


@pytest.mark.parametrize("how", ["all", "mask", "tba"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_moments_of_misaligned_device_views(dtype, how):
    """40 x 64 would take the four-wide forms; a view one element (the mask: one byte) into its buffer passes raster_pair and must take
    the scalar forms of dh_valid_kernel and dh_moments_rows_kernel: the oracle's moments, the aligned plan's count."""
    import torch

    from xdem_amd.biascorr import DhPlan

    H, W = 40, 64
    ref, tba, inl, want5 = _pair(H, W, dtype, True)
    with DhPlan(ref, tba, inl) as aligned:
        n_aligned = aligned.n_valid
    dref, dtba, dinl = _device_inputs(ref, tba, inl, how, torch)
    if how in ("all", "mask"):
        assert dinl.data_ptr() % 4 == 1
    assert (dref.data_ptr() % 16 != 0) == (how == "all") and (dtba.data_ptr() % 16 != 0) == (how in ("all", "tba"))
    with DhPlan(dref, dtba, dinl) as plan:
        assert plan.n_valid == n_aligned == want5.count
        for order in SOME_ORDERS:
            _check(plan.poly_moments(order), do.sub(want5, order), do.additions_rows(H, W, False, _num_cu()),
                   f"misaligned ({how}) {H}x{W} {dtype} order {order}")
    # the aligned device tensors: the four-wide forms over device memory the plan does not own
    dref, dtba, dinl = _device_inputs(ref, tba, inl, "none", torch)
    with DhPlan(dref, dtba, dinl) as plan:
        assert plan.n_valid == n_aligned
        _check(plan.poly_moments(5), want5, do.additions_rows(H, W, True, _num_cu()), f"aligned device {H}x{W} {dtype} order 5")


def _ranks(n_valid, k, seed):
    """k distinct ranks in random order and a few of them again."""
    rng = np.random.default_rng(seed)
    ranks = rng.choice(n_valid, size=k, replace=False)
    again = ranks[: min(3, k)] if k + 3 <= n_valid else ranks[:0]
    return np.concatenate([ranks, again, again[:1]]).astype(np.int64)


@pytest.mark.parametrize("k", do.LIST_SMALL_K)
@pytest.mark.parametrize("dtype", DTYPES)
def test_moments_list_route(dtype, k):
    """dh_moments_list_kernel over k drawn pixels of a 64 x 80 raster with about 5 % NaN: one workgroup with a padded tile (1, 255), a full
    tile (256), a second workgroup (257) and four (1000); repeated ranks count once."""
    from xdem_amd.biascorr import DhPlan

    H, W = 64, 80
    ref, tba, inl, whole = _pair(H, W, dtype, False, 0.025)   # (2.5 % of each raster: about 5 % of the pixels)
    assert 0.03 < 1 - whole.count / (H * W) < 0.07
    ranks = _ranks(whole.count, k, seed=k)
    assert ranks.size > k and np.unique(ranks).size == k
    want5 = do.moments(ref, tba, inl, do.MAX_ORDER, ranks=ranks)
    per, nb = do.list_grid(k, _num_cu())
    assert per == 256 and nb == math.ceil(k / 256)
    with DhPlan(ref, tba, inl) as plan:
        assert plan.subsample(ranks) == k == want5.count
        for order in SOME_ORDERS:
            _check(plan.poly_moments(order), do.sub(want5, order), do.additions_list(k, _num_cu()), f"list k={k} {dtype} order {order}")


def test_moments_list_route_walks_several_tiles_per_workgroup():
    """k > 1024 CUs drawn pixels: ``per`` exceeds 256, so a workgroup adds several tiles into one accumulator, and the last one is partial."""
    from xdem_amd.biascorr import DhPlan

    cu = _num_cu()
    side, k = do.list_large_case(cu)
    per, nb = do.list_grid(k, cu)
    assert k > 1024 * cu and per > 256 and per % 256 == 0 and nb <= 4 * cu and (nb - 1) * per < k <= nb * per
    ref, tba, inl = _rasters(side, side, "float32", False, 0.0025)
    n_valid = int(do.valid_mask(ref, tba, inl).sum())
    assert k + 3 <= n_valid < side * side
    ranks = _ranks(n_valid, k, seed=1)
    want5 = do.moments(ref, tba, inl, do.MAX_ORDER, ranks=ranks)
    with DhPlan(ref, tba, inl) as plan:
        assert plan.subsample(ranks) == k == want5.count
        for order in SOME_ORDERS:
            _check(plan.poly_moments(order), do.sub(want5, order), do.additions_list(k, cu), f"list k={k} ({side}x{side}, per={per}) order {order}")


@pytest.mark.parametrize("order", [0, 4, 5])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(37, 61), (40, 64)], ids=["scalar", "vec"])
def test_deramp_fit_matches_lstsq(shape, dtype, order):
    """The whole fit against the unit-norm-column least squares of tests/test_biascorr_host.py, with its criterion."""
    from xdem_amd import coreg
    from xdem_amd.biascorr import polynomial_2d

    H, W = shape
    ref, tba, inl = do.make_pair(H, W, np.dtype(dtype), seed=order, masked=True, outliers=0.0)   # (a surface of a few metres)
    d = coreg.Deramp(poly_order=order, subsample=1).fit(ref, tba, inlier_mask=inl)
    params = d.meta["outputs"]["fitorbin"]["fit_params"]
    valid = do.valid_mask(ref, tba, inl)
    assert d.meta["outputs"]["random"]["subsample_final"] == int(valid.sum())
    y, x = np.nonzero(valid)
    dh = (ref[valid] - tba[valid]).astype(np.float64)
    A = np.stack([x.astype(float) ** i * y.astype(float) ** j for i in range(order + 1) for j in range(order + 1)], 1)
    scale = np.linalg.norm(A, axis=0)
    lst = np.linalg.lstsq(A / scale, dh, rcond=None)[0] / scale
    mine = polynomial_2d((x, y), *params)
    gap, lim = float(np.max(np.abs(mine - polynomial_2d((x, y), *lst)))), 1e-8 * (1 + float(np.max(np.abs(mine))))
    print(f"fit {H}x{W} {dtype} order {order}: surface gap {gap:.3e}, limit {lim:.3e}")
    assert gap <= lim


# ---- 3. polynomial apply ----------------------------------------------------------------------------------------------------------
def _apply_grid(H, W, vec, cu):
    """(gx, G, gy) as launch_apply computes them: G rows of workgroups before the caps at H and 65535."""
    gx = math.ceil(W / 1024) if vec else min(math.ceil(W / 256), 64)
    G = math.ceil(8 * cu / gx)
    return gx, G, max(1, min(G, H, 65535))


def _apply_shape(name, cu):
    G = math.ceil(8 * cu / 1)
    return {"33x61": (33, 61), "33x64": (33, 64), "G+5x8": (G + 5, 8), "2G+3x8": (2 * G + 3, 8), "G+5x7": (G + 5, 7),
            "2G+3x7": (2 * G + 3, 7), "3xwide": (3, 64 * 256 + 9), "2x1028": (2, 1028)}[name]


def _coeffs(order, seed=0):
    rng = np.random.default_rng(100 + order + seed)
    K = order + 1
    return np.array([rng.normal() * 10.0 ** (-2 * (i + j)) for i in range(K) for j in range(K)])


@functools.lru_cache(maxsize=None)
def _elev(H, W, dtype):
    rng = np.random.default_rng(H + 3 * W)
    e = (1000.0 + 50.0 * rng.normal(size=(H, W))).astype(np.dtype(dtype))
    n = H * W
    flat = e.reshape(-1)
    for i, p in enumerate(sorted({0, n - 1, n // 2, W - 1, min(n - 1, W), 5 % n, 6 % n, 7 % n, (n - 2) % n, (n // 3) % n})):
        if n > 4 or i == 0:
            flat[p] = (np.nan, np.inf, -np.inf)[i % 3]
    return _frozen(e)[0]


@functools.lru_cache(maxsize=None)
def _apply_want(H, W, dtype, order, row_offset):
    return _frozen(do.apply(_elev(H, W, dtype), _coeffs(order), row_offset))[0]


@pytest.mark.parametrize("row_offset", [0, 1000])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["33x61", "33x64", "G+5x8", "2G+3x8", "G+5x7", "2G+3x7", "3xwide", "2x1028"])
def test_apply_matches_numpy_bit_for_bit(name, dtype, row_offset):
    """poly2d_apply from host arrays (aligned uploads: VEC where W % 4 == 0) against deramp_oracle.apply with the same row offset."""
    from xdem_amd.biascorr import poly2d_apply

    cu = _num_cu()
    H, W = _apply_shape(name, cu)
    vec = W % 4 == 0
    gx, G, gy = _apply_grid(H, W, vec, cu)
    if name in ("G+5x8", "G+5x7"):
        assert gx == 1 and gy == G < H < 2 * G                    # (rows 0..4 have a partner G rows on, the others none)
    if name in ("2G+3x8", "2G+3x7"):
        assert gx == 1 and gy == G and 2 * G < H < 3 * G            # (every row paired, then a second trip of three single rows)
    if name == "3xwide":
        assert not vec and math.ceil(W / 256) > gx == 64           # (the column loop wraps)
    if name == "2x1028":
        assert vec and gx == 2 and gy == H
    if name in ("33x61", "33x64"):
        assert gx == 1 and gy == H
    elev = _elev(H, W, dtype)
    assert np.isnan(elev).any() and np.isposinf(elev).any() and np.isneginf(elev).any()
    for order in (ALL_ORDERS if name in ("33x61", "33x64") else SOME_ORDERS):
        want = _apply_want(H, W, dtype, order, row_offset)
        got = poly2d_apply(elev, _coeffs(order), row_offset=row_offset)
        assert got.dtype == elev.dtype and np.array_equal(got, want, equal_nan=True), (name, dtype, order, row_offset)
        # the polynomial is no rounding-sized nudge: it moves most pixels
        assert np.mean(want != elev) > 0.5
    print(f"apply {name} = {H}x{W} {dtype} row_offset {row_offset}: gx {gx}, G {G}, gy {gy}, {'VEC' if vec else 'scalar'}: bit for bit")


@pytest.mark.parametrize("dtype", DTYPES)
def test_apply_on_misaligned_device_tensors(dtype):
    """33 x 64 on the device: aligned (VEC), elev one element into its buffer, an aligned elev with a misaligned out (both scalar); out
    given and not given: NumPy's bits every time."""
    import torch

    from xdem_amd.biascorr import poly2d_apply

    H, W = 33, 64
    elev = _elev(H, W, dtype)
    aligned = torch.from_numpy(np.array(elev)).cuda()
    assert aligned.data_ptr() % 16 == 0
    shifted = _offset_view(elev, torch)
    for order in ALL_ORDERS:
        for row_offset in (0, 1000):
            want = _apply_want(H, W, dtype, order, row_offset)
            c = _coeffs(order)
            base = poly2d_apply(aligned, c, row_offset=row_offset)
            assert base.data_ptr() % 16 == 0 and np.array_equal(base.cpu().numpy(), want, equal_nan=True)
            out = torch.empty_like(aligned)
            assert poly2d_apply(aligned, c, row_offset=row_offset, out=out) is out and np.array_equal(out.cpu().numpy(), want, equal_nan=True)
            got = poly2d_apply(shifted, c, row_offset=row_offset)
            assert np.array_equal(got.cpu().numpy(), want, equal_nan=True), ("misaligned elev", order, row_offset)
            off_out = _offset_view(np.zeros((H, W), dtype=elev.dtype), torch)
            assert off_out.data_ptr() % 16 != 0
            assert poly2d_apply(aligned, c, row_offset=row_offset, out=off_out) is off_out
            assert np.array_equal(off_out.cpu().numpy(), want, equal_nan=True), ("misaligned out", order, row_offset)
            assert poly2d_apply(shifted, c, row_offset=row_offset, out=off_out) is off_out
            assert np.array_equal(off_out.cpu().numpy(), want, equal_nan=True), ("both misaligned", order, row_offset)


# ---- 4. valid counts and the values route at the tile edges ----------------------------------------------------------------------
TILE_EDGE_N = (1, 3, 4, 5, 1023, 1024, 1025, 4095, 4096, 4097, 8193)


def _row_case(n, dtype, masked):
    rng = np.random.default_rng(n)
    ref = (1000.0 + 50.0 * rng.normal(size=(1, n))).astype(np.dtype(dtype))
    tba = (ref - 2.0 + rng.normal(size=(1, n))).astype(np.dtype(dtype))
    tba[0, rng.random(n) < 0.2] *= 0.37   # (another binade: a float32 difference that rounds)
    for a, bad in ((ref, np.nan), (tba, np.inf), (ref, -np.inf)):
        a[0, rng.random(n) < 0.04] = bad
    inl = (rng.random((1, n)) >= 0.15) if masked else None
    if n >= 5:   # the last pixel and the last group: once invalid, once valid, by the parity of n
        ref[0, n - 1] = np.nan if n % 2 else 1001.0
        tba[0, n - 1] = 999.5
        ref[0, n - 3], tba[0, n - 3] = 1002.0, (np.inf if n % 2 == 0 else 1000.25)
        if inl is not None:
            inl[0, n - 1] = inl[0, n - 3] = True
            inl[0, n - 2] = False
    ref[0, 0], tba[0, 0] = 1003.25, 1001.5
    if inl is not None:
        inl[0, 0] = True
    return ref, tba, inl


@pytest.mark.parametrize("how", ["host", "all", "one"])
@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_valid_counts_values_and_median_at_tile_edges(dtype, masked, how):
    """Single rows of n pixels around the 4-pixel groups, the 1024-pixel strides and the 4096-pixel tiles of dh_valid_kernel, from
    aligned host arrays (VEC) and from misaligned device views (scalar): the count, the values route and the median, bit for bit."""
    import torch

    from xdem_amd.biascorr import DhPlan

    if how == "one":   # (one input alone off its boundary: the mask where there is one, a raster otherwise)
        how = "mask" if masked else "tba"
    parities = set()
    for n in TILE_EDGE_N:
        ref, tba, inl = _row_case(n, dtype, masked)
        flat = np.flatnonzero(do.valid_mask(ref, tba, inl).ravel())
        row, col = np.divmod(flat, n)
        with np.errstate(invalid="ignore", over="ignore"):
            dh = (ref - tba).ravel()[flat]
        assert flat.size >= 1 and np.all(np.isfinite(dh))
        parities.add(flat.size % 2)
        args = (ref, tba, inl) if how == "host" else _device_inputs(ref, tba, inl, how, torch)
        with DhPlan(*args) as plan:
            assert plan.n_valid == flat.size, (n, plan.n_valid, flat.size)
            med = plan.median()
            g_dh, g_col, g_row = plan.values()
            assert plan.median() == med
        assert g_dh.dtype == dh.dtype and np.array_equal(g_dh, dh) and np.array_equal(g_col, col) and np.array_equal(g_row, row), n
        assert med == (float(np.median(dh)), flat.size), (n, med)
    assert parities == {0, 1}
