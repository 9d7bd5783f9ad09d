"""GPU tests of the raster-in / raster-out kernels at the shapes where such kernels go wrong: a length-1 axis, odd FFT lengths,
rasters smaller than the filter or than one workgroup tile, shifts at and beyond the raster's extent or within 2^-40 of an
integer, a raster past 2^31 pixels.  Every case against the plain reference of the same operation in oracle/:
* texture shading (csrc/texture.hip)            vs terrain_oracle.texture_shading: scipy.fft in the DEM's dtype and in float64;
* NaN mean filter (csrc/meanfilter.hip)         vs patches_oracle.mean_filter_nan and scipy.ndimage.convolve itself, bit-exact;
* translation resample (xdemhip_shift_bilinear) vs nuthkaab_oracle.bilinear_shifted under every "nk_nan_rule", bit-exact;
* spatialstats.convolution (csrc/convolve.hip)  vs conv_oracle.convolution on images smaller than the filter, bit-exact."""
import math
import warnings

import numpy as np
import pytest

import conv_oracle as co
import nuthkaab_oracle as nko
import patches_oracle as po
import terrain_oracle as to
from conftest import decided

pytestmark = pytest.mark.gpu


def _ids(shape):
    return "x".join(str(s) for s in shape)


@pytest.fixture(scope="module")
def terrain():
    from xdem_amd import terrain as t

    return t


@pytest.fixture(scope="module")
def ss():
    from xdem_amd import spatialstats as s

    return s


@pytest.fixture(scope="module")
def coreg():
    from xdem_amd import coreg as c

    return c


# ---- 1. texture shading ------------------------------------------------------------------------------------------------------
# FFT lengths: powers of two up to 1024, the next 7-smooth integer above (1025 -> 1029 = 3 * 7^3, 1121 -> 1125, 1203 -> 1215,
# 2187 = 3^7, 2001 -> 2016, 1030 -> 1050).  Odd lengths exercise the fftfreq split of tex_filter_kernel and a C2R transform
# without a Nyquist column; a length-1 axis makes a 1 x N / N x 1 transform.
TEX_SHAPES = [(1, 1), (1, 2), (1, 7), (7, 1), (2, 3),   # degenerate
              (1, 1030), (1030, 1),                      # a length-1 axis beside a long one
              (3, 1025), (1025, 3), (1121, 517),         # one odd FFT axis
              (1029, 1203),                              # both FFT axes odd
              (513, 2187), (2001, 1025)]                 # mixed
TEX_ALPHAS = (0.0, 0.8, 2.0)
SMALL_ALPHA_SHAPES = ((3, 1025), (1121, 517))            # alpha = 1e-3 as well: a filter of ~1 but for the zeroed DC term
U32, U64 = 2.0**-24, 2.0**-53


def _terrain_like(shape, seed, holes=0.02):
    """Cumulative-sum terrain near 800 m (float64) with about `holes` of its pixels NaN; at least one pixel finite."""
    rng = np.random.default_rng(seed)
    dem = 800.0 + np.cumsum(np.cumsum(rng.normal(scale=0.3, size=shape), axis=0), axis=1)
    dem[rng.uniform(size=shape) < holes] = np.nan
    if not np.isfinite(dem).any():
        dem.flat[0] = 800.0
    return dem


def _tex_check(got, dem, alpha, work_dtype, record_property, label):
    """NaN mask bit for bit against the oracle, then the value bound, recorded as (e, bound, ratio).
    e(x) = max|x - ref64| / max|ref64| over the finite pixels, ref64 = the oracle on the DEM cast to float64.
    float32 work: e(got) <= 4 max(e(ref32), u32 S), ref32 = the oracle in float32 (the reference's own float32 error), S = max|filled
    DEM| / max|ref64| the cancellation factor, 4 the margin of the committed T10 bar (1e-5 against 2.5e-6 measured).
    float64 work: e(got) <= 1e-12 (the committed bar), widened to 4 u64 S log2(FH FW) only where cancellation makes 1e-12
    unreachable.  Evaluated as absolute errors (times max|ref64|), which keeps the bound defined where the output is all zero."""
    ref_w = to.texture_shading(dem.astype(work_dtype), alpha)
    ref64 = to.texture_shading(dem.astype(np.float64), alpha)
    assert np.array_equal(np.isnan(got), np.isnan(ref_w)), label
    assert np.array_equal(np.isnan(got), np.isnan(ref64)), label
    fin = np.isfinite(ref64)
    if not fin.any():
        return None
    d64 = dem.astype(np.float64)
    filled_max = float(np.abs(np.where(np.isfinite(d64), d64, np.nanmean(d64))).max())
    ref_max = float(np.abs(ref64[fin]).max())

    def err(x):
        return float(np.abs(x[fin].astype(np.float64) - ref64[fin]).max())

    g = err(got)
    if np.dtype(work_dtype) == np.float32:
        bound_abs = 4.0 * max(err(ref_w), U32 * filled_max)
    else:
        n_fft = to._next_fft_len(dem.shape[0]) * to._next_fft_len(dem.shape[1])
        bound_abs = max(1e-12 * ref_max, 4.0 * U64 * filled_max * math.log2(n_fft))
    e = g / ref_max if ref_max > 0 else (0.0 if g == 0 else math.inf)
    bound = bound_abs / ref_max if ref_max > 0 else bound_abs
    ratio = g / bound_abs if bound_abs > 0 else (0.0 if g == 0 else math.inf)
    record_property(label, f"e={e:.3e} bound={bound:.3e} ratio={ratio:.4f}")
    print(f"{label}: e={e:.3e} bound={bound:.3e} ratio={ratio:.4f}")
    assert g <= bound_abs, (label, e, bound)
    return ratio


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("shape", TEX_SHAPES, ids=_ids)
def test_texture_shading_shapes(terrain, record_property, shape, dtype):
    dem = _terrain_like(shape, seed=shape[0] * 7919 + shape[1]).astype(dtype)
    alphas = TEX_ALPHAS + ((1e-3,) if shape in SMALL_ALPHA_SHAPES else ())
    for alpha in alphas:
        got = terrain.texture_shading(dem, alpha=alpha)
        assert got.dtype == dtype and got.shape == shape
        _tex_check(got, dem, alpha, dtype, record_property, f"{_ids(shape)}|{np.dtype(dtype).name}|{alpha}")
        if shape == (1, 1):   # a length-1 transform is the identity: only the filter's DC factor (0 for alpha > 0, else 1) is left
            assert np.array_equal(got, np.zeros_like(dem) if alpha > 0 else dem), (alpha, got, dem)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("shape", [(1, 7), (7, 1), (2, 3), (3, 1025), (1025, 3), (1121, 517)], ids=_ids)
def test_texture_shading_special_inputs(terrain, record_property, shape, dtype):
    """A single finite pixel (it is the fill: the filled raster is constant); a +Inf pixel, which poisons the fill (np.nanmean skips
    NaN only) so that every output is NaN, as upstream; +Inf and -Inf together (a NaN fill); an all-NaN raster."""
    H, W = shape
    rng = np.random.default_rng(H * 31 + W)
    base = _terrain_like(shape, seed=H * 131 + W, holes=0.0)
    one = np.full(shape, np.nan, dtype=dtype)
    one[H // 2, W // 2] = base[H // 2, W // 2]
    pinf = base.astype(dtype)
    pinf[rng.uniform(size=shape) < 0.02] = np.nan
    pinf[0, W - 1] = np.inf
    both = pinf.copy()
    both[H - 1, 0] = -np.inf
    allnan = np.full(shape, np.nan, dtype=dtype)
    for alpha in TEX_ALPHAS:
        got = terrain.texture_shading(one, alpha=alpha)
        assert got.dtype == dtype and np.count_nonzero(np.isfinite(got)) == 1
        _tex_check(got, one, alpha, dtype, record_property, f"{_ids(shape)}|{np.dtype(dtype).name}|single|{alpha}")
        for name, d in (("+inf", pinf), ("+-inf", both), ("allnan", allnan)):
            got = terrain.texture_shading(d, alpha=alpha)
            assert got.dtype == dtype and np.isnan(got).all(), (name, alpha)
            _tex_check(got, d, alpha, dtype, record_property, f"{_ids(shape)}|{np.dtype(dtype).name}|{name}|{alpha}")


@pytest.mark.parametrize("shape", [(1, 7), (3, 1025), (1121, 517)], ids=_ids)
def test_texture_shading_integer_dem(terrain, record_property, shape):
    """An integer DEM is shaded as float32 (as upstream's caller converts it), into float32."""
    dem = np.round(_terrain_like(shape, seed=shape[1], holes=0.0)).astype(np.int32)
    for alpha in TEX_ALPHAS:
        got = terrain.texture_shading(dem, alpha=alpha)
        assert got.dtype == np.float32 and got.shape == shape
        _tex_check(got, dem, alpha, np.float32, record_property, f"{_ids(shape)}|int32|{alpha}")


@pytest.mark.parametrize("shape", [(1, 1), (1, 1030), (1030, 1), (3, 1025), (1121, 517), (1029, 1203)], ids=_ids)
def test_texture_shading_float32_in_float64_out(terrain, record_property, shape):
    """texture_typed<float, double>: float32 transforms, widened at the crop -- the float32 result exactly, in float64."""
    dem = _terrain_like(shape, seed=shape[0] + 3 * shape[1]).astype(np.float32)
    for alpha in TEX_ALPHAS:
        got = terrain.get_terrain_attribute(dem, "texture_shading", texture_alpha=alpha, out_dtype=np.float64)
        assert got.dtype == np.float64 and got.shape == shape
        same = terrain.texture_shading(dem, alpha=alpha)
        assert np.array_equal(got, same.astype(np.float64), equal_nan=True), alpha
        _tex_check(got, dem, alpha, np.float32, record_property, f"{_ids(shape)}|float32->float64|{alpha}")


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_texture_shading_is_repeatable(terrain, dtype):
    """The fill value (the DEM's nanmean) is a sum over ~2300 workgroups: the same bits on every call, and so is the output."""
    dem = _terrain_like((1121, 517), seed=77, holes=0.05).astype(dtype)
    first = terrain.texture_shading(dem, alpha=0.8)
    bits = np.uint32 if dtype == np.float32 else np.uint64
    for _ in range(2):
        again = terrain.texture_shading(dem, alpha=0.8)
        assert np.array_equal(again.view(bits), first.view(bits))


# ---- 2. NaN mean filter (patches method) ---------------------------------------------------------------------------------------
# rasters smaller than the kernel; H or W of 1; below one 64 x 16 tile; one past a multiple of 16 or 64
MF_SHAPES = [(1, 1), (1, 200), (200, 1), (5, 5), (12, 700), (17, 65), (31, 129), (130, 63)]
MF_KERNELS = [("square", p) for p in range(1, 12)] + [("circular", p) for p in range(1, 14)]   # every kernel the int8 count allows


def _mf_image(shape, dtype, seed):
    rng = np.random.default_rng(seed)
    img = (500.0 + np.cumsum(rng.normal(size=shape), axis=1)).astype(dtype)
    img[rng.uniform(size=shape) < 0.1] = np.nan
    if img.size >= 3:
        a, b = rng.choice(img.size, 2, replace=False)
        img.flat[a] = np.inf
        img.flat[b] = -np.inf
    return img


def _scipy_mean_filter(img, p, kernel_shape):
    """The reference's two scipy.ndimage.convolve(..., mode="constant", cval=nan) calls (xdem/spatialstats.py:2616-2650) on the
    zeroed image and on its int8 validity image, stored as float64, and their quotient -- without the reference's final squeeze."""
    from scipy import ndimage

    k = po.kernel_of(p, kernel_shape)
    fin = np.isfinite(img)
    zeroed = np.where(fin, img, 0).astype(img.dtype)
    valid = fin.astype(np.int8)
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        s = ndimage.convolve(zeroed, k, mode="constant", cval=np.nan).astype(np.float64)
        c = ndimage.convolve(valid, k, mode="constant", cval=np.nan).astype(np.float64)
        return s / c, c


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("shape", MF_SHAPES, ids=_ids)
def test_mean_filter_nan_shapes(ss, shape, dtype):
    img = _mf_image(shape, dtype, seed=shape[0] * 1000 + shape[1])
    allnan = np.full(shape, np.nan, dtype=dtype)
    small = min(shape) < 13   # narrower than the largest kernel: compared with SciPy itself as well
    for kernel_shape, p in MF_KERNELS:
        for name, x in (("terrain", img), ("allnan", allnan)):
            mean, valid, npx = ss.mean_filter_nan(x, p, kernel_shape)
            m0, v0, n0 = po.mean_filter_nan(x, p, kernel_shape)
            assert mean.shape == valid.shape == shape and mean.dtype == valid.dtype == np.float64
            assert npx == n0, (name, kernel_shape, p)
            assert np.array_equal(valid, v0), (name, kernel_shape, p)
            assert np.array_equal(mean, m0, equal_nan=True), (name, kernel_shape, p)
            if small:
                m1, v1 = _scipy_mean_filter(x, p, kernel_shape)
                assert np.array_equal(valid, v1) and np.array_equal(mean, m1, equal_nan=True), (name, kernel_shape, p)
    for kernel_shape, p in (("square", 12), ("circular", 14)):
        with pytest.raises(NotImplementedError, match="int8"):
            ss.mean_filter_nan(img, p, kernel_shape)


# ---- 3. translation resample -----------------------------------------------------------------------------------------------------
RS_SHAPES = [(1, 1), (1, 9), (9, 1), (2, 2), (3, 517), (257, 1)]


def _axis_shifts(n):
    """Pixel shifts along an axis of extent n: zero of both signs, whole and half pixels, to the last pixel, the extent and
    beyond it, within 2^-40 of zero and the largest float64 below one."""
    return [0.0, -0.0, 1.0, -1.0, 0.5, -0.5, n - 1.0, -(n - 1.0), float(n), -float(n), 10.0 * n, -10.0 * n,
            2.0**-40, -(2.0**-40), 1.0 - 2.0**-52]


def _rs_image(shape, dtype):
    rng = np.random.default_rng(shape[0] * 100 + shape[1])
    img = (300.0 + np.cumsum(rng.normal(scale=2.0, size=shape[0] * shape[1]))).reshape(shape).astype(dtype)
    if img.size >= 9:
        img.flat[img.size // 2] = np.nan
    if img.size >= 100:
        img.flat[img.size // 3] = np.inf
    return img


@pytest.mark.parametrize("rule", [0, 1, 2, 3])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("shape", RS_SHAPES, ids=_ids)
def test_translation_resample_shapes_and_shifts(coreg, shape, dtype, rule):
    """Every row shift with every column shift (each alone where the other is 0), shift_z = 0.1 (not exact in float32):
    bit-exact against the oracle; a shift of at least the extent leaves every pixel NaN; rule 1 at a zero shift is the identity."""
    ctx = coreg._lib.default_context()
    img = _rs_image(shape, dtype)
    H, W = shape
    try:
        ctx.set_option("nk_nan_rule", rule)
        for dr in _axis_shifts(H):
            for dc in _axis_shifts(W):
                got = coreg.apply_translation(img, -dc, dr, 0.1, 1.0)   # position (row + shift_y, col - shift_x) / res
                want = nko.bilinear_shifted(img, dr, dc, nan_rule=rule) + img.dtype.type(0.1)
                assert got.dtype == img.dtype and got.shape == shape
                assert np.array_equal(got, want, equal_nan=True), (dr, dc)
                if abs(dr) >= H or abs(dc) >= W:
                    assert np.isnan(got).all(), (dr, dc)
        if rule == 1:   # (a +-Inf pixel is nodata under every rule: it comes back NaN)
            same = np.where(np.isfinite(img), img, np.nan)
            for z in (0.0, -0.0):
                assert np.array_equal(coreg.apply_translation(img, z, z, 0.0, 1.0), same, equal_nan=True), z
    finally:
        ctx.set_option("nk_nan_rule", decided("nk_nan_rule"))


def test_translation_resample_past_2g_pixels(coreg):
    """46341 x 46341 float32 raster: 2 147 488 281 pixels > 2^31, pixel 2^31 in the last row -- the float64 row / column split of
    the linear index and the int64 grid-stride loop.  Shift (0.3, -1.7) px in x and y (taps 1.7 rows above and 0.3 columns left
    of each pixel): the first and last 4 rows and 8 seeded rows against the oracle on a slab of +-4 rows around them, tap
    positions formed from the raster row as the kernel forms them (row_offset); only rows at least 3 rows from a slab edge that
    is not a raster edge are compared.  About 8.6 GB of host memory for each of input and output."""
    n = 46341
    assert n * n > 2**31 and 2**31 // n == n - 1
    rng = np.random.default_rng(2031)
    picks = sorted({int(r) for r in rng.integers(4, n - 4, 8)})
    col = (400.0 + np.cumsum(rng.normal(scale=0.5, size=n))).astype(np.float32)
    row = (50.0 * np.sin(np.arange(n) * 1e-3)).astype(np.float32)
    img = np.empty((n, n), dtype=np.float32)
    for r0 in range(0, n, 4096):
        np.add(row[r0:r0 + 4096, None], col[None, :], out=img[r0:r0 + 4096])
    compared = list(range(4)) + list(range(n - 4, n)) + picks
    for r in compared:   # holes in the rows the compared rows read
        for rr in (r - 2, r - 1):
            if rr >= 0:
                img[rr, rng.integers(0, n, 30)] = np.nan
    shift_x, shift_y, dz = 0.3, -1.7, 0.1
    dr, dc = shift_y, -shift_x
    rule = decided("nk_nan_rule")
    out = coreg.apply_translation(img, shift_x, shift_y, dz, 1.0)
    slabs = [(0, 8, range(0, 4)), (n - 8, n, range(n - 4, n))] + [(r - 4, r + 5, (r,)) for r in picks]
    for a, b, rows in slabs:
        want = nko.bilinear_shifted(img[a:b], dr, dc, nan_rule=rule, row_offset=a) + np.float32(dz)
        for r in rows:
            assert np.array_equal(out[r], want[r - a], equal_nan=True), r
            if r >= 2:   # (rows 0 and 1 read above the raster: NaN)
                assert np.count_nonzero(np.isfinite(out[r])) > n // 2, r


# ---- 4. convolution on images smaller than the filter ----------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("ishape", [(1, 1, 1), (1, 1, 200), (1, 200, 1), (1, 2, 2)], ids=_ids)
def test_convolution_images_smaller_than_the_filter(ss, ishape, dtype):
    """3 x 3, 5 x 5, 7 x 7 (the register-window kernels) and 21 x 35 (the tap-list kernel), both engines, one NaN pixel.  Besides
    a dense and a half-zero filter, one with only its middle row and one with only its middle column non-zero: the SciPy engine
    skips zero weights, so those reach no tap beyond the border of a 1 x N / N x 1 image and give finite sums."""
    rng = np.random.default_rng(sum(ishape) + 7)
    imgs = (50.0 + np.cumsum(rng.normal(size=ishape), axis=-1)).astype(dtype)
    if imgs.size > 1:
        imgs.flat[imgs.size // 2] = np.nan
    for fshape in ((3, 3), (5, 5), (7, 7), (21, 35)):
        m1, m2 = fshape
        filters = rng.normal(size=(4,) + fshape)
        filters[1][rng.uniform(size=fshape) < 0.5] = 0.0
        filters[2][np.arange(m1) != m1 // 2] = 0.0
        filters[3][:, np.arange(m2) != m2 // 2] = 0.0
        for method in ("scipy", "numba"):
            got = ss.convolution(imgs, filters, method=method)
            want = co.convolution(imgs, filters, method)
            assert got.dtype == np.float64 and got.shape == want.shape == (1, 4) + ishape[1:]
            assert np.array_equal(got, want, equal_nan=True), (fshape, method)
