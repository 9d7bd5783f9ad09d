"""Synthetic inputs for tests and benchmarks: fractional-Brownian DEMs by spectral synthesis."""
from __future__ import annotations

import math

import numpy as np


def fbm_numpy(shape, hurst: float = 0.7, seed: int = 42, mean: float = 1000.0, std: float = 300.0,
              dtype=np.float32) -> np.ndarray:
    """Periodic fBm surface: white noise x |k|^-(H+1) in the Fourier domain, rescaled to (mean, std)."""
    n, m = shape
    rng = np.random.default_rng(seed)
    f = np.fft.rfft2(rng.normal(size=(n, m)))
    ky = np.fft.fftfreq(n)[:, None]
    kx = np.fft.rfftfreq(m)[None, :]
    k = np.sqrt(kx**2 + ky**2)
    k[0, 0] = 1.0
    z = np.fft.irfft2(f * k ** (-(hurst + 1.0)), s=(n, m))
    z = (z - z.mean()) / z.std()
    return (mean + std * z).astype(dtype)


def fbm_torch(H: int, W: int, device, hurst: float = 0.7, seed: int = 42, mean: float = 1000.0, std: float = 300.0,
              tile: int = 8192, row0: int = 0, total_rows: int | None = None):
    """float32 fBm DEM of any size built on the device: one periodic `tile`^2 fBm patch repeated over the raster
    (continuous across repeats) plus a smooth large-scale trend so that repeats differ.  `row0`/`total_rows`
    let a rank generate only its row block of a larger raster (identical values to the full build)."""
    import torch

    total_rows = total_rows or H
    t = min(tile, 1 << max(1, math.ceil(math.log2(max(total_rows, W)))))
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    w = torch.randn((t, t), generator=g, device=device, dtype=torch.float32)
    f = torch.fft.rfft2(w)
    ky = torch.fft.fftfreq(t, device=device)[:, None]
    kx = torch.fft.rfftfreq(t, device=device)[None, :]
    k = torch.sqrt(kx * kx + ky * ky)
    k[0, 0] = 1.0
    f = f * k.pow(-(hurst + 1.0))
    z = torch.fft.irfft2(f, s=(t, t))
    del f, w, k
    z = (z - z.mean()) / z.std()
    out = torch.empty((H, W), device=device, dtype=torch.float32)
    two_pi = 2.0 * math.pi
    xs = torch.arange(W, device=device, dtype=torch.float32)
    trend_x = 50.0 * torch.sin(two_pi * xs / W)
    for y0 in range(0, H, t):
        y1 = min(H, y0 + t)
        gy = torch.arange(row0 + y0, row0 + y1, device=device)
        ys = gy.to(torch.float32)
        trend_y = 50.0 * torch.cos(two_pi * ys / total_rows)
        src_rows = z[gy % t]
        for x0 in range(0, W, t):
            x1 = min(W, x0 + t)
            out[y0:y1, x0:x1] = mean + std * src_rows[:, : x1 - x0] + trend_x[None, x0:x1] + trend_y[:, None]
    return out


def c5_variogram_blocks(device, runs: int = 100, samples: int = 9091, size: int = 20000, seed: int = 45, rings: int = 10):
    """BASELINE C5 input as SURVEY.md 8d states it: a dh-like fBm(H = 0.3) field on a `size`^2 grid (gsd 1, no NaN, seed 45) and,
    per run, the centre-disk x equidistant-ring blocks of the product's own raster sampler
    (spatialstats.equidistant_blocks_from_raster; disk radius = extent diagonal / sqrt(2)^rings as
    `_choose_cdist_equidistant_sampling_parameters` sets it for this grid).  samples = 9091 is reading B (1e7 points drawn in
    total), samples = 223607 reading A (subsample = 1e7 in the reference's sense, 5e13 pairs).  Returns (blocks, right edges):
    50 explicit edges geomspace(sqrt 2, maxlag, 50).  Rings that leave the raster hold fewer points -- that is the geometry."""
    import torch

    from . import spatialstats as ss

    field = fbm_torch(size, size, device, hurst=0.3, seed=seed, mean=0.0, std=1.0).reshape(-1)
    maxdist = math.sqrt(2.0) * (size - 1)
    ratio = samples / (math.pi * maxdist**2 / math.sqrt(2.0) ** (2 * rings))   # res = 1: spatialstats.py:1176-1181

    def values_of(idx):
        return field[torch.from_numpy(np.ascontiguousarray(idx)).to(device)].cpu().numpy()

    rng = np.random.default_rng(seed)
    blocks = ss.equidistant_blocks_from_raster(None, 1.0, runs, samples, ratio, rng, values_of=values_of, shape=(size, size))
    edges = np.geomspace(math.sqrt(2.0), maxdist, 50)
    return blocks, edges


def _hash01(n: int, salt: int) -> np.ndarray:
    """n reproducible numbers in [0, 1): a 64-bit integer mix of the index (wrapping uint64 arithmetic, exact on every platform and
    NumPy version -- unlike a generator's stream, which NumPy does not pin across releases)."""
    with np.errstate(over="ignore"):
        x = (np.arange(n, dtype=np.uint64) + np.uint64(salt)) * np.uint64(0x9E3779B97F4A7C15)
        x ^= x >> np.uint64(29)
        x *= np.uint64(0xBF58476D1CE4E5B9)
        x ^= x >> np.uint64(32)
    return (x >> np.uint64(11)).astype(np.float64) / float(2**53)


def bias_case(H: int, W: int, dtype=np.float32) -> dict:
    """Inputs of the bias-correction fixtures and tests (tools/gen_golden_bincorr.py records the reference's results on exactly
    these): a DEM pair whose difference depends on three variables, NaNs in both rasters and in one variable plane, a patchy
    inlier mask, and the planes the corrections are applied with -- values exactly on bin edges, on the rightmost edge, outside the
    binned range and NaN.  Only exactly rounded operations (+, -, *, /, sqrt) on hashed integers: the same bits everywhere, so
    nothing of it needs storing.  The float64 pair is the float32 pair widened and perturbed below float32 resolution."""
    n = H * W
    row, col = np.divmod(np.arange(n), W)
    u = [_hash01(n, 1000 * k + 17) for k in range(8)]
    v1 = (10.0 * u[0]).astype(np.float32)                                   # uniform in [0, 10)
    v2 = 2.0 * (0.7 * u[1] + 0.3 * (row / max(H - 1, 1))) - 1.0              # float64 in [-1, 1)
    v3 = (30.0 * np.sqrt(u[2])).astype(np.float32)
    v3[(v3 >= 10.0) & (v3 < 14.0)] += np.float32(4.0)                       # a gap: empty bins
    ref = 800.0 + 0.5 * col + 0.3 * row + 25.0 * (u[3] - 0.5)
    bias = 0.3 * v1.astype(np.float64) - 0.02 * v1.astype(np.float64) ** 2 + 1.5 * v2 + 0.05 * v3.astype(np.float64)
    tba = ref - bias + 0.4 * (u[4] - 0.5)
    ref32, tba32 = ref.astype(np.float32), tba.astype(np.float32)
    if np.dtype(dtype) == np.float64:
        ref_o, tba_o = ref32.astype(np.float64) + 0.1, tba32.astype(np.float64) * 1.000000123
    else:
        ref_o, tba_o = ref32, tba32
    ref_o[u[5] < 0.03] = np.nan
    tba_o[u[6] < 0.03] = np.nan
    v1[u[7] < 0.02] = np.nan
    inlier = (_hash01(n, 9001) >= 0.02)
    out = {"v1": v1.reshape(H, W), "v2": v2.reshape(H, W), "v3": v3.reshape(H, W)}
    ref_o, tba_o, inlier = ref_o.reshape(H, W), tba_o.reshape(H, W), inlier.reshape(H, W)
    if H > 12 and W > 30:
        tba_o[5:9, 20:31] = np.nan
        inlier[H // 2:H // 2 + 6, W // 3:W // 3 + 15] = False
    # the planes of apply: the fit's planes with special values planted
    a1, a2, a3 = out["v1"].copy().reshape(-1), out["v2"].copy().reshape(-1), out["v3"].copy().reshape(-1)
    k = np.arange(n)
    for value, phase in ((2.5, 0), (5.0, 1), (10.0, 2), (-3.0, 3), (14.0, 4), (0.0, 5), (7.5, 6)):
        a1[k % 37 == phase] = np.float32(value)
    a2[k % 41 == 0] = 1.0
    a2[k % 41 == 1] = -1.0
    a2[k % 41 == 2] = 1.0 / 3.0
    a2[k % 41 == 3] = 2.5
    a2[k % 43 == 7] = np.nan
    a3[k % 47 == 0] = np.float32(12.0)    # inside the gap
    a3[k % 47 == 1] = np.float32(45.0)    # beyond the binned range
    out.update(ref=ref_o, tba=tba_o, inlier=inlier, a1=a1.reshape(H, W), a2=a2.reshape(H, W), a3=a3.reshape(H, W))
    return out


VOLUME_LABELS = {"plain": (3, 7, 77, 1000, (1 << 20) - 1), "tiny": 5, "no_valid": 11, "below_signal_coverage": 13,
                 "below_interp_coverage": 17, "flat": 19, "on_edges": 23, "sparse_bins": 29}


def volume_case(H: int, W: int, dtype=np.float32) -> dict:
    """Inputs of the xdem_amd.volume fixtures and tests (tools/gen_golden_volume.py records the reference's results on exactly these):
    a tilted reference DEM with relief (multiples of 1/8 m), a dDEM with an elevation trend and ties among its values, NaN voids and
    a few +-inf, a copy of the reference with voids, and a glacier index map (VOLUME_LABELS): non-contiguous ids up to 2^20 - 1,
    label 0, an outline of 6 pixels, one without a valid dDEM, one just below each coverage threshold (4 and 9 valid pixels of 100),
    one of constant elevation, one whose elevations are the bin edges themselves, one that leaves bins with 0, 1, 2 and 3 samples.
    Rasters too small for that layout (below 50 x 80) get runs of five labels along the flattened raster.  Only exactly rounded
    operations on hashed integers: the same bits everywhere.  The float64 pair is the float32 pair widened and moved by multiples of
    2^-10 / 2^-12, below what float32 resolves there."""
    n = H * W
    k = np.arange(n)
    row, col = np.divmod(k, W)
    u = [_hash01(n, 2000 * j + 31) for j in range(5)]
    ref = (8000.0 + 64.0 * row + 16.0 * col + np.floor(240.0 * u[0])) / 8.0
    ddem = -(ref - 1000.0) / 64.0 + (np.floor(64.0 * u[1]) - 32.0) / 16.0
    if np.dtype(dtype) == np.float64:
        ref = ref + np.floor(8.0 * u[3]) / 1024.0
        ddem = ddem + np.floor(8.0 * u[4]) / 4096.0
    finite_ddem = ddem.copy()
    ddem[u[2] < 0.2] = np.nan
    ddem[k % 997 == 3] = np.inf
    ddem[k % 997 == 5] = -np.inf
    ref, ddem, finite_ddem = ref.reshape(H, W), ddem.reshape(H, W), finite_ddem.reshape(H, W)
    lab = np.zeros((H, W), dtype=np.int32)
    if H >= 50 and W >= 80:
        ddem[H // 4:H // 4 + 5, W // 5:W // 5 + 9] = np.nan
        a, b, c = W // 3, 2 * W // 3, H // 2
        lab[2:c, 2:a] = 3
        lab[2:c, a + 2:b] = 7
        lab[c + 2:H - 2, 2:a] = 77
        lab[c + 2:H - 2, a + 2:b] = 1000
        lab[2:H // 3, b + 2:W - 2] = (1 << 20) - 1
        r0, xa, xb = H // 3 + 1, b + 2, b + 13

        def place(label, r, x, h, w, ref_values=None, n_valid=None):
            sl = (slice(r, r + h), slice(x, x + w))
            lab[sl] = label
            if ref_values is not None:
                ref[sl] = np.asarray(ref_values, dtype=np.float64).reshape(h, w)
            d = finite_ddem[sl].copy()
            if n_valid is not None:
                d.reshape(-1)[n_valid:] = np.nan
            ddem[sl] = d

        place(13, r0, xa, 10, 10, n_valid=4)
        place(17, r0 + 11, xa, 10, 10, n_valid=9)
        sparse = [1500.0, 1700.0, 1525.0, 1545.0, 1546.0, 1565.0, 1566.0, 1567.0] + [1620.0 + 2.5 * j for j in range(32)]
        place(29, r0 + 22, xa, 4, 10, ref_values=sparse)
        place(5, r0, xb, 2, 3)
        place(11, r0 + 3, xb, 4, 5, n_valid=0)
        place(19, r0 + 8, xb, 4, 5, ref_values=[1111.0] * 20)
        place(23, r0 + 13, xb, 3, 7, ref_values=[1200.0 + 5.0 * j for j in range(21)])
    else:
        flat = lab.reshape(-1)
        for label, lo, hi in ((3, n // 10, 4 * n // 10), (5, 4 * n // 10, 4 * n // 10 + 6), (7, 9 * n // 20, 13 * n // 20),
                              (11, 13 * n // 20, 15 * n // 20), (1000, 15 * n // 20, n)):
            flat[lo:hi] = label
        ddem.reshape(-1)[13 * n // 20:15 * n // 20] = np.nan
    ref_voids = ref.copy()
    ref_voids.reshape(-1)[k % 211 == 7] = np.nan
    mask = (lab == 3) | (lab == 7) | (lab == 77) | (lab == 1000)
    if not (H >= 50 and W >= 80):
        mask = lab > 0
    dt = np.dtype(dtype)
    return {"ddem": ddem.astype(dt), "ref": ref.astype(dt), "ref_voids": ref_voids.astype(dt), "labels": lab, "mask": mask}


CLOUD_SHIFT = (7.5, -4.0, 2.25)   # the offsets (easting, northing, vertical) a Nuth-Kaab fit of cloud_case finds with the cloud as reference


def cloud_surface(x, y, t6, shape):
    """The smooth surface of ``cloud_case`` at georeferenced (x, y): a bowl with a cross term and a cubic, so that every aspect occurs and
    the slope tangent is a few tenths over most of the raster and passes 1 at its rim: the signal of the shift, slope times 8.5 m, stands
    well above the 0.3 m of noise everywhere but within a few pixels of the bowl's floor.  Only +, -, * on float64."""
    H, W = shape
    u = (x - (t6[2] + 0.5 * W * t6[0])) * 1e-3          # kilometres from the raster's centre
    v = (y - (t6[5] + 0.5 * H * t6[4])) * 1e-3
    return 1000.0 + 720.0 * u * u + 1040.0 * v * v + 360.0 * u * v + 600.0 * u * u * u - 480.0 * u * v * v


def cloud_case(H: int, W: int, n: int, dtype=np.float32) -> dict:
    """Inputs of the raster-point fixtures and tests (tools/gen_golden_rstpts.py records the reference's results on exactly these): a
    raster of ``cloud_surface`` on a 10 m grid with a NaN block and an outlier-mask region, and a cloud of about ``n`` points of the
    same surface displaced by ``CLOUD_SHIFT`` with 0.3 m of noise.  Of the points, some lie off the raster by less and by more than
    one pixel, some exactly on pixel centres (the last row and column included, where the four tap rules differ), some are duplicated,
    some have a NaN or infinite z and some a NaN coordinate; about a tenth is invalid.  Hashed integers and exactly rounded operations
    only: the same bits everywhere, nothing of it needs storing."""
    dt = np.dtype(dtype)
    t6 = (10.0, 0.0, 500000.0, 0.0, -10.0, 4200000.0 + 10.0 * H)
    rows, cols = np.divmod(np.arange(H * W), W)
    px, py = t6[2] + (cols + 0.5) * t6[0], t6[5] + (rows + 0.5) * t6[4]
    raster = cloud_surface(px, py, t6, (H, W)).astype(np.float32)
    raster = (raster.astype(np.float64) + 1e-5 * (_hash01(H * W, 77) - 0.5) if dt == np.float64 else raster).reshape(H, W)
    raster[H // 5:H // 5 + 6, W // 2:W // 2 + 9] = np.nan
    inlier = np.ones((H, W), dtype=bool)
    inlier[H // 2:H // 2 + 7, W // 6:W // 6 + 11] = False
    m = n - 24   # the random points; the 24 others are planted below
    u = [_hash01(m, 5000 * k + 31) for k in range(4)]
    # positions over the raster's extent widened by 1.6 pixels on every side
    x = t6[2] + (u[0] * (W + 3.2) - 1.6) * t6[0]
    y = t6[5] + (u[1] * (H + 3.2) - 1.6) * t6[4]
    noise = 0.3 * ((u[2] + u[3] + _hash01(m, 20031)) * 2.0 - 3.0)   # sum of three uniforms: standard deviation 0.3 * 2 * 0.5 = 0.3
    sx, sy, sz = CLOUD_SHIFT
    # planted points: pixel centres (corners, last row / column, interior), then duplicates of the first random points
    pr = np.array([0, 0, H - 1, H - 1, H - 1, H // 3, 1, H - 2], dtype=np.float64)
    pc = np.array([0, W - 1, 0, W - 1, W // 2, W - 1, 1, W - 2], dtype=np.float64)
    x = np.concatenate([x, t6[2] + (pc + 0.5) * t6[0], x[:8], x[8:16]])
    y = np.concatenate([y, t6[5] + (pr + 0.5) * t6[4], y[:8], y[8:16]])
    z = cloud_surface(x + sx, y + sy, t6, (H, W)) + sz
    z[:m] += noise
    z[m + 8:m + 16] = z[:8]
    # non-finite entries among the last eight (copies of random points 8..15)
    z[m + 16] = np.nan
    z[m + 17] = np.inf
    z[m + 18] = -np.inf
    x[m + 19] = np.nan
    y[m + 20] = np.nan
    return {"raster": raster.astype(dt), "inlier": inlier, "transform": t6, "x": x, "y": y, "z": z, "shift": CLOUD_SHIFT,
            "res": (10.0, 10.0)}
