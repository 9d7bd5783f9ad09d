"""Polygon tables for the Vector tests (test_vector_host.py, test_vector_gpu.py), on the two grids of ``synth.cloud_case`` (61 x 83 and
96 x 128 at 10 m, origin 5e5 / 4.2e6: coordinates with few spare bits) and on unit grids with origin 0, where half-integer coordinates
make the abscissa arithmetic exact.  Everything is made from hashed integers (``synth._hash01``): the same bits everywhere.

Geometry is written in PIXEL coordinates (u right, v down, pixel (r, c) has its centre at (c + 0.5, r + 0.5)) and moved to the grid's
coordinates by ``world``."""
from __future__ import annotations

import numpy as np

from xdem_amd.synth import _hash01

SHAPES = ((61, 83), (96, 128))
SEG_REG, SEG_LDS, WIDE = 8, 4096, 64   # VEC_SEG_REG, VEC_SEG_LDS, VEC_WIDE of csrc/vector.hip

# Measured on the MI355X (tools/bench_rasterize.py -> profiles/vector_bench.json; ROCm 7.2.0): median wall clock in ms of a mask / label
# call on a 20000^2 grid with device planes, and the kernels launched per call.  Nothing in the tests depends on a time.
MEASURED = {"rgi_like_ms": (5.0, 9.4), "giant_ms": (2.5, 4.1), "pixel_sized_ms": (6.0, 5.9), "launches": 18,
            "min_centre_to_edge_px": {(61, 83): 1.8e-5, (96, 128): 5.2e-5}}   # (the star with its hole; the strips: 2.9e-4, 8.6e-4)


def grid(H: int, W: int) -> tuple:
    return (H, W), (10.0, 0.0, 500000.0, 0.0, -10.0, 4200000.0 + 10.0 * H)


def unit_grid(H: int, W: int) -> tuple:
    return (H, W), (1.0, 0.0, 0.0, 0.0, -1.0, float(H))


def world(t6, uv) -> np.ndarray:
    uv = np.asarray(uv, dtype=np.float64).reshape(-1, 2)
    return np.stack([t6[2] + uv[:, 0] * t6[0], t6[5] + uv[:, 1] * t6[4]], axis=1)


def star(shape, t6, n: int = 37, salt: int = 1, centre=None, r_out=None, r_in=None) -> np.ndarray:
    """A star of n vertices with hashed radii; by default about the grid's centre and leaving the grid."""
    H, W = shape
    cu, cv = centre if centre is not None else (0.47 * W, 0.52 * H)
    r_out = r_out if r_out is not None else 0.75 * max(H, W)
    r_in = r_in if r_in is not None else 0.18 * min(H, W)
    h = _hash01(n, 100 * salt + 7)
    ang = 2 * np.pi * (np.arange(n) + 0.3 * h) / n
    rad = np.where(np.arange(n) % 2 == 0, r_out, r_in) * (0.85 + 0.3 * _hash01(n, 100 * salt + 9))
    return world(t6, np.stack([cu + rad * np.cos(ang), cv + rad * np.sin(ang)], axis=1))


def star_with_hole(shape, t6) -> tuple:
    """(exterior, [hole]): the 37-vertex star that leaves the grid and a REVERSED (clockwise against it) 9-gon hole about its centre."""
    H, W = shape
    hole = star(shape, t6, n=9, salt=3, r_out=0.11 * min(H, W), r_in=0.09 * min(H, W))[::-1]
    ext = star(shape, t6)
    assert min_centre_to_edge([ext, hole], shape, t6) >= 1e-6   # (away from edges the result is geometry alone: matplotlib must agree)
    return ext, [hole]


def strips(shape, t6, n: int = 7) -> list:
    """n strips between n + 1 jittered polylines that run from above the grid to below it; the outer two lie beyond the grid's sides,
    so the strips cover every pixel exactly once."""
    H, W = shape
    m = 9   # vertices per polyline
    v = np.linspace(-3.3, H + 2.7, m)
    lines = []
    for k in range(n + 1):
        base = -2.6 + k * (W + 5.3) / n
        jitter = (W / n) * 0.3 * (_hash01(m, 40 + k) - 0.5)
        lines.append(np.stack([base + jitter, v], axis=1))
    out = [world(t6, np.concatenate([lines[k], lines[k + 1][::-1]], axis=0)) for k in range(n)]
    assert min_centre_to_edge(out, shape, t6) >= 1e-6
    return out


def comb(t6, n_teeth: int, u0: float, v_top: float, v_base: float, v_bottom: float, pitch: float, salt: int = 0) -> np.ndarray:
    """A comb: a base between rows v_base and v_bottom with n_teeth teeth up to v_top.  A row through the teeth is crossed
    2 * n_teeth times, a row through the base twice.  Teeth are `pitch` apart, about half of that wide, with hashed slants."""
    h = _hash01(4 * n_teeth, 900 + salt)
    pts = [(u0, v_bottom)]
    for k in range(n_teeth):
        left = u0 + k * pitch
        width = pitch * (0.35 + 0.3 * h[4 * k])
        s0, s1 = pitch * 0.1 * (h[4 * k + 1] - 0.5), pitch * 0.1 * (h[4 * k + 2] - 0.5)
        if k:
            pts.append((left, v_base))
        pts.append((left + s0, v_top))
        pts.append((left + width + s1, v_top))
        if k < n_teeth - 1:
            pts.append((left + width, v_base))
    pts.append((u0 + (n_teeth - 1) * pitch + pitch * 0.5, v_bottom))
    return world(t6, pts)


def rect(t6, u0, u1, v0, v1, ccw: bool = True) -> np.ndarray:
    r = np.array([(u0, v0), (u1, v0), (u1, v1), (u0, v1)], dtype=np.float64)
    return world(t6, r if ccw else r[::-1])


def span_rects(t6, W: int, widths=(0, 1, 63, 64, 65, 255, 256, 257)) -> tuple:
    """One thin rectangle per row of a grid: spans of the given numbers of columns (0: between two centres), then one over the full
    width and one that ends on column W - 1.  Returns (rectangles, expected (first column, columns) per row)."""
    rects, want = [], []
    for k, w in enumerate(widths):
        if w == 0:
            rects.append(rect(t6, 3.6, 3.9, k + 0.25, k + 0.75))
        else:
            rects.append(rect(t6, 3.25, 3.25 + w, k + 0.25, k + 0.75))
        want.append((3, w))
    k = len(widths)
    rects.append(rect(t6, -5.0, W + 5.0, k + 0.25, k + 0.75))
    want.append((0, W))
    rects.append(rect(t6, W - 10.75, W + 3.0, k + 1.25, k + 1.75))
    want.append((W - 11, 11))
    return rects, want


def many_small(shape, t6, n: int = 3000) -> list:
    """n quadrilaterals of one to three pixels each on a lattice over the grid, hashed corners; neighbours may overlap."""
    H, W = shape
    per_row = int(np.ceil(np.sqrt(n * W / H)))
    k = np.arange(n)
    cu = (k % per_row + 0.5) * W / per_row
    cv = (k // per_row + 0.5) * H / (n // per_row + 1)
    h = [_hash01(n, 7000 + 13 * j) for j in range(8)]
    out = []
    for i in range(n):
        corners = [(cu[i] - 0.4 - 1.2 * h[0][i], cv[i] - 0.4 - 1.2 * h[1][i]), (cu[i] + 0.4 + 1.2 * h[2][i], cv[i] - 0.4 - 1.2 * h[3][i]),
                   (cu[i] + 0.4 + 1.2 * h[4][i], cv[i] + 0.4 + 1.2 * h[5][i]), (cu[i] - 0.4 - 1.2 * h[6][i], cv[i] + 0.4 + 1.2 * h[7][i])]
        out.append(world(t6, corners))
    return out


# ---- the independent comparator: matplotlib's point-in-polygon on the pixel centres, XOR-ed over the rings of a polygon ------------------
def mpl_mask(rings, shape, t6) -> np.ndarray:
    from matplotlib.path import Path

    H, W = shape
    cx = t6[2] + (np.arange(W) + 0.5) * t6[0]
    cy = t6[5] + (np.arange(H) + 0.5) * t6[4]
    pts = np.stack([np.tile(cx, H), np.repeat(cy, W)], axis=1)
    inside = np.zeros(H * W, dtype=bool)
    for ring in rings:
        inside ^= Path(np.asarray(ring)).contains_points(pts)
    return inside.reshape(H, W)


def min_centre_to_edge(rings, shape, t6) -> float:
    """The smallest distance of a pixel centre to an edge of `rings`, in pixels."""
    H, W = shape
    cu, cv = np.meshgrid(np.arange(W) + 0.5, np.arange(H) + 0.5)
    p = np.stack([cu.ravel(), cv.ravel()], axis=1)
    best = np.inf
    for ring in rings:
        uv = np.stack([(np.asarray(ring)[:, 0] - t6[2]) / t6[0], (np.asarray(ring)[:, 1] - t6[5]) / t6[4]], axis=1)
        for i in range(len(uv)):
            a, b = uv[i], uv[(i + 1) % len(uv)]
            ab = b - a
            den = float(ab @ ab)
            t = np.clip(((p - a) @ ab) / den, 0.0, 1.0) if den > 0 else np.zeros(len(p))
            d = np.hypot(*(p - (a + t[:, None] * ab)).T)
            best = min(best, float(d.min()))
    return best
