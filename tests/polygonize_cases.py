"""The class planes of the polygonize tests, sized from ``xdemhip_label_plan`` so that under either value of the test switch
``"ccl_route"`` (0: automatic tiles, 2: minimal tiles) every plane crosses tile borders: with T_r x T_c the tile, the standard shape is
``(2 T_r + 3) x (2 T_c + 5)``, nine partial tiles."""
import functools

import numpy as np

from xdem_amd import polygonize

SWITCHES = (0, 2)
CONNECTIVITIES = (4, 8)
TRANSFORM = (2.5, 0.0, 1000.25, 0.0, -1.75, 5000.5)   # (exact in binary: the vertices are, too)
ROUND_TRIP_TRANSFORM = (30.0, 0.0, 412345.0, 0.0, -30.0, 5267890.0)

PINCH = np.array([[1, 1, 1, 1, 0, 0],     # holes at (1, 1) and (2, 2) meet diagonally: a pinch between two hole rings
                  [1, 0, 1, 1, 1, 1],     # the hole at (4, 4) meets the background pixel (5, 5) diagonally: a pinch between the
                  [1, 1, 0, 1, 1, 1],     # exterior and a hole
                  [1, 1, 1, 1, 1, 1],
                  [0, 1, 1, 1, 0, 1],
                  [0, 1, 1, 1, 1, 0]], np.int32)


def tile(switch):
    p = polygonize.label_plan(8, 8, switch)
    return p["tile_rows"], p["tile_cols"]


def _serpentine(H, W):
    a = np.zeros((H, W), np.int32)
    a[::2] = 1
    for k, r in enumerate(range(1, H, 2)):
        a[r, W - 1 if k % 2 == 0 else 0] = 1
    return a


def _spiral(H, W):
    """A one-pixel-wide path that winds inwards, a background pixel between its turns."""
    a = np.zeros((H, W), np.int32)
    r = c = d = stuck = 0
    a[0, 0] = 1
    while stuck < 2:
        dr, dc = ((0, 1), (1, 0), (0, -1), (-1, 0))[d]
        r1, c1, r2, c2 = r + dr, c + dc, r + 2 * dr, c + 2 * dc
        if 0 <= r1 < H and 0 <= c1 < W and not a[r1, c1] and not (0 <= r2 < H and 0 <= c2 < W and a[r2, c2]):
            r, c, stuck = r1, c1, 0
            a[r, c] = 1
        else:
            d, stuck = (d + 1) % 4, stuck + 1
    return a


def _nested(H, W):
    a = np.zeros((H, W), np.int32)
    for k, v in enumerate((1, 0, 1, 0, 2)):   # island in lake in island, and a second class in the innermost lake
        m = 1 + 3 * k
        if H - 2 * m > 0 and W - 2 * m > 0:
            a[m:H - m, m:W - m] = v
    return a


@functools.lru_cache(maxsize=None)
def cases(switch):
    """``[(name, int32 class plane)]`` for a value of the switch (read-only arrays, shared among the tests)."""
    tr, tc = tile(switch)
    H, W = 2 * tr + 3, 2 * tc + 5
    rng = np.random.default_rng(20261021 + switch)
    rr, cc = np.indices((H, W))
    out = [("one_pixel", np.ones((1, 1), np.int32)),
           ("one_pixel_background", np.zeros((1, 1), np.int32)),
           ("row", (rng.random((1, W)) < 0.6).astype(np.int32)),
           ("column", (rng.random((H, 1)) < 0.6).astype(np.int32)),
           ("all_foreground", np.ones((H, W), np.int32)),
           ("all_background", np.zeros((H, W), np.int32)),
           ("serpentine", _serpentine(H, W)),
           ("serpentine_columns", np.ascontiguousarray(_serpentine(W, H).T)),
           ("spiral", _spiral(H, W)),
           ("checkerboard", ((rr + cc) % 2 == 0).astype(np.int32)),
           ("diagonals", ((rr + cc) % 5 == 0).astype(np.int32) + 2 * ((rr - cc) % 7 == 3).astype(np.int32) * ((rr + cc) % 5 != 0)),
           ("two_classes", np.where(cc < tc + 1, 3, 7).astype(np.int32)),
           ("nested", _nested(H, W))]
    corner = np.zeros((H, W), np.int32)   # pairs that touch only diagonally at the four-tile corner, both ways
    corner[tr - 1, tc - 1] = corner[tr, tc] = 1
    corner[2 * tr - 1, 2 * tc] = corner[2 * tr, 2 * tc - 1] = 1
    corner[2 * tr - 1, tc] = corner[2 * tr, tc - 1] = 5
    out.append(("tile_corner_pairs", corner))
    pinch = np.zeros((H, W), np.int32)
    r0, c0 = max(tr - 3, 0), max(tc - 3, 0)   # (across a four-tile corner where the tile is large enough)
    pinch[r0:r0 + 6, c0:c0 + 6] = PINCH
    if W >= 20:
        pinch[:6, W - 6:] = PINCH[::-1]
        pinch[H - 6:, :6] = PINCH.T * 4
    out.append(("pinches", pinch))
    n = max(H, 140)   # a staircase: 2 n + 2 corners on one ring, more than a workgroup's 256 lanes and nine jumping rounds
    out.append(("staircase", (np.indices((n, n))[1] <= np.indices((n, n))[0]).astype(np.int32)))
    for density in (0.3, 0.59, 0.8):
        out.append((f"random_{density}", (rng.random((H, W)) < density).astype(np.int32)))
    wide = np.ones((3, 2100), np.int32)   # more pixels than one workgroup of the table pass walks (4096), in rows longer than a wave's share of them
    wide[1, 1500:1600] = 0
    wide[2, 100] = 2
    wide[0, 1024:2048] = 3
    out.append(("wide_rows", wide))
    out.append(("random_classes", rng.integers(0, 4, (H, W)).astype(np.int32) * (rng.random((H, W)) < 0.8)))
    out = [(name, np.ascontiguousarray(a, dtype=np.int32)) for name, a in out]
    for _, a in out:
        a.setflags(write=False)
    return out


def case(switch, name):
    return dict(cases(switch))[name]
