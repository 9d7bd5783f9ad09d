"""The rule of xdemhip_label / xdemhip_label_table / xdemhip_outlines (include/xdemhip.h) restated in plain NumPy and
Python: a raster-order flood fill, the per-component table, and the outline rings followed edge by edge.  ``OracleEngine`` has the
methods of ``xdem_amd.polygonize.DeviceEngine`` and stands in for it where no GPU is at hand."""
import numpy as np

from xdem_amd.polygonize import RingTable, TABLE_COLUMNS

# sides 0 top, 1 left, 2 bottom, 3 right: the direction an edge runs in (row, col) and the step to the pixel across it
DIR = ((0, -1), (1, 0), (0, 1), (-1, 0))
ACROSS = ((-1, 0), (0, -1), (1, 0), (0, 1))
NEIGH4 = ((-1, 0), (0, -1), (0, 1), (1, 0))
NEIGH8 = NEIGH4 + ((-1, -1), (-1, 1), (1, -1), (1, 1))


def label(classes, connectivity=4):
    """``(int32 labels, K)``: components numbered in raster order of their first pixel, by flood fill."""
    cls = np.asarray(classes)
    H, W = cls.shape
    out = np.zeros((H, W), np.int32)
    neigh = NEIGH4 if connectivity == 4 else NEIGH8
    K = 0
    for r in range(H):
        for c in range(W):
            v = cls[r, c]
            if v == 0 or out[r, c]:
                continue
            K += 1
            out[r, c] = K
            stack = [(r, c)]
            while stack:
                y, x = stack.pop()
                for dy, dx in neigh:
                    yy, xx = y + dy, x + dx
                    if 0 <= yy < H and 0 <= xx < W and not out[yy, xx] and cls[yy, xx] == v:
                        out[yy, xx] = K
                        stack.append((yy, xx))
    return out, K


def table(classes, labels, K):
    """The ``(7, K)`` int64 table of ``TABLE_COLUMNS``."""
    cls, lab = np.asarray(classes), np.asarray(labels)
    W = lab.shape[1]
    t = np.zeros((len(TABLE_COLUMNS), K), np.int64)
    rows, cols = np.nonzero(lab)
    which = lab[rows, cols] - 1
    for k in range(K):
        m = which == k
        r, c = rows[m], cols[m]
        first = int((r * W + c).min())
        t[:, k] = (int(cls.reshape(-1)[first]), r.size, r.min(), r.max(), c.min(), c.max(), first)
    return t


def _shifted(pad, dy, dx, H, W):
    return pad[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]


def edge_turns(labels):
    """int8 ``(H, W, 4)``: per pixel and side -1 no edge, 0 the successor goes straight on, 1 it turns left, 2 it turns right."""
    lab = np.asarray(labels)
    H, W = lab.shape
    pad = np.zeros((H + 2, W + 2), lab.dtype)
    pad[1:-1, 1:-1] = lab
    turn = np.full((H, W, 4), -1, np.int8)
    fg = lab != 0
    for s in range(4):
        (dr, dc), (nr, nc) = DIR[s], ACROSS[s]
        edge = fg & (_shifted(pad, nr, nc, H, W) != lab)
        right = _shifted(pad, nr + dr, nc + dc, H, W) == lab
        ahead = _shifted(pad, dr, dc, H, W) == lab
        turn[..., s] = np.where(edge, np.where(right, 2, np.where(ahead, 0, 1)), -1)
    return turn


def successor(turn, r, c, s):
    t = turn[r, c, s]
    (dr, dc), (nr, nc) = DIR[s], ACROSS[s]
    if t == 1:
        return r, c, (s + 1) % 4
    if t == 0:
        return r + dr, c + dc, s
    return r + nr + dr, c + nc + dc, (s + 3) % 4


def end_vertex(r, c, s):
    return r + (1 if s in (1, 2) else 0), c + (1 if s >= 2 else 0)


def rings_of(labels):
    """The rings of a label plane in the stated order: a list of ``(label, leader edge number, [(i, j) corner vertices])``."""
    lab = np.asarray(labels)
    H, W = lab.shape
    turn = edge_turns(lab)
    seen = np.zeros((H, W, 4), bool)
    found = []
    for r, c, s in zip(*np.nonzero(turn > 0)):   # (corner edges in edge-number order: the first one met on a ring is its lowest)
        if seen[r, c, s]:
            continue
        verts = []
        e = (int(r), int(c), int(s))
        while True:
            seen[e] = True
            assert turn[e] >= 0 and lab[e[0], e[1]] == lab[r, c]
            if turn[e] > 0:
                verts.append(end_vertex(*e))
            e = successor(turn, *e)
            if e == (r, c, s):
                break
        found.append((int(lab[r, c]), 4 * (int(r) * W + int(c)) + int(s), verts))
    assert np.array_equal(seen, turn >= 0), "every edge lies on exactly one ring"
    found.sort(key=lambda g: (g[0], g[1]))
    return found


def signed_area(verts) -> int:
    """The signed area of a ring of (i, j) vertices in map orientation (x = j, y = -i), exact."""
    v = np.asarray(verts, dtype=np.int64)
    x, y = v[:, 1], -v[:, 0]
    twice = int(np.sum(x * np.roll(y, -1) - np.roll(x, -1) * y))
    assert twice % 2 == 0
    return twice // 2


def outlines(labels, K, t6) -> RingTable:
    a, _, c0, _, e, f = (np.float64(v) for v in t6)
    rings = rings_of(labels)
    i = np.array([v[0] for _, _, verts in rings for v in verts], dtype=np.float64)
    j = np.array([v[1] for _, _, verts in rings for v in verts], dtype=np.float64)
    xy = np.stack([c0 + a * j, f + e * i]) if i.size else np.zeros((2, 0))
    ring_off = np.zeros(len(rings) + 1, np.int64)
    ring_off[1:] = np.cumsum([len(verts) for _, _, verts in rings])
    owner = np.array([lb - 1 for lb, _, _ in rings], dtype=np.int32)
    area = np.array([signed_area(verts) for _, _, verts in rings], dtype=np.int64)
    return RingTable(np.ascontiguousarray(xy, dtype=np.float64), ring_off, owner, area, int(K))


def even_odd_fill(verts, shape):
    """The pixels whose centre is inside a set of rings of (i, j) vertices, even-odd, in integer arithmetic: a vertical edge at column
    j over rows [lo, hi) toggles every pixel of those rows from column j on."""
    H, W = shape
    toggles = np.zeros((H, W + 1), np.int64)
    for ring in verts:
        v = np.asarray(ring, dtype=np.int64)
        nxt = np.roll(v, -1, axis=0)
        for (i0, j0), (i1, j1) in zip(v, nxt):
            if j0 == j1 and i0 != i1:
                toggles[min(i0, i1):max(i0, i1), j0] += 1
    return (np.cumsum(toggles, axis=1)[:, :W] % 2).astype(bool)


class OracleEngine:
    """``xdem_amd.polygonize.DeviceEngine`` on the CPU."""

    def label(self, classes, connectivity=4, ctx=None):
        return label(classes, connectivity)

    def table(self, classes, labels, K, ctx=None):
        return table(classes, labels, K)

    def outlines(self, labels, K, t6, ctx=None):
        return outlines(labels, K, t6)
