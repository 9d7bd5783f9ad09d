"""The rasterisation rule of include/xdemhip.h ("polygons burnt into a grid") in NumPy float64, edge by edge: what csrc/vector.hip
must return bit for bit.  Own code; nothing of it comes from geoutils, rasterio or GDAL, none of which is installed.

    cy(r) = f + (r + 0.5) * e,  cx(c) = c0 + (c + 0.5) * a
    an edge (x1, y1) -> (x2, y2), y1 != y2, crosses row r iff min(y1, y2) <= cy(r) < max(y1, y2), at
    x = x1 + (cy(r) - y1) * (x2 - x1) / (y2 - y1); pixel (r, c) is inside iff an odd number of crossings of row r have x <= cx(c).

NumPy evaluates ``a * b / c`` as ``(a * b) / c`` and rounds every operation on its own, which is what the kernel does without contraction.
"""
from __future__ import annotations

import contextlib

import numpy as np


def centres(shape, t6):
    H, W = shape
    cy = t6[5] + (np.arange(H, dtype=np.float64) + 0.5) * t6[4]
    cx = t6[2] + (np.arange(W, dtype=np.float64) + 0.5) * t6[0]
    return cx, cy


def rings_mask(rings, shape, t6) -> np.ndarray:
    """Even-odd over all `rings` (each (N, 2), closed implicitly; fewer than three vertices: nothing)."""
    cx, cy = centres(shape, t6)
    inside = np.zeros(shape, dtype=bool)
    for ring in rings:
        ring = np.asarray(ring, dtype=np.float64)
        n = ring.shape[0]
        if n < 3:
            continue
        for i in range(n):
            x1, y1 = ring[i]
            x2, y2 = ring[(i + 1) % n]
            if y1 == y2:
                continue
            rows = np.flatnonzero((min(y1, y2) <= cy) & (cy < max(y1, y2)))
            if rows.size == 0:
                continue
            x = x1 + (cy[rows] - y1) * (x2 - x1) / (y2 - y1)
            inside[rows] ^= x[:, None] <= cx[None, :]
    return inside


def table_rings(table) -> list:
    """Per polygon of a ``Vector.tables()`` tuple the list of its rings."""
    xy, ring_off, poly_of_ring, n_poly = table
    out = [[] for _ in range(n_poly)]
    for r, p in enumerate(poly_of_ring):
        out[p].append(np.stack([xy[0, ring_off[r]:ring_off[r + 1]], xy[1, ring_off[r]:ring_off[r + 1]]], axis=1))
    return out


def mask(tables, shape, t6) -> np.ndarray:
    out = np.zeros(shape, dtype=bool)
    for table in tables:
        for rings in table_rings(table):
            out |= rings_mask(rings, shape, t6)
    return out


def labels(table, burn, out_value, shape, t6):
    """(int32 plane, burnt pixels): the LAST polygon of the table that holds a pixel gives its value."""
    out = np.full(shape, out_value, dtype=np.int32)
    burnt = np.zeros(shape, dtype=bool)
    for p, rings in enumerate(table_rings(table)):
        m = rings_mask(rings, shape, t6)
        out[m] = burn[p]
        burnt |= m
    return out, int(burnt.sum())


class OracleRasterizer:
    """Stands in for ``xdem_amd.vector.DeviceRasterizer`` (``vector._RASTERIZER``) where no GPU is at hand: host arrays only."""

    last_count = 0
    calls = 0

    def mask(self, tables, shape, t6, device=False, ctx=None):
        assert not device, "the oracle has no device route"
        OracleRasterizer.calls += 1
        out = mask(tables, shape, t6)
        self.last_count = int(out.sum())
        return out

    def labels(self, table, burn, out_value, shape, t6, device=False, ctx=None):
        assert not device, "the oracle has no device route"
        OracleRasterizer.calls += 1
        out, self.last_count = labels(table, burn, out_value, shape, t6)
        return out


@contextlib.contextmanager
def patched():
    """xdem_amd.vector with its device rasteriser replaced by the restatement above."""
    from xdem_amd import vector

    saved = vector._RASTERIZER
    vector._RASTERIZER = OracleRasterizer()
    try:
        yield vector
    finally:
        vector._RASTERIZER = saved
