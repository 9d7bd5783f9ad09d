"""Empirical variogram sampling on MI355X -- host-side mirror of ``xdem.spatialstats.sample_empirical_variogram``.

Same signature and DataFrame result (``exp``, ``lags``, ``count``, ``err_exp``; last lag dropped) as the reference
(``xdem/spatialstats.py:1295-1546``).  The host preparation (grid coordinates, ``maxlag``, sqrt(2)-geometric right
bin edges, child seeds, equidistant sampling parameters ``_choose_cdist_equidistant_sampling_parameters`` 1104-1183,
multi-run aggregation) follows the reference line by line -- deliberately: the integer parameter rule must reproduce ``runs /
samples / ratio`` exactly, the reference's tests assert the messages, and the aggregation IS pandas' ``groupby().mean() / .std()``
(its compensated summation is part of the recorded DataFrames), so those three blocks keep the reference's statements rather than
an equivalent of their own; the pairwise work that upstream delegates to scikit-gstat
(``skg.Variogram`` / ``skg.RasterEquidistantMetricSpace``) runs in ``csrc/variogram.hip`` through the
``xdemhip_pairs_*`` C-ABI: distances, lag classes, and per-class Matheron / Cressie-Hawkins sums or the exact
median for Dowd (radix selection over integer histograms, all-reducible across GPUs).

scikit-gstat conventions restated here (package un-vendored and absent -- "parity unpinned"): lag class
k = [e_{k-1}, e_k); matheron = sum d^2/(2n); cressie = 0.5 (mean sqrt d)^4/(0.457 + 0.494/n + 0.045/n^2);
dowd = 2.198 median(d)^2 / 2.  Random subsampling uses NumPy generators (geoutils' ``subsample_array`` is absent).
"""
from __future__ import annotations

import ctypes
import logging
import os
import warnings
from collections.abc import Iterable
from typing import Any, Callable, TypedDict

import numpy as np

from . import _args, _lib
from ._args import dp, i64p, ptr

_ESTIMATORS = ("matheron", "cressie", "dowd")


def _host_threads() -> int:
    """Threads of the host-side preparation (sampling runs, Morton orders of the pair blocks): the cores this process may use,
    at most 16; XDEM_HOST_THREADS overrides (1 = serial)."""
    import os

    env = os.environ.get("XDEM_HOST_THREADS")
    if env:
        return max(1, int(env))
    try:
        n = len(os.sched_getaffinity(0))
    except AttributeError:  # pragma: no cover
        n = os.cpu_count() or 1
    return max(1, min(16, n))


def _host_map(fn, jobs: list) -> list:
    """`[fn(j) for j in jobs]` on a pool of host threads, results in job order (the jobs are NumPy-bound and independent)."""
    n = min(_host_threads(), len(jobs))
    if n <= 1:
        return [fn(j) for j in jobs]
    from concurrent.futures import ThreadPoolExecutor

    with ThreadPoolExecutor(max_workers=n) as pool:
        return list(pool.map(fn, jobs))


def _count_finite(values: np.ndarray, want_mask: bool = False) -> tuple[int, np.ndarray | None]:
    """(number of finite elements, their mask or None) of a host array: ``np.isfinite`` on the library's host threads
    (xdemhip_host_count_finite) for C-contiguous float32 / float64 arrays, NumPy otherwise."""
    if values.dtype in (np.dtype(np.float32), np.dtype(np.float64)) and values.flags.c_contiguous and values.size > 0:
        L = _lib.host_library()
        n = ctypes.c_int64()
        mask = np.empty(values.shape, dtype=np.bool_) if want_mask else None
        rc = L.xdemhip_host_count_finite(ptr(values), _args.code(values), int(values.size), _host_threads(), ctypes.byref(n), ptr(mask))
        if rc != 0:
            raise _lib.XdemHipError(f"xdemhip_host_count_finite: status {rc}")
        return int(n.value), mask
    mask = np.isfinite(values)
    return int(np.count_nonzero(mask)), (mask if want_mask else None)


def _morton_order(x: np.ndarray, y: np.ndarray) -> np.ndarray | None:
    """Permutation that sorts the points along a Z-order curve over their bounding box (16 bits per axis)."""
    if x.size < 3:
        return None
    with np.errstate(invalid="ignore"):
        fin = np.isfinite(x) & np.isfinite(y)
    if not fin.all():
        return None
    x0, y0 = x.min(), y.min()
    spanx, spany = float(x.max() - x0), float(y.max() - y0)
    qx = ((x - x0) * (65535.0 / spanx if spanx > 0 else 0.0)).astype(np.uint32)
    qy = ((y - y0) * (65535.0 / spany if spany > 0 else 0.0)).astype(np.uint32)

    def spread(v):
        v = (v | (v << np.uint32(8))) & np.uint32(0x00FF00FF)
        v = (v | (v << np.uint32(4))) & np.uint32(0x0F0F0F0F)
        v = (v | (v << np.uint32(2))) & np.uint32(0x33333333)
        v = (v | (v << np.uint32(1))) & np.uint32(0x55555555)
        return v

    # (32-bit keys and NumPy's default sort -- the vectorised quicksort, 5x the stable merge sort on 3e5 keys; points that share a
    #  cell of the 65536^2 grid may come out in either order, which the pair sums and medians do not depend on)
    return np.argsort(spread(qx) | (spread(qy) << np.uint32(1)))


def _morton_sorted_block(b: tuple) -> tuple:
    # (round 6: a Morton order of (log distance from the centre sample, angle) for the B points -- the order with the fewest lag-class
    #  changes per wave in simulation, 0.316 against 0.350 of the wave-pairs -- measured no faster on the GPU: exact Dowd 41.3 -> 41.6 ms on
    #  C5, Matheron pass 31.1 -> 31.7: profiles/r06_vario_class_change_sim.txt)
    out = list(np.asarray(c) for c in b)
    for k in range(0, len(out), 3):
        o = _morton_order(np.asarray(out[k], dtype=np.float64).ravel(), np.asarray(out[k + 1], dtype=np.float64).ravel())
        if o is not None:
            out[k], out[k + 1], out[k + 2] = (np.asarray(out[k]).ravel()[o], np.asarray(out[k + 1]).ravel()[o], np.asarray(out[k + 2]).ravel()[o])
    return tuple(out)


class _Blocks(list):
    """A list of pair blocks that also carries them PACKED -- the concatenated arrays and offsets `xdemhip_pairs_create` takes --
    in the caller's order (`packed`) and in Morton order (`packed_sorted`): what the native sampler produces in one go, so that
    PairSet neither concatenates nor sorts again."""
    packed = None
    packed_sorted = None


def _native_equidistant_blocks(values2d: np.ndarray, valid2d, gsd: float, centres: list, rings: list, samples: int, seed: int) -> "_Blocks":
    """The draws of `equidistant_blocks_from_raster` by the library's host-side sampler (csrc/hostprep.hip: xdemhip_host_ring_sample, one
    random stream per (run, ring), std::threads over them) + the gather of coordinates and values, once in the order drawn and once
    in Morton order (xdemhip_host_gather_points).  rings[0] is the centre disk, rings[1:] the B rings, inner to outer."""
    L = _lib.host_library()
    ny, nx = values2d.shape
    runs, nr, thr = len(centres), len(rings), _host_threads()
    cx = np.ascontiguousarray([c[0] for c in centres], dtype=np.int64)
    cy = np.ascontiguousarray([c[1] for c in centres], dtype=np.int64)
    lo = np.ascontiguousarray([r[0] for r in rings], dtype=np.float64)
    hi = np.ascontiguousarray([r[1] for r in rings], dtype=np.float64)
    idx = np.empty((runs, nr, samples), dtype=np.int64)
    cnt = np.empty((runs, nr), dtype=np.int64)
    vmask = None if valid2d is None else np.ascontiguousarray(valid2d, dtype=np.bool_).view(np.uint8)
    rc = L.xdemhip_host_ring_sample(ptr(vmask), ny, nx, float(gsd), runs, i64p(cx), i64p(cy), nr, dp(lo), dp(hi), int(samples),
                                    ctypes.c_uint64(seed & (2**64 - 1)), thr, i64p(idx), i64p(cnt))
    if rc != 0:
        raise _lib.XdemHipError(f"xdemhip_host_ring_sample: status {rc}")
    # runs whose centre disk or rings came out empty are dropped (as the NumPy form drops them)
    na, nb = cnt[:, 0], cnt[:, 1:].sum(axis=1)
    keep = np.flatnonzero((na > 0) & (nb > 0))
    a_idx = np.concatenate([idx[r, 0, :na[r]] for r in keep]) if keep.size else np.empty(0, dtype=np.int64)
    b_idx = (np.concatenate([idx[r, k, :cnt[r, k]] for r in keep for k in range(1, nr)]) if keep.size else np.empty(0, dtype=np.int64))
    a_off = np.concatenate(([0], np.cumsum(na[keep]))).astype(np.int64)
    b_off = np.concatenate(([0], np.cumsum(nb[keep]))).astype(np.int64)
    vals = np.ascontiguousarray(values2d)
    dt = _args.code(vals)

    def gather(off, flat):   # -> (x, y, v) in the order drawn, (x, y, v) in Morton order
        outs = [np.empty(flat.size, dtype=np.float64), np.empty(flat.size, dtype=np.float64), np.empty(flat.size, dtype=vals.dtype),
                np.empty(flat.size, dtype=np.float64), np.empty(flat.size, dtype=np.float64), np.empty(flat.size, dtype=vals.dtype)]
        rc_ = L.xdemhip_host_gather_points(ptr(vals), dt, nx, float(gsd), int(off.size - 1), i64p(off), i64p(flat), thr, dp(outs[0]),
                                           dp(outs[1]), ptr(outs[2]), dp(outs[3]), dp(outs[4]), ptr(outs[5]))
        if rc_ != 0:
            raise _lib.XdemHipError(f"xdemhip_host_gather_points: status {rc_}")
        return outs

    out = _Blocks()
    ax, ay, av, sax, say, sav = gather(a_off, a_idx)
    bx, by, bv, sbx, sby, sbv = gather(b_off, b_idx)
    out.packed = (a_off, ax, ay, av, b_off, bx, by, bv)
    out.packed_sorted = (a_off, sax, say, sav, b_off, sbx, sby, sbv)
    for k in range(keep.size):
        sa, sb = slice(a_off[k], a_off[k + 1]), slice(b_off[k], b_off[k + 1])
        out.append((ax[sa], ay[sa], av[sa], bx[sb], by[sb], bv[sb]))
    out.kept_runs = keep
    return out


class PairSet(_lib._Plan):
    """Device-resident pair blocks + lag edges (``xdemhip_pairs``).  ``blocks`` is a list of (ax, ay, av, bx, by, bv)
    (every a with every b) or (ax, ay, av) (all i < j)."""

    def __init__(self, blocks: list[tuple], right_edges, ctx: _lib.Context | None = None, selection: bool = True):
        """``selection=False``: the caller will only ask for sums (Matheron / Cressie) -- the copy in the caller's order, which only the
        exact-median selection reads, is not made (half the uploads and lattice scans of the construction)."""
        if not blocks:
            raise ValueError("at least one pair block is required")
        pd = len(blocks[0]) == 3
        if any((len(b) == 3) != pd for b in blocks):
            raise ValueError("cannot mix pdist and cdist blocks")
        self.ctx = ctx or _lib.default_context()
        self.ctx.adopt(self)
        vdt = np.float64 if any(np.asarray(b[2]).dtype == np.float64 for b in blocks) else np.float32
        # option "vario_diff" = 1: |dv| in float64 whatever the value dtype (values are widened).  Float32 inputs then also get a
        # float32 SHADOW of the set for the exact-median route (below): same medians, the passes at float32 speed
        widened = bool(self.ctx.options.get("vario_diff")) and vdt == np.float32
        if self.ctx.options.get("vario_diff"):
            vdt = np.float64
        # TWO device copies of the pair set (same pairs, different slot order):
        #  * `handle` -- points in MORTON ORDER within each block (neighbouring slots = neighbouring points) for the sum passes
        #    (Matheron / Cressie): the pair kernels accumulate run-length, a lane keeps the sum of its current lag class in
        #    registers and touches the LDS accumulators only when the class changes, and consecutive B points of one
        #    neighbourhood mostly share the class (2.1 -> 2.7 Tpairs/s on SURVEY 8d's C5 input);
        #  * `handle_sel` -- the caller's order for the exact-median selection (Dowd): the SAMPLED digit passes that place the
        #    brackets assume tiles that are no spatial clusters.  The one pass over all pairs (counting against the brackets,
        #    compacting the candidates) reads the Morton copy through ``xdemhip_pairs_link_sorted`` and counts run-length
        #    (round 4; round 2 measured 88 -> 590 ms for that pass on sorted tiles when the brackets held 5 % of the pairs and the
        #    staging buffer had no spill path -- both changed since).
        # Counts and medians do not depend on the order; float64 sums agree to rounding.  Option "vario_sort" = 0: one copy.
        cat = lambda bl, i, dt: np.ascontiguousarray(np.concatenate([np.asarray(b[i], dtype=dt).ravel() for b in bl]))
        off = lambda i: np.ascontiguousarray(np.concatenate([[0], np.cumsum([np.asarray(b[i]).size for b in blocks])]), dtype=np.int64)
        self.edges = np.ascontiguousarray(right_edges, dtype=np.float64)
        self.nb = int(self.edges.size)
        self.vdtype = np.dtype(vdt)
        self.key_bits = 32 if vdt == np.float32 else 64

        def create(bl, vdt=vdt, packed=None):
            if packed is not None and not pd and packed[3].dtype == np.dtype(vdt):
                keep = [np.ascontiguousarray(a) for a in packed]
            else:
                keep = [off(0), cat(bl, 0, np.float64), cat(bl, 1, np.float64), cat(bl, 2, vdt)]
                if not pd:
                    keep += [off(3), cat(bl, 3, np.float64), cat(bl, 4, np.float64), cat(bl, 5, vdt)]
            p = [ptr(a) for a in keep] + ([None] * 4 if pd else [])
            h, n_pairs = ctypes.c_void_p(), ctypes.c_int64()
            self.ctx.check(self.ctx._L.xdemhip_pairs_create(
                self.ctx.handle, len(bl), p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7],
                _args.code(vdt), ptr(self.edges), self.nb, _lib.HOST, ctypes.byref(h), ctypes.byref(n_pairs)))
            return h, int(n_pairs.value)

        self.handle = self.handle_sel = None
        self.shadow = self.shadow_sel = None
        def create_sorted():
            if getattr(blocks, "packed_sorted", None) is not None and not pd:
                return create(blocks, packed=blocks.packed_sorted)
            return create(_host_map(_morton_sorted_block, list(blocks)))

        if not selection and self.ctx.options.get("vario_sort", 1):
            # sums only: the Morton-ordered copy alone (it also answers a selection, should one be asked for after all)
            self.handle, self.n_pairs = create_sorted()
            self.handle_sel = self.handle
        else:
            self.handle_sel, self.n_pairs = create(blocks, packed=getattr(blocks, "packed", None))
            if self.ctx.options.get("vario_sort", 1):
                try:
                    self.handle, n2 = create_sorted()
                except Exception:
                    self.close()
                    raise
                assert n2 == self.n_pairs
                # the selection's one pass over all pairs reads the sorted copy (run-length counters, csrc/variogram.hip)
                self.ctx.check(self.ctx._L.xdemhip_pairs_link_sorted(self.handle_sel, self.handle))
            else:
                self.handle = self.handle_sel
        # float64 differences of float32 values, large sets (the bracketed route's domain, csrc/variogram.hip: PAIRS_BRACKET_MIN):
        # float32 copies of both orders, linked as the shadow of the float64 selection set (xdemhip_pairs_link_shadow)
        takes = ctypes.c_int(0)
        if widened and selection:   # (the library knows its own route: size threshold, classes per sweep, selection mode, reduction hook)
            self.ctx.check(self.ctx._L.xdemhip_pairs_takes_brackets(self.handle_sel, ctypes.byref(takes)))
        if widened and takes.value:
            try:
                with self.ctx.option_scope("vario_diff", 0):   # (the library itself widens float32 values under the option: not the shadow's)
                    self.shadow_sel, _ = create(blocks, np.float32)
                    if self.ctx.options.get("vario_sort", 1):
                        self.shadow, _ = create([_morton_sorted_block(b) for b in blocks], np.float32)
                        self.ctx.check(self.ctx._L.xdemhip_pairs_link_sorted(self.shadow_sel, self.shadow))
                self.ctx.check(self.ctx._L.xdemhip_pairs_link_shadow(self.handle_sel, self.shadow_sel))
            except Exception:
                self.close()
                raise

    def sums(self, kind: int):
        s = np.zeros(self.nb, dtype=np.float64)
        c = np.zeros(self.nb, dtype=np.int64)
        self.ctx.check(self.ctx._L.xdemhip_pairs_sums(self.handle, kind, dp(s), i64p(c)))
        return s, c

    def hist(self, shift: int, first: bool, prefix: np.ndarray | None) -> np.ndarray:
        h = np.zeros((self.nb, 256), dtype=np.uint64)
        pp = _args.u64p(np.ascontiguousarray(prefix, dtype=np.uint64)) if prefix is not None else None
        self.ctx.check(self.ctx._L.xdemhip_pairs_hist(self.handle_sel, shift, int(first), pp, _args.u64p(h)))
        return h

    def succ(self, key: np.ndarray) -> np.ndarray:
        out = np.zeros(self.nb, dtype=np.uint64)
        self.ctx.check(self.ctx._L.xdemhip_pairs_succ(self.handle_sel, _args.u64p(np.ascontiguousarray(key, dtype=np.uint64)), _args.u64p(out)))
        return out

    def close(self) -> None:
        h, hs = getattr(self, "handle", None), getattr(self, "handle_sel", None)
        if not getattr(self.ctx, "handle", None):   # (the context is gone and took the sets with it)
            self.handle = self.handle_sel = None
            return
        sh, shs = getattr(self, "shadow", None), getattr(self, "shadow_sel", None)
        if shs:
            if hs:
                self.ctx._L.xdemhip_pairs_link_shadow(hs, None)
            if sh:
                self.ctx._L.xdemhip_pairs_link_sorted(shs, None)
                self.ctx._L.xdemhip_pairs_destroy(sh)
            self.ctx._L.xdemhip_pairs_destroy(shs)
        self.shadow = self.shadow_sel = None
        if hs and h and hs.value != h.value:
            self.ctx._L.xdemhip_pairs_link_sorted(hs, None)
        if h:
            self.ctx._L.xdemhip_pairs_destroy(h)
        if hs and (not h or hs.value != h.value):
            self.ctx._L.xdemhip_pairs_destroy(hs)
        self.handle = self.handle_sel = None


def _key_to_value(key: np.ndarray, bits: int) -> np.ndarray:
    """Inverse of the variogram key map (csrc/variogram.hip key_abs): key = IEEE bits of |dv| shifted left by one."""
    if bits == 32:
        return (key.astype(np.uint64) >> np.uint64(1)).astype(np.uint32).view(np.float32)
    return (key.astype(np.uint64) >> np.uint64(1)).view(np.float64)


def _allreduce(arr: np.ndarray, group=None) -> np.ndarray:
    """Sum an integer / float64 host array over the ranks of the process group (no-op when not distributed)."""
    try:
        import torch
        import torch.distributed as dist
    except Exception:  # pragma: no cover
        return arr
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) == 1:
        return arr
    dev = "cuda" if dist.get_backend(group) == "nccl" else "cpu"
    t = torch.from_numpy(arr.view(np.int64) if arr.dtype == np.uint64 else arr).to(dev)
    dist.all_reduce(t, op=dist.ReduceOp.SUM, group=group)
    out = t.cpu().numpy()
    return out.view(np.uint64) if arr.dtype == np.uint64 else out


def class_medians(pairs: PairSet, group=None):
    """Exact per-class median of |dv| (np.median semantics) + counts (``xdemhip_pairs_medians``): radix selection with the
    state on the device, bracketed for large pair sets.  With an initialised process group every rank holds its share of the
    blocks; the integer histograms / counters are combined through the library's reduction hook (exact)."""
    ctx = pairs.ctx
    hooked = group is not None or _dist_on()
    if hooked:
        ctx.set_allreduce("world" if group is None else group)
    try:
        counts = np.zeros(pairs.nb, dtype=np.int64)
        med = np.full(pairs.nb, np.nan)
        ctx.check(ctx._L.xdemhip_pairs_medians(pairs.handle_sel, i64p(counts), dp(med)))
    finally:
        if hooked:
            ctx.set_allreduce(None)
    return med, counts


def class_medians_host_driven(pairs: PairSet, group=None):
    """The same selection advanced on the host from raw digit histograms (``xdemhip_pairs_hist`` / ``_succ``): the
    pass-by-pass form of the C-ABI, kept as an independent cross-check of ``class_medians``."""
    nb, bits = pairs.nb, pairs.key_bits
    passes = bits // 8
    prefix = np.zeros(nb, dtype=np.uint64)
    n_less = np.zeros(nb, dtype=np.uint64)
    count = rank = n_eq = None
    rows = np.arange(nb)
    for p in range(passes):
        shift = 8 * (passes - 1 - p)
        h = _allreduce(pairs.hist(shift, p == 0, None if p == 0 else prefix), group)
        if p == 0:
            count = h.sum(axis=1)
            rank = np.where(count > 0, (count - np.uint64(1)) // np.uint64(2), np.uint64(0)).astype(np.uint64)
        cum = np.cumsum(h, axis=1)
        d = np.minimum((cum > rank[:, None]).argmax(axis=1), 255)
        d = np.where(count > 0, d, 0)
        before = cum[rows, d] - h[rows, d]
        prefix |= d.astype(np.uint64) << np.uint64(shift)
        n_less += before
        rank = rank - before
        if p == passes - 1:
            n_eq = h[rows, d]
    n_le = n_less + n_eq
    k2 = count // np.uint64(2)
    even = (count > 0) & (count % np.uint64(2) == 0)
    lo = _key_to_value(prefix, bits)
    hi = lo.copy()
    need = even & (n_le <= k2)
    if _allreduce(np.array([int(need.any())], dtype=np.int64), group)[0]:
        s = pairs.succ(prefix)
        if group is not None or _dist_on():
            s = _allreduce_min(s, group)
        hi = np.where(need, _key_to_value(s, bits), lo)
    med = np.where(even, ((lo + hi) / lo.dtype.type(2)).astype(lo.dtype), lo).astype(np.float64)
    med[count == 0] = np.nan
    return med, count.astype(np.int64)


def _dist_on() -> bool:
    try:
        import torch.distributed as dist

        return dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1
    except Exception:  # pragma: no cover
        return False


def _allreduce_min(arr: np.ndarray, group=None) -> np.ndarray:
    import torch
    import torch.distributed as dist

    if not _dist_on():
        return arr
    dev = "cuda" if dist.get_backend(group) == "nccl" else "cpu"
    # uint64 keys: compare as two int64 halves is overkill -- keys of |dv| are < 2^63, all-ones means "none"
    t = torch.from_numpy(np.where(arr == np.uint64(0xFFFFFFFFFFFFFFFF), np.uint64(0x7FFFFFFFFFFFFFFF), arr).view(np.int64)).to(dev)
    dist.all_reduce(t, op=dist.ReduceOp.MIN, group=group)
    return t.cpu().numpy().view(np.uint64)


def empirical_variogram_pairs(blocks: list[tuple], right_edges, estimator: str = "matheron", ctx: _lib.Context | None = None,
                              group=None):
    """(exp float64[n], count int64[n]) of the pair blocks: the stand-in for ``skg.Variogram(...).get_empirical()``
    / ``.bin_count``.  With an initialised process group every rank passes ITS share of the blocks and all ranks
    receive the combined result (counts, sums and histograms are all-reduced)."""
    estimator = estimator.lower()
    if estimator not in _ESTIMATORS:
        raise ValueError(f"estimator must be one of {_ESTIMATORS}")
    pairs = PairSet(blocks, right_edges, ctx, selection=estimator == "dowd")
    try:
        if estimator == "dowd":
            med, count = class_medians(pairs, group)
            # per class as scalars: `median ** 2` on a float64 scalar goes through libm's pow (what scikit-gstat's scalar
            # expression and the oracle evaluate), which can differ from an array square in the last bit
            exp = np.array([2.198 * float(m) ** 2 / 2 for m in med], dtype=np.float64)
        else:
            s, count = pairs.sums(0 if estimator == "matheron" else 1)
            s, count = _allreduce(s, group), _allreduce(count, group)
            n = count.astype(np.float64)
            with np.errstate(divide="ignore", invalid="ignore"):
                if estimator == "matheron":
                    exp = s / (2 * n)
                else:
                    exp = 0.5 * (s / n) ** 4 / (0.457 + 0.494 / n + 0.045 / n**2)
            exp[count == 0] = np.nan
        return exp, count
    finally:
        pairs.close()


# ---- host preparation mirrored from the reference --------------------------------------------------------------
def _pair_budget_split(n_pairs_per_ring: float) -> tuple[int, int]:
    """How a ring's pair budget is spread over independent runs: (runs, points per run and ring).  Budgets below 10 pairs run
    budget / 4 times; otherwise 10 x ceil(cbrt(budget / 40)) runs capped at 100; each run then draws ceil(sqrt(budget / runs))
    points.  Integer results pinned by tests/golden (T7 table recorded from the reference)."""
    if n_pairs_per_ring < 10:
        n_runs = int(n_pairs_per_ring / 4)
    else:
        n_runs = int(min(100, 10 * np.ceil((n_pairs_per_ring / 40) ** (1 / 3))))
    return n_runs, int(np.ceil(np.sqrt(n_pairs_per_ring / n_runs)))


def _choose_cdist_equidistant_sampling_parameters(**kwargs: Any) -> tuple[int, int, float]:
    """(runs, samples, ratio_subsample) of the equidistant sampler for a pair budget of subsample^2 / 2 spread over `nb_rings`
    rings (default 10) -- the integer rule and the disk ratio of xdem/spatialstats.py:1104-1183, which the T7 fixture table pins."""
    n_rings = kwargs.get("nb_rings", 10)
    budget_points = kwargs["subsample"]
    fewest = np.ceil(np.sqrt(8 * n_rings) + 1)   # two points per ring pair at the very least
    if budget_points < fewest:
        raise ValueError(f"The number of subsamples needs to be at least {fewest:.0f}.")
    runs, per_run = _pair_budget_split(np.ceil(budget_points**2 / (2 * n_rings)))

    x0, x1, y0, y1 = kwargs["extent"][:4]
    ny, nx = kwargs["shape"][:2]
    diagonal = np.sqrt((x1 - x0) ** 2 + (y1 - y0) ** 2)
    pixel = 0.5 * ((x1 - x0) / (ny - 1) + (y1 - y0) / (nx - 1))
    # the centre disk is the innermost of rings whose radii grow by sqrt(2): its area is the extent circle's / 2^rings
    centre_disk_area = np.pi * diagonal**2 / np.sqrt(2) ** (2 * n_rings)
    ratio = pixel**2 * per_run / centre_disk_area
    logging.info("equidistant sampling: %d runs x (%d centre-disk points against %d points in each of %d rings) = about %d pairs",
                 runs, per_run, per_run, n_rings, runs * per_run**2 * n_rings)
    return runs, per_run, ratio


# The keyword arguments `sample_empirical_variogram` forwards (upstream's typing aid of the same name, xdem/spatialstats.py:1284-1292)
EmpiricalVariogramKArgs = TypedDict("EmpiricalVariogramKArgs", {"runs": int, "pdist_multi_ranges": list, "ratio_subsample": float, "samples": int,
                                                                "nb_rings": int, "maxlag": float, "bin_func": Any, "estimator": str}, total=False)


def sample_empirical_variogram(values, gsd: float = None, coords: np.ndarray = None, subsample: int = 1000,
                               subsample_method: str = "cdist_equidistant", n_variograms: int = 1, n_jobs: int = 1,
                               random_state=None, **kwargs: Any):
    """Sample empirical variograms; drop-in for ``xdem.spatialstats.sample_empirical_variogram`` (1295-1546).

    Returns a DataFrame with the empirical variance ``exp``, the upper bound of the lag ``lags``, the pair ``count``
    and ``err_exp`` (NaN for a single run), the last -- always under-sampled -- lag removed.
    All five ``subsample_method`` values are supported: "cdist_equidistant" (default), "cdist_point", "pdist_point" and the
    multi-range "pdist_disk" / "pdist_ring"; the random draws inside them belong to un-vendored dependencies (skgstat metric
    spaces, ``geoutils.subsample_array``) and are restated with NumPy generators -- parity of the *draws* is unpinned, the
    pair arithmetic is what the tests pin.
    """
    import pandas as pd

    if hasattr(values, "res") and hasattr(values, "data"):  # Raster-like
        gsd = values.res[0]
        values = values.data
    if isinstance(values, np.ma.MaskedArray):
        arr = np.array(values.data, dtype=values.dtype if np.issubdtype(values.dtype, np.floating) else np.float32, copy=True)
        arr[np.ma.getmaskarray(values)] = np.nan
        values = arr
    elif isinstance(values, np.ndarray):
        # (upstream copies its input before filtering it; nothing below writes to the array, and a copy of a 20000^2 raster is 0.15 s)
        if np.issubdtype(values.dtype, np.integer):
            values = values.astype(np.float32)
    else:
        raise ValueError("Values must be of type NDArrayf, np.ma.masked_array or Raster subclass.")
    values = values.squeeze()

    # argument rules of upstream (xdem/spatialstats.py:1366-1400; messages as its tests assert them), first violated rule wins
    raster_methods = ("cdist_equidistant", "pdist_disk", "pdist_ring")
    all_methods = raster_methods[:1] + ("cdist_point", "pdist_point") + raster_methods[1:]
    flat, gridded = values.ndim == 1, values.ndim == 2
    shape_rules = (
        (flat and (gsd is not None or subsample_method in raster_methods),
         'Values array must be 2D when using any of the "cdist_equidistant", "pdist_disk" and '
         '"pdist_ring" methods, or providing a ground sampling distance instead of coordinates.'),
        (coords is not None and not flat, "Values array must be 1D when providing coordinates."),
        (coords is not None and 2 not in coords.shape[:2], "The coordinates array must have one dimension with length equal to 2"),
        (gridded and gsd is None, "The ground sampling distance must be defined when passing a 2D values array."),
    )
    for violated, message in shape_rules:
        if violated:
            raise ValueError(message)
    if subsample_method not in all_methods:
        raise TypeError('The subsampling method must be one of "cdist_equidistant, "cdist_point", "pdist_point", '
                        '"pdist_disk" or "pdist_ring".')
    named_bin_func = "bin_func" in kwargs and not isinstance(kwargs["bin_func"], Iterable)
    if named_bin_func and n_variograms > 1:
        warnings.warn("Using a named binning function of scikit-gstat might provide different binnings for each "
                      "independent run. To remediate that issue, pass bin_func as an Iterable of right bin edges, "
                      "(or use default bin_func).")
    if "bin_func" in kwargs and not isinstance(kwargs["bin_func"], Iterable):
        raise NotImplementedError("bin_func must be an iterable of right bin edges, 'even' (or omitted) on the GPU path.")
    # scikit-gstat's named binnings (strings -- Iterables to the check above, as upstream): 'even' needs nothing but maxlag and
    # n_lags (skgstat.binning.even_width_lags: linspace(0, maxlag, n_lags + 1)[1:]); the others ('uniform', 'fd', 'sturges',
    # 'scott', 'doane', 'sqrt', 'kmeans', 'ward', 'stable_entropy') are functions of the sampled pair distances of each run --
    # exactly the per-run binnings upstream warns about -- and are refused
    if isinstance(kwargs.get("bin_func"), str) and kwargs["bin_func"] != "even":
        raise NotImplementedError(f"bin_func='{kwargs['bin_func']}': of scikit-gstat's named binnings only 'even' is available on the "
                                  "GPU path; pass bin_func as an Iterable of right bin edges (or use default bin_func).")

    shape2d = None
    if coords is not None:
        if coords.shape[0] == 2 and coords.shape[1] != 2:
            coords = np.transpose(coords)
    else:
        # Upstream builds meshgrid(arange(0, shape[0] gsd, gsd), arange(0, shape[1] gsd, gsd)) and pairs it with the C-order
        # flattening of the values as is (spatialstats.py:1413-1416): flat element k sits at x = (k % shape[0]) gsd,
        # y = (k // shape[0]) gsd.  The coordinates are formed on demand from k (a 20000^2 raster would need 6.4 GB of them).
        shape2d = values.shape
        values = values.reshape(-1)   # (a view of a C-contiguous raster; upstream's flatten() copies)
    if gsd is None:
        gsd = np.mean([coords[0, 0] - coords[0, 1], coords[0, 0] - coords[1, 0]])
    if coords is not None:
        extent = (np.min(coords[:, 0]), np.max(coords[:, 0]), np.min(coords[:, 1]), np.max(coords[:, 1]))
        xy_of = lambda k: (coords[k, 0], coords[k, 1])
    else:
        extent = (0.0, float(np.arange(shape2d[0])[-1] * gsd), 0.0, float(np.arange(shape2d[1])[-1] * gsd))
        xy_of = lambda k: ((np.asarray(k) % shape2d[0]) * gsd, (np.asarray(k) // shape2d[0]) * gsd)
    if "maxlag" not in kwargs:
        kwargs["maxlag"] = np.sqrt((extent[1] - extent[0]) ** 2 + (extent[3] - extent[2]) ** 2)
    if "bin_func" not in kwargs:
        bin_func = []
        right_bin_edge = np.sqrt(2) * gsd
        while right_bin_edge < kwargs["maxlag"]:
            bin_func.append(right_bin_edge)
            right_bin_edge *= np.sqrt(2)
        bin_func.append(kwargs["maxlag"])
        kwargs["bin_func"] = bin_func
    # 'even' (checked above; n_lags: scikit-gstat's default is 10): skgstat.binning.even_width_lags(distances, n, maxlag) first CLIPS
    # maxlag to nanmax(distances) of the sampled pairs -- and upstream's default maxlag, the extent diagonal, is practically always
    # larger -- so the edges are linspace(0, min(maxlag, largest sampled pair distance), n_lags + 1)[1:], per Variogram object:
    # formed below for every pair set (`edges_for`), with the largest distance taken from the hulls of the point sets
    even_lags = int(kwargs.get("n_lags", 10)) if isinstance(kwargs["bin_func"], str) else None
    edges = None if even_lags is not None else np.asarray(list(kwargs["bin_func"]), dtype=np.float64)
    estimator = kwargs.get("estimator", "matheron")

    def edges_for(blocks):
        if even_lags is None:
            return edges
        dmax = _max_pair_distance(blocks)
        top = kwargs["maxlag"] if not (dmax < kwargs["maxlag"]) else dmax
        return np.linspace(0, top, even_lags + 1)[1:]

    if random_state is not None:
        rng = np.random.default_rng(random_state)
        list_random_state = list(rng.choice(n_variograms, n_variograms, replace=False))
    else:
        list_random_state = [None for _ in range(n_variograms)]

    # np.isfinite over the whole raster (upstream's NaN filter): counted on the host threads of the library; the mask itself is formed
    # only if something is not finite, and only where a sampler needs it (0.2 s + 400 MB for a 20000^2 raster otherwise)
    n_finite, valid = _count_finite(values)
    all_valid = n_finite == values.size

    def valid_mask():
        nonlocal valid
        if valid is None:
            valid = np.ones(values.shape, dtype=bool) if all_valid else _count_finite(values, want_mask=True)[1]
        return valid

    list_df_run = []

    def equidistant_blocks(i):
        """The point sets of variogram `i` under ``cdist_equidistant`` (its own generator: nothing it draws depends on the other variograms)."""
        run_rng = np.random.default_rng(list_random_state[i])
        if "runs" in kwargs or "samples" in kwargs:
            # user-defined: upstream only auto-chooses when NEITHER is given (spatialstats.py:1203) and otherwise leaves
            # the missing one to RasterEquidistantMetricSpace's defaults (samples=100, ratio_subsample=0.01,
            # runs = 1 % of the coordinates / samples)
            samples = int(kwargs.get("samples", 100))
            ratio = kwargs.get("ratio_subsample", 0.01)
            runs = int(kwargs["runs"]) if kwargs.get("runs") is not None else int(n_finite * 0.01 / samples)
        else:
            runs, samples, ratio = _choose_cdist_equidistant_sampling_parameters(
                extent=extent, shape=shape2d, subsample=subsample, **({"nb_rings": kwargs["nb_rings"]} if "nb_rings" in kwargs else {}))
        if coords is not None:
            return equidistant_blocks_from_coords(coords, values, valid_mask(), gsd, runs, samples, ratio, run_rng)
        # full raster, indexed (values.shape[0] along x) like upstream's meshgrid call
        return equidistant_blocks_from_raster(values.reshape(shape2d[1], shape2d[0]), gsd, runs, samples, ratio, run_rng,
                                              valid2d=None if all_valid else valid_mask().reshape(shape2d[1], shape2d[0]),
                                              assume_valid=all_valid)

    # Several variograms (the error bars of upstream's n_variograms): the host preparation of the NEXT one -- sampling of the metric
    # space, gathers, Morton-ordered copies: native threaded code that releases the GIL -- runs while the GPU works through the
    # pair passes of the current one (a helper thread, one variogram ahead; every variogram has its own generator, so the numbers
    # drawn do not depend on when)
    ahead = None
    pool = None
    # (not for the largest samples: a prepared variogram of subsample 1e7 is ~12 GB of host arrays, and its passes take 15-20 s
    #  against 3.5 s of preparation -- nothing worth a second copy in memory)
    if subsample_method == "cdist_equidistant" and n_variograms > 1 and subsample <= 2_000_000:
        from concurrent.futures import ThreadPoolExecutor

        pool = ThreadPoolExecutor(max_workers=1)
        ahead = pool.submit(equidistant_blocks, 0)
    try:
        for i in range(n_variograms):
            run_rng = np.random.default_rng(list_random_state[i])
            if subsample_method == "cdist_equidistant" and ahead is not None:
                blocks = ahead.result()
                ahead = pool.submit(equidistant_blocks, i + 1) if i + 1 < n_variograms else None
                if ahead is None:
                    pool.shutdown(wait=False)
                    pool = None
            elif subsample_method == "cdist_equidistant":
                blocks = equidistant_blocks(i)
            elif subsample_method == "cdist_point":
                idx = np.flatnonzero(valid_mask())
                n = min(int(subsample), idx.size)
                a = run_rng.choice(idx, n, replace=False)
                b = run_rng.choice(idx, n, replace=False)
                blocks = [xy_of(a) + (values[a],) + xy_of(b) + (values[b],)]
            elif subsample_method == "pdist_point":
                idx = np.flatnonzero(valid_mask())
                a = run_rng.choice(idx, min(int(subsample), idx.size), replace=False)
                blocks = [xy_of(a) + (values[a],)]
            else:  # pdist_disk / pdist_ring: one pdist variogram per range, all rows kept (1007-1060)
                for sel in _pdist_multi_range_subsamples(valid_mask(), shape2d, int(subsample), subsample_method, gsd, kwargs["maxlag"],
                                                         kwargs.get("pdist_multi_ranges"), list_random_state[i]):
                    blk = [xy_of(sel) + (values[sel],)]
                    e_run = edges_for(blk)
                    exp, count = empirical_variogram_pairs(blk, e_run, estimator)
                    list_df_run.append(pd.DataFrame().assign(exp=exp, bins=e_run, count=count))
                continue
            e_run = edges_for(blocks) if blocks else (edges if edges is not None else np.linspace(0, kwargs["maxlag"], even_lags + 1)[1:])
            if blocks:
                exp, count = empirical_variogram_pairs(blocks, e_run, estimator)
            else:
                exp, count = np.full(e_run.size, np.nan), np.zeros(e_run.size, dtype=np.int64)
            list_df_run.append(pd.DataFrame().assign(exp=exp, bins=e_run, count=count))
    finally:
        if pool is not None:   # (an exception on the way: the helper thread is not left waiting on the executor)
            pool.shutdown(wait=False, cancel_futures=True)

    every_run = pd.concat(list_df_run)
    if n_variograms == 1:
        table = every_run.rename(columns={"bins": "lags"}).assign(err_exp=np.nan)
    else:
        # one row per lag class over the runs: mean of the estimates, their standard error, pairs added up (pandas' NaN-skipping
        # group reductions, as upstream aggregates its runs: spatialstats.py:1518-1532)
        per_lag = every_run.groupby("bins", dropna=False)
        table = per_lag.agg(exp=("exp", "mean"), spread=("exp", "std"), count=("count", "sum"))
        table["lags"] = table.index.values
        table["err_exp"] = table.pop("spread") / np.sqrt(n_variograms)
        table = table[["exp", "lags", "err_exp", "count"]]
    # the last lag is always under-sampled.  Dropped BY INDEX LABEL, as upstream does (spatialstats.py:1540): the frames of a
    # multi-range run (pdist_disk / pdist_ring) are concatenated with their own 0..n-1 labels, so the last lag of EVERY range goes
    df = table.drop(table.tail(1).index)
    df = df.astype({"exp": "float64", "err_exp": "float64", "lags": "float64", "count": "int64"})
    return df


def _hull_points(x: np.ndarray, y: np.ndarray) -> np.ndarray:
    """Vertices of the convex hull of a point set as an (m, 2) array (all points when the set is tiny or degenerate: collinear
    points have no 2-D hull -- their two extremes along the longer axis of the bounding box, plus the box's corner-most points, do)."""
    pts = np.column_stack([np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)])
    pts = pts[np.isfinite(pts).all(axis=1)]
    if pts.shape[0] <= 64:
        return pts
    try:
        from scipy.spatial import ConvexHull

        return pts[ConvexHull(pts).vertices]
    except Exception:   # degenerate (collinear / duplicate) sets: the extremes of x, y, x + y and x - y hold the farthest pair of a line
        k = [f(v) for v in (pts[:, 0], pts[:, 1], pts[:, 0] + pts[:, 1], pts[:, 0] - pts[:, 1]) for f in (np.argmin, np.argmax)]
        return pts[np.unique(k)]


def _max_pair_distance(blocks) -> float:
    """``np.nanmax`` of the pair distances of a pair set -- what ``skgstat.binning.even_width_lags`` clips ``maxlag`` to -- without
    forming the pairs: the farthest pair of two point sets (or of one) joins two vertices of their convex hulls, and its distance
    is evaluated like SciPy's ``pdist`` / ``cdist`` evaluate it (``sqrt(dx*dx + dy*dy)`` in float64).  `blocks`: (x, y, v) = every
    i < j pair of one set, (xa, ya, va, xb, yb, vb) = every a with every b.  Empty pair sets give 0."""
    best = 0.0
    for blk in blocks:
        a = _hull_points(blk[0], blk[1])
        b = a if len(blk) == 3 else _hull_points(blk[3], blk[4])
        if a.shape[0] == 0 or b.shape[0] == 0 or (len(blk) == 3 and a.shape[0] < 2):
            continue
        for i0 in range(0, a.shape[0], 4096):   # (hulls of lattice points are small; chunked all the same)
            dx = a[i0:i0 + 4096, 0][:, None] - b[None, :, 0]
            dy = a[i0:i0 + 4096, 1][:, None] - b[None, :, 1]
            best = max(best, float(np.sqrt(np.max(dx * dx + dy * dy))))
    return best


def _create_circular_mask(shape: tuple[int, int], center=None, radius=None) -> np.ndarray:
    """Mirror of ``_create_circular_mask`` (xdem/spatialstats.py:880-905), axis convention included (``center[0]`` is
    compared with the second array axis)."""
    w, h = shape
    if center is None:
        center = (int(w / 2), int(h / 2))
    if radius is None:
        radius = min(center[0], center[1], w - center[0], h - center[1])
    Y, X = np.ogrid[:w, :h]
    return np.sqrt((X - center[0]) ** 2 + (Y - center[1]) ** 2) < radius


def _create_ring_mask(shape: tuple[int, int], center=None, in_radius: float = 0, out_radius=None) -> np.ndarray:
    """Mirror of ``_create_ring_mask`` (xdem/spatialstats.py:908-937)."""
    w, h = shape
    if center is None:
        center = (int(w / 2), int(h / 2))
    if out_radius is None:
        out_radius = min(center[0], center[1], w - center[0], h - center[1])
    return np.logical_and(~_create_circular_mask((w, h), center=center, radius=in_radius),
                          _create_circular_mask((w, h), center=center, radius=out_radius))


def _pdist_multi_range_subsamples(valid: np.ndarray, shape: tuple[int, int], subsample: int, subsample_method: str, gsd: float,
                                  maxlag: float, pdist_multi_ranges, random_state) -> list[np.ndarray]:
    """Flat indices of the point subsample of every range of the "pdist_disk" / "pdist_ring" methods
    (``_aggregate_pdist_empirical_variogram`` + ``_subsample_wrapper``, xdem/spatialstats.py:985-1060, 940-982): ranges
    double from 10 gsd up to maxlag / 2, then maxlag; per range a random centre, the disk (or the ring between consecutive
    ranges) around it, and ``subsample`` valid points of it (empty subsamples are skipped).  Every range re-seeds its
    generator with the run's ``random_state``, as upstream does, so a seeded run keeps one centre for all its ranges."""
    if pdist_multi_ranges is None:
        pdist_multi_ranges = []
        new_range = gsd * 10
        while new_range < maxlag / 2:
            pdist_multi_ranges.append(new_range)
            new_range *= 2
        pdist_multi_ranges.append(maxlag)
    nx, ny = shape
    binned = [0.0] + list(pdist_multi_ranges)
    out = []
    for j in range(len(pdist_multi_ranges)):
        outside = binned[j + 1] / gsd
        inside = binned[j] / gsd if subsample_method == "pdist_ring" else 0.0
        rng = np.random.default_rng(random_state)
        center = (rng.choice(nx, 1)[0], rng.choice(ny, 1)[0])
        if subsample_method == "pdist_ring":
            sub = _create_ring_mask((nx, ny), center=center, in_radius=inside, out_radius=outside)
        else:
            sub = _create_circular_mask((nx, ny), center=center, radius=outside)
        idx = np.flatnonzero(sub.flatten() & valid)
        if idx.size == 0:
            continue
        # geoutils.subsample_array(values_sp, subsample, return_indices=True, random_state): its own generator on the same seed
        draw = np.random.default_rng(random_state)
        out.append(draw.choice(idx, min(subsample, idx.size), replace=False))
    return out


def equidistant_blocks_from_coords(coords: np.ndarray, values: np.ndarray, valid: np.ndarray, gsd: float, runs: int,
                                   samples: int, ratio_subsample: float, rng: np.random.Generator,
                                   exp_increase_fac: float = np.sqrt(2)) -> list[tuple]:
    """Centre-disk x equidistant-ring pair blocks (Hugonnet et al. 2022, Suppl. Fig. 13; the scheme of skgstat's
    RasterEquidistantMetricSpace restated -- the package is absent offline, oracle/pin_thirdparty.py records its pair
    structure where it is importable): per run a random valid centre and a "centre sample" of up to `samples` valid
    points of the disk of radius r0 = sqrt(samples / (ratio_subsample pi)) gsd; the "equidistant sample" takes up to
    `samples` valid points of every ring between the radii 0, r0, r0 f, r0 f^2, ... (f = sqrt 2) below the extent diagonal
    and the diagonal itself as the last radius.  Its first ring is the centre disk again, drawn independently ("so that the
    other half can be used by the equidistant sample for low distances"): the short lags come from disk x disk pairs.
    Pairs = centre sample x the union of the ring samples."""
    cx, cy = coords[:, 0], coords[:, 1]
    r0 = np.sqrt(samples / (ratio_subsample * np.pi)) * gsd
    maxdist = np.sqrt((cx.max() - cx.min()) ** 2 + (cy.max() - cy.min()) ** 2)
    radii = [0.0]
    r = r0
    while r < maxdist:
        radii.append(r)
        r *= exp_increase_fac
    radii.append(maxdist)
    flat_valid = np.flatnonzero(valid)
    blocks = []
    for _ in range(runs):
        c = rng.choice(flat_valid)
        dist = np.sqrt((cx - cx[c]) ** 2 + (cy - cy[c]) ** 2)
        # digitize: radii[i] <= d < radii[i+1] -> i; d >= maxdist (the far corner only) falls outside every ring;
        # the centre disk is d < r0 whichever radius list the diagonal cuts short
        ring = np.digitize(dist, radii) - 1
        ring[(~valid) | (ring >= len(radii) - 1)] = -1
        a = np.flatnonzero(valid & (dist < r0))
        if a.size > samples:
            a = rng.choice(a, samples, replace=False)
        sets = []
        for i in range(len(radii) - 1):
            idx = np.flatnonzero(ring == i)
            if idx.size > samples:
                idx = rng.choice(idx, samples, replace=False)
            sets.append(idx)
        b = np.concatenate(sets) if sets else np.array([], dtype=np.int64)
        if a.size and b.size:
            blocks.append((cx[a], cy[a], values[a], cx[b], cy[b], values[b]))
    return blocks


def _equidistant_radii(samples: int, ratio_subsample: float, gsd: float, maxdist: float, exp_increase_fac: float = np.sqrt(2)):
    """Centre-disk radius r0 and the ring bounds 0, r0, r0 f, r0 f^2, ... (< maxdist), maxdist of the equidistant scheme."""
    r0 = np.sqrt(samples / (ratio_subsample * np.pi)) * gsd
    radii = [0.0]
    r = r0
    while r < maxdist:
        radii.append(r)
        r *= exp_increase_fac
    radii.append(maxdist)
    return r0, radii


def _draw_ring_pixels(valid2d, ny: int, nx: int, cxi: int, cyi: int, lo: float, hi: float, gsd: float, samples: int,
                      rng: np.random.Generator) -> np.ndarray:
    """Up to `samples` distinct valid pixels (flat indexes iy * nx + ix) with lo <= distance to pixel (cxi, cyi) < hi, drawn
    uniformly without replacement, without forming the distance of every raster pixel (4e8 of them at 20000^2).  Per raster row
    the ring is two column spans known in closed form (taken one pixel generous); independent uniform draws over the
    concatenated spans, filtered by the exact distance test and the validity mask, are independent uniform draws over the ring;
    the SET of distinct pixels among them is exchangeable over the ring's pixels, so a uniformly random subset of it of the wanted
    size is a uniform sample without replacement (returned in random order).  The draws are sorted before they are mapped to
    pixels (sorted look-ups into the span table run 4x faster than random ones, and duplicates fall out by comparing neighbours).
    Small rings are enumerated instead."""
    reach = int(np.floor(hi / gsd)) + 1
    y0, y1 = max(0, cyi - reach), min(ny - 1, cyi + reach)
    if y1 < y0:
        return np.empty(0, dtype=np.int64)
    rows = np.arange(y0, y1 + 1, dtype=np.int64)
    dy2 = ((rows - cyi).astype(np.float64)) ** 2
    wo = np.floor(np.sqrt(np.maximum((hi / gsd) ** 2 - dy2, 0.0))).astype(np.int64) + 1     # generous outer half width
    wi = np.maximum(np.ceil(np.sqrt(np.maximum((lo / gsd) ** 2 - dy2, 0.0))).astype(np.int64) - 1, 0)  # shrunk inner one
    # left span [cxi - wo, cxi - wi], right span [cxi + max(wi, 1), cxi + wo] (the centre column belongs to the left span)
    la, lb = np.maximum(cxi - wo, 0), np.minimum(cxi - wi, nx - 1)
    ra, rb = np.maximum(cxi + np.maximum(wi, 1), 0), np.minimum(cxi + wo, nx - 1)
    nl, nr = np.maximum(lb - la + 1, 0), np.maximum(rb - ra + 1, 0)
    cum = np.cumsum(nl + nr)
    total = int(cum[-1])
    if total == 0:
        return np.empty(0, dtype=np.int64)
    start = cum - (nl + nr)

    def pixels(k):  # k-th candidate of the concatenated spans -> (ix, iy)
        r = np.searchsorted(cum, k, side="right")
        o = k - start[r]
        left = o < nl[r]
        return np.where(left, la[r] + o, ra[r] + (o - nl[r])), rows[r]

    def exact(ix, iy):
        d = np.sqrt(((ix - cxi) * gsd) ** 2 + ((iy - cyi) * gsd) ** 2)
        ok = (d >= lo) & (d < hi)
        if valid2d is not None:
            ok &= valid2d[iy, ix]
        return ok

    def enumerate_all():
        out = []
        for k0 in range(0, total, 1 << 24):
            ix, iy = pixels(np.arange(k0, min(total, k0 + (1 << 24)), dtype=np.int64))
            ok = exact(ix, iy)
            out.append(iy[ok] * nx + ix[ok])
        idx = np.concatenate(out)
        return rng.choice(idx, samples, replace=False) if idx.size > samples else idx

    if total <= max(1 << 16, 4 * samples):
        return enumerate_all()
    kept = np.empty(0, dtype=np.int64)    # distinct ring pixels met so far, ascending
    batch = int(1.3 * samples) + 64
    drawn = accepted = 0
    for _ in range(16):
        k = rng.integers(0, total, batch)
        k.sort()
        k = k[np.concatenate(([True], k[1:] != k[:-1]))]
        ix, iy = pixels(k)
        ok = exact(ix, iy)
        drawn += batch
        accepted += int(ok.sum())
        new = iy[ok] * nx + ix[ok]          # (ascending: rows ascend with k, within a row the left span lies left of the right one)
        kept = new if kept.size == 0 else np.union1d(kept, new)
        if kept.size >= samples:
            return rng.choice(kept, samples, replace=False)
        if accepted * (total / drawn) < 1.5 * samples:   # about as many (valid) ring pixels as wanted, or fewer: take them all
            return enumerate_all()
        batch = int(min(4e7, 1.5 * (samples - kept.size) * drawn / max(accepted, 1))) + 64
    return enumerate_all()


def equidistant_blocks_from_raster(values2d: np.ndarray, gsd: float, runs: int, samples: int, ratio_subsample: float,
                                   rng: np.random.Generator, valid2d: np.ndarray | None = None,
                                   exp_increase_fac: float = np.sqrt(2), values_of=None, shape=None,
                                   centres_out: list | None = None, native: bool | None = None, assume_valid: bool = False) -> list[tuple]:
    """The centre-disk x equidistant-ring scheme of `equidistant_blocks_from_coords` for a full raster (pixel (iy, ix) at
    x = ix gsd, y = iy gsd), drawn ring by ring without forming the distance of every pixel to the centre: same disk and ring
    definitions (centre sample = valid pixels with d < r0; rings [0, r0), [r0, r0 f), ... the last one ending at the extent
    diagonal; up to `samples` pixels of each), uniform without replacement.  RNG protocol: centre by rejection among the
    valid pixels, then `_draw_ring_pixels` for the centre sample and for each ring, inner to outer.  `values_of(flat_idx)`
    may supply the values (e.g. a gather from a device-resident raster; then `values2d` may be None and `shape` = (ny, nx)
    names the raster).  With a host raster the draws, the gather and the Morton-ordered copies the pair kernels want are made by the
    library's native host code on all cores (csrc/hostprep.hip; `native=False` keeps the NumPy form below, which is its
    specification: same rings, same uniform-without-replacement law, other random streams)."""
    ny, nx = values2d.shape if values2d is not None else (valid2d.shape if valid2d is not None else shape)
    maxdist = np.sqrt(((nx - 1) * gsd) ** 2 + ((ny - 1) * gsd) ** 2)
    r0, radii = _equidistant_radii(samples, ratio_subsample, gsd, maxdist, exp_increase_fac)
    if valid2d is None and values2d is not None and not assume_valid:   # (assume_valid: the caller has looked already)
        valid2d = np.isfinite(values2d)
        if valid2d.all():
            valid2d = None
    get = values_of if values_of is not None else (lambda idx: values2d.reshape(-1)[idx])
    # RNG protocol (round 6): the centres of all runs first, from `rng`; then one child generator per run (`rng.spawn`), so that
    # the runs -- independent of each other -- are drawn by a pool of host threads (NumPy releases the GIL in the sorts, look-ups
    # and gathers that make up a draw) and still come out the same for the same seed whatever the number of threads
    centres = []
    for _ in range(runs):
        for _try in range(10000):
            cyi, cxi = int(rng.integers(0, ny)), int(rng.integers(0, nx))
            if valid2d is None or valid2d[cyi, cxi]:
                break
        else:
            break  # (practically) no valid pixel
        centres.append((cxi, cyi))
    if (native is not False and values_of is None and values2d is not None and values2d.dtype in (np.dtype(np.float32), np.dtype(np.float64))
            and centres and _lib.host_library(required=False) is not None):
        # the library's host-side sampler: same rings, same distribution, its own random streams seeded from `rng`
        rings = [(0.0, r0)] + list(zip(radii[:-1], radii[1:]))
        blocks = _native_equidistant_blocks(values2d, valid2d, gsd, centres, rings, samples, int(rng.integers(0, 2**63)))
        if centres_out is not None:
            centres_out.extend(centres[k] for k in blocks.kept_runs)
        return blocks
    try:
        children = rng.spawn(len(centres))
    except (AttributeError, TypeError):   # (a Generator over a bit generator without a seed sequence)
        children = [np.random.default_rng(int(s_)) for s_ in rng.integers(0, 2**63, len(centres))]

    def one_run(job):
        (cxi, cyi), run_rng = job
        a = _draw_ring_pixels(valid2d, ny, nx, cxi, cyi, 0.0, r0, gsd, samples, run_rng)
        sets = [_draw_ring_pixels(valid2d, ny, nx, cxi, cyi, lo, hi, gsd, samples, run_rng) for lo, hi in zip(radii[:-1], radii[1:])]
        b = np.concatenate(sets) if sets else np.empty(0, dtype=np.int64)
        if not (a.size and b.size):
            return None
        return ((a % nx) * float(gsd), (a // nx) * float(gsd), get(a), (b % nx) * float(gsd), (b // nx) * float(gsd), get(b))

    blocks = []
    for (cxi, cyi), blk in zip(centres, _host_map(one_run, list(zip(centres, children)))):
        if blk is not None:
            blocks.append(blk)
            if centres_out is not None:
                centres_out.append((cxi, cyi))
    return blocks


# ======================================================================================================================
# N-D binned statistics: mirror of xdem/spatialstats.py:76-216 over csrc/binstats.hip
# ======================================================================================================================
def nmad(data, nfact: float = 1.4826):
    """Normalized median absolute deviation, ``nfact * nanmedian(|x - nanmedian(x)|)`` (geoutils.stats.nmad, what
    xdem/spatialstats.py:76-88 forwards to).  Host NumPy helper; as an ``nd_binning`` statistic it is evaluated per bin
    on the GPU.  Large float arrays (rasters) go through the exact selection of ``nmad_device`` when a GPU is there -- the same
    number, bit for bit, in the same scalar type (0.9 s -> 0.06 s for a 12000^2 float32 raster); NumPy otherwise."""
    arr = np.ma.filled(data, np.nan) if isinstance(data, np.ma.MaskedArray) else np.asarray(data)
    if arr.size >= 4_000_000 and arr.dtype in (np.dtype(np.float32), np.dtype(np.float64)) and isinstance(nfact, (int, float)):
        try:
            _, nm, cnt = nmad_device(arr, float(nfact))
        except _lib.XdemHipError:
            cnt = -1   # (no GPU in this process: the host helper stays what it was)
        if cnt > 0:
            return arr.dtype.type(nm)
    return nfact * np.nanmedian(np.abs(arr - np.nanmedian(arr)))


_GPU_STATS = {"count": "count", "nanmedian": "median", "median": "median", "nmad": "nmad"}


def _scipy_range(rng, ndim: int, one_d: bool):
    """``range=`` as scipy.stats.binned_statistic / _2d / _dd read it (scipy/stats/_binned_statistic.py: binned_statistic wraps a
    2-element range into a list, ``_bin_edges`` checks the length and the order and unpacks a (start, stop) pair per dimension):
    -> (smin, smax) arrays, raising what SciPy raises for what it refuses.  upstream hands ``list_ranges`` AS IS to every 1-D,
    2-D and N-D call (xdem/spatialstats.py:147, 176, 190), so with more than one variable only SciPy's errors can come out --
    reproduced, not repaired."""
    if one_d and len(rng) == 2:
        rng = [rng]
    if len(rng) != ndim:
        raise ValueError(f"range given for {len(rng)} dimensions; {ndim} required")
    smin, smax = np.empty(ndim), np.empty(ndim)
    for i in range(ndim):
        if rng[i][1] < rng[i][0]:
            raise ValueError(f"In {f'dimension {i + 1} of ' if ndim > 1 else ''}range, start must be <= stop")
        smin[i], smax[i] = rng[i]
    return smin, smax


def _scipy_edges(sample_cols: list[np.ndarray], mins: list[float], maxs: list[float], bins: list) -> tuple[list[np.ndarray], list[int], Any]:
    """Bin edges, rounding decimals and sample dtype exactly as scipy.stats._binned_statistic._bin_edges /
    _bin_numbers derive them: ``smin, smax`` of the kept rows (range=None) or of the given range as float, +-0.5 when equal,
    ``np.linspace`` in the dtype of SciPy's sample matrix (the variables' common float dtype)."""
    sdt = np.result_type(*[c.dtype for c in sample_cols])
    edges_dtype = sdt if np.issubdtype(sdt, np.floating) else np.dtype(float)
    edges, decimals = [], []
    for i in range(len(sample_cols)):
        if np.isscalar(bins[i]):
            smin, smax = float(mins[i]), float(maxs[i])
            if smin == smax:
                smin, smax = smin - 0.5, smax + 0.5
            e = np.linspace(smin, smax, int(bins[i]) + 1, dtype=edges_dtype)
        else:
            e = np.asarray(np.asarray(bins[i], float), edges_dtype)
            len(e)   # (a 0-d array -- BiasCorr's dict of INTEGER bin sizes -- is no scalar to SciPy either: its TypeError, `nbin = len(edges) + 1`)
        d = np.diff(e)
        dmin = d.min()
        if dmin == 0:
            raise ValueError("The smallest edge difference is numerically 0.")
        decimals.append(int(-np.log10(dmin)) + 6)
        edges.append(e)
    return edges, decimals, edges_dtype


class _DeviceColumn:
    """A 1-D float32 / float64 CUDA tensor as a column of ``BinStatsPlan``: what the plan reads of a NumPy column (``dtype``,
    ``size``) without the values leaving the device; ``host()`` fetches them once if a host-evaluated statistic needs them."""

    def __init__(self, tensor):
        self.tensor = _args.device_float(tensor, "device columns must be contiguous 1-D float32 / float64 CUDA tensors", ndim=1)
        self.dtype = _args.np_dtype(tensor)
        self.size = int(tensor.numel())
        self._host = None

    def host(self) -> np.ndarray:
        if self._host is None:
            self._host = self.tensor.cpu().numpy()
        return self._host


class BinStatsPlan(_lib._Plan):
    """Device-resident values + explanatory variables of one ``nd_binning`` call (``xdemhip_binstats``).  ``values`` / ``list_var``:
    NumPy arrays (uploaded), or 1-D CUDA tensors of one length (read in place and kept alive by the plan: the columns a dh plan
    gathers on the device, ``DhPlan.var_columns``)."""

    _DESTROY = "xdemhip_binstats_destroy"

    def __init__(self, values, list_var: list, ctx: _lib.Context | None = None):
        device = _args.is_tensor(values)
        self.ctx = ctx or (_lib.default_context(values.device.index) if device else _lib.default_context())
        self.ctx.adopt(self)
        L = self.ctx._L

        def prep(a):
            a = np.asarray(a).ravel()
            if a.dtype not in (np.dtype(np.float32), np.dtype(np.float64)):
                a = a.astype(np.float64)
            return np.ascontiguousarray(a)

        if device:
            if not all(_args.is_tensor(v) for v in list_var):
                raise ValueError("values on the device need every explanatory variable on the device")
            _args.synchronize_torch(values)   # (the library reads the columns on the context's stream)
            self._dev_values = _DeviceColumn(values)
            self.vars = [_DeviceColumn(v) for v in list_var]
        else:
            self._dev_values = None
            self._values = prep(values)
            self.vars = [prep(v) for v in list_var]
        first = self._dev_values if device else self._values
        n, space = first.size, _args.space(values)
        if any(v.size != n for v in self.vars):
            raise ValueError("values and explanatory variables must have the same number of elements")
        self.size = n
        h = ctypes.c_void_p()
        data = lambda a: getattr(a, "tensor", a)  # noqa: E731  (the array or tensor of a column)
        self.ctx.check(L.xdemhip_binstats_create(self.ctx.handle, ptr(data(first)), _args.code(first), n, space, ctypes.byref(h)))
        self.handle = h
        for v in self.vars:
            rc = L.xdemhip_binstats_add_var(self.handle, ptr(data(v)), _args.code(v), space)
            if rc < 0:
                self.ctx.check(rc)
        nv = ctypes.c_int64()
        k = max(len(self.vars), 1)
        vmin, vmax = np.empty(k), np.empty(k)
        self.ctx.check(L.xdemhip_binstats_finalize(self.handle, ctypes.byref(nv), dp(vmin), dp(vmax)))
        self.n_valid = int(nv.value)
        self.var_min, self.var_max = vmin, vmax

    @property
    def values(self) -> np.ndarray:
        """The values on the host (device columns: fetched on first use -- only a host-evaluated statistic asks)."""
        return self._values if self._dev_values is None else self._dev_values.host()

    def run(self, var_ids: list[int], bins: list, want_nmad: bool = True, nfact: float = 1.4826, ranges=None):
        """One binning over the given variables -> (count int64, median f64, nmad f64 | None, edges) in C order.  ``ranges`` =
        (smin, smax) per variable instead of the data's own extent (SciPy's ``range=``; samples outside fall into no bin)."""
        cols = [self.vars[i] for i in var_ids]
        mins, maxs = ([self.var_min[i] for i in var_ids], [self.var_max[i] for i in var_ids]) if ranges is None else ranges
        edges, decimals, sdt = _scipy_edges(cols, mins, maxs, bins)
        shape = tuple(len(e) - 1 for e in edges)
        nb = int(np.prod(shape))
        flat = np.concatenate([np.asarray(e, np.float64) for e in edges])
        counts = np.zeros(nb, np.int64)
        med = np.full(nb, np.nan)
        nm = np.full(nb, np.nan)
        ids = (ctypes.c_int * len(var_ids))(*var_ids)
        ne = (ctypes.c_int * len(var_ids))(*[len(e) for e in edges])
        dec = (ctypes.c_int * len(var_ids))(*decimals)
        if self.n_valid > 0:
            self.ctx.check(self.ctx._L.xdemhip_binstats_run(
                self.handle, len(var_ids), ids, dp(flat), ne, dec, _args.code(sdt), int(want_nmad), float(nfact), i64p(counts), dp(med), dp(nm)))
        return counts.reshape(shape), med.reshape(shape), (nm.reshape(shape) if want_nmad else None), edges

    def bin_numbers(self) -> np.ndarray:
        """uint16 flat bin number (C order over the dimensions of the last ``run``) of every sample, 0xFFFF = dropped by the joint
        finiteness filter or in no bin: for statistics evaluated on the host (``xdemhip_binstats_bin_numbers``)."""
        out = np.empty(self.size, dtype=np.uint16)
        if self.n_valid > 0:
            self.ctx.check(self.ctx._L.xdemhip_binstats_bin_numbers(self.handle, ptr(out)))
        else:
            out[:] = 0xFFFF
        return out


def nd_binning(values, list_var, list_var_names, list_var_bins=None, statistics=("count", np.nanmedian, nmad),
               list_ranges=None, ctx: _lib.Context | None = None):
    """N-dimensional binning of ``values`` by explanatory variables with per-bin statistics on the GPU.

    Drop-in for ``xdem.spatialstats.nd_binning`` (xdem/spatialstats.py:91-216): same flattening, joint finite filter,
    1-D binnings per variable, all 2-D combinations, one N-D binning when there are more than two variables, and the
    same DataFrame layout (``nd``, statistic columns named after the callables, one ``pd.IntervalIndex`` column per
    variable).  Statistics evaluated on the device: ``"count"``, ``np.nanmedian`` / ``"median"`` and ``nmad``.  Every other
    statistic upstream would pass on to SciPy -- ``"mean"`` / ``"std"`` / ``"sum"`` / ``"min"`` / ``"max"``, the NumPy function
    objects of those names, any callable of a 1-D array (``np.nanmean``, ``np.nanstd``, a lambda ...) -- is applied on the HOST to
    the values of each bin, from the bin numbers the device computed (``xdemhip_binstats_bin_numbers``), exactly as
    ``scipy.stats.binned_statistic_dd`` does (``xdem_amd/_binstat_host.py``): a Python callable cannot run anywhere else.  ``values``
    and ``list_var`` may also be 1-D CUDA tensors of one length (the columns ``DhPlan.var_columns`` gathers): they are binned in place,
    the DataFrame is the one the same values give from the host.  ``list_ranges`` goes to every binning exactly as
    upstream hands it to SciPy's ``range=`` (a (start, stop) pair or a one-element list of pairs for ONE variable; with several
    variables SciPy's own ValueError / TypeError comes out, as upstream).
    """
    import itertools

    import pandas as pd

    if list_var_bins is None:
        list_var_bins = (10,) * len(list_var_names)
    elif isinstance(list_var_bins, (int, np.integer)):
        list_var_bins = (list_var_bins,) * len(list_var_names)
    statistics = list(statistics)
    if "count" not in statistics:
        statistics.insert(0, "count")
    statistics_name = [f if isinstance(f, str) else f.__name__ for f in statistics]
    # "count", the exact median and the NMAD are evaluated on the device; anything else upstream would hand to SciPy -- its other
    # names ("mean", "std", "sum", "min", "max"), the NumPy function objects it answers itself, any callable of a 1-D array -- is
    # evaluated on the host from the bin numbers the device produced, the way scipy.stats.binned_statistic_dd does it
    from ._binstat_host import KNOWN_NAMES, binned_statistic_host

    kinds = []
    for f, name in zip(statistics, statistics_name):
        on_device = name in _GPU_STATS and (isinstance(f, str) or f is np.nanmedian or f is np.median or name == "nmad")
        if not on_device and not callable(f) and f not in KNOWN_NAMES:
            raise ValueError(f"invalid statistic {f!r}")   # (SciPy's refusal of an unknown name)
        kinds.append(_GPU_STATS[name] if on_device else None)
    want_nmad = "nmad" in kinds

    if _args.is_tensor(values):   # device columns (a dh plan's gather): binned where they are
        plan = BinStatsPlan(values, list(list_var), ctx)
    else:
        plan = BinStatsPlan(np.asarray(values), [np.asarray(v) for v in list_var], ctx)
    try:
        def stats_df(var_ids, bins, one_d=False):
            rng = None if list_ranges is None else _scipy_range(list_ranges, len(var_ids), one_d)
            c, m, s, edges = plan.run(var_ids, bins, want_nmad, ranges=rng)
            df = pd.DataFrame()
            sample_bins = None
            for f, name, kind in zip(statistics, statistics_name, kinds):
                if kind is None:
                    if sample_bins is None:
                        sample_bins = plan.bin_numbers()
                        kept = sample_bins != 0xFFFF
                        sample_bins, sample_vals = sample_bins[kept], plan.values[kept]
                    df[name] = binned_statistic_host(f, sample_bins, sample_vals, c.size)
                else:
                    df[name] = {"count": c.astype(float), "median": m, "nmad": s}[kind].flatten()
            return df, edges

        list_df_1d = []
        for i in range(len(list_var)):
            df, (e,) = stats_df([i], [list_var_bins[i]], one_d=True)
            df[list_var_names[i]] = pd.IntervalIndex.from_breaks(e, closed="left")
            df.insert(0, "nd", 1)
            list_df_1d.append(df)
        list_df_2d = []
        if len(list_var) > 1:
            for v1, v2 in itertools.combinations(list_var_names, 2):
                i1, i2 = list_var_names.index(v1), list_var_names.index(v2)
                df, (e1, e2) = stats_df([i1, i2], [list_var_bins[i1], list_var_bins[i2]])
                ii1 = pd.IntervalIndex.from_breaks(e1, closed="left")
                ii2 = pd.IntervalIndex.from_breaks(e2, closed="left")
                df[v1] = [a for a in ii1 for b in ii2]
                df[v2] = [b for a in ii1 for b in ii2]
                df.insert(0, "nd", 2)
                list_df_2d.append(df)
        df_nd = pd.DataFrame()
        if len(list_var) > 2:
            df_nd, list_edges = stats_df(list(range(len(list_var))), list(list_var_bins))
            list_ii = [pd.IntervalIndex.from_breaks(e, closed="left") for e in list_edges]
            iind = np.meshgrid(*list_ii)  # (upstream's default 'xy' indexing, spatialstats.py:202)
            for i, name in enumerate(list_var_names):
                df_nd[name] = iind[i].flatten()
            df_nd.insert(0, "nd", len(list_var_names))
    finally:
        plan.close()
    return pd.concat(list_df_1d + list_df_2d + [df_nd])


# ---- heteroscedasticity inference on top of nd_binning (xdem/spatialstats.py:237-421, 530-631, 808-878) ---------------
class GridInterpolant:
    """Multilinear interpolant on a regular N-D grid, evaluated on the GPU (``xdemhip_interp_grid_linear``).

    Call signature of the object ``interp_nd_binning`` returns upstream (a ``scipy.interpolate.RegularGridInterpolator``
    with ``method="linear", bounds_error=False, fill_value=None``): ``fun((x1, x2, ...))`` with arrays of one common
    shape (or scalars) -> float64 array of that shape; NaN coordinates give NaN, outside points extrapolate linearly.
    ``scale`` multiplies the result (the re-scaling factor of the two-step standardization)."""

    def __init__(self, axes: list[np.ndarray], values: np.ndarray, scale: float = 1.0, ctx: _lib.Context | None = None):
        self.grid = tuple(np.ascontiguousarray(a, dtype=np.float64) for a in axes)
        self.values = np.ascontiguousarray(values, dtype=np.float64)
        if self.values.shape != tuple(len(a) for a in self.grid):
            raise ValueError("grid values do not match the axes")
        self.scale = float(scale)
        self.ctx = ctx

    def scaled(self, factor: float) -> "GridInterpolant":
        return GridInterpolant(list(self.grid), self.values, self.scale * float(factor), self.ctx)

    def __call__(self, xi) -> np.ndarray:
        if isinstance(xi, np.ndarray) and xi.ndim >= 1 and xi.shape[-1] == len(self.grid) and not isinstance(xi, tuple):
            xi = tuple(xi[..., d] for d in range(len(self.grid)))
        if len(xi) != len(self.grid):
            raise ValueError(f"The requested sample points xi have dimension {len(xi)} but this interpolant has dimension {len(self.grid)}")
        arrs = np.broadcast_arrays(*[np.asarray(x) for x in xi])
        shape = arrs[0].shape
        cols = []
        for a in arrs:
            a = np.ascontiguousarray(a).ravel()
            if a.dtype not in (np.dtype(np.float32), np.dtype(np.float64)):
                a = a.astype(np.float64)
            cols.append(a)
        n = cols[0].size
        out = np.empty(n, dtype=np.float64)
        if n == 0:
            return out.reshape(shape)
        ctx = self.ctx or _lib.default_context()
        nd = len(cols)
        ptrs = (ctypes.c_void_p * nd)(*[ptr(c) for c in cols])
        dts = (ctypes.c_int * nd)(*[_args.code(c) for c in cols])
        na = (ctypes.c_int * nd)(*[len(a) for a in self.grid])
        axes = np.concatenate(self.grid)
        ctx.check(ctx._L.xdemhip_interp_grid_linear(ctx.handle, nd, dp(axes), na, dp(self.values), ptrs, dts, n, self.scale, dp(out), _lib.HOST))
        return out.reshape(shape)


def nmad_device(values: np.ndarray, nfact: float = 1.4826, abs_limit: float = np.inf, ctx: _lib.Context | None = None):
    """(nanmedian, nmad, count) of an array on the GPU by exact selection; ``|v| > abs_limit`` is dropped first."""
    v = np.ascontiguousarray(np.asarray(values).ravel())
    if v.dtype not in (np.dtype(np.float32), np.dtype(np.float64)):
        v = v.astype(np.float64)
    ctx = ctx or _lib.default_context()
    med, nm, cnt = ctypes.c_double(), ctypes.c_double(), ctypes.c_int64()
    ctx.check(ctx._L.xdemhip_nmad(ctx.handle, ptr(v), _args.code(v), v.size, float(nfact),
                                  float(abs_limit), _lib.HOST, ctypes.byref(med), ctypes.byref(nm), ctypes.byref(cnt)))
    return med.value, nm.value, int(cnt.value)


def _pandas_str_to_interval(istr):
    """A ``pd.Interval`` written to text (a DataFrame saved to CSV without its MultiIndex) read back: ``"[0.0, 2.5)"`` ->
    ``Interval(0.0, 2.5, closed="left")``; a float cell (NaN of another binning's rows) or an interval pandas refuses -> NaN.
    Mirror of xdem/spatialstats.py:221-234."""
    import pandas as pd

    if isinstance(istr, float):
        return np.nan
    closed = {("[", ")"): "left", ("(", "]"): "right", ("[", "]"): "both"}.get((istr[0] if istr[0] == "[" else "(", istr[-1] if istr[-1] == "]" else ")"), "neither")
    left, right = (float(t) for t in istr[1:-1].split(","))
    try:
        return pd.Interval(left, right, closed)
    except Exception:
        return np.nan


def _edge_as_numpy_compares(dtype: np.dtype, edge) -> float:
    """The value ``arr >= edge`` really tests against for an array of `dtype`: NumPy converts a Python number (a weak scalar: the
    ends of an interval parsed from text) to the array's dtype before comparing, while a ``np.float64`` end -- what nd_binning's
    ``pd.IntervalIndex.from_breaks`` stores -- widens a float32 array instead.  ``np.result_type`` answers for whichever
    promotion rules the installed NumPy applies."""
    return float(np.asarray(edge).astype(np.result_type(dtype, edge)))


def _perbin_tables(df, var_dtypes: list, list_var_names: list, statistic_name: str, min_count: int | None):
    """The host tables of ``xdemhip_perbin_lookup`` for the rows of `df` that bin exactly `list_var_names`, whose arrays have
    `var_dtypes`: (intervals per variable, left ends, right ends -- as NumPy compares them against those dtypes --, the statistic
    and the decision byte per bin of the product of the intervals, whether the intervals are disjoint, the count column)."""
    import pandas as pd

    rows = df.copy()
    if "nd" in rows.columns:
        rows = rows[rows.nd == len(list_var_names)]
    for name in list_var_names:
        cells = rows[name].values
        if any(isinstance(x, pd.Interval) for x in cells):
            continue
        parsed = [_pandas_str_to_interval(x) for x in cells]
        if not any(isinstance(x, pd.Interval) for x in parsed):
            raise ValueError("The bin intervals of the dataframe should be pandas.Interval.")
        rows[name] = parsed
    n_var = len(list_var_names)
    uniques = [np.unique(rows[name].values) for name in list_var_names]
    counts = [len(u) for u in uniques]
    n_bins = int(np.prod(counts, dtype=np.int64)) if all(counts) else 0
    count_col = rows["count"].values if "count" in rows.columns else None
    if n_bins == 0:
        return counts, None, None, None, None, True, count_col
    left = np.array([_edge_as_numpy_compares(var_dtypes[k], iv.left) for k in range(n_var) for iv in uniques[k]], dtype=np.float64)
    right = np.array([_edge_as_numpy_compares(var_dtypes[k], iv.right) for k in range(n_var) for iv in uniques[k]], dtype=np.float64)
    # the bin table over the product of the intervals (itertools.product order); the FIRST row of a bin counts (`.values[0]`)
    table = np.full(n_bins, np.nan, dtype=np.float64)
    decided = np.full(n_bins, 2, dtype=np.uint8)   # 2 = the DataFrame has no row for this bin
    place = [{iv: j for j, iv in enumerate(u)} for u in uniques]
    stat_col = rows[statistic_name].values
    cols = [rows[name].values for name in list_var_names]
    for r in range(len(rows)):
        flat = 0
        for k in range(n_var):
            flat = flat * counts[k] + place[k][cols[k][r]]
        if decided[flat] != 2:
            continue
        table[flat] = stat_col[r]
        if min_count is None:
            continue   # stays "undecidable": upstream's `count > None` raises as soon as a pixel lies in a bin
        decided[flat] = 1 if count_col[r] > min_count else 0
    disjoint = all(all(uniques[k][j].right <= uniques[k][j + 1].left for j in range(counts[k] - 1)) for k in range(n_var))
    return counts, left, right, table, decided, disjoint, count_col


def get_perbin_nd_binning(df, list_var, list_var_names, statistic=np.nanmedian, min_count: int | None = 0,
                          ctx: _lib.Context | None = None) -> np.ndarray:
    """Per-pixel value of a binned statistic: every element of the explanatory variables receives the statistic of the bin of
    `df` (an ``nd_binning`` output, or a DataFrame of ``pd.Interval`` columns) it falls into -- NaN outside every bin and in
    bins whose count does not exceed `min_count`.  Drop-in for ``xdem.spatialstats.get_perbin_nd_binning``
    (xdem/spatialstats.py:425-527; `statistic` a column name or a callable whose ``__name__`` is one, upstream's default is
    ``np.nanmedian``), used by the bias corrections (xdem/coreg/biascorr.py:302).

    Upstream builds one boolean mask per interval and variable and walks the product of the intervals, writing bin after bin;
    here the small tables are prepared on the host -- sorted unique intervals per variable (``np.unique``, as upstream), the
    statistic and the "count > min_count" decision per bin of the product -- and ``xdemhip_perbin_lookup`` does the per-pixel
    search on the GPU.  Same results bit for bit, including overlapping intervals (the last bin of upstream's walk that writes
    wins) and NaN variables.  Where upstream fails, this fails the same way: a pixel in a bin the DataFrame has no row for ->
    ``IndexError`` (upstream's ``.values[0]`` on an empty selection); ``min_count=None`` with a pixel in any bin -> the
    ``TypeError`` of ``count > None``.  One deviation: cells that are neither ``pd.Interval`` nor their text form raise the
    ``ValueError`` upstream constructs at spatialstats.py:479 but forgets to raise (it dies with an ``AttributeError`` a few
    lines later)."""
    import itertools

    import pandas as pd

    shape = np.shape(list_var[0])
    if isinstance(list_var_names, str):
        list_var_names = [list_var_names]
    if len(list_var) != len(list_var_names):
        raise ValueError("The lists of variables and variable names should be the same length.")
    for var in list_var_names:
        if var not in df.columns:
            raise ValueError('Variable "' + var + '" does not exist in the provided dataframe.')
    statistic_name = statistic if isinstance(statistic, str) else statistic.__name__
    if statistic_name not in df.columns:
        raise ValueError('Statistic "' + statistic_name + '" does not exist in the provided dataframe.')
    if min_count is not None and "count" not in df.columns:
        raise ValueError('Statistic "count" is not in the provided dataframe, necessary to use the min_count argument.')
    if df.empty:
        raise ValueError("Dataframe is empty.")
    n_var = len(list_var)
    if n_var > 8:
        raise NotImplementedError("get_perbin_nd_binning: at most 8 explanatory variables")
    arrays = []
    for k, name in enumerate(list_var_names):
        a = np.ascontiguousarray(list_var[k])
        if a.dtype not in (np.dtype(np.float32), np.dtype(np.float64)):
            a = a.astype(np.float64)   # (integers and half floats compare as float64 against float ends: exact below 2^53)
        if a.shape != shape:
            raise ValueError(f"variable {name!r} has shape {a.shape}, the first variable {shape}")   # (upstream: a boolean-index error)
        arrays.append(a.reshape(-1))
    counts, left, right, table, decided, disjoint, count_col = _perbin_tables(df, [a.dtype for a in arrays], list_var_names, statistic_name,
                                                                              min_count)
    out = np.full(int(np.prod(shape, dtype=np.int64)), np.nan, dtype=np.float64)
    if table is None or out.size == 0:
        return out.reshape(shape)
    ctx = ctx or _lib.default_context()
    ptrs = (ctypes.c_void_p * n_var)(*[ptr(a) for a in arrays])
    dts = (ctypes.c_int * n_var)(*[_args.code(a) for a in arrays])
    nint = (ctypes.c_int * n_var)(*counts)
    missing = ctypes.c_int64()
    with ctx.call_lock:
        rc = ctx._L.xdemhip_perbin_lookup(ctx.handle, ptrs, dts, n_var, out.size, nint, dp(left), dp(right), dp(table), _args.chars(decided),
                                          1 if disjoint else 0, ptr(out), ctypes.byref(missing), _lib.HOST)
    ctx.check(rc)
    if missing.value:
        if min_count is None and count_col is not None:
            count_col[0] > min_count   # noqa: B015 -- raises upstream's TypeError ('>' between a float and None)
        raise IndexError("index 0 is out of bounds for axis 0 with size 0")   # upstream's `.values[0]` of a bin without a row
    return out.reshape(shape)


def _rows_of_one_binning(df, names: list[str], stat_col: str, min_count: int | None):
    """The rows of `df` that belong to the binning over exactly `names`, bin positions as numbers: (rows, statistic values,
    mask of the usable ones).  Refusals and their messages are upstream's (xdem/spatialstats.py:292-352, asserted by its tests)."""
    import pandas as pd

    missing = [v for v in names if v not in df.columns]
    if missing:
        raise ValueError('Variable "' + missing[0] + '" does not exist in the provided dataframe.')
    if stat_col not in df.columns:
        raise ValueError('Statistic "' + stat_col + '" does not exist in the provided dataframe.')
    if min_count is not None and "count" not in df.columns:
        raise ValueError('Statistic "count" is not in the provided dataframe, necessary to use the min_count argument.')
    if df.empty:
        raise ValueError("Dataframe is empty.")
    rows = df[df.nd == len(names)].copy() if "nd" in df.columns else df.copy()
    numeric = (int, float, np.integer, np.floating)
    position = {}
    for v in names:   # a bin's position: its mid value, given as a number or as the pandas interval nd_binning writes
        cells = rows[v].values
        if all(isinstance(x, numeric) for x in cells):
            position[v] = np.asarray(cells, dtype=float) if len(cells) else np.empty(0)
        elif any(isinstance(x, pd.Interval) for x in cells):
            position[v] = pd.IntervalIndex(rows[v]).mid.values
        else:
            raise ValueError("The variable columns must be provided as numerical mid values, or pd.Interval values.")
        rows[v] = position[v]
    placed = np.ones(len(rows), dtype=bool)
    for v in names:
        placed &= np.isfinite(position[v])
    rows = rows[placed]
    if rows.empty:
        raise ValueError("Dataframe does not contain a nd binning with the variables corresponding to the list of variables.")
    if not np.isfinite(rows[stat_col].values).any():
        raise ValueError("Dataframe does not contain any valid statistic values.")
    if min_count is not None:
        rows.loc[rows["count"] < min_count, stat_col] = np.nan
    stat = rows[stat_col].values
    usable = np.isfinite(stat)
    if not usable.any():
        raise ValueError("Dataframe does not contain any valid statistic values after filtering with min_count = "
                         + str(min_count) + ".")
    return rows, stat, usable


def interp_nd_binning(df, list_var_names, statistic="nmad", interpolate_method: str = "linear", min_count: int | None = 100,
                      ctx: _lib.Context | None = None) -> GridInterpolant:
    """Interpolant of a binned statistic over its explanatory variables (mirror of xdem/spatialstats.py:237-421).

    Same three stages as upstream on the (small) table of bins, done with the same SciPy routines on the host: (1)
    ``griddata`` of the valid bins onto the full grid of bin centres, (2) nearest-neighbour filling of what lies outside
    the convex hull, on the grid and on the grid extended by one node per side, (3) a linear regular-grid interpolant
    over the extended grid, so that extrapolation behaves as nearest neighbour.  Stage 3's evaluation is the dense
    operation: it runs on the GPU (``GridInterpolant``)."""
    import pandas as pd
    from scipy.interpolate import griddata

    names = [list_var_names] if isinstance(list_var_names, str) else list(list_var_names)
    stat_col = statistic if isinstance(statistic, str) else statistic.__name__
    sub, stat, good = _rows_of_one_binning(df, names, stat_col, min_count)
    list_var_names = names
    centres = [sorted(np.unique(sub[var][good])) for var in list_var_names]
    shape = [len(c) for c in centres]
    # (1) inside the convex hull of the valid bins
    pts_good = tuple(sub[var].values[good] for var in list_var_names)
    mesh = np.meshgrid(*centres, indexing="ij")
    pts_grid = tuple(m.flatten() for m in mesh)
    on_grid = griddata(pts_good, stat[good], pts_grid, method=interpolate_method)
    # (2) nearest neighbour outside it, first on the grid itself, then on the grid grown by one node per side
    filled = np.isfinite(on_grid)
    on_grid = griddata(tuple(p[filled] for p in pts_grid), on_grid[filled], pts_grid, method="nearest")
    grown = [np.append(np.insert(c, 0, c[0] - 1), c[-1] + 1) for c in centres]
    mesh_g = np.meshgrid(*grown, indexing="ij")
    on_grown = griddata(pts_grid, on_grid, tuple(m.flatten() for m in mesh_g), method="nearest").reshape(tuple(s + 2 for s in shape))
    # (3)
    return GridInterpolant(grown, on_grown, 1.0, ctx)


def two_step_standardization(dvalues, list_var, unscaled_error_fun, spread_statistic=nmad, fac_spread_outliers: float | None = 7,
                             ctx: _lib.Context | None = None):
    """Standardize ``dvalues`` by the modelled spread, filter outliers, re-scale to unit spread
    (mirror of xdem/spatialstats.py:530-573).  Returns (z-scores, final error function).  ``nmad`` -- the default -- is evaluated by
    exact selection on the GPU; any other `spread_statistic` is called on the z-scores on the host, as upstream calls it."""
    name = spread_statistic if isinstance(spread_statistic, str) else getattr(spread_statistic, "__name__", "")
    on_device = name == "nmad"
    with np.errstate(all="ignore"):
        zscores = np.asarray(dvalues) / unscaled_error_fun(tuple(list_var))
    spread = (lambda z: nmad_device(z, ctx=ctx)[1]) if on_device else spread_statistic
    if fac_spread_outliers is not None:
        with np.errstate(invalid="ignore"):
            zscores[np.abs(zscores) > fac_spread_outliers * spread(zscores)] = np.nan
    zscore_nmad = spread(zscores)
    zscores /= zscore_nmad
    if isinstance(unscaled_error_fun, GridInterpolant):
        error_fun = unscaled_error_fun.scaled(zscore_nmad)
    else:
        def error_fun(*args):
            return zscore_nmad * unscaled_error_fun(*args)
    return zscores, error_fun


def _estimate_model_heteroscedasticity(dvalues, list_var, list_var_names, spread_statistic=nmad, list_var_bins=None,
                                       min_count: int | None = 100, fac_spread_outliers: float | None = 7,
                                       ctx: _lib.Context | None = None):
    """N-D binning of the spread -> interpolant -> two-step standardization (mirror of xdem/spatialstats.py:576-631)."""
    df = nd_binning(values=dvalues, list_var=list_var, list_var_names=list_var_names, statistics=[spread_statistic],
                    list_var_bins=list_var_bins, ctx=ctx)
    fun = interp_nd_binning(df, list_var_names=list_var_names, statistic=spread_statistic.__name__, min_count=min_count, ctx=ctx)
    final_fun = two_step_standardization(np.asarray(dvalues).ravel(), [np.asarray(v).ravel() for v in list_var], fun,
                                         spread_statistic, fac_spread_outliers, ctx)[1]
    return df, final_fun


def _burn_vector_masks(masks, raster) -> list:
    """`masks` with every ``xdem_amd.Vector`` among them burnt into the grid of `raster` (``Vector.create_mask`` on the GPU); the rest
    as it came, for the callers' own checks."""
    from .vector import Vector

    out = []
    for m in masks:
        if isinstance(m, Vector):
            if not (hasattr(raster, "transform") and hasattr(raster, "data")):
                raise ValueError("a Vector mask needs the grid it is burnt into: pass the values as a Raster-like object (.data, .transform)")
            m = m.create_mask((tuple(np.shape(raster.data))[-2:], raster.transform))
        out.append(m)
    return out


def infer_heteroscedasticity_from_stable(dvalues, list_var, stable_mask=None, unstable_mask=None, list_var_names=None,
                                         spread_statistic=nmad, list_var_bins=None, min_count: int | None = 100,
                                         fac_spread_outliers: float | None = 7, ctx: _lib.Context | None = None):
    """Error map, binned-spread DataFrame and error function from differences on stable terrain
    (mirror of xdem/spatialstats.py:808-878 for array inputs and boolean-array masks; Raster-likes are read through
    ``.data`` and the error map is returned as ``dvalues.copy(new_array=...)`` when that method exists)."""
    def arr_of(v):
        if isinstance(v, np.ndarray):
            return np.ma.filled(v, np.nan) if isinstance(v, np.ma.MaskedArray) else v
        data = getattr(v, "data", None)
        if data is None:
            raise ValueError("The values must be a Raster or NumPy array, or a list of those.")
        return np.ma.filled(data.astype(np.float32) if not np.issubdtype(data.dtype, np.floating) else data, np.nan)

    if list_var_names is None:
        list_var_names = ["var" + str(i + 1) for i in range(len(list_var))]
    arrs = [arr_of(dvalues)] + [arr_of(v) for v in list_var]
    stable_mask, unstable_mask = _burn_vector_masks((stable_mask, unstable_mask), dvalues)
    for m in (stable_mask, unstable_mask):
        if m is not None and not isinstance(m, np.ndarray):
            raise ValueError("xdem_amd takes stable / unstable masks as boolean arrays (vector rasterisation is outside the hot path).")
    if stable_mask is None and unstable_mask is None:
        # (everything is stable terrain: upstream's all-True mask selects every element in C order -- the flat views, without three
        #  raster-sized boolean-index copies; nothing below writes to them)
        stable = [np.asarray(a).squeeze().reshape(-1) for a in arrs]
    else:
        include = np.ones(np.shape(arrs[0]), dtype=bool) if stable_mask is None else np.asarray(stable_mask, dtype=bool)
        exclude = np.zeros(np.shape(arrs[0]), dtype=bool) if unstable_mask is None else np.asarray(unstable_mask, dtype=bool)
        include = np.logical_and(include, ~exclude).squeeze()
        stable = [a[include] for a in arrs]
    df, fun = _estimate_model_heteroscedasticity(stable[0], stable[1:], list_var_names, spread_statistic, list_var_bins, min_count,
                                                 fac_spread_outliers, ctx)
    error = fun(tuple(arrs[1:]))
    if not isinstance(dvalues, np.ndarray) and hasattr(dvalues, "copy"):
        try:
            return dvalues.copy(new_array=error), df, fun
        except TypeError:
            pass
    return error, df, fun


# ======================================================================================================================
# Spatial correlation of errors: variogram model fitting around the GPU variogram (callers of the hot path;
# mirror of xdem/spatialstats.py:1583-1964).  Host-side SciPy, like upstream.
# ======================================================================================================================
def _check_validity_params_variogram(params_variogram_model) -> None:
    from . import variogram_models as vm

    if not all(c in params_variogram_model for c in ("model", "range", "psill")):
        raise ValueError('The dataframe with variogram parameters must contain the columns "model", "range" and "psill".')
    for model in params_variogram_model["model"].values:
        vm.model_name(model)
    num = (float, np.floating, int, np.integer)
    for r in params_variogram_model["range"].values:
        if not isinstance(r, num):
            raise ValueError("The variogram ranges must be float or integer.")
        if r <= 0:
            raise ValueError("The variogram ranges must have non-zero, positive values.")
    for p in params_variogram_model["psill"].values:
        if not isinstance(p, num):
            raise ValueError("The variogram partial sills must be float or integer.")
        if p <= 0:
            raise ValueError("The variogram partial sills must have non-zero, positive values.")
    names = [vm.model_name(m) for m in params_variogram_model["model"].values]
    if any(n in ("stable", "matern") for n in names):
        if "smooth" not in params_variogram_model:
            raise ValueError('The dataframe with variogram parameters must contain the column "smooth" for '
                             "the smoothness factor when using Matern or Stable models.")
        for n, s in zip(names, params_variogram_model["smooth"].values):
            if n in ("stable", "matern"):
                if not isinstance(s, num):
                    raise ValueError("The variogram smoothness parameter must be float or integer.")
                if s <= 0:
                    raise ValueError("The variogram smoothness parameter must have non-zero, positive values.")


def get_variogram_model_func(params_variogram_model):
    """Sum of variogram models from a parameter table (columns model, range, psill[, smooth]) -> function of the lag."""
    from . import variogram_models as vm

    _check_validity_params_variogram(params_variogram_model)
    rows = []
    for i in range(len(params_variogram_model)):
        name = vm.model_name(params_variogram_model["model"].values[i])
        args = [params_variogram_model["range"].values[i], params_variogram_model["psill"].values[i]]
        if vm.n_params(name) == 3:
            args.append(params_variogram_model["smooth"].values[i])
        rows.append((getattr(vm, name), args))

    def sum_model(h):
        fn = np.zeros(np.shape(h))
        for f, args in rows:
            fn = fn + f(h, *args)
        return fn

    return sum_model


def covariance_from_variogram(params_variogram_model):
    """C(h) = total sill - sum of variograms."""
    _check_validity_params_variogram(params_variogram_model)
    total_sill = np.sum(params_variogram_model["psill"])
    sum_variogram = get_variogram_model_func(params_variogram_model)
    return lambda h: total_sill - sum_variogram(h)


def correlation_from_variogram(params_variogram_model):
    """rho(h) = C(h) / total sill, between 0 and 1."""
    _check_validity_params_variogram(params_variogram_model)
    total_sill = np.sum(params_variogram_model["psill"].values)
    cov = covariance_from_variogram(params_variogram_model)
    return lambda h: cov(h) / total_sill


def fit_sum_model_variogram(list_models, empirical_variogram, bounds=None, p0=None, maxfev=None):
    """Weighted least-squares fit of a sum of variogram models to an empirical variogram (the DataFrame of
    ``sample_empirical_variogram``): same bounds / first guesses / weighting rules as xdem/spatialstats.py:1680-1804.
    Returns (fitted sum function, DataFrame of model, range, psill[, smooth])."""
    import pandas as pd
    from scipy.optimize import curve_fit

    from . import variogram_models as vm

    names = [vm.model_name(m) for m in list_models]

    def variogram_sum(h, *args):
        fn, i = 0.0, 0
        for name in names:
            k = vm.n_params(name)
            fn = fn + getattr(vm, name)(h, *args[i:i + k])
            i += k
        return fn

    ev = empirical_variogram[np.isfinite(empirical_variogram.exp.values)]
    n_average = np.ceil(len(ev.exp.values) / 10)
    max_var = np.max(np.convolve(ev.exp.values, np.ones(int(n_average)) / n_average, mode="valid"))
    if bounds is None:
        bounds = [(0, ev.lags.values[-1]), (0, max_var)] * len(names)
    if p0 is None:
        p0 = []
        for i in range(len(names)):
            p0.append(((i + 1) / len(names)) * ev.lags.values[-1])
            p0.append(((i + 1) / len(names)) * max_var)
    final_bounds = np.transpose(np.array(bounds))
    err = ev.err_exp.values
    if np.all(np.isnan(err)) or np.all(err == 0):
        cof, _ = curve_fit(variogram_sum, ev.lags.values, ev.exp.values, method="trf", p0=p0, bounds=final_bounds, maxfev=maxfev)
    else:
        valid = np.isfinite(err)
        cof, _ = curve_fit(variogram_sum, ev.lags.values[valid], ev.exp.values[valid], method="trf", p0=p0, bounds=final_bounds,
                           sigma=err[valid], maxfev=maxfev)
    list_df, i = [], 0
    for name in names:
        k = vm.n_params(name)
        d = {"model": [name], "range": [cof[i]], "psill": [cof[i + 1]]}
        if k == 3:
            d["smooth"] = [cof[i + 2]]
        list_df.append(pd.DataFrame(d))
        i += k
    df_params = pd.concat(list_df)
    return get_variogram_model_func(df_params), df_params


def _estimate_model_spatial_correlation(dvalues, list_models, estimator: str = "dowd", gsd: float = None, coords=None,
                                        subsample: int = 1000, subsample_method: str = "cdist_equidistant", n_variograms: int = 1,
                                        n_jobs: int = 1, random_state=None, bounds=None, p0=None, **kwargs):
    """Empirical variogram on the GPU + model fit + correlation function (mirror of xdem/spatialstats.py:1807-1873)."""
    empirical_variogram = sample_empirical_variogram(values=dvalues, estimator=estimator, gsd=gsd, coords=coords, subsample=subsample,
                                                     subsample_method=subsample_method, n_variograms=n_variograms, n_jobs=n_jobs,
                                                     random_state=random_state, **kwargs)
    params = fit_sum_model_variogram(list_models=list_models, empirical_variogram=empirical_variogram, bounds=bounds, p0=p0)[1]
    return empirical_variogram, params, correlation_from_variogram(params_variogram_model=params)


def infer_spatial_correlation_from_stable(dvalues, list_models, stable_mask=None, unstable_mask=None, errors=None,
                                          estimator: str = "dowd", gsd: float = None, coords=None, subsample: int = 1000,
                                          subsample_method: str = "cdist_equidistant", n_variograms: int = 1, n_jobs: int = 1,
                                          bounds=None, p0=None, random_state=None, **kwargs):
    """Spatial correlation of errors from differences on stable terrain (mirror of xdem/spatialstats.py:1876-1964 for
    array inputs with boolean-array masks, Raster-likes read through ``.data`` / ``.res``): non-stable pixels become NaN
    (shape preserved), values are standardized by ``errors`` if given, then the variogram is sampled on the GPU and fitted."""
    if isinstance(dvalues, np.ndarray):
        arr = np.ma.filled(dvalues, np.nan) if isinstance(dvalues, np.ma.MaskedArray) else dvalues
        if gsd is None:
            raise ValueError("The ground sampling distance must be provided if no Raster object is passed.")
    else:
        data = getattr(dvalues, "data", None)
        if data is None:
            raise ValueError("The values must be a Raster or NumPy array, or a list of those.")
        arr = np.ma.filled(data, np.nan)
        if gsd is None:
            gsd = dvalues.res[0]
    stable_mask, unstable_mask = _burn_vector_masks((stable_mask, unstable_mask), dvalues)
    for m in (stable_mask, unstable_mask):
        if m is not None and not isinstance(m, np.ndarray):
            raise ValueError("xdem_amd takes stable / unstable masks as boolean arrays (vector rasterisation is outside the hot path).")
    include = np.ones(np.shape(arr), dtype=bool) if stable_mask is None else np.asarray(stable_mask, dtype=bool)
    exclude = np.zeros(np.shape(arr), dtype=bool) if unstable_mask is None else np.asarray(unstable_mask, dtype=bool)
    include = np.logical_and(include, ~exclude).squeeze()
    stable = np.array(arr, dtype=arr.dtype if np.issubdtype(arr.dtype, np.floating) else np.float32, copy=True)
    stable[~include] = np.nan
    if errors is not None:
        err = errors if isinstance(errors, np.ndarray) else np.ma.filled(getattr(errors, "data"), np.nan)
        with np.errstate(all="ignore"):
            stable = stable / err
    return _estimate_model_spatial_correlation(dvalues=stable, list_models=list_models, estimator=estimator, gsd=gsd, coords=coords,
                                               subsample=subsample, subsample_method=subsample_method, n_variograms=n_variograms,
                                               n_jobs=n_jobs, random_state=random_state, bounds=bounds, p0=p0, **kwargs)


# ======================================================================================================================
# Number of effective samples (xdem/spatialstats.py:2011-2308): closed forms on the host, the O(N^2) double covariance sums
# on the GPU (csrc/covsum.hip)
# ======================================================================================================================
_COV_MODEL_ID = {"spherical": 0, "exponential": 1, "gaussian": 2, "cubic": 3, "stable": 4}


def _cov_double_sum(coords_a, errors_a, coords_b, errors_b, params_variogram_model, ctx: _lib.Context | None = None) -> float:
    """sum_i sum_j e_i e_j rho(d_ij) on the device (``xdemhip_cov_double_sum``); coords_b None = the A set itself."""
    from . import variogram_models as vm

    _check_validity_params_variogram(params_variogram_model)
    names = [vm.model_name(m) for m in params_variogram_model["model"].values]
    for n in names:
        if n not in _COV_MODEL_ID:
            raise NotImplementedError(f"Variogram model '{n}' is not available on the HIP engine (no modified Bessel function there).")
    ctx = ctx or _lib.default_context()

    def col(a, k=None):
        return np.ascontiguousarray(np.asarray(a, dtype=np.float64) if k is None else np.asarray(a, dtype=np.float64)[:, k])

    ax, ay, ae = col(coords_a, 0), col(coords_a, 1), col(errors_a)
    if coords_b is None:
        bx = by = be = None
        nb = 0
    else:
        bx, by, be = col(coords_b, 0), col(coords_b, 1), col(errors_b)
        nb = bx.size
    k = len(names)
    types = (ctypes.c_int * k)(*[_COV_MODEL_ID[n] for n in names])
    rng_ = np.ascontiguousarray(params_variogram_model["range"].values, dtype=np.float64)
    sil = np.ascontiguousarray(params_variogram_model["psill"].values, dtype=np.float64)
    smooth = np.ones(k)
    if "smooth" in params_variogram_model:
        sm = np.asarray(params_variogram_model["smooth"].values, dtype=np.float64)
        smooth = np.where(np.isfinite(sm), sm, 1.0)
    out = ctypes.c_double()
    ctx.check(ctx._L.xdemhip_cov_double_sum(ctx.handle, dp(ax), dp(ay), dp(ae), ax.size, dp(bx), dp(by), dp(be), nb, k, types,
                                            dp(rng_), dp(sil), dp(np.ascontiguousarray(smooth)), ctypes.byref(out), _lib.HOST))
    return float(out.value)


def neff_circular_approx_theoretical(area: float, params_variogram_model) -> float:
    """Number of effective samples over a disk of the given area from the closed-form radial integrals of the spherical,
    exponential, gaussian and cubic covariances (after Rolstad et al., 2009; mirror of xdem/spatialstats.py:2011-2114)."""
    from . import variogram_models as vm

    _check_validity_params_variogram(params_variogram_model)
    L = np.sqrt(area / np.pi)
    squared_se = 0.0
    for i in range(len(params_variogram_model)):
        name = vm.model_name(params_variogram_model["model"].values[i])
        a1, c1 = params_variogram_model["range"].values[i], params_variogram_model["psill"].values[i]
        if name == "spherical":
            squared_se += c1 * (1 - L / a1 + 1 / 5 * (L / a1) ** 3) if L <= a1 else c1 / 5 * (a1 / L) ** 2
        elif name == "exponential":
            a = a1 / 3
            squared_se += 2 * c1 * (a / L) ** 2 * (1 - np.exp(-L / a) * (1 + L / a))
        elif name == "gaussian":
            a = a1 / 2
            squared_se += c1 * (a / L) ** 2 * (1 - np.exp(-(L**2) / a**2))
        elif name == "cubic":
            squared_se += (c1 * (6 * a1**7 - 21 * a1**5 * L**2 + 21 * a1**4 * L**3 - 6 * a1**2 * L**5 + L**7) / (6 * a1**7)
                           if L <= a1 else 1 / 6 * c1 * a1**2 / L**2)
    return np.nansum(params_variogram_model.psill) / squared_se


def neff_circular_approx_numerical(area: float, params_variogram_model) -> float:
    """Same by numerical integration of h * covariance(h) over the disk, for any sum of models (spatialstats.py:2129-2172)."""
    from scipy import integrate

    _check_validity_params_variogram(params_variogram_model)
    total_sill = np.nansum(params_variogram_model.psill)
    cov = covariance_from_variogram(params_variogram_model)
    h_equiv = np.sqrt(area / np.pi)
    full_int = integrate.quad(lambda h: h * cov(h), 0, h_equiv)[0]
    return total_sill / (2 * np.pi * full_int / area)


def neff_exact(coords, errors, params_variogram_model, vectorized: bool = True, ctx: _lib.Context | None = None) -> float:
    """Exact number of effective samples from the double sum of covariances over all ordered point pairs (mirror of
    xdem/spatialstats.py:2175-2236; the N x N work runs on the GPU, no N x N matrix is formed)."""
    errors = np.asarray(errors, dtype=np.float64)
    n = len(coords)
    var = _cov_double_sum(coords, errors, None, None, params_variogram_model, ctx)
    return float(np.mean(errors)) ** 2 / (var / n**2)


def neff_hugonnet_approx(coords, errors, params_variogram_model, subsample: int = 1000, vectorized: bool = True, random_state=None,
                         ctx: _lib.Context | None = None) -> float:
    """Approximate number of effective samples: one of the two sums runs over a random subset (Hugonnet et al., 2022; mirror
    of xdem/spatialstats.py:2239-2308, same random draw)."""
    rng = np.random.default_rng(random_state)
    coords = np.asarray(coords, dtype=np.float64)
    errors = np.asarray(errors, dtype=np.float64)
    n = len(coords)
    subsample = min(subsample, n)
    rand_points = rng.choice(n, size=subsample, replace=False)
    var = _cov_double_sum(coords, errors, coords[rand_points, :], errors[rand_points], params_variogram_model, ctx)
    return float(np.mean(errors)) ** 2 / (var / (n * subsample))


def number_effective_samples(area, params_variogram_model, rasterize_resolution=None, **kwargs: Any) -> float:
    """Number of effective (uncorrelated) samples in an area for a sum of variogram models; mirror of
    ``xdem.spatialstats.number_effective_samples`` (xdem/spatialstats.py:2311-2404).

    A numeric ``area`` takes the continuous disk approximation (host SciPy integration, as upstream).  An ``xdem_amd.Vector`` area is
    burnt on the GPU into a grid of ``rasterize_resolution`` -- a number (the grid of ``Vector.create_mask(res=)``, coordinates
    relative) or a Raster-like object (its grid, the coordinates of its pixel centres) -- as upstream's two constructions do.  The
    rasterised area itself is taken too: a 2-D boolean ``area`` mask on a grid of ``rasterize_resolution``.  The double sum of
    covariances runs on the GPU (``neff_hugonnet_approx``; ``kwargs`` go to it)."""
    from .vector import Vector

    _check_validity_params_variogram(params_variogram_model)
    if isinstance(area, Vector):
        if rasterize_resolution is None:
            rasterize_resolution = np.min(params_variogram_model["range"].values) / 5.0
            warnings.warn(
                "Resolution for vector rasterization is not defined and thus set at 20% of the shortest "
                "correlation range, which might result in large memory usage."
            )
        if isinstance(rasterize_resolution, (float, int, np.floating, np.integer)):
            area = area.create_mask(res=rasterize_resolution)   # (the bool-mask branch below builds upstream's relative coordinates)
        elif hasattr(rasterize_resolution, "transform") and hasattr(rasterize_resolution, "shape"):
            shape, t6 = tuple(rasterize_resolution.shape)[-2:], tuple(rasterize_resolution.transform)
            mask = area.create_mask((shape, t6))
            xc = t6[2] + (np.arange(shape[1]) + 0.5) * t6[0]
            yc = t6[5] + (np.arange(shape[0]) + 0.5) * t6[4]
            coords_on_mask = np.array(np.meshgrid(xc, yc))[:, mask].T
            return neff_hugonnet_approx(coords=coords_on_mask, errors=np.ones(len(coords_on_mask)),
                                        params_variogram_model=params_variogram_model, **kwargs)
        else:
            raise ValueError("The rasterize resolution must be a float, integer or Raster subclass.")
    if isinstance(area, (float, int)) and not isinstance(area, bool):
        return neff_circular_approx_numerical(area=area, params_variogram_model=params_variogram_model)
    if isinstance(area, np.ndarray) and area.dtype == bool and area.ndim == 2:
        mask = area
        if rasterize_resolution is None:
            rasterize_resolution = np.min(params_variogram_model["range"].values) / 5.0
            warnings.warn(
                "Resolution for vector rasterization is not defined and thus set at 20% of the shortest "
                "correlation range, which might result in large memory usage."
            )
        if not isinstance(rasterize_resolution, (float, int, np.floating, np.integer)):
            raise ValueError("The rasterize resolution must be a float, integer or Raster subclass.")
        x = rasterize_resolution * np.arange(0, mask.shape[0])
        y = rasterize_resolution * np.arange(0, mask.shape[1])
        coords = np.array(np.meshgrid(y, x))
        coords_on_mask = coords[:, mask].T
        errors_on_mask = np.ones(len(coords_on_mask))  # heteroscedasticity does not matter here: errors standardized to one
        return neff_hugonnet_approx(coords=coords_on_mask, errors=errors_on_mask, params_variogram_model=params_variogram_model,
                                    **kwargs)
    raise ValueError("Area must be a float, integer, Vector subclass or geopandas dataframe.")


def spatial_error_propagation(areas, errors, params_variogram_model, **kwargs: Any) -> list:
    """Standard error (1-sigma) of the mean elevation error in each area: mean error / sqrt(number of effective samples); mirror
    of ``xdem.spatialstats.spatial_error_propagation`` (xdem/spatialstats.py:2407-2458) for the array-level inputs of
    ``number_effective_samples``: ``errors`` is the error map (array, masked array or Raster-like with ``.data`` / ``.res``),
    an area is a float (disk of that surface, mean over the whole map), a boolean mask on the map's grid or an ``xdem_amd.Vector``
    (burnt into the grid of Raster-like ``errors``)."""
    gsd = errors.res[0] if hasattr(errors, "res") and hasattr(errors, "data") else None
    arr = errors.data if gsd is not None else errors
    if isinstance(arr, np.ma.MaskedArray):
        arr = np.where(np.ma.getmaskarray(arr), np.nan, arr.data.astype(np.float64, copy=False))
    arr = np.asarray(arr)
    from .vector import Vector

    standard_errors = []
    for area in areas:
        if isinstance(area, Vector):   # (upstream: the errors' own grid for the area's coordinates, the mean error inside the outline)
            if gsd is None:
                raise ValueError("a Vector area needs the errors' grid: pass a Raster-like `errors` (.data, .transform)")
            kw = {k: v for k, v in kwargs.items() if k != "rasterize_resolution"}
            neff = number_effective_samples(area, params_variogram_model, rasterize_resolution=errors, **kw)
            average_spread = np.nanmean(arr[area.create_mask((tuple(arr.shape)[-2:], errors.transform))])
        elif isinstance(area, np.ndarray):
            if gsd is None and "rasterize_resolution" not in kwargs:
                raise ValueError("a mask area needs the grid spacing: pass a Raster-like `errors` or rasterize_resolution=")
            kw = dict(kwargs)
            res = kw.pop("rasterize_resolution", gsd)
            neff = number_effective_samples(area, params_variogram_model, rasterize_resolution=res, **kw)
            average_spread = np.nanmean(arr[area])
        else:
            kw = {k: v for k, v in kwargs.items() if k != "rasterize_resolution"}
            neff = number_effective_samples(area, params_variogram_model, **kw)
            # (upstream averages over the whole map for `float` areas only; an `int` area reaches its vector branch and fails)
            average_spread = np.nanmean(arr)
        standard_errors.append(average_spread / np.sqrt(neff))
    return standard_errors


# ======================================================================================================================
# Patches method: mirror of xdem/spatialstats.py:2597-3048 over csrc/meanfilter.hip
# ======================================================================================================================
def convolution(imgs: np.ndarray, filters: np.ndarray, method: str = "scipy", ctx: _lib.Context | None = None) -> np.ndarray:
    """Convolution of `n_N` images (N1 x N2) with `n_M` filters (M1 x M2): float64 array (n_N, n_M, N1, N2).  Drop-in for
    ``xdem.spatialstats.convolution`` (xdem/spatialstats.py:2558-2594), the engine under the reference's surface fit
    (surfit.py:1107) and mean filter, as ONE HIP kernel that reads an image once for all filters (``xdemhip_convolution``,
    csrc/convolve.hip).  `method` selects WHICH of upstream's two engines is reproduced bit for bit, not where it runs:
    "scipy" = ``scipy.ndimage.convolve(img, filter, mode="constant", cval=nan)`` (true convolution, zero weights skipped, NaN
    beyond the border, the float64 sum rounded to the image dtype), any name containing "numba" = upstream's Numba loop on the
    NaN-padded images (correlation over every tap, unrounded; an even filter size leaves the last row / column 0).
    Images must be float32 or float64 (SciPy's result for integer images under ``cval=nan`` is a C cast of NaN: refused);
    filters are taken as float64, as SciPy takes its weights.  torch device tensors are accepted for `imgs` and return a
    device tensor."""
    m = method.lower()
    if m != "scipy" and "numba" not in m:
        raise ValueError('Method must be "scipy" or "numba".')
    code = 0 if m == "scipy" else 1
    filt = np.ascontiguousarray(np.asarray(filters, dtype=np.float64))
    if filt.ndim != 3:
        raise ValueError(f"filters must have three dimensions (n_M, M1, M2), got shape {filt.shape}")
    n_f, m1, m2 = filt.shape
    ctx = ctx or _lib.default_context()
    device = _args.is_tensor(imgs)
    if device:
        import torch

        t = imgs.contiguous()
        if t.dim() != 3 or t.dtype not in (torch.float32, torch.float64) or not t.is_cuda:
            raise TypeError("convolution: a device tensor must be a float32 / float64 CUDA tensor of shape (n_N, N1, N2)")
        out = torch.empty((t.shape[0], n_f, t.shape[1], t.shape[2]), dtype=torch.float64, device=t.device)
    else:
        t = np.ascontiguousarray(imgs)
        if t.ndim != 3:
            raise ValueError(f"imgs must have three dimensions (n_N, N1, N2), got shape {t.shape}")
        if t.dtype not in _args.FLOATS:
            raise TypeError(f"convolution: images must be float32 or float64, got {t.dtype} (with cval=nan SciPy's result for other "
                            "dtypes is a C cast of NaN; convert the images first)")
        out = np.empty((t.shape[0], n_f, t.shape[1], t.shape[2]), dtype=np.float64)
        if out.size == 0:
            return out
    with ctx.call_lock:
        if device:
            ctx.set_stream(torch.cuda.current_stream(t.device).cuda_stream)
        rc = ctx._L.xdemhip_convolution(ctx.handle, ptr(t), _args.code(t), t.shape[0], t.shape[1], t.shape[2], dp(filt), n_f, m1, m2, code,
                                        ptr(out), _args.space(t))
    ctx.check(rc)
    return out


def mean_filter_nan(img: np.ndarray, kernel_size: int, kernel_shape: str = "circular", method: str = "scipy",
                    ctx: _lib.Context | None = None) -> tuple[np.ndarray, np.ndarray, int]:
    """Mean filter with a square or circular kernel that ignores NaNs; drop-in for ``xdem.spatialstats.mean_filter_nan``
    (2597-2655).  Returns (mean image, number of valid pixels per window, number of pixels in the kernel), the two images
    float64 like upstream's.  Runs the HIP kernel (``xdemhip_mean_filter_nan``), which reproduces the two
    ``scipy.ndimage.convolve(..., mode="constant", cval=nan)`` calls bit for bit: windows that leave the raster give
    (NaN, 0).  ``method`` ("scipy" / "numba" upstream) only names upstream's CPU engines and is accepted for signature
    compatibility.  Kernels of more than 127 pixels (``kernel_size`` > 11 square, > 13 circular) raise
    ``NotImplementedError``: upstream counts the valid pixels in an int8 image, which wraps beyond 127 (a 12 x 12 square
    reports -112 valid pixels) -- there is no meaningful result to reproduce."""
    if kernel_shape.lower() not in ("square", "circular"):
        raise ValueError('Kernel shape should be "square" or "circular".')
    if method.lower() != "scipy" and "numba" not in method.lower():
        raise ValueError('Method must be "scipy" or "numba".')
    arr = np.ascontiguousarray(img)
    if arr.ndim != 2:
        raise ValueError("img must be a 2D array")
    if arr.dtype not in (np.dtype(np.float32), np.dtype(np.float64)):
        arr = arr.astype(np.float64 if arr.dtype.itemsize > 4 else np.float32)
    ctx = ctx or _lib.default_context()
    mean = np.empty(arr.shape, dtype=np.float64)
    nvalid = np.empty(arr.shape, dtype=np.float64)
    npx = ctypes.c_int()
    rc = ctx._L.xdemhip_mean_filter_nan(ctx.handle, ptr(arr), _args.code(arr), arr.shape[0], arr.shape[1], int(kernel_size),
                                        0 if kernel_shape.lower() == "square" else 1, ptr(mean), ptr(nvalid), ctypes.byref(npx), _lib.HOST)
    if rc == -5:   # XDEMHIP_EUNSUPPORTED
        raise NotImplementedError(
            f"mean_filter_nan: a {kernel_shape} kernel of size {kernel_size} holds {npx.value if npx.value <= 127 else 'more than 127'} "
            "pixels; the reference counts valid pixels in an int8 image, which wraps beyond 127 pixels "
            "(xdem/spatialstats.py:2637-2646) -- such kernels are refused instead of reproducing the wrap-around."
        )
    ctx.check(rc)
    return mean, nvalid, int(npx.value)


def _patches_convolution(values: np.ndarray, gsd: float, area: float, perc_min_valid: float = 80.0, patch_shape: str = "circular",
                         method: str = "scipy", statistic_between_patches: Callable[[np.ndarray], Any] = nmad,
                         return_in_patch_statistics: bool = False):
    """Vectorized patches method: every pixel is the centre of a patch (``mean_filter_nan``), the statistic between patches is
    averaged over the kernel_size^2 sets of non-overlapping patches (xdem/spatialstats.py:2658-2741)."""
    import pandas as pd

    if patch_shape.lower() == "circular":
        kernel_size = int(np.round(2 * np.sqrt(area / np.pi) / gsd, decimals=0))   # the diameter
    elif patch_shape.lower() == "square":
        kernel_size = int(np.round(np.sqrt(area) / gsd, decimals=0))               # the side
    else:
        raise ValueError('Kernel shape should be "square" or "circular".')
    logging.info("Computing the convolution on the entire array...")
    mean_img, nb_valid_img, nb_pixel_per_kernel = mean_filter_nan(img=values, kernel_size=kernel_size, kernel_shape=patch_shape, method=method)
    mean_img[nb_valid_img < nb_pixel_per_kernel * perc_min_valid / 100.0] = np.nan
    logging.info("Computing statistic between patches for all independent combinations...")
    stats, nbs = [], []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)   # all-NaN subsets (upstream lets NumPy warn)
        for i in range(kernel_size):
            for j in range(kernel_size):
                sub = mean_img[i::kernel_size, j::kernel_size]
                stats.append(statistic_between_patches(sub.ravel()))
                nbs.append(np.count_nonzero(np.isfinite(sub)))
        average_statistic = float(np.nanmean(np.asarray(stats)))
        nb_independent_patches = float(np.nanmean(np.asarray(nbs)))
    exact_area = nb_pixel_per_kernel * gsd**2
    if return_in_patch_statistics:
        df = pd.DataFrame(data={"nanmean": mean_img[::kernel_size, ::kernel_size].ravel(),
                                "count": nb_valid_img[::kernel_size, ::kernel_size].ravel()})
        return average_statistic, nb_independent_patches, exact_area, df
    return average_statistic, nb_independent_patches, exact_area


def _patches_loop_quadrants(values: np.ndarray, gsd: float, area: float, patch_shape: str = "circular", n_patches: int = 1000,
                            perc_min_valid: float = 80.0, statistics_in_patch=(np.nanmean,),
                            statistic_between_patches: Callable[[np.ndarray], Any] = nmad, random_state=None,
                            return_in_patch_statistics: bool = False):
    """Patches method by random quadrants (xdem/spatialstats.py:2744-2879): host-side sampling of at most `n_patches` patches, any
    in-patch statistics (a few thousand small patches: not a dense array step, no kernel involved).  Upstream's bookkeeping is
    kept as it is -- for square patches "the exact number of pixels" is the number of quadrants, so square patches only ever
    qualify when kernel_size^2 happens to equal it."""
    import pandas as pd

    stats_in = list(statistics_in_patch) + ["count"]
    names = [f if isinstance(f, str) else f.__name__ for f in stats_in]
    rng = np.random.default_rng(random_state)
    nx, ny = np.shape(values)
    kernel_size = int(np.round(np.sqrt(area) / gsd, decimals=0))
    nx_sub, ny_sub = int(np.floor((nx - 1) / kernel_size)), int(np.floor((ny - 1) / kernel_size))
    rad = int(np.round(np.sqrt(area / np.pi) / gsd, decimals=0))
    if patch_shape.lower() == "square":
        nb_pixel_exact = nx_sub * ny_sub
    elif patch_shape.lower() == "circular":
        nb_pixel_exact = np.count_nonzero(_create_circular_mask(shape=(nx, ny), radius=rad))
    else:
        raise ValueError("Patch method must be square or circular.")
    exact_area = nb_pixel_exact * gsd**2
    quadrants = [[i, j] for i in range(nx_sub) for j in range(ny_sub)]
    u, remaining = 0, n_patches
    rows = []
    while len(quadrants) > 0 and u < n_patches:
        drawn = rng.choice(len(quadrants), size=min(len(quadrants), 10 * remaining))
        for iq in drawn:
            i, j = quadrants[iq]
            if patch_shape.lower() == "square":
                patch = values[kernel_size * i : kernel_size * (i + 1), kernel_size * j : kernel_size * (j + 1)].flatten()
            else:
                center = (np.floor(kernel_size * (i + 1 / 2)), np.floor(kernel_size * (j + 1 / 2)))
                patch = values[_create_circular_mask((nx, ny), center=center, radius=rad)]
            nb_total = len(patch)
            valid = patch[np.isfinite(patch)]
            if len(valid) >= np.ceil(perc_min_valid / 100.0 * nb_total) and nb_total == nb_pixel_exact:
                u += 1
                if u > n_patches:
                    break
                row = {"tile": f"{i}_{j}"}
                for name, stat in zip(names, stats_in):
                    if isinstance(stat, str):
                        if stat != "count":
                            raise ValueError('No other string than "count" are supported for named statistics.')
                        row[stat] = len(valid)
                    else:
                        row[name] = stat(valid.astype("float64"))
                rows.append(row)
        remaining = n_patches - u
        taken = {int(q) for q in drawn}
        quadrants = [c for q, c in enumerate(quadrants) if q not in taken]
    if rows:
        df_all = pd.DataFrame(rows)
        average_statistic = float(statistic_between_patches(df_all[names[0]].values))
        nb_independent_patches = np.count_nonzero(np.isfinite(df_all[names[0]].values))
    else:
        df_all = pd.DataFrame({name: [np.nan] for name in names})
        average_statistic, nb_independent_patches = np.nan, 0
        warnings.warn("No valid patch found covering this area size, returning NaN for statistic.")
    if return_in_patch_statistics:
        return average_statistic, nb_independent_patches, exact_area, df_all
    return average_statistic, nb_independent_patches, exact_area


def patches_method(values, areas: list[float], gsd: float = None, stable_mask=None, unstable_mask=None,
                   statistics_in_patch=(np.nanmean,), statistic_between_patches: Callable[[np.ndarray], Any] = nmad,
                   perc_min_valid: float = 80.0, patch_shape: str = "circular", vectorized: bool = True,
                   convolution_method: str = "scipy", n_patches: int = 1000, return_in_patch_statistics: bool = False,
                   random_state=None):
    """Monte-Carlo patches method: empirical standard error of the mean over patches of given areas; drop-in for
    ``xdem.spatialstats.patches_method`` (2928-3048) for arrays (or Raster-like objects with ``.data`` / ``.res``) and boolean
    array masks (an ``xdem_amd.Vector`` mask is burnt into the grid of Raster-like `values`).  ``vectorized=True`` runs the mean filter on the GPU
    for every pixel at once; ``False`` samples quadrants on the host."""
    import pandas as pd

    stable_mask, unstable_mask = _burn_vector_masks((stable_mask, unstable_mask), values)
    if hasattr(values, "res") and hasattr(values, "data"):
        gsd = values.res[0] if gsd is None else gsd
        values = values.data
    if not isinstance(values, np.ndarray):
        raise ValueError("The values must be a Raster or NumPy array, or a list of those.")
    for m_ in (stable_mask, unstable_mask):
        if m_ is not None and not isinstance(m_, np.ndarray):
            raise NotImplementedError("stable / unstable masks must be boolean arrays here (vector masks need rasterisation: out of scope)")
    if gsd is None:
        raise ValueError("The ground sampling distance must be provided if no Raster object is passed.")
    if isinstance(values, np.ma.MaskedArray):
        arr = np.array(values.data, dtype=values.dtype if np.issubdtype(values.dtype, np.floating) else np.float32, copy=True)
        arr[np.ma.getmaskarray(values)] = np.nan
    else:
        arr = np.array(values, dtype=values.dtype if np.issubdtype(values.dtype, np.floating) else np.float32, copy=True)
    include = np.ones(arr.shape, dtype=bool) if stable_mask is None else np.asarray(stable_mask, dtype=bool).reshape(arr.shape)
    exclude = np.zeros(arr.shape, dtype=bool) if unstable_mask is None else np.asarray(unstable_mask, dtype=bool).reshape(arr.shape)
    arr[~(include & ~exclude)] = np.nan      # masked terrain -> NaN, shape preserved (spatialstats.py:737-760)
    list_stats, list_nb, list_exact, list_df = [], [], [], []
    for area in areas:
        if vectorized:
            outputs = _patches_convolution(arr, gsd, area, perc_min_valid, patch_shape, convolution_method, statistic_between_patches,
                                           return_in_patch_statistics)
        else:
            outputs = _patches_loop_quadrants(arr, gsd, area, patch_shape, n_patches, perc_min_valid, statistics_in_patch,
                                              statistic_between_patches, random_state, return_in_patch_statistics)
        list_stats.append(outputs[0])
        list_nb.append(outputs[1])
        list_exact.append(outputs[2])
        if return_in_patch_statistics:
            df = outputs[3]
            df["areas"] = area
            df["exact_areas"] = outputs[2]
            list_df.append(df)
    df_statistic = pd.DataFrame(data={statistic_between_patches.__name__: list_stats, "nb_indep_patches": list_nb,
                                      "exact_areas": list_exact, "areas": areas})
    if return_in_patch_statistics:
        return df_statistic, pd.concat(list_df)
    return df_statistic
