"""NumPy oracles of three one-shot entry points (test infrastructure, not a fall-back of the product):

  * ``perbin_tables``  -- xdemhip_perbin_lookup (csrc/perbin.hip) on the flat tables the C entry point takes, by upstream's masks;
  * ``grid_linear``    -- xdemhip_interp_grid_linear (csrc/binstats.hip) with the operation order of csrc/grid_interp.h;
  * ``cov_reference``  -- xdemhip_cov_double_sum (csrc/covsum.hip): the per-pair terms in float64 with the kernel's expression order,
                          and their sum evaluated in long double and added exactly.

tests/test_lookup_routes_host.py ties each of them to an independent reference (the recorded outputs of the reference project,
SciPy's RegularGridInterpolator, the long-double evaluation)."""
import itertools
import math

import numpy as np

SPHERICAL, EXPONENTIAL, GAUSSIAN, CUBIC, STABLE = range(5)
KIND_NAMES = ("spherical", "exponential", "gaussian", "cubic", "stable")


# ---- per-bin lookup ----------------------------------------------------------------------------------------------------------------
def perbin_tables(variables, n_int, left, right, table, passb):
    """(out, n_missing) of upstream's walk (xdem/spatialstats.py:499-525) over flat tables: the bins in itertools.product order, the
    last variable fastest; the mask of a bin is ``(v >= left) & (v < right)`` over every variable, in float64; a bin of pass byte 1
    writes its value, 0 writes nothing, 2 adds the mask's population to the count; later bins overwrite earlier ones.  Nothing here
    knows whether the intervals are disjoint."""
    var = [np.asarray(v).astype(np.float64) for v in variables]
    n_int = [int(c) for c in n_int]
    left, right, table, passb = np.asarray(left), np.asarray(right), np.asarray(table), np.asarray(passb)
    assert len(var) == len(n_int) and left.size == right.size == sum(n_int) and table.size == passb.size == math.prod(n_int)
    off = np.cumsum([0] + n_int)
    # one mask per interval of every variable (as upstream), combined per bin
    masks = [[(var[k] >= left[off[k] + j]) & (var[k] < right[off[k] + j]) for j in range(n_int[k])] for k in range(len(var))]
    out = np.full(var[0].size, np.nan)
    n_missing = 0
    for b, combo in enumerate(itertools.product(*[range(c) for c in n_int])):
        m = masks[0][combo[0]]
        for k in range(1, len(var)):
            m = m & masks[k][combo[k]]
        if passb[b] == 1:
            out[m] = table[b]
        elif passb[b] == 2:
            n_missing += int(np.count_nonzero(m))
    return out, n_missing


# ---- multilinear interpolation -----------------------------------------------------------------------------------------------------
def grid_linear(axes, V, X, scale, with_bound=False):
    """``scale *`` the multilinear interpolant of the grid values `V` (C order over `axes`) at the points `X` (one array per
    dimension, float32 or float64), NaN where a coordinate is NaN, in float64 with the operations of csrc/grid_interp.h in their order:
    interval ``clip(searchsorted(g, x, 'right') - 1, 0, m - 2)``, ``y = (x - g[i]) / (g[i+1] - g[i])``, the corners in
    itertools.product order (first dimension slowest), each weight multiplied left to right from 1.0 by ``y`` or ``1.0 - y``,
    ``value = value + V * w``, one final ``scale * value``.

    with_bound: also ``2^-52 (3 nd + 2^nd) sum_c |V_c| prod_d max(1, |y_d|, |1 - y_d|)`` per point, which bounds what another order of
    the same operations can differ by (at most 3 nd roundings per weight, 2^nd in the sum; absolute in the corners' magnitudes because
    ``1 - y`` loses relative accuracy near y = 1)."""
    nd = len(axes)
    axes = [np.asarray(g, dtype=np.float64) for g in axes]
    shape = tuple(g.size for g in axes)
    V = np.asarray(V, dtype=np.float64).reshape(shape)
    x = [np.asarray(c).astype(np.float64) for c in X]
    idx, y = [], []
    for d in range(nd):
        g = axes[d]
        i = np.clip(np.searchsorted(g, x[d], side="right") - 1, 0, g.size - 2)
        idx.append(i)
        with np.errstate(invalid="ignore"):
            y.append((x[d] - g[i]) / (g[i + 1] - g[i]))
    value = np.zeros(x[0].size)
    mags = np.zeros(x[0].size)
    with np.errstate(invalid="ignore"):
        for corner in itertools.product((0, 1), repeat=nd):
            w = np.ones(x[0].size)
            for d in range(nd):
                w = w * (y[d] if corner[d] else (1.0 - y[d]))
            vc = V[tuple(idx[d] + corner[d] for d in range(nd))]
            value = value + vc * w
            mags = mags + np.abs(vc)
        out = np.float64(scale) * value
    isnan_any = np.zeros(x[0].size, bool)
    for d in range(nd):
        isnan_any |= np.isnan(x[d])
    out[isnan_any] = np.nan
    if not with_bound:
        return out
    grow = np.ones(x[0].size)
    for d in range(nd):
        grow = grow * np.fmax(1.0, np.fmax(np.abs(y[d]), np.abs(1.0 - y[d])))
    return out, 2.0 ** -52 * (3 * nd + 2 ** nd) * mags * grow * abs(float(scale))


# ---- covariance double sum ---------------------------------------------------------------------------------------------------------
def cov_rho(models, h):
    """``1 - sum_m gamma_m(h) / sill`` as ``cov_rho`` of csrc/covsum.hip writes it, in the floating-point type of `h` (float64: the
    kernel's operations in their order; long double: the reference).  models: (kind, range, partial sill, smoothness) each."""
    ft = h.dtype.type
    c = lambda v: ft(v)   # noqa: E731 -- every constant below is exact in both types
    sill = ft(0.0)
    for _, _, c0, _ in models:
        sill = sill + ft(c0)
    inv_sill = c(1.0) / sill
    g = np.zeros_like(h)
    for kind, r, c0, s in models:
        r, c0 = ft(r), ft(c0)
        if kind == SPHERICAL:
            x = h / r
            v = np.where(h <= r, c0 * (c(1.5) * x - c(0.5) * x * x * x), c0)
        elif kind == EXPONENTIAL:
            v = c0 * (c(1.0) - np.exp(-h / (r / c(3.0))))
        elif kind == GAUSSIAN:
            a = r / c(2.0)
            v = c0 * (c(1.0) - np.exp(-(h * h) / (a * a)))
        elif kind == CUBIC:
            x = h / r
            x2 = x * x
            v = np.where(h < r, c0 * (c(7.0) * x2 - c(8.75) * x2 * x + c(3.5) * x2 * x2 * x - c(0.75) * x2 * x2 * x2 * x), c0)
        elif kind == STABLE:
            s = ft(s)
            a = r / np.power(c(3.0), c(1.0) / s)
            v = c0 * (c(1.0) - np.exp(-np.power(h / a, s)))
        else:
            raise ValueError(kind)
        g = g + v
    return c(1.0) - g * inv_sill


COV_EXACT_PAIRS = 5_000_000   # up to here every term goes through one math.fsum


def cov_reference(a, b, models, rows=256):
    """The double sum over the pairs of the point sets a = (x, y, e) and b (None: a itself), evaluated over `rows` points of a at a time.

    Returns a dict: ``S_ref`` -- the terms ``e_i (e_j rho(h_ij))`` with ``h = sqrt(dx dx + dy dy)`` evaluated in long double (64-bit
    mantissa) and added by ONE math.fsum over the float64 head and tail of every term, i.e. rounded once, and ``S_err = 0``.  Beyond
    COV_EXACT_PAIRS pairs the terms of a block of rows are added in long double by NumPy instead, and math.fsum adds the heads and tails
    of the blocks' sums: whatever the order of the m additions of a block, its sum is off by at most ``(m - 1) 2^-64 sum |terms|`` to
    first order, so ``S_err = 1.001 m 2^-64 T`` bounds |S_ref - the exact sum|, and the tests add it to their bound.
    ``S64`` -- the float64 terms, each block added by math.fsum (or, beyond COV_EXACT_PAIRS, in long double) and the blocks' sums by
    math.fsum: a checked quantity, not a reference; ``T = sum |terms|`` and ``A = sum |e_i e_j|`` (float64); ``k_pair`` -- the largest
    ``|rho_float64 - rho_longdouble| / 2^-52`` over the pairs; ``h_zero``, ``h_on_range`` -- the numbers of pairs at a distance of
    exactly 0 and of exactly one of the models' ranges."""
    ld = np.longdouble
    assert np.finfo(ld).nmant >= 63, "long double is double here: evaluate the reference in mpmath instead"
    ax, ay, ae = (np.asarray(v, dtype=np.float64) for v in a)
    bx, by, be = (ax, ay, ae) if b is None else (np.asarray(v, dtype=np.float64) for v in b)
    exact = ax.size * bx.size <= COV_EXACT_PAIRS
    ranges = sorted({float(m[1]) for m in models})
    lbx, lby, lbe = bx.astype(ld), by.astype(ld), be.astype(ld)
    st = {"T": 0.0, "A": 0.0, "k_pair": 0.0, "h_zero": 0, "h_on_range": 0, "parts64": []}

    def heads_and_tails():
        for i0 in range(0, ax.size, rows):
            sl = slice(i0, i0 + rows)
            dx, dy = ax[sl, None] - bx[None, :], ay[sl, None] - by[None, :]
            h = np.sqrt(dx * dx + dy * dy)
            rho = cov_rho(models, h)
            terms = ae[sl, None] * (be[None, :] * rho)
            ldx, ldy = ax[sl, None].astype(ld) - lbx[None, :], ay[sl, None].astype(ld) - lby[None, :]
            rho_ld = cov_rho(models, np.sqrt(ldx * ldx + ldy * ldy))
            terms_ld = (ae[sl, None].astype(ld) * (lbe[None, :] * rho_ld)).ravel()
            st["parts64"].append(math.fsum(terms.ravel().tolist()) if exact else float(terms.astype(ld).sum()))
            st["T"] += float(np.abs(terms).sum())
            st["A"] += float(np.abs(ae[sl, None] * be[None, :]).sum())
            st["k_pair"] = max(st["k_pair"], float(np.abs(rho.astype(ld) - rho_ld).max()) / 2.0 ** -52)
            st["h_zero"] += int(np.count_nonzero(h == 0.0))
            st["h_on_range"] += int(sum(np.count_nonzero(h == r) for r in ranges))
            if not exact:
                terms_ld = terms_ld.sum(keepdims=True)
            hi = terms_ld.astype(np.float64)
            yield from hi.tolist()
            yield from (terms_ld - hi.astype(ld)).astype(np.float64).tolist()

    s_ref = math.fsum(heads_and_tails())
    parts64 = st.pop("parts64")
    s_err = 0.0 if exact else 1.001 * min(rows, ax.size) * bx.size * 2.0 ** -64 * st["T"]
    return {"S_ref": s_ref, "S_err": s_err, "S64": math.fsum(parts64), **st}
