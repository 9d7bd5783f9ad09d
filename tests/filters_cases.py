"""The inputs of the filter tests (tests/test_filters_host.py, tests/test_filters_gpu.py): planes, parameters, and which route each takes.

Planes (``case(switch, name, dtype)``; read-only, made once).  Elevation-like ones are 1500 + 100 N(0, 1), dDEM-like ones 5 N(0, 1); none
holds a zero of either sign (the device orders -0.0 below +0.0, NumPy does not say).  Voids are scattered pixels plus a block of
10 x 10 pixels, larger than the largest window (9).

  (a) ``elev``, ``ddem``   (2 T_r + 3) x (2 T_c + 5), T_r x T_c the largest tile ``xdemhip_filter_plan`` gives any of the parameter sets
                           below: under ``"filter_route"`` 1 (also used for 0 and 2) and under 3 (minimal tiles), so nine partial tiles exist
  (b) ``small``            5 x 7: smaller than the Gaussian radius for sigma = 2.5 (lw = 10), so the mirror repeats
  (c) ``row``, ``column``  1 x 37 and 37 x 1
  (d) ``all_nan``, ``no_nan``
  (e) ``inf``              one +Inf and one -Inf among values and a few NaNs

Parameters (``FILTERS``).  Median sizes 3 and 5 are sorted in registers (kernel modes FW_MED3 / FW_MED5 of csrc/filter.hip), size 9 is
beyond the register route and takes the bisection on the key bits; both run under the tiled and under the global route.  Minimum,
maximum, mean and distance walk the footprint; sigma 0.6 gives lw = 2 and sigma 2.5 gives lw = 10.  ``distance`` takes its threshold from
the case: 1.2 times the spread of the plane, which removes some pixels and not all."""
from __future__ import annotations

import functools

import numpy as np

from xdem_amd import filters

SWITCHES = (0, 1, 2, 3)
DTYPES = (np.float32, np.float64)
SIGMAS = (0.6, 2.5)
SIZES = (3, 5, 9)
FILTERS = (
    [("gaussian", {"sigma": s}) for s in SIGMAS] +
    [("gaussian", {"sigma": 0.6, "normalise": True}), ("gaussian", {"sigma": 2.5, "normalise": False})] +
    [(m, {"size": s}) for m in ("median", "min", "max") for s in SIZES] +
    [("mean", {"size": 3}), ("mean", {"size": 7}), ("mean", {"radius": 1}), ("mean", {"radius": 4})] +
    [("distance", {"radius": 3})]
)
BLOCK = 10   # side of the void block: larger than the largest window


def label(method, kw) -> str:
    return method + "".join(f"-{k}{v}" for k, v in kw.items())


def halo_of(method, kw) -> int:
    if method == "gaussian":
        return filters.gaussian_radius(kw["sigma"], kw.get("truncate", 4.0))
    return kw["size"] // 2 if "size" in kw else kw["radius"]


def plan_switch(switch: int) -> int:
    """The planes of switches 0, 1 and 2 are sized under switch 1, those of switch 3 under switch 3."""
    return 3 if switch == 3 else 1


@functools.lru_cache(maxsize=None)
def big_shape(switch: int) -> tuple[int, int]:
    tr = tc = 0
    for method, kw in FILTERS:
        for dt in DTYPES:
            p = filters.filter_plan(64, 64, method, halo_of(method, kw), dt, plan_switch(switch))
            tr, tc = max(tr, p["tile_rows"]), max(tc, p["tile_cols"])
    return 2 * tr + 3, 2 * tc + 5


def _values(rng, shape, kind):
    return 1500.0 + 100.0 * rng.standard_normal(shape) if kind == "elev" else 5.0 * rng.standard_normal(shape)


def _voids(rng, a, fraction=0.08, block=True):
    a.reshape(-1)[rng.random(a.size) < fraction] = np.nan
    if block:
        H, W = a.shape
        r0, c0 = max(0, H // 2 - BLOCK // 2), max(0, W // 3)
        a[r0:r0 + BLOCK, c0:c0 + BLOCK] = np.nan
    return a


SCALE = {"elev": 100.0, "ddem": 5.0, "small": 100.0, "row": 5.0, "column": 5.0, "all_nan": 1.0, "no_nan": 100.0, "inf": 5.0}
NAMES = tuple(SCALE)


@functools.lru_cache(maxsize=None)
def _case64(switch: int, name: str) -> np.ndarray:
    rng = np.random.default_rng([17, plan_switch(switch), NAMES.index(name)])
    if name in ("elev", "ddem"):
        a = _voids(rng, _values(rng, big_shape(switch), name))
    elif name == "small":
        a = _values(rng, (5, 7), "elev")
        a[1, 2] = a[4, 6] = np.nan
    elif name in ("row", "column"):
        a = _voids(rng, _values(rng, (1, 37) if name == "row" else (37, 1), "ddem"), 0.15, block=False)
    elif name == "all_nan":
        a = np.full((6, 9), np.nan)
    elif name == "no_nan":
        a = _values(rng, big_shape(switch), "elev")
    else:
        a = _voids(rng, _values(rng, (13, 18), "ddem"), 0.1, block=False)
        a[3, 4], a[9, 12] = np.inf, -np.inf
    return a


@functools.lru_cache(maxsize=None)
def case(switch: int, name: str, dtype) -> np.ndarray:
    a = np.ascontiguousarray(_case64(switch, name).astype(dtype))
    assert not np.any(a == 0)
    a.setflags(write=False)
    return a


def kwargs_for(method, kw, name) -> dict:
    """The keywords of a call on a case: ``distance`` gets the case's threshold."""
    return dict(kw, outlier_threshold=1.2 * SCALE[name]) if method == "distance" else dict(kw)
