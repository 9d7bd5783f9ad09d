"""Golden vectors for ``xdem_amd.dDEM`` and ``xdem_amd.DEMCollection``, recorded from the REFERENCE's own classes (needs the reference
source tree, so it runs only where that tree is present; the fixtures it writes are what the tests read).  Data only:
tests/golden/demcollection_golden.npz and tests/golden/signatures_ddem.json.

The reference's classes sit on geoutils, which is absent; its methods run on duck-typed stand-ins:

1. ``dDEM`` is instantiated on a namespace raster (its ``__init__`` takes over the raster's ``__dict__``): ``time``, ``filled_data``
   (getter, setter and its assertion), ``fill_method`` and ``interpolate``'s refusals are the reference's.
2. ``DEMCollection.get_dh_series``, ``get_dv_series``, ``get_cumulative_series`` and ``get_ddem_mask`` (empty outlines) are called
   unbound on a namespace with ``ddems``, ``reference_dem.res``, ``reference_timestamp`` and ``outlines`` that forwards the three
   methods they call back to the unbound ones.  The dDEMs are NumPy's ``ref - dem`` of tests/demcollection_cases.stack, the filled
   ones the reference's ``xdem.volume.hypsometric_interpolation`` inside the case's mask.
3. ``DEMCollection.__init__`` runs with a stand-in ``DEM`` class set on the stub ``xdem`` package: ``reference_index``, ``timestamps``
   and ``reference_timestamp`` for sorted and unsorted stamps and both forms of ``reference_dem``.

Recorded per shape, dtype and variant of demcollection_cases.VARIANTS: the dh frame, the dv series, both cumulative series (indexes as
int64 nanoseconds) and the warnings' texts; the constructor's figures; the messages of upstream's errors; the signatures.

    python tools/gen_golden_demcollection.py
"""
from __future__ import annotations

import importlib
import json
import os
import sys
import types
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
import _refimport  # noqa: E402
import demcollection_cases as dc  # noqa: E402
from gen_golden_volume import load_reference, signature_of  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
CTOR_CASES = {"sorted_first": ((1990, 2000, 2010, 2020), 0), "sorted_third": ((1990, 2000, 2010, 2020), 2),
              "unsorted_first": ((2010, 1990, 2020, 2000), 0), "unsorted_object": ((2010, 1990, 2020, 2000), "object:1")}


def message_of(fn) -> str:
    try:
        fn()
    except Exception as e:  # noqa: BLE001
        return f"{type(e).__name__}: {e}"
    raise AssertionError("no error raised")


def main() -> None:
    volume = load_reference()
    import geoutils

    geoutils.Vector = type("Vector", (), {})   # isinstance() sentinel, never instantiated
    ref_dc = importlib.import_module("xdem.demcollection").DEMCollection
    ref_ddem = importlib.import_module("xdem.ddem").dDEM

    class StandInDEM(_refimport._Raster):
        datetime = None

        def __init__(self, tag):
            self.tag = tag

    sys.modules["xdem"].DEM = StandInDEM

    def collection_of(ddems, reference_timestamp):
        ns = types.SimpleNamespace(ddems=ddems, reference_dem=types.SimpleNamespace(res=dc.RES), reference_timestamp=reference_timestamp, outlines={})
        ns.get_ddem_mask = lambda ddem, outlines_filter=None: ref_dc.get_ddem_mask(ns, ddem, outlines_filter)
        ns.get_dh_series = lambda **kw: ref_dc.get_dh_series(ns, **kw)
        ns.get_dv_series = lambda **kw: ref_dc.get_dv_series(ns, **kw)
        return ns

    rec: dict = {}
    texts: dict = {}
    stamps = np.array(dc.stamps()).astype("datetime64[ns]")
    t_ref = stamps[dc.REFERENCE]
    for H, W in dc.SHAPES:
        for dtype in dc.DTYPES:
            s = dc.stack(H, W, dtype)
            ref = s["dems"][dc.REFERENCE]
            ddems = []
            for t, dem in enumerate(s["dems"]):
                with np.errstate(invalid="ignore"):
                    data = np.zeros_like(ref) if t == dc.REFERENCE else ref - dem
                raster = types.SimpleNamespace(data=data, transform=dc.TRANSFORM, crs=None, nodata=None)
                if t == dc.REFERENCE:
                    ddems.append(ref_ddem(raster, start_time=t_ref, end_time=t_ref, error=0))
                else:
                    ddems.append(ref_ddem(raster, start_time=min(t_ref, stamps[t]), end_time=max(t_ref, stamps[t])))
            ns = collection_of(ddems, t_ref)
            assert ref_dc.get_ddem_mask(ns, ddems[0]).all()   # (empty outlines: every pixel)
            assert [d.fill_method for d in ddems] == [""] * len(ddems) and ddems[0].time == t_ref - stamps[0]
            for variant in dc.VARIANTS:
                state, region = variant.split("_")
                if state == "filled" and ddems[0]._filled_data is None:
                    for t, d in enumerate(ddems):
                        with warnings.catch_warnings():
                            warnings.simplefilter("ignore")
                            d.filled_data = volume.hypsometric_interpolation(d.data, ref, mask=s["mask"]).data
                mask = None if region == "full" else s["mask"]
                with warnings.catch_warnings(record=True) as caught:
                    warnings.simplefilter("always")
                    dh = ref_dc.get_dh_series(ns, mask=mask)
                    texts[f"{H}x{W}_{dtype}_{variant}"] = [str(w.message) for w in caught]
                    dv = ref_dc.get_dv_series(ns, mask=mask, nans_ok=True)
                    cum_dh = ref_dc.get_cumulative_series(ns, kind="dh", mask=mask, nans_ok=True)
                    cum_dv = ref_dc.get_cumulative_series(ns, kind="dv", mask=mask, nans_ok=True)
                dc.series_columns(f"{H}x{W}_{dtype}_{variant}", dh, dv, cum_dh, cum_dv, rec)
                print(H, W, dtype, variant, "dh", dh["dh"].values, "warnings", len(texts[f"{H}x{W}_{dtype}_{variant}"]))

    # the constructor
    for name, (years, reference) in CTOR_CASES.items():
        dems = [StandInDEM(i) for i in range(len(years))]
        obj = ref_dc.__new__(ref_dc)
        ref_dc.__init__(obj, dems, timestamps=dc.stamps(years), outlines=None,
                        reference_dem=dems[int(reference.split(":")[1])] if isinstance(reference, str) else reference)
        rec[f"ctor_{name}_index"] = np.array(obj.reference_index, dtype=np.int64)
        rec[f"ctor_{name}_timestamps"] = obj.timestamps.astype(np.int64)
        rec[f"ctor_{name}_reference_timestamp"] = np.array(ref_dc.reference_timestamp.fget(obj).astype(np.int64))
        rec[f"ctor_{name}_order"] = np.array([d.tag for d in obj.dems], dtype=np.int64)
        assert ref_dc.reference_dem.fget(obj) is obj.dems[obj.reference_index] and obj.ddems == [] and obj.outlines == {}
        print("ctor", name, "index", obj.reference_index, "reference_timestamp", ref_dc.reference_timestamp.fget(obj))

    # the messages
    raster = types.SimpleNamespace(data=np.zeros((3, 4), np.float32), transform=dc.TRANSFORM, crs=None, nodata=None)
    one = ref_ddem(raster, start_time=stamps[0], end_time=stamps[1])
    other = ref_ddem(types.SimpleNamespace(data=np.zeros((3, 4), np.float32)), start_time=stamps[0], end_time=stamps[1])
    ns = collection_of([one], stamps[1])
    dems = [StandInDEM(0), StandInDEM(1)]

    def construct(**kw):
        ref_dc.__init__(ref_dc.__new__(ref_dc), dems, **kw)

    def set_filled():
        one.filled_data = np.zeros(5)

    messages = {
        "no_timestamps": message_of(lambda: construct()),
        "bad_outlines": message_of(lambda: construct(timestamps=dc.stamps((2000, 2010)), outlines={dc.stamps((2000,))[0]: 3})),
        "not_calculated": message_of(lambda: ref_dc.get_dh_series(collection_of([], stamps[1]))),
        "foreign_ddem": message_of(lambda: ref_dc.get_ddem_mask(ns, other)),
        "bad_kind": message_of(lambda: ref_dc.get_cumulative_series(ns, kind="dz")),
        "filled_size": message_of(set_filled),
        "bad_method": message_of(lambda: one.interpolate(method="linear")),
        "reference_shape": message_of(lambda: one.interpolate(method="regional_hypsometric", reference_elevation=np.zeros((2, 2)), mask=np.ones((3, 4), bool))),
    }
    for k, v in messages.items():
        print(k, "->", v)

    out = os.path.join(GOLDEN, "demcollection_golden.npz")
    np.savez_compressed(out, **rec)
    print(out, os.path.getsize(out), "bytes")
    signatures = {f"dDEM.{m}": signature_of(getattr(ref_ddem, m)) for m in ("__init__", "copy", "from_array", "interpolate")}
    signatures.update({f"DEMCollection.{m}": signature_of(getattr(ref_dc, m)) for m in (
        "__init__", "subtract_dems", "interpolate_ddems", "get_ddem_mask", "get_dh_series", "get_dv_series", "get_cumulative_series")})
    properties = {"dDEM": sorted(k for k, v in vars(ref_ddem).items() if isinstance(v, property)),
                  "DEMCollection": sorted(k for k, v in vars(ref_dc).items() if isinstance(v, property))}
    with open(os.path.join(GOLDEN, "signatures_ddem.json"), "w") as f:
        json.dump({"signatures": signatures, "properties": properties, "messages": messages, "warnings": texts}, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
