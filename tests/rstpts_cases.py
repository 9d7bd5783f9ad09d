"""Shapes and measured figures of the raster-point tests (shared by tools/gen_golden_rstpts.py and the tests)."""

SHAPES = ((61, 83, 700), (96, 128, 3000))   # (H, W, points) of xdem_amd.synth.cloud_case

# Largest deviation of a whole fit's final offsets from the recorded reference run (tests/golden/rstpts_golden_*.npz), in PIXELS for the
# horizontal offsets of NuthKaab (the unit of its stopping threshold, 1e-3 pixel) and in metres for the vertical one.  "cpu": the
# product's host code over tests/rstpts_oracle.py -- p0 is NumPy's nanmean / nanstd of y as in the reference, the runs coincide; "mi355x":
# over the device plan -- float32 coincides too, float64 differs through the last bit of the device's arctangent (the aspect decides the
# bins).  The bar of the tests is 4 x the larger.
MEASURED = {"cpu": {"nk_horizontal_px": 0.0, "nk_vertical": 0.0}, "mi355x": {"nk_horizontal_px": 5.467e-7, "nk_vertical": 1.608e-7}}


def _bar(key: str) -> float:
    return 4 * max(v[key] for v in MEASURED.values())


NK_BAR_PX, NK_BAR_Z = _bar("nk_horizontal_px"), _bar("nk_vertical")
