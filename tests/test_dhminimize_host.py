"""Host-side contract of ``xdem_amd.coreg.DhMinimize`` (no GPU): the reference's signatures (tests/golden/signatures_dhminimize.json,
written by tools/gen_golden_dhminimize.py), the constructor's meta, the errors shared with the other steps, and the self-consistency of
the recorded trajectories: SciPy over the oracle, run again on the recorded inputs, evaluates the recorded points."""
import inspect
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN

SIG = json.load(open(os.path.join(GOLDEN, "signatures_dhminimize.json")))["coreg"]


@pytest.mark.parametrize("name", sorted(SIG))
def test_reference_parameters_are_mirrored(name):
    from xdem_amd import coreg

    cls, meth = name.split(".")
    mine = list(inspect.signature(getattr(getattr(coreg, cls), meth)).parameters.items())
    names = [n for n, _ in mine]
    catch_all = any(p.kind is inspect.Parameter.VAR_KEYWORD for _, p in mine)
    pos = -1
    for rec in SIG[name]:
        if rec["kind"] in ("VAR_KEYWORD", "VAR_POSITIONAL"):
            continue
        if rec["name"] not in names:
            assert catch_all, f"{name}: parameter '{rec['name']}' of the reference is missing"
            continue
        p = dict(mine)[rec["name"]]
        if rec["kind"] == "POSITIONAL_OR_KEYWORD" and p.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD:
            assert names.index(rec["name"]) > pos, f"{name}: '{rec['name']}' is out of the reference's order"
            pos = names.index(rec["name"])
        if rec["default"] == "<required>":
            assert p.default is inspect.Parameter.empty, f"{name}: '{rec['name']}' must stay required"
        elif rec["default"] == "<object>":
            assert p.default is not inspect.Parameter.empty
        else:
            assert p.default == rec["default"], f"{name}: default of '{rec['name']}' is {p.default!r}, reference {rec['default']!r}"
    if meth in ("__init__", "apply"):   # the reference's parameters, one for one and in its order (apply: then `resolution`, for arrays)
        ref_names = [rec["name"] for rec in SIG[name] if rec["kind"] not in ("VAR_KEYWORD", "VAR_POSITIONAL")]
        assert names[:len(ref_names)] == ref_names and names[len(ref_names):] in ([], ["resolution"])


def test_constructor_meta_and_defaults():
    import scipy.optimize
    from xdem_amd import coreg, spatialstats

    c = coreg.DhMinimize()
    assert c.meta["inputs"]["fitorbin"] == {"fit_or_bin": "fit", "fit_minimizer": scipy.optimize.minimize,
                                            "fit_loss_func": spatialstats.nmad}
    assert c.meta["inputs"]["random"] == {"subsample": 5e5, "random_state": None}
    assert "initial_shift" not in c.meta["inputs"]["affine"] and c.meta["outputs"] == {}
    assert isinstance(c, coreg._Step) and c.is_affine and c.to_rotations() == (0.0, 0.0, 0.0)
    assert coreg.DhMinimize(initial_shift=(1.0, 2)).meta["inputs"]["affine"]["initial_shift"] == (1.0, 2, 0)
    with pytest.warns(UserWarning, match="Initial shift in altitude"):
        assert coreg.DhMinimize(initial_shift=(1.0, 2.0, 3.0)).meta["inputs"]["affine"]["initial_shift"] == (1.0, 2.0, 0)
    with pytest.raises(ValueError, match="must be a tuple of exactly two or three numerical values"):
        coreg.DhMinimize(initial_shift=[1.0, 2.0])
    with pytest.raises(TypeError, match="fit_loss_func"):
        coreg.DhMinimize(fit_loss_func="nmad")
    # `+` makes a pipeline and drops the initial shift, as for NuthKaab
    pipe = coreg.DhMinimize(initial_shift=(1.0, 2.0)) + coreg.VerticalShift()
    assert isinstance(pipe, coreg.CoregPipeline) and "initial_shift" not in pipe.pipeline[0].meta["inputs"]["affine"]
    assert pipe.is_affine and not (coreg.DhMinimize() + coreg.Deramp()).is_affine
    c.meta["outputs"]["affine"] = {"shift_x": 1.5, "shift_y": -2.0, "shift_z": 0.25}
    assert c.to_translations() == (1.5, -2.0, 0.25) and np.array_equal(c.to_matrix()[:3, 3], [1.5, -2.0, 0.25])


def test_errors_are_those_of_the_other_steps():
    from xdem_amd import coreg

    z = np.zeros((10, 10), dtype=np.float32)
    with pytest.raises(NotImplementedError, match="Weights have not yet been implemented"):
        coreg.DhMinimize().fit(z, z, weights=np.ones((10, 10)), resolution=1.0)
    with pytest.raises(NotImplementedError, match="bias_vars is not used by DhMinimize"):
        coreg.DhMinimize().fit(z, z, bias_vars={"a": z}, resolution=1.0)
    with pytest.raises(ValueError, match="'transform' must be given if both DEMs are array-like"):
        coreg.DhMinimize().fit(z, z)
    # point-cloud input (coordinates and elevations as 1-D columns) is refused where the rasters are checked, as by the other steps
    pts = np.zeros(10, dtype=np.float32)
    with pytest.raises(ValueError, match="ref and tba must be 2D arrays of the same shape"):
        coreg.DhMinimize().fit(z, pts, resolution=1.0)
    with pytest.raises(ValueError, match="ref and tba must be 2D arrays of the same shape"):
        coreg.Deramp().fit(z, pts)


@pytest.mark.parametrize("case", ["f32", "f64"])
def test_recorded_trajectory_is_reproduced_by_scipy_over_the_oracle(case):
    """The fixture is self-consistent: Nelder-Mead from (1, 1) over the oracle interpolator and ``binning_oracle.nmad`` evaluates the
    recorded points with the recorded losses and ends at the recorded offsets (sign flipped, affine.py:669-672)."""
    import binning_oracle
    import nuthkaab_oracle
    import scipy.optimize

    g = np.load(os.path.join(GOLDEN, "dhminimize_golden.npz"))
    ref, tba, inlier, mask = (g[f"{case}_{k}"] for k in ("ref", "tba", "inlier", "mask"))
    assert np.array_equal(mask, inlier & np.isfinite(ref) & np.isfinite(tba))
    assert ref.dtype == {"f32": np.float32, "f64": np.float64}[case] and ref.shape == (96, 128)
    res = tuple(float(v) for v in g[f"{case}_res"])
    for rule in (0, 3):
        calls = []

        def loss(x):
            v = binning_oracle.nmad(nuthkaab_oracle.shifted_dh(ref, tba, float(x[0]), float(x[1]), res, rule)[mask])
            calls.append((float(x[0]), float(x[1]), float(v)))
            return v

        r = scipy.optimize.minimize(loss, (1, 1), method="Nelder-Mead")
        assert np.array_equal(np.array(calls), g[f"{case}_r{rule}_traj"])
        off = g[f"{case}_r{rule}_offsets"]
        assert (-r.x[0], -r.x[1]) == (off[0], off[1])
        assert float(np.nanmedian(nuthkaab_oracle.shifted_dh(ref, tba, r.x[0], r.x[1], res, rule)[mask])) == off[2]
