"""xdem_amd/fit.py without the GPU: the 1-D models against NumPy expressions, the cost functions, the choice of an order, and the
two robust fits against what the reference's own functions returned on the same binned tables with the same seed
(tests/golden/bincorr_golden.npz, written by tools/gen_golden_bincorr.py).  The restatement makes the same SciPy / scikit-learn
calls in the same order, so equality is the bar."""
import os
import warnings

import numpy as np
import pytest

from conftest import GOLDEN


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "bincorr_golden.npz"))


def test_sumsin_1d_is_the_sum_of_sinusoids():
    from xdem_amd import fit

    x = np.linspace(-3.0, 40.0, 57)
    p = (2.0, 11.0, 0.3, 0.5, 4.0, 1.7, 0.1, 90.0, 5.0)
    want = sum(p[i] * np.sin(2 * np.pi / p[i + 1] * x + p[i + 2]) for i in (0, 3, 6))
    assert np.allclose(fit.sumsin_1d(x, *p), want, rtol=0, atol=1e-15 * 3)
    one = fit.sumsin_1d(x, *p[:3])
    assert np.array_equal(one, p[0] * np.sin(2 * np.pi / p[1] * x + p[2]))
    # a 1-tuple of a 2-D array, as the corrections pass it: squeezed to the array's shape
    x2 = x[:56].reshape(7, 8)
    assert np.array_equal(fit.sumsin_1d((x2,), *p[:3]), p[0] * np.sin(2 * np.pi / p[1] * x2 + p[2]))


def test_polynomial_1d_is_polyval():
    from xdem_amd import fit

    x = np.linspace(-2.0, 3.0, 31)
    c = (1.5, -0.25, 0.125, 3.0)
    assert np.array_equal(fit.polynomial_1d(x, *c), np.polynomial.polynomial.polyval(x, c))
    assert np.allclose(fit.polynomial_1d(x, *c), c[0] + c[1] * x + c[2] * x**2 + c[3] * x**3, rtol=1e-14)
    assert fit.polynomial_1d((x.reshape(1, 31),), *c).shape == (1, 1, 31)   # (the reference's (1, H, W) for a tuple of one plane)


def test_polynomial_2d_is_the_one_of_deramp():
    from xdem_amd import biascorr, fit

    assert fit.polynomial_2d is biascorr.polynomial_2d


def test_cost_functions():
    from xdem_amd import fit

    y = np.array([0.0, 1.0, 4.0, np.nan])
    p = np.array([0.5, 1.0, 1.0, 2.0])
    assert fit.rmse(y, p) == np.sqrt(np.nanmean((y - p) ** 2))
    z = np.array([3.0, 0.5, -2.0])
    assert fit.huber_loss(z, np.zeros(3)) == (2 * np.sqrt(3.0) - 1) + 0.25 + 4.0
    assert fit.soft_loss(z, np.zeros(3)) == np.sum(0.25 * 2 * (np.sqrt(1 + (z / 0.5) ** 2) - 1))
    assert fit.soft_loss(z, np.zeros(3), scale=2.0) == np.sum(4.0 * 2 * (np.sqrt(1 + (z / 2.0) ** 2) - 1))


def test_choice_best_order_keeps_the_lowest_order_within_the_margin():
    from xdem_amd import fit

    assert fit._choice_best_order(np.array([10.0, 5.5, 5.0, 5.2])) == 1          # 5.5 is within 20 % of 5.0
    assert fit._choice_best_order(np.array([10.0, 7.0, 5.0, 4.9])) == 2          # 5.0 within 20 % of 4.9, 7.0 not
    assert fit._choice_best_order(np.array([10.0, 7.0, 5.0, 4.9]), margin_improvement=1.0) == 3
    assert fit._choice_best_order(np.array([1.0, 2.0, 3.0])) == 0
    assert fit._choice_best_order(np.array([5.0, 1.0, 1.1])) == 1                 # nothing above the minimum's order is kept


def test_workflows_name_the_restated_functions():
    from xdem_amd import fit

    assert fit.fit_workflows == {"norder_polynomial": {"func": fit.polynomial_1d, "optimizer": fit.robust_norder_polynomial_fit},
                                 "nfreq_sumsin": {"func": fit.sumsin_1d, "optimizer": fit.robust_nfreq_sumsin_fit}}


def test_robust_polynomial_fit_reproduces_the_reference(golden):
    from xdem_amd import fit

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")   # (scikit-learn's convergence warnings for the high orders, as in the reference's run)
        coefs, order = fit.robust_norder_polynomial_fit(golden["poly|x"], golden["poly|y"])
    assert order == int(golden["poly|order"])
    assert np.array_equal(coefs, golden["poly|fit_params"])


def test_robust_polynomial_fit_refuses_unknown_names():
    from xdem_amd import fit

    x = np.arange(10.0)
    with pytest.raises(ValueError, match='Attribute `estimator` must be one of "Linear", "Theil-Sen", "RANSAC" or "Huber".'):
        fit.robust_norder_polynomial_fit(x, x, estimator_name="yay")
    with pytest.raises(ValueError, match='Attribute `linear_pkg` must be one of "scipy" or "sklearn".'):
        fit.robust_norder_polynomial_fit(x, x, linear_pkg="yay")


def test_robust_polynomial_fit_linear_scipy_route_finds_the_polynomial():
    from xdem_amd import fit

    x = np.linspace(1.0, 10.0, 60)
    y = 2.0 - 0.5 * x + 0.25 * x**2
    coefs, order = fit.robust_norder_polynomial_fit(x, y, estimator_name="Linear", linear_pkg="scipy")
    assert order == 2 and np.allclose(coefs, [2.0, -0.5, 0.25], atol=2e-5)   # (coefficients are rounded to 5 decimals)


def test_robust_sumsin_fit_reproduces_the_reference(golden):
    from xdem_amd import fit

    coefs, n_freq = fit.robust_nfreq_sumsin_fit(golden["sumsin|x"], golden["sumsin|y"], random_state=42, niter=3)
    assert n_freq == int(golden["sumsin|order"])
    assert np.array_equal(coefs, golden["sumsin|fit_params"])
