"""Host-side fitting helpers of the bias corrections -- what ``xdem.coreg.base.fit_workflows`` needs of ``xdem/fit.py``:
the 1-D models (``sumsin_1d``, ``polynomial_1d``; ``polynomial_2d`` is Deramp's), the cost functions, and the two robust fits
that choose their own order / number of frequencies.  Everything here works on the few thousand values of a binned table or of
a subsample and stays on the host; the same SciPy / scikit-learn calls are made in the same order as upstream makes them, so the
results are the installed libraries' results.  ``subsample != 1`` draws through ``xdem_amd._coregbase.subsample_ranks`` (geoutils'
``subsample_array`` restated: parity unpinned, as everywhere in this package)."""
from __future__ import annotations

import inspect
import logging
import warnings
from typing import Any, Callable

import numpy as np
import scipy.optimize
from numpy.polynomial.polynomial import polyval

from ._coregbase import subsample_ranks
from .biascorr import polynomial_2d  # noqa: F401  (xdem/fit.py:127-149 lives next to Deramp here)


# ---- cost functions (xdem/fit.py:42-79) -----------------------------------------------------------------------------------------
def rmse(ytrue, ypred) -> float:
    """Root mean square error, NaN-skipping."""
    return np.sqrt(np.nanmean(np.square(ytrue - ypred)))


def huber_loss(ytrue, ypred) -> float:
    """Huber cost: quadratic up to a residual of 1, ``2 sqrt(z) - 1`` beyond."""
    z = ytrue - ypred
    big = z > 1
    return np.where(big, 2 * np.sqrt(z[np.where(big)]) - 1, np.square(z)).sum()


def soft_loss(ytrue, ypred, scale: float = 0.5) -> float:
    """Soft-L1 cost ``sum 2 s^2 (sqrt(1 + (z / s)^2) - 1)``."""
    return np.sum(np.square(scale) * 2 * (np.sqrt(1 + np.square((ytrue - ypred) / scale)) - 1))


# ---- the 1-D models (xdem/fit.py:87-124) ----------------------------------------------------------------------------------------
def sumsin_1d(xx, *params):
    """Sum of N sinusoids ``sum_k a_k sin(2 pi / b_k x + c_k)``; ``params`` = (a_0, b_0, c_0, a_1, ...): amplitude (Y unit),
    wavelength (X unit), phase (radians).  ``xx`` may be a 1-tuple of an array, as the corrections pass it."""
    xx = np.array(xx).squeeze()
    p = np.array(params).copy()
    amp, wave, phase = (np.arange(s, len(p), 3) for s in (0, 1, 2))
    # the parameters on axis 0, the data's axes behind it
    p = np.moveaxis(np.array(p, ndmin=xx.ndim + 1), source=xx.ndim, destination=0)
    return np.sum(p[amp, :] * np.sin(2 * np.pi / p[wave, :] * np.expand_dims(xx, axis=0) + p[phase, :]), axis=0)


def polynomial_1d(xx, *params):
    """N-order 1-D polynomial ``np.polynomial.polynomial.polyval(xx, params)``."""
    return polyval(x=xx, c=params)


# ---- choosing an order (xdem/fit.py:157-186) ----------------------------------------------------------------------------------
def _choice_best_order(cost: np.ndarray, margin_improvement: float = 20.0) -> int:
    """Index of the lowest order whose cost is within ``margin_improvement`` percent of the minimal cost (and not above the
    order of that minimum): higher orders overfit, so the first one after which the gain is negligible is kept."""
    ind_min = cost.argmin()
    min_cost = cost[ind_min]
    gain = (cost - min_cost) / min_cost
    good = np.logical_and(gain < margin_improvement / 100.0, np.arange(len(cost)) <= ind_min)
    ind = next(i for i, ok in enumerate(good) if ok)
    logging.debug("Order %d has the minimum cost value of %s", ind_min + 1, min_cost)
    logging.debug("Order %d is selected as its cost is within a %s%% margin of the minimum cost", ind + 1, margin_improvement)
    return ind


def _split_kwargs(kwargs: dict, accepted: list) -> dict:
    """The keyword arguments a callee accepts; the others are reported once, as upstream does."""
    rest = [k for k in kwargs if k not in accepted]
    if rest:
        warnings.warn("Keyword arguments: " + ",".join(rest) + " were not used.")
    return {k: kwargs[k] for k in accepted if k in kwargs}


def _wrapper_scipy_leastsquares(f: Callable[..., Any], xdata, ydata, sigma=None, p0=None, **kwargs: Any):
    """``scipy.optimize.curve_fit`` with the keywords it (or ``least_squares`` behind it) takes; returns (cost, coefficients
    rounded to 5 decimals).  The cost follows the ``loss`` passed down (xdem/fit.py:189-252)."""
    code_cf, code_ls = scipy.optimize.curve_fit.__code__, scipy.optimize.least_squares.__code__
    accepted = list(code_cf.co_varnames[: code_cf.co_argcount]) + list(code_ls.co_varnames[: code_ls.co_argcount])
    passed = _split_kwargs(kwargs, accepted)
    coefs = scipy.optimize.curve_fit(f=f, xdata=xdata, ydata=ydata, p0=p0, sigma=sigma, absolute_sigma=True, **passed)[0]
    coefs = np.array([np.round(c, 5) for c in coefs])
    if "loss" in kwargs:
        from scipy.optimize._lsq.least_squares import construct_loss_function

        loss_func = construct_loss_function(m=ydata.size, loss=kwargs["loss"], f_scale=kwargs.get("f_scale", 1.0))
        cost = 0.5 * sum(np.atleast_1d(loss_func((f(xdata, *coefs) - ydata) ** 2, cost_only=True)))
    else:
        cost = 0.5 * sum((f(xdata, *coefs) - ydata) ** 2)
    return cost, coefs


def _wrapper_sklearn_robustlinear(model, cost_func, xdata, ydata, sigma=None, estimator_name: str = "Linear", **kwargs: Any):
    """A scikit-learn linear estimator behind ``model`` (polynomial features) in a pipeline; returns (cost, coefficients)
    (xdem/fit.py:255-344)."""
    from sklearn.linear_model import HuberRegressor, LinearRegression, RANSACRegressor, TheilSenRegressor
    from sklearn.pipeline import make_pipeline

    est = {"Linear": LinearRegression, "Theil-Sen": TheilSenRegressor, "RANSAC": RANSACRegressor, "Huber": HuberRegressor}[estimator_name]
    passed = _split_kwargs(kwargs, list(inspect.signature(est.__init__).parameters.keys()))
    init_estimator = est(**passed)
    pipeline = make_pipeline(model, init_estimator)
    if sigma is not None and "sample_weight" in inspect.signature(est.fit).parameters.keys():
        # (upstream hands the weights over as positional arguments of Pipeline.fit -- reproduced)
        args = {est.__name__.lower() + "__sample_weight": 1 / sigma**2}
        pipeline.fit(xdata.reshape(-1, 1), ydata, *args)
    else:
        pipeline.fit(xdata.reshape(-1, 1), ydata)
    cost = cost_func(ydata, pipeline.predict(xdata.reshape(-1, 1)))
    coefs = init_estimator.estimator_.coef_ if estimator_name == "RANSAC" else init_estimator.coef_
    return cost, coefs


def _drop_fixed(kwargs: dict) -> None:
    for k in ("f", "absolute_sigma"):   # (both are fixed by the workflows)
        kwargs.pop(k, None)


# ---- robust polynomial fit (xdem/fit.py:347-448) --------------------------------------------------------------------------------
def robust_norder_polynomial_fit(xdata, ydata, sigma=None, max_order: int = 6, estimator_name: str = "Huber",
                                 cost_func: Callable[..., float] = soft_loss, margin_improvement: float = 20.0, subsample: float | int = 1,
                                 linear_pkg: str = "scipy", random_state=None, **kwargs: Any):
    """Robust polynomial fit of 1-D data; the order (1 .. ``max_order``) is chosen by comparing the costs of all orders with a
    margin of improvement.  Returns (coefficients in increasing power, order).  Other keywords go down to
    ``scipy.optimize.least_squares`` / the scikit-learn estimator."""
    _drop_fixed(kwargs)
    if not isinstance(estimator_name, str) or estimator_name not in ["Linear", "Theil-Sen", "RANSAC", "Huber"]:
        raise ValueError('Attribute `estimator` must be one of "Linear", "Theil-Sen", "RANSAC" or "Huber".')
    if not isinstance(linear_pkg, str) or linear_pkg not in ["sklearn", "scipy"]:
        raise ValueError('Attribute `linear_pkg` must be one of "scipy" or "sklearn".')
    if len(xdata) == 1:
        xdata = xdata[0]
    keep = np.logical_and(np.isfinite(ydata), np.isfinite(xdata))
    x, y = xdata[keep], ydata[keep]
    if subsample != 1:
        pick = subsample_ranks(x.size, subsample, random_state)
        x, y = x[pick], y[pick]
    costs = np.empty(max_order)
    coeffs = np.zeros((max_order, max_order + 1))
    for deg in np.arange(1, max_order + 1):
        if estimator_name == "Linear" and linear_pkg == "scipy":
            p0 = np.polyfit(x, y, deg)
            try:
                cost, coef = _wrapper_scipy_leastsquares(f=polynomial_1d, xdata=x, ydata=y, p0=p0, sigma=sigma, **kwargs)
            except RuntimeError:
                cost, coef = np.inf, np.full(len(p0), np.nan)
        else:
            from sklearn.preprocessing import PolynomialFeatures

            cost, coef = _wrapper_sklearn_robustlinear(PolynomialFeatures(degree=deg), estimator_name=estimator_name, cost_func=cost_func,
                                                       xdata=x, ydata=y, sigma=sigma, **kwargs)
        costs[deg - 1] = cost
        coeffs[deg - 1, 0:coef.size] = coef
    best = _choice_best_order(cost=costs, margin_improvement=margin_improvement)
    return np.trim_zeros(coeffs[best], "b"), best + 1


# ---- robust sum-of-sinusoids fit (xdem/fit.py:451-627) --------------------------------------------------------------------------
def _cost_sumofsin(x, y, cost_func, *p) -> float:
    return cost_func(y, sumsin_1d(x, *p))


def robust_nfreq_sumsin_fit(xdata, ydata, sigma=None, max_nb_frequency: int = 3, bounds_amp_wave_phase=None,
                            cost_func: Callable[..., float] = soft_loss, subsample: float | int = 1, hop_length: float | None = None,
                            random_state=None, **kwargs: Any):
    """Robust fit of a sum of sinusoids to 1-D data by ``scipy.optimize.basinhopping``, for 1 .. ``max_nb_frequency`` frequencies;
    the number kept is chosen on the costs with a margin of improvement, a frequency of negligible amplitude is dropped and the
    rest ordered by amplitude.  Returns ((a, b, c) x N flattened, N).  Other keywords go to ``basinhopping``."""
    _drop_fixed(kwargs)
    if len(xdata) == 1:
        xdata = xdata[0]
    if "niter_success" not in kwargs:
        kwargs.update({"niter_success": min(40, kwargs["niter"]) if "niter" in kwargs else 40})

    def cost_of(p, x, y) -> float:
        return _cost_sumofsin(x, y, cost_func, *p)

    x_res = np.mean(np.diff(np.sort(xdata)))   # the resolution of the sampled coordinate
    hop = float(np.percentile(ydata, 90) - np.percentile(ydata, 10)) if hop_length is None else hop_length
    costs = np.empty(max_nb_frequency)
    found = np.zeros((max_nb_frequency, 3 * max_nb_frequency)) * np.nan
    for nb_freq in np.arange(1, max_nb_frequency + 1):
        logging.info("Fitting with %d frequency", nb_freq)
        b = bounds_amp_wave_phase
        if b is None:   # the widest bounds the data allow; the wavelength stays off zero
            one = [(0, ydata.max() - ydata.min()), (x_res / 5, xdata.max() - xdata.min()), (0, 2 * np.pi)]
            b = []
            for _ in range(nb_freq):
                b += one
        lb = np.asarray([b[i][0] for i in range(3 * nb_freq)])
        ub = np.asarray([b[i][1] for i in range(3 * nb_freq)])
        p0 = (np.abs((lb + ub) / 2)).squeeze()
        res = scipy.optimize.basinhopping(cost_of, p0, disp=logging.getLogger().getEffectiveLevel() < logging.WARNING, T=hop,
                                          minimizer_kwargs=dict(args=(xdata, ydata), bounds=scipy.optimize.Bounds(lb, ub)),
                                          seed=random_state, **kwargs)
        best_x = np.array([np.round(v, 5) for v in res.lowest_optimization_result.x])
        costs[nb_freq - 1] = cost_of(best_x, xdata, ydata)
        found[nb_freq - 1, 0:3 * nb_freq] = best_x
    costs[np.isnan(costs)] = np.inf
    best = _choice_best_order(cost=costs)
    coefs = found[best][~np.isnan(found[best])]
    degree = best + 1
    # one frequency whose amplitude is below 0.1 % of the signal's 10-90 percentile range goes (at least one frequency stays)
    for i in range(best + 1):
        if np.abs(coefs[3 * i]) < (np.nanpercentile(ydata, 90) - np.nanpercentile(ydata, 10)) / 1000 and len(coefs) > 3:
            coefs = np.delete(coefs, slice(3 * i, 3 * i + 3))
            degree -= 1
            break
    order = np.flip(np.argsort(coefs[0::3]))
    amp, wave, phase = coefs[0::3][order], coefs[1::3][order], coefs[2::3][order]
    return np.array([(amp[i], wave[i], phase[i]) for i in range(degree)]).flatten(), degree


fit_workflows = {
    "norder_polynomial": {"func": polynomial_1d, "optimizer": robust_norder_polynomial_fit},
    "nfreq_sumsin": {"func": sumsin_1d, "optimizer": robust_nfreq_sumsin_fit},
}
