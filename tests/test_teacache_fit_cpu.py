"""TeaCache calibration, host side (chronoedit_amd/teacache.py): the least-squares fit of the rescaling polynomial from the (ratio, distance)
points of measured edits - which points it uses, the degree it falls back to, and the coefficient order the plan takes.  No GPU."""
import math

import numpy as np
import pytest

from chronoedit_amd.teacache import TeaCacheCalibration, fit_calibration, fit_coefficients, plan_from_ratios

QUARTIC = (3.0, -7.5, 6.25, -1.5, 0.125)  # highest power first


def _points(n=12, lo=0.6, hi=1.1):
    x = np.linspace(lo, hi, n)
    return x, np.polyval(QUARTIC, x)


def test_a_known_quartic_is_recovered_at_the_points():
    """Predictions, not coefficients: the Vandermonde matrix of degree 4 on [0.6, 1.1] is ill-conditioned."""
    x, y = _points()
    ratios, distances = [0.0] + list(x), [math.nan] + list(y)  # entry 0 is the step without a predecessor
    coef = fit_coefficients(ratios, distances, degree=4)
    assert isinstance(coef, tuple) and len(coef) == 5 and all(isinstance(c, float) for c in coef)
    got = np.polyval(coef, x)
    assert np.all(np.abs(got - y) <= 1e-9 * np.abs(y)), np.max(np.abs(got - y) / np.abs(y))
    cal = fit_calibration(ratios, distances, degree=4)
    assert isinstance(cal, TeaCacheCalibration) and cal.coefficients == coef and cal.degree == 4
    assert cal.points == tuple(zip(x.tolist(), y.tolist()))
    assert 0.0 <= cal.rms_residual <= cal.max_residual <= 1e-9 * float(np.abs(y).max())
    with pytest.raises(Exception):  # frozen
        cal.degree = 3


def test_entry_zero_and_non_finite_points_are_ignored_and_edits_are_pooled():
    x, y = _points()
    clean = fit_coefficients([0.0] + list(x), [0.0] + list(y))
    # entry 0 carries garbage that would wreck the fit; so do a NaN and an infinite distance and a NaN ratio further in
    r1 = [0.9, *x[:6], 0.7, 0.8, math.nan]
    d1 = [1e6, *y[:6], math.nan, math.inf, 5.0]
    r2 = [0.3, *x[6:]]
    d2 = [-1e6, *y[6:]]
    cal = fit_calibration([r1, r2], [d1, d2])
    assert len(cal.points) == 12 and cal.points == tuple(zip(x.tolist(), y.tolist()))
    assert np.allclose(np.polyval(cal.coefficients, x), np.polyval(clean, x), rtol=1e-9, atol=0)
    assert fit_calibration([r1[:4]], [d1[:4]]).degree == 2  # (a list of ONE edit; its three usable points cannot carry a quartic)


def test_too_few_distinct_ratios_lower_the_degree():
    r = [0.0, 0.5, 0.7, 0.9, 0.5, 0.7, 0.9]
    d = [0.0, 0.10, 0.21, 0.40, 0.12, 0.19, 0.40]
    cal = fit_calibration(r, d, degree=4)
    assert cal.degree == 2 and len(cal.coefficients) == 3
    want = np.polyfit(np.array(r[1:]), np.array(d[1:]), 2)
    assert np.allclose(cal.coefficients, want, rtol=1e-12, atol=0)
    # one distinct ratio: a constant
    cal = fit_calibration([0.0, 0.5, 0.5], [0.0, 0.2, 0.4])
    assert cal.degree == 0 and cal.coefficients == (pytest.approx(0.3),)


def test_fewer_than_two_usable_points_raise():
    with pytest.raises(ValueError, match="usable"):
        fit_coefficients([0.0, 0.5], [math.nan, 0.2])
    with pytest.raises(ValueError, match="usable"):
        fit_coefficients([0.0, 0.5, 0.6, 0.7], [0.1, 0.2, math.nan, math.inf])
    with pytest.raises(ValueError, match="usable"):
        fit_coefficients([[0.0], [0.0, 0.4]], [[1.0], [1.0, 0.3]])


def test_coefficients_feed_the_plan_highest_power_first():
    x, y = _points()
    ratios = [0.0] + list(x)
    coef = fit_coefficients(ratios, [math.nan] + list(y))
    n, thresh = len(ratios), 0.35
    want, acc = [], 0.0
    for i in range(n):  # the rule of plan_from_ratios by hand, with np.polyval (highest power first)
        compute = i == 0 or i == n - 1
        if not compute:
            acc += float(np.polyval(np.asarray(coef), ratios[i]))
            compute = not acc < thresh
        if compute:
            acc = 0.0
        want.append(compute)
    assert want.count(False) >= 2 and want.count(True) >= 4, want  # both kinds of step occur away from the ends
    assert plan_from_ratios(ratios, n, thresh, coef) == want
    assert plan_from_ratios(ratios, n, thresh, coef[::-1]) != want  # the order matters for this polynomial
