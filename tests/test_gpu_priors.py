"""GPU: nmc_prior_logpdf (csrc/special.h) through nmc_debug_prior_logpdf -- the function step.h
calls at every Metropolis decision under none or complete pooling -- over the grid of
tests/prior_ref.py: nine families x five (loc, scale) x their shapes x about 320 y (640 where
the support has both signs), support edges with loc != 0, overflowing and denormal y.

1. NaN / -inf / +inf fall where scipy's (as installed: the parity contract) fall, and the
   support edges have scipy's values: gamma at y = 0 (+inf for a < 1, -gammaln(a) - log(scale)
   for a = 1, -inf for a > 1), uniform at both closed ends and -inf one ulp outside, halfnorm
   and expon at -0.0, lognorm and invgamma at 0.
2. Finite values are within 4 x prior_ref.SCIPY_WORST[family] units of 2^-53 max(A, 1) of the
   mpmath reference: four times what scipy's own float64 logpdf shows on the same grid.
3. Laplace beyond |y| = 700 follows prior_ref.check_finite's tail rule.
4. Cauchy follows scipy's two-branch form: finite at y = 1e155 and 1e300, where the one-branch
   form -log(pi) - log1p(y^2) gives -inf from |y| = 2^512 on.

Device figures measured per family: DESIGN 3.7.
"""

import numpy
import pytest
import scipy.stats

import prior_ref as pr
from nestmc import _lib, priors

pytestmark = pytest.mark.gpu


def _device(lib, fam, prm, x):
    x = numpy.ascontiguousarray(x, dtype=numpy.float64)
    prm = numpy.ascontiguousarray(prm, dtype=numpy.float64)
    out = numpy.full(len(x), -12345.0)
    assert lib.nmc_debug_prior_logpdf(int(fam), _lib.dptr(prm), _lib.dptr(x), len(x),
                                      _lib.dptr(out)) == 0
    return out


def _combo(lib, c):
    fam, prm = pr.params(*c)
    return _device(lib, fam, prm, pr.grid_x(c[0], c[1], c[2]))


@pytest.mark.parametrize("name", pr.FAMILIES)
def test_family_over_the_grid(gpu_lib, name):
    worst, at = 0.0, None
    for c in [c for c in pr.combos() if c[0] == name]:
        got = _combo(gpu_lib, c)
        pr.check_classification(got, *c)
        w = pr.check_finite(got, *c)
        if w > worst:
            worst, at = w, c
    bound = pr.DEVICE_FACTOR * pr.SCIPY_WORST[name]
    print("nmc_prior_logpdf %s: worst %.2f units at %s; scipy's own %.2f, bound %.2f"
          % (name, worst, at, pr.SCIPY_WORST[name], bound))
    assert worst <= bound, (name, worst, at, bound)


def _at(lib, dist, x):
    fam, prm = priors.encode(dist)
    x = numpy.atleast_1d(numpy.asarray(x, dtype=numpy.float64))
    got = _device(lib, fam, prm, x)
    with numpy.errstate(all="ignore"):
        return got, numpy.asarray(dist.logpdf(x), dtype=numpy.float64)


@pytest.mark.parametrize("loc,scale", [ls for ls in pr.LOC_SCALE if ls[0] != 0.0])
def test_support_edges_with_loc(gpu_lib, loc, scale):
    """The x whose y = (x - loc) / scale lands on 0 or 1, and the nearest x on either side whose
    y is another.  y == 0 is x == loc for every (loc, scale); y == 1 is met exactly at (-1, 2)
    and (100, 10), while at (0.3, 1e-3) the spacing of x steps y by 5e-14 and may pass over 1:
    prior_ref.edge_x then gives the nearest x, and the uniform check below takes each of the
    three upper points by its own y, closed at 1."""
    ls = float(numpy.log(scale))
    lo = pr.edge_x(loc, scale, 0.0)                 # below, y == 0, above
    hi = pr.edge_x(loc, scale, 1.0)
    assert (lo[1] - loc) / scale == 0.0
    # gamma at y = 0
    for a, want in ((0.5, numpy.inf), (1.0, 0.0 - ls), (2.0, -numpy.inf), (10.0, -numpy.inf)):
        got, sp = _at(gpu_lib, scipy.stats.gamma(a, loc=loc, scale=scale), lo)
        assert got[0] == -numpy.inf and got[1] == want and numpy.isfinite(got[2]), (a, got)
        assert sp[1] == want and numpy.array_equal(numpy.isfinite(got), numpy.isfinite(sp))
    # uniform: both closed ends, -inf one ulp outside
    got, sp = _at(gpu_lib, scipy.stats.uniform(loc=loc, scale=scale), numpy.concatenate([lo, hi]))
    yhi = (hi - loc) / scale
    assert got[0] == -numpy.inf and got[1] == 0.0 - ls and got[2] == 0.0 - ls
    for i in range(3):
        assert got[3 + i] == (0.0 - ls if yhi[i] <= 1.0 else -numpy.inf), (i, yhi, got)
    assert yhi[2] > 1.0 and got[5] == -numpy.inf
    assert numpy.array_equal(got, sp)
    # halfnorm and expon: closed at 0; lognorm and invgamma: open
    for d, closed in ((scipy.stats.halfnorm(loc=loc, scale=scale), True),
                      (scipy.stats.expon(loc=loc, scale=scale), True),
                      (scipy.stats.lognorm(0.7, loc=loc, scale=scale), False),
                      (scipy.stats.invgamma(3.0, loc=loc, scale=scale), False)):
        got, sp = _at(gpu_lib, d, lo)
        assert got[0] == -numpy.inf and numpy.isfinite(got[2]), (d.dist.name, got)
        assert numpy.isfinite(got[1]) == closed and (closed or got[1] == -numpy.inf)
        assert numpy.array_equal(numpy.isfinite(got), numpy.isfinite(sp)), (d.dist.name, got, sp)
        if closed:
            assert abs(got[1] - sp[1]) <= 2.0 ** -52 * max(1.0, abs(sp[1])), (d.dist.name, got, sp)


def test_minus_zero_is_inside_the_closed_supports(gpu_lib):
    x = numpy.array([-0.0, 0.0])
    for d in (scipy.stats.halfnorm(), scipy.stats.expon(), scipy.stats.halfnorm(scale=3.0),
              scipy.stats.expon(scale=0.5), scipy.stats.uniform(), scipy.stats.gamma(1.0)):
        got, sp = _at(gpu_lib, d, x)
        assert numpy.all(numpy.isfinite(got)) and got[0] == got[1], (d.dist.name, got)
        assert numpy.allclose(got, sp, rtol=2.0 ** -52, atol=0), (d.dist.name, got, sp)
    for d in (scipy.stats.lognorm(0.7), scipy.stats.invgamma(3.0), scipy.stats.gamma(2.0)):
        got, sp = _at(gpu_lib, d, x)
        assert numpy.all(got == -numpy.inf) and numpy.all(sp == -numpy.inf), (d.dist.name, got)


def test_bad_parameters_give_nan(gpu_lib):
    x = numpy.array([-1.0, 0.0, 0.5, 1.0, 3.0, numpy.inf, numpy.nan])
    for name in pr.FAMILIES:
        shape = pr.SHAPES.get(name, (None,))[0]
        for scale in (0.0, -1.0, numpy.nan):
            fam, prm = pr.params(name, 0.5, scale, shape)
            got = _device(gpu_lib, fam, prm, x)
            assert numpy.all(numpy.isnan(got)), (name, scale, got)
            with numpy.errstate(all="ignore"):
                assert numpy.all(numpy.isnan(pr.frozen(name, 0.5, scale, shape).logpdf(x)))
        if shape is not None:
            fam, prm = pr.params(name, 0.0, 1.0, numpy.nan)
            got = _device(gpu_lib, fam, prm, x)
            with numpy.errstate(all="ignore"):
                sp = pr.frozen(name, 0.0, 1.0, numpy.nan).logpdf(x)
            assert numpy.all(numpy.isnan(sp))
            assert numpy.all(numpy.isnan(got)), (name, "nan shape", got)
    prm = numpy.array([0.0, 1.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0])
    for fam in (-1, 9, 1000):
        assert numpy.all(numpy.isnan(_device(gpu_lib, fam, prm, x))), fam


def test_cauchy_beyond_the_overflow_of_y_squared(gpu_lib):
    """y * y overflows from |y| = 2^512 on; scipy's second branch, 2 log|y| + log1p(1 / y^2), does
    not, and neither may the device."""
    edge = pr.CAUCHY_OVERFLOW
    d = scipy.stats.cauchy(1, 2)
    x = numpy.array([1e155, 1e300, -1e155, -1e300, 2.0 * edge, -2.0 * edge, 1.7e308,
                     2.0 * numpy.nextafter(edge, 0.0), 1e150, 3.0, 1.0, -1.0, 1.0 + 2.0 ** -40])
    got, sp = _at(gpu_lib, d, x)
    assert abs(sp[0] - -714.2529615334436) < 1e-12
    assert numpy.all(numpy.isfinite(got)), got
    # both are within their own figure of the exact value (A is about |value| out here): the
    # device's 4 x and scipy's 1 x prior_ref.SCIPY_WORST units of 2^-53 |value|
    assert numpy.allclose(got, sp, rtol=5 * pr.SCIPY_WORST["cauchy"] * 2.0 ** -53, atol=0), (got, sp)
