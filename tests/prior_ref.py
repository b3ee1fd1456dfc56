"""Inputs and the mpmath reference for nmc_prior_logpdf (csrc/special.h), the scipy frozen priors
of none and complete pooling (tests/test_prior_ref.py on the CPU, tests/test_gpu_priors.py on
the GPU through nmc_debug_prior_logpdf, which compiles the function step.h calls).

Reference.  scipy's rv_continuous.logpdf is _logpdf(y) - log(scale) with y = (x - loc) / scale
in float64; the device forms y with the same two IEEE operations, so the reference starts
from that float64 y and evaluates scipy's _logpdf formula of the family in mpmath at 200 bits,
then subtracts the float64 log(scale) and uses the float64 gammaln(shape) that
nestmc.priors.encode passes to the device.  With it comes A, the sum of the absolute values of
the formula's addends; errors are counted in units of 2^-53 max(A, 1):

  norm      -y^2/2 - log(sqrt(2 pi))                     lognorm  -log(y)^2 / (2 s^2) - log(s y sqrt(2 pi))
  gamma     (a - 1) log(y) - y - gammaln(a)              invgamma -(a + 1) log(y) - gammaln(a) - 1/y
  uniform   0            expon  -y                       halfnorm log(2/pi)/2 - y^2/2
  cauchy    -log(pi) - log(1 + y^2)                      laplace  log(1/2) - |y|

Grid, per family: (loc, scale) of LOC_SCALE, the shapes of SHAPES, and the y of y_targets():
300 seeded 10^U(-12, 3) on both signs, 1 +- 1e-9, 5e-324, 1e-300, 1e150, 1e155, 1e300, the support
edges with loc != 0 (the x for which y lands on 0 or 1, and its two float neighbours), +-inf
and NaN; x = loc + scale y in float64, and y is then recomputed from x as the device does.

scipy's own float64 logpdf (1.15.3) against this reference over this grid, worst error per
family in the units above (SCIPY_WORST, measured on the CPU by tests/test_prior_ref.py, which
keeps the figures honest); the device is allowed 4 times its family's figure -- its log, log1p
and exp are not libm's, and each contributes a few ulp of one addend:

  norm 2.50   gamma 2.38   uniform 0.00   expon 0.96   halfnorm 2.08   cauchy 1.78
  laplace 1.81 (|y| <= 700)   lognorm 4.25 (s = 0.05)   invgamma 2.51

(lognorm: where the float64 product s y sqrt(2 pi) is denormal -- y = 5e-324 -- the reference
takes the logarithm of that float64 product: see _formula.)

Laplace mirrors scipy's log(0.5 exp(-|y|)): beyond |y| = 708 that is the log of a denormal,
where one denormal ulp of exp moves the result by far more than any of these units.  The
mpmath comparison stops at |y| = 700; for 700 < |y| < 745.2 the device is compared with
scipy's float64 value within 2 spacing(e) / e, e = 0.5 exp(-|y|) in float64 (one denormal ulp on
each side), and from |y| = 746 on both give -inf (LAPLACE_Y).
"""

import functools

import mpmath
import numpy
import scipy.special
import scipy.stats

PREC = 200
U53 = 2.0 ** -53
FAMILIES = ("norm", "gamma", "uniform", "expon", "halfnorm", "cauchy", "laplace", "lognorm",
            "invgamma")
LOC_SCALE = ((0.0, 1.0), (-1.0, 2.0), (100.0, 10.0), (0.3, 1e-3), (0.0, 1e6))
SHAPES = {"gamma": (0.5, 1.0, 2.0, 10.0, 300.0), "lognorm": (0.05, 0.7, 5.0),
          "invgamma": (0.5, 3.0)}
TWO_SIDED = ("norm", "cauchy", "laplace")
# scipy's worst error per family over the grid, in units of 2^-53 max(A, 1), rounded up to the
# next 0.01 (tests/test_prior_ref.py measures it again)
SCIPY_WORST = {"norm": 2.50, "gamma": 2.38, "uniform": 0.00, "expon": 0.96, "halfnorm": 2.08,
               "cauchy": 1.78, "laplace": 1.81, "lognorm": 4.25, "invgamma": 2.51}
DEVICE_FACTOR = 4.0
LAPLACE_MP_MAX = 700.0
LAPLACE_Y = (700.5, 701.0, 705.25, 708.0, 708.5, 709.0, 710.0, 720.0, 730.0, 740.0, 744.0, 745.0,
             745.1, 746.0, 750.0, 800.0, 1e4)


def _ro(a):
    a = numpy.ascontiguousarray(a, dtype=numpy.float64)
    a.setflags(write=False)
    return a


def frozen(name, loc, scale, shape=None):
    d = getattr(scipy.stats, name)
    return d(loc=loc, scale=scale) if shape is None else d(shape, loc=loc, scale=scale)


def combos():
    """Every (family, loc, scale, shape or None) of the grid."""
    out = []
    for name in FAMILIES:
        for loc, scale in LOC_SCALE:
            for shape in SHAPES.get(name, (None,)):
                out.append((name, loc, scale, shape))
    return out


@functools.lru_cache(None)
def y_targets():
    r = numpy.random.RandomState(9301)
    y = numpy.concatenate([10.0 ** r.uniform(-12.0, 3.0, size=300),
                           [1.0 - 1e-9, 1.0 + 1e-9, 5e-324, 1e-300, 1e150, 1e155, 1e300,
                            0.0, 1.0, numpy.inf, numpy.nan]])
    return _ro(y)


def edge_x(loc, scale, at):
    """The float64 x whose y = (x - loc) / scale lands on `at` (0 or 1) -- or as near as the
    spacing of x allows -- and the nearest float on either side whose y is another, ascending."""
    x = numpy.float64(loc + scale * at)
    best = x
    for _ in range(64):
        y = (x - loc) / scale
        if y == at:
            best = x
            break
        x = numpy.nextafter(x, -numpy.inf if y > at else numpy.inf)
        if abs((x - loc) / scale - at) < abs((best - loc) / scale - at):
            best = x
    # the neighbours: the nearest floats whose y differs (several x can share one y)
    # (the step doubles until y moves: the division can round several x onto one y)
    y0 = (best - loc) / scale
    lo, hi = numpy.nextafter(best, -numpy.inf), numpy.nextafter(best, numpy.inf)
    d = best - lo
    while not (lo - loc) / scale < y0:
        d *= 2.0
        lo = best - d
    d = hi - best
    while not (hi - loc) / scale > y0:
        d *= 2.0
        hi = best + d
    return numpy.array([lo, best, hi])


@functools.lru_cache(None)
def grid_x(name, loc, scale):
    """The x of one (family, loc, scale): see the module docstring."""
    t = y_targets()
    ys = numpy.concatenate([t, -t]) if name in TWO_SIDED else numpy.concatenate([t, [-0.0, -1e-9,
                                                                                    -numpy.inf]])
    if name == "laplace":
        ys = numpy.concatenate([ys, LAPLACE_Y, -numpy.array(LAPLACE_Y)])
    with numpy.errstate(all="ignore"):
        x = loc + scale * ys
    x = numpy.concatenate([x, edge_x(loc, scale, 0.0), edge_x(loc, scale, 1.0)])
    return _ro(x)


def params(name, loc, scale, shape):
    """(family id, prm[8]) as nestmc.priors.encode gives them."""
    from nestmc import priors
    fam, prm = priors.encode(frozen(name, loc, scale, shape))
    return fam, numpy.array(prm, dtype=numpy.float64)


def _formula(name, y, a, lga):
    """(value, A) of scipy's _logpdf formula at the mpmath number y (inside the support)."""
    mp = mpmath
    if name == "norm":
        t = [-(y * y) / 2, -mp.log(mp.sqrt(2 * mp.pi))]
    elif name == "gamma":
        t = [(a - 1) * mp.log(y) if a != 1 else mp.mpf(0), -y, -lga]
    elif name == "uniform":
        t = [mp.mpf(0)]
    elif name == "expon":
        t = [-y]
    elif name == "halfnorm":
        t = [mp.log(2 / mp.pi) / 2, -(y * y) / 2]
    elif name == "cauchy":
        t = [-mp.log(mp.pi), -mp.log(1 + y * y)]
    elif name == "laplace":
        t = [mp.log(mp.mpf(0.5)), -abs(y)]
    elif name == "lognorm":
        p = a * y * mp.sqrt(2 * mp.pi)
        p64 = float(a) * float(y) * 2.5066282746310002      # scipy's and the device's product
        if p64 < 2.0 ** -1022:
            # a denormal product is rounded to a multiple of 2^-1074, not to 53 bits: no relative
            # bound holds for it.  IEEE multiplication gives scipy and the device the same
            # denormal, so the reference takes the logarithm of that float64 number.
            p = mp.mpf(p64)
        t = [-(mp.log(y) ** 2) / (2 * a * a), -mp.log(p)]
    elif name == "invgamma":
        t = [-(a + 1) * mp.log(y), -lga, -1 / y]
    else:
        raise ValueError(name)
    return sum(t), sum(abs(v) for v in t)


@functools.lru_cache(None)
def reference(name, loc, scale, shape):
    """(y float64 [n], value [n] mpmath or None, A [n] mpmath or None) over grid_x: None where
    the formula has no finite value (outside the open support, y not finite, gamma at 0 with
    a != 1)."""
    x = grid_x(name, loc, scale)
    fam, prm = params(name, loc, scale, shape)
    with numpy.errstate(all="ignore"):
        y = (x - loc) / scale
    vals, As = [], []
    with mpmath.workprec(PREC):
        a = mpmath.mpf(float(prm[2]))
        lga, ls = mpmath.mpf(float(prm[3])), mpmath.mpf(float(prm[4]))
        for yi in y:
            ok = numpy.isfinite(yi)
            if name not in TWO_SIDED:
                ok = ok and yi >= 0
            if name in ("lognorm", "invgamma") or (name == "gamma" and shape != 1.0):
                ok = ok and yi > 0
            if name == "uniform":
                ok = ok and yi <= 1
            if not ok:
                vals.append(None)
                As.append(None)
                continue
            v, A = _formula(name, mpmath.mpf(float(yi)), a, lga)
            vals.append(v - ls)
            As.append(A + abs(ls))
    return _ro(y), tuple(vals), tuple(As)


def units(got, name, loc, scale, shape, y_max=None):
    """|got - reference| / (2^-53 max(A, 1)) per grid point, NaN where there is no finite
    reference, where got is not finite, or where |y| > y_max."""
    y, vals, As = reference(name, loc, scale, shape)
    out = numpy.full(len(y), numpy.nan)
    with mpmath.workprec(PREC):
        for i, (g, v, A) in enumerate(zip(got, vals, As)):
            if v is None or not numpy.isfinite(g) or (y_max is not None and abs(y[i]) > y_max):
                continue
            out[i] = float(abs(mpmath.mpf(float(g)) - v) / (U53 * max(A, 1)))
    return out


def scipy_logpdf(name, loc, scale, shape):
    with numpy.errstate(all="ignore"):
        return numpy.asarray(frozen(name, loc, scale, shape).logpdf(grid_x(name, loc, scale)),
                             dtype=numpy.float64)


def y_max_of(name):
    return LAPLACE_MP_MAX if name == "laplace" else None


CAUCHY_OVERFLOW = 2.0 ** 512    # y * y overflows from here on; scipy's second branch does not


def laplace_tail(name, y):
    """The grid points of Laplace's denormal tail, 700 < |y| < 746, whose -inf pattern is not
    held to scipy's exactly but to check_finite's one-denormal-ulp rule."""
    if name != "laplace":
        return numpy.zeros(len(y), bool)
    ay = numpy.abs(y)
    return (ay > LAPLACE_MP_MAX) & (ay < 746.0)


def check_classification(got, name, loc, scale, shape):
    """Assertion 1: NaN, -inf and +inf fall where scipy's (as installed) fall -- the parity
    contract -- and every other value is finite."""
    c = (name, loc, scale, shape)
    want = scipy_logpdf(*c)
    x = grid_x(name, loc, scale)
    y = reference(*c)[0]
    keep = ~laplace_tail(name, y)
    for what, f in (("nan", numpy.isnan), ("-inf", lambda v: v == -numpy.inf),
                    ("+inf", lambda v: v == numpy.inf)):
        bad = numpy.flatnonzero((f(got) != f(want)) & (keep | (what != "-inf")))
        assert bad.size == 0, (c, what, x[bad[:5]], got[bad[:5]], want[bad[:5]])


def check_finite(got, name, loc, scale, shape):
    """Assertions 2 and 3: returns the worst error in units against the mpmath reference; raises
    where a finite value of scipy's has no reference, or on Laplace's tail rule: from |y| = 746
    on -inf; for 700 < |y| < 745.2 within 2 spacing(e) / e of scipy's float64 value, e = 0.5
    exp(-|y|) in float64 -- and where that e is 0 (scipy gives -inf from |y| = 744.04 on: half
    the smallest denormal rounds to 0) either -inf or, one denormal ulp up, the logarithm of the
    smallest denormal minus log(scale), within 4 ulp of that value."""
    c = (name, loc, scale, shape)
    want = scipy_logpdf(*c)
    y, vals, _ = reference(*c)
    fin = numpy.isfinite(want)
    u = units(got, *c, y_max=y_max_of(name))
    far = numpy.abs(y) > LAPLACE_MP_MAX if name == "laplace" else numpy.zeros(len(y), bool)
    missing = numpy.flatnonzero(fin & ~far & numpy.isnan(u))
    assert missing.size == 0, (c, "no reference for", y[missing[:5]], got[missing[:5]])
    if name == "laplace":
        ay = numpy.abs(y)
        assert numpy.all(got[far & (ay >= 746.0)] == -numpy.inf), c
        mid = numpy.flatnonzero(far & (ay < 745.2))
        assert len(mid) >= 20, c
        tiny = 5e-324
        ls = float(numpy.log(scale))
        for i in mid:
            e = 0.5 * numpy.exp(-ay[i])
            if e > 0.0:
                tol = 2.0 * float(numpy.spacing(e)) / e
                ok = abs(got[i] - want[i]) <= tol
            else:
                assert want[i] == -numpy.inf
                # one denormal ulp up is exactly the smallest denormal: its logarithm within
                # 2 ulp (the device's log), the subtraction of log(scale) one rounding more
                up = numpy.log(tiny) - ls
                ok = got[i] == -numpy.inf or abs(got[i] - up) <= 4.0 * numpy.spacing(abs(up))
            assert ok, (c, "laplace tail", y[i], got[i], want[i], e)
    return float(numpy.nanmax(u)) if numpy.any(~numpy.isnan(u)) else 0.0
