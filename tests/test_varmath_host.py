"""CPU: the host forms of the variate math (csrc/rng.h, csrc/special.h) against mpmath.

nmc_log_unit, nmc_cos2pi and nmc_box_muller are built from IEEE + - * /, fma, sqrt and frexp
alone and compiled without contraction, so the host and the device compute the same bits
(tests/test_gpu_varmath.py asserts that on these very inputs); the accuracy sweep against
200-bit references therefore runs here, once, through nmc_debug_varmath(on_device = 0).
nmc_igamci's host form uses libm's log / exp / pow / lgamma where the device uses its own, so
each is held to the mpmath root of Q(a, x) = q by itself (the device's in the GPU test).

The inputs, references, bounds and their derivations are in tests/varmath_ref.py.  Every test
prints its measured worst value; DESIGN 3.2 records them.
"""

import numpy
import pytest
import scipy.special

import varmath_ref as vr
from oracle import philox as ph


@pytest.fixture(scope="module")
def lib():
    from nestmc import _lib
    return _lib.load()


def test_log_unit_host_against_mpmath(lib):
    x = vr.log_inputs()
    got = vr.varmath(lib, vr.WHICH_LOG, x)
    err = vr.rel_u(got, vr.log_reference())
    den = x < 2.0 ** -1021
    worst = int(numpy.argmax(err))
    print("VARMATH log_unit: worst %.3f x 2^-53 at x = %r (%d inputs); denormal arguments %.3f"
          % (err[worst], x[worst], len(x), err[den].max()))
    assert den.sum() == 2
    assert err.max() <= vr.LOG_BOUND, (x[worst], got[worst], err[worst])
    assert got[x == 1.0].size and numpy.all(got[x == 1.0] == 0.0)
    sp = vr.varmath(lib, vr.WHICH_LOG, numpy.array([0.0, -0.0, numpy.nan]))
    assert sp[0] == -numpy.inf and sp[1] == -numpy.inf and numpy.isnan(sp[2])


def test_cos2pi_host_against_mpmath(lib):
    u = vr.cos_inputs()
    got = vr.varmath(lib, vr.WHICH_COS, u)
    ref = vr.cos_reference()
    err = vr.rel_u(got, ref)
    small = numpy.array([abs(float(w)) < 1e-3 for w in ref])
    assert small.sum() >= 2 * 87       # the 87 branch points around each of the two zeros
    worst = int(numpy.argmax(err))
    print("VARMATH cos2pi: worst %.3f x 2^-53 at u = %r (%d inputs); where |cos| < 1e-3: %.3f "
          "(%d inputs); elsewhere %.3f" % (err[worst], u[worst], len(u), err[small].max(),
                                          small.sum(), err[~small].max()))
    assert err.max() <= vr.COS_BOUND, (u[worst], got[worst], err[worst])
    for z in (0.25, 0.75):             # exact zeros, and they are among the inputs
        assert numpy.any(u == z) and numpy.all(got[u == z] == 0.0)
    assert numpy.all(got[u == 0.0] == 1.0) and numpy.all(got[u == 0.5] == -1.0)
    assert numpy.any(u == 0.0) and numpy.any(u == 0.5)
    # the odd eighths, where w == 1/8 takes the cosine polynomial (w > 0.125 is false): it
    # returns the double nearest to sqrt(1/2); the sine polynomial at t = 1/8 gives the one below
    r = numpy.sqrt(0.5)
    assert abs(float(ref[int(numpy.flatnonzero(u == 0.125)[0])]) - r) < 1e-16
    for k, want in ((1, r), (3, -r), (5, -r), (7, r)):
        assert numpy.all(got[u == k / 8.0] == want), (k, got[u == k / 8.0], want)
    # the symmetries are exact: every fold of the reduction is an exact difference
    w = lambda v: v.view(numpy.uint64)   # noqa: E731
    mirror = vr.varmath(lib, vr.WHICH_COS, 1.0 - u)
    assert numpy.array_equal(w(mirror), w(got))
    lo = u[u <= 0.5]
    anti = vr.varmath(lib, vr.WHICH_COS, 0.5 - lo)
    assert numpy.array_equal(anti, -got[u <= 0.5])
    nz = got[u <= 0.5] != 0.0            # (+0 and -0 compare equal; the rest word for word)
    assert numpy.array_equal(w(anti[nz]), w((-got[u <= 0.5])[nz]))


def test_oracle_cos2pi_against_mpmath():
    """oracle/philox.py:cos2pi (numpy's sin / cos of 2 pi t after the same exact reduction).  In
    units of 2^-53 relative: the rounded constant 2 pi and the rounded product each bring at
    most 1 to the argument, which the sine and the cosine pass on with a condition number of at
    most 1 on [0, pi / 4] (x cot x <= 1, x tan x <= pi / 4); the library's sin / cos are below
    1 ulp = 2 units: 4 in all, as the docstring there states."""
    u = vr.cos_inputs()
    err = vr.rel_u(ph.cos2pi(u), vr.cos_reference())
    print("VARMATH oracle cos2pi: worst %.3f x 2^-53" % err.max())
    assert err.max() <= 4.0


def test_box_muller_host_against_mpmath(lib):
    ua, ub = vr.bm_inputs()
    got = vr.varmath(lib, vr.WHICH_BM, ua, ub)
    err = vr.rel_u(got, vr.bm_reference())
    worst = int(numpy.argmax(err))
    print("VARMATH box_muller: worst %.3f x 2^-53 at (ua, ub) = (%r, %r) (%d inputs); "
          "max |z| %.6f" % (err[worst], ua[worst], ub[worst], len(ua), numpy.abs(got).max()))
    assert numpy.all(numpy.isfinite(got))
    assert numpy.abs(got).max() <= vr.BM_MAX
    assert numpy.abs(got).max() >= 8.5          # the far end of ua is among the inputs
    assert (ua == 0.0).sum() > 100 and numpy.all(got[ua == 0.0] == 0.0)
    assert err.max() <= vr.BM_BOUND, (ua[worst], ub[worst], got[worst], err[worst])


def test_igamci_host_against_mpmath_root(lib):
    a, q = vr.igamci_inputs()
    ref = vr.igamci_reference()
    got = vr.igamci_host(lib, a, q)
    err = vr.igamci_rel(got, ref)
    sci = vr.igamci_rel(scipy.special.gammainccinv(a, q), ref)
    for s in vr.IGAMCI_SHAPES:
        k = a == s
        i = numpy.flatnonzero(k)[numpy.argmax(err[k])]
        print("VARMATH igamci host a = %-6g worst %.3e at q = %r; scipy's own %.3e"
              % (s, err[i], q[i], sci[k].max()))
    print("VARMATH igamci host: worst %.3e, scipy's own worst %.3e (bar %.0e)"
          % (err.max(), sci.max(), vr.IGAMCI_RTOL))
    # the reference does not move with the precision it was computed at
    for i in (0, 13, len(ref) - 214, len(ref) - 201):
        again = vr.igamci_root(a[i], q[i], prec=2 * vr.PREC)
        assert abs(again / ref[i] - 1) < 1e-40, (a[i], q[i])
    assert sci.max() <= vr.IGAMCI_RTOL / 10      # scipy itself is well inside the bar
    bad = numpy.flatnonzero(~(err <= vr.IGAMCI_RTOL))
    assert bad.size == 0, [(a[i], q[i], got[i], err[i]) for i in bad[:8]]


def test_igamci_host_special_values(lib):
    a = numpy.array([s[0] for s in vr.IGAMCI_SPECIAL])
    q = numpy.array([s[1] for s in vr.IGAMCI_SPECIAL])
    want = numpy.array([s[2] for s in vr.IGAMCI_SPECIAL])
    got = vr.igamci_host(lib, a, q)
    assert vr.same_words(got, want).size == 0, (got, want)


def test_igamci_host_beyond_the_claimed_shapes(lib):
    """a = 2047.5 (G = 4096) is beyond the shapes the 1e-12 bar was shown for: printed only."""
    q = vr.igamci_q(vr.IGAMCI_BEYOND)
    a = numpy.full(len(q), vr.IGAMCI_BEYOND)
    ref = [vr.igamci_root(ai, qi) for ai, qi in zip(a, q)]
    err = vr.igamci_rel(vr.igamci_host(lib, a, q), ref)
    print("VARMATH igamci host a = %g: worst %.3e at q = %r (not asserted)"
          % (vr.IGAMCI_BEYOND, err.max(), q[int(numpy.argmax(err))]))
    assert numpy.all(numpy.isfinite(err))


@pytest.mark.parametrize("a", vr.GAMMA_SHAPES)
def test_gamma_cases_decide_nothing_by_rounding(a):
    """The shared counters of the GPU Gamma test: no comparison of any draw is nearer to its
    threshold than 1e-9 (a device log or Box-Muller that differs by rounding cannot change an
    attempt), enough draws reach a second attempt, and the oracle's own draws meet the
    distribution conditions the device's will be held to."""
    x, k, m = vr.gamma_oracle(a)
    again = int((k >= 1).sum())
    p, em, ev = vr.gamma_distribution_ok(x, a)
    print("VARMATH gamma cases a = %-6g min margin %.3e, second attempts %d, third %d, KS p "
          "%.3f, mean off %.2f se, variance off %.2f se"
          % (a, m.min(), again, int((k >= 2).sum()), p, em, ev))
    assert numpy.array_equal(x, ph.gamma_mt(a, vr.GAMMA_IT, vr.GAMMA_PARAM,
                                            numpy.arange(vr.GAMMA_N), vr.GAMMA_SEED))
    assert numpy.all(k >= 0) and numpy.all(x > 0)
    assert m.min() > vr.GAMMA_MARGIN
    if a in vr.GAMMA_SECOND_ATTEMPT_SHAPES:
        assert again >= vr.GAMMA_SECOND_ATTEMPTS
    assert p > vr.GAMMA_KS_P and em <= 5.0 and ev <= 5.0


def test_stream_cases_are_the_smallest_of_their_modes():
    """STREAM_G: 2 and 3 (the boosted shape 0.5, and shape 1), the first G of every (kernel,
    mode) that rowpath_cases.gibbs_mode tells apart, and the first G of more than four numpy
    leaves."""
    import rowpath_cases as rc
    first = {}
    for G in range(2, 600):
        first.setdefault(rc.gibbs_mode(*rc.gibbs_model(vr.STREAM_KIND, G)), G)
    assert len(first) == 4, first
    assert len(rc.pairwise_leaves(512)) <= 4 < len(rc.pairwise_leaves(513))
    assert tuple(sorted(set(first.values()) | {2, 3, 513})) == vr.STREAM_G, first
    ctr = vr.stream_counters(3, 2)
    assert ctr.shape == (vr.STREAM_ITERS, 2, vr.STREAM_C, 5)
    assert ctr[3, 1, 69].tolist() == [3, 0, 1, ph.PURPOSE_HYPER_NORMAL, 76]


def _literals(body, var, arg):
    import re
    number = r"(-?[0-9.]+(?:e[+-]?[0-9]+)?)"
    return [float(v) for v in re.findall(
        r"(?:double %s = |%s = fma\(%s, %s, )%s\)?;" % (var, var, var, arg, number), body)]


def test_polynomial_coefficients_are_the_rounded_series_terms():
    """Every coefficient of rng.h's three polynomials is the double nearest to its term of the
    series the header names: 2 / (2k + 1) for 2 atanh(s), (-1)^k (2 pi)^2k / (2k)! for the cosine,
    (-1)^k (2 pi)^(2k+1) / (2k+1)! for the sine; 2 pi and the two parts of ln 2 likewise (ln2_hi
    with 32 significant bits, so that e * ln2_hi is exact).  One changed last digit of a
    coefficient moves results by less than the rounding of the evaluation, which no accuracy
    bound sees; it does not pass here."""
    import os
    import mpmath
    import nestmc
    pkg = os.path.dirname(os.path.dirname(nestmc.__file__))
    with open(os.path.join(pkg, "csrc", "rng.h")) as f:
        src = f.read()
    log_body = src.split("NMC_HD double nmc_log_unit")[1].split("NMC_HD double nmc_cos2pi")[0]
    cos_body = src.split("NMC_HD double nmc_cos2pi")[1].split("NMC_HD double nmc_box_muller")[0]
    with mpmath.workprec(vr.PREC):
        tp = 2 * mpmath.pi
        want_q = [float(mpmath.mpf(2) / (2 * k + 1)) for k in range(11, 0, -1)]
        want_c = [float((-1) ** k * tp ** (2 * k) / mpmath.factorial(2 * k))
                  for k in range(9, -1, -1)]
        want_p = [float((-1) ** k * tp ** (2 * k + 1) / mpmath.factorial(2 * k + 1))
                  for k in range(9, 0, -1)]
        ln2_hi = 0.6931471803691238
        want_lo = float(mpmath.log(2) - mpmath.mpf(ln2_hi))
        assert abs(mpmath.log(2) - ln2_hi) < mpmath.mpf(2) ** -32
        two_pi = float(tp)
    assert _literals(log_body, "q", "z") == want_q
    assert _literals(cos_body, "c", "x") == want_c
    assert _literals(cos_body, "p", "x") == want_p
    assert numpy.float64(ln2_hi).view(numpy.uint64) & numpy.uint64((1 << 21) - 1) == 0
    assert "fma(ed, %r, l)" % ln2_hi in log_body and "fma(ed, %r, 2.0 * s)" % want_lo in log_body
    assert "%r * t" % two_pi in cos_body
