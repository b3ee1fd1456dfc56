"""Inputs and high-precision references for the variate math of csrc/rng.h and csrc/special.h
(tests/test_varmath_host.py on the CPU, tests/test_gpu_varmath.py on the GPU).

Nothing here needs a GPU: numpy builds the inputs, mpmath (200 bits) the references,
oracle/philox.py the stream; varmath() and igamci_host() call the hooks of a library the
caller loaded.  Every list is built once and cached; the callers must
leave the arrays unchanged.

Error measure: rel_u(got, want) = |got - want| / (|want| 2^-53), want from mpmath; where the
exact value is 0 (log at 1, the cosine at 1/4 and 3/4, Box-Muller with ua = 0 or a zero of the
cosine) the result must be 0 exactly, and rel_u returns inf otherwise.

Bounds (in these units, 2 per ulp at the top of a binade):
  LOG_BOUND = COS_BOUND = 4.8    DESIGN 3.2 documents "within 2.4 ulp" for nmc_log_unit and
                                 nmc_cos2pi; one ulp is at most 2 * 2^-53 relative.
  BM_BOUND = 9.2 (1 + 1e-6)      z = sqrt(-2 L) c with L, c the two functions above.  -2 L is
                                 exact; sqrt(L (1 + e)) = sqrt(L) (1 + e / 2 + ...), so the
                                 radius carries 4.8 / 2 from the log plus 1 for the rounding of
                                 the square root; the cosine brings 4.8 and the product one more
                                 rounding: 2.4 + 1 + 4.8 + 1 = 9.2.  The second-order terms are
                                 products of two of these, below 9.2^2 2^-53 < 1e-14 units; the
                                 factor 1 + 1e-6 covers them a hundred million times over.
  IGAMCI_RTOL = 1e-12            the project's bar for the inverse incomplete gamma
                                 (tests/test_gpu_parity.py::test_igamci_matches_scipy;
                                 gibbs_order.check relies on it).
"""

import functools

import mpmath
import numpy

from oracle import philox as ph

PREC = 200                      # bits of every mpmath reference
U53 = 2.0 ** -53
LOG_BOUND = 4.8
COS_BOUND = 4.8
BM_BOUND = 9.2 * (1.0 + 1e-6)
IGAMCI_RTOL = 1e-12
# |z| <= sqrt(-2 log(2^-53)): the radius at ua = 1 - 2^-53, the largest the stream can draw
BM_MAX = numpy.sqrt(2.0 * 53.0 * numpy.log(2.0)) * (1.0 + 1e-15)
LOG_SWITCH = 0.70710678118654752   # rng.h: m < this doubles m

WHICH_LOG, WHICH_COS, WHICH_BM = 0, 1, 2    # nmc_debug_varmath's selector


def _ro(a):
    a = numpy.ascontiguousarray(a, dtype=numpy.float64)
    a.setflags(write=False)
    return a


def rel_u(got, want):
    """|got - want| / (|want| 2^-53) per element, as floats; want: mpmath numbers.  An exact 0
    must be met exactly (else inf)."""
    out = numpy.empty(len(want))
    with mpmath.workprec(PREC):
        for i, (g, w) in enumerate(zip(got, want)):
            if w == 0:
                out[i] = 0.0 if g == 0.0 else numpy.inf
            elif not numpy.isfinite(g):
                out[i] = numpy.inf
            else:
                out[i] = float(abs(mpmath.mpf(float(g)) - w) / (abs(w) * U53))
    return out


# ---------------------------------------------------------------------------------------
# nmc_log_unit
# ---------------------------------------------------------------------------------------
@functools.lru_cache(None)
def log_inputs():
    """Arguments of nmc_log_unit with a finite reference: the ends of the grid k 2^-53, its
    first 64 points, the m < sqrt(1/2) switch at four exponents, the two denormal ends of
    "x in [0, 1]", and random grid points (whole range, k < 2^20, 1 - k 2^-53 at every scale)."""
    r = numpy.random.RandomState(5301)
    parts = [[1.0, 1.0 - U53, 1.0 - 2.0 ** -52, 0.5, 0.75],
             numpy.arange(1, 65) * U53]
    for e in (0, 1, 26, 52):
        c = LOG_SWITCH * 2.0 ** -e
        parts.append([numpy.nextafter(c, 0.0), c, numpy.nextafter(c, 1.0)])
    parts.append([5e-324, 2.0 ** -1022])
    parts.append(r.randint(1, 2 ** 53, size=20000, dtype=numpy.int64) * U53)
    parts.append(r.randint(1, 2 ** 20, size=2000, dtype=numpy.int64) * U53)
    k = numpy.floor(2.0 ** r.uniform(0.0, 53.0, size=2000))
    parts.append(1.0 - k * U53)
    x = numpy.concatenate([numpy.asarray(p, dtype=numpy.float64) for p in parts])
    assert numpy.all((x > 0.0) & (x <= 1.0))
    return _ro(x)


@functools.lru_cache(None)
def log_reference():
    with mpmath.workprec(PREC):
        return tuple(mpmath.log(mpmath.mpf(float(x))) for x in log_inputs())


# ---------------------------------------------------------------------------------------
# nmc_cos2pi
# ---------------------------------------------------------------------------------------
@functools.lru_cache(None)
def cos_branch_points():
    """c + k 2^-53 around every eighth (the three folds of the reduction, the zeros at 1/4 and
    3/4, the ends), |k| <= 40 and k = +-2^10, +-2^20, +-2^30, clipped to [0, 1), and 1 - 2^-53."""
    ks = list(range(-40, 41)) + [s * 2 ** j for j in (10, 20, 30) for s in (-1, 1)]
    u = numpy.array([c / 8.0 + k * U53 for c in range(8) for k in ks] + [1.0 - U53])
    u = numpy.unique(u[(u >= 0.0) & (u < 1.0)])
    assert numpy.array_equal(u * 2.0 ** 53, numpy.round(u * 2.0 ** 53))   # all on the grid
    return _ro(u)


@functools.lru_cache(None)
def cos_inputs():
    r = numpy.random.RandomState(5302)
    return _ro(numpy.concatenate([cos_branch_points(),
                                  r.randint(0, 2 ** 53, size=20000, dtype=numpy.int64) * U53]))


def _cos2pi_mp(u):
    """cos(2 pi u) from the argument itself: mpmath.cospi reduces 2 u exactly, so the zeros at
    u = 1/4, 3/4 are exact zeros, whatever the precision of pi."""
    return mpmath.cospi(2 * mpmath.mpf(float(u)))


@functools.lru_cache(None)
def cos_reference():
    with mpmath.workprec(PREC):
        return tuple(_cos2pi_mp(u) for u in cos_inputs())


# ---------------------------------------------------------------------------------------
# nmc_box_muller
# ---------------------------------------------------------------------------------------
@functools.lru_cache(None)
def bm_inputs():
    """(ua, ub): the ends and the middle of ua against every cosine branch point, and random
    pairs of 53-bit uniforms."""
    r = numpy.random.RandomState(5303)
    ub = cos_branch_points()
    ua = numpy.array([0.0, U53, 0.5, 1.0 - U53])
    a = numpy.concatenate([numpy.repeat(ua, len(ub)),
                           r.randint(0, 2 ** 53, size=20000, dtype=numpy.int64) * U53])
    b = numpy.concatenate([numpy.tile(ub, len(ua)),
                           r.randint(0, 2 ** 53, size=20000, dtype=numpy.int64) * U53])
    return _ro(a), _ro(b)


@functools.lru_cache(None)
def bm_reference():
    ua, ub = bm_inputs()
    with mpmath.workprec(PREC):
        return tuple(mpmath.sqrt(-2 * mpmath.log(1 - mpmath.mpf(float(a)))) * _cos2pi_mp(b)
                     for a, b in zip(ua, ub))


def device_extra():
    """Inputs beyond the functions' domains that host and device must still agree on."""
    return numpy.array([0.0, -0.0, numpy.inf, -numpy.inf, numpy.nan, 2.0, -1.0, 1.0])


def same_words(a, b):
    """Indices where two float64 arrays differ as 64-bit words; any NaN equals any NaN."""
    a, b = numpy.ascontiguousarray(a), numpy.ascontiguousarray(b)
    same = (a.view(numpy.uint64) == b.view(numpy.uint64)) | (numpy.isnan(a) & numpy.isnan(b))
    return numpy.flatnonzero(~same)


def varmath(lib, which, a, b=None, on_device=0):
    """nmc_debug_varmath of the loaded library lib on a (and b: Box-Muller's second uniform)."""
    from nestmc._lib import check, dptr
    a = numpy.ascontiguousarray(a, dtype=numpy.float64)
    b = a if b is None else numpy.ascontiguousarray(b, dtype=numpy.float64)
    out = numpy.empty_like(a)
    check(lib.nmc_debug_varmath(which, dptr(a), dptr(b), len(a), dptr(out), on_device))
    return out


def igamci_host(lib, a, q):
    """nmc_debug_igamci_host (no GPU) with gammaln(a) from scipy, as the engine passes it."""
    import scipy.special
    from nestmc._lib import check, dptr
    a = numpy.ascontiguousarray(a, dtype=numpy.float64)
    q = numpy.ascontiguousarray(q, dtype=numpy.float64)
    with numpy.errstate(all="ignore"):
        lga = numpy.ascontiguousarray(scipy.special.gammaln(a))
    out = numpy.empty_like(a)
    check(lib.nmc_debug_igamci_host(dptr(a), dptr(q), dptr(lga), len(a), dptr(out)))
    return out


# ---------------------------------------------------------------------------------------
# nmc_igamci: x with Q(a, x) = q
# ---------------------------------------------------------------------------------------
IGAMCI_SHAPES = (0.5, 1.0, 1.5, 2.0, 3.5, 16.0, 31.5, 64.0, 127.5, 512.0)   # G = 2 ... 1025
IGAMCI_Q = (2.0 ** -53, 1e-12, 1e-6, 1e-3, 0.05, 0.25, 0.5 - 2.0 ** -54, 0.5, 0.5 + 2.0 ** -53,
            0.75, 0.95, 0.999, 1.0 - 1e-9, 1.0 - 2.0 ** -53)
IGAMCI_BEYOND = 2047.5          # printed, not asserted


def igamci_q(a):
    """The probabilities of shape a: the grid and 200 random ones."""
    r = numpy.random.RandomState(5304 + int(2 * a))
    return numpy.concatenate([IGAMCI_Q, r.uniform(size=200)])


@functools.lru_cache(None)
def igamci_inputs():
    a = numpy.concatenate([numpy.full(len(igamci_q(s)), s) for s in IGAMCI_SHAPES])
    q = numpy.concatenate([igamci_q(s) for s in IGAMCI_SHAPES])
    return _ro(a), _ro(q)


def igamci_root(a, q, prec=PREC):
    """The root x of Q(a, x) = q as an mpmath number: Newton's iteration in mpmath on the
    smaller tail (Q = q below 1/2, P = 1 - q, exact, above), started from scipy's double.  The
    start only saves iterations: the loop ends when a step moves x by less than 2^-(prec/2)
    relative, and Newton's next iterate is then good to about 2^-prec, so nothing of scipy's
    error is left in the result."""
    import scipy.special
    with mpmath.workprec(prec + 40):
        am, qm = mpmath.mpf(float(a)), mpmath.mpf(float(q))
        upper = q < 0.5
        target = qm if upper else 1 - qm
        x = mpmath.mpf(float(scipy.special.gammainccinv(a, q)))
        lga = mpmath.loggamma(am)
        for _ in range(12):
            if upper:
                f = mpmath.gammainc(am, x, mpmath.inf, regularized=True) - target
            else:
                f = target - mpmath.gammainc(am, 0, x, regularized=True)
            dens = mpmath.exp((am - 1) * mpmath.log(x) - x - lga)     # -dQ/dx
            step = f / dens
            x = x + step
            if abs(step) <= abs(x) * mpmath.mpf(2) ** (-(prec // 2)):
                return +x
        raise AssertionError(("igamci_root did not converge", a, q))


@functools.lru_cache(None)
def igamci_reference():
    a, q = igamci_inputs()
    return tuple(igamci_root(ai, qi) for ai, qi in zip(a, q))


def igamci_rel(got, want):
    """|got / want - 1| per element."""
    with mpmath.workprec(PREC):
        return numpy.array([float(abs(mpmath.mpf(float(g)) / w - 1)) if numpy.isfinite(g)
                            else numpy.inf for g, w in zip(got, want)])


# (a, q) -> the special value nmc_igamci must return, word for word (NaN: any NaN)
IGAMCI_SPECIAL = ((1.5, 0.0, numpy.inf), (1.0, 0.0, numpy.inf), (1.5, 1.0, 0.0), (0.5, 1.0, 0.0),
                  (1.5, numpy.nan, numpy.nan), (1.5, -1e-300, numpy.nan), (1.5, -1.0, numpy.nan),
                  (1.5, 1.0 + 2.0 ** -52, numpy.nan), (1.5, numpy.inf, numpy.nan),
                  (0.0, 0.5, numpy.nan), (-1.0, 0.5, numpy.nan), (numpy.nan, 0.5, numpy.nan),
                  (-numpy.inf, 0.5, numpy.nan))


# ---------------------------------------------------------------------------------------
# the Gamma draw (nmc_gamma_mt against oracle/philox.py:gamma_mt)
# ---------------------------------------------------------------------------------------
GAMMA_SHAPES = (0.5, 1.0, 1.5, 2.0, 31.5, 511.5, 2047.5)   # 1.0: the first that does not boost
GAMMA_IT, GAMMA_PARAM, GAMMA_SEED, GAMMA_N = 5, 1, 1234, 20000
GAMMA_RTOL = 1e-13
GAMMA_MARGIN = 1e-9             # no acceptance test of any draw is decided by less
GAMMA_KS_P = 1e-3               # tests/test_oracle_golden.py::test_philox_gamma_distribution
# Marsaglia-Tsang rejects 4.8 % of its attempts at a = 1 (boosted 0.5 runs at 1.5), 2-3 % at
# 1.5 and 2, and ever fewer as the shape grows (about 1 in 10^4 at 511.5): these shapes must
# each send at least 50 of the 20 000 draws to a second attempt (purposes 18 and 19); the large
# ones cannot, and only print their count.
GAMMA_SECOND_ATTEMPT_SHAPES = (0.5, 1.0, 1.5, 2.0)
GAMMA_SECOND_ATTEMPTS = 50


def gamma_counters():
    """nmc_debug_rng's counters (iter, group, param, purpose, chain) of the shared draws."""
    ctr = numpy.zeros((GAMMA_N, 5), numpy.uint32)
    ctr[:, 0], ctr[:, 2], ctr[:, 4] = GAMMA_IT, GAMMA_PARAM, numpy.arange(GAMMA_N)
    return ctr


@functools.lru_cache(None)
def gamma_oracle(a):
    """(draws, accepting attempt, decision margin) of the oracle for shape a."""
    x, k, m = ph.gamma_mt(a, GAMMA_IT, GAMMA_PARAM, numpy.arange(GAMMA_N), GAMMA_SEED,
                          return_attempts=True)
    return _ro(x), k, _ro(m)


def gamma_moments(x, a):
    """(|mean - a| in standard errors, |variance - a| in standard errors) of draws x from
    Gamma(a, 1): Var(mean) = a / n; Var(s^2) = (mu4 - sigma^4 (n - 3) / (n - 1)) / n with the
    fourth central moment mu4 = 3 a (a + 2) of Gamma(a)."""
    n = len(x)
    se_mean = numpy.sqrt(a / n)
    se_var = numpy.sqrt((3.0 * a * (a + 2.0) - a * a * (n - 3.0) / (n - 1.0)) / n)
    return abs(numpy.mean(x) - a) / se_mean, abs(numpy.var(x, ddof=1) - a) / se_var


def gamma_distribution_ok(x, a):
    """The distribution conditions of the GPU test: (KS p, mean error, variance error)."""
    import scipy.stats
    p = scipy.stats.kstest(x, scipy.stats.gamma(a).cdf).pvalue
    em, ev = gamma_moments(x, a)
    return p, em, ev


# ---------------------------------------------------------------------------------------
# the hyper rows from the stream (nmc_k_fill<false>, the sweep's in-kernel draw)
# ---------------------------------------------------------------------------------------
STREAM_KIND, STREAM_C, STREAM_BASE, STREAM_ITERS = "linreg2", 70, 7, 4
# G = 2 (shape 0.5: the boost) and 3 (shape 1), the smallest G of every further (kernel, mode)
# that rowpath_cases.gibbs_mode tells apart for this model, and 513, where the groups are more
# than four numpy leaves and the all-wave update returns (tests/test_varmath_host.py derives
# them from gibbs_mode)
STREAM_G = (2, 3, 65, 117, 129, 513)


def stream_counters(G, P, n_iter=STREAM_ITERS, C=STREAM_C, base=STREAM_BASE):
    """Counters [n_iter, P, C, 5] of the hyper draws of recorded row i = iteration i
    (oracle/restatement.py: PhiloxRNG.hyper_mean / hyper_s2 draw at (i, 0, p, purpose, chain),
    i counted from 0 as run()'s loop counts it, chain = chain_base + c)."""
    ctr = numpy.zeros((n_iter, P, C, 5), numpy.uint32)
    ctr[..., 0] = numpy.arange(n_iter)[:, None, None]
    ctr[..., 2] = numpy.arange(P)[None, :, None]
    ctr[..., 3] = ph.PURPOSE_HYPER_NORMAL
    ctr[..., 4] = base + numpy.arange(C)[None, None, :]
    return ctr


def check_stream_rows(rows, s2_start, hz, g, G, P, what):
    """rows [C, n, cols] recorded from the start (burn 0, thin 1); hz, g [n, P, C]: the normal
    and the Gamma((G - 1) / 2) draw of each (row, parameter, chain).  Bit for bit, from the
    row's own mu, s2 and values x (gibbs.h's expressions):
      mu == numpy.sum(x) / G + numpy.sqrt(s2_prev / G) * hz
      s2 == (1.0 / g) * (a * (numpy.sum((x - mu)**2) / (G - 1)))"""
    C, n = rows.shape[0], rows.shape[1]
    a = (G - 1) / 2.0
    for i in range(n):
        for p in range(P):
            o = p * (G + 2)
            mu, s2, x = rows[:, i, o], rows[:, i, o + 1], rows[:, i, o + 2:o + 2 + G]
            s2_prev = rows[:, i - 1, o + 1] if i else s2_start[:, p]
            assert numpy.all(numpy.isfinite(mu)) and numpy.all(s2 > 0), (what, i, p)
            x = numpy.ascontiguousarray(x)
            tot = numpy.array([numpy.sum(x[c]) for c in range(C)])
            want = tot / G + numpy.sqrt(s2_prev / G) * hz[i, p]
            bad = numpy.flatnonzero(mu != want)
            assert bad.size == 0, ("hyper mean", what, i, p, bad[:5], mu[bad[0]], want[bad[0]])
            d = x - mu[:, None]
            dd = numpy.ascontiguousarray(d * d)
            ss = numpy.array([numpy.sum(dd[c]) for c in range(C)])
            want = (1.0 / g[i, p]) * (a * (ss / (G - 1)))
            bad = numpy.flatnonzero(s2 != want)
            assert bad.size == 0, ("hyper s2", what, i, p, bad[:5], s2[bad[0]], want[bad[0]])
