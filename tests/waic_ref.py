"""The longdouble reference and the two tolerances of the WAIC tests.

u = 2^-52; L is the float64 matrix ll[S, n_obs] cast to numpy.longdouble; the reference is
the direct max-shifted log-sum-exp and the two-pass variance, both in longdouble.

  Tol-lppd  |lppd_i - ref| <= (S + 64) u (1 + |lppd_i|)
            sequential summation of S positive terms has relative error <= (S - 1) u; the 64
            covers exp's ulp and the rounding of its argument x - m (relative effect
            |x - m| u) for |x - m| up to about 50
  Tol-M2    |M2_i - ref| <= (S + 64) u sum_s ll_is^2,  M2_i = p_waic_i (S - 1)
            the Chan-Golub-LeVeque bound c S u ||x|| sqrt(M2), weakened to ||x||^2
"""

import numpy

U = 2.0 ** -52


def reference(ll):
    """(lppd_i, M2_i, sum_s ll_is^2, max_s |ll_is|) of ll[S, n_obs], in longdouble."""
    L = numpy.asarray(ll, dtype=numpy.float64).astype(numpy.longdouble)
    S = L.shape[0]
    mx = L.max(axis=0)
    lppd = mx + numpy.log(numpy.sum(numpy.exp(L - mx), axis=0) / S)
    mean = numpy.sum(L, axis=0) / S
    M2 = numpy.sum((L - mean) ** 2, axis=0)
    return lppd, M2, numpy.sum(L * L, axis=0), numpy.abs(L).max(axis=0)


def check(res, ll, rel_ll=0.0, what=""):
    """Tol-lppd and Tol-M2 on every observation of WaicResult res against ll[S, n_obs];
    rel_ll: the relative agreement granted to the ll themselves (0: they are the device's
    own), which widens lppd by rel_ll (1 + max_s |ll_is|) and M2 by 4 rel_ll sum_s ll_is^2.
    Prints the worst ratios error / tolerance before it asserts."""
    lppd, M2, sq, amax = reference(ll)
    S = numpy.asarray(ll).shape[0]
    assert res.n_samples == S, (what, res.n_samples, S)
    tol_l = (S + 64) * U * (1 + numpy.abs(lppd)) + rel_ll * (1 + amax)
    tol_m = (S + 64) * U * sq + 4 * rel_ll * sq
    err_l = numpy.abs(res.lppd_i.astype(numpy.longdouble) - lppd)
    err_m = numpy.abs(res.p_waic_i.astype(numpy.longdouble) * (S - 1) - M2)
    rl, rm = float(numpy.max(err_l / tol_l)), float(numpy.max(err_m / tol_m))
    print("waic check %s: S=%d n_obs=%d  max err/Tol-lppd=%.3g  max err/Tol-M2=%.3g"
          % (what, S, len(lppd), rl, rm))
    assert numpy.all(err_l <= tol_l), (what, "lppd", rl)
    assert numpy.all(err_m <= tol_m), (what, "M2", rm)
    # the derived fields follow the definitions
    assert numpy.array_equal(res.elpd_i, res.lppd_i - res.p_waic_i)
    assert res.elpd == float(numpy.sum(res.elpd_i)) and res.waic == -2.0 * res.elpd
    assert res.p_waic == float(numpy.sum(res.p_waic_i))
    return rl, rm
