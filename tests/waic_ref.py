"""The longdouble reference and the two tolerances of the WAIC tests.

u = 2^-52; L is the float64 matrix ll[S, n_obs] cast to numpy.longdouble; the reference is
the direct max-shifted log-sum-exp and the two-pass variance, both in longdouble.

  Tol-lppd  |lppd_i - ref| <= (S + 64) u (1 + |lppd_i|)
            sequential summation of S positive terms has relative error <= (S - 1) u; the 64
            covers exp's ulp and the rounding of its argument x - m (relative effect
            |x - m| u) for |x - m| up to about 50
  Tol-M2    |M2_i - ref| <= (S + 64) u sum_s ll_is^2,  M2_i = p_waic_i (S - 1)
            the Chan-Golub-LeVeque bound c S u ||x|| sqrt(M2), weakened to ||x||^2

Tol-lppd beyond |x - m| of about 50 (the stores of tests/store_cases.py, whose ll of one
observation spread over more than 1490).  A step is s' = s e + 1 (a new maximum), s + e, or
the merge's sA exp(mA - m) + sB, with e = exp(-|d|); the rounding of d = x - m changes e by
the relative amount |d| u.  Relative to the new sum (>= 1, the term of the maximum) that is
|d| u s e / (s e + 1) <= u min(|d|, |d| s e^-|d|) <= (1 + ln s) u: below |d| = 1 + ln s the
first, above it the second, which falls in |d| and is (1 + ln s) / e there.  So however
large |d| is, a step costs at most (2 + ln S) u with its own rounding.  A term passes
through at most R steps of its lane, 6 of the butterfly and CB - 1 of the host merge -- the
kernel's longest chain, not the S - 1 additions Tol-lppd allows for: (R + 5 + CB)
(2 + ln S) u + 3 u in all (exp's ulp, the division, the log), which is below (S + 64) u for
every window and n_valid of the tests (R = 20, CB = 2, S = 1400: 252 u against 1464 u;
R = 1, S = 64: 53 u against 128 u).  The tolerance stands as it is, and
tests/test_store_cases.py holds the restatement to it on those stores.

Tol-M2-sharp  |M2_i - ref| <= C_M2 (S + 64) u (M2 + ||ll_i||_2 sqrt(M2)),  C_M2 = 4
            the unweakened form (``tol_m2_sharp``; ``check`` keeps Tol-M2).  Welford's running
            mean after k terms has the error eps_k <= (k / 2) u max_j |mean_j| to first order
            (each update rounds the new mean, u |mean|, and the error of the old one is damped
            by 1 - 1/k), and |mean| <= ||x|| / sqrt(S): eps <= (S / 2) u ||x|| / sqrt(S).  The
            addend dl (x - mean_k) then carries eps (|dl| + |x - mean_k|) <= 2 eps |dl| beside
            its own 3 u, and sum_k |dl_k| <= sqrt(S) sqrt(sum dl_k^2) <= sqrt(S) sqrt(2 M2)
            (sum_k dl_k^2 (k - 1) / k = M2): the updates contribute sqrt(2) S u ||x|| sqrt(M2)
            and the sum itself (S + 2) u M2.  A merge adds d^2 nA nB / n with d = meanB - meanA
            in error by 2 eps: 4 eps |d| nA nB / n <= 4 eps sqrt(M2') sqrt(n) / 2 for the
            merged M2' and count n; over the 2^l merges of level l (n = S / 2^l, sum of the
            sqrt(M2') <= 2^(l/2) sqrt(M2), eps <= (n / 2) u ||x|| / sqrt(S)) that is
            S u ||x|| sqrt(M2) / 2^l, over all levels at most 2 S u ||x|| sqrt(M2).  In all
            (S + 2) u M2 + (sqrt(2) + 2) S u ||x|| sqrt(M2): C_M2 = 4 covers both factors, the
            64 the lower-order terms.  The bound counts the mean's error as if one chain of S
            updates had made it; the kernel's lanes make R and the merges 6 + CB more, so the
            measured ratios are far below 1.  A one-pass sum x^2 - (sum x)^2 / S is in error by
            about u ||x||^2, beyond this bound once ||x|| / sqrt(M2) exceeds 4 (S + 64).

``restate`` is nmc_k_waic's arithmetic (csrc/waic.h) in float64, operation by operation:
the lanes' recurrences over the rows, the butterfly (a balanced tree over the 64 lanes, the
lower lane's state the A operand), chains >= n_valid as the identity, nestmc.waic.merge over
the chain blocks.  It differs from the device only in exp itself (numpy's against the
device library's, each within an ulp): on the same log-likelihoods m, n, mean and M2 are the
device's words bit for bit, s and with it lppd agree within twice Tol-lppd.  Its ``mutant``
forms are the errors tests/test_store_cases.py shows the tolerances catch.
"""

import numpy

U = 2.0 ** -52
C_M2 = 4.0


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


def tol_lppd(lppd, S):
    return (S + 64) * U * (1 + numpy.abs(lppd))


def tol_m2_sharp(M2, sq, S):
    """Tol-M2-sharp from the reference's M2 and sum_s ll_is^2."""
    return C_M2 * (S + 64) * U * (M2 + numpy.sqrt(sq) * numpy.sqrt(M2))


def ratios(partial, ll):
    """(max err / Tol-lppd, max err / Tol-M2-sharp, per-observation arrays of both) of a merged
    [5, n_obs] partial against the longdouble reference over ll[S, n_obs].  A zero tolerance
    (every ll of an observation identical: M2 = 0) asks for a zero error."""
    from nestmc import waic
    lppd, M2, sq, _ = reference(ll)
    S = numpy.asarray(ll).shape[0]
    res = waic.finish(partial, [0, partial.shape[1]])
    assert res.n_samples == S, (res.n_samples, S)
    err_l = numpy.abs(res.lppd_i.astype(numpy.longdouble) - lppd)
    err_m = numpy.abs(numpy.asarray(partial[4]).astype(numpy.longdouble) - M2)
    tl, tm = tol_lppd(lppd, S), tol_m2_sharp(M2, sq, S)
    with numpy.errstate(invalid="ignore", divide="ignore"):
        rl = numpy.asarray(err_l / tl, dtype=float)
        rm = numpy.asarray(numpy.where(tm > 0, err_m / tm, numpy.where(err_m > 0, numpy.inf, 0)),
                           dtype=float)
    return float(numpy.max(rl)), float(numpy.max(rm)), rl, rm


def _dev_merge(A, B, mutant=None):
    """nmc_waic_merge (csrc/waic.h) on arrays of states (m, s, n, mean, M2)."""
    mA, sA, nA, meanA, M2A = A
    mB, sB, nB, meanB, M2B = B
    m = numpy.fmax(mA, mB)
    if mutant == "n0":   # (empty is told by m, not by n)
        ta = numpy.where(mA > -numpy.inf, sA * numpy.exp(mA - m), 0.0)
        tb = numpy.where(mB > -numpy.inf, sB * numpy.exp(mB - m), 0.0)
    else:
        ta = numpy.where(nA > 0.0, sA * numpy.exp(mA - m), 0.0)
        tb = numpy.where(nB > 0.0, sB * numpy.exp(mB - m), 0.0)
    s = ta + tb
    n = nA + nB
    d = meanB - meanA
    some = n > 0.0
    mean = numpy.where(some, meanA + d * nB / n, 0.0)
    M2 = numpy.where(some, M2A + M2B + d * d * nA * nB / n, 0.0)
    return m, s, n, mean, M2


def restate_parts(ll, C, n_valid, mutant=None):
    """nmc_k_waic over ll[chains >= n_valid][R][n_obs] (Engine.obs_ll_rows' layout, float64) for
    an engine of C chains: the chain blocks' partials [CB, 5, n_obs].

    mutant: None, or one of the errors the tolerances must catch --
      "naive"      a lane's variance as sum x^2 - (sum x)^2 / R in one pass,
      "norescale"  s + 1 in place of s e + 1 at a new maximum,
      "n0"         padding chains' (m, s) enter the merge with n = 0 and the merge tells an
                   empty side by m = -inf, not by n = 0 (a lane past n_valid holds the state
                   of its own chain)."""
    ll = numpy.asarray(ll, dtype=numpy.float64)
    nc, R, n_obs = ll.shape
    CB = (C + 63) // 64
    assert n_valid <= C and (nc >= n_valid if mutant != "n0" else nc >= C)
    lanes = CB * 64
    x_all = numpy.zeros((lanes, R, n_obs))
    x_all[:min(nc, lanes)] = ll[:lanes]
    valid = numpy.arange(lanes) < n_valid
    with numpy.errstate(all="ignore"):
        m = numpy.full((lanes, n_obs), -numpy.inf)
        s = numpy.zeros((lanes, n_obs))
        mean = numpy.zeros((lanes, n_obs))
        M2 = numpy.zeros((lanes, n_obs))
        sx = numpy.zeros((lanes, n_obs))
        sxx = numpy.zeros((lanes, n_obs))
        for r in range(R):
            x = x_all[:, r]
            ik = 1.0 / float(r + 1)
            dm = x - m
            e = numpy.exp(-numpy.abs(dm))
            grow = s + 1.0 if mutant == "norescale" else s * e + 1.0
            s = numpy.where(dm <= 0.0, s + e, grow)
            m = numpy.fmax(m, x)
            dl = x - mean
            mean = mean + dl * ik
            M2 = M2 + dl * (x - mean)
            sx = sx + x
            sxx = sxx + x * x
        if mutant == "naive":
            mean, M2 = sx / float(R), sxx - sx * sx / float(R)
        v = valid[:, None]
        keep = (numpy.arange(lanes) < C)[:, None] if mutant == "n0" else v
        st = (numpy.where(keep, m, -numpy.inf), numpy.where(keep, s, 0.0),
              numpy.where(v, float(R), 0.0) * numpy.ones((lanes, n_obs)),
              numpy.where(v, mean, 0.0), numpy.where(v, M2, 0.0))
        st = tuple(a.reshape(CB, 64, n_obs) for a in st)
        for _ in range(6):   # lane ^ 1, ^ 2, ... ^ 32: a balanced tree, the lower lane is A
            st = _dev_merge(tuple(a[:, 0::2] for a in st), tuple(a[:, 1::2] for a in st), mutant)
    return numpy.ascontiguousarray(numpy.stack([a[:, 0] for a in st], axis=1))


def restate(ll, C, n_valid, mutant=None):
    """The merged [5, n_obs] partial: restate_parts through nestmc.waic.merge."""
    from nestmc import waic
    parts = restate_parts(ll, C, n_valid, mutant)
    if mutant == "n0":   # (the host merge of the same error: blocks added whatever their n)
        acc = tuple(parts[0])
        with numpy.errstate(all="ignore"):
            for p in parts[1:]:
                acc = _dev_merge(acc, tuple(p), mutant)
        return numpy.stack(acc)
    return waic.merge(list(parts))
