"""The checker of tests/test_gpu_gibbs_order.py, and a numpy model of the Gibbs update with a
summation order of choice (tests/test_gibbs_order_check.py runs the checker on it: numpy's
order passes, a sequential sum fails at every G >= 8)."""

import numpy
import scipy.special

from oracle import restatement as rs


def sums(a):
    """numpy.sum of every row of a [C, G] (each a contiguous 1-D array: numpy's pairwise
    order) and the rows' sequential sums."""
    a = numpy.ascontiguousarray(a)
    return (numpy.array([numpy.sum(a[c]) for c in range(a.shape[0])]),
            numpy.cumsum(a, axis=1)[:, -1])


def check(rows, s2_start, hz, hu, G, P, what):
    """rows [C, n, cols]: recorded partial-pooling rows of consecutive iterations from the
    start (burn 0, thin 1); s2_start [C, P]; hz [C, n, P] the hyper mean's normal variates;
    hu [n, P] the uniform every chain's inverse-gamma draw replays.  Asserts for every (row,
    parameter), from the row's own mu, s2 and values x:
      mu == numpy.sum(x) / G + numpy.sqrt(s2_prev / G) * hz              bit for bit
      s2 == r * (a * (numpy.sum((x - mu)**2) / (G - 1))), a = (G - 1) / 2  bit for bit
    with one double r for all chains, within 1e-12 + 2 ulp of 1 / gammainccinv(a, u).
    Returns the share of the checked sums that differ from their sequential sum."""
    C, n = rows.shape[0], rows.shape[1]
    a = (G - 1) / 2.0
    differ = []
    for i in range(n):
        for p in range(P):
            o = p * (G + 2)
            mu, s2, x = rows[:, i, o], rows[:, i, o + 1], rows[:, i, o + 2:o + 2 + G]
            s2_prev = rows[:, i - 1, o + 1] if i else s2_start[:, p]
            assert numpy.all(numpy.isfinite(mu)) and numpy.all(s2 > 0), (what, i, p)
            tot, seq = sums(x)
            differ.append(tot != seq)
            for c in range(C):
                assert rs.pairwise_sum(x[c]) == tot[c], (what, i, p, c)
            want = tot / G + numpy.sqrt(s2_prev / G) * hz[:, i, p]
            bad = numpy.argwhere(mu != want)
            assert bad.size == 0, ("hyper mean", what, i, p, bad[:5].ravel(),
                                   mu[bad[0, 0]], want[bad[0, 0]])
            d = x - mu[:, None]
            ss, seq = sums(d * d)
            differ.append(ss != seq)
            scale = a * (ss / (G - 1))
            up = dn = s2[0] / scale[0]
            cand = [up]
            for _ in range(8):
                up, dn = numpy.nextafter(up, numpy.inf), numpy.nextafter(dn, -numpy.inf)
                cand += [up, dn]
            ok = [r for r in cand if numpy.array_equal(r * scale, s2)]
            assert ok, ("no single 1 / hx gives every chain's s2", what, i, p,
                        [int((r * scale != s2).sum()) for r in cand[:3]])
            ref = 1.0 / scipy.special.gammainccinv(a, hu[i, p])
            for r in ok:
                assert abs(r / ref - 1.0) <= 1e-12 + 2 * 2.0 ** -52, (what, i, p, r, ref)
    return float(numpy.mean(numpy.concatenate(differ)))


def start(C, P, G, seed):
    """(value [C, P, G] of spread magnitudes, mu, s2 [C, P])."""
    r = numpy.random.RandomState(seed)
    mu = r.normal(size=(C, P))
    s2 = r.uniform(0.2, 1.0, size=(C, P))
    value = r.normal(size=(C, P, G)) * numpy.exp(2.0 * r.normal(size=(C, P, G)))
    return value, mu, s2


def variates(C, P, G, n, seed):
    """Replay variates (z, u [C, n, P, G]; hz [C, n, P]; hu [n, P], one per (row, parameter)
    for every chain)."""
    r = numpy.random.RandomState(seed + 1)
    return (r.normal(size=(C, n, P, G)), r.uniform(size=(C, n, P, G)), r.normal(size=(C, n, P)),
            r.uniform(0.02, 0.98, size=(n, P)))


def model_rows(value, s2, hz, hu, summer, igamci_error=3e-13):
    """Rows a device would record whose values never move (every proposal rejected) and whose
    Gibbs update sums with ``summer`` (a function of a 1-D array); its inverse incomplete
    gamma is off by igamci_error relative."""
    C, P, G = value.shape
    n = hz.shape[1]
    a = (G - 1) / 2.0
    rows = numpy.empty((C, n, P * (G + 2)))
    s2 = s2.copy()
    for i in range(n):
        for p in range(P):
            x = value[:, p, :]
            tot = numpy.array([summer(x[c]) for c in range(C)])
            mu = tot / G + numpy.sqrt(s2[:, p] / G) * hz[:, i, p]
            d = x - mu[:, None]
            ss = numpy.array([summer((d * d)[c]) for c in range(C)])
            hx = scipy.special.gammainccinv(a, hu[i, p]) * (1.0 + igamci_error)
            s2[:, p] = (1.0 / hx) * (a * (ss / (G - 1)))
            o = p * (G + 2)
            rows[:, i, o], rows[:, i, o + 1], rows[:, i, o + 2:o + 2 + G] = mu, s2[:, p], x
    return rows
