"""The reference, the inputs and the tolerances of the LOO-PIT tests.

``column(ll, yrep, y, dtype)`` restates nestmc/loopit.py's formulas in numpy on top of
``psis_ref.column``: the tail's membership (r > cut) and the ties (ll == ll) are float64
comparisons by definition, everything after them runs in ``dtype``.  The reference is the
longdouble evaluation on the float64 inputs.

Tolerances, derived, with u = 2^-52, S the samples, delta = max_j Tol-lw_j of
``psis_ref.tolerances`` (0 for a short tail) and Y = max_s |y_rep_s|:

  Tol-pit   |wlt|, |weq|, |loo_pit - ref|  <= 2 (S + 64) u + delta
  Tol-mean  |loo_mean - ref|               <= (2 (S + 64) u + 2 delta) Y
  Tol-var   |loo_var - ref|                <= (2 (S + 64) u + 2 delta) 4 Y^2 + 4 Y Tol-mean
  Tol-ess   |ess - ref|                    <= (4 (S + 64) u + 4 delta) ess

Each quantity is a ratio of two sums of S non-negative (or, for the mean, Y-bounded) terms:
each sum carries the sequential-sum bound (S + 64) u of psis_ref's Tol-lppd argument (exp's
ulp and its argument's rounding in the 64), hence the 2 (4 for ess: a squared sum over a sum
of squares).  A change of at most delta in every tail log-weight moves a normalised weighted
indicator sum by at most delta times the tail's normalised weight, <= delta (d pit / d lw_j is
at most the normalised weight); the mean's numerator and denominator both move, 2 delta Y;
(y_rep - mean)^2 <= 4 Y^2, and an error e in the mean moves the variance by at most 4 Y e.

The float64 numpy evaluation against longdouble reached at most 0.002 of Tol-pit, 0.0009 of
Tol-mean, 0.00009 of Tol-var and 0.0015 of Tol-ess (``python tests/loopit_ref.py`` prints the
measurement).

Exact requirements: n_tail; a column of equal ll gives loo_pit == (lt + eq / 2) / S and
ess == S; y_rep == y everywhere gives loo_pit == 0.5; swapping the replicates of tied tail
samples changes no bit (the tests that own the route under test do the swap).
"""

import numpy

import psis_ref

U = psis_ref.U
STORES = ("s4224", "s30", "s4160")
KINDS = ("normal", "binary", "same")


def column(ll, yrep, y, dtype=numpy.longdouble, psis=None):
    """dict(ess, wlt, weq, pit, mean, var, w (normalised, sample order), n_tail) in dtype;
    psis: psis_ref.column(ll, dtype) if the caller has it."""
    T = dtype
    ll64 = numpy.asarray(ll, dtype=numpy.float64)
    col = psis if psis is not None else psis_ref.column(ll64, T)
    lw_tail = col["lw_tail"]
    n2 = len(lw_tail)
    r64 = numpy.min(ll64) - ll64
    with numpy.errstate(all="ignore"):
        if n2 == 0:
            w = numpy.exp(r64.astype(T))
        else:
            order = numpy.argsort(ll64, kind="stable")[:n2 + 1]       # the head and the body's first
            a = ll64[order]
            D = max(T(a[0] - a[n2]), numpy.max(lw_tail))
            w = numpy.exp(r64.astype(T) - D)
            e = numpy.exp(lw_tail - D)
            w[order[:n2]] = e[::-1]                                   # position p: place n2 - 1 - p
            start = numpy.flatnonzero(numpy.concatenate([[True], a[1:n2] != a[:n2 - 1]]))
            stop = numpy.concatenate([start[1:], [n2]])
            for p0, p1 in zip(start, stop):
                if p1 - p0 > 1:                                       # ties: places [n2 - p1, n2 - p0)
                    w[order[p0:p1]] = numpy.sum(e[n2 - p1:n2 - p0]) / T(p1 - p0)
        yr = numpy.asarray(yrep, dtype=numpy.float64).astype(T)
        Z = numpy.sum(w)
        mean = numpy.sum(w * yr) / Z
        wlt, weq = numpy.sum(w[yr < y]) / Z, numpy.sum(w[yr == y]) / Z
        out = dict(ess=Z * Z / numpy.sum(w * w), wlt=wlt, weq=weq, pit=wlt + weq / T(2),
                   mean=mean, var=numpy.sum(w * (yr - mean) ** 2) / Z, w=w / Z,
                   n_tail=col["n_tail"])
    return out


def tolerances(ref, psis, S, yrep):
    """(Tol-pit, Tol-mean, Tol-var, Tol-ess) of one column and replicate vector."""
    _, tol_lw, _, _ = psis_ref.tolerances(psis, S)
    delta = float(numpy.max(tol_lw)) if len(psis["lw_tail"]) > 0 else 0.0
    Y = float(numpy.max(numpy.abs(yrep)))
    s = 2 * (S + 64) * U
    tol_pit = s + delta
    tol_mean = (s + 2 * delta) * Y
    tol_var = (s + 2 * delta) * 4 * Y * Y + 4 * Y * tol_mean
    tol_ess = (2 * s + 4 * delta) * float(ref["ess"])
    return tol_pit, tol_mean, tol_var, tol_ess


# ---- the inputs ----------------------------------------------------------------------------
_CASES = {}


def cases():
    """{store: (rows, C, n_valid, {column: ll[S]})}: psis_ref's finite columns of the three
    small stores, and in the first a column with five equal values INSIDE the tail (psis_ref's
    "ties" sit at the cutoff and never enter it)."""
    if not _CASES:
        for s in STORES:
            rows, C, nv, cols = psis_ref.cases()[s]
            _CASES[s] = (rows, C, nv, dict(cols))
        rows, C, nv, cols = _CASES["s4224"]
        r = numpy.random.RandomState(21)
        a = numpy.sort(cols["gauss"])
        a[20:25] = a[22]                       # positions 20..24 of M = 195: tail places
        cols["tail5"] = r.permutation(a)
        # (not in STORES: one column whose M = 7 800 takes 124 800 bytes of dynamic LDS in
        # nmc_k_psis_expect, past the 64 KiB a launch has without a raised limit)
        _CASES["s6758400"] = psis_ref.cases()["s6758400"]
    return _CASES


def replicates(sname, cname, S):
    """{kind: (yrep[S], y)}: normal draws, {0, 1} draws with y = 1, and y_rep == y."""
    seed = (sum(map(ord, sname + cname)) * 7919) % (2 ** 31)
    r = numpy.random.RandomState(seed)
    return {"normal": (0.4 + 1.7 * r.normal(size=S), 0.9),
            "binary": ((r.uniform(size=S) < 0.3).astype(numpy.float64), 1.0),
            "same": (numpy.full(S, -2.5), -2.5)}


_REF = {}


def reference(sname, cname, kind):
    """(column(...) in longdouble, the psis_ref reference, yrep, y), computed once and shared."""
    key = (sname, cname, kind)
    if key not in _REF:
        ll = cases()[sname][3][cname]
        psis = psis_ref.reference(sname + "/" + cname, ll)
        yrep, y = replicates(sname, cname, len(ll))[kind]
        _REF[key] = (column(ll, yrep, y, numpy.longdouble, psis), psis, yrep, y)
    return _REF[key]


def check(sname, cname, kind, got, what=""):
    """got: dict(ess, wlt, weq, mean, var, n_tail) of one observation against the reference of
    a named column and replicate kind.  Prints the ratios error / tolerance first; returns
    them."""
    ref, psis, yrep, y = reference(sname, cname, kind)
    return check_values("%s/%s/%s" % (sname, cname, kind), cases()[sname][3][cname], yrep, y, got,
                        what, ref, psis)


def check_values(name, ll, yrep, y, got, what="", ref=None, psis=None):
    """The same for any column ll[S] with replicates yrep[S] and the observed y (the engine
    tests: the device's own log-likelihoods and draws)."""
    if ref is None:
        psis = psis_ref.reference(name, ll)
        ref = column(ll, yrep, y, numpy.longdouble, psis)
    S = len(yrep)
    tp, tm, tv, te = tolerances(ref, psis, S, yrep)
    L = numpy.longdouble
    pit = L(got["wlt"]) + L(got["weq"]) / 2
    err = dict(wlt=abs(L(got["wlt"]) - ref["wlt"]) / tp, weq=abs(L(got["weq"]) - ref["weq"]) / tp,
               pit=abs(pit - ref["pit"]) / tp, mean=abs(L(got["mean"]) - ref["mean"]) / tm,
               var=abs(L(got["var"]) - ref["var"]) / tv, ess=abs(L(got["ess"]) - ref["ess"]) / te)
    err = {k: float(v) for k, v in err.items()}
    print("loopit check %s %s: S=%d n_tail=%d  err/Tol: %s"
          % (what, name, S, ref["n_tail"], " ".join("%s %.3g" % kv for kv in err.items())))
    assert int(got["n_tail"]) == ref["n_tail"], (what, name, "n_tail")
    for k, v in err.items():
        assert v <= 1.0, (what, name, k, v)
    ll = numpy.asarray(ll)
    if numpy.all(ll == ll[0]):
        lt, eq = numpy.sum(yrep < y), numpy.sum(yrep == y)
        assert got["wlt"] + got["weq"] / 2.0 == (lt + eq / 2.0) / S, (what, name)
        assert got["ess"] == S, (what, name, got["ess"])
    if numpy.all(numpy.asarray(yrep) == y):
        assert got["wlt"] + got["weq"] / 2.0 == 0.5, (what, name, got["wlt"], got["weq"])
    return err


def all_columns():
    """[(store, column, kind)] of every check."""
    return [(s, c, k) for s in STORES for c in cases()[s][3] for k in KINDS]


def measure():
    """The worst err / Tol of the float64 numpy restatement against longdouble."""
    worst = {}
    for s, c, k in all_columns():
        ll = cases()[s][3][c]
        yrep, y = replicates(s, c, len(ll))[k]
        got = column(ll, yrep, y, numpy.float64)
        err = check(s, c, k, {f: float(got[f]) if f != "n_tail" else got[f]
                              for f in ("ess", "wlt", "weq", "mean", "var", "n_tail")},
                    what="float64")
        for f, v in err.items():
            worst[f] = max(worst.get(f, 0.0), v)
    print("worst err / Tol of float64 numpy: " + " ".join("%s %.3g" % kv for kv in worst.items()))
    return worst


if __name__ == "__main__":
    measure()
