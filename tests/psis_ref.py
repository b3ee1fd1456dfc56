"""The reference, the inputs and the tolerances of the PSIS-LOO tests.

``column(ll, dtype)`` restates nestmc/loo.py's formulas in numpy with a dtype parameter.  The
raw log-weights r = min(ll) - ll and the cutoff are float64 numbers by definition (loo.py:
the tail's membership is discrete), so n_tail and cut are compared EXACTLY; everything after
them runs in ``dtype``.  The reference is the longdouble evaluation on the float64 inputs.

u = 2^-52, n2 = n_tail.

  Tol-k    |k - ref|       <= C n2 u (1 + |ref|)     the shape of a sequential-sum bound over
  Tol-lw   |lw_j - ref_j|  <= C n2 u (1 + |ref_j|)   the n2 tail terms
           C is measured, not chosen: the worst ratio err / (n2 u (1 + |ref|)) of the float64
           evaluation column(ll, float64) against the longdouble one over every column of
           ``cases()`` (all the shapes of the tests), k and the smoothed log-weights together,
           was 0.934 on the CPU (column "floor_a" of the S = 4160 store: a smoothed
           log-weight); C is the least power of two >= 8 x that = 8.  The factor 8 covers the
           device's exp / log1p / expm1 differing from numpy's by a few ulp and its reduction
           order.  (``python tests/psis_ref.py`` prints the measurement.  The columns of the
           Engine.loo tests are the device's own log-likelihoods and exist on a GPU only; the
           device's error on them was at most 0.42 n2 u (1 + |ref|), inside the measured
           worst.)
  Tol-elpd |elpd_i - ref|  <= (S + 64) u (1 + |ref|) + E_w
  Tol-lppd |lppd_i - ref|  <= (S + 64) u (1 + |ref|)
           the first term is waic_ref's Tol-lppd argument (a sequential sum of S positive
           terms, exp's ulp and its argument's rounding).  E_w propagates Tol-lw: elpd =
           log sum exp(lw + ll) - log sum exp(lw), so d elpd / d lw_j = pn_j - pd_j with
           pn, pd the two sums' normalised terms; a change of at most d in every tail weight
           moves elpd by at most d (sum_tail pn_j + sum_tail pd_j) <= 2 d:
             E_w = 2 max_j C n2 u (1 + |lw_ref_j|)       (0 for a short tail, and for lppd)

An observation whose k is +inf (short tail) must give +inf exactly.
"""

import numpy

U = 2.0 ** -52
C_TAIL = 8.0
LOG_TINY = float(numpy.log(numpy.finfo(numpy.float64).tiny))
EPS = float(numpy.finfo(numpy.float64).eps)


def tail_length(S):
    return int(numpy.ceil(min(S / 5.0, 3.0 * numpy.sqrt(float(S)))))


def column(ll, dtype=numpy.longdouble):
    """dict(elpd, lppd, k, n_tail, cut, lw_tail) of one observation's values, in dtype."""
    T = dtype
    a64 = numpy.sort(numpy.asarray(ll, dtype=numpy.float64))
    S = len(a64)
    M = tail_length(S)
    r64 = a64[0] - a64
    cut64 = max(float(r64[M]), LOG_TINY)
    n2 = int(numpy.sum(r64[:M] > cut64))
    a, lw = a64.astype(T), r64.astype(T)
    k = T(numpy.inf)
    lw_tail = numpy.empty(0, dtype=T)
    with numpy.errstate(all="ignore"):
        if n2 > 4:
            ecut = numpy.exp(T(cut64))
            x = numpy.exp(lw[:n2][::-1]) - ecut
            m = 30 + int(numpy.sqrt(n2))
            b = T(1) - numpy.sqrt(T(m) / (numpy.arange(1, m + 1).astype(T) - T(0.5)))
            b = b / (T(3) * x[int(n2 / 4.0 + 0.5) - 1])
            b = b + T(1) / x[-1]
            kj = numpy.sum(numpy.log1p(-b[:, None] * x), axis=1) / T(n2)
            L = T(n2) * (numpy.log(-b / kj) - kj - T(1))
            w = T(1) / numpy.sum(numpy.exp(L - L[:, None]), axis=1)
            keep = w >= T(10.0 * EPS)
            w = w[keep] / numpy.sum(w[keep])
            bb = numpy.sum(b[keep] * w)
            k1 = numpy.sum(numpy.log1p(-bb * x)) / T(n2)
            sigma = -k1 / bb
            k = (T(n2) * k1 + T(5)) / (T(n2) + T(10))
            l1 = numpy.log1p(-(numpy.arange(n2).astype(T) + T(0.5)) / T(n2))
            q = -sigma * l1 if abs(k) < EPS else sigma * numpy.expm1(-k * l1) / k
            lw_tail = numpy.minimum(numpy.log(q + ecut), T(0))
            lw[:n2] = lw_tail[::-1]
        t = lw + a
        mn, md = numpy.max(t), numpy.max(lw)
        elpd = (mn + numpy.log(numpy.sum(numpy.exp(t - mn)))) \
            - (md + numpy.log(numpy.sum(numpy.exp(lw - md))))
        lppd = a[-1] + numpy.log(numpy.sum(numpy.exp(a - a[-1])) / T(S))
    return dict(elpd=elpd, lppd=lppd, k=k, n_tail=n2, cut=cut64, lw_tail=lw_tail)


_REF = {}


def reference(name, ll):
    """column(ll, longdouble), computed once per named column and shared."""
    if name not in _REF:
        _REF[name] = column(ll, numpy.longdouble)
    return _REF[name]


def tolerances(ref, S):
    n2 = ref["n_tail"]
    fit = len(ref["lw_tail"]) > 0
    tol_k = C_TAIL * n2 * U * (1 + abs(ref["k"])) if fit else 0.0
    tol_lw = C_TAIL * n2 * U * (1 + numpy.abs(ref["lw_tail"]))
    e_w = 2 * float(numpy.max(tol_lw)) if fit else 0.0
    tol_l = (S + 64) * U * (1 + abs(ref["lppd"]))
    tol_e = (S + 64) * U * (1 + abs(ref["elpd"])) + e_w
    return tol_k, tol_lw, tol_e, tol_l


def check(name, ll, elpd, lppd, k, n_tail, cut=None, lw_tail=None, what=""):
    """One observation against its longdouble reference; cut and lw_tail where the route
    under test returns them (the host route).  Prints the ratios error / tolerance first."""
    ref = reference(name, ll)
    S = len(ll)
    tol_k, tol_lw, tol_e, tol_l = tolerances(ref, S)
    L = numpy.longdouble
    err_e, err_l = abs(L(elpd) - ref["elpd"]), abs(L(lppd) - ref["lppd"])
    fit = len(ref["lw_tail"]) > 0
    err_k = abs(L(k) - ref["k"]) if fit else 0.0
    rk = float(err_k / tol_k) if fit else 0.0
    rw = 0.0
    if fit and lw_tail is not None and len(lw_tail) == len(ref["lw_tail"]):
        rw = float(numpy.max(numpy.abs(numpy.asarray(lw_tail).astype(L) - ref["lw_tail"])
                             / tol_lw))
    print("psis check %s %s: S=%d n_tail=%d k=%.6g  err/Tol: elpd %.3g lppd %.3g k %.3g lw %.3g"
          % (what, name, S, n_tail, float(k), float(err_e / tol_e), float(err_l / tol_l), rk, rw))
    assert int(n_tail) == ref["n_tail"], (what, name, "n_tail", n_tail, ref["n_tail"])
    if cut is not None:
        assert float(cut) == ref["cut"], (what, name, "cut", cut, ref["cut"])
    if fit:
        assert err_k <= tol_k, (what, name, "k", float(k), float(ref["k"]), rk)
        if lw_tail is not None:
            assert len(lw_tail) == len(ref["lw_tail"]), (what, name, "lw_tail length")
            assert rw <= 1.0, (what, name, "lw", rw)
    else:
        assert numpy.isposinf(k), (what, name, "k of a short tail", k)
        if lw_tail is not None:
            assert len(lw_tail) == 0
    assert err_e <= tol_e, (what, name, "elpd", float(elpd), float(ref["elpd"]))
    assert err_l <= tol_l, (what, name, "lppd", float(lppd), float(ref["lppd"]))
    return ref


# ---- the inputs ----------------------------------------------------------------------------
def _finite_columns(S, seed):
    """The named finite columns of S values (ll, in sample order s = row * n_valid + chain)."""
    r = numpy.random.RandomState(seed)
    M = tail_length(S)
    out = {}
    out["gauss"] = -0.5 * r.normal(size=S) ** 2 - 0.9
    out["t3"] = r.standard_t(3, size=S)                       # k > 0.7
    out["uniform"] = -numpy.log(r.uniform(1.0, 2.0, size=S))  # bounded ratios: k < 0
    out["equal"] = numpy.full(S, -1.25)                       # n2 = 0, k = inf
    a = numpy.sort(r.normal(size=S))
    a[M - 10:M + 20] = a[M]          # ties at the cutoff reach 10 places into the head
    out["ties"] = r.permutation(a)
    a = numpy.full(S, -0.5)
    a[:3] = [-3.0, -2.0, -1.0]       # three values above the cutoff: a short tail
    out["three"] = r.permutation(a)
    out["floor"] = 600.0 * r.normal(size=S)                   # the cutoff at log(DBL_MIN)
    return out


_CASES = {}


def cases():
    """{store name: (rows, C, n_valid, {column name: ll[S]})}: every shape of the tests, built
    once.  The last store's M = 7 800 tail candidates take 62 400 bytes of dynamic LDS, with the
    kernel's static 3 328 more than the 64 KiB a launch has without a raised limit."""
    if not _CASES:
        big = _finite_columns(64 * 66, 11)
        small = {k: v for k, v in _finite_columns(30, 12).items()
                 if k in ("gauss", "t3", "uniform")}
        pad = {k + "_a": v for k, v in _finite_columns(64 * 65, 13).items()
               if k in ("gauss", "t3", "floor")}
        r = numpy.random.RandomState(14)
        huge = {"gauss_h": -0.5 * r.normal(size=6600 * 1024) ** 2 - 0.9}
        _CASES.update({"s4224": (64, 66, 66, big), "s30": (10, 3, 3, small),
                       "s4160": (64, 128, 65, pad), "s6758400": (6600, 1024, 1024, huge)})
    return _CASES


def store(rows, C, n_valid, columns, pad=numpy.nan):
    """ll[rows][n_obs][C] in the sample store's layout: column i's value s = q * n_valid + c at
    [q][i][c]; the chains from n_valid on hold ``pad`` (they must never be read)."""
    out = numpy.full((rows, len(columns), C), pad)
    for i, v in enumerate(columns):
        out[:, i, :n_valid] = numpy.asarray(v).reshape(rows, n_valid)
    return out


def measure_c():
    """The worst err / (n2 u (1 + |ref|)) of float64 against longdouble over cases()."""
    worst, where = 0.0, None
    for sname, (rows, C, nv, cols) in cases().items():
        for cname, ll in cols.items():
            ref, got = column(ll, numpy.longdouble), column(ll, numpy.float64)
            assert got["n_tail"] == ref["n_tail"] and got["cut"] == ref["cut"]
            if len(ref["lw_tail"]) == 0:
                continue
            n2 = ref["n_tail"]
            rk = float(abs(got["k"] - ref["k"]) / (n2 * U * (1 + abs(ref["k"]))))
            rw = float(numpy.max(numpy.abs(got["lw_tail"] - ref["lw_tail"])
                                 / (n2 * U * (1 + numpy.abs(ref["lw_tail"])))))
            print("%s %s: n2=%d k=%.6g  ratio k %.3g  lw %.3g" % (sname, cname, n2,
                                                               float(ref["k"]), rk, rw))
            if max(rk, rw) > worst:
                worst, where = max(rk, rw), (sname, cname)
    c = 2.0 ** numpy.ceil(numpy.log2(8 * worst))
    print("worst ratio %.3g at %s -> C = %g" % (worst, where, c))
    return worst, c


if __name__ == "__main__":
    measure_c()
