"""The references of the posterior predictive tests (tests/test_ppc_host.py on the CPU,
tests/test_gpu_ppc.py on the device), on the stores of tests/store_cases.py.  numpy only.

``draws(name)``      the replicates of a case's store: the stream of csrc/ppc.h restated with
                     oracle.philox -- one block per (row r, observation i, field j, chain),
                     counter (r, i, j, purpose 4), key (chain_base + chain, seed), z its
                     Box-Muller normal (numpy's log and cos, float64) -- and the family's formula
                     in numpy.longdouble on the float64 store.
``restate(...)``     nmc_k_ppc_obs and nmc_k_ppc_group (+ nmc_k_ppc_group_fin) in float64,
                     operation by operation: Welford's recurrences, the 64-lane butterfly (the
                     lower lane the A operand), for the groups the rows dealt to four waves,
                     the waves merged 0..3 and the row slices 0..NS-1 (nestmc.ppc.group_slices);
                     the chain blocks are left to nestmc.ppc.merge.  IEEE + - x / only: on the
                     same replicates every word is the device's.
``reference(...)``   the same quantities in longdouble, by the two-pass formulas.

Tolerances.  u = 2^-52, S samples.
  draws   Gaussian families: |dev - ref| <= (K + 3) 2^-53 A + 1e-14 |s z|, A = the sum of the
          absolute addends of yhat plus |s z| (K products, K additions with the intercept's, the
          product s z and the last addition: below K + 3 roundings of at most 2^-53 A each;
          1e-14 is the agreement the project holds between the device's and numpy's z, rng.h).
          Logistic: equal everywhere, which needs |ua - p| above the error of p (a few ulp of
          p <= 1: 1e-15) -- test_ppc_host.py holds min |ua - p| > 1e-12 on the case.
  mean    |mean - ref| <= (S + 64) u max |x|        (S - 1 updates of Welford's mean, each
          within u of max |x|, and the merges' 6 + CB)
  M2      Tol-M2 of tests/waic_ref.py, (S + 64) u sum x^2: the same recurrence and merge.
For the group states x is the float64 statistic T(y_rep) the reduction is handed (``t_stats``,
the device's function word for word): what the tolerances bound is the reduction over the
samples.  T itself is held against longdouble through the counts: a comparison of T(y_rep)
with T(y) must come out as in longdouble unless the two are closer than the float64 T's own
error, ``t_bound``:
  mean    (n + 2) u max |x|
  var     Tol-M2-sharp of waic_ref over the group's n values, divided by n
  min, max  exact: 0
Two sides that are EQUAL in longdouble are not left out: the float64 statistics must say equal
too.  For a response with integer values (the logistic's 0 / 1) such ties are a tenth and more
of all comparisons and equal sums are equal in every precision; Welford's mean would decide
them by the order of the values (which is why csrc/ppc.h takes the sums there, RESP_INT).
"""

import functools

import numpy

import store_cases as sc
import waic_ref
from nestmc import ppc
from oracle import philox

LD = numpy.longdouble
U = 2.0 ** -52
SEED = 1                 # the engines of the store tests are made with seed = 1
PURPOSE_PREDICT = 4      # csrc/rng.h NMC_PURPOSE_PREDICT


MISFIT_GROUP, MISFIT_SHIFT = 3, 5.0


@functools.lru_cache(maxsize=None)
def case_of(name):
    """A case of store_cases by name, or "misfit": the ``ties`` store (every sample at the
    groups' least-squares lines) with the y of group 3 raised by 5 noise sd."""
    if name != "misfit":
        return sc.BY_NAME[name]
    y = sc.Y_LIN.copy()
    y[sc.OFF[MISFIT_GROUP]:sc.OFF[MISFIT_GROUP + 1]] += MISFIT_SHIFT
    from nestmc.families import LinearRegression
    return sc.BY_NAME["ties"]._replace(name="misfit",
                                       fam=LinearRegression.simple(sc.X_LIN, y, sigma=1.0))


def resp_fields(case):
    return list(case.fam.response_fields())


def y_of(case):
    """The observed response fields [n_obs, NRESP]."""
    return numpy.ascontiguousarray(numpy.asarray(case.fam.obs())[:, resp_fields(case)])


def variates(n_resp, chain_base=0, n_chains=sc.C, rows=None, seed=SEED):
    """(ua, ub, z), each [C][R][n_obs][NRESP] float64."""
    rows = numpy.arange(sc.R) if rows is None else numpy.asarray(rows)
    c = (chain_base + numpy.arange(n_chains))[:, None, None, None]
    r = rows[None, :, None, None]
    i = numpy.arange(sc.N_OBS)[None, None, :, None]
    j = numpy.arange(n_resp)[None, None, None, :]
    ua, ub = philox.uniforms(r, i, j, PURPOSE_PREDICT, c, seed)
    return ua, ub, philox.box_muller(ua, ub)


@functools.lru_cache(maxsize=None)
def draws(name):
    """A dict of yrep, tol [C][R][n_obs][NRESP] (longdouble / float64; tol is the draws'
    tolerance, 0 for the logistic), z, ua, and for the logistic gap = |ua - p|."""
    case = case_of(name)
    NR = len(resp_fields(case))
    ua, ub, z = variates(NR)
    th = numpy.transpose(sc.theta_of(case), (1, 0, 2, 3)).astype(LD)[:, :, :, sc.GRP]  # [C][R][P][n]
    obs = numpy.asarray(case.fam.obs()).astype(LD)
    zl = z.astype(LD)
    out = dict(z=z, ua=ua)
    with numpy.errstate(all="ignore"):
        if case.kind == "gauss":
            sd = sc.SD_GAUSS.astype(LD)[None, None, None, :]
            t = numpy.transpose(th, (0, 1, 3, 2))                       # [C][R][n][P = NRESP]
            sz = sd * zl
            yrep = t + sz
            A, K = numpy.abs(t) + numpy.abs(sz), 0
        else:
            K = case.fam.n_fields - 1
            x = obs[:, :K].T
            b0, b = th[:, :, 0], th[:, :, 1:1 + K]
            eta = (b0 + (b * x[None, None]).sum(axis=2))[..., None]     # [C][R][n][1]
            E = (numpy.abs(b0) + (numpy.abs(b) * numpy.abs(x)[None, None]).sum(axis=2))[..., None]
            if case.kind == "logistic":
                p = 1 / (1 + numpy.exp(-eta))
                yrep = numpy.where(ua.astype(LD) < p, LD(1), LD(0))
                yrep = numpy.where(numpy.isnan(eta), LD(numpy.nan), yrep)
                out["gap"] = numpy.abs(ua.astype(LD) - p).astype(numpy.float64)
                A = sz = numpy.zeros_like(yrep)
            else:
                sig = th[:, :, K + 1][..., None] if case.P == K + 2 else numpy.ones_like(eta)
                ok = sig > 0
                sz = numpy.where(ok, sig, LD(1)) * zl
                yrep = numpy.where(ok, eta + sz, LD(numpy.nan))
                A = E + numpy.abs(sz)
        tol = (K + 3) * 2.0 ** -53 * A + 1e-14 * numpy.abs(sz)
    out["yrep"] = yrep
    out["tol"] = numpy.asarray(numpy.where(numpy.isfinite(tol), tol, 0), dtype=numpy.float64)
    for v in out.values():
        v.setflags(write=False)
    return out


def f64(name):
    """The reference draws rounded to float64 [C][R][n_obs][NRESP]: the replicates the CPU
    tests reduce (the device tests reduce the device's own)."""
    with numpy.errstate(all="ignore"):
        return numpy.asarray(draws(name)["yrep"], dtype=numpy.float64)


# ---------------------------------------------------------------------------------------
# the float64 restatement
# ---------------------------------------------------------------------------------------
def t_stats(x, integer=False):
    """nmc_ppc_T_add and nmc_ppc_T_fin along the last axis, in order -> [..., 4] (mean, var,
    min, max); float64 in, float64 out, every operation the device's.  integer (Fam::RESP_INT):
    the mean and the variance from the sums s1 and s2, else Welford's recurrence."""
    x = numpy.asarray(x, dtype=numpy.float64)
    n = x.shape[-1]
    if integer:
        s1 = numpy.zeros(x.shape[:-1])
        s2 = numpy.zeros(x.shape[:-1])
        with numpy.errstate(all="ignore"):
            for k in range(n):
                s1 = s1 + x[..., k]
                s2 = s2 + x[..., k] * x[..., k]
            mn, mx = numpy.fmin.reduce(x, axis=-1), numpy.fmax.reduce(x, axis=-1)
            nn = float(n)
            return numpy.stack([s1 / nn, (nn * s2 - s1 * s1) / (nn * nn), mn, mx], axis=-1)
    mean = numpy.zeros(x.shape[:-1])
    M2 = numpy.zeros(x.shape[:-1])
    mn = numpy.full(x.shape[:-1], numpy.inf)
    mx = numpy.full(x.shape[:-1], -numpy.inf)
    with numpy.errstate(all="ignore"):
        for k in range(n):
            v = x[..., k]
            dl = v - mean
            mean = mean + dl * (1.0 / float(k + 1))
            M2 = M2 + dl * (v - mean)
            mn = numpy.fmin(mn, v)
            mx = numpy.fmax(mx, v)
        return numpy.stack([mean, M2 / float(n), mn, mx], axis=-1)


def group_stats(yrep, integer=False):
    """T(y_rep) of every (.., group, field): yrep [..., n_obs, NRESP] -> [..., G, NRESP, 4]; a
    sample of a group with a draw that is not finite has four NaN."""
    yrep = numpy.asarray(yrep, dtype=numpy.float64)
    out = []
    for g in range(sc.G):
        seg = numpy.moveaxis(yrep[..., sc.OFF[g]:sc.OFF[g + 1], :], -2, -1)   # [..., NRESP, n]
        t = t_stats(seg, integer)
        bad = ~numpy.all(numpy.isfinite(seg), axis=-1)
        out.append(numpy.where(bad[..., None], numpy.nan, t))
    return numpy.stack(out, axis=-3)


def _dev_merge(A, B):
    """nmc_ppc_merge (csrc/ppc.h) on arrays of states (n, mean, M2)."""
    nA, meanA, M2A = A
    nB, meanB, M2B = B
    with numpy.errstate(all="ignore"):
        n = nA + nB
        d = meanB - meanA
        some = n > 0.0
        mean = numpy.where(some, meanA + d * nB / n, 0.0)
        M2 = numpy.where(some, M2A + M2B + d * d * nA * nB / n, 0.0)
    return n, mean, M2


def _butterfly(st):
    """[CB, 64, ...] states -> [CB, ...]: lane ^ 1, ^ 2, ... ^ 32, the lower lane is A."""
    for _ in range(6):
        st = _dev_merge(tuple(a[:, 0::2] for a in st), tuple(a[:, 1::2] for a in st))
    return tuple(a[:, 0] for a in st)


def _welford_rows(x, rows):
    """A lane's recurrence over x[lanes, rows, ...] at the given rows in order:
    (k, mean, M2) with k the rows' count."""
    mean = numpy.zeros(x.shape[:1] + x.shape[2:])
    M2 = numpy.zeros_like(mean)
    k = 0.0
    with numpy.errstate(all="ignore"):
        for r in rows:
            k = k + 1.0
            ik = 1.0 / k
            v = x[:, r]
            dl = v - mean
            mean = mean + dl * ik
            M2 = M2 + dl * (v - mean)
    return k, mean, M2


def restate(yrep, y, C, n_valid, integer=False):
    """The chain blocks' partials (a list of nestmc.ppc dicts) of an engine of C chains over
    the window's replicates yrep[chains >= n_valid][rows][n_obs][NRESP] (float64); integer: the
    family's response_integer."""
    yrep = numpy.asarray(yrep, dtype=numpy.float64)
    y = numpy.asarray(y, dtype=numpy.float64)
    nc, nrows, n_obs, NR = yrep.shape
    CB = (C + 63) // 64
    lanes = CB * 64
    assert n_valid <= C and nc >= n_valid
    x = numpy.zeros((lanes, nrows, n_obs, NR))
    x[:min(nc, lanes)] = yrep[:lanes]
    valid = numpy.arange(lanes) < n_valid
    sh = lambda a: a.reshape((CB, 64) + a.shape[1:])   # noqa: E731

    def masked(k, mean, M2):
        v = valid.reshape((lanes,) + (1,) * (mean.ndim - 1))
        return (sh(numpy.where(v, k, 0.0) * numpy.ones_like(mean)), sh(numpy.where(v, mean, 0.0)),
                sh(numpy.where(v, M2, 0.0)))

    # ---- nmc_k_ppc_obs ----
    with numpy.errstate(all="ignore"):
        fin = numpy.isfinite(x)
        vm = valid[:, None, None, None]
        lt = sh(((fin & (x < y) & vm).sum(axis=1)))
        eq = sh(((fin & (x == y) & vm).sum(axis=1)))
    ost = _butterfly(masked(*_welford_rows(x, range(nrows))))            # each [CB, n_obs, NR]
    olt, oeq = lt.sum(axis=1), eq.sum(axis=1)

    # ---- nmc_k_ppc_group and nmc_k_ppc_group_fin ----
    Tv = group_stats(x, integer)                                         # [lanes][rows][G][NR][4]
    Ty = group_stats(y[None], integer)[0]                                # [G][NR][4]
    with numpy.errstate(all="ignore"):
        vm = valid[:, None, None, None, None]
        gt = sh(((Tv > Ty) & vm)).astype(numpy.int64)                    # [CB][64][rows]...
        ge = sh(((Tv == Ty) & vm)).astype(numpy.int64)
    ggt, gge = gt.sum(axis=(1, 2)), ge.sum(axis=(1, 2))
    NS = ppc.group_slices(nrows, sc.G, NR, CB)
    acc_s = None
    for s in range(NS):
        rb, re = s * nrows // NS, (s + 1) * nrows // NS
        acc_w = None
        for w in range(4):
            st = _butterfly(masked(*_welford_rows(Tv, range(rb + w, re, 4))))
            acc_w = st if acc_w is None else _dev_merge(acc_w, st)
        acc_s = acc_w if acc_s is None else _dev_merge(acc_s, acc_w)

    parts = []
    for b in range(CB):
        parts.append(dict(
            obs_state=numpy.stack([numpy.transpose(a[b], (1, 0)) for a in ost]),
            obs_count=numpy.stack([olt[b].T, oeq[b].T]).astype(numpy.int64),
            group_state=numpy.stack([a[b] for a in acc_s], axis=-1),
            group_count=numpy.stack([ggt[b], gge[b]], axis=-1).astype(numpy.int64),
            ty=Ty, nonfinite=0))
    return parts


# ---------------------------------------------------------------------------------------
# the longdouble reference
# ---------------------------------------------------------------------------------------
def _moments(L):
    """Over axis 0 of longdouble L: (mean, M2, max |x|, sum x^2)."""
    S = L.shape[0]
    mean = L.sum(axis=0) / S
    return mean, ((L - mean) ** 2).sum(axis=0), numpy.abs(L).max(axis=0), (L * L).sum(axis=0)


def _t_ld(L, integer=False):
    """(T [..., 4], bound [..., 4]) of longdouble L[..., n] along the last axis: the two-pass
    formulas (integer values: var = (n sum x^2 - (sum x)^2) / n^2, every operation but the
    division exact) and ``t_bound``.  The values are sorted first: equal multisets then give equal
    statistics in longdouble too (its sums round as well)."""
    n = L.shape[-1]
    L = numpy.sort(L, axis=-1)
    mean = L.sum(axis=-1) / n
    M2 = ((L - mean[..., None]) ** 2).sum(axis=-1)
    amax, sq = numpy.abs(L).max(axis=-1), (L * L).sum(axis=-1)
    var = (n * sq - L.sum(axis=-1) ** 2) / LD(n * n) if integer else M2 / n
    T = numpy.stack([mean, var, L.min(axis=-1), L.max(axis=-1)], axis=-1)
    zero = numpy.zeros_like(mean)
    bound = numpy.stack([(n + 2) * U * amax, waic_ref.tol_m2_sharp(M2, sq, n) / n, zero, zero],
                        axis=-1)
    return T, bound


def reference(yrep, y, n_valid, integer=False):
    """The quantities of ``restate`` merged over the chain blocks, in longdouble, over the
    valid chains of yrep[chains][rows][n_obs][NRESP] (float64; every draw finite):
      S; obs: mean, M2, amax, sq [n_obs, NRESP], lt, eq
      group: t_obs [G, NRESP, 4], gt, geq and ambiguous [S, G, NRESP, 4] (the two sides differ
             and are closer than t_bound of both), tmean, tM2, tamax, tsq [G, NRESP, 4] over the
             float64 statistics of ``group_stats``."""
    x = numpy.asarray(yrep, dtype=numpy.float64)[:n_valid]
    x = x.reshape((-1,) + x.shape[2:])                                   # [S][n_obs][NR]
    L, yl = x.astype(LD), numpy.asarray(y, dtype=numpy.float64).astype(LD)
    out = dict(S=x.shape[0])
    out["mean"], out["M2"], out["amax"], out["sq"] = _moments(L)
    out["lt"], out["eq"] = (L < yl).sum(axis=0), (L == yl).sum(axis=0)
    T, B, Ty, By = [], [], [], []
    for g in range(sc.G):
        a, b = sc.OFF[g], sc.OFF[g + 1]
        t, bd = _t_ld(numpy.moveaxis(L[:, a:b], 1, -1), integer)         # [S][NR][4]
        T.append(t), B.append(bd)
        t, bd = _t_ld(yl[a:b].T, integer)                                # [NR][4]
        Ty.append(t), By.append(bd)
    T, B = numpy.stack(T, axis=1), numpy.stack(B, axis=1)                # [S][G][NR][4]
    Ty, By = numpy.stack(Ty), numpy.stack(By)
    out["t_obs"] = Ty
    out["gt"], out["geq"] = T > Ty, T == Ty
    bound = B + By
    out["ambiguous"] = (T != Ty) & (numpy.abs(T - Ty) <= bound)
    Tf = group_stats(x, integer).astype(LD)
    out["tmean"], out["tM2"], out["tamax"], out["tsq"] = _moments(Tf)
    return out


def tol_mean(S, amax):
    return (S + 64) * U * numpy.asarray(amax, dtype=numpy.float64)


def tol_m2(S, sq):
    return (S + 64) * U * numpy.asarray(sq, dtype=numpy.float64)


def check_states(part, ref, what=""):
    """A merged partial's n, mean and M2 (observations and groups) against ``reference`` within
    the tolerances above; prints and returns the worst error / tolerance ratio."""
    S = ref["S"]
    worst = 0.0
    for key, st, m, M2, amax, sq in (
            ("obs", part["obs_state"], ref["mean"].T, ref["M2"].T, ref["amax"].T, ref["sq"].T),
            ("group", numpy.moveaxis(part["group_state"], -1, 0), ref["tmean"], ref["tM2"],
             ref["tamax"], ref["tsq"])):
        assert numpy.all(st[0] == S), (what, key, "n")
        for name, got, want, tol in (("mean", st[1], m, tol_mean(S, amax)),
                                     ("M2", st[2], M2, tol_m2(S, sq))):
            err = numpy.abs(got.astype(LD) - want).astype(numpy.float64)
            with numpy.errstate(invalid="ignore", divide="ignore"):
                ratio = numpy.where(tol > 0, err / tol, numpy.where(err > 0, numpy.inf, 0.0))
            r = float(numpy.max(ratio))
            worst = max(worst, r)
            assert r <= 1.0, (what, key, name, r)
    print("ppc states %s: S=%d  max err/tol=%.3g" % (what, S, worst))
    return worst
