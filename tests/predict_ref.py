"""The references of the prediction tests (tests/test_predict_host.py on the CPU,
tests/test_gpu_predict.py on the device), on the stores of tests/store_cases.py.  numpy only.

The new table has 44 rows in this order of group codes (T = 8 = NMC_WAIC_T):
  group 0 x 1, group 3 x 9 (T + 1), new 0 x 8 (T), group 1 x 7 (T - 1), new 1 x 17 (2 T + 1),
  group 3 x 2 (a revisited group: a second tile run)
and every third row (i % 3 == 2) has NaN in all its response fields.  Cases under partial
pooling ("benign", "logistic", "poisson") use a copy of their store whose <name>_sigma2 columns
are |x| + 0.1 (the stores' hyper columns are N(0, 1)); cases without pooling ("sigma", "gauss")
have no hyper-parameters: their table has training group 2 in place of new 0 and 4 of new 1.

``theta_new_ref(name)`` the new groups' values: the stream of csrc/predict.h restated with
                     oracle.philox -- z of the block (r, k, q, purpose 5), key (chain, seed) --
                     and mu + sqrt(sigma2) z in longdouble on the float64 store; tolerance
                     2 * 2^-53 (|mu| + |sd z|) + 1e-14 |sd z|: two roundings (the product, the
                     sum; sqrt's is inside the first) plus the project's agreement on z.
``theta_rows(...)``  float64 theta of every new row [C][R][P][n_new]: the store's columns for a
                     training group, the given float64 theta_new for a new one.
``evaluate(...)``    the family's formulas in longdouble AT those float64 theta: the draws (the
                     block (r, i, j, purpose 6)) with ppc_ref's tolerance (K + 3) 2^-53 A +
                     1e-14 |s z|, and ll with its scale A (store_cases.ll_ref's definitions) for
                     store_cases.obs_ll_units.  The device tests hand it the device's own
                     theta_new (held to theta_new_ref separately), the CPU tests the reference's
                     rounded to float64.
``restate(...)``     nmc_k_predict in float64, operation by operation, over given draws and ll:
                     waic_ref.restate_parts' (m, s) with the exponential as an argument
                     (``restate_dens``), ppc_ref's Welford rows and butterfly, the counts; the
                     chain blocks are left to nestmc.predict.merge.
``reference(...)``   the same quantities in longdouble.

The Poisson case (tests/user_models.py POISSON, rows [x, y, lgamma(y + 1)], k = log exposure)
draws by the normal approximation y_rep = lam + sqrt(lam) z, lam = exp(eta): tolerance
2^-53 ((3 E + 2) (lam + |s z| / 2) + 3 (lam + |s z|)) + 1e-14 |s z|, E = |a| + |b x| + |k| --
eta's three roundings move lam by 3 E 2^-53 lam and sqrt(lam) by half of that, exp and sqrt
round once each, then the product and the sum.  Its ll scale is A = |y| E + lam (1 + E) + |lg|.
"""

import functools

import numpy

import ppc_ref
import store_cases as sc
import user_models
import waic_ref
from nestmc import predict
from nestmc.families import DeviceLikelihood, GaussianMean, LinearRegression, Logistic
from oracle import philox

LD = numpy.longdouble
SEED = ppc_ref.SEED
PURPOSE_NEW_GROUP = 5      # csrc/rng.h NMC_PURPOSE_NEW_GROUP
PURPOSE_PREDICT_NEW = 6    # csrc/rng.h NMC_PURPOSE_PREDICT_NEW
T = sc.T
RUNS = ((0, 1), (3, T + 1), (-1, T), (1, T - 1), (-2, 2 * T + 1), (3, 2))
CODES = numpy.concatenate([[c] * n for c, n in RUNS]).astype(numpy.int32)
CODES_TRAIN = numpy.where(CODES == -1, 2, numpy.where(CODES == -2, 4, CODES)).astype(numpy.int32)
N_NEW = len(CODES)
NO_RESP = numpy.arange(N_NEW) % 3 == 2
LOG_EXPOSURE = 0.1
NAMES = ["benign", "logistic", "gauss", "sigma", "poisson"]

POISSON_PREDICT = user_models.POISSON + r"""
__device__ double nmc_user_predict(const double* th, const double* row, const double* k,
                                   double ua, double ub, double z) {
  const double eta = th[0] + th[1] * row[0] + k[0];
  const double lam = exp(eta);
  return lam + sqrt(lam) * z;
}
"""

Setup = __import__("collections").namedtuple(
    "Setup", "name kind case fam store new K pooling resp")


@functools.lru_cache(maxsize=None)
def poisson_family(predict_fn=True):
    r = numpy.random.RandomState(4302)
    y = r.poisson(2.0, size=sc.N_OBS).astype(float)
    return DeviceLikelihood(user_models.poisson_rows(sc.X_LIN, y),
                            POISSON_PREDICT if predict_fn else user_models.POISSON, 2,
                            consts=[LOG_EXPOSURE], response_field=1 if predict_fn else None)


def _new_obs(kind):
    r = numpy.random.RandomState(4301)
    if kind in ("linreg", "regression"):
        x = r.normal(size=N_NEW)
        obs = LinearRegression.simple(x, 2.0 * x + r.normal(size=N_NEW), sigma=1.0).obs()
    elif kind == "logistic":
        x = r.randint(-8, 9, size=(N_NEW, 3)) / 4.0
        y = (r.uniform(size=N_NEW) < 0.5).astype(float)
        obs = Logistic(numpy.hstack([numpy.ones((N_NEW, 1)), x]), y).obs()
    elif kind == "gauss":
        obs = GaussianMean(r.normal(size=(N_NEW, 3)), sc.SD_GAUSS).obs()
    else:
        x = r.normal(size=N_NEW)
        obs = user_models.poisson_rows(x, r.poisson(2.0, size=N_NEW).astype(float))
    return numpy.array(obs, dtype=numpy.float64)


@functools.lru_cache(maxsize=None)
def setup(name):
    """The case's family, store (its sigma2 columns made positive under partial pooling), the
    NewData and what goes with it."""
    case = sc.BY_NAME["benign" if name == "poisson" else name]
    kind = "poisson" if name == "poisson" else case.kind
    fam = poisson_family() if name == "poisson" else case.fam
    store = case.store.copy()
    partial = case.pooling == "partial"
    if partial:
        for q in range(case.P):
            c = q * (sc.G + 2) + 1
            store[:, c, :] = numpy.abs(store[:, c, :]) + 0.1
    store.setflags(write=False)
    resp = list(fam.response_fields())
    obs = _new_obs(kind)
    assert obs.shape[1] == fam.n_fields
    obs[numpy.ix_(NO_RESP, resp)] = numpy.nan
    new = predict.NewData(obs, CODES if partial else CODES_TRAIN)
    return Setup(name, kind, case, fam, store, new, new.K, case.pooling, resp)


def _bcast(n_chains, chain_base, rows):
    rows = numpy.arange(sc.R) if rows is None else numpy.asarray(rows)
    c = (chain_base + numpy.arange(n_chains))[:, None, None, None]
    return c, rows[None, :, None, None]


def theta_new_ref(name, chain_base=0, n_chains=sc.C, rows=None, store=None):
    """(theta [C][R][K][P] longdouble, tol float64, z float64) of the case's new groups."""
    s = setup(name)
    st = s.store if store is None else store
    rows_ = numpy.arange(sc.R) if rows is None else numpy.asarray(rows)
    c, r = _bcast(n_chains, chain_base, rows)
    k = numpy.arange(s.K)[None, None, :, None]
    q = numpy.arange(s.case.P)[None, None, None, :]
    z = philox.normal(r, k, q, PURPOSE_NEW_GROUP, c, SEED)              # [C][R][K][P]
    cols = numpy.arange(s.case.P) * (sc.G + 2)
    sel = st[rows_][:, :, chain_base:chain_base + n_chains]             # [R][cols][C]
    mu = numpy.transpose(sel[:, cols], (2, 0, 1))[:, :, None, :].astype(LD)
    s2 = numpy.transpose(sel[:, cols + 1], (2, 0, 1))[:, :, None, :].astype(LD)
    with numpy.errstate(all="ignore"):
        ok = (s2 > 0) & numpy.isfinite(s2)
        sz = numpy.sqrt(numpy.where(ok, s2, LD(1))) * z.astype(LD)
        th = numpy.where(ok, mu + sz, LD(numpy.nan))
        tol = 2 * 2.0 ** -53 * (numpy.abs(mu) + numpy.abs(sz)) + 1e-14 * numpy.abs(sz)
    return th, numpy.asarray(tol + 0 * z, dtype=numpy.float64), z


def theta_rows(name, theta_new, chain_base=0, n_chains=sc.C, rows=None, store=None):
    """float64 [C][R][P][n_new]: theta of every new row."""
    s = setup(name)
    st = s.store if store is None else store
    rows_ = numpy.arange(sc.R) if rows is None else numpy.asarray(rows)
    th = sc.theta_of(s.case, st)[rows_][:, chain_base:chain_base + n_chains]   # [R][C][P][G]
    th = numpy.transpose(th, (1, 0, 2, 3))
    out = numpy.empty(th.shape[:3] + (N_NEW,))
    for i, code in enumerate(s.new.group):
        out[..., i] = th[..., code] if code >= 0 else theta_new[:, :, -(code + 1), :]
    return out


def evaluate(name, th, chain_base=0, rows=None):
    """From float64 theta th[C][R][P][n_new]: a dict of yrep, tol [C][R][n_new][NRESP], ll, A
    [C][R][n_new] (longdouble; tol float64), and for the logistic gap = |ua - p|."""
    s = setup(name)
    NR = len(s.resp)
    nc = th.shape[0]
    c, r = _bcast(nc, chain_base, rows)
    i = numpy.arange(N_NEW)[None, None, :, None]
    j = numpy.arange(NR)[None, None, None, :]
    ua, ub = philox.uniforms(r, i, j, PURPOSE_PREDICT_NEW, c, SEED)
    z = philox.box_muller(ua, ub)
    zl = z.astype(LD)
    th = numpy.asarray(th, dtype=numpy.float64).astype(LD)
    obs = s.new.obs.astype(LD)
    out = {}
    with numpy.errstate(all="ignore"):
        if s.kind == "gauss":
            sd = sc.SD_GAUSS.astype(LD)
            t = numpy.transpose(th, (0, 1, 3, 2))                       # [C][R][n][P]
            sz = sd * zl
            yrep, A, K = t + sz, numpy.abs(t) + numpy.abs(sz), 0
            e = (th - obs.T[None, None]) / sd[None, None, :, None]
            sq = sc._to_f64_range(e * e)
            lsd = numpy.log(sd)[None, None, :, None]
            ll = (-sq / 2 - sc.LOG_C_LD - lsd).sum(axis=2)
            AL = (sq / 2 + sc.LOG_C_LD + numpy.abs(lsd)).sum(axis=2)
            tol = (K + 3) * 2.0 ** -53 * A + 1e-14 * numpy.abs(sz)
        elif s.kind == "poisson":
            x, y, lg = obs[:, 0], obs[:, 1], obs[:, 2]
            k0 = LD(LOG_EXPOSURE)
            eta = th[:, :, 0] + th[:, :, 1] * x + k0
            E = numpy.abs(th[:, :, 0]) + numpy.abs(th[:, :, 1] * x) + numpy.abs(k0)
            lam = numpy.exp(eta)
            ll = y * eta - lam - lg
            AL = numpy.abs(y) * E + lam * (1 + E) + numpy.abs(lg)
            sz = (numpy.sqrt(lam))[..., None] * zl
            yrep = lam[..., None] + sz
            tol = 2.0 ** -53 * ((3 * E[..., None] + 2) * (lam[..., None] + numpy.abs(sz) / 2)
                                + 3 * (lam[..., None] + numpy.abs(sz))) + 1e-14 * numpy.abs(sz)
        else:
            K = s.fam.n_fields - 1
            x, y = obs[:, :K].T, obs[:, K]
            b0, b = th[:, :, 0], th[:, :, 1:1 + K]
            eta = b0 + (b * x[None, None]).sum(axis=2)
            E = numpy.abs(b0) + (numpy.abs(b) * numpy.abs(x)[None, None]).sum(axis=2)
            if s.kind == "logistic":
                ll = y * eta - numpy.logaddexp(LD(0), eta)
                AL = numpy.abs(y) * E + numpy.logaddexp(LD(0), E)
                p = (1 / (1 + numpy.exp(-eta)))[..., None]
                yrep = numpy.where(ua.astype(LD) < p, LD(1), LD(0))
                yrep = numpy.where(numpy.isnan(p), LD(numpy.nan), yrep)
                out["gap"] = numpy.abs(ua.astype(LD) - p).astype(numpy.float64)
                tol = numpy.zeros(yrep.shape)
            else:
                sig = th[:, :, K + 1] if s.case.P == K + 2 else numpy.ones_like(eta)
                ok = sig > 0
                sg = numpy.where(ok, sig, LD(1))
                t = (eta - y) / sg
                sq = sc._to_f64_range(t * t)
                ll = numpy.where(ok, -sq / 2 - sc.LOG_C_LD - numpy.log(sg), LD(numpy.nan))
                ra = (E + numpy.abs(y)) / sg
                AL = numpy.where(ok, sc._to_f64_range(ra * ra) / 2 + sc.LOG_C_LD
                                 + numpy.abs(numpy.log(sg)), LD(numpy.nan))
                sz = sg[..., None] * zl
                yrep = numpy.where(ok[..., None], eta[..., None] + sz, LD(numpy.nan))
                tol = (K + 3) * 2.0 ** -53 * (E[..., None] + numpy.abs(sz)) \
                    + 1e-14 * numpy.abs(sz)
    out.update(yrep=yrep, ll=ll, A=AL,
               tol=numpy.asarray(numpy.where(numpy.isfinite(tol), tol, 0), dtype=numpy.float64))
    return out


@functools.lru_cache(maxsize=None)
def host(name):
    """The CPU tests' inputs: the reference theta_new rounded to float64, and ``evaluate`` at
    it; yrep and ll also rounded to float64 (yrep64, ll64)."""
    s = setup(name)
    tn = None
    if s.K:
        with numpy.errstate(all="ignore"):
            tn = numpy.asarray(theta_new_ref(name)[0], dtype=numpy.float64)
    ev = evaluate(name, theta_rows(name, tn))
    with numpy.errstate(all="ignore"):
        ev["yrep64"] = numpy.asarray(ev["yrep"], dtype=numpy.float64)
        ev["ll64"] = numpy.asarray(ev["ll"], dtype=numpy.float64)
    ev["theta_new"] = tn
    return ev


# ---------------------------------------------------------------------------------------
# the float64 restatement and the longdouble reference of the reduction
# ---------------------------------------------------------------------------------------
def restate_dens(ll, C, n_valid, exp=numpy.exp):
    """nmc_k_predict's density pass over ll[chains >= n_valid][R][n_new] in float64: the (m, s, n)
    of waic_ref.restate_parts, operation by operation, with the exponential as an argument.
    With numpy's exp it IS restate_parts' (m, s, n); handed the device library's exp
    (tests/test_gpu_predict.py evaluates it on the GPU) every word, s included, is the
    kernel's.  -> [CB][3][n_new]."""
    ll = numpy.asarray(ll, dtype=numpy.float64)
    nc, R, n = ll.shape
    CB = (C + 63) // 64
    lanes = CB * 64
    assert n_valid <= C and nc >= n_valid
    x_all = numpy.zeros((lanes, R, n))
    x_all[:min(nc, lanes)] = ll[:lanes]
    v = (numpy.arange(lanes) < n_valid)[:, None]
    with numpy.errstate(all="ignore"):
        m = numpy.full((lanes, n), -numpy.inf)
        s = numpy.zeros((lanes, n))
        for r in range(R):
            x = x_all[:, r]
            dm = x - m
            e = exp(-numpy.abs(dm))
            s = numpy.where(dm <= 0.0, s + e, s * e + 1.0)
            m = numpy.fmax(m, x)
        st = (numpy.where(v, m, -numpy.inf), numpy.where(v, s, 0.0),
              numpy.where(v, float(R), 0.0) * numpy.ones((lanes, n)))
        st = tuple(a.reshape(CB, 64, n) for a in st)
        for _ in range(6):   # lane ^ 1, ^ 2, ... ^ 32: a balanced tree, the lower lane is A
            (mA, sA, nA), (mB, sB, nB) = (tuple(a[:, h::2] for a in st) for h in (0, 1))
            mm = numpy.fmax(mA, mB)
            ta = numpy.where(nA > 0.0, sA * exp(mA - mm), 0.0)
            tb = numpy.where(nB > 0.0, sB * exp(mB - mm), 0.0)
            st = (mm, ta + tb, nA + nB)
    return numpy.ascontiguousarray(numpy.stack([a[:, 0] for a in st], axis=1))


def restate(yrep, ll, y, C, n_valid, exp=numpy.exp):
    """The chain blocks' partials (nestmc.predict dicts) of an engine of C chains over the
    window's draws yrep[chains >= n_valid][rows][n_new][NRESP] and ll[chains][rows][n_new]
    (float64), y [n_new][NRESP] the held-out responses (NaN: none)."""
    yrep = numpy.asarray(yrep, dtype=numpy.float64)
    ll = numpy.asarray(ll, dtype=numpy.float64)
    y = numpy.asarray(y, dtype=numpy.float64)
    nc, nrows, n_new, NR = yrep.shape
    CB = (C + 63) // 64
    lanes = CB * 64
    dens = restate_dens(ll, C, n_valid, exp)                            # [CB][m, s, n][n_new]
    x = numpy.zeros((lanes, nrows, n_new, NR))
    x[:min(nc, lanes)] = yrep[:lanes]
    valid = numpy.arange(lanes) < n_valid
    sh = lambda a: a.reshape((CB, 64) + a.shape[1:])   # noqa: E731
    with numpy.errstate(all="ignore"):
        fin = numpy.isfinite(x)
        vm = valid[:, None, None, None]
        lt = sh((fin & (x < y) & vm).sum(axis=1)).sum(axis=1)           # [CB][n_new][NR]
        eq = sh((fin & (x == y) & vm).sum(axis=1)).sum(axis=1)
    k, mean, M2 = ppc_ref._welford_rows(x, range(nrows))
    v = valid[:, None, None]
    st = ppc_ref._butterfly((sh(numpy.where(v, k, 0.0) * numpy.ones_like(mean)),
                             sh(numpy.where(v, mean, 0.0)), sh(numpy.where(v, M2, 0.0))))
    return [dict(dens=dens[b], state=numpy.stack([a[b].T for a in st]),
                 count=numpy.stack([lt[b].T, eq[b].T]).astype(numpy.int64),
                 nonfinite_draws=0, nonfinite_ll=0) for b in range(CB)]


def reference(yrep, ll, y, n_valid):
    """In longdouble over the valid chains: S; lpd [n_new]; mean, M2, amax, sq [n_new][NRESP];
    lt, eq."""
    x = numpy.asarray(yrep, dtype=numpy.float64)[:n_valid]
    x = x.reshape((-1,) + x.shape[2:]).astype(LD)
    L = numpy.asarray(ll, dtype=numpy.float64)[:n_valid]
    L = L.reshape(-1, L.shape[-1])
    yl = numpy.asarray(y, dtype=numpy.float64).astype(LD)
    out = dict(S=x.shape[0], lpd=waic_ref.reference(L)[0])
    out["mean"], out["M2"], out["amax"], out["sq"] = ppc_ref._moments(x)
    with numpy.errstate(invalid="ignore"):
        out["lt"], out["eq"] = (x < yl).sum(axis=0), (x == yl).sum(axis=0)
    return out


def check(merged, ref, has, what=""):
    """A merged partial against ``reference``: counts equal; mean and M2 within ppc_ref.tol_mean
    / tol_m2; lpd within waic_ref.tol_lppd at the observations with a response.  Prints and
    returns the worst error / tolerance ratio."""
    S = ref["S"]
    assert numpy.all(merged["state"][0] == S) and numpy.all(merged["dens"][2] == S), what
    assert numpy.array_equal(merged["count"][0], ref["lt"].T), (what, "lt")
    assert numpy.array_equal(merged["count"][1], ref["eq"].T), (what, "eq")
    worst = 0.0
    for nm, got, want, tol in (
            ("mean", merged["state"][1], ref["mean"].T, ppc_ref.tol_mean(S, ref["amax"].T)),
            ("M2", merged["state"][2], ref["M2"].T, ppc_ref.tol_m2(S, ref["sq"].T))):
        err = numpy.abs(got.astype(LD) - want).astype(numpy.float64)
        with numpy.errstate(invalid="ignore", divide="ignore"):
            ratio = numpy.where(tol > 0, err / tol, numpy.where(err > 0, numpy.inf, 0.0))
        r = float(numpy.max(ratio)) if ratio.size else 0.0
        worst = max(worst, r)
        assert r <= 1.0, (what, nm, r)
    m, s_, _ = merged["dens"]
    with numpy.errstate(all="ignore"):
        lpd = m + numpy.log(s_ / S)
    err = numpy.abs(lpd.astype(LD) - ref["lpd"])[has].astype(numpy.float64)
    r = float(numpy.max(err / waic_ref.tol_lppd(ref["lpd"][has], S).astype(numpy.float64)))
    worst = max(worst, r)
    assert r <= 1.0, (what, "lpd", r)
    print("predict %s: S=%d  max err/tol=%.3g" % (what, S, worst))
    return worst
