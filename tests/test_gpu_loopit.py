"""LOO-PIT and the leave-one-out predictive moments on the GPU: nmc_k_loo_yrep, nmc_k_psis with
its exported tail and nmc_k_psis_expect (csrc/loopit.h, csrc/psis.h) through
nmc_psis_expect_of, Engine.loo_pit / loo_pit_raw and samplePosterior(computeLooPit=True).

Reference, inputs and tolerances: tests/loopit_ref.py (the longdouble evaluation of
nestmc/loopit.py's formulas on top of tests/psis_ref.py; n_tail and the identities exact,
Tol-pit, Tol-mean, Tol-var, Tol-ess).  Every check prints its error / tolerance ratios."""

import ctypes
import os

import numpy
import pytest

import loopit_ref
import psis_ref
from gpu_cases import synthetic
from nestmc import _lib, loopit
from nestmc.families import DeviceLikelihood
from test_gpu_loo import LINREG_USER, SIZES, _linreg66, _psis_of, _run, _state, _to_store

pytestmark = pytest.mark.gpu

LOO = ("elpd", "lppd", "k", "n_tail", "nonfinite")
PIT = ("ess", "wlt", "weq", "mean", "var", "nonfinite_draws")


def _expect_of(lib, ll, yrep, y, n_valid, obs_batch=0, rc=False):
    """nmc_psis_expect_of over the host arrays ll, yrep [rows][n_obs][C] and y [n_obs]."""
    x = numpy.ascontiguousarray(ll, dtype=numpy.float64)
    r = numpy.ascontiguousarray(yrep, dtype=numpy.float64)
    yo = numpy.ascontiguousarray(y, dtype=numpy.float64)
    rows, n, C = x.shape
    assert r.shape == x.shape and yo.shape == (n,)
    f = {k: numpy.full(n, -7.0) for k in ("elpd", "lppd", "k", "ess", "wlt", "weq", "mean", "var")}
    nt = numpy.full(n, -7, dtype=numpy.int32)
    bad = numpy.full(n, -7, dtype=numpy.int64)
    badd = numpy.full(n, -7, dtype=numpy.int64)
    i64 = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))   # noqa: E731
    d = _lib.dptr
    code = lib.nmc_psis_expect_of(0, d(x), d(r), d(yo), rows, n, C, n_valid, obs_batch,
                                  d(f["elpd"]), d(f["lppd"]), d(f["k"]),
                                  nt.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), i64(bad),
                                  d(f["ess"]), d(f["wlt"]), d(f["weq"]), d(f["mean"]),
                                  d(f["var"]), i64(badd))
    out = dict(f, n_tail=nt, nonfinite=bad, nonfinite_draws=badd)
    if rc:
        return code, out
    _lib.check(code)
    return out


def _same(a, b, keys=LOO + PIT):
    return all(numpy.asarray(a[f]).tobytes() == numpy.asarray(b[f]).tobytes() for f in keys)


def _one(got, i, j=None):
    pick = (lambda a: a[i]) if j is None else (lambda a: a[i, j])
    return dict(ess=got["ess"][i], wlt=pick(got["wlt"]), weq=pick(got["weq"]),
                mean=pick(got["mean"]), var=pick(got["var"]), n_tail=got["n_tail"][i])


def _injected(sname, kinds=loopit_ref.KINDS):
    """(the observations [(column, kind)], ll store, yrep store, y) of one store."""
    rows, C, nv, cols = loopit_ref.cases()[sname]
    obs = [(c, k) for c in cols for k in kinds]
    reps = [loopit_ref.replicates(sname, c, rows * nv)[k] for c, k in obs]
    return (obs, psis_ref.store(rows, C, nv, [cols[c] for c, _ in obs]),
            psis_ref.store(rows, C, nv, [r for r, _ in reps]), numpy.array([y for _, y in reps]))


# ---- (a) nmc_psis_expect_of on injected columns ---------------------------------------------
@pytest.mark.parametrize("sname", loopit_ref.STORES)
def test_injected_columns(gpu_lib, sname):
    rows, C, nv, cols = loopit_ref.cases()[sname]
    obs, ll, yrep, y = _injected(sname)
    got = _expect_of(gpu_lib, ll, yrep, y, nv)
    assert not got["nonfinite"].any() and not got["nonfinite_draws"].any()   # (NaN padding unread)
    assert _same(_psis_of(gpu_lib, ll, nv), got, LOO)        # the LOO results of the same sort
    for i, (c, k) in enumerate(obs):
        loopit_ref.check(sname, c, k, _one(got, i), what="device")
    # one observation at a time and a ragged last batch: the same bits
    assert _same(_expect_of(gpu_lib, ll, yrep, y, nv, obs_batch=1), got)
    assert _same(_expect_of(gpu_lib, ll, yrep, y, nv, obs_batch=5), got)


def test_raised_lds_limit(gpu_lib):
    """nmc_k_psis_expect keeps the head and its weights in LDS, 16 M bytes: one column whose
    M = 7 800 needs the raised dynamic-LDS limit."""
    rows, C, nv, cols = loopit_ref.cases()["s6758400"]
    assert 2 * psis_ref.tail_length(rows * nv) * 8 > 64 * 1024
    yrep, y = loopit_ref.replicates("s6758400", "gauss_h", rows * nv)["normal"]
    got = _expect_of(gpu_lib, psis_ref.store(rows, C, nv, [cols["gauss_h"]]),
                     psis_ref.store(rows, C, nv, [yrep]), numpy.array([y]), nv)
    loopit_ref.check("s6758400", "gauss_h", "normal", _one(got, 0), what="device")


def test_swapping_replicates_of_tied_tail_samples_changes_no_bit(gpu_lib):
    rows, C, nv, cols = loopit_ref.cases()["s4224"]
    ll = cols["tail5"]
    tied = numpy.argsort(ll, kind="stable")[20:25]
    assert numpy.all(ll[tied] == ll[tied[0]])
    a, b, ys = [], [], []
    for kind in loopit_ref.KINDS:
        yrep, y = loopit_ref.replicates("s4224", "tail5", len(ll))[kind]
        yrep = yrep.copy()
        if kind == "binary":
            yrep[tied] = [0.0, 1.0, 1.0, 0.0, 1.0]
        sw = yrep.copy()
        sw[tied] = yrep[numpy.roll(tied, 2)]
        assert kind == "same" or not numpy.array_equal(sw, yrep)
        a.append(yrep), b.append(sw), ys.append(y)
    st = psis_ref.store(rows, C, nv, [ll] * 3)
    ga = _expect_of(gpu_lib, st, psis_ref.store(rows, C, nv, a), numpy.array(ys), nv)
    gb = _expect_of(gpu_lib, st, psis_ref.store(rows, C, nv, b), numpy.array(ys), nv)
    for f in PIT:
        print(f, ga[f], gb[f])
    assert _same(ga, gb)
    # and the tied samples share the mean weight of their places: within tolerance of the
    # reference whichever of them carries which replicate
    for i, kind in enumerate(loopit_ref.KINDS):
        psis = psis_ref.reference("s4224/tail5", ll)
        loopit_ref.check_values("s4224/tail5", ll, b[i], ys[i], _one(gb, i), what="device swapped",
                                ref=loopit_ref.column(ll, b[i], ys[i], numpy.longdouble, psis),
                                psis=psis)


# ---- (b) inputs that are not finite ---------------------------------------------------------
def test_nonfinite_inputs(gpu_lib):
    rows, C, nv, cols = loopit_ref.cases()["s4224"]
    S = rows * nv
    la = cols["gauss"].copy()
    la[1234] = -numpy.inf
    lb = cols["t3"].copy()
    lb[7], lb[4100] = numpy.nan, numpy.inf
    yr, y = loopit_ref.replicates("s4224", "gauss", S)["normal"]
    ya, yb = yr.copy(), yr.copy()
    ya[5], ya[4000] = numpy.nan, numpy.inf
    yb[4223] = -numpy.inf
    lls = [cols["gauss"], la, cols["gauss"], lb, cols["gauss"], la]
    yrs = [yr, yr, ya, yr, yb, ya]
    got = _expect_of(gpu_lib, psis_ref.store(rows, C, nv, lls), psis_ref.store(rows, C, nv, yrs),
                     numpy.full(6, y), nv)
    assert got["nonfinite"].tolist() == [0, 1, 0, 2, 0, 1]
    assert got["nonfinite_draws"].tolist() == [0, 0, 2, 0, 1, 2]
    for i in (1, 3, 5):             # log-likelihoods: NaN everywhere, as in nmc_loo
        assert all(numpy.isnan(got[f][i]) for f in ("elpd", "lppd", "k", "ess", "wlt", "weq",
                                                    "mean", "var")) and got["n_tail"][i] == 0
    for i in (2, 4):                # replicates: the field's results; ess and LOO are the column's
        assert all(numpy.isnan(got[f][i]) for f in ("wlt", "weq", "mean", "var"))
        assert all(got[f][i] == got[f][0] for f in ("elpd", "lppd", "k", "ess", "n_tail"))
    loopit_ref.check("s4224", "gauss", "normal", _one(got, 0), what="beside non-finite columns")


def test_expect_of_bad_arguments(gpu_lib):
    rows, C, nv, cols = loopit_ref.cases()["s30"]
    st = psis_ref.store(rows, C, nv, [cols["gauss"]])
    y = numpy.zeros(1)
    for kw in (dict(n_valid=0), dict(n_valid=4), dict(obs_batch=-1)):
        code, out = _expect_of(gpu_lib, st, st, y, **dict(dict(n_valid=3, rc=True), **kw))
        assert code == -1, kw
        assert (out["elpd"] == -7.0).all() and (out["wlt"] == -7.0).all()
    code, out = _expect_of(gpu_lib, st[:1, :, :1], st[:1, :, :1], y, 1, rc=True)      # S = 1
    assert code == -1 and (out["ess"] == -7.0).all()
    code, out = _expect_of(gpu_lib, st[:, :0], st[:, :0], y[:0], 3, rc=True)          # no observations
    assert code == -1


# ---- (c) Engine.loo_pit on small models -----------------------------------------------------
def _draw_store(eng, rb=0, nr=None):
    """(ll, yrep[field]) of a window in the store's layout, from obs_ll_rows / predictive_draws."""
    ll = eng.obs_ll_rows(rb, nr)
    yr = eng.predictive_draws(rb, nr)
    return ll, yr, _to_store(ll), [_to_store(yr[..., j]) for j in range(yr.shape[3])]


def _check_engine(gpu_lib, eng, got, rb, nr, nv, what):
    """got against nmc_psis_expect_of fed the engine's own values (bit for bit) and against
    the reference over them."""
    ll, yr, lls, yrs = _draw_store(eng, rb, nr)
    y = eng.observed()
    for j, yst in enumerate(yrs):
        of = _expect_of(gpu_lib, lls, yst, y[:, j], nv)
        assert _same(of, got, LOO) and of["ess"].tobytes() == got["ess"].tobytes(), (what, j)
        for f in PIT[1:]:
            assert of[f].tobytes() == numpy.ascontiguousarray(got[f][:, j]).tobytes(), (what, j, f)
        for i in range(ll.shape[2]):
            col = numpy.ascontiguousarray(ll[:nv, :, i].T).reshape(-1)    # s = row * n_valid + chain
            rep = numpy.ascontiguousarray(yr[:nv, :, i, j].T).reshape(-1)
            loopit_ref.check_values("%s/%d" % (what, i), col, rep, y[i, j], _one(got, i, j),
                                    what="device field %d" % j)
    assert not got["nonfinite"].any() and not got["nonfinite_draws"].any()


@pytest.fixture(scope="module")
def eng66(gpu_lib):
    """test_gpu_loo's partial-pooling linreg: 66 chains, ragged groups, 64 recorded rows."""
    eng = _run(_linreg66(), SIZES, None, "partial", 66, 148, 20, 2)
    assert eng.n_rows == 64
    yield eng, eng.loo_pit_raw()
    eng.close()


def test_engine_linreg_partial(gpu_lib, eng66):
    eng, got = eng66
    assert got["n_samples"] == 66 * 64 and got["wlt"].shape == (40, 1)
    assert _same(eng.loo_raw(), got, LOO)                      # nmc_loo's bits from the same sort
    _check_engine(gpu_lib, eng, got, 0, None, 66, "linreg66")
    res = eng.loo_pit()
    assert eng.loo_nonfinite == 0 and eng.loo_pit_nonfinite == 0
    assert res.loo.elpd_i.tobytes() == got["elpd"].tobytes() and res.n_samples == 4224
    assert res.loo_pit.tobytes() == (got["wlt"] + got["weq"] / 2.0).tobytes()
    assert numpy.array_equal(res.y, eng.observed()) and res.pit_mean_g.shape == (4,)
    assert numpy.all((res.loo_pit > 0) & (res.loo_pit < 1)) and numpy.all(res.weq == 0)
    assert numpy.all(res.ess > 1) and numpy.all(res.ess <= 4224) and numpy.all(res.loo_sd > 0)


def test_engine_gauss_none(gpu_lib):
    fam, sizes, priors, pooling, _ = synthetic("gauss_none", 3, 4, 5)
    eng = _run(fam, sizes, priors, pooling, 3, 60, 20, 4)
    try:
        assert eng.n_rows == 10 and eng.n_resp() == 3
        got = eng.loo_pit_raw()
        assert got["wlt"].shape == (20, 3)
        assert _same(eng.loo_raw(), got, LOO)
        _check_engine(gpu_lib, eng, got, 0, None, 3, "gauss3")
    finally:
        eng.close()


# ---- (d) batches, row windows and padding ---------------------------------------------------
def test_obs_batch_bit_identical(eng66):
    eng, got = eng66
    for b in (1, 7, 0):                                 # 40 = 5 * 7 + 5: a ragged last batch
        assert _same(eng.loo_pit_raw(obs_batch=b), got), b


def test_row_range_and_padding(gpu_lib, eng66):
    eng, _ = eng66
    sub = eng.loo_pit_raw(row_begin=5, n_rows=30)
    assert _same(eng.loo_raw(row_begin=5, n_rows=30), sub, LOO)
    _check_engine(gpu_lib, eng, sub, 5, 30, 66, "linreg66 rows 5..34")
    pad = eng.loo_pit_raw(n_valid=65)                   # the last chain as padding
    _check_engine(gpu_lib, eng, pad, 0, None, 65, "linreg66 n_valid 65")
    # ... and never read: its rows of the store set to NaN change no bit
    raw = eng.samples_raw()
    try:
        nan = raw.copy()
        nan[:, :, 65] = numpy.nan
        eng.set_samples_raw(nan)
        again = eng.loo_pit_raw(n_valid=65)
        assert _same(again, pad) and not again["nonfinite"].any()
        assert not again["nonfinite_draws"].any()
    finally:
        eng.set_samples_raw(raw)


def test_engine_bad_arguments(eng66):
    eng, got = eng66
    for kw in (dict(n_rows=0), dict(row_begin=60, n_rows=5), dict(row_begin=-1, n_rows=2),
               dict(n_valid=0), dict(n_valid=67), dict(obs_batch=-1), dict(n_rows=1, n_valid=1)):
        with pytest.raises(_lib.NestmcError):
            eng.loo_pit_raw(**kw)
    assert _same(eng.loo_pit_raw(), got)                # (the context still works)


# ---- (e) a discrete response; user families -------------------------------------------------
def test_logistic_discrete_response(gpu_lib):
    fam, sizes, priors, pooling, _ = synthetic("logistic_partial", 66, 3, 6)
    eng = _run(fam, sizes, priors, pooling, 66, 100, 20, 4)
    try:
        assert eng.n_rows == 20
        got = eng.loo_pit_raw()
        _check_engine(gpu_lib, eng, got, 0, None, 66, "logistic66")
        y = eng.observed()[:, 0]
        assert set(y.tolist()) == {0.0, 1.0}
        assert numpy.all(got["weq"] > 0)                 # replicates that equal y carry weight
        # wlt + weq: the weighted mass at or below y -- all of it for y = 1, the zeros' for y = 0
        ll, yr = eng.obs_ll_rows(), eng.predictive_draws()
        for i in range(len(y)):
            col = numpy.ascontiguousarray(ll[:, :, i].T).reshape(-1)
            w = loopit.psis_weights(col)
            rep = numpy.ascontiguousarray(yr[:, :, i, 0].T).reshape(-1)
            mass = float(numpy.sum(w[rep <= y[i]]))
            # (the device's sum and the host's are each within Tol-pit of the exact one)
            tol = loopit_ref.tolerances(dict(ess=1.0), psis_ref.reference("logistic66/%d" % i, col),
                                        len(w), [1.0])[0]
            assert abs(got["wlt"][i, 0] + got["weq"][i, 0] - mass) <= 2 * tol, i
            if y[i] == 1.0:
                assert got["wlt"][i, 0] + got["weq"][i, 0] == pytest.approx(1.0, abs=2 * tol)
            else:
                assert got["wlt"][i, 0] == 0.0
    finally:
        eng.close()


LINREG_USER_PREDICT = LINREG_USER + r"""
__device__ double nmc_user_predict(const double* th, const double* row, const double* k,
                                   double ua, double ub, double z) {
  double yh = th[0];
  yh = yh + row[0] * th[1];
  const double s = k[0];
  if (!(s > 0.0)) return nmc_nan();
  return yh + s * z;
}
"""


def test_user_family_bit_identical_to_builtin(gpu_lib):
    """nmc_k_loo_yrep<FamUser> compiled at run time against the built-in linreg's instance on
    bit-identical sample stores; a source without nmc_user_predict is refused."""
    fam = _linreg66()
    st = _state(fam, SIZES, 66, 2, "partial")
    user = DeviceLikelihood(fam.obs(), LINREG_USER_PREDICT, 2, consts=[1.0, 0.0],
                            host_function=fam, response_field=1)
    plain = DeviceLikelihood(fam.obs(), LINREG_USER, 2, consts=[1.0, 0.0], host_function=fam)
    a = _run(fam, SIZES, None, "partial", 66, 60, 20, 4, state=st)
    b = _run(user, SIZES, None, "partial", 66, 60, 20, 4, state=st)
    c = _run(plain, SIZES, None, "partial", 66, 60, 20, 4, state=st)
    try:
        assert a.samples_raw().tobytes() == b.samples_raw().tobytes()
        assert a.predictive_draws().tobytes() == b.predictive_draws().tobytes()
        ga = a.loo_pit_raw()
        assert _same(ga, b.loo_pit_raw()) and _same(ga, b.loo_pit_raw(obs_batch=3))
        with pytest.raises(ValueError, match="nmc_user_predict"):
            c.loo_pit()
        n = 40
        buf = [numpy.full(n, -7.0) for _ in range(8)]
        nt = numpy.zeros(n, dtype=numpy.int32)
        bad, badd = numpy.zeros(n, dtype=numpy.int64), numpy.zeros(n, dtype=numpy.int64)
        i64 = lambda x: x.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))   # noqa: E731
        d = _lib.dptr
        code = gpu_lib.nmc_loo_pit(c.h, 0, c.n_rows, 66, 0, d(buf[0]), d(buf[1]), d(buf[2]),
                                   nt.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), i64(bad),
                                   d(buf[3]), d(buf[4]), d(buf[5]), d(buf[6]), d(buf[7]), i64(badd))
        assert code == -1 and b"nmc_user_predict" in gpu_lib.nmc_last_error()
        assert all((x == -7.0).all() for x in buf)
    finally:
        a.close()
        b.close()
        c.close()


# ---- (f) samplePosterior(computeLooPit=True) ------------------------------------------------
def test_sample_posterior_compute_loo_pit(gpu_lib, tmp_path):
    from nestmc.sampler import sample_posterior
    C, G, N = 70, 5, 30
    fam, sizes, priors, pooling, names = synthetic("linreg_partial", C, G, N)
    ranges = {n: [-0.5, 0.5] for n in names}
    kw = dict(saveLogLikelihood=False, priorDistribution=priors, startingPointValueRange=ranges,
              displayProgress=False, seed=17, return_samples=True, write_files=True)
    out = str(tmp_path / "pit")
    res = sample_posterior(C, 60, 20, names, G, N, pooling, fam, out, computeLooPit=True, **kw)
    r = res["loo_pit"]
    assert "loo" not in res
    assert sorted(os.listdir(out)) == ["log", "loo_pit_groups.csv", "loo_pit_pointwise.csv",
                                       "sample"]
    path = os.path.join(out, "loo_pit_pointwise.csv")
    assert open(path).readline().strip() == loopit.HEADER_POINTWISE
    p = numpy.loadtxt(path, delimiter=",", skiprows=1)
    assert numpy.array_equal(p[:, 0], numpy.arange(150))
    assert numpy.array_equal(p[:, 1], numpy.repeat(numpy.arange(G), N)) and not p[:, 2].any()
    assert numpy.array_equal(p[:, 3:], numpy.stack(
        [r.y[:, 0], r.loo_mean[:, 0], r.loo_sd[:, 0], r.loo_residual[:, 0], r.loo_pit[:, 0],
         r.wlt[:, 0], r.weq[:, 0], r.ess, r.pareto_k], 1))
    path = os.path.join(out, "loo_pit_groups.csv")
    assert open(path).readline().strip() == loopit.HEADER_GROUPS
    g = numpy.loadtxt(path, delimiter=",", skiprows=1)
    assert numpy.array_equal(g, numpy.stack([numpy.arange(G), r.n_g, r.pit_mean_g,
                                             r.n_outside_g], 1))
    assert r.n_pit == 150 and r.n_samples == r.loo.n_samples
    log = open(os.path.join(out, "log", "samplePosterior.log")).read()
    assert log.count("LOO-PIT: %d of 150" % r.n_outside) == 1 and "expected 5 %" in log
    # with computeLoo the one pass serves both: loo.csv is computeLoo's own
    both = str(tmp_path / "both")
    rb = sample_posterior(C, 60, 20, names, G, N, pooling, fam, both, computeLoo=True,
                          computeLooPit=True, **kw)
    alone = str(tmp_path / "loo")
    ra = sample_posterior(C, 60, 20, names, G, N, pooling, fam, alone, computeLoo=True, **kw)
    assert rb["loo"] is rb["loo_pit"].loo
    assert numpy.array_equal(rb["loo"].elpd_i, ra["loo"].elpd_i)
    assert numpy.array_equal(rb["loo_pit"].loo_pit, r.loo_pit)
    for f in ("loo.csv", "loo_pointwise.csv"):
        assert open(os.path.join(both, f)).read() == open(os.path.join(alone, f)).read()
    assert sorted(os.listdir(both)) == ["log", "loo.csv", "loo_pit_groups.csv",
                                        "loo_pit_pointwise.csv", "loo_pointwise.csv", "sample"]
    # off by default
    assert "loo_pit" not in ra and sorted(os.listdir(alone)) == ["log", "loo.csv",
                                                                 "loo_pointwise.csv", "sample"]
    # several engines: not yet, and nothing is written
    with pytest.raises(NotImplementedError):
        sample_posterior(C, 60, 20, names, G, N, pooling, fam, str(tmp_path / "two"),
                         computeLooPit=True, devices=[0, 0], **kw)
    assert not os.path.exists(str(tmp_path / "two"))
