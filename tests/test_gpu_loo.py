"""PSIS-LOO on the GPU: nmc_k_loo_ll, the column sort and nmc_k_psis (csrc/psis.h) through
nmc_psis_of, Engine.loo / loo_raw and samplePosterior(computeLoo=True).

Reference, inputs and tolerances: tests/psis_ref.py (the longdouble evaluation of
nestmc/loo.py's formulas; n_tail exact, Tol-k, Tol-elpd, Tol-lppd).  The C-ABI returns elpd,
lppd, k, n_tail and the non-finite count per observation: the cutoff and the smoothed
log-weights themselves stay on the device, so they are checked on the host route
(test_loo_host.py) and, here, through n_tail, k and elpd, which they determine."""

import ctypes
import os

import numpy
import pytest

import psis_ref
import waic_ref
from gpu_cases import synthetic
from nestmc import _lib, loo
from nestmc.engine import Engine
from nestmc.families import DeviceLikelihood, LinearRegression
from oracle import restatement as rs

pytestmark = pytest.mark.gpu


def _psis_of(lib, store, n_valid, obs_batch=0, rc=False):
    """nmc_psis_of over the host array store[rows][n_obs][C]."""
    x = numpy.ascontiguousarray(store, dtype=numpy.float64)
    rows, n, C = x.shape
    elpd, lppd, k = (numpy.full(n, -7.0) for _ in range(3))
    nt = numpy.full(n, -7, dtype=numpy.int32)
    bad = numpy.full(n, -7, dtype=numpy.int64)
    code = lib.nmc_psis_of(0, _lib.dptr(x), rows, n, C, n_valid, obs_batch, _lib.dptr(elpd),
                           _lib.dptr(lppd), _lib.dptr(k),
                           nt.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                           bad.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)))
    out = dict(elpd=elpd, lppd=lppd, k=k, n_tail=nt, nonfinite=bad)
    if rc:
        return code, out
    _lib.check(code)
    return out


def _same(a, b):
    return all(a[f].tobytes() == b[f].tobytes() for f in ("elpd", "lppd", "k", "n_tail",
                                                          "nonfinite"))


def _to_store(ll):
    """Engine.obs_ll_rows' [C, rows, n_obs] as the store layout [rows][n_obs][C]."""
    return numpy.ascontiguousarray(numpy.transpose(ll, (1, 2, 0)))


def _check_matrix(got, ll, what):
    """Every observation of got against the reference over ll[C, rows, n_obs][:n_valid]."""
    n = ll.shape[2]
    for i in range(n):
        col = numpy.ascontiguousarray(ll[:, :, i].T).reshape(-1)     # s = row * n_valid + chain
        psis_ref.check("%s/%d" % (what, i), col, got["elpd"][i], got["lppd"][i], got["k"][i],
                       got["n_tail"][i], what="device")
    assert not got["nonfinite"].any()


# ---- 1. nmc_psis_of on injected columns ------------------------------------------------------
@pytest.mark.parametrize("sname", ["s4224", "s30", "s4160", "s6758400"])
def test_injected_columns(gpu_lib, sname):
    rows, C, nv, cols = psis_ref.cases()[sname]
    names = list(cols)
    got = _psis_of(gpu_lib, psis_ref.store(rows, C, nv, [cols[n] for n in names]), nv)
    assert not got["nonfinite"].any()          # (the NaN of the padding chains is never read)
    for i, n in enumerate(names):
        ref = psis_ref.check(sname + "/" + n, cols[n], got["elpd"][i], got["lppd"][i],
                             got["k"][i], got["n_tail"][i], what="device")
        if n == "t3":
            assert sname == "s30" or got["k"][i] > 0.7
        if n == "uniform":
            assert got["k"][i] < 0
        if n == "equal":
            assert got["n_tail"][i] == 0 and numpy.isposinf(got["k"][i])
        if n == "ties":
            assert got["n_tail"][i] == psis_ref.tail_length(rows * nv) - 10
        if n == "three":
            assert got["n_tail"][i] == 3 and numpy.isposinf(got["k"][i])
        if n.startswith("floor"):
            assert ref["cut"] == psis_ref.LOG_TINY
    if len(names) == 1:
        assert psis_ref.tail_length(rows * nv) * 8 + 3328 > 64 * 1024   # (a raised LDS limit)
        return
    # one observation at a time and a ragged last batch: the same bits
    assert _same(_psis_of(gpu_lib, psis_ref.store(rows, C, nv, [cols[n] for n in names]), nv,
                          obs_batch=1), got)
    assert _same(_psis_of(gpu_lib, psis_ref.store(rows, C, nv, [cols[n] for n in names]), nv,
                          obs_batch=2), got)


def test_nonfinite_columns(gpu_lib):
    rows, C, nv, cols = psis_ref.cases()["s4224"]
    a, b = cols["gauss"].copy(), cols["t3"].copy()
    a[1234] = -numpy.inf
    b[7], b[4100] = numpy.nan, numpy.inf
    names = ["gauss", "uniform", "t3"]
    got = _psis_of(gpu_lib, psis_ref.store(rows, C, nv, [cols["gauss"], a, cols["uniform"], b,
                                                       cols["t3"]]), nv)
    assert got["nonfinite"].tolist() == [0, 1, 0, 2, 0]
    for i in (1, 3):
        assert numpy.isnan(got["elpd"][i]) and numpy.isnan(got["lppd"][i])
        assert numpy.isnan(got["k"][i]) and got["n_tail"][i] == 0
    for i, n in zip((0, 2, 4), names):       # the other columns are unaffected
        psis_ref.check("s4224/" + n, cols[n], got["elpd"][i], got["lppd"][i], got["k"][i],
                       got["n_tail"][i], what="beside non-finite columns")


def test_psis_of_bad_arguments(gpu_lib):
    rows, C, nv, cols = psis_ref.cases()["s30"]
    st = psis_ref.store(rows, C, nv, [cols["gauss"]])
    for kw in (dict(n_valid=0), dict(n_valid=4), dict(obs_batch=-1)):
        code, out = _psis_of(gpu_lib, st, **dict(dict(n_valid=3, rc=True), **kw))
        assert code == -1, kw
        assert (out["elpd"] == -7.0).all() and (out["n_tail"] == -7).all()
    code, out = _psis_of(gpu_lib, st[:1, :, :1], 1, rc=True)             # S = 1
    assert code == -1 and (out["k"] == -7.0).all()
    code, out = _psis_of(gpu_lib, st[:, :0], 3, rc=True)                 # no observations
    assert code == -1
    assert b"loo" in gpu_lib.nmc_last_error()


# ---- 2. Engine.loo on small models -----------------------------------------------------------
def _state(fam, sizes, C, P, pooling, seed=5):
    r = numpy.random.RandomState(seed)
    G = len(sizes)
    value = r.normal(size=(C, P, G)) * 0.3
    lp = numpy.zeros((C, P, G))
    nested = rs.Nested(fam, sizes)
    ll = numpy.array([nested.group_ll(value[c]) for c in range(C)])
    mu = numpy.zeros((C, P)) if pooling == "partial" else None
    s2 = numpy.full((C, P), 0.5) if pooling == "partial" else None
    return value, lp, ll, mu, s2


def _run(fam, sizes, priors, pooling, C, n_iter, burn, thin, state=None, seed=3):
    st = state or _state(fam, sizes, C, fam.n_params, pooling)
    eng = Engine(fam, sizes, C, pooling, priors, seed=seed)
    eng.set_state(*st)
    eng.set_schedule(n_iter, burn, thin)
    eng.run(0, n_iter)
    eng.synchronize()
    return eng


SIZES = [1, 7, 9, 23]


def _linreg66():
    n = sum(SIZES)
    r = numpy.random.RandomState(3)
    x = r.normal(size=n)
    y = 0.5 + 2.0 * x + r.normal(size=n)
    return LinearRegression.simple(x, y, sigma=1.0)


@pytest.fixture(scope="module")
def eng66(gpu_lib):
    """Partial-pooling linreg, 66 chains, ragged groups, 64 recorded rows; its LL matrix and
    the results of the whole window, computed once."""
    eng = _run(_linreg66(), SIZES, None, "partial", 66, 148, 20, 2)
    assert eng.n_rows == 64
    ll = eng.obs_ll_rows()
    yield eng, ll, eng.loo_raw()
    eng.close()


def test_engine_linreg_partial(gpu_lib, eng66):
    eng, ll, got = eng66
    assert got["n_samples"] == 66 * 64 and len(got["elpd"]) == 40
    assert _same(_psis_of(gpu_lib, _to_store(ll), 66), got)      # nmc_k_loo_ll = obs_ll_rows
    _check_matrix(got, ll, "linreg66")
    res = eng.loo()
    assert eng.loo_nonfinite == 0
    assert res.elpd_i.tobytes() == got["elpd"].tobytes() and res.n_samples == 4224
    assert res.elpd_g.shape == (4,) and res.k_threshold == 0.7
    assert res.n_bad == int(numpy.sum(got["k"] > 0.7))
    assert numpy.all(res.p_loo_i > 0)


def test_engine_gauss_none(gpu_lib):
    fam, sizes, priors, pooling, _ = synthetic("gauss_none", 3, 4, 5)
    eng = _run(fam, sizes, priors, pooling, 3, 60, 20, 4)
    try:
        assert eng.n_rows == 10
        ll, got = eng.obs_ll_rows(), eng.loo_raw()
        assert _same(_psis_of(gpu_lib, _to_store(ll), 3), got)
        _check_matrix(got, ll, "gauss3")
    finally:
        eng.close()


def test_obs_batch_bit_identical(eng66):
    eng, _, got = eng66
    assert _same(eng.loo_raw(obs_batch=7), got)        # 40 = 5 * 7 + 5: a ragged last batch
    assert _same(eng.loo_raw(obs_batch=0), got)


def test_row_range_and_padding(gpu_lib, eng66):
    eng, ll, _ = eng66
    sub = eng.loo_raw(row_begin=5, n_rows=30)
    assert _same(_psis_of(gpu_lib, _to_store(ll[:, 5:35]), 66), sub)
    _check_matrix(sub, ll[:, 5:35], "linreg66 rows 5..34")
    pad = eng.loo_raw(n_valid=65)                     # the last chain as padding
    assert _same(_psis_of(gpu_lib, _to_store(ll), 65), pad)
    _check_matrix(pad, ll[:65], "linreg66 n_valid 65")


def test_engine_bad_arguments(eng66):
    eng, _, got = eng66
    for kw in (dict(n_rows=0), dict(row_begin=60, n_rows=5), dict(row_begin=-1, n_rows=2),
               dict(n_valid=0), dict(n_valid=67), dict(obs_batch=-1),
               dict(n_rows=1, n_valid=1)):
        with pytest.raises(_lib.NestmcError):
            eng.loo_raw(**kw)
    assert _same(eng.loo_raw(), got)                  # (the context still works)


# FamLinreg::obs_ll's own expression (csrc/families.h) for rows {x, y}, an intercept and a known
# sigma: numpy's row sum rounded term by term; k = {sigma, log sigma}
LINREG_USER = r"""
__device__ double nmc_user_loglik(const double* th, const double* row, const double* k) {
  double yh = th[0];
  yh = yh + row[0] * th[1];
  const double t = (yh - row[1]) / k[0];
  return (-(t * t) / 2.0 - NMC_LOG_C) - k[1];
}
"""


def test_user_family_bit_identical_to_builtin(gpu_lib):
    """nmc_k_loo_ll<FamUser> compiled at run time against the built-in linreg's instance, on
    bit-identical sample stores (the user family sums per-observation values where the
    built-in sums squares, so the stores are compared first)."""
    fam = _linreg66()
    st = _state(fam, SIZES, 66, 2, "partial")
    user = DeviceLikelihood(fam.obs(), LINREG_USER, 2, consts=[1.0, 0.0], host_function=fam)
    a = _run(fam, SIZES, None, "partial", 66, 60, 20, 4, state=st)
    b = _run(user, SIZES, None, "partial", 66, 60, 20, 4, state=st)
    try:
        assert a.samples_raw().tobytes() == b.samples_raw().tobytes()
        lla = a.obs_ll_rows()
        assert lla.tobytes() == b.obs_ll_rows().tobytes()
        assert _same(a.loo_raw(), b.loo_raw())
        assert _same(_psis_of(gpu_lib, _to_store(lla), 66), b.loo_raw(obs_batch=3))
    finally:
        a.close()
        b.close()


# ---- 3. samplePosterior(computeLoo=True) -----------------------------------------------------
def test_sample_posterior_compute_loo(gpu_lib, tmp_path):
    from nestmc.sampler import sample_posterior
    C, G, N = 70, 5, 30
    fam, sizes, priors, pooling, names = synthetic("linreg_partial", C, G, N)
    ranges = {n: [-0.5, 0.5] for n in names}
    kw = dict(saveLogLikelihood=False, priorDistribution=priors, startingPointValueRange=ranges,
              displayProgress=False, seed=17, return_samples=True, write_files=True)
    out = str(tmp_path / "one")
    res = sample_posterior(C, 60, 20, names, G, N, pooling, fam, out, computeLoo=True,
                           computeWaic=True, **kw)
    r, w = res["loo"], res["waic"]
    assert sorted(os.listdir(out)) == ["log", "loo.csv", "loo_pointwise.csv", "sample",
                                       "waic.csv", "waic_pointwise.csv"]
    assert open(os.path.join(out, "loo.csv")).readline().strip() == loo.HEADER
    v = numpy.loadtxt(os.path.join(out, "loo.csv"), delimiter=",", skiprows=1)
    assert v.tolist() == [r.looic, r.se_looic, r.elpd, r.se, r.p_loo, float(r.n_bad),
                          r.k_threshold, float(r.n_samples), 150.0]
    p = numpy.loadtxt(os.path.join(out, "loo_pointwise.csv"), delimiter=",", skiprows=1)
    assert numpy.array_equal(p[:, 1], numpy.repeat(numpy.arange(G), N))
    assert numpy.array_equal(p[:, 2:6], numpy.stack([r.lppd_i, r.p_loo_i, r.elpd_i, r.pareto_k],
                                                    1))
    S = r.n_samples
    assert S == w.n_samples and r.k_threshold == min(1 - 1 / numpy.log10(S), 0.7)
    # lppd is WAIC's within Tol-lppd (tests/waic_ref.py)
    tol = (S + 64) * waic_ref.U * (1 + numpy.abs(w.lppd_i))
    print("lppd loo vs waic: max err/tol %.3g" % numpy.max(numpy.abs(r.lppd_i - w.lppd_i) / tol))
    assert numpy.all(numpy.abs(r.lppd_i - w.lppd_i) <= tol)
    log = open(os.path.join(out, "log", "samplePosterior.log")).read()
    assert log.count("PSIS-LOO:") == (1 if r.n_bad else 0)
    # without files: the result alone
    mem = sample_posterior(C, 60, 20, names, G, N, pooling, fam, None, computeLoo=True,
                           **dict(kw, write_files=False))
    assert numpy.array_equal(mem["loo"].elpd_i, r.elpd_i)
    assert numpy.array_equal(mem["loo"].pareto_k, r.pareto_k)
    # off by default
    off = sample_posterior(C, 60, 20, names, G, N, pooling, fam, str(tmp_path / "off"), **kw)
    assert "loo" not in off and sorted(os.listdir(str(tmp_path / "off"))) == ["log", "sample"]
    # several engines: not yet
    with pytest.raises(NotImplementedError):
        sample_posterior(C, 60, 20, names, G, N, pooling, fam, str(tmp_path / "two"),
                         computeLoo=True, devices=[0, 0], **kw)
    assert not os.path.exists(str(tmp_path / "two"))
