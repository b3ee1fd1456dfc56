"""WAIC on the GPU: nmc_k_waic's reduction of the per-observation log-likelihood over the
device sample store, through Engine.waic / waic_partials and samplePosterior(computeWaic).

Reference and tolerances (Tol-lppd, Tol-M2): tests/waic_ref.py -- the longdouble formulas
over the device's own LL matrix (Engine.obs_ll_rows), or over the reference callable
(oracle.restatement.Nested.obs_ll) with the 1e-12 relative agreement test_gpu_outputs.py
grants it.  Engines as in test_gpu_outputs.py: set_schedule(60, 20, 4), 10 recorded rows.
"""

import os

import numpy
import pytest

import user_models
import waic_ref
from gpu_cases import synthetic
from nestmc import _lib, waic
from nestmc.engine import Engine
from nestmc.families import DeviceLikelihood, LinearRegression
from oracle import restatement as rs

pytestmark = pytest.mark.gpu

T = 8   # csrc/waic.h NMC_WAIC_T: observations per tile


def _state(fam, sizes, C, P, pooling, seed=5):
    r = numpy.random.RandomState(seed)
    G = len(sizes)
    value = r.normal(size=(C, P, G)) * 0.3
    if fam.family == "linreg" and P == 3:
        value[:, 2] = 1.0 + numpy.abs(value[:, 2])     # sigma > 0
    lp = numpy.zeros((C, P, G))
    nested = rs.Nested(fam, sizes)
    ll = numpy.array([nested.group_ll(value[c]) for c in range(C)])
    mu = numpy.zeros((C, P)) if pooling == "partial" else None
    s2 = numpy.full((C, P), 0.5) if pooling == "partial" else None
    return value, lp, ll, mu, s2, nested


def _run(fam, sizes, priors, pooling, C, seed=3, sel=None, chain_base=0, state=None):
    """An engine after 60 iterations (10 rows) on chains sel of the C-chain state."""
    st = state or _state(fam, sizes, C, fam.n_params, pooling)
    sel = numpy.arange(C) if sel is None else numpy.asarray(sel)
    eng = Engine(fam, sizes, len(sel), pooling, priors, seed=seed, chain_base=chain_base)
    pick = lambda a: None if a is None else a[sel]   # noqa: E731
    eng.set_state(*(pick(a) for a in st[:5]))
    eng.set_schedule(60, 20, 4)
    eng.run(0, 60)
    eng.synchronize()
    assert eng.n_rows == 10
    return eng, st


def _matrix(eng, rows=slice(None), chains=slice(None)):
    """The device's own LL matrix [S, n_obs] of the given rows and chains."""
    ll = eng.obs_ll_rows()[chains, rows]
    return ll.reshape(-1, ll.shape[-1])


@pytest.fixture(scope="module")
def eng70(gpu_lib):
    fam, sizes, priors, pooling, _ = synthetic("linreg_partial", 70, 5, 30)
    eng, st = _run(fam, sizes, priors, pooling, 70)
    yield eng, st[5]
    eng.close()


@pytest.fixture(scope="module")
def eng65(gpu_lib):
    fam, sizes, priors, pooling, _ = synthetic("gauss_none", 65, 4, 25)
    eng, st = _run(fam, sizes, priors, pooling, 65)
    yield eng, st[5]
    eng.close()


def _check_engine(eng, what):
    res = eng.waic()
    assert eng.waic_nonfinite == 0
    assert res.n_samples == eng.C * eng.n_rows
    waic_ref.check(res, _matrix(eng), what=what)
    parts = eng.waic_partials()
    assert parts.shape == ((eng.C + 63) // 64, 5, int(eng.off[-1]))
    return res


# ---- 1. the reduction against the device LL matrix ---------------------------------------
def test_linreg_partial(eng70):
    res = _check_engine(eng70[0], "linreg_partial")
    assert res.elpd_g.shape == (5,)
    assert abs(res.elpd_g.sum() - res.elpd) <= res.n_obs * waic_ref.U * numpy.abs(res.elpd_i).sum()


def test_gauss_none(eng65):
    _check_engine(eng65[0], "gauss_none")


@pytest.mark.parametrize("kind,C,G,N", [("linreg_complete", 3, 1, 200),
                                        ("logistic_partial", 64, 3, 20),
                                        ("regression3_none", 70, 4, 20)])
def test_other_families(gpu_lib, kind, C, G, N):
    fam, sizes, priors, pooling, _ = synthetic(kind, C, G, N)
    eng, _ = _run(fam, sizes, priors, pooling, C)
    try:
        _check_engine(eng, kind)
    finally:
        eng.close()


def test_ragged_groups(gpu_lib):
    fam, sizes, priors, pooling, _ = synthetic("linreg_partial", 70, 5, 30, ragged=True)
    eng, _ = _run(fam, sizes, priors, pooling, 70)
    try:
        _check_engine(eng, "ragged %s" % (sizes,))
    finally:
        eng.close()


def test_group_sizes_around_a_tile(gpu_lib):
    """A one-row group and groups of T - 1, T, T + 1 and 2 T + 1 rows."""
    sizes = [1, T - 1, T, T + 1, 2 * T + 1]
    n = sum(sizes)
    r = numpy.random.RandomState(3)
    x = r.normal(size=n)
    y = 0.5 + 2.0 * x + r.normal(size=n)
    fam = LinearRegression.simple(x, y, sigma=1.0)
    eng, _ = _run(fam, sizes, None, "partial", 70)
    try:
        _check_engine(eng, "sizes %s" % (sizes,))
    finally:
        eng.close()


# ---- 2. independent of the device's own LL -------------------------------------------------
def _callable_matrix(eng, nested):
    rows = eng.samples()                                  # [C, rows, cols]
    P, G = eng.P, eng.G
    pc = 2 if eng.pooling == "partial" else 0
    out = []
    for c in range(eng.C):
        for r in range(eng.n_rows):
            theta = numpy.stack([rows[c, r, q * (G + pc) + pc:(q + 1) * (G + pc)]
                                 for q in range(P)])
            out.append(nested.obs_ll(theta))
    return numpy.array(out)


def test_against_reference_callable_linreg(eng70):
    eng, nested = eng70
    waic_ref.check(eng.waic(), _callable_matrix(eng, nested), rel_ll=1e-12, what="callable linreg")


def test_against_reference_callable_gauss(eng65):
    eng, nested = eng65
    waic_ref.check(eng.waic(), _callable_matrix(eng, nested), rel_ll=1e-12, what="callable gauss")


# ---- 3. row range, single row, errors -----------------------------------------------------
def test_row_range(eng70):
    eng = eng70[0]
    res = eng.waic(row_begin=3, n_rows=4)
    assert res.n_samples == 70 * 4
    waic_ref.check(res, _matrix(eng, rows=slice(3, 7)), what="rows 3..6")
    waic_ref.check(eng.waic(row_begin=9), _matrix(eng, rows=slice(9, 10)), what="last row")


def test_single_row(eng65):
    eng = eng65[0]
    res = eng.waic(row_begin=2, n_rows=1)
    assert res.n_samples == 65
    waic_ref.check(res, _matrix(eng, rows=slice(2, 3)), what="one row")


def test_bad_arguments(eng70):
    eng = eng70[0]
    for kw in (dict(n_rows=0), dict(row_begin=8, n_rows=3), dict(row_begin=-1, n_rows=2),
               dict(row_begin=10, n_rows=1), dict(n_valid=0), dict(n_valid=71)):
        with pytest.raises(_lib.NestmcError):
            eng.waic_partials(**kw)
    assert eng.waic_partials().shape == (2, 5, 150)        # (the context still works)


# ---- 4. padding chains ----------------------------------------------------------------------
@pytest.mark.parametrize("n_valid", [64, 67])
def test_padding(eng70, n_valid):
    eng = eng70[0]
    parts = eng.waic_partials(n_valid=n_valid)
    res = waic.finish(waic.merge(list(parts)), eng.off)
    assert res.n_samples == n_valid * 10
    waic_ref.check(res, _matrix(eng, chains=slice(0, n_valid)), what="n_valid %d" % n_valid)
    if n_valid == 64:
        assert parts[1].tobytes() == waic.identity(150).tobytes()
    full = eng.waic_partials()
    assert parts[0].tobytes() == full[0].tobytes()         # (block 0 has no padding either way)


# ---- 5. sharding ------------------------------------------------------------------------------
def test_shards_of_whole_chain_blocks_bit_identical(gpu_lib):
    fam, sizes, priors, pooling, _ = synthetic("linreg_partial", 128, 3, 20)
    st = _state(fam, sizes, 128, 2, pooling)
    a, _ = _run(fam, sizes, priors, pooling, 128, state=st)
    b1, _ = _run(fam, sizes, priors, pooling, 128, state=st, sel=range(0, 64))
    b2, _ = _run(fam, sizes, priors, pooling, 128, state=st, sel=range(64, 128), chain_base=64)
    try:
        pa, p1, p2 = a.waic_partials(), b1.waic_partials(), b2.waic_partials()
        assert pa.shape[0] == 2 and p1.shape[0] == p2.shape[0] == 1
        assert p1[0].tobytes() == pa[0].tobytes() and p2[0].tobytes() == pa[1].tobytes()
        assert waic.merge(list(p1) + list(p2)).tobytes() == waic.merge(list(pa)).tobytes()
    finally:
        for e in (a, b1, b2):
            e.close()


def test_uneven_shards_within_tolerance(eng70):
    eng = eng70[0]
    fam, sizes, priors, pooling, _ = synthetic("linreg_partial", 70, 5, 30)
    st = _state(fam, sizes, 70, 2, pooling)
    b1, _ = _run(fam, sizes, priors, pooling, 70, state=st, sel=range(0, 3))
    b2, _ = _run(fam, sizes, priors, pooling, 70, state=st, sel=range(3, 70), chain_base=3)
    try:
        assert numpy.array_equal(numpy.concatenate([b1.samples(), b2.samples()]), eng.samples())
        merged = waic.merge(list(b1.waic_partials()) + list(b2.waic_partials()))
        waic_ref.check(waic.finish(merged, eng.off), _matrix(eng), what="3 + 67 chains")
    finally:
        b1.close()
        b2.close()


# ---- 6. a run-time-compiled user family ---------------------------------------------------
# FamLogistic::obs_ll's own expression (csrc/families.h): the reference's numpy row sum,
# eta = b0 + x1 b1 + ... rounded term by term, not the fma chain of its group sums
LOGISTIC4_OBS = r"""
__device__ double nmc_user_loglik(const double* th, const double* row, const double* k) {
  double eta = th[0];
  for (int j = 0; j < 3; ++j) eta = eta + row[j] * th[j + 1];
  return row[3] * eta - nmc_logaddexp0(eta);
}
"""


def test_user_family_bit_identical_to_builtin(gpu_lib):
    """nmc_k_waic<FamUser> compiled at run time against the built-in Logistic's instance, on
    bit-identical sample stores.  The user source restates FamLogistic::obs_ll (the unfused
    row sum).  tests/user_models.LOGISTIC4 restates the fma chain of the GROUP sums instead:
    it shares the built-in's samples bit for bit but its per-observation values differ from
    obs_ll in the last place (test_gpu_user.py compares those to 2e-6 only; measured on an
    MI355X: 46 of the 300 partial words differ from the built-in's, by at most 2.3e-13), so
    its partials are checked against its own LL matrix within Tol-lppd / Tol-M2."""
    fam, sizes, priors, pooling, _ = synthetic("logistic_partial", 64, 3, 20)
    st = _state(fam, sizes, 64, 4, pooling)
    user = DeviceLikelihood(fam.obs(), LOGISTIC4_OBS, 4, host_function=fam)
    fma = DeviceLikelihood(fam.obs(), user_models.LOGISTIC4, 4, host_function=fam)
    a, _ = _run(fam, sizes, priors, pooling, 64, state=st)
    b, _ = _run(user, sizes, priors, pooling, 64, state=st)
    c, _ = _run(fma, sizes, priors, pooling, 64, state=st)
    try:
        assert a.samples_raw().tobytes() == b.samples_raw().tobytes()
        assert a.obs_ll_rows().tobytes() == b.obs_ll_rows().tobytes()
        pa, pb = a.waic_partials(), b.waic_partials()
        assert pa.tobytes() == pb.tobytes()
        assert a.samples_raw().tobytes() == c.samples_raw().tobytes()
        _check_engine(c, "user logistic (fma chain)")
        pc = c.waic_partials()
        print("user_models.LOGISTIC4 against the built-in: %d of %d partial words differ, "
              "max abs difference %.3g" % (numpy.sum(pa != pc), pa.size,
                                           numpy.max(numpy.abs(pa - pc))))
    finally:
        for e in (a, b, c):
            e.close()


# ---- 7. samplePosterior(computeWaic=True) -------------------------------------------------
def test_sample_posterior_compute_waic(gpu_lib, tmp_path):
    from nestmc.init import init_chains
    from nestmc.sampler import sample_posterior, schedule
    C, G, N = 70, 5, 30
    fam, sizes, priors, pooling, names = synthetic("linreg_partial", C, G, N)
    ranges = {n: [-0.5, 0.5] for n in names}
    kw = dict(saveLogLikelihood=False, priorDistribution=priors, startingPointValueRange=ranges,
              displayProgress=False, seed=17, return_samples=True, write_files=True)
    out = str(tmp_path / "one")
    res = sample_posterior(C, 60, 20, names, G, N, pooling, fam, out, computeWaic=True, **kw)
    w = res["waic"]
    assert sorted(os.listdir(out)) == ["log", "sample", "waic.csv", "waic_pointwise.csv"]
    assert not [f for f in os.listdir(os.path.join(out, "sample")) if f.startswith("logLik")]
    head = open(os.path.join(out, "waic.csv")).readline().strip()
    assert head == "waic,se_waic,elpd,se_elpd,p_waic,n_samples,n_obs"
    v = numpy.loadtxt(os.path.join(out, "waic.csv"), delimiter=",", skiprows=1)
    assert v.tolist() == [w.waic, w.se_waic, w.elpd, w.se, w.p_waic, float(w.n_samples), 150.0]
    p = numpy.loadtxt(os.path.join(out, "waic_pointwise.csv"), delimiter=",", skiprows=1)
    assert numpy.array_equal(p[:, 1], numpy.repeat(numpy.arange(G), N))
    assert numpy.array_equal(p[:, 2:], numpy.stack([w.lppd_i, w.p_waic_i, w.elpd_i], 1))
    # an Engine run of the same seed and start
    burn, thin = schedule(60, 20)
    eng = Engine(fam, sizes, C, pooling, priors, seed=17)
    try:
        st = init_chains(fam, sizes, names, list(range(C)), pooling, priors, ranges, False,
                         group_ll=eng.eval_group_ll)
        eng.set_state(st["value"], st["log_prior"], st["ll"], st["mu"], st["s2"])
        eng.set_schedule(60, burn, thin, 100)
        eng.run(0, 60)
        eng.synchronize()
        assert numpy.array_equal(eng.samples(), res["rows"])
        ll = _matrix(eng)
        assert w.n_samples == C * eng.n_rows
        waic_ref.check(w, ll, what="samplePosterior")
        waic_ref.check(eng.waic(), ll, what="its Engine run")
    finally:
        eng.close()
    # two engines on one GPU: 35 + 35 chains
    two = sample_posterior(C, 60, 20, names, G, N, pooling, fam, str(tmp_path / "two"),
                           computeWaic=True, devices=[0, 0], **kw)
    assert numpy.array_equal(two["rows"], res["rows"])
    waic_ref.check(two["waic"], ll, what="devices=[0, 0]")
    # without files: the result alone
    mem = sample_posterior(C, 60, 20, names, G, N, pooling, fam, None, computeWaic=True,
                           **dict(kw, write_files=False))
    assert numpy.array_equal(mem["waic"].elpd_i, w.elpd_i) and mem["waic"].waic == w.waic
    # off by default: the output directory is what it was
    off = sample_posterior(C, 60, 20, names, G, N, pooling, fam, str(tmp_path / "off"), **kw)
    assert "waic" not in off
    assert sorted(os.listdir(str(tmp_path / "off"))) == ["log", "sample"]
    assert sorted(os.listdir(str(tmp_path / "off" / "sample"))) == \
        sorted(os.listdir(os.path.join(out, "sample")))


def test_process_per_device_rank_path(gpu_lib, tmp_path):
    """process_per_device: the rank reduces its chains, sends its merged partial over the
    host group and rank 0 finishes and writes -- with one rank (one device here) the files
    and the result are the in-process path's bit for bit.  The rank-order merge of several
    ranks' partials, padding ranks included, is covered on the host (test_waic_host.py)."""
    from nestmc.sampler import sample_posterior
    C, G, N = 70, 5, 30
    fam, sizes, priors, pooling, names = synthetic("linreg_partial", C, G, N)
    kw = dict(saveLogLikelihood=False, priorDistribution=priors, computeWaic=True,
              startingPointValueRange={n: [-0.5, 0.5] for n in names}, displayProgress=False,
              seed=23, return_samples=True, devices=[0])
    one, ppd = str(tmp_path / "one"), str(tmp_path / "ppd")
    r1 = sample_posterior(C, 60, 20, names, G, N, pooling, fam, one, **kw)
    r2 = sample_posterior(C, 60, 20, names, G, N, pooling, fam, ppd, process_per_device=True,
                          **kw)
    assert numpy.array_equal(r1["rows"], r2["rows"])
    for k in ("lppd_i", "p_waic_i", "elpd_i", "elpd_g", "p_waic_g"):
        assert numpy.array_equal(getattr(r1["waic"], k), getattr(r2["waic"], k)), k
    assert (r1["waic"].waic, r1["waic"].se, r1["waic"].n_samples) == \
        (r2["waic"].waic, r2["waic"].se, r2["waic"].n_samples)
    for fn in ("waic.csv", "waic_pointwise.csv"):
        assert open(os.path.join(one, fn), "rb").read() == open(os.path.join(ppd, fn), "rb").read()
