"""nestmc.loo on the host: the formulas against the longdouble reference of tests/psis_ref.py,
the edge columns, a known answer of the fit, compare, the files and the signature."""

import inspect
import os

import numpy
import pytest

import psis_ref
from nestmc import loo, waic


def _columns():
    for sname, (rows, C, nv, cols) in psis_ref.cases().items():
        for cname, ll in cols.items():
            yield sname + "/" + cname, ll


@pytest.mark.parametrize("name", [n for n, _ in _columns()])
def test_column_against_longdouble(name):
    ll = dict(_columns())[name]
    got = loo.psis_column(ll)
    ref = psis_ref.check(name, ll, got["elpd"], got["lppd"], got["k"], got["n_tail"],
                         cut=got["cut"], lw_tail=got["lw_tail"], what="host")
    # the result depends on the multiset alone
    again = loo.psis_column(numpy.random.RandomState(1).permutation(ll))
    assert (again["elpd"], again["k"], again["n_tail"]) == (got["elpd"], got["k"], got["n_tail"])
    short = name.split("/")[1]
    if short.startswith("t3") and len(ll) > 1000:
        assert ref["k"] > 0.7
    if short == "uniform":
        assert ref["k"] < 0
    if short == "equal":
        assert got["n_tail"] == 0 and numpy.isposinf(got["k"])
        assert got["elpd"] == pytest.approx(-1.25, abs=1e-12)
    if short == "ties":
        assert got["n_tail"] == psis_ref.tail_length(len(ll)) - 10
    if short == "three":
        assert got["n_tail"] == 3 and numpy.isposinf(got["k"])
    if short.startswith("floor"):
        assert got["cut"] == psis_ref.LOG_TINY and got["n_tail"] < psis_ref.tail_length(len(ll))


def test_from_ll_matrix_and_totals():
    rows, C, nv, cols = psis_ref.cases()["s4224"]
    names = ["gauss", "t3", "uniform", "ties", "three"]
    ll = numpy.stack([cols[n] for n in names], axis=1)
    off = [0, 2, 5]
    res = loo.from_ll_matrix(ll, off)
    for i, n in enumerate(names):
        psis_ref.check("s4224/" + n, cols[n], res.elpd_i[i], res.lppd_i[i], res.pareto_k[i],
                       res.n_tail[i], what="from_ll_matrix")
    S = ll.shape[0]
    assert res.n_samples == S and res.n_obs == 5
    assert numpy.array_equal(res.p_loo_i, res.lppd_i - res.elpd_i)
    assert res.elpd == float(numpy.sum(res.elpd_i)) and res.looic == -2.0 * res.elpd
    assert res.p_loo == float(numpy.sum(res.p_loo_i))
    assert res.se == float(numpy.sqrt(5 * numpy.var(res.elpd_i, ddof=1)))
    assert res.elpd_g.tolist() == [numpy.sum(res.elpd_i[:2]), numpy.sum(res.elpd_i[2:])]
    assert res.p_loo_g.tolist() == [numpy.sum(res.p_loo_i[:2]), numpy.sum(res.p_loo_i[2:])]
    assert res.k_threshold == min(1 - 1 / numpy.log10(S), 0.7) == 0.7
    assert loo.k_threshold(30) == 1 - 1 / numpy.log10(30)
    # gauss (0.80), t3 (2.0) and the short tail (inf) are above the threshold
    assert res.n_bad == int(numpy.sum(res.pareto_k > 0.7)) == 3
    assert "3 of 5" in res.warning()
    # lppd is WAIC's
    w = waic.from_ll_matrix(ll, off)
    assert numpy.allclose(res.lppd_i, w.lppd_i, rtol=0, atol=1e-12)
    with pytest.raises(ValueError):
        loo.from_ll_matrix(ll[:1], off)
    bad = ll.copy()
    bad[3, 1] = numpy.nan
    with pytest.raises(ValueError):
        loo.from_ll_matrix(bad, off)


def test_gpd_known_answer():
    """2 000 draws of GPD(k = 0.5, sigma = 1) by inversion from RandomState(20).uniform: the
    fit returned k = 0.516388976914683, sigma = 0.96566596960955176 on the CPU this was
    written on (the estimator's standard error at n = 2 000 is about 0.03)."""
    u = numpy.random.RandomState(20).uniform(size=2000)
    x = numpy.sort(numpy.expm1(-0.5 * numpy.log1p(-u)) / 0.5)
    k, sigma = loo.gpdfit(x)
    print("gpdfit: k = %.17g sigma = %.17g" % (k, sigma))
    assert abs(k - K_GPD) <= 1e-9 and abs(k - 0.5) < 0.1
    assert abs(sigma - SIGMA_GPD) <= 1e-9 and abs(sigma - 1.0) < 0.1


K_GPD = 0.516388976914683
SIGMA_GPD = 0.96566596960955176


def test_compare():
    rows, C, nv, cols = psis_ref.cases()["s30"]
    ll = numpy.stack([cols[n] for n in ("gauss", "t3", "uniform")], axis=1)
    a = loo.from_ll_matrix(ll, [0, 3])
    b = loo.from_ll_matrix(ll[:, ::-1] * 1.1, [0, 3])
    d, se = loo.compare(a, b)
    d2, se2 = loo.compare(b, a)
    assert (d2, se2) == (-d, se) and se > 0
    assert d == float(numpy.sum(a.elpd_i - b.elpd_i))
    assert se == float(numpy.sqrt(3 * numpy.var(a.elpd_i - b.elpd_i, ddof=1)))
    assert loo.compare(a, a) == (0.0, 0.0)
    wa, wb = waic.from_ll_matrix(ll, [0, 3]), waic.from_ll_matrix(ll * 1.1, [0, 3])
    dw, sw = loo.compare(wa, wb)
    assert dw == -loo.compare(wb, wa)[0] and loo.compare(wa, wa) == (0.0, 0.0)
    with pytest.raises(TypeError):
        loo.compare(a, wa)


def test_csvs_read_back(tmp_path):
    rows, C, nv, cols = psis_ref.cases()["s30"]
    ll = numpy.stack([cols[n] for n in ("gauss", "t3", "uniform")] + [numpy.full(30, -2.0)],
                     axis=1)
    res = loo.from_ll_matrix(ll, [0, 1, 4])
    loo.write_csvs(res, str(tmp_path))
    assert open(os.path.join(str(tmp_path), "loo.csv")).readline().strip() == loo.HEADER
    v = numpy.loadtxt(os.path.join(str(tmp_path), "loo.csv"), delimiter=",", skiprows=1)
    assert v.tolist() == [res.looic, res.se_looic, res.elpd, res.se, res.p_loo, float(res.n_bad),
                          res.k_threshold, 30.0, 4.0]
    head = open(os.path.join(str(tmp_path), "loo_pointwise.csv")).readline().strip()
    assert head == loo.HEADER_POINTWISE
    p = numpy.loadtxt(os.path.join(str(tmp_path), "loo_pointwise.csv"), delimiter=",", skiprows=1)
    assert p[:, 0].tolist() == [0, 1, 2, 3] and p[:, 1].tolist() == [0, 1, 1, 1]
    assert numpy.array_equal(p[:, 2:6], numpy.stack([res.lppd_i, res.p_loo_i, res.elpd_i,
                                                     res.pareto_k], 1))
    assert numpy.isposinf(p[3, 5]) and p[:, 6].tolist() == res.n_tail.tolist()


def test_from_directory(tmp_path):
    rows, C, nv, cols = psis_ref.cases()["s30"]
    ll = numpy.round(numpy.stack([cols[n] for n in ("gauss", "t3")], axis=1), 6)
    os.makedirs(str(tmp_path / "sample"))
    for c in range(3):
        numpy.savetxt(str(tmp_path / "sample" / ("logLikelihood.%d.csv" % c)),
                      ll[c * 10:(c + 1) * 10], delimiter=",", fmt="%f")
    a, b = loo.from_directory(str(tmp_path), [0, 2]), loo.from_ll_matrix(ll, [0, 2])
    assert numpy.array_equal(a.elpd_i, b.elpd_i) and numpy.array_equal(a.pareto_k, b.pareto_k)


def test_compute_loo_in_the_signatures():
    import posteriorSampling
    from nestmc.sampler import sample_posterior
    for f in (posteriorSampling.samplePosterior, sample_posterior):
        p = inspect.signature(f).parameters["computeLoo"]
        assert p.default is False
