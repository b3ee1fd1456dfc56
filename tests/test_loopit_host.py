"""nestmc.loopit on the host: the formulas against the longdouble reference of
tests/loopit_ref.py, the exact identities, the weights, the files, the errors and the
signature."""

import inspect
import os

import numpy
import pytest

import loopit_ref
from nestmc import loo, loopit

FIELDS = ("ess", "wlt", "weq", "mean", "var")


def _got(e, col):
    return dict({f: e[f] for f in FIELDS}, n_tail=col["n_tail"])


@pytest.mark.parametrize("sname,cname", sorted({(s, c) for s, c, _ in loopit_ref.all_columns()}))
def test_column_against_longdouble(sname, cname):
    ll = loopit_ref.cases()[sname][3][cname]
    for kind in loopit_ref.KINDS:
        yrep, y = loopit_ref.replicates(sname, cname, len(ll))[kind]
        e, col = loopit.expect_column(ll, yrep, y)
        assert e["nonfinite_draws"] == 0
        loopit_ref.check(sname, cname, kind, _got(e, col), what="host")
        # the multiset of (ll, y_rep) pairs alone: one permutation of both, within rounding
        p = numpy.random.RandomState(2).permutation(len(ll))
        e2, col2 = loopit.expect_column(ll[p], yrep[p], y)
        loopit_ref.check(sname, cname, kind, _got(e2, col2), what="host permuted")


def test_psis_weights():
    for sname, cname in (("s4224", "gauss"), ("s4224", "three"), ("s4224", "equal"),
                         ("s4224", "tail5"), ("s30", "t3"), ("s4160", "floor_a")):
        ll = loopit_ref.cases()[sname][3][cname]
        w = loopit.psis_weights(ll)
        ref = loopit_ref.reference(sname, cname, "normal")[0]["w"]
        assert w.shape == ll.shape and numpy.all(w >= 0)
        assert abs(numpy.sum(w) - 1.0) <= 4 * len(ll) * loopit_ref.U
        # (a weight is a normalised indicator sum of one sample: Tol-pit)
        full, psis = loopit_ref.reference(sname, cname, "normal")[:2]
        assert float(numpy.max(numpy.abs(w - ref))) <= loopit_ref.tolerances(full, psis, len(ll),
                                                                             [1.0])[0]
    ll = loopit_ref.cases()["s4224"][3]["equal"]
    assert numpy.all(loopit.psis_weights(ll) == 1.0 / len(ll))


def test_tied_tail_samples_share_their_weight():
    ll = loopit_ref.cases()["s4224"][3]["tail5"]
    col = loo.psis_column(ll)
    o = numpy.argsort(ll, kind="stable")
    tied = o[20:25]
    assert numpy.all(ll[tied] == ll[tied[0]]) and col["n_tail"] > 25
    w = loopit.psis_weights(ll)
    assert len(set(w[tied].tolist())) == 1
    # the mean of their places' weights: between the neighbours'
    assert w[o[25]] < w[tied[0]] < w[o[19]]
    # swapping replicates among the tied samples changes no bit
    yrep, y = loopit_ref.replicates("s4224", "tail5", len(ll))["normal"]
    e, _ = loopit.expect_column(ll, yrep, y)
    for kind in loopit_ref.KINDS:
        yrep, y = loopit_ref.replicates("s4224", "tail5", len(ll))[kind]
        if kind == "binary":
            yrep = yrep.copy()
            yrep[tied] = [0.0, 1.0, 1.0, 0.0, 1.0]
        e, _ = loopit.expect_column(ll, yrep, y)
        sw = yrep.copy()
        sw[tied] = yrep[numpy.roll(tied, 2)]
        e2, _ = loopit.expect_column(ll, sw, y)
        print(kind, [(f, e[f], e2[f]) for f in FIELDS if e[f] != e2[f]])
        assert all(e[f] == e2[f] for f in FIELDS), kind


def _matrices():
    rows, C, nv, cols = loopit_ref.cases()["s30"]
    names = ["gauss", "t3", "uniform"]
    ll = numpy.stack([cols[n] for n in names] + [numpy.full(30, -2.0)], axis=1)
    reps = [loopit_ref.replicates("s30", n, 30)["normal"] for n in names]
    r = numpy.random.RandomState(4)
    yrep = numpy.stack([a for a, _ in reps] + [r.normal(size=30)], axis=1)
    y = numpy.array([b for _, b in reps] + [0.1])
    return names, ll, yrep, y


def test_from_matrices_and_summaries():
    names, ll, yrep, y = _matrices()
    off = [0, 1, 4]
    res = loopit.from_matrices(ll, yrep, y, off)
    for i, n in enumerate(names):
        loopit_ref.check("s30", n, "normal",
                         dict(ess=res.ess[i], wlt=res.wlt[i, 0], weq=res.weq[i, 0],
                              mean=res.loo_mean[i, 0], var=res.loo_var[i, 0],
                              n_tail=res.loo.n_tail[i]), what="from_matrices")
    want = loo.from_ll_matrix(ll, off)
    assert numpy.array_equal(res.loo.elpd_i, want.elpd_i)
    assert numpy.array_equal(res.pareto_k, want.pareto_k) and res.n_samples == 30
    assert numpy.array_equal(res.loo_pit, res.wlt + res.weq / 2.0)
    assert numpy.array_equal(res.loo_sd, numpy.sqrt(res.loo_var))
    assert numpy.array_equal(res.loo_residual, (res.y - res.loo_mean) / res.loo_sd)
    # the equal column: weights 1 / S, so the PIT is the plain mid-PIT and ess = S
    lt, eq = numpy.sum(yrep[:, 3] < y[3]), numpy.sum(yrep[:, 3] == y[3])
    assert res.loo_pit[3, 0] == (lt + eq / 2.0) / 30 and res.ess[3] == 30.0
    out = (res.loo_pit < 0.025) | (res.loo_pit > 0.975)
    assert res.n_outside == int(out.sum()) and res.n_pit == 4
    assert res.frac_outside == res.n_outside / 4.0
    assert res.n_outside_g.tolist() == [int(out[:1].sum()), int(out[1:].sum())]
    assert res.pit_mean_g.tolist() == [float(numpy.mean(res.loo_pit[:1])),
                                       float(numpy.mean(res.loo_pit[1:]))]
    u = numpy.sort(res.loo_pit.ravel())
    assert res.ks == max(max((k + 1) / 4.0 - u[k], u[k] - k / 4.0) for k in range(4))
    assert "expected 5 %" in res.summary() and "%d of 4" % res.n_outside in res.summary()
    # two response fields
    two = loopit.from_matrices(ll, numpy.stack([yrep, yrep + 1.0], axis=2),
                               numpy.stack([y, y + 1.0], axis=1), off)
    assert two.loo_pit.shape == (4, 2)
    assert numpy.array_equal(two.loo_pit[:, 0], res.loo_pit[:, 0])
    assert numpy.allclose(two.loo_pit[:, 1], res.loo_pit[:, 0], rtol=0, atol=1e-12)


def test_kolmogorov_distance():
    assert loopit.kolmogorov_distance([0.5]) == 0.5
    assert loopit.kolmogorov_distance([0.25, 0.75]) == 0.25
    assert loopit.kolmogorov_distance([1.0, 1.0, numpy.nan]) == 1.0
    assert numpy.isnan(loopit.kolmogorov_distance([numpy.nan]))


def test_nonfinite_and_value_errors():
    names, ll, yrep, y = _matrices()
    off = [0, 1, 4]
    bad = yrep.copy()
    bad[3, 1], bad[7, 1], bad[9, 2] = numpy.nan, numpy.inf, -numpy.inf
    res = loopit.from_matrices(ll, bad, y, off)
    assert res.nonfinite_draws[:, 0].tolist() == [0, 2, 1, 0]
    for f in (res.wlt, res.weq, res.loo_pit, res.loo_mean, res.loo_sd, res.loo_residual):
        assert numpy.isnan(f[1:3, 0]).all() and numpy.isfinite(f[[0, 3], 0]).all()
    assert numpy.isfinite(res.ess).all() and res.n_pit == 2
    with pytest.raises(ValueError, match="two samples"):
        loopit.from_matrices(ll[:1], yrep[:1], y, off)
    nan = ll.copy()
    nan[3, 1] = numpy.nan
    with pytest.raises(ValueError, match="not finite"):
        loopit.from_matrices(nan, yrep, y, off)
    with pytest.raises(ValueError):
        loopit.from_matrices(ll, yrep[:, :3], y, off)
    with pytest.raises(ValueError):
        loopit.from_matrices(ll, yrep, y[:3], off)
    with pytest.raises(ValueError):
        loopit.from_matrices(ll[:, 0], yrep, y, off)
    with pytest.raises(ValueError):
        loopit.from_matrices(ll, yrep, y, [0, 1, 3])


def test_csvs_read_back(tmp_path):
    names, ll, yrep, y = _matrices()
    res = loopit.from_matrices(ll, yrep, y, [0, 1, 4])
    loopit.write_csvs(res, str(tmp_path))
    assert sorted(os.listdir(str(tmp_path))) == ["loo_pit_groups.csv", "loo_pit_pointwise.csv"]
    path = os.path.join(str(tmp_path), "loo_pit_pointwise.csv")
    assert open(path).readline().strip() == loopit.HEADER_POINTWISE == \
        "obs,group,field,y,loo_mean,loo_sd,loo_residual,loo_pit,wlt,weq,ess,pareto_k"
    p = numpy.loadtxt(path, delimiter=",", skiprows=1)
    assert p[:, 0].tolist() == [0, 1, 2, 3] and p[:, 1].tolist() == [0, 1, 1, 1]
    assert p[:, 2].tolist() == [0, 0, 0, 0]
    want = numpy.stack([res.y[:, 0], res.loo_mean[:, 0], res.loo_sd[:, 0], res.loo_residual[:, 0],
                        res.loo_pit[:, 0], res.wlt[:, 0], res.weq[:, 0], res.ess, res.pareto_k], 1)
    assert numpy.array_equal(p[:, 3:], want)          # (%.17g reads back exactly; k = inf too)
    assert numpy.isposinf(p[3, 11])
    path = os.path.join(str(tmp_path), "loo_pit_groups.csv")
    assert open(path).readline().strip() == loopit.HEADER_GROUPS
    g = numpy.loadtxt(path, delimiter=",", skiprows=1)
    assert numpy.array_equal(g, numpy.stack([[0, 1], res.n_g, res.pit_mean_g, res.n_outside_g], 1))


def test_compute_loo_pit_in_the_signatures():
    import posteriorSampling
    from nestmc.sampler import sample_posterior
    for f in (posteriorSampling.samplePosterior, sample_posterior):
        assert inspect.signature(f).parameters["computeLooPit"].default is False


def test_sample_posterior_refuses_before_sampling(tmp_path):
    """The pre-sampling checks need no GPU: several engines, a family that cannot draw, fewer
    than two samples."""
    from nestmc.families import DeviceLikelihood, LinearRegression
    from nestmc.sampler import sample_posterior
    r = numpy.random.RandomState(0)
    x, yy = r.normal(size=6), r.normal(size=6)
    fam = LinearRegression.simple(x, yy, sigma=1.0)
    names = ("a", "b")
    out = str(tmp_path / "o")
    for kw in (dict(devices=[0, 0]), dict(chains=[0, 1]), dict(process_per_device=True)):
        with pytest.raises(NotImplementedError, match="computeLooPit"):
            sample_posterior(4, 20, 5, names, 2, 3, "partial", fam, out, computeLooPit=True, **kw)
    src = "__device__ double nmc_user_loglik(const double* t, const double* r, const double* k)" \
          " { return 0.0; }"
    plain = DeviceLikelihood(numpy.stack([x, yy], 1), src, 2)
    assert plain.response_fields() == []
    with pytest.raises(ValueError, match="nmc_user_predict"):
        sample_posterior(4, 20, 5, names, 2, 3, "partial", plain, out, computeLooPit=True)
    assert not os.path.exists(out)
