"""nestmc.rankdiag on the host: the normal score's restatement against mpmath, the exact
quantities, the restated device route against the host route within the derived bounds, and
the conditions the diagnostics must meet (tests/rankdiag_ref.py has the bounds)."""

import numpy
import pytest
from scipy.special import ndtri

import convergence_ref as cr
import rankdiag_ref as rr
from nestmc import convergence as conv
from nestmc import rankdiag as rd
from test_convergence_host import ar1, rows_of


# ---- the normal score ----------------------------------------------------------------------
def test_ndtri_restatement_against_mpmath():
    p = numpy.unique(rr.probe_p())
    assert p.min() < 2e-5 and p.max() > 1 - 2e-5 and numpy.any(p == 0.5)
    ra = rr.ratio_to_exact(rr.ndtri_as241(p), p)
    rs = rr.ratio_to_exact(ndtri(p), p)
    print("ndtri on %d p: restatement worst %.3g u at p = %r, scipy worst %.3g u"
          % (len(p), ra.max(), p[ra.argmax()], rs.max()))
    assert ra.max() <= rr.NDTRI_C / 8
    assert rs.max() <= rr.NDTRI_C / 8
    z0 = rr.ndtri_as241(numpy.array([0.5]))
    assert z0[0] == 0.0 and not numpy.signbit(z0[0])


# ---- the exact quantities ------------------------------------------------------------------
@pytest.mark.parametrize("rows,nv", [(4, 1), (18, 1), (100, 7), (34, 3)])
def test_derive_host_is_the_restatement(rows, nv):
    xs = rr.store(rows, nv, nv, seed=rows)                      # (derive_host: all chains real)
    want = rr.derive(xs, nv)
    derived, r2, bad = rd.derive_host(numpy.transpose(xs, (2, 0, 1)))
    t = lambda a: numpy.transpose(a, (1, 2, 0))                 # noqa: E731  [C][R][K] -> store
    assert numpy.array_equal(t(r2[0]), want["twice_rank"][0])
    assert numpy.array_equal(t(r2[1]), want["twice_rank"][1])
    assert numpy.array_equal(bad, want["nonfinite"]) and list(bad[-2:]) == [1, 1]
    assert numpy.array_equal(t(derived[2]), want["I05"], equal_nan=True)
    assert numpy.array_equal(t(derived[3]), want["I95"], equal_nan=True)
    ok = bad == 0
    assert numpy.array_equal(t(derived[0])[:, ok], ndtri(want["p"][:, ok]))
    assert numpy.array_equal(t(derived[1])[:, ok], ndtri(want["pf"][:, ok]))
    assert numpy.all(numpy.isnan(derived[:, :, :, ~ok]))
    assert numpy.all(t(derived[0])[:, 2] == 0.0)                # the constant column: p = 1/2
    # the -0.0 / +0.0 mix ties: every zero has one rank
    z = xs[:, 5, :nv]
    assert len(numpy.unique(want["twice_rank"][0][:, 5, :nv][z == 0])) == 1


def test_indicator_is_numpy_quantile_lower():
    r = numpy.random.RandomState(3)
    for N in (20, 21, 40, 1000, 7000):
        x = numpy.round(r.normal(size=N), 1)
        r2, lo = rr.twice_rank(x)
        for kq, q in (((N - 1) // 20, 0.05), (19 * (N - 1) // 20, 0.95)):
            s = numpy.sort(x)
            assert numpy.array_equal(lo <= kq, x <= s[kq])
            if (N - 1) % 20 == 0:      # (where the float product q (N - 1) is an integer for sure)
                assert s[kq] == numpy.quantile(x, q, method="lower")


# ---- the restated device route against the host route ----------------------------------------
def restated_route(rows, names=None):
    """The device route on the host: rr.derive's exact quantities, ndtri_as241's scores,
    convergence_ref.partials per quantity, rankdiag.finish."""
    C, R, K = rows.shape
    xs = numpy.ascontiguousarray(numpy.transpose(rows, (1, 2, 0)))
    d = rr.derive(xs, C)
    with numpy.errstate(invalid="ignore"):
        q = [rr.ndtri_as241(d["p"].ravel()).reshape(d["p"].shape),
             rr.ndtri_as241(d["pf"].ravel()).reshape(d["p"].shape), d["I05"], d["I95"]]
    parts = [cr.partials(numpy.ascontiguousarray(numpy.transpose(a, (2, 0, 1)))) for a in q]
    vg, mean, m2 = (numpy.stack([p[i] for p in parts]) for i in range(3))
    return rd.finish(vg, mean, m2, R // 2, names, C, d["nonfinite"])


def check_routes(dev, host, rows, CB, what):
    """dev (device route, or its restatement) against host (from_rows of the same rows):
    equal cutoffs T, V, rhat and ESS of every derived column within the bounds.  Returns the
    worst err/bound ratios."""
    worst = {}
    derived = rd.derive_host(rows)[0]
    for t, q in enumerate(rd.QUANTITIES):
        a, b = dev.parts[q], host.parts[q]
        x = conv.halfchains(derived[t])
        if t < 2:
            tol = rr.tolerances_z(x, CB)
        else:                      # exact data: convergence_ref's bounds as they stand
            tol = cr.tolerances(x, CB)
            tol["ess_rel"] = tol["neff_rel"]
        assert numpy.array_equal(a.T, b.T), (what, q, a.T, b.T)
        assert numpy.array_equal(a.T, rr.cutoffs_longdouble(x)), (what, q)
        for name in ("V", "rhat"):
            err = numpy.abs(getattr(a, name) - getattr(b, name))
            bound = numpy.asarray(tol[name], dtype=numpy.float64)
            ok = bound > 0
            worst[q, name] = float(numpy.max(err[ok] / bound[ok])) if ok.any() else 0.0
            assert numpy.all(err <= bound), (what, q, name, worst[q, name])
        tau_a, tau_b = dev.tau[t], host.tau[t]
        rel = numpy.abs(tau_a - tau_b) / numpy.abs(tau_b)
        bound = tol["ess_rel"](b.T, dev.N / tau_b)
        worst[q, "tau"] = float(numpy.max(rel / bound))
        assert numpy.all(rel <= bound), (what, q, "tau", worst[q, "tau"])
    print("rank diagnostics %s: worst err/bound %s" % (
        what, ", ".join("%s %s %.3g" % (k[0], k[1], v) for k, v in sorted(worst.items()))))
    for name in ("converged", "enough"):
        assert numpy.array_equal(getattr(dev, name), getattr(host, name)), (what, name)
    return worst


@pytest.mark.parametrize("K,m,n,seed", [(6, 140, 5, 21), (4, 140, 50, 22)])
def test_restated_device_route_against_host_route(K, m, n, seed):
    """The shapes of the GPU comparison (70 chains, 10 and 100 rows): the float64 routes and
    the longdouble formulas cut at the same T for these seeds, and the routes agree within
    the bounds."""
    rows = rows_of(ar1(K, m, n, seed))
    dev, host = restated_route(rows), rd.from_rows(rows)
    check_routes(dev, host, rows, (m // 2 + 63) // 64, "x[%d][%d][%d]" % (K, m, n))


# ---- the conditions --------------------------------------------------------------------------
def _iid(C, R, seed):
    return numpy.random.RandomState(seed).normal(size=(C, R, 1))


def test_ess_identity():
    """On the same partials N / ess = N / effective_n - 2 (effective_n's sum starts at lag 0,
    where rho is 1) whenever the floor 1 / log10 N is not active."""
    rows = rows_of(ar1(5, 140, 50, 31))
    res = rd.from_rows(rows)
    N = res.N
    for t, q in enumerate(rd.QUANTITIES):
        neff = res.parts[q].effective_n
        tau = res.tau[t]
        active = tau < 1.0 / numpy.log10(N)
        assert not active.all()
        ess = N / tau
        lhs, rhs = N / ess[~active], N / neff[~active] - 2
        assert numpy.all(numpy.abs(lhs - rhs) <= 8 * cr.U * (numpy.abs(rhs) + 2)), (q, lhs, rhs)
    assert numpy.array_equal(res.ess_bulk, N / numpy.maximum(res.tau[0], 1 / numpy.log10(N)))


def test_independent_draws():
    res = rd.from_rows(_iid(70, 100, 9))        # (a seed whose sum has lags: T = 4)
    assert res.parts["z"].T[0] > 0 and res.tau[0][0] != 1.0
    print("independent 70 x 100: ess_bulk %.1f of %d, ess_tail %.1f, effective_n %.1f"
          % (res.ess_bulk[0], res.N, res.ess_tail[0], res.parts["z"].effective_n[0]))
    assert abs(res.ess_bulk[0] - 7000) <= 700
    assert res.rhat[0] < 1.01 and res.converged[0] and res.enough[0]
    assert res.parts["z"].effective_n[0] < 7000 / 2.5          # (the reference's N / 3)


@pytest.mark.parametrize("C,R", [(70, 100), (4, 200)])
def test_scale_column(C, R):
    """Half the chains at scale 1, half at scale 3: the location agrees, the scale does not."""
    rows = _iid(C, R, 2)
    rows[C // 2:] *= 3.0
    res = rd.from_rows(rows)
    old = conv.from_halfchains(conv.halfchains(rows), variogram=conv.variogram_host)
    print("scale column %d x %d: rhat %.3f on the values, bulk %.3f, folded %.3f"
          % (C, R, old.rhat[0], res.rhat_bulk[0], res.rhat_folded[0]))
    assert res.rhat_bulk[0] < 1.01 and res.rhat_folded[0] > 1.1
    assert res.rhat[0] == res.rhat_folded[0] and not res.converged[0]
    assert old.rhat[0] < 1.01


def test_cauchy_column():
    rows = numpy.random.RandomState(4).standard_cauchy(size=(70, 100, 1))
    res = rd.from_rows(rows)
    assert res.rhat_bulk[0] < 1.01


def test_shifted_chain():
    rows = _iid(4, 200, 5)
    rows[3] += 3.0
    assert rd.from_rows(rows).rhat[0] > 1.3


def test_degenerate_columns():
    rows = numpy.random.RandomState(6).normal(size=(4, 20, 3))
    rows[:, :, 1] = 7.0
    rows[2, 3, 2] = numpy.inf
    res = rd.from_rows(rows, ["a", "b", "c"])
    assert list(res.nonfinite) == [0, 0, 1]
    for name in ("rhat", "rhat_bulk", "rhat_folded", "ess_bulk", "ess_tail"):
        v = getattr(res, name)
        assert numpy.isfinite(v[0]) and numpy.isnan(v[1]) and numpy.isnan(v[2]), name
    assert not res.converged[1:].any() and not res.enough[1:].any()


def test_too_short_or_odd_raises():
    for R in (2, 5):
        with pytest.raises(ValueError):
            rd.from_rows(numpy.zeros((3, R, 1)))


def test_csv_text(tmp_path):
    rows = rows_of(ar1(2, 8, 6, 41))
    res = rd.from_rows(rows, ["b'x", "a"])
    res.rhat[:] = [1.23456, 1.0]
    res.rhat_bulk[:] = [1.2, 1.0004]
    res.rhat_folded[:] = [1.1, numpy.nan]
    res.converged[:] = [False, True]
    res.ess_bulk[:] = [12.3456, 4000.0]
    res.ess_tail[:] = [7.0, 401.25]
    res.enough[:] = [False, True]
    text = rd.csv_text(res)
    assert text == ("parameter,rhat,rhat bulk,rhat folded,converged,ess bulk,ess tail,enough\n"
                    "'a',1.000,1.000,nan,True,4000.000,401.250,True\n"
                    "'b'x',1.235,1.200,1.100,False,12.346,7.000,False\n")
    rd.write_csv(res, str(tmp_path))
    assert open(str(tmp_path / "rank_diagnostics.csv")).read() == text
