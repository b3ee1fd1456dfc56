"""CPU: the cases of tests/decision_cases.py are not vacuous.

The oracle alone runs every case; from its trace, each case must take every branch of the
Metropolis decision and apply every factor of the tuning table often enough that a device
that got one of them wrong could not pass tests/test_gpu_decision.py by luck:

* branches 1, 2 and 4 at least 20 times each; branch 3 at least 200 times under none and
  complete pooling (under partial pooling the prior is a normal density of finite
  hyper-parameters: it is never -inf, so a finite proposal likelihood gives a finite
  difference or branch 1);
* each tuning factor 0.1, 0.5, 0.9, 1.0, 1.1, 2.0, 10 at least 50 times;
* the least decision margin |log u - diff| at least 1e-7: the device's likelihoods are
  within about 1e-13 relative of the oracle's, so a flipped flag is a bug and not rounding;
* every prior with a bounded support returns -inf at least once.
"""

import numpy
import pytest

import decision_cases as dc


@pytest.mark.parametrize("name,pset", dc.IDS, ids=["%s-%s" % i for i in dc.IDS])
def test_case_reaches_every_branch(name, pset):
    b = dc.build(name, pset)
    s = dc.stats(name, pset)
    print("DECISION %-14s %s branches %s factors %s margin %.3g -inf priors %s" % (
        name, pset, s["branch"], s["factor"], s["margin"], s["neginf"]))
    n_tune = len(range(dc.TUNE, b.case.n_iter - 4, dc.TUNE))
    assert sum(s["factor"].values()) == n_tune * b.st.value[b.sel].size
    assert sum(s["branch"].values()) == s["steps"]
    for k in (1, 2, 4):
        assert s["branch"][k] >= 20, (k, s["branch"])
    if b.case.pooling == "partial":
        assert s["branch"][3] == 0, s["branch"]
    else:
        assert s["branch"][3] >= 200, s["branch"]
    for f in dc.FACTORS:
        assert s["factor"][f] >= 50, (f, s["factor"])
    assert s["margin"] >= 1e-7, s["margin"]
    assert s["nan_start"] >= 16
    for p, d in enumerate(b.priors or []):
        if d.dist.name in dc.BOUNDED:
            assert s["neginf"][p] >= 1, (p, d.dist.name, s["neginf"])


def test_prior_sets_hold_every_device_family():
    """The four sets between them: all nine families, gamma with a shape below 1 and with a
    loc among them."""
    from nestmc import _lib
    ds = [d for k in "ABCD" for d in dc.PRIOR_SETS[k]()]
    assert {d.dist.name for d in ds} == set(_lib.PRIOR)
    gam = [d.dist._parse_args(*d.args, **d.kwds) for d in ds if d.dist.name == "gamma"]
    assert any(sh[0] < 1 for sh, _, _ in gam) and any(loc != 0 for _, loc, _ in gam)


def test_host_linreg_is_the_familys_callable():
    """decision_cases.HostLinreg (no scipy freeze per call) against LinearRegression.__call__,
    bit for bit, negative and zero sigma (NaN) included."""
    b = dc.build("none-half", "A")
    r = numpy.random.RandomState(0)
    n = int(sum(b.sizes))
    for _ in range(20):
        par = [r.normal(1, 2, size=n), r.normal(3, 2, size=n), r.normal(0.3, 0.7, size=n)]
        par[2][:3] = [0.0, -0.0, numpy.inf]
        with numpy.errstate(all="ignore"):
            assert numpy.array_equal(b.nested.f(par), b.fam(par), equal_nan=True)
    assert numpy.isnan(b.nested.f(par)).any()


def test_start_states_are_scipys():
    """The non-finite start values reach set_state as scipy and the oracle give them."""
    b = dc.build("none-half", "A")
    c = b.case
    assert numpy.all(numpy.isnan(b.st.ll[:c.nan][:, numpy.asarray(b.sizes) > 0]))
    assert numpy.all(numpy.isneginf(b.st.lp[c.nan:c.out, 0, :]))       # uniform(0.5, 1) at -5
    assert numpy.all(numpy.isneginf(b.st.lp[:c.nan, 2, :]))            # invgamma at -0.3
    u = dc.build("user", "U")
    assert numpy.all(numpy.isneginf(u.st.ll[u.case.nan:u.case.out]))   # exp overflow
    assert numpy.all(numpy.isneginf(u.st.lp[:u.case.nan, 1, :]))
    p = dc.build("partial-reg", "-")
    assert numpy.isnan(p.st.ll[:p.case.nan, 0]).all() and numpy.isfinite(p.st.lp).all()
