"""Cases of tests/test_decision_cases.py (CPU) and tests/test_gpu_decision.py (GPU): the
control path of a step -- prior, Metropolis decision, tuning table, state write-back -- on
inputs that reach every branch of it.

The decision (csrc/step.h, csrc/sweep.h; posteriorSampling.py:347-364) has four branches:
  1  current posterior not finite, proposal's finite        -> accept
  2  proposal likelihood not finite                         -> reject
  3  difference of the posteriors not finite                -> reject
  4  log u < difference
and the tuning table (:385-437) seven factors.  Every case starts some chains outside their
prior's support (branch 1 needs it) or where the likelihood is NaN / -inf, proposes from
scales spread over five decades (every acceptance rate, so every factor) and tunes at an
interval above 20 (the factor 0.5 needs a rate in [0.001, 0.05): one acceptance in 25).

``stats`` reads what a case reached from the oracle's own trace; the CPU test asserts its
thresholds, so a case that stops reaching a branch fails there and not silently.

The complete-pooling cases have one cell per (chain, parameter), so they differ from the
others where the thresholds need it: five tunings instead of three (n_iter 130), 40 chains
that start with a NaN likelihood (a cell takes branch 1 once at the most), and for those
chains a scale of the parameter that has to move of 10**U(-0.5, 1.5), so that they do get
out; their other scales are 10**U(-3.6, 1.4), since with so few cells the factor 10 (a rate
above 0.95) was short of its count at 10**U(-3, 2).  The split case's posterior is a tenth as
wide (8200 rows), so its starts lie closer (sd 0.01) and its scales 1.2 decades lower.
"""

import collections
import functools
import zlib

import numpy
import scipy.stats

import user_models
from gpu_cases import run_oracle_state
from nestmc.families import DeviceLikelihood, LinearRegression
from oracle import restatement as rs
from rowpath_cases import FastNested

TUNE = 25                                # tunes at iterations 25, 50, 75 (, 100, 125)
SEED, BASE = 20260, 3                    # Philox seed, global id of chain 0
FACTORS = (0.1, 0.5, 0.9, 1.0, 1.1, 2.0, 10.0)
HEAD = 24                                # chains 0 .. 23 hold every non-finite start of the
                                         # cases whose oracle runs a subset of the chains

PRIOR_SETS = {
    "A": lambda: [scipy.stats.uniform(0.5, 1.0), scipy.stats.expon(loc=2.5, scale=2),
                  scipy.stats.invgamma(3.0, scale=2)],
    "B": lambda: [scipy.stats.cauchy(1, 2), scipy.stats.laplace(3, 1.5),
                  scipy.stats.lognorm(0.7)],
    "C": lambda: [scipy.stats.gamma(0.5, loc=0.5, scale=2), scipy.stats.norm(3, 10),
                  scipy.stats.halfnorm(scale=3)],
    "D": lambda: [scipy.stats.gamma(1.0, loc=0.9), scipy.stats.uniform(2.8, 0.5),
                  scipy.stats.gamma(2)],
    # the user (Poisson) model's two parameters: the intercept's support holds every start,
    # the slope's is left by most proposals of the larger scales
    "U": lambda: [scipy.stats.expon(loc=-2.0, scale=50.0), scipy.stats.uniform(0.0, 0.6)],
}
# families whose support is bounded: the prior must return -inf at least once in a case
BOUNDED = {"uniform", "expon", "invgamma", "lognorm", "gamma", "halfnorm"}

# n_iter: burn-in ends 4 iterations before it; nan / out: chains [0, nan) start with a NaN
# (user: -inf ... see build) likelihood, [nan, out) outside a bounded support; start_sd: of
# the start values around the truth; decades: the proposal scales are 10**U(decades)
Case = collections.namedtuple(
    "Case", "name pooling sizes C sets kind all_chains n_iter nan out start_sd decades")


def _ragged(G, nmax, seed):
    s = [int(v) for v in numpy.random.RandomState(seed).randint(0, nmax + 1, size=G)]
    s[0] = max(s[0], 1)
    return s


_D = (-3.0, 2.0)
CASES = [
    Case("none-half", "none", [12, 0, 7, 1, 23], 70, ("A", "B", "C", "D"), "linreg", True,
         80, 16, 24, 0.1, _D),
    Case("complete", "complete", [43], 70, ("A", "D"), "linreg", True, 130, 40, 48, 0.1,
         (-3.6, 1.4)),
    Case("complete-split", "complete", [8200], 66, ("A",), "linreg", True, 130, 40, 48, 0.01,
         (-4.8, 0.2)),
    Case("user", "none", [40] * 5, 65, ("U",), "user", True, 80, 16, 24, 0.1, _D),
    Case("partial-reg", "partial", [12, 0, 7, 1, 23], 70, ("-",), "linreg", True,
         80, 20, 20, 0.1, _D),
    Case("partial-lds", "partial", _ragged(70, 16, 70), 70, ("-",), "linreg", False,
         80, 20, 20, 0.1, _D),
    Case("partial-sweep", "partial", _ragged(129, 8, 129), 70, ("-",), "linreg", False,
         80, 20, 20, 0.1, _D),
]
BY_NAME = {c.name: c for c in CASES}
IDS = [(c.name, s) for c in CASES for s in c.sets]


class HostLinreg:
    """LinearRegression.__call__ (sigma sampled) without freezing a scipy distribution per
    call: oracle.restatement.norm_logpdf is scipy's norm(loc, scale).logpdf restated, so the
    values are the family's own bit for bit (tests/test_decision_cases.py asserts it)."""

    def __init__(self, fam):
        assert fam.sigma is None
        self.X, self.y = fam.X, fam.y

    def __call__(self, parameter):
        K = self.X.shape[1]
        betaHat = numpy.vstack([parameter[j] for j in range(K)]).T
        yHat = numpy.sum(self.X * betaHat, axis=1)
        return rs.norm_logpdf(yHat, self.y, numpy.array(parameter[K]))


Built = collections.namedtuple("Built", "case fam sizes priors st scale nested sel")


@functools.lru_cache(maxsize=None)
def build(name, pset):
    """The case's family, priors, start state of all C chains ([C, P, G]; non-finite log
    priors and likelihoods as scipy and the oracle's group_ll give them), proposal scales,
    the oracle's Nested and the chains the oracle runs."""
    c = BY_NAME[name]
    G, C = len(c.sizes), c.C
    n = int(sum(c.sizes))
    r = numpy.random.RandomState(zlib.crc32(("%s/%s" % (name, pset)).encode()))
    if c.kind == "user":
        x, y = user_models.poisson_data(G, c.sizes[0])
        host = user_models.poisson_host(x, y, 0.1)
        fam = DeviceLikelihood(user_models.poisson_rows(x, y), user_models.POISSON, 2,
                               consts=[0.1], host_function=host)
        centre = numpy.array([0.5, 0.3])
    else:
        d = numpy.random.RandomState(3)
        x = d.normal(size=n)
        y = 1.0 + 3.0 * x + d.normal(size=n) * 0.7
        fam = LinearRegression(numpy.vstack([numpy.ones(n), x]).T, y)
        host = HostLinreg(fam)
        centre = numpy.array([1.0, 3.0, 0.7])
    P = len(centre)
    assert fam.n_params == P
    nested = FastNested(host, c.sizes)
    scale = 10.0 ** r.uniform(c.decades[0], c.decades[1], size=(C, P, G))
    with numpy.errstate(all="ignore"):
        if c.pooling == "partial":
            priors = None
            mu = r.normal(0, 0.5, size=(C, P)) + centre
            s2 = r.uniform(0.2, 1.0, size=(C, P)) * 0.2
            value = mu[:, :, None] + numpy.sqrt(s2)[:, :, None] * r.normal(size=(C, P, G))
            # sigma < 0 in every second group of the first chains: NaN likelihood
            value[:c.nan, 2, ::2] = -numpy.abs(value[:c.nan, 2, ::2])
            lp = rs.norm_logpdf(value, mu[:, :, None], numpy.sqrt(s2)[:, :, None])
        else:
            priors = PRIOR_SETS[pset]()
            mu = s2 = None
            start = centre + r.normal(0, c.start_sd, size=(C, P))
            if c.kind == "user":
                start[:c.nan, 1] = -0.5               # outside the slope's support
                start[c.nan:c.out, 0] = 709.5         # exp(eta) overflows: LL = -inf
            else:
                start[:c.nan, 2] = -0.3               # sigma < 0: NaN likelihood
                start[c.nan:c.out, 0] = -5.0          # outside the bounded supports
            if c.pooling == "complete":               # (module docstring)
                scale[:c.nan, 2, :] = 10.0 ** r.uniform(-0.5, 1.5, size=(c.nan, G))
                scale[c.nan:c.out, 0, :] = 10.0 ** r.uniform(-0.5, 1.5, size=(c.out - c.nan, G))
            value = numpy.repeat(start[:, :, None], G, axis=2)
            lp = numpy.stack([numpy.asarray(priors[p].logpdf(value[:, p, :]), float)
                              for p in range(P)], 1)
        sel = numpy.arange(C) if c.all_chains else numpy.r_[0:HEAD, C - 1]
        assert c.all_chains or c.out <= HEAD
        ll = numpy.array([nested.group_ll(value[k]) for k in range(C)])
    return Built(c, fam, c.sizes, priors, rs.State(value, lp, ll, mu, s2), scale, nested, sel)


def run_kw(b):
    """The keywords gpu_cases.run_engine and run_oracle_state share."""
    return dict(pooling=b.case.pooling, priors=b.priors, burn=b.case.n_iter - 4, thin=1,
                tune_interval=TUNE, scale=b.scale)


@functools.lru_cache(maxsize=None)
def oracle(name, pset):
    """(flags, proposal LLs, rows, min margin, final State, trace) of chains build().sel."""
    b = build(name, pset)
    with numpy.errstate(all="ignore"):   # (the non-finite starts are the point)
        return run_oracle_state(b.nested, b.st, b.sel, b.sel + BASE, b.case.n_iter, SEED,
                                **run_kw(b))


def stats(name, pset):
    """What the oracle's run reached: {"branch": {1..4: steps}, "factor": {f: times applied},
    "margin": the least |log u - diff| of branch 4, "neginf": per parameter, how often the
    proposal's log prior was -inf, "nan_start": cells whose start likelihood is not finite}."""
    b = build(name, pset)
    acc, llp, rows, margin, state, trace = oracle(name, pset)
    br = numpy.stack(trace["branch"])                      # [iter * P, C, G]
    lpp = numpy.stack(trace["lpp"])
    P = b.st.value.shape[1]
    fac = collections.Counter()
    for _, _, old, new in trace["tune"]:
        hit = numpy.zeros(old.shape, int)
        for f in FACTORS:
            m = (old * f == new)
            hit += m
            fac[f] += int(m.sum())
        assert numpy.all(hit == 1), "a tuning step applied no factor of the table, or two"
    return {"branch": {k: int((br == k).sum()) for k in (1, 2, 3, 4)},
            "factor": {f: fac[f] for f in FACTORS},
            "margin": float(margin),
            "neginf": [int(numpy.isneginf(lpp[p::P]).sum()) for p in range(P)],
            "nan_start": int((~numpy.isfinite(b.st.ll[b.sel])).sum()),
            "steps": int(br.size)}
