"""GPU: the control path of a step -- prior, Metropolis decision, tuning table, state
write-back -- against the oracle on the cases of tests/decision_cases.py, which reach every
branch of it (tests/test_decision_cases.py asserts that from the oracle's trace):

* all nine prior families inside a step kernel (gamma with a shape below 1 and with a loc);
* the four branches of the decision (csrc/step.h, csrc/sweep.h): chains that start with a
  NaN or -inf likelihood or outside their prior's support take "current posterior not
  finite, proposal finite -> accept", finite likelihoods under a -inf prior take "difference
  not finite -> reject";
* all seven tuning factors (interval 25: one acceptance in 25 is the factor 0.5);
* the state the kernel writes back, against the oracle's final State: scale BIT FOR BIT
  (a product of table factors, one IEEE multiplication each in both), accept counts exact,
  value / ll / log_prior / mu / s2 to tolerance, with equal NaN and equal infinities.  The
  log prior is Engine.log_prior() (nmc_get_log_prior): under partial pooling the reference
  holds each value's under the CURRENT hyper-parameters, where get_state's is the device's
  copy under those of the step that decided the value.

Every case asserts from Engine.launch_config() the kernel, mode or row split it is about.

Measured on an MI355X (oracle chains: all; chains 0-23 and the last for partial-lds and
partial-sweep).  Branch counts, tuning-factor counts and the least decision margin are the
oracle's; "d lp" is the device's worst |log_prior - oracle's| over the final state,
relative to |oracle's| and (in brackets) to 1 + |oracle's|; "d llp" the worst relative
error of the proposal likelihoods of the whole run.

    case            branch 1 / 2 / 3 / 4         factor 0.1/0.5/0.9/1.0/1.1/2.0/10  margin   d lp               d llp
    none-half A     50 / 9866 / 21271 / 52813    600/196/424/651/417/431/431        1.8e-05  9.6e-13 (1.1e-14)  7.4e-13
    none-half B     39 / 10339 / 1940 / 71682    485/149/402/606/444/509/555        1.3e-05  9.0e-15 (2.8e-15)  2.8e-12
    none-half C     60 / 10728 / 9386 / 63826    582/182/384/568/440/445/549        2.4e-05  1.5e-12 (2.8e-14)  1.9e-12
    none-half D     114 / 10731 / 24770 / 48385  692/214/470/583/401/425/365        1.0e-04  7.6e-14 (1.2e-14)  1.5e-12
    complete A      42 / 1751 / 3912 / 21595     85/68/206/289/183/128/91           3.1e-05  4.8e-14 (1.7e-15)  3.9e-13
    complete D      43 / 1926 / 7122 / 18209     130/73/231/280/163/103/70          2.3e-04  5.9e-14 (7.6e-16)  5.3e-13
    complete-split  43 / 1269 / 1163 / 23265     115/84/197/235/148/132/79          2.0e-05  4.8e-14 (5.8e-15)  1.2e-12
    user            49 / 4578 / 16087 / 31286    553/178/299/323/242/216/139        4.2e-05  4.5e-16 (3.6e-16)  1.1e-13
    partial-reg     47 / 16155 / 0 / 67798       658/186/419/568/425/504/390        8.0e-06  4.2e-13 (1.4e-14)  8.3e-13
    partial-lds     386 / 113697 / 0 / 305917    4448/984/2238/2602/1883/2080/1515  7.4e-06  1.9e-12 (7.6e-15)  4.4e-12
    partial-sweep   787 / 210123 / 0 / 563090    8042/1600/3719/4966/3522/3902/3274 9.8e-06  1.9e-12 (1.6e-14)  2.0e-10

The log prior is held to the issue's 1e-12 relative plus an absolute floor of 1e-14,
|d| <= 1e-14 + 1e-12 |ref|.  A purely relative bound is missed in three cases (1.5e-12,
1.9e-12, 1.9e-12 above), each at a log density that passes through zero: 6.7e-16 absolute at
a gamma(0.5, loc 0.5, scale 2) log density of 4.6e-4.  A log density is a sum of up to four
terms (log Gamma(a), log scale, the terms in x) of magnitude up to about 10 here, each
rounded to 2^-53 of ITSELF in the device and in scipy, with libraries whose log differs by
an ulp, so the error of the sum does not shrink with it: 2 sides x 4 terms x 2^-53 x 10 is
9e-15, hence 1e-14.  The test prints the worst |d| - 1e-12 |ref| of each case beside it
(measured: 1.6e-15 at the most).
(partial-sweep's 2.0e-10 on a proposal likelihood is likewise a sum near zero, inside the
suite's 1e-9 absolute.)

Which decisions the demonstrated breaks cover: the temporary breaks of
profiles/r09_breaks.txt were made in csrc/step.h alone.  csrc/sweep.h's own copy of the
decision (nmc_k_sweep, the partial-sweep case) and the user family's kernel, which is
compiled at run time, are held by the oracle comparison here, not by a break shown to fail.
"""

import numpy
import pytest

import decision_cases as dc
from gpu_cases import run_engine

pytestmark = pytest.mark.gpu

# what each case must run as: (kernel prefix, modes or None for any, split members)
PATHS = {
    "none-half": ("nmc_k_run<", ("NMC_MODE_HALF",), 1),
    "complete": ("nmc_k_run<", ("NMC_MODE_HALF", "NMC_MODE_NOPOOL"), 1),
    "complete-split": ("nmc_k_run<", None, 3),
    "user": ("nmc_k_run<FamUser, ", ("NMC_MODE_HALF", "NMC_MODE_NOPOOL"), 1),
    "partial-reg": ("nmc_k_run<", ("NMC_MODE_SYNC_REG",), 1),
    "partial-lds": ("nmc_k_run<", ("NMC_MODE_SYNC_LDS",), 1),
    "partial-sweep": ("nmc_k_sweep<", ("NMC_MODE_SYNC_OWN",), 1),
}
# the same case on the other kernel or layout: bit-identical
VARIANTS = {
    "none-half": ({"NMC_HALF": "0"}, "nmc_k_run<", "NMC_MODE_NOPOOL"),
    "partial-sweep": ({"NMC_SWEEP": "0"}, "nmc_k_run<", None),
}


def _run(b, env=None):
    C = b.case.C
    return run_engine(b.fam, b.sizes, b.st, numpy.arange(C), dc.BASE, b.case.n_iter, dc.SEED,
                      env=env, **dc.run_kw(b))


def _same_special(a, b, what):
    """NaN where the other has NaN, each infinity where the other has the same one."""
    for f in (numpy.isnan, numpy.isposinf, numpy.isneginf):
        bad = numpy.argwhere(f(a) != f(b))
        assert bad.size == 0, (what, f.__name__, bad[:5])


def _close(a, b, what, rtol, atol):
    _same_special(a, b, what)
    ok = numpy.isclose(a, b, rtol=rtol, atol=atol, equal_nan=True)
    bad = numpy.argwhere(~ok)
    assert bad.size == 0, (what, bad[:5], a[tuple(bad[0])], b[tuple(bad[0])])


def _worst_rel(a, b, floor=0.0):
    """max |a - b| / (floor + |b|) over the finite, non-zero b."""
    fin = numpy.isfinite(b) & (b != 0)
    if not fin.any():
        return 0.0
    return float(numpy.max(numpy.abs(a[fin] - b[fin]) / (floor + numpy.abs(b[fin]))))


@pytest.mark.parametrize("name,pset", dc.IDS, ids=["%s-%s" % i for i in dc.IDS])
def test_control_path_matches_oracle(gpu_lib, name, pset):
    b = dc.build(name, pset)
    partial = b.case.pooling == "partial"
    G, sel = len(b.sizes), b.sel
    acc, llp, rows, cfg = _run(b)
    kernel, modes, split = PATHS[name]
    assert cfg["kernel"].startswith(kernel), cfg
    assert (modes is None or cfg["mode"] in modes) and cfg["split_members"] == split, cfg
    if name == "complete":
        assert G == 1
    for_variant = VARIANTS.get(name)
    if for_variant:
        env, vkernel, vmode = for_variant
        o = _run(b, env)
        assert o[3]["kernel"].startswith(vkernel), o[3]
        assert vmode is None or o[3]["mode"] == vmode, o[3]
        for k in range(3):
            assert numpy.array_equal(o[k], (acc, llp, rows)[k], equal_nan=True), (env, k)
        for k, v in cfg["state"].items():
            assert numpy.array_equal(o[3]["state"][k], v, equal_nan=True), (env, k)
        assert numpy.array_equal(o[3]["log_prior"], cfg["log_prior"], equal_nan=True), env
        assert numpy.array_equal(o[3]["accept"], cfg["accept"]), env

    oacc, ollp, orows, margin, ost, _ = dc.oracle(name, pset)
    dev, dev_lp = cfg["state"], cfg["log_prior"]
    print("DECISION %-14s %s worst: log_prior %.3g rel, %.3g against 1 + |ref|; llp %.3g rel "
          "(min margin %.3g)" % (
              name, pset, _worst_rel(dev_lp[sel], ost.lp),
              _worst_rel(dev_lp[sel], ost.lp, 1.0),
              _worst_rel(llp[sel], ollp), margin))
    # the run: flags exact, proposal likelihoods and recorded rows to the suite's tolerances
    bad = numpy.argwhere(acc[sel].astype(bool) != oacc)
    assert bad.size == 0, "flag mismatch at %s (min decision margin %g)" % (bad[:5], margin)
    _close(llp[sel], ollp, "llp", 1e-10, 1e-9)
    _close(rows[sel], orows, "rows", 1e-9, 1e-9)
    # the state written back
    bad = numpy.argwhere(dev["scale"][sel] != ost.scale)
    assert bad.size == 0, ("scale", bad[:5], dev["scale"][sel][tuple(bad[0])],
                           ost.scale[tuple(bad[0])])
    assert numpy.array_equal(cfg["accept"][sel], ost.total_acc), "accept counts"
    _close(dev["value"][sel], ost.value, "value", 1e-10, 1e-9)
    _close(dev["ll"][sel], ost.ll, "ll", 1e-10, 1e-9)
    # (1e-12 relative, floor 1e-14: the module docstring)
    with numpy.errstate(invalid="ignore"):   # (-inf against -inf)
        need = numpy.abs(dev_lp[sel] - ost.lp) - 1e-12 * numpy.abs(ost.lp)
    print("DECISION %-14s %s log_prior: worst |d| - 1e-12 |ref| = %.3g (floor 1e-14)" % (
        name, pset, numpy.nanmax(numpy.where(numpy.isfinite(need), need, -numpy.inf))))
    _close(dev_lp[sel], ost.lp, "log_prior", 1e-12, 1e-14)
    if partial:   # (columns of the recorded rows: the rows' tolerances)
        _close(dev["mu"][sel], ost.mu, "mu", 1e-9, 1e-9)
        _close(dev["s2"][sel], ost.s2, "s2", 1e-9, 1e-9)
        # (nmc_get_log_prior: the division form on the host, every chain)
        from oracle import restatement as rs
        with numpy.errstate(all="ignore"):
            want = rs.norm_logpdf(dev["value"], dev["mu"][:, :, None],
                                  numpy.sqrt(dev["s2"])[:, :, None])
        _close(dev_lp, want, "log_prior of the device's own state", 1e-14, 1e-14)
    else:
        # the accepted values' own log priors: what the kernel wrote back
        assert numpy.array_equal(dev_lp, dev["log_prior"], equal_nan=True)
        # no hyper-parameters: NaN, not device memory nothing ever wrote
        assert numpy.isnan(dev["mu"]).all() and numpy.isnan(dev["s2"]).all()
    # not vacuous on the device either: chains that started non-finite got out
    assert numpy.isfinite(dev["ll"][:b.case.nan]).mean() > 0.3


def test_log_prior_is_the_references(gpu_lib):
    """Partial pooling.  Before any iteration Engine.log_prior() returns the log priors
    set_state was given (the reference leaves a redrawn start value's stale, :284-285), as
    get_state does; after a run, each value's normal log density under the hyper-parameters
    get_state returns, while get_state's own log_prior stays the device's copy."""
    from nestmc.engine import Engine
    from oracle import restatement as rs
    b = dc.build("partial-reg", "-")
    eng = Engine(b.fam, b.sizes, b.case.C, "partial", None, seed=dc.SEED, chain_base=dc.BASE)
    stale = b.st.lp + 1.0
    eng.set_state(b.st.value, stale, b.st.ll, b.st.mu, b.st.s2)
    assert numpy.array_equal(eng.log_prior(), stale)
    assert numpy.array_equal(eng.get_state()["log_prior"], stale)
    eng.set_schedule(3, 0, 1, tune_interval=dc.TUNE)
    eng.run(0, 3)
    st, lp = eng.get_state(), eng.log_prior()
    assert numpy.all(numpy.isfinite(st["log_prior"]))
    eng.close()
    with numpy.errstate(all="ignore"):
        want = rs.norm_logpdf(st["value"], st["mu"][:, :, None], numpy.sqrt(st["s2"])[:, :, None])
    assert not numpy.array_equal(st["mu"], b.st.mu)
    _close(lp, want, "log_prior", 1e-14, 1e-14)
