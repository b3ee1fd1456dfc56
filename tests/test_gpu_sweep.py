"""GPU: nmc_k_sweep (csrc/sweep.h, csrc/sweep_gibbs.h) on every family, row width and row
shape it can take, each reached by its shape and asserted from Engine.launch_config().

sweep.h: "Same work, tile partition, summation orders, variates and outputs as nmc_k_run --
the two are bit-identical".  tests/sweep_cases.py holds the cases: all fifteen instantiations
that partial pooling over more than 128 groups can choose (FamLinreg<1..6>,
FamLogistic<1..6>, FamGaussMean<1..3>), with a sampled sigma and without an intercept, on
ragged groups (empty, one row, the row-block and tile edges; odd row widths on both start
parities of the prologue's row copy, the table ending on an odd double), a group at the
limit of the LDS carve and one row beyond it, 129 / 136 / 256 / 512 groups, and one and two
chain blocks (twelve and four waves).

a. test_sweep_equals_run: launch_config() names the case's kernel; the same run under
   NMC_SWEEP=0 names nmc_k_run; flags, proposal LLs, recorded rows (hyper columns included),
   the final state, log_prior() and accept_counts() of the two are equal BIT FOR BIT; the
   sweep's stored group LLs are eval_group_ll of its stored values bit for bit, 0.0 for an
   empty group.
b. test_sweep_matches_oracle: chains 0, 1 and C - 1 of every ragged and at-limit case against
   the numpy oracle on the same Philox stream, within the suite's bounds.
c. test_sweep_variants: NMC_ZIN, NMC_SWEEP_WAVES, NMC_GSEP, launches of 3, 3, 2 iterations
   (with and without tuning between them) and NMC_PERSIST=0, bit for bit, for four
   parameters, three accumulator sets, a sampled sigma and three-field rows.
d. test_gibbs_takeover_four_parameters: the likelihood workgroups take the Gibbs tasks over
   when their kernel is serialized before or behind them.
e. test_sweep_replay: replayed variates (the replay branch of nmc_sweep_variate_part).
f. test_unreachable_instantiations / test_over_limit_leaves_the_sweep: what the sweep is
   never chosen for launches nmc_k_run on rows beyond LDS.
"""

import functools

import numpy
import pytest

import gibbs_order as go
import rowpath_cases as rp
import sweep_cases as sc
from gpu_cases import run_engine
from nestmc.engine import Engine
from oracle import restatement as rs

pytestmark = pytest.mark.gpu

TRIPLE = ("accept flags", "proposal LLs", "recorded rows")
STATE = ("value", "ll", "mu", "s2", "scale")


@functools.lru_cache(maxsize=None)
def _start(name):
    """The case's start with the device's own group LLs (eval_group_ll) on every chain the
    oracle does not run; its chains keep the oracle's LLs, which the device's must match."""
    case, run = sc.BY_NAME[name], sc.run_of(name)
    st = run.state
    ll = _group_ll(name, st.value)
    assert numpy.allclose(ll, st.ll, rtol=1e-10, atol=1e-9) and numpy.all(numpy.isfinite(ll))
    ll[run.sel] = st.ll[run.sel]
    return rs.State(st.value, st.lp, ll, st.mu, st.s2)


def _run(name, env=None, chains=None, **kw):
    """The case's run on the engine (chains: the first so many of them only)."""
    case, run = sc.BY_NAME[name], sc.run_of(name)
    return run_engine(run.fam, run.sizes, _start(name), numpy.arange(chains or case.C), run.base,
                      run.n_iter, run.seed, env=env, **dict(run.kw, **kw))


@functools.lru_cache(maxsize=None)
def _sweep_run(name):
    """The case's default run, shared (and left unchanged) by the tests that compare to it."""
    out = _run(name)
    _assert_sweep(sc.BY_NAME[name], out[3])
    return out


@functools.lru_cache(maxsize=None)
def _plain_run(name):
    """The same run on nmc_k_run (NMC_SWEEP=0)."""
    out = _run(name, env={"NMC_SWEEP": "0"})
    assert out[3]["kernel"].startswith("nmc_k_run<"), (name, out[3])
    return out


def _assert_sweep(case, cfg, waves=None):
    what = (case.name, cfg)
    assert cfg["kernel"] == case.kernel and cfg["mode"] == "NMC_MODE_SYNC_OWN", what
    assert cfg["split_members"] == 1 and cfg["chains_per_block"] == 64, what
    assert cfg["waves_per_group"] == (waves or case.waves), what
    assert cfg["chain_blocks"] == case.blocks, what


def _assert_same(got, want, what):
    """Flags, proposal LLs, rows, final state, log priors and accept counts, bit for bit."""
    for k, part in enumerate(TRIPLE):
        assert got[k].shape == want[k].shape, (what, part)
        bad = numpy.argwhere(~((got[k] == want[k]) | ((got[k] != got[k]) & (want[k] != want[k]))))
        assert bad.size == 0, (what, part, len(bad), bad[:5].tolist())
    for key in STATE:
        assert numpy.array_equal(got[3]["state"][key], want[3]["state"][key], equal_nan=True), \
            (what, "state", key)
    assert numpy.array_equal(got[3]["log_prior"], want[3]["log_prior"], equal_nan=True), what
    assert numpy.array_equal(got[3]["accept"], want[3]["accept"]), what


def _group_ll(name, value):
    case, (fam, sizes) = sc.BY_NAME[name], sc.model(name)
    eng = Engine(fam, sizes, case.C, "partial", None)
    out = eng.eval_group_ll(value)
    eng.close()
    return out


def _not_vacuous(case, acc):
    nonempty = numpy.asarray(case.sizes) > 0
    moved = acc.astype(bool).any(axis=(1, 2))[:, nonempty].mean()
    assert 0.05 < acc.mean() < 0.95, (case.name, acc.mean())
    assert moved >= 0.5, (case.name, moved)
    return moved


@pytest.mark.parametrize("case", sc.SWEEP_CASES, ids=repr)
def test_sweep_equals_run(gpu_lib, case):
    assert case.sweep and case.lds
    dev = _sweep_run(case.name)
    acc, llp, rows, cfg = dev
    ref = _plain_run(case.name)
    assert ref[3]["kernel"].startswith("nmc_k_run<%s<%d>, " % (sc.FAMILY[case.kind], case.nf))
    assert ref[3]["kernel"].endswith(", true>"), ref[3]
    moved = _not_vacuous(case, acc)
    print("SWEEP %-30s kernel %s waves %d acceptance %.3f moved %.3f" % (
        case.name, cfg["kernel"], cfg["waves_per_group"], acc.mean(), moved))
    assert acc.shape == (case.C, case.n_iter, case.P, case.G)
    assert rows.shape[:2] == (case.C, case.n_iter) and numpy.all(numpy.isfinite(rows))
    _assert_same(dev, ref, (case.name, "sweep against nmc_k_run"))
    # the stored group LL is the group kernel's LL of the stored values (the start's LLs are
    # the group kernel's too, but for the oracle's chains: there a cell that never moved keeps
    # the oracle's LL of its start); an empty group's is 0
    state = cfg["state"]
    ll1 = _group_ll(case.name, state["value"])
    start, sel = _start(case.name), sc.run_of(case.name).sel
    still = numpy.zeros(ll1.shape, bool)
    still[sel] = ~acc[sel].astype(bool).any(axis=(1, 2))
    assert numpy.array_equal(state["value"].transpose(0, 2, 1)[still],
                             start.value.transpose(0, 2, 1)[still])
    ll1[still] = start.ll[still]
    bad = numpy.argwhere(state["ll"] != ll1)
    assert bad.size == 0, (case.name, bad[:5].tolist(), state["ll"][tuple(bad[0])],
                           ll1[tuple(bad[0])])
    empty = numpy.asarray(case.sizes) == 0
    assert numpy.all(state["ll"][:, empty] == 0.0) and numpy.all(llp[:, :, :, empty] == 0.0)
    assert numpy.all(numpy.isfinite(state["ll"]))
    # the last recorded row holds the stored values, the accept counts the flags
    last = rs.State(state["value"], state["log_prior"], state["ll"], state["mu"], state["s2"])
    assert numpy.array_equal(rows[:, -1, :], rs.row_values(last, True))
    assert numpy.array_equal(cfg["accept"], acc.astype(numpy.int64).sum(axis=1))
    if case.sigma == "sampled":     # proposals at or below zero: a NaN LL, never accepted
        nan = numpy.isnan(llp[:, :, -1, :])
        assert nan[:, :, ~empty].sum() > 0 and not acc[:, :, -1, :][nan].any()
        # (an empty group has no likelihood to refuse a sigma <= 0: the prior alone decides)
        assert numpy.all(state["value"][:, -1, :][:, ~empty] > 0)
    else:
        assert numpy.all(numpy.isfinite(llp))


@pytest.mark.parametrize("case", sc.ORACLE_CASES, ids=repr)
def test_sweep_matches_oracle(gpu_lib, case):
    acc, llp, rows, cfg = _sweep_run(case.name)
    sel = sc.run_of(case.name).sel
    oacc, ollp, orows, margin = sc.oracle_of(case.name)
    print("SWEEP %-30s kernel %s waves %d oracle acceptance %.3f least margin %.3g" % (
        case.name, cfg["kernel"], cfg["waves_per_group"], oacc.mean(), margin))
    bad = numpy.argwhere(acc[sel].astype(bool) != oacc)
    assert bad.size == 0, "flag mismatch at %s (min decision margin %g)" % (bad[:5], margin)
    assert numpy.allclose(llp[sel], ollp, rtol=1e-10, atol=1e-9, equal_nan=True)
    assert numpy.allclose(rows[sel], orows, rtol=1e-9, atol=1e-9, equal_nan=True)
    assert numpy.all(numpy.isfinite(rows))


VARIANTS = [("zin", {"NMC_ZIN": "1"}, {}), ("waves3", {"NMC_SWEEP_WAVES": "3"}, {}),
            ("waves4", {"NMC_SWEEP_WAVES": "4"}, {}),
            ("waves12", {"NMC_SWEEP_WAVES": "12"}, {"chains": 64}),
            ("gsep", {"NMC_GSEP": "1"}, {}), ("launch3", {}, {"launch_iters": 3})]


def _chains(out, n):
    """The first n chains of a run's results (a chain's results depend on no other chain)."""
    cfg = dict(out[3], state={k: v[:n] for k, v in out[3]["state"].items()},
               log_prior=out[3]["log_prior"][:n], accept=out[3]["accept"][:n])
    return out[0][:n], out[1][:n], out[2][:n], cfg


@pytest.mark.parametrize("name", sc.VARIANT_CASES)
def test_sweep_variants(gpu_lib, name):
    """Twelve waves run on the first chain block alone: two chain blocks of twelve-wave
    workgroups (three waves per SIMD at 168 VGPRs) leave no CU room for a Gibbs workgroup, and
    the host then runs nmc_k_run, which the last lines hold to the NMC_SWEEP=0 run."""
    case = sc.BY_NAME[name]
    assert case.C == 65 and case.waves == 4
    dev = _sweep_run(name)
    assert dev[3]["zin"] == 0 and dev[3]["gibbs_fallbacks"] == 0, dev[3]
    for tag, env, kw in VARIANTS:
        o = _run(name, env=env, **kw)
        cfg, n = o[3], kw.get("chains", case.C)
        what = (name, tag, {k: v for k, v in cfg.items() if numpy.ndim(v) == 0})
        assert cfg["kernel"] == case.kernel and cfg["mode"] == "NMC_MODE_SYNC_OWN", what
        assert cfg["split_members"] == 1 and cfg["chains_per_block"] == 64, what
        assert cfg["waves_per_group"] == int(env.get("NMC_SWEEP_WAVES", case.waves)), what
        assert cfg["chain_blocks"] == -(-n // 64), what
        assert cfg["zin"] == (1 if tag == "zin" else 0), what
        assert cfg["gibbs_fallbacks"] == 0, what     # (the kernels met)
        print("SWEEP %-30s %-8s kernel %s waves %d zin %d blocks per launch %d" % (
            name, tag, cfg["kernel"], cfg["waves_per_group"], cfg["zin"],
            cfg["chain_blocks_per_launch"]))
        _assert_same(o, _chains(dev, n), (name, tag))
    o = _run(name, env={"NMC_SWEEP_WAVES": "12"})
    assert o[3]["kernel"].startswith("nmc_k_run<"), o[3]["kernel"]
    _assert_same(o, _plain_run(name), (name, "twelve waves, two chain blocks"))
    # the same with tuning (burn n - 1: the scales are tuned at iterations 3 and 6, the first
    # steps of the second and third launch, from the accept and reject counters carried there)
    burn = case.n_iter - 1
    tuned = _run(name, burn=burn)
    _assert_sweep(case, tuned[3])
    assert (tuned[3]["state"]["scale"] != sc.run_of(name).kw["scale"]).mean() > 0.3
    _assert_same(_run(name, burn=burn, launch_iters=3), tuned, (name, "tuned, launches of 3"))
    o = _run(name, burn=burn, env={"NMC_SWEEP": "0"})
    assert o[3]["kernel"].startswith("nmc_k_run<"), o[3]["kernel"]
    _assert_same(o, tuned, (name, "tuned, nmc_k_run"))
    # a launch per iteration is nmc_k_run's: against the NMC_SWEEP=0 run
    o = _run(name, env={"NMC_PERSIST": "0"})
    assert not o[3]["persistent"] and o[3]["kernel"].startswith("nmc_k_run<"), o[3]
    assert o[3]["mode"] == "NMC_MODE_LAUNCH", o[3]
    _assert_same(o, _plain_run(name), (name, "NMC_PERSIST=0"))


def test_gibbs_takeover_four_parameters(gpu_lib):
    """tests/test_gpu_configs.py test_cfg4_gsep_serialized_kernels_fall_back with four
    parameters (lag 2 over P = 4 tasks per iteration, RB * P Gibbs workgroups): the Gibbs kernel
    serialized before the likelihood kernel (it gives up after the patience and leaves) or
    behind it (it finds the launch taken over).  Every (launch, chain block) falls back and
    the results are nmc_k_run's bit for bit."""
    name = sc.TAKEOVER_CASE
    case = sc.BY_NAME[name]
    assert (case.kind, case.nf, case.P, case.blocks) == ("logistic", 4, 4, 2)
    ref = _plain_run(name)
    launches = -(-case.n_iter // 2)
    for order in ("1", "2"):
        o = _run(name, launch_iters=2, env={"NMC_GSEP": "1", "NMC_GSEP_SERIAL": order,
                                            "NMC_GSEP_PATIENCE_US": "500"})
        _assert_sweep(case, o[3])
        print("SWEEP %-30s serial %s kernel %s waves %d fallbacks %d" % (
            name, order, o[3]["kernel"], o[3]["waves_per_group"], o[3]["gibbs_fallbacks"]))
        assert o[3]["gibbs_fallbacks"] == launches * case.blocks, (order, o[3])
        _assert_same(o, ref, (name, "serial", order))


N_REPLAY = 4


def _replay(name, env):
    case, run = sc.BY_NAME[name], sc.run_of(name)
    st = run.state
    z, u, hz, hu = go.variates(case.C, case.P, case.G, N_REPLAY, 7)
    with rp.environ(env):
        eng = Engine(run.fam, run.sizes, case.C, "partial", None, rng="replay")
    eng.set_state(st.value, st.lp, st.ll, st.mu, st.s2, scale=run.kw["scale"])
    eng.set_replay(z, u, hz, numpy.broadcast_to(hu[None], (case.C, N_REPLAY, case.P)).copy())
    eng.set_schedule(N_REPLAY, 0, 1, tune_interval=100)
    eng.set_trace(True)
    eng.run(0, N_REPLAY)
    eng.synchronize()
    acc, llp = eng.trace(N_REPLAY)
    cfg = eng.launch_config()
    cfg.update(state=eng.get_state(), log_prior=eng.log_prior(), accept=eng.accept_counts())
    out = acc, llp, eng.samples(), cfg
    eng.close()
    return out, (hz, hu)


def test_sweep_replay(gpu_lib):
    name = sc.REPLAY_CASE
    case = sc.BY_NAME[name]
    assert (case.kind, case.nf, case.G) == ("logistic", 3, 129)
    ref, _ = _replay(name, {"NMC_SWEEP": "0"})
    assert ref[3]["kernel"].startswith("nmc_k_run<"), ref[3]
    for env in ({}, {"NMC_ZIN": "1"}):
        o, (hz, hu) = _replay(name, env)
        _assert_sweep(case, o[3])
        assert o[3]["zin"] == (1 if env else 0), o[3]
        moved = _not_vacuous(case, o[0])
        print("SWEEP %-30s replay zin %d kernel %s waves %d acceptance %.3f moved %.3f" % (
            name, o[3]["zin"], o[3]["kernel"], o[3]["waves_per_group"], o[0].mean(), moved))
        _assert_same(o, ref, (name, "replay", env))
        # the hyper columns are numpy's sums of the recorded values (tests/gibbs_order.py)
        go.check(o[2], sc.run_of(name).state.s2, hz, hu, case.G, case.P, (name, env))


@pytest.mark.parametrize("case", [c for c in sc.CASES if c.role == "over"], ids=repr)
def test_over_limit_leaves_the_sweep(gpu_lib, case):
    """One row more than the carve holds: rows beyond LDS, nmc_k_run (whose stored group LLs
    are the group kernel's, as in tests/test_gpu_rowpaths.py)."""
    twin = sc.BY_NAME[case.name.replace("over-", "limit-")]
    assert _sweep_run(twin.name)[3]["kernel"] == twin.kernel
    acc, llp, rows, cfg = _run(case.name)
    print("SWEEP %-30s kernel %s waves %d acceptance %.3f" % (
        case.name, cfg["kernel"], cfg["waves_per_group"], acc.mean()))
    assert cfg["kernel"].startswith(case.kernel) and cfg["kernel"].endswith(", false>"), cfg
    assert cfg["mode"] != "NMC_MODE_SYNC_OWN" and cfg["split_members"] == 1, cfg
    assert numpy.array_equal(cfg["state"]["ll"], _group_ll(case.name, cfg["state"]["value"]))
    _not_vacuous(case, acc)


@pytest.mark.parametrize("case", [c for c in sc.CASES if c.role == "unreachable"], ids=repr)
def test_unreachable_instantiations(gpu_lib, case):
    """FamLinreg<7>, FamLogistic<7>, FamGaussMean<4> over 129 groups of one to three rows: no
    room for a row beside the hyper state, so never the sweep."""
    fam, sizes = sc.model(case.name)
    eng = Engine(fam, sizes, case.C, "partial", None)
    cfg = eng.launch_config()
    eng.close()
    print("SWEEP %-30s kernel %s waves %d" % (case.name, cfg["kernel"], cfg["waves_per_group"]))
    assert cfg["kernel"].startswith(case.kernel) and cfg["kernel"].endswith(", false>"), cfg
    assert cfg["mode"] != "NMC_MODE_SYNC_OWN", cfg
