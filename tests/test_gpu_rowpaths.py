"""GPU: every likelihood row path and Gibbs geometry edge, reached by its shape.

csrc/nestmc.hip (nmc_create, choose_geometry) picks a row loop and a tiling from
(n_fields, rows per group, groups) alone; rowpath_cases.CASES holds one shape per choice,
and every test asserts from Engine.launch_config() that its shape took the path it names.

1. test_group_ll_reference: nmc_k_group_part/_fin (eval_group_ll) against the
   numpy.longdouble reference, within the derived bound
       |dev - ref| <= (n_member / 64 + 48 + 4 (nf + 4)) 2^-53 A
   (rowpath_cases.bound_units), and never beyond the suite's 1e-10 |ref| + 1e-9.
2. test_step_equals_group_kernel: after a short run the step kernel's stored group LLs are
   eval_group_ll of its stored values BIT FOR BIT -- the quad / paired / broadcast LDS
   loops, the scalar-load loop and the staged loop against the group kernel's summation of
   the same rows (ll_kernels.h: "a chain's stored group LL never depends on which kernel
   produced it") -- and the variants of a path (NMC_ROWS, NMC_HALF,
   NMC_PERSIST) agree with each other bit for bit.
3. test_chain_matches_oracle: oracle chain parity on the paths that never had one.
4. test_gibbs_geometry_edges: the Gibbs update at numpy's unroll and leaf boundaries and at
   the hand-off boundaries of the kernels.

5. test_group_ll_fixed_order_model: the documented summation order itself, restated in exact
   float64 arithmetic for y-only regression rows, bit for bit (pins nmc_tiles).

Device error of eval_group_ll, worst |dev - ref| / (2^-53 A) over 65 + 1 chains per case,
measured on an MI355X (the bound is 71 .. 200 in these units, never below 68).  Beyond LDS
the group kernel runs the scalar-load loop at every row width; the step kernel's loops --
the staged loop among them -- have the same error, being bit-identical to it (test 2).

    family     rows in LDS             beyond LDS, nf <= 4   beyond LDS, nf > 4   row split
    linreg     2.30 (nf 1..9; tiles)   2.63                  1.19                 1.49 (LDS)
    gauss      2.55 (nf 1..8; balance) 1.83                  2.30                 -
    logistic   5.56 (nf 1..9)          1.49                  8.27                 2.02 / 5.58

(row split, logistic: members on the scalar-load loop / on the staged loop's rows.)  The
float64 oracle, summing sequentially, reaches 33.7 on the same shapes
(tests/test_rowpath_reference.py).

What the matrix found: nmc_ll_rows_staged clamped its LDS-DMA reads at the last aligned
16 bytes wholly inside the group, so a group ENDING on an odd double offset (odd n_fields x
an odd row count before its end) lost its last double -- the y of its last row -- and summed
a stale value instead.  Every staged case with odd n_fields failed tests 2 and 3 until the
clamp moved to the 16 bytes that hold the last double (rows.h nmc_ll_rows_staged).
"""

import numpy
import pytest

import rowpath_cases as rp
from rowpath_cases import environ as _environ, gibbs_mode as _gibbs_mode, \
    gibbs_model as _gibbs_model
from gpu_cases import partial_state, run_engine, run_oracle
from nestmc.engine import Engine
from oracle import restatement as rs

pytestmark = pytest.mark.gpu

C = 65      # one full chain block and a partly filled second one


def _engine(case, n_chains, env=None, seed=0, chain_base=0):
    m = rp.model(case.name)
    with _environ(env):
        return Engine(m.fam, case.sizes, n_chains, case.pooling, m.priors, seed=seed,
                      chain_base=chain_base)


def _want_half(case, n_chains):
    """choose_geometry: none/complete pooling on the paired loop whose 64-chain grid fills at
    most half the CUs runs 32 chains per workgroup."""
    blocks = -(-n_chains // 64)
    return (case.pooling != "partial" and case.S == 1 and case.lds and case.nf <= 4
            and blocks * case.G * 2 <= rp.NCU)


def _assert_path(case, cfg, n_chains, env=None):
    """The launch took the path the case means to test."""
    env = env or {}
    what = (case.name, env, cfg)
    assert cfg["split_members"] == case.S, what
    assert cfg["kernel"].startswith("nmc_k_run<"), what
    assert cfg["kernel"].endswith(", true>" if case.lds else ", false>"), what
    if case.pooling == "partial":
        if env.get("NMC_PERSIST") == "0":
            assert not cfg["persistent"] and cfg["mode"] == "NMC_MODE_LAUNCH", what
        else:
            assert cfg["persistent"] and cfg["mode"] == "NMC_MODE_SYNC_REG", what
        assert cfg["chains_per_block"] == 64, what
    else:
        half = (_want_half(case, n_chains) and env.get("NMC_HALF") != "0"
                and env.get("NMC_ROWS") != "bcast")
        assert cfg["mode"] == ("NMC_MODE_HALF" if half else "NMC_MODE_NOPOOL"), what
        assert cfg["chains_per_block"] == (32 if half else 64), what


@pytest.mark.parametrize("case", rp.CASES, ids=repr)
def test_group_ll_reference(gpu_lib, case):
    m = rp.model(case.name)
    for n_chains in (C, 1):
        theta = rp.thetas(case.name, n_chains, seed=n_chains)
        eng = _engine(case, n_chains)
        _assert_path(case, eng.launch_config(), n_chains)
        got = eng.eval_group_ll(theta)
        eng.close()
        ref, A = rp.reference(m.fam, case.sizes, theta)
        tol = rp.tolerance(case.n_member, case.nf, ref, A)
        err = numpy.abs(numpy.asarray(got.astype(rp.LD) - ref, float))
        worst = rp.ratio(got, ref, A).max()
        print("RATIO group %-24s C=%-2d worst %.3f of %.1f" % (
            case.name, n_chains, worst, rp.bound_units(case.n_member, case.nf)))
        assert numpy.all(numpy.isfinite(got)), case.name
        bad = numpy.argwhere(~(err <= tol))
        assert bad.size == 0, (case.name, n_chains, bad[:5], worst)
        assert numpy.all(got[:, numpy.asarray(case.sizes) == 0] == 0.0)


def test_group_ll_fixed_order_model(gpu_lib):
    """The documented order of one sum -- nmc_tiles' partition, the row blocks' four
    accumulators, the tail rows, the 16-slot combine, finish_fast -- restated in exact float64
    arithmetic for y-only regression rows: eval_group_ll must equal it BIT FOR BIT at every
    tile edge (1, 15 / 16 / 17, 63 / 64 / 65, 1023 / 1024 / 1025 rows)."""
    case = rp.BY_NAME["order-linreg1"]
    m = rp.model(case.name)
    n_chains = 3
    theta = rp.thetas(case.name, n_chains, seed=9)
    eng = _engine(case, n_chains)
    _assert_path(case, eng.launch_config(), n_chains)
    got = eng.eval_group_ll(theta)
    eng.close()
    y = m.fam.obs()[:, 0]
    off = numpy.concatenate([[0], numpy.cumsum(case.sizes)])
    for g in range(case.G):
        for c in range(n_chains):
            want = rp.linreg1_fixed_order(y[off[g]:off[g + 1]], theta[c, 0, g])
            assert got[c, g] == want, (case.sizes[g], c, got[c, g], want)


def _step_run(case, env=None, seed=31):
    """A short run (burn 0, thin 1, trace on) from a start whose LLs are the device's own
    eval_group_ll; returns flags, proposal LLs, rows, launch config, final state and the
    group kernel's LLs of the final values."""
    value, lp, mu, s2, scale = rp.start(case.name, C)
    n_iter = case.step_iters
    eng = _engine(case, C, env=env, seed=seed, chain_base=3)
    ll0 = eng.eval_group_ll(value)
    eng.set_state(value, lp, ll0, mu, s2, scale=scale)
    eng.set_schedule(n_iter, 0, 1, tune_interval=100)
    eng.set_trace(True)
    eng.run(0, n_iter)
    eng.synchronize()
    acc, llp = eng.trace(n_iter)
    rows = eng.samples()
    cfg = eng.launch_config()
    state = eng.get_state()
    ll1 = eng.eval_group_ll(state["value"])
    eng.close()
    return acc, llp, rows, cfg, state, ll1, ll0


def _variants(case):
    v = {}
    if case.lds and case.nf <= 4:
        v["bcast"] = {"NMC_ROWS": "bcast"}            # the one-chain broadcast loop
        if case.kind.startswith("linreg") and case.nf == 2:
            v["pair"] = {"NMC_ROWS": "pair"}          # the paired loop where quad is default
    if _want_half(case, C):
        v["full"] = {"NMC_HALF": "0"}                 # 64 chains per workgroup
    if case.pooling == "partial" and case.S == 1:
        v["launch"] = {"NMC_PERSIST": "0"}            # one launch per iteration
    return v


@pytest.mark.parametrize("case", rp.CASES, ids=repr)
def test_step_equals_group_kernel(gpu_lib, case):
    acc, llp, rows, cfg, state, ll1, ll0 = _step_run(case)
    _assert_path(case, cfg, C)
    # not vacuous: the chains move, in most cells that have rows
    nonempty = numpy.asarray(case.sizes) > 0
    moved = acc.astype(bool).any(axis=(1, 2))[:, nonempty].mean()
    print("STEP %-24s acceptance %.3f, cells moved %.3f" % (case.name, acc.mean(), moved))
    assert moved >= 0.5, (case.name, moved)
    assert 0.05 < acc.mean() < 0.95, (case.name, acc.mean())
    assert numpy.all(numpy.isfinite(ll0))
    # the step kernel's stored LL is the group kernel's LL of the stored values
    bad = numpy.argwhere(state["ll"] != ll1)
    assert bad.size == 0, (case.name, bad[:5], state["ll"][tuple(bad[0])], ll1[tuple(bad[0])])
    # recorded rows of the last iteration are the stored values
    last = rs.State(state["value"], state["log_prior"], state["ll"], state["mu"], state["s2"])
    assert numpy.array_equal(rows[:, -1, :], rs.row_values(last, case.pooling == "partial"))
    for name, env in _variants(case).items():
        other = _step_run(case, env=env)
        _assert_path(case, other[3], C, env)
        for k in range(3):
            assert numpy.array_equal(other[k], (acc, llp, rows)[k], equal_nan=True), \
                (case.name, name, k)
        assert numpy.array_equal(other[4]["ll"], state["ll"]), (case.name, name)
        assert numpy.array_equal(other[5], ll1), (case.name, name)


ORACLE_CASES = ["scalar-linreg2-4097", "scalar-linreg2-8192", "scalar-linreg2sig-8192",
                "split-scalar", "split-staged", "staged-logistic5-last",
                "staged-logistic5-first", "staged-logistic9-first", "staged-linreg9-last",
                "R-linreg-nf1", "R-logistic-nf9"]


@pytest.mark.parametrize("name", ORACLE_CASES)
def test_chain_matches_oracle(gpu_lib, name):
    case, m = rp.BY_NAME[name], rp.model(name)
    value, lp, mu, s2, scale = rp.start(name, C)
    nested = rs.Nested(m.fam, case.sizes)
    sel = numpy.array([0, 1, C - 1])
    ll = numpy.full((C, case.G), numpy.nan)
    if case.pooling == "partial":
        ll[sel] = [nested.group_ll(value[c]) for c in sel]
    st = rs.State(value, lp, ll, mu, s2)
    n_iter, seed, base = case.step_iters, 77, 5
    kw = dict(pooling=case.pooling, priors=m.priors, tune_interval=3, scale=scale)
    if case.pooling == "partial":       # (the other chains' LLs: the device's own)
        eng = _engine(case, C)
        dev_ll = eng.eval_group_ll(value)
        eng.close()
        assert numpy.allclose(dev_ll[sel], ll[sel], rtol=1e-10, atol=1e-9)
        dev_ll[sel] = ll[sel]
        st.ll = dev_ll
    acc, llp, rows, cfg = run_engine(m.fam, case.sizes, st, numpy.arange(C), base, n_iter, seed,
                                     **kw)
    _assert_path(case, cfg, C)
    oacc, ollp, orows, margin = run_oracle(nested, st, sel, sel + base, n_iter, seed, **kw)
    bad = numpy.argwhere(acc[sel].astype(bool) != oacc)
    assert bad.size == 0, "flag mismatch at %s (min decision margin %g)" % (bad[:5], margin)
    assert numpy.allclose(llp[sel], ollp, rtol=1e-10, atol=1e-9, equal_nan=True)
    assert numpy.allclose(rows[sel], orows, rtol=1e-9, atol=1e-9, equal_nan=True)
    assert acc.mean() > 0.02


@pytest.mark.parametrize("G", [2, 3, 7, 8, 9, 63, 64, 65, 120, 121, 127, 128, 129, 136, 512,
                               513])
@pytest.mark.parametrize("kind", ["linreg2", "gauss1"])
def test_gibbs_geometry_edges(gpu_lib, kind, G):
    """numpy's unrolled-by-8 boundary (7 / 8 / 9) and G = 2 (Gamma shape 1/2), the register /
    LDS hand-off (64 / 65), the last G whose two-parameter payload fits LDS (120 / 121; with
    one parameter it fits up to 128), one leaf / two leaves and nmc_k_run / nmc_k_sweep
    (128 / 129), four leaves (512), and five (513: no auxiliary Gibbs wave and no sweep --
    nmc_k_run's all-wave update over the five leaves, which runs and matches the oracle).
    Rows (hyper-parameter columns included) and flags of every chain against the oracle."""
    fam, sizes = _gibbs_model(kind, G)
    P = fam.n_params
    n_iter, seed, base = (10 if G <= 136 else 6), 13, 2
    st, _ = partial_state(fam, sizes, C, P)
    sel = numpy.arange(C)
    dev = run_engine(fam, sizes, st, sel, base, n_iter, seed, tune_interval=3)
    cfg = dev[3]
    kernel, modes = _gibbs_mode(fam, sizes)
    want = {2: "SYNC_REG", 64: "SYNC_REG", 65: "SYNC_LDS", 120: "SYNC_LDS", 129: "SYNC_OWN",
            512: "SYNC_OWN", 513: "SYNC"}.get(G)
    assert want is None or modes[0] == "NMC_MODE_" + want, (G, modes)
    assert modes[0] == "NMC_MODE_" + {"linreg2": "SYNC", "gauss1": "SYNC_LDS"}[kind] or G != 128
    assert cfg["kernel"].startswith(kernel) and cfg["mode"] in modes, (cfg["kernel"], cfg["mode"])
    assert cfg["split_members"] == 1 and cfg["chains_per_block"] == 64, cfg
    others = {"launch": {"NMC_PERSIST": "0"}}
    if 128 < G <= 512:
        others["run"] = {"NMC_SWEEP": "0"}
    for name, env in others.items():
        o = run_engine(fam, sizes, st, sel, base, n_iter, seed, tune_interval=3, env=env)
        if name == "launch":
            assert not o[3]["persistent"], o[3]
        assert o[3]["kernel"].startswith("nmc_k_run<"), o[3]
        for k in range(3):
            assert numpy.array_equal(o[k], dev[k], equal_nan=True), (name, k)
    nested = rp.FastNested(fam, sizes)
    oacc, ollp, orows, margin = run_oracle(nested, st, sel, sel + base, n_iter, seed,
                                           tune_interval=3)
    bad = numpy.argwhere(dev[0].astype(bool) != oacc)
    assert bad.size == 0, "flag mismatch at %s (min decision margin %g)" % (bad[:5], margin)
    assert numpy.allclose(dev[1], ollp, rtol=1e-10, atol=1e-9, equal_nan=True)
    assert numpy.allclose(dev[2], orows, rtol=1e-9, atol=1e-9, equal_nan=True)
    assert numpy.all(numpy.isfinite(dev[2]))
    assert dev[0].mean() > 0.02
