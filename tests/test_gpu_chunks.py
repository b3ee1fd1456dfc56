"""GPU: nmc_run across variate-buffer ends and counter resets changes no bit
(tests/chunk_cases.py holds the plans, their written-out figures and the host planner's model;
tests/test_chunk_cases.py what they reach).

Every kernel reads its variates at (t - vbase) of a buffer of vcap iterations, and in every
other test vcap == n_iter.  Here NMC_VARIATE_BYTES makes the buffers 1, 2, 3, 5 or 8
iterations long on the 26 iterations of schedule_cases' cases (tuning at 5 and 10, rows from
13), and nmc_debug_set_counter_wrap makes the reset of the launch-spanning counters run every
few launches.  A wrong offset does not crash: the chain reads another iteration's variates and
still looks like a chain.  So every run is compared BIT FOR BIT with the same case in one call
with nothing set -- accept flags, proposal log-likelihoods, recorded rows, the final value,
log_prior, ll, scale, mu and s2, Engine.log_prior() and the accept counts -- and asserts

* from nmc_debug_variate_plan, that vcap and the launch chunk are the plan's and (plans A-E)
  below n_iter: the buffer really was short;
* from launch_config(), the case's kernel and mode (test_gpu_schedule's check);
* that prefill_stats(), the resident launches, calls, refusal reasons in order and the reset
  count are the literals of chunk_cases.py, which the CPU test holds to the model.

The baseline of a case is computed once and shared, unchanged; reg's and half's are also held
to the numpy oracle.  No tolerance anywhere but in that comparison (the suite's 1e-9).
"""

import functools
import os

import numpy
import pytest

import chunk_cases as cc
import schedule_cases as sc
from golden_cases import Case
from gpu_cases import family_for, run_engine
from nestmc._lib import NestmcError
from nestmc.engine import Engine
from oracle import restatement as rs
from test_gpu_schedule import _assert_path, _assert_trajectory, _bits

pytestmark = pytest.mark.gpu

SENT = int(sc.SENTINEL)
ROWS = cc.N_ITER - cc.TUNE["burn"]


def _run(name, **kw):
    b = sc.build(name)
    kw = dict(sc.engine_kw(name, **cc.TUNE), **kw)
    return run_engine(b.fam, b.sizes, b.st, numpy.arange(b.case.C), sc.BASE, cc.N_ITER, sc.SEED,
                      sentinel=sc.SENTINEL, **kw)


@functools.lru_cache(maxsize=None)
def _baseline(name):
    """One call, nothing set: the buffer holds the whole run.  Shared and left unchanged."""
    out = _run(name)
    acc, llp, rows, cfg = out
    _assert_path(name, cfg)
    c = sc.BY_NAME[name]
    vp = cfg["variate_plan"]
    assert vp["vcap"] == cc.N_ITER and vp["counter_wrap"] == cc.WRAP_DEFAULT, (name, vp)
    assert vp["chunk"] == (c.launch_iters or cc.N_ITER) and vp["counter_resets"] == 0, (name, vp)
    assert cfg["split_members"] == cc.shape(name).S, (name, cfg["split_members"])
    assert rows.shape[:2] == (c.C, ROWS) and numpy.all(numpy.isfinite(rows)), name
    assert not (_bits(rows) == SENT).any(), name
    assert 0.05 < acc.mean() < 0.95, (name, acc.mean())
    # the chains move and tuning ran: a variate of the wrong iteration shows
    assert (rows[:, 1:, :] != rows[:, :-1, :]).any(axis=(0, 2)).all(), name
    assert (cfg["state"]["scale"] != sc.build(name).scale).mean() > 0.3, name
    for a in out[:3]:
        a.setflags(write=False)
    return out


def _assert_same(got, base, what):
    assert got[2].shape == base[2].shape, (what, got[2].shape)
    g, w = _bits(got[2]), _bits(base[2])
    assert not (g == SENT).any(), (what, "rows nobody wrote")
    bad = numpy.argwhere(g != w)
    assert bad.size == 0, (what, len(bad), "first (chain, row, col):", bad[:5].tolist())
    _assert_trajectory(got, base, what)


def _refusals(calls, log):
    """res_continue's refusal reasons in order: the runs that found the launch active and
    did not continue it."""
    out, prev = [], {"active": False, "calls": 0}
    for (op, _, _), entry in zip(calls, log):
        r = entry["resident"]
        if op == "run" and prev["active"] and r["calls"] == prev["calls"]:
            out.append(r["last_refusal"])
        prev = r
    return out


def _assert_figures(plan, name, cfg):
    p = cc.BY_PLAN[plan]
    e, what = p.expect, (plan, name)
    vp, r = cfg["variate_plan"], cfg["resident"]
    pl = cc.model(p, name)
    print("CHUNKS %-22s %-15s vcap %2d chunk %2d prefill %s resident %d/%d refusals %s resets %d"
          % (plan, name, vp["vcap"], vp["chunk"], cfg["prefill"], r["launches"], r["calls"],
             _refusals(p.calls, cfg["log"]), vp["counter_resets"]))
    assert vp["vcap"] == p.vcap == pl.vcap and vp["chunk"] == pl.chunk(), (what, vp)
    if not plan.startswith("F-"):
        assert vp["chunk"] <= vp["vcap"] < cc.N_ITER, (what, vp)
    assert vp["counter_wrap"] == (p.wrap or cc.WRAP_DEFAULT), (what, vp)
    assert cfg["split_members"] == cc.shape(name).S, (what, cfg["split_members"])
    assert cfg["prefill"] == e["prefill"], (what, cfg["prefill"])
    assert r["enabled"] == (p.resident and name in sc.RESIDENT_CASES), (what, r)
    assert (r["launches"], r["calls"], r["last_refusal"]) == \
        (e["launches"], e["calls"], e["last_refusal"]), (what, r)
    assert _refusals(p.calls, cfg["log"]) == e["refusals"], what
    assert vp["counter_resets"] == e["resets"], (what, vp)


@pytest.mark.parametrize("plan,name", cc.RUNS, ids=["%s-%s" % r for r in cc.RUNS])
def test_plan_is_the_baseline_bit_for_bit(gpu_lib, plan, name, monkeypatch):
    monkeypatch.setenv("NMC_RESIDENT_IDLE_US", "5000")
    p = cc.BY_PLAN[plan]
    base = _baseline(name)
    li = p.launch_iters or sc.BY_NAME[name].launch_iters
    got = _run(name, launch_iters=li, calls=p.calls, resident=p.resident, counter_wrap=p.wrap,
               schedule_env=cc.schedule_env(p, name), log_calls=True)
    _assert_path(name, got[3], launch_iters=min(li, p.vcap) if li else p.vcap)
    _assert_figures(plan, name, got[3])
    _assert_same(got, base, (plan, name))


@pytest.mark.parametrize("name", sc.RESIDENT_CASES)
def test_baseline_matches_oracle(gpu_lib, name):
    acc, llp, rows, cfg = _baseline(name)
    sel = sc.build(name).sel
    oacc, ollp, oiters, orows, margin = sc.oracle(name, **cc.TUNE)
    assert oiters == list(range(cc.TUNE["burn"], cc.N_ITER))
    bad = numpy.argwhere(acc[sel].astype(bool) != oacc)
    assert bad.size == 0, "flag mismatch at %s (min decision margin %g)" % (bad[:5], margin)
    assert numpy.allclose(llp[sel], ollp, rtol=1e-9, atol=1e-9, equal_nan=True)
    assert numpy.allclose(rows[sel], orows, rtol=1e-9, atol=1e-9, equal_nan=True)


def test_replay_at_vcap_3_matches_reference(gpu_lib, monkeypatch):
    """nmc_k_fill<true> indexes the replay arrays by the absolute iteration while it writes at
    the buffer offset: the reference's own variates through 134 launches of at most 3
    iterations must give the reference's flags and rows
    (test_gpu_prefill.test_prefill_replay_chunks_match_reference, with a short buffer)."""
    c = Case(cc.E_CASE)
    a = c.arr
    eng = Engine(family_for(c), c.sizes, c.n_chains, c.pooling, c.priors, rng="replay")
    sh = cc.E_SHAPE
    assert (eng.G, eng.P, eng.C, c.n_iter) == (sh.G, sh.P, sh.C, cc.E_N_ITER)
    eng.set_state(a["init_value"], a["init_lp"], a["init_ll"][:, 0, :],
                  a.get("init_mu"), a.get("init_s2"))
    eng.set_replay(a["z"], a["u"], a["hz"], a["hu"])
    burn, thin = rs.schedule(c.n_iter, c.n_samples)
    monkeypatch.setenv("NMC_VARIATE_BYTES", str(cc.variate_bytes(sh, cc.E_VCAP)))
    eng.set_schedule(c.n_iter, burn, thin)
    monkeypatch.delenv("NMC_VARIATE_BYTES")
    eng.set_trace(True)
    vp = eng.variate_plan()
    assert vp["vcap"] == vp["chunk"] == cc.E_VCAP < c.n_iter, vp
    half = c.n_iter // 2
    eng.run(0, half)
    eng.run(half, c.n_iter)
    acc, llp = eng.trace(c.n_iter)
    assert numpy.array_equal(acc.astype(numpy.int8), a["acc"])
    assert numpy.allclose(llp, a["ll"], rtol=1e-9, atol=1e-9, equal_nan=True)
    assert numpy.allclose(eng.samples(), a["rows"], rtol=1e-9, atol=1e-9, equal_nan=True)
    assert eng.prefill_stats() == cc.E_EXPECT["prefill"]
    eng.close()


@pytest.mark.parametrize("text", cc.ODD_BYTES)
def test_odd_variate_bytes(gpu_lib, text):
    """NMC_VARIATE_BYTES of 0, 1, a negative number and text: a buffer of at least one
    iteration, and the baseline's bits."""
    got = _run("reg", schedule_env={"NMC_VARIATE_BYTES": text})
    vp = got[3]["variate_plan"]
    print("CHUNKS NMC_VARIATE_BYTES=%r vcap %d chunk %d" % (text, vp["vcap"], vp["chunk"]))
    assert 1 <= vp["chunk"] <= vp["vcap"] <= cc.N_ITER, (text, vp)
    if text in ("0", "1", "plenty"):       # atoll: 0, 1, 0 bytes -- the least buffer
        assert vp["vcap"] == 1, (text, vp)
    _assert_path("reg", got[3])
    _assert_same(got, _baseline("reg"), ("reg", "NMC_VARIATE_BYTES=" + text))
    assert "NMC_VARIATE_BYTES" not in os.environ


def test_counter_wrap_limits(gpu_lib):
    """A limit of 0, below 0 or above 2^31 is refused (rc -1) and leaves the limit in force;
    1 and 2^31 are taken; the context then runs the baseline's bits."""
    b = sc.build("reg")
    eng = Engine(b.fam, b.sizes, b.case.C, b.pooling, b.priors, seed=sc.SEED, chain_base=sc.BASE)
    eng.set_state(b.st.value, b.st.lp, b.st.ll, b.st.mu, b.st.s2, scale=b.scale)
    with pytest.raises(NestmcError):       # (no schedule yet)
        eng.variate_plan()
    eng.set_schedule(cc.N_ITER, cc.TUNE["burn"], cc.TUNE["thin"],
                     tune_interval=cc.TUNE["tune_interval"])
    assert eng.variate_plan()["counter_wrap"] == cc.WRAP_DEFAULT == 2 ** 31
    for bad in (0, -1, 2 ** 31 + 1, 2 ** 40):
        with pytest.raises(NestmcError, match="counter wrap"):
            eng.set_counter_wrap(bad)
        assert eng.lib.nmc_debug_set_counter_wrap(eng.h, bad) == -1
        assert eng.variate_plan()["counter_wrap"] == cc.WRAP_DEFAULT, bad
    eng.set_counter_wrap(1)                # every launch resets
    assert eng.variate_plan()["counter_wrap"] == 1
    eng.set_launch_iters(9)
    eng.run(0, 18)
    eng.set_counter_wrap(2 ** 31)
    eng.run(18, cc.N_ITER)
    vp = eng.variate_plan()
    assert (vp["counter_wrap"], vp["counter_resets"], vp["chunk"]) == (2 ** 31, 2, 9), vp
    rows = eng.samples()
    eng.close()
    assert numpy.array_equal(_bits(rows), _bits(_baseline("reg")[2]))
