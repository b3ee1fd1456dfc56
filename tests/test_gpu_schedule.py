"""GPU: which iteration lands in which row of the sample store, on every kernel that writes
the store (csrc/dev.h nmc_record_row and its six callers; tests/schedule_cases.py holds the
cases, the schedules and the call plans, tests/test_schedule_cases.py what they reach).

Every case asserts its path from Engine.launch_config() (kernel, mode, persistent, chains per
block, split members, Gibbs fall-backs), so a case that stops reaching its path fails.

a. test_thinned_store_is_the_baselines_rows: with a tune interval above n_iter the trajectory
   depends on neither burn nor thin, so under every schedule (burn, thin) the store must be
   rows record_iterations(26, burn, thin) of the baseline run (burn 0, thin 1) BIT FOR BIT --
   every column, hyper columns included, every chain -- with the baseline's flags, proposal
   LLs, final state, log priors and accept counts, Engine.n_rows rows, and none of the quiet
   NaNs the store was filled with before the run.  Schedules without rows run to the end.
b. test_call_plans: launches of three iterations and calls whose boundaries fall between, on
   and just after a recorded iteration: the one-call store bit for bit.  Each plan runs on
   separate launches and again with set_resident and prefilled variates.  reg and half have a
   resident kernel instance: resident_stats() must show the resident launch and, on the plans
   of plain runs, calls that continued it.  lds, sweep and p4 have none: resident_stats()
   must show the request declined, and the second run holds that asking changes nothing.
c. test_burn_drives_tuning_and_recording: tune interval 5, burn 13 -- the thinned run is rows
   2, 5, 8, 11 of the thin-1 run, with its tuned scales.
d. test_rescheduling: two set_schedule calls on one engine are the last one's fresh engine.
e. test_thinned_run_matches_oracle: schedule (7, 3) on chains 0, 1 and C - 1 against the numpy
   oracle, which thins on its own: independent of the thin-1 path.

The baseline and the (7, 3) run of a case are computed once and shared, unchanged.
"""

import functools

import numpy
import pytest

import schedule_cases as sc
from gpu_cases import run_engine
from nestmc import sampler

pytestmark = pytest.mark.gpu

TRIPLE = ("accept flags", "proposal LLs")
STATE = ("value", "log_prior", "ll", "mu", "s2", "scale")
SENT = int(sc.SENTINEL)


def _run(name, burn, thin, **kw):
    b = sc.build(name)
    kw = dict(sc.engine_kw(name, burn, thin), **kw)
    return run_engine(b.fam, b.sizes, b.st, numpy.arange(b.case.C), sc.BASE, sc.N_ITER, sc.SEED,
                      sentinel=sc.SENTINEL, **kw)


def _assert_path(name, cfg, launch_iters=None):
    c = sc.BY_NAME[name]
    what = (name, {k: v for k, v in cfg.items() if numpy.ndim(v) == 0 and k != "state"})
    assert cfg["kernel"].startswith(c.kernel), what
    assert cfg["mode"] in c.modes, what
    assert cfg["persistent"] == c.persistent, what
    assert c.cpb is None or cfg["chains_per_block"] == c.cpb, what
    assert cfg["chain_blocks"] == -(-c.C // cfg["chains_per_block"]), what
    if c.split is None:
        assert cfg["split_members"] > 1, what
    else:
        assert cfg["split_members"] == c.split, what
    blocks = -(-c.C // 64)
    if c.fallbacks == "all":      # every (launch, chain block) fell back
        li = launch_iters or c.launch_iters
        assert cfg["gibbs_fallbacks"] == -(-sc.N_ITER // li) * blocks, what
    else:
        assert cfg["gibbs_fallbacks"] == 0, what
    # the sweep's Gibbs workgroups: their own kernel where the case says so, else in the grid
    assert cfg["gibbs_separate"] == ("NMC_GSEP" in c.env), what
    if name == "complete":
        assert len(c.sizes) == 1
    if name == "p4":
        assert cfg["state"]["value"].shape[1] == 4


def _bits(a):
    return numpy.ascontiguousarray(a, dtype=numpy.float64).view(numpy.uint64)


def _assert_store(name, got, rows_want, what):
    """The store of run ``got`` is rows_want bit for bit, sized as the schedule says, with no
    sentinel left."""
    c = sc.BY_NAME[name]
    rows, cfg = got[2], got[3]
    cols = c.P * (len(c.sizes) + (2 if sc.build(name).pooling == "partial" else 0))
    assert cfg["cols"] == cols, what
    assert rows.shape == (c.C, cfg["n_rows"], cols) == rows_want.shape, (what, rows.shape)
    g, w = _bits(rows), _bits(rows_want)
    assert not (g == SENT).any(), (what, "rows nobody wrote", numpy.argwhere(g == SENT)[:5])
    bad = numpy.argwhere(g != w)
    assert bad.size == 0, (what, len(bad), "first (chain, row, col):", bad[:5].tolist())


def _assert_trajectory(got, want, what):
    """Flags, proposal LLs, final state, log priors and accept counts, bit for bit."""
    for k, part in enumerate(TRIPLE):
        assert got[k].shape == want[k].shape, (what, part)
        assert numpy.array_equal(_bits(got[k]) if k else got[k],
                                 _bits(want[k]) if k else want[k]), (what, part)
    for key in STATE:
        assert numpy.array_equal(got[3]["state"][key], want[3]["state"][key], equal_nan=True), \
            (what, "state", key)
    assert numpy.array_equal(got[3]["log_prior"], want[3]["log_prior"], equal_nan=True), what
    assert numpy.array_equal(got[3]["accept"], want[3]["accept"]), what


@functools.lru_cache(maxsize=None)
def _baseline(name):
    """Burn 0, thin 1: every iteration's row.  Shared and left unchanged."""
    out = _run(name, 0, 1)
    _assert_path(name, out[3])
    acc, llp, rows, cfg = out
    c = sc.BY_NAME[name]
    assert cfg["n_rows"] == sc.N_ITER and rows.shape[:2] == (c.C, sc.N_ITER)
    assert not (_bits(rows) == SENT).any(), name
    assert numpy.all(numpy.isfinite(rows)), name
    # the chains move, on the device too: no two neighbouring rows of the store are equal
    assert 0.05 < acc.mean() < 0.95, (name, acc.mean())
    assert (rows[:, 1:, :] != rows[:, :-1, :]).any(axis=(0, 2)).all(), name
    # tuning was off: the scales are the start's
    assert numpy.array_equal(cfg["state"]["scale"], sc.build(name).scale), name
    for a in out[:3]:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _thinned(name, burn, thin):
    out = _run(name, burn, thin)
    _assert_path(name, out[3])
    for a in out[:3]:
        a.setflags(write=False)
    return out


@pytest.mark.parametrize("name,schedule", sc.IDENTITY,
                         ids=["%s-%d-%d" % (n, s[0], s[1]) for n, s in sc.IDENTITY])
def test_thinned_store_is_the_baselines_rows(gpu_lib, name, schedule):
    burn, thin = schedule
    base = _baseline(name)
    got = _thinned(name, burn, thin)
    iters = sampler.record_iterations(sc.N_ITER, burn, thin)
    assert iters == sc.SCHEDULES[schedule]
    what = (name, "burn %d thin %d" % schedule)
    assert got[3]["n_rows"] == len(iters) == sc.schedule_rows(sc.N_ITER, burn, thin), what
    _assert_store(name, got, base[2][:, iters, :], what)
    _assert_trajectory(got, base, what)


@pytest.mark.parametrize("name", sc.PLAN_CASES)
def test_call_plans(gpu_lib, name, monkeypatch):
    monkeypatch.setenv("NMC_RESIDENT_IDLE_US", "5000")
    burn, thin = sc.PLAN_SCHEDULE
    one = _thinned(name, burn, thin)
    iters = sc.SCHEDULES[sc.PLAN_SCHEDULE]
    want = _baseline(name)[2][:, iters, :]
    _assert_store(name, one, want, (name, "one call"))
    for plan, (launch_iters, calls) in sc.PLANS.items():
        for resident in (False, True):
            what = (name, plan, "resident" if resident else "launched")
            got = _run(name, burn, thin, launch_iters=launch_iters,
                       calls=sc.resident_calls(calls) if resident else calls,
                       resident=resident)
            _assert_path(name, got[3])
            r = got[3]["resident"]
            print("SCHEDULE %-6s %-18s %-8s resident launches %d continued calls %d" % (
                name, plan, what[2], r["launches"], r["calls"]))
            if not resident:
                assert not r["enabled"] and r["launches"] == 0 and r["calls"] == 0, (what, r)
            elif name in sc.RESIDENT_CASES:
                # an instance with a resident form (schedule_cases.RESIDENT_CASES): launches of
                # a fixed length are never resident, and a state read parks the launch
                assert r["enabled"], (what, r)
                if launch_iters == 0:
                    assert r["launches"] >= 1, (what, r)
                else:
                    assert r["launches"] == 0 and r["calls"] == 0, (what, r)
                if plan in sc.CONTINUED:
                    assert r["calls"] >= 1, (what, r)
            else:
                # no resident form of this kernel: the request is declined, and the plan runs
                # on separate launches with set_resident called
                assert not r["enabled"] and r["launches"] == 0 and r["calls"] == 0, (what, r)
            _assert_store(name, got, want, what)
            _assert_trajectory(got, one, what)


@pytest.mark.parametrize("name", sc.TUNE_CASES)
def test_burn_drives_tuning_and_recording(gpu_lib, name):
    burn = sc.TUNE_BURN
    every = _run(name, burn, 1, tune_interval=sc.TUNE_ON)
    third = _run(name, burn, 3, tune_interval=sc.TUNE_ON)
    for o in (every, third):
        _assert_path(name, o[3])
    assert every[3]["n_rows"] == sc.N_ITER - burn and third[3]["n_rows"] == 4
    pick = [i - burn for i in sc.SCHEDULES[(burn, 3)]]
    assert pick == [2, 5, 8, 11]
    _assert_store(name, third, every[2][:, pick, :], (name, "tuned, thin 3 against thin 1"))
    _assert_trajectory(third, every, (name, "tuned"))
    changed = (every[3]["state"]["scale"] != sc.build(name).scale).mean()
    print("SCHEDULE %-6s tuned scales changed: %.3f" % (name, changed))
    assert changed > 0.3, (name, changed)
    # and the tuned run is another trajectory than the untuned baseline's
    assert not numpy.array_equal(every[2][:, pick, :],
                                 _baseline(name)[2][:, sc.SCHEDULES[(burn, 3)], :])


def test_rescheduling(gpu_lib):
    burn, thin = sc.PLAN_SCHEDULE
    fresh = _thinned("reg", burn, thin)
    again = _run("reg", burn, thin, pre_schedules=[(sc.N_ITER, 0, 1)])
    _assert_path("reg", again[3])
    assert again[3]["n_rows"] == fresh[3]["n_rows"] == len(sc.SCHEDULES[sc.PLAN_SCHEDULE])
    _assert_store("reg", again, fresh[2], ("reg", "set_schedule twice"))
    _assert_trajectory(again, fresh, ("reg", "set_schedule twice"))


@pytest.mark.parametrize("name", sc.NAMES)
def test_thinned_run_matches_oracle(gpu_lib, name):
    burn, thin = sc.ORACLE_SCHEDULE
    acc, llp, rows, cfg = _thinned(name, burn, thin)
    sel = sc.build(name).sel
    oacc, ollp, oiters, orows, margin = sc.oracle(name, burn, thin)
    print("SCHEDULE %-15s kernel %s mode %s oracle acceptance %.3f least margin %.3g" % (
        name, cfg["kernel"], cfg["mode"], oacc.mean(), margin))
    assert oiters == sc.SCHEDULES[sc.ORACLE_SCHEDULE]
    assert cfg["n_rows"] == rows.shape[1] == orows.shape[1] == len(oiters), name
    bad = numpy.argwhere(acc[sel].astype(bool) != oacc)
    assert bad.size == 0, "flag mismatch at %s (min decision margin %g)" % (bad[:5], margin)
    assert numpy.allclose(llp[sel], ollp, rtol=1e-9, atol=1e-9, equal_nan=True)
    assert numpy.allclose(rows[sel], orows, rtol=1e-9, atol=1e-9, equal_nan=True)
    assert numpy.all(numpy.isfinite(rows))
