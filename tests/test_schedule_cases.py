"""CPU: the recording schedule.

* nmc_record_row (csrc/dev.h), the function every kernel that writes the sample store calls,
  compiled for the host (nmc_debug_record_rows_host) and held exhaustively to
  nestmc.sampler.record_iterations, with the row count of nmc_set_schedule's own loop
  (nmc_debug_schedule_rows), for every reference schedule(n_iter, n_samples) too;
* the cases of tests/schedule_cases.py: the schedules' written-out iterations, the call
  plans' boundaries, and that each case's oracle run moves, so that a store shifted by one
  iteration differs from the right one in every case (tests/test_gpu_schedule.py).
"""

import ctypes
import os

import numpy
import pytest

import schedule_cases as sc
from golden_cases import GOLDEN
from nestmc import sampler
from oracle import restatement as rs


@pytest.fixture(scope="module")
def lib():
    from nestmc import _lib
    return _lib.load()


def _int_p(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_int))


def _n_rows(lib, n_iter, burn, thin):
    n = ctypes.c_int(-1)
    assert lib.nmc_debug_schedule_rows(n_iter, burn, thin, ctypes.byref(n)) == 0
    return n.value


def _rows(lib, burn, thin, n_rows, iters):
    iters = numpy.ascontiguousarray(iters, dtype=numpy.intc)
    out = numpy.full(len(iters), -7, dtype=numpy.intc)
    assert lib.nmc_debug_record_rows_host(burn, thin, n_rows, _int_p(iters), len(iters),
                                          _int_p(out)) == 0
    return out


def _check(lib, n_iter, burn, thin):
    """Iterations 0 .. n_iter + thin under (n_iter, burn, thin); returns the row count."""
    n_rows = _n_rows(lib, n_iter, burn, thin)
    iters = numpy.arange(n_iter + thin + 1)
    got = _rows(lib, burn, thin, n_rows, iters)
    rec = sampler.record_iterations(n_iter, burn, thin)
    want = numpy.full(len(iters), -1)
    want[rec] = numpy.arange(len(rec))      # rows 0, 1, 2, ... in order; -1 everywhere else
    assert n_rows == len(rec) == sc.schedule_rows(n_iter, burn, thin), (n_iter, burn, thin)
    assert numpy.array_equal(got, want), (n_iter, burn, thin, got.tolist(), want.tolist())
    return n_rows


def test_record_row_exhaustive(lib):
    calls = 0
    for n_iter in range(41):
        for burn in range(n_iter + 1):
            for thin in range(1, 46):
                _check(lib, n_iter, burn, thin)
                calls += 1
    assert calls == sum(45 * (n + 1) for n in range(41))


def test_record_row_reference_schedules(lib):
    """schedule(n_iter, n_samples): the same, at least one row, and the reference's short-row
    behaviour (fewer rows than samples asked for) as tests/golden records it."""
    short = 0
    for n_iter in range(1, 41):
        for n_samples in range(1, n_iter + 1):
            burn, thin = sampler.schedule(n_iter, n_samples)
            assert (burn, thin) == rs.schedule(n_iter, n_samples)
            n_rows = _check(lib, n_iter, burn, thin)
            assert 1 <= n_rows <= n_samples, (n_iter, n_samples, burn, thin, n_rows)
            short += n_rows < n_samples
    assert short > 0
    k = numpy.load(os.path.join(GOLDEN, "known_answers.npz"))
    assert len(k["schedule"]) > 0
    some_short = False
    for n_iter, n_samples, burn, thin, n_rows in (tuple(int(v) for v in r)
                                                  for r in k["schedule"]):
        assert sampler.schedule(n_iter, n_samples) == (burn, thin)
        assert _check(lib, n_iter, burn, thin) == n_rows
        some_short = some_short or n_rows < n_samples
    assert some_short


def test_record_row_rejects_and_caps(lib):
    """A row count below the schedule's (nmc_record_row's own cap) gives -1 from there on."""
    got = _rows(lib, 7, 3, 2, numpy.arange(30))
    assert got[9] == 0 and got[12] == 1 and (numpy.delete(got, [9, 12]) == -1).all()
    got = _rows(lib, 3, 1, 2, numpy.arange(10))
    assert got.tolist() == [-1, -1, -1, 0, 1, -1, -1, -1, -1, -1]
    n = ctypes.c_int()
    assert lib.nmc_debug_schedule_rows(5, 6, 1, ctypes.byref(n)) != 0
    assert lib.nmc_debug_schedule_rows(5, 0, 0, ctypes.byref(n)) != 0


def test_schedules_are_what_they_say():
    for (burn, thin), iters in sc.SCHEDULES.items():
        assert sampler.record_iterations(sc.N_ITER, burn, thin) == iters, (burn, thin)
        assert rs.record_iterations(sc.N_ITER, burn, thin) == iters, (burn, thin)
        assert 0 <= burn <= sc.N_ITER
    assert sampler.schedule(26, 5) == (13, 3) and len(sc.SCHEDULES[(13, 3)]) == 4
    first = lambda b, t: -(-b // t) * t                             # noqa: E731
    assert first(6, 3) == 6 and first(7, 3) == 9 != 7 // 3 * 3      # ceil, not floor
    assert set(sc.CORE) <= set(sc.SCHEDULES) and sc.PLAN_SCHEDULE in sc.CORE
    # what the mutants of DESIGN.md move on the schedules every case runs.  Floor instead of
    # ceil: under (7, 3) and (13, 3) every recorded iteration lands one row late, the last
    # one beyond the store
    for b, t in ((7, 3), (13, 3)):
        assert [(i - b // t * t) // t for i in sc.SCHEDULES[(b, t)]] == \
            list(range(1, len(sc.SCHEDULES[(b, t)]) + 1))
    # (iter - burn) / thin is the same row wherever iter % thin == 0 and iter >= burn, since
    # 0 <= first - burn < thin: an equivalent mutant, no test can tell it
    for b in range(41):
        for t in range(1, 46):
            assert all((i - b) // t == (i - first(b, t)) // t
                       for i in range(first(b, t), 100, t))
    assert sc.TUNE_OFF > sc.N_ITER
    assert [i for i in range(1, sc.TUNE_BURN) if i % sc.TUNE_ON == 0] == [5, 10]
    rec = sc.SCHEDULES[(sc.TUNE_BURN, 3)]
    assert [i - sc.TUNE_BURN for i in rec] == [2, 5, 8, 11]


def test_call_plans_cover_the_boundaries():
    rec = set(sc.SCHEDULES[sc.PLAN_SCHEDULE])
    burn = sc.PLAN_SCHEDULE[0]
    assert {9, 12} <= rec
    ends = {}
    for name, (launch_iters, calls) in sc.PLANS.items():
        runs = [(a, b) for op, a, b in calls if op == "run"]
        assert runs[0][0] == 0 and runs[-1][1] == sc.N_ITER
        assert all(a[1] == b[0] for a, b in zip(runs, runs[1:])), name
        ends[name] = [b for _, b in runs[:-1]]
        res = sc.resident_calls(calls)
        assert [c for c in res if c[0] != "prefill"] == calls
        assert sum(c[0] == "prefill" for c in res) == len(runs) - 1
    assert sc.PLANS["launches-of-3"][0] == 3
    # a call that closes on an iteration not recorded (8), then a recorded iteration alone
    assert ends["9-alone"] == [9, 10] and 8 not in rec and 9 in rec
    # calls that close on a recorded iteration (9, 12), the second boundary just before one
    assert ends["close-on-recorded"] == [10, 12, 13] and {9, 12} <= rec and 11 not in rec
    assert ends["boundary-at-burn"] == [burn]
    assert set(sc.PLAN_CASES) <= set(sc.NAMES) and set(sc.TUNE_CASES) <= set(sc.NAMES)
    assert set(sc.RESIDENT_CASES) < set(sc.PLAN_CASES)
    for name in sc.PLAN_CASES:    # csrc/fam_ops.h nmc_run_kernel_res, nmc_set_resident
        c = sc.BY_NAME[name]
        has = (c.kernel.startswith("nmc_k_run<") and sc.build(name).fam.n_fields <= 3
               and set(c.modes) <= {"NMC_MODE_SYNC_REG", "NMC_MODE_HALF", "NMC_MODE_NOPOOL"})
        assert has == (name in sc.RESIDENT_CASES), name
    for name in sc.CONTINUED:
        launch_iters, calls = sc.PLANS[name]
        assert launch_iters == 0 and all(op == "run" for op, _, _ in calls) and len(calls) > 1


def test_cases_take_the_shapes_of_the_table():
    by = sc.BY_NAME
    assert len(sc.NAMES) == len(set(sc.NAMES)) == 15
    for c in sc.CASES:
        b = sc.build(c.name)
        G = len(c.sizes)
        assert b.st.value.shape == (c.C, c.P, G) and b.scale.shape == (c.C, c.P, G)
        # two chain blocks, the second one short (the split cases' 64 or 66 chains aside)
        assert 64 <= c.C <= 70 and (c.C > 64 or c.name in ("partial-split", "sweep-off-1"))
        assert b.fam.obs().shape[0] == sum(c.sizes)
        assert b.sel.tolist() == [0, 1, c.C - 1]
    assert by["reg"].sizes == [12, 0, 7, 1, 23] and by["reg"].C == 70
    assert len(by["lds"].sizes) == 70 and 64 < 70 <= 128
    assert by["sweep-off-1"].sizes == by["sweep"].sizes and by["sweep-off-1"].C == 64
    for n in ("sweep", "sweep-gsep", "sweep-takeover", "sweep-off", "launch"):
        assert len(by[n].sizes) == 129 and by[n].sizes == by["sweep"].sizes and by[n].C == 70
        # one shape, one start: the five can be compared with each other
        assert sc.build(n).st is not None
        assert numpy.array_equal(sc.build(n).st.value, sc.build("sweep").st.value)
    assert by["sweep-takeover"].launch_iters == 2
    assert by["p4"].P == 4 and by["p4"].C == 66
    assert by["complete"].sizes == [43] and by["complete-split"].sizes == [8200]
    assert by["partial-split"].C == 64 and len(set(by["partial-split"].sizes)) == 1
    # csrc/nestmc.hip nmc_create: {x, y} rows split above 2 * 4096 rows per group
    assert by["partial-split"].sizes[0] == 2 * 4096 + 1
    assert sc.build("user").fam.family == "user"
    # every caller of nmc_record_row is some case's
    sites = {s.split(" ")[0] for c in sc.CASES for s in c.sites}
    assert sites == {"store_pending", "nmc_hyper", "nmc_hyper_compute", "nmc_hyper_finish",
                     "sweep.h", "sweep_gibbs.h"}
    assert (7, 3) in sc.CORE and 7 % 3 != 0        # ... on a burn that is no multiple of thin


def test_identity_list():
    assert [s for n, s in sc.IDENTITY if n == "reg"] == list(sc.SCHEDULES)
    for name in sc.NAMES[1:]:
        assert [s for n, s in sc.IDENTITY if n == name] == sc.CORE


@pytest.mark.parametrize("name", sc.NAMES)
def test_oracle_moves_and_thins(name):
    c = sc.BY_NAME[name]
    acc, llp, iters, rows, margin = sc.oracle(name, 0, 1)
    cols = c.P * (len(c.sizes) + (2 if sc.build(name).pooling == "partial" else 0))
    assert iters == list(range(sc.N_ITER)) and rows.shape == (3, sc.N_ITER, cols)
    print("SCHEDULE %-15s oracle acceptance %.3f least margin %.3g" % (name, acc.mean(), margin))
    assert 0.05 < acc.mean() < 0.95, (name, acc.mean())
    assert numpy.all(numpy.isfinite(rows))
    # a store shifted by one iteration is another store: every recorded iteration's rows
    # differ from the rows before and the rows after it (over the chains the oracle runs: a
    # chain of three cells does reject all three proposals of an iteration now and then)
    recorded = sorted({i for s in (sc.SCHEDULES if name == "reg" else sc.CORE)
                       for i in sc.SCHEDULES[s]})
    def differs(block, what):
        for i in recorded:
            for j in (i - 1, i + 1):
                if 0 <= j < sc.N_ITER:
                    assert (block[:, i, :] != block[:, j, :]).any(), (name, what, i, j)

    differs(rows, "rows")
    if sc.build(name).pooling == "partial":
        # ... and so do the hyper columns alone and the value columns alone: either part of a
        # row in the wrong iteration shows by itself
        G = len(c.sizes)
        hyper = [p * (G + 2) + k for p in range(c.P) for k in (0, 1)]
        assert (rows[:, 1:, hyper] != rows[:, :-1, hyper]).all()
        differs(numpy.delete(rows, hyper, axis=2), "values")
    # the oracle thins on its own: the recorded iterations and rows of every schedule
    for (burn, thin) in (sc.SCHEDULES if name == "reg" else sc.CORE):
        a2, l2, it2, r2, _ = sc.oracle(name, burn, thin)
        assert it2 == sampler.record_iterations(sc.N_ITER, burn, thin) == \
            sc.SCHEDULES[(burn, thin)]
        assert numpy.array_equal(a2, acc) and numpy.array_equal(l2, llp, equal_nan=True)
        assert numpy.array_equal(r2, rows[:, it2, :])
