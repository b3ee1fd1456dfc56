"""CPU: the plans of tests/chunk_cases.py.

* every plan's written-out figures (chunks, prefill and resident statistics, refusal reasons,
  counter resets, paths taken) against chunk_cases.Planner, the host planner of
  csrc/nestmc.hip restated in Python;
* on the model's trace of every plan, the invariants the pipelined fill rests on:
    1. at every launch (and continued resident call) each iteration it reads sits at offset
       t - vbase of the launch's buffer, put there by a fill that is ordered before the
       launch, and over the plan every iteration read was filled once: what was filled is
       what was read plus what the prefill statistics call unused;
    2. every offset a fill writes or a launch reads lies in [0, vcap);
    3. no fill writes slots of a buffer that an earlier launch reads unless it is ordered
       after that launch (its rd_ev, the stream's order, or a park's host wait);
* that every path the plans claim is one whose literals show it taken, the buffer really is
  shorter than the run, and the reset plans reset at least three times with a launch without a
  reset between;
* NMC_VARIATE_BYTES for a wanted vcap (chunk_cases.variate_bytes), with the floor.

tests/test_gpu_chunks.py holds the library to the same literals on the MI355X.
"""

import pytest

import chunk_cases as cc
import schedule_cases as sc


def _figures(plan, name):
    p = cc.BY_PLAN[plan]
    f = cc.model(p, name).figures()
    if isinstance(p.expect["chunks"], int):
        f["chunks"] = len(f["chunks"])
    return f


@pytest.mark.parametrize("plan,name", cc.RUNS, ids=["%s-%s" % r for r in cc.RUNS])
def test_literals_are_the_models(plan, name):
    assert _figures(plan, name) == cc.BY_PLAN[plan].expect, (plan, name)


def check_invariants(pl):
    """The three invariants on a played Planner; returns (iterations filled, read)."""
    vcap, tr = pl.vcap, pl.trace
    slots = {0: {}, 1: {}}            # buffer -> offset -> (iteration, index of the fill)
    readers = []                      # (index, owner launch's index, buf, lo, hi)
    owner = None
    waited = -1                       # the latest launch the prefill stream has waited for
    last_join = last_park = -1
    active = False
    filled = read = 0
    for i, e in enumerate(tr):
        if e["ev"] == "join":
            last_join = i
        elif e["ev"] == "park":
            last_park, active = i, False
        elif e["ev"] == "fill":
            lo, hi = e["a"] - e["vb"], e["b"] - e["vb"]
            assert 0 <= lo < hi <= vcap, (i, e)                               # 2
            if e["stream"] == "pre":
                if e["wait"] not in ("none", None):
                    waited = max(waited, e["wait"])
            else:
                assert not active, (i, e, "a fill on the step stream behind a resident launch")
            for j, own, buf, rlo, rhi in readers:                             # 3
                if buf == e["buf"] and rlo < hi and lo < rhi:
                    ordered = e["stream"] == "main" or own <= waited or j < last_park
                    assert ordered, (i, e, "writes what", tr[j], "reads")
            for off in range(lo, hi):
                slots[e["buf"]][off] = (e["vb"] + off, i, e["stream"])
            filled += hi - lo
        elif e["ev"] in ("launch", "call"):
            if e["ev"] == "launch":
                owner = i
                active = e["resident"]
            else:
                assert active, (i, e)
            lo, hi = e["c0"] - e["vb"], e["c1"] - e["vb"]
            assert 0 <= lo < hi <= vcap, (i, e)                               # 2
            for t in range(e["c0"], e["c1"]):                                 # 1
                it, at, stream = slots[e["buf"]].get(t - e["vb"], (None, None, None))
                assert it == t, (i, e, "iteration", t, "finds", it)
                assert stream == "main" or at < last_join, (i, e, "prefill not waited for")
            readers.append((i, owner, e["buf"], lo, hi))
            read += hi - lo
    assert filled == read + pl.issued - pl.used, (filled, read, pl.issued, pl.used)
    return filled, read


@pytest.mark.parametrize("plan,name", cc.RUNS, ids=["%s-%s" % r for r in cc.RUNS])
def test_invariants_hold_on_every_plan(plan, name):
    p = cc.BY_PLAN[plan]
    pl = cc.model(p, name)
    filled, read = check_invariants(pl)
    assert read == cc.N_ITER, (plan, read)
    runs = [(a, b) for op, a, b in p.calls if op == "run"]
    assert runs[0][0] == 0 and runs[-1][1] == cc.N_ITER
    assert all(a[1] == b[0] for a, b in zip(runs, runs[1:])), plan
    # the chunks tile the run, each inside its buffer
    spans = [c[3] for c in pl.chunks]
    assert spans[0][0] == 0 and spans[-1][1] == cc.N_ITER
    assert all(a[1] == b[0] for a, b in zip(spans, spans[1:])), plan
    for buf, vb, (f0, f1), (c0, c1) in pl.chunks:
        assert vb <= c0 <= f0 <= f1 == c1 <= vb + pl.vcap, (plan, buf, vb, f0, f1, c0, c1)
    if not plan.startswith("F-"):
        # the buffer is shorter than the run and the plan crosses its end
        assert pl.vcap == p.vcap < cc.N_ITER and pl.chunk() <= pl.vcap
        assert len({vb for _, vb, _, _ in pl.chunks}) >= 3, plan


def test_invariant_checker_sees_a_wrong_offset():
    """The checker is not vacuous: a planner that clamps a prefill one iteration too far, one
    whose prefill does not wait for the launch reading its buffer, and a step stream that does
    not wait for the prefill are each caught."""
    sh = cc.shape("reg")

    class Far(cc.Planner):
        def enqueue_prefill(self, a, b):
            self.vcap += 1
            try:
                super().enqueue_prefill(a, b)
            finally:
                self.vcap -= 1

    with pytest.raises(AssertionError):
        check_invariants(Far(sh, cc.N_ITER, 5).play(cc.C_CALLS))

    class NoWait(cc.Planner):
        def _fill(self, stream, buf, vb, a, b, wait="none"):
            super()._fill(stream, buf, vb, a, b)

    with pytest.raises(AssertionError):
        check_invariants(NoWait(sh, cc.N_ITER, 5).play(cc.ONE))
    pl = cc.Planner(sh, cc.N_ITER, 5).play(cc.ONE)
    pl.trace = [e for e in pl.trace if e["ev"] != "join"]
    with pytest.raises(AssertionError):
        check_invariants(pl)


def test_model_only_plans():
    """Reasons the GPU plans cannot reach without changing the trajectory, and replay."""
    sh = cc.shape("reg")
    # reason 1: a call that does not start where the launch's last call ended
    pl = cc.Planner(sh, cc.N_ITER, 8, resident=True).play([("run", 0, 3), ("run", 5, 8)])
    assert pl.refusals == [1] and pl.launches == 2 and pl.calls == 0
    assert pl.paths["prefill-unused"] == 1
    # replay: prefills within a call only, and never a resident launch
    pl = cc.Planner(sh, 10, cc.E_VCAP, resident=True, replay=True).play(
        [("run", 0, 5), ("run", 5, 10)])
    check_invariants(pl)
    assert (pl.issued, pl.used, pl.launches) == (4, 4, 0)
    assert [c[3] for c in pl.chunks] == [(0, 3), (3, 5), (5, 8), (8, 10)]
    assert [c[1] for c in pl.chunks] == [0, 3, 5, 8]
    # ... the golden case of tests/test_gpu_chunks.py's replay test
    from golden_cases import Case
    c = Case(cc.E_CASE)
    assert (c.n_iter, c.n_chains, len(c.sizes), c.pooling) == (cc.E_N_ITER, 3, 8, "partial")
    half = cc.E_N_ITER // 2
    pl = cc.Planner(cc.E_SHAPE, cc.E_N_ITER, cc.E_VCAP, replay=True).play(
        [("run", 0, half), ("run", half, cc.E_N_ITER)])
    check_invariants(pl)
    f = pl.figures()
    assert dict(prefill=f["prefill"], chunks=len(f["chunks"])) == cc.E_EXPECT
    # fill_chunk
    for vcap, li, want in ((5, 0, 5), (5, 3, 3), (5, 5, 5), (5, 8, 5), (1, 3, 1)):
        assert cc.Planner(sh, cc.N_ITER, vcap, li).chunk() == want
    # a buffer as long as the run: one chunk, nothing after the schedule's end
    pl = cc.Planner(sh, cc.N_ITER, 1 << 20).play(cc.ONE)
    assert pl.vcap == cc.N_ITER and pl.figures()["prefill"] == {"issued": 0, "used": 0}


def test_every_listed_path_is_reached():
    listed = set(cc.REACHED_BY)
    named = {ln.split()[0] for ln in cc.__doc__.split("The paths, by the names")[1].splitlines()
             if ln.startswith("  ") and not ln.startswith("   ")}
    named = {n for n in named if n != "refusal-N"} | {"refusal-%d" % k for k in (3, 4, 5, 6)}
    assert named == listed, named ^ listed
    taken = set()
    for p in cc.PLANS:
        taken |= {k for k, v in p.expect["paths"].items() if v > 0}
    assert taken == listed, taken ^ listed
    for path, plan in cc.REACHED_BY.items():
        assert cc.BY_PLAN[plan].expect["paths"].get(path, 0) > 0, (path, plan)
    # by the issue's own list: the paths of nmc_run never exercised before
    d1, d2 = cc.BY_PLAN["D1-resident"].expect, cc.BY_PLAN["D2-resident"].expect
    assert d1["refusals"] == [4, 3] and 5 in d2["refusals"]
    assert d1["paths"]["continued"] == 3 and d1["launches"] == 4
    # (the call refused for reason 4 starts a launch whose vbase is its own start)
    assert (0, 14, (14, 17), (14, 17)) in d1["chunks"]
    assert (1, 8, (12, 12), (10, 12)) in d1["chunks"]        # Dev.vbase = pf.vb = 8 < c0 = 10
    assert cc.BY_PLAN["D1-declined"].expect["launches"] == 0


def test_plans_run_the_cases_the_issue_names():
    at5 = cc.BY_PLAN["A-vcap5"].cases + cc.BY_PLAN["A-vcap5-takeover"].cases
    assert sorted(at5) == sorted(sc.NAMES) and len(sc.NAMES) == 15
    assert cc.BY_PLAN["A-vcap5-takeover"].launch_iters == 2
    for v in ("A-vcap1", "A-vcap2"):
        assert cc.BY_PLAN[v].cases == ("reg", "sweep", "launch")
    assert cc.BY_PLAN["B-launch3"].launch_iters == 3 < 5 < cc.BY_PLAN["B-launch8"].launch_iters
    assert cc.BY_PLAN["C-calls"].cases == ("reg", "sweep", "half", "launch")
    assert cc.BY_PLAN["C-calls"].calls == [("run", 0, 4), ("run", 4, 12), ("prefill", 12, 26),
                                           ("run", 12, 26)]
    assert cc.BY_PLAN["C-unused"].cases == cc.BY_PLAN["C-calls"].cases
    assert cc.BY_PLAN["D1-resident"].cases == sc.RESIDENT_CASES == ("reg", "half")
    assert not cc.shape("lds").res_form
    assert [p.vcap for p in cc.PLANS if p.name[0] in "AB"] == [5, 5, 5, 1, 2, 5, 5]
    assert 26 % 5 != 0
    # tuning on: a tuning iteration (5, 10) and the first recorded row (13) fall on, just
    # before and just after buffer ends of the vcap-5 plans (ends at 5, 10, 15; 9 | 12 | 17)
    assert cc.TUNE == dict(burn=13, thin=1, tune_interval=5)
    ends = {c[3][1] for c in cc.BY_PLAN["A-vcap5"].expect["chunks"]}
    assert {5, 10, 15} <= ends
    ends = {c[3][1] for c in cc.BY_PLAN["C-calls"].expect["chunks"]}
    assert {4, 9, 12} <= ends and 10 - 1 in ends and 12 + 1 == 13


@pytest.mark.parametrize("name", cc.F_CASES)
def test_reset_plans_reset(name):
    sh = cc.shape(name)
    assert (name in cc.SPLIT) == (sc.BY_NAME[name].split is None)
    for plan in ("F-launch3-" + name, "F-calls-" + name):
        p = cc.BY_PLAN[plan]
        pl = cc.model(p, name)
        assert 1 <= p.wrap < cc.WRAP_DEFAULT
        assert pl.resets >= 3, (plan, pl.resets)
        # which launches reset: not the first, not all, and one without a reset between two
        marks, pending = [], False
        for e in pl.trace:
            if e["ev"] == "reset":
                pending = True
            elif e["ev"] == "launch":
                marks.append(pending)
                pending = False
        assert not marks[0] and sum(marks) == pl.resets, (plan, marks)
        first, last = marks.index(True), len(marks) - 1 - marks[::-1].index(True)
        assert False in marks[first:last], (plan, marks)
    # the split cases reset on the arrivals (S * xbase), the others on the publishes
    pl = cc.Planner(sh, cc.N_ITER, cc.N_ITER, 3, wrap=cc.F_WRAP[name])
    pl.run(0, 3)
    pl.run(3, 6)
    by_x = sh.S * (pl.xbase + 3 * sh.P) >= pl.wrap
    by_p = sh.G * (pl.pbase + 3) >= pl.wrap
    assert (by_x, by_p) == ((True, False) if name in cc.SPLIT else (False, True)), name
    if name == "complete-split":
        assert not sh.partial and pl.pbase == 0      # no publishes without a Gibbs update


def test_resident_reset_plan():
    p = cc.BY_PLAN["F-resident"]
    assert p.expect["refusals"] == [6] * 4 and p.expect["launches"] == 5
    assert p.expect["resets"] == 4
    # the default limit: one launch, eight continued calls, no reset
    pl = cc.Planner(cc.shape("reg"), cc.N_ITER, cc.N_ITER, resident=True).play(cc.F_RES_CALLS)
    assert (pl.launches, pl.calls, pl.resets, pl.refusals) == (1, 8, 0, [])


def test_variate_bytes_gives_the_vcap():
    for name in sc.NAMES:
        sh = cc.shape(name)
        per = cc.per_iter_bytes(sh)
        assert per == (2 * sh.P * sh.G * sh.C + 2 * sh.P * sh.C) * 8
        for vcap in (1, 2, 3, 5, 8, 25):
            lo, hi = cc.variate_bytes(sh, vcap), cc.variate_bytes(sh, vcap, slack=True)
            assert hi - lo == per - 1
            assert cc.vcap_of(sh, cc.N_ITER, lo) == cc.vcap_of(sh, cc.N_ITER, hi) == vcap
            assert cc.vcap_of(sh, cc.N_ITER, lo - 1) == max(vcap - 1, 1)
            assert cc.vcap_of(sh, cc.N_ITER, hi + 1) == vcap + 1
        assert cc.vcap_of(sh, cc.N_ITER, None) == cc.N_ITER       # 1 GiB: the whole run
        assert cc.vcap_of(sh, cc.N_ITER, 0) == cc.vcap_of(sh, cc.N_ITER, 1) == 1
    assert cc.schedule_env("A-vcap5", "reg") == {"NMC_VARIATE_BYTES": str(5 * 13440)}
    assert cc.schedule_env("A-vcap5-floor", "reg") == {"NMC_VARIATE_BYTES": str(6 * 13440 - 1)}
    assert cc.schedule_env("F-calls-reg", "reg") == {}
