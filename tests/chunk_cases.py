"""Cases of tests/test_chunk_cases.py (CPU) and tests/test_gpu_chunks.py (GPU): nmc_run with
variate buffers shorter than the run, and with the reset of the launch-spanning counters.

csrc/nestmc.hip draws a chunk's variates into one of two buffers of ``vcap`` iterations and
every kernel reads them at ``(t - vbase)``.  In every other test vcap == n_iter, so nothing
that depends on where a buffer ends ever runs.  Here NMC_VARIATE_BYTES makes vcap 1, 2, 3, 5
or 8 on the 26 iterations of schedule_cases' cases, and nmc_debug_set_counter_wrap makes the
counter reset run every few launches.

``Planner`` restates the host planner in plain Python -- fill_chunk, nmc_run's chunk loop,
enqueue_prefill, res_prefill, res_continue's reasons 1, 3, 4, 5 and 6, nmc_prefill and the wrap
test -- and yields for a plan the chunks (buffer, vbase, filled range, launch range), the
prefill and resident statistics, the refusal reasons in order, the counter resets and the
named paths the plan took.  PLANS holds the plans with all those figures WRITTEN OUT; the CPU
test holds the literals to the model and the model's trace to the invariants the design rests
on; the GPU test holds the library to the literals and the results to a run that never meets
a buffer end, bit for bit.

The paths, by the names the literals use (``paths`` of a plan: name -> times taken):
  ragged-chunk          the last chunk of a call is shorter than the others
  chunk-capped          launch_iters above vcap: the buffer caps the chunk
  fill-at-offset        launch_fill writing at a - vb > 0 (the rest of a taken prefill)
  prefill-clamped       enqueue_prefill's b = min(b, a + vcap) binding
  take                  a chunk starting where the pending prefill starts takes it
  take-at-offset        ... a parked resident launch's, at its offset (Dev.vbase = pf.vb < c0)
  take-past-buffer      ... refused: c1 - pf.vb > vcap, the chunk fills its own buffer
  prefill-unused        a pending prefill no chunk starts at: dropped
  prefill-replaced      a pending prefill replaced by a later one before any chunk
  continued             a resident call handed to the running launch
  refusal-N             res_continue's reason N
  next-clamped          res_continue's next-call prefill cut at vbase + vcap
  next-cancelled        ... cut to nothing
  res-prefill-clamped   res_prefill's own b = min(b, vbase + vcap) binding (a fresh launch)
  res-prefill-cancelled res_prefill's b <= a return
  prefill-into-launch   nmc_prefill into the resident launch's buffer
  prefill-parks         nmc_prefill past the launch's buffer: parks it
  reset                 the counters zeroed before a launch
This module imports no GPU code.
"""

import collections

import schedule_cases as sc

N_ITER = sc.N_ITER
TUNE = dict(burn=sc.TUNE_BURN, thin=1, tune_interval=sc.TUNE_ON)   # tunes at 5 and 10
WRAP_DEFAULT = 1 << 31
GET_STATE = ("get_state", 0, 0)

# members of the row split (csrc/nestmc.hip nmc_create: ceil(rows / 4096) above 2 * 4096 rows)
SPLIT = {"partial-split": 3, "complete-split": 3}

Shape = collections.namedtuple("Shape", "G P C S partial persistent res_form")


def shape(name):
    c = sc.BY_NAME[name]
    return Shape(len(c.sizes), c.P, c.C, SPLIT.get(name, 1), c.model.endswith("-partial"),
                 c.persistent, name in sc.RESIDENT_CASES)


def per_iter_bytes(sh):
    """nmc_set_schedule's bytes of variates per iteration: {z, log u} [P][G][C] and the two
    hyper variates [P][C], doubles."""
    return (2 * sh.P * sh.G * sh.C + 2 * sh.P * sh.C) * 8


def variate_bytes(sh, vcap, slack=False):
    """NMC_VARIATE_BYTES for a buffer of vcap iterations; slack: the most that still floors
    to vcap."""
    return vcap * per_iter_bytes(sh) + (per_iter_bytes(sh) - 1 if slack else 0)


def vcap_of(sh, n_iter, nbytes):
    """nmc_set_schedule's vcap for a budget of nbytes >= 0 (None: the 1 GiB default): floored,
    then clamped to 1 .. n_iter."""
    budget = (1 << 30) if nbytes is None else int(nbytes)
    assert budget >= 0
    return max(1, min(budget // per_iter_bytes(sh), n_iter if n_iter > 0 else 1))


class Planner:
    """The host planner of csrc/nestmc.hip, restated.  trace: the events in the order the host
    issues them --
      fill    stream ("main" | "pre"), buf, vb, a, b; wait: the index of the launch whose rd_ev
              a "pre" fill waits for (None: no launch has read buf; "none": it does not wait)
      launch  buf, vb, c0, c1, resident
      call    a continued resident call: buf, vb, c0, c1
      join    the main stream (or the host) waits for the prefill stream
      park    the resident launch ends
      reset   the counters are zeroed on the main stream
    """

    def __init__(self, sh, n_iter, vcap, launch_iters=0, resident=False, wrap=WRAP_DEFAULT,
                 replay=False):
        self.sh, self.n_iter, self.launch_iters, self.wrap = sh, n_iter, launch_iters, wrap
        self.vcap = max(1, min(vcap, n_iter if n_iter > 0 else 1))
        self.replay = replay
        self.vbuf, self.pf = 1, None
        self.issued = self.used = 0
        self.pbase = self.xbase = 0
        self.resets = 0
        self.res_on = bool(resident and sh.res_form and not replay)
        self.active, self.r_end, self.r_buf, self.r_vbase = False, 0, 0, 0
        self.launches = self.calls = 0
        self.why = 0
        self.refusals = []
        self.trace, self.chunks = [], []
        self.paths = collections.Counter()
        self.rd = [None, None]

    # -- helpers ----------------------------------------------------------------------------
    def chunk(self):
        li = self.launch_iters
        return li if 0 < li < self.vcap else self.vcap

    def _ev(self, ev, **kw):
        self.trace.append(dict(ev=ev, **kw))
        return len(self.trace) - 1

    def _fill(self, stream, buf, vb, a, b, wait="none"):
        if a - vb > 0 and stream == "main":
            self.paths["fill-at-offset"] += 1
        self._ev("fill", stream=stream, buf=buf, vb=vb, a=a, b=b, wait=wait)

    def _wraps(self, n):
        sh = self.sh
        return (sh.G * (self.pbase + n) >= self.wrap or
                sh.S * (self.xbase + n * sh.P) >= self.wrap)

    def _drop(self, how):
        if self.pf is not None:
            self.paths[how] += 1

    def park(self):
        if self.active:
            self.active = False
            self._ev("park")

    # -- nestmc.hip ---------------------------------------------------------------------------
    def enqueue_prefill(self, a, b):
        if b > a + self.vcap:
            b = a + self.vcap
            self.paths["prefill-clamped"] += 1
        buf = self.vbuf ^ 1
        self._fill("pre", buf, a, a, b, wait=self.rd[buf])
        self._drop("prefill-replaced")
        self.pf = dict(i0=a, i1=b, buf=buf, vb=a)
        self.issued += b - a

    def res_prefill(self, a, b):
        if b > self.r_vbase + self.vcap:
            b = self.r_vbase + self.vcap
            self.paths["res-prefill-clamped" if b > a else "res-prefill-cancelled"] += 1
        if b <= a:
            return
        self._fill("pre", self.r_buf, self.r_vbase, a, b)
        self._drop("prefill-replaced")
        self.pf = dict(i0=a, i1=b, buf=self.r_buf, vb=self.r_vbase)
        self.issued += b - a

    def res_continue(self, i0, i1):
        pf = self.pf
        why = (1 if i0 != self.r_end else
               3 if i1 - i0 > self.chunk() else
               4 if i1 - self.r_vbase > self.vcap else
               5 if not (pf and pf["buf"] == self.r_buf and pf["i0"] == i0 and pf["i1"] >= i1)
               else 6 if self._wraps(i1 - i0) else 0)
        if why:
            self.why = why
            self.refusals.append(why)
            self.paths["refusal-%d" % why] += 1
            self.park()
            return False
        self._ev("join")
        self._ev("call", buf=self.r_buf, vb=self.r_vbase, c0=i0, c1=i1)
        self.chunks.append((self.r_buf, self.r_vbase, (i1, i1), (i0, i1)))
        self.paths["continued"] += 1
        self.used += i1 - i0
        self.pf = None
        self.r_end = i1
        self.calls += 1
        self.pbase += i1 - i0
        self.xbase += (i1 - i0) * self.sh.P
        free = min(i1 + (i1 - i0), self.n_iter)
        n1 = min(free, self.r_vbase + self.vcap)
        if n1 < free:
            self.paths["next-clamped" if n1 > i1 else "next-cancelled"] += 1
        if n1 > i1:
            self.res_prefill(i1, n1)
        return True

    def run(self, i0, i1):
        assert 0 <= i0 <= i1
        if i0 == i1:
            return
        if self.active and self.res_continue(i0, i1):
            return
        sh, chunk = self.sh, self.chunk()
        if self.launch_iters > self.vcap:
            self.paths["chunk-capped"] += 1
        for c0 in range(i0, i1, chunk):
            c1 = min(c0 + chunk, i1)
            if c1 - c0 < chunk and c0 > i0:
                self.paths["ragged-chunk"] += 1
            buf, have, vb = self.vbuf ^ 1, c0, c0
            if self.pf is not None:
                pf = self.pf
                self._ev("join")
                if pf["i0"] == c0 and c1 - pf["vb"] <= self.vcap:
                    buf, vb, have = pf["buf"], pf["vb"], min(c1, pf["i1"])
                    self.used += have - c0
                    self.paths["take-at-offset" if vb < c0 else "take"] += 1
                elif pf["i0"] == c0:
                    self.paths["take-past-buffer"] += 1
                else:
                    self.paths["prefill-unused"] += 1
                self.pf = None
            self.vbuf = buf
            if have < c1:
                self._fill("main", buf, vb, have, c1)
            n0 = c1
            n1 = (min(c1 + chunk, i1) if c1 < i1
                  else min(c1 + (i1 - i0), c1 + chunk, self.n_iter))
            if self.replay and c1 == i1:
                n1 = n0
            if self._wraps(c1 - c0):
                self._ev("reset")
                self.pbase = self.xbase = 0
                self.resets += 1
                self.paths["reset"] += 1
            steps = (c1 - c0) * sh.P
            resl = self.res_on and c0 == i0 and c1 == i1 and (not sh.partial or sh.persistent)
            at = self._ev("launch", buf=buf, vb=vb, c0=c0, c1=c1, resident=resl)
            self.chunks.append((buf, vb, (have, c1), (c0, c1)))
            if resl:
                self.active, self.r_end, self.r_buf, self.r_vbase = True, c1, buf, vb
                self.launches += 1
                self.pbase += c1 - c0
                self.xbase += steps
            elif not sh.partial:
                self.xbase += steps
            elif sh.persistent:
                self.pbase += c1 - c0
                self.xbase += steps
            self.rd[buf] = at
            if n1 > n0:
                if resl:
                    self.res_prefill(n0, n1)
                else:
                    self.enqueue_prefill(n0, n1)

    def prefill(self, i0, i1):
        assert 0 <= i0 <= i1 <= self.n_iter
        if i0 == i1:
            return
        if self.active:
            if i0 == self.r_end and i1 - self.r_vbase <= self.vcap:
                self.paths["prefill-into-launch"] += 1
                return self.res_prefill(i0, i1)
            self.paths["prefill-parks"] += 1
            self.park()
        self.enqueue_prefill(i0, i1)

    def play(self, calls):
        for op, a, b in calls:
            if op == "run":
                self.run(a, b)
            elif op == "prefill":
                self.prefill(a, b)
            elif op == "get_state":
                self.park()
            else:
                assert op == "synchronize", op
        return self

    def figures(self):
        """What the literals of a plan hold."""
        return dict(prefill={"issued": self.issued, "used": self.used},
                    launches=self.launches, calls=self.calls, refusals=list(self.refusals),
                    last_refusal=self.why, resets=self.resets,
                    paths=dict(sorted(self.paths.items())), chunks=list(self.chunks))


# ---------------------------------------------------------------------------------------------
# The plans.  A plan: what is set (vcap through NMC_VARIATE_BYTES, launch_iters, resident,
# wrap) , the calls, the cases it runs on, and the model's figures written out -- ``chunks``
# as (buffer, vbase, filled range, launch range) where ``chunks`` is given, else their number;
# the filled range is what the chunk's own fill drew, (c1, c1) where a prefill held it all.
# Figures that depend on the case's shape (the resets of F) are keyed by case.
# ---------------------------------------------------------------------------------------------
Plan = collections.namedtuple(
    "Plan", "name cases vcap launch_iters resident wrap calls expect slack")


def _plan(name, cases, vcap, calls, expect, launch_iters=0, resident=False, wrap=None,
          slack=False):
    return Plan(name, tuple(cases), vcap, launch_iters, resident, wrap, calls, expect, slack)


ONE = [("run", 0, N_ITER)]
A_SMALL = ("reg", "sweep", "launch")
B_CASES = ("reg", "sweep")
C_CASES = ("reg", "sweep", "half", "launch")
D_CASES = sc.RESIDENT_CASES + ("lds",)      # lds has no resident form: the request is void
F_CASES = ("reg", "lds", "sweep", "sweep-gsep", "sweep-off-1", "partial-split",
           "complete-split")

# C: calls across buffer ends at vcap 5
C_CALLS = [("run", 0, 4),            # prefills [4, 8)
           ("run", 4, 12),           # takes [4, 8) into its chunk [4, 9), draws 8; chunk [9, 12)
           ("prefill", 12, 26),      # replaces nmc_run's own [12, 17); clamped to [12, 17)
           ("run", 12, 26)]          # chunk [12, 17) takes it; [17, 22), [22, 26)
# ... a prefill that no chunk starts at, which nmc_run replaces by its own
C2_CALLS = [("run", 0, 7),           # chunks [0, 5), [5, 7); prefills [7, 12)
            ("prefill", 9, 12),      # replaces it
            ("run", 7, 19),          # no chunk starts at 9: fills its own [7, 12); [12, 17), [17, 19)
            ("prefill", 19, 26),     # replaces nmc_run's own [19, 24); clamped to [19, 24)
            ("run", 19, 26)]

# D: resident, vcap 8 (the walk-through: the comments of test_chunk_cases.test_plan_d)
D1_CALLS = [("run", 0, 3), ("run", 3, 6), ("run", 6, 8), ("prefill", 8, 10), ("run", 8, 10),
            GET_STATE, ("run", 10, 12), ("run", 12, 14), ("run", 14, 17), ("run", 17, 26)]
D2_CALLS = [("run", 0, 8), ("run", 8, 13), ("run", 13, 16), ("run", 16, 18),
            ("prefill", 18, 19), ("run", 18, 20), ("run", 20, 26)]

# F: counter resets.  One call in launches of 3, and calls of 4 | 5 | 1 | 8 | 8
F_CALLS = [("run", 0, 4), ("run", 4, 9), ("run", 9, 10), ("run", 10, 18), ("run", 18, N_ITER)]
F_RES_CALLS = [("run", k, min(k + 3, N_ITER)) for k in range(0, N_ITER, 3)]
# the limit per case: G * (iterations since the reset) or S * (steps since the reset) reaches
# it within three launches of 3
F_WRAP = {"reg": 40, "lds": 70 * 8, "sweep": 129 * 8, "sweep-gsep": 129 * 8,
          "sweep-off-1": 129 * 8, "partial-split": 40, "complete-split": 70}

_NO_RES = dict(launches=0, calls=0, refusals=[], last_refusal=0, resets=0)


def _exp(issued, used, chunks, paths, **kw):
    return dict(dict(_NO_RES, prefill={"issued": issued, "used": used}, chunks=chunks,
                     paths=paths), **kw)


PLANS = [
    # -- A: one call, the buffer shorter than the run ------------------------------------------
    _plan("A-vcap5", [n for n in sc.NAMES if n != "sweep-takeover"], 5, ONE, _exp(21, 21, [
        (0, 0, (0, 5), (0, 5)), (1, 5, (10, 10), (5, 10)), (0, 10, (15, 15), (10, 15)),
        (1, 15, (20, 20), (15, 20)), (0, 20, (25, 25), (20, 25)), (1, 25, (26, 26), (25, 26))],
        {"ragged-chunk": 1, "take": 5})),
    # (sweep-takeover is a case of launches of 2: two or three launches per buffer)
    _plan("A-vcap5-takeover", ("sweep-takeover",), 5, ONE, _exp(24, 24, 13, {"take": 12}),
          launch_iters=sc.BY_NAME["sweep-takeover"].launch_iters),
    _plan("A-vcap5-floor", ("reg",), 5, ONE, _exp(21, 21, 6, {"ragged-chunk": 1, "take": 5}),
          slack=True),
    _plan("A-vcap1", A_SMALL, 1, ONE, _exp(25, 25, 26, {"take": 25})),
    _plan("A-vcap2", A_SMALL, 2, ONE, _exp(24, 24, 13, {"take": 12})),
    # -- B: launch_iters below and above the buffer --------------------------------------------
    _plan("B-launch3", B_CASES, 5, ONE, _exp(23, 23, 9, {"ragged-chunk": 1, "take": 8}),
          launch_iters=3),
    _plan("B-launch8", B_CASES, 5, ONE, _exp(21, 21, 6, {"chunk-capped": 1, "ragged-chunk": 1,
                                                         "take": 5}), launch_iters=8),
    # -- C: calls across buffer ends -----------------------------------------------------------
    _plan("C-calls", C_CASES, 5, C_CALLS, _exp(26, 21, [
        (0, 0, (0, 4), (0, 4)),
        (1, 4, (8, 9), (4, 9)),            # took [4, 8), drew 8 at offset 4
        (0, 9, (12, 12), (9, 12)),
        (1, 12, (17, 17), (12, 17)),       # the explicit prefill, clamped to 17
        (0, 17, (22, 22), (17, 22)),
        (1, 22, (26, 26), (22, 26))],
        {"fill-at-offset": 1, "prefill-clamped": 1, "prefill-replaced": 1, "ragged-chunk": 2,
         "take": 5})),
    _plan("C-unused", C_CASES, 5, C2_CALLS, _exp(29, 16, [
        (0, 0, (0, 5), (0, 5)),
        (1, 5, (7, 7), (5, 7)),
        (0, 7, (7, 12), (7, 12)),          # the prefill of [9, 12) dropped
        (1, 12, (17, 17), (12, 17)),
        (0, 17, (19, 19), (17, 19)),
        (1, 19, (24, 24), (19, 24)),       # the explicit prefill, clamped to 24
        (0, 24, (26, 26), (24, 26))],
        {"prefill-clamped": 1, "prefill-replaced": 2, "prefill-unused": 1, "ragged-chunk": 3,
         "take": 5})),
    # -- D: resident, vcap 8 -------------------------------------------------------------------
    _plan("D1-resident", sc.RESIDENT_CASES, 8, D1_CALLS, _exp(17, 12, [
        (0, 0, (0, 3), (0, 3)),            # launch 1, vbase 0
        (0, 0, (6, 6), (3, 6)),            # continued; the next prefill cut to [6, 8)
        (0, 0, (8, 8), (6, 8)),            # continued to the buffer's end; next: nothing
        (1, 8, (10, 10), (8, 10)),         # prefill(8, 10) parked it; launch 2, vbase 8
        (1, 8, (12, 12), (10, 12)),        # after the state read: launch 3 at offset 2
        (1, 8, (14, 14), (12, 14)),        # continued
        (0, 14, (14, 17), (14, 17)),       # reason 4; [14, 16) at vbase 8 not usable: launch 4
        (1, 17, (17, 25), (17, 25)),       # reason 3; [17, 20) at vbase 14 not usable
        (0, 25, (26, 26), (25, 26))],
        {"continued": 3, "next-cancelled": 1, "next-clamped": 1, "prefill-parks": 1,
         "ragged-chunk": 1, "refusal-3": 1, "refusal-4": 1, "take": 2, "take-at-offset": 1,
         "take-past-buffer": 2},
        launches=4, calls=3, refusals=[4, 3], last_refusal=3), resident=True),
    _plan("D2-resident", sc.RESIDENT_CASES, 8, D2_CALLS, _exp(8, 4, [
        (0, 0, (0, 8), (0, 8)),            # a whole buffer: its next prefill cancelled
        (1, 8, (8, 13), (8, 13)),          # reason 4; launch 2; its prefill cut to [13, 16)
        (1, 8, (16, 16), (13, 16)),        # continued to the buffer's end
        (0, 16, (16, 18), (16, 18)),       # reason 4; launch 3; prefills [18, 20)
        (0, 16, (19, 20), (18, 20)),       # prefill(18, 19) replaced it: reason 5; launch 4
        (1, 20, (20, 26), (20, 26))],      # reason 4; [20, 22) at vbase 16 not usable
        {"continued": 1, "fill-at-offset": 1, "next-cancelled": 1, "prefill-into-launch": 1,
         "prefill-replaced": 1, "refusal-4": 3, "refusal-5": 1, "res-prefill-cancelled": 1,
         "res-prefill-clamped": 1, "take-at-offset": 1, "take-past-buffer": 1},
        launches=5, calls=1, refusals=[4, 4, 5, 4], last_refusal=4), resident=True),
    # (no resident form: the same calls on separate launches)
    _plan("D1-declined", ("lds",), 8, D1_CALLS, _exp(20, 17, 9,
          {"fill-at-offset": 2, "prefill-replaced": 1, "ragged-chunk": 1, "take": 8}),
          resident=True),
]

# -- F: the reset, per case (the limit differs with the shape) ---------------------------------
# resets of the one call in launches of 3 (9 launches) and of F_CALLS (5 launches)
F_RESETS = {"reg": (4, 3), "lds": (4, 3), "sweep": (4, 3), "sweep-gsep": (4, 3),
            "sweep-off-1": (4, 3), "partial-split": (4, 3), "complete-split": (4, 3)}
for _n in F_CASES:
    PLANS.append(_plan("F-launch3-" + _n, (_n,), N_ITER, ONE,
                       _exp(23, 23, 9, {"ragged-chunk": 1, "reset": F_RESETS[_n][0], "take": 8},
                            resets=F_RESETS[_n][0]), launch_iters=3, wrap=F_WRAP[_n]))
    PLANS.append(_plan("F-calls-" + _n, (_n,), N_ITER, F_CALLS,
                       _exp(18, 14, 5, {"fill-at-offset": 2, "reset": F_RESETS[_n][1], "take": 4},
                            resets=F_RESETS[_n][1]), wrap=F_WRAP[_n]))
PLANS.append(_plan("F-resident", ("reg",), N_ITER, F_RES_CALLS, _exp(
    23, 23, 9, {"continued": 4, "refusal-6": 4, "reset": 4, "take-at-offset": 4},
    launches=5, calls=4, refusals=[6, 6, 6, 6], last_refusal=6, resets=4),
    resident=True, wrap=F_WRAP["reg"]))
# (launches of a fixed length are never resident: the request changes nothing)
PLANS.append(_plan("F-resident-launch3", ("reg",), N_ITER, ONE, _exp(
    23, 23, 9, {"ragged-chunk": 1, "reset": 4, "take": 8}, resets=4),
    launch_iters=3, resident=True, wrap=F_WRAP["reg"]))

BY_PLAN = {p.name: p for p in PLANS}
RUNS = [(p.name, n) for p in PLANS for n in p.cases]

# E: the golden case linreg_partial (400 iterations, 8 groups, 3 chains), its variates
# replayed, in two calls of 200 at vcap 3: 2 * 67 launches, each but a call's last prefilling
# the next (replayed variates are prefilled within a call only)
E_VCAP = 3
E_CASE, E_N_ITER, E_SHAPE = "linreg_partial", 400, Shape(8, 2, 3, 1, True, True, False)
E_EXPECT = dict(prefill={"issued": 394, "used": 394}, chunks=134)

# every path the issue lists, and the plan whose literals show it taken
REACHED_BY = {
    "ragged-chunk": "A-vcap5", "chunk-capped": "B-launch8", "fill-at-offset": "C-calls",
    "prefill-clamped": "C-calls", "take": "A-vcap5", "take-at-offset": "D1-resident",
    "take-past-buffer": "D1-resident", "prefill-unused": "C-unused",
    "prefill-replaced": "C-calls", "continued": "D1-resident", "refusal-3": "D1-resident",
    "refusal-4": "D1-resident", "refusal-5": "D2-resident", "refusal-6": "F-resident",
    "next-clamped": "D1-resident", "next-cancelled": "D1-resident",
    "res-prefill-clamped": "D2-resident", "res-prefill-cancelled": "D2-resident",
    "prefill-into-launch": "D2-resident", "prefill-parks": "D1-resident",
    "reset": "F-launch3-reg",
}

# NMC_VARIATE_BYTES values that mean nothing: vcap >= 1 and the baseline's bits (case reg)
ODD_BYTES = ["0", "1", "-4096", "plenty"]


def model(plan, name):
    p = BY_PLAN[plan] if isinstance(plan, str) else plan
    return Planner(shape(name), N_ITER, p.vcap, p.launch_iters, p.resident,
                   p.wrap or WRAP_DEFAULT).play(p.calls)


def schedule_env(plan, name):
    p = BY_PLAN[plan] if isinstance(plan, str) else plan
    if p.vcap >= N_ITER:
        return {}
    return {"NMC_VARIATE_BYTES": str(variate_bytes(shape(name), p.vcap, p.slack))}
