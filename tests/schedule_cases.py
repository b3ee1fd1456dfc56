"""Cases of tests/test_schedule_cases.py (CPU) and tests/test_gpu_schedule.py (GPU): which
iteration lands in which row of the device sample store (csrc/dev.h nmc_record_row), on
every kernel that writes the store.

nmc_record_row has two paths, ``thin == 1`` and the thinned one, and six callers:

  step.h        store_pending             group values of nmc_k_run
  gibbs.h       nmc_hyper                 launch per iteration; nmc_k_run persistent over
                                          more than 128 groups, in its loop and closing a call
  gibbs.h       nmc_hyper_compute         the LDS payload, 65..128 groups (loop and closing)
  gibbs.h       nmc_hyper_finish          the register hand-off (loop and closing); the
                                          sweep's take-over
  sweep.h                                 group values of nmc_k_sweep
  sweep_gibbs.h                           the Gibbs workgroups of nmc_k_sweep

CASES holds one case per recording path at the smallest shape that takes it, SCHEDULES the
(burn, thin) pairs with the iterations each records (written out here, asserted against
nestmc.sampler.record_iterations by the CPU test), PLANS the call plans that put a call
boundary between, on and just after a recorded iteration.

The identity the GPU test asserts: tuning happens at ``t < burn and t % tune_interval == 0``
alone, so with a tune interval above n_iter the trajectory depends on neither burn nor thin,
and a run under (burn, thin) must store rows record_iterations(n_iter, burn, thin) of the
baseline (burn 0, thin 1: every iteration) bit for bit, hyper columns included.

Shapes that differ from a literal reading of "the smallest":
  partial-split  three groups of 8193 rows: a {x, y} row table splits above 2 * 4096 rows per
                 group (csrc/nestmc.hip nmc_create), into ceil(8193 / 4096) = 3 members; three
                 groups, not two, keep the inverse-gamma shape (G - 1) / 2 at 1.
  sweep-off      NMC_SWEEP=0 over 129 groups and two chain blocks is 258 workgroups, more
                 than nmc_k_run keeps resident on 256 CUs: the engine launches it per
                 iteration (NMC_MODE_LAUNCH, asserted), the path of case "launch".  Case
                 sweep-off-1 is the same model on one chain block of 64 chains: nmc_k_run
                 persistent over more than 128 groups (NMC_MODE_SYNC), whose Gibbs update is
                 nmc_hyper inside the step loop.
The two split cases run N_ITER iterations like every other case (measured times: DESIGN.md,
"What the recording schedule is tested on").

This module imports no GPU code: families are built, never compiled or run.
"""

import collections
import functools
import zlib

import numpy

import decision_cases as dc
import user_models
from gpu_cases import run_oracle_state, synthetic
from nestmc.families import DeviceLikelihood, LinearRegression
from oracle import restatement as rs
from rowpath_cases import FastNested

N_ITER = 26
TUNE_OFF = 100                 # above N_ITER: no tuning, the trajectory ignores burn
TUNE_ON, TUNE_BURN = 5, 13     # tunes at iterations 5 and 10
SEED, BASE = 20261, 5          # Philox seed, global id of chain 0
# a quiet NaN no arithmetic produces: the store is filled with it before a run
SENTINEL = numpy.uint64(0x7FF85CED0123ABCD)

# (burn, thin): the iterations recorded
SCHEDULES = collections.OrderedDict([
    ((0, 3), [0, 3, 6, 9, 12, 15, 18, 21, 24]),   # iteration 0 on the thinned path
    ((6, 3), [6, 9, 12, 15, 18, 21, 24]),         # burn a multiple of thin: first == burn
    ((7, 3), [9, 12, 15, 18, 21, 24]),            # burn no multiple of thin
    ((13, 3), [15, 18, 21, 24]),                  # schedule(26, 5): four rows for five samples
    ((25, 5), [25]),                              # one row, the last iteration
    ((23, 2), [24]),                              # one row, the last iteration not recorded
    ((0, 50), [0]),                               # one row, thin > n_iter
    ((10, 50), []),                               # no rows
    ((26, 1), []),                                # no rows on the fast path
    ((13, 1), list(range(13, 26))),               # the fast path with burn > 0
])
CORE = [(0, 3), (7, 3), (13, 3), (25, 5)]         # what every case runs
ORACLE_SCHEDULE = PLAN_SCHEDULE = (7, 3)          # 9 and 12 are recorded

# call plans under PLAN_SCHEDULE: (launch_iters, calls).  CONTINUED: the plans whose resident
# calls continue a launch (launches of a fixed length are never resident, and a state read
# parks the launch)
CONTINUED = ("9-alone", "close-on-recorded")
PLANS = collections.OrderedDict([
    ("launches-of-3", (3, [("run", 0, N_ITER)])),
    # the first call's closing Gibbs update is iteration 8 (not recorded); the second call is
    # the recorded iteration 9 alone
    ("9-alone", (0, [("run", 0, 9), ("run", 9, 10), ("run", 10, N_ITER)])),
    # a closing update of a recorded iteration (9, then 12), then a boundary just after one
    ("close-on-recorded", (0, [("run", 0, 10), ("run", 10, 12), ("run", 12, 13),
                               ("run", 13, N_ITER)])),
    ("boundary-at-burn", (0, [("run", 0, 7), ("get_state", 0, 0), ("run", 7, N_ITER)])),
])
PLAN_CASES = ("reg", "lds", "sweep", "p4", "half")
# The plan cases with a resident instance of their kernel (csrc/fam_ops.h nmc_run_kernel_res:
# NMC_MODE_SYNC_REG, NMC_MODE_HALF and NMC_MODE_NOPOOL of families of at most three fields):
# their resident plans must run in a resident launch.  The others have none -- lds runs
# NMC_MODE_SYNC_LDS, p4 FamLogistic<4> (four fields), and nmc_set_resident leaves the sweep
# alone -- so set_resident must leave them on separate launches: their "resident" plans hold
# that the request changes nothing, and fail when one of them gains a resident instance.
RESIDENT_CASES = ("reg", "half")
TUNE_CASES = ("reg", "sweep")


def resident_calls(calls):
    """The plan for a resident engine: each continuing run's variates prefilled, so that the
    call continues the launch (tests/test_gpu_restart_lds.py)."""
    out = []
    for op, a, b in calls:
        if op == "run" and a > 0:
            out.append(("prefill", a, b))
        out.append((op, a, b))
    return out


# kernel: prefix of launch_config()["kernel"]; modes: the modes accepted; split: members
# (None: more than one); fallbacks: gibbs_fallbacks expected (None: not a sweep case);
# sites: the callers of nmc_record_row the case reaches (DESIGN.md holds the same table)
Case = collections.namedtuple(
    "Case", "name model sizes C env launch_iters kernel modes persistent cpb split fallbacks "
            "P scale sites")

_RAG70 = dc._ragged(70, 16, 70)
_RAG129 = dc._ragged(129, 8, 129)
_SWEEP = dict(model="linreg-partial", sizes=_RAG129, C=70, launch_iters=0, persistent=True,
              cpb=64, split=1, P=2, scale=0.5)
_TAKEOVER = {"NMC_GSEP": "1", "NMC_GSEP_SERIAL": "1", "NMC_GSEP_PATIENCE_US": "500"}

CASES = [
    Case("reg", "linreg-partial", [12, 0, 7, 1, 23], 70, {}, 0, "nmc_k_run<FamLinreg<2>, ",
         ("NMC_MODE_SYNC_REG",), True, 64, 1, None, 2, 0.3,
         ("store_pending", "nmc_hyper_finish")),
    Case("lds", "linreg-partial", _RAG70, 70, {}, 0, "nmc_k_run<FamLinreg<2>, ",
         ("NMC_MODE_SYNC_LDS",), True, 64, 1, None, 2, 0.5,
         ("store_pending", "nmc_hyper_compute")),
    Case(name="sweep", env={}, kernel="nmc_k_sweep<FamLinreg<2>, ", modes=("NMC_MODE_SYNC_OWN",),
         fallbacks=0, sites=("sweep.h", "sweep_gibbs.h"), **_SWEEP),
    Case(name="sweep-gsep", env={"NMC_GSEP": "1"}, kernel="nmc_k_sweep<FamLinreg<2>, ",
         modes=("NMC_MODE_SYNC_OWN",), fallbacks=0,
         sites=("sweep.h", "sweep_gibbs.h"), **_SWEEP),
    Case(name="sweep-takeover", env=_TAKEOVER, kernel="nmc_k_sweep<FamLinreg<2>, ",
         modes=("NMC_MODE_SYNC_OWN",), fallbacks="all",
         sites=("sweep.h", "nmc_hyper_finish"),
         **dict(_SWEEP, launch_iters=2)),
    # (module docstring: two chain blocks of 129 workgroups are launched per iteration)
    Case(name="sweep-off", env={"NMC_SWEEP": "0"}, kernel="nmc_k_run<FamLinreg<2>, ",
         modes=("NMC_MODE_LAUNCH",), fallbacks=None, sites=("store_pending", "nmc_hyper"),
         **dict(_SWEEP, persistent=False)),
    Case(name="sweep-off-1", env={"NMC_SWEEP": "0"}, kernel="nmc_k_run<FamLinreg<2>, ",
         modes=("NMC_MODE_SYNC",), fallbacks=None,
         sites=("store_pending", "nmc_hyper (in the persistent step loop)"),
         **dict(_SWEEP, C=64)),
    Case(name="launch", env={"NMC_PERSIST": "0"}, kernel="nmc_k_run<FamLinreg<2>, ",
         modes=("NMC_MODE_LAUNCH",), fallbacks=None, sites=("store_pending", "nmc_hyper"),
         **dict(_SWEEP, persistent=False)),
    Case("p4", "logistic-partial", [30] * 5, 66, {}, 0, "nmc_k_run<FamLogistic<4>, ",
         ("NMC_MODE_SYNC_REG",), True, 64, 1, None, 4, 0.7,
         ("store_pending", "nmc_hyper_finish")),
    Case("half", "gauss-none", [25] * 4, 65, {}, 0, "nmc_k_run<FamGaussMean<3>, ",
         ("NMC_MODE_HALF",), True, 32, 1, None, 3, 0.3, ("store_pending",)),
    Case("full", "gauss-none", [25] * 4, 65, {"NMC_HALF": "0"}, 0,
         "nmc_k_run<FamGaussMean<3>, ", ("NMC_MODE_NOPOOL",), True, 64, 1, None, 3, 0.3,
         ("store_pending",)),
    Case("complete", "linreg-complete", [43], 70, {}, 0, "nmc_k_run<FamLinreg<2>, ",
         ("NMC_MODE_HALF", "NMC_MODE_NOPOOL"), True, None, 1, None, 3, 0.05,
         ("store_pending",)),
    Case("complete-split", "linreg-complete", [8200], 66, {}, 0, "nmc_k_run<FamLinreg<2>, ",
         ("NMC_MODE_NOPOOL",), True, 64, None, None, 3, 0.002, ("store_pending",)),
    Case("partial-split", "linreg-partial", [8193] * 3, 64, {}, 0, "nmc_k_run<FamLinreg<2>, ",
         ("NMC_MODE_SYNC_REG",), True, 64, None, None, 2, 0.02,
         ("store_pending", "nmc_hyper_finish")),
    Case("user", "user-none", [40] * 5, 65, {}, 0, "nmc_k_run<FamUser, ",
         ("NMC_MODE_HALF", "NMC_MODE_NOPOOL"), True, None, 1, None, 2, 0.2,
         ("store_pending (hiprtc)",)),
]
BY_NAME = {c.name: c for c in CASES}
NAMES = [c.name for c in CASES]
# every (case, schedule) the identity is asserted on: reg runs all, the others CORE
IDENTITY = [(c.name, s) for c in CASES for s in (SCHEDULES if c.name == "reg" else CORE)]


class HostLinregKnown:
    """LinearRegression.__call__ with a known sigma, without freezing a scipy distribution
    per call (oracle.restatement.norm_logpdf is scipy's logpdf restated)."""

    def __init__(self, fam):
        assert fam.sigma is not None
        self.X, self.y, self.sigma = fam.X, fam.y, numpy.float64(fam.sigma)

    def __call__(self, parameter):
        K = self.X.shape[1]
        betaHat = numpy.vstack([parameter[j] for j in range(K)]).T
        yHat = numpy.sum(self.X * betaHat, axis=1)
        return rs.norm_logpdf(yHat, self.y, self.sigma)


Built = collections.namedtuple("Built", "case fam sizes pooling priors st scale nested sel")


def _linreg_data(n):
    d = numpy.random.RandomState(3)
    x = d.normal(size=n)
    return x, 1.0 + 3.0 * x + d.normal(size=n) * 0.7


@functools.lru_cache(maxsize=None)
def _model(model, sizes, C):
    """(family, pooling, priors, host function, centre of the start values) of a model."""
    sizes = list(sizes)
    n, G = int(sum(sizes)), len(sizes)
    if model == "linreg-partial":
        x, y = _linreg_data(n)
        fam = LinearRegression.simple(x, y, sigma=1.0)
        return fam, "partial", None, HostLinregKnown(fam), numpy.array([1.0, 3.0])
    if model == "linreg-complete":
        x, y = _linreg_data(n)
        fam = LinearRegression(numpy.vstack([numpy.ones(n), x]).T, y)
        return (fam, "complete", dc.PRIOR_SETS["A"](), dc.HostLinreg(fam),
                numpy.array([1.0, 3.0, 0.7]))
    if model == "logistic-partial":
        assert len(set(sizes)) == 1
        fam, s, priors, pooling, _ = synthetic("logistic_partial", C, G, sizes[0])
        assert s == sizes and pooling == "partial" and priors is None
        return fam, pooling, None, fam, numpy.zeros(4)
    if model == "gauss-none":
        assert len(set(sizes)) == 1
        fam, s, priors, pooling, _ = synthetic("gauss_none", C, G, sizes[0])
        assert s == sizes and pooling == "none"
        return fam, pooling, priors, fam, numpy.zeros(3)
    if model == "user-none":
        x, y = user_models.poisson_data(G, sizes[0])
        host = user_models.poisson_host(x, y, 0.1)
        fam = DeviceLikelihood(user_models.poisson_rows(x, y), user_models.POISSON, 2,
                               consts=[0.1], host_function=host)
        return fam, "none", dc.PRIOR_SETS["U"](), host, numpy.array([0.5, 0.3])
    raise KeyError(model)


@functools.lru_cache(maxsize=None)
def build(name):
    """The case's family, priors, start state of all C chains (finite everywhere), proposal
    scales [C, P, G], the oracle's Nested and the chains the oracle runs (0, 1 and C - 1).
    Cases of one shape share one start, so they can be compared with each other."""
    c = BY_NAME[name]
    fam, pooling, priors, host, centre = _model(c.model, tuple(c.sizes), c.C)
    G, C, P = len(c.sizes), c.C, len(centre)
    assert fam.n_params == P == c.P
    r = numpy.random.RandomState(zlib.crc32(("%s/%r/%d" % (c.model, c.sizes, C)).encode()))
    nested = FastNested(host, c.sizes)
    sd = 4.0 * c.scale if max(c.sizes) > 1000 else 0.3
    if pooling == "partial":
        mu = centre + r.normal(0, sd / 3, size=(C, P))
        s2 = r.uniform(0.2, 1.0, size=(C, P)) * sd ** 2
        value = mu[:, :, None] + numpy.sqrt(s2)[:, :, None] * r.normal(size=(C, P, G))
        lp = rs.norm_logpdf(value, mu[:, :, None], numpy.sqrt(s2)[:, :, None])
    else:
        mu = s2 = None
        start = centre + r.normal(0, sd / 3, size=(C, P))
        if c.model == "user-none":
            start[:, 1] = numpy.clip(start[:, 1], 0.05, 0.55)    # the slope's support
        value = numpy.repeat(start[:, :, None], G, axis=2)
        lp = numpy.stack([numpy.asarray(priors[p].logpdf(value[:, p, :]), float)
                          for p in range(P)], 1)
    ll = numpy.array([nested.group_ll(value[k]) for k in range(C)])
    assert numpy.all(numpy.isfinite(lp)) and numpy.all(numpy.isfinite(ll)), name
    scale = numpy.full((C, P, G), c.scale)
    sel = numpy.array([0, 1, C - 1])
    return Built(c, fam, list(c.sizes), pooling, priors, rs.State(value, lp, ll, mu, s2), scale,
                 nested, sel)


def engine_kw(name, burn, thin, tune_interval=TUNE_OFF):
    """The keywords of gpu_cases.run_engine for the case under (burn, thin)."""
    b = build(name)
    return dict(pooling=b.pooling, priors=b.priors, env=b.case.env, burn=burn, thin=thin,
                tune_interval=tune_interval, launch_iters=b.case.launch_iters, scale=b.scale)


@functools.lru_cache(maxsize=None)
def oracle(name, burn, thin, tune_interval=TUNE_OFF):
    """(flags, proposal LLs, recorded iterations, rows [3, n_rows, cols], least margin) of
    chains build().sel under (burn, thin): gpu_cases.run_oracle_state, whose
    oracle.restatement.run thins on its own."""
    b = build(name)
    with numpy.errstate(all="ignore"):    # (a proposed sigma <= 0: a NaN likelihood)
        acc, llp, rows, margin, _, trace = run_oracle_state(
            b.nested, b.st, b.sel, b.sel + BASE, N_ITER, SEED, pooling=b.pooling,
            priors=b.priors, burn=burn, thin=thin, tune_interval=tune_interval, scale=b.scale)
    return acc, llp, trace["recorded"], rows, float(margin)


def schedule_rows(n_iter, burn, thin):
    """nmc_set_schedule's row count, restated (the GPU test holds it to Engine.n_rows; the CPU
    test to the library's own loop, nmc_debug_schedule_rows)."""
    return sum(1 for i in range(burn, n_iter) if i % thin == 0)
