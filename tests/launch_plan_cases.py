"""The shapes whose launch plan -- what csrc/nestmc.hip (nmc_create, choose_geometry and the
kernel choice after it) decides from the shape alone -- is recorded in
tests/golden/launch_plans.json by tools/record_launch_plans.py and compared key for key by
tests/test_gpu_launch_plans.py.

A case is (name, family kind, n_fields, group sizes, chains, pooling).  The observations
are zeros: nmc_create never evaluates them, only the shapes matter.  ``expect`` names the
path the case is in the table for, as a subset of the plan's keys; the recorder refuses a
case that does not take it (so does tests/test_launch_plan_fixture.py, from the file).
"""

import collections
import os

import numpy
import scipy.stats

from nestmc.families import GaussianMean, LinearRegression, Logistic

PlanCase = collections.namedtuple("PlanCase", "name kind nf sizes chains pooling expect")

SWEEP_CFG4 = "nmc_k_sweep<FamLinreg<2>, NMC_MODE_SYNC_OWN>"


def _gibbs(G, mode, kernel="nmc_k_run<FamLinreg<1>, %s, true>", chains=65, n=32):
    """Partial pooling, one parameter, G small groups: the Gibbs hand-off by group count."""
    mode = "NMC_MODE_" + mode
    return PlanCase("gibbs-G%d" % G, "linreg", 1, [n] * G, chains, "partial",
                    dict(mode=mode, kernel=kernel % mode if "%s" in kernel else kernel))


CASES = [
    PlanCase("cfg3", "linreg", 2, [1000] * 64, 256, "partial",
             dict(mode="NMC_MODE_SYNC_REG", persistent=True)),
    PlanCase("cfg2", "gauss", 3, [500] * 32, 256, "none",
             dict(mode="NMC_MODE_HALF", chains_per_block=32)),
    PlanCase("cfg2-c1024", "gauss", 3, [500] * 32, 1024, "none",
             dict(mode="NMC_MODE_NOPOOL", chains_per_block=64)),
    PlanCase("complete", "linreg", 2, [100] * 8, 64, "complete", dict(split_members=1)),
    _gibbs(2, "SYNC_REG"),
    _gibbs(64, "SYNC_REG"),
    _gibbs(65, "SYNC_LDS"),
    _gibbs(120, "SYNC_LDS"),
    _gibbs(129, "SYNC_OWN", "nmc_k_sweep<FamLinreg<1>, NMC_MODE_SYNC_OWN>"),
    _gibbs(512, "SYNC_OWN", "nmc_k_sweep<FamLinreg<1>, NMC_MODE_SYNC_OWN>"),
    # (five numpy leaves: 48 KiB of hyper carve, three workgroups per CU.  One chain block of
    # four-wave workgroups is co-resident; three-wave ones keep a workgroup of margin and two
    # chain blocks are 1026 workgroups: both launch per iteration)
    _gibbs(513, "SYNC", chains=64, n=100),
    # the sweep with its Gibbs kernel: two chain blocks resident at once
    PlanCase("cfg4-shard", "linreg", 2, [2000] * 256, 128, "partial",
             dict(mode="NMC_MODE_SYNC_OWN", kernel=SWEEP_CFG4, persistent=True, chain_blocks=2,
                  chain_blocks_per_launch=2)),
    # 16 chain blocks: resident batches of the sweep or nmc_k_run, as recorded
    PlanCase("cfg4-whole", "linreg", 2, [2000] * 256, 1024, "partial", dict(chain_blocks=16)),
    # a grid between one and two workgroups per CU
    PlanCase("four-waves", "linreg", 2, [500] * 128, 192, "partial", dict(waves_per_group=4)),
    # a grid that is not co-resident
    PlanCase("launch", "linreg", 2, [100] * 64, 4096, "partial",
             dict(mode="NMC_MODE_LAUNCH", persistent=False)),
    PlanCase("rows-global", "linreg", 2, [5000] * 4, 64, "partial",
             dict(split_members=1, kernel="nmc_k_run<FamLinreg<2>, NMC_MODE_SYNC_REG, false>")),
    PlanCase("split-none", "linreg", 2, [20000] * 4, 64, "none", dict(split_members=5)),
    PlanCase("split-partial", "linreg", 2, [20000] * 4, 64, "partial",
             dict(split_members=5, persistent=True)),
    # nine parameters' hyper state leaves the rows no room in the carve: staged rows
    PlanCase("staged", "logistic", 9, [300] * 8, 64, "partial",
             dict(kernel="nmc_k_run<FamLogistic<9>, NMC_MODE_SYNC_REG, false>")),
    PlanCase("gauss-partial", "gauss", 3, [20] * 4, 64, "partial",
             dict(kernel="nmc_k_run<FamGaussMean<3>, NMC_MODE_SYNC_REG, true>")),
    PlanCase("three-waves", "linreg", 2, [10] * 2, 1, "partial", dict(waves_per_group=3)),
    PlanCase("ragged", "linreg", 2, [1, 15, 0, 64, 65, 300, 1023], 65, "partial",
             dict(split_members=1)),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def family(case):
    n = int(sum(case.sizes))
    if case.kind == "gauss":
        return GaussianMean(numpy.zeros((n, case.nf)), numpy.ones(case.nf))
    X = numpy.hstack([numpy.ones((n, 1)), numpy.zeros((n, case.nf - 1))])
    if case.kind == "logistic":
        return Logistic(X, numpy.zeros(n))
    return LinearRegression(X, numpy.zeros(n), sigma=1.0)


def plan(case):
    """launch_config() of the case's engine; no step kernel is launched."""
    from nestmc.engine import Engine
    set_knobs = sorted(k for k in os.environ if k.startswith("NMC_"))
    assert not set_knobs, "launch plans are the defaults: unset %s" % set_knobs
    fam = family(case)
    assert fam.n_fields == case.nf, (case.name, fam.n_fields)
    priors = None if case.pooling == "partial" else [scipy.stats.norm(0, 10)] * fam.n_params
    eng = Engine(fam, case.sizes, case.chains, case.pooling, priors)
    try:
        return eng.launch_config()
    finally:
        eng.close()


def off_path(case, got):
    """The keys of case.expect that the plan ``got`` does not meet: {key: (want, got)}."""
    return {k: (v, got.get(k)) for k, v in case.expect.items() if got.get(k) != v}
