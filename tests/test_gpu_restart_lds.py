"""GPU: the step restart without gathers changes no bit.

With two or more parameters the next step proposes another parameter than the current step
decides, so nmc_k_run's control wave forms the next proposal a step ahead and leaves it in an
LDS column; after barrier B the tile waves on the quad row loop read the four chains of their
quarter position straight from the parameters' columns, beside the first tile's rows
(csrc/step.h lik_tiles, csrc/rows.h nmc_rows_lds_linreg2_quad_first).  The paired and the
broadcast loops (NMC_ROWS=pair / bcast) keep forming the proposal in every wave and gathering
it across lanes, and so does the first step of every call: each case here runs the same chains

* on the default path in one call (the reference of the case),
* on the default path in calls of 1, 2 and 7 iterations, launched and resident (the first
  step of a call and the step after a resident gate keep the gathers),
* with NMC_ROWS=pair in the same resident calls and with NMC_ROWS=bcast in one call,

and compares accept flags, trace LLs, sample rows and the final state bit for bit.  The
burn-in of 6 iterations tunes every other iteration (tune_interval 2): a scale changes at its
own parameter's decision while the other parameter's proposal is already in the column.

The quad path cannot be read back from the device; launch_config() names what selects it
(csrc/nestmc.hip nmc_create: {x, y} regression rows in LDS and no NMC_ROWS): the kernel
instance nmc_k_run<FamLinreg<2>, ..., true>.  Shapes without it -- one parameter, three
fields -- run the same comparison on the path they keep.
"""

import numpy
import pytest

import rowpath_cases as rp
from gpu_cases import run_engine
from nestmc.engine import Engine
from nestmc.families import LinearRegression
from oracle import restatement as rs

pytestmark = pytest.mark.gpu

N_ITER, BURN, TUNE, SEED = 10, 6, 2, 41
ONE_CALL = [("run", 0, N_ITER)]
CALLS_1_2_7 = [("run", 0, 1), ("run", 1, 3), ("run", 3, 10)]
# (resident: a call continues the launch when its variates were prefilled for it)
RESIDENT_1_2_7 = [("run", 0, 1), ("prefill", 1, 3), ("run", 1, 3), ("prefill", 3, 10),
                  ("run", 3, 10)]
RAGGED = [1, 15, 0, 64, 65, 300]    # empty, fewer than 16 rows, a tail, several tiles

# name: (fields, intercept, sigma known, group sizes, chains, quad rows)
CASES = {
    "ragged-C65": (2, True, True, RAGGED, 65, True),     # a second chain block, one live lane
    "ragged-C130": (2, True, True, RAGGED, 130, True),   # an even chain count, a partial block
    "G2": (2, True, True, [40, 300], 130, True),
    "G64": (2, True, True, None, 65, True),
    "P3-sigma": (2, True, False, RAGGED, 130, True),     # FamLinreg<2>, sigma sampled: P = 3
    "P2-slope-sigma": (2, False, False, RAGGED, 65, True),   # no intercept column to read
    "P3-fields3": (3, True, True, RAGGED, 65, False),    # FamLinreg<3>: no quad loop
    "P1": (1, True, True, RAGGED, 65, False),            # the proposal depends on the decision
}


def _model(name):
    nf, icpt, known, sizes, C, quad = CASES[name]
    r = numpy.random.RandomState(sum(map(ord, name)))
    if sizes is None:
        sizes = [int(s) for s in r.randint(16, 49, size=64)]
        sizes[5] = 0
    G, n = len(sizes), int(sum(sizes))
    grp = numpy.repeat(numpy.arange(G), sizes)
    X = numpy.hstack([numpy.ones((n, 1)), r.normal(size=(n, nf - 1))])
    if not icpt:
        X = X[:, 1:]
    K = X.shape[1]
    beta = r.normal(0, 0.7, size=(K, G)) + numpy.arange(K)[:, None]
    y = numpy.sum(X * beta[:, grp].T, axis=1) + 0.8 * r.normal(size=n)
    fam = LinearRegression(X, y, sigma=1.0 if known else None)
    P = fam.n_params
    assert fam.n_fields == nf and P == K + (0 if known else 1)
    mu = beta.mean(axis=1)[None] + r.normal(0, 0.2, size=(C, K))
    s2 = r.uniform(0.3, 0.8, size=(C, P))
    value = beta[None] + 0.3 * r.normal(size=(C, K, G))
    if not known:
        mu = numpy.hstack([mu, numpy.full((C, 1), 0.9)])
        value = numpy.concatenate([value, 0.6 + r.uniform(0, 0.6, size=(C, 1, G))], axis=1)
    lp = rs.norm_logpdf(value, mu[:, :, None], numpy.sqrt(s2)[:, :, None])
    eng = Engine(fam, sizes, C, "partial", None, seed=SEED)
    ll = eng.eval_group_ll(value)      # the start's LLs: the device's own, once per case
    eng.close()
    assert numpy.all(numpy.isfinite(ll))
    return fam, sizes, rs.State(value, lp, ll, mu, s2), C, quad


def _run(model, calls=ONE_CALL, env=None, resident=False):
    fam, sizes, st, C, _ = model
    return run_engine(fam, sizes, st, numpy.arange(C), 3, N_ITER, SEED, burn=BURN,
                      tune_interval=TUNE, calls=calls, env=env, resident=resident)


def _same(a, b, what):
    for k in range(3):      # accept flags, trace LLs, sample rows
        assert numpy.array_equal(a[k], b[k], equal_nan=True), (what, k)
    for k in ("value", "log_prior", "ll", "scale", "mu", "s2"):
        assert numpy.array_equal(a[3]["state"][k], b[3]["state"][k], equal_nan=True), (what, k)
    assert numpy.array_equal(a[3]["accept"], b[3]["accept"]), what


@pytest.mark.parametrize("name", list(CASES))
def test_restart_bit_identical(gpu_lib, name, monkeypatch):
    monkeypatch.setenv("NMC_RESIDENT_IDLE_US", "5000")
    model = _model(name)
    fam, sizes, st, C, quad = model
    base = _run(model)
    cfg = base[3]
    what = (name, cfg)
    # the path: the persistent register-hand-off kernel with the group's rows in LDS; quad
    # rows are its {x, y} instance without NMC_ROWS
    assert cfg["persistent"] and cfg["mode"] == "NMC_MODE_SYNC_REG", what
    assert cfg["split_members"] == 1 and cfg["chains_per_block"] == 64, what
    assert cfg["chain_blocks"] == -(-C // 64), what
    assert cfg["kernel"].startswith("nmc_k_run<FamLinreg<%d>" % fam.n_fields), what
    assert cfg["kernel"].endswith(", true>"), what
    assert quad == (fam.n_fields == 2), what
    if sizes[:6] == RAGGED:   # the shapes mean what the table says (dev.h nmc_tiles)
        assert [len(rp.tiles(s)) for s in RAGGED] == [1, 1, 0, 1, 2, 5]
        assert rp.tiles(65)[1] == (48, 17) and rp.tiles(300)[4] == (256, 44)
    # not vacuous: chains move, scales were tuned, every value is finite
    assert 0.02 < base[0].mean() < 0.98, (name, base[0].mean())
    assert numpy.any(cfg["state"]["scale"] != 1.0), name
    assert numpy.all(numpy.isfinite(base[2])), name
    # calls of 1, 2 and 7 iterations: the first step of every call, then the resident gate
    split = _run(model, calls=CALLS_1_2_7)
    assert split[3]["resident"]["launches"] == 0
    _same(split, base, (name, "calls"))
    res = _run(model, calls=RESIDENT_1_2_7, resident=True)
    r = res[3]["resident"]
    if quad:    # (the other instances: resident where their registers allow it)
        assert r["enabled"] and r["launches"] >= 1 and r["calls"] >= 1, (name, r)
    _same(res, base, (name, "resident"))
    # the loops that keep the gathers
    variants = {"bcast": ({"NMC_ROWS": "bcast"}, ONE_CALL, False)}
    if fam.n_fields == 2:
        variants["pair"] = ({"NMC_ROWS": "pair"}, RESIDENT_1_2_7, True)
    for vname, (env, calls, resident) in variants.items():
        got = _run(model, calls=calls, env=env, resident=resident)
        assert got[3]["kernel"] == cfg["kernel"] and got[3]["mode"] == cfg["mode"], (name, vname)
        _same(got, base, (name, vname))
