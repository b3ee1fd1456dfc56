"""Posterior predictive checks on the GPU (csrc/ppc.h): nmc_ppc_draws and nmc_ppc_partials
through Engine.predictive_draws / ppc_partials / ppc and samplePosterior(
computePredictiveChecks=True), on the sample stores of tests/store_cases.py (written with
Engine.set_samples_raw: no test samples but the last two).

References and tolerances: tests/ppc_ref.py, which tests/test_ppc_host.py holds on the CPU --
the draws against the stream restated with oracle.philox and the family's formula in
longdouble; the reductions of the device's own draws against ppc_ref.restate word for word
(counts, T(y), n, mean, M2: IEEE + - x / only) and against the longdouble reference within
the tolerances.  Every test prints its worst error / tolerance ratio.
"""

import os

import numpy
import pytest

import ppc_ref
import store_cases as sc
from gpu_cases import synthetic
from nestmc import _lib, ppc
from nestmc.engine import Engine
from nestmc.families import DeviceLikelihood

pytestmark = pytest.mark.gpu

WINDOWS = ((0, sc.R), (3, 1), (sc.R - 2, 2))
KEYS = ("obs_state", "obs_count", "group_state", "group_count", "ty")


class Engines:
    """One engine per family object (seed ppc_ref.SEED), made on first use; ``load`` writes a
    case's store unless it is the one the engine holds; ``draws``: the device's own replicates
    of a case's whole store, computed once."""

    def __init__(self):
        self.eng, self.holds, self.yrep = {}, {}, {}

    def load(self, name, fam=None, key=None, n_chains=sc.C, chain_base=0):
        case = ppc_ref.case_of(name)
        key = key or (case.kind, name if name in ("offset", "misfit") else "")
        if key not in self.eng:
            e = Engine(fam or case.fam, sc.SIZES, n_chains, case.pooling, case.priors,
                       seed=ppc_ref.SEED, chain_base=chain_base)
            e.set_schedule(sc.R, 0, 1)             # R recorded rows; no run()
            assert (e.n_rows, e.cols) == (sc.R, case.cols)
            self.eng[key] = e
        e = self.eng[key]
        if self.holds.get(key) != name:
            e.set_samples_raw(numpy.ascontiguousarray(
                case.store[:, :, chain_base:chain_base + n_chains]))
            self.holds[key] = name
        return e

    def draws(self, name):
        if name not in self.yrep:
            self.yrep[name] = self.load(name).predictive_draws()
            self.yrep[name].setflags(write=False)
        return self.yrep[name]

    def close(self):
        for e in self.eng.values():
            e.close()


@pytest.fixture(scope="module")
def engines(gpu_lib):
    es = Engines()
    yield es
    es.close()


def _words(a):
    return numpy.ascontiguousarray(a, dtype=numpy.float64).view(numpy.uint64)


def _same(a, b, what):
    for k in KEYS:
        x, y = numpy.asarray(a[k]), numpy.asarray(b[k])
        assert x.shape == y.shape, (what, k, x.shape, y.shape)
        if x.dtype == numpy.float64:
            assert numpy.array_equal(_words(x), _words(y)), \
                (what, k, int((_words(x) != _words(y)).sum()), x.size)
        else:
            assert numpy.array_equal(x, y), (what, k)


# ---- 1. the draws ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["benign", "offset", "sigma", "gauss", "logistic"])
def test_draws(engines, name):
    case = sc.BY_NAME[name]
    dev = engines.draws(name)
    ref = ppc_ref.draws(name)
    NR = len(case.fam.response_fields())
    assert dev.shape == (sc.C, sc.R, sc.N_OBS, NR) and engines.load(name).n_resp() == NR
    assert numpy.isfinite(dev).all()
    if case.kind == "logistic":
        want = numpy.asarray(ref["yrep"], dtype=numpy.float64)
        print("ppc draws %s: %d of %d differ (min |ua - p| = %.3g)"
              % (name, int((dev != want).sum()), dev.size, ref["gap"].min()))
        assert numpy.array_equal(dev, want)
        assert set(numpy.unique(dev)) == {0.0, 1.0}
        return
    err = numpy.abs(dev.astype(ppc_ref.LD) - ref["yrep"]).astype(numpy.float64)
    ratio = float(numpy.max(err / ref["tol"]))
    print("ppc draws %s: max err/tol = %.3g (max err %.3g)" % (name, ratio, err.max()))
    assert ratio <= 1.0


# ---- 2. keying ------------------------------------------------------------------------------
def test_draws_depend_on_row_and_global_chain_alone(engines):
    full = engines.draws("benign")
    eng = engines.load("benign")
    one = eng.predictive_draws(3, 1)
    assert one.shape == (sc.C, 1, sc.N_OBS, 1)
    assert one.tobytes() == numpy.ascontiguousarray(full[:, 3:4]).tobytes()
    tail = eng.predictive_draws(sc.R - 2, 2)
    assert tail.tobytes() == numpy.ascontiguousarray(full[:, sc.R - 2:]).tobytes()
    a = engines.load("benign", key="shard0", n_chains=64, chain_base=0).predictive_draws()
    b = engines.load("benign", key="shard64", n_chains=6, chain_base=64).predictive_draws()
    assert numpy.concatenate([a, b]).tobytes() == full.tobytes()
    # and the partials of whole chain blocks are the one engine's blocks
    pa = engines.load("benign", key="shard0", n_chains=64).ppc_partials()
    pb = engines.load("benign", key="shard64", n_chains=6, chain_base=64).ppc_partials()
    whole = eng.ppc_partials()
    _same(pa[0], whole[0], "shard 0")
    _same(pb[0], whole[1], "shard 64")


# ---- 3. the reductions on the device's own draws --------------------------------------------
@pytest.mark.parametrize("name", sc.FINITE)
def test_reductions(engines, name):
    case = sc.BY_NAME[name]
    yrep = engines.draws(name)
    eng = engines.load(name)
    y = ppc_ref.y_of(case)
    integer = case.fam.response_integer
    assert numpy.array_equal(eng.observed(), y)
    worst = 0.0
    for rb, nr in WINDOWS:
        for nv in case.n_valid:
            what = "%s rows %d+%d n_valid %d" % (name, rb, nr, nv)
            parts, bad = eng.ppc_partials_raw(rb, nr, nv)
            assert bad == 0 and len(parts) == 2, what
            want = ppc_ref.restate(yrep[:, rb:rb + nr], y, sc.C, nv, integer)
            for b in range(2):
                _same(parts[b], want[b], "%s block %d" % (what, b))
            ref = ppc_ref.reference(yrep[:, rb:rb + nr], y, nv, integer)
            merged = ppc.merge(parts)
            assert numpy.array_equal(merged["obs_count"][0], ref["lt"].T), what
            assert numpy.array_equal(merged["obs_count"][1], ref["eq"].T), what
            worst = max(worst, ppc_ref.check_states(merged, ref, what))
    print("ppc reductions %s: worst err/tol = %.3g" % (name, worst))


# ---- 4. padding -----------------------------------------------------------------------------
def test_padding_block_is_the_identity(engines):
    eng = engines.load("gauss")
    parts, bad = eng.ppc_partials_raw(0, sc.R, 64)
    ident = ppc.identity(sc.N_OBS, sc.G, 3)
    for k in ("obs_state", "obs_count", "group_state", "group_count"):
        assert numpy.asarray(parts[1][k]).tobytes() == numpy.asarray(ident[k]).tobytes(), k
    full, _ = eng.ppc_partials_raw(0, sc.R, sc.C)
    _same(parts[0], full[0], "block 0")          # (block 0 has no padding either way)
    res = ppc.finish(ppc.merge(parts), sc.OFF, eng.observed())
    assert res.n_samples == 64 * sc.R


# ---- 5. draws that are not finite -----------------------------------------------------------
def test_nonfinite(engines):
    case = sc.BY_NAME["sigma_bad"]
    ref = ppc_ref.draws("sigma_bad")["yrep"]
    isbad = ~numpy.isfinite(numpy.asarray(ref, dtype=numpy.float64))      # [C][R][n_obs][1]
    assert isbad.sum() > 0
    dev = engines.draws("sigma_bad")
    assert numpy.array_equal(~numpy.isfinite(dev), isbad)
    base = {}
    eng = engines.load("sigma")
    for rb, nr in WINDOWS:
        for nv in case.n_valid:
            base[rb, nr, nv] = eng.ppc_partials_raw(rb, nr, nv)[0]
    eng = engines.load("sigma_bad")
    seen = 0
    for rb, nr in WINDOWS:
        for nv in case.n_valid:
            parts, bad = eng.ppc_partials_raw(rb, nr, nv)
            want = int(isbad[:nv, rb:rb + nr].sum())
            assert bad == want, (rb, nr, nv, bad, want)
            seen += bad
            touched = sc.touched_groups(case, rb, nr, nv)
            clean_g = [g for g in range(sc.G) if g not in touched]
            clean_o = numpy.isin(sc.GRP, clean_g)
            for b in range(2):
                p, q = parts[b], base[rb, nr, nv][b]
                assert numpy.array_equal(_words(p["obs_state"][..., clean_o]),
                                         _words(q["obs_state"][..., clean_o]))
                assert numpy.array_equal(p["obs_count"][..., clean_o], q["obs_count"][..., clean_o])
                assert numpy.array_equal(_words(p["group_state"][clean_g]),
                                         _words(q["group_state"][clean_g]))
                assert numpy.array_equal(p["group_count"][clean_g], q["group_count"][clean_g])
                # a non-finite draw enters no count: the counts do not exceed the base's
                assert numpy.all(p["obs_count"].sum(axis=0) <= nr * 64)
            merged = ppc.merge(parts)
            if want:      # the NaN reached the states of the groups it touched
                assert numpy.isnan(merged["obs_state"][1:]).any()
                assert numpy.isnan(merged["group_state"][..., 1:]).any()
    print("ppc nonfinite: %d draws counted over the windows" % seen)
    assert seen > 0
    with pytest.raises(_lib.NestmcError, match="not finite"):
        eng.ppc()
    assert eng.ppc_nonfinite == int(isbad.sum())


# ---- 6. a group the model does not fit ------------------------------------------------------
def test_misfit_group_is_flagged(engines):
    case = ppc_ref.case_of("misfit")
    eng = engines.load("misfit")
    res = eng.ppc()
    g = ppc_ref.MISFIT_GROUP
    print("ppc misfit p:\n%s" % res.p[:, 0])
    assert res.p[g, 0, 0] == 0.0 and res.gt[g, 0, 0] == 0 and res.geq[g, 0, 0] == 0
    assert {f[0] for f in res.flagged()} == {g}
    others = numpy.delete(res.p, g, axis=0)
    assert numpy.all((others > 0.025) & (others < 0.975))
    assert "group %d mean" % g in res.warning()
    # the CPU test's decision (tests/test_ppc_host.py) on the reference draws
    y = ppc_ref.y_of(case)
    host = ppc.finish(ppc.merge(ppc_ref.restate(ppc_ref.f64("misfit"), y, sc.C, sc.C)), sc.OFF, y)
    assert {f[0] for f in host.flagged()} == {g}


# ---- 7. a run-time-compiled user family -----------------------------------------------------
# FamLinreg<2>'s obs_ll and predict with the known sigma = 1 (csrc/families.h), restated
LINREG2 = r"""
__device__ double nmc_user_loglik(const double* th, const double* row, const double* k) {
  double yh = th[0];
  yh = yh + row[0] * th[1];
  const double s = k[0];
  const double t = (yh - row[1]) / s;
  return (-(t * t) / 2.0 - NMC_LOG_C) - k[1];
}
"""
LINREG2_PREDICT = LINREG2 + r"""
__device__ double nmc_user_predict(const double* th, const double* row, const double* k,
                                   double ua, double ub, double z) {
  double yh = th[0];
  yh = yh + row[0] * th[1];
  const double s = k[0];
  if (!(s > 0.0)) return nmc_nan();
  return yh + s * z;
}
"""


def test_user_family_bit_identical_to_builtin(engines):
    case = sc.BY_NAME["benign"]
    user = DeviceLikelihood(case.fam.obs(), LINREG2_PREDICT, 2, consts=[1.0, 0.0],
                            response_field=1)
    assert user.response_fields() == [1]
    a = engines.load("benign")
    b = engines.load("benign", fam=user, key="user")
    assert b.n_resp() == 1
    assert a.obs_ll_rows().tobytes() == b.obs_ll_rows().tobytes()
    assert engines.draws("benign").tobytes() == b.predictive_draws().tobytes()
    for rb, nr in WINDOWS:
        pa, pb = a.ppc_partials_raw(rb, nr, 65), b.ppc_partials_raw(rb, nr, 65)
        assert pa[1] == pb[1] == 0
        for k in range(2):
            _same(pa[0][k], pb[0][k], "user rows %d+%d block %d" % (rb, nr, k))
    # a source without nmc_user_predict cannot draw
    plain = DeviceLikelihood(case.fam.obs(), LINREG2, 2, consts=[1.0, 0.0])
    assert plain.response_fields() == []
    c = engines.load("benign", fam=plain, key="user_plain")
    assert c.n_resp() == 0
    for call in (c.ppc_partials, c.predictive_draws):
        with pytest.raises(_lib.NestmcError, match="nmc_user_predict"):
            call()
    with pytest.raises(ValueError, match="nmc_user_predict"):
        DeviceLikelihood(case.fam.obs(), LINREG2, 2, response_field=1)


# ---- 8. argument errors ---------------------------------------------------------------------
def test_bad_arguments(engines):
    eng = engines.load("benign")
    for kw in (dict(n_rows=0), dict(row_begin=sc.R - 2, n_rows=3), dict(row_begin=-1, n_rows=2),
               dict(row_begin=sc.R, n_rows=1), dict(n_valid=0), dict(n_valid=sc.C + 1)):
        with pytest.raises(_lib.NestmcError):
            eng.ppc_partials(**kw)
    for kw in (dict(row_begin=sc.R - 2, n_rows=3), dict(row_begin=-1, n_rows=2),
               dict(row_begin=sc.R, n_rows=1)):
        with pytest.raises(_lib.NestmcError):
            eng.predictive_draws(**kw)
    assert len(eng.ppc_partials()) == 2                     # (the context still works)
    assert eng.predictive_draws(2, 0).size == 0


# ---- 9. samplePosterior(computePredictiveChecks=True) ---------------------------------------
def _close_to(res, other, yrep, y, off, what):
    """The floats of two PpcResults of the same samples within the reductions' tolerances
    (ppc_ref: mean (S + 64) u max |x|, M2 (S + 64) u sum x^2), from the replicates yrep[S]."""
    S = yrep.shape[0]
    L = yrep.astype(ppc_ref.LD)
    worst = 0.0

    def cmp(a, b, amax, sq):
        nonlocal worst
        tm, t2 = ppc_ref.tol_mean(S, amax), ppc_ref.tol_m2(S, sq)
        em = numpy.abs(a[0] - b[0])
        e2 = numpy.abs(a[1] ** 2 - b[1] ** 2) * (S - 1)
        with numpy.errstate(invalid="ignore", divide="ignore"):
            r = max(float(numpy.max(numpy.where(tm > 0, em / tm, em > 0))),
                    float(numpy.max(numpy.where(t2 > 0, e2 / t2, e2 > 0))))
        worst = max(worst, r)
        assert r <= 1.0, (what, r)

    cmp((res.mean_i, res.sd_i), (other.mean_i, other.sd_i),
        numpy.abs(L).max(axis=0), (L * L).sum(axis=0))
    T = numpy.stack([ppc_ref.t_stats(numpy.moveaxis(yrep[:, a:b], 1, -1))
                     for a, b in zip(off[:-1], off[1:])], axis=1).astype(ppc_ref.LD)  # [S][G][NR][4]
    cmp((res.t_mean, res.t_sd), (other.t_mean, other.t_sd), numpy.abs(T).max(axis=0),
        (T * T).sum(axis=0))
    print("ppc %s: worst err / tol = %.3g" % (what, worst))


def test_sample_posterior_compute_predictive_checks(gpu_lib, tmp_path):
    from nestmc.init import init_chains
    from nestmc.sampler import sample_posterior, schedule
    C, G, N = 70, 5, 30
    fam, sizes, priors, pooling, names = synthetic("linreg_partial", C, G, N)
    ranges = {n: [-0.5, 0.5] for n in names}
    kw = dict(saveLogLikelihood=False, priorDistribution=priors, startingPointValueRange=ranges,
              displayProgress=False, seed=17, return_samples=True, write_files=True)
    out = str(tmp_path / "one")
    res = sample_posterior(C, 60, 20, names, G, N, pooling, fam, out,
                           computePredictiveChecks=True, **kw)
    r = res["predictive_checks"]
    assert sorted(os.listdir(out)) == ["log", "ppc_groups.csv", "ppc_pointwise.csv", "sample"]
    back = ppc.read_csvs(out)
    for k in ("y", "mean_i", "sd_i", "residual_i", "pit_i", "lt", "eq", "t_obs", "t_mean", "t_sd",
              "p", "gt", "geq", "offsets"):
        assert numpy.array_equal(getattr(r, k), getattr(back, k)), k
    assert back.n_samples == r.n_samples
    # an Engine run of the same seed and start: its replicates through the host route
    burn, thin = schedule(60, 20)
    eng = Engine(fam, sizes, C, pooling, priors, seed=17)
    try:
        st = init_chains(fam, sizes, names, list(range(C)), pooling, priors, ranges, False,
                         group_ll=eng.eval_group_ll)
        eng.set_state(st["value"], st["log_prior"], st["ll"], st["mu"], st["s2"])
        eng.set_schedule(60, burn, thin, 100)
        eng.run(0, 60)
        eng.synchronize()
        assert numpy.array_equal(eng.samples(), res["rows"])
        yrep = eng.predictive_draws().reshape(-1, G * N, 1)
        y, off, n_rows = eng.observed(), eng.off, eng.n_rows
    finally:
        eng.close()
    assert r.n_samples == yrep.shape[0] == C * n_rows
    host = ppc.from_replicates(yrep, y, off)
    for k in ("lt", "eq", "gt", "geq"):
        assert numpy.array_equal(getattr(r, k), getattr(host, k)), k
    assert numpy.array_equal(r.p, host.p) and numpy.array_equal(r.pit_i, host.pit_i)
    _close_to(r, host, yrep, y, off, "samplePosterior against from_replicates")
    # two engines on one GPU: 35 + 35 chains
    two = sample_posterior(C, 60, 20, names, G, N, pooling, fam, str(tmp_path / "two"),
                           computePredictiveChecks=True, devices=[0, 0], **kw)
    assert numpy.array_equal(two["rows"], res["rows"])
    t = two["predictive_checks"]
    for k in ("lt", "eq", "gt", "geq", "t_obs"):
        assert numpy.array_equal(getattr(r, k), getattr(t, k)), k
    _close_to(r, t, yrep, y, off, "devices=[0, 0]")
    # off by default
    off_ = sample_posterior(C, 60, 20, names, G, N, pooling, fam, str(tmp_path / "off"), **kw)
    assert "predictive_checks" not in off_
    assert sorted(os.listdir(str(tmp_path / "off"))) == ["log", "sample"]
    # a family that cannot draw is refused before sampling starts
    plain = DeviceLikelihood(fam.obs(), LINREG2, 2, consts=[1.0, 0.0], host_function=fam)
    with pytest.raises(ValueError, match="nmc_user_predict"):
        sample_posterior(C, 60, 20, names, G, N, pooling, plain, str(tmp_path / "no"),
                         computePredictiveChecks=True, **kw)
    assert not os.path.exists(str(tmp_path / "no"))


def test_process_per_device_rank_path(gpu_lib, tmp_path):
    """process_per_device with one rank: the rank reduces its chains, sends its merged partial
    over the host group and rank 0 finishes and writes -- the files are the in-process path's
    byte for byte."""
    from nestmc.sampler import sample_posterior
    C, G, N = 70, 5, 30
    fam, sizes, priors, pooling, names = synthetic("linreg_partial", C, G, N)
    kw = dict(saveLogLikelihood=False, priorDistribution=priors, computePredictiveChecks=True,
              startingPointValueRange={n: [-0.5, 0.5] for n in names}, displayProgress=False,
              seed=23, return_samples=True, devices=[0])
    one, ppd = str(tmp_path / "one"), str(tmp_path / "ppd")
    r1 = sample_posterior(C, 60, 20, names, G, N, pooling, fam, one, **kw)
    r2 = sample_posterior(C, 60, 20, names, G, N, pooling, fam, ppd, process_per_device=True,
                          **kw)
    assert numpy.array_equal(r1["rows"], r2["rows"])
    for k in ("mean_i", "sd_i", "pit_i", "lt", "eq", "t_obs", "t_mean", "t_sd", "p", "gt", "geq"):
        assert numpy.array_equal(getattr(r1["predictive_checks"], k),
                                 getattr(r2["predictive_checks"], k)), k
    for fn in ("ppc_groups.csv", "ppc_pointwise.csv"):
        assert open(os.path.join(one, fn), "rb").read() == open(os.path.join(ppd, fn), "rb").read()
