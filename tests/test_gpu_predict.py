"""Held-out and new-group prediction on the GPU (csrc/predict.h): nmc_predict_set,
nmc_predict_draws and nmc_predict_partials through Engine.set_new_data / predict_draws /
predict_partials / predict and samplePosterior(predictFor=...), on the sample stores of
tests/store_cases.py (written with Engine.set_samples_raw: no test samples but the last).

References and tolerances: tests/predict_ref.py, which tests/test_predict_host.py holds on the
CPU.  The reductions of the device's own draws and log densities are held against
predict_ref.restate word for word: counts, n, mean, M2, m AND s.  s passes through exp, and
numpy's exp differs from the device library's in the last place (about 50 of 540 s words of a
case came out different with numpy's), so the restatement is handed the DEVICE's exp:
``DeviceExp`` evaluates it on the GPU through a one-line user family (exp(theta) as the
log-likelihood of a one-row group, Engine.eval_group_ll).  Everything is also held against the
longdouble reference within the tolerances.  Every test prints its worst error / tolerance
ratio.
"""

import ctypes
import os

import numpy
import pytest

import ppc_ref
import predict_ref as pr
import store_cases as sc
import waic_ref
from gpu_cases import synthetic
from nestmc import NewData, _lib, predict
from nestmc._lib import dptr
from nestmc.engine import Engine
from nestmc.families import DeviceLikelihood

pytestmark = pytest.mark.gpu

WINDOWS = ((0, sc.R), (3, 1), (sc.R - 2, 2))
LD = pr.LD


class Engines:
    """One engine per key (seed predict_ref.SEED), made on first use; ``load`` writes the store
    and sets the new table unless the engine holds them; ``draws``: the device's own draws, log
    densities and new-group values over a case's whole store, computed once."""

    def __init__(self):
        self.eng, self.holds, self.out = {}, {}, {}

    def load(self, name, key=None, n_chains=sc.C, chain_base=0, fam=None, store=None,
             new=None, tag=""):
        s = pr.setup(name)
        key = key or name
        if key not in self.eng:
            e = Engine(fam or s.fam, sc.SIZES, n_chains, s.pooling, s.case.priors, seed=pr.SEED,
                       chain_base=chain_base)
            e.set_schedule(sc.R, 0, 1)             # R recorded rows; no run()
            assert (e.n_rows, e.cols) == (sc.R, s.case.cols)
            self.eng[key] = e
        e = self.eng[key]
        if self.holds.get(key) != (name, tag):
            st = s.store if store is None else store
            e.set_samples_raw(numpy.ascontiguousarray(st[:, :, chain_base:chain_base + n_chains]))
            e.set_new_data(s.new if new is None else new)
            self.holds[key] = (name, tag)
        return e

    def draws(self, name):
        if name not in self.out:
            d = self.load(name).predict_draws()
            for v in d.values():
                v.setflags(write=False)
            self.out[name] = d
        return self.out[name]

    def close(self):
        for e in self.eng.values():
            e.close()


@pytest.fixture(scope="module")
def engines(gpu_lib):
    es = Engines()
    yield es
    es.close()


EXP_SOURCE = r"""
__device__ double nmc_user_loglik(const double* th, const double* row, const double* k) {
  return exp(th[0]);
}
"""


class DeviceExp:
    """exp of float64 arrays as the device library computes it: a user family whose
    log-likelihood of a one-row group is exp(theta) (a group's sum is 0 + the value: exact),
    evaluated for C x G arguments per call.  Arguments that are not finite are answered here
    (NaN -> NaN, -inf -> 0, +inf -> inf) and never sent."""

    C, G = 128, pr.N_NEW

    def __init__(self):
        import scipy.stats
        fam = DeviceLikelihood(numpy.zeros((self.G, 1)), EXP_SOURCE, 1)
        self.eng = Engine(fam, [1] * self.G, self.C, "none", [scipy.stats.norm(0, 1)], seed=0)
        self.calls = 0

    def __call__(self, x):
        x = numpy.asarray(x, dtype=numpy.float64)
        flat = x.reshape(-1)
        fin = numpy.isfinite(flat)
        with numpy.errstate(all="ignore"):
            out = numpy.exp(flat)              # (the answers for NaN and the infinities)
        arg = flat[fin]
        n = self.C * self.G
        got = numpy.empty(len(arg))
        for a in range(0, len(arg), n):
            chunk = numpy.zeros(n)
            m = min(n, len(arg) - a)
            chunk[:m] = arg[a:a + m]
            res = self.eng.eval_group_ll(chunk.reshape(self.C, 1, self.G))
            got[a:a + m] = res.reshape(-1)[:m]
            self.calls += 1
        out[fin] = got
        return out.reshape(x.shape)

    def close(self):
        self.eng.close()


@pytest.fixture(scope="module")
def device_exp(gpu_lib):
    e = DeviceExp()
    yield e
    e.close()


def _words(a):
    return numpy.ascontiguousarray(a, dtype=numpy.float64).view(numpy.uint64)


def _same(a, b, what, keys=("dens", "state", "count")):
    for k in keys:
        x, y = numpy.asarray(a[k]), numpy.asarray(b[k])
        assert x.shape == y.shape, (what, k, x.shape, y.shape)
        if x.dtype == numpy.float64:
            assert numpy.array_equal(_words(x), _words(y)), \
                (what, k, int((_words(x) != _words(y)).sum()), x.size)
        else:
            assert numpy.array_equal(x, y), (what, k)


def _ratio(err, tol):
    with numpy.errstate(invalid="ignore", divide="ignore"):
        r = numpy.where(tol > 0, err / tol, numpy.where(err > 0, numpy.inf, 0.0))
    return float(numpy.max(r)) if r.size else 0.0


# ---- 1. draws, ll and theta_new -------------------------------------------------------------
@pytest.mark.parametrize("name", pr.NAMES)
def test_draws(engines, name):
    s = pr.setup(name)
    eng = engines.load(name)
    d = engines.draws(name)
    NR = len(s.resp)
    has = s.new.has_response(s.resp)
    assert eng.n_resp() == NR
    assert d["yrep"].shape == (sc.C, sc.R, pr.N_NEW, NR)
    assert d["ll"].shape == (sc.C, sc.R, pr.N_NEW)
    assert d["theta_new"].shape == (sc.C, sc.R, s.K, s.case.P)
    rt = 0.0
    if s.K:
        want, tol, _ = pr.theta_new_ref(name)
        rt = _ratio(numpy.abs(d["theta_new"].astype(LD) - want).astype(numpy.float64), tol)
        assert rt <= 1.0, rt
    ev = pr.evaluate(name, pr.theta_rows(name, d["theta_new"]))
    assert numpy.isfinite(d["yrep"]).all()
    if s.kind == "logistic":
        want = numpy.asarray(ev["yrep"], dtype=numpy.float64)
        print("predict draws %s: %d of %d differ (min |ua - p| = %.3g)"
              % (name, int((d["yrep"] != want).sum()), want.size, ev["gap"].min()))
        assert ev["gap"].min() > 1e-12
        assert numpy.array_equal(d["yrep"], want)
        ry = 0.0
    else:
        ry = _ratio(numpy.abs(d["yrep"].astype(LD) - ev["yrep"]).astype(numpy.float64), ev["tol"])
        assert ry <= 1.0, ry
    assert numpy.isnan(d["ll"][:, :, ~has]).all() and numpy.isfinite(d["ll"][:, :, has]).all()
    unit = sc.obs_ll_units(s.fam.n_fields) * 2.0 ** -53
    err = numpy.abs(d["ll"].astype(LD) - ev["ll"])[:, :, has].astype(numpy.float64)
    rl = _ratio(err, unit * numpy.asarray(ev["A"][:, :, has], dtype=numpy.float64))
    print("predict draws %s: max err/tol  theta_new %.3g  yrep %.3g  ll %.3g" % (name, rt, ry, rl))
    assert rl <= 1.0, rl


def test_family_without_predict_has_the_density_alone(engines):
    full = engines.load("poisson")
    want = engines.draws("poisson")
    plain = pr.poisson_family(False)
    assert plain.response_fields() == []
    eng = engines.load("poisson", key="poisson_plain", fam=plain)
    assert eng.n_resp() == 0
    with pytest.raises(_lib.NestmcError, match="nmc_user_predict"):
        eng.predict_draws()
    got = eng.predict_draws(yrep=False)
    assert got["yrep"] is None
    assert got["ll"].tobytes() == want["ll"].tobytes()
    assert got["theta_new"].tobytes() == want["theta_new"].tobytes()
    # every row counts as one with a response: the NaN rows are in the ll counter
    parts, bad = eng.predict_partials_raw()
    assert bad == (0, int(pr.NO_RESP.sum()) * sc.C * sc.R)
    assert parts[0]["state"].shape == (3, 0, pr.N_NEW)
    fp, fbad = full.predict_partials_raw()
    assert fbad == (0, 0)
    _same(parts[0], fp[0], "density of the plain source", keys=("dens",))
    res = full.predict()
    with pytest.raises(_lib.NestmcError, match="not finite"):
        eng.predict()
    lpd = predict.finish(predict.merge(parts), full.new_data, []).lpd_i
    keep = ~pr.NO_RESP
    assert numpy.array_equal(_words(lpd[keep]), _words(res.lpd_i[keep]))


# ---- 2. keying ------------------------------------------------------------------------------
def test_keying(engines):
    full = engines.draws("benign")
    eng = engines.load("benign")
    for rb, nr in WINDOWS[1:]:
        part = eng.predict_draws(rb, nr)
        for k in ("yrep", "ll", "theta_new"):
            assert part[k].shape[1] == nr
            assert part[k].tobytes() == numpy.ascontiguousarray(full[k][:, rb:rb + nr]).tobytes(), k
    a = engines.load("benign", key="shard0", n_chains=64, chain_base=0)
    b = engines.load("benign", key="shard64", n_chains=6, chain_base=64)
    da, db = a.predict_draws(), b.predict_draws()
    for k in ("yrep", "ll", "theta_new"):
        assert numpy.concatenate([da[k], db[k]]).tobytes() == full[k].tobytes(), k
    whole = eng.predict_partials()
    _same(a.predict_partials()[0], whole[0], "shard 0")
    _same(b.predict_partials()[0], whole[1], "shard 64")
    # rows 2 and 3 (one tile of group 3) trade places: position i keeps its stream, the rows
    # their densities; nothing else moves
    s = pr.setup("benign")
    perm = numpy.arange(pr.N_NEW)
    perm[[2, 3]] = [3, 2]
    swapped = NewData(s.new.obs[perm], s.new.group[perm])
    e2 = engines.load("benign", new=swapped, tag="swapped")
    d2 = e2.predict_draws()
    assert d2["ll"].tobytes() == numpy.ascontiguousarray(full["ll"][:, :, perm]).tobytes()
    assert d2["theta_new"].tobytes() == full["theta_new"].tobytes()
    rest = numpy.setdiff1d(perm, [2, 3])
    assert numpy.array_equal(_words(d2["yrep"][:, :, rest]), _words(full["yrep"][:, :, rest]))
    x = s.new.obs[:, 0]
    th = sc.theta_of(s.case, s.store)                                   # [R][C][P][G]
    slope = numpy.transpose(th[:, :, 1, 3], (1, 0))                     # group 3
    for i, other in ((2, 3), (3, 2)):   # y_rep(i) moved by slope (x_other - x_i): z(i) stayed
        moved = d2["yrep"][:, :, i, 0] - full["yrep"][:, :, i, 0]
        want = slope * (x[other] - x[i])
        assert numpy.allclose(moved, want, rtol=0, atol=1e-12 * (1 + numpy.abs(want).max()))
    engines.load("benign")              # (the table of the other tests back in place)


# ---- 3. the training table as the new table -------------------------------------------------
@pytest.mark.parametrize("name", ["benign", "logistic", "gauss", "sigma"])
def test_training_table_ties_to_waic(engines, name):
    s = pr.setup(name)
    train = NewData(s.fam.obs(), sc.GRP)
    eng = engines.load(name, new=train, tag="train")
    d = eng.predict_draws(yrep=False, theta_new=False)
    assert d["ll"].tobytes() == eng.obs_ll_rows().tobytes()
    for rb, nr in WINDOWS:
        for nv in sc.N_VALID:
            parts, bad = eng.predict_partials_raw(rb, nr, nv)
            w = eng.waic_partials(rb, nr, nv)                           # [CB][5][n_obs]
            assert bad == (0, 0)
            for b in range(2):
                assert numpy.array_equal(_words(parts[b]["dens"]), _words(w[b][:3])), (rb, nr, nv, b)
    res = eng.predict()
    assert numpy.array_equal(_words(res.lpd_i), _words(eng.waic().lppd_i))
    assert res.n_response == sc.N_OBS and numpy.array_equal(res.group_codes, numpy.arange(sc.G))


# ---- 4. the reductions on the device's own draws and ll -------------------------------------
@pytest.mark.parametrize("name", pr.NAMES)
def test_reductions(engines, device_exp, name):
    s = pr.setup(name)
    d = engines.draws(name)
    eng = engines.load(name)
    y, has = s.new.y(s.resp), s.new.has_response(s.resp)
    worst = 0.0
    for rb, nr in WINDOWS:
        for nv in sc.N_VALID:
            what = "%s rows %d+%d n_valid %d" % (name, rb, nr, nv)
            parts, bad = eng.predict_partials_raw(rb, nr, nv)
            assert bad == (0, 0) and len(parts) == 2, what
            yr, ll = d["yrep"][:, rb:rb + nr], d["ll"][:, rb:rb + nr]
            want = pr.restate(yr, ll, y, sc.C, nv, exp=device_exp)
            S = nr * nv
            for b in range(2):
                _same(parts[b], want[b], "%s block %d" % (what, b), keys=("state", "count"))
                # dens: (m, s, n); rows without a response hold (-inf, NaN, n) on both sides
                for row in range(3):
                    g, w = parts[b]["dens"][row], want[b]["dens"][row]
                    assert numpy.array_equal(numpy.isnan(g), numpy.isnan(w)), (what, b, row)
                    assert numpy.array_equal(_words(g[has]), _words(w[has])), \
                        (what, b, row, int((_words(g[has]) != _words(w[has])).sum()))
                    assert numpy.array_equal(_words(g[~numpy.isnan(g)]),
                                             _words(w[~numpy.isnan(w)])), (what, b, row)
            merged = predict.merge(parts)
            worst = max(worst, pr.check(merged, pr.reference(yr, ll, y, nv), has, what))
            res = predict.finish(merged, s.new, s.resp)
            assert numpy.isnan(res.lpd_i[~has]).all() and numpy.isnan(res.pit_i[~has]).all()
            assert not merged["count"][:, :, ~has].any(), what
            assert res.n_samples == S and res.n_response == has.sum()
    print("predict reductions %s: worst err/tol = %.3g; dens, state and count word for word "
          "(%d calls of the device's exp so far)" % (name, worst, device_exp.calls))


# ---- 5. values that are not finite ----------------------------------------------------------
def test_nonfinite_new_groups(engines):
    s = pr.setup("benign")
    st = s.store.copy()
    s2 = lambda q: q * (sc.G + 2) + 1   # noqa: E731
    # (row, column, chain, value): <= 0 breaks both new groups of that sample, 1e-300 does not
    cells = [(2, s2(0), 5, 0.0), (3, s2(1), 66, -1.0), (sc.R - 1, s2(0), 64, 0.0),
             (4, s2(0), 7, 1e-300), (5, s2(1), 68, 1e-300)]
    for r, c, ch, v in cells:
        st[r, c, ch] = v
    isnew = s.new.group < 0
    has = s.new.has_response(s.resp)
    base = {}
    eng = engines.load("benign")
    for rb, nr in WINDOWS:
        for nv in sc.N_VALID:
            base[rb, nr, nv] = eng.predict_partials_raw(rb, nr, nv)[0]
    eng = engines.load("benign", store=st, tag="bad sigma2")
    d = eng.predict_draws()
    bad_s = numpy.zeros((sc.C, sc.R), dtype=bool)
    for r, c, ch, v in cells:
        bad_s[ch, r] |= not v > 0
    assert numpy.array_equal(numpy.isnan(d["theta_new"]).any(axis=(2, 3)), bad_s)
    assert numpy.array_equal(~numpy.isfinite(d["yrep"][..., 0]), bad_s[:, :, None] & isnew)
    seen = 0
    for rb, nr in WINDOWS:
        for nv in sc.N_VALID:
            parts, bad = eng.predict_partials_raw(rb, nr, nv)
            k = int(bad_s[:nv, rb:rb + nr].sum())
            assert bad == (k * int(isnew.sum()), k * int((isnew & has).sum())), (rb, nr, nv, bad)
            seen += k
            for b in range(2):      # the training groups keep their bits
                for key in ("dens", "state", "count"):
                    p, q = parts[b][key][..., ~isnew], base[rb, nr, nv][b][key][..., ~isnew]
                    assert p.tobytes() == q.tobytes(), (rb, nr, nv, b, key)
    print("predict nonfinite: %d broken samples counted over the windows" % seen)
    assert seen > 0
    with pytest.raises(_lib.NestmcError, match="not finite"):
        eng.predict()
    engines.load("benign")


def test_nonfinite_training_group(engines):
    case = sc.BY_NAME["sigma_bad"]
    s = pr.setup("sigma")
    has = s.new.has_response(s.resp)
    base = {}
    eng = engines.load("sigma")
    for rb, nr in WINDOWS:
        for nv in sc.N_VALID:
            base[rb, nr, nv] = eng.predict_partials_raw(rb, nr, nv)[0]
    eng = engines.load("sigma", store=case.store, tag="sigma_bad")
    seen = 0
    for rb, nr in WINDOWS:
        for nv in sc.N_VALID:
            parts, bad = eng.predict_partials_raw(rb, nr, nv)
            nd = nl = 0
            for c in case.bad:      # (store_cases.nonfinite_per_obs, on the new table's rows)
                if rb <= c.row < rb + nr and c.chain < nv:
                    rows = s.new.group == c.group
                    nd += int(rows.sum()) * (not c.value > 0)       # a draw needs sigma > 0
                    nl += int((rows & has).sum()) * (not c.value > 0 or c.value < 1e-200)
            assert bad == (nd, nl), (rb, nr, nv, bad, nd, nl)
            seen += nd + nl
            clean = ~numpy.isin(s.new.group, sc.touched_groups(case, rb, nr, nv))
            for b in range(2):
                for key in ("dens", "state", "count"):
                    p, q = parts[b][key][..., clean], base[rb, nr, nv][b][key][..., clean]
                    assert p.tobytes() == q.tobytes(), (rb, nr, nv, b, key)
    assert seen > 0
    engines.load("sigma")


# ---- 6. argument errors ---------------------------------------------------------------------
def test_bad_arguments(engines):
    eng = engines.load("benign")
    s = pr.setup("benign")
    for kw in (dict(n_rows=0), dict(row_begin=sc.R - 2, n_rows=3), dict(row_begin=-1, n_rows=2),
               dict(row_begin=sc.R, n_rows=1), dict(n_valid=0), dict(n_valid=sc.C + 1)):
        with pytest.raises(_lib.NestmcError):
            eng.predict_partials(**kw)
    for kw in (dict(row_begin=sc.R - 2, n_rows=3), dict(row_begin=-1, n_rows=2)):
        with pytest.raises(_lib.NestmcError):
            eng.predict_draws(**kw)
    i32 = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))   # noqa: E731
    g = s.new.group
    wide = numpy.zeros((pr.N_NEW, 3))
    too_big = numpy.where(g == 3, sc.G, g).astype(numpy.int32)
    for obs, nf, grp, K in ((wide, 3, g, 2), (s.new.obs, 2, too_big, 2), (s.new.obs, 2, g, 1)):
        assert eng.lib.nmc_predict_set(eng.h, dptr(obs), pr.N_NEW, nf, i32(grp), K) == -1
    before = eng.predict_partials()       # (a refused table changed nothing)
    _same(before[0], engines.load("benign", key="shard0", n_chains=64).predict_partials()[0], "kept")
    none = engines.load("sigma")
    assert none.lib.nmc_predict_set(none.h, dptr(s.new.obs), pr.N_NEW, 2, i32(g), 2) == -1
    with pytest.raises(ValueError, match="partial"):
        none.set_new_data(s.new)
    eng.set_new_data(None)
    with pytest.raises(ValueError, match="set_new_data"):
        eng.predict()
    assert eng.lib.nmc_predict_partials(eng.h, 0, 2, 1, None, None, None, None, None) == -1
    engines.holds.pop("benign")
    assert len(engines.load("benign").predict_partials()) == 2          # (the context still works)


# ---- 7. samplePosterior(predictFor=...) -----------------------------------------------------
def _new_table(G, seed=5):
    r = numpy.random.RandomState(seed)
    codes = numpy.array([0] * 5 + [1] * 9 + [-1] * 10 + [0] * 3, dtype=numpy.int32)
    x = r.normal(size=len(codes))
    y = 0.5 + 2.0 * x + r.normal(size=len(codes))
    y[::4] = numpy.nan
    return NewData(numpy.stack([x, y], 1), codes)


def test_sample_posterior_predict_for(gpu_lib, tmp_path):
    from nestmc.init import init_chains
    from nestmc.sampler import sample_posterior, schedule
    C, G, N = 8, 2, 12
    fam, sizes, priors, pooling, names = synthetic("linreg_partial", C, G, N)
    new = _new_table(G)
    ranges = {n: [-0.5, 0.5] for n in names}
    kw = dict(saveLogLikelihood=False, priorDistribution=priors, startingPointValueRange=ranges,
              displayProgress=False, seed=17, return_samples=True, write_files=True)
    out = str(tmp_path / "one")
    res = sample_posterior(C, 40, 10, names, G, N, pooling, fam, out, predictFor=new, **kw)
    r = res["predictions"]
    assert sorted(os.listdir(out)) == ["log", "prediction_groups.csv",
                                       "prediction_pointwise.csv", "sample"]
    back = predict.read_csvs(out)
    for k in ("y", "mean_i", "sd_i", "pit_i", "lt", "eq", "lpd_i", "group", "has_response",
              "group_codes", "elpd_g", "n_g"):
        assert numpy.array_equal(getattr(r, k), getattr(back, k), equal_nan=True), k
    assert (back.elpd_test, back.se, back.n_samples) == (r.elpd_test, r.se, r.n_samples)
    assert "elpd_test" in open(os.path.join(out, "log", "samplePosterior.log")).read()
    assert [predict.group_label(c) for c in r.group_codes] == ["0", "1", "new0"]
    # an Engine run of the same seed and start: its draws through the host route
    burn, thin = schedule(40, 10)
    eng = Engine(fam, sizes, C, pooling, priors, seed=17)
    try:
        st = init_chains(fam, sizes, names, list(range(C)), pooling, priors, ranges, False,
                         group_ll=eng.eval_group_ll)
        eng.set_state(st["value"], st["log_prior"], st["ll"], st["mu"], st["s2"])
        eng.set_schedule(40, burn, thin, 100)
        eng.run(0, 40)
        eng.synchronize()
        assert numpy.array_equal(eng.samples(), res["rows"])
        eng.set_new_data(new)
        d = eng.predict_draws()
        n_rows = eng.n_rows
    finally:
        eng.close()
    S = C * n_rows
    yrep, ll = d["yrep"].reshape(S, new.n_new, 1), d["ll"].reshape(S, new.n_new)
    assert r.n_samples == S
    host = predict.from_draws(yrep, ll, new.y([1]), new.group)
    has = r.has_response
    assert numpy.array_equal(r.lt, host.lt) and numpy.array_equal(r.eq, host.eq)
    assert numpy.array_equal(r.pit_i, host.pit_i, equal_nan=True)
    ref = pr.reference(d["yrep"], d["ll"], new.y([1]), C)
    tm, t2 = ppc_ref.tol_mean(S, ref["amax"]), ppc_ref.tol_m2(S, ref["sq"])
    tl = waic_ref.tol_lppd(ref["lpd"][has], S)

    def close(p, what):
        rm = _ratio(numpy.abs(p.mean_i.astype(LD) - ref["mean"]).astype(float), tm)
        r2 = _ratio(numpy.abs((p.sd_i.astype(LD) ** 2) * (S - 1) - ref["M2"]).astype(float), t2)
        rl = _ratio(numpy.abs(p.lpd_i.astype(LD) - ref["lpd"])[has].astype(float),
                    numpy.asarray(tl, dtype=float))
        print("predict %s: err/tol mean %.3g  M2 %.3g  lpd %.3g" % (what, rm, r2, rl))
        assert max(rm, r2, rl) <= 1.0, what

    close(r, "samplePosterior")
    close(host, "from_draws")
    # two engines on one GPU: 4 + 4 chains
    two = sample_posterior(C, 40, 10, names, G, N, pooling, fam, str(tmp_path / "two"),
                           predictFor=new, devices=[0, 0], **kw)
    assert numpy.array_equal(two["rows"], res["rows"])
    t = two["predictions"]
    assert numpy.array_equal(r.lt, t.lt) and numpy.array_equal(r.eq, t.eq)
    assert numpy.array_equal(r.has_response, t.has_response) and t.n_samples == S
    close(t, "devices=[0, 0]")
    # off by default
    off_ = sample_posterior(C, 40, 10, names, G, N, pooling, fam, str(tmp_path / "off"), **kw)
    assert "predictions" not in off_
    assert sorted(os.listdir(str(tmp_path / "off"))) == ["log", "sample"]
    # the refusals, before sampling starts
    no = str(tmp_path / "no")
    fn, sn, pn, pooln, nn = synthetic("regression3_none", C, G, N)
    with pytest.raises(ValueError, match="partial"):
        sample_posterior(C, 40, 10, nn, G, N, pooln, fn, no, priorDistribution=pn,
                         displayProgress=False, predictFor=new)
    with pytest.raises(ValueError, match="fields"):
        sample_posterior(C, 40, 10, names, G, N, pooling, fam, no, predictFor=NewData(
            numpy.zeros((3, 3)), [0, 1, 0]), **kw)
    assert not os.path.exists(no)


def test_process_per_device_rank_path(gpu_lib, tmp_path):
    """process_per_device with one rank: the rank reduces its chains, sends its merged partial
    over the host group and rank 0 finishes and writes -- the files are the in-process path's
    byte for byte."""
    from nestmc.sampler import sample_posterior
    C, G, N = 8, 2, 12
    fam, sizes, priors, pooling, names = synthetic("linreg_partial", C, G, N)
    kw = dict(saveLogLikelihood=False, priorDistribution=priors, predictFor=_new_table(G),
              startingPointValueRange={n: [-0.5, 0.5] for n in names}, displayProgress=False,
              seed=23, return_samples=True, devices=[0])
    one, ppd = str(tmp_path / "one"), str(tmp_path / "ppd")
    r1 = sample_posterior(C, 40, 10, names, G, N, pooling, fam, one, **kw)
    r2 = sample_posterior(C, 40, 10, names, G, N, pooling, fam, ppd, process_per_device=True,
                          **kw)
    assert numpy.array_equal(r1["rows"], r2["rows"])
    for fn in ("prediction_groups.csv", "prediction_pointwise.csv"):
        assert open(os.path.join(one, fn), "rb").read() == open(os.path.join(ppd, fn), "rb").read()
