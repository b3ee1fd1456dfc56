"""The sample store's consumers on stores written by the test (tests/store_cases.py).

Every test builds an engine, sizes the store with set_schedule, never samples, writes the rows
with Engine.set_samples_raw (nmc_debug_set_samples) and calls the consumers: obs_ll_rows and
the LL files, nmc_k_waic, nmc_k_loo_ll + PSIS, nmc_k_conv.  The references, the expected
non-finite counts and the tolerances are those tests/test_store_cases.py holds on the CPU:

* obs_ll_rows against store_cases.ll_ref (numpy.longdouble, the family's formula) on every
  (chain, row, observation): finite terms within 4 (nf + 4) 2^-53 A, NaN where the reference
  has NaN, -inf where it has -inf;
* WAIC against the longdouble reference over the device's own log-likelihoods within Tol-lppd
  and Tol-M2-sharp (tests/waic_ref.py), and against waic_ref.restate of the same
  log-likelihoods.  The restatement repeats the kernel's float64 operations in the kernel's
  order, so m, n, mean and M2 -- IEEE additions, multiplications and divisions only -- must
  be its words bit for bit.  s passes through exp, numpy's there and the device library's
  here, each within an ulp of the exact value and not of each other: for lppd the bar is
  twice Tol-lppd (both sides hold it against the same reference), not bit identity.  The
  count of identical words is printed;
* LOO against nmc_psis_of over the transposed obs_ll_rows, bit for bit;
* conv_partials against convergence_ref.partials word for word (NaN compared as NaN: the sign
  of inf - inf differs between x86 and the device).

Every test prints its worst error / tolerance ratio.
"""

import ctypes
import os

import numpy
import pytest

import convergence_ref as cref
import psis_ref
import store_cases as sc
import user_models
import waic_ref
from nestmc import _lib, waic
from nestmc.engine import Engine
from nestmc.families import DeviceLikelihood

pytestmark = pytest.mark.gpu

WINDOWS = ((0, sc.R), (3, 1), (sc.R - 2, 2))


class Engines:
    """One engine per family object, made on first use; ``load`` writes a case's store unless
    it is the one the engine holds."""

    def __init__(self):
        self.eng, self.holds, self.ll = {}, {}, {}

    def get(self, case, fam=None, key=None):
        key = key or (case.kind, case.name == "offset")
        if key not in self.eng:
            e = Engine(fam or case.fam, sc.SIZES, sc.C, case.pooling, case.priors, seed=1)
            e.set_schedule(sc.R, 0, 1)             # R recorded rows; no run()
            assert (e.n_rows, e.cols) == (sc.R, case.cols)
            self.eng[key] = e
        return key, self.eng[key]

    def load(self, name, fam=None, key=None):
        case = sc.BY_NAME[name]
        key, e = self.get(case, fam, key)
        if self.holds.get(key) != name:
            e.set_samples_raw(case.store)
            self.holds[key] = name
        return e

    def dev_ll(self, name):
        """The device's own obs_ll_rows of a case's store, [C][R][n_obs], computed once."""
        if name not in self.ll:
            self.ll[name] = self.load(name).obs_ll_rows()
            self.ll[name].setflags(write=False)
        return self.ll[name]

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


def _same_words_nan(a, b):
    """Word for word, a NaN equal to any NaN."""
    a, b = numpy.asarray(a, dtype=numpy.float64), numpy.asarray(b, dtype=numpy.float64)
    na, nb = numpy.isnan(a), numpy.isnan(b)
    return a.shape == b.shape and numpy.array_equal(na, nb) and \
        numpy.array_equal(_words(a)[~na], _words(b)[~nb])


def _waic_parts(eng, rb, nr, nv):
    """nmc_waic_partials itself (Engine.waic_partials raises on non-finite terms):
    (parts [CB, 5, n_obs], the non-finite count)."""
    out = numpy.full(((eng.C + 63) // 64, 5, sc.N_OBS), -7.0)
    bad = ctypes.c_int64(-7)
    _lib.check(eng.lib.nmc_waic_partials(eng.h, rb, nr, nv, _lib.dptr(out), ctypes.byref(bad)))
    return out, bad.value


# ---- the hook ---------------------------------------------------------------------------------------
def test_hook_round_trip_window_and_errors(engines):
    case = sc.BY_NAME["benign"]
    _, eng = engines.get(case)
    r = numpy.random.RandomState(9)
    x = r.normal(size=(sc.R, case.cols, sc.C))
    x[0, 0, 0], x[3, 5, 69], x[sc.R - 1, 13, 64] = -0.0, numpy.nan, -numpy.inf
    x[7, 2, 1] = numpy.float64(5e-324)
    eng.set_samples_raw(x)
    engines.holds.clear()
    got = eng.samples_raw()
    assert got.tobytes() == x.tobytes()
    assert numpy.signbit(got[0, 0, 0]) and numpy.isnan(got[3, 5, 69])
    w = r.normal(size=(4, case.cols, sc.C))
    eng.set_samples_raw(w, row_begin=5)
    want = x.copy()
    want[5:9] = w
    assert eng.samples_raw().tobytes() == want.tobytes()
    assert eng.samples_raw(5, 4).tobytes() == w.tobytes()
    eng.set_samples_raw(w[:0], row_begin=sc.R)              # (no rows: nothing written)
    assert eng.samples_raw().tobytes() == want.tobytes()
    for rb, nr in ((-1, 2), (sc.R - 1, 2), (0, sc.R + 1), (sc.R + 1, 0), (2, -1)):
        buf = numpy.zeros((max(nr, 1), case.cols, sc.C))
        rc = eng.lib.nmc_debug_set_samples(eng.h, rb, nr, _lib.dptr(buf))
        assert rc == -1 and b"row range out of bounds" in eng.lib.nmc_last_error(), (rb, nr)
    with pytest.raises(_lib.NestmcError):
        eng.set_samples_raw(w, row_begin=sc.R - 3)
    for bad in (w[:, :-1], w[:, :, :-1], w[0], w.astype(numpy.float32),
                numpy.asfortranarray(w), w.tolist()):
        with pytest.raises(ValueError):
            eng.set_samples_raw(bad)
    assert eng.samples_raw().tobytes() == want.tobytes()    # (the context still works)
    assert eng.obs_ll_rows().shape == (sc.C, sc.R, sc.N_OBS)


# ---- obs_ll_rows -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sc.NAMES)
def test_obs_ll_rows_against_longdouble(engines, name):
    case = sc.BY_NAME[name]
    got = engines.dev_ll(name)
    ref, A = sc.ll_ref(name)
    assert got.shape == ref.shape == (sc.C, sc.R, sc.N_OBS)
    assert numpy.array_equal(numpy.isnan(got), numpy.isnan(ref)), name
    assert numpy.array_equal(numpy.isneginf(got), numpy.isneginf(ref)), name
    assert not numpy.isposinf(got).any()
    fin = numpy.isfinite(ref)
    ratio = numpy.abs(got[fin].astype(sc.LD) - ref[fin]) / (sc.U * A[fin])
    unit = sc.obs_ll_units(case.fam.n_fields)
    print("OBS_LL %-12s worst error %.3g of 2^-53 A (granted %d); %d finite, %d NaN, %d -inf"
          % (name, float(ratio.max()), unit, fin.sum(), numpy.isnan(ref).sum(),
             numpy.isneginf(ref).sum()))
    assert float(ratio.max()) <= unit, name
    # windows read the same words
    assert engines.load(name).obs_ll_rows(3, 4).tobytes() == \
        numpy.ascontiguousarray(got[:, 3:7]).tobytes()


# ---- WAIC ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sc.FINITE)
def test_waic_on_finite_stores(engines, name):
    case = sc.BY_NAME[name]
    ll = engines.dev_ll(name)
    eng = engines.load(name)
    wl = wm = dl = 0.0
    same = total = 0
    for nv in case.n_valid:
        for rb, nr in WINDOWS:
            parts, bad = _waic_parts(eng, rb, nr, nv)
            assert bad == 0, (name, nv, rb, nr)
            if nv == 64:
                assert parts[1].tobytes() == waic.identity(sc.N_OBS).tobytes()
            got = waic.merge(list(parts))
            mat = sc.matrix(ll, rb, nr, nv)
            rl, rm, _, _ = waic_ref.ratios(got, mat)
            wl, wm = max(wl, rl), max(wm, rm)
            assert rl <= 1.0 and rm <= 1.0, (name, nv, rb, nr, rl, rm)
            # against the restatement of the same log-likelihoods
            rs = waic_ref.restate(ll[:, rb:rb + nr], sc.C, nv)
            # m, n, mean and M2 never pass through exp: those words are the restatement's
            for f, what in ((0, "m"), (2, "n"), (3, "mean"), (4, "M2")):
                assert got[f].tobytes() == rs[f].tobytes(), (name, nv, rb, nr, what)
            lppd = waic_ref.reference(mat)[0]
            S = nv * nr
            e_l = numpy.abs((got[0] + numpy.log(got[1] / S)) - (rs[0] + numpy.log(rs[1] / S)))
            t_l = 2 * waic_ref.tol_lppd(lppd, S)
            assert numpy.all(e_l <= t_l), (name, nv, rb, nr)
            dl = max(dl, float(numpy.max(e_l / t_l)))
            same += int(numpy.sum(_words(got) == _words(rs)))
            total += got.size
            if S >= 2 and (rb, nr) == (0, sc.R):
                waic_ref.check(waic.finish(got, eng.off), mat, what="%s n_valid %d" % (name, nv))
    print("WAIC %-12s device vs longdouble: err/Tol-lppd %.3g err/Tol-M2-sharp %.3g; vs the "
          "restatement: lppd within %.3g of twice Tol-lppd, m / n / mean / M2 identical, %d of "
          "%d words identical" % (name, wl, wm, dl, same, total))


def test_waic_ties_exact(engines):
    ll = engines.dev_ll("ties")
    assert numpy.all(ll == ll[0, 0][None, None, :])
    eng = engines.load("ties")
    for nv in sc.N_VALID:
        for rb, nr in WINDOWS:
            parts, bad = _waic_parts(eng, rb, nr, nv)
            m, s, n, mean, M2 = waic.merge(list(parts))
            assert bad == 0 and numpy.all(M2 == 0.0) and numpy.all(s == float(nv * nr))
            if nv * nr >= 2:
                res = waic.finish(waic.merge(list(parts)), eng.off)
                assert numpy.all(res.p_waic_i == 0.0), (nv, rb, nr)
                assert res.lppd_i.tobytes() == ll[0, 0].tobytes(), (nv, rb, nr)


@pytest.mark.parametrize("name", sc.NONFINITE)
def test_waic_nonfinite_counts_and_untouched_groups(engines, name):
    case = sc.BY_NAME[name]
    base = engines.load(case.base)
    clean = {(nv, w): _waic_parts(base, w[0], w[1], nv) for nv in case.n_valid for w in WINDOWS}
    eng = engines.load(name)
    for (nv, (rb, nr)), (want, bad0) in clean.items():
        assert bad0 == 0
        parts, bad = _waic_parts(eng, rb, nr, nv)
        expect = int(sc.nonfinite_per_obs(case, rb, nr, nv).sum())
        assert bad == expect, (name, nv, rb, nr, bad, expect)
        touched = sc.touched_groups(case, rb, nr, nv)
        for g in range(sc.G):
            a, b = sc.OFF[g], sc.OFF[g + 1]
            if g not in touched:   # (cells in padding chains or outside the window: no word)
                assert parts[:, :, a:b].tobytes() == want[:, :, a:b].tobytes(), (name, nv, rb, g)
        print("WAIC %-10s n_valid=%d rows %d+%d: %d non-finite terms, groups touched %s"
              % (name, nv, rb, nr, bad, touched))
    if name == "sigma_pad":
        assert all(sc.touched_groups(case, 0, sc.R, nv) == [] for nv in case.n_valid)


# ---- LOO -------------------------------------------------------------------------------------------------
def _psis_of(lib, store, n_valid, obs_batch=0):
    x = numpy.ascontiguousarray(store, dtype=numpy.float64)
    rows, n, C = x.shape
    elpd, lppd, k = (numpy.full(n, -7.0) for _ in range(3))
    nt = numpy.full(n, -7, dtype=numpy.int32)
    bad = numpy.full(n, -7, dtype=numpy.int64)
    _lib.check(lib.nmc_psis_of(0, _lib.dptr(x), rows, n, C, n_valid, obs_batch, _lib.dptr(elpd),
                               _lib.dptr(lppd), _lib.dptr(k),
                               nt.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                               bad.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))))
    return dict(elpd=elpd, lppd=lppd, k=k, n_tail=nt, nonfinite=bad)


def _same_loo(a, b):
    return all(_same_words_nan(a[f], b[f]) for f in ("elpd", "lppd", "k")) and \
        numpy.array_equal(a["n_tail"], b["n_tail"]) and \
        numpy.array_equal(a["nonfinite"], b["nonfinite"])


@pytest.mark.parametrize("name", sc.NAMES)
def test_loo_equals_psis_of_the_ll_rows(engines, name):
    case = sc.BY_NAME[name]
    ll = engines.dev_ll(name)
    eng = engines.load(name)
    for nv in case.n_valid:
        for rb, nr in ((0, sc.R), (sc.R - 2, 2)):
            store = numpy.ascontiguousarray(numpy.transpose(ll[:, rb:rb + nr], (1, 2, 0)))
            want = _psis_of(eng.lib, store, nv)
            expect = sc.nonfinite_per_obs(case, rb, nr, nv)
            assert numpy.array_equal(want["nonfinite"], expect), (name, nv, rb)
            for b in (0, 1, 5, 8, 9):
                got = eng.loo_raw(rb, nr, nv, obs_batch=b)
                assert numpy.array_equal(got["nonfinite"], expect), (name, nv, rb, b)
                assert _same_loo(got, want), (name, nv, rb, b)
            assert numpy.all(numpy.isnan(want["elpd"][expect > 0]))
    print("LOO %-12s equals nmc_psis_of of obs_ll_rows for n_valid %s, obs_batch 0, 1, 5, 8, 9; "
          "%d non-finite terms" % (name, list(case.n_valid), int(expect.sum())))


@pytest.mark.parametrize("name", ["benign", "logistic"])
def test_loo_against_longdouble(engines, name):
    ll = engines.dev_ll(name)
    got = engines.load(name).loo_raw()
    for i in range(sc.N_OBS):
        col = numpy.ascontiguousarray(ll[:, :, i].T).reshape(-1)      # s = row * C + chain
        psis_ref.check("store-%s/%d" % (name, i), col, got["elpd"][i], got["lppd"][i],
                       got["k"][i], got["n_tail"][i], what="device")
    assert not got["nonfinite"].any()


# ---- a run-time-compiled user family ---------------------------------------------------------------
def test_user_logistic_word_identical_to_builtin(engines):
    """user_models.LOGISTIC4 forms eta as an fma chain, FamLogistic::obs_ll term by term; on
    the logistic store every product and partial sum of eta is exact (store_cases), so the two
    are the same numbers and every consumer must give the same words."""
    case = sc.BY_NAME["logistic"]
    user = DeviceLikelihood(case.fam.obs(), user_models.LOGISTIC4, 4, host_function=case.fam)
    a = engines.dev_ll("logistic")
    ea = engines.load("logistic")
    eb = engines.load("logistic", fam=user, key="user-logistic")
    assert eb.obs_ll_rows().tobytes() == a.tobytes()
    for nv in sc.N_VALID:
        pa, ba = _waic_parts(ea, 0, sc.R, nv)
        pb, bb = _waic_parts(eb, 0, sc.R, nv)
        assert pa.tobytes() == pb.tobytes() and ba == bb == 0
        la, lb = ea.loo_raw(n_valid=nv, obs_batch=5), eb.loo_raw(n_valid=nv, obs_batch=5)
        assert all(la[f].tobytes() == lb[f].tobytes()
                   for f in ("elpd", "lppd", "k", "n_tail", "nonfinite"))


# ---- the LL files --------------------------------------------------------------------------------------
def test_ll_files_with_nan_and_inf(engines, tmp_path):
    ll = engines.dev_ll("sigma_bad")
    eng = engines.load("sigma_bad")
    ids = list(range(200, 200 + sc.C))
    eng.write_ll_csvs(str(tmp_path), ids, threads=4)
    seen = set()
    for c in (3, 10, 63, 64):          # sigma 0 (NaN), -1 (NaN), 1e-300 (-inf), 1e300 and -1
        text = open(os.path.join(str(tmp_path), "logLikelihood.%d.csv" % ids[c]), "rb").read()
        want = "".join(",".join("%f" % v for v in ll[c, r]) + "\n" for r in range(sc.R))
        assert text == want.encode(), c
        seen |= {t for t in ("nan", "-inf") if t in want}
    assert seen == {"nan", "-inf"}


# ---- conv --------------------------------------------------------------------------------------------------
def test_conv_partials_on_hard_columns(engines):
    case = sc.BY_NAME["benign"]
    key, eng = engines.get(case)
    st = sc.conv_store()
    eng.set_samples_raw(numpy.array(st))
    engines.holds[key] = "conv"
    # (the relative bounds assume no underflow: the denormal column, 4, is held word for word
    # to the restatement, which test_store_cases.py holds to the subnormal grid)
    finite = [k for k in range(14) if k not in sc.CONV_FLAGGED and k != 4]
    worst = dict(mean=0.0, m2=0.0, v=0.0)
    for rb, nr in sc.CONV_WINDOWS:
        rows = sc.conv_rows(st, rb, nr)
        n = nr // 2
        for nv in sc.N_VALID:
            with numpy.errstate(all="ignore"):
                want = cref.partials(rows, nv)
            got = eng.conv_partials(rb, nr, nv)
            for w, g, what in zip(want, got, ("vg", "mean", "m2")):
                assert _same_words_nan(g, w), (what, rb, nr, nv,
                                               numpy.argwhere(_words(g) != _words(w))[:5])
            # the finite columns against the longdouble formulas
            vg, mean, m2 = got
            x = cref.halves(rows[:nv])
            with numpy.errstate(all="ignore"):
                f = cref.longdouble_formulas(x[finite].reshape(len(finite), nv * 2, n))
            mj = numpy.transpose(mean[finite][:, :, :nv], (0, 2, 1)).reshape(len(finite), -1)
            qj = numpy.transpose(m2[finite][:, :, :nv], (0, 2, 1)).reshape(len(finite), -1)
            V = (vg[0] + vg[1])[finite] / (numpy.float64(2 * nv)
                                          * numpy.maximum(n - numpy.arange(n), 1))
            for keyw, e, t in (
                    ("mean", numpy.abs(mj - f["mean_j"]), cref.tol_mean(f["absmean_j"], n)),
                    ("m2", numpy.abs(qj - f["M2_j"]), cref.tol_m2(f["M2_j"], f["absmean_j"], n)),
                    ("v", numpy.abs(V - f["V"]), cref.tol_v_exact(f["V"], n, 2))):
                assert numpy.all(e <= t), (keyw, rb, nr, nv)
                r = numpy.where(t > 0, e / numpy.where(t > 0, t, 1), 0)
                worst[keyw] = max(worst[keyw], float(r.max()))
    print("CONV device against longdouble: worst err/TOL_MEAN %.3g err/TOL_M2 %.3g err/TOL_V %.3g"
          % (worst["mean"], worst["m2"], worst["v"]))


def test_convergence_clean_column_unmoved_by_flagged_ones(engines):
    case = sc.BY_NAME["benign"]
    key, eng = engines.get(case)
    out = {}
    for replaced in (False, True):
        eng.set_samples_raw(numpy.array(sc.conv_store(replaced)))
        engines.holds[key] = "conv"
        for rb, nr in sc.CONV_WINDOWS:
            for nv in sc.N_VALID:
                with numpy.errstate(all="ignore"):
                    res = eng.convergence(None, rb, nr, nv)
                k = sc.CONV_CLEAN
                out[replaced, rb, nr, nv] = (res.rhat[k], res.effective_n[k], res.mean[k],
                                             res.sd[k], res.T[k]) + tuple(res.V[k])
                if not replaced and (rb, nr) == (0, sc.R):
                    print("CONV n_valid=%d constant column 0.1: rhat %r; clean column: rhat %r"
                          % (nv, float(res.rhat[2]), float(res.rhat[k])))
    for (replaced, rb, nr, nv), v in out.items():
        if not replaced:
            w = out[True, rb, nr, nv]
            assert _words(numpy.array(v)).tobytes() == _words(numpy.array(w)).tobytes(), \
                (rb, nr, nv)
            assert numpy.all(numpy.isfinite(v))
