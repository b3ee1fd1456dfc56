"""CPU: the stores of tests/store_cases.py are not vacuous, their references behave, and the
tolerances of tests/test_gpu_store_cases.py are held by float64 restatements alone -- before
any device runs.

* the spread stores force what they are named for (exp underflowing in the rescale, a maximum
  in the last valid lane, a maximum in padding only);
* waic_ref.restate, nmc_k_waic's arithmetic in float64, stays within Tol-lppd and the
  sharpened Tol-M2-sharp (tests/waic_ref.py) of the longdouble reference on every finite
  store, n_valid and window; three mutants of it each break a tolerance on a named store;
* the non-finite counts expected from the construction are those of the reference;
* the conv columns go through convergence_ref.partials, and the finite ones stay within
  TOL_MEAN, TOL_M2 and TOL_V of the longdouble formulas.

Every test prints its worst error / tolerance ratio (DESIGN section 4 records them).
"""

import warnings

import numpy
import pytest

import convergence_ref as cref
import psis_ref
import store_cases as sc
import waic_ref

WINDOWS = ((0, sc.R), (3, 1), (sc.R - 2, 2))


def _ll64(name):
    """The reference rounded to float64: what a correct device would hand the reduction."""
    return numpy.asarray(sc.ll_ref(name)[0], dtype=numpy.float64)


def test_geometry():
    assert sc.SIZES == [1, 7, 8, 9, 17] and sc.N_OBS == 42 and (sc.C, sc.R) == (70, 20)
    # group boundaries inside an 8-observation walk from observation 0: at 1 and 8
    assert list(sc.OFF[1:3]) == [1, 8]
    for c in sc.CASES:
        assert c.store.shape == (sc.R, c.cols, sc.C) and c.cols == c.P * (sc.G + c.pc)
        assert c.store.flags["C_CONTIGUOUS"] and c.store.dtype == numpy.float64
        assert c.fam.n_params == c.P and c.fam.obs().shape[0] == sc.N_OBS
        hyper = [k for k in range(c.cols) if k % (sc.G + c.pc) < c.pc]
        assert numpy.all(numpy.isfinite(c.store[:, hyper]))
    assert sc.BY_NAME["logistic"].fam.n_fields == 4 and sc.BY_NAME["gauss"].fam.n_fields == 3


def test_spread_stores_force_the_rescale():
    for name in sc.SPREAD:
        ll = _ll64(name)
        nv = sc.BY_NAME[name].n_valid[-1]
        spread = (ll[:nv].max(axis=(0, 1)) - ll[:nv].min(axis=(0, 1))).min()
        print("STORE %-12s least spread of an observation's ll %.1f" % (name, spread))
        assert spread > 1490.0, (name, spread)
    # ascending: new maxima row after row, and for every observation a step whose exp(-|d|)
    # is 0.0 in float64 (the s e + 1 branch with e underflown)
    ll = _ll64("ascending")
    run = numpy.maximum.accumulate(ll, axis=1)
    new = ll[:, 1:] > run[:, :-1]                       # [C][R-1][n_obs]
    under = new & (numpy.exp(-(ll[:, 1:] - run[:, :-1])) == 0.0)
    print("STORE ascending    new maxima per (chain, obs): min %d of %d; underflowing steps "
          "per observation: min %d" % (new.sum(axis=1).min(), sc.R - 1,
                                        under.sum(axis=(0, 1)).min()))
    assert new.sum(axis=1).min() >= sc.R // 2
    assert numpy.all(new[:, :, 0])                      # (the one-row group: every row)
    assert under.sum(axis=(0, 1)).min() >= sc.C // 2
    # descending: the maximum is on row 0 (or, where a residual outweighs the last steps of
    # delta, within two rows of it), and nothing after it is a new maximum
    am = _ll64("descending").argmax(axis=1)
    assert numpy.all(am <= 2) and numpy.all(am[:, 0] == 0) and (am == 0).mean() > 0.5
    # late_max: the maximum sits in the last valid lane, on the last row
    for nv in sc.N_VALID:
        ll = _ll64("late_max-%d" % nv)[:nv]
        flat = ll.reshape(-1, sc.N_OBS).argmax(axis=0)
        assert numpy.all(flat == (nv - 1) * sc.R + sc.R - 1), nv


def test_pad_max_has_its_maximum_in_padding_only():
    ll = _ll64("pad_max")
    for nv in sc.BY_NAME["pad_max"].n_valid:
        ref_valid = waic_ref.reference(sc.matrix(ll, n_valid=nv))[0]
        ref_all = waic_ref.reference(sc.matrix(ll))[0]
        gap = float((ref_all - ref_valid).min())
        print("STORE pad_max n_valid=%d: the valid chains' lppd lies %.1f below all chains'"
              % (nv, gap))
        assert gap > 1000.0


# ---- the restatement against the longdouble reference ---------------------------------------
@pytest.mark.parametrize("name", sc.FINITE)
def test_restatement_within_tolerances(name):
    ll = _ll64(name)
    assert numpy.all(numpy.isfinite(ll))
    worst_l = worst_m = 0.0
    for nv in sc.BY_NAME[name].n_valid:
        for rb, nr in WINDOWS:
            part = waic_ref.restate(ll[:, rb:rb + nr], sc.C, nv)
            rl, rm, _, _ = waic_ref.ratios(part, sc.matrix(ll, rb, nr, nv))
            worst_l, worst_m = max(worst_l, rl), max(worst_m, rm)
            # (the weakened Tol-M2 and the derived fields, as the existing tests ask)
            from nestmc import waic
            if nv * nr >= 2:
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    res = waic.finish(part, [0, sc.N_OBS])
                err = numpy.abs(res.p_waic_i.astype(numpy.longdouble) * (nv * nr - 1)
                                - waic_ref.reference(sc.matrix(ll, rb, nr, nv))[1])
                assert numpy.all(err <= (nv * nr + 64) * waic_ref.U
                                 * waic_ref.reference(sc.matrix(ll, rb, nr, nv))[2])
    print("RESTATE %-12s worst err/Tol-lppd %.3g  err/Tol-M2-sharp %.3g" % (name, worst_l, worst_m))
    assert worst_l <= 1.0 and worst_m <= 1.0, (name, worst_l, worst_m)


def _violation(name, mutant, nv):
    ll = _ll64(name)
    part = waic_ref.restate(ll, sc.C, nv, mutant=mutant)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        rl, rm, _, _ = waic_ref.ratios(part, sc.matrix(ll, n_valid=nv))
    return rl, rm


def test_mutants_break_the_tolerances():
    """Teeth: a naive one-pass variance on ``offset`` (Tol-M2-sharp; it passes the weakened
    Tol-M2), the recurrence without the rescale on ``ascending`` (Tol-lppd), a merge that
    does not treat n = 0 as empty on ``pad_max`` (Tol-lppd)."""
    _, rm = _violation("offset", "naive", 70)
    ll = _ll64("offset")
    part = waic_ref.restate(ll, sc.C, 70, mutant="naive")
    lppd, M2, sq, _ = waic_ref.reference(sc.matrix(ll))
    weak = float(numpy.max(numpy.abs(part[4].astype(numpy.longdouble) - M2)
                           / ((1400 + 64) * waic_ref.U * sq)))
    print("MUTANT naive variance on offset: err/Tol-M2-sharp %.3g (err/Tol-M2 %.3g)" % (rm, weak))
    assert rm > 1.0 and weak <= 1.0
    rl, _ = _violation("ascending", "norescale", 70)
    print("MUTANT no rescale on ascending: err/Tol-lppd %.3g" % rl)
    assert rl > 1.0
    rl, _ = _violation("pad_max", "n0", 65)
    print("MUTANT merge ignoring n = 0 on pad_max: err/Tol-lppd %.3g" % rl)
    assert rl > 1.0
    # and the restatement proper passes the same three
    for name, nv in (("offset", 70), ("ascending", 70), ("pad_max", 65)):
        rl, rm = _violation(name, None, nv)
        assert rl <= 1.0 and rm <= 1.0, (name, rl, rm)


def test_ties_are_exact():
    ll = _ll64("ties")
    assert numpy.all(ll == ll[0, 0][None, None, :])
    for nv in sc.N_VALID:
        for rb, nr in WINDOWS:
            m, s, n, mean, M2 = waic_ref.restate(ll[:, rb:rb + nr], sc.C, nv)
            assert numpy.all(M2 == 0.0) and numpy.all(s == float(nv * nr)), (nv, rb, nr)
            assert numpy.all(n == float(nv * nr))
            lppd = m + numpy.log(s / n)
            assert lppd.tobytes() == ll[0, 0].tobytes() and mean.tobytes() == ll[0, 0].tobytes()


# ---- non-finite terms ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", sc.NONFINITE)
def test_nonfinite_counts_follow_the_construction(name):
    case = sc.BY_NAME[name]
    ll = sc.ll_ref(name)[0]
    base = sc.ll_ref(case.base)[0]
    assert numpy.all(numpy.isfinite(base))
    assert numpy.isnan(ll).any() or name == "gauss_inf"
    assert numpy.isneginf(ll).any() and not numpy.isposinf(ll).any()
    for nv in sc.N_VALID:
        for rb, nr in WINDOWS:
            want = sc.nonfinite_per_obs(case, rb, nr, nv)
            got = (~numpy.isfinite(ll[:nv, rb:rb + nr])).sum(axis=(0, 1))
            assert numpy.array_equal(want, got), (name, nv, rb, nr)
            if nv in case.n_valid and (rb, nr) == (0, sc.R):
                print("STORE %-10s n_valid=%d: %d non-finite terms" % (name, nv, want.sum()))
    # observations of groups without an overwritten cell are those of the base store
    for g in set(range(sc.G)) - set(sc.touched_groups(case)):
        a, b = sc.OFF[g], sc.OFF[g + 1]
        assert numpy.array_equal(ll[:, :, a:b], base[:, :, a:b])
    if name == "sigma_pad":
        assert sc.nonfinite_per_obs(case, n_valid=65).sum() == 0
        assert sc.nonfinite_per_obs(case, n_valid=70).sum() > 0
        assert sc.touched_groups(case, n_valid=65) == []
    if name == "sigma_bad":     # the finite sigma = 1e300: ll = -log sqrt(2 pi) - log 1e300
        b = [x for x in case.bad if x.value == 1e300][0]
        v = ll[b.chain, b.row, sc.OFF[b.group]:sc.OFF[b.group + 1]]
        assert numpy.all(numpy.abs(v + 691.694) < 0.01)


# ---- the references against the families' own float64 callables -----------------------------
@pytest.mark.parametrize("name", ["benign", "offset", "sigma_bad", "logistic", "gauss",
                                  "gauss_inf"])
def test_reference_against_the_family_callable(name):
    """ll_ref against the family's numpy / scipy __call__ (float64) on every sixth sample and
    on the overwritten cells: within the unit the device is granted, non-finite alike."""
    case = sc.BY_NAME[name]
    ll, A = sc.ll_ref(name)
    th = sc.theta_of(case)
    pick = [(r, c) for r in range(sc.R) for c in range(sc.C) if (r * sc.C + c) % 6 == 0]
    pick += [(b.row, b.chain) for b in case.bad]
    worst = 0.0
    with numpy.errstate(all="ignore"):
        for r, c in pick:
            got = numpy.asarray(case.fam([th[r, c, q][sc.GRP] for q in range(case.P)]))
            ref, a = ll[c, r], A[c, r]
            fin = numpy.isfinite(ref)
            assert numpy.array_equal(numpy.isnan(ref), numpy.isnan(got)), (name, r, c)
            assert numpy.array_equal(numpy.isneginf(ref), numpy.isneginf(got)), (name, r, c)
            ratio = numpy.abs(got[fin].astype(sc.LD) - ref[fin]) / (sc.U * a[fin])
            worst = max(worst, float(ratio.max()) if fin.any() else 0.0)
    unit = sc.obs_ll_units(case.fam.n_fields)
    print("OBS_LL callable %-10s worst error %.3g of 2^-53 A (granted %d)" % (name, worst, unit))
    assert worst <= unit


def test_logistic_store_reaches_the_softplus_edges():
    ll = _ll64("logistic")
    first = ll[:, :, sc.OFF[:-1]]
    th = sc.theta_of(sc.BY_NAME["logistic"])
    for g in range(sc.G):
        assert set(sc.ETAS) <= set(th[:, :, 0, g].ravel()), g
    assert ll.max() == 0.0 and -800.5 < first.min() <= -800.0
    assert ll.min() > -900.0
    # every eta of the store is exact in float64: the fused and the unfused dot product agree
    case = sc.BY_NAME["logistic"]
    x = case.fam.obs()[:, :3]
    b = th[:, :, :, sc.GRP]                                 # [R][C][4][n]
    eta = b[:, :, 0].copy()
    for j in range(3):
        p = x[:, j] * b[:, :, j + 1]
        assert numpy.all(p.astype(sc.LD) == x[:, j].astype(sc.LD) * b[:, :, j + 1].astype(sc.LD))
        nxt = eta + p
        assert numpy.all(nxt.astype(sc.LD) == eta.astype(sc.LD) + p.astype(sc.LD))
        eta = nxt


@pytest.mark.parametrize("name", ["benign", "logistic"])
def test_psis_tolerances_hold_in_float64(name):
    """The stores Engine.loo_raw is checked on with psis_ref.check: the float64 evaluation of
    nestmc/loo.py's formulas stays within psis_ref's tolerances of the longdouble one."""
    ll = _ll64(name)
    worst = 0.0
    for i in range(sc.N_OBS):
        colv = numpy.ascontiguousarray(ll[:, :, i].T).reshape(-1)
        got = psis_ref.column(colv, numpy.float64)
        ref = psis_ref.check("%s/%d" % (name, i), colv, got["elpd"], got["lppd"], got["k"],
                             got["n_tail"], what="float64")
        tk, _, te, tl = psis_ref.tolerances(ref, len(colv))
        worst = max(worst, float(abs(got["elpd"] - ref["elpd"]) / te))
    print("PSIS float64 %-8s worst err/Tol-elpd %.3g" % (name, worst))


# ---- conv columns ---------------------------------------------------------------------------------
def test_conv_columns():
    st = sc.conv_store()
    assert st.shape == (sc.R, 14, sc.C)
    assert numpy.isposinf(st[:, 6]).sum() == 1 and numpy.isnan(st[:, 7]).sum() == 1
    assert numpy.signbit(st[:, 3]).any() and not numpy.signbit(st[:, 3]).all()
    assert numpy.all(numpy.abs(st[:, 4]) < 2.3e-308) and (st[:, 4] != 0).any()
    # the relative bounds assume no underflow: the denormal column is held to its own below
    finite = [k for k in range(14) if k not in sc.CONV_FLAGGED and k != 4]
    worst = dict(mean=0.0, m2=0.0, v=0.0)
    for rb, nr in sc.CONV_WINDOWS:
        rows = sc.conv_rows(st, rb, nr)
        n = nr // 2
        for nv in sc.N_VALID:
            with numpy.errstate(all="ignore"):
                vg, mean, m2 = cref.partials(rows, nv)
            assert vg.shape == (2, 14, n) and mean.shape == m2.shape == (14, 2, sc.C)
            x = cref.halves(rows[:nv])                      # [K][nv][2][n]
            with numpy.errstate(all="ignore"):
                f = cref.longdouble_formulas(x[finite].reshape(len(finite), nv * 2, n))
            mj = numpy.transpose(mean[finite][:, :, :nv], (0, 2, 1)).reshape(len(finite), -1)
            qj = numpy.transpose(m2[finite][:, :, :nv], (0, 2, 1)).reshape(len(finite), -1)
            tm = cref.tol_mean(f["absmean_j"], n)
            t2 = cref.tol_m2(f["M2_j"], f["absmean_j"], n)
            em, e2 = numpy.abs(mj - f["mean_j"]), numpy.abs(qj - f["M2_j"])
            assert numpy.all(em <= tm) and numpy.all(e2 <= t2), (rb, nr, nv)
            from nestmc import convergence
            V = convergence.merge(list(vg))[finite] / (
                numpy.float64(2 * nv) * numpy.maximum(n - numpy.arange(n), 1))
            tv = cref.tol_v_exact(f["V"], n, 2)
            ev = numpy.abs(V - f["V"])
            assert numpy.all(ev <= tv), (rb, nr, nv)
            with numpy.errstate(all="ignore"):
                for key, e, t in (("mean", em, tm), ("m2", e2, t2), ("v", ev, tv)):
                    r = numpy.where(t > 0, e / numpy.where(t > 0, t, 1), 0)
                    worst[key] = max(worst[key], float(r.max()))
            # flagged columns: NaN / inf where the construction puts them
            rin, cin = sc.CONV_INF_AT
            if rb <= rin < rb + nr and cin < nv:
                h = (rin - rb) // n
                assert numpy.isposinf(mean[6, h, cin]) and numpy.isnan(m2[6, h, cin])
            rna, cna = sc.CONV_NAN_AT
            if rb <= rna < rb + nr and cna < nv:
                h = (rna - rb) // n
                assert numpy.isnan(mean[7, h, cna]) and numpy.isnan(vg[0, 7, 1])
            assert numpy.isposinf(vg[0, 5, 1:]).all()       # (2e300)^2 overflows
            # denormals: the mean is the exact one rounded to the subnormal grid, every
            # square underflows to +0.0
            xd = cref.halves(rows[:nv])[4].astype(sc.LD)     # [nv][2][n]
            md = numpy.transpose(mean[4][:, :nv], (1, 0))
            assert numpy.all(numpy.abs(md - xd.sum(axis=2) / n) <= sc.LD(5e-324))
            assert not m2[4].any() and not vg[:, 4].any()
            assert numpy.all(numpy.isfinite(vg[:, sc.CONV_CLEAN]))
    print("CONV restatement against longdouble: worst err/TOL_MEAN %.3g  err/TOL_M2 %.3g  "
          "err/TOL_V %.3g" % (worst["mean"], worst["m2"], worst["v"]))
    # the constant column, as observed: the mean is (0.1 n) / n, which need not be 0.1
    rows = sc.conv_rows(st, 0, sc.R)
    from nestmc import convergence
    with numpy.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        vg, mean, m2 = cref.partials(rows)
        res = convergence.finish(convergence.merge(list(vg)), mean, m2, sc.R // 2,
                                 ["c%d" % k for k in range(14)])
    print("CONV constant column 0.1, n = 10: mean == 0.1: %s, M2 = %r, rhat = %r"
          % (bool(numpy.all(mean[2] == 0.1)), float(m2[2].max()), float(res.rhat[2])))
