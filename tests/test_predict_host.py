"""Held-out and new-group prediction on the host (nestmc/predict.py) and the references the
device tests use (tests/predict_ref.py).  Runs without a GPU.

* predict_ref.restate (nmc_k_predict's float64 arithmetic) against predict_ref.reference
  (longdouble) on the reference draws and log densities of every case: counts equal, mean and
  M2 within ppc_ref.tol_mean / tol_m2, lpd within waic_ref.tol_lppd;
* the logistic case keeps every uniform 1e-12 away from its probability; the new groups'
  normals have mean 0 and variance 1 and do not repeat the draws' stream;
* merge: the identity, the order, shape errors; finish against from_draws; the CSV round trip;
* NewData's validation and every ValueError of sample_posterior that needs no device.
"""

import os

import numpy
import pytest

import predict_ref as pr
import store_cases as sc
from nestmc import NewData, predict
from nestmc.sampler import sample_posterior

WINDOWS = ((0, sc.R), (3, 1), (sc.R - 2, 2))


def _y(s):
    return s.new.y(s.resp)


@pytest.mark.parametrize("name", pr.NAMES)
def test_restatement_against_longdouble(name):
    s = pr.setup(name)
    h = pr.host(name)
    y, has = _y(s), s.new.has_response(s.resp)
    assert has.sum() == pr.N_NEW - pr.NO_RESP.sum() and not has[pr.NO_RESP].any()
    worst = 0.0
    for rb, nr in WINDOWS:
        for nv in sc.N_VALID:
            what = "%s rows %d+%d n_valid %d" % (name, rb, nr, nv)
            yr, ll = h["yrep64"][:, rb:rb + nr], h["ll64"][:, rb:rb + nr]
            parts = pr.restate(yr, ll, y, sc.C, nv)
            assert len(parts) == 2
            # the density restatement with numpy's exp is waic_ref.restate_parts' (m, s, n)
            assert numpy.array_equal(numpy.stack([p["dens"] for p in parts]),
                                     pr.waic_ref.restate_parts(ll, sc.C, nv)[:, :3],
                                     equal_nan=True), what
            merged = predict.merge(parts)
            worst = max(worst, pr.check(merged, pr.reference(yr, ll, y, nv), has, what))
            # no response: no counts, and NaN in the density state
            assert not merged["count"][:, :, ~has].any(), what
            assert numpy.isnan(merged["dens"][1][~has]).all(), what
            if nv == 64:   # the second block is padding only: the identity
                ident = predict.identity(pr.N_NEW, len(s.resp))
                for k in ("dens", "state", "count"):
                    assert numpy.asarray(parts[1][k]).tobytes() == ident[k].tobytes(), (what, k)
    print("predict restatement %s: worst err/tol = %.3g" % (name, worst))


def test_logistic_uniforms_stay_clear_of_the_probabilities():
    gap = pr.host("logistic")["gap"]
    print("predict logistic: min |ua - p| = %.3g" % gap.min())
    assert gap.min() > 1e-12


def test_new_group_stream():
    th, tol, z = pr.theta_new_ref("benign")
    assert z.shape == (sc.C, sc.R, 2, 2) and th.shape == z.shape
    assert abs(z.mean()) < 4 / numpy.sqrt(z.size) and abs(z.var() - 1) < 0.1
    assert len(numpy.unique(z)) == z.size
    assert numpy.isfinite(numpy.asarray(th, dtype=float)).all() and (tol > 0).all()
    # all observations of a new group share theta within a sample; the draws differ
    h = pr.host("benign")
    rows = pr.theta_rows("benign", h["theta_new"])
    new0 = numpy.flatnonzero(pr.CODES == -1)
    assert numpy.array_equal(rows[..., new0[0]], rows[..., new0[-1]])
    assert not numpy.array_equal(h["yrep64"][:, :, new0[0]], h["yrep64"][:, :, new0[1]])
    # a sigma2 that is not > 0, or not finite, gives NaN
    st = pr.setup("benign").store.copy()
    st[2, 1, 5], st[3, 8, 6], st[4, 1, 7] = 0.0, -1.0, numpy.inf
    bad = numpy.isnan(numpy.asarray(pr.theta_new_ref("benign", store=st)[0], dtype=float))
    assert bad.sum() == 6 and bad[5, 2, :, 0].all() and bad[6, 3, :, 1].all() \
        and bad[7, 4, :, 0].all()


def _parts(name="gauss"):
    s, h = pr.setup(name), pr.host(name)
    return s, pr.restate(h["yrep64"], h["ll64"], _y(s), sc.C, sc.C)


def test_merge_identity_order_and_shapes():
    s, parts = _parts()
    ident = predict.identity(pr.N_NEW, len(s.resp))
    whole = predict.merge(parts)
    for seq in ([ident] + parts, parts + [ident], [parts[0], ident, parts[1]]):
        got = predict.merge(seq)
        for k in ("dens", "state", "count"):
            assert got[k].tobytes() == whole[k].tobytes(), k
    assert whole["count"].dtype == numpy.int64
    swapped = predict.merge(parts[::-1])
    assert numpy.array_equal(swapped["count"], whole["count"])
    assert numpy.allclose(swapped["state"], whole["state"], rtol=1e-12, atol=1e-12)
    assert swapped["state"].tobytes() != whole["state"].tobytes()      # the order is in the bits
    assert predict.unpack(predict.pack(whole))["dens"].tobytes() == whole["dens"].tobytes()
    assert predict.merge_ranks([parts[0], parts[1]])["state"].tobytes() == whole["state"].tobytes()
    with pytest.raises(ValueError):
        predict.merge([])
    with pytest.raises(ValueError):
        predict.merge([parts[0], predict.identity(pr.N_NEW + 1, len(s.resp))])
    with pytest.raises(ValueError):
        predict.merge([parts[0], predict.identity(pr.N_NEW, 1)])
    bad = dict(parts[0], nonfinite_draws=2, nonfinite_ll=3)
    m = predict.merge([bad, parts[1]])
    assert (m["nonfinite_draws"], m["nonfinite_ll"]) == (2, 3)


@pytest.mark.parametrize("name", ["benign", "gauss", "logistic"])
def test_finish_against_from_draws(name):
    s, parts = _parts(name)
    h = pr.host(name)
    res = predict.finish(predict.merge(parts), s.new, s.resp)
    S = sc.C * sc.R
    yr = h["yrep64"].reshape(S, pr.N_NEW, -1)
    ll = h["ll64"].reshape(S, pr.N_NEW)
    direct = predict.from_draws(yr, ll, _y(s), s.new.group)
    has = res.has_response
    assert res.n_samples == direct.n_samples == S and res.n_response == has.sum()
    assert numpy.array_equal(res.lt, direct.lt) and numpy.array_equal(res.eq, direct.eq)
    assert numpy.array_equal(res.pit_i, direct.pit_i, equal_nan=True)
    assert numpy.isnan(res.pit_i[~has]).all() and numpy.isnan(res.lpd_i[~has]).all()
    assert not res.lt[~has].any() and not res.eq[~has].any()
    # both routes within the reductions' tolerances of the longdouble reference
    ref = pr.reference(h["yrep64"], h["ll64"], _y(s), sc.C)
    LD = pr.LD
    for r in (res, direct):
        assert numpy.all(numpy.abs(r.mean_i.astype(LD) - ref["mean"])
                         <= pr.ppc_ref.tol_mean(S, ref["amax"]))
        assert numpy.all(numpy.abs((r.sd_i.astype(LD) ** 2) * (S - 1) - ref["M2"])
                         <= pr.ppc_ref.tol_m2(S, ref["sq"]))
        assert numpy.all(numpy.abs(r.lpd_i.astype(LD) - ref["lpd"])[has]
                         <= pr.waic_ref.tol_lppd(ref["lpd"][has], S))
    assert numpy.isclose(res.elpd_test, direct.elpd_test, rtol=1e-12)
    v = res.lpd_i[has]
    assert res.elpd_test == float(numpy.sum(v))
    assert res.se == float(numpy.sqrt(len(v) * numpy.var(v, ddof=1)))
    codes = [int(c) for c in res.group_codes]
    assert codes == sorted(set(int(c) for c in s.new.group), key=lambda c: (c < 0, abs(c)))
    for c, e, n in zip(codes, res.elpd_g, res.n_g):
        sel = has & (s.new.group == c)
        assert n == sel.sum() and e == numpy.sum(res.lpd_i[sel])
    assert numpy.isclose(res.elpd_g.sum(), res.elpd_test, rtol=1e-12)
    assert "elpd_test" in repr(res)
    with pytest.raises(ValueError, match="two samples"):
        predict.from_draws(yr[:1], ll[:1], _y(s))
    one = pr.restate(h["yrep64"][:1, :1], h["ll64"][:1, :1], _y(s), 1, 1)
    with pytest.raises(ValueError, match="two samples"):
        predict.finish(predict.merge(one), s.new, s.resp)


@pytest.mark.parametrize("name", ["benign", "gauss"])
def test_csv_round_trip(name, tmp_path):
    s, parts = _parts(name)
    res = predict.finish(predict.merge(parts), s.new, s.resp)
    predict.write_csvs(res, str(tmp_path))
    assert sorted(os.listdir(str(tmp_path))) == ["prediction_groups.csv",
                                                 "prediction_pointwise.csv"]
    back = predict.read_csvs(str(tmp_path))
    for k in ("y", "mean_i", "sd_i", "pit_i", "lt", "eq", "lpd_i", "group", "has_response",
              "group_codes", "elpd_g", "n_g"):
        assert numpy.array_equal(getattr(res, k), getattr(back, k), equal_nan=True), k
    assert (back.elpd_test, back.se, back.n_samples) == (res.elpd_test, res.se, res.n_samples)
    lines = open(str(tmp_path / "prediction_groups.csv")).read().splitlines()
    assert lines[1].startswith("all,") and len(lines) == 2 + len(res.group_codes)
    if name == "benign":
        assert [ln.split(",")[0] for ln in lines[2:]] == ["0", "1", "3", "new0", "new1"]


def test_a_family_that_cannot_draw_has_the_density_alone(tmp_path):
    s, h = pr.setup("poisson"), pr.host("poisson")
    new = NewData(s.new.obs, s.new.group)
    assert new.has_response([]).all()            # (no response field named: every row counts)
    parts = pr.restate(h["yrep64"][..., :0], h["ll64"], new.y([]), sc.C, sc.C)
    res = predict.finish(predict.merge(parts), new, [])
    assert res.mean_i.shape == (pr.N_NEW, 0) and res.n_response == pr.N_NEW
    assert numpy.isfinite(res.lpd_i[~pr.NO_RESP]).all()
    predict.write_csvs(res, str(tmp_path))
    back = predict.read_csvs(str(tmp_path))
    assert numpy.array_equal(back.lpd_i, res.lpd_i, equal_nan=True) and back.y.shape[1] == 0


def test_new_data_validation():
    obs = numpy.zeros((4, 2))
    d = NewData(obs, [0, 1, -1, -3])
    assert (d.n_new, d.n_fields, d.K) == (4, 2, 3) and d.group.dtype == numpy.int32
    assert NewData(obs, [0, 1, 1, 0]).K == 0 and "n_new=4" in repr(d)
    assert NewData(numpy.zeros(3), [0, 0, 0]).obs.shape == (3, 1)
    for o, g in ((numpy.zeros((4, 2, 1)), [0] * 4), (obs, [0, 1]), (obs, [[0, 1], [0, 1]]),
                 (obs, [0.5, 1, 1, 1]), (numpy.zeros((0, 2)), []), (obs, [0, 1, 2, 2 ** 31])):
        with pytest.raises(ValueError):
            NewData(o, g)
    y = numpy.array([[1.0, numpy.nan], [2.0, 3.0], [numpy.inf, 1.0], [0.0, 0.0]])
    assert list(NewData(y, [0] * 4).has_response([1])) == [False, True, True, True]
    assert list(NewData(y, [0] * 4).has_response([0, 1])) == [False, True, False, True]
    fam = sc.BY_NAME["benign"].fam
    d.check(fam, 2, "partial")
    with pytest.raises(ValueError, match="partial"):
        d.check(fam, 2, "none")
    with pytest.raises(ValueError, match="training groups"):
        d.check(fam, 1, "partial")
    with pytest.raises(ValueError, match="fields"):
        NewData(numpy.zeros((4, 3)), [0] * 4).check(fam, 2, "partial")


def test_sample_posterior_refuses_before_sampling(tmp_path):
    sig, ben = sc.BY_NAME["sigma"], sc.BY_NAME["benign"]
    new = pr.setup("benign").new                      # (two new groups)
    out = str(tmp_path / "no")

    def run(fam, pooling, names, pf, priors=None):
        return sample_posterior(4, 20, 10, names, sc.G, sc.SIZES, pooling, fam, out,
                                priorDistribution=priors, displayProgress=False, predictFor=pf)

    with pytest.raises(ValueError, match="partial"):     # a new group without partial pooling
        run(sig.fam, "none", ("a", "b", "s"), new, sig.priors)
    with pytest.raises(ValueError, match="fields"):      # another width
        run(ben.fam, "partial", ("a", "b"), NewData(numpy.zeros((3, 3)), [0, 1, 2]))
    with pytest.raises(ValueError, match="training groups"):
        run(ben.fam, "partial", ("a", "b"), NewData(numpy.zeros((2, 2)), [0, sc.G]))
    with pytest.raises(ValueError, match="training groups"):   # complete pooling: one group
        run(sig.fam, "complete", ("a", "b", "s"), NewData(numpy.zeros((2, 2)), [0, 1]),
            sig.priors)
    with pytest.raises(ValueError, match="NewData"):
        run(ben.fam, "partial", ("a", "b"), (numpy.zeros((2, 2)), [0, 1]))
    assert not os.path.exists(out)
