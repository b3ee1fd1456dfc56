"""Posterior predictive checks on the host (nestmc/ppc.py) and the references the device tests
use (tests/ppc_ref.py).  Runs without a GPU.

* from_replicates against brute force; merge of split partials against the whole; identity;
  the CSV round trip;
* ppc_ref.restate (the kernels' float64 arithmetic) against ppc_ref.reference (longdouble) on
  the reference draws of one finite case per family kind: the per-observation counts must be
  equal (a draw against y is one exact comparison); a group comparison T(y_rep) against T(y)
  must come out as in longdouble unless the two are closer than the float64 statistic's own
  error bound (ppc_ref ``t_bound``) -- such comparisons are left out, at most 1 in 1000, and
  their number is printed (two sides equal in longdouble are not left out: float64 must say
  equal); n, mean and M2 within the tolerances of ppc_ref;
* the logistic case keeps every uniform 1e-12 away from its probability; the normals of the
  stream have mean 0 and variance 1; the misfit store flags exactly its group.
"""

import numpy
import pytest

import ppc_ref
import store_cases as sc
from nestmc import ppc

KINDS = ["benign", "sigma", "gauss", "logistic"]      # linreg, regression, gauss, logistic


def _brute(yrep, y, off):
    S, n, NR = yrep.shape
    G = len(off) - 1
    lt = numpy.zeros((n, NR), dtype=numpy.int64)
    eq = numpy.zeros((n, NR), dtype=numpy.int64)
    for s in range(S):
        for i in range(n):
            for j in range(NR):
                lt[i, j] += yrep[s, i, j] < y[i, j]
                eq[i, j] += yrep[s, i, j] == y[i, j]
    gt = numpy.zeros((G, NR, 4), dtype=numpy.int64)
    ge = numpy.zeros((G, NR, 4), dtype=numpy.int64)
    tr = numpy.zeros((S, G, NR, 4))
    ty = numpy.zeros((G, NR, 4))
    f = lambda v: [sum(v) / len(v), sum((a - sum(v) / len(v)) ** 2 for a in v) / len(v),   # noqa: E731
                   min(v), max(v)]
    for g in range(G):
        for j in range(NR):
            ty[g, j] = f(list(y[off[g]:off[g + 1], j]))
            for s in range(S):
                tr[s, g, j] = f(list(yrep[s, off[g]:off[g + 1], j]))
                gt[g, j] += tr[s, g, j] > ty[g, j]
                ge[g, j] += tr[s, g, j] == ty[g, j]
    return lt, eq, gt, ge, tr, ty


def test_from_replicates_against_brute_force():
    r = numpy.random.RandomState(11)
    off = numpy.array([0, 1, 4, 9])
    S, n, NR = 13, 9, 2
    y = numpy.round(r.normal(size=(n, NR)) * 2) / 2          # (halves: ties happen)
    yrep = numpy.round(r.normal(size=(S, n, NR)) * 2) / 2
    res = ppc.from_replicates(yrep, y, off)
    lt, eq, gt, ge, tr, ty = _brute(yrep, y, off)
    assert numpy.array_equal(res.lt, lt) and numpy.array_equal(res.eq, eq)
    assert eq.sum() > 0
    assert numpy.array_equal(res.pit_i, (lt + eq / 2.0) / S)
    assert numpy.allclose(res.t_obs, ty, rtol=1e-13, atol=1e-13)
    # the means' ties are decided by rounding: the minimum and maximum are exact
    assert numpy.array_equal(res.gt[..., 2:], gt[..., 2:])
    assert numpy.array_equal(res.geq[..., 2:], ge[..., 2:])
    assert numpy.array_equal(res.p, (res.gt + res.geq / 2.0) / S)
    assert numpy.allclose(res.mean_i, yrep.mean(0)) and numpy.allclose(res.sd_i, yrep.std(0, ddof=1))
    assert numpy.allclose(res.residual_i, (y - yrep.mean(0)) / yrep.std(0, ddof=1))
    assert numpy.allclose(res.t_mean, tr.mean(0)) and numpy.allclose(res.t_sd, tr.std(0, ddof=1))
    assert res.n_samples == S and res.n_obs == n
    with pytest.raises(ValueError):
        ppc.from_replicates(yrep[:1], y, off)


def _window(name, rb=0, nr=sc.R):
    return ppc_ref.f64(name)[:, rb:rb + nr]


def test_merge_of_split_partials_against_the_whole():
    case = sc.BY_NAME["benign"]
    y, yrep = ppc_ref.y_of(case), _window("benign")
    whole = ppc.merge(ppc_ref.restate(yrep, y, sc.C, sc.C))
    split = ppc.merge(ppc_ref.restate(yrep[:3], y, 3, 3) + ppc_ref.restate(yrep[3:], y, 67, 67))
    for k in ("obs_count", "group_count"):
        assert numpy.array_equal(whole[k], split[k]), k
        assert whole[k].dtype == numpy.int64
    assert numpy.array_equal(whole["ty"], split["ty"])
    ref = ppc_ref.reference(yrep, y, sc.C)
    ppc_ref.check_states(whole, ref, "whole")
    ppc_ref.check_states(split, ref, "3 + 67 chains")
    assert numpy.array_equal(whole["obs_state"][0], split["obs_state"][0])
    # the same partials in the same order: the same bits
    again = ppc.merge(ppc_ref.restate(yrep, y, sc.C, sc.C))
    assert all(numpy.asarray(whole[k]).tobytes() == numpy.asarray(again[k]).tobytes()
               for k in ("obs_state", "group_state"))
    with pytest.raises(ValueError):
        bad = dict(split, ty=split["ty"] + 1.0)
        ppc.merge([whole, bad])


def test_identity():
    case = sc.BY_NAME["gauss"]
    y = ppc_ref.y_of(case)
    parts = ppc_ref.restate(_window("gauss", 3, 1), y, sc.C, 65)
    ident = ppc.identity(sc.N_OBS, sc.G, 3)
    for order in ([ident, parts[0]], [parts[0], ident], [ident, ident, parts[0], ident]):
        m = ppc.merge(order)
        for k in ("obs_state", "obs_count", "group_state", "group_count", "ty"):
            assert numpy.asarray(m[k]).tobytes() == numpy.asarray(parts[0][k]).tobytes(), k
    two = ppc.merge([ident, ident])
    assert not two["obs_state"].any() and not two["group_count"].any()
    assert numpy.isnan(two["ty"]).all() and two["nonfinite"] == 0
    # n_valid = 64: the restatement's second block is the identity
    pad = ppc_ref.restate(_window("gauss"), y, sc.C, 64)[1]
    for k in ("obs_state", "obs_count", "group_state", "group_count"):
        assert numpy.asarray(pad[k]).tobytes() == numpy.asarray(ident[k]).tobytes(), k
    with pytest.raises(ValueError):
        ppc.finish(ident, sc.OFF, y)


def test_csv_round_trip(tmp_path):
    case = sc.BY_NAME["gauss"]
    y = ppc_ref.y_of(case)
    res = ppc.finish(ppc.merge(ppc_ref.restate(_window("gauss"), y, sc.C, sc.C)), sc.OFF, y)
    ppc.write_csvs(res, str(tmp_path))
    assert open(str(tmp_path / "ppc_groups.csv")).readline().strip() == ppc.HEADER_GROUPS
    assert open(str(tmp_path / "ppc_pointwise.csv")).readline().strip() == ppc.HEADER_POINTWISE
    back = ppc.read_csvs(str(tmp_path))
    for k in ("y", "mean_i", "sd_i", "residual_i", "pit_i", "lt", "eq", "t_obs", "t_mean", "t_sd",
              "p", "gt", "geq", "offsets"):
        assert numpy.array_equal(getattr(res, k), getattr(back, k)), k
    assert back.n_samples == res.n_samples == sc.C * sc.R
    assert res.lt.dtype == numpy.int64 and back.gt.dtype == numpy.int64
    lines = open(str(tmp_path / "ppc_groups.csv")).read().splitlines()
    assert len(lines) == 1 + sc.G * 3 * 4
    assert len(open(str(tmp_path / "ppc_pointwise.csv")).read().splitlines()) == 1 + sc.N_OBS * 3


@pytest.mark.parametrize("name", KINDS)
def test_restate_against_reference(name):
    case = sc.BY_NAME[name]
    y = ppc_ref.y_of(case)
    total = left = 0
    for rb, nr, nv in ((0, sc.R, 70), (0, sc.R, 65), (sc.R - 2, 2, 64), (3, 1, 70)):
        yrep = _window(name, rb, nr)
        assert numpy.isfinite(yrep).all()
        integer = case.fam.response_integer
        part = ppc.merge(ppc_ref.restate(yrep, y, sc.C, nv, integer))
        ref = ppc_ref.reference(yrep, y, nv, integer)
        assert numpy.array_equal(part["obs_count"][0], ref["lt"].T)
        assert numpy.array_equal(part["obs_count"][1], ref["eq"].T)
        ppc_ref.check_states(part, ref, "%s rows %d+%d n_valid %d" % (name, rb, nr, nv))
        # T(y) against longdouble within its bound
        keep = ~ref["ambiguous"]
        Tv = ppc_ref.group_stats(yrep[:nv].reshape((-1,) + yrep.shape[2:]), integer)
        with numpy.errstate(invalid="ignore"):
            gt, ge = Tv > part["ty"], Tv == part["ty"]
        assert numpy.array_equal(gt[keep], ref["gt"][keep]), (name, rb, nr, nv)
        assert numpy.array_equal(ge[keep], ref["geq"][keep]), (name, rb, nr, nv)
        assert numpy.array_equal(part["group_count"][..., 0], gt.sum(axis=0))
        assert numpy.array_equal(part["group_count"][..., 1], ge.sum(axis=0))
        total += keep.size
        left += int((~keep).sum())
    print("ppc restate %s: %d of %d group comparisons left out (closer than the float64 "
          "statistic's error bound)" % (name, left, total))
    assert left * 1000 <= total, (name, left, total)


def test_logistic_uniforms_keep_away_from_the_probabilities():
    gap = ppc_ref.draws("logistic")["gap"]
    assert gap.shape == (sc.C, sc.R, sc.N_OBS, 1)
    print("ppc logistic: min |ua - p| = %.3g over %d draws" % (gap.min(), gap.size))
    assert gap.min() > 1e-12


def test_normals_of_the_stream():
    z = ppc_ref.draws("benign")["z"].reshape(-1)
    n = z.size
    assert n == 58800
    m, v = z.mean(), z.var()
    print("ppc z: n=%d mean=%.4g (se %.3g) var=%.4g (se %.3g)"
          % (n, m, n ** -0.5, v, (2.0 / n) ** 0.5))
    assert abs(m) <= 4 * n ** -0.5
    assert abs(v - 1.0) <= 4 * (2.0 / n) ** 0.5


def test_misfit_store_flags_exactly_its_group():
    case = ppc_ref.case_of("misfit")
    y = ppc_ref.y_of(case)
    res = ppc.finish(ppc.merge(ppc_ref.restate(_window("misfit"), y, sc.C, sc.C)), sc.OFF, y)
    g = ppc_ref.MISFIT_GROUP
    print("ppc misfit p:\n%s" % res.p[:, 0])
    assert res.p[g, 0, 0] == 0.0 and res.gt[g, 0, 0] == 0 and res.geq[g, 0, 0] == 0
    assert {f[0] for f in res.flagged()} == {g}
    others = numpy.delete(res.p, g, axis=0)
    assert numpy.all((others > 0.025) & (others < 0.975))
    w = res.warning()
    assert w is not None and "group %d mean" % g in w and "\n" not in w
    host = ppc.from_replicates(_window("misfit").reshape(-1, sc.N_OBS, 1), y, sc.OFF)
    assert numpy.array_equal(host.lt, res.lt) and numpy.array_equal(host.eq, res.eq)
    assert {f[0] for f in host.flagged()} == {g}
