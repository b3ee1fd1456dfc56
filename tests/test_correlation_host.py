"""nestmc.correlation on the host: the numpy route against the longdouble reference of
correlation_ref (derived tolerance), merge (Chan's update) of chain splits against the whole,
the identity part, pack / unpack, finish on hand-made parts, the pairs table, the CSV round
trip and the keyword."""

import inspect
import os

import numpy
import pytest

import correlation_ref as cr
from nestmc import correlation as co


def test_host_route_against_reference():
    for seed, rows, cols, C, nv in ((1, 20, 42, 70, 70), (2, 3, 42, 70, 65), (3, 1, 42, 70, 64),
                                    (4, 7, 1, 5, 3)):
        x = cr.store_case(seed, rows, cols, C)
        x[:, :, nv:] = numpy.nan                                # never read
        got = co.comoments_from_samples(x, nv)
        cr.check(got, cr.reference(x, nv), rows * nv, 4)
    with pytest.raises(ValueError):
        co.comoments_from_samples(numpy.zeros((1, 3, 1)))          # one sample
    with pytest.raises(ValueError):
        co.comoments_from_samples(numpy.zeros((2, 3, 4)), 5)


def test_host_route_special_columns():
    x = cr.store_case(5, 4, 6, 9)
    x[:, 2] = 3.25                                              # constant
    x[1, 4, 3] = numpy.nan
    x[2, 5, 8] = numpy.inf
    got = co.comoments_from_samples(x)
    assert got["nonfinite"].tolist() == [0, 0, 0, 0, 1, 1]
    M = got["M"]
    keep = [0, 1, 3]
    assert numpy.isnan(M[4]).all() and numpy.isnan(M[:, 5]).all()
    assert numpy.isnan(got["mean"][4:]).all()
    assert not M[2, keep].any() and not M[keep, 2].any() and M[2, 2] == 0.0
    assert not numpy.signbit(M[2, keep]).any()
    clean = co.comoments_from_samples(numpy.ascontiguousarray(x[:, keep]))
    assert numpy.array_equal(M[numpy.ix_(keep, keep)], clean["M"])
    res = co.finish(got)
    assert numpy.isnan(res.corr[2]).all() and numpy.isnan(res.corr[:, 2]).all()
    assert res.constant.tolist() == [False, False, True, False, False, False]


def test_merge_of_chain_splits():
    rows, cols, C = 12, 42, 70
    x = cr.store_case(6, rows, cols, C)
    ref = cr.reference(x)
    for cuts in ((0, 33, 70), (0, 1, 40, 70)):
        parts = [co.comoments_from_samples(numpy.ascontiguousarray(x[:, :, a:b]))
                 for a, b in zip(cuts, cuts[1:])]
        m = co.merge(parts)
        cr.check(m, ref, rows * C, 8)
    # the identity, anywhere in the list, changes nothing
    whole = co.comoments_from_samples(x)
    for parts in ([co.identity(cols), whole], [whole, co.identity(cols)],
                  [co.identity(cols), whole, co.identity(cols)]):
        m = co.merge(parts)
        for k in ("mean", "min", "max", "M", "nonfinite"):
            assert numpy.array_equal(m[k], whole[k]), k
        assert m["n_samples"] == whole["n_samples"]
    assert co.merge([co.identity(3), co.identity(3)])["n_samples"] == 0
    with pytest.raises(ValueError):
        co.merge([])
    with pytest.raises(ValueError):
        co.merge([co.identity(3), co.identity(4)])


def test_pack_unpack():
    part = co.comoments_from_samples(cr.store_case(7, 5, 9, 6), 4)
    part["nonfinite"][3] = 12345
    vec = co.pack(part)
    assert vec.dtype == numpy.float64 and vec.shape == (1 + 4 * 9 + 81,)
    back = co.unpack(numpy.frombuffer(vec.tobytes(), dtype=numpy.float64), 9)
    for k in ("mean", "min", "max", "M", "nonfinite"):
        assert numpy.array_equal(back[k], part[k]), k
    assert back["n_samples"] == 20 and back["nonfinite"].dtype == numpy.int64
    idn = co.unpack(co.pack(co.identity(2)), 2)
    assert idn["n_samples"] == 0 and numpy.isinf(idn["min"]).all()
    with pytest.raises(ValueError):
        co.unpack(vec, 8)


def hand_part():
    """Three columns, S = 5: M chosen so that rounding pushes a ratio past 1."""
    M = numpy.array([[4.0, 6.0000000000000009, -2.0],
                     [6.0000000000000009, 9.0, 1.5],
                     [-2.0, 1.5, 16.0]])
    return dict(mean=numpy.array([1.0, -2.0, 0.5]), min=numpy.array([0.0, -4.0, -1.0]),
                max=numpy.array([2.0, 0.0, 3.0]), M=M, nonfinite=numpy.zeros(3, dtype=numpy.int64),
                n_samples=5)


def test_finish_formulas_diagonal_and_clipping():
    p = hand_part()
    assert p["M"][0, 1] / numpy.sqrt(4.0 * 9.0) > 1.0           # would exceed 1 unclipped
    r = co.finish(p, ["a", "b", "c"])
    assert r.parameter == ["a", "b", "c"] and r.n_samples == 5
    assert numpy.array_equal(r.cov, p["M"] / 4.0)
    assert numpy.array_equal(r.sd, numpy.sqrt(numpy.array([1.0, 2.25, 4.0])))
    assert numpy.array_equal(numpy.diagonal(r.corr), [1.0, 1.0, 1.0])
    assert r.corr[0, 1] == 1.0 and r.corr[1, 0] == 1.0           # clipped
    assert r.corr[0, 2] == -2.0 / numpy.sqrt(4.0 * 16.0) == r.pair("a", "c") == r.pair(2, 0)
    assert r.corr[1, 2] == 1.5 / numpy.sqrt(9.0 * 16.0)
    q = hand_part()
    q["M"][0, 1] = q["M"][1, 0] = -6.0000000000000009
    assert co.finish(q).corr[0, 1] == -1.0
    with pytest.raises(ValueError):
        co.finish(dict(p, n_samples=1))
    with pytest.raises(ValueError):
        co.finish(p, ["a", "b"])


def test_finish_constant_column_is_nan():
    p = hand_part()
    p["min"][1] = p["max"][1] = -2.0
    p["M"][1, :] = 0.0
    p["M"][:, 1] = 0.0
    r = co.finish(p)
    assert numpy.isnan(r.corr[1]).all() and numpy.isnan(r.corr[:, 1]).all()
    assert r.corr[0, 0] == 1.0 and r.corr[2, 2] == 1.0 and r.corr[0, 2] == -0.25
    assert r.sd[1] == 0.0 and not r.cov[1].any()


def _result(P, G, partial):
    cols = P * (G + 2 * partial)
    from nestmc import output
    names = output.header_names(["a", "b", "c"][:P], G, partial)
    x = cr.store_case(8, 6, cols, 5)
    return co.finish(co.comoments_from_samples(x), names), names


def test_pairs_rows_and_order():
    r, names = _result(2, 3, True)
    rows = r.pairs(2, 3, True)
    want = [("within_group", "a_mu", "b_mu"), ("within_group", "a_sigma2", "b_sigma2"),
            ("within_group", "a[000]", "b[000]"), ("within_group", "a[001]", "b[001]"),
            ("within_group", "a[002]", "b[002]"),
            ("with_mu", "a[000]", "a_mu"), ("with_mu", "a[001]", "a_mu"),
            ("with_mu", "a[002]", "a_mu"), ("with_mu", "b[000]", "b_mu"),
            ("with_mu", "b[001]", "b_mu"), ("with_mu", "b[002]", "b_mu"),
            ("with_sigma2", "a[000]", "a_sigma2"), ("with_sigma2", "a[001]", "a_sigma2"),
            ("with_sigma2", "a[002]", "a_sigma2"), ("with_sigma2", "b[000]", "b_sigma2"),
            ("with_sigma2", "b[001]", "b_sigma2"), ("with_sigma2", "b[002]", "b_sigma2")]
    assert [row[:3] for row in rows] == want
    for kind, a, b, v in rows:
        assert v == r.corr[names.index(a), names.index(b)]
    r, names = _result(2, 3, False)
    rows = r.pairs(2, 3, False)
    assert [row[:3] for row in rows] == [("within_group", "a[%03d]" % g, "b[%03d]" % g)
                                         for g in range(3)]
    r, names = _result(3, 2, False)                              # three parameters: p < q
    assert [row[1:3] for row in r.pairs(3, 2, False)] == [
        ("a[000]", "b[000]"), ("a[000]", "c[000]"), ("b[000]", "c[000]"),
        ("a[001]", "b[001]"), ("a[001]", "c[001]"), ("b[001]", "c[001]")]
    with pytest.raises(ValueError):
        r.pairs(2, 2, False)


def test_pairs_one_parameter_has_no_within_group_rows():
    r, names = _result(1, 3, True)
    rows = r.pairs(1, 3, True)
    assert [row[0] for row in rows] == ["with_mu"] * 3 + ["with_sigma2"] * 3
    r, names = _result(1, 3, False)
    assert r.pairs(1, 3, False) == []


def test_csv_round_trip(tmp_path):
    r, names = _result(2, 3, True)
    co.write_csvs(r, str(tmp_path), 2, 3, True)
    assert sorted(os.listdir(str(tmp_path))) == [co.FILE_MATRIX, co.FILE_PAIRS]
    text = open(os.path.join(str(tmp_path), co.FILE_MATRIX)).read().splitlines()
    assert text[0] == "parameter," + ",".join("'%s'" % n for n in names)
    assert text[1].startswith("'a_mu',1.000000,") and len(text) == 1 + len(names)
    pt = open(os.path.join(str(tmp_path), co.FILE_PAIRS)).read().splitlines()
    assert pt[0] == "kind,column,other,correlation" and len(pt) == 1 + 5 + 12
    assert pt[1] == "within_group,'a_mu','b_mu',%.6f" % r.pair("a_mu", "b_mu")
    back = co.read_csvs(str(tmp_path))
    assert back["parameter"] == names
    assert numpy.abs(back["corr"] - r.corr).max() <= 0.5e-6         # the %.6f of convergence.csv
    rows = r.pairs(2, 3, True)
    assert [b[:3] for b in back["pairs"]] == [w[:3] for w in rows]
    assert max(abs(b[3] - w[3]) for b, w in zip(back["pairs"], rows)) <= 0.5e-6


def test_keyword_in_both_signatures():
    import posteriorSampling
    from nestmc import sampler
    for f in (posteriorSampling.samplePosterior, sampler.sample_posterior):
        assert inspect.signature(f).parameters["computeCorrelation"].default is False


def test_fewer_than_two_samples_raise_before_any_device(monkeypatch):
    """One chain, one recorded row: ValueError before an engine exists."""
    from nestmc import LinearRegression, engine, sampler
    monkeypatch.setattr(sampler._lib, "device_count",
                        lambda: pytest.fail("the device was asked for"))
    monkeypatch.setattr(engine.Engine, "__init__",
                        lambda *a, **k: pytest.fail("an engine was made"))
    x = numpy.arange(8.0)
    fam = LinearRegression.simple(x, 2.0 * x, sigma=1.0)
    with pytest.raises(ValueError, match="computeCorrelation"):
        sampler.sample_posterior(1, 10, 1, ("a", "b"), 2, 4, "partial", fam, None,
                                 write_files=False, displayProgress=False,
                                 computeCorrelation=True)
