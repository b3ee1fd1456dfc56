"""nestmc.summary on the host: gap_of, finish / from_sorted, merge_sorted, csv_text,
assessment, and the restatement tests/summary_ref.py that the GPU tests compare against.
No GPU.  References: numpy.median and nestmc.diagnosis.hpd_interval (the product's statement
of computeHpdInterval); everything is compared as uint64 words."""

import numpy
import pytest

import summary_ref as sr
from nestmc import convergence as conv
from nestmc import diagnosis
from nestmc import summary as sm


def _same(a, b, what):
    a, b = sr.words(a), sr.words(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert numpy.array_equal(a, b), (what, a, b)


def _data(N, kind, seed=0):
    r = numpy.random.RandomState(seed + N)
    x = r.normal(size=(3, N)) * [[1.0], [30.0], [1e-3]] + [[0.0], [5.0], [-2.0]]
    return numpy.round(x, 1) + 0.0 if kind == "ties" else x   # (+ 0.0: no negative zeros)


# ---- the key ------------------------------------------------------------------------------
def test_key_orders_like_the_number_and_inverts():
    big = numpy.finfo(numpy.float64).max
    v = numpy.array([-numpy.inf, -big, -1.5, -5e-324, -0.0, 0.0, 5e-324, 1.5, big, numpy.inf,
                     numpy.nan])
    k = sr.key(v)
    assert numpy.all(k[1:] > k[:-1])
    _same(sr.unkey(k), v, "inverse")
    _same(sm.sort_unkey(sm.sort_key(v)), v, "the module's inverse")
    assert numpy.array_equal(sm.sort_key(v), k)
    x = numpy.random.RandomState(1).normal(size=5000)
    _same(sr.unkey(numpy.sort(sr.key(x))), numpy.sort(x), "numpy.sort")


# ---- median and HDI against numpy.median and hpd_interval ---------------------------------------
@pytest.mark.parametrize("kind", ["continuous", "ties"])
@pytest.mark.parametrize("N", [2, 3, 10, 11, 4097])
def test_stats_against_numpy_and_hpd_interval(N, kind):
    x = _data(N, kind)
    s = sr.sorted_ref(x.T[:, :, None])            # a store of N rows, 3 columns, one chain
    _same(s, numpy.sort(x, axis=1), "sorted_ref against numpy.sort")
    gap = sm.gap_of(N)
    assert gap == sr.gap_ref(N)
    res = sm.from_sorted(s, ["a", "b", "c"])
    assert res.n == N and res.gap == gap and not res.nonfinite.any()
    for k in range(3):
        st = sr.stats_ref(s[k], gap, ranks=[0, N - 1])
        lo, hi = diagnosis.hpd_interval(x[k], 95)
        _same(st["median"], numpy.median(x[k]), "stats_ref median")
        _same([st["lower"], st["upper"]], [lo, hi], "stats_ref HDI")
        _same(res.median[k], numpy.median(x[k]), "median")
        _same([res.hdi_lower[k], res.hdi_upper[k]], [lo, hi], "HDI")
        _same([res.minimum[k], res.maximum[k]], [x[k].min(), x[k].max()], "min, max")
        _same(st["ranks"], [x[k].min(), x[k].max()], "ranks")
        width = s[k][gap:] - s[k][:N - gap]
        assert st["at"] == int(numpy.argmax(width == width.min()))
        assert (width[:st["at"]] > width[st["at"]]).all()     # the FIRST minimum


def test_finish_is_from_sorted():
    x = _data(10, "ties")
    s = numpy.sort(x, axis=1)
    gap = sm.gap_of(10)
    at = s[:, sm.stat_ranks(10)]
    hdi = numpy.array([sm.hdi_of_sorted(c, gap)[:2] for c in s])
    a = sm.finish(at, hdi, numpy.zeros(3, dtype=numpy.int64), 10, None)
    b = sm.from_sorted(s)
    assert a.parameter == b.parameter == ["col0", "col1", "col2"]
    for f in ("median", "hdi_lower", "hdi_upper", "minimum", "maximum"):
        _same(getattr(a, f), getattr(b, f), f)


def test_nonfinite_column_is_flagged():
    x = _data(11, "continuous")
    x[1, 4] = numpy.inf
    res = sm.from_sorted(sr.sorted_ref(x.T[:, :, None]))
    assert list(res.nonfinite) == [0, 1, 0]
    for f in ("median", "hdi_lower", "hdi_upper", "minimum", "maximum"):
        v = getattr(res, f)
        assert numpy.isnan(v[1]) and numpy.isfinite(v[[0, 2]]).all()
    st = sr.stats_ref(sr.sorted_ref(x.T[:, :, None])[1], sm.gap_of(11), ranks=[3])
    assert st["at"] == -1 and numpy.isnan(st["median"]) and numpy.isnan(st["ranks"]).all()


# ---- merge_sorted -------------------------------------------------------------------------------
@pytest.mark.parametrize("cuts", [(0,), (1,), (7,), (3, 3, 9), (12, 5)])
def test_merge_of_any_split_is_the_sort_of_the_union(cuts):
    x = _data(13, "ties", seed=3)
    x[0, :4] = [-0.0, 0.0, 0.0, -0.0]
    whole = sr.unkey(numpy.sort(sr.key(x), axis=1))
    edges = sorted(cuts)
    parts = [p for p in numpy.split(x, edges, axis=1)]
    _same(sm.merge_sorted(parts), whole, "merge")
    _same(sm.merge_sorted(parts[::-1]), whole, "merge, parts reversed")
    # (sorted by key: numpy.sort of floats does not promise to keep the signs of equal zeros)
    _same(sm.merge_sorted([sr.unkey(numpy.sort(sr.key(p), axis=1)) for p in parts]), whole,
          "merge of sorted parts")


# ---- gap_of ---------------------------------------------------------------------------------------
def test_gap_of():
    # N * 0.95 = 1.9, 9.5, 19.0, 19.95, 28.5: Python rounds halves to even, and N - 1 caps
    assert [sm.gap_of(N) for N in (2, 10, 20, 21, 30)] == [1, 9, 19, 20, 28]
    assert sm.gap_of(10, 50) == 5 and sm.gap_of(3, 1) == 1 and sm.gap_of(5, 100) == 4
    for N in (2, 10, 20, 21, 30, 4097):
        x = numpy.arange(N, dtype=numpy.float64) ** 2
        lo, hi = diagnosis.hpd_interval(x, 95)
        assert (lo, hi) == (x[0], x[sm.gap_of(N)])


# ---- csv_text -------------------------------------------------------------------------------------
def test_csv_text(tmp_path):
    res = sm.SummaryResult(["b[01]", "a_mu", "a[10]"], [1.0, -2.5, 1e-7], [0.5, -3.0, 0.0],
                           [1.5, -2.0, 2.0], [0.0, -4.0, -1.0], [2.0, 0.0, 3.0], 10,
                           [0, 0, 0])
    text = sm.csv_text(res)
    assert text == ("parameter,median,HDI lower,HDI upper,min,max\n"
                    "'a[10]',0.000000,0.000000,2.000000,-1.000000,3.000000\n"
                    "'a_mu',-2.500000,-3.000000,-2.000000,-4.000000,0.000000\n"
                    "'b[01]',1.000000,0.500000,1.500000,0.000000,2.000000\n")
    sm.write_csv(res, str(tmp_path))
    assert (tmp_path / "summary.csv").read_text() == text


# ---- assessment -----------------------------------------------------------------------------------
def test_assessment_field_by_field():
    r = numpy.random.RandomState(4)
    x = r.normal(size=(3, 6, 8))                      # [K][m][n]
    names = ["b[01]", "a_mu", "a[10]"]
    c = conv.from_halfchains(x, names, variogram=conv.variogram_host)
    s = sm.from_sorted(numpy.sort(x.reshape(3, -1), axis=1), names)
    a = sm.assessment(c, s)
    assert a.dtype == numpy.dtype(diagnosis.ASSESS_DTYPE)
    assert list(a["parameter"]) == [b"a[10]", b"a_mu", b"b[01]"]
    for row, k in zip(a, (2, 1, 0)):
        flat = x[k].reshape(-1)
        lo, hi = diagnosis.hpd_interval(flat, 95)
        _same(row["rhat"], c.rhat[k], "rhat")
        _same(row["effective n"], c.effective_n[k], "effective n")
        assert row["converged"] == (c.rhat[k] < 1.1)
        assert row["enough n"] == (c.effective_n[k] > c.m * 10)
        _same(row["median"], numpy.median(flat), "median")
        _same([row["HDI lower"], row["HDI upper"]], [lo, hi], "HDI")
    with pytest.raises(ValueError):
        sm.assessment(c, sm.from_sorted(numpy.sort(x.reshape(3, -1), axis=1), ["x", "y", "z"]))


# ---- the argument errors --------------------------------------------------------------------------
def test_argument_errors():
    with pytest.raises(ValueError):
        sm.gap_of(1)
    with pytest.raises(ValueError):
        sm.from_sorted(numpy.zeros(5))
    with pytest.raises(ValueError):
        sm.from_sorted(numpy.zeros((2, 1)))
    with pytest.raises(ValueError):
        sm.from_sorted(numpy.zeros((2, 5)), ["only one"])
    with pytest.raises(ValueError):
        sm.merge_sorted([])
    with pytest.raises(ValueError):
        sm.merge_sorted([numpy.zeros((2, 3)), numpy.zeros((3, 3))])
    with pytest.raises(ValueError):
        sm.finish(numpy.zeros((2, 3)), numpy.zeros((2, 2)), numpy.zeros(2), 5, None)
    with pytest.raises(ValueError):
        sm.finish(numpy.zeros((2, 4)), numpy.zeros((2, 3)), numpy.zeros(2), 5, None)
