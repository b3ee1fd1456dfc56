"""The columns' sort and order statistics on the GPU: nmc_k_sort_tiles / _merge / _scan
(csrc/sortcol.h) through nmc_summary_of, Engine.summary_raw / summary and
samplePosterior(computeSummary=True).

Reference: tests/summary_ref.py.  Order statistics depend on the multiset of a column's values
alone, so whole sorted columns and every statistic are compared as uint64 words: no tolerance.

One case of the proposal is stated differently here: its column of extreme values names
+-1.8e308, which is no double (the literal reads as infinity, which case 2 covers on its own);
the column holds +-1.7976931348623157e308, the largest finite doubles, instead."""

import ctypes
import os

import numpy
import pytest

import summary_ref as sr
from gpu_cases import synthetic
from nestmc import _lib
from nestmc import summary as sm
from nestmc.engine import Engine
from oracle import restatement as rs

pytestmark = pytest.mark.gpu

T = sr.T   # csrc/sortcol.h NMC_SORT_TILE: the keys of one LDS tile = one workgroup's outputs


def _same(a, b, what):
    a, b = sr.words(a), sr.words(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    bad = a != b
    assert not bad.any(), "%s: %d of %d words differ, first at %s (%#x against %#x)" % (
        what, bad.sum(), bad.size, numpy.argwhere(bad)[0], a[bad][0], b[bad][0])


def _i64(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))


def _of(lib, x, n_valid, ranks=None, col_batch=0, gap=None, want_sorted=True, rc=False):
    """nmc_summary_of over the host array x [rows][cols][C]."""
    x = numpy.ascontiguousarray(x, dtype=numpy.float64)
    rows, cols, C = x.shape
    N = rows * n_valid
    gap = (sm.gap_of(N) if N >= 2 else 1) if gap is None else gap
    rk = numpy.ascontiguousarray(sm.stat_ranks(N) if ranks is None and N >= 2 else
                                 [0] if ranks is None else ranks, dtype=numpy.int64)
    at = numpy.full((cols, len(rk)), -7.0)
    hdi = numpy.full((cols, 2), -7.0)
    hdi_at = numpy.full(cols, -7, dtype=numpy.int64)
    bad = numpy.full(cols, -7, dtype=numpy.int64)
    srt = numpy.full((cols, max(N, 0)), -7.0) if want_sorted else None
    code = lib.nmc_summary_of(0, _lib.dptr(x), rows, cols, C, n_valid, gap, _i64(rk), len(rk),
                              col_batch, _lib.dptr(at), _lib.dptr(hdi), _i64(hdi_at), _i64(bad),
                              _lib.dptr(srt))
    if rc:
        return code
    _lib.check(code)
    return dict(at_ranks=at, hdi=hdi, hdi_at=hdi_at, nonfinite=bad, sorted=srt, N=N, gap=gap,
                ranks=rk)


def _check(got, store, row_begin=0, n_rows=None, n_valid=None, what=""):
    """Everything a call returned against the restatement over the same window."""
    want = sr.sorted_ref(store, row_begin, n_rows, n_valid)
    assert want.shape[1] == got["N"]
    if got["sorted"] is not None:
        _same(got["sorted"], want, what + " sorted columns")
    rk = got.get("ranks", numpy.asarray(sm.stat_ranks(got["N"])))
    for k in range(want.shape[0]):
        st = sr.stats_ref(want[k], got["gap"], rk)
        assert got["nonfinite"][k] == st["nonfinite"], (what, k)
        assert got["hdi_at"][k] == st["at"], (what, k, got["hdi_at"][k], st["at"])
        _same(got["hdi"][k], [st["lower"], st["upper"]], "%s HDI of column %d" % (what, k))
        if st["nonfinite"]:
            assert numpy.isnan(got["at_ranks"][k]).all()
        else:
            _same(got["at_ranks"][k], st["ranks"], "%s ranks of column %d" % (what, k))
    return want


# ---- 1. sizes ---------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [2, 3, T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1, 3 * T + 5,
                               5 * T + 1, 8 * T, 8 * T + 3])
def test_sizes_one_chain(gpu_lib, N):
    x = numpy.random.RandomState(N).normal(size=(N, 2, 3))
    got = _of(gpu_lib, x, 1)
    want = _check(got, x, n_valid=1, what="N = %d" % N)
    _same(want, numpy.sort(x[:, :, 0].T, axis=1), "the restatement against numpy.sort")
    res = sm.finish(got["at_ranks"], got["hdi"], got["nonfinite"], N, None)
    for k in range(2):
        _same(res.median[k], numpy.median(x[:, k, 0]), "median")


@pytest.mark.parametrize("rows,C,n_valid", [(100, 70, 70), (257, 130, 129)])
def test_sizes_whole_chain_blocks(gpu_lib, rows, C, n_valid):
    """N = 7 000 (two tiles), and N = 33 153: 9 runs, so a run without a partner in three of
    the four passes."""
    x = numpy.random.RandomState(rows).normal(size=(rows, 2, C))
    rk = [0, 1, rows * n_valid // 2, rows * n_valid - 1]
    _check(_of(gpu_lib, x, n_valid, ranks=rk), x, n_valid=n_valid, what="%dx%d" % (rows, n_valid))


# ---- 2. values ----------------------------------------------------------------------------------
def test_values(gpu_lib):
    N = 2 * T + 1
    r = numpy.random.RandomState(2)
    big = numpy.finfo(numpy.float64).max
    special = r.normal(size=N)
    special[:8] = [-0.0, 0.0, 5e-324, -5e-324, big, -big, 0.0, -0.0]
    r.shuffle(special)
    with_inf = r.normal(size=N)
    with_inf[N // 3] = numpy.inf
    with_nan = r.normal(size=N)
    with_nan[N - 2] = numpy.nan
    cols = [numpy.full(N, 1.25),                                   # 0 all equal
            numpy.arange(N) * 0.5 - 100.0,                         # 1 ascending
            -(numpy.arange(N) * 0.25) + 7.0,                       # 2 descending
            numpy.where(r.uniform(size=N) < 0.3, -1.0, 2.0),       # 3 two distinct values
            numpy.round(r.normal(size=N), 1) + 0.0,                # 4 ties
            r.permutation(N).astype(numpy.float64),                # 5 integers: equal widths
            special,                                               # 6
            with_inf,                                              # 7
            with_nan,                                              # 8
            r.normal(size=N)]                                      # 9 after the flagged ones
    x = numpy.zeros((N, len(cols), 3))
    x[:, :, 0] = numpy.array(cols).T
    x[:, :, 1:] = r.normal(size=(N, len(cols), 2))
    got = _of(gpu_lib, x, 1)
    _check(got, x, n_valid=1, what="values")
    assert list(got["nonfinite"]) == [0, 0, 0, 0, 0, 0, 0, 1, 1, 0]
    assert list(got["hdi_at"][[0, 1, 2, 5]]) == [0, 0, 0, 0]
    assert list(got["hdi_at"][[7, 8]]) == [-1, -1]
    assert numpy.isnan(got["hdi"][[7, 8]]).all() and numpy.isnan(got["at_ranks"][[7, 8]]).all()
    assert numpy.isfinite(got["hdi"][[6, 9]]).all()
    s = got["sorted"]
    assert numpy.isnan(s[8, -1]) and s[7, -1] == numpy.inf          # key order: +inf < NaN
    zeros = s[6][s[6] == 0.0]
    assert list(numpy.signbit(zeros)) == [True, True, False, False]   # -0.0 before +0.0
    _same(s[6][[0, -1]], [-big, big], "the largest finite doubles")


# ---- 3. padding chains --------------------------------------------------------------------------
def test_padding_chains_do_not_enter(gpu_lib):
    rows, C, n_valid = 50, 70, 33
    x = numpy.random.RandomState(3).normal(size=(rows, 2, C))
    x[:, :, n_valid:] = numpy.where(numpy.arange(C - n_valid) % 2, 1e300, -1e300)
    got = _of(gpu_lib, x, n_valid)
    _check(got, x, n_valid=n_valid, what="padding")
    assert numpy.abs(got["sorted"]).max() < 10 and numpy.abs(got["hdi"]).max() < 10
    assert numpy.abs(got["at_ranks"]).max() < 10


# ---- 4. column batches --------------------------------------------------------------------------
def test_column_batches(gpu_lib):
    x = numpy.random.RandomState(4).normal(size=(300, 5, 20))       # N = 6 000: two tiles
    x[7, 3, 2] = numpy.nan
    a = _of(gpu_lib, x, 20, col_batch=0)
    b = _of(gpu_lib, x, 20, col_batch=2)                            # batches of 2, 2 and 1
    c = _of(gpu_lib, x, 20, col_batch=9)
    _check(a, x, what="one batch")
    for k in ("sorted", "at_ranks", "hdi"):
        _same(a[k], b[k], "col_batch=2: " + k)
        _same(a[k], c[k], "col_batch=9: " + k)
    for k in ("hdi_at", "nonfinite"):
        assert numpy.array_equal(a[k], b[k]) and numpy.array_equal(a[k], c[k])
    assert list(a["nonfinite"]) == [0, 0, 0, 1, 0]


def test_argument_errors(gpu_lib):
    x = numpy.random.RandomState(5).normal(size=(10, 2, 4))
    N = 10 * 3
    assert _of(gpu_lib, x, 3, rc=True) == 0
    for kw in (dict(n_valid=0), dict(n_valid=5), dict(n_valid=3, gap=0), dict(n_valid=3, gap=N),
               dict(n_valid=3, ranks=[-1]), dict(n_valid=3, ranks=[0, N])):
        assert _of(gpu_lib, x, rc=True, **kw) == -1, kw
    assert _of(gpu_lib, x[:1], 1, gap=1, ranks=[0], rc=True) == -1           # N = 1
    got = _of(gpu_lib, x, 3, gap=N - 1, ranks=[N - 1, 0])                    # the bounds themselves
    _check(got, x, n_valid=3, what="bounds")


# ---- 5. an engine's store -----------------------------------------------------------------------
def _state(fam, sizes, C, P, pooling, seed=5):
    r = numpy.random.RandomState(seed)
    G = len(sizes)
    value = r.normal(size=(C, P, G)) * 0.3
    lp = numpy.zeros((C, P, G))
    nested = rs.Nested(fam, sizes)
    ll = numpy.array([nested.group_ll(value[c]) for c in range(C)])
    mu = numpy.zeros((C, P)) if pooling == "partial" else None
    s2 = numpy.full((C, P), 0.5) if pooling == "partial" else None
    return value, lp, ll, mu, s2


def _run(fam, sizes, priors, pooling, C, sched, seed=3, sel=None, chain_base=0, state=None):
    """An engine after sched[0] iterations on chains sel of the C-chain state."""
    st = state or _state(fam, sizes, C, fam.n_params, pooling)
    sel = numpy.arange(C) if sel is None else numpy.asarray(sel)
    eng = Engine(fam, sizes, len(sel), pooling, priors, seed=seed, chain_base=chain_base)
    pick = lambda a: None if a is None else a[sel]   # noqa: E731
    eng.set_state(*(pick(a) for a in st))
    eng.set_schedule(*sched)
    eng.run(0, sched[0])
    eng.synchronize()
    return eng


@pytest.fixture(scope="module")
def eng70(gpu_lib):
    fam, sizes, priors, pooling, _ = synthetic("linreg_partial", 70, 5, 30)
    eng = _run(fam, sizes, priors, pooling, 70, (120, 20, 1))
    assert eng.n_rows == 100 and eng.cols == 14
    yield eng
    eng.close()


def test_engine_store(eng70):
    eng = eng70
    store = eng.samples_raw()
    got = eng.summary_raw(want_sorted=True)
    assert got["N"] == 7000 and got["sorted"].shape == (14, 7000)
    want = _check(got, store, what="whole store")
    res = eng.summary(["p%02d" % k for k in range(14)])
    ref = sm.from_sorted(want, ["p%02d" % k for k in range(14)])
    for f in ("median", "hdi_lower", "hdi_upper", "minimum", "maximum"):
        _same(getattr(res, f), getattr(ref, f), f)
    assert res.n == 7000 and res.gap == 6650 and not res.nonfinite.any()
    assert eng.summary_raw()["sorted"] is None
    # a window
    got = eng.summary_raw(row_begin=3, n_rows=41, want_sorted=True)
    assert got["N"] == 41 * 70
    _check(got, store, row_begin=3, n_rows=41, what="window")
    # ranks at the 2.5 / 25 / 75 / 97.5 % positions
    rk = [int(7000 * p) for p in (0.025, 0.25, 0.75, 0.975)]
    got = eng.summary_raw(ranks=rk)
    got["ranks"] = numpy.asarray(rk)
    _check(got, store, what="quartile ranks")
    _same(got["at_ranks"], want[:, rk], "the values at the ranks")
    # the real chains of a padded shard
    got = eng.summary_raw(n_valid=60, want_sorted=True, col_batch=5)
    _check(got, store, n_valid=60, what="n_valid = 60")


def test_engine_argument_errors(eng70):
    eng = eng70
    for kw in (dict(row_begin=-1, n_rows=4), dict(row_begin=98, n_rows=3), dict(n_rows=101),
               dict(n_valid=0, n_rows=100), dict(n_valid=71), dict(ranks=[7000]),
               dict(ranks=[-1])):
        with pytest.raises((_lib.NestmcError, ValueError)):
            eng.summary_raw(**kw)
    with pytest.raises(ValueError):
        eng.summary_raw(n_rows=1, n_valid=1)
    _check(eng.summary_raw(), eng.samples_raw(), what="the context still works")


# ---- 6. shards ----------------------------------------------------------------------------------
def test_shards_merge_to_the_same_words(gpu_lib):
    fam, sizes, priors, pooling, _ = synthetic("linreg_partial", 128, 3, 20)
    st = _state(fam, sizes, 128, 2, pooling)
    sched = (60, 20, 4)
    engs = [_run(fam, sizes, priors, pooling, 128, sched, state=st)]
    try:
        for a, b in ((0, 64), (64, 128), (0, 33), (33, 128)):
            engs.append(_run(fam, sizes, priors, pooling, 128, sched, state=st, sel=range(a, b),
                             chain_base=a))
        one = engs[0].summary_raw(want_sorted=True)
        _check(one, engs[0].samples_raw(), what="one engine")
        whole = engs[0].summary()
        for pair, what in ((engs[1:3], "64 + 64"), (engs[3:5], "33 + 95")):
            parts = [e.summary_raw(want_sorted=True)["sorted"] for e in pair]
            assert sum(p.shape[1] for p in parts) == one["N"]
            merged = sm.merge_sorted(parts)
            _same(merged, one["sorted"], what)
            _same(sm.merge_sorted(parts[::-1]), one["sorted"], what + " reversed")
            res = sm.from_sorted(merged)
            for f in ("median", "hdi_lower", "hdi_upper", "minimum", "maximum"):
                _same(getattr(res, f), getattr(whole, f), "%s: %s" % (what, f))
    finally:
        for e in engs:
            e.close()


# ---- 7. samplePosterior(computeSummary=True) ----------------------------------------------------
FIELDS = ("median", "hdi_lower", "hdi_upper", "minimum", "maximum")


def _api_case():
    C, G, N = 6, 3, 20
    fam, sizes, priors, pooling, names = synthetic("linreg_partial", C, G, N)
    kw = dict(saveLogLikelihood=False, priorDistribution=priors,
              startingPointValueRange={n: [-0.5, 0.5] for n in names}, displayProgress=False,
              seed=17, return_samples=True, computeSummary=True)
    return (C, 64, 16, names, G, N, pooling, fam), kw       # burn 32, thin 2: 16 rows


def _restated(rows, header):
    """rows [C][rows][cols] of samplePosterior -> the SummaryResult of the restatement."""
    return sm.from_sorted(sr.sorted_ref(numpy.transpose(rows, (1, 2, 0))), header)


def test_sample_posterior_compute_summary(gpu_lib, tmp_path):
    from nestmc import diagnosis
    from nestmc.sampler import sample_posterior
    args, kw = _api_case()
    nothing = str(tmp_path / "nothing")
    mem = sample_posterior(*args, nothing, **dict(kw, write_files=False))
    assert not os.path.exists(nothing)
    res = mem["summary"]
    assert mem["rows"].shape == (6, 16, 10) and res.parameter == list(mem["header"])
    assert "assessment" not in mem and "convergence" not in mem
    want = _restated(mem["rows"], mem["header"])
    for f in FIELDS:
        _same(getattr(res, f), getattr(want, f), f)
    assert res.n == 96 and res.gap == 91 and not res.nonfinite.any()
    for k in range(10):
        flat = mem["rows"][:, :, k].reshape(-1)
        _same(res.median[k], numpy.median(flat), "numpy.median")
        _same([res.hdi_lower[k], res.hdi_upper[k]], diagnosis.hpd_interval(flat), "hpd_interval")
    # with files: summary.csv is csv_text of that result
    out = str(tmp_path / "one")
    one = sample_posterior(*args, out, **dict(kw, write_files=True))
    assert sorted(os.listdir(out)) == ["log", "sample", "summary.csv"]
    assert numpy.array_equal(one["rows"], mem["rows"])
    assert open(os.path.join(out, "summary.csv")).read() == sm.csv_text(want)
    assert sm.csv_text(one["summary"]) == sm.csv_text(want)
    # with computeDiagnostics as well: the assessment table of the two results
    both = sample_posterior(*args, None, **dict(kw, write_files=False, computeDiagnostics=True))
    a = both["assessment"]
    b = sm.assessment(both["convergence"], both["summary"])
    assert a.dtype == b.dtype == numpy.dtype(diagnosis.ASSESS_DTYPE)
    assert a.tobytes() == b.tobytes() and len(a) == 10
    assert list(a["parameter"]) == sorted(h.encode() for h in mem["header"])
    for f in FIELDS:
        _same(getattr(both["summary"], f), getattr(want, f), f)
    # two engines on one GPU, 3 + 3 chains: merged on the host, the same words
    two = sample_posterior(*args, None, **dict(kw, write_files=False, devices=[0, 0]))
    assert numpy.array_equal(two["rows"], mem["rows"])
    for f in FIELDS:
        _same(getattr(two["summary"], f), getattr(want, f), "two engines: " + f)
    # off by default: the directory and the dict as they were
    off_dir = str(tmp_path / "off")
    off = sample_posterior(*args, off_dir, **dict(kw, write_files=True, computeSummary=False))
    assert sorted(os.listdir(off_dir)) == ["log", "sample"]
    assert sorted(off) == ["accepted", "burn", "header", "loop_seconds", "row_index", "rows",
                           "thin"]
    assert numpy.array_equal(off["rows"], mem["rows"])


def test_too_few_values_raise_before_sampling(gpu_lib):
    from nestmc.sampler import record_iterations, sample_posterior, schedule
    args, kw = _api_case()
    assert len(record_iterations(1, *schedule(1, 1))) == 1
    with pytest.raises(ValueError, match="computeSummary"):
        sample_posterior(1, 1, 1, *args[3:], None, **dict(kw, write_files=False))


# ---- 8. the rank path of process_per_device -----------------------------------------------------
def test_process_per_device_rank_path(gpu_lib, tmp_path):
    """process_per_device: the rank sends its sorted columns over the host group and rank 0
    merges, finishes and writes -- with one rank the file and the result are the in-process
    path's bit for bit."""
    from nestmc.sampler import sample_posterior
    args, kw = _api_case()
    kw = dict(kw, devices=[0], computeDiagnostics=True)
    one, ppd = str(tmp_path / "one"), str(tmp_path / "ppd")
    r1 = sample_posterior(*args, one, **kw)
    r2 = sample_posterior(*args, ppd, process_per_device=True, **kw)
    assert numpy.array_equal(r1["rows"], r2["rows"])
    for f in FIELDS:
        _same(getattr(r1["summary"], f), getattr(r2["summary"], f), f)
    assert r1["assessment"].tobytes() == r2["assessment"].tobytes()
    assert open(os.path.join(one, "summary.csv"), "rb").read() == \
        open(os.path.join(ppd, "summary.csv"), "rb").read()
