"""Rank-normalised R-hat, bulk- and tail-ESS on the GPU: nmc_k_rank_transform (csrc/rankz.h)
between the column sort and nmc_k_conv (nmc_rank_partials / nmc_rank_partials_of,
Engine.rank_partials / rank_diagnostics, samplePosterior(computeRankDiagnostics=True)).

Reference: tests/rankdiag_ref.py -- the exact quantities by numpy's sort and searchsorted,
compared as words; the normal score against mpmath at 50 digits within NDTRI_C u |z|; the
partials bit for bit against convergence_ref.partials of the device's own derived values; the
finished numbers against the host route (nestmc.rankdiag.from_rows) within the derived
bounds."""

import ctypes
import os

import numpy
import pytest

import convergence_ref as cr
import rankdiag_ref as rr
from nestmc import _lib
from nestmc import rankdiag as rd
from test_gpu_convergence import _api_case, _engine
from test_rankdiag_host import check_routes

pytestmark = pytest.mark.gpu

_i64 = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))   # noqa: E731


def _of(lib, xs, n_valid, col_batch=0, inside=True):
    """nmc_rank_partials_of over xs [rows][cols][C]: dict of vg, mean, m2, nonfinite and,
    with inside, derived, twice_rank and zeta."""
    xs = numpy.ascontiguousarray(xs, dtype=numpy.float64)
    R, K, C = xs.shape
    n, CB = R // 2, (C + 63) // 64
    out = dict(vg=numpy.empty((4, CB, K, n)), mean=numpy.empty((4, K, 2, C)),
               m2=numpy.empty((4, K, 2, C)), nonfinite=numpy.empty(K, dtype=numpy.int64),
               derived=numpy.empty((4, R, K, C)) if inside else None,
               twice_rank=numpy.empty((2, R, K, C), dtype=numpy.int64) if inside else None,
               zeta=numpy.empty((R, K, C)) if inside else None)
    _lib.check(lib.nmc_rank_partials_of(
        0, _lib.dptr(xs), R, K, C, int(n_valid), int(col_batch), _lib.dptr(out["vg"]),
        _lib.dptr(out["mean"]), _lib.dptr(out["m2"]), _i64(out["nonfinite"]),
        _lib.dptr(out["derived"]), None if not inside else _i64(out["twice_rank"]),
        _lib.dptr(out["zeta"])))
    return out


def _same(a, b, what):
    a, b = numpy.ascontiguousarray(a), numpy.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape)
    bad = a.view(numpy.uint64) != b.view(numpy.uint64)
    assert not bad.any(), "%s: %d of %d words differ, first at %s (%r against %r)" % (
        what, bad.sum(), bad.size, numpy.argwhere(bad)[0], a[bad][0], b[bad][0])


def _check_scores(z, r2, N, what):
    """Device scores z with twice-ranks r2 (flat, one column's or several of N values):
    every element against the float64 restatement within (NDTRI_C - NDTRI_C / 8) u |z| (the
    restatement is within NDTRI_C / 8 u of the exact score: NDTRI_C u in all), the probes
    against mpmath within NDTRI_C u |z|, and z = 0 exactly at p = 1/2."""
    p = rr.p_of(r2, N)
    rest = rr.ndtri_as241(p)
    err = numpy.abs(z - rest)
    bound = 0.875 * rr.NDTRI_C * rr.U * numpy.abs(rest)
    assert numpy.all(err <= bound), (what, float(numpy.max(err / numpy.maximum(bound, 1e-300))))
    mid = p == 0.5
    assert numpy.all(z[mid] == 0.0) and not numpy.signbit(z[mid]).any(), what
    u, first = numpy.unique(r2, return_index=True)
    pick = first[numpy.isin(u, rr.probe_r2(N))]
    ratio = rr.ratio_to_exact(z[pick], p[pick])
    print("ndtri %s: %d probes, worst %.3g u (bound %g u); against the restatement worst "
          "%.3g u" % (what, len(pick), ratio.max(), rr.NDTRI_C,
                      float(numpy.max(err[~mid] / (rr.U * numpy.abs(rest[~mid]))))
                      if (~mid).any() else 0.0))
    assert ratio.max() <= rr.NDTRI_C, (what, ratio.max())


def _check_exact(out, xs, nv, what, partials):
    R, K, C = xs.shape
    N = R * nv
    want = rr.derive(xs, nv)
    ok = want["nonfinite"] == 0
    assert list(want["nonfinite"][-2:]) == [1, 1] and ok[:-2].all()
    _same(out["nonfinite"], want["nonfinite"], what + " nonfinite")
    _same(out["twice_rank"], want["twice_rank"], what + " twice_rank")
    d = out["derived"]
    _same(out["zeta"][:, ok], want["zeta"][:, ok], what + " zeta")
    assert numpy.all(numpy.isnan(out["zeta"][:, ~ok, :nv])) and not out["zeta"][:, :, nv:].any()
    assert N < 6 or numpy.isinf(want["zeta"][:, 6]).any(), what    # (the overflow column)
    _same(d[2][:, ok], want["I05"][:, ok], what + " I05")
    _same(d[3][:, ok], want["I95"][:, ok], what + " I95")
    assert numpy.all(numpy.isnan(d[:, :, ~ok, :nv])), what
    assert not d[:, :, :, nv:].any(), what            # (padding chains: +0.0)
    for t, name in ((0, "z"), (1, "zf")):
        z = d[t][:, ok, :nv].reshape(-1)
        r2 = want["twice_rank"][t][:, ok, :nv].reshape(-1)
        _check_scores(z, r2, N, "%s %s" % (what, name))
    if partials:
        # the unchanged nmc_k_conv on a buffer in store layout: the restatement of its fixed
        # order over the device's own derived values, bit for bit
        for t, name in enumerate(rd.QUANTITIES):
            rows = numpy.ascontiguousarray(numpy.transpose(d[t][:, ok], (2, 0, 1)))
            vg, mean, m2 = cr.partials(rows, nv)
            _same(out["vg"][t][:, ok], vg, "%s vg(%s)" % (what, name))
            _same(out["mean"][t][ok], mean, "%s mean(%s)" % (what, name))
            _same(out["m2"][t][ok], m2, "%s m2(%s)" % (what, name))
            assert numpy.all(numpy.isnan(out["vg"][t][0][~ok][:, 1:]))
            assert numpy.all(numpy.isnan(out["mean"][t][~ok][:, :, :nv]))


# ---- 1. the exact quantities, the scores and the partials ------------------------------------
@pytest.mark.parametrize("rows,C,nv", rr.SHAPES)
def test_exact_scores_and_partials(gpu_lib, rows, C, nv):
    xs = rr.store(rows, C, nv, seed=rows + nv)
    out = _of(gpu_lib, xs, nv)
    _check_exact(out, xs, nv, "%d x %d of %d" % (rows, nv, C), partials=rows <= 100)


# ---- 2. batching -------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,C,nv", [(100, 70, 60), (4098, 1, 1)])
def test_col_batch_changes_no_word(gpu_lib, rows, C, nv):
    xs = rr.store(rows, C, nv, seed=7)
    a = _of(gpu_lib, xs, nv, 0)
    for cb in (1, 2, 3):
        b = _of(gpu_lib, xs, nv, cb)
        for k in a:
            _same(a[k], b[k], "col_batch %d %s" % (cb, k))


# ---- 3. the engine: window, arguments, finished numbers ------------------------------------
@pytest.fixture(scope="module")
def eng70(gpu_lib):
    eng = _engine("linreg_partial", 70, 5, 30)
    assert eng.n_rows == 10 and eng.cols == 14
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def eng70_100(gpu_lib):
    eng = _engine("linreg_partial", 70, 5, 30, (120, 20, 1))
    assert eng.n_rows == 100
    yield eng
    eng.close()


def test_window_and_arguments(gpu_lib, eng70):
    eng = eng70
    for kw in (dict(row_begin=2, n_rows=6), dict(row_begin=6, n_rows=4), dict(),
               dict(row_begin=2, n_rows=8, n_valid=60)):
        vg, mean, m2, bad = eng.rank_partials(**kw)
        r0, nr = kw.get("row_begin", 0), kw.get("n_rows", eng.n_rows - kw.get("row_begin", 0))
        nv = kw.get("n_valid", 70)
        ref = _of(gpu_lib, eng.samples_raw(r0, nr), nv)
        _same(vg, ref["vg"], "vg %r" % kw)
        _same(mean, ref["mean"], "mean %r" % kw)
        _same(m2, ref["m2"], "m2 %r" % kw)
        _same(bad, ref["nonfinite"], "nonfinite %r" % kw)
        assert vg.shape == (4, 2, 14, nr // 2) and not bad.any()
        want = rr.derive(eng.samples_raw(r0, nr), nv)
        _same(ref["twice_rank"], want["twice_rank"], "twice_rank %r" % kw)
    for kw in (dict(row_begin=2, n_rows=5), dict(row_begin=0, n_rows=2), dict(n_rows=0),
               dict(row_begin=8, n_rows=4), dict(row_begin=-2, n_rows=4),
               dict(row_begin=0, n_rows=12), dict(n_valid=0), dict(n_valid=71),
               dict(col_batch=-1)):
        with pytest.raises(_lib.NestmcError):
            eng.rank_partials(**kw)
    eng.rank_partials()                                   # (the context still works)


def test_against_host_route(eng70, eng70_100):
    for eng, what in ((eng70, "n = 5"), (eng70_100, "n = 50")):
        res = eng.rank_diagnostics()
        rows = eng.samples()
        assert res.m == 140 and res.n == eng.n_rows // 2 and len(res.parameter) == 14
        host = rd.from_rows(rows)
        check_routes(res, host, rows, 2, what)
        assert not res.nonfinite.any()
        print("rank diagnostics %s: rhat %.4f..%.4f, ess_bulk %.1f..%.1f, ess_tail %.1f..%.1f"
              % (what, res.rhat.min(), res.rhat.max(), res.ess_bulk.min(), res.ess_bulk.max(),
                 res.ess_tail.min(), res.ess_tail.max()))


# ---- 4. samplePosterior(computeRankDiagnostics=True) -------------------------------------------
def _case():
    args, kw = _api_case()
    kw = dict(kw, computeDiagnostics=False, computeRankDiagnostics=True)
    return args, kw


def test_sample_posterior_compute_rank_diagnostics(gpu_lib, tmp_path):
    from nestmc.sampler import sample_posterior
    args, kw = _case()
    mem =sample_posterior(*args, None, **dict(kw, write_files=False))
    res = mem["rank_diagnostics"]
    assert mem["rows"].shape == (6, 16, 10) and res.parameter == list(mem["header"])
    assert (res.n, res.m, res.N) == (8, 12, 96)
    # Engine.rank_diagnostics on the same run: the partials of the same rows, finished alike
    xs = numpy.ascontiguousarray(numpy.transpose(mem["rows"], (1, 2, 0)))
    ref = _of(gpu_lib, xs, 6, inside=False)
    want = rd.finish(ref["vg"], ref["mean"], ref["m2"], 8, mem["header"], 6, ref["nonfinite"])
    for k in ("rhat", "rhat_bulk", "rhat_folded", "ess_bulk", "ess_tail", "tau"):
        _same(getattr(res, k), getattr(want, k), k)
    out = str(tmp_path / "one")
    one = sample_posterior(*args, out, **dict(kw, write_files=True))
    assert sorted(os.listdir(out)) == ["log", "rank_diagnostics.csv", "sample"]
    assert open(os.path.join(out, "rank_diagnostics.csv")).read() == rd.csv_text(res)
    assert rd.csv_text(one["rank_diagnostics"]) == rd.csv_text(res)
    off = sample_posterior(*args, None, **dict(kw, write_files=False,
                                                computeRankDiagnostics=False))
    assert "rank_diagnostics" not in off
    assert numpy.array_equal(off["rows"], mem["rows"])
    assert numpy.array_equal(one["rows"], mem["rows"])


def test_odd_row_count_raises(gpu_lib):
    from nestmc.sampler import sample_posterior
    args, kw = _case()
    with pytest.raises(ValueError):                       # 15 recorded rows
        sample_posterior(args[0], 60, 20, *args[3:], None, **dict(kw, write_files=False))
    with pytest.raises(ValueError):                       # two rows: halves of one row
        sample_posterior(args[0], 4, 2, *args[3:], None, **dict(kw, write_files=False))


@pytest.mark.parametrize("extra", [dict(devices=[0, 0]), dict(chains=[0, 1, 2]),
                                   dict(devices=[0], process_per_device=True)])
def test_several_engines_not_implemented(gpu_lib, extra):
    from nestmc.sampler import sample_posterior
    args, kw = _case()
    with pytest.raises(NotImplementedError):
        sample_posterior(*args, None, **dict(kw, write_files=False, **extra))
