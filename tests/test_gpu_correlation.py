"""nmc_k_col_moments / nmc_k_comoment (csrc/comoment.h) against numpy and the longdouble
reference of correlation_ref.

The exact-arithmetic cases are what catch layout, indexing and padding mistakes: their stores
hold multiples of 1/4 in [-8, 8] and S is a power of two, so every sum is exact in any order,
with or without fusion, and the device must equal numpy's float64 bit for bit.  The shapes sit
at the kernel's edges -- one MFMA block (cols 15, 16, 17), one workgroup tile (64, 65), three
tiles with all six tile pairs (130), a chain chunk that is padding only, a partial chunk, K
slices with a last one that is not full -- not at workload size.  The tolerance cases cover the
shapes that cannot be exact, with the bound derived in correlation_ref."""

import ctypes
import os

import numpy
import pytest

import correlation_ref as cr
from gpu_cases import synthetic
from nestmc import _lib
from nestmc import correlation as co
from nestmc.engine import Engine

pytestmark = pytest.mark.gpu

I64 = ctypes.POINTER(ctypes.c_int64)
SENT, SENT64 = -7.25e77, -7777
SLICE_ROWS = 12            # NMC_CM_SLICE_ROWS of csrc/comoment.h: recorded rows per K-slice


def cm_of(lib, x, n_valid, rows=None, cols=None, C=None):
    """nmc_comoments_of on x [rows][cols][C]: (rc, part dict); the outputs start as sentinels."""
    r, k, c = x.shape
    cols = k if cols is None else cols
    mean = numpy.full(max(cols, 1), SENT)
    mm = numpy.full((2, max(cols, 1)), SENT)
    nm = cols if 1 <= cols <= 1024 else 1          # (a refused call writes nothing)
    M = numpy.full((nm, nm), SENT)
    bad = numpy.full(max(cols, 1), SENT64, dtype=numpy.int64)
    rc = lib.nmc_comoments_of(0, _lib.dptr(x), r if rows is None else rows, cols,
                              c if C is None else C, n_valid, _lib.dptr(mean), _lib.dptr(mm),
                              _lib.dptr(M), bad.ctypes.data_as(I64))
    return rc, dict(mean=mean, min=mm[0], max=mm[1], M=M, nonfinite=bad,
                    n_samples=(r if rows is None else rows) * n_valid)


def untouched(p):
    return bool((p["mean"] == SENT).all() and (p["min"] == SENT).all()
                and (p["max"] == SENT).all() and (p["M"] == SENT).all()
                and (p["nonfinite"] == SENT64).all())


def bits(a):
    return numpy.ascontiguousarray(a, dtype=numpy.float64).view(numpy.int64)


def same_bits(a, b, keys=("mean", "min", "max", "M")):
    for k in keys:
        assert numpy.array_equal(bits(a[k]), bits(b[k])), k
    assert numpy.array_equal(a["nonfinite"], b["nonfinite"])


def numpy_f64(x, nv):
    """mean, M, min, max in plain float64 (exact on the exact stores, in any order)."""
    rows, cols, C = x.shape
    X = numpy.transpose(x[:, :, :nv], (1, 0, 2)).reshape(cols, rows * nv)
    mean = X.sum(axis=1) / (rows * nv)
    d = X - mean[:, None]
    return mean, d @ d.T, X.min(axis=1), X.max(axis=1)


def exact_store(seed, rows, cols, C, nv):
    r = numpy.random.RandomState(seed)
    x = r.randint(-32, 33, size=(rows, cols, C)) / 4.0
    x[:, :, nv:] = numpy.nan                  # padding chains: never read
    return x


def check_exact(lib, x, nv):
    rc, got = cm_of(lib, x, nv)
    assert rc == 0, lib.nmc_last_error()
    mean, M, mn, mx = numpy_f64(x, nv)
    assert numpy.array_equal(got["mean"], mean), "mean"
    assert numpy.array_equal(got["min"], mn) and numpy.array_equal(got["max"], mx)
    bad = numpy.argwhere(got["M"] != M)
    assert bad.size == 0, "M differs at %s ..." % bad[:4].tolist()
    assert numpy.array_equal(bits(got["M"]), bits(got["M"].T))
    assert not got["nonfinite"].any()


# ---- 1. exact arithmetic ------------------------------------------------------------------------
# Values are multiples of 2^-2 in [-8, 8] and S = 1024: the sum is a multiple of 2^-2 below 2^13
# (exact), mean = sum / 2^10 exact, every centred value a multiple of 2^-12 below 2^4 (17 bits),
# every product a multiple of 2^-24 below 2^8 (32 bits), every partial sum of <= 1024 of them
# fits 42 bits.
@pytest.mark.parametrize("rows,C,nv", [(16, 64, 64), (16, 70, 64), (8, 128, 128)])
@pytest.mark.parametrize("cols", [1, 15, 16, 17, 64, 65, 130])
def test_exact(gpu_lib, rows, C, nv, cols):
    assert rows * nv == 1024
    check_exact(gpu_lib, exact_store(cols * 7 + rows, rows, cols, C, nv), nv)


# (rows, C, nv): S = 2048 = 2^11 and 1024.  32 rows are K-slices of 12, 12 and 8 rows, 64 rows
# of 16 valid chains 5 slices of 12 and one of 4 (SLICE_ROWS = NMC_CM_SLICE_ROWS = 12: the last
# slice is not full), the second with a partial chain chunk (16 of 32) and padding beside it.
# Bit budget at S = 2^11: mean = sum / 2^11 is a multiple of 2^-13, centred values multiples of
# 2^-13 below 2^4 (17 bits), products multiples of 2^-26 below 2^8 (34 bits), sums of 2^11 of
# them below 2^19: 45 bits <= 53.
@pytest.mark.parametrize("rows,C,nv,cols", [(32, 64, 64, 65), (64, 20, 16, 17)])
def test_exact_k_slices(gpu_lib, rows, C, nv, cols):
    S = rows * nv
    assert S & (S - 1) == 0 and S <= 1 << 14
    assert rows > 2 * SLICE_ROWS and rows % SLICE_ROWS
    check_exact(gpu_lib, exact_store(rows + cols, rows, cols, C, nv), nv)


# ---- 2. tolerance cases -------------------------------------------------------------------------
@pytest.mark.parametrize("nv", [70, 65, 64])
@pytest.mark.parametrize("rows", [20, 3, 1])
def test_tolerance(gpu_lib, rows, nv):
    C, cols = 70, 42
    x = cr.store_case(rows * 100 + nv, rows, cols, C)
    rc, got = cm_of(gpu_lib, x, nv)
    assert rc == 0, gpu_lib.nmc_last_error()
    ref = cr.reference(x, nv)
    cr.check(got, ref, rows * nv, 4)
    if rows == 20:                           # the strongly correlated columns are seen as such
        res = co.finish(got)
        assert res.pair(3, 10) > 0.998 and res.pair(8, 29) < -0.998
        assert numpy.array_equal(numpy.diagonal(res.corr), numpy.ones(cols))


# ---- 3. padding is never read as data ---------------------------------------------------------
@pytest.mark.parametrize("nv", [65, 33])
def test_padding_never_read(gpu_lib, nv):
    x = cr.store_case(11, 5, 42, 70)
    outs = []
    for fill in (numpy.nan, 1e300, 0.0):
        y = x.copy()
        y[:, :, nv:] = fill
        rc, got = cm_of(gpu_lib, y, nv)
        assert rc == 0
        outs.append(got)
    same_bits(outs[0], outs[1])
    same_bits(outs[0], outs[2])
    assert numpy.isfinite(outs[0]["M"]).all() and not outs[0]["nonfinite"].any()
    # and the chain count C itself does not enter: the same values in a narrower store
    rc, narrow = cm_of(gpu_lib, numpy.ascontiguousarray(x[:, :, :nv]), nv)
    assert rc == 0
    same_bits(outs[0], narrow)


# ---- 4. row window through a context ----------------------------------------------------------
def small_engine(C, G=6, rows=16):
    fam, sizes, priors, pooling, names = synthetic("linreg_partial", C, G, 8)
    eng = Engine(fam, sizes, C, pooling, priors, seed=2)
    eng.set_schedule(rows, 0, 1)          # rows recorded rows; no run()
    return eng


def test_engine_row_window(gpu_lib):
    C, rows = 70, 16
    eng = small_engine(C, rows=rows)
    try:
        cols = eng.cols
        assert cols == 16
        x = cr.store_case(12, rows, cols, C)
        eng.set_samples_raw(x)
        for rb, nr, nv in ((4, 12, C), (0, rows, C), (3, 5, 65), (15, 1, 64)):
            got = eng.comoments(rb, nr, nv)
            rc, want = cm_of(gpu_lib, numpy.ascontiguousarray(x[rb:rb + nr]), nv)
            assert rc == 0
            same_bits(got, want)
            assert got["n_samples"] == nr * nv
        assert eng.event_elapsed_ms(2, 3) >= 0.0                   # slots 2 / 3 bracket the kernels
        res = eng.correlation(["n%d" % k for k in range(cols)], 4, 12)
        want = co.finish(eng.comoments(4, 12), ["n%d" % k for k in range(cols)])
        assert numpy.array_equal(res.corr, want.corr) and numpy.array_equal(res.cov, want.cov)
        assert res.n_samples == 12 * C
        for rb, nr, nv in ((-1, 2, C), (15, 2, C), (0, 17, C), (0, 0, C), (0, 16, 0),
                           (0, 16, C + 1), (0, 1, 1)):
            p = dict(mean=numpy.full(cols, SENT), mm=numpy.full((2, cols), SENT),
                     M=numpy.full((cols, cols), SENT), bad=numpy.full(cols, SENT64, numpy.int64))
            rc = eng.lib.nmc_comoments(eng.h, rb, nr, nv, _lib.dptr(p["mean"]), _lib.dptr(p["mm"]),
                                       _lib.dptr(p["M"]), p["bad"].ctypes.data_as(I64))
            assert rc == -1, (rb, nr, nv)
            assert all((p[k] == SENT).all() for k in ("mean", "mm", "M")), (rb, nr, nv)
            assert (p["bad"] == SENT64).all()
        with pytest.raises(_lib.NestmcError):
            eng.comoments(n_valid=C + 1)
    finally:
        eng.close()


def test_bad_arguments_of(gpu_lib):
    x = cr.store_case(1, 2, 3, 4)
    for kw in (dict(n_valid=0), dict(n_valid=5), dict(rows=0), dict(C=0), dict(cols=0),
               dict(rows=1, n_valid=1),                                     # S = 1
               dict(rows=65536, C=32768, n_valid=32768),                    # S = 2^31
               dict(cols=8193)):                                            # M + scratch > 1 GiB
        a = dict(n_valid=4, rows=None, cols=None, C=None)
        a.update(kw)
        rc, p = cm_of(gpu_lib, x, a["n_valid"], a["rows"], a["cols"], a["C"])
        assert rc == -1, kw
        assert untouched(p), kw
    assert b"1 GiB" in gpu_lib.nmc_last_error()


# ---- 5. special columns -------------------------------------------------------------------------
def test_special_columns(gpu_lib):
    rows, cols, C, nv = 6, 70, 66, 65
    x = cr.store_case(13, rows, cols, C)
    rc, base = cm_of(gpu_lib, x, nv)
    assert rc == 0
    k = 37
    others = numpy.array([c for c in range(cols) if c != k])

    def others_unchanged(got):
        assert numpy.array_equal(bits(got["M"][numpy.ix_(others, others)]),
                                 bits(base["M"][numpy.ix_(others, others)]))
        for key in ("mean", "min", "max"):
            assert numpy.array_equal(bits(got[key][others]), bits(base[key][others])), key
        assert not got["nonfinite"][others].any()

    y = x.copy()
    y[:, k, :] = 0.1                                   # constant (0.1 S / S need not be 0.1)
    rc, got = cm_of(gpu_lib, y, nv)
    assert rc == 0
    assert numpy.array_equal(bits(got["M"][k]), numpy.zeros(cols, numpy.int64))     # +0.0 bits
    assert numpy.array_equal(bits(got["M"][:, k]), numpy.zeros(cols, numpy.int64))
    assert got["min"][k] == got["max"][k] == 0.1 and got["nonfinite"][k] == 0
    others_unchanged(got)
    res = co.finish(got)
    assert numpy.isnan(res.corr[k]).all() and numpy.isnan(res.corr[:, k]).all()
    assert numpy.isfinite(res.corr[numpy.ix_(others, others)]).all()

    for cell, value in (((2, k, 64), numpy.nan), ((5, k, 0), numpy.inf)):
        y = x.copy()
        y[cell] = value
        y[0, k, 65] = numpy.nan                        # a padding chain: not counted
        rc, got = cm_of(gpu_lib, y, nv)
        assert rc == 0
        assert got["nonfinite"][k] == 1
        assert numpy.isnan(got["M"][k]).all() and numpy.isnan(got["M"][:, k]).all()
        assert numpy.isnan(got["mean"][k])
        others_unchanged(got)


def test_engine_nonfinite_raises(gpu_lib):
    C, rows = 66, 4
    eng = small_engine(C, rows=rows)
    try:
        x = cr.store_case(14, rows, eng.cols, C)
        x[1, 3, 7] = numpy.nan
        x[2, 9, 65] = -numpy.inf
        eng.set_samples_raw(x)
        assert eng.comoments()["nonfinite"].sum() == 2
        with pytest.raises(_lib.NestmcError, match="2 values were not finite"):
            eng.correlation()
        assert eng.correlation_nonfinite == 2
        ok = eng.correlation(row_begin=3, n_rows=1)                 # a clean window
        assert ok.n_samples == C
    finally:
        eng.close()


# ---- 6. determinism and symmetry --------------------------------------------------------------
def test_determinism_and_symmetry(gpu_lib):
    x = cr.store_case(15, 30, 130, 70)                 # three K-slices, six tile pairs
    rc, a = cm_of(gpu_lib, x, 67)
    rc2, b = cm_of(gpu_lib, x, 67)
    assert rc == 0 and rc2 == 0
    same_bits(a, b)
    assert numpy.array_equal(bits(a["M"]), bits(a["M"].T))
    cr.check(a, cr.reference(x, 67), 30 * 67, 4)


# ---- 7. sample_posterior(computeCorrelation=True) ---------------------------------------------
def _api_case():
    C, G, N = 66, 6, 20
    fam, sizes, priors, pooling, names = synthetic("linreg_partial", C, G, N)
    kw = dict(saveLogLikelihood=False, priorDistribution=priors,
              startingPointValueRange={n: [-0.5, 0.5] for n in names}, displayProgress=False,
              seed=17, return_samples=True, computeCorrelation=True)
    return (C, 60, 15, names, G, N, pooling, fam), kw        # burn 30, thin 2: 15 rows


@pytest.fixture(scope="module")
def one_run(gpu_lib, tmp_path_factory):
    """The one-engine run the other routes are compared with: (result, directory, reference)."""
    from nestmc.sampler import sample_posterior
    args, kw = _api_case()
    one_dir = str(tmp_path_factory.mktemp("correlation") / "one")
    one = sample_posterior(*args, one_dir, **kw)
    raw = numpy.ascontiguousarray(numpy.transpose(one["rows"], (1, 2, 0)))
    return one, one_dir, raw, cr.reference(raw)


def _within(res, ref, S, factor, what):
    rm, rv = cr.ratios(dict(M=res.cov * (S - 1), mean=res.mean), ref, S, factor)
    print("%s: M error / bound = %.3g, mean error / bound = %.3g" % (what, rm, rv))
    assert rm <= 1.0 and rv <= 1.0, (what, rm, rv)


def test_sample_posterior_correlation(one_run, tmp_path):
    from nestmc.sampler import sample_posterior
    one, one_dir, raw, ref = one_run
    C, G, S = 66, 6, 15 * 66
    res = one["correlation"]
    assert sorted(os.listdir(one_dir)) == [co.FILE_MATRIX, co.FILE_PAIRS, "log", "sample"]
    assert res.parameter == list(one["header"]) and res.n_samples == S
    assert raw.shape == (15, 2 * (G + 2), C)
    _within(res, ref, S, 4, "one engine")
    host = co.finish(co.comoments_from_samples(raw), res.parameter)
    assert numpy.abs(res.corr - host.corr).max() <= 24 * S * cr.U    # two results, each within
    assert numpy.array_equal(numpy.diagonal(res.corr), numpy.ones(16))  # 3 bounds of the truth
    back = co.read_csvs(one_dir)
    assert back["parameter"] == res.parameter
    assert numpy.abs(back["corr"] - res.corr).max() <= 0.5e-6          # %.6f
    rows = res.pairs(2, G, True)
    assert len(rows) == (2 + G) + 2 * 2 * G
    assert [b[:3] for b in back["pairs"]] == [w[:3] for w in rows]
    assert max(abs(b[3] - w[3]) for b, w in zip(back["pairs"], rows)) <= 0.5e-6
    assert rows[0][:3] == ("within_group", "b0_mu", "b1_mu")
    # without the option nothing changes: no key, no file
    args, kw = _api_case()
    off_dir = str(tmp_path / "off")
    off = sample_posterior(*args, off_dir, **dict(kw, computeCorrelation=False))
    assert sorted(os.listdir(off_dir)) == ["log", "sample"]
    assert sorted(off) == ["accepted", "burn", "header", "loop_seconds", "row_index", "rows",
                           "thin"]
    assert numpy.array_equal(off["rows"], one["rows"])


def test_sample_posterior_two_engines(one_run, tmp_path):
    """devices=[0, 0]: 33 + 33 chains, the parts merged by Chan's update in engine order."""
    from nestmc.sampler import sample_posterior
    one, one_dir, raw, ref = one_run
    args, kw = _api_case()
    two_dir = str(tmp_path / "two")
    two = sample_posterior(*args, two_dir, **dict(kw, devices=[0, 0]))
    assert numpy.array_equal(two["rows"], one["rows"])
    _within(two["correlation"], ref, 15 * 66, 8, "two engines")
    assert os.path.exists(os.path.join(two_dir, co.FILE_PAIRS))


def test_sample_posterior_process_per_device(one_run, tmp_path):
    """process_per_device: the rank's part travels as bytes over the host group to rank 0."""
    from nestmc.sampler import sample_posterior
    one, one_dir, raw, ref = one_run
    args, kw = _api_case()
    ppd_dir = str(tmp_path / "ppd")
    ppd = sample_posterior(*args, ppd_dir, **dict(kw, devices=[0], process_per_device=True))
    assert numpy.array_equal(ppd["rows"], one["rows"])
    _within(ppd["correlation"], ref, 15 * 66, 8, "process_per_device")
    back = co.read_csvs(ppd_dir)
    assert numpy.abs(back["corr"] - ppd["correlation"].corr).max() <= 0.5e-6
