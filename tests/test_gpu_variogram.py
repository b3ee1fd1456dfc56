"""GPU: nmc_k_variogram / nmc_variogram (csrc/diag.hip) on the cases of tests/variogram_cases.py.

* exact cases: the device equals plain numpy float64 bit for bit at every shape (any wrong
  index, loop bound or stale LDS row changes an exactly representable sum);
* tolerance cases: within (n + m + 3) 2^-53 V of the numpy.longdouble reference, and bit for
  bit nestmc.convergence.variogram_host's numbers, lag 0 included;
* special columns (constant, signed zeros, denormals, +-1e300, one +inf and one NaN cell)
  between normal ones: their own expectations, and the normal columns' words unchanged from
  the run in which N(0, 1) stands in the special columns' place;
* batches of columns: a shrunk byte budget (NMC_VARIO_BATCH_BYTES) and more columns than one
  grid holds give the one-batch words;
* arguments: the sentinel survives every refused call and K = 0.

Worst |V - V_ref| / (2^-53 V_ref) measured on the device per tolerance case: DESIGN 3.6.1.
"""

import numpy
import pytest

import variogram_cases as vc
from nestmc import _lib, convergence as conv, diagnosis

pytestmark = pytest.mark.gpu


def _words(a):
    return numpy.ascontiguousarray(a, dtype=numpy.float64).view(numpy.uint64)


def _same_words(a, b):
    """Bit for bit; any NaN equals any NaN."""
    a, b = numpy.asarray(a), numpy.asarray(b)
    return bool(numpy.all((_words(a) == _words(b)) | (numpy.isnan(a) & numpy.isnan(b))))


@pytest.mark.parametrize("shape", vc.SHAPES, ids=vc.shape_id)
def test_exact_cases_bit_for_bit(gpu_lib, shape):
    K, m, n = shape
    x = vc.exact_x(shape)
    at = vc.lags(n)
    got = diagnosis.variogram(x)
    assert got.shape == (K, n)
    want = vc.numpy_v(x, at)
    bad = numpy.argwhere(_words(got[:, at]) != _words(want))
    assert bad.size == 0, (shape, bad[:5], got[:, at][tuple(bad[0])], want[tuple(bad[0])])


@pytest.mark.parametrize("mn", vc.tol_shapes(), ids=lambda mn: "m%d-n%d" % mn)
def test_tolerance_cases_within_bound_and_equal_to_host(gpu_lib, mn):
    m, n = mn
    x = vc.tol_x(m, n)
    at = vc.lags(n)
    ref = vc.tol_ref(m, n)
    got = diagnosis.variogram(x)[:, at]
    worst = [vc.units(got[k], ref[k], m, n) for k in range(len(vc.TOL_KINDS))]
    print("nmc_variogram m=%d n=%d: worst |V - V_ref| / (u V_ref) per kind %s, bound %d"
          % (m, n, ["%.1f" % w for w in worst], n + m + 3))
    err = numpy.abs(got.astype(vc.LD) - ref)
    assert numpy.all(err <= vc.bound(ref, m, n)), (mn, worst)
    host = conv.variogram_host(x, at)
    assert numpy.all(numpy.isfinite(host))
    bad = numpy.argwhere(_words(got) != _words(host))
    assert bad.size == 0, (mn, bad[:5])


@pytest.mark.parametrize("mn", vc.SPECIAL_SHAPES, ids=lambda mn: "m%d-n%d" % mn)
def test_special_columns(gpu_lib, mn):
    m, n = mn
    x, plain = vc.special_x(m, n)
    got = diagnosis.variogram(x)
    vc.check_special(got, m, n)
    assert _same_words(got, conv.variogram_host(x))
    # nothing leaks between columns, or between the blocks of one column
    base = diagnosis.variogram(plain)
    for k, kind in enumerate(vc.SPECIAL_LAYOUT):
        if kind == "normal":
            assert numpy.array_equal(_words(got[k]), _words(base[k])), (mn, k)
    assert _same_words(base, conv.variogram_host(plain))


def test_batches_give_the_one_batch_words(gpu_lib, monkeypatch):
    K, m, n = vc.BATCH_SHAPE
    x = vc.batch_x()
    monkeypatch.delenv("NMC_VARIO_BATCH_BYTES", raising=False)
    one = diagnosis.variogram(x)
    assert _same_words(one, conv.variogram_host(x))
    col = m * n * 8
    for budget in (3 * col, 2 * col + 1, col, 1):     # 3+3+1, 2+2+2+1, and one column at a time
        plan = vc.batch_plan(K, m, n, budget)
        assert len(plan) >= 3 and sum(plan) == K
        monkeypatch.setenv("NMC_VARIO_BATCH_BYTES", str(budget))
        many = diagnosis.variogram(x)
        assert numpy.array_equal(_words(many), _words(one)), budget
    assert vc.batch_plan(K, m, n, 3 * col) == [3, 3, 1]
    monkeypatch.setenv("NMC_VARIO_BATCH_BYTES", "0")      # not positive: the default budget
    assert numpy.array_equal(_words(diagnosis.variogram(x)), _words(one))


def test_more_columns_than_one_grid(gpu_lib, monkeypatch):
    monkeypatch.delenv("NMC_VARIO_BATCH_BYTES", raising=False)
    x = vc.wide_x()
    assert x.shape == (65537, 1, 2)
    got = diagnosis.variogram(x)
    want = conv.variogram_host(x)
    bad = numpy.flatnonzero(numpy.any(_words(got) != _words(want), axis=1))
    assert bad.size == 0, bad[:5]


def test_arguments(gpu_lib):
    x = numpy.zeros(8)
    for K, m, n in ((-1, 1, 1), (1, 0, 1), (1, 1, 0), (1, 1, 8193)):
        out = numpy.full(8, -7.5)
        assert gpu_lib.nmc_variogram(0, _lib.dptr(x), K, m, n, _lib.dptr(out)) == -1, (K, m, n)
        assert numpy.all(out == -7.5)
    out = numpy.full(8, -7.5)
    assert gpu_lib.nmc_variogram(0, _lib.dptr(x), 0, 2, 4, _lib.dptr(out)) == 0
    assert numpy.all(out == -7.5)
    # and the largest n is accepted: one column of the documented maximum
    x = vc.exact_x((2, 2, 8192))[:1, :1]
    assert numpy.array_equal(diagnosis.variogram(x)[:, [0, 8191]], vc.numpy_v(x, [0, 8191]))
