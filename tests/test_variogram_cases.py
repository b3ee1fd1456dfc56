"""CPU: the cases of tests/variogram_cases.py held to account, without a GPU.

* the exactness bit budget of the exact cases, and that plain numpy, variogram_host and (at
  the small shapes) the float64 oracle agree on them bit for bit;
* nestmc.convergence.variogram_host -- the float64 restatement of the device's order -- stays
  within (n + m + 3) 2^-53 V of the longdouble reference on every tolerance case, so the
  bound the device is held to is one its own order of operations meets;
* the special columns' expectations are met by the float64 oracle (oracle/diagnosis.py) and
  by variogram_host, lag 0 included;
* nmc_variogram's argument checks (they return before any device call) and the batch plan.
"""

import numpy
import pytest

import variogram_cases as vc
from nestmc import convergence as conv
from oracle import diagnosis as od


def _oracle(x, at):
    with numpy.errstate(all="ignore"):
        return numpy.array([[od.variogram(x[k], int(t)) for t in at] for k in range(x.shape[0])],
                           dtype=numpy.float64)


def test_shapes_cover_the_issue_grid():
    assert numpy.finfo(numpy.longdouble).nmant >= 63        # the reference is wider than float64
    assert {n for _, _, n in vc.SHAPES} == {1, 2, 3, 255, 256, 257, 511, 512, 513, 8191, 8192}
    assert {m for _, m, _ in vc.SHAPES} == {1, 2, 3, 5}
    assert {K for K, _, _ in vc.SHAPES} == {1, 2, 7}
    assert 12 <= len(vc.SHAPES) <= 16 and len(set(vc.SHAPES)) == len(vc.SHAPES)
    for K, m, n in vc.SHAPES:
        assert n < 8191 or (K, m) == (2, 2)
        at = vc.lags(n)
        assert numpy.all(numpy.diff(at) > 0) and at[0] == 0 and at[-1] == n - 1
        if n >= 8191:
            assert 32 <= len(at) <= 44
            assert {0, 1, 2, 255, 256, 257, 4095, 4096, 4097, n - 3, n - 2, n - 1} <= set(at.tolist())
        else:
            assert len(at) == n
    assert max(n for _, _, n in vc.SHAPES) == vc.N_MAX


@pytest.mark.parametrize("shape", vc.SHAPES, ids=vc.shape_id)
def test_exact_cases_are_exact(shape):
    K, m, n = shape
    x = vc.exact_x(shape)
    assert x.shape == shape
    assert numpy.array_equal(x * 4, numpy.round(x * 4)) and numpy.max(numpy.abs(x)) <= 8
    if m * n > 4:
        assert len(numpy.unique(x)) > 4
    assert vc.exact_bits(m, n) <= 28 < 53
    at = vc.lags(n)
    want = vc.numpy_v(x, at)
    # nothing but the division rounds: integer arithmetic gives the same words
    assert numpy.array_equal(want.view(numpy.uint64), vc.int_v(x, at).view(numpy.uint64))
    host = conv.variogram_host(x, at)
    assert numpy.array_equal(host.view(numpy.uint64), want.view(numpy.uint64))
    if n <= 257:                                                         # (Python loops)
        sub = at if n <= 3 else at[[0, 1, 2, n // 2, n - 2, n - 1]]
        assert numpy.array_equal(_oracle(x, sub), vc.numpy_v(x, sub))


def test_variogram_host_lags_select_columns():
    x = vc.tol_x(3, 257)
    full = conv.variogram_host(x)
    at = [0, 5, 256]
    assert numpy.array_equal(conv.variogram_host(x, at), full[:, at])
    assert numpy.all(full[:, 0] == 0)


@pytest.mark.parametrize("mn", vc.tol_shapes(), ids=lambda mn: "m%d-n%d" % mn)
def test_variogram_host_within_bound_of_longdouble(mn):
    m, n = mn
    x = vc.tol_x(m, n)
    assert x.shape == (len(vc.TOL_KINDS), m, n) and numpy.all(numpy.isfinite(x))
    at = vc.lags(n)
    ref = vc.tol_ref(m, n)
    V = conv.variogram_host(x, at)
    worst = [vc.units(V[k], ref[k], m, n) for k in range(len(vc.TOL_KINDS))]
    print("variogram_host m=%d n=%d: worst |V - V_ref| / (u V_ref) per kind %s, bound %d"
          % (m, n, ["%.1f" % w for w in worst], n + m + 3))
    assert numpy.all(numpy.abs(V.astype(vc.LD) - ref) <= vc.bound(ref, m, n))
    if n > 1:
        assert numpy.all(ref[:, 1:] > 0)
    # the bound is far below what one missing pair would cost
    assert (n + m + 3) * vc.U < 0.01 / (m * n)


@pytest.mark.parametrize("mn", vc.SPECIAL_SHAPES, ids=lambda mn: "m%d-n%d" % mn)
def test_special_columns_expectations_hold_for_the_oracle_and_the_host(mn):
    m, n = mn
    x, plain = vc.special_x(m, n)
    assert x.shape == plain.shape == (len(vc.SPECIAL_LAYOUT), m, n)
    normal = [k for k, kind in enumerate(vc.SPECIAL_LAYOUT) if kind == "normal"]
    assert numpy.array_equal(x[normal], plain[normal]) and numpy.all(numpy.isfinite(plain))
    j, r_inf, r_nan = vc.special_rows(m, n)
    k = vc.SPECIAL_LAYOUT.index("nonfinite")
    assert x[k, j, r_inf] == numpy.inf and numpy.isnan(x[k, j, r_nan])
    assert numpy.sum(~numpy.isfinite(x)) == 2
    if n > 400:
        assert j == 1 and r_inf >= 256 and r_nan >= 256
    assert numpy.any(numpy.signbit(x[vc.SPECIAL_LAYOUT.index("zeros")]))
    d = x[vc.SPECIAL_LAYOUT.index("denormal")]
    assert numpy.any(d != 0) and numpy.max(numpy.abs(d)) < 2.0 ** -1022
    at = vc.special_lags(n)
    vc.check_special(_oracle(x, at), m, n, at)
    host = conv.variogram_host(x)
    vc.check_special(host, m, n)
    # the non-finite column has all three kinds of lag where the rows allow it
    if n > 400:
        assert numpy.isnan(host[k]).any() and numpy.isinf(host[k]).any() \
            and numpy.isfinite(host[k]).any()


def test_batch_plan():
    K, m, n = vc.BATCH_SHAPE
    col = m * n * 8
    assert vc.batch_plan(K, m, n, 3 * col) == [3, 3, 1]
    assert vc.batch_plan(K, m, n, 3 * col + col - 1) == [3, 3, 1]
    assert vc.batch_plan(K, m, n, 1) == [1] * 7                 # at least one column
    assert vc.batch_plan(K, m, n, 256 << 20) == [7]
    assert vc.batch_plan(*vc.WIDE_SHAPE, 256 << 20) == [65535, 2]
    assert vc.wide_x().nbytes == 65537 * 2 * 8


def test_variogram_arguments():
    """The argument checks come before any device call: they run without a GPU."""
    from nestmc import _lib
    lib = _lib.load()
    x = numpy.zeros(8)
    for K, m, n in ((-1, 1, 1), (1, 0, 1), (1, 1, 0), (1, -3, 4), (1, 1, -1), (1, 1, 8193)):
        out = numpy.full(8, -7.5)
        assert lib.nmc_variogram(0, _lib.dptr(x), K, m, n, _lib.dptr(out)) == -1, (K, m, n)
        assert b"variogram" in lib.nmc_last_error()
        assert numpy.all(out == -7.5)
    out = numpy.full(8, -7.5)
    assert lib.nmc_variogram(0, _lib.dptr(x), 0, 2, 4, _lib.dptr(out)) == 0
    assert numpy.all(out == -7.5)
