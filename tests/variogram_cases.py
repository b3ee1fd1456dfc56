"""Inputs, references and bounds for nmc_k_variogram / nmc_variogram (csrc/diag.hip):
tests/test_variogram_cases.py holds them to account on the CPU, tests/test_gpu_variogram.py
runs the device on them.  numpy only; every array is built once, cached and read-only.

  V_t = sum_j sum_{q < n - t} (x_j[q + t] - x_j[q])^2 / (m (n - t)),  x [K][m][n], t < n.

Shapes (K, m, n).  The kernel runs 256 threads per block, ceil(n / 256) blocks per column, one
lag per thread, and stages one half-chain row of n doubles in LDS at a time, so n decides the
path: one block with idle threads (n < 256), exactly full blocks (256, 512, 8192), one lag
in a further block (257, 513), the LDS maximum of 64 KiB (8192) and the row below it; m = 1
never takes the `total + s` branch; K > 1 moves to the next column's offset.

Exact arithmetic.  exact_x holds multiples of 1/4 in [-8, 8]: a difference is a multiple of
1/4 of magnitude <= 16, a square a multiple of 1/16 <= 256, so a sum of m (n - t) <= 5 * 8192 of
them is an integer multiple of 1/16 below 5 * 8192 * 256 * 16 / 16: 5 * 2^25 < 2^28 sixteenths.
Every partial sum in any order is exact in float64 (53 bits), and the one division of two
exactly known numbers rounds the same everywhere: the device, numpy in any order and
variogram_host must agree bit for bit.  A wrong index, loop bound or a stale LDS row changes
the exact sum, so it changes the bits.

Tolerance columns against the numpy.longdouble reference: tests/convergence_ref.py's bound for
the sequential route, |V - V_ref| <= (n + m + 3) 2^-53 V_ref (3 u a square, n - 1 additions over
q, m - 1 over j, the division).  One missing pair costs about V_t / (m (n - t)) >= V_t / (m n)
relative, and (n + m + 3) 2^-53 < 1e-12 is far below 1 / (5 * 8192).

Lags: all of them below n = 8191; there the reference takes the ends, the block boundaries,
the middle and 32 seeded lags (the device still computes every lag; the exact case pins them
all at 513 and below).
"""

import functools

import numpy

LD = numpy.longdouble
U = 2.0 ** -53
F64_MAX = LD(numpy.finfo(numpy.float64).max)
N_MAX = 8192

# (K, m, n): every n of {1, 2, 3, 255, 256, 257, 511, 512, 513, 8191, 8192}, m of {1, 2, 3, 5},
# K of {1, 2, 7}
SHAPES = ((1, 1, 1), (2, 2, 1), (2, 1, 2), (7, 5, 2), (1, 3, 3), (7, 2, 3), (2, 5, 255),
          (7, 1, 256), (1, 2, 256), (2, 3, 257), (1, 5, 511), (7, 2, 512), (2, 3, 513),
          (1, 1, 513), (2, 2, 8191), (2, 2, 8192))
TOL_KINDS = ("normal", "offset", "walk", "scaled")   # the four columns of every tolerance case


def shape_id(s):
    return "K%d-m%d-n%d" % s


def _ro(a):
    a = numpy.ascontiguousarray(a)
    a.setflags(write=False)
    return a


def lags(n):
    """The lags the references are taken at."""
    if n < 8191:
        return _ro(numpy.arange(n))
    fixed = [0, 1, 2, 255, 256, 257, 4095, 4096, 4097, n - 3, n - 2, n - 1]
    seeded = numpy.random.RandomState(n).randint(0, n, size=32)
    return _ro(numpy.unique(numpy.concatenate([fixed, seeded])))


def exact_bits(m, n):
    """Bits of the largest possible sum of squares counted in sixteenths: m n squares of at
    most 256 = 4096 sixteenths each (see the module docstring)."""
    return int(m * n * 256 * 16).bit_length()


@functools.lru_cache(None)
def exact_x(shape):
    K, m, n = shape
    r = numpy.random.RandomState(7000 + 31 * n + 7 * m + K)
    return _ro(r.randint(-32, 33, size=(K, m, n)) / 4.0)


def numpy_v(x, at=None):
    """Plain numpy float64, numpy's own (pairwise) order: the exact cases' expected value."""
    x = numpy.asarray(x, dtype=numpy.float64)
    K, m, n = x.shape
    at = lags(n) if at is None else at
    V = numpy.empty((K, len(at)))
    for i, t in enumerate(at):
        d = x[:, :, t:] - x[:, :, :n - t]
        V[:, i] = numpy.sum(d * d, axis=(1, 2)) / (float(m) * float(n - t))
    return V


def int_v(x, at=None):
    """The exact cases in integer arithmetic: the sum of squares counted in sixteenths (int64),
    converted exactly, and the one float64 division."""
    xi = numpy.round(numpy.asarray(x) * 4).astype(numpy.int64)
    K, m, n = xi.shape
    at = lags(n) if at is None else at
    V = numpy.empty((K, len(at)))
    for i, t in enumerate(at):
        d = xi[:, :, t:] - xi[:, :, :n - t]
        S = numpy.sum(d * d, axis=(1, 2))
        assert numpy.all(S < 2 ** 28)
        V[:, i] = (S.astype(numpy.float64) / 16.0) / (float(m) * float(n - t))
    return V


def ld_v(x, at=None):
    """The numpy.longdouble reference; squares beyond the float64 range become inf, as float64
    arithmetic gives them (tests/store_cases.py does the same)."""
    X = numpy.asarray(x, dtype=numpy.float64).astype(LD)
    K, m, n = X.shape
    at = lags(n) if at is None else at
    V = numpy.empty((K, len(at)), dtype=LD)
    with numpy.errstate(all="ignore"):
        for i, t in enumerate(at):
            d = X[:, :, t:] - X[:, :, :n - t]
            sq = d * d
            sq = numpy.where(sq > F64_MAX, LD(numpy.inf), sq)
            V[:, i] = numpy.sum(sq, axis=(1, 2)) / (LD(m) * LD(n - t))
    return V


def bound(Vref, m, n):
    """(n + m + 3) u V_ref, in longdouble."""
    return LD((n + m + 3) * U) * numpy.abs(Vref)


def units(V, Vref, m, n):
    """max |V - V_ref| / (u V_ref) over the finite non-zero reference values (0 if none); where
    the reference is 0 the value must be 0 (else inf)."""
    V = numpy.asarray(V, dtype=numpy.float64).astype(LD)
    with numpy.errstate(all="ignore"):
        e = numpy.abs(V - Vref) / (LD(U) * numpy.abs(Vref))
    e = numpy.where(Vref == 0, numpy.where(V == 0, LD(0), LD(numpy.inf)), e)
    return float(numpy.max(e)) if e.size else 0.0


def _column(kind, m, n, r):
    if kind == "normal":
        return r.normal(size=(m, n))
    if kind == "offset":
        return 1e8 + 1e-3 * r.normal(size=(m, n))
    if kind == "walk":
        return numpy.cumsum(r.normal(size=(m, n)), axis=1)
    if kind == "scaled":      # half-chain j scaled by 10^j: the order of the sum over j matters
        return r.normal(size=(m, n)) * (10.0 ** numpy.arange(m))[:, None]
    raise ValueError(kind)


@functools.lru_cache(None)
def tol_x(m, n):
    """x [4][m][n]: one column of each of TOL_KINDS."""
    r = numpy.random.RandomState(9000 + 13 * n + m)
    return _ro(numpy.stack([_column(k, m, n, r) for k in TOL_KINDS]))


def tol_shapes():
    """The (m, n) of SHAPES, each once, in order."""
    seen = []
    for _, m, n in SHAPES:
        if (m, n) not in seen:
            seen.append((m, n))
    return seen


@functools.lru_cache(None)
def tol_ref(m, n):
    return _ro(ld_v(tol_x(m, n)))


# ---------------------------------------------------------------------------------------
# special columns between normal ones
# ---------------------------------------------------------------------------------------
SPECIAL_SHAPES = ((3, 513), (2, 3), (1, 300))            # (m, n); K = len(SPECIAL_LAYOUT)
SPECIAL_LAYOUT = ("normal", "const", "normal", "zeros", "normal", "denormal", "normal", "huge",
                  "normal", "nonfinite", "normal")


def special_rows(m, n):
    """(half-chain, row of the +inf cell, row of the NaN cell): the second half-chain where
    there is one, rows of at least 256 where n allows."""
    j = 1 if m > 1 else 0
    return (j, 400, 260) if n > 400 else (j, n - 1, 0)


@functools.lru_cache(None)
def special_x(m, n):
    """(x with the special columns, x with N(0, 1) in their place), each [11][m][n]."""
    r = numpy.random.RandomState(11000 + 17 * n + m)
    plain = numpy.stack([r.normal(size=(m, n)) for _ in SPECIAL_LAYOUT])
    x = plain.copy()
    for k, kind in enumerate(SPECIAL_LAYOUT):
        if kind == "const":
            x[k] = -3.7
        elif kind == "zeros":
            x[k] = numpy.where(r.randint(0, 2, size=(m, n)) == 1, 0.0, -0.0)
        elif kind == "denormal":
            x[k] = r.randint(-1000, 1001, size=(m, n)) * 5e-324
        elif kind == "huge":
            x[k] = numpy.where(r.randint(0, 2, size=(m, n)) == 1, 1e300, -1e300)
        elif kind == "nonfinite":
            j, r_inf, r_nan = special_rows(m, n)
            x[k, j, r_inf] = numpy.inf
            x[k, j, r_nan] = numpy.nan
    return _ro(x), _ro(plain)


def special_lags(n):
    """All lags; the float64 oracle (Python loops) takes these few."""
    if n <= 16:
        return _ro(numpy.arange(n))
    return _ro(numpy.unique(numpy.array([0, 1, 2, 100, 252, 253, 255, 256, 257, 260, 261, 300, 399,
                                         400, 401, n - 2, n - 1]) % n))


def check_special(V, m, n, at=None):
    """V [11][len(at)] (at: lags, default all) of special_x(m, n)[0] against what the issue of
    each special column demands; raises AssertionError naming the column."""
    x, _ = special_x(m, n)
    at = numpy.arange(n) if at is None else numpy.asarray(at)
    V = numpy.asarray(V, dtype=numpy.float64)
    assert V.shape == (len(SPECIAL_LAYOUT), len(at))
    ref = ld_v(x, at)
    for k, kind in enumerate(SPECIAL_LAYOUT):
        got = V[k]
        if kind in ("const", "zeros", "denormal"):
            # +0.0 bits: the float64 squares are +0 (the denormals' underflow; the longdouble
            # reference's do not, so the bits are asserted, not the bound)
            assert numpy.all(got.view(numpy.uint64) == 0), (kind, m, n, got[:8])
        elif kind == "huge":
            inf = numpy.isinf(ref[k])
            assert inf.any(), (kind, m, n)
            assert numpy.all(got[inf] == numpy.inf), (kind, m, n)
            assert numpy.all(got[~inf].astype(LD) == ref[k][~inf]), (kind, m, n)
        elif kind == "nonfinite":
            assert numpy.isnan(got[at == 0]).all(), (kind, m, n, "lag 0 is inf - inf")
            assert numpy.array_equal(numpy.isnan(got), numpy.isnan(ref[k])), (kind, m, n)
            assert numpy.array_equal(got == numpy.inf, ref[k] == numpy.inf), (kind, m, n)
            assert not numpy.any(got == -numpy.inf), (kind, m, n)
            fin = numpy.isfinite(ref[k])
            assert numpy.all(numpy.abs(got[fin].astype(LD) - ref[k][fin])
                             <= bound(ref[k][fin], m, n)), (kind, m, n)
        else:
            assert numpy.all(numpy.abs(got.astype(LD) - ref[k]) <= bound(ref[k], m, n)), (k, m, n)


# ---------------------------------------------------------------------------------------
# batching
# ---------------------------------------------------------------------------------------
BATCH_SHAPE = (7, 3, 257)       # 7 columns; a budget of 3 columns: batches of 3, 3 and 1
WIDE_SHAPE = (65537, 1, 2)      # more columns than gridDim.y allows: 1 MiB of input


def batch_plan(K, m, n, budget):
    """Columns per batch as nmc_variogram plans them: min(65535, budget / (m n 8), K), at least
    one; returns the list of batch sizes."""
    kb = max(1, min(65535, budget // (m * n * 8), K))
    return [min(kb, K - k0) for k0 in range(0, K, kb)]


@functools.lru_cache(None)
def batch_x():
    K, m, n = BATCH_SHAPE
    r = numpy.random.RandomState(12001)
    return _ro(numpy.stack([_column(TOL_KINDS[k % 4], m, n, r) for k in range(K)]))


@functools.lru_cache(None)
def wide_x():
    return _ro(numpy.random.RandomState(12002).normal(size=WIDE_SHAPE))
