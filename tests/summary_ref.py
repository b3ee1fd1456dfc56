"""The restatement, in numpy, of the columns' sort and order statistics (csrc/sortcol.h,
nmc_summary), written from their definition:

  key(b)      a double's bits b as a uint64 that orders like the number: ~b when the sign is
              set, b | 1 << 63 otherwise; -inf < ... < -0.0 < +0.0 < ... < +inf < +NaN
  sorted_ref  column k of a store [row][col][C] over the rows [row_begin, row_begin + n_rows)
              and the chains [0, n_valid): its N = n_rows * n_valid values in key order
  stats_ref   of one sorted column s: the median (the middle value, or numpy.mean of the two
              middle ones), the interval (s[i], s[i + gap]) of the FIRST i in [0, N - gap) that
              minimises the fp64 difference s[i + gap] - s[i], that i, and s at given ranks;
              a column with a NaN or an infinity: NaN everywhere and i = -1

Order statistics depend on the multiset alone, so the device must give these bits exactly."""

import numpy

T = 4096   # csrc/sortcol.h NMC_SORT_TILE: the keys of one LDS tile

_TOP = numpy.uint64(1 << 63)
_ABS = numpy.uint64((1 << 63) - 1)


def key(x):
    b = numpy.ascontiguousarray(x, dtype=numpy.float64).view(numpy.uint64)
    neg = (b >> numpy.uint64(63)) == 1
    return numpy.where(neg, ~b, b | _TOP)


def unkey(k):
    k = numpy.ascontiguousarray(k, dtype=numpy.uint64)
    pos = (k >> numpy.uint64(63)) == 1
    return numpy.where(pos, k & _ABS, ~k).view(numpy.float64)


def sorted_ref(store, row_begin=0, n_rows=None, n_valid=None):
    """store [rows][cols][C] -> [cols][N], every column's values in key order."""
    store = numpy.asarray(store, dtype=numpy.float64)
    rows, cols, C = store.shape
    n_rows = rows - row_begin if n_rows is None else n_rows
    n_valid = C if n_valid is None else n_valid
    w = store[row_begin:row_begin + n_rows, :, :n_valid]
    flat = numpy.ascontiguousarray(numpy.transpose(w, (1, 0, 2))).reshape(cols, n_rows * n_valid)
    return unkey(numpy.sort(key(flat), axis=1))


def gap_ref(N, hdi_p=95):
    return max(1, min(N - 1, round(N * (hdi_p / 100.))))


def stats_ref(s, gap, ranks=()):
    """One sorted column -> dict(median, lower, upper, at, ranks' values, nonfinite)."""
    s = numpy.asarray(s, dtype=numpy.float64)
    N = len(s)
    bad = int(numpy.sum(~numpy.isfinite(s)))
    if bad:
        nan = numpy.nan
        return dict(median=nan, lower=nan, upper=nan, at=-1,
                    ranks=numpy.full(len(ranks), nan), nonfinite=bad)
    median = s[N // 2] if N % 2 else numpy.mean(s[N // 2 - 1:N // 2 + 1])
    best, at = None, -1
    with numpy.errstate(over="ignore"):
        width = s[gap:] - s[:N - gap]
    for i in range(N - gap) if N - gap <= 64 else ():   # the definition, spelled out when short
        if best is None or width[i] < best:
            best, at = width[i], i
    if N - gap > 64:
        at = int(numpy.flatnonzero(width == numpy.min(width))[0])
    return dict(median=median, lower=s[at], upper=s[at + gap], at=at,
                ranks=s[numpy.asarray(ranks, dtype=numpy.int64)], nonfinite=0)


def words(a):
    """float64 -> its uint64 words (so that -0.0 != +0.0 and NaN == NaN in a comparison)."""
    return numpy.ascontiguousarray(a, dtype=numpy.float64).view(numpy.uint64)
