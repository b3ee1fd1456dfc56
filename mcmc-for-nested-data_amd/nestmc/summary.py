"""Posterior median and highest-density interval of every column -- without sample files.

The two numbers of nestmc.diagnosis.Diagnostic's assessment that need a sort of a column's
N values (Diagnostic._computeMedianAndHdi, sampleDiagnosis.py:419-427; computeHpdInterval
:766-776), s the sorted column:

  median     = s[N // 2] for odd N, numpy.mean of s[N / 2 - 1] and s[N / 2] otherwise
               (what numpy.median does)
  gap        = max(1, min(N - 1, round(N * (hdi_p / 100))))          Python's round
  HDI        = (s[i], s[i + gap]) for the first i that minimises s[i + gap] - s[i]
  min, max   = s[0], s[N - 1]

Two routes lead here.  The device route (Engine.summary,
samplePosterior(computeSummary=True)) sorts the columns of the device sample store as they
lie (csrc/sortcol.h, nmc_summary) and returns the values at the four ranks above and the
interval; ``finish`` makes the result of them.  The host route (``from_sorted``) starts from
sorted columns: it finishes the merge of several engines' or ranks' columns (``merge_sorted``),
and it is how the tests restate the device's numbers.  Order statistics depend only on the
multiset of a column's values: both routes give the same bits, whatever the sharding, where
diagnoseSamples reads the values back from files of six decimals.

The order is that of the device's sort key: a double's bits as an unsigned integer, inverted
when the sign is set and with the top bit set otherwise, so
-inf < ... < -0.0 < +0.0 < ... < +inf < NaN.  A column that holds a NaN or an infinity is
counted in ``nonfinite`` and gets NaN for every statistic.

This module is numpy only and imports without a GPU.
"""

import os

import numpy

_TOP = numpy.uint64(1 << 63)


def sort_key(x):
    """float64 -> uint64 that orders like the number (csrc/sortcol.h nmc_sort_key)."""
    b = numpy.ascontiguousarray(x, dtype=numpy.float64).view(numpy.uint64)
    return numpy.where(b >> numpy.uint64(63) != 0, ~b, b | _TOP)


def sort_unkey(k):
    """The inverse of sort_key."""
    k = numpy.ascontiguousarray(k, dtype=numpy.uint64)
    return numpy.where(k >> numpy.uint64(63) != 0, k & ~_TOP, ~k).view(numpy.float64)


def gap_of(N, hdi_p=95):
    """The HDI's distance in ranks (computeHpdInterval :767-770) of N >= 2 values."""
    N = int(N)
    if N < 2:
        raise ValueError("an interval needs at least two values (got %d)" % N)
    return max(1, min(N - 1, round(N * (hdi_p / 100.))))


def stat_ranks(N):
    """The ranks ``finish`` needs: the median's two (equal for odd N), the minimum's and the
    maximum's."""
    N = int(N)
    return [(N - 1) // 2, N // 2, 0, N - 1]


class SummaryResult:
    """Per column, in the order of ``parameter``: median, hdi_lower, hdi_upper, minimum,
    maximum and nonfinite (the column's values that are NaN or infinite; its statistics are
    then NaN); n = the values per column; also hdi_p and gap."""

    def __init__(self, parameter, median, hdi_lower, hdi_upper, minimum, maximum, n, nonfinite,
                 hdi_p=95, gap=None):
        self.parameter = [str(p) for p in parameter]
        f = lambda a: numpy.asarray(a, dtype=numpy.float64)   # noqa: E731
        self.median, self.hdi_lower, self.hdi_upper = f(median), f(hdi_lower), f(hdi_upper)
        self.minimum, self.maximum = f(minimum), f(maximum)
        self.n = int(n)
        self.nonfinite = numpy.asarray(nonfinite, dtype=numpy.int64)
        self.hdi_p = hdi_p
        self.gap = gap_of(self.n, hdi_p) if gap is None else int(gap)

    def __repr__(self):
        return ("SummaryResult(%d columns of n=%d values, %g %% HDI: %d with values that are "
                "not finite)" % (len(self.parameter), self.n, self.hdi_p,
                                 int(numpy.sum(self.nonfinite != 0))))


def _names(names, K):
    names = ["col%d" % k for k in range(K)] if names is None else list(names)
    if len(names) != K:
        raise ValueError("%d names for %d columns" % (len(names), K))
    return names


def finish(at_ranks, hdi, nonfinite, N, names, hdi_p=95):
    """The SummaryResult of the device's numbers: at_ranks [cols, >= 4], the values at
    stat_ranks(N) in its first four places; hdi [cols, 2]; nonfinite [cols]."""
    N = int(N)
    at = numpy.asarray(at_ranks, dtype=numpy.float64)
    hdi = numpy.asarray(hdi, dtype=numpy.float64)
    bad = numpy.asarray(nonfinite, dtype=numpy.int64)
    if at.ndim != 2 or at.shape[1] < 4:
        raise ValueError("at_ranks must be [cols, >= 4]: the values at stat_ranks(N)")
    K = at.shape[0]
    if hdi.shape != (K, 2) or bad.shape != (K,):
        raise ValueError("hdi must be [cols, 2] and nonfinite [cols]")
    with numpy.errstate(invalid="ignore", over="ignore"):
        median = at[:, 1].copy() if N % 2 else numpy.mean(at[:, 0:2], axis=1)
    return SummaryResult(_names(names, K), median, hdi[:, 0], hdi[:, 1], at[:, 2], at[:, 3], N,
                         bad, hdi_p, gap_of(N, hdi_p))


def hdi_of_sorted(s, gap):
    """(lower, upper, i) of one sorted column: the first i that minimises s[i + gap] - s[i]."""
    n = len(s)
    with numpy.errstate(invalid="ignore", over="ignore"):
        width = s[gap:n] - s[0:n - gap]
        i = int(numpy.argmax(width == width.min()))
    return s[i], s[i + gap], i


def from_sorted(sorted_columns, names=None, hdi_p=95):
    """The host route: sorted_columns [cols][N], every column in the key's order."""
    s = numpy.asarray(sorted_columns, dtype=numpy.float64)
    if s.ndim != 2:
        raise ValueError("sorted_columns must be [cols][N]")
    K, N = s.shape
    gap = gap_of(N, hdi_p)
    bad = numpy.sum(~numpy.isfinite(s), axis=1).astype(numpy.int64)
    at = numpy.full((K, 4), numpy.nan)
    hdi = numpy.full((K, 2), numpy.nan)
    for k in range(K):
        if bad[k]:
            continue
        at[k] = s[k, stat_ranks(N)]
        hdi[k, 0], hdi[k, 1], _ = hdi_of_sorted(s[k], gap)
    return finish(at, hdi, bad, N, names, hdi_p)


def merge_sorted(parts):
    """Several shards' columns [cols][N_e] (sorted or not) -> [cols][sum N_e] in the key's
    order: the sort of the union, whatever the order of the parts."""
    parts = [numpy.asarray(p, dtype=numpy.float64) for p in parts]
    if not parts:
        raise ValueError("nothing to merge")
    for p in parts:
        if p.ndim != 2 or p.shape[0] != parts[0].shape[0]:
            raise ValueError("the parts must all be [cols][N_e] with the same columns")
    return sort_unkey(numpy.sort(sort_key(numpy.concatenate(parts, axis=1)), axis=1))


HEADER = "parameter,median,HDI lower,HDI upper,min,max"


def csv_text(result):
    """The text of summary.csv: the header and one line per column, sorted by parameter."""
    r = result
    order = sorted(range(len(r.parameter)), key=lambda k: r.parameter[k].encode())
    return HEADER + "\n" + "".join(
        "'%s',%.6f,%.6f,%.6f,%.6f,%.6f\n" % (r.parameter[k], r.median[k], r.hdi_lower[k],
                                             r.hdi_upper[k], r.minimum[k], r.maximum[k])
        for k in order)


def write_csv(result, directory):
    """directory/summary.csv (csv_text)."""
    with open(os.path.join(directory, "summary.csv"), "w") as f:
        f.write(csv_text(result))


def assessment(conv_result, summary_result):
    """The table of nestmc.diagnosis.Diagnostic.assessment from the store: a structured array
    of nestmc.diagnosis.ASSESS_DTYPE (parameter, rhat, converged, effective n, enough n,
    median, HDI lower, HDI upper), sorted by parameter.  conv_result: a
    nestmc.convergence.ConvergenceResult of the same columns."""
    from .diagnosis import ASSESS_DTYPE
    c, s = conv_result, summary_result
    if list(c.parameter) != list(s.parameter):
        raise ValueError("the two results are not of the same columns")
    rows = [(p.encode(), c.rhat[k], bool(c.converged[k]), c.effective_n[k], bool(c.enough_n[k]),
             s.median[k], s.hdi_lower[k], s.hdi_upper[k]) for k, p in enumerate(s.parameter)]
    return numpy.sort(numpy.array(rows, dtype=ASSESS_DTYPE), order="parameter")
