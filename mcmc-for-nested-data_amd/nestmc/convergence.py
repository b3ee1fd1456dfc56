"""Convergence diagnostics -- R-hat and the effective sample size -- without sample files.

Every chain's recorded rows are cut into two halves of n rows (the reference's split,
sampleDiagnosis.py:136-155); the m = 2 * chains half-chains x_j of a column give, with the
formulas of nestmc.diagnosis.Diagnostic._assess (sampleDiagnosis.py:158-255),

  B     = n var_j(mean_j, ddof = 1)                 between-sequence variance
  W     = mean_j(M2_j / (n - 1))                    within-sequence variance
  vhat  = W (n - 1) / n + B / n
  rhat  = sqrt(vhat / W)                            converged: rhat < 1.1
  V_t   = sum_j sum_q (x_j[q + t] - x_j[q])^2 / (m (n - t))
  rho_t = 1 - V_t / (2 vhat)
  T     = the first even lag whose next two rho sum below zero (n - 1 if there is none)
  neff  = m n / (1 + 2 sum_{t <= T} rho_t)          enough: neff > 10 m
  mean  = mean_j(mean_j),  sd = sqrt(vhat)

Two routes lead here.  The device route (Engine.convergence,
samplePosterior(computeDiagnostics=True)) reduces the device sample store as it lies
(csrc/conv.h, nmc_conv_partials): per chain block the undivided variogram sums vg[cols, n],
per half-chain mean_j and M2_j; ``merge`` adds the blocks and ``finish`` applies the formulas.
The host route (``from_halfchains``) starts from an array x[K][m][n] with numpy's own mean and
var and nestmc.diagnosis.variogram.  Both diagnose the chains at full precision, where
diagnoseSamples reads them back from files of six decimals.

The median and the 95 % HDI of diagnoseSamples need a sort of all m n values of a column:
nestmc.summary (Engine.summary, samplePosterior(computeSummary=True)) computes them from the
store, and nestmc.summary.assessment joins the two results into Diagnostic's table.

This module is numpy only and imports without a GPU (from_halfchains calls the GPU unless it
is given ``variogram=variogram_host``).
"""

import os

import numpy


class ConvergenceResult:
    """Per column, in the order of ``parameter``: rhat, converged, effective_n, enough_n,
    mean, sd; also the variogram V [cols, n], the cutoff lag T [cols], n (rows per half-chain)
    and m (half-chains)."""

    def __init__(self, parameter, rhat, effective_n, mean, sd, V, T, n, m):
        self.parameter = [str(p) for p in parameter]
        self.rhat = numpy.asarray(rhat, dtype=numpy.float64)
        self.effective_n = numpy.asarray(effective_n, dtype=numpy.float64)
        self.mean = numpy.asarray(mean, dtype=numpy.float64)
        self.sd = numpy.asarray(sd, dtype=numpy.float64)
        self.V = numpy.asarray(V, dtype=numpy.float64)
        self.T = numpy.asarray(T, dtype=numpy.int64)
        self.n, self.m = int(n), int(m)
        self.converged = self.rhat < 1.1
        self.enough_n = self.effective_n > self.m * 10

    def __repr__(self):
        return ("ConvergenceResult(%d columns, m=%d half-chains of n=%d: %d converged, "
                "%d with enough n)" % (len(self.parameter), self.m, self.n,
                                       int(numpy.sum(self.converged)),
                                       int(numpy.sum(self.enough_n))))


def merge(parts):
    """Add variogram-sum blocks vg[cols, n] IN THE GIVEN ORDER, left to right: an engine's
    chain blocks in order, then the engines, then the ranks in rank order.  The order is part
    of the result's definition; a block of +0.0 (padding chains only) changes nothing."""
    parts = [numpy.asarray(p, dtype=numpy.float64) for p in parts]
    if not parts:
        raise ValueError("nothing to merge")
    for p in parts:
        if p.ndim != 2 or p.shape != parts[0].shape:
            raise ValueError("variogram blocks must all be [cols, n]")
    acc = parts[0].copy()
    for p in parts[1:]:
        acc = acc + p
    return acc


def merge_ranks(rank_parts):
    """process_per_device: the ranks' merged vg[cols, n], added in rank order."""
    return merge(rank_parts)


def _assess(V, vhat, n, m):
    """(T, neff) per column: the loop of Diagnostic._assess."""
    rho = 1. - V / (2. * vhat[:, None])
    K = len(vhat)
    T = numpy.empty(K, dtype=numpy.int64)
    neff = numpy.empty(K)
    for k in range(K):
        r = rho[k]
        hit = numpy.nonzero((r[1:n - 1] + r[2:n] < 0) & (numpy.arange(n - 2) % 2 == 0))[0]
        T[k] = int(hit[0]) if hit.size else n - 1
        neff[k] = (m * n) / (1 + 2 * numpy.sum(r[0:T[k] + 1]))
    return T, neff


def _names(names, K):
    names = ["col%d" % k for k in range(K)] if names is None else list(names)
    if len(names) != K:
        raise ValueError("%d names for %d columns" % (len(names), K))
    return names


def finish(vg, mean, m2, n, names, n_valid=None):
    """The ConvergenceResult of merged variogram sums vg[cols, n] and the half-chain moments
    mean, m2 [cols, 2, chains] (half 0 = a chain's first n rows), chains in global order.
    n_valid: only chains [0, n_valid) are real; the others (padding) are ignored.  The
    half-chains are ordered (chain, half), half minor; m = 2 * real chains."""
    n = int(n)
    if n < 2:
        raise ValueError("convergence needs half-chains of at least two rows (got %d)" % n)
    vg = numpy.asarray(vg, dtype=numpy.float64)
    mean = numpy.asarray(mean, dtype=numpy.float64)
    m2 = numpy.asarray(m2, dtype=numpy.float64)
    if vg.ndim != 2 or vg.shape[1] != n:
        raise ValueError("vg must be [cols, n]")
    K = vg.shape[0]
    if mean.shape != m2.shape or mean.ndim != 3 or mean.shape[:2] != (K, 2):
        raise ValueError("mean and m2 must be [cols, 2, chains]")
    if n_valid is not None:
        mean, m2 = mean[:, :, :int(n_valid)], m2[:, :, :int(n_valid)]
    if mean.shape[2] < 1:
        raise ValueError("no chains")
    m = 2 * mean.shape[2]
    means = numpy.ascontiguousarray(numpy.transpose(mean, (0, 2, 1))).reshape(K, m)
    M2 = numpy.ascontiguousarray(numpy.transpose(m2, (0, 2, 1))).reshape(K, m)
    with numpy.errstate(invalid="ignore", divide="ignore"):
        B = n * numpy.var(means, axis=1, ddof=1)
        W = numpy.mean(M2 / (n - 1), axis=1)
        vhat = W * (n - 1) / n + B / n
        rhat = numpy.sqrt(vhat / W)
        V = vg / (float(m) * (n - numpy.arange(n, dtype=numpy.float64)))[None, :]
        T, neff = _assess(V, vhat, n, m)
    return ConvergenceResult(_names(names, K), rhat, neff, numpy.mean(means, axis=1),
                             numpy.sqrt(vhat), V, T, n, m)


def variogram_host(x, lags=None):
    """nestmc.diagnosis.variogram's numbers on the host, bit for bit (its order: rows ascending
    inside a half-chain, the half-chains' sums in j order, one division): x [K][m][n] -> V [K][n],
    or V [K][len(lags)] at the given lags only."""
    x = numpy.asarray(x, dtype=numpy.float64)
    K, m, n = x.shape
    lags = range(n) if lags is None else [int(t) for t in lags]
    V = numpy.zeros((K, len(lags)))
    with numpy.errstate(invalid="ignore", over="ignore"):
        for i, t in enumerate(lags):   # lag 0 like every other: inf - inf = NaN, as on the device
            d = x[:, :, t:] - x[:, :, :n - t]
            s = numpy.cumsum(d * d, axis=2)[:, :, -1]
            V[:, i] = numpy.cumsum(s, axis=1)[:, -1] / (float(m) * float(n - t))
    return V


def from_halfchains(x, names=None, device=0, variogram=None):
    """The host route: x [K][m][n], column k's m half-chains of n rows, ordered (chain, half)
    like Diagnostic's.  The same formulas with numpy's own mean and var and
    nestmc.diagnosis.variogram (the GPU's nmc_variogram on ``device``; pass
    variogram=variogram_host to stay on the host)."""
    x = numpy.ascontiguousarray(x, dtype=numpy.float64)
    if x.ndim != 3:
        raise ValueError("x must be [K][m][n]")
    K, m, n = x.shape
    if n < 2:
        raise ValueError("convergence needs half-chains of at least two rows (got %d)" % n)
    if variogram is None:
        from . import diagnosis
        V = diagnosis.variogram(x, device)
    else:
        V = numpy.asarray(variogram(x), dtype=numpy.float64)
    with numpy.errstate(invalid="ignore", divide="ignore"):
        means = numpy.mean(x, axis=2)
        B = n * numpy.var(means, axis=1, ddof=1)
        W = numpy.mean(numpy.var(x, axis=2, ddof=1), axis=1)
        vhat = W * (n - 1) / n + B / n
        rhat = numpy.sqrt(vhat / W)
        T, neff = _assess(V, vhat, n, m)
    return ConvergenceResult(_names(names, K), rhat, neff, numpy.mean(means, axis=1),
                             numpy.sqrt(vhat), V, T, n, m)


def halfchains(rows):
    """rows [C][2n][cols] (Engine.samples(), or "rows" of samplePosterior) -> x [cols][2C][n],
    the half-chains in (chain, half) order."""
    rows = numpy.asarray(rows, dtype=numpy.float64)
    C, R, K = rows.shape
    if R % 2 or R < 4:
        raise ValueError("%d rows cannot be cut into two halves of at least two rows" % R)
    return numpy.ascontiguousarray(numpy.transpose(rows.reshape(C * 2, R // 2, K), (2, 0, 1)))


HEADER = "parameter,rhat,converged,effective n,enough n,mean,sd"


def csv_text(result):
    """The text of convergence.csv: the header and one line per column, sorted by parameter."""
    r = result
    order = sorted(range(len(r.parameter)), key=lambda k: r.parameter[k].encode())
    return HEADER + "\n" + "".join(
        "'%s',%.3f,%s,%.3f,%s,%.6f,%.6f\n" % (r.parameter[k], r.rhat[k], bool(r.converged[k]),
                                              r.effective_n[k], bool(r.enough_n[k]),
                                              r.mean[k], r.sd[k]) for k in order)


def write_csv(result, directory):
    """directory/convergence.csv (csv_text)."""
    with open(os.path.join(directory, "convergence.csv"), "w") as f:
        f.write(csv_text(result))
