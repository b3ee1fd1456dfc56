"""WAIC (Watanabe-Akaike information criterion) with its pointwise terms.

Samples are s = (chain, recorded row), S of them; ll_is is observation i's log-likelihood
at sample s (StepMethod.logLikelihood, posteriorSampling.py:656-659, at the recorded values:
the rows saveLogLikelihood prints, :890-891, :907-909).

  lppd_i   = log((1/S) sum_s exp(ll_is))
  p_waic_i = sum_s (ll_is - mean_i)^2 / (S - 1)           (sample variance, ddof = 1)
  elpd_i   = lppd_i - p_waic_i
  elpd     = sum_i elpd_i,  p_waic = sum_i p_waic_i,  waic = -2 elpd
  se       = sqrt(n_obs var_i(elpd_i, ddof = 1))          (se_elpd; se_waic = 2 se)
  elpd_g, p_waic_g: the sums over the observations of group g

Two routes lead here.  The device route (Engine.waic, samplePosterior(computeWaic=True))
never forms the [S, n_obs] matrix: the GPU reduces every observation over the samples of a
chain block to the combinable state (m, s, n, mean, M2) -- m = max ll, s = sum exp(ll - m),
n = count, Welford's mean and M2 -- and ``merge`` / ``finish`` combine the blocks here.  The
host route (``from_ll_matrix``, ``from_directory``) computes the same numbers from the
matrix or from the logLikelihood.<chain>.csv files of a run.  This module is numpy only
and imports without a GPU.
"""

import glob
import os
import re

import numpy


class WaicResult:
    """lppd_i, p_waic_i, elpd_i [n_obs]; elpd, p_waic, waic, se, se_waic, lppd (scalars);
    n_samples, n_obs; elpd_g, p_waic_g [G]; offsets [G + 1] (the groups' CSR offsets)."""

    def __init__(self, lppd_i, p_waic_i, n_samples, offsets):
        off = numpy.asarray(offsets, dtype=numpy.int64)
        self.lppd_i = numpy.asarray(lppd_i, dtype=numpy.float64)
        self.p_waic_i = numpy.asarray(p_waic_i, dtype=numpy.float64)
        if off.ndim != 1 or len(off) < 1 or off[-1] != len(self.lppd_i):
            raise ValueError("offsets end at %s, there are %d observations"
                             % (off[-1:], len(self.lppd_i)))
        self.elpd_i = self.lppd_i - self.p_waic_i
        self.n_samples = int(n_samples)
        self.n_obs = len(self.lppd_i)
        self.offsets = off
        self.lppd = float(numpy.sum(self.lppd_i))
        self.elpd = float(numpy.sum(self.elpd_i))
        self.p_waic = float(numpy.sum(self.p_waic_i))
        self.waic = -2.0 * self.elpd
        self.se = float(numpy.sqrt(self.n_obs * numpy.var(self.elpd_i, ddof=1))) \
            if self.n_obs > 1 else float("nan")
        self.se_waic = 2.0 * self.se
        self.elpd_g = numpy.array([numpy.sum(self.elpd_i[a:b]) for a, b in zip(off[:-1], off[1:])])
        self.p_waic_g = numpy.array([numpy.sum(self.p_waic_i[a:b])
                                     for a, b in zip(off[:-1], off[1:])])

    def __repr__(self):
        return ("WaicResult(waic=%.6f, se_waic=%.6f, elpd=%.6f, p_waic=%.6f, n_samples=%d, "
                "n_obs=%d)" % (self.waic, self.se_waic, self.elpd, self.p_waic, self.n_samples,
                               self.n_obs))


def identity(n_obs):
    """The merge's neutral element: (-inf, 0, 0, 0, 0) for every observation."""
    p = numpy.zeros((5, int(n_obs)))
    p[0] = -numpy.inf
    return p


def _merge2(A, B):
    mA, sA, nA, meanA, M2A = A
    mB, sB, nB, meanB, M2B = B
    with numpy.errstate(invalid="ignore", divide="ignore", over="ignore"):
        m = numpy.maximum(mA, mB)
        s = numpy.where(nA > 0, sA * numpy.exp(mA - m), 0.0) \
            + numpy.where(nB > 0, sB * numpy.exp(mB - m), 0.0)
        d = meanB - meanA
        n = nA + nB
        mean = meanA + d * nB / n
        M2 = M2A + M2B + d * d * nA * nB / n
    out = numpy.stack([m, s, n, mean, M2])
    # an empty side leaves the other exactly as it is (and two empty sides the identity)
    out = numpy.where(nB == 0, A, out)
    return numpy.where((nA == 0) & (nB != 0), B, out)


def merge(parts):
    """Merge [5, n_obs] partials IN THE GIVEN ORDER (A then B, left to right):
      m = max(mA, mB);  s = sA exp(mA - m) + sB exp(mB - m), a side with n = 0 adding 0
      d = meanB - meanA;  n = nA + nB;  mean = meanA + d nB / n
      M2 = M2A + M2B + d^2 nA nB / n                                  (Chan et al.)
    The order is part of the result's definition: the same partials merged in the same
    order give the same bits."""
    parts = [numpy.asarray(p, dtype=numpy.float64) for p in parts]
    if not parts:
        raise ValueError("nothing to merge")
    for p in parts:
        if p.ndim != 2 or p.shape != parts[0].shape or p.shape[0] != 5:
            raise ValueError("partials must all be [5, n_obs]")
    acc = parts[0].copy()
    for p in parts[1:]:
        acc = _merge2(acc, p)
    return acc


def finish(partial, offsets):
    """The WaicResult of one merged [5, n_obs] partial; raises for fewer than two samples."""
    m, s, n, _, M2 = numpy.asarray(partial, dtype=numpy.float64)
    if len(n) and not numpy.all(n == n[0]):
        raise ValueError("observations were reduced over different sample counts")
    S = float(n[0]) if len(n) else 0.0
    if S < 2:
        raise ValueError("WAIC needs at least two samples (got %g)" % S)
    with numpy.errstate(invalid="ignore", divide="ignore"):
        lppd_i = m + numpy.log(s / S)
        p_waic_i = M2 / (S - 1.0)
    return WaicResult(lppd_i, p_waic_i, S, offsets)


def from_ll_matrix(ll, offsets):
    """The same result straight from the matrix ll[S, n_obs]: the plain host route, and the
    formulas as one would write them down."""
    from scipy.special import logsumexp
    ll = numpy.asarray(ll, dtype=numpy.float64)
    if ll.ndim != 2:
        raise ValueError("ll must be [S, n_obs]")
    S = ll.shape[0]
    if S < 2:
        raise ValueError("WAIC needs at least two samples (got %d)" % S)
    lppd_i = logsumexp(ll, axis=0) - numpy.log(S)
    p_waic_i = numpy.var(ll, axis=0, ddof=1)
    return WaicResult(lppd_i, p_waic_i, S, offsets)


def read_directory(outputDirectory):
    """ll[S, n_obs] of a run's sample/logLikelihood.<chain>.csv files, chains in id order,
    each chain's recorded rows in file order."""
    files = glob.glob(os.path.join(outputDirectory, "sample", "logLikelihood.*.csv"))
    ids = {}
    for f in files:
        mt = re.match(r"logLikelihood\.(\d+)\.csv$", os.path.basename(f))
        if mt:
            ids[int(mt.group(1))] = f
    if not ids:
        raise FileNotFoundError("no sample/logLikelihood.<chain>.csv under %s" % outputDirectory)
    return numpy.concatenate([numpy.loadtxt(ids[c], delimiter=",", ndmin=2, dtype=numpy.float64)
                              for c in sorted(ids)], axis=0)


def from_directory(outputDirectory, offsets):
    """from_ll_matrix over the reference-format logLikelihood.<chain>.csv files of a run
    (this sampler's with saveLogLikelihood=True, or the reference's).  The files carry six
    decimals ("%f"), so every term is known to 5e-7 only and this route is exact to about
    1e-6 per pointwise term, not to rounding: use the device route, or from_ll_matrix on
    Engine.obs_ll_rows, when that matters."""
    return from_ll_matrix(read_directory(outputDirectory), offsets)


def merge_ranks(rank_parts):
    """process_per_device: the ranks' merged [5, n_obs] partials, merged in rank order."""
    return merge(rank_parts)


HEADER = "waic,se_waic,elpd,se_elpd,p_waic,n_samples,n_obs"
HEADER_POINTWISE = "obs,group,lppd,p_waic,elpd"


def write_csvs(result, outputDirectory):
    """outputDirectory/waic.csv (header and one line) and waic_pointwise.csv (header and
    one line per observation); floating-point values as %.17g, which reads back exactly."""
    r = result
    g = "%.17g"
    with open(os.path.join(outputDirectory, "waic.csv"), "w") as f:
        f.write(HEADER + "\n")
        f.write(",".join([g % r.waic, g % r.se_waic, g % r.elpd, g % r.se, g % r.p_waic,
                          "%d" % r.n_samples, "%d" % r.n_obs]) + "\n")
    group = numpy.repeat(numpy.arange(len(r.offsets) - 1), numpy.diff(r.offsets))
    with open(os.path.join(outputDirectory, "waic_pointwise.csv"), "w") as f:
        f.write(HEADER_POINTWISE + "\n")
        f.write("".join("%d,%d,%.17g,%.17g,%.17g\n" % (i, group[i], r.lppd_i[i], r.p_waic_i[i],
                                                       r.elpd_i[i]) for i in range(r.n_obs)))
