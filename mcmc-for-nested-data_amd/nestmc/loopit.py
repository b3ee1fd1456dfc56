"""LOO-PIT and the leave-one-out predictive moments: every sample's replicate of observation
i re-weighted by the PSIS weight of leaving i out (Gelman et al., BDA3 section 7; arviz
``loo_pit``; loo ``E_loo``).  The in-sample PIT of nestmc.ppc uses each observation twice, to
fit and to check, and is pulled towards 0.5; this one is not.

The definitions extend nestmc/loo.py's docstring.  Observation i has the samples s = (recorded
row, chain), S = n_rows * n_valid of them.  From loo.py, unchanged: ll_s, r_s = min(ll) - ll_s
(one float64 subtraction), ``cut``, n2 and the smoothed tail lw_tail_j, j = 0..n2 - 1 ascending,
present only when n2 > 4.

Log-weight of a sample
  lw_s = r_s when r_s <= cut, or when the tail is short (n2 <= 4).  Otherwise the sample is in
  the tail: let the samples whose ll EQUALS ll_s occupy the ascending tail places [a, b).
  With b - a = 1, the usual case, lw_s = lw_tail_a.

Shift
  D = max(r of the first body position, max_j lw_tail_j) -- nmc_k_psis' shift of the weights'
  sum; D = 0 with a short tail.

Weight
  W_s = exp(lw_s - D); for a tie in the tail W_s = (1 / (b - a)) sum_{j in [a, b)}
  exp(lw_tail_j - D): tied samples share the mean weight of their places, so everything below
  depends on the multiset of (ll_s, y_rep_s) pairs alone.   Z = sum_s W_s.  Ties are common: a
  chain that rejects between two recorded rows repeats its log-likelihoods.  Swapping the
  replicates of tied tail samples changes no bit of any result: both routes put a tie
  group's replicates in ascending order before they sum.

Replicate
  y_rep_s of response field j is computePredictiveChecks' replicate: the same Philox block
  (NMC_PURPOSE_PREDICT, row, observation, field, global chain, seed); it equals
  Engine.predictive_draws bit for bit.

Results, per observation
  ess_i = Z^2 / sum_s W_s^2
and per observation and response field, y the observed value
  wlt          = sum_s W_s [y_rep_s < y] / Z
  weq          = sum_s W_s [y_rep_s == y] / Z
  loo_pit      = wlt + weq / 2                      (nestmc.ppc's convention for discrete responses)
  loo_mean     = sum_s W_s y_rep_s / Z
  loo_var      = sum_s W_s (y_rep_s - loo_mean)^2 / Z,   loo_sd = sqrt(loo_var)
  loo_residual = (y - loo_mean) / loo_sd

Non-finite inputs
  A replicate that is not finite is counted and its observation and field get NaN, as in
  nestmc.ppc.  A log-likelihood that is not finite behaves as in PSIS-LOO: the device gives the
  observation NaN and its count, the host route and Engine.loo_pit raise.

Summaries
  per group the mean PIT and the number of its (observation, field) pairs with PIT < 0.025 or
  > 0.975 (nestmc.ppc's limits); overall the fraction outside those limits (5 % for a
  calibrated continuous model) and the Kolmogorov distance sup |F_n(u) - u| of the PITs from
  U(0, 1).  For a discrete response the mid-PIT is not uniform even for the true model: there
  the distance is descriptive only.

Two routes lead here.  The device route (Engine.loo_pit, samplePosterior(computeLooPit=True))
writes the batch's log-likelihoods and one response field's replicates side by side in the
store's layout, sorts the log-likelihood columns once -- the sort PSIS-LOO itself needs, whose
results come out of the same pass -- and runs one workgroup per observation over the two
unsorted buffers (csrc/psis.h nmc_k_psis_expect): neither [S, n_obs] matrix ever reaches the
host.  The host route (``from_matrices``) evaluates the same formulas with numpy.  This module
is numpy only and imports without a GPU.
"""

import os

import numpy

from . import loo as _loo

PIT_LO, PIT_HI = 0.025, 0.975


def _weights(ll):
    """(W_s in sample order, the psis_column dict, the ties) of one column ll[S]: the tail's
    samples take the smoothed weight of their place, ties the mean weight of their places;
    the ties: the sample indices, ascending, of every group of several tail samples with one
    log-likelihood."""
    ll = numpy.asarray(ll, dtype=numpy.float64)
    col = _loo.psis_column(ll)
    with numpy.errstate(all="ignore"):
        r = numpy.min(ll) - ll
        lw_tail = col["lw_tail"]
        n2 = len(lw_tail)
        if n2 == 0:
            return numpy.exp(r), col, []                     # D = r of position 0 = 0
        order = numpy.argsort(ll, kind="stable")[:n2]        # the head, ascending in ll
        body = numpy.sort(ll)[n2]
        D = max(float(numpy.min(ll) - body), float(numpy.max(lw_tail)))
        w = numpy.exp(r - D)
        e = numpy.exp(lw_tail - D)[::-1]                     # by head position
        v = ll[order]
        start = numpy.flatnonzero(numpy.concatenate([[True], v[1:] != v[:-1]]))
        stop = numpy.concatenate([start[1:], [n2]])
        ties = []
        for a, b in zip(start, stop):
            # (ascending tail places, as the device adds them)
            w[order[a:b]] = numpy.sum(e[a:b][::-1]) / (b - a) if b - a > 1 else e[a]
            if b - a > 1:
                ties.append(numpy.sort(order[a:b]))
    return w, col, ties


def psis_weights(ll):
    """The normalised weights W_s / Z of one column ll[S], in sample order."""
    w = _weights(ll)[0]
    return w / numpy.sum(w)


def expect_column(ll, yrep, y):
    """One observation and field: dict(ess, wlt, weq, mean, var, nonfinite_draws) and the
    psis_column dict of ll[S], from the replicates yrep[S] and the observed value y.  Tied
    tail samples share one weight, so which of them carries which replicate must not matter,
    not in the last bit either: a group's replicates are put in ascending order first."""
    w, col, ties = _weights(ll)
    yrep = numpy.array(yrep, dtype=numpy.float64)
    for idx in ties:
        yrep[idx] = numpy.sort(yrep[idx])
    with numpy.errstate(all="ignore"):
        Z = numpy.sum(w)
        bad = int(numpy.sum(~numpy.isfinite(yrep)))
        out = dict(ess=float(Z * Z / numpy.sum(w * w)), nonfinite_draws=bad)
        if bad:
            out.update(wlt=numpy.nan, weq=numpy.nan, mean=numpy.nan, var=numpy.nan)
        else:
            mean = numpy.sum(w * yrep) / Z
            out.update(wlt=float(numpy.sum(w[yrep < y]) / Z), weq=float(numpy.sum(w[yrep == y]) / Z),
                       mean=float(mean), var=float(numpy.sum(w * (yrep - mean) ** 2) / Z))
    return out, col


def kolmogorov_distance(pit):
    """sup_u |F_n(u) - u| of the finite values of pit against U(0, 1) (NaN if none)."""
    u = numpy.sort(numpy.asarray(pit, dtype=numpy.float64).ravel())
    u = u[numpy.isfinite(u)]
    n = len(u)
    if n == 0:
        return float("nan")
    i = numpy.arange(1, n + 1, dtype=numpy.float64)
    return float(max(numpy.max(i / n - u), numpy.max(u - (i - 1) / n)))


class LooPitResult:
    """Per observation and field [n_obs, NRESP]: y, wlt, weq, loo_pit, loo_mean, loo_var,
    loo_sd, loo_residual, nonfinite_draws (int); per observation [n_obs]: ess, pareto_k; per
    group [G]: pit_mean_g, n_outside_g, n_g (its finite PITs); overall: n_outside,
    frac_outside, ks (kolmogorov_distance; descriptive only for a discrete response), n_pit;
    n_samples, n_obs, offsets; loo: the LooResult of the same pass."""

    def __init__(self, loo, ess, wlt, weq, mean, var, y, nonfinite_draws=None):
        self.loo = loo
        self.offsets = loo.offsets
        self.n_obs, self.n_samples = loo.n_obs, loo.n_samples
        self.pareto_k = loo.pareto_k
        f2 = lambda a: numpy.asarray(a, dtype=numpy.float64).reshape(self.n_obs, -1)  # noqa: E731
        self.ess = numpy.asarray(ess, dtype=numpy.float64).reshape(self.n_obs)
        self.wlt, self.weq, self.loo_mean, self.loo_var, self.y = (f2(a) for a in
                                                                   (wlt, weq, mean, var, y))
        if not (self.wlt.shape == self.weq.shape == self.loo_mean.shape == self.loo_var.shape
                == self.y.shape):
            raise ValueError("wlt, weq, mean, var and y must all be [n_obs, NRESP]")
        self.nonfinite_draws = numpy.zeros(self.wlt.shape, dtype=numpy.int64) \
            if nonfinite_draws is None else \
            numpy.asarray(nonfinite_draws, dtype=numpy.int64).reshape(self.wlt.shape)
        with numpy.errstate(all="ignore"):
            self.loo_pit = self.wlt + self.weq / 2.0
            self.loo_sd = numpy.sqrt(self.loo_var)
            self.loo_residual = (self.y - self.loo_mean) / self.loo_sd
            out = (self.loo_pit < PIT_LO) | (self.loo_pit > PIT_HI)
        fin = numpy.isfinite(self.loo_pit)
        off = self.offsets
        seg = list(zip(off[:-1], off[1:]))
        self.n_g = numpy.array([int(numpy.sum(fin[a:b])) for a, b in seg], dtype=numpy.int64)
        self.n_outside_g = numpy.array([int(numpy.sum(out[a:b])) for a, b in seg],
                                       dtype=numpy.int64)
        self.pit_mean_g = numpy.array([numpy.mean(self.loo_pit[a:b][fin[a:b]])
                                       if numpy.any(fin[a:b]) else numpy.nan for a, b in seg])
        self.n_pit = int(numpy.sum(fin))
        self.n_outside = int(numpy.sum(out))
        self.frac_outside = self.n_outside / self.n_pit if self.n_pit else float("nan")
        self.ks = kolmogorov_distance(self.loo_pit)

    def summary(self):
        """One line: the PITs outside the limits against the 5 % a calibrated model gives."""
        return ("LOO-PIT: %d of %d (observation, field) pairs have PIT < %.3f or > %.3f "
                "(%.1f %%, expected 5 %%); Kolmogorov distance from U(0, 1) %.4f; smallest "
                "importance ESS %.1f of %d samples"
                % (self.n_outside, self.n_pit, PIT_LO, PIT_HI, 100.0 * self.frac_outside,
                   self.ks, float(numpy.nanmin(self.ess)) if self.n_obs else float("nan"),
                   self.n_samples))

    def __repr__(self):
        return ("LooPitResult(n_samples=%d, n_obs=%d, n_outside=%d, frac_outside=%.4f, ks=%.4f)"
                % (self.n_samples, self.n_obs, self.n_outside, self.frac_outside, self.ks))


def from_matrices(ll, yrep, y, offsets):
    """The host route: the formulas above over ll[S, n_obs], the replicates yrep[S, n_obs] or
    [S, n_obs, NRESP] of the same samples and the observed y[n_obs] or [n_obs, NRESP]."""
    ll = numpy.asarray(ll, dtype=numpy.float64)
    yrep = numpy.asarray(yrep, dtype=numpy.float64)
    if ll.ndim != 2:
        raise ValueError("ll must be [S, n_obs]")
    S, n = ll.shape
    if yrep.ndim == 2:
        yrep = yrep[:, :, None]
    if yrep.ndim != 3 or yrep.shape[:2] != (S, n):
        raise ValueError("yrep must be [S, n_obs] or [S, n_obs, NRESP] like ll")
    NR = yrep.shape[2]
    y = numpy.asarray(y, dtype=numpy.float64)
    if y.size != n * NR:
        raise ValueError("y must be [n_obs] or [n_obs, NRESP]")
    y = y.reshape(n, NR)
    if S < 2:
        raise ValueError("LOO-PIT needs at least two samples (got %d)" % S)
    if not numpy.all(numpy.isfinite(ll)):
        raise ValueError("LOO-PIT: %d per-observation log-likelihood terms were not finite"
                         % int(numpy.sum(~numpy.isfinite(ll))))
    ess = numpy.empty(n)
    f = {k: numpy.empty((n, NR)) for k in ("wlt", "weq", "mean", "var")}
    bad = numpy.zeros((n, NR), dtype=numpy.int64)
    cols = []
    for i in range(n):
        for j in range(NR):
            e, col = expect_column(ll[:, i], yrep[:, i, j], y[i, j])
            for k in f:
                f[k][i, j] = e[k]
            bad[i, j] = e["nonfinite_draws"]
        ess[i] = e["ess"]
        cols.append(col)
    res = _loo.LooResult([c["elpd"] for c in cols], [c["lppd"] for c in cols],
                         [c["k"] for c in cols], [c["n_tail"] for c in cols], S, offsets)
    return LooPitResult(res, ess, f["wlt"], f["weq"], f["mean"], f["var"], y, bad)


HEADER_POINTWISE = "obs,group,field,y,loo_mean,loo_sd,loo_residual,loo_pit,wlt,weq,ess,pareto_k"
HEADER_GROUPS = "group,n_pit,pit_mean,n_outside"


def write_csvs(result, outputDirectory):
    """outputDirectory/loo_pit_pointwise.csv (one line per observation and field) and
    loo_pit_groups.csv (one line per group); floating-point values as %.17g, which reads back
    exactly."""
    r = result
    NR = r.wlt.shape[1]
    group = numpy.repeat(numpy.arange(len(r.offsets) - 1), numpy.diff(r.offsets))
    with open(os.path.join(outputDirectory, "loo_pit_pointwise.csv"), "w") as f:
        f.write(HEADER_POINTWISE + "\n")
        f.write("".join("%d,%d,%d,%.17g,%.17g,%.17g,%.17g,%.17g,%.17g,%.17g,%.17g,%.17g\n"
                        % (i, group[i], j, r.y[i, j], r.loo_mean[i, j], r.loo_sd[i, j],
                           r.loo_residual[i, j], r.loo_pit[i, j], r.wlt[i, j], r.weq[i, j],
                           r.ess[i], r.pareto_k[i])
                        for i in range(r.n_obs) for j in range(NR)))
    with open(os.path.join(outputDirectory, "loo_pit_groups.csv"), "w") as f:
        f.write(HEADER_GROUPS + "\n")
        f.write("".join("%d,%d,%.17g,%d\n" % (g, r.n_g[g], r.pit_mean_g[g], r.n_outside_g[g])
                        for g in range(len(r.n_g))))
