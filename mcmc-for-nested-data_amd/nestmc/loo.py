"""PSIS-LOO: Pareto-smoothed importance-sampling leave-one-out cross-validation with its
pointwise terms and the Pareto k diagnostic (Vehtari, Gelman, Gabry 2017; Vehtari, Simpson,
Gelman, Yao, Gabry 2024; the generalised Pareto fit of Zhang and Stephens 2009 as loo /
arviz ``gpdfitnew`` write it).

Samples are s = (chain, recorded row), S = n_rows * n_valid of them; ll_s is observation i's
log-likelihood at sample s (the values of Engine.obs_ll_rows).  For observation i:

Shift and cutoff
  r_s = -ll_s - max_s(-ll_s) = min_s(ll_s) - ll_s, so r <= 0; ONE float64 subtraction -- the
        tail's membership is discrete, so r and cut are float64 numbers by definition, in
        every evaluation of these formulas
  M   = ceil(min(S / 5, 3 sqrt(S)))
  cut = max(the (M + 1)-th largest r, log(DBL_MIN))
  the tail is the values with r > cut, strictly, in ascending order, n2 <= M of them

Short tail
  n2 <= 4: k = +inf and the weights stay r

Fit (Zhang-Stephens)
  x_j = exp(tail_j) - exp(cut)
  m   = 30 + floor(sqrt(n2))
  b_j = (1 - sqrt(m / (j - 0.5))) / (3 x[floor(n2 / 4 + 0.5) - 1]) + 1 / x[n2 - 1], j = 1..m
  k_j = mean_t log1p(-b_j x_t)
  L_j = n2 (log(-b_j / k_j) - k_j - 1)
  w_j = 1 / sum_i exp(L_i - L_j); the weights below 10 DBL_EPSILON dropped, the rest
        renormalised
  b   = sum_j b_j w_j,  k' = mean_t log1p(-b x_t),  sigma = -k' / b
  k   = (n2 k' + 5) / (n2 + 10)

Smoothed tail
  p_j  = (j + 0.5) / n2, j = 0..n2 - 1
  q_j  = sigma expm1(-k log1p(-p_j)) / k     (|k| < DBL_EPSILON: q_j = -sigma log1p(-p_j))
  lw_j = min(log(q_j + exp(cut)), 0): these replace the tail's weights in order

Pointwise terms
  elpd_loo_i = log sum_s exp(lw_s + ll_s) - log sum_s exp(lw_s)     (both sums max-shifted)
  lppd_i     = log((1 / S) sum_s exp(ll_s))                          (as in nestmc.waic)
  p_loo_i    = lppd_i - elpd_loo_i

Totals
  elpd, p_loo, looic = -2 elpd;  se = sqrt(n_obs var_i(elpd_loo_i, ddof = 1))
  elpd_g, p_loo_g: the sums over the observations of group g
  k_threshold = min(1 - 1 / log10(S), 0.7),  n_bad = #{k_i > k_threshold}

Every quantity depends only on the multiset of the observation's values.

Two routes lead here.  The device route (Engine.loo, samplePosterior(computeLoo=True)) never
brings the [S, n_obs] matrix to the host: the GPU writes the log-likelihoods of a batch of
observations in the sample store's layout, sorts those columns and runs one workgroup per
observation over its sorted column (csrc/psis.h).  The host route (``from_ll_matrix``,
``from_directory``) evaluates the same formulas with numpy.  This module is numpy only and
imports without a GPU.
"""

import os

import numpy

from . import waic as _waic

LOG_TINY = float(numpy.log(numpy.finfo(numpy.float64).tiny))
EPS = float(numpy.finfo(numpy.float64).eps)


def tail_length(S):
    """M = ceil(min(S / 5, 3 sqrt(S)))."""
    return int(numpy.ceil(min(S / 5.0, 3.0 * numpy.sqrt(float(S)))))


def k_threshold(S):
    return float(min(1.0 - 1.0 / numpy.log10(S), 0.7))


def gpdfit(x):
    """(k, sigma) of the Zhang-Stephens fit above to the ascending positive values x."""
    x = numpy.asarray(x, dtype=numpy.float64)
    n2 = len(x)
    m = 30 + int(numpy.sqrt(n2))
    with numpy.errstate(all="ignore"):
        b = 1.0 - numpy.sqrt(m / (numpy.arange(1, m + 1, dtype=numpy.float64) - 0.5))
        b = b / (3.0 * x[int(n2 / 4.0 + 0.5) - 1])
        b = b + 1.0 / x[-1]
        kj = numpy.mean(numpy.log1p(-b[:, None] * x), axis=1)
        L = n2 * (numpy.log(-b / kj) - kj - 1.0)
        w = 1.0 / numpy.sum(numpy.exp(L - L[:, None]), axis=1)
        keep = w >= 10.0 * EPS
        w = w[keep] / numpy.sum(w[keep])
        bb = numpy.sum(b[keep] * w)
        k1 = numpy.mean(numpy.log1p(-bb * x))
        sigma = -k1 / bb
        k = (n2 * k1 + 5.0) / (n2 + 10.0)
    return float(k), float(sigma)


def psis_column(ll):
    """One observation: dict(elpd, lppd, k, n_tail, cut, lw_tail) of its S values ll (any
    order); lw_tail: the smoothed log-weights of the tail, ascending (empty for a short tail)."""
    a = numpy.sort(numpy.asarray(ll, dtype=numpy.float64))
    S = len(a)
    M = tail_length(S)
    with numpy.errstate(all="ignore"):
        r = a[0] - a                          # descending from 0
        cut = max(float(r[M]), LOG_TINY)
        n2 = int(numpy.sum(r[:M] > cut))
        lw = r.copy()
        k = numpy.inf
        lw_tail = numpy.empty(0)
        if n2 > 4:
            ecut = numpy.exp(cut)
            x = numpy.exp(r[:n2][::-1]) - ecut
            k, sigma = gpdfit(x)
            l1 = numpy.log1p(-(numpy.arange(n2) + 0.5) / n2)
            q = -sigma * l1 if abs(k) < EPS else sigma * numpy.expm1(-k * l1) / k
            lw_tail = numpy.minimum(numpy.log(q + ecut), 0.0)
            lw[:n2] = lw_tail[::-1]
        t = lw + a
        mn, md = numpy.max(t), numpy.max(lw)
        elpd = (mn + numpy.log(numpy.sum(numpy.exp(t - mn)))) \
            - (md + numpy.log(numpy.sum(numpy.exp(lw - md))))
        lppd = a[-1] + numpy.log(numpy.sum(numpy.exp(a - a[-1])) / S)
    return dict(elpd=float(elpd), lppd=float(lppd), k=float(k), n_tail=n2, cut=cut,
                lw_tail=lw_tail)


class LooResult:
    """elpd_i (elpd_loo_i), lppd_i, p_loo_i, pareto_k [n_obs], n_tail [n_obs] (int);
    elpd, p_loo, looic, se, se_looic, lppd (scalars); n_samples, n_obs; k_threshold, n_bad;
    elpd_g, p_loo_g [G]; offsets [G + 1] (the groups' CSR offsets)."""

    def __init__(self, elpd_i, lppd_i, pareto_k, n_tail, n_samples, offsets):
        off = numpy.asarray(offsets, dtype=numpy.int64)
        self.elpd_i = numpy.asarray(elpd_i, dtype=numpy.float64)
        self.lppd_i = numpy.asarray(lppd_i, dtype=numpy.float64)
        self.pareto_k = numpy.asarray(pareto_k, dtype=numpy.float64)
        self.n_tail = numpy.asarray(n_tail, dtype=numpy.int64)
        if off.ndim != 1 or len(off) < 1 or off[-1] != len(self.elpd_i):
            raise ValueError("offsets end at %s, there are %d observations"
                             % (off[-1:], len(self.elpd_i)))
        self.p_loo_i = self.lppd_i - self.elpd_i
        self.n_samples = int(n_samples)
        self.n_obs = len(self.elpd_i)
        self.offsets = off
        self.lppd = float(numpy.sum(self.lppd_i))
        self.elpd = float(numpy.sum(self.elpd_i))
        self.p_loo = float(numpy.sum(self.p_loo_i))
        self.looic = -2.0 * self.elpd
        self.se = float(numpy.sqrt(self.n_obs * numpy.var(self.elpd_i, ddof=1))) \
            if self.n_obs > 1 else float("nan")
        self.se_looic = 2.0 * self.se
        self.elpd_g = numpy.array([numpy.sum(self.elpd_i[a:b]) for a, b in zip(off[:-1], off[1:])])
        self.p_loo_g = numpy.array([numpy.sum(self.p_loo_i[a:b])
                                    for a, b in zip(off[:-1], off[1:])])
        self.k_threshold = k_threshold(self.n_samples)
        with numpy.errstate(invalid="ignore"):
            self.n_bad = int(numpy.sum(self.pareto_k > self.k_threshold))

    def __repr__(self):
        return ("LooResult(looic=%.6f, se_looic=%.6f, elpd=%.6f, p_loo=%.6f, n_bad=%d, "
                "k_threshold=%.4f, n_samples=%d, n_obs=%d)"
                % (self.looic, self.se_looic, self.elpd, self.p_loo, self.n_bad,
                   self.k_threshold, self.n_samples, self.n_obs))

    def warning(self):
        """One line when some Pareto k exceed the threshold, else None."""
        if self.n_bad == 0:
            return None
        return ("PSIS-LOO: %d of %d observations have Pareto k > %.3f (largest %.3f): their "
                "elpd_loo terms are unreliable" % (self.n_bad, self.n_obs, self.k_threshold,
                                                   float(numpy.nanmax(self.pareto_k))))


def from_ll_matrix(ll, offsets):
    """The host route: the formulas above over the matrix ll[S, n_obs], column by column."""
    ll = numpy.asarray(ll, dtype=numpy.float64)
    if ll.ndim != 2:
        raise ValueError("ll must be [S, n_obs]")
    S = ll.shape[0]
    if S < 2:
        raise ValueError("PSIS-LOO needs at least two samples (got %d)" % S)
    if not numpy.all(numpy.isfinite(ll)):
        raise ValueError("PSIS-LOO: %d per-observation log-likelihood terms were not finite"
                         % int(numpy.sum(~numpy.isfinite(ll))))
    cols = [psis_column(ll[:, i]) for i in range(ll.shape[1])]
    return LooResult([c["elpd"] for c in cols], [c["lppd"] for c in cols],
                     [c["k"] for c in cols], [c["n_tail"] for c in cols], S, offsets)


def from_directory(outputDirectory, offsets):
    """from_ll_matrix over the logLikelihood.<chain>.csv files of a run (nestmc.waic's reader;
    the files carry six decimals, so every term is known to 5e-7 only)."""
    return from_ll_matrix(_waic.read_directory(outputDirectory), offsets)


def compare(a, b):
    """(elpd_diff, se_diff) of two results over the same observations -- two LooResults or two
    WaicResults: elpd_diff = sum_i (elpd_i^a - elpd_i^b), se_diff = sqrt(n var_i(elpd_i^a -
    elpd_i^b, ddof = 1))."""
    if type(a) is not type(b):
        raise TypeError("compare needs two results of one kind")
    if a.n_obs != b.n_obs:
        raise ValueError("the results cover %d and %d observations" % (a.n_obs, b.n_obs))
    d = a.elpd_i - b.elpd_i
    n = len(d)
    se = float(numpy.sqrt(n * numpy.var(d, ddof=1))) if n > 1 else float("nan")
    return float(numpy.sum(d)), se


HEADER = "looic,se_looic,elpd,se_elpd,p_loo,n_bad,k_threshold,n_samples,n_obs"
HEADER_POINTWISE = "obs,group,lppd,p_loo,elpd,pareto_k,n_tail"


def write_csvs(result, outputDirectory):
    """outputDirectory/loo.csv (header and one line) and loo_pointwise.csv (header and one
    line per observation); floating-point values as %.17g, which reads back exactly."""
    r = result
    g = "%.17g"
    with open(os.path.join(outputDirectory, "loo.csv"), "w") as f:
        f.write(HEADER + "\n")
        f.write(",".join([g % r.looic, g % r.se_looic, g % r.elpd, g % r.se, g % r.p_loo,
                          "%d" % r.n_bad, g % r.k_threshold, "%d" % r.n_samples,
                          "%d" % r.n_obs]) + "\n")
    group = numpy.repeat(numpy.arange(len(r.offsets) - 1), numpy.diff(r.offsets))
    with open(os.path.join(outputDirectory, "loo_pointwise.csv"), "w") as f:
        f.write(HEADER_POINTWISE + "\n")
        f.write("".join("%d,%d,%.17g,%.17g,%.17g,%.17g,%d\n"
                        % (i, group[i], r.lppd_i[i], r.p_loo_i[i], r.elpd_i[i], r.pareto_k[i],
                           r.n_tail[i]) for i in range(r.n_obs)))
