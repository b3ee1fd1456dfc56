"""Rank-normalised split-R-hat, folded R-hat, bulk- and tail-ESS without sample files.

The convergence check of Vehtari, Gelman, Simpson, Carpenter and Buerkner (2021, "Rank-
normalization, folding, and localization: an improved R-hat for assessing convergence of
MCMC", Bayesian Analysis 16), as Stan, ArviZ and ``posterior`` report it.  nestmc.convergence
keeps the reference's 1992 formulas bit for bit; they cannot see chains that agree in location
but not in scale, are undefined without a variance, and their effective n starts its sum at
lag 0 (independent draws report N / 3).  This module carries the textbook estimator beside it.

Definitions.  The window is 2n rows over the real chains [0, n_valid), the same split and
half-chain order as nestmc.convergence.  A column has N = 2n * n_valid values x_i; s is the
sorted column.

  Ties      are numeric ties: -0.0 and +0.0 tie although their sort keys differ.
            lo_i = #{x < x_i}, hi_i = #{x <= x_i}; the average rank r_i = (lo_i + hi_i + 1) / 2
            is exact in float64.
  Normal score  z_i = ndtri(p_i), p_i = (r_i - 0.375) / (N + 0.25): one float64 division of two
            exact numbers, the same bits on the host and on the device.
  Fold      med = (s[N/2 - 1] + s[N/2]) / 2.0 (N is even: one addition and one division,
            numpy.median's bits); zeta_i = |x_i - med| (one subtraction); zf_i is the normal
            score of zeta_i's average rank among the zeta.  A zeta that overflows to +inf is a
            legitimate largest value, tied with its like, not a "nonfinite" input.
  Tail indicators  the order statistics are chosen by integers: k05 = (N - 1) // 20,
            k95 = 19 (N - 1) // 20; I05_i = 1.0 if lo_i <= k05 else 0.0, which is
            x_i <= s[k05] (numpy.quantile(method="lower")); I95_i the same with k95.
  Partials  each of the four derived columns (z, zf, I05, I95) gets exactly nmc_k_conv's
            partial sums (mean, m2, vg) with its orders and its tree (csrc/conv.h), and
            nestmc.convergence.finish gives rhat and the cutoff lag T of each unchanged.
            rhat_bulk = rhat(z), rhat_folded = rhat(zf), rhat = the larger of the two.
  ESS       tau = 1 + 2 sum_{t = 1..T} rho_t with nestmc.convergence._assess's rho_t =
            1 - V_t / (2 vhat) and its T: the sum starts at lag 1.
            ess = N / max(tau, 1 / log10 N); ess_bulk = ess(z),
            ess_tail = min(ess(I05), ess(I95)).
  Flags     converged = rhat < RHAT_THRESHOLD (1.01),
            enough = min(ess_bulk, ess_tail) > ESS_THRESHOLD (400).
  Degenerate columns  a column with a NaN or an infinity among the x is counted in
            ``nonfinite`` and gets NaN everywhere (as nestmc.summary does).  A constant column
            has p = 1/2 exactly, z = 0, W = 0: NaN R-hat and NaN ESS.

This is the published recipe except for the autocorrelation estimate: rho_t is this project's
variogram estimate with this project's cutoff T (the first even lag whose next two rho sum
below zero), not an FFT autocovariance truncated by Geyer's initial monotone sequence.

Two routes lead here.  The device route (Engine.rank_diagnostics,
samplePosterior(computeRankDiagnostics=True)) sorts the store's columns, turns every value into
its derived values (csrc/rankz.h) and reduces them with nmc_k_conv (nmc_rank_partials);
``finish`` applies the formulas.  The host route (``from_rows``) uses numpy.sort and
searchsorted, scipy.special.ndtri and nestmc.convergence.from_halfchains with variogram_host.

numpy and scipy only; imports without a GPU.
"""

import os

import numpy

from . import convergence as _conv

RHAT_THRESHOLD = 1.01
ESS_THRESHOLD = 400.0
QUANTITIES = ("z", "zf", "I05", "I95")


class RankDiagnosticsResult:
    """Per column, in the order of ``parameter``: rhat (the larger of rhat_bulk and
    rhat_folded), rhat_bulk, rhat_folded, converged, ess_bulk, ess_tail, enough, nonfinite;
    also ``parts`` (the ConvergenceResult of each derived column, by name in QUANTITIES),
    ``tau`` [4, cols], N (values per column), n (rows per half-chain) and m (half-chains)."""

    def __init__(self, parameter, parts, tau, nonfinite):
        self.parameter = [str(p) for p in parameter]
        self.parts = dict(parts)
        z = self.parts["z"]
        self.n, self.m = z.n, z.m
        self.N = self.n * self.m
        self.nonfinite = numpy.asarray(nonfinite, dtype=numpy.int64)
        bad = self.nonfinite != 0
        nan = lambda a: numpy.where(bad, numpy.nan, numpy.asarray(a, dtype=numpy.float64))  # noqa: E731
        self.tau = nan(tau)
        with numpy.errstate(invalid="ignore", divide="ignore"):
            ess = self.N / numpy.maximum(self.tau, 1.0 / numpy.log10(float(self.N)))
        self.rhat_bulk = nan(z.rhat)
        self.rhat_folded = nan(self.parts["zf"].rhat)
        # (numpy.maximum: NaN if either is)
        self.rhat = numpy.maximum(self.rhat_bulk, self.rhat_folded)
        self.ess_bulk = ess[0]
        self.ess_tail = numpy.minimum(ess[2], ess[3])
        with numpy.errstate(invalid="ignore"):
            self.converged = self.rhat < RHAT_THRESHOLD
            self.enough = numpy.minimum(self.ess_bulk, self.ess_tail) > ESS_THRESHOLD

    def __repr__(self):
        return ("RankDiagnosticsResult(%d columns, m=%d half-chains of n=%d: %d converged, "
                "%d with enough draws)" % (len(self.parameter), self.m, self.n,
                                           int(numpy.sum(self.converged)),
                                           int(numpy.sum(self.enough))))


def tau_of(V, vhat, T):
    """1 + 2 sum_{t = 1..T} rho_t per column, rho = 1 - V / (2 vhat) as in
    nestmc.convergence._assess (whose sum starts at lag 0, where rho is 1)."""
    V = numpy.asarray(V, dtype=numpy.float64)
    with numpy.errstate(invalid="ignore", divide="ignore"):
        rho = 1. - V / (2. * numpy.asarray(vhat, dtype=numpy.float64)[:, None])
    return numpy.array([1 + 2 * numpy.sum(rho[k, 1:int(T[k]) + 1]) for k in range(len(rho))])


def _vhat_of_moments(mean, m2, n, n_valid):
    """vhat as nestmc.convergence.finish computes it from mean, m2 [cols, 2, chains]."""
    mean, m2 = mean[:, :, :n_valid], m2[:, :, :n_valid]
    K, m = mean.shape[0], 2 * mean.shape[2]
    means = numpy.ascontiguousarray(numpy.transpose(mean, (0, 2, 1))).reshape(K, m)
    M2 = numpy.ascontiguousarray(numpy.transpose(m2, (0, 2, 1))).reshape(K, m)
    with numpy.errstate(invalid="ignore", divide="ignore"):
        B = n * numpy.var(means, axis=1, ddof=1)
        W = numpy.mean(M2 / (n - 1), axis=1)
        return W * (n - 1) / n + B / n


def finish(vg, mean, m2, n, names, n_valid=None, nonfinite=None):
    """The RankDiagnosticsResult of nmc_rank_partials' outputs: vg [4, CB, cols, n] (the chain
    blocks are merged in order, nestmc.convergence.merge), mean and m2 [4, cols, 2, chains],
    the quantities in the order z, zf, I05, I95; only chains [0, n_valid) are real."""
    vg = numpy.asarray(vg, dtype=numpy.float64)
    mean = numpy.asarray(mean, dtype=numpy.float64)
    m2 = numpy.asarray(m2, dtype=numpy.float64)
    if vg.ndim != 4 or vg.shape[0] != 4 or mean.ndim != 4 or mean.shape != m2.shape \
            or mean.shape[0] != 4:
        raise ValueError("vg must be [4, CB, cols, n], mean and m2 [4, cols, 2, chains]")
    K = vg.shape[2]
    nv = mean.shape[3] if n_valid is None else int(n_valid)
    names = _conv._names(names, K)
    parts, tau = {}, numpy.empty((4, K))
    for t, q in enumerate(QUANTITIES):
        r = _conv.finish(_conv.merge(list(vg[t])), mean[t], m2[t], n, names, nv)
        parts[q] = r
        tau[t] = tau_of(r.V, _vhat_of_moments(mean[t], m2[t], int(n), nv), r.T)
    bad = numpy.zeros(K, dtype=numpy.int64) if nonfinite is None else nonfinite
    return RankDiagnosticsResult(names, parts, tau, bad)


def normal_scores(x):
    """(z, twice_rank, lo) of a flat array x: the normal score of every value's average rank,
    lo + hi + 1 and lo = #{< x} (numpy.sort, searchsorted and scipy.special.ndtri)."""
    from scipy.special import ndtri
    s = numpy.sort(x)
    lo = numpy.searchsorted(s, x, side="left").astype(numpy.int64)
    hi = numpy.searchsorted(s, x, side="right").astype(numpy.int64)
    r2 = lo + hi + 1
    p = (r2.astype(numpy.float64) * 0.5 - 0.375) / (float(len(x)) + 0.25)
    return ndtri(p), r2, lo


def derive_host(rows):
    """rows [C][2n][cols] -> (derived [4][C][2n][cols] in the order z, zf, I05, I95,
    twice_rank [2][C][2n][cols] of x and of zeta, nonfinite [cols]); a column counted in
    nonfinite has NaN derived values and twice_rank 0."""
    rows = numpy.asarray(rows, dtype=numpy.float64)
    C, R, K = rows.shape
    if R % 2 or R < 4:
        raise ValueError("%d rows cannot be cut into two halves of at least two rows" % R)
    N = C * R
    k05, k95 = (N - 1) // 20, 19 * (N - 1) // 20
    derived = numpy.full((4, C, R, K), numpy.nan)
    r2s = numpy.zeros((2, C, R, K), dtype=numpy.int64)
    bad = numpy.zeros(K, dtype=numpy.int64)
    for k in range(K):
        x = rows[:, :, k].reshape(N)
        bad[k] = int(numpy.sum(~numpy.isfinite(x)))
        if bad[k]:
            continue
        z, r2, lo = normal_scores(x)
        s = numpy.sort(x)
        with numpy.errstate(over="ignore"):
            med = (s[N // 2 - 1] + s[N // 2]) / 2.0
            zeta = numpy.abs(x - med)
        zf, r2f, _ = normal_scores(zeta)
        for t, a in enumerate((z, zf, (lo <= k05).astype(numpy.float64),
                               (lo <= k95).astype(numpy.float64))):
            derived[t, :, :, k] = a.reshape(C, R)
        r2s[0, :, :, k] = r2.reshape(C, R)
        r2s[1, :, :, k] = r2f.reshape(C, R)
    return derived, r2s, bad


def from_rows(rows, names=None):
    """The host route: rows [C][2n][cols] (Engine.samples(), or "rows" of samplePosterior), all
    chains real."""
    derived, _, bad = derive_host(rows)
    K = derived.shape[3]
    names = _conv._names(names, K)
    parts, tau = {}, numpy.empty((4, K))
    for t, q in enumerate(QUANTITIES):
        x = _conv.halfchains(derived[t])
        r = _conv.from_halfchains(x, names, variogram=_conv.variogram_host)
        n = r.n
        with numpy.errstate(invalid="ignore", divide="ignore"):
            B = n * numpy.var(numpy.mean(x, axis=2), axis=1, ddof=1)
            W = numpy.mean(numpy.var(x, axis=2, ddof=1), axis=1)
            vhat = W * (n - 1) / n + B / n
        parts[q] = r
        tau[t] = tau_of(r.V, vhat, r.T)
    return RankDiagnosticsResult(names, parts, tau, bad)


HEADER = "parameter,rhat,rhat bulk,rhat folded,converged,ess bulk,ess tail,enough"


def csv_text(result):
    """The text of rank_diagnostics.csv: the header and one line per column, sorted by
    parameter, in convergence.csv's style."""
    r = result
    order = sorted(range(len(r.parameter)), key=lambda k: r.parameter[k].encode())
    return HEADER + "\n" + "".join(
        "'%s',%.3f,%.3f,%.3f,%s,%.3f,%.3f,%s\n" % (
            r.parameter[k], r.rhat[k], r.rhat_bulk[k], r.rhat_folded[k], bool(r.converged[k]),
            r.ess_bulk[k], r.ess_tail[k], bool(r.enough[k])) for k in order)


def write_csv(result, directory):
    """directory/rank_diagnostics.csv (csv_text)."""
    with open(os.path.join(directory, "rank_diagnostics.csv"), "w") as f:
        f.write(csv_text(result))
