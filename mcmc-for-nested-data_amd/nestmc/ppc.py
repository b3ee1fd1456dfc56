"""Posterior predictive checks (Gelman, Meng and Stern 1996; BDA3 ch. 6).

Samples are s = (chain, recorded row), S of them.  From every sample a replicated data set
y_rep is drawn from the likelihood at the sample's values, one value per observation i and
response field j (csrc/ppc.h has the stream: one Philox block per (row, observation, field,
chain)), and compared with the observed y.

  per observation and field
    mean_i, sd_i   of y_rep_i over the samples (sd with ddof = 1)
    residual_i     = (y_i - mean_i) / sd_i
    pit_i          = (lt + eq / 2) / S,  lt = #{y_rep_i < y_i}, eq = #{y_rep_i == y_i}
  per group g, field and statistic T in (mean, var, min, max) of the group's observations
    t_obs          = T(y_g)
    mean, sd       of T(y_rep_g) over the samples (sd with ddof = 1)
    p              = (gt + eq / 2) / S,  gt = #{T(y_rep_g) > T(y_g)}, eq = #{==}

T takes the group's values in observation order: Welford's mean and M2 (var = M2 / n, the
population variance), fmin and fmax; for a response with integer values (the logistic's 0 / 1,
a family's response_integer) the mean and the variance come from the exact sums of x and x^2
instead, so that a replicate that ties with the data compares equal whatever the order of its
values.  p near 0 or 1 says the model does not reproduce that
statistic of that group.

Two routes lead here.  The device route (Engine.ppc, samplePosterior(
computePredictiveChecks=True)) never forms y_rep[S, n_obs]: the GPU reduces the draws of a
chain block to integer counts and the combinable states (n, mean, M2), and ``merge`` /
``finish`` combine the blocks here.  The host route (``from_replicates``) computes the same
quantities from the replicates as one writes the formulas down.  This module is numpy only and
imports without a GPU.

A partial is a dict:
  obs_state   [3, NRESP, n_obs]  float64   n, mean, M2 of y_rep
  obs_count   [2, NRESP, n_obs]  int64     lt, eq
  group_state [G, NRESP, 4, 3]   float64   n, mean, M2 of T(y_rep)
  group_count [G, NRESP, 4, 2]   int64     gt, eq
  ty          [G, NRESP, 4]      float64   T(y) (NaN in the identity: it has seen no data)
  nonfinite   int                          draws that were not finite
"""

import os
import pickle

import numpy

STATS = ("mean", "var", "min", "max")
SLICE_WGS = 512          # csrc/ppc.h NMC_PPC_WGS


def group_slices(n_rows, n_groups, n_resp, chain_blocks):
    """csrc/ppc.h nmc_ppc_slices: the row slices of nmc_k_ppc_group (a function of the shape
    alone, so that the merge order -- and every bit of the result -- is the same everywhere)."""
    triples = int(chain_blocks) * int(n_groups) * int(n_resp)
    want = (SLICE_WGS + triples - 1) // triples if triples > 0 else 1
    most = (int(n_rows) + 3) // 4
    return max(1, min(want, most, 65535))


class PpcResult:
    """y, mean_i, sd_i, residual_i, pit_i [n_obs, NRESP]; lt, eq [n_obs, NRESP] (int64);
    t_obs, t_mean, t_sd, p [G, NRESP, 4]; gt, geq [G, NRESP, 4] (int64); n_samples, n_obs,
    offsets [G + 1]; the last axis of the group arrays follows STATS."""

    def __init__(self, y, mean_i, sd_i, lt, eq, t_obs, t_mean, t_sd, gt, geq, n_samples,
                 offsets):
        f = lambda a: numpy.asarray(a, dtype=numpy.float64)   # noqa: E731
        self.y, self.mean_i, self.sd_i = f(y), f(mean_i), f(sd_i)
        self.lt = numpy.asarray(lt, dtype=numpy.int64)
        self.eq = numpy.asarray(eq, dtype=numpy.int64)
        self.t_obs, self.t_mean, self.t_sd = f(t_obs), f(t_mean), f(t_sd)
        self.gt = numpy.asarray(gt, dtype=numpy.int64)
        self.geq = numpy.asarray(geq, dtype=numpy.int64)
        self.n_samples = int(n_samples)
        self.offsets = numpy.asarray(offsets, dtype=numpy.int64)
        self.n_obs = self.y.shape[0]
        if self.offsets[-1] != self.n_obs:
            raise ValueError("offsets end at %d, there are %d observations"
                             % (self.offsets[-1], self.n_obs))
        S = float(self.n_samples)
        with numpy.errstate(invalid="ignore", divide="ignore"):
            self.residual_i = (self.y - self.mean_i) / self.sd_i
        self.pit_i = (self.lt + self.eq / 2.0) / S
        self.p = (self.gt + self.geq / 2.0) / S

    def flagged(self, lo=0.025, hi=0.975):
        """[(group, field, statistic name, p)] with p < lo or p > hi, in group order."""
        out = []
        G, NR, _ = self.p.shape
        for g in range(G):
            for j in range(NR):
                for s, name in enumerate(STATS):
                    v = self.p[g, j, s]
                    if v < lo or v > hi:
                        out.append((g, j, name, float(v)))
        return out

    def warning(self):
        """One line naming the groups and statistics with p < 0.025 or p > 0.975, or None."""
        fl = self.flagged()
        if not fl:
            return None
        nr = self.p.shape[1]
        what = ", ".join("group %d %s%s (p = %.4g)" % (g, "" if nr == 1 else "field %d " % j, n, v)
                         for g, j, n, v in fl)
        return ("Posterior predictive checks: %d of %d (group, statistic) pairs have p < 0.025 or "
                "p > 0.975: %s." % (len(fl), self.p.size, what))

    def __repr__(self):
        return ("PpcResult(n_samples=%d, n_obs=%d, groups=%d, flagged=%d)"
                % (self.n_samples, self.n_obs, self.p.shape[0], len(self.flagged())))


def identity(n_obs, n_groups, n_resp=1):
    """The merge's neutral element: zero states and counts."""
    return dict(obs_state=numpy.zeros((3, n_resp, n_obs)),
                obs_count=numpy.zeros((2, n_resp, n_obs), dtype=numpy.int64),
                group_state=numpy.zeros((n_groups, n_resp, 4, 3)),
                group_count=numpy.zeros((n_groups, n_resp, 4, 2), dtype=numpy.int64),
                ty=numpy.full((n_groups, n_resp, 4), numpy.nan), nonfinite=0)


def _chan(nA, meanA, M2A, nB, meanB, M2B):
    """Chan's update, A then B; an empty side leaves the other exactly as it is."""
    with numpy.errstate(invalid="ignore", divide="ignore", over="ignore"):
        d = meanB - meanA
        n = nA + nB
        mean = meanA + d * nB / n
        M2 = M2A + M2B + d * d * nA * nB / n
    eA, eB = nA == 0, nB == 0
    n = numpy.where(eB, nA, numpy.where(eA, nB, n))
    mean = numpy.where(eB, meanA, numpy.where(eA, meanB, mean))
    M2 = numpy.where(eB, M2A, numpy.where(eA, M2B, M2))
    return n, mean, M2


def _same_ty(a, b):
    na, nb = numpy.isnan(a), numpy.isnan(b)
    return numpy.array_equal(na, nb) and numpy.array_equal(a[~na], b[~nb])


def merge(parts):
    """Merge partials IN THE GIVEN ORDER (A then B, left to right): counts add (int64), the
    states merge by Chan's update
      d = meanB - meanA;  n = nA + nB;  mean = meanA + d nB / n;  M2 = M2A + M2B + d^2 nA nB / n
    and T(y) must agree between the parts that have seen data.  The order is part of the
    result's definition: the same partials in the same order give the same bits."""
    parts = list(parts)
    if not parts:
        raise ValueError("nothing to merge")
    acc = {k: (numpy.array(v, copy=True) if isinstance(v, numpy.ndarray) else v)
           for k, v in parts[0].items()}
    acc["obs_count"] = acc["obs_count"].astype(numpy.int64)
    acc["group_count"] = acc["group_count"].astype(numpy.int64)
    acc["nonfinite"] = int(acc["nonfinite"])
    for p in parts[1:]:
        for k in ("obs_state", "obs_count", "group_state", "group_count", "ty"):
            if numpy.shape(p[k]) != acc[k].shape:
                raise ValueError("partials of different shapes (%s)" % k)
        a, b = acc["obs_state"], numpy.asarray(p["obs_state"], dtype=numpy.float64)
        acc["obs_state"] = numpy.stack(_chan(a[0], a[1], a[2], b[0], b[1], b[2]))
        a, b = acc["group_state"], numpy.asarray(p["group_state"], dtype=numpy.float64)
        acc["group_state"] = numpy.stack(_chan(a[..., 0], a[..., 1], a[..., 2],
                                               b[..., 0], b[..., 1], b[..., 2]), axis=-1)
        acc["obs_count"] = acc["obs_count"] + numpy.asarray(p["obs_count"], dtype=numpy.int64)
        acc["group_count"] = acc["group_count"] + numpy.asarray(p["group_count"],
                                                                dtype=numpy.int64)
        seen_a = bool(numpy.any(a[..., 0] > 0))
        seen_b = bool(numpy.any(b[..., 0] > 0))
        tb = numpy.asarray(p["ty"], dtype=numpy.float64)
        if seen_a and seen_b and not _same_ty(acc["ty"], tb):
            raise ValueError("partials disagree on T(y): they were reduced over different data")
        if seen_b and not seen_a:
            acc["ty"] = tb.copy()
        acc["nonfinite"] += int(p["nonfinite"])
    return acc


def merge_ranks(rank_parts):
    """process_per_device: the ranks' merged partials, merged in rank order."""
    return merge(rank_parts)


def pack(part):
    """A partial as bytes (the ranks of process_per_device send theirs over the host group)."""
    return pickle.dumps({k: (numpy.ascontiguousarray(v) if isinstance(v, numpy.ndarray) else v)
                         for k, v in part.items()}, protocol=4)


def unpack(buf):
    return pickle.loads(buf)


def finish(partial, offsets, y):
    """The PpcResult of one merged partial; y [n_obs, NRESP]: the observed response fields
    (the family's table at its response_fields()).  Raises for fewer than two samples."""
    y = numpy.asarray(y, dtype=numpy.float64)
    if y.ndim == 1:
        y = y[:, None]
    n, mean, M2 = numpy.asarray(partial["obs_state"], dtype=numpy.float64)
    gs = numpy.asarray(partial["group_state"], dtype=numpy.float64)
    ns = numpy.concatenate([n.reshape(-1), gs[..., 0].reshape(-1)])
    if len(ns) and not numpy.all(ns == ns[0]):
        raise ValueError("observations and groups were reduced over different sample counts")
    S = float(ns[0]) if len(ns) else 0.0
    if S < 2:
        raise ValueError("posterior predictive checks need at least two samples (got %g)" % S)
    if y.shape != (n.shape[1], n.shape[0]):
        raise ValueError("y must be [n_obs, NRESP] = [%d, %d]" % (n.shape[1], n.shape[0]))
    with numpy.errstate(invalid="ignore"):
        sd_i = numpy.sqrt(M2 / (S - 1.0))
        t_sd = numpy.sqrt(gs[..., 2] / (S - 1.0))
    oc = numpy.asarray(partial["obs_count"], dtype=numpy.int64)
    gc = numpy.asarray(partial["group_count"], dtype=numpy.int64)
    return PpcResult(y, mean.T, sd_i.T, oc[0].T, oc[1].T, partial["ty"], gs[..., 1], t_sd,
                     gc[..., 0], gc[..., 1], S, offsets)


def stats_of(x):
    """T of x[..., n] along the last axis, the formulas as one writes them down: mean,
    population variance, minimum, maximum -> [..., 4].  The values are sorted first, so that
    equal multisets give equal statistics (a replicate that ties with the data compares equal
    whatever the order of its values; numpy's sums depend on the order in the last place)."""
    x = numpy.sort(numpy.asarray(x, dtype=numpy.float64), axis=-1)
    return numpy.stack([x.mean(axis=-1), x.var(axis=-1), x.min(axis=-1), x.max(axis=-1)], axis=-1)


def from_replicates(yrep, y, offsets):
    """The same result straight from the replicates yrep[S, n_obs, NRESP] and the observed
    y[n_obs, NRESP]: the plain host route."""
    yrep = numpy.asarray(yrep, dtype=numpy.float64)
    y = numpy.asarray(y, dtype=numpy.float64)
    if y.ndim == 1:
        y = y[:, None]
    if yrep.ndim == 2:
        yrep = yrep[:, :, None]
    if yrep.ndim != 3 or yrep.shape[1:] != y.shape:
        raise ValueError("yrep must be [S, n_obs, NRESP] and y [n_obs, NRESP]")
    S = yrep.shape[0]
    if S < 2:
        raise ValueError("posterior predictive checks need at least two samples (got %d)" % S)
    off = numpy.asarray(offsets, dtype=numpy.int64)
    G, NR = len(off) - 1, y.shape[1]
    t_obs, t_mean, t_sd = (numpy.empty((G, NR, 4)) for _ in range(3))
    gt, geq = (numpy.empty((G, NR, 4), dtype=numpy.int64) for _ in range(2))
    for g in range(G):
        a, b = off[g], off[g + 1]
        for j in range(NR):
            ty = stats_of(y[a:b, j])
            tr = stats_of(yrep[:, a:b, j])                  # [S, 4]
            t_obs[g, j] = ty
            t_mean[g, j] = tr.mean(axis=0)
            t_sd[g, j] = tr.std(axis=0, ddof=1)
            gt[g, j] = (tr > ty).sum(axis=0)
            geq[g, j] = (tr == ty).sum(axis=0)
    return PpcResult(y, yrep.mean(axis=0), yrep.std(axis=0, ddof=1), (yrep < y).sum(axis=0),
                     (yrep == y).sum(axis=0), t_obs, t_mean, t_sd, gt, geq, S, off)


HEADER_GROUPS = "group,field,statistic,t_obs,t_rep_mean,t_rep_sd,p,gt,eq,n_samples"
HEADER_POINTWISE = "obs,group,field,y,mean,sd,residual,pit,lt,eq"


def write_csvs(result, outputDirectory):
    """outputDirectory/ppc_groups.csv (one line per group, field and statistic) and
    ppc_pointwise.csv (one line per observation and field); floating-point values as %.17g,
    which reads back exactly, counts as integers."""
    r = result
    G, NR, _ = r.p.shape
    with open(os.path.join(outputDirectory, "ppc_groups.csv"), "w") as f:
        f.write(HEADER_GROUPS + "\n")
        for g in range(G):
            for j in range(NR):
                for s, name in enumerate(STATS):
                    f.write("%d,%d,%s,%.17g,%.17g,%.17g,%.17g,%d,%d,%d\n"
                            % (g, j, name, r.t_obs[g, j, s], r.t_mean[g, j, s], r.t_sd[g, j, s],
                               r.p[g, j, s], r.gt[g, j, s], r.geq[g, j, s], r.n_samples))
    group = numpy.repeat(numpy.arange(len(r.offsets) - 1), numpy.diff(r.offsets))
    with open(os.path.join(outputDirectory, "ppc_pointwise.csv"), "w") as f:
        f.write(HEADER_POINTWISE + "\n")
        f.write("".join("%d,%d,%d,%.17g,%.17g,%.17g,%.17g,%.17g,%d,%d\n"
                        % (i, group[i], j, r.y[i, j], r.mean_i[i, j], r.sd_i[i, j],
                           r.residual_i[i, j], r.pit_i[i, j], r.lt[i, j], r.eq[i, j])
                        for i in range(r.n_obs) for j in range(NR)))


def read_csvs(outputDirectory):
    """The two files back as a PpcResult (every value %.17g: exactly what was written)."""
    with open(os.path.join(outputDirectory, "ppc_groups.csv")) as f:
        assert f.readline().strip() == HEADER_GROUPS
        rows = [ln.strip().split(",") for ln in f if ln.strip()]
    G = 1 + max(int(r[0]) for r in rows)
    NR = 1 + max(int(r[1]) for r in rows)
    t_obs, t_mean, t_sd = (numpy.empty((G, NR, 4)) for _ in range(3))
    gt, geq = (numpy.empty((G, NR, 4), dtype=numpy.int64) for _ in range(2))
    S = int(rows[0][9])
    for r in rows:
        k = (int(r[0]), int(r[1]), STATS.index(r[2]))
        t_obs[k], t_mean[k], t_sd[k] = float(r[3]), float(r[4]), float(r[5])
        gt[k], geq[k] = int(r[7]), int(r[8])
    p = numpy.loadtxt(os.path.join(outputDirectory, "ppc_pointwise.csv"), delimiter=",",
                      skiprows=1, ndmin=2)
    n = p.shape[0] // NR
    cut = lambda c: p[:, c].reshape(n, NR)   # noqa: E731
    sizes = numpy.bincount(p[::NR, 1].astype(numpy.int64), minlength=G)
    off = numpy.concatenate([[0], numpy.cumsum(sizes)])
    return PpcResult(cut(3), cut(4), cut(5), cut(8).astype(numpy.int64),
                     cut(9).astype(numpy.int64), t_obs, t_mean, t_sd, gt, geq, S, off)
