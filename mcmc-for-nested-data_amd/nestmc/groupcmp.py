"""Group rankings and pairwise comparisons of a nested model's group estimates.

People who fit a partially pooled model to hospitals, schools or subjects read the group
estimates against each other: is group 17 really above group 4, where does it stand among
the G groups, and how sure is that position?  Both questions depend on the joint posterior of
a parameter's G group values within each sample -- the league-table analysis of multilevel
models (Goldstein and Spiegelhalter 1996) -- and cannot be answered from marginal medians and
intervals.  The reference has no counterpart (its Figure.bivariates only plots pairs).  This
module is the single place of definition; the device route (csrc/grouporder.h,
nmc_group_order) and the host route here (counts_from_samples) compute the same integers.

Samples and columns
  The samples are s = (recorded row, chain), S = n_rows * n_valid of them.  For parameter p
  the group values of sample s are theta_g, g = 0..G-1; theta_g is store column
  p (G + 2 partial) + 2 partial + g, the order of output.header_names: the _mu and _sigma2
  columns are not groups and are skipped.

Comparisons
  Numeric fp64 comparisons: -0.0 == +0.0, and a comparison with a NaN is false both ways.

Per-sample rank
  rank_s(p, g) = #{h : theta_h < theta_g}: 0-based and strict, tied groups share the lowest
  rank.

Counts
  H[p][g][r] = #{s : rank_s(p, g) = r}, r = 0..G-1       the rank histogram
  W[p][g][h] = #{s : theta_g > theta_h}                   the pairwise win count, W[p][g][g] = 0
  nonfinite[p] = #{(s, g) : theta_g is NaN or +-inf}; the counts are still defined by the
  comparison rules above.  A non-zero nonfinite is an error at the Engine and samplePosterior
  level, as in WAIC and LOO.

Invariants of every correct result
  sum_r H[p][g][r] = S
  sum_h W[p][g][h] = sum_r r H[p][g][r]
  W[p][g][h] + W[p][h][g] = S - #{s : theta_g == theta_h}
  (a sample in which theta_g or theta_h is NaN is in neither W: it counts with the equal ones)

Host finish (exact functions of the integers, evaluated in one fixed order)
  per (p, g):  mean_rank   = 1 + (sum_r r H) / S          (the sum an integer, one division)
               median_rank = the smallest 1-based rank whose cumulative count is >= ceil(0.5 S)
               rank_lo, rank_hi  the same at ceil(0.025 S) and ceil(0.975 S)
               p_lowest = H[.][0] / S,  p_highest = H[.][G-1] / S
  per (p, g, h):  p_greater = W / S
  The ceilings are integer expressions: (S + 1) // 2, (S + 39) // 40, (39 S + 39) // 40.

Several engines, or the ranks of process_per_device, each count their own chains' samples;
the counts and the sample numbers add (merge), so the result is the same bit for bit whatever
the batching, row window, engine count or rank count.
"""

import os

import numpy

HEADER_RANKING = "parameter,group,mean_rank,median_rank,rank_lo,rank_hi,p_lowest,p_highest"
HEADER_PAIRWISE = "parameter,group,other,wins,p_greater"
FILE_RANKING = "group_ranking.csv"
FILE_PAIRWISE = "group_pairwise.csv"


def group_columns(P, G, partial):
    """[P, G]: the store column of theta_g of parameter p."""
    pc = 2 if partial else 0
    return (numpy.arange(P)[:, None] * (G + pc) + pc) + numpy.arange(G)[None, :]


def zero_counts(P, G):
    """The counts of no samples (an engine without a real chain)."""
    return dict(hist=numpy.zeros((P, G, G), dtype=numpy.int64),
                wins=numpy.zeros((P, G, G), dtype=numpy.int64),
                nonfinite=numpy.zeros(P, dtype=numpy.int64), n_samples=0)


def counts_from_samples(raw, P, G, partial, n_valid=None):
    """The host route: raw [rows][cols][C] in the store's layout (Engine.samples_raw), chains
    [0, n_valid) -> a dict of hist [P, G, G], wins [P, G, G], nonfinite [P] (int64) and
    n_samples.  Chains from n_valid on are never read."""
    raw = numpy.asarray(raw, dtype=numpy.float64)
    if raw.ndim != 3:
        raise ValueError("raw must be [rows][cols][C]")
    rows, cols, C = raw.shape
    P, G = int(P), int(G)
    pc = 2 if partial else 0
    if G < 2:
        raise ValueError("a group comparison needs at least two groups")
    if cols != P * (G + pc):
        raise ValueError("raw has %d columns, P (G + 2 partial) = %d" % (cols, P * (G + pc)))
    n_valid = C if n_valid is None else int(n_valid)
    if not 1 <= n_valid <= C or rows < 1:
        raise ValueError("need rows >= 1 and 1 <= n_valid <= C")
    out = zero_counts(P, G)
    S = rows * n_valid
    out["n_samples"] = S
    col = group_columns(P, G, partial)
    step = max(1, (1 << 24) // (G * G))        # samples at a time: G^2 step booleans
    garange = numpy.arange(G)[None, :] * G
    for p in range(P):
        th = raw[:, col[p], :n_valid]                           # [rows, G, n_valid]
        th = numpy.ascontiguousarray(numpy.transpose(th, (0, 2, 1))).reshape(S, G)
        out["nonfinite"][p] = int(numpy.count_nonzero(~numpy.isfinite(th)))
        hist = numpy.zeros(G * G, dtype=numpy.int64)
        wins = numpy.zeros((G, G), dtype=numpy.int64)
        for s0 in range(0, S, step):
            t = th[s0:s0 + step]
            with numpy.errstate(invalid="ignore"):
                lt = t[:, None, :] < t[:, :, None]              # [s, g, h]: theta_h < theta_g
            wins += lt.sum(axis=0, dtype=numpy.int64)
            rank = lt.sum(axis=2, dtype=numpy.int64)            # [s, g]
            hist += numpy.bincount((rank + garange).ravel(), minlength=G * G)
        out["hist"][p] = hist.reshape(G, G)
        out["wins"][p] = wins
    return out


def merge(parts):
    """The int64 sum of several engines' or ranks' counts (dicts of hist, wins, nonfinite,
    n_samples) and of their sample numbers."""
    parts = list(parts)
    if not parts:
        raise ValueError("nothing to merge")
    out = dict(hist=numpy.array(parts[0]["hist"], dtype=numpy.int64),
               wins=numpy.array(parts[0]["wins"], dtype=numpy.int64),
               nonfinite=numpy.array(parts[0]["nonfinite"], dtype=numpy.int64),
               n_samples=int(parts[0]["n_samples"]))
    for q in parts[1:]:
        for k in ("hist", "wins", "nonfinite"):
            a = numpy.asarray(q[k], dtype=numpy.int64)
            if a.shape != out[k].shape:
                raise ValueError("merge: %s shapes differ" % k)
            out[k] += a
        out["n_samples"] += int(q["n_samples"])
    return out


def pack(counts):
    """A counts dict as one int64 vector (hist, wins, nonfinite, n_samples) for a gather."""
    return numpy.concatenate([numpy.asarray(counts["hist"], dtype=numpy.int64).ravel(),
                              numpy.asarray(counts["wins"], dtype=numpy.int64).ravel(),
                              numpy.asarray(counts["nonfinite"], dtype=numpy.int64).ravel(),
                              numpy.array([counts["n_samples"]], dtype=numpy.int64)])


def unpack(vec, P, G):
    """The inverse of pack."""
    vec = numpy.asarray(vec, dtype=numpy.int64)
    n = P * G * G
    if vec.shape != (2 * n + P + 1,):
        raise ValueError("unpack: wrong length")
    return dict(hist=vec[:n].reshape(P, G, G).copy(), wins=vec[n:2 * n].reshape(P, G, G).copy(),
                nonfinite=vec[2 * n:2 * n + P].copy(), n_samples=int(vec[-1]))


class GroupComparisonResult:
    """names [P]; n_samples S; hist, wins [P, G, G] (int64); per (p, g): mean_rank (float),
    median_rank, rank_lo, rank_hi (1-based, int64), p_lowest, p_highest; per (p, g, h):
    p_greater = P(theta_g > theta_h)."""

    def __init__(self, names, n_samples, hist, wins, mean_rank, median_rank, rank_lo, rank_hi,
                 p_lowest, p_highest, p_greater):
        self.names = list(names)
        self.n_samples = int(n_samples)
        self.hist, self.wins = hist, wins
        self.mean_rank, self.median_rank = mean_rank, median_rank
        self.rank_lo, self.rank_hi = rank_lo, rank_hi
        self.p_lowest, self.p_highest = p_lowest, p_highest
        self.p_greater = p_greater
        self.n_params, self.n_groups = hist.shape[0], hist.shape[1]

    def _p(self, p):
        return self.names.index(p) if isinstance(p, str) else int(p)

    def probability_greater(self, p, g, h):
        """P(theta_g > theta_h) of parameter p (its name or index): wins / S."""
        return float(self.p_greater[self._p(p), g, h])

    def ranking(self, p):
        """The groups of parameter p ordered by mean rank, lowest first (ties by group)."""
        return numpy.argsort(self.mean_rank[self._p(p)], kind="stable")


def finish(hist, wins, n_samples, names=None):
    """The GroupComparisonResult of merged counts (the docstring's host finish).  names: the
    P parameters' names (default "p<k>")."""
    hist = numpy.ascontiguousarray(hist, dtype=numpy.int64)
    wins = numpy.ascontiguousarray(wins, dtype=numpy.int64)
    S = int(n_samples)
    if hist.ndim != 3 or hist.shape[1] != hist.shape[2] or hist.shape != wins.shape:
        raise ValueError("hist and wins must both be [P, G, G]")
    if S < 1:
        raise ValueError("a group comparison needs at least one sample")
    P, G = hist.shape[:2]
    if names is None:
        names = ["p%d" % k for k in range(P)]
    if len(names) != P:
        raise ValueError("%d names for %d parameters" % (len(names), P))
    if numpy.any(hist.sum(axis=2) != S):
        raise ValueError("rank histograms do not sum to n_samples")
    r = numpy.arange(G, dtype=numpy.int64)
    mean_rank = 1.0 + (hist * r).sum(axis=2).astype(numpy.float64) / float(S)
    cum = numpy.cumsum(hist, axis=2)

    def at(need):       # the smallest 1-based rank whose cumulative count is >= need
        return (cum < need).sum(axis=2).astype(numpy.int64) + 1

    return GroupComparisonResult(
        names, S, hist, wins, mean_rank, at((S + 1) // 2), at((S + 39) // 40),
        at((39 * S + 39) // 40), hist[:, :, 0] / float(S), hist[:, :, G - 1] / float(S),
        wins / float(S))


def write_csvs(result, outputDirectory):
    """outputDirectory/group_ranking.csv (header and one line per (parameter, group)) and
    group_pairwise.csv (header and one line per ordered pair g != h); floating-point values as
    %.17g, which reads back exactly."""
    r = result
    G = r.n_groups
    with open(os.path.join(outputDirectory, FILE_RANKING), "w") as f:
        f.write(HEADER_RANKING + "\n")
        for p, name in enumerate(r.names):
            f.write("".join("%s,%d,%.17g,%d,%d,%d,%.17g,%.17g\n"
                            % (name, g, r.mean_rank[p, g], r.median_rank[p, g], r.rank_lo[p, g],
                               r.rank_hi[p, g], r.p_lowest[p, g], r.p_highest[p, g])
                            for g in range(G)))
    with open(os.path.join(outputDirectory, FILE_PAIRWISE), "w") as f:
        f.write(HEADER_PAIRWISE + "\n")
        for p, name in enumerate(r.names):
            for g in range(G):
                f.write("".join("%s,%d,%d,%d,%.17g\n"
                                % (name, g, h, r.wins[p, g, h], r.p_greater[p, g, h])
                                for h in range(G) if h != g))


def read_csvs(outputDirectory):
    """The two files of write_csvs back as a dict: names, and the arrays mean_rank,
    median_rank, rank_lo, rank_hi, p_lowest, p_highest [P, G], wins, p_greater [P, G, G]
    (diagonals 0)."""
    with open(os.path.join(outputDirectory, FILE_RANKING)) as f:
        lines = f.read().splitlines()
    if lines[0] != HEADER_RANKING:
        raise ValueError("unexpected header in " + FILE_RANKING)
    rows = [ln.split(",") for ln in lines[1:]]
    names = []
    for row in rows:
        if row[0] not in names:
            names.append(row[0])
    P, G = len(names), len(rows) // max(1, len(names))
    out = {"names": names}
    for k, key in enumerate(("mean_rank", "median_rank", "rank_lo", "rank_hi", "p_lowest",
                             "p_highest")):
        kind = numpy.int64 if key in ("median_rank", "rank_lo", "rank_hi") else numpy.float64
        out[key] = numpy.array([kind(row[2 + k]) for row in rows], dtype=kind).reshape(P, G)
    with open(os.path.join(outputDirectory, FILE_PAIRWISE)) as f:
        lines = f.read().splitlines()
    if lines[0] != HEADER_PAIRWISE:
        raise ValueError("unexpected header in " + FILE_PAIRWISE)
    out["wins"] = numpy.zeros((P, G, G), dtype=numpy.int64)
    out["p_greater"] = numpy.zeros((P, G, G))
    for ln in lines[1:]:
        name, g, h, w, pg = ln.split(",")
        p = names.index(name)
        out["wins"][p, int(g), int(h)] = int(w)
        out["p_greater"][p, int(g), int(h)] = float(pg)
    return out
