"""Posterior covariance and correlation matrix of all recorded columns of a nested model.

WAIC, LOO, the convergence diagnostics and median / HDI describe every column on its own, and
the group comparison (nestmc.groupcmp) one parameter's groups; none of them describes the
joint posterior across columns.  In a nested model that is where the structure is: the
intercept and the slope of a group trade off against each other, under partial pooling every
theta_g is tied to its _mu and _sigma2 (the funnel that makes these chains mix badly), and
neighbouring groups move together through the hyper-parameters.  The reference answers this
with pictures only (Figure.bivariates, sampleDiagnosis.py:690-725, draws nFigures randomly
chosen pairs); the numeric counterpart is the covariance / correlation matrix of all columns.
This module is the single place of definition; the device route (csrc/comoment.h,
nmc_comoments) and the host route here (comoments_from_samples) follow it.

Samples and columns
  The samples are s = (recorded row, chain) over rows [row_begin, row_begin + n_rows) and local
  chains [0, n_valid): S = n_rows * n_valid of them.  The columns are k = 0..cols-1 in
  output.header_names order.

Moments
  mean[k] = (sum_s x_k) / S, the sum in one fixed order: on the device, thread t of 256 walks
  the rows in blocks of 8, within a block its chains t, t + 256, ... in order and per chain the
  block's rows in order, and the 256 partial sums are added by a binary tree (t += t + 128,
  ..., t += t + 1); on the host, numpy's sum.
  min[k], max[k] by fp64 comparison.
  nonfinite[k] = #{s : x_k is NaN or +-inf}.

Comoments
  M[k][l] = sum_s fl(x_k - mean[k]) fl(x_l - mean[l]): the differences are rounded to double,
  the products are accumulated in fp64; fused multiply-add is allowed (the device's matrix
  instruction is fused).  The order of the sum is fixed by the shape (n_rows, cols, C, n_valid)
  alone: rows in slices of a fixed number of rows, inside a slice rows in order, inside a row
  the chains in chunks of 32 and steps of 4 in order, and the slices' partial sums added in
  slice order -- no floating-point atomics.  M[k][l] and M[l][k] are the same bits.
  The bits depend on the window's values and on that shape only: not on where the window lies
  in the store, and not on what chains >= n_valid hold -- those contribute exactly +0.0 after
  the centring, not -mean.

Special columns
  A column with min == max is constant: its row and column of M are +0.0, the diagonal included.
  A column with nonfinite[k] > 0 has mean NaN and NaN in its row and column of M (also where it
  meets a constant column); no other entry changes a bit.  At the Engine.correlation and
  samplePosterior level a non-zero count is a NestmcError, as in WAIC, LOO and the group
  comparison.

Host finish (plain numpy, one fixed formula each)
  cov = M / (S - 1)                 sd[k] = sqrt(cov[k][k])
  corr[k][l] = M[k][l] / sqrt(M[k][k] M[l][l]), clipped to [-1, 1]; the diagonal is exactly 1.0;
  a constant column's row and column of corr are NaN (its diagonal too).

Several engines, or the ranks of process_per_device (merge)
  Chan's update, in engine / rank order:  n = n_a + n_b,  delta = mean_b - mean_a,
    mean = mean_a + delta n_b / n,   M = M_a + M_b + (n_a n_b / n) delta delta^T,
  min and max are taken and the nonfinite counts added; a part with n = 0 (an engine of padding
  chains only) is the identity.  The merged result is within tolerance of the one-engine
  result, NOT bit-identical to it: the parts are centred at their own means, and the rank-one
  term is rounded.

correlation_pairs.csv (pairs) -- the part of the matrix a person reads first
  within_group  for every level -- under partial pooling the _mu level and the _sigma2 level,
                then each group g -- every parameter pair p < q
  with_mu, with_sigma2  (partial pooling only) each theta_{p,g} against its own parameter's two
                hyper columns: all with_mu rows in (p, g) order, then all with_sigma2 rows
"""

import os

import numpy

FILE_MATRIX = "correlation.csv"
FILE_PAIRS = "correlation_pairs.csv"
HEADER_PAIRS = "kind,column,other,correlation"


def identity(cols):
    """The part of no samples (an engine without a real chain): merge's identity."""
    cols = int(cols)
    return dict(mean=numpy.zeros(cols), min=numpy.full(cols, numpy.inf),
                max=numpy.full(cols, -numpy.inf), M=numpy.zeros((cols, cols)),
                nonfinite=numpy.zeros(cols, dtype=numpy.int64), n_samples=0)


def comoments_from_samples(raw, n_valid=None):
    """The host route: raw [rows][cols][C] in the store's layout (Engine.samples_raw), chains
    [0, n_valid) -> a dict of mean, min, max [cols], M [cols, cols], nonfinite [cols] (int64)
    and n_samples.  Chains from n_valid on are never read."""
    raw = numpy.asarray(raw, dtype=numpy.float64)
    if raw.ndim != 3:
        raise ValueError("raw must be [rows][cols][C]")
    rows, cols, C = raw.shape
    n_valid = C if n_valid is None else int(n_valid)
    if not 1 <= n_valid <= C or rows < 1 or cols < 1:
        raise ValueError("need rows >= 1, cols >= 1 and 1 <= n_valid <= C")
    S = rows * n_valid
    if S < 2:
        raise ValueError("comoments need at least two samples")
    X = numpy.ascontiguousarray(numpy.transpose(raw[:, :, :n_valid], (1, 0, 2))).reshape(cols, S)
    bad = numpy.count_nonzero(~numpy.isfinite(X), axis=1).astype(numpy.int64)
    with numpy.errstate(invalid="ignore", over="ignore"):
        mean = X.sum(axis=1) / S
        mean[bad > 0] = numpy.nan
        mn, mx = X.min(axis=1), X.max(axis=1)
        d = X - mean[:, None]
        M = numpy.triu(d @ d.T)
    M = M + numpy.triu(M, 1).T
    const = (mn == mx) & (bad == 0)
    M[const, :] = 0.0
    M[:, const] = 0.0
    M[bad > 0, :] = numpy.nan
    M[:, bad > 0] = numpy.nan
    return dict(mean=mean, min=mn, max=mx, M=M, nonfinite=bad, n_samples=S)


def _part(p):
    M = numpy.array(p["M"], dtype=numpy.float64)
    if M.ndim != 2 or M.shape[0] != M.shape[1]:
        raise ValueError("M must be [cols, cols]")
    out = dict(mean=numpy.array(p["mean"], dtype=numpy.float64),
               min=numpy.array(p["min"], dtype=numpy.float64),
               max=numpy.array(p["max"], dtype=numpy.float64), M=M,
               nonfinite=numpy.array(p["nonfinite"], dtype=numpy.int64),
               n_samples=int(p["n_samples"]))
    for k in ("mean", "min", "max", "nonfinite"):
        if out[k].shape != (M.shape[0],):
            raise ValueError("merge: %s has the wrong shape" % k)
    return out


def merge(parts):
    """Several engines' or ranks' parts (dicts of mean, min, max, M, nonfinite, n_samples) as
    one, by Chan's update in the order given (the docstring's merge)."""
    parts = [_part(p) for p in parts]
    if not parts:
        raise ValueError("nothing to merge")
    out = parts[0]
    for q in parts[1:]:
        if q["M"].shape != out["M"].shape:
            raise ValueError("merge: M shapes differ")
        if q["n_samples"] == 0:
            continue
        if out["n_samples"] == 0:
            out = q
            continue
        na, nb = out["n_samples"], q["n_samples"]
        n = na + nb
        with numpy.errstate(invalid="ignore", over="ignore"):
            delta = q["mean"] - out["mean"]
            out["mean"] = out["mean"] + delta * (nb / n)
            out["M"] = out["M"] + q["M"] + (na * nb / n) * numpy.outer(delta, delta)
        out["min"] = numpy.minimum(out["min"], q["min"])
        out["max"] = numpy.maximum(out["max"], q["max"])
        out["nonfinite"] = out["nonfinite"] + q["nonfinite"]
        out["n_samples"] = n
    return out


def pack(part):
    """A part as one float64 vector (n_samples, mean, min, max, nonfinite, M) for a gather;
    the counts are below 2^53 and travel exactly."""
    p = _part(part)
    return numpy.concatenate([numpy.array([p["n_samples"]], dtype=numpy.float64), p["mean"],
                              p["min"], p["max"], p["nonfinite"].astype(numpy.float64),
                              p["M"].ravel()])


def unpack(vec, cols):
    """The inverse of pack."""
    vec = numpy.asarray(vec, dtype=numpy.float64)
    cols = int(cols)
    if vec.shape != (1 + 4 * cols + cols * cols,):
        raise ValueError("unpack: wrong length")
    c = cols
    return dict(n_samples=int(vec[0]), mean=vec[1:1 + c].copy(), min=vec[1 + c:1 + 2 * c].copy(),
                max=vec[1 + 2 * c:1 + 3 * c].copy(),
                nonfinite=vec[1 + 3 * c:1 + 4 * c].astype(numpy.int64),
                M=vec[1 + 4 * c:].reshape(c, c).copy())


def column_index(P, G, partial):
    """(theta [P, G], mu [P], sigma2 [P]): the store columns in output.header_names order (mu
    and sigma2 are None without partial pooling)."""
    pc = 2 if partial else 0
    base = numpy.arange(P) * (G + pc)
    theta = (base + pc)[:, None] + numpy.arange(G)[None, :]
    return (theta, base, base + 1) if partial else (theta, None, None)


class CorrelationResult:
    """parameter [cols] (the columns' names); n_samples S; mean, sd [cols]; cov, corr
    [cols, cols]; constant [cols] (bool: min == max); part: the merged moments and comoments
    the result was finished from (what merge takes: chains= shards are merged by the caller)."""

    def __init__(self, parameter, n_samples, mean, sd, cov, corr, constant, part):
        self.parameter = list(parameter)
        self.n_samples = int(n_samples)
        self.mean, self.sd, self.cov, self.corr = mean, sd, cov, corr
        self.constant = constant
        self.part = part

    def _k(self, a):
        return self.parameter.index(a) if isinstance(a, str) else int(a)

    def pair(self, a, b):
        """The correlation of columns a and b (names or indices)."""
        return float(self.corr[self._k(a), self._k(b)])

    def pairs(self, P, G, partial):
        """The rows of correlation_pairs.csv as (kind, column, other, correlation) tuples (the
        docstring's order) for P parameters, G groups and the pooling."""
        P, G = int(P), int(G)
        theta, mu, s2 = column_index(P, G, partial)
        if len(self.parameter) != P * (G + (2 if partial else 0)):
            raise ValueError("pairs: %d columns are not P (G + 2 partial)" % len(self.parameter))
        levels = ([mu, s2] if partial else []) + [theta[:, g] for g in range(G)]
        rows = [("within_group", lv[p], lv[q]) for lv in levels for p in range(P)
                for q in range(p + 1, P)]
        if partial:
            rows += [("with_mu", theta[p, g], mu[p]) for p in range(P) for g in range(G)]
            rows += [("with_sigma2", theta[p, g], s2[p]) for p in range(P) for g in range(G)]
        return [(kind, self.parameter[a], self.parameter[b], float(self.corr[a, b]))
                for kind, a, b in rows]


def finish(part, names=None):
    """The CorrelationResult of a (merged) part: the docstring's host finish.  names: the
    columns' names (default "c<k>")."""
    p = _part(part)
    S, M = p["n_samples"], p["M"]
    cols = M.shape[0]
    if S < 2:
        raise ValueError("a covariance needs at least two samples")
    if names is None:
        names = ["c%d" % k for k in range(cols)]
    if len(names) != cols:
        raise ValueError("%d names for %d columns" % (len(names), cols))
    constant = p["min"] == p["max"]
    with numpy.errstate(invalid="ignore", divide="ignore", over="ignore"):
        cov = M / (S - 1)
        dg = numpy.diagonal(M)
        sd = numpy.sqrt(numpy.diagonal(cov))
        corr = numpy.clip(M / numpy.sqrt(dg[:, None] * dg[None, :]), -1.0, 1.0)
    ok = ~constant & (dg > 0)            # (a NaN diagonal compares false)
    corr[numpy.arange(cols), numpy.arange(cols)] = numpy.where(ok, 1.0, numpy.nan)
    corr[constant, :] = numpy.nan
    corr[:, constant] = numpy.nan
    return CorrelationResult(names, S, p["mean"], sd, cov, corr, constant, p)


def csv_text(result):
    """The text of correlation.csv: the square matrix, a parameter column and one column per
    name, in header order and the number format of convergence.csv."""
    r = result
    head = "parameter," + ",".join("'%s'" % n for n in r.parameter)
    return head + "\n" + "".join(
        "'%s',%s\n" % (n, ",".join("%.6f" % v for v in r.corr[k]))
        for k, n in enumerate(r.parameter))


def pairs_csv_text(result, P, G, partial):
    """The text of correlation_pairs.csv (CorrelationResult.pairs)."""
    return HEADER_PAIRS + "\n" + "".join(
        "%s,'%s','%s',%.6f\n" % row for row in result.pairs(P, G, partial))


def write_csvs(result, directory, P, G, partial):
    """directory/correlation.csv (csv_text) and correlation_pairs.csv (pairs_csv_text)."""
    with open(os.path.join(directory, FILE_MATRIX), "w") as f:
        f.write(csv_text(result))
    with open(os.path.join(directory, FILE_PAIRS), "w") as f:
        f.write(pairs_csv_text(result, P, G, partial))


def read_csvs(directory):
    """The two files of write_csvs back: a dict of parameter (names), corr [cols, cols] and
    pairs (a list of (kind, column, other, correlation))."""
    with open(os.path.join(directory, FILE_MATRIX)) as f:
        lines = f.read().splitlines()
    head = lines[0].split(",")
    if head[0] != "parameter":
        raise ValueError("unexpected header in " + FILE_MATRIX)
    names = [h.strip("'") for h in head[1:]]
    corr = numpy.array([[float(v) for v in ln.split(",")[1:]] for ln in lines[1:]])
    if [ln.split(",")[0].strip("'") for ln in lines[1:]] != names:
        raise ValueError("rows and columns of " + FILE_MATRIX + " differ")
    with open(os.path.join(directory, FILE_PAIRS)) as f:
        lines = f.read().splitlines()
    if lines[0] != HEADER_PAIRS:
        raise ValueError("unexpected header in " + FILE_PAIRS)
    pairs = []
    for ln in lines[1:]:
        kind, a, b, v = ln.split(",")
        pairs.append((kind, a.strip("'"), b.strip("'"), float(v)))
    return dict(parameter=names, corr=corr.reshape(len(names), len(names)), pairs=pairs)
