"""Held-out and new-group prediction from the sample store.

New data.  A table new_obs[n_new][n_fields] in the family's own row layout and width, and
new_group[n_new] (int32).  A code g >= 0 is training group g.  A code -(k + 1) is new group k,
0 <= k < K: a group the model has never seen, allowed under pooling="partial" only (its values
come from the hyper-parameters).  Any other combination raises ValueError before sampling
starts.  An observation has a held-out response when all of its response fields (the family's
response_fields()) are finite; NaN there means "predict only".

Samples are s = (chain, recorded row), S of them.

theta for a training group is the store's column q (G + pc) + pc + g, as WAIC reads it.
theta for new group k at sample (row r, chain c) and parameter q is
    theta_q = mu_q + sqrt(sigma2_q) z
with mu_q, sigma2_q that sample's <name>_mu and <name>_sigma2 columns (columns q (G + 2) and
q (G + 2) + 1 of the store: nestmc.output.header_names) and z the Box-Muller normal of the
Philox block with counter (r, k, q, purpose 5) and key (chain_base + c, seed).  A sigma2_q that
is not > 0, or not finite, gives NaN.  All observations of new group k share this theta within
a sample.

y_rep of response field j of new observation i is the family's predict on the block with
counter (r, i, j, purpose 6), i the row's position in new_obs as passed: a draw depends on
(seed, global chain, row, i, j) and on theta alone, not on the window, the sharding or the
launch geometry.  The in-sample predictive checks (nestmc.ppc) keep purpose 4: prediction and
checks never share a block.

Per new observation i, and per field j where it applies:
    mean_i, sd_i   of y_rep over the samples (sd with ddof = 1)
    lt = #{y_rep < y}, eq = #{y_rep == y}, pit = (lt + eq / 2) / S
                   (counts 0 and pit NaN without a held-out response)
    lpd_i = log((1 / S) sum_s exp(ll_is)),  ll_is the family's log density of new row i at
                   theta_s: the log predictive density of the held-out value, one value per
                   observation (NaN without a held-out response)
Totals: elpd_test = sum of lpd_i over the observations with a response, its standard error
sqrt(n var(lpd_i)) (ddof = 1), and the same sum per predicted group, training and new.

Two routes lead here.  The device route (Engine.predict, samplePosterior(predictFor=...))
never forms y_rep[S, n_new]: the GPU (csrc/predict.h) reduces a chain block to WAIC's (m, s)
of ll, Welford's (n, mean, M2) of y_rep and integer counts, and ``merge`` / ``finish`` combine
the blocks here.  The host route (``from_draws``) computes the same quantities from the draws
and the ll matrix as one writes the formulas down.  numpy only; imports without a GPU.

A partial is a dict:
  dens   [3, n_new]          float64   m = max ll, s = sum exp(ll - m), n = samples
  state  [3, NRESP, n_new]   float64   n, mean, M2 of y_rep
  count  [2, NRESP, n_new]   int64     lt, eq
  nonfinite_draws, nonfinite_ll  int   draws / ll terms (at observations with a response) that
                                       were not finite
A family that cannot draw (a DeviceLikelihood without nmc_user_predict) has NRESP = 0: its
partials carry the density alone.
"""

import os
import pickle

import numpy


class NewData:
    """obs [n_new, n_fields] (float64) and group [n_new] (int32 codes: g >= 0 a training
    group, -(k + 1) new group k); K: the new groups, 1 + the largest k used."""

    def __init__(self, obs, group):
        obs = numpy.asarray(obs, dtype=numpy.float64)
        if obs.ndim == 1:
            obs = obs[:, None]
        if obs.ndim != 2:
            raise ValueError("new observations must be (n_new, n_fields)")
        g = numpy.asarray(group)
        if g.ndim != 1 or len(g) != obs.shape[0]:
            raise ValueError("need one group code per new observation (%d rows, group has shape "
                             "%s)" % (obs.shape[0], g.shape))
        if len(g) and not numpy.issubdtype(g.dtype, numpy.integer):
            if not numpy.all(g == numpy.round(g)):
                raise ValueError("group codes must be integers")
        if obs.shape[0] == 0:
            raise ValueError("the new table is empty")
        if obs.shape[0] >= 2 ** 32:
            raise ValueError("2^32 or more new observations")
        if numpy.any(numpy.abs(numpy.asarray(g, dtype=numpy.float64)) >= 2.0 ** 31):
            raise ValueError("group codes must fit int32")
        self.obs = numpy.ascontiguousarray(obs)
        self.group = numpy.ascontiguousarray(g, dtype=numpy.int32)
        self.n_new, self.n_fields = self.obs.shape
        self.K = int(max(0, -int(self.group.min())))

    def check(self, family, n_groups, pooling):
        """Raise ValueError unless the table fits the family's width, its training group codes
        are below n_groups and its new groups come with pooling="partial"."""
        if self.n_fields != family.n_fields:
            raise ValueError("the new table has %d fields, the family's rows have %d"
                             % (self.n_fields, family.n_fields))
        if self.K > 0 and pooling != "partial":
            raise ValueError("new groups (negative group codes) take their values from the "
                             "hyper-parameters: pooling='partial' only, not %r" % (pooling,))
        if int(self.group.max()) >= int(n_groups):
            raise ValueError("group code %d: the training groups are 0..%d"
                             % (int(self.group.max()), int(n_groups) - 1))

    def y(self, response_fields):
        """[n_new, NRESP]: the table at the family's response fields."""
        return numpy.ascontiguousarray(self.obs[:, list(response_fields)])

    def has_response(self, response_fields):
        """[n_new] bool: all response fields finite (a family without any: every row)."""
        return numpy.all(numpy.isfinite(self.y(response_fields)), axis=1)

    def __repr__(self):
        return "NewData(n_new=%d, n_fields=%d, new_groups=%d)" % (self.n_new, self.n_fields, self.K)


def group_label(code):
    """"3" for training group 3, "new0" for new group 0 (code -1)."""
    code = int(code)
    return "%d" % code if code >= 0 else "new%d" % (-(code + 1))


def _code_of(label):
    return -(int(label[3:]) + 1) if label.startswith("new") else int(label)


class PredictionResult:
    """y, mean_i, sd_i, pit_i [n_new, NRESP]; lt, eq [n_new, NRESP] (int64); lpd_i [n_new];
    group [n_new] (the codes), has_response [n_new]; elpd_test, se, n_response (scalars);
    group_codes [n_g] (training groups ascending, then the new groups), elpd_g, n_g (the
    observations with a response per predicted group); n_samples, n_new."""

    def __init__(self, y, group, has_response, mean_i, sd_i, lt, eq, lpd_i, n_samples):
        f = lambda a: numpy.asarray(a, dtype=numpy.float64)   # noqa: E731
        self.y, self.mean_i, self.sd_i = f(y), f(mean_i), f(sd_i)
        self.group = numpy.asarray(group, dtype=numpy.int32)
        self.has_response = numpy.asarray(has_response, dtype=bool)
        self.n_new = len(self.group)
        self.n_samples = int(n_samples)
        S = float(self.n_samples)
        has = self.has_response
        self.lt = numpy.where(has[:, None], numpy.asarray(lt, dtype=numpy.int64), 0)
        self.eq = numpy.where(has[:, None], numpy.asarray(eq, dtype=numpy.int64), 0)
        self.pit_i = numpy.where(has[:, None], (self.lt + self.eq / 2.0) / S, numpy.nan)
        self.lpd_i = numpy.where(has, f(lpd_i), numpy.nan)
        self.n_response = int(has.sum())
        v = self.lpd_i[has]
        self.elpd_test = float(numpy.sum(v))
        self.se = float(numpy.sqrt(len(v) * numpy.var(v, ddof=1))) if len(v) > 1 \
            else float("nan")
        codes = sorted(set(int(c) for c in self.group), key=lambda c: (c < 0, abs(c)))
        self.group_codes = numpy.asarray(codes, dtype=numpy.int32)
        self.elpd_g = numpy.array([numpy.sum(self.lpd_i[has & (self.group == c)])
                                   for c in codes], dtype=numpy.float64)
        self.n_g = numpy.array([int(numpy.sum(has & (self.group == c))) for c in codes],
                               dtype=numpy.int64)

    def __repr__(self):
        return ("PredictionResult(elpd_test=%.6f, se=%.6f, n_new=%d, n_response=%d, groups=%d, "
                "n_samples=%d)" % (self.elpd_test, self.se, self.n_new, self.n_response,
                                   len(self.group_codes), self.n_samples))


def identity(n_new, n_resp=1):
    """The merge's neutral element: (-inf, 0, 0), zero states and counts."""
    d = numpy.zeros((3, int(n_new)))
    d[0] = -numpy.inf
    return dict(dens=d, state=numpy.zeros((3, int(n_resp), int(n_new))),
                count=numpy.zeros((2, int(n_resp), int(n_new)), dtype=numpy.int64),
                nonfinite_draws=0, nonfinite_ll=0)


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


def _lse(A, B):
    """WAIC's (m, s) merge with the counts: nestmc.waic._merge2 without its moments."""
    mA, sA, nA = A
    mB, sB, nB = B
    with numpy.errstate(invalid="ignore", divide="ignore", over="ignore"):
        m = numpy.maximum(mA, mB)
        s = numpy.where(nA > 0, sA * numpy.exp(mA - m), 0.0) \
            + numpy.where(nB > 0, sB * numpy.exp(mB - m), 0.0)
    out = numpy.stack([m, s, nA + nB])
    out = numpy.where(nB == 0, A, out)
    return numpy.where((nA == 0) & (nB != 0), B, out)


def merge(parts):
    """Merge partials IN THE GIVEN ORDER (A then B, left to right): counts add (int64), the
    states merge by Chan's update, the densities by WAIC's
      m = max(mA, mB);  s = sA exp(mA - m) + sB exp(mB - m), a side with n = 0 adding 0.
    The order is part of the result's definition: the same partials in the same order give the
    same bits."""
    parts = list(parts)
    if not parts:
        raise ValueError("nothing to merge")
    acc = dict(dens=numpy.array(parts[0]["dens"], dtype=numpy.float64),
               state=numpy.array(parts[0]["state"], dtype=numpy.float64),
               count=numpy.array(parts[0]["count"]).astype(numpy.int64),
               nonfinite_draws=int(parts[0]["nonfinite_draws"]),
               nonfinite_ll=int(parts[0]["nonfinite_ll"]))
    n_new = acc["dens"].shape[-1]
    if acc["dens"].shape != (3, n_new) or acc["state"].ndim != 3 \
            or acc["state"].shape[0] != 3 or acc["state"].shape[2] != n_new \
            or acc["count"].shape != (2,) + acc["state"].shape[1:]:
        raise ValueError("a partial is dens [3, n_new], state [3, NRESP, n_new], count "
                         "[2, NRESP, n_new]")
    for p in parts[1:]:
        for k in ("dens", "state", "count"):
            if numpy.shape(p[k]) != acc[k].shape:
                raise ValueError("partials of different shapes (%s)" % k)
        acc["count"] = acc["count"] + numpy.asarray(p["count"]).astype(numpy.int64)
        a, b = acc["state"], numpy.asarray(p["state"], dtype=numpy.float64)
        acc["state"] = numpy.stack(_chan(a[0], a[1], a[2], b[0], b[1], b[2]))
        acc["dens"] = _lse(acc["dens"], numpy.asarray(p["dens"], dtype=numpy.float64))
        acc["nonfinite_draws"] += int(p["nonfinite_draws"])
        acc["nonfinite_ll"] += int(p["nonfinite_ll"])
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


def finish(partial, new_data, response_fields):
    """The PredictionResult of one merged partial over new_data (a NewData) for a family with
    these response fields.  Raises for fewer than two samples."""
    m, s, n = numpy.asarray(partial["dens"], dtype=numpy.float64)
    st = numpy.asarray(partial["state"], dtype=numpy.float64)
    ct = numpy.asarray(partial["count"], dtype=numpy.int64)
    NR = len(list(response_fields))
    if m.shape != (new_data.n_new,) or st.shape != (3, NR, new_data.n_new):
        raise ValueError("the partial is not of this new table (n_new = %d, NRESP = %d)"
                         % (new_data.n_new, NR))
    ns = numpy.concatenate([n.reshape(-1), st[0].reshape(-1)])
    if not numpy.all(ns == ns[0]):
        raise ValueError("observations were reduced over different sample counts")
    S = float(ns[0])
    if S < 2:
        raise ValueError("prediction needs at least two samples (got %g)" % S)
    with numpy.errstate(invalid="ignore", divide="ignore"):
        lpd_i = m + numpy.log(s / S)
        sd_i = numpy.sqrt(st[2] / (S - 1.0))
    return PredictionResult(new_data.y(response_fields), new_data.group,
                            new_data.has_response(response_fields), st[1].T, sd_i.T, ct[0].T,
                            ct[1].T, lpd_i, S)


def from_draws(yrep, ll, y, group=None):
    """The same result straight from the draws yrep[S, n_new, NRESP], the log densities
    ll[S, n_new] and the held-out y[n_new, NRESP] (NaN: no response): the plain host route,
    the formulas as one writes them down.  group: the codes (default: all training group 0)."""
    ll = numpy.asarray(ll, dtype=numpy.float64)
    y = numpy.asarray(y, dtype=numpy.float64)
    if y.ndim == 1:
        y = y[:, None]
    yrep = numpy.asarray(yrep, dtype=numpy.float64)
    if yrep.ndim == 2:
        yrep = yrep[:, :, None]
    if ll.ndim != 2 or yrep.ndim != 3 or yrep.shape[:2] != ll.shape or yrep.shape[1:] != y.shape:
        raise ValueError("yrep must be [S, n_new, NRESP], ll [S, n_new] and y [n_new, NRESP]")
    S = ll.shape[0]
    if S < 2:
        raise ValueError("prediction needs at least two samples (got %d)" % S)
    group = numpy.zeros(y.shape[0], dtype=numpy.int32) if group is None else group
    has = numpy.all(numpy.isfinite(y), axis=1)
    with numpy.errstate(invalid="ignore", divide="ignore"):
        lpd_i = numpy.logaddexp.reduce(ll, axis=0) - numpy.log(S)
        return PredictionResult(y, group, has, yrep.mean(axis=0), yrep.std(axis=0, ddof=1),
                                (yrep < y).sum(axis=0), (yrep == y).sum(axis=0), lpd_i, S)


HEADER_POINTWISE = "obs,group,has_response,lpd,field,y,mean,sd,pit,lt,eq"
HEADER_GROUPS = "group,n_response,elpd_test,se,n_samples"


def write_csvs(result, outputDirectory):
    """outputDirectory/prediction_pointwise.csv (one line per new observation and response
    field; a family that cannot draw: one line per observation, field -1) and
    prediction_groups.csv (the line "all" with elpd_test and its standard error, then one line
    per predicted group); floating-point values as %.17g, which reads back exactly."""
    r = result
    NR = r.y.shape[1]
    with open(os.path.join(outputDirectory, "prediction_pointwise.csv"), "w") as f:
        f.write(HEADER_POINTWISE + "\n")
        for i in range(r.n_new):
            head = "%d,%s,%d,%.17g," % (i, group_label(r.group[i]), r.has_response[i],
                                        r.lpd_i[i])
            if NR == 0:
                f.write(head + "-1,nan,nan,nan,nan,0,0\n")
            for j in range(NR):
                f.write(head + "%d,%.17g,%.17g,%.17g,%.17g,%d,%d\n"
                        % (j, r.y[i, j], r.mean_i[i, j], r.sd_i[i, j], r.pit_i[i, j],
                           r.lt[i, j], r.eq[i, j]))
    with open(os.path.join(outputDirectory, "prediction_groups.csv"), "w") as f:
        f.write(HEADER_GROUPS + "\n")
        f.write("all,%d,%.17g,%.17g,%d\n" % (r.n_response, r.elpd_test, r.se, r.n_samples))
        for c, e, n in zip(r.group_codes, r.elpd_g, r.n_g):
            f.write("%s,%d,%.17g,nan,%d\n" % (group_label(c), n, e, r.n_samples))


def read_csvs(outputDirectory):
    """The two files back as a PredictionResult (every value %.17g: exactly what was written;
    the totals are formed again from the pointwise values, in the same order)."""
    with open(os.path.join(outputDirectory, "prediction_groups.csv")) as f:
        assert f.readline().strip() == HEADER_GROUPS
        S = int(f.readline().strip().split(",")[4])
    with open(os.path.join(outputDirectory, "prediction_pointwise.csv")) as f:
        assert f.readline().strip() == HEADER_POINTWISE
        rows = [ln.strip().split(",") for ln in f if ln.strip()]
    n_new = 1 + max(int(r[0]) for r in rows)
    NR = 1 + max(int(r[4]) for r in rows)
    group = numpy.zeros(n_new, dtype=numpy.int32)
    has = numpy.zeros(n_new, dtype=bool)
    lpd = numpy.empty(n_new)
    y, mean, sd = (numpy.empty((n_new, NR)) for _ in range(3))
    lt, eq = (numpy.zeros((n_new, NR), dtype=numpy.int64) for _ in range(2))
    for r in rows:
        i, j = int(r[0]), int(r[4])
        group[i], has[i], lpd[i] = _code_of(r[1]), bool(int(r[2])), float(r[3])
        if j >= 0:
            y[i, j], mean[i, j], sd[i, j] = float(r[5]), float(r[6]), float(r[7])
            lt[i, j], eq[i, j] = int(r[9]), int(r[10])
    return PredictionResult(y, group, has, mean, sd, lt, eq, lpd, S)
