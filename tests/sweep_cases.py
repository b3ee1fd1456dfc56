"""Cases of tests/test_gpu_sweep.py and tests/test_sweep_cases.py: nmc_k_sweep (csrc/sweep.h,
csrc/sweep_gibbs.h) on every family, row width and row shape it can take.

The sweep is the step kernel of a built-in family under partial pooling over 129 to 512
groups (at most four numpy leaves) whose rows are in LDS without a row split
(csrc/nestmc.hip choose_geometry, sweep_want).  rowpath_cases.rows_fit_lds restates the LDS
condition; by it these instantiations can be chosen (the largest group that still fits, at
G = 129 / 136 / 256 / 512; tests/test_sweep_cases.py asserts the table):

    model                                   NF  P   129   136   256   512
    linreg, logistic, with intercept         1  1  8192  8192  8192  7168
                                             2  2  3008  3136  3136  1984
                                             3  3  1280  1408  1408   256
                                             4  4   416   544   544     0
                                             5  5     0    25    25     0
    linreg, logistic, without intercept      5  4   332   435   435     0
                                             6  5     0    21    21     0
    linreg, sigma sampled                    1  2  6016  6272  6272  3968
                                             2  3  1920  2112  2112   384
                                             3  4   554   725   725     0
                                             4  5     0    32    32     0
    gauss                                    1  1  8192  8192  8192  7168
                                             2  2  2496  2624  2624  1472
                                             3  3   597   725   725     0

Nothing wider fits under partial pooling with more than 128 groups: FamLinreg<7..9>,
FamLogistic<7..9> and FamGaussMean<4..9> -- twelve of the 27 instantiations of
csrc/sweep_ops.h -- are never chosen (UNREACHABLE: one model per family, asserted on the GPU
to launch nmc_k_run<..., false>).

Every reachable instantiation has a *ragged* case at the smallest G it fits.  Its sizes cycle
through 0, 1, R - 1, R, R + 1, 4 R + 1, 63, 64, 65 (R = rows.h nmc_row_block; cut to what
fits).  With an odd row width the pattern's odd counts put group starts on odd double
offsets (the prologue's plain copy) and on even ones with an odd count of doubles (its
16-byte LDS-DMA with one double of slack), and the table ends with one of the latter: the
slack double is then the first one past the observations.  The first group is empty in the
odd widths' cases and the last one in the even widths'.  *At-limit* cases hold one group of
exactly the largest size that fits (16 tiles; the pipelined loop's prefetch past a wave's
rows) among small ones, their *over* twins the same group one row larger (beyond LDS:
nmc_k_run), and the *groups* cases run the widest models that fit 512 groups at every leaf
shape (64 + 65, 64 + 72, 128 + 128, 4 x 128).  C = 64 is one chain block -- G + P workgroups,
one per CU, twelve waves each; C = 65 two, the second with one live lane, four waves each.
"""

import collections
import functools

import numpy

import rowpath_cases as rp

NCU = rp.NCU
LDS_CU = rp.LDS_CU
REACH_G = (129, 136, 256, 512)
# (kind, NF, intercept): the rows of the table above
REACH = collections.OrderedDict([
    (("linreg", 1, True), (8192, 8192, 8192, 7168)),
    (("linreg", 2, True), (3008, 3136, 3136, 1984)),
    (("linreg", 3, True), (1280, 1408, 1408, 256)),
    (("linreg", 4, True), (416, 544, 544, 0)),
    (("linreg", 5, True), (0, 25, 25, 0)),
    (("linreg", 5, False), (332, 435, 435, 0)),
    (("linreg", 6, False), (0, 21, 21, 0)),
    (("linreg_sig", 1, True), (6016, 6272, 6272, 3968)),
    (("linreg_sig", 2, True), (1920, 2112, 2112, 384)),
    (("linreg_sig", 3, True), (554, 725, 725, 0)),
    (("linreg_sig", 4, True), (0, 32, 32, 0)),
    (("gauss", 1, True), (8192, 8192, 8192, 7168)),
    (("gauss", 2, True), (2496, 2624, 2624, 1472)),
    (("gauss", 3, True), (597, 725, 725, 0)),
])
# one model per family that no G > 128 takes to the sweep (the narrowest of each)
UNREACHABLE = (("linreg", 7, True), ("logistic", 7, True), ("gauss", 4, True),
               ("linreg", 7, False), ("logistic", 9, False), ("gauss", 9, True))
FAMILY = {"linreg": "FamLinreg", "linreg_sig": "FamLinreg", "logistic": "FamLogistic",
          "gauss": "FamGaussMean"}


def shape(kind, nf, intercept=True):
    """(parameters, accumulator sets)."""
    if kind == "gauss":
        return nf, nf
    return nf - (0 if intercept else 1) + (1 if kind == "linreg_sig" else 0), 1


def max_rows(kind, nf, intercept, G):
    """The largest group whose rows are in LDS under partial pooling over G groups."""
    P, nacc = shape(kind, nf, intercept)
    n = 65536 // (nf * 8)
    while n > 0 and not rp.rows_fit_lds(n, nf, nacc, P, True, G):
        n -= 1
    return n


def sweep_columns(nacc, P, row_doubles):
    """sweep.h nmc_sweep_lds: the sweep's own carve in 512-byte columns."""
    return 1 + P + nacc * 16 + 5 * P + 6 * P + 4 + 2 + 8 + (
        (row_doubles + 63) // 64 + 1 if row_doubles else 0)


class SweepCase:
    """role: ragged, limit, over, groups, unreachable.  sweep / lds: the predicted path;
    kernel: the exact name launch_config() must report (a prefix for nmc_k_run, whose mode
    depends on residency); waves: waves_per_group of the sweep."""

    def __init__(self, name, role, kind, nf, intercept, sizes, C, seed=13):
        self.name, self.role, self.kind, self.nf, self.intercept = name, role, kind, nf, intercept
        self.sizes = [int(s) for s in sizes]
        self.G, self.C, self.seed = len(self.sizes), C, seed
        self.P, self.nacc = shape(kind, nf, intercept)
        self.n_iter = 6 if self.G >= 512 else 8
        self.sigma = "sampled" if kind == "linreg_sig" else "known"
        path = rp.predict(nf, self.sizes, self.nacc, self.P, "partial")
        self.S, self.lds = path.S, path.lds
        self.sweep = (self.lds and self.S == 1 and 128 < self.G
                      and len(rp.pairwise_leaves(self.G)) <= 4)
        self.blocks = -(-C // 64)
        fam = "%s<%d>" % (FAMILY[kind], nf)
        if self.sweep:
            self.kernel = "nmc_k_sweep<%s, NMC_MODE_SYNC_OWN>" % fam
            self.waves = 12 if self.blocks * (self.G + self.P) <= NCU else 4
        else:
            self.kernel, self.waves = "nmc_k_run<%s, " % fam, None
        self.oracle = role in ("ragged", "limit")

    def __repr__(self):
        return self.name

    @property
    def model_kind(self):
        return {"linreg_sig": "linregsig"}.get(self.kind, self.kind) + str(self.nf)

    @property
    def offsets(self):
        """Each group's first double in the observation table, and the table's end."""
        return numpy.concatenate([[0], numpy.cumsum(self.sizes)]) * self.nf

    @property
    def tiles(self):
        return [len(rp.tiles(n)) for n in self.sizes]

    def resident_batch_fits(self):
        """One chain block's likelihood workgroups beside one Gibbs workgroup within a CU's
        LDS (sweep_ops.h NMC_OP_CAN_PERSIST, the two-kernel form: what the host falls back to
        before it gives the sweep up)."""
        per = -(-self.G // NCU)
        own = sweep_columns(self.nacc, self.P, max(self.sizes) * self.nf)
        return (per * own + rp.carve_columns(0, self.P, True, self.G)) * 512 <= LDS_CU


def pattern(nf, cap):
    R = rp.row_block(nf)
    return [min(s, cap) for s in (0, 1, R - 1, R, R + 1, 4 * R + 1, 63, 64, 65)]


def ragged_sizes(nf, cap, G):
    """The pattern cycled over G groups.  Odd widths: the first group is empty and the last
    one starts on an even double offset with an odd count of doubles (the group before it is
    changed to an entry of the other parity where the cycle leaves the start odd).  Even
    widths: the cycle ends on its empty entry."""
    pat = pattern(nf, cap)
    if nf % 2 == 0:
        return [pat[(i + 1 - G) % 9] for i in range(G)]       # (sizes[G - 1] = pat[0] = 0)
    sizes = [pat[i % 9] for i in range(G)]
    sizes[-1] = max(s for s in pat if s % 2 == 1)
    if sum(sizes[:-1]) % 2 == 1:
        sizes[-2] = next(s for s in reversed(pat) if s % 2 != sizes[-2] % 2)
    return sizes


def limit_sizes(nf, big, G, at):
    """Small groups (1 .. 5 rows, odd and even) around one of ``big`` rows at index ``at``."""
    sizes = [1 + i % 5 for i in range(G)]
    sizes[at] = big
    return sizes


def _tag(kind, nf, intercept):
    return "%s%d%s" % (kind.replace("_", ""), nf, "" if intercept else "-noint")


def _cases():
    out = []
    models = list(REACH) + [(("logistic",) + k[1:]) for k in REACH if k[0] == "linreg"]
    # ragged: every instantiation and form, at the smallest G it fits, two chain blocks
    for kind, nf, intercept in models:
        G = next(G for G in (129, 136, 256) if max_rows(kind, nf, intercept, G) > 0)
        sizes = ragged_sizes(nf, max_rows(kind, nf, intercept, G), G)
        out.append(SweepCase("ragged-%s-G%d" % (_tag(kind, nf, intercept), G), "ragged", kind,
                             nf, intercept, sizes, 65))
    # at the limit of the carve, and one row beyond it: quad, paired, generic rows; gauss
    for kind, nf, G, C, at in (("linreg", 2, 129, 64, 77), ("logistic", 3, 129, 65, 128),
                               ("linreg", 5, 136, 65, 0), ("gauss", 3, 129, 65, 40)):
        big = max_rows(kind, nf, True, G)
        tag = _tag(kind, nf, True)
        out.append(SweepCase("limit-%s-G%d" % (tag, G), "limit", kind, nf, True,
                             limit_sizes(nf, big, G, at), C))
        out.append(SweepCase("over-%s-G%d" % (tag, G), "over", kind, nf, True,
                             limit_sizes(nf, big + 1, G, at), C))
    # the widest models that fit 512 groups, at every leaf shape
    for kind, nf in (("logistic", 3), ("gauss", 2)):
        for G in REACH_G:
            cap = min(max_rows(kind, nf, True, G), 200)
            out.append(SweepCase("groups-%s-G%d" % (_tag(kind, nf, True), G), "groups", kind, nf,
                                 True, ragged_sizes(nf, cap, G), 64 if G <= 136 else 65))
    # one chain block of the quad rows (twelve waves), ragged
    out.append(SweepCase("groups-linreg2-G129", "groups", "linreg", 2, True,
                         ragged_sizes(2, 200, 129), 64))
    for kind, nf, intercept in UNREACHABLE[:3]:
        out.append(SweepCase("unreachable-%s" % _tag(kind, nf, intercept), "unreachable", kind,
                             nf, intercept, [1 + i % 3 for i in range(129)], 65))
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
RUN_CASES = [c for c in CASES if c.role != "unreachable"]
SWEEP_CASES = [c for c in CASES if c.sweep]
ORACLE_CASES = [c for c in CASES if c.oracle]
# the cases of the variant, take-over and replay tests
VARIANT_CASES = ["ragged-logistic4-G129", "ragged-gauss3-G129", "ragged-linregsig2-G129",
                 "ragged-linreg3-G129"]
TAKEOVER_CASE = "ragged-logistic4-G129"
REPLAY_CASE = "groups-logistic3-G129"


@functools.lru_cache(maxsize=None)
def model(name):
    """(family, sizes) of a case: rowpath_cases.gibbs_model's data over the case's sizes."""
    c = BY_NAME[name]
    fam, sizes = rp.gibbs_model(c.model_kind, c.G, sizes=c.sizes, intercept=c.intercept)
    assert (fam.n_fields, fam.n_params) == (c.nf, c.P), (name, fam.n_fields, fam.n_params)
    return fam, sizes


def proposal_scale(case):
    """Proposal scales [P, G] of 2.4 rough posterior sds (prior precision 2 beside the rows'),
    so that groups of 0 and of 3000 rows both accept a fair share."""
    fam, sizes = model(case.name)
    nn = numpy.asarray(sizes, float)
    if case.kind == "gauss":
        sd = numpy.asarray(fam.sd)[:, None]
    else:
        sd = {"logistic": 2.2, "linreg": 1.0, "linreg_sig": 0.7}[case.kind]
    post = 1.0 / numpy.sqrt(nn[None, :] / sd ** 2 + 2.0) * numpy.ones((case.P, 1))
    if case.kind == "linreg_sig":
        post[-1] = numpy.minimum(0.7 / numpy.sqrt(2 * numpy.maximum(nn, 1.0)), 0.3)
    return 2.4 * post


@functools.lru_cache(maxsize=None)
def run_of(name):
    """The case's run: gpu_cases.partial_state's random start (a sampled sigma folded to
    |sigma| + 0.05, with its log prior and the group LLs taken again), proposal scales by group
    size, every iteration recorded (burn 0, thin 1).  The oracle runs chains 0, 1 and C - 1."""
    from gpu_cases import partial_state
    from oracle import restatement as rs
    c = BY_NAME[name]
    fam, sizes = model(name)
    st, _ = partial_state(fam, sizes, c.C, c.P)
    if c.kind == "linreg_sig":
        st.value[:, -1, :] = numpy.abs(st.value[:, -1, :]) + 0.05
        st.lp = rs.norm_logpdf(st.value, st.mu[:, :, None], numpy.sqrt(st.s2)[:, :, None])
        nested = rp.FastNested(fam, sizes)
        st.ll = numpy.array([nested.group_ll(st.value[k]) for k in range(c.C)])
    scale = numpy.broadcast_to(proposal_scale(c)[None], st.value.shape).copy()
    kw = dict(tune_interval=3, burn=0, thin=1, scale=scale)
    return rp.Run(fam, sizes, st, rp.oracle_sel(c.C), c.n_iter, c.seed, 2, kw)


@functools.lru_cache(maxsize=None)
def oracle_of(name):
    """(flags, proposal LLs, rows, least decision margin) of the oracle on the compared
    chains; computed once."""
    return rp.run_oracle_of(run_of(name))
