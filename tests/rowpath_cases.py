"""Cases, path arithmetic and the extended-precision reference of tests/test_gpu_rowpaths.py
and tests/test_rowpath_reference.py.

* ``predict`` restates, in Python, how csrc/nestmc.hip (nmc_create, choose_geometry) picks
  the row split and whether a member's rows live in LDS -- from (n_fields, rows per group,
  groups, parameters, pooling) alone.  The GPU tests assert the device's launch_config()
  against it, so a case that stops reaching its path fails.
* ``reference`` evaluates the three families' group log-likelihoods in numpy.longdouble
  (per-row terms and their sum), with the formulas of nestmc/families.py, and returns
  beside each sum ``ref`` the same sum with every addend replaced by its absolute value,
  ``A`` -- the scale of ``tolerance``.
* USER_CASES and the helpers after them are the same for runtime-compiled user families
  (tests/test_gpu_user_rowpaths.py, tests/test_user_rowpath_cases.py): rows of up to 64
  fields, the staged loop's chunk arithmetic, the step-kernel instance by pooling and Gibbs
  hand-off, and the parameter limit of the partial-pooling workgroup state.
"""

import collections
import contextlib
import functools
import os

import numpy
import scipy.stats

from nestmc.families import GaussianMean, LinearRegression, Logistic

LD = numpy.longdouble
U = 2.0 ** -53
PI_LD = 4 * numpy.arctan(LD(1))
LOG_C_LD = numpy.log(2 * PI_LD) / 2          # log sqrt(2 pi)
NCU = 256                                    # CUs of an MI355X (the half-layout condition)


# ---------------------------------------------------------------------------------------
# path arithmetic (csrc/rows.h nmc_row_block, csrc/dev.h nmc_lds; csrc/nestmc.hip)
# ---------------------------------------------------------------------------------------
def row_block(nf):
    """rows.h nmc_row_block: rows per block of the scalar-load / staged loops."""
    if nf <= 4:
        return 16 // nf
    return 4 if 32 // nf >= 4 else max(32 // nf, 1)


def stage_rows(nf):
    """rows.h nmc_stage_rows: rows per chunk of the staged loop -- whole row blocks within the
    1008 bytes one 1 KiB DMA carries beside 16 B of alignment slack, at least one block."""
    R = row_block(nf)
    return R * ((1008 // (nf * 8)) // R) if (1008 // (nf * 8)) // R > 0 else R


def stage_buf(nf):
    """rows.h nmc_stage_buf: doubles of one staging buffer (whole 1 KiB DMAs)."""
    return ((stage_rows(nf) * nf + 2) * 8 + 1023) // 1024 * 128


def pairwise_leaves(G):
    """Leaf lengths of numpy's pairwise sum over G elements (nestmc.hip pairwise_plan)."""
    if G <= 128:
        return [G]
    n2 = G // 2
    n2 -= n2 % 8
    return pairwise_leaves(n2) + pairwise_leaves(G - n2)


def carve_columns(nacc, P, partial, G):
    """dev.h nmc_lds without the rows and without a Gibbs payload: 512-byte columns."""
    leaves = pairwise_leaves(G)
    ntail = max(m - (m - m % 8 if m >= 8 else 0) for m in leaves)
    cols = P + nacc * 16 + 5 * P + 4 + 8 + 1
    if partial:
        cols += 6 * P + P * len(leaves) * (8 + ntail) + P * len(leaves) + 2 * P
    return cols


def rows_fit_lds(n_member, nf, nacc, P, partial, G):
    """choose_geometry's Dev.rows_lds: 64 KiB of rows, inside a 96 KiB carve."""
    doubles = n_member * nf
    cols = carve_columns(nacc, P, partial, G) + ((doubles + 63) // 64 + 1 if doubles else 0)
    return doubles * 8 <= 65536 and cols * 512 <= 96 * 1024


Path = collections.namedtuple("Path", "S n_member lds")


def predict(nf, sizes, nacc, P, pooling):
    G, nmax = len(sizes), max(sizes)
    target = max(256, 65536 // (nf * 8))
    S = 1
    if nmax > 2 * target:
        S = min(64, -(-nmax // target), max(1, 256 // G))
    n_member = -(-nmax // S)
    return Path(S, n_member, rows_fit_lds(n_member, nf, nacc, P, pooling == "partial", G))


# ---------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------
def family_shape(kind, nf):
    """(parameters, accumulator sets) of a case kind over nf fields."""
    P = {"linreg_sig": nf + 1, "wide": 2}.get(kind, nf)
    return P, (nf if kind == "gauss" else 1)


class RowCase:
    """kind: linreg (sigma = 1 known), linreg_sig (sigma sampled), gauss, logistic; the user
    families of tests/user_models.py: wide (theta [a, b] over nf - 1 weighted fields), coef
    (one coefficient per field)."""

    def __init__(self, name, kind, nf, sizes, pooling, lds, S, step_iters=8, P=None):
        self.name, self.kind, self.nf, self.pooling = name, kind, nf, pooling
        self.sizes = [int(s) for s in sizes]
        self.lds, self.S, self.step_iters = lds, S, step_iters
        self.P, self.nacc = family_shape(kind, nf)
        if P is not None:       # (a user family's parameters need not follow its fields)
            self.P = P
        self.G = len(self.sizes)

    def __repr__(self):
        return self.name

    @property
    def path(self):
        return predict(self.nf, self.sizes, self.nacc, self.P, self.pooling)

    @property
    def n_member(self):
        return self.path.n_member


def max_lds_rows(kind, nf, pooling, G):
    """The largest group that still has its rows in LDS (unsplit)."""
    P, nacc = family_shape(kind, nf)
    n = 65536 // (nf * 8)
    while n > 0 and not rows_fit_lds(n, nf, nacc, P, pooling == "partial", G):
        n -= 1
    return n


def _cases():
    out = []
    # tile partition edges of nmc_tiles, one ragged engine.  The issue's at-limit group of
    # 4096 {x, y} rows (exactly 64 KiB) does not fit the 96 KiB carve under partial pooling
    # (83 columns of state beside the rows): the largest group that does, 3456 rows, stands
    # in for it -- still 16 tiles of more than 64 rows
    big = max_lds_rows("linreg", 2, "partial", 12)
    out.append(RowCase("tiles", "linreg", 2, [1, 15, 16, 17, 0, 63, 64, 65, 1023, 1024, 1025, big],
                       "partial", True, 1))
    # the same edges on y-only rows, whose summation order numpy can restate exactly
    # (linreg1_fixed_order)
    out.append(RowCase("order-linreg1", "linreg", 1, [1, 15, 16, 17, 0, 63, 64, 65, 1023, 1024, 1025],
                       "none", True, 1))
    # ends of the none-pooling tile-balance window (7 likelihood waves: 449 .. 832 rows)
    for n in (449, 832, 833):
        out.append(RowCase("balance-%d" % n, "gauss", 3, [n, 7, 0, 100, 300], "none", True, 1))
    # every template instance, at the row-block edges of the generic loops.  None pooling:
    # under partial pooling the hyper state of 9 parameters leaves the rows no room in the
    # carve.  gauss keeps one accumulator set per field (16 partial-sum columns each), so at
    # nf = 8 only 16 rows fit the carve (sizes above are cut to that) and at nf = 9 none do:
    # that instance can only run, and is asserted, beyond LDS
    for kind in ("linreg", "gauss", "logistic"):
        for nf in range(1, 10):
            R = row_block(nf)
            sizes = [1, R - 1, R, R + 1, 4 * R + 1, 200, 0]
            cap = max_lds_rows(kind, nf, "none", len(sizes))
            if cap > 0:
                sizes = [min(s, cap) for s in sizes]
            out.append(RowCase("R-%s-nf%d" % (kind, nf), kind, nf, sizes, "none", cap > 0, 1))
    # the scalar-load loop of the step kernel: <= 4 fields, beyond LDS, below the split
    out.append(RowCase("scalar-linreg2-4097", "linreg", 2, [4097, 0, 1, 17], "partial", False, 1))
    out.append(RowCase("scalar-linreg2-8192", "linreg", 2, [0, 1, 17, 8192], "partial", False, 1))
    out.append(RowCase("scalar-linreg2sig-8192", "linreg_sig", 2, [17, 8192, 0, 1], "none",
                       False, 1))
    out.append(RowCase("scalar-logistic4-2049", "logistic", 4, [2049, 0, 1, 17], "none", False, 1))
    out.append(RowCase("scalar-gauss3-2731", "gauss", 3, [0, 2731, 1, 17], "none", False, 1))
    out.append(RowCase("scalar-linreg1-8193", "linreg", 1, [0, 1, 17, 8193], "none", False, 1))
    # the staged loop: > 4 fields beyond LDS.  Odd nf with the odd small groups puts group
    # starts (big group last) and group ends (big group first) on odd double offsets; the
    # big group last is the end of the table
    for kind, nf, n in (("logistic", 5, 1639), ("logistic", 7, 1171), ("logistic", 8, 1025),
                        ("logistic", 9, 911), ("linreg", 9, 911)):
        out.append(RowCase("staged-%s%d-last" % (kind, nf), kind, nf, [0, 1, 3, 13, n], "none",
                           False, 1))
        out.append(RowCase("staged-%s%d-first" % (kind, nf), kind, nf, [n, 0, 1, 3, 13], "none",
                           False, 1))
    out.append(RowCase("staged-gauss9", "gauss", 9, [5, 0, 1, 37, 12], "none", False, 1))
    # row split
    out.append(RowCase("split-lds", "linreg_sig", 2, [8193], "complete", True, 3))
    rs = numpy.random.RandomState(100)
    small = list(rs.randint(0, 40, size=99))
    small[3] = 0
    out.append(RowCase("split-scalar", "logistic", 4, small[:50] + [4200] + small[50:], "none",
                       False, 2, step_iters=6))
    out.append(RowCase("split-staged", "logistic", 8, small[:50] + [2100] + small[50:], "none",
                       False, 2, step_iters=6))
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}


# ---------------------------------------------------------------------------------------
# user-family cases (tests/test_gpu_user_rowpaths.py, tests/test_user_rowpath_cases.py)
# ---------------------------------------------------------------------------------------
# the logistic cases of the matrix above, run again as a user family (user_models.user_logistic)
USER_LOGISTIC = (["R-logistic-nf%d" % nf for nf in range(1, 10)] + ["scalar-logistic4-2049"]
                 + ["staged-logistic%d-%s" % (nf, e) for nf in (5, 7, 8, 9)
                    for e in ("first", "last")] + ["split-scalar", "split-staged"])
# partial pooling beyond LDS, unsplit: the scalar-load loop (one group past 64 KiB of rows) and
# the staged loop (seven parameters' hyper state leaves the rows no room in the 96 KiB carve,
# whatever the group sizes; odd n_fields x odd row counts: odd double offsets)
USER_PARTIAL = [RowCase("partial-scalar-logistic4", "logistic", 4, [2049, 0, 1, 17], "partial",
                        False, 1),
                RowCase("partial-staged-logistic7", "logistic", 7, [301, 0, 1, 13], "partial",
                        False, 1)]
# row widths no built-in family has: where nmc_row_block, nmc_stage_rows and nmc_stage_buf
# change regime (R = 3, 2, 1; 32 / nf == 0; two rows filling the 1 KiB buffer to the last
# double; one row per chunk), and 11 / 32, the far ends of R = 2 and R = 1
WIDE_WIDTHS = (10, 11, 16, 17, 32, 33, 63, 64)
COEF_NF = 16      # the P = 16 model: one coefficient per field


def _wide_cases(kind, nf):
    R = row_block(nf)
    sizes = [1, R - 1, R, R + 1, 4 * R + 1, 37, 0]
    cap = max_lds_rows(kind, nf, "none", len(sizes))
    assert cap >= 37, (kind, nf, cap)
    # one group just past the LDS row area, with an odd row count, among small odd groups
    big = max_lds_rows(kind, nf, "none", 5) + 1
    big += 1 - big % 2
    tag = "%s%d" % (kind, nf)
    return [RowCase(tag + "-lds", kind, nf, sizes, "none", True, 1),
            RowCase(tag + "-staged-last", kind, nf, [0, 1, 3, 13, big], "none", False, 1),
            RowCase(tag + "-staged-first", kind, nf, [big, 0, 1, 3, 13], "none", False, 1)]


WIDE_CASES = {nf: _wide_cases("wide", nf) for nf in WIDE_WIDTHS}
COEF_CASES = _wide_cases("coef", COEF_NF)
USER_CASES = USER_PARTIAL + [c for nf in WIDE_WIDTHS for c in WIDE_CASES[nf]] + COEF_CASES
BY_NAME.update({c.name: c for c in USER_CASES})


def want_half(case, n_chains):
    """choose_geometry: none/complete pooling on the paired loop (rows in LDS, <= 4 fields,
    any family) whose 64-chain grid fills at most half the CUs runs 32 chains per workgroup."""
    blocks = -(-n_chains // 64)
    return (case.pooling != "partial" and case.S == 1 and case.lds and case.nf <= 4
            and blocks * case.G * 2 <= NCU)


def run_columns(nf, n_member, nacc, P, partial, G, lds, payload=False):
    """ctx.h lds_bytes_for in 512-byte columns: the carve, the two Gibbs payload buffers
    (SYNC_LDS) and the member's rows or, beyond LDS with more than 4 fields, every wave's two
    staging buffers (choose_geometry's wave count: control + one per 64 rows + the Gibbs wave,
    at most 8)."""
    w = 1 + (n_member + 63) // 64
    w = min(8, w + 1 if partial and w >= 2 else w)
    doubles = n_member * nf if lds else (0 if nf <= 4 else w * 2 * stage_buf(nf))
    return (carve_columns(nacc, P, partial, G) + (2 * (G + 1) if partial and payload else 0)
            + ((doubles + 63) // 64 + 1 if doubles else 0))


LDS_CU = 160 * 1024       # choose_kernel refuses a workgroup state beyond it


def user_step_kernel(case, n_chains, env=None):
    """(kernel name, persistent) nmc_launch_config reports for a user family on ``case``:
    choose_geometry's mode by pooling, Gibbs hand-off and NMC_PERSIST / NMC_HALF / NMC_ROWS,
    with the rows suffix of predict().  A user family never sweeps."""
    env = env or {}
    p = case.path
    assert (p.lds, p.S) == (case.lds, case.S), (case.name, p)
    persistent = True     # (none / complete pooling: one launch runs all the iterations)
    if case.pooling != "partial":
        half = (want_half(case, n_chains) and env.get("NMC_HALF") != "0"
                and env.get("NMC_ROWS") != "bcast")
        mode = "HALF" if half else "NOPOOL"
    else:
        args = (case.nf, p.n_member, case.nacc, case.P, True, case.G, p.lds)
        assert run_columns(*args) * 512 <= LDS_CU, case.name
        w = 1 + (p.n_member + 63) // 64
        naux = w + 1 >= 3 and len(pairwise_leaves(case.G)) <= 4
        hlds = naux and case.G <= 128 and run_columns(*args, payload=True) * 512 <= LDS_CU
        persistent = env.get("NMC_PERSIST") != "0"
        mode = ("LAUNCH" if not persistent else
                "SYNC_REG" if hlds and case.G <= 64 else "SYNC_LDS" if hlds else "SYNC")
    return ("nmc_k_run<FamUser, NMC_MODE_%s, %s>" % (mode, "true" if p.lds else "false"),
            persistent)


def user_gibbs_mode(fam, sizes):
    """gibbs_mode for a user family: nmc_k_sweep takes built-in families only
    (choose_geometry's sweep_want), so more than one numpy leaf runs nmc_k_run's all-wave
    update."""
    kernel, modes = gibbs_mode(fam, sizes)
    if kernel == "nmc_k_sweep<":
        return "nmc_k_run<", ("NMC_MODE_SYNC", "NMC_MODE_LAUNCH")
    return kernel, modes


def gibbs_persistent(G, C):
    """Whether the partial-pooling grid of C chains over G small groups is co-resident, and so
    runs persistent: the workgroup states of the user Gibbs cases are beyond 53 KiB, where the
    residency rule (ctx.h nmc_safe_blocks over the occupancy of 160 KiB of LDS) keeps one
    workgroup per CU."""
    return -(-C // 64) * G <= NCU


def max_partial_params(nf, n_member, G):
    """The largest n_params whose partial-pooling workgroup state (rows beyond LDS where the
    96 KiB carve has no room for them) fits the CU's 160 KiB: what choose_kernel accepts."""
    best = 0
    for P in range(1, 17):
        lds = rows_fit_lds(n_member, nf, 1, P, True, G)
        if run_columns(nf, n_member, 1, P, True, G, lds) * 512 <= LDS_CU:
            best = P
    return best

Model = collections.namedtuple("Model", "fam priors truth post_sd")


@functools.lru_cache(maxsize=None)
def model(name):
    """The case's family object and priors, the parameters its data were drawn from
    ([P, G]) and a rough posterior sd per (parameter, group) -- the proposal scale's basis."""
    c = BY_NAME[name]
    r = numpy.random.RandomState(sum(map(ord, name)))
    sizes = numpy.asarray(c.sizes)
    n, G, nf = int(sizes.sum()), c.G, c.nf
    grp = numpy.repeat(numpy.arange(G), sizes)
    nn = numpy.maximum(sizes, 0).astype(float)
    prior_prec = 2.0 if c.pooling == "partial" else 0.01
    if c.kind == "gauss":
        mu = r.normal(size=(nf, G))
        sd = r.uniform(0.5, 1.5, size=nf)
        fam = GaussianMean.from_groups(mu, sd, c.sizes)
        truth = mu
        post = 1.0 / numpy.sqrt(nn[None, :] / sd[:, None] ** 2 + prior_prec)
    elif c.kind in ("wide", "coef"):
        import user_models
        x = r.normal(size=(n, nf - 1))
        if c.kind == "wide":
            w = user_models.wide_weights(nf)
            truth = numpy.vstack([r.normal(size=G), r.normal(1.0, 0.5, size=G)])
            y = truth[0, grp] + truth[1, grp] * (x @ w) + r.normal(size=n)
            fam = user_models.wide_family(numpy.hstack([x, y[:, None]]))
            post = 1.0 / numpy.sqrt(nn[None, :] * numpy.array([[1.0], [w @ w]]) + prior_prec)
        else:
            truth = r.normal(0, 0.5, size=(nf, G))
            y = truth[0, grp] + numpy.sum(x * truth[1:, grp].T, axis=1) + r.normal(size=n)
            fam = user_models.coef_family(numpy.hstack([x, y[:, None]]))
            post = 1.0 / numpy.sqrt(nn[None, :] + prior_prec) * numpy.ones((nf, 1))
    else:
        K = nf - 1
        X = numpy.hstack([numpy.ones((n, 1)), r.normal(size=(n, K))])
        beta = r.normal(0, 0.5, size=(nf, G))
        eta = numpy.sum(X * beta[:, grp].T, axis=1)
        if c.kind == "logistic":
            y = (r.uniform(size=n) < 1 / (1 + numpy.exp(-eta))).astype(float)
            fam = Logistic(X, y)
            truth = beta
            post = 1.0 / numpy.sqrt(nn[None, :] / 2.2 ** 2 + prior_prec) * numpy.ones((nf, 1))
        else:
            sig = 1.0 if c.kind == "linreg" else 0.7
            y = eta + sig * r.normal(size=n)
            fam = LinearRegression(X, y, sigma=1.0 if c.kind == "linreg" else None)
            truth = beta
            post = 1.0 / numpy.sqrt(nn[None, :] / sig ** 2 + prior_prec) * numpy.ones((nf, 1))
            if c.kind == "linreg_sig":
                truth = numpy.vstack([beta, numpy.full((1, G), sig)])
                ps = numpy.minimum(sig / numpy.sqrt(2 * numpy.maximum(nn, 1.0)), 0.3)
                post = numpy.vstack([post, ps[None, :]])
    priors = None
    if c.pooling != "partial":
        priors = [scipy.stats.norm(0, 10)] * (2 if c.kind == "wide" else nf)
        if c.kind == "linreg_sig":
            priors = priors + [scipy.stats.gamma(2)]
    assert fam.n_fields == nf and fam.n_params == c.P, (fam.n_fields, fam.n_params)
    return Model(fam, priors, truth, post)


def thetas(name, C, seed=1):
    """Random parameters of posterior-like scale around the truth: [C, P, G]."""
    c, m = BY_NAME[name], model(name)
    r = numpy.random.RandomState(seed)
    th = m.truth[None] + 0.2 * r.normal(size=(C, c.P, c.G))
    if c.kind == "linreg_sig":
        th[:, -1, :] = 0.7 + r.uniform(0, 0.5, size=(C, c.G))
    return th


def start(name, C, seed=2):
    """A start near the posterior: (value, log prior, mu, s2, proposal scale).  The scale
    is 2.4 posterior sd per (parameter, group), so that big groups still accept."""
    from oracle import restatement as rs
    c, m = BY_NAME[name], model(name)
    r = numpy.random.RandomState(seed)
    value = m.truth[None] + m.post_sd[None] * r.normal(size=(C, c.P, c.G))
    if c.kind == "linreg_sig":
        value[:, -1, :] = numpy.abs(value[:, -1, :]) + 0.05
    scale = numpy.broadcast_to(2.4 * m.post_sd[None], value.shape).copy()
    if c.pooling == "partial":
        mu = m.truth.mean(axis=1)[None] + r.normal(0, 0.2, size=(C, c.P))
        s2 = r.uniform(0.3, 0.8, size=(C, c.P))
        lp = rs.norm_logpdf(value, mu[:, :, None], numpy.sqrt(s2)[:, :, None])
        return value, lp, mu, s2, scale
    lp = numpy.stack([numpy.asarray(m.priors[p].logpdf(value[:, p, :])) for p in range(c.P)], 1)
    return value, lp, None, None, scale


# ---------------------------------------------------------------------------------------
# extended-precision reference
# ---------------------------------------------------------------------------------------
def reference(fam, sizes, theta):
    """Group log-likelihoods of theta [C, P, G] in numpy.longdouble: (ref, A), each [C, G].

    A is ref with every addend replaced by its absolute value.  For the regression the
    residual is taken as sum |b_j x_j| + |y| before squaring; log sqrt(2 pi) and |log sigma|
    count once per row."""
    theta = numpy.asarray(theta)
    C, P, G = theta.shape
    obs = numpy.asarray(fam.obs()).astype(LD)
    off = numpy.concatenate([[0], numpy.cumsum(sizes)])
    ref = numpy.zeros((C, G), LD)
    A = numpy.zeros((C, G), LD)
    for g in range(G):
        rows = obs[off[g]:off[g + 1]]
        if rows.shape[0] == 0:
            continue
        th = theta[:, :, g].astype(LD)                         # [C, P]
        if getattr(fam, "model", None) is not None:            # user_models wide / coef
            ll, a = _user_rows(fam, rows, th)
            ref[:, g], A[:, g] = ll.sum(axis=1), a.sum(axis=1)
            continue
        if isinstance(fam, GaussianMean):
            sd = fam.sd.astype(LD)
            e = (th[:, None, :] - rows[None, :, :]) / sd        # [C, n, P]
            const = LOG_C_LD + numpy.log(sd)
            ref[:, g] = (-(e * e) / 2 - const).sum(axis=(1, 2))
            A[:, g] = ((e * e) / 2 + LOG_C_LD + numpy.abs(numpy.log(sd))).sum(axis=(1, 2))
            continue
        K = fam.n_fields - 1
        assert fam.intercept
        x, y = rows[:, :K], rows[:, K]
        b0, b = th[:, 0], th[:, 1:1 + K]
        eta = b0[:, None] + (b[:, None, :] * x[None, :, :]).sum(axis=2)         # [C, n]
        if isinstance(fam, Logistic):
            sp = numpy.logaddexp(LD(0), eta)
            ref[:, g] = (y[None, :] * eta - sp).sum(axis=1)
            A[:, g] = (numpy.abs(y[None, :] * eta) + numpy.abs(sp)).sum(axis=1)
            continue
        sig = (th[:, K + 1] if fam.sigma is None else numpy.full(C, LD(fam.sigma)))[:, None]
        res = (eta - y[None, :]) / sig
        ref[:, g] = (-(res * res) / 2 - LOG_C_LD - numpy.log(sig)).sum(axis=1)
        ra = (numpy.abs(b0)[:, None] + (numpy.abs(b)[:, None, :] * numpy.abs(x)[None]).sum(axis=2)
              + numpy.abs(y)[None, :]) / sig
        A[:, g] = ((ra * ra) / 2 + LOG_C_LD + numpy.abs(numpy.log(sig))).sum(axis=1)
    return ref, A


def _user_rows(fam, rows, th):
    """Per-row terms of the user models of tests/user_models.py in longdouble: rows [n, nf],
    th [C, P] -> (ll, a), each [C, n].  Both are ll = -(y - eta)^2 / 2; a takes the residual
    as |a| + |b| sum |w_j x_j| + |y| (wide) or |b_0| + sum |b_j x_j| + |y| (coef) before
    squaring, like the regression's."""
    import user_models
    nf = rows.shape[1]
    x, y = rows[:, :nf - 1], rows[:, nf - 1]
    if fam.model == "wide":
        w = user_models.wide_weights(nf).astype(LD)
        # (the weights are the float64 constants the device holds, products in field order)
        eta = th[:, 0, None] + th[:, 1, None] * (x * w[None, :]).sum(axis=1)[None, :]
        ra = (numpy.abs(th[:, 0, None]) + numpy.abs(th[:, 1, None])
              * numpy.abs(x * w[None, :]).sum(axis=1)[None, :] + numpy.abs(y)[None, :])
    else:
        assert fam.model == "coef", fam.model
        eta = th[:, 0, None] + (th[:, None, 1:] * x[None, :, :]).sum(axis=2)
        ra = (numpy.abs(th[:, 0, None]) + (numpy.abs(th[:, None, 1:]) * numpy.abs(x)[None]).sum(axis=2)
              + numpy.abs(y)[None, :])
    e = y[None, :] - eta
    return -(e * e) / 2, (ra * ra) / 2


def reference_rows(fam, sizes, theta):
    """Per-observation log-likelihoods of a user model at theta [C, P, G] in longdouble:
    (ref, A), each [C, n_obs]."""
    theta = numpy.asarray(theta)
    obs = numpy.asarray(fam.obs()).astype(LD)
    off = numpy.concatenate([[0], numpy.cumsum(sizes)])
    ref = numpy.zeros((theta.shape[0], obs.shape[0]), LD)
    A = numpy.zeros_like(ref)
    for g in range(theta.shape[2]):
        if off[g + 1] > off[g]:
            ref[:, off[g]:off[g + 1]], A[:, off[g]:off[g + 1]] = _user_rows(
                fam, obs[off[g]:off[g + 1]], theta[:, :, g].astype(LD))
    return ref, A


def bound_units(n_member, nf, chain=None):
    """The derived bound in units of 2^-53 A.

    n_member / 64: first-order summation bound of the longest addition chain of the kernels'
    fixed order (a tile of at most n_member / 16 + 80 rows over 4 accumulators, then the
    4-way, the 16-slot and the <= 64-member four-way combines).  48 + 4 (nf + 4): the per-row
    evaluation (a dot product of nf terms squared or fed to the softplus, whose 2.5 ulp
    tests/test_softplus.py pins).  chain: the additions of the longest chain of another
    summation order, in place of the kernels' n_member / 64 (the oracle's sequential sum of
    n rows: n - 1)."""
    return (n_member / 64.0 if chain is None else chain) + 48 + 4 * (nf + 4)


def tolerance(n_member, nf, ref, A, chain=None):
    """min(derived bound, the suite's 1e-10 relative + 1e-9): float64 [C, G]."""
    derived = bound_units(n_member, nf, chain) * U * numpy.asarray(A, float)
    return numpy.minimum(derived, 1e-10 * numpy.abs(numpy.asarray(ref, float)) + 1e-9)


def ratio(got, ref, A):
    """|got - ref| / (2^-53 A), 0 where A is 0 (empty groups: got must be 0 there)."""
    err = numpy.abs(numpy.asarray(got).astype(LD) - ref)
    with numpy.errstate(invalid="ignore", divide="ignore"):
        out = numpy.where(A > 0, err / (U * A), 0)
    return numpy.asarray(out, float)


class FastNested:
    """oracle.restatement.Nested with the parameters handed to the family as arrays, not
    lists: the same float64 operations and the same sequential sums, without the list
    round trip (the Gibbs edge tests run the oracle on every chain)."""

    def __init__(self, ll_function, sizes):
        from oracle import restatement as rs
        self._n = rs.Nested(ll_function, sizes)
        self.f, self.sizes, self.off, self.n_total = (self._n.f, self._n.sizes, self._n.off,
                                                      self._n.n_total)

    @property
    def G(self):
        return len(self.sizes)

    def obs_ll(self, theta_pg):
        param = [numpy.repeat(numpy.asarray(t, float), self.sizes) for t in theta_pg]
        return numpy.asarray(self.f(param), dtype=numpy.float64)

    def group_ll(self, theta_pg):
        ll = self.obs_ll(theta_pg)
        out = numpy.zeros(self.G)
        for g in range(self.G):
            a, b = self.off[g], self.off[g + 1]
            if b > a:
                out[g] = numpy.cumsum(ll[a:b])[-1]
        return out


# ---------------------------------------------------------------------------------------
# the kernels' fixed summation order, restated for the one family whose arithmetic numpy
# can reproduce exactly (y-only regression rows, sigma = 1: e = b0 - y, acc = fma(e, e, acc))
# ---------------------------------------------------------------------------------------
def tiles(n, tile=64, nslot=16):
    """dev.h nmc_tiles: [(start, rows)] of a group of n rows."""
    if n <= 0:
        return []
    t = min(-(-n // tile), nslot)
    per = (-(-n // t) + 15) & ~15
    return [(s, min(per, n - s)) for s in range(0, n, per)]


def _fma(a, b, c):
    from fractions import Fraction
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def linreg1_fixed_order(y, b0):
    """The group LL of rows {y} (intercept only, sigma = 1) for one chain, summed as
    nmc_ll_rows_lds, the 16-slot combine and FamLinreg::finish_fast sum it: per tile, an even
    number of 16-row blocks with row r into accumulator r & 3, the remaining rows into
    accumulator 0 in order, (a0 + a1) + (a2 + a3); tile k into slot accumulator k & 3 (unused
    slots -0.0), combined the same way; then -0.5 acc - n log sqrt(2 pi)."""
    n = len(y)
    if n == 0:
        return 0.0
    slots = [-0.0] * 16
    for k, (s, m) in enumerate(tiles(n)):
        a = [0.0] * 4
        paired = ((m // 16) & ~1) * 16
        for r in range(m):
            e = b0 - y[s + r]
            j = r & 3 if r < paired else 0
            a[j] = _fma(e, e, a[j])
        slots[k] = (a[0] + a[1]) + (a[2] + a[3])
    a4 = slots[:4]
    for u in range(4, 16):
        a4[u & 3] = a4[u & 3] + slots[u]
    acc = (a4[0] + a4[1]) + (a4[2] + a4[3])
    return -0.5 * (acc * 1.0) - float(n) * 0.9189385332046727


# ---------------------------------------------------------------------------------------
# helpers of the Gibbs geometry tests (tests/test_gpu_rowpaths.py, tests/test_gpu_gibbs_order.py)
# ---------------------------------------------------------------------------------------
@contextlib.contextmanager
def environ(env):
    """The environment variables ``env`` set while an Engine is created (NMC_* knobs)."""
    old = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update(env or {})
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k)
            else:
                os.environ[k] = v


GAUSS_SD = (0.8, 1.25, 0.6, 1.0, 0.9, 1.1, 0.7, 1.3, 0.85)


def gibbs_model(kind, G, sizes=None, intercept=True):
    """(family, sizes) of ``kind`` = "<family><n_fields>" over G groups: linreg (sigma = 1
    known), linregsig (sigma sampled), logistic, gauss.  sizes: the group sizes (default: 16
    to 32 rows, drawn); intercept: whether the design matrix of a regression or a logistic
    model leads with the ones column (the family then has one parameter more than stored
    covariates)."""
    r = numpy.random.RandomState(1000 + G)
    drawn = [int(s) for s in r.randint(16, 33, size=G)]
    sizes = drawn if sizes is None else [int(s) for s in sizes]
    assert len(sizes) == G
    n = sum(sizes)
    grp = numpy.repeat(numpy.arange(G), sizes)
    if kind == "linreg2" and intercept:
        x = r.normal(size=n)
        b0, b1 = r.normal(size=G), r.normal(2, 1, size=G)
        y = b0[grp] + b1[grp] * x + r.normal(size=n)
        return LinearRegression.simple(x, y, sigma=1.0), sizes
    name = kind.rstrip("0123456789")
    nf = int(kind[len(name):])
    if name == "gauss":
        return GaussianMean.from_groups(r.normal(size=(nf, G)), list(GAUSS_SD[:nf]), sizes), sizes
    assert name in ("linreg", "linregsig", "logistic") and (intercept or nf >= 2), kind
    X = numpy.hstack([numpy.ones((n, 1 if intercept else 0)), r.normal(size=(n, nf - 1))])
    th = r.normal(0, 0.5, size=(G, X.shape[1]))
    eta = numpy.sum(X * th[grp], axis=1)
    if name == "logistic":
        p = 1 / (1 + numpy.exp(-eta))
        return Logistic(X, (r.uniform(size=n) < p).astype(float)), sizes
    sig = 1.0 if name == "linreg" else 0.7
    return LinearRegression(X, eta + sig * r.normal(size=n),
                            sigma=1.0 if name == "linreg" else None), sizes


def gibbs_mode(fam, sizes):
    """The step kernel and mode choose_geometry picks for partial pooling over G small groups
    with rows in LDS: the register hand-off up to 64 groups, the Gibbs payload in LDS up to
    128 while two payload buffers of G + 1 columns fit the CU's 160 KiB beside the carve
    (P = 2: up to G = 120), nmc_k_run's all-wave update where they do not or where the
    groups are more than four numpy leaves, nmc_k_sweep between."""
    G, P = len(sizes), fam.n_params
    if 128 < G and len(pairwise_leaves(G)) <= 4:
        return "nmc_k_sweep<", ("NMC_MODE_SYNC_OWN",)
    nacc = fam.n_fields if isinstance(fam, GaussianMean) else 1
    doubles = max(sizes) * fam.n_fields
    cols = carve_columns(nacc, P, True, G) + 2 * (G + 1) + (doubles + 63) // 64 + 1
    if G <= 128 and cols * 512 <= 160 * 1024:
        return "nmc_k_run<", ("NMC_MODE_SYNC_REG" if G <= 64 else "NMC_MODE_SYNC_LDS",)
    return "nmc_k_run<", ("NMC_MODE_SYNC", "NMC_MODE_LAUNCH")


# ---------------------------------------------------------------------------------------
# the oracle-compared runs of the user-family tests, defined once: the GPU tests run them
# (tests/test_gpu_user_rowpaths.py) and the CPU tests check from the oracle's trace alone that
# they accept a fair share of their proposals and decide none by a near tie
# (tests/test_user_rowpath_cases.py)
# ---------------------------------------------------------------------------------------
USER_C = 65               # one full chain block and a partly filled second one
USER_GIBBS_G = (64, 65, 96, 100, 128, 129, 513)
Run = collections.namedtuple("Run", "fam sizes state sel n_iter seed base kw")


def oracle_sel(C=USER_C):
    return numpy.array([0, 1, C - 1])


def chain_run(name, C=USER_C):
    """test_chain_matches_oracle's run of a none-pooling case: a start near the posterior with
    proposal scales of 2.4 posterior sd, no stored LL (the reference's own start)."""
    from oracle import restatement as rs
    case, m = BY_NAME[name], model(name)
    value, lp, mu, s2, scale = start(name, C)
    assert case.pooling == "none"
    st = rs.State(value, lp, numpy.full((C, case.G), numpy.nan), mu, s2)
    kw = dict(pooling=case.pooling, priors=m.priors, tune_interval=3, scale=scale)
    return Run(m.fam, case.sizes, st, oracle_sel(C), case.step_iters, 77, 5, kw)


def gibbs_run(G, C=USER_C):
    """test_gibbs_geometry_edges' run for the four-parameter logistic over G small groups;
    every chain is compared."""
    from gpu_cases import partial_state
    fam, sizes = gibbs_model("logistic4", G)
    st, _ = partial_state(fam, sizes, C, fam.n_params)
    # (the Philox seed is chosen on the CPU: with seed 13 the oracle decides one of the 800 000
    # steps of the 513 groups by a margin of 7e-8)
    return Run(fam, sizes, st, numpy.arange(C), 10 if G <= 136 else 6, 14 if G == 513 else 13,
               2, dict(tune_interval=3))


def param_limit_run(P, C=USER_C):
    """A P-parameter polynomial (user_models.poly_family: two fields) over G = 8 groups of 20
    rows under partial pooling: the parameter limit of the workgroup state."""
    import user_models
    from gpu_cases import partial_state
    G, n = 8, 20
    r = numpy.random.RandomState(500 + P)
    x = r.uniform(-1, 1, size=G * n)
    c = r.normal(0, 0.5, size=(G, P))
    y = numpy.sum(c[numpy.repeat(numpy.arange(G), n)] * x[:, None] ** numpy.arange(P), axis=1)
    fam = user_models.poly_family(x, y + 0.5 * r.normal(size=G * n), P)
    st, _ = partial_state(fam, [n] * G, C, P, spread=0.3)
    return Run(fam, [n] * G, st, oracle_sel(C), 8, 21, 1, dict(tune_interval=3))


def run_oracle_of(run):
    """(flags, proposal LLs, rows, least decision margin) of the oracle on run.sel."""
    from gpu_cases import run_oracle
    return run_oracle(FastNested(run.fam, run.sizes), run.state, run.sel, run.sel + run.base,
                      run.n_iter, run.seed, **run.kw)
