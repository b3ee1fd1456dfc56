"""Sample stores written by the test, and the longdouble reference of their log-likelihoods
(tests/test_store_cases.py on the CPU, tests/test_gpu_store_cases.py on the device).

Everything computed after sampling reads the device sample store samples[row][col][C].
Engine.set_samples_raw writes it, so the store's consumers (obs_ll_rows and the LL files,
nmc_k_waic, nmc_k_loo_ll, nmc_k_conv) can be handed rows no sampler produces.  This module
needs numpy and scipy only: it imports no GPU code.

Geometry, one for every family: groups of 1, 7, 8, 9 and 17 observations (42 in all: runs of
T - 1, T, T + 1 and 2 T + 1 for NMC_WAIC_T = NMC_LOO_OT = 8, group boundaries inside an
8-observation walk at observations 1 and 8), C = 70 chains (a full chain block and one of 6
chains), R = 20 recorded rows (conv halves of n = 10 > NMC_CONV_L; the window (4, 12) gives
n = 6 < L), n_valid in {70, 65, 64} (64: the second block is padding only).

A case is a family, a pooling, a store [R][cols][C] and the n_valid values it is run with.
The parameter of (param q, group g) sits in column q (G + pc) + pc + g, pc = 2 hyper columns
under partial pooling (arbitrary finite values here: no consumer but nmc_k_conv reads them).
``bad`` lists the cells (row, chain, group, param, value) a non-finite case overwrites in its
``base`` case's store; a cell makes every observation of its group non-finite.

``ll_ref(name)`` evaluates the family's formula in numpy.longdouble on the float64 store:
(ll, A), each [C][R][n_obs].  A is ll with every addend replaced by its absolute value, the
scale of the per-row unit of DESIGN section 4 (as rowpath_cases.reference does for group
sums): for the regression the residual is taken as |b0| + sum |b_j x_j| + |y| before
squaring; for the logistic, with E = |b0| + sum |b_j x_j|, A = |y| E + logaddexp(0, E)
(the softplus has slope <= 1, so an error in eta passes into it at most as it is); log
sqrt(2 pi) and |log sigma| count once.  A sigma that is not positive gives NaN, as
scipy.stats.norm does, and a value beyond the float64 range is the infinity float64
arithmetic gives (a squared residual of 1e600 does not overflow a longdouble).
"""

import collections
import functools

import numpy

from nestmc.families import GaussianMean, LinearRegression, Logistic

LD = numpy.longdouble
U = 2.0 ** -53
T = 8                                  # csrc/waic.h NMC_WAIC_T, csrc/ll_kernels.h NMC_LOO_OT
SIZES = [1, T - 1, T, T + 1, 2 * T + 1]
G = len(SIZES)
N_OBS = sum(SIZES)
OFF = numpy.concatenate([[0], numpy.cumsum(SIZES)])
GRP = numpy.repeat(numpy.arange(G), SIZES)
C = 70
R = 20
N_VALID = (70, 65, 64)
DELTA = 60.0
F64_MAX = numpy.finfo(numpy.float64).max

Case = collections.namedtuple("Case", "name kind pooling fam priors P pc cols store n_valid "
                                      "base bad")
Bad = collections.namedtuple("Bad", "row chain group param value")


# ---------------------------------------------------------------------------------------
# data
# ---------------------------------------------------------------------------------------
def _linreg_data():
    r = numpy.random.RandomState(4201)
    x = r.normal(size=N_OBS)
    b0, b1 = r.normal(size=G), r.normal(2.0, 0.5, size=G)
    y = b0[GRP] + b1[GRP] * x + r.normal(size=N_OBS)
    ls = numpy.zeros((2, G))
    for g in range(G):
        xs, ys = x[OFF[g]:OFF[g + 1]], y[OFF[g]:OFF[g + 1]]
        if len(xs) < 2:
            ls[:, g] = ys[0] - 2.0 * xs[0], 2.0      # (one row: the line through it, slope 2)
        else:
            A = numpy.stack([numpy.ones_like(xs), xs], 1)
            ls[:, g] = numpy.linalg.lstsq(A, ys, rcond=None)[0]
    return x, y, ls


X_LIN, Y_LIN, LS = _linreg_data()


def _logistic_data():
    """Rows {x1, x2, x3, y}; every x a multiple of 1/4 in [-2, 2] and every theta of the store
    a multiple of 2^-6, so that every product and partial sum of eta is exact in float64 (the
    fused and the unfused dot product then agree bit for bit).  A group's first observation
    has x = 0: its eta is the intercept itself."""
    r = numpy.random.RandomState(4202)
    x = r.randint(-8, 9, size=(N_OBS, 3)) / 4.0
    x[OFF[:-1]] = 0.0
    y = (r.uniform(size=N_OBS) < 0.5).astype(float)
    y[OFF[:-1]] = [1.0, 0.0, 1.0, 0.0, 1.0]
    return x, y


X_LOG, Y_LOG = _logistic_data()
# the intercepts put into every seventh sample: softplus.h's clamp (|eta| > 746), its tail,
# eta == 0, and both sides of the e > 1/2 branch (|eta| around ln 2)
ETAS = [800.0, -800.0, 40.0, -40.0, 0.0, 0.5, -0.5, 0.75, -0.75]


def _gauss_data():
    r = numpy.random.RandomState(4203)
    mu = r.normal(size=(3, G))
    return mu[:, GRP].T + r.normal(size=(N_OBS, 3)), numpy.array([0.5, 1.0, 2.0])


M_GAUSS, SD_GAUSS = _gauss_data()


def col(q, g, pc):
    return q * (G + pc) + pc + g


def _store(P, pc, theta, seed):
    """theta [R][C][P][G] -> store [R][cols][C], hyper columns N(0, 1)."""
    st = numpy.random.RandomState(seed).normal(size=(R, P * (G + pc), C))
    for q in range(P):
        for g in range(G):
            st[:, col(q, g, pc), :] = theta[:, :, q, g]
    return numpy.ascontiguousarray(st)


def theta_of(case, store=None):
    """[R][C][P][G] of a case's store."""
    st = case.store if store is None else store
    th = numpy.empty((R, C, case.P, G))
    for q in range(case.P):
        for g in range(G):
            th[:, :, q, g] = st[:, col(q, g, case.pc), :]
    return th


def _linreg_case(name, delta, n_valid, y=None, slope_sd=0.0, seed=1):
    """delta [R][C]: the intercept of sample (row, chain) is the group's least-squares
    intercept plus delta."""
    r = numpy.random.RandomState(seed)
    th = numpy.empty((R, C, 2, G))
    th[:, :, 0, :] = LS[0][None, None, :] + numpy.asarray(delta, float)[:, :, None]
    th[:, :, 1, :] = LS[1][None, None, :] + slope_sd * r.normal(size=(R, C, G))
    fam = LinearRegression.simple(X_LIN, Y_LIN if y is None else y, sigma=1.0)
    return Case(name, "linreg", "partial", fam, None, 2, 2, 14, _store(2, 2, th, seed + 50),
                tuple(n_valid), None, ())


def ramp():
    """|delta| per row of ``ascending``: 60, 44, 20 (steps of more than 745 in the ll, so that
    exp(-|d|) underflows to 0 in the rescale), then 17 even steps down to 0."""
    return numpy.concatenate([[DELTA, 44.0, 20.0], numpy.linspace(18.0, 0.0, R - 3)])


def _bad_case(name, base, bad, n_valid):
    st = base.store.copy()
    for b in bad:
        st[b.row, col(b.param, b.group, base.pc), b.chain] = b.value
    return base._replace(name=name, store=st, n_valid=tuple(n_valid), base=base.name,
                         bad=tuple(bad))


def _cases():
    out = []
    r = numpy.random.RandomState(4210)
    sign = numpy.where(numpy.arange(C) % 2 == 0, 1.0, -1.0)
    out.append(_linreg_case("benign", 0.3 * r.normal(size=(R, C)), N_VALID, slope_sd=0.1))
    asc = ramp()[:, None] * sign[None, :]
    out.append(_linreg_case("ascending", asc, N_VALID))
    out.append(_linreg_case("descending", asc[::-1], N_VALID))
    for nv in N_VALID:
        d = numpy.full((R, C), DELTA)
        d[R - 1, nv - 1] = 0.0
        out.append(_linreg_case("late_max-%d" % nv, d, (nv,)))
    d = numpy.full((R, C), DELTA)
    d[:, 65:] = 0.0
    out.append(_linreg_case("pad_max", d, (65, 64)))
    out.append(_linreg_case("offset", 1e-3 * r.normal(size=(R, C)), N_VALID, y=Y_LIN + 1000.0))
    out.append(_linreg_case("ties", numpy.zeros((R, C)), N_VALID))

    # regression with sampled sigma, no pooling
    import scipy.stats
    th = numpy.empty((R, C, 3, G))
    th[:, :, :2, :] = LS[None, None] + 0.2 * r.normal(size=(R, C, 2, G))
    th[:, :, 2, :] = 0.7 + r.uniform(0, 0.5, size=(R, C, G))
    fam = LinearRegression.simple(X_LIN, Y_LIN)
    pri = [scipy.stats.norm(0, 10)] * 2 + [scipy.stats.gamma(2)]
    sig = Case("sigma", "regression", "none", fam, pri, 3, 0, 15, _store(3, 0, th, 61), N_VALID,
               None, ())
    out.append(sig)
    out.append(_bad_case("sigma_bad", sig, [
        Bad(2, 3, 0, 2, 0.0), Bad(5, 10, 1, 2, -1.0), Bad(7, 63, 2, 2, 1e-300),
        Bad(R - 1, 64, 3, 2, 1e300), Bad(0, 66, 4, 2, 0.0), Bad(R - 2, 0, 1, 2, 1e-300),
        Bad(3, 64, 2, 2, -1.0)], N_VALID))
    out.append(_bad_case("sigma_pad", sig, [
        Bad(3, 65, 0, 2, 0.0), Bad(4, 69, 2, 2, 1e-300), Bad(R - 1, 67, 4, 2, -1.0),
        Bad(0, 66, 3, 2, 1e300)], (65, 64)))

    # logistic, partial pooling, 4 fields
    th = numpy.round(r.normal(size=(R, C, 4, G)) * 64) / 64
    s = numpy.arange(R)[:, None] * C + numpy.arange(C)[None, :]
    for g in range(G):
        pick = s % 7 == g % 7
        th[:, :, 0, g] = numpy.where(pick, numpy.take(ETAS, (s // 7 + g) % len(ETAS)),
                                     th[:, :, 0, g])
    out.append(Case("logistic", "logistic", "partial",
                    Logistic(numpy.hstack([numpy.ones((N_OBS, 1)), X_LOG]), Y_LOG), None, 4, 2,
                    28, _store(4, 2, th, 62), N_VALID, None, ()))

    # Gaussian means, 3 fields, no pooling: theta at the data (a group's first row), near it,
    # and 1e8 away; the non-finite case puts cells 1e154 away on the field of sd 0.5, whose
    # squared deviation (2e154)^2 overflows
    first = M_GAUSS[OFF[:-1]].T                                   # [3][G]
    th = first[None, None] + 0.5 * r.normal(size=(R, C, 3, G))
    th[s % 3 == 0] = first
    far = s % 5 == 1
    th[far] = first + 1e8 * numpy.where(r.uniform(size=(int(far.sum()), 3, G)) < 0.5, -1.0, 1.0)
    gau = Case("gauss", "gauss", "none", GaussianMean(M_GAUSS, SD_GAUSS),
               [scipy.stats.norm(0, 10)] * 3, 3, 0, 15, _store(3, 0, th, 63), N_VALID, None, ())
    out.append(gau)
    out.append(_bad_case("gauss_inf", gau, [
        Bad(1, 2, 0, 0, first[0, 0] + 1e154), Bad(9, 63, 3, 0, first[0, 3] - 1e154),
        Bad(R - 1, 64, 4, 0, first[0, 4] + 1e154), Bad(6, 69, 1, 0, first[0, 1] - 1e154)],
        N_VALID))
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
NAMES = [c.name for c in CASES]
FINITE = [c.name for c in CASES if not c.bad]
NONFINITE = [c.name for c in CASES if c.bad]
SPREAD = ["ascending", "descending"] + ["late_max-%d" % nv for nv in N_VALID]


# ---------------------------------------------------------------------------------------
# the longdouble reference
# ---------------------------------------------------------------------------------------
PI_LD = 4 * numpy.arctan(LD(1))
LOG_C_LD = numpy.log(2 * PI_LD) / 2


def _to_f64_range(v):
    """Values beyond the float64 range as the infinities float64 arithmetic gives."""
    v = numpy.where(v > F64_MAX, LD(numpy.inf), v)
    return numpy.where(v < -F64_MAX, LD(-numpy.inf), v)


@functools.lru_cache(maxsize=None)
def ll_ref(name):
    """(ll, A), each [C][R][n_obs] in numpy.longdouble: the family's formula written out."""
    case = BY_NAME[name]
    th = numpy.transpose(theta_of(case), (1, 0, 2, 3)).astype(LD)[:, :, :, GRP]   # [C][R][P][n]
    obs = numpy.asarray(case.fam.obs()).astype(LD)
    with numpy.errstate(all="ignore"):
        if case.kind == "gauss":
            sd = SD_GAUSS.astype(LD)[None, None, :, None]
            e = (th - obs.T[None, None]) / sd
            sq = _to_f64_range(e * e)
            ll = (-sq / 2 - LOG_C_LD - numpy.log(sd)).sum(axis=2)
            A = (sq / 2 + LOG_C_LD + numpy.abs(numpy.log(sd))).sum(axis=2)
        else:
            K = case.fam.n_fields - 1
            x, y = obs[:, :K].T, obs[:, K]
            b0, b = th[:, :, 0], th[:, :, 1:1 + K]
            eta = b0 + (b * x[None, None]).sum(axis=2)
            E = numpy.abs(b0) + (numpy.abs(b) * numpy.abs(x)[None, None]).sum(axis=2)
            if case.kind == "logistic":
                ll = y * eta - numpy.logaddexp(LD(0), eta)
                A = numpy.abs(y) * E + numpy.logaddexp(LD(0), E)
            else:
                sig = th[:, :, K + 1] if case.P == K + 2 else numpy.ones_like(eta)
                ok = sig > 0
                sg = numpy.where(ok, sig, LD(1))
                t = (eta - y) / sg
                sq = _to_f64_range(t * t)
                ll = numpy.where(ok, -sq / 2 - LOG_C_LD - numpy.log(sg), LD(numpy.nan))
                ra = (E + numpy.abs(y)) / sg
                A = numpy.where(ok, _to_f64_range(ra * ra) / 2 + LOG_C_LD
                                + numpy.abs(numpy.log(sg)), LD(numpy.nan))
    ll.setflags(write=False)
    A.setflags(write=False)
    return ll, A


def obs_ll_units(nf):
    """The per-row evaluation unit of DESIGN section 4 in units of 2^-53 A: 4 (nf + 4).  The
    logistic's softplus is within 2.5 ulp = 5 of these units of a value that is one addend of
    A (softplus.h), inside 4 (nf + 4) >= 20 with the dot product's nf + 1 roundings."""
    return 4 * (nf + 4)


def nonfinite_per_obs(case, row_begin=0, n_rows=R, n_valid=C):
    """From the construction: per observation, the bad cells of its group with a value that
    makes the term NaN or -inf (a sigma of 1e300 does not), inside the window and below
    n_valid."""
    out = numpy.zeros(N_OBS, dtype=numpy.int64)
    for b in case.bad:
        breaks = (abs(b.value) > 1e100) if case.kind == "gauss" else \
            (not b.value > 0 or b.value < 1e-200)
        if breaks and row_begin <= b.row < row_begin + n_rows and b.chain < n_valid:
            out[OFF[b.group]:OFF[b.group + 1]] += 1
    return out


def touched_groups(case, row_begin=0, n_rows=R, n_valid=C):
    """The groups with an overwritten cell (finite or not) the window and n_valid can see."""
    return sorted({b.group for b in case.bad
                   if row_begin <= b.row < row_begin + n_rows and b.chain < n_valid})


def matrix(ll, row_begin=0, n_rows=R, n_valid=C):
    """[C][R][n_obs] -> [S][n_obs] of the window's samples, chain-major as waic_ref takes it."""
    a = numpy.asarray(ll)[:n_valid, row_begin:row_begin + n_rows]
    return a.reshape(-1, a.shape[-1])


# ---------------------------------------------------------------------------------------
# nmc_k_conv's columns (family-independent): the store of the linreg engine, cols = 14
# ---------------------------------------------------------------------------------------
CONV_COLUMNS = ["normal", "1e8+1e-3 normal", "constant 0.1", "+-0.0", "denormals", "+-1e300",
                "one +inf", "one NaN", "clean normal", "normal", "normal", "normal", "normal",
                "normal"]
CONV_FLAGGED = (5, 6, 7)      # columns whose results are not finite
CONV_CLEAN = 8
CONV_INF_AT = (13, 66)        # (row, chain) of the +inf: second half, second chain block
CONV_NAN_AT = (5, 3)
CONV_WINDOWS = ((0, 20), (4, 12), (16, 4))


@functools.lru_cache(maxsize=None)
def conv_store(replaced=False):
    """[R][14][C]; replaced: the flagged columns hold N(0, 1) instead."""
    r = numpy.random.RandomState(4220)
    st = r.normal(size=(R, 14, C))
    if not replaced:
        st[:, 1] = 1e8 + 1e-3 * r.normal(size=(R, C))
        st[:, 2] = 0.1
        st[:, 3] = numpy.where(r.uniform(size=(R, C)) < 0.5, -0.0, 0.0)
        st[:, 4] = r.randint(-40, 41, size=(R, C)) * 5e-324
        st[:, 5] = numpy.where(r.uniform(size=(R, C)) < 0.5, -1e300, 1e300)
        st[CONV_INF_AT[0], 6, CONV_INF_AT[1]] = numpy.inf
        st[CONV_NAN_AT[0], 7, CONV_NAN_AT[1]] = numpy.nan
    else:
        keep = conv_store(False)
        for k in range(14):
            if k not in CONV_FLAGGED:
                st[:, k] = keep[:, k]
    st = numpy.ascontiguousarray(st)
    st.setflags(write=False)
    return st


def conv_rows(store, row_begin, n_rows):
    """A store window as convergence_ref takes it: [C][rows][cols]."""
    return numpy.ascontiguousarray(numpy.transpose(store[row_begin:row_begin + n_rows],
                                                   (2, 0, 1)))
