"""The restatement and the bounds of the rank-diagnostics tests (nestmc/rankdiag.py has the
definitions; csrc/rankz.h the kernel).

Exact quantities (``derive``): twice_rank = searchsorted left + right + 1 of x among the x and
of zeta = |x - med| among the zeta, zeta itself (nmc_rank_partials_of hands it out as pass 1
wrote it, before pass 2 overwrites it with zf), I05 and I95 from the integer order statistics,
the nonfinite counts -- compared with the device as words, no tolerance.

The normal score (``ndtri_as241``): the float64 restatement of nmc_ndtri, Wichura's AS 241
PPND16 with every operation rounded on its own, Horner from the highest coefficient, and
numpy's log and sqrt where the device has its own.  The exact score (``ratio_to_exact``) is
mpmath's sqrt(2) erfinv(2 p - 1) at 50 digits, at the same float64 p.  Over the p of every
test shape (``probe_p``: both ends, the N/2 region and an even sample of the ranks and half
ranks of N = 4, 6, 16, 18, 34, 4094, 4096, 4098, 8194, 6000, 7000, 33 282) the restatement's
worst |err| / (u |z|) measured 5.35 (u = 2^-53; at p = 0.9908, and 5.33 / 5.11 in the lower
tail and the centre), scipy.special.ndtri's 5.22; the convention of psis_ref.py -- the least
power of two >= 8 x the measured ratio, 42.8 -- gives
    NDTRI_C = 64:   |z_device - z_exact| <= 64 u |z|,   z = 0 exact at p = 1/2
and the CPU test re-measures both (the restatement and scipy each within NDTRI_C / 8 = 8).
The device differs from the restatement only in log and sqrt (each within 1 ulp of its exact
value: a relative change of at most about 1.5 u in r = sqrt(-log p), which the tails'
rational functions pass on with a factor |r z'(r) / z| < 2): the factor 8 covers it.  The GPU
test compares the probes with mpmath within NDTRI_C u |z| and EVERY element with the
restatement within (NDTRI_C - NDTRI_C / 8) u |z|, which with the restatement's own NDTRI_C / 8
is the same bound against the exact score.

Finished numbers, device route against host route (``tolerances_z``): the first-order effect
of a relative data error EPS = NDTRI_C u.  Datum q of one route is the other's times
(1 + e_q); the device is within NDTRI_C / 8 u (restatement) plus its log and sqrt of the exact
score and scipy within NDTRI_C / 8 u, so |e_q| <= EPS with room.  Per half-chain x of n values,
d = x - mean:
  mean   |d mean| <= EPS mean_q |x_q|
  M2     = sum d_q^2: d M2 = 2 sum d_q (dx_q - d mean) and sum d_q = 0, so
         |d M2| <= 2 EPS sum_q |d_q| |x_q|
  S_t    = sum_q (x_{q+t} - x_q)^2: |d S_t| <= 2 EPS sum_q |x_{q+t} - x_q| (|x_{q+t}| + |x_q|)
         and V_t = sum_j S_t / (m (n - t)) inherits the sum over the half-chains j.
These are added to convergence_ref's rounding bounds TOL_MEAN, TOL_M2 and TOL_V, and the
derived bounds (W, B, vhat, rhat, rho, and the ESS through d ess / ess = 2 sum_t |d rho_t|
ess / N while both routes cut at the same T) follow as in convergence_ref.tolerances, with its
factors (V as it is, the derived ones doubled), restated here because that file stays as it
is.  The indicators I05 and I95 are exact data: convergence_ref.tolerances applies to them as
it stands.
"""

import functools

import numpy

import convergence_ref as cr

U = cr.U
NDTRI_C = 64.0
EPS = NDTRI_C * U

# (rows, C, n_valid) of the exact tests; N = rows * n_valid
SHAPES = [(r, 1, 1) for r in (4, 6, 16, 18, 34, 4094, 4096, 4098, 8194)] + \
    [(100, 70, 70), (100, 70, 60), (258, 130, 129)]


# ---- the normal score ----------------------------------------------------------------------
_A = (2509.0809287301226727, 33430.575583588128105, 67265.770927008700853,
      45921.953931549871457, 13731.693765509461125, 1971.5909503065514427,
      133.14166789178437745, 3.387132872796366608)
_B = (5226.495278852545925, 28729.085735721942674, 39307.89580009271061,
      21213.794301586595867, 5394.1960214247511077, 687.1870074920579083,
      42.313330701600911252, 1.0)
_C = (7.7454501427834140764e-4, 0.0227238449892691845833, 0.24178072517745061177,
      1.27045825245236838258, 3.64784832476320460504, 5.7694972214606914055,
      4.6303378461565452959, 1.42343711074968357734)
_D = (1.05075007164441684324e-9, 5.475938084995344946e-4, 0.0151986665636164571966,
      0.14810397642748007459, 0.68976733498510000455, 1.6763848301838038494,
      2.05319162663775882187, 1.0)
_E = (2.01033439929228813265e-7, 2.71155556874348757815e-5, 0.0012426609473880784386,
      0.026532189526576123093, 0.29656057182850489123, 1.7848265399172913358,
      5.4637849111641143699, 6.6579046435011037772)
_F = (2.04426310338993978564e-15, 1.4215117583164458887e-7, 1.8463183175100546818e-5,
      7.868691311456132591e-4, 0.0148753612908506148525, 0.13692988092273580531,
      0.59983224388101963777, 1.0)


def _horner(c, r):
    v = c[0] * r + c[1]
    for a in c[2:]:
        v = v * r + a
    return v


def ndtri_as241(p):
    """nmc_ndtri in float64 numpy, for 0 < p < 1."""
    p = numpy.asarray(p, dtype=numpy.float64)
    q = p - 0.5
    out = numpy.empty(p.shape)
    mid = numpy.abs(q) <= 0.425
    r = 0.180625 - q[mid] * q[mid]
    out[mid] = q[mid] * _horner(_A, r) / _horner(_B, r)
    t = ~mid
    r = numpy.sqrt(-numpy.log(numpy.where(q[t] < 0.0, p[t], 1.0 - p[t])))
    near = r <= 5.0
    v = numpy.empty(r.shape)
    rn = r[near] - 1.6
    v[near] = _horner(_C, rn) / _horner(_D, rn)
    rf = r[~near] - 5.0
    v[~near] = _horner(_E, rf) / _horner(_F, rf)
    out[t] = numpy.where(q[t] < 0.0, -v, v)
    return out


@functools.lru_cache(maxsize=None)
def _exact(p):
    import mpmath
    with mpmath.workdps(50):
        return mpmath.sqrt(2) * mpmath.erfinv(2 * mpmath.mpf(p) - 1)


def ratio_to_exact(z, p):
    """|z - exact(p)| / (u |exact|) per element (0 where both are 0; inf where only the
    exact one is), the exact score by mpmath at 50 digits."""
    import mpmath
    out = numpy.empty(len(p))
    with mpmath.workdps(50):
        for i, (zi, pi) in enumerate(zip(numpy.asarray(z).tolist(), numpy.asarray(p).tolist())):
            e = _exact(pi)
            if e == 0:
                out[i] = 0.0 if zi == 0.0 else numpy.inf
            else:
                out[i] = float(abs((mpmath.mpf(zi) - e) / e) / mpmath.mpf(U))
    return out


def p_of(r2, N):
    """p of twice the average rank: one float64 division of two exact numbers."""
    return (numpy.asarray(r2, dtype=numpy.float64) * 0.5 - 0.375) / (float(N) + 0.25)


def probe_r2(N):
    """The twice-ranks probed against mpmath for a column of N values: every one in [2, 2 N]
    for N <= 512, else both ends, the N/2 region and an even sample."""
    if N <= 512:
        return numpy.arange(2, 2 * N + 1)
    return numpy.unique(numpy.concatenate([
        numpy.arange(2, 130), numpy.arange(2 * N - 127, 2 * N + 1),
        numpy.arange(N + 1 - 128, N + 1 + 129), numpy.arange(2, 2 * N + 1, (2 * N) // 509)]))


def probe_p():
    """The p of every test shape's probes."""
    return numpy.concatenate([p_of(probe_r2(r * nv), r * nv) for r, _, nv in SHAPES])


# ---- the exact quantities ------------------------------------------------------------------
def twice_rank(x):
    s = numpy.sort(x)
    lo = numpy.searchsorted(s, x, side="left").astype(numpy.int64)
    return lo + numpy.searchsorted(s, x, side="right") + 1, lo


def derive(xs, n_valid):
    """xs [rows][cols][C] (store layout), chains [0, n_valid) real -> dict of twice_rank
    [2][rows][cols][C] (0 for padding chains and nonfinite columns), zeta, I05, I95
    [rows][cols][C] (+0.0 for padding chains, NaN for nonfinite columns), p and pf (the normal
    scores' arguments) and nonfinite [cols]."""
    xs = numpy.asarray(xs, dtype=numpy.float64)
    R, K, C = xs.shape
    N = R * n_valid
    k05, k95 = (N - 1) // 20, 19 * (N - 1) // 20
    tr = numpy.zeros((2, R, K, C), dtype=numpy.int64)
    ind = numpy.zeros((2, R, K, C))
    zt = numpy.zeros((R, K, C))
    p = numpy.full((2, R, K, C), numpy.nan)
    bad = numpy.zeros(K, dtype=numpy.int64)
    for k in range(K):
        x = xs[:, k, :n_valid].reshape(N)
        bad[k] = numpy.sum(~numpy.isfinite(x))
        if bad[k]:
            ind[:, :, k, :n_valid] = numpy.nan
            zt[:, k, :n_valid] = numpy.nan
            continue
        r2, lo = twice_rank(x)
        s = numpy.sort(x)
        with numpy.errstate(over="ignore"):
            zeta = numpy.abs(x - (s[N // 2 - 1] + s[N // 2]) / 2.0)
        r2f, _ = twice_rank(zeta)
        zt[:, k, :n_valid] = zeta.reshape(R, n_valid)
        tr[0, :, k, :n_valid] = r2.reshape(R, n_valid)
        tr[1, :, k, :n_valid] = r2f.reshape(R, n_valid)
        ind[0, :, k, :n_valid] = (lo <= k05).reshape(R, n_valid)
        ind[1, :, k, :n_valid] = (lo <= k95).reshape(R, n_valid)
        p[0, :, k, :n_valid] = p_of(r2, N).reshape(R, n_valid)
        p[1, :, k, :n_valid] = p_of(r2f, N).reshape(R, n_valid)
    return dict(twice_rank=tr, zeta=zt, I05=ind[0], I95=ind[1], p=p[0], pf=p[1], nonfinite=bad)


def columns(rows, nv, seed):
    """The test columns as a [rows][n_valid][K] array: normal draws; draws rounded to one
    decimal (long tie runs); all equal; ascending; descending; a mix of -0.0 and +0.0 among
    draws; the two largest magnitudes with a median whose distance to them overflows; a
    symmetric column (every zeta tied in pairs); one NaN; one infinity."""
    r = numpy.random.RandomState(seed)
    N = rows * nv
    g = r.normal(size=N)
    big = 1.7976931348623157e308
    zeros = numpy.where(r.uniform(size=N) < 0.5, -0.0, 0.0)
    zeros = numpy.where(r.uniform(size=N) < 0.3, r.normal(size=N), zeros)
    over = numpy.full(N, -0.8e308)
    over[r.permutation(N)[:max(1, N // 5)]] = big
    over[r.permutation(N)[:max(1, N // 5)]] = -big
    over = numpy.where(r.uniform(size=N) < 0.1, r.normal(size=N), over)
    half = r.normal(size=N // 2)
    sym = r.permutation(numpy.concatenate([half, -half, numpy.zeros(N - 2 * (N // 2))]))
    nan = g.copy()
    nan[N // 3] = numpy.nan
    inf = g.copy()
    inf[N // 2] = -numpy.inf
    cols = [g, numpy.round(r.normal(size=N), 1), numpy.full(N, 2.5), numpy.arange(N) * 0.25,
            -numpy.arange(N) * 0.5, zeros, over, sym, nan, inf]
    return numpy.stack(cols, axis=1).reshape(rows, nv, len(cols))


def store(rows, C, nv, seed):
    """columns() in store layout [rows][K][C]; the padding chains hold a NaN that nothing may
    read."""
    c = columns(rows, nv, seed)
    xs = numpy.full((rows, c.shape[2], C), numpy.nan)
    xs[:, :, :nv] = numpy.transpose(c, (0, 2, 1))
    return xs


# ---- the bounds of the finished numbers ----------------------------------------------------
def tolerances_z(x, CB, eps=EPS):
    """convergence_ref.tolerances with the first-order effect of a relative data error eps
    added to the bounds of the mean, M2 and V_t (the docstring has the derivation):
    dict(V, rhat, ess_rel(T, ess), f)."""
    f = cr.longdouble_formulas(x)
    X = numpy.asarray(x, dtype=numpy.float64).astype(numpy.longdouble)
    K, m, n = X.shape
    aX = numpy.abs(X)
    d = X - f["mean_j"][:, :, None]
    e_mean = cr.tol_mean(f["absmean_j"], n) + eps * f["absmean_j"]
    e_m2 = cr.tol_m2(f["M2_j"], f["absmean_j"], n) + 2 * eps * numpy.sum(numpy.abs(d) * aX, axis=2)
    eV = cr.tol_v(f["V"], m, CB)
    for t in range(1, n):
        dd = numpy.abs(X[:, :, t:] - X[:, :, :n - t]) * (aX[:, :, t:] + aX[:, :, :n - t])
        eV[:, t] = eV[:, t] + 2 * eps * numpy.sum(dd, axis=(1, 2)) / (numpy.longdouble(m) * (n - t))
    eW = numpy.sum(e_m2, axis=1) / (m * (n - 1)) + (m + 2) * U * f["W"]
    em = numpy.max(e_mean, axis=1)
    varm = f["B"] / n
    r = numpy.longdouble(m) / (m - 1)
    eB = n * (2 * numpy.sqrt(varm * r) * em + em * em * r + (m + 4) * U * varm)
    evhat = eW + eB / n + 4 * U * f["vhat"]
    erhat = f["rhat"] * (evhat / f["vhat"] + eW / f["W"]) / 2 + 2 * U * f["rhat"]
    erho = eV / (2 * f["vhat"][:, None]) + f["V"] * (evhat / (2 * f["vhat"] ** 2))[:, None] \
        + 3 * U * (1 + numpy.abs(f["rho"]))

    def ess_rel(T, ess):
        out = numpy.empty(K)
        for k in range(K):
            s = numpy.sum(erho[k, 1:T[k] + 1]) + (T[k] + 4) * U * numpy.sum(
                numpy.abs(f["rho"][k, 1:T[k] + 1]))
            out[k] = float(2 * s * abs(ess[k]) / (m * n) + 4 * U)
        return 2.0 * out
    return dict(V=eV, rhat=2.0 * erhat, ess_rel=ess_rel, f=f)


def cutoffs_longdouble(x):
    """The cutoff lag T per column by the longdouble formulas (the loop of _assess)."""
    f = cr.longdouble_formulas(x)
    K, m, n = numpy.asarray(x).shape
    T = numpy.empty(K, dtype=numpy.int64)
    for k in range(K):
        r = f["rho"][k]
        hit = numpy.nonzero((r[1:n - 1] + r[2:n] < 0) & (numpy.arange(n - 2) % 2 == 0))[0]
        T[k] = int(hit[0]) if hit.size else n - 1
    return T
