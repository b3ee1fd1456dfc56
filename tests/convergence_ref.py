"""The float64 restatement of nmc_k_conv's fixed order (csrc/conv.h), the longdouble formulas
and the bounds of the convergence tests.

Restatement (``partials``), per column k, chain c, half h, x the n values of the half:
  mean = (x[0] + x[1] + ... + x[n-1]) / n      sequential (cumsum), one division
  M2   = sum_q d d, d = x[q] - mean            sequential (cumsum), d * d, never ** 2
  S[t] = sum_{q < n-t} d d, d = x[q+t] - x[q]  sequential (cumsum); S[0] = 0
  vg[cb][k][t]: the 128 leaves (chain, half), half minor, of chain block cb (chains
  >= n_valid and beyond C as +0.0), v = v[0::2] + v[1::2] seven times.

Bounds, u = 2^-53 (the unit roundoff of float64; every bound below is first order in u with
the (1 + O(k u)) factor absorbed by the slack named):

V_t.  All addends d d are >= 0, so every partial sum is bounded by the exact total and an
  addition chain of depth D loses at most D u relative to the total.  Restatement: a square
  is 2 roundings (the difference, the product: 3 u), the sequential sum over q at most n - 1
  additions, the tree 7 levels, the host merge of CB blocks CB - 1 additions, the division by
  m (n - t) one rounding: (n + CB + 10) u.  The sequential-j host route (nmc_variogram /
  variogram_host): 3 u, n - 1 additions over q, m - 1 over j, one division: (n + m + 3) u.
  The squares and the sums over q are the same operations on the same numbers in both routes
  -- the per-half-chain S[t] agree bit for bit -- so the two differ only in how the m values
  S_j[t] are added: the tree and the block merge (7 + CB - 1 levels) against the sequential
  chain (m - 1), each with the division: |V_gpu - V_host| <= (m + CB + 8) u V_t, stated as
    TOL_V = (m + CB + 16) u V_t.
mean of a half-chain.  Sequential sum of n terms and a division: |err| <= n u sum_q |x[q]| / n
  = n u mean|x|.   TOL_MEAN = n u mean_q |x[q]|  (numpy's pairwise mean is within the same).
M2.  With the mean exact: 3 u per square, n - 1 additions: (n + 2) u M2; (n + 4) u with the
  rounding of the subtraction's operand.  An error e in the mean changes M2 by n e^2 exactly
  (sum_q (x[q] - mean) = 0 to first order, the cross term 2 e sum d_q vanishes up to
  2 |e| n u mean|x|): the second-order term.
    TOL_M2 = (n + 4) u M2 + n e^2 + 2 e n u mean|x|,  e = TOL_MEAN.
Derived quantities (``tolerances``): W is a mean of m values M2 / (n - 1), B = n var of the
  m half-chain means, whose error is bounded through |d var| <= 2 sqrt(var) e sqrt(m/(m-1))
  + e^2 m/(m-1); vhat, rhat, sd and rho follow by the triangle inequality, neff through
  d neff = neff^2 / (m n) 2 sum_t |d rho_t| as long as both routes cut at the same T (the host
  test checks that they do on the inputs used).  TOL_V bounds the difference of the two
  routes directly; the derived bounds hold for each route against the exact value, so the
  routes are within twice of each other.
"""

import numpy

U = 2.0 ** -53


def halves(rows):
    """rows [C][2n][cols] -> x [cols][C][2][n]."""
    rows = numpy.asarray(rows, dtype=numpy.float64)
    C, R, K = rows.shape
    assert R % 2 == 0
    return numpy.ascontiguousarray(numpy.transpose(rows.reshape(C, 2, R // 2, K), (3, 0, 1, 2)))


def moments(x):
    """x [..., n] -> (mean, M2, S[..., n]) in the fixed order."""
    n = x.shape[-1]
    mean = numpy.cumsum(x, axis=-1)[..., -1] / float(n)
    d = x - mean[..., None]
    M2 = numpy.cumsum(d * d, axis=-1)[..., -1]
    S = numpy.zeros(x.shape)
    for t in range(1, n):
        d = x[..., t:] - x[..., :n - t]
        S[..., t] = numpy.cumsum(d * d, axis=-1)[..., -1]
    return mean, M2, S


def partials(rows, n_valid=None):
    """The restatement of Engine.conv_partials over rows [C][2n][cols] (chain-major, as
    Engine.samples() gives them): (vg [CB, cols, n], mean [cols, 2, C], m2 [cols, 2, C]).
    Chains >= n_valid enter vg as +0.0 and have mean = m2 = +0.0."""
    x = halves(rows)                                   # [K][C][2][n]
    K, C, _, n = x.shape
    nv = C if n_valid is None else n_valid
    mean, M2, S = moments(x)
    mean[:, nv:] = 0.0
    M2[:, nv:] = 0.0
    S[:, nv:] = 0.0
    CB = (C + 63) // 64
    leaves = numpy.zeros((K, CB * 64, 2, n))
    leaves[:, :C] = S
    v = leaves.reshape(K, CB, 128, n)
    for _ in range(7):
        v = v[:, :, 0::2] + v[:, :, 1::2]
    vg = numpy.ascontiguousarray(numpy.transpose(v[:, :, 0], (1, 0, 2)))
    return vg, numpy.ascontiguousarray(numpy.transpose(mean, (0, 2, 1))), \
        numpy.ascontiguousarray(numpy.transpose(M2, (0, 2, 1)))


def longdouble_formulas(x):
    """x [K][m][n] -> dict of the formulas in numpy.longdouble (mean_j, M2_j, V, W, B, vhat,
    rhat, sd, mean, rho)."""
    X = numpy.asarray(x, dtype=numpy.float64).astype(numpy.longdouble)
    K, m, n = X.shape
    mean_j = numpy.sum(X, axis=2) / n
    d = X - mean_j[:, :, None]
    M2_j = numpy.sum(d * d, axis=2)
    V = numpy.zeros((K, n), dtype=numpy.longdouble)
    for t in range(1, n):
        d = X[:, :, t:] - X[:, :, :n - t]
        V[:, t] = numpy.sum(d * d, axis=(1, 2)) / (numpy.longdouble(m) * (n - t))
    gm = numpy.sum(mean_j, axis=1) / m
    dm = mean_j - gm[:, None]
    B = n * numpy.sum(dm * dm, axis=1) / (m - 1)
    W = numpy.sum(M2_j / (n - 1), axis=1) / m
    vhat = W * (n - 1) / n + B / n
    return dict(mean_j=mean_j, M2_j=M2_j, V=V, B=B, W=W, vhat=vhat, rhat=numpy.sqrt(vhat / W),
                sd=numpy.sqrt(vhat), mean=gm, rho=1 - V / (2 * vhat[:, None]),
                absmean_j=numpy.sum(numpy.abs(X), axis=2) / n)


def tol_v(V, m, CB):
    return (m + CB + 16) * U * numpy.abs(V)


def tol_v_exact(V, n, CB):
    """The restatement (or the device) against the exact V_t: (n + CB + 10) u V_t."""
    return (n + CB + 10) * U * numpy.abs(V)


def tol_mean(absmean_j, n):
    return n * U * absmean_j


def tol_m2(M2_j, absmean_j, n):
    e = tol_mean(absmean_j, n)
    return (n + 4) * U * M2_j + n * e * e + 2 * e * n * U * absmean_j


def tolerances(x, CB):
    """Bounds on |device route - host route| for the finished quantities of x [K][m][n]:
    dict(V, mean, sd, rhat, neff_rel(T, neff), f = the longdouble formulas)."""
    f = longdouble_formulas(x)
    K, m, n = numpy.asarray(x).shape
    e_mean = tol_mean(f["absmean_j"], n)                      # [K][m]
    e_m2 = tol_m2(f["M2_j"], f["absmean_j"], n)
    eW = numpy.sum(e_m2, axis=1) / (m * (n - 1)) + (m + 2) * U * f["W"]
    em = numpy.max(e_mean, axis=1)
    varm = f["B"] / n
    r = numpy.longdouble(m) / (m - 1)
    eB = n * (2 * numpy.sqrt(varm * r) * em + em * em * r + (m + 4) * U * varm)
    evhat = eW + eB / n + 4 * U * f["vhat"]
    esd = evhat / (2 * f["sd"]) + U * f["sd"]
    erhat = f["rhat"] * (evhat / f["vhat"] + eW / f["W"]) / 2 + 2 * U * f["rhat"]
    eV = tol_v(f["V"], m, CB)
    # rho = 1 - V / (2 vhat): d rho = dV / (2 vhat) + V dvhat / (2 vhat^2) + 3 u (1 + |rho|)
    erho = eV / (2 * f["vhat"][:, None]) + f["V"] * (evhat / (2 * f["vhat"] ** 2))[:, None] \
        + 3 * U * (1 + numpy.abs(f["rho"]))
    emean = em + (m + 1) * U * numpy.abs(f["mean"]) + (m + 1) * U * numpy.max(f["absmean_j"], axis=1)

    def neff_rel(T, neff):
        """relative bound on neff given the cutoffs T [K] and neff [K]."""
        out = numpy.empty(K)
        for k in range(K):
            s = numpy.sum(erho[k, :T[k] + 1]) + (T[k] + 4) * U * numpy.sum(
                numpy.abs(f["rho"][k, :T[k] + 1]))
            out[k] = float(2 * s * abs(neff[k]) / (m * n) + 4 * U)
        return out
    two = 2.0
    return dict(V=eV, mean=two * emean, sd=two * esd, rhat=two * erhat,
                neff_rel=lambda T, neff: two * neff_rel(T, neff), f=f)
