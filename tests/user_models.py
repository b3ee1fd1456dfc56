"""Device log-likelihood sources for the user-family tests (DeviceLikelihood)."""

import numpy
import scipy.special



def logistic_source(k):
    """FamLogistic's own expression (csrc/families.h) as a user function, rows
    [x_1..x_k, y], theta [b0, b1..bk]: eta = b0 + fma chain; ll = y eta - logaddexp(0, eta)
    (nmc_logaddexp0, the library's numpy.logaddexp restatement)."""
    return r"""
__device__ double nmc_user_loglik(const double* th, const double* row, const double* k) {
  double eta = th[0];
  for (int j = 0; j < %d; ++j) eta = fma(row[j], th[j + 1], eta);
  return row[%d] * eta - nmc_logaddexp0(eta);
}
""" % (k, k)


LOGISTIC4 = logistic_source(3)
LOGISTIC8 = logistic_source(7)

# A model no built-in family covers: Poisson regression with a log link and an exposure
# constant, rows [x, y, lgamma(y + 1)] (the data-only term precomputed per row), theta
# [a, b], k = {log exposure}:  ll = y eta - exp(eta) - lgamma(y + 1),  eta = a + b x + k[0]
POISSON = r"""
__device__ double nmc_user_loglik(const double* th, const double* row, const double* k) {
  const double eta = th[0] + th[1] * row[0] + k[0];
  return row[1] * eta - exp(eta) - row[2];
}
"""


def poisson_rows(x, y):
    return numpy.stack([x, y, scipy.special.gammaln(y + 1.0)], 1)


def poisson_host(x, y, log_exposure):
    """The same model in the reference's calling convention (parameter[P][n] -> ll[n])."""
    lgy = scipy.special.gammaln(y + 1.0)

    def f(parameter):
        eta = numpy.asarray(parameter[0]) + numpy.asarray(parameter[1]) * x + log_exposure
        return y * eta - numpy.exp(eta) - lgy
    return f


def poisson_data(G, N, seed=2):
    r = numpy.random.RandomState(seed)
    x = r.normal(size=G * N)
    a = r.normal(0.5, 0.3, size=G)
    b = r.normal(0.3, 0.2, size=G)
    g = numpy.repeat(numpy.arange(G), N)
    y = r.poisson(numpy.exp(a[g] + b[g] * x + 0.1)).astype(float)
    return x, y


# ---------------------------------------------------------------------------------------
# rows wider than any built-in family (tests/test_gpu_user_rowpaths.py)
# ---------------------------------------------------------------------------------------
def wide_weights(nf):
    """The constants of wide_source: w_j = (-1)^(j+1) / (j + 1), j = 1..nf-1 -- distinct in
    magnitude and alternating in sign, so a dropped, shifted or repeated field changes s."""
    j = numpy.arange(1, nf)
    return numpy.where(j % 2 == 1, 1.0, -1.0) / (j + 1.0)


def wide_source(nf):
    """Rows [x_1..x_{nf-1}, y], theta [a, b], k = w_1..w_{nf-1}: s an fma chain of w_j x_j in
    field order, eta = a + b s, ll = -0.5 (y - eta)^2."""
    return r"""
__device__ double nmc_user_loglik(const double* th, const double* row, const double* k) {
  double s = 0.0;
  for (int j = 0; j < %d; ++j) s = fma(k[j], row[j], s);
  const double e = row[%d] - (th[0] + th[1] * s);
  return -0.5 * (e * e);
}
""" % (nf - 1, nf - 1)


def wide_host(rows):
    """wide_source in the reference's calling convention (parameter[2][n] -> ll[n])."""
    rows = numpy.asarray(rows, float)
    nf = rows.shape[1]
    w, y = wide_weights(nf), rows[:, nf - 1]

    def f(parameter):
        s = numpy.zeros(rows.shape[0])
        for j in range(nf - 1):
            s = s + w[j] * rows[:, j]
        e = y - (numpy.asarray(parameter[0]) + numpy.asarray(parameter[1]) * s)
        return -0.5 * (e * e)
    return f


def coef_source(nf):
    """Rows [x_1..x_{nf-1}, y], theta [b_0..b_{nf-1}] (P = nf, up to the library's 16):
    eta = b_0 + fma chain of x_j b_j, ll = -0.5 (y - eta)^2."""
    return r"""
__device__ double nmc_user_loglik(const double* th, const double* row, const double* k) {
  double eta = th[0];
  for (int j = 0; j < %d; ++j) eta = fma(row[j], th[j + 1], eta);
  const double e = row[%d] - eta;
  return -0.5 * (e * e);
}
""" % (nf - 1, nf - 1)


def coef_host(rows):
    rows = numpy.asarray(rows, float)
    nf = rows.shape[1]
    y = rows[:, nf - 1]

    def f(parameter):
        eta = numpy.asarray(parameter[0], float)
        for j in range(nf - 1):
            eta = eta + rows[:, j] * numpy.asarray(parameter[j + 1])
        e = y - eta
        return -0.5 * (e * e)
    return f


def wide_family(rows):
    """The DeviceLikelihood of wide_source over ``rows`` (.model = "wide": what
    rowpath_cases.reference dispatches on)."""
    from nestmc.families import DeviceLikelihood
    rows = numpy.asarray(rows, float)
    nf = rows.shape[1]
    fam = DeviceLikelihood(rows, wide_source(nf), 2, consts=wide_weights(nf),
                           host_function=wide_host(rows))
    fam.model = "wide"
    return fam


def coef_family(rows):
    from nestmc.families import DeviceLikelihood
    rows = numpy.asarray(rows, float)
    nf = rows.shape[1]
    fam = DeviceLikelihood(rows, coef_source(nf), nf, host_function=coef_host(rows))
    fam.model = "coef"
    return fam


def poly_source(P):
    """Rows [x, y], theta [c_0..c_{P-1}]: any number of parameters over two fields.
    eta = c_0 + x (c_1 + x (c_2 + ...)) by Horner's rule, ll = -0.5 (y - eta)^2."""
    return r"""
__device__ double nmc_user_loglik(const double* th, const double* row, const double* k) {
  double eta = th[%d];
  for (int j = %d; j >= 0; --j) eta = fma(eta, row[0], th[j]);
  const double e = row[1] - eta;
  return -0.5 * (e * e);
}
""" % (P - 1, P - 2)


def poly_family(x, y, P):
    from nestmc.families import DeviceLikelihood
    x, y = numpy.asarray(x, float), numpy.asarray(y, float)

    def f(parameter):
        eta = numpy.asarray(parameter[P - 1], float)
        for j in range(P - 2, -1, -1):
            eta = eta * x + numpy.asarray(parameter[j])
        e = y - eta
        return -0.5 * (e * e)
    return DeviceLikelihood(numpy.stack([x, y], 1), poly_source(P), P, host_function=f)


def user_logistic(fam):
    """The built-in Logistic family ``fam`` (with intercept) as a user family on the same
    rows: FamLogistic's own expression, so every sum is the built-in's bit for bit."""
    from nestmc.families import DeviceLikelihood
    assert fam.intercept and fam.n_params == fam.n_fields
    return DeviceLikelihood(fam.obs(), logistic_source(fam.n_fields - 1), fam.n_params,
                            host_function=fam)
