"""The reference of the correlation tests: nestmc.correlation's definitions in numpy.longdouble
on the float64 store, and the derived tolerance.  numpy only, no GPU import.

The tolerance is derived, not measured (u = 2^-53):
  * A dot product of S terms has error <= gamma_S sum_s |d_k| |d_l| <= gamma_S sqrt(M_kk M_ll)
    (Cauchy-Schwarz), gamma_S ~ S u; the rounding of the two differences adds 2 u per term.
  * An error Delta in a mean enters M only as S Delta_k Delta_l, because the true deviations
    sum to zero; with |Delta| <= S u mean(|x|) that term is negligible while |mean| <= 2^10 sd.
    THE BOUND ASSUMES |mean| <= 2^10 sd: the tests' data stay inside it (store_case).
  * So one engine's |M - M_ref|[k][l] <= 4 S u sqrt(M_ref[k][k] M_ref[l][l])  (factor 4), a
    merged result's the same with factor 8 (two parts' bounds plus the rank-one term), and
    |mean - mean_ref| <= 2 S u mean_ref(|x|).
The bound is loose (real error grows like sqrt(S)); the exact-arithmetic cases of
test_gpu_correlation.py are what catch layout, indexing and padding mistakes."""

import numpy

U = 2.0 ** -53
LD = numpy.longdouble


def reference(raw, n_valid=None):
    """raw [rows][cols][C] float64, chains [0, n_valid) -> dict of mean_ref, M_ref, absmean
    (longdouble), min, max (float64), nonfinite (int64) and S."""
    raw = numpy.asarray(raw, dtype=numpy.float64)
    rows, cols, C = raw.shape
    nv = C if n_valid is None else int(n_valid)
    S = rows * nv
    X = numpy.transpose(raw[:, :, :nv], (1, 0, 2)).reshape(cols, S)
    Xl = X.astype(LD)
    mean = Xl.sum(axis=1) / LD(S)
    d = Xl - mean[:, None]
    M = numpy.empty((cols, cols), dtype=LD)
    for k in range(cols):
        M[k] = (d * d[k][None, :]).sum(axis=1)
    return dict(mean_ref=mean, M_ref=M, absmean=numpy.abs(Xl).sum(axis=1) / LD(S),
                min=X.min(axis=1), max=X.max(axis=1),
                nonfinite=numpy.count_nonzero(~numpy.isfinite(X), axis=1).astype(numpy.int64),
                S=S)


def ratios(result, ref, S, factor):
    """(largest |M - M_ref| / bound, largest |mean - mean_ref| / bound) of a part dict."""
    dg = numpy.diagonal(ref["M_ref"])
    bound = LD(factor) * S * U * numpy.sqrt(dg[:, None] * dg[None, :])
    err = numpy.abs(numpy.asarray(result["M"]).astype(LD) - ref["M_ref"])
    mbound = LD(2) * S * U * ref["absmean"]
    merr = numpy.abs(numpy.asarray(result["mean"]).astype(LD) - ref["mean_ref"])
    with numpy.errstate(invalid="ignore", divide="ignore"):
        rm = numpy.where(bound > 0, err / bound, numpy.where(err > 0, numpy.inf, 0))
        rv = numpy.where(mbound > 0, merr / mbound, numpy.where(merr > 0, numpy.inf, 0))
    return float(rm.max()), float(rv.max())


def check(result, ref, S, factor):
    """Assert a part dict (mean, min, max, M, nonfinite, n_samples) against reference():
    M and mean within the derived bounds, the rest exactly.  Returns ratios()."""
    assert int(result["n_samples"]) == S == ref["S"]
    assert numpy.array_equal(result["min"], ref["min"]), "min"
    assert numpy.array_equal(result["max"], ref["max"]), "max"
    assert numpy.array_equal(result["nonfinite"], ref["nonfinite"]), "nonfinite"
    M = numpy.asarray(result["M"])
    assert numpy.isfinite(M).all() and numpy.array_equal(M, M.T)
    rm, rv = ratios(result, ref, S, factor)
    print("correlation_ref.check: S = %d, factor %d: M error / bound = %.3g, mean error / bound "
          "= %.3g" % (S, factor, rm, rv))
    assert rm <= 1.0, "M: %.3g of the bound" % rm
    assert rv <= 1.0, "mean: %.3g of the bound" % rv
    return rm, rv


def store_case(seed, rows, cols, C):
    """The tolerance cases' store [rows][cols][C]: column k is offset by 100 (k mod 7) and
    scaled by 10^((k mod 5) - 2); columns 3 / 10 and 8 / 29 are strongly correlated (rho about
    +0.999 and -0.999).  |mean| <= 600 scale and sd ~ scale: inside |mean| <= 2^10 sd."""
    r = numpy.random.RandomState(seed)
    z = r.normal(size=(rows, cols, C))
    if cols > 29:
        z[:, 10] = z[:, 3] + 0.045 * r.normal(size=(rows, C))
        z[:, 29] = -z[:, 8] + 0.045 * r.normal(size=(rows, C))
    k = numpy.arange(cols)
    scale = 10.0 ** ((k % 5) - 2)
    return (z + 100.0 * (k % 7)[None, :, None]) * scale[None, :, None]
