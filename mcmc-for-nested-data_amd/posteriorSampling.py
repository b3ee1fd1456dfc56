"""Drop-in module: ``from posteriorSampling import samplePosterior``.

Same name, signature, defaults and output files as the reference module
(posteriorSampling.py:28-35 in tkngch/MCMC-for-Nested-Data); the MCMC loop runs on
MI355X through libnestmc (see nestmc.sampler).  The likelihood argument must be a
device family from ``nestmc`` (LinearRegression, GaussianMean, Logistic), which is
also callable with the reference's parameter[P][n] -> ll[n] convention.
"""

import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from nestmc.families import GaussianMean, LinearRegression, Logistic  # noqa: E402,F401
from nestmc.sampler import sample_posterior  # noqa: E402


def samplePosterior(nChains, nIter, nSamples,
                    parameterName, nGroups, nResponsesPerGroup,
                    pooling, logLikelihoodFunction,
                    outputDirectory,
                    saveLogLikelihood=True,
                    priorDistribution=None,
                    startWithMLE=False, startingPointValueRange=None,
                    nProcesses=1, displayProgress=True, loggingLevel="info",
                    computeWaic=False, computeDiagnostics=False, computeSummary=False,
                    computeLoo=False, computeRankDiagnostics=False,
                    computeGroupComparison=False, computeCorrelation=False,
                    computePredictiveChecks=False, predictFor=None, computeLooPit=False,
                    **gpu_options):
    """Sample the posterior of a nested model; samples go to outputDirectory/sample/.

    Arguments mirror the reference (posteriorSampling.py:28-145).  Keyword-only
    GPU options: seed, devices, rng, chains, return_samples (nestmc.sampler).
    computeWaic=True also reduces the per-observation log-likelihood of the recorded rows
    to WAIC on the GPU (waic.csv, waic_pointwise.csv; nestmc.waic), with or without
    saveLogLikelihood.  computeDiagnostics=True also computes R-hat and the effective sample
    size of every column on the GPU from the device sample store (convergence.csv;
    nestmc.convergence) -- an even number of recorded rows is needed.  computeSummary=True
    also sorts every column of the store on the GPU for its median, 95 % HDI, minimum and
    maximum (summary.csv; nestmc.summary).  computeLoo=True also computes PSIS-LOO with the
    Pareto k diagnostic of every observation on the GPU (loo.csv, loo_pointwise.csv;
    nestmc.loo) -- one engine only.  computeRankDiagnostics=True also computes the
    rank-normalised and folded split-R-hat, bulk-ESS and tail-ESS of every column on the GPU
    (rank_diagnostics.csv; nestmc.rankdiag) -- an even number of recorded rows and one engine
    only.  computeGroupComparison=True also counts, per parameter, every group's rank among the
    groups and every pair's wins on the GPU (group_ranking.csv, group_pairwise.csv;
    nestmc.groupcmp) -- at least two groups, any number of engines.  computeCorrelation=True
    also computes the posterior covariance and correlation matrix of all columns on the GPU
    (correlation.csv, correlation_pairs.csv; nestmc.correlation) -- at least two samples, any
    number of engines.  computePredictiveChecks=True also draws a replicated data set from
    every recorded sample on the GPU and compares it with the observed data, per observation
    and per group (ppc_groups.csv, ppc_pointwise.csv; nestmc.ppc) -- a built-in family or a
    DeviceLikelihood with nmc_user_predict, any number of engines.  predictFor=nestmc.NewData(
    obs, group) also predicts rows the model was not fitted to, of training groups and of
    groups it has never seen, on the GPU (prediction_pointwise.csv, prediction_groups.csv;
    nestmc.predict).  computeLooPit=True also computes the leave-one-out PIT and predictive mean
    and sd of every observation on the GPU, its replicates re-weighted by the PSIS weights of
    leaving it out (loo_pit_pointwise.csv, loo_pit_groups.csv; nestmc.loopit) -- a family that
    can draw, one engine only; with computeLoo the one pass serves both.  Returns None like the reference unless return_samples=True.
    """
    return sample_posterior(nChains, nIter, nSamples, parameterName, nGroups,
                            nResponsesPerGroup, pooling, logLikelihoodFunction,
                            outputDirectory, saveLogLikelihood=saveLogLikelihood,
                            priorDistribution=priorDistribution, startWithMLE=startWithMLE,
                            startingPointValueRange=startingPointValueRange,
                            nProcesses=nProcesses, displayProgress=displayProgress,
                            loggingLevel=loggingLevel, computeWaic=computeWaic,
                            computeDiagnostics=computeDiagnostics,
                            computeSummary=computeSummary, computeLoo=computeLoo,
                            computeRankDiagnostics=computeRankDiagnostics,
                            computeGroupComparison=computeGroupComparison,
                            computeCorrelation=computeCorrelation,
                            computePredictiveChecks=computePredictiveChecks,
                            predictFor=predictFor, computeLooPit=computeLooPit, **gpu_options)
