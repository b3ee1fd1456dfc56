"""samplePosterior on the GPU: the reference's API and files, the device's loop.

Control flow of posteriorSampling.samplePosterior (:28-216) with the per-chain
Python hot loop (MCMC/Sampler/StepMethod, :790-1158) replaced by libnestmc:

  validate + prepare directories/logs        (:147-168, :1018-1043)
  shard chains over GPUs (contiguous blocks of global chain ids)      nestmc.parallel
  init of every chain, RandomState(c), LLs batched on its GPU
                                             (:1060-1141, :725-758)   nestmc.init
  device loop: nmc_run over all iterations   (:862-896)               nestmc.engine
  device sample store -> sample.<c>.csv      (:898-936)               nestmc.output
  optional per-observation LL rows           (:890-891, :907-909)

The product path never falls back to the CPU: a likelihood that is not a device
family (nestmc.families) or a missing GPU/library raises.
"""

import datetime
import os
from concurrent.futures import ThreadPoolExecutor

import numpy

from . import _lib
from . import output
from . import convergence as _conv
from . import correlation as _correlation
from . import groupcmp as _groupcmp
from . import summary as _summary
from . import loo as _loo
from . import loopit as _loopit
from . import rankdiag as _rankdiag
from . import ppc as _ppc
from . import predict as _predict
from . import waic as _waic
from .engine import Engine
from .families import is_family
from .init import init_chains
from .parallel import shard


def schedule(n_iter, n_samples):
    """MCMC.__init__ burn/thin (posteriorSampling.py:1018-1027)."""
    if n_iter < n_samples:
        print("nIter (%i) cannot be less than nSamples (%i)." % (n_iter, n_samples))
        raise Exception()
    burn = n_iter // 2 if n_iter // 2 > n_samples else n_iter - n_samples
    thin = int(numpy.ceil((n_iter - burn) / n_samples))
    return burn, thin


def record_iterations(n_iter, burn, thin):
    return [i for i in range(n_iter) if i % thin == 0 and i >= burn]


def _sizes(n_groups, n_responses, pooling):
    if isinstance(n_responses, (int, numpy.integer)):
        sizes = [int(n_responses)] * n_groups
    else:
        sizes = [int(v) for v in n_responses]       # list or tuple (the reference: list only)
        if len(sizes) != n_groups:
            raise ValueError("nResponsesPerGroup needs one entry per group")
    if pooling == "complete":
        sizes = [int(sum(sizes))]                  # CompletePooling: one group (:667-671)
    return sizes


def sample_posterior(nChains, nIter, nSamples, parameterName, nGroups, nResponsesPerGroup,
                     pooling, logLikelihoodFunction, outputDirectory, saveLogLikelihood=True,
                     priorDistribution=None, startWithMLE=False, startingPointValueRange=None,
                     nProcesses=1, displayProgress=True, loggingLevel="info", *,
                     seed=0, devices=None, rng="philox", chains=None, return_samples=False,
                     write_files=True, replay=None, process_per_device=False, _rank=None,
                     computeWaic=False, computeDiagnostics=False, computeSummary=False,
                     computeLoo=False, computeRankDiagnostics=False,
                     computeGroupComparison=False, computeCorrelation=False,
                     computePredictiveChecks=False, predictFor=None, computeLooPit=False):
    """Drop-in for posteriorSampling.samplePosterior (same positional/keyword API).

    Extra keyword-only options (all optional):
      seed       Philox seed (key = (global chain id, seed)); default 0
      devices    GPU ids to shard chains over (default: [0]); chains are split in
                 contiguous blocks so chain c always draws the same stream
      process_per_device  one process per GPU instead of one engine per GPU in this
                 process: this process starts len(devices) ranks (nestmc.ranks) before it
                 makes any HIP call; rank r runs its contiguous block of chains on
                 devices[r], and after the loop ONE RCCL gather brings every rank's sample
                 store to rank 0, which writes every sample file (the reference's process
                 fan-out, posteriorSampling.py:182-201, at the GPU level); the files are
                 byte-identical to the one-process path's
      rng        "philox" (default) or "replay" (test use)
      replay     rng="replay": dict of captured variates z, u [C, iter, P, G] and
                 hz, hu [C, iter, P] (chain axis = position in ``chains``)
      chains     run only these global chain ids (multi-process sharding)
      return_samples  also return {"rows": [C][rows][cols], "row_index", "header"}
      computeWaic  after the loop, reduce the per-observation log-likelihood of every
                 recorded row (the numbers saveLogLikelihood would print) to WAIC on the
                 GPU (nestmc.waic): outputDirectory/waic.csv and waic_pointwise.csv, and
                 "waic" (a nestmc.waic.WaicResult) in the returned dict; needs no
                 logLikelihood files, so saveLogLikelihood may be False
      computeDiagnostics  after the loop, compute R-hat and the effective sample size of every
                 column on the GPU from the device sample store (nestmc.convergence; the
                 statistics of diagnoseSamples at full precision, without sample files):
                 outputDirectory/convergence.csv, and "convergence" (a
                 nestmc.convergence.ConvergenceResult) in the returned dict.  The recorded
                 rows are cut into two halves: an odd number of them (or fewer than four)
                 raises ValueError before sampling starts.  Median and HDI: computeSummary
      computeSummary  after the loop, sort every column of the device sample store on the GPU
                 and take its median, 95 % HDI, minimum and maximum (nestmc.summary; the
                 numbers of diagnoseSamples at full precision, without sample files):
                 outputDirectory/summary.csv, and "summary" (a nestmc.summary.SummaryResult)
                 in the returned dict; with computeDiagnostics as well also "assessment", the
                 table of Diagnostic.assessment.  With one engine only per-column results
                 leave the device; several engines (devices=[...]) and the ranks of
                 process_per_device each sort their own chains' values and rank 0 merges the
                 sorted columns on the host -- as many bytes as the sample gather those paths
                 already do.  Fewer than two values per column raise ValueError before
                 sampling starts
      computeLoo  after the loop, compute PSIS-LOO on the GPU from the device sample store
                 (nestmc.loo): elpd_loo with its pointwise terms and the Pareto k of every
                 observation, which says which terms not to trust: outputDirectory/loo.csv
                 and loo_pointwise.csv, "loo" (a nestmc.loo.LooResult) in the returned dict,
                 and one warning line in the log when some k exceed the threshold.  One
                 engine only: with several devices, chains= shards or process_per_device it
                 raises NotImplementedError before sampling starts (DESIGN section 10 has the
                 protocol that would lift this)
      computeRankDiagnostics  after the loop, compute the rank-normalised and the folded
                 split-R-hat, bulk-ESS and tail-ESS of every column (Vehtari et al. 2021)
                 on the GPU from the device sample store (nestmc.rankdiag):
                 outputDirectory/rank_diagnostics.csv, and "rank_diagnostics" (a
                 nestmc.rankdiag.RankDiagnosticsResult) in the returned dict.  The recorded
                 rows are cut into two halves: an odd number of them (or fewer than four)
                 raises ValueError before sampling starts.  Ranks are global, so one engine
                 only: several devices, chains= shards or process_per_device raise
                 NotImplementedError before sampling starts (DESIGN section 10 has the
                 protocol that would lift this)
      computeGroupComparison  after the loop, count on the GPU from the device sample store,
                 per parameter, every group's rank among the G groups in every sample and
                 every ordered pair's wins (nestmc.groupcmp: the league table of a multilevel
                 model): outputDirectory/group_ranking.csv (mean and median rank with a 95 %
                 rank interval, the probabilities of being lowest and highest) and
                 group_pairwise.csv (P(theta_g > theta_h)), and "group_comparison" (a
                 nestmc.groupcmp.GroupComparisonResult) in the returned dict.  The counts are
                 integers: several engines (devices=[...]), chains= shards merged by the
                 caller and the ranks of process_per_device give the one engine's numbers bit
                 for bit.  pooling="complete" has one group and raises ValueError before
                 sampling starts
      computeCorrelation  after the loop, compute on the GPU from the device sample store the
                 posterior covariance and correlation matrix of all columns over all recorded
                 rows and chains (nestmc.correlation: the comoments by fp64 matrix
                 instructions, only [cols, cols] leaves the device):
                 outputDirectory/correlation.csv (the square correlation matrix),
                 correlation_pairs.csv (the pairs a person reads first: the parameters of a
                 group against each other and, under partial pooling, every theta_g against
                 its _mu and _sigma2) and "correlation" (a nestmc.correlation
                 .CorrelationResult) in the returned dict.  Several engines and the ranks of
                 process_per_device are merged by Chan's update: within rounding of the one
                 engine's numbers, not bit-identical.  Fewer than two samples raise ValueError
                 before sampling starts
      computePredictiveChecks  after the loop, draw on the GPU a replicated data set from every
                 recorded sample and compare it with the observed data (nestmc.ppc; the
                 replicates are reduced where they are drawn and never leave the device): per
                 observation the predictive mean, sd, standardised residual and PIT, per group
                 the posterior predictive p-values of its mean, variance, minimum and maximum:
                 outputDirectory/ppc_groups.csv and ppc_pointwise.csv, "predictive_checks" (a
                 nestmc.ppc.PpcResult) in the returned dict and one warning line naming the
                 groups and statistics with p < 0.025 or p > 0.975.  Any number of engines and
                 ranks (merged in engine and rank order: counts exactly, moments by Chan's
                 update).  A family that cannot draw (a DeviceLikelihood without
                 nmc_user_predict) raises ValueError before sampling starts
      computeLooPit  after the loop, compute on the GPU from the device sample store the
                 leave-one-out PIT and predictive moments of every observation (nestmc.loopit):
                 every sample's replicate of observation i -- computePredictiveChecks' own --
                 re-weighted by the PSIS weight of leaving i out, so that, unlike the in-sample
                 PIT, an observation is not checked against a fit that has seen it:
                 outputDirectory/loo_pit_pointwise.csv and loo_pit_groups.csv, "loo_pit" (a
                 nestmc.loopit.LooPitResult; its .loo is the LooResult of the same pass) in
                 the returned dict and one log line with the PITs outside [0.025, 0.975]
                 against the expected 5 %.  With computeLoo as well the one pass serves both.
                 One engine only, as computeLoo; a family that cannot draw and fewer than two
                 samples raise ValueError before sampling starts
      predictFor  a nestmc.NewData(obs, group): rows the model was not fitted to, in the
                 family's row layout, each with a group code -- g >= 0 a training group,
                 -(k + 1) new group k, a group the model has never seen, whose values are drawn
                 from every sample's hyper-parameters (pooling="partial" only).  After the loop
                 the GPU evaluates, from the device sample store, per new row the predictive
                 mean and sd and, where the row's response is given (not NaN), its PIT and the
                 log predictive density of the held-out value (nestmc.predict; the draws never
                 leave the device): outputDirectory/prediction_pointwise.csv and
                 prediction_groups.csv, "predictions" (a nestmc.predict.PredictionResult) in
                 the returned dict and one log line with elpd_test and its standard error.
                 Any number of engines and ranks, merged as the predictive checks are.  A
                 DeviceLikelihood without nmc_user_predict gets the density alone.  A table of
                 another width, a group code beyond the training groups or a new group without
                 partial pooling raises ValueError before sampling starts
    nProcesses sizes the host threads used for chain initialisation and CSV writing.
    """
    start_time = datetime.datetime.now()
    if not is_family(logLikelihoodFunction):
        raise TypeError(
            "logLikelihoodFunction must be a nestmc device family: a built-in one "
            "(nestmc.LinearRegression, GaussianMean, Logistic) or "
            "nestmc.DeviceLikelihood(obs_rows, source, n_params, consts=...) wrapping a "
            "per-observation '__device__ double nmc_user_loglik(theta, row, k)' that is "
            "compiled for the GPU at run time. A plain Python callable -- e.g. the "
            "reference examples' functools.partial(computeLogLikelihood, data=data) "
            "(example/regression.py:53-67, 91) -- cannot run on the GPU, and this sampler "
            "has no CPU fallback by design; pass the callable as "
            "DeviceLikelihood(..., host_function=callable) to keep it for host-side checks "
            "(INTEGRATION.md, 'Porting a likelihood callable').")
    if pooling not in ("partial", "none", "complete"):
        raise Exception("Invalid pooling: ", pooling)
    if computeLoo and ((devices is not None and len(list(devices)) > 1) or chains is not None
                       or process_per_device or _rank is not None):
        raise NotImplementedError(
            "computeLoo needs every chain in one engine: several devices, chains= shards and "
            "process_per_device are not supported yet")
    if computeLooPit and ((devices is not None and len(list(devices)) > 1) or chains is not None
                          or process_per_device or _rank is not None):
        raise NotImplementedError(
            "computeLooPit needs every chain in one engine: several devices, chains= shards and "
            "process_per_device are not supported yet")
    if computeRankDiagnostics and ((devices is not None and len(list(devices)) > 1)
                                   or chains is not None or process_per_device
                                   or _rank is not None):
        raise NotImplementedError(
            "computeRankDiagnostics needs every chain in one engine (ranks are global): several "
            "devices, chains= shards and process_per_device are not supported yet")
    if computeGroupComparison and (pooling == "complete" or nGroups < 2):
        raise ValueError("computeGroupComparison compares a parameter's groups with each other: "
                         "it needs at least two groups (pooling='complete' has one)")
    if computePredictiveChecks and not logLikelihoodFunction.response_fields():
        raise ValueError("computePredictiveChecks needs a family that can draw from its "
                         "likelihood: this DeviceLikelihood's source does not define "
                         "nmc_user_predict (INTEGRATION.md, 'Posterior predictive checks')")
    if computeLooPit and not logLikelihoodFunction.response_fields():
        raise ValueError("computeLooPit needs a family that can draw from its likelihood: this "
                         "DeviceLikelihood's source does not define nmc_user_predict "
                         "(INTEGRATION.md, 'Posterior predictive checks')")
    if predictFor is not None:
        if not isinstance(predictFor, _predict.NewData):
            raise ValueError("predictFor must be a nestmc.NewData(obs, group)")
        predictFor.check(logLikelihoodFunction, 1 if pooling == "complete" else nGroups, pooling)
    names = tuple(parameterName)
    if len(names) != logLikelihoodFunction.n_params:
        raise ValueError("parameterName has %d names, the likelihood family has %d parameters"
                         % (len(names), logLikelihoodFunction.n_params))
    if nProcesses is None or nProcesses <= 0:
        nProcesses = os.cpu_count() or 1
    threads = max(1, min(int(nProcesses), 64))
    if _rank is not None:
        # a rank of process_per_device: the parent prepared the directories and logs the run
        hg, world, rank = _rank
        displayProgress = displayProgress and rank == 0
        sample_dir = outputDirectory + "/sample/" if write_files else None
        log_dir = outputDirectory + "/log/" if write_files else None
        logger = None
    elif write_files:
        sample_dir, log_dir = output.prepare_directories(outputDirectory)
        logger = output.get_logger(log_dir + "samplePosterior.log", "samplePosterior",
                                   loggingLevel)
    else:
        sample_dir = log_dir = None
        logger = None
    msg = "MCMC sampling.\n\tpooling: %s.\n\tnChains: %i, nIterPerChain: %i, " \
          "nSamplesPerChain: %i." % (pooling, nChains, nIter, nSamples)
    if logger:
        logger.info(msg)
    if displayProgress:
        print(msg)

    burn, thin = schedule(nIter, nSamples)
    if computeDiagnostics:
        n_rec = len(record_iterations(nIter, burn, thin))
        if n_rec % 2 or n_rec < 4:
            raise ValueError("computeDiagnostics cuts the %d recorded rows of a chain into two "
                             "halves: their number must be even and at least 4" % n_rec)
    if computeRankDiagnostics:
        n_rec = len(record_iterations(nIter, burn, thin))
        if n_rec % 2 or n_rec < 4:
            raise ValueError("computeRankDiagnostics cuts the %d recorded rows of a chain into "
                             "two halves: their number must be even and at least 4" % n_rec)
    if computeSummary:
        n_val = len(record_iterations(nIter, burn, thin)) * \
            (nChains if chains is None else len(chains))
        if n_val < 2:
            raise ValueError("computeSummary needs at least two values per column: the "
                             "recorded rows of all chains give %d" % n_val)
    if computeLoo and len(record_iterations(nIter, burn, thin)) * nChains < 2:
        raise ValueError("computeLoo needs at least two samples")
    if computeLooPit and len(record_iterations(nIter, burn, thin)) * nChains < 2:
        raise ValueError("computeLooPit needs at least two samples")
    if computePredictiveChecks and len(record_iterations(nIter, burn, thin)) * nChains < 2:
        raise ValueError("computePredictiveChecks needs at least two samples")
    if predictFor is not None and len(record_iterations(nIter, burn, thin)) * nChains < 2:
        raise ValueError("predictFor needs at least two samples")
    if computeCorrelation:
        n_val = len(record_iterations(nIter, burn, thin)) * \
            (nChains if chains is None else len(chains))
        if n_val < 2:
            raise ValueError("computeCorrelation needs at least two samples: the recorded rows "
                             "of all chains give %d" % n_val)
    sizes = _sizes(nGroups, nResponsesPerGroup, pooling)
    G = len(sizes)
    priors = None
    if pooling in ("none", "complete"):
        if priorDistribution is None or len(priorDistribution) != len(names):
            raise ValueError("Invalid prior")
        priors = list(priorDistribution)
    elif priorDistribution is not None and logger:
        logger.info("Partial pooling ignores prior distribution.")
    # partial pooling still draws start values from the priors when given
    # (MCMC._findStartingPoint :1076-1077); the sampler itself ignores them (:713-715)
    start_priors = list(priorDistribution) if priorDistribution is not None else None
    if pooling == "partial" and G < 2:
        raise ValueError("partial pooling needs at least two groups (the invgamma update of "
                         "posteriorSampling.py:494-498 has shape (G-1)/2)")

    chain_ids = list(range(nChains)) if chains is None else [int(c) for c in chains]
    if (rng == "replay") != (replay is not None):
        raise ValueError("rng='replay' needs replay= variates (and only then)")
    devices = [0] if devices is None else list(devices)
    if process_per_device and _rank is None:
        # one process per GPU, started before this process makes any HIP call
        if chains is not None or replay is not None:
            raise ValueError("process_per_device runs all nChains chains on the Philox "
                             "stream (no chains= / replay=)")
        from . import ranks
        kw = dict(nChains=nChains, nIter=nIter, nSamples=nSamples, parameterName=names,
                  nGroups=nGroups, nResponsesPerGroup=nResponsesPerGroup, pooling=pooling,
                  logLikelihoodFunction=logLikelihoodFunction, outputDirectory=outputDirectory,
                  saveLogLikelihood=saveLogLikelihood, priorDistribution=priorDistribution,
                  startWithMLE=startWithMLE, startingPointValueRange=startingPointValueRange,
                  nProcesses=max(1, threads // len(devices)), displayProgress=displayProgress,
                  loggingLevel=loggingLevel, seed=seed, rng=rng,
                  return_samples=return_samples, write_files=write_files,
                  computeWaic=computeWaic, computeDiagnostics=computeDiagnostics,
                  computeSummary=computeSummary,
                  computeGroupComparison=computeGroupComparison,
                  computeCorrelation=computeCorrelation,
                  computePredictiveChecks=computePredictiveChecks, predictFor=predictFor)
        res = ranks.run_per_device(kw, devices)
        _finish_log(logger, [], start_time, displayProgress)
        return res
    if _lib.device_count() < 1:
        raise _lib.NestmcError("no HIP device visible: the sampler runs on MI355X only")
    rank_info = None
    if _rank is not None:
        # this rank's padded contiguous shard (equal store sizes for the RCCL gather; chains
        # with ids >= nChains are padding, run and dropped) on its own device
        from .parallel import padded_shard
        s0, per, real = padded_shard(nChains, world, rank)
        chain_ids = list(range(s0, s0 + per))
        rank_info = dict(hg=hg, world=world, rank=rank, device=devices[rank], n_total=nChains)
        devices = [devices[rank]]
    partial = pooling == "partial"

    # ---- chain logs; initialisation (reference RNG order, RandomState(chain)) ----
    if displayProgress:
        output.print_progress("Initialising %d chains." % len(chain_ids))
    chain_logs = []
    if log_dir:
        for c in chain_ids:
            if c >= nChains:        # (a rank's padding chains)
                continue
            lg = output.get_logger(log_dir + "/mcmc.chain%.2i.log" % c, "mcmc.chain%.2i" % c,
                                   loggingLevel)
            lg.info("chain %i. Started looking for a reasonable starting state." % c)
            chain_logs.append(lg)
    # ---- shard contiguous blocks of chains over the devices; every device
    #      initialises its own chains, their likelihoods evaluated in batches on it --
    def make_engine(r, dev):
        s0, cnt = shard(len(chain_ids), len(devices), r)
        if cnt == 0:
            return None
        ids = chain_ids[s0:s0 + cnt]
        if ids != list(range(ids[0], ids[0] + cnt)):
            raise ValueError("chains must be contiguous global ids per device")
        eng = Engine(logLikelihoodFunction, sizes, cnt, pooling, priors, seed=seed,
                     chain_base=ids[0], device=dev, rng=rng)
        try:
            sl = slice(s0, s0 + cnt)
            st = init_chains(logLikelihoodFunction, sizes, names, ids, pooling, start_priors,
                             startingPointValueRange, startWithMLE,
                             threads=max(1, threads // len(devices)),
                             group_ll=eng.eval_group_ll)
            eng.set_state(st["value"], st["log_prior"], st["ll"], st["mu"], st["s2"])
            if replay is not None:
                eng.set_replay(*(numpy.asarray(replay[k])[sl] for k in ("z", "u", "hz", "hu")))
            eng.set_schedule(nIter, burn, thin, 100)
        except BaseException:
            eng.close()
            raise
        return (eng, s0, ids)

    # one host thread per engine: each initialises its chains (reference RNG order) with
    # their likelihoods batched on its own device, concurrently with the others
    if len(devices) > 1:
        with ThreadPoolExecutor(max_workers=len(devices)) as ex:
            futs = [ex.submit(make_engine, r, dev) for r, dev in enumerate(devices)]
        made, err = [], None
        for f in futs:                 # (every worker has finished: the pool has shut down)
            try:
                made.append(f.result())
            except BaseException as e:   # one device failed: release the others' engines
                err = err or e
        if err is not None:
            for m in made:
                if m is not None:
                    m[0].close()
            raise err
    else:
        made = [make_engine(0, devices[0])]
    engines = [e for e in made if e is not None]
    try:
        return _sample_loop(engines, nIter, burn, thin, names, G, partial, saveLogLikelihood,
                            write_files, sample_dir, threads, displayProgress, return_samples,
                            logger, chain_logs, start_time, rank_info,
                            compute_waic=bool(computeWaic), waic_dir=outputDirectory,
                            n_real=nChains, compute_conv=bool(computeDiagnostics),
                            compute_summary=bool(computeSummary), compute_loo=bool(computeLoo),
                            compute_rank=bool(computeRankDiagnostics),
                            compute_group=bool(computeGroupComparison),
                            compute_corr=bool(computeCorrelation),
                            compute_ppc=bool(computePredictiveChecks), predict_for=predictFor,
                            compute_loo_pit=bool(computeLooPit))
    finally:
        for eng, _, _ in engines:
            eng.close()


def _finish_log(logger, chain_logs, start_time, displayProgress):
    elapsed = datetime.datetime.now() - start_time
    msg = "Finished. The elapsed time in total is %s." \
        % datetime.timedelta(seconds=int(elapsed.total_seconds()))
    for lg in chain_logs:
        lg.info("100% complete.")
        output.close_logger(lg)
    if logger:
        logger.info(msg)
        output.close_logger(logger)
    if displayProgress:
        print("")
        output.print_progress(msg)


def _gather_rank(engines, rank_info):
    """process_per_device: ONE ncclGather of every rank's sample store to rank 0 (RCCL over
    xGMI), the padding chains dropped -> rank 0: [rows][cols][nChains], others: None; the
    accepted counts travel over the host group (rank 0: [nChains, P, G])."""
    from . import parallel
    eng = engines[0][0]
    hg, world, rank, n = (rank_info[k] for k in ("hg", "world", "rank", "n_total"))
    comm = parallel.rccl_comm(hg, world, rank, rank_info["device"])
    try:
        full = parallel.gather_samples(eng, comm, root=0)
    finally:
        parallel.rccl_destroy(comm)
    reals = [parallel.padded_shard(n, world, r)[2] for r in range(world)]
    acc = hg.gather(numpy.ascontiguousarray(eng.accept_counts()).tobytes())
    if rank != 0:
        return None, None
    raw = parallel.assemble(full, reals)
    P, G = eng.P, eng.G
    accs = [numpy.frombuffer(a, dtype=numpy.int64).reshape(-1, P, G)[:reals[r]]
            for r, a in enumerate(acc)]
    return raw, numpy.concatenate(accs, axis=0)


def _waic_of(engines, rank_info, n_real):
    """computeWaic: every engine's chain-block partials over all recorded rows (its padding
    chains, ids >= n_real, as the identity), merged in engine order; the ranks of
    process_per_device send theirs over the host group and rank 0 merges them in rank order
    (the other ranks: None)."""
    parts = []
    for eng, _, ids in engines:
        n_valid = sum(1 for c in ids if c < n_real)
        if n_valid > 0:
            parts.extend(eng.waic_partials(n_valid=n_valid))
        else:
            parts.append(_waic.identity(int(eng.off[-1])))
    part = _waic.merge(parts)
    off = engines[0][0].off
    if rank_info is not None:
        got = rank_info["hg"].gather(numpy.ascontiguousarray(part).tobytes())
        if rank_info["rank"] != 0:
            return None
        part = _waic.merge_ranks([numpy.frombuffer(b, dtype=numpy.float64).reshape(5, -1)
                                  for b in got])
    return _waic.finish(part, off)


def _ppc_of(engines, rank_info, n_real):
    """computePredictiveChecks: every engine's chain-block partials over all recorded rows (its
    padding chains, ids >= n_real, as the identity), merged in engine order; the ranks of
    process_per_device send theirs over the host group and rank 0 merges them in rank order
    and finishes (the other ranks: None).  A draw that is not finite is an error."""
    eng0 = engines[0][0]
    parts = []
    for eng, _, ids in engines:
        n_valid = sum(1 for c in ids if c < n_real)
        if n_valid > 0:
            blocks, bad = eng.ppc_partials_raw(n_valid=n_valid)
            blocks[0]["nonfinite"] = bad
            parts.extend(blocks)
        else:
            parts.append(_ppc.identity(int(eng.off[-1]), eng.G, eng.n_resp()))
    part = _ppc.merge(parts)
    if rank_info is not None:
        got = rank_info["hg"].gather(_ppc.pack(part))
        if rank_info["rank"] != 0:
            return None
        part = _ppc.merge_ranks([_ppc.unpack(b) for b in got])
    if part["nonfinite"]:
        raise _lib.NestmcError("posterior predictive checks: %d draws were not finite"
                               % part["nonfinite"])
    return _ppc.finish(part, eng0.off, eng0.observed())


def _predict_of(engines, rank_info, n_real, new_data):
    """predictFor: every engine's chain-block partials for the new table over all recorded rows
    (its padding chains, ids >= n_real, as the identity), merged in engine order; the ranks of
    process_per_device send theirs over the host group and rank 0 merges them in rank order and
    finishes (the other ranks: None).  A draw or a held-out log density that is not finite is an
    error."""
    eng0 = engines[0][0]
    parts = []
    for eng, _, ids in engines:
        n_valid = sum(1 for c in ids if c < n_real)
        if n_valid > 0:
            eng.set_new_data(new_data)
            blocks, bad = eng.predict_partials_raw(n_valid=n_valid)
            blocks[0]["nonfinite_draws"], blocks[0]["nonfinite_ll"] = bad
            parts.extend(blocks)
        else:
            parts.append(_predict.identity(new_data.n_new, eng.n_resp()))
    part = _predict.merge(parts)
    if rank_info is not None:
        got = rank_info["hg"].gather(_predict.pack(part))
        if rank_info["rank"] != 0:
            return None
        part = _predict.merge_ranks([_predict.unpack(b) for b in got])
    if part["nonfinite_draws"] or part["nonfinite_ll"]:
        raise _lib.NestmcError("prediction: %d draws and %d log densities were not finite"
                               % (part["nonfinite_draws"], part["nonfinite_ll"]))
    return _predict.finish(part, new_data, eng0.family.response_fields())


def _conv_of(engines, rank_info, n_real, header):
    """computeDiagnostics: every engine's partial sums over all recorded rows (its padding
    chains, ids >= n_real, excluded); the chain blocks' variogram sums merged in engine order
    and the half-chain moments concatenated in global chain order; the ranks of
    process_per_device send theirs over the host group and rank 0 merges them in rank order
    (the other ranks: None)."""
    parts, means, m2s = [], [], []
    eng0 = engines[0][0]
    n = eng0.n_rows // 2
    for eng, _, ids in engines:
        n_valid = sum(1 for c in ids if c < n_real)
        if n_valid > 0:
            vg, mean, m2 = eng.conv_partials(n_valid=n_valid)
            parts.extend(vg)
            means.append(mean[:, :, :n_valid])
            m2s.append(m2[:, :, :n_valid])
        else:
            parts.append(numpy.zeros((eng.cols, n)))
    vg = _conv.merge(parts)
    cols = eng0.cols
    mean = numpy.concatenate(means, axis=2) if means else numpy.zeros((cols, 2, 0))
    m2 = numpy.concatenate(m2s, axis=2) if m2s else numpy.zeros((cols, 2, 0))
    if rank_info is not None:
        buf = numpy.concatenate([vg.ravel(), mean.ravel(), m2.ravel()])
        got = rank_info["hg"].gather(numpy.ascontiguousarray(buf).tobytes())
        if rank_info["rank"] != 0:
            return None
        vgs, means, m2s = [], [], []
        for b in got:
            a = numpy.frombuffer(b, dtype=numpy.float64)
            nv = (len(a) - cols * n) // (4 * cols)
            vgs.append(a[:cols * n].reshape(cols, n))
            means.append(a[cols * n:cols * n + 2 * cols * nv].reshape(cols, 2, nv))
            m2s.append(a[cols * n + 2 * cols * nv:].reshape(cols, 2, nv))
        vg = _conv.merge_ranks(vgs)
        mean, m2 = numpy.concatenate(means, axis=2), numpy.concatenate(m2s, axis=2)
    return _conv.finish(vg, mean, m2, n, header)


def _group_of(engines, rank_info, n_real, names):
    """computeGroupComparison: every engine's integer counts over all recorded rows and its
    real chains (padding chains, ids >= n_real, excluded; an engine with none adds zeros),
    merged in engine order; the ranks of process_per_device send theirs over the host group
    and rank 0 merges them in rank order (the other ranks: None).  A group value that is not
    finite is an error."""
    eng0 = engines[0][0]
    P, G = eng0.P, eng0.G
    parts = []
    for eng, _, ids in engines:
        n_valid = sum(1 for c in ids if c < n_real)
        parts.append(eng.group_order_counts(n_valid=n_valid) if n_valid > 0
                     else _groupcmp.zero_counts(P, G))
    part = _groupcmp.merge(parts)
    if rank_info is not None:
        got = rank_info["hg"].gather(numpy.ascontiguousarray(_groupcmp.pack(part)).tobytes())
        if rank_info["rank"] != 0:
            return None
        part = _groupcmp.merge([_groupcmp.unpack(numpy.frombuffer(b, dtype=numpy.int64), P, G)
                                for b in got])
    bad = int(part["nonfinite"].sum())
    if bad:
        raise _lib.NestmcError("group comparison: %d group values were not finite" % bad)
    return _groupcmp.finish(part["hist"], part["wins"], part["n_samples"], names)


def _correlation_of(engines, rank_info, n_real, header):
    """computeCorrelation: every engine's moments and comoments over all recorded rows and its
    real chains (padding chains, ids >= n_real, excluded through n_valid; an engine with none
    adds the identity), merged in engine order by Chan's update; the ranks of
    process_per_device send theirs as bytes over the host group and rank 0 merges them in rank
    order and finishes (the other ranks: None).  A value that is not finite is an error."""
    cols = engines[0][0].cols
    parts = []
    for eng, _, ids in engines:
        n_valid = sum(1 for c in ids if c < n_real)
        parts.append(eng.comoments(n_valid=n_valid) if n_valid > 0
                     else _correlation.identity(cols))
    part = _correlation.merge(parts)
    if rank_info is not None:
        got = rank_info["hg"].gather(numpy.ascontiguousarray(_correlation.pack(part)).tobytes())
        if rank_info["rank"] != 0:
            return None
        part = _correlation.merge([_correlation.unpack(numpy.frombuffer(b, dtype=numpy.float64),
                                                       cols) for b in got])
    bad = int(part["nonfinite"].sum())
    if bad:
        raise _lib.NestmcError("correlation: %d values were not finite" % bad)
    return _correlation.finish(part, header)


def _summary_of(engines, rank_info, n_real, header):
    """computeSummary: one engine sorts its store's columns and only per-column results leave
    the device.  Several engines, and the ranks of process_per_device, each sort the values of
    their own real chains (padding chains, ids >= n_real, excluded) and hand over the sorted
    columns -- as many bytes as the sample gather; the engines' columns are merged here, the
    ranks' on rank 0 after a gather over the host group (the other ranks: None).  Order
    statistics depend on the multiset alone: the result is the one engine's, bit for bit."""
    if len(engines) == 1 and rank_info is None:
        eng, _, ids = engines[0]
        return eng.summary(header, n_valid=sum(1 for c in ids if c < n_real))
    cols = engines[0][0].cols
    parts = []
    for eng, _, ids in engines:
        n_valid = sum(1 for c in ids if c < n_real)
        if n_valid * eng.n_rows >= 2:
            parts.append(eng.summary_raw(n_valid=n_valid, want_sorted=True)["sorted"])
        elif n_valid > 0:       # (a single value per column: nothing to sort)
            parts.append(eng.samples_raw()[:, :, 0].T)
        else:
            parts.append(numpy.empty((cols, 0)))
    part = _summary.merge_sorted(parts)
    if rank_info is not None:
        got = rank_info["hg"].gather(numpy.ascontiguousarray(part).tobytes())
        if rank_info["rank"] != 0:
            return None
        part = _summary.merge_sorted([numpy.frombuffer(b, dtype=numpy.float64).reshape(cols, -1)
                                      for b in got])
    return _summary.from_sorted(part, header)


def _sample_loop(engines, nIter, burn, thin, names, G, partial, saveLogLikelihood, write_files,
                 sample_dir, threads, displayProgress, return_samples, logger, chain_logs,
                 start_time, rank_info=None, compute_waic=False, waic_dir=None,
                 n_real=None, compute_conv=False, compute_summary=False, compute_loo=False,
                 compute_rank=False, compute_group=False, compute_corr=False, compute_ppc=False,
                 predict_for=None, compute_loo_pit=False):
    """The device loop, the per-observation LL rows and the sample files of
    sample_posterior (the caller closes the engines whatever happens here).  rank_info: a
    rank of process_per_device -- this rank writes its chains' logLikelihood files, rank 0
    every sample file after the gather."""
    # ---- the device loop ----------------------------------------------------
    rec = record_iterations(nIter, burn, thin)
    if displayProgress:
        output.print_progress("Sampling started. 0% complete.")
    t_loop = datetime.datetime.now()
    steps = 10 if displayProgress and nIter >= 10 else 1
    bounds = [round(nIter * k / steps) for k in range(steps + 1)]
    # the progress steps' calls continue one another: each engine's calls share one resident
    # step launch (nmc_set_resident; bit-identical) when the engine has its device to itself
    devs = [eng.device for eng, _, _ in engines]
    if steps > 1 and len(set(devs)) == len(devs):
        for eng, _, _ in engines:
            eng.set_resident(True)
    for k in range(steps):
        for eng, _, _ in engines:
            eng.run(bounds[k], bounds[k + 1])
        if displayProgress and steps > 1:
            for eng, _, _ in engines:
                eng.synchronize()
            output.print_progress("%i%% complete." % (100 * (k + 1) // steps))
    for eng, _, _ in engines:
        eng.synchronize()
    loop_seconds = (datetime.datetime.now() - t_loop).total_seconds()
    n_total = None if rank_info is None else rank_info["n_total"]
    if saveLogLikelihood and write_files:
        # every recorded row's per-observation LL (:890-891, :907-909 at the values of
        # :656-659), re-evaluated on the device from the sample store and streamed out
        # (a rank's padding chains: file id -1, no file)
        for eng, _, ids in engines:
            fids = ids if n_total is None else [c if c < n_total else -1 for c in ids]
            eng.write_ll_csvs(sample_dir, fids, threads=threads)

    waic_result = None
    if compute_waic:
        waic_result = _waic_of(engines, rank_info, n_real)
        if waic_result is not None and write_files:
            _waic.write_csvs(waic_result, waic_dir)

    loo_result = None
    loo_pit_result = None
    if compute_loo_pit:   # (one engine, no padding chains; the one pass serves computeLoo too)
        loo_pit_result = engines[0][0].loo_pit()
        if write_files:
            _loopit.write_csvs(loo_pit_result, waic_dir)
        line = loo_pit_result.summary()
        if logger:
            logger.info(line)
        if displayProgress:
            output.print_progress(line)
    if compute_loo:   # (one engine, no padding chains: sample_posterior checked)
        loo_result = loo_pit_result.loo if loo_pit_result is not None else engines[0][0].loo()
        if write_files:
            _loo.write_csvs(loo_result, waic_dir)
        warn = loo_result.warning()
        if warn:
            if logger:
                logger.warning(warn)
            if displayProgress:
                output.print_progress(warn)

    header = output.header_names(names, G, partial)
    conv_result = None
    if compute_conv:
        conv_result = _conv_of(engines, rank_info, n_real, header)
        if conv_result is not None and write_files:
            _conv.write_csv(conv_result, waic_dir)
    rank_result = None
    if compute_rank:   # (one engine, no padding chains: sample_posterior checked)
        rank_result = engines[0][0].rank_diagnostics(header)
        if write_files:
            _rankdiag.write_csv(rank_result, waic_dir)
    group_result = None
    if compute_group:
        group_result = _group_of(engines, rank_info, n_real, names)
        if group_result is not None and write_files:
            _groupcmp.write_csvs(group_result, waic_dir)
    corr_result = None
    if compute_corr:
        corr_result = _correlation_of(engines, rank_info, n_real, header)
        if corr_result is not None and write_files:
            _correlation.write_csvs(corr_result, waic_dir, len(names), G, partial)
    ppc_result = None
    if compute_ppc:
        ppc_result = _ppc_of(engines, rank_info, n_real)
        if ppc_result is not None:
            if write_files:
                _ppc.write_csvs(ppc_result, waic_dir)
            warn = ppc_result.warning()
            if warn:
                if logger:
                    logger.warning(warn)
                if displayProgress:
                    output.print_progress(warn)
    predict_result = None
    if predict_for is not None:
        predict_result = _predict_of(engines, rank_info, n_real, predict_for)
        if predict_result is not None:
            if write_files:
                _predict.write_csvs(predict_result, waic_dir)
            line = ("Prediction for %d new observations (%d with a held-out response, %d new "
                    "groups): elpd_test = %.6g +- %.3g."
                    % (predict_result.n_new, predict_result.n_response, predict_for.K,
                       predict_result.elpd_test, predict_result.se))
            if logger:
                logger.info(line)
            if displayProgress:
                output.print_progress(line)
    summary_result = None
    if compute_summary:
        summary_result = _summary_of(engines, rank_info, n_real, header)
        if summary_result is not None and write_files:
            _summary.write_csv(summary_result, waic_dir)

    # ---- samples -> files ----------------------------------------------------
    hdr = header if burn < nIter else None
    rows_all = []
    if rank_info is not None:
        raw, accept = _gather_rank(engines, rank_info)
        if raw is not None:
            if write_files:
                ids = list(range(n_total))
                output.write_sample_csvs(sample_dir, raw, ids, ids, hdr, rec, threads=threads)
            rows_all.append(numpy.transpose(raw, (2, 0, 1)))
        accept = [accept] if accept is not None else []
    else:
        for eng, s0, ids in engines:
            raw = eng.samples_raw()                     # [rows][cols][C_local]
            if write_files:
                output.write_sample_csvs(sample_dir, raw, list(range(len(ids))), ids, hdr, rec,
                                         threads=threads)
            if return_samples:
                rows_all.append(numpy.transpose(raw, (2, 0, 1)))
        accept = [eng.accept_counts() for eng, _, _ in engines] if return_samples else None

    # (a rank: the parent prints and logs the end of the run)
    _finish_log(logger, chain_logs, start_time, displayProgress and rank_info is None)
    if rank_info is not None and rank_info["rank"] != 0:
        return None
    if return_samples:
        res = {"rows": numpy.concatenate(rows_all, axis=0), "row_index": rec,
               "header": header, "burn": burn, "thin": thin,
               "accepted": numpy.concatenate(accept, axis=0),
               "loop_seconds": loop_seconds}
        if waic_result is not None:
            res["waic"] = waic_result
        if loo_result is not None:
            res["loo"] = loo_result
        if loo_pit_result is not None:
            res["loo_pit"] = loo_pit_result
        if conv_result is not None:
            res["convergence"] = conv_result
        if rank_result is not None:
            res["rank_diagnostics"] = rank_result
        if group_result is not None:
            res["group_comparison"] = group_result
        if corr_result is not None:
            res["correlation"] = corr_result
        if ppc_result is not None:
            res["predictive_checks"] = ppc_result
        if predict_result is not None:
            res["predictions"] = predict_result
        if summary_result is not None:
            res["summary"] = summary_result
            if conv_result is not None:
                res["assessment"] = _summary.assessment(conv_result, summary_result)
        return res
    return None
