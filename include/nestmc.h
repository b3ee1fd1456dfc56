/*
 * nestmc.h -- C-ABI of libnestmc.so, the MI355X (gfx950) engine for the MCMC
 * inner loop of tkngch/MCMC-for-Nested-Data.
 *
 * The reference has no FFI: its hot path is Python (posteriorSampling.py).  Each
 * entry point below replaces a piece of that Python, cited file:line, and is
 * bound by the drop-in Python host (mcmc-for-nested-data_amd/nestmc/_lib.py)
 * through ctypes.  Plain C types only; all host buffers are caller-owned and
 * copied; device buffers are owned by the context.  Every function returns 0 on
 * success and a negative code on failure, with the message in nmc_last_error()
 * (thread-local).  A context is used by one host thread at a time.
 *
 * Array layouts (all fp64 unless noted; "c" = local chain, fastest-varying):
 *   value, log_prior, scale  [P][G][C]       ll           [G][C]
 *   (on the device the values after iteration t live in one of two buffers, t & 1)
 *   hyper mu, sigma2         [P][C]          samples      [row][col][C]
 *   replay z, u              [iter][P][G][C] replay hz, hu [iter][P][C]
 *   obs                      [n_obs][n_fields] (group-major, CSR by group_offsets)
 */
#ifndef NESTMC_H
#define NESTMC_H

#ifndef __HIPCC_RTC__
#include <stdint.h>
#else   /* hiprtc (runtime-compiled user families): its own fixed-width types */
typedef __hip_internal::int64_t int64_t;
typedef __hip_internal::uint64_t uint64_t;
typedef __hip_internal::int32_t int32_t;
typedef __hip_internal::uint32_t uint32_t;
typedef __hip_internal::uint8_t uint8_t;
typedef __hip_internal::uint64_t uintptr_t;
#endif

#ifdef __cplusplus
extern "C" {
#endif

typedef struct nmc_ctx nmc_ctx;

/* pooling: StepMethod subclasses, posteriorSampling.py:662-787 */
enum { NMC_POOL_COMPLETE = 0, NMC_POOL_NONE = 1, NMC_POOL_PARTIAL = 2 };

/* likelihood families: device restatements of the user logLikelihoodFunction
 * contract (posteriorSampling.py:61-102) for the models the reference ships or
 * benchmarks (example/regression.py:53-67, example/distribution.py:18-24, cfg 5).
 *   NMC_LL_LINREG    obs = [x_1..x_k, y] (+ implicit ones column if consts[1]=1)
 *                    consts = {k, intercept, sigma (<=0: sigma is the last param)}
 *   NMC_LL_GAUSS_MEAN obs = [m_0..m_{P-1}]; consts = {sd_0..sd_{P-1}}
 *   NMC_LL_LOGISTIC  obs = [x_1..x_k, y]; consts = {k, intercept}              */
enum { NMC_LL_LINREG = 0, NMC_LL_GAUSS_MEAN = 1, NMC_LL_LOGISTIC = 2 };
/* User families (the reference's arbitrary logLikelihoodFunction, :61-102, as device
 * code): ids >= NMC_LL_USER_BASE come from nmc_user_family_compile; consts = the model's
 * constants, passed to the user function as k.                                     */
enum { NMC_LL_USER_BASE = 100 };

/* prior families for none/complete pooling: scipy frozen distributions the
 * reference evaluates with .logpdf (posteriorSampling.py:293-294).
 * params[8] per parameter = {loc, scale, shape, gammaln(shape), log(scale), 0,0,0}
 * (gammaln and log(scale) computed on the host with scipy/numpy).            */
enum { NMC_PRIOR_NORM = 0, NMC_PRIOR_GAMMA = 1, NMC_PRIOR_UNIFORM = 2,
       NMC_PRIOR_EXPON = 3, NMC_PRIOR_HALFNORM = 4, NMC_PRIOR_CAUCHY = 5,
       NMC_PRIOR_LAPLACE = 6, NMC_PRIOR_LOGNORM = 7, NMC_PRIOR_INVGAMMA = 8 };

/* random streams: philox = device Philox4x32-10 (replaces numpy legacy MT19937
 * draws at posteriorSampling.py:306,362,487,498); replay = variates supplied by
 * nmc_set_replay (captured from the reference, for parity).                    */
enum { NMC_RNG_PHILOX = 0, NMC_RNG_REPLAY = 1 };

const char* nmc_last_error(void);
const char* nmc_version(void);
int nmc_device_count(int* n);

/* Replaces the per-chain StepMethod construction (posteriorSampling.py:517-582,
 * :1146-1151): CSR offsets (:554-555), data, priors.  chain_base = global id of
 * local chain 0 (Philox key, posteriorSampling.py:225 seed = chain).           */
/* Compile a user log-likelihood (hiprtc, gfx950) and register it as a family:
 *   source defines  __device__ double nmc_user_loglik(const double* theta,  // [n_params]
 *                                                     const double* row,    // [n_fields]
 *                                                     const double* k);     // consts
 * returning ONE observation's log-likelihood (the reference's logLikelihoodFunction,
 * posteriorSampling.py:61-102, evaluated per row); include_dir = the library's csrc
 * directory (kernels.h and its parts, fam_user.h).  *family_id -> pass as nmc_create's
 * ll_family.
 * 1 <= n_fields <= 64 and 1 <= n_params <= 16, else -1; nmc_create takes the family with
 * an observation table of exactly that width and that many parameters.  Under partial
 * pooling nmc_create also needs the workgroup's Gibbs state of all parameters in a CU's
 * 160 KiB of LDS -- (14 + nleaf (9 + ntail)) n_params + 29 columns of 512 bytes, nleaf and
 * ntail the leaves and the longest tail of numpy's pairwise sum over the groups: at most
 * 12 parameters up to 128 groups, fewer over more leaves -- and refuses a model beyond it
 * ("workgroup state exceeds the 160 KiB LDS of a CU") before anything is launched.
 * Errors carry the compiler log (nmc_last_error).                                  */
int nmc_user_family_compile(const char* source, int n_fields, int n_params,
                            const char* include_dir, int* family_id);
int nmc_user_family_shape(int family_id, int* n_fields, int* n_params);

int nmc_create(nmc_ctx** out, int device, int n_chains, int chain_base,
               int n_groups, int n_params, int pooling, int ll_family,
               const double* ll_consts, int n_ll_consts,
               const int64_t* group_offsets, const double* obs, int64_t n_obs,
               int n_fields, const int* prior_family, const double* prior_params,
               uint32_t seed, int rng_mode);
int nmc_destroy(nmc_ctx* ctx);

/* Chain state after initialisation (PartialPooling._initialiseParameters /
 * _determineIndividualStartingPoint :725-758; StepMethod._setStartingPoint
 * :584-592).  hyper_* may be NULL for none/complete; scale NULL -> 1.0.      */
int nmc_set_state(nmc_ctx* ctx, const double* value, const double* log_prior,
                  const double* ll, const double* hyper_mu, const double* hyper_sigma2,
                  const double* scale);
/* The chain state after the last iteration run (any pointer may be NULL).
 * None / complete pooling: no hyper-parameters exist, hyper_mu and hyper_sigma2
 * come back as NaN.  Partial pooling: log_prior is the device's own copy, each
 * value's log prior under the hyper-parameters of the step that decided it (the
 * step kernels recompute the current one and never read it back); the
 * reference's quantity is nmc_get_log_prior's.                                 */
int nmc_get_state(nmc_ctx* ctx, double* value, double* log_prior, double* ll,
                  double* hyper_mu, double* hyper_sigma2, double* scale);
/* The log priors [P][G][C] as the reference holds them after the last iteration.
 * Partial pooling, once an iteration has run: norm.logpdf(value, mu,
 * sqrt(sigma2)) under the CURRENT hyper-parameters (setPrior :273-282 after
 * every Gibbs update), evaluated on the host from the state nmc_get_state
 * returns, y = (x - loc) / scale as nmc_norm_logpdf.  Before any iteration, and
 * under none / complete pooling: nmc_get_state's log_prior.                   */
int nmc_get_log_prior(nmc_ctx* ctx, double* log_prior);

/* Replay variates [n_iter] (RNG mode NMC_RNG_REPLAY). */
int nmc_set_replay(nmc_ctx* ctx, const double* z, const double* u,
                   const double* hz, const double* hu, int n_iter);

/* Sampler.sample schedule (posteriorSampling.py:827-860, MCMC.__init__
 * :1018-1027): allocates the device sample store for every recorded row.     */
int nmc_set_schedule(nmc_ctx* ctx, int n_iter, int burn, int thin, int tune_interval);
int nmc_n_rows(nmc_ctx* ctx, int* rows, int* cols);

/* Optional per-step trace [n_iter][P][G][C]: accept flags (uint8) and the
 * proposal's group log-likelihood; for parity tests.                         */
int nmc_set_trace(nmc_ctx* ctx, int enable);
int nmc_get_trace(nmc_ctx* ctx, uint8_t* accept, double* ll_prop);

/* Sampler._loop (posteriorSampling.py:862-896) for iterations [iter_begin,
 * iter_end): StepMethod.step (:594-613) + HyperParameter.update (:463-498)
 * + the recorder (:887-889) into the device sample store.  Asynchronous on the
 * context's stream; call nmc_synchronize before reading results.
 * The variates of a launch chunk are drawn before it; the next chunk's (the
 * rest of the call, then as many iterations again after it, within the
 * schedule) are drawn on a second stream beside the chunk's step launch and
 * taken by the chunk or call that starts there (NMC_PREFILL=0: off).  The
 * variates depend on (seed, chain, iteration) alone: results are identical.  */
int nmc_run(nmc_ctx* ctx, int iter_begin, int iter_end);
/* Waits for everything nmc_run / nmc_prefill enqueued (both streams).         */
int nmc_synchronize(nmc_ctx* ctx);
/* Draw the variates of iterations [iter_begin, iter_end) (at most one buffer's
 * worth) now, beside whatever runs, for a later nmc_run that starts at
 * iter_begin: a caller that knows its next call's range (replaces nmc_run's
 * own guess).  No effect on results.  iter_end <= the schedule's n_iter.      */
int nmc_prefill(nmc_ctx* ctx, int iter_begin, int iter_end);
/* Iterations drawn by prefills so far / taken by nmc_run from a prefill.      */
int nmc_prefill_stats(nmc_ctx* ctx, int64_t* issued, int64_t* used);
/* Resident step launch for the consecutive nmc_run calls of a sampling loop
 * (Sampler._loop :872-891 driven in chunks, e.g. samplePosterior's progress
 * steps): a call that continues where the previous one ended is handed to the
 * running launch (a command word in pinned host memory) instead of a new launch;
 * the rows and chain state stay in LDS.  Each call completes its results as a
 * launch does -- after nmc_synchronize its sample / trace rows and hyper-
 * parameters are in HBM, bit for bit those of separate launches; the chain
 * state reaches HBM when the launch parks.  Any other entry point parks the
 * launch first (so every read sees the state of separate launches); it parks
 * itself after NMC_RESIDENT_IDLE_US (20 ms) without a call.  No effect where
 * the context's kernel has no resident form (enabled 0 in nmc_resident_stats).
 * No reference counterpart: host plumbing.                                   */
int nmc_set_resident(nmc_ctx* ctx, int enable);
/* enabled: resident launches possible and on; active: one is running now;
 * launches / calls: resident launches made / calls continued inside one;
 * last_refusal: why the latest call not continued was not (1 another start,
 * 2 kernel timing, 3 longer than a chunk, 4 past the launch's variate buffer,
 * 5 variates not prefilled there, 6 counters would wrap, 7 the launch had
 * parked itself after its idle limit, 8 its prefill did not finish beside
 * the launch within 2 ms -- kernels serialized, e.g. by a profiler's counter
 * pass: the resident form is then turned off for the context).               */
int nmc_resident_stats(nmc_ctx* ctx, int* enabled, int* active, int64_t* launches,
                       int64_t* calls, int* last_refusal);

/* Recorded rows [row_begin, row_begin+n_rows) as [row][col][C].
 * Columns follow StepMethod.values / PartialPooling.values (:648-654, :780-787). */
int nmc_get_samples(nmc_ctx* ctx, int row_begin, int n_rows, double* out);
/* Total accepted proposals per (p, g, c) since nmc_set_state. */
int nmc_get_accept_counts(nmc_ctx* ctx, int64_t* out);

/* StepMethod._computeParameterLogLikelihood (:629-635) on device for arbitrary
 * values theta[P][G][C] -> out[G][C] (used by the host init loop :746-758).  */
int nmc_eval_group_ll(nmc_ctx* ctx, const double* theta, double* out);
/* StepMethod.logLikelihood (:656-659): per-observation LL at the current state,
 * out[C][n_obs] (saveLogLikelihood rows, :907-909).                          */
int nmc_eval_obs_ll(nmc_ctx* ctx, double* out);
/* The same at recorded rows [row_begin, row_begin+n_rows) of the sample store -- the
 * state Sampler._printLogLikelihood (:890-891) evaluated at each recorded iteration:
 * out[C][n_rows][n_obs].                                                       */
int nmc_obs_ll_rows(nmc_ctx* ctx, int row_begin, int n_rows, double* out);
/* saveLogLikelihood=True (:890-891, :907-909): logLikelihood.<chain_ids[c]>.csv in dir
 * (a path prefix ending in '/') for every local chain and recorded row, "%f" joined by
 * ",".  Batches of rows are evaluated on the device and copied to pinned memory while
 * the host formats the previous batch with `threads` threads; a chain whose id is
 * negative gets no file (a rank's padding chains).                             */
int nmc_write_ll_csvs(nmc_ctx* ctx, const char* dir, const int32_t* chain_ids, int threads);
/* WAIC's reduction of that per-observation LL (StepMethod.logLikelihood :656-659 at the
 * recorded values of :890-891, the rows saveLogLikelihood prints at :907-909) over recorded
 * rows [row_begin, row_begin+n_rows) and local chains [0, n_valid), on the device and without
 * forming the matrix; the reduction itself has no counterpart in the reference, whose users
 * compute it from the files.  part[CB][5][n_obs], CB = ceil(C / 64): per chain block and
 * observation the combinable state (m, s, n, mean, M2) -- m = max ll, s = sum exp(ll - m),
 * n = samples, Welford's mean and M2 -- with the block's 64 chains merged in a fixed order
 * (csrc/waic.h; nestmc/waic.py merges the blocks and finishes).  Chains >= n_valid (a rank's
 * padding) enter as the identity (-inf, 0, 0, 0, 0).  1 <= n_valid <= C, n_rows >= 1 and the
 * rows inside the schedule's, else -1; any number of rows per call.  *nonfinite: the terms
 * that were not finite (they propagate into the state; callers treat a count as an error).
 * Event slots 14 and 15 bracket the kernel.                                      */
int nmc_waic_partials(nmc_ctx* ctx, int row_begin, int n_rows, int n_valid, double* part,
                      int64_t* nonfinite);
/* Posterior predictive checks (csrc/ppc.h; no counterpart in the reference).  A replicate
 * y_rep of response field j of observation i at the values of recorded row r and chain c is
 * the family's predict() on the Philox block with counter (r, i, j, purpose 4) and key
 * (chain_base + c, seed): it depends on nothing else.  *nresp: the family's response fields
 * (linreg, logistic: 1, the last field; gauss_mean: every field; a user family: 1 if its
 * source defines nmc_user_predict and NMC_USER_RESP, else 0).  A family with 0, or 2^32 or
 * more observations, is refused (-1) by the two calls below.
 * nmc_ppc_draws: out[C][n_rows][n_obs][nresp], the replicates themselves (at most 65535 rows
 * per call, as nmc_obs_ll_rows).
 * nmc_ppc_partials: over recorded rows [row_begin, row_begin + n_rows) and local chains
 * [0, n_valid), per chain block (CB = ceil(C / 64)):
 *   obs_state[CB][3][nresp][n_obs]      n, Welford's mean and M2 of y_rep over the samples
 *   obs_count[CB][2][nresp][n_obs]      lt = #{y_rep < y}, eq = #{y_rep == y}
 *   group_state[CB][G][nresp][4][3]     n, mean, M2 of T(y_rep) over the samples, T = the
 *                                       group's mean, population variance, minimum, maximum of
 *                                       its observations taken in order
 *   group_count[CB][G][nresp][4][2]     gt = #{T(y_rep) > T(y)}, eq = #{T(y_rep) == T(y)}
 *   ty[G][nresp][4]                     T(y), by the same device function
 * the 64 chains of a block (and, for the groups, waves and row slices) merged in the fixed
 * order csrc/ppc.h documents; nestmc/ppc.py merges the blocks and finishes.  Chains >= n_valid
 * enter as the identity (zero states and counts).  The counts are uint32: a block's count is
 * at most 64 n_rows, so n_rows < 2^26; callers add blocks in int64.  Other argument errors as
 * nmc_waic_partials.  *nonfinite: the draws that were not finite, each counted once; they
 * enter the states as NaN and no count (callers treat a count as an error).  Event slots 13,
 * 14 and 15: the observation kernel runs between 13 and 14, the group kernels between 14
 * and 15.                                                                         */
int nmc_ppc_nresp(nmc_ctx* ctx, int* nresp);
int nmc_ppc_draws(nmc_ctx* ctx, int row_begin, int n_rows, double* out);
int nmc_ppc_partials(nmc_ctx* ctx, int row_begin, int n_rows, int n_valid, double* obs_state,
                     uint32_t* obs_count, double* group_state, uint32_t* group_count, double* ty,
                     int64_t* nonfinite);
/* Held-out rows and new groups (csrc/predict.h; no counterpart in the reference): the family's
 * density and draw on a table other than the training table, from the sample store.
 * nmc_predict_set: new_obs[n_new][n_fields] in the family's row layout (n_fields = the
 * context's width) and new_group[n_new]: a code g >= 0 is training group g, -(k + 1) is new
 * group k, 0 <= k < n_new_groups (partial pooling only), whose values at recorded row r and
 * chain c are mu_q + sqrt(sigma2_q) z from that sample's hyper columns, z the normal of the
 * Philox block with counter (r, k, q, purpose 5) and key (chain_base + c, seed); NaN where
 * sigma2_q is not > 0 or not finite.  The call copies the table, cuts it into tiles (at every
 * change of the code and every 8 rows) and replaces the table in place; new_obs = NULL with
 * n_new = 0 clears it; nmc_destroy frees it.  -1 and nothing changed: another width, a code
 * >= G or < -n_new_groups, a new group without partial pooling, n_new >= 2^32.
 * A row has a held-out response when all its response fields (nmc_ppc_nresp's) are finite; a
 * draw y_rep of response field j of new row i is the family's predict() on the block with
 * counter (r, i, j, purpose 6): it depends on (seed, global chain, r, i, j) and theta alone.
 * nmc_predict_draws: yrep[C][n_rows][n_new][nresp], ll[C][n_rows][n_new] (the log density of
 * row i at the sample's values) and theta_new[C][n_rows][n_new_groups][P]; each may be NULL
 * (at most 65535 rows per call).  yrep needs a family that can draw.
 * nmc_predict_partials: over recorded rows [row_begin, row_begin + n_rows) and local chains
 * [0, n_valid), per chain block (CB = ceil(C / 64)):
 *   dens[CB][2][n_new]            m = max ll, s = sum exp(ll - m)  (nmc_waic_partials' words)
 *   state[CB][3][nresp][n_new]    n, Welford's mean and M2 of y_rep over the samples
 *   count[CB][2][nresp][n_new]    lt = #{y_rep < y}, eq = #{y_rep == y}  (0 without a response)
 * merged in the fixed order csrc/predict.h documents; nestmc/predict.py merges the blocks and
 * finishes.  dens may be NULL, and state with count (a family that cannot draw has the
 * density only; asking it for state is refused as nmc_ppc_draws refuses).  Chains >= n_valid
 * enter as the identity.  n_rows < 2^26 (uint32 counts); other argument errors as
 * nmc_waic_partials.  *nonfinite_draws: draws that were not finite; *nonfinite_ll: ll terms
 * that were not finite at rows WITH a response.  Event slots 16 and 17 bracket the kernel. */
int nmc_predict_set(nmc_ctx* ctx, const double* new_obs, int64_t n_new, int n_fields,
                    const int32_t* new_group, int n_new_groups);
int nmc_predict_draws(nmc_ctx* ctx, int row_begin, int n_rows, double* yrep, double* ll,
                      double* theta_new);
int nmc_predict_partials(nmc_ctx* ctx, int row_begin, int n_rows, int n_valid, double* dens,
                         double* state, uint32_t* count, int64_t* nonfinite_draws,
                         int64_t* nonfinite_ll);
/* The convergence diagnostic's partial sums (Diagnostic, sampleDiagnosis.py:136-255: the split
 * of every chain into two halves :136-155, the means and variances of :158-187, the variogram
 * of :189-194) over recorded rows [row_begin, row_begin + n_rows) and local chains
 * [0, n_valid), on the device from the sample store as it lies; n = n_rows / 2, half 0 = the
 * window's rows [0, n), half 1 = rows [n, 2n).  Per (column k, chain c, half h), x the n values:
 *   mean[k][h][c] = (x[0] + ... + x[n-1]) / n,  m2[k][h][c] = sum_q (x[q] - mean)^2,
 *   S[t] = sum_{q < n-t} (x[q+t] - x[q])^2,  S[0] = 0          (all sums in row order)
 * vg[CB][cols][n], CB = ceil(C / 64): per chain block, column and lag the block's 128 values
 * S[t] added as a balanced tree over (chain, half), half minor (csrc/conv.h); not divided.
 * Chains >= n_valid (a rank's padding) add +0.0 and their mean / m2 entries are +0.0.
 * nestmc/convergence.py merges the blocks and finishes.  n_rows even and >= 4, the rows
 * inside the schedule's, 1 <= n_valid <= C, else -1.  Event slots 12 and 13 bracket the
 * kernel (nmc_waic_partials uses 14 and 15).                                      */
int nmc_conv_partials(nmc_ctx* ctx, int row_begin, int n_rows, int n_valid, double* mean,
                      double* m2, double* vg);
/* The order statistics of every column of the sample store (the median and HDI of
 * Diagnostic._computeMedianAndHdi, sampleDiagnosis.py:419-427, and computeHpdInterval
 * :766-776) over recorded rows [row_begin, row_begin + n_rows) and local chains [0, n_valid),
 * on the device from the store as it lies: a column's N = n_rows * n_valid values are sorted
 * (csrc/sortcol.h: tiles of 4096 keys in LDS, then merge passes) by the key that orders a
 * double's bits like the number (-inf < ... < -0.0 < +0.0 < ... < +inf < +NaN), s the result:
 *   at_ranks[col][r] = s[ranks[r]]                      (n_ranks may be 0, at_ranks then unused)
 *   hdi[col]         = (s[i], s[i + gap]), hdi_at[col] = i, the first i in [0, N - gap) that
 *                      minimises s[i + gap] - s[i]      (one fp64 subtraction per i)
 *   nonfinite[col]   = the column's values that are NaN or +-inf; such a column gets NaN for
 *                      every statistic and hdi_at = -1
 *   sorted           = NULL, or [cols][N]: every column in key order
 * All of it depends on the multiset of a column's values alone.  Columns are sorted in batches
 * whose temporary buffers (2 * batch * N * 8 bytes, allocated and freed by the call) fit
 * 1 GiB; col_batch > 0 sets the columns per batch.  The rows inside the schedule's,
 * 1 <= n_valid <= C, 2 <= N < 2^31, 1 <= gap <= N - 1, 0 <= ranks[r] <= N - 1, else -1.
 * Event slots 10 and 11 bracket the kernels.                                       */
int nmc_summary(nmc_ctx* ctx, int row_begin, int n_rows, int n_valid, int64_t gap,
                const int64_t* ranks, int n_ranks, int col_batch, double* at_ranks, double* hdi,
                int64_t* hdi_at, int64_t* nonfinite, double* sorted);
/* The same over a host array x[rows][cols][C] in the store's layout (all of its rows), copied
 * to `device`; needs no context.                                                      */
int nmc_summary_of(int device, const double* x, int rows, int cols, int C, int n_valid,
                   int64_t gap, const int64_t* ranks, int n_ranks, int col_batch,
                   double* at_ranks, double* hdi, int64_t* hdi_at, int64_t* nonfinite,
                   double* sorted);
/* PSIS-LOO (Vehtari, Gelman, Gabry 2017) of every observation over recorded rows [row_begin,
 * row_begin + n_rows) and local chains [0, n_valid), on the device from the sample store; the
 * definitions are nestmc/loo.py's docstring.  Observations go in batches: the batch's
 * per-observation log-likelihoods (the values of nmc_obs_ll_rows, bit for bit) are written in
 * the store's layout [n_rows][batch][C] (nmc_k_loo_ll), their columns sorted by the kernels of
 * nmc_summary, and one workgroup per observation fits and smooths the tail of its sorted
 * column (csrc/psis.h).  Per observation i:
 *   elpd_i[i], lppd_i[i]  the leave-one-out and the plain log pointwise predictive density
 *   k_i[i]                the Pareto shape estimate; +inf when the tail has 4 values or fewer
 *   n_tail_i[i]           the values strictly above the cutoff, <= M = ceil(min(S/5, 3 sqrt(S)))
 *   nonfinite_i[i]        its log-likelihoods that are NaN or +-inf; such an observation gets
 *                         NaN for elpd, lppd and k and n_tail 0
 * with S = n_rows * n_valid.  All of it depends on the multiset of an observation's values
 * alone: batches and row ranges change no bit.  The three temporary buffers of a batch (the
 * log-likelihoods and two key buffers, allocated and freed by the call) fit 1 GiB; obs_batch > 0
 * sets the observations per batch.  The rows inside the schedule's, 1 <= n_valid <= C,
 * 2 <= S < 2^31, M <= 8191 (S up to about 7.4e6), obs_batch >= 0, else -1 and nothing is
 * written.  Event slots 8 and 9 bracket the kernels.                                   */
int nmc_loo(nmc_ctx* ctx, int row_begin, int n_rows, int n_valid, int obs_batch,
            double* elpd_i, double* lppd_i, double* k_i, int32_t* n_tail_i,
            int64_t* nonfinite_i);
/* The same sort and fit over a host array ll[rows][n_obs][C] in the store's layout (all of
 * its rows), copied to `device`; needs no context.                                     */
int nmc_psis_of(int device, const double* ll, int rows, int64_t n_obs, int C, int n_valid,
                int obs_batch, double* elpd_i, double* lppd_i, double* k_i, int32_t* n_tail_i,
                int64_t* nonfinite_i);
/* LOO-PIT and the leave-one-out predictive moments (BDA3 section 7; arviz loo_pit, loo E_loo;
 * the definitions are nestmc/loopit.py's docstring): nmc_loo's pass, whose five outputs it
 * fills with nmc_loo's bits, and on the same sort of every batch, per response field j, the
 * replicates of the batch in the store's layout beside the log-likelihoods (nmc_k_loo_yrep:
 * nmc_ppc_draws' values, bit for bit) and one workgroup per observation that weights them
 * (nmc_k_psis_expect, csrc/psis.h).  With W_s = exp(lw_s - D) the PSIS weight of sample s,
 * tied tail samples sharing the mean weight of their places, and Z = sum_s W_s:
 *   ess_i[i]                    Z^2 / sum_s W_s^2
 *   wlt[i][j], weq[i][j]        sum_s W_s [y_rep_s < y] / Z and sum_s W_s [y_rep_s == y] / Z
 *   mean[i][j], var[i][j]       sum_s W_s y_rep_s / Z and sum_s W_s (y_rep_s - mean)^2 / Z
 *   nonfinite_draws[i][j]       the replicates that are NaN or +-inf; such a field gets NaN
 *                               for wlt, weq, mean and var
 * ([n_obs][NRESP] arrays, NRESP of nmc_ppc_nresp).  An observation with log-likelihoods that
 * are not finite gets NaN everywhere.  Every sum has a fixed order: the bits depend on
 * (n_rows, n_valid) and the tail's length alone, not on batches or row ranges; the replicates
 * of tail samples with one log-likelihood enter in the order of their own values, so which of
 * the tied samples carries which replicate changes no bit.  The batch's two value buffers, two
 * key buffers, smoothed tails and tie scratch fit 1 GiB.  Argument errors are nmc_loo's;
 * a family that cannot draw (nmc_ppc_nresp 0) and n_obs >= 2^32 also give -1.  Event slots 8
 * and 9 bracket the kernels.                                                             */
int nmc_loo_pit(nmc_ctx* ctx, int row_begin, int n_rows, int n_valid, int obs_batch,
                double* elpd_i, double* lppd_i, double* k_i, int32_t* n_tail_i,
                int64_t* nonfinite_i, double* ess_i, double* wlt, double* weq, double* mean,
                double* var, int64_t* nonfinite_draws);
/* The same over host arrays ll[rows][n_obs][C] and yrep[rows][n_obs][C] in the store's layout
 * (all of their rows) and the observed values y[n_obs] of one response field (NRESP = 1),
 * copied to `device`; needs no context.                                                  */
int nmc_psis_expect_of(int device, const double* ll, const double* yrep, const double* y,
                       int rows, int64_t n_obs, int C, int n_valid, int obs_batch,
                       double* elpd_i, double* lppd_i, double* k_i, int32_t* n_tail_i,
                       int64_t* nonfinite_i, double* ess_i, double* wlt, double* weq,
                       double* mean, double* var, int64_t* nonfinite_draws);
/* The rank-normalised convergence diagnostics' partial sums (Vehtari, Gelman, Simpson,
 * Carpenter, Buerkner 2021; the definitions are nestmc/rankdiag.py's docstring) over recorded
 * rows [row_begin, row_begin + n_rows) and local chains [0, n_valid), on the device from the
 * sample store.  A column's N = n_rows * n_valid values are sorted (the kernels of
 * nmc_summary); every value x becomes four derived values, in this order (csrc/rankz.h):
 *   z    the normal score of its average rank r: ndtri((r - 0.375) / (N + 0.25)), ties
 *        numeric (-0.0 ties +0.0), 2 r = #{< x} + #{<= x} + 1
 *   zf   the same of zeta = |x - med| among the column's zeta, med = (s[N/2-1] + s[N/2]) / 2.0
 *   I05  1.0 if #{< x} <= (N - 1) / 20, else 0.0          (x <= the lower 5 % order statistic)
 *   I95  1.0 if #{< x} <= 19 (N - 1) / 20, else 0.0
 * written in the store's layout, and each derived column gets exactly nmc_conv_partials' sums
 * (the same kernel): vg[4][CB][cols][n], mean[4][cols][2][C], m2[4][cols][2][C], n = n_rows / 2.
 * nonfinite[col]: the column's values that are NaN or +-inf; such a column's derived values
 * are all NaN.  nestmc/rankdiag.py finishes.  Columns go in batches whose temporary buffers
 * (two key buffers and the derived values, 16 N + 32 n_rows C bytes a column, allocated and
 * freed by the call) fit 1 GiB; col_batch > 0 sets the columns per batch, and no bit depends
 * on it.  n_rows even and >= 4, the rows inside the schedule's, 1 <= n_valid <= C, N < 2^31,
 * col_batch >= 0, else -1 and nothing is written.  Event slots 6 and 7 bracket the kernels
 * (with several batches also the earlier batches' copies).                              */
int nmc_rank_partials(nmc_ctx* ctx, int row_begin, int n_rows, int n_valid, int col_batch,
                      double* vg, double* mean, double* m2, int64_t* nonfinite);
/* The same over a host array x[rows][cols][C] in the store's layout (all of its rows), copied
 * to `device`; needs no context.  Three more outputs, each may be NULL:
 *   derived[4][rows][cols][C]     the derived values (z, zf, I05, I95); chains >= n_valid +0.0
 *   twice_rank[2][rows][cols][C]  #{<} + #{<=} + 1 of x among the x and of zeta among the
 *                                 zeta; 0 for chains >= n_valid and for a column counted in
 *                                 nonfinite
 *   zeta[rows][cols][C]           |x - med| as pass 1 wrote it (pass 2 replaces it by zf);
 *                                 chains >= n_valid +0.0, NaN for a column counted in nonfinite */
int nmc_rank_partials_of(int device, const double* x, int rows, int cols, int C, int n_valid,
                         int col_batch, double* vg, double* mean, double* m2,
                         int64_t* nonfinite, double* derived, int64_t* twice_rank,
                         double* zeta);
/* Group rankings and pairwise comparisons of a parameter's G group values (the league table
 * of a multilevel model, Goldstein and Spiegelhalter 1996; the definitions are
 * nestmc/groupcmp.py's docstring) over recorded rows [row_begin, row_begin + n_rows) and local
 * chains [0, n_valid), on the device from the sample store as it lies: the values are the
 * recorded ones of posteriorSampling.py:640-659, 771-787; the counts themselves have no
 * counterpart in the reference.  Per sample s = (row, chain) and parameter p, theta_g is store
 * column p (G + pc) + pc + g (pc = 2 under partial pooling: _mu and _sigma2 are skipped);
 * comparisons are fp64 comparisons (NaN false both ways, -0.0 == +0.0):
 *   hist[p][g][r] = #{s : #{h : theta_h < theta_g} = r}      (0-based strict rank)
 *   wins[p][g][h] = #{s : theta_g > theta_h}
 *   nonfinite[p]  = #{(s, g) : theta_g is NaN or +-inf}      (callers treat a count as an error)
 * Integer counts only (csrc/grouporder.h): the words do not depend on the row window's
 * slicing, and several engines' or ranks' counts add.  The call allocates and frees the two
 * device count arrays (2 P G^2 4 bytes).  G >= 2, n_rows >= 1 and the rows inside the
 * schedule's, 1 <= n_valid <= C, n_rows * n_valid < 2^31, else -1 and nothing is written.
 * Event slots 4 and 5 bracket the kernel.                                              */
int nmc_group_order(nmc_ctx* ctx, int row_begin, int n_rows, int n_valid, uint32_t* hist,
                    uint32_t* wins, int64_t* nonfinite);
/* The same over a host array x[rows][cols][C] in the store's layout (all of its rows),
 * cols = P * (G + 2 * partial), partial 0 or 1, copied to `device`; needs no context.   */
int nmc_group_order_of(int device, const double* x, int rows, int P, int G, int partial, int C,
                       int n_valid, uint32_t* hist, uint32_t* wins, int64_t* nonfinite);
/* Posterior comoments of all store columns -- what the covariance and correlation matrix of
 * the joint posterior are made of (the definitions are nestmc/correlation.py's docstring) --
 * over recorded rows [row_begin, row_begin + n_rows) and local chains [0, n_valid), on the
 * device from the sample store as it lies: the values are the recorded ones of
 * posteriorSampling.py:640-659, 771-787; the reference only plots random pairs
 * (sampleDiagnosis.py:690-725).  Samples s = (row, chain), S = n_rows * n_valid; columns k in
 * header order:
 *   mean[k]      = (sum_s x_k) / S, the sum in one fixed order (csrc/comoment.h)
 *   minmax[0][k] = min_s x_k, minmax[1][k] = max_s x_k      (fp64 comparison)
 *   nonfinite[k] = #{s : x_k is NaN or +-inf}       (callers treat a count as an error)
 *   M[k][l]      = sum_s fl(x_k - mean[k]) fl(x_l - mean[l])
 * in fp64 with fused multiply-adds (v_mfma_f64_16x16x4_f64) and no floating-point atomics:
 * the partial tiles of the K-slices are added in slice order, so the bits depend on the
 * window's values and on (n_rows, cols, C, n_valid) only -- not on where the window lies and
 * not on what chains >= n_valid hold (they add exactly +0.0).  M[k][l] and M[l][k] are the
 * same bits.  A constant column (min == max) has +0.0 in its row and column of M, the diagonal
 * included; a column with a non-finite value has mean NaN and NaN in its row and column (also
 * where it meets a constant one), and no other entry changes.  The call allocates and frees M
 * and the partial tiles on the device (at most 1 GiB: cols <= 8192).  n_rows >= 1 and the rows
 * inside the schedule's, 1 <= n_valid <= C, 2 <= S < 2^31, else -1 and nothing is written.
 * Event slots 2 and 3 bracket the kernels.                                               */
int nmc_comoments(nmc_ctx* ctx, int row_begin, int n_rows, int n_valid, double* mean,
                  double* minmax /* [2][cols] */, double* M /* [cols][cols] */,
                  int64_t* nonfinite);
/* The same over a host array x[rows][cols][C] in the store's layout (all of its rows), copied
 * to `device`; needs no context.                                                         */
int nmc_comoments_of(int device, const double* x, int rows, int cols, int C, int n_valid,
                     double* mean, double* minmax, double* M, int64_t* nonfinite);

/* Timing on the context's stream (hipEvents). */
int nmc_event_record(nmc_ctx* ctx, int slot);                 /* slot 0..17 */
int nmc_event_elapsed(nmc_ctx* ctx, int slot_a, int slot_b, float* ms);
/* Bracket every step launch with events (adds a little overhead): per-kernel
 * average duration for the roofline; step_iters = iterations those launches ran. */
int nmc_set_kernel_timing(nmc_ctx* ctx, int enable);
int nmc_get_kernel_timing(nmc_ctx* ctx, double* step_ms_total, int64_t* step_launches,
                          int64_t* step_iters, double* hyper_ms_total, int64_t* hyper_launches);
/* Cap the iterations one persistent launch covers (0 = the variate chunk, the
 * default); e.g. equal-length launches for profiling.                           */
int nmc_set_launch_iters(nmc_ctx* ctx, int max_iters);
/* Launch geometry of the step kernel: waves per workgroup, chain blocks, whether one
 * resident launch runs a whole chunk of iterations (1) or one launch per iteration
 * (0), chains per workgroup (64, or 32 in the half-lane layout) and the kernel mode
 * (0 none/complete, 1 launch per iteration, 2 persistent sync, 3 LDS Gibbs payload,
 * 4 register Gibbs hand-off, 5 pair); chains_per_block and mode may be NULL.      */
int nmc_launch_config(nmc_ctx* ctx, int* waves_per_group, int* chain_blocks, int* persistent,
                      int* chains_per_block, int* mode);
/* Row split of none/complete pooling (CompletePooling._setGroupIndex :667-671 puts every
 * observation in ONE group): members = workgroups sharing each (chain block, group),
 * exchanging partial sums every step (1: no split); chain blocks per resident launch. */
int nmc_split_config(nmc_ctx* ctx, int* members, int* chain_blocks_per_launch);
/* The step kernel a run launches, e.g. "nmc_k_step<FamLinreg<2>, NMC_MODE_SYNC_REG>"
 * (NUL-terminated, truncated to cap bytes); for the profiles and the bench report.    */
int nmc_kernel_name(nmc_ctx* ctx, char* out, int cap);
/* Where a run's per-step variates come from: *in_kernel = 1 when the step kernel draws
 * them itself (no nmc_k_fill launch for them), 0 when nmc_k_fill writes them to a ring in
 * HBM first.  Both give the same bits (Parameter.propose :304-306, the accept draw :362). */
int nmc_variate_source(nmc_ctx* ctx, int* in_kernel);
/* Partial pooling over G > 128 groups runs the Gibbs update (HyperParameter.update
 * :463-498, once per chain block) as a kernel of its own beside the step kernel; when the
 * two did not run at the same time (a profiler or AMD_SERIALIZE_KERNEL serializes kernels)
 * the step kernel updated that launch's tasks itself, with the same results.  *out = the
 * (launch, chain block) pairs that did so since nmc_create (diagnostics and tests).     */
int nmc_gibbs_fallbacks(nmc_ctx* ctx, int64_t* out);
/* *separate = 1 when that Gibbs update runs as a kernel of its own (nmc_k_sweep_gibbs on a
 * second stream), 0 when its workgroups share nmc_k_sweep's grid or another kernel runs.  */
int nmc_gibbs_kernel(nmc_ctx* ctx, int* separate);

/* Sampler._printSample (:902-905) + _print (:933-936): append rows of local
 * chain c to a CSV file with the reference's "%i,%i,%f,..." formatting (and the
 * header line of :898-900 when header != NULL).  Host only; thread-safe.     */
int nmc_write_sample_csv(const char* path, int append, const char* header,
                         const double* samples, int n_chains, int c, int cols,
                         const int32_t* row_index, int n_rows, int chain_id);
/* _printLogLikelihood (:907-909): one "%f,..." line per row of ll[n_rows][n]. */
int nmc_write_ll_csv(const char* path, int append, const double* ll, int64_t n,
                     int n_rows);

/* Multi-GPU (replaces the process-per-chain fan-out, posteriorSampling.py:182-201):
 * RCCL communicator over xGMI and ONE gather of every rank's sample store.    */
/* Diagnostic._computeVariogram (sampleDiagnosis.py:189-194) for every lag: x = [K][m][n]
 * (K columns, m half-chains of n samples, host memory), out = [K][n] with
 * out[k][t] = sum_j sum_{i>=t} (x[k][j][i] - x[k][j][i-t])^2 / (m (n - t)), the
 * reference's summation order; runs on `device`; n <= 8192.                          */
int nmc_variogram(int device, const double* x, int K, int m, int n, double* out);

int nmc_comm_unique_id(unsigned char* out /* 128 bytes */);
int nmc_comm_init(void** comm, const unsigned char* id, int nranks, int rank, int device);
int nmc_comm_destroy(void* comm);
/* Rank count and this rank's id of a communicator (ncclCommCount/UserRank). */
int nmc_comm_size(void* comm, int* nranks, int* rank);
/* root receives [rank][row][col][C_local] (all ranks must have equal C_local) in
 * host_out, which must hold host_capacity >= nranks * rows * cols * C_local doubles
 * (ignored on the other ranks, which may pass NULL).                            */
int nmc_gather_samples(nmc_ctx* ctx, void* comm, int root, double* host_out,
                       int64_t host_capacity);

/* Verification hooks (tests only): device numerics on caller inputs.
 *   prior logpdf of family fam with params[8] at xs[n]   (scipy .logpdf)
 *   gammainccinv(a[i], q[i]) with lga[i] = gammaln(a[i]) (scipy.special)
 *   per counter ctr5[i] = (iter, group, param, purpose, chain): out4[i] =
 *   {Box-Muller normal, uniform a, uniform b, Gamma(gamma_shape) draw}.       */
int nmc_debug_prior_logpdf(int fam, const double* params8, const double* xs, int n,
                           double* out);
int nmc_debug_igamci(const double* a, const double* q, const double* lga, int n,
                     double* out);
int nmc_debug_rng(const uint32_t* ctr5, int n, uint32_t seed, double gamma_shape,
                  double* out4);
/* numpy.logaddexp(0, x[i]) as the likelihood kernels evaluate it (csrc/softplus.h): on the
 * host (on_device = 0, no GPU needed) or by a device kernel (on_device = 1); the two are
 * bit-identical by construction (IEEE add / mul / fma / div, rint, ldexp only).          */
int nmc_debug_softplus(const double* x, int n, double* out, int on_device);
/* The variate math of csrc/rng.h on caller inputs, on the host (on_device = 0, no GPU needed)
 * or by a device kernel: which = 0 nmc_log_unit(a[i]), 1 nmc_cos2pi(a[i]), 2
 * nmc_box_muller(a[i], b[i]) (b is read for which = 2 only, but must hold n doubles).  IEEE
 * add / mul / fma / div, sqrt and frexp only, so the two are bit-identical.                */
int nmc_debug_varmath(int which, const double* a, const double* b, int n, double* out,
                      int on_device);
/* nmc_debug_igamci's host form (no GPU needed): the same code with libm's log / exp / pow /
 * lgamma, so it agrees with the device to rounding, not bit for bit.                       */
int nmc_debug_igamci_host(const double* a, const double* q, const double* lga, int n,
                          double* out);
/* The recording schedule without a context or a GPU.  nmc_debug_schedule_rows: the sample rows
 * nmc_set_schedule allocates for (n_iter, burn, thin).  nmc_debug_record_rows_host: out[i] =
 * the row iteration iter[i] is recorded in under (burn, thin, n_rows), -1 for none -- the
 * kernels' own function (csrc/dev.h nmc_record_row) compiled for the host.                */
int nmc_debug_schedule_rows(int n_iter, int burn, int thin, int* rows);
int nmc_debug_record_rows_host(int burn, int thin, int n_rows, const int* iter, int n,
                               int* out);
/* The inverse of nmc_get_samples: writes recorded rows [row_begin, row_begin+n_rows) of the
 * device sample store from in[row][col][C] (the store as set_schedule sized it; no sampling
 * needed), so that the store's consumers -- nmc_obs_ll_rows, nmc_write_ll_csvs,
 * nmc_waic_partials, nmc_ppc_partials, nmc_loo, nmc_conv_partials, nmc_summary,
 * nmc_rank_partials -- can be run
 * on rows a sampler would not produce.  Nothing in the product path calls it.           */
int nmc_debug_set_samples(nmc_ctx* ctx, int row_begin, int n_rows, const double* in);
/* The plan nmc_run works to, for tests that run with variate buffers shorter than the run
 * (NMC_VARIATE_BYTES).  nmc_debug_variate_plan (after nmc_set_schedule): vcap, the iterations
 * one variate buffer holds; chunk, the iterations of one step launch (nmc_set_launch_iters,
 * at most vcap); counter_wrap, the limit in force below.  Any output may be NULL.
 * nmc_debug_set_counter_wrap: the counters that run on across launches (publishes, hyper-ready
 * counts, row-split arrivals) are zeroed before groups * iterations or members * steps since
 * the last reset would reach the limit, 2^31 by default; a lower limit (1 .. 2^31, else -1)
 * makes that reset run within a short run.  It changes no result.
 * nmc_debug_counter_resets: the resets so far.  Nothing in the product path calls these.  */
int nmc_debug_variate_plan(nmc_ctx* ctx, int* vcap, int* chunk, int64_t* counter_wrap);
int nmc_debug_set_counter_wrap(nmc_ctx* ctx, int64_t limit);
int nmc_debug_counter_resets(nmc_ctx* ctx, int64_t* resets);
/* Diagnostic build only (make stamps -> libnestmc_stamps.so): shader-clock phase
 * stamps of the step kernel, [2 blocks][2 waves][8 iterations][16 slots]; n > 0
 * arms (zeroes) the buffer, out != NULL copies it back.  Error in the shipped lib. */
int nmc_debug_stamps(nmc_ctx* ctx, int n, uint64_t* out);

#ifdef __cplusplus
}
#endif
#endif /* NESTMC_H */
