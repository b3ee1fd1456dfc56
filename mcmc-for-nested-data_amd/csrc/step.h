// step.h -- the step kernel nmc_k_run (its launch modes NMC_MODE_*) with the pieces of a
// Metropolis step it shares with nmc_k_sweep and nmc_k_fill: the step's variates
// (nmc_step_variate) and Parameter.tune (nmc_tune).
#pragma once

#include "families.h"
#include "rng.h"
#include "special.h"
#include "dev.h"
#include "stamps.h"
#include "mem.h"
#include "rows.h"
#include "gibbs.h"

// {z, log u} of step (it, p) of group g, chain c (the chain's global id is chain_base +
// c): Philox4x32-10 normal and log of a 53-bit uniform, or the replayed reference
// variates.  nmc_k_fill and the step kernels' variate jobs both call this, so a step's variates
// never depend on which kernel drew them.
enum { NMC_RNG_MODE_REPLAY = 1 };   // (include/nestmc.h NMC_RNG_REPLAY)
#ifndef NMC_ZIN_BUILD
#define NMC_ZIN_BUILD 0
#endif
__device__ __forceinline__ void nmc_step_variate(const Dev& d, int it, int p, int g, int c,
                                                 double& z, double& lu) {
  if (d.rng_mode == NMC_RNG_MODE_REPLAY) {
    const size_t k = (((size_t)it * d.P + p) * d.G + g) * d.C + c;
    z = it < d.replay_n ? d.rz[k] : nmc_nan();
    lu = it < d.replay_n ? log(d.ru[k]) : nmc_nan();
  } else {
    const uint32_t ch = (uint32_t)(d.chain_base + c);
    z = nmc_normal(it, g, p, NMC_PURPOSE_PROPOSAL, ch, d.seed);
    lu = nmc_log_unit(nmc_uniform2(it, g, p, NMC_PURPOSE_ACCEPT, ch, d.seed).a);
  }
}

// Parameter.tune (posteriorSampling.py:385-437)
__device__ __forceinline__ void nmc_tune(double& s, double& na, double& nr) {
  const double tot = na + nr;
  if (!(tot > 0.0)) return;
  const double rate = na / tot;
  double f = 1.0;
  if (rate < 0.001) f = 0.1;
  else if (rate < 0.05) f = 0.5;
  else if (rate < 0.2) f = 0.9;
  else if (rate > 0.95) f = 10.0;
  else if (rate > 0.75) f = 2.0;
  else if (rate > 0.5) f = 1.1;
  const double ns = s * f;
  na = 0.0;
  nr = 0.0;
  if (ns != 0.0) s = ns;
}

// ---------------------------------------------------------------------------
// K_run: iterations [i0, i1) for every (chain, group); grid = CB*G workgroups of
// 64*W threads (W <= 8); dynamic LDS = nmc_lds(...).total columns.
// Wave roles:
//   wave 0            control: proposal priors, Metropolis decision, tuning, state,
//                     sample/trace stores, variate DMA, publishing, and (persistent
//                     payload-in-LDS mode, P >= 2) the Gibbs payload copy;
//   wave 1 (NAUX = 1) Gibbs update (persistent payload-in-LDS mode): the task the
//                     control wave copied at the previous step (P == 1: poll, copy
//                     and update in the same step);
//   every wave        once its own work is done, takes likelihood row tiles from an
//                     LDS counter until none is left, so a wave that shares its SIMD
//                     with a busy control or Gibbs wave simply takes fewer tiles.
// The control wave adds the tile partials in a fixed order (nmc_tiles): the sums do
// not depend on which wave took which tile.
//   flags & NMC_RUN_HYPER_LOAD: the hyper-parameters after iteration i0-1 are in
//     global memory (chunk start / initial state); otherwise (launch per iteration)
//     they are recomputed from vb[(i0-1)&1] at step 0 of i0.
//   MODE SYNC / SYNC_LDS (partial, persistent): publish every iteration, wait on
//     the chain block's counter before each Gibbs update, close with the update
//     after i1-1 (workgroups of group 0, which also record it).
// ---------------------------------------------------------------------------
// MODE: how the partial-pooling Gibbs update gets the chain block's values.
enum { NMC_MODE_NOPOOL = 0,      // none/complete pooling: no coupling
       NMC_MODE_LAUNCH = 1,      // one launch per iteration, plain loads after the boundary
       NMC_MODE_SYNC = 2,        // persistent, sc1 loads after the barrier
       NMC_MODE_SYNC_LDS = 3,    // persistent, the Gibbs wave works on an LDS copy
       NMC_MODE_SYNC_REG = 4,    // persistent, G <= 64: the Gibbs wave fetches the task's
                                 // values straight into registers and updates in one step
       NMC_MODE_SYNC_OWN = 5,    // nmc_k_sweep (G > 128): Gibbs workgroups update each task
       NMC_MODE_HALF = 6 };      // none/complete pooling, 32 chains per workgroup: lanes l
                                 // and l + 32 hold chain l, on the two row parities
// RL: the groups' rows are staged in LDS for the launch (d.rows_lds) -- a template
// parameter so each instance holds only its own row loop (the LDS-DMA staged loop's
// registers raised the rows-in-LDS kernel's pressure: ~5 % of its time at cfg 3)
// RES: the resident launch (Dev.rcmd): iterations [i0, i1) are the first call; later calls
// extend the end (res_gate below).
template <class Fam, int MODE, bool RL = true, bool RES = false>
__global__ void __launch_bounds__(NMC_RUN_THREADS)
nmc_k_run(Dev d_arg, Fam fam, const double* __restrict__ obs, int i0, int i1, int flags) {
  (void)d_arg;   // (read through nmc_kdev(): the same bytes)
  const Dev* dP = nmc_kdev();
#define d (*dP)
  constexpr bool PARTIAL = MODE != NMC_MODE_NOPOOL && MODE != NMC_MODE_HALF;
  // half layout: the grid of 64-chain blocks would leave CUs idle (none/complete pooling,
  // RB * G * 2 <= CUs): 32 chains per workgroup, twice the workgroups, each lane pair
  // (l, l + 32) one chain with the paired row loop's two row parities -- the same rows,
  // accumulators and order as the 64-chain layout, so every sum is bit-identical
  constexpr bool HALF = MODE == NMC_MODE_HALF;
  NMC_RUN_SL(0);
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int W = blockDim.x >> 6;
  const int P = d.P, G = d.G, C = d.C;
  const int b = blockIdx.x;
  const int S = d.S;
  // the two Dev words the step's restart branches on, held for the launch (read after the
  // per-step argument laundering they cost a scalar round trip each before the first tile)
  const bool paired = d.paired;
  const bool quad = d.quad;
  const bool nstatic = d.nstatic;
  const bool ctlprio = !(d.noprio & 1);
  // The restart without gathers (quad rows, P >= 2): step gs + 1 proposes another parameter
  // than step gs decides, so the control wave forms its proposal a step ahead -- before
  // barrier A of step gs -- and leaves it in the LDS column NMC_CW_PN; after barrier B the tile
  // waves read the four chains of their quarter position straight from the parameters' columns
  // (lik_tiles) instead of forming the proposal again, each, and gathering it across lanes.
  // The first step of a call has no step before it and keeps the gathers.
  constexpr bool QF = Fam::ASM_ROWS && RL && !HALF;
  int qib0 = -1, qib = 0;   // the parameters that are the rows' intercept and slope
  if constexpr (QF) {
    fam.quad_params(qib0, qib);
    qib0 = __builtin_amdgcn_readfirstlane(qib0);   // (scalar: the row loop branches on it)
    qib = __builtin_amdgcn_readfirstlane(qib);
  }
  const bool fastq = QF && quad && d.P >= 2 && !(NMC_ZIN_BUILD && d.zin);
  const int mb = b % S;                           // row-split member (S == 1: 0)
  // (chain block, group) of unit u = b / S: chain-block-major, or (Dev.xpc > 0, S == 1) dealt
  // so that a chain block's workgroups share xpc XCDs -- blocks b and b + 8 share an XCD
  // (MI355X_MICROARCH.md, XCD placement) -- and its Gibbs payload is fetched into xpc L2s
  // rather than all 8.  Placement only: every (chain block, group) computes the same.
  const int u = b / S, xpc = d.xpc;
  const int g = xpc ? (u >> 3) * xpc + (u & 7) % xpc : u % G;
  const int cb = (xpc ? (u & 7) / xpc : u / G) + d.cb0;
  const int c = HALF ? cb * 32 + (lane & 31) : nmc_lane_chain(d, cb, lane);
  // member 0 writes the outputs (half layout: lanes 0-31)
  const bool live = nmc_lane_owns(d, c, lane) && mb == 0 && (!HALF || lane < 32);
  const bool g0w = g == 0 && mb == 0;   // writes the chain block's hyper-parameters
  const int cc = c < C ? c : C - 1;
  constexpr bool sync = MODE == NMC_MODE_SYNC || MODE == NMC_MODE_SYNC_LDS ||
                        MODE == NMC_MODE_SYNC_REG;
  static_assert(MODE != NMC_MODE_SYNC_OWN, "SYNC_OWN is nmc_k_sweep's mode");
  // Gibbs-wave modes: payload in LDS (two-stage pipeline) or in registers (one stage)
  constexpr bool hr = MODE == NMC_MODE_SYNC_REG;
  constexpr bool hl = MODE == NMC_MODE_SYNC_LDS || hr;
  // the Gibbs wave's task at global step gs is gs - lag; the register mode updates a
  // task two steps after its publication (P >= 2: the hand-off latency -- store drain,
  // counter add, poll -- is behind a whole step) and the priors that need it come from
  // the Gibbs wave when it lands in the step that uses it (P <= 2)
  const int lag = hr && P >= 2 ? 2 : 1;
  int ie = i1;            // end of the current call (RES: moved by the host's commands)
  int gfirst = i0 * P;    // first global step of the current call: the Gibbs tasks of the
                          // steps before it were closed by the launch before / the last gate
  // register mode: the task this workgroup closes at the end of a call ending at iend (-1:
  // none) -- tasks ge-lag .. ge-1, task ge-lag+j by the workgroup of group j
  auto close_of = [&](int iend) {
    const int ge = iend * P, k0 = ge - lag > gfirst ? ge - lag : gfirst;
    return hr && mb == 0 && k0 + g < ge ? k0 + g : -1;
  };
  // rows in LDS for the launch, or every wave's two staging buffers (nmc_ll_rows_staged)
  const int row_doubles = RL ? d.nmax * Fam::NFIELDS
                             : (Fam::NFIELDS <= 4 ? 0 : nmc_stage_doubles(Fam::NFIELDS, blockDim.x >> 6));
  const nmc_lds_layout L =
      nmc_lds(Fam::NACC, P, PARTIAL, d.nleaf, d.ntail, W, G, hl && !hr ? 1 : 0, row_doubles);
  double* th = lds + L.th * 64 + lane;            // th[p * 64]: this lane's chain, parameter p
  double* st = lds + L.st * 64 + lane;            // st[(k * P + p) * 64]
  double* hy = lds + L.hyp * 64 + lane;           // hy[(k * P + p) * 64]
  // tile counters, one per step parity (two 32-bit words in the flag column)
  unsigned* tcnt = (unsigned*)(lds + L.flag * 64 + 4);
  const int ngrp = (int)(d.off[g + 1] - d.off[g]);   // the group's rows (finish)
  int64_t r0;
  int nrow;                                           // this member's rows
  nmc_chunk(d.off[g], d.off[g + 1], mb, S, &r0, &nrow);
  const nmc_tiling TI = nmc_tiles(nrow, d.tile);
  const int nt = TI.nt;
  const double* grows = obs + r0 * Fam::NFIELDS;
  const double* glim = obs + d.off[g + 1] * Fam::NFIELDS;   // end of the group's rows
  const size_t PGC = (size_t)P * G * C;
  const size_t gc = (size_t)g * C + cc;
  const bool ctl = w == 0;
  const bool gw = hl && w == 1;                   // the Gibbs wave
  // latency-bound roles (control, Gibbs) issue ahead of the waves sharing their SIMD
  if (W > 1 && (ctl || gw) && !(d.noprio & 1)) __builtin_amdgcn_s_setprio(3);

  // ---- prologue: values and state -> LDS (parameter p by wave p % W) ----
  const double* vin = ((i0 - 1) & 1) ? d.vb1 : d.vb0;
  for (int p = w; p < P; p += W) {
    const size_t ip = (size_t)p * G * C + gc;
    th[p * 64] = vin[ip];
    st[(NMC_ST_S * P + p) * 64] = d.scale[ip];
    st[(NMC_ST_LP * P + p) * 64] = d.lp[ip];
    st[(NMC_ST_NA * P + p) * 64] = (double)d.nacc[ip];
    st[(NMC_ST_NR * P + p) * 64] = (double)d.nrej[ip];
    st[(NMC_ST_TA * P + p) * 64] = (double)d.tacc[ip];
    if (PARTIAL) {
      // hyper-parameters after iteration i0-1 (chunk start), or after i0-2 when this
      // launch recomputes the update after i0-1 at step 0 (launch per iteration): that
      // update is written to the other slot, so no workgroup of this launch can read it
      const size_t ho =
          nmc_hslot(d, (flags & NMC_RUN_HYPER_LOAD) ? i0 - 1 : i0 - 2) + (size_t)p * C + cc;
      const double s2 = d.s2[ho];
      hy[(NMC_HY_MU * P + p) * 64] = d.mu[ho];
      hy[(NMC_HY_SD * P + p) * 64] = d.hsd[ho];
      hy[(NMC_HY_LSD * P + p) * 64] = d.hlsd[ho];
      hy[(NMC_HY_S2 * P + p) * 64] = s2;
      hy[(NMC_HY_SDM * P + p) * 64] = sqrt(s2 / G);
      hy[(NMC_HY_ISD * P + p) * 64] = 1.0 / d.hsd[ho];
    }
  }
  const double gcst = fam.gconst((long)ngrp);   // per-group constant of finish_fast
  // the decision's family constants (finish_fast) and publish targets (this lane's value of
  // parameter 0 in vb0 / vb1), held in registers for the launch: read through the per-step
  // laundered argument pointer they are scalar round trips on the decision's critical path,
  // and barrier B's lgkmcnt(0) waits for them
  Fam fh = fam;   // (used for every family call below)
  fh.hold();
  double* pub0 = d.vb0 + gc;
  double* pub1 = d.vb1 + gc;
  asm volatile("" : "+v"(pub0), "+v"(pub1));
  double* lrows = lds + L.rows * 64;
  if constexpr (RL) {   // this group's rows -> LDS, once for the whole launch
    const int nd = nrow * Fam::NFIELDS;
    if (((r0 * Fam::NFIELDS) & 1) == 0) {
      // LDS-DMA in 16-byte pieces (global_load_lds_dwordx4: 1 KiB per wave-instruction, no
      // VGPRs), every piece in flight at once -- one memory round trip instead of one per
      // strided pass; an odd nd copies one double of slack (the carve has a column spare)
      const int npc = (nd + 1) / 2;
      for (int b0 = w * 64; b0 < npc; b0 += W * 64)
        if (b0 + lane < npc) nmc_dma16(grows + 2 * (b0 + lane), lrows + 2 * b0);
      nmc_drain_vm();   // (this wave's pieces have landed before the barrier below)
    } else {
      for (int i = threadIdx.x; i < nd; i += blockDim.x) lrows[i] = grows[i];
    }
  }
  auto zl_src = [&](int tn, int pn) -> const double* {
    return d.vzl + ((size_t)(tn - d.vbase) * PGC + (size_t)pn * G * C + gc) * 2;
  };
  // {z, log u} of step (tn, pn) -> LDS slot: LDS-DMA of the variates nmc_k_fill wrote
  auto put_zl = [&](int tn, int pn, int slot) {
    nmc_dma16(zl_src(tn, pn), lds + (L.zl + 2 * slot) * 64);
  };
  // ... or drawn here (d.zin, build option NMC_ZIN_BUILD=1): the calling wave's 64 lanes,
  // one chain each.  Measured slower: with the Philox / Box-Muller / log code inlined
  // into the tile loop the cfg-3 kernel spills twice the SGPRs (955 against 548) and runs
  // 11.7 against 7.5 us/iter (profiles/r03d_*), more than the fill it saves (0.53 us/iter
  // + 7 us per launch) -- so the shipped build keeps the fill.
  auto gen_zl = [&](int tn, int pn, int slot) {
#if NMC_ZIN_BUILD
    double z, lu;
    nmc_step_variate(d, tn, pn, g, cc, z, lu);
    lds[(L.zl + 2 * slot) * 64 + 2 * lane] = z;
    lds[(L.zl + 2 * slot) * 64 + 2 * lane + 1] = lu;
#else
    (void)tn; (void)pn; (void)slot;
#endif
  };
  double* cwv = lds + L.cw * 64 + lane;    // cwv[k * 64]: control-wave values across barriers
  if (ctl) {     // {z, log u} of the first step -> LDS slot of step i0*P
    if (NMC_ZIN_BUILD && d.zin)
      gen_zl(i0, 0, (i0 * P) & 1);
    else
      put_zl(i0, 0, (i0 * P) & 1);
    for (int j = 0; j < Fam::NACC; ++j)   // x + (-0.0) == x: the fixed slot sum
      for (int k = nt; k < NMC_NSLOT; ++k) lds[(L.part + j * NMC_NSLOT + k) * 64 + lane] = -0.0;
    nmc_drain_vm();
    lds[L.flag * 64 + lane] = 0.0;
    // both tile counters start at the static entries: waves 2 .. W-1 begin on entries
    // 0 .. W-3 by rank, without a take (every wave from 2 on runs lik_tiles in every mode)
    if (lane < 2) tcnt[lane] = (unsigned)(nstatic && W > 2 ? W - 2 : 0);
    if (RES && b == 0 && lane == 0) {   // the launch's own call taken now (its GPU span)
      const unsigned long long clk = __builtin_amdgcn_s_memrealtime();
      __hip_atomic_store(d.rack + 2, (unsigned)clk, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      __hip_atomic_store(d.rack + 3, (unsigned)(clk >> 32), __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_SYSTEM);
      nmc_drain_vm();
      __hip_atomic_store(d.rack, d.rseq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }
  __syncthreads();
  NMC_RUN_SL(1);

  bool ok = true;
  int pub_p = -1;     // control wave: parameter whose sc1 value store awaits its counter add
  int pend_p = -1, pend_t = 0;   // control wave: decided step whose state update is pending
  // Control-wave values, in registers across the step's barriers (the LDS queue is
  // saturated by the likelihood tiles while they are produced): the proposal, current
  // value, log accept uniform and priors of the step, both outcomes of its counters and
  // scale, the group log-likelihood of the current state, and the decided-but-pending
  // step's accept flag, log prior and log-likelihood.
  // (step-local ones are declared inside the step loop, so they are not live across the
  // Gibbs wave's bursts; the counters' outcomes wait in LDS)
  double c_LL = ctl ? d.ll[gc] : 0.0;
  bool q_acc = false;
  double q_plp = 0, q_pll = 0;
  // the rest of a decided step's state update (:369-383, :608-610): counters, log prior,
  // log-likelihood, sample and trace rows
  // its sample / trace stores wait in registers (w_*) until store_pending, which the control
  // wave issues after the step's publication count: the count's vmcnt drain then waits for
  // the publish store alone, not for stores issued just before it
  int w_q = -1, w_t = 0;
  bool w_acc = false;
  double w_v = 0, w_ll = 0;
  auto apply_pending = [&]() {
    const int q = pend_p, tq = pend_t;
    st[(NMC_ST_LP * P + q) * 64] = q_plp;
    st[(NMC_ST_NA * P + q) * 64] = cwv[(q_acc ? NMC_CW_NAA : NMC_CW_NAR) * 64];
    st[(NMC_ST_NR * P + q) * 64] = cwv[(q_acc ? NMC_CW_NRA : NMC_CW_NRR) * 64];
    st[(NMC_ST_TA * P + q) * 64] = cwv[NMC_CW_TA * 64] + (q_acc ? 1.0 : 0.0);
    if (q_acc) c_LL = q_pll;
    w_q = q;
    w_t = tq;
    w_v = th[q * 64];
    w_acc = q_acc;
    w_ll = q_pll;
    pend_p = -1;
  };
  auto store_pending = [&]() {
    if (w_q < 0) return;
    const int q = w_q, tq = w_t;
    if (live) {
      const int row = nmc_record_row(d, tq);
      if (row >= 0) {
        const int col = q * (G + (PARTIAL ? 2 : 0)) + (PARTIAL ? 2 : 0) + g;
        d.samples[((size_t)row * d.cols + col) * C + c] = w_v;
      }
      if (tq < d.trace_n) {
        const size_t it = (((size_t)tq * P + q) * G + g) * C + c;
        d.tflag[it] = w_acc ? 1 : 0;
        d.tllp[it] = w_ll;
      }
    }
    w_q = -1;
  };
  // ---- the likelihood of step (t, p)'s proposal (:615-635), tile by tile: the wave
  //      takes row tiles from the step's LDS counter until none is left; `between` runs
  //      after its first tile (the control wave's pre-barrier work) ----
  auto lik_tiles = [&](int t, int p, int sp, auto&& between) {
    if (w == 2) NMC_CS((t - i0) * P + p, 12);
    // the proposal was formed a step ahead (fastq above; not at the first step of a call)
    const bool ahead = fastq && t * P + p > gfirst;
    typename Fam::Reg reg;
    // quad rows: intercept and slope of the four chains of this lane's quarter position
    // (ahead: the first tile's row loop reads them, below)
    double qc[4], qd[4];
    double thp[Fam::MAXP];
    if (ahead) {
      // this lane's own chain, for the tiles' rows beyond the 16-row blocks: read only, prepared
      // behind the first tile's row loop
#pragma unroll
      for (int q = 0; q < Fam::MAXP; ++q)
        thp[q] = q < P ? (q == p ? cwv[NMC_CW_PN * 64] : th[q * 64]) : 0.0;
    } else {
      // every LDS read of the restart issued before any is used: one round trip (left alone
      // the scheduler waits for the values before it issues the scale and variate reads)
      const double sv = st[(NMC_ST_S * P + p) * 64], zv = lds[(L.zl + 2 * sp) * 64 + 2 * lane];
#pragma unroll
      for (int q = 0; q < Fam::MAXP; ++q) thp[q] = q < P ? th[q * 64] : 0.0;
      __builtin_amdgcn_sched_barrier(0);
      double vp = 0.0;   // thp[p] (a select per parameter: no dynamically indexed array)
#pragma unroll
      for (int q = 0; q < Fam::MAXP; ++q)
        if (q == p) vp = thp[q];
      const double prop = vp + (1.0 * sv) * zv;
#pragma unroll
      for (int q = 0; q < Fam::MAXP; ++q)
        if (q == p) thp[q] = prop;
      reg = fh.prepare(thp);
      if constexpr (QF) if (quad) {
        nmc_quarters(reg.b0, qc);
        nmc_quarters(reg.b[0], qd);
      }
    }
    // paired rows: the partner lane's (lane ^ 32) proposal parameters
    typename Fam::Reg preg{};   // (ahead: quad rows, no partner)
    if (!ahead) preg = reg;
    if constexpr (nmc_paired_rows_ok<Fam>() && !HALF) if (paired && !quad) {
      const bool hi = lane >= 32;
#pragma unroll
      for (int q = 0; q < Fam::MAXP; ++q) {
        const nmc_pair2 e = nmc_halves(thp[q]);
        thp[q] = hi ? e.lo : e.hi;
      }
      preg = fh.prepare(thp);
    }
    if (w == 2) NMC_CS((t - i0) * P + p, 13);
    // the next tile is requested before the current one is computed: the atomic's
    // return rides under the tile's own row reads.  Families with the hand-written row loops:
    // nmc_lds_grab, not behind this wave's outstanding global memory (its value only through
    // nmc_lds_grab_value).  The compiled row loops keep the compiler's atomic, whose return it
    // tracks through their reads: with nmc_lds_grab cfg 2 measured 2.7 % slower.
    auto grab = [&]() -> unsigned {
      if constexpr (Fam::ASM_ROWS) {
        return nmc_lds_grab(tcnt + sp);
      } else {
        unsigned k = 0;
        if (lane == 0)
          k = __hip_atomic_fetch_add(tcnt + sp, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        return k;
      }
    };
    auto grabbed = [&](unsigned r) -> int {
      if constexpr (Fam::ASM_ROWS) return nmc_lds_grab_value(r);
      else return (int)__builtin_amdgcn_readlane(r, 0);
    };
    // d.zin: queue entry 0 is the next step's variate job, entries 1.. the tiles
    const int tn = p + 1 < P ? t : t + 1, pn = p + 1 < P ? p + 1 : 0;
    const int zj = NMC_ZIN_BUILD && d.zin && tn < ie ? 1 : 0;
    // (waves 2.. start on their static entry: one LDS round trip off the step's restart)
    int kq = nstatic && w >= 2 ? (w - 2 < nt + zj ? w - 2 : nt + zj)
                               : grabbed(grab());
#ifdef NMC_CSTAMPS
    bool first_tile = true;
#endif
    // ahead: the wave's first tile apart -- its row loop reads qc / qd, this lane's quarter
    // position (lane & 15) of the intercept's and the slope's columns (NMC_CW_PN for the
    // proposed parameter), beside its first rows, for the step's later tiles too (zj == 0)
    if constexpr (QF) if (ahead && kq < nt) {
      const unsigned kn = grab();
#ifdef NMC_CSTAMPS
      NMC_CS((t - i0) * P + p, 16 + w);
      first_tile = false;
#endif
      const double* col = lds + (lane & 15);
      const int cc0 = qib0 == p ? L.cw + NMC_CW_PN : L.th + (qib0 < 0 ? 0 : qib0);
      const int cc1 = qib == p ? L.cw + NMC_CW_PN : L.th + qib;
      NMC_TILE_STAMP(kq, 0);
      double acc[Fam::NACC];
      nmc_ll_rows_lds_quad<Fam, true>(fh, reg, lrows + (size_t)TI.start(kq) * Fam::NFIELDS,
                                      TI.len(kq), acc, qc, qd, thp, qib0 >= 0,
                                      col + cc0 * 64, col + cc1 * 64);
      lds[(L.part + kq) * 64 + lane] = acc[0];
      NMC_TILE_STAMP(kq, 1);
      between();
      kq = grabbed(kn);
    }
    while (kq < nt + zj) {
      const unsigned kn = grab();
#ifdef NMC_CSTAMPS
      if (first_tile) NMC_CS((t - i0) * P + p, 16 + w);
      first_tile = false;
#endif
      if (kq < zj) {   // the variate job: {z, log u} of the next step -> the other slot
        gen_zl(tn, pn, sp ^ 1);
        kq = grabbed(kn);
        continue;
      }
      const int k = kq - zj;
      const int ra = TI.start(k);
      const int rn = TI.len(k);
      NMC_TILE_STAMP(k, 0);
      double acc[Fam::NACC];
      if constexpr (RL) {
        bool done = false;
        if constexpr (Fam::ASM_ROWS && !HALF) if (quad) {
          nmc_ll_rows_lds_quad(fh, reg, lrows + (size_t)ra * Fam::NFIELDS, rn, acc, qc, qd);
          done = true;
        }
        if constexpr (nmc_paired_rows_ok<Fam>()) if (!done && (HALF || paired)) {
          // two chains per lane, row pairs split by lane half (half layout: one chain per
          // lane pair, each lane its row parity)
          nmc_ll_rows_lds<Fam, true, HALF>(fh, reg, lrows + (size_t)ra * Fam::NFIELDS, rn,
                                           acc, &preg);
          done = true;
        }
        if (!done)   // wave-uniform LDS address: broadcast ds_reads, pipelined
          nmc_ll_rows_lds(fh, reg, lrows + (size_t)ra * Fam::NFIELDS, rn, acc);
      } else if constexpr (Fam::NFIELDS <= 4) {
        // rows beyond LDS, narrow rows: blocks of >= 4 rows per scalar load run ahead in
        // the scalar cache (the staged loop measured 1.7x slower for 2-field rows)
        nmc_ll_rows(fh, reg, grows + (size_t)ra * Fam::NFIELDS, rn, acc);
      } else {          // wide rows beyond LDS: staged per wave by LDS-DMA, two chunks deep
        nmc_ll_rows_staged(fh, reg, grows + (size_t)ra * Fam::NFIELDS, rn, glim,
                           lrows + (size_t)w * 2 * nmc_stage_buf(Fam::NFIELDS), acc);
      }
#pragma unroll
      for (int j = 0; j < Fam::NACC; ++j) lds[(L.part + j * NMC_NSLOT + k) * 64 + lane] = acc[j];
      NMC_TILE_STAMP(k, 1);
      between();
      kq = grabbed(kn);
    }
  };
  // ---- register mode: the Gibbs wave runs its own loop (gibbs_step below), so its 64-value
  //      payload never shares registers with the control code, and it meets the other
  //      waves at the same two barriers ----
  // the register hand-off's task of step (t, p): task k = gs - lag = (kt, kq) -- poll, fetch,
  // update, and (P <= 2) this step's priors; lane 0 leaves the verdict in the flag word
  auto gibbs_step = [&](int t, int p) {
    const int gs = t * P + p;
    if (gs - lag < gfirst) return;
    // task gs - lag as (kt, kq) without dividing by P (lag <= P)
    const int kq = p >= lag ? p - lag : p - lag + P, kt = p >= lag ? t : t - 1;
    NMC_CS(gs - i0 * P, 24);
    const bool r = nmc_poll_published(d, cb, kq, (unsigned)G * (unsigned)(kt - i0 + 1));
    NMC_CS(gs - i0 * P, 25);
    if (lane == 0)
      __hip_atomic_store(lds + L.flag * 64 + 1, r ? 2.0 * ((double)gs + 1) : -2.0 * ((double)gs + 1),
                         __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (p == 0) NMC_STAMP_AUX(t, 13);
    if (r) {
      // keep the payload loads below the poll (no instruction: wavefront scope)
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#ifdef NMC_CSTAMPS
      {   // (diagnostics: the fetch and the update stamped apart)
        double xv[64], fz, fx;
        nmc_hyper_fetch_reg(d, kt, kq, cc, xv, fz, fx);
        NMC_CS(gs - i0 * P, 26);
        nmc_hyper_compute_reg(d, cb, kt, kq, lds, L.hyp, g0w, fz, fx, xv);
        NMC_CS(gs - i0 * P, 27);
      }
#else
      nmc_hyper_update_reg(d, cb, kt, kq, cc, lds, L.hyp, g0w);
#endif
      if (p == 0) NMC_STAMP_AUX(t, 15);
      if (P <= 2) {   // the update lands in the step that needs it: this step's priors
        const int sp = gs & 1;
        const double v = th[p * 64];
        const double prop = v + (1.0 * st[(NMC_ST_S * P + p) * 64]) *
                                    lds[(L.zl + 2 * sp) * 64 + 2 * lane];
        const double m = hy[(NMC_HY_MU * P + p) * 64], sd = hy[(NMC_HY_SD * P + p) * 64];
        const double lsd = hy[(NMC_HY_LSD * P + p) * 64], isd = hy[(NMC_HY_ISD * P + p) * 64];
        cwv[NMC_CW_LPC * 64] =
            t > 0 ? nmc_norm_logpdf_r(v, m, sd, isd, lsd) : st[(NMC_ST_LP * P + p) * 64];
        cwv[NMC_CW_LPP * 64] = nmc_norm_logpdf_r(prop, m, sd, isd, lsd);
      }
      NMC_CS(gs - i0 * P, 28);
    }
  };
  // ---- the state after iteration iend - 1 -> HBM (control wave; the launch's epilogue) ----
  auto write_state = [&](int iend) {
    if (!(ctl && live)) return;
    double* vo = ((iend - 1) & 1) ? d.vb1 : d.vb0;
    for (int p = 0; p < P; ++p) {
      const size_t ip = (size_t)p * G * C + gc;
      if (!sync) vo[ip] = th[p * 64];
      d.lp[ip] = st[(NMC_ST_LP * P + p) * 64];
      d.scale[ip] = st[(NMC_ST_S * P + p) * 64];
      d.nacc[ip] = (int)st[(NMC_ST_NA * P + p) * 64];
      d.nrej[ip] = (int)st[(NMC_ST_NR * P + p) * 64];
      d.tacc[ip] = (long long)st[(NMC_ST_TA * P + p) * 64];
    }
    d.ll[gc] = c_LL;
  };
  // ---- resident launch: the end of a call (t == ie), every wave (uniform) ----
  // The call's results are completed as a launch completes them -- the last publication
  // counted, the pending step's state update and sample / trace stores, the call's last Gibbs
  // tasks (register mode: the workgroups of groups 0 .. lag-1, written through and recorded)
  // -- and every wave's stores drained; the workgroup counts itself done (the last one of the
  // grid tells the host: pinned memory) and takes the next command: workgroup 0 polls the
  // host's command word and relays it, the others poll the relay of their XCD.  On a new
  // end: the first step's variates and the hyper-parameters reloaded as a launch's prologue
  // loads them; the Gibbs pipeline restarts as at a launch's start (gfirst), so the next call
  // runs exactly as a new launch of [t, end) would.  The chain state (values, scales,
  // counters, priors, group LLs) stays in LDS and is written to HBM when the launch parks.
  // false: the launch ends (park, or a timeout in d.tmo).
  unsigned rseq = d.rseq, rcall = 0;   // (rcall: calls of this launch done)
  // (s_memrealtime when this workgroup started the current call: reported with its done)
  unsigned long long rt_start = RES ? __builtin_amdgcn_s_memrealtime() : 0ull;
  // (GIBBS: the register-mode Gibbs wave's own loop, which runs the closing update; the
  //  main loop's copy holds no update and no 64-value payload)
  auto res_gate = [&](int t, auto gibbs) -> bool {
    if constexpr (!RES) {
      (void)t;
      (void)gibbs;
      return false;
    } else {
      const unsigned long long rt_end = __builtin_amdgcn_s_memrealtime();   // the call's loop done
      if (ctl) {
        if constexpr (sync) if (pub_p >= 0) {
          nmc_drain_vm();
          if (lane == 0)
            __hip_atomic_fetch_add(nmc_counter(d, cb, pub_p, g & 7), 1u, __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
          pub_p = -1;
        }
        if (pend_p >= 0) apply_pending();
        store_pending();
      }
      // the call's last Gibbs tasks, as a launch closes them: task ge-lag+j by the workgroup
      // of group j, written through and recorded (every workgroup reloads them below)
      if constexpr (hr) {
        const int ck = close_of(ie);
        if (ck >= 0) {
          const bool pub = nmc_wait_published(d, cb, ck % P,
                                              (unsigned)G * (unsigned)(ck / P - i0 + 1), lds, L);
          if constexpr (decltype(gibbs)::value)
            if (pub) nmc_hyper_update_reg(d, cb, ck / P, ck % P, cc, lds, L.hyp, true);
        }
      }
      nmc_drain_vm();
      __syncthreads();
      if (ctl) {
        if (lane == 0) {
          // done: this workgroup's start / loop-end clocks into the launch's maxima, then its
          // arrival on the device counter; the last of the grid tells the host (one write
          // to pinned memory per call, not one per workgroup: PCIe writes are the slow part)
          unsigned long long* mx = (unsigned long long*)(d.rsync + NMC_RSYNC_MAX);
          __hip_atomic_fetch_max(mx, rt_start, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          __hip_atomic_fetch_max(mx + 1, rt_end, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          nmc_drain_vm();
          rcall += 1;
          const unsigned n = __hip_atomic_fetch_add(d.rsync + NMC_RSYNC_CNT, 1u,
                                                    __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          if (n + 1 == rcall * gridDim.x) {
            const unsigned long long ck[3] = {
                __builtin_amdgcn_s_memrealtime(),
                __hip_atomic_load(mx + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT),
                __hip_atomic_load(mx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)};
            __hip_atomic_store(mx, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(mx + 1, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
            for (int k = 0; k < 3; ++k) {
              __hip_atomic_store(d.rdone + 2 + 2 * k, (unsigned)ck[k], __ATOMIC_RELAXED,
                                 __HIP_MEMORY_SCOPE_SYSTEM);
              __hip_atomic_store(d.rdone + 3 + 2 * k, (unsigned)(ck[k] >> 32), __ATOMIC_RELAXED,
                                 __HIP_MEMORY_SCOPE_SYSTEM);
            }
            nmc_drain_vm();
            __hip_atomic_store(d.rdone, rseq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
          }
        }
        unsigned end = 0xffffffffu;
        if (blockIdx.x == 0) {
          const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
          unsigned seq = rseq;
          for (unsigned spins = 0;; ++spins) {
            const unsigned long long v =
                __hip_atomic_load(d.rcmd, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            if ((int)((unsigned)v - rseq) > 0) {
              seq = (unsigned)v;
              end = (unsigned)(v >> 32);
              break;
            }
            if (__builtin_amdgcn_s_memrealtime() - t0 > d.ridle) break;   // idle: park
            if ((spins & 63) == 63 &&
                __hip_atomic_load(d.tmo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != 0)
              break;
            __builtin_amdgcn_s_sleep(4);
          }
          // (an idle park relays the next seq: the relay only ever moves forward); one copy
          // per XCD's workgroups (b & 7), each on its own 128-B line: 32 pollers a line
          if (lane < 8)
            __hip_atomic_store(
                (unsigned long long*)(d.rsync + NMC_RSYNC_REL + 32 * lane),
                ((unsigned long long)end << 32) | (seq != rseq ? seq : rseq + 1u),
                __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          if (lane == 0) {
            if (seq != rseq && end != 0xffffffffu) {   // taken: the clock, then the seq
              const unsigned long long clk = __builtin_amdgcn_s_memrealtime();
              __hip_atomic_store(d.rack + 2, (unsigned)clk, __ATOMIC_RELAXED,
                                 __HIP_MEMORY_SCOPE_SYSTEM);
              __hip_atomic_store(d.rack + 3, (unsigned)(clk >> 32), __ATOMIC_RELAXED,
                                 __HIP_MEMORY_SCOPE_SYSTEM);
              nmc_drain_vm();
              __hip_atomic_store(d.rack, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            } else {   // parked (idle, or the host's park command seq)
              __hip_atomic_store(d.rack + 1, 0x80000000u | seq, __ATOMIC_RELAXED,
                                 __HIP_MEMORY_SCOPE_SYSTEM);
            }
          }
          rseq = seq;
        } else {
          for (unsigned spins = 0;; ++spins) {
            const unsigned long long v =
                __hip_atomic_load((unsigned long long*)(d.rsync + NMC_RSYNC_REL +
                                                        32 * (blockIdx.x & 7)),
                                  __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if ((int)((unsigned)v - rseq) > 0) {
              rseq = (unsigned)v;
              end = (unsigned)(v >> 32);
              break;
            }
            if ((spins & 255) == 255 &&
                __hip_atomic_load(d.tmo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != 0)
              break;
            if (spins >= NMC_SPIN_LIMIT) {
              __hip_atomic_store(d.tmo, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
              break;
            }
            __builtin_amdgcn_s_sleep(2);
          }
        }
        const bool go = end != 0xffffffffu && (int)end > t;
        if (go) put_zl(t, 0, (t * P) & 1);   // the first step's {z, log u}
        if (lane == 0) lds[L.flag * 64 + 2] = go ? (double)end : -1.0;
      }
      __syncthreads();
      const double e = lds[L.flag * 64 + 2];
      if (e < 0.0) return false;
      if constexpr (hr) {   // the hyper-parameters after iteration t - 1, as a launch's
                            // prologue loads them (parameter p by wave p % W; sc1: the closing
                            // workgroups wrote them through before the call was reported done)
        for (int p = w; p < P; p += W) {
          const size_t ho = nmc_hslot(d, t - 1) + (size_t)p * C + cc;
          const double s2 = nmc_ldv<NMC_SRC_SC1>(d.s2 + ho);
          const double m = nmc_ldv<NMC_SRC_SC1>(d.mu + ho);
          const double sd = nmc_ldv<NMC_SRC_SC1>(d.hsd + ho);
          const double lsd = nmc_ldv<NMC_SRC_SC1>(d.hlsd + ho);
          hy[(NMC_HY_MU * P + p) * 64] = m;
          hy[(NMC_HY_SD * P + p) * 64] = sd;
          hy[(NMC_HY_LSD * P + p) * 64] = lsd;
          hy[(NMC_HY_S2 * P + p) * 64] = s2;
          hy[(NMC_HY_SDM * P + p) * 64] = sqrt(s2 / G);
          hy[(NMC_HY_ISD * P + p) * 64] = 1.0 / sd;
        }
      }
      nmc_drain_vm();   // (the control wave's variate DMA has landed)
      __syncthreads();
      ie = (int)e;
      gfirst = t * P;
      rt_start = __builtin_amdgcn_s_memrealtime();
      return true;
    }
  };
  if constexpr (hr) if (gw) {
    const int gs0 = i0 * P;
    (void)gs0;   // (the control-path stamps build)
    for (int t = i0; ok; ++t) {
      if (t == ie && !res_gate(t, nmc_bool_c<true>{})) break;
      for (int p = 0; p < P; ++p) {
        dP = nmc_kdev();
        const int gs = t * P + p;
        const bool due = gs - lag >= gfirst;
        gibbs_step(t, p);
        NMC_CS(gs - gs0, w);
        nmc_step_barrier();   // A
        if (due) {
          ok = lds[L.flag * 64 + 1] == 2.0 * ((double)gs + 1);
          if (!ok) break;
        }
        nmc_step_barrier();   // B
      }
    }
    // closing: tasks ge-lag .. ge-1, task ge-lag+j by the workgroup of group j (member 0),
    // which writes and records it -- in parallel, not one after the other; the same
    // barrier as the other waves' nmc_wait_published (RES: closed at the last gate)
    const int close_k = close_of(ie);
    if (!RES && ok && close_k >= 0) {
      if (nmc_wait_published(d, cb, close_k % P, (unsigned)G * (unsigned)(close_k / P - i0 + 1),
                             lds, L))
        nmc_hyper_update_reg(d, cb, close_k / P, close_k % P, cc, lds, L.hyp, true);
    }
    nmc_drain_vm();
    return;
  }

  for (int t = i0; ok; ++t) {
    if (t == ie && !res_gate(t, nmc_bool_c<false>{})) break;
    NMC_STAMP(t, 0);
    for (int p = 0; p < P; ++p) {
      dP = nmc_kdev();
      const int sp = (t * P + p) & 1;
      double c_prop, c_v, c_lu, c_lpc, c_lpp, c_sA, c_sR;   // control wave, this step
      // the proposal's prepared parameters, formed before barrier A (the other values
      // cannot change before the decision), so only the slot sum, finish and the
      // Metropolis test remain between the barriers
      typename Fam::Reg c_reg{};
      // Gibbs update after iteration t-1 in the all-wave modes (persistent SYNC, launch per
      // iteration): every parameter at step 0 of t
      const bool hyper_now = !hl && PARTIAL && p == 0 && t > 0 &&
                             !(t == i0 && (flags & NMC_RUN_HYPER_LOAD));
      // persistent Gibbs wave: the Gibbs update of parameter q after iteration tq is
      // task k = tq*P + q; every workgroup publishes it right after its decision at
      // global step k, so it is counted at the start of step k+1.  P == 1: the Gibbs
      // wave polls, copies and updates task gs-1 at step gs (needed at once).  P >= 2
      // (two-stage pipeline): the control wave polls task gs-1 at step gs and copies its
      // payload into LDS buffer (gs-1)&1; the Gibbs wave updates task gs-2 from buffer
      // gs&1 at step gs, beside the tiles -- needed first at step gs-2+P.
      const int gs = t * P + p, gs0 = i0 * P;
      const bool pipe = hl && !hr && P >= 2;   // two-stage (payload-in-LDS) hand-off
      const int aq = p > 0 ? p - 1 : P - 1;        // task gs-1 = (atq, aq)
      const int atq = p > 0 ? t : t - 1;
      const bool aux_now = hl && gs - lag >= gfirst;   // the Gibbs wave's task this step
      const bool comp_now = pipe && gs - 2 >= gs0;  // Gibbs task gs-2 = (ctq, cq)
      const int cq = (p + 2 * P - 2) % P;
      const int ctq = p >= 2 ? t : t - 1;
      // this step's priors come from the Gibbs wave when the update they depend on
      // lands during this step (P == 1, or P == 2 with the pipeline full)
      const bool post_prior =
          hr ? P <= 2 && aux_now : (P == 1 ? aux_now : (P == 2 && comp_now));
      // ---- the Gibbs wave, beside this step's likelihood tiles (LDS payload modes) ----
      if constexpr (hl && !hr) if (gw) {
        bool upd = false;
        if (!pipe && aux_now) {   // P == 1: poll task gs-1, copy it, update it
          const size_t hvi = (((size_t)(atq - d.vbase) * P + aq) * C + cc) * 2;
          const double hz = d.vh[hvi], hx = d.vh[hvi + 1];
          const bool r = nmc_poll_published(d, cb, aq, (unsigned)G * (unsigned)(atq - i0 + 1));
          if (lane == 0)
            __hip_atomic_store(lds + L.flag * 64 + 1, r ? 2.0 * ((double)gs + 1) : -2.0 * ((double)gs + 1),
                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
          if (p == 0) NMC_STAMP_AUX(t, 13);
          if (r) {
            // keep the payload loads below the poll (no instruction: wavefront scope)
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            const double* src = (atq & 1) ? d.vb1 : d.vb0;
            if ((C & 1) == 0) {
              nmc_hyper_dma(d, src, aq, cb, 0, G, lds, L, 0);
              nmc_drain_vm();
            } else {
              nmc_hyper_load(d, src, aq, cc, 0, G, lds, L, 0);
              asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            }
            nmc_hyper_compute(d, cb, atq, aq, lds, L, g0w, hz, hx, 0);
            upd = true;
          }
        } else if (comp_now) {   // P >= 2: task gs-2, copied into buffer (gs-2)&1 at step gs-1
          const size_t hvi = (((size_t)(ctq - d.vbase) * P + cq) * C + cc) * 2;
          if (p == 0) NMC_STAMP_CMP(t, 13);
          nmc_hyper_compute(d, cb, ctq, cq, lds, L, g0w, d.vh[hvi], d.vh[hvi + 1],
                            (gs & 1) * (G + 1));
          if (p == 0) NMC_STAMP_CMP(t, 14);
          upd = post_prior;
        }
        if (upd) {   // this step's priors (:293-294) from the update just made
          const double v = th[p * 64];
          const double prop = v + (1.0 * st[(NMC_ST_S * P + p) * 64]) *
                                      lds[(L.zl + 2 * sp) * 64 + 2 * lane];
          const double m = hy[(NMC_HY_MU * P + p) * 64], sd = hy[(NMC_HY_SD * P + p) * 64];
          const double lsd = hy[(NMC_HY_LSD * P + p) * 64], isd = hy[(NMC_HY_ISD * P + p) * 64];
          cwv[NMC_CW_LPC * 64] =
              t > 0 ? nmc_norm_logpdf_r(v, m, sd, isd, lsd) : st[(NMC_ST_LP * P + p) * 64];
          cwv[NMC_CW_LPP * 64] = nmc_norm_logpdf_r(prop, m, sd, isd, lsd);
          if (p == 0) NMC_STAMP_CMP(t, 15);
        }
      }
      // ---- control wave: counter add of the last publish, the poll and payload copy of
      //      task gs-1, the pending state update, both outcomes of the decision --
      //      accept (sA, naA, nrA, ta + 1) / reject (sR, naR, nrR, ta), tuned if due --,
      //      the next step's variates in flight, priors ----
      auto ctl_work = [&]() {
        if constexpr (sync && !hr) {   // the previous step's value is stored; count it published
          if (pub_p >= 0) {
            nmc_drain_vm();
            if (lane == 0)
              __hip_atomic_fetch_add(nmc_counter(d, cb, pub_p, g & 7), 1u, __ATOMIC_RELAXED,
                                     __HIP_MEMORY_SCOPE_AGENT);
            pub_p = -1;
          }
        }
        if constexpr (hl) if (pipe && aux_now) {   // verdict word (checked after barrier A), copy
          const bool r = nmc_poll_published(d, cb, aq, (unsigned)G * (unsigned)(atq - i0 + 1));
          if (lane == 0)
            __hip_atomic_store(lds + L.flag * 64 + 1, r ? 2.0 * ((double)gs + 1) : -2.0 * ((double)gs + 1),
                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
          if (p == 0) NMC_STAMP(t, 8);
          if (r) {
            // keep the payload loads below the poll (no instruction: wavefront scope)
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            const double* src = (atq & 1) ? d.vb1 : d.vb0;
            if ((C & 1) == 0)
              nmc_hyper_dma(d, src, aq, cb, 0, G, lds, L, ((gs - 1) & 1) * (G + 1));
            else
              nmc_hyper_load(d, src, aq, cc, 0, G, lds, L, ((gs - 1) & 1) * (G + 1));
          }
        }
        if (pend_p >= 0) apply_pending();
        c_v = th[p * 64];
        const double s = st[(NMC_ST_S * P + p) * 64];
        if (fastq && gs > gfirst)   // formed a step ahead (below, before barrier A)
          c_prop = cwv[NMC_CW_PN * 64];
        else
          c_prop = c_v + (1.0 * s) * lds[(L.zl + 2 * sp) * 64 + 2 * lane];   // propose (:304-306)
        c_lu = lds[(L.zl + 2 * sp) * 64 + 2 * lane + 1];
        {
          double thp[Fam::MAXP];
#pragma unroll
          for (int q = 0; q < Fam::MAXP; ++q)
            thp[q] = q < P ? (q == p ? c_prop : th[q * 64]) : 0.0;
          c_reg = fh.prepare(thp);
        }
        {
          const double na = st[(NMC_ST_NA * P + p) * 64], nr = st[(NMC_ST_NR * P + p) * 64];
          double naA = na + 1.0, nrA = nr, naR = na, nrR = nr + 1.0;
          c_sA = s;
          c_sR = s;
          // (tuning is the control wave's alone: evaluated here, the burn-in and interval
          //  loads and the division stay off the other waves' restart)
          const bool tune = t > 0 && t < d.burn && t % d.tune_interval == 0;
          if (tune) {
            nmc_tune(c_sA, naA, nrA);
            nmc_tune(c_sR, naR, nrR);
          }
          cwv[NMC_CW_NAA * 64] = naA;
          cwv[NMC_CW_NRA * 64] = nrA;
          cwv[NMC_CW_NAR * 64] = naR;
          cwv[NMC_CW_NRR * 64] = nrR;
          cwv[NMC_CW_TA * 64] = st[(NMC_ST_TA * P + p) * 64];
        }
        if (!hl && hyper_now) nmc_hyper_variates(d, cb, t - 1, lds, L, 0, 1);
        if (PARTIAL && !hl && p == (P > 1 ? 1 : 0)) nmc_hyper_sdm(d, lds, L, lane);
        if (!hyper_now && !(hl && post_prior)) {   // priors (:293-294)
          if (PARTIAL) {
            const double m = hy[(NMC_HY_MU * P + p) * 64], sd = hy[(NMC_HY_SD * P + p) * 64];
            const double lsd = hy[(NMC_HY_LSD * P + p) * 64], isd = hy[(NMC_HY_ISD * P + p) * 64];
            c_lpc = t > 0 ? nmc_norm_logpdf_r(c_v, m, sd, isd, lsd) : st[(NMC_ST_LP * P + p) * 64];
            c_lpp = nmc_norm_logpdf_r(c_prop, m, sd, isd, lsd);
          } else {
            c_lpc = st[(NMC_ST_LP * P + p) * 64];
            c_lpp = nmc_prior_logpdf(d.pfam[p], d.ppar + 8 * p, c_prop);
          }
        }
      };
      // ---- the control wave's memory work, last before its tiles: the count of the previous
      //      step's publication (register Gibbs mode: after the pre-work above, so the publish
      //      store has drained), then the pending sample / trace stores (issued after the count,
      //      whose vmcnt wait then covers the publish store alone) and the next step's variate
      //      DMA.  (Deferring this work until after the control wave's first tile measured
      //      slower: 15.4-15.6 against 14.7-15.0 ms per 2 000 iterations, profiles/r06.)
      auto ctl_post = [&]() {
        if constexpr (hr) {   // count the previous step's value published (the Gibbs waves
                              // poll it two steps on)
          if (pub_p >= 0) {
            nmc_drain_vm();
            if (lane == 0)
              __hip_atomic_fetch_add(nmc_counter(d, cb, pub_p, g & 7), 1u, __ATOMIC_RELAXED,
                                     __HIP_MEMORY_SCOPE_AGENT);
            pub_p = -1;
          }
        }
        store_pending();
        const int tn = p + 1 < P ? t : t + 1;
        const int pn = p + 1 < P ? p + 1 : 0;
        if (tn < ie && !(NMC_ZIN_BUILD && d.zin)) put_zl(tn, pn, sp ^ 1);   // (zin: the job)
      };
      if (ctl) {
        ctl_work();
        ctl_post();
      }
      // the control wave's tiles at the issue priority of the tile waves (its SIMD partner is
      // one of them); the decision after barrier A runs at priority 3 again
      if (ctl && ctlprio) __builtin_amdgcn_s_setprio(0);
      // ---- likelihood of the proposal (:615-635), tile by tile, every wave ----
      lik_tiles(t, p, sp, [] {});
      if (ctl && ctlprio) __builtin_amdgcn_s_setprio(3);
      NMC_STAMP(t, 1 + 3 * (p & 1));
      if (ctl || (hl && !pipe && gw)) nmc_drain_vm();   // this wave's LDS-DMA has landed
      // the next step's proposal (fastq), the expression of ctl_work: that step proposes
      // another parameter (P >= 2), whose value and scale no decision in between changes, and
      // its variates have just landed.  Written after barrier A, when every wave has read this
      // step's from the column, and read after barrier B.
      const bool pn_now = ctl && fastq && (p + 1 < P ? t : t + 1) < ie;
      double c_pn = 0.0;
      if (pn_now) {
        const int pn = p + 1 < P ? p + 1 : 0;
        c_pn = th[pn * 64] + (1.0 * st[(NMC_ST_S * P + pn) * 64]) *
                                 lds[(L.zl + 2 * (sp ^ 1)) * 64 + 2 * lane];
      }
      NMC_CS(gs - gs0, w);
      nmc_step_barrier();   // A
      if (pn_now) cwv[NMC_CW_PN * 64] = c_pn;
      NMC_STAMP(t, 2 + 3 * (p & 1));
      if (ctl) NMC_CS(gs - gs0, 8);

      // ---- Gibbs update after iteration t-1 (needed by this iteration's priors) ----
      // (Gibbs-wave modes: the poller's verdict is read in the same LDS batch as the
      // decision's operands and checked after the decision; an aborted step's decision is
      // never used -- the launch reports the timeout)
      double verdict = 0.0;
      if constexpr (hl) if (aux_now) verdict = lds[L.flag * 64 + 1];
      if constexpr (PARTIAL && !hl) if (hyper_now) {
        const int wp = P - 1;   // every parameter at step 0, once the last one's count is full
        if constexpr (sync) {   // iteration t-1 is published once parameter wp's count is full
          ok = nmc_wait_published(d, cb, wp, (unsigned)G * (unsigned)(t - i0), lds, L);
          if (!ok) break;
          nmc_hyper<NMC_SRC_SC1>(d, ((t - 1) & 1) ? d.vb1 : d.vb0, cb, t - 1, lds, L, g0w);
        } else {
          nmc_hyper<NMC_SRC_GLOBAL>(d, ((t - 1) & 1) ? d.vb1 : d.vb0, cb, t - 1, lds, L, g0w);
        }
        if (ctl) {
          const double m = hy[(NMC_HY_MU * P + p) * 64], sd = hy[(NMC_HY_SD * P + p) * 64];
          const double lsd = hy[(NMC_HY_LSD * P + p) * 64], isd = hy[(NMC_HY_ISD * P + p) * 64];
          c_lpc = nmc_norm_logpdf_r(c_v, m, sd, isd, lsd);   // t > 0 (setPrior :281)
          c_lpp = nmc_norm_logpdf_r(c_prop, m, sd, isd, lsd);
        }
        NMC_STAMP(t, 9);
      }

      // ---- control wave: group log-likelihood of the proposal (tiles in order) and
      //      the Metropolis decision, one chain per lane (:334-383) ----
      if (ctl) {
        // this step's tiles are all taken; reused at step +2 (from the static entries on)
        if (lane == 0) tcnt[sp] = (unsigned)(nstatic && W > 2 ? W - 2 : 0);
        if (hl && post_prior) {   // the Gibbs wave evaluated this step's priors (read in the
                                  // slot sums' LDS round trip)
          c_lpc = cwv[NMC_CW_LPC * 64];
          c_lpp = cwv[NMC_CW_LPP * 64];
        }
        double acc[Fam::NACC];
#pragma unroll
        for (int j = 0; j < Fam::NACC; ++j) {
          acc[j] = nmc_sum_slots(lds + (L.part + j * NMC_NSLOT) * 64 + lane);
        }
        if (S > 1)   // row split: every member's partials, in member order
          nmc_split_exchange(d, cb, g, mb, t * P + p - i0 * P, acc);
        if (p == 0) NMC_STAMP(t, 10);
        NMC_CS(gs - gs0, 14);
        const double llp = fh.finish_fast(c_reg, acc, (long)ngrp, gcst);
        if (p == 0) NMC_STAMP(t, 11);
        NMC_CS(gs - gs0, 15);
        const double postp = c_lpp + llp;
        const double post = c_lpc + c_LL;
        const double diff = postp - post;
        bool accept;
        if (!isfinite(post) && isfinite(postp)) accept = true;        // :347-352
        else if (!isfinite(llp)) accept = false;                      // :354-356
        else if (!isfinite(diff)) accept = false;                     // :358-360
        else accept = c_lu < diff;                                    // :362-364
        // :369-383, :608-610 (+ tune :385-437, prepared above)
        const double vn = accept ? c_prop : c_v;
        th[p * 64] = vn;
        if constexpr (sync) {   // publish write-through; counted at the next step's start
          if (live) nmc_store_wt(((t & 1) ? pub1 : pub0) + (size_t)p * G * C, vn);
          if (mb == 0) pub_p = p;   // (row split: member 0 publishes and counts)
        }
        st[(NMC_ST_S * P + p) * 64] = accept ? c_sA : c_sR;
        q_acc = accept;
        q_plp = accept ? c_lpp : c_lpc;
        q_pll = llp;
        pend_p = p;
        pend_t = t;
        // the rest of the update waits for the next step's pre-barrier slack
        if (p == 0) NMC_STAMP(t, 12);
      }
      if constexpr (hl) if (aux_now) {
        ok = verdict == 2.0 * ((double)gs + 1);
        if (!ok) break;
      }
      if (p == 0) NMC_STAMP(t, 3);
      if (ctl) NMC_CS(gs - gs0, 9);
      nmc_step_barrier();   // B: the new value is visible to every wave
      if (ctl) NMC_CS(gs - gs0, 10);
      if (w == 2) NMC_CS(gs - gs0, 11);
    }
    NMC_STAMP(t, 6);
    if (!ok) break;
    NMC_STAMP(t, 7);
  }

  NMC_RUN_SL(2);
  if constexpr (RES) {   // (the last call was closed at its gate): the state to HBM
    if (ok) write_state(ie);
    nmc_drain_vm();
    return;
  }
  if constexpr (sync) if (ctl && pub_p >= 0) {   // the last parameter's count
    nmc_drain_vm();
    if (lane == 0)
      __hip_atomic_fetch_add(nmc_counter(d, cb, pub_p, g & 7), 1u, __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_AGENT);
  }

  if (ctl && pend_p >= 0) apply_pending();
  if (ctl) store_pending();
  // ---- epilogue: state back to HBM (control wave) ----
  if (ok) write_state(i1);
  // ---- closing Gibbs updates after i1-1 (group-0 workgroups write and record them; the
  //      register mode: the workgroups of groups 0 .. lag-1) ----
  const int close_k = close_of(i1);
  if constexpr (hl) if (ok && (hr ? close_k >= 0 : g0w)) {
    const int ge = i1 * P;   // tasks ge-2 (copied at the last step; P >= 2) and ge-1 are left
    if (!hr && P >= 2 && gw) {
      const size_t hvi = (((size_t)(i1 - 1 - d.vbase) * P + (P - 2)) * C + cc) * 2;
      nmc_hyper_compute(d, cb, i1 - 1, P - 2, lds, L, true, d.vh[hvi], d.vh[hvi + 1],
                        ((ge - 2) & 1) * (G + 1));
    }
    // (register mode: the Gibbs wave closes in its own loop; this is the matching barrier)
    const int wk = hr ? close_k : ge - 1;   // the task whose publication is awaited
    const bool pub = nmc_wait_published(d, cb, wk % P, (unsigned)G * (unsigned)(wk / P - i0 + 1),
                                        lds, L);
    if (!hr && pub && gw) {
      const double* src = ((i1 - 1) & 1) ? d.vb1 : d.vb0;
      const int ho = ((ge - 1) & 1) * (G + 1);
      if ((C & 1) == 0) {
        nmc_hyper_dma(d, src, P - 1, cb, 0, G, lds, L, ho);
        nmc_drain_vm();
      } else {
        nmc_hyper_load(d, src, P - 1, cc, 0, G, lds, L, ho);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      }
      const size_t hvi = (((size_t)(i1 - 1 - d.vbase) * P + (P - 1)) * C + cc) * 2;
      nmc_hyper_compute(d, cb, i1 - 1, P - 1, lds, L, true, d.vh[hvi], d.vh[hvi + 1], ho);
    }
  }
  if constexpr (sync && !hl) if (ok && g0w) {
    nmc_hyper_sdm(d, lds, L, lane);
    nmc_hyper_variates(d, cb, i1 - 1, lds, L, 0, W);
    nmc_drain_vm();
    if (nmc_wait_published(d, cb, P - 1, (unsigned)G * (unsigned)(i1 - i0), lds, L))
      nmc_hyper<NMC_SRC_SC1>(d, ((i1 - 1) & 1) ? d.vb1 : d.vb0, cb, i1 - 1, lds, L, true);
  }
  NMC_RUN_SL(3);
#undef d
}
