// kernels.h -- the MCMC sampling kernels for gfx950 (CDNA4, wave64, fp64).
//
// Layout: chain-on-lane.  A workgroup owns one (chain block of 64 chains, group g)
// pair (none/complete pooling on few workgroups: 32 chains, NMC_MODE_HALF); its W waves
// split the group's CSR rows obs[off[g]..off[g+1]), staged once per launch in LDS.
// Every lane holds one chain's parameters in registers while the wave walks the same
// rows, so one broadcast ds_read feeds 64 chains (the paired loop: two chains per lane,
// one row pair per read) -- the cross-chain reuse that keeps the dataset on chip.
//
// nmc_k_run runs the reference's Sampler._loop body (posteriorSampling.py:872-891)
// for iterations [i0, i1) of every (chain, group).  Per parameter step p
// (StepMethod.step :594-613):
//   1. every wave proposes theta_p' = theta_p + scale*z (Parameter.propose :304-306)
//      and takes likelihood row tiles of the group from an LDS queue (:615-635); the
//      tile partition depends on the rows alone, so every sum is fixed;
//   2. barrier A: the control wave (wave 0) adds the tile partials in a fixed order and
//      makes the Metropolis decision (:334-383, branch order exact, IEEE isfinite),
//      tuning (:385-437) and group-LL propagation (:608-610);
//   3. barrier B: the decided value is visible; the rest of the state update is
//      deferred into the next step's slack.
// The step's {z, log u} are drawn by a job in the previous step's tile queue (Philox,
// or the replayed reference variates).
//
// Partial pooling couples the G groups of a chain through the Gibbs update of the
// hyper-parameters (HyperParameter.update :463-498).  The update of parameter q after
// iteration t is needed first by the decision of step (t + 1, q), not by any
// likelihood, so it is pipelined behind the steps in between:
//   * persistent modes (every workgroup resident): decided values are published
//     write-through (sc1 stores, vmcnt drain, one agent-scope counter add per
//     workgroup and step); the Gibbs wave (wave 1) polls the chain block's counter two
//     steps later, reads the values with sc1 loads (MI355X_MICROARCH.md, inter-workgroup
//     visibility) and updates in numpy's pairwise order (exact mean/variance parity);
//   * launch-per-iteration mode (grid too large to be resident): the kernel boundary
//     publishes, plain loads read.
// Every spin is bounded: a timeout sets d.tmo (pinned host memory) and every
// workgroup drains.
#pragma once

// The parts, by role (this header only includes them):
#include "dev.h"         // struct Dev, constants, LDS carve, row tiling: shared with the host
#include "stamps.h"      // diagnostic clock stamps (empty in the shipped build)
#include "mem.h"         // sc1 loads, LDS-DMA, publish counters and polls, barriers
#include "rows.h"        // likelihood row loops
#include "gibbs.h"       // hyper-parameter Gibbs update, row-split exchange
#include "step.h"        // nmc_k_run, tuning, the step variates
#include "ll_kernels.h"  // group and per-observation log-likelihood kernels
#include "waic.h"        // WAIC: per-observation reduction over the sample store
#include "ppc.h"         // posterior predictive draws and their reductions over the store
#include "predict.h"     // held-out rows and new groups: draws, densities and their reduction
#include "loopit.h"      // LOO-PIT: one response field's replicates in the store's layout
