// loopit.h -- the replicates of one response field in the sample store's layout, for the
// leave-one-out PIT and predictive moments (nmc_loo_pit in nestmc.hip; nmc_k_psis_expect in
// psis.h; nestmc/loopit.py has the definitions).  No reference counterpart.
//
// nmc_k_loo_yrep is nmc_k_loo_ll's twin (ll_kernels.h): the same grid, lane = chain, the same
// theta column arithmetic and prepare, but where that one evaluates obs_ll this one draws
// y_rep of response field j by nmc_ppc_draw (ppc.h) -- the Philox block of (absolute row,
// observation, field, global chain, seed), so every value has the bits of nmc_k_ppc_draws'
// and of the replicate nmc_k_ppc_obs compares.  out[r][o - o0][C] lies value for value beside
// the log-likelihoods nmc_k_loo_ll wrote for the same batch: nmc_k_psis_expect walks the two
// in step.  Workgroups (., 0, 0) also write yobs[o - o0] = the observed row[resp_field(j)].
#pragma once

#include "ll_kernels.h"
#include "ppc.h"

template <class Fam>
__global__ void __launch_bounds__(256)
nmc_k_loo_yrep(Dev d, Fam fam, const int* __restrict__ gidx, int pc, int row0, int nrows,
               int64_t o0, int B, int j, double* __restrict__ out, double* __restrict__ yobs) {
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int c = (int)blockIdx.y * 64 + lane;
  const int cc = c < d.C ? c : d.C - 1;   // (a padding lane reads the last chain, stores nothing)
  const uint32_t chain = (uint32_t)(d.chain_base + cc);
  const int b0 = ((int)blockIdx.x * 4 + w) * NMC_LOO_OT;
  if (b0 >= B) return;
  const int b1 = b0 + NMC_LOO_OT < B ? b0 + NMC_LOO_OT : B;
  if (blockIdx.y == 0 && blockIdx.z == 0 && lane < b1 - b0)
    yobs[b0 + lane] = d.obs[(o0 + b0 + lane) * Fam::NFIELDS + Fam::resp_field(j)];
  for (int r = blockIdx.z; r < nrows; r += gridDim.z) {
    const double* row = d.samples + (size_t)(row0 + r) * d.cols * d.C + cc;
    int gp = -1;
    typename Fam::Reg reg;
    for (int b = b0; b < b1; ++b) {
      const int64_t i = o0 + b;
      const int g = gidx[i];
      if (g != gp) {
        double th[Fam::MAXP];
#pragma unroll
        for (int q = 0; q < Fam::MAXP; ++q)
          th[q] = q < d.P ? row[((size_t)q * (d.G + pc) + pc + g) * d.C] : 0.0;
        reg = fam.prepare(th);
        gp = g;
      }
      const double v = nmc_ppc_draw(fam, reg, d.obs + i * Fam::NFIELDS, (uint32_t)(row0 + r),
                                    (uint32_t)i, j, chain, d.seed);
      if (c < d.C) out[((size_t)r * B + b) * d.C + c] = v;
    }
  }
}
