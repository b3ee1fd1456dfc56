// ll_kernels.h -- the small log-likelihood kernels beside the step kernels: group
// log-likelihoods of arbitrary values (nmc_k_group_part, nmc_k_group_fin) and
// per-observation log-likelihoods (nmc_k_obs_ll_rows, nmc_k_obs_ll).  User families
// instantiate them through hiprtc (user.hip kNames).
#pragma once

#include "dev.h"
#include "rows.h"

// theta[q] = src[q][g][c] for q < P.
template <int MP>
__device__ __forceinline__ void nmc_load_theta(const Dev& d, const double* src, int g, int c,
                                               double (&th)[MP]) {
#pragma unroll
  for (int q = 0; q < MP; ++q) {
    th[q] = 0.0;
    if (q < d.P) th[q] = src[((size_t)q * d.G + g) * d.C + c];
  }
}

// Group log-likelihoods for arbitrary theta [P][G][C] (the batched start-point search and
// partial init of nestmc/init.py), summed EXACTLY as the step kernels sum a proposal's
// likelihood: the same row-split members, tile partition (nmc_tiles), row loop (rows
// staged in LDS or read from global memory, as the step kernel of this context does),
// 16-slot combine, member order and finish_fast -- so a chain's stored group LL never
// depends on which kernel produced it, on the wave count or on the chain sharding.
// Part 1: grid CB * G * S workgroups (member m of group g of chain block cb), W waves take
// tiles k = w, w + W, ...; out part[m][j][g][C] (NACC accumulators).
template <class Fam, bool RL>
__global__ void __launch_bounds__(512)
nmc_k_group_part(Dev d, Fam fam, const double* __restrict__ obs, const double* theta,
                 double* part) {
  extern __shared__ __attribute__((aligned(16))) double lds[];   // [NACC][NSLOT] slots, rows
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int W = blockDim.x >> 6;
  const int S = d.S;
  const int mb = blockIdx.x % S;
  const int g = (blockIdx.x / S) % d.G, cb = (blockIdx.x / S) / d.G;
  const int c = cb * 64 + lane;
  const int cc = c < d.C ? c : d.C - 1;
  double th[Fam::MAXP];
  nmc_load_theta(d, theta, g, cc, th);
  const typename Fam::Reg reg = fam.prepare(th);
  int64_t r0;
  int nrow;
  nmc_chunk(d.off[g], d.off[g + 1], mb, S, &r0, &nrow);
  const nmc_tiling TI = nmc_tiles(nrow, d.tile);
  const double* grows = obs + r0 * Fam::NFIELDS;
  double* lrows = lds + Fam::NACC * NMC_NSLOT * 64;
  if constexpr (RL) {
    const int nd = nrow * Fam::NFIELDS;
    for (int i = threadIdx.x; i < nd; i += blockDim.x) lrows[i] = grows[i];
  }
  for (int j = 0; j < Fam::NACC; ++j)
    for (int k = TI.nt + w; k < NMC_NSLOT; k += W) lds[(j * NMC_NSLOT + k) * 64 + lane] = -0.0;
  __syncthreads();
  for (int k = w; k < TI.nt; k += W) {
    const int ra = TI.start(k), rn = TI.len(k);
    double acc[Fam::NACC];
    if constexpr (RL)
      nmc_ll_rows_lds(fam, reg, lrows + (size_t)ra * Fam::NFIELDS, rn, acc);
    else
      nmc_ll_rows(fam, reg, grows + (size_t)ra * Fam::NFIELDS, rn, acc);
#pragma unroll
    for (int j = 0; j < Fam::NACC; ++j) lds[(j * NMC_NSLOT + k) * 64 + lane] = acc[j];
  }
  __syncthreads();
  if (w != 0 || c >= d.C) return;
#pragma unroll
  for (int j = 0; j < Fam::NACC; ++j)
    part[(((size_t)mb * Fam::NACC + j) * d.G + g) * d.C + c] = nmc_sum_slots(lds + j * NMC_NSLOT * 64 + lane);
}

// Part 2: the members' partials in member order (nmc_split_exchange's four streams),
// finish_fast -> out [G][C].  One thread per (group, chain).
template <class Fam>
__global__ void __launch_bounds__(256)
nmc_k_group_fin(Dev d, Fam fam, const double* theta, const double* part, double* out) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)d.G * d.C) return;
  const int c = (int)(i % d.C), g = (int)(i / d.C);
  const int S = d.S;
  double th[Fam::MAXP];
  nmc_load_theta(d, theta, g, c, th);
  const typename Fam::Reg reg = fam.prepare(th);
  double acc[Fam::NACC];
#pragma unroll
  for (int j = 0; j < Fam::NACC; ++j) {
    double s4[4] = {0.0, 0.0, 0.0, 0.0};
    for (int m = 0; m < S; ++m) {
      const double v = part[(((size_t)m * Fam::NACC + j) * d.G + g) * d.C + c];
      s4[m & 3] = m < 4 ? v : s4[m & 3] + v;
    }
    acc[j] = S >= 4 ? (s4[0] + s4[1]) + (s4[2] + s4[3])
                    : (S == 1 ? s4[0] : (S == 2 ? s4[0] + s4[1] : (s4[0] + s4[1]) + s4[2]));
  }
  const long n = (long)(d.off[g + 1] - d.off[g]);
  out[i] = fam.finish_fast(reg, acc, n, fam.gconst(n));
}

// StepMethod.logLikelihood (:656-659) at recorded rows of the device sample store:
// out[c - c0][r][i] = observation i's log-likelihood at the values of row row0 + r (the state
// Sampler._printLogLikelihood evaluated at that recorded iteration, :890-891).  One
// thread per (observation, chain, row), writes coalesced along the observations.
// pc: 2 if the sample columns carry the hyper-parameters (partial pooling), else 0.
template <class Fam>
__global__ void __launch_bounds__(256)
nmc_k_obs_ll_rows(Dev d, Fam fam, const int* __restrict__ gidx, int64_t n_obs, int pc, int row0,
                  int nrows, int c0, double* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int c = c0 + (int)blockIdx.y, r = blockIdx.z;   // (chains [c0, c0 + gridDim.y))
  if (i >= n_obs) return;
  const int g = gidx[i];
  const double* row = d.samples + (size_t)(row0 + r) * d.cols * d.C + c;
  double th[Fam::MAXP];
#pragma unroll
  for (int q = 0; q < Fam::MAXP; ++q)
    th[q] = q < d.P ? row[((size_t)q * (d.G + pc) + pc + g) * d.C] : 0.0;
  const typename Fam::Reg reg = fam.prepare(th);
  out[((size_t)blockIdx.y * nrows + r) * n_obs + i] = fam.obs_ll(reg, d.obs + i * Fam::NFIELDS);
}

// The same values in the sample store's layout, for the column sort of sortcol.h (PSIS-LOO,
// psis.h): observations [o0, o0 + B) at rows [row0, row0 + nrows) ->
// out[r][o - o0][C], the chain fastest.  Grid (ceil(B / (4 NMC_LOO_OT)), CB, min(nrows, 65535)),
// 256 threads: lane = chain of chain block blockIdx.y, every load of theta and every store one
// coalesced run of the wave; wave w of workgroup bx walks the NMC_LOO_OT consecutive
// observations from o0 + (4 bx + w) NMC_LOO_OT on and prepares again only where the group
// changes (wave-uniform).  theta's column arithmetic, prepare and obs_ll are
// nmc_k_obs_ll_rows' own: every value has its bits.
enum { NMC_LOO_OT = 8 };
template <class Fam>
__global__ void __launch_bounds__(256)
nmc_k_loo_ll(Dev d, Fam fam, const int* __restrict__ gidx, int pc, int row0, int nrows,
             int64_t o0, int B, double* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int c = (int)blockIdx.y * 64 + lane;
  const int cc = c < d.C ? c : d.C - 1;   // (a padding lane reads the last chain, stores nothing)
  const int b0 = ((int)blockIdx.x * 4 + w) * NMC_LOO_OT;
  if (b0 >= B) return;
  const int b1 = b0 + NMC_LOO_OT < B ? b0 + NMC_LOO_OT : B;
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
      const double v = fam.obs_ll(reg, d.obs + i * Fam::NFIELDS);
      if (c < d.C) out[((size_t)r * B + b) * d.C + c] = v;
    }
  }
}

// Per-observation LL at the values in `value` [P][G][C] -> out [C][n_obs].
template <class Fam>
__global__ void __launch_bounds__(64)
nmc_k_obs_ll(Dev d, Fam fam, const double* value, double* out, int64_t n_obs) {
  const int lane = threadIdx.x & 63;
  const int g = blockIdx.x % d.G, cb = blockIdx.x / d.G;
  const int c = cb * 64 + lane;
  const int cc = c < d.C ? c : d.C - 1;
  double th[Fam::MAXP];
  nmc_load_theta(d, value, g, cc, th);
  const typename Fam::Reg reg = fam.prepare(th);
  const int nf = Fam::NFIELDS;
  for (int64_t r = d.off[g]; r < d.off[g + 1]; ++r) {
    const double v = fam.obs_ll(reg, d.obs + r * nf);
    if (c < d.C) out[(size_t)c * n_obs + r] = v;
  }
}
