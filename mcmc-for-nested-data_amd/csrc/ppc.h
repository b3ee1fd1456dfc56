// ppc.h -- posterior predictive checks over the device sample store (Gelman, Meng and Stern
// 1996; BDA3 ch. 6): a replicated data set y_rep from every sample s = (chain, recorded row),
// compared with the observed data per observation (nmc_k_ppc_obs) and per group
// (nmc_k_ppc_group); nmc_k_ppc_draws writes the replicates themselves.  The reference has no
// counterpart: its users draw on the host from the sample files.
//
// The stream.  One Philox block per (recorded row r, observation i, response field j, chain):
//   (ua, ub) = nmc_uniform2(it = r, group = i, param = j, purpose = NMC_PURPOSE_PREDICT,
//                           chain = chain_base + local chain, seed),  z = nmc_box_muller(ua, ub)
// r the absolute row of the store, i the observation's index in the family's table
// (n_obs < 2^32), and y_rep = Fam::predict(reg, row_i, j, ua, ub, z) (families.h).  A draw
// depends on (seed, global chain, row, observation, field) alone: not on the window, the
// launch geometry, the sharding or the kernel that asks, so the two reducing kernels see the
// same replicates without an S x n_obs buffer between them -- each draws them again.
//
// Both reductions keep Welford's (n, mean, M2) -- waic.h's recurrence and merge without its
// (m, s) -- and integer counts; identity (0, 0, 0) and zero counts.  merge A then B:
//   d = meanB - meanA, n = nA + nB, mean = meanA + d nB / n, M2 = M2A + M2B + d^2 nA nB / n
// (n = 0: mean = M2 = 0).  The counts are uint32: a chain block's count is at most 64 n_rows,
// so a call takes n_rows < 2^26; the host adds blocks and engines in int64.  A draw that is not
// finite is counted in the device counter by nmc_k_ppc_obs alone (each draw once), propagates
// as NaN into the floating-point states and is counted in no lt, eq or gt.
#pragma once

#include "dev.h"
#include "rng.h"
#include "waic.h"

enum {
  NMC_PPC_NSTAT = 4,    // the group statistics: mean, population variance, minimum, maximum
  NMC_PPC_WGS = 512     // nmc_k_ppc_group: workgroups below which the rows are sliced
};

struct nmc_ppc_state { double n, mean, M2; };

__device__ __forceinline__ nmc_ppc_state nmc_ppc_merge(const nmc_ppc_state& A,
                                                       const nmc_ppc_state& B) {
  nmc_ppc_state r;
  r.n = A.n + B.n;
  const double d = B.mean - A.mean;
  const bool some = r.n > 0.0;
  r.mean = some ? A.mean + d * B.n / r.n : 0.0;
  r.M2 = some ? A.M2 + B.M2 + d * d * A.n * B.n / r.n : 0.0;
  return r;
}

// The 64 lanes' states merged as waic.h merges them: partner lane ^ 1, ^ 2, ... ^ 32, the lower
// lane's state the A operand at every level; every lane ends with the wave's state.
__device__ __forceinline__ nmc_ppc_state nmc_ppc_butterfly(nmc_ppc_state a, int lane) {
#pragma unroll
  for (int k = 1; k < 64; k <<= 1) {
    nmc_ppc_state b;
    b.n = __shfl_xor(a.n, k);
    b.mean = __shfl_xor(a.mean, k);
    b.M2 = __shfl_xor(a.M2, k);
    const bool hi = (lane & k) != 0;
    const nmc_ppc_state A = {hi ? b.n : a.n, hi ? b.mean : a.mean, hi ? b.M2 : a.M2};
    const nmc_ppc_state B = {hi ? a.n : b.n, hi ? a.mean : b.mean, hi ? a.M2 : b.M2};
    a = nmc_ppc_merge(A, B);
  }
  return a;
}
__device__ __forceinline__ unsigned nmc_ppc_wave_sum(unsigned v) {
#pragma unroll
  for (int k = 1; k < 64; k <<= 1) v += (unsigned)__shfl_xor((int)v, k);
  return v;
}

template <class Fam>
__device__ __forceinline__ double nmc_ppc_draw(const Fam& fam, const typename Fam::Reg& reg,
                                               const double* __restrict__ row, uint32_t r,
                                               uint32_t i, int j, uint32_t chain, uint32_t seed) {
  const nmc_d2 u = nmc_uniform2(r, i, (uint32_t)j, NMC_PURPOSE_PREDICT, chain, seed);
  const double z = nmc_box_muller(u.a, u.b);
  return fam.predict(reg, row, j, u.a, u.b, z);
}

// The replicates themselves: out[c][r][i][j] of chain c, row row0 + r, observation i and
// response field j, in nmc_k_obs_ll_rows' shape (one thread per observation, chain and row;
// grid (ceil(n_obs / 256), C, nrows)) with its theta arithmetic.  For small windows, tests and
// users with a statistic of their own.
template <class Fam>
__global__ void __launch_bounds__(256)
nmc_k_ppc_draws(Dev d, Fam fam, const int* __restrict__ gidx, int64_t n_obs, int pc, int row0,
                int nrows, double* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int c = (int)blockIdx.y, r = blockIdx.z;
  if (i >= n_obs) return;
  const int g = gidx[i];
  const double* row = d.samples + (size_t)(row0 + r) * d.cols * d.C + c;
  double th[Fam::MAXP];
#pragma unroll
  for (int q = 0; q < Fam::MAXP; ++q)
    th[q] = q < d.P ? row[((size_t)q * (d.G + pc) + pc + g) * d.C] : 0.0;
  const typename Fam::Reg reg = fam.prepare(th);
  double* o = out + (((size_t)c * nrows + r) * n_obs + i) * Fam::NRESP;
  for (int j = 0; j < Fam::NRESP; ++j)
    o[j] = nmc_ppc_draw(fam, reg, d.obs + i * Fam::NFIELDS, (uint32_t)(row0 + r), (uint32_t)i, j,
                        (uint32_t)(d.chain_base + c), d.seed);
}

// Per observation and response field, over the samples of a chain block: n, Welford's mean and
// M2 of y_rep and the counts lt = #{y_rep < y}, eq = #{y_rep == y}.  nmc_k_waic's launch: grid
// (ceil(ntiles / 4), CB), 256 threads, wave w of workgroup (bx, cb) serves tile 4 bx + w of
// x->wtiles for the 64 chains of chain block cb, lane = chain, theta by its column arithmetic
// with the next row's loads issued before this row is consumed, observation rows wave-uniform
// reads.  The response fields loop OUTSIDE the row loop, so a lane holds the state of one
// field at a time (4 words per observation of the tile).  Per field the 64 lanes merge in the
// butterfly above, chains >= n_valid entering as the identity, and lanes [0, 3 T) store
// st[cb][3][NRESP][n_obs] (n, mean, M2), lanes [0, 2 T) ct[cb][2][NRESP][n_obs] (lt, eq).  No
// LDS, no barrier, no waiting on another workgroup.
template <class Fam>
__global__ void __launch_bounds__(256)
nmc_k_ppc_obs(Dev d, Fam fam, const double* __restrict__ obs,
              const nmc_waic_tile* __restrict__ tiles, int ntiles, int64_t n_obs, int pc, int row0,
              int nrows, int n_valid, double* __restrict__ st, uint32_t* __restrict__ ct,
              unsigned long long* nonfinite) {
  constexpr int T = NMC_WAIC_T, NR = Fam::NRESP;
  const int lane = threadIdx.x & 63;
  const int tile = (int)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (tile >= ntiles) return;
  const int cb = blockIdx.y;
  const int64_t start = tiles[tile].start;
  const int g = tiles[tile].g, len = tiles[tile].len;
  const int c = cb * 64 + lane;
  const bool valid = c < n_valid;
  const int cc = valid ? c : n_valid - 1;   // (n_valid <= C: the read stays inside the store)
  const uint32_t chain = (uint32_t)(d.chain_base + cc);
  // the tile's observation rows; a short tile draws for its last row again and drops it
  const double* orow[T];
  uint32_t oi[T];
#pragma unroll
  for (int t = 0; t < T; ++t) {
    const int64_t i = start + (t < len ? t : len - 1);
    orow[t] = obs + i * (int64_t)Fam::NFIELDS;
    oi[t] = (uint32_t)i;
  }
  const size_t rstride = (size_t)d.cols * d.C, qstride = (size_t)(d.G + pc) * d.C;
  const double* col = d.samples + (size_t)row0 * rstride + (size_t)(pc + g) * d.C + cc;
  unsigned bad = 0;
  for (int j = 0; j < NR; ++j) {
    double y[T], mean[T], M2[T];
    unsigned lt[T], eq[T];
#pragma unroll
    for (int t = 0; t < T; ++t) {
      y[t] = orow[t][Fam::resp_field(j)];
      mean[t] = 0.0; M2[t] = 0.0; lt[t] = 0; eq[t] = 0;
    }
    if (cb * 64 < n_valid) {   // (a chain block of padding only: the identity, no rows read)
      double thn[Fam::MAXP];
#pragma unroll
      for (int q = 0; q < Fam::MAXP; ++q) thn[q] = q < d.P ? col[q * qstride] : 0.0;
      for (int r = 0; r < nrows; ++r) {
        double th[Fam::MAXP];
#pragma unroll
        for (int q = 0; q < Fam::MAXP; ++q) th[q] = thn[q];
        const double* nxt = col + (size_t)(r + 1 < nrows ? r + 1 : r) * rstride;
#pragma unroll
        for (int q = 0; q < Fam::MAXP; ++q) thn[q] = q < d.P ? nxt[q * qstride] : 0.0;
        const typename Fam::Reg reg = fam.prepare(th);
        const double ik = 1.0 / (double)(r + 1);
#pragma unroll
        for (int t = 0; t < T; ++t) {
          const double x = nmc_ppc_draw(fam, reg, orow[t], (uint32_t)(row0 + r), oi[t], j, chain,
                                        d.seed);
          const bool fin = isfinite(x);
          if (!fin && t < len) ++bad;
          lt[t] += fin && x < y[t] ? 1u : 0u;
          eq[t] += fin && x == y[t] ? 1u : 0u;
          const double dl = x - mean[t];
          mean[t] = mean[t] + dl * ik;
          M2[t] = M2[t] + dl * (x - mean[t]);
        }
      }
    }
    const int sel = lane < 3 * T ? lane : -1;   // state component sel / T of observation sel % T
    double outv = 0.0;
    unsigned outc = 0;
#pragma unroll
    for (int t = 0; t < T; ++t) {
      nmc_ppc_state a;
      a.n = valid ? (double)nrows : 0.0;
      a.mean = valid ? mean[t] : 0.0;
      a.M2 = valid ? M2[t] : 0.0;
      a = nmc_ppc_butterfly(a, lane);
      const unsigned sl = nmc_ppc_wave_sum(valid ? lt[t] : 0u);
      const unsigned se = nmc_ppc_wave_sum(valid ? eq[t] : 0u);
      if (sel == 0 * T + t) { outv = a.n; outc = sl; }
      if (sel == 1 * T + t) { outv = a.mean; outc = se; }
      if (sel == 2 * T + t) outv = a.M2;
    }
    if (sel >= 0 && sel % T < len) {
      const size_t at = (size_t)j * n_obs + start + sel % T;
      st[((size_t)cb * 3 + sel / T) * NR * n_obs + at] = outv;
      if (sel < 2 * T) ct[((size_t)cb * 2 + sel / T) * NR * n_obs + at] = outc;
    }
  }
  if (bad && valid) atomicAdd(nonfinite, (unsigned long long)bad);
}

// The four statistics T of a group's values taken in observation order: Welford's mean and
// M2 (var = M2 / n, the population variance), fmin and fmax.  The same function serves the
// observed field and every replicate.
//
// INT (Fam::RESP_INT: the response takes integer values, e.g. the logistic's 0 / 1): the mean
// and the variance come from the sums s1 = sum x and s2 = sum x^2 instead, mean = s1 / n,
// var = (n s2 - s1 s1) / (n n).  Integer sums and products are exact (below 2^53), one
// division rounds: the statistic depends on the values alone and not on their order, and a
// replicate that ties with the data -- the same count of ones, or for the variance also the
// complementary count -- compares EQUAL.
// Welford's mean of 0 / 1 values depends on their order in the last place ([1, 1, 0] gives
// 0.66666666666666674, [0, 1, 1] 0.66666666666666663), which would decide every tie -- for a
// binary response a tenth and more of the samples -- by rounding: on the logistic case of
// tests/store_cases.py that moved p by up to 0.11 (tests/test_ppc_host.py).
struct nmc_ppc_T { double mean, M2, mn, mx; };
__device__ __forceinline__ nmc_ppc_T nmc_ppc_T0() {
  return nmc_ppc_T{0.0, 0.0, __builtin_huge_val(), -__builtin_huge_val()};
}
template <bool INT>
__device__ __forceinline__ void nmc_ppc_T_add(nmc_ppc_T& a, double x, double k) {
  if constexpr (INT) {
    a.mean = a.mean + x;
    a.M2 = a.M2 + x * x;
  } else {
    const double dl = x - a.mean;
    a.mean = a.mean + dl * (1.0 / k);
    a.M2 = a.M2 + dl * (x - a.mean);
  }
  a.mn = fmin(a.mn, x);
  a.mx = fmax(a.mx, x);
}
template <bool INT>
__device__ __forceinline__ void nmc_ppc_T_fin(const nmc_ppc_T& a, double n,
                                              double (&T)[NMC_PPC_NSTAT]) {
  if constexpr (INT) {
    T[0] = a.mean / n;
    T[1] = (n * a.M2 - a.mean * a.mean) / (n * n);
  } else {
    T[0] = a.mean;
    T[1] = a.M2 / n;
  }
  T[2] = a.mn;
  T[3] = a.mx;
}

// Slices of nmc_k_ppc_group's rows for G * NRESP * CB (group, field, chain block) triples: as
// many as bring the grid to NMC_PPC_WGS workgroups, at least four rows (one per wave) each.
// A function of the shape alone, never of the device: the merge order, and with it every bit
// of the result, is the same everywhere (nestmc/ppc.py group_slices restates it).
static inline int nmc_ppc_slices(int nrows, int64_t triples) {
  const int64_t want = triples > 0 ? (NMC_PPC_WGS + triples - 1) / triples : 1;
  const int64_t most = ((int64_t)nrows + 3) / 4;
  const int64_t ns = want < most ? want : most;
  return ns < 1 ? 1 : (ns > 65535 ? 65535 : (int)ns);
}

// Per (group g, response field j) and per sample: T(y_rep) of the group's replicated
// observations i = off[g] .. off[g + 1] - 1 against T(y) of the observed field (the same
// device function, nmc_ppc_T_add / _fin, in the same order), reduced over
// the samples to the counts gt = #{T(y_rep) > T(y)}, eq = #{==} and Welford's (n, mean, M2) of
// each T(y_rep).  A sample with a draw that is not finite has four NaN statistics (fmin and
// fmax would drop the NaN): they enter the states and no count.
//
// Grid (G * NRESP, CB, NS), 256 threads: workgroup (g NRESP + j, cb, sl), lane = chain of
// chain block cb, serves the rows of slice sl, [sl nrows / NS, (sl + 1) nrows / NS) of the
// window, dealt to its four waves: wave w walks rows w, w + 4, ... of the slice in order, the
// next row's theta loaded before this row is consumed.  Merge order, fixed:
//   1. a lane's samples by Welford's recurrence in row order (k = its own count);
//   2. the 64 lanes of a wave by the butterfly above (chains >= n_valid the identity);
//   3. the four waves in the order 0, 1, 2, 3 (A = the merged so far), through LDS;
//   4. the slices in the order 0 .. NS - 1 (nmc_k_ppc_group_fin, nestmc.hip);
//   5. the chain blocks and engines on the host (nestmc/ppc.py merge).
// Workgroup (., 0, 0) also writes ty[g][j][4] = T(y).  No kernel waits on another workgroup.
template <class Fam>
__global__ void __launch_bounds__(256)
nmc_k_ppc_group(Dev d, Fam fam, const double* __restrict__ obs, int pc, int row0, int nrows,
                int n_valid, double* __restrict__ gs, uint32_t* __restrict__ gc,
                double* __restrict__ ty) {
  constexpr int NS_ = NMC_PPC_NSTAT, NR = Fam::NRESP;
  __shared__ double sst[4][NS_][3];
  __shared__ unsigned sct[4][NS_][2];
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int g = (int)blockIdx.x / NR, j = (int)blockIdx.x % NR;
  const int cb = blockIdx.y, sl = blockIdx.z, NS = gridDim.z;
  const int64_t i0 = d.off[g], i1 = d.off[g + 1];
  const double ng = (double)(i1 - i0);
  const int f = Fam::resp_field(j);
  constexpr bool INT = Fam::RESP_INT;
  nmc_ppc_T o = nmc_ppc_T0();
  for (int64_t i = i0; i < i1; ++i)
    nmc_ppc_T_add<INT>(o, obs[i * Fam::NFIELDS + f], (double)(i - i0 + 1));
  double Ty[NS_];
  nmc_ppc_T_fin<INT>(o, ng, Ty);
  if (cb == 0 && sl == 0 && threadIdx.x == 0) {
#pragma unroll
    for (int s = 0; s < NS_; ++s) ty[((size_t)g * NR + j) * NS_ + s] = Ty[s];
  }

  const int c = cb * 64 + lane;
  const bool valid = c < n_valid;
  const int cc = valid ? c : n_valid - 1;
  const uint32_t chain = (uint32_t)(d.chain_base + cc);
  const int rb = (int)((int64_t)sl * nrows / NS), re = (int)((int64_t)(sl + 1) * nrows / NS);
  double k = 0.0, mean[NS_], M2[NS_];
  unsigned gt[NS_], eq[NS_];
#pragma unroll
  for (int s = 0; s < NS_; ++s) { mean[s] = 0.0; M2[s] = 0.0; gt[s] = 0; eq[s] = 0; }
  if (cb * 64 < n_valid && rb + w < re) {
    const size_t rstride = (size_t)d.cols * d.C, qstride = (size_t)(d.G + pc) * d.C;
    const double* col = d.samples + (size_t)row0 * rstride + (size_t)(pc + g) * d.C + cc;
    double thn[Fam::MAXP];
    const double* fst = col + (size_t)(rb + w) * rstride;
#pragma unroll
    for (int q = 0; q < Fam::MAXP; ++q) thn[q] = q < d.P ? fst[q * qstride] : 0.0;
    for (int r = rb + w; r < re; r += 4) {
      double th[Fam::MAXP];
#pragma unroll
      for (int q = 0; q < Fam::MAXP; ++q) th[q] = thn[q];
      const double* nxt = col + (size_t)(r + 4 < re ? r + 4 : r) * rstride;
#pragma unroll
      for (int q = 0; q < Fam::MAXP; ++q) thn[q] = q < d.P ? nxt[q * qstride] : 0.0;
      const typename Fam::Reg reg = fam.prepare(th);
      nmc_ppc_T a = nmc_ppc_T0();
      unsigned nb = 0;
      for (int64_t i = i0; i < i1; ++i) {
        const double x = nmc_ppc_draw(fam, reg, obs + i * Fam::NFIELDS, (uint32_t)(row0 + r),
                                      (uint32_t)i, j, chain, d.seed);
        nb += isfinite(x) ? 0u : 1u;
        nmc_ppc_T_add<INT>(a, x, (double)(i - i0 + 1));
      }
      double Tv[NS_];
      nmc_ppc_T_fin<INT>(a, ng, Tv);
#pragma unroll
      for (int s = 0; s < NS_; ++s) Tv[s] = nb ? __builtin_nan("") : Tv[s];
      k = k + 1.0;
      const double ik = 1.0 / k;
#pragma unroll
      for (int s = 0; s < NS_; ++s) {
        gt[s] += Tv[s] > Ty[s] ? 1u : 0u;
        eq[s] += Tv[s] == Ty[s] ? 1u : 0u;
        const double dl = Tv[s] - mean[s];
        mean[s] = mean[s] + dl * ik;
        M2[s] = M2[s] + dl * (Tv[s] - mean[s]);
      }
    }
  }
#pragma unroll
  for (int s = 0; s < NS_; ++s) {
    nmc_ppc_state a;
    a.n = valid ? k : 0.0;
    a.mean = valid ? mean[s] : 0.0;
    a.M2 = valid ? M2[s] : 0.0;
    a = nmc_ppc_butterfly(a, lane);
    const unsigned sg = nmc_ppc_wave_sum(valid ? gt[s] : 0u);
    const unsigned se = nmc_ppc_wave_sum(valid ? eq[s] : 0u);
    if (lane == 0) {
      sst[w][s][0] = a.n; sst[w][s][1] = a.mean; sst[w][s][2] = a.M2;
      sct[w][s][0] = sg; sct[w][s][1] = se;
    }
  }
  __syncthreads();
  if (threadIdx.x < NS_) {
    const int s = threadIdx.x;
    nmc_ppc_state a = {sst[0][s][0], sst[0][s][1], sst[0][s][2]};
    unsigned sg = sct[0][s][0], se = sct[0][s][1];
    for (int v = 1; v < 4; ++v) {
      const nmc_ppc_state b = {sst[v][s][0], sst[v][s][1], sst[v][s][2]};
      a = nmc_ppc_merge(a, b);
      sg += sct[v][s][0];
      se += sct[v][s][1];
    }
    const size_t at = ((((size_t)sl * gridDim.y + cb) * d.G + g) * NR + j) * NS_ + s;
    gs[at * 3 + 0] = a.n; gs[at * 3 + 1] = a.mean; gs[at * 3 + 2] = a.M2;
    gc[at * 2 + 0] = sg; gc[at * 2 + 1] = se;
  }
}
