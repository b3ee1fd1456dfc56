// waic.h -- WAIC's per-observation reduction over the device sample store (nmc_k_waic).
//
// The widely applicable information criterion needs, per observation i, a log-mean-exp and
// a variance of ll_is over the samples s = (chain, recorded row), where ll_is is the
// per-observation log-likelihood nmc_k_obs_ll_rows evaluates (StepMethod.logLikelihood,
// posteriorSampling.py:656-659, at the recorded values of :890-891).  The [S][n_obs] matrix
// is never formed: every lane keeps, per observation, the combinable state
//   (m, s, n, mean, M2):  m = max ll, s = sum exp(ll - m), n = count, Welford's mean and M2
// over its own chain's rows, and the 64 lanes of a chain block are merged in a fixed order.
// identity (-inf, 0, 0, 0, 0); merge A then B:
//   m = max(mA, mB), s = sA exp(mA - m) + sB exp(mB - m)   (a side with n = 0 contributes 0)
//   d = meanB - meanA, n = nA + nB, mean = meanA + d nB / n, M2 = M2A + M2B + d^2 nA nB / n
// The host (nestmc/waic.py) merges the chain blocks' partials with the same formulas.
#pragma once

#include "dev.h"

// Observations per tile = per-lane states in registers (4 doubles each: n is the row count).
enum { NMC_WAIC_T = 8 };

// A tile: len <= NMC_WAIC_T consecutive observations [start, start + len) of group g.  Tiles
// never straddle a group (theta depends on the group); the table is built once per context.
struct nmc_waic_tile {
  int64_t start;
  int g, len;
};

struct nmc_waic_state { double m, s, n, mean, M2; };

__device__ __forceinline__ nmc_waic_state nmc_waic_merge(const nmc_waic_state& A,
                                                         const nmc_waic_state& B) {
  nmc_waic_state r;
  r.m = fmax(A.m, B.m);
  const double ta = A.n > 0.0 ? A.s * exp(A.m - r.m) : 0.0;
  const double tb = B.n > 0.0 ? B.s * exp(B.m - r.m) : 0.0;
  r.s = ta + tb;
  r.n = A.n + B.n;
  const double d = B.mean - A.mean;
  const bool some = r.n > 0.0;
  r.mean = some ? A.mean + d * B.n / r.n : 0.0;
  r.M2 = some ? A.M2 + B.M2 + d * d * A.n * B.n / r.n : 0.0;
  return r;
}

// Grid (ceil(ntiles / 4), CB), 256 threads: wave w of workgroup (bx, cb) serves tile 4 bx + w
// for the 64 chains of chain block cb, lane = chain.  It walks sample rows
// [row0, row0 + nrows) in order: the lane's theta of (group, chain) from the store (the column
// arithmetic of nmc_k_obs_ll_rows; pc = 2 hyper columns under partial pooling), the next
// row's loads issued before this row is consumed; prepare once; obs_ll of the tile's
// observations, whose rows are wave-uniform reads.  Per term one exp:
//   d = x - m, e = exp(-|d|), s = d <= 0 ? s + e : s e + 1, m = max(m, x)
// and Welford's update with the row's 1 / k.  Then the 64 lanes merge in a butterfly --
// partner lane ^ 1, ^ 2, ^ 4, ^ 8, ^ 16, ^ 32, the lower lane's state the A operand at every
// level -- with chains >= n_valid entering as the identity; every lane ends with the chain
// block's state and lanes [0, 5 T) store part[cb][5][n_obs] (one store, five 64-byte runs).
// Non-finite terms propagate and are counted in *nonfinite.  No LDS, no barrier, no waiting
// on another workgroup: any number of workgroups may be resident.
template <class Fam>
__global__ void __launch_bounds__(256)
nmc_k_waic(Dev d, Fam fam, const double* __restrict__ obs,
           const nmc_waic_tile* __restrict__ tiles, int ntiles, int64_t n_obs, int pc, int row0,
           int nrows, int n_valid, double* __restrict__ part, unsigned long long* nonfinite) {
  constexpr int T = NMC_WAIC_T;
  const int lane = threadIdx.x & 63;
  const int tile = (int)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (tile >= ntiles) return;
  const int cb = blockIdx.y;
  const int64_t start = tiles[tile].start;
  const int g = tiles[tile].g, len = tiles[tile].len;
  const int c = cb * 64 + lane;
  const bool valid = c < n_valid;
  const int cc = valid ? c : n_valid - 1;   // (n_valid <= C: the read stays inside the store)
  // the tile's observation rows; a short tile evaluates its last row again and drops it
  const double* orow[T];
#pragma unroll
  for (int t = 0; t < T; ++t)
    orow[t] = obs + (start + (t < len ? t : len - 1)) * (int64_t)Fam::NFIELDS;

  double m[T], s[T], mean[T], M2[T];
#pragma unroll
  for (int t = 0; t < T; ++t) {
    m[t] = -__builtin_huge_val(); s[t] = 0.0; mean[t] = 0.0; M2[t] = 0.0;
  }
  unsigned bad = 0;
  if (cb * 64 < n_valid) {   // (a chain block of padding only: the identity, no rows read)
    const size_t rstride = (size_t)d.cols * d.C, qstride = (size_t)(d.G + pc) * d.C;
    const double* col = d.samples + (size_t)row0 * rstride + (size_t)(pc + g) * d.C + cc;
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
        const double x = fam.obs_ll(reg, orow[t]);
        if (!isfinite(x) && t < len) ++bad;
        const double dm = x - m[t];
        const double e = exp(-fabs(dm));
        s[t] = dm <= 0.0 ? s[t] + e : s[t] * e + 1.0;
        m[t] = fmax(m[t], x);
        const double dl = x - mean[t];
        mean[t] = mean[t] + dl * ik;
        M2[t] = M2[t] + dl * (x - mean[t]);
      }
    }
  }
  if (bad && valid) atomicAdd(nonfinite, (unsigned long long)bad);

  const int sel = lane < 5 * T ? lane : -1;   // lane 5-tuple component sel / T of obs sel % T
  double outv = 0.0;
#pragma unroll
  for (int t = 0; t < T; ++t) {
    nmc_waic_state a;
    a.m = valid ? m[t] : -__builtin_huge_val();
    a.s = valid ? s[t] : 0.0;
    a.n = valid ? (double)nrows : 0.0;
    a.mean = valid ? mean[t] : 0.0;
    a.M2 = valid ? M2[t] : 0.0;
#pragma unroll
    for (int k = 1; k < 64; k <<= 1) {
      nmc_waic_state b;
      b.m = __shfl_xor(a.m, k);
      b.s = __shfl_xor(a.s, k);
      b.n = __shfl_xor(a.n, k);
      b.mean = __shfl_xor(a.mean, k);
      b.M2 = __shfl_xor(a.M2, k);
      const bool hi = (lane & k) != 0;   // (the lower lane's state is A)
      const nmc_waic_state A = {hi ? b.m : a.m, hi ? b.s : a.s, hi ? b.n : a.n,
                                hi ? b.mean : a.mean, hi ? b.M2 : a.M2};
      const nmc_waic_state B = {hi ? a.m : b.m, hi ? a.s : b.s, hi ? a.n : b.n,
                                hi ? a.mean : b.mean, hi ? a.M2 : b.M2};
      a = nmc_waic_merge(A, B);
    }
    if (sel == 0 * T + t) outv = a.m;
    if (sel == 1 * T + t) outv = a.s;
    if (sel == 2 * T + t) outv = a.n;
    if (sel == 3 * T + t) outv = a.mean;
    if (sel == 4 * T + t) outv = a.M2;
  }
  if (sel >= 0 && sel % T < len)
    part[((size_t)cb * 5 + sel / T) * n_obs + start + sel % T] = outv;
}
