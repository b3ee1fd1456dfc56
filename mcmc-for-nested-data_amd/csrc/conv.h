// conv.h -- convergence diagnostics' partial sums over the device sample store (nmc_k_conv).
//
// R-hat and the effective sample size (Diagnostic._assess; sampleDiagnosis.py:158-255) need,
// per column k and half-chain (chain c, half h -- the reference's split :136-155 of a chain's
// rows into [0, n) and [n, 2n)), the mean, the sum of squared deviations and, per lag t, the
// variogram sum of nmc_k_variogram (diag.hip).  Here they are taken from the store
// [row][col][C] as it lies: lane = chain, every row of 64 chains one 512-byte load; no
// transposed copy.  Fixed orders (every product and sum rounded on its own):
//   mean = (x[0] + x[1] + ... + x[n-1]) / n          row order, one division
//   M2   = sum_q d d,  d = x[q] - mean               row order
//   S[t] = sum_{q=0}^{n-t-1} d d,  d = x[q+t] - x[q] q ascending; S[0] = 0
// and per (chain block, column, lag) the 64 chains x 2 halves of S[t] added as a balanced
// binary tree over the 128 leaves (chain, half), half minor: a lane's two halves first, then
// lane l with l ^ 1, 2, 4, 8, 16, 32.  Chains >= n_valid enter as +0.0.
#pragma once

#include <hip/hip_runtime.h>

// Lags per task = per-lane accumulators, and the rows of one unrolled block.
enum { NMC_CONV_L = 8 };

// A lane's reads of consecutive rows of one half: next() returns x[clamp(q, 0, n - 1)] and
// steps to row q + 1.  The pointer moves by one row stride while 0 <= q < n - 1 and stands
// still otherwise, so it never leaves the half whatever is prefetched, and no load pays a
// multiplication.
struct nmc_conv_rows {
  const double* p;   // the lane's x[clamp(q, 0, n - 1)]
  size_t rstride;
  int q, nm1;
  __device__ __forceinline__ nmc_conv_rows(const double* xh, size_t rs, int q0, int n)
      : p(xh + (size_t)(q0 < 0 ? 0 : q0 > n - 1 ? n - 1 : q0) * rs), rstride(rs), q(q0),
        nm1(n - 1) {}
  __device__ __forceinline__ double next() {
    const double v = *p;
    p += (unsigned)q < (unsigned)nm1 ? rstride : 0;
    ++q;
    return v;
  }
};

// One unrolled block of L rows q = qb + i against lags t0 + j, all L x L terms valid (FIRST:
// rows with q < 0 are the alignment's padding and are skipped).  a[i] = x[q], the window
// W = (V0, V1), W[s] = x[qb + t0 + s]: row i reads W[i .. i + L - 1].  a[i] and V0[i] are dead
// after row i: the next block's a and the block after's V1 are loaded into them there, a
// block of arithmetic ahead of their first use.  The caller swaps V0 and V1 from block to
// block: no register is moved.
template <bool FIRST>
__device__ __forceinline__ void nmc_conv_block(double (&acc)[NMC_CONV_L], double (&a)[NMC_CONV_L],
                                               double (&V0)[NMC_CONV_L], double (&V1)[NMC_CONV_L],
                                               int qb, nmc_conv_rows& ra, nmc_conv_rows& rw) {
  constexpr int L = NMC_CONV_L;
#pragma unroll
  for (int i = 0; i < L; ++i) {
    if (!FIRST || qb + i >= 0) {
#pragma unroll
      for (int j = 0; j < L; ++j) {
        const int s = i + j;   // (static after unrolling)
        const double d = (s < L ? V0[s < L ? s : 0] : V1[s < L ? 0 : s - L]) - a[i];
        acc[j] = acc[j] + d * d;
      }
    }
    a[i] = ra.next();    // x[qb + L + i]
    V0[i] = rw.next();   // x[qb + t0 + 2 L + i]
  }
}

// The last L - 1 rows q = qb + i of a lag block: lag t0 + j has a term while i + j < L - 1
// (q + t0 + j <= n - 1).  Rows with q < 0 (fewer than L - 1 rows in all) are skipped.
__device__ __forceinline__ void nmc_conv_tail(double (&acc)[NMC_CONV_L],
                                              const double (&a)[NMC_CONV_L],
                                              const double (&V)[NMC_CONV_L], int qb) {
  constexpr int L = NMC_CONV_L;
#pragma unroll
  for (int i = 0; i < L - 1; ++i) {
    if (qb + i >= 0) {
#pragma unroll
      for (int j = 0; j < L - 1 - i; ++j) {
        const double d = V[i + j] - a[i];
        acc[j] = acc[j] + d * d;
      }
    }
  }
}

// Grid ((nlb + 1) * cols, CB), 64 threads; nlb = ceil((n - 1) / L).  Workgroup (w * cols + k,
// cb) is one wave, for column k and the 64 chains of chain block cb, both halves.  w = 0: the
// means and M2 (two dependent passes over the rows: latency, not arithmetic, so they start
// first, beside the lag tasks) and S[0] = 0.  w = m + 1: lags t0 .. t0 + L - 1, t0 = 1 + m L;
// the longest lag tasks (m = 0) have the lowest ids and start first, and the dispatcher
// balances the rest.  Lag t0 + j has terms for q < n - t0 - j.  With
// Rp = n - t0 - L + 1: rows [0, Rp) have all L lags (blocks of L rows, the first one padded in
// front so that the last ends at Rp), rows [Rp, Rp + L - 1) the staircase of nmc_conv_tail.
// Every row read is clamped into [0, n) (nmc_conv_rows): no read leaves the half, whatever is
// prefetched.
// No LDS, no atomics, no waiting on another workgroup.
//   vg[CB][cols][n], mean[cols][2][C], m2[cols][2][C]  (chains >= n_valid: +0.0)
__global__ void __launch_bounds__(64)
nmc_k_conv(const double* __restrict__ samples, int C, int cols, int row0, int n, int n_valid,
           double* __restrict__ vg, double* __restrict__ mean, double* __restrict__ m2) {
  constexpr int L = NMC_CONV_L;
  const int lane = threadIdx.x;
  const int m = (int)(blockIdx.x / (unsigned)cols) - 1, k = (int)(blockIdx.x % (unsigned)cols);
  const int cb = blockIdx.y;
  const int c = cb * 64 + lane;
  const bool valid = c < n_valid;
  const bool any = cb * 64 < n_valid;   // (a chain block of padding only reads nothing)
  const int cc = valid ? c : n_valid - 1;   // (n_valid <= C: the read stays inside the store)
  const size_t rstride = (size_t)cols * C;
  const double* base = samples + (size_t)row0 * rstride + (size_t)k * C + cc;
  double* o = vg + ((size_t)cb * cols + k) * n;

  if (m < 0) {
#pragma unroll 1
    for (int h = 0; h < 2; ++h) {
      double mu = 0.0, M2 = 0.0;
      if (any) {
        const double* xh = base + (size_t)h * n * rstride;
        double s = xh[0];
#pragma unroll 8
        for (int q = 1; q < n; ++q) s = s + xh[(size_t)q * rstride];
        mu = s / (double)n;
        const double d0 = xh[0] - mu;
        M2 = d0 * d0;
#pragma unroll 8
        for (int q = 1; q < n; ++q) {
          const double d = xh[(size_t)q * rstride] - mu;
          M2 = M2 + d * d;
        }
      }
      if (c < C) {
        mean[((size_t)k * 2 + h) * C + c] = valid ? mu : 0.0;
        m2[((size_t)k * 2 + h) * C + c] = valid ? M2 : 0.0;
      }
    }
    if (lane == 0) o[0] = 0.0;
    return;
  }
  const int t0 = 1 + m * L;

  double tot[L];
#pragma unroll
  for (int j = 0; j < L; ++j) tot[j] = 0.0;
  if (any) {
    const int Rp = n - t0 - L + 1;
    const int off = Rp > 0 ? (L - Rp % L) % L : 0;
    const int NB = Rp > 0 ? (Rp + off) / L : 0;
#pragma unroll 1
    for (int h = 0; h < 2; ++h) {
      const double* xh = base + (size_t)h * n * rstride;
      double acc[L], a[L], V0[L], V1[L];
      int qb = Rp > 0 ? -off : Rp;
      nmc_conv_rows ra(xh, rstride, qb, n), rw(xh, rstride, qb + t0, n);
#pragma unroll
      for (int i = 0; i < L; ++i) {
        acc[i] = 0.0;
        a[i] = ra.next();
        V0[i] = rw.next();
      }
#pragma unroll
      for (int i = 0; i < L; ++i) V1[i] = rw.next();
      if (NB > 0) {
        nmc_conv_block<true>(acc, a, V0, V1, qb, ra, rw);
        qb += L;
        int b = 1;
#pragma unroll 1
        for (; b + 2 <= NB; b += 2) {
          nmc_conv_block<false>(acc, a, V1, V0, qb, ra, rw);
          qb += L;
          nmc_conv_block<false>(acc, a, V0, V1, qb, ra, rw);
          qb += L;
        }
        if (b < NB) {
          nmc_conv_block<false>(acc, a, V1, V0, qb, ra, rw);
          qb += L;
          nmc_conv_tail(acc, a, V0, qb);
        } else {
          nmc_conv_tail(acc, a, V1, qb);
        }
      } else {
        nmc_conv_tail(acc, a, V0, qb);
      }
      // the tree's first stage: a chain's two halves
#pragma unroll
      for (int j = 0; j < L; ++j) tot[j] = h == 0 ? acc[j] : tot[j] + acc[j];
    }
  }

  double outv = 0.0;
#pragma unroll
  for (int j = 0; j < L; ++j) {
    double v = valid ? tot[j] : 0.0;
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) v = v + __shfl_xor(v, s);
    if (lane == j) outv = v;
  }
  if (lane < L && t0 + lane < n) o[t0 + lane] = outv;
}
