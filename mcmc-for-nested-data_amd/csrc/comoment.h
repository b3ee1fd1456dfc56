// comoment.h -- column moments and the centred Gram matrix of all store columns over the device
// sample store (nmc_k_col_moments, nmc_k_comoment, nmc_k_comoment_sum).
//
// Per sample s = (recorded row, chain), S of them, and store column k; nestmc/correlation.py's
// docstring has the definitions:
//   mean[k] = (sum_s x_k) / S       min[k], max[k] by fp64 comparison
//   nonfinite[k] = #{s : x_k is NaN or +-inf}
//   M[k][l] = sum_s fl(x_k - mean[k]) fl(x_l - mean[l])      (fp64, fused multiply-add)
// The reference has no counterpart (its Figure.bivariates only plots random pairs).  No
// floating-point atomics anywhere: every sum runs in an order that the shape (n_rows, cols, C,
// n_valid) alone fixes, so the bits depend on the window's values and that shape only -- not on
// where the window lies in the store and not on what chains >= n_valid hold.
//
// The choices and their reasons:
//   NMC_CM_TILE  64 columns per tile.  A workgroup of 4 waves owns a pair of tiles (ti <= tj);
//     wave w owns the 16 rows [16 w, 16 w + 16) of tile i against all 64 columns of tile j:
//     four 16x16 accumulators of v_mfma_f64_16x16x4_f64 (32 VGPRs), which share one A operand --
//     5 LDS reads (ds_read_b64) per 4 MFMAs, and the four independent accumulators cover the
//     MFMA's dependent latency.
//   NMC_CM_KC    32 chains of one recorded row are staged at a time (8 MFMA k-steps): two
//     tiles of [64 columns][32 chains] are 36 KiB of LDS, and the kernel is held to 128 VGPRs
//     (amdgpu_waves_per_eu(4): the tiles' means wait in LDS, the column offsets are computed at
//     the load; no spill), so four workgroups fit a CU and another workgroup's MFMAs run while
//     this one waits at its barriers; at 184 VGPRs (two per CU) the 765 workgroups of 516
//     columns ran in two rounds.  The next stage's 16 global loads per thread are issued
//     unconditionally and back to back before the current stage's MFMAs and are waited for
//     only when they are centred and written to LDS (register prefetch): with every load
//     under its own bounds branch the compiler waited for each before issuing the next, and
//     the kernel took twice as long.
//   NMC_CM_LD    36 doubles per staged column (32 + 4 of padding): 72 dwords = 8 mod 64 banks.
//     A wave's operand read takes column l & 15 and chain 4 ks + (l >> 4): dword 8 (l & 15) +
//     2 (l >> 4) mod 64 -- every even bank pair twice over the 64 lanes, the floor of a 64-lane
//     8-byte read.  The staging writes are 32 consecutive doubles per column: conflict-free.
//   NMC_CM_SLICE_ROWS  12 recorded rows per K-slice (times the smallest integer that keeps the
//     slices within NMC_CM_MAX_SLICES = 64): 200 rows give 17 slices, so the 6 tile pairs of
//     132 columns are 102 workgroups and the 45 pairs of 516 columns 765, against 256 CUs; a
//     slice still has 12 rows x (n_valid / 32) stages to amortise its start and its 32 KiB
//     partial tile.  Scratch is nslice cols^2 doubles (at most 64 M's).
#pragma once

#include <stdint.h>

enum { NMC_CM_TILE = 64, NMC_CM_KC = 32, NMC_CM_LD = 36, NMC_CM_SLICE_ROWS = 12,
       NMC_CM_MAX_SLICES = 64, NMC_CM_THREADS = 256, NMC_CM_ROWBLK = 8 };

// Rows per K-slice for a window of n_rows rows: a multiple of NMC_CM_SLICE_ROWS, the smallest
// that needs no more than max_slices slices (max_slices >= 1).
static inline int nmc_cm_slice_rows(int n_rows, int max_slices) {
  const int64_t per = (int64_t)NMC_CM_SLICE_ROWS * max_slices;
  return (int)(NMC_CM_SLICE_ROWS * ((n_rows + per - 1) / per));
}

// Pass 1.  Grid cols, 256 threads: workgroup k reduces column k over rows [row0, row0 + nrows)
// and chains [0, n_valid).  Thread t walks the rows in blocks of NMC_CM_ROWBLK = 8 (8 loads in
// flight: one load at a time left the kernel waiting on memory latency); within a block it
// takes its chains t, t + 256, ... in order and adds, per chain, the block's rows in order into
// one accumulator (a thread without a chain holds +0.0); the 256 accumulators are then added
// by a binary tree in LDS (t += t + 128, t += t + 64, ... t += t + 1).  min and max go the
// same way by "<" and ">"; the non-finite count is an integer.  A column with a non-finite
// value gets mean = NaN.  Chains >= n_valid are never read (a block's rows past the window
// read the window's last row again and are not used).
__global__ void __launch_bounds__(NMC_CM_THREADS)
nmc_k_col_moments(const double* __restrict__ samples, int C, int cols, int row0, int nrows,
                  int n_valid, double* __restrict__ mean, double* __restrict__ minmax,
                  unsigned long long* __restrict__ nonfinite) {
  __shared__ double s_sum[NMC_CM_THREADS], s_min[NMC_CM_THREADS], s_max[NMC_CM_THREADS];
  __shared__ unsigned long long s_bad;
  const int t = (int)threadIdx.x, k = (int)blockIdx.x;
  if (t == 0) s_bad = 0;
  const double* col = samples + ((size_t)row0 * cols + k) * C;
  const size_t rstride = (size_t)cols * C;
  double sum = 0.0, mn = __builtin_huge_val(), mx = -__builtin_huge_val();
  unsigned long long bad = 0;
  for (int rb = 0; rb < nrows; rb += NMC_CM_ROWBLK) {
    for (int c = t; c < n_valid; c += NMC_CM_THREADS) {
      double v[NMC_CM_ROWBLK];
#pragma unroll
      for (int i = 0; i < NMC_CM_ROWBLK; ++i)
        v[i] = col[(size_t)(rb + i < nrows ? rb + i : nrows - 1) * rstride + c];
#pragma unroll
      for (int i = 0; i < NMC_CM_ROWBLK; ++i)
        if (rb + i < nrows) {
          sum += v[i];
          mn = v[i] < mn ? v[i] : mn;
          mx = v[i] > mx ? v[i] : mx;
          if (!(__builtin_fabs(v[i]) < __builtin_huge_val())) ++bad;
        }
    }
  }
  s_sum[t] = sum; s_min[t] = mn; s_max[t] = mx;
  __syncthreads();
  if (bad) atomicAdd(&s_bad, bad);     // (an integer: the order does not matter)
  for (int h = NMC_CM_THREADS / 2; h >= 1; h >>= 1) {
    if (t < h) {
      s_sum[t] += s_sum[t + h];
      s_min[t] = s_min[t + h] < s_min[t] ? s_min[t + h] : s_min[t];
      s_max[t] = s_max[t + h] > s_max[t] ? s_max[t + h] : s_max[t];
    }
    __syncthreads();
  }
  if (t == 0) {
    const double S = (double)nrows * (double)n_valid;
    mean[k] = s_bad ? __builtin_nan("") : s_sum[0] / S;
    minmax[k] = s_min[0];
    minmax[cols + k] = s_max[0];
    nonfinite[k] = s_bad;
  }
}

// Pass 2.  Grid (npair, nslice), 256 threads, npair = nt (nt + 1) / 2 tile pairs ti <= tj in
// row-major order of the upper triangle, nt = ceil(cols / 64).  Workgroup (pair; z) adds, over
// rows [row0 + z rps, row0 + min(nrows, (z + 1) rps)) in order and within a row over the chain
// chunks [32 b, 32 b + 32), b = 0 .. ceil(n_valid / 32) - 1, in order, the products of the
// centred values of tile i's and tile j's columns: per chunk 8 MFMA k-steps of 4 chains each,
// in order.  Staging: thread t takes chain t & 31 of the chunk and columns (t >> 5) + 8 q, q =
// 0..7, of each tile; the value is x - mean[col], and +0.0 for a chain >= n_valid or a column
// >= cols (neither is read).  Operands: lane l gives A[i = l & 15][k = l >> 4] and B[k = l >> 4]
// [j = l & 15], one double each; result register u of a lane is D[row (l >> 4) + 4 u]
// [col l & 15] (the f64 map, not the f32 one).  The partial tile goes to scratch[z][cols][cols]
// (entries inside the matrix only); nothing else is written.  No spin, no waiting on another
// workgroup.
typedef double nmc_cm_d4 __attribute__((ext_vector_type(4)));

__global__ void __launch_bounds__(NMC_CM_THREADS) __attribute__((amdgpu_waves_per_eu(4)))
nmc_k_comoment(const double* __restrict__ samples, int C, int cols, int nt, int row0,
               int nrows, int rps, int n_valid, const double* __restrict__ mean,
               double* __restrict__ scratch) {
  constexpr int T = NMC_CM_TILE, KC = NMC_CM_KC, LD = NMC_CM_LD, NQ = T / 8;
  __shared__ double lds[2][T * LD];
  __shared__ double lmean[2 * T];               // the means of tile i's, then tile j's columns
  const int t = (int)threadIdx.x;
  const int lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  // the pair's tiles: pair index -> (ti, tj), ti <= tj
  int ti = 0, rest = (int)blockIdx.x;
  while (rest >= nt - ti) { rest -= nt - ti; ++ti; }
  const int tj = ti + rest;
  const bool diag = ti == tj;
  const int ci0 = ti * T, cj0 = tj * T;
  const int r0 = (int)blockIdx.y * rps;
  const int r1 = nrows < r0 + rps ? nrows : r0 + rps;
  const int nb = (n_valid + KC - 1) / KC;
  const int nstage = (r1 - r0) * nb;

  const int sc = t & (KC - 1), sq = t >> 5;     // staged chain of the chunk, first column
  // Every staging load is unconditional (a column >= cols reads column cols - 1, a chain >=
  // n_valid chain 0 of its chunk's row: both inside the store) and the value is replaced by
  // +0.0 when it is written to LDS: a load under a branch of its own would be waited for
  // before the next is issued.  The tiles' means wait in LDS and the column offsets are
  // computed at the load, so that the kernel fits 128 VGPRs (4 workgroups per CU).
  if (t < 2 * T) {
    const int a = (t < T ? ci0 : cj0 - T) + t;
    lmean[t] = mean[a < cols ? a : cols - 1];
  }
  const size_t rstride = (size_t)cols * C;
  double vi[NQ], vj[NQ];
  bool cv_next = false;
  auto load = [&](int stage) {
    const int r = row0 + r0 + stage / nb, c = (stage % nb) * KC + sc;
    cv_next = c < n_valid;
    const double* row = samples + (size_t)r * rstride + (cv_next ? c : (stage % nb) * KC);
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const int a = ci0 + sq + 8 * q;
      vi[q] = row[(size_t)(a < cols ? a : cols - 1) * C];
    }
    if (!diag) {
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
        const int a = cj0 + sq + 8 * q;
        vj[q] = row[(size_t)(a < cols ? a : cols - 1) * C];
      }
    }
  };

  nmc_cm_d4 acc[4];
#pragma unroll
  for (int b = 0; b < 4; ++b) acc[b] = nmc_cm_d4{0.0, 0.0, 0.0, 0.0};
  const double* la = lds[0] + (wave * 16 + (lane & 15)) * LD + (lane >> 4);
  const double* lb = lds[diag ? 0 : 1] + (lane & 15) * LD + (lane >> 4);

  if (nstage > 0) load(0);
  __syncthreads();                              // lmean
  for (int stage = 0; stage < nstage; ++stage) {
    const bool cv = cv_next;
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const int k = sq + 8 * q;
      lds[0][k * LD + sc] = (cv && ci0 + k < cols) ? vi[q] - lmean[k] : 0.0;
      if (!diag) lds[1][k * LD + sc] = (cv && cj0 + k < cols) ? vj[q] - lmean[T + k] : 0.0;
    }
    __syncthreads();
    if (stage + 1 < nstage) load(stage + 1);
#pragma unroll
    for (int ks = 0; ks < KC / 4; ++ks) {
      const double a = la[ks * 4];
#pragma unroll
      for (int b = 0; b < 4; ++b)
        acc[b] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, lb[b * 16 * LD + ks * 4], acc[b], 0, 0, 0);
    }
    __syncthreads();
  }

  double* out = scratch + (size_t)blockIdx.y * cols * cols;
#pragma unroll
  for (int b = 0; b < 4; ++b) {
    const int l = cj0 + b * 16 + (lane & 15);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int k = ci0 + wave * 16 + (lane >> 4) + 4 * u;
      if (k < cols && l < cols) out[(size_t)k * cols + l] = acc[b][u];
    }
  }
}

// The slice sum.  Thread (k, l), k <= l, adds scratch[z][k][l], z = 0 .. nslice - 1, in that
// order, and writes the sum to M[k][l] and M[l][k] (the same bits).  A column with a non-finite
// value makes its row and column NaN; otherwise a constant column (min == max) makes them +0.0.
__global__ void __launch_bounds__(NMC_CM_THREADS)
nmc_k_comoment_sum(const double* __restrict__ scratch, int cols, int nslice,
                   const double* __restrict__ minmax,
                   const unsigned long long* __restrict__ nonfinite, double* __restrict__ M) {
  const int l = (int)(blockIdx.x * blockDim.x + threadIdx.x), k = (int)blockIdx.y;
  if (l >= cols || l < k) return;
  const size_t n = (size_t)cols * cols, o = (size_t)k * cols + l;
  double s = scratch[o];
  for (int z = 1; z < nslice; ++z) s += scratch[z * n + o];
  if (nonfinite[k] || nonfinite[l]) s = __builtin_nan("");
  else if (minmax[k] == minmax[cols + k] || minmax[l] == minmax[cols + l]) s = 0.0;
  M[o] = s;
  M[(size_t)l * cols + k] = s;
}
