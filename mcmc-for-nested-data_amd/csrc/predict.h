// predict.h -- held-out and new-group prediction over the device sample store: the family's
// obs_ll() and predict() evaluated on a table OTHER than the training table, new[n_new][NF]
// in the family's row layout, with a group code per row (nmc_predict_set, nestmc.hip).  The
// reference has no counterpart: its users read the sample files back and draw on the host.
//
// Group codes.  g >= 0: training group g, theta from the store's column q (G + pc) + pc + g as
// nmc_k_waic reads it.  -(k + 1): new group k (partial pooling only, pc = 2), whose theta at
// sample (row r, chain c) is drawn from that sample's hyper-parameters,
//   theta_q = mu_q + sqrt(sigma2_q) z,   mu_q = column q (G + 2), sigma2_q = column q (G + 2) + 1,
//   z = nmc_normal(it = r, group = k, param = q, NMC_PURPOSE_NEW_GROUP, chain_base + c, seed)
// and NaN where sigma2_q is not > 0 or not finite; every observation of new group k shares it
// within a sample (nmc_pred_theta, the one function both kernels form theta with).
//
// The draw.  y_rep of response field j of new observation i (its position in the table):
//   Fam::predict on the block (it = r, group = i, param = j, NMC_PURPOSE_PREDICT_NEW, chain, seed)
// (nmc_pred_draw): a function of (seed, global chain, row, i, j) and theta alone, not of the
// window, the sharding or the launch geometry, and never the in-sample checks' block (ppc.h
// keeps purpose 4).
//
// nmc_k_predict reduces per observation over the samples of a chain block: WAIC's (m, s) of
// ll = obs_ll(theta, new row) (waic.h's recurrence, one exp per term), and per response field
// Welford's (n, mean, M2) and the counts lt = #{y_rep < y}, eq = #{y_rep == y} of y_rep
// (ppc.h's).  A row whose response fields are not all finite has no held-out response: NaN
// compares false, so its counts are 0, its (m, s) are NaN and its ll terms are kept out of the
// non-finite counter.  nmc_k_predict_draws writes the draws, the ll terms and the new groups'
// theta themselves, through the same device functions: both kernels see the same bits.
#pragma once

#include "dev.h"
#include "ppc.h"
#include "rng.h"
#include "waic.h"

// theta_q of a tile's group at one sample from the two words loaded for it: a = the store's
// value (training group) or mu_q (new group), b = sigma2_q (new group only).
__device__ __forceinline__ double nmc_pred_theta(bool isnew, double a, double b, uint32_t r,
                                                 uint32_t k, int q, uint32_t chain,
                                                 uint32_t seed) {
  if (!isnew) return a;
  const double z = nmc_normal(r, k, (uint32_t)q, NMC_PURPOSE_NEW_GROUP, chain, seed);
  const bool ok = b > 0.0 && isfinite(b);
  return ok ? a + sqrt(b) * z : __builtin_nan("");
}

template <class Fam>
__device__ __forceinline__ double nmc_pred_draw(const Fam& fam, const typename Fam::Reg& reg,
                                                const double* __restrict__ row, uint32_t r,
                                                uint32_t i, int j, uint32_t chain, uint32_t seed) {
  if constexpr (Fam::NRESP > 0) {
    const nmc_d2 u = nmc_uniform2(r, i, (uint32_t)j, NMC_PURPOSE_PREDICT_NEW, chain, seed);
    const double z = nmc_box_muller(u.a, u.b);
    return fam.predict(reg, row, j, u.a, u.b, z);
  } else {
    return __builtin_nan("");   // (a family that cannot draw: NRESP = 0, never reached)
  }
}

// all response fields of a row finite (a family that cannot draw names none: every row has one)
template <class Fam>
__device__ __forceinline__ bool nmc_pred_has_response(const double* __restrict__ row) {
  bool has = true;
  if constexpr (Fam::NRESP > 0) {
#pragma unroll
    for (int j = 0; j < Fam::NRESP; ++j) has = has && isfinite(row[Fam::resp_field(j)]);
  }
  return has;
}

// The lane's walk over the window's rows in order for one tile: the 1 (training) or 2 (new
// group) words per parameter of the next row are loaded before this row is consumed, theta is
// formed (for a new group from the P Philox blocks of (row, k)), prepare runs once per row and
// body(r, reg) sees the row's index in the window.
template <class Fam, class Body>
__device__ __forceinline__ void nmc_pred_rows(const Dev& d, const Fam& fam, int code, int pc,
                                              int row0, int nrows, int cc, uint32_t chain,
                                              Body&& body) {
  const bool isnew = code < 0;                      // (wave-uniform: a tile has one code)
  const uint32_t k = (uint32_t)(-(code + 1));
  const size_t rstride = (size_t)d.cols * d.C, qstride = (size_t)(d.G + pc) * d.C;
  const double* col = d.samples + (size_t)row0 * rstride +
                      (isnew ? (size_t)0 : (size_t)(pc + code) * d.C) + cc;
  double an[Fam::MAXP], bn[Fam::MAXP];
#pragma unroll
  for (int q = 0; q < Fam::MAXP; ++q) {
    an[q] = q < d.P ? col[q * qstride] : 0.0;
    bn[q] = q < d.P && isnew ? col[q * qstride + d.C] : 0.0;
  }
  for (int r = 0; r < nrows; ++r) {
    double a[Fam::MAXP], b[Fam::MAXP];
#pragma unroll
    for (int q = 0; q < Fam::MAXP; ++q) { a[q] = an[q]; b[q] = bn[q]; }
    const double* nxt = col + (size_t)(r + 1 < nrows ? r + 1 : r) * rstride;
#pragma unroll
    for (int q = 0; q < Fam::MAXP; ++q) {
      an[q] = q < d.P ? nxt[q * qstride] : 0.0;
      bn[q] = q < d.P && isnew ? nxt[q * qstride + d.C] : 0.0;
    }
    double th[Fam::MAXP];
#pragma unroll
    for (int q = 0; q < Fam::MAXP; ++q)
      th[q] = q < d.P ? nmc_pred_theta(isnew, a[q], b[q], (uint32_t)(row0 + r), k, q, chain, d.seed)
                      : 0.0;
    const typename Fam::Reg reg = fam.prepare(th);
    body(r, reg);
  }
}

// The plain form, for tests and for users with a statistic of their own: one thread per
// (slot i, chain c, row r), grid (ceil(max(n_new, K) / 256), C, nrows).  Slot i < n_new is new
// observation i: yrep[c][r][i][NRESP] and ll[c][r][i].  Slot i < K also writes new group i's
// theta_new[c][r][i][P].  Each of the three arrays may be null.
template <class Fam>
__global__ void __launch_bounds__(256)
nmc_k_predict_draws(Dev d, Fam fam, const double* __restrict__ nobs,
                    const int* __restrict__ ngrp, int64_t n_new, int K, int pc, int row0,
                    int nrows, double* __restrict__ yrep, double* __restrict__ ll,
                    double* __restrict__ theta_new) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int c = (int)blockIdx.y, r = blockIdx.z;
  const uint32_t chain = (uint32_t)(d.chain_base + c), ar = (uint32_t)(row0 + r);
  const size_t qstride = (size_t)(d.G + pc) * d.C;
  const double* row = d.samples + (size_t)(row0 + r) * d.cols * d.C + c;
  if (theta_new && i < K) {   // (K > 0: partial pooling, pc = 2)
    for (int q = 0; q < d.P; ++q)
      theta_new[(((size_t)c * nrows + r) * K + i) * d.P + q] =
          nmc_pred_theta(true, row[q * qstride], row[q * qstride + d.C], ar, (uint32_t)i, q,
                         chain, d.seed);
  }
  if (i >= n_new || (!yrep && !ll)) return;
  const int code = ngrp[i];
  const bool isnew = code < 0;
  const uint32_t k = (uint32_t)(-(code + 1));
  const double* col = row + (isnew ? (size_t)0 : (size_t)(pc + code) * d.C);
  double th[Fam::MAXP];
#pragma unroll
  for (int q = 0; q < Fam::MAXP; ++q) {
    const double a = q < d.P ? col[q * qstride] : 0.0;
    const double b = q < d.P && isnew ? col[q * qstride + d.C] : 0.0;
    th[q] = q < d.P ? nmc_pred_theta(isnew, a, b, ar, k, q, chain, d.seed) : 0.0;
  }
  const typename Fam::Reg reg = fam.prepare(th);
  const double* orow = nobs + i * Fam::NFIELDS;
  const size_t at = ((size_t)c * nrows + r) * n_new + i;
  if (ll) ll[at] = fam.obs_ll(reg, orow);
  if constexpr (Fam::NRESP > 0) {
    if (yrep)
      for (int j = 0; j < Fam::NRESP; ++j)
        yrep[at * Fam::NRESP + j] = nmc_pred_draw(fam, reg, orow, ar, (uint32_t)i, j, chain, d.seed);
  }
}

// The reduction.  nmc_k_waic's launch: grid (ceil(ntiles / 4), CB), 256 threads, wave w of
// workgroup (bx, cb) serves tile 4 bx + w -- at most NMC_WAIC_T consecutive new observations
// with one group code -- for the 64 chains of chain block cb, lane = chain; the new rows are
// wave-uniform reads.  First the density pass (when dens is not null): per observation
// (m, s) of ll by waic.h's recurrence.  Then, per response field j OUTSIDE the row loop as in
// nmc_k_ppc_obs (when st is not null), Welford's (mean, M2) and the counts (lt, eq) of the
// draws: a lane's live state is one pass's worth.  A new group's theta is formed again in
// every pass from the same blocks.  Merge order, fixed:
//   1. a lane's samples in row order;
//   2. the 64 lanes by nmc_waic_merge's butterfly (lane ^ 1 .. ^ 32, the lower lane the A
//      operand; mean and M2 held at 0, so (m, s) are nmc_k_waic's words), nmc_ppc_butterfly and
//      nmc_ppc_wave_sum; chains >= n_valid enter as the identity and read inside the store;
//   3. the chain blocks, engines and ranks on the host (nestmc/predict.py merge).
// Lanes [0, 2 T) store dens[cb][2][n_new] (m, s); per field lanes [0, 3 T) st[cb][3][NRESP][n_new]
// (n, mean, M2) and lanes [0, 2 T) ct[cb][2][NRESP][n_new] (lt, eq).  bad[0]: draws that are not
// finite; bad[1]: ll terms that are not finite at observations WITH a response.  No LDS, no
// barrier, no waiting on another workgroup, no floating-point atomics.
template <class Fam>
__global__ void __launch_bounds__(256)
nmc_k_predict(Dev d, Fam fam, const double* __restrict__ nobs,
              const nmc_waic_tile* __restrict__ tiles, int ntiles, int64_t n_new, int pc, int row0,
              int nrows, int n_valid, double* __restrict__ dens, double* __restrict__ st,
              uint32_t* __restrict__ ct, unsigned long long* bad) {
  constexpr int T = NMC_WAIC_T, NR = Fam::NRESP;
  const int lane = threadIdx.x & 63;
  const int tile = (int)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (tile >= ntiles) return;
  const int cb = blockIdx.y;
  const int64_t start = tiles[tile].start;
  const int code = tiles[tile].g, len = tiles[tile].len;
  const int c = cb * 64 + lane;
  const bool valid = c < n_valid;
  const int cc = valid ? c : n_valid - 1;   // (n_valid <= C: the read stays inside the store)
  const uint32_t chain = (uint32_t)(d.chain_base + cc);
  const bool some = cb * 64 < n_valid;      // (else a chain block of padding only: no rows read)
  // the tile's new rows; a short tile evaluates its last row again and drops it
  const double* orow[T];
  uint32_t oi[T];
#pragma unroll
  for (int t = 0; t < T; ++t) {
    const int64_t i = start + (t < len ? t : len - 1);
    orow[t] = nobs + i * (int64_t)Fam::NFIELDS;
    oi[t] = (uint32_t)i;
  }

  if (dens) {
    double m[T], s[T];
    bool has[T];
#pragma unroll
    for (int t = 0; t < T; ++t) {
      m[t] = -__builtin_huge_val(); s[t] = 0.0;
      has[t] = t < len && nmc_pred_has_response<Fam>(orow[t]);
    }
    unsigned nb = 0;
    if (some)
      nmc_pred_rows(d, fam, code, pc, row0, nrows, cc, chain,
                    [&](int, const typename Fam::Reg& reg) {
#pragma unroll
                      for (int t = 0; t < T; ++t) {
                        const double x = fam.obs_ll(reg, orow[t]);
                        if (!isfinite(x) && has[t]) ++nb;
                        const double dm = x - m[t];
                        const double e = exp(-fabs(dm));
                        s[t] = dm <= 0.0 ? s[t] + e : s[t] * e + 1.0;
                        m[t] = fmax(m[t], x);
                      }
                    });
    if (nb && valid) atomicAdd(bad + 1, (unsigned long long)nb);
    const int sel = lane < 2 * T ? lane : -1;
    double outv = 0.0;
#pragma unroll
    for (int t = 0; t < T; ++t) {
      nmc_waic_state a;
      a.m = valid ? m[t] : -__builtin_huge_val();
      a.s = valid ? s[t] : 0.0;
      a.n = valid ? (double)nrows : 0.0;
      a.mean = 0.0;
      a.M2 = 0.0;
#pragma unroll
      for (int k = 1; k < 64; k <<= 1) {
        nmc_waic_state b;
        b.m = __shfl_xor(a.m, k);
        b.s = __shfl_xor(a.s, k);
        b.n = __shfl_xor(a.n, k);
        b.mean = 0.0;
        b.M2 = 0.0;
        const bool hi = (lane & k) != 0;   // (the lower lane's state is A)
        const nmc_waic_state A = {hi ? b.m : a.m, hi ? b.s : a.s, hi ? b.n : a.n, 0.0, 0.0};
        const nmc_waic_state B = {hi ? a.m : b.m, hi ? a.s : b.s, hi ? a.n : b.n, 0.0, 0.0};
        a = nmc_waic_merge(A, B);
      }
      if (sel == 0 * T + t) outv = a.m;
      if (sel == 1 * T + t) outv = a.s;
    }
    if (sel >= 0 && sel % T < len)
      dens[((size_t)cb * 2 + sel / T) * n_new + start + sel % T] = outv;
  }

  if constexpr (NR > 0) {
    if (!st) return;
    unsigned nbd = 0;
    for (int j = 0; j < NR; ++j) {
      double y[T], mean[T], M2[T];
      unsigned lt[T], eq[T];
#pragma unroll
      for (int t = 0; t < T; ++t) {
        y[t] = orow[t][Fam::resp_field(j)];
        mean[t] = 0.0; M2[t] = 0.0; lt[t] = 0; eq[t] = 0;
      }
      if (some)
        nmc_pred_rows(d, fam, code, pc, row0, nrows, cc, chain,
                      [&](int r, const typename Fam::Reg& reg) {
                        const double ik = 1.0 / (double)(r + 1);
#pragma unroll
                        for (int t = 0; t < T; ++t) {
                          const double x = nmc_pred_draw(fam, reg, orow[t], (uint32_t)(row0 + r),
                                                         oi[t], j, chain, d.seed);
                          const bool fin = isfinite(x);
                          if (!fin && t < len) ++nbd;
                          lt[t] += fin && x < y[t] ? 1u : 0u;
                          eq[t] += fin && x == y[t] ? 1u : 0u;
                          const double dl = x - mean[t];
                          mean[t] = mean[t] + dl * ik;
                          M2[t] = M2[t] + dl * (x - mean[t]);
                        }
                      });
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
        const size_t at = (size_t)j * n_new + start + sel % T;
        st[((size_t)cb * 3 + sel / T) * NR * n_new + at] = outv;
        if (sel < 2 * T) ct[((size_t)cb * 2 + sel / T) * NR * n_new + at] = outc;
      }
    }
    if (nbd && valid) atomicAdd(bad, (unsigned long long)nbd);
  }
}
