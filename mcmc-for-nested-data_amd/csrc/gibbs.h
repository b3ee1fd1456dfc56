// gibbs.h -- the Gibbs update of the hyper-parameters in numpy's pairwise order, in every
// form the kernels use: all waves of a workgroup (nmc_hyper), one wave from an LDS copy
// (nmc_hyper_compute), one wave from registers (nmc_hyper_*_reg, nmc_pairwise_reg), streamed
// (nmc_pairwise_stream); and the row split's partial-sum exchange (nmc_split_exchange).
#pragma once

#include "dev.h"
#include "mem.h"

// ---------------------------------------------------------------------------
// Gibbs update of the hyper-parameters after iteration t for chain block cb
// (HyperParameter._updateMean :481-487, _updateVar :489-498, setPrior :273-282),
// cooperatively by ALL threads of the workgroup (contains barriers).
// numpy's pairwise order: leaves of <= 128 groups, each summed as 8 interleaved
// accumulator streams r_j = x_j + x_{j+8} + ... combined ((r0+r1)+(r2+r3))+((r4+r5)+
// (r6+r7)) plus the tail added in sequence; leaves merged in numpy's recursion
// order (d.merge).  One stream per wave-iteration, loads issued together.
// In: values of iteration t ([P][G][C] at src); LDS hyp
//     sigma2/sdm columns of the previous update; LDS hv = {hyper normal, Gamma(a)
//     draw} of iteration t, [p][lane][2].
// Out: LDS hyp mu/sd/lsd/s2; write: global mu/s2/sd/lsd + the sample row of t.
// ---------------------------------------------------------------------------
template <int SRC, bool SQ, int NS = 1>
__device__ __forceinline__ void nmc_hyper_streams(const Dev& d, const double* src, int cc,
                                                  double* lds, const nmc_lds_layout& L,
                                                  int ponly = -1) {
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int W = blockDim.x >> 6;
  const int P = d.P, G = d.G, C = d.C, nl = d.nleaf, ncol = 8 + d.ntail;
  const int per = 8 + (d.ntail ? 1 : 0);
  // the streams of every parameter, or of parameter ponly only
  const int sbeg = ponly < 0 ? 0 : ponly * nl * per;
  const int nst = ponly < 0 ? P * nl * per : (ponly + 1) * nl * per;
  // NS streams per wave-iteration, their loads in flight together
  struct Strm {
    int j, pl, p, m, m8;
    const double* xp;
  };
  auto strm = [&](int s) {
    Strm q;
    q.j = s % per;
    q.pl = s / per;   // pl = p * nleaf + leaf
    const int lf = q.pl % nl;
    q.p = q.pl / nl;
    const int a = nl == 1 ? 0 : d.leaf[lf];
    q.m = nl == 1 ? G : d.leaf[lf + 1] - a;
    q.m8 = q.m >= 8 ? q.m - q.m % 8 : 0;
    // element k of the leaf for this lane's chain
    q.xp = src + ((size_t)q.p * G + a) * C + cc;
    return q;
  };
  const size_t xs = (size_t)C;
  for (int s0 = sbeg + w; s0 < nst; s0 += W * NS) {
    double t[NS][16];
#pragma unroll
    for (int k = 0; k < NS; ++k) {
      const int s = s0 + k * W;
      const Strm q = strm(s < nst ? s : s0);
      const int cnt = s < nst && q.j < 8 ? q.m8 >> 3 : 0;   // <= 16
#pragma unroll
      for (int u = 0; u < 16; ++u)
        t[k][u] = u < cnt ? nmc_ldv<SRC>(q.xp + (size_t)(q.j + 8 * u) * xs) : 0.0;
    }
#pragma unroll
    for (int k = 0; k < NS; ++k) {
      const int s = s0 + k * W;
      if (s >= nst) continue;
      const Strm q = strm(s);
      double* out = lds + (size_t)(L.hst + q.pl * ncol) * 64 + lane;
      const double mu = SQ ? lds[(L.hyp + NMC_HY_MU * P + q.p) * 64 + lane] : 0.0;
      if (q.j < 8) {
        const int cnt = q.m8 >> 3;
        double r = 0.0;
#pragma unroll
        for (int u = 0; u < 16; ++u) {
          if (u < cnt) {
            double v = t[k][u];
            if (SQ) {
              v = v - mu;
              v = v * v;
            }
            r = u == 0 ? v : r + v;
          }
        }
        out[q.j * 64] = r;
      } else {
        for (int u = q.m8; u < q.m; ++u) {
          double v = nmc_ldv<SRC>(q.xp + (size_t)u * xs);
          if (SQ) {
            v = v - mu;
            v = v * v;
          }
          out[(8 + u - q.m8) * 64] = v;
        }
      }
    }
  }
}

__device__ __forceinline__ double nmc_hyper_combine(const Dev& d, double* lds,
                                                    const nmc_lds_layout& L, int p, int lane) {
  const int nl = d.nleaf, ncol = 8 + d.ntail;
  for (int lf = 0; lf < nl; ++lf) {
    const int pl = p * nl + lf;
    const int m = nl == 1 ? d.G : d.leaf[lf + 1] - d.leaf[lf];
    const int m8 = m >= 8 ? m - m % 8 : 0;
    const double* r = lds + (size_t)(L.hst + pl * ncol) * 64 + lane;
    double res = m8 ? ((r[0] + r[64]) + (r[128] + r[192])) + ((r[256] + r[320]) + (r[384] + r[448]))
                    : 0.0;
    for (int u = m8; u < m; ++u) res += r[(8 + u - m8) * 64];
    lds[(L.hleaf + pl) * 64 + lane] = res;
  }
  for (int k = 0; k < d.nmerge; ++k) {
    double* A = lds + (L.hleaf + p * nl + d.merge[2 * k]) * 64 + lane;
    *A = *A + lds[(L.hleaf + p * nl + d.merge[2 * k + 1]) * 64 + lane];
  }
  return lds[(L.hleaf + p * nl) * 64 + lane];
}

// sqrt(sigma2 / G): the sd of the hyper mean's normal draw (eq. 11.12, :485),
// precomputed off the critical path for the next update.
__device__ __forceinline__ void nmc_hyper_sdm(const Dev& d, double* lds, const nmc_lds_layout& L,
                                              int lane) {
  for (int p = 0; p < d.P; ++p)
    lds[(L.hyp + NMC_HY_SDM * d.P + p) * 64 + lane] =
        sqrt(lds[(L.hyp + NMC_HY_S2 * d.P + p) * 64 + lane] / d.G);
}

// Issue the LDS-DMA of the hyper variates of iteration t (waves w = p % nw from
// w0; one 1 KiB block per parameter); the issuing waves drain before the next barrier.
__device__ __forceinline__ void nmc_hyper_variates(const Dev& d, int cb, int t, double* lds,
                                                   const nmc_lds_layout& L, int w0, int nw) {
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int c = nmc_lane_chain(d, cb, lane);
  const int cc = c < d.C ? c : d.C - 1;
  for (int p = w - w0; p >= 0 && p < d.P; p += nw)
    nmc_dma16(d.vh + (((size_t)(t - d.vbase) * d.P + p) * d.C + cc) * 2,
              lds + L.hv * 64 + p * 128);
}

// ponly >= 0: the update of that parameter alone (nmc_k_sweep's Gibbs workgroups, one task
// each).
// NS: streams per wave-iteration with their loads in flight together (1 in the step kernel:
// 2 and 4 measured slower at cfg 4; nmc_k_sweep's four-wave Gibbs workgroups use 4); WT: the
// global hyper state is stored write-through (agent scope: other workgroups read it inside
// the launch).
template <int SRC, int NS = 1, bool WT = false>
__device__ __forceinline__ void nmc_hyper(const Dev& d, const double* src, int cb, int t,
                                          double* lds, const nmc_lds_layout& L, bool write,
                                          int ponly = -1) {
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int W = blockDim.x >> 6;
  const int P = d.P, G = d.G, C = d.C;
  const int c = nmc_lane_chain(d, cb, lane);
  const int cc = c < C ? c : C - 1;
  const bool own = nmc_lane_owns(d, c, lane);
  const int pb = ponly < 0 ? 0 : ponly, pe = ponly < 0 ? P : ponly + 1;
  nmc_hyper_streams<SRC, false, NS>(d, src, cc, lds, L, ponly);
  __syncthreads();
  for (int p = pb + w; p < pe; p += W) {
    const double tot = nmc_hyper_combine(d, lds, L, p, lane);
    const double sdm = lds[(L.hyp + NMC_HY_SDM * P + p) * 64 + lane];
    const double hz = lds[L.hv * 64 + (p * 64 + lane) * 2];
    lds[(L.hyp + NMC_HY_MU * P + p) * 64 + lane] = tot / G + sdm * hz;   // mu ~ N(mean(x), sqrt(s2/G))
  }
  __syncthreads();
  nmc_hyper_streams<SRC, true, NS>(d, src, cc, lds, L, ponly);
  __syncthreads();
  const int row = write ? nmc_record_row(d, t) : -1;
  for (int p = pb + w; p < pe; p += W) {
    const double ss = nmc_hyper_combine(d, lds, L, p, lane);
    const double hat = ss / (double)(G - 1);
    const double scale = d.ha * hat;
    const double hx = lds[L.hv * 64 + (p * 64 + lane) * 2 + 1];
    // scipy invgamma.rvs: (1/gammainccinv(a, U)) * scale + loc; loc when scale == 0
    const double s2n = scale == 0.0 ? 0.0 : (1.0 / hx) * scale;
    const double sdn = sqrt(s2n);
    const double lsd = log(sdn);
    const double m = lds[(L.hyp + NMC_HY_MU * P + p) * 64 + lane];
    lds[(L.hyp + NMC_HY_SD * P + p) * 64 + lane] = sdn;
    lds[(L.hyp + NMC_HY_LSD * P + p) * 64 + lane] = lsd;
    lds[(L.hyp + NMC_HY_S2 * P + p) * 64 + lane] = s2n;
    lds[(L.hyp + NMC_HY_ISD * P + p) * 64 + lane] = 1.0 / sdn;
    if (write && own) {
      const size_t ho = nmc_hslot(d, t) + (size_t)p * C + c;
      if constexpr (WT) {
        __hip_atomic_store(d.mu + ho, m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(d.s2 + ho, s2n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(d.hsd + ho, sdn, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(d.hlsd + ho, lsd, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      } else {
        d.mu[ho] = m;
        d.s2[ho] = s2n;
        d.hsd[ho] = sdn;
        d.hlsd[ho] = lsd;
      }
      if (row >= 0) {
        double* out = d.samples + ((size_t)row * d.cols + (size_t)p * (G + 2)) * C + c;
        out[0] = m;
        out[C] = s2n;
      }
    }
  }
  __syncthreads();
}

// Groups [kb, ke) of the chain block's published values of parameter p (64 chains
// each) -> LDS hval, sc1 loads, 8 in flight (used when C is odd).
__device__ __forceinline__ void nmc_hyper_load(const Dev& d, const double* src, int p, int cc,
                                               int kb, int ke, double* lds,
                                               const nmc_lds_layout& L, int hoff) {
  const int lane = threadIdx.x & 63;
  const int C = d.C;
  src += (size_t)p * d.G * C;
  constexpr int NB = 8;   // the odd-C fallback of the LDS-DMA copy: few registers
  for (int k0 = kb; k0 < ke; k0 += NB) {
    double tv[NB];
#pragma unroll
    for (int u = 0; u < NB; ++u)
      tv[u] = k0 + u < ke ? nmc_ldv<NMC_SRC_SC1>(src + (size_t)(k0 + u) * C + cc) : 0.0;
#pragma unroll
    for (int u = 0; u < NB; ++u)
      if (k0 + u < ke) lds[(size_t)(L.hval + hoff + k0 + u) * 64 + lane] = tv[u];
  }
}

// The same by LDS-DMA (global_load_lds_dwordx4, sc1): one instruction moves two groups'
// 64-chain rows (lanes 0-31 / 32-63, two chains per lane) into two consecutive hval
// columns, so one wave has the whole payload in flight without registers.  Needs C
// even (16-byte rows); an odd group count writes one pad column past ke.  The issuing
// wave retires the copies with s_waitcnt vmcnt(0).
__device__ __forceinline__ void nmc_hyper_dma(const Dev& d, const double* src, int p, int cb,
                                              int kb, int ke, double* lds,
                                              const nmc_lds_layout& L, int hoff) {
  const int lane = threadIdx.x & 63;
  const double* s = src + (size_t)p * d.G * d.C + (size_t)cb * 64 + 2 * (lane & 31);
  for (int k0 = kb; k0 < ke; k0 += 2) {
    const int gk = k0 + (lane >> 5) < ke ? k0 + (lane >> 5) : ke - 1;
    __builtin_amdgcn_global_load_lds((nmc_glb_ptr)(s + (size_t)gk * d.C),
                                     (nmc_lds_ptr)(lds + (size_t)(L.hval + hoff + k0) * 64), 16,
                                     0, 16 /* sc1 */);
  }
}

// The Gibbs update of parameter p after iteration t for this wave's 64 chains, by ONE
// wave, from the LDS copy hval of the chain block's values of p (hv[i * 64]: group i):
// numpy's pairwise sum (8 interleaved streams r_j = x_j + x_{j+8} + ..., combined
// ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)), the G % 8 tail added in order; G < 8: a
// sequential sum from 0; G <= 128: one numpy leaf) for mean(x) and sum((x - mu)^2)
// (HyperParameter._updateMean :481-487, _updateVar :489-498).  Run beside the
// likelihood tiles: reads in bursts of 4 elements per stream (32 in flight, one LDS
// round trip per burst under the tiles' broadcast traffic).  hz/hx: this lane's hyper variates of
// (t, p).  Writes the LDS hyp columns of p (and, if write, the global slot of t and the
// sample row of t).
__device__ __forceinline__ void nmc_hyper_compute(const Dev& d, int cb, int t, int p, double* lds,
                                                  const nmc_lds_layout& L, bool write, double hz,
                                                  double hx, int hoff) {
  const int lane = threadIdx.x & 63;
  const int P = d.P, G = d.G, C = d.C;
  const int c = nmc_lane_chain(d, cb, lane);
  const double* hv = lds + (size_t)(L.hval + hoff) * 64 + lane;   // hv[i * 64]: group i of p
  double* hy = lds + L.hyp * 64 + lane;
  const double sdm = sqrt(hy[(NMC_HY_S2 * P + p) * 64] / G);
  const int m8 = G >= 8 ? G - G % 8 : 0;
  const int cnt = m8 >> 3;   // elements per stream, 0..16
  auto pass = [&](bool sq, double mu) -> double {
    double r[8];
#pragma unroll 1
    for (int e0 = 0; e0 < cnt; e0 += 4) {
      double xv[8][4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int uu = e0 + u < cnt ? e0 + u : cnt - 1;
#pragma unroll
        for (int j = 0; j < 8; ++j) xv[j][u] = hv[(8 * uu + j) * 64];
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        double acc = e0 > 0 ? r[j] : 0.0;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          if (e0 + u < cnt) {
            double x = xv[j][u];
            if (sq) {
              x = x - mu;
              x = x * x;
            }
            acc = e0 + u == 0 ? x : acc + x;
          }
        }
        r[j] = acc;
      }
    }
    double res = cnt ? ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7])) : 0.0;
#pragma unroll 1
    for (int i = m8; i < G; ++i) {   // the G % 8 tail, in order (G < 8: from 0)
      double x = hv[i * 64];
      if (sq) {
        x = x - mu;
        x = x * x;
      }
      res += x;
    }
    return res;
  };
  const double tot = pass(false, 0.0);
  const double mu = tot / G + sdm * hz;                        // mu ~ N(mean(x), sqrt(s2/G))
  const double ss = pass(true, mu);
  const double hat = ss / (double)(G - 1);
  const double scale = d.ha * hat;
  // scipy invgamma.rvs: (1/gammainccinv(a, U)) * scale + loc; loc when scale == 0
  const double s2n = scale == 0.0 ? 0.0 : (1.0 / hx) * scale;
  const double sdn = sqrt(s2n);
  const double lsd = log(sdn);
  hy[(NMC_HY_MU * P + p) * 64] = mu;
  hy[(NMC_HY_SD * P + p) * 64] = sdn;
  hy[(NMC_HY_LSD * P + p) * 64] = lsd;
  hy[(NMC_HY_S2 * P + p) * 64] = s2n;
  hy[(NMC_HY_ISD * P + p) * 64] = 1.0 / sdn;
  if (write && nmc_lane_owns(d, c, lane)) {
    const size_t ho = nmc_hslot(d, t) + (size_t)p * C + c;
    // write-through (sc1): nmc_k_sweep's readers poll for them inside the launch
    __hip_atomic_store(d.mu + ho, mu, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(d.s2 + ho, s2n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(d.hsd + ho, sdn, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(d.hlsd + ho, lsd, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int row = nmc_record_row(d, t);
    if (row >= 0) {
      double* out = d.samples + ((size_t)row * d.cols + (size_t)p * (G + 2)) * C + c;
      out[0] = mu;
      out[C] = s2n;
    }
  }
}

// numpy's pairwise sum (the order of nmc_hyper_compute's pass) over x[0..G) held in
// registers, G <= 64: every index is a compile-time constant, the G-dependent parts
// are wave-uniform branches (cnt blocks of 8, the G % 8 tail picked by m8).
__device__ __forceinline__ double nmc_pairwise_reg(const double (&x)[64], int G, bool sq,
                                                   double mu) {
  const int m8 = G >= 8 ? G - G % 8 : 0;
  const int cnt = m8 >> 3;   // 0..8 blocks of 8
  auto tr = [&](double v) {
    if (sq) {
      v = v - mu;
      v = v * v;
    }
    return v;
  };
  double r[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) r[j] = tr(x[j]);
  if (G == 64) {   // eight full blocks, no tail: no selects (the general path below is
                   // if-converted into a v_cndmask per element and block)
#pragma unroll
    for (int u = 1; u < 8; ++u)
#pragma unroll
      for (int j = 0; j < 8; ++j) r[j] = r[j] + tr(x[8 * u + j]);
    return ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
  }
#pragma unroll
  for (int u = 1; u < 8; ++u)
    if (u < cnt) {
#pragma unroll
      for (int j = 0; j < 8; ++j) r[j] = r[j] + tr(x[8 * u + j]);
    }
  double res = cnt ? ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7])) : 0.0;
  double tv[7];
#pragma unroll
  for (int k = 0; k < 7; ++k) tv[k] = 0.0;
#pragma unroll
  for (int u = 0; u < 8; ++u)
    if (8 * u == m8) {
#pragma unroll
      for (int k = 0; k < 7; ++k) tv[k] = x[8 * u + k < 64 ? 8 * u + k : 63];
    }
  const int nt = G - m8;   // the G % 8 tail, in order (G < 8: the whole sum from 0)
#pragma unroll
  for (int k = 0; k < 7; ++k)
    if (k < nt) res += tr(tv[k]);
  return res;
}

__device__ __forceinline__ void nmc_hyper_finish(const Dev& d, int cb, int t, int p, double* lds,
                                                 int hyp, bool write, double mu, double ss,
                                                 double hx);

// The Gibbs update of parameter p after iteration t for this wave's 64 chains from the
// chain block's values x[0..G) of p in registers (G <= 64); otherwise identical to
// nmc_hyper_compute (same sums in the same order, same draws, same outputs).
// hyp: the LDS column of the hyper state ([6][P] columns, NMC_HY_*).
__device__ __forceinline__ void nmc_hyper_compute_reg(const Dev& d, int cb, int t, int p,
                                                      double* lds, int hyp, bool write,
                                                      double hz, double hx,
                                                      const double (&x)[64]) {
  const int lane = threadIdx.x & 63;
  const int P = d.P, G = d.G;
  double* hy = lds + hyp * 64 + lane;
  const double sdm = sqrt(hy[(NMC_HY_S2 * P + p) * 64] / G);
  const double tot = nmc_pairwise_reg(x, G, false, 0.0);
  const double mu = tot / G + sdm * hz;                        // mu ~ N(mean(x), sqrt(s2/G))
  const double ss = nmc_pairwise_reg(x, G, true, mu);
  nmc_hyper_finish(d, cb, t, p, lds, hyp, write, mu, ss, hx);
}

// mu and sum((x - mu)^2) -> sigma2 draw, LDS hyper state, (write) global slot of t and
// the sample row of t (HyperParameter._updateVar :489-498, setPrior :273-282).
__device__ __forceinline__ void nmc_hyper_finish(const Dev& d, int cb, int t, int p, double* lds,
                                                 int hyp, bool write, double mu, double ss,
                                                 double hx) {
  const int lane = threadIdx.x & 63;
  const int P = d.P, G = d.G, C = d.C;
  const int c = nmc_lane_chain(d, cb, lane);
  double* hy = lds + hyp * 64 + lane;
  const double hat = ss / (double)(G - 1);
  const double scale = d.ha * hat;
  // scipy invgamma.rvs: (1/gammainccinv(a, U)) * scale + loc; loc when scale == 0
  const double s2n = scale == 0.0 ? 0.0 : (1.0 / hx) * scale;
  const double sdn = sqrt(s2n);
  const double lsd = log(sdn);
  hy[(NMC_HY_MU * P + p) * 64] = mu;
  hy[(NMC_HY_SD * P + p) * 64] = sdn;
  hy[(NMC_HY_LSD * P + p) * 64] = lsd;
  hy[(NMC_HY_S2 * P + p) * 64] = s2n;
  hy[(NMC_HY_ISD * P + p) * 64] = 1.0 / sdn;
  if (write && nmc_lane_owns(d, c, lane)) {
    const size_t ho = nmc_hslot(d, t) + (size_t)p * C + c;
    // write-through (sc1): nmc_k_sweep's readers poll for them inside the launch
    __hip_atomic_store(d.mu + ho, mu, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(d.s2 + ho, s2n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(d.hsd + ho, sdn, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(d.hlsd + ho, lsd, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int row = nmc_record_row(d, t);
    if (row >= 0) {
      double* out = d.samples + ((size_t)row * d.cols + (size_t)p * (G + 2)) * C + c;
      out[0] = mu;
      out[C] = s2n;
    }
  }
}

// Poll-free half of the register Gibbs hand-off: the chain block's published values of
// parameter q after iteration tq -> x[0..64) (sc1 loads, all in flight at once: one
// global round trip, no LDS traffic beside the likelihood waves' broadcasts; x[G..64)
// read the buffers' 72-group slack or the next parameter and are never summed), and
// the update's variates {hyper z, gamma}.
__device__ __forceinline__ void nmc_hyper_fetch_reg(const Dev& d, int tq, int q, int cc,
                                                    double (&x)[64], double& hz, double& hx) {
  const int G = d.G, C = d.C;
  const double* src = ((tq & 1) ? d.vb1 : d.vb0) + (size_t)q * G * C + cc;
#pragma unroll
  for (int k = 0; k < 64; ++k) x[k] = nmc_ldv<NMC_SRC_SC1>(src + (size_t)k * C);
  const size_t hvi = (((size_t)(tq - d.vbase) * d.P + q) * C + cc) * 2;
  hz = d.vh[hvi];
  hx = d.vh[hvi + 1];
}

// Row split: member m's partial sums of step k -> xbuf (sc1), counted on the unit's
// counter; once all S members of step k have arrived, every member sums the S partials in
// member order (four interleaved streams m & 3, combined (s0+s1)+(s2+s3)) -- identical in
// every member.  A member is at most one step ahead of the slowest (it cannot pass step
// k+1 before all partials of k+1 exist), so two step-parity slots suffice.  Call with
// the whole (control) wave; bounded spin (d.tmo).
template <int NA>
__device__ __forceinline__ void nmc_split_exchange(const Dev& d, int cb, int g, int m, int k,
                                                   double (&acc)[NA]) {
  const int lane = threadIdx.x & 63;
  const int S = d.S;
  const size_t unit = (size_t)cb * d.G + g;
  double* xb = d.xbuf + (((size_t)((k + d.xbase) & 1) * d.RB * d.G + unit) * S) * NA * 64 + lane;
#pragma unroll
  for (int j = 0; j < NA; ++j)
    __hip_atomic_store(xb + ((size_t)m * NA + j) * 64, acc[j], __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
  nmc_drain_vm();
  unsigned* ctr = d.xcnt + unit * 32;
  if (lane == 0) __hip_atomic_fetch_add(ctr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const unsigned target = (unsigned)S * ((unsigned)k + d.xbase + 1u);
  for (unsigned spins = 0;; ++spins) {
    const unsigned v = __hip_atomic_load(ctr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (v >= target) break;
    if ((spins & 255) == 255 &&
        __hip_atomic_load(d.tmo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != 0)
      break;
    if (spins >= NMC_SPIN_LIMIT) {
      __hip_atomic_store(d.tmo, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      break;
    }
    __builtin_amdgcn_s_sleep(1);
  }
  // keep the partial loads below the poll (no instruction: wavefront scope)
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
  for (int j = 0; j < NA; ++j) {
    double s4[4] = {0.0, 0.0, 0.0, 0.0};
    for (int m0 = 0; m0 < S; m0 += 8) {
      double v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u)
        v[u] = m0 + u < S ? __hip_atomic_load(xb + ((size_t)(m0 + u) * NA + j) * 64,
                                              __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                          : 0.0;
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int mm = m0 + u;
        if (mm < S) s4[mm & 3] = mm < 4 ? v[u] : s4[mm & 3] + v[u];
      }
    }
    acc[j] = S >= 4 ? (s4[0] + s4[1]) + (s4[2] + s4[3])
                    : (S == 1 ? s4[0] : (S == 2 ? s4[0] + s4[1] : (s4[0] + s4[1]) + s4[2]));
  }
}

// numpy's pairwise sum over the chain block's G (64 < G <= 256) values of one parameter,
// streamed from global memory (sc1) in chunks of 64: each numpy leaf (<= 128 values, the
// host plan d.leaf) as 8 interleaved streams carried across chunks plus its tail in
// order, the leaves merged in numpy's recursion order (d.merge) -- the order of
// nmc_hyper_compute and the oracle.  src: the parameter's [G][C] values + this chain.
// CH: values per chunk (loads in flight together, 2 * CH VGPRs).
template <int CH = 64>
__device__ __forceinline__ double nmc_pairwise_stream(const Dev& d, const double* src, bool sq,
                                                      double mu) {
  static_assert(CH % 8 == 0 && CH <= 64, "chunks of whole 8-value blocks");
  const int C = d.C, G = d.G, nl = d.nleaf;
  auto tr = [&](double v) {
    if (sq) {
      v = v - mu;
      v = v * v;
    }
    return v;
  };
  double ls[4] = {0.0, 0.0, 0.0, 0.0};
  for (int lf = 0; lf < nl; ++lf) {
    const int a = nl == 1 ? 0 : d.leaf[lf];
    const int m = nl == 1 ? G : d.leaf[lf + 1] - a;
    const int m8 = m >= 8 ? m - m % 8 : 0;
    double r[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int e0 = 0; e0 < m8; e0 += CH) {
      double x[CH];
#pragma unroll
      for (int k = 0; k < CH; ++k)
        x[k] = e0 + k < m8 ? nmc_ldv<NMC_SRC_SC1>(src + (size_t)(a + e0 + k) * C) : 0.0;
#pragma unroll
      for (int k = 0; k < CH; ++k)
        if (e0 + k < m8) r[k & 7] = e0 + k < 8 ? tr(x[k]) : r[k & 7] + tr(x[k]);
    }
    double res = m8 ? ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7])) : 0.0;
    for (int e = m8; e < m; ++e) res += tr(nmc_ldv<NMC_SRC_SC1>(src + (size_t)(a + e) * C));
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (i == lf) ls[i] = res;
  }
  for (int k = 0; k < d.nmerge; ++k) {   // slot A += slot B
    const int A = d.merge[2 * k], B = d.merge[2 * k + 1];
    double vb = ls[0];
#pragma unroll
    for (int i = 1; i < 4; ++i)
      if (i == B) vb = ls[i];
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (i == A) ls[i] = ls[i] + vb;
  }
  return ls[0];
}

// SYNC_OWN: the hyper-parameters of task (tq, q) as its Gibbs workgroup stored them (global
// slot of tq, sc1 loads) -> this workgroup's LDS hyper state (nmc_hyper_finish's values).
__device__ __forceinline__ void nmc_hyper_read(const Dev& d, int tq, int q, int cc, double* lds,
                                               int hyp) {
  const int lane = threadIdx.x & 63;
  const int P = d.P;
  const size_t ho = nmc_hslot(d, tq) + (size_t)q * d.C + cc;
  const double mu = nmc_ldv<NMC_SRC_SC1>(d.mu + ho), s2 = nmc_ldv<NMC_SRC_SC1>(d.s2 + ho);
  const double sd = nmc_ldv<NMC_SRC_SC1>(d.hsd + ho), lsd = nmc_ldv<NMC_SRC_SC1>(d.hlsd + ho);
  double* hy = lds + hyp * 64 + lane;
  hy[(NMC_HY_MU * P + q) * 64] = mu;
  hy[(NMC_HY_SD * P + q) * 64] = sd;
  hy[(NMC_HY_LSD * P + q) * 64] = lsd;
  hy[(NMC_HY_S2 * P + q) * 64] = s2;
  hy[(NMC_HY_ISD * P + q) * 64] = 1.0 / sd;
}

// The register Gibbs update of task (tq, q) for this wave's 64 chains (G <= 64): one
// 64-value fetch (nmc_hyper_fetch_reg), then nmc_hyper_compute_reg.
__device__ __forceinline__ void nmc_hyper_update_reg(const Dev& d, int cb, int tq, int q, int cc,
                                                     double* lds, int hyp, bool write) {
  double xv[64], fz, fx;
  nmc_hyper_fetch_reg(d, tq, q, cc, xv, fz, fx);
  nmc_hyper_compute_reg(d, cb, tq, q, lds, hyp, write, fz, fx, xv);
}
