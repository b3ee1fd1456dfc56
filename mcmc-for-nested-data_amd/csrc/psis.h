// psis.h -- Pareto-smoothed importance sampling of one observation's leave-one-out weights
// over its sorted log-likelihood column (nmc_k_psis; nmc_loo and nmc_psis_of in nestmc.hip).
//
// The definitions are nestmc/loo.py's docstring (Vehtari, Gelman, Gabry 2017; the generalised
// Pareto fit of Zhang and Stephens 2009 as loo / arviz `gpdfitnew` write it).  Observation i
// has S = n_rows * n_valid values ll_s; sortcol.h has sorted their keys ascending, so position
// p holds the (p + 1)-th smallest ll.  With llmin = ll[0] the raw log-weight of position p is
//   r_p = llmin - ll_p <= 0        (one fp64 subtraction; r_0 = 0, r falls with p)
// and everything PSIS needs in order is the head [0, M], M = ceil(min(S / 5, 3 sqrt(S))):
//   cut = max(r_M, log(DBL_MIN)),  n2 = #{p < M : r_p > cut},  tail_j = r_{n2 - 1 - j}
// The rest of the column enters through sums only.  Every quantity depends on the multiset
// of the column's values alone.
//
// Mapping: one 256-thread workgroup per observation.  The tail's x_j = exp(tail_j) - exp(cut)
// lies in LDS as consecutive doubles, thread t reading x[t], x[t + 256], ...: the lanes of a
// ds_read_b64 fall on consecutive bank pairs.  The m = 30 + floor(sqrt(n2)) profile sums
// sum_t log1p(-b_j x_t) run NMC_PSIS_GP grid points at a time -- one read of x_t feeds all of
// them and one reduction (two barriers) serves all of them.  Every reduction is a per-thread
// sum over t = tid, tid + 256, ... in ascending order, then the xor butterfly over the 64 lanes
// (IEEE addition commutes: every lane holds the same bits) and ((w0 + w1) + (w2 + w3)) over
// the four waves: its order depends on the trip counts, that is on (S, n2), alone.  No spins,
// no waiting on another workgroup, no co-residency requirement.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sortcol.h"

enum { NMC_PSIS_THREADS = 256, NMC_PSIS_GP = 8, NMC_PSIS_MAXTAIL = 8191, NMC_PSIS_MAXM = 128 };
static_assert(NMC_PSIS_MAXM % NMC_PSIS_GP == 0, "whole passes over the grid points");
// log(DBL_MIN) as loo.py has it: numpy.log(numpy.finfo(float).tiny)
#define NMC_PSIS_LOG_TINY (-708.3964185322641)
#define NMC_PSIS_EPS 2.220446049250313e-16

// M of S values (host and device): ceil(min(S / 5, 3 sqrt(S))) in fp64 as loo.py computes it
__host__ __device__ __forceinline__ int64_t nmc_psis_m(int64_t S) {
  const double a = (double)S / 5.0, b = 3.0 * sqrt((double)S);
  return (int64_t)ceil(a < b ? a : b);
}

struct nmc_psis_add { __device__ double operator()(double a, double b) const { return a + b; } };
struct nmc_psis_max { __device__ double operator()(double a, double b) const { return a > b ? a : b; } };

// The workgroup's reduction of NV values per thread (red: [4][NV] doubles of LDS); every
// thread returns with the results in v.  Two barriers.
template <int NV, class Op>
__device__ __forceinline__ void nmc_psis_reduce(double (&v)[NV], double* red, int tid, Op op) {
#pragma unroll
  for (int k = 1; k < 64; k <<= 1) {
#pragma unroll
    for (int i = 0; i < NV; ++i) v[i] = op(v[i], __shfl_xor(v[i], k));
  }
  const int w = tid >> 6;
  if ((tid & 63) == 0) {
#pragma unroll
    for (int i = 0; i < NV; ++i) red[w * NV + i] = v[i];
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < NV; ++i)
    v[i] = op(op(red[i], red[NV + i]), op(red[2 * NV + i], red[3 * NV + i]));
  __syncthreads();   // (red may be written again)
}

// Grid (observations of the batch), 256 threads, M doubles of dynamic LDS.  keys[batch][S]: the
// sorted key columns; nonfinite, elpd, lppd, khat, ntail, bad: the batch's entries (index
// blockIdx.x).  An observation with values that are not finite gets NaN results and k = NaN.
__global__ void __launch_bounds__(NMC_PSIS_THREADS)
nmc_k_psis(const uint64_t* __restrict__ keys, int64_t S, int M,
           const unsigned long long* __restrict__ nonfinite, double* __restrict__ elpd,
           double* __restrict__ lppd, double* __restrict__ khat, int* __restrict__ ntail,
           int64_t* __restrict__ bad) {
  extern __shared__ __attribute__((aligned(16))) double xs[];   // [M] the tail's x, then its lw
  __shared__ double red[4 * NMC_PSIS_GP];
  __shared__ double bs[NMC_PSIS_MAXM], Ls[NMC_PSIS_MAXM], ws[NMC_PSIS_MAXM];
  constexpr int NT = NMC_PSIS_THREADS;
  const int tid = threadIdx.x;
  const size_t col = blockIdx.x;
  const uint64_t* s = keys + col * (size_t)S;
  const unsigned long long nbad = nonfinite[col];
  if (nbad != 0) {   // (the whole workgroup)
    if (tid == 0) {
      const double nan = __longlong_as_double(0x7ff8000000000000ll);
      elpd[col] = nan;
      lppd[col] = nan;
      khat[col] = nan;
      ntail[col] = 0;
      bad[col] = (int64_t)nbad;
    }
    return;
  }
  const double llmin = nmc_sort_value(s[0]), llmax = nmc_sort_value(s[S - 1]);
  const double rM = llmin - nmc_sort_value(s[M]);   // (M < S: the host checked)
  const double cut = rM > NMC_PSIS_LOG_TINY ? rM : NMC_PSIS_LOG_TINY;
  // n2: the head positions strictly above the cutoff (a prefix: r falls with the position)
  int n2;
  {
    double c[1] = {0.0};
    for (int p = tid; p < M; p += NT) c[0] += (llmin - nmc_sort_value(s[p])) > cut ? 1.0 : 0.0;
    nmc_psis_reduce(c, red, tid, nmc_psis_add());
    n2 = (int)c[0];   // (<= 8191: exact)
  }
  const double ecut = exp(cut);
  const int nfit = n2 > 4 ? n2 : 0;   // the positions whose weights are replaced
  double k = __builtin_huge_val();
  if (nfit) {
    const double dn = (double)n2;
    for (int j = tid; j < n2; j += NT)
      xs[j] = exp(llmin - nmc_sort_value(s[n2 - 1 - j])) - ecut;
    __syncthreads();
    int m = 30;
    while ((m - 30 + 1) * (m - 30 + 1) <= n2) ++m;   // 30 + floor(sqrt(n2))
    const double xq = xs[(n2 + 2) / 4 - 1], xn = xs[n2 - 1];
    if (tid < NMC_PSIS_MAXM) {
      double b = 0.0;   // (a grid point past m: log1p(-0 x) = 0, never read)
      if (tid < m) {
        b = 1.0 - sqrt((double)m / ((double)(tid + 1) - 0.5));
        b = b / (3.0 * xq);
        b = b + 1.0 / xn;
      }
      bs[tid] = b;
    }
    __syncthreads();
    // the profile log-likelihood of every grid point, NMC_PSIS_GP of them per pass
    for (int g0 = 0; g0 < m; g0 += NMC_PSIS_GP) {
      double acc[NMC_PSIS_GP], bg[NMC_PSIS_GP];
#pragma unroll
      for (int i = 0; i < NMC_PSIS_GP; ++i) {
        acc[i] = 0.0;
        bg[i] = bs[g0 + i];
      }
      for (int t = tid; t < n2; t += NT) {
        const double x = xs[t];
#pragma unroll
        for (int i = 0; i < NMC_PSIS_GP; ++i) acc[i] += log1p(-bg[i] * x);
      }
      nmc_psis_reduce(acc, red, tid, nmc_psis_add());
      if (tid < NMC_PSIS_GP && g0 + tid < m) {
        double sum = acc[0];
#pragma unroll
        for (int i = 1; i < NMC_PSIS_GP; ++i) sum = tid == i ? acc[i] : sum;
        const double kj = sum / dn;
        Ls[g0 + tid] = dn * (log(-bs[g0 + tid] / kj) - kj - 1.0);
      }
    }
    __syncthreads();
    if (tid < NMC_PSIS_MAXM) {
      double w = 0.0;
      if (tid < m) {
        const double Lj = Ls[tid];
        double a = 0.0;
        for (int i = 0; i < m; ++i) a += exp(Ls[i] - Lj);
        w = 1.0 / a;
      }
      ws[tid] = w;
    }
    __syncthreads();
    // weights below 10 eps dropped, the others renormalised; b their mean of the grid (every
    // thread the same serial sums over LDS broadcasts)
    double wsum = 0.0;
    for (int j = 0; j < m; ++j) {
      const double w = ws[j];
      if (w >= 10.0 * NMC_PSIS_EPS) wsum += w;
    }
    double b = 0.0;
    for (int j = 0; j < m; ++j) {
      const double w = ws[j];
      if (w >= 10.0 * NMC_PSIS_EPS) b += bs[j] * (w / wsum);
    }
    double kp[1] = {0.0};
    for (int t = tid; t < n2; t += NT) kp[0] += log1p(-b * xs[t]);
    nmc_psis_reduce(kp, red, tid, nmc_psis_add());
    const double k1 = kp[0] / dn;
    const double sigma = -k1 / b;
    k = (dn * k1 + 5.0) / (dn + 10.0);
    // the smoothed tail replaces x in LDS (the reduction's barriers lie behind every read of x)
    for (int j = tid; j < n2; j += NT) {
      const double p = ((double)j + 0.5) / dn;
      const double l1 = log1p(-p);
      const double q = fabs(k) < NMC_PSIS_EPS ? -sigma * l1 : sigma * expm1(-k * l1) / k;
      const double lw = log(q + ecut);
      xs[j] = lw > 0.0 ? 0.0 : lw;   // (a NaN stays a NaN)
    }
    // (each thread reads back its own places only: no barrier)
  }
  // the two shifts: the largest log-weight, and the largest lw + ll
  double mx[2] = {llmin - nmc_sort_value(s[nfit]), llmin};   // (the body's first; its lw + ll)
  for (int j = tid; j < nfit; j += NT) {
    const double lw = xs[j];
    const double a = lw + nmc_sort_value(s[nfit - 1 - j]);
    mx[0] = lw > mx[0] ? lw : mx[0];
    mx[1] = a > mx[1] ? a : mx[1];
  }
  nmc_psis_reduce(mx, red, tid, nmc_psis_max());
  // sums: the tail's exp(lw - D) and exp(lw + ll - N), the body's exp(r - D), all exp(ll - max)
  double sm[4] = {0.0, 0.0, 0.0, 0.0};
  for (int j = tid; j < nfit; j += NT) {
    const double lw = xs[j];
    sm[0] += exp(lw - mx[0]);
    sm[1] += exp(lw + nmc_sort_value(s[nfit - 1 - j]) - mx[1]);
  }
  for (int64_t p = nfit + tid; p < S; p += NT) sm[2] += exp(llmin - nmc_sort_value(s[p]) - mx[0]);
  for (int64_t p = tid; p < S; p += NT) sm[3] += exp(nmc_sort_value(s[p]) - llmax);
  nmc_psis_reduce(sm, red, tid, nmc_psis_add());
  if (tid == 0) {
    // the body's lw + ll is llmin at every position: (S - nfit) exp(llmin - N)
    const double num = mx[1] + log(sm[1] + (double)(S - nfit) * exp(llmin - mx[1]));
    const double den = mx[0] + log(sm[0] + sm[2]);
    elpd[col] = num - den;
    lppd[col] = llmax + log(sm[3] / (double)S);
    khat[col] = k;
    ntail[col] = n2;
    bad[col] = 0;
  }
}
