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
//
// nmc_k_psis_expect (below) brings the same weights together with one response field's
// replicates for the leave-one-out PIT and predictive moments (nestmc/loopit.py).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sortcol.h"

enum { NMC_PSIS_THREADS = 256, NMC_PSIS_GP = 8, NMC_PSIS_MAXTAIL = 8191, NMC_PSIS_MAXM = 128,
       NMC_PSIS_U = 4 /* nmc_k_psis_expect: samples whose loads are in flight per thread */ };
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
// lw_out (LW; null without): [batch][M], the smoothed tail's log-weights lw_j, j < n2, of every
// observation with n2 > 4 -- what nmc_k_psis_expect reads; the other places are not written.
// The instance without LW never looks at the pointer: it is PSIS-LOO's kernel as it was,
// register for register (nmc_psis_launch picks the instance by the pointer).
template <bool LW>
__global__ void __launch_bounds__(NMC_PSIS_THREADS)
nmc_k_psis(const uint64_t* __restrict__ keys, int64_t S, int M,
           const unsigned long long* __restrict__ nonfinite, double* __restrict__ elpd,
           double* __restrict__ lppd, double* __restrict__ khat, int* __restrict__ ntail,
           int64_t* __restrict__ bad, double* __restrict__ lw_out) {
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
      if constexpr (LW) lw_out[col * (size_t)M + j] = xs[j];
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

// nmc_k_psis over k sorted columns: lw_out null is the instance that keeps the tail in LDS
// alone.  lds > 60 KiB (with the kernel's static 3.3 KiB: past the 64 KiB every launch may
// have) raises the instance's limit first.
static inline hipError_t nmc_psis_launch(hipStream_t st, int k, size_t lds, const uint64_t* keys,
                                         int64_t S, int M, const unsigned long long* nonfinite,
                                         double* elpd, double* lppd, double* khat, int* ntail,
                                         int64_t* bad, double* lw_out) {
  const auto kern = lw_out ? nmc_k_psis<true> : nmc_k_psis<false>;
  if (lds > 60 * 1024) {
    const hipError_t e = hipFuncSetAttribute(
        (const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(kern, dim3((unsigned)k), dim3(NMC_PSIS_THREADS), lds, st, keys, S, M,
                     nonfinite, elpd, lppd, khat, ntail, bad, lw_out);
  return hipGetLastError();
}

// The weight W_s = exp(lw_s - D) of a sample with log-likelihood l (nestmc/loopit.py): the raw
// exp(r - D) at or below the cutoff or with a short tail (nfit = 0), and then lo = hi = 0; else
// the mean of es[j] = exp(lw_tail_j - D) over the tail places [nfit - hi, nfit - lo) of the
// head positions [lo, hi) whose values equal l (hs[p]: the p-th smallest log-likelihood,
// p < nfit; two binary searches; one place unless the tail has ties, and then x / 1.0 is x).
__device__ __forceinline__ double nmc_psis_weight(double l, double llmin, double cut, double D,
                                                  int nfit, const double* hs, const double* es,
                                                  int& lo, int& hi) {
  const double r = llmin - l;
  lo = hi = 0;
  if (nfit == 0 || !(r > cut)) return exp(r - D);
  int n = nfit;                  // the first p with hs[p] >= l
  while (n > 0) {
    const int h = n >> 1;
    const bool right = hs[lo + h] < l;
    lo = right ? lo + h + 1 : lo;
    n = right ? n - h - 1 : h;
  }
  hi = lo;                       // the first p with hs[p] > l
  n = nfit - lo;
  while (n > 0) {
    const int h = n >> 1;
    const bool right = hs[hi + h] <= l;
    hi = right ? hi + h + 1 : hi;
    n = right ? n - h - 1 : h;
  }
  double w = 0.0;
  for (int j = nfit - hi; j < nfit - lo; ++j) w += es[j];   // (ascending places; 0.0 + x = x)
  return w / (double)(hi - lo);
}
// Sample i = q n_valid + c (row q, chain c) for i = tid, tid + 256, ...: one division at the
// start, then a step of (256 / n_valid, 256 % n_valid) with a carry.
struct nmc_psis_walk {
  unsigned q, c, dq, dc, nv;
  __device__ __forceinline__ nmc_psis_walk(int tid, int n_valid)
      : q((unsigned)tid / (unsigned)n_valid), c((unsigned)tid % (unsigned)n_valid),
        dq((unsigned)NMC_PSIS_THREADS / (unsigned)n_valid),
        dc((unsigned)NMC_PSIS_THREADS % (unsigned)n_valid), nv((unsigned)n_valid) {}
  __device__ __forceinline__ void next() {
    q += dq;
    c += dc;
    if (c >= nv) {
      c -= nv;
      ++q;
    }
  }
};
// Is head position p one of several with its value (a tie inside the tail)?
__device__ __forceinline__ bool nmc_psis_tied(const double* hs, int nfit, int p) {
  return (p > 0 && hs[p - 1] == hs[p]) || (p + 1 < nfit && hs[p + 1] == hs[p]);
}

// The leave-one-out expectations of one response field (nestmc/loopit.py has the definitions).
// Grid (observations of the batch), 256 threads, 2 M doubles of dynamic LDS: the head's values
// and exp(lw_tail - D).  ll and yrep: two stores [rows][cols][C] of one shape, the batch's
// observations their columns [col0, col0 + batch), read UNSORTED and in step over rows
// [row_begin, ...) and chains [0, n_valid): sample i = q n_valid + c is row q, chain c, thread
// t takes i = t, t + 256, ... (nmc_psis_walk) -- consecutive lanes on consecutive chains, every
// load a contiguous run, a chain >= n_valid never read.  keys, nonfinite, ntail, lw: what
// sort_columns and nmc_k_psis left for the batch; y[batch]: the observed values.  Two passes over the
// samples in the same order: Z, sum W^2, sum W [yrep < y], sum W [yrep == y], sum W yrep and
// the count of replicates that are not finite; then sum W (yrep - mean)^2.  Every sum by
// nmc_psis_reduce: the bits depend on (n_rows, n_valid, n2) alone.
//
// Ties inside the tail (samples that repeat a log-likelihood: a chain that rejected between two
// recorded rows) share one weight, so which of them carries which replicate must not matter --
// not in the last bit either.  Their replicates therefore leave the sample order: a tied sample
// puts its replicate in a place of its group (tie: [batch][3 M] doubles of scratch -- the
// gathered values, the ordered values, the groups' counters; an integer atomicAdd hands out
// the places), every group is put in the order of its replicates' sort keys (a rank by
// counting: the group's multiset decides, not who came first), and the ordered places join
// the threads' sums after the samples, place p at thread p mod 256.  Only Z and sum W^2, where
// equal weights are equal terms, take the tied samples in sample order.
//
// Results at index blockIdx.x (ess) and blockIdx.x * nresp + j (the others).  An observation
// whose log-likelihoods are not all finite gets NaN everywhere; a field with replicates that
// are not finite gets NaN for wlt, weq, mean and var.  No spins, no waiting on another
// workgroup, no floating-point atomics.
__global__ void __launch_bounds__(NMC_PSIS_THREADS)
nmc_k_psis_expect(const double* __restrict__ ll, const double* __restrict__ yrep, int C, int cols,
                  int row_begin, int n_valid, int col0, const uint64_t* __restrict__ keys,
                  int64_t S, int M, const unsigned long long* __restrict__ nonfinite,
                  const int* __restrict__ ntail, const double* __restrict__ lw, double* tie,
                  const double* __restrict__ y, int nresp, int j, double* __restrict__ ess,
                  double* __restrict__ wlt, double* __restrict__ weq, double* __restrict__ mean,
                  double* __restrict__ var, int64_t* __restrict__ baddraws) {
  extern __shared__ __attribute__((aligned(16))) double hs[];   // [nfit] head, [nfit] exp(lw - D)
  __shared__ double red[4 * 6];
  constexpr int NT = NMC_PSIS_THREADS;
  const int tid = threadIdx.x;
  const size_t col = blockIdx.x;
  const uint64_t* s = keys + col * (size_t)S;
  const size_t rstride = (size_t)cols * C;
  const size_t at0 = (size_t)row_begin * rstride + (size_t)(col0 + (int)col) * C;
  const double* lc = ll + at0;
  const double* yc = yrep + at0;
  const size_t o = col * (size_t)nresp + j;
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  if (nonfinite[col] != 0) {   // (the whole workgroup) the replicates are still counted
    double nb[1] = {0.0};
    nmc_psis_walk at(tid, n_valid);
    for (int64_t i = tid; i < S; i += NT, at.next())
      nb[0] += isfinite(yc[(size_t)at.q * rstride + at.c]) ? 0.0 : 1.0;
    nmc_psis_reduce(nb, red, tid, nmc_psis_add());
    if (tid == 0) {
      ess[col] = nan;
      wlt[o] = nan;
      weq[o] = nan;
      mean[o] = nan;
      var[o] = nan;
      baddraws[o] = (int64_t)nb[0];
    }
    return;
  }
  const int n2 = ntail[col];
  const int nfit = n2 > 4 ? n2 : 0;
  double* es = hs + nfit;
  double* tmp = tie + col * (size_t)(3 * M);   // [M] a group's replicates as they came
  double* ys = tmp + M;                        // [M] in the order of their keys
  int* cnt = (int*)(ys + M);                   // [lo]: the places of group [lo, hi) handed out
  const double llmin = nmc_sort_value(s[0]);
  const double rM = llmin - nmc_sort_value(s[M]);
  const double cut = rM > NMC_PSIS_LOG_TINY ? rM : NMC_PSIS_LOG_TINY;
  // D: nmc_k_psis' mx[0] (a maximum: exact in any order)
  double mx[1] = {llmin - nmc_sort_value(s[nfit])};
  for (int p = tid; p < nfit; p += NT) {
    hs[p] = nmc_sort_value(s[p]);
    cnt[p] = 0;
    const double v = lw[col * (size_t)M + p];
    mx[0] = v > mx[0] ? v : mx[0];
  }
  nmc_psis_reduce(mx, red, tid, nmc_psis_max());
  const double D = mx[0];
  for (int p = tid; p < nfit; p += NT) es[p] = exp(lw[col * (size_t)M + p] - D);
  __syncthreads();
  const double yo = y[col];
  double sm[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  // (NMC_PSIS_U samples' loads are issued before the first is consumed: the walk is bound by
  // the loads' latency, not by their bytes; the sums keep the samples' order)
  constexpr int U = NMC_PSIS_U;
  nmc_psis_walk wk(tid, n_valid);
  for (int64_t i = tid; i < S; i += (int64_t)NT * U) {
    double lv[U], yv[U];
#pragma unroll
    for (int u = 0; u < U; ++u, wk.next()) {
      // (past the end: sample 0 again, row 0 and chain 0 of the window, and dropped)
      const size_t at = i + (int64_t)u * NT < S ? (size_t)wk.q * rstride + wk.c : 0;
      lv[u] = lc[at];
      yv[u] = yc[at];
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (i + (int64_t)u * NT >= S) break;
      int lo, hi;
      const double W = nmc_psis_weight(lv[u], llmin, cut, D, nfit, hs, es, lo, hi);
      const double yr = yv[u];
      sm[0] += W;
      sm[1] += W * W;
      sm[5] += isfinite(yr) ? 0.0 : 1.0;
      if (hi - lo > 1) {   // a tie inside the tail: the replicate joins its group
        const int at2 = lo + atomicAdd(&cnt[lo], 1);
        if (at2 < hi) tmp[at2] = yr;   // (the group has hi - lo samples: always)
      } else {
        sm[2] += yr < yo ? W : 0.0;
        sm[3] += yr == yo ? W : 0.0;
        sm[4] += W * yr;
      }
    }
  }
  __syncthreads();   // (the groups are complete: global writes of this workgroup)
  for (int p = tid; p < nfit; p += NT) {
    if (!nmc_psis_tied(hs, nfit, p)) continue;
    int lo, hi;
    nmc_psis_weight(hs[p], llmin, cut, D, nfit, hs, es, lo, hi);
    const double v = tmp[p];
    const uint64_t kv = nmc_sort_key((uint64_t)__double_as_longlong(v));
    int rank = 0;
    for (int q = lo; q < hi; ++q) {
      const uint64_t kq = nmc_sort_key((uint64_t)__double_as_longlong(tmp[q]));
      rank += (kq < kv || (kq == kv && q < p)) ? 1 : 0;
    }
    ys[lo + rank] = v;
  }
  __syncthreads();
  for (int p = tid; p < nfit; p += NT) {
    if (!nmc_psis_tied(hs, nfit, p)) continue;
    int lo, hi;
    const double W = nmc_psis_weight(hs[p], llmin, cut, D, nfit, hs, es, lo, hi);
    const double yr = ys[p];
    sm[2] += yr < yo ? W : 0.0;
    sm[3] += yr == yo ? W : 0.0;
    sm[4] += W * yr;
  }
  nmc_psis_reduce(sm, red, tid, nmc_psis_add());
  const double Z = sm[0], mu = sm[4] / Z;
  double m2[1] = {0.0};
  wk = nmc_psis_walk(tid, n_valid);
  for (int64_t i = tid; i < S; i += (int64_t)NT * U) {
    double lv[U], yv[U];
#pragma unroll
    for (int u = 0; u < U; ++u, wk.next()) {
      const size_t at = i + (int64_t)u * NT < S ? (size_t)wk.q * rstride + wk.c : 0;
      lv[u] = lc[at];
      yv[u] = yc[at];
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (i + (int64_t)u * NT >= S) break;
      int lo, hi;
      const double W = nmc_psis_weight(lv[u], llmin, cut, D, nfit, hs, es, lo, hi);
      const double d = yv[u] - mu;
      if (hi - lo <= 1) m2[0] += W * (d * d);
    }
  }
  for (int p = tid; p < nfit; p += NT) {
    if (!nmc_psis_tied(hs, nfit, p)) continue;
    int lo, hi;
    const double W = nmc_psis_weight(hs[p], llmin, cut, D, nfit, hs, es, lo, hi);
    const double d = ys[p] - mu;
    m2[0] += W * (d * d);
  }
  nmc_psis_reduce(m2, red, tid, nmc_psis_add());
  if (tid == 0) {
    const bool bad = sm[5] != 0.0;
    ess[col] = Z * Z / sm[1];
    wlt[o] = bad ? nan : sm[2] / Z;
    weq[o] = bad ? nan : sm[3] / Z;
    mean[o] = bad ? nan : mu;
    var[o] = bad ? nan : m2[0] / Z;
    baddraws[o] = (int64_t)sm[5];
  }
}
