// rankz.h -- rank-normalised convergence diagnostics: the pass that turns every value of a
// column into its average rank's normal score, its folded counterpart and the two tail
// indicators (nmc_k_rank_transform; nmc_rank_partials in nestmc.hip; the definitions are
// nestmc/rankdiag.py's docstring).  Included by nestmc.hip only.
//
// A column's N = 2n * n_valid values have been sorted into keys s[0, N) (sortcol.h).  For a
// value x with key k, ties being numeric (the keys of -0.0 and +0.0 are neighbours and count
// as one value):
//   lo = #{s < x}, hi = #{s <= x}, twice the average rank 2 r = lo + hi + 1
//   z  = nmc_ndtri((r - 0.375) / (N + 0.25))
// Pass 1 reads x from the store as it lies and writes, into D[2n][4 kb][C] (store layout, kb
// the columns of the batch; the four quantities are the column ranges [0, kb), [kb, 2 kb), ...):
//   z | zeta = |x - med| | I05 = (lo <= k05) | I95 = (lo <= k95)
// with med = (s[N/2 - 1] + s[N/2]) / 2.0.  The zeta range is then sorted like any store
// column, and pass 2 replaces every zeta by the normal score of its rank among the zeta, each
// element read and written by the same thread.  The stream orders the passes: no workgroup
// waits on another.
//
// The search.  A workgroup stages every S-th key of its column, S = ceil(N / 4096), as at most
// 4096 splitters in 32 KiB of LDS.  The lower-bound search #{s < key} takes 13 LDS probes (the
// first ones read the same address in every lane: broadcasts) and then bisects the one segment
// of S - 1 keys in global memory that the splitters leave (none for N <= 4096, at most 4 probes
// for N = 51 200; a batch's sorted columns are larger than an XCD's L2, so these dependent
// probes' latency is what the pass costs -- DESIGN 3.13).  hi is lo + 1 unless the key after
// s[lo] ties, which one probe tells; only a tied value searches a second time.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sortcol.h"

enum { NMC_RANK_THREADS = 256, NMC_RANK_TILE = 16384, NMC_RANK_SPLIT = 4096 };
static_assert(NMC_RANK_TILE % NMC_RANK_THREADS == 0, "a thread owns TILE / THREADS elements");

// The keys of the two zeros: neighbours, -0.0 below +0.0.
#define NMC_KEY_NZERO 0x7fffffffffffffffull
#define NMC_KEY_PZERO 0x8000000000000000ull

// The inverse of the standard normal distribution function to full fp64 precision: Wichura's
// algorithm AS 241, routine PPND16 (Appl. Statist. 37 (1988) 477-484), three rational
// approximations of degree 7 in r = 0.180625 - q^2 (|q| = |p - 1/2| <= 0.425) and in
// sqrt(-log(min(p, 1 - p))) - 1.6 or - 5 (the tails, split at sqrt(-log) = 5).  Every
// operation is rounded on its own (the build has no contraction), Horner from the highest
// coefficient: tests/rankdiag_ref.py restates it in numpy.  p = 1/2 gives +0.0 exactly;
// p <= 0 gives -inf, p >= 1 +inf, NaN NaN.
__host__ __device__ inline double nmc_ndtri(double p) {
  if (p != p) return p;
  if (p <= 0.0) return -__builtin_inf();
  if (p >= 1.0) return __builtin_inf();
  const double q = p - 0.5;
  if (fabs(q) <= 0.425) {
    const double r = 0.180625 - q * q;
    const double num = (((((((2509.0809287301226727 * r + 33430.575583588128105) * r +
                             67265.770927008700853) * r + 45921.953931549871457) * r +
                           13731.693765509461125) * r + 1971.5909503065514427) * r +
                         133.14166789178437745) * r + 3.387132872796366608);
    const double den = (((((((5226.495278852545925 * r + 28729.085735721942674) * r +
                             39307.89580009271061) * r + 21213.794301586595867) * r +
                           5394.1960214247511077) * r + 687.1870074920579083) * r +
                         42.313330701600911252) * r + 1.0);
    return q * num / den;
  }
  double r = sqrt(-log(q < 0.0 ? p : 1.0 - p));
  double v;
  if (r <= 5.0) {
    r = r - 1.6;
    const double num = (((((((7.7454501427834140764e-4 * r + 0.0227238449892691845833) * r +
                             0.24178072517745061177) * r + 1.27045825245236838258) * r +
                           3.64784832476320460504) * r + 5.7694972214606914055) * r +
                         4.6303378461565452959) * r + 1.42343711074968357734);
    const double den = (((((((1.05075007164441684324e-9 * r + 5.475938084995344946e-4) * r +
                             0.0151986665636164571966) * r + 0.14810397642748007459) * r +
                           0.68976733498510000455) * r + 1.6763848301838038494) * r +
                         2.05319162663775882187) * r + 1.0);
    v = num / den;
  } else {
    r = r - 5.0;
    const double num = (((((((2.01033439929228813265e-7 * r + 2.71155556874348757815e-5) * r +
                             0.0012426609473880784386) * r + 0.026532189526576123093) * r +
                           0.29656057182850489123) * r + 1.7848265399172913358) * r +
                         5.4637849111641143699) * r + 6.6579046435011037772);
    const double den = (((((((2.04426310338993978564e-15 * r + 1.4215117583164458887e-7) * r +
                             1.8463183175100546818e-5) * r + 7.868691311456132591e-4) * r +
                           0.0148753612908506148525) * r + 0.13692988092273580531) * r +
                         0.59983224388101963777) * r + 1.0);
    v = num / den;
  }
  return q < 0.0 ? -v : v;
}

// #{s < key} over a column's N sorted keys s, spl[j] = s[j S] for j < ns = ceil(N / S).
__device__ __forceinline__ int64_t nmc_rank_below(const uint64_t* __restrict__ s, int64_t N,
                                                  int64_t S, int ns, const uint64_t* spl,
                                                  uint64_t key) {
  int j = 0;   // the splitters below key: the largest j with j <= ns and spl[j - 1] < key
#pragma unroll
  for (int step = NMC_RANK_SPLIT; step > 0; step >>= 1) {
    const int t = j + step;
    if (t <= ns && spl[t - 1] < key) j = t;
  }
  // s[(j - 1) S] < key <= s[j S] (where they exist): the bound lies in ((j - 1) S, j S]
  int64_t lo = j == 0 ? 0 : (int64_t)(j - 1) * S + 1;
  int64_t hi = j < ns ? (int64_t)j * S : N;
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);   // lo <= mid < hi <= N
    if (s[mid] < key) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// Grid (ceil(N / NMC_RANK_TILE), columns of the batch), 256 threads.  Workgroup (w, j):
// elements i in [w TILE, min(N, (w + 1) TILE)) of batch column j, i = q n_valid + c (row q
// of the window, chain c), consecutive lanes on consecutive i.
//   PASS 1: x = src[row_begin + q][src_col0 + j][c] (the store, src_cols columns); keys: the
//           sorted x; writes z, zeta, I05, I95 to D[q][t k + j][c], t = 0..3.
//   PASS 2: src = D, src_cols = 4 k, src_col0 = k, row_begin = 0: zeta = D[q][k + j][c];
//           keys: the sorted zeta; overwrites it with zf.
// nonfinite[bad0 + j] != 0 (the column's x hold a NaN or an infinity): NaN everywhere and no
// search.  twice_rank (or NULL): [rows_tr][tr_cols][C] of lo + hi + 1, column tr_col0 + j,
// 0 for such a column.  Chains >= n_valid have no element: nothing of theirs is read or written.
template <int PASS>
__global__ void __launch_bounds__(NMC_RANK_THREADS)
nmc_k_rank_transform(const double* src, int C, int src_cols, int row_begin,
                     int src_col0, int n_valid, int64_t N, const uint64_t* __restrict__ keys,
                     double* D, int k, const unsigned long long* __restrict__ nonfinite,
                     int bad0, long long* __restrict__ twice_rank, int tr_cols, int tr_col0) {
  __shared__ uint64_t spl[NMC_RANK_SPLIT];
  const int tid = threadIdx.x;
  const int j = blockIdx.y;
  const uint64_t* s = keys + (size_t)j * (size_t)N;
  const bool bad = nonfinite[bad0 + j] != 0;
  const int64_t S = (N + NMC_RANK_SPLIT - 1) / NMC_RANK_SPLIT;
  const int ns = (int)((N + S - 1) / S);   // <= 4096; (ns - 1) S < N
  if (!bad)
    for (int e = tid; e < ns; e += NMC_RANK_THREADS) spl[e] = s[(int64_t)e * S];
  __syncthreads();
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  const double med = bad || PASS != 1 ? 0.0
                                      : (nmc_sort_value(s[N / 2 - 1]) + nmc_sort_value(s[N / 2])) / 2.0;
  const int64_t k05 = (N - 1) / 20, k95 = 19 * (N - 1) / 20;
  const double den = (double)N + 0.25;
  const size_t sstride = (size_t)src_cols * C, dstride = (size_t)4 * k * C;
  const double* xs = src + (size_t)row_begin * sstride + (size_t)(src_col0 + j) * C;
  const int64_t base = (int64_t)blockIdx.x * NMC_RANK_TILE;
#pragma unroll 1
  for (int it = 0; it < NMC_RANK_TILE / NMC_RANK_THREADS; ++it) {
    const int64_t i = base + it * NMC_RANK_THREADS + tid;
    if (i >= N) break;   // (i ascends with it)
    const unsigned q = (unsigned)i / (unsigned)n_valid;   // (N < 2^31)
    const unsigned c = (unsigned)i - q * (unsigned)n_valid;
    double* d = D + (size_t)q * dstride + (size_t)j * C + c;
    const size_t qstep = (size_t)k * C;   // from one quantity to the next
    long long* tr = twice_rank ? twice_rank + ((size_t)q * tr_cols + (tr_col0 + j)) * C + c : nullptr;
    if (bad) {
      if (PASS == 1) {
        d[0] = nan;
        d[qstep] = nan;
        d[2 * qstep] = nan;
        d[3 * qstep] = nan;
      } else {
        d[qstep] = nan;
      }
      if (tr) *tr = 0;
      continue;
    }
    const double x = xs[(size_t)q * sstride + c];
    const uint64_t key = nmc_sort_key((uint64_t)__double_as_longlong(x));
    const uint64_t klo = key == NMC_KEY_PZERO ? NMC_KEY_NZERO : key;
    const uint64_t khi = key == NMC_KEY_NZERO ? NMC_KEY_PZERO : key;
    const int64_t lo = nmc_rank_below(s, N, S, ns, spl, klo);
    // s[lo] is x or its tie (x is in the column): lo < N
    int64_t hi = lo + 1;
    if (hi < N && s[hi] <= khi) hi = nmc_rank_below(s, N, S, ns, spl, khi + 1);   // (khi is finite)
    const int64_t r2 = lo + hi + 1;
    const double z = nmc_ndtri(((double)r2 * 0.5 - 0.375) / den);
    if (tr) *tr = r2;
    if (PASS == 1) {
      d[0] = z;
      d[qstep] = fabs(x - med);
      d[2 * qstep] = lo <= k05 ? 1.0 : 0.0;
      d[3 * qstep] = lo <= k95 ? 1.0 : 0.0;
    } else {
      d[qstep] = z;
    }
  }
}
