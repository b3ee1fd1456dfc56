// sortcol.h -- a segmented sort of the sample store's columns and the order statistics read
// off it (nmc_k_sort_tiles, nmc_k_sort_merge, nmc_k_sort_scan; nmc_summary in nestmc.hip).
//
// The median and the highest-density interval of a column (Diagnostic._computeMedianAndHdi,
// sampleDiagnosis.py:419-427; computeHpdInterval :766-776) are order statistics of its
// N = n_rows * n_valid values.  A column k of the store samples[row][col][C] over the rows
// [row_begin, row_begin + n_rows) and the real chains [0, n_valid) has the flat index
// i = q * n_valid + c (row q of the window, chain c); it is read as it lies, every (row, chain
// run) coalesced, and no transposed copy is made.
//
// Key: a double's bits b as a uint64 that orders like the number,
//   sign set: ~b        sign clear: b | 1 << 63
// so -NaN < -inf < ... < -0.0 < +0.0 < ... < +inf < +NaN.  Order statistics depend on the
// multiset alone: the sorted column is the same bits whatever the tiling, sharding or batch.
//
//   nmc_k_sort_tiles   runs of T = NMC_SORT_TILE keys, each sorted in LDS (bitonic)
//   nmc_k_sort_merge   one pass: runs of length L merged in pairs by merge path
//   nmc_k_sort_scan    values at given ranks and the narrowest interval of `gap` steps
// None of them waits on another workgroup: the stream orders the passes.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

enum { NMC_SORT_TILE = 4096, NMC_SORT_THREADS = 256, NMC_SORT_PER = 16 };
static_assert(NMC_SORT_THREADS * NMC_SORT_PER == NMC_SORT_TILE, "a thread owns 16 keys of a tile");

// The pad of a short last tile: the largest key.  Only a +NaN of all-ones payload has it, and
// equal keys are the same bits, so a pad never displaces a real key from the first len places.
#define NMC_SORT_PAD 0xffffffffffffffffull

__host__ __device__ __forceinline__ uint64_t nmc_sort_key(uint64_t b) {
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__host__ __device__ __forceinline__ uint64_t nmc_sort_unkey(uint64_t k) {
  return (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
}
__device__ __forceinline__ double nmc_sort_value(uint64_t k) {
  return __longlong_as_double((long long)nmc_sort_unkey(k));
}

// A tile's place e in LDS: 16 keys at a pitch of 17 words.  A thread that holds 16 consecutive
// keys (window 0 below) is then 34 dwords from its neighbour: the 32 lanes of a ds_read_b64
// group fall on 32 different bank pairs, where a pitch of 16 would put them all on two.
__device__ __forceinline__ int nmc_sort_at(int e) { return e + (e >> 4); }

// The compare-exchanges of the bitonic stage k = 1 << p whose partners differ in a bit of
// [B, B + 4), in registers: the thread holds the 16 keys whose places differ in those four
// bits only (B = 0: 16 consecutive keys; B = 4, 8: a stride of 16 or 256), does the stage's
// steps j = 1 << (B + 3) ... 1 << B that exist (j < k) and puts the keys back.  Every thread
// reads and writes its own 16 places: the steps of a window need no barrier among themselves.
template <int B>
__device__ __forceinline__ void nmc_sort_window(uint64_t* s, int tid, int k, int p) {
  const int base = ((tid >> B) << (B + 4)) | (tid & ((1 << B) - 1));
  uint64_t v[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) v[r] = s[nmc_sort_at(base | (r << B))];
#pragma unroll
  for (int m = 3; m >= 0; --m) {
    if (B + m < p) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        if (r & (1 << m)) continue;
        const int r2 = r | (1 << m);
        const bool up = ((base | (r << B)) & k) == 0;   // (k = T: every pair ascends)
        const uint64_t a = v[r], b = v[r2];
        const bool sw = (a > b) == up;
        v[r] = sw ? b : a;
        v[r2] = sw ? a : b;
      }
    }
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) s[nmc_sort_at(base | (r << B))] = v[r];
}

// Grid (tiles, columns of the batch), 256 threads.  Tile t of column col0 + blockIdx.y: the
// flat indices [t T, min(N, (t + 1) T)), loaded with consecutive lanes on consecutive i,
// sorted in LDS (34 KiB with the pitch) and written to out[column of the batch][N] at the same
// places.  Values that are not finite are counted per column (one vector atomicAdd per thread
// that saw any).  The bitonic network's 78 steps run as 24 register windows (nmc_sort_window:
// up to four steps between two barriers), the windows of a stage from the top bits down.
__global__ void __launch_bounds__(NMC_SORT_THREADS)
nmc_k_sort_tiles(const double* __restrict__ samples, int C, int cols, int row_begin, int n_valid,
                 int64_t N, int col0, uint64_t* __restrict__ out,
                 unsigned long long* __restrict__ nonfinite) {
  constexpr int T = NMC_SORT_TILE;
  static_assert(T == 1 << 12, "three windows of four bits");
  __shared__ uint64_t s[T + T / 16];
  const int tid = threadIdx.x;
  const int col = col0 + (int)blockIdx.y;
  const int64_t base = (int64_t)blockIdx.x * T;
  const size_t rstride = (size_t)cols * C;
  const double* x = samples + (size_t)row_begin * rstride + (size_t)col * C;
  unsigned bad = 0;
#pragma unroll
  for (int j = 0; j < NMC_SORT_PER; ++j) {
    const int e = j * NMC_SORT_THREADS + tid;
    const int64_t i = base + e;
    uint64_t key = NMC_SORT_PAD;
    if (i < N) {
      const unsigned q = (unsigned)i / (unsigned)n_valid;   // (N < 2^31)
      const unsigned c = (unsigned)i - q * (unsigned)n_valid;
      const uint64_t b = (uint64_t)__double_as_longlong(x[(size_t)q * rstride + c]);
      bad += (b & 0x7ff0000000000000ull) == 0x7ff0000000000000ull;
      key = nmc_sort_key(b);
    }
    s[nmc_sort_at(e)] = key;
  }
  if (bad) atomicAdd(&nonfinite[col], (unsigned long long)bad);
  __syncthreads();
#pragma unroll 1
  for (int p = 1; p <= 12; ++p) {
    const int k = 1 << p;
    if (p > 8) {
      nmc_sort_window<8>(s, tid, k, p);
      __syncthreads();
    }
    if (p > 4) {
      nmc_sort_window<4>(s, tid, k, p);
      __syncthreads();
    }
    nmc_sort_window<0>(s, tid, k, p);
    __syncthreads();
  }
  uint64_t* o = out + (size_t)blockIdx.y * (size_t)N;
#pragma unroll
  for (int j = 0; j < NMC_SORT_PER; ++j) {
    const int e = j * NMC_SORT_THREADS + tid;
    if (base + e < N) o[base + e] = s[nmc_sort_at(e)];
  }
}

// The merge-path split of diagonal d over two sorted runs a[0, la) and b[0, lb), ties taking
// the left run first: the number of a's elements among the first d outputs.  0 <= d <= la + lb.
template <class P>
__device__ __forceinline__ int64_t nmc_sort_split(P a, int64_t la, P b, int64_t lb, int64_t d) {
  int64_t lo = d > lb ? d - lb : 0, hi = d < la ? d : la;
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);   // lo <= mid < hi <= la; 0 <= d - 1 - mid < lb
    if (a[mid] <= b[d - 1 - mid]) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// One merge pass.  Grid (tiles, columns of the batch), 256 threads.  The column's N sorted
// keys lie in runs of L (a multiple of T; the last run may be shorter); runs 2 r and 2 r + 1
// are merged.  Workgroup w owns the outputs [w T, min(N, (w + 1) T)), all inside one pair: it
// finds the splits of its two diagonals by binary search on the runs in global memory (two
// lanes, one diagonal each), stages exactly the inputs in between in LDS -- at most T -- and
// every thread merges its 16 outputs serially from its own split in LDS.  The outputs go
// back through the same LDS for a coalesced store, a thread's 16 at a pitch of 17 words: 16
// lanes of a ds_write_b64 group then fall on 16 different bank pairs instead of one.  A pair
// whose right run is empty (a run without a partner) is a merge with nothing: a copy.
__global__ void __launch_bounds__(NMC_SORT_THREADS)
nmc_k_sort_merge(const uint64_t* __restrict__ in, uint64_t* __restrict__ out, int64_t N, int64_t L) {
  constexpr int T = NMC_SORT_TILE;
  __shared__ uint64_t s[T + T / NMC_SORT_PER];
  __shared__ int64_t cut[2];
  const int tid = threadIdx.x;
  const uint64_t* src = in + (size_t)blockIdx.y * (size_t)N;
  uint64_t* dst = out + (size_t)blockIdx.y * (size_t)N;
  const int64_t o0 = (int64_t)blockIdx.x * T;
  const int64_t pbase = o0 / (2 * L) * (2 * L);
  const int64_t la = N - pbase < L ? N - pbase : L;
  const int64_t lb = N - pbase - la < L ? N - pbase - la : L;
  const uint64_t* a = src + pbase;
  const uint64_t* b = a + la;
  const int64_t d0 = o0 - pbase;
  const int64_t d1 = d0 + T < la + lb ? d0 + T : la + lb;
  if (tid == 0) cut[0] = nmc_sort_split(a, la, b, lb, d0);
  if (tid == 64) cut[1] = nmc_sort_split(a, la, b, lb, d1);
  __syncthreads();
  const int64_t a0 = cut[0], a1 = cut[1];
  const int64_t b0 = d0 - a0;
  const int n = (int)(d1 - d0);          // 1 <= n <= T outputs
  const int na = (int)(a1 - a0);         // 0 <= na <= n of them from the left run
  const int nb = n - na;
#pragma unroll
  for (int j = 0; j < NMC_SORT_PER; ++j) {
    const int e = j * NMC_SORT_THREADS + tid;
    if (e < n) s[e] = e < na ? a[a0 + e] : b[b0 + (e - na)];
  }
  __syncthreads();
  const int t0 = tid * NMC_SORT_PER < n ? tid * NMC_SORT_PER : n;
  int ia = (int)nmc_sort_split(s, (int64_t)na, s + na, (int64_t)nb, (int64_t)t0);
  int ib = t0 - ia;
  uint64_t r[NMC_SORT_PER];
  uint64_t ka = ia < na ? s[ia] : NMC_SORT_PAD;
  uint64_t kb = ib < nb ? s[na + ib] : NMC_SORT_PAD;
#pragma unroll
  for (int j = 0; j < NMC_SORT_PER; ++j) {
    const bool left = ia < na && (ib >= nb || ka <= kb);
    r[j] = left ? ka : kb;
    if (left) {
      ++ia;
      ka = ia < na ? s[ia] : NMC_SORT_PAD;
    } else {
      ++ib;
      kb = ib < nb ? s[na + ib] : NMC_SORT_PAD;
    }
  }
  __syncthreads();   // every thread has read its inputs
#pragma unroll
  for (int j = 0; j < NMC_SORT_PER; ++j) s[tid * (NMC_SORT_PER + 1) + j] = r[j];
  __syncthreads();
#pragma unroll
  for (int j = 0; j < NMC_SORT_PER; ++j) {
    const int e = j * NMC_SORT_THREADS + tid;
    if (e < n) dst[o0 + e] = s[e + e / NMC_SORT_PER];
  }
}

// Grid (columns of the batch), 256 threads: one workgroup per column over its N sorted keys.
//   at[col][r]  = the value at ranks[r]
//   hdi[col]    = (s[i], s[i + gap]) for the first i in [0, N - gap) that minimises
//                 s[i + gap] - s[i] (one fp64 subtraction each), hdi_at[col] = i
// by a lexicographic minimum of (width, i): per thread over i = tid, tid + 256, ... (ascending,
// so a strict < keeps the first), then over the workgroup through LDS.  A column with values
// that are not finite gets NaN everywhere and hdi_at = -1.
__global__ void __launch_bounds__(NMC_SORT_THREADS)
nmc_k_sort_scan(const uint64_t* __restrict__ keys, int64_t N, int64_t gap,
                const int64_t* __restrict__ ranks, int n_ranks, int col0,
                const unsigned long long* __restrict__ nonfinite, double* __restrict__ at,
                double* __restrict__ hdi, int64_t* __restrict__ hdi_at) {
  __shared__ double sw[NMC_SORT_THREADS];
  __shared__ int64_t si[NMC_SORT_THREADS];
  const int tid = threadIdx.x;
  const int col = col0 + (int)blockIdx.x;
  const uint64_t* s = keys + (size_t)blockIdx.x * (size_t)N;
  if (nonfinite[col] != 0) {
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    for (int r = tid; r < n_ranks; r += NMC_SORT_THREADS) at[(size_t)col * n_ranks + r] = nan;
    if (tid == 0) {
      hdi[2 * (size_t)col] = nan;
      hdi[2 * (size_t)col + 1] = nan;
      hdi_at[col] = -1;
    }
    return;
  }
  for (int r = tid; r < n_ranks; r += NMC_SORT_THREADS)
    at[(size_t)col * n_ranks + r] = nmc_sort_value(s[ranks[r]]);
  double bw = __longlong_as_double(0x7ff0000000000000ll);   // +inf
  int64_t bi = INT64_MAX;
  const int64_t m = N - gap;   // >= 1 candidates
#pragma unroll 4
  for (int64_t i = tid; i < m; i += NMC_SORT_THREADS) {
    const double w = nmc_sort_value(s[i + gap]) - nmc_sort_value(s[i]);
    if (w < bw || bi == INT64_MAX) {
      bw = w;
      bi = i;
    }
  }
  sw[tid] = bw;
  si[tid] = bi;
  __syncthreads();
  for (int h = NMC_SORT_THREADS / 2; h > 0; h >>= 1) {
    if (tid < h) {
      const double w2 = sw[tid + h];
      const int64_t i2 = si[tid + h];
      if (w2 < sw[tid] || (w2 == sw[tid] && i2 < si[tid])) {
        sw[tid] = w2;
        si[tid] = i2;
      }
    }
    __syncthreads();
  }
  if (tid == 0) {
    const int64_t i = si[0];
    hdi[2 * (size_t)col] = nmc_sort_value(s[i]);
    hdi[2 * (size_t)col + 1] = nmc_sort_value(s[i + gap]);
    hdi_at[col] = i;
  }
}
