// diag.hip -- the convergence diagnostic's variogram on the GPU.
//
// The reference's effective sample size (Diagnostic._computeVariogram,
// sampleDiagnosis.py:189-194, called for every lag t < n by _computeAutocorrelation
// :196-208) is
//   V_t = sum_j sum_{i=t}^{n-1} (x_j[i] - x_j[i-t])^2 / (m (n - t))
// over the m half-chains j of each column: O(m n^2) pure-Python work per column, the
// part that does not scale.  nmc_variogram takes any number of columns (cfg 4/5 have tens
// of thousands), in batches of at most 65535 columns and 256 MiB of input.  Here one
// thread owns one (column, lag) and adds in the reference's order: i ascending inside a
// half-chain, the half-chains' sums in j order, then one division.  A block stages one
// half-chain row of its column in LDS at a time; thread t reads row[s + t] (consecutive
// lanes) and row[s] (a broadcast) for s = i - t.  Squares are d * d, correctly rounded; the
// reference's numpy float64 ** 2 goes through libm pow, which rounds a few in 10^4
// squares the other way, so V_t agree to a few ulp (the printed %.3f values agree).
#include <hip/hip_runtime.h>

#include <stdlib.h>

#include <string>

#include "ctx.h"

// x: [K][m][n] columns' half-chains; out: [K][n].  grid = (ceil(n / 256), K), 256 threads;
// dynamic LDS = n doubles.
__global__ void __launch_bounds__(256) nmc_k_variogram(const double* __restrict__ x, int m, int n,
                                                       double* __restrict__ out) {
  extern __shared__ double row[];
  const int k = blockIdx.y;
  const int t = blockIdx.x * 256 + threadIdx.x;
  const double* xk = x + (size_t)k * m * n;
  double total = 0.0;
  for (int j = 0; j < m; ++j) {
    __syncthreads();   // the previous row is no longer read
    for (int i = threadIdx.x; i < n; i += 256) row[i] = xk[(size_t)j * n + i];
    __syncthreads();
    if (t < n) {
      double s = 0.0;
      for (int q = 0; q + t < n; ++q) {   // i = q + t, i - t = q
        const double d = row[q + t] - row[q];
        s = s + d * d;
      }
      total = j == 0 ? s : total + s;
    }
  }
  if (t < n) out[(size_t)k * n + t] = total / ((double)m * (double)(n - t));
}

// K is worked through in batches of columns: at most 65535 of them (gridDim.y) and at most a
// byte budget of input, 256 MiB as nmc_write_ll_csvs uses (NMC_VARIO_BATCH_BYTES, read at every
// call: a smaller budget, so the tests can reach the batched branch), never fewer than one
// column.  One allocation holds the largest batch's input and output.  A column's V_t are
// computed from that column alone, so the batches' results are those of one launch, bit for
// bit, whatever the store's width.
extern "C" int nmc_variogram(int device, const double* x, int K, int m, int n, double* out) {
  if (K < 0 || m < 1 || n < 1) return nmc_fail(-1, "variogram: need K >= 0, m >= 1, n >= 1");
  if ((size_t)n * 8 > (size_t)64 * 1024) return nmc_fail(-1, "variogram: n > 8192 half-chain rows");
  if (K == 0) return 0;
  size_t budget = (size_t)256 << 20;
  if (const char* e = getenv("NMC_VARIO_BATCH_BYTES"))
    if (atoll(e) > 0) budget = (size_t)atoll(e);
  const size_t per_in = (size_t)m * n, per_out = (size_t)n;   // doubles per column
  size_t kb = budget / (per_in * 8);
  if (kb > 65535) kb = 65535;
  if (kb > (size_t)K) kb = (size_t)K;
  if (kb < 1) kb = 1;
  HIPCHK(hipSetDevice(device));
  hipStream_t st;
  HIPCHK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
  double* dbuf = nullptr;   // [kb][m][n] input, then [kb][n] output
  hipError_t e = hipMalloc(&dbuf, kb * (per_in + per_out) * 8);
  double* dx = dbuf;
  double* dout = dbuf ? dbuf + kb * per_in : nullptr;
  for (size_t k0 = 0; k0 < (size_t)K && e == hipSuccess; k0 += kb) {
    const size_t nk = (size_t)K - k0 < kb ? (size_t)K - k0 : kb;
    e = hipMemcpyAsync(dx, x + k0 * per_in, nk * per_in * 8, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) {
      hipLaunchKernelGGL(nmc_k_variogram, dim3((n + 255) / 256, (unsigned)nk), dim3(256),
                         (size_t)n * 8, st, dx, m, n, dout);
      e = hipGetLastError();
    }
    if (e == hipSuccess)
      e = hipMemcpyAsync(out + k0 * per_out, dout, nk * per_out * 8, hipMemcpyDeviceToHost, st);
    // (the next batch overwrites dx and dout: the stream orders it behind this copy)
  }
  const hipError_t es = hipStreamSynchronize(st);
  if (e == hipSuccess) e = es;
  hipFree(dbuf);
  hipStreamDestroy(st);
  if (e != hipSuccess) return nmc_fail(-2, std::string("variogram: ") + hipGetErrorString(e));
  return 0;
}
