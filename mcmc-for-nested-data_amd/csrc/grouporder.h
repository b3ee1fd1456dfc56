// grouporder.h -- rank histogram and pairwise win counts of a parameter's group values over
// the device sample store (nmc_k_group_order).
//
// Per sample s = (recorded row, chain) and parameter p the G group values theta_g (store
// column p (G + pc) + pc + g, pc = 2 hyper columns under partial pooling) are compared with
// each other; nestmc/groupcmp.py's docstring has the definitions:
//   rank_s(g) = #{h : theta_h < theta_g}     H[p][g][r] = #{s : rank_s(g) = r}
//   W[p][g][h] = #{s : theta_g > theta_h}    nonfinite[p] = #{(s, g) : theta_g NaN or +-inf}
// Every comparison is one fp64 "<" (NaN false both ways, -0.0 == +0.0) and every result an
// integer count: no floating-point accumulation, so nothing depends on the order of the adds.
// The league-table analysis of multilevel models (Goldstein and Spiegelhalter 1996) is what
// the counts serve; the reference has no counterpart (its Figure.bivariates only plots pairs).
#pragma once

#include <stdint.h>

// Groups a wave owns (their theta_g and ranks live in registers), waves of a workgroup at the
// most, the workgroup's LDS ceiling and the theta_h loads a wave keeps in flight (16 measured
// 10 % faster than 8 at 256 groups, where LDS leaves two waves per SIMD to hide them).  A
// wave keeps hist[8][G] and wins[8][G] (uint32) of its own groups in LDS, 64 G bytes: 4 waves
// up to G = 640, 2 up to 1280, 1 up to 2560; beyond that nothing is kept in LDS and the adds
// go straight to global memory (DIRECT).
enum { NMC_GO_T = 8, NMC_GO_WAVES = 4, NMC_GO_LDS_MAX = 160 * 1024, NMC_GO_U = 16 };

// Waves per workgroup for G groups; 0: the direct form (one wave, no LDS).
static inline int nmc_go_waves(int G) {
  const int64_t per_wave = (int64_t)2 * NMC_GO_T * G * 4;
  const int64_t w = NMC_GO_LDS_MAX / per_wave;
  return (int)(w > NMC_GO_WAVES ? NMC_GO_WAVES : w);
}

// Grid (P * ntile, ceil(n_valid / 64), nslice), nw * 64 threads (nw = 1 in the direct form),
// dynamic LDS nw * 64 G bytes (none in the direct form).  Wave w of workgroup (p, tile; cb; z)
// owns groups [g0, g0 + 8), g0 = (tile nw + w) 8, of parameter p for the 64 chains of chain
// block cb, lane = chain, over rows [row0 + z rps, row0 + min(nrows, (z + 1) rps)).  Per row
// the lane holds its chain's 8 theta_g; it walks all h in chunks of 64, 16 loads in flight,
// each load a 512-byte run of the store as it lies.  Per pair one compare gives a 64-bit
// lane mask: the lane adds its own bit to rank[i], and the mask's popcount (wave-uniform) is
// kept by lane h & 63 in cnt[i]; after a chunk, cnt[i] is added to the wave's
// wins[i][chunk 64 + lane] in LDS -- the row of LDS is the wave's own: no atomics, no barrier.
// After the last h every lane adds 1 to hist[i][rank[i]] (an LDS atomic: lanes share bins).
// Chains >= n_valid read chain n_valid - 1 (inside the store) and compare as NaN, so they
// count nothing.  At the end of the row slice the wave adds its non-zero LDS counts to H and W
// with global atomics on uint32 (integer addition commutes: any schedule gives the same
// words).  No spin, no waiting on another workgroup.
template <bool DIRECT>
__global__ void __launch_bounds__(NMC_GO_WAVES * 64)
nmc_k_group_order(const double* __restrict__ samples, int C, int cols, int P, int G, int pc,
                  int ntile, int row0, int nrows, int rps, int n_valid,
                  uint32_t* __restrict__ H, uint32_t* __restrict__ W,
                  unsigned long long* __restrict__ nonfinite) {
  constexpr int T = NMC_GO_T, U = NMC_GO_U;
  extern __shared__ uint32_t go_lds[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int nw = (int)blockDim.x >> 6;
  const int p = (int)blockIdx.x / ntile, tile = (int)blockIdx.x % ntile;
  const int g0 = (tile * nw + wave) * T;
  if (g0 >= G) return;   // (no barrier below: a wave may leave alone)
  const int ng = G - g0 < T ? G - g0 : T;
  const int c = (int)blockIdx.y * 64 + lane;
  const bool valid = c < n_valid;
  const int cc = valid ? c : n_valid - 1;
  const int r0 = row0 + (int)blockIdx.z * rps;
  const int r1 = row0 + (nrows < ((int)blockIdx.z + 1) * rps ? nrows : ((int)blockIdx.z + 1) * rps);
  const int nch = (G + 63) / 64;
  const double qnan = __builtin_nan("");

  uint32_t* hist = go_lds + (size_t)wave * 2 * T * G;   // [T][G], then wins [T][G]
  uint32_t* wins = hist + (size_t)T * G;
  if (!DIRECT)
    for (int k = lane; k < 2 * T * G; k += 64) hist[k] = 0;
  uint32_t* Hg = H + ((size_t)p * G + g0) * G;           // row i: + i G
  uint32_t* Wg = W + ((size_t)p * G + g0) * G;

  const size_t rstride = (size_t)cols * C;
  const double* base = samples + ((size_t)p * (G + pc) + pc) * C + cc;   // theta_0 of p
  unsigned bad = 0;
  for (int r = r0; r < r1; ++r) {
    const double* row = base + (size_t)r * rstride;
    double tg[T];
    uint32_t rank[T];
#pragma unroll
    for (int i = 0; i < T; ++i) {
      const double v = row[(size_t)(g0 + (i < ng ? i : ng - 1)) * C];
      if (i < ng && !(__builtin_fabs(v) < __builtin_huge_val())) ++bad;
      tg[i] = valid ? v : qnan;
      rank[i] = 0;
    }
    for (int ch = 0; ch < nch; ++ch) {
      const int h0 = ch * 64;
      const int hn = G - h0 < 64 ? G - h0 : 64;
      uint32_t cnt[T];
#pragma unroll
      for (int i = 0; i < T; ++i) cnt[i] = 0;
      for (int j0 = 0; j0 < hn; j0 += U) {
        double th[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int j = j0 + u;
          const double v = row[(size_t)(h0 + (j < hn ? j : hn - 1)) * C];
          th[u] = j < hn ? v : qnan;   // (past the last group: compares false)
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
#pragma unroll
          for (int i = 0; i < T; ++i) {
            const bool lt = th[u] < tg[i];
            rank[i] += lt ? 1u : 0u;
            const uint32_t n = (uint32_t)__popcll(__ballot(lt));
            cnt[i] = lane == j0 + u ? n : cnt[i];
          }
        }
      }
      if (h0 + lane < G) {
#pragma unroll
        for (int i = 0; i < T; ++i)
          if (i < ng && cnt[i]) {
            if (DIRECT) atomicAdd(Wg + (size_t)i * G + h0 + lane, cnt[i]);
            else wins[i * G + h0 + lane] += cnt[i];
          }
      }
    }
    if (valid) {
#pragma unroll
      for (int i = 0; i < T; ++i)
        if (i < ng) {
          if (DIRECT) atomicAdd(Hg + (size_t)i * G + rank[i], 1u);
          else atomicAdd(hist + i * G + rank[i], 1u);
        }
    }
  }
  if (bad && valid) atomicAdd(nonfinite + p, (unsigned long long)bad);
  if (!DIRECT)
    for (int i = 0; i < ng; ++i)
      for (int k = lane; k < G; k += 64) {
        const uint32_t a = hist[i * G + k], b = wins[i * G + k];
        if (a) atomicAdd(Hg + (size_t)i * G + k, a);
        if (b) atomicAdd(Wg + (size_t)i * G + k, b);
      }
}
