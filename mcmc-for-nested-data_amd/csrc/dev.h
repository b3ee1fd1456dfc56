// dev.h -- what the host and the kernels share: struct Dev (one launch's arguments), the
// NMC_* enums and build-time geometry constants, the LDS carve (nmc_lds), the row tiling
// (nmc_tiles), the row-split chunks (nmc_chunk) and the slot / sample-row index helpers.
#pragma once
#ifndef __HIPCC_RTC__   // (hiprtc, user families: the runtime provides these)
#include <hip/hip_runtime.h>
#include <stdint.h>
#endif

#include "../../include/nestmc.h"   // (fixed-width integer types, also under hiprtc)

struct Dev {
  int C, G, P, pooling, nf, chain_base, rng_mode, W, CB;
  // step kernel: chains per workgroup CL (64, one per lane; reported by
  // nmc_launch_config) and its chain blocks RB = ceil(C / CL).  (A 32-chain half-lane
  // layout -- two workgroups per CU -- measured 11.5 against 8.5 us per iteration at
  // cfg 3 and was removed.)
  int CL, RB;
  int paired;            // likelihood rows: two chains per lane (nmc_ll_rows_lds<Fam, true>)
  int quad;              // nmc_k_run, {x, y} rows in LDS: four chains per lane
                         // (nmc_ll_rows_lds_quad; NMC_ROWS=pair keeps the paired loop)
  // Row split (none/complete pooling with large groups): S workgroups ("members") share
  // one (chain block, group), member m owning the m-th contiguous chunk of the group's
  // rows (nmc_chunk); each step they exchange their partial sums through xbuf
  // ([2 step parity][RB][G][S][NACC][64], sc1 stores + the unit's counter xcnt[RB*G][32])
  // and all make the same decision.  S depends on the rows, the group count and the CU
  // count only, never on the chain count: results are shard- and batch-invariant.
  // cb0: first chain block of this launch (chain blocks are launched in resident batches).
  int S, cb0;
  // publish / exchange counters are never reset between launches: they already hold
  // G * pbase publishes per (chain block, parameter) and S * xbase arrivals per unit from
  // the context's earlier launches (the host advances both; no memset per launch)
  unsigned pbase, xbase;
  double* xbuf;
  unsigned* xcnt;
  uint32_t seed;
  const int64_t* off;    // [G+1] CSR offsets
  const double* obs;     // [n_obs][nf]
  const int* pfam;       // [P]
  const double* ppar;    // [P][8]
  double* vb0;           // values after iteration t live in vb[t & 1]: [P][G][C]
  double* vb1;
  double* lp;            // [P][G][C]
  double* ll;            // [G][C]
  double* scale;         // [P][G][C]
  int* nacc;             // [P][G][C]  since last tune
  int* nrej;
  long long* tacc;       // [P][G][C]  total accepted
  double* mu;            // [2][P][C]: after iteration t in slot t & 1 (nmc_hslot)
  double* s2;
  double* hsd;           // sqrt(s2)
  double* hlsd;          // log(sqrt(s2))
  double ha, hlga;       // invgamma shape a = (G-1)/2 and gammaln(a)
  // numpy pairwise-sum plan over the G groups (numpy/_core/src/umath/loops_utils.h)
  const int* leaf;       // [nleaf+1] start of each <=128-element leaf block
  const int* merge;      // [nmerge][2] post-order merges: slot a += slot b
  int nleaf, nmerge, ntail;
  int nmax;              // rows of the largest group
  int hlds, naux;        // persistent partial: Gibbs payload via LDS, auxiliary waves
  int hreg;              // persistent partial, G <= 64: Gibbs payload in registers (SYNC_REG)
  int xpc;               // nmc_k_run, persistent partial pooling, RB | 8: XCDs per chain block
                         // (workgroup placement, nmc_k_run; 0: chain-block-major)
  unsigned* hrd;         // [RB][P][32] hyper-ready counts of nmc_k_sweep's Gibbs workgroups
                         // (SYNC_OWN; pbase tasks per parameter before)
  int noprio;            // diagnostics: no issue priority for the latency-bound waves
  int pubearly;          // nmc_k_sweep: the control counts the previous step's publication
                         // before taking a tile (its store drained first), not after one
  int gwaves;            // waves of nmc_k_sweep_gibbs (4)
  int nstatic;           // nmc_k_run: waves 2.. start on static tile entries (W - 2; 0 off,
                         // NMC_STATIC_TILES=0)
  int gsep;              // nmc_k_sweep SYNC_OWN: the Gibbs workgroups run as their own kernel
                         // (nmc_k_sweep_gibbs) on a second stream
  // gsep progress without co-scheduling (sweep.h nmc_grole_*): per chain block a role word
  // [63:32] launch epoch, [31:1] Gibbs workgroups started, [0] fallback -- if the Gibbs
  // kernel has not started within gpat ticks (s_memrealtime, 100 MHz), the likelihood
  // workgroups update every task themselves (bit-identical) and the Gibbs kernel leaves
  unsigned long long* grole;   // [RB][16] (one 128-B line per chain block)
  unsigned* gfb;         // chain-block launches that fell back, since create
  unsigned gep, gpat;    // this launch's epoch (the host counts gsep launches), patience
  int ctiles;            // nmc_k_sweep, the control wave in the tile queue (NMC_CTL_TILES):
                         // 0 never, 1 only while the other waves have more than a round of
                         // entries left (default), 2 like every other wave
  int gtiles;            // nmc_k_sweep, the Gibbs wave after its task (NMC_GIBBS_TILES): 0 no
                         // tiles, 1 as ctiles 1 (default)
  int rows_lds;          // 1: each workgroup stages its group's rows in LDS once per launch
  int tile;              // target rows per likelihood tile (nmc_tiles)
  unsigned* cnt;         // [CB][P][32] publish counters (persistent partial): zeroed at create,
                         // then they keep counting across launches (targets offset by pbase);
                         // reset only before pbase would overflow (nestmc.hip nmc_run)
  unsigned* tmo;         // timeout word: pinned host memory, mapped (host reads it directly)
  // variates of iterations [vbase, vbase + vcap): filled by nmc_k_fill
  double* vzl;           // [t][P][G][C][2] {proposal normal, log accept uniform}
  // zin: the step's {z, log u} are drawn inside the step kernel (jobs in the step's tile
  // queue) and nmc_k_fill is not launched (nmc_k_sweep: every variate, NMC_ZIN=1; nmc_k_run:
  // build option NMC_ZIN_BUILD=1 only, the fill still writes vh); 0: nmc_k_fill writes vzl
  // (+ vh) and the control wave DMAs each step's pair into LDS
  int zin;
  double* vh;            // [t][P][C][2]    {hyper mean normal, hyper Gamma(a) draw}
  int vbase, vcap;
  const double* rz;      // replay [iter][P][G][C]
  const double* ru;
  const double* rhz;     // replay [iter][P][C]
  const double* rhu;
  int replay_n;
  int burn, thin, tune_interval, n_rows, cols;
  double* samples;       // [row][col][C]
  uint8_t* tflag;        // trace [iter][P][G][C]
  double* tllp;
  int trace_n;
  // Resident launch (nmc_k_run<..., RES = true>; nestmc.hip nmc_set_resident): one launch
  // serves consecutive nmc_run calls of a sampling loop.  At the end of a call every
  // workgroup completes its results as a launch does (the last Gibbs tasks, sample rows),
  // counts itself done and waits for the host's next command; workgroup 0 alone reads the
  // command word in pinned host memory and relays it (rsync) to the others, so all take the
  // same decision -- a new end, or the park after ridle ticks of s_memrealtime (100 MHz)
  // without one.  The groups' rows and the chain state stay in LDS between calls; the state
  // goes to HBM when the launch parks.
  unsigned long long* rcmd;   // pinned host, mapped: (end << 32) | seq; end 0xffffffff = park
  unsigned* rsync;       // device, zeroed per launch: the relay (end << 32) | seq, one copy
                         // per XCD line (NMC_RSYNC_REL + 32 k), the done count (NMC_RSYNC_CNT)
                         // and the calls' start / loop-end clock maxima (NMC_RSYNC_MAX, u64)
  unsigned* rack;        // pinned host: [0] last seq taken, [1] 0x80000000 | seq when parked,
                         // [2], [3] s_memrealtime when it was taken (lo, hi)
  unsigned* rdone;       // pinned host, written by the last workgroup done: {seq done, 0, then
                         // the s_memrealtime (lo, hi) of: done, the latest loop end, the
                         // latest start of the call}
  unsigned rseq;         // the latest seq the host issued before this launch
  unsigned ridle;        // idle ticks before workgroup 0 parks the launch
  unsigned long long* stamps;   // diagnostic build only (-DNMC_STAMPS)
};

// The chain of this lane in step-kernel chain block cb (64 chains per workgroup, one per
// lane), and whether the lane's chain exists.
__device__ __forceinline__ int nmc_lane_chain(const Dev&, int cb, int lane) {
  return cb * 64 + lane;
}
__device__ __forceinline__ bool nmc_lane_owns(const Dev& d, int c, int) { return c < d.C; }

enum { NMC_RUN_HYPER_LOAD = 1 };
template <bool B> struct nmc_bool_c { static constexpr bool value = B; };
// Dev.rsync word offsets (u32): relay lines, done counter, clock maxima; 512 words in all
enum { NMC_RSYNC_REL = 0, NMC_RSYNC_CNT = 256, NMC_RSYNC_MAX = 288, NMC_RSYNC_WORDS = 512 };
// Largest step-kernel workgroup (build option): 512 threads = 8 waves, 256 VGPRs per lane;
// 768 = 12 waves (three per SIMD) caps the kernel at 168 VGPRs.
#ifndef NMC_RUN_THREADS
#define NMC_RUN_THREADS 512
#endif
// Likelihood tiles per group (nmc_tiles) = partial-sum slots per accumulator.
#ifndef NMC_NSLOT_N
#define NMC_NSLOT_N 16
#endif
enum { NMC_NSLOT = NMC_NSLOT_N };
enum { NMC_SPIN_LIMIT = 1 << 22 };
// diagnostic stamps buffer (make stamps): 1024 phase / tile words + 4 per workgroup
enum { NMC_STAMP_WORDS = 1024 + 4 * 4096 + 512 };
// CU count the row split is sized for (a full MI355X), whatever the device reports
enum { NMC_SPLIT_CU_BASIS = 256 };

// Offset of the hyper-parameter slot holding the state after iteration t ([2][P][C]:
// slot t & 1, like the values vb[t & 1]); a launch reads one slot and writes the other.
__device__ __forceinline__ size_t nmc_hslot(const Dev& d, int t) {
  return (size_t)(t & 1) * d.P * d.C;
}

// The sample row iteration iter is recorded in, -1 for none (host: nmc_debug_record_rows_host).
__host__ __device__ __forceinline__ int nmc_record_row(const Dev& d, int iter) {
  if (iter < d.burn) return -1;
  if (d.thin == 1) {   // (every post-burn iteration: no integer divisions on the step's path)
    const int row = iter - d.burn;
    return row < d.n_rows ? row : -1;
  }
  if ((iter % d.thin) != 0) return -1;
  const int first = ((d.burn + d.thin - 1) / d.thin) * d.thin;
  const int row = (iter - first) / d.thin;
  return row < d.n_rows ? row : -1;
}

// ---------------------------------------------------------------------------
// LDS carve, in columns of 64 doubles (one per lane); the host computes the same.
// ---------------------------------------------------------------------------
struct nmc_lds_layout {
  int th;      // [P]            current values (control wave writes, all read)
  int part;    // [NACC][NSLOT]  per-tile likelihood partial sums (unused slots: -0.0)
  int st;      // [5][P]         scale, log prior, n acc, n rej, total acc (control wave)
  int hyp;     // [6][P]         mu, sd, log sd, sigma2, sqrt(sigma2/G), 1/sd of the hyper-prior
  int hval;    // [2][G + 1]     Gibbs payload of two tasks (persistent Gibbs-wave mode)
  int hst;     // [P][nleaf][8 + ntail]  stream sums / tail elements (pairwise sum)
  int hleaf;   // [P][nleaf]     leaf sums
  int zl;      // [2][2]         {z, log u} of this and the next step (LDS-DMA, step parity)
  int hv;      // [2P]           {hyper z, gamma} of the Gibbs update (LDS-DMA)
  int cw;      // [8]            control-wave values across the step barriers
  int flag;    // [1]            broadcast / epoch words
  int xchg;    // [2][8]         stream sums exchanged by the two compute waves
  int rows;    // [nrows_lds][NF] the group's observation rows (staged once per launch)
  int total;   // columns
};
__host__ __device__ inline nmc_lds_layout nmc_lds(int nacc, int P, int partial, int nleaf,
                                                  int ntail, int W, int G, int hlds,
                                                  int row_doubles = 0) {
  nmc_lds_layout L;
  L.th = 0;
  L.part = L.th + P;
  L.st = L.part + nacc * NMC_NSLOT;   // partial slots per accumulator (unused: -0.0)
  L.hyp = L.st + 5 * P;
  L.hval = L.hyp + (partial ? 6 * P : 0);
  L.hst = L.hval + (partial && hlds ? 2 * (G + 1) : 0);   // two payload buffers (+1 DMA pad)
  L.hleaf = L.hst + (partial ? P * nleaf * (8 + ntail) : 0);
  L.zl = L.hleaf + (partial ? P * nleaf : 0);
  L.hv = L.zl + 4;
  L.cw = L.hv + (partial ? 2 * P : 0);
  L.flag = L.cw + 8;    // (NMC_CW_* uses all 8 columns)
  L.xchg = L.flag + 1;
  L.rows = L.xchg;
  // (+1 column: the pipelined likelihood loop prefetches one block past a wave's rows)
  L.total = L.rows + (row_doubles > 0 ? (row_doubles + 63) / 64 + 1 : 0);
  return L;
}
enum { NMC_ST_S = 0, NMC_ST_LP, NMC_ST_NA, NMC_ST_NR, NMC_ST_TA };
enum { NMC_HY_MU = 0, NMC_HY_SD, NMC_HY_LSD, NMC_HY_S2, NMC_HY_SDM, NMC_HY_ISD };
// control-wave columns of the LDS carve (cw): LPC/LPP: priors of the step made by the
// Gibbs wave; NAA..TA: counter outcomes of the decided step; PN: the next step's proposal
// (nmc_k_run's restart without gathers: written between the step's barriers A and B)
enum { NMC_CW_LPC = 0, NMC_CW_LPP, NMC_CW_NAA, NMC_CW_NRA, NMC_CW_NAR, NMC_CW_NRR, NMC_CW_TA,
       NMC_CW_PN };

// Chunk k of nchunks of [r0, r1) (contiguous, balanced).
__device__ __forceinline__ void nmc_chunk(int64_t r0, int64_t r1, int k, int nchunks,
                                          int64_t* a, int* n) {
  const int64_t len = r1 - r0;
  const int64_t per = (len + nchunks - 1) / nchunks;
  int64_t s = r0 + (int64_t)k * per;
  int64_t e = s + per;
  if (s > r1) s = r1;
  if (e > r1) e = r1;
  *a = s;
  *n = (int)(e - s);
}

// ---------------------------------------------------------------------------
// Row tiles of one group (the likelihood partition): NT = min(NSLOT, ceil(n/tile)) tiles
// (tile = 64 rows unless a diagnostics override sets it) of a multiple of 16 rows, so
// every tile but the last runs whole 16-row blocks of the pipelined loop.  Depends only
// on the group's row count: the tile partials -- and so every log-likelihood sum -- are
// the same whichever wave computes a tile, whatever the chain count, launch mode or GPU
// count.  Tile k covers [start(k), start(k) + len(k)).  (A two-length partition -- the
// first half of the tiles carrying 5/8 of the rows -- measured 9.6 against 8.4 us per
// iteration at cfg 3: the late tiles were not the tail.)
struct nmc_tiling {
  int nt;     // tiles
  int h;      // tiles [0, h) have a rows, [h, nt) b rows (the last one the remainder)
  int a, b;
  int n;
  __device__ __forceinline__ int start(int k) const { return k < h ? k * a : h * a + (k - h) * b; }
  __device__ __forceinline__ int len(int k) const {
    const int s = start(k);
    const int e = s + (k < h ? a : b);
    return (e < n ? e : n) - s;
  }
};
__device__ __forceinline__ nmc_tiling nmc_tiles(int n, int tile) {
  nmc_tiling T;
  T.n = n > 0 ? n : 0;
  if (n <= 0) {
    T.nt = 1; T.h = 1; T.a = T.b = 0;
    return T;
  }
  int t = (n + tile - 1) / tile;
  if (t > NMC_NSLOT) t = NMC_NSLOT;
  int per = (n + t - 1) / t;
  per = (per + 15) & ~15;
  T.a = T.b = per;
  T.nt = (n + per - 1) / per;
  T.h = T.nt;
  return T;
}
