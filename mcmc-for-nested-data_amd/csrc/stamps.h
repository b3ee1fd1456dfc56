// stamps.h -- the diagnostic builds' in-kernel clock stamps: the NMC_STAMP family
// (make stamps, -DNMC_STAMPS) and NMC_CS (make cstamps, -DNMC_CSTAMPS).  Every macro is empty
// in the shipped build.
#pragma once

// Diagnostic build only (make stamps -> libnestmc_stamps.so, never shipped): shader-
// clock stamps of workgroups 0 and last, waves 0 and W-1, first 8 iterations of a
// launch: stamps[((blk * 2 + wv) * 8 + iter) * 8 + slot].
#ifdef NMC_STAMPS
#define NMC_STAMP(t, slot)                                                              \
  do {                                                                                  \
    const int sb_ = blockIdx.x == 0 ? 0 : (blockIdx.x == gridDim.x - 1 ? 1 : -1);         \
    const int sw_ = w == 0 ? 0 : (w == W - 1 ? 1 : -1);                                 \
    if (d.stamps && sb_ >= 0 && sw_ >= 0 && (t) - i0 < 8 && lane == 0)                  \
      d.stamps[((sb_ * 2 + sw_) * 8 + ((t) - i0)) * 16 + (slot)] = __builtin_amdgcn_s_memtime(); \
  } while (0)
// auxiliary wave 1 of workgroup 0, into the wave-W-1 row of block 0 (slots 13-15)
#define NMC_STAMP_AUX(t, slot)                                                          \
  do {                                                                                  \
    if (d.stamps && blockIdx.x == 0 && w == 1 && (t) - i0 < 8 && lane == 0)              \
      d.stamps[((0 * 2 + 1) * 8 + ((t) - i0)) * 16 + (slot)] = __builtin_amdgcn_s_memtime(); \
  } while (0)
// compute wave half 0 (wave 1) of workgroup 0, into the control-wave row (slots 13-15)
#define NMC_STAMP_CMP(t, slot)                                                          \
  do {                                                                                  \
    if (d.stamps && blockIdx.x == 0 && w == 1 && (t) - i0 < 8 && lane == 0)              \
      d.stamps[((0 * 2 + 0) * 8 + ((t) - i0)) * 16 + (slot)] = __builtin_amdgcn_s_memtime(); \
  } while (0)
// tile k of the step (t, p), workgroup 0, first 8 steps of a launch: start/end clock
// and the wave that ran it, stamps[512 + ((step * 16 + k) * 4 + {0, 1, 2})]
#define NMC_TILE_STAMP(k, e)                                                              \
  do {                                                                                    \
    const int si_ = (t - i0) * P + p;                                                     \
    if (d.stamps && blockIdx.x == 0 && si_ < 8 && (k) < 16 && lane == 0) {               \
      d.stamps[512 + (si_ * 16 + (k)) * 4 + (e)] = __builtin_amdgcn_s_memtime();         \
      if (e) d.stamps[512 + (si_ * 16 + (k)) * 4 + 2] = (unsigned long long)w;           \
    }                                                                                     \
  } while (0)
// wave w of workgroup 0 arriving at barrier A of step si (< 8): stamps[512 + (si * 16 + w) * 4 + 3]
#define NMC_ARRIVE_STAMP(si)                                                              \
  do {                                                                                    \
    if (d.stamps && blockIdx.x == 0 && (si) < 8 && w < 16 && lane == 0)                   \
      d.stamps[512 + ((si) * 16 + w) * 4 + 3] = __builtin_amdgcn_s_memtime();              \
  } while (0)
// wave w of workgroup 0 at step si (< 8): stamps[1024 + 4 * 4096 + (si * 16 + w) * 4 + k],
// k = 0 step top, 1 before the first take, 2 first take resolved
#define NMC_RS_STAMP(si, k)                                                               \
  do {                                                                                    \
    if (d.stamps && blockIdx.x == 0 && (si) < 8 && w < 16 && lane == 0)                   \
      d.stamps[1024 + 4 * 4096 + ((si) * 16 + w) * 4 + (k)] = __builtin_amdgcn_s_memtime(); \
  } while (0)
// the control wave of workgroup 0 at step si: stamps[512 + (si * 16 + 12 + k) * 4 + 3],
// k = 0 barrier A passed, 1 decided, 2 barrier B passed (W <= 12)
#define NMC_CTL_STAMP(si, k)                                                              \
  do {                                                                                    \
    if (d.stamps && blockIdx.x == 0 && (si) < 8 && w == 0 && lane == 0)                   \
      d.stamps[512 + ((si) * 16 + 12 + (k)) * 4 + 3] = __builtin_amdgcn_s_memtime();       \
  } while (0)
// every workgroup b: stamps[1024 + b * 4 + {entry, prologue done, loop done, exit}],
// s_memrealtime (100 MHz, one clock for the whole chip; tools/launchtl.py)
#define NMC_RUN_SL(slot)                                                                  \
  do {                                                                                    \
    if (d.stamps && threadIdx.x == 0)                                                     \
      d.stamps[1024 + (size_t)blockIdx.x * 4 + (slot)] = __builtin_amdgcn_s_memrealtime(); \
  } while (0)
#else
#define NMC_RUN_SL(slot) do {} while (0)
#define NMC_TILE_STAMP(k, e) do {} while (0)
#define NMC_ARRIVE_STAMP(si) do {} while (0)
#define NMC_RS_STAMP(si, k) do {} while (0)
#define NMC_CTL_STAMP(si, k) do {} while (0)
#define NMC_STAMP_CMP(t, slot) do {} while (0)
#define NMC_STAMP_AUX(t, slot) do {} while (0)
#define NMC_STAMP(t, slot) do {} while (0)
#endif

// Diagnostic build only (make cstamps -> libnestmc_cst.so, never shipped): shader clock of
// workgroup 0's waves at the step loop's phase points, steps 0..15 of a launch:
// stamps[step * 32 + slot], slot = w (wave w arrives at barrier A), 8 (barrier A passed,
// control), 9 (decided), 10 (barrier B passed), 16 + w (wave w's first tile starts); wave 2:
// 11 (barrier B passed, the step before), 12 (the step's likelihood entered), 13 (proposal
// prepared); control: 14 (slot sums done), 15 (log-likelihood finished).  Every
// lane of the wave stores the same value (no lane-divergent store: the kernel's laundered
// argument pointer stays scalar).
#ifdef NMC_CSTAMPS
#define NMC_CS(si, slot)                                                                  \
  do {                                                                                    \
    if (d.stamps && blockIdx.x == 0 && (si) >= 0 && (si) < 16)                            \
      d.stamps[(si) * 32 + (slot)] = __builtin_amdgcn_s_memtime();                        \
  } while (0)
#else
#define NMC_CS(si, slot) do {} while (0)
#endif
