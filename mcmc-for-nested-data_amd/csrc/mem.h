// mem.h -- memory and synchronisation primitives of the step kernels: sc1 loads (nmc_ldv),
// LDS-DMA (nmc_dma16), write-through stores, the publish counters and their bounded polls,
// the workgroup barriers and the laundered kernel-argument pointer (nmc_kdev).
#pragma once

#include "dev.h"

// How the Gibbs update reads the published values from global memory: plain loads after a
// kernel boundary, or sc1 loads in a persistent launch.
enum { NMC_SRC_GLOBAL = 0, NMC_SRC_SC1 = 1 };

template <int SRC>
__device__ __forceinline__ double nmc_ldv(const double* p) {
  if constexpr (SRC == NMC_SRC_SC1)
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // global_load sc1
  else
    return *p;
}

// One wave copies 64 lanes x 16 bytes from global memory straight into LDS
// (global_load_lds_dwordx4: no VGPR destination, so the copy stays in flight across
// the scalar-load likelihood loop).  The issuing wave retires it with its own
// s_waitcnt vmcnt(0) before the barrier that precedes the first read.
typedef __attribute__((address_space(3))) void* nmc_lds_ptr;
typedef __attribute__((address_space(1))) const void* nmc_glb_ptr;
__device__ __forceinline__ void nmc_dma16(const double* src_lane, double* lds_dst) {
  __builtin_amdgcn_global_load_lds((nmc_glb_ptr)src_lane, (nmc_lds_ptr)lds_dst, 16, 0, 0);
}
__device__ __forceinline__ void nmc_drain_vm() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
// Write-through store of v to global memory -- what __hip_atomic_store(relaxed, agent scope)
// emits for a global pointer (global_store_dwordx2 ... sc1) -- for an address held in VGPRs
// whose address space the compiler no longer sees: it would emit a flat store, which counts
// in lgkmcnt as well, and the LDS-only step barrier would then wait for its write-through.
__device__ __forceinline__ void nmc_store_wt(double* p, double v) {
  asm volatile("global_store_dwordx2 %0, %1, off sc1" ::"v"(p), "v"(v) : "memory");
}

// The step's tile grab: lane 0 adds 1 to the LDS counter at ctr, the value before in lane 0 of
// the result (call with the whole wave; the other lanes' results are undefined).  Written as
// the instruction because the compiler orders every LDS access of a wave that also issues
// LDS-DMA behind that wave's outstanding global memory (s_waitcnt vmcnt(0) in front of
// the __hip_atomic_fetch_add's ds_add_rtn_u32): the tile counters are never a DMA target, and
// on the control wave that wait stood for the variate DMA, the sample / trace stores and the
// publish count before every tile.  The compiler does not know of the return in flight either:
// nmc_lds_grab_value waits for it (lgkmcnt) and hands out lane 0's value, and nothing else may
// touch the result.
__device__ __forceinline__ unsigned nmc_lds_grab(unsigned* ctr) {
  const unsigned a = (unsigned)(uintptr_t)(__attribute__((address_space(3))) unsigned*)ctr;
  const unsigned one = 1u;
  unsigned r;
  unsigned long long ex;
  asm volatile(
      "s_mov_b64 %[ex], exec\n\t"
      "s_mov_b64 exec, 1\n\t"
      "ds_add_rtn_u32 %[r], %[a], %[one]\n\t"
      "s_mov_b64 exec, %[ex]"
      : [r] "=&v"(r), [ex] "=&s"(ex)
      : [a] "v"(a), [one] "v"(one)
      : "memory");
  return r;
}
__device__ __forceinline__ int nmc_lds_grab_value(unsigned r) {
  int k;   // (the result is an input only: no tied copy of it in front of the wait)
  asm volatile("s_waitcnt lgkmcnt(0)\n\tv_readlane_b32 %0, %1, 0" : "=s"(k) : "v"(r) : "memory");
  return k;
}

// The calling wave polls the chain block's publish counter until it reaches target
// (bounded; a timeout is recorded in d.tmo and reported by the host).  The counter is
// sharded 8 ways (workgroup g adds to shard g % 8, each shard on its own 128-B line)
// so the G arrivals do not serialise on one line; lanes 0-7 read the shards with one
// sc1 load and the wave sums them.  Wave-uniform result; call with the whole wave.
__device__ __forceinline__ unsigned* nmc_counter(const Dev& d, int cb, int p, int shard) {
  return d.cnt + (((size_t)cb * d.P + p) * 8 + shard) * 32;
}
__device__ __forceinline__ bool nmc_poll_published(const Dev& d, int cb, int p, unsigned target) {
  const int lane = threadIdx.x & 63;
  target += (unsigned)d.G * d.pbase;   // (counts of the context's earlier launches)
  unsigned* ctr = nmc_counter(d, cb, p, lane & 7);
  for (unsigned spins = 0;; ++spins) {
    const unsigned v =
        lane < 8 ? __hip_atomic_load(ctr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
    unsigned tot = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) tot += __builtin_amdgcn_readlane(v, k);
    if (tot >= target) return true;
    if ((spins & 255) == 255 &&
        __hip_atomic_load(d.tmo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != 0)
      return false;
    if (spins >= NMC_SPIN_LIMIT) {
      __hip_atomic_store(d.tmo, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      return false;
    }
    __builtin_amdgcn_s_sleep(2);
  }
}

// The hyper-ready count of (cb, q) (nmc_k_sweep's Gibbs workgroups, SYNC_OWN) and the
// calling wave's bounded poll of such a count.
__device__ __forceinline__ unsigned* nmc_hrd(const Dev& d, int cb, int q) {
  return d.hrd + ((size_t)cb * d.P + q) * 32;
}
__device__ __forceinline__ bool nmc_poll_count(const Dev& d, const unsigned* ctr,
                                               unsigned target) {
  for (unsigned spins = 0;; ++spins) {
    const unsigned v = __hip_atomic_load(ctr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (v >= target) return true;
    if ((spins & 255) == 255 &&
        __hip_atomic_load(d.tmo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != 0)
      return false;
    if (spins >= NMC_SPIN_LIMIT) {
      __hip_atomic_store(d.tmo, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      return false;
    }
    __builtin_amdgcn_s_sleep(2);
  }
}

// Whole-workgroup wait (thread 0 polls, result broadcast through LDS).
__device__ __forceinline__ bool nmc_wait_published(const Dev& d, int cb, int p, unsigned target,
                                                   double* lds, const nmc_lds_layout& L) {
  if (threadIdx.x < 64) {
    const bool r = nmc_poll_published(d, cb, p, target);
    if (threadIdx.x == 0) lds[L.flag * 64] = r ? 1.0 : 0.0;
  }
  __syncthreads();
  // keep the payload loads below the poll (no instruction: wavefront scope)
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  return lds[L.flag * 64] != 0.0;
}

// The step loops' workgroup barrier (nmc_k_run, nmc_k_sweep): LDS traffic only.
// __syncthreads() is a workgroup-scope release/acquire, which waits for every outstanding global store of the wave (vmcnt(0)):
// the control wave's write-through publish and sample stores, the Gibbs wave's hyper-state
// stores would then sit on the step's critical path.  The step loop shares nothing through
// global memory inside the workgroup (a wave whose LDS-DMA must have landed drains vmcnt
// itself first), so the barrier waits for LDS operations only; the "memory" clobber keeps
// the compiler from moving memory accesses across it.
__device__ __forceinline__ void nmc_step_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

// The step kernel's Dev argument (the first kernel argument: offset 0 of the kernarg
// segment) read through a pointer laundered at the top of every step: its fields are
// scalar-loaded (s_load, scalar cache) where a step uses them instead of being hoisted out
// of the persistent loop and held in SGPRs for the whole launch -- some 60 fields, which
// spilled 160-600 SGPRs per instance (MI355X: <= 102 SGPRs per wave).
typedef __attribute__((address_space(4))) const Dev* nmc_kdev_ptr;
__device__ __forceinline__ const Dev* nmc_kdev() {
  nmc_kdev_ptr p = (nmc_kdev_ptr)__builtin_amdgcn_kernarg_segment_ptr();
#if !defined(NMC_STAMPS)
  // (the stamps build's divergent stamp stores make the backend move the laundered pointer
  //  to VGPRs, an illegal copy: diagnostics keep it plain)
  asm volatile("" : "+s"(p));
#endif
  return (const Dev*)p;
}
