// sweep_gibbs.h -- the Gibbs side of nmc_k_sweep (sweep.h, which includes this file where
// its kernel needs it: after nmc_sweep_args and the variate helpers).  The one-load update
// nmc_hyper_once; the Dev.gsep role protocol nmc_grole_*; the likelihood workgroups' fallback
// update nmc_hyper_update_stream; the Gibbs workgroup's loop nmc_sweep_gibbs_wg and its
// kernel nmc_k_sweep_gibbs.
#pragma once

// HyperParameter.update (:463-498) of parameter q for one chain block, as nmc_hyper<SC1, NS,
// true> (the same streams, sums and order, so the same bits) but loading the G values once:
// each wave keeps its NS streams' values in registers for the second pass (sum of squares
// about the new mean) instead of fetching them again -- one device-scope round trip per
// task instead of two.  The tail stream's raw values wait in LDS (pass 1 writes them).
template <int NS>
__device__ __forceinline__ void nmc_hyper_once(const Dev& d, const double* src, int cb, int t,
                                               double* lds, const nmc_lds_layout& L, int q) {
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int W = blockDim.x >> 6;
  const int P = d.P, G = d.G, C = d.C, nl = d.nleaf, ncol = 8 + d.ntail;
  const int per = 8 + (d.ntail ? 1 : 0);
  const int c = nmc_lane_chain(d, cb, lane);
  const int cc = c < C ? c : C - 1;
  const int sbeg = q * nl * per, nst = (q + 1) * nl * per;
  struct Strm {
    int j, pl, m, m8;
    const double* xp;
  };
  auto strm = [&](int s) {
    Strm r;
    r.j = s % per;
    r.pl = s / per;
    const int lf = r.pl % nl;
    const int a = nl == 1 ? 0 : d.leaf[lf];
    r.m = nl == 1 ? G : d.leaf[lf + 1] - a;
    r.m8 = r.m >= 8 ? r.m - r.m % 8 : 0;
    r.xp = src + ((size_t)q * G + a) * C + cc;
    return r;
  };
  // one round: this wave's streams w, w + W, ..., w + (NS-1) W of [sbeg, nst)
  static_assert(NS >= 1, "streams per wave");
  double v[NS][16];
#pragma unroll
  for (int k = 0; k < NS; ++k) {
    const int s = sbeg + w + k * W;
    const Strm r = strm(s < nst ? s : sbeg);
    const int cnt = s < nst && r.j < 8 ? r.m8 >> 3 : 0;
#pragma unroll
    for (int u = 0; u < 16; ++u)
      v[k][u] = u < cnt ? nmc_ldv<NMC_SRC_SC1>(r.xp + (size_t)(r.j + 8 * u) * C) : 0.0;
  }
  auto pass = [&](bool sq) {
    const double mu = sq ? lds[(L.hyp + NMC_HY_MU * P + q) * 64 + lane] : 0.0;
#pragma unroll
    for (int k = 0; k < NS; ++k) {
      const int s = sbeg + w + k * W;
      if (s >= nst) continue;
      const Strm r = strm(s);
      double* out = lds + (size_t)(L.hst + r.pl * ncol) * 64 + lane;
      if (r.j < 8) {
        const int cnt = r.m8 >> 3;
        double acc = 0.0;
#pragma unroll
        for (int u = 0; u < 16; ++u) {
          if (u < cnt) {
            double x = v[k][u];
            if (sq) {
              x = x - mu;
              x = x * x;
            }
            acc = u == 0 ? x : acc + x;
          }
        }
        out[r.j * 64] = acc;
      } else {   // the tail: raw values in pass 1, their squares about mu in pass 2
        for (int u = r.m8; u < r.m; ++u) {
          double x = sq ? out[(8 + u - r.m8) * 64] : nmc_ldv<NMC_SRC_SC1>(r.xp + (size_t)u * C);
          if (sq) {
            x = x - mu;
            x = x * x;
          }
          out[(8 + u - r.m8) * 64] = x;
        }
      }
    }
  };
  // (a wave holds NS streams: the whole parameter's streams in one round)
  pass(false);
  __syncthreads();
  if (w == 0) {
    const double tot = nmc_hyper_combine(d, lds, L, q, lane);
    const double sdm = lds[(L.hyp + NMC_HY_SDM * P + q) * 64 + lane];
    const double hz = lds[L.hv * 64 + (q * 64 + lane) * 2];
    lds[(L.hyp + NMC_HY_MU * P + q) * 64 + lane] = tot / G + sdm * hz;   // mu ~ N(mean, s2/G)
  }
  __syncthreads();
  pass(true);
  __syncthreads();
  if (w == 0) {
    const bool own = nmc_lane_owns(d, c, lane);
    const int row = nmc_record_row(d, t);
    const double ss = nmc_hyper_combine(d, lds, L, q, lane);
    const double hat = ss / (double)(G - 1);
    const double scale = d.ha * hat;
    const double hx = lds[L.hv * 64 + (q * 64 + lane) * 2 + 1];
    // scipy invgamma.rvs: (1/gammainccinv(a, U)) * scale + loc; loc when scale == 0
    const double s2n = scale == 0.0 ? 0.0 : (1.0 / hx) * scale;
    const double sdn = sqrt(s2n);
    const double lsd = log(sdn);
    const double m = lds[(L.hyp + NMC_HY_MU * P + q) * 64 + lane];
    lds[(L.hyp + NMC_HY_SD * P + q) * 64 + lane] = sdn;
    lds[(L.hyp + NMC_HY_LSD * P + q) * 64 + lane] = lsd;
    lds[(L.hyp + NMC_HY_S2 * P + q) * 64 + lane] = s2n;
    lds[(L.hyp + NMC_HY_ISD * P + q) * 64 + lane] = 1.0 / sdn;
    if (own) {
      const size_t ho = nmc_hslot(d, t) + (size_t)q * C + c;
      __hip_atomic_store(d.mu + ho, m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(d.s2 + ho, s2n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(d.hsd + ho, sdn, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(d.hlsd + ho, lsd, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (row >= 0) {
        double* out = d.samples + ((size_t)row * d.cols + (size_t)q * (G + 2)) * C + c;
        out[0] = m;
        out[C] = s2n;
      }
    }
  }
}

// ---- Dev.gsep without co-scheduling ----
// The two kernels of the gsep path each wait on counters only the other advances, and HIP
// does not promise that kernels on two streams run at the same time (a profiler's PMC pass,
// AMD_SERIALIZE_KERNEL or a shared hardware queue serialize them).  So each chain block of a
// launch has a role word (Dev.grole, epoch = Dev.gep): a Gibbs workgroup marks itself
// started once its first task's values are published; if no Gibbs workgroup of the chain
// block has started within Dev.gpat ticks, whichever side notices first sets the fallback
// bit.  Then the Gibbs workgroups leave, and the likelihood workgroups' Gibbs waves update
// every task of the launch themselves (nmc_hyper_update_stream: the same sums, draws and
// outputs, so the same bits), group 0's writing and counting them as the Gibbs workgroup
// would.  Either every task of a (launch, chain block) comes from the Gibbs kernel or every
// one from the fallback: the bit is only set while no Gibbs workgroup has started.
__device__ __forceinline__ unsigned long long* nmc_grole(const Dev& d, int cb) {
  return d.grole + (size_t)cb * 16;
}
__device__ __forceinline__ bool nmc_grole_is_fallback(const Dev& d, unsigned long long v) {
  return (unsigned)(v >> 32) == d.gep && (v & 1ull);
}
// (one lane) set the fallback bit of this launch; false: a Gibbs workgroup has started
__device__ __forceinline__ bool nmc_grole_fallback(const Dev& d, int cb) {
  unsigned long long* r = nmc_grole(d, cb);
  const unsigned long long ep = (unsigned long long)d.gep << 32;
  unsigned long long v = __hip_atomic_load(r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  for (;;) {
    if ((unsigned)(v >> 32) == d.gep) {
      if (v & 1ull) return true;
      if (v != ep) return false;   // started
    }
    if (__hip_atomic_compare_exchange_strong(r, &v, ep | 1ull, __ATOMIC_RELAXED,
                                             __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
      __hip_atomic_fetch_add(d.gfb, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      return true;
    }
  }
}
// (one lane) a Gibbs workgroup starts its first task; false: the fallback is set, leave
__device__ __forceinline__ bool nmc_grole_start(const Dev& d, int cb) {
  unsigned long long* r = nmc_grole(d, cb);
  const unsigned long long ep = (unsigned long long)d.gep << 32;
  unsigned long long v = __hip_atomic_load(r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  for (;;) {
    unsigned long long nv = ep + 2ull;
    if ((unsigned)(v >> 32) == d.gep) {
      if (v & 1ull) return false;
      nv = v + 2ull;
    }
    if (__hip_atomic_compare_exchange_strong(r, &v, nv, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                             __HIP_MEMORY_SCOPE_AGENT))
      return true;
  }
}
// The calling wave's patience clock (s_memrealtime: 100 MHz, one clock for the chip).
__device__ __forceinline__ bool nmc_grole_patience_over(const Dev& d, unsigned long long t0) {
  return __builtin_amdgcn_s_memrealtime() - t0 > (unsigned long long)d.gpat;
}
// A Gibbs workgroup's wait for its FIRST task's publications (wave 0; wave-uniform result):
// 1 go on (started), 0 leave (the fallback is set, or a timeout recorded in d.tmo).
__device__ __forceinline__ int nmc_grole_first_wait(const Dev& d, int cb, int q, unsigned target) {
  const int lane = threadIdx.x & 63;
  target += (unsigned)d.G * d.pbase;
  unsigned* ctr = nmc_counter(d, cb, q, lane & 7);
  const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
  bool patient = true;
  for (unsigned spins = 0;; ++spins) {
    const unsigned v =
        lane < 8 ? __hip_atomic_load(ctr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
    unsigned tot = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) tot += __builtin_amdgcn_readlane(v, k);
    if (tot >= target) {
      const bool go = lane == 0 ? nmc_grole_start(d, cb) : false;
      return __builtin_amdgcn_readlane((int)go, 0);
    }
    if ((spins & 63) == 63) {
      const unsigned long long rv =
          __hip_atomic_load(nmc_grole(d, cb), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (nmc_grole_is_fallback(d, rv)) return 0;
      if (patient && nmc_grole_patience_over(d, t0)) {
        const bool fb = lane == 0 ? nmc_grole_fallback(d, cb) : false;
        if (__builtin_amdgcn_readlane((int)fb, 0)) return 0;
        patient = false;   // a sibling has started: the likelihood kernel runs, wait for it
      }
    }
    if ((spins & 255) == 255 &&
        __hip_atomic_load(d.tmo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != 0)
      return 0;
    if (spins >= NMC_SPIN_LIMIT) {
      __hip_atomic_store(d.tmo, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      return 0;
    }
    __builtin_amdgcn_s_sleep(2);
  }
}
// A likelihood workgroup's Gibbs wave waiting for task (cb, q)'s ready count (wave-uniform):
// 1 ready, -1 fallback (update it here), 0 timeout (d.tmo).
__device__ __forceinline__ int nmc_grole_own_wait(const Dev& d, int cb, int q, unsigned target) {
  const int lane = threadIdx.x & 63;
  const unsigned* ctr = nmc_hrd(d, cb, q);
  const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
  bool patient = true;
  for (unsigned spins = 0;; ++spins) {
    if (__hip_atomic_load(ctr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= target) return 1;
    if ((spins & 63) == 63) {
      const unsigned long long rv =
          __hip_atomic_load(nmc_grole(d, cb), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (nmc_grole_is_fallback(d, rv)) return -1;
      if (patient && nmc_grole_patience_over(d, t0)) {
        const bool fb = lane == 0 ? nmc_grole_fallback(d, cb) : false;
        if (__builtin_amdgcn_readlane((int)fb, 0)) return -1;
        patient = false;   // a Gibbs workgroup has started: wait as long as it takes
      }
    }
    if ((spins & 255) == 255 &&
        __hip_atomic_load(d.tmo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != 0)
      return 0;
    if (spins >= NMC_SPIN_LIMIT) {
      __hip_atomic_store(d.tmo, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      return 0;
    }
    __builtin_amdgcn_s_sleep(2);
  }
}
// The fallback's update of task (tq, q) by one wave: HyperParameter.update (:463-498) with
// the values streamed from global memory (sc1) in 8-value chunks -- nmc_pairwise_stream,
// the order of nmc_hyper / nmc_hyper_once -- and the task's variates from the fill's ring or
// drawn here (Dev.zin).  write: the global slot of tq and the sample row (group 0's wave).
// Inlined, with short chunks: a rare path (the Gibbs kernel did not run beside the sweep)
// whose registers must not cost the likelihood loop -- as a call it added 58 SGPR spills and
// 128 B of scratch to the cfg-4 instance; inlined with 32-value chunks, one VGPR spill.
__device__ __forceinline__ void nmc_hyper_update_stream(const Dev& d, int cb, int tq, int q,
                                                     int cc, double* lds, int hyp, bool write) {
  const int lane = threadIdx.x & 63;
  const int P = d.P, G = d.G, C = d.C;
  const double* src = ((tq & 1) ? d.vb1 : d.vb0) + (size_t)q * G * C + cc;
  nmc_d2 hv;
  if (d.zin) {
    hv = nmc_sweep_hyper_variate(d.rhz, d.rhu, d.replay_n, d.rng_mode, P, C,
                                 (uint32_t)(d.chain_base + cc), d.seed, d.ha, d.hlga, tq, q, cc);
  } else {
    const size_t hvi = (((size_t)(tq - d.vbase) * P + q) * C + cc) * 2;
    hv.a = d.vh[hvi];
    hv.b = d.vh[hvi + 1];
  }
  const double sdm = sqrt(lds[(hyp + NMC_HY_S2 * P + q) * 64 + lane] / G);
  const double tot = nmc_pairwise_stream<8>(d, src, false, 0.0);
  const double mu = tot / G + sdm * hv.a;                        // mu ~ N(mean(x), sqrt(s2/G))
  const double ss = nmc_pairwise_stream<8>(d, src, true, mu);
  nmc_hyper_finish(d, cb, tq, q, lds, hyp, write, mu, ss, hv.b);
}

// SYNC_OWN's Gibbs workgroup kb = (chain block, parameter q), four waves: every task (t, q)
// of the launch in order, once its publication is complete -- HyperParameter.update
// (:463-498) computed once per chain block, written through and counted ready (nmc_hrd)
// for the likelihood workgroups' Gibbs waves.
// GW: the waves of the Gibbs kernel of its own (nmc_k_sweep_gibbs: the one-load update, four
// streams per wave on 4 waves, two on 8); 0: inside nmc_k_sweep, where the update streams its
// values twice (168-VGPR budget shared with the likelihood code).
template <class Fam, int GW>
__device__ __forceinline__ void nmc_sweep_gibbs_wg(int kb, double* lds) {
  const nmc_sweep_args<Fam>* A = nmc_sweep_args_at<Fam>();
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int W = blockDim.x >> 6;
  const int i0 = A->i0, i1 = A->i1;
#define d (A->d)
  const int P = d.P, G = d.G, C = d.C;
  const int hcb = d.cb0 + kb / P, q = kb % P;
  const int c = hcb * 64 + lane;
  const int cc = c < C ? c : C - 1;
  const nmc_lds_layout H = nmc_lds(0, P, 1, d.nleaf, d.ntail, W, G, 0, 0);
  double* hy = lds + H.hyp * 64 + lane;
  if (w == 0) {   // the state of q after iteration i0-1 (slot (i0-1) & 1)
    const size_t ho = nmc_hslot(d, i0 - 1) + (size_t)q * C + cc;
    hy[(NMC_HY_MU * P + q) * 64] = d.mu[ho];
    hy[(NMC_HY_SD * P + q) * 64] = d.hsd[ho];
    hy[(NMC_HY_LSD * P + q) * 64] = d.hlsd[ho];
    hy[(NMC_HY_S2 * P + q) * 64] = d.s2[ho];
  }
#ifdef NMC_STAMPS   // chain block 0's Gibbs workgroups, iterations < 8 of the launch:
                    // stamps[1024 + 4*4096 + ((t - i0) * 16 + 12 + q) * 4 + k]
#define NMC_GSTAMP(k)                                                                        \
  do {                                                                                       \
    if (d.stamps && hcb == 0 && q < 4 && t - i0 < 8 && threadIdx.x == 0)                      \
      d.stamps[1024 + 4 * 4096 + ((t - i0) * 16 + 12 + q) * 4 + (k)] = __builtin_amdgcn_s_memtime(); \
  } while (0)
#else
#define NMC_GSTAMP(k) do {} while (0)
#endif
  for (int t = i0; t < i1; ++t) {
    A = nmc_sweep_args_at<Fam>();
    NMC_GSTAMP(3);
    if (GW > 0 && t == i0) {   // (Dev.gsep: the first task starts this workgroup, or the
                               //  likelihood workgroups have taken the launch over)
      if (threadIdx.x < 64) {
        const int r = nmc_grole_first_wait(d, hcb, q, (unsigned)d.G);
        if (threadIdx.x == 0) lds[H.flag * 64] = r ? 1.0 : 0.0;
      }
      __syncthreads();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      if (lds[H.flag * 64] == 0.0) break;
    } else if (!nmc_wait_published(d, hcb, q, (unsigned)d.G * (unsigned)(t - i0 + 1), lds, H)) {
      break;
    }
    NMC_GSTAMP(0);
    if (w == 0) {   // the task's variates and sqrt(s2 / G) of the previous update
      nmc_d2 hv;
      if (d.zin) {
        hv = nmc_sweep_hyper_variate(d.rhz, d.rhu, d.replay_n, d.rng_mode, d.P, d.C,
                                     (uint32_t)(d.chain_base + cc), d.seed, d.ha, d.hlga, t, q,
                                     cc);
      } else {
        const size_t hvi = (((size_t)(t - d.vbase) * d.P + q) * d.C + cc) * 2;
        hv.a = d.vh[hvi];
        hv.b = d.vh[hvi + 1];
      }
      lds[H.hv * 64 + (q * 64 + lane) * 2] = hv.a;
      lds[H.hv * 64 + (q * 64 + lane) * 2 + 1] = hv.b;
      hy[(NMC_HY_SDM * d.P + q) * 64] = sqrt(hy[(NMC_HY_S2 * d.P + q) * 64] / d.G);
    }
    __syncthreads();
    // HyperParameter.update (:463-498) for the chain block, written through to the global
    // slot of t (and the sample row); wave 0 stored it and counts it ready
#ifdef NMC_STAMPS   // the update's phases (entry 14 + q): pass 1, mean, pass 2
    {
      const double* src = (t & 1) ? d.vb1 : d.vb0;
      auto gs2 = [&](int k) {
        if (d.stamps && hcb == 0 && q < 2 && t - i0 < 8 && threadIdx.x == 0)
          d.stamps[1024 + 4 * 4096 + ((t - i0) * 16 + 14 + q) * 4 + k] = __builtin_amdgcn_s_memtime();
      };
      nmc_hyper_streams<NMC_SRC_SC1, false, 4>(d, src, cc, lds, H, q);
      __syncthreads();
      gs2(0);
      if (w == 0) {
        const double tot = nmc_hyper_combine(d, lds, H, q, lane);
        const double sdm = lds[(H.hyp + NMC_HY_SDM * P + q) * 64 + lane];
        const double hz = lds[H.hv * 64 + (q * 64 + lane) * 2];
        lds[(H.hyp + NMC_HY_MU * P + q) * 64 + lane] = tot / G + sdm * hz;
      }
      __syncthreads();
      gs2(1);
      nmc_hyper_streams<NMC_SRC_SC1, true, 4>(d, src, cc, lds, H, q);
      __syncthreads();
      gs2(2);
      // (diagnostics only: the full update below runs on the same inputs)
    }
#endif
    if (GW > 0 && d.nleaf * (8 + (d.ntail ? 1 : 0)) <= 16)   // every stream in one round
      nmc_hyper_once<GW == 8 ? 2 : 4>(d, (t & 1) ? d.vb1 : d.vb0, hcb, t, lds, H, q);
    else
      nmc_hyper<NMC_SRC_SC1, GW == 8 ? 1 : 4, true>(d, (t & 1) ? d.vb1 : d.vb0, hcb, t, lds, H,
                                                    true, q);
    NMC_GSTAMP(1);
    if (w == 0) {
      nmc_drain_vm();
      if (lane == 0)
        __hip_atomic_fetch_add(nmc_hrd(d, hcb, q), 1u, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
    }
    NMC_GSTAMP(2);
  }
#undef NMC_GSTAMP
  nmc_drain_vm();
#undef d
}

// Dev.gsep: the Gibbs workgroups of SYNC_OWN as a kernel of their own (RB * P workgroups
// of four waves, the small nmc_lds carve), launched on a second stream beside
// nmc_k_sweep's RB * G likelihood workgroups: co-resident with two 61-KB likelihood
// workgroups per CU where one kernel with a single LDS size would not be.
// GW: its waves (4: four streams per wave, every stream of a 256-group update in one round)
template <class Fam, int GW>
__global__ void __launch_bounds__(64 * GW) nmc_k_sweep_gibbs(nmc_sweep_args<Fam> a_arg) {
  (void)a_arg;
  extern __shared__ __attribute__((aligned(16))) double lds[];
  // (its waves share a CU with two likelihood workgroups: issue ahead of their tile waves,
  //  the update is on every step's critical path; NMC_NOPRIO bit 2 drops it)
  if (!(a_arg.d.noprio & 2)) __builtin_amdgcn_s_setprio(3);
  nmc_sweep_gibbs_wg<Fam, GW>((int)blockIdx.x, lds);
}
