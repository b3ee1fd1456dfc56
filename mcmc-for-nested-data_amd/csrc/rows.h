// rows.h -- the likelihood row loops, chain-on-lane: scalar-load rows (nmc_ll_rows), the
// hand-written {x, y} loops over rows in LDS (broadcast, paired, quad) and their C++ forms
// (nmc_ll_rows_lds, nmc_ll_rows_lds_quad), the LDS-DMA staged loop (nmc_ll_rows_staged), the
// fixed-order tile-slot sum (nmc_sum_slots) and the permlane helpers they share.
#pragma once

#include "dev.h"
#include "mem.h"

// Both halves' values of v in every lane (v_permlane32_swap, gfx950): lo = lanes 0-31's
// value of the lane's pair, hi = lanes 32-63's.
struct nmc_pair2 { double lo, hi; };
__device__ __forceinline__ nmc_pair2 nmc_halves(double v) {
  const unsigned l = (unsigned)__double2loint(v), h = (unsigned)__double2hiint(v);
  const auto a = __builtin_amdgcn_permlane32_swap(l, l, false, false);
  const auto b = __builtin_amdgcn_permlane32_swap(h, h, false, false);
  nmc_pair2 r;
  r.lo = __hiloint2double((int)b[0], (int)a[0]);
  r.hi = __hiloint2double((int)b[1], (int)a[1]);
  return r;
}

// ---------------------------------------------------------------------------
// log-likelihood of one group over one row range, chain-on-lane: n rows from p
// (wave-uniform address: scalar loads from global memory, broadcast ds_reads from
// LDS), R rows (~BLK doubles) per block, four accumulator sets to break the
// dependence chain.
// ---------------------------------------------------------------------------
// rows per block of the global-memory / staged row loops: >= 4 rows of narrow rows (the
// scalar-load loop runs ahead in the scalar cache), 4 rows of 5-8 fields (four independent
// per-row chains -- e.g. logistic's exp / log1p -- in flight per lane), fewer for wider rows
// (registers)
__host__ __device__ constexpr int nmc_row_block(int nf) {
  return nf <= 4 ? 16 / nf : (32 / nf >= 4 ? 4 : (32 / nf > 0 ? 32 / nf : 1));
}
template <class Fam>
__device__ __forceinline__ void nmc_ll_rows(const Fam& fam, const typename Fam::Reg& reg,
                                            const double* __restrict__ p, int n,
                                            double (&acc)[Fam::NACC]) {
  constexpr int NF = Fam::NFIELDS;
  constexpr int R = nmc_row_block(NF);
  double a[4][Fam::NACC];
#pragma unroll
  for (int s = 0; s < 4; ++s)
#pragma unroll
    for (int k = 0; k < Fam::NACC; ++k) a[s][k] = 0.0;
  const int nb = n / R;
  for (int b = 0; b < nb; ++b) {
    double cur[R * NF];
#pragma unroll
    for (int j = 0; j < R * NF; ++j) cur[j] = p[(size_t)b * (R * NF) + j];
    fam.template accumN<R>(reg, cur, a);
  }
  for (int r = nb * R; r < n; ++r) fam.accum(reg, p + (size_t)r * NF, a[0]);
#pragma unroll
  for (int k = 0; k < Fam::NACC; ++k) acc[k] = (a[0][k] + a[1][k]) + (a[2][k] + a[3][k]);
}

// The regression row loop (FamLinreg<2>: rows {x, y}, e = fma(x, b1, b0 - y),
// acc[i & 3] = fma(e, e, acc[i & 3]) for row i of each 8-row block) written by hand:
// two fixed register sets v[104:135] / v[136:167] (below 168, so the step kernel can run
// three waves per SIMD), block b+1's eight broadcast
// ds_read_b128 in flight while block b is consumed (counted lgkmcnt(8)).  The compiler
// does not keep this prefetch (it sinks the reads below the arithmetic and copies the
// register sets); measured at the LDS-broadcast floor, ~5 cycles per row per CU
// (tools/llbench4.hip).  Same operations in the same order as FamLinreg::accumN, so
// the sums are bit-identical to the C++ loop.  nb: even number of 8-row blocks >= 2.
#define NMC_L8(b, off)                                                     \
  "ds_read_b128 v[" #b "+0:" #b "+3], %[addr] offset:" #off "+0\n"         \
  "ds_read_b128 v[" #b "+4:" #b "+7], %[addr] offset:" #off "+16\n"        \
  "ds_read_b128 v[" #b "+8:" #b "+11], %[addr] offset:" #off "+32\n"       \
  "ds_read_b128 v[" #b "+12:" #b "+15], %[addr] offset:" #off "+48\n"      \
  "ds_read_b128 v[" #b "+16:" #b "+19], %[addr] offset:" #off "+64\n"      \
  "ds_read_b128 v[" #b "+20:" #b "+23], %[addr] offset:" #off "+80\n"      \
  "ds_read_b128 v[" #b "+24:" #b "+27], %[addr] offset:" #off "+96\n"      \
  "ds_read_b128 v[" #b "+28:" #b "+31], %[addr] offset:" #off "+112\n"
#define NMC_E(b, k)                                                                  \
  "v_fma_f64 v[" #b "+" #k ":" #b "+" #k "+1], v[" #b "+" #k ":" #b "+" #k "+1], %[b1], v[" #b \
  "+" #k "+2:" #b "+" #k "+3]\n"
#define NMC_D(b, k)                                                                  \
  "v_add_f64 v[" #b "+" #k "+2:" #b "+" #k "+3], %[b0], -v[" #b "+" #k "+2:" #b "+" #k "+3]\n"
#define NMC_S(b, k, a) \
  "v_fma_f64 %[" #a "], v[" #b "+" #k ":" #b "+" #k "+1], v[" #b "+" #k ":" #b "+" #k "+1], %[" #a "]\n"
#define NMC_B8(b)                                                                       \
  NMC_D(b, 0) NMC_D(b, 4) NMC_D(b, 8) NMC_D(b, 12) NMC_D(b, 16) NMC_D(b, 20) NMC_D(b, 24)  \
  NMC_D(b, 28) NMC_E(b, 0) NMC_E(b, 4) NMC_E(b, 8) NMC_E(b, 12) NMC_E(b, 16) NMC_E(b, 20)  \
  NMC_E(b, 24) NMC_E(b, 28) NMC_S(b, 0, a0) NMC_S(b, 4, a1) NMC_S(b, 8, a2)               \
  NMC_S(b, 12, a3) NMC_S(b, 16, a0) NMC_S(b, 20, a1) NMC_S(b, 24, a2) NMC_S(b, 28, a3)
typedef __attribute__((address_space(3))) const double* nmc_lds_cptr;
__device__ __forceinline__ void nmc_rows_lds_linreg2(const double* p, int nb, double b0,
                                                     double b1, double& a0, double& a1,
                                                     double& a2, double& a3) {
  unsigned addr = (unsigned)(uintptr_t)(nmc_lds_cptr)p;
  int cnt = nb;
  asm volatile(
      NMC_L8(104, 0)
      "L_nmc_rows_%=:\n"
      NMC_L8(136, 128)
      "s_waitcnt lgkmcnt(8)\n"
      NMC_B8(104)
      "v_add_u32 %[addr], 0x100, %[addr]\n"
      "s_sub_u32 %[cnt], %[cnt], 2\n"
      "s_cmp_gt_i32 %[cnt], 0\n"
      "s_cbranch_scc0 L_nmc_last_%=\n"
      NMC_L8(104, 0)
      "s_waitcnt lgkmcnt(8)\n"
      NMC_B8(136)
      "s_branch L_nmc_rows_%=\n"
      "L_nmc_last_%=:\n"
      "s_waitcnt lgkmcnt(0)\n"
      NMC_B8(136)
      : [addr] "+v"(addr), [cnt] "+s"(cnt), [a0] "+v"(a0), [a1] "+v"(a1), [a2] "+v"(a2),
        [a3] "+v"(a3)
      : [b0] "v"(b0), [b1] "v"(b1)
      : "v104", "v105", "v106", "v107", "v108", "v109", "v110", "v111", "v112", "v113", "v114",
        "v115", "v116", "v117", "v118", "v119", "v120", "v121", "v122", "v123", "v124", "v125",
        "v126", "v127", "v128", "v129", "v130", "v131", "v132", "v133", "v134", "v135", "v136",
        "v137", "v138", "v139", "v140", "v141", "v142", "v143", "v144", "v145", "v146", "v147",
        "v148", "v149", "v150", "v151", "v152", "v153", "v154", "v155", "v156", "v157", "v158",
        "v159", "v160", "v161", "v162", "v163", "v164", "v165", "v166", "v167", "scc", "memory");
}

// The paired-chain form of the same loop (NMC_ROWS_PAIRED): lanes 0-31 read row 2m and
// lanes 32-63 row 2m+1 of every row pair m, and each lane evaluates its row for TWO
// chains -- its own and its partner lane's (lane ^ 32) -- so one ds_read_b128 feeds 128
// (chain, row) terms instead of 64: half the LDS instructions for the same fp64 work.
// An 8-row block is four reads (rows v[b:b+15], residual temporaries v[t:t+7]); row pair
// m feeds the own chain's u0/u1 and the partner's w0/w1 (m even / odd).  In half h those
// are the full loop's a[h] / a[2 + h] of the respective chain, with the same rows in the
// same order, and nmc_ll_rows_lds<Fam, true> reassembles them (one lane swap), so the
// sums are bit-identical to the broadcast loop.  p: this half's first row (tile start +
// h rows); nb: even number of 8-row blocks >= 2.
#define NMC_P4(b, off)                                                     \
  "ds_read_b128 v[" #b "+0:" #b "+3], %[addr] offset:" #off "+0\n"         \
  "ds_read_b128 v[" #b "+4:" #b "+7], %[addr] offset:" #off "+32\n"        \
  "ds_read_b128 v[" #b "+8:" #b "+11], %[addr] offset:" #off "+64\n"       \
  "ds_read_b128 v[" #b "+12:" #b "+15], %[addr] offset:" #off "+96\n"
// partner residual seed c0 - y into t, own b0 - y in place of y, then both fmas with x
#define NMC_PDX(b, t, k4, k2) \
  "v_add_f64 v[" #t "+" #k2 ":" #t "+" #k2 "+1], %[c0], -v[" #b "+" #k4 "+2:" #b "+" #k4 "+3]\n"
#define NMC_PDO(b, k4) \
  "v_add_f64 v[" #b "+" #k4 "+2:" #b "+" #k4 "+3], %[b0], -v[" #b "+" #k4 "+2:" #b "+" #k4 "+3]\n"
#define NMC_PEO(b, k4)                                                                      \
  "v_fma_f64 v[" #b "+" #k4 "+2:" #b "+" #k4 "+3], v[" #b "+" #k4 ":" #b "+" #k4 "+1], %[b1], v[" \
  #b "+" #k4 "+2:" #b "+" #k4 "+3]\n"
#define NMC_PEX(b, t, k4, k2)                                                               \
  "v_fma_f64 v[" #t "+" #k2 ":" #t "+" #k2 "+1], v[" #b "+" #k4 ":" #b "+" #k4 "+1], %[c1], v[" \
  #t "+" #k2 ":" #t "+" #k2 "+1]\n"
#define NMC_PSO(b, k4, a) \
  "v_fma_f64 %[" #a "], v[" #b "+" #k4 "+2:" #b "+" #k4 "+3], v[" #b "+" #k4 "+2:" #b "+" #k4 "+3], %[" #a "]\n"
#define NMC_PSX(t, k2, a) \
  "v_fma_f64 %[" #a "], v[" #t "+" #k2 ":" #t "+" #k2 "+1], v[" #t "+" #k2 ":" #t "+" #k2 "+1], %[" #a "]\n"
#define NMC_PB(b, t)                                                                        \
  NMC_PDX(b, t, 0, 0) NMC_PDX(b, t, 4, 2) NMC_PDX(b, t, 8, 4) NMC_PDX(b, t, 12, 6)           \
  NMC_PDO(b, 0) NMC_PDO(b, 4) NMC_PDO(b, 8) NMC_PDO(b, 12)                                   \
  NMC_PEO(b, 0) NMC_PEO(b, 4) NMC_PEO(b, 8) NMC_PEO(b, 12)                                   \
  NMC_PEX(b, t, 0, 0) NMC_PEX(b, t, 4, 2) NMC_PEX(b, t, 8, 4) NMC_PEX(b, t, 12, 6)           \
  NMC_PSO(b, 0, u0) NMC_PSX(t, 0, w0) NMC_PSO(b, 4, u1) NMC_PSX(t, 2, w1)                   \
  NMC_PSO(b, 8, u0) NMC_PSX(t, 4, w0) NMC_PSO(b, 12, u1) NMC_PSX(t, 6, w1)
__device__ __forceinline__ void nmc_rows_lds_linreg2_paired(const double* p, int nb, double b0,
                                                            double b1, double c0, double c1,
                                                            double& u0, double& u1, double& w0,
                                                            double& w1) {
  unsigned addr = (unsigned)(uintptr_t)(nmc_lds_cptr)p;
  int cnt = nb;
  asm volatile(
      NMC_P4(120, 0)
      "L_nmc_prows_%=:\n"
      NMC_P4(144, 128)
      "s_waitcnt lgkmcnt(4)\n"
      NMC_PB(120, 136)
      "v_add_u32 %[addr], 0x100, %[addr]\n"
      "s_sub_u32 %[cnt], %[cnt], 2\n"
      "s_cmp_gt_i32 %[cnt], 0\n"
      "s_cbranch_scc0 L_nmc_plast_%=\n"
      NMC_P4(120, 0)
      "s_waitcnt lgkmcnt(4)\n"
      NMC_PB(144, 160)
      "s_branch L_nmc_prows_%=\n"
      "L_nmc_plast_%=:\n"
      "s_waitcnt lgkmcnt(0)\n"
      NMC_PB(144, 160)
      : [addr] "+v"(addr), [cnt] "+s"(cnt), [u0] "+v"(u0), [u1] "+v"(u1), [w0] "+v"(w0),
        [w1] "+v"(w1)
      : [b0] "v"(b0), [b1] "v"(b1), [c0] "v"(c0), [c1] "v"(c1)
      : "v120", "v121", "v122", "v123", "v124", "v125", "v126", "v127", "v128", "v129", "v130",
        "v131", "v132", "v133", "v134", "v135", "v136", "v137", "v138", "v139", "v140", "v141",
        "v142", "v143", "v144", "v145", "v146", "v147", "v148", "v149", "v150", "v151", "v152",
        "v153", "v154", "v155", "v156", "v157", "v158", "v159", "v160", "v161", "v162", "v163",
        "v164", "v165", "v166", "v167", "scc", "memory");
}

// The quad-chain form (Dev.quad, the default for {x, y} rows): a wave's four quarters (rows
// of 16 lanes) read rows 4m+q of every 16-row block, q = the lane's quarter, and every lane
// evaluates its row for FOUR chains -- those of lanes (lane & 15) + 16j, j = 0..3, the same
// position in each quarter -- so one ds_read_b128 feeds 256 (chain, row) terms: a quarter
// of the broadcast loop's LDS reads and half the paired loop's, and 48 fp64 instructions
// per four reads, which keeps one wave's issue off the LDS latency.  Chain slot j's
// accumulator a[j] in quarter q sums rows = q (mod 4) in row order: exactly the broadcast
// loop's a[q] of chain (lane & 15) + 16j (its 8-row blocks put row i into a[i & 3]), so a
// 4 x 4 transpose across the quarters (nmc_transpose4) hands every lane its own chain's
// a[0..3] and the sums are bit-identical to the broadcast and paired loops.
// Registers: row sets v[120:135] / v[136:151] (block b+1's four reads in flight while block
// b is consumed), residual temporaries v[152:167] -- the paired loop's range, so the kernel's
// register budget is unchanged.  p: this quarter's first row (tile start + q rows);
// nb: 16-row blocks >= 1, any count.
#define NMC_Q4(b, off)                                                     \
  "ds_read_b128 v[" #b "+0:" #b "+3], %[addr] offset:" #off "+0\n"         \
  "ds_read_b128 v[" #b "+4:" #b "+7], %[addr] offset:" #off "+64\n"        \
  "ds_read_b128 v[" #b "+8:" #b "+11], %[addr] offset:" #off "+128\n"      \
  "ds_read_b128 v[" #b "+12:" #b "+15], %[addr] offset:" #off "+192\n"
// chain slot j of a row (x at v[xr], y at v[yr]) into temporary t: t = c_j - y, then
// t = fma(x, d_j, t), then a_j = fma(t, t, a_j) -- FamLinreg::accum's operations
#define NMC_QD(t, yr, j) "v_add_f64 v[" #t ":" #t "+1], %[c" #j "], -v[" #yr ":" #yr "+1]\n"
#define NMC_QE(t, xr, j) \
  "v_fma_f64 v[" #t ":" #t "+1], v[" #xr ":" #xr "+1], %[d" #j "], v[" #t ":" #t "+1]\n"
#define NMC_QS(t, j) "v_fma_f64 %[a" #j "], v[" #t ":" #t "+1], v[" #t ":" #t "+1], %[a" #j "]\n"
// two rows (x0/y0, then x1/y1) for the four chain slots: 8 adds, 8 fmas, 8 accumulations
// (slot j gets row x0 before row x1, the row order)
#define NMC_QH(x0, y0, x1, y1)                                                               \
  NMC_QD(152, y0, 0) NMC_QD(154, y0, 1) NMC_QD(156, y0, 2) NMC_QD(158, y0, 3)                \
  NMC_QD(160, y1, 0) NMC_QD(162, y1, 1) NMC_QD(164, y1, 2) NMC_QD(166, y1, 3)                \
  NMC_QE(152, x0, 0) NMC_QE(154, x0, 1) NMC_QE(156, x0, 2) NMC_QE(158, x0, 3)                \
  NMC_QE(160, x1, 0) NMC_QE(162, x1, 1) NMC_QE(164, x1, 2) NMC_QE(166, x1, 3)                \
  NMC_QS(152, 0) NMC_QS(154, 1) NMC_QS(156, 2) NMC_QS(158, 3)                                \
  NMC_QS(160, 0) NMC_QS(162, 1) NMC_QS(164, 2) NMC_QS(166, 3)
// a 16-row block from register set A (v[120:135]) / B (v[136:151]): its rows 4m+q, m = 0..3
#define NMC_QBA NMC_QH(120, 122, 124, 126) NMC_QH(128, 130, 132, 134)
#define NMC_QBB NMC_QH(136, 138, 140, 142) NMC_QH(144, 146, 148, 150)
// the loop over nb 16-row blocks (shared by the two entries below)
#define NMC_QLOOP                                  \
      NMC_Q4(120, 0)                               \
      "L_nmc_q_%=:\n"                              \
      "s_sub_u32 %[cnt], %[cnt], 1\n"              \
      "s_cmp_gt_i32 %[cnt], 0\n"                   \
      "s_cbranch_scc0 L_nmc_qla_%=\n"              \
      NMC_Q4(136, 256)                             \
      "s_waitcnt lgkmcnt(4)\n"                     \
      NMC_QBA                                      \
      "v_add_u32 %[addr], 0x200, %[addr]\n"        \
      "s_sub_u32 %[cnt], %[cnt], 1\n"              \
      "s_cmp_gt_i32 %[cnt], 0\n"                   \
      "s_cbranch_scc0 L_nmc_qlb_%=\n"              \
      NMC_Q4(120, 0)                               \
      "s_waitcnt lgkmcnt(4)\n"                     \
      NMC_QBB                                      \
      "s_branch L_nmc_q_%=\n"                      \
      "L_nmc_qla_%=:\n"                            \
      "s_waitcnt lgkmcnt(0)\n"                     \
      NMC_QBA                                      \
      "s_branch L_nmc_qend_%=\n"                   \
      "L_nmc_qlb_%=:\n"                            \
      "s_waitcnt lgkmcnt(0)\n"                     \
      NMC_QBB                                      \
      "L_nmc_qend_%=:\n"
#define NMC_QCLOBBERS                                                                            \
  "v120", "v121", "v122", "v123", "v124", "v125", "v126", "v127", "v128", "v129", "v130",       \
      "v131", "v132", "v133", "v134", "v135", "v136", "v137", "v138", "v139", "v140", "v141",   \
      "v142", "v143", "v144", "v145", "v146", "v147", "v148", "v149", "v150", "v151", "v152",   \
      "v153", "v154", "v155", "v156", "v157", "v158", "v159", "v160", "v161", "v162", "v163",   \
      "v164", "v165", "v166", "v167", "scc", "memory"
__device__ __forceinline__ void nmc_rows_lds_linreg2_quad(const double* p, int nb,
                                                          const double (&c)[4],
                                                          const double (&dd)[4],
                                                          double (&a)[4]) {
  unsigned addr = (unsigned)(uintptr_t)(nmc_lds_cptr)p;
  int cnt = nb;
  asm volatile(
      NMC_QLOOP
      : [addr] "+v"(addr), [cnt] "+s"(cnt), [a0] "+v"(a[0]), [a1] "+v"(a[1]), [a2] "+v"(a[2]),
        [a3] "+v"(a[3])
      : [c0] "v"(c[0]), [c1] "v"(c[1]), [c2] "v"(c[2]), [c3] "v"(c[3]), [d0] "v"(dd[0]),
        [d1] "v"(dd[1]), [d2] "v"(dd[2]), [d3] "v"(dd[3])
      : NMC_QCLOBBERS);
}
// The same loop for a step's first tile in the step kernel's restart without gathers (step.h):
// the four chains' intercepts and slopes are read here, from the parameters' LDS columns -- cp /
// dp point at this lane's quarter position (lane & 15) of the intercept / slope column, whose
// elements + 16j are chain slot j's -- and returned in c / dd for the step's later tiles.  The
// eight reads go out back to back with the first block's row reads -- the rows do not depend on
// the parameters -- and the loop's first wait covers both: one LDS round trip, where parameters
// handed in as operands are waited for before the block.  ic == 0 (wave-uniform): the model has
// no intercept, c = 0.0.
__device__ __forceinline__ void nmc_rows_lds_linreg2_quad_first(const double* p, int nb, int ic,
                                                                const double* cp,
                                                                const double* dp, double (&c)[4],
                                                                double (&dd)[4], double (&a)[4]) {
  unsigned addr = (unsigned)(uintptr_t)(nmc_lds_cptr)p;
  const unsigned ca = (unsigned)(uintptr_t)(nmc_lds_cptr)cp;
  const unsigned da = (unsigned)(uintptr_t)(nmc_lds_cptr)dp;
  int cnt = nb;
  asm volatile(
      "v_cmp_eq_u32_e32 vcc, 0, %[ic]\n"
      "s_cbranch_vccnz L_nmc_qnc_%=\n"
      "ds_read_b64 %[c0], %[ca]\n"
      "ds_read_b64 %[c1], %[ca] offset:128\n"
      "ds_read_b64 %[c2], %[ca] offset:256\n"
      "ds_read_b64 %[c3], %[ca] offset:384\n"
      "s_branch L_nmc_qd_%=\n"
      "L_nmc_qnc_%=:\n"
      "v_mov_b64 %[c0], 0\n"
      "v_mov_b64 %[c1], 0\n"
      "v_mov_b64 %[c2], 0\n"
      "v_mov_b64 %[c3], 0\n"
      "L_nmc_qd_%=:\n"
      "ds_read_b64 %[d0], %[da]\n"
      "ds_read_b64 %[d1], %[da] offset:128\n"
      "ds_read_b64 %[d2], %[da] offset:256\n"
      "ds_read_b64 %[d3], %[da] offset:384\n"
      NMC_QLOOP
      : [addr] "+v"(addr), [cnt] "+s"(cnt), [a0] "+v"(a[0]), [a1] "+v"(a[1]), [a2] "+v"(a[2]),
        [a3] "+v"(a[3]), [c0] "=&v"(c[0]), [c1] "=&v"(c[1]), [c2] "=&v"(c[2]), [c3] "=&v"(c[3]),
        [d0] "=&v"(dd[0]), [d1] "=&v"(dd[1]), [d2] "=&v"(dd[2]), [d3] "=&v"(dd[3])
      : [ca] "v"(ca), [da] "v"(da), [ic] "v"(ic)
      : "vcc", NMC_QCLOBBERS);
}

// v of the four lanes (lane & 15) + 16j, j = 0..3 (the lane's position in each quarter):
// v_permlane16_swap exchanges odd rows of its first operand with even rows of its second
// (rows of 16 lanes), v_permlane32_swap the upper half of the first with the lower half of
// the second (gfx950); swapping a value with itself yields its row pair / half pair
__device__ __forceinline__ void nmc_quarters(double v, double (&o)[4]) {
  const unsigned l = (unsigned)__double2loint(v), h = (unsigned)__double2hiint(v);
  const auto a = __builtin_amdgcn_permlane16_swap(l, l, false, false);   // [0]: row 2k, [1]: 2k+1
  const auto b = __builtin_amdgcn_permlane16_swap(h, h, false, false);
  const nmc_pair2 ev = nmc_halves(__hiloint2double((int)b[0], (int)a[0]));   // rows 0, 2
  const nmc_pair2 od = nmc_halves(__hiloint2double((int)b[1], (int)a[1]));   // rows 1, 3
  o[0] = ev.lo;
  o[1] = od.lo;
  o[2] = ev.hi;
  o[3] = od.hi;
}
template <bool R16>
__device__ __forceinline__ void nmc_swap_rows(double& x, double& y) {
  const unsigned xl = (unsigned)__double2loint(x), xh = (unsigned)__double2hiint(x);
  const unsigned yl = (unsigned)__double2loint(y), yh = (unsigned)__double2hiint(y);
  const auto l = R16 ? __builtin_amdgcn_permlane16_swap(xl, yl, false, false)
                     : __builtin_amdgcn_permlane32_swap(xl, yl, false, false);
  const auto h = R16 ? __builtin_amdgcn_permlane16_swap(xh, yh, false, false)
                     : __builtin_amdgcn_permlane32_swap(xh, yh, false, false);
  x = __hiloint2double((int)h[0], (int)l[0]);
  y = __hiloint2double((int)h[1], (int)l[1]);
}
// a[j] of quarter q -> a[q] of quarter j (4 x 4 transpose over the quarters): half swaps of
// (a0, a2), (a1, a3), then row swaps of (a0, a1), (a2, a3)
__device__ __forceinline__ void nmc_transpose4(double (&a)[4]) {
  nmc_swap_rows<false>(a[0], a[2]);
  nmc_swap_rows<false>(a[1], a[3]);
  nmc_swap_rows<true>(a[0], a[1]);
  nmc_swap_rows<true>(a[2], a[3]);
}

// The same over rows staged in LDS: blocks of R rows read with wave-uniform
// (broadcast) ds_reads; block b+1 is requested before block b is consumed (LDS
// returns in order, so the wait covers only block b).
#ifndef NMC_LDS_ROW_DOUBLES
#define NMC_LDS_ROW_DOUBLES 16   // doubles per software-pipelined LDS block (8 regression rows)
#endif
// PAIRED (NMC_ROWS_PAIRED): the R-row blocks are split by row parity between the two
// lane halves and every lane evaluates its rows for its own chain (reg) and its partner
// lane's (preg); one lane swap hands each chain the other parity's accumulators, then
// the tail rows are added in order per chain -- bit-identical to PAIRED == false.
template <class Fam>
constexpr bool nmc_paired_rows_ok() {
  constexpr int NF = Fam::NFIELDS;
  constexpr int BD = NF <= 2 ? 16 : 8;
  constexpr int R = (BD / NF) > 0 ? (BD / NF) : 1;
  return R % 2 == 0;
}
// SAME (half layout): lanes l and l + 32 hold the same chain -- each evaluates its row
// parity for that chain only, and the partner's own accumulators are this chain's other
// parity (no partner evaluation).
template <class Fam, bool PAIRED = false, bool SAME = false>
__device__ __forceinline__ void nmc_ll_rows_lds(const Fam& fam, const typename Fam::Reg& reg,
                                                const double* __restrict__ p, int n,
                                                double (&acc)[Fam::NACC],
                                                const typename Fam::Reg* preg = nullptr) {
  constexpr int NF = Fam::NFIELDS;
  // 8-row blocks for 2-field rows (measured: -17 % per iteration for regression),
  // 8 doubles otherwise (register pressure of the wider families)
  constexpr int BD = NF <= 2 ? NMC_LDS_ROW_DOUBLES : 8;
  constexpr int R = (BD / NF) > 0 ? (BD / NF) : 1;
  double a[4][Fam::NACC];
#pragma unroll
  for (int s = 0; s < 4; ++s)
#pragma unroll
    for (int k = 0; k < Fam::NACC; ++k) a[s][k] = 0.0;
  // two register sets A/B over an even number of R-row blocks: block b+1's reads are
  // issued before block b is consumed, pinned by scheduling barriers (left alone the
  // compiler sinks the reads below the arithmetic and every block pays the full LDS
  // latency).  No condition inside the loop (a conditional load costs register
  // copies): the last prefetch reads one block past the range, which the LDS row
  // area is padded for (nmc_lds) and which is never consumed.
  const int nb2 = (n / R) & ~1;
  if constexpr (PAIRED) {
    static_assert(R % 2 == 0, "the paired split needs row pairs in every block");
    constexpr int RH = R / 2;
    const int h = (threadIdx.x >> 5) & 1;
    const double* ph = p + (size_t)h * NF;   // row 2m + h of pair m
    double u[2][Fam::NACC], v[2][Fam::NACC];   // own chain / partner chain, m even / odd
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int k = 0; k < Fam::NACC; ++k) u[s][k] = v[s][k] = 0.0;
    if constexpr (Fam::ASM_ROWS && !SAME) {
      static_assert(R == 8 && NF == 2, "the asm row loop is the 8-row {x, y} block");
      if (nb2 > 0)
        nmc_rows_lds_linreg2_paired(ph, nb2, reg.b0, reg.b[0], preg->b0, preg->b[0], u[0][0],
                                    u[1][0], v[0][0], v[1][0]);
    } else if (nb2 > 0) {
      double A[RH * NF], B[RH * NF];
#pragma unroll
      for (int m = 0; m < RH; ++m)
#pragma unroll
        for (int f = 0; f < NF; ++f) A[m * NF + f] = ph[(size_t)2 * m * NF + f];
      for (int b = 0; b < nb2; b += 2) {
        const double* q = ph + (size_t)b * (R * NF);
#pragma unroll
        for (int m = 0; m < RH; ++m)
#pragma unroll
          for (int f = 0; f < NF; ++f) B[m * NF + f] = q[R * NF + (size_t)2 * m * NF + f];
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int m = 0; m < RH; ++m) {
          fam.accum(reg, A + m * NF, u[m & 1]);
          if constexpr (!SAME) fam.accum(*preg, A + m * NF, v[m & 1]);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int m = 0; m < RH; ++m)
#pragma unroll
          for (int f = 0; f < NF; ++f) A[m * NF + f] = q[2 * R * NF + (size_t)2 * m * NF + f];
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int m = 0; m < RH; ++m) {
          fam.accum(reg, B + m * NF, u[m & 1]);
          if constexpr (!SAME) fam.accum(*preg, B + m * NF, v[m & 1]);
        }
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    // own chain: a[2k + h] = u[k]; a[2k + 1 - h] = the partner lane's v[k] (the partner's
    // partner chain is this lane's chain)
#pragma unroll
    for (int k = 0; k < Fam::NACC; ++k) {
      // (SAME: the other parity of this chain is the partner lane's own accumulators)
      const nmc_pair2 e = nmc_halves(SAME ? u[0][k] : v[0][k]);
      const nmc_pair2 o = nmc_halves(SAME ? u[1][k] : v[1][k]);
      const double p0 = h ? e.lo : e.hi, p1 = h ? o.lo : o.hi;
      a[0][k] = h ? p0 : u[0][k];
      a[1][k] = h ? u[0][k] : p0;
      a[2][k] = h ? p1 : u[1][k];
      a[3][k] = h ? u[1][k] : p1;
    }
  } else if constexpr (Fam::ASM_ROWS) {
    static_assert(R == 8 && NF == 2, "the asm row loop is the 8-row {x, y} block");
    if (nb2 > 0) nmc_rows_lds_linreg2(p, nb2, reg.b0, reg.b[0], a[0][0], a[1][0], a[2][0], a[3][0]);
  } else if (nb2 > 0) {
    double A[R * NF], B[R * NF];
#pragma unroll
    for (int j = 0; j < R * NF; ++j) A[j] = p[j];
    for (int b = 0; b < nb2; b += 2) {
      const double* q = p + (size_t)b * (R * NF);
#pragma unroll
      for (int j = 0; j < R * NF; ++j) B[j] = q[R * NF + j];
      __builtin_amdgcn_sched_barrier(0);
      fam.template accumN<R>(reg, A, a);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int j = 0; j < R * NF; ++j) A[j] = q[2 * R * NF + j];
      __builtin_amdgcn_sched_barrier(0);
      fam.template accumN<R>(reg, B, a);
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  // the remaining (< 2R) rows into a[0], in order; their reads are issued in batches of
  // TB rows (one LDS round trip per batch, not per row)
  constexpr int TB = (16 / NF) > 0 ? (16 / NF) : 1;
  for (int r0 = nb2 * R; r0 < n; r0 += TB) {
    double tv[TB * NF];
#pragma unroll
    for (int i = 0; i < TB; ++i) {
      const int rr = r0 + i < n ? r0 + i : n - 1;
#pragma unroll
      for (int f = 0; f < NF; ++f) tv[i * NF + f] = p[(size_t)rr * NF + f];
    }
#pragma unroll
    for (int i = 0; i < TB; ++i)
      if (r0 + i < n) fam.accum(reg, tv + i * NF, a[0]);
  }
#pragma unroll
  for (int k = 0; k < Fam::NACC; ++k) acc[k] = (a[0][k] + a[1][k]) + (a[2][k] + a[3][k]);
}

// The quad-chain row loop (nmc_rows_lds_linreg2_quad) over one tile of n rows at p: c / dd
// hold the intercept and slope of the four chains of the lane's quarter position
// (nmc_quarters).  The 16-row blocks cover the broadcast loop's even number of 8-row blocks;
// after the transpose the lane's own chain's four accumulators take the remaining rows in
// order into a[0], as in nmc_ll_rows_lds -- every sum bit-identical to it.
// FIRST (step.h, the restart without gathers): the step's first tile, whose row loop reads c /
// dd from the LDS columns at cp / dp (nmc_rows_lds_linreg2_quad_first) and returns them for the
// later tiles; a first tile of fewer than 16 rows is the group's last tile and needs none.  The
// lane's own chain (reg, for the rows beyond the 16-row blocks) is prepared here from thp, read
// by the caller and first used behind the row loop: no LDS round trip of its own either.
template <class Fam, bool FIRST = false, class RG, class QV>
__device__ __forceinline__ void nmc_ll_rows_lds_quad(const Fam& fam, RG& reg,
                                                     const double* __restrict__ p, int n,
                                                     double (&acc)[Fam::NACC], QV (&c)[4],
                                                     QV (&dd)[4], const double* thp = nullptr,
                                                     int ic = 0, const double* cp = nullptr,
                                                     const double* dp = nullptr) {
  static_assert(Fam::ASM_ROWS && Fam::NFIELDS == 2 && Fam::NACC == 1, "{x, y} rows only");
  constexpr int NF = Fam::NFIELDS;
  const int q = (threadIdx.x >> 4) & 3;
  const int nb16 = (n / 8) >> 1;      // = the broadcast loop's (n / 8) & ~1 8-row blocks / 2
  double a[4] = {0.0, 0.0, 0.0, 0.0};
  if constexpr (FIRST) {
    if (nb16 > 0) {
      __builtin_amdgcn_sched_barrier(0);   // (thp's reads are in flight, not waited for)
      nmc_rows_lds_linreg2_quad_first(p + (size_t)q * NF, nb16, ic, cp, dp, c, dd, a);
      nmc_transpose4(a);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) c[j] = dd[j] = 0.0;
    }
    reg = fam.prepare(thp);
  } else if (nb16 > 0) {
    nmc_rows_lds_linreg2_quad(p + (size_t)q * NF, nb16, c, dd, a);
    nmc_transpose4(a);
  }
  double at[1] = {a[0]};
  constexpr int TB = 8;
  for (int r0 = nb16 * 16; r0 < n; r0 += TB) {
    double tv[TB * NF];
#pragma unroll
    for (int i = 0; i < TB; ++i) {
      const int rr = r0 + i < n ? r0 + i : n - 1;
#pragma unroll
      for (int f = 0; f < NF; ++f) tv[i * NF + f] = p[(size_t)rr * NF + f];
    }
#pragma unroll
    for (int i = 0; i < TB; ++i)
      if (r0 + i < n) fam.accum(reg, tv + i * NF, at);
  }
  acc[0] = (at[0] + a[1]) + (a[2] + a[3]);
}

// ---------------------------------------------------------------------------
// Rows that do not fit LDS (groups over 64 KiB): each wave stages its tile through two
// private LDS buffers of NMC_SR(NF) rows, copied by LDS-DMA (global_load_lds_dwordx4, no
// registers) one chunk ahead of the chunk it computes, so the row fetch -- an L2 / MALL
// round trip per row for the scalar-load loop it replaces -- hides behind the arithmetic.
// Same R-row blocks, accumulators and order as nmc_ll_rows (bit-identical sums).
// ---------------------------------------------------------------------------
// rows per chunk: as many whole row blocks as one 1 KiB DMA instruction carries beside
// 16 B of alignment slack (n_fields <= 64: at least one row)
__host__ __device__ constexpr int nmc_stage_rows(int nf) {
  return (1008 / (nf * 8)) / nmc_row_block(nf) > 0
             ? nmc_row_block(nf) * ((1008 / (nf * 8)) / nmc_row_block(nf))
             : nmc_row_block(nf);
}
// one buffer: the chunk's doubles plus 16 B of alignment slack, in whole 1 KiB DMAs
__host__ __device__ constexpr int nmc_stage_buf(int nf) {
  return ((nmc_stage_rows(nf) * nf + 2) * 8 + 1023) / 1024 * 128;
}
__host__ __device__ constexpr int nmc_stage_doubles(int nf, int W) { return W * 2 * nmc_stage_buf(nf); }

template <class Fam>
__device__ __forceinline__ void nmc_ll_rows_staged(const Fam& fam, const typename Fam::Reg& reg,
                                                   const double* __restrict__ p, int n,
                                                   const double* lim, double* stage,
                                                   double (&acc)[Fam::NACC]) {
  constexpr int NF = Fam::NFIELDS;
  constexpr int R = nmc_row_block(NF);
  constexpr int SR = nmc_stage_rows(NF);
  constexpr int BUF = nmc_stage_buf(NF);        // doubles per buffer
  constexpr int K = BUF / 128;                  // 1 KiB DMA instructions per chunk
  static_assert(K >= 1 && K <= 15, "vmcnt immediate");
  const int lane = threadIdx.x & 63;
  double a[4][Fam::NACC];
#pragma unroll
  for (int s = 0; s < 4; ++s)
#pragma unroll
    for (int k = 0; k < Fam::NACC; ++k) a[s][k] = 0.0;
  // the aligned 16 B that hold the group's last double: when the group ends on an odd double
  // offset (odd NF x odd row count) they reach 8 B into the next group, or into the slack
  // that nmc_create allocates behind the table
  const uintptr_t last = ((uintptr_t)lim - 8) & ~(uintptr_t)15;
  auto issue = [&](int c, double* buf) -> int {   // chunk c -> buf; returns its offset (doubles)
    const uintptr_t src = (uintptr_t)(p + (size_t)c * SR * NF);
    const uintptr_t a16 = src & ~(uintptr_t)15;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // the buffer's last reads are done
#pragma unroll
    for (int q = 0; q < K; ++q) {
      uintptr_t g = a16 + (uintptr_t)(q * 64 + lane) * 16;
      g = g > last ? (last > a16 ? last : a16) : g;      // never past the group's rows
      __builtin_amdgcn_global_load_lds((nmc_glb_ptr)g, (nmc_lds_ptr)(buf + q * 128), 16, 0, 0);
    }
    return (int)((src - a16) / 8);
  };
  const int nch = (n + SR - 1) / SR;
  int off_cur = nch > 0 ? issue(0, stage) : 0;
  for (int c = 0; c < nch; ++c) {
    double* cur = stage + (c & 1) * BUF;
    int off_next = 0;
    if (c + 1 < nch) {
      off_next = issue(c + 1, stage + ((c + 1) & 1) * BUF);
      // chunk c has landed once at most chunk c+1's K copies are outstanding (loads return
      // in order); vmcnt field [3:0], expcnt / lgkmcnt left unconstrained
      __builtin_amdgcn_s_waitcnt((K & 15) | (7 << 4) | (15 << 8));
    } else {
      __builtin_amdgcn_s_waitcnt(0 | (7 << 4) | (15 << 8));
    }
    __builtin_amdgcn_sched_barrier(0);
    const double* q = cur + off_cur;
    const int rows = n - c * SR < SR ? n - c * SR : SR;
    const int nb = rows / R;
    for (int b = 0; b < nb; ++b) {
      double v[R * NF];
#pragma unroll
      for (int j = 0; j < R * NF; ++j) v[j] = q[(size_t)b * (R * NF) + j];
      fam.template accumN<R>(reg, v, a);
    }
    for (int r = nb * R; r < rows; ++r) fam.accum(reg, q + (size_t)r * NF, a[0]);
    __builtin_amdgcn_sched_barrier(0);
    off_cur = off_next;
  }
#pragma unroll
  for (int k = 0; k < Fam::NACC; ++k) acc[k] = (a[0][k] + a[1][k]) + (a[2][k] + a[3][k]);
}

// The tile partials of one sum in a fixed order: tile k into accumulator k % 4, combined
// (a0+a1)+(a2+a3); every LDS read in flight at once (slots past the last tile hold -0.0,
// and x + (-0.0) == x).
typedef double nmc_v2d __attribute__((ext_vector_type(2)));
__device__ __forceinline__ double nmc_sum_slots(const double* pt) {
  double v[NMC_NSLOT];
#if NMC_NSLOT_N == 16
  // the 16 slots (512 B apart) as eight ds_read2st64_b64, all in flight, one wait: left to
  // itself the scheduler splits them over two LDS round trips on the decision's path
  {
    const unsigned a = (unsigned)(uintptr_t)(nmc_lds_cptr)pt;
    nmc_v2d r[8];
    asm volatile(
        "ds_read2st64_b64 %0, %8 offset1:1\n\t"
        "ds_read2st64_b64 %1, %8 offset0:2 offset1:3\n\t"
        "ds_read2st64_b64 %2, %8 offset0:4 offset1:5\n\t"
        "ds_read2st64_b64 %3, %8 offset0:6 offset1:7\n\t"
        "ds_read2st64_b64 %4, %8 offset0:8 offset1:9\n\t"
        "ds_read2st64_b64 %5, %8 offset0:10 offset1:11\n\t"
        "ds_read2st64_b64 %6, %8 offset0:12 offset1:13\n\t"
        "ds_read2st64_b64 %7, %8 offset0:14 offset1:15\n\t"
        "s_waitcnt lgkmcnt(0)"
        : "=&v"(r[0]), "=&v"(r[1]), "=&v"(r[2]), "=&v"(r[3]), "=&v"(r[4]), "=&v"(r[5]),
          "=&v"(r[6]),
          "=&v"(r[7])
        : "v"(a)
        : "memory");
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      v[2 * u] = r[u].x;
      v[2 * u + 1] = r[u].y;
    }
  }
#else
#pragma unroll
  for (int u = 0; u < NMC_NSLOT; ++u) v[u] = pt[u * 64];
#endif
  double a4[4];
#pragma unroll
  for (int u = 0; u < NMC_NSLOT; ++u) a4[u & 3] = u < 4 ? v[u] : a4[u & 3] + v[u];
  return (a4[0] + a4[1]) + (a4[2] + a4[3]);
}
