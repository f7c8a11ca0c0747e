// Kernel selection of launch_gemm: WHICH kernel family, tile, epilogue and split a GemmArgs runs on, or why it is refused. Host code
// only -- no HIP, no device query, no launch; pointers are looked at for null-ness and alignment and never dereferenced -- so that the
// one function gemm_route() is held on the CPU (tests/test_gemm_route_build.py) to the table tests/golden/gemm_routes.json.
//   launch_t (gemm.hip)            routes, fills GemmDev, switches on the family into a launcher that computes launch geometry only
//   gemm_*_ok / gemm_pair_large    ask gemm_route() about a canonical problem of their form (end of this file); no rule lives in them
// The priority order of the families is the order of the statements in gemm_route(), top to bottom.
#pragma once
#include "gemm_args.h"
#include <stdlib.h>

namespace vima {

constexpr int kGemmInvalid = 1;   // hipErrorInvalidValue (gemm.hip asserts the number)

// Knob resolution: the handle's Tuning value when set (>= 0), otherwise the process default from the environment
// (read once; never written afterwards, so it is safe to share between handles).
inline int env_int(const char* name, int dflt) {
  const char* e = getenv(name);
  return (e && e[0]) ? atoi(e) : dflt;
}
inline int env_cached(const char* name, int& cache, int dflt) {
  if (cache < 0) cache = env_int(name, dflt);
  return cache;
}
#define VIMA_KNOB(fn, env, dflt)                                                                                                    \
  inline int g_env_##fn = -1;                                                                                                        \
  inline int fn(const Tuning* t) { return (t && t->fn >= 0) ? t->fn : env_cached(env, g_env_##fn, dflt); }
VIMA_KNOB(gemm_variant, "VIMA_GEMM_VARIANT", 1)
VIMA_KNOB(gemm_tile, "VIMA_GEMM_TILE", 0)
VIMA_KNOB(gemm_raster, "VIMA_GEMM_RASTER", 0)
VIMA_KNOB(gemm_epi, "VIMA_GEMM_EPI", 1)
VIMA_KNOB(gemm_persist, "VIMA_GEMM_PERSIST", 1)
VIMA_KNOB(gemm_small, "VIMA_GEMM_SMALL", 1)
VIMA_KNOB(gemm_splitk, "VIMA_GEMM_SPLITK", 0)
VIMA_KNOB(gemm_wide, "VIMA_GEMM_WIDE", 0)
VIMA_KNOB(gemm_pp, "VIMA_GEMM_PP", 1)
VIMA_KNOB(gemm_q4, "VIMA_GEMM_Q4", 6)
VIMA_KNOB(gemm_q4_rs, "VIMA_GEMM_Q4_RS", 1)
VIMA_KNOB(gemm_resident, "VIMA_GEMM_RESIDENT", 1)
VIMA_KNOB(gemm_res_maxwg, "VIMA_GEMM_RES_MAXWG", 256)
VIMA_KNOB(gemm_res_nch, "VIMA_GEMM_RES_NCH", 0)
VIMA_KNOB(gemm_skinny, "VIMA_GEMM_SKINNY", 1)
VIMA_KNOB(gemm_flat, "VIMA_GEMM_FLAT", 1)
#undef VIMA_KNOB

// The families: the number is GemmArgs::kernel_id / 1000 (x3 turns 5 into 21 and 8 into 23; the two lab tiles report no id)
enum GemmFamily : int {
  GF_NONE = 0,        // nothing to do (M or N <= 0)
  GF_PP = 1,          // gemm_pp_kernel, 256x256 persistent ping-pong
  GF_PERSISTENT = 2,  // gemm_persistent_kernel, 256x256
  GF_WIDE = 3,        // gemm_wide_kernel, 256x384
  GF_TILE_L = 4, GF_TILE_S = 5, GF_TILE_64 = 6, GF_TILE_XS = 7,   // gemm_kernel, one tile per workgroup: 256x256, 128x128, 64x64, 32x64
  GF_SPLITK = 8,      // two passes: the route of the partial problem, then gemm_reduce_kernel
  GF_PP_F8 = 9,       // gemm_pp_kernel<.., F8>: fp8 activations and weights
  GF_RT32 = 10, GF_RT64x32 = 11, GF_RT64 = 12,   // gemm_resident_kernel
  GF_TILE_64x128 = 13, GF_TILE_128x64 = 14,      // gemm_kernel, gemm_tile 13 / 14 only
  GF_RT32_DUAL = 15, GF_RT64_DUAL = 16, GF_SKINNY = 17, GF_SKINNY_DUAL = 18,
  GF_Q4_256 = 19, GF_Q4_128 = 20,                // gemm_q4_kernel, 256x384 / 128x384
};

struct SplitPlan { int S; int Ks; };

struct GemmRoute {
  int err = 0;                   // kGemmInvalid: refused
  GemmFamily family = GF_NONE;
  int epi = 0;                   // epilogue instantiation of the persistent / wide / four-wave kernels (0 elsewhere)
  bool vec = false;              // 4-column vector epilogue (every output and epilogue operand 4-element aligned)
  bool wide8 = false;            // 8-column bf16-output epilogue layout
  bool asm_lds = true;           // gemm_kernel: inline-asm LDS-DMA pipeline
  SplitPlan split{1, 0};         // GF_SPLITK: S partial problems of Ks columns of K
  int kernel_id = 0;             // GemmArgs::kernel_id; a refusal from inside a persistent family still names it
};

inline bool aligned_to(const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) % a) == 0; }
inline long long gemm_batches(const GemmArgs& a) { return a.batch > 0 ? a.batch : 1; }
inline long long tiles_of(long long M, long long N, int BM, int BN) { return ((M + BM - 1) / BM) * ((N + BN - 1) / BN); }
// the 256x256 grid fills the chip (>= ~1 workgroup per CU; measured: 192 tiles of 256x256 beat 768 of 128x128 by 10-28 %)
inline bool fills_chip(long long tiles256) { return tiles256 >= 160; }
// the 128x128 grid would leave most CUs idle: the small-grid kernels
inline bool underfilled(long long tiles128) { return tiles128 < 128; }
// 32-bit LDS-DMA offsets of the persistent / wide / four-wave kernels (A is priced at 2 bytes per element, fp8 included)
inline bool lds_dma_offsets_fit(const GemmArgs& a, long long w_bytes) {
  return (long long)a.M * a.lda * 2 < (1LL << 32) && (long long)a.N * a.ldw * w_bytes < (1LL << 32);
}
// gemm_tile 0 with the small-grid kernels on: what the grouped and dual forms (gemm_resident_kernel only) need
inline bool small_grid_kernels_on(const Tuning* t) { return gemm_tile(t) == 0 && gemm_small(t) && gemm_resident(t); }
// the 256x256 / 256x384 / four-wave persistent kernels share these knobs
inline bool persistent_knobs_on(const Tuning* t) { return gemm_persist(t) && gemm_raster(t) == 0 && gemm_epi(t); }

// ------------------------------------------------------------------------------------------------ refusals: malformed forms
inline bool bad_operands(const GemmArgs& a, bool is_bf16) {
  const size_t es = is_bf16 ? 2 : 4, esw = a.w8 ? 1 : es;   // fp8 weights: ldw / bsW count bytes
  const int BK = 128 / (int)es;                             // K granularity of the widest K-slice
  if (a.K <= 0 || a.K % BK != 0) return true;
  if (a.x3 && is_bf16) return true;   // split-bf16 splits fp32 operands
  if (a.w8 && (!is_bf16 || !a.wscale || a.N % 4 != 0 || a.K % 64 != 0 || a.batch > 1 || !aligned_to(a.wscale, 16))) return true;
  // LDS-DMA reads 16-B chunks: rows must start 16-B aligned
  return !aligned_to(a.A, 16) || !aligned_to(a.W, 16) || (a.lda * es) % 16 || (a.ldw * esw) % 16 || (a.bsA * es) % 16 || (a.bsW * esw) % 16;
}
inline bool bad_grouped(const GemmArgs& a, bool is_bf16) {
  return !is_bf16 || a.w8 || a.a8 || a.act != ACT_NONE || a.mul || a.res || a.resT || a.outT || a.out8 || a.ssq_out || a.rs_ssq || a.rb > 0 || !a.out32 ||
         a.K % 64 != 0 || !small_grid_kernels_on(a.tune);
}
inline bool bad_dual(const GemmArgs& a, bool is_bf16) {
  return !is_bf16 || a.w8 || a.a8 || a.mul || a.res || a.resT || a.out32 || a.out8 || a.ssq_out || (a.rs_ssq && !a.rs_sum) || a.rb > 0 || a.batch > 1 || a.grp_col ||
         !a.outT || !a.A2 || a.K % 64 != 0 || a.N % 4 != 0 || !aligned_to(a.A2, 16) || !aligned_to(a.W2, 16) || (a.lda2 * 2) % 16 || (a.ldw2 * 2) % 16 ||
         !small_grid_kernels_on(a.tune);
}
// a batch of hm_L rows must be whole 256-row tiles, the columns whole 256-column tiles and a head a power of two >= 8 columns; the opt-in 256x384
// kernel has no head-major epilogue.
// Whether the problem REACHES a kernel with that epilogue is the route's business (gemm_route refuses hm_D at its end).
inline bool bad_headmajor(const GemmArgs& a, bool is_bf16) {
  if (!is_bf16 || !a.outT || a.out32 || a.mul || a.res || a.resT || a.out8 || a.ssq_out || a.rb > 0 || a.batch > 1 || a.grp_col || a.W2) return true;
  if (a.hm_D < 8 || (a.hm_D & (a.hm_D - 1)) || a.hm_L <= 0 || a.hm_L % 256 != 0 || a.M % a.hm_L != 0 || a.N % a.hm_D != 0 || a.N % 256 != 0 || gemm_wide(a.tune)) return true;
  if (a.a8) return a.lda % 16 != 0;                 // fp8 rows are bytes (bad_operands prices lda at two)
  return !lds_dma_offsets_fit(a, 2);                // W priced as bf16 whatever it holds
}
inline bool bad_split_n(const GemmArgs& a, bool is_bf16, bool vec) {
  return !is_bf16 || !vec || !a.outT || !a.outT_lo || a.out32 || a.out8 || a.mul || a.res || a.resT || a.ssq_out || a.hm_D || a.pair32 || a.W2 || a.grp_col ||
         a.batch > 1 || a.split_n <= 0 || a.split_n >= a.N || a.split_n % 128 != 0 || a.N % 8 != 0 || a.ldT_lo % 8 != 0 || !aligned_to(a.outT_lo, 16) ||
         a.w8 || a.a8 || gemm_splitk(a.tune);
}
inline bool bad_pair(const GemmArgs& a, bool is_bf16, bool vec) {
  return !is_bf16 || !vec || a.w8 || a.a8 || a.act != ACT_GELU || a.mul || a.res || a.resT || a.out32 || a.out8 || a.ssq_out || (a.rs_ssq && !a.rs_sum) || a.rb > 0 ||
         a.batch > 1 || a.hm_D || !a.outT || a.N % 128 != 0 || a.K % 64 != 0 || a.ldT % 8 != 0 || !aligned_to(a.outT, 16);
}

inline bool vector_epilogue(const GemmArgs& a, size_t es) {
  bool v = (a.N % 4 == 0);
  if (a.bias) v = v && aligned_to(a.bias, 16) && (a.bsBias % 4 == 0);
  if (a.mul) v = v && aligned_to(a.mul, 4 * es) && (a.ldmul % 4 == 0) && (a.bsMul % 4 == 0);
  if (a.res) v = v && aligned_to(a.res, 16) && (a.ldres % 4 == 0) && (a.bsRes % 4 == 0);
  if (a.resT) v = v && aligned_to(a.resT, 4 * es) && (a.ldresT % 4 == 0);
  if (a.out32) v = v && aligned_to(a.out32, 16) && (a.ld32 % 4 == 0) && (a.bs32 % 4 == 0);
  if (a.outT) v = v && aligned_to(a.outT, 4 * es) && (a.ldT % 4 == 0) && (a.bsT % 4 == 0);
  return v;
}
inline bool wide8_epilogue(const GemmArgs& a, bool vec) {
  return vec && (a.outT || a.out8) && !a.out32 && a.N % 8 == 0 && a.ldT % 8 == 0 && a.bsT % 8 == 0 && aligned_to(a.outT, 16) &&
         (!a.out8 || (a.ld8 % 8 == 0 && aligned_to(a.out8, 8))) && (!a.mul || (a.ldmul % 8 == 0 && a.bsMul % 8 == 0 && aligned_to(a.mul, 16))) &&
         (!a.resT || (a.ldresT % 8 == 0 && aligned_to(a.resT, 16)));
}

// ------------------------------------------------------------------------------------------------ split-K
// With M = 8 .. 512 rows (batch 1 .. 32 decoder / prompt GEMMs) a 128x128 grid has 6 .. 100 workgroups, each walking
// its K dimension serially at the per-CU operand-path rate (~23 B/clk): 8 us at K = 768, 30 us at K = 3072, most CUs
// idle. Such problems are split along K into S ranges (pass 1: the same kernel, batched over the ranges, raw fp32
// partials) and finished by an elementwise pass that sums the partials in split order -- deterministic -- and applies
// the whole epilogue. The summation order differs from the single-pass kernels, i.e. results would depend (at fp32
// rounding level) on whether a problem was small enough to be split -- batch-composition and chunking invariance would
// only hold to bf16 tolerance. Measured gain: 35 -> 25 us at M = 8, K = 3072; nothing at K = 768 (a second launch costs
// as much as the saved slices); batch-1 step 6.2 -> 5.5 ms. It is therefore OPT-IN (option gemm_splitk / VIMA_GEMM_SPLITK).
inline SplitPlan splitk_plan(const GemmArgs& a, bool is_bf16) {
  SplitPlan p{1, a.K};
  if (!gemm_splitk(a.tune) || a.w8) return p;
  const int bk = is_bf16 ? 64 : 32;
  if (a.batch > 1 || a.M <= 0 || a.N <= 0 || a.K % bk || a.N % 4 || a.ssq_out || a.rb > 0 || a.resT) return p;
  if (a.pair32 || a.hm_D || a.W2 || a.grp_col || a.rs_sum || a.sum_out) return p;   // forms whose epilogue the reduce pass does not have
  const long long tiles = tiles_of(a.M, a.N, 128, 128);
  const int slices = a.K / bk;
  if (tiles >= 128 || slices < 24) return p;   // measured: the second pass only pays from K = 1536 (bf16) on
  const int want = (int)((256 + tiles - 1) / tiles);
  int best = 1;
  for (int s = 2; s <= want && s * 2 <= slices; ++s)
    if (slices % s == 0) best = s;
  if (best > 1) { p.S = best; p.Ks = slices / best * bk; }
  return p;
}
// takes it when the caller brought the scratch (GemmArgs::splitk_ws) and the reduce pass can use 4-element vectors throughout
inline bool splitk_takes(const GemmArgs& a, bool is_bf16, SplitPlan& sp) {
  if (!a.splitk_ws) return false;
  const size_t es = is_bf16 ? 2 : 4;
  sp = splitk_plan(a, is_bf16);
  const bool ok4 = (!a.bias || aligned_to(a.bias, 16)) && (!a.mul || (aligned_to(a.mul, 4 * es) && a.ldmul % 4 == 0)) &&
                   (!a.res || (aligned_to(a.res, 16) && a.ldres % 4 == 0)) && (!a.out32 || (aligned_to(a.out32, 16) && a.ld32 % 4 == 0)) &&
                   (!a.outT || (aligned_to(a.outT, 4 * es) && a.ldT % 4 == 0));
  return sp.S > 1 && ok4 && a.splitk_ws_bytes >= (size_t)sp.S * a.M * a.N * sizeof(float) && aligned_to(a.splitk_ws, 16);
}

// ------------------------------------------------------------------------------------------------ the families' own tests
// Each answers with the epilogue / tile it would run, or 0 / GF_NONE / false: declines, the next family is asked.

// 256x256 persistent kernels: the specialised epilogue for the combinations the policy uses (0 = none of them)
inline int persistent_epi(const GemmArgs& a, bool wide8) {
  if (a.rb != 0) return 0;
  if (wide8 && !a.mul && !a.res && !a.resT && !a.ssq_out) return 1;
  if (wide8 && a.mul && a.outT && !a.out8 && !a.res && !a.resT && !a.rs_ssq && !a.ssq_out) return 2;
  if (!wide8 && a.out32 && !a.mul && !a.rs_ssq && !a.resT) return 3;   // fp32 (+ operand-type) output, with or without a residual
  if (wide8 && a.resT && !a.mul && !a.res && !a.rs_ssq) return 4;
  return 0;
}
// gemm_persistent_kernel; also the second half of gemm_pp_kernel's test. Head-major output is its own instantiation (5; as a run-time
// branch of epilogue 1 it cost every row-major launch ~9 %).
inline int persistent_takes(const GemmArgs& a, bool wide8) {
  if (a.split_n) return 0;   // (the column-split output is not part of the 256x256 epilogues)
  const int epi = persistent_epi(a, wide8);
  if (a.resT && epi != 4) return 0;
  if (a.hm_D) return 5;
  switch (a.act * 8 + epi) {   // the instantiations; everything else (the all-runtime form spills) is left to the one-tile-per-workgroup kernel
    case ACT_NONE * 8 + 1: case ACT_NONE * 8 + 3: case ACT_NONE * 8 + 4: case ACT_RELU * 8 + 1: case ACT_GELU * 8 + 2: case ACT_QUICKGELU * 8 + 1: return epi;
    default: return 0;
  }
}
// gemm_pp_kernel: as above plus an even number of K-tiles and bf16 weights, or both operands fp8 with K % 256 == 0 (F8: the bf16-output and
// bf16-stream epilogues only); 6 = the GEGLU pair over block-interleaved weights
inline int pp_takes(const GemmArgs& a, bool wide8) {
  if (a.a8) { if (!a.w8 || a.K % 256 != 0) return 0; }
  else if (a.w8 || (a.K / 64) % 2 != 0 || a.out8) return 0;   // (an fp8 copy of a bf16-operand GEMM's output: gemm_persistent_kernel)
  if (a.pair32) return (a.split_n || a.a8 || a.act != ACT_GELU) ? 0 : 6;
  return persistent_takes(a, wide8);
}
// ... and what the two REFUSE outright once they have taken a problem (nothing after them has these forms either): head-major output other than
// of the bf16-output epilogue without activation, fp8 operands outside the bf16-output and bf16-stream epilogues
inline bool persistent_epilogue_exists(const GemmArgs& a, bool wide8, int epi) {
  if (a.hm_D && (persistent_epi(a, wide8) != 1 || a.act != ACT_NONE)) return false;
  return !(a.a8 && epi != 1 && epi != 4 && epi != 5);
}
// gemm_wide_kernel (256x384): bf16-output and bf16-stream epilogues on at least 128 full tiles
inline int wide_takes(const GemmArgs& a, bool wide8) {
  if (a.w8 || a.rb != 0 || a.batch > 1 || a.M % 256 || a.N % 384 || a.K < 2 * 64 || a.K % 64 || !wide8) return 0;
  if (!lds_dma_offsets_fit(a, 2)) return 0;
  if (a.mul || a.res || a.out32 || a.hm_D || a.split_n) return 0;
  if ((long long)(a.M / 256) * (a.N / 384) < 128) return 0;
  if (!a.resT && !a.ssq_out) return (a.act == ACT_NONE || a.act == ACT_RELU || a.act == ACT_QUICKGELU) ? 1 : 0;
  return (a.resT && !a.rs_ssq && a.act == ACT_NONE) ? 4 : 0;
}
// gemm_q4_kernel (BM x 384, BM = 256 or 128): bf16-output / bf16-stream / head-major epilogues on at least 128 full tiles
inline int q4_takes(const GemmArgs& a, bool wide8, int BM) {
  if (a.w8 || a.a8 || a.rb != 0 || a.batch > 1 || a.M % BM || a.N % 384 || a.K < 128 || a.K % 128 || !wide8) return 0;
  if (!lds_dma_offsets_fit(a, 2)) return 0;
  if (a.mul || a.res || a.out32 || a.out8 || a.split_n || a.pair32 || a.sum_out || a.rs_sum) return 0;
  if (a.rs_ssq && (a.rs_parts != 24 || a.resT)) return 0;   // fused-RMSNorm consumer: E = 768 (24 partials per row), bf16-output epilogues
  if ((long long)(a.M / BM) * (a.N / 384) < 128) return 0;
  // ... on the 128 x 384 tile the partials sit in LDS behind the ring (epilogues 1 / 5 as they are); the 256 x 384 tile has no LDS left and carries the four
  // row scales of a lane in registers: its own epilogue 7 -- bf16 output, no bias (the form is instantiated without the bias epilogue: its 48 column registers
  // beside the four held scales do not fit the kernel's 256 VGPRs, which already stand at 254 / 256), no activation or ReLU: T5's q|k|v and wi. Option gemm_q4_rs = 0 leaves these consumers to gemm_pp_kernel.
  if (a.rs_ssq && BM == 256) {
    if (!gemm_q4_rs(a.tune) || a.bias || a.ssq_out || a.hm_D) return 0;
    return (a.act == ACT_NONE || a.act == ACT_RELU) ? 7 : 0;
  }
  if (!a.resT && !a.ssq_out) {
    if (a.hm_D) return (a.act == ACT_NONE && a.hm_L % BM == 0) ? 5 : 0;
    return (a.act == ACT_NONE || a.act == ACT_RELU || a.act == ACT_QUICKGELU) ? 1 : 0;
  }
  return (a.resT && a.act == ACT_NONE && !a.hm_D) ? 4 : 0;
}
// gemm_q4: 1 = the 256 x 384 tile wherever it fits, 2 = the 128 x 384 tile wherever it fits, 3 = the 128 x 384 tile where it needs fewer ROUNDS of the chip than
// the 256 x 256 tiling. A round of 128 x 384 tiles is 0.75 of a round of 256 x 256 tiles in FLOPs and measures ~0.8 of it in time (12 MFMAs per phase and barrier
// instead of 24); the margin keeps the choice away from ties. M = 16 384 (batch 32): N = 768 one round instead of one of 192 tiles, N = 1536 / 2304 2 / 3 rounds
// instead of 2 / 3 larger ones; the batch-256 shapes (M = 131 072, 81 920) never qualify. The choice depends on the SHAPE only, and the tile is bit-identical anyway.
// 6 (the default since the end of round 6) = the 256 x 384 tile for GEMMs of at least 32 768 rows. Kernel for kernel the two tilings take the same time
// (power-bound: DESIGN.md 4.2c) -- but with the model's TWO streams the four-wave kernel's 7 % fewer busy cycles are left to whatever runs beside it:
// wall clock of the headline step 53.63 -> 52.89 ms, 1024-token prompt 109.8 -> 108.2, T = 8 65.6 -> 65.0, batch 128 27.85 -> 27.58 (alternating, same box:
// profiles/r06_q4_wall_clock.txt); below that size it loses (batch 32 +5 %, the env steps +1 %, VIMA-20M batch 32 +3 %), hence the row threshold.
// 4 / 5 (lab): the 256 x 384 tile for the wide-N GEMMs only / for N = 768 only. -> the tile's rows (256 / 128), 0 = not this problem
inline int q4_tile_rows(const GemmArgs& a, int ncu) {
  int mode = gemm_q4(a.tune);
  if (mode == 6) mode = a.M >= 32768 ? 1 : 0;
  if (mode == 4) mode = a.N >= 1536 ? 1 : 0;
  if (mode == 5) mode = a.N == 768 ? 1 : 0;
  if (mode == 3) {
    mode = 0;
    if (a.M % 128 == 0 && a.N % 384 == 0 && a.M % 256 == 0 && a.N % 256 == 0) {
      const long long r_pp = ((long long)(a.M / 256) * (a.N / 256) + ncu - 1) / ncu;
      const long long r_h = ((long long)(a.M / 128) * (a.N / 384) + ncu - 1) / ncu;
      if (r_h * 80 <= r_pp * 93) mode = 2;
    }
  }
  return mode == 0 ? 0 : (mode == 2 ? 128 : 256);
}
// gemm_resident_kernel, bf16 problems with a vector-aligned epilogue and no fp8 operands. Tile (`force`: gemm_tile 10 / 11 / 12 = 32x32 /
// 64x32 / 64x64 whatever the grid): the smallest one whose grid still fits the chip once (`gemm_res_maxwg`, default 256 = one
// workgroup per CU; M <= 32 always takes 32x32) -- a lone 32x32 accumulator per wave is a dependent MFMA chain, so what counts is
// how many of them run side by side, not the operand bytes per FLOP (measured, profiles/r03_small_m.txt).
// GEGLU pair (W2): 32x32 for M <= 32, else 64x64 while its grid fits the chip once.
inline GemmFamily resident_takes(const GemmArgs& a, int force) {
  if (a.w8 || a.a8 || a.out8 || a.K % 64 != 0 || (a.N % 4 != 0 && !a.grp_col)) return GF_NONE;
  if ((a.ssq_out || a.resT) && a.act != ACT_NONE) return GF_NONE;   // the kernel applies the bf16 residual / the statistics only without an activation
  const long long nb = gemm_batches(a), maxwg = gemm_res_maxwg(a.tune);
  const long long m32 = (a.M + 31) / 32, m64 = (a.M + 63) / 64, n32 = (a.N + 31) / 32, n64 = (a.N + 63) / 64;
  if (a.W2) return a.act != ACT_GELU ? GF_NONE : (a.M <= 32 ? GF_RT32_DUAL : (m64 * n64 <= maxwg ? GF_RT64_DUAL : GF_NONE));
  if (force) return (GemmFamily)force;
  if (a.M <= 32) return (n32 * nb <= 4 * maxwg || a.grp_col) ? GF_RT32 : GF_NONE;
  if (m32 * n32 * nb <= maxwg) return GF_RT32;
  if (m64 * n32 * nb <= maxwg) return GF_RT64x32;
  return (m64 * n64 * nb <= maxwg || a.grp_col) ? GF_RT64 : GF_NONE;
}
// gemm_skinny_kernel: bf16 problems of at most 32 rows with a vector-aligned epilogue and no fp8 operands (buffer descriptors with 31-bit byte ranges)
inline bool skinny_takes(const GemmArgs& a) {
  if (a.M > 32 || a.w8 || a.a8 || a.out8 || a.K % 64 != 0 || a.N % 4 != 0 || a.grp_col || a.hm_D || a.pair32) return false;
  if ((a.ssq_out || a.resT) && a.act != ACT_NONE) return false;
  if (a.W2 && (a.act != ACT_GELU || a.K > 2048)) return false;
  if ((long long)a.M * a.lda * 2 >= (1LL << 31) || (long long)a.N * a.ldw * 2 >= (1LL << 31)) return false;
  return !(a.W2 && ((long long)a.M * a.lda2 * 2 >= (1LL << 31) || (long long)a.N * a.ldw2 * 2 >= (1LL << 31)));
}
// The GEGLU pair over block-interleaved weights ([M, N / 2] output) is the form to USE -- a preference, not only availability: not where the
// dual form runs (small grids), not where the GELU GEMM takes a persistent kernel's gate epilogue (the chip is filled but the pair's own
// conditions for gemm_pp_kernel fail), not on small grids that the 64x64 / resident tiles serve. Otherwise: gemm_pp_kernel's pair epilogue
// when the interleaved [M, N] problem fills the chip with full tiles, else the 128x128 ring tile's.
inline bool pair_takes_pp(const GemmArgs& a) {
  const Tuning* t = a.tune;
  if (a.M % 256 != 0 || a.N % 256 != 0 || a.K < 128 || gemm_tile(t) != 0 || !persistent_knobs_on(t) || !gemm_pp(t) || gemm_wide(t) || gemm_variant(t) != 1) return false;
  return fills_chip((long long)(a.M / 256) * (a.N / 256)) && pp_takes(a, true) == 6;
}
inline bool pair_preferred(const GemmArgs& a) {
  const Tuning* t = a.tune;
  const int Nout = a.N / 2;
  if (gemm_tile(t) != 0 || gemm_variant(t) != 1 || !gemm_epi(t) || gemm_raster(t) != 0) return false;
  GemmArgs dual = a;   // the same output as a dual launch
  dual.N = Nout; dual.W2 = a.W;
  if (small_grid_kernels_on(t) && Nout % 4 == 0 && resident_takes(dual, 0) != GF_NONE) return false;
  if (pair_takes_pp(a)) return true;
  if (fills_chip(tiles_of(a.M, Nout, 256, 256))) return false;
  return !(gemm_small(t) && underfilled(tiles_of(a.M, Nout, 128, 128)));
}

#ifdef VIMA_GEMM_LAB
// scripts/micro/gemm_lab.hip instantiates the 256-row bf16 kernels only (fp8 weights: together with fp8 activations)
inline bool lab_build_has(const GemmRoute& r, const GemmArgs& a) {
  switch (r.family) {
    case GF_PP: case GF_PERSISTENT: case GF_WIDE: case GF_TILE_L: case GF_Q4_256: case GF_Q4_128: return !a.w8;
    case GF_PP_F8: case GF_NONE: return true;
    default: return false;
  }
}
#endif

// ------------------------------------------------------------------------------------------------ the route
inline GemmRoute gemm_route_full(const GemmArgs& a, bool is_bf16, int ncu) {
  GemmRoute r;
  const size_t es = is_bf16 ? 2 : 4;
  const Tuning* t = a.tune;
  const auto refuse = [&r]() { r.err = kGemmInvalid; return r; };
  const auto take = [&](GemmFamily f, int epi = 0) {
    const int kind = (a.x3 && f == GF_TILE_S) ? 21 : (a.x3 && f == GF_SPLITK) ? 23 : (f == GF_TILE_64x128 || f == GF_TILE_128x64) ? 0 : (int)f;
    r.family = f; r.epi = epi;
    r.kernel_id = kind ? kind * 1000 + (a.act + 1) * 10 + epi : 0;
    return r;
  };
  if (a.M <= 0 || a.N <= 0) return r;
  if (bad_operands(a, is_bf16)) return refuse();
  if (splitk_takes(a, is_bf16, r.split)) return take(GF_SPLITK);   // underfilled grid: two deterministic passes
  r.split = SplitPlan{1, a.K};

  // ---- malformed forms
  if (a.grp_col && bad_grouped(a, is_bf16)) return refuse();
  if (a.W2 && bad_dual(a, is_bf16)) return refuse();
  if (a.resT && (a.res || a.batch > 1 || a.act != ACT_NONE)) return refuse();
  if (a.hm_D && bad_headmajor(a, is_bf16)) return refuse();
  // fused LayerNorm: partial sums ride with the partial sums of squares of an fp32-output producer; the consumers are the two GEGLU-pair forms.
  // They exist in the resident kernel's epilogue and in the ring tiles' LDS epilogue: off the `large` path, counted without its padding-waste
  // test so that the answer depends on the tile count alone.
  const int gt = gemm_tile(t);
  const bool fills = fills_chip(tiles_of(a.M, a.N, 256, 256) * gemm_batches(a));
  if (a.sum_out && (!is_bf16 || !a.ssq_out || !a.out32 || a.N % 32 != 0 || (gt >= 2 && gt < 7) || (gt == 0 && fills))) return refuse();
  if (a.rs_sum && (!is_bf16 || !a.rs_ssq || !a.rs_c || !(a.pair32 || a.W2) || !aligned_to(a.rs_c, 16))) return refuse();
  if (a.ssq_out && ((!a.out32 && !a.outT) || a.batch > 1 || a.N % 32 != 0)) return refuse();
  if (a.rs_ssq && a.rs_parts <= 0) return refuse();
  const bool v = r.vec = vector_epilogue(a, es);
  if (a.w8 && !v) return refuse();   // fp8 weights need the vector epilogue (16-byte aligned outputs)
  // column-split output: the VECTOR epilogues of the one-tile-per-workgroup / resident / skinny kernels only (the scalar epilogue and the persistent
  // kernels' epilogues do not know split_n: a launch that could reach them is refused, never mis-stored)
  if (a.split_n && bad_split_n(a, is_bf16, v)) return refuse();
  r.wide8 = is_bf16 && wide8_epilogue(a, v);
  // RMS partials without the fp32 stream exist only in the 8-column layout (statistics of the stored bf16 values)
  if (is_bf16 && a.ssq_out && !a.out32 && !r.wide8) return refuse();

  // ---- forms with one home
  if (is_bf16 && (a.grp_col || a.W2)) {   // grouped / dual: the skinny kernel (dual, M <= 32), else the resident kernel
    if (a.W2 && !v) return refuse();
    if (a.W2 && a.M <= 32 && gemm_skinny(t) && skinny_takes(a)) return take(GF_SKINNY_DUAL);
    const GemmFamily f = resident_takes(a, 0);
    return f != GF_NONE ? take(f) : refuse();
  }
  if (a.pair32) {
    if (bad_pair(a, is_bf16, v) || !pair_preferred(a)) return refuse();
    if (pair_takes_pp(a) && lds_dma_offsets_fit(a, 2)) { r.wide8 = true; return take(GF_PP, 6); }
    return take(GF_TILE_S);
  }

  // ---- bf16: the 256-row kernels while the 256x256 grid fills the chip and padding waste is small
  if (is_bf16) {
    const long long mt = (a.M + 255) / 256, nt = (a.N + 255) / 256;
    const double waste = (double)(mt * 256) * (double)(nt * 256) / ((double)a.M * (double)a.N);
    bool large = v && fills && waste < 1.15;
    if (gt == 1) large = false;
    if (gt >= 2 && gt < 7) large = v;
    if (gt >= 7) large = false;
    if (a.split_n) large = false;   // after every override: the column-split output exists in the one-tile-per-workgroup / resident / skinny epilogues only
    const bool auto_fast = large && gt == 0 && persistent_knobs_on(t);
    if (auto_fast && gemm_q4(t)) {
      if (const int BM = q4_tile_rows(a, ncu))
        if (const int epi = q4_takes(a, r.wide8, BM)) return take(BM == 128 ? GF_Q4_128 : GF_Q4_256, epi);
    }
    if (auto_fast && gemm_wide(t)) {
      if (const int epi = wide_takes(a, r.wide8)) return take(GF_WIDE, epi);
    }
    if (large && (gt == 0 || gt == 2) && persistent_knobs_on(t) && a.batch <= 1 && a.K >= 2 * 64 && a.M % 256 == 0 && a.N % 256 == 0 &&
        lds_dma_offsets_fit(a, a.w8 ? 1 : 2)) {
      if (gemm_pp(t) || a.a8) {
        if (const int epi = pp_takes(a, r.wide8)) { take(a.a8 ? GF_PP_F8 : GF_PP, epi); return persistent_epilogue_exists(a, r.wide8, epi) ? r : refuse(); }
      }
      if (a.a8) return refuse();   // fp8 activations exist on the ping-pong kernel only
      if (const int epi = persistent_takes(a, r.wide8)) { take(GF_PERSISTENT, epi); return persistent_epilogue_exists(a, r.wide8, epi) ? r : refuse(); }
    }
    if (a.a8 || a.hm_D) return refuse();   // (head-major output exists in the persistent kernels' epilogue only)
    if (large) return take(GF_TILE_L);
  }
  if (a.a8 || a.hm_D) return refuse();

  // ---- bf16: underfilled 128x128 grids (batch 1 .. 32: M = 8 .. 512) are bound by how fast ONE workgroup walks its K dimension
  // (a 32-KiB slice per ~1400 clocks, most of the A tile being padding rows): smaller tiles move fewer bytes per slice
  // and spread the problem over more CUs. Every tile shape accumulates K in the same order, so results do not depend on the choice.
  if (is_bf16 && v) {
    const bool under = underfilled(tiles_of(a.M, a.N, 128, 128) * gemm_batches(a));
    const int force = (gt >= 10 && gt <= 12) ? gt : 0;
    if (a.M <= 32 && small_grid_kernels_on(t) && gemm_skinny(t) && skinny_takes(a)) return take(GF_SKINNY);   // at most 32 rows: K split over the waves
    if (force || (small_grid_kernels_on(t) && under)) {   // (almost) the whole K extent in flight; bit-identical to the ring tiles
      const GemmFamily f = resident_takes(a, force);
      if (f != GF_NONE) return take(f);
    }
    if (gt == 0 && gemm_small(t) && under) return take(a.M <= 32 ? GF_TILE_XS : GF_TILE_64);
    if (gt == 13) return take(GF_TILE_64x128);
    if (gt == 14) return take(GF_TILE_128x64);
    if (gt == 7) return take(GF_TILE_XS);
    if (gt == 8) return take(GF_TILE_64);
  }
  r.asm_lds = gemm_variant(t) == 1 || a.w8;
  return take(GF_TILE_S);
}

inline GemmRoute gemm_route(const GemmArgs& a, bool is_bf16, int ncu) {
  GemmRoute r = gemm_route_full(a, is_bf16, ncu);
#ifdef VIMA_GEMM_LAB
  if (!r.err && !lab_build_has(r, a)) r.err = kGemmInvalid;   // the ONE place where the lab binary narrows the route
#endif
  return r;
}

// ------------------------------------------------------------------------------------------------ the questions callers ask first
// Each builds the canonical problem of its form -- aligned operands, dense leading dimensions unless given -- and reads the route.
namespace route_q {
inline const void* const kPtr = reinterpret_cast<const void*>(uintptr_t(1) << 20);   // any aligned non-null address: never dereferenced
inline void* out_ptr() { return const_cast<void*>(kPtr); }
inline bool fits_int(long long v) { return v >= -2147483647LL - 1 && v <= 2147483647LL; }
// a dense bf16 problem with a bf16 output; sizes beyond int have no GemmArgs and get M = 0 (every question then answers 0)
inline GemmArgs problem(const Tuning* t, long long M, long long N, long long K, long long lda, long long ldw) {
  GemmArgs a;
  const bool fits = fits_int(M) && fits_int(N) && fits_int(K) && fits_int(lda) && fits_int(ldw);
  a.A = kPtr; a.W = kPtr; a.M = fits ? (int)M : 0; a.N = (int)N; a.K = (int)K; a.lda = (int)lda; a.ldw = (int)ldw; a.tune = t;
  a.outT = out_ptr(); a.ldT = (int)N;
  return a;
}
inline bool routed(const GemmArgs& a, int ncu) {
  const GemmRoute r = gemm_route(a, true, ncu);
  return !r.err && r.family != GF_NONE;
}
inline GemmArgs pair_problem(const Tuning* t, long long M, long long Nout, long long K) {
  GemmArgs a = problem(t, M, 2 * Nout, K, K, K);
  a.pair32 = 1; a.act = ACT_GELU; a.ldT = (int)Nout;
  return a;
}
// the block-interleaved GEGLU pair is the form to use for an [M, Nout] output (gemm_route refuses it elsewhere: pair_preferred)
inline int pair_ok(const Tuning* t, long long M, long long Nout, long long K, int ncu) { return routed(pair_problem(t, M, Nout, K), ncu); }
// ... and runs on gemm_pp_kernel's pair epilogue: 0 as well where the pair is not the form to use (gemm_res_maxwg raised past 1280: the dual
// form wins) or the operands are beyond the kernel's 32-bit offsets (4 GiB of A), i.e. where the launch does not take that kernel.
inline int pair_large(const Tuning* t, long long M, long long Nout, long long K, int ncu) {
  const GemmRoute r = gemm_route(pair_problem(t, M, Nout, K), true, ncu);
  return !r.err && r.family == GF_PP;
}
// GemmArgs::sum_out beside ssq_out on an [M, N] fp32 output
inline int lnfold_producer_ok(const Tuning* t, long long M, long long N, int ncu) {
  GemmArgs a = problem(t, M, N, 64, 64, 64);
  a.outT = nullptr; a.out32 = static_cast<float*>(out_ptr()); a.ld32 = (int)N; a.ssq_out = a.out32; a.sum_out = a.out32;
  return routed(a, ncu);
}
inline int dual_ok(const Tuning* t, int M, int N, int ncu) {
  GemmArgs a = problem(t, M, N, 64, 64, 64);
  a.A2 = kPtr; a.W2 = kPtr; a.lda2 = a.ldw2 = 64; a.act = ACT_GELU;
  return routed(a, ncu);
}
inline int grouped_ok(const Tuning* t, int ncu) {
  GemmArgs a = problem(t, 1, 4, 64, 64, 64);
  a.outT = nullptr; a.out32 = static_cast<float*>(out_ptr()); a.ld32 = 4; a.grp_col = static_cast<const int*>(kPtr);
  return routed(a, ncu);
}
inline GemmArgs a8_problem(const Tuning* t, long long M, long long N, long long K, long long lda, long long ldw) {
  GemmArgs a = problem(t, M, N, K, lda, ldw);
  a.a8 = a.w8 = 1; a.wscale = static_cast<const float*>(kPtr);
  return a;
}
// fp8 activations: the route is gemm_pp_kernel<.., F8>, so that callers can decide BEFORE quantising. Narrower than the route in one point: fp8 rows
// are bytes and must start 16-byte aligned, which bad_operands (pricing lda at two bytes) lets through at lda % 8 == 0.
inline int a8_ok(const Tuning* t, long long M, long long N, long long K, long long lda, long long ldw, int ncu) {
  return lda % 16 == 0 && gemm_route(a8_problem(t, M, N, K, lda, ldw), true, ncu).family == GF_PP_F8;
}
inline int headmajor_ok(const Tuning* t, long long M, long long N, long long K, long long lda, long long ldw, int hm_D, int hm_L, int a8, int ncu) {
  GemmArgs a = a8 ? a8_problem(t, M, N, K, lda, ldw) : problem(t, M, N, K, lda, ldw);
  a.hm_D = hm_D; a.hm_L = hm_L;
  return hm_D != 0 && routed(a, ncu);   // (hm_D 0 is not a head-major problem)
}
}  // namespace route_q

}  // namespace vima
