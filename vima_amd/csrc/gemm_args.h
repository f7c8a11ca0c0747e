// The GEMM launcher's plain declarations -- activation ids, the per-handle knobs and the launch descriptor -- free of HIP, so that
// kernel selection (gemm_route.h) compiles and is tested on the host alone. Included by common.h (Act) and kernels.h.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace vima {

// activations (ids shared with the host side)
enum Act : int { ACT_NONE = 0, ACT_RELU = 1, ACT_GELU = 2, ACT_QUICKGELU = 3 };

// Kernel-selection knobs of ONE handle (vima_set_option). -1 = process default (the VIMA_* environment variable named
// beside each field, read once). They travel with every launch (GemmArgs::tune / AttnArgs::tune): two handles in one
// process never see each other's settings, and a handle's captured hipGraphs are keyed on its own generation counter.
struct Tuning {
  int gemm_variant = -1;   // VIMA_GEMM_VARIANT  1 = inline-asm LDS-DMA pipeline (default), 0 = compiler-tracked builtin (TileS)
  int gemm_tile = -1;      // VIMA_GEMM_TILE     0 auto, 1 128x128, 2 256x256 8 waves, 7 32x64, 8 64x64, 10 / 11 / 12 resident-K 32x32 / 64x32 / 64x64
  int gemm_raster = -1;    // VIMA_GEMM_RASTER   tile order: 0 XCD x n-walk, 1 XCD x resident n-group, 2 row-major
  int gemm_epi = -1;       // VIMA_GEMM_EPI      1 = LDS-transposed row-contiguous epilogue (default), 0 = direct
  int gemm_persist = -1;   // VIMA_GEMM_PERSIST  1 = large bf16 GEMMs on the persistent kernel (default)
  int gemm_small = -1;     // VIMA_GEMM_SMALL    1 = 64x64 / 32x64 tiles for underfilled grids (default)
  int gemm_wide = -1;      // VIMA_GEMM_WIDE     1 = 256x384 persistent tile where N % 384 == 0 (bf16-out / bf16-residual epilogues)
  int gemm_pp = -1;        // VIMA_GEMM_PP       1 = ping-pong (8-phase) main loop on the persistent 256x256 kernel (default), 0 = the round-2 loop
  int gemm_q4 = -1;        // VIMA_GEMM_Q4       four-wave (one wave per SIMD) kernel, N % 384 == 0, K % 128 == 0, bf16-out / bf16-stream / head-major epilogues: 1 = its 256x384 tile wherever it fits,
                           //                    2 = its 128x384 tile wherever it fits, 3 = the 128x384 tile where it needs fewer rounds of the chip than 256x256 tiles (batch 32), 6 = the 256x384 tile from 32 768 rows on (default), 0 = off
  int gemm_q4_rs = -1;     // VIMA_GEMM_Q4_RS    1 = fused-RMSNorm consumers (24 partials per row, bf16 output, no bias) take the 256x384 tile too, row scales carried in registers (default); 0 = they stay on gemm_pp_kernel
  int gemm_splitk = -1;    // VIMA_GEMM_SPLITK   1 = two-pass split-K for underfilled grids with K >= 1536 (default 0)
  int gemm_resident = -1;  // VIMA_GEMM_RESIDENT 1 = underfilled grids on gemm_resident_kernel (whole K in flight; default), 0 = the 4-deep ring tiles
  int gemm_res_maxwg = -1; // VIMA_GEMM_RES_MAXWG largest grid (workgroups) that kernel takes at M > 32 (default 256 = one per CU)
  int gemm_skinny = -1;    // VIMA_GEMM_SKINNY   1 = GEMMs of at most 32 rows on gemm_skinny_kernel (K split over the waves of a workgroup; default), 0 = the resident 32x32 tile (bit-identical to every other tile)
  int gemm_flat = -1;        // VIMA_GEMM_FLAT     1: gemm_pp_kernel drops the XCD raster for small grids where it costs a round (default); 0: never
  int gemm_res_nch = -1;   // VIMA_GEMM_RES_NCH  chunk buffers of that kernel's LDS ring (0 = default: 4 / 5 / 4 = up to 128 KiB; max 5 / 6 / 5 = 160 KiB)
  long long* gemm_dbg = nullptr;   // device buffer [blocks*4] of shader-clock stamps (nullptr = off)
  int attn_split = -1;     // 1 = split-key 4-wave kernel for Lq <= 32 (default), 0 = one-wave kernel
  int attn4_min_lq = -1;   // Lq from which the 4-wave LDS-shared flash kernel is used (default 64)
  int attn_qg = -1;        // query groups of 32 per wave in that kernel: 1 (default) or 2 (64 queries per wave, Lq >= 256)
  long long* attn_dbg = nullptr;   // device buffer [workgroups*8] of phase clocks of the 4-wave kernel (nullptr = off)
};

// ---------------------------------------------------------------- GEMM
// C[M,N] = epilogue( A[M,K] . W[N,K]^T ), fp32 accumulation on the matrix cores.
//   epilogue(v) = ((act(v + bias[n])) * mul[r][n]) + res[r][n]
// Operand type T (A, W, mul, outT) is bf16 (mfma_f32_32x32x16_bf16) or float
// (mfma_f32_32x32x2_f32, exact-fp32 parity mode).
struct GemmArgs {
  const void* A = nullptr;   // [M,K] row-major, row stride lda (elements)
  const void* W = nullptr;   // [N,K] row-major (nn.Linear layout), row stride ldw
  int M = 0, N = 0, K = 0;
  int lda = 0, ldw = 0;
  int batch = 1;             // blockIdx.y; strides below in elements
  // GROUPED form (batch = groups; bf16, gemm_resident_kernel only -- gemm_grouped_ok()): group z multiplies A + z * bsA with the rows
  // [grp_col[z], grp_col[z + 1]) of ONE packed W [sum N_z, K] and writes bias + product to the same COLUMNS of out32 (fp32, any
  // alignment: scalar stores); N = the largest group; no activation / mul / residual / outT. grp_col: DEVICE array [batch + 1].
  const int* grp_col = nullptr;
  // DUAL form (bf16, gemm_resident_kernel only -- ask gemm_dual_ok() first): out = act(A . W^T + bias) * bf16(A2 . W2^T), the value /
  // gate pair of a GEGLU in ONE launch (W2 [N, K] row stride ldw2, A2 [M, K] row stride lda2; A2 may be A). Bit-identical to the two
  // launches (gate stored in bf16, then read as `mul`). outT only; act = ACT_GELU; no mul / residual / batch.
  const void* A2 = nullptr; const void* W2 = nullptr; int lda2 = 0, ldw2 = 0;
  long long bsA = 0, bsW = 0, bsBias = 0, bsMul = 0, bsRes = 0, bs32 = 0, bsT = 0;
  const float* bias = nullptr;
  int act = ACT_NONE;
  const void* mul = nullptr;  // T [M, ldmul]
  int ldmul = 0;
  const float* res = nullptr; // fp32 [M, ldres]  (may alias out32: each element is read then written by one thread)
  int ldres = 0;
  const void* resT = nullptr; // the same residual term in the OPERAND type T [M, ldresT] (residual stream carried in T; may
  int ldresT = 0;             // alias outT). At most one of res / resT.
  float* out32 = nullptr;
  int ld32 = 0;
  void* outT = nullptr;
  int ldT = 0;
  // HEAD-MAJOR output (hm_D > 0; bf16-only output of the persistent 256x256 kernels, ask gemm_headmajor_ok() first): rows are hm_L-row
  // batches, columns hm_D-wide heads, and element (r, n) goes to outT[((r / hm_L) * (N / hm_D) + n / hm_D) * hm_L * hm_D + (r % hm_L) * hm_D + n % hm_D]
  // -- [batch][head][row][hm_D], every head's rows contiguous -- instead of outT[r * ldT + n]. The decoder's prompt K / V cache is written
  // this way so that the split-key cross attention streams 32-KB runs per (batch, head) instead of 64-byte slices of 3-KB rows.
  int hm_D = 0, hm_L = 0;
  // GEGLU PAIR (pair32 = 1; bf16, act = ACT_GELU, ask gemm_pair_ok() first): W [N, K] and bias [N] hold TWO layers of N / 2 outputs each, alternating in
  // blocks of 32 rows -- block 2j = rows 32j.. of the GELU'd layer, block 2j + 1 = rows 32j.. of its plain multiplier -- and the output is
  // outT[m][j] = bf16(gelu(A.W1[j] + b1[j]) * bf16(A.Wg[j] + bg[j])), [M, N / 2]: bit-identical to the multiplier GEMM (bf16 output) followed by the
  // GELU GEMM with `mul`, in one launch of the 128x128 ring tile (both factors of an output element sit in one lane's accumulators).
  int pair32 = 0;
  // output-row remap (outputs only): orow = (r / rb) * s_hi + (r % rb) * s_lo + ro ; rb == 0 -> identity
  int rb = 0, s_hi = 0, s_lo = 0, ro = 0;
  // COLUMN-SPLIT output (bf16, outT only, no residual / gate / statistics; split_n % 128 == 0): columns n < split_n are stored to outT_lo[r * ldT_lo + n]
  // (rows NOT remapped), columns n >= split_n to outT[orow * ldT + (n - split_n)]. One launch for the self-attention projection of an incremental
  // decoding step: q of the new tokens to a dense buffer, their k | v rows appended to the episode cache through the row remap (components.py:51-58).
  void* outT_lo = nullptr;
  int ldT_lo = 0, split_n = 0;
  // RMS statistics fused into the GEMMs either side of a T5 RMSNorm (the norm's weight is folded into W at pack time):
  //   producer: ssq_out[r][j] = sum over columns [32j, 32j+32) of out[r][n]^2 (final fp32 values; needs out32, N % 32 == 0,
  //             batch 1). Plain stores of N/32 partials per row -- no atomics, so the result is deterministic and the
  //             same for every tile shape.
  //   consumer: accumulator row r is multiplied by rsqrt((sum_j rs_ssq[r][j], j < rs_parts) * rs_invk + rs_eps) before
  //             bias / activation
  float* ssq_out = nullptr;
  const float* rs_ssq = nullptr;
  int rs_parts = 0;
  float rs_invk = 0.f, rs_eps = 0.f;
  // nn.LayerNorm (mean AND variance, affine) folded the same way -- the pre-LN in front of XAttention's feed-forward (components.py:220-226), whose
  // GEGLU then reads ONE input (the un-normed stream) for both products:
  //   producer (fp32-output residual GEMM, with ssq_out): sum_out[r][j] = sum over columns [32j, 32j+32) of out[r][n]; ask gemm_lnfold_producer_ok()
  //   consumer (the GEGLU pair forms, pair32 or W2, with rs_ssq): mean = sum_j rs_sum[r][j] * rs_invk, var = sum_j rs_ssq[r][j] * rs_invk - mean^2,
  //             and the GELU'd factor's pre-activation becomes rsqrt(var + rs_eps) * (A.W'^T - mean * rs_c[n]) + bias[n], where W' = W diag(gamma) is
  //             what the caller packed, rs_c[n] = sum_k W'[n][k] (of the ROUNDED operand values) and bias[n] = sum_k beta[k] W[n][k] (+ the layer's bias);
  //             the plain multiplier factor is untouched. rs_c is indexed like bias (pair32: the interleaved column space).
  float* sum_out = nullptr;
  const float* rs_sum = nullptr;
  const float* rs_c = nullptr;
  // split-K scratch (fp32 [S][M][N] partial products) for grids that would leave most CUs idle; size it with
  // gemm_splitk_bytes(). Without it the launch is a single pass.
  float* splitk_ws = nullptr;
  size_t splitk_ws_bytes = 0;
  const Tuning* tune = nullptr;   // the calling handle's knobs (nullptr: process defaults)
  // out (profiling): which kernel the launcher chose = kind * 1000 + (act + 1) * 10 + epi ; kind 1 gemm_pp_kernel,
  // 2 gemm_persistent_kernel, 3 gemm_wide_kernel, 4..7 gemm_kernel with the 256x256 / 128x128 / 64x64 / 32x64 tile (epi 0),
  // 8 two-pass split-K, 10 / 11 / 12 gemm_resident_kernel with the 32x32 / 64x32 / 64x64 tile, 15 / 16 its DUAL (GEGLU pair) form on the 32x32 / 64x64 tile,
  // 17 / 18 gemm_skinny_kernel (M <= 32) / its DUAL form, 19 / 20 gemm_q4_kernel, 21 gemm_kernel<float, ..., X3> (128x128 tile), 23 two-pass split-K over it
  int* kernel_id = nullptr;
  // precision "bf16x3" (fp32 operands only): the products run in split-bf16 on gemm_kernel<float, ..., X3> -- each fp32 operand is hi + lo
  // (two bf16), a.b ~ hi_a.hi_b + hi_a.lo_b + lo_a.hi_b on v_mfma_f32_32x32x16_bf16 -- instead of v_mfma_f32_32x32x2_f32.
  // Same tiles, epilogues and split-K plan as the fp32 path.
  int x3 = 0;
  // fp8 weights (precision "fp8w", bf16 activations): W is [N,K] OCP e4m3 BYTES (ldw / bsW in elements = bytes) and
  // wscale[n] the per-output-channel dequantisation scale; the kernel widens the fragments to bf16 in registers and
  // multiplies accumulator column n by wscale[n] before bias / activation. Needs N % 4 == 0, K % 64 == 0, batch 1.
  int w8 = 0;
  const float* wscale = nullptr;
  // fp8 ACTIVATIONS (precision "fp8"): with a8 = 1, A is [M,K] OCP e4m3 BYTES as well (lda in bytes) with ONE dequantisation scale
  // `ascale` for the tensor; both operands go to v_mfma_scale_f32_32x32x64_f8f6f4 (gemm_pp_kernel<.., F8>: needs w8, K % 256 == 0 and
  // the persistent-kernel shape conditions; anything else fails), the accumulator column is multiplied by wscale[n] * ascale.
  int a8 = 0;
  float ascale = 1.0f;
  // optional fp8 copy of the result for an fp8 consumer: out8[r][n] = e4m3(value * out8_inv) (saturating), row stride ld8 BYTES;
  // bf16-only-output and bf16-stream epilogues of the persistent kernels. With out8 the bf16 output outT may be omitted.
  void* out8 = nullptr;
  int ld8 = 0;
  float out8_inv = 1.0f;
};

}  // namespace vima
