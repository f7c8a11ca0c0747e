/* vima_hip.h -- C ABI of the MI355X-native (gfx950) VIMA policy forward pass.
 *
 * The reference (vimalabs/VIMA) is pure Python: it has no FFI of its own, its seam is the method surface of
 * `VIMAPolicy` (vima/policy/vima_policy.py:11-322) and the checkpoint contract of `create_policy_from_ckpt`
 * (vima/__init__.py:7-16). This library is what a binding for that seam binds to: one opaque handle per
 * (model, device) and one entry point per policy method. All tensors are plain device pointers owned by the
 * caller (row-major, contiguous unless strides are given); the library never frees caller memory, launches on
 * the caller's hipStream_t and keeps its own workspace. Every function returns 0 on success, otherwise an error
 * code whose text is available from vima_last_error(). The Python host side (vima_amd/policy.py) loads this
 * library with ctypes; INTEGRATION.md shows the binding.
 *
 * Conventions: f32 = float, i64 = int64_t, u8 = uint8_t (also used for torch.bool). Views are ordered
 * sorted(["front","top"]) = {front, top} (obj_encoder.py:31). E = embed_dim.
 */
#ifndef VIMA_HIP_H
#define VIMA_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct VimaHandle VimaHandle;
typedef void* vima_stream_t; /* hipStream_t */

/* FP8W (BASELINE.json configs[4]): bf16 activations and bf16 matrix instructions, but the weights of the large Linear
 * layers are stored as OCP FP8 E4M3 with one fp32 scale per output channel (half the weight bytes in HBM / L2 / LDS);
 * the GEMM kernels widen the fp8 fragments to bf16 in registers. Logit error vs the fp32 reference is a few 1e-3 (weights
 * only carry 3 mantissa bits) -- measured and reported by the tests, not covered by the 1e-3 gate of the bf16 mode. */
enum { VIMA_PRECISION_FP32 = 0, VIMA_PRECISION_BF16 = 1, VIMA_PRECISION_FP8W = 2, VIMA_PRECISION_FP8 = 3, VIMA_PRECISION_BF16X3 = 4 };
/* BF16X3: storage and every non-matrix kernel exactly as FP32 (fp32 operands, fp32 streams, fp32 LayerNorm / softmax statistics);
 * the matrix products run in split-bf16: each fp32 operand is written x = hi + lo with hi = bf16(x), lo = bf16(x - hi) (round to
 * nearest even) and a.b ~ hi_a.hi_b + hi_a.lo_b + lo_a.hi_b on three v_mfma_f32_32x32x16_bf16 with fp32 accumulation (about 3 x 2^-18
 * relative error per product against 2^-8 for bf16; 3/16 of the cost of the fp32 matrix instruction). Every GEMM runs on
 * gemm_kernel<float, ..., X3> (kinds 21 / 23 of vima_prof_read_gemm_kernels); attention with impl 1 and head dim 32 / 64 on attn_mfma_kernel<D, MODE, X3>, other
 * head dims on the exact generic kernel. The 5-token ViT attention is the fp32 kernel. ABI version unchanged (additive). */
/* FP8W: bf16 activations and matrix instruction, OCP e4m3 weights (+ one fp32 scale per output channel) for the large Linear layers.
 * FP8 : FP8W plus e4m3 ACTIVATIONS into the large GEMMs of the T5 stack, the ViT and the decoder's prompt K/V projection (one static
 *       scale per layer and site, calibrated by the handle's first pass through each, which runs the FP8W kernels) on
 *       v_mfma_scale_f32_32x32x64_f8f6f4 -- BASELINE.json configs[4]. Shapes the fp8 kernel does not cover, and handles whose kernel-
 *       selection options leave that kernel unreachable (gemm_persist = 0, gemm_tile = 1, gemm_raster != 0, gemm_epi = 0, operands beyond the
 *       32-bit LDS-DMA offsets), keep bf16 activations; no documented option makes a forward fail.
 *       CALIBRATION CONTRACT: the scales are STATIC and come from the first eligible pass of each group, so (i) that first call runs the
 *       FP8W kernels and the SAME input gives (slightly) different outputs on call 1 and on call 2 -- warm a handle up once on
 *       representative data before comparing or serving; (ii) scale = headroom x max |x| / 448 with option "fp8_headroom_pct" (default 125):
 *       later activations up to 1.25x the calibrating maximum stay representable, larger ones SATURATE at +-448 x scale silently (call
 *       "fp8_recalibrate" when the input distribution changes); (iii) a calibrating batch that holds an inf / NaN activation is refused
 *       (the call fails, nothing is frozen: max |x| is taken over the magnitude bit patterns, where every NaN orders above inf). A NaN
 *       AFTER calibration is NOT detected: fmed3(NaN, -448, 448) is -448, so every e4m3 producer turns a NaN activation into the byte
 *       0xFE (-448) silently (vima_op_fp8_quant; tests/test_fp8_producers_gpu.py pins the byte); (iv) vima_decode_restart rebuilds the restarted samples' prompt K/V rows with bf16
 *       activations (M = Lp rows is below the fp8 kernel's size), i.e. a restarted sample matches a fresh episode to the fp8 tolerance, not
 *       bit for bit. */

/* Which policy class of vima/policy/ the handle implements. VIMA is the hot path (vima_policy.py); the other three are the
 * reference's baseline policies, which consume whole 64x128 RGB frames instead of object crops:
 *   GPT      VIMAGPTPolicy      (vima_gpt_policy.py): cls feature of a rectangular ViT per view, decoder-only HFGPT over
 *                                [prompt | sep | obs, action, obs, ...]
 *   GATO     VIMAGatoPolicy     (vima_gato_policy.py): the 2 x 8 patch tokens of every frame pair go into the same sequence
 *   FLAMINGO VIMAFlamingoPolicy (vima_flamingo_policy.py): patch tokens resampled to 4 latents by a Perceiver, then XAttnGPT
 * For them xf_n_layers / sattn_n_heads are the constructor's n_layer / n_head (dt_n_layers / dt_n_heads); xattn_n_heads is
 * only used by FLAMINGO (pass n_head otherwise). */
enum { VIMA_POLICY_VIMA = 0, VIMA_POLICY_GPT = 1, VIMA_POLICY_GATO = 2, VIMA_POLICY_FLAMINGO = 3 };

/* Constructor arguments of VIMAPolicy (vima_policy.py:12-19) plus the two table sizes the reference hard-codes
 * (xattn_n_positions=256 at vima_policy.py:30, n_positions=512 at xattn_gpt.py:18). */
typedef struct VimaConfig {
  int32_t embed_dim;
  int32_t xf_n_layers;
  int32_t sattn_n_heads;
  int32_t xattn_n_heads;
  int32_t xattn_n_positions;
  int32_t n_positions;
  int32_t precision; /* VIMA_PRECISION_*: operand type T of the matrix-core GEMMs / attention. Accumulation, LayerNorm /
                        RMSNorm and softmax statistics are always fp32; the DECODER's residual stream is fp32; the residual
                        streams of the T5 stack and of the ViT are carried in T as well when option "stream_T" is 1 (the
                        default: bf16 streams in the BF16 / FP8W precisions, fp32 in FP32) and in fp32 when it is 0. */
  int32_t policy_kind; /* VIMA_POLICY_* (ABI version 3; 0 = VIMAPolicy) */
} VimaConfig;

/* ---- lifetime ------------------------------------------------------------------------------------------------ */
/* replaces VIMAPolicy.__init__ (vima_policy.py:12-114) */
int vima_create(const VimaConfig* cfg, int device, VimaHandle** out);
void vima_destroy(VimaHandle* h);
const char* vima_last_error(void);
/* 2: + vima_crop_objects, vima_comm_*, vima_allgather_logits, vima_prof_read_ex, precision fp8w; 3: + VimaConfig.policy_kind and the
 * baseline-policy entry points; 4: + VIMA_PRECISION_FP8, vima_fp8_act_scales, vima_decode_restart, vima_prof_read_gemm_kernels;
 * 5: + vima_prof_read_gemm_launches, option "fp8_headroom_pct".
 * The ONE place the number lives: the library returns it, the ctypes binding parses it from this header and refuses a mismatch. */
#define VIMA_ABI_VERSION 5
int vima_abi_version(void);

/* ---- weights: the reference checkpoint contract -------------------------------------------------------------- */
/* replaces nn.Module.load_state_dict(strict=True) as used by create_policy_from_ckpt (vima/__init__.py:11-14).
 * `name` is the reference state_dict key, `data` a HOST fp32 array in the reference's own
 * layout (HF Conv1D weights are [in,out], nn.Linear [out,in] -- the library repacks). Integer buffers of the
 * reference state_dict (position_ids, attn.bias, ...) carry no information and are not passed. */
int vima_set_param(VimaHandle* h, const char* name, const float* data, const int64_t* shape, int ndim);
/* Packs / converts / uploads; fails (strict) listing any key that was never set or has the wrong shape. */
int vima_finalize_params(VimaHandle* h);
/* Host-only (no GPU needed): writes the NUL-separated list of state_dict keys vima_finalize_params requires for
 * this config into buf (when it fits) and returns the number of bytes needed. */
int64_t vima_required_params(const VimaConfig* cfg, char* buf, int64_t buflen);

/* ---- policy methods ------------------------------------------------------------------------------------------ */
/* ObjEncoder.forward (obj_encoder.py:66-95): crops[v] u8 [n,Qv,3,32,32], bbox[v] i64 [n,Qv,4] (xc,yc,h,w px)
 * -> out f32 [n, 2*Qv, E] with the object axis ordered [front objs..., top objs...]. */
int vima_obj_encode(VimaHandle* h, const uint8_t* const crops[2], const int64_t* const bbox[2], int n, int qv,
                    float* out, vima_stream_t stream);

/* VIMAPolicy.forward_obs_token (vima_policy.py:242-259): leading dims [T,B] flattened to n = T*B.
 * mask[v] u8 [n,Qv]; ee i64 [n] in {0,1} -> out_tokens f32 [n, 2*Qv, E], out_mask u8 [n, 2*Qv]. */
int vima_obs_encode(VimaHandle* h, const uint8_t* const crops[2], const int64_t* const bbox[2],
                    const uint8_t* const mask[2], const int64_t* ee, int n, int qv, float* out_tokens,
                    uint8_t* out_mask, vima_stream_t stream);

/* VIMAPolicy.forward_prompt_assembly (vima_policy.py:161-240). The python double loop over token types is replaced
 * by an index array built on the host: tok_src i32 [B*Lp] (device), one code per (b, l):
 *     >= 0 : index into word_ids            (word token, mask True)
 *     -1   : padding                        (zeros, mask False)
 *     <= -2: object token -(code+2) = img*2*Qv + q of the encoded prompt images (mask = object mask)
 * word_ids i64 [n_words]; crops/bbox/mask as above with n = n_img.
 * -> out_tokens f32 [B, Lp, E] (batch-first; the reference returns the [Lp,B,E] transposed view of it),
 *    out_mask u8 [B, Lp]. */
int vima_prompt_encode(VimaHandle* h, const int64_t* word_ids, int n_words, const uint8_t* const crops[2],
                       const int64_t* const bbox[2], const uint8_t* const mask[2], int n_img, int qv,
                       const int32_t* tok_src, int B, int Lp, float* out_tokens, uint8_t* out_mask,
                       vima_stream_t stream);

/* T5PromptEncoder.forward (prompt_encoder.py:30-58) on already assembled embeddings x f32 [B,L,768], mask u8 [B,L]
 * -> out f32 [B,L,768] (before t5_prompt_encoder_post_layer). Exposed for operator-level parity tests. */
int vima_t5_encode(VimaHandle* h, const float* x, const uint8_t* mask, int B, int L, float* out,
                   vima_stream_t stream);

/* VIMAPolicy.forward (vima_policy.py:116-159) -> XAttnGPT.forward (xattn_gpt.py:73-139).
 * obs_tok f32 [T,B,Q,E], obs_mask u8 [T,B,Q], act_tok f32 [L_act,B,E] or NULL (L_act in {T-1, T}),
 * prompt f32 element (b,l,e) at prompt[b*stride_b + l*stride_l + e] (so both the [B,Lp,E] buffer and the reference's
 * sequence-first [Lp,B,E] layout can be passed), prompt_mask u8 [B,Lp] -> out f32 [T,B,E] (sequence-first).
 * kv_cache_mode: the per-layer prompt K/V projection (components.py:175) is loop-invariant over the env steps of an
 * episode. 0 = stateless (recompute, like the reference); 1 = compute it into the handle's
 * cache and use it; 2 = reuse the cache of the last mode-1 call (same B, Lp; `prompt` is not read). Outputs are
 * bit-identical in all three modes. */
int vima_decode(VimaHandle* h, const float* obs_tok, const uint8_t* obs_mask, const float* act_tok, int T, int B,
                int Q, int L_act, const float* prompt, int64_t stride_b, int64_t stride_l,
                const uint8_t* prompt_mask, int Lp, int kv_cache_mode, float* out, vima_stream_t stream);

/* Incremental form of vima_decode for the env-step loop of an episode (scripts/example.py:135-190 re-feeds the whole
 * history every step): call with step = 0, 1, 2, ... and only the NEWEST tokens -- obs_tok f32
 * [B,Q,E] / obs_mask u8 [B,Q] of env step `step` and, for step > 0, act_tok f32 [B,E] = the embedded action of step-1.
 * The handle keeps the per-layer prompt K/V (built at step 0, so `prompt` must be valid there) and the self-attention
 * K/V, key mask and position counters of the history. out f32 [B,E] = the predicted action token of this step, equal
 * (up to floating-point reassociation) to row `step` of vima_decode on the full history. step 0 starts a new
 * episode; any other step must follow step-1 with the same B, Q, Lp.
 * The histories of the B samples share ONE row index space of n_positions rows: step s writes rows s (Q + 1) - 1 .. of every sample, so a batch
 * takes (n_positions + 1) / (Q + 1) steps after its step 0 (code 34 beyond), restarts or not.
 * Option "decode_ring" = 1 turns that row space into a ring, for batches that never stop (vectorised environments). `step` keeps its meaning
 * (previous + 1) and is unbounded.
 * THE ROW BOOKKEEPING of this ring and of option "seq_ring" of the decoder-only policies (vima_seq_decode_restart below) is one piece of host
 * code (vima_amd/csrc/episode_book.h): rows [0, P0) are a fixed prefix (P0 = 0 here, P0 = Lp + 1 there), rows [P0, n_positions) the ring of
 * R = n_positions - P0 rows. The host keeps wp (next row), hw (one past the highest row written since step 0 / the prefill, both = P0 there) and
 * age[b] (ring rows advanced since sample b's episode began, 0 there). A call of Lq rows (Q at step 0 of the batch, Q + 1 afterwards, T times as
 * many for a chunk) goes to row = wp and advances Lq rows, or, when wp + Lq > n_positions, to row = P0 and advances n_positions - wp + Lq rows
 * (the tail is skipped: a call's rows are never split). It is legal iff every row it overwrites or skips is dead for every sample:
 * age[b] + advance <= R; otherwise it fails with code 34, names the first such sample, changes nothing, and succeeds once that sample has been
 * restarted (a restart sets age[b] = 0 and takes no rows; vima_decode_steps_left tells in advance). On success age[b] += advance, wp = row + Lq,
 * hw = max(hw, wp). A sample's own episode is thus still bounded by n_positions tokens, the position table and the reference's limit. The self-attention reads the written part of the ring with a WINDOWED causal rule (key j is
 * "future" for the step's query i iff i + write pointer < j < write pointer + Q + 1; the rows behind the window hold older history): the
 * predictions of a sample depend on its own episode only and equal those of the linear cache up to the order of the softmax sums. With
 * option "graphs" the captured graphs are keyed on (write pointer, rows read, action slot), and one eager step warms them all; the set stops growing once the
 * high-water mark of the ring has stopped moving (during the third lap). */
int vima_decode_step(VimaHandle* h, const float* obs_tok, const uint8_t* obs_mask, const float* act_tok, int step, int B,
                     int Q, const float* prompt, int64_t stride_b, int64_t stride_l, const uint8_t* prompt_mask,
                     int Lp, float* out, vima_stream_t stream);
/* Multi-step prefill of the episode caches (additive, ABI version unchanged): the T calls vima_decode_step(step), ..., (step + T - 1) made as
 * ONE pass -- resuming an interrupted rollout, switching from vima_decode to vima_decode_step mid-episode, teacher-forced scoring of a recorded
 * prefix that leaves the caches filled. obs_tok f32 [T,B,Q,E], obs_mask u8 [T,B,Q], out f32 [T,B,E]; act_tok f32 [T,B,E] when step > 0 (row 0
 * = the embedded action of step-1, row j = that of step+j-1) and f32 [T-1,B,E] when step == 0 (row j = the action of step j; NULL for T = 1).
 * out[j] equals row step+j of vima_decode on the full history up to floating-point reassociation. Afterwards the episode state is that of the
 * T single calls: the next call carries step + T, key mask / position counters / restart flags are the same (a sample restarted right before
 * the chunk has the chunk's FIRST action slot masked, as in a single step).
 * Rows: the chunk's T (Q + 1) rows (T (Q + 1) - 1 at step 0; at most 512) are contiguous; step u's slot is [action row, Q obs rows] at
 * row0 + u (Q + 1) (no action row in the first slot of batch step 0). Without "decode_ring" they are the rows the T single steps would have
 * written; a chunk that does not fit in front of n_positions fails with code 34, tells how many steps still fit, and changes nothing. With
 * "decode_ring" the chunk is ONE unit of the ring: never split, the tail is skipped when it does not fit, legal iff
 * age[b] + rows advanced <= n_positions for every b -- otherwise code 34, the first such sample is named, nothing changes (so a chunk can be
 * refused where single steps would still pass: the skipped tail is longer). The chunk's own rows are causal among themselves, everything else
 * written is history (the windowed rule above with the window = the chunk's rows).
 * T == 1 IS vima_decode_step (same code, same bits, same graph keys). With option "graphs" a chunk of T > 1 runs eager; the graphs of
 * vima_decode_step stay valid and keep being replayed afterwards. Launches: those of ONE step whatever T (give or take a GEMM form
 * that runs as two launches at the larger row count: 135 -> 157 at 11 layers, batch 256, T >= 8).
 * Precision: no precision-specific code; in fp8 / fp8w the call runs the GEMM forms vima_decode_step runs at T (Q + 1) B rows. */
int vima_decode_chunk(VimaHandle* h, const float* obs_tok, const uint8_t* obs_mask, const float* act_tok, int step, int T, int B,
                      int Q, const float* prompt, int64_t stride_b, int64_t stride_l, const uint8_t* prompt_mask, int Lp,
                      float* out, vima_stream_t stream);
/* Per-sample episode restart inside a running batch of incremental decoding (no reference counterpart: scripts/example.py:97-110 runs
 * one episode at a time; batched environments end their episodes at different steps). For every sample with restart[b] != 0 (HOST
 * array of B bytes): its cached history is masked out, its position counter restarts at 0, its next step has no previous action, and
 * its rows of the per-layer prompt K/V cache are rebuilt from ITS row of `prompt` / `prompt_mask` (the new episode's prompt; layout and
 * strides as in vima_decode_step; rows of the other samples are not read). The batch then keeps calling vima_decode_step with
 * step + 1 (pass any act_tok row for restarted samples: it is ignored). n_positions still bounds the steps since the batch's step 0,
 * except with option "decode_ring", where the restart also returns the sample's rows to the ring (its age restarts at 0).
 * The flagged samples' prompt K/V are rebuilt TOGETHER (option "restart_batched", prompts of more than 32 tokens): one gather of their
 * prompts, one GEMM of n_flagged x Lp rows and one scatter per layer, 2 + 2 x layers launches whatever the number of flagged samples; the
 * cache receives the bits of the per-sample loop (option 0). */
int vima_decode_restart(VimaHandle* h, const uint8_t* restart, int B, const float* prompt, int64_t stride_b, int64_t stride_l,
                        const uint8_t* prompt_mask, int Lp, vima_stream_t stream);

/* Restart with a history (additive, ABI version unchanged): everything vima_decode_restart does for the flagged samples, then T env steps of
 * history are installed for each of them, so that an in-flight episode can JOIN a running batch (re-balancing vectorised environments over
 * handles, merging half-empty batches, resuming single episodes). hist_obs f32 [T,n_r,Q,E], hist_mask u8 [T,n_r,Q], hist_act f32 [T-1,n_r,E]
 * (NULL for T = 1): the observation tokens of the sample's steps 0 .. T-1 and the embedded actions of steps 0 .. T-2; n_r = the number of flagged
 * samples, in increasing sample order; all samples flagged in one call share T (ragged histories: one call per length). T == 0 IS
 * vima_decode_restart, bit for bit. out (may be NULL): f32 [T,n_r,E], the predicted action tokens of the installed steps (the teacher-forced
 * pass; it costs nothing extra). Afterwards the sample is mid-episode: its next vima_decode_step consumes its row of act_tok (= the action of
 * history step T-1), its outputs equal vima_decode on (history + later steps) at the matching rows up to reassociation, its position ids continue
 * from the history's number of valid tokens. The state of every other sample is untouched (their later outputs keep their bits).
 * Placement: history step s takes the cache rows that BATCH step t-T+s wrote (t = the next batch step): its Q obs rows that slot's obs rows,
 * a_{s-1} its action row (s > 0; the first slot's action row stays masked). With "decode_ring" the sample's age becomes exactly that of a sample
 * restarted right before batch step t-T, and so does its vima_decode_steps_left entry. T may be at most vima_decode_history_room (below);
 * beyond it the call fails with code 34, the message names the room, and NOTHING changes (no restart either).
 * The history runs as one full-history pass over the n_r samples (plain causal attention under the history's own mask, against the prompt K/V
 * this call has just rebuilt); per layer its K | V rows are scattered to the mapped rows. On top of the restart's launches: those of ONE vima_decode
 * pass plus 2 + 2 x layers (the prompt-mask gather, per layer the prompt K/V gather and the K | V scatter, the install), whatever n_r
 * (the restart's own count depends on n_r for prompts of at most 32 tokens, see above). T (Q + 1) - 1 <= min(512, n_positions). Runs eager also with option "graphs"; the step graphs stay valid.
 * Precision: no precision-specific code; in fp8 / fp8w the pass runs the GEMM forms vima_decode runs at n_r (T (Q + 1) - 1) rows. */
int vima_decode_restart_history(VimaHandle* h, const uint8_t* restart, int B, const float* prompt, int64_t stride_b, int64_t stride_l,
                                const uint8_t* prompt_mask, int Lp, const float* hist_obs, const uint8_t* hist_mask,
                                const float* hist_act, int T, float* out, vima_stream_t stream);
/* Host-only: *steps_host = the largest T vima_decode_restart_history accepts now = the number of most recent batch steps whose cache rows are all
 * still there. Without "decode_ring": the batch steps taken since step 0. With it: the largest R such that the ring rows advanced by the last R
 * batch steps (skipped tails included; a chunk's tail counts with its first step) sum to at most n_positions. */
int vima_decode_history_room(VimaHandle* h, int32_t* steps_host);

/* Host-only (additive, ABI version unchanged): out_host[b], b < B = how many further vima_decode_step calls of the running episode batch would
 * succeed if sample b ALONE were never restarted again (the row bookkeeping of vima_decode_step run forward; no device work, no state change).
 * Without option "decode_ring" the number is the same for every sample: the steps left before the whole batch must start over.
 * On a GPT / GATO handle the call reports the episode of vima_seq_prefill / vima_seq_decode_step: every entry is
 * floor((n_positions - rows used) / (Q + 1)) (before step 0, which feeds Q rows only: floor((n_positions - rows used + 1) / (Q + 1))).
 * With option "seq_ring" the ring bookkeeping of vima_seq_decode_step is run forward per sample, as with "decode_ring" above. */
int vima_decode_steps_left(VimaHandle* h, int B, int32_t* out_host);

/* VIMAPolicy.forward_action_decoder (vima_policy.py:264-265 -> action_decoder.py:51-52,165-166): tokens f32 [R,E]
 * -> raw logits f32 [R,700] = concat over keys (pose0_position, pose0_rotation, pose1_position, pose1_rotation) of
 * the 12 MLP outputs. The distribution over them (dists.py MultiCategorical: mode / sample / log_prob / entropy) is available on
 * the device from vima_action_select and vima_act below; the Python MultiCategorical wrapper of forward_action_decoder remains
 * as the reference's host-side interface. */
int vima_action_head(VimaHandle* h, const float* tokens, int R, float* out_logits, vima_stream_t stream);

/* VIMAPolicy.forward_action_token (vima_policy.py:261-262 -> :301-322 -> action_embd.py:29-56): discrete bin
 * indices i64, keys in sorted order: pose0_position [R,2], pose0_rotation [R,4], pose1_position [R,2],
 * pose1_rotation [R,4] -> out f32 [R,E]. */
int vima_action_embed(VimaHandle* h, const int64_t* const idx[4], int R, float* out, vima_stream_t stream);

/* Action selection on the device (additive, ABI version unchanged): what the eval loop does between the logits and env.step
 * (MultiCategorical.mode / sample / log_prob / entropy, dists.py:7-28; _de_discretize_actions, vima_policy.py:301-322; the rescaling to
 * the task's action bounds, scripts/example.py:213-234) as ONE launch of act_select_kernel, one workgroup per row. No handle: there
 * are no weights involved. logits f32 [R,700] (the layout of vima_action_head); the 12 segments are (50,100 | 50 x4 | 50,100 | 50 x4).
 *   u       f32 [R,12] uniforms or NULL. NULL: every bin is the mode = the FIRST index of the segment's maximum (torch.argmax of the
 *           logits, exact comparisons). Otherwise the inverse-CDF sample: bin = number of bins whose inclusive cumulative probability
 *           cumsum(exp(x - max)) / sum (fp32) is <= clamp(u, [0, 1)), clamped to n - 1. Bins are always in [0, n), whatever the logits hold.
 *   bounds  HOST float[4] = {low[0], low[1], high[0], high[1]} of the position keys (meta["action_bounds"]) or NULL; read during the call.
 *   idx     four DEVICE arrays i64 [R,2], [R,4], [R,2], [R,4] (required): the bins, exactly what vima_action_embed takes.
 *   cont    f32 [R,12] or NULL: (float)bin / n_bins (division by 50 / 100 like _de_discretize_actions); with bounds, positions
 *           clamp(x * (high - low) + low, low, high) and rotations clamp(x * 2 - 1, -1, 1), every operation rounded to fp32 on its own
 *           (no fused multiply-add), i.e. the values of the torch expressions of the reference loop, bit for bit.
 *   log_prob, entropy  f32 [R,4] or NULL: per key, summed over the key's 2 / 4 dimensions (MultiCategorical.log_prob(bins) / .entropy());
 *           log p = x - (max + log sum exp(x - max)). */
int vima_action_select(const float* logits, int R, const float* u, const float* bounds, int64_t* const idx[4], float* cont,
                       float* log_prob, float* entropy, vima_stream_t stream);

/* One call from the predicted action tokens to everything the env-step loop needs, without host synchronisation: the launches of
 * vima_action_head (tokens f32 [R,E] -> logits, bit-equal; written to logits_out f32 [R,700] when it is not NULL), then
 * act_select_kernel as in vima_action_select (u, bounds, idx, cont, log_prob, entropy as above) which also computes the first layer
 * of the action embedding from the bins it chose, then the rest of vima_action_embed (the batched 4 x (256 -> 256) GEMM and the post
 * layer; identity for E = 1024) -> token f32 [R,E], bit-identical to vima_action_embed on idx. token NULL skips the embedding.
 * Every policy_kind and precision. With option "graphs" the call is captured like the two it chains: the key holds every pointer and
 * the VALUES of the bounds; u is read from device memory at replay, so new uniforms written in place take effect. */
int vima_act(VimaHandle* h, const float* tokens, int R, const float* u, const float* bounds, float* logits_out, int64_t* const idx[4],
             float* cont, float* log_prob, float* entropy, float* token, vima_stream_t stream);

/* Sampling controls and action scoring for the two calls above (additive, ABI version unchanged). opts NULL = all defaults. Per row r
 * of logits, per sample s < n_samples and per segment of n bins:
 *   temperature  DEVICE f32 [R], one per row of LOGITS, or NULL = 1. z = x / T, one correctly rounded fp32 division per element; T is
 *                clamped to [1e-4, 1e4] and a NaN is 1, so z is finite for finite logits. Read from device memory during the launch.
 *   top_k        rank(i) = #{j : z_j > z_i} + #{j < i : z_j == z_i} (exact comparisons, ties to the lower index); bin i survives iff
 *                rank(i) < top_k. <= 0 or >= n keeps every bin; one value for all segments, so 50 truncates only the 100-bin heads.
 *   top_p        after top_k: q = softmax(z) over the survivors; the bin of rank r survives iff the mass of the surviving bins of
 *                rank < r is < top_p (rank 0 always survives). >= 1: off; must be > 0.
 *   n_samples    S >= 1 candidates per row of logits: OUTPUT row r * S + s is sample s of logits row r. Every output and u have R * S rows.
 *   given        idx are INPUTS (i64, clamped to [0, n), left as they are): nothing is selected, u is ignored, and cont, log_prob,
 *                entropy (and the token of vima_act_ex) are computed for those bins. Requires n_samples == 1.
 * The kept set K defines pi = softmax(z) over K and 0 elsewhere; log pi = z - (max_K z + log sum_K exp(z - max_K z)) on K, -inf
 * outside (only a given bin can be outside). u NULL selects the first index of the segment's maximum, whatever the filters; otherwise
 * the inverse CDF of vima_action_select runs over pi in bin order, and a result outside K (possible through rounding at the upper end
 * only) becomes the last bin of K at or below it. log_prob and entropy describe pi, per key as above. */
typedef struct VimaSampleOpts {
  const float* temperature; /* DEVICE f32 [R] or NULL */
  int top_k;                /* <= 0: off */
  float top_p;              /* >= 1: off; must be > 0 */
  int n_samples;            /* S >= 1 */
  int given;                /* idx are inputs */
} VimaSampleOpts;

/* vima_action_select with VimaSampleOpts: ONE launch of act_sample_kernel (vima_amd/csrc/action_sample.hip), one workgroup per output
 * row; logits f32 [R,700], u f32 [R*S,12] or NULL, idx / cont / log_prob / entropy with R*S rows. With opts NULL (or temperature NULL,
 * top_k <= 0, top_p >= 1, n_samples 1, given 0) every output equals vima_action_select's, bit for bit. Refused before any launch:
 * top_p <= 0 or NaN, n_samples < 1, given with n_samples != 1, null idx. */
int vima_action_select_ex(const float* logits, int R, const float* u, const VimaSampleOpts* opts, const float* bounds,
                          int64_t* const idx[4], float* cont, float* log_prob, float* entropy, vima_stream_t stream);

/* vima_act with VimaSampleOpts: the launches of vima_action_head on R rows (tokens f32 [R,E]; logits_out f32 [R,700] or NULL), then
 * act_sample_kernel on R*S rows, then the rest of vima_action_embed on R*S rows -> token f32 [R*S,E] (NULL skips it), bit-identical to
 * vima_action_embed on the chosen (or given) bins. Every policy_kind and precision; the refusals of vima_action_select_ex. With option
 * "graphs" it is captured like vima_act: the key holds every pointer, R, S, top_k, the bits of top_p, given and the VALUES of the
 * bounds; u and temperature are read from device memory at replay, so new values written in place take effect. */
int vima_act_ex(VimaHandle* h, const float* tokens, int R, const float* u, const VimaSampleOpts* opts, const float* bounds,
                float* logits_out, int64_t* const idx[4], float* cont, float* log_prob, float* entropy, float* token,
                vima_stream_t stream);

/* ---- baseline policies (policy_kind != VIMA_POLICY_VIMA) ---------------------------------------- */
/* Tokens one frame pair contributes: Q = 1 (GPT), 16 (GATO: 8 patches x 2 views), 4 (FLAMINGO: Perceiver latents); feature
 * width of obj_encoder's output Eo = 2E (GPT: views concatenated on the feature axis, obj_encoder.py:232-245) or E. */
int vima_rgb_tokens_per_image(const VimaConfig* cfg);
/* obj_encoder.forward of the handle's policy (MultiViewRGBEncoder obj_encoder.py:207-246, GatoMultiViewRGBEncoder :98-145,
 * MultiViewRGBPerceiverEncoder :148-204): rgb[v] u8 [n,3,64,128] -> out f32 [n, Q, Eo]. */
int vima_rgb_encode(VimaHandle* h, const uint8_t* const rgb[2], int n, float* out, vima_stream_t stream);
/* forward_obs_token (vima_gpt_policy.py:249-259, vima_gato_policy.py:253-264, vima_flamingo_policy.py:216-227): leading dims
 * [T,B] flattened to n; ee i64 [n] in {0,1} -> out f32 [n, Q, E] (GPT: Q = 1, the reference returns [T,B,E]). */
int vima_rgb_obs_encode(VimaHandle* h, const uint8_t* const rgb[2], const int64_t* ee, int n, float* out, vima_stream_t stream);
/* forward_prompt_assembly (vima_gpt_policy.py:189-247, vima_gato_policy.py:190-251, vima_flamingo_policy.py:156-214): like
 * vima_prompt_encode with whole frames: tok_src codes >= 0 word index, -1 padding, <= -2 image token -(code+2) = img*Q + q;
 * every assembled token is valid (these policies have no object masks). -> out_tokens f32 [B,Lp,E], out_mask u8 [B,Lp]. */
int vima_rgb_prompt_encode(VimaHandle* h, const int64_t* word_ids, int n_words, const uint8_t* const rgb[2], int n_img,
                           const int32_t* tok_src, int B, int Lp, float* out_tokens, uint8_t* out_mask, vima_stream_t stream);
/* VIMAGPTPolicy.forward / VIMAGatoPolicy.forward (vima_gpt_policy.py:118-187, vima_gato_policy.py:115-188) -> HFGPT.forward
 * (gpt/gpt.py:45-80): sequence [prompt (Lp) | prompt_sep_token | o_1..o_Q, a, o_1..o_Q, a, ...] per sample, key mask = prompt
 * mask then ones, position ids continuing after the sample's valid prompt tokens. obs_tok f32 [T,B,Q,E], act_tok f32
 * [L_act,B,E] or NULL (L_act in {T-1, T}), prompt/strides/mask as in vima_decode -> out f32 [T,B,E].
 * (VIMAFlamingoPolicy.forward is vima_decode with an all-ones obs_mask.) */
int vima_seq_decode(VimaHandle* h, const float* obs_tok, const float* act_tok, int T, int B, int L_act, const float* prompt,
                    int64_t stride_b, int64_t stride_l, const uint8_t* prompt_mask, int Lp, float* out, vima_stream_t stream);

/* ---- incremental decoding of the decoder-only policies (additive, ABI version unchanged; VIMA_POLICY_GPT / VIMA_POLICY_GATO handles only,
 * every other kind fails; option "decode_ring" is refused here: the ring of these policies is option "seq_ring", below) -----------------
 * The rollout form of vima_seq_decode: the prompt is a sequence PREFIX that is consumed once, every env step then feeds only its own rows
 * against a per-layer K | V cache [B][n_positions][2E] in the handle. HFGPT blocks are post-LN and act per row and the attention is causal,
 * so the cached prefix is exact: step t returns row t of vima_seq_decode on the whole history (L_act = T - 1) up to summation order.
 *
 * vima_seq_prefill starts an episode batch: rows [0, Lp] ([prompt | prompt_sep_token], position ids min(l, nv - 1) / nv with nv = the
 * sample's valid prompt tokens) go through the stack, every layer's K | V are left in rows [0, Lp] of the cache (copied from the call's
 * dense q | k | v, which its attention reads), the key mask (prompt mask, 1 for the separator) and the per-sample position base nv + 1
 * are stored. prompt / strides / mask as in vima_decode. Fails with code 34 when Lp + 1 > n_positions. */
int vima_seq_prefill(VimaHandle* h, const float* prompt, int64_t stride_b, int64_t stride_l, const uint8_t* prompt_mask, int B, int Lp,
                     vima_stream_t stream);
/* One env step. step 0 follows vima_seq_prefill and feeds the Q observation tokens obs_tok f32 [B,Q,E] (act_tok ignored, may be NULL);
 * step s > 0 feeds [a_{s-1}, o_s^1 .. o_s^Q] (act_tok f32 [B,E] required), Q + 1 rows at cache row Lp + 1 + s (Q + 1) - 1. Position ids
 * continue the sample's counter, k | v of the new rows are appended to every layer's cache by the c_attn GEMM, the new queries attend to
 * the cache with a causal offset. out f32 [B,E] = the last new row of every sample. Fails with code 34, changing nothing, when
 * Lp + 1 + rows so far + rows of this call > n_positions (the bound of vima_seq_decode), and with code 1 when the call does not continue
 * the episode state (no prefill, wrong B, wrong step number). With option "graphs" the call is captured and replayed (key: the pointers,
 * B, the row offset, whether there is an action token), bit-identical to eager; no auxiliary stream is used. */
int vima_seq_decode_step(VimaHandle* h, const float* obs_tok, const float* act_tok, int step, int B, float* out, vima_stream_t stream);
/* Per-sample restart inside a running batch, the decoder-only form of vima_decode_restart: for every sample with restart[b] != 0 (HOST
 * array [B]) the history rows [Lp + 1, current) are masked out, the position base is reset from ITS row of the new prompt, the next step's
 * action slot becomes a masked row (zeros are embedded: that row of act_tok is never read) and rows [0, Lp] of every layer's cache are
 * rebuilt. All flagged samples are rebuilt together: one prefill of n_flagged x (Lp + 1) rows and one scatter per layer by sample list,
 * the same number of launches whatever n_flagged is. Lp must equal the episode's; rows of `prompt` of unflagged samples are not read. The
 * batch keeps ONE row index space: a restart does not give rows back (vima_decode_steps_left) -- unless that space is a ring:
 *
 * Option "seq_ring" = 1 (default 0: every call behaves bit for bit as described above; changing it ends a running episode) makes the rows
 * behind the prefix a ring, for batches that never stop. Rows [0, P0), P0 = Lp + 1, of every sample's cache block stay the fixed prefix
 * (prompt + separator; a restart rewrites them in place); rows [P0, n_positions) are the ring, R = n_positions - P0 rows, still ONE row index
 * space for the whole batch. wp, hw, age[b], where a step's rows go and when it is legal (code 34 naming the first sample over age, nothing
 * changed, otherwise) are THE ROW BOOKKEEPING described at vima_decode_step, with this P0; vima_seq_prefill begins it. `step` keeps its meaning
 * (previous + 1) and is unbounded. The step's k | v go to rows [row, row + Lq) and its queries read the written image [0, hw) under the
 * WINDOWED causal rule of vima_decode_step's ring (key j is "future" for the step's query i iff i + row < j < row + Lq; the rows from
 * row + Lq on hold older history) and the cache's key mask; rows at and beyond hw were never written and are never read. In the first lap
 * hw = row + Lq: the launches are those of the linear cache, bit for bit. vima_seq_decode_restart clears a flagged sample's key mask over the
 * whole ring image [P0, hw), rebuilds its prefix and position base as above, takes no ring rows and sets age[b] = 0: the predictions of a
 * sample depend on its own episode only and equal those of the linear cache up to the order of the softmax sums. Position ids stay the
 * per-sample device counters and never reach the clamp of the position table: a sample's counter is at most Lp + 1 (prefix) plus one per
 * ring row of its episode, and those rows are at most age[b] <= R, so posbase <= Lp + 1 + age <= n_positions and every id used is below
 * n_positions. A sample's own episode is thus bounded by n_positions tokens, as in vima_seq_decode. With option "graphs" the key also
 * carries hw; one eager step with an action slot warms the whole family and every (row, hw) is captured when first seen. From the second
 * lap on every step has Q + 1 rows starting at P0, so the rows repeat exactly and the set of graphs stops growing one lap after hw has
 * stopped moving. */
int vima_seq_decode_restart(VimaHandle* h, const uint8_t* restart, int B, const float* prompt, int64_t stride_b, int64_t stride_l,
                            const uint8_t* prompt_mask, int Lp, vima_stream_t stream);
/* Episode prefill of the decoder-only policies (GPT / GATO handles only, option decode_ring refused, like the other vima_seq_* calls): the
 * counterparts of vima_decode_chunk / vima_decode_restart_history / vima_decode_history_room.
 *
 * vima_seq_decode_chunk: the T calls vima_seq_decode_step(step) .. (step + T - 1) as ONE pass. obs_tok f32 [T,B,Q,E], out f32 [T,B,E]; act_tok
 * f32 [T,B,E] when step > 0 (row 0 = the action of step - 1, row j that of step + j - 1), f32 [T-1,B,E] when step == 0 (NULL for T = 1). `step`
 * must continue the episode state as for the single step. The chunk is Lq = T (Q + 1) - (step == 0) contiguous rows: slot u is [a, o^1 .. o^Q] at
 * row + u (Q + 1) - (step == 0); the first slot of batch step 0 has no action row. Linear cache: legal iff rows so far + Lq <= n_positions, else
 * code 34, the message says how many steps still fit ("room for N more steps") and nothing changes. Option "seq_ring": the chunk is ONE unit of
 * the ring -- row = wp, or P0 after skipping the tail [wp, n_positions) when wp + Lq > n_positions; never split -- legal iff age[b] + advance <= R
 * for every b, else code 34, the first such sample is named and nothing changes; because the skipped tail is longer a chunk can be refused where
 * single steps still pass. The new queries attend with q_off = row, win_end = row + Lq (ring; the plain rule otherwise) to the keys
 * [0, max(hw, row + Lq)): the chunk's rows are causal among themselves, everything else written is history. The episode state afterwards is that
 * of the T single calls (step number, rows, ages, hw, one position id per valid row). A sample restarted right before the chunk has only the
 * chunk's FIRST action slot masked (zeros embedded, no position id, its act_tok row not read). T == 1 is vima_seq_decode_step itself: same
 * code, same bits, same graph keys. T > 1 runs eager also with option "graphs"; the captured step graphs stay valid and are replayed afterwards.
 * There is no bound on Lq beyond the two legality rules: the chunk has its own embedding kernel (no 64-row limit of the single step's) and
 * GEMM, attention, LayerNorm and gather take any row count.
 * Every successful step / chunk appends one host record per env step (first obs row, ring rows advanced; a chunk's skipped tail counts with its
 * first step); vima_seq_prefill clears the record.
 *
 * vima_seq_history_room (host only): the largest T vima_seq_decode_restart_history accepts now -- without seq_ring the batch steps taken since
 * the prefill, with it the largest r such that the ring rows advanced by the last r batch steps sum to at most R.
 *
 * vima_seq_decode_restart_history: everything vima_seq_decode_restart does for the flagged samples, then T env steps of history installed for
 * each of them, so that an episode recorded elsewhere continues inside this running batch. hist_obs f32 [T,n_r,Q,E], hist_act f32 [T-1,n_r,E]
 * (NULL for T = 1), n_r = the flagged samples in increasing order, one T per call; out NULL or f32 [T,n_r,E] = the teacher-forced predictions.
 * T == 0 is vima_seq_decode_restart, bit for bit. Code 34 before ANYTHING changes (the restart included) when T > room (the message names the
 * room) or Lp + T (Q + 1) > n_positions. With t the next batch step, history step s takes the cache rows batch step t - T + s wrote: its Q obs
 * rows in that slot's obs rows, a_{s-1} in its action row (s > 0); the first slot's action row stays masked. With seq_ring age[b] becomes the sum
 * of those T slots' advances -- the age of a sample restarted right before batch step t - T (vima_decode_steps_left agrees). ONE pass of the
 * vima_seq_decode form, [prompt | sep | o_0, a_0, .., o_{T-1}] = Lp + T (Q + 1) rows of the n_r samples, replaces the restart's prefix prefill; per
 * layer one launch scatters K | V by (sample list, row map); one kernel masks the old episode's history rows and writes the key mask (prompt mask,
 * 1 for the separator and every mapped row), posbase[b] = nv_b + T (Q + 1) and fresh[b] = 0: the next step consumes the sample's act_tok row, the
 * action of history step T - 1. Other samples are not touched; the launch count does not depend on n_r; eager also with "graphs". */
int vima_seq_decode_chunk(VimaHandle* h, const float* obs_tok, const float* act_tok, int step, int T, int B, float* out, vima_stream_t stream);
int vima_seq_decode_restart_history(VimaHandle* h, const uint8_t* restart, int B, const float* prompt, int64_t stride_b, int64_t stride_l,
                                    const uint8_t* prompt_mask, int Lp, const float* hist_obs, const float* hist_act, int T, float* out,
                                    vima_stream_t stream);
int vima_seq_history_room(VimaHandle* h, int32_t* steps_host);

/* ---- branch rollouts: fork a sample's episode into other batch slots (additive, ABI version unchanged) ------------
 * source: HOST int32 [B]; slot b continues the episode of slot source[b], source[b] == b leaves b untouched. Nothing is recomputed: the
 * destination's state is a copy of the source's -- in every layer the rows of the episode K | V cache the source's episode has written and that
 * are still there (EpisodeBook::live_ranges: the last age[source] advanced rows behind the write pointer, at most two ranges in a ring; the
 * batch shares one row index space, so they already sit at the row numbers the destination needs), its key-mask row (whole), its position
 * counter and its "fresh" flag; vima_decode_fork also copies the sample's block of every layer's prompt K / V cache (contiguous in either
 * layout), vima_seq_decode_fork the fixed prefix rows [0, Lp] (prompt | separator) instead. On the host the destination takes its source's ring
 * age, so its vima_decode_steps_left entry is its source's; write pointer, high-water mark and slot record are batch-wide and stay. The
 * destination's old episode is dropped, as by a restart. Its next step consumes or ignores its act_tok row exactly as the source's would; fed
 * the source's inputs it returns the source's bits, fed others it is a branch. vima_decode_fork: the caller passes the SOURCE's prompt mask row
 * for the destination from the next vima_decode_step on (VIMAPolicy.fork_samples updates the tensors).
 * Every source must be its own source (source[source[b]] == source[b]: no chains, no swaps), so that the copy runs in place and no slot is both
 * read and written; any beam reorder can be written that way, survivors keep their slots. Refusals, before anything changes: no running episode
 * batch of this B (vima_decode_step(step = 0) / vima_seq_prefill); the other policy family's handle (the message names the other entry); a
 * source map that breaks the rule: code 22, naming the first offending sample. The identity map launches nothing.
 * Cost, whatever the number of pairs and layers: ONE upload of a job table (host copy kept in the handle) and at most 3 launches -- episode K | V
 * (episode_fork_kernel: all layers, groups and ranges; a source's chunk is loaded once and stored to each of its destinations, 16-byte accesses),
 * prompt K / V (the same kernel; vima_decode_fork only) and the per-sample state. Stream-ordered and asynchronous; no allocation beyond the
 * handle's workspace. Captured step graphs stay valid (no pointer and no plan changes). */
int vima_decode_fork(VimaHandle* h, const int32_t* source /* HOST [B] */, int B, vima_stream_t stream);
int vima_seq_decode_fork(VimaHandle* h, const int32_t* source /* HOST [B] */, int B, vima_stream_t stream);

/* ---- episode snapshots: save a sample's decoder state, restore it later (additive, ABI version unchanged) -----------
 * A fork copies an episode between slots of one batch at one moment; a snapshot carries it across time, slots and handles. The snapshot of sample b
 * is its episode in COMPACT TIME ORDER, independent of where the ring holds the rows: with n = the env steps the episode has taken (the trailing
 * batch steps whose advanced rows sum to the sample's ring age, EpisodeBook::steps_of; no such suffix: internal error, nothing changes), the
 * R = max(n (Q + 1) - 1, 0) rows [o_0 (Q), a_0, o_1 (Q), ...] of every layer's episode K | V cache, in the order of EpisodeBook::history_rows(n),
 * their key-mask bytes, the position counter and the fresh flag; and (flag VIMA_SNAPSHOT_PROMPT) the sample's prompt: vima_decode_snapshot stores its
 * block of every layer's prompt K / V cache ROW-MAJOR [layers][Lp][2E] whatever layout the handle's cache has (option kv_headmajor; converted as
 * kv_rows_kernel does from the cache, and back as it does to the cache), vima_seq_decode_snapshot the prefix rows [0, P0 = Lp + 1) of the episode cache and
 * their mask bytes. A snapshot without the prompt leaves the destination's prompt K / V block (prefix rows) untouched on restore: the caller vouches
 * that the slot holds this prompt -- the cheap form for backtracking inside one prompt group.
 *
 * Payload (DEVICE memory, 16-byte aligned, one buffer per snapshot; elements of the handle's operand type, elem_bytes 4 or 2), sections in this order,
 * each a multiple of 16 bytes:
 *   header  16 bytes   int32 {position counter, fresh flag, R, 0} -- written and read on the device: neither call synchronises with the host
 *   mask    pad16(M)   key-mask bytes, M = R (vima_seq_* with the prompt: P0 prefix bytes first, M = P0 + R)
 *   rows    layers x R x 2E elements
 *   prompt  layers x Lp x 2E elements (vima_seq_*: layers x P0 x 2E), only with VIMA_SNAPSHOT_PROMPT
 * VimaEpisodeSnapshotInfo is the host-side description; restore refuses (code 22) an info that does not match the handle: policy kind, embed_dim,
 * layers, elem_bytes, Q, prompt_len, or a byte count that is not the format's.
 *
 * vima_*_snapshot_size: host only; fills infos[i] for samples[i] so that the caller can allocate infos[i].bytes. vima_*_snapshot: packs sample
 * samples[i] into payloads[i] (capacity[i] >= the size, else code 22) and fills infos[i]; a sample may be listed more than once.
 * vima_*_restore: slot slots[i] becomes the episode of (payloads[i], infos[i]), at any later time and on any matching handle -- a restart of the slot
 * followed by an install: its mask row is cleared, the rows go to history_rows(n) of the CURRENT book (the rows the last n batch steps wrote), the
 * mask bytes to the same rows, counter and flag are written, and on the host the slot's ring age becomes that of a sample restarted n batch steps ago
 * (so is its vima_decode_steps_left entry). The rule is that of vima_decode_restart_history: n <= the history room, else code 34 and nothing changes.
 * n = 0 is legal (a just-restarted sample: only the prompt and fresh = 1 travel). Each pair has its own n; one snapshot may go to several slots; a
 * slot listed twice is refused (22). Other samples keep their bits. vima_decode_restore: the caller passes the snapshot's prompt mask row for the slot
 * from the next vima_decode_step on (VIMAPolicy.restore_samples updates the tensors).
 * Refusals, all before anything changes: the other policy family's handle, no running episode batch, a sample / slot outside the batch, a mismatched
 * info, a too-small capacity, a misaligned payload, and a payload that is not DEVICE memory (hipPointerGetAttributes; code 22).
 * Cost, whatever the number of pairs and layers: ONE table upload (host copy kept in the handle) and at most 3 launches per call -- episode rows
 * (episode_pack_kernel / episode_unpack_kernel), prompt K / V (the same kernel), state; vima_seq_*: 2, the prefix rows ride in the first.
 * Stream-ordered and asynchronous. Captured step graphs stay valid: no pointer and no plan changes. */
#define VIMA_SNAPSHOT_PROMPT 1
typedef struct VimaEpisodeSnapshotInfo {
  int32_t steps;        /* n */
  int32_t Q;
  int32_t embed_dim;
  int32_t layers;
  int32_t prompt_len;   /* Lp (GPT / Gato: P0 = Lp + 1) */
  int32_t elem_bytes;
  int32_t flags;        /* VIMA_SNAPSHOT_* */
  int32_t policy_kind;  /* VIMA_POLICY_* */
  int64_t bytes;        /* of the payload */
} VimaEpisodeSnapshotInfo;
int vima_decode_snapshot_size(VimaHandle* h, const int32_t* samples /* HOST [n] */, int n, int with_prompt, VimaEpisodeSnapshotInfo* infos /* HOST [n] */);
int vima_decode_snapshot(VimaHandle* h, const int32_t* samples, int n, int with_prompt, void* const* payloads /* HOST [n] of DEVICE pointers */,
                         const int64_t* capacity /* HOST [n], bytes */, VimaEpisodeSnapshotInfo* infos, vima_stream_t stream);
int vima_decode_restore(VimaHandle* h, const int32_t* slots /* HOST [n] */, int n, const void* const* payloads, const VimaEpisodeSnapshotInfo* infos,
                        vima_stream_t stream);
int vima_seq_decode_snapshot_size(VimaHandle* h, const int32_t* samples, int n, int with_prompt, VimaEpisodeSnapshotInfo* infos);
int vima_seq_decode_snapshot(VimaHandle* h, const int32_t* samples, int n, int with_prompt, void* const* payloads, const int64_t* capacity,
                             VimaEpisodeSnapshotInfo* infos, vima_stream_t stream);
int vima_seq_decode_restore(VimaHandle* h, const int32_t* slots, int n, const void* const* payloads, const VimaEpisodeSnapshotInfo* infos,
                            vima_stream_t stream);

/* ---- image preprocessing in front of the policy ------------------------------------------- */
/* The per-object work of prepare_obs / prepare_prompt (/root/reference/scripts/example.py:374-473 and :243-371; numpy +
 * cv2 per object on the host there): for every frame and every object id, segmentation mask -> pixel bbox ->
 * inclusive crop -> zero-pad to a square -> cv2.resize(32x32, INTER_AREA) -> uint8, with the reference's slot order
 * (objects covering >= 2 pixels first, in obj_ids order; the rest zero rows with mask 0).
 * rgb u8 [n_frames,3,H,W], segm [n_frames,H,W] of uint8 (segm_elem_bytes 1) or int32 (4), obj_ids i32 [n_obj <= 64]
 * (all device pointers; H, W <= 320) -> crops u8 [n_frames,n_obj,3,32,32], bbox i64 [n_frames,n_obj,4] = (int x-centre,
 * int y-centre, ymax-ymin, xmax-xmin), mask u8 [n_frames,n_obj]: exactly the cropped_img / bbox / mask arrays of ONE view
 * that vima_obs_encode / vima_prompt_encode take. No handle: there are no weights involved. */
int vima_crop_objects(const uint8_t* rgb, const void* segm, int segm_elem_bytes, const int32_t* obj_ids, int n_frames,
                      int n_obj, int H, int W, uint8_t* crops, int64_t* bbox, uint8_t* mask, vima_stream_t stream);

/* ---- multi-GPU: the one exchange step of the data-parallel path ----------------------------------- */
/* The reference has no distributed code (no torch.distributed / NCCL call site anywhere under vima/); batched episodes
 * are independent, so the path shards over one process per GPU with a full weight replica and ONE collective per
 * step: an all-gather of the raw action logits (the output of vima_action_head) over RCCL / xGMI.
 * vima_comm_unique_id: rank 0 creates the 128-byte rendezvous id (ncclGetUniqueId) and hands it to the other ranks
 * out of band (the Python host broadcasts it through the torch.distributed store);
 * vima_comm_create: every rank joins (ncclCommInitRank) on its own `device`;
 * vima_allgather_logits: local f32 [rows_per_rank, width] -> global f32 [world * rows_per_rank, width] on every
 * rank, enqueued on `stream` (no host synchronisation). Equal shard sizes (the host pads ragged tails). */
#define VIMA_COMM_ID_BYTES 128
typedef struct VimaComm VimaComm;
int vima_comm_unique_id(uint8_t id[VIMA_COMM_ID_BYTES]);
int vima_comm_create(const uint8_t id[VIMA_COMM_ID_BYTES], int world, int rank, int device, VimaComm** out);
int vima_comm_world(const VimaComm* c);
int vima_comm_rank(const VimaComm* c);
int vima_allgather_logits(VimaComm* c, const float* local, float* global, int64_t rows_per_rank, int width,
                          vima_stream_t stream);
void vima_comm_destroy(VimaComm* c);

/* ---- operator-level entry points (parity tests / microbenchmarks) ---------------------------------------------- */
/* out = epilogue(A[M,K] . W[N,K]^T) in the handle's precision; fp32 host-visible device buffers in/out, the
 * operand conversion is done internally. act: 0 none, 1 relu, 2 gelu(erf), 3 quickgelu. bias/mul/res may be NULL. */
int vima_op_linear(VimaHandle* h, const float* A, const float* W, const float* bias, const float* mul,
                   const float* res, int M, int N, int K, int act, float* out, vima_stream_t stream);
/* ONE GEMM launch described field for field (additive, ABI version unchanged; parity tests of the launcher's structured forms). Every field has the meaning of the
 * GemmArgs field of the same name in vima_amd/csrc/kernels.h; strides are in elements. A, W, A2, W2, mul, resT, outT and outT_lo are
 * DEVICE buffers in the handle's operand type (bf16 on BF16 / FP8W handles, fp32 on FP32 / BF16X3 handles), the others fp32 / int32
 * device buffers; nothing is cast, widened or staged, and the launcher's own validation is the only one: a form or geometry it
 * refuses is returned as an error with no output written. x3 = 1 asks for the split-bf16 products of a BF16X3 handle. The handle's
 * GEMM options apply; *kernel_id (optional) receives the kernel the launcher chose (the ids of vima_prof_read_gemm_kernels).
 * The GEMM's fp8 operands (GemmArgs::a8 / w8) and its e4m3 output (out8) are not reachable through this entry or any other operator entry:
 * they are held at model level only (tests/test_fp8_gpu.py). The e4m3 producers OUTSIDE the GEMM epilogue have entries of their own
 * (vima_op_fp8_quant ... vima_op_vit_attention_cls_fp8 below). */
typedef struct VimaGemmDesc {
  const void* A; const void* W; const void* A2; const void* W2; const void* mul; const void* resT;
  void* outT; void* outT_lo;
  const float* bias; const float* res; const float* rs_ssq; const float* rs_sum; const float* rs_c;
  float* out32; float* ssq_out; float* sum_out;
  const int32_t* grp_col;
  int64_t bsA, bsW, bsBias, bsMul, bsRes, bs32, bsT;
  int32_t M, N, K, lda, ldw, lda2, ldw2, ldmul, ldres, ldresT, ld32, ldT, ldT_lo, batch, act;
  int32_t hm_D, hm_L, pair32, rb, s_hi, s_lo, ro, split_n, rs_parts, x3;
  float rs_invk, rs_eps;
} VimaGemmDesc;
int vima_op_gemm(VimaHandle* h, const VimaGemmDesc* desc, int* kernel_id, vima_stream_t stream);
/* LayerNorm (rms=0) / T5 RMSNorm (rms=1) over rows of length E. */
int vima_op_layernorm(VimaHandle* h, const float* x, const float* gamma, const float* beta, float eps, int rms,
                      int rows, int E, float* out, vima_stream_t stream);
/* attention on fp32 buffers q [B,Lq,H*D], k/v [B,Lk,H*D]; mode 0 T5 (relbias [H][2Lk-1]), 1 cross, 2 causal;
 * impl 0 = exact generic kernel, 1 = MFMA flash kernel (bf16 precision; on a BF16X3 handle the split-bf16 kernel, head dims 32 / 64). */
int vima_op_attention(VimaHandle* h, const float* q, const float* k, const float* v, const uint8_t* kmask,
                      const float* relbias, int B, int H, int Lq, int Lk, int D, float scale, int mode, int impl,
                      float* out, vima_stream_t stream);
/* the causal mode over a RING image k/v [B,Lk,H*D] (option "decode_ring"): the Lq queries sit at rows [q_off, q_off + Lq) and key j is "future"
 * (score -1e4) for query i iff i + q_off < j < q_off + Lq; every other key, in front of or behind the window, is visible unless kmask hides it.
 * q_off = 0, Lq = Lk is vima_op_attention mode 2, bit for bit. impl as above. */
int vima_op_attention_window(VimaHandle* h, const float* q, const float* k, const float* v, const uint8_t* kmask, int B, int H, int Lq,
                             int Lk, int D, float scale, int impl, int q_off, float* out, vima_stream_t stream);
/* The ViT front end's non-GEMM kernels, ONE launcher call each (additive, ABI version unchanged; tests/test_vit_front_gpu.py holds every output
 * element against fp64). Conventions of vima_op_attention: fp32 device buffers in and out, q | k | v cast to the handle's operand type
 * internally, the operand-type result widened back to fp32; the fp32 side inputs (cls, pos, g, b, the bbox weights) are read as they are.
 * Whatever a launcher refuses, and every non-positive size or NULL buffer, comes back as an error with nothing written to `out`.
 * ViT self-attention (nn.MultiheadAttention, head dim 32, scale 1/sqrt(32)) of M crops with S <= 16 tokens: qkv [M*S, 3W] (q | k | v of a
 * token, head h at columns h*32) -> out [M*S, W]. impl 0 = the launcher's own choice (on a bf16 handle at S = 5, W = 768, heads = 24 the
 * LDS-staged kernel unless VIMA_VIT_ATTN_LDS=0), 1 = the register kernel with the instantiation S asks for (8 scores for S <= 8, else 16),
 * 2 = the register kernel's 16-score instantiation whatever S. The three are bit-identical where more than one applies. */
int vima_op_vit_attention(VimaHandle* h, const float* qkv, int M, int S, int W, int heads, int impl, float* out, vima_stream_t stream);
/* the last ViT block's form: only the cls query. q [M, W], kv [M*S, 2W] (k | v of every token), S <= 8 -> out [M, W]; the bits of row 0 of
 * every crop of vima_op_vit_attention on the same values. */
int vima_op_vit_attention_cls(VimaHandle* h, const float* q, const float* kv, int M, int S, int W, int heads, float* out, vima_stream_t stream);
/* /255, (x - mean) / std and the im2col of the PxP stride-P conv: img u8 [M, 3, H, W] -> out [M*(H/P)*(W/P), 3*P*P], row = image, gy, gx,
 * column = c, py, px. P a multiple of 16 that divides H and W. impl 0: (H, W, P) = (32, 32, 16) runs the object-crop kernel, anything else
 * the rectangular one; impl 1: the rectangular kernel at every shape (bit-identical at the crop shape). */
int vima_op_patchify(VimaHandle* h, const uint8_t* img, int M, int H, int W, int P, int impl, float* out, vima_stream_t stream);
/* ln_pre((t == 0 && cls ? cls : patch row) + pos[t]) over width 768, eps 1e-5, written in the operand type (the path that rounds): pre
 * [M*n_patch, 768], cls [768] or NULL (then token t is patch t), pos [S, 768], g, b [768] -> out [M*S, 768]; S - (cls ? 1 : 0) <= n_patch.
 * impl 0: cls != NULL, S = 5, n_patch = 4 runs the object-crop kernel, anything else the rectangular one; impl 1: the rectangular kernel
 * at every shape (bit-identical at the crop shape). */
int vima_op_vit_embed(VimaHandle* h, const float* pre, const float* cls, const float* pos, const float* g, const float* b, int M, int S,
                      int n_patch, int impl, float* out, vima_stream_t stream);
/* first layer of the bbox MLP: relu(W [N, 4] . (bbox / [256, 128, 128, 256]) + b [N]); bbox i64 [R, 4] -> out [R, N]. */
int vima_op_bbox_l1(VimaHandle* h, const int64_t* bbox, const float* W, const float* b, int R, int N, float* out, vima_stream_t stream);
/* The norm and sequence-assembly kernels (elementwise.hip, baseline_kernels.hip), ONE launcher call each (additive, ABI version unchanged;
 * tests/test_seq_norm_gpu.py holds every output element against fp64 or, for the exact ones, bit for bit). Conventions of the block above.
 * Buffers named x32 / out32 are written by the kernel in fp32; buffers named xT / outT / out2T receive the operand-type output widened to
 * fp32 (bf16 handles: bf16-exact values). Index arrays (tok_src, word_ids, list, sel) are DEVICE arrays and are not validated, as on the hot
 * path. State buffers (hist_mask, poscnt, fresh, cache_mask, posbase) are the caller's and are updated in place. A NULL required argument,
 * a non-positive size or anything the launcher refuses is an error with no caller buffer written.
 * vima_op_norm: kind VIMA_NORM_LN launch_layernorm (fp32 rows), VIMA_NORM_LN_T launch_layernorm_T (x cast to the operand type first: x holds
 * rows * ldin elements), VIMA_NORM_LN2 launch_layernorm2 (y = LN(x; gamma, beta, eps) -> out32 / outT, LN(y; gamma2, beta2, eps2) -> out2T),
 * VIMA_NORM_RMS_STATS launch_rms_stats (outT = x, ssq[r] = sum x[r][:]^2; ldin == E). rms = 1: T5 RMSNorm (beta NULL). out32 / outT optional
 * where the launcher makes them so. The e4m3 output of launch_layernorm_T is reached through vima_op_norm_fp8 (below), not through this entry;
 * no other norm launcher has one. */
enum { VIMA_NORM_LN = 0, VIMA_NORM_LN_T = 1, VIMA_NORM_LN2 = 2, VIMA_NORM_RMS_STATS = 3 };
typedef struct VimaNormDesc {
  const float* x; const float* gamma; const float* beta; const float* gamma2; const float* beta2;
  float* out32; float* outT; float* out2T; float* ssq;
  int64_t ldin;
  int32_t kind, rms, rows, E;
  float eps, eps2;
} VimaNormDesc;
int vima_op_norm(VimaHandle* h, const VimaNormDesc* desc, vima_stream_t stream);
/* The e4m3 producers of precision "fp8" outside the GEMM epilogue and the calibration's max |x|, ONE launcher call each (additive, ABI version
 * unchanged; tests/test_fp8_producers_gpu.py holds them bit for bit). Every one of them ends in fmed3(v * inv, -448, 448) and cvt_pk_fp8_f32
 * (round to nearest even) on an fp32 value v: out8 byte = OCP e4m3 code of clamp(v * inv), 0x7E / 0xFE at saturation, +-inf -> +-448, a NaN
 * -> 0xFE (-448). Conventions of the blocks above: fp32 device buffers in, cast to bf16 internally (exact for bf16-exact values); out8 is the
 * caller's DEVICE byte buffer and is written by the launcher directly. The launchers emit e4m3 from bf16 operands only: on an FP32 / BF16X3
 * handle every entry fails with nothing written, as does a NULL required argument, a non-positive size or anything the launcher refuses.
 * vima_op_fp8_quant: launch_quant_fp8, out8[r, c] = e4m3(x[r, c] * inv) for c < cols; x [rows, ldin], out8 [rows, ldo]; cols, ldin and ldo
 *   multiples of 8 (else refused); columns >= cols are neither read into the result nor written; rows = 0 succeeds and writes nothing.
 * vima_op_fp8_amax: launch_amax, *slot = max(*slot, max |x[:, :cols]|) on a DEVICE float that is NOT zeroed here (a non-negative value is the
 *   caller's to provide); all-zero data leaves it as it was, an inf in the data makes it inf and a NaN makes it a NaN. cols, ldin multiples of 8.
 * vima_op_norm_fp8: launch_layernorm_T (kind VIMA_NORM_LN_T only) with its e4m3 output: out8 [rows, E] = e4m3(y * inv8) of the fp32 y the
 *   kernel also stores to desc->out32 (NOT of its bf16 rounding); out32 and outT are optional, out8 alone works.
 * vima_op_vit_attention_fp8 / _cls_fp8: vima_op_vit_attention / _cls with out8 [M*S, W] / [M, W] = e4m3(out * inv8) of the fp32 head outputs
 *   written INSTEAD of the operand-type output; impl as there, the kernels bit-identical where more than one applies. */
int vima_op_fp8_quant(VimaHandle* h, const float* x, int64_t ldin, int64_t rows, int cols, float inv, uint8_t* out8, int64_t ldo,
                      vima_stream_t stream);
int vima_op_fp8_amax(VimaHandle* h, const float* x, int64_t ldin, int64_t rows, int cols, float* slot, vima_stream_t stream);
int vima_op_norm_fp8(VimaHandle* h, const VimaNormDesc* desc, uint8_t* out8, float inv8, vima_stream_t stream);
int vima_op_vit_attention_fp8(VimaHandle* h, const float* qkv, int M, int S, int W, int heads, int impl, float inv8, uint8_t* out8,
                              vima_stream_t stream);
int vima_op_vit_attention_cls_fp8(VimaHandle* h, const float* q, const float* kv, int M, int S, int W, int heads, float inv8, uint8_t* out8,
                                  vima_stream_t stream);
/* row r: tok_src[r] >= 0 word_table[word_ids[tok_src[r]]], -1 zeros (mask 0), <= -2 object row -(v + 2) of obj_tokens / obj_mask -> x [rows, E],
 * mask [rows]. stats = 0 launch_prompt_assemble (x fp32); stats = 1 launch_prompt_assemble_stats (x = the operand-type rows widened, ssq [rows]). */
int vima_op_prompt_assemble(VimaHandle* h, const int32_t* tok_src, const int64_t* word_ids, const float* word_table, const float* obj_tokens,
                            const uint8_t* obj_mask, int rows, int E, int stats, float* x, float* ssq, uint8_t* mask, vima_stream_t stream);
/* launch_dec_embed: obs_tok [T, B, Q, E], obs_mask [T, B, Q], act_tok [L_act, B, E], pos_table [n_pos, E] -> x32 / xT (optional) [B, T Q + L_act, E],
 * mask [B, T Q + L_act]; L_act = T or T - 1. */
int vima_op_dec_embed(VimaHandle* h, const float* obs_tok, const uint8_t* obs_mask, const float* act_tok, const float* pos_table, int n_pos,
                      int T, int B, int Q, int L_act, int E, float* x32, float* xT, uint8_t* mask, vima_stream_t stream);
/* One env step = launch_dec_embed_chunk, the chunk kernel at T = 1: obs_tok [B, Q, E], obs_mask [B, Q], act_tok [B, E] (has_act) -> x32 / xT
 * (optional) [B, Q + has_act, E]; hist_mask [B, Lmax] rows [L_hist, L_hist + Q + has_act), poscnt [B] and fresh [B] (optional) are updated.
 * Refused: Q + has_act > 64, rows past Lmax, E % 4. */
int vima_op_dec_embed_step(VimaHandle* h, const float* obs_tok, const uint8_t* obs_mask, const float* act_tok, const float* pos_table, int n_pos,
                           int L_hist, int Lmax, int B, int Q, int has_act, int E, float* x32, float* xT, uint8_t* hist_mask, int32_t* poscnt,
                           uint8_t* fresh, vima_stream_t stream);
/* launch_restart_samples: samples with flags[b] != 0 get hist_mask[b][:] = 0, poscnt[b] = 0, fresh[b] = 1. */
int vima_op_restart_samples(VimaHandle* h, const uint8_t* flags, uint8_t* hist_mask, int32_t* poscnt, uint8_t* fresh, int B, int Lmax,
                            vima_stream_t stream);
/* launch_prompt_pos: out block r [Lp, E] = prompt rows (element strides sb, sl) + pos_table[cumsum(mask) - 1] of sample list[r] (list NULL: r);
 * mask [samples, Lp]. */
int vima_op_prompt_pos(VimaHandle* h, const float* prompt, int64_t sb, int64_t sl, const uint8_t* mask, const float* pos_table, int n_pos,
                       const int32_t* list, int B, int Lp, int E, float* out, vima_stream_t stream);
/* launch_gather_pred: out [T, B, E] = x [B, Lq, E] rows (Q - 1) + (Q + 1) t. */
int vima_op_gather_pred(VimaHandle* h, const float* x, int T, int B, int Q, int Lq, int E, float* out, vima_stream_t stream);
/* launch_action_l1: relu(W [256, K] . (idx / bins) + b) -> columns [col0, col0 + 256) of out [R, ldo]; K = 2 bins (50, 100), K = 4 bins 50.
 * `out` is read first (values exact in the operand type): the columns the kernel does not write come back unchanged. */
int vima_op_action_l1(VimaHandle* h, const int64_t* idx, int K, const float* W, const float* b, int R, int ldo, int col0, float* out,
                      vima_stream_t stream);
/* launch_add_row_table: out [rows, E] += table[clamp(sel[r / group], 0, 1)], in place. */
int vima_op_add_row_table(VimaHandle* h, float* out, int rows, int E, const float* table, const int64_t* sel, int group, vima_stream_t stream);
/* The operand-type copies: `in` is cast to the operand type, `out` is read first like vima_op_action_l1's (blocks and rows the kernel does
 * not write come back unchanged). rows_to_headmajor: in [L, N] -> out [N / D, L, D]. kv_scatter: in [n, L, N] -> block list[r] of out
 * [n_blocks, L N], row-major (hm = 0) or head-major. seq_kv_store: in [n L, ld_in] columns [0, N) -> rows [0, L) of block list[r] (NULL: r)
 * of out [n_blocks, Lmax, N]. broadcast_rows (fp32): out [rows, E] = src [period, E] rows r % period. */
int vima_op_rows_to_headmajor(VimaHandle* h, const float* in, int L, int N, int D, float* out, vima_stream_t stream);
int vima_op_kv_scatter(VimaHandle* h, const float* in, const int32_t* list, int n, int L, int N, int D, int hm, int n_blocks, float* out,
                       vima_stream_t stream);
int vima_op_seq_kv_store(VimaHandle* h, const float* in, int64_t ld_in, const int32_t* list, int n, int L, int N, int Lmax, int n_blocks,
                         float* out, vima_stream_t stream);
int vima_op_broadcast_rows(VimaHandle* h, const float* src, int64_t rows, int E, int period, float* out, vima_stream_t stream);
/* The decoder-only sequence (launch_seq_embed, _prefill, launch_seq_restart; vima_op_seq_embed_step is launch_seq_embed_chunk, the chunk kernel at
 * T = 1, and refuses Q + has_act > 64, rows past n_pos, E % 4): prompt (element strides sb, sl), pmask [samples, Lp],
 * sep [E], obs_tok [T, B, Q, E] / act_tok [T, B, E] (step: [B, Q, E] / [B, E]) -> x32 and xT (optional) [B, L, E] / [n, Lp + 1, E] /
 * [B, Q + has_act, E], mask; cache_mask [samples, n_pos], posbase [samples], fresh [samples] are the episode state. */
int vima_op_seq_embed(VimaHandle* h, const float* prompt, int64_t sb, int64_t sl, const uint8_t* pmask, const float* sep, const float* obs_tok,
                      const float* act_tok, const float* pos_table, int n_pos, int B, int L, int Lp, int Q, int E, float* x32, float* xT,
                      uint8_t* mask, vima_stream_t stream);
int vima_op_seq_embed_prefill(VimaHandle* h, const float* prompt, int64_t sb, int64_t sl, const uint8_t* pmask, const float* sep,
                              const float* pos_table, int n_pos, const int32_t* list, int n, int Lp, int E, float* x32, float* xT, uint8_t* mask,
                              uint8_t* cache_mask, int32_t* posbase, vima_stream_t stream);
int vima_op_seq_embed_step(VimaHandle* h, const float* obs_tok, const float* act_tok, const float* pos_table, int n_pos, int row0, int B, int Q,
                           int has_act, int E, float* x32, float* xT, uint8_t* cache_mask, int32_t* posbase, uint8_t* fresh, vima_stream_t stream);
int vima_op_seq_restart(VimaHandle* h, const int32_t* list, int n, int lo, int hi, int n_pos, uint8_t* cache_mask, uint8_t* fresh,
                        vima_stream_t stream);
/* launch_seq_embed_chunk: obs_tok [T, B, Q, E], act_tok [T, B, E] (has_act) / [T - 1, B, E] -> x32 and xT (optional) [B, T (Q + 1) - (1 - has_act), E];
 * writes cache_mask[b][row0 .. row0 + rows), advances posbase, consumes fresh. launch_seq_history_install: mask [n, L], list [n], rowmap [L]
 * (DEVICE arrays; rowmap values must lie in [0, n_pos)): cache_mask[list[r]][lo .. hi) = 0, then [rowmap[l]] = mask[r][l]; posbase[list[r]] = the
 * valid rows; fresh[list[r]] = 0. Rows and samples the kernels do not write come back unchanged. */
int vima_op_seq_embed_chunk(VimaHandle* h, const float* obs_tok, const float* act_tok, const float* pos_table, int n_pos, int row0, int T, int B, int Q,
                            int has_act, int E, float* x32, float* xT, uint8_t* cache_mask, int32_t* posbase, uint8_t* fresh, vima_stream_t stream);
int vima_op_seq_history_install(VimaHandle* h, const uint8_t* mask, const int32_t* list, const int32_t* rowmap, int n, int L, int lo, int hi, int n_pos,
                                uint8_t* cache_mask, int32_t* posbase, uint8_t* fresh, vima_stream_t stream);
/* launch_episode_fork (episode_fork_kernel) alone, IN PLACE on the caller's DEVICE buffer `cache` [NL][B][L][N] of elem_bytes-wide elements (4: fp32,
 * 2: bf16; the handle's precision plays no part; N * elem_bytes a multiple of 16 and the buffer 16-byte aligned, else code 22). HOST arrays in CSR
 * form: group g copies from sample group_src[g] to the samples dsts[group_ptr[g] .. group_ptr[g + 1]) the row ranges [ranges[2 i], ranges[2 i + 1])
 * for i in [range_ptr[g], range_ptr[g + 1]), in every layer; group_ptr and range_ptr hold n_groups + 1 entries starting at 0. Sources and
 * destinations must be disjoint sets of distinct samples and every range must lie in [0, L] (refused otherwise); empty ranges and groups without
 * destinations copy nothing. Rows and samples outside the listed (destination, range) set come back unchanged. */
int vima_op_episode_fork(VimaHandle* h, void* cache, int elem_bytes, int NL, int B, int L, int N, const int32_t* group_src, const int32_t* group_ptr,
                         const int32_t* dsts, const int32_t* range_ptr, const int32_t* ranges, int n_groups, vima_stream_t stream);
/* launch_episode_pack / launch_episode_unpack (episode_pack_kernel / episode_unpack_kernel) alone, on the caller's DEVICE buffer `cache`
 * [NL][B][L][N] of elem_bytes-wide elements (4 or 2; N * elem_bytes a multiple of 16 and the buffer 16-byte aligned, else code 22). D = 0: every
 * sample's block is rows [L][N]; D > 0: head-major [N / D][L][D] (D * elem_bytes a multiple of 16, N a multiple of D). rowmap: HOST [n_map], every
 * entry in [0, L) (NULL: the identity 0 .. n_map - 1, n_map <= L). Job j moves the nrows[j] <= n_map rows rowmap[n_map - nrows[j] ..] -- a SUFFIX of
 * the one table -- of sample samples[j], in every layer, between the cache and payloads[j], a DEVICE buffer [NL][nrows[j]][N] (row-major whatever D;
 * 16-byte aligned; anything but device memory is refused with code 22 before any launch). samples / nrows: HOST [n_jobs]; payloads: HOST array of
 * n_jobs DEVICE pointers. Pack reads the cache; unpack writes it, refuses a sample listed twice, and leaves every other row and sample unchanged. */
int vima_op_episode_pack(VimaHandle* h, const void* cache, int elem_bytes, int NL, int B, int L, int N, int D, const int32_t* rowmap, int n_map,
                         const int32_t* samples, const int32_t* nrows, void* const* payloads, int n_jobs, vima_stream_t stream);
int vima_op_episode_unpack(VimaHandle* h, void* cache, int elem_bytes, int NL, int B, int L, int N, int D, const int32_t* rowmap, int n_map,
                           const int32_t* samples, const int32_t* nrows, const void* const* payloads, int n_jobs, vima_stream_t stream);
/* precision FP8: the calibrated activation scales (dequantisation scale = headroom x max |x| / 448, see VIMA_PRECISION_FP8) of group 0 the T5 stack [12 layers][4 sites:
 * stream before qkv, attention context, stream before wi, ReLU hidden], 1 the ViT [4 blocks][4 sites: ln_1 output, attention output,
 * ln_2 output, QuickGELU hidden], 2 the decoder's prompt K/V projection [1]; returns their number (0 before that group's calibrating
 * pass, < 0 on error). Option "fp8_recalibrate" makes the next pass of every group measure them again. */
int vima_fp8_act_scales(VimaHandle* h, int group, float* out, int max_n);
/* host-only: the fp32 -> OCP FP8 E4M3 (round to nearest even, saturating at 448) encoder the FP8W weight packing uses */
void vima_fp8_e4m3_encode(const float* src, uint8_t* dst, int64_t n);
/* host-only: HF T5 bidirectional relative-position bucket (32 buckets, max distance 128) of (key_pos - query_pos) */
int vima_t5_bucket(int relative_position);

/* ---- tuning / instrumentation ---------------------------------------------------------------------------------- */
/* Per-handle options (every key vima_set_option accepts; unknown keys fail). Defaults in brackets.
 *   kernel selection, GEMM:  "gemm_variant" [1] 1 inline-asm LDS-DMA pipeline, 0 compiler-tracked builtin (128x128 tile only)
 *                            "gemm_tile"    [0] 0 auto, 1 force 128x128, 2 force 256x256, 7 force 32x64, 8 force 64x64,
 *                                               10 / 11 / 12 force the resident-K kernel's 32x32 / 64x32 / 64x64 tile
 *                            "gemm_persist" [1] large bf16 GEMMs on the persistent 256x256 kernels
 *                            "gemm_pp"      [1] ping-pong (8-phase) main loop of the persistent kernel (0: the round-2 loop)
 *                            "gemm_wide"    [0] 256x384 persistent tile where N % 384 == 0
 *                            "gemm_q4"      [6] gemm_q4_kernel, FOUR waves (one per SIMD) with a 384-column tile, where N % 384 == 0, K % 128 == 0 (bf16-output /
 *                                               bf16-stream / head-major epilogues): 1 its 256x384 tile wherever it fits, 2 its 128x384 tile wherever it fits,
 *                                               3 the 128x384 tile where it needs fewer rounds of the chip than the 256x256 tiling (batch 32), 6 (default) the 256x384 tile
 *                                               for GEMMs of >= 32 768 rows (wall clock of the two-stream model: -1.4 % on the headline step), 0 off; bit-identical results in every mode
 *                            "gemm_q4_rs"   [1] the fused-RMSNorm consumers with 24 partials per row, a bf16 output and no bias (T5 q|k|v and wi) take gemm_q4_kernel's
 *                                               256x384 tile as well, wherever "gemm_q4" gives that tile: a lane carries its four row scales through the K loop in
 *                                               registers; 0 = they stay on gemm_pp_kernel; bit-identical either way
 *                            "gemm_small"   [1] 64x64 / 32x64 tiles for grids that would leave most CUs idle
 *                            "gemm_resident" [1] underfilled grids on gemm_resident_kernel ((almost) the whole K extent in flight, one
 *                                               barrier per chunk of K-slices; bit-identical to the ring tiles), 0: the 4-deep ring tiles
 *                            "gemm_res_maxwg" [256] largest grid (workgroups) gemm_resident_kernel takes for M > 32
 *                            "gemm_skinny"  [1] GEMMs of at most 32 rows (one env step at batch <= 3, the action head ...) on gemm_skinny_kernel: K split
 *                                               over the 4 / 8 / 16 waves of a workgroup, operands straight from global memory, 8 / 16 / 32-column tiles.
 *                                               A DIFFERENT summation order than every other tile (which all agree bit for bit): a sample evaluated alone and the
 *                                               same sample inside a large batch then agree to bf16 rounding (~2e-4 on logits of 0.08), not bit for bit;
 *                                               0 = the resident 32x32 tile for these shapes
 *                            "gemm_flat"    [1] gemm_pp_kernel enumerates its tiles plainly (no XCD raster) where the raster's padding of the A panels to a
 *                                               multiple of 8 would cost a round and the grid is at most two tiles per workgroup (M = 2304: the GEGLU pair
 *                                               of an incremental env step at batch 256); bit-identical, 0 = always the raster
 *                            "gemm_res_nch" [0] chunk buffers of its LDS ring: 0 = default (4 / 5 / 4 for the 32x32 / 64x32 / 64x64 tile: 128 KiB),
 *                                               up to 5 / 6 / 5 (160 KiB)
 *                            "gemm_splitk"  [0] deterministic two-pass split-K for underfilled grids with K >= 1536
 *                            "gemm_raster"  [0] tile order of the one-tile-per-workgroup kernels: 0 XCD x n-walk, 1 XCD x
 *                                               resident n-group, 2 row-major
 *                            "gemm_epi"     [1] LDS-transposed row-contiguous epilogue (0: direct per-lane stores)
 *   kernel selection, attention: "attn_impl" [1] 1 MFMA flash kernels, 0 exact generic kernel
 *                            "attn_split"   [1] split-key 4-wave kernel for <= 32 queries
 *                            "attn4_min_lq" [64] query count from which the 4-wave LDS-shared flash kernel is used
 *                            "attn_qg"      [1] 32-query groups per wave in that kernel (2: 64 queries per wave from 256 queries on)
 *   numerics / fusion:       "stream_T"     [1] T5 / ViT residual streams carried in the operand type (see VimaConfig)
 *                            "t5_fuse_rms"  [1] T5 RMSNorms folded into the neighbouring GEMMs
 *                            "vit_prune_last" [1] last ViT block evaluated for the cls row only (identical values)
 *                            "fp8_recalibrate" (any value) VIMA_PRECISION_FP8: the next pass of every group measures the activation scales again
 *                            "fp8_headroom_pct" [125] VIMA_PRECISION_FP8: scale = pct/100 x max |x| / 448 (>= 100); setting it re-calibrates
 *                            "kv_headmajor" [1] decoder prompt K / V written head-major ([B][2 heads][Lp][head dim]) where the projection runs on the
 *                                               persistent 256x256 GEMM (batch x prompt large enough): same values, contiguous reads in the cross attention
 *                            "geglu_pair"   [1] a GEGLU whose two products read the same input (the decoder blocks' MLP) as ONE GEMM launch over
 *                                               block-interleaved weights (128x128 ring tile, or the persistent 256x256 kernel's pair epilogue from 160 full
 *                                               tiles of the interleaved [M, 8E] problem on: 2048 rows at E = 768) where the grid is beyond the
 *                                               dual-accumulator form: same values
 *                            "ln_fuse"      [1] decoder LayerNorms (bf16 precisions): ln_2 of layer i and the query pre-LN of XAttention in layer i + 1 as ONE
 *                                               launch (bit-identical); the pre-LN in front of XAttention's feed-forward folded into the GEMMs either side of
 *                                               it (sums / sums of squares per 32 columns from attention_out's epilogue, mean / rstd applied to the GELU'd factor
 *                                               in the GEGLU pair's epilogue, gamma folded into the weight) where a pair form exists for the row count --
 *                                               the operand is then bf16(a) instead of bf16(LN(a)): same precision class, different rounding point
 *   rollouts:                "decode_ring"  [0] the episode caches' shared row index space is a ring (vima_decode_step): a batch steps without bound as long as
 *                                               every sample is restarted before ITS episode exceeds n_positions rows; setting it ends a running episode
 *                            "seq_ring"     [0] the same for the decoder-only policies (vima_seq_prefill / vima_seq_decode_step / vima_seq_decode_restart on GPT /
 *                                               GATO handles, where "decode_ring" is refused): the rows behind the prompt prefix are a ring and a restart gives a
 *                                               sample's rows back; setting it ends a running episode
 *                            "restart_batched" [1] vima_decode_restart rebuilds the prompt K / V of all flagged samples together (prompts of more than 32
 *                                               tokens); 0 = one sample at a time: same bits, launches proportional to the number of flagged samples
 *   scheduling:              "dual_stream"  [1] independent halves of the work on an auxiliary HIP stream
 *                            "graphs"       [0] replay the per-step entry points as captured hipGraphs
 *                            "vit_chunk"    [16384] crops per ViT pass
 *                            "dual_t5_rows" [0] 0 = automatic (two streams unless the batch is one nearly full round of 256x256 tiles, 14.4 k .. 21.8 k rows), > 0: batch x prompt length from which dual_stream splits the T5 stack over two streams; "dual_vit_crops" [8192] the same for the ViT's chunks (crops)
 *                            "t5_pad"       [1] the T5 stack is computed on the next multiple of 256 rows when batch x prompt length (>= 2048 rows per stream) is not one (zero pad rows, never read)
 *                            "vit_pad"      [1] ViT passes of >= 1024 crops are computed on a multiple of 256 crops (zero-image pad crops, never read) so their GEMMs stay on the 256-row tile kernels at any crop count
 *   test / instrumentation:  "op_bf16_out", "op_stream_T" (route vima_op_linear through the bf16-output / bf16-residual
 *                            epilogues; op_stream_T also feeds vima_op_layernorm a bf16 input), "op_bias_far" (vima_op_attention, T5 mode: promise
 *                            that the relbias table is constant from that |key - query| on, as the bucketed T5 table is from 91; 0 = no promise),
 *                            "gemm_dbg_ptr", "attn_dbg_ptr" (device buffers for shader-clock stamps, 0 = off)
 * Process-wide A/B switches read once from the environment (results do not depend on them beyond fp32 summation order inside
 * a LayerNorm row): VIMA_LN_ROWS2=0 (one-wave-per-row LayerNorm instead of the half-wave kernel), VIMA_VIT_ATTN_LDS=0 (per-thread
 * ViT attention instead of the LDS-staged kernel; identical bits), VIMA_GEMM_* (defaults of the GEMM options above),
 * VIMA_GEMM_NGROUP_KB (n-group size of the persistent GEMM's raster, default 2560). */
int vima_set_option(VimaHandle* h, const char* key, int64_t value);
/* When enabled every kernel launch is bracketed by HIP events on the launch stream and attributed to a class:
 * 0 = GEMM, 1 = attention, 2 = other. vima_prof_read synchronises and returns per class
 * {milliseconds, launches, algorithmic FLOPs (2*M*N*K for GEMMs, 4*B*H*Lq*Lk*D for attention)}; then resets. */
int vima_prof_enable(VimaHandle* h, int on);
int vima_prof_read(VimaHandle* h, double out_ms[3], int64_t out_launches[3], double out_flops[3]);
/* The same with the GEMM class split in two and the ALGORITHMIC HBM bytes of every GEMM launch (each operand, output and
 * epilogue input counted once): class 0 = GEMMs without, class 3 = GEMMs with an fp32-residual epilogue (read fp32
 * residual, write the fp32 stream [+ operand-type copy + RMS partials]: the HBM-heavy ones), 1 = attention, 2 = other. */
int vima_prof_read_ex(VimaHandle* h, double out_ms[4], int64_t out_launches[4], double out_flops[4], double out_bytes[4]);
/* The GEMM launches recorded since vima_prof_enable, grouped by the KERNEL the launcher chose: ids[i] = kind * 1000 +
 * (activation + 1) * 10 + epilogue (1 bf16 output, 2 GEGLU gate, 3 fp32 output +- residual, 4 bf16 residual stream, 5 bf16 output written head-major, 6 GEGLU pair over block-interleaved weights),
 * kind 1 gemm_pp_kernel<ACT, EPI>, 2 gemm_persistent_kernel<ACT, EPI>, 3 gemm_wide_kernel,
 * 4..7 gemm_kernel with the 256x256 / 128x128 / 64x64 / 32x64 tile (kind 5 with N = 8 x embed_dim: the block-interleaved GEGLU pair, two products per launch), 8 two-pass split-K, 10..12 gemm_resident_kernel with the
 * 32x32 / 64x32 / 64x64 tile (also the grouped launch of the action head's last layers), 15 / 16 its GEGLU-pair form (two products per launch:
 * 32x32 / 64x64 tile), 17 / 18 gemm_skinny_kernel (at most 32 rows) / its GEGLU-pair form, 21 gemm_kernel<float, ..., X3> (precision BF16X3: split-bf16
 * products, 128x128 tile), 23 two-pass split-K over it; per kernel the summed milliseconds,
 * launches, algorithmic FLOPs and algorithmic HBM bytes. Returns the number of kernels (<= max_n) or a negative error; does
 * NOT reset the records (call it before vima_prof_read / vima_prof_read_ex). */
int vima_prof_read_gemm_kernels(VimaHandle* h, int max_n, int32_t* ids, double* ms, int64_t* launches, double* flops, double* bytes);
/* The same records ONE BY ONE in launch order (ABI version 5): ids[i] as above, mnk[3 i .. 3 i + 2] = M, N, K of launch i, us[i] (may be
 * NULL) its HIP-event duration in microseconds. With "dual_stream" 0 the launch order is the dispatch order of a rocprofv3 trace of the
 * same call sequence, which is how scripts/pmc_summary.py attributes per-dispatch counter values to GEMM SHAPES. Returns the number of
 * recorded GEMM launches (it may exceed max_n: only the first max_n are written) or a negative error; does not reset the records. */
int vima_prof_read_gemm_launches(VimaHandle* h, int max_n, int32_t* ids, int32_t* mnk, float* us);
/* bytes currently held by the workspace arena */
int64_t vima_workspace_bytes(VimaHandle* h);
/* hipGraph replay (vima_set_option(h, "graphs", 1)): the per-env-step entry points (vima_obs_encode, vima_decode,
 * vima_decode_step, vima_action_head, vima_action_embed, vima_act) capture their launch sequence the second time the same call
 * (shapes, pointers, options) is seen and replay it afterwards -- at small batch a step is ~1300 microsecond kernels and
 * the host launch rate is the bound. Results are bit-identical to eager execution. Counts since handle creation. */
int vima_graph_stats(VimaHandle* h, int64_t* replays, int64_t* captures);

#ifdef __cplusplus
}
#endif
#endif /* VIMA_HIP_H */
