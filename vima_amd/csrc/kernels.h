// Launcher declarations for the hand-written gfx950 kernels (definitions in *.hip).
#pragma once
#include "common.h"

namespace vima {

// ---------------------------------------------------------------- GEMM (Tuning, GemmArgs: gemm_args.h; kernel selection: gemm_route.h)
// returns hipError_t as int; is_bf16 selects the operand type
int launch_gemm(const GemmArgs& a, bool is_bf16, hipStream_t st);
// CUs the persistent GEMM grids plan with (the device's count rounded down to a multiple of 8; queried once)
int num_cu();
// Bytes of split-K scratch this problem wants (0: single pass). Deterministic two-pass split-K: pass 1 = the same GEMM
// kernel over S K-ranges writing fp32 partials, pass 2 = gemm_reduce_kernel (sum in split order + the full epilogue).
size_t gemm_splitk_bytes(const GemmArgs& a, bool is_bf16);
int gemm_splitk_enabled(const Tuning* t);   // the effective split-K setting for a handle
int gemm_k_multiple(bool is_bf16);  // K must be a multiple of this
// What a caller asks BEFORE it builds a structured form. None of them keeps a rule of its own: each puts the canonical problem of its form to
// gemm_route() (gemm_route.h), the function launch_gemm itself routes with, so a "yes" here and a refusal there cannot drift apart.
int gemm_pair_large(const Tuning* t, long long M, long long Nout, long long K);   // ... and it will run on gemm_pp_kernel's pair epilogue (full 256x256 tiles that fill the chip)
int gemm_pair_ok(const Tuning* t, long long M, long long Nout, long long K);   // the block-interleaved GEGLU pair (GemmArgs::pair32) is the form to use for an [M, Nout] output
int gemm_lnfold_producer_ok(const Tuning* t, long long M, long long N);   // GemmArgs::sum_out is available for an [M, N] fp32 output with this handle's knobs
int gemm_dual_ok(const Tuning* t, int M, int N);   // the DUAL form (GemmArgs::W2) is available for an [M, N] output with this handle's knobs
int gemm_headmajor_ok(const Tuning* t, long long M, long long N, long long K, long long lda, long long ldw, int hm_D, int hm_L, int a8);   // GemmArgs::hm_D / hm_L usable for this problem
int gemm_a8_ok(const Tuning* t, long long M, long long N, long long K, long long lda, long long ldw);   // an fp8-ACTIVATION GEMM (GemmArgs::a8) of this shape is launchable with this handle's knobs
int gemm_grouped_ok(const Tuning* t);   // the grouped form (GemmArgs::grp_col) is available with this handle's knobs

// ---------------------------------------------------------------- normalisation / elementwise
// LayerNorm (rms=0: mean/var, affine) or T5 RMSNorm (rms=1: no mean, no bias). fp32 statistics.
// in: fp32 rows of length E at row stride ldin; outputs optional.
int launch_layernorm(const float* in, long long ldin, const float* gamma, const float* beta, float eps, int rms,
                     int rows, int E, float* out32, void* outT, bool is_bf16, hipStream_t st);
// two LayerNorms in a row: y = LN(in; gamma, beta) -> out32 / outT (both optional), z = LN(y; gamma2, beta2) -> out2T (operand type);
// bit-identical to launch_layernorm twice (the second on the fp32 y)
int launch_layernorm2(const float* in, long long ldin, const float* gamma, const float* beta, float eps, const float* gamma2,
                      const float* beta2, float eps2, int rows, int E, float* out32, void* outT, void* out2T, bool is_bf16, hipStream_t st);
// the same with the input rows in the operand type T (residual stream carried in T)
// out8 (bf16 mode only): additionally (or, with outT == nullptr, only) the fp8 e4m3 copy e4m3(result * inv8), row stride E bytes
int launch_layernorm_T(const void* inT, long long ldin, const float* gamma, const float* beta, float eps, int rms, int rows,
                       int E, float* out32, void* outT, bool is_bf16, hipStream_t st, void* out8 = nullptr, float inv8 = 1.0f);
int launch_cast(const float* in, void* outT, long long n, bool is_bf16, hipStream_t st);
// fp8 activations (precision "fp8"): out8[r][c] = e4m3(in[r][c] * inv) of bf16 rows (saturating at 448; cols, strides % 8 == 0);
// *slot = max(*slot, max |in|) (slot holds a non-negative float, zero it before the first call)
int launch_quant_fp8(const void* inT, long long ldin, long long rows, int cols, float inv, void* out8, long long ldo, hipStream_t st);
int launch_amax(const void* inT, long long ldin, long long rows, int cols, float* slot, hipStream_t st);
// operand-type copy of fp32 rows + their sum of squares (entry point of the fused-RMSNorm chain): outT[r][:] = in[r][:],
// ssq[r] = sum in[r][:]^2
int launch_rms_stats(const float* in, int rows, int E, void* outT, float* ssq, bool is_bf16, hipStream_t st);

// uint8 crops [M,3,32,32] -> normalised patch matrix T [M*4, 768], k = c*256 + py*16 + px (conv1 weight order)
int launch_patchify(const uint8_t* crops, void* outT, int M, bool is_bf16, hipStream_t st);
// tokens = LN_pre(concat(cls, patches) + pos): pre fp32 [M*4,768] -> x fp32 [M*5,768] and / or xT (operand type)
int launch_vit_embed(const float* pre, const float* cls, const float* pos, const float* g, const float* b,
                     float* x, void* xT, int M, bool is_bf16, hipStream_t st);
// first bbox-MLP layer: relu(W[768,4] . (bbox/[256,128,128,256]) + b) -> T [R,768]
int launch_bbox_l1(const long long* bbox, const float* W, const float* b, void* outT, int R, int Nout,
                   bool is_bf16, hipStream_t st);
// first action-embedding layer for one key: x = idx / bins ; relu(W[256,K] x + b) -> T [R, ldo] at column col0
int launch_action_l1(const long long* idx, int K, const float* W, const float* b, void* outT, int R, int ldo,
                     int col0, bool is_bf16, hipStream_t st);
// action selection (action_select.hip), one launch per batch of rows: logits f32 [R,700] -> per segment (kHeadBins) the mode (first
// index of the maximum) or, with u f32 [R,12], the inverse-CDF sample; idx[k] i64 [R,2|4] in the layout launch_action_l1 reads;
// optional cont f32 [R,12] = bin / bins (has_bounds: positions clamp(x * (high - low) + low, low, high), rotations clamp(x * 2 - 1,
// -1, 1), each operation rounded on its own), logp / ent f32 [R,4] per key; with t1 (operand type [R,1024]) also the first
// action-embedding layer of the four keys (w0[k] f32 [256, 2|4], b0[k] f32 [256]), bit-identical to launch_action_l1 on idx
struct ActSelectArgs {
  const float* logits = nullptr;
  const float* u = nullptr;
  int R = 0;
  int has_bounds = 0;
  float low[2] = {0.f, 0.f}, high[2] = {1.f, 1.f};
  long long* idx[4] = {nullptr, nullptr, nullptr, nullptr};
  float* cont = nullptr;
  float* logp = nullptr;
  float* ent = nullptr;
  void* t1 = nullptr;
  const float* w0[4] = {nullptr, nullptr, nullptr, nullptr};
  const float* b0[4] = {nullptr, nullptr, nullptr, nullptr};
};
int launch_act_select(const ActSelectArgs& a, bool is_bf16, hipStream_t st);
// action selection with sampling controls (action_sample.hip, act_sample_kernel): sel as above with sel.R = R * S OUTPUT rows, output
// row r * S + s reading logits row r and u[r * S + s]; temp f32 [R] (device, or null = 1; clamped to [1e-4, 1e4], NaN = 1) divides the
// logits, top_k (<= 0 or >= n: off) and top_p (>= 1: off; > 0) truncate every segment (ranks by exact comparison, ties to the lower
// index; top-p after top-k), log-probability and entropy are those of the truncated distribution. given: sel.idx are INPUTS (clamped
// to [0, n), not written), nothing is selected and sel.u is ignored. With every control off: the outputs of launch_act_select, bit for bit
struct ActSampleArgs {
  ActSelectArgs sel;
  const float* temp = nullptr;
  int top_k = 0;
  float top_p = 1.0f;
  int S = 1;
  int given = 0;
};
int launch_act_sample(const ActSampleArgs& p, bool is_bf16, hipStream_t st);
// out[r, :] += table[sel[r / group]][:]   (obs_fusion end-effector term)
int launch_add_row_table(float* out, int rows, int E, const float* table, const long long* sel, int group,
                         hipStream_t st);
// prompt assembly: x[b,l,:] = word table row / object token / 0 ; mask likewise
int launch_prompt_assemble(const int* tok_src, const long long* word_ids, const float* word_table,
                           const float* obj_tokens, const uint8_t* obj_mask, float* x, uint8_t* mask, int rows,
                           int E, hipStream_t st);
// the same gather as the entry of the T5 stack's fused-RMSNorm chain: operand-type rows xT [rows, E] + ssq[r] = sum xT-source[r][:]^2 (what
// launch_rms_stats would produce from the fp32 rows, bit for bit) + mask; the fp32 prompt is not materialised
int launch_prompt_assemble_stats(const int* tok_src, const long long* word_ids, const float* word_table, const float* obj_tokens,
                                 const uint8_t* obj_mask, void* xT, float* ssq, uint8_t* mask, int rows, int E, bool is_bf16, hipStream_t st);
// decoder input: interleave [o_1..o_Q, a] per step, cumsum position ids, + positions_embed
int launch_dec_embed(const float* obs_tok, const uint8_t* obs_mask, const float* act_tok, const float* pos_table,
                     int n_pos, float* x32, void* xT, uint8_t* mask, int T, int B, int Q, int L_act, int E,
                     bool is_bf16, hipStream_t st);
// T >= 1 env steps of incremental decoding in one pass (vima_decode_step is T = 1): obs_tok [T,B,Q,E], obs_mask [T,B,Q], act_tok [T,B,E] (has_act)
// or [T-1,B,E] (batch step 0: the first slot has no action row) -> x32 / xT [B, Ln, E], Ln = T (Q + 1) - (1 - has_act) <= 512 rows = the slots
// [action, Q obs] back to back; position ids continue poscnt[b]; hist_mask[b][row0 + l], poscnt[b] and fresh[b] (first slot only; optional: nullptr
// = no sample is fresh) are updated
int launch_dec_embed_chunk(const float* obs_tok, const uint8_t* obs_mask, const float* act_tok, const float* pos_table, int n_pos,
                           float* x32, void* xT, uint8_t* hist_mask, int* poscnt, int row0, int Lmax, int T, int B, int Q,
                           int has_act, int E, bool is_bf16, hipStream_t st, uint8_t* fresh);
// prompt + xattn_positions_embed[cumsum(mask)-1] -> T [B*Lp, E]; input strides in elements (seq-first views ok)
// list (DEVICE array [B], optional): output block r is computed from sample list[r] of prompt / mask instead of sample r
int launch_prompt_pos(const float* prompt, long long sb, long long sl, const uint8_t* mask, const float* pos_table,
                      int n_pos, void* outT, int B, int Lp, int E, bool is_bf16, hipStream_t st, const int* list = nullptr);
// out[r][l] = in[list[r]][l], r < n: rows of a byte mask [B][L] by a sample list (DEVICE array)
int launch_mask_rows_gather(const uint8_t* in, uint8_t* out, const int* list, int n, int L, hipStream_t st);
// out[t,b,:] = x[b, lead + (Q-1) + (Q+1) t, :]; lead = 1 when every slot of Q + 1 rows starts with an action row (a chunk behind batch step 0)
int launch_gather_pred(const float* x, float* out, int T, int B, int Q, int Lq, int E, hipStream_t st, int lead = 0);

// ---- baseline policies (baseline_kernels.hip): whole RGB frames, decoder-only sequences
// uint8 frames [M,3,H,W] -> normalised patch matrix T [M*(H/P)*(W/P), 3*P*P], k = c*P*P + py*P + px
int launch_patchify_rect(const uint8_t* img, void* outT, int M, int H, int W, int P, bool is_bf16, hipStream_t st);
// tokens = LN_pre(concat([cls,] patches) + pos): pre fp32 [M*n_patch,768] -> x fp32 [M*S,768] and / or xT; cls == nullptr: S = n_patch
int launch_vit_embed_rect(const float* pre, const float* cls, const float* pos, const float* g, const float* b, float* x, void* xT,
                          int M, int S, int n_patch, bool is_bf16, hipStream_t st);
// out[r,:] = src[r % period,:] (fp32)
int launch_broadcast_rows(const float* src, float* out, long long rows, int E, int period, hipStream_t st);
// incremental decoding of the decoder-only policies. Episode state on the device: cache_mask [B][n_pos] (key mask at the cache's row stride),
// posbase[b] (position id of sample b's next valid row), fresh[b] (1 after a restart: the next action slot is absent).
// decoder-only input [B,L,E]: [prompt | sep | (Q obs tokens, action)*] + positions_embed, key mask [B,L]; block r comes from sample list[r] of
// prompt / pmask (DEVICE array, optional: identity). With cache_mask / posbase (the prefill of an episode: L = Lp + 1, no obs_tok / act_tok) the
// episode state of that sample is written too: cache_mask[.][0 .. Lp] at row stride cache_ld and posbase (= valid prompt tokens + 1)
int launch_seq_embed(const float* prompt, long long sb, long long sl, const uint8_t* pmask, const float* sep, const float* obs_tok,
                     const float* act_tok, const float* pos_table, int n_pos, float* x32, void* xT, uint8_t* mask, int B, int L, int Lp,
                     int Q, int E, bool is_bf16, hipStream_t st, const int* list = nullptr, uint8_t* cache_mask = nullptr, int* posbase = nullptr,
                     int cache_ld = 0);
// the rows of T >= 1 env steps as one chunk (vima_seq_decode_step is T = 1): T (Q + 1) rows per sample (one fewer without has_act: the first slot of
// batch step 0 has no action row) at cache rows [row0, ..); obs_tok [T, B, Q, E], act_tok [T, B, E] (has_act) / [T - 1, B, E] -> x32 / xT; positions
// continue posbase[b]; cache_mask[b][row0 + i] and posbase[b] are updated, fresh[b] is consumed (a fresh sample's first action row: zeros, key
// mask 0, no position id). No row limit beyond row0 + rows <= n_pos.
int launch_seq_embed_chunk(const float* obs_tok, const float* act_tok, const float* pos_table, int n_pos, float* x32, void* xT,
                           uint8_t* cache_mask, int* posbase, uint8_t* fresh, int row0, int T, int B, int Q, int has_act, int E, bool is_bf16,
                           hipStream_t st);
int launch_fill_u8(uint8_t* p, long long n, uint8_t v, hipStream_t st);

// ---- episode caches, both policy families (episode_rows.hip)
// Rows between a compact buffer and the samples' blocks of a cache, one launch: 16-byte vectors, grid (vectors of a sample, n)
struct KvRowsArgs {
  const void* in = nullptr;
  void* out = nullptr;
  const int* list = nullptr;     // DEVICE [n]: cache block of compact sample r (nullptr: r)
  const int* rowmap = nullptr;   // DEVICE [L]: cache row of compact row l, shared by the samples (nullptr: l)
  int n = 0, L = 0, N = 0;       // compact side: n samples x L rows x N elements ...
  long long ld = 0;              // ... at this leading dimension (>= N)
  int Lc = 0;                    // rows per sample block of the cache (block = Lc * N elements)
  int D = 0;                     // > 0: block is head-major [N / D][Lc][D]; 0: row-major [Lc][N]
  bool to_cache = true;          // compact -> cache (scatter / store) or cache -> compact (gather)
};
// hipErrorInvalidValue when N, ld or D is no whole number of 16-byte vectors, N % D != 0, ld < N, L > Lc, n > 65535 or a buffer is misaligned
int launch_kv_rows(const KvRowsArgs& a, int elem_bytes, hipStream_t st);
// for the n listed samples (DEVICE array): mask[b][lo .. hi) = 0, fresh[b] = 1 (consumed by the next chunk's embedding), poscnt[b] = 0 (optional)
int launch_episode_restart(const int* list, int n, uint8_t* mask, int* poscnt, uint8_t* fresh, int lo, int hi, int Lmax, hipStream_t st);
// installed history of the n listed samples: cache_mask[list[r]][lo .. hi) = 0, then cache_mask[list[r]][rowmap[l]] = mask[r][l] (l < L),
// poscnt[list[r]] = the number of valid rows, fresh[list[r]] = 0
int launch_history_install(const uint8_t* mask, const int* list, const int* rowmap, int n, int L, int lo, int hi, int Lmax, uint8_t* cache_mask,
                           int* poscnt, uint8_t* fresh, hipStream_t st);

// ---- episode fork (episode_fork.hip): a sample's episode state copied into other batch slots, in place
// One job = one row range [row0, row0 + nrows) of sample `src`, copied to the ndst samples dsts[dst0 ..) in EVERY layer of a cache [NL][B][L][N]:
// the range is one contiguous span per layer, cut into chunks of kForkChunk 16-byte vectors; unit0 = the chunks of the jobs in front of it
// (per layer), so that a flat unit number finds its job by bisection.
struct ForkJob { int src, dst0, ndst, row0, nrows, unit0; };
constexpr int kForkChunk = 1024;   // 16-byte vectors per work unit: 256 threads x 4
constexpr int kForkMaxDst = 8;     // a source with more destinations is split into jobs of at most this many (more units, the source read once per job)
struct EpisodeForkArgs {
  void* cache = nullptr;            // [NL][B][L][N], operand type
  const ForkJob* jobs = nullptr;    // DEVICE [n_jobs], nrows > 0, unit0 ascending
  const int* dsts = nullptr;        // DEVICE
  int n_jobs = 0, units = 0;        // units: chunks of all jobs in one layer
  int NL = 0, B = 0, L = 0, N = 0;
};
// A workgroup loads a chunk of the source span once (dwordx4) and stores it to every destination of the job. Sources and destinations must be disjoint
// sets (EpisodeBook::fork_ok). hipErrorInvalidValue (1) for a bad shape, 22 when N * sizeof(element) is no multiple of 16. The grid is
// min(NL * units, 2048) workgroups, whatever B
int launch_episode_fork(const EpisodeForkArgs& a, bool is_bf16, hipStream_t st);
// per-sample episode state of n (destination, source) pairs (DEVICE arrays): the whole key-mask row [Lmax], the position counter and the fresh flag
int launch_episode_fork_state(const int* dsts, const int* srcs, int n, uint8_t* mask, int* poscnt, uint8_t* fresh, int Lmax, hipStream_t st);

// ---- episode snapshots (episode_snapshot.hip): a sample's episode rows packed into / unpacked from a caller's payload, in compact time order
// One job = nrows compact rows of one sample in EVERY layer of a cache [NL][B][L][N]: compact row k of the job is cache row map[map0 + k] (map ==
// nullptr: row map0 + k) and sits at payload + layer * layer_stride + k * N elements. A work unit = rpc whole rows of one (layer, job); unit0 =
// the units of the jobs in front of it (per layer), so that a flat unit number finds its job by bisection.
struct SnapJob { long long payload, layer_stride; int sample, map0, nrows, unit0; };   // payload: DEVICE address, layer_stride in bytes
constexpr int kSnapChunk = 1024;   // 16-byte vectors a workgroup keeps in flight: 256 threads x 4
struct EpisodeSnapArgs {
  void* cache = nullptr;            // [NL][B][L][N], operand type
  const SnapJob* jobs = nullptr;    // DEVICE [n_jobs], nrows > 0, unit0 ascending
  const int* map = nullptr;         // DEVICE row table of the call (every entry in [0, L): the caller checks), or nullptr
  int n_jobs = 0, units = 0;        // units: of all jobs in one layer
  int NL = 0, B = 0, L = 0, N = 0;
  int D = 0;                        // > 0: the sample's block is head-major [N / D][L][D] (the prompt K / V cache under kv_headmajor); 0: rows [L][N]
  int rpc = 1;                      // rows per unit: max(1, kSnapChunk / (16-byte vectors per row))
};
inline int snap_rows_per_unit(long long row_vectors) { return row_vectors >= kSnapChunk ? 1 : (int)(kSnapChunk / row_vectors); }
// hipErrorInvalidValue (1) for a bad shape, 22 when N (or D) * sizeof(element) is no multiple of 16 or the cache is misaligned. The grid is
// min(NL * units, 2048) workgroups. pack reads the cache and writes the payloads, unpack the reverse; jobs of one unpack call name distinct samples
int launch_episode_pack(const EpisodeSnapArgs& a, bool is_bf16, hipStream_t st);
int launch_episode_unpack(const EpisodeSnapArgs& a, bool is_bf16, hipStream_t st);
// The per-sample state of n pairs, one workgroup each. The payload starts with 16 bytes {position counter, fresh flag, rows, 0} (int32), followed by
// npre + nrows key-mask bytes: those of cache rows [0, npre) and of rows map[map0 + k]. Unpack first clears the slot's mask row over [lo, hi).
struct SnapStateJob { long long payload; int sample, map0, nrows, npre; };
int launch_episode_pack_state(const SnapStateJob* jobs, int n, const int* map, const uint8_t* mask, const int* poscnt, const uint8_t* fresh, int Lmax,
                              hipStream_t st);
int launch_episode_unpack_state(const SnapStateJob* jobs, int n, const int* map, uint8_t* mask, int* poscnt, uint8_t* fresh, int Lmax, int lo, int hi,
                                hipStream_t st);

// ---------------------------------------------------------------- attention
// ViT: 5-token (S <= 8) multi-head attention on packed qkv T [M*S, 3*W] -> T [M*S, W]; head dim 32
// out8 (bf16 mode): write the result as fp8 e4m3(value * inv8) [M*S, W] bytes INSTEAD of the operand-type output
// force (vima_op_vit_attention's A/B): 0 the launcher's own choice, 1 the register kernel with the instantiation S asks for (never the
// LDS-staged one), 2 the register kernel's 16-score instantiation whatever S
int launch_vit_attn(const void* qkv, void* out, int M, int S, int W, int heads, bool is_bf16, hipStream_t st, void* out8 = nullptr, float inv8 = 1.0f,
                    int force = 0);
// last ViT block: cls-token query only. q T [M, W], kv T [M*S, 2W] -> out T [M, W]
int launch_vit_attn_cls(const void* q, const void* kv, void* out, int M, int S, int W, int heads, bool is_bf16, hipStream_t st,
                        void* out8 = nullptr, float inv8 = 1.0f);

enum AttnMode : int { ATTN_T5 = 0, ATTN_CROSS = 1, ATTN_CAUSAL = 2 };
struct AttnArgs {
  const void* q = nullptr; int ldq = 0;   // row (b*Lq + i), head h at column h*D
  const void* k = nullptr; int ldk = 0;   // row (b*Lk + j)
  const void* v = nullptr; int ldv = 0;
  void* out = nullptr; int ldo = 0;
  const uint8_t* kmask = nullptr;         // [B, Lk] 1 = attend; masked keys get score finfo(fp32).min
  const float* relbias = nullptr;         // T5: [H][2*Lk-1], index (j - i) + Lk - 1
  int bias_far = 0;                       // T5: > 0 promises that relbias[h] is CONSTANT for j - i >= bias_far and for j - i <= -bias_far (the bucketed
                                          // T5 table is, from |j - i| = 91 on): key tiles wholly beyond it take the constant instead of per-score reads
  int B = 0, H = 0, Lq = 0, Lk = 0, D = 0;
  // K / V addressing: element (b, h, j, d) of K sits at k + b * k_bs + h * k_hs + j * ldk + d (V likewise). 0 = the default layout, rows
  // (b * Lk_rows + j) of width ldk with the heads side by side: k_bs = Lk_rows * ldk, k_hs = D. A head-major cache ([B][heads][Lk][D]: ldk = D,
  // k_hs = Lk * D, k_bs = heads * Lk * D) is read with every (batch, head)'s keys contiguous.
  long long k_bs = 0, v_bs = 0;
  int k_hs = 0, v_hs = 0;
  float scale = 1.0f;
  int mode = ATTN_CROSS;
  // incremental decoding (keys / values / key mask live in an episode cache with room for Lk_rows >= Lk rows per sample,
  // the queries are the newest tokens): K/V row = b * Lk_rows + j, mask = kmask[b * Lk_rows + j] (0 -> Lk), and the causal
  // rule compares key j with the query's GLOBAL position i + q_off.
  int Lk_rows = 0;
  int q_off = 0;
  // RING episode cache (option decode_ring): the step's rows are [q_off, q_off + Lq) = [q_off, win_end) of a ring image of Lk rows and key j is
  // "future" for query i iff i + q_off < j < win_end -- rows from win_end on hold OLDER history of the episode. 0 = Lk: the plain causal rule.
  int win_end = 0;
  const Tuning* tune = nullptr;   // the calling handle's knobs (nullptr: process defaults)
};
// generic exact kernel (any T); the MFMA flash kernel (bf16, D in {32,64})
int launch_attn_generic(const AttnArgs& a, bool is_bf16, hipStream_t st);
int launch_attn_mfma(const AttnArgs& a, hipStream_t st);
// precision "bf16x3": fp32 operands, split-bf16 products on the matrix cores (D in {32,64}; attn_mfma_kernel<D, MODE, X3 = true>, always the one-wave kernel)
int launch_attn_x3(const AttnArgs& a, hipStream_t st);

}  // namespace vima
