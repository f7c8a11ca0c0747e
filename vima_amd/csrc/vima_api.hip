// Host orchestration + C ABI (include/vima_hip.h) of the MI355X-native VIMA policy forward pass.
// One VimaHandle = packed weights + workspace arena for one (model, device). Every policy method is a fixed
// sequence of hand-written gfx950 kernels (gemm.hip / attention.hip / elementwise.hip) on the caller's stream.
#include "../../include/vima_hip.h"
#include "kernels.h"
#include "episode_book.h"

#include <math.h>
#include <stdio.h>
#include <string.h>

#include <map>
#include <set>
#include <unordered_map>
#include <string>
#include <vector>

using namespace vima;

namespace {

thread_local std::string g_err;

int fail(const std::string& m, int code = 1) {
  g_err = m;
  return code ? code : 1;
}

#define HIPCK(expr)                                                                                   \
  do {                                                                                                \
    hipError_t e__ = (expr);                                                                          \
    if (e__ != hipSuccess)                                                                            \
      return fail(std::string(#expr) + ": " + hipGetErrorString(e__), (int)e__);                      \
  } while (0)

#define KCK(expr)                                                                                     \
  do {                                                                                                \
    int e__ = (expr);                                                                                 \
    if (e__ != 0)                                                                                     \
      return fail(std::string(#expr) + ": " + hipGetErrorString((hipError_t)e__) + " @" + __func__, e__); \
  } while (0)

}  // namespace
namespace vima {
int api_fail(const std::string& m) { return fail(m); }   // for the other translation units of the C ABI (comm.hip)

// precision "fp8": freeze the dequantisation scales of a site group from the calibrating pass's max |x|: a non-finite maximum
// (an inf / NaN activation in the calibrating batch) is REFUSED -- scale = inf would zero every later activation of the site --, a dead site
// (max 0) gets scale 1, every other site headroom x max / 448. Returns 0, or the failure code with the handle left uncalibrated.
int fp8_scales_from_amax(const std::vector<float>& am, int headroom_pct, const char* group, std::vector<float>& out) {
  const float hr = (headroom_pct >= 100 ? headroom_pct : 100) * 0.01f;
  std::vector<float> sc(am.size());
  for (size_t i = 0; i < am.size(); ++i) {
    if (!std::isfinite(am[i])) {
      char buf[160];
      snprintf(buf, sizeof buf, "precision fp8: calibration of %s site %zu saw a non-finite activation (max |x| = %g); the scales were NOT frozen -- "
               "fix the input and call again", group, i, (double)am[i]);
      return fail(buf);
    }
    sc[i] = am[i] > 0.f ? am[i] * hr / 448.0f : 1.0f;
  }
  out.swap(sc);
  return 0;
}
}
namespace {

constexpr int kVitW = 768, kVitLayers = 4, kVitHeads = 24;
constexpr int kT5Layers = 12, kT5Heads = 12, kT5D = 64, kT5FF = 3072, kT5Model = 768, kT5Buckets = 32;
constexpr int kVocab = 32128;
constexpr int kHeadHidden = 512, kNumHeadsOut = 12, kLogits = 700;
const int kHeadBins[kNumHeadsOut] = {50, 100, 50, 50, 50, 50, 50, 100, 50, 50, 50, 50};
const char* kViews[2] = {"front", "top"};
const char* kActKeys[4] = {"pose0_position", "pose0_rotation", "pose1_position", "pose1_rotation"};
const int kActDims[4] = {2, 4, 2, 4};

// HF modeling_t5._relative_position_bucket, bidirectional, 32 buckets, max distance 128 (fp32 log like torch)
int t5_bucket(int rel) {
  const int nb = 16, max_exact = 8;
  int out = rel > 0 ? nb : 0;
  int n = rel < 0 ? -rel : rel;
  if (n < max_exact) return out + n;
  const float ratio = (float)n / (float)max_exact;
  const float v = logf(ratio) / (float)log(128.0 / 8.0) * (float)(nb - max_exact);
  int large = max_exact + (int)v;
  if (large > nb - 1) large = nb - 1;
  return out + large;
}

struct HostParam {
  std::vector<float> data;
  std::vector<int64_t> shape;
};

struct Lin {            // packed nn.Linear-layout weight [N,K] (+ optional fp32 bias [N]): operand type T, or -- precision
  void* W = nullptr;    // "fp8w", large matrices -- OCP e4m3 bytes with one fp32 dequantisation scale per output channel
  float* b = nullptr;
  int N = 0, K = 0;
  float* ws = nullptr;  // [N] scales; non-null <=> W holds fp8
  float* c = nullptr;   // [N] fused LayerNorm (GemmArgs::rs_c): sum_k of the ROUNDED operand values of row n of W = W0 diag(gamma)
};

// fp32 -> OCP FP8 E4M3 (e4m3fn: bias 7, no infinities, max 448), round to nearest even, saturating. Host side of the fp8w
// weight format (the device side is v_cvt_pk_f32_fp8 in gemm.hip); exported as vima_fp8_e4m3_encode for the tests.
uint8_t f32_to_e4m3(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  const uint8_t sgn = (uint8_t)((u >> 24) & 0x80);
  const float a = fabsf(f);
  if (!(a == a)) return (uint8_t)(sgn | 0x7f);
  if (a >= 464.0f) return (uint8_t)(sgn | 0x7e);                 // beyond the rounding range of 448: saturate
  if (a < 0.015625f) return (uint8_t)(sgn | (uint8_t)(int)nearbyintf(a * 512.0f));   // subnormals: multiples of 2^-9 (8 -> 2^-6)
  int e;
  const float fr = frexpf(a, &e);                                // a = fr * 2^e, fr in [0.5, 1)
  int E = e - 1;
  int m = (int)nearbyintf((fr * 2.0f - 1.0f) * 8.0f);            // 3 mantissa bits, ties to even
  if (m == 8) { m = 0; ++E; }
  int code = ((E + 7) << 3) | m;
  if (code > 0x7e) code = 0x7e;
  return (uint8_t)(sgn | code);
}
inline bool fp8_eligible(int N, int K) { return K % 64 == 0 && N % 4 == 0 && (long long)N * K >= 65536; }

struct Arena {          // stream-ordered bump allocator; chunks are only released at reset()
  struct Chunk { char* p; size_t cap; };
  std::vector<Chunk> chunks;
  size_t used = 0;      // in the last chunk
  size_t total_need = 0;
  uint64_t gen = 0;     // bumped whenever a chunk is allocated or freed (addresses baked into captured graphs go stale)
  int reset() {
    if (chunks.size() > 1) {   // consolidate so steady state is a single allocation
      size_t tot = 0;
      for (auto& c : chunks) tot += c.cap;
      if (hipDeviceSynchronize() != hipSuccess) return 1;
      for (auto& c : chunks) (void)hipFree(c.p);
      chunks.clear();
      ++gen;
      char* p = nullptr;
      if (hipMalloc((void**)&p, tot) != hipSuccess) return 1;
      chunks.push_back({p, tot});
    }
    used = 0;
    return 0;
  }
  void* alloc(size_t bytes) {
    bytes = (bytes + 255) & ~(size_t)255;
    if (bytes == 0) bytes = 256;
    if (chunks.empty() || used + bytes > chunks.back().cap) {
      size_t cap = bytes > ((size_t)64 << 20) ? bytes : ((size_t)64 << 20);
      char* p = nullptr;
      if (hipMalloc((void**)&p, cap) != hipSuccess) return nullptr;
      chunks.push_back({p, cap});
      ++gen;
      used = 0;
    }
    void* r = chunks.back().p + used;
    used += bytes;
    return r;
  }
  size_t bytes() const {
    size_t t = 0;
    for (auto& c : chunks) t += c.cap;
    return t;
  }
  void release() {
    for (auto& c : chunks) (void)hipFree(c.p);
    chunks.clear();
  }
};

// precision "fp8": one group of activation sites with static e4m3 dequantisation scales (headroom x max |x| of the calibrating pass / 448). The group's first
// eligible pass runs on operand-type activations and records max |x| per site (cal_begin .. cal_freeze, below the handle); later passes take the scales.
struct Fp8Cal {
  const char* group;
  int sites;
  bool ready = false;
  std::vector<float> scale;   // [sites], valid while ready
  float* amax = nullptr;      // device [sites], allocated by the first calibrating pass
};
enum { CAL_T5 = 0, CAL_VIT = 1, CAL_KV = 2 };

struct ProfRec { int cls; hipEvent_t a, b; double flops; double bytes; int kid = 0; int M = 0, N = 0, K = 0; };   // kid: GemmArgs::kernel_id of a GEMM launch (M, N, K: its shape)

}  // namespace

struct VimaHandle {
  VimaConfig cfg;
  int device = 0;
  bool bf16 = true;
  bool x3 = false;          // precision "bf16x3": the fp32 path (bf16 = false) with split-bf16 GEMMs and MFMA attention
  bool w8 = false;          // precision "fp8w" / "fp8": fp8 e4m3 weights (+ per-output-channel scales) for the large Linear layers
  // precision "fp8": the T5 stack's GEMMs ALSO take fp8 e4m3 activations with one static scale per (layer, site) and run on
  // v_mfma_scale_f32_32x32x64_f8f6f4 (gemm_pp_kernel<.., F8>). Scales are calibrated by the first T5 pass of the handle (which runs
  // the fp8w kernels and records max |x| per site); sites per layer: 0 stream before qkv, 1 attention context, 2 stream before
  // wi, 3 ReLU hidden.
  bool a8 = false;
  // the same for the ViT (chunks of >= 13824 crops: sites per block 0 ln_1 output, 1 attention output, 2 ln_2 output, 3 QuickGELU
  // hidden) and for the decoder's prompt K/V projection (one site: prompt + position embedding)
  Fp8Cal cal8[3] = {{"T5", kT5Layers * 4}, {"ViT", kVitLayers * 4}, {"prompt K/V", 1}};   // CAL_T5, CAL_VIT, CAL_KV: the group numbers of vima_fp8_act_scales
  int fp8_headroom_pct = 125;        // option "fp8_headroom_pct": a site's scale = headroom x (max |x| of the calibrating batch) / 448, so that a later
                                     // activation up to `headroom` x larger than anything the calibrating batch held still maps below the e4m3 maximum
                                     // instead of saturating (e4m3 is a floating-point format: headroom costs no relative precision above its subnormals)
  bool finalized = false;
  int attn_impl = 1;
  Tuning tune;              // GEMM / attention kernel-selection knobs of THIS handle (travel with every launch)
  int vit_chunk = 16384;
  int dual_t5_rows = 0;                           // option "dual_t5_rows": batch x prompt length from which the T5 stack splits the batch over two streams (with dual_stream)
  int dual_vit_crops = 8192;                      // option "dual_vit_crops": crop count from which the ViT alternates its chunks between two streams (with dual_stream). 8192: the 2 048
                                                  // observation crops of a batch-256 env step as two 1 024-crop chunks on two streams were 4 % SLOWER than one pass (warm step 4.11 -> 3.93 ms,
                                                  // incremental 4.58 -> 4.44; batch-16 prompts 5.97 -> 5.86); from 16 384 crops on the split pays (profiles/r06_dual_stream_thresholds.txt)
  int t5_pad = 1;                                 // option "t5_pad": the T5 stack's GEMMs run on the next multiple of 256 rows (pad rows: zeros in, never read) when B * L is not one
  int vit_pad = 1;                                // option "vit_pad": ViT chunks of >= 1024 crops run on a multiple of 256 crops (pad crops computed and never read), so that their
                                                 // GEMMs keep the 256x256 kernels at ANY crop count (a chunk of 13 654 crops: 57.8 -> 53.5 ms on the headline workload)
  int vit_prune_last = 1;   // compute the last ViT block only for the cls token (only row ln_post reads)
  int stream_T = 1;         // residual stream of the T5 stack carried in the operand type (bf16) instead of fp32 + bf16 copy:
                            // 4 instead of 10 bytes of HBM traffic per element and residual GEMM; measured effect on the
                            // logits 1.5e-4. 0 = fp32 stream (round-1 behaviour)
  int t5_fuse_rms = 1;      // T5 RMSNorms folded into the neighbouring GEMMs (statistics in the producer epilogue, row scale in the consumer)
  int op_bf16_out = 0;      // vima_op_linear: route the result through the operand-type output (tests the T store paths)
  int op_stream_T = 0;      // vima_op_linear: pass `res` in the operand type (resT) like the T5 / ViT residual GEMMs do; vima_op_layernorm: bf16 input
  int dual_stream = 1;      // split independent work over two HIP streams so that HBM-bound kernels (norms, attention,
                            // GEMM epilogues) of one half overlap the MFMA-bound GEMM main loops of the other half
  hipStream_t aux = nullptr;
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  std::vector<hipEvent_t> ev_layer;   // per decoder layer: "prompt K/V of layer i projected" (aux -> main)
  // cross-step prompt K/V cache: per-layer key_value(prompt + pos-emb) (components.py:175) is loop-invariant across the env
  // steps of an episode. Built by kv_cache_mode 1 (full-history vima_decode, step 0 of an episode) for B samples of Lp rows; hm: its layout as
  // built, [B][2 Hx][Lp][D] instead of [B * Lp][2E]
  struct PromptKV { void* ptr = nullptr; size_t bytes = 0; int B = 0, Lp = 0; bool valid = false, hm = false; } pkv;
  // The episode batch of incremental decoding (vima_decode_step on VIMA / Flamingo handles, vima_seq_prefill / vima_seq_decode_step on GPT / GATO
  // handles; a handle runs one family only): per-layer self-attention K | V of the history [NL][B][Lmax][2E] (operand type), its key mask
  // [B][Lmax], the per-sample count of valid tokens (next position id) and fresh [B], 1 = the sample was restarted: its next step has no previous
  // action. book: the ONE row index space of the caches behind the fixed prefix (XAttnGPT: none; GPT / GATO: prompt + separator), linear or a
  // ring (options "decode_ring" / "seq_ring"): write pointer, high-water mark, next batch step, per-sample ages and the slot record
  // (episode_book.h). live: a batch is running and the book is valid -- false from a step-0 decode_prepare until decode_commit, and from the
  // start of vima_seq_prefill until its end; ep_running() is the one check of it
  struct Episode {
    void* kv = nullptr; size_t kv_bytes = 0;
    uint8_t* mask = nullptr; int* poscnt = nullptr; size_t aux_cap = 0;
    uint8_t* fresh = nullptr;
    int B = 0, Q = 0, Lp = 0, Lmax = 0;
    bool live = false;
    EpisodeBook book;
  } ep;
  int seq_ring = 0, decode_ring = 0;
  int restart_batched = 1;                       // option "restart_batched": vima_decode_restart rebuilds the flagged samples' prompt K / V together (0: one sample at a time)
  std::vector<int> restart_list;                 // host copy of the flagged sample indices (source of the upload)
  std::vector<int> hist_rowmap;                  // host copy of the history's compact row -> cache row map (source of the upload)
  std::vector<int> fork_table;                   // host copy of a fork's job table (vima_decode_fork / vima_seq_decode_fork; source of the upload)
  std::vector<long long> snap_table;             // host copy of a snapshot / restore call's table (jobs, state jobs, row map; source of the upload)
  // hipGraph replay of the per-env-step entry points (option "graphs"): at small batch a step is ~1300 launches of
  // microsecond kernels and the HOST launch rate is the bound. The launch sequence of a call is captured the second time
  // the same (entry point, shapes, pointers, options, workspace generation) is seen and replayed afterwards.
  int graph_mode = 0;
  uint64_t state_gen = 0;       // bumped when options / cache allocations change what a captured graph bakes in
  hipStream_t gstream = nullptr;
  hipEvent_t ev_gin = nullptr, ev_gout = nullptr;
  struct GraphEntry { hipGraphExec_t exec; uint64_t last_use; };
  std::unordered_map<std::string, GraphEntry> graphs;
  std::unordered_map<std::string, int> graph_seen;   // eager runs so far; -1: capture failed, stay eager
  uint64_t graph_clock = 0;
  int64_t graph_replays = 0, graph_captures = 0;
  std::map<std::string, HostParam> host;       // staged until finalize
  std::vector<void*> owned;                     // device allocations of packed weights
  Arena arena;
  // ---- packed weights
  struct VitBlock { float *ln1g, *ln1b, *ln2g, *ln2b; Lin in_proj, out_proj, fc, proj; };
  struct {
    float *cls, *pos, *lnpre_g, *lnpre_b, *lnpost_g, *lnpost_b;
    Lin conv, projection;
    VitBlock blk[kVitLayers];
  } vit;
  struct { float *w0, *b0; Lin l1, l2; Lin pre; } view[2];
  Lin fuse; float* ee_table = nullptr;           // [2][E]
  Lin pobj[3];
  float* word_table = nullptr;                   // [32128,768] fp32
  struct T5Layer { float *rms1, *rms2; Lin qkv, o, wi, wo; Lin qkv_g, wi_g; };   // *_g: RMSNorm weight folded in (W diag(g))
  T5Layer t5[kT5Layers];
  float* t5_final = nullptr;
  std::vector<float> t5_relbias_host;            // [32][12]
  std::map<int, float*> t5_bias_tables;          // L -> device [12][2L-1]
  std::map<int, int> t5_bias_far;                // L -> distance from which that table is constant on both sides (AttnArgs::bias_far; 0: never)
  int op_bias_far = 0;                           // option "op_bias_far": AttnArgs::bias_far of vima_op_attention calls (tests)
  int ln_fuse = 1;                               // option "ln_fuse": the decoder's ln_2 and the next layer's XAttention pre-LN as ONE launch (layernorm2_kernel), and the pre-LN in front of
                                                 // XAttention's feed-forward folded into the GEMMs either side of it (GemmArgs::sum_out / rs_sum) where the GEGLU pair forms exist
  int geglu_pair = 1;                            // option "geglu_pair": GEGLU layers whose two products read the same input run as ONE launch over block-interleaved weights where gemm_pair_ok()
  int kv_headmajor = 1;                          // option "kv_headmajor": write the decoder's prompt K / V head-major where the projection GEMM allows it
  Lin t5_post; bool has_t5_post = false;
  float *pos_emb = nullptr, *xpos_emb = nullptr;
  struct DecLayer {
    float *xln_g, *xln_b, *xln2_g, *xln2_b; Lin q, kv, ao, l1, gate, l2;
    float *ln1_g, *ln1_b, *ln2_g, *ln2_b; Lin c_attn, c_proj, fc, mgate, mproj;
    Lin fc_pair;   // fc and mgate block-interleaved (GemmArgs::pair32); bf16 weights only
    // XAttention's feed-forward with its pre-LN folded in (option ln_fuse; bf16 weights only): l1 diag(ln.weight) with bias l1 . ln.bias and the
    // column sums `c`, alone (small grids: the dual-accumulator form beside `gate`) and block-interleaved with `gate` (pair32 form)
    Lin xl1g, xl1_pair;
  };
  std::vector<DecLayer> dec;
  Lin head1; void* head2_W = nullptr; float* head2_b = nullptr; Lin head3[kNumHeadsOut];
  // the 12 last layers (512 -> bins) packed for ONE grouped launch: W [700, 512] in logits order, bias [700], column starts [13]
  void* head3_Wall = nullptr; float* head3_ball = nullptr; int* head3_col = nullptr;
  struct { float *w0, *b0; } act0[4];
  void* act1_W = nullptr; float* act1_b = nullptr; Lin act_post;
  // ---- baseline policies (policy_kind != VIMA; baselines.inc): the ViT above holds the rectangular variant (vit_S tokens per
  // frame, 32x32 patches); decoder-only kinds use the Block half of `dec` + sep_token; FLAMINGO adds the Perceiver
  int vit_S = 5, vit_patches = 4;
  float* sep_token = nullptr;
  struct PercLayer { float *ln1g, *ln1b, *ln2g, *ln2b, *lng, *lnb; Lin q, kv, o, d1, d2; };   // kv = [key; value] stacked
  PercLayer perc_cross, perc_self[4];
  float* latents = nullptr;
  // ---- profiling
  bool prof = false;
  std::vector<ProfRec> recs;
  std::vector<hipEvent_t> ev_pool;
  size_t ev_used = 0;

  size_t esz() const { return bf16 ? 2 : 4; }
};

namespace {

// ------------------------------------------------------------------------------------------------ fp8 calibration (Fp8Cal)
// Begin a calibrating pass: the group's max |x| slots (allocated once) are zeroed on the stream; the pass then runs launch_amax into them.
int cal_begin(VimaHandle* h, Fp8Cal& c, hipStream_t st) {
  if (!c.amax) {
    HIPCK(hipMalloc((void**)&c.amax, c.sites * sizeof(float)));
    h->owned.push_back(c.amax);
  }
  HIPCK(hipMemsetAsync(c.amax, 0, c.sites * sizeof(float), st));
  return 0;
}
// Freeze: read the maxima back and turn them into scales (a dead site gets 1). A refused (non-finite) calibration leaves the group not ready and returns the error.
int cal_freeze(VimaHandle* h, Fp8Cal& c, hipStream_t st) {
  std::vector<float> am(c.sites);
  HIPCK(hipMemcpyAsync(am.data(), c.amax, am.size() * sizeof(float), hipMemcpyDeviceToHost, st));
  HIPCK(hipStreamSynchronize(st));
  if (int e = fp8_scales_from_amax(am, h->fp8_headroom_pct, c.group, c.scale)) return e;
  c.ready = true;
  ++h->state_gen;
  return 0;
}

// ------------------------------------------------------------------------------------------------ weight packing
uint16_t h_f2bf(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40u);
  u += 0x7fffu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}

struct Packer {
  VimaHandle* h;
  std::string missing;
  const HostParam* get(const std::string& name, std::initializer_list<int64_t> shape) {
    auto it = h->host.find(name);
    if (it == h->host.end()) {
      missing += "\n  missing key: " + name;
      return nullptr;
    }
    std::vector<int64_t> want(shape);
    if (it->second.shape != want) {
      std::string s = "\n  shape mismatch for " + name + ": got [";
      for (auto d : it->second.shape) s += std::to_string(d) + ",";
      s += "] want [";
      for (auto d : want) s += std::to_string(d) + ",";
      missing += s + "]";
      return nullptr;
    }
    return &it->second;
  }
  float* up_f32(const float* src, size_t n) {
    float* d = nullptr;
    if (hipMalloc((void**)&d, n * 4 + 16) != hipSuccess) { missing += "\n  hipMalloc failed"; return nullptr; }
    h->owned.push_back(d);
    if (hipMemcpy(d, src, n * 4, hipMemcpyHostToDevice) != hipSuccess) missing += "\n  hipMemcpy failed";
    return d;
  }
  void* up_T(const std::vector<float>& src) {
    if (!h->bf16) return up_f32(src.data(), src.size());
    std::vector<uint16_t> t(src.size());
    for (size_t i = 0; i < src.size(); ++i) t[i] = h_f2bf(src[i]);
    void* d = nullptr;
    if (hipMalloc(&d, t.size() * 2 + 16) != hipSuccess) { missing += "\n  hipMalloc failed"; return nullptr; }
    h->owned.push_back(d);
    if (hipMemcpy(d, t.data(), t.size() * 2, hipMemcpyHostToDevice) != hipSuccess) missing += "\n  hipMemcpy failed";
    return d;
  }
  // weight of a Linear layer [l.N, l.K] row-major: operand type, or fp8 e4m3 + per-output-channel scale (amax / 448)
  void pack_w(Lin& l, const std::vector<float>& w) {
    if (!h->w8 || !fp8_eligible(l.N, l.K)) { l.W = up_T(w); return; }
    std::vector<uint8_t> q((size_t)l.N * l.K);
    std::vector<float> sc((size_t)l.N);
    for (int n = 0; n < l.N; ++n) {
      const float* row = &w[(size_t)n * l.K];
      float amax = 0.f;
      for (int k = 0; k < l.K; ++k) amax = fmaxf(amax, fabsf(row[k]));
      const float scale = amax > 0.f ? amax / 448.0f : 1.0f;
      sc[n] = scale;
      for (int k = 0; k < l.K; ++k) q[(size_t)n * l.K + k] = f32_to_e4m3(row[k] / scale);
    }
    void* d = nullptr;
    if (hipMalloc(&d, q.size() + 64) != hipSuccess) { missing += "\n  hipMalloc failed"; return; }
    h->owned.push_back(d);
    if (hipMemcpy(d, q.data(), q.size(), hipMemcpyHostToDevice) != hipSuccess) missing += "\n  hipMemcpy failed";
    l.W = d;
    l.ws = up_f32(sc.data(), sc.size());
  }
  float* vec(const std::string& name, int64_t n) {
    const HostParam* p = get(name, {n});
    return p ? up_f32(p->data.data(), (size_t)n) : nullptr;
  }
  // nn.Linear weight [N,K] (+ bias)
  Lin linear(const std::string& prefix, int N, int K, bool bias, const char* wname = ".weight") {
    Lin l;
    l.N = N; l.K = K;
    const HostParam* w = get(prefix + wname, {N, K});
    if (w) pack_w(l, w->data);
    if (bias) l.b = vec(prefix + ".bias", N);
    return l;
  }
  // GEGLU pair (GemmArgs::pair32): the GELU'd Conv1D layer [K, N] (+ bias) and its bias-less nn.Linear multiplier [N, K] as ONE [2N, K] weight,
  // alternating in blocks of 32 output rows (block 2j: GELU'd rows 32j.., block 2j + 1: multiplier rows 32j..); the multiplier's bias entries are 0
  Lin pair32(const std::string& conv_prefix, const std::string& lin_prefix, int N, int K) {
    Lin l;
    l.N = 2 * N; l.K = K;
    const HostParam* w1 = get(conv_prefix + ".weight", {K, N});
    const HostParam* b1 = get(conv_prefix + ".bias", {N});
    const HostParam* wg = get(lin_prefix + ".weight", {N, K});
    if (!w1 || !b1 || !wg) return l;
    std::vector<float> t((size_t)2 * N * K), bb((size_t)2 * N, 0.0f);
    for (int n = 0; n < N; ++n) {
      const size_t r1 = (size_t)(n / 32) * 64 + (n % 32), rg = r1 + 32;
      for (int k = 0; k < K; ++k) {
        t[r1 * K + k] = w1->data[(size_t)k * N + n];
        t[rg * K + k] = wg->data[(size_t)n * K + k];
      }
      bb[r1] = b1->data[n];
    }
    l.W = up_T(t);
    l.b = up_f32(bb.data(), bb.size());
    return l;
  }
  // nn.Linear [N, K] (no bias) behind a LayerNorm (gamma, beta over K) with the norm folded in: W' = W diag(gamma) in the operand type,
  // bias'[n] = sum_k beta[k] W[n][k], c[n] = sum_k bf16(W'[n][k]) (the mean term must cancel against what the matrix core actually multiplies).
  // `gate_prefix` non-empty: block-interleaved in 32-row blocks with that bias-less nn.Linear [N, K] as the plain multiplier (GemmArgs::pair32):
  // [2N, K], the multiplier's rows carry bias 0 and c 0
  Lin ln_folded(const std::string& lin_prefix, const std::string& ln_prefix, const std::string& gate_prefix, int N, int K) {
    Lin l;
    const bool pair = !gate_prefix.empty();
    l.N = pair ? 2 * N : N; l.K = K;
    const HostParam* w = get(lin_prefix + ".weight", {N, K});
    const HostParam* g = get(ln_prefix + ".weight", {K});
    const HostParam* b = get(ln_prefix + ".bias", {K});
    const HostParam* wg = pair ? get(gate_prefix + ".weight", {N, K}) : nullptr;
    if (!w || !g || !b || (pair && !wg)) return l;
    std::vector<float> t((size_t)l.N * K), bb((size_t)l.N, 0.0f), cc((size_t)l.N, 0.0f);
    for (int n = 0; n < N; ++n) {
      const size_t r1 = pair ? (size_t)(n / 32) * 64 + (n % 32) : (size_t)n;
      double sb = 0.0, sc = 0.0;
      for (int k = 0; k < K; ++k) {
        const float wf = w->data[(size_t)n * K + k] * g->data[k];
        t[r1 * K + k] = wf;
        uint32_t u = (uint32_t)h_f2bf(wf) << 16;
        float wr;
        memcpy(&wr, &u, 4);
        sc += (double)wr;
        sb += (double)b->data[k] * (double)w->data[(size_t)n * K + k];
        if (pair) t[(r1 + 32) * K + k] = wg->data[(size_t)n * K + k];
      }
      bb[r1] = (float)sb;
      cc[r1] = (float)sc;
    }
    l.W = up_T(t);
    l.b = up_f32(bb.data(), bb.size());
    l.c = up_f32(cc.data(), cc.size());
    return l;
  }
  // HF Conv1D weight [K(in), N(out)] -> packed [N,K]
  Lin conv1d(const std::string& prefix, int N, int K) {
    Lin l;
    l.N = N; l.K = K;
    const HostParam* w = get(prefix + ".weight", {K, N});
    if (w) {
      std::vector<float> t((size_t)N * K);
      for (int k = 0; k < K; ++k)
        for (int n = 0; n < N; ++n) t[(size_t)n * K + k] = w->data[(size_t)k * N + n];
      pack_w(l, t);
    }
    l.b = vec(prefix + ".bias", N);
    return l;
  }
};

int pack_all(VimaHandle* h) {
  Packer P{h, ""};
  const int E = h->cfg.embed_dim, NL = h->cfg.xf_n_layers;
  const int kind = h->cfg.policy_kind;
  const bool is_vima = kind == VIMA_POLICY_VIMA;
  const bool has_xattn = is_vima || kind == VIMA_POLICY_FLAMINGO;
  // baselines: (Gato)VisionTransformerRectangular on 64x128 frames with 32x32 patches (vit.py:83-135, 262-329): 8 patch
  // tokens, + cls for VIMAGPTPolicy; projection [768, E]
  const bool vit_cls = is_vima || kind == VIMA_POLICY_GPT;
  const int patch = is_vima ? 16 : 32;
  h->vit_patches = is_vima ? 4 : 8;
  h->vit_S = h->vit_patches + (vit_cls ? 1 : 0);
  const int vit_out = is_vima ? kVitW : E;
  const int obj_dim = kind == VIMA_POLICY_GPT ? 2 * E : E;   // obj_encoder.output_dim (obj_encoder.py:243-245)
  char buf[256];
  // ---- ViT (vit.py:137-169)
  const std::string v = "obj_encoder.cropped_img_encoder.vit.";
  if (vit_cls) h->vit.cls = P.vec(v + "cls_token", kVitW);
  if (const HostParam* p = P.get(v + "pos_embed", {h->vit_S, kVitW})) h->vit.pos = P.up_f32(p->data.data(), p->data.size());
  h->vit.lnpre_g = P.vec(v + "ln_pre.weight", kVitW);
  h->vit.lnpre_b = P.vec(v + "ln_pre.bias", kVitW);
  h->vit.lnpost_g = P.vec(v + "ln_post.weight", kVitW);
  h->vit.lnpost_b = P.vec(v + "ln_post.bias", kVitW);
  if (const HostParam* p = P.get(v + "conv1.weight", {kVitW, 3, patch, patch})) {  // [768, 3*P*P] already [N,K]
    h->vit.conv.N = kVitW; h->vit.conv.K = 3 * patch * patch;
    P.pack_w(h->vit.conv, p->data);
  }
  if (const HostParam* p = P.get(v + "projection", {kVitW, vit_out})) {        // x @ projection: [in,out] -> [out,in]
    std::vector<float> t((size_t)kVitW * vit_out);
    for (int k = 0; k < kVitW; ++k)
      for (int n = 0; n < vit_out; ++n) t[(size_t)n * kVitW + k] = p->data[(size_t)k * vit_out + n];
    h->vit.projection.N = vit_out; h->vit.projection.K = kVitW;
    P.pack_w(h->vit.projection, t);
  }
  for (int j = 0; j < kVitLayers; ++j) {
    snprintf(buf, sizeof buf, "%sblocks.%d.", v.c_str(), j);
    const std::string b = buf;
    auto& B = h->vit.blk[j];
    B.ln1g = P.vec(b + "ln_1.weight", kVitW); B.ln1b = P.vec(b + "ln_1.bias", kVitW);
    B.ln2g = P.vec(b + "ln_2.weight", kVitW); B.ln2b = P.vec(b + "ln_2.bias", kVitW);
    B.in_proj.N = 3 * kVitW; B.in_proj.K = kVitW;
    if (const HostParam* p = P.get(b + "attn.in_proj_weight", {3 * kVitW, kVitW})) P.pack_w(B.in_proj, p->data);
    B.in_proj.b = P.vec(b + "attn.in_proj_bias", 3 * kVitW);
    B.out_proj = P.linear(b + "attn.out_proj", kVitW, kVitW, true);
    B.fc = P.linear(b + "mlp.c_fc", 4 * kVitW, kVitW, true);
    B.proj = P.linear(b + "mlp.c_proj", kVitW, 4 * kVitW, true);
  }
  // ---- bbox MLPs + per-view projection (obj_encoder.py:44-64)
  for (int vi = 0; vi < 2 && is_vima; ++vi) {
    const std::string bp = std::string("obj_encoder.bbox_mlp.") + kViews[vi];
    if (const HostParam* p = P.get(bp + ".0.weight", {768, 4})) h->view[vi].w0 = P.up_f32(p->data.data(), p->data.size());
    h->view[vi].b0 = P.vec(bp + ".0.bias", 768);
    h->view[vi].l1 = P.linear(bp + ".3", 768, 768, true);
    h->view[vi].l2 = P.linear(bp + ".6", 768, 768, true);
    h->view[vi].pre = P.linear(std::string("obj_encoder.pre_transformer_layer.") + kViews[vi], E, 2 * kVitW, true);
  }
  // ---- obs fusion (vima_policy.py:47-49,253-256): Linear(E+2 -> E) on cat(img, ee_emb[ee]) = W[:, :E] img + table[ee]
  {
    const int Kf = obj_dim;   // width of the image feature in front of the 2 end-effector columns
    const HostParam* w = P.get("obs_fusion_layer.weight", {E, Kf + 2});
    const HostParam* b = P.get("obs_fusion_layer.bias", {E});
    const HostParam* ee = P.get("end_effector_encoder.weight", {2, 2});
    if (w && b && ee) {
      std::vector<float> wm((size_t)E * Kf), tab((size_t)2 * E);
      for (int n = 0; n < E; ++n) {
        for (int k = 0; k < Kf; ++k) wm[(size_t)n * Kf + k] = w->data[(size_t)n * (Kf + 2) + k];
        for (int e = 0; e < 2; ++e) {
          float t = ee->data[e * 2 + 0] * w->data[(size_t)n * (Kf + 2) + Kf];
          t = fmaf(ee->data[e * 2 + 1], w->data[(size_t)n * (Kf + 2) + Kf + 1], t);
          tab[(size_t)e * E + n] = t + b->data[n];
        }
      }
      h->fuse.N = E; h->fuse.K = Kf;
      P.pack_w(h->fuse, wm);
      h->ee_table = P.up_f32(tab.data(), tab.size());
    }
  }
  // ---- prompt object post MLP (vima_policy.py:103-108)
  h->pobj[0] = P.linear("prompt_obj_post_layer.0", 768, obj_dim, true);
  h->pobj[1] = P.linear("prompt_obj_post_layer.3", 768, 768, true);
  h->pobj[2] = P.linear("prompt_obj_post_layer.6", 768, 768, true);
  // ---- word embedding table (word_embd.py:8-23)
  if (const HostParam* p = P.get("prompt_embedding._embed_layer.weight", {kVocab, 768}))
    h->word_table = P.up_f32(p->data.data(), p->data.size());
  // ---- T5 encoder (prompt_encoder.py; HF T5Attention/T5LayerFF)
  const std::string t5 = "t5_prompt_encoder.t5.encoder.";
  for (int l = 0; l < kT5Layers; ++l) {
    snprintf(buf, sizeof buf, "%sblock.%d.layer.0.", t5.c_str(), l);
    const std::string a = buf;
    snprintf(buf, sizeof buf, "%sblock.%d.layer.1.", t5.c_str(), l);
    const std::string f = buf;
    auto& L = h->t5[l];
    L.rms1 = P.vec(a + "layer_norm.weight", kT5Model);
    L.rms2 = P.vec(f + "layer_norm.weight", kT5Model);
    const int inner = kT5Heads * kT5D;
    const HostParam* q = P.get(a + "SelfAttention.q.weight", {inner, kT5Model});
    const HostParam* k = P.get(a + "SelfAttention.k.weight", {inner, kT5Model});
    const HostParam* vv = P.get(a + "SelfAttention.v.weight", {inner, kT5Model});
    if (q && k && vv) {   // fused [q;k;v] -> one GEMM
      std::vector<float> t;
      t.reserve((size_t)3 * inner * kT5Model);
      t.insert(t.end(), q->data.begin(), q->data.end());
      t.insert(t.end(), k->data.begin(), k->data.end());
      t.insert(t.end(), vv->data.begin(), vv->data.end());
      L.qkv.N = 3 * inner; L.qkv.K = kT5Model;
      P.pack_w(L.qkv, t);
      // (x_hat * g) W^T = x_hat (W diag(g))^T : the RMSNorm weight folded into the consumer (fused-RMSNorm path)
      if (const HostParam* g = P.get(a + "layer_norm.weight", {kT5Model})) {
        for (size_t n = 0; n < (size_t)3 * inner; ++n)
          for (int k = 0; k < kT5Model; ++k) t[n * kT5Model + k] *= g->data[k];
        L.qkv_g.N = 3 * inner; L.qkv_g.K = kT5Model;
        P.pack_w(L.qkv_g, t);
      }
    }
    L.o = P.linear(a + "SelfAttention.o", kT5Model, inner, false);
    L.wi = P.linear(f + "DenseReluDense.wi", kT5FF, kT5Model, false);
    {
      const HostParam* w = P.get(f + "DenseReluDense.wi.weight", {kT5FF, kT5Model});
      const HostParam* g = P.get(f + "layer_norm.weight", {kT5Model});
      if (w && g) {
        std::vector<float> t(w->data);
        for (size_t n = 0; n < (size_t)kT5FF; ++n)
          for (int k = 0; k < kT5Model; ++k) t[n * kT5Model + k] *= g->data[k];
        L.wi_g.N = kT5FF; L.wi_g.K = kT5Model;
        P.pack_w(L.wi_g, t);
      }
    }
    L.wo = P.linear(f + "DenseReluDense.wo", kT5Model, kT5FF, false);
  }
  if (const HostParam* p = P.get(t5 + "block.0.layer.0.SelfAttention.relative_attention_bias.weight", {kT5Buckets, kT5Heads}))
    h->t5_relbias_host = p->data;
  h->t5_final = P.vec(t5 + "final_layer_norm.weight", kT5Model);
  h->has_t5_post = (E != kT5Model);
  if (h->has_t5_post) h->t5_post = P.linear("t5_prompt_encoder_post_layer", E, kT5Model, false);
  // ---- XAttnGPT (xattn_gpt.py:45-68, components.py); decoder-only baselines: HFGPT (gpt/gpt.py:83-100), whose Block is
  // a second copy of the same class (gpt/gpt.py:223-301) under "transformer.lm."
  const std::string gp = has_xattn ? "xattn_gpt." : "transformer.lm.";
  if (const HostParam* p = P.get(gp + "positions_embed.weight", {h->cfg.n_positions, E}))
    h->pos_emb = P.up_f32(p->data.data(), p->data.size());
  if (has_xattn)
    if (const HostParam* p = P.get("xattn_gpt.xattn_positions_embed.weight", {h->cfg.xattn_n_positions, E}))
      h->xpos_emb = P.up_f32(p->data.data(), p->data.size());
  if (!has_xattn) h->sep_token = P.vec("prompt_sep_token", E);
  h->dec.resize(NL);
  for (int i = 0; i < NL; ++i) {
    auto& D = h->dec[i];
    snprintf(buf, sizeof buf, "xattn_gpt.xattns.%d.", i);
    const std::string x = buf;
    if (has_xattn) {
    D.xln_g = P.vec(x + "layernorm.weight", E); D.xln_b = P.vec(x + "layernorm.bias", E);
    D.xln2_g = P.vec(x + "ln.weight", E); D.xln2_b = P.vec(x + "ln.bias", E);
    D.q = P.linear(x + "query", E, E, false);
    D.kv = P.linear(x + "key_value", 2 * E, E, false);
    D.ao = P.linear(x + "attention_out", E, E, false);
    D.l1 = P.linear(x + "linear1", 4 * E, E, false);
    D.gate = P.linear(x + "gated_layer", 4 * E, E, false);
    D.l2 = P.linear(x + "linear2", E, 4 * E, false);
    if (h->bf16 && !h->w8 && (4 * E) % 64 == 0) {
      D.xl1g = P.ln_folded(x + "linear1", x + "ln", "", 4 * E, E);
      D.xl1_pair = P.ln_folded(x + "linear1", x + "ln", x + "gated_layer", 4 * E, E);
    }
    }
    snprintf(buf, sizeof buf, "%sh.%d.", gp.c_str(), i);
    const std::string b = buf;
    D.ln1_g = P.vec(b + "ln_1.weight", E); D.ln1_b = P.vec(b + "ln_1.bias", E);
    D.ln2_g = P.vec(b + "ln_2.weight", E); D.ln2_b = P.vec(b + "ln_2.bias", E);
    D.c_attn = P.conv1d(b + "attn.c_attn", 3 * E, E);
    D.c_proj = P.conv1d(b + "attn.c_proj", E, E);
    D.fc = P.conv1d(b + "mlp.c_fc", 4 * E, E);
    D.mproj = P.conv1d(b + "mlp.c_proj", E, 4 * E);
    D.mgate = P.linear(b + "mlp.gated_layer", 4 * E, E, false);
    if (h->bf16 && !h->w8 && (4 * E) % 64 == 0) D.fc_pair = P.pair32(b + "mlp.c_fc", b + "mlp.gated_layer", 4 * E, E);
  }
  // ---- action decoder: 12 MLPs E->512->512->bins (action_decoder.py:128-166), layer 1 stacked, layer 2 batched
  {
    std::vector<float> w1((size_t)kNumHeadsOut * kHeadHidden * E), b1((size_t)kNumHeadsOut * kHeadHidden);
    std::vector<float> w2((size_t)kNumHeadsOut * kHeadHidden * kHeadHidden), b2((size_t)kNumHeadsOut * kHeadHidden);
    std::vector<float> w3((size_t)kLogits * kHeadHidden), b3((size_t)kLogits);
    int col3[kNumHeadsOut + 1];
    col3[0] = 0;
    for (int j = 0; j < kNumHeadsOut; ++j) col3[j + 1] = col3[j] + kHeadBins[j];
    int hidx = 0;
    bool ok = true;
    for (int k = 0; k < 4; ++k) {
      const int nsub = kActDims[k];
      for (int j = 0; j < nsub; ++j, ++hidx) {
        snprintf(buf, sizeof buf, "action_decoder._decoders.%s.mlps.%d", kActKeys[k], j);
        const std::string m = buf;
        const HostParam* a = P.get(m + ".0.weight", {kHeadHidden, E});
        const HostParam* ab = P.get(m + ".0.bias", {kHeadHidden});
        const HostParam* c = P.get(m + ".3.weight", {kHeadHidden, kHeadHidden});
        const HostParam* cb = P.get(m + ".3.bias", {kHeadHidden});
        if (a && ab && c && cb) {
          memcpy(&w1[(size_t)hidx * kHeadHidden * E], a->data.data(), a->data.size() * 4);
          memcpy(&b1[(size_t)hidx * kHeadHidden], ab->data.data(), ab->data.size() * 4);
          memcpy(&w2[(size_t)hidx * kHeadHidden * kHeadHidden], c->data.data(), c->data.size() * 4);
          memcpy(&b2[(size_t)hidx * kHeadHidden], cb->data.data(), cb->data.size() * 4);
        } else {
          ok = false;
        }
        h->head3[hidx] = P.linear(m + ".6", kHeadBins[hidx], kHeadHidden, true);
        const HostParam* e3 = P.get(m + ".6.weight", {kHeadBins[hidx], kHeadHidden});
        const HostParam* eb3 = P.get(m + ".6.bias", {kHeadBins[hidx]});
        if (e3 && eb3) {
          memcpy(&w3[(size_t)col3[hidx] * kHeadHidden], e3->data.data(), e3->data.size() * 4);
          memcpy(&b3[(size_t)col3[hidx]], eb3->data.data(), eb3->data.size() * 4);
        } else {
          ok = false;
        }
      }
    }
    if (ok) {
      h->head1.N = kNumHeadsOut * kHeadHidden; h->head1.K = E;
      P.pack_w(h->head1, w1); h->head1.b = P.up_f32(b1.data(), b1.size());
      h->head2_W = P.up_T(w2); h->head2_b = P.up_f32(b2.data(), b2.size());
      if (h->bf16) {   // grouped launch of the last layers (bf16 operands; these matrices are below the fp8 size threshold)
        h->head3_Wall = P.up_T(w3); h->head3_ball = P.up_f32(b3.data(), b3.size());
        h->head3_col = reinterpret_cast<int*>(P.up_f32(reinterpret_cast<const float*>(col3), kNumHeadsOut + 1));
      }
    }
  }
  // ---- action encoder (action_embd.py): sorted key order == kActKeys order
  {
    std::vector<float> w((size_t)4 * 256 * 256), b((size_t)4 * 256);
    bool ok = true;
    for (int k = 0; k < 4; ++k) {
      snprintf(buf, sizeof buf, "action_encoder._embed_dict.%s._layer", kActKeys[k]);
      const std::string m = buf;
      const int K = kActDims[k];
      if (const HostParam* p = P.get(m + ".0.weight", {256, K})) h->act0[k].w0 = P.up_f32(p->data.data(), p->data.size());
      h->act0[k].b0 = P.vec(m + ".0.bias", 256);
      const HostParam* c = P.get(m + ".3.weight", {256, 256});
      const HostParam* cb = P.get(m + ".3.bias", {256});
      if (c && cb) {
        memcpy(&w[(size_t)k * 256 * 256], c->data.data(), c->data.size() * 4);
        memcpy(&b[(size_t)k * 256], cb->data.data(), cb->data.size() * 4);
      } else {
        ok = false;
      }
    }
    if (ok) { h->act1_W = P.up_T(w); h->act1_b = P.up_f32(b.data(), b.size()); }
    // ActionEmbedding._post_layer is nn.Identity when embed_dim == 4 * 256 (action_embd.py:24-27): no such key then
    if (E != 1024) h->act_post = P.linear("action_encoder._post_layer", E, 1024, true);
  }
  if (kind == VIMA_POLICY_FLAMINGO) {
    // HF PerceiverModel (modeling_perceiver.py:125-527; obj_encoder.py:176-204 `peceiver` sic): 4 latents, one cross-attention
    // layer, 4 self-attention layers applied 4 times, widening factor 1
    const std::string pc = "obj_encoder.peceiver.model.";
    if (const HostParam* p = P.get(pc + "embeddings.latents", {4, E})) h->latents = P.up_f32(p->data.data(), p->data.size());
    auto layer = [&](VimaHandle::PercLayer& L, const std::string& pre, bool cross) {
      const std::string a = pre + "attention.";
      L.ln1g = P.vec(a + "self.layernorm1.weight", E); L.ln1b = P.vec(a + "self.layernorm1.bias", E);
      if (cross) { L.ln2g = P.vec(a + "self.layernorm2.weight", E); L.ln2b = P.vec(a + "self.layernorm2.bias", E); }
      L.q = P.linear(a + "self.query", E, E, true);
      const HostParam* kw = P.get(a + "self.key.weight", {E, E});
      const HostParam* kb = P.get(a + "self.key.bias", {E});
      const HostParam* vw = P.get(a + "self.value.weight", {E, E});
      const HostParam* vb = P.get(a + "self.value.bias", {E});
      if (kw && kb && vw && vb) {
        std::vector<float> w(kw->data), b(kb->data);
        w.insert(w.end(), vw->data.begin(), vw->data.end());
        b.insert(b.end(), vb->data.begin(), vb->data.end());
        L.kv.N = 2 * E; L.kv.K = E;
        P.pack_w(L.kv, w);
        L.kv.b = P.up_f32(b.data(), b.size());
      }
      L.o = P.linear(a + "output.dense", E, E, true);
      L.lng = P.vec(pre + "layernorm.weight", E); L.lnb = P.vec(pre + "layernorm.bias", E);
      L.d1 = P.linear(pre + "mlp.dense1", E, E, true);
      L.d2 = P.linear(pre + "mlp.dense2", E, E, true);
    };
    layer(h->perc_cross, pc + "encoder.cross_attention.", true);
    for (int i = 0; i < 4; ++i) {
      snprintf(buf, sizeof buf, "%sencoder.self_attends.%d.", pc.c_str(), i);
      layer(h->perc_self[i], buf, false);
    }
  }
  if (!P.missing.empty()) return fail("vima_finalize_params (strict):" + P.missing);
  return 0;
}

// ------------------------------------------------------------------------------------------------ launch helpers
// A GEMM input or output of the encoder stacks (T5, ViT, prompt K/V projection), described once: the operand-type buffer and its leading dimension, where the
// stage runs fp8 activations its e4m3 copy with the site's dequantisation scale (s8 > 0), and for a residual stream kept in fp32 that buffer (same ld).
struct Opnd { void* p = nullptr; int ld = 0; void* p8 = nullptr; float s8 = 0.f; float* p32 = nullptr; };

struct Run {
  VimaHandle* h;
  hipStream_t st;
  int err = 0;
  void prof_begin(int cls, double flops, double bytes = 0.0) {
    if (!h->prof) return;
    if (h->ev_used + 2 > h->ev_pool.size()) {
      for (int i = 0; i < 256; ++i) {
        hipEvent_t e;
        (void)hipEventCreate(&e);
        h->ev_pool.push_back(e);
      }
    }
    ProfRec r{cls, h->ev_pool[h->ev_used], h->ev_pool[h->ev_used + 1], flops, bytes};
    h->ev_used += 2;
    (void)hipEventRecord(r.a, st);
    h->recs.push_back(r);
  }
  void prof_end() {
    if (!h->prof) return;
    (void)hipEventRecord(h->recs.back().b, st);
  }
  template <typename P> P* ws(size_t n) {   // workspace elements of type P
    void* p = h->arena.alloc(n * sizeof(P));
    if (!p && !err) err = fail("workspace allocation failed");
    return reinterpret_cast<P*>(p);
  }
  void* wsT(size_t n) {
    void* p = h->arena.alloc(n * h->esz());
    if (!p && !err) err = fail("workspace allocation failed");
    return p;
  }
  // A handle-owned host vector -> the workspace carved for it, on the stream (the vector is the source of an asynchronous copy: it must outlive the
  // call). Issued where the open-coded copies were: behind the call's workspace carving and its R.err check
  template <typename P> int upload(P* dst, const std::vector<P>& v) {
    if (err) return err;
    const hipError_t e = hipMemcpyAsync(dst, v.data(), v.size() * sizeof(P), hipMemcpyHostToDevice, st);
    if (e != hipSuccess) err = fail(std::string("hipMemcpyAsync (upload): ") + hipGetErrorString(e), (int)e);
    return err;
  }
  void* offT(void* p, long long elems) const { return reinterpret_cast<char*>(p) + elems * (long long)h->esz(); }
  const void* offT(const void* p, long long elems) const { return reinterpret_cast<const char*>(p) + elems * (long long)h->esz(); }

  int gemm(GemmArgs a) {
    if (err) return err;
    a.tune = &h->tune;
    if (const size_t wsb = gemm_splitk_bytes(a, h->bf16)) {   // underfilled grid: scratch for the two-pass split-K
      a.splitk_ws = ws<float>(wsb / sizeof(float));
      a.splitk_ws_bytes = wsb;
      if (err) return err;
    }
    {   // class 3 = GEMMs whose epilogue adds an fp32 residual and writes the fp32 stream (the HBM-heavy ones); algorithmic
        // bytes = each operand / output / epilogue input once
      const double nb = a.batch > 0 ? a.batch : 1, es = (double)h->esz(), mn = (double)a.M * a.N;
      const double bytes = nb * ((double)a.M * a.K * es + (double)a.N * a.K * (a.w8 ? 1.0 : es) + (a.out32 ? mn * 4 : 0) + (a.outT ? (a.pair32 ? mn / 2 : mn) * es : 0) +
                                 (a.res ? mn * 4 : 0) + (a.resT ? mn * es : 0) + (a.mul ? mn * es : 0) + (a.ssq_out ? (double)a.M * (a.N / 32) * 4 : 0));
      const double two = a.W2 ? 2.0 : 1.0;   // GEGLU pair: two products in one launch
      prof_begin(((a.res && a.out32) || a.resT) ? 3 : 0, two * 2.0 * a.M * (double)a.N * a.K * nb,
                 bytes + (a.W2 ? nb * ((double)a.M * a.K * es + (double)a.N * a.K * es) : 0.0));
    }
    int kid = 0;
    a.kernel_id = &kid;
    a.x3 = h->x3 ? 1 : 0;
    int e = launch_gemm(a, h->bf16, st);
    prof_end();
    if (h->prof && !h->recs.empty()) { ProfRec& r = h->recs.back(); r.kid = kid; r.M = a.M; r.N = a.N; r.K = a.K; }
    if (e) err = fail(std::string("gemm launch failed: ") + hipGetErrorString((hipError_t)e) + " (M=" + std::to_string(a.M) +
                      " N=" + std::to_string(a.N) + " K=" + std::to_string(a.K) + ")", e);
    return err;
  }
  // weight operand of a GEMM from a packed Linear layer, optionally starting at output channel row0
  void setW(GemmArgs& a, const Lin& L, int row0 = 0) const {
    a.ldw = L.K;
    if (L.ws) {
      a.W = reinterpret_cast<const char*>(L.W) + (long long)row0 * L.K;
      a.w8 = 1;
      a.wscale = L.ws + row0;
    } else {
      a.W = offT(L.W, (long long)row0 * L.K);
    }
  }
  // out = act(A . W^T + b) [* mul] [+ res]
  int linear(const void* A, int lda, const Lin& L, int M, int act, const void* mul, int ldmul, const float* res, int ldres,
             float* out32, int ld32, void* outT, int ldT) {
    GemmArgs a;
    a.A = A; a.lda = lda; setW(a, L); a.M = M; a.N = L.N; a.K = L.K;
    a.bias = L.b; a.act = act; a.mul = mul; a.ldmul = ldmul; a.res = res; a.ldres = ldres;
    a.out32 = out32; a.ld32 = ld32; a.outT = outT; a.ldT = ldT;
    return gemm(a);
  }
  // The same over operands (the encoder stacks): out = act(rs . in . L[row0 .. row0 + N)^T + b) [+ res], M rows. fp8 travels with the operand: an input with a
  // scale is read from its e4m3 copy, an output with a scale also gets (or, without p, only gets) one. res: the residual stream, fp32 if it has p32, else operand
  // type. rs / rs_parts: row sums of squares of the T5 RMSNorm folded into L (GemmArgs::rs_ssq); ssq_out: the same statistics of the output, for the next norm.
  GemmArgs linear_args(const Opnd& in, const Lin& L, int row0, int N, int M, int act, const Opnd* res, const Opnd& out, const float* rs = nullptr,
                    int rs_parts = 0, float* ssq_out = nullptr) const {
    GemmArgs a;
    if (in.s8 > 0.f) { a.A = in.p8; a.a8 = 1; a.ascale = in.s8; }
    else a.A = in.p;
    a.lda = in.ld; setW(a, L, row0); a.M = M; a.N = N; a.K = L.K; a.bias = L.b ? L.b + row0 : nullptr; a.act = act;
    if (res && res->p32) { a.res = res->p32; a.ldres = res->ld; }
    else if (res) { a.resT = res->p; a.ldresT = res->ld; }
    a.out32 = out.p32; a.ld32 = out.ld; a.outT = out.p; a.ldT = out.ld;
    if (out.s8 > 0.f) { a.out8 = out.p8; a.ld8 = out.ld; a.out8_inv = 1.0f / out.s8; }
    a.rs_ssq = rs; a.rs_parts = rs_parts; a.rs_invk = 1.0f / (float)L.K; a.rs_eps = 1e-6f;
    a.ssq_out = ssq_out;
    return a;
  }
  int linear(const Opnd& in, const Lin& L, int row0, int N, int M, int act, const Opnd* res, const Opnd& out, const float* rs = nullptr, int rs_parts = 0,
             float* ssq_out = nullptr) {
    return gemm(linear_args(in, L, row0, N, M, act, res, out, rs, rs_parts, ssq_out));
  }
  // u = GELU(A1 . L1^T + b1) * bf16(A2 . Lg^T): the value / gate pair of a GEGLU (components.py:31-33, 221-226). ONE dual-accumulator
  // launch where the library has one for this shape (bf16 weights, underfilled grid: batch <= ~32), else the gate GEMM into `g` followed
  // by the value GEMM with the gate as its epilogue multiplier -- bit-identical either way
  int geglu(const void* A1, const Lin& L1, const void* A2, const Lin& Lg, int M, void* g, void* u, const Lin* pair = nullptr) {
    if (pair && pair->W && A1 == A2 && h->geglu_pair && h->bf16 && pair->N == 2 * L1.N && gemm_pair_ok(&h->tune, M, L1.N, L1.K)) {
      GemmArgs a;   // one launch over the block-interleaved weights (the grid is neither small enough for the dual form nor large enough for the 256x256 kernels)
      a.A = A1; a.lda = L1.K; setW(a, *pair); a.M = M; a.N = pair->N; a.K = L1.K; a.bias = pair->b; a.act = ACT_GELU; a.outT = u; a.ldT = L1.N;
      a.pair32 = 1;
      return gemm(a);
    }
    if (h->bf16 && !L1.ws && !Lg.ws && L1.N == Lg.N && L1.K == Lg.K && gemm_dual_ok(&h->tune, M, L1.N)) {
      GemmArgs a;
      a.A = A1; a.lda = L1.K; setW(a, L1); a.A2 = A2; a.lda2 = Lg.K; a.W2 = Lg.W; a.ldw2 = Lg.K;
      a.M = M; a.N = L1.N; a.K = L1.K; a.bias = L1.b; a.act = ACT_GELU; a.outT = u; a.ldT = L1.N;
      return gemm(a);
    }
    linear(A2, Lg.K, Lg, M, ACT_NONE, nullptr, 0, nullptr, 0, nullptr, 0, g, Lg.N);
    return linear(A1, L1.K, L1, M, ACT_GELU, g, Lg.N, nullptr, 0, nullptr, 0, u, L1.N);
  }
  int ln(const float* in, long long ldin, const float* g, const float* b, float eps, int rms, int rows, int E, float* out32,
         void* outT) {
    if (err) return err;
    prof_begin(2, 0);
    int e = launch_layernorm(in, ldin, g, b, eps, rms, rows, E, out32, outT, h->bf16, st);
    prof_end();
    if (e) err = fail(std::string("layernorm launch failed: ") + hipGetErrorString((hipError_t)e), e);
    return err;
  }
  int lnT(const void* inT, long long ldin, const float* g, const float* b, float eps, int rms, int rows, int E, float* out32,
          void* outT, void* out8 = nullptr, float inv8 = 1.0f) {
    if (err) return err;
    prof_begin(2, 0);
    int e = launch_layernorm_T(inT, ldin, g, b, eps, rms, rows, E, out32, outT, h->bf16, st, out8, inv8);
    prof_end();
    if (e) err = fail(std::string("layernorm launch failed: ") + hipGetErrorString((hipError_t)e), e);
    return err;
  }
  int other(int e, const char* what) {
    if (err) return err;
    if (e) err = fail(std::string(what) + " launch failed: " + hipGetErrorString((hipError_t)e), e);
    return err;
  }
  int attn(AttnArgs a, int impl) {
    if (err) return err;
    a.tune = &h->tune;
    prof_begin(1, 4.0 * a.B * (double)a.H * a.Lq * (double)a.Lk * a.D);
    int e;
    if (impl == 1 && h->x3 && (a.D == 32 || a.D == 64)) e = launch_attn_x3(a, st);        // split-bf16 on fp32 operands
    else if (impl == 1 && h->bf16 && (a.D == 32 || a.D == 64)) e = launch_attn_mfma(a, st);   // other head dims: exact generic kernel
    else e = launch_attn_generic(a, h->bf16, st);
    prof_end();
    if (e) err = fail(std::string("attention launch failed: ") + hipGetErrorString((hipError_t)e), e);
    return err;
  }
};

#define OTHER(run, call, what)              \
  do {                                      \
    (run).prof_begin(2, 0);                 \
    int e___ = (call);                      \
    (run).prof_end();                       \
    (run).other(e___, what);                \
  } while (0)

// ------------------------------------------------------------------------------------------------ episode cache (decode_launch, hfgpt_step_stack)
// the episode family of the handle: vima_seq_* (GPT / GATO, decoder-only) or vima_decode_* (VIMA / Flamingo, XAttnGPT)
bool ep_seq(const VimaHandle* h) { return h->cfg.policy_kind == VIMA_POLICY_GPT || h->cfg.policy_kind == VIMA_POLICY_GATO; }

// Layer i of the episode batch's caches (ep.B samples): the self-attention K | V cache [NL][ep.B][ep.Lmax][2E] and the prompt K / V cache
// [NL][ep.B][Lp][2E] (either layout)
void* ep_layer(const VimaHandle* h, int i) {
  return reinterpret_cast<char*>(h->ep.kv) + (size_t)i * h->ep.B * h->ep.Lmax * 2 * h->cfg.embed_dim * h->esz();
}
void* kv_layer(const VimaHandle* h, int i, int Lp) {
  return reinterpret_cast<char*>(h->pkv.ptr) + (size_t)i * h->ep.B * Lp * 2 * h->cfg.embed_dim * h->esz();
}

// c_attn of the new rows xT [rq = B Lq, E]: q dense [rq, E], k | v APPENDED to the layer's episode cache [B][Lmax][2E] by the GEMM's row-remap
// epilogue (row b Lq + i -> b Lmax + row + i). One launch (q columns dense, k | v columns remapped) where the split form exists, two otherwise.
int c_attn_append(Run& R, const Lin& c_attn, const void* xT, int rq, int Lq, int row, int Lmax, void* cache, void* q) {
  VimaHandle* h = R.h;
  const int E = h->cfg.embed_dim;
  if (h->bf16 && !c_attn.ws && E % 128 == 0 && !gemm_splitk_enabled(&h->tune)) {
    GemmArgs gq;
    gq.A = xT; gq.lda = E; R.setW(gq, c_attn, 0); gq.M = rq; gq.N = 3 * E; gq.K = E; gq.bias = c_attn.b;
    gq.outT_lo = q; gq.ldT_lo = E; gq.split_n = E;
    gq.outT = cache; gq.ldT = 2 * E; gq.rb = Lq; gq.s_hi = Lmax; gq.s_lo = 1; gq.ro = row;
    return R.gemm(gq);
  }
  GemmArgs gq;
  gq.A = xT; gq.lda = E; R.setW(gq, c_attn, 0); gq.M = rq; gq.N = E; gq.K = E; gq.bias = c_attn.b;
  gq.outT = q; gq.ldT = E;
  R.gemm(gq);
  GemmArgs gk;
  gk.A = xT; gk.lda = E; R.setW(gk, c_attn, E); gk.M = rq; gk.N = 2 * E; gk.K = E;
  gk.bias = c_attn.b ? c_attn.b + E : nullptr;
  gk.outT = cache; gk.ldT = 2 * E; gk.rb = Lq; gk.s_hi = Lmax; gk.s_lo = 1; gk.ro = row;
  return R.gemm(gk);
}

// The new queries q [B Lq, E] against the layer's episode cache: keys [0, Lk) under the episode key mask with the causal offset `row`. Linear cache:
// Lk = row + Lq, win_end = 0 (the plain rule). Ring: row is the write pointer, the keys are the whole written image [0, hw) and only the unit's own
// rows [row, win_end = row + Lq) are causal; the rows behind hold OLDER history of the ring, which stays visible (AttnArgs::win_end).
void attn_from_cache(Run& R, AttnArgs& s, const void* q, void* cache, int row, int Lmax, int Lk, int win_end) {
  const int E = R.h->cfg.embed_dim;
  s.q = q; s.ldq = E; s.k = cache; s.ldk = 2 * E; s.v = R.offT(cache, E); s.ldv = 2 * E;
  s.kmask = R.h->ep.mask; s.Lk = Lk; s.Lk_rows = Lmax; s.q_off = row; s.win_end = win_end;
}

// ------------------------------------------------------------------------------------------------ stages
// aux stream starts after everything already queued on the caller's stream / caller's stream waits for aux
int fork_aux(Run& R) {
  HIPCK(hipEventRecord(R.h->ev_fork, R.st));
  HIPCK(hipStreamWaitEvent(R.h->aux, R.h->ev_fork, 0));
  return 0;
}
int join_aux(Run& R) {
  HIPCK(hipEventRecord(R.h->ev_join, R.h->aux));
  HIPCK(hipStreamWaitEvent(R.st, R.h->ev_join, 0));
  return 0;
}

struct VitBuf { void* P; float* pre; float* x; void *hT, *qkv, *att, *u, *y; void *xT, *cT; void *h8 = nullptr, *att8 = nullptr, *u8 = nullptr; };   // xT / cT: stream in the operand type; *8: fp8 operands (precision "fp8")

// One ResidualAttentionBlock (vit.py:199-236) over M images of S tokens, for the object-crop ViT (vit_chunk) and the baselines' whole-frame ViT (rgb_vit):
//   ln_1 -> in_proj -> attention -> out_proj (+ stream) -> ln_2 -> fc (QuickGELU) -> proj (+ stream)
// on the stream in the operand type (b.xT, option stream_T) or in fp32 (b.x). sc: the block's four fp8 scales (null: operand-type activations): the LayerNorms and
// the attention then write e4m3 only, fc writes its hidden in e4m3 only. amax: the block's four max |x| slots (null: not calibrating).
// cls_only: the last block when only ln_post's row is wanted (vit.py:186): K / V of all rows from in_proj rows [W, 3W), Q of the cls rows (stride S W), and everything
// behind the attention on M rows, the residual read at stride S W and written compact to b.cT / b.pre (identical values for that row; the others are never read).
void vit_block(Run& R, const VimaHandle::VitBlock& B, int M, int S, const VitBuf& b, bool cls_only, const float* sc, float* amax) {
  VimaHandle* h = R.h;
  constexpr int W = kVitW;
  const bool sT = h->stream_T != 0;
  const int rows = M * S, n = cls_only ? M : rows;   // n: rows behind the attention
  auto s8 = [&](int site) { return sc ? sc[site] : 0.f; };
  const Opnd x{sT ? b.xT : nullptr, cls_only ? S * W : W, nullptr, 0.f, sT ? nullptr : b.x};                           // the stream as the residual GEMMs read it
  const Opnd xo = cls_only ? Opnd{sT ? b.cT : nullptr, W, nullptr, 0.f, sT ? nullptr : b.pre} : x;                      // ... and as they write it
  const Opnd h1{b.hT, W, b.h8, s8(0)}, att{sc ? nullptr : b.att, W, b.att8, s8(1)}, h2{b.hT, W, b.h8, s8(2)}, u{sc ? nullptr : b.u, 4 * W, b.u8, s8(3)};
  auto norm = [&](const Opnd& in, long long ldin, const float* g, const float* bb, int nrows, const Opnd& out) {
    if (in.p32) return R.ln(in.p32, ldin, g, bb, 1e-5f, 0, nrows, W, nullptr, out.p);
    if (out.s8 > 0.f) return R.lnT(in.p, ldin, g, bb, 1e-5f, 0, nrows, W, nullptr, nullptr, out.p8, 1.0f / out.s8);   // the bf16 stream straight to e4m3
    return R.lnT(in.p, ldin, g, bb, 1e-5f, 0, nrows, W, nullptr, out.p);
  };
  auto cal = [&](int site, const void* t, long long nrows, int cols) {
    if (amax) OTHER(R, launch_amax(t, cols, nrows, cols, amax + site, R.st), "amax");
  };
  norm(x, W, B.ln1g, B.ln1b, rows, h1);
  cal(0, b.hT, rows, W);
  int e;
  if (!cls_only) {
    R.linear(h1, B.in_proj, 0, 3 * W, rows, ACT_NONE, nullptr, Opnd{b.qkv, 3 * W});
    // nn.MultiheadAttention(768, 24) over the S tokens of an image: no mask, 1/sqrt(32) -- the per-(image, query, head) register kernel
    R.prof_begin(1, 4.0 * M * kVitHeads * (double)S * S * 32);
    e = launch_vit_attn(b.qkv, att.p, M, S, W, kVitHeads, h->bf16, R.st, sc ? att.p8 : nullptr, sc ? 1.0f / att.s8 : 1.0f);
  } else {
    R.linear(h1, B.in_proj, W, 2 * W, rows, ACT_NONE, nullptr, Opnd{b.qkv, 2 * W});                         // K, V of all S tokens
    R.linear(Opnd{h1.p, S * W, h1.p8, h1.s8}, B.in_proj, 0, W, M, ACT_NONE, nullptr, Opnd{b.y, W});         // Q of the cls token: A rows strided by S tokens
    R.prof_begin(1, 4.0 * M * kVitHeads * (double)S * 32);
    e = launch_vit_attn_cls(b.y, b.qkv, att.p, M, S, W, kVitHeads, h->bf16, R.st, sc ? att.p8 : nullptr, sc ? 1.0f / att.s8 : 1.0f);
  }
  R.prof_end();
  R.other(e, cls_only ? "vit_attn_cls" : "vit_attn");
  cal(1, b.att, n, W);
  R.linear(att, B.out_proj, 0, W, n, ACT_NONE, &x, xo);   // stream += attention (cls_only: xc = x_cls + attention)
  norm(xo, W, B.ln2g, B.ln2b, n, h2);
  cal(2, b.hT, n, W);
  R.linear(h2, B.fc, 0, 4 * W, n, ACT_QUICKGELU, nullptr, u);
  cal(3, b.u, n, 4 * W);
  R.linear(u, B.proj, 0, W, n, ACT_NONE, &xo, xo);
}

// ViT (vit.py:171-191) on internal crop rows [r0, r0+mc) -> cat[r0.., 0:768]
// f8mode 0: operand-type activations; 1: the same + max |x| of every fp8 site into amax[block * 4 + site] (calibration);
// 2: fp8 e4m3 activations into the 16 large GEMMs with the scales sc[block * 4 + site] (needs stream_T and a chunk whose GEMM
// shapes fit gemm_pp_kernel<.., F8>: the caller checks)
// mp >= mc: crop rows the chunk is COMPUTED on (option vit_pad: the next multiple of 256). The pad crops' patches are zeros; their rows run through every
// row-wise kernel and GEMM like any other crop's and land in cat rows [r0 + mc, r0 + mp), which belong to nobody (obj_encode sizes cat for them).
void vit_chunk(Run& R, const uint8_t* const crops[2], int per_view, int r0, int mc_valid, int mp, const VitBuf& b, void* cat, int f8mode = 0,
               float* amax = nullptr, const float* sc = nullptr) {
  VimaHandle* h = R.h;
  const int mc = mp;   // everything behind the patchify runs on the padded count
  if (mp > mc_valid) OTHER(R, (int)hipMemsetAsync(R.offT(b.P, (long long)mc_valid * 4 * kVitW), 0, (size_t)(mp - mc_valid) * 4 * kVitW * h->esz(), R.st), "vit_pad");
  // patchify, honouring the view boundary inside the chunk
  for (int vi = 0; vi < 2; ++vi) {
    const int lo = r0 > vi * per_view ? r0 : vi * per_view;
    const int hi_ = (r0 + mc_valid) < (vi + 1) * per_view ? (r0 + mc_valid) : (vi + 1) * per_view;
    if (hi_ > lo)
      OTHER(R, launch_patchify(crops[vi] + (size_t)(lo - vi * per_view) * 3072, R.offT(b.P, (long long)(lo - r0) * 4 * kVitW),
                               hi_ - lo, h->bf16, R.st), "patchify");
  }
  // conv1 as GEMM (vit.py:172), fp32 out
  R.linear(b.P, kVitW, h->vit.conv, mc * 4, ACT_NONE, nullptr, 0, nullptr, 0, b.pre, kVitW, nullptr, 0);
  const bool sT = h->stream_T != 0;   // residual stream carried in the operand type (see t5_layer_fused)
  OTHER(R, launch_vit_embed(b.pre, h->vit.cls, h->vit.pos, h->vit.lnpre_g, h->vit.lnpre_b, sT ? nullptr : b.x, sT ? b.xT : nullptr, mc,
                            h->bf16, R.st), "vit_embed");
  // the last block computes everything behind its K/V projection for the cls token only (option vit_prune_last) and leaves that row compact in b.cT / b.pre
  const bool prune = h->vit_prune_last != 0;
  for (int j = 0; j < kVitLayers; ++j)   // (the pad crops are zero images: real activations, inside the valid rows' range of a calibrating pass)
    vit_block(R, h->vit.blk[j], mc, 5, b, prune && j == kVitLayers - 1, f8mode == 2 ? sc + j * 4 : nullptr, f8mode == 1 ? amax + j * 4 : nullptr);
  // ln_post on the cls rows, then @ projection into cat[:, 0:768]   (vit.py:186-189)
  const long long ld_post = prune ? kVitW : 5 * kVitW;
  if (sT) R.lnT(prune ? b.cT : b.xT, ld_post, h->vit.lnpost_g, h->vit.lnpost_b, 1e-5f, 0, mc, kVitW, nullptr, b.y);
  else R.ln(prune ? b.pre : b.x, ld_post, h->vit.lnpost_g, h->vit.lnpost_b, 1e-5f, 0, mc, kVitW, nullptr, b.y);
  R.linear(b.y, kVitW, h->vit.projection, mc, ACT_NONE, nullptr, 0, nullptr, 0, nullptr, 0,
           R.offT(cat, (long long)r0 * 2 * kVitW), 2 * kVitW);
}

// ObjEncoder.forward (obj_encoder.py:66-95). Produces featT [n*2qv, E] (T) and optionally feat32 (fp32).
int obj_encode(Run& R, const uint8_t* const crops[2], const int64_t* const bbox[2], int n, int qv, float* feat32,
               void* featT) {
  VimaHandle* h = R.h;
  const int E = h->cfg.embed_dim;
  const int per_view = n * qv;
  const int M = 2 * per_view;   // internal crop row r = view * per_view + (i*qv + q)
  if (M == 0) return 0;
  // equal-size chunks (crops are independent); with dual_stream an even number of them, alternating between streams
  const int cmax = h->vit_chunk > 0 ? h->vit_chunk : M;
  const bool dual = h->dual_stream && M >= (h->dual_vit_crops > 512 ? h->dual_vit_crops : 512);
  int nchunks = (M + cmax - 1) / cmax;
  if (dual && (nchunks & 1)) ++nchunks;
  if (dual && nchunks < 2) nchunks = 2;
  int chunk = (M + nchunks - 1) / nchunks;
  // option vit_pad: chunks of a multiple of 256 crops (5 rows per crop: only then are the ViT's GEMMs whole 256-row tiles); the last chunk is computed on the
  // next multiple of 256 when that costs at most an eighth more rows (its pad crops are zero images whose features land behind row M of cat)
  const bool pad = h->vit_pad != 0 && chunk >= 1024;   // (5 120 rows: from there on the wide-N GEMMs of a chunk fill the chip with 256x256 tiles)
  if (pad) chunk = (chunk + 255) / 256 * 256;
  void* cat = R.wsT((size_t)(M + (pad ? 256 : 0)) * 2 * kVitW);   // [M (+ pad), 1536] = [vit feature | bbox feature]
  VitBuf vb[2];
  for (int i = 0; i < (dual ? 2 : 1); ++i) {
    vb[i].P = R.wsT((size_t)chunk * 4 * kVitW);
    vb[i].pre = R.ws<float>((size_t)chunk * 4 * kVitW);
    vb[i].x = R.ws<float>((size_t)chunk * 5 * kVitW);
    vb[i].hT = R.wsT((size_t)chunk * 5 * kVitW);
    vb[i].qkv = R.wsT((size_t)chunk * 5 * 3 * kVitW);
    vb[i].att = R.wsT((size_t)chunk * 5 * kVitW);
    vb[i].u = R.wsT((size_t)chunk * 5 * 4 * kVitW);
    vb[i].y = R.wsT((size_t)chunk * kVitW);
    vb[i].xT = h->stream_T ? R.wsT((size_t)chunk * 5 * kVitW) : nullptr;
    vb[i].cT = h->stream_T ? R.wsT((size_t)chunk * kVitW) : nullptr;
  }
  // precision "fp8": chunks whose GEMMs fit the fp8 kernel (full 256x256 tiles; >= 160 of them in the N = 768 GEMMs of the
  // cls-only last block, M = crops) take fp8 activations once the 16 site scales are calibrated; the first such call calibrates
  auto fits8 = [&](int mc) { return mc % 256 == 0 && (mc / 256) * (kVitW / 256) >= 160; };
  // ... and only while the handle's knobs leave the fp8-activation kernel reachable (gemm_a8_ok mirrors launch_gemm's eligibility incl. the
  // 32-bit offset bounds: with gemm_persist = 0, gemm_tile = 1, gemm_raster = 1 ... the stage keeps bf16 activations instead of failing)
  auto a8ok = [&](int mc) {
    return gemm_a8_ok(&h->tune, mc, kVitW, kVitW, kVitW, kVitW) && gemm_a8_ok(&h->tune, (long long)mc * 5, 3 * kVitW, kVitW, kVitW, kVitW) &&
           gemm_a8_ok(&h->tune, (long long)mc * 5, 4 * kVitW, kVitW, kVitW, kVitW) && gemm_a8_ok(&h->tune, (long long)mc * 5, kVitW, 4 * kVitW, 4 * kVitW, 4 * kVitW);
  };
  const bool can8 = h->a8 && h->bf16 && h->stream_T && h->vit_prune_last && fits8(chunk) && a8ok(chunk);
  Fp8Cal& c8 = h->cal8[CAL_VIT];
  const bool calibrate = can8 && !c8.ready;
  if (calibrate) {
    if (int e = cal_begin(h, c8, R.st)) return R.err = e;
    if (dual) { HIPCK(hipStreamSynchronize(R.st)); }   // the auxiliary stream's chunks must see the zeroed slots
  }
  if (can8 && c8.ready)
    for (int i = 0; i < (dual ? 2 : 1); ++i) {
      vb[i].h8 = R.ws<uint8_t>((size_t)chunk * 5 * kVitW);
      vb[i].att8 = R.ws<uint8_t>((size_t)chunk * 5 * kVitW);
      vb[i].u8 = R.ws<uint8_t>((size_t)chunk * 5 * 4 * kVitW);
    }
  if (R.err) return R.err;
  Run Rb{h, h->aux};
  if (dual && fork_aux(R)) return R.err = 1;
  int ci = 0;
  for (int r0 = 0; r0 < M; r0 += chunk, ++ci) {
    const int mc = (M - r0) < chunk ? (M - r0) : chunk;
    const int up = (mc + 255) / 256 * 256;
    const int mp = (pad && (up - mc) * 8 <= mc) ? up : mc;
    Run& Rc = (dual && (ci & 1)) ? Rb : R;
    const int f8mode = (can8 && fits8(mp) && a8ok(mp)) ? (c8.ready ? 2 : 1) : 0;
    vit_chunk(Rc, crops, per_view, r0, mc, mp, vb[dual ? (ci & 1) : 0], cat, f8mode, c8.amax, c8.scale.data());
    if (R.err || Rb.err) return R.err = (R.err ? R.err : Rb.err);
  }
  if (dual && join_aux(R)) return R.err = 1;
  if (calibrate)
    if (int e = cal_freeze(h, c8, R.st)) return R.err = e;
  // bbox MLP per view -> cat[:, 768:1536]; then per-view Linear(1536 -> E) scattered to [n, 2qv, E]
  void* t1 = R.wsT((size_t)per_view * 768);
  void* t2 = R.wsT((size_t)per_view * 768);
  if (R.err) return R.err;
  for (int vi = 0; vi < 2; ++vi) {
    OTHER(R, launch_bbox_l1((const long long*)bbox[vi], h->view[vi].w0, h->view[vi].b0, t1, per_view, 768, h->bf16, R.st), "bbox_l1");
    R.linear(t1, 768, h->view[vi].l1, per_view, ACT_RELU, nullptr, 0, nullptr, 0, nullptr, 0, t2, 768);
    void* catv = R.offT(cat, (long long)vi * per_view * 2 * kVitW);
    R.linear(t2, 768, h->view[vi].l2, per_view, ACT_NONE, nullptr, 0, nullptr, 0, nullptr, 0, R.offT(catv, kVitW), 2 * kVitW);
    GemmArgs a;
    a.A = catv; a.lda = 2 * kVitW; R.setW(a, h->view[vi].pre); a.M = per_view; a.N = E; a.K = 2 * kVitW;
    a.bias = h->view[vi].pre.b;
    a.out32 = feat32; a.ld32 = E; a.outT = featT; a.ldT = E;
    a.rb = qv; a.s_hi = 2 * qv; a.s_lo = 1; a.ro = vi * qv;
    R.gemm(a);
  }
  return R.err;
}

__global__ void concat_mask_kernel(const uint8_t* a, const uint8_t* b, uint8_t* out, int n, int qv) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n * 2 * qv) return;
  const int r = i / (2 * qv), c = i % (2 * qv);
  out[i] = c < qv ? (a[r * qv + c] ? 1 : 0) : (b[r * qv + (c - qv)] ? 1 : 0);
}

int concat_mask(Run& R, const uint8_t* const mask[2], int n, int qv, uint8_t* out) {
  if (n * qv == 0) return 0;
  R.prof_begin(2, 0);
  hipLaunchKernelGGL(concat_mask_kernel, dim3((n * 2 * qv + 255) / 256), dim3(256), 0, R.st, mask[0], mask[1], out, n, qv);
  R.prof_end();
  return R.other((int)hipGetLastError(), "concat_mask");
}

int t5_bias_table(VimaHandle* h, int L, float** out) {
  auto it = h->t5_bias_tables.find(L);
  if (it != h->t5_bias_tables.end()) { *out = it->second; return 0; }
  const int W = 2 * L - 1;
  std::vector<float> t((size_t)kT5Heads * W);
  for (int d = -(L - 1); d <= L - 1; ++d) {
    const int bkt = t5_bucket(d);
    for (int hh = 0; hh < kT5Heads; ++hh) t[(size_t)hh * W + d + L - 1] = h->t5_relbias_host[(size_t)bkt * kT5Heads + hh];
  }
  {   // distance from which THIS table is constant on both sides for every head (the T5 bucket function saturates at |delta| = 91):
      // AttnArgs::bias_far. Found by scanning the table itself, so it is exact whatever the bucket function.
    int far = L;   // L: never
    for (int n0 = L - 1; n0 >= 1; --n0) {
      bool same = true;
      for (int hh = 0; hh < kT5Heads && same; ++hh)
        same = t[(size_t)hh * W + n0 + L - 1] == t[(size_t)hh * W + (L - 1) + L - 1] && t[(size_t)hh * W - n0 + L - 1] == t[(size_t)hh * W + 0];
      if (!same) break;
      far = n0;
    }
    h->t5_bias_far[L] = far < L ? far : 0;
  }
  float* d = nullptr;
  HIPCK(hipMalloc((void**)&d, t.size() * 4));
  h->owned.push_back(d);
  HIPCK(hipMemcpy(d, t.data(), t.size() * 4, hipMemcpyHostToDevice));
  h->t5_bias_tables[L] = d;
  *out = d;
  return 0;
}

struct T5Buf { void *hT, *qkv, *ctx, *u; float *ssA, *ssB; void *h8 = nullptr, *ctx8 = nullptr, *u8 = nullptr; };   // ssA / ssB: RMS partial sums [rows][24] (fused path); *8: fp8 copies (precision "fp8")

// self-attention of a T5 layer (every form): q | k | v in b.qkv -> b.ctx, relative-position bias from `table`, no 1/sqrt(d)
AttnArgs t5_attn_args(Run& R, const T5Buf& b, const uint8_t* mask, const float* table, int B, int L) {
  AttnArgs a;
  a.q = b.qkv; a.ldq = 3 * kT5Model;
  a.k = R.offT(b.qkv, kT5Model); a.ldk = 3 * kT5Model;
  a.v = R.offT(b.qkv, 2 * kT5Model); a.ldv = 3 * kT5Model;
  a.out = b.ctx; a.ldo = kT5Model;
  a.kmask = mask; a.relbias = table; a.bias_far = R.h->t5_bias_far.count(L) ? R.h->t5_bias_far[L] : 0; a.B = B; a.H = kT5Heads; a.Lq = L; a.Lk = L; a.D = kT5D; a.scale = 1.0f;
  a.mode = ATTN_T5;
  return a;
}

void t5_layer(Run& R, const VimaHandle::T5Layer& Ly, float* x, const uint8_t* mask, const float* table, int B, int L,
              const T5Buf& b, int attn_impl) {
  const int rows = B * L;
  R.ln(x, kT5Model, Ly.rms1, nullptr, 1e-6f, 1, rows, kT5Model, nullptr, b.hT);
  R.linear(b.hT, kT5Model, Ly.qkv, rows, ACT_NONE, nullptr, 0, nullptr, 0, nullptr, 0, b.qkv, 3 * kT5Model);
  R.attn(t5_attn_args(R, b, mask, table, B, L), attn_impl);
  R.linear(b.ctx, kT5Model, Ly.o, rows, ACT_NONE, nullptr, 0, x, kT5Model, x, kT5Model, nullptr, 0);
  R.ln(x, kT5Model, Ly.rms2, nullptr, 1e-6f, 1, rows, kT5Model, nullptr, b.hT);
  R.linear(b.hT, kT5Model, Ly.wi, rows, ACT_RELU, nullptr, 0, nullptr, 0, nullptr, 0, b.u, kT5FF);
  R.linear(b.u, kT5FF, Ly.wo, rows, ACT_NONE, nullptr, 0, x, kT5Model, x, kT5Model, nullptr, 0);
}

// Same layer with both RMSNorms (T5LayerNorm: x * rsqrt(mean(x^2) + eps) * g, HF modeling_t5) folded into the GEMMs:
//   * g lives in the consumer's weight (W diag(g), packed once),
//   * the consumer reads the operand-type copy of the residual stream x (b.hT) that the PRODUCER of x wrote next to
//     the fp32 stream, and scales its accumulator rows by rsqrt(sum x^2 / 768 + eps),
//   * sum x^2 comes from the producer's epilogue as 24 per-32-column partials per row (deterministic, no atomics).
// Entry: b.hT / ssq_in describe the incoming x (`parts_in` partials per row); exit: b.hT and the returned buffer
// describe the outgoing x (24 partials). Removes two 600-MB HBM passes (fp32 read + bf16 write) per layer at cfg-3.
// One function for every fused form:
//   * option stream_T: the residual stream IS hT (operand type: bf16 in the bf16 / fp8w precisions, fp32 in the parity mode), hT = T(hT + ctx Wo^T) in place, and
//     the fp32 copy `x` is not maintained (4 instead of 10 bytes of HBM traffic per stream element and residual GEMM); stream_T = 0: the residual GEMMs update x
//     and write its operand-type copy to hT.
//   * sc (precision "fp8" after calibration, stream_T form only; null: operand-type activations) = this layer's four dequantisation scales followed by the next
//     layer's first one (0 for the last layer): fp8 e4m3 activations into all four GEMMs. The residual GEMMs write the fp8 copy of the new stream next to the bf16
//     stream, wi writes its ReLU hidden in fp8 only; the attention context is quantised by a separate pass (its kernel owns 64 of a row's 768 columns).
//   * amax (null: not calibrating): this layer's four max |x| slots of the calibrating pass.
//   * rows_gemm: option t5_pad, the GEMMs' row count (>= rows, a multiple of 256; the buffers hold that many).
const float* t5_layer_fused(Run& R, const VimaHandle::T5Layer& Ly, float* x, const uint8_t* mask, const float* table, int B, int L, const T5Buf& b,
                            int attn_impl, const float* ssq_in, int parts_in, const float* sc, float* amax, int rows_gemm) {
  const int rows = B * L;
  const int m = rows_gemm > rows ? rows_gemm : rows;
  constexpr int D = kT5Model, kParts = kT5Model / 32;
  auto s8 = [&](int site) { return sc ? sc[site] : 0.f; };
  auto hs = [&](int site) { return Opnd{b.hT, D, b.h8, s8(site), R.h->stream_T ? nullptr : x}; };   // the stream, as the input of / the output for `site`
  const Opnd ctx{b.ctx, D, b.ctx8, s8(1)}, u{sc ? nullptr : b.u, kT5FF, b.u8, s8(3)}, res = hs(0);
  // calibration of the fp8 activation scales: max |x| of the four GEMM inputs of this layer (bf16 tensors)
  auto cal = [&](int site, const void* t, int cols) {
    if (amax) OTHER(R, launch_amax(t, cols, rows, cols, amax + site, R.st), "amax");
  };
  cal(0, b.hT, D);
  R.linear(hs(0), Ly.qkv_g, 0, 3 * D, m, ACT_NONE, nullptr, Opnd{b.qkv, 3 * D}, ssq_in, parts_in);
  R.attn(t5_attn_args(R, b, mask, table, B, L), attn_impl);
  cal(1, b.ctx, D);
  if (sc) OTHER(R, launch_quant_fp8(b.ctx, D, rows, D, 1.0f / sc[1], b.ctx8, D, R.st), "quant_fp8");
  R.linear(ctx, Ly.o, 0, D, m, ACT_NONE, &res, hs(2), nullptr, 0, b.ssA);      // stream += ctx Wo^T; partial sums of its squares -> ssA
  cal(2, b.hT, D);
  R.linear(hs(2), Ly.wi_g, 0, kT5FF, m, ACT_RELU, nullptr, u, b.ssA, kParts);
  cal(3, b.u, kT5FF);
  R.linear(u, Ly.wo, 0, D, m, ACT_NONE, &res, hs(4), nullptr, 0, b.ssB);
  return b.ssB;
}

// T5 encoder stack on x fp32 [B*L, 768] (updated in place); result (after final RMSNorm) -> out32 and/or outT.
// Samples are independent, so with dual_stream the batch is split in two halves that run the 12 layers on two streams.
// `src` (vima_prompt_encode): the stack's input is still to be ASSEMBLED from word embeddings / object tokens (x == nullptr, `mask` is the
// output mask the assembly writes). With the fused RMSNorm chain and the stream in the operand type the assembly writes that chain's entry
// (operand-type rows + row sums of squares) directly and the fp32 prompt never exists; otherwise it is assembled into a workspace x first.
struct PromptSrc { const int* tok_src; const long long* word_ids; const float* objtok; const uint8_t* objmask; };

int t5_stack(Run& R, float* x, const uint8_t* mask, int B, int L, float* out32, void* outT, const PromptSrc* src = nullptr) {
  VimaHandle* h = R.h;
  float* table = nullptr;
  if (int e = t5_bias_table(h, L, &table)) return R.err = e;
  // Two streams (half the batch each) overlap one half's attention with the other's GEMMs and interleave partial rounds of tiles -- except where the whole batch's
  // N = 768 GEMMs are ONE nearly full round of 256x256 tiles (169 .. 256 of them: 14.4 k .. 21.8 k rows, e.g. batch 32 or 40 x 512 tokens): two half-filled grids side by
  // side are then slower than the one (batch 32: 9.10 -> 8.78 ms, batch 40: 10.57 -> 10.28; batch 24 / 48 / 64 the other way round: profiles/r06_dual_stream_thresholds.txt).
  // Option dual_t5_rows > 0 replaces the rule by a plain minimum row count.
  const long long t5_rows = (long long)B * L, t5_tiles768 = (t5_rows + 255) / 256 * (kT5Model / 256);
  // (169 .. 256 on the 256 CUs of an MI355X; the lower bound, about two thirds of a round, scales with the chip as the round does)
  const bool one_round = h->dual_t5_rows == 0 && t5_tiles768 > num_cu() * 168 / 256 && t5_tiles768 <= num_cu();
  const bool dual = h->dual_stream && B >= 2 && t5_rows >= h->dual_t5_rows && !one_round;
  const int nb[2] = {dual ? B - B / 2 : B, dual ? B / 2 : 0};
  // the halves: half 0 on the caller's stream, half 1 (dual only) on the auxiliary one. Every step below issues all of half 0's launches, then all of half 1's.
  struct Half { Run& R; int n; long long r0, rows; T5Buf b; const float* ss; int rpad; };   // samples, first row, row count, buffers, the running RMS statistics, padded row count
  Run Rb{h, h->aux};
  Half halves[2] = {{R, nb[0], 0, (long long)nb[0] * L, {}, nullptr, 0}, {Rb, nb[1], (long long)nb[0] * L, (long long)nb[1] * L, {}, nullptr, 0}};
  const int nh = dual ? 2 : 1;
  // option t5_pad: a half whose row count is not a multiple of 256 (the 256x256 tile kernels take nothing else) is computed on the next multiple when it has at
  // least 2048 rows: the pad rows enter as zeros, run through the GEMM chain like any row, are neither attended to nor read back (fused RMSNorm chain with the
  // stream in the operand type only; the fp8-activation layers need whole tiles of REAL rows and are left alone)
  for (int i = 0; i < nh; ++i) {
    Half& H = halves[i];
    if (h->t5_pad && h->t5_fuse_rms && h->stream_T && H.rows >= 2048 && H.rows % 256 != 0 && !gemm_splitk_enabled(&h->tune)) H.rpad = (int)((H.rows + 255) / 256 * 256);
    const size_t rows = H.rpad ? (size_t)H.rpad : (size_t)H.rows;
    H.b.hT = R.wsT(rows * kT5Model);
    H.b.qkv = R.wsT(rows * 3 * kT5Model);
    H.b.ctx = R.wsT(rows * kT5Model);
    H.b.u = R.wsT(rows * kT5FF);
    H.b.ssA = R.ws<float>(rows * (kT5Model / 32));
    H.b.ssB = R.ws<float>(rows * (kT5Model / 32));
  }
  // precision "fp8": fp8 activations when the four GEMM shapes of a layer fit the fp8 kernel (full 256x256 tiles, >= 160 of them for
  // the N = 768 GEMMs) and the scales are calibrated; the first pass of a handle calibrates (fp8w kernels + max |x| per site)
  auto fits8 = [&](int n) { const long long r = (long long)n * L; return n == 0 || (r % 256 == 0 && (r / 256) * (kT5Model / 256) >= 160); };
  auto a8ok = [&](int n) {   // the four GEMM shapes of a layer on the fp8-activation kernel with this handle's knobs (see obj_encode)
    const long long r = (long long)n * L;
    return n == 0 || (gemm_a8_ok(&h->tune, r, 3 * kT5Model, kT5Model, kT5Model, kT5Model) && gemm_a8_ok(&h->tune, r, kT5Model, kT5Model, kT5Model, kT5Model) &&
                      gemm_a8_ok(&h->tune, r, kT5FF, kT5Model, kT5Model, kT5Model) && gemm_a8_ok(&h->tune, r, kT5Model, kT5FF, kT5FF, kT5FF));
  };
  const bool can8 = h->a8 && h->bf16 && h->stream_T && h->t5_fuse_rms && !gemm_splitk_enabled(&h->tune) && fits8(nb[0]) && fits8(nb[1]) &&
                    a8ok(nb[0]) && a8ok(nb[1]);
  Fp8Cal& c8 = h->cal8[CAL_T5];
  const bool run8 = can8 && c8.ready;
  const bool calibrate = can8 && !c8.ready;
  if (calibrate)
    if (int e = cal_begin(h, c8, R.st)) return R.err = e;
  if (run8)
    for (int i = 0; i < nh; ++i) {
      Half& H = halves[i];
      H.b.h8 = R.ws<uint8_t>((size_t)H.rows * kT5Model);
      H.b.ctx8 = R.ws<uint8_t>((size_t)H.rows * kT5Model);
      H.b.u8 = R.ws<uint8_t>((size_t)H.rows * kT5FF);
    }
  if (R.err) return R.err;
  // with the opt-in split-K, small problems keep the standalone RMSNorm: the producer-side statistics are not available
  // from the two-pass split-K, and the norm kernels cost microseconds there
  const bool fused = h->t5_fuse_rms != 0 && (!gemm_splitk_enabled(&h->tune) || (long long)nb[0] * L >= 8192);
  const bool direct = src != nullptr && fused && h->stream_T != 0;   // the assembly writes the chain's entry itself
  if (src && !direct) {   // assemble the fp32 prompt first (before the halves diverge)
    x = R.ws<float>((size_t)B * L * kT5Model);
    if (R.err) return R.err;
    OTHER(R, launch_prompt_assemble(src->tok_src, src->word_ids, h->word_table, src->objtok, src->objmask, x, const_cast<uint8_t*>(mask),
                                    B * L, kT5Model, R.st), "prompt_assemble");
  }
  if (dual && fork_aux(R)) return R.err = 1;
  auto xh = [&](const Half& H) { return x ? x + H.r0 * kT5Model : nullptr; };   // the half's rows of the fp32 stream (direct assembly: there is none, and the stream_T layers never touch it)
  int parts = 1;
  for (int i = 0; i < nh; ++i) {   // entry of the fused chain: operand-type rows of the incoming x in hT and their row sums of squares (one partial per row) in ssB
    Half& H = halves[i];
    if (direct)
      OTHER(H.R, launch_prompt_assemble_stats(src->tok_src + H.r0, src->word_ids, h->word_table, src->objtok, src->objmask, H.b.hT, H.b.ssB,
                                              const_cast<uint8_t*>(mask) + H.r0, (int)H.rows, kT5Model, h->bf16, H.R.st), "prompt_assemble");
    else if (fused)
      H.R.other(launch_rms_stats(xh(H), (int)H.rows, kT5Model, H.b.hT, H.b.ssB, h->bf16, H.R.st), "rms_stats");
    if (fused) H.ss = H.b.ssB;
  }
  if (run8)   // entry: fp8 copy of the incoming stream with layer 0's first scale
    for (int i = 0; i < nh; ++i) {
      Half& H = halves[i];
      OTHER(H.R, launch_quant_fp8(H.b.hT, kT5Model, H.rows, kT5Model, 1.0f / c8.scale[0], H.b.h8, kT5Model, H.R.st), "quant_fp8");
    }
  for (int i = 0; i < nh; ++i)
    if (halves[i].rpad) {   // zero pad rows: the stream's entry, its entry statistics (one partial per row: what layer 0's qkv GEMM reads), and the attention output rows no attention launch writes
      Half& H = halves[i];
      const long long r = H.rows, np = H.rpad - r;
      HIPCK(hipMemsetAsync(R.offT(H.b.hT, r * kT5Model), 0, (size_t)np * kT5Model * h->esz(), H.R.st));
      HIPCK(hipMemsetAsync(R.offT(H.b.ctx, r * kT5Model), 0, (size_t)np * kT5Model * h->esz(), H.R.st));
      HIPCK(hipMemsetAsync(H.b.ssB + r, 0, (size_t)np * sizeof(float), H.R.st));
    }
  for (int l = 0; l < kT5Layers; ++l) {
    float sc[5];   // run8: this layer's four scales and the next layer's first one (0 behind the last layer: no e4m3 copy of the final stream)
    for (int k = 0; k < 5 && run8; ++k) sc[k] = l * 4 + k < kT5Layers * 4 ? c8.scale[l * 4 + k] : 0.f;
    for (int i = 0; i < nh; ++i) {
      Half& H = halves[i];
      if (fused)
        H.ss = t5_layer_fused(H.R, h->t5[l], xh(H), mask + H.r0, table, H.n, L, H.b, h->attn_impl, H.ss, parts, run8 ? sc : nullptr,
                              calibrate ? c8.amax + l * 4 : nullptr, H.rpad);
      else
        t5_layer(H.R, h->t5[l], xh(H), mask + H.r0, table, H.n, L, H.b, h->attn_impl);
    }
    parts = kT5Model / 32;
    if (R.err || Rb.err) return R.err = (R.err ? R.err : Rb.err);
  }
  for (int i = 0; i < nh; ++i) {   // final RMSNorm; with the fused chain and stream_T the stream lives in hT
    Half& H = halves[i];
    float* const o32 = out32 ? out32 + H.r0 * kT5Model : nullptr;
    void* const oT = outT ? R.offT(outT, H.r0 * kT5Model) : nullptr;
    if (fused && h->stream_T) H.R.lnT(H.b.hT, kT5Model, h->t5_final, nullptr, 1e-6f, 1, (int)H.rows, kT5Model, o32, oT);
    else H.R.ln(xh(H), kT5Model, h->t5_final, nullptr, 1e-6f, 1, (int)H.rows, kT5Model, o32, oT);
  }
  if (dual) {
    if (Rb.err) return R.err = Rb.err;
    if (join_aux(R)) return R.err = 1;
  }
  if (calibrate && !R.err)   // one-time: read the 48 maxima back and freeze the scales
    if (int e = cal_freeze(h, c8, R.st)) return R.err = e;
  return R.err;
}

int check_ready(VimaHandle* h) {
  if (!h) return fail("null handle");
  if (!h->finalized) return fail("weights not finalized: call vima_set_param for every key, then vima_finalize_params");
  HIPCK(hipSetDevice(h->device));
  if (h->arena.reset()) return fail("workspace reset failed");
  return 0;
}

int vima_only(VimaHandle* h, const char* fn) {
  if (!h) return fail("null handle");
  if (h->cfg.policy_kind != VIMA_POLICY_VIMA)
    return fail(std::string(fn) + ": object-crop entry point of VIMAPolicy called on a baseline-policy handle (use the vima_rgb_* entry points)");
  return 0;
}


// ---------------------------------------------------------------------------------------------- hipGraph replay
void drop_graphs(VimaHandle* h) {
  for (auto& kv : h->graphs) (void)hipGraphExecDestroy(kv.second.exec);
  h->graphs.clear();
  h->graph_seen.clear();
}

std::string gkey(const char* name, std::initializer_list<long long> vals) {
  std::string k = name;
  char buf[24];
  for (long long v : vals) {
    snprintf(buf, sizeof buf, ":%llx", (unsigned long long)v);
    k += buf;
  }
  return k;
}

// Runs fn(stream) -- the pure launch sequence of one entry point -- eagerly, or, in graph mode, as a captured and cached
// hipGraph on the handle's internal stream (ordered after / before the caller's stream by events; the caller's stream may
// be the legacy NULL stream, which cannot be captured). A key is captured the second time it is seen: the first, eager,
// run sizes the workspace, creates events and sets the kernels' function attributes. Anything that fails during a
// capture (e.g. the workspace had to grow) makes that key permanently eager.
// warm (optional): the key under which that first eager run is counted, for families of calls whose launch sequences differ only in values baked
// into the kernel arguments (ring mode of vima_decode_step: write pointer and keys read) -- one eager run warms the whole family and every member is
// captured the first time it is seen.
template <typename F>
int run_graphed(VimaHandle* h, std::string key, hipStream_t user, F&& fn, std::string warm = std::string()) {
  if (!h->graph_mode || h->prof) return fn(user);
  HIPCK(hipSetDevice(h->device));
  if (!h->gstream) {
    HIPCK(hipStreamCreateWithFlags(&h->gstream, hipStreamNonBlocking));
    HIPCK(hipEventCreateWithFlags(&h->ev_gin, hipEventDisableTiming));
    HIPCK(hipEventCreateWithFlags(&h->ev_gout, hipEventDisableTiming));
  }
  HIPCK(hipEventRecord(h->ev_gin, user));
  HIPCK(hipStreamWaitEvent(h->gstream, h->ev_gin, 0));
  const std::string gen = gkey("", {(long long)h->state_gen, (long long)h->arena.gen, h->bf16 ? 1 : 0});
  key += gen;
  int rc = 0;
  auto it = h->graphs.find(key);
  if (it != h->graphs.end()) {
    it->second.last_use = ++h->graph_clock;
    ++h->graph_replays;
    if (hipGraphLaunch(it->second.exec, h->gstream) != hipSuccess) rc = fail("hipGraphLaunch failed");
  } else {
    int& seen = h->graph_seen[warm.empty() ? key : warm + gen];
    int& dead = h->graph_seen[key];   // -1: this key stays eager (the same entry as `seen` without a warm key)
    if (seen < 1 || dead < 0) {
      if (seen == 0) seen = 1;
      rc = fn(h->gstream);
    } else if (hipStreamBeginCapture(h->gstream, hipStreamCaptureModeRelaxed) != hipSuccess) {
      (void)hipGetLastError();
      dead = -1;
      rc = fn(h->gstream);
    } else {
      const uint64_t gen0 = h->arena.gen;
      const int e = fn(h->gstream);
      hipGraph_t g = nullptr;
      const hipError_t ec = hipStreamEndCapture(h->gstream, &g);
      hipGraphExec_t exec = nullptr;
      if (!e && ec == hipSuccess && g && h->arena.gen == gen0 &&
          hipGraphInstantiate(&exec, g, nullptr, nullptr, 0) == hipSuccess) {
        if (h->graphs.size() >= 96) {   // evict the least recently used executable
          auto lru = h->graphs.begin();
          for (auto j = h->graphs.begin(); j != h->graphs.end(); ++j)
            if (j->second.last_use < lru->second.last_use) lru = j;
          (void)hipGraphExecDestroy(lru->second.exec);
          h->graphs.erase(lru);
        }
        h->graphs[key] = {exec, ++h->graph_clock};
        ++h->graph_captures;
        if (hipGraphLaunch(exec, h->gstream) != hipSuccess) rc = fail("hipGraphLaunch failed");
      } else {
        (void)hipGetLastError();
        dead = -1;
        rc = e ? e : fn(h->gstream);   // nothing ran during the failed capture
      }
      if (g) (void)hipGraphDestroy(g);
    }
  }
  HIPCK(hipEventRecord(h->ev_gout, h->gstream));
  HIPCK(hipStreamWaitEvent(user, h->ev_gout, 0));
  return rc;
}

// The launch sequence of vima_action_head (shared with vima_act): cast, the stacked first layers, the batched second layers, the
// grouped (or looped) last layers -> out_logits f32 [Rn,700]
int action_head_run(Run& R, const float* tokens, int Rn, float* out_logits) {
  VimaHandle* h = R.h;
  const int E = h->cfg.embed_dim;
  const int HH = kNumHeadsOut * kHeadHidden;
  void* tT = R.wsT((size_t)Rn * E);
  void* h1 = R.wsT((size_t)Rn * HH);
  void* h2 = R.wsT((size_t)Rn * HH);
  if (R.err) return R.err;
  OTHER(R, launch_cast(tokens, tT, (long long)Rn * E, h->bf16, R.st), "cast");
  R.linear(tT, E, h->head1, Rn, ACT_RELU, nullptr, 0, nullptr, 0, nullptr, 0, h1, HH);
  GemmArgs a;   // 12 independent 512x512 layers as one batched launch
  a.A = h1; a.lda = HH; a.bsA = kHeadHidden; a.W = h->head2_W; a.ldw = kHeadHidden; a.bsW = (long long)kHeadHidden * kHeadHidden;
  a.M = Rn; a.N = kHeadHidden; a.K = kHeadHidden; a.batch = kNumHeadsOut; a.bias = h->head2_b; a.bsBias = kHeadHidden;
  a.act = ACT_RELU; a.outT = h2; a.ldT = HH; a.bsT = kHeadHidden;
  R.gemm(a);
  if (h->head3_Wall && gemm_grouped_ok(&h->tune)) {   // the 12 last layers (512 -> 50 / 100 bins) as ONE grouped launch, bit-identical to the loop below
    GemmArgs b;
    b.A = h2; b.lda = HH; b.bsA = kHeadHidden; b.W = h->head3_Wall; b.ldw = kHeadHidden; b.M = Rn; b.N = 100; b.K = kHeadHidden;
    b.batch = kNumHeadsOut; b.grp_col = h->head3_col; b.bias = h->head3_ball; b.out32 = out_logits; b.ld32 = kLogits;
    R.gemm(b);
    return R.err;
  }
  int col = 0;
  for (int j = 0; j < kNumHeadsOut; ++j) {
    GemmArgs b;
    b.A = R.offT(h2, (long long)j * kHeadHidden); b.lda = HH; R.setW(b, h->head3[j]);
    b.M = Rn; b.N = kHeadBins[j]; b.K = kHeadHidden; b.bias = h->head3[j].b;
    b.out32 = out_logits + col; b.ld32 = kLogits;
    R.gemm(b);
    col += kHeadBins[j];
  }
  return R.err;
}

// The rest of vima_action_embed after its first layer t1 (operand type [Rn,1024]; shared with vima_act): the batched 4 x (256 -> 256)
// GEMM and the post layer -> out f32 [Rn,E]
int action_embed_tail(Run& R, void* t1, int Rn, float* out) {
  VimaHandle* h = R.h;
  const int E = h->cfg.embed_dim;
  GemmArgs a;
  a.A = t1; a.lda = 1024; a.bsA = 256; a.W = h->act1_W; a.ldw = 256; a.bsW = 256 * 256; a.M = Rn; a.N = 256; a.K = 256; a.batch = 4;
  a.bias = h->act1_b; a.bsBias = 256;
  if (E == 1024) {   // Identity post layer: the concatenated 4 x 256 outputs ARE the token
    a.out32 = out; a.ld32 = 1024; a.bs32 = 256;
    return R.gemm(a);
  }
  void* t2 = R.wsT((size_t)Rn * 1024);
  if (R.err) return R.err;
  a.outT = t2; a.ldT = 1024; a.bsT = 256;
  R.gemm(a);
  return R.linear(t2, 1024, h->act_post, Rn, ACT_NONE, nullptr, 0, nullptr, 0, out, E, nullptr, 0);
}

// host bounds {low[2], high[2]} of the position keys into the kernel's argument block
void set_bounds(ActSelectArgs& s, const float* bounds) {
  if (!bounds) return;
  s.has_bounds = 1;
  s.low[0] = bounds[0]; s.low[1] = bounds[1]; s.high[0] = bounds[2]; s.high[1] = bounds[3];
}

#include "baselines.inc"

// One unit of the running episode batch -- T env steps as ONE pass (decode_launch's incremental branch, seq_step_launch) of Lq = T (Q + 1) rows per
// sample (one fewer at batch step 0) at one row offset, one unit of the ring, instead of T passes of Q + 1 rows; 1 / T of the launches -- and its
// commit on success. A step (T = 1) is the only form that is graphed, under the caller's key. A longer chunk runs eager also with option "graphs":
// it is a rare call (prefill, resume), and every distinct (T, row, keys read) would be a graph of its own; the step graphs captured before stay
// valid (they read the episode state from the device and the plan from their key) and are replayed again from the next step on.
// Ring mode: the launch sequence of a step depends on (write pointer, keys read, action slot), not on the step number -- from the second lap on
// the write pointers repeat, so the set of captured graphs stays bounded however long the rollout runs -- and one eager step with an action slot
// warms all of them (`warm`: same shapes, same workspace, same kernels: the attention launcher picks by Lk < 64 / >= 64): each (write pointer,
// keys read) is captured when first seen.
template <class Launch, class Commit>
int episode_unit(VimaHandle* h, int T, hipStream_t stream, const std::string& key, const std::string& warm, Launch launch, Commit commit) {
  const int rc = T > 1 ? launch(stream) : run_graphed(h, key, stream, launch, warm);
  if (!rc) commit();
  return rc;
}

}  // namespace

// =================================================================================================== C ABI
extern "C" {

int vima_abi_version(void) { return VIMA_ABI_VERSION; }   // include/vima_hip.h
const char* vima_last_error(void) { return g_err.c_str(); }
int vima_t5_bucket(int rel) { return t5_bucket(rel); }
void vima_fp8_e4m3_encode(const float* src, uint8_t* dst, int64_t n) {
  for (int64_t i = 0; i < n; ++i) dst[i] = f32_to_e4m3(src[i]);
}

int vima_create(const VimaConfig* cfg, int device, VimaHandle** out) {
  if (!cfg || !out) return fail("vima_create: null argument");
  const int E = cfg->embed_dim;
  if (E <= 0 || cfg->xf_n_layers <= 0 || cfg->sattn_n_heads <= 0 || cfg->xattn_n_heads <= 0)
    return fail("vima_create: non-positive config value");
  if (E % cfg->sattn_n_heads || E % cfg->xattn_n_heads)   // components.py:120-123 raises ValueError
    return fail("dim (" + std::to_string(E) + ") must be divisible by num_heads", 22);
  const int ds = E / cfg->sattn_n_heads, dx = E / cfg->xattn_n_heads;
  auto head_ok = [](int d) { return d == 16 || d == 32 || d == 64 || d == 128; };   // 32 / 64: MFMA flash kernels
  if (!head_ok(ds) || !head_ok(dx))
    return fail("vima_create: head dim must be 16, 32, 64 or 128 (got " + std::to_string(ds) + "/" + std::to_string(dx) + ")");
  if (E % 64 || E > 1024) return fail("vima_create: embed_dim must be a multiple of 64 and <= 1024");
  if (cfg->precision != VIMA_PRECISION_FP32 && cfg->precision != VIMA_PRECISION_BF16 && cfg->precision != VIMA_PRECISION_FP8W &&
      cfg->precision != VIMA_PRECISION_FP8 && cfg->precision != VIMA_PRECISION_BF16X3)
    return fail("vima_create: bad precision");
  if (cfg->n_positions <= 0 || cfg->n_positions > 512 || cfg->xattn_n_positions <= 0) return fail("vima_create: bad table sizes");
  if (cfg->policy_kind < VIMA_POLICY_VIMA || cfg->policy_kind > VIMA_POLICY_FLAMINGO) return fail("vima_create: bad policy_kind");
  if (cfg->policy_kind == VIMA_POLICY_FLAMINGO) {   // the Perceiver has 8 heads whatever the width (vima_flamingo_policy.py:42-44)
    const int dp = E / 8;
    if (E % 8 || !(head_ok(dp) || dp == 40 || dp == 48 || dp == 80 || dp == 96)) return fail("vima_create: embed_dim / 8 is not a supported Perceiver head dim");
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail("vima_create: no HIP device available -- this library has no CPU fallback");
  if (device < 0 || device >= ndev) return fail("vima_create: bad device index");
  HIPCK(hipSetDevice(device));
  VimaHandle* h = new VimaHandle();
  h->cfg = *cfg;
  h->device = device;
  h->bf16 = cfg->precision != VIMA_PRECISION_FP32 && cfg->precision != VIMA_PRECISION_BF16X3;
  h->x3 = cfg->precision == VIMA_PRECISION_BF16X3;
  h->w8 = cfg->precision == VIMA_PRECISION_FP8W || cfg->precision == VIMA_PRECISION_FP8;
  h->a8 = cfg->precision == VIMA_PRECISION_FP8;
  if (hipStreamCreateWithFlags(&h->aux, hipStreamNonBlocking) != hipSuccess ||
      hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&h->ev_join, hipEventDisableTiming) != hipSuccess) {
    delete h;
    return fail("vima_create: could not create the auxiliary stream/events");
  }
  *out = h;
  return 0;
}

void vima_destroy(VimaHandle* h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  (void)hipDeviceSynchronize();
  for (void* p : h->owned) (void)hipFree(p);
  h->arena.release();
  for (auto e : h->ev_pool) (void)hipEventDestroy(e);
  for (auto e : h->ev_layer) (void)hipEventDestroy(e);
  if (h->pkv.ptr) (void)hipFree(h->pkv.ptr);
  if (h->ep.kv) (void)hipFree(h->ep.kv);
  if (h->ep.mask) (void)hipFree(h->ep.mask);
  if (h->ep.poscnt) (void)hipFree(h->ep.poscnt);
  if (h->ep.fresh) (void)hipFree(h->ep.fresh);
  drop_graphs(h);
  if (h->ev_gin) (void)hipEventDestroy(h->ev_gin);
  if (h->ev_gout) (void)hipEventDestroy(h->ev_gout);
  if (h->gstream) (void)hipStreamDestroy(h->gstream);
  if (h->ev_fork) (void)hipEventDestroy(h->ev_fork);
  if (h->ev_join) (void)hipEventDestroy(h->ev_join);
  if (h->aux) (void)hipStreamDestroy(h->aux);
  delete h;
}

int vima_set_param(VimaHandle* h, const char* name, const float* data, const int64_t* shape, int ndim) {
  if (!h || !name || !data || (ndim > 0 && !shape)) return fail("vima_set_param: null argument");
  if (h->finalized) return fail("vima_set_param: weights already finalized");
  HostParam p;
  int64_t n = 1;
  for (int i = 0; i < ndim; ++i) { p.shape.push_back(shape[i]); n *= shape[i]; }
  p.data.assign(data, data + n);
  h->host[name] = std::move(p);
  return 0;
}

int vima_finalize_params(VimaHandle* h) {
  if (!h) return fail("null handle");
  if (h->finalized) return 0;
  HIPCK(hipSetDevice(h->device));
  int e = pack_all(h);
  if (e) {
    for (void* p : h->owned) (void)hipFree(p);
    h->owned.clear();
    return e;
  }
  h->host.clear();
  h->finalized = true;
  HIPCK(hipDeviceSynchronize());
  return 0;
}

int64_t vima_required_params(const VimaConfig* cfg, char* buf, int64_t buflen) {
  // host-only: run the packer against an empty staging map and collect the "missing key" names
  if (!cfg) return -1;
  VimaHandle tmp;
  tmp.cfg = *cfg; tmp.bf16 = cfg->precision != VIMA_PRECISION_FP32 && cfg->precision != VIMA_PRECISION_BF16X3;
  std::string saved = g_err;
  (void)pack_all(&tmp);
  std::string msg = g_err;
  g_err = saved;
  std::string out;
  size_t pos = 0;
  const std::string tag = "missing key: ";
  std::set<std::string> seen;
  while ((pos = msg.find(tag, pos)) != std::string::npos) {
    pos += tag.size();
    size_t end = msg.find('\n', pos);
    const std::string key = msg.substr(pos, end == std::string::npos ? std::string::npos : end - pos);
    if (!seen.insert(key).second) continue;   // a key the packer reads twice (e.g. a norm weight folded into a GEMM weight)
    out += key;
    out.push_back('\0');
  }
  if (buf && buflen >= (int64_t)out.size()) memcpy(buf, out.data(), out.size());
  return (int64_t)out.size();
}

int vima_set_option(VimaHandle* h, const char* key, int64_t value) {
  if (!h || !key) return fail("vima_set_option: null argument");
  const std::string k = key;
  ++h->state_gen;   // any option may change what a captured launch sequence contains
  if (!h->graphs.empty()) {
    HIPCK(hipSetDevice(h->device));
    HIPCK(hipDeviceSynchronize());
  }
  drop_graphs(h);
  if (k == "graphs") h->graph_mode = (int)value;
  else if (k == "attn_impl") h->attn_impl = (int)value;
  else if (k == "gemm_variant") h->tune.gemm_variant = (int)value;
  else if (k == "gemm_tile") h->tune.gemm_tile = (int)value;
  else if (k == "gemm_raster") h->tune.gemm_raster = (int)value;
  else if (k == "gemm_epi") h->tune.gemm_epi = (int)value;
  else if (k == "gemm_persist") h->tune.gemm_persist = (int)value;
  else if (k == "gemm_splitk") h->tune.gemm_splitk = (int)value;
  else if (k == "gemm_wide") h->tune.gemm_wide = (int)value;
  else if (k == "gemm_q4") h->tune.gemm_q4 = (int)value;
  else if (k == "gemm_q4_rs") h->tune.gemm_q4_rs = (int)value;
  else if (k == "gemm_pp") h->tune.gemm_pp = (int)value;
  else if (k == "gemm_small") h->tune.gemm_small = (int)value;
  else if (k == "gemm_resident") h->tune.gemm_resident = (int)value;
  else if (k == "gemm_res_maxwg") h->tune.gemm_res_maxwg = (int)value;
  else if (k == "gemm_res_nch") h->tune.gemm_res_nch = (int)value;
  else if (k == "gemm_skinny") h->tune.gemm_skinny = (int)value;
  else if (k == "gemm_flat") h->tune.gemm_flat = (int)value;

  else if (k == "gemm_dbg_ptr") h->tune.gemm_dbg = reinterpret_cast<long long*>((uintptr_t)value);
  else if (k == "attn4_min_lq") h->tune.attn4_min_lq = (int)value;
  else if (k == "attn_qg") h->tune.attn_qg = (int)value;
  else if (k == "attn_dbg_ptr") h->tune.attn_dbg = reinterpret_cast<long long*>((uintptr_t)value);
  else if (k == "attn_split") h->tune.attn_split = (int)value;
  else if (k == "vit_chunk") h->vit_chunk = (int)value;
  else if (k == "vit_pad") h->vit_pad = (int)value;
  else if (k == "t5_pad") h->t5_pad = (int)value;
  else if (k == "dual_t5_rows") h->dual_t5_rows = (int)value;
  else if (k == "dual_vit_crops") h->dual_vit_crops = (int)value;
  else if (k == "vit_prune_last") h->vit_prune_last = (int)value;
  else if (k == "dual_stream") h->dual_stream = (int)value;
  else if (k == "op_bf16_out") h->op_bf16_out = (int)value;
  else if (k == "op_stream_T") h->op_stream_T = (int)value;
  else if (k == "op_bias_far") h->op_bias_far = (int)value;
  else if (k == "geglu_pair") h->geglu_pair = (int)value;
  else if (k == "ln_fuse") h->ln_fuse = (int)value;
  // The episode has ONE live flag for both families (ep_seq): decode_ring ends the running episode of every handle kind, kv_headmajor that of an
  // XAttnGPT handle, seq_ring that of a decoder-only handle -- start a new one with vima_decode_step(step = 0) / vima_seq_prefill
  else if (k == "kv_headmajor") { h->kv_headmajor = (int)value; h->pkv.valid = false; if (!ep_seq(h)) h->ep.live = false; }   // the next decode rebuilds the cache in the chosen layout
  else if (k == "decode_ring") { h->decode_ring = value != 0; h->ep.live = false; }
  else if (k == "seq_ring") { h->seq_ring = value != 0; if (ep_seq(h)) h->ep.live = false; }
  else if (k == "restart_batched") h->restart_batched = (int)value;
  else if (k == "t5_fuse_rms") h->t5_fuse_rms = (int)value;
  else if (k == "stream_T") h->stream_T = (int)value;
  else if (k == "fp8_headroom_pct" || k == "fp8_recalibrate") {   // precision "fp8": measure the activation scales (of every group) again
    if (k == "fp8_headroom_pct") h->fp8_headroom_pct = value < 100 ? 100 : (int)value;
    for (Fp8Cal& c : h->cal8) c.ready = false;
  }
  else return fail("vima_set_option: unknown key " + k);
  return 0;
}

int vima_fp8_act_scales(VimaHandle* h, int group, float* out, int max_n) {
  if (!h) { (void)fail("null handle"); return -1; }
  if (group < 0 || group > CAL_KV || !h->cal8[group].ready) return 0;
  const std::vector<float>& v = h->cal8[group].scale;
  const int n = (int)v.size();
  for (int i = 0; i < n && i < max_n; ++i) out[i] = v[i];
  return n;
}

int vima_prof_enable(VimaHandle* h, int on) {
  if (!h) return fail("null handle");
  h->prof = on != 0;
  h->recs.clear();
  h->ev_used = 0;
  return 0;
}

int vima_prof_read_gemm_kernels(VimaHandle* h, int max_n, int32_t* ids, double* ms, int64_t* launches, double* flops, double* bytes) {
  if (!h || max_n < 0 || (max_n > 0 && (!ids || !ms || !launches || !flops || !bytes))) {
    (void)fail("vima_prof_read_gemm_kernels: bad argument");
    return -1;
  }
  std::map<int, int> slot;
  int n = 0;
  for (auto& r : h->recs) {
    if (r.cls != 0 && r.cls != 3) continue;
    float t = 0.f;
    if (hipEventSynchronize(r.b) != hipSuccess || hipEventElapsedTime(&t, r.a, r.b) != hipSuccess) {
      (void)fail("vima_prof_read_gemm_kernels: event query failed");
      return -1;
    }
    auto it = slot.find(r.kid);
    int i;
    if (it == slot.end()) {
      if (n >= max_n) continue;
      i = n++;
      slot[r.kid] = i;
      ids[i] = r.kid; ms[i] = 0; launches[i] = 0; flops[i] = 0; bytes[i] = 0;
    } else {
      i = it->second;
    }
    ms[i] += t; launches[i] += 1; flops[i] += r.flops; bytes[i] += r.bytes;
  }
  return n;
}

int vima_prof_read_gemm_launches(VimaHandle* h, int max_n, int32_t* ids, int32_t* mnk, float* us) {
  if (!h || max_n < 0 || (max_n > 0 && (!ids || !mnk))) {
    (void)fail("vima_prof_read_gemm_launches: bad argument");
    return -1;
  }
  int n = 0;
  for (auto& r : h->recs) {
    if (r.cls != 0 && r.cls != 3) continue;
    if (n < max_n) {
      ids[n] = r.kid; mnk[3 * n] = r.M; mnk[3 * n + 1] = r.N; mnk[3 * n + 2] = r.K;
      if (us) {
        float t = 0.f;
        if (hipEventSynchronize(r.b) != hipSuccess || hipEventElapsedTime(&t, r.a, r.b) != hipSuccess) {
          (void)fail("vima_prof_read_gemm_launches: event query failed");
          return -1;
        }
        us[n] = t * 1e3f;
      }
    }
    ++n;
  }
  return n;
}

int vima_prof_read_ex(VimaHandle* h, double out_ms[4], int64_t out_launches[4], double out_flops[4], double out_bytes[4]) {
  if (!h) return fail("null handle");
  for (int i = 0; i < 4; ++i) { out_ms[i] = 0; out_launches[i] = 0; out_flops[i] = 0; out_bytes[i] = 0; }
  for (auto& r : h->recs) {
    HIPCK(hipEventSynchronize(r.b));
    float ms = 0.f;
    HIPCK(hipEventElapsedTime(&ms, r.a, r.b));
    out_ms[r.cls] += ms;
    out_launches[r.cls] += 1;
    out_flops[r.cls] += r.flops;
    out_bytes[r.cls] += r.bytes;
  }
  h->recs.clear();
  h->ev_used = 0;
  return 0;
}

int vima_prof_read(VimaHandle* h, double out_ms[3], int64_t out_launches[3], double out_flops[3]) {
  double ms[4], fl[4], by[4];
  int64_t n[4];
  if (int e = vima_prof_read_ex(h, ms, n, fl, by)) return e;
  ms[0] += ms[3]; n[0] += n[3]; fl[0] += fl[3];   // class 3 is a GEMM class
  for (int i = 0; i < 3; ++i) { out_ms[i] = ms[i]; out_launches[i] = n[i]; out_flops[i] = fl[i]; }
  return 0;
}

int64_t vima_workspace_bytes(VimaHandle* h) { return h ? (int64_t)h->arena.bytes() : 0; }

int vima_graph_stats(VimaHandle* h, int64_t* replays, int64_t* captures) {
  if (!h || !replays || !captures) return fail("vima_graph_stats: null argument");
  *replays = h->graph_replays;
  *captures = h->graph_captures;
  return 0;
}

int vima_obj_encode(VimaHandle* h, const uint8_t* const crops[2], const int64_t* const bbox[2], int n, int qv, float* out,
                    vima_stream_t stream) {
  if (int e = vima_only(h, "vima_obj_encode")) return e;
  if (int e = check_ready(h)) return e;
  Run R{h, (hipStream_t)stream};
  void* featT = R.wsT((size_t)n * 2 * qv * h->cfg.embed_dim);
  if (R.err) return R.err;
  return obj_encode(R, crops, bbox, n, qv, out, featT);
}

int vima_obs_encode(VimaHandle* h, const uint8_t* const crops[2], const int64_t* const bbox[2],
                    const uint8_t* const mask[2], const int64_t* ee, int n, int qv, float* out_tokens, uint8_t* out_mask,
                    vima_stream_t stream) {
  if (int e = vima_only(h, "vima_obs_encode")) return e;
  const std::string key = gkey("obs_encode", {(long long)(uintptr_t)crops[0], (long long)(uintptr_t)crops[1], (long long)(uintptr_t)bbox[0],
                                              (long long)(uintptr_t)bbox[1], (long long)(uintptr_t)mask[0], (long long)(uintptr_t)mask[1],
                                              (long long)(uintptr_t)ee, n, qv, (long long)(uintptr_t)out_tokens, (long long)(uintptr_t)out_mask});
  return run_graphed(h, key, (hipStream_t)stream, [&](hipStream_t st) -> int {
    if (int e = check_ready(h)) return e;
    Run R{h, st};
    const int E = h->cfg.embed_dim;
    const int rows = n * 2 * qv;
    if (rows == 0) return 0;
    void* featT = R.wsT((size_t)rows * E);
    if (R.err) return R.err;
    if (obj_encode(R, crops, bbox, n, qv, nullptr, featT)) return R.err;
    // obs_fusion_layer on cat(img_feats, ee_feats) (vima_policy.py:253-256)
    R.linear(featT, E, h->fuse, rows, ACT_NONE, nullptr, 0, nullptr, 0, out_tokens, E, nullptr, 0);
    OTHER(R, launch_add_row_table(out_tokens, rows, E, h->ee_table, (const long long*)ee, 2 * qv, R.st), "ee_table");
    concat_mask(R, mask, n, qv, out_mask);
    return R.err;
  });
}

int vima_t5_encode(VimaHandle* h, const float* x, const uint8_t* mask, int B, int L, float* out, vima_stream_t stream) {
  if (int e = check_ready(h)) return e;
  Run R{h, (hipStream_t)stream};
  const size_t n = (size_t)B * L * kT5Model;
  float* xw = R.ws<float>(n);
  if (R.err) return R.err;
  HIPCK(hipMemcpyAsync(xw, x, n * 4, hipMemcpyDeviceToDevice, R.st));
  return t5_stack(R, xw, mask, B, L, out, nullptr);
}

int vima_prompt_encode(VimaHandle* h, const int64_t* word_ids, int n_words, const uint8_t* const crops[2],
                       const int64_t* const bbox[2], const uint8_t* const mask[2], int n_img, int qv,
                       const int32_t* tok_src, int B, int Lp, float* out_tokens, uint8_t* out_mask, vima_stream_t stream) {
  if (int e = vima_only(h, "vima_prompt_encode")) return e;
  if (int e = check_ready(h)) return e;
  (void)n_words;
  Run R{h, (hipStream_t)stream};
  const int E = h->cfg.embed_dim;
  const int orows = n_img * 2 * qv;
  float* objtok = R.ws<float>((size_t)(orows > 0 ? orows : 1) * 768);
  uint8_t* objmask = R.ws<uint8_t>((size_t)(orows > 0 ? orows : 1));
  if (R.err) return R.err;
  if (orows > 0) {
    void* featT = R.wsT((size_t)orows * E);
    void* p1 = R.wsT((size_t)orows * 768);
    void* p2 = R.wsT((size_t)orows * 768);
    if (R.err) return R.err;
    if (obj_encode(R, crops, bbox, n_img, qv, nullptr, featT)) return R.err;
    // prompt_obj_post_layer (vima_policy.py:165)
    R.linear(featT, E, h->pobj[0], orows, ACT_RELU, nullptr, 0, nullptr, 0, nullptr, 0, p1, 768);
    R.linear(p1, 768, h->pobj[1], orows, ACT_RELU, nullptr, 0, nullptr, 0, nullptr, 0, p2, 768);
    R.linear(p2, 768, h->pobj[2], orows, ACT_NONE, nullptr, 0, nullptr, 0, objtok, 768, nullptr, 0);
    concat_mask(R, mask, n_img, qv, objmask);
  }
  const int rows = B * Lp;
  const PromptSrc src{tok_src, (const long long*)word_ids, objtok, objmask};   // assembled inside the stack (see t5_stack)
  if (!h->has_t5_post) return t5_stack(R, nullptr, out_mask, B, Lp, out_tokens, nullptr, &src);
  void* yT = R.wsT((size_t)rows * 768);
  if (R.err) return R.err;
  if (t5_stack(R, nullptr, out_mask, B, Lp, nullptr, yT, &src)) return R.err;
  return R.linear(yT, 768, h->t5_post, rows, ACT_NONE, nullptr, 0, nullptr, 0, out_tokens, E, nullptr, 0);
}

// vima_decode (step < 0: the whole history is re-fed, like the reference) and vima_decode_step (step >= 0: only the newest
// tokens of env step `step` are processed against the episode's cached self-attention K/V) share three stages:
// decode_prepare (validation, cache (re)allocation, state invalidation -- host only), decode_launch (the pure launch
// sequence: eager, captured or replayed) and decode_commit (host state after a successful launch).
// u: the unit of the episode book this call writes (episode_book.h: first cache row = the history length or the ring's write pointer, rows, keys the
// self-attention reads and the end of its causal window); a full-history call has only u.Lq
struct DecodePlan { bool inc; int has_act, kv_mode; EpisodeBook::Plan u; };

// the samples a restart call flags (restart: HOST array [B])
static std::vector<int> flagged_list(const uint8_t* restart, int B) {
  std::vector<int> list;
  for (int b = 0; b < B; ++b)
    if (restart[b]) list.push_back(b);
  return list;
}

// A unit the book refuses (vima_decode_step / _chunk, vima_seq_decode_step / _chunk): code 34, nothing has changed
static int plan_refused(const char* fn, const char* restart_fn, const EpisodeBook& bk, const EpisodeBook::Plan& p, int T) {
  const std::string what = std::string(fn) + ": " + std::to_string(T) + " step(s) from step " + std::to_string(bk.next);
  const std::string space = "n_positions " + std::to_string(bk.Lmax) + " - " + std::to_string(bk.P0);
  if (p.refused == EpisodeBook::FULL)
    return fail(what + " do not fit in front of n_positions " + std::to_string(bk.Lmax) + " (" + std::to_string(bk.wp) + " cache rows in use, room for " +
                std::to_string(p.fit) + " more steps)", 34);
  if (p.refused == EpisodeBook::TOO_LONG) return fail(what + " are longer than the whole ring (" + space + " rows)", 34);
  return fail(what + ": the episode of sample " + std::to_string(p.sample) + " is longer than the ring (" + std::to_string(p.age) + " + " +
              std::to_string(p.advance) + " ring rows > " + space + "): restart it with " + restart_fn +
              ", or take fewer steps at once (a chunk skips the ring's tail as ONE unit)", 34);
}

// THE check that an episode batch of the entry's family is running (seq: the vima_seq_* entries, else vima_decode_*). B / Lp: what the entry
// compares (kAny: not that one); prompt_kv: the batch's prompt K / V cache must stand too (the XAttnGPT entries that read or rebuild it; valid
// beside a live episode it has the batch's B and Lp: only decode_commit writes the three). which: how the entry words the batch it asks for;
// family: its own refusal of a handle of the other family (nullptr: it has none, such a handle simply has no running batch)
constexpr int kAny = -1;
static int ep_running(const VimaHandle* h, const char* fn, bool seq, int B, int Lp, bool prompt_kv, const char* which, const char* family = nullptr) {
  const bool mine = ep_seq(h) == seq;
  if (!mine && family) return fail(std::string(fn) + ": " + family);
  const VimaHandle::Episode& e = h->ep;
  if (mine && e.live && (B == kAny || e.B == B) && (Lp == kAny || e.Lp == Lp) && (!prompt_kv || (h->pkv.valid && h->pkv.B == e.B && h->pkv.Lp == e.Lp)))
    return 0;
  return fail(std::string(fn) + ": no running episode batch" + which + " (start one with " + (seq ? "vima_seq_prefill)" : "vima_decode_step(step = 0))"));
}

// A history longer than the room (EpisodeBook::history): code 34, nothing has changed. lead: "<entry>: a history of T steps" / "<entry>: snapshot i
// holds n steps and"
static int room_refused(const std::string& lead, int room) {
  return fail(lead + " does not fit: room for " + std::to_string(room) + " (the batch steps whose cache rows are all still there)", 34);
}

// The episode caches for B samples of Lmax rows: per-layer self-attention K | V [layer][B][Lmax][2E], key mask [B][Lmax], position counter and
// restart flag [B]. Grown (never shrunk) on demand; a reallocation invalidates the captured graphs.
static int ep_reserve(VimaHandle* h, int B, int Lmax) {
  const size_t need = (size_t)h->cfg.xf_n_layers * B * Lmax * 2 * h->cfg.embed_dim * h->esz();
  if (h->ep.kv_bytes >= need && h->ep.aux_cap >= (size_t)B * Lmax) return 0;
  HIPCK(hipDeviceSynchronize());
  if (h->ep.kv) (void)hipFree(h->ep.kv);
  if (h->ep.mask) (void)hipFree(h->ep.mask);
  if (h->ep.poscnt) (void)hipFree(h->ep.poscnt);
  if (h->ep.fresh) (void)hipFree(h->ep.fresh);
  h->ep.kv = nullptr; h->ep.mask = nullptr; h->ep.poscnt = nullptr; h->ep.fresh = nullptr; h->ep.kv_bytes = 0; h->ep.aux_cap = 0;
  HIPCK(hipMalloc(&h->ep.kv, need));
  HIPCK(hipMalloc((void**)&h->ep.mask, (size_t)B * Lmax));
  HIPCK(hipMalloc((void**)&h->ep.poscnt, (size_t)B * sizeof(int)));
  HIPCK(hipMalloc((void**)&h->ep.fresh, (size_t)B));
  h->ep.kv_bytes = need; h->ep.aux_cap = (size_t)B * Lmax;
  ++h->state_gen;
  return 0;
}

static int decode_prepare(VimaHandle* h, const float* act_tok, int T, int B, int Q, int L_act, int Lp, int kv_cache_mode, int step,
                          DecodePlan& P) {
  if (!h) return fail("null handle");
  if (!h->finalized) return fail("weights not finalized: call vima_set_param for every key, then vima_finalize_params");
  if (h->cfg.policy_kind != VIMA_POLICY_VIMA && h->cfg.policy_kind != VIMA_POLICY_FLAMINGO)
    return fail("vima_decode: the handle's policy has no XAttnGPT (decoder-only baselines use vima_seq_decode)");
  HIPCK(hipSetDevice(h->device));
  const int E = h->cfg.embed_dim;
  const bool inc = step >= 0;
  if (T <= 0 || B <= 0 || Q <= 0) return fail("vima_decode: empty input");
  if (!inc && (L_act < 0 || L_act > T || (L_act > 0 && !act_tok) || L_act < T - 1)) return fail("vima_decode: L_act must be T-1 or T");
  const int has_act = inc && step > 0 ? 1 : 0;
  const int L_hist = inc && step > 0 ? step * (Q + 1) - 1 : 0;     // tokens already in the episode cache
  // tokens processed by this call, per sample. Incremental: T env steps (vima_decode_step: 1; vima_decode_chunk: more), each a slot of
  // [action, Q obs] rows; the first slot of batch step 0 has no action row
  const int Lmax = h->cfg.n_positions;
  const bool chunk = inc && T > 1;
  const char* fn = chunk ? "vima_decode_chunk" : "vima_decode_step";
  // dec_embed_chunk_kernel's pos_s[512]. The bound is on T full slots of Q + 1 rows: batch step 0 has one row fewer and is held to the same T and Q
  if (inc && (long long)T * (Q + 1) > 512)
    return fail(std::string(fn) + ": an incremental call holds at most 512 rows in T slots of Q + 1 (T (Q + 1) = " + std::to_string((long long)T * (Q + 1)) + ")");
  const int Lq = inc ? T * (Q + 1) - (has_act ? 0 : 1) : T * Q + L_act;
  const bool ring = inc && h->decode_ring != 0;
  if (chunk && !ring && L_hist + Lq > Lmax)
    return fail("vima_decode_chunk: " + std::to_string(T) + " steps from step " + std::to_string(step) + " need " + std::to_string(L_hist + Lq) +
                " cache rows > n_positions " + std::to_string(Lmax) + " (room for " + std::to_string(std::max(0, (Lmax + 1) / (Q + 1) - step)) +
                " more steps)", 34);
  if (ring ? Lq > Lmax : L_hist + Lq > h->cfg.n_positions) return fail("vima_decode: history longer than n_positions", 34);
  if (Lp > h->cfg.xattn_n_positions)   // xattn_gpt.py:110 assert
    return fail("AssertionError: prompt_tokens.size(1) <= xattn_n_positions (" + std::to_string(Lp) + " > " +
                std::to_string(h->cfg.xattn_n_positions) + ")", 33);
  EpisodeBook::Plan u{};
  u.Lq = Lq;
  if (inc) {
    if (has_act && !act_tok) return fail("vima_decode_step: the previous action token is required for step > 0");
    if (chunk && !act_tok) return fail("vima_decode_chunk: the action tokens between the chunk's steps are required");
    if (step > 0 && !(h->ep.live && h->ep.book.next == step && h->ep.B == B && h->ep.Q == Q && h->ep.Lp == Lp && h->pkv.valid))
      return fail(std::string(fn) + ": step " + std::to_string(step) + " does not continue the episode state (last step " +
                  std::to_string(h->ep.live ? h->ep.book.next - 1 : -1) + "); start an episode with step 0");
    kv_cache_mode = step == 0 ? 1 : 2;
    if (step == 0) {   // a new episode batch: the one that ran ends here
      if (int e = ep_reserve(h, B, Lmax)) return e;
      h->ep.live = false; h->ep.B = B; h->ep.Lmax = Lmax;   // the caches' shape (ep_layer); the episode itself is live from decode_commit on
      h->ep.book.begin(B, Q, 0, Lmax, ring);
    }
    u = h->ep.book.plan(T);   // the book is at `step` (the continuity check above): a chunk is ONE unit of Lq rows
    if (u.refused) return plan_refused(fn, "vima_decode_restart", h->ep.book, u, T);
  }
  if (kv_cache_mode < 0 || kv_cache_mode > 2) return fail("vima_decode: kv_cache_mode must be 0, 1 or 2");
  if (kv_cache_mode == 2 && !(h->pkv.valid && h->pkv.B == B && h->pkv.Lp == Lp))
    return fail("vima_decode: kv_cache_mode 2 without a matching cache (build it with mode 1 for the same B, Lp)");
  if (kv_cache_mode == 1) {
    const size_t need = (size_t)B * Lp * 2 * E * h->esz() * h->cfg.xf_n_layers;
    h->pkv.valid = false;
    if (h->pkv.bytes < need) {
      HIPCK(hipDeviceSynchronize());
      if (h->pkv.ptr) (void)hipFree(h->pkv.ptr);
      h->pkv.ptr = nullptr; h->pkv.bytes = 0;
      HIPCK(hipMalloc(&h->pkv.ptr, need));
      h->pkv.bytes = need;
      ++h->state_gen;
    }
  }
  if (!inc) h->ep.live = false;   // a full-history call may rebuild the prompt cache: the episode state no longer matches
  P = DecodePlan{inc, has_act, kv_cache_mode, u};
  return 0;
}

// T: how many env steps the call took (vima_decode_chunk)
static void decode_commit(VimaHandle* h, const DecodePlan& P, int B, int Q, int Lp, int T = 1) {
  if (P.kv_mode == 1) { h->pkv.valid = true; h->pkv.B = B; h->pkv.Lp = Lp; }
  if (P.inc) {
    h->ep.book.commit(P.u, T);
    h->ep.live = true; h->ep.B = B; h->ep.Q = Q; h->ep.Lp = Lp; h->ep.Lmax = h->ep.book.Lmax;
  }
}

static int decode_launch(VimaHandle* h, const float* obs_tok, const uint8_t* obs_mask, const float* act_tok, int T, int B, int Q,
                         int L_act, const float* prompt, int64_t stride_b, int64_t stride_l, const uint8_t* prompt_mask, int Lp,
                         const DecodePlan& P, float* out, hipStream_t stream, bool hist = false) {
  // hist (vima_decode_restart_history): the full-history branch over the B = n_r flagged samples (h->restart_list) of a running episode batch. Their
  // prompt K / V are gathered from the handle's cache, every layer's self-attention K | V rows are scattered into the episode cache at
  // h->hist_rowmap, and the episode state is installed at the end; `prompt` / `prompt_mask` (the batch's) are indexed through the list
  if (int e = check_ready(h)) return e;
  const int E = h->cfg.embed_dim;
  const bool inc = P.inc;
  const int has_act = P.has_act, L_hist = P.u.row, Lq = P.u.Lq, Lmax = h->cfg.n_positions, kv_cache_mode = P.kv_mode;
  if (inc && !has_act) {   // step 0
    HIPCK(hipMemsetAsync(h->ep.poscnt, 0, (size_t)B * sizeof(int), stream));
    HIPCK(hipMemsetAsync(h->ep.fresh, 0, (size_t)B, stream));
  }
  Run R{h, (hipStream_t)stream};
  const int rq = B * Lq, rp = B * Lp;
  const int Hx = h->cfg.xattn_n_heads, Hs = h->cfg.sattn_n_heads;
  float* x32 = R.ws<float>((size_t)rq * E);
  void* xT = R.wsT((size_t)rq * E);
  uint8_t* dmask = R.ws<uint8_t>((size_t)rq);
  void* pT = R.wsT((size_t)rp * E);
  void* qn = R.wsT((size_t)rq * E);
  void* Qb = R.wsT((size_t)rq * E);
  // The prompt K/V projections (components.py:175) depend only on the prompt, not on the token stream: with dual_stream
  // they are all issued on the auxiliary stream up front (one buffer per layer) and overlap the serial decoder chain;
  // with kv_cache_mode 1/2 they live in a handle-owned cache that survives across calls (one episode = one prompt).
  const int NL = h->cfg.xf_n_layers;
  const bool use_cache = kv_cache_mode != 0 && !hist;
  const bool build_kv = kv_cache_mode != 2 && !hist;
  const size_t kv_layer_bytes = (size_t)rp * 2 * E * h->esz();
  const bool dual = h->dual_stream != 0 && build_kv;
  std::vector<void*> KVs(NL);
  if (use_cache) {
    for (int i = 0; i < NL; ++i) KVs[i] = reinterpret_cast<char*>(h->pkv.ptr) + kv_layer_bytes * i;
  } else {
    for (int i = 0; i < (dual ? NL : 1); ++i) KVs[i] = R.wsT((size_t)rp * 2 * E);
    if (!dual) for (int i = 1; i < NL; ++i) KVs[i] = KVs[0];
  }
  void* ctx = R.wsT((size_t)rq * E);
  float* a32 = R.ws<float>((size_t)rq * E);
  void* aT = R.wsT((size_t)rq * E);
  void* g = R.wsT((size_t)rq * 4 * E);
  void* u = R.wsT((size_t)rq * 4 * E);
  void* qkv = R.wsT((size_t)rq * 3 * E);
  float* n32 = R.ws<float>((size_t)rq * E);
  void* nT = R.wsT((size_t)rq * E);
  // option ln_fuse (bf16 weights): (1) ln_2 of layer i and XAttention's query pre-LN of layer i + 1 are one launch; (2) the pre-LN in front of
  // XAttention's feed-forward (components.py:220) disappears: attention_out's epilogue leaves per-32-column sums / sums of squares of the new stream
  // next to it and the feed-forward's GEGLU -- both products now read the UN-normed stream, so it is one launch at every size that has a pair form --
  // applies mean / rstd to the GELU'd factor in its epilogue (GemmArgs::sum_out / rs_sum / rs_c)
  const bool lnf = h->ln_fuse != 0 && h->bf16;
  const int ffold = (lnf && !h->w8 && h->dec[0].xl1g.W && h->dec[0].xl1_pair.W && !gemm_splitk_enabled(&h->tune) && gemm_lnfold_producer_ok(&h->tune, rq, E))
                        ? (gemm_dual_ok(&h->tune, rq, 4 * E) ? 1 : ((h->geglu_pair && gemm_pair_ok(&h->tune, rq, 4 * E, E)) ? 2 : 0))
                        : 0;
  float* st_sum = ffold ? R.ws<float>((size_t)rq * (E / 32)) : nullptr;
  float* st_ssq = ffold ? R.ws<float>((size_t)rq * (E / 32)) : nullptr;
  int* hlist = hist ? R.ws<int>((size_t)B) : nullptr;
  int* hmap = hist ? R.ws<int>((size_t)Lq) : nullptr;
  uint8_t* hpmask = hist ? R.ws<uint8_t>((size_t)rp) : nullptr;   // the flagged samples' rows of the prompt mask
  if (R.err) return R.err;
  if (hist) {
    if ((int)h->restart_list.size() != B || (int)h->hist_rowmap.size() != Lq) return fail("vima_decode_restart_history: internal row map mismatch");
    if (R.upload(hlist, h->restart_list) || R.upload(hmap, h->hist_rowmap)) return R.err;
    OTHER(R, launch_mask_rows_gather(prompt_mask, hpmask, hlist, B, Lp, R.st), "mask_rows_gather");
    prompt_mask = hpmask;
  }
  if (inc)   // T env steps (a step is a chunk of one): Lq = T (Q + 1) [- 1 at step 0] rows per sample at row L_hist
    OTHER(R, launch_dec_embed_chunk(obs_tok, obs_mask, act_tok, h->pos_emb, h->cfg.n_positions, x32, xT, h->ep.mask, h->ep.poscnt,
                                    L_hist, Lmax, T, B, Q, has_act, E, h->bf16, R.st, h->ep.fresh), "dec_embed_chunk");
  else
    OTHER(R, launch_dec_embed(obs_tok, obs_mask, act_tok, h->pos_emb, h->cfg.n_positions, x32, xT, dmask, T, B, Q, L_act, E,
                              h->bf16, R.st), "dec_embed");
  if (build_kv)
    OTHER(R, launch_prompt_pos(prompt, stride_b, stride_l, prompt_mask, h->xpos_emb, h->cfg.xattn_n_positions, pT, B, Lp, E,
                               h->bf16, R.st), "prompt_pos");
  // precision "fp8": the prompt K/V projections (M = B * Lp rows, the only large GEMMs of the decoder) take the prompt in fp8 e4m3 with
  // one calibrated scale when their shape fits the fp8 kernel; the first such call measures max |prompt + position embedding|
  void* p8 = nullptr;
  float kv_scale = 0.f;
  if (build_kv && h->a8 && h->bf16 && E % 256 == 0 && rp % 256 == 0 && (long long)(rp / 256) * (2 * E / 256) >= 160 && h->dec[0].kv.ws &&
      gemm_a8_ok(&h->tune, rp, 2 * E, E, E, E)) {
    Fp8Cal& c8 = h->cal8[CAL_KV];
    if (!c8.ready) {   // measure and freeze inside this call, which itself still runs on operand-type activations
      if (int e = cal_begin(h, c8, R.st)) return R.err = e;
      OTHER(R, launch_amax(pT, E, rp, E, c8.amax, R.st), "amax");
      if (int e = cal_freeze(h, c8, R.st)) return R.err = e;
    } else {
      kv_scale = c8.scale[0];
      p8 = R.ws<uint8_t>((size_t)rp * E);
      if (R.err) return R.err;
      OTHER(R, launch_quant_fp8(pT, E, rp, E, 1.0f / kv_scale, p8, E, R.st), "quant_fp8");
    }
  }
  // Layout of the per-layer prompt K / V: head-major [B][2 Hx][Lp][Dx] when the projection runs on the persistent 256x256 kernels (whose epilogue
  // can write it: GemmArgs::hm_D) -- the split-key cross attention then streams Lp x Dx contiguous elements per (batch, head) instead of 2 Dx-byte
  // slices of 4 E-byte rows (round 3 measured 86 against 104 us per layer at the benchmark shape); row-major [B * Lp][2E] otherwise. A cache keeps
  // the layout it was built with (h->pkv.hm); the values are the same, so is every result.
  const int Dx = E / Hx;
  bool hm = false;
  if (build_kv)
    hm = h->kv_headmajor && h->bf16 && gemm_headmajor_ok(&h->tune, rp, 2 * E, E, E, E, Dx, Lp, p8 != nullptr ? 1 : 0) != 0;
  else
    hm = hist ? false : h->pkv.hm;   // hist: gathered below, row-major
  if (use_cache && build_kv) h->pkv.hm = hm;
  auto kv_proj = [&](Run& Rr, int i, void* KV) {
    GemmArgs g = Rr.linear_args(Opnd{pT, E, p8, p8 ? kv_scale : 0.f}, h->dec[i].kv, 0, 2 * E, rp, ACT_NONE, nullptr, Opnd{KV, 2 * E});
    if (hm) { g.hm_D = Dx; g.hm_L = Lp; }
    return Rr.gemm(g);
  };
  if (dual) {
    while ((int)h->ev_layer.size() < NL) {
      hipEvent_t e;
      HIPCK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
      h->ev_layer.push_back(e);
    }
    if (fork_aux(R)) return 1;
    Run Rb{h, h->aux};
    for (int i = 0; i < NL; ++i) {
      kv_proj(Rb, i, KVs[i]);
      if (Rb.err) return Rb.err;
      HIPCK(hipEventRecord(h->ev_layer[i], h->aux));
    }
  }
  for (int i = 0; i < h->cfg.xf_n_layers; ++i) {
    auto& D = h->dec[i];
    void* KV = KVs[i];
    // ---- XAttention.forward (components.py:158-228)
    if (i == 0 || !lnf) R.ln(x32, E, D.xln_g, D.xln_b, 1e-5f, 0, rq, E, nullptr, qn);   // (else: written by the previous layer's ln_2 launch)
    R.linear(qn, E, D.q, rq, ACT_NONE, nullptr, 0, nullptr, 0, nullptr, 0, Qb, E);
    if (dual) HIPCK(hipStreamWaitEvent(R.st, h->ev_layer[i], 0));
    else if (build_kv)   // single stream: project right before use (without a cache all layers share one buffer)
      kv_proj(R, i, KV);
    else if (hist) {     // the flagged samples' blocks of the prompt K / V cache (either layout), which the restart in front of this pass has rebuilt
      KvRowsArgs c;
      c.in = kv_layer(h, i, Lp); c.out = KV; c.list = hlist; c.n = B; c.L = c.Lc = Lp; c.N = c.ld = 2 * E; c.D = h->pkv.hm ? Dx : 0; c.to_cache = false;
      OTHER(R, launch_kv_rows(c, (int)h->esz(), R.st), "kv_gather");
    }
    AttnArgs a;
    a.q = Qb; a.ldq = E; a.out = ctx; a.ldo = E;
    if (hm) {   // [B][2 Hx][Lp][Dx]: K heads 0 .. Hx-1, V heads Hx .. 2 Hx-1
      a.k = KV; a.v = R.offT(KV, (long long)E * Lp); a.ldk = a.ldv = Dx; a.k_hs = a.v_hs = Lp * Dx; a.k_bs = a.v_bs = (long long)2 * E * Lp;
    } else {
      a.k = KV; a.ldk = 2 * E; a.v = R.offT(KV, E); a.ldv = 2 * E;
    }
    a.kmask = prompt_mask; a.B = B; a.H = Hx; a.Lq = Lq; a.Lk = Lp; a.D = E / Hx;
    a.scale = 1.0f / sqrtf((float)(E / Hx)); a.mode = ATTN_CROSS;
    R.attn(a, h->attn_impl);
    if (ffold) {
      GemmArgs ga;   // a = x + ctx Wo^T -> a32 / aT, + the LayerNorm partials of a32
      ga.A = ctx; ga.lda = E; R.setW(ga, D.ao); ga.M = rq; ga.N = E; ga.K = E; ga.res = x32; ga.ldres = E; ga.out32 = a32; ga.ld32 = E; ga.outT = aT; ga.ldT = E;
      ga.ssq_out = st_ssq; ga.sum_out = st_sum;
      R.gemm(ga);
      GemmArgs gf;   // u = gelu(LN(a) W1^T) * bf16(a Wg^T), LN folded: both products read aT
      gf.A = aT; gf.lda = E; gf.M = rq; gf.K = E; gf.act = ACT_GELU; gf.outT = u; gf.ldT = 4 * E;
      gf.rs_ssq = st_ssq; gf.rs_sum = st_sum; gf.rs_parts = E / 32; gf.rs_invk = 1.0f / (float)E; gf.rs_eps = 1e-5f;
      if (ffold == 1) { R.setW(gf, D.xl1g); gf.N = 4 * E; gf.bias = D.xl1g.b; gf.rs_c = D.xl1g.c; gf.A2 = aT; gf.lda2 = E; gf.W2 = D.gate.W; gf.ldw2 = E; }
      else { R.setW(gf, D.xl1_pair); gf.N = 8 * E; gf.bias = D.xl1_pair.b; gf.rs_c = D.xl1_pair.c; gf.pair32 = 1; }
      R.gemm(gf);
    } else {
    R.linear(ctx, E, D.ao, rq, ACT_NONE, nullptr, 0, x32, E, a32, E, aT, E);            // + q residual
    R.ln(a32, E, D.xln2_g, D.xln2_b, 1e-5f, 0, rq, E, nullptr, qn);
    R.geglu(qn, D.l1, aT, D.gate, rq, g, u);                                              // gate reads the UN-normed stream
    }
    R.linear(u, 4 * E, D.l2, rq, ACT_NONE, nullptr, 0, a32, E, x32, E, xT, E);
    // ---- Block.forward (components.py:23-37), post-LN
    AttnArgs s;
    s.out = ctx; s.ldo = E; s.B = B; s.H = Hs; s.Lq = Lq; s.D = E / Hs;
    s.scale = 1.0f / sqrtf((float)(E / Hs)); s.mode = ATTN_CAUSAL;
    if (inc) {
      // q of the new tokens, their k | v rows appended to the layer's episode cache at rows [L_hist, L_hist + Lq); history + themselves are the keys
      void* cache = ep_layer(h, i);
      c_attn_append(R, D.c_attn, xT, rq, Lq, L_hist, Lmax, cache, qkv);
      attn_from_cache(R, s, qkv, cache, L_hist, Lmax, P.u.Lk, P.u.win_end);
    } else {
      R.linear(xT, E, D.c_attn, rq, ACT_NONE, nullptr, 0, nullptr, 0, nullptr, 0, qkv, 3 * E);
      s.q = qkv; s.ldq = 3 * E; s.k = R.offT(qkv, E); s.ldk = 3 * E; s.v = R.offT(qkv, 2 * E); s.ldv = 3 * E;
      s.kmask = dmask; s.Lk = Lq;
      if (hist) {   // the history's K | V rows of this layer -> the episode cache, at the rows the batch steps behind them wrote
        KvRowsArgs c;
        c.in = R.offT(qkv, E); c.ld = 3 * E; c.out = ep_layer(h, i); c.list = hlist; c.rowmap = hmap; c.n = B; c.L = Lq; c.N = 2 * E; c.Lc = Lmax;
        OTHER(R, launch_kv_rows(c, (int)h->esz(), R.st), "kv_scatter_rows");
      }
    }
    R.attn(s, h->attn_impl);
    R.linear(ctx, E, D.c_proj, rq, ACT_NONE, nullptr, 0, x32, E, a32, E, nullptr, 0);   // x + a
    R.ln(a32, E, D.ln1_g, D.ln1_b, 1e-5f, 0, rq, E, n32, nT);                           // n = ln_1(x + a)
    R.geglu(nT, D.fc, nT, D.mgate, rq, g, u, &D.fc_pair);
    R.linear(u, 4 * E, D.mproj, rq, ACT_NONE, nullptr, 0, n32, E, a32, E, nullptr, 0);  // n + m
    if (lnf && i + 1 < h->cfg.xf_n_layers) {                                             // h = ln_2(n + m) and the next layer's query pre-LN of h
      auto& Dn = h->dec[i + 1];
      OTHER(R, launch_layernorm2(a32, E, D.ln2_g, D.ln2_b, 1e-5f, Dn.xln_g, Dn.xln_b, 1e-5f, rq, E, x32, xT, qn, h->bf16, R.st), "layernorm2");
    } else {
      R.ln(a32, E, D.ln2_g, D.ln2_b, 1e-5f, 0, rq, E, x32, xT);                         // h = ln_2(n + m)
    }
    if (R.err) return R.err;
  }
  if (inc) OTHER(R, launch_gather_pred(x32, out, T, B, Q, Lq, E, R.st, has_act), "gather_pred");   // the last obs row of every slot (T = 1: row Lq - 1)
  else if (out) OTHER(R, launch_gather_pred(x32, out, T, B, Q, Lq, E, R.st), "gather_pred");
  if (hist)   // lo = hi = 0: the restart in front of this pass has cleared the samples' mask rows
    OTHER(R, launch_history_install(dmask, hlist, hmap, B, Lq, 0, 0, Lmax, h->ep.mask, h->ep.poscnt, h->ep.fresh, R.st), "history_install");
  if (dual && join_aux(R)) return 1;
  return R.err;
}

int vima_decode(VimaHandle* h, const float* obs_tok, const uint8_t* obs_mask, const float* act_tok, int T, int B, int Q,
                int L_act, const float* prompt, int64_t stride_b, int64_t stride_l, const uint8_t* prompt_mask, int Lp,
                int kv_cache_mode, float* out, vima_stream_t stream) {
  DecodePlan P;
  if (int e = decode_prepare(h, act_tok, T, B, Q, L_act, Lp, kv_cache_mode, -1, P)) return e;
  const std::string key = gkey("decode", {(long long)(uintptr_t)obs_tok, (long long)(uintptr_t)obs_mask, (long long)(uintptr_t)act_tok, T, B, Q,
                                          L_act, (long long)(uintptr_t)prompt, stride_b, stride_l, (long long)(uintptr_t)prompt_mask, Lp,
                                          P.kv_mode, (long long)(uintptr_t)out, (long long)(uintptr_t)h->pkv.ptr});
  const int rc = run_graphed(h, key, (hipStream_t)stream, [&](hipStream_t st) {
    return decode_launch(h, obs_tok, obs_mask, act_tok, T, B, Q, L_act, prompt, stride_b, stride_l, prompt_mask, Lp, P, out, st);
  });
  if (!rc) decode_commit(h, P, B, Q, Lp);
  return rc;
}

// vima_decode_step (T = 1) and vima_decode_chunk
static int decode_unit(VimaHandle* h, const float* obs_tok, const uint8_t* obs_mask, const float* act_tok, int step, int T, int B, int Q,
                       const float* prompt, int64_t stride_b, int64_t stride_l, const uint8_t* prompt_mask, int Lp, float* out, hipStream_t stream) {
  DecodePlan P;
  if (int e = decode_prepare(h, act_tok, T, B, Q, 0, Lp, 0, step, P)) return e;
  const EpisodeBook& bk = h->ep.book;
  std::string key, warm;
  if (T == 1) {
    const long long kstep = bk.ring ? -1 - (((long long)P.u.row * (bk.Lmax + 1) + P.u.Lk) * 2 + P.has_act) : step;
    key = gkey("decode_step", {(long long)(uintptr_t)obs_tok, (long long)(uintptr_t)obs_mask, (long long)(uintptr_t)act_tok, kstep, B, Q,
                               (long long)(uintptr_t)prompt, stride_b, stride_l, (long long)(uintptr_t)prompt_mask, Lp, (long long)(uintptr_t)out,
                               (long long)(uintptr_t)h->pkv.ptr, (long long)(uintptr_t)h->ep.kv});
    if (bk.ring && P.has_act) warm = gkey("decode_step_ring", {B, Q, Lp, P.u.Lk >= 64 ? 1 : 0});
  }
  return episode_unit(h, T, stream, key, warm, [&](hipStream_t st) {
    return decode_launch(h, obs_tok, obs_mask, act_tok, T, B, Q, 0, prompt, stride_b, stride_l, prompt_mask, Lp, P, out, st);
  }, [&] { decode_commit(h, P, B, Q, Lp, T); });
}

int vima_decode_step(VimaHandle* h, const float* obs_tok, const uint8_t* obs_mask, const float* act_tok, int step, int B, int Q,
                     const float* prompt, int64_t stride_b, int64_t stride_l, const uint8_t* prompt_mask, int Lp, float* out,
                     vima_stream_t stream) {
  if (step < 0) return fail("vima_decode_step: step must be >= 0");
  return decode_unit(h, obs_tok, obs_mask, act_tok, step, 1, B, Q, prompt, stride_b, stride_l, prompt_mask, Lp, out, (hipStream_t)stream);
}

int vima_decode_chunk(VimaHandle* h, const float* obs_tok, const uint8_t* obs_mask, const float* act_tok, int step, int T, int B, int Q,
                      const float* prompt, int64_t stride_b, int64_t stride_l, const uint8_t* prompt_mask, int Lp, float* out,
                      vima_stream_t stream) {
  if (step < 0 || T < 1) return fail("vima_decode_chunk: step must be >= 0 and T >= 1");
  return decode_unit(h, obs_tok, obs_mask, act_tok, step, T, B, Q, prompt, stride_b, stride_l, prompt_mask, Lp, out, (hipStream_t)stream);
}

// What vima_seq_decode_restart and the two *_restart_history entries share in front of their launches (vima_decode_restart keeps its own
// prologue, the one text the clock was held against; profiles/episode_entry_time.txt): the null-argument refusal, the running-batch check (family: ep_running) and
// the flagged samples (restart: HOST array [B]). None flagged: the entry returns 0 with nothing launched and nothing uploaded; an entry that goes
// on to launch moves the list into h->restart_list, the source of its R.upload and of its closing book.restart / install -- a refused call
// leaves the handle as it was
static int restart_begin(const VimaHandle* h, const char* fn, bool seq, bool null_arg, const uint8_t* restart, int B, int Lp, const char* family,
                         std::vector<int>& flagged) {
  if (null_arg) return fail(std::string(fn) + ": null argument");
  if (int e = ep_running(h, fn, seq, B, Lp, !seq, " with this B / Lp", family)) return e;
  flagged = flagged_list(restart, B);
  return 0;
}

// vima_decode_history_room / vima_seq_history_room behind their preambles
static int history_room(VimaHandle* h, const char* fn, bool seq, int32_t* steps_host, const char* family) {
  if (!steps_host) return fail(std::string(fn) + ": null argument");
  if (int e = ep_running(h, fn, seq, kAny, kAny, false, "", family)) return e;
  *steps_host = h->ep.book.room();
  return 0;
}

// Per-sample episode restart inside a running batch of incremental decoding (batched environments whose episodes end at different
// steps; scripts/example.py:97-110 starts a new episode with a new prompt). For every sample with restart[b] != 0 (HOST array): its
// cached history is masked out (the caches keep ONE row index space for the batch: the next step's tokens of all samples still land
// at the same cache rows), its position counter restarts at 0, its next step carries no previous action, and its rows of the per-layer
// prompt K/V cache are rebuilt from its row of `prompt` (the NEW prompts; rows of the other samples are not read). The batch keeps
// stepping with vima_decode_step(step + 1, ...); n_positions bounds the number of steps since the last step 0 of the whole batch -- unless the
// row index space is a ring (option decode_ring), where a restart gives the sample's rows back (EpisodeBook::restart).
// The prompt K / V rows of ALL flagged samples are rebuilt together (option restart_batched, prompts longer than 32 tokens): one gather of their
// prompts + positions into [n_r * Lp, E], per layer one GEMM of n_r * Lp rows and one scatter into the cache (either layout) -- 1 + 2 NL launches
// whatever n_r is, against n_r (1 + NL .. 2 NL) for the per-sample loop. The tile GEMM kernels agree bit for bit at every row count (option
// gemm_skinny in the header), so the cache holds the loop's bits; at Lp <= 32 the loop's GEMMs run on gemm_skinny_kernel, whose summation order
// differs, and the loop is kept. In precision fp8 this GEMM takes bf16 activations whatever its size (header, VIMA_PRECISION_FP8 (iv)).
int vima_decode_restart(VimaHandle* h, const uint8_t* restart, int B, const float* prompt, int64_t stride_b, int64_t stride_l,
                        const uint8_t* prompt_mask, int Lp, vima_stream_t stream) {
  if (int e = check_ready(h)) return e;
  if (!restart || !prompt || !prompt_mask) return fail("vima_decode_restart: null argument");
  if (!(h->ep.live && !ep_seq(h) && h->ep.B == B && h->ep.Lp == Lp && h->pkv.valid && h->pkv.B == B && h->pkv.Lp == Lp))
    return fail("vima_decode_restart: no running episode batch with this B / Lp (start one with vima_decode_step(step = 0))");
  const int E = h->cfg.embed_dim, NL = h->cfg.xf_n_layers;
  Run R{h, (hipStream_t)stream};
  h->restart_list = flagged_list(restart, B);
  const int n_r = (int)h->restart_list.size();
  if (n_r == 0) return 0;   // nothing flagged: nothing to launch
  const bool batched = h->restart_batched != 0 && Lp > 32;
  const int n_ws = batched ? n_r : 1;
  int* list = R.ws<int>((size_t)n_r);
  void* pT = R.wsT((size_t)n_ws * Lp * E);
  void* kvrow = (h->pkv.hm || batched) ? R.wsT((size_t)n_ws * Lp * 2 * E) : nullptr;   // row-major K | V before the scatter / the head-major transposition
  if (R.upload(list, h->restart_list)) return R.err;
  OTHER(R, launch_episode_restart(list, n_r, h->ep.mask, h->ep.poscnt, h->ep.fresh, 0, h->ep.Lmax, h->ep.Lmax, R.st), "restart_samples");
  KvRowsArgs c;   // row-major K | V rows of kvrow -> the samples' blocks of a layer of the prompt K / V cache, in the cache's layout
  c.in = kvrow; c.L = c.Lc = Lp; c.N = c.ld = 2 * E; c.D = h->pkv.hm ? E / h->cfg.xattn_n_heads : 0;
  if (batched) {
    OTHER(R, launch_prompt_pos(prompt, stride_b, stride_l, prompt_mask, h->xpos_emb, h->cfg.xattn_n_positions, pT, n_r, Lp, E, h->bf16, R.st, list),
          "prompt_pos");
    for (int i = 0; i < NL && !R.err; ++i) {
      R.linear(pT, E, h->dec[i].kv, n_r * Lp, ACT_NONE, nullptr, 0, nullptr, 0, nullptr, 0, kvrow, 2 * E);
      c.out = kv_layer(h, i, Lp); c.list = list; c.n = n_r;
      OTHER(R, launch_kv_rows(c, (int)h->esz(), R.st), "kv_scatter");
    }
  }
  for (int b = 0; b < B && !R.err && !batched; ++b) {
    if (!restart[b]) continue;
    OTHER(R, launch_prompt_pos(prompt + (long long)b * stride_b, stride_b, stride_l, prompt_mask + (long long)b * Lp, h->xpos_emb,
                               h->cfg.xattn_n_positions, pT, 1, Lp, E, h->bf16, R.st), "prompt_pos");
    for (int i = 0; i < NL; ++i) {
      void* KV = R.offT(kv_layer(h, i, Lp), (long long)b * Lp * 2 * E);
      if (!h->pkv.hm) {
        R.linear(pT, E, h->dec[i].kv, Lp, ACT_NONE, nullptr, 0, nullptr, 0, nullptr, 0, KV, 2 * E);
      } else {   // head-major cache: the sample's block is [2 Hx][Lp][Dx]; Lp rows are too few for the kernel that writes it directly
        R.linear(pT, E, h->dec[i].kv, Lp, ACT_NONE, nullptr, 0, nullptr, 0, nullptr, 0, kvrow, 2 * E);
        c.out = KV; c.n = 1;
        OTHER(R, launch_kv_rows(c, (int)h->esz(), R.st), "rows_to_headmajor");
      }
    }
  }
  if (!R.err) h->ep.book.restart(h->restart_list);
  return R.err;
}

int vima_decode_history_room(VimaHandle* h, int32_t* steps_host) {   // host only: the device is not touched
  if (!h) return fail("vima_decode_history_room: null argument");
  return history_room(h, "vima_decode_history_room", false, steps_host, "the handle's policy has no XAttnGPT episode caches");
}

// vima_decode_restart with a history: the restart itself (same code, same bits), then the T env steps of history of the n_r flagged samples as ONE
// full-history pass over [n_r, T (Q + 1) - 1] rows (decode_launch, hist): plain causal attention under the history's own mask against the prompt K / V
// the restart has just rebuilt, every layer's K | V rows scattered to the cache rows that batch steps t - T .. t - 1 wrote, then the key mask, position
// counter and restart flag. The launches of one vima_decode pass plus 2 + 2 x layers on top of the restart's, whatever n_r. Host: the samples' ring
// age becomes that of a sample restarted right before batch step t - T.
int vima_decode_restart_history(VimaHandle* h, const uint8_t* restart, int B, const float* prompt, int64_t stride_b, int64_t stride_l,
                                const uint8_t* prompt_mask, int Lp, const float* hist_obs, const uint8_t* hist_mask, const float* hist_act, int T,
                                float* out, vima_stream_t stream) {
  if (T == 0) return vima_decode_restart(h, restart, B, prompt, stride_b, stride_l, prompt_mask, Lp, stream);
  const char* fn = "vima_decode_restart_history";
  std::vector<int> flagged;
  if (!h) return fail("null handle");
  if (T < 0) return fail("vima_decode_restart_history: T must be >= 0");
  if (int e = restart_begin(h, fn, false, !restart || !prompt || !prompt_mask || !hist_obs || !hist_mask || (T > 1 && !hist_act), restart, B, Lp,
                            "the handle's policy has no XAttnGPT episode caches", flagged))
    return e;
  // history step s sits in the slot of batch step t - T + s: its Q obs rows in the slot's obs rows, a_{s-1} in its action row (s > 0; the first
  // slot's action row stays masked). Compact rows (dec_embed_kernel): [o_0 (Q), a_0, o_1 (Q), a_1, ...]
  EpisodeBook::History H = h->ep.book.history(T, false);
  if (!H.fits) return room_refused(std::string(fn) + ": a history of " + std::to_string(T) + " steps", H.room);
  const int Q = h->ep.Q, Lmax = h->ep.Lmax;
  const long long Lh = (long long)T * (Q + 1) - 1;
  if (Lh > 512 || Lh > Lmax) return fail("vima_decode_restart_history: a history holds at most min(512, n_positions) rows");
  if (!H.in_range) return fail("vima_decode_restart_history: internal error: history row outside the written cache");
  if (int e = vima_decode_restart(h, restart, B, prompt, stride_b, stride_l, prompt_mask, Lp, stream)) return e;
  if (flagged.empty()) return 0;
  const int n_r = (int)flagged.size();   // (the restart has put the list into h->restart_list)
  h->hist_rowmap = std::move(H.rows);
  DecodePlan P{false, 0, 0, {}};
  P.u.Lq = (int)Lh;
  const int rc = decode_launch(h, hist_obs, hist_mask, hist_act, T, n_r, Q, T - 1, prompt, stride_b, stride_l, prompt_mask, Lp, P, out,
                               (hipStream_t)stream, true);
  if (!rc) h->ep.book.install(h->restart_list, H.age);
  return rc;
}

// Host-only: how many further vima_decode_step / vima_seq_decode_step calls would succeed if sample b alone were never restarted (EpisodeBook::steps_left).
int vima_decode_steps_left(VimaHandle* h, int B, int32_t* out_host) {
  if (!h || !out_host) return fail("vima_decode_steps_left: null argument");
  if (int e = ep_running(h, "vima_decode_steps_left", ep_seq(h), B, kAny, false, " of this size")) return e;   // either family's episode
  for (int b = 0; b < B; ++b) out_host[b] = h->ep.book.steps_left(b);
  return 0;
}

// ---- baseline policies --------------------------------------------------------------------------
int vima_rgb_tokens_per_image(const VimaConfig* cfg) {
  if (!cfg || cfg->policy_kind == VIMA_POLICY_VIMA) return 0;
  return rgb_tokens_per_image(cfg->policy_kind);
}

int vima_rgb_encode(VimaHandle* h, const uint8_t* const rgb[2], int n, float* out, vima_stream_t stream) {
  if (int e = baseline_ready(h, "vima_rgb_encode")) return e;
  Run R{h, (hipStream_t)stream};
  return rgb_obj_encode(R, rgb, n, out, nullptr);
}

int vima_rgb_obs_encode(VimaHandle* h, const uint8_t* const rgb[2], const int64_t* ee, int n, float* out, vima_stream_t stream) {
  if (int e = baseline_ready(h, "vima_rgb_obs_encode")) return e;
  if (n <= 0) return 0;
  Run R{h, (hipStream_t)stream};
  const int E = h->cfg.embed_dim, Q = rgb_tokens_per_image(h->cfg.policy_kind);
  const int Kf = h->fuse.K;            // 2E (GPT: one row per frame pair) or E (one row per token)
  const int rows = n * Q;
  void* featT = R.wsT((size_t)rows * Kf);
  if (R.err) return R.err;
  if (rgb_obj_encode(R, rgb, n, nullptr, featT)) return R.err;
  // obs_fusion_layer on cat(img_feats, ee_feats) (vima_gpt_policy.py:256-258; the ee feature repeated over the Q tokens,
  // vima_gato_policy.py:261-263): W[:, :Kf] . feats + (W[:, Kf:] . ee_emb[ee] + b)
  R.linear(featT, Kf, h->fuse, rows, ACT_NONE, nullptr, 0, nullptr, 0, out, E, nullptr, 0);
  OTHER(R, launch_add_row_table(out, rows, E, h->ee_table, (const long long*)ee, Q, R.st), "ee_table");
  return R.err;
}

int vima_rgb_prompt_encode(VimaHandle* h, const int64_t* word_ids, int n_words, const uint8_t* const rgb[2], int n_img,
                           const int32_t* tok_src, int B, int Lp, float* out_tokens, uint8_t* out_mask, vima_stream_t stream) {
  if (int e = baseline_ready(h, "vima_rgb_prompt_encode")) return e;
  (void)n_words;
  Run R{h, (hipStream_t)stream};
  const int E = h->cfg.embed_dim, Q = rgb_tokens_per_image(h->cfg.policy_kind);
  const int Kf = h->fuse.K;
  const int orows = n_img * Q;
  float* objtok = R.ws<float>((size_t)(orows > 0 ? orows : 1) * 768);
  uint8_t* objmask = R.ws<uint8_t>((size_t)(orows > 0 ? orows : 1));
  if (R.err) return R.err;
  if (orows > 0) {
    void* featT = R.wsT((size_t)orows * Kf);
    void* p1 = R.wsT((size_t)orows * 768);
    void* p2 = R.wsT((size_t)orows * 768);
    if (R.err) return R.err;
    if (rgb_obj_encode(R, rgb, n_img, nullptr, featT)) return R.err;
    // prompt_obj_post_layer (vima_gpt_policy.py:207)
    R.linear(featT, Kf, h->pobj[0], orows, ACT_RELU, nullptr, 0, nullptr, 0, nullptr, 0, p1, 768);
    R.linear(p1, 768, h->pobj[1], orows, ACT_RELU, nullptr, 0, nullptr, 0, nullptr, 0, p2, 768);
    R.linear(p2, 768, h->pobj[2], orows, ACT_NONE, nullptr, 0, nullptr, 0, objtok, 768, nullptr, 0);
    OTHER(R, launch_fill_u8(objmask, orows, 1, R.st), "fill");   // no object masks in these policies: every image token is valid
  }
  const int rows = B * Lp;
  float* x = R.ws<float>((size_t)rows * 768);
  if (R.err) return R.err;
  OTHER(R, launch_prompt_assemble(tok_src, (const long long*)word_ids, h->word_table, objtok, objmask, x, out_mask, rows, 768, R.st),
        "prompt_assemble");
  if (!h->has_t5_post) return t5_stack(R, x, out_mask, B, Lp, out_tokens, nullptr);
  void* yT = R.wsT((size_t)rows * 768);
  if (R.err) return R.err;
  if (t5_stack(R, x, out_mask, B, Lp, nullptr, yT)) return R.err;
  return R.linear(yT, 768, h->t5_post, rows, ACT_NONE, nullptr, 0, nullptr, 0, out_tokens, E, nullptr, 0);
}

int vima_seq_decode(VimaHandle* h, const float* obs_tok, const float* act_tok, int T, int B, int L_act, const float* prompt,
                    int64_t stride_b, int64_t stride_l, const uint8_t* prompt_mask, int Lp, float* out, vima_stream_t stream) {
  if (int e = baseline_ready(h, "vima_seq_decode")) return e;
  if (h->cfg.policy_kind == VIMA_POLICY_FLAMINGO)
    return fail("vima_seq_decode: VIMAFlamingoPolicy decodes with XAttnGPT (vima_decode with an all-ones obs_mask)");
  const int E = h->cfg.embed_dim, Q = rgb_tokens_per_image(h->cfg.policy_kind);
  if (T <= 0 || B <= 0 || Lp <= 0) return fail("vima_seq_decode: empty input");
  if (L_act < 0 || L_act > T || (L_act > 0 && !act_tok) || L_act < T - 1) return fail("vima_seq_decode: L_act must be T-1 or T");
  const int L = Lp + 1 + T * Q + L_act;
  // The bound is on the PADDED length L, like the reference's: its position ids only reach max_b(valid prompt tokens) + 1 + T*Q +
  // L_act - 1 (vima_gato_policy.py:156-184), but the causal-mask buffer of the HF OpenAI-GPT attention is [n_positions, n_positions]
  // and is cropped to it (`b = self.bias[:, :, : w.size(-2), : w.size(-1)]`; `w * b` then fails to broadcast for L > n_positions),
  // so a padded batch longer than the table does not run there either. One deviation is deliberate: a sample whose prompt mask is
  // ALL false gets position id 0 for its padding (seq_embed_kernel clamps), where the reference's embedding lookup raises
  // IndexError for the id -1 it builds (torch.arange(0) ++ fill_(n_valids - 1)); the mask lives on the device and this call is
  // asynchronous, so the host mirror (vima_amd/baselines.py) is the place that can refuse such a batch before calling.
  if (L > h->cfg.n_positions)   // (also the positions_embed lookup beyond the table, gpt/gpt.py:177-185)
    return fail("vima_seq_decode: sequence of " + std::to_string(L) + " tokens exceeds n_positions " + std::to_string(h->cfg.n_positions), 34);
  Run R{h, (hipStream_t)stream};
  const int rq = B * L;
  float* x32 = R.ws<float>((size_t)rq * E);
  void* xT = R.wsT((size_t)rq * E);
  uint8_t* mask = R.ws<uint8_t>((size_t)rq);
  if (R.err) return R.err;
  OTHER(R, launch_seq_embed(prompt, stride_b, stride_l, prompt_mask, h->sep_token, obs_tok, act_tok, h->pos_emb, h->cfg.n_positions, x32,
                            xT, mask, B, L, Lp, Q, E, h->bf16, R.st), "seq_embed");
  if (hfgpt_stack(R, x32, xT, mask, B, L)) return R.err;
  // predicted = tokens_out[Lp + 1 + Q - 1 :: Q + 1] (vima_gato_policy.py:185-187)
  OTHER(R, launch_gather_pred(x32 + (size_t)(Lp + 1) * E, out, T, B, Q, L, E, R.st), "gather_pred");
  return R.err;
}

// ---- incremental decoding of the decoder-only policies ------------------------------------------------------------------------------
// HFGPT blocks are post-LN and act per row, the attention is causal (future keys get -1e4 in the reference: exp underflows to 0 in fp32), so
// the K | V of a prefix are final once computed: the prompt rows run through the stack once (vima_seq_prefill), every env step feeds only its
// own rows against the per-layer episode cache (vima_seq_decode_step) and equals the same rows of vima_seq_decode on the whole history.
static int seq_ready(VimaHandle* h, const char* fn) {
  if (int e = baseline_ready(h, fn)) return e;
  if (h->cfg.policy_kind != VIMA_POLICY_GPT && h->cfg.policy_kind != VIMA_POLICY_GATO)
    return fail(std::string(fn) + ": decoder-only policies (GPT / GATO) only; VIMAFlamingoPolicy steps with vima_decode_step");
  if (h->decode_ring) return fail(std::string(fn) + ": option decode_ring is not available for the decoder-only policies (set it to 0)");
  return 0;
}

int vima_seq_prefill(VimaHandle* h, const float* prompt, int64_t stride_b, int64_t stride_l, const uint8_t* prompt_mask, int B, int Lp,
                     vima_stream_t stream) {
  if (int e = seq_ready(h, "vima_seq_prefill")) return e;
  if (!prompt || !prompt_mask) return fail("vima_seq_prefill: null argument");
  if (B <= 0 || Lp <= 0) return fail("vima_seq_prefill: empty input");
  const int E = h->cfg.embed_dim, Lmax = h->cfg.n_positions, L = Lp + 1;
  if (L > Lmax)
    return fail("vima_seq_prefill: prompt of " + std::to_string(Lp) + " tokens + separator exceeds n_positions " + std::to_string(Lmax), 34);
  h->ep.live = false;   // from here on the caches belong to the new episode
  if (int e = ep_reserve(h, B, Lmax)) return e;
  Run R{h, (hipStream_t)stream};
  float* x32 = R.ws<float>((size_t)B * L * E);
  void* xT = R.wsT((size_t)B * L * E);
  uint8_t* mask = R.ws<uint8_t>((size_t)B * L);
  if (R.err) return R.err;
  HIPCK(hipMemsetAsync(h->ep.fresh, 0, (size_t)B, R.st));
  h->ep.B = B; h->ep.Q = rgb_tokens_per_image(h->cfg.policy_kind); h->ep.Lp = Lp; h->ep.Lmax = Lmax;   // (ep_layer reads the caches' shape)
  OTHER(R, launch_seq_embed(prompt, stride_b, stride_l, prompt_mask, h->sep_token, nullptr, nullptr, h->pos_emb, Lmax, x32, xT, mask, B, L, Lp, h->ep.Q,
                            E, h->bf16, R.st, nullptr, h->ep.mask, h->ep.poscnt, Lmax), "seq_embed_prefill");
  if (hfgpt_stack(R, x32, xT, mask, B, L, true)) return R.err;
  h->ep.live = true;
  h->ep.book.begin(B, h->ep.Q, L, Lmax, h->seq_ring != 0);   // the fixed prefix: prompt + separator
  return 0;
}

// One unit of T env steps (plan P): embed its rows, the blocks against the episode cache, the last obs row of every slot (T = 1: the last new row)
static int seq_step_launch(VimaHandle* h, const float* obs_tok, const float* act_tok, int T, int B, int Q, int has_act, const EpisodeBook::Plan& P,
                           float* out, hipStream_t stream) {
  if (int e = check_ready(h)) return e;
  const int E = h->cfg.embed_dim, Lmax = h->ep.Lmax, Lq = P.Lq;
  Run R{h, stream};
  float* x32 = R.ws<float>((size_t)B * Lq * E);
  void* xT = R.wsT((size_t)B * Lq * E);
  if (R.err) return R.err;
  OTHER(R, launch_seq_embed_chunk(obs_tok, act_tok, h->pos_emb, Lmax, x32, xT, h->ep.mask, h->ep.poscnt, h->ep.fresh, P.row, T, B, Q, has_act, E, h->bf16,
                                  R.st), "seq_embed_chunk");
  if (hfgpt_step_stack(R, x32, xT, B, Lq, P.row, Lmax, P.Lk, P.win_end)) return R.err;
  OTHER(R, launch_gather_pred(x32, out, T, B, Q, Lq, E, R.st, has_act), "gather_pred");
  return R.err;
}

// vima_seq_decode_step (T = 1) and vima_seq_decode_chunk: validation, the continuity check and the plan -- host only, nothing changes
static int seq_prepare(VimaHandle* h, const char* fn, const float* obs_tok, const float* act_tok, int step, int T, int B, const float* out,
                       EpisodeBook::Plan& P) {
  if (int e = seq_ready(h, fn)) return e;
  if (!obs_tok || !out) return fail(std::string(fn) + ": null argument");
  if (step < 0 || T < 1 || B <= 0) return fail(std::string(fn) + ": step must be >= 0, T >= 1 and B > 0");
  if (!(h->ep.live && h->ep.book.next == step && h->ep.B == B))
    return fail(std::string(fn) + ": step " + std::to_string(step) + " of " + std::to_string(B) + " samples does not continue the episode state (" +
                (h->ep.live ? "next step " + std::to_string(h->ep.book.next) + " of " + std::to_string(h->ep.B) + " samples" : std::string("no episode")) +
                "); start an episode with vima_seq_prefill");
  if ((step > 0 || T > 1) && !act_tok)
    return fail(std::string(fn) + ": the action tokens are required (the previous action for step > 0, those between a chunk's steps)");
  P = h->ep.book.plan(T);
  return P.refused ? plan_refused(fn, "vima_seq_decode_restart", h->ep.book, P, T) : 0;
}

// vima_seq_decode_step (T = 1) and vima_seq_decode_chunk
static int seq_unit(VimaHandle* h, const char* fn, const float* obs_tok, const float* act_tok, int step, int T, int B, float* out, hipStream_t stream) {
  EpisodeBook::Plan P;
  if (int e = seq_prepare(h, fn, obs_tok, act_tok, step, T, B, out, P)) return e;
  const int has_act = step > 0 ? 1 : 0, Q = h->ep.Q;
  std::string key, warm;
  if (T == 1) {
    key = gkey("seq_step", {(long long)(uintptr_t)obs_tok, (long long)(uintptr_t)act_tok, (long long)(uintptr_t)out, B, P.row, has_act,
                            (long long)(uintptr_t)h->ep.kv, P.Lk, P.win_end});
    if (h->ep.book.ring && has_act) warm = gkey("seq_step_ring", {B, P.Lk >= 64 ? 1 : 0});
  }
  return episode_unit(h, T, stream, key, warm, [&](hipStream_t st) {
    return seq_step_launch(h, obs_tok, has_act || T > 1 ? act_tok : nullptr, T, B, Q, has_act, P, out, st);
  }, [&] { h->ep.book.commit(P, T); });
}

int vima_seq_decode_step(VimaHandle* h, const float* obs_tok, const float* act_tok, int step, int B, float* out, vima_stream_t stream) {
  return seq_unit(h, "vima_seq_decode_step", obs_tok, act_tok, step, 1, B, out, (hipStream_t)stream);
}

int vima_seq_decode_chunk(VimaHandle* h, const float* obs_tok, const float* act_tok, int step, int T, int B, float* out, vima_stream_t stream) {
  return seq_unit(h, T == 1 ? "vima_seq_decode_step" : "vima_seq_decode_chunk", obs_tok, act_tok, step, T, B, out, (hipStream_t)stream);
}

// All flagged samples are rebuilt TOGETHER: one compact prefill of n_flagged x (Lp + 1) rows through the stack, whose k | v copy per layer
// scatters by the sample list -- 2 + launches of one stack pass, whatever the number of flagged samples.
int vima_seq_decode_restart(VimaHandle* h, const uint8_t* restart, int B, const float* prompt, int64_t stride_b, int64_t stride_l,
                            const uint8_t* prompt_mask, int Lp, vima_stream_t stream) {
  std::vector<int> flagged;
  if (int e = seq_ready(h, "vima_seq_decode_restart")) return e;
  if (int e = restart_begin(h, "vima_seq_decode_restart", true, !restart || !prompt || !prompt_mask, restart, B, Lp, nullptr, flagged)) return e;
  if (flagged.empty()) return 0;
  h->restart_list = std::move(flagged);
  const int E = h->cfg.embed_dim, Lmax = h->ep.Lmax, L = Lp + 1, n_r = (int)h->restart_list.size();
  Run R{h, (hipStream_t)stream};
  int* list = R.ws<int>((size_t)n_r);
  float* x32 = R.ws<float>((size_t)n_r * L * E);
  void* xT = R.wsT((size_t)n_r * L * E);
  uint8_t* mask = R.ws<uint8_t>((size_t)n_r * L);
  if (R.upload(list, h->restart_list)) return R.err;
  // ring mode: the sample's history may lie anywhere in the written part [P0, hw) of the ring
  OTHER(R, launch_episode_restart(list, n_r, h->ep.mask, nullptr, h->ep.fresh, L, h->ep.book.written_end(), Lmax, R.st), "seq_restart");
  OTHER(R, launch_seq_embed(prompt, stride_b, stride_l, prompt_mask, h->sep_token, nullptr, nullptr, h->pos_emb, Lmax, x32, xT, mask, n_r, L, Lp, h->ep.Q,
                            E, h->bf16, R.st, list, h->ep.mask, h->ep.poscnt, Lmax), "seq_embed_prefill");
  hfgpt_stack(R, x32, xT, mask, n_r, L, true, list);
  if (!R.err) h->ep.book.restart(h->restart_list);
  return R.err;
}

int vima_seq_history_room(VimaHandle* h, int32_t* steps_host) {
  if (int e = seq_ready(h, "vima_seq_history_room")) return e;
  return history_room(h, "vima_seq_history_room", true, steps_host, nullptr);
}

// vima_seq_decode_restart with a history: ONE full pass of the vima_seq_decode form over the n_r flagged samples, [prompt | sep | o_0, a_0, .., o_{T-1}],
// L = Lp + T (Q + 1) rows through hfgpt_stack, in place of the restart's prefix prefill. Per layer the K | V rows are scattered by (sample list, row map)
// in one launch: the prefix to rows [0, Lp], history step s to the cache rows batch step t - T + s wrote (t: the next batch step). Then one kernel
// writes the episode state. 3 launches + one stack pass (one launch more than the plain restart), whatever n_r. Host: the samples' ring age becomes that of a sample restarted right before
// batch step t - T.
int vima_seq_decode_restart_history(VimaHandle* h, const uint8_t* restart, int B, const float* prompt, int64_t stride_b, int64_t stride_l,
                                    const uint8_t* prompt_mask, int Lp, const float* hist_obs, const float* hist_act, int T, float* out,
                                    vima_stream_t stream) {
  if (T == 0) return vima_seq_decode_restart(h, restart, B, prompt, stride_b, stride_l, prompt_mask, Lp, stream);
  const char* fn = "vima_seq_decode_restart_history";
  if (int e = seq_ready(h, fn)) return e;
  if (T < 0) return fail("vima_seq_decode_restart_history: T must be >= 0");
  std::vector<int> flagged;
  if (int e = restart_begin(h, fn, true, !restart || !prompt || !prompt_mask || !hist_obs || (T > 1 && !hist_act), restart, B, Lp, nullptr, flagged)) return e;
  const int E = h->cfg.embed_dim, Q = h->ep.Q, Lmax = h->ep.Lmax, P0 = Lp + 1;
  // compact row l of the sequence -> cache row: the identity over the prefix; history step s sits in the slot of batch step t - T + s, its Q obs rows
  // in the slot's obs rows and a_s in the action row of the NEXT slot (the first slot's own action row, if it has one, stays masked)
  EpisodeBook::History H = h->ep.book.history(T, true);
  if (!H.fits) return room_refused(std::string(fn) + ": a history of " + std::to_string(T) + " steps", H.room);
  const long long L64 = (long long)Lp + (long long)T * (Q + 1);
  if (L64 > h->cfg.n_positions)
    return fail("vima_seq_decode_restart_history: sequence of " + std::to_string(L64) + " tokens (prompt, separator and " + std::to_string(T) +
                " steps) exceeds n_positions " + std::to_string(h->cfg.n_positions), 34);
  const int L = (int)L64, hi = h->ep.book.written_end(), n_r = (int)flagged.size();
  if (n_r == 0) return 0;
  if (!H.in_range || (int)H.rows.size() != L) return fail("vima_seq_decode_restart_history: internal error: history row outside the written cache");
  h->restart_list = std::move(flagged);
  h->hist_rowmap = std::move(H.rows);
  Run R{h, (hipStream_t)stream};
  int* list = R.ws<int>((size_t)n_r);
  int* hmap = R.ws<int>((size_t)L);
  float* x32 = R.ws<float>((size_t)n_r * L * E);
  void* xT = R.wsT((size_t)n_r * L * E);
  uint8_t* mask = R.ws<uint8_t>((size_t)n_r * L);
  if (R.upload(list, h->restart_list) || R.upload(hmap, h->hist_rowmap)) return R.err;
  OTHER(R, launch_seq_embed(prompt, stride_b, stride_l, prompt_mask, h->sep_token, hist_obs, hist_act, h->pos_emb, h->cfg.n_positions, x32, xT, mask,
                            n_r, L, Lp, Q, E, h->bf16, R.st, list), "seq_embed");
  if (hfgpt_stack(R, x32, xT, mask, n_r, L, true, list, hmap)) return R.err;
  if (out) OTHER(R, launch_gather_pred(x32 + (size_t)P0 * E, out, T, n_r, Q, L, E, R.st), "gather_pred");   // teacher-forced: the last obs row of every history step
  OTHER(R, launch_history_install(mask, list, hmap, n_r, L, P0, hi, Lmax, h->ep.mask, h->ep.poscnt, h->ep.fresh, R.st), "seq_history_install");
  if (!R.err) h->ep.book.install(h->restart_list, H.age);
  return R.err;
}

int vima_action_head(VimaHandle* h, const float* tokens, int Rn, float* out_logits, vima_stream_t stream) {
  if (!h) return fail("null handle");
  const std::string key = gkey("action_head", {(long long)(uintptr_t)tokens, Rn, (long long)(uintptr_t)out_logits});
  return run_graphed(h, key, (hipStream_t)stream, [&](hipStream_t st) -> int {
  if (int e = check_ready(h)) return e;
  if (Rn <= 0) return 0;
  Run R{h, st};
  return action_head_run(R, tokens, Rn, out_logits);
  });
}

int vima_action_embed(VimaHandle* h, const int64_t* const idx[4], int Rn, float* out, vima_stream_t stream) {
  if (!h) return fail("null handle");
  const std::string key = gkey("action_embed", {(long long)(uintptr_t)idx[0], (long long)(uintptr_t)idx[1], (long long)(uintptr_t)idx[2],
                                                (long long)(uintptr_t)idx[3], Rn, (long long)(uintptr_t)out});
  return run_graphed(h, key, (hipStream_t)stream, [&](hipStream_t st) -> int {
  if (int e = check_ready(h)) return e;
  if (Rn <= 0) return 0;
  Run R{h, st};
  void* t1 = R.wsT((size_t)Rn * 1024);
  if (R.err) return R.err;
  for (int k = 0; k < 4; ++k)
    OTHER(R, launch_action_l1((const long long*)idx[k], kActDims[k], h->act0[k].w0, h->act0[k].b0, t1, Rn, 1024, k * 256, h->bf16, R.st),
          "action_l1");
  return action_embed_tail(R, t1, Rn, out);
  });
}

int vima_action_select(const float* logits, int Rn, const float* u, const float* bounds, int64_t* const idx[4], float* cont,
                       float* log_prob, float* entropy, vima_stream_t stream) {
  if (Rn <= 0) return 0;
  if (!logits || !idx || !idx[0] || !idx[1] || !idx[2] || !idx[3]) return fail("vima_action_select: null argument");
  // the launch goes to the device that owns the logits (not necessarily the current one: the call has no handle)
  int cur_dev = 0, out_dev = 0;
  hipPointerAttribute_t pa;
  HIPCK(hipGetDevice(&cur_dev));
  out_dev = cur_dev;
  if (hipPointerGetAttributes(&pa, logits) == hipSuccess) out_dev = pa.device;
  else (void)hipGetLastError();
  struct DeviceGuard {
    int back; bool active;
    ~DeviceGuard() { if (active) (void)hipSetDevice(back); }
  } guard{cur_dev, false};
  if (out_dev != cur_dev) {
    HIPCK(hipSetDevice(out_dev));
    guard.active = true;
  }
  ActSelectArgs s;
  s.logits = logits; s.u = u; s.R = Rn; set_bounds(s, bounds);
  for (int k = 0; k < 4; ++k) s.idx[k] = (long long*)idx[k];
  s.cont = cont; s.logp = log_prob; s.ent = entropy;
  const int e = launch_act_select(s, false, (hipStream_t)stream);
  if (e) return fail(std::string("act_select launch failed: ") + hipGetErrorString((hipError_t)e), e);
  return 0;
}

int vima_act(VimaHandle* h, const float* tokens, int Rn, const float* u, const float* bounds, float* logits_out, int64_t* const idx[4],
             float* cont, float* log_prob, float* entropy, float* token, vima_stream_t stream) {
  if (!h) return fail("null handle");
  if (!tokens || !idx || !idx[0] || !idx[1] || !idx[2] || !idx[3]) return fail("vima_act: null argument");
  uint32_t bb[4] = {0, 0, 0, 0};   // the VALUES of the bounds are kernel arguments: part of the graph key
  if (bounds) memcpy(bb, bounds, sizeof bb);
  const std::string key = gkey("act", {(long long)(uintptr_t)tokens, Rn, (long long)(uintptr_t)u, bounds ? 1 : 0, (long long)bb[0], (long long)bb[1],
                                       (long long)bb[2], (long long)bb[3], (long long)(uintptr_t)logits_out, (long long)(uintptr_t)idx[0],
                                       (long long)(uintptr_t)idx[1], (long long)(uintptr_t)idx[2], (long long)(uintptr_t)idx[3],
                                       (long long)(uintptr_t)cont, (long long)(uintptr_t)log_prob, (long long)(uintptr_t)entropy,
                                       (long long)(uintptr_t)token});
  return run_graphed(h, key, (hipStream_t)stream, [&](hipStream_t st) -> int {
  if (int e = check_ready(h)) return e;
  if (Rn <= 0) return 0;
  Run R{h, st};
  float* logits = logits_out ? logits_out : R.ws<float>((size_t)Rn * kLogits);
  void* t1 = token ? R.wsT((size_t)Rn * 1024) : nullptr;
  if (R.err) return R.err;
  if (action_head_run(R, tokens, Rn, logits)) return R.err;
  ActSelectArgs s;
  s.logits = logits; s.u = u; s.R = Rn; set_bounds(s, bounds);
  for (int k = 0; k < 4; ++k) { s.idx[k] = (long long*)idx[k]; s.w0[k] = h->act0[k].w0; s.b0[k] = h->act0[k].b0; }
  s.cont = cont; s.logp = log_prob; s.ent = entropy; s.t1 = t1;
  OTHER(R, launch_act_select(s, h->bf16, R.st), "act_select");
  if (!token || R.err) return R.err;
  return action_embed_tail(R, t1, Rn, token);
  });
}

// VimaSampleOpts (NULL = defaults) into the kernel's argument block; the refusals of include/vima_hip.h, before any launch
static int set_sample_opts(ActSampleArgs& p, const VimaSampleOpts* o, const char* who) {
  if (!o) return 0;
  if (!(o->top_p > 0.f)) return fail(std::string(who) + ": top_p must be > 0");
  if (o->n_samples < 1) return fail(std::string(who) + ": n_samples must be >= 1");
  if (o->given && o->n_samples != 1) return fail(std::string(who) + ": given actions take n_samples == 1");
  p.temp = o->temperature; p.top_k = o->top_k; p.top_p = o->top_p; p.S = o->n_samples; p.given = o->given ? 1 : 0;
  return 0;
}

int vima_action_select_ex(const float* logits, int Rn, const float* u, const VimaSampleOpts* opts, const float* bounds,
                          int64_t* const idx[4], float* cont, float* log_prob, float* entropy, vima_stream_t stream) {
  ActSampleArgs p;
  if (!idx || !idx[0] || !idx[1] || !idx[2] || !idx[3]) return fail("vima_action_select_ex: null idx");
  if (int e = set_sample_opts(p, opts, "vima_action_select_ex")) return e;
  if (Rn <= 0) return 0;
  if (!logits) return fail("vima_action_select_ex: null argument");
  if ((long long)Rn * p.S > 0x7fffffffLL) return fail("vima_action_select_ex: R * n_samples exceeds 2^31 - 1");
  // the launch goes to the device that owns the logits, as in vima_action_select
  int cur_dev = 0, out_dev = 0;
  hipPointerAttribute_t pa;
  HIPCK(hipGetDevice(&cur_dev));
  out_dev = cur_dev;
  if (hipPointerGetAttributes(&pa, logits) == hipSuccess) out_dev = pa.device;
  else (void)hipGetLastError();
  struct DeviceGuard {
    int back; bool active;
    ~DeviceGuard() { if (active) (void)hipSetDevice(back); }
  } guard{cur_dev, false};
  if (out_dev != cur_dev) {
    HIPCK(hipSetDevice(out_dev));
    guard.active = true;
  }
  ActSelectArgs& s = p.sel;
  s.logits = logits; s.u = u; s.R = Rn * p.S; set_bounds(s, bounds);
  for (int k = 0; k < 4; ++k) s.idx[k] = (long long*)idx[k];
  s.cont = cont; s.logp = log_prob; s.ent = entropy;
  const int e = launch_act_sample(p, false, (hipStream_t)stream);
  if (e) return fail(std::string("act_sample launch failed: ") + hipGetErrorString((hipError_t)e), e);
  return 0;
}

int vima_act_ex(VimaHandle* h, const float* tokens, int Rn, const float* u, const VimaSampleOpts* opts, const float* bounds,
                float* logits_out, int64_t* const idx[4], float* cont, float* log_prob, float* entropy, float* token,
                vima_stream_t stream) {
  if (!h) return fail("null handle");
  if (!idx || !idx[0] || !idx[1] || !idx[2] || !idx[3]) return fail("vima_act_ex: null idx");
  ActSampleArgs p;
  if (int e = set_sample_opts(p, opts, "vima_act_ex")) return e;
  if (!tokens) return fail("vima_act_ex: null argument");
  if ((long long)Rn * p.S > 0x7fffffffLL) return fail("vima_act_ex: R * n_samples exceeds 2^31 - 1");
  uint32_t bb[4] = {0, 0, 0, 0}, pb = 0;   // the VALUES of the bounds and of top_p are kernel arguments: part of the graph key
  if (bounds) memcpy(bb, bounds, sizeof bb);
  memcpy(&pb, &p.top_p, sizeof pb);
  const std::string key = gkey("act_ex", {(long long)(uintptr_t)tokens, Rn, (long long)(uintptr_t)u, (long long)(uintptr_t)p.temp, p.S, p.top_k,
                                          (long long)pb, p.given, bounds ? 1 : 0, (long long)bb[0], (long long)bb[1], (long long)bb[2],
                                          (long long)bb[3], (long long)(uintptr_t)logits_out, (long long)(uintptr_t)idx[0],
                                          (long long)(uintptr_t)idx[1], (long long)(uintptr_t)idx[2], (long long)(uintptr_t)idx[3],
                                          (long long)(uintptr_t)cont, (long long)(uintptr_t)log_prob, (long long)(uintptr_t)entropy,
                                          (long long)(uintptr_t)token});
  return run_graphed(h, key, (hipStream_t)stream, [&](hipStream_t st) -> int {
  if (int e = check_ready(h)) return e;
  if (Rn <= 0) return 0;
  const int Ro = Rn * p.S;
  Run R{h, st};
  float* logits = logits_out ? logits_out : R.ws<float>((size_t)Rn * kLogits);
  void* t1 = token ? R.wsT((size_t)Ro * 1024) : nullptr;
  if (R.err) return R.err;
  if (action_head_run(R, tokens, Rn, logits)) return R.err;
  ActSampleArgs q = p;
  ActSelectArgs& s = q.sel;
  s.logits = logits; s.u = u; s.R = Ro; set_bounds(s, bounds);
  for (int k = 0; k < 4; ++k) { s.idx[k] = (long long*)idx[k]; s.w0[k] = h->act0[k].w0; s.b0[k] = h->act0[k].b0; }
  s.cont = cont; s.logp = log_prob; s.ent = entropy; s.t1 = t1;
  OTHER(R, launch_act_sample(q, h->bf16, R.st), "act_sample");
  if (!token || R.err) return R.err;
  return action_embed_tail(R, t1, Ro, token);
  });
}

// ---------------------------------------------------------------------------------------------- operator-level
__global__ void widen_kernel(const bf16_t* in, float* out, long long n) {
  long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = bf16_to_f32(in[i]);
}

int vima_op_linear(VimaHandle* h, const float* A, const float* W, const float* bias, const float* mul, const float* res, int M,
                   int N, int K, int act, float* out, vima_stream_t stream) {
  if (!h) return fail("null handle");
  HIPCK(hipSetDevice(h->device));
  if (h->arena.reset()) return fail("workspace reset failed");
  Run R{h, (hipStream_t)stream};
  void* aT = R.wsT((size_t)M * K);
  void* wT = R.wsT((size_t)N * K);
  void* mT = mul ? R.wsT((size_t)M * N) : nullptr;
  if (R.err) return R.err;
  if ((long long)M * K % 4 || (long long)N * K % 4 || (mul && (long long)M * N % 4)) return fail("vima_op_linear: sizes must be multiples of 4");
  OTHER(R, launch_cast(A, aT, (long long)M * K, h->bf16, R.st), "cast");
  OTHER(R, launch_cast(W, wT, (long long)N * K, h->bf16, R.st), "cast");
  if (mul) OTHER(R, launch_cast(mul, mT, (long long)M * N, h->bf16, R.st), "cast");
  GemmArgs a;
  a.A = aT; a.lda = K; a.W = wT; a.ldw = K; a.M = M; a.N = N; a.K = K; a.bias = bias; a.act = act; a.mul = mT; a.ldmul = N;
  a.res = res; a.ldres = N;
  if (h->op_stream_T && res) {   // residual carried in the operand type (the T5 / ViT stream form): res -> T, added in the epilogue
    void* rT = R.wsT((size_t)M * N);
    if (R.err) return R.err;
    if ((long long)M * N % 4) return fail("vima_op_linear: sizes must be multiples of 4");
    OTHER(R, launch_cast(res, rT, (long long)M * N, h->bf16, R.st), "cast");
    a.res = nullptr; a.resT = rT; a.ldresT = N;
  }
  if ((h->op_bf16_out || (h->op_stream_T && res)) && h->bf16) {   // exercise the operand-type (bf16) output path, then widen
    void* oT = R.wsT((size_t)M * N);
    if (R.err) return R.err;
    a.outT = oT; a.ldT = N;
    if (R.gemm(a)) return R.err;
    hipLaunchKernelGGL(widen_kernel, dim3((unsigned)(((long long)M * N + 255) / 256)), dim3(256), 0, R.st, (const bf16_t*)oT, out,
                       (long long)M * N);
    return R.other((int)hipGetLastError(), "widen");
  }
  a.out32 = out; a.ld32 = N;
  return R.gemm(a);
}

// One launch_gemm call described field for field by the caller: no casts, no widening, no gemm_*_ok question of its own -- what
// launch_gemm refuses comes back as the error. The only workspace is the split-K scratch, sized the way Run::gemm sizes it.
int vima_op_gemm(VimaHandle* h, const VimaGemmDesc* g, int* kernel_id, vima_stream_t stream) {
  if (!h) return fail("null handle");
  if (!g) return fail("vima_op_gemm: null descriptor");
  HIPCK(hipSetDevice(h->device));
  if (h->arena.reset()) return fail("workspace reset failed");
  Run R{h, (hipStream_t)stream};
  GemmArgs a;
  a.A = g->A; a.W = g->W; a.M = g->M; a.N = g->N; a.K = g->K; a.lda = g->lda; a.ldw = g->ldw; a.batch = g->batch;
  a.grp_col = g->grp_col;
  a.A2 = g->A2; a.W2 = g->W2; a.lda2 = g->lda2; a.ldw2 = g->ldw2;
  a.bsA = g->bsA; a.bsW = g->bsW; a.bsBias = g->bsBias; a.bsMul = g->bsMul; a.bsRes = g->bsRes; a.bs32 = g->bs32; a.bsT = g->bsT;
  a.bias = g->bias; a.act = g->act; a.mul = g->mul; a.ldmul = g->ldmul; a.res = g->res; a.ldres = g->ldres;
  a.resT = g->resT; a.ldresT = g->ldresT; a.out32 = g->out32; a.ld32 = g->ld32; a.outT = g->outT; a.ldT = g->ldT;
  a.hm_D = g->hm_D; a.hm_L = g->hm_L; a.pair32 = g->pair32;
  a.rb = g->rb; a.s_hi = g->s_hi; a.s_lo = g->s_lo; a.ro = g->ro;
  a.outT_lo = g->outT_lo; a.ldT_lo = g->ldT_lo; a.split_n = g->split_n;
  a.ssq_out = g->ssq_out; a.rs_ssq = g->rs_ssq; a.rs_parts = g->rs_parts; a.rs_invk = g->rs_invk; a.rs_eps = g->rs_eps;
  a.sum_out = g->sum_out; a.rs_sum = g->rs_sum; a.rs_c = g->rs_c;
  a.x3 = g->x3;
  a.tune = &h->tune;
  if (const size_t wsb = gemm_splitk_bytes(a, h->bf16)) {
    a.splitk_ws = R.ws<float>(wsb / sizeof(float));
    a.splitk_ws_bytes = wsb;
    if (R.err) return R.err;
  }
  int kid = 0;
  a.kernel_id = &kid;
  const int e = launch_gemm(a, h->bf16, R.st);
  if (kernel_id) *kernel_id = kid;
  if (e) return fail(std::string("vima_op_gemm: launch_gemm refused or failed: ") + hipGetErrorString((hipError_t)e) + " (M=" + std::to_string(a.M) +
                     " N=" + std::to_string(a.N) + " K=" + std::to_string(a.K) + ")", e);
  return 0;
}

int vima_op_layernorm(VimaHandle* h, const float* x, const float* gamma, const float* beta, float eps, int rms, int rows, int E,
                      float* out, vima_stream_t stream) {
  if (!h) return fail("null handle");
  HIPCK(hipSetDevice(h->device));
  Run R{h, (hipStream_t)stream};
  if (h->op_stream_T && h->bf16) {   // test instrumentation: the input carried in the operand type, like the ViT / decoder streams
    if (h->arena.reset()) return fail("workspace reset failed");
    void* xT = R.wsT((size_t)rows * E);
    if (R.err) return R.err;
    OTHER(R, launch_cast(x, xT, (long long)rows * E, true, R.st), "cast");
    return R.lnT(xT, E, gamma, beta, eps, rms, rows, E, out, nullptr);
  }
  return R.ln(x, E, gamma, beta, eps, rms, rows, E, out, nullptr);
}

static int op_attention(VimaHandle* h, const float* q, const float* k, const float* v, const uint8_t* kmask, const float* relbias,
                        int B, int H, int Lq, int Lk, int D, float scale, int mode, int impl, int q_off, int win_end, float* out, vima_stream_t stream) {
  if (!h) return fail("null handle");
  HIPCK(hipSetDevice(h->device));
  if (h->arena.reset()) return fail("workspace reset failed");
  Run R{h, (hipStream_t)stream};
  const long long nq = (long long)B * Lq * H * D, nk = (long long)B * Lk * H * D;
  void* qT = R.wsT(nq); void* kT = R.wsT(nk); void* vT = R.wsT(nk); void* oT = R.wsT(nq);
  if (R.err) return R.err;
  OTHER(R, launch_cast(q, qT, nq, h->bf16, R.st), "cast");
  OTHER(R, launch_cast(k, kT, nk, h->bf16, R.st), "cast");
  OTHER(R, launch_cast(v, vT, nk, h->bf16, R.st), "cast");
  AttnArgs a;
  a.q = qT; a.ldq = H * D; a.k = kT; a.ldk = H * D; a.v = vT; a.ldv = H * D; a.out = oT; a.ldo = H * D;
  a.kmask = kmask; a.relbias = relbias; a.bias_far = h->op_bias_far; a.B = B; a.H = H; a.Lq = Lq; a.Lk = Lk; a.D = D; a.scale = scale; a.mode = mode;
  a.q_off = q_off; a.win_end = win_end;
  if (impl == 1 && !h->bf16 && !h->x3) return fail("vima_op_attention: the MFMA kernel needs bf16 or bf16x3 precision");
  if (R.attn(a, impl)) return R.err;
  if (h->bf16) {
    hipLaunchKernelGGL(widen_kernel, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, R.st, (const bf16_t*)oT, out, nq);
    return R.other((int)hipGetLastError(), "widen");
  }
  HIPCK(hipMemcpyAsync(out, oT, nq * 4, hipMemcpyDeviceToDevice, R.st));
  return 0;
}

int vima_op_attention(VimaHandle* h, const float* q, const float* k, const float* v, const uint8_t* kmask, const float* relbias,
                      int B, int H, int Lq, int Lk, int D, float scale, int mode, int impl, float* out, vima_stream_t stream) {
  return op_attention(h, q, k, v, kmask, relbias, B, H, Lq, Lk, D, scale, mode, impl, 0, 0, out, stream);
}

int vima_op_attention_window(VimaHandle* h, const float* q, const float* k, const float* v, const uint8_t* kmask, int B, int H, int Lq, int Lk,
                             int D, float scale, int impl, int q_off, float* out, vima_stream_t stream) {
  if (q_off < 0 || Lq <= 0 || q_off + Lq > Lk) return fail("vima_op_attention_window: the window [q_off, q_off + Lq) must lie inside the Lk keys");
  return op_attention(h, q, k, v, kmask, nullptr, B, H, Lq, Lk, D, scale, ATTN_CAUSAL, impl, q_off, q_off + Lq, out, stream);
}

// ---- the ViT front end's non-GEMM kernels, one launcher call each (tests/test_vit_front_gpu.py). Same conventions as above: fp32 device
// buffers in and out, operands cast to the handle's operand type in the arena, the operand-type result widened back.
static int op_widen(Run& R, const void* oT, float* out, long long n) {
  if (R.err) return R.err;
  if (R.h->bf16) {
    hipLaunchKernelGGL(widen_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, R.st, (const bf16_t*)oT, out, n);
    return R.other((int)hipGetLastError(), "widen");
  }
  if (hipMemcpyAsync(out, oT, n * 4, hipMemcpyDeviceToDevice, R.st) != hipSuccess) return fail("widen: hipMemcpyAsync failed");
  return 0;
}

static int op_begin(VimaHandle* h, const char* fn) {
  if (!h) return fail(std::string(fn) + ": null handle");
  HIPCK(hipSetDevice(h->device));
  if (h->arena.reset()) return fail("workspace reset failed");
  return 0;
}

int vima_op_vit_attention(VimaHandle* h, const float* qkv, int M, int S, int W, int heads, int impl, float* out, vima_stream_t stream) {
  if (int e = op_begin(h, "vima_op_vit_attention")) return e;
  if (!qkv || !out) return fail("vima_op_vit_attention: null argument");
  if (M <= 0 || S <= 0 || W <= 0 || heads <= 0) return fail("vima_op_vit_attention: M, S, W and heads must be positive");
  if (impl < 0 || impl > 2) return fail("vima_op_vit_attention: impl must be 0 (the launcher's choice), 1 (register kernel) or 2 (its 16-score instantiation)");
  if (W % heads || W / heads != 32) return fail("vima_op_vit_attention: the head dim W / heads must be 32");
  Run R{h, (hipStream_t)stream};
  const long long rows = (long long)M * S;
  void* qT = R.wsT((size_t)rows * 3 * W); void* oT = R.wsT((size_t)rows * W);
  if (R.err) return R.err;
  OTHER(R, launch_cast(qkv, qT, rows * 3 * W, h->bf16, R.st), "cast");
  OTHER(R, launch_vit_attn(qT, oT, M, S, W, heads, h->bf16, R.st, nullptr, 1.0f, impl), "vima_op_vit_attention: vit_attn");
  return op_widen(R, oT, out, rows * W);
}

int vima_op_vit_attention_cls(VimaHandle* h, const float* q, const float* kv, int M, int S, int W, int heads, float* out, vima_stream_t stream) {
  if (int e = op_begin(h, "vima_op_vit_attention_cls")) return e;
  if (!q || !kv || !out) return fail("vima_op_vit_attention_cls: null argument");
  if (M <= 0 || S <= 0 || W <= 0 || heads <= 0) return fail("vima_op_vit_attention_cls: M, S, W and heads must be positive");
  if (W % heads || W / heads != 32) return fail("vima_op_vit_attention_cls: the head dim W / heads must be 32");
  Run R{h, (hipStream_t)stream};
  const long long rows = (long long)M * S;
  void* qT = R.wsT((size_t)M * W); void* kvT = R.wsT((size_t)rows * 2 * W); void* oT = R.wsT((size_t)M * W);
  if (R.err) return R.err;
  OTHER(R, launch_cast(q, qT, (long long)M * W, h->bf16, R.st), "cast");
  OTHER(R, launch_cast(kv, kvT, rows * 2 * W, h->bf16, R.st), "cast");
  OTHER(R, launch_vit_attn_cls(qT, kvT, oT, M, S, W, heads, h->bf16, R.st), "vima_op_vit_attention_cls: vit_attn_cls");
  return op_widen(R, oT, out, (long long)M * W);
}

int vima_op_patchify(VimaHandle* h, const uint8_t* img, int M, int H, int W, int P, int impl, float* out, vima_stream_t stream) {
  if (int e = op_begin(h, "vima_op_patchify")) return e;
  if (!img || !out) return fail("vima_op_patchify: null argument");
  if (M <= 0 || H <= 0 || W <= 0 || P <= 0) return fail("vima_op_patchify: M, H, W and P must be positive");
  if (impl < 0 || impl > 1) return fail("vima_op_patchify: impl must be 0 (by shape) or 1 (the rectangular kernel)");
  Run R{h, (hipStream_t)stream};
  const long long n = (long long)M * 3 * H * W;   // = rows x 3 P^2 when P divides H and W (anything else is refused below)
  void* oT = R.wsT((size_t)n);
  if (R.err) return R.err;
  if (H == 32 && W == 32 && P == 16 && impl == 0) OTHER(R, launch_patchify(img, oT, M, h->bf16, R.st), "vima_op_patchify: patchify");
  else OTHER(R, launch_patchify_rect(img, oT, M, H, W, P, h->bf16, R.st), "vima_op_patchify: patchify_rect");
  return op_widen(R, oT, out, n);
}

int vima_op_vit_embed(VimaHandle* h, const float* pre, const float* cls, const float* pos, const float* g, const float* b, int M, int S,
                      int n_patch, int impl, float* out, vima_stream_t stream) {
  if (int e = op_begin(h, "vima_op_vit_embed")) return e;
  if (!pre || !pos || !g || !b || !out) return fail("vima_op_vit_embed: null argument");
  if (M <= 0 || S <= 0 || n_patch <= 0) return fail("vima_op_vit_embed: M, S and n_patch must be positive");
  if (impl < 0 || impl > 1) return fail("vima_op_vit_embed: impl must be 0 (by shape) or 1 (the rectangular kernel)");
  if (S - (cls ? 1 : 0) > n_patch) return fail("vima_op_vit_embed: S tokens need S - (cls ? 1 : 0) <= n_patch patch rows per image");
  Run R{h, (hipStream_t)stream};
  const long long n = (long long)M * S * 768;
  void* xT = R.wsT((size_t)n);
  if (R.err) return R.err;
  if (cls && S == 5 && n_patch == 4 && impl == 0) OTHER(R, launch_vit_embed(pre, cls, pos, g, b, nullptr, xT, M, h->bf16, R.st), "vima_op_vit_embed: vit_embed");
  else OTHER(R, launch_vit_embed_rect(pre, cls, pos, g, b, nullptr, xT, M, S, n_patch, h->bf16, R.st), "vima_op_vit_embed: vit_embed_rect");
  return op_widen(R, xT, out, n);
}

int vima_op_bbox_l1(VimaHandle* h, const int64_t* bbox, const float* W, const float* b, int R_, int N, float* out, vima_stream_t stream) {
  if (int e = op_begin(h, "vima_op_bbox_l1")) return e;
  if (!bbox || !W || !b || !out) return fail("vima_op_bbox_l1: null argument");
  if (R_ <= 0 || N <= 0) return fail("vima_op_bbox_l1: R and N must be positive");
  Run R{h, (hipStream_t)stream};
  const long long n = (long long)R_ * N;
  void* oT = R.wsT((size_t)n);
  if (R.err) return R.err;
  OTHER(R, launch_bbox_l1((const long long*)bbox, W, b, oT, R_, N, h->bf16, R.st), "vima_op_bbox_l1: bbox_l1");
  return op_widen(R, oT, out, n);
}

// ---- the norm and sequence-assembly kernels of elementwise.hip / baseline_kernels.hip, one launcher call each (tests/test_seq_norm_gpu.py).
// Same conventions: fp32 / integer device buffers in and out, operands cast to the operand type in the arena, ONE call of the launcher under
// test, operand-type results widened back. Every check and every launcher refusal comes before the first write to a caller's buffer.
// Index arrays (tok_src, word_ids, list, sel) live on the device and are NOT validated here, as on the hot path: the caller sizes the buffers.
#define OP_REQ(cond, msg) do { if (!(cond)) return fail(std::string(fn) + ": " + (msg)); } while (0)

// an operand-type buffer whose untouched elements must come back as the caller left them: the caller's fp32 `out` (values exact in the operand
// type) is cast in before the launch and the whole buffer widened back after it
static void* op_stage_out(Run& R, const float* out, long long n) {
  void* oT = R.wsT((size_t)n);
  if (R.err) return nullptr;
  OTHER(R, launch_cast(out, oT, n, R.h->bf16, R.st), "cast");
  return R.err ? nullptr : oT;
}

int vima_op_norm(VimaHandle* h, const VimaNormDesc* d, vima_stream_t stream) {
  const char* fn = "vima_op_norm";
  if (int e = op_begin(h, fn)) return e;
  OP_REQ(d, "null descriptor");
  OP_REQ(d->x && d->rows > 0 && d->E > 0, "x, rows and E are required");
  OP_REQ(d->kind >= VIMA_NORM_LN && d->kind <= VIMA_NORM_RMS_STATS, "kind must be 0 (launch_layernorm), 1 (launch_layernorm_T), 2 (launch_layernorm2) or 3 (launch_rms_stats)");
  Run R{h, (hipStream_t)stream};
  const long long n = (long long)d->rows * d->E;
  if (d->kind == VIMA_NORM_RMS_STATS) {
    OP_REQ(d->outT && d->ssq, "rms_stats writes outT and ssq");
    OP_REQ(d->ldin == d->E, "rms_stats reads dense rows (ldin == E)");
    void* oT = R.wsT((size_t)n);
    if (R.err) return R.err;
    OTHER(R, launch_rms_stats(d->x, d->rows, d->E, oT, d->ssq, h->bf16, R.st), "vima_op_norm: rms_stats");
    return op_widen(R, oT, d->outT, n);
  }
  OP_REQ(d->gamma, "gamma is required");
  OP_REQ(d->ldin >= d->E, "ldin must be at least E");
  const bool two = d->kind == VIMA_NORM_LN2;
  OP_REQ(two || d->out32 || d->outT, "no output requested");
  OP_REQ(!two || (d->gamma2 && d->out2T && !d->rms), "layernorm2 needs gamma2 and out2T and has no rms form");
  void* oT = d->outT ? R.wsT((size_t)n) : nullptr;
  void* o2T = two ? R.wsT((size_t)n) : nullptr;
  if (R.err) return R.err;
  if (d->kind == VIMA_NORM_LN_T) {
    const long long nin = (long long)d->rows * d->ldin;   // the caller's buffer holds rows * ldin elements
    void* xT = R.wsT((size_t)nin);
    if (R.err) return R.err;
    OTHER(R, launch_cast(d->x, xT, nin, h->bf16, R.st), "cast");
    OTHER(R, launch_layernorm_T(xT, d->ldin, d->gamma, d->beta, d->eps, d->rms, d->rows, d->E, d->out32, oT, h->bf16, R.st), "vima_op_norm: layernorm_T");
  } else if (two) {
    OTHER(R, launch_layernorm2(d->x, d->ldin, d->gamma, d->beta, d->eps, d->gamma2, d->beta2, d->eps2, d->rows, d->E, d->out32, oT, o2T, h->bf16, R.st),
          "vima_op_norm: layernorm2");
  } else {
    OTHER(R, launch_layernorm(d->x, d->ldin, d->gamma, d->beta, d->eps, d->rms, d->rows, d->E, d->out32, oT, h->bf16, R.st), "vima_op_norm: layernorm");
  }
  if (R.err) return R.err;
  if (oT && op_widen(R, oT, d->outT, n)) return R.err ? R.err : 1;
  return two ? op_widen(R, o2T, d->out2T, n) : 0;
}

// ---- the e4m3 producers outside the GEMM epilogue and the calibration's max |x| (tests/test_fp8_producers_gpu.py), one launcher call each.
// Same conventions; the caller's out8 receives the launcher's bytes directly (nothing to widen). The launchers only emit e4m3 from bf16 operands, so
// every entry refuses a handle whose operand type is fp32 before anything is written.
static int op_fp8_begin(VimaHandle* h, const char* fn) {
  if (int e = op_begin(h, fn)) return e;
  OP_REQ(h->bf16, "the e4m3 producers read bf16 operands: needs a BF16 / FP8W / FP8 handle");
  return 0;
}

// the fp32 rows [rows, ldin] of a caller as the bf16 operand the launcher reads
static void* op_stage_rows(Run& R, const float* x, long long rows, long long ldin) {
  void* xT = R.wsT((size_t)(rows * ldin));
  if (R.err) return nullptr;
  OTHER(R, launch_cast(x, xT, rows * ldin, true, R.st), "cast");
  return R.err ? nullptr : xT;
}

int vima_op_fp8_quant(VimaHandle* h, const float* x, int64_t ldin, int64_t rows, int cols, float inv, uint8_t* out8, int64_t ldo, vima_stream_t stream) {
  const char* fn = "vima_op_fp8_quant";
  if (int e = op_fp8_begin(h, fn)) return e;
  OP_REQ(x && out8, "null argument");
  OP_REQ(rows >= 0 && cols > 0, "rows must not be negative and cols must be positive");
  OP_REQ(ldin >= cols && ldo >= cols, "ldin and ldo must be at least cols");
  if (rows == 0) return 0;
  Run R{h, (hipStream_t)stream};
  void* xT = op_stage_rows(R, x, rows, ldin);
  if (!xT) return R.err;
  OTHER(R, launch_quant_fp8(xT, ldin, rows, cols, inv, out8, ldo, R.st), "vima_op_fp8_quant: quant_fp8");
  return R.err;
}

int vima_op_fp8_amax(VimaHandle* h, const float* x, int64_t ldin, int64_t rows, int cols, float* slot, vima_stream_t stream) {
  const char* fn = "vima_op_fp8_amax";
  if (int e = op_fp8_begin(h, fn)) return e;
  OP_REQ(x && slot, "null argument");
  OP_REQ(rows >= 0 && cols > 0, "rows must not be negative and cols must be positive");
  OP_REQ(ldin >= cols, "ldin must be at least cols");
  if (rows == 0) return 0;
  Run R{h, (hipStream_t)stream};
  void* xT = op_stage_rows(R, x, rows, ldin);
  if (!xT) return R.err;
  OTHER(R, launch_amax(xT, ldin, rows, cols, slot, R.st), "vima_op_fp8_amax: amax");
  return R.err;
}

int vima_op_norm_fp8(VimaHandle* h, const VimaNormDesc* d, uint8_t* out8, float inv8, vima_stream_t stream) {
  const char* fn = "vima_op_norm_fp8";
  if (int e = op_fp8_begin(h, fn)) return e;
  OP_REQ(d && out8, "null argument");
  OP_REQ(d->kind == VIMA_NORM_LN_T, "kind must be 1 (launch_layernorm_T), the only norm launcher with an e4m3 output");
  OP_REQ(d->x && d->gamma && d->rows > 0 && d->E > 0, "x, gamma, rows and E are required");
  OP_REQ(d->ldin >= d->E, "ldin must be at least E");
  Run R{h, (hipStream_t)stream};
  const long long n = (long long)d->rows * d->E;
  void* oT = d->outT ? R.wsT((size_t)n) : nullptr;
  if (R.err) return R.err;
  void* xT = op_stage_rows(R, d->x, d->rows, d->ldin);
  if (!xT) return R.err;
  OTHER(R, launch_layernorm_T(xT, d->ldin, d->gamma, d->beta, d->eps, d->rms, d->rows, d->E, d->out32, oT, true, R.st, out8, inv8), "vima_op_norm_fp8: layernorm_T");
  if (R.err) return R.err;
  return oT ? op_widen(R, oT, d->outT, n) : 0;
}

int vima_op_vit_attention_fp8(VimaHandle* h, const float* qkv, int M, int S, int W, int heads, int impl, float inv8, uint8_t* out8, vima_stream_t stream) {
  const char* fn = "vima_op_vit_attention_fp8";
  if (int e = op_fp8_begin(h, fn)) return e;
  OP_REQ(qkv && out8, "null argument");
  OP_REQ(M > 0 && S > 0 && W > 0 && heads > 0, "M, S, W and heads must be positive");
  OP_REQ(impl >= 0 && impl <= 2, "impl must be 0 (the launcher's choice), 1 (register kernel) or 2 (its 16-score instantiation)");
  OP_REQ(W % heads == 0 && W / heads == 32, "the head dim W / heads must be 32");
  Run R{h, (hipStream_t)stream};
  const long long rows = (long long)M * S;
  void* oT = R.wsT((size_t)rows * W);   // the operand-type output of the launcher: not written on this path
  if (R.err) return R.err;
  void* qT = op_stage_rows(R, qkv, rows, 3LL * W);
  if (!qT) return R.err;
  OTHER(R, launch_vit_attn(qT, oT, M, S, W, heads, true, R.st, out8, inv8, impl), "vima_op_vit_attention_fp8: vit_attn");
  return R.err;
}

int vima_op_vit_attention_cls_fp8(VimaHandle* h, const float* q, const float* kv, int M, int S, int W, int heads, float inv8, uint8_t* out8, vima_stream_t stream) {
  const char* fn = "vima_op_vit_attention_cls_fp8";
  if (int e = op_fp8_begin(h, fn)) return e;
  OP_REQ(q && kv && out8, "null argument");
  OP_REQ(M > 0 && S > 0 && W > 0 && heads > 0, "M, S, W and heads must be positive");
  OP_REQ(W % heads == 0 && W / heads == 32, "the head dim W / heads must be 32");
  Run R{h, (hipStream_t)stream};
  void* oT = R.wsT((size_t)M * W);
  if (R.err) return R.err;
  void* qT = op_stage_rows(R, q, M, W);
  if (!qT) return R.err;
  void* kvT = op_stage_rows(R, kv, (long long)M * S, 2LL * W);
  if (!kvT) return R.err;
  OTHER(R, launch_vit_attn_cls(qT, kvT, oT, M, S, W, heads, true, R.st, out8, inv8), "vima_op_vit_attention_cls_fp8: vit_attn_cls");
  return R.err;
}

int vima_op_prompt_assemble(VimaHandle* h, const int32_t* tok_src, const int64_t* word_ids, const float* word_table, const float* obj_tokens,
                            const uint8_t* obj_mask, int rows, int E, int stats, float* x, float* ssq, uint8_t* mask, vima_stream_t stream) {
  const char* fn = "vima_op_prompt_assemble";
  if (int e = op_begin(h, fn)) return e;
  OP_REQ(tok_src && word_ids && word_table && obj_tokens && obj_mask && x && mask && (ssq || !stats), "null argument");
  OP_REQ(rows > 0 && E > 0, "rows and E must be positive");
  Run R{h, (hipStream_t)stream};
  if (!stats) {
    OTHER(R, launch_prompt_assemble(tok_src, (const long long*)word_ids, word_table, obj_tokens, obj_mask, x, mask, rows, E, R.st), "vima_op_prompt_assemble: prompt_assemble");
    return R.err;
  }
  void* xT = R.wsT((size_t)rows * E);
  if (R.err) return R.err;
  OTHER(R, launch_prompt_assemble_stats(tok_src, (const long long*)word_ids, word_table, obj_tokens, obj_mask, xT, ssq, mask, rows, E, h->bf16, R.st),
        "vima_op_prompt_assemble: prompt_assemble_stats");
  return op_widen(R, xT, x, (long long)rows * E);
}

int vima_op_dec_embed(VimaHandle* h, const float* obs_tok, const uint8_t* obs_mask, const float* act_tok, const float* pos_table, int n_pos,
                      int T, int B, int Q, int L_act, int E, float* x32, float* xT, uint8_t* mask, vima_stream_t stream) {
  const char* fn = "vima_op_dec_embed";
  if (int e = op_begin(h, fn)) return e;
  OP_REQ(obs_tok && obs_mask && pos_table && x32 && mask && (act_tok || L_act == 0), "null argument");
  OP_REQ(T > 0 && B > 0 && Q > 0 && E > 0 && n_pos > 0, "T, B, Q, E and n_pos must be positive");
  OP_REQ(L_act == T || L_act == T - 1, "L_act must be T or T - 1");
  Run R{h, (hipStream_t)stream};
  const long long n = (long long)B * (T * Q + L_act) * E;
  void* oT = xT ? R.wsT((size_t)n) : nullptr;
  if (R.err) return R.err;
  OTHER(R, launch_dec_embed(obs_tok, obs_mask, act_tok, pos_table, n_pos, x32, oT, mask, T, B, Q, L_act, E, h->bf16, R.st), "vima_op_dec_embed: dec_embed");
  return oT ? op_widen(R, oT, xT, n) : R.err;
}

int vima_op_dec_embed_step(VimaHandle* h, const float* obs_tok, const uint8_t* obs_mask, const float* act_tok, const float* pos_table, int n_pos,
                           int L_hist, int Lmax, int B, int Q, int has_act, int E, float* x32, float* xT, uint8_t* hist_mask, int32_t* poscnt,
                           uint8_t* fresh, vima_stream_t stream) {
  const char* fn = "vima_op_dec_embed_step";
  if (int e = op_begin(h, fn)) return e;
  OP_REQ(obs_tok && obs_mask && pos_table && x32 && hist_mask && poscnt && (act_tok || !has_act), "null argument");
  OP_REQ(B > 0 && Q > 0 && E > 0 && n_pos > 0 && L_hist >= 0 && (has_act == 0 || has_act == 1), "B, Q, E, n_pos must be positive, L_hist >= 0, has_act 0 or 1");
  OP_REQ(Q + has_act <= 64 && E % 4 == 0 && (long long)L_hist + Q + has_act <= Lmax, "dec_embed_step takes Q + has_act <= 64 rows inside Lmax, E % 4 == 0");
  Run R{h, (hipStream_t)stream};
  const long long n = (long long)B * (Q + has_act) * E;
  void* oT = xT ? R.wsT((size_t)n) : nullptr;
  if (R.err) return R.err;
  OTHER(R, launch_dec_embed_chunk(obs_tok, obs_mask, act_tok, pos_table, n_pos, x32, oT, hist_mask, poscnt, L_hist, Lmax, 1, B, Q, has_act, E, h->bf16, R.st, fresh),
        "vima_op_dec_embed_step: dec_embed_chunk");
  return oT ? op_widen(R, oT, xT, n) : R.err;
}

int vima_op_restart_samples(VimaHandle* h, const uint8_t* flags, uint8_t* hist_mask, int32_t* poscnt, uint8_t* fresh, int B, int Lmax, vima_stream_t stream) {
  const char* fn = "vima_op_restart_samples";
  if (int e = op_begin(h, fn)) return e;
  OP_REQ(flags && hist_mask && poscnt && fresh, "null argument");
  OP_REQ(B > 0 && Lmax > 0, "B and Lmax must be positive");
  // a test entry, never captured: the DEVICE flags come back to the host, which builds the sample list launch_episode_restart takes
  Run R{h, (hipStream_t)stream};
  std::vector<uint8_t> host((size_t)B);
  HIPCK(hipMemcpyAsync(host.data(), flags, (size_t)B, hipMemcpyDeviceToHost, R.st));
  HIPCK(hipStreamSynchronize(R.st));
  const std::vector<int> flagged = flagged_list(host.data(), B);
  if (flagged.empty()) return 0;
  int* list = R.ws<int>(flagged.size());
  if (R.err) return R.err;
  HIPCK(hipMemcpyAsync(list, flagged.data(), flagged.size() * sizeof(int), hipMemcpyHostToDevice, R.st));
  OTHER(R, launch_episode_restart(list, (int)flagged.size(), hist_mask, poscnt, fresh, 0, Lmax, Lmax, R.st), "vima_op_restart_samples: restart_samples");
  HIPCK(hipStreamSynchronize(R.st));   // `flagged` is the source of the upload
  return R.err;
}

int vima_op_prompt_pos(VimaHandle* h, const float* prompt, int64_t sb, int64_t sl, const uint8_t* mask, const float* pos_table, int n_pos,
                       const int32_t* list, int B, int Lp, int E, float* out, vima_stream_t stream) {
  const char* fn = "vima_op_prompt_pos";
  if (int e = op_begin(h, fn)) return e;
  OP_REQ(prompt && mask && pos_table && out, "null argument");
  OP_REQ(B > 0 && Lp > 0 && E > 0 && n_pos > 0, "B, Lp, E and n_pos must be positive");
  Run R{h, (hipStream_t)stream};
  const long long n = (long long)B * Lp * E;
  void* oT = R.wsT((size_t)n);
  if (R.err) return R.err;
  OTHER(R, launch_prompt_pos(prompt, sb, sl, mask, pos_table, n_pos, oT, B, Lp, E, h->bf16, R.st, list), "vima_op_prompt_pos: prompt_pos");
  return op_widen(R, oT, out, n);
}

int vima_op_gather_pred(VimaHandle* h, const float* x, int T, int B, int Q, int Lq, int E, float* out, vima_stream_t stream) {
  const char* fn = "vima_op_gather_pred";
  if (int e = op_begin(h, fn)) return e;
  OP_REQ(x && out, "null argument");
  OP_REQ(T > 0 && B > 0 && Q > 0 && E > 0 && E % 4 == 0, "T, B, Q must be positive, E a positive multiple of 4");
  OP_REQ((Q - 1) + (long long)(Q + 1) * (T - 1) < Lq, "row Q - 1 of the last step lies beyond Lq");
  Run R{h, (hipStream_t)stream};
  OTHER(R, launch_gather_pred(x, out, T, B, Q, Lq, E, R.st), "vima_op_gather_pred: gather_pred");
  return R.err;
}

int vima_op_action_l1(VimaHandle* h, const int64_t* idx, int K, const float* W, const float* b, int R_, int ldo, int col0, float* out,
                      vima_stream_t stream) {
  const char* fn = "vima_op_action_l1";
  if (int e = op_begin(h, fn)) return e;
  OP_REQ(idx && W && b && out, "null argument");
  OP_REQ(K == 2 || K == 4, "K must be 2 (position) or 4 (rotation)");
  OP_REQ(R_ > 0 && col0 >= 0 && col0 + 256 <= ldo && ldo % 4 == 0, "R must be positive and the 256 columns from col0 on lie inside ldo (a multiple of 4)");
  Run R{h, (hipStream_t)stream};
  const long long n = (long long)R_ * ldo;
  void* oT = op_stage_out(R, out, n);
  if (!oT) return R.err;
  OTHER(R, launch_action_l1((const long long*)idx, K, W, b, oT, R_, ldo, col0, h->bf16, R.st), "vima_op_action_l1: action_l1");
  return op_widen(R, oT, out, n);
}

int vima_op_add_row_table(VimaHandle* h, float* out, int rows, int E, const float* table, const int64_t* sel, int group, vima_stream_t stream) {
  const char* fn = "vima_op_add_row_table";
  if (int e = op_begin(h, fn)) return e;
  OP_REQ(out && table && sel, "null argument");
  OP_REQ(rows > 0 && E > 0 && group > 0, "rows, E and group must be positive");
  Run R{h, (hipStream_t)stream};
  OTHER(R, launch_add_row_table(out, rows, E, table, (const long long*)sel, group, R.st), "vima_op_add_row_table: add_row_table");
  return R.err;
}

int vima_op_rows_to_headmajor(VimaHandle* h, const float* in, int L, int N, int D, float* out, vima_stream_t stream) {
  const char* fn = "vima_op_rows_to_headmajor";
  if (int e = op_begin(h, fn)) return e;
  OP_REQ(in && out, "null argument");
  OP_REQ(L > 0 && N > 0 && D > 0 && N % 4 == 0, "L, N and D must be positive, N a multiple of 4");
  Run R{h, (hipStream_t)stream};
  const long long n = (long long)L * N;
  void* iT = R.wsT((size_t)n); void* oT = R.wsT((size_t)n);
  if (R.err) return R.err;
  OTHER(R, launch_cast(in, iT, n, h->bf16, R.st), "cast");
  KvRowsArgs c;
  c.in = iT; c.out = oT; c.n = 1; c.L = c.Lc = L; c.N = c.ld = N; c.D = D;
  OTHER(R, launch_kv_rows(c, (int)h->esz(), R.st), "vima_op_rows_to_headmajor: rows_to_headmajor");
  return op_widen(R, oT, out, n);
}

int vima_op_kv_scatter(VimaHandle* h, const float* in, const int32_t* list, int n, int L, int N, int D, int hm, int n_blocks, float* out,
                       vima_stream_t stream) {
  const char* fn = "vima_op_kv_scatter";
  if (int e = op_begin(h, fn)) return e;
  OP_REQ(in && list && out, "null argument");
  OP_REQ(n > 0 && L > 0 && N > 0 && D > 0 && n_blocks > 0 && N % 4 == 0, "n, L, N, D and n_blocks must be positive, N a multiple of 4");
  Run R{h, (hipStream_t)stream};
  const long long ni = (long long)n * L * N, no = (long long)n_blocks * L * N;
  void* iT = R.wsT((size_t)ni);
  if (R.err) return R.err;
  OTHER(R, launch_cast(in, iT, ni, h->bf16, R.st), "cast");
  void* oT = op_stage_out(R, out, no);
  if (!oT) return R.err;
  KvRowsArgs c;
  c.in = iT; c.out = oT; c.list = list; c.n = n; c.L = c.Lc = L; c.N = c.ld = N; c.D = hm ? D : 0;
  OTHER(R, launch_kv_rows(c, (int)h->esz(), R.st), "vima_op_kv_scatter: kv_scatter");
  return op_widen(R, oT, out, no);
}

int vima_op_seq_kv_store(VimaHandle* h, const float* in, int64_t ld_in, const int32_t* list, int n, int L, int N, int Lmax, int n_blocks,
                         float* out, vima_stream_t stream) {
  const char* fn = "vima_op_seq_kv_store";
  if (int e = op_begin(h, fn)) return e;
  OP_REQ(in && out, "null argument");
  OP_REQ(n > 0 && L > 0 && N > 0 && Lmax > 0 && n_blocks > 0 && ld_in >= N && ld_in % 4 == 0 && N % 4 == 0,
         "n, L, N, Lmax and n_blocks must be positive, ld_in >= N, ld_in and N multiples of 4");
  Run R{h, (hipStream_t)stream};
  const long long ni = (long long)n * L * ld_in, no = (long long)n_blocks * Lmax * N;
  void* iT = R.wsT((size_t)ni);
  if (R.err) return R.err;
  OTHER(R, launch_cast(in, iT, ni, h->bf16, R.st), "cast");
  void* oT = op_stage_out(R, out, no);
  if (!oT) return R.err;
  KvRowsArgs c;
  c.in = iT; c.ld = ld_in; c.out = oT; c.list = list; c.n = n; c.L = L; c.N = N; c.Lc = Lmax;
  OTHER(R, launch_kv_rows(c, (int)h->esz(), R.st), "vima_op_seq_kv_store: seq_kv_store");
  return op_widen(R, oT, out, no);
}

int vima_op_broadcast_rows(VimaHandle* h, const float* src, int64_t rows, int E, int period, float* out, vima_stream_t stream) {
  const char* fn = "vima_op_broadcast_rows";
  if (int e = op_begin(h, fn)) return e;
  OP_REQ(src && out, "null argument");
  OP_REQ(rows > 0 && E > 0, "rows and E must be positive");
  Run R{h, (hipStream_t)stream};
  OTHER(R, launch_broadcast_rows(src, out, rows, E, period, R.st), "vima_op_broadcast_rows: broadcast_rows");
  return R.err;
}

int vima_op_seq_embed(VimaHandle* h, const float* prompt, int64_t sb, int64_t sl, const uint8_t* pmask, const float* sep, const float* obs_tok,
                      const float* act_tok, const float* pos_table, int n_pos, int B, int L, int Lp, int Q, int E, float* x32, float* xT,
                      uint8_t* mask, vima_stream_t stream) {
  const char* fn = "vima_op_seq_embed";
  if (int e = op_begin(h, fn)) return e;
  OP_REQ(prompt && pmask && sep && pos_table && x32 && mask, "null argument");
  OP_REQ(B > 0 && Lp > 0 && Q > 0 && E > 0 && n_pos > 0 && L >= Lp + 1, "B, Lp, Q, E and n_pos must be positive and L >= Lp + 1");
  OP_REQ(L == Lp + 1 || obs_tok, "rows past the separator need obs_tok");
  OP_REQ(L - Lp - 1 <= Q || act_tok, "rows past the first step's observations need act_tok");
  Run R{h, (hipStream_t)stream};
  const long long n = (long long)B * L * E;
  void* oT = R.wsT((size_t)n);
  if (R.err) return R.err;
  OTHER(R, launch_seq_embed(prompt, sb, sl, pmask, sep, obs_tok, act_tok, pos_table, n_pos, x32, oT, mask, B, L, Lp, Q, E, h->bf16, R.st), "vima_op_seq_embed: seq_embed");
  return xT ? op_widen(R, oT, xT, n) : R.err;
}

int vima_op_seq_embed_prefill(VimaHandle* h, const float* prompt, int64_t sb, int64_t sl, const uint8_t* pmask, const float* sep,
                              const float* pos_table, int n_pos, const int32_t* list, int n, int Lp, int E, float* x32, float* xT, uint8_t* mask,
                              uint8_t* cache_mask, int32_t* posbase, vima_stream_t stream) {
  const char* fn = "vima_op_seq_embed_prefill";
  if (int e = op_begin(h, fn)) return e;
  OP_REQ(prompt && pmask && sep && pos_table && x32 && mask && cache_mask && posbase, "null argument");
  OP_REQ(n > 0 && Lp > 0 && E > 0 && n_pos > 0, "n, Lp, E and n_pos must be positive");
  Run R{h, (hipStream_t)stream};
  const long long ne = (long long)n * (Lp + 1) * E;
  void* oT = R.wsT((size_t)ne);
  if (R.err) return R.err;
  OTHER(R, launch_seq_embed(prompt, sb, sl, pmask, sep, nullptr, nullptr, pos_table, n_pos, x32, oT, mask, n, Lp + 1, Lp, 1, E, h->bf16, R.st, list,
                            cache_mask, posbase, n_pos), "vima_op_seq_embed_prefill: seq_embed_prefill");
  return xT ? op_widen(R, oT, xT, ne) : R.err;
}

int vima_op_seq_embed_step(VimaHandle* h, const float* obs_tok, const float* act_tok, const float* pos_table, int n_pos, int row0, int B, int Q,
                           int has_act, int E, float* x32, float* xT, uint8_t* cache_mask, int32_t* posbase, uint8_t* fresh, vima_stream_t stream) {
  const char* fn = "vima_op_seq_embed_step";
  if (int e = op_begin(h, fn)) return e;
  OP_REQ(obs_tok && pos_table && x32 && cache_mask && posbase && fresh, "null argument");
  OP_REQ(B > 0 && E > 0 && n_pos > 0 && (has_act == 0 || has_act == 1), "B, E and n_pos must be positive, has_act 0 or 1");
  OP_REQ(Q > 0 && Q + has_act <= 64 && E % 4 == 0 && row0 >= 0 && (long long)row0 + Q + has_act <= n_pos && (act_tok || !has_act),
         "seq_embed_step takes 1 <= Q, Q + has_act <= 64 rows inside n_pos, E % 4 == 0, act_tok with has_act");
  Run R{h, (hipStream_t)stream};
  const long long n = (long long)B * (Q + has_act) * E;
  void* oT = R.wsT((size_t)n);
  if (R.err) return R.err;
  OTHER(R, launch_seq_embed_chunk(obs_tok, act_tok, pos_table, n_pos, x32, oT, cache_mask, posbase, fresh, row0, 1, B, Q, has_act, E, h->bf16, R.st),
        "vima_op_seq_embed_step: seq_embed_chunk");
  return xT ? op_widen(R, oT, xT, n) : R.err;
}

int vima_op_seq_embed_chunk(VimaHandle* h, const float* obs_tok, const float* act_tok, const float* pos_table, int n_pos, int row0, int T, int B, int Q,
                            int has_act, int E, float* x32, float* xT, uint8_t* cache_mask, int32_t* posbase, uint8_t* fresh, vima_stream_t stream) {
  const char* fn = "vima_op_seq_embed_chunk";
  if (int e = op_begin(h, fn)) return e;
  OP_REQ(obs_tok && pos_table && x32 && cache_mask && posbase && fresh, "null argument");
  OP_REQ(T > 0 && B > 0 && Q > 0 && E > 0 && n_pos > 0 && (has_act == 0 || has_act == 1), "T, B, Q, E and n_pos must be positive, has_act 0 or 1");
  Run R{h, (hipStream_t)stream};
  const long long n = (long long)B * ((long long)T * (Q + 1) - (has_act ? 0 : 1)) * E;
  void* oT = R.wsT((size_t)n);
  if (R.err) return R.err;
  OTHER(R, launch_seq_embed_chunk(obs_tok, act_tok, pos_table, n_pos, x32, oT, cache_mask, posbase, fresh, row0, T, B, Q, has_act, E, h->bf16, R.st),
        "vima_op_seq_embed_chunk: seq_embed_chunk");
  return xT ? op_widen(R, oT, xT, n) : R.err;
}

int vima_op_seq_history_install(VimaHandle* h, const uint8_t* mask, const int32_t* list, const int32_t* rowmap, int n, int L, int lo, int hi, int n_pos,
                                uint8_t* cache_mask, int32_t* posbase, uint8_t* fresh, vima_stream_t stream) {
  const char* fn = "vima_op_seq_history_install";
  if (int e = op_begin(h, fn)) return e;
  OP_REQ(mask && list && rowmap && cache_mask && posbase && fresh, "null argument");
  OP_REQ(n > 0 && L > 0 && n_pos > 0, "n, L and n_pos must be positive");
  Run R{h, (hipStream_t)stream};
  OTHER(R, launch_history_install(mask, list, rowmap, n, L, lo, hi, n_pos, cache_mask, posbase, fresh, R.st),
        "vima_op_seq_history_install: seq_history_install");
  return R.err;
}

int vima_op_seq_restart(VimaHandle* h, const int32_t* list, int n, int lo, int hi, int n_pos, uint8_t* cache_mask, uint8_t* fresh, vima_stream_t stream) {
  const char* fn = "vima_op_seq_restart";
  if (int e = op_begin(h, fn)) return e;
  OP_REQ(list && cache_mask && fresh, "null argument");
  OP_REQ(n > 0 && n_pos > 0, "n and n_pos must be positive");
  Run R{h, (hipStream_t)stream};
  OTHER(R, launch_episode_restart(list, n, cache_mask, nullptr, fresh, lo, hi, n_pos, R.st), "vima_op_seq_restart: seq_restart");
  return R.err;
}

// ---- episode fork (episode_fork.hip) ---------------------------------------------------------------------------------------------
// The host side of one fork call, kept in the handle (fork_table: the source of the ONE upload): [jobs of cache 0 | jobs of cache 1 | dsts | srcs],
// the (destination, source) pairs grouped by source, the jobs of a group split over at most kForkMaxDst destinations each.
namespace {
struct ForkGroup { int src, dst0, ndst; };   // destinations dsts[dst0 .. dst0 + ndst)
struct ForkTable {
  std::vector<ForkJob> jobs[2];
  int units[2] = {0, 0};
  // one range [row0, row1) of group g into cache c, whose rows hold rv 16-byte vectors
  void add(int c, const ForkGroup& g, int row0, int row1, long long rv) {
    if (row1 <= row0 || g.ndst <= 0) return;
    const int chunks = (int)(((long long)(row1 - row0) * rv + kForkChunk - 1) / kForkChunk);
    for (int d = 0; d < g.ndst; d += kForkMaxDst) {
      jobs[c].push_back(ForkJob{g.src, g.dst0 + d, std::min(kForkMaxDst, g.ndst - d), row0, row1 - row0, units[c]});
      units[c] += chunks;
    }
  }
};
}  // namespace

// uploads the table and launches: per cache with jobs one episode_fork launch, then (mask given) the per-sample state -- at most 3 launches
static int fork_launch(Run& R, const ForkTable& T, const std::vector<int>& dsts, const std::vector<int>& srcs, void* const cache[2], const int L[2],
                       int NL, int B, int N, bool is_bf16, uint8_t* mask, int* poscnt, uint8_t* fresh, int Lmax) {
  VimaHandle* h = R.h;
  const size_t nj0 = T.jobs[0].size(), nj1 = T.jobs[1].size(), np = dsts.size(), ji = sizeof(ForkJob) / sizeof(int);
  std::vector<int>& tab = h->fork_table;
  tab.resize((nj0 + nj1) * ji + 2 * np);
  if (nj0) memcpy(tab.data(), T.jobs[0].data(), nj0 * sizeof(ForkJob));
  if (nj1) memcpy(tab.data() + nj0 * ji, T.jobs[1].data(), nj1 * sizeof(ForkJob));
  std::copy(dsts.begin(), dsts.end(), tab.begin() + (nj0 + nj1) * ji);
  std::copy(srcs.begin(), srcs.end(), tab.begin() + (nj0 + nj1) * ji + np);
  int* dev = R.ws<int>(tab.size());
  if (R.upload(dev, tab)) return R.err;
  const int* ddst = dev + (nj0 + nj1) * ji;
  for (int c = 0; c < 2; ++c) {
    if (T.jobs[c].empty()) continue;
    EpisodeForkArgs a;
    a.cache = cache[c]; a.jobs = reinterpret_cast<const ForkJob*>(dev + (c ? nj0 * ji : 0)); a.dsts = ddst;
    a.n_jobs = (int)T.jobs[c].size(); a.units = T.units[c]; a.NL = NL; a.B = B; a.L = L[c]; a.N = N;
    OTHER(R, launch_episode_fork(a, is_bf16, R.st), "episode_fork");
  }
  if (mask) OTHER(R, launch_episode_fork_state(ddst, ddst + np, (int)np, mask, poscnt, fresh, Lmax, R.st), "episode_fork_state");
  return R.err;
}

// vima_decode_fork / vima_seq_decode_fork behind check_ready; family: the entry's refusal of a handle of the other family, which comes first
static int fork_episode(VimaHandle* h, const char* fn, bool seq, const int32_t* source, int B, hipStream_t st, const char* family) {
  if (!source && ep_seq(h) == seq) return fail(std::string(fn) + ": null argument");
  if (int e = ep_running(h, fn, seq, B, kAny, !seq, " with this B", family)) return e;
  const std::vector<int> src(source, source + B);
  if (!h->ep.book.fork_ok(src)) {
    for (int b = 0; b < B; ++b) {
      const int s = src[(size_t)b];
      if (s < 0 || s >= B) return fail(std::string(fn) + ": source[" + std::to_string(b) + "] = " + std::to_string(s) + " is not a sample of the batch [0, " + std::to_string(B) + ")", 22);
      if (src[(size_t)s] != s)
        return fail(std::string(fn) + ": source[" + std::to_string(b) + "] = " + std::to_string(s) + " is itself a destination (source[" + std::to_string(s) + "] = " +
                    std::to_string(src[(size_t)s]) + "): a source must be its own source, no chains and no swaps", 22);
    }
  }
  const int E = h->cfg.embed_dim, NL = h->cfg.xf_n_layers, Lmax = h->ep.Lmax, Lp = h->ep.Lp;
  if (((size_t)2 * E * h->esz()) % 16) return fail(std::string(fn) + ": rows of 2 x embed_dim elements must be a multiple of 16 bytes", 22);
  const long long rv = (long long)2 * E * (long long)h->esz() / 16;
  std::vector<int> dsts, srcs;
  ForkTable T;
  for (int s = 0; s < B; ++s) {   // groups in increasing source order
    ForkGroup g{s, (int)dsts.size(), 0};
    for (int b = 0; b < B; ++b)
      if (src[(size_t)b] == s && b != s) { dsts.push_back(b); srcs.push_back(s); ++g.ndst; }
    if (!g.ndst) continue;
    int rg[2][2];
    const int nr = h->ep.book.live_ranges(s, rg);
    if (seq) T.add(0, g, 0, h->ep.book.P0, rv);          // the fixed prefix [prompt | sep]
    for (int i = 0; i < nr; ++i) T.add(0, g, rg[i][0], rg[i][1], rv);
    if (!seq) T.add(1, g, 0, Lp, rv);                 // the sample's block of the prompt K / V cache, either layout
  }
  if (dsts.empty()) return 0;
  Run R{h, st};
  void* const cache[2] = {h->ep.kv, h->pkv.ptr};
  const int L[2] = {Lmax, Lp};
  if (fork_launch(R, T, dsts, srcs, cache, L, NL, B, 2 * E, h->bf16, h->ep.mask, h->ep.poscnt, h->ep.fresh, Lmax)) return R.err;
  h->ep.book.fork(src);
  return 0;
}

int vima_decode_fork(VimaHandle* h, const int32_t* source, int B, vima_stream_t stream) {
  if (int e = check_ready(h)) return e;
  return fork_episode(h, "vima_decode_fork", false, source, B, (hipStream_t)stream,
                      "the handle's policy has no XAttnGPT episode caches (GPT / GATO handles fork with vima_seq_decode_fork)");
}

int vima_seq_decode_fork(VimaHandle* h, const int32_t* source, int B, vima_stream_t stream) {
  if (int e = check_ready(h)) return e;
  return fork_episode(h, "vima_seq_decode_fork", true, source, B, (hipStream_t)stream,
                      "decoder-only policies (GPT / GATO) only; VIMAPolicy / VIMAFlamingoPolicy handles fork with vima_decode_fork");
}

int vima_op_episode_fork(VimaHandle* h, void* cache, int elem_bytes, int NL, int B, int L, int N, const int32_t* group_src, const int32_t* group_ptr,
                         const int32_t* dsts, const int32_t* range_ptr, const int32_t* ranges, int n_groups, vima_stream_t stream) {
  const char* fn = "vima_op_episode_fork";
  if (int e = op_begin(h, fn)) return e;
  OP_REQ(cache && group_src && group_ptr && dsts && range_ptr && ranges, "null argument");
  OP_REQ(elem_bytes == 2 || elem_bytes == 4, "elem_bytes must be 4 (fp32) or 2 (bf16)");
  OP_REQ(NL > 0 && B > 0 && L > 0 && N > 0 && n_groups >= 0, "NL, B, L and N must be positive");
  if (((long long)N * elem_bytes) % 16 || ((uintptr_t)cache & 15))
    return fail(std::string(fn) + ": rows of N elements must be a multiple of 16 bytes and the cache 16-byte aligned", 22);
  const long long rv = (long long)N * elem_bytes / 16;
  std::vector<int> role((size_t)B, 0), d, s;   // 1 = source, 2 = destination
  ForkTable T;
  OP_REQ(group_ptr[0] == 0 && range_ptr[0] == 0, "group_ptr and range_ptr start at 0");
  for (int g = 0; g < n_groups; ++g) {
    const int sb = group_src[g];
    OP_REQ(sb >= 0 && sb < B, "a source is not a sample of the cache");
    OP_REQ(role[(size_t)sb] == 0, "a source is listed twice or is a destination");
    OP_REQ(group_ptr[g + 1] >= group_ptr[g] && range_ptr[g + 1] >= range_ptr[g], "group_ptr and range_ptr must not decrease");
    role[(size_t)sb] = 1;
    ForkGroup G{sb, (int)d.size(), group_ptr[g + 1] - group_ptr[g]};
    for (int i = group_ptr[g]; i < group_ptr[g + 1]; ++i) {
      OP_REQ(dsts[i] >= 0 && dsts[i] < B && role[(size_t)dsts[i]] == 0, "a destination is not a sample of the cache, is listed twice or is a source");
      role[(size_t)dsts[i]] = 2;
      d.push_back(dsts[i]); s.push_back(sb);
    }
    for (int i = range_ptr[g]; i < range_ptr[g + 1]; ++i) {
      OP_REQ(ranges[2 * i] >= 0 && ranges[2 * i] <= ranges[2 * i + 1] && ranges[2 * i + 1] <= L, "a range must be 0 <= row0 <= row1 <= L");
      T.add(0, G, ranges[2 * i], ranges[2 * i + 1], rv);
    }
  }
  if (T.jobs[0].empty()) return 0;
  Run R{h, (hipStream_t)stream};
  void* const caches[2] = {cache, nullptr};
  const int Ls[2] = {L, 0};
  return fork_launch(R, T, d, s, caches, Ls, NL, B, N, elem_bytes == 2, nullptr, nullptr, nullptr, 0);
}

// ---- episode snapshots (episode_snapshot.hip) -------------------------------------------------------------------------------------
// The host side of one snapshot / restore call, kept in the handle (snap_table: the source of the ONE upload): [jobs of cache 0 | jobs of cache 1 |
// state jobs | row map]. Cache 0 is the episode K | V cache under the call's row map, cache 1 the prompt K / V cache under the identity.
namespace {
struct SnapTable {
  std::vector<SnapJob> jobs[2];
  int units[2] = {0, 0};
  std::vector<SnapStateJob> state;
  std::vector<int> map;
  void add(int c, const void* payload, long long layer_stride, int sample, int map0, int nrows, int rpc) {
    if (nrows <= 0) return;
    jobs[c].push_back(SnapJob{(long long)(uintptr_t)payload, layer_stride, sample, map0, nrows, units[c]});
    units[c] += (nrows + rpc - 1) / rpc;
  }
};
struct SnapCache { void* cache; int L, D; bool mapped; };
// byte offsets of the payload's sections (include/vima_hip.h)
struct SnapLayout { long long mask, rows, prompt, bytes, row_bytes; int R, npre; bool has_prompt; };
SnapLayout snap_layout(const VimaEpisodeSnapshotInfo& I, bool seq) {
  SnapLayout s{};
  const long long R = std::max<long long>((long long)I.steps * (I.Q + 1) - 1, 0);
  s.has_prompt = (I.flags & VIMA_SNAPSHOT_PROMPT) != 0;
  s.R = (int)R;
  s.npre = seq && s.has_prompt ? I.prompt_len : 0;
  s.row_bytes = (long long)2 * I.embed_dim * I.elem_bytes;
  s.mask = 16;
  s.rows = s.mask + (s.npre + R + 15) / 16 * 16;
  s.prompt = s.rows + (long long)I.layers * R * s.row_bytes;
  s.bytes = s.prompt + (s.has_prompt ? (long long)I.layers * I.prompt_len * s.row_bytes : 0);
  return s;
}
// a payload must be DEVICE memory: a kernel is never handed a pageable or unregistered host address
int snap_device_ptr(const std::string& fn, const void* p, long long bytes, int i) {
  const std::string what = fn + ": payload " + std::to_string(i);
  if (!p) return fail(what + " is null", 22);
  if (reinterpret_cast<uintptr_t>(p) & 15) return fail(what + " is not 16-byte aligned", 22);
  hipPointerAttribute_t pa{};
  if (hipPointerGetAttributes(&pa, p) != hipSuccess) {
    (void)hipGetLastError();
    return fail(what + " is not device memory (hipPointerGetAttributes does not know the address)", 22);
  }
  if (pa.type != hipMemoryTypeDevice) return fail(what + " is not device memory (host and managed addresses are refused)", 22);
  hipDeviceptr_t base = nullptr;
  size_t size = 0;
  if (hipMemGetAddressRange(&base, &size, const_cast<void*>(p)) == hipSuccess) {
    if (reinterpret_cast<const char*>(p) + bytes > reinterpret_cast<const char*>(base) + size)
      return fail(what + " is shorter than the " + std::to_string(bytes) + " bytes the call moves", 22);
  } else {
    (void)hipGetLastError();
  }
  return 0;
}
}  // namespace

// uploads the table and launches: per cache with jobs one pack / unpack launch, then (mask given) the per-pair state -- at most 3 launches
static int snap_launch(Run& R, const SnapTable& T, bool pack, const SnapCache c[2], int NL, int B, int N, bool is_bf16, uint8_t* mask, int* poscnt,
                       uint8_t* fresh, int Lmax, int lo, int hi) {
  VimaHandle* h = R.h;
  static_assert(sizeof(SnapJob) == 32 && sizeof(SnapStateJob) == 24, "the table is laid out in 8-byte words");
  const size_t nj0 = T.jobs[0].size(), nj1 = T.jobs[1].size(), ns = T.state.size(), nm = T.map.size();
  const size_t o1 = nj0 * 4, os = o1 + nj1 * 4, om = os + ns * 3, words = om + (nm + 1) / 2;
  if (words == 0) return 0;
  std::vector<long long>& tab = h->snap_table;
  tab.assign(words, 0);
  if (nj0) memcpy(tab.data(), T.jobs[0].data(), nj0 * sizeof(SnapJob));
  if (nj1) memcpy(tab.data() + o1, T.jobs[1].data(), nj1 * sizeof(SnapJob));
  if (ns) memcpy(tab.data() + os, T.state.data(), ns * sizeof(SnapStateJob));
  if (nm) memcpy(tab.data() + om, T.map.data(), nm * sizeof(int));
  long long* dev = R.ws<long long>(words);
  if (R.upload(dev, tab)) return R.err;
  const int* dmap = reinterpret_cast<const int*>(dev + om);
  const int rpc = snap_rows_per_unit((long long)N * (is_bf16 ? 2 : 4) / 16);
  for (int i = 0; i < 2; ++i) {
    if (T.jobs[i].empty()) continue;
    EpisodeSnapArgs a;
    a.cache = c[i].cache; a.jobs = reinterpret_cast<const SnapJob*>(dev + (i ? o1 : 0)); a.map = c[i].mapped ? dmap : nullptr;
    a.n_jobs = (int)T.jobs[i].size(); a.units = T.units[i]; a.NL = NL; a.B = B; a.L = c[i].L; a.N = N; a.D = c[i].D; a.rpc = rpc;
    if (pack) OTHER(R, launch_episode_pack(a, is_bf16, R.st), "episode_pack");
    else OTHER(R, launch_episode_unpack(a, is_bf16, R.st), "episode_unpack");
  }
  if (mask && ns) {
    const SnapStateJob* sj = reinterpret_cast<const SnapStateJob*>(dev + os);
    if (pack) OTHER(R, launch_episode_pack_state(sj, (int)ns, dmap, mask, poscnt, fresh, Lmax, R.st), "episode_pack_state");
    else OTHER(R, launch_episode_unpack_state(sj, (int)ns, dmap, mask, poscnt, fresh, Lmax, lo, hi, R.st), "episode_unpack_state");
  }
  return R.err;
}

// the policy and running-batch checks of the six entry points
static int snap_ready(VimaHandle* h, const std::string& fn, bool seq) {
  if (int e = seq ? seq_ready(h, fn.c_str()) : check_ready(h)) return e;
  if (int e = ep_running(h, fn.c_str(), seq, kAny, kAny, !seq, "", "the handle's policy has no XAttnGPT episode caches (GPT / GATO handles use the vima_seq_decode_* form)"))
    return e;
  if (((size_t)2 * h->cfg.embed_dim * h->esz()) % 16) return fail(fn + ": rows of 2 x embed_dim elements must be a multiple of 16 bytes", 22);
  if (!seq && h->pkv.hm && ((size_t)(h->cfg.embed_dim / h->cfg.xattn_n_heads) * h->esz()) % 16)
    return fail(fn + ": head-major prompt K / V pieces must be a multiple of 16 bytes", 22);
  return 0;
}

static VimaEpisodeSnapshotInfo snap_info(const VimaHandle* h, bool seq, int steps, bool with_prompt) {
  VimaEpisodeSnapshotInfo I{};
  I.steps = steps; I.Q = h->ep.Q; I.embed_dim = h->cfg.embed_dim; I.layers = h->cfg.xf_n_layers;
  I.prompt_len = seq ? h->ep.book.P0 : h->ep.Lp; I.elem_bytes = (int)h->esz();
  I.flags = with_prompt ? VIMA_SNAPSHOT_PROMPT : 0; I.policy_kind = h->cfg.policy_kind;
  I.bytes = snap_layout(I, seq).bytes;
  return I;
}

// fills infos[i] for samples[i]; refuses a sample outside the batch (22) or whose age no suffix of the slot record sums to (internal error)
static int snap_infos(VimaHandle* h, const std::string& fn, bool seq, const int32_t* samples, int n, int with_prompt, VimaEpisodeSnapshotInfo* infos) {
  if (!samples || !infos || n < 0) return fail(fn + ": null argument");
  for (int i = 0; i < n; ++i) {
    const int b = samples[i];
    if (b < 0 || b >= h->ep.B) return fail(fn + ": sample " + std::to_string(b) + " is not a sample of the batch [0, " + std::to_string(h->ep.B) + ")", 22);
    const int steps = h->ep.book.steps_of(b);
    if (steps < 0 || steps > h->ep.book.room())
      return fail(fn + ": internal error: no run of the last batch steps adds up to the age of sample " + std::to_string(b));
    infos[i] = snap_info(h, seq, steps, with_prompt != 0);
  }
  return 0;
}

// row table of a call whose longest episode has nmax steps (at most the room: snap_infos, snap_restore): [identity over the prefix (seq) |
// history_rows(nmax)]
static int snap_rowmap(VimaHandle* h, const std::string& fn, int nmax, std::vector<int>& map) {
  EpisodeBook::History H = h->ep.book.history(nmax, true);
  if (!H.fits || !H.in_range) return fail(fn + ": internal error: episode row outside the cache");
  map = std::move(H.rows);
  return 0;
}

static int snap_take(VimaHandle* h, const std::string& fn, bool seq, const int32_t* samples, int n, int with_prompt, void* const* payloads,
                     const int64_t* capacity, VimaEpisodeSnapshotInfo* infos, hipStream_t st) {
  if (int e = snap_ready(h, fn, seq)) return e;
  if (!payloads || !capacity) return fail(fn + ": null argument");
  std::vector<VimaEpisodeSnapshotInfo> I((size_t)std::max(n, 0));
  if (int e = snap_infos(h, fn, seq, samples, n, with_prompt, I.data())) return e;
  if (n == 0) return 0;
  int nmax = 0;
  for (int i = 0; i < n; ++i) {
    nmax = std::max(nmax, I[(size_t)i].steps);
    if (capacity[i] < I[(size_t)i].bytes)
      return fail(fn + ": payload " + std::to_string(i) + " has room for " + std::to_string(capacity[i]) + " bytes, the snapshot takes " +
                  std::to_string(I[(size_t)i].bytes), 22);
    if (int e = snap_device_ptr(fn, payloads[i], I[(size_t)i].bytes, i)) return e;
    for (int j = 0; j < i; ++j)
      if (payloads[j] == payloads[i]) return fail(fn + ": payloads " + std::to_string(j) + " and " + std::to_string(i) + " are the same buffer", 22);
  }
  SnapTable T;
  if (int e = snap_rowmap(h, fn, nmax, T.map)) return e;
  const int E = h->cfg.embed_dim, NL = h->cfg.xf_n_layers, Lmax = h->ep.Lmax, B = h->ep.B;
  const int rpc = snap_rows_per_unit((long long)2 * E * (long long)h->esz() / 16), total = (int)T.map.size();
  for (int i = 0; i < n; ++i) {
    const SnapLayout s = snap_layout(I[(size_t)i], seq);
    char* p = static_cast<char*>(payloads[i]);
    T.add(0, p + s.rows, (long long)s.R * s.row_bytes, samples[i], total - s.R, s.R, rpc);
    if (s.has_prompt) T.add(seq ? 0 : 1, p + s.prompt, (long long)I[(size_t)i].prompt_len * s.row_bytes, samples[i], 0, I[(size_t)i].prompt_len, rpc);
    T.state.push_back(SnapStateJob{(long long)(uintptr_t)p, samples[i], total - s.R, s.R, s.npre});
  }
  Run R{h, st};
  const SnapCache c[2] = {{h->ep.kv, Lmax, 0, true}, {h->pkv.ptr, h->ep.Lp, h->pkv.hm ? E / h->cfg.xattn_n_heads : 0, false}};
  if (snap_launch(R, T, true, c, NL, B, 2 * E, h->bf16, h->ep.mask, h->ep.poscnt, h->ep.fresh, Lmax, 0, 0)) return R.err;
  for (int i = 0; i < n; ++i) infos[i] = I[(size_t)i];
  return 0;
}

static int snap_restore(VimaHandle* h, const std::string& fn, bool seq, const int32_t* slots, int n, const void* const* payloads,
                        const VimaEpisodeSnapshotInfo* infos, hipStream_t st) {
  if (int e = snap_ready(h, fn, seq)) return e;
  if (!slots || !payloads || !infos || n < 0) return fail(fn + ": null argument");
  if (n == 0) return 0;
  const int B = h->ep.B;
  std::vector<int> ages((size_t)n);
  int nmax = 0;
  for (int i = 0; i < n; ++i) {
    const VimaEpisodeSnapshotInfo& I = infos[i];
    const std::string who = fn + ": snapshot " + std::to_string(i);
    if (slots[i] < 0 || slots[i] >= B) return fail(fn + ": slot " + std::to_string(slots[i]) + " is not a sample of the batch [0, " + std::to_string(B) + ")", 22);
    for (int j = 0; j < i; ++j)
      if (slots[j] == slots[i]) return fail(fn + ": slot " + std::to_string(slots[i]) + " is listed twice", 22);
    const VimaEpisodeSnapshotInfo want = snap_info(h, seq, I.steps, (I.flags & VIMA_SNAPSHOT_PROMPT) != 0);
    if (I.policy_kind != want.policy_kind) return fail(who + " was taken from another policy kind", 22);
    if (I.embed_dim != want.embed_dim || I.layers != want.layers)
      return fail(who + " has embed_dim " + std::to_string(I.embed_dim) + " and " + std::to_string(I.layers) + " layers, the handle " +
                  std::to_string(want.embed_dim) + " and " + std::to_string(want.layers), 22);
    if (I.elem_bytes != want.elem_bytes)
      return fail(who + " holds " + std::to_string(I.elem_bytes) + "-byte elements, the handle's caches " + std::to_string(want.elem_bytes) + "-byte (precision)", 22);
    if (I.Q != want.Q) return fail(who + " has Q = " + std::to_string(I.Q) + ", the running batch Q = " + std::to_string(want.Q), 22);
    if (I.prompt_len != want.prompt_len)
      return fail(who + " has a prompt of " + std::to_string(I.prompt_len) + " rows, the running batch " + std::to_string(want.prompt_len) + " (Lp)", 22);
    if (I.steps < 0 || (I.flags & ~VIMA_SNAPSHOT_PROMPT) || I.bytes != want.bytes) return fail(who + ": the info is not one this library wrote", 22);
    const EpisodeBook::History H = h->ep.book.history(I.steps, false);
    if (!H.fits) return room_refused(who + " holds " + std::to_string(I.steps) + " steps and", H.room);
    ages[(size_t)i] = H.age;
    if (int e = snap_device_ptr(fn, payloads[i], I.bytes, i)) return e;
    nmax = std::max(nmax, I.steps);
  }
  SnapTable T;
  if (int e = snap_rowmap(h, fn, nmax, T.map)) return e;
  const int E = h->cfg.embed_dim, NL = h->cfg.xf_n_layers, Lmax = h->ep.Lmax, P0 = seq ? h->ep.book.P0 : 0;
  const int rpc = snap_rows_per_unit((long long)2 * E * (long long)h->esz() / 16), total = (int)T.map.size();
  for (int i = 0; i < n; ++i) {
    const SnapLayout s = snap_layout(infos[i], seq);
    const char* p = static_cast<const char*>(payloads[i]);
    T.add(0, p + s.rows, (long long)s.R * s.row_bytes, slots[i], total - s.R, s.R, rpc);
    if (s.has_prompt) T.add(seq ? 0 : 1, p + s.prompt, (long long)infos[i].prompt_len * s.row_bytes, slots[i], 0, infos[i].prompt_len, rpc);
    T.state.push_back(SnapStateJob{(long long)(uintptr_t)p, slots[i], total - s.R, s.R, s.npre});
  }
  Run R{h, st};
  const SnapCache c[2] = {{h->ep.kv, Lmax, 0, true}, {h->pkv.ptr, h->ep.Lp, h->pkv.hm ? E / h->cfg.xattn_n_heads : 0, false}};
  // the restart of the slot: its old episode's keys are masked -- everywhere behind the prefix (the ring's written part; rows beyond it are never read)
  if (snap_launch(R, T, false, c, NL, B, 2 * E, h->bf16, h->ep.mask, h->ep.poscnt, h->ep.fresh, Lmax, P0, seq ? h->ep.book.written_end() : Lmax)) return R.err;
  for (int i = 0; i < n; ++i) h->ep.book.install(std::vector<int>{slots[i]}, ages[(size_t)i]);
  return 0;
}

int vima_decode_snapshot_size(VimaHandle* h, const int32_t* samples, int n, int with_prompt, VimaEpisodeSnapshotInfo* infos) {
  if (int e = snap_ready(h, "vima_decode_snapshot_size", false)) return e;
  return snap_infos(h, "vima_decode_snapshot_size", false, samples, n, with_prompt, infos);
}

int vima_decode_snapshot(VimaHandle* h, const int32_t* samples, int n, int with_prompt, void* const* payloads, const int64_t* capacity,
                         VimaEpisodeSnapshotInfo* infos, vima_stream_t stream) {
  return snap_take(h, "vima_decode_snapshot", false, samples, n, with_prompt, payloads, capacity, infos, (hipStream_t)stream);
}

int vima_decode_restore(VimaHandle* h, const int32_t* slots, int n, const void* const* payloads, const VimaEpisodeSnapshotInfo* infos,
                        vima_stream_t stream) {
  return snap_restore(h, "vima_decode_restore", false, slots, n, payloads, infos, (hipStream_t)stream);
}

int vima_seq_decode_snapshot_size(VimaHandle* h, const int32_t* samples, int n, int with_prompt, VimaEpisodeSnapshotInfo* infos) {
  if (int e = snap_ready(h, "vima_seq_decode_snapshot_size", true)) return e;
  return snap_infos(h, "vima_seq_decode_snapshot_size", true, samples, n, with_prompt, infos);
}

int vima_seq_decode_snapshot(VimaHandle* h, const int32_t* samples, int n, int with_prompt, void* const* payloads, const int64_t* capacity,
                             VimaEpisodeSnapshotInfo* infos, vima_stream_t stream) {
  return snap_take(h, "vima_seq_decode_snapshot", true, samples, n, with_prompt, payloads, capacity, infos, (hipStream_t)stream);
}

int vima_seq_decode_restore(VimaHandle* h, const int32_t* slots, int n, const void* const* payloads, const VimaEpisodeSnapshotInfo* infos,
                            vima_stream_t stream) {
  return snap_restore(h, "vima_seq_decode_restore", true, slots, n, payloads, infos, (hipStream_t)stream);
}

// vima_op_episode_pack / vima_op_episode_unpack behind one body
static int op_episode_snap(VimaHandle* h, const char* fn, bool pack, void* cache, int elem_bytes, int NL, int B, int L, int N, int D,
                           const int32_t* rowmap, int n_map, const int32_t* samples, const int32_t* nrows, const void* const* payloads, int n_jobs,
                           hipStream_t st) {
  if (int e = op_begin(h, fn)) return e;
  OP_REQ(cache && samples && nrows && payloads, "null argument");
  OP_REQ(elem_bytes == 2 || elem_bytes == 4, "elem_bytes must be 4 (fp32) or 2 (bf16)");
  OP_REQ(NL > 0 && B > 0 && L > 0 && N > 0 && D >= 0 && n_map >= 0 && n_jobs >= 0, "NL, B, L and N must be positive, D, n_map and n_jobs not negative");
  if (((long long)N * elem_bytes) % 16 || ((uintptr_t)cache & 15))
    return fail(std::string(fn) + ": rows of N elements must be a multiple of 16 bytes and the cache 16-byte aligned", 22);
  if (D > 0 && (((long long)D * elem_bytes) % 16 || N % D))
    return fail(std::string(fn) + ": head-major pieces of D elements must be a multiple of 16 bytes and divide N", 22);
  OP_REQ(rowmap || n_map <= L, "the identity map holds at most L rows");
  SnapTable T;
  for (int l = 0; l < n_map && rowmap; ++l) {
    if (rowmap[l] < 0 || rowmap[l] >= L) return fail(std::string(fn) + ": rowmap[" + std::to_string(l) + "] = " + std::to_string(rowmap[l]) + " is not a row of the cache [0, " + std::to_string(L) + ")", 22);
    T.map.push_back(rowmap[l]);
  }
  const long long row_bytes = (long long)N * elem_bytes;
  const int rpc = snap_rows_per_unit(row_bytes / 16);
  std::vector<char> seen((size_t)B, 0);
  for (int j = 0; j < n_jobs; ++j) {
    OP_REQ(samples[j] >= 0 && samples[j] < B, "a sample is not a sample of the cache");
    OP_REQ(nrows[j] >= 0 && nrows[j] <= n_map, "a job moves at most n_map rows");
    if (!pack) {
      if (seen[(size_t)samples[j]]) return fail(std::string(fn) + ": sample " + std::to_string(samples[j]) + " is listed twice", 22);
      seen[(size_t)samples[j]] = 1;
    }
    if (nrows[j] == 0) continue;
    if (int e = snap_device_ptr(fn, payloads[j], (long long)NL * nrows[j] * row_bytes, j)) return e;
    T.add(0, payloads[j], (long long)nrows[j] * row_bytes, samples[j], n_map - nrows[j], nrows[j], rpc);
  }
  if (T.jobs[0].empty()) return 0;
  if (int e = snap_device_ptr(std::string(fn) + " (cache)", cache, (long long)NL * B * L * row_bytes, 0)) return e;
  Run R{h, st};
  const SnapCache c[2] = {{cache, L, D, rowmap != nullptr}, {nullptr, 0, 0, false}};
  return snap_launch(R, T, pack, c, NL, B, N, elem_bytes == 2, nullptr, nullptr, nullptr, 0, 0, 0);
}

int vima_op_episode_pack(VimaHandle* h, const void* cache, int elem_bytes, int NL, int B, int L, int N, int D, const int32_t* rowmap, int n_map,
                         const int32_t* samples, const int32_t* nrows, void* const* payloads, int n_jobs, vima_stream_t stream) {
  return op_episode_snap(h, "vima_op_episode_pack", true, const_cast<void*>(cache), elem_bytes, NL, B, L, N, D, rowmap, n_map, samples, nrows,
                         const_cast<const void* const*>(payloads), n_jobs, (hipStream_t)stream);
}

int vima_op_episode_unpack(VimaHandle* h, void* cache, int elem_bytes, int NL, int B, int L, int N, int D, const int32_t* rowmap, int n_map,
                           const int32_t* samples, const int32_t* nrows, const void* const* payloads, int n_jobs, vima_stream_t stream) {
  return op_episode_snap(h, "vima_op_episode_unpack", false, cache, elem_bytes, NL, B, L, N, D, rowmap, n_map, samples, nrows, payloads, n_jobs,
                         (hipStream_t)stream);
}
#undef OP_REQ

}  // extern "C"
