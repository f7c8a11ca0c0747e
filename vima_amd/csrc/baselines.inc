// Baseline policies of the reference (SURVEY.md 8(f) row 4) on the kernels of the VIMA hot path. Included by vima_api.hip
// (inside its anonymous namespace: uses Run, VimaHandle, OTHER, t5_stack). Not performance-tuned like the VIMAPolicy path:
// one chunk, no stream overlap, fp32 decoder stream (round 6: the ViT's stream in the operand type and its attention on the register kernel) -- the arithmetic is the
// same GEMM / attention / LayerNorm kernels.
//
//   rgb_vit          (Gato)ViTEncoder(Rectangular).forward   vit.py:49-81, 239-268  -> (Gato)VisionTransformerRectangular :119-135, :305-329
//   rgb_obj_encode   MultiViewRGBEncoder / GatoMultiViewRGBEncoder / MultiViewRGBPerceiverEncoder .forward   obj_encoder.py:123-139, 195-204, 232-240
//   perceiver        PerceiverEncoder.forward                modeling_perceiver.py:468-527 (transformers; not under /root/reference)
//   seq_decode       VIMAGPTPolicy.forward / VIMAGatoPolicy.forward -> HFGPT.forward   vima_gpt_policy.py:118-187, gpt/gpt.py:45-80

constexpr int kRgbH = 64, kRgbW = 128, kRgbPatch = 32;

int rgb_tokens_per_image(int kind) { return kind == VIMA_POLICY_GPT ? 1 : (kind == VIMA_POLICY_GATO ? 16 : 4); }

// ViT over M frames (both views stacked: rows [0, per_view) front, [per_view, 2 per_view) top). Returns ln_post'ed rows in
// the operand type: yT [M * S, 768] (Gato / Flamingo: every token) or [M, 768] (GPT: cls token).
int rgb_vit(Run& R, const uint8_t* const rgb[2], int per_view, void** y_out) {
  VimaHandle* h = R.h;
  const int M = 2 * per_view, S = h->vit_S, NP = h->vit_patches;
  const int Kc = 3 * kRgbPatch * kRgbPatch;
  const bool cls = h->vit.cls != nullptr;
  void* P = R.wsT((size_t)M * NP * Kc);
  float* pre = R.ws<float>((size_t)M * NP * kVitW);
  const bool sT = h->stream_T != 0;   // the ViT's residual stream in the operand type (bf16: 4 instead of 10 bytes of HBM traffic per element and residual GEMM), like vit_chunk
  float* x = sT ? nullptr : R.ws<float>((size_t)M * S * kVitW);
  void* xT = sT ? R.wsT((size_t)M * S * kVitW) : nullptr;
  void* hT = R.wsT((size_t)M * S * kVitW);
  void* qkv = R.wsT((size_t)M * S * 3 * kVitW);
  void* att = R.wsT((size_t)M * S * kVitW);
  void* u = R.wsT((size_t)M * S * 4 * kVitW);
  void* y = R.wsT((size_t)M * S * kVitW);
  if (R.err) return R.err;
  for (int vi = 0; vi < 2; ++vi)
    OTHER(R, launch_patchify_rect(rgb[vi], R.offT(P, (long long)vi * per_view * NP * Kc), per_view, kRgbH, kRgbW, kRgbPatch, h->bf16, R.st),
          "patchify_rect");
  R.linear(P, Kc, h->vit.conv, M * NP, ACT_NONE, nullptr, 0, nullptr, 0, pre, kVitW, nullptr, 0);           // conv1 (vit.py:120, :306)
  OTHER(R, launch_vit_embed_rect(pre, h->vit.cls, h->vit.pos, h->vit.lnpre_g, h->vit.lnpre_b, x, xT, M, S, NP, h->bf16, R.st),
        "vit_embed_rect");
  // the blocks of the object-crop ViT over the S (8 or 9) tokens of a frame (rounds 1-5 ran the exact generic attention kernel here: 261 us per launch for 191 MB of q|k|v)
  VitBuf vb{P, pre, x, hT, qkv, att, u, y, xT, nullptr};
  for (int j = 0; j < kVitLayers; ++j) {
    vit_block(R, h->vit.blk[j], M, S, vb, false, nullptr, nullptr);
    if (R.err) return R.err;
  }
  const long long ldp = cls ? (long long)S * kVitW : kVitW;   // x[:, 0, :] (vit.py:326) / every token (vit.py:132)
  if (sT) R.lnT(xT, ldp, h->vit.lnpost_g, h->vit.lnpost_b, 1e-5f, 0, cls ? M : M * S, kVitW, nullptr, y);
  else R.ln(x, ldp, h->vit.lnpost_g, h->vit.lnpost_b, 1e-5f, 0, cls ? M : M * S, kVitW, nullptr, y);
  *y_out = y;
  return R.err;
}

// One PerceiverLayer (modeling_perceiver.py:383-415): z fp32 [n*Lz, E] is updated in place. inputsT == nullptr: self-attention.
int perceiver_layer(Run& R, const VimaHandle::PercLayer& L, float* z, int n, int Lz, const float* inputs32, int Lin) {
  VimaHandle* h = R.h;
  const int E = h->cfg.embed_dim, H = 8, D = E / H;
  const int rz = n * Lz, rk = inputs32 ? n * Lin : rz;
  void* hq = R.wsT((size_t)rz * E);
  void* hk = inputs32 ? R.wsT((size_t)rk * E) : hq;
  void* q = R.wsT((size_t)rz * E);
  void* kv = R.wsT((size_t)rk * 2 * E);
  void* ctx = R.wsT((size_t)rz * E);
  float* att = R.ws<float>((size_t)rz * E);
  void* m = R.wsT((size_t)rz * E);
  void* m1 = R.wsT((size_t)rz * E);
  if (R.err) return R.err;
  R.ln(z, E, L.ln1g, L.ln1b, 1e-5f, 0, rz, E, nullptr, hq);                       // layernorm1(hidden_states)  (:192)
  if (inputs32) R.ln(inputs32, E, L.ln2g, L.ln2b, 1e-5f, 0, rk, E, nullptr, hk);   // layernorm2(inputs)         (:193)
  R.linear(hq, E, L.q, rz, ACT_NONE, nullptr, 0, nullptr, 0, nullptr, 0, q, E);
  R.linear(hk, E, L.kv, rk, ACT_NONE, nullptr, 0, nullptr, 0, nullptr, 0, kv, 2 * E);
  AttnArgs a;   // softmax(q k^T / sqrt(d)) v, all inputs valid (obj_encoder.py:199-202 passes a mask of ones)
  a.q = q; a.ldq = E; a.k = kv; a.ldk = 2 * E; a.v = R.offT(kv, E); a.ldv = 2 * E; a.out = ctx; a.ldo = E;
  a.B = n; a.H = H; a.Lq = Lz; a.Lk = inputs32 ? Lin : Lz; a.D = D; a.scale = 1.0f / sqrtf((float)D); a.mode = ATTN_CROSS;
  R.attn(a, 0);
  R.linear(ctx, E, L.o, rz, ACT_NONE, nullptr, 0, z, E, att, E, nullptr, 0);       // output dense + query residual (:322-330)
  R.ln(att, E, L.lng, L.lnb, 1e-5f, 0, rz, E, nullptr, m);                         // MLP on layernorm(attention_output) (:412-415)
  R.linear(m, E, L.d1, rz, ACT_GELU, nullptr, 0, nullptr, 0, nullptr, 0, m1, E);
  R.linear(m1, E, L.d2, rz, ACT_NONE, nullptr, 0, att, E, z, E, nullptr, 0);       // + attention_output (:408)
  return R.err;
}

// obj_encoder.forward of the handle's policy: rgb[v] u8 [n,3,64,128] -> out32 [n, Q, Eo] fp32 and / or outT (operand type)
int rgb_obj_encode(Run& R, const uint8_t* const rgb[2], int n, float* out32, void* outT) {
  VimaHandle* h = R.h;
  const int E = h->cfg.embed_dim, kind = h->cfg.policy_kind;
  if (n <= 0) return 0;
  void* y = nullptr;
  if (rgb_vit(R, rgb, n, &y)) return R.err;
  if (kind == VIMA_POLICY_GPT) {
    // cls feature @ projection per view, concatenated on the FEATURE axis: out[i, v*E:(v+1)*E] (obj_encoder.py:237-240)
    for (int vi = 0; vi < 2; ++vi) {
      GemmArgs g;
      g.A = R.offT(y, (long long)vi * n * kVitW); g.lda = kVitW; R.setW(g, h->vit.projection); g.M = n; g.N = E; g.K = kVitW;
      if (out32) { g.out32 = out32 + (size_t)vi * E; g.ld32 = 2 * E; }
      if (outT) { g.outT = R.offT(outT, (long long)vi * E); g.ldT = 2 * E; }
      R.gemm(g);
    }
    return R.err;
  }
  // Gato / Flamingo: every patch token @ projection, views concatenated on the TOKEN axis: row i*16 + v*8 + t (obj_encoder.py:134-138)
  const int NP = h->vit_patches;
  float* tok32 = kind == VIMA_POLICY_GATO ? out32 : R.ws<float>((size_t)n * 2 * NP * E);
  void* tokT = kind == VIMA_POLICY_GATO ? outT : nullptr;
  if (R.err) return R.err;
  for (int vi = 0; vi < 2; ++vi) {
    GemmArgs g;
    g.A = R.offT(y, (long long)vi * n * NP * kVitW); g.lda = kVitW; R.setW(g, h->vit.projection); g.M = n * NP; g.N = E; g.K = kVitW;
    g.out32 = tok32; g.ld32 = E; g.outT = tokT; g.ldT = E;
    g.rb = NP; g.s_hi = 2 * NP; g.s_lo = 1; g.ro = vi * NP;
    R.gemm(g);
  }
  if (kind == VIMA_POLICY_GATO) return R.err;
  // Flamingo: Perceiver resampler (obj_encoder.py:195-204): latents [4,E] expanded over the frames, one cross-attention onto
  // the 16 patch tokens, then 4 blocks of the SAME 4 self-attention layers (modeling_perceiver.py:499-512)
  const int Lz = 4;
  float* z = out32 ? out32 : R.ws<float>((size_t)n * Lz * E);
  if (R.err) return R.err;
  OTHER(R, launch_broadcast_rows(h->latents, z, (long long)n * Lz, E, Lz, R.st), "latents");
  if (perceiver_layer(R, h->perc_cross, z, n, Lz, tok32, 2 * NP)) return R.err;
  for (int blk = 0; blk < 4; ++blk)
    for (int i = 0; i < 4; ++i)
      if (perceiver_layer(R, h->perc_self[i], z, n, Lz, nullptr, 0)) return R.err;
  if (outT) OTHER(R, launch_cast(z, outT, (long long)n * Lz * E, h->bf16, R.st), "cast");
  return R.err;
}

int baseline_ready(VimaHandle* h, const char* fn) {
  if (!h) return fail("null handle");
  if (h->cfg.policy_kind == VIMA_POLICY_VIMA)
    return fail(std::string(fn) + ": the handle is a VIMAPolicy (policy_kind 0); this entry point belongs to the baseline policies");
  return check_ready(h);
}

// Workspace of one pass of HFGPT blocks over rq rows: q | k | v of the call (qcols = 3E) or its q alone (E: k | v go to the episode cache)
struct HfgptWs { void *qkv, *ctx; float *a32, *n32; void *nT, *g, *u; };
HfgptWs hfgpt_ws(Run& R, int rq, int qcols) {
  const int E = R.h->cfg.embed_dim;
  HfgptWs w;
  w.qkv = R.wsT((size_t)rq * qcols);
  w.ctx = R.wsT((size_t)rq * E);
  w.a32 = R.ws<float>((size_t)rq * E);
  w.n32 = R.ws<float>((size_t)rq * E);
  w.nT = R.wsT((size_t)rq * E);
  w.g = R.wsT((size_t)rq * 4 * E);
  w.u = R.wsT((size_t)rq * 4 * E);
  return w;
}

// A post-LN block behind its attention (gpt/gpt.py:231-246), per row: a = w.ctx; n = ln_1(x + c_proj(a)); h = ln_2(n + mlp(n)) -> x32 / xT
int hfgpt_block_tail(Run& R, const VimaHandle::DecLayer& D, const HfgptWs& w, float* x32, void* xT, int rq) {
  const int E = R.h->cfg.embed_dim;
  R.linear(w.ctx, E, D.c_proj, rq, ACT_NONE, nullptr, 0, x32, E, w.a32, E, nullptr, 0);   // x + a
  R.ln(w.a32, E, D.ln1_g, D.ln1_b, 1e-5f, 0, rq, E, w.n32, w.nT);                         // n = ln_1(x + a)
  R.linear(w.nT, E, D.mgate, rq, ACT_NONE, nullptr, 0, nullptr, 0, nullptr, 0, w.g, 4 * E);
  R.linear(w.nT, E, D.fc, rq, ACT_GELU, w.g, 4 * E, nullptr, 0, nullptr, 0, w.u, 4 * E);   // gelu(c_fc(n)) * gated_layer(n)
  R.linear(w.u, 4 * E, D.mproj, rq, ACT_NONE, nullptr, 0, w.n32, E, w.a32, E, nullptr, 0);  // n + m
  return R.ln(w.a32, E, D.ln2_g, D.ln2_b, 1e-5f, 0, rq, E, x32, xT);                        // h = ln_2(n + m)
}

// HFGPT.forward (gpt/gpt.py:45-80) on an assembled sequence: x32 / xT [B*L, E] (positions already added), key mask [B, L].
// Post-LN blocks: a = attn(x), then hfgpt_block_tail. Result in x32 (and xT).
// kv_store (vima_seq_prefill / vima_seq_decode_restart): every layer's k | v rows are also COPIED to rows [0, L) of the episode cache
// (ep_layer), block kv_list[r] (DEVICE array; nullptr: r) for the r-th sample of this call. A copy, not the c_attn GEMM's
// row-remap epilogue: the attention of these rows reads the dense q | k | v of the call, so the remap would need the k | v columns twice (a
// second GEMM launch per layer), while the copy is one HBM-bound pass over 2E columns, leaves the arithmetic of `vima_seq_decode` untouched
// (same GEMM, same attention launch: the prefilled rows carry its bits) and serves the full prefill and the listed restart alike.
// kv_rowmap (vima_seq_decode_restart_history; DEVICE array [L], needs kv_list): row l goes to cache row kv_rowmap[l] instead of l -- still one launch per layer.
int hfgpt_stack(Run& R, float* x32, void* xT, const uint8_t* mask, int B, int L, bool kv_store = false, const int* kv_list = nullptr,
                const int* kv_rowmap = nullptr) {
  VimaHandle* h = R.h;
  const int E = h->cfg.embed_dim, Hs = h->cfg.sattn_n_heads, rq = B * L;
  const HfgptWs w = hfgpt_ws(R, rq, 3 * E);
  void* qkv = w.qkv;   // q | k | v of the call
  if (R.err) return R.err;
  for (int i = 0; i < h->cfg.xf_n_layers; ++i) {
    auto& D = h->dec[i];
    R.linear(xT, E, D.c_attn, rq, ACT_NONE, nullptr, 0, nullptr, 0, nullptr, 0, qkv, 3 * E);
    if (kv_store) {
      KvRowsArgs c;
      c.in = R.offT(qkv, E); c.ld = 3 * E; c.out = ep_layer(h, i); c.list = kv_list; c.rowmap = kv_rowmap; c.n = B; c.L = L; c.N = 2 * E; c.Lc = h->ep.Lmax;
      OTHER(R, launch_kv_rows(c, (int)h->esz(), R.st), kv_rowmap ? "kv_scatter_rows" : "seq_kv_store");
    }
    AttnArgs s;   // Attention._attn (gpt/gpt.py:268-301): /sqrt(d), w*b + -1e4*(1-b), + (1-mask)*finfo.min
    s.q = qkv; s.ldq = 3 * E; s.k = R.offT(qkv, E); s.ldk = 3 * E; s.v = R.offT(qkv, 2 * E); s.ldv = 3 * E;
    s.out = w.ctx; s.ldo = E; s.B = B; s.H = Hs; s.Lq = L; s.Lk = L; s.D = E / Hs; s.kmask = mask;
    s.scale = 1.0f / sqrtf((float)(E / Hs)); s.mode = ATTN_CAUSAL;
    R.attn(s, h->attn_impl);
    if (hfgpt_block_tail(R, D, w, x32, xT, rq)) return R.err;
  }
  return R.err;
}

// The same blocks for the rows of ONE unit (T env steps; vima_seq_decode_step: T = 1) against the episode cache: x32 / xT [B * Lq, E] are the new
// rows at cache rows [row, row + Lq) of every sample. c_attn appends their k | v to the layer's cache (c_attn_append) and the new queries attend
// to the cache (attn_from_cache: Lk keys, causal window [row, win_end)). Everything after the attention acts per row, as in hfgpt_stack.
int hfgpt_step_stack(Run& R, float* x32, void* xT, int B, int Lq, int row, int Lmax, int Lk, int win_end) {
  VimaHandle* h = R.h;
  const int E = h->cfg.embed_dim, Hs = h->cfg.sattn_n_heads, rq = B * Lq;
  const HfgptWs w = hfgpt_ws(R, rq, E);
  if (R.err) return R.err;
  for (int i = 0; i < h->cfg.xf_n_layers; ++i) {
    auto& D = h->dec[i];
    void* cache = ep_layer(h, i);
    c_attn_append(R, D.c_attn, xT, rq, Lq, row, Lmax, cache, w.qkv);
    AttnArgs s;
    attn_from_cache(R, s, w.qkv, cache, row, Lmax, Lk, win_end);
    s.out = w.ctx; s.ldo = E; s.B = B; s.H = Hs; s.Lq = Lq; s.D = E / Hs;
    s.scale = 1.0f / sqrtf((float)(E / Hs)); s.mode = ATTN_CAUSAL;
    R.attn(s, h->attn_impl);
    if (hfgpt_block_tail(R, D, w, x32, xT, rq)) return R.err;
  }
  return R.err;
}
