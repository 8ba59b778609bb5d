// The launches of one forward, written once and compiled once per 16-bit flavour: engine.hip includes this file inside namespace fwd_bf16
// (using namespace ats_bf16: bf16 and the fp32 parity mode) and inside namespace fwd_f16 (using namespace ats_f16), so that every ats_*
// call below binds to the kernels of the model's arithmetic type.  No include guard on purpose.
// The RoPE + KV-scatter pass of a layer whose qkv projection stored plain 16-bit (fp32) outputs: with an adapter (atspeed_llama_set_lora) the
// pass that adds lora_B's term first
static int rope_pass(atspeed_llama* m, int l, const SegTable& t, const SegTable* dtab, size_t loff, hipStream_t st) {
  const atspeed_llama_config& c = m->cfg;
  ActCtx* cx = m->act;
  if (!m->has_lora()) return ats_rope_kv_segs(cx->qkv, t, dtab, m->cos_tab, m->sin_tab, loff, c.n_heads, m->head_dim, c.max_slots, c.dtype, st);
  m->lora_cnt++;
  if (m->n_slots > 0)            // resident adapters: each row's slot from the segment table (atspeed_llama_add_lora)
    return ats_lora_rope_kv_segs_multi(cx->qkv, cx->lora_u, m->slot_tab + (size_t)l * (ATSPEED_LORA_MAX_ADAPTERS + 1), t, dtab, m->cos_tab,
                                       m->sin_tab, loff, c.n_heads, m->head_dim, c.max_slots, c.dtype, st);
  const atspeed_llama::LoraLayer& a = m->lora[l];
  return ats_lora_rope_kv_segs(cx->qkv, cx->lora_u, a.b[0], a.b[1], a.b[2], m->lora_r16, m->lora_scaling, t, dtab, m->cos_tab, m->sin_tab, loff,
                               c.n_heads, m->head_dim, c.max_slots, c.dtype, st);
}
// lora_A of a layer's normed input for q, k and v at once, from the residual stream (so it does not matter whether the forward left xn or xq / sx)
static int lora_shrink(atspeed_llama* m, int l, const SegTable& t, const SegTable* dtab, hipStream_t st) {
  if (!m->has_lora()) return ATSPEED_OK;
  const int T = t.total_tok;
  m->lora_cnt++;
  if (m->n_slots > 0)
    return ats_lora_shrink_segs(m->act->h, m->layers[l].input_norm, m->slot_tab + (size_t)l * (ATSPEED_LORA_MAX_ADAPTERS + 1), true, m->act->lora_u,
                                t, dtab, m->cfg.hidden, m->cfg.rms_eps, m->cfg.dtype, st);
  return ats_lora_shrink(m->act->h, m->layers[l].input_norm, m->lora[l].a_cat, m->act->lora_u, T, m->cfg.hidden, 3 * m->lora_r16, m->cfg.rms_eps,
                         m->cfg.dtype, st);
}

// the launches of one forward (also the body of a captured graph: no allocation, no synchronisation, no staging in here)
static int llama_forward_body(atspeed_llama* m, const SegTable& t, const SegTable* dtab, float* logits_out, hipStream_t st,
                              const unsigned char* tile_store, int logit_row_off) {
  const atspeed_llama_config& c = m->cfg;
  ActCtx* cx = m->act;
  const int T = t.total_tok;
  const int H = c.hidden, dt = c.dtype, pk = m->pk;
  const SkArena* sk = cx->sk.ws ? &cx->sk : nullptr;       // this model's arena for the ring kernel's split-K tail (ordered by this stream alone)
  ATS_TRY(ats_embed_segs(m->embed, t, dtab, cx->h, H, c.vocab_size, dt, st));
  // What this forward runs, decided here once (the rules depend on the model and the token count alone, not on the layer).  Per projection:
  // its scheme -- a W4A8 model's are all W4A8, a W8A8 model's are W8A8 where the W8A8 kernels take the shape at T tokens, the rest is 16-bit --
  // and whether its producer hands it its input as e4m3 rows + scales in cx->xq / cx->sx (no quantisation pass, no 16-bit cx->xn).  The
  // producers that can are the fused norm + quantisation (hidden <= 8192) of the first layer's input norm and of a quantised residual
  // projection: o_proj for gate_up, down for the next layer's qkv.  o_proj and down read att / act, which are 16-bit always.
  ProjShape shape[N_PROJ];
  int scheme[N_PROJ];
  for (int p = 0; p < N_PROJ; ++p) {
    shape[p] = proj_shape(c, p);
    scheme[p] = m->scheme == SCHEME_W8A8 && !ats_gemm_fp8_applies(T, shape[p].n, shape[p].k, shape[p].ldc, shape[p].epi) ? SCHEME_16 : m->scheme;
  }
  const bool norm_quant = H <= 8192;
  const bool first_in_q = norm_quant && scheme[P_QKV] != SCHEME_16;          // the first layer's qkv, from the norm below
  bool in_q[N_PROJ] = {};
  in_q[P_QKV] = first_in_q && scheme[P_DOWN] != SCHEME_16;                     // every later layer's
  in_q[P_GU] = norm_quant && scheme[P_GU] != SCHEME_16 && scheme[P_O] != SCHEME_16;
  if (first_in_q) ATS_TRY(ats_rmsnorm_quant_fp8(cx->h, m->layers[0].input_norm, nullptr, cx->xq, cx->sx, T, H, c.rms_eps, st, pk));
  else ATS_TRY(ats_rmsnorm(cx->h, m->layers[0].input_norm, cx->xn, T, H, c.rms_eps, dt, st, pk));
  // The forms only qkv has.  RoPE and the KV scatter ride in the projection's epilogue (one pass over qkv / one launch less per layer): the ring
  // kernels of the batched 16-bit and W8A8 forwards, and since round 6 ONE user's W8A8 projection on the weight-streaming kernel
  // (gemm_wdma_kernel<..., EPI_QKV_ROPE, F8>).  Else one user's 16-bit or W8A8 projection may leave fp32 split-K slabs that the RoPE kernel sums
  // itself (one launch less per layer; W8A8: a width where the projection is cut in K, hidden < 3200).  W4A8 and any adapter: the plain store,
  // then rope_pass (which adds the adapter's term before it rotates).
  const bool lora = m->has_lora();
  const bool qkv_plain = lora || scheme[P_QKV] == SCHEME_W4A8;
  const bool qkv_rope_fused = qkv_plain ? false : scheme[P_QKV] == SCHEME_W8A8 ? ats_gemm_fp8_qkv_rope_applies(T, H, m->head_dim) : ats_gemm_qkv_rope_applies(T, H, m->head_dim, dt);
  const bool qkv_slabs = !qkv_plain && !qkv_rope_fused && ats_switch(ATS_SW_FUSE_QKV_REDUCE) != 0 && m->head_dim % 16 == 0;
  if (qkv_rope_fused) ATS_TRY(ats_row_info(t, dtab, cx->rowinfo, c.max_slots, st));

  // The two operations of a layer, over M rows, each inside the projection's profile bracket and counted under the scheme it ran in.  A
  // quantised projection reads e4m3 rows: `x` (16-bit) is quantised first unless `x_in_q` says the producer left them.
  struct Weights { const void *w16, *wq, *sq; };
  auto begin = [&](int p, int l, const void* x, bool x_in_q, int M, Weights* w) -> int {
    m->proj_cnt[scheme[p]][p]++;
    *w = Weights{proj_weight(m->layers[l], p), nullptr, nullptr};
    if (scheme[p] == SCHEME_16) return ATSPEED_OK;
    w->wq = m->quant[l].w[p]; w->sq = m->quant[l].s[p];
    return x_in_q ? ATSPEED_OK : ats_quant_rows_fp8(x, M, shape[p].k, shape[p].k, cx->xq, cx->sx, st, pk);
  };
  // out = epilogue(x W^T)
  auto gemm = [&](int p, const Weights& w, const void* x, void* out, int M) -> int {
    const ProjShape& s = shape[p];
    if (scheme[p] == SCHEME_W8A8) return ats_gemm_fp8(cx->xq, cx->sx, w.wq, (const float*)w.sq, out, M, s.n, s.k, s.ldc, s.epi, st, pk, cx->ws, cx->ws_bytes);
    if (scheme[p] == SCHEME_W4A8) return ats_gemm_w4a8(cx->xq, cx->sx, w.wq, w.sq, out, M, s.n, s.k, s.ldc, s.epi, st, pk, cx->ws, cx->ws_bytes);
    return ats_gemm(x, w.w16, out, M, s.n, s.k, s.k, s.ldc, dt, s.epi, cx->ws, cx->ws_bytes, st, pk, sk);
  };
  auto project = [&](int p, int l, const void* x, bool x_in_q, void* out, int M) -> int {
    ProfBracket pb(m, p, M, st);
    Weights w;
    ATS_TRY(begin(p, l, x, x_in_q, M, &w));
    return gemm(p, w, x, out, M);
  };
  // h += x W^T ; then rmsnorm(h) * norm_w for the consumer `next`: its e4m3 rows when in_q[next], else cx->xn
  auto project_resid_norm = [&](int p, int l, const void* x, void* h, const void* norm_w, int next, int M) -> int {
    ProfBracket pb(m, p, M, st);
    const ProjShape& s = shape[p];
    Weights w;
    ATS_TRY(begin(p, l, x, false, M, &w));
    void* xn = in_q[next] ? nullptr : cx->xn; void* xq = in_q[next] ? cx->xq : nullptr; float* sx = in_q[next] ? cx->sx : nullptr;
    if (scheme[p] == SCHEME_W8A8)
      return ats_gemm_fp8_resid_norm(cx->xq, cx->sx, w.wq, (const float*)w.sq, h, M, s.n, s.k, s.ldc, norm_w, xn, xq, sx, c.rms_eps, cx->ws, cx->ws_bytes, st, pk);
    if (scheme[p] == SCHEME_W4A8)
      return ats_gemm_w4a8_resid_norm(cx->xq, cx->sx, w.wq, w.sq, h, M, s.n, s.k, s.ldc, norm_w, xn, xq, sx, c.rms_eps, cx->ws, cx->ws_bytes, st, pk);
    return ats_gemm_resid_norm(x, w.w16, h, M, s.n, s.k, s.k, s.ldc, dt, norm_w, xn, c.rms_eps, cx->ws, cx->ws_bytes, st, pk, sk);
  };
  // qkv of layer l from its normed input (x_in_q: e4m3 rows, else cx->xn).  *splits > 0: the projection left that many slabs in cx->ws
  auto project_qkv = [&](int l, size_t loff, bool x_in_q, int* splits) -> int {
    ProfBracket pb(m, P_QKV, T, st);
    Weights w;
    ATS_TRY(begin(P_QKV, l, cx->xn, x_in_q, T, &w));
    const bool q = scheme[P_QKV] == SCHEME_W8A8;
    if (qkv_rope_fused) {
      m->rope_fused_cnt++;
      const RopeEpi e{cx->rowinfo, m->cos_tab, m->sin_tab, loff, H};
      return q ? ats_gemm_fp8_qkv_rope(cx->xq, cx->sx, w.wq, (const float*)w.sq, cx->qkv, T, H, e, st, pk) : ats_gemm_qkv_rope(cx->xn, w.w16, cx->qkv, T, H, e, st, pk, sk);
    }
    if (qkv_slabs)
      ATS_TRY(q ? ats_gemm_fp8_partials(cx->xq, cx->sx, w.wq, (const float*)w.sq, T, 3 * H, H, cx->ws, cx->ws_bytes, st, splits, pk)
                : ats_gemm_partials(cx->xn, w.w16, T, 3 * H, H, H, dt, cx->ws, cx->ws_bytes, st, splits, pk));
    return *splits > 0 ? ATSPEED_OK : gemm(P_QKV, w, cx->xn, cx->qkv, T);
  };

  // the row-pruned tail of the last layer (engine.hip: forward_prunes_tail): its back part runs over the R logit rows only
  const bool prune_tail = forward_prunes_tail(m, t);
  const int R = t.total_logit;
  // A layer behind its attention, over the M rows of (h: residual stream, att: attention output): o_proj + post-attention norm, gate_up + SwiGLU,
  // down (+ the next layer's input norm; the last layer's down is the plain residual epilogue and leaves nothing for a consumer).  Every layer
  // calls it on (T, cx->h, cx->att); the pruned last layer on (R, cx->gath, cx->att_tail).  xn, act, xq / sx are used from row 0 either way.
  auto layer_back = [&](int l, int M, void* h, const void* att) -> int {
    ATS_TRY(project_resid_norm(P_O, l, att, h, m->layers[l].post_norm, P_GU, M));
    ATS_TRY(project(P_GU, l, cx->xn, in_q[P_GU], cx->act, M));
    if (l + 1 < c.n_layers) return project_resid_norm(P_DOWN, l, cx->act, h, m->layers[l + 1].input_norm, P_QKV, M);
    return project(P_DOWN, l, cx->act, false, h, M);
  };
  for (int l = 0; l < c.n_layers; ++l) {
    const size_t loff = (size_t)l * m->layer_kv_bytes;
    // the layer's normed input is here: from the first norm above or the previous layer's down
    ATS_TRY(lora_shrink(m, l, t, dtab, st));
    int qkv_splits = 0;
    ATS_TRY(project_qkv(l, loff, l == 0 ? first_in_q : in_q[P_QKV], &qkv_splits));
    if (qkv_rope_fused) {}
    else if (qkv_splits > 0)
      ATS_TRY(ats_rope_kv_segs_slabs((const float*)cx->ws, qkv_splits, cx->qkv, t, dtab, m->cos_tab, m->sin_tab, loff, c.n_heads, m->head_dim, c.max_slots, st));
    else
      ATS_TRY(rope_pass(m, l, t, dtab, loff, st));
    ATS_TRY(ats_tree_attention_segs(cx->qkv, 3 * H, t, dtab, loff, m->vis_words, cx->att, H, c.n_heads, m->head_dim, dt, st, 0, pk));
    if (prune_tail && l + 1 == c.n_layers) {     // nobody reads the other rows of the last layer's output (their K / V are in the cache)
      if (R == 0) break;
      ATS_TRY(ats_gather_tail_rows(cx->h, cx->att, t, dtab, cx->gath, cx->att_tail, H, dt, st, pk));
      ATS_TRY(layer_back(l, R, cx->gath, cx->att_tail));
    } else {
      ATS_TRY(layer_back(l, T, cx->h, cx->att));
    }
  }
  if (R > 0) {
    if (!prune_tail) ATS_TRY(ats_gather_logit_rows(cx->h, t, dtab, cx->gath, H, dt, st));     // (the pruned tail left the last layer's output in gath)
    ATS_TRY(ats_rmsnorm(cx->gath, m->final_norm, cx->xn, R, H, c.rms_eps, dt, st, pk));
    float* lo = logits_out ? logits_out : cx->logits + (size_t)logit_row_off * m->logits_ld;
    float* lse = cx->lse + logit_row_off;
    if (tile_store) {      // decoder forwards: logits + full-vocabulary normaliser (beamSD.py:58,285) from ONE kernel where the batch is large enough
      ProfBracket pb(m, 4, R, st);
      ATS_TRY(ats_lmhead_lse(cx->xn, m->lm_head, lo, R, c.vocab_size, H, H, m->logits_ld, dt, tile_store, cx->lse_part, cx->lse_part_bytes, lse,
                             cx->ws, cx->ws_bytes, st, nullptr, pk, sk));
    } else {
      { ProfBracket pb(m, 4, R, st);
        ATS_TRY(ats_gemm(cx->xn, m->lm_head, lo, R, c.vocab_size, H, H, m->logits_ld, dt, EPI_F32, cx->ws, cx->ws_bytes, st, pk, sk)); }
      ATS_TRY(ats_lse_rows(lo, R, c.vocab_size, m->logits_ld, lse, st));     // beamSD.py:58,285: full-vocab normaliser
    }
  }
  return ATSPEED_OK;
}

