// The launches of one forward, written once and compiled once per 16-bit flavour: engine.hip includes this file inside namespace fwd_bf16
// (using namespace ats_bf16: bf16 and the fp32 parity mode) and inside namespace fwd_f16 (using namespace ats_f16), so that every ats_*
// call below binds to the kernels of the model's arithmetic type.  No include guard on purpose.
// fp8 projection when enabled and the shape is on the batched path: quantise the activations per token, then W8A8 GEMM
// x == nullptr: cx->xq / cx->sx already hold the quantised activations (written by the fused RMSNorm)
static int proj_fp8(atspeed_llama* m, const void* x, const void* wq, const float* sw, void* out, int M, int N, int K, int ldc,
                    int epi, hipStream_t st) {
  ActCtx* cx = m->act;
  if (x) ATS_TRY(ats_quant_rows_fp8(x, M, K, K, cx->xq, cx->sx, st, m->pk));
  return ats_gemm_fp8(cx->xq, cx->sx, wq, sw, out, M, N, K, ldc, epi, st, m->pk, cx->ws, cx->ws_bytes);
}

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

// One layer of the 4-bit target (atspeed_llama_enable_fp4): all four projections W4A8 at every size, the activations exactly the W8A8 ones
// (per-token e4m3 from the fused RMSNorm / residual reduce or ats_quant_rows_fp8).  qkv: plain 16-bit store, then the RoPE / KV pass (the
// projection rounded to 16 bits, the rotation in fp32).  On entry cx->xq / cx->sx hold the layer's normed input when xq_ready, else cx->xn does.
static int layer_fp4(atspeed_llama* m, int l, const SegTable& t, const SegTable* dtab, size_t loff, bool& xq_ready, hipStream_t st) {
  const atspeed_llama_config& c = m->cfg;
  ActCtx* cx = m->act;
  const atspeed_llama::Fp4Layer& f = m->fp4[l];
  const int T = t.total_tok, H = c.hidden, pk = m->pk;
  const bool q_next = H <= 8192;                           // the fused norm + e4m3 quantisation exists up to hidden 8192
  ATS_TRY(lora_shrink(m, l, t, dtab, st));
  { ProfBracket pb(m, 0, T, st);
    m->fp4_cnt[0]++;
    if (!xq_ready) ATS_TRY(ats_quant_rows_fp8(cx->xn, T, H, H, cx->xq, cx->sx, st, pk));
    ATS_TRY(ats_gemm_w4a8(cx->xq, cx->sx, f.wqkv, f.sqkv, cx->qkv, T, 3 * H, H, 3 * H, EPI_STORE, st, pk, cx->ws, cx->ws_bytes)); }
  ATS_TRY(rope_pass(m, l, t, dtab, loff, st));
  ATS_TRY(ats_tree_attention_segs(cx->qkv, 3 * H, t, dtab, loff, m->vis_words, cx->att, H, c.n_heads, m->head_dim, c.dtype, st, 0, pk));
  { ProfBracket pb(m, 1, T, st);     // h += att Wo^T ; then gate_up's input norm (e4m3 rows + scales, or xn)
    m->fp4_cnt[1]++;
    ATS_TRY(ats_quant_rows_fp8(cx->att, T, H, H, cx->xq, cx->sx, st, pk));
    ATS_TRY(ats_gemm_w4a8_resid_norm(cx->xq, cx->sx, f.wo, f.so, cx->h, T, H, H, H, m->layers[l].post_norm, q_next ? nullptr : cx->xn,
                                     q_next ? cx->xq : nullptr, q_next ? cx->sx : nullptr, c.rms_eps, cx->ws, cx->ws_bytes, st, pk)); }
  { ProfBracket pb(m, 2, T, st);
    m->fp4_cnt[2]++;
    if (!q_next) ATS_TRY(ats_quant_rows_fp8(cx->xn, T, H, H, cx->xq, cx->sx, st, pk));
    ATS_TRY(ats_gemm_w4a8(cx->xq, cx->sx, f.wgu, f.sgu, cx->act, T, 2 * c.ffn, H, c.ffn, EPI_SWIGLU, st, pk, cx->ws, cx->ws_bytes)); }
  { ProfBracket pb(m, 3, T, st);     // h += act Wd^T ; then the next layer's input norm
    m->fp4_cnt[3]++;
    ATS_TRY(ats_quant_rows_fp8(cx->act, T, c.ffn, c.ffn, cx->xq, cx->sx, st, pk));
    if (l + 1 < c.n_layers) {
      ATS_TRY(ats_gemm_w4a8_resid_norm(cx->xq, cx->sx, f.wd, f.sd, cx->h, T, H, c.ffn, H, m->layers[l + 1].input_norm, q_next ? nullptr : cx->xn,
                                       q_next ? cx->xq : nullptr, q_next ? cx->sx : nullptr, c.rms_eps, cx->ws, cx->ws_bytes, st, pk));
      xq_ready = q_next;
    } else {
      ATS_TRY(ats_gemm_w4a8(cx->xq, cx->sx, f.wd, f.sd, cx->h, T, H, c.ffn, H, EPI_RESID, st, pk, cx->ws, cx->ws_bytes));
      xq_ready = false;
    } }
  return ATSPEED_OK;
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
  // fp8 projections fed by an RMSNorm take their e4m3 rows + scales straight from the norm kernel (no quantisation pass, no bf16 xn)
  const bool f4 = !m->fp4.empty();                         // the 4-bit target: layer_fp4 above
  // which projections of the 8-bit target run as W8A8 GEMMs in this forward (the rule depends on the token count alone, not on the layer)
  const bool f8 = !m->fp8.empty();
  const bool qkv_in_fp8 = f8 && ats_gemm_fp8_applies(T, 3 * H, H, 3 * H, EPI_STORE);
  const bool o_in_fp8 = f8 && ats_gemm_fp8_applies(T, H, H, H, EPI_RESID);
  const bool gu_in_fp8 = f8 && ats_gemm_fp8_applies(T, 2 * c.ffn, H, c.ffn, EPI_SWIGLU);
  const bool down_in_fp8 = f8 && ats_gemm_fp8_applies(T, H, c.ffn, H, EPI_RESID);
  const bool f8_qkv = f4 ? H <= 8192 : qkv_in_fp8 && H <= 8192;
  const bool f8_gu = gu_in_fp8 && H <= 8192;
  bool xq_ready = false;
  if (f8_qkv) { ATS_TRY(ats_rmsnorm_quant_fp8(cx->h, m->layers[0].input_norm, nullptr, cx->xq, cx->sx, T, H, c.rms_eps, st, pk)); xq_ready = true; }
  else ATS_TRY(ats_rmsnorm(cx->h, m->layers[0].input_norm, cx->xn, T, H, c.rms_eps, dt, st, pk));
  // RoPE and the KV scatter ride in the qkv projection's epilogue (one pass over qkv / one launch less per layer): the ring kernels of the batched
  // 16-bit and W8A8 forwards, and since round 6 ONE user's W8A8 projection on the weight-streaming kernel (gemm_wdma_kernel<..., EPI_QKV_ROPE, F8>)
  // a model with an adapter: the plain 16-bit store, then the pass that adds the adapter's term before it rotates (no fused epilogue, no slabs)
  const bool lora = m->has_lora();
  const bool qkv_rope_fused = f4 || lora ? false : qkv_in_fp8 ? ats_gemm_fp8_qkv_rope_applies(T, H, m->head_dim) : ats_gemm_qkv_rope_applies(T, H, m->head_dim, dt);
  if (qkv_rope_fused) ATS_TRY(ats_row_info(t, dtab, cx->rowinfo, c.max_slots, st));
  // the row-pruned tail of the last layer (engine.hip: forward_prunes_tail): its back part runs over the R logit rows only
  const bool prune_tail = forward_prunes_tail(m, t);
  const int R = t.total_logit;
  // A layer behind its attention, over the M rows of (h: residual stream, att: attention output): o_proj + post-attention norm, gate_up + SwiGLU,
  // down (+ the next layer's input norm).  Every layer calls it on (T, cx->h, cx->att); the pruned last layer on (R, cx->gath, cx->att_tail).
  // xn, act, xq / sx are used from row 0 either way.
  auto layer_back = [&](int l, int M, void* h, const void* att) -> int {
    const atspeed_llama_layer_weights& w = m->layers[l];
    { ProfBracket pb(m, 1, M, st);     // h += att Wo^T ; xn = rmsnorm(h) * post_norm
      if (o_in_fp8) {
        m->fp8_cnt[1]++;
        ATS_TRY(ats_quant_rows_fp8(att, M, H, H, cx->xq, cx->sx, st, pk));
        ATS_TRY(ats_gemm_fp8_resid_norm(cx->xq, cx->sx, m->fp8[l].wo, m->fp8[l].so, h, M, H, H, H, w.post_norm, f8_gu ? nullptr : cx->xn,
                                        f8_gu ? cx->xq : nullptr, f8_gu ? cx->sx : nullptr, c.rms_eps, cx->ws, cx->ws_bytes, st, pk));
        xq_ready = f8_gu;
      } else {
        m->other_cnt[1]++;
        ATS_TRY(ats_gemm_resid_norm(att, w.wo, h, M, H, H, H, H, dt, w.post_norm, cx->xn, c.rms_eps, cx->ws, cx->ws_bytes, st, pk, sk));
        xq_ready = false;
      } }
    { ProfBracket pb(m, 2, M, st);
      if (gu_in_fp8) {
        m->fp8_cnt[2]++;
        ATS_TRY(proj_fp8(m, xq_ready ? nullptr : cx->xn, m->fp8[l].wgu, m->fp8[l].sgu, cx->act, M, 2 * c.ffn, H, c.ffn, EPI_SWIGLU, st));
      } else {
        m->other_cnt[2]++;
        ATS_TRY(ats_gemm(cx->xn, w.wgu, cx->act, M, 2 * c.ffn, H, H, c.ffn, dt, EPI_SWIGLU, cx->ws, cx->ws_bytes, st, pk, sk));
      } }
    { ProfBracket pb(m, 3, M, st);     // h += act Wd^T ; xn = rmsnorm(h) * next layer's input_norm
      (down_in_fp8 ? m->fp8_cnt : m->other_cnt)[3]++;
      if (down_in_fp8) {
        if (l + 1 < c.n_layers) {
          ATS_TRY(ats_quant_rows_fp8(cx->act, M, c.ffn, c.ffn, cx->xq, cx->sx, st, pk));
          ATS_TRY(ats_gemm_fp8_resid_norm(cx->xq, cx->sx, m->fp8[l].wd, m->fp8[l].sd, h, M, H, c.ffn, H, m->layers[l + 1].input_norm,
                                          f8_qkv ? nullptr : cx->xn, f8_qkv ? cx->xq : nullptr, f8_qkv ? cx->sx : nullptr, c.rms_eps, cx->ws, cx->ws_bytes, st, pk));
          xq_ready = f8_qkv;
        } else {
          ATS_TRY(proj_fp8(m, cx->act, m->fp8[l].wd, m->fp8[l].sd, h, M, H, c.ffn, H, EPI_RESID, st));
          xq_ready = false;
        }
      } else if (l + 1 < c.n_layers) {
        ATS_TRY(ats_gemm_resid_norm(cx->act, w.wd, h, M, H, c.ffn, c.ffn, H, dt, m->layers[l + 1].input_norm, cx->xn, c.rms_eps,
                                    cx->ws, cx->ws_bytes, st, pk, sk));
        xq_ready = false;
      } else {
        ATS_TRY(ats_gemm(cx->act, w.wd, h, M, H, c.ffn, c.ffn, H, dt, EPI_RESID, cx->ws, cx->ws_bytes, st, pk, sk));
      } }
    return ATSPEED_OK;
  };
  for (int l = 0; l < c.n_layers; ++l) {
    const atspeed_llama_layer_weights& w = m->layers[l];
    const size_t loff = (size_t)l * m->layer_kv_bytes;
    if (f4) { ATS_TRY(layer_fp4(m, l, t, dtab, loff, xq_ready, st)); continue; }
    // cx->xn holds rmsnorm(h) * input_norm here (from the embed above or the previous layer's fused down_proj epilogue)
    const bool fuse_qkv_reduce = !lora && ats_switch(ATS_SW_FUSE_QKV_REDUCE) != 0;
    ATS_TRY(lora_shrink(m, l, t, dtab, st));
    int qkv_splits = 0;
    { ProfBracket pb(m, 0, T, st);
      if (qkv_in_fp8) {
        m->fp8_cnt[0]++;
        if (qkv_rope_fused) {
          m->rope_fused_cnt++;
          if (!xq_ready) ATS_TRY(ats_quant_rows_fp8(cx->xn, T, H, H, cx->xq, cx->sx, st, pk));
          ATS_TRY(ats_gemm_fp8_qkv_rope(cx->xq, cx->sx, m->fp8[l].wqkv, m->fp8[l].sqkv, cx->qkv, T, H,
                                        RopeEpi{cx->rowinfo, m->cos_tab, m->sin_tab, loff, H}, st, pk));
        } else {
          // one user's forward at a width where the projection is cut in K (hidden < 3200): scaled fp32 split-K slabs that RoPE sums itself (as the
          // 16-bit path below), else the plain projection
          if (!xq_ready) ATS_TRY(ats_quant_rows_fp8(cx->xn, T, H, H, cx->xq, cx->sx, st, pk));
          if (fuse_qkv_reduce && m->head_dim % 16 == 0)
            ATS_TRY(ats_gemm_fp8_partials(cx->xq, cx->sx, m->fp8[l].wqkv, m->fp8[l].sqkv, T, 3 * H, H, cx->ws, cx->ws_bytes, st, &qkv_splits, pk));
          if (qkv_splits == 0) ATS_TRY(proj_fp8(m, nullptr, m->fp8[l].wqkv, m->fp8[l].sqkv, cx->qkv, T, 3 * H, H, 3 * H, EPI_STORE, st));
        }
      } else if (qkv_rope_fused) {
        m->other_cnt[0]++; m->rope_fused_cnt++;
        ATS_TRY(ats_gemm_qkv_rope(cx->xn, w.wqkv, cx->qkv, T, H, RopeEpi{cx->rowinfo, m->cos_tab, m->sin_tab, loff, H}, st, pk, sk));
      } else {
        m->other_cnt[0]++;
        // one user's forward: the projection leaves fp32 split-K slabs and RoPE sums them itself (one launch less per layer)
        if (fuse_qkv_reduce && m->head_dim % 16 == 0) ATS_TRY(ats_gemm_partials(cx->xn, w.wqkv, T, 3 * H, H, H, dt, cx->ws, cx->ws_bytes, st, &qkv_splits, pk));
        if (qkv_splits == 0) ATS_TRY(ats_gemm(cx->xn, w.wqkv, cx->qkv, T, 3 * H, H, H, 3 * H, dt, EPI_STORE, cx->ws, cx->ws_bytes, st, pk, sk));
      } }
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

