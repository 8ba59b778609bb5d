// Host-side interfaces of the kernel translation units that exist once per 16-bit flavour (gemm.hip, attn.hip, elementwise.hip: common.h,
// "the 16-bit flavour").  internal.h includes this file inside namespace ats_bf16 (which also holds the fp32 parity kernels) and inside
// namespace ats_f16; callers outside those translation units choose with ATS_KD(dtype, call).  No include guard on purpose.
// ---- elementwise.hip --------------------------------------------------------------
// `t` = host copy (sizes), `dt` = the staged device copy the kernels read
int ats_fill_hash_normal(void* dst, size_t n, uint32_t seed, float scale, float add, int dtype, uint64_t offset, hipStream_t st);
int ats_embed_segs(const void* table, const SegTable& t, const SegTable* dt, void* out, int hidden, int vocab, int dtype, hipStream_t st);
// qkv_slabs != nullptr: the projection's fp32 split-K slabs [splits][total_tok][3 * hidden]; q is written (rotated) to qkv, k / v only to the caches
int ats_rope_kv_segs_slabs(const float* qkv_slabs, int splits, void* qkv, const SegTable& t, const SegTable* dt, const float* cos_tab,
                           const float* sin_tab, size_t layer_off_bytes, int n_heads, int head_dim, int max_pos, hipStream_t st);
// rotate q and k in place inside the fused qkv buffer ([T][3*hidden]) and scatter k,v to the cache slots
int ats_rope_kv_segs(void* qkv, const SegTable& t, const SegTable* dt, const float* cos_tab, const float* sin_tab, size_t layer_off_bytes,
                     int n_heads, int head_dim, int max_pos, int dtype, hipStream_t st);
int ats_row_info(const SegTable& t, const SegTable* dt, RowInfo* out, int max_pos, hipStream_t st);
int ats_gather_logit_rows(const void* h, const SegTable& t, const SegTable* dt, void* out, int hidden, int dtype, hipStream_t st);
// the same rows of h (row-major) and of att (a GEMM operand: packed when pk) to consecutive rows of h_out / att_out, in one launch
int ats_gather_tail_rows(const void* h, const void* att, const SegTable& t, const SegTable* dt, void* h_out, void* att_out, int hidden, int dtype,
                         hipStream_t st, int pk = 0);
int ats_rmsnorm(const void* x, const void* w, void* y, int rows, int hidden, float eps, int dtype, hipStream_t st, int pk = 0);   // pk: y in the packed operand layout
// row-major [rows][row_bytes] -> packed operand layout (common.h ats_pk_byte) or back; out of place, row_bytes % 64 == 0
int ats_pack_rows(const void* src, void* dst, int rows, int row_bytes, int to_packed, hipStream_t st);
// rows [0, len) of every layer between a compact store [layers][len][row_bytes] (K and V) and arenas [layers][max_slots][row_bytes]: to_store = 0
// scatters the store to the arenas of n_users (dev_users: DEVICE array) in one launch, 1 gathers it from dev_users[0]'s.  Bytes only: no flavour
int ats_kv_rows_copy(void* store_k, void* store_v, const KvRowsUser* dev_users, int n_users, int len, int layers, int row_bytes, int max_slots,
                     int to_store, hipStream_t st);

// ---- lora.hip -------------------------------------------------------------------------
// u [rows][r3] = round(A_cat . xn^T) per row, xn = the RMSNorm of h's row under norm_w (recomputed: independent of what the forward left in xn / xq);
// r3 = 3 x the padded rank (48, 96, 144 or 192), A_cat [r3][hidden]
int ats_lora_shrink(const void* h, const void* norm_w, const void* a_cat, void* u, int rows, int hidden, int r3, float eps, int dtype,
                    hipStream_t st);
// ats_rope_kv_segs with y = base + scaling * (B_m u_m) in front for every module whose B_m [hidden][r16] is not NULL (common.h: lora_add)
int ats_lora_rope_kv_segs(void* qkv, const void* u, const void* bq, const void* bk, const void* bv, int r16, float scaling, const SegTable& t,
                          const SegTable* dt, const float* cos_tab, const float* sin_tab, size_t layer_off_bytes, int n_heads, int head_dim,
                          int max_pos, int dtype, hipStream_t st);
// the two above with the adapter picked per row -- the same kernels over the adapter source LoraBySeg instead of LoraOne (Seg::adapter ->
// dev_slots[adapter], DEVICE table of ATSPEED_LORA_MAX_ADAPTERS + 1 entries, entry 0 = none); u has a fixed row stride of 3 x 64 elements, rows
// of slot 0 are neither written nor read.  slots_aligned: every a_cat is 16-byte aligned (the MFMA shrink's operand loads)
int ats_lora_shrink_segs(const void* h, const void* norm_w, const atspeed_lora_slot* dev_slots, bool slots_aligned, void* u, const SegTable& t,
                         const SegTable* dt, int hidden, float eps, int dtype, hipStream_t st);
int ats_lora_rope_kv_segs_multi(void* qkv, const void* u, const atspeed_lora_slot* dev_slots, const SegTable& t, const SegTable* dt,
                                const float* cos_tab, const float* sin_tab, size_t layer_off_bytes, int n_heads, int head_dim, int max_pos,
                                int dtype, hipStream_t st);

// ---- gemm.hip -------------------------------------------------------------------------
size_t ats_gemm_workspace_bytes(int m, int n, int k, int dtype);
// pk = 1: a and w (and a SwiGLU output) are in the packed operand layout of common.h (bf16 / fp8 engine); 0: row-major (HF layout, fp32 mode, ABI tests)
int ats_gemm(const void* a, const void* w, void* c, int m, int n, int k, int lda, int ldc, int dtype, int epilogue,
             void* workspace, size_t workspace_bytes, hipStream_t st, int pk = 0, const SkArena* sk = nullptr);

int ats_gemm_resid_norm(const void* a, const void* w, void* h, int m, int n, int k, int lda, int ldh, int dtype,
                        const void* norm_w, void* xn, float eps, void* workspace, size_t workspace_bytes, hipStream_t st, int pk = 0,
                        const SkArena* sk = nullptr);
// The batched qkv projection with the rotation and the cache scatter in its epilogue: qkv[m][3*hidden] receives only the rotated q,
// rotated k and v go straight to the caches (bit-identical to ats_gemm + ats_rope_kv_segs: both round the projection to bf16 first).
// Applies to bf16, head_dim 128, hidden % 256 == 0 at shapes the ring kernel takes; the caller asks first.
bool ats_gemm_qkv_rope_applies(int m, int hidden, int head_dim, int dtype);
int ats_gemm_qkv_rope(const void* x, const void* wqkv, void* qkv, int m, int hidden, const RopeEpi& rope, hipStream_t st, int pk = 0,
                      const SkArena* sk = nullptr);
bool ats_gemm_fp8_qkv_rope_applies(int m, int hidden, int head_dim);
int ats_gemm_fp8_qkv_rope(const void* xq, const float* sx, const void* wq, const float* sw, void* qkv, int m, int hidden, const RopeEpi& rope,
                          hipStream_t st, int pk = 0);

// fp8 (e4m3, per-row scales) variants of the batched projections; returns ATSPEED_ERR_INVALID if the shape does not
// qualify (ats_gemm_fp8_applies)
int ats_quant_rows_fp8(const void* x, int rows, int cols, int ld, void* q, float* scale, hipStream_t st, int pk = 0);          // pk: x and q packed
// RMSNorm fused with the per-token quantisation of its output (bf16, hidden <= 8192); y may be null
int ats_rmsnorm_quant_fp8(const void* x, const void* w, void* y, void* q, float* scale, int rows, int hidden, float eps, hipStream_t st, int pk = 0);   // pk: y and q packed
bool ats_gemm_fp8_applies(int m, int n, int k, int ldc, int epilogue);
// 1-256 rows: the weight-streaming kernel (one user's forwards); narrow N is then cut in K and needs `ws` for its fp32 slabs
// (ats_gemm_fp8_workspace_bytes; without it the launch runs one part per tile)
size_t ats_gemm_fp8_workspace_bytes(int m, int n, int k);
int ats_gemm_fp8(const void* xq, const float* sx, const void* wq, const float* sw, void* c, int m, int n, int k, int ldc,
                 int epilogue, hipStream_t st, int pk = 0, void* ws = nullptr, size_t ws_bytes = 0);
int ats_gemm_fp8_partials(const void* xq, const float* sx, const void* wq, const float* sw, int m, int n, int k, void* ws, size_t ws_bytes,
                          hipStream_t st, int* splits_out, int pk = 0);
int ats_gemm_fp8_resid_norm(const void* xq, const float* sx, const void* wq, const float* sw, void* h, int m, int n, int k, int ldh,
                            const void* norm_w, void* xn, void* q_out, float* s_out, float eps, void* ws, size_t ws_bytes, hipStream_t st, int pk = 0);

// W4A8 (OCP MXFP4 weights, e4m3 activations with per-token scales; format: gemm.hip "W4A8"): weights row-major [rows][K / 2] e2m1 nibbles +
// [rows][K / 32] E8M0 scale bytes; K % 256 == 0.  pk: the 16-bit input of the quantiser / xq and a SwiGLU output in the packed operand layout
int ats_quant_weights_mxfp4(const void* w, int rows, int k, void* q, void* scales, hipStream_t st, int pk = 0);
size_t ats_gemm_w4a8_workspace_bytes(int m, int n, int k);
int ats_gemm_w4a8(const void* xq, const float* sx, const void* wq, const void* wsc, void* c, int m, int n, int k, int ldc, int epilogue,
                  hipStream_t st, int pk = 0, void* ws = nullptr, size_t ws_bytes = 0);
int ats_gemm_w4a8_resid_norm(const void* xq, const float* sx, const void* wq, const void* wsc, void* h, int m, int n, int k, int ldh,
                             const void* norm_w, void* xn, void* q_out, float* s_out, float eps, void* ws, size_t ws_bytes, hipStream_t st, int pk = 0);

size_t ats_lmhead_lse_part_bytes(int m, int n);
int ats_lmhead_lse(const void* a, const void* w, float* logits, int m, int n, int k, int lda, int ldc, int dtype, const unsigned char* tile_store,
                   float* part, size_t part_bytes, float* lse, void* workspace, size_t workspace_bytes, hipStream_t st, int* fused_out = nullptr,
                   int pk = 0, const SkArena* sk = nullptr);

int ats_gemm_partials(const void* a, const void* w, int m, int n, int k, int lda, int dtype, void* workspace, size_t workspace_bytes,
                      hipStream_t st, int* splits_out, int pk = 0);

// ---- attn.hip -------------------------------------------------------------------------
int ats_tree_attention(const void* q, int ldq, const void* kcache, const void* vcache, const uint64_t* vis,
                       int vis_words, void* out, int ldo, int n_tokens, int n_slots, int n_heads, int head_dim,
                       int dtype, hipStream_t st, int qtile_rows = 0, int rows_per_wave = 0);

int ats_tree_attention_segs(const void* q, int ldq, const SegTable& t, const SegTable* dt, size_t layer_off_bytes, int vis_words,
                            void* out, int ldo, int n_heads, int head_dim, int dtype, hipStream_t st, int rows_per_wave = 0,
                            int pk = 0);       // pk: out (the o_proj operand) in the packed operand layout

