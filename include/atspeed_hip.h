/*
 * atspeed_hip.h — C-ABI of libatspeed_hip.so, the MI355X (gfx950) engine behind the
 * AtSpeed beam-speculative-decoding hot path.
 *
 * The reference (/root/reference, Linxyhaha/AtSpeed) has NO native layer and no FFI: its
 * "plugin surface" for this path is four Python callables.  Each entry point below names
 * the reference interface it replaces (file:line under /root/reference/code).  A
 * maintainer binds these with ctypes; atspeed_amd/_lib.py is that
 * binding.
 *
 * Conventions
 *   - every pointer named *_dev is DEVICE memory owned by the caller (PyTorch-ROCm
 *     tensors' data_ptr()); the library never allocates caller-visible memory.  Handles
 *     own only their private workspace / KV arena (create/destroy pairs).
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); calls are
 *     stream-ordered and never synchronise the device unless documented.
 *   - return value: 0 = ok, negative = atspeed_status; atspeed_last_error() gives the text
 *     (thread-local).
 *   - dtype: ATSPEED_F32 (fp32 weights/activations, exact-fp32 MFMA; parity mode),
 *     ATSPEED_BF16 (bf16 weights/activations/KV, fp32 accumulate, fp32 logits) or
 *     ATSPEED_F16 (the same engine on IEEE half: the type the reference loads both models in, code/inference.py:75-100
 *     `torch_dtype=torch.float16` -- a checkpoint's fp16 weights are used bit for bit; same kernels, v_mfma_f32_*_f16).
 */
#ifndef ATSPEED_HIP_H
#define ATSPEED_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum atspeed_status {
  ATSPEED_OK = 0,
  ATSPEED_ERR_INVALID = -1,      /* bad argument / shape the kernels do not support   */
  ATSPEED_ERR_HIP = -2,          /* a HIP runtime call failed                          */
  ATSPEED_ERR_CAPACITY = -3,     /* prompt/beam/slot count exceeds the handle's limits */
  ATSPEED_ERR_CONSTRAINT = -4,   /* a beam reached a node with no allowed token (HF raises ValueError there) */
  ATSPEED_ERR_NO_DEVICE = -5,
  ATSPEED_ERR_FILTERED = -6      /* every beam of a step fell to the post-top-k id filter of beamSD.py:80-86 (the reference then dies on a shape mismatch) */
} atspeed_status;

typedef enum atspeed_dtype { ATSPEED_F32 = 0, ATSPEED_BF16 = 1, ATSPEED_F16 = 2 } atspeed_dtype;

#define ATSPEED_MAX_BEAMS 64      /* K, DK <= 64 (one wavefront holds a beam list)       */
#define ATSPEED_MAX_NEW_TOKENS 16 /* generated-suffix capacity per beam                  */
#define ATSPEED_MAX_GAMMA 8

const char* atspeed_version(void);
const char* atspeed_last_error(void);
/* number of HIP devices visible (0 on a CPU-only host; never initialises a context) */
int atspeed_device_count(void);

/* ------------------------------------------------------------------ synthetic fill
 * value(i) = float(int(s_i) - 131070) * scale, s_i = sum of four 16-bit hash pieces of
 * (i + offset, seed) — bit-identical to atspeed_amd.synth.hash_normal.  `add` is added
 * after scaling (norm weights: 1 + jitter).  No reference counterpart (test/bench input). */
int atspeed_fill_hash_normal(void* dst_dev, size_t n, uint32_t seed, float scale, float add,
                             int dtype, uint64_t offset, void* stream);

/* ------------------------------------------------------------------ constraint automaton
 * Device form of the reference's mask functions — Trie.get() (generation_trie.py:27-70),
 * prefix_allowed_tokens_fn (generation_trie.py:92-98), the position-set function
 * (data.py:84-104) — which the reference calls once per beam per step on the host through
 * HF's PrefixConstrainedLogitsProcessor (beamSD.py:62-64,288-291).
 * CSR: node n allows tok[row_ptr[n]..row_ptr[n+1]) (strictly ascending), edge e leads to
 * node nxt[e].  Arrays are HOST pointers, copied to the device. */
typedef struct atspeed_fsm atspeed_fsm;
int atspeed_fsm_create(const int32_t* row_ptr, const int32_t* tok, const int32_t* nxt,
                       int32_t n_nodes, int32_t n_edges, int32_t vocab_size, atspeed_fsm** out);
void atspeed_fsm_destroy(atspeed_fsm* fsm);
/* The "automaton" of a call WITHOUT a mask: BSSD(..., logits_processor=None, prefix_allowed_tokens_fn=None) is legal in the reference
 * (beamSD.py:460-481: both optional; with an empty processor list :60-64 is the identity and the id filter :80-86 is skipped).  Every
 * token of the vocabulary is then a candidate of every beam; the decoder first reduces each logit row to its k best tokens
 * (atspeed_row_topk) and expands those.  Greedy mode only. */
int atspeed_fsm_create_free(int32_t vocab_size, atspeed_fsm** out);
/* one_step_beam_search drops, AFTER the top-k, every pick whose token is `< 32000 and != 2` (beamSD.py:80-86, hard-coded for the
 * Llama-2 vocabulary + item codes).  An automaton is created with those two numbers; other vocabularies set their own here
 * (min_item_token <= 0: keep every pick).  If a step loses ALL its beams to the filter the generate call returns ATSPEED_ERR_FILTERED. */
int atspeed_fsm_set_id_filter(atspeed_fsm* fsm, int32_t min_item_token, int32_t eos_token);
/* host-side flattening of token sequences into the CSR above (breadth-first node ids,
 * children ascending): native counterpart of Trie.__init__/_add_to_trie
 * (generation_trie.py:8-14,40-44).  Two-call protocol: pass NULL outputs to get the sizes. */
int atspeed_trie_flatten(const int32_t* seq_tokens, const int32_t* seq_offsets, int32_t n_seqs,
                         int32_t* row_ptr_out, int32_t* tok_out, int32_t* nxt_out,
                         int32_t* n_nodes_out, int32_t* n_edges_out);

/* ------------------------------------------------------------------ model
 * Replaces the model object the path calls as model(**inputs) (beamSD.py:52,221):
 * a Llama decoder whose weights live in HBM.  Weight pointers are device pointers in the
 * handle's dtype, row-major [out, in] like HF nn.Linear:
 *   wqkv  [3*hidden, hidden]   rows = q_proj | k_proj | v_proj
 *   wo    [hidden, hidden]
 *   wgu   [2*ffn, hidden]      gate/up interleaved in 16-row groups: rows 32b..32b+15 =
 *                              gate[16b..], rows 32b+16..32b+31 = up[16b..]
 *   wd    [hidden, ffn]
 *   norm weights [hidden]; embed [vocab, hidden]; lm_head [vocab, hidden]           */
/* ATSPEED_WEIGHTS_ROW_MAJOR: [out, in] row-major as HF stores them.  ATSPEED_WEIGHTS_PACKED (bf16 only; hidden and ffn multiples of 32):
 * each matrix run through atspeed_pack_rows -- two consecutive rows share one 128-byte line per 64-byte block of the in dimension, which
 * is what lets every LDS-DMA piece of the projection GEMMs fetch FULL cache lines (83 against 55 GB/s per CU from L2, measured).  With
 * packed weights the engine keeps the activations a projection reads in the same layout internally; results are identical. */
typedef enum atspeed_weight_layout { ATSPEED_WEIGHTS_ROW_MAJOR = 0, ATSPEED_WEIGHTS_PACKED = 1 } atspeed_weight_layout;
/* row-major [rows][row_bytes] (row_bytes % 64 == 0) -> packed operand layout, out of place: byte b of row r goes to
 * ((r >> 1) * (row_bytes / 64) + (b >> 6)) * 128 + (r & 1) * 64 + (b & 63); dst holds rows rounded up to even (the pad row is zeroed).
 * atspeed_unpack_rows is the inverse.  Both 16-byte aligned device buffers. */
int atspeed_pack_rows(const void* src_dev, void* dst_dev, int32_t rows, int32_t row_bytes, void* stream);
int atspeed_unpack_rows(const void* src_dev, void* dst_dev, int32_t rows, int32_t row_bytes, void* stream);

typedef struct atspeed_llama_layer_weights {
  const void* input_norm;
  const void* wqkv;
  const void* wo;
  const void* post_norm;
  const void* wgu;
  const void* wd;
} atspeed_llama_layer_weights;

typedef struct atspeed_llama_config {
  int32_t vocab_size, hidden, n_layers, n_heads, ffn;
  float rope_theta, rms_eps;
  int32_t dtype;          /* atspeed_dtype */
  int32_t max_slots;      /* KV capacity (multiple of 64) */
  int32_t max_tokens;     /* max tokens per forward */
  int32_t max_logit_rows; /* max rows the lm_head is applied to */
  int32_t weight_layout;  /* atspeed_weight_layout of the projection weights and lm_head (embed and norms are always plain) */
} atspeed_llama_config;

typedef struct atspeed_llama atspeed_llama;
int atspeed_llama_create(const atspeed_llama_config* cfg, const void* embed_dev, const void* final_norm_dev,
                         const void* lm_head_dev, const atspeed_llama_layer_weights* layers /* host array */,
                         atspeed_llama** out);
void atspeed_llama_destroy(atspeed_llama* m);

/* One forward (beamSD.py:52 / :221): T tokens, written to KV slots `slots`, each row seeing
 * the slots whose bit is set in vis_bits[t][0..max_slots/64).  The 4-D additive mask of the
 * reference (beamSD.py:89,204-209) is never materialised.  Logits (fp32, row stride
 * atspeed_llama_logits_ld()) of the LAST n_logit_rows tokens go to the handle's logits
 * buffer (atspeed_llama_logits()) or to logits_out_dev when not NULL. */
int atspeed_llama_forward(atspeed_llama* m, const int32_t* ids_dev, const int32_t* pos_dev,
                          const int32_t* slots_dev, const uint64_t* vis_bits_dev, int32_t n_tokens,
                          int32_t n_slots_visible, int32_t n_logit_rows, float* logits_out_dev, void* stream);
/* n independent sequences as ONE forward (generate_teacher_data.py:225-232 scores the label and the K beams of every sample;
 * the reference runs one sample at a time).  Host arrays of n device pointers / counts; sequence i gets KV arena i of a pool the
 * handle owns (grown on demand), so slot numbers are private to a sequence.  The logits of the last n_logit_rows[i] rows of
 * sequence 0, 1, ... follow each other in logits_out_dev (row stride atspeed_llama_logits_ld()).  n <= 256. */
int atspeed_llama_forward_batch(atspeed_llama* m, int32_t n, const int32_t* const* ids_dev, const int32_t* const* pos_dev,
                                const int32_t* const* slots_dev, const uint64_t* const* vis_bits_dev, const int32_t* n_tokens,
                                const int32_t* n_slots_visible, const int32_t* n_logit_rows, float* logits_out_dev, void* stream);
float* atspeed_llama_logits(atspeed_llama* m);
/* Copy the first `bytes` of one of the handle's buffers to dst_dev, ordered on `stream` (what tests compare after a forward): the logits buffer
 * (atspeed_llama_logits()), the log-sum-exp over the whole vocabulary of each logit row of the last forward (fp32 [n_logit_rows]), or the K / V
 * arena `index` of the pool atspeed_llama_forward_batch gives its sequences ([layers][max_slots][hidden] in the model's type each; zero-filled
 * when created), or the residual-stream buffer [tokens][hidden] in the model's type: after a forward it holds the last layer's output, after a
 * row-pruned one (switch "tail_rows_tokens") the residual stream in front of the last layer's o_proj -- no part of the engine reads it.  More bytes than the buffer holds, or an arena the pool does not have: ATSPEED_ERR_INVALID. */
enum { ATSPEED_READ_LOGITS = 0, ATSPEED_READ_LSE = 1, ATSPEED_READ_BATCH_K = 2, ATSPEED_READ_BATCH_V = 3, ATSPEED_READ_HIDDEN = 4 };
int atspeed_llama_read(atspeed_llama* m, int32_t what, int32_t index, void* dst_dev, size_t bytes, void* stream);
/* hipEvent brackets around the forward's five GEMM kinds (0 qkv, 1 o_proj, 2 gate_up+SwiGLU, 3 down,
 * 4 lm_head), recorded on the launch stream.  Returns the sums since the last reset in ms_out[5] /
 * count_out[5] / rows_out[5] (sum of M); enable = 1/0 switches the brackets on/off and resets,
 * enable < 0 only reads.  Measurement hook for bench.py's roofline (no reference counterpart). */
int atspeed_llama_profile(atspeed_llama* m, int32_t enable, double* ms_out, int64_t* count_out, int64_t* rows_out);
/* The same accumulators restricted to launches of >= 1024 tokens (the 256x256 ring kernel's launches): read BEFORE the
 * atspeed_llama_profile call that resets them.  bench.py's roofline uses these so that its average launch time is
 * that of one kernel (gemm_ring_kernel<EPI, 8, false>) and can be checked against the rocprofv3 kernel summary. */
int atspeed_llama_profile_big(atspeed_llama* m, double* ms_out, int64_t* count_out, int64_t* rows_out);
/* Token counts of the forwards this model ran since logging was switched on: enable = 1 starts (and clears) the log, 0 stops it, < 0
 * only reads.  Writes up to `max_pairs` (tokens, logit rows) pairs, oldest first, to pairs_out (may be NULL) and returns how many forwards
 * the log holds (it keeps the first 4096).  bench.py prices every forward of a decode against max(weight stream, MFMA time) with these:
 * the packed verification of beamSD.py:203-221 makes the token count of a forward data dependent.  No reference counterpart. */
int32_t atspeed_llama_forward_log(atspeed_llama* m, int32_t enable, int32_t* pairs_out, int32_t max_pairs);
/* Measured peaks for the roofline report (nominal peaks are re-measured on the box).  No reference counterpart.
 * atspeed_probe_mfma_bf16: register-only loop of v_mfma_f32_16x16x32_bf16 on random operands, `iters` trips of 32 MFMAs per wave,
 * 8 waves x 1024 workgroups; scratch_dev >= 2 MiB.  atspeed_probe_hbm_read: `reps` read-only passes over buf_dev (use a buffer far
 * larger than the 256 MB Infinity Cache); scratch_dev >= 4 bytes.  Both time themselves with HIP events on `stream` and synchronise. */
int atspeed_probe_mfma_bf16(int32_t iters, void* scratch_dev, size_t scratch_bytes, void* stream, double* tflops_out);
int atspeed_probe_hbm_read(const void* buf_dev, size_t bytes, int32_t reps, void* scratch_dev, void* stream, double* gbs_out);
int32_t atspeed_llama_logits_ld(const atspeed_llama* m);
/* BASELINE config 5 (fp8 target verification): build OCP-e4m3 copies of the layer projections (per-output-row scales,
 * library-owned) from the bf16 weights.  From then on the batched forwards (M >= 512 tokens, shapes that fill the chip)
 * quantise activations per token and run W8A8 MFMA GEMMs (v_mfma_f32_16x16x32_fp8_fp8, fp32 accumulate); smaller
 * forwards, the lm_head, norms, attention and the KV cache stay bf16.  No reference counterpart (its target is int8
 * weights via bitsandbytes, inference.py:88). */
int atspeed_llama_enable_fp8(atspeed_llama* m, void* stream);
/* how many launches of each layer projection (0 qkv, 1 o_proj, 2 gate_up, 3 down; one per layer per forward) ran as an fp8 GEMM
 * (fp8_out[4]) and how many as a bf16 / fp32 GEMM (other_out[4]) since the last reset: lets a test or a bench state that config 5
 * really ran its projections in fp8 rather than fell back by shape.  Either output may be NULL.  No reference counterpart. */
int atspeed_llama_fp8_counters(atspeed_llama* m, int64_t* fp8_out, int64_t* other_out, int32_t reset);
/* 4-bit target (W4A8 on the block-scaled MFMA, v_mfma_scale_f32_16x16x128_f8f6f4 with an e2m1 A operand): build library-owned OCP MXFP4
 * copies of the four layer projections from the model's own 16-bit weights -- per row, blocks of 32 consecutive k with one E8M0 scale byte
 * 127 + X, X = clamp(floor(log2(amax)) - 2, -127, 127), elements e2m1(v / 2^X) rounded to nearest (ties to the even mantissa), saturating at
 * 6 (INTEGRATION.md "4-bit target").  From then on EVERY forward runs qkv, o_proj, gate_up and down as W4A8 (activations exactly the W8A8
 * ones: per-token e4m3, fp32 scale; fp32 accumulation); embedding, norms, attention, KV cache and lm_head stay 16-bit.  Refused
 * (ATSPEED_ERR_INVALID, atspeed_last_error says why): fp32 models, hidden or ffn not a multiple of 256, a model with fp8 copies
 * (atspeed_llama_enable_fp8 in turn refuses a model with fp4 copies).  A second call is a no-op.  Opt-in: MXFP4 without rotation or
 * outlier handling costs model quality on real checkpoints. */
int atspeed_llama_enable_fp4(atspeed_llama* m, void* stream);
/* as atspeed_llama_fp8_counters for the 4-bit target: launches of each layer projection that ran as W4A8 (fp4_out[4]) and as 16-bit / fp32
 * GEMMs (other_out[4]) since the last reset */
int atspeed_llama_fp4_counters(atspeed_llama* m, int64_t* fp4_out, int64_t* other_out, int32_t reset);
/* how many qkv projections (one per layer per forward) ran with the rotary embedding and the KV-cache scatter in the GEMM's epilogue
 * (batched bf16 forwards, head_dim 128, hidden % 256 == 0: the reference's apply_rotary_pos_emb + cache update, modeling_llama.py as
 * called from beamSD.py:120, without re-reading the projection) rather than as the separate pass, since the last reset; -1 on a NULL
 * model.  The switch "fuse_qkv_rope" (atspeed_set_switch; initial value ATSPEED_FUSE_QKV_ROPE, default 1) = 0 selects the separate pass:
 * results are bit-identical.  Since round 6 ONE user's W8A8 qkv projection (1-256 tokens, 150-256 unsplit tiles of 64 weight rows: Llama-7B's
 * 192) carries the same epilogue in the weight-streaming kernel. */
int64_t atspeed_llama_rope_fused_launches(atspeed_llama* m, int32_t reset);
/* bytes of the split-K arena this model owns (0: none yet -- it is allocated in front of the model's first forward of >= 257 tokens, so a
 * draft or a one-user target never holds one; thin ring-kernel grids of a model without one take the device's shared arena or the plain grid) */
int64_t atspeed_llama_sk_arena_bytes(const atspeed_llama* m);

/* ---- LoRA adapter kept beside the base weights (peft's unmerged forward: the reference wraps its 8-bit base with
 * PeftModel.from_pretrained, code/inference.py:86-100).  For an adapted module m of q / k / v of a layer, in the model's dtype T with fp32
 * accumulation inside each product (round = to T; the fp32 engine rounds nothing):
 *   u = round(A_m xn),  d = round(B_m u),  y = round(base + round(scaling * d))
 * xn = the layer's input RMSNorm output, base = the projection's T output (16-bit, W8A8 or W4A8 base alike); RoPE and the KV scatter then
 * work on y.  A model with an adapter runs per layer one shrink launch (all three modules), the qkv projection with its plain store, and the
 * RoPE pass that adds the adapter's term first -- no fused RoPE epilogue, no split-K slab hand-off.  A model without one runs launch for
 * launch as if this section did not exist. */
#define ATSPEED_LORA_MAX_RANK 64
/* one layer's adapter, DEVICE pointers in the model's dtype, HF / peft layout: A [rank][hidden] (lora_A.weight), B [hidden][rank]
 * (lora_B.weight), row-major and dense; a NULL (A, B) pair = that module is not adapted (one NULL half of a pair is refused) */
typedef struct atspeed_lora_layer { const void *a_q, *b_q, *a_k, *b_k, *a_v, *b_v; } atspeed_lora_layer;
/* Give the model an adapter, replacing the one it has: layers = HOST array of cfg.n_layers entries.  Memory contract: the library copies
 * every A and B into zero-padded device copies of its own (one allocation, (3 * R16 * hidden + 3 * hidden * R16) elements per layer, R16 = rank
 * rounded up to 16) on `stream` and waits for the copies, so the caller's tensors may be freed on return; it also allocates the model's
 * lora_A output buffer (once, sized for rank 64) -- nothing is allocated inside a forward afterwards.  Waits for the device to be idle and
 * drops the model's captured graphs.  On failure the model is as it was.  1 <= rank <= ATSPEED_LORA_MAX_RANK, finite scaling (alpha / rank,
 * or alpha / sqrt(rank) for rslora), at least one adapted module. */
int atspeed_llama_set_lora(atspeed_llama* m, int32_t rank, float scaling, const atspeed_lora_layer* layers, void* stream);
/* remove the adapter (no-op without one): waits for the device, frees the copies, drops the captured graphs; later forwards are bit for bit
 * those of a model that never had one */
int atspeed_llama_clear_lora(atspeed_llama* m);
/* shrink + expand launches since the last reset (2 per layer per forward with an adapter, 0 without); -1 on a NULL model */
int64_t atspeed_llama_lora_launches(atspeed_llama* m, int32_t reset);

/* ---- several RESIDENT adapters on one model, picked per user.  A model holds up to ATSPEED_LORA_MAX_ADAPTERS adapters in
 * slots 1 .. 16, each with its own rank and scaling; every user of a forward, a lock-step batch or a session names one of them (or 0 = none)
 * and the two side-path kernels pick the adapter per token row.  The arithmetic per row is that of the model-wide adapter above.
 * atspeed_llama_add_lora: atspeed_llama_set_lora's arguments, checks and memory contract (library-owned zero-padded copies in one allocation
 *   per adapter, made on `stream` and waited for: the caller's tensors may be freed on return; the lora_A output buffer is made sure of here,
 *   nothing is allocated inside a forward afterwards); the adapter goes into the lowest free slot, returned in *slot_out.  No free slot:
 *   ATSPEED_ERR_CAPACITY, and the model is as it was.
 * atspeed_llama_remove_lora: frees the slot (ATSPEED_ERR_INVALID for one that is not occupied).  Removing a slot that a decoder still names
 *   makes that decoder's next generate call return ATSPEED_ERR_INVALID before anything is launched; removing one that a queued or in-lane
 *   user of a live session names is the caller's error: the round that finds it returns ATSPEED_ERR_INVALID and ends the users in lanes, as
 *   any failed round does.
 * Both wait for the device to be idle and drop the model's captured graphs.  The kernels read the slots from a device table the model owns,
 *   at a fixed address and rewritten by these two calls alone, and the user's slot from the segment table, so a captured forward stays valid
 *   whatever the users of a later replay name.
 * The model-wide adapter and resident slots exclude each other: atspeed_llama_set_lora on a model with occupied slots and atspeed_llama_add_lora
 *   on a model that holds a model-wide adapter return ATSPEED_ERR_INVALID.
 * A model with at least one occupied slot runs every forward as a model with an adapter does (one shrink and one expand launch per layer,
 *   counted by atspeed_llama_lora_launches; plain qkv store, no fused RoPE epilogue, no row-pruned tail, no staged verification), whatever
 *   its users name; rows of slot 0 take the unadapted arithmetic bit for bit.  After the last slot is removed the model runs launch for launch
 *   as one that never had an adapter. */
#define ATSPEED_LORA_MAX_ADAPTERS 16
/* one slot of one layer as the kernels read it (the model's table, and the bare kernel entry points below): DEVICE pointers in the model's
 * dtype to the stacked zero-padded A_cat [3 r16][hidden] (q, k, v thirds; an absent module's rows are zero) and B_m [hidden][r16] (NULL =
 * module not adapted), r16 = rank rounded up to 16 (16 .. 64); entry 0 of a table means "none" and is never read */
typedef struct atspeed_lora_slot { const void *a_cat, *b_q, *b_k, *b_v; int32_t r16; float scaling; } atspeed_lora_slot;
int atspeed_llama_add_lora(atspeed_llama* m, int32_t rank, float scaling, const atspeed_lora_layer* layers, void* stream, int32_t* slot_out);
int atspeed_llama_remove_lora(atspeed_llama* m, int32_t slot);
int32_t atspeed_llama_lora_slots(const atspeed_llama* m);          /* occupied slots; -1 on a NULL model */
/* atspeed_llama_forward_batch with one resident slot per sequence: adapters = HOST array [n] of slots (0 = none), NULL = all 0.  A slot that is
 * not occupied: ATSPEED_ERR_INVALID before anything is launched. */
int atspeed_llama_forward_batch_adapters(atspeed_llama* m, int32_t n, const int32_t* const* ids_dev, const int32_t* const* pos_dev,
                                         const int32_t* const* slots_dev, const uint64_t* const* vis_bits_dev, const int32_t* n_tokens,
                                         const int32_t* n_slots_visible, const int32_t* n_logit_rows, const int32_t* adapters /* [n], NULL = all 0 */,
                                         float* logits_out_dev, void* stream);

/* lm_head fused with the full-vocabulary normaliser of beamSD.py:58,285 (log_softmax over ALL columns, before masking): bf16
 * x [rows, hidden] times w [vocab, hidden]^T -> fp32 logits (row stride ld) and lse[row] = log sum_v exp(logits[row][v]).  On the
 * batched path (rows >= 257 and a tile grid that fills the chip) the (max, sum exp) partials come out of the GEMM epilogue, the
 * logits are never re-read, and with `fsm` given only the 256-column tiles that hold a token of the automaton are written (the
 * others are never read by a step: Beauty 5 of 129 tiles) -- *fused_out = 1; otherwise the plain GEMM + atspeed_lse_rows (0).
 * workspace: at least rows * ceil(vocab / 256) * 8 bytes for the fused path (+ the split-K slabs of the small path).  This is what
 * the decoder's forwards run; standalone for tests and benches.
 * Memory contract (tests/test_guard_bands_gpu.py::test_lmhead_lse_guard_bands, both paths): x_dev and w_dev 16-byte aligned; of the
 * logits only [rows][0 .. vocab) is written (columns vocab .. ld - 1 and everything outside the rows stay untouched), lse_dev gets `rows`
 * floats, nothing from workspace_bytes on is written; weight rows >= vocab and x rows >= rows influence no result. */
int atspeed_lmhead_lse(const void* x_dev, const void* w_dev, float* logits_dev, float* lse_dev, int32_t rows, int32_t vocab,
                       int32_t hidden, int32_t ld, const atspeed_fsm* fsm /* may be NULL */, void* workspace_dev, size_t workspace_bytes,
                       int32_t* fused_out /* may be NULL */, void* stream);

/* ------------------------------------------------------------------ scan kernels
 * log-softmax normaliser over the FULL vocabulary, before masking (beamSD.py:58,285):
 * lse[r] = log(sum_v exp(logits[r][v])).  Rows are `ld` floats apart. */
int atspeed_lse_rows(const float* logits_dev, int32_t n_rows, int32_t vocab, int32_t ld,
                     float* lse_out_dev, void* stream);

/* out[r][c] = logits[r][c] - lse[r] for c < vocab: the log-softmax rows (beamSD.py:58) as a tensor, for callers that must hand them to
 * host-side logits processors (beamSD.py:62-64 with a non-empty LogitsProcessorList); the decoder itself never materialises them. */
int atspeed_log_softmax_rows(const float* logits_dev, int32_t ld, const float* lse_dev, int32_t n_rows, int32_t vocab, float* out_dev,
                             int32_t ld_out, void* stream);

/* Fused constraint mask + beam expand + prune (beamSD.py:60-87):
 *   cand(r, t) = logits[r][t] - lse[r] + beam_score[r]   for t allowed at node[r]
 *   top-k by (score desc, flat id r*vocab+t asc)  ->  out_*[0..k)
 * -inf / missing candidates are flagged out_flat = -1 (never a beam).
 * Standalone form used by tests; the decoder uses the same device code inside its step
 * kernels together with the mask/position bookkeeping (beamSD.py:88-91). */
int atspeed_beam_expand_prune(const float* logits_dev, int32_t ld, const float* lse_dev,
                              const float* beam_score_dev, const int32_t* beam_node_dev, int32_t n_rows,
                              const atspeed_fsm* fsm, int32_t k,
                              float* out_score_dev, int32_t* out_parent_dev, int32_t* out_token_dev,
                              int32_t* out_node_dev, int32_t* out_flat_dev, void* stream);

/* The same without a mask (beamSD.py:58,69-78 with an empty processor list; also the expand of rows that a host-side logits
 * processor has already rewritten: pass lse = 0): candidates are ALL `vocab` columns of each row; -inf entries are never picked.
 * atspeed_row_topk: out_tokens[r][ATSPEED_MAX_BEAMS] = the k best columns of row r (value desc, column asc; -1 = fewer finite ones) --
 * the k best (row, token) pairs lie among them.  Equal values rank by column, lowest first, and -0.0 equals +0.0 (a plateau of a
 * rewritten row yields its lowest columns).  row_cand_ws_dev: n_rows * ATSPEED_MAX_BEAMS int32 of scratch. */
int atspeed_row_topk(const float* scores_dev, int32_t n_rows, int32_t vocab, int32_t ld, int32_t k, int32_t* out_tokens_dev, void* stream);
int atspeed_beam_expand_prune_free(const float* logits_dev, int32_t ld, const float* lse_dev, const float* beam_score_dev, int32_t n_rows,
                                   int32_t vocab, int32_t k, int32_t* row_cand_ws_dev, float* out_score_dev, int32_t* out_parent_dev,
                                   int32_t* out_token_dev, int32_t* out_flat_dev, void* stream);

/* Top-K-aligned acceptance test (beamSD.py:371-380): accept iff every target id is among
 * the draft ids.  hit[r] = r-th smallest draft position that was hit, score_by_hit[r] = the
 * target score of that entry (beamSD.py:295-296,373-376).  out_accept = 1/0. */
int atspeed_accept(const int32_t* target_flat_dev, const float* target_score_dev, int32_t k,
                   const int32_t* draft_flat_dev, int32_t dk,
                   int32_t* hit_out_dev, float* score_by_hit_out_dev, int32_t* accept_out_dev, void* stream);

/* ------------------------------------------------------------------ decoder
 * Replaces BSSD() (beamSD.py:458-542) and target_generate() (beamSD.py:544-595) for one
 * user stream: draft steps, the packed target verification forward, verify(), and all
 * bookkeeping (masks as bitsets, positions, KV slots, beam suffixes) stay on the device;
 * the host reads back one small mailbox per round. */
typedef struct atspeed_decoder atspeed_decoder;
int atspeed_decoder_create(atspeed_llama* target, atspeed_llama* draft /* may be NULL */,
                           int32_t max_prompt, atspeed_decoder** out);
void atspeed_decoder_destroy(atspeed_decoder* d);

/* Sampling mode of a decoder (generation_config.do_sample / temperature; beamSD.py:65-75 draft and final steps,
 * :293-321,332-369 verification, :529-531 final sort).  Off by default: every BASELINE config is greedy.  Draws are
 * counter-based functions of (seed, round, step, candidate), so a call is reproducible and the CPU restatement
 * (oracle/beamsd_sample_ref.py, HashRng) makes the same decisions; the law is that of the reference's torch.multinomial /
 * rand / randperm draws (statistical parity).  Applies to the bssd and target_generate calls made with this decoder. */
int atspeed_decoder_set_sampling(atspeed_decoder* d, int32_t do_sample, float temperature, uint32_t seed);

/* Sampling-mode warpers of a decoder: what transformers' `_get_logits_warper` puts after the temperature for a beam search,
 * TopKLogitsWarper(top_k, min_tokens_to_keep) then TopPLogitsWarper(top_p, min_tokens_to_keep) (beamSD.py:479-481, applied at :65-66 and
 * :293-294).  top_k = 0 and top_p >= 1 switch a warper off (the default: both off, nothing new is launched and every result is what it was
 * without this call); min_tokens_to_keep is 2 for a beam search with more than one beam, else 1.  Only sampled calls look at them: in
 * every sampled step and verify walk a candidate below its row's cutoff is absent (score -inf, probability 0) for the draws, the
 * draft's q, the target's p, the residual and the bonus draw. */
int atspeed_decoder_set_warpers(atspeed_decoder* d, int32_t top_k, float top_p, int32_t min_tokens_to_keep);

/* The kernel behind it, bare: cutoffs_out[r] for r < n_rows, where row r of `logits` (leading dimension ld, normaliser lse[r]) sits at
 * automaton node nodes[r] and its entries are that node's children scored s = (logit - lse) / temperature.
 *   top-k: k' = max(top_k, min_tokens_to_keep); with at least k' finite entries everything strictly below the k'-th largest is cut
 *          (ties with it survive), with fewer nothing is;
 *   top-p: on what top-k left, in descending order an entry is kept while the softmax mass strictly above it is below top_p, the first
 *          min_tokens_to_keep always.
 * A candidate survives iff s >= cutoffs_out[r]; -inf = nothing cut (both warpers off, or a row without finite entries).  Rows of any
 * length: up to 1024 children are sorted in LDS, longer lists go through a radix select.  atspeed_warp_cutoff_launches: launches of
 * this kernel by the process so far, decoders included (greedy calls and calls with both warpers off make none). */
int atspeed_warp_cutoffs(const float* logits_dev, int32_t ld, const float* lse_dev, int32_t n_rows, const atspeed_fsm* fsm,
                         const int32_t* nodes_dev, float temperature, int32_t top_k, float top_p, int32_t min_tokens_to_keep,
                         float* cutoffs_out_dev, void* stream);
int64_t atspeed_warp_cutoff_launches(void);

typedef struct atspeed_gen_stats {
  int32_t n_run;               /* verification rounds (beamSD.py:527)                 */
  int32_t total_accept_steps;  /* sum of n_matches (beamSD.py:528)                    */
  int32_t accept_steps[ATSPEED_MAX_NEW_TOKENS];
  int32_t n_valid;             /* beams with a finite score                           */
  int32_t n_target_forwards, n_draft_forwards;
  float draft_ms, target_ms, verify_ms, total_ms;   /* hipEvent stage times (Timer, beamSD.py:12-37) */
  int32_t status;              /* batched calls: ATSPEED_OK, or ATSPEED_ERR_FILTERED for a user whose step lost every beam to the id
                                  filter of beamSD.py:80-86 -- that user ends with n_valid = 0, the rest of the batch finishes (the
                                  one-user calls return the error instead)                */
  int32_t n_target_passes;     /* passes over the target's weights that included this user: n_target_forwards, plus one per further phase
                                  of a round verified in stages (switch "verify_staged")  */
} atspeed_gen_stats;

/* prompt_ids_dev: [prompt_len] int32.  out_tokens_dev: [k][max_new_tokens] int32 generated
 * suffixes ordered by score desc; out_scores_dev: [k] fp32.  Synchronises `stream` once per
 * round (to read n_matches) and at exit. */
int atspeed_bssd_generate(atspeed_decoder* d, const int32_t* prompt_ids_dev, int32_t prompt_len,
                          const atspeed_fsm* fsm, int32_t start_node, int32_t gamma, int32_t max_new_tokens,
                          int32_t k, int32_t dk, int32_t* out_tokens_dev, float* out_scores_dev,
                          atspeed_gen_stats* stats_host, void* stream);

/* Staged verification (switches "verify_staged", "verify_staged_tokens", "verify_staged_pass_tokens"): a greedy round of
 * atspeed_bssd_generate_batch or of a session may forward the round inputs first and then one draft block per phase, only for the users whose
 * verify walk still needs it; each phase but the last ends with one more synchronisation of the stream.  Tokens, accepted steps and
 * n_target_forwards are the packed round's, scores to fp32 rounding; n_target_passes counts the phases.  atspeed_bssd_generate never stages. */
/* n independent users, one decoder each, interleaved on the decoders' private streams (the reference runs users
 * strictly one after another, inference.py:162-176): hides the per-round mailbox sync and the launch latency of
 * the small forwards, and lets forwards of different users overlap.  Results equal n sequential calls. */
int atspeed_bssd_generate_batch(atspeed_decoder** decoders, int32_t n, const int32_t* const* prompt_ids_dev,
                                const int32_t* prompt_lens, const atspeed_fsm* fsm, const int32_t* start_nodes,
                                int32_t gamma, int32_t max_new_tokens, int32_t k, int32_t dk,
                                int32_t* const* out_tokens_dev, float* const* out_scores_dev,
                                atspeed_gen_stats* stats_host /* [n] */, void* stream);

/* ------------------------------------------------------------------ sessions: a queue of users over a fixed set of lanes
 * atspeed_bssd_generate_batch decodes a fixed list in lock step: a user that finishes leaves its place empty until the slowest user of the
 * call is done.  A session keeps `n_lanes` decoders (lanes) busy instead: users are submitted to a host queue at any time, and at every round
 * boundary each free lane takes the next queued user (in submission order) before the round runs.  A round is exactly the round of the batch
 * call -- draft steps, ONE target forward (packed, or verified in stages: below), verify / final steps, exports, one stream synchronisation per
 * phase -- over the occupied lanes; a user's
 * prompt is ingested inside its first round's forwards.  Every user's result equals its own atspeed_bssd_generate call (scores to fp32
 * rounding, as in the batch call).  No reference counterpart (the reference decodes one user at a time, inference.py:162-176).
 *
 * Ownership: the lanes' decoders, the automaton and the models belong to the caller and must outlive the session; the session never creates or
 * destroys a decoder, and a lane must not be used by another call while the session holds a user on it.  Per user, prompt_dev, out_tokens_dev
 * [k][max_new_tokens], out_scores_dev [k] and stats_host must stay valid from submit until the user's ticket has been returned by
 * atspeed_session_round / _drain (the statistics are written by then; the result block is written -- for a filtered user blanked -- in stream order,
 * so it is read on the session's stream or after synchronising it).  One host thread drives a session.
 *
 * atspeed_session_create: lanes[n_lanes] (1 .. 256) of ONE target / draft pair, each with max_prompt capacity >= `max_prompt`, all in the
 * same sampling mode, temperature and warpers (else ATSPEED_ERR_INVALID).  Makes every allocation a round can need: the models' activation
 * buffers for the worst round (n_lanes x (max(max_prompt, k) + gamma x dk) target tokens), the staging ring and stage events, and -- when that
 * round reaches 257 tokens on a 16-bit model -- the split-K arena that otherwise appears in front of the first large forward.  An arena that
 * cannot be had does not fail the call: atspeed_last_error says so and the counter arena_failed is set.
 * atspeed_session_submit: queues one user (launches nothing) and returns its ticket (1, 2, ... in submission order) in *ticket_out.  `seed` is
 * the user's sampling stream (ignored by greedy lanes): it is put on the lane the user is admitted to, so draws follow users, not lanes.  A
 * prompt longer than max_prompt returns ATSPEED_ERR_CAPACITY and leaves the session as it was; so does a prompt whose rounds could need more KV
 * slots than the models have (prompt_len + (max_new_tokens - 1) x dk: every draft block of the call kept) -- the lock-step calls find that only in
 * the round that runs out, where it would end every user of the round.
 * atspeed_session_round: admission (per free lane the next queued user; one prompt-init launch for all of them), one round, retirement.  One record per user that
 * finished goes to done_out[0 .. *n_out) (cap >= n_lanes always suffices; with less room the call is refused before it launches anything):
 * its ticket, the lane it held, its status, and how many rounds of the session it waited in the queue and spent in its lane.
 * A user whose step lost every beam to the id filter retires with stats.status = ATSPEED_ERR_FILTERED, n_valid = 0 and a blanked result block
 * (scores -inf, tokens 0), as in the batch call; the other lanes go on.  With nothing queued and no lane occupied the call does nothing and
 * returns ATSPEED_OK with *n_out = 0.  Any other error is returned by the call and ends the users then in lanes: the lanes are freed,
 * and the NEXT round / drain call hands out their records with that error as status (stats_host->status likewise, n_valid = 0, result block
 * undefined), so every ticket still comes back exactly once; queued users are untouched.
 * atspeed_session_drain: rounds until queue and lanes are empty; records as above, cap >= users pending (queued + in lanes), else
 * ATSPEED_ERR_CAPACITY before anything is launched.  A round that fails ends the drain with its error; the records of that round's users and of
 * users that finished in earlier rounds of that drain are handed out by the next round / drain call.
 * Stage times: a round's stage time is shared equally by the users active in it; n_target_forwards / n_draft_forwards stay per user. */
typedef struct atspeed_session atspeed_session;
typedef struct atspeed_session_counters {
  int64_t rounds;                  /* rounds that ran (empty rounds do not count)                                  */
  int64_t target_forwards;         /* target forwards launched (one per round, whether packed or verified in stages)  */
  int64_t draft_forwards;          /* draft forwards launched (up to gamma per round)                               */
  int64_t lane_rounds;             /* sum over rounds of the lanes occupied in it                                   */
  int64_t users_admitted, users_retired;
  int64_t allocs_after_create;     /* on-demand allocations the library made while this session's rounds ran: stays 0.  Counted: activation
                                      buffers, a model's and the device's shared split-K arena, staging ring, stage and profiling events, graph
                                      capture stream and graph instantiations (switch "graphs"), decoders' sampling tables.  The count is
                                      process-wide: what another host thread makes the library allocate during a round is charged here too */
  int32_t arena_reserved;          /* 1: the target owns its split-K arena                                          */
  int32_t arena_failed;            /* 1: create wanted the arena and could not get it                               */
  int32_t n_lanes, lanes_occupied; /* now                                                                           */
  int64_t queued;                  /* users submitted and not yet admitted                                          */
  int64_t target_passes;           /* passes over the target's weights launched: target_forwards, plus one per further phase of a round
                                      verified in stages (switch "verify_staged")                                    */
} atspeed_session_counters;
int atspeed_session_create(atspeed_decoder* const* lanes, int32_t n_lanes, const atspeed_fsm* fsm, int32_t gamma, int32_t max_new_tokens,
                           int32_t k, int32_t dk, int32_t max_prompt, void* stream, atspeed_session** out);
int atspeed_session_submit(atspeed_session* s, const int32_t* prompt_ids_dev, int32_t prompt_len, int32_t start_node, uint32_t seed,
                           int32_t* out_tokens_dev, float* out_scores_dev, atspeed_gen_stats* stats_host, int64_t* ticket_out);
typedef struct atspeed_session_done {
  int64_t ticket;
  int32_t lane, status;            /* ATSPEED_OK, ATSPEED_ERR_FILTERED, or the error of the round that ended it (= stats_host->status) */
  int64_t rounds_queued;           /* rounds the session ran between this user's submit and its admission           */
  int64_t rounds_in_lane;          /* rounds it took part in                                                        */
} atspeed_session_done;
int atspeed_session_round(atspeed_session* s, atspeed_session_done* done_out, int32_t cap, int32_t* n_out);
int atspeed_session_drain(atspeed_session* s, atspeed_session_done* done_out, int32_t cap, int32_t* n_out);
int atspeed_session_get_counters(const atspeed_session* s, atspeed_session_counters* out);
void atspeed_session_destroy(atspeed_session* s);   /* frees the session's own tables only: the lanes' decoders are not touched */

/* ------------------------------------------------------------------ item filters: exclude or allow lists per user
 * All users of a call share ONE automaton and differ in their start node; a filter adds, per user, a bitset over the automaton's node ids
 * (bit 1 = blocked) that every walk of the automaton consults.  No reference counterpart: there a per-user filter is a Python closure around
 * the mask function, called per beam per step.
 *
 * A filter is a list of token sequences: the tokens a beam generates after the prompt (for a strict item trie an item's code tokens, with or
 * without the EOS), each walked through the automaton from the user's start node.
 *   - a sequence with a token that has no edge is UNKNOWN: ignored, and counted per user (unknown_out);
 *   - an empty sequence, or one longer than ATSPEED_MAX_NEW_TOKENS, is ATSPEED_ERR_INVALID;
 *   - the END NODE of a sequence is the node it leads to; it need not be a leaf.
 * ATSPEED_MASK_BLOCK: B = the end nodes of the known sequences, closed bottom-up along the listed paths: a node on a listed path, the start
 *   node included, all of whose children are in B, is in B -- so a live beam never stands on a node with no way on.  No sequences: all bits
 *   0, the run equals an unfiltered one.
 * ATSPEED_MASK_ALLOW: K = every node on a known path (the start node included), E = the end nodes.  A node is blocked iff it is a child of a
 *   node in K \ E and not itself in K.  An end node's own children stay free (with a sequence that is a prefix of another, the end node
 *   wins there); nodes that are no children of a path node keep bit 0, they cannot be reached.
 * Bits at or above n_nodes are 0.  status_out[u] = ATSPEED_ERR_CONSTRAINT when user u's start node ends up blocked (block mode) or the user
 * has no known sequence (allow mode), else ATSPEED_OK: HF's "returned an empty list" case, for the caller to refuse before it launches.
 * The automaton must be a tree below the start nodes (whatever atspeed_trie_flatten produces is one).
 *
 * Decoding: a candidate (row r, child edge e) is absent iff the bit of the node the edge leads to is set -- treated exactly like a candidate
 * below a warper cutoff: no key, score -inf, probability 0; the warper cutoffs are taken over the unblocked children only.  A live row all of
 * whose children are blocked contributes nothing and raises no error; with fewer than k survivors the tail picks are "not a beam" (flat -1)
 * and n_valid says how many are real.  Draft and target see the same bits, so beam-SD under a filter equals plain beam search under it.
 *
 * atspeed_node_masks_create: all arrays are HOST pointers.  User u owns sequences [user_seq_offsets[u], user_seq_offsets[u + 1]); sequence s
 *   is seq_tokens[seq_offsets[s] .. seq_offsets[s + 1]).  The bitsets are built on the device (the automaton lives there; the library keeps
 *   no host copy), one workgroup per user; the call synchronises `stream`.  Every allocation is made here.
 * atspeed_node_masks_read: user's ceil(n_nodes / 32) words to the host (tests).
 * atspeed_decoder_set_node_mask: the filter of `user` for the generate calls made with this decoder (one user, batch, target_generate(_batch)),
 *   like the sampling mode; masks = NULL clears it.  The masks must have been built on the automaton the call uses (else the call returns
 *   ATSPEED_ERR_INVALID) and stay alive while set.
 * atspeed_session_submit_masked: atspeed_session_submit with a filter (masks = NULL: none).  It goes onto the lane at the user's admission and
 *   off at its retirement -- it follows the user, not the lane -- and must stay valid until the ticket has come back. */
typedef struct atspeed_node_masks atspeed_node_masks;
#define ATSPEED_MASK_BLOCK 0
#define ATSPEED_MASK_ALLOW 1
int atspeed_node_masks_create(const atspeed_fsm* fsm, int32_t n_users, const int32_t* start_nodes, const int32_t* seq_tokens,
                              const int32_t* seq_offsets, const int32_t* user_seq_offsets, int32_t mode, int32_t* unknown_out /* [n_users], may be NULL */,
                              int32_t* status_out /* [n_users] */, void* stream, atspeed_node_masks** out);
void atspeed_node_masks_destroy(atspeed_node_masks* masks);
int atspeed_node_masks_read(const atspeed_node_masks* masks, int32_t user, uint32_t* words_out_host, int32_t n_words);
int atspeed_decoder_set_node_mask(atspeed_decoder* d, const atspeed_node_masks* masks, int32_t user);
int atspeed_session_submit_masked(atspeed_session* s, const int32_t* prompt_ids_dev, int32_t prompt_len, int32_t start_node, uint32_t seed,
                                  int32_t* out_tokens_dev, float* out_scores_dev, atspeed_gen_stats* stats_host,
                                  const atspeed_node_masks* masks, int32_t user, int64_t* ticket_out);
/* ---- a user's resident adapter (atspeed_llama_add_lora).
 * atspeed_decoder_set_adapter: the slot of the decoder's TARGET that the generate calls made with this decoder run under (atspeed_bssd_generate,
 *   _batch, atspeed_target_generate, _batch and every target forward they make); 0, the default, = none.  The draft model is never adapted.
 *   Like the sampling mode it stays until it is set again.  The slot is looked up when a generate call starts: one that is not occupied then
 *   makes the call return ATSPEED_ERR_INVALID before anything is launched.
 * atspeed_session_submit_ex: the session's one submit entry with every per-user property in a struct (struct_size = sizeof(atspeed_session_user):
 *   a shorter struct of an older caller leaves the members it does not have at 0); atspeed_session_submit and _submit_masked forward to it with
 *   adapter 0.  The adapter follows the user to whichever lane admits it, as the seed and the filter do, and is validated here. */
int atspeed_decoder_set_adapter(atspeed_decoder* d, int32_t slot);
typedef struct atspeed_prefix atspeed_prefix;          /* "prompt prefixes" below */
typedef struct atspeed_session_user {
  size_t struct_size;              /* sizeof(atspeed_session_user) of the caller's build                                */
  const int32_t* prompt_ids_dev; int32_t prompt_len; int32_t start_node; uint32_t seed;
  int32_t* out_tokens_dev; float* out_scores_dev; atspeed_gen_stats* stats_host;
  const atspeed_node_masks* masks; int32_t mask_user;   /* item filter, NULL = none (atspeed_session_submit_masked)     */
  int32_t adapter;                 /* resident slot of the session's target, 0 = none                                    */
  const struct atspeed_prefix* target_prefix;   /* prompt prefix of the session's target and of its draft ("prompt prefixes" below): both or  */
  const struct atspeed_prefix* draft_prefix;    /* neither; NULL = the whole prompt is prefilled                                              */
} atspeed_session_user;
int atspeed_session_submit_ex(atspeed_session* s, const atspeed_session_user* u, int64_t* ticket_out);
/* The step and the cutoff kernel alone under a filter (tests): their unmasked twins' arguments plus (masks, user); masks = NULL: the twin. */
int atspeed_beam_expand_prune_masked(const float* logits_dev, int32_t ld, const float* lse_dev,
                                     const float* beam_score_dev, const int32_t* beam_node_dev, int32_t n_rows,
                                     const atspeed_fsm* fsm, int32_t k,
                                     float* out_score_dev, int32_t* out_parent_dev, int32_t* out_token_dev,
                                     int32_t* out_node_dev, int32_t* out_flat_dev, const atspeed_node_masks* masks, int32_t user, void* stream);
int atspeed_warp_cutoffs_masked(const float* logits_dev, int32_t ld, const float* lse_dev, int32_t n_rows, const atspeed_fsm* fsm,
                                const int32_t* nodes_dev, float temperature, int32_t top_k, float top_p, int32_t min_tokens_to_keep,
                                float* cutoffs_out_dev, const atspeed_node_masks* masks, int32_t user, void* stream);

/* The sampled beam step alone (tests): one do_sample expand of n_rows beams, i.e. the step kernel with the sampling branch that
 * atspeed_beam_expand_prune never takes.  k picks are drawn without replacement with probability proportional to
 * exp((logit - lse) / temperature + beam score) over the children of every live beam's node (a child under its row's cutoff or behind a
 * blocked edge has probability 0), by the counter-based generator: rng_sub is what ats_rng_sub gives for (seed, purpose, round, step,
 * model).  filter_ids != 0 applies the automaton's post-top-k id filter (atspeed_fsm_set_id_filter): dropped picks leave the block, the
 * survivors keep their order and "no beam" (flat -1, score -inf) fills the end.  Outputs hold k entries each.  Optional, all NULL or none:
 * tab_score_dev [candidates in expand order], tab_off_dev [n_rows + 1], tab_lse_dev [1] -- the whole distribution as the verify walk reads
 * it.  Optional cutoffs_dev [n_rows] (atspeed_warp_cutoffs), optional mailbox_dev [4] int32 {n_matches, status, n_valid, pad}: n_valid is
 * written, status only when the step has one to report.  Refused before any launch: a NULL required pointer, ld <= 0, temperature <= 0, a
 * mask-free automaton (ATSPEED_ERR_INVALID); k or n_rows outside [1, ATSPEED_MAX_BEAMS] (ATSPEED_ERR_CAPACITY). */
int atspeed_beam_sample_step(const float* logits_dev, int32_t ld, const float* lse_dev, const float* beam_score_dev,
                             const int32_t* beam_node_dev, int32_t n_rows, const atspeed_fsm* fsm, const atspeed_node_masks* masks,
                             int32_t user, int32_t k, float temperature, uint32_t rng_sub, const float* cutoffs_dev, int32_t filter_ids,
                             float* out_score_dev, int32_t* out_parent_dev, int32_t* out_token_dev, int32_t* out_node_dev,
                             int32_t* out_flat_dev, float* tab_score_dev, int32_t* tab_off_dev, float* tab_lse_dev, int32_t* mailbox_dev,
                             void* stream);

/* One verify walk alone (tests), greedy or sampled: what a round hands its walk kernel, as device pointers and ints.
 *   Blocks: block 0 = the nb round beams, block i = the dk beams of draft step i, i <= dl.  score / node of blocks 0 .. dl and flat of
 *   blocks 1 .. dl are required; seq (block i: [rows][ATSPEED_MAX_NEW_TOKENS]) may be NULL (the suffixes then count as zeros).
 *   Logits: block i's first row of logits / lse / row_cand / cutoff is blk_row0[i] (a packed round: 0, nb, nb + dk, ...); blocks_ready =
 *   how many blocks have rows (greedy walk only: a walk that needs block i >= blocks_ready writes mailbox[0] = -1 and, if it has one,
 *   a status, and nothing else but the trace of the steps it took).
 *   Automaton: fsm (+ optional masks, user), or fsm = NULL for the mask-free search over `vocab` tokens (greedy only), whose candidates are
 *   the n_row_cand first entries of row_cand_dev [logit row][ATSPEED_MAX_BEAMS].
 *   cur_*: the packed target inputs of the round, n0 rows of round input then dk rows per draft block; next_* (k rows), dnext_* (dk + k
 *   rows, written only when every block was accepted and dl > 0), res_* (k entries; node / seq may be NULL), vis rows of vis_words words.
 *   mailbox_dev [4] int32 {n_matches, status, n_valid, pad}.  sample != 0: temperature, seed, round and the draft's tables dtab_*[i],
 *   i < dl, as atspeed_beam_sample_step writes them.  vtrace_dev (greedy, optional): [dl + 1][3][ATSPEED_MAX_BEAMS] words.
 * Refused before any launch: struct_size other than sizeof(atspeed_walk_args), a NULL required pointer, ld <= 0, vis_words < 1, n0 < nb,
 * gen_len0 < 0, blocks_ready outside [0, dl + 1], a sampled walk without automaton, tables or a positive temperature (ATSPEED_ERR_INVALID);
 * k, dk, nb outside [1, ATSPEED_MAX_BEAMS], dl outside [0, ATSPEED_MAX_GAMMA], gen_len0 + dl > ATSPEED_MAX_NEW_TOKENS (ATSPEED_ERR_CAPACITY). */
typedef struct atspeed_walk_args {
  size_t struct_size;
  const float* blk_score[ATSPEED_MAX_GAMMA + 1];
  const int32_t* blk_node[ATSPEED_MAX_GAMMA + 1];
  const int32_t* blk_flat[ATSPEED_MAX_GAMMA + 1];
  const int32_t* blk_seq[ATSPEED_MAX_GAMMA + 1];
  int32_t nb, dl, k, dk, gen_len0;
  int32_t ld;
  const float* logits;
  const float* lse;
  int32_t blk_row0[ATSPEED_MAX_GAMMA + 1];
  int32_t blocks_ready;
  const atspeed_fsm* fsm;
  const atspeed_node_masks* masks;
  int32_t user;
  int32_t vocab, n_row_cand, n0;
  const int32_t* row_cand;
  const int32_t* cur_ids; const int32_t* cur_pos; const int32_t* cur_slot; const uint64_t* cur_vis;
  int32_t* next_ids; int32_t* next_pos; int32_t* next_slot; uint64_t* next_vis;
  int32_t* dnext_ids; int32_t* dnext_pos; int32_t* dnext_slot; uint64_t* dnext_vis;
  float* res_score; int32_t* res_node; int32_t* res_seq; int32_t* res_parent; int32_t* res_tok; int32_t* res_flat;
  int32_t* mailbox;
  int32_t vis_words;
  int32_t sample;
  float temperature;
  uint32_t seed;
  int32_t round;
  int32_t pad;
  const float* dtab_score[ATSPEED_MAX_GAMMA];
  const int32_t* dtab_off[ATSPEED_MAX_GAMMA];
  const float* dtab_lse[ATSPEED_MAX_GAMMA];
  const float* cutoff;
  int32_t* vtrace;
} atspeed_walk_args;
int atspeed_verify_walk(const atspeed_walk_args* args, void* stream);

int atspeed_target_generate(atspeed_decoder* d, const int32_t* prompt_ids_dev, int32_t prompt_len,
                            const atspeed_fsm* fsm, int32_t start_node, int32_t max_new_tokens, int32_t k,
                            int32_t* out_tokens_dev, float* out_scores_dev, atspeed_gen_stats* stats_host,
                            void* stream);

/* target_generate for n users in lock step (one forward + one beam-step launch per generated position for all of
 * them): the constrained beam search of generate_teacher_data.py:211-244 at scale.  Results equal n single calls. */
int atspeed_target_generate_batch(atspeed_decoder** decoders, int32_t n, const int32_t* const* prompt_ids_dev,
                                  const int32_t* prompt_lens, const atspeed_fsm* fsm, const int32_t* start_nodes,
                                  int32_t max_new_tokens, int32_t k, int32_t* const* out_tokens_dev,
                                  float* const* out_scores_dev, atspeed_gen_stats* stats_host /* [n] */, void* stream);

/* Result tensors of a whole batch in one launch (the reference builds `beam_sequence` per beam per step with torch.cat,
 * beamSD.py:87,383): user u's [k][P_u + new_tokens] int64 rows = its prompt followed by the generated suffix of beam j, written at
 * out_dev + k * (prompt_off[u] + u * new_tokens).  prompts_flat_dev: the prompts one after the other (int32); prompt_off_host[n + 1]:
 * their offsets (HOST array); toks_dev [n][k][new_tokens] int32 (the out_tokens of atspeed_bssd_generate_batch laid out contiguously). */
int atspeed_assemble_sequences(const int32_t* prompts_flat_dev, const int64_t* prompt_off_host, const int32_t* toks_dev, int32_t n, int32_t k,
                               int32_t new_tokens, int64_t* out_dev, void* stream);

/* per-round trace of the last atspeed_bssd_generate call (host memory, for parity tests):
 * for round r, step i: the draft's flat ids (dk entries, -1 = not a beam).  Returns the
 * number of ints written. */
int atspeed_decoder_trace(atspeed_decoder* d, int32_t* rounds_out, int32_t cap);

/* Decision trace (parity tests at batch sizes the per-round trace above skips; greedy mode; no reference counterpart -- the reference
 * keeps these as Python locals of verify(), beamSD.py:277-380).  level 1: after every round of the bssd calls made with this decoder
 * the beam blocks and the verify walk's picks are copied to the host (about 60 KB per user and round); level 0 (default): off.
 * atspeed_decoder_decisions returns the number of int32 words of the last call's trace and copies up to cap_words of them.  One
 * record per round: header {kind (0 verify round, 1 final single step), nb, dl, n_matches, tokens generated before the round, k, dk,
 * n_blocks}; n_blocks beam-set images of 5 * 64 + 64 * 16 words each {score bits[64], node[64], parent[64], tok[64], flat[64],
 * seq[64][16]} -- kind 0: the round's beams, draft blocks 1..dl, the new round beams; kind 1: the step's parents, its result --; for
 * kind 0 then (ATSPEED_MAX_GAMMA + 1) * 3 * 64 words: the target's picks of verify step i as {score bits[64], parent[64] (index into
 * block i), token[64] (-1 = no pick)}, valid for steps 0..n_matches. */
int atspeed_decoder_set_trace(atspeed_decoder* d, int32_t level);
int64_t atspeed_decoder_decisions(atspeed_decoder* d, int32_t* out, int64_t cap_words);
/* The decoder's private K / V arenas of its target (draft = 0) or draft model (test hook).  Each arena is [n_layers][max_slots][hidden] elements
 * of the model's type, row s of a layer = KV slot s; atspeed_decoder_kv_bytes is one arena's size (-1: no such model).  atspeed_decoder_kv_copy
 * copies both arenas from (to_cache = 1) or to (0) the caller's device buffers of that size, stream ordered: a test fills them with a sentinel
 * and reads back which slots a call wrote (a round verified in stages leaves the slots of blocks it never forwarded untouched). */
int64_t atspeed_decoder_kv_bytes(const atspeed_decoder* d, int32_t draft);
int atspeed_decoder_kv_copy(atspeed_decoder* d, int32_t draft, int32_t to_cache, void* k_dev, void* v_dev, void* stream);

/* ------------------------------------------------------------------ prompt prefixes: K / V of a shared prompt opening kept resident
 * Prompts built from one template open with the same tokens.  An atspeed_prefix holds the K and V rows those tokens produce in ONE model, in
 * every layer, as a compact store [layers][len][hidden] each in the model's type, plus the token ids.  A user that names a prefix gets the rows
 * copied into slots [0, len) of its private arenas by one scatter launch (all users of a batch call / all users a session round admits that
 * name the same prefix share the launch) and prefills only prompt tokens len .. P - 1: its first round is (base = len, n0 = P - len), which is
 * what every later round looks like.  The attention kernels and every forward are untouched.  No reference counterpart: the reference
 * prefills every prompt whole (beamSD.py:52,221).
 *
 * atspeed_prefix_create: runs m's own forward over the len tokens of ids_dev (one causal segment, positions and slots 0 .. len - 1, in the
 *   mode the model is in: 16-bit / fp32 / W8A8 / W4A8, under its model-wide adapter or the resident slot adapter_slot, 0 = none) into a
 *   scratch arena, gathers rows [0, len) of every layer into the store and keeps the ids.  Every allocation is made here (the scratch is freed
 *   again); the call synchronises `stream`.  1 <= len < max_slots, else ATSPEED_ERR_INVALID.  The model must outlive the prefix.
 * Staleness: the prefix remembers the arithmetic that produced it -- W8A8 on / off, W4A8 on / off, the model-wide adapter's generation, and
 *   its slot with that slot's generation.  A later atspeed_llama_enable_fp8 / _enable_fp4 / _set_lora / _clear_lora that changes the model, or
 *   an atspeed_llama_remove_lora / _add_lora of THAT slot, makes it stale (atspeed_prefix_info returns 1); other slots coming and going do not.
 * Refused with ATSPEED_ERR_INVALID before anything is launched: a stale prefix, a prefix of another model, a target prefix whose slot differs
 *   from the user's adapter, len > P - 1 (one suffix row is needed for the first logit row), target and draft prefixes of different length,
 *   and -- for the beam-SD calls and sessions, whose two models share one token buffer -- a target prefix without a draft prefix or the reverse.
 *   atspeed_target_generate(_batch) look at the target prefix alone.
 * A prompt that does not open with the prefix's ids is found on the device by the prompt-init launch (no extra synchronisation): at the first
 *   read-back that user ends with ATSPEED_ERR_INVALID -- in the batch calls and sessions alone, with stats.status set and a blanked result
 *   block (scores -inf, tokens 0) as an ATSPEED_ERR_FILTERED user does, while the others go on; the one-user calls return the error.
 * atspeed_prefix_info: *len, *users_served (users whose arenas received the rows so far), *bytes (device bytes the object owns); each may be
 *   NULL.  Returns 1 for a stale prefix, 0 for a usable one, negative on error.
 * atspeed_prefix_read: the store and the ids to the caller's device buffers ([layers][len][hidden] elements each, [len] int32), stream
 *   ordered (tests); any of the three may be NULL.
 * atspeed_decoder_set_prefix: the prefixes the generate calls made with this decoder use, like atspeed_decoder_set_adapter; either may be NULL,
 *   both NULL clears.  A prefix must belong to the decoder's model of that role and stay alive while set (and, in a session, until the user's
 *   ticket has come back). */
int atspeed_prefix_create(atspeed_llama* m, const int32_t* ids_dev, int32_t len, int32_t adapter_slot, void* stream, atspeed_prefix** out);
void atspeed_prefix_destroy(atspeed_prefix* p);
int atspeed_prefix_info(const atspeed_prefix* p, int32_t* len, int64_t* users_served, int64_t* bytes);
int atspeed_prefix_read(const atspeed_prefix* p, void* k_dst_dev, void* v_dst_dev, int32_t* ids_dst_dev, void* stream);
int atspeed_decoder_set_prefix(atspeed_decoder* d, const atspeed_prefix* target_prefix, const atspeed_prefix* draft_prefix);
/* The rows into arenas [first, first + n) of the pool atspeed_llama_forward_batch(_adapters) gives the sequences of the prefix's model (grown
 * on demand, as that call grows it), one launch: a following forward whose sequences carry positions and slots from len on, and see slots
 * [0, len + row], continues the prefix.  A stale prefix is refused; first + n <= 256.  Counts n users served. */
int atspeed_prefix_to_batch_arenas(const atspeed_prefix* p, int32_t first, int32_t n, void* stream);
/* The copy kernel alone.  store_k / store_v: [layers][len][row_bytes] device bytes, 16-byte aligned, row_bytes % 16 == 0; arenas: HOST arrays
 * of n (1 .. 256) 16-byte aligned device pointers to [layers][max_slots][row_bytes] each.  atspeed_kv_rows_scatter writes rows [0, len) of every
 * layer of every arena (each 16-byte piece of the store is loaded once and stored n times) and nothing else; atspeed_kv_rows_gather fills the
 * store from ONE arena pair.  1 <= len <= max_slots.  tests/test_prefix_gpu.py::test_copy_kernel_guard_bands */
int atspeed_kv_rows_scatter(const void* store_k_dev, const void* store_v_dev, void* const* k_arenas_dev, void* const* v_arenas_dev, int32_t n,
                            int32_t len, int32_t layers, int32_t row_bytes, int32_t max_slots, void* stream);
int atspeed_kv_rows_gather(void* store_k_dev, void* store_v_dev, const void* k_arena_dev, const void* v_arena_dev, int32_t len, int32_t layers,
                           int32_t row_bytes, int32_t max_slots, void* stream);

/* ------------------------------------------------------------------ scoring candidates: exact target log-probs of item lists
 * "What does the target give each of these N items?" -- the second stage of retrieve-then-rank, and a label's rank beyond K.  The score of an
 * item is exactly what a constrained beam search reports for it (beamSD.py:58-64: log_softmax over the FULL vocabulary, then the mask, then
 * the beam's running score): the sum over its tokens of logit - LSE(full vocabulary) at the row that predicts the token, added in token
 * order in fp32.  No reference counterpart: the reference scores sequences by repeating the prompt per sequence
 * (generate_teacher_data.py:225-232).
 *
 * Lists use atspeed_node_masks_create's format: user u owns sequences [user_seq_offsets[u], user_seq_offsets[u + 1]), sequence s is
 * seq_tokens[seq_offsets[s] .. seq_offsets[s + 1]), 1 .. ATSPEED_MAX_NEW_TOKENS tokens, lengths may differ.  A user's sequences must be
 * STRICTLY ASCENDING lexicographically (sorted, no duplicates; a proper prefix sorts before its extensions): the builder checks the order.
 *
 * Row layout of a user with a prompt of P tokens (one segment of a batched forward, slots private to the user): rows 0 .. P - 1 are the
 * prompt, causal (pos = slot = row, row r sees slots [0, r]).  Then the tree: with lcp(s) = the tokens s shares with its predecessor and
 * e(s) = min(lcp(s), len(s - 1) - 1) (0 for the first sequence), token d of sequence s gets a row of its own iff e(s) <= d < len(s) - 1 -- an
 * item's last token needs none, nothing is predicted from it, which is also why a sequence that continues its predecessor owns the
 * predecessor's last depth itself.  Rows are numbered P, P + 1, ... in (sequence, depth) order; a tree row has ids = the token, pos = P + d,
 * slot = row and sees slots [0, P), the rows of its prefix and itself.  The row that PREDICTS token d is the prompt's last row for d = 0, else
 * the row of prefix depth d - 1: the sequence's own, or that of the nearest earlier sequence that is new at that depth.  Rows are shared by
 * prefix, never by automaton node.  Each sequence is walked through the automaton from the user's start node; one with a token that has no
 * edge is UNKNOWN: it keeps its rows (the layout is a function of the token lists alone), is flagged and counted per user, and scores -inf.
 *
 * atspeed_score_items: all arrays are HOST pointers except prompt_ids_dev[u] (device, [prompt_len[u]]) and scores_out_dev (device,
 *   [sequences] fp32, in list order).  Stages the lists, runs the builder, ONE segmented forward over all users (user = one segment and one KV
 *   arena of the pool atspeed_llama_forward_batch uses; adapter_slots[u] = the user's resident adapter, NULL = none; the decoder's lm_head
 *   form: normaliser from the epilogue, only the automaton's logit tiles stored) and the path-score kernel.  status_out[u]: ATSPEED_OK;
 *   ATSPEED_ERR_CAPACITY when prompt + tree exceed max_tokens or max_slots, or the rows from the prompt's last on exceed max_logit_rows (found
 *   on the host before anything is launched); ATSPEED_ERR_INVALID for a list that is not strictly ascending or whose row count the builder
 *   and the host disagree on.  A refused user takes no part in the forward and its scores are -inf; the other users are scored.
 *   unknown_out[u] (may be NULL) counts its unknown sequences.  The model keeps one scratch block for the lists and rows, grown on demand as
 *   the arena pool is; the call synchronises `stream` (once after the builder, once at its end).
 * atspeed_score_tree_build: the builder alone on caller-owned DEVICE buffers (prompt_ids, prompt_len, start_nodes, user_seq_offsets and
 *   row_offsets are HOST arrays; prompt_ids[u] is a device pointer).  User u's rows are rows [row_offsets[u], row_offsets[u + 1]) of ids / pos /
 *   slots (int32) and vis_bits ([row][max_slots / 64] uint64); no row at or past a user's range, nor past max_slots, is written.
 *   pred_row_dev [sequences][ATSPEED_MAX_NEW_TOKENS]: the user's row that predicts token d, -1 past the sequence's end; known_dev [sequences]
 *   1 / 0; n_rows_dev / unknown_dev / status_dev [n_users]: prompt + tree rows (whether they fit or not), unknown sequences, and ATSPEED_OK,
 *   ATSPEED_ERR_INVALID (order violated, or offsets outside [0, n_seq_tokens] / a length outside 1 .. ATSPEED_MAX_NEW_TOKENS) or
 *   ATSPEED_ERR_CAPACITY (more rows than the user's range or max_slots hold; the rows that fit are written).
 * atspeed_path_scores: scores_out[s] = sum over d of (logits[r][tok_d] - lse[r]), r = seq_base[s] + pred_row[s][d] (seq_base NULL = 0), on
 *   caller-owned device buffers; logits rows are ld floats apart.  -inf for a sequence whose known flag is 0, or that names a row outside
 *   [0, n_rows) or a token outside [0, vocab). */
int atspeed_score_items(atspeed_llama* model, const atspeed_fsm* fsm, int32_t n_users, const int32_t* const* prompt_ids_dev,
                        const int32_t* prompt_len, const int32_t* start_nodes, const int32_t* seq_tokens, const int32_t* seq_offsets,
                        const int32_t* user_seq_offsets, const int32_t* adapter_slots /* may be NULL */, float* scores_out_dev,
                        int32_t* unknown_out /* [n_users], may be NULL */, int32_t* status_out /* [n_users] */, void* stream);
int atspeed_score_tree_build(const atspeed_fsm* fsm, int32_t n_users, const int32_t* const* prompt_ids_dev, const int32_t* prompt_len,
                             const int32_t* start_nodes, const int32_t* seq_tokens_dev, int32_t n_seq_tokens, const int32_t* seq_offsets_dev,
                             const int32_t* user_seq_offsets, int32_t max_slots, const int32_t* row_offsets, int32_t* ids_dev, int32_t* pos_dev,
                             int32_t* slots_dev, uint64_t* vis_bits_dev, int32_t* pred_row_dev, int32_t* known_dev, int32_t* n_rows_dev,
                             int32_t* unknown_dev, int32_t* status_dev, void* stream);
int atspeed_path_scores(const float* logits_dev, int32_t ld, const float* lse_dev, int32_t n_rows, int32_t vocab, const int32_t* seq_tokens_dev,
                        const int32_t* seq_offsets_dev, const int32_t* pred_row_dev, const int32_t* seq_base_dev /* may be NULL */,
                        const int32_t* known_dev, int32_t n_seqs, float* scores_out_dev, void* stream);

/* ------------------------------------------------------------------ low-level ops (tests, benches)
 * C[M,N] = A[M,K] * W[N,K]^T on MFMA; epilogue: 0 store (dtype), 1 fp32 store, 2 residual add into
 * C (dtype), 3 SwiGLU over interleaved gate/up column groups (C is [M, N/2]).
 * Memory contract (tests/test_guard_bands_gpu.py::test_gemm_guard_bands, every kernel form x epilogue x type; ::test_workspace_ladder):
 *   - a_dev and w_dev are 16-byte aligned (no more is needed); K and lda are multiples of 8 elements (fp32: 4); lda >= K; w has row
 *     stride K; ldc >= the output's columns (tested: multiples of 8, fp32 outputs of 4, and the dense ldc = N of any parity).
 *   - no byte outside [M][0 .. N) (SwiGLU: [M][0 .. N/2)) of C is written -- not the columns up to ldc, not a row past M -- and none from
 *     workspace_bytes on; the workspace need not be 16-byte aligned.
 *   - no element outside a[M][0 .. K) and w[N][0 .. K) influences a result, whatever its bits (NaN included): not a row past M or N,
 *     not what lies between column K and lda of a row.  No slack is required after an operand -- every kernel clamps the rows it
 *     fetches to M - 1 and N - 1 -- and the reference call of each case runs on exactly-sized buffers.
 *   - a form that leaves split-K slabs in the workspace runs only where parts x M x N x 4 bytes fit workspace_bytes; with less (or no)
 *     workspace another form computes the same product. */
int atspeed_gemm(const void* a_dev, const void* w_dev, void* c_dev, int32_t m, int32_t n, int32_t k,
                 int32_t lda, int32_t ldc, int32_t dtype, int32_t epilogue, void* workspace_dev,
                 size_t workspace_bytes, void* stream);
/* Which kernel family the library's GEMM launches took since the last reset (dispatch is a fitted cost model: tests assert the path they
 * mean to exercise).  out[i], i < n: 0 ring kernel, 1 ring kernel with its split-K tail, 2 weight-streaming kernel, 3 the same split in K,
 * 4 ring kernel in split-K mode, 5 LDS-tiled kernel, 6 fp8 ring kernel, 7 / 8 fp8 weight-streaming kernel / split, 9 / 10 panel kernel /
 * split, 11 fp8 ring kernel cut in K, 12 W4A8 kernel (any form); 13 / 14 count launches of the 32-rows-per-wave attention kernel, by its
 * single-buffered 64-row tile / its double-buffered 128- and 256-row tiles.  Returns the number of counters the library keeps. */
int atspeed_gemm_path_counters(int64_t* out, int32_t n, int32_t reset);
/* Process-wide tuning / test switches.  Each is an int read ONCE from its environment variable when the library first needs one (the
 * variable is the way to set it for a whole run) and changeable afterwards only through this call (tests and sweeps that compare two
 * settings in one process) -- the dispatch path never calls getenv.  Names: "gemm_sk" (ATSPEED_GEMM_SK, 1), "gemm_sk_g" (no variable; test
 * hook, 0), "gemm_panel" (ATSPEED_GEMM_PANEL, 1), "gemm_force_mt" (ATSPEED_GEMM_FORCE_MT, 0), "graphs" (ATSPEED_GRAPHS, 0),
 * "fuse_qkv_rope" (ATSPEED_FUSE_QKV_ROPE, 1), "fuse_qkv_reduce" (ATSPEED_FUSE_QKV_REDUCE, 1), "gemm_kcut" (ATSPEED_GEMM_KCUT, 2),
 * "verify_staged" (ATSPEED_VERIFY_STAGED, 1), "verify_staged_tokens" (ATSPEED_VERIFY_STAGED_TOKENS, the measured threshold T*),
 * "verify_staged_pass_tokens" (ATSPEED_VERIFY_STAGED_PASS_TOKENS, the measured cost of a phase in tokens),
 * "tail_rows_tokens" (ATSPEED_TAIL_ROWS_TOKENS, 512: a forward of more tokens, at most half of whose rows get logits, runs the last layer's
 * o_proj / gate_up / down over its logit rows only -- 0 every such forward, a huge value none; 16-bit and fp32 models without W8A8 / W4A8
 * copies and without adapter), "attn_short" (ATSPEED_ATTN_SHORT, 1: a lock-step batch whose segments all have at most 64 rows attends in
 * 64-row query tiles, 0 in 128-row tiles; bit-identical); meanings in INTEGRATION.md.  Unknown name: ATSPEED_ERR_INVALID. */
int atspeed_set_switch(const char* name, int32_t value);
int atspeed_get_switch(const char* name, int32_t* value_out);
/* atspeed_gemm / atspeed_gemm_fp8 on operands in the packed layout (a / xq and w / wq through atspeed_pack_rows; K % 32 == 0, for fp8 K % 64 == 0):
 * what the bf16 / fp8 engine runs.  The SwiGLU epilogue's output (ldc % 32 == 0) is packed as well -- it is the down projection's operand --,
 * every other output is row-major.  Same arithmetic as the row-major calls: results are bit-identical.
 * Packed buffers hold an even number of rows: the pad row of an odd m (or n) may hold anything (NaN included) and reaches no output row
 * < m; of a packed SwiGLU output neither the pad row nor, with ldc > N / 2 (a multiple of 32), the columns N / 2 .. ldc - 1 are written
 * (::test_gemm_packed_pad_rows, ::test_gemm_fp8_packed_pad_rows). */
int atspeed_gemm_packed(const void* a_dev, const void* w_dev, void* c_dev, int32_t m, int32_t n, int32_t k, int32_t ldc, int32_t epilogue,
                        void* workspace_dev, size_t workspace_bytes, void* stream);
int atspeed_gemm_fp8_packed(const void* xq_dev, const float* sx_dev, const void* wq_dev, const float* sw_dev, void* c_dev, int32_t m,
                            int32_t n, int32_t k, int32_t ldc, int32_t epilogue, void* workspace_dev, size_t workspace_bytes, void* stream);
/* MXFP4 weight quantiser (format: atspeed_llama_enable_fp4): w [rows][k] 16-bit (dtype ATSPEED_BF16 / ATSPEED_F16; packed = 1: in the packed
 * operand layout, rows even, else row-major) -> q [rows][k / 2] bytes (element j of a row in byte j / 2, low nibble = even j; e2m1 codes: bit 3
 * sign, 0..7 = 0, .5, 1, 1.5, 2, 3, 4, 6) and scales [rows][k / 32] E8M0 bytes; k % 256 == 0, 16-byte aligned buffers. */
int atspeed_quant_weights_mxfp4(const void* w_dev, int32_t rows, int32_t k, int32_t dtype, int32_t packed, void* q_dev, void* scales_dev, void* stream);
/* W4A8 GEMM: C[m][n] = epilogue((sum_k e4m3(xq[m][k]) e2m1(wq[n][k]) 2^(wscale[n][k / 32] - 127)) * sx[m]) in fp32; xq from
 * atspeed_quant_rows_fp8 (packed = 1: atspeed_quant_rows_fp8_packed, and a SwiGLU output comes out packed too), wq / wscale from
 * atspeed_quant_weights_mxfp4; epilogues as atspeed_gemm (0 store, 1 fp32, 2 residual add, 3 SwiGLU) in dtype (ATSPEED_BF16 / ATSPEED_F16);
 * any m >= 1 (tiled over m); k % 256 == 0.  Thin grids are cut in k into fp32 slabs in workspace_dev when it holds them (parts x m x n x 4
 * bytes), else one part per tile.
 * Memory contract (::test_gemm_w4a8_guard_bands, ::test_workspace_ladder[w4a8_split]): xq_dev and wq_dev 16-byte aligned; only
 * [m][0 .. n) of C (SwiGLU: n / 2) and nothing from workspace_bytes on is written; xq rows >= m, sx entries >= m, weight rows >= n and
 * their scale bytes influence no result. */
int atspeed_gemm_w4a8(const void* xq_dev, const float* sx_dev, const void* wq_dev, const void* wscale_dev, void* c_dev, int32_t m, int32_t n,
                      int32_t k, int32_t ldc, int32_t epilogue, int32_t dtype, int32_t packed, void* workspace_dev, size_t workspace_bytes,
                      void* stream);
/* per-row e4m3 quantisation q = e4m3(x / scale[r]), scale[r] = max|x[r]| / 448, and the W8A8 GEMM over such operands */
int atspeed_quant_rows_fp8(const void* x_bf16_dev, int32_t rows, int32_t cols, void* q_dev, float* scale_dev, void* stream);
/* the same on operands in the packed layout (x through atspeed_pack_rows with row_bytes = 2 cols, q comes out as atspeed_pack_rows with
 * row_bytes = cols would lay it out; cols % 64 == 0; both buffers hold an even number of rows): what the engine runs between a bf16
 * producer (attention, SwiGLU) and the fp8 projection that consumes it -- one workgroup per row PAIR, whole 128-byte lines in and out.
 * The pad row of an odd row count is read (any bits) and never written, in q as in scale (::test_quant_rows_fp8_and_packed_guard_bands). */
int atspeed_quant_rows_fp8_packed(const void* x_bf16_packed_dev, int32_t rows, int32_t cols, void* q_packed_dev, float* scale_dev, void* stream);
/* m >= 257: the block-scaled MFMA ring kernel (K % 256 == 0, lock-step batches).  m <= 256 (round 5: one user's forwards, the reference's
 * own regime -- code/inference.py:86-91 loads its target 8-bit for every batch-1 forward): the weight-streaming kernel on e4m3 rows
 * (K % 128 == 0, K >= 512).  There a narrow N is cut in K and finished by a reduce pass over fp32 partial sums in `workspace_dev`
 * (parts x m x n x 4 bytes with parts = min(256 / tiles, K / 512), tiles = N / 64 up to N = 16384, else N / 128 -- up to 256 parts for a very
 * small N; 64 MB always suffices); with too little workspace the launch runs one part per tile; the residual epilogue (2) then takes the ring
 * kernel when K % 256 == 0 and returns ATSPEED_ERR_CAPACITY otherwise.
 * SIGNATURE NOTE: (workspace_dev, workspace_bytes) were inserted before `stream` in round 5; atspeed_version() reports 0.2 since round 6 so
 * that a caller built against the 0.1 header (stream in the workspace position) can tell.
 * Memory contract (::test_gemm_fp8_guard_bands, ::test_workspace_ladder[fp8_*], ::test_gemm_fp8_residual_without_room_for_slabs_is_refused_before_any_launch):
 * xq_dev and wq_dev 16-byte aligned, rows K bytes apart; only [m][0 .. n) of C (SwiGLU: n / 2) and nothing from workspace_bytes on is
 * written, and a refused call has written nothing at all; xq rows >= m, wq rows >= n, sx entries >= m and sw entries >= n influence no
 * result. */
int atspeed_gemm_fp8(const void* xq_dev, const float* sx_dev, const void* wq_dev, const float* sw_dev, void* c_dev, int32_t m,
                     int32_t n, int32_t k, int32_t ldc, int32_t epilogue, void* workspace_dev, size_t workspace_bytes, void* stream);
int atspeed_rmsnorm(const void* x_dev, const void* w_dev, void* y_dev, int32_t rows, int32_t hidden,
                    float eps, int32_t dtype, void* stream);
/* bf16 RMSNorm fused with the per-token e4m3 quantisation of its output (what the fp8 forward runs in front of the qkv and
 * gate_up projections); y_dev may be NULL; q / scale equal atspeed_quant_rows_fp8 of the bf16 norm output bit for bit */
int atspeed_rmsnorm_quant_fp8(const void* x_dev, const void* w_dev, void* y_dev, void* q_dev, float* scale_dev, int32_t rows,
                              int32_t hidden, float eps, void* stream);
/* The adapter's shrink kernel alone: u[row][j] = round(sum_k xn[row][k] a_cat[j][k]), xn = norm_w * round(h * rsqrt(mean(h^2) + eps)) rounded
 * as atspeed_rmsnorm rounds it (the row statistic is the kernel's own fp32 sum), for rows x r3 outputs; r3 = 48, 96, 144 or 192 (3 modules x
 * the rank rounded up to 16).  Memory contract: reads h [rows][hidden], norm_w [hidden], a_cat [r3][hidden] (dense, row-major, dtype);
 * writes exactly u [rows][r3] (dense), nothing else; an all-zero row of a_cat gives exact zeros in its column.  16-bit with hidden % 128 == 0
 * and 16-byte aligned inputs takes the MFMA kernel (16 rows per workgroup; rows past `rows` are neither read nor written), everything else,
 * fp32 included, one workgroup per row.  Two runs give the same bits. */
int atspeed_lora_shrink(const void* h_dev, const void* norm_w_dev, const void* a_cat_dev, void* u_dev, int32_t rows, int32_t hidden, int32_t r3,
                        float eps, int32_t dtype, void* stream);
/* tree attention over a slot-addressed KV cache ([max_slots][hidden] per K and V)
 * Memory contract (tests/test_guard_bands_gpu.py::test_tree_attention_mfma_guard_bands, ::test_tree_attention_scalar_guard_bands): q rows are ldq
 * >= 3 * hidden elements apart (tested: a multiple of 8), 16-byte aligned; out gets [n_tokens][hidden] and nothing else; q rows >=
 * n_tokens, the columns 3 * hidden .. ldq - 1 and cache slots >= n_slots influence no result, whatever their bits.  Slots BELOW n_slots
 * that no row sees must hold FINITE values: with any finite content, the type's largest value included, they change no output bit
 * (::test_tree_attention_invisible_slots_below_n_slots_are_never_seen), but p = 0 times a NaN or Inf V inside an MFMA is NaN -- callers
 * zero-fill a cache before its first use, as the engine does. */
int atspeed_tree_attention(const void* q_dev, int32_t ldq, const void* kcache_dev, const void* vcache_dev,
                           const uint64_t* vis_bits_dev, int32_t vis_words, void* out_dev, int32_t n_tokens,
                           int32_t n_slots, int32_t n_heads, int32_t head_dim, int32_t dtype, void* stream);
/* the same with the tiling chosen by the caller (parity tests reach every kernel form): qtile_rows 0 (auto) / 64 / 128 / 256 query rows
 * per workgroup; rows_per_wave 0 (auto) / 16 (v_mfma 16x16x32, register-staged tiles: small grids) / 32 (v_mfma 32x32x16, LDS-DMA
 * double buffer: the lock-step batches).  bf16 with head_dim 64 / 128 only; other inputs take the scalar kernel whatever is asked. */
int atspeed_tree_attention_tiled(const void* q_dev, int32_t ldq, const void* kcache_dev, const void* vcache_dev,
                                 const uint64_t* vis_bits_dev, int32_t vis_words, void* out_dev, int32_t n_tokens,
                                 int32_t n_slots, int32_t n_heads, int32_t head_dim, int32_t dtype, int32_t qtile_rows,
                                 int32_t rows_per_wave, void* stream);

/* ---- the kernels behind the segment table, one at a time (tests/test_segs_gpu.py pins each to an fp64 reference).  No reference counterpart:
 * the reference runs one user per forward.  The segments are described as atspeed_llama_forward_batch describes them -- n (1 .. 256) and HOST
 * arrays of n per-segment DEVICE pointers (ids, pos, slots: int32 [n_tokens[i]]; vis: uint64 [n_tokens[i]][vis_words]; kcache, vcache: the
 * segment's K / V cache, layer-0 base, [layers][max_slots][hidden]) and HOST arrays of counts -- except that the caches are the caller's.  Each
 * call builds the engine's segment table from them (row0 / logit_row0 = running sums, query tiles) and stages it; a per-segment array a call's
 * kernel does not read may be NULL.  Rows of segment 0, 1, ... follow each other in the batched buffers (total_tok = sum of n_tokens). */
#define ATSPEED_SEGMENTS                                                                                                                   \
  int32_t n, const int32_t* const* ids_dev, const int32_t* const* pos_dev, const int32_t* const* slots_dev, const uint64_t* const* vis_bits_dev, \
      void* const* kcache_dev, void* const* vcache_dev, const int32_t* n_tokens, const int32_t* n_slots_visible, const int32_t* n_logit_rows
/* out[row][0 .. hidden) = table[clamp(id, 0, vocab - 1)][:] for every row (reads ids); rows >= total_tok are not written.  hidden * element
 * size % 16 == 0, 16-byte aligned buffers.  ::test_embed_gather_row_info */
int atspeed_segs_embed(const void* table_dev, int32_t hidden, int32_t vocab, int32_t dtype, void* out_dev, ATSPEED_SEGMENTS, void* stream);
/* out = the LAST n_logit_rows[i] rows of every segment's rows of h [total_tok][hidden], segment after segment (a segment with 0 logit rows
 * contributes none); rows >= sum of n_logit_rows are not written.  Reads no per-segment array.  ::test_embed_gather_row_info */
int atspeed_segs_gather_logit_rows(const void* h_dev, int32_t hidden, int32_t dtype, void* out_dev, ATSPEED_SEGMENTS, void* stream);
/* The two gathers of a row-pruned last layer in one launch: the same rows as atspeed_segs_gather_logit_rows, of h [total_tok][hidden] (row-major)
 * to h_out and of att [total_tok][hidden] to att_out; packed = 1: att and att_out are GEMM operands in the packed layout (atspeed_pack_rows;
 * hidden * element size % 64 == 0, both buffers hold an even number of rows), else row-major.  Rows >= sum of n_logit_rows of either output,
 * the pad row of an odd count included, are not written.  tests/test_tail_rows_gpu.py::test_gather_guard_band */
int atspeed_segs_gather_tail_rows(const void* h_dev, const void* att_dev, int32_t hidden, int32_t dtype, int32_t packed, void* h_out_dev,
                                  void* att_out_dev, ATSPEED_SEGMENTS, void* stream);
/* out[row] = one 24-byte record per row, what the fused qkv epilogues load: { uint64 kc; uint64 vc; int32 pos; int32 slot; } = the row's
 * segment's kcache / vcache pointers, its position clamped to [0, max_pos - 1] (the rotation index) and its cache slot (reads pos, slots).
 * ::test_embed_gather_row_info */
int atspeed_segs_row_info(void* out_dev, int32_t max_pos, ATSPEED_SEGMENTS, void* stream);
/* RoPE + KV scatter as a pass of its own (modeling_llama.py apply_rotary_pos_emb + the cache update): qkv [total_tok][3 * n_heads * head_dim] =
 * q | k | v per row; cos / sin tables fp32 [max_pos][head_dim / 2], row = clamp(pos, 0, max_pos - 1); HF rotate-half pairs (i, i + head_dim / 2):
 * q is rotated in place, rotated k and v go to row `slot` of the segment's caches at layer_off_bytes (reads pos, slots, kcache, vcache); the k
 * and v columns of qkv stay as they were.  16-bit with head_dim % 16 == 0 takes the vector kernel, everything else the scalar one.
 * slabs_dev != NULL (16-bit, head_dim % 16 == 0): the projection as fp32 split-K slabs [splits][total_tok][3 * hidden], summed in ascending
 * slab order in fp32 and rounded to 16 bits first; then only the q columns of qkv are written.  ::test_rope_kv, ::test_rope_kv_slabs */
int atspeed_segs_rope_kv(void* qkv_dev, const float* slabs_dev /* may be NULL */, int32_t splits, const float* cos_dev, const float* sin_dev,
                         size_t layer_off_bytes, int32_t n_heads, int32_t head_dim, int32_t max_pos, int32_t dtype, ATSPEED_SEGMENTS, void* stream);
/* atspeed_segs_rope_kv (slabs == NULL form) with the adapter's expand in front: for every module whose b_*_dev is not NULL, column c of the
 * module becomes y = round(base + round(scaling * round(sum_j u[row][module * r16 + j] * b[c][j]))) before q and k are rotated and k, v are
 * scattered; a module with a NULL b takes atspeed_segs_rope_kv's path bit for bit.  Memory contract: reads u_dev [total_tok][3 * r16] (q, k, v
 * thirds) and b_*_dev [n_heads * head_dim][r16] (dense, pad columns zero; r16 = 16, 32, 48 or 64; 16-byte aligned on the 16-bit vector
 * path); writes what atspeed_segs_rope_kv writes: the q columns of qkv (the k and v columns stay the projection's) and row `slot` of the
 * segment's caches.  16-bit with head_dim % 16 == 0 takes the vector kernel, everything else the scalar one. */
int atspeed_segs_lora_rope_kv(void* qkv_dev, const void* u_dev, const void* b_q_dev, const void* b_k_dev, const void* b_v_dev, int32_t r16,
                              float scaling, const float* cos_dev, const float* sin_dev, size_t layer_off_bytes, int32_t n_heads, int32_t head_dim,
                              int32_t max_pos, int32_t dtype, ATSPEED_SEGMENTS, void* stream);
/* The two adapter kernels with the adapter picked PER SEGMENT (resident adapters, atspeed_llama_add_lora; tests/test_lora_multi_gpu.py):
 * slots_host = HOST array of n_slots (1 .. ATSPEED_LORA_MAX_ADAPTERS + 1) entries, index 0 ignored; seg_adapters = HOST array [n] of indices
 * into it (0 = none).  The calls stage the slot array to the device.  u_dev has a FIXED row stride of 3 * ATSPEED_LORA_MAX_RANK elements,
 * whatever the ranks: row r of a segment with slot a holds that slot's 3 * r16 outputs (q, k, v thirds of r16 each) from element 0 on.
 * atspeed_segs_lora_shrink_multi: atspeed_lora_shrink per row with the row's slot's a_cat and r16.  Writes u_dev [row][0 .. 3 r16) of the rows
 *   whose segment names a slot > 0 and nothing else: rows of slot 0 and the columns from 3 r16 on are not written.  A row's result does not
 *   depend on its place in the batch nor on what the other rows name: it equals atspeed_lora_shrink of that row with that slot bit for bit.
 *   16-bit with hidden % 128 == 0 and 16-byte aligned h, norm_w, u and a_cat takes the MFMA kernel, everything else one workgroup per row.
 * atspeed_segs_lora_rope_kv_multi: atspeed_segs_lora_rope_kv per row with (b_q, b_k, b_v, r16, scaling) of the row's slot; a row of slot 0
 *   and a module whose b is NULL in the row's slot take atspeed_segs_rope_kv's path bit for bit.  u rows of slot 0 are never read.  On the
 *   16-bit vector path (head_dim % 16 == 0) u_dev and every b must be 16-byte aligned. */
int atspeed_segs_lora_shrink_multi(const void* h_dev, const void* norm_w_dev, const atspeed_lora_slot* slots_host, int32_t n_slots, void* u_dev,
                                   int32_t hidden, float eps, int32_t dtype, const int32_t* seg_adapters, ATSPEED_SEGMENTS, void* stream);
int atspeed_segs_lora_rope_kv_multi(void* qkv_dev, const void* u_dev, const atspeed_lora_slot* slots_host, int32_t n_slots, const float* cos_dev,
                                    const float* sin_dev, size_t layer_off_bytes, int32_t n_heads, int32_t head_dim, int32_t max_pos, int32_t dtype,
                                    const int32_t* seg_adapters, ATSPEED_SEGMENTS, void* stream);
/* atspeed_tree_attention_tiled over several segments in one launch: row r of segment i attends to the slots < n_slots_visible[i] of that
 * segment's own caches (at layer_off_bytes) whose bit is set in its visibility words (reads vis, kcache, vcache).  qtile_rows 0 = the engine's
 * choice (128 from 16 segments or when half the segments exceed 96 rows, else 64); rows_per_wave as atspeed_tree_attention_tiled.  packed_out =
 * 1 (16-bit, ldo % 32 == 0): out in the packed operand layout o_proj reads (= atspeed_pack_rows of the row-major result; the pad row of an odd
 * total_tok is not written).  Rows >= total_tok are not written.  ::test_tree_attention_segs, ::test_tree_attention_segs_many32 */
int atspeed_segs_tree_attention(const void* q_dev, int32_t ldq, size_t layer_off_bytes, int32_t vis_words, void* out_dev, int32_t ldo,
                                int32_t n_heads, int32_t head_dim, int32_t dtype, int32_t qtile_rows, int32_t rows_per_wave, int32_t packed_out,
                                ATSPEED_SEGMENTS, void* stream);
/* The residual projections as the forwards run them: h[m][0 .. n) += a w^T exactly as atspeed_gemm(..., epilogue 2) on the same operands and
 * workspace, then xn[m][n] = norm_w * round(h * rsqrt(mean(h^2) + eps)) of the h just stored (HF LlamaRMSNorm on the updated residual stream:
 * the next op's input).  Where the GEMM leaves split-K slabs and n <= 8192 one kernel sums them, adds the residual and normalises; elsewhere the
 * norm kernels follow the GEMM, and those read h densely: ldh > n is accepted only where the fused kernel runs, a call is refused before it
 * writes anything otherwise.  packed = 1 (16-bit; n % 32 == 0): a, w and xn in the packed operand layout (xn has ld = n).
 * atspeed_gemm_fp8_resid_norm / _w4a8_resid_norm: the same behind atspeed_gemm_fp8 / atspeed_gemm_w4a8 (dtype bf16 / fp16; packed: xq and q_out);
 * xn may be NULL when q_out and s_out are given: q_out [m][n] e4m3 and s_out [m] = atspeed_quant_rows_fp8 of xn (the next W8A8 projection's
 * operand; n % 8 == 0, and beyond 8192 columns the e4m3 rows are made from xn, which must then be given; packed: xn needs n % 32 == 0 and q_out
 * n % 64 == 0).  A call these rules refuse is refused before its first launch: h is untouched.  ::test_gemm_resid_norm, ::test_gemm_fp8_resid_norm, ::test_gemm_w4a8_resid_norm */
int atspeed_gemm_resid_norm(const void* a_dev, const void* w_dev, void* h_dev, int32_t m, int32_t n, int32_t k, int32_t lda, int32_t ldh,
                            int32_t dtype, const void* norm_w_dev, void* xn_dev, float eps, void* workspace_dev, size_t workspace_bytes,
                            int32_t packed, void* stream);
int atspeed_gemm_fp8_resid_norm(const void* xq_dev, const float* sx_dev, const void* wq_dev, const float* sw_dev, void* h_dev, int32_t m, int32_t n,
                                int32_t k, int32_t ldh, int32_t dtype, const void* norm_w_dev, void* xn_dev /* may be NULL */,
                                void* q_out_dev /* may be NULL */, float* s_out_dev /* may be NULL */, float eps, void* workspace_dev,
                                size_t workspace_bytes, int32_t packed, void* stream);
int atspeed_gemm_w4a8_resid_norm(const void* xq_dev, const float* sx_dev, const void* wq_dev, const void* wscale_dev, void* h_dev, int32_t m,
                                 int32_t n, int32_t k, int32_t ldh, int32_t dtype, const void* norm_w_dev, void* xn_dev /* may be NULL */,
                                 void* q_out_dev /* may be NULL */, float* s_out_dev /* may be NULL */, float eps, void* workspace_dev,
                                 size_t workspace_bytes, int32_t packed, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ATSPEED_HIP_H */
