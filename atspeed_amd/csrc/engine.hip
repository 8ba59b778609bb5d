// Host-side engine: model handle (weights in HBM, KV arena, forward sequencing) and the
// decoder that runs BSSD / target_generate for one user stream with all state on the device.
// Reference: beamSD.py:458-542 (BSSD), :544-595 (target_generate), :108-179, :190-232, :242-456.
#include <math.h>
#include <stdarg.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <memory>
#include <mutex>
#include <vector>

#include "internal.h"
#include "round_plan.h"
#include "session_queue.h"

// ---------------------------------------------------------------------------- errors / misc
static thread_local std::string g_last_error;

void atspeed_set_error(const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_last_error = buf;
}

extern "C" const char* atspeed_last_error(void) { return g_last_error.c_str(); }
// internal.h: activation buffers, a model's and the device's shared split-K arena, staging ring, stage and profiling events, the graph capture
// stream and every instantiated graph, a decoder's sampling tables (atspeed_session_counters::allocs_after_create)
std::atomic<long long> g_ats_lazy_allocs{0};
// 0.2 (round 6): atspeed_gemm_fp8 / atspeed_gemm_fp8_packed take (workspace, bytes) before the stream (changed in round 5 without a bump);
// atspeed_set_switch / atspeed_get_switch; atspeed_llama_enable_fp8 on fp16 models
extern "C" const char* atspeed_version(void) { return "atspeed_hip 0.2 (gfx950)"; }

// ---- process-wide switches (internal.h: ATS_SW_*)
namespace {
// Staged verification's two measured constants (DESIGN.md "Staged verification"; profiles/staged_verify_ab.txt).  T*: only a greedy lock-step
// round whose packed target forward would hold more tokens than this may verify block by block (below it a forward is bound by the weight
// stream and a speculative row costs nothing).  The pass cost: what one more phase costs, in tokens of a compute-bound forward -- a round is
// staged when the rows it expects to skip (from the target's recent accepted steps) outnumber that per expected extra phase
constexpr int ATS_VERIFY_STAGED_TOKENS = 4096;
constexpr int ATS_VERIFY_STAGED_PASS_TOKENS = 1024;
// Row-pruned tail of the last layer: only a forward of more tokens than this runs the last layer's o_proj / gate_up /
// down over its logit rows alone.  Measured (profiles/tail_rows_ab.txt section 1: one prefill forward of Llama-7B bf16, one logit row per
// user, full and pruned form alternating in one process, median ms of 5-9 calls, spread = max - min of the full runs):
//   tokens   100    188    336    454    696    902    1732   3392   6454   13784   26566
//   full     4.797  5.959  7.788  8.435  12.322 13.332 21.105 36.228 65.847 135.824 255.000
//   pruned   4.797  5.905  7.717  8.363  12.110 13.100 20.711 35.387 64.587 133.040 249.646
//   spread   0.103  0.231  0.061  0.057  0.140  0.329  0.061  0.578  0.790  0.331   1.014
// Up to 256 tokens every projection streams its weights whatever M is and nothing is gained (0.00-0.05 ms, inside the spread); from the first
// size the ring kernels take (257 tokens) the pruned form is never slower than the full runs' spread and wins 0.9 % at 336 tokens, 1.7-2.3 %
// from 696 on.  The staged rule's 4096 was the candidate; the table puts the boundary at the kernel families' own, 256.  The default is 512:
// ONE user's forwards (at most 512 tokens: the one-user models' max_tokens and the graph replay's bound) stay launch for launch what they
// were, which costs the 257-512 band its 0.07 ms; 696 tokens, the first measured size above, wins beyond the spread.
constexpr int ATS_TAIL_ROWS_TOKENS = 512;
struct SwDef { const char* name; const char* env; int dflt; };
const SwDef kSwitches[ATS_N_SW] = {{"gemm_sk", "ATSPEED_GEMM_SK", 1},           {"gemm_sk_g", nullptr, 0},
                                   {"gemm_panel", "ATSPEED_GEMM_PANEL", 1},     {"gemm_force_mt", "ATSPEED_GEMM_FORCE_MT", 0},
                                   {"graphs", "ATSPEED_GRAPHS", 0},             {"fuse_qkv_rope", "ATSPEED_FUSE_QKV_ROPE", 1},
                                   {"gemm_kcut", "ATSPEED_GEMM_KCUT", 2},       {"fuse_qkv_reduce", "ATSPEED_FUSE_QKV_REDUCE", 1},
                                   {"verify_staged", "ATSPEED_VERIFY_STAGED", 1},
                                   {"verify_staged_tokens", "ATSPEED_VERIFY_STAGED_TOKENS", ATS_VERIFY_STAGED_TOKENS},
                                   {"verify_staged_pass_tokens", "ATSPEED_VERIFY_STAGED_PASS_TOKENS", ATS_VERIFY_STAGED_PASS_TOKENS},
                                   {"tail_rows_tokens", "ATSPEED_TAIL_ROWS_TOKENS", ATS_TAIL_ROWS_TOKENS},
                                   {"attn_short", "ATSPEED_ATTN_SHORT", 1}};
std::atomic<int> g_switch[ATS_N_SW];
std::once_flag g_switch_once;
void switches_init() {
  std::call_once(g_switch_once, [] {
    for (int i = 0; i < ATS_N_SW; ++i) {
      const char* v = kSwitches[i].env ? getenv(kSwitches[i].env) : nullptr;
      g_switch[i].store(v ? atoi(v) : kSwitches[i].dflt, std::memory_order_relaxed);
    }
  });
}
}  // namespace
int ats_switch(int id) { switches_init(); return g_switch[id].load(std::memory_order_relaxed); }
extern "C" int atspeed_set_switch(const char* name, int32_t value) {
  ATS_REQUIRE(name, ATSPEED_ERR_INVALID, "set_switch: null name");
  switches_init();
  for (int i = 0; i < ATS_N_SW; ++i)
    if (!strcmp(name, kSwitches[i].name)) { g_switch[i].store(value, std::memory_order_relaxed); return ATSPEED_OK; }
  atspeed_set_error("set_switch: unknown switch '%s'", name);
  return ATSPEED_ERR_INVALID;
}
extern "C" int atspeed_get_switch(const char* name, int32_t* value_out) {
  ATS_REQUIRE(name && value_out, ATSPEED_ERR_INVALID, "get_switch: null argument");
  switches_init();
  for (int i = 0; i < ATS_N_SW; ++i)
    if (!strcmp(name, kSwitches[i].name)) { *value_out = g_switch[i].load(std::memory_order_relaxed); return ATSPEED_OK; }
  atspeed_set_error("get_switch: unknown switch '%s'", name);
  return ATSPEED_ERR_INVALID;
}
std::atomic<long long> g_ats_path_cnt[ATS_N_PATHS];
extern "C" int atspeed_gemm_path_counters(int64_t* out, int32_t n, int32_t reset) {
  for (int i = 0; i < ATS_N_PATHS; ++i) {
    const long long v = reset ? g_ats_path_cnt[i].exchange(0) : g_ats_path_cnt[i].load();
    if (out && i < n) out[i] = v;
  }
  return ATS_N_PATHS;
}
extern "C" int atspeed_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

// ---------------------------------------------------------------------------- host->device staging ring
// Small host-built tables (segment tables, per-user argument blocks) travel through one pinned buffer and one
// device buffer; a slot is reused only after ats_stage_reset() (called after a stream synchronisation) or, if the
// ring fills up, after an explicit synchronisation of the stream.
namespace {
struct StageRing {
  char *host = nullptr, *dev = nullptr;
  size_t cap = 0, used = 0;
};
thread_local StageRing g_stage_dev[ATS_MAX_DEVICES];      // one ring per device (ats_cur_device)
constexpr size_t kStageBytes = 8u << 20;
}  // namespace

// the current device's ring with `bytes` of host_obj copied to the pinned side; *off_out is the slot's offset on both sides
static int stage_slot(const void* host_obj, size_t bytes, hipStream_t st, StageRing** ring_out, size_t* off_out) {
  const int dev = ats_cur_device();
  ATS_REQUIRE(dev >= 0, ATSPEED_ERR_NO_DEVICE, "staging: no current HIP device, or its id is >= %d", ATS_MAX_DEVICES);
  StageRing& r = g_stage_dev[dev];
  if (!r.dev) {                                          // (a pinned side whose device side did not fit is kept for the next try)
    g_ats_lazy_allocs++;
    if (!r.host) ATS_HIP(hipHostMalloc((void**)&r.host, kStageBytes));
    ATS_HIP(hipMalloc((void**)&r.dev, kStageBytes));
    r.cap = kStageBytes; r.used = 0;
  }
  size_t need = (bytes + 255) / 256 * 256;
  ATS_REQUIRE(need <= r.cap, ATSPEED_ERR_CAPACITY, "staging: object of %zu bytes too large", bytes);
  if (r.used + need > r.cap) { ATS_HIP(hipStreamSynchronize(st)); r.used = 0; }
  memcpy(r.host + r.used, host_obj, bytes);
  *ring_out = &r; *off_out = r.used;
  r.used += need;
  return ATSPEED_OK;
}
int ats_stage(const void* host_obj, size_t bytes, const void** dev_out, hipStream_t st) {
  StageRing* r = nullptr; size_t off = 0;
  ATS_TRY(stage_slot(host_obj, bytes, st, &r, &off));
  ATS_HIP(hipMemcpyAsync(r->dev + off, r->host + off, bytes, hipMemcpyHostToDevice, st));
  *dev_out = r->dev + off;
  return ATSPEED_OK;
}
// the same through the pinned ring, but to a device address of the caller's choice
int ats_stage_to(const void* host_obj, size_t bytes, void* dev_dst, hipStream_t st) {
  StageRing* r = nullptr; size_t off = 0;
  ATS_TRY(stage_slot(host_obj, bytes, st, &r, &off));
  ATS_HIP(hipMemcpyAsync(dev_dst, r->host + off, bytes, hipMemcpyHostToDevice, st));
  return ATSPEED_OK;
}
void ats_stage_reset() { const int dev = ats_cur_device(); if (dev >= 0) g_stage_dev[dev].used = 0; }

// ---------------------------------------------------------------------------- FSM
// A create function owns its half-built object through one of these: any early return (ATS_HIP / ATS_TRY / ATS_REQUIRE) then runs
// the handle's own destroy function, which takes a partly filled object (handles are value-initialised, hipFree(nullptr) does nothing).
template <typename T>
using Building = std::unique_ptr<T, void (*)(T*)>;

extern "C" int atspeed_fsm_create(const int32_t* row_ptr, const int32_t* tok, const int32_t* nxt, int32_t n_nodes,
                                  int32_t n_edges, int32_t vocab_size, atspeed_fsm** out) {
  ATS_REQUIRE(row_ptr && out && n_nodes >= 1 && n_edges >= 0 && vocab_size > 0, ATSPEED_ERR_INVALID, "fsm_create: bad arguments");
  ATS_REQUIRE(row_ptr[0] == 0 && row_ptr[n_nodes] == n_edges, ATSPEED_ERR_INVALID, "fsm_create: row_ptr must span [0, n_edges]");
  for (int n = 0; n < n_nodes; ++n) {
    ATS_REQUIRE(row_ptr[n + 1] >= row_ptr[n], ATSPEED_ERR_INVALID, "fsm_create: row_ptr not monotone at node %d", n);
    for (int e = row_ptr[n]; e < row_ptr[n + 1]; ++e) {
      ATS_REQUIRE(tok[e] >= 0 && tok[e] < vocab_size, ATSPEED_ERR_INVALID, "fsm_create: token %d out of vocab at edge %d", tok[e], e);
      ATS_REQUIRE(nxt[e] >= 0 && nxt[e] < n_nodes, ATSPEED_ERR_INVALID, "fsm_create: next node %d out of range at edge %d", nxt[e], e);
      ATS_REQUIRE(e == row_ptr[n] || tok[e] > tok[e - 1], ATSPEED_ERR_INVALID, "fsm_create: children of node %d not strictly ascending", n);
    }
  }
  ATS_REQUIRE((int64_t)ATSPEED_MAX_BEAMS * vocab_size < (int64_t)0x7fffffff, ATSPEED_ERR_CAPACITY, "fsm_create: vocab too large for 32-bit flat ids");
  Building<atspeed_fsm> f(new atspeed_fsm(), atspeed_fsm_destroy);
  size_t ne = (size_t)std::max(n_edges, 1);
  ATS_HIP(hipMalloc(&f->d_row_ptr, (size_t)(n_nodes + 1) * sizeof(int32_t)));
  ATS_HIP(hipMalloc(&f->d_tok, ne * sizeof(int32_t)));
  ATS_HIP(hipMalloc(&f->d_nxt, ne * sizeof(int32_t)));
  ATS_HIP(hipMemcpy(f->d_row_ptr, row_ptr, (size_t)(n_nodes + 1) * sizeof(int32_t), hipMemcpyHostToDevice));
  if (n_edges > 0) {
    ATS_HIP(hipMemcpy(f->d_tok, tok, (size_t)n_edges * sizeof(int32_t), hipMemcpyHostToDevice));
    ATS_HIP(hipMemcpy(f->d_nxt, nxt, (size_t)n_edges * sizeof(int32_t), hipMemcpyHostToDevice));
  }
  f->dev = FsmDev{f->d_row_ptr, f->d_tok, f->d_nxt, n_nodes, n_edges, vocab_size, 32000, 2};     // id filter of beamSD.py:80-86
  // which 256-column tiles of a logit row a step can ever read: the fused lm_head epilogue stores only those (gemm.hip EPI_F32_LSE)
  // one byte per 256-column tile of THIS vocabulary (the epilogue indexes it with every tile of the lm_head's grid)
  std::vector<unsigned char> tiles((size_t)(vocab_size + 255) / 256, 0);
  for (int e = 0; e < n_edges; ++e) tiles[tok[e] / 256] = 1;
  ATS_HIP(hipMalloc((void**)&f->d_tile_store, tiles.size()));
  ATS_HIP(hipMemcpy(f->d_tile_store, tiles.data(), tiles.size(), hipMemcpyHostToDevice));
  *out = f.release();
  return ATSPEED_OK;
}

// "no mask": BSSD(..., prefix_allowed_tokens_fn=None) with an empty processor list (beamSD.py:469-478 builds no processor, :60-64 is
// the identity, :80-86 is skipped): every token of the vocabulary is a candidate of every beam
extern "C" int atspeed_fsm_create_free(int32_t vocab_size, atspeed_fsm** out) {
  ATS_REQUIRE(out && vocab_size > 0, ATSPEED_ERR_INVALID, "fsm_create_free: bad arguments");
  ATS_REQUIRE((int64_t)ATSPEED_MAX_BEAMS * vocab_size < (int64_t)0x7fffffff, ATSPEED_ERR_CAPACITY, "fsm_create_free: vocab too large for 32-bit flat ids");
  Building<atspeed_fsm> f(new atspeed_fsm(), atspeed_fsm_destroy);
  f->dev = FsmDev{nullptr, nullptr, nullptr, 0, 0, vocab_size, 0, -1};
  std::vector<unsigned char> tiles((size_t)(vocab_size + 255) / 256, 1);      // every logit tile can be read
  ATS_HIP(hipMalloc((void**)&f->d_tile_store, tiles.size()));
  ATS_HIP(hipMemcpy(f->d_tile_store, tiles.data(), tiles.size(), hipMemcpyHostToDevice));
  *out = f.release();
  return ATSPEED_OK;
}

extern "C" int atspeed_fsm_set_id_filter(atspeed_fsm* f, int32_t min_item_token, int32_t eos_token) {
  ATS_REQUIRE(f, ATSPEED_ERR_INVALID, "fsm_set_id_filter: null automaton");
  ATS_REQUIRE(f->dev.n_nodes > 0, ATSPEED_ERR_INVALID, "fsm_set_id_filter: a mask-free automaton has no id filter (beamSD.py:80 applies it only with a processor)");
  f->dev.filter_min = min_item_token;
  f->dev.filter_eos = eos_token;
  return ATSPEED_OK;
}

extern "C" void atspeed_fsm_destroy(atspeed_fsm* f) {
  if (!f) return;
  hipFree(f->d_row_ptr); hipFree(f->d_tok); hipFree(f->d_nxt); hipFree(f->d_tile_store);
  delete f;
}

extern "C" int atspeed_trie_flatten(const int32_t* seq_tokens, const int32_t* seq_offsets, int32_t n_seqs,
                                    int32_t* row_ptr_out, int32_t* tok_out, int32_t* nxt_out, int32_t* n_nodes_out,
                                    int32_t* n_edges_out) {
  ATS_REQUIRE(seq_offsets && n_nodes_out && n_edges_out && n_seqs >= 0, ATSPEED_ERR_INVALID, "trie_flatten: bad arguments");
  // build with ordered child maps, then renumber breadth-first so a level's nodes are contiguous
  std::vector<std::map<int32_t, int32_t>> kids(1);
  for (int s = 0; s < n_seqs; ++s) {
    int32_t node = 0;
    for (int32_t i = seq_offsets[s]; i < seq_offsets[s + 1]; ++i) {
      int32_t t = seq_tokens[i];
      auto it = kids[node].find(t);
      if (it == kids[node].end()) {
        int32_t nn = (int32_t)kids.size();
        kids[node][t] = nn;
        kids.emplace_back();
        node = nn;
      } else {
        node = it->second;
      }
    }
  }
  std::vector<int32_t> order{0}, newid(kids.size(), -1);
  newid[0] = 0;
  for (size_t i = 0; i < order.size(); ++i)
    for (auto& kv : kids[order[i]]) { newid[kv.second] = (int32_t)order.size(); order.push_back(kv.second); }
  int32_t n_nodes = (int32_t)order.size(), n_edges = n_nodes - 1;
  *n_nodes_out = n_nodes;
  *n_edges_out = n_edges;
  if (!row_ptr_out || !tok_out || !nxt_out) return ATSPEED_OK;
  int32_t e = 0;
  for (int32_t i = 0; i < n_nodes; ++i) {
    row_ptr_out[i] = e;
    for (auto& kv : kids[order[i]]) { tok_out[e] = kv.first; nxt_out[e] = newid[kv.second]; ++e; }
  }
  row_ptr_out[n_nodes] = e;
  return ATSPEED_OK;
}

// ---------------------------------------------------------------------------- model
// Weights / config / RoPE tables are shared and read-only.  What a forward WRITES is split in two:
//   KvCache — per user (decoder): the slot-addressed K/V arena;
//   ActCtx  — per forward batch: activations, logits, split-K slabs, sized for the tokens of ALL users of the batch.
struct KvCache { void* k = nullptr; void* v = nullptr; };

struct ActCtx {
  int cap_tok = 0, cap_rows = 0;
  void *h = nullptr, *xn = nullptr, *qkv = nullptr, *att = nullptr, *act = nullptr, *gath = nullptr;
  void* att_tail = nullptr;                      // [cap_rows][hidden] the logit rows of att, compact: the o_proj operand of a row-pruned last layer
  float* logits = nullptr;                       // [cap_rows][logits_ld]
  float* lse = nullptr;                          // [cap_rows]
  float* lse_part = nullptr; size_t lse_part_bytes = 0;   // [cap_rows][vocab tiles] (max, sum exp) partials of the fused lm_head epilogue
  int32_t* row_cand = nullptr;                   // [cap_rows][ATSPEED_MAX_BEAMS] best tokens per logit row (mask-free search only)
  RowInfo* rowinfo = nullptr;                    // [cap_tok] cache / slot / rotation of each batched row (qkv projection's fused epilogue)
  void* lora_u = nullptr;                        // [cap_tok][3 * 64] lora_A outputs of a model with an adapter (lora_u_ensure: atspeed_llama_set_lora, or with the buffers above)
  void* xq = nullptr; float* sx = nullptr;       // fp8 activations [cap_tok][max(hidden, ffn)] + per-token scales
  void* ws = nullptr; size_t ws_bytes = 0;       // split-K slabs
  SkArena sk;                                    // the ring kernel's split-K tail (16-bit models: internal.h SkArena): allocated in front of the first forward of
  bool sk_tried = false;                         // >= 257 tokens that is not being captured (sk_arena_lazy), never inside the launch sequence
  // forwards of a recurring shape are replayed as hipGraphs (one launch instead of ~9 per layer: a user's later rounds are
  // 20-140 tokens and launch-bound); the segment table lives at a fixed device address so that it is data, not a kernel argument
  SegTable* segtab_dev = nullptr;
  hipStream_t cap_stream = nullptr;
  // tokens, logit rows, segments, query tiles, tile rows, weight scheme (Scheme), last layer's tail row-pruned (forward_prunes_tail)
  typedef std::tuple<int, int, int, int, int, int, int> GraphKey;
  std::map<GraphKey, hipGraphExec_t> graphs;
  std::map<GraphKey, int> graph_seen;
  // optional per-GEMM hipEvent brackets (bench.py roofline): 0 qkv, 1 o_proj, 2 gate_up, 3 down, 4 lm_head
  bool prof_pending = false;
  std::vector<hipEvent_t> prof_ev;               // 2 events per bracket
  std::vector<int> prof_kind, prof_m;            // kind / M per bracket of the pending forward
};

// The arithmetic of a layer projection: the model's 16-bit (fp32) weights, or library-owned quantised copies of them -- W8A8 (e4m3 rows, one
// float scale per output row: atspeed_llama_enable_fp8) or W4A8 (MXFP4: e2m1 nibbles [rows][K / 2] + E8M0 scale bytes [rows][K / 32], gemm.hip
// "W4A8": atspeed_llama_enable_fp4).  A model holds ONE scheme; a forward of a W8A8 model runs 16-bit the projections whose shape the W8A8
// kernels do not take at its token count (engine_forward.inc).
enum Scheme { SCHEME_16 = 0, SCHEME_W8A8 = 1, SCHEME_W4A8 = 2, N_SCHEMES = 3 };
// The four projections of a layer, in the order of the profile brackets and the counters, and their GEMM shapes: out[M][ldc] = epi(x[M][K] W[N][K]^T)
enum Proj { P_QKV = 0, P_O = 1, P_GU = 2, P_DOWN = 3, N_PROJ = 4 };
struct ProjShape { int n, k, ldc, epi; };
static ProjShape proj_shape(const atspeed_llama_config& c, int p) {
  const int H = c.hidden, F = c.ffn;
  switch (p) {
    case P_QKV: return {3 * H, H, 3 * H, EPI_STORE};
    case P_O: return {H, H, H, EPI_RESID};
    case P_GU: return {2 * F, H, F, EPI_SWIGLU};
    default: return {H, F, H, EPI_RESID};
  }
}
static const void* proj_weight(const atspeed_llama_layer_weights& w, int p) { return p == P_QKV ? w.wqkv : p == P_O ? w.wo : p == P_GU ? w.wgu : w.wd; }
// the quantised copies of one layer's projections: weights and scales (float per row or packed bytes by the scheme, cast where each family is called)
namespace { struct QuantLayer { void* w[N_PROJ] = {}; void* s[N_PROJ] = {}; }; }
static void quant_layers_free(std::vector<QuantLayer>& v) {
  for (auto& f : v) for (int p = 0; p < N_PROJ; ++p) { hipFree(f.w[p]); hipFree(f.s[p]); }
  v.clear();
}

struct atspeed_llama {
  atspeed_llama_config cfg;
  const void *embed, *final_norm, *lm_head;
  std::vector<atspeed_llama_layer_weights> layers;
  int esz, head_dim, vis_words, logits_ld;
  int pk;                                        // 1: weights and GEMM-operand activations in the packed operand layout (common.h), bf16 only
  size_t layer_kv_bytes;
  float *cos_tab, *sin_tab;                      // [max_slots][head_dim/2]
  int scheme = SCHEME_16;                        // Scheme; quant holds the copies of every layer unless it is SCHEME_16
  std::vector<QuantLayer> quant;
  bool plain16() const { return scheme == SCHEME_16 && !has_lora(); }   // a 16-bit (fp32) target without adapter: row-pruned tail, staged verification
  // optional LoRA adapter kept beside the base (atspeed_llama_set_lora): library-owned zero-padded copies in ONE device block, per layer the
  // stacked A_cat [3 R16][hidden] (q, k, v; an absent module's rows are zero) and B_m [hidden][R16] (NULL = module not adapted)
  struct LoraLayer { const void* a_cat = nullptr; const void* b[3] = {nullptr, nullptr, nullptr}; };
  std::vector<LoraLayer> lora;                   // empty = no adapter: the forward is then launch for launch what it was without this feature
  void* lora_mem = nullptr;
  int lora_r16 = 0;
  float lora_scaling = 0.f;
  long lora_cnt = 0;                             // shrink + expand launches (atspeed_llama_lora_launches)
  // resident adapters picked per user (atspeed_llama_add_lora), exclusive with the model-wide one above: slot s (1 .. 16) owns one device block
  // laid out as set_lora's; slot_tab is the DEVICE table the segmented kernels read, [n_layers][17] entries (entry 0 = none), at a fixed address
  // from the first add to the model's end and rewritten by add / remove alone
  struct LoraSlot { void* mem = nullptr; int r16 = 0; float scaling = 0.f; };
  LoraSlot slots[ATSPEED_LORA_MAX_ADAPTERS + 1];
  int n_slots = 0;                               // occupied
  atspeed_lora_slot* slot_tab = nullptr;
  // what a prompt prefix (atspeed_prefix) remembers of the adapters that produced it: bumped by set_lora / clear_lora, and per slot by the
  // add_lora / remove_lora of that slot
  long lora_gen = 0, slot_gen[ATSPEED_LORA_MAX_ADAPTERS + 1] = {};
  bool has_lora() const { return !lora.empty() || n_slots > 0; }   // the forward takes the adapter side path (either kind)
  bool slot_ok(int s) const { return s == 0 || (s >= 1 && s <= ATSPEED_LORA_MAX_ADAPTERS && slots[s].mem); }
  KvCache kv0;                                   // cache of the plain atspeed_llama_forward API
  std::vector<KvCache> kv_pool;                  // one more cache per segment of atspeed_llama_forward_batch (grown on demand)
  ActCtx* act;                                   // grown on demand (ensure_act)
  void* score_mem = nullptr; size_t score_bytes = 0;   // atspeed_score_items' lists, tree rows and per-sequence tables: one block, grown on demand like the pool
  bool prof_on = false;
  double prof_ms[5] = {0, 0, 0, 0, 0};
  long prof_cnt[5] = {0, 0, 0, 0, 0};
  long prof_rows[5] = {0, 0, 0, 0, 0};           // sum of M over the bracketed launches
  // the same, restricted to launches of at least ATS_PROF_BIG_ROWS tokens (these take the 256x256 ring kernel)
  double prof_big_ms[5] = {0, 0, 0, 0, 0};
  long prof_big_cnt[5] = {0, 0, 0, 0, 0};
  long prof_big_rows[5] = {0, 0, 0, 0, 0};
  // how often each layer projection ran in each scheme (atspeed_llama_fp8_counters, atspeed_llama_fp4_counters: both report SCHEME_16 as `other`)
  long proj_cnt[N_SCHEMES][N_PROJ] = {};
  long rope_fused_cnt = 0;                       // qkv projections that carried RoPE + the KV scatter in their epilogue (atspeed_llama_rope_fused_launches)
  // staged verification's memory (bssd_round_staged): over the recent greedy verify walks on this target, decayed per round, how often a
  // draft block j was drafted and how often the walk needed its rows (n_matches >= j)
  double stg_drafted[ATSPEED_MAX_GAMMA + 1] = {}, stg_needed[ATSPEED_MAX_GAMMA + 1] = {};
  bool fwd_log_on = false;                       // (tokens, logit rows) of every forward while on (atspeed_llama_forward_log)
  std::vector<int32_t> fwd_log;
};
constexpr int ATS_PROF_BIG_ROWS = 1024;

static void prof_harvest(atspeed_llama* m) {
  ActCtx* cx = m->act;
  if (!cx || !cx->prof_pending) return;
  for (size_t b = 0; b < cx->prof_kind.size(); ++b) {
    float ms = 0.f;
    if (hipEventSynchronize(cx->prof_ev[2 * b + 1]) == hipSuccess &&
        hipEventElapsedTime(&ms, cx->prof_ev[2 * b], cx->prof_ev[2 * b + 1]) == hipSuccess) {
      int kd = cx->prof_kind[b];
      m->prof_ms[kd] += ms; m->prof_cnt[kd] += 1; m->prof_rows[kd] += cx->prof_m[b];
      if (cx->prof_m[b] >= ATS_PROF_BIG_ROWS) { m->prof_big_ms[kd] += ms; m->prof_big_cnt[kd] += 1; m->prof_big_rows[kd] += cx->prof_m[b]; }
    }
  }
  cx->prof_kind.clear(); cx->prof_m.clear();
  cx->prof_pending = false;
}

struct ProfBracket {
  ActCtx* cx; hipStream_t st; bool on; size_t idx;
  ProfBracket(atspeed_llama* m, int kind, int rows, hipStream_t st_) : cx(m->act), st(st_), on(m->prof_on), idx(0) {
    if (!on) return;
    idx = cx->prof_kind.size();
    while (cx->prof_ev.size() < 2 * (idx + 1)) { hipEvent_t e; hipEventCreate(&e); cx->prof_ev.push_back(e); g_ats_lazy_allocs++; }
    cx->prof_kind.push_back(kind); cx->prof_m.push_back(rows);
    hipEventRecord(cx->prof_ev[2 * idx], st);
  }
  ~ProfBracket() { if (on) { hipEventRecord(cx->prof_ev[2 * idx + 1], st); cx->prof_pending = true; } }
};

static size_t gemm_ws_for(const atspeed_llama_config& c, int max_tok, int max_rows) {
  size_t best = 0;
  for (int m = 1; m <= max_tok; ++m) {          // the split-K plan depends on the exact M: take the true maximum
    for (int p = 0; p < N_PROJ; ++p) {
      const ProjShape s = proj_shape(c, p);
      best = std::max(best, ATS_KD(c.dtype, ats_gemm_workspace_bytes(m, s.n, s.k, c.dtype)));
      if (c.dtype == ATSPEED_F32) continue;        // a 16-bit model may get quantised copies later (enable_fp8 / enable_fp4): their split plans too
      // (gate_up's W8A8 slabs have never been counted in: whether they fit decides its plan, so counting them in is a change of its own)
      if (p != P_GU) best = std::max(best, ATS_KD(c.dtype, ats_gemm_fp8_workspace_bytes(m, s.n, s.k)));
      best = std::max(best, ATS_KD(c.dtype, ats_gemm_w4a8_workspace_bytes(m, s.n, s.k)));
    }
    if (m <= max_rows) best = std::max(best, ATS_KD(c.dtype, ats_gemm_workspace_bytes(m, c.vocab_size, c.hidden, c.dtype)));
  }
  return best + (1 << 20);
}

static void act_free(ActCtx* cx) {
  if (!cx) return;
  hipFree(cx->h); hipFree(cx->xn); hipFree(cx->qkv); hipFree(cx->att); hipFree(cx->act); hipFree(cx->gath); hipFree(cx->att_tail);
  hipFree(cx->logits); hipFree(cx->lse); hipFree(cx->lse_part); hipFree(cx->ws); hipFree(cx->xq); hipFree(cx->sx); hipFree(cx->rowinfo); hipFree(cx->lora_u);
  hipFree(cx->row_cand); hipFree(cx->sk.ws); hipFree(cx->sk.cnt);
  for (hipEvent_t e : cx->prof_ev) hipEventDestroy(e);
  for (auto& g : cx->graphs) hipGraphExecDestroy(g.second);
  if (cx->cap_stream) hipStreamDestroy(cx->cap_stream);
  hipFree(cx->segtab_dev);
  delete cx;
}

// lora_A's outputs of every token the context can hold, at the largest rank (3 x 64 per token): an adapter of another rank needs no new buffer
static int lora_u_ensure(atspeed_llama* m, ActCtx* cx) {
  if (cx->lora_u) return ATSPEED_OK;
  ATS_HIP(hipMalloc(&cx->lora_u, (size_t)cx->cap_tok * 3 * ATSPEED_LORA_MAX_RANK * m->esz));
  return ATSPEED_OK;
}

// make sure the model's activation context can hold `tok` tokens and `rows` logit rows (device must be idle on it)
static int ensure_act(atspeed_llama* m, int tok, int rows) {
  if (m->act && m->act->cap_tok >= tok && m->act->cap_rows >= rows) return ATSPEED_OK;
  if (m->act) { prof_harvest(m); ATS_HIP(hipDeviceSynchronize()); act_free(m->act); m->act = nullptr; }
  const atspeed_llama_config& c = m->cfg;
  g_ats_lazy_allocs++;
  Building<ActCtx> cx(new ActCtx(), act_free);
  // 25 % headroom: the next batch's token count differs by a few prompt tokens, and growing costs a device synchronisation plus
  // the re-allocation of every activation buffer (seen as 30-40 ms hiccups inside timed regions)
  // even counts: the packed operand layout stores row pairs, a last row with an even index still owns a full 128-byte line pair
  cx->cap_tok = (std::max((tok + tok / 4 + 255) / 256 * 256, c.max_tokens) + 1) & ~1;
  cx->cap_rows = (std::max((rows + rows / 4 + 63) / 64 * 64, c.max_logit_rows) + 1) & ~1;
  size_t T = cx->cap_tok, H = c.hidden, e = m->esz;
  ATS_HIP(hipMalloc(&cx->h, T * H * e));
  ATS_HIP(hipMalloc(&cx->xn, T * H * e));
  ATS_HIP(hipMalloc(&cx->qkv, T * 3 * H * e));
  ATS_HIP(hipMalloc(&cx->att, T * H * e));
  ATS_HIP(hipMalloc(&cx->act, T * (size_t)c.ffn * e));
  ATS_HIP(hipMalloc(&cx->gath, (size_t)cx->cap_rows * H * e));
  ATS_HIP(hipMalloc(&cx->att_tail, (size_t)cx->cap_rows * H * e));
  ATS_HIP(hipMalloc((void**)&cx->logits, (size_t)cx->cap_rows * m->logits_ld * sizeof(float)));
  ATS_HIP(hipMalloc((void**)&cx->lse, (size_t)cx->cap_rows * sizeof(float)));
  ATS_HIP(hipMalloc((void**)&cx->row_cand, (size_t)cx->cap_rows * ATSPEED_MAX_BEAMS * sizeof(int32_t)));
  cx->lse_part_bytes = ats_bf16::ats_lmhead_lse_part_bytes(cx->cap_rows, c.vocab_size);
  ATS_HIP(hipMalloc((void**)&cx->lse_part, cx->lse_part_bytes));
  ATS_HIP(hipMalloc(&cx->xq, T * (size_t)std::max(c.hidden, c.ffn)));
  ATS_HIP(hipMalloc((void**)&cx->sx, T * sizeof(float)));
  ATS_HIP(hipMalloc((void**)&cx->rowinfo, T * sizeof(RowInfo)));
  cx->ws_bytes = gemm_ws_for(c, cx->cap_tok, cx->cap_rows);
  ATS_HIP(hipMalloc(&cx->ws, cx->ws_bytes));
  ATS_HIP(hipMalloc((void**)&cx->segtab_dev, sizeof(SegTable)));
  if (m->has_lora()) ATS_TRY(lora_u_ensure(m, cx.get()));
  m->act = cx.release();
  return ATSPEED_OK;
}

// The split-K tail's arena (128 MB + counters) belongs to the model, but only a model that really runs forwards of >= 257 tokens gets one
// (every model used to own one from creation -- the 68M draft and every rank's one-user target included, whose forwards never reach
// the ring kernel).  Allocated HERE, in front of the launch sequence of the first such forward, never inside it; a forward whose stream is
// being captured by the caller allocates nothing (its thin grids run the plain kernel, as before).  Optional: without room for it the model
// still runs (thin / partly filled grids then take the device's shared arena or the plain grid).  atspeed_llama_sk_arena_bytes reports it.
static void sk_arena_lazy(atspeed_llama* m, int T, hipStream_t st) {
  ActCtx* cx = m->act;
  const atspeed_llama_config& c = m->cfg;
  if (cx->sk.ws || cx->sk_tried || T < 257 || c.dtype == ATSPEED_F32 || c.hidden % 128 != 0) return;   // shapes the ring kernel can take at all (big_kernel_applies)
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(st, &cs) != hipSuccess) { (void)hipGetLastError(); return; }
  if (cs != hipStreamCaptureStatusNone) return;
  cx->sk_tried = true;
  g_ats_lazy_allocs++;
  if (hipMalloc((void**)&cx->sk.ws, ATS_SK_ARENA_BYTES) != hipSuccess || hipMalloc((void**)&cx->sk.cnt, ATS_SK_ARENA_COUNTERS * sizeof(int)) != hipSuccess ||
      hipMemsetAsync(cx->sk.cnt, 0, ATS_SK_ARENA_COUNTERS * sizeof(int), st) != hipSuccess) {
    (void)hipGetLastError();
    hipFree(cx->sk.ws); hipFree(cx->sk.cnt);
    cx->sk = SkArena{};
  }
}
extern "C" int64_t atspeed_llama_sk_arena_bytes(const atspeed_llama* m) { return m && m->act && m->act->sk.ws ? (int64_t)ATS_SK_ARENA_BYTES : 0; }

static void kv_free(KvCache* kv) { hipFree(kv->k); hipFree(kv->v); kv->k = kv->v = nullptr; }
static int kv_create(atspeed_llama* m, KvCache* kv) {           // both halves or, on failure, neither
  size_t bytes = (size_t)m->cfg.n_layers * m->layer_kv_bytes;
  auto make = [&]() -> int {
    ATS_HIP(hipMalloc(&kv->k, bytes));
    ATS_HIP(hipMalloc(&kv->v, bytes));
    ATS_HIP(hipMemset(kv->k, 0, bytes));
    ATS_HIP(hipMemset(kv->v, 0, bytes));
    return ATSPEED_OK;
  };
  const int rc = make();
  if (rc != ATSPEED_OK) kv_free(kv);
  return rc;
}

extern "C" int atspeed_llama_create(const atspeed_llama_config* cfg, const void* embed, const void* final_norm,
                                    const void* lm_head, const atspeed_llama_layer_weights* layers, atspeed_llama** out) {
  ATS_REQUIRE(cfg && embed && final_norm && lm_head && layers && out, ATSPEED_ERR_INVALID, "llama_create: null argument");
  ATS_REQUIRE(cfg->dtype == ATSPEED_F32 || cfg->dtype == ATSPEED_BF16 || cfg->dtype == ATSPEED_F16, ATSPEED_ERR_INVALID, "llama_create: bad dtype");
  ATS_REQUIRE(cfg->n_heads > 0 && cfg->hidden % cfg->n_heads == 0, ATSPEED_ERR_INVALID, "llama_create: hidden %% n_heads != 0");
  int hd = cfg->hidden / cfg->n_heads;
  ATS_REQUIRE(hd % 8 == 0 && hd <= 256, ATSPEED_ERR_INVALID, "llama_create: head_dim %d unsupported", hd);
  ATS_REQUIRE(cfg->hidden % 8 == 0 && cfg->ffn % 16 == 0, ATSPEED_ERR_INVALID, "llama_create: hidden %% 8 / ffn %% 16 required");
  ATS_REQUIRE(cfg->max_slots > 0 && cfg->max_slots % 64 == 0 && cfg->max_slots <= 2048, ATSPEED_ERR_INVALID,
              "llama_create: max_slots must be a multiple of 64, <= 2048");
  ATS_REQUIRE(cfg->max_tokens > 0 && cfg->max_logit_rows > 0 && cfg->max_logit_rows <= cfg->max_tokens, ATSPEED_ERR_INVALID,
              "llama_create: bad token limits");
  ATS_REQUIRE(cfg->weight_layout == ATSPEED_WEIGHTS_ROW_MAJOR || cfg->weight_layout == ATSPEED_WEIGHTS_PACKED, ATSPEED_ERR_INVALID,
              "llama_create: weight_layout must be ATSPEED_WEIGHTS_ROW_MAJOR (0) or ATSPEED_WEIGHTS_PACKED (1)");
  Building<atspeed_llama> m(new atspeed_llama(), atspeed_llama_destroy);
  m->cfg = *cfg;
  m->embed = embed; m->final_norm = final_norm; m->lm_head = lm_head;
  m->layers.assign(layers, layers + cfg->n_layers);
  m->esz = cfg->dtype == ATSPEED_F32 ? 4 : 2;
  m->head_dim = hd;
  m->vis_words = cfg->max_slots / 64;
  m->logits_ld = (cfg->vocab_size + 63) / 64 * 64;
  m->layer_kv_bytes = (size_t)cfg->max_slots * cfg->hidden * m->esz;
  m->pk = cfg->weight_layout == ATSPEED_WEIGHTS_PACKED ? 1 : 0;
  ATS_REQUIRE(!m->pk || ((cfg->dtype == ATSPEED_BF16 || cfg->dtype == ATSPEED_F16) && cfg->hidden % 32 == 0 && cfg->ffn % 32 == 0), ATSPEED_ERR_INVALID,
              "llama_create: packed weights need bf16 / fp16 and hidden / ffn multiples of 32 (hidden %d, ffn %d)", cfg->hidden, cfg->ffn);
  ATS_TRY(kv_create(m.get(), &m->kv0));
  ATS_TRY(ensure_act(m.get(), cfg->max_tokens, cfg->max_logit_rows));
  // RoPE tables: HF computes inv_freq and the angle in fp32; cos/sin of that angle in double, rounded once
  int half = hd / 2;
  std::vector<float> ct((size_t)cfg->max_slots * half), stv((size_t)cfg->max_slots * half);
  for (int p = 0; p < cfg->max_slots; ++p)
    for (int i = 0; i < half; ++i) {
      float inv = 1.0f / powf(cfg->rope_theta, (float)(2 * i) / (float)hd);
      float ang = (float)p * inv;
      ct[(size_t)p * half + i] = (float)cos((double)ang);
      stv[(size_t)p * half + i] = (float)sin((double)ang);
    }
  ATS_HIP(hipMalloc((void**)&m->cos_tab, ct.size() * sizeof(float)));
  ATS_HIP(hipMalloc((void**)&m->sin_tab, stv.size() * sizeof(float)));
  ATS_HIP(hipMemcpy(m->cos_tab, ct.data(), ct.size() * sizeof(float), hipMemcpyHostToDevice));
  ATS_HIP(hipMemcpy(m->sin_tab, stv.data(), stv.size() * sizeof(float), hipMemcpyHostToDevice));
  *out = m.release();
  return ATSPEED_OK;
}

extern "C" void atspeed_llama_destroy(atspeed_llama* m) {
  if (!m) return;
  kv_free(&m->kv0);
  for (KvCache& kv : m->kv_pool) kv_free(&kv);
  act_free(m->act);
  hipFree(m->score_mem);
  quant_layers_free(m->quant);
  hipFree(m->lora_mem);
  for (auto& sl : m->slots) hipFree(sl.mem);
  hipFree(m->slot_tab);
  hipFree(m->cos_tab); hipFree(m->sin_tab);
  delete m;
}

extern "C" int atspeed_llama_profile(atspeed_llama* m, int32_t enable, double* ms_out, int64_t* count_out, int64_t* rows_out) {
  ATS_REQUIRE(m, ATSPEED_ERR_INVALID, "profile: null model");
  prof_harvest(m);
  for (int i = 0; i < 5; ++i) {
    if (ms_out) ms_out[i] = m->prof_ms[i];
    if (count_out) count_out[i] = m->prof_cnt[i];
    if (rows_out) rows_out[i] = m->prof_rows[i];
  }
  if (enable >= 0) {
    m->prof_on = enable != 0;
    for (int i = 0; i < 5; ++i) {
      m->prof_ms[i] = 0; m->prof_cnt[i] = 0; m->prof_rows[i] = 0;
      m->prof_big_ms[i] = 0; m->prof_big_cnt[i] = 0; m->prof_big_rows[i] = 0;
    }
  }
  return ATSPEED_OK;
}

extern "C" int32_t atspeed_llama_forward_log(atspeed_llama* m, int32_t enable, int32_t* pairs_out, int32_t max_pairs) {
  if (!m) return -1;
  const int32_t n = (int32_t)(m->fwd_log.size() / 2);
  if (pairs_out) for (int32_t i = 0; i < n && i < max_pairs; ++i) { pairs_out[2 * i] = m->fwd_log[2 * i]; pairs_out[2 * i + 1] = m->fwd_log[2 * i + 1]; }
  if (enable >= 0) { m->fwd_log_on = enable != 0; if (enable) m->fwd_log.clear(); }
  return n;
}

extern "C" int atspeed_llama_profile_big(atspeed_llama* m, double* ms_out, int64_t* count_out, int64_t* rows_out) {
  ATS_REQUIRE(m && ms_out && count_out && rows_out, ATSPEED_ERR_INVALID, "profile_big: null argument");
  prof_harvest(m);
  for (int i = 0; i < 5; ++i) { ms_out[i] = m->prof_big_ms[i]; count_out[i] = m->prof_big_cnt[i]; rows_out[i] = m->prof_big_rows[i]; }
  return ATSPEED_OK;
}

extern "C" int atspeed_lmhead_lse(const void* x, const void* w, float* logits, float* lse, int32_t rows, int32_t vocab, int32_t hidden, int32_t ld,
                                  const atspeed_fsm* fsm, void* workspace, size_t workspace_bytes, int32_t* fused_out, void* stream) {
  ATS_REQUIRE(x && w && logits && lse && rows >= 0 && vocab > 0 && hidden > 0 && ld >= vocab, ATSPEED_ERR_INVALID, "lmhead_lse: bad arguments");
  const size_t pb = ats_bf16::ats_lmhead_lse_part_bytes(rows, vocab);
  const bool have = workspace && workspace_bytes >= pb && ((uintptr_t)workspace & 15) == 0;
  char* rest = have ? (char*)workspace + (pb + 255) / 256 * 256 : (char*)workspace;
  const size_t rest_bytes = have ? (workspace_bytes > (pb + 255) / 256 * 256 ? workspace_bytes - (pb + 255) / 256 * 256 : 0) : workspace_bytes;
  int fused = 0;
  const int rc = ats_bf16::ats_lmhead_lse(x, w, logits, rows, vocab, hidden, hidden, ld, ATSPEED_BF16, fsm ? fsm->d_tile_store : nullptr, have ? (float*)workspace : nullptr,
                                have ? pb : 0, lse, rest, rest_bytes, (hipStream_t)stream, &fused);
  if (fused_out) *fused_out = fused;
  return rc;
}

// how often each layer projection ran in the quantised `scheme` and how often as a 16-bit (fp32) GEMM
static int quant_counters(atspeed_llama* m, const char* who, int scheme, int64_t* quant_out, int64_t* other_out, int32_t reset) {
  ATS_REQUIRE(m, ATSPEED_ERR_INVALID, "%s: null model", who);
  for (int i = 0; i < N_PROJ; ++i) {
    if (quant_out) quant_out[i] = m->proj_cnt[scheme][i];
    if (other_out) other_out[i] = m->proj_cnt[SCHEME_16][i];
    if (reset) { m->proj_cnt[scheme][i] = 0; m->proj_cnt[SCHEME_16][i] = 0; }
  }
  return ATSPEED_OK;
}
extern "C" int atspeed_llama_fp8_counters(atspeed_llama* m, int64_t* fp8_out, int64_t* other_out, int32_t reset) {
  return quant_counters(m, "fp8_counters", SCHEME_W8A8, fp8_out, other_out, reset);
}
extern "C" int atspeed_llama_fp4_counters(atspeed_llama* m, int64_t* fp4_out, int64_t* other_out, int32_t reset) {
  return quant_counters(m, "fp4_counters", SCHEME_W4A8, fp4_out, other_out, reset);
}

extern "C" int64_t atspeed_llama_rope_fused_launches(atspeed_llama* m, int32_t reset) {
  if (!m) return -1;
  const int64_t n = m->rope_fused_cnt;
  if (reset) m->rope_fused_cnt = 0;
  return n;
}

extern "C" float* atspeed_llama_logits(atspeed_llama* m) { return m && m->act ? m->act->logits : nullptr; }
extern "C" int32_t atspeed_llama_logits_ld(const atspeed_llama* m) { return m ? m->logits_ld : 0; }
// the first `bytes` of one of the handle's buffers to dst, ordered on the stream (tests compare what two forms of a forward left)
extern "C" int atspeed_llama_read(atspeed_llama* m, int32_t what, int32_t index, void* dst, size_t bytes, void* stream) {
  ATS_REQUIRE(m && m->act && dst, ATSPEED_ERR_INVALID, "llama_read: null argument");
  const void* src = nullptr; size_t cap = 0;
  if (what == ATSPEED_READ_LOGITS) { src = m->act->logits; cap = (size_t)m->act->cap_rows * m->logits_ld * sizeof(float); }
  else if (what == ATSPEED_READ_LSE) { src = m->act->lse; cap = (size_t)m->act->cap_rows * sizeof(float); }
  else if (what == ATSPEED_READ_HIDDEN) { src = m->act->h; cap = (size_t)m->act->cap_tok * m->cfg.hidden * m->esz; }
  else if (what == ATSPEED_READ_BATCH_K || what == ATSPEED_READ_BATCH_V) {
    ATS_REQUIRE(index >= 0 && index < (int)m->kv_pool.size(), ATSPEED_ERR_INVALID, "llama_read: the pool holds %d caches, not %d", (int)m->kv_pool.size(), index + 1);
    src = what == ATSPEED_READ_BATCH_K ? m->kv_pool[index].k : m->kv_pool[index].v; cap = (size_t)m->cfg.n_layers * m->layer_kv_bytes;
  }
  ATS_REQUIRE(src && bytes <= cap, ATSPEED_ERR_INVALID, "llama_read: buffer %d holds %zu bytes, %zu asked", what, cap, bytes);
  ATS_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return ATSPEED_OK;
}

// The quantised copies of every layer for `scheme`, made by `quant` (allocates one projection's copy and scales, launches its quantiser on st)
// from the model's own 16-bit values with the kernel of its flavour (round 6: the reference loads fp16 checkpoints and runs the target 8-bit,
// code/inference.py:75-91); the activations between the quantised projections stay in that type.  The copies are built aside and reach the
// model only after the last quantiser has run: on any failure the copies made so far are freed and the model is as before.
template <typename Quant>
static int quant_layers_build(atspeed_llama* m, const char* who, int scheme, hipStream_t st, Quant quant) {
  ATS_REQUIRE(m, ATSPEED_ERR_INVALID, "%s: null model", who);
  ATS_REQUIRE(m->cfg.dtype == ATSPEED_BF16 || m->cfg.dtype == ATSPEED_F16, ATSPEED_ERR_INVALID, "%s: the model must hold bf16 or fp16 weights", who);
  ATS_REQUIRE(m->cfg.hidden % 256 == 0 && m->cfg.ffn % 256 == 0, ATSPEED_ERR_INVALID, "%s: hidden and ffn must be multiples of 256", who);
  const int other_bits = scheme == SCHEME_W8A8 ? 4 : 8;
  ATS_REQUIRE(m->scheme == SCHEME_16 || m->scheme == scheme, ATSPEED_ERR_INVALID, "%s: the model already runs the %d-bit target (atspeed_llama_enable_fp%d)",
              who, other_bits, other_bits);
  if (m->scheme == scheme) return ATSPEED_OK;
  std::vector<QuantLayer> q(m->cfg.n_layers);
  int rc = ATSPEED_OK;
  for (int l = 0; rc == ATSPEED_OK && l < m->cfg.n_layers; ++l)
    for (int p = 0; rc == ATSPEED_OK && p < N_PROJ; ++p) {
      const ProjShape s = proj_shape(m->cfg, p);
      rc = quant(proj_weight(m->layers[l], p), s.n, s.k, &q[l].w[p], &q[l].s[p]);
    }
  const hipError_t e = hipStreamSynchronize(st);      // on failure too: the quantisers already launched write the copies
  if (rc != ATSPEED_OK || e != hipSuccess) {
    quant_layers_free(q);
    ATS_TRY(rc);
    ATS_HIP(e);
  }
  m->quant = std::move(q);
  m->scheme = scheme;
  return ATSPEED_OK;
}

extern "C" int atspeed_llama_enable_fp8(atspeed_llama* m, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  return quant_layers_build(m, "enable_fp8", SCHEME_W8A8, st, [&](const void* w, int rows, int cols, void** q, void** sc) -> int {     // packed 16-bit rows -> packed e4m3 rows (or row-major both)
    ATS_HIP(hipMalloc(q, (size_t)((rows + 1) & ~1) * cols));
    ATS_HIP(hipMalloc(sc, (size_t)rows * sizeof(float)));
    return ATS_KD(m->cfg.dtype, ats_quant_rows_fp8(w, rows, cols, cols, *q, (float*)*sc, st, m->pk));
  });
}

extern "C" int atspeed_llama_enable_fp4(atspeed_llama* m, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  return quant_layers_build(m, "enable_fp4", SCHEME_W4A8, st, [&](const void* w, int rows, int cols, void** q, void** sc) -> int {     // 16-bit rows (packed or row-major) -> nibbles + scale bytes (gemm.hip quant_mxfp4_kernel)
    if (hipMalloc(q, (size_t)rows * cols / 2) != hipSuccess || hipMalloc(sc, (size_t)rows * cols / 32) != hipSuccess) {
      atspeed_set_error("enable_fp4: out of device memory for the MXFP4 copies");
      (void)hipGetLastError();
      return ATSPEED_ERR_HIP;
    }
    return ATS_KD(m->cfg.dtype, ats_quant_weights_mxfp4(w, rows, cols, *q, *sc, st, m->pk));
  });
}

// ---- LoRA adapter beside the base (lora.hip) ----
// a model's captured forwards hold the launch sequence of the moment of their capture: setting or clearing an adapter changes it
static void graphs_drop(atspeed_llama* m) {
  ActCtx* cx = m->act;
  if (!cx) return;
  for (auto& g : cx->graphs) hipGraphExecDestroy(g.second);
  cx->graphs.clear();
  cx->graph_seen.clear();
}

extern "C" int atspeed_llama_clear_lora(atspeed_llama* m) {
  ATS_REQUIRE(m, ATSPEED_ERR_INVALID, "clear_lora: null model");
  if (m->lora.empty()) return ATSPEED_OK;
  ATS_HIP(hipDeviceSynchronize());                 // forwards in flight read the copies
  graphs_drop(m);
  m->lora.clear();
  m->lora_gen++;
  hipFree(m->lora_mem);
  m->lora_mem = nullptr;
  m->lora_r16 = 0; m->lora_scaling = 0.f;
  return ATSPEED_OK;
}

// what atspeed_llama_set_lora and atspeed_llama_add_lora share: the checks, then the library's zero-padded copies of one adapter in ONE new
// device block (*mem_out; per layer A_cat, then the three B), complete and waited for, with the model's lora_A output buffer made sure of and
// the device idle.  The model itself is not changed: on failure nothing is left behind.
static int lora_build(atspeed_llama* m, const char* who, int32_t rank, float scaling, const atspeed_lora_layer* layers, hipStream_t st,
                      char** mem_out, std::vector<atspeed_llama::LoraLayer>* ll_out) {
  ATS_REQUIRE(m && layers, ATSPEED_ERR_INVALID, "%s: null argument", who);
  ATS_REQUIRE(rank >= 1 && rank <= ATSPEED_LORA_MAX_RANK, ATSPEED_ERR_INVALID, "%s: rank %d (1 .. %d)", who, rank, ATSPEED_LORA_MAX_RANK);
  ATS_REQUIRE(scaling == scaling && scaling - scaling == 0.f, ATSPEED_ERR_INVALID, "%s: scaling must be finite", who);
  const int L = m->cfg.n_layers, H = m->cfg.hidden, r16 = (rank + 15) / 16 * 16;
  const size_t e = m->esz;
  bool any = false;
  for (int l = 0; l < L; ++l) {
    const void* const ab[3][2] = {{layers[l].a_q, layers[l].b_q}, {layers[l].a_k, layers[l].b_k}, {layers[l].a_v, layers[l].b_v}};
    for (int k = 0; k < 3; ++k) {
      ATS_REQUIRE(!ab[k][0] == !ab[k][1], ATSPEED_ERR_INVALID, "%s: layer %d has one half of a module's (A, B) pair", who, l);
      any = any || ab[k][0];
    }
  }
  ATS_REQUIRE(any, ATSPEED_ERR_INVALID, "%s: no module is adapted (atspeed_llama_clear_lora / _remove_lora take an adapter away)", who);
  // the new copies are built aside; the model changes only after they are complete
  const size_t a_bytes = (size_t)3 * r16 * H * e, b_bytes = (size_t)H * r16 * e;       // multiples of 16 bytes (hidden % 8 == 0, r16 % 16 == 0)
  const size_t per_layer = a_bytes + 3 * b_bytes;
  char* mem = nullptr;
  ATS_HIP(hipMalloc((void**)&mem, per_layer * L));
  std::vector<atspeed_llama::LoraLayer> ll(L);
  auto fill = [&]() -> int {
    ATS_HIP(hipMemsetAsync(mem, 0, per_layer * L, st));
    for (int l = 0; l < L; ++l) {
      char* base = mem + per_layer * l;
      const void* const ab[3][2] = {{layers[l].a_q, layers[l].b_q}, {layers[l].a_k, layers[l].b_k}, {layers[l].a_v, layers[l].b_v}};
      ll[l].a_cat = base;
      for (int k = 0; k < 3; ++k) {
        if (!ab[k][0]) continue;
        char* bdst = base + a_bytes + k * b_bytes;
        ATS_HIP(hipMemcpyAsync(base + (size_t)k * r16 * H * e, ab[k][0], (size_t)rank * H * e, hipMemcpyDeviceToDevice, st));              // A [rank][H] -> rows of A_cat
        ATS_HIP(hipMemcpy2DAsync(bdst, r16 * e, ab[k][1], rank * e, rank * e, H, hipMemcpyDeviceToDevice, st));                          // B [H][rank] -> [H][R16]
        ll[l].b[k] = bdst;
      }
    }
    ATS_HIP(hipStreamSynchronize(st));             // the caller's tensors may go once this returns
    return ATSPEED_OK;
  };
  int rc = fill();
  if (rc == ATSPEED_OK && m->act) rc = lora_u_ensure(m, m->act);
  if (rc == ATSPEED_OK && hipDeviceSynchronize() != hipSuccess) { (void)hipGetLastError(); atspeed_set_error("%s: device synchronisation failed", who); rc = ATSPEED_ERR_HIP; }
  if (rc != ATSPEED_OK) { hipFree(mem); return rc; }
  *mem_out = mem;
  *ll_out = std::move(ll);
  return ATSPEED_OK;
}

extern "C" int atspeed_llama_set_lora(atspeed_llama* m, int32_t rank, float scaling, const atspeed_lora_layer* layers, void* stream) {
  ATS_REQUIRE(!m || m->n_slots == 0, ATSPEED_ERR_INVALID, "set_lora: the model holds %d resident adapters (atspeed_llama_add_lora): a model-wide adapter "
              "and resident slots exclude each other", m->n_slots);
  char* mem = nullptr;
  std::vector<atspeed_llama::LoraLayer> ll;
  ATS_TRY(lora_build(m, "set_lora", rank, scaling, layers, (hipStream_t)stream, &mem, &ll));
  graphs_drop(m);
  hipFree(m->lora_mem);                            // a second adapter replaces the first
  m->lora_mem = mem;
  m->lora = std::move(ll);
  m->lora_gen++;
  m->lora_r16 = (rank + 15) / 16 * 16; m->lora_scaling = scaling;
  return ATSPEED_OK;
}

// ---- resident adapters, picked per user (header: "several RESIDENT adapters on one model")
// the device table as the host knows the slots: written whole, with the device idle (add / remove wait for it first)
static int slot_tab_write(atspeed_llama* m, int slot, const std::vector<atspeed_llama::LoraLayer>* ll) {
  constexpr int NS = ATSPEED_LORA_MAX_ADAPTERS + 1;
  for (int l = 0; l < m->cfg.n_layers; ++l) {
    atspeed_lora_slot e{};                         // ll == NULL: the entry of a freed slot, all zero
    if (ll) e = atspeed_lora_slot{(*ll)[l].a_cat, (*ll)[l].b[0], (*ll)[l].b[1], (*ll)[l].b[2], m->slots[slot].r16, m->slots[slot].scaling};
    ATS_HIP(hipMemcpy(m->slot_tab + (size_t)l * NS + slot, &e, sizeof(e), hipMemcpyHostToDevice));
  }
  return ATSPEED_OK;
}

extern "C" int atspeed_llama_add_lora(atspeed_llama* m, int32_t rank, float scaling, const atspeed_lora_layer* layers, void* stream, int32_t* slot_out) {
  ATS_REQUIRE(m && slot_out, ATSPEED_ERR_INVALID, "add_lora: null argument");
  ATS_REQUIRE(m->lora.empty(), ATSPEED_ERR_INVALID, "add_lora: the model holds a model-wide adapter (atspeed_llama_set_lora): a model-wide adapter and "
              "resident slots exclude each other");
  int slot = 0;
  for (int s = 1; s <= ATSPEED_LORA_MAX_ADAPTERS && !slot; ++s) if (!m->slots[s].mem) slot = s;
  ATS_REQUIRE(slot, ATSPEED_ERR_CAPACITY, "add_lora: all %d slots are occupied", ATSPEED_LORA_MAX_ADAPTERS);
  constexpr int NS = ATSPEED_LORA_MAX_ADAPTERS + 1;
  if (!m->slot_tab) {
    const size_t bytes = (size_t)m->cfg.n_layers * NS * sizeof(atspeed_lora_slot);
    ATS_HIP(hipMalloc((void**)&m->slot_tab, bytes));
    ATS_HIP(hipMemset(m->slot_tab, 0, bytes));
  }
  char* mem = nullptr;
  std::vector<atspeed_llama::LoraLayer> ll;
  ATS_TRY(lora_build(m, "add_lora", rank, scaling, layers, (hipStream_t)stream, &mem, &ll));
  m->slots[slot] = atspeed_llama::LoraSlot{mem, (rank + 15) / 16 * 16, scaling};
  const int rc = slot_tab_write(m, slot, &ll);
  if (rc != ATSPEED_OK) { hipFree(mem); m->slots[slot] = atspeed_llama::LoraSlot{}; return rc; }
  graphs_drop(m);
  m->n_slots++;
  m->slot_gen[slot]++;
  *slot_out = slot;
  return ATSPEED_OK;
}

extern "C" int atspeed_llama_remove_lora(atspeed_llama* m, int32_t slot) {
  ATS_REQUIRE(m, ATSPEED_ERR_INVALID, "remove_lora: null model");
  ATS_REQUIRE(slot >= 1 && slot <= ATSPEED_LORA_MAX_ADAPTERS && m->slots[slot].mem, ATSPEED_ERR_INVALID, "remove_lora: slot %d is not occupied", slot);
  ATS_HIP(hipDeviceSynchronize());                 // forwards in flight read the copies and the table
  graphs_drop(m);
  ATS_TRY(slot_tab_write(m, slot, nullptr));
  hipFree(m->slots[slot].mem);
  m->slots[slot] = atspeed_llama::LoraSlot{};
  m->n_slots--;
  m->slot_gen[slot]++;
  return ATSPEED_OK;
}

extern "C" int32_t atspeed_llama_lora_slots(const atspeed_llama* m) { return m ? m->n_slots : -1; }

extern "C" int64_t atspeed_llama_lora_launches(atspeed_llama* m, int32_t reset) {
  if (!m) return -1;
  const int64_t n = m->lora_cnt;
  if (reset) m->lora_cnt = 0;
  return n;
}

// One forward over the tokens of every segment (user) of the table.  Logits of each segment's last n_logit rows land
// in act->logits rows [logit_row0, ..) (or in logits_out), their log-sum-exp in act->lse.
// What act->h holds afterwards is NOT part of the contract and nothing reads it (no hidden-state export, lora_shrink reads it only inside
// the forward, the teacher path and the tests read logits): after an ordinary forward it is the residual stream behind the last layer, after
// a row-pruned one (forward_prunes_tail) the residual stream in front of the last layer's o_proj -- the last layer's output then exists
// only for the logit rows, in act->gath.
//
// Row-pruned tail: a token row that gets no logits is needed in the LAST layer only for its K and V, which the qkv projection scatters to the
// cache.  Where the rule below holds, the last layer's o_proj, post-attention norm, gate_up, SwiGLU and down run over the R logit rows alone
// (gathered from act->att / act->h into act->att_tail / act->gath); qkv, RoPE, the KV scatter and the attention run over all T rows as in
// every layer, so the caches are bit for bit what the full forward leaves.  Only the last layer: row r's K/V in layer l needs row r's whole
// output of layer l - 1.  The rule: a 16-bit or fp32 target without adapter and without W8A8 / W4A8 copies (their kernels are chosen by the
// forward's token count and that case has not been measured: left on the full path, as staged verification leaves them), at most half
// of the rows get logits, and the forward holds more than "tail_rows_tokens" tokens (below, a projection is bound by its weight stream).
static bool forward_prunes_tail(const atspeed_llama* m, const SegTable& t) {
  return m->plain16() && 2 * t.total_logit <= t.total_tok && t.total_tok > ats_switch(ATS_SW_TAIL_ROWS_TOKENS);
}
static int llama_forward_body(atspeed_llama* m, const SegTable& t, const SegTable* dtab, float* logits_out, hipStream_t st,
                              const unsigned char* tile_store, int logit_row_off);

// tile_store (device bytes, one per 256 vocabulary columns; NULL = every column): which logit tiles the caller will read.  The decoder
// passes its automaton's (atspeed_fsm::d_tile_store): rows then get their full-vocabulary normaliser from the lm_head epilogue and
// only those tiles are written to the logits buffer.
// logit_row_off: the forward's logit rows (and their lse) start at that row of the model's buffers instead of row 0 -- a phase of a staged
// verification round keeps the rows of the phases before it (decoder forwards only: logits_out == NULL)
static int llama_forward_segs(atspeed_llama* m, const SegTable& t, float* logits_out, hipStream_t st, const unsigned char* tile_store = nullptr,
                              int logit_row_off = 0) {
  const atspeed_llama_config& c = m->cfg;
  ActCtx* cx = m->act;
  const int T = t.total_tok;
  ATS_REQUIRE(T >= 1 && T <= cx->cap_tok, ATSPEED_ERR_CAPACITY, "forward: %d tokens exceed the activation capacity %d", T, cx->cap_tok);
  ATS_REQUIRE(logit_row_off >= 0 && (logit_row_off == 0 || !logits_out), ATSPEED_ERR_INVALID, "forward: bad logit row offset %d", logit_row_off);
  ATS_REQUIRE(t.total_logit >= 0 && logit_row_off + t.total_logit <= cx->cap_rows, ATSPEED_ERR_CAPACITY, "forward: %d logit rows exceed the capacity %d",
              logit_row_off + t.total_logit, cx->cap_rows);
  for (int i = 0; i < t.n; ++i) {
    ATS_REQUIRE(t.seg[i].n_tok >= 1 && t.seg[i].n_slots >= 1 && t.seg[i].n_slots <= c.max_slots, ATSPEED_ERR_CAPACITY,
                "forward: segment %d has %d tokens / %d slots (max_slots %d)", i, t.seg[i].n_tok, t.seg[i].n_slots, c.max_slots);
    ATS_REQUIRE(t.seg[i].n_logit >= 0 && t.seg[i].n_logit <= t.seg[i].n_tok, ATSPEED_ERR_INVALID, "forward: bad logit row count");
  }
  if (m->prof_on) prof_harvest(m);
  if (m->fwd_log_on && m->fwd_log.size() < 2 * 4096) { m->fwd_log.push_back(T); m->fwd_log.push_back(t.total_logit); }
  sk_arena_lazy(m, T, st);
  // the table travels through the pinned ring to its fixed device address (stream ordered behind the previous forward)
  ATS_TRY(ats_stage_to(&t, sizeof(t), cx->segtab_dev, st));
  const SegTable* dtab = cx->segtab_dev;
  // opt-in (ATSPEED_GRAPHS=1): measured on MI355X, replaying a 100-token forward as one hipGraph does not shorten it (676 vs 679
  // items/s in the one-user-at-a-time loop) -- the ~10 us between dependent kernels is the GPU's own barrier / cache-flush latency,
  // not host launch cost, and a graph keeps every node boundary
  const int use_graphs = ats_switch(ATS_SW_GRAPHS);                // (atspeed_set_switch("graphs", 1): the tests compare both modes in one process)
  constexpr int graph_max_tok = 512;
  if (use_graphs && !m->prof_on && logits_out == nullptr && logit_row_off == 0 && T <= graph_max_tok) {
    const ActCtx::GraphKey key(T, t.total_logit, t.n, t.n_qtiles, t.qtile_rows, m->scheme, forward_prunes_tail(m, t) ? 1 : 0);
    auto it = cx->graphs.find(key);
    if (it == cx->graphs.end() && cx->graphs.size() < 64 && ++cx->graph_seen[key] >= 2) {   // a shape seen twice recurs (K + dl*DK tokens)
      g_ats_lazy_allocs++;                             // the capture stream (first time) and this shape's graph
      if (!cx->cap_stream) ATS_HIP(hipStreamCreateWithFlags(&cx->cap_stream, hipStreamNonBlocking));
      ATS_HIP(hipStreamBeginCapture(cx->cap_stream, hipStreamCaptureModeThreadLocal));
      const int rc = llama_forward_body(m, t, dtab, nullptr, cx->cap_stream, nullptr, 0);
      hipGraph_t g = nullptr;
      hipError_t e = hipStreamEndCapture(cx->cap_stream, &g);
      if (rc != ATSPEED_OK) { if (g) hipGraphDestroy(g); return rc; }
      ATS_HIP(e);
      hipGraphExec_t ex = nullptr;
      e = hipGraphInstantiate(&ex, g, nullptr, nullptr, 0);
      hipGraphDestroy(g);
      ATS_HIP(e);
      it = cx->graphs.emplace(key, ex).first;
    }
    if (it != cx->graphs.end()) {
      ATS_HIP(hipGraphLaunch(it->second, st));
      return ATSPEED_OK;
    }
  }
  return llama_forward_body(m, t, dtab, logits_out, st, logits_out ? nullptr : tile_store, logit_row_off);
}

namespace fwd_bf16 {
using namespace ats_bf16;
#include "engine_forward.inc"
}
namespace fwd_f16 {
using namespace ats_f16;
#include "engine_forward.inc"
}
static int llama_forward_body(atspeed_llama* m, const SegTable& t, const SegTable* dtab, float* logits_out, hipStream_t st,
                              const unsigned char* tile_store, int logit_row_off) {
  return m->cfg.dtype == ATSPEED_F16 ? fwd_f16::llama_forward_body(m, t, dtab, logits_out, st, tile_store, logit_row_off)
                                     : fwd_bf16::llama_forward_body(m, t, dtab, logits_out, st, tile_store, logit_row_off);
}

extern "C" int atspeed_llama_forward(atspeed_llama* m, const int32_t* ids, const int32_t* pos, const int32_t* slots,
                                     const uint64_t* vis, int32_t n_tokens, int32_t n_slots_visible, int32_t n_logit_rows,
                                     float* logits_out, void* stream) {
  ATS_REQUIRE(m && ids && pos && slots && vis, ATSPEED_ERR_INVALID, "forward: null argument");
  ATS_REQUIRE(n_tokens >= 1 && n_tokens <= m->cfg.max_tokens, ATSPEED_ERR_CAPACITY, "forward: %d tokens exceed max_tokens %d", n_tokens, m->cfg.max_tokens);
  ATS_REQUIRE(n_logit_rows >= 0 && n_logit_rows <= n_tokens && n_logit_rows <= m->cfg.max_logit_rows, ATSPEED_ERR_CAPACITY,
              "forward: %d logit rows exceed the limit %d", n_logit_rows, m->cfg.max_logit_rows);
  SegTable t{};
  t.n = 1; t.total_tok = n_tokens; t.total_logit = n_logit_rows;
  Seg& s = t.seg[0];
  s.ids = ids; s.pos = pos; s.slot = slots; s.vis = vis; s.kc = m->kv0.k; s.vc = m->kv0.v;
  s.row0 = 0; s.n_tok = n_tokens; s.n_slots = n_slots_visible; s.logit_row0 = 0; s.n_logit = n_logit_rows;
  t.n_qtiles = 0; t.qtile_rows = n_tokens > 96 ? 128 : 64;
  for (int j = 0; j * t.qtile_rows < n_tokens; ++j) { t.qtile_seg[t.n_qtiles] = 0; t.qtile_idx[t.n_qtiles++] = (unsigned char)j; }
  return llama_forward_segs(m, t, logits_out, (hipStream_t)stream);
}


// n independent forwards as ONE batched forward (segment table): sequence i has its own token / position / slot / visibility
// arrays and a KV arena of its own from the model's pool; logits of its last n_logit[i] rows follow each other in logits_out.
// What the teacher-data job needs to score the label and the K beams of many samples at once (generate_teacher_data.py:225-232).
extern "C" int atspeed_llama_forward_batch(atspeed_llama* m, int32_t n, const int32_t* const* ids, const int32_t* const* pos,
                                           const int32_t* const* slots, const uint64_t* const* vis, const int32_t* n_tokens,
                                           const int32_t* n_slots_visible, const int32_t* n_logit_rows, float* logits_out,
                                           void* stream) {
  return atspeed_llama_forward_batch_adapters(m, n, ids, pos, slots, vis, n_tokens, n_slots_visible, n_logit_rows, nullptr, logits_out, stream);
}

// the same with one resident adapter slot per sequence (adapters == NULL: none)
extern "C" int atspeed_llama_forward_batch_adapters(atspeed_llama* m, int32_t n, const int32_t* const* ids, const int32_t* const* pos,
                                                    const int32_t* const* slots, const uint64_t* const* vis, const int32_t* n_tokens,
                                                    const int32_t* n_slots_visible, const int32_t* n_logit_rows, const int32_t* adapters,
                                                    float* logits_out, void* stream) {
  ATS_REQUIRE(m && ids && pos && slots && vis && n_tokens && n_slots_visible && n_logit_rows && logits_out, ATSPEED_ERR_INVALID,
              "forward_batch: null argument");
  ATS_REQUIRE(n >= 1 && n <= ATS_MAX_SEGS, ATSPEED_ERR_CAPACITY, "forward_batch: %d sequences per call (max %d)", n, ATS_MAX_SEGS);
  for (int i = 0; adapters && i < n; ++i)
    ATS_REQUIRE(m->slot_ok(adapters[i]), ATSPEED_ERR_INVALID, "forward_batch: sequence %d names adapter slot %d, which is not occupied", i, adapters[i]);
  while ((int)m->kv_pool.size() < n) {
    KvCache kv;
    ATS_TRY(kv_create(m, &kv));
    m->kv_pool.push_back(kv);
  }
  SegTable t{};
  int tot = 0, rows = 0;
  for (int i = 0; i < n; ++i) {
    ATS_REQUIRE(ids[i] && pos[i] && slots[i] && vis[i], ATSPEED_ERR_INVALID, "forward_batch: null array for sequence %d", i);
    ATS_REQUIRE(n_tokens[i] >= 1 && n_tokens[i] <= m->cfg.max_tokens, ATSPEED_ERR_CAPACITY, "forward_batch: %d tokens exceed max_tokens %d",
                n_tokens[i], m->cfg.max_tokens);
    ATS_REQUIRE(n_logit_rows[i] >= 0 && n_logit_rows[i] <= n_tokens[i], ATSPEED_ERR_INVALID, "forward_batch: bad logit row count");
    Seg& sg = t.seg[t.n++];
    sg.ids = ids[i]; sg.pos = pos[i]; sg.slot = slots[i]; sg.vis = vis[i]; sg.kc = m->kv_pool[i].k; sg.vc = m->kv_pool[i].v;
    sg.n_tok = n_tokens[i]; sg.n_slots = n_slots_visible[i]; sg.n_logit = n_logit_rows[i];
    sg.adapter = adapters ? adapters[i] : 0;
    tot += n_tokens[i]; rows += n_logit_rows[i];
  }
  ATS_TRY(ats_seg_finish(t));
  ATS_TRY(ensure_act(m, tot, rows));
  return llama_forward_segs(m, t, logits_out, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------- scoring candidates
// The exact target log-prob of every item of a list per user from ONE segmented forward (include/atspeed_hip.h "scoring candidates"): the
// lists are staged into the model's score block, the tree builder packs each user's prompt + prefix-sharing tree, the forward runs the
// decoder's lm_head form (full-vocabulary normaliser from the epilogue, only the automaton's logit tiles stored) and the path-score kernel
// adds each item's terms as a beam search would (beamSD.py:58-64).
// rows a user's list packs to, prompt included, by the builder's own rule: e(s) = min(lcp(s), len(s - 1) - 1), len(s) - 1 - e(s) new rows
static int64_t score_tree_rows(const int32_t* tok, const int32_t* off, int s0, int s1, int P) {
  int64_t rows = P;
  for (int s = s0; s < s1; ++s) {
    const int L = off[s + 1] - off[s];
    int e = 0;
    if (s > s0) {
      const int Lp = off[s] - off[s - 1];
      int lcp = 0;
      while (lcp < L && lcp < Lp && tok[off[s - 1] + lcp] == tok[off[s] + lcp]) ++lcp;
      e = std::max(0, std::min(lcp, Lp - 1));
    }
    rows += std::max(0, L - 1 - e);
  }
  return rows;
}

extern "C" int atspeed_score_items(atspeed_llama* m, const atspeed_fsm* fsm, int32_t n_users, const int32_t* const* prompt_ids,
                                   const int32_t* prompt_len, const int32_t* start_nodes, const int32_t* seq_tokens, const int32_t* seq_offsets,
                                   const int32_t* user_seq_offsets, const int32_t* adapter_slots, float* scores_out, int32_t* unknown_out,
                                   int32_t* status_out, void* stream) {
  ATS_REQUIRE(m && fsm && prompt_ids && prompt_len && start_nodes && seq_tokens && seq_offsets && user_seq_offsets && scores_out && status_out,
              ATSPEED_ERR_INVALID, "score_items: null argument");
  ATS_REQUIRE(fsm->dev.n_nodes > 0 && fsm->dev.vocab == m->cfg.vocab_size, ATSPEED_ERR_INVALID,
              "score_items: needs a constraint automaton over the model's vocabulary (a mask-free search knows no items)");
  ATS_REQUIRE(n_users >= 1 && n_users <= ATS_MAX_SEGS, ATSPEED_ERR_CAPACITY, "score_items: %d users per call (1 .. %d)", n_users, ATS_MAX_SEGS);
  ATS_REQUIRE(user_seq_offsets[0] == 0 && seq_offsets[0] == 0, ATSPEED_ERR_INVALID, "score_items: offsets must start at 0");
  const atspeed_llama_config& c = m->cfg;
  for (int u = 0; u < n_users; ++u) {
    ATS_REQUIRE(user_seq_offsets[u + 1] > user_seq_offsets[u], ATSPEED_ERR_INVALID, "score_items: user %d has no sequence", u);
    ATS_REQUIRE(prompt_ids[u] && prompt_len[u] >= 1, ATSPEED_ERR_INVALID, "score_items: user %d has no prompt", u);
    ATS_REQUIRE(start_nodes[u] >= 0 && start_nodes[u] < fsm->dev.n_nodes, ATSPEED_ERR_INVALID, "score_items: start node of user %d out of range", u);
    ATS_REQUIRE(!adapter_slots || m->slot_ok(adapter_slots[u]), ATSPEED_ERR_INVALID, "score_items: user %d names adapter slot %d, which is not occupied", u,
                adapter_slots ? adapter_slots[u] : 0);
  }
  const int n_seq = user_seq_offsets[n_users];
  for (int s = 0; s < n_seq; ++s) {
    const int64_t len = (int64_t)seq_offsets[s + 1] - seq_offsets[s];
    ATS_REQUIRE(len >= 1 && len <= ATSPEED_MAX_NEW_TOKENS, ATSPEED_ERR_INVALID, "score_items: sequence %d holds %lld tokens (1 .. %d)", s, (long long)len,
                ATSPEED_MAX_NEW_TOKENS);
  }
  const int n_tok = seq_offsets[n_seq];
  hipStream_t st = (hipStream_t)stream;
  // per user: rows by the lcp rule, and whether they fit the model (found here, before anything is launched; the others are still scored)
  std::vector<int> rows((size_t)n_users), status((size_t)n_users, ATSPEED_OK);
  std::vector<size_t> row0((size_t)n_users + 1, 0);
  for (int u = 0; u < n_users; ++u) {
    const int64_t r = score_tree_rows(seq_tokens, seq_offsets, user_seq_offsets[u], user_seq_offsets[u + 1], prompt_len[u]);
    const bool fits = r <= c.max_tokens && r <= c.max_slots && r - (prompt_len[u] - 1) <= c.max_logit_rows;
    rows[u] = fits ? (int)r : 0;
    if (!fits) status[u] = ATSPEED_ERR_CAPACITY;
    row0[u + 1] = row0[u] + (size_t)rows[u];
  }
  // the model's score block: lists, per-user records and results, per-sequence tables, then the packed rows of every user
  const int W = m->vis_words;
  const size_t total_rows = row0[n_users];
  auto up = [](size_t x) { return (x + 15) / 16 * 16; };
  size_t o = 0;
  const size_t o_users = o;  o += up(sizeof(ScoreTreeUser) * n_users);
  const size_t o_vis = o;    o += up(sizeof(uint64_t) * std::max<size_t>(total_rows, 1) * W);
  const size_t o_tok = o;    o += up(4 * (size_t)n_tok);
  const size_t o_off = o;    o += up(4 * ((size_t)n_seq + 1));
  const size_t o_pred = o;   o += up(4 * (size_t)n_seq * ATSPEED_MAX_NEW_TOKENS);
  const size_t o_known = o;  o += up(4 * (size_t)n_seq);
  const size_t o_base = o;   o += up(4 * (size_t)n_seq);
  const size_t o_res = o;    o += up(4 * 3 * (size_t)n_users);
  const size_t o_rows = o;   o += up(4 * 3 * std::max<size_t>(total_rows, 1));
  if (o > m->score_bytes) {
    ATS_HIP(hipStreamSynchronize(st));                                  // an earlier call's launches may still read the old block
    hipFree(m->score_mem); m->score_mem = nullptr; m->score_bytes = 0;
    g_ats_lazy_allocs++;
    const size_t want = o + o / 4;
    ATS_HIP(hipMalloc(&m->score_mem, want));
    m->score_bytes = want;
  }
  char* blk = (char*)m->score_mem;
  int32_t* d_tok = (int32_t*)(blk + o_tok);
  int32_t* d_off = (int32_t*)(blk + o_off);
  int32_t* d_pred = (int32_t*)(blk + o_pred);
  int32_t* d_known = (int32_t*)(blk + o_known);
  int32_t* d_base = (int32_t*)(blk + o_base);
  int32_t* d_res = (int32_t*)(blk + o_res);                             // n_rows | unknown | status, [n_users] each
  int32_t* d_rows = (int32_t*)(blk + o_rows);                           // ids | pos | slot, [total_rows] each
  uint64_t* d_vis = (uint64_t*)(blk + o_vis);
  std::vector<ScoreTreeUser> users((size_t)n_users);
  for (int u = 0; u < n_users; ++u) {
    ScoreTreeUser& su = users[u];
    su.prompt = prompt_ids[u]; su.P = prompt_len[u]; su.start = start_nodes[u]; su.s0 = user_seq_offsets[u]; su.s1 = user_seq_offsets[u + 1];
    su.cap = rows[u]; su.pad = 0;                                       // a user that does not fit writes no row at all
    su.ids = d_rows + row0[u]; su.pos = d_rows + total_rows + row0[u]; su.slot = d_rows + 2 * total_rows + row0[u];
    su.vis = d_vis + row0[u] * W;
  }
  ATS_HIP(hipMemcpyAsync(blk + o_users, users.data(), sizeof(ScoreTreeUser) * n_users, hipMemcpyHostToDevice, st));
  ATS_HIP(hipMemcpyAsync(d_tok, seq_tokens, 4 * (size_t)n_tok, hipMemcpyHostToDevice, st));
  ATS_HIP(hipMemcpyAsync(d_off, seq_offsets, 4 * ((size_t)n_seq + 1), hipMemcpyHostToDevice, st));
  ScoreTreeBuild b{};
  b.fsm = fsm->dev; b.users = (const ScoreTreeUser*)(blk + o_users); b.seq_tok = d_tok; b.seq_off = d_off; b.n_tok = n_tok;
  b.pred_row = d_pred; b.known = d_known; b.n_rows = d_res; b.unknown = d_res + n_users; b.status = d_res + 2 * n_users; b.vis_words = W;
  ATS_TRY(ats_score_tree_build(b, n_users, st));
  // what the builder found: its row count must be the host's, and an unsorted list is refused -- before such a user's rows reach a forward
  std::vector<int32_t> res(3 * (size_t)n_users);
  ATS_HIP(hipMemcpyAsync(res.data(), d_res, 4 * res.size(), hipMemcpyDeviceToHost, st));
  ATS_HIP(hipStreamSynchronize(st));
  ats_stage_reset();
  for (int u = 0; u < n_users; ++u) {
    if (unknown_out) unknown_out[u] = res[n_users + u];
    if (status[u] != ATSPEED_OK) continue;
    if (res[2 * n_users + u] != ATSPEED_OK || res[u] != rows[u]) status[u] = ATSPEED_ERR_INVALID;
  }
  // one segment (and KV arena of the pool) per user that is left
  SegTable t{};
  std::vector<int32_t> base((size_t)n_seq, -(1 << 30));                 // a refused user's sequences name no row: -inf
  int tot = 0, lrows = 0;
  for (int u = 0; u < n_users; ++u) {
    if (status[u] != ATSPEED_OK) continue;
    while ((int)m->kv_pool.size() <= t.n) {
      KvCache kv;
      ATS_TRY(kv_create(m, &kv));
      m->kv_pool.push_back(kv);
    }
    Seg& sg = t.seg[t.n];
    sg.ids = users[u].ids; sg.pos = users[u].pos; sg.slot = users[u].slot; sg.vis = users[u].vis;
    sg.kc = m->kv_pool[t.n].k; sg.vc = m->kv_pool[t.n].v;
    sg.n_tok = rows[u]; sg.n_slots = rows[u]; sg.n_logit = rows[u] - (prompt_len[u] - 1);
    sg.adapter = adapter_slots ? adapter_slots[u] : 0;
    // segment row r's logits are row lrows + r - (P - 1) of the model's buffer: the prompt's last row is the segment's first logit row
    for (int s = user_seq_offsets[u]; s < user_seq_offsets[u + 1]; ++s) base[s] = lrows - (prompt_len[u] - 1);
    tot += sg.n_tok; lrows += sg.n_logit;
    t.n++;
  }
  for (int u = 0; u < n_users; ++u) status_out[u] = status[u];
  ATS_HIP(hipMemcpyAsync(d_base, base.data(), 4 * (size_t)n_seq, hipMemcpyHostToDevice, st));
  if (t.n > 0) {
    ATS_TRY(ats_seg_finish(t));
    ATS_TRY(ensure_act(m, tot, lrows));
    ATS_TRY(llama_forward_segs(m, t, nullptr, st, fsm->d_tile_store));
  }
  // with no user left there is no forward and no row: every score is -inf (n_rows = 1 keeps the kernel's range test meaningful)
  const float* lg = t.n > 0 ? m->act->logits : (const float*)d_base;
  const float* ls = t.n > 0 ? m->act->lse : (const float*)d_base;
  ATS_TRY(ats_path_scores(lg, m->logits_ld, ls, std::max(lrows, 1), c.vocab_size, d_tok, d_off, d_pred, d_base, d_known, n_seq, scores_out, st));
  ATS_HIP(hipStreamSynchronize(st));                                    // the host vectors staged above die with this call
  ats_stage_reset();
  return ATSPEED_OK;
}

// ---------------------------------------------------------------------------- segment-table kernels, one at a time (tests)
// The low-level atspeed_segs_* entry points describe their segments as atspeed_llama_forward_batch does -- host arrays of n device pointers
// and counts -- except that the caches are the caller's.  This builds the table with the engine's own ats_seg_finish and stages it; `need`
// names the per-segment arrays the wrapper's kernel reads (the others may be NULL).
enum { SEGS_IDS = 1, SEGS_POS = 2, SEGS_SLOTS = 4, SEGS_VIS = 8, SEGS_KV = 16 };
static int segs_table(const char* who, int need, int qtile_rows, int32_t n, const int32_t* const* ids, const int32_t* const* pos,
                      const int32_t* const* slots, const uint64_t* const* vis, void* const* kcache, void* const* vcache, const int32_t* n_tokens,
                      const int32_t* n_slots_visible, const int32_t* n_logit_rows, hipStream_t st, SegTable& t, const SegTable** dt,
                      const int32_t* adapters = nullptr /* [n] resident adapter slot per segment: the _multi adapter kernels */) {
  ATS_REQUIRE(n_tokens && n_slots_visible && n_logit_rows, ATSPEED_ERR_INVALID, "%s: null count array", who);
  ATS_REQUIRE(n >= 1 && n <= ATS_MAX_SEGS, ATSPEED_ERR_CAPACITY, "%s: %d segments per call (max %d)", who, n, ATS_MAX_SEGS);
  ATS_REQUIRE(qtile_rows == 0 || qtile_rows == 64 || qtile_rows == 128 || qtile_rows == 256, ATSPEED_ERR_INVALID, "%s: query tile of %d rows", who, qtile_rows);
  ATS_REQUIRE((!(need & SEGS_IDS) || ids) && (!(need & SEGS_POS) || pos) && (!(need & SEGS_SLOTS) || slots) && (!(need & SEGS_VIS) || vis) &&
              (!(need & SEGS_KV) || (kcache && vcache)), ATSPEED_ERR_INVALID, "%s: null segment array", who);
  t.n = 0;
  for (int i = 0; i < n; ++i) {
    ATS_REQUIRE(n_tokens[i] >= 1 && n_slots_visible[i] >= 0 && n_logit_rows[i] >= 0 && n_logit_rows[i] <= n_tokens[i], ATSPEED_ERR_INVALID,
                "%s: bad counts for segment %d", who, i);
    ATS_REQUIRE((n_tokens[i] + (qtile_rows ? qtile_rows : 64) - 1) / (qtile_rows ? qtile_rows : 64) <= 256, ATSPEED_ERR_CAPACITY,
                "%s: segment %d has too many query tiles", who, i);
    Seg& sg = t.seg[t.n++];
    sg.ids = ids ? ids[i] : nullptr; sg.pos = pos ? pos[i] : nullptr; sg.slot = slots ? slots[i] : nullptr; sg.vis = vis ? vis[i] : nullptr;
    sg.kc = kcache ? kcache[i] : nullptr; sg.vc = vcache ? vcache[i] : nullptr;
    ATS_REQUIRE((!(need & SEGS_IDS) || sg.ids) && (!(need & SEGS_POS) || sg.pos) && (!(need & SEGS_SLOTS) || sg.slot) && (!(need & SEGS_VIS) || sg.vis) &&
                (!(need & SEGS_KV) || (sg.kc && sg.vc)), ATSPEED_ERR_INVALID, "%s: null array for segment %d", who, i);
    sg.n_tok = n_tokens[i]; sg.n_slots = n_slots_visible[i]; sg.n_logit = n_logit_rows[i];
    sg.adapter = adapters ? adapters[i] : 0;
  }
  ATS_TRY(ats_seg_finish(t, qtile_rows));
  const void* p = nullptr;
  ATS_TRY(ats_stage(&t, sizeof(t), &p, st));
  *dt = (const SegTable*)p;
  return ATSPEED_OK;
}
static bool segs_dtype_ok(int dtype) { return dtype == ATSPEED_F32 || dtype == ATSPEED_BF16 || dtype == ATSPEED_F16; }
#define ATS_SEGS_PARAMS int32_t n, const int32_t* const* ids, const int32_t* const* pos, const int32_t* const* slots, const uint64_t* const* vis, \
                        void* const* kcache, void* const* vcache, const int32_t* n_tokens, const int32_t* n_slots_visible, const int32_t* n_logit_rows
#define ATS_SEGS_ARGS n, ids, pos, slots, vis, kcache, vcache, n_tokens, n_slots_visible, n_logit_rows

// out[row][:] = table[clamp(id of the row, 0, vocab - 1)][:] for the total_tok rows of the segments (embed_segs_kernel); tests/test_segs_gpu.py::test_embed_gather_row_info
extern "C" int atspeed_segs_embed(const void* table, int32_t hidden, int32_t vocab, int32_t dtype, void* out, ATS_SEGS_PARAMS, void* stream) {
  ATS_REQUIRE(table && out && hidden > 0 && vocab > 0 && segs_dtype_ok(dtype), ATSPEED_ERR_INVALID, "segs_embed: bad arguments");
  ATS_REQUIRE(hidden * (dtype == ATSPEED_F32 ? 4 : 2) % 16 == 0 && (((uintptr_t)table | (uintptr_t)out) & 15) == 0, ATSPEED_ERR_INVALID,
              "segs_embed: rows must be whole, aligned 16-byte chunks");
  SegTable t{}; const SegTable* dt = nullptr;
  ATS_TRY(segs_table("segs_embed", SEGS_IDS, 0, ATS_SEGS_ARGS, (hipStream_t)stream, t, &dt));
  return ATS_KD(dtype, ats_embed_segs(table, t, dt, out, hidden, vocab, dtype, (hipStream_t)stream));
}

// out = the last n_logit_rows[i] rows of every segment of h, one after the other (gather_logit_rows_kernel); ::test_embed_gather_row_info
extern "C" int atspeed_segs_gather_logit_rows(const void* h, int32_t hidden, int32_t dtype, void* out, ATS_SEGS_PARAMS, void* stream) {
  ATS_REQUIRE(h && out && hidden > 0 && segs_dtype_ok(dtype), ATSPEED_ERR_INVALID, "segs_gather_logit_rows: bad arguments");
  ATS_REQUIRE(hidden * (dtype == ATSPEED_F32 ? 4 : 2) % 16 == 0 && (((uintptr_t)h | (uintptr_t)out) & 15) == 0, ATSPEED_ERR_INVALID,
              "segs_gather_logit_rows: rows must be whole, aligned 16-byte chunks");
  SegTable t{}; const SegTable* dt = nullptr;
  ATS_TRY(segs_table("segs_gather_logit_rows", 0, 0, ATS_SEGS_ARGS, (hipStream_t)stream, t, &dt));
  return ATS_KD(dtype, ats_gather_logit_rows(h, t, dt, out, hidden, dtype, (hipStream_t)stream));
}

// the same rows of h (row-major) and of att (packed = 1: in the packed operand layout) to h_out / att_out in one launch (gather_tail_rows_kernel);
// tests/test_tail_rows_gpu.py::test_gather_guard_band
extern "C" int atspeed_segs_gather_tail_rows(const void* h, const void* att, int32_t hidden, int32_t dtype, int32_t packed, void* h_out, void* att_out,
                                             ATS_SEGS_PARAMS, void* stream) {
  ATS_REQUIRE(h && att && h_out && att_out && hidden > 0 && segs_dtype_ok(dtype), ATSPEED_ERR_INVALID, "segs_gather_tail_rows: bad arguments");
  ATS_REQUIRE((((uintptr_t)h | (uintptr_t)att | (uintptr_t)h_out | (uintptr_t)att_out) & 15) == 0, ATSPEED_ERR_INVALID,
              "segs_gather_tail_rows: buffers must be 16-byte aligned");
  SegTable t{}; const SegTable* dt = nullptr;
  ATS_TRY(segs_table("segs_gather_tail_rows", 0, 0, ATS_SEGS_ARGS, (hipStream_t)stream, t, &dt));
  return ATS_KD(dtype, ats_gather_tail_rows(h, att, t, dt, h_out, att_out, hidden, dtype, (hipStream_t)stream, packed ? 1 : 0));
}

// out[row] = {kcache, vcache of the row's segment, clamp(pos, 0, max_pos - 1), slot} (row_info_kernel; record layout: the header); ::test_embed_gather_row_info
extern "C" int atspeed_segs_row_info(void* out, int32_t max_pos, ATS_SEGS_PARAMS, void* stream) {
  ATS_REQUIRE(out && max_pos >= 1 && ((uintptr_t)out & 7) == 0, ATSPEED_ERR_INVALID, "segs_row_info: bad arguments");
  SegTable t{}; const SegTable* dt = nullptr;
  ATS_TRY(segs_table("segs_row_info", SEGS_POS | SEGS_SLOTS, 0, ATS_SEGS_ARGS, (hipStream_t)stream, t, &dt));
  return ats_bf16::ats_row_info(t, dt, (RowInfo*)out, max_pos, (hipStream_t)stream);
}

// the separate RoPE + KV-scatter pass on qkv [total_tok][3 * n_heads * head_dim]: q rotated in place, rotated k and v to row `slot` of the
// segment's caches at layer_off_bytes (slabs == NULL: ats_rope_kv_segs; else the slab-summing form on fp32 [splits][total_tok][3 hidden]);
// ::test_rope_kv, ::test_rope_kv_slabs
extern "C" int atspeed_segs_rope_kv(void* qkv, const float* slabs, int32_t splits, const float* cos_tab, const float* sin_tab, size_t layer_off_bytes,
                                    int32_t n_heads, int32_t head_dim, int32_t max_pos, int32_t dtype, ATS_SEGS_PARAMS, void* stream) {
  ATS_REQUIRE(qkv && cos_tab && sin_tab && n_heads >= 1 && head_dim >= 2 && head_dim % 2 == 0 && max_pos >= 1 && segs_dtype_ok(dtype), ATSPEED_ERR_INVALID,
              "segs_rope_kv: bad arguments");
  ATS_REQUIRE(((uintptr_t)qkv & 15) == 0 && layer_off_bytes % 16 == 0, ATSPEED_ERR_INVALID, "segs_rope_kv: qkv and the layer offset must be 16-byte aligned");
  ATS_REQUIRE(!slabs || (dtype != ATSPEED_F32 && splits >= 1 && ((uintptr_t)slabs & 15) == 0), ATSPEED_ERR_INVALID, "segs_rope_kv: slabs need a 16-bit type, splits >= 1 and 16-byte alignment");
  SegTable t{}; const SegTable* dt = nullptr;
  ATS_TRY(segs_table("segs_rope_kv", SEGS_POS | SEGS_SLOTS | SEGS_KV, 0, ATS_SEGS_ARGS, (hipStream_t)stream, t, &dt));
  if (slabs) return ATS_KD(dtype, ats_rope_kv_segs_slabs(slabs, splits, qkv, t, dt, cos_tab, sin_tab, layer_off_bytes, n_heads, head_dim, max_pos, (hipStream_t)stream));
  return ATS_KD(dtype, ats_rope_kv_segs(qkv, t, dt, cos_tab, sin_tab, layer_off_bytes, n_heads, head_dim, max_pos, dtype, (hipStream_t)stream));
}

// tree attention of every segment's rows over that segment's own caches (at layer_off_bytes), n_slots and visibility words: the lock-step form
// of atspeed_tree_attention_tiled (qtile_rows 0 / 64 / 128 / 256, rows_per_wave 0 / 16 / 32 as there); packed_out: out in the packed operand
// layout (16-bit, ldo % 32 == 0).  ::test_tree_attention_segs, ::test_tree_attention_segs_many32
extern "C" int atspeed_segs_tree_attention(const void* q, int32_t ldq, size_t layer_off_bytes, int32_t vis_words, void* out, int32_t ldo, int32_t n_heads,
                                           int32_t head_dim, int32_t dtype, int32_t qtile_rows, int32_t rows_per_wave, int32_t packed_out, ATS_SEGS_PARAMS,
                                           void* stream) {
  ATS_REQUIRE(q && out && n_heads >= 1 && head_dim >= 1 && vis_words >= 1 && segs_dtype_ok(dtype), ATSPEED_ERR_INVALID, "segs_tree_attention: bad arguments");
  ATS_REQUIRE(ldq >= 3 * n_heads * head_dim && ldo >= n_heads * head_dim && layer_off_bytes % 16 == 0, ATSPEED_ERR_INVALID, "segs_tree_attention: bad strides");
  ATS_REQUIRE(rows_per_wave == 0 || rows_per_wave == 16 || rows_per_wave == 32, ATSPEED_ERR_INVALID, "segs_tree_attention: %d rows per wave", rows_per_wave);
  SegTable t{}; const SegTable* dt = nullptr;
  ATS_TRY(segs_table("segs_tree_attention", SEGS_VIS | SEGS_KV, qtile_rows, ATS_SEGS_ARGS, (hipStream_t)stream, t, &dt));
  return ATS_KD(dtype, ats_tree_attention_segs(q, ldq, t, dt, layer_off_bytes, vis_words, out, ldo, n_heads, head_dim, dtype, (hipStream_t)stream, rows_per_wave,
                                               packed_out ? 1 : 0));
}

// what atspeed_segs_lora_rope_kv and its per-segment form ask of the arguments they share
static int segs_lora_rope_args(const char* who, const void* qkv, const void* u, const float* cos_tab, const float* sin_tab, size_t layer_off_bytes,
                               int32_t n_heads, int32_t head_dim, int32_t max_pos, int32_t dtype) {
  ATS_REQUIRE(qkv && u && cos_tab && sin_tab && n_heads >= 1 && head_dim >= 2 && head_dim % 2 == 0 && max_pos >= 1 && segs_dtype_ok(dtype), ATSPEED_ERR_INVALID,
              "%s: bad arguments", who);
  ATS_REQUIRE(((uintptr_t)qkv & 15) == 0 && layer_off_bytes % 16 == 0, ATSPEED_ERR_INVALID, "%s: qkv and the layer offset must be 16-byte aligned", who);
  return ATSPEED_OK;
}

// atspeed_segs_rope_kv with the adapter's expand in front (lora_rope_kv_segs kernels with one adapter for every row; header: the memory
// contract); tests/test_lora_gpu.py
extern "C" int atspeed_segs_lora_rope_kv(void* qkv, const void* u, const void* b_q, const void* b_k, const void* b_v, int32_t r16, float scaling,
                                         const float* cos_tab, const float* sin_tab, size_t layer_off_bytes, int32_t n_heads, int32_t head_dim,
                                         int32_t max_pos, int32_t dtype, ATS_SEGS_PARAMS, void* stream) {
  ATS_TRY(segs_lora_rope_args("segs_lora_rope_kv", qkv, u, cos_tab, sin_tab, layer_off_bytes, n_heads, head_dim, max_pos, dtype));
  SegTable t{}; const SegTable* dt = nullptr;
  ATS_TRY(segs_table("segs_lora_rope_kv", SEGS_POS | SEGS_SLOTS | SEGS_KV, 0, ATS_SEGS_ARGS, (hipStream_t)stream, t, &dt));
  return ATS_KD(dtype, ats_lora_rope_kv_segs(qkv, u, b_q, b_k, b_v, r16, scaling, t, dt, cos_tab, sin_tab, layer_off_bytes, n_heads, head_dim, max_pos, dtype,
                                             (hipStream_t)stream));
}

// the caller's HOST slot array checked and staged as the fixed-size device table the segmented adapter kernels index (entries from n_slots on:
// none); *aligned: every a_cat and B is 16-byte aligned
static int segs_lora_slots(const char* who, const atspeed_lora_slot* slots, int32_t n_slots, const int32_t* seg_adapters, int32_t n, bool need_a,
                           hipStream_t st, const atspeed_lora_slot** dev_out, bool* aligned) {
  constexpr int NS = ATSPEED_LORA_MAX_ADAPTERS + 1;
  ATS_REQUIRE(slots && seg_adapters && n_slots >= 1 && n_slots <= NS, ATSPEED_ERR_INVALID, "%s: needs 1 .. %d slots and one slot index per segment", who, NS);
  atspeed_lora_slot tab[NS] = {};
  *aligned = true;
  for (int s = 1; s < n_slots; ++s) {
    tab[s] = slots[s];
    if (!slots[s].a_cat && !slots[s].b_q && !slots[s].b_k && !slots[s].b_v) { tab[s] = atspeed_lora_slot{}; continue; }     // an empty entry: no segment may name it
    ATS_REQUIRE(slots[s].r16 >= 16 && slots[s].r16 <= ATSPEED_LORA_MAX_RANK && slots[s].r16 % 16 == 0, ATSPEED_ERR_INVALID,
                "%s: slot %d has a padded rank of %d (16, 32, 48 or 64)", who, s, slots[s].r16);
    ATS_REQUIRE(!need_a || slots[s].a_cat, ATSPEED_ERR_INVALID, "%s: slot %d has no a_cat", who, s);
    if ((((uintptr_t)slots[s].a_cat | (uintptr_t)slots[s].b_q | (uintptr_t)slots[s].b_k | (uintptr_t)slots[s].b_v) & 15) != 0) *aligned = false;
  }
  for (int i = 0; i < n && i < ATS_MAX_SEGS; ++i)
    ATS_REQUIRE(seg_adapters[i] >= 0 && seg_adapters[i] < n_slots && (seg_adapters[i] == 0 || tab[seg_adapters[i]].r16), ATSPEED_ERR_INVALID,
                "%s: segment %d names slot %d, which the table does not hold", who, i, seg_adapters[i]);
  const void* p = nullptr;
  ATS_TRY(ats_stage(tab, sizeof(tab), &p, st));
  *dev_out = (const atspeed_lora_slot*)p;
  return ATSPEED_OK;
}

// lora_shrink with the adapter picked per segment (the shrink kernels over LoraBySeg; header: the memory contract); tests/test_lora_multi_gpu.py
extern "C" int atspeed_segs_lora_shrink_multi(const void* h, const void* norm_w, const atspeed_lora_slot* lora_slots, int32_t n_slots, void* u, int32_t hidden,
                                              float eps, int32_t dtype, const int32_t* seg_adapters, ATS_SEGS_PARAMS, void* stream) {
  ATS_REQUIRE(h && norm_w && u && hidden > 0 && segs_dtype_ok(dtype), ATSPEED_ERR_INVALID, "segs_lora_shrink_multi: bad arguments");
  const atspeed_lora_slot* dslots = nullptr;
  bool aligned = false;
  ATS_TRY(segs_lora_slots("segs_lora_shrink_multi", lora_slots, n_slots, seg_adapters, n, true, (hipStream_t)stream, &dslots, &aligned));
  SegTable t{}; const SegTable* dt = nullptr;
  ATS_TRY(segs_table("segs_lora_shrink_multi", 0, 0, ATS_SEGS_ARGS, (hipStream_t)stream, t, &dt, seg_adapters));
  return ATS_KD(dtype, ats_lora_shrink_segs(h, norm_w, dslots, aligned, u, t, dt, hidden, eps, dtype, (hipStream_t)stream));
}

// atspeed_segs_lora_rope_kv with the adapter picked per segment (the same kernels over LoraBySeg); tests/test_lora_multi_gpu.py
extern "C" int atspeed_segs_lora_rope_kv_multi(void* qkv, const void* u, const atspeed_lora_slot* lora_slots, int32_t n_slots, const float* cos_tab,
                                               const float* sin_tab, size_t layer_off_bytes, int32_t n_heads, int32_t head_dim, int32_t max_pos,
                                               int32_t dtype, const int32_t* seg_adapters, ATS_SEGS_PARAMS, void* stream) {
  ATS_TRY(segs_lora_rope_args("segs_lora_rope_kv_multi", qkv, u, cos_tab, sin_tab, layer_off_bytes, n_heads, head_dim, max_pos, dtype));
  const atspeed_lora_slot* dslots = nullptr;
  bool aligned = false;
  ATS_TRY(segs_lora_slots("segs_lora_rope_kv_multi", lora_slots, n_slots, seg_adapters, n, false, (hipStream_t)stream, &dslots, &aligned));
  ATS_REQUIRE(aligned || dtype == ATSPEED_F32 || head_dim % 16 != 0, ATSPEED_ERR_INVALID, "segs_lora_rope_kv_multi: every B must be 16-byte aligned");
  SegTable t{}; const SegTable* dt = nullptr;
  ATS_TRY(segs_table("segs_lora_rope_kv_multi", SEGS_POS | SEGS_SLOTS | SEGS_KV, 0, ATS_SEGS_ARGS, (hipStream_t)stream, t, &dt, seg_adapters));
  return ATS_KD(dtype, ats_lora_rope_kv_segs_multi(qkv, u, dslots, t, dt, cos_tab, sin_tab, layer_off_bytes, n_heads, head_dim, max_pos, dtype,
                                                   (hipStream_t)stream));
}
#undef ATS_SEGS_PARAMS
#undef ATS_SEGS_ARGS

// ---------------------------------------------------------------------------- decoder
namespace {
constexpr int MAXB = ATSPEED_MAX_BEAMS;
constexpr int LMAX = ATSPEED_MAX_NEW_TOKENS;
constexpr int NBLK = ATSPEED_MAX_GAMMA + 1;

// What a user brings to the decoder it runs on: written by atspeed_decoder_set_node_mask / _set_adapter / _set_prefix, or handed over whole
// when a session admits the user (SessionJob::opts); UserOpts{} = nothing named, which is what a decoder holds once its user has left.
struct UserOpts {
  const atspeed_node_masks* masks = nullptr; int mask_user = 0;   // item filter: the user's blocked-node bits over the call's automaton
  int adapter = 0;        // the target's resident adapter slot, 0 = none: it rides in the user's segment of every target forward (the draft's keep 0)
  const atspeed_prefix *tprefix = nullptr, *dprefix = nullptr;    // prompt prefixes: the user's first round starts at base = their length, the arenas'
};                                                                // slots below that filled by the scatter launch in front of the first forward
}  // namespace

// One user: private KV caches for target and draft, device-side beam state, pinned mailbox and argument staging,
// plus the bookkeeping of the generate call in flight.  Forwards of several users are batched (SegTable).
struct atspeed_decoder {
  atspeed_llama *target, *draft;
  KvCache tkv, dkv;
  int max_prompt, tok_cap, W;
  char* arena;
  TokBuf tin[2], dround;
  BeamSet round_beams[2], blk[NBLK];
  Mailbox* mail_dev;
  Mailbox* mail_host;       // pinned
  int32_t* trace_host;      // pinned: per round [dl][MAXB] draft flat ids
  std::vector<int32_t> trace;   // rounds: {dl, n_matches, nb, flat ids...}
  // decision trace (atspeed_decoder_set_trace level 1): after every round the whole beam area (round beams, draft blocks) and the
  // verify walk's picks travel to the host; one record per round in `decisions` (format: include/atspeed_hip.h)
  int trace_level = 0;
  char* beam_area = nullptr; size_t beam_area_bytes = 0, bs_bytes = 0;
  int32_t* vtrace_dev = nullptr;
  char* dump_host = nullptr;    // pinned, beam_area_bytes (allocated on first use)
  std::vector<int32_t> decisions;
  // sampling mode (atspeed_decoder_set_sampling): off by default = the greedy path of every BASELINE config
  bool sample = false; float temperature = 1.f; uint32_t seed = 0;
  float* tab_score = nullptr;   // [ATSPEED_MAX_GAMMA][ATS_MAX_CAND] the draft's candidate scores per step (allocated on first use)
  int32_t* tab_off = nullptr;   // [ATSPEED_MAX_GAMMA][MAXB + 1]
  float* tab_lse = nullptr;     // [ATSPEED_MAX_GAMMA]
  // sampling-mode warpers (atspeed_decoder_set_warpers): off by default; `cutoff` holds one value per logits row of the step or round in flight
  int top_k = 0; float top_p = 1.f; int min_keep = 1;
  float* cutoff = nullptr;      // [MAXB + ATSPEED_MAX_GAMMA * MAXB] (allocated on first use)
  bool warps() const { return sample && (top_k > 0 || top_p < 1.f); }
  UserOpts opts;                // item filter, resident adapter and prompt prefixes of the user on this decoder
  // the automaton as this user's kernels take it by value: the shared arrays and the user's own blocked-node bits
  FsmDev fsm_dev(const atspeed_fsm* fsm) const { FsmDev f = fsm->dev; f.blocked = ats_mask_bits(opts.masks, opts.mask_user); return f; }
  struct Run : ats_round::User {                // n0, nb, base, k, dk, gen, reingest: the part round_plan.h's rules read and move on
    const atspeed_fsm* fsm; int gamma, max_new;
    int32_t* out_tokens; float* out_scores; atspeed_gen_stats* stats_out;
    atspeed_gen_stats s;
    int cur, dl;
    bool final_step, export_only, done;
  } run;
};

static size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

static void carve_tokbuf(char*& p, TokBuf& tb, int rows, int W) {
  tb.ids = (int32_t*)p;  p += align_up((size_t)rows * 4, 256);
  tb.pos = (int32_t*)p;  p += align_up((size_t)rows * 4, 256);
  tb.slot = (int32_t*)p; p += align_up((size_t)rows * 4, 256);
  tb.vis = (uint64_t*)p; p += align_up((size_t)rows * W * 8, 256);
}
static void carve_beams(char*& p, BeamSet& b) {
  b.score = (float*)p;    p += 256;
  b.node = (int32_t*)p;   p += 256;
  b.parent = (int32_t*)p; p += 256;
  b.tok = (int32_t*)p;    p += 256;
  b.flat = (int32_t*)p;   p += 256;
  b.seq = (int32_t*)p;    p += align_up((size_t)MAXB * LMAX * 4, 256);
}

extern "C" int atspeed_decoder_create(atspeed_llama* target, atspeed_llama* draft, int32_t max_prompt, atspeed_decoder** out) {
  ATS_REQUIRE(target && out && max_prompt >= 1, ATSPEED_ERR_INVALID, "decoder_create: bad arguments");
  if (draft) {
    ATS_REQUIRE(draft->cfg.vocab_size == target->cfg.vocab_size, ATSPEED_ERR_INVALID, "decoder_create: draft/target vocab differ");
    ATS_REQUIRE(draft->cfg.max_slots == target->cfg.max_slots, ATSPEED_ERR_INVALID, "decoder_create: draft/target max_slots differ");
  }
  Building<atspeed_decoder> d(new atspeed_decoder(), atspeed_decoder_destroy);
  d->target = target; d->draft = draft;
  ATS_TRY(kv_create(target, &d->tkv));
  if (draft) ATS_TRY(kv_create(draft, &d->dkv));
  d->max_prompt = max_prompt;
  d->W = target->vis_words;
  d->tok_cap = max_prompt + ATSPEED_MAX_GAMMA * MAXB + MAXB;
  size_t tb_bytes = 3 * align_up((size_t)d->tok_cap * 4, 256) + align_up((size_t)d->tok_cap * d->W * 8, 256);
  size_t bs_bytes = 5 * 256 + align_up((size_t)MAXB * LMAX * 4, 256);
  size_t vt_bytes = align_up((size_t)NBLK * 3 * MAXB * sizeof(int32_t), 256);
  size_t total = 3 * tb_bytes + (2 + NBLK) * bs_bytes + vt_bytes + 256;
  ATS_HIP(hipMalloc((void**)&d->arena, total));
  ATS_HIP(hipMemset(d->arena, 0, total));
  char* p = d->arena;
  carve_tokbuf(p, d->tin[0], d->tok_cap, d->W);
  carve_tokbuf(p, d->tin[1], d->tok_cap, d->W);
  carve_tokbuf(p, d->dround, d->tok_cap, d->W);
  d->beam_area = p; d->bs_bytes = bs_bytes; d->beam_area_bytes = (2 + NBLK) * bs_bytes + vt_bytes;
  carve_beams(p, d->round_beams[0]);
  carve_beams(p, d->round_beams[1]);
  for (int i = 0; i < NBLK; ++i) carve_beams(p, d->blk[i]);
  d->vtrace_dev = (int32_t*)p; p += vt_bytes;
  p += 256;
  // the mailbox is pinned host memory the kernels write directly (16 bytes per round over PCIe): the host reads it after the
  // round's stream synchronisation, no copy to enqueue per user
  ATS_HIP(hipHostMalloc((void**)&d->mail_host, sizeof(Mailbox), hipHostMallocMapped));
  ATS_HIP(hipHostGetDevicePointer((void**)&d->mail_dev, d->mail_host, 0));
  ATS_HIP(hipHostMalloc((void**)&d->trace_host, sizeof(int32_t) * ATSPEED_MAX_GAMMA * MAXB));
  d->run.done = true;
  *out = d.release();
  return ATSPEED_OK;
}

extern "C" void atspeed_decoder_destroy(atspeed_decoder* d) {
  if (!d) return;
  hipDeviceSynchronize();
  hipFree(d->tab_score); hipFree(d->tab_off); hipFree(d->tab_lse); hipFree(d->cutoff);
  kv_free(&d->tkv);
  kv_free(&d->dkv);
  hipFree(d->arena);
  if (d->mail_host) hipHostFree(d->mail_host);
  if (d->trace_host) hipHostFree(d->trace_host);
  if (d->dump_host) hipHostFree(d->dump_host);
  delete d;
}

extern "C" int atspeed_decoder_set_sampling(atspeed_decoder* d, int32_t do_sample, float temperature, uint32_t seed) {
  ATS_REQUIRE(d, ATSPEED_ERR_INVALID, "set_sampling: null decoder");
  ATS_REQUIRE(!do_sample || (temperature > 0.f && temperature == temperature), ATSPEED_ERR_INVALID, "set_sampling: temperature must be positive");
  d->sample = do_sample != 0; d->temperature = do_sample ? temperature : 1.f; d->seed = seed;
  if (d->sample && !d->tab_score) {
    g_ats_lazy_allocs++;
    ATS_HIP(hipMalloc((void**)&d->tab_score, sizeof(float) * ATSPEED_MAX_GAMMA * ATS_MAX_CAND));
    ATS_HIP(hipMalloc((void**)&d->tab_off, sizeof(int32_t) * ATSPEED_MAX_GAMMA * (MAXB + 1)));
    ATS_HIP(hipMalloc((void**)&d->tab_lse, sizeof(float) * ATSPEED_MAX_GAMMA));
  }
  return ATSPEED_OK;
}

extern "C" int atspeed_decoder_set_warpers(atspeed_decoder* d, int32_t top_k, float top_p, int32_t min_tokens_to_keep) {
  ATS_REQUIRE(d, ATSPEED_ERR_INVALID, "set_warpers: null decoder");
  ATS_REQUIRE(top_k >= 0 && top_p > 0.f && min_tokens_to_keep >= 1, ATSPEED_ERR_INVALID,
              "set_warpers: top_k %d must be >= 0 (0 = off), top_p %g in (0, 1] (>= 1 = off), min_tokens_to_keep %d >= 1", top_k, (double)top_p, min_tokens_to_keep);
  d->top_k = top_k; d->top_p = top_p < 1.f ? top_p : 1.f; d->min_keep = min_tokens_to_keep;
  if ((d->top_k > 0 || d->top_p < 1.f) && !d->cutoff) {
    g_ats_lazy_allocs++;
    ATS_HIP(hipMalloc((void**)&d->cutoff, sizeof(float) * (MAXB + ATSPEED_MAX_GAMMA * MAXB)));
  }
  return ATSPEED_OK;
}

extern "C" int atspeed_decoder_set_node_mask(atspeed_decoder* d, const atspeed_node_masks* masks, int32_t user) {
  ATS_REQUIRE(d, ATSPEED_ERR_INVALID, "set_node_mask: null decoder");
  ATS_REQUIRE(!masks || (user >= 0 && user < masks->n_users), ATSPEED_ERR_INVALID, "set_node_mask: user %d out of [0, %d)", user, masks ? masks->n_users : 0);
  d->opts.masks = masks; d->opts.mask_user = masks ? user : 0;
  return ATSPEED_OK;
}

extern "C" int atspeed_decoder_set_adapter(atspeed_decoder* d, int32_t slot) {
  ATS_REQUIRE(d, ATSPEED_ERR_INVALID, "set_adapter: null decoder");
  ATS_REQUIRE(slot >= 0 && slot <= ATSPEED_LORA_MAX_ADAPTERS, ATSPEED_ERR_INVALID, "set_adapter: slot %d out of [0, %d]", slot, ATSPEED_LORA_MAX_ADAPTERS);
  d->opts.adapter = slot;                          // whether the target holds it is looked up when a generate call starts
  return ATSPEED_OK;
}

// the decoder's private K / V arenas, copied to or from the caller's device buffers (tests fill them with a sentinel and read back which slots
// a call wrote)
extern "C" int64_t atspeed_decoder_kv_bytes(const atspeed_decoder* d, int32_t draft) {
  if (!d || (draft && !d->draft)) return -1;
  const atspeed_llama* m = draft ? d->draft : d->target;
  return (int64_t)m->cfg.n_layers * (int64_t)m->layer_kv_bytes;
}
extern "C" int atspeed_decoder_kv_copy(atspeed_decoder* d, int32_t draft, int32_t to_cache, void* k_dev, void* v_dev, void* stream) {
  ATS_REQUIRE(d && k_dev && v_dev, ATSPEED_ERR_INVALID, "decoder_kv_copy: null argument");
  ATS_REQUIRE(!draft || d->draft, ATSPEED_ERR_INVALID, "decoder_kv_copy: the decoder has no draft model");
  const KvCache& kv = draft ? d->dkv : d->tkv;
  const size_t bytes = (size_t)atspeed_decoder_kv_bytes(d, draft);
  hipStream_t st = (hipStream_t)stream;
  ATS_HIP(hipMemcpyAsync(to_cache ? kv.k : k_dev, to_cache ? k_dev : kv.k, bytes, hipMemcpyDeviceToDevice, st));
  ATS_HIP(hipMemcpyAsync(to_cache ? kv.v : v_dev, to_cache ? v_dev : kv.v, bytes, hipMemcpyDeviceToDevice, st));
  return ATSPEED_OK;
}

extern "C" int atspeed_decoder_set_trace(atspeed_decoder* d, int32_t level) {
  ATS_REQUIRE(d && (level == 0 || level == 1), ATSPEED_ERR_INVALID, "set_trace: level must be 0 or 1");
  if (level == 1 && !d->dump_host) ATS_HIP(hipHostMalloc((void**)&d->dump_host, d->beam_area_bytes));
  d->trace_level = level;
  return ATSPEED_OK;
}

extern "C" int64_t atspeed_decoder_decisions(atspeed_decoder* d, int32_t* out, int64_t cap_words) {
  if (!d) return 0;
  const int64_t n = (int64_t)d->decisions.size();
  if (out && cap_words > 0) memcpy(out, d->decisions.data(), sizeof(int32_t) * (size_t)std::min(n, cap_words));
  return n;
}

// one record of the decision trace from the host copy of the beam area: header {kind, nb, dl, nm, gen0, k, dk, n_blocks}, the blocks
// (beam-set images in arena order: score, node, parent, tok, flat [MAXB] each, seq [MAXB][LMAX]) and, for a verify round, the walk's picks
static void decisions_append(atspeed_decoder* d, int kind, int nb, int dl, int nm, int gen0, int k, int dk, const std::vector<int>& blocks) {
  std::vector<int32_t>& v = d->decisions;
  const int32_t hdr[8] = {kind, nb, dl, nm, gen0, k, dk, (int32_t)blocks.size()};
  v.insert(v.end(), hdr, hdr + 8);
  const size_t bw = d->bs_bytes / 4;
  for (int b : blocks) {
    const int32_t* src = (const int32_t*)(d->dump_host + (size_t)b * d->bs_bytes);
    v.insert(v.end(), src, src + bw);
  }
  if (kind == 0) {
    const int32_t* vt = (const int32_t*)(d->dump_host + (size_t)(2 + NBLK) * d->bs_bytes);
    v.insert(v.end(), vt, vt + (size_t)NBLK * 3 * MAXB);
  }
}

static TokBuf tb_offset(const TokBuf& t, int row, int W) {
  TokBuf o;
  o.ids = t.ids + row; o.pos = t.pos + row; o.slot = t.slot + row; o.vis = t.vis + (size_t)row * W;
  return o;
}

// the ranges of a call's sizes, under the name of the entry point that was given them: every generate call's (draft = false), and those a
// beam-SD call or a session adds
static int check_ranges(const char* who, int max_new, int k, bool draft = false, int dk = 0, int gamma = 0) {
  ATS_REQUIRE(max_new >= 1 && max_new <= LMAX, ATSPEED_ERR_CAPACITY, "%s: max_new_tokens %d out of [1,%d]", who, max_new, LMAX);
  ATS_REQUIRE(k >= 1 && k <= MAXB, ATSPEED_ERR_CAPACITY, "%s: beam size %d out of [1,%d]", who, k, MAXB);
  if (!draft) return ATSPEED_OK;
  ATS_REQUIRE(dk >= k && dk <= MAXB, ATSPEED_ERR_CAPACITY, "%s: draft beam size %d must be in [k=%d, %d]", who, dk, k, MAXB);
  ATS_REQUIRE(gamma >= 1 && gamma <= ATSPEED_MAX_GAMMA, ATSPEED_ERR_CAPACITY, "%s: gamma %d out of [1,%d]", who, gamma, ATSPEED_MAX_GAMMA);
  return ATSPEED_OK;
}
// decoder i of a call's list: it is there, runs the models of decoder 0 and stands in the list once.  draft: 0 = the target alone counts,
// 1 = the draft must be the same too, 2 = and there must be one
static int same_pair_once(const char* who, const char* rule, atspeed_decoder* const* decs, int i, int draft) {
  const atspeed_decoder *d = decs[i], *d0 = decs[0];
  ATS_REQUIRE(d && (draft < 2 || d->draft) && d->target == d0->target && (draft < 1 || d->draft == d0->draft), ATSPEED_ERR_INVALID, "%s: %s", who, rule);
  for (int j = 0; j < i; ++j) ATS_REQUIRE(decs[i] != decs[j], ATSPEED_ERR_INVALID, "%s: decoder %d used twice", who, i);
  return ATSPEED_OK;
}

static int check_common(atspeed_decoder* d, const int32_t* prompt, int P, const atspeed_fsm* fsm, int start_node,
                        int max_new, int k, const int32_t* out_tokens, const float* out_scores) {
  ATS_REQUIRE(d && prompt && fsm && out_tokens && out_scores, ATSPEED_ERR_INVALID, "generate: null argument");
  ATS_REQUIRE(P >= 1 && P <= d->max_prompt, ATSPEED_ERR_CAPACITY, "generate: prompt length %d exceeds max_prompt %d", P, d->max_prompt);
  ATS_TRY(check_ranges("generate", max_new, k));
  ATS_REQUIRE(fsm->dev.vocab == d->target->cfg.vocab_size, ATSPEED_ERR_INVALID, "generate: constraint vocab %d != model vocab %d",
              fsm->dev.vocab, d->target->cfg.vocab_size);
  ATS_REQUIRE(start_node >= 0 && start_node < std::max(fsm->dev.n_nodes, 1), ATSPEED_ERR_INVALID, "generate: start node out of range");
  ATS_REQUIRE(!(d->sample && fsm->dev.n_nodes == 0), ATSPEED_ERR_INVALID, "generate: sampling needs a constraint automaton (mask-free search is greedy only)");
  return ATSPEED_OK;             // the user's own options: user_opts_check, which every caller runs next
}

// a user that ends with NO valid beam (per-user ERR_FILTERED inside a lock-step batch): its result block must not keep whatever the caller's
// buffer held before (torch.empty hands back the previous batch's block): scores = -inf, tokens = 0, stream ordered
static int blank_outputs(int32_t* out_tokens, float* out_scores, int k, int max_new, hipStream_t st) {
  ATS_HIP(hipMemsetAsync(out_tokens, 0, (size_t)k * max_new * sizeof(int32_t), st));
  ATS_HIP(hipMemsetD32Async((hipDeviceptr_t)out_scores, (int)0xff800000u, (size_t)k, st));      // -inf
  return ATSPEED_OK;
}

static int mailbox_status(atspeed_decoder* d) {
  if (d->mail_host->status == ATSPEED_ERR_CONSTRAINT) {
    atspeed_set_error("`prefix_allowed_tokens_fn` returned an empty list for batch ID 0. This means that the constraint is unsatisfiable.");
    return ATSPEED_ERR_CONSTRAINT;
  }
  if (d->mail_host->status == ATSPEED_ERR_FILTERED) {
    atspeed_set_error("every beam of a step was dropped by the post-top-k id filter (tokens below %d other than %d, beamSD.py:80-86): "
                      "set the automaton's thresholds with atspeed_fsm_set_id_filter", d->run.fsm ? d->run.fsm->dev.filter_min : 32000,
                      d->run.fsm ? d->run.fsm->dev.filter_eos : 2);
    return ATSPEED_ERR_FILTERED;
  }
  if (d->mail_host->status != 0) {
    atspeed_set_error("decoder: device status %d (candidate capacity exceeded?)", d->mail_host->status);
    return d->mail_host->status;
  }
  return ATSPEED_OK;
}
// a user of a lock-step call that ends alone while the others go on, by what its mailbox holds: its prompt does not open with its prompt
// prefix (Mailbox::pad, found by prompt init) or it lost every beam of a step to the id filter (beamSD.py:80-86; the reference dies on a
// shape mismatch there).  ATSPEED_OK: neither.  The one-user calls return these as errors instead
static int ends_alone_status(const atspeed_decoder* d) {
  if (d->mail_host->pad) return ATSPEED_ERR_INVALID;
  return d->mail_host->status == ATSPEED_ERR_FILTERED ? ATSPEED_ERR_FILTERED : ATSPEED_OK;
}
// "this user ends here": its status and count of valid beams, its time, its stats record; blank: it leaves no beam (blank_outputs)
static int finish_user(atspeed_decoder* d, int status, int n_valid, bool blank, hipStream_t st) {
  atspeed_decoder::Run& r = d->run;
  r.s.n_valid = n_valid; r.s.status = status;
  if (blank) ATS_TRY(blank_outputs(r.out_tokens, r.out_scores, r.k, r.max_new, st));
  r.s.total_ms = r.s.draft_ms + r.s.target_ms + r.s.verify_ms;
  if (r.stats_out) *r.stats_out = r.s;
  r.done = true;
  return ATSPEED_OK;
}

// ---- a group of users decoded in lock step ----------------------------------------------------------------------
struct StageEvents { hipEvent_t ev[8]; bool init = false; };
static thread_local StageEvents g_ev_dev[ATS_MAX_DEVICES];    // stage-time events, per device
static int stage_events(hipEvent_t** out) {
  const int dev = ats_cur_device();
  ATS_REQUIRE(dev >= 0, ATSPEED_ERR_NO_DEVICE, "stage events: no current HIP device, or its id is >= %d", ATS_MAX_DEVICES);
  StageEvents& s = g_ev_dev[dev];
  if (!s.init) { g_ats_lazy_allocs++; for (auto& e : s.ev) ATS_HIP(hipEventCreate(&e)); s.init = true; }
  *out = s.ev;
  return ATSPEED_OK;
}

// several users' argument blocks through one launch of a multi kernel (one workgroup or grid column per block): the vector goes to the
// device through the staging ring, then launch(device array, count, stream)
template <typename A, typename F>
static int launch_staged(const std::vector<A>& args, F launch, hipStream_t st) {
  const void* dev = nullptr;
  ATS_TRY(ats_stage(args.data(), args.size() * sizeof(A), &dev, st));
  return launch((const A*)dev, (int)args.size(), st);
}

static Seg make_seg(const TokBuf& tb, int n_tok, int n_slots, int n_logit, const KvCache& kv, int adapter = 0) {
  Seg s{};
  s.ids = tb.ids; s.pos = tb.pos; s.slot = tb.slot; s.vis = tb.vis; s.kc = kv.k; s.vc = kv.v;
  s.n_tok = n_tok; s.n_slots = n_slots; s.n_logit = n_logit; s.adapter = adapter;
  return s;
}
// a span of a user's round (round_plan.h) as a segment: its rows of the user's token buffer tb
static Seg span_seg(const TokBuf& tb, int W, const ats_round::Span& sp, const KvCache& kv, int adapter = 0) {
  return make_seg(tb_offset(tb, sp.row0, W), sp.n_tok, sp.n_slots, sp.n_logit, kv, adapter);
}
int ats_seg_finish(SegTable& t, int qtile_rows) {
  t.total_tok = t.total_logit = t.n_qtiles = 0;
  int long_segs = 0;
  for (int i = 0; i < t.n; ++i) long_segs += t.seg[i].n_tok > 96 ? 1 : 0;
  // 128-row tiles (8 waves) halve the K/V re-reads of long segments; 256-row tiles (16 waves, kept in attn.hip) measured slower:
  // 393 vs ~210 us per launch at 64 users x 220 tokens
  t.qtile_rows = (2 * long_segs >= t.n) ? 128 : 64;
  // lock-step batches (thousands of workgroups) run the 32-rows-per-wave kernel: its 4-wave 128-row tile also wins on short segments
  // (the idle waves still carry a quarter of the tile's DMA): 249 vs 286 us at 256 users
  if (t.n >= 16) t.qtile_rows = 128;
  // (that was the 64-row tile behind a double buffer).  Where every segment fits a 64-row tile (a round's 20-row inputs, a phase's 40-row
  // block) the batch takes 64-row tiles all the same: their 32-rows-per-wave launch is single-buffered now, four workgroups per CU instead
  // of two -- 150 vs 191 us at 256 users x 20 rows, 201 vs 241 us at 40 rows (profiles/attn_short_ab.txt)
  int max_tok = 0;
  for (int i = 0; i < t.n; ++i) max_tok = std::max(max_tok, t.seg[i].n_tok);
  if (t.n >= 16 && max_tok <= 64 && ats_switch(ATS_SW_ATTN_SHORT)) t.qtile_rows = 64;
  if (qtile_rows) t.qtile_rows = qtile_rows;
  for (int i = 0; i < t.n; ++i) {
    t.seg[i].row0 = t.total_tok; t.total_tok += t.seg[i].n_tok;
    t.seg[i].logit_row0 = t.total_logit; t.total_logit += t.seg[i].n_logit;
    for (int j = 0; j * t.qtile_rows < t.seg[i].n_tok; ++j) {
      ATS_REQUIRE(t.n_qtiles < ATS_MAX_QTILES, ATSPEED_ERR_CAPACITY, "forward: too many query tiles in one batch");
      t.qtile_seg[t.n_qtiles] = (unsigned char)i; t.qtile_idx[t.n_qtiles++] = (unsigned char)j;
    }
  }
  return ATSPEED_OK;
}

// ---- prompt prefixes (include/atspeed_hip.h "prompt prefixes"): the K / V rows of a shared prompt opening, kept compact per model
struct atspeed_prefix {
  atspeed_llama* m = nullptr;
  int len = 0, slot = 0;                       // tokens; the resident adapter slot the rows were made under (0 = none)
  void *k = nullptr, *v = nullptr;             // [layers][len][hidden] in the model's type
  int32_t* ids = nullptr;                      // [len]
  int scheme = SCHEME_16; long lora_gen = 0, slot_gen = 0;     // the arithmetic that produced the rows (prefix_stale)
  mutable int64_t users_served = 0;
  size_t bytes = 0;
};
static bool prefix_stale(const atspeed_prefix* p) {
  const atspeed_llama* m = p->m;
  return p->scheme != m->scheme || p->lora_gen != m->lora_gen || (p->slot && p->slot_gen != m->slot_gen[p->slot]);
}

extern "C" void atspeed_prefix_destroy(atspeed_prefix* p) {
  if (!p) return;
  hipFree(p->k); hipFree(p->v); hipFree(p->ids);
  delete p;
}

static int kv_rows_launch(void* store_k, void* store_v, const std::vector<KvRowsUser>& users, int len, const atspeed_llama* m, int to_store, hipStream_t st) {
  return launch_staged(users, [&](const KvRowsUser* du, int n, hipStream_t s) {
    return ats_bf16::ats_kv_rows_copy(store_k, store_v, du, n, len, m->cfg.n_layers, m->cfg.hidden * m->esz, m->cfg.max_slots, to_store, s); }, st);
}

extern "C" int atspeed_prefix_create(atspeed_llama* m, const int32_t* ids, int32_t len, int32_t adapter_slot, void* stream, atspeed_prefix** out) {
  ATS_REQUIRE(m && ids && out, ATSPEED_ERR_INVALID, "prefix_create: null argument");
  ATS_REQUIRE(len >= 1 && len < m->cfg.max_slots, ATSPEED_ERR_INVALID, "prefix_create: %d tokens (1 .. max_slots - 1 = %d)", len, m->cfg.max_slots - 1);
  ATS_REQUIRE(adapter_slot >= 0 && m->slot_ok(adapter_slot), ATSPEED_ERR_INVALID, "prefix_create: adapter slot %d is not occupied", adapter_slot);
  hipStream_t st = (hipStream_t)stream;
  Building<atspeed_prefix> p(new atspeed_prefix(), atspeed_prefix_destroy);
  p->m = m; p->len = len; p->slot = adapter_slot;
  p->scheme = m->scheme; p->lora_gen = m->lora_gen; p->slot_gen = m->slot_gen[adapter_slot];
  const size_t store = (size_t)m->cfg.n_layers * len * m->cfg.hidden * m->esz;
  ATS_HIP(hipMalloc(&p->k, store));
  ATS_HIP(hipMalloc(&p->v, store));
  ATS_HIP(hipMalloc((void**)&p->ids, (size_t)len * sizeof(int32_t)));
  p->bytes = 2 * store + (size_t)len * sizeof(int32_t);
  // scratch of this call: an arena in the engine's layout for the forward to write, the forward's token rows, and what prompt init writes besides
  KvCache kv;
  char* scr = nullptr;
  const int W = m->vis_words;
  const size_t tb_bytes = 3 * align_up((size_t)len * 4, 256) + align_up((size_t)len * W * 8, 256);
  auto run = [&]() -> int {
    ATS_TRY(kv_create(m, &kv));
    ATS_HIP(hipMalloc((void**)&scr, tb_bytes + 6 * 256));
    char* q = scr;
    TokBuf tb; carve_tokbuf(q, tb, len, W);
    BeamSet bs{}; bs.score = (float*)q; bs.node = (int32_t*)(q + 256); bs.parent = (int32_t*)(q + 512); bs.tok = (int32_t*)(q + 768); bs.flat = (int32_t*)(q + 1024);
    ATS_TRY(ats_init_prompt(tb, ids, len, W, bs, 0, m->cfg.vocab_size, (Mailbox*)(q + 1280), st));
    ATS_TRY(ensure_act(m, len, 1));
    SegTable t{};
    t.seg[t.n++] = make_seg(tb, len, len, 1, kv, adapter_slot);
    ATS_TRY(ats_seg_finish(t));
    ATS_TRY(llama_forward_segs(m, t, nullptr, st));
    ATS_TRY(kv_rows_launch(p->k, p->v, std::vector<KvRowsUser>{KvRowsUser{kv.k, kv.v}}, len, m, 1, st));
    ATS_HIP(hipMemcpyAsync(p->ids, ids, (size_t)len * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
    return ATSPEED_OK;
  };
  const int rc = run();
  const hipError_t e = hipStreamSynchronize(st);       // on failure too: what was launched writes the scratch
  ats_stage_reset();
  kv_free(&kv); hipFree(scr);
  ATS_TRY(rc);
  ATS_HIP(e);
  *out = p.release();
  return ATSPEED_OK;
}

extern "C" int atspeed_prefix_info(const atspeed_prefix* p, int32_t* len, int64_t* users_served, int64_t* bytes) {
  ATS_REQUIRE(p, ATSPEED_ERR_INVALID, "prefix_info: null prefix");
  if (len) *len = p->len;
  if (users_served) *users_served = p->users_served;
  if (bytes) *bytes = (int64_t)p->bytes;
  return prefix_stale(p) ? 1 : 0;
}

extern "C" int atspeed_prefix_read(const atspeed_prefix* p, void* k_dst, void* v_dst, int32_t* ids_dst, void* stream) {
  ATS_REQUIRE(p, ATSPEED_ERR_INVALID, "prefix_read: null prefix");
  const size_t store = (p->bytes - (size_t)p->len * sizeof(int32_t)) / 2;
  if (k_dst) ATS_HIP(hipMemcpyAsync(k_dst, p->k, store, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  if (v_dst) ATS_HIP(hipMemcpyAsync(v_dst, p->v, store, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  if (ids_dst) ATS_HIP(hipMemcpyAsync(ids_dst, p->ids, (size_t)p->len * sizeof(int32_t), hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return ATSPEED_OK;
}

// the copy kernel alone (tests): the caller's arenas, staged as the engine stages its users'
static int kv_rows_abi(const char* who, void* store_k, void* store_v, void* const* k_arenas, void* const* v_arenas, int n, int len, int layers, int row_bytes,
                       int max_slots, int to_store, hipStream_t st) {
  ATS_REQUIRE(store_k && store_v && k_arenas && v_arenas, ATSPEED_ERR_INVALID, "%s: null argument", who);
  ATS_REQUIRE(n >= 1 && n <= ATS_MAX_SEGS, ATSPEED_ERR_CAPACITY, "%s: %d arenas per call (max %d)", who, n, ATS_MAX_SEGS);
  std::vector<KvRowsUser> users(n);
  for (int i = 0; i < n; ++i) {
    ATS_REQUIRE(k_arenas[i] && v_arenas[i] && (((uintptr_t)k_arenas[i] | (uintptr_t)v_arenas[i]) & 15) == 0, ATSPEED_ERR_INVALID,
                "%s: arena %d is null or not 16-byte aligned", who, i);
    users[i] = KvRowsUser{k_arenas[i], v_arenas[i]};
  }
  return launch_staged(users, [&](const KvRowsUser* du, int m, hipStream_t s) {
    return ats_bf16::ats_kv_rows_copy(store_k, store_v, du, m, len, layers, row_bytes, max_slots, to_store, s); }, st);
}
extern "C" int atspeed_kv_rows_scatter(const void* store_k, const void* store_v, void* const* k_arenas, void* const* v_arenas, int32_t n, int32_t len,
                                       int32_t layers, int32_t row_bytes, int32_t max_slots, void* stream) {
  return kv_rows_abi("kv_rows_scatter", (void*)store_k, (void*)store_v, k_arenas, v_arenas, n, len, layers, row_bytes, max_slots, 0, (hipStream_t)stream);
}
extern "C" int atspeed_kv_rows_gather(void* store_k, void* store_v, const void* k_arena, const void* v_arena, int32_t len, int32_t layers,
                                      int32_t row_bytes, int32_t max_slots, void* stream) {
  void* ka = (void*)k_arena; void* va = (void*)v_arena;
  return kv_rows_abi("kv_rows_gather", store_k, store_v, &ka, &va, 1, len, layers, row_bytes, max_slots, 1, (hipStream_t)stream);
}

extern "C" int atspeed_prefix_to_batch_arenas(const atspeed_prefix* p, int32_t first, int32_t n, void* stream) {
  ATS_REQUIRE(p, ATSPEED_ERR_INVALID, "prefix_to_batch_arenas: null prefix");
  ATS_REQUIRE(first >= 0 && n >= 1 && first + n <= ATS_MAX_SEGS, ATSPEED_ERR_CAPACITY, "prefix_to_batch_arenas: arenas [%d, %d) of at most %d", first, first + n, ATS_MAX_SEGS);
  ATS_REQUIRE(!prefix_stale(p), ATSPEED_ERR_INVALID, "prefix_to_batch_arenas: the prompt prefix is stale: its model's quantisation or adapter changed after it was built");
  atspeed_llama* m = p->m;
  while ((int)m->kv_pool.size() < first + n) {
    KvCache kv;
    ATS_TRY(kv_create(m, &kv));
    m->kv_pool.push_back(kv);
  }
  std::vector<KvRowsUser> users;
  for (int i = first; i < first + n; ++i) users.push_back(KvRowsUser{m->kv_pool[i].k, m->kv_pool[i].v});
  ATS_TRY(kv_rows_launch(p->k, p->v, users, p->len, m, 0, (hipStream_t)stream));
  p->users_served += n;
  return ATSPEED_OK;
}

extern "C" int atspeed_decoder_set_prefix(atspeed_decoder* d, const atspeed_prefix* tp, const atspeed_prefix* dp) {
  ATS_REQUIRE(d, ATSPEED_ERR_INVALID, "set_prefix: null decoder");
  ATS_REQUIRE(!tp || tp->m == d->target, ATSPEED_ERR_INVALID, "set_prefix: the target prefix was built on another model");
  ATS_REQUIRE(!dp || (d->draft && dp->m == d->draft), ATSPEED_ERR_INVALID, "set_prefix: the draft prefix was built on another model");
  d->opts.tprefix = tp; d->opts.dprefix = dp;
  return ATSPEED_OK;
}

// what a generate call or a session's submit asks of a user's options before anything is launched or queued: the filter lives on the call's
// automaton, the target holds the adapter slot, and the prefixes fit models, adapter and prompt.  bssd: a beam-SD call or a session (draft
// and target share one token buffer, so both models start at the same offset), else target_generate (the target's prefix alone counts)
static int user_opts_check(const char* who, const atspeed_llama* T, const atspeed_llama* D, const atspeed_fsm* fsm, const UserOpts& o, int P, bool bssd) {
  ATS_REQUIRE(!o.masks || o.masks->fsm == fsm, ATSPEED_ERR_INVALID, "%s: the user's item filter was built on another automaton", who);
  ATS_REQUIRE(T->slot_ok(o.adapter), ATSPEED_ERR_INVALID, "%s: the user names adapter slot %d, which the target does not hold", who, o.adapter);
  const atspeed_prefix *tp = o.tprefix, *dp = bssd ? o.dprefix : nullptr;
  if (!tp && !dp) return ATSPEED_OK;
  ATS_REQUIRE(!bssd || (tp && dp), ATSPEED_ERR_INVALID, "%s: a beam-SD user needs the prefix of both models or of neither (the %s one is missing)", who,
              tp ? "draft's" : "target's");
  ATS_REQUIRE(tp, ATSPEED_ERR_INVALID, "%s: no target prefix", who);
  ATS_REQUIRE(tp->m == T && (!dp || dp->m == D), ATSPEED_ERR_INVALID, "%s: the prompt prefix was built on another model", who);
  ATS_REQUIRE(!prefix_stale(tp) && (!dp || !prefix_stale(dp)), ATSPEED_ERR_INVALID,
              "%s: the prompt prefix is stale: its model's quantisation or adapter changed after it was built (build a new one)", who);
  ATS_REQUIRE(tp->slot == o.adapter, ATSPEED_ERR_INVALID, "%s: the prompt prefix was built under adapter slot %d, the user runs under slot %d", who, tp->slot, o.adapter);
  ATS_REQUIRE(!dp || dp->slot == 0, ATSPEED_ERR_INVALID, "%s: the draft is never adapted, its prefix names slot %d", who, dp ? dp->slot : 0);
  ATS_REQUIRE(!dp || dp->len == tp->len, ATSPEED_ERR_INVALID, "%s: target and draft prefixes hold %d and %d tokens", who, tp->len, dp ? dp->len : 0);
  ATS_REQUIRE(tp->len <= P - 1, ATSPEED_ERR_INVALID, "%s: a prefix of %d tokens needs a prompt of at least %d (one suffix row gives the first logit row), got %d",
              who, tp->len, tp->len + 1, P);
  return ATSPEED_OK;
}
static int prefix_len(const atspeed_decoder* d) { return d->opts.tprefix ? d->opts.tprefix->len : 0; }

// the users' prefix rows into their arenas, in front of their first forward: per model one launch for all users that name the same prefix
// (draft: the draft model's side too).  No user with a prefix: nothing is staged or launched
static int prefixes_scatter(atspeed_decoder* const* decs, int n, bool draft_too, hipStream_t st) {
  for (int side = 0; side < (draft_too ? 2 : 1); ++side) {
    std::map<const atspeed_prefix*, std::vector<KvRowsUser>> by;
    for (int u = 0; u < n; ++u) {
      const atspeed_prefix* p = side ? decs[u]->opts.dprefix : decs[u]->opts.tprefix;
      if (p && decs[u]->opts.tprefix) by[p].push_back(side ? KvRowsUser{decs[u]->dkv.k, decs[u]->dkv.v} : KvRowsUser{decs[u]->tkv.k, decs[u]->tkv.v});
    }
    for (auto& e : by) {
      ATS_TRY(kv_rows_launch(e.first->k, e.first->v, e.second, e.first->len, e.first->m, 0, st));
      e.first->users_served += (int64_t)e.second.size();
    }
  }
  return ATSPEED_OK;
}
static int prefix_mismatch_error(const atspeed_decoder* d) {
  atspeed_set_error("generate: the prompt does not open with the %d tokens of its prompt prefix", prefix_len(d));
  return ATSPEED_ERR_INVALID;
}

// ---- one decode step: forward, then every user's beam step on its rows of the result
// where a segment's logit rows, their normalisers and their candidate lists start in the model's buffers
struct RowViews { const float* logits; const float* lse; const int32_t* row_cand; };
static RowViews seg_rows(const atspeed_llama* m, const Seg& sg) {
  const ActCtx* cx = m->act;
  const size_t r0 = (size_t)sg.logit_row0;
  return RowViews{cx->logits + r0 * m->logits_ld, cx->lse + r0, cx->row_cand + r0 * MAXB};
}

// the forward of a decode step: only the logit tiles the automaton can read are written; a mask-free search takes its candidates from
// the kk best tokens of every row instead
// row_off: the step's logit rows, normalisers and candidate lists start at that row of the model's buffers (staged verification's phases)
static int decode_forward(atspeed_llama* m, const SegTable& t, const atspeed_fsm* fsm, int kk, hipStream_t st, int row_off = 0) {
  ATS_TRY(llama_forward_segs(m, t, nullptr, st, fsm->d_tile_store, row_off));
  if (fsm->dev.n_nodes == 0)
    ATS_TRY(ats_row_topk(m->act->logits + (size_t)row_off * m->logits_ld, t.total_logit, m->cfg.vocab_size, m->logits_ld, kk,
                         m->act->row_cand + (size_t)row_off * MAXB, st));
  return ATSPEED_OK;
}

// what every beam step shares: user d expands the sg.n_logit beams of `src`, scored by model m's logit rows of segment sg, into the k best
// of `dst`.  The caller adds what differs: emit with the in / out token rows, the tab_* tables and, when a.sample is set, rng_sub.
static BeamStepArgs beam_step_args(const atspeed_decoder* d, const atspeed_llama* m, const Seg& sg, const atspeed_fsm* fsm, const BeamSet& src,
                                   const BeamSet& dst, int gen_len, int k) {
  const RowViews rv = seg_rows(m, sg);
  BeamStepArgs a{};
  a.src = src; a.n_src = sg.n_logit; a.gen_len = gen_len; a.dst = dst; a.k = k;
  a.logits = rv.logits; a.ld = m->logits_ld; a.lse = rv.lse; a.row_cand = rv.row_cand; a.n_row_cand = k;
  a.fsm = d->fsm_dev(fsm); a.filter_ids = fsm->dev.n_nodes == 0 ? 0 : 1;
  a.mail = d->mail_dev; a.vis_words = d->W;
  if (d->sample) { a.sample = 1; a.temperature = d->temperature; }
  if (d->warps()) a.cutoff = d->cutoff;
  return a;
}
// the per-round part of user d's verify walk on target T: beams, sizes, token buffers, outputs, sampling tables.  The round's phases add
// where the rows are (logits / lse / row_cand, blk_row0) and how many blocks have rows (blocks_ready)
static VerifyArgs verify_args(const atspeed_decoder* d, const atspeed_llama* T) {
  const atspeed_decoder::Run& r = d->run;
  VerifyArgs va{};
  va.blk[0] = d->round_beams[r.cur];
  for (int b = 1; b <= r.dl; ++b) va.blk[b] = d->blk[b];
  va.nb = r.nb; va.dl = r.dl; va.k = r.k; va.dk = r.dk; va.gen_len0 = r.gen;
  va.ld = T->logits_ld; va.fsm = d->fsm_dev(r.fsm); va.n_row_cand = r.k;
  va.cur = d->tin[r.cur]; va.n0 = r.n0; va.next = d->tin[r.cur ^ 1]; va.dnext = d->dround; va.vis_words = d->W;
  va.res = d->round_beams[r.cur ^ 1]; va.mail = d->mail_dev;
  va.vtrace = (d->trace_level >= 1 && !d->sample) ? d->vtrace_dev : nullptr;
  if (d->sample) {
    va.sample = 1; va.temperature = d->temperature; va.seed = d->seed; va.round = r.s.n_run;
    for (int b = 0; b < r.dl; ++b) {
      va.dtab_score[b] = d->tab_score + (size_t)b * ATS_MAX_CAND; va.dtab_off[b] = d->tab_off + (size_t)b * (MAXB + 1);
      va.dtab_lse[b] = d->tab_lse + b;
    }
  }
  if (d->warps()) va.cutoff = d->cutoff;
  return va;
}
// sampling-mode warpers: the cutoff job in front of a sampled beam step (one segment: the step's source beams) ...
static WarpCutArgs warp_cut_args(const atspeed_decoder* d, const BeamStepArgs& s) {
  WarpCutArgs w{};
  w.seg[0] = WarpSeg{s.src.node, s.n_src}; w.n_seg = 1;
  w.logits = s.logits; w.ld = s.ld; w.lse = s.lse; w.fsm = s.fsm;
  w.temperature = d->temperature; w.top_k = d->top_k; w.top_p = d->top_p; w.min_keep = d->min_keep; w.cutoff = d->cutoff;
  return w;
}
// ... and in front of a sampled verify walk (the round beams' rows, then every draft block's)
static WarpCutArgs warp_cut_args(const atspeed_decoder* d, const VerifyArgs& v) {
  WarpCutArgs w{};
  w.seg[0] = WarpSeg{v.blk[0].node, v.nb};
  for (int i = 1; i <= v.dl; ++i) w.seg[i] = WarpSeg{v.blk[i].node, v.dk};
  w.n_seg = v.dl + 1;
  w.logits = v.logits; w.ld = v.ld; w.lse = v.lse; w.fsm = v.fsm;
  w.temperature = d->temperature; w.top_k = d->top_k; w.top_p = d->top_p; w.min_keep = d->min_keep; w.cutoff = d->cutoff;
  return w;
}
// one job by value, several through one staged launch; no job (greedy, or both warpers off): no launch
static int warp_cutoffs(const std::vector<WarpCutArgs>& w, hipStream_t st) {
  if (w.empty()) return ATSPEED_OK;
  if (w.size() == 1) return ats_row_warp_cutoff(w[0], st);
  int max_rows = 0;
  for (const WarpCutArgs& a : w) { int rows = 0; for (int s = 0; s < a.n_seg; ++s) rows += a.seg[s].n; max_rows = std::max(max_rows, rows); }
  return launch_staged(w, [&](const WarpCutArgs* dw, int n, hipStream_t s) { return ats_row_warp_cutoff_multi(dw, n, max_rows, s); }, st);
}
// the step also writes the next forward's inputs: the parents' rows start at in_row0 of tb, the k new rows go to out_row0 (KV slots from out_slot0)
static void beam_step_emit(BeamStepArgs& a, const TokBuf& tb, int in_row0, int out_row0, int out_slot0) {
  a.emit = 1; a.in = tb; a.in_row0 = in_row0; a.out = tb; a.out_row0 = out_row0; a.out_slot0 = out_slot0;
}

// out_tokens / out_scores of the users that finish: one user by value, several through one staged launch
static int export_beams(const std::vector<ExportBeamsArgs>& ex, int k, int max_new, hipStream_t st) {
  if (ex.size() == 1) return ats_export_beams(ex[0].b, k, max_new, ex[0].out_tokens, ex[0].out_scores, st, ex[0].sort_desc != 0);
  return launch_staged(ex, [&](const ExportBeamsArgs* de, int n, hipStream_t s) { return ats_export_beams_multi(de, n, k, max_new, s); }, st);
}

// what stands in front of a user's first forward.  One user: the prompt -> token buffer, start beams and mailbox, by value; then the rows of
// its prompt prefixes into its arenas (draft_too: the draft's as well)
static int start_user(atspeed_decoder* d, const int32_t* prompt, int P, int start_node, bool draft_too, hipStream_t st) {
  ATS_TRY(ats_init_prompt(d->tin[0], prompt, P, d->W, d->round_beams[0], start_node, d->target->cfg.vocab_size, d->mail_dev, st, prefix_len(d),
                          d->opts.tprefix ? d->opts.tprefix->ids : nullptr));
  return prefixes_scatter(&d, 1, draft_too, st);
}
// ... and every user of a batch, or every user a session admits in a round: one prompt launch for all of them, then the prefixes
static int start_users(atspeed_decoder** decs, int n, const int32_t* const* prompts, const int32_t* prompt_lens, const int32_t* start_nodes,
                       bool draft_too, hipStream_t st) {
  std::vector<InitPromptArgs> ia(n);
  int max_p = 1;
  for (int u = 0; u < n; ++u) {
    atspeed_decoder* d = decs[u];
    ia[u] = InitPromptArgs{d->tin[0], prompts[u], prompt_lens[u], start_nodes[u], d->round_beams[0], d->mail_dev, prefix_len(d),
                           d->opts.tprefix ? d->opts.tprefix->ids : nullptr};
    max_p = std::max(max_p, (int)prompt_lens[u]);
  }
  ATS_TRY(launch_staged(ia, [&](const InitPromptArgs* dev, int m, hipStream_t s) {
    return ats_init_prompt_multi(dev, m, max_p, decs[0]->W, decs[0]->target->cfg.vocab_size, s); }, st));
  return prefixes_scatter(decs, n, draft_too, st);
}

static int bssd_begin(atspeed_decoder* d, const int32_t* prompt, int P, const atspeed_fsm* fsm, int start_node, int gamma,
                      int max_new, int k, int dk, int32_t* out_tokens, float* out_scores, atspeed_gen_stats* stats,
                      hipStream_t st, bool init_prompt = true) {
  ATS_TRY(check_common(d, prompt, P, fsm, start_node, max_new, k, out_tokens, out_scores));
  ATS_REQUIRE(d->draft, ATSPEED_ERR_INVALID, "bssd: decoder was created without a draft model");
  ATS_TRY(check_ranges("bssd", max_new, k, true, dk, gamma));           // (max_new and k have passed check_common)
  ATS_TRY(user_opts_check("bssd", d->target, d->draft, fsm, d->opts, P, true));
  const int lp = prefix_len(d);                    // the first round starts behind the prefix: what every later round looks like
  atspeed_decoder::Run& r = d->run;
  r.fsm = fsm; r.gamma = gamma; r.max_new = max_new; r.k = k; r.dk = dk;
  r.out_tokens = out_tokens; r.out_scores = out_scores; r.stats_out = stats;
  memset(&r.s, 0, sizeof(r.s));
  r.cur = 0; r.gen = 0; r.base = lp; r.n0 = P - lp; r.nb = 1; r.dl = 0;
  r.reingest = false; r.final_step = false; r.export_only = false; r.done = false;
  d->trace.clear();
  d->decisions.clear();
  if (init_prompt) ATS_TRY(start_user(d, prompt, P, start_node, true, st));
  return ATSPEED_OK;
}

// activation capacity of both models for the worst round of these users (round_plan.h; n0: each user's longest round inputs)
static int bssd_ensure_capacity(atspeed_llama* T, atspeed_llama* D, const std::vector<int>& n0, int gamma, int k, int dk) {
  const ats_round::Capacity c = ats_round::worst_round(n0.data(), (int)n0.size(), gamma, k, dk, MAXB);
  ATS_TRY(ensure_act(T, c.t_tok, c.t_rows));
  return ensure_act(D, c.d_tok, c.d_rows);
}

// what differs between the callers of a round, and what a round reports back
struct RoundCtl {
  bool flat_trace;          // copy the draft's flat ids to the per-round trace (atspeed_decoder_trace; groups of up to 4 users)
  bool keep_filtered;       // a user that loses every beam to the id filter ends alone with ATSPEED_ERR_FILTERED; else the round returns the error
  bool lock_step;           // the batch call or a session: the round may verify in stages (the one-user call never does)
  bool any = false;         // out: a user of the group is not done yet
  int target_forwards = 0, draft_forwards = 0;   // out: forwards this round launched (a staged round's phases are one target forward ...
  int target_passes = 0;                         // ... and one pass over the target's weights each)
};

// Staged verification: does this round verify block by block?  Greedy users on a plain 16-bit or fp32 target only: a sampled round's
// draws keep their order in the packed forward, and W8A8 / W4A8 / LoRA targets stay packed (their kernels are chosen by the forward's token count;
// not measured here).  Switch "verify_staged": 0 never, 2 always, 1 (auto) when both hold:
//   - the packed forward would exceed "verify_staged_tokens" tokens (T*);
//   - by the target's recent walks (stg_needed / stg_drafted: block j is needed with probability Q_j; no history: never) the rows the round
//     expects to skip, sum over users and blocks of (1 - Q_j) x DK, exceed "verify_staged_pass_tokens" per phase it expects to add (the
//     blocks j that at least half a user is expected to need).  Where every block is accepted nothing can be skipped and the round stays
//     packed; where the walks stop at step 0 no phase is added and every round above T* is staged.
static bool bssd_round_staged(const std::vector<atspeed_decoder*>& ver, const std::vector<atspeed_decoder*>& fin) {
  const int mode = ats_switch(ATS_SW_VERIFY_STAGED);
  if (mode <= 0 || ver.empty()) return false;
  const atspeed_llama* T = ver[0]->target;
  if (!T->plain16()) return false;
  long long tok = 0;
  for (const atspeed_decoder* d : ver) { if (d->sample) return false; tok += d->run.n0 + d->run.dl * d->run.dk; }
  for (const atspeed_decoder* d : fin) { if (d->sample) return false; tok += d->run.n0; }
  if (mode >= 2) return true;
  if (tok <= ats_switch(ATS_SW_VERIFY_STAGED_TOKENS)) return false;
  const int pass_tok = ats_switch(ATS_SW_VERIFY_STAGED_PASS_TOKENS);
  if (pass_tok <= 0) return true;
  double skipped = 0., users_at[ATSPEED_MAX_GAMMA + 1] = {};
  for (const atspeed_decoder* d : ver)
    for (int j = 1; j <= d->run.dl; ++j) {
      const double q = T->stg_drafted[j] >= 1. ? T->stg_needed[j] / T->stg_drafted[j] : 0.;
      skipped += (1. - q) * d->run.dk;
      users_at[j] += q;
    }
  int extra = 0;
  for (int j = 1; j <= ATSPEED_MAX_GAMMA; ++j) extra += users_at[j] >= 0.5 ? 1 : 0;
  return skipped > (double)extra * pass_tok;
}

// ONE round of BSSD (beamSD.py:458-542) over the n decoders handed to it (users that are done are skipped): every draft step and the target
// verification of the round is ONE forward over the tokens of all users that need it (weights are streamed once per forward, not per user),
// then verify and final steps, the exports of the users that finish, the round's single synchronisation and the per-user bookkeeping.
// The activation buffers must hold the round (bssd_ensure_capacity).
static int bssd_round(atspeed_decoder** decs, int n, hipStream_t st, hipEvent_t* g_ev, RoundCtl& ctl) {
  atspeed_llama *T = decs[0]->target, *D = decs[0]->draft;
  const int W = decs[0]->W;
  std::vector<atspeed_decoder*> ver, fin;          // users doing a verify round / the final single step this round
  int max_dl = 0;
  for (int u = 0; u < n; ++u) {
    atspeed_decoder* d = decs[u];
    atspeed_decoder::Run& r = d->run;
    if (r.done) continue;
    // (a slot removed under a user that is in a lane: the caller's error, found here before the round launches anything)
    ATS_REQUIRE(T->slot_ok(d->opts.adapter), ATSPEED_ERR_INVALID, "bssd: a user names adapter slot %d, which the target no longer holds", d->opts.adapter);
    const ats_round::Start start = ats_round::classify(r.gen, r.max_new, r.gamma);  // beamSD.py:504-509
    r.final_step = start.kind != ats_round::VERIFY; r.export_only = start.kind == ats_round::EXPORT_ONLY;
    if (r.export_only) continue;
    r.dl = start.dl;
    if (r.final_step) { fin.push_back(d); continue; }
    const ats_round::Span all = ats_round::span(r, 0, r.dl);                        // the round's reach, whether it is forwarded at once or in phases
    ATS_REQUIRE(all.n_tok <= d->tok_cap, ATSPEED_ERR_CAPACITY, "bssd: packed target input too long");
    ATS_REQUIRE(all.n_slots <= T->cfg.max_slots, ATSPEED_ERR_CAPACITY, "bssd: KV slots exhausted (%d needed, %d available)", all.n_slots, T->cfg.max_slots);
    ver.push_back(d);
    max_dl = std::max(max_dl, r.dl);
  }
  hipEventRecord(g_ev[0], st);
  // ---- 1. draft: step i of one_step_beam_search for every user that still drafts (:108-179)
  for (int i = 0; i < max_dl; ++i) {
    SegTable t{};
    std::vector<BeamStepArgs> args;
    std::vector<WarpCutArgs> wargs;
    std::vector<atspeed_decoder*> us;
    for (atspeed_decoder* d : ver) if (d->run.dl > i) us.push_back(d);
    for (atspeed_decoder* d : us) {
      atspeed_decoder::Run& r = d->run;
      const ats_round::Span sp = ats_round::span(r, i, i);     // step 0 reads the round inputs, step i the block step i - 1 wrote
      t.seg[t.n++] = (i == 0 && r.reingest) ? span_seg(d->dround, W, ats_round::reingest_span(r), d->dkv) : span_seg(d->tin[r.cur], W, sp, d->dkv);
      r.s.n_draft_forwards++;
    }
    ATS_TRY(ats_seg_finish(t));
    ATS_TRY(decode_forward(D, t, decs[0]->run.fsm, decs[0]->run.dk, st));
    ctl.draft_forwards++;
    for (size_t j = 0; j < us.size(); ++j) {
      atspeed_decoder* d = us[j];
      atspeed_decoder::Run& r = d->run;
      BeamStepArgs a = beam_step_args(d, D, t.seg[j], r.fsm, i == 0 ? d->round_beams[r.cur] : d->blk[i], d->blk[i + 1], r.gen + i, r.dk);
      beam_step_emit(a, d->tin[r.cur], ats_round::beam_row0(r, i), ats_round::span(r, i + 1, i + 1).row0, ats_round::span(r, i, i).n_slots);
      if (a.sample) {
        a.rng_sub = ats_rng_sub(d->seed, ATS_RNG_STEP, r.s.n_run, i, 1);
        a.tab_score = d->tab_score + (size_t)i * ATS_MAX_CAND; a.tab_off = d->tab_off + (size_t)i * (MAXB + 1); a.tab_lse = d->tab_lse + i;
      }
      if (a.cutoff) wargs.push_back(warp_cut_args(d, a));
      args.push_back(a);
    }
    ATS_TRY(warp_cutoffs(wargs, st));
    ATS_TRY(launch_staged(args, ats_beam_step_multi, st));
  }
  hipEventRecord(g_ev[1], st);
  hipEventRecord(g_ev[5], st);                     // the draft's end (g_ev[1] moves on to the start of a staged round's last phase)
  // ---- 2. target forward and 3. verify (:190-232, :242-456, :505-509), in phases.  A phase forwards blocks b0 .. b1 (round_plan.h) of every
  //         verifying user whose walk is still pending -- phase 0 also the inputs of every user on its final step -- and ends with those users'
  //         walks over the blocks that have rows so far.  Packed: one phase that holds every block.  Staged (bssd_round_staged): phase p holds
  //         block p, and every phase but the last ends with one mailbox read-back
  float ms_t = 0.f, ms_v = 0.f;                    // target / verify time of the phases already read back
  if (!ver.empty() || !fin.empty()) {
    const bool staged = ctl.lock_step && bssd_round_staged(ver, fin);
    std::vector<VerifyArgs> vall(ver.size());      // every verifying user's walk, built in phase 0; a later phase adds its block's rows
    std::vector<int> row_first(ver.size());        // ... whose rows are counted from the user's first logit row of the round
    std::vector<size_t> pend(ver.size());          // indices into ver: the users of the phase
    for (size_t j = 0; j < ver.size(); ++j) pend[j] = j;
    int row_off = 0;                               // logit rows the earlier phases of the round hold
    for (int p = 0;; ++p) {
      SegTable t{};
      for (size_t j : pend) {
        atspeed_decoder* d = ver[j];
        atspeed_decoder::Run& r = d->run;
        const ats_round::Blocks ph = ats_round::phase_blocks(staged, p, r.dl);
        t.seg[t.n++] = span_seg(d->tin[r.cur], W, ats_round::span(r, ph.b0, ph.b1), d->tkv, d->opts.adapter);
        if (p == 0) r.s.n_target_forwards++;
        r.s.n_target_passes++;
      }
      if (p == 0) for (atspeed_decoder* d : fin) {
        atspeed_decoder::Run& r = d->run;
        t.seg[t.n++] = span_seg(d->tin[r.cur], W, ats_round::span(r, 0, 0), d->tkv, d->opts.adapter);
        r.s.n_target_forwards++; r.s.n_target_passes++;
      }
      ATS_TRY(ats_seg_finish(t));
      ATS_TRY(decode_forward(T, t, decs[0]->run.fsm, decs[0]->run.k, st, row_off));
      if (p == 0) ctl.target_forwards++;
      ctl.target_passes++;
      hipEventRecord(g_ev[2], st);
      // ---- 3. verify for the phase's users, one workgroup each
      std::vector<VerifyArgs> vargs;
      std::vector<WarpCutArgs> wargs;                  // sampling-mode warpers: the cutoffs of this round's verify walks and final steps
      bool more = false;                               // a walk can be pending only where the user has a block without rows left
      for (size_t i = 0; i < pend.size(); ++i) {
        atspeed_decoder* d = ver[pend[i]];
        atspeed_decoder::Run& r = d->run;
        VerifyArgs& va = vall[pend[i]];
        if (p == 0) {                                  // the walk's rows start at the user's first row of the round ...
          va = verify_args(d, T);
          const RowViews rv = seg_rows(T, t.seg[i]);
          va.logits = rv.logits; va.lse = rv.lse; va.row_cand = rv.row_cand;
          row_first[pend[i]] = t.seg[i].logit_row0;
        }
        // ... and block b's are where the phase that forwarded it put them: behind the span's earlier blocks
        const ats_round::Blocks ph = ats_round::phase_blocks(staged, p, r.dl);
        const int span_row0 = row_off + t.seg[i].logit_row0 - row_first[pend[i]];
        for (int b = ph.b0; b <= ph.b1; ++b) va.blk_row0[b] = span_row0 + ats_round::logit_row(r, ph.b0, b);
        va.blocks_ready = ph.b1 + 1;
        more = more || ph.b1 < r.dl;
        if (va.cutoff) wargs.push_back(warp_cut_args(d, va));
        vargs.push_back(va);
      }
      std::vector<BeamStepArgs> fargs;
      if (p == 0) for (size_t j = 0; j < fin.size(); ++j) {
        atspeed_decoder* d = fin[j];
        atspeed_decoder::Run& r = d->run;
        BeamStepArgs a = beam_step_args(d, T, t.seg[ver.size() + j], r.fsm, d->round_beams[r.cur], d->round_beams[r.cur ^ 1], r.gen, r.k);   // emits nothing
        if (a.sample) a.rng_sub = ats_rng_sub(d->seed, ATS_RNG_STEP, r.s.n_run, 0, 0);
        if (a.cutoff) wargs.push_back(warp_cut_args(d, a));
        fargs.push_back(a);
      }
      ATS_TRY(warp_cutoffs(wargs, st));
      if (!vargs.empty()) ATS_TRY(launch_staged(vargs, ats_verify_walk_multi, st));
      if (!fargs.empty()) ATS_TRY(launch_staged(fargs, ats_beam_step_multi, st));
      if (p == 0) for (atspeed_decoder* d : fin) { d->run.cur ^= 1; d->run.gen += 1; }
      if (!more) break;
      // ---- hand-over: the phase's mailbox read-back; the next phase is built for the users still pending
      hipEventRecord(g_ev[3], st);
      ATS_HIP(hipStreamSynchronize(st));
      ats_stage_reset();
      float a_ms = 0.f, b_ms = 0.f;
      hipEventElapsedTime(&a_ms, g_ev[1], g_ev[2]);
      hipEventElapsedTime(&b_ms, g_ev[2], g_ev[3]);
      ms_t += a_ms; ms_v += b_ms;
      std::vector<size_t> next;
      for (size_t j : pend) if (ver[j]->mail_host->n_matches == ATS_WALK_PENDING && ver[j]->mail_host->status == 0) next.push_back(j);
      row_off += t.total_logit;
      pend.swap(next);
      hipEventRecord(g_ev[1], st);                   // the next phase's start (the last phase's brackets are read with the round's own read-back)
      hipEventRecord(g_ev[2], st);
      if (pend.empty()) break;
    }
  } else {
    hipEventRecord(g_ev[2], st);
  }
  hipEventRecord(g_ev[3], st);
  // ---- 4. outputs of finished users, mailboxes, the round's single synchronisation
  std::vector<ExportBeamsArgs> ex;                  // users finishing this round: one export launch for all of them
  for (int u = 0; u < n; ++u) {
    atspeed_decoder* d = decs[u];
    atspeed_decoder::Run& r = d->run;
    if (!r.done && r.final_step) ex.push_back(ExportBeamsArgs{d->round_beams[r.cur], r.out_tokens, r.out_scores, d->sample ? 1 : 0});
  }
  if (!ex.empty()) ATS_TRY(export_beams(ex, decs[0]->run.k, decs[0]->run.max_new, st));
  for (int u = 0; u < n; ++u) {
    atspeed_decoder* d = decs[u];
    atspeed_decoder::Run& r = d->run;
    if (r.done) continue;
    if (!r.final_step && ctl.flat_trace)  // trace of the draft's flat ids (parity tests drive one user at a time; batches skip the copies)
      for (int i = 1; i <= r.dl; ++i)
        ATS_HIP(hipMemcpyAsync(d->trace_host + (i - 1) * MAXB, d->blk[i].flat, sizeof(int32_t) * r.dk, hipMemcpyDeviceToHost, st));
    if (d->trace_level >= 1 && !r.export_only)
      ATS_HIP(hipMemcpyAsync(d->dump_host, d->beam_area, d->beam_area_bytes, hipMemcpyDeviceToHost, st));
  }
  ATS_HIP(hipStreamSynchronize(st));
  ats_stage_reset();
  float ms_d = 0.f, ms_tl = 0.f, ms_vl = 0.f;
  hipEventElapsedTime(&ms_d, g_ev[0], g_ev[5]);
  hipEventElapsedTime(&ms_tl, g_ev[1], g_ev[2]);
  hipEventElapsedTime(&ms_vl, g_ev[2], g_ev[3]);
  ms_t += ms_tl; ms_v += ms_vl;
  int n_act = 0;
  for (int u = 0; u < n; ++u) if (!decs[u]->run.done) ++n_act;
  if (!ver.empty() && !ver[0]->sample)             // staged verification's memory: a round of walks halves the weight of what came before
    for (int j = 1; j <= ATSPEED_MAX_GAMMA; ++j) { T->stg_drafted[j] *= 0.5; T->stg_needed[j] *= 0.5; }
  ctl.any = false;
  for (int u = 0; u < n; ++u) {
    atspeed_decoder* d = decs[u];
    atspeed_decoder::Run& r = d->run;
    if (r.done) continue;
    // a lock-step batch does not die with one user: a prefix mismatch or a filtered user ends here with no valid beam, the others go on
    if (d->mail_host->pad && !ctl.keep_filtered) return prefix_mismatch_error(d);
    if (ctl.keep_filtered && ends_alone_status(d) != ATSPEED_OK) { ATS_TRY(finish_user(d, ends_alone_status(d), 0, true, st)); continue; }
    ATS_TRY(mailbox_status(d));
    // stage times: the group's stage time shared equally by the users that were active in the round
    r.s.draft_ms += ms_d / n_act; r.s.target_ms += ms_t / n_act; r.s.verify_ms += ms_v / n_act;
    if (r.final_step) {
      // `cur` was flipped when the step was launched: the parents are round_beams[cur ^ 1], the result round_beams[cur]
      if (d->trace_level >= 1 && !r.export_only) decisions_append(d, 1, r.nb, 0, 0, r.gen - 1, r.k, r.dk, {r.cur ^ 1, r.cur});
      ATS_TRY(finish_user(d, ATSPEED_OK, d->mail_host->n_valid, false, st));
      continue;
    }
    const int nm = d->mail_host->n_matches, dl = r.dl, dk = r.dk;
    ATS_REQUIRE(nm >= 0 && nm <= dl, ATSPEED_ERR_HIP, "bssd: a verify walk reported %d accepted steps of %d", nm, dl);
    if (!d->sample) for (int j = 1; j <= dl; ++j) { T->stg_drafted[j] += 1.; T->stg_needed[j] += nm >= j ? 1. : 0.; }
    if (ctl.flat_trace) {
      d->trace.push_back(dl); d->trace.push_back(nm); d->trace.push_back(r.nb);
      for (int i = 0; i < dl; ++i) for (int j = 0; j < dk; ++j) d->trace.push_back(d->trace_host[i * MAXB + j]);
    }
    if (d->trace_level >= 1) {
      std::vector<int> blocks{r.cur};
      for (int i = 1; i <= dl; ++i) blocks.push_back(2 + i);
      blocks.push_back(r.cur ^ 1);
      decisions_append(d, 0, r.nb, dl, nm, r.gen, r.k, dk, blocks);
    }
    if (r.s.n_run < ATSPEED_MAX_NEW_TOKENS) r.s.accept_steps[r.s.n_run] = nm;
    r.s.n_run++; r.s.total_accept_steps += nm;
    ats_round::advance(r, nm, dl);        // :522: compact (keep up to the end of block nm), the k new beams are the next inputs
    r.cur ^= 1;
    ctl.any = true;
  }
  return ATSPEED_OK;
}

// n users in lock step from their first round to the last one's end (the one-user and the batch call): a user leaves when its last round
// ends, nobody takes its place
static int bssd_group_run(atspeed_decoder** decs, int n, hipStream_t st, bool lock_step) {
  hipEvent_t* g_ev = nullptr;
  ATS_TRY(stage_events(&g_ev));
  std::vector<int> n0(n);
  for (int u = 0; u < n; ++u) n0[u] = decs[u]->run.n0;
  const atspeed_decoder::Run& r0 = decs[0]->run;     // one gamma, k and dk for the whole call
  ATS_TRY(bssd_ensure_capacity(decs[0]->target, decs[0]->draft, n0, r0.gamma, r0.k, r0.dk));
  RoundCtl ctl{n <= 4, n > 1, lock_step};
  do ATS_TRY(bssd_round(decs, n, st, g_ev, ctl)); while (ctl.any);
  return ATSPEED_OK;
}

extern "C" int atspeed_bssd_generate_batch(atspeed_decoder** decs, int32_t n, const int32_t* const* prompts,
                                           const int32_t* prompt_lens, const atspeed_fsm* fsm, const int32_t* start_nodes,
                                           int32_t gamma, int32_t max_new, int32_t k, int32_t dk, int32_t* const* out_tokens,
                                           float* const* out_scores, atspeed_gen_stats* stats, void* stream) {
  ATS_REQUIRE(decs && prompts && prompt_lens && start_nodes && out_tokens && out_scores, ATSPEED_ERR_INVALID, "bssd_batch: null argument");
  ATS_REQUIRE(n >= 1 && n <= ATS_MAX_SEGS, ATSPEED_ERR_CAPACITY, "bssd_batch: %d users per call (max %d)", n, ATS_MAX_SEGS);
  hipStream_t st = (hipStream_t)stream;
  for (int i = 0; i < n; ++i) {
    ATS_TRY(same_pair_once("bssd_batch", "decoders must share one target/draft pair", decs, i, 1));
    ATS_TRY(bssd_begin(decs[i], prompts[i], prompt_lens[i], fsm, start_nodes[i], gamma, max_new, k, dk, out_tokens[i], out_scores[i],
                       stats ? &stats[i] : nullptr, st, false));
  }
  ATS_TRY(start_users(decs, n, prompts, prompt_lens, start_nodes, true, st));
  return bssd_group_run(decs, n, st, true);
}

extern "C" int atspeed_bssd_generate(atspeed_decoder* d, const int32_t* prompt, int32_t P, const atspeed_fsm* fsm,
                                     int32_t start_node, int32_t gamma, int32_t max_new, int32_t k, int32_t dk,
                                     int32_t* out_tokens, float* out_scores, atspeed_gen_stats* stats, void* stream) {
  ATS_TRY(bssd_begin(d, prompt, P, fsm, start_node, gamma, max_new, k, dk, out_tokens, out_scores, stats, (hipStream_t)stream));
  return bssd_group_run(&d, 1, (hipStream_t)stream, false);
}

// ---- sessions (include/atspeed_hip.h "sessions"): the same round over a fixed set of lanes, each free lane refilled from a host queue at the
// round boundary.  The tables (lanes, tickets, queue) are host-only code in session_queue.h; here is what touches the device.
namespace {
struct SessionJob {          // a submitted user, as it waits in the queue and then sits in its lane
  const int32_t* prompt = nullptr; int P = 0, start_node = 0; uint32_t seed = 0;
  int32_t* out_tokens = nullptr; float* out_scores = nullptr; atspeed_gen_stats* stats = nullptr;
  UserOpts opts;             // its item filter, adapter slot and prompt prefixes (atspeed_session_submit_ex): its lane's decoder holds them while it decodes
};
}  // namespace
struct atspeed_session {
  std::vector<atspeed_decoder*> lanes;
  const atspeed_fsm* fsm = nullptr;
  int gamma = 0, max_new = 0, k = 0, dk = 0, max_prompt = 0;
  hipStream_t st = nullptr;
  ats_session::Queue<SessionJob> q;
  int64_t target_forwards = 0, target_passes = 0, draft_forwards = 0, allocs_after_create = 0;
  bool arena_failed = false;
  explicit atspeed_session(int n) : q(n) {}
};

// the split-K arena a model's forwards of >= 257 tokens take, reserved ahead of the first of them; false: wanted and not to be had
static bool session_reserve_arena(atspeed_llama* m, int worst_tokens, hipStream_t st) {
  const bool wanted = worst_tokens >= 257 && m->cfg.dtype != ATSPEED_F32 && m->cfg.hidden % 128 == 0;     // as sk_arena_lazy
  if (!wanted) return true;
  sk_arena_lazy(m, worst_tokens, st);
  return m->act->sk.ws != nullptr;
}

extern "C" int atspeed_session_create(atspeed_decoder* const* lanes, int32_t n_lanes, const atspeed_fsm* fsm, int32_t gamma, int32_t max_new,
                                      int32_t k, int32_t dk, int32_t max_prompt, void* stream, atspeed_session** out) {
  ATS_REQUIRE(lanes && fsm && out, ATSPEED_ERR_INVALID, "session_create: null argument");
  ATS_REQUIRE(n_lanes >= 1 && n_lanes <= ATS_MAX_SEGS, ATSPEED_ERR_CAPACITY, "session_create: %d lanes (1 .. %d)", n_lanes, ATS_MAX_SEGS);
  ATS_REQUIRE(max_prompt >= 1, ATSPEED_ERR_INVALID, "session_create: max_prompt %d must be positive", max_prompt);
  ATS_TRY(check_ranges("session_create", max_new, k, true, dk, gamma));
  for (int i = 0; i < n_lanes; ++i) {
    ATS_TRY(same_pair_once("session_create", "lanes must be decoders of one target/draft pair", lanes, i, 2));
    const atspeed_decoder *d = lanes[i], *d0 = lanes[0];
    ATS_REQUIRE(d->max_prompt >= max_prompt, ATSPEED_ERR_CAPACITY, "session_create: lane %d holds prompts of %d tokens, the session asks for %d",
                i, d->max_prompt, max_prompt);
    ATS_REQUIRE(d->sample == d0->sample && d->temperature == d0->temperature && d->top_k == d0->top_k && d->top_p == d0->top_p &&
                d->min_keep == d0->min_keep, ATSPEED_ERR_INVALID, "session_create: lane %d differs from lane 0 in sampling mode, temperature or warpers", i);
  }
  atspeed_llama *T = lanes[0]->target, *D = lanes[0]->draft;
  ATS_REQUIRE(fsm->dev.vocab == T->cfg.vocab_size, ATSPEED_ERR_INVALID, "session_create: constraint vocab %d != model vocab %d", fsm->dev.vocab,
              T->cfg.vocab_size);
  ATS_REQUIRE(!(lanes[0]->sample && fsm->dev.n_nodes == 0), ATSPEED_ERR_INVALID,
              "session_create: sampling needs a constraint automaton (mask-free search is greedy only)");
  Building<atspeed_session> s(new atspeed_session(n_lanes), atspeed_session_destroy);
  s->lanes.assign(lanes, lanes + n_lanes);
  s->fsm = fsm; s->gamma = gamma; s->max_new = max_new; s->k = k; s->dk = dk; s->max_prompt = max_prompt; s->st = (hipStream_t)stream;
  // everything a round allocates on demand, now: activations for the worst round, stage events, the staging ring, the split-K arenas
  const std::vector<int> n0(n_lanes, max_prompt);          // any lane may hold the longest prompt
  ATS_TRY(bssd_ensure_capacity(T, D, n0, gamma, k, dk));
  hipEvent_t* ev = nullptr;
  ATS_TRY(stage_events(&ev));
  const int32_t zero = 0; const void* staged = nullptr;
  ATS_TRY(ats_stage(&zero, sizeof(zero), &staged, s->st));
  const ats_round::Capacity worst = ats_round::worst_round(n0.data(), n_lanes, gamma, k, dk, MAXB);
  const bool got_t = session_reserve_arena(T, worst.t_tok, s->st);
  const bool got_d = session_reserve_arena(D, worst.d_tok, s->st);
  ATS_HIP(hipStreamSynchronize(s->st));
  ats_stage_reset();
  g_last_error.clear();
  if (!got_t || !got_d) {
    s->arena_failed = true;
    atspeed_set_error("session_create: no room for the %s model's split-K arena (%zu MB): thin GEMM grids of rounds above 256 tokens take the "
                      "device's shared arena or the plain grid", got_t ? "draft" : "target", ATS_SK_ARENA_BYTES >> 20);
  }
  *out = s.release();
  return ATSPEED_OK;
}

// a decoder whose user has gone (finished, failed with its round, or left in its lane by a session that is closed) holds nobody's options:
// the filter and the prefixes may be freed, and the decoder's next caller starts from nothing
static void user_leaves(atspeed_decoder* d) { d->opts = UserOpts{}; }

extern "C" void atspeed_session_destroy(atspeed_session* s) {
  for (int l = 0; s && l < s->q.n_lanes(); ++l) if (s->q.lane_busy(l)) user_leaves(s->lanes[l]);    // the lanes' decoders outlive the session
  delete s;
}

extern "C" int atspeed_session_submit_masked(atspeed_session* s, const int32_t* prompt, int32_t P, int32_t start_node, uint32_t seed,
                                             int32_t* out_tokens, float* out_scores, atspeed_gen_stats* stats, const atspeed_node_masks* masks,
                                             int32_t user, int64_t* ticket_out) {
  atspeed_session_user u{};
  u.struct_size = sizeof(u); u.prompt_ids_dev = prompt; u.prompt_len = P; u.start_node = start_node; u.seed = seed;
  u.out_tokens_dev = out_tokens; u.out_scores_dev = out_scores; u.stats_host = stats; u.masks = masks; u.mask_user = user;
  return atspeed_session_submit_ex(s, &u, ticket_out);
}

// the one submit entry: every per-user property in a struct (members past the caller's struct_size are 0)
extern "C" int atspeed_session_submit_ex(atspeed_session* s, const atspeed_session_user* user_in, int64_t* ticket_out) {
  ATS_REQUIRE(s && user_in && ticket_out, ATSPEED_ERR_INVALID, "session_submit: null argument");
  ATS_REQUIRE(user_in->struct_size >= offsetof(atspeed_session_user, masks), ATSPEED_ERR_INVALID, "session_submit: struct_size %zu is too small",
              user_in->struct_size);
  atspeed_session_user uu{};
  memcpy(&uu, user_in, std::min(user_in->struct_size, sizeof(uu)));
  const int32_t P = uu.prompt_len;
  const UserOpts opts{uu.masks, uu.masks ? uu.mask_user : 0, uu.adapter, uu.target_prefix, uu.draft_prefix};
  ATS_REQUIRE(!opts.masks || (opts.mask_user >= 0 && opts.mask_user < opts.masks->n_users), ATSPEED_ERR_INVALID, "session_submit: filter user %d out of [0, %d)",
              opts.mask_user, opts.masks ? opts.masks->n_users : 0);
  ATS_TRY(check_common(s->lanes[0], uu.prompt_ids_dev, P, s->fsm, uu.start_node, s->max_new, s->k, uu.out_tokens_dev, uu.out_scores_dev));
  ATS_TRY(user_opts_check("session_submit", s->lanes[0]->target, s->lanes[0]->draft, s->fsm, opts, P, true));
  ATS_REQUIRE(P <= s->max_prompt, ATSPEED_ERR_CAPACITY, "session_submit: prompt length %d exceeds the session's max_prompt %d", P, s->max_prompt);
  // a user's rounds need up to P + (max_new - 1) * dk KV slots (every draft block of the call kept): refused here, where it costs nobody else
  // a round, rather than inside one
  const int slots = ats_round::call_slots(P, s->max_new, s->dk), max_slots = s->lanes[0]->target->cfg.max_slots;
  ATS_REQUIRE(slots <= max_slots, ATSPEED_ERR_CAPACITY, "session_submit: prompt of %d tokens can need %d KV slots (%d available)", P, slots, max_slots);
  *ticket_out = s->q.submit(SessionJob{uu.prompt_ids_dev, P, uu.start_node, uu.seed, uu.out_tokens_dev, uu.out_scores_dev, uu.stats_host, opts});
  return ATSPEED_OK;
}

extern "C" int atspeed_session_submit(atspeed_session* s, const int32_t* prompt, int32_t P, int32_t start_node, uint32_t seed,
                                      int32_t* out_tokens, float* out_scores, atspeed_gen_stats* stats, int64_t* ticket_out) {
  return atspeed_session_submit_masked(s, prompt, P, start_node, seed, out_tokens, out_scores, stats, nullptr, 0, ticket_out);
}

// admission, one round over the occupied lanes, retirement
static int session_round(atspeed_session* s) {
  hipEvent_t* g_ev = nullptr;
  ATS_TRY(stage_events(&g_ev));
  std::vector<atspeed_decoder*> fresh;
  std::vector<const int32_t*> prompts; std::vector<int32_t> lens, starts;
  ATS_TRY(s->q.admit([&](int lane, int64_t, SessionJob& j) {
    atspeed_decoder* d = s->lanes[lane];
    d->seed = j.seed;                                   // draws follow the user, not the lane
    d->opts = j.opts;                                   // and so do its options: on at admission, off at retirement (user_leaves)
    ATS_TRY(bssd_begin(d, j.prompt, j.P, s->fsm, j.start_node, s->gamma, s->max_new, s->k, s->dk, j.out_tokens, j.out_scores, j.stats, s->st, false));
    fresh.push_back(d); prompts.push_back(j.prompt); lens.push_back(j.P); starts.push_back(j.start_node);
    return (int)ATSPEED_OK;
  }));
  if (!fresh.empty()) ATS_TRY(start_users(fresh.data(), (int)fresh.size(), prompts.data(), lens.data(), starts.data(), true, s->st));
  std::vector<atspeed_decoder*> decs; std::vector<int> lane_of;
  for (int l = 0; l < s->q.n_lanes(); ++l) if (s->q.lane_busy(l)) { decs.push_back(s->lanes[l]); lane_of.push_back(l); }
  if (decs.empty()) return ATSPEED_OK;
  ATS_TRY(bssd_ensure_capacity(decs[0]->target, decs[0]->draft, std::vector<int>(s->q.n_lanes(), s->max_prompt), s->gamma, s->k, s->dk));   // create made it: a no-op
  s->q.begin_round();
  RoundCtl ctl{false, true, true};
  ATS_TRY(bssd_round(decs.data(), (int)decs.size(), s->st, g_ev, ctl));
  s->target_forwards += ctl.target_forwards; s->draft_forwards += ctl.draft_forwards; s->target_passes += ctl.target_passes;
  for (size_t i = 0; i < decs.size(); ++i)
    if (decs[i]->run.done) {
      user_leaves(decs[i]);
      s->q.retire(lane_of[i], decs[i]->run.s.status);
    }
  return ATSPEED_OK;
}

// session_round with the allocation count around it; a failed round ends the users in lanes with its status (their state on the device is
// not to be trusted): their records are handed out by the next call, so every ticket still comes back exactly once
static int session_round_guarded(atspeed_session* s) {
  const long long a0 = g_ats_lazy_allocs.load();
  const int rc = session_round(s);
  s->allocs_after_create += g_ats_lazy_allocs.load() - a0;
  if (rc != ATSPEED_OK) {
    const std::string why = g_last_error;
    (void)hipStreamSynchronize(s->st); (void)hipGetLastError();
    ats_stage_reset();
    for (int l = 0; l < s->q.n_lanes(); ++l)
      if (s->q.lane_busy(l)) {
        (void)finish_user(s->lanes[l], rc, 0, false, s->st);
        user_leaves(s->lanes[l]);
        s->q.retire(l, rc);
      }
    g_last_error = why;
  }
  return rc;
}

// the finished users not yet reported, oldest first, as the ABI's records
static int session_take_done(atspeed_session* s, atspeed_session_done* out, int cap) {
  int n = 0;
  for (ats_session::Done d; n < cap && s->q.take_done(&d, 1) == 1; ++n)
    out[n] = atspeed_session_done{d.ticket, d.lane, d.status, d.rounds_queued, d.rounds_in_lane};
  return n;
}

extern "C" int atspeed_session_round(atspeed_session* s, atspeed_session_done* done_out, int32_t cap, int32_t* n_out) {
  ATS_REQUIRE(s && n_out, ATSPEED_ERR_INVALID, "session_round: null argument");
  *n_out = 0;
  const int64_t in_lanes = std::min<int64_t>(s->q.n_lanes(), s->q.pending());
  ATS_REQUIRE(in_lanes + s->q.done_waiting() == 0 || (done_out && cap >= in_lanes + s->q.done_waiting()), ATSPEED_ERR_CAPACITY,
              "session_round: room for %d records, %lld users can finish", cap, (long long)(in_lanes + s->q.done_waiting()));
  if (!s->q.idle()) ATS_TRY(session_round_guarded(s));
  *n_out = session_take_done(s, done_out, cap);
  return ATSPEED_OK;
}

extern "C" int atspeed_session_drain(atspeed_session* s, atspeed_session_done* done_out, int32_t cap, int32_t* n_out) {
  ATS_REQUIRE(s && n_out, ATSPEED_ERR_INVALID, "session_drain: null argument");
  *n_out = 0;
  const int64_t all = s->q.pending() + s->q.done_waiting();
  ATS_REQUIRE(all == 0 || (done_out && cap >= all), ATSPEED_ERR_CAPACITY, "session_drain: room for %d records, %lld users pending", cap, (long long)all);
  while (!s->q.idle()) ATS_TRY(session_round_guarded(s));
  *n_out = session_take_done(s, done_out, cap);
  return ATSPEED_OK;
}

extern "C" int atspeed_session_get_counters(const atspeed_session* s, atspeed_session_counters* out) {
  ATS_REQUIRE(s && out, ATSPEED_ERR_INVALID, "session_get_counters: null argument");
  const atspeed_llama* T = s->lanes[0]->target;
  *out = atspeed_session_counters{s->q.rounds(), s->target_forwards, s->draft_forwards, s->q.lane_rounds(), s->q.admitted(), s->q.retired(),
                                  s->allocs_after_create, T->act && T->act->sk.ws ? 1 : 0, s->arena_failed ? 1 : 0, s->q.n_lanes(), s->q.occupied(),
                                  s->q.queued(), s->target_passes};
  return ATSPEED_OK;
}

// ---- target_generate (beamSD.py:544-595) for n users in lock step: step g of every user is ONE forward + one beam-step launch
// (the teacher-data job of generate_teacher_data.py:211-244 is exactly this loop over a whole training set)
static int target_check(atspeed_decoder* d, const int32_t* prompt, int P, const atspeed_fsm* fsm, int start_node, int max_new, int k,
                        const int32_t* out_tokens, const float* out_scores) {
  ATS_TRY(check_common(d, prompt, P, fsm, start_node, max_new, k, out_tokens, out_scores));
  ATS_REQUIRE(P + max_new * k <= d->target->cfg.max_slots, ATSPEED_ERR_CAPACITY, "target_generate: KV slots exhausted");
  ATS_REQUIRE(P + max_new * k <= d->tok_cap, ATSPEED_ERR_CAPACITY, "target_generate: token buffer too small");
  ATS_TRY(user_opts_check("target_generate", d->target, d->draft, fsm, d->opts, P, false));
  return ATSPEED_OK;
}

// the users have passed target_check.  One user's launches take their arguments by value (nothing but the segment table is staged: no
// host-to-device copy in front of its beam kernels); several users' go through staged argument blocks, one workgroup per user.
static int target_group_run(atspeed_decoder** decs, int n, const int32_t* const* prompts, const int32_t* prompt_lens, const atspeed_fsm* fsm,
                            const int32_t* start_nodes, int max_new, int k, int32_t* const* out_tokens, float* const* out_scores,
                            atspeed_gen_stats* stats, hipStream_t st) {
  atspeed_llama* T = decs[0]->target;
  const int W = decs[0]->W;
  const ats_round::Capacity cap = ats_round::worst_round(prompt_lens, n, 0, k, k, MAXB);     // no draft blocks: the target's steps alone
  ATS_TRY(ensure_act(T, cap.t_tok, cap.t_rows));
  hipEvent_t* g_ev = nullptr;
  ATS_TRY(stage_events(&g_ev));
  if (n == 1) ATS_TRY(start_user(decs[0], prompts[0], prompt_lens[0], start_nodes[0], false, st));
  else        ATS_TRY(start_users(decs, n, prompts, prompt_lens, start_nodes, false, st));
  hipEventRecord(g_ev[0], st);
  struct St { int row0, n_in, nb, base, cur; };
  std::vector<St> s(n);
  for (int u = 0; u < n; ++u) s[u] = St{0, prompt_lens[u] - prefix_len(decs[u]), 1, prefix_len(decs[u]), 0};   // behind the user's prefix, if it has one
  std::vector<BeamStepArgs> args(n);
  std::vector<WarpCutArgs> wargs;
  for (int g = 0; g < max_new; ++g) {                                                // beamSD.py:579-588
    SegTable t{};
    for (int u = 0; u < n; ++u)
      t.seg[t.n++] = make_seg(tb_offset(decs[u]->tin[0], s[u].row0, W), s[u].n_in, s[u].base + s[u].n_in, s[u].nb, decs[u]->tkv, decs[u]->opts.adapter);
    ATS_TRY(ats_seg_finish(t));
    ATS_TRY(decode_forward(T, t, fsm, k, st));
    for (int u = 0; u < n; ++u) {
      atspeed_decoder* d = decs[u];
      BeamStepArgs& a = args[u];
      a = beam_step_args(d, T, t.seg[u], fsm, d->round_beams[s[u].cur], d->round_beams[s[u].cur ^ 1], g, k);
      beam_step_emit(a, d->tin[0], s[u].row0 + s[u].n_in - s[u].nb, s[u].row0 + s[u].n_in, s[u].base + s[u].n_in);
      if (a.sample) a.rng_sub = ats_rng_sub(d->seed, ATS_RNG_STEP, g, 0, 0);
      if (a.cutoff) wargs.push_back(warp_cut_args(d, a));
      s[u].row0 += s[u].n_in; s[u].base += s[u].n_in; s[u].n_in = k; s[u].nb = k; s[u].cur ^= 1;
    }
    ATS_TRY(warp_cutoffs(wargs, st));
    wargs.clear();
    if (n == 1) ATS_TRY(ats_beam_step(args[0], st));
    else        ATS_TRY(launch_staged(args, ats_beam_step_multi, st));
  }
  std::vector<ExportBeamsArgs> ex;
  for (int u = 0; u < n; ++u) ex.push_back(ExportBeamsArgs{decs[u]->round_beams[s[u].cur], out_tokens[u], out_scores[u], decs[u]->sample ? 1 : 0});
  ATS_TRY(export_beams(ex, k, max_new, st));
  hipEventRecord(g_ev[1], st);
  ATS_HIP(hipStreamSynchronize(st));
  ats_stage_reset();
  float ms = 0.f;
  hipEventElapsedTime(&ms, g_ev[0], g_ev[1]);
  // a lock-step batch does not die with a user that lost every beam of a step to the id filter: that user ends with a blanked result block
  // and its status, the others go on (as in the beam-SD batch loop); the one-user call returns the error
  // so does a user whose prompt does not open with its prompt prefix, with ATSPEED_ERR_INVALID (ends_alone_status)
  if (n == 1 && decs[0]->mail_host->pad) return prefix_mismatch_error(decs[0]);
  bool any_filtered = false;
  for (int u = 0; u < n; ++u)
    if (n > 1 && ends_alone_status(decs[u]) != ATSPEED_OK) { ATS_TRY(blank_outputs(out_tokens[u], out_scores[u], k, max_new, st)); any_filtered = true; }
  if (any_filtered) ATS_HIP(hipStreamSynchronize(st));
  for (int u = 0; u < n; ++u) {
    const int alone = n > 1 ? ends_alone_status(decs[u]) : ATSPEED_OK;
    const bool filtered = alone != ATSPEED_OK;
    if (!filtered) ATS_TRY(mailbox_status(decs[u]));
    if (stats) {
      atspeed_gen_stats gs;
      memset(&gs, 0, sizeof(gs));
      gs.n_target_forwards = gs.n_target_passes = max_new; gs.n_valid = filtered ? 0 : decs[u]->mail_host->n_valid;
      gs.status = alone;
      gs.total_ms = gs.target_ms = ms / n;                      // the group's time shared equally by its users
      stats[u] = gs;
    }
  }
  return ATSPEED_OK;
}

extern "C" int atspeed_target_generate_batch(atspeed_decoder** decs, int32_t n, const int32_t* const* prompts,
                                             const int32_t* prompt_lens, const atspeed_fsm* fsm, const int32_t* start_nodes,
                                             int32_t max_new, int32_t k, int32_t* const* out_tokens, float* const* out_scores,
                                             atspeed_gen_stats* stats, void* stream) {
  ATS_REQUIRE(decs && prompts && prompt_lens && start_nodes && out_tokens && out_scores, ATSPEED_ERR_INVALID, "target_generate_batch: null argument");
  ATS_REQUIRE(n >= 1 && n <= ATS_MAX_SEGS, ATSPEED_ERR_CAPACITY, "target_generate_batch: %d users per call (max %d)", n, ATS_MAX_SEGS);
  for (int u = 0; u < n; ++u) {
    ATS_TRY(same_pair_once("target_generate_batch", "decoders must share one target model", decs, u, 0));
    ATS_TRY(target_check(decs[u], prompts[u], prompt_lens[u], fsm, start_nodes[u], max_new, k, out_tokens[u], out_scores[u]));
  }
  return target_group_run(decs, n, prompts, prompt_lens, fsm, start_nodes, max_new, k, out_tokens, out_scores, stats, (hipStream_t)stream);
}

extern "C" int atspeed_target_generate(atspeed_decoder* d, const int32_t* prompt, int32_t P, const atspeed_fsm* fsm,
                                       int32_t start_node, int32_t max_new, int32_t k, int32_t* out_tokens,
                                       float* out_scores, atspeed_gen_stats* stats, void* stream) {
  ATS_TRY(target_check(d, prompt, P, fsm, start_node, max_new, k, out_tokens, out_scores));
  return target_group_run(&d, 1, &prompt, &P, fsm, &start_node, max_new, k, &out_tokens, &out_scores, stats, (hipStream_t)stream);
}

extern "C" int atspeed_decoder_trace(atspeed_decoder* d, int32_t* rounds_out, int32_t cap) {
  if (!d) return 0;
  int n = (int)std::min<size_t>(d->trace.size(), (size_t)std::max(cap, 0));
  if (rounds_out && n > 0) memcpy(rounds_out, d->trace.data(), sizeof(int32_t) * n);
  return (int)d->trace.size();
}
