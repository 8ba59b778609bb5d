// Scan kernels of beam speculative decoding: full-vocabulary log-sum-exp, fused
// constraint-mask + beam expand + top-K prune, the top-K-aligned acceptance test, and the
// on-device bookkeeping (visibility bitsets, positions, KV slots, beam suffixes) that the
// reference does with host round trips (beamSD.py:58-91, :278-380, :383-416).
//
// Each piece the kernels share is written once, where its section comment stands: candidate keys (below), block top-k, the candidate
// enumeration of an expand (cand_rows / cand_at) with the blocked-edge test and the tempered score, the argument-block loader of the
// multi kernels, the step rows and the output tail of the two verify walks.  Block sums and maxima are common.h's (block_sum / block_max).
#include "internal.h"
#include <cstdlib>
#include <memory>

namespace {

constexpr int kScanThreads = 1024;
constexpr int kScanWaves = kScanThreads / 64;
constexpr int kCPT = 16;                               // candidate slots per thread
constexpr int kMaxCand = kScanThreads * kCPT;          // 16384 >= 64 beams * 256 children
constexpr int MAXB = ATSPEED_MAX_BEAMS;
constexpr int LMAX = ATSPEED_MAX_NEW_TOKENS;

// Candidate keys are 64-bit: (monotone(score) << 32) | ~flat_id, so an unsigned max gives "highest score first, lowest flat id on ties" --
// the tie-break this build defines (torch.topk leaves it unspecified).  Key 0 = no candidate.  A -0.0 score takes +0.0's key (ford_key),
// so the two zeros tie by flat id.  A score of -inf is no candidate and a NaN is one: the callers that can meet either say so themselves.
__device__ __forceinline__ unsigned long long cand_key(float score, uint32_t flat) {
  return ((unsigned long long)ford_key(score) << 32) | (unsigned long long)(~flat);
}
__device__ __forceinline__ int flat_of_key(unsigned long long key) { return key ? (int)(~(uint32_t)(key & 0xffffffffull)) : -1; }

// one multi-kernel workgroup's argument block, from the device array into its __shared__ copy
template <typename A>
__device__ __forceinline__ void load_args(A& a, const A* __restrict__ src) {
  static_assert(sizeof(A) % 4 == 0, "argument blocks are copied word by word");
  for (int i = threadIdx.x; i < (int)(sizeof(A) / 4); i += blockDim.x) reinterpret_cast<uint32_t*>(&a)[i] = reinterpret_cast<const uint32_t*>(src)[i];
  __syncthreads();
}

// ---------------------------------------------------------------------------- LSE
// one workgroup per row, 16-byte non-temporal streaming reads (the row is read once and never again), online (max, sum) per lane.
// Chunks of 8 independent loads per thread, double-buffered: chunk c+1 is in flight while chunk c is exponentiated (with one chunk per
// 1024-thread workgroup the loads and the exponentials of a row alternated and only other workgroups overlapped them: 6.5 TB/s; the
// read-only stream peak measured by atspeed_probe_hbm_read is 7.05 TB/s).  One running-max rescale per chunk instead of per element.
template <int NT>
__global__ __launch_bounds__(NT) void lse_rows_kernel(const float* __restrict__ logits, int vocab, int ld, float* __restrict__ lse) {
  constexpr int U = 8, NWV = NT / 64;
  __shared__ float smax[NWV], ssum[NWV];
  const float* row = logits + (size_t)blockIdx.x * ld;
  const f32x4_t* row4 = reinterpret_cast<const f32x4_t*>(row);
  float m = -INFINITY, s = 0.f;
  const int nv4 = vocab >> 2;
  const int n_full = nv4 / (NT * U);                      // chunks in which every thread has all U loads
  auto load = [&](int c, f32x4_t (&v)[U]) {
#pragma unroll
    for (int u = 0; u < U; ++u) v[u] = __builtin_nontemporal_load(row4 + (size_t)c * NT * U + u * NT + threadIdx.x);
  };
  auto consume = [&](const f32x4_t (&v)[U]) {
    float cm = -INFINITY;
#pragma unroll
    for (int u = 0; u < U; ++u) cm = fmaxf(cm, fmaxf(fmaxf(v[u][0], v[u][1]), fmaxf(v[u][2], v[u][3])));
    if (cm > m) { s *= __expf(m - cm); m = cm; }
    if (m != -INFINITY) {
#pragma unroll
      for (int u = 0; u < U; ++u) s += __expf(v[u][0] - m) + __expf(v[u][1] - m) + __expf(v[u][2] - m) + __expf(v[u][3] - m);
    }
  };
  f32x4_t a[U], b[U];
  if (n_full > 0) load(0, a);
  for (int c = 0; c < n_full; c += 2) {
    if (c + 1 < n_full) load(c + 1, b);
    consume(a);
    if (c + 1 >= n_full) break;
    if (c + 2 < n_full) load(c + 2, a);
    consume(b);
  }
  for (int i = n_full * NT * U + threadIdx.x; i < nv4; i += NT) {           // the last partial chunk: at most U - 1 loads per thread
    const f32x4_t v = __builtin_nontemporal_load(row4 + i);
    const float cm = fmaxf(fmaxf(v[0], v[1]), fmaxf(v[2], v[3]));
    if (cm > m) { s *= __expf(m - cm); m = cm; }
    if (m != -INFINITY) s += __expf(v[0] - m) + __expf(v[1] - m) + __expf(v[2] - m) + __expf(v[3] - m);
  }
  for (int i = (nv4 << 2) + threadIdx.x; i < vocab; i += NT) {
    float v = row[i];
    if (v > m) { s *= __expf(m - v); m = v; }
    s += __expf(v - m);
  }
  float wm = wave_max_f32(m);
  s = (m == -INFINITY) ? 0.f : s * expf(m - wm);
  s = wave_sum_f32(s);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (lane == 0) { smax[wave] = wm; ssum[wave] = s; }
  __syncthreads();
  if (threadIdx.x == 0) {
    float gm = smax[0];
    for (int w = 1; w < NWV; ++w) gm = fmaxf(gm, smax[w]);
    float gs = 0.f;
    for (int w = 0; w < NWV; ++w) gs += (smax[w] == -INFINITY) ? 0.f : ssum[w] * expf(smax[w] - gm);
    lse[blockIdx.x] = gm + logf(gs);
  }
}

// ---------------------------------------------------------------------------- block top-k
struct TopkShared {
  unsigned long long wtop[kScanWaves][MAXB];
  unsigned long long sel[MAXB];
  unsigned long long bound;                      // block_topk: lower bound of the k-th largest key after the lead rounds
};

// rounds j0 .. j1-1 of wave-argmax: the owner lane retires its key, out[j] = the j-th largest key of this wave.  Stops early -- zero-filling
// out[j .. k) -- when the wave has nothing left or its best remaining key is below `floor_key`; returns true when it stopped.
template <int NK>
__device__ __forceinline__ bool wave_topk_rounds(unsigned long long (&keys)[NK], int j0, int j1, int k, unsigned long long floor_key,
                                                 unsigned long long* out, int lane) {
  for (int j = j0; j < j1; ++j) {
    unsigned long long m = 0;
#pragma unroll
    for (int c = 0; c < NK; ++c) m = keys[c] > m ? keys[c] : m;
    const unsigned long long M = wave_max_u64(m);
    if (M == 0 || M < floor_key) {                  // wave-uniform: nothing left that can be among the block's k best
      for (int jj = j + lane; jj < k; jj += 64) out[jj] = 0;
      return true;
    }
    if (m == M) {
#pragma unroll
      for (int c = 0; c < NK; ++c) if (keys[c] == M) keys[c] = 0;
    }
    if (lane == 0) out[j] = M;
  }
  return false;
}

// every thread passes its NK candidate keys (distinct, 0 = none); afterwards sh.sel[0..k) holds the k largest, descending.
// Two phases: every wave extracts its kTopkLead best keys; the k-th largest of those 16 x kTopkLead keys is a lower bound of the block's k-th
// largest key, so a wave goes on only while its best remaining key reaches that bound -- 16 x 4 + about k wave-rounds instead of 16 x k
// (the 16 waves of a workgroup share four SIMDs: at k = 40 the full rounds were 50 of the 85 us of one user's beam step).  The selected set
// and its order are the same: every key at or above the bound is extracted by its wave, and the merge takes the k best of their union.
constexpr int kTopkLead = 4;
static_assert(kScanWaves * kTopkLead <= 64, "the bound is computed by one wave, one lead key per lane");
template <int NK>
__device__ void block_topk(unsigned long long (&keys)[NK], int k, TopkShared& sh) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int lead = k < kTopkLead ? k : kTopkLead;
  const bool done = wave_topk_rounds<NK>(keys, 0, lead, k, 0ull, sh.wtop[wave], lane);
  __syncthreads();
  if (wave == 0) {
    const unsigned long long x = lane < kScanWaves * lead ? sh.wtop[lane / lead][lane % lead] : 0ull;
    const unsigned xlo = (unsigned)(x & 0xffffffffull), xhi = (unsigned)(x >> 32);
    int rank = 0;                                    // lead keys above mine
#pragma unroll
    for (int l = 0; l < 64; ++l) {
      const unsigned long long y = ((unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)xhi, l) << 32) | (unsigned)__builtin_amdgcn_readlane((int)xlo, l);
      rank += y > x ? 1 : 0;
    }
    // the lead key with k - 1 keys above it (fewer than k lead keys: no such lane, or only lanes holding 0 -> no bound)
    const unsigned long long hit = __ballot(rank == k - 1);
    unsigned long long bound = 0;
    if (hit) {
      const int src = __ffsll((long long)hit) - 1;
      bound = ((unsigned long long)(unsigned)__shfl((int)xhi, src, 64) << 32) | (unsigned)__shfl((int)xlo, src, 64);
    }
    if (lane == 0) sh.bound = bound;
  }
  __syncthreads();
  if (!done) wave_topk_rounds<NK>(keys, lead, k, k, sh.bound, sh.wtop[wave], lane);
  __syncthreads();
  if (wave == 0) {
    unsigned long long k2[kScanWaves];
#pragma unroll
    for (int c = 0; c < kScanWaves; ++c) {
      int e = lane + 64 * c;                         // < 16*64
      k2[c] = (e < kScanWaves * k) ? sh.wtop[e / k][e % k] : 0ull;
    }
    wave_topk_rounds<kScanWaves>(k2, 0, k, k, 0ull, sh.sel, lane);
  }
  __syncthreads();
}

__device__ __forceinline__ int find_edge(const FsmDev& f, int node, int tok) {
  int lo = f.row_ptr[node], hi = f.row_ptr[node + 1];
  while (lo < hi) {                                   // children strictly ascending
    int mid = (lo + hi) >> 1;
    int t = f.tok[mid];
    if (t == tok) return mid;
    if (t < tok) lo = mid + 1; else hi = mid;
  }
  return -1;
}

// item filter: is `node` blocked for the user this automaton copy belongs to?  Callers test f.blocked first (uniform: NULL = no filter)
__device__ __forceinline__ bool node_blocked(const uint32_t* __restrict__ blocked, int node) { return (blocked[node >> 5] >> (node & 31)) & 1u; }

// item filter: an edge into a blocked node is no candidate
__device__ __forceinline__ bool edge_blocked(const FsmDev& f, int e) { return f.blocked && node_blocked(f.blocked, f.nxt[e]); }

// sampling: the log-softmax of a token at the user's temperature.  The cutoff kernel, the expand and the picks must form it bit for bit alike.
__device__ __forceinline__ float tempered(float logit, float lse, float temperature) { return (logit - lse) / temperature; }

// ---------------------------------------------------------------------------- candidate enumeration
// The candidates of an expand are the children of every live row's automaton node, rows in order, children ascending: candidate c is
// child c - off[r] of the last row r with off[r] <= c, and slot i of thread t holds candidate c = t + i * kScanThreads.
struct ExpandShared {
  TopkShared topk;
  int off[MAXB + 1];
  int node[MAXB];
  int brow[MAXB];       // row index inside the block (parent id space)
  int lrow[MAXB];       // row index inside the logits buffer
  float bscore[MAXB];
  float lse[MAXB];
  int rp[MAXB];         // first edge of the row's node (fsm.row_ptr[node]) and its number of children
  int deg[MAXB];
  float cut[MAXB];      // sampling-mode warpers: the row's cutoff of the tempered score (-inf = none)
  int status;
  float red_m[kScanWaves], red_s[kScanWaves];   // block reductions of the sampling paths
  float red_out;
};

// Row set-up of an expand over the n_rows parent rows the caller put into sh.node/brow/lrow/bscore: fills sh.lse/rp/deg (SAMPLED: and sh.cut,
// with no cutoff array -inf), then sh.off by a serial prefix over the live rows, and returns the number of candidates.  Greedy expands
// alone know free mode (no mask, prefix_allowed_tokens_fn = None): a row's candidates are then the n_row_cand entries of its row_cand list.
template <bool SAMPLED>
__device__ __forceinline__ int cand_rows(ExpandShared& sh, int n_rows, const float* __restrict__ lse, const FsmDev& fsm,
                                         const float* __restrict__ cutoff, int n_row_cand) {
  const int tid = threadIdx.x;
  const bool free_mode = !SAMPLED && fsm.n_nodes == 0;
  if (tid < n_rows) {
    // every row fetches its own edge range (one thread walking 40 rows paid 40 dependent global round trips: 35 of the 87 us a step of ONE
    // user took); the range's start stays in LDS for cand_at
    sh.lse[tid] = lse[sh.lrow[tid]];
    if constexpr (SAMPLED) sh.cut[tid] = cutoff ? cutoff[sh.lrow[tid]] : -INFINITY;
    const int nd = sh.node[tid];
    const int e0 = free_mode ? 0 : fsm.row_ptr[nd];
    sh.rp[tid] = e0;
    sh.deg[tid] = free_mode ? n_row_cand : fsm.row_ptr[nd + 1] - e0;
  }
  __syncthreads();
  if (tid == 0) {
    int tot = 0;
    for (int r = 0; r < n_rows; ++r) {
      sh.off[r] = tot;
      const int deg = sh.deg[r];
      bool live = sh.bscore[r] > -INFINITY;
      if (live && deg == 0) sh.status = ATSPEED_ERR_CONSTRAINT;   // HF: "returned an empty list" ValueError
      tot += live ? deg : 0;
    }
    sh.off[n_rows] = tot;
    if (tot > kMaxCand) sh.status = ATSPEED_ERR_CAPACITY;
  }
  __syncthreads();
  return min(sh.off[n_rows], kMaxCand);
}

// candidate c of the expand cand_rows set up: its row, its child index in the row, its edge (free mode has no edges: e is not to be used)
struct Cand { int r, j, e; };
__device__ __forceinline__ Cand cand_at(const ExpandShared& sh, int n_rows, int c) {
  int lo = 0, hi = n_rows;                            // last r with off[r] <= c
  while (hi - lo > 1) { int mid = (lo + hi) >> 1; if (sh.off[mid] <= c) lo = mid; else hi = mid; }
  const int j = c - sh.off[lo];
  return Cand{lo, j, sh.rp[lo] + j};
}

// Greedy expand: leave the k best candidates in sh.topk.sel, scored log-softmax + beam score; a blocked edge or a negative token (a padded
// row_cand entry) is dropped before it is scored.  beamSD.py:58-78.
__device__ void expand_and_select(ExpandShared& sh, int n_rows, const float* __restrict__ logits, int ld,
                                  const float* __restrict__ lse, const FsmDev& fsm, int k,
                                  const int32_t* __restrict__ row_cand = nullptr, int n_row_cand = 0) {
  const int tid = threadIdx.x;
  const bool free_mode = fsm.n_nodes == 0;
  const int total = cand_rows<false>(sh, n_rows, lse, fsm, nullptr, n_row_cand);
  unsigned long long keys[kCPT];
#pragma unroll
  for (int i = 0; i < kCPT; ++i) {
    int c = tid + i * kScanThreads;
    unsigned long long key = 0;
    if (c < total) {
      const Cand cd = cand_at(sh, n_rows, c);
      const int r = cd.r;
      int tok = free_mode ? row_cand[(size_t)sh.lrow[r] * MAXB + cd.j] : fsm.tok[cd.e];
      if (edge_blocked(fsm, cd.e)) tok = -1;
      if (tok >= 0) {
        float sc = (logits[(size_t)sh.lrow[r] * ld + tok] - sh.lse[r]) + sh.bscore[r];
        // -0.0 reaches here only as (-0.0 - +0.0) + -0.0 (x - y of unequal values is never zero and x - x is +0.0), e.g. a processor-rewritten
        // row with lse = 0: it ties with +0.0 by flat id, and comes out as +0.0
        uint32_t flat = (uint32_t)sh.brow[r] * (uint32_t)fsm.vocab + (uint32_t)tok;
        if (sc > -INFINITY || sc != sc) key = cand_key(sc, flat);
      }
    }
    keys[i] = key;
  }
  block_topk<kCPT>(keys, k, sh.topk);
}

// The k best columns of one logits row by (value desc, column asc), -inf excluded: with no mask the candidates of a beam are all V
// tokens, and the k best (row, token) pairs of an expand lie among each row's k best tokens (within a row the score is the logit plus a
// constant).  One workgroup per row; chunks of kMaxCand columns, the running best list rides along as a 17th key per thread.
__global__ __launch_bounds__(kScanThreads) void row_topk_kernel(const float* __restrict__ logits, int vocab, int ld, int kk, int32_t* __restrict__ out) {
  __shared__ TopkShared sh;
  __shared__ unsigned long long best[MAXB];
  const int tid = threadIdx.x;
  const float* row = logits + (size_t)blockIdx.x * ld;
  if (tid < MAXB) best[tid] = 0;
  __syncthreads();
  for (int c0 = 0; c0 < vocab; c0 += kMaxCand) {
    unsigned long long keys[kCPT + 1];
#pragma unroll
    for (int i = 0; i < kCPT; ++i) {
      const int col = c0 + tid + i * kScanThreads;
      unsigned long long key = 0;
      if (col < vocab) {
        const float v = row[col];
        if (v > -INFINITY || v != v) key = cand_key(v, (uint32_t)col);   // equal values, the two zeros included, rank by column
      }
      keys[i] = key;
    }
    keys[kCPT] = tid < kk ? best[tid] : 0;
    block_topk<kCPT + 1>(keys, kk, sh);
    if (tid < kk) best[tid] = sh.sel[tid];
    __syncthreads();
  }
  if (tid < MAXB) out[(size_t)blockIdx.x * MAXB + tid] = tid < kk ? flat_of_key(best[tid]) : -1;
}

struct Pick { float score; int parent; int tok; int node; int flat; };
__device__ __forceinline__ Pick no_pick() { return Pick{-INFINITY, 0, 0, 0, -1}; }

__device__ __forceinline__ Pick decode_pick(unsigned long long key, const FsmDev& fsm, const int* rows_brow,
                                            const int* rows_node, int n_rows) {
  if (key == 0) return no_pick();
  Pick p;
  const uint32_t flat = (uint32_t)flat_of_key(key);
  p.flat = (int)flat;
  p.parent = (int)(flat / (uint32_t)fsm.vocab);
  p.tok = (int)(flat % (uint32_t)fsm.vocab);
  p.score = ford_inv((uint32_t)(key >> 32));
  if (fsm.n_nodes == 0) { p.node = 0; return p; }       // no mask: there is no automaton to walk
  int nd = 0;
  for (int r = 0; r < n_rows; ++r) if (rows_brow[r] == p.parent) { nd = rows_node[r]; break; }
  int e = find_edge(fsm, nd, p.tok);
  p.node = e >= 0 ? fsm.nxt[e] : 0;
  return p;
}

// ---------------------------------------------------------------------------- sampling helpers (do_sample)
// Candidates of an expand kept in registers, slot i of thread t = candidate t + i * kScanThreads.  sc = log-softmax / temperature + beam score.
struct CandRegs { int flat[kCPT]; float sc[kCPT]; };

// Sampled expand: every candidate keeps its flat id; one below its row's cutoff or behind a blocked edge is absent by a score of -inf
// (probability 0 in every distribution formed from the table).  Returns the number of candidates.
__device__ int expand_candidates(ExpandShared& sh, int n_rows, const float* __restrict__ logits, int ld,
                                  const float* __restrict__ lse, const FsmDev& fsm, float temperature, const float* __restrict__ cutoff,
                                  CandRegs& cr) {
  const int tid = threadIdx.x;
  const int total = cand_rows<true>(sh, n_rows, lse, fsm, cutoff, 0);
#pragma unroll
  for (int i = 0; i < kCPT; ++i) {
    int c = tid + i * kScanThreads;
    cr.flat[i] = -1; cr.sc[i] = -INFINITY;
    if (c < total) {
      const Cand cd = cand_at(sh, n_rows, c);
      const int r = cd.r;
      int tok = fsm.tok[cd.e];
      const float s = tempered(logits[(size_t)sh.lrow[r] * ld + tok], sh.lse[r], temperature);
      cr.sc[i] = s < sh.cut[r] ? -INFINITY : s + sh.bscore[r];
      if (edge_blocked(fsm, cd.e)) cr.sc[i] = -INFINITY;
      cr.flat[i] = sh.brow[r] * fsm.vocab + tok;
    }
  }
  return total;
}

// log sum exp over every thread's kCPT values (block-wide); -inf entries contribute nothing.  The leading barrier: red_m / red_s / red_out
// may still be read from the previous reduction.
__device__ float block_lse(ExpandShared& sh, const float (&v)[kCPT]) {
  float m = -INFINITY;
#pragma unroll
  for (int i = 0; i < kCPT; ++i) m = fmaxf(m, v[i]);
  float s = 0.f;
  if (m > -INFINITY) {
#pragma unroll
    for (int i = 0; i < kCPT; ++i) s += (v[i] > -INFINITY) ? expf(v[i] - m) : 0.f;
  }
  float wm = wave_max_f32(m);
  s = (m > -INFINITY) ? s * expf(m - wm) : 0.f;
  s = wave_sum_f32(s);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  __syncthreads();
  // block_put (common.h) twice, written out: profiles/scan_refactor_isa_and_speed.txt, item 6
  if (lane == 0) { sh.red_m[wave] = wm; sh.red_s[wave] = s; }
  __syncthreads();
  if (threadIdx.x == 0) {
    const float gm = red_max(sh.red_m);                 // never NaN: fmaxf keeps the lanes' maxima free of them
    float gs = 0.f;
    for (int w = 0; w < kScanWaves; ++w) gs += (sh.red_m[w] > -INFINITY) ? sh.red_s[w] * expf(sh.red_m[w] - gm) : 0.f;
    sh.red_out = gm > -INFINITY ? gm + logf(gs) : -INFINITY;
  }
  __syncthreads();
  return sh.red_out;
}

// n draws without replacement with probability proportional to exp(logw): the n largest logw + Gumbel(hash(flat))
// (Plackett-Luce, the law of torch.multinomial's sequential draws); result in sh.topk.sel, key 0 = none
__device__ void sample_topn(ExpandShared& sh, const CandRegs& cr, const float (&logw)[kCPT], int n, uint32_t sub) {
  unsigned long long keys[kCPT];
#pragma unroll
  for (int i = 0; i < kCPT; ++i) {
    unsigned long long key = 0;
    if (cr.flat[i] >= 0 && logw[i] > -INFINITY) {
      float kf = logw[i] + ats_gumbel(ats_hash_u32((uint32_t)cr.flat[i], sub));
      // the CPU restatement compares the noisy keys as values: a -0.0 ties with a +0.0
      key = cand_key(kf, (uint32_t)cr.flat[i]);
    }
    keys[i] = key;
  }
  block_topk<kCPT>(keys, n, sh.topk);
}

// a pick by flat id with the TRUE tempered score (sampling keys carry noise); rows describe the expand that produced it
__device__ Pick pick_of_flat(int flat, const FsmDev& fsm, const ExpandShared& sh, int n_rows, const float* __restrict__ logits,
                             int ld, float temperature) {
  if (flat < 0) return no_pick();                     // -1 is the only negative flat id there is
  Pick p;
  p.flat = flat;
  p.parent = flat / fsm.vocab;
  p.tok = flat % fsm.vocab;
  int r = -1;
  for (int q = 0; q < n_rows; ++q) if (sh.brow[q] == p.parent) { r = q; break; }
  if (r < 0) { p.score = -INFINITY; p.node = 0; return p; }
  const float s = tempered(logits[(size_t)sh.lrow[r] * ld + p.tok], sh.lse[r], temperature);
  p.score = s + sh.bscore[r];
  int e = find_edge(fsm, sh.node[r], p.tok);
  p.node = e >= 0 ? fsm.nxt[e] : 0;
  if (e < 0 || s < sh.cut[r]) p.score = -INFINITY;
  if (e >= 0 && edge_blocked(fsm, e)) p.score = -INFINITY;
  return p;
}

// write a block of k new beams + (optionally) the forward inputs that feed them next
__device__ void emit_block(const Pick& pk, int j, int k, const BeamSet& src, int gen_len, const BeamSet& dst, bool emit,
                           const TokBuf& in, int in_row0, const TokBuf& out, int out_row0, int out_slot0) {
  if (j < k) {
    dst.score[j] = pk.score; dst.parent[j] = pk.parent; dst.tok[j] = pk.tok; dst.flat[j] = pk.flat;
    if (dst.node) dst.node[j] = pk.node;
    if (dst.seq) {
      for (int g = 0; g < gen_len; ++g) dst.seq[j * LMAX + g] = src.seq ? src.seq[pk.parent * LMAX + g] : 0;
      if (gen_len < LMAX) dst.seq[j * LMAX + gen_len] = pk.tok;
    }
    if (emit) {
      out.ids[out_row0 + j] = pk.tok;
      out.pos[out_row0 + j] = in.pos[in_row0 + pk.parent] + 1;
      out.slot[out_row0 + j] = out_slot0 + j;
    }
  }
}
__device__ void emit_vis(const int* parents /*LDS*/, int k, const TokBuf& in, int in_row0, const TokBuf& out,
                         int out_row0, int out_slot0, int W) {
  for (int idx = threadIdx.x; idx < k * W; idx += blockDim.x) {
    int j = idx / W, w = idx - j * W;
    uint64_t bits = in.vis[(size_t)(in_row0 + parents[j]) * W + w];
    int s = out_slot0 + j;
    if ((s >> 6) == w) bits |= 1ull << (s & 63);
    out.vis[(size_t)(out_row0 + j) * W + w] = bits;
  }
}

// ---------------------------------------------------------------------------- sampling-mode warpers (top-k, top-p)
// One cutoff per score row (internal.h WarpCutArgs).  The row's entries are the children of its automaton node, scored
// s = tempered(logit, lse, temperature), the expand's own function; -inf and NaN entries are no candidates.
//   top-k: k' = max(top_k, min_keep); with at least k' finite entries the k'-th largest is the threshold (ties with it survive), with
//          fewer nothing is cut (transformers' `scores < topk(scores, k')[0][..., -1]` on the full row: its k'-th largest is -inf then).
//   top-p: over what top-k left, p = softmax(s); in DESCENDING score order an entry is kept while the probability mass strictly above it
//          is below top_p, the first min_keep always (TopPLogitsWarper removes, ascending, the entries whose cumulative sum is
//          <= 1 - top_p and never the last min_keep: the same boundary seen from the other end).
// The cutoff is the score of the last kept entry, so entries tied with it survive as well.
// Nucleus sum order: fp32, over the survivors in descending score order, in runs of at most 1024 (one entry per thread): inside a run
// each wave adds its 64 entries with a Hillis-Steele ladder over the lanes, the 16 wave sums are then added in wave order onto the mass
// carried in from the earlier runs; a group of equal scores that ends a run is added entry by entry.  The normaliser (sum of
// exp(s - max) over the survivors) is a butterfly over the lanes of each wave and then the wave sums in wave order.
// A row of at most 1024 entries is sorted in LDS; a longer one takes a 4 x 8-bit radix select on ford(s) for the top-k threshold and for
// the lower end of every run, so no child-list length is assumed.
struct WarpShared {
  uint32_t key[kScanThreads];     // a descending run of keys (0 = none)
  int hist[256];
  float redf[kScanWaves];         // block_sum / block_max (common.h) of floats, and the nucleus ladder's wave sums
  uint32_t redu[kScanWaves];      // ... of counts and keys.  A barrier stands before a reduction whose array an earlier one may still be read from
  int cnt;                        // compaction cursor / first entry the nucleus drops
  int pick, above;                // radix select: the bin that holds the rank, keys above that bin
};
struct WarpRow {
  const float* logits; const FsmDev& fsm; int e0, deg; float lse, temperature;     // child j of the row's node is edge e0 + j
  __device__ __forceinline__ uint32_t key(int j) const {          // 0 = not a candidate
    if (edge_blocked(fsm, e0 + j)) return 0u;                     // the cutoffs are taken over the unblocked children only
    const float s = tempered(logits[fsm.tok[e0 + j]], lse, temperature);
    return s > -INFINITY ? ford_key(s) : 0u;         // a -0.0 (logit -0.0, lse +0.0) is tied with +0.0, as in expand_candidates' `s < cut`
  }
};

// sh.key[0 .. n2) descending, n2 a power of two <= kScanThreads (bitonic network, one entry per thread)
__device__ void warp_sort_desc(WarpShared& sh, int n2) {
  const int tid = threadIdx.x;
  for (int k = 2; k <= n2; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      __syncthreads();
      const int o = tid ^ j;
      if (tid < n2 && o > tid) {
        const uint32_t a = sh.key[tid], b = sh.key[o];
        if (((tid & k) == 0) ? a < b : a > b) { sh.key[tid] = b; sh.key[o] = a; }
      }
    }
  __syncthreads();
}

// the r-th largest (r >= 1) of the row's keys in [1, upper); the caller has counted at least r of them.  *n_above = keys in (result, upper).
__device__ uint32_t warp_radix_select(WarpShared& sh, const WarpRow& row, unsigned long long upper, int r, int* n_above) {
  const int tid = threadIdx.x;
  unsigned long long prefix = 0;
  int above = 0;
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 24 - 8 * pass;
    __syncthreads();
    if (tid < 256) sh.hist[tid] = 0;
    if (tid == 0) { sh.pick = 0; sh.above = above; }
    __syncthreads();
    for (int j = tid; j < row.deg; j += kScanThreads) {
      const unsigned long long o = row.key(j);
      if (o != 0 && o < upper && (o >> (shift + 8)) == (prefix >> (shift + 8))) atomicAdd(&sh.hist[(int)((o >> shift) & 255)], 1);
    }
    __syncthreads();
    if (tid < 256) {                                   // the bin b with  above + |bins above b| < r <= that + |b|
      int gt = above;
      for (int b = tid + 1; b < 256; ++b) gt += sh.hist[b];
      if (gt < r && r <= gt + sh.hist[tid]) { sh.pick = tid; sh.above = gt; }
    }
    __syncthreads();
    prefix |= (unsigned long long)sh.pick << shift;
    above = sh.above;
  }
  *n_above = above;
  return (uint32_t)prefix;
}

// sh.key[0 .. n) is a descending run of surviving keys; `rank` survivors of mass `head` lie above it.  Returns how many leading entries of
// the run the nucleus keeps, *mass = the mass of the whole run (sum order: see the section comment).
__device__ int warp_nucleus_run(WarpShared& sh, int n, float m, float Z, float head, int rank, float top_p, int min_keep, float* mass) {
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const float p = tid < n ? expf(ford_inv(sh.key[tid]) - m) / Z : 0.f;
  float inc = p;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) { const float u = __shfl_up(inc, o, 64); if (lane >= o) inc += u; }
  const float lower = __shfl_up(inc, 1, 64);
  __syncthreads();
  if (lane == 63) sh.redf[wave] = inc;
  if (tid == 0) sh.cnt = n;
  __syncthreads();
  float base = head, tot = 0.f;
  for (int w = 0; w < kScanWaves; ++w) { if (w < wave) base += sh.redf[w]; tot += sh.redf[w]; }
  const float before = lane ? base + lower : base;
  if (tid < n && !(before < top_p || rank + tid < min_keep)) atomicMin(&sh.cnt, tid);
  __syncthreads();
  *mass = tot;
  return sh.cnt;
}

__device__ void row_warp_cutoff_body(const WarpCutArgs& a, int r) {
  __shared__ WarpShared sh;
  const int tid = threadIdx.x;
  int sg = 0, r0 = r;
  while (sg < a.n_seg - 1 && r0 >= a.seg[sg].n) { r0 -= a.seg[sg].n; ++sg; }
  const int node = a.seg[sg].node ? a.seg[sg].node[r0] : 0;
  const int e0 = a.fsm.row_ptr[node];
  const WarpRow row{a.logits + (size_t)r * a.ld, a.fsm, e0, a.fsm.row_ptr[node + 1] - e0, a.lse[r], a.temperature};
  const bool use_p = a.top_p < 1.f;
  const int kk = a.top_k > 0 ? max(a.top_k, a.min_keep) : 0;     // 0 = top-k off
  // finite entries and the largest key
  int nf = 0;
  uint32_t kmax = 0;
  for (int j = tid; j < row.deg; j += kScanThreads) { const uint32_t o = row.key(j); nf += o ? 1 : 0; kmax = o > kmax ? o : kmax; }
  nf = (int)block_sum((uint32_t)nf, sh.redu);
  __syncthreads();
  kmax = block_max(kmax, sh.redu);
  float cut = -INFINITY;
  const bool cut_k = kk > 0 && kk <= nf;
  if (nf > 0 && (cut_k || use_p)) {
    const float m = ford_inv(kmax);
    if (row.deg <= kScanThreads) {
      int n2 = 1;
      while (n2 < row.deg) n2 <<= 1;
      sh.key[tid] = tid < row.deg ? row.key(tid) : 0u;
      warp_sort_desc(sh, n2);
      int n_surv = nf;
      if (cut_k) {
        const uint32_t tk = sh.key[kk - 1];
        n_surv = __syncthreads_count(sh.key[tid] >= tk);
        cut = ford_inv(tk);
      }
      if (use_p) {
        const float Z = block_sum(tid < n_surv ? expf(ford_inv(sh.key[tid]) - m) : 0.f, sh.redf);
        float mass;
        const int n_keep = warp_nucleus_run(sh, n_surv, m, Z, 0.f, 0, a.top_p, a.min_keep, &mass);
        cut = ford_inv(sh.key[max(n_keep, 1) - 1]);
      }
    } else {
      uint32_t tk = 1;                                 // survivors of top-k: keys >= tk
      int above;
      if (cut_k) { tk = warp_radix_select(sh, row, 1ull << 32, kk, &above); cut = ford_inv(tk); }
      if (use_p) {
        float z = 0.f;
        for (int j = tid; j < row.deg; j += kScanThreads) { const uint32_t o = row.key(j); z += o >= tk ? expf(ford_inv(o) - m) : 0.f; }
        const float Z = block_sum(z, sh.redf);
        unsigned long long upper = 1ull << 32;         // survivors not yet walked: keys in [tk, upper)
        float head = 0.f;
        int rank = 0;
        uint32_t last = kmax;
        for (;;) {
          int rem = 0;
          for (int j = tid; j < row.deg; j += kScanThreads) { const uint32_t o = row.key(j); rem += (o >= tk && o < upper) ? 1 : 0; }
          __syncthreads();
          rem = (int)block_sum((uint32_t)rem, sh.redu);
          if (rem == 0) break;                         // every survivor of top-k is kept
          // the next run: the keys in (lo, upper), fewer than 1024, and then the group of keys equal to lo; a last run takes [tk, upper)
          const bool more = rem > kScanThreads;
          uint32_t lo = tk;
          if (more) lo = warp_radix_select(sh, row, upper, kScanThreads, &above);
          __syncthreads();
          sh.key[tid] = 0u;
          if (tid == 0) sh.cnt = 0;
          __syncthreads();
          int n_eq = 0;
          for (int j = tid; j < row.deg; j += kScanThreads) {
            const uint32_t o = row.key(j);
            n_eq += (more && o == lo) ? 1 : 0;
            if (o < upper && (more ? o > lo : o >= lo)) { const int at = atomicAdd(&sh.cnt, 1); if (at < kScanThreads) sh.key[at] = o; }
          }
          __syncthreads();
          n_eq = (int)block_sum((uint32_t)n_eq, sh.redu);
          const int n = min(sh.cnt, kScanThreads);
          int n2 = 1;
          while (n2 < n) n2 <<= 1;
          warp_sort_desc(sh, n2);
          float mass;
          const int n_keep = warp_nucleus_run(sh, n, m, Z, head, rank, a.top_p, a.min_keep, &mass);
          if (n_keep > 0) last = sh.key[n_keep - 1];
          if (n_keep < n || !more) break;              // the boundary lies inside this run, or nothing is left below it
          head += mass; rank += n;
          if (!(head < a.top_p || rank < a.min_keep)) break;
          last = lo;
          const float p = expf(ford_inv(lo) - m) / Z;
          for (int i = 0; i < n_eq; ++i) head += p;
          rank += n_eq;
          upper = lo;
        }
        cut = ford_inv(last);
      }
    }
  }
  if (tid == 0) a.cutoff[r] = cut;
}

__global__ __launch_bounds__(kScanThreads) void row_warp_cutoff_kernel(WarpCutArgs a) { row_warp_cutoff_body(a, blockIdx.x); }
__global__ __launch_bounds__(kScanThreads) void row_warp_cutoff_multi_kernel(const WarpCutArgs* __restrict__ args) {
  __shared__ WarpCutArgs a;                        // grid column = job
  load_args(a, args + blockIdx.y);
  int rows = 0;
  for (int s2 = 0; s2 < a.n_seg; ++s2) rows += a.seg[s2].n;
  if ((int)blockIdx.x < rows) row_warp_cutoff_body(a, blockIdx.x);
}

// ---------------------------------------------------------------------------- beam step
__device__ void beam_step_body(const BeamStepArgs& a) {
  __shared__ ExpandShared sh;
  __shared__ int parents[MAXB];
  const int tid = threadIdx.x;
  if (tid == 0) sh.status = 0;
  if (tid < a.n_src) {
    sh.node[tid] = a.src.node ? a.src.node[tid] : 0;
    sh.brow[tid] = tid;
    sh.lrow[tid] = tid;
    sh.bscore[tid] = a.src.score[tid];
  }
  __syncthreads();
  Pick pk;
  if (a.sample) {                                                        // beamSD.py:65-75
    CandRegs cr;
    const int total = expand_candidates(sh, a.n_src, a.logits, a.ld, a.lse, a.fsm, a.temperature, a.cutoff, cr);
    if (a.tab_score) {                                                   // the draft's whole distribution, for verify
      const float L = block_lse(sh, cr.sc);
#pragma unroll
      for (int i = 0; i < kCPT; ++i) { int c = tid + i * kScanThreads; if (c < total) a.tab_score[c] = cr.sc[i]; }
      if (tid <= a.n_src) a.tab_off[tid] = sh.off[tid];
      if (tid == 0) *a.tab_lse = L;
    }
    sample_topn(sh, cr, cr.sc, a.k, a.rng_sub);
    if (tid < a.k) {
      pk = pick_of_flat(flat_of_key(sh.topk.sel[tid]), a.fsm, sh, a.n_src, a.logits, a.ld, a.temperature);
      parents[tid] = pk.parent;
    }
  } else {
    expand_and_select(sh, a.n_src, a.logits, a.ld, a.lse, a.fsm, a.k, a.row_cand, a.n_row_cand);
    if (tid < a.k) {
      pk = decode_pick(sh.topk.sel[tid], a.fsm, sh.brow, sh.node, a.n_src);
      parents[tid] = pk.parent;
    }
  }
  __syncthreads();
  int slot = tid;
  if (a.filter_ids) {
    // beamSD.py:80-86: picks whose token is neither an item code (>= 32000) nor EOS (2) are dropped AFTER the top-k, so the
    // beam set shrinks instead of lower-ranked candidates moving up; the survivors keep their order (stable compaction),
    // the freed slots hold "no beam" (flat = -1) at the end of the block
    __shared__ int keep[MAXB];
    const bool had = tid < a.k && pk.flat >= 0;
    const bool ok = had && (pk.tok >= a.fsm.filter_min || pk.tok == a.fsm.filter_eos);     // reference: tok >= 32000 | tok == 2
    if (tid < MAXB) keep[tid] = ok ? 1 : 0;
    const int n_had = __syncthreads_count(had);
    if (tid == 0) {
      int total = 0;
      for (int j = 0; j < a.k; ++j) total += keep[j];
      // every pick dropped: the reference goes on with an empty beam set and fails in the next forward (quirk 6); say what happened
      if (n_had > 0 && total == 0) sh.status = ATSPEED_ERR_FILTERED;
    }
    if (tid < a.k) {
      int before = 0, total = 0;
      for (int j = 0; j < a.k; ++j) { total += keep[j]; before += (j < tid) ? keep[j] : 0; }
      slot = ok ? before : total + (tid - before);
      if (!ok) pk = no_pick();
    }
    __syncthreads();
    if (tid < a.k) parents[slot] = pk.parent;
    __syncthreads();
  }
  emit_block(pk, slot, a.k, a.src, a.gen_len, a.dst, a.emit != 0, a.in, a.in_row0, a.out, a.out_row0, a.out_slot0);
  if (a.emit) emit_vis(parents, a.k, a.in, a.in_row0, a.out, a.out_row0, a.out_slot0, a.vis_words);
  if (a.mail) {
    int valid = __syncthreads_count(tid < a.k && pk.flat >= 0);
    if (tid == 0) {
      if (sh.status != 0) a.mail->status = sh.status;
      a.mail->n_valid = valid;
    }
  }
}

__global__ __launch_bounds__(kScanThreads) void beam_step_kernel(BeamStepArgs a) { beam_step_body(a); }
__global__ __launch_bounds__(kScanThreads) void beam_step_multi_kernel(const BeamStepArgs* __restrict__ args) {
  __shared__ BeamStepArgs a;                       // one workgroup per user
  load_args(a, args + blockIdx.x);
  beam_step_body(a);
}

// ---------------------------------------------------------------------------- verify
// What the two walks share.  Step i of a walk expands the round beams (i == 0, rows 0 .. nb of the logits) or the k beams that matched the
// draft's block i: hit[] = a beam's position in that block, sbh[] = its score, and its logits row is blk_row0[i] + hit (a packed walk,
// sampled ones always: blk_row0 = 0, nb, nb + dk, ...).
__device__ __forceinline__ void verify_step_rows(ExpandShared& sh, const VerifyArgs& a, int i, int n_rows, const int* hit, const float* sbh) {
  const int tid = threadIdx.x;
  __syncthreads();
  if (tid < n_rows) {                                                    // beamSD.py:279-296
    int br = i == 0 ? tid : hit[tid];
    sh.brow[tid] = br;
    sh.node[tid] = a.blk[i].node[br];
    sh.lrow[tid] = a.blk_row0[i] + br;
    sh.bscore[tid] = i == 0 ? a.blk[0].score[tid] : sbh[tid];
  }
  __syncthreads();
}

// Outputs of a walk that accepted nm draft blocks: thread j < k holds pick j of the new round beams (parents, in the row space of block nm,
// in t_parent).  Writes the beams, the next round's target inputs, the draft's re-ingest inputs and the mailbox (beamSD.py:383-416).
__device__ __forceinline__ void verify_outputs(const VerifyArgs& a, const ExpandShared& sh, const Pick& pk, const int* t_parent, int nm) {
  const int tid = threadIdx.x;
  const int k = a.k, dk = a.dk;
  __syncthreads();
  const int cnt = nm == 0 ? a.nb : dk;
  const int rowbase = nm == 0 ? a.n0 - a.nb : a.n0 + (nm - 1) * dk;
  const int base_next = a.cur.slot[rowbase] + cnt;
  const int W = a.vis_words;
  emit_block(pk, tid, k, a.blk[nm], a.gen_len0 + nm, a.res, true, a.cur, rowbase, a.next, 0, base_next);
  emit_vis(t_parent, k, a.cur, rowbase, a.next, 0, base_next, W);
  if (nm == a.dl && a.dl > 0) {
    // the draft has not seen its own last block: next draft input = that block ++ the new beams (:402-416)
    for (int j = tid; j < dk; j += blockDim.x) {
      a.dnext.ids[j] = a.cur.ids[rowbase + j];
      a.dnext.pos[j] = a.cur.pos[rowbase + j];
      a.dnext.slot[j] = a.cur.slot[rowbase + j];
    }
    for (int idx = tid; idx < dk * W; idx += blockDim.x) a.dnext.vis[idx] = a.cur.vis[(size_t)rowbase * W + idx];
    emit_block(pk, tid, k, a.blk[nm], a.gen_len0 + nm, a.res, true, a.cur, rowbase, a.dnext, dk, base_next);
    emit_vis(t_parent, k, a.cur, rowbase, a.dnext, dk, base_next, W);
  }
  int valid = __syncthreads_count(tid < k && pk.flat >= 0);
  if (tid == 0) {
    a.mail->n_matches = nm;
    a.mail->n_valid = valid;
    if (sh.status != 0) a.mail->status = sh.status;
  }
}

// Sampling verification (beamSD.py:293-321 distributions, :332-369 accept / resample, :303-309 bonus draw), one launch for
// all steps.  Per step i: p = softmax over (hit beams x allowed tokens) of the target's tempered cumulative scores, q the
// draft's (kept by its step kernel: tab_*); draft candidate j is accepted iff u_j q_j <= p_j; with >= K accepted, K of them
// (the K smallest hashes) become the next beams in ascending flat-id order and the walk goes on; otherwise the missing
// beams are drawn from max(p - q, 0) without the accepted ones and the walk stops.  All draws are counter-based
// (ats_rng_sub), so the CPU restatement (oracle/beamsd_sample_ref.py, HashRng) makes the same decisions.
__device__ void verify_sample_body(const VerifyArgs& a) {
  __shared__ ExpandShared sh;
  __shared__ int t_parent[MAXB], hit[MAXB], d_flat[MAXB], d_acc[MAXB], fin_flat[MAXB];
  __shared__ uint32_t d_h[MAXB];
  __shared__ float sbh[MAXB], d_sc[MAXB];
  const int tid = threadIdx.x;
  const int k = a.k, dk = a.dk;
  if (tid == 0) sh.status = 0;
  int nm = 0, n_rows_last = a.nb;
  Pick pk = no_pick();
  for (int i = 0; i <= a.dl; ++i) {
    const int n_rows = i == 0 ? a.nb : k;
    n_rows_last = n_rows;
    verify_step_rows(sh, a, i, n_rows, hit, sbh);
    CandRegs cr;
    expand_candidates(sh, n_rows, a.logits, a.ld, a.lse, a.fsm, a.temperature, a.cutoff, cr);
    if (i == a.dl) {                                                     // bonus draw from the target (:303-309)
      sample_topn(sh, cr, cr.sc, k, ats_rng_sub(a.seed, ATS_RNG_BONUS, a.round, i, 0));
      if (tid < k) fin_flat[tid] = flat_of_key(sh.topk.sel[tid]);
      __syncthreads();
      break;
    }
    const float Lt = block_lse(sh, cr.sc);
    const float Ld = *a.dtab_lse[i];
    // ---- accept test of the draft's candidates (:334-339)
    if (tid < MAXB) { d_flat[tid] = -1; d_acc[tid] = 0; d_sc[tid] = -INFINITY; d_h[tid] = 0; }
    __syncthreads();
    int acc = 0;
    if (tid < dk) {
      const int fl = a.blk[i + 1].flat[tid];
      d_flat[tid] = fl;
      if (fl >= 0) {
        Pick t = pick_of_flat(fl, a.fsm, sh, n_rows, a.logits, a.ld, a.temperature);
        const float p = t.score > -INFINITY ? expf(t.score - Lt) : 0.f;
        const float q = expf(a.blk[i + 1].score[tid] - Ld);
        const float u = ats_u01(ats_hash_u32((uint32_t)tid, ats_rng_sub(a.seed, ATS_RNG_ACCEPT, a.round, i, 0)));
        acc = (u * q <= p) ? 1 : 0;
        d_sc[tid] = t.score;
        d_h[tid] = ats_hash_u32((uint32_t)tid, ats_rng_sub(a.seed, ATS_RNG_PERM, a.round, i, 0));
      }
      d_acc[tid] = acc;
    }
    const int n_acc = __syncthreads_count(acc);
    if (n_acc >= k) {                                                    // :341-350
      int chosen = 0;
      if (tid < dk && acc) {
        int rank = 0;
        for (int j = 0; j < dk; ++j) rank += (d_acc[j] && (d_h[j] < d_h[tid] || (d_h[j] == d_h[tid] && j < tid))) ? 1 : 0;
        chosen = rank < k;
      }
      __syncthreads();
      if (tid < dk) d_acc[tid] = chosen;
      __syncthreads();
      if (tid < dk && chosen) {
        int rf = 0;
        for (int j = 0; j < dk; ++j) rf += (d_acc[j] && d_flat[j] < d_flat[tid]) ? 1 : 0;
        hit[rf] = tid;                 // position in the draft's block i+1
        sbh[rf] = d_sc[tid];
        fin_flat[rf] = d_flat[tid];
      }
      __syncthreads();
      nm += 1;
      continue;
    }
    // ---- rejected: the missing k - n_acc beams from the residual max(p - q, 0) without the accepted ones (:351-369)
    float logw[kCPT], pr[kCPT];
    float part = 0.f;
    const float* dts = a.dtab_score[i];
    const int* dto = a.dtab_off[i];
#pragma unroll
    for (int s2 = 0; s2 < kCPT; ++s2) {
      logw[s2] = -INFINITY; pr[s2] = 0.f;
      const int fl = cr.flat[s2];
      if (fl >= 0 && cr.sc[s2] > -INFINITY) {
        const Cand cd = cand_at(sh, n_rows, tid + s2 * kScanThreads);
        const float q = expf(dts[dto[sh.brow[cd.r]] + cd.j] - Ld);             // same node -> same children order in the draft's table
        const float p = expf(cr.sc[s2] - Lt);
        bool taken = false;
        for (int j = 0; j < dk; ++j) taken |= (d_acc[j] && d_flat[j] == fl);
        if (!taken) {
          pr[s2] = p;
          const float rsd = fmaxf(p - q, 0.f);
          if (rsd > 0.f) { logw[s2] = logf(rsd); part += rsd; }
        }
      }
    }
    const float tot = block_sum(part, sh.red_s);                         // red_s is free: block_lse ends in a barrier behind its last read
    if (tot == 0.f) {
#pragma unroll
      for (int s2 = 0; s2 < kCPT; ++s2) logw[s2] = pr[s2] > 0.f ? logf(pr[s2]) : -INFINITY;
    }
    sample_topn(sh, cr, logw, k - n_acc, ats_rng_sub(a.seed, ATS_RNG_RESID, a.round, i, 0));
    // final set = accepted ++ drawn, ascending flat id
    if (tid < dk && acc) {
      int r0 = 0;
      for (int j = 0; j < tid; ++j) r0 += d_acc[j];
      hit[r0] = d_flat[tid];                                           // scratch: unsorted flats
    }
    if (tid < k - n_acc) {
      const int fl = flat_of_key(sh.topk.sel[tid]);
      hit[n_acc + tid] = fl < 0 ? 0x7fffffff : fl;                     // "none" sorts last
    }
    __syncthreads();
    if (tid < k) {
      const int fl = hit[tid];
      int rf = 0;
      for (int j = 0; j < k; ++j) rf += (hit[j] < fl || (hit[j] == fl && j < tid)) ? 1 : 0;
      fin_flat[rf] = fl == 0x7fffffff ? -1 : fl;
    }
    __syncthreads();
    break;
  }
  // picks of the final set, in the row space of block nm (sh.* still describe the expand of the last step)
  if (tid < k) {
    pk = pick_of_flat(fin_flat[tid], a.fsm, sh, n_rows_last, a.logits, a.ld, a.temperature);
    t_parent[tid] = pk.parent;
  }
  verify_outputs(a, sh, pk, t_parent, nm);
}

// Greedy verification: the target's k best of every step must all be among the draft's dk of the next block (beamSD.py:279-298, :323-330, :371-380)
__device__ void verify_walk_body(const VerifyArgs& a) {
  __shared__ ExpandShared sh;
  __shared__ int t_parent[MAXB], t_pos[MAXB], hit[MAXB];
  __shared__ float sbh[MAXB];
  __shared__ int reject;
  const int tid = threadIdx.x;
  const int k = a.k, dk = a.dk;
  if (tid == 0) { sh.status = 0; reject = 0; }
  int nm = 0;
  Pick pk = no_pick();
  for (int i = 0; i <= a.dl; ++i) {
    // staged verification: block i's rows come with a later forward.  Nothing has been written yet (the trace's picks are rewritten by the
    // walk that finishes, which starts from step 0 again and so takes every decision exactly as the one-forward round does)
    if (i >= a.blocks_ready) {                                           // uniform
      if (tid == 0) { a.mail->n_matches = ATS_WALK_PENDING; if (sh.status != 0) a.mail->status = sh.status; }
      return;
    }
    const int n_rows = i == 0 ? a.nb : k;
    verify_step_rows(sh, a, i, n_rows, hit, sbh);
    expand_and_select(sh, n_rows, a.logits, a.ld, a.lse, a.fsm, k, a.row_cand, a.n_row_cand);     // :297-298,323-328
    if (tid < k) {
      pk = decode_pick(sh.topk.sel[tid], a.fsm, sh.brow, sh.node, n_rows);
      t_parent[tid] = pk.parent;
      if (a.vtrace) {                                                    // decision trace: what the target chose at step i
        int32_t* vt = a.vtrace + (size_t)i * 3 * MAXB;
        vt[tid] = (int32_t)__float_as_uint(pk.score); vt[MAXB + tid] = pk.parent; vt[2 * MAXB + tid] = pk.flat >= 0 ? pk.tok : -1;
      }
    }
    if (i == a.dl) break;                                                // :329-330 (uniform)
    // acceptance: every target id must be among the draft's ids of step i+1 (:371-380)
    int pos = -1;
    if (tid < k && pk.flat >= 0) {
      const int* df = a.blk[i + 1].flat;
      for (int d = 0; d < dk; ++d) if (df[d] == pk.flat) { pos = d; break; }
    }
    if (tid < k) { t_pos[tid] = pos; if (pos < 0) atomicOr(&reject, 1); }
    __syncthreads();
    if (reject) break;                                                   // uniform
    if (tid < k) {                                                       // :373-376: order by draft position
      int rank = 0;
      for (int j = 0; j < k; ++j) rank += (t_pos[j] < pos) ? 1 : 0;
      hit[rank] = pos;
      sbh[rank] = pk.score;
    }
    nm += 1;
  }
  verify_outputs(a, sh, pk, t_parent, nm);
}

__global__ __launch_bounds__(kScanThreads) void verify_walk_multi_kernel(const VerifyArgs* __restrict__ args) {
  __shared__ VerifyArgs a;
  load_args(a, args + blockIdx.x);
  if (a.sample) verify_sample_body(a); else verify_walk_body(a);
}

// ---------------------------------------------------------------------------- prompt init / export / accept
// row i of the token buffer = prompt token t = lp + i (lp = the length of a prompt prefix whose K / V are already in the user's arenas, 0 = none)
__device__ __forceinline__ void init_prompt_row(const TokBuf& tb, const int32_t* __restrict__ prompt, int i, int lp, int W, int vocab) {
  const int t = lp + i;
  int id = prompt[t];
  tb.ids[i] = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
  tb.pos[i] = t;
  tb.slot[i] = t;
  for (int w = 0; w < W; ++w) {                         // causal prefix: bits [0, t]
    int lo = w * 64;
    uint64_t bits = (t >= lo + 63) ? ~0ull : (t < lo ? 0ull : ((~0ull) >> (63 - (t - lo))));
    tb.vis[(size_t)i * W + w] = bits;
  }
}
// does prompt[0 .. lp) differ from the prefix's own ids?  Workgroup 0 alone asks (its thread 0 writes the mailbox); lp == 0: no
__device__ __forceinline__ int prompt_prefix_differs(const int32_t* __restrict__ prompt, const int32_t* __restrict__ prefix_ids, int lp) {
  if (lp <= 0 || blockIdx.x != 0) return 0;
  int bad = 0;
  for (int i = threadIdx.x; i < lp; i += blockDim.x) bad |= prompt[i] != prefix_ids[i] ? 1 : 0;
  return __syncthreads_or(bad);
}
// a user whose prompt does not open with its prefix ends with ATSPEED_ERR_INVALID at the first read-back: `pad` keeps the finding whatever a
// later step writes into status
__device__ __forceinline__ void init_mailbox(Mailbox* mail, int differs) {
  mail->n_matches = 0; mail->status = differs ? ATSPEED_ERR_INVALID : 0; mail->n_valid = 1; mail->pad = differs;
}
__global__ void init_prompt_kernel(TokBuf tb, const int32_t* __restrict__ prompt, int P, int W, BeamSet beams,
                                   int start_node, int vocab, Mailbox* mail, int lp, const int32_t* __restrict__ prefix_ids) {
  int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < P - lp) init_prompt_row(tb, prompt, t, lp, W, vocab);
  const int differs = prompt_prefix_differs(prompt, prefix_ids, lp);
  if (t == 0) {
    beams.score[0] = 0.f; beams.node[0] = start_node; beams.parent[0] = 0; beams.tok[0] = 0; beams.flat[0] = 0;
    init_mailbox(mail, differs);
  }
}

// every user of a lock-step batch in ONE launch (grid.y = user): 256 launches per batch less than the per-user form
__global__ void init_prompt_multi_kernel(const InitPromptArgs* __restrict__ args, int W, int vocab) {
  const InitPromptArgs a = args[blockIdx.y];
  int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < a.prompt_len - a.lp) init_prompt_row(a.tb, a.prompt, t, a.lp, W, vocab);
  const int differs = prompt_prefix_differs(a.prompt, a.prefix_ids, a.lp);
  if (t == 0) {
    a.beams.score[0] = 0.f; a.beams.node[0] = a.start_node; a.beams.parent[0] = 0; a.beams.tok[0] = 0; a.beams.flat[0] = 0;
    init_mailbox(a.mail, differs);
  }
}

__device__ __forceinline__ void export_beams_row(const BeamSet& b, int j, int k, int max_new, int32_t* out_tokens, float* out_scores, int sort_desc) {
  int dst = j;
  if (sort_desc) {                                     // beamSD.py:529-531: stable sort by score, best first
    const float sj = b.score[j];
    dst = 0;
    for (int i = 0; i < k; ++i) { const float si = b.score[i]; dst += (si > sj || (si == sj && i < j)) ? 1 : 0; }
  }
  out_scores[dst] = b.score[j];
  for (int g = 0; g < max_new; ++g) out_tokens[dst * max_new + g] = b.seq[j * LMAX + g];
}
__global__ void export_beams_multi_kernel(const ExportBeamsArgs* __restrict__ args, int k, int max_new) {
  const ExportBeamsArgs a = args[blockIdx.x];
  if ((int)threadIdx.x < k) export_beams_row(a.b, threadIdx.x, k, max_new, a.out_tokens, a.out_scores, a.sort_desc);
}

// beam_sequence of every user of a batch (beamSD.py:87,383: prompt ++ generated suffix per beam, int64) in one launch:
// block (beam j, user u) writes row j of user u
__global__ void assemble_sequences_kernel(const int32_t* __restrict__ prompts, const int64_t* __restrict__ off, const int32_t* __restrict__ toks,
                                          int k, int L, int64_t* __restrict__ out) {
  const int u = blockIdx.y, j = blockIdx.x;
  const int64_t p0 = off[u];
  const int P = (int)(off[u + 1] - p0);
  int64_t* row = out + (int64_t)k * (p0 + (int64_t)u * L) + (int64_t)j * (P + L);
  for (int t = threadIdx.x; t < P; t += blockDim.x) row[t] = prompts[p0 + t];
  for (int t = threadIdx.x; t < L; t += blockDim.x) row[P + t] = toks[((size_t)u * k + j) * L + t];
}

__global__ void export_beams_kernel(BeamSet b, int k, int max_new, int32_t* out_tokens, float* out_scores, int sort_desc) {
  int j = threadIdx.x;
  if (j < k) export_beams_row(b, j, k, max_new, out_tokens, out_scores, sort_desc);
}

// out[r][c] = logits[r][c] - lse[r]: the log-softmax rows a host-side logits processor receives (beamSD.py:58 -> :62-64)
__global__ void log_softmax_rows_kernel(const float* __restrict__ logits, int ld, const float* __restrict__ lse, int vocab, float* __restrict__ out, int ld_out) {
  const float l = lse[blockIdx.y];
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c < vocab) out[(size_t)blockIdx.y * ld_out + c] = logits[(size_t)blockIdx.y * ld + c] - l;
}

__global__ void accept_kernel(const int32_t* __restrict__ tflat, const float* __restrict__ tscore, int k,
                              const int32_t* __restrict__ dflat, int dk, int32_t* hit, float* sbh, int32_t* accept) {
  __shared__ int t_pos[MAXB];
  int j = threadIdx.x;
  int pos = -1;
  if (j < k && tflat[j] >= 0)
    for (int d = 0; d < dk; ++d) if (dflat[d] == tflat[j]) { pos = d; break; }
  if (j < k) t_pos[j] = pos;
  int bad = __syncthreads_count(j < k && pos < 0);
  if (j == 0) *accept = bad == 0;
  if (j < k) { hit[j] = -1; sbh[j] = -INFINITY; }
  __syncthreads();
  if (bad == 0 && j < k) {
    int rank = 0;
    for (int i = 0; i < k; ++i) rank += t_pos[i] < pos ? 1 : 0;
    hit[rank] = pos;
    sbh[rank] = tscore[j];
  }
}

// ---------------------------------------------------------------------------- item filters: per-user node bitsets
// One workgroup per user (semantics: include/atspeed_hip.h "item filters").  Every pass strides over the user's sequences with uniform bounds
// and ends at a workgroup barrier.  Bits are set with vector atomics and read back with device-scope atomic loads (a plain load could be
// served from a line the vector cache fetched before another wave's atomic reached L2); an OR is idempotent and commutative, and every
// pass reads only what earlier passes finished, so the result does not depend on the order in which threads run.
constexpr int kMaskThreads = 256;
__device__ __forceinline__ void mask_set(uint32_t* bits, int node) { atomicOr(bits + (node >> 5), 1u << (node & 31)); }
__device__ __forceinline__ bool mask_get(const uint32_t* bits, int node) {
  return (__hip_atomic_load(bits + (node >> 5), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >> (node & 31)) & 1u;
}
__global__ __launch_bounds__(kMaskThreads) void node_masks_kernel(NodeMaskBuild b) {
  __shared__ int n_unknown, n_known;
  const int u = blockIdx.x, tid = threadIdx.x;
  const int s0 = b.user_off[u], s1 = b.user_off[u + 1], start = b.start[u];
  uint32_t* bits = b.bits + (size_t)u * b.words;
  uint32_t* kept = b.kept + (size_t)u * b.words;
  uint32_t* ends = b.ends + (size_t)u * b.words;
  const bool allow = b.mode == ATSPEED_MASK_ALLOW;
  if (tid == 0) { n_unknown = 0; n_known = 0; }
  __syncthreads();
  // walk: path[s][0 .. len] of a known sequence; its end node goes into B (block) or E (allow), its path nodes into K (allow)
  for (int s = s0 + tid; s < s1; s += kMaskThreads) {
    const int t0 = b.seq_off[s], L = b.seq_off[s + 1] - t0;          // 1 .. LMAX (checked by the host)
    int32_t* path = b.path + (size_t)s * (LMAX + 1);
    int node = start, d = 0;
    path[0] = node;
    for (; d < L; ++d) {
      const int e = find_edge(b.fsm, node, b.seq_tok[t0 + d]);
      if (e < 0) break;
      node = b.fsm.nxt[e];
      path[d + 1] = node;
    }
    const bool known = d == L;
    b.len[s] = known ? L : -1;
    if (!known) { atomicAdd(&n_unknown, 1); continue; }
    atomicAdd(&n_known, 1);
    if (allow) {
      for (int i = 0; i <= L; ++i) mask_set(kept, path[i]);
      mask_set(ends, node);
    } else {
      mask_set(bits, node);
    }
  }
  __threadfence();
  __syncthreads();
  if (allow) {
    // a child of a path node that is no end node, and not itself on a path, is blocked
    for (int s = s0 + tid; s < s1; s += kMaskThreads) {
      const int L = b.len[s];
      const int32_t* path = b.path + (size_t)s * (LMAX + 1);
      for (int d = 0; d < L; ++d) {
        const int node = path[d];
        if (mask_get(ends, node)) continue;
        for (int e = b.fsm.row_ptr[node]; e < b.fsm.row_ptr[node + 1]; ++e) {
          const int c = b.fsm.nxt[e];
          if (!mask_get(kept, c)) mask_set(bits, c);
        }
      }
    }
  } else {
    // closure, deepest ancestors first: a path node all of whose children are blocked is blocked (below the start node the automaton is a
    // tree, so the children of a depth-d node were settled by pass d + 1)
    for (int d = LMAX - 1; d >= 0; --d) {
      for (int s = s0 + tid; s < s1; s += kMaskThreads) {
        if (b.len[s] <= d) continue;
        const int node = b.path[(size_t)s * (LMAX + 1) + d];
        bool all = true;
        for (int e = b.fsm.row_ptr[node]; e < b.fsm.row_ptr[node + 1] && all; ++e) all = mask_get(bits, b.fsm.nxt[e]);
        if (all) mask_set(bits, node);
      }
      __threadfence();
      __syncthreads();
    }
  }
  __threadfence();
  __syncthreads();
  if (tid == 0) {
    b.unknown[u] = n_unknown;
    b.status[u] = (allow ? n_known == 0 : mask_get(bits, start)) ? ATSPEED_ERR_CONSTRAINT : ATSPEED_OK;
  }
}

// ---------------------------------------------------------------------------- scoring candidates: prompt + prefix-sharing tree of an item list
// One workgroup per user (semantics: include/atspeed_hip.h "scoring candidates"; the scoring rule is beamSD.py:58-64).  The user's sequences
// are strictly ascending, so the sequences that share a prefix are neighbours and a prefix's row belongs to the first of them that goes on
// beyond it.  With lcp(s) = the tokens sequence s shares with its predecessor and e(s) = min(lcp(s), len(s - 1) - 1) -- the predecessor owns
// no row for its LAST token, so a sequence that continues its predecessor owns that depth itself --, token d of s gets a row iff
// e(s) <= d < len(s) - 1, rows are numbered P, P + 1, ... in (sequence, depth) order, and the row of prefix depth d < e(s) is that of the nearest
// s' < s with e(s') <= d.  The sequences are taken in passes of kTreeThreads; `carry` hands the owner of every depth to the next pass.  Rows are
// shared by PREFIX, never by automaton node: two prefixes that reach one node (a position-set automaton has one node per depth) see
// different tokens.  Every row's arrays are written whole by the thread that owns it, every write is bounded by the user's `cap`.
constexpr int kTreeThreads = 256;
__device__ __forceinline__ uint64_t low_bits_word(int n, int w) {          // word w of the bitset [0, n)
  const int k = n - 64 * w;
  return k >= 64 ? ~0ull : k <= 0 ? 0ull : (1ull << k) - 1ull;
}
__global__ __launch_bounds__(kTreeThreads) void score_tree_kernel(ScoreTreeBuild b) {
  __shared__ int sh_e[kTreeThreads], sh_base[kTreeThreads], sh_len[kTreeThreads], sh_scan[kTreeThreads];
  __shared__ int carry[LMAX];
  __shared__ int total, n_unknown, bad;
  const ScoreTreeUser u = b.users[blockIdx.x];
  const int tid = threadIdx.x, P = u.P, W = b.vis_words, cap = u.cap;
  if (tid == 0) { total = P; n_unknown = 0; bad = 0; }
  if (tid < LMAX) carry[tid] = -1;
  for (int r = tid; r < P && r < cap; r += kTreeThreads) {             // the prompt: causal
    u.ids[r] = u.prompt[r]; u.pos[r] = r; u.slot[r] = r;
    uint64_t* v = u.vis + (size_t)r * W;
    for (int w = 0; w < W; ++w) v[w] = low_bits_word(r + 1, w);
  }
  __syncthreads();
  auto seq_span = [&](int s, int* t0) {                                  // a sequence's tokens; 0 = offsets the token array does not hold
    const int a = b.seq_off[s], z = b.seq_off[s + 1];
    *t0 = a;
    return (a >= 0 && z > a && z - a <= LMAX && z <= b.n_tok) ? z - a : 0;
  };
  for (int c0 = u.s0; c0 < u.s1; c0 += kTreeThreads) {
    const int s = c0 + tid;
    const bool active = s < u.s1;
    int tk[LMAX], row[LMAX];
    int L = 0, e = 0, t0 = 0;
    if (active) {
      L = seq_span(s, &t0);
      if (L == 0) atomicOr(&bad, 1);
#pragma unroll
      for (int d = 0; d < LMAX; ++d) tk[d] = d < L ? b.seq_tok[t0 + d] : -1;
      if (s > u.s0 && L > 0) {
        int p0 = 0;
        const int Lp = seq_span(s - 1, &p0);
        int lcp = 0;
#pragma unroll
        for (int d = 0; d < LMAX; ++d) if (lcp == d && d < L && d < Lp && b.seq_tok[p0 + d] == tk[d]) lcp = d + 1;
        // strictly ascending: the predecessor is a proper prefix, or the first token that differs is larger here
        bool ok = Lp > 0 && (lcp == Lp ? L > Lp : lcp < L);
        if (ok && lcp < Lp) {
          int cur = 0;
#pragma unroll
          for (int d = 0; d < LMAX; ++d) if (d == lcp) cur = tk[d];
          ok = b.seq_tok[p0 + lcp] < cur;
        }
        if (!ok) atomicOr(&bad, 1);
        e = max(0, min(lcp, Lp - 1));
      }
      int node = u.start, d = 0;
      for (; d < L; ++d) {
        int cur = 0;
#pragma unroll
        for (int i = 0; i < LMAX; ++i) if (i == d) cur = tk[i];
        const int ed = find_edge(b.fsm, node, cur);
        if (ed < 0 || edge_blocked(b.fsm, ed)) break;
        node = b.fsm.nxt[ed];
      }
      const bool known = L > 0 && d == L;
      b.known[s] = known ? 1 : 0;
      if (!known) atomicAdd(&n_unknown, 1);
    }
    const int cnt = active ? max(0, L - 1 - e) : 0;
    sh_e[tid] = e; sh_len[tid] = L; sh_scan[tid] = cnt;
    __syncthreads();
    for (int off = 1; off < kTreeThreads; off <<= 1) {                  // inclusive prefix sum of the passes' new rows
      const int v = tid >= off ? sh_scan[tid - off] : 0;
      __syncthreads();
      sh_scan[tid] += v;
      __syncthreads();
    }
    const int base = total + sh_scan[tid] - cnt;
    sh_base[tid] = base;
    __syncthreads();
    if (active) {
      // the row of every prefix depth: own rows from e on, below it the nearest earlier sequence that is new at the depth
      int m = min(e, L - 1);
#pragma unroll
      for (int d = 0; d < LMAX; ++d) row[d] = (d >= e && d < L - 1) ? base + d - e : -1;
      for (int j = tid - 1; m > 0 && j >= 0; --j) {
        const int ej = sh_e[j];
        if (ej < m) {
#pragma unroll
          for (int d = 0; d < LMAX; ++d) if (d >= ej && d < m) row[d] = sh_base[j] + d - ej;
          m = ej;
        }
      }
#pragma unroll
      for (int d = 0; d < LMAX; ++d) if (d < m) row[d] = carry[d];
#pragma unroll
      for (int d = 0; d < LMAX; ++d) {
        const int r = row[d];
        if (d >= e && d < L - 1 && r >= 0 && r < cap) {
          u.ids[r] = tk[d]; u.pos[r] = P + d; u.slot[r] = r;
          uint64_t* v = u.vis + (size_t)r * W;
          for (int w = 0; w < W; ++w) {
            uint64_t word = low_bits_word(P, w);
#pragma unroll
            for (int a = 0; a < LMAX; ++a) {
              const int ra = row[a];
              if (a <= d && ra >= 0 && ra < cap && (ra >> 6) == w) word |= 1ull << (ra & 63);
            }
            v[w] = word;
          }
        }
      }
      int32_t* pr = b.pred_row + (size_t)s * LMAX;
#pragma unroll
      for (int d = 0; d < LMAX; ++d) pr[d] = d >= L ? -1 : d == 0 ? P - 1 : row[d - 1];
    }
    __syncthreads();
    // hand over: the owner of each depth as the next pass's first sequence sees it, and the rows so far
    const int n_act = min(kTreeThreads, u.s1 - c0);
    if (tid < LMAX) {
      for (int j = n_act - 1; j >= 0; --j)
        if (sh_e[j] <= tid) { carry[tid] = tid < sh_len[j] - 1 ? sh_base[j] + tid - sh_e[j] : -1; break; }
    }
    if (tid == n_act - 1) total = base + cnt;
    __syncthreads();
  }
  if (tid == 0) {
    b.n_rows[blockIdx.x] = total;
    b.unknown[blockIdx.x] = n_unknown;
    b.status[blockIdx.x] = bad ? ATSPEED_ERR_INVALID : total > cap ? ATSPEED_ERR_CAPACITY : ATSPEED_OK;
  }
}

// One thread per candidate: the sum of its tokens' log-probs in token order, each term formed by the beam expand's own rule (`tempered`,
// temperature 1) and added onto the running sum in fp32 as expand_candidates adds a beam's score.
__global__ void path_scores_kernel(const float* __restrict__ logits, int ld, const float* __restrict__ lse, int n_rows, int vocab,
                                   const int32_t* __restrict__ seq_tok, const int32_t* __restrict__ seq_off, const int32_t* __restrict__ pred_row,
                                   const int32_t* __restrict__ seq_base, const int32_t* __restrict__ known, int n_seq, float* __restrict__ scores) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n_seq) return;
  const int t0 = seq_off[s], L = seq_off[s + 1] - t0;
  bool ok = known[s] != 0 && L >= 1 && L <= LMAX;
  const long long base = seq_base ? seq_base[s] : 0;
  float sum = 0.f;
  for (int d = 0; ok && d < L; ++d) {
    const long long r = base + pred_row[(size_t)s * LMAX + d];
    const int tok = seq_tok[t0 + d];
    if (r < 0 || r >= n_rows || tok < 0 || tok >= vocab) { ok = false; break; }
    sum = sum + tempered(logits[(size_t)r * ld + tok], lse[r], 1.0f);
  }
  scores[s] = ok ? sum : -INFINITY;
}

}  // namespace

int ats_lse_rows(const float* logits, int n_rows, int vocab, int ld, float* lse, hipStream_t st) {
  if (n_rows <= 0) return ATSPEED_OK;
  ATS_REQUIRE((ld & 3) == 0 && ((uintptr_t)logits & 15) == 0, ATSPEED_ERR_INVALID, "lse: rows must be 16-byte aligned (ld %d)", ld);
  // measured (tools/lse_bench.py, 30976 rows of 32859): 1024 threads 6.2 TB/s, 512: 6.5, 256 (four double-buffered chunks per row, eight
  // workgroups per CU): 6.9 TB/s = 98 % of the measured read peak; a single user's 121 rows are launch-bound (6.0 us with 512 threads, 6.6 with 256)
  const int nt = n_rows >= 1024 ? 256 : 512;
  if (nt == 256) lse_rows_kernel<256><<<n_rows, 256, 0, st>>>(logits, vocab, ld, lse);
  else           lse_rows_kernel<512><<<n_rows, 512, 0, st>>>(logits, vocab, ld, lse);
  ATS_LAUNCH_CHECK();
  return ATSPEED_OK;
}

int ats_row_topk(const float* logits, int n_rows, int vocab, int ld, int kk, int32_t* out, hipStream_t st) {
  if (n_rows <= 0) return ATSPEED_OK;
  ATS_REQUIRE(kk >= 1 && kk <= MAXB, ATSPEED_ERR_CAPACITY, "row_topk: k=%d out of [1,%d]", kk, MAXB);
  row_topk_kernel<<<n_rows, kScanThreads, 0, st>>>(logits, vocab, ld, kk, out);
  ATS_LAUNCH_CHECK();
  return ATSPEED_OK;
}

std::atomic<long long> g_ats_warp_launches{0};

// ---- item filters (include/atspeed_hip.h): per-user node bitsets, built on the device where the automaton lives
int ats_node_masks_build(const NodeMaskBuild& b, int n_users, hipStream_t st) {
  if (n_users <= 0) return ATSPEED_OK;
  node_masks_kernel<<<n_users, kMaskThreads, 0, st>>>(b);
  ATS_LAUNCH_CHECK();
  return ATSPEED_OK;
}

extern "C" void atspeed_node_masks_destroy(atspeed_node_masks* m) {
  if (!m) return;
  hipFree(m->block);
  delete m;
}

extern "C" int atspeed_node_masks_create(const atspeed_fsm* fsm, int32_t n_users, const int32_t* start_nodes, const int32_t* seq_tokens,
                                         const int32_t* seq_offsets, const int32_t* user_seq_offsets, int32_t mode, int32_t* unknown_out,
                                         int32_t* status_out, void* stream, atspeed_node_masks** out) {
  ATS_REQUIRE(fsm && start_nodes && seq_offsets && user_seq_offsets && status_out && out, ATSPEED_ERR_INVALID, "node_masks_create: null argument");
  ATS_REQUIRE(fsm->dev.n_nodes > 0, ATSPEED_ERR_INVALID, "node_masks_create: a mask-free automaton has no nodes to filter");
  ATS_REQUIRE(n_users >= 1, ATSPEED_ERR_INVALID, "node_masks_create: %d users", n_users);
  ATS_REQUIRE(mode == ATSPEED_MASK_BLOCK || mode == ATSPEED_MASK_ALLOW, ATSPEED_ERR_INVALID, "node_masks_create: mode %d is neither ATSPEED_MASK_BLOCK nor ATSPEED_MASK_ALLOW", mode);
  ATS_REQUIRE(user_seq_offsets[0] == 0 && seq_offsets[0] == 0, ATSPEED_ERR_INVALID, "node_masks_create: offsets must start at 0");
  for (int u = 0; u < n_users; ++u) {
    ATS_REQUIRE(user_seq_offsets[u + 1] >= user_seq_offsets[u], ATSPEED_ERR_INVALID, "node_masks_create: user offsets not monotone at user %d", u);
    ATS_REQUIRE(start_nodes[u] >= 0 && start_nodes[u] < fsm->dev.n_nodes, ATSPEED_ERR_INVALID, "node_masks_create: start node of user %d out of range", u);
  }
  const int n_seq = user_seq_offsets[n_users];
  for (int s = 0; s < n_seq; ++s) {
    const int64_t len = (int64_t)seq_offsets[s + 1] - seq_offsets[s];
    ATS_REQUIRE(len >= 1, ATSPEED_ERR_INVALID, "node_masks_create: sequence %d is empty", s);
    ATS_REQUIRE(len <= LMAX, ATSPEED_ERR_INVALID, "node_masks_create: sequence %d holds %lld tokens (max %d)", s, (long long)len, LMAX);
  }
  const int n_tok = seq_offsets[n_seq];
  ATS_REQUIRE(n_tok == 0 || seq_tokens, ATSPEED_ERR_INVALID, "node_masks_create: null token array");
  hipStream_t st = (hipStream_t)stream;
  std::unique_ptr<atspeed_node_masks, void (*)(atspeed_node_masks*)> m(new atspeed_node_masks(), atspeed_node_masks_destroy);
  m->fsm = fsm; m->n_users = n_users; m->words = (fsm->dev.n_nodes + 31) / 32; m->bits = nullptr; m->block = nullptr;
  // one block: the bitsets, allow mode's two scratch sets, then the int32 arrays
  const size_t set_words = (size_t)n_users * m->words;
  const size_t n_sets = mode == ATSPEED_MASK_ALLOW ? 3 : 1;
  const size_t ints = (size_t)n_users /*start*/ + (size_t)std::max(n_tok, 1) + (size_t)(n_seq + 1) + (size_t)(n_users + 1) +
                      (size_t)std::max(n_seq, 1) * (LMAX + 1) /*path*/ + (size_t)std::max(n_seq, 1) /*len*/ + 2 * (size_t)n_users /*unknown, status*/;
  const size_t bytes = (n_sets * set_words + ints) * 4;
  ATS_HIP(hipMalloc(&m->block, bytes));
  ATS_HIP(hipMemsetAsync(m->block, 0, n_sets * set_words * 4, st));
  uint32_t* w = (uint32_t*)m->block;
  m->bits = w;
  NodeMaskBuild b{};
  b.fsm = fsm->dev; b.words = m->words; b.mode = mode;
  b.bits = w; w += set_words;
  b.kept = b.ends = b.bits;                      // block mode never touches them
  if (mode == ATSPEED_MASK_ALLOW) { b.kept = w; w += set_words; b.ends = w; w += set_words; }
  int32_t* p = (int32_t*)w;
  int32_t* d_start = p; p += n_users;
  int32_t* d_tok = p; p += std::max(n_tok, 1);
  int32_t* d_soff = p; p += n_seq + 1;
  int32_t* d_uoff = p; p += n_users + 1;
  b.path = p; p += (size_t)std::max(n_seq, 1) * (LMAX + 1);
  b.len = p; p += std::max(n_seq, 1);
  b.unknown = p; p += n_users;
  b.status = p; p += n_users;
  b.start = d_start; b.seq_tok = d_tok; b.seq_off = d_soff; b.user_off = d_uoff;
  ATS_HIP(hipMemcpyAsync(d_start, start_nodes, sizeof(int32_t) * n_users, hipMemcpyHostToDevice, st));
  if (n_tok > 0) ATS_HIP(hipMemcpyAsync(d_tok, seq_tokens, sizeof(int32_t) * n_tok, hipMemcpyHostToDevice, st));
  ATS_HIP(hipMemcpyAsync(d_soff, seq_offsets, sizeof(int32_t) * (n_seq + 1), hipMemcpyHostToDevice, st));
  ATS_HIP(hipMemcpyAsync(d_uoff, user_seq_offsets, sizeof(int32_t) * (n_users + 1), hipMemcpyHostToDevice, st));
  ATS_TRY(ats_node_masks_build(b, n_users, st));
  ATS_HIP(hipMemcpyAsync(status_out, b.status, sizeof(int32_t) * n_users, hipMemcpyDeviceToHost, st));
  if (unknown_out) ATS_HIP(hipMemcpyAsync(unknown_out, b.unknown, sizeof(int32_t) * n_users, hipMemcpyDeviceToHost, st));
  ATS_HIP(hipStreamSynchronize(st));
  *out = m.release();
  return ATSPEED_OK;
}

extern "C" int atspeed_node_masks_read(const atspeed_node_masks* m, int32_t user, uint32_t* words_out, int32_t n_words) {
  ATS_REQUIRE(m && words_out, ATSPEED_ERR_INVALID, "node_masks_read: null argument");
  ATS_REQUIRE(user >= 0 && user < m->n_users, ATSPEED_ERR_INVALID, "node_masks_read: user %d out of [0, %d)", user, m->n_users);
  ATS_REQUIRE(n_words == m->words, ATSPEED_ERR_INVALID, "node_masks_read: a user's bitset holds %d words, not %d", m->words, n_words);
  ATS_HIP(hipMemcpy(words_out, ats_mask_bits(m, user), sizeof(uint32_t) * m->words, hipMemcpyDeviceToHost));
  return ATSPEED_OK;
}

// ---- scoring candidates (include/atspeed_hip.h): the tree builder and the path-score kernel
int ats_score_tree_build(const ScoreTreeBuild& b, int n_users, hipStream_t st) {
  if (n_users <= 0) return ATSPEED_OK;
  score_tree_kernel<<<n_users, kTreeThreads, 0, st>>>(b);
  ATS_LAUNCH_CHECK();
  return ATSPEED_OK;
}

int ats_path_scores(const float* logits, int ld, const float* lse, int n_rows, int vocab, const int32_t* seq_tok, const int32_t* seq_off,
                    const int32_t* pred_row, const int32_t* seq_base, const int32_t* known, int n_seq, float* scores, hipStream_t st) {
  if (n_seq <= 0) return ATSPEED_OK;
  path_scores_kernel<<<(n_seq + 255) / 256, 256, 0, st>>>(logits, ld, lse, n_rows, vocab, seq_tok, seq_off, pred_row, seq_base, known, n_seq, scores);
  ATS_LAUNCH_CHECK();
  return ATSPEED_OK;
}

extern "C" int atspeed_score_tree_build(const atspeed_fsm* fsm, int32_t n_users, const int32_t* const* prompt_ids, const int32_t* prompt_len,
                                        const int32_t* start_nodes, const int32_t* seq_tokens, int32_t n_seq_tokens, const int32_t* seq_offsets,
                                        const int32_t* user_seq_offsets, int32_t max_slots, const int32_t* row_offsets, int32_t* ids, int32_t* pos,
                                        int32_t* slots, uint64_t* vis, int32_t* pred_row, int32_t* known, int32_t* n_rows, int32_t* unknown,
                                        int32_t* status, void* stream) {
  ATS_REQUIRE(fsm && prompt_ids && prompt_len && start_nodes && seq_tokens && seq_offsets && user_seq_offsets && row_offsets && ids && pos && slots &&
              vis && pred_row && known && n_rows && unknown && status, ATSPEED_ERR_INVALID, "score_tree_build: null argument");
  ATS_REQUIRE(fsm->dev.n_nodes > 0, ATSPEED_ERR_INVALID, "score_tree_build: a mask-free automaton knows no items");
  ATS_REQUIRE(n_users >= 1 && n_users <= ATS_MAX_SEGS, ATSPEED_ERR_CAPACITY, "score_tree_build: %d users per call (1 .. %d)", n_users, ATS_MAX_SEGS);
  ATS_REQUIRE(max_slots >= 64 && max_slots % 64 == 0 && n_seq_tokens >= 1, ATSPEED_ERR_INVALID, "score_tree_build: max_slots %d must be a positive multiple of 64, and there must be tokens", max_slots);
  ATS_REQUIRE(user_seq_offsets[0] == 0 && row_offsets[0] == 0, ATSPEED_ERR_INVALID, "score_tree_build: offsets must start at 0");
  std::vector<ScoreTreeUser> users((size_t)n_users);
  const int W = max_slots / 64;
  for (int u = 0; u < n_users; ++u) {
    ATS_REQUIRE(user_seq_offsets[u + 1] > user_seq_offsets[u], ATSPEED_ERR_INVALID, "score_tree_build: user %d has no sequence", u);
    ATS_REQUIRE(row_offsets[u + 1] >= row_offsets[u], ATSPEED_ERR_INVALID, "score_tree_build: row offsets not monotone at user %d", u);
    ATS_REQUIRE(prompt_ids[u] && prompt_len[u] >= 1, ATSPEED_ERR_INVALID, "score_tree_build: user %d has no prompt", u);
    ATS_REQUIRE(start_nodes[u] >= 0 && start_nodes[u] < fsm->dev.n_nodes, ATSPEED_ERR_INVALID, "score_tree_build: start node of user %d out of range", u);
    ScoreTreeUser& su = users[u];
    const size_t r0 = (size_t)row_offsets[u];
    su.prompt = prompt_ids[u]; su.P = prompt_len[u]; su.start = start_nodes[u]; su.s0 = user_seq_offsets[u]; su.s1 = user_seq_offsets[u + 1];
    su.cap = std::min(row_offsets[u + 1] - row_offsets[u], max_slots); su.pad = 0;       // a row past max_slots has no visibility bit
    su.ids = ids + r0; su.pos = pos + r0; su.slot = slots + r0; su.vis = vis + r0 * W;
  }
  hipStream_t st = (hipStream_t)stream;
  ScoreTreeBuild b{};
  const void* d_users = nullptr;
  ATS_TRY(ats_stage(users.data(), users.size() * sizeof(ScoreTreeUser), &d_users, st));
  b.fsm = fsm->dev; b.users = (const ScoreTreeUser*)d_users; b.seq_tok = seq_tokens; b.seq_off = seq_offsets; b.n_tok = n_seq_tokens;
  b.pred_row = pred_row; b.known = known; b.n_rows = n_rows; b.unknown = unknown; b.status = status; b.vis_words = W;
  return ats_score_tree_build(b, n_users, st);
}

extern "C" int atspeed_path_scores(const float* logits, int32_t ld, const float* lse, int32_t n_rows, int32_t vocab, const int32_t* seq_tokens,
                                   const int32_t* seq_offsets, const int32_t* pred_row, const int32_t* seq_base, const int32_t* known, int32_t n_seqs,
                                   float* scores_out, void* stream) {
  ATS_REQUIRE(logits && lse && seq_tokens && seq_offsets && pred_row && known && scores_out, ATSPEED_ERR_INVALID, "path_scores: null argument");
  ATS_REQUIRE(n_rows >= 1 && vocab >= 1 && ld >= vocab && n_seqs >= 0, ATSPEED_ERR_INVALID, "path_scores: bad shape (rows %d, vocab %d, ld %d, sequences %d)",
              n_rows, vocab, ld, n_seqs);
  return ats_path_scores(logits, ld, lse, n_rows, vocab, seq_tokens, seq_offsets, pred_row, seq_base, known, n_seqs, scores_out, (hipStream_t)stream);
}

// the filter of `user` on a by-value copy of the automaton, for the bare kernel entries
static int masked_fsm(const atspeed_fsm* fsm, const atspeed_node_masks* masks, int user, const char* who, FsmDev* out) {
  *out = fsm->dev;
  if (!masks) return ATSPEED_OK;
  ATS_REQUIRE(masks->fsm == fsm, ATSPEED_ERR_INVALID, "%s: the masks were built on another automaton", who);
  ATS_REQUIRE(user >= 0 && user < masks->n_users, ATSPEED_ERR_INVALID, "%s: user %d out of [0, %d)", who, user, masks->n_users);
  out->blocked = ats_mask_bits(masks, user);
  return ATSPEED_OK;
}

static int warp_cut_check(const WarpCutArgs& a, int* rows_out) {
  ATS_REQUIRE(a.n_seg >= 1 && a.n_seg <= ATSPEED_MAX_GAMMA + 1 && a.fsm.n_nodes > 0, ATSPEED_ERR_INVALID, "warp cutoffs: need an automaton and 1..%d row segments",
              ATSPEED_MAX_GAMMA + 1);
  ATS_REQUIRE(a.temperature > 0.f && a.top_k >= 0 && a.top_p > 0.f && a.min_keep >= 1, ATSPEED_ERR_INVALID,
              "warp cutoffs: temperature %g / top_k %d / top_p %g / min_tokens_to_keep %d out of range", (double)a.temperature, a.top_k, (double)a.top_p, a.min_keep);
  int rows = 0;
  for (int s = 0; s < a.n_seg; ++s) { ATS_REQUIRE(a.seg[s].n >= 0, ATSPEED_ERR_INVALID, "warp cutoffs: negative row count"); rows += a.seg[s].n; }
  *rows_out = rows;
  return ATSPEED_OK;
}

int ats_row_warp_cutoff(const WarpCutArgs& a, hipStream_t st) {
  int rows = 0;
  ATS_TRY(warp_cut_check(a, &rows));
  if (rows == 0) return ATSPEED_OK;
  row_warp_cutoff_kernel<<<rows, kScanThreads, 0, st>>>(a);
  ATS_LAUNCH_CHECK();
  g_ats_warp_launches.fetch_add(1, std::memory_order_relaxed);
  return ATSPEED_OK;
}

int ats_row_warp_cutoff_multi(const WarpCutArgs* dev_args, int n, int max_rows, hipStream_t st) {
  if (n <= 0 || max_rows <= 0) return ATSPEED_OK;
  ATS_REQUIRE(n <= 65535, ATSPEED_ERR_CAPACITY, "warp cutoffs: %d jobs per launch (max 65535)", n);
  row_warp_cutoff_multi_kernel<<<dim3(max_rows, n), kScanThreads, 0, st>>>(dev_args);
  ATS_LAUNCH_CHECK();
  g_ats_warp_launches.fetch_add(1, std::memory_order_relaxed);
  return ATSPEED_OK;
}

extern "C" int64_t atspeed_warp_cutoff_launches(void) { return (int64_t)g_ats_warp_launches.load(std::memory_order_relaxed); }

extern "C" int atspeed_warp_cutoffs_masked(const float* logits, int32_t ld, const float* lse, int32_t n_rows, const atspeed_fsm* fsm, const int32_t* nodes,
                                           float temperature, int32_t top_k, float top_p, int32_t min_keep, float* cutoffs,
                                           const atspeed_node_masks* masks, int32_t user, void* stream) {
  ATS_REQUIRE(logits && lse && fsm && nodes && cutoffs && n_rows >= 0 && ld > 0, ATSPEED_ERR_INVALID, "warp_cutoffs: bad arguments");
  WarpCutArgs a{};
  a.seg[0] = WarpSeg{nodes, n_rows}; a.n_seg = 1;
  a.logits = logits; a.ld = ld; a.lse = lse;
  ATS_TRY(masked_fsm(fsm, masks, user, "warp_cutoffs_masked", &a.fsm));
  a.temperature = temperature; a.top_k = top_k; a.top_p = top_p; a.min_keep = min_keep; a.cutoff = cutoffs;
  return ats_row_warp_cutoff(a, (hipStream_t)stream);
}

extern "C" int atspeed_warp_cutoffs(const float* logits, int32_t ld, const float* lse, int32_t n_rows, const atspeed_fsm* fsm, const int32_t* nodes,
                                    float temperature, int32_t top_k, float top_p, int32_t min_keep, float* cutoffs, void* stream) {
  return atspeed_warp_cutoffs_masked(logits, ld, lse, n_rows, fsm, nodes, temperature, top_k, top_p, min_keep, cutoffs, nullptr, 0, stream);
}

int ats_beam_step(const BeamStepArgs& a, hipStream_t st) {
  ATS_REQUIRE(a.k >= 1 && a.k <= MAXB && a.n_src >= 1 && a.n_src <= MAXB, ATSPEED_ERR_CAPACITY,
              "beam step: k=%d / rows=%d exceed %d", a.k, a.n_src, MAXB);
  beam_step_kernel<<<1, kScanThreads, 0, st>>>(a);
  ATS_LAUNCH_CHECK();
  return ATSPEED_OK;
}

int ats_beam_step_multi(const BeamStepArgs* dev_args, int n, hipStream_t st) {
  if (n <= 0) return ATSPEED_OK;
  beam_step_multi_kernel<<<n, kScanThreads, 0, st>>>(dev_args);
  ATS_LAUNCH_CHECK();
  return ATSPEED_OK;
}

int ats_verify_walk_multi(const VerifyArgs* dev_args, int n, hipStream_t st) {
  if (n <= 0) return ATSPEED_OK;
  verify_walk_multi_kernel<<<n, kScanThreads, 0, st>>>(dev_args);
  ATS_LAUNCH_CHECK();
  return ATSPEED_OK;
}

int ats_init_prompt(TokBuf tb, const int32_t* prompt, int prompt_len, int vis_words, BeamSet beams, int start_node,
                    int vocab, Mailbox* mail, hipStream_t st, int lp, const int32_t* prefix_ids) {
  init_prompt_kernel<<<(prompt_len + 255) / 256, 256, 0, st>>>(tb, prompt, prompt_len, vis_words, beams, start_node, vocab, mail, lp, prefix_ids);
  ATS_LAUNCH_CHECK();
  return ATSPEED_OK;
}

int ats_init_prompt_multi(const InitPromptArgs* dev_args, int n, int max_prompt_len, int vis_words, int vocab, hipStream_t st) {
  if (n <= 0) return ATSPEED_OK;
  init_prompt_multi_kernel<<<dim3((max_prompt_len + 255) / 256, n), 256, 0, st>>>(dev_args, vis_words, vocab);
  ATS_LAUNCH_CHECK();
  return ATSPEED_OK;
}

int ats_export_beams_multi(const ExportBeamsArgs* dev_args, int n, int k, int max_new, hipStream_t st) {
  if (n <= 0) return ATSPEED_OK;
  export_beams_multi_kernel<<<n, 64, 0, st>>>(dev_args, k, max_new);
  ATS_LAUNCH_CHECK();
  return ATSPEED_OK;
}

extern "C" int atspeed_assemble_sequences(const int32_t* prompts_flat, const int64_t* prompt_off_host, const int32_t* toks, int32_t n, int32_t k,
                                          int32_t new_tokens, int64_t* out, void* stream) {
  ATS_REQUIRE(prompts_flat && prompt_off_host && toks && out && n >= 1 && k >= 1 && k <= 65535 && new_tokens >= 0, ATSPEED_ERR_INVALID,
              "assemble_sequences: bad arguments");
  ATS_REQUIRE(n <= 65535, ATSPEED_ERR_CAPACITY, "assemble_sequences: %d users per call (max 65535)", n);
  for (int u = 0; u < n; ++u)
    ATS_REQUIRE(prompt_off_host[u + 1] >= prompt_off_host[u], ATSPEED_ERR_INVALID, "assemble_sequences: offsets not monotone at user %d", u);
  const void* off_dev = nullptr;
  ATS_TRY(ats_stage(prompt_off_host, (size_t)(n + 1) * sizeof(int64_t), &off_dev, (hipStream_t)stream));
  assemble_sequences_kernel<<<dim3(k, n), 128, 0, (hipStream_t)stream>>>(prompts_flat, (const int64_t*)off_dev, toks, k, new_tokens, out);
  ATS_LAUNCH_CHECK();
  return ATSPEED_OK;
}

int ats_export_beams(BeamSet b, int k, int max_new, int32_t* out_tokens, float* out_scores, hipStream_t st, bool sort_desc) {
  export_beams_kernel<<<1, 64, 0, st>>>(b, k, max_new, out_tokens, out_scores, sort_desc ? 1 : 0);
  ATS_LAUNCH_CHECK();
  return ATSPEED_OK;
}

int ats_accept(const int32_t* target_flat, const float* target_score, int k, const int32_t* draft_flat, int dk,
               int32_t* hit, float* score_by_hit, int32_t* accept, hipStream_t st) {
  ATS_REQUIRE(k >= 1 && k <= MAXB && dk >= 1 && dk <= MAXB, ATSPEED_ERR_CAPACITY, "accept: k=%d dk=%d out of range", k, dk);
  accept_kernel<<<1, 64, 0, st>>>(target_flat, target_score, k, draft_flat, dk, hit, score_by_hit, accept);
  ATS_LAUNCH_CHECK();
  return ATSPEED_OK;
}

extern "C" int atspeed_lse_rows(const float* logits, int32_t n_rows, int32_t vocab, int32_t ld, float* lse, void* stream) {
  ATS_REQUIRE(logits && lse && vocab > 0 && ld >= vocab, ATSPEED_ERR_INVALID, "lse: bad arguments");
  return ats_lse_rows(logits, n_rows, vocab, ld, lse, (hipStream_t)stream);
}

extern "C" int atspeed_log_softmax_rows(const float* logits, int32_t ld, const float* lse, int32_t n_rows, int32_t vocab, float* out, int32_t ld_out,
                                        void* stream) {
  ATS_REQUIRE(logits && lse && out && vocab > 0 && ld >= vocab && ld_out >= vocab && n_rows >= 0 && n_rows <= 65535, ATSPEED_ERR_INVALID,
              "log_softmax_rows: bad arguments");
  if (n_rows == 0) return ATSPEED_OK;
  log_softmax_rows_kernel<<<dim3((vocab + 255) / 256, n_rows), 256, 0, (hipStream_t)stream>>>(logits, ld, lse, vocab, out, ld_out);
  ATS_LAUNCH_CHECK();
  return ATSPEED_OK;
}

extern "C" int atspeed_accept(const int32_t* target_flat, const float* target_score, int32_t k, const int32_t* draft_flat,
                              int32_t dk, int32_t* hit, float* score_by_hit, int32_t* accept, void* stream) {
  ATS_REQUIRE(target_flat && target_score && draft_flat && hit && score_by_hit && accept, ATSPEED_ERR_INVALID, "accept: null argument");
  return ats_accept(target_flat, target_score, k, draft_flat, dk, hit, score_by_hit, accept, (hipStream_t)stream);
}

extern "C" int atspeed_beam_expand_prune_masked(const float* logits, int32_t ld, const float* lse, const float* beam_score,
                                                const int32_t* beam_node, int32_t n_rows, const atspeed_fsm* fsm, int32_t k,
                                                float* out_score, int32_t* out_parent, int32_t* out_token, int32_t* out_node,
                                                int32_t* out_flat, const atspeed_node_masks* masks, int32_t user, void* stream) {
  ATS_REQUIRE(logits && lse && beam_score && beam_node && fsm && out_score && out_parent && out_token && out_node && out_flat,
              ATSPEED_ERR_INVALID, "beam_expand_prune: null argument");
  BeamStepArgs a{};
  a.src.score = const_cast<float*>(beam_score);
  a.src.node = const_cast<int32_t*>(beam_node);
  a.src.seq = nullptr;
  a.n_src = n_rows; a.gen_len = 0;
  a.logits = logits; a.ld = ld; a.lse = lse;
  ATS_TRY(masked_fsm(fsm, masks, user, "beam_expand_prune_masked", &a.fsm));
  a.k = k;
  a.dst.score = out_score; a.dst.parent = out_parent; a.dst.tok = out_token; a.dst.node = out_node; a.dst.flat = out_flat;
  a.dst.seq = nullptr;
  a.emit = 0; a.mail = nullptr; a.vis_words = 0;
  ATS_REQUIRE(fsm->dev.n_nodes > 0, ATSPEED_ERR_INVALID, "beam_expand_prune: a mask-free automaton needs atspeed_beam_expand_prune_free");
  return ats_beam_step(a, (hipStream_t)stream);
}

extern "C" int atspeed_beam_expand_prune(const float* logits, int32_t ld, const float* lse, const float* beam_score,
                                         const int32_t* beam_node, int32_t n_rows, const atspeed_fsm* fsm, int32_t k,
                                         float* out_score, int32_t* out_parent, int32_t* out_token, int32_t* out_node,
                                         int32_t* out_flat, void* stream) {
  return atspeed_beam_expand_prune_masked(logits, ld, lse, beam_score, beam_node, n_rows, fsm, k, out_score, out_parent, out_token, out_node, out_flat,
                                          nullptr, 0, stream);
}

// ---- the sampled step and the verify walks alone (tests): the argument blocks a round builds, from plain pointers.  Host code only
extern "C" int atspeed_beam_sample_step(const float* logits, int32_t ld, const float* lse, const float* beam_score, const int32_t* beam_node,
                                        int32_t n_rows, const atspeed_fsm* fsm, const atspeed_node_masks* masks, int32_t user, int32_t k,
                                        float temperature, uint32_t rng_sub, const float* cutoffs, int32_t filter_ids, float* out_score,
                                        int32_t* out_parent, int32_t* out_token, int32_t* out_node, int32_t* out_flat, float* tab_score,
                                        int32_t* tab_off, float* tab_lse, int32_t* mailbox, void* stream) {
  ATS_REQUIRE(logits && lse && beam_score && beam_node && fsm && out_score && out_parent && out_token && out_node && out_flat,
              ATSPEED_ERR_INVALID, "beam_sample_step: null argument");
  ATS_REQUIRE((tab_score && tab_off && tab_lse) || (!tab_score && !tab_off && !tab_lse), ATSPEED_ERR_INVALID,
              "beam_sample_step: the table is tab_score, tab_off and tab_lse together, or none of them");
  ATS_REQUIRE(ld > 0 && temperature > 0.f, ATSPEED_ERR_INVALID, "beam_sample_step: ld %d / temperature %g out of range", ld, (double)temperature);
  ATS_REQUIRE(fsm->dev.n_nodes > 0, ATSPEED_ERR_INVALID, "beam_sample_step: a sampled step needs an automaton with nodes");
  ATS_REQUIRE(k >= 1 && k <= MAXB && n_rows >= 1 && n_rows <= MAXB, ATSPEED_ERR_CAPACITY, "beam_sample_step: k=%d / rows=%d out of [1,%d]", k, n_rows, MAXB);
  BeamStepArgs a{};
  a.src.score = const_cast<float*>(beam_score);
  a.src.node = const_cast<int32_t*>(beam_node);
  a.n_src = n_rows; a.gen_len = 0;
  a.logits = logits; a.ld = ld; a.lse = lse;
  ATS_TRY(masked_fsm(fsm, masks, user, "beam_sample_step", &a.fsm));
  a.k = k;
  a.dst.score = out_score; a.dst.parent = out_parent; a.dst.tok = out_token; a.dst.node = out_node; a.dst.flat = out_flat;
  a.emit = 0; a.filter_ids = filter_ids ? 1 : 0; a.vis_words = 0;
  a.mail = reinterpret_cast<Mailbox*>(mailbox);
  a.sample = 1; a.temperature = temperature; a.rng_sub = rng_sub;
  a.tab_score = tab_score; a.tab_off = tab_off; a.tab_lse = tab_lse;
  a.cutoff = cutoffs;
  return ats_beam_step(a, (hipStream_t)stream);
}

static_assert(sizeof(Mailbox) == 4 * sizeof(int32_t), "atspeed_walk_args::mailbox is the four words of a Mailbox");

extern "C" int atspeed_verify_walk(const atspeed_walk_args* w, void* stream) {
  ATS_REQUIRE(w && w->struct_size == sizeof(atspeed_walk_args), ATSPEED_ERR_INVALID, "verify_walk: null argument block, or one of another size");
  ATS_REQUIRE(w->k >= 1 && w->k <= MAXB && w->dk >= 1 && w->dk <= MAXB && w->nb >= 1 && w->nb <= MAXB, ATSPEED_ERR_CAPACITY,
              "verify_walk: k=%d / dk=%d / nb=%d out of [1,%d]", w->k, w->dk, w->nb, MAXB);
  ATS_REQUIRE(w->dl >= 0 && w->dl <= ATSPEED_MAX_GAMMA, ATSPEED_ERR_CAPACITY, "verify_walk: %d draft blocks (0 .. %d)", w->dl, ATSPEED_MAX_GAMMA);
  ATS_REQUIRE(w->gen_len0 >= 0 && w->n0 >= w->nb && w->ld > 0 && w->vis_words >= 1 && w->blocks_ready >= 0 && w->blocks_ready <= w->dl + 1,
              ATSPEED_ERR_INVALID, "verify_walk: gen_len0 %d / n0 %d / ld %d / vis_words %d / blocks_ready %d out of range", w->gen_len0, w->n0, w->ld,
              w->vis_words, w->blocks_ready);
  ATS_REQUIRE(w->gen_len0 + w->dl <= LMAX, ATSPEED_ERR_CAPACITY, "verify_walk: %d tokens + %d blocks exceed the %d a suffix holds", w->gen_len0, w->dl, LMAX);
  ATS_REQUIRE(w->logits && w->lse && w->cur_ids && w->cur_pos && w->cur_slot && w->cur_vis && w->next_ids && w->next_pos && w->next_slot &&
              w->next_vis && w->dnext_ids && w->dnext_pos && w->dnext_slot && w->dnext_vis && w->res_score && w->res_parent && w->res_tok &&
              w->res_flat && w->mailbox, ATSPEED_ERR_INVALID, "verify_walk: null argument");
  for (int i = 0; i <= w->dl; ++i) {
    ATS_REQUIRE(w->blk_score[i] && w->blk_node[i] && (i == 0 || w->blk_flat[i]), ATSPEED_ERR_INVALID, "verify_walk: block %d lacks score, node or flat", i);
    ATS_REQUIRE(w->blk_row0[i] >= 0, ATSPEED_ERR_INVALID, "verify_walk: block %d starts at row %d", i, w->blk_row0[i]);
  }
  VerifyArgs a{};
  if (w->fsm) {
    ATS_TRY(masked_fsm(w->fsm, w->masks, w->user, "verify_walk", &a.fsm));
  } else {
    ATS_REQUIRE(!w->masks && w->vocab > 0 && (int64_t)MAXB * w->vocab < (int64_t)0x7fffffff, ATSPEED_ERR_INVALID, "verify_walk: no automaton and no usable vocabulary");
    a.fsm = FsmDev{nullptr, nullptr, nullptr, 0, 0, w->vocab, 0, -1, nullptr};
  }
  if (a.fsm.n_nodes == 0)
    ATS_REQUIRE(!w->sample && w->row_cand && w->n_row_cand >= 1 && w->n_row_cand <= MAXB, ATSPEED_ERR_INVALID,
                "verify_walk: the mask-free search is greedy and needs row_cand with 1 .. %d entries per row", MAXB);
  if (w->sample) {
    ATS_REQUIRE(w->temperature > 0.f, ATSPEED_ERR_INVALID, "verify_walk: temperature %g", (double)w->temperature);
    for (int i = 0; i < w->dl; ++i)
      ATS_REQUIRE(w->dtab_score[i] && w->dtab_off[i] && w->dtab_lse[i], ATSPEED_ERR_INVALID, "verify_walk: draft step %d has no table", i);
  }
  for (int i = 0; i <= w->dl; ++i) {
    a.blk[i].score = const_cast<float*>(w->blk_score[i]); a.blk[i].node = const_cast<int32_t*>(w->blk_node[i]);
    a.blk[i].flat = const_cast<int32_t*>(w->blk_flat[i]); a.blk[i].seq = const_cast<int32_t*>(w->blk_seq[i]);
    a.blk_row0[i] = w->blk_row0[i];
  }
  a.nb = w->nb; a.dl = w->dl; a.k = w->k; a.dk = w->dk; a.gen_len0 = w->gen_len0;
  a.logits = w->logits; a.ld = w->ld; a.lse = w->lse; a.blocks_ready = w->blocks_ready;
  a.cur = TokBuf{const_cast<int32_t*>(w->cur_ids), const_cast<int32_t*>(w->cur_pos), const_cast<int32_t*>(w->cur_slot), const_cast<uint64_t*>(w->cur_vis)};
  a.n0 = w->n0;
  a.next = TokBuf{w->next_ids, w->next_pos, w->next_slot, w->next_vis};
  a.dnext = TokBuf{w->dnext_ids, w->dnext_pos, w->dnext_slot, w->dnext_vis};
  a.vis_words = w->vis_words;
  a.res.score = w->res_score; a.res.node = w->res_node; a.res.seq = w->res_seq; a.res.parent = w->res_parent; a.res.tok = w->res_tok; a.res.flat = w->res_flat;
  a.mail = reinterpret_cast<Mailbox*>(w->mailbox);
  a.row_cand = w->row_cand; a.n_row_cand = w->n_row_cand;
  a.sample = w->sample ? 1 : 0; a.temperature = w->temperature; a.seed = w->seed; a.round = w->round;
  for (int i = 0; i < w->dl; ++i) { a.dtab_score[i] = w->dtab_score[i]; a.dtab_off[i] = w->dtab_off[i]; a.dtab_lse[i] = w->dtab_lse[i]; }
  a.cutoff = w->cutoff; a.vtrace = w->vtrace;
  hipStream_t st = (hipStream_t)stream;
  const void* dev = nullptr;
  ATS_TRY(ats_stage(&a, sizeof(a), &dev, st));
  return ats_verify_walk_multi((const VerifyArgs*)dev, 1, st);
}

extern "C" int atspeed_row_topk(const float* scores, int32_t n_rows, int32_t vocab, int32_t ld, int32_t k, int32_t* out_tokens, void* stream) {
  ATS_REQUIRE(scores && out_tokens && vocab > 0 && ld >= vocab && n_rows >= 0, ATSPEED_ERR_INVALID, "row_topk: bad arguments");
  return ats_row_topk(scores, n_rows, vocab, ld, k, out_tokens, (hipStream_t)stream);
}

extern "C" int atspeed_beam_expand_prune_free(const float* logits, int32_t ld, const float* lse, const float* beam_score, int32_t n_rows,
                                              int32_t vocab, int32_t k, int32_t* row_cand_ws, float* out_score, int32_t* out_parent,
                                              int32_t* out_token, int32_t* out_flat, void* stream) {
  ATS_REQUIRE(logits && lse && beam_score && row_cand_ws && out_score && out_parent && out_token && out_flat, ATSPEED_ERR_INVALID,
              "beam_expand_prune_free: null argument");
  ATS_REQUIRE(vocab > 0 && ld >= vocab && (int64_t)MAXB * vocab < (int64_t)0x7fffffff, ATSPEED_ERR_INVALID, "beam_expand_prune_free: bad vocabulary");
  ATS_REQUIRE(n_rows >= 1 && n_rows <= MAXB && k >= 1 && k <= MAXB, ATSPEED_ERR_CAPACITY, "beam_expand_prune_free: rows=%d / k=%d out of [1,%d] (row_cand_ws holds rows x %d ids)",
              n_rows, k, MAXB, MAXB);
  ATS_TRY(ats_row_topk(logits, n_rows, vocab, ld, k, row_cand_ws, (hipStream_t)stream));
  BeamStepArgs a{};
  a.src.score = const_cast<float*>(beam_score);
  a.src.node = nullptr; a.src.seq = nullptr;
  a.n_src = n_rows; a.gen_len = 0;
  a.logits = logits; a.ld = ld; a.lse = lse;
  a.fsm = FsmDev{nullptr, nullptr, nullptr, 0, 0, vocab, 0, -1};
  a.k = k;
  a.dst.score = out_score; a.dst.parent = out_parent; a.dst.tok = out_token; a.dst.node = nullptr; a.dst.flat = out_flat;
  a.dst.seq = nullptr;
  a.row_cand = row_cand_ws; a.n_row_cand = k;
  a.emit = 0; a.mail = nullptr; a.vis_words = 0;
  return ats_beam_step(a, (hipStream_t)stream);
}
