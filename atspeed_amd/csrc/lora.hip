// LoRA adapters kept OUT of the base weights (peft's unmerged forward, code/inference.py:86-100 of the reference): a 16-bit side path beside
// the q / k / v projections of a layer, whatever format the base runs in (16-bit, W8A8, W4A8).  Two kernels per layer:
//   lora_shrink    u = lora_A of the layer's normed input, for the three modules at once (stacked A_cat [3 R16][H]);
//   lora_rope_kv   the RoPE + KV-scatter pass with lora_B and the add in front (y = base + scaling * B u), per adapted module.
// R16 = the rank rounded up to 16: pad rows of A_cat / pad columns of B_m are zero, an absent module's rows of A_cat are zero and its B_m is
// NULL.  The arithmetic is common.h's "LoRA side path" (lora_u / lora_add).
// Every kernel exists once and takes the SOURCE of a row's adapter as a type (LoraOne / LoraBySeg below): a row's arithmetic -- the k
// partition, the order of every sum -- is the same text in both forms, so its result depends neither on the form, nor on the row's place in a
// 16-row tile, nor on what its neighbours name.
#include "internal.h"

namespace ATS_NS {

// ---------------------------------------------------------------------------- where a row's adapter comes from
// A source answers: which slot a row has (0 = none; by row, or by the row's segment where the caller has looked that up), that slot's record
// (all NULL for none), and where a row of u starts.
constexpr int LORA_U_LD = 3 * ATSPEED_LORA_MAX_RANK;

__device__ __forceinline__ int seg_adapter(const Seg& sg) { return sg.adapter > 0 && sg.adapter <= ATSPEED_LORA_MAX_ADAPTERS ? sg.adapter : 0; }

// one adapter for every row (the model-wide adapter, atspeed_lora_shrink / atspeed_segs_lora_rope_kv): u [T][3 R16].  The host has checked
// the record, the kernels do not.
struct LoraOne {
  atspeed_lora_slot s;
  static constexpr bool host_checked = true;
  __device__ __forceinline__ int seg_slot(const Seg&) const { return 1; }
  __device__ __forceinline__ int row_slot(const SegTable*, int) const { return 1; }
  __device__ __forceinline__ atspeed_lora_slot slot(int) const { return s; }
  template <typename P> __device__ __forceinline__ P u_row(P u, int row) const { return u + (size_t)row * 3 * s.r16; }
};

// several resident adapters, picked per row: seg_of_row -> Seg::adapter -> the model's slot table (entry 0 = none).  u has a fixed row stride
// of 3 x 64 elements; a row of slot 0 is neither written by the shrink nor read by the expand.
struct LoraBySeg {
  const atspeed_lora_slot* tab;
  static constexpr bool host_checked = false;
  __device__ __forceinline__ int seg_slot(const Seg& sg) const { return seg_adapter(sg); }
  __device__ __forceinline__ int row_slot(const SegTable* t, int row) const { return seg_slot(t->seg[seg_of_row(t, row)]); }
  __device__ __forceinline__ atspeed_lora_slot slot(int a) const { return a ? tab[a] : atspeed_lora_slot{}; }
  template <typename P> __device__ __forceinline__ P u_row(P u, int row) const { return u + (size_t)row * LORA_U_LD; }
};

// ---------------------------------------------------------------------------- shrink
// Any type, any hidden: one workgroup per token row; a row of slot 0 leaves at once.  The row's RMS statistic as rmsnorm_kernel takes it, xn
// re-formed per output (the fallback of shapes the MFMA kernel does not take, and the fp32 engine's kernel).  Wave w owns outputs w, w + 4,
// ...: fixed order, so two runs give the same bits.
template <typename T, typename L>
__global__ __launch_bounds__(256) void lora_shrink_kernel(const T* __restrict__ h, const T* __restrict__ nw, const L lora, T* __restrict__ u,
                                                          const SegTable* __restrict__ t, int hidden, float eps) {
  __shared__ float red[4];
  const int a = lora.row_slot(t, blockIdx.x);
  if (a == 0) return;
  const atspeed_lora_slot sl = lora.slot(a);
  const T* a_cat = (const T*)sl.a_cat;
  const int r3 = 3 * sl.r16;
  if (!L::host_checked && (!a_cat || r3 < 48 || r3 > LORA_U_LD)) return;
  const T* xr = h + (size_t)blockIdx.x * hidden;
  float ss = 0.f;
  for (int i = threadIdx.x; i < hidden; i += 256) { float v = Elt<T>::load(xr + i); ss += v * v; }
  const float rs = rsqrtf(block_sum(ss, red) / (float)hidden + eps);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int j = wave; j < r3; j += 4) {
    const T* ar = a_cat + (size_t)j * hidden;
    float acc = 0.f;
    for (int k = lane; k < hidden; k += 64) {
      const float xn = round_elt<T>(Elt<T>::load(nw + k) * norm_scale<T>(Elt<T>::load(xr + k), rs));
      acc = __fmaf_rn(xn, Elt<T>::load(ar + k), acc);
    }
    acc = wave_sum_f32(acc);
    if (lane == 0) Elt<T>::store(lora.u_row(u, blockIdx.x) + j, lora_u<T>(acc));
  }
}

// 16-bit, hidden % 128 == 0: a workgroup of four waves takes 16 token rows.  Lane l of a wave holds row l & 15, k-group l >> 4 of a 32-wide
// k-step -- its 16-byte load IS the MFMA A operand of v_mfma_f32_16x16x32 (after the norm), and the same load of A_cat row 16 t + (l & 15) the B
// operand of output tile t; acc[t][i] = u[row 4 (l >> 4) + i][16 t + (l & 15)].  Each wave sums a quarter of K; the prologue takes the rows'
// sums of squares, a pass re-reads the rows (L2 hits).  The waves' partial tiles meet in LDS and are added in wave order.
struct ShrinkRows {
  const bf16_t* xr;            // this lane's row
  int kq, k0;                  // this wave's quarter of K, this lane's 8 of every 32
  float rs;                    // the row's RMS factor
};

__device__ __forceinline__ ShrinkRows lora_shrink_rows(const bf16_t* __restrict__ h, int rows, int hidden, float eps, int lane, int wave,
                                                       float (*red)[16]) {
  const int r = lane & 15, g = lane >> 4;
  const int row = blockIdx.x * 16 + r;
  ShrinkRows w;
  w.xr = h + (size_t)(row < rows ? row : rows - 1) * hidden;                  // rows past the end: read the last row, store nothing
  w.kq = hidden >> 2, w.k0 = wave * w.kq + g * 8;
  float ss = 0.f;
  for (int k = 0; k < w.kq; k += 32) {
    const uint4 v = *reinterpret_cast<const uint4*>(w.xr + w.k0 + k);
    const bf16_t* e = reinterpret_cast<const bf16_t*>(&v);
#pragma unroll
    for (int j = 0; j < 8; ++j) { const float f = bf2f(e[j]); ss += f * f; }
  }
  ss += __shfl_xor(ss, 16, 64);
  ss += __shfl_xor(ss, 32, 64);
  if (g == 0) red[wave][r] = ss;
  __syncthreads();
  w.rs = rsqrtf((((red[0][r] + red[1][r]) + red[2][r]) + red[3][r]) / (float)hidden + eps);
  return w;
}

// one adapter's pass over a workgroup's 16 rows: the k-loop against this adapter's A_cat and the wave-order sum; only the rows whose bit is
// set in `mine` are stored, u_ld elements apart.  `part` [4][PT >= NT][64] is free again after the caller's next barrier.
template <int NT, int PT>
__device__ __forceinline__ void lora_shrink_pass(const ShrinkRows& w, const bf16_t* __restrict__ nw, const bf16_t* __restrict__ a_cat,
                                                 bf16_t* __restrict__ u, int u_ld, int rows, int hidden, int lane, int wave,
                                                 f32x4_t (*part)[PT][64], unsigned mine) {
  static_assert(NT <= PT, "the partial tiles do not fit");
  const bf16_t* xr = w.xr;
  const int kq = w.kq, k0 = w.k0;
  const float rs = w.rs;
  const int r = lane & 15, g = lane >> 4;
  f32x4_t acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  const bf16_t* ar = a_cat + (size_t)r * hidden + k0;
  for (int k = 0; k < kq; k += 32) {
    const uint4 xv = *reinterpret_cast<const uint4*>(xr + k0 + k);
    const uint4 wv = *reinterpret_cast<const uint4*>(nw + k0 + k);
    const bf16_t* xe = reinterpret_cast<const bf16_t*>(&xv);
    const bf16_t* we = reinterpret_cast<const bf16_t*>(&wv);
    uint4 xn;
    uint32_t* xw = reinterpret_cast<uint32_t*>(&xn);
#pragma unroll
    for (int j = 0; j < 8; j += 2)
      xw[j >> 1] = f2bf_pk(bf2f(we[j]) * norm_scale<bf16_t>(bf2f(xe[j]), rs), bf2f(we[j + 1]) * norm_scale<bf16_t>(bf2f(xe[j + 1]), rs));
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const uint4 av = *reinterpret_cast<const uint4*>(ar + (size_t)t * 16 * hidden + k);
      acc[t] = ATS_MFMA_16x16x32(__builtin_bit_cast(bf16x8_t, xn), __builtin_bit_cast(bf16x8_t, av), acc[t]);
    }
  }
#pragma unroll
  for (int t = 0; t < NT; ++t) part[wave][t][lane] = acc[t];
  __syncthreads();
  for (int t = wave; t < NT; t += 4) {
    const f32x4_t s = ((part[0][t][lane] + part[1][t][lane]) + part[2][t][lane]) + part[3][t][lane];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int lr = g * 4 + i, orow = blockIdx.x * 16 + lr;
      if (orow < rows && ((mine >> lr) & 1u)) u[(size_t)orow * u_ld + t * 16 + r] = f2bf(lora_u<bf16_t>(s[i]));
    }
  }
}

template <int NT>
__global__ __launch_bounds__(256) void lora_shrink_mfma_kernel(const bf16_t* __restrict__ h, const bf16_t* __restrict__ nw,
                                                               const bf16_t* __restrict__ a_cat, bf16_t* __restrict__ u, int rows, int hidden,
                                                               float eps) {
  __shared__ float red[4][16];
  __shared__ f32x4_t part[4][NT][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const ShrinkRows w = lora_shrink_rows(h, rows, hidden, eps, lane, wave, red);
  lora_shrink_pass<NT>(w, nw, a_cat, u, NT * 16, rows, hidden, lane, wave, part, 0xffffu);
}

// the same over rows of several adapters: the workgroup takes its 16 rows' RMS statistic once, then runs one pass per DISTINCT adapter among
// them (rows come grouped by segment: typically one or two) with that adapter's tile count.  Everything that steers the passes is uniform
// over the workgroup.
__global__ __launch_bounds__(256) void lora_shrink_segs_mfma_kernel(const bf16_t* __restrict__ h, const bf16_t* __restrict__ nw, const LoraBySeg lora,
                                                                    bf16_t* __restrict__ u, const SegTable* __restrict__ t, int hidden, float eps) {
  __shared__ float red[4][16];
  __shared__ int ad[16];
  __shared__ f32x4_t part[4][12][64];
  const int rows = t->total_tok;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (threadIdx.x < 16) {
    const int rr = blockIdx.x * 16 + threadIdx.x;
    ad[threadIdx.x] = rr < rows ? lora.row_slot(t, rr) : 0;
  }
  __syncthreads();
  int any = 0;
#pragma unroll
  for (int i = 0; i < 16; ++i) any |= ad[i];
  if (any == 0) return;                                                       // no row of this tile names an adapter
  const ShrinkRows w = lora_shrink_rows(h, rows, hidden, eps, lane, wave, red);
  for (int i = 0; i < 16; ++i) {
    const int a = ad[i];
    if (a == 0) continue;
    bool seen = false;
    unsigned mine = 0;
    for (int j = 0; j < 16; ++j) {
      if (ad[j] != a) continue;
      if (j < i) seen = true;
      mine |= 1u << j;
    }
    if (seen) continue;                                                       // this adapter's pass ran at its first row
    const atspeed_lora_slot sl = lora.slot(a);
    const bf16_t* a_cat = (const bf16_t*)sl.a_cat;
    if (!a_cat) continue;
    auto pass = [&](auto nt) {                                                // one barrier per pass run, none for a rank that is refused
      lora_shrink_pass<decltype(nt)::value>(w, nw, a_cat, u, LORA_U_LD, rows, hidden, lane, wave, part, mine);
      __syncthreads();                                                        // the next pass reuses `part`
    };
    switch (sl.r16) {
      case 16: pass(std::integral_constant<int, 3>{}); break;
      case 32: pass(std::integral_constant<int, 6>{}); break;
      case 48: pass(std::integral_constant<int, 9>{}); break;
      case 64: pass(std::integral_constant<int, 12>{}); break;
      default: break;
    }
  }
}

int ats_lora_shrink(const void* h, const void* norm_w, const void* a_cat, void* u, int rows, int hidden, int r3, float eps, int dtype,
                    hipStream_t st) {
  if (rows <= 0) return ATSPEED_OK;
  ATS_REQUIRE(h && norm_w && a_cat && u && hidden > 0, ATSPEED_ERR_INVALID, "lora_shrink: null argument");
  ATS_REQUIRE(r3 >= 48 && r3 <= 192 && r3 % 48 == 0, ATSPEED_ERR_INVALID, "lora_shrink: %d outputs per row (3 x the rank rounded up to 16, rank <= 64)", r3);
  const LoraOne one{{a_cat, nullptr, nullptr, nullptr, r3 / 3, 0.f}};
  if (dtype == ATSPEED_F32) {
    lora_shrink_kernel<float><<<rows, 256, 0, st>>>((const float*)h, (const float*)norm_w, one, (float*)u, nullptr, hidden, eps);
  } else if (hidden % 128 == 0 && (((uintptr_t)h | (uintptr_t)norm_w | (uintptr_t)a_cat) & 15) == 0) {
    const bf16_t *hb = (const bf16_t*)h, *wb = (const bf16_t*)norm_w, *ab = (const bf16_t*)a_cat;
    bf16_t* ub = (bf16_t*)u;
    const int grid = (rows + 15) / 16;
    switch (r3 / 48) {
      case 1: lora_shrink_mfma_kernel<3><<<grid, 256, 0, st>>>(hb, wb, ab, ub, rows, hidden, eps); break;
      case 2: lora_shrink_mfma_kernel<6><<<grid, 256, 0, st>>>(hb, wb, ab, ub, rows, hidden, eps); break;
      case 3: lora_shrink_mfma_kernel<9><<<grid, 256, 0, st>>>(hb, wb, ab, ub, rows, hidden, eps); break;
      default: lora_shrink_mfma_kernel<12><<<grid, 256, 0, st>>>(hb, wb, ab, ub, rows, hidden, eps); break;
    }
  } else {
    lora_shrink_kernel<bf16_t><<<rows, 256, 0, st>>>((const bf16_t*)h, (const bf16_t*)norm_w, one, (bf16_t*)u, nullptr, hidden, eps);
  }
  ATS_LAUNCH_CHECK();
  return ATSPEED_OK;
}

int ats_lora_shrink_segs(const void* h, const void* norm_w, const atspeed_lora_slot* dev_slots, bool slots_aligned, void* u, const SegTable& t,
                         const SegTable* dt, int hidden, float eps, int dtype, hipStream_t st) {
  const int rows = t.total_tok;
  if (rows <= 0) return ATSPEED_OK;
  ATS_REQUIRE(h && norm_w && dev_slots && u && dt && hidden > 0, ATSPEED_ERR_INVALID, "lora_shrink_segs: null argument");
  const LoraBySeg by_seg{dev_slots};
  if (dtype == ATSPEED_F32) {
    lora_shrink_kernel<float><<<rows, 256, 0, st>>>((const float*)h, (const float*)norm_w, by_seg, (float*)u, dt, hidden, eps);
  } else if (hidden % 128 == 0 && slots_aligned && (((uintptr_t)h | (uintptr_t)norm_w) & 15) == 0) {
    lora_shrink_segs_mfma_kernel<<<(rows + 15) / 16, 256, 0, st>>>((const bf16_t*)h, (const bf16_t*)norm_w, by_seg, (bf16_t*)u, dt, hidden, eps);
  } else {
    lora_shrink_kernel<bf16_t><<<rows, 256, 0, st>>>((const bf16_t*)h, (const bf16_t*)norm_w, by_seg, (bf16_t*)u, dt, hidden, eps);
  }
  ATS_LAUNCH_CHECK();
  return ATSPEED_OK;
}

// ---------------------------------------------------------------------------- expand + RoPE + KV scatter
// rope_kv_segs_kernel (elementwise.hip) with the expand in front: thread = (token, head, pair i).  A module whose B is NULL -- every module
// of a row of slot 0 -- takes that kernel's path unchanged.  The k and v columns of qkv stay the projection's (attention reads the caches).
template <typename T>
__device__ __forceinline__ float lora_col(float base, const T* __restrict__ u, const T* __restrict__ b, int col, int r16, float scaling) {
  if (!b) return base;
  const T* br = b + (size_t)col * r16;
  float acc = 0.f;
  for (int j = 0; j < r16; ++j) acc = __fmaf_rn(Elt<T>::load(u + j), Elt<T>::load(br + j), acc);
  return lora_add<T>(base, acc, scaling);
}

template <typename T, typename L>
__global__ void lora_rope_kv_segs_kernel(T* __restrict__ qkv, const T* __restrict__ u, const L lora, const SegTable* __restrict__ t,
                                         const float* __restrict__ cos_tab, const float* __restrict__ sin_tab, size_t layer_off, int n_heads,
                                         int head_dim, int max_pos) {
  int half = head_dim >> 1;
  int hidden = n_heads * head_dim;
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= t->total_tok * n_heads * half) return;
  int p = i % half;
  int h = (i / half) % n_heads;
  int row = i / (half * n_heads);
  const Seg& sg = t->seg[seg_of_row(t, row)];
  const atspeed_lora_slot sl = lora.slot(lora.seg_slot(sg));
  const T *bq = (const T*)sl.b_q, *bk = (const T*)sl.b_k, *bv = (const T*)sl.b_v;
  const int r16 = sl.r16;
  const float scaling = sl.scaling;
  int lt = row - sg.row0;
  const int ps = rope_pos(sg.pos[lt], max_pos);
  float c = cos_tab[(size_t)ps * half + p], s = sin_tab[(size_t)ps * half + p];
  T* r = qkv + (size_t)row * 3 * hidden;
  const T* ur = lora.u_row(u, row);
  int d0 = h * head_dim + p, d1 = d0 + half;
  float q0 = lora_col<T>(Elt<T>::load(r + d0), ur, bq, d0, r16, scaling), q1 = lora_col<T>(Elt<T>::load(r + d1), ur, bq, d1, r16, scaling);
  Elt<T>::store(r + d0, q0 * c - q1 * s);
  Elt<T>::store(r + d1, q1 * c + q0 * s);
  float k0 = lora_col<T>(Elt<T>::load(r + hidden + d0), ur + r16, bk, d0, r16, scaling);
  float k1 = lora_col<T>(Elt<T>::load(r + hidden + d1), ur + r16, bk, d1, r16, scaling);
  T* kc = kv_row<T>(sg.kc, layer_off, sg.slot[lt], hidden);
  T* vc = kv_row<T>(sg.vc, layer_off, sg.slot[lt], hidden);
  Elt<T>::store(kc + d0, k0 * c - k1 * s);
  Elt<T>::store(kc + d1, k1 * c + k0 * s);
  if (bv) {
    Elt<T>::store(vc + d0, lora_col<T>(Elt<T>::load(r + 2 * hidden + d0), ur + 2 * r16, bv, d0, r16, scaling));
    Elt<T>::store(vc + d1, lora_col<T>(Elt<T>::load(r + 2 * hidden + d1), ur + 2 * r16, bv, d1, r16, scaling));
  } else {
    vc[d0] = r[2 * hidden + d0];
    vc[d1] = r[2 * hidden + d1];
  }
}

// eight adjacent columns col0 .. col0 + 7 of one module: x = the projection's 16-bit outputs, returned with the adapter's term added.  u: the
// module's R16 entries of the token's row; B rows are R16 contiguous elements (16-byte loads, j ascending).
__device__ __forceinline__ uint4 lora_cols8(const uint4& x, const bf16_t* __restrict__ u, const bf16_t* __restrict__ b, int col0, int r16,
                                            float scaling) {
  float acc[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) acc[e] = 0.f;
  for (int j0 = 0; j0 < r16; j0 += 8) {
    const uint4 uv = *reinterpret_cast<const uint4*>(u + j0);
    const uint32_t* uw = reinterpret_cast<const uint32_t*>(&uv);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const uint4 bv = *reinterpret_cast<const uint4*>(b + (size_t)(col0 + e) * r16 + j0);
      const uint32_t* bw = reinterpret_cast<const uint32_t*>(&bv);
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        acc[e] = __fmaf_rn(bf_lo(uw[w]), bf_lo(bw[w]), acc[e]);
        acc[e] = __fmaf_rn(bf_hi(uw[w]), bf_hi(bw[w]), acc[e]);
      }
    }
  }
  uint4 y;
  const uint32_t* xw = reinterpret_cast<const uint32_t*>(&x);
  uint32_t* yw = reinterpret_cast<uint32_t*>(&y);
#pragma unroll
  for (int w = 0; w < 4; ++w)
    yw[w] = f2bf_pk(lora_add<bf16_t>(bf_lo(xw[w]), acc[2 * w], scaling), lora_add<bf16_t>(bf_hi(xw[w]), acc[2 * w + 1], scaling));
  return y;
}

// 16-bit, head_dim % 16 == 0: rope_kv_segs_vec_kernel (a thread owns 8 consecutive (i, i + dh/2) pairs of a head) with the expand in front
template <typename L>
__global__ void lora_rope_kv_segs_vec_kernel(bf16_t* __restrict__ qkv, const bf16_t* __restrict__ u, const L lora, const SegTable* __restrict__ t,
                                             const float* __restrict__ cos_tab, const float* __restrict__ sin_tab, size_t layer_off, int n_heads,
                                             int head_dim, int max_pos) {
  const int half = head_dim >> 1, groups = half >> 3;
  const int hidden = n_heads * head_dim;
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= t->total_tok * n_heads * groups) return;
  const int gi = i % groups;
  const int h = (i / groups) % n_heads;
  const int row = i / (groups * n_heads);
  const Seg& sg = t->seg[seg_of_row(t, row)];
  const atspeed_lora_slot sl = lora.slot(lora.seg_slot(sg));
  const bf16_t *bq = (const bf16_t*)sl.b_q, *bk = (const bf16_t*)sl.b_k, *bv = (const bf16_t*)sl.b_v;
  const int r16 = sl.r16;
  const float scaling = sl.scaling;
  const int lt = row - sg.row0;
  const int ps = rope_pos(sg.pos[lt], max_pos);
  const float* cp = cos_tab + (size_t)ps * half + gi * 8;
  const float* sp = sin_tab + (size_t)ps * half + gi * 8;
  bf16_t* r = qkv + (size_t)row * 3 * hidden;
  const bf16_t* ur = lora.u_row(u, row);
  const int d0 = h * head_dim + gi * 8, d1 = d0 + half;
  bf16_t* kc = kv_row(sg.kc, layer_off, sg.slot[lt], hidden);
  bf16_t* vc = kv_row(sg.vc, layer_off, sg.slot[lt], hidden);
  uint4 q0v = *reinterpret_cast<const uint4*>(r + d0), q1v = *reinterpret_cast<const uint4*>(r + d1);
  uint4 k0v = *reinterpret_cast<const uint4*>(r + hidden + d0), k1v = *reinterpret_cast<const uint4*>(r + hidden + d1);
  uint4 v0v = *reinterpret_cast<const uint4*>(r + 2 * hidden + d0), v1v = *reinterpret_cast<const uint4*>(r + 2 * hidden + d1);
  if (bq) { q0v = lora_cols8(q0v, ur, bq, d0, r16, scaling); q1v = lora_cols8(q1v, ur, bq, d1, r16, scaling); }
  if (bk) { k0v = lora_cols8(k0v, ur + r16, bk, d0, r16, scaling); k1v = lora_cols8(k1v, ur + r16, bk, d1, r16, scaling); }
  if (bv) { v0v = lora_cols8(v0v, ur + 2 * r16, bv, d0, r16, scaling); v1v = lora_cols8(v1v, ur + 2 * r16, bv, d1, r16, scaling); }
  uint4 qo0, qo1, ko0, ko1;
  const uint32_t *q0 = (const uint32_t*)&q0v, *q1 = (const uint32_t*)&q1v, *k0 = (const uint32_t*)&k0v, *k1 = (const uint32_t*)&k1v;
  uint32_t *a0 = (uint32_t*)&qo0, *a1 = (uint32_t*)&qo1, *b0 = (uint32_t*)&ko0, *b1 = (uint32_t*)&ko1;
#pragma unroll
  for (int e = 0; e < 4; ++e) {                                   // two elements per packed register
    const float ca = cp[2 * e], sa = sp[2 * e], cb = cp[2 * e + 1], sb = sp[2 * e + 1];
    const uint2 qr = rope_pk(q0[e], q1[e], ca, sa, cb, sb), kr = rope_pk(k0[e], k1[e], ca, sa, cb, sb);
    a0[e] = qr.x; a1[e] = qr.y;
    b0[e] = kr.x; b1[e] = kr.y;
  }
  *reinterpret_cast<uint4*>(r + d0) = qo0; *reinterpret_cast<uint4*>(r + d1) = qo1;
  *reinterpret_cast<uint4*>(kc + d0) = ko0; *reinterpret_cast<uint4*>(kc + d1) = ko1;
  *reinterpret_cast<uint4*>(vc + d0) = v0v;
  *reinterpret_cast<uint4*>(vc + d1) = v1v;
}

static bool lora_rope_vec_form(int dtype, int head_dim) { return dtype == ATS_HALF && head_dim % 16 == 0; }

template <typename L>
static int lora_rope_kv_launch(void* qkv, const void* u, const L& lora, const SegTable& t, const SegTable* dt, const float* cos_tab,
                               const float* sin_tab, size_t layer_off_bytes, int n_heads, int head_dim, int max_pos, int dtype, hipStream_t st) {
  const bool vec = lora_rope_vec_form(dtype, head_dim);
  const int total = t.total_tok * n_heads * (vec ? head_dim / 16 : head_dim / 2);
  if (total <= 0) return ATSPEED_OK;
  const int grid = (total + 255) / 256;
  if (vec)
    lora_rope_kv_segs_vec_kernel<<<grid, 256, 0, st>>>((bf16_t*)qkv, (const bf16_t*)u, lora, dt, cos_tab, sin_tab, layer_off_bytes, n_heads, head_dim, max_pos);
  else if (dtype == ATSPEED_F32)
    lora_rope_kv_segs_kernel<<<grid, 256, 0, st>>>((float*)qkv, (const float*)u, lora, dt, cos_tab, sin_tab, layer_off_bytes, n_heads, head_dim, max_pos);
  else
    lora_rope_kv_segs_kernel<<<grid, 256, 0, st>>>((bf16_t*)qkv, (const bf16_t*)u, lora, dt, cos_tab, sin_tab, layer_off_bytes, n_heads, head_dim, max_pos);
  ATS_LAUNCH_CHECK();
  return ATSPEED_OK;
}

int ats_lora_rope_kv_segs(void* qkv, const void* u, const void* bq, const void* bk, const void* bv, int r16, float scaling, const SegTable& t,
                          const SegTable* dt, const float* cos_tab, const float* sin_tab, size_t layer_off_bytes, int n_heads, int head_dim,
                          int max_pos, int dtype, hipStream_t st) {
  ATS_REQUIRE(u && r16 >= 16 && r16 <= 64 && r16 % 16 == 0, ATSPEED_ERR_INVALID, "lora_rope_kv: needs u and a rank of 16, 32, 48 or 64 after padding (got %d)", r16);
  ATS_REQUIRE(!lora_rope_vec_form(dtype, head_dim) || t.total_tok <= 0 || (((uintptr_t)u | (uintptr_t)bq | (uintptr_t)bk | (uintptr_t)bv) & 15) == 0,
              ATSPEED_ERR_INVALID, "lora_rope_kv: u and B must be 16-byte aligned");
  return lora_rope_kv_launch(qkv, u, LoraOne{{nullptr, bq, bk, bv, r16, scaling}}, t, dt, cos_tab, sin_tab, layer_off_bytes, n_heads, head_dim, max_pos,
                             dtype, st);
}

int ats_lora_rope_kv_segs_multi(void* qkv, const void* u, const atspeed_lora_slot* dev_slots, const SegTable& t, const SegTable* dt,
                                const float* cos_tab, const float* sin_tab, size_t layer_off_bytes, int n_heads, int head_dim, int max_pos,
                                int dtype, hipStream_t st) {
  ATS_REQUIRE(u && dev_slots && dt, ATSPEED_ERR_INVALID, "lora_rope_kv_multi: null argument");
  ATS_REQUIRE(!lora_rope_vec_form(dtype, head_dim) || t.total_tok <= 0 || ((uintptr_t)u & 15) == 0, ATSPEED_ERR_INVALID,
              "lora_rope_kv_multi: u must be 16-byte aligned");
  return lora_rope_kv_launch(qkv, u, LoraBySeg{dev_slots}, t, dt, cos_tab, sin_tab, layer_off_bytes, n_heads, head_dim, max_pos, dtype, st);
}

}  // namespace ATS_NS

#ifndef ATS_F16_FLAVOUR          // the C ABI exists once; it picks the flavour by the dtype code
extern "C" int atspeed_lora_shrink(const void* h, const void* norm_w, const void* a_cat, void* u, int32_t rows, int32_t hidden, int32_t r3,
                                   float eps, int32_t dtype, void* stream) {
  ATS_REQUIRE(dtype == ATSPEED_F32 || dtype == ATSPEED_BF16 || dtype == ATSPEED_F16, ATSPEED_ERR_INVALID, "lora_shrink: bad dtype");
  return ATS_KD(dtype, ats_lora_shrink(h, norm_w, a_cat, u, rows, hidden, r3, eps, dtype, (hipStream_t)stream));
}
#endif
