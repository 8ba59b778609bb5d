// LoRA adapters kept OUT of the base weights (peft's unmerged forward, code/inference.py:86-100 of the reference): a 16-bit side path beside
// the q / k / v projections of a layer, whatever format the base runs in (16-bit, W8A8, W4A8).  Two kernels per layer:
//   lora_shrink    u [T][3 R16] = lora_A of the layer's normed input, for the three modules at once (stacked A_cat [3 R16][H]);
//   lora_rope_kv   the RoPE + KV-scatter pass with lora_B and the add in front (y = base + scaling * B u), per adapted module.
// R16 = the rank rounded up to 16: pad rows of A_cat / pad columns of B_m are zero, an absent module's rows of A_cat are zero and its B_m is
// NULL.  The arithmetic is common.h's "LoRA side path" (lora_u / lora_add).
#include "internal.h"

namespace ATS_NS {

// ---------------------------------------------------------------------------- shrink
// Any type, any hidden: one workgroup per token row.  The row's RMS statistic as rmsnorm_kernel takes it, xn re-formed per output (the
// fallback of shapes the MFMA kernel does not take, and the fp32 engine's kernel).  Wave w owns outputs w, w + 4, ...: fixed order, so two
// runs give the same bits.
template <typename T>
__global__ __launch_bounds__(256) void lora_shrink_kernel(const T* __restrict__ h, const T* __restrict__ nw, const T* __restrict__ a_cat,
                                                          T* __restrict__ u, int hidden, int r3, float eps) {
  __shared__ float red[4];
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
    if (lane == 0) Elt<T>::store(u + (size_t)blockIdx.x * r3 + j, lora_u<T>(acc));
  }
}

// 16-bit, hidden % 128 == 0: a workgroup of four waves takes 16 token rows.  Lane l of a wave holds row l & 15, k-group l >> 4 of a 32-wide
// k-step -- its 16-byte load IS the MFMA A operand of v_mfma_f32_16x16x32 (after the norm), and the same load of A_cat row 16 t + (l & 15) the B
// operand of output tile t; acc[t][i] = u[row 4 (l >> 4) + i][16 t + (l & 15)].  Each wave sums a quarter of K; pass 1 takes the rows'
// sums of squares, pass 2 re-reads the rows (L2 hits).  The waves' partial tiles meet in LDS and are added in wave order.
template <int NT>
__global__ __launch_bounds__(256) void lora_shrink_mfma_kernel(const bf16_t* __restrict__ h, const bf16_t* __restrict__ nw,
                                                               const bf16_t* __restrict__ a_cat, bf16_t* __restrict__ u, int rows, int hidden,
                                                               float eps) {
  __shared__ float red[4][16];
  __shared__ f32x4_t part[4][NT][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 15, g = lane >> 4;
  const int row = blockIdx.x * 16 + r;
  const bf16_t* xr = h + (size_t)(row < rows ? row : rows - 1) * hidden;      // rows past the end: read the last row, store nothing
  const int kq = hidden >> 2, k0 = wave * kq + g * 8;                         // this wave's quarter of K, this lane's 8 of every 32
  float ss = 0.f;
  for (int k = 0; k < kq; k += 32) {
    const uint4 v = *reinterpret_cast<const uint4*>(xr + k0 + k);
    const bf16_t* e = reinterpret_cast<const bf16_t*>(&v);
#pragma unroll
    for (int j = 0; j < 8; ++j) { const float f = bf2f(e[j]); ss += f * f; }
  }
  ss += __shfl_xor(ss, 16, 64);
  ss += __shfl_xor(ss, 32, 64);
  if (g == 0) red[wave][r] = ss;
  __syncthreads();
  const float rs = rsqrtf((((red[0][r] + red[1][r]) + red[2][r]) + red[3][r]) / (float)hidden + eps);
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
      const int orow = blockIdx.x * 16 + g * 4 + i;
      if (orow < rows) u[(size_t)orow * (NT * 16) + t * 16 + r] = f2bf(lora_u<bf16_t>(s[i]));
    }
  }
}

int ats_lora_shrink(const void* h, const void* norm_w, const void* a_cat, void* u, int rows, int hidden, int r3, float eps, int dtype,
                    hipStream_t st) {
  if (rows <= 0) return ATSPEED_OK;
  ATS_REQUIRE(h && norm_w && a_cat && u && hidden > 0, ATSPEED_ERR_INVALID, "lora_shrink: null argument");
  ATS_REQUIRE(r3 >= 48 && r3 <= 192 && r3 % 48 == 0, ATSPEED_ERR_INVALID, "lora_shrink: %d outputs per row (3 x the rank rounded up to 16, rank <= 64)", r3);
  if (dtype == ATSPEED_F32) {
    lora_shrink_kernel<float><<<rows, 256, 0, st>>>((const float*)h, (const float*)norm_w, (const float*)a_cat, (float*)u, hidden, r3, eps);
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
    lora_shrink_kernel<bf16_t><<<rows, 256, 0, st>>>((const bf16_t*)h, (const bf16_t*)norm_w, (const bf16_t*)a_cat, (bf16_t*)u, hidden, r3, eps);
  }
  ATS_LAUNCH_CHECK();
  return ATSPEED_OK;
}

// ---------------------------------------------------------------------------- expand + RoPE + KV scatter
// rope_kv_segs_kernel (elementwise.hip) with the expand in front: thread = (token, head, pair i).  A module whose B is NULL takes that
// kernel's path unchanged.  The k and v columns of qkv stay the projection's (attention reads the caches).
template <typename T>
__device__ __forceinline__ float lora_col(float base, const T* __restrict__ u, const T* __restrict__ b, int col, int r16, float scaling) {
  if (!b) return base;
  const T* br = b + (size_t)col * r16;
  float acc = 0.f;
  for (int j = 0; j < r16; ++j) acc = __fmaf_rn(Elt<T>::load(u + j), Elt<T>::load(br + j), acc);
  return lora_add<T>(base, acc, scaling);
}

template <typename T>
__global__ void lora_rope_kv_segs_kernel(T* __restrict__ qkv, const T* __restrict__ u, const T* __restrict__ bq, const T* __restrict__ bk,
                                         const T* __restrict__ bv, int r16, float scaling, const SegTable* __restrict__ t,
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
  int lt = row - sg.row0;
  const int ps = rope_pos(sg.pos[lt], max_pos);
  float c = cos_tab[(size_t)ps * half + p], s = sin_tab[(size_t)ps * half + p];
  T* r = qkv + (size_t)row * 3 * hidden;
  const T* ur = u + (size_t)row * 3 * r16;
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
__global__ void lora_rope_kv_segs_vec_kernel(bf16_t* __restrict__ qkv, const bf16_t* __restrict__ u, const bf16_t* __restrict__ bq,
                                             const bf16_t* __restrict__ bk, const bf16_t* __restrict__ bv, int r16, float scaling,
                                             const SegTable* __restrict__ t, const float* __restrict__ cos_tab, const float* __restrict__ sin_tab,
                                             size_t layer_off, int n_heads, int head_dim, int max_pos) {
  const int half = head_dim >> 1, groups = half >> 3;
  const int hidden = n_heads * head_dim;
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= t->total_tok * n_heads * groups) return;
  const int gi = i % groups;
  const int h = (i / groups) % n_heads;
  const int row = i / (groups * n_heads);
  const Seg& sg = t->seg[seg_of_row(t, row)];
  const int lt = row - sg.row0;
  const int ps = rope_pos(sg.pos[lt], max_pos);
  const float* cp = cos_tab + (size_t)ps * half + gi * 8;
  const float* sp = sin_tab + (size_t)ps * half + gi * 8;
  bf16_t* r = qkv + (size_t)row * 3 * hidden;
  const bf16_t* ur = u + (size_t)row * 3 * r16;
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

int ats_lora_rope_kv_segs(void* qkv, const void* u, const void* bq, const void* bk, const void* bv, int r16, float scaling, const SegTable& t,
                          const SegTable* dt, const float* cos_tab, const float* sin_tab, size_t layer_off_bytes, int n_heads, int head_dim,
                          int max_pos, int dtype, hipStream_t st) {
  ATS_REQUIRE(u && r16 >= 16 && r16 <= 64 && r16 % 16 == 0, ATSPEED_ERR_INVALID, "lora_rope_kv: needs u and a rank of 16, 32, 48 or 64 after padding (got %d)", r16);
  if (dtype == ATS_HALF && head_dim % 16 == 0) {
    int totalv = t.total_tok * n_heads * (head_dim / 16);
    if (totalv <= 0) return ATSPEED_OK;
    ATS_REQUIRE((((uintptr_t)u | (uintptr_t)bq | (uintptr_t)bk | (uintptr_t)bv) & 15) == 0, ATSPEED_ERR_INVALID, "lora_rope_kv: u and B must be 16-byte aligned");
    lora_rope_kv_segs_vec_kernel<<<(totalv + 255) / 256, 256, 0, st>>>((bf16_t*)qkv, (const bf16_t*)u, (const bf16_t*)bq, (const bf16_t*)bk,
                                                                       (const bf16_t*)bv, r16, scaling, dt, cos_tab, sin_tab, layer_off_bytes,
                                                                       n_heads, head_dim, max_pos);
    ATS_LAUNCH_CHECK();
    return ATSPEED_OK;
  }
  int total = t.total_tok * n_heads * (head_dim / 2);
  if (total <= 0) return ATSPEED_OK;
  if (dtype == ATSPEED_F32)
    lora_rope_kv_segs_kernel<float><<<(total + 255) / 256, 256, 0, st>>>((float*)qkv, (const float*)u, (const float*)bq, (const float*)bk,
                                                                         (const float*)bv, r16, scaling, dt, cos_tab, sin_tab, layer_off_bytes,
                                                                         n_heads, head_dim, max_pos);
  else
    lora_rope_kv_segs_kernel<bf16_t><<<(total + 255) / 256, 256, 0, st>>>((bf16_t*)qkv, (const bf16_t*)u, (const bf16_t*)bq, (const bf16_t*)bk,
                                                                          (const bf16_t*)bv, r16, scaling, dt, cos_tab, sin_tab, layer_off_bytes,
                                                                          n_heads, head_dim, max_pos);
  ATS_LAUNCH_CHECK();
  return ATSPEED_OK;
}

// ---------------------------------------------------------------------------- several resident adapters, picked per row
// The two kernels above with the adapter looked up per token row: seg_of_row -> Seg::adapter -> the model's slot table (entry 0 = none).  The
// arithmetic of a row is exactly that of the single-adapter kernels with the row's slot (same k partition, same order of every sum), so a row's
// result depends neither on its place in a 16-row tile nor on what its neighbours name.  u has a fixed row stride of 3 x 64 elements; a row
// of slot 0 is neither written by the shrink nor read by the expand.
constexpr int LORA_U_LD = 3 * ATSPEED_LORA_MAX_RANK;

__device__ __forceinline__ int seg_adapter(const Seg& sg) { return sg.adapter > 0 && sg.adapter <= ATSPEED_LORA_MAX_ADAPTERS ? sg.adapter : 0; }

// lora_shrink_kernel with the row's slot: one workgroup per token row, rows of slot 0 leave at once
template <typename T>
__global__ __launch_bounds__(256) void lora_shrink_segs_kernel(const T* __restrict__ h, const T* __restrict__ nw,
                                                               const atspeed_lora_slot* __restrict__ tab, T* __restrict__ u,
                                                               const SegTable* __restrict__ t, int hidden, float eps) {
  __shared__ float red[4];
  const int a = seg_adapter(t->seg[seg_of_row(t, blockIdx.x)]);
  if (a == 0) return;
  const T* a_cat = (const T*)tab[a].a_cat;
  const int r3 = 3 * tab[a].r16;
  if (!a_cat || r3 < 48 || r3 > LORA_U_LD) return;
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
    if (lane == 0) Elt<T>::store(u + (size_t)blockIdx.x * LORA_U_LD + j, lora_u<T>(acc));
  }
}

// one adapter's pass of the MFMA shrink over a workgroup's 16 rows: lora_shrink_mfma_kernel<NT>'s k-loop and wave-order sum against this
// adapter's A_cat; only the rows whose bit is set in `mine` are stored.  Ends with a barrier: the next pass reuses `part`.
template <int NT>
__device__ __forceinline__ void lora_shrink_pass(const bf16_t* __restrict__ xr, const bf16_t* __restrict__ nw, const bf16_t* __restrict__ a_cat,
                                                 bf16_t* __restrict__ u, int rows, int hidden, float rs, int kq, int k0, int lane, int wave,
                                                 f32x4_t (*part)[12][64], unsigned mine) {
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
      if (orow < rows && ((mine >> lr) & 1u)) u[(size_t)orow * LORA_U_LD + t * 16 + r] = f2bf(lora_u<bf16_t>(s[i]));
    }
  }
  __syncthreads();
}

// lora_shrink_mfma_kernel over rows of several adapters: the workgroup takes its 16 rows' RMS statistic once, then runs one pass per
// DISTINCT adapter among them (rows come grouped by segment: typically one or two) with that adapter's tile count.  Everything that
// steers the passes is uniform over the workgroup.
__global__ __launch_bounds__(256) void lora_shrink_segs_mfma_kernel(const bf16_t* __restrict__ h, const bf16_t* __restrict__ nw,
                                                                    const atspeed_lora_slot* __restrict__ tab, bf16_t* __restrict__ u,
                                                                    const SegTable* __restrict__ t, int hidden, float eps) {
  __shared__ float red[4][16];
  __shared__ int ad[16];
  __shared__ f32x4_t part[4][12][64];
  const int rows = t->total_tok;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 15, g = lane >> 4;
  if (threadIdx.x < 16) {
    const int rr = blockIdx.x * 16 + threadIdx.x;
    ad[threadIdx.x] = rr < rows ? seg_adapter(t->seg[seg_of_row(t, rr)]) : 0;
  }
  __syncthreads();
  int any = 0;
#pragma unroll
  for (int i = 0; i < 16; ++i) any |= ad[i];
  if (any == 0) return;                                                       // no row of this tile names an adapter
  const int row = blockIdx.x * 16 + r;
  const bf16_t* xr = h + (size_t)(row < rows ? row : rows - 1) * hidden;      // rows past the end: read the last row, store nothing
  const int kq = hidden >> 2, k0 = wave * kq + g * 8;                         // this wave's quarter of K, this lane's 8 of every 32
  float ss = 0.f;
  for (int k = 0; k < kq; k += 32) {
    const uint4 v = *reinterpret_cast<const uint4*>(xr + k0 + k);
    const bf16_t* e = reinterpret_cast<const bf16_t*>(&v);
#pragma unroll
    for (int j = 0; j < 8; ++j) { const float f = bf2f(e[j]); ss += f * f; }
  }
  ss += __shfl_xor(ss, 16, 64);
  ss += __shfl_xor(ss, 32, 64);
  if (g == 0) red[wave][r] = ss;
  __syncthreads();
  const float rs = rsqrtf((((red[0][r] + red[1][r]) + red[2][r]) + red[3][r]) / (float)hidden + eps);
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
    const bf16_t* a_cat = (const bf16_t*)tab[a].a_cat;
    if (!a_cat) continue;
    switch (tab[a].r16) {
      case 16: lora_shrink_pass<3>(xr, nw, a_cat, u, rows, hidden, rs, kq, k0, lane, wave, part, mine); break;
      case 32: lora_shrink_pass<6>(xr, nw, a_cat, u, rows, hidden, rs, kq, k0, lane, wave, part, mine); break;
      case 48: lora_shrink_pass<9>(xr, nw, a_cat, u, rows, hidden, rs, kq, k0, lane, wave, part, mine); break;
      case 64: lora_shrink_pass<12>(xr, nw, a_cat, u, rows, hidden, rs, kq, k0, lane, wave, part, mine); break;
      default: break;
    }
  }
}

int ats_lora_shrink_segs(const void* h, const void* norm_w, const atspeed_lora_slot* dev_slots, bool slots_aligned, void* u, const SegTable& t,
                         const SegTable* dt, int hidden, float eps, int dtype, hipStream_t st) {
  const int rows = t.total_tok;
  if (rows <= 0) return ATSPEED_OK;
  ATS_REQUIRE(h && norm_w && dev_slots && u && dt && hidden > 0, ATSPEED_ERR_INVALID, "lora_shrink_segs: null argument");
  if (dtype == ATSPEED_F32) {
    lora_shrink_segs_kernel<float><<<rows, 256, 0, st>>>((const float*)h, (const float*)norm_w, dev_slots, (float*)u, dt, hidden, eps);
  } else if (hidden % 128 == 0 && slots_aligned && (((uintptr_t)h | (uintptr_t)norm_w) & 15) == 0) {
    lora_shrink_segs_mfma_kernel<<<(rows + 15) / 16, 256, 0, st>>>((const bf16_t*)h, (const bf16_t*)norm_w, dev_slots, (bf16_t*)u, dt, hidden, eps);
  } else {
    lora_shrink_segs_kernel<bf16_t><<<rows, 256, 0, st>>>((const bf16_t*)h, (const bf16_t*)norm_w, dev_slots, (bf16_t*)u, dt, hidden, eps);
  }
  ATS_LAUNCH_CHECK();
  return ATSPEED_OK;
}

// lora_rope_kv_segs_kernel with (bq, bk, bv, r16, scaling) of the row's slot; slot 0 = every B NULL: rope_kv_segs_kernel's path
template <typename T>
__global__ void lora_rope_kv_segs_multi_kernel(T* __restrict__ qkv, const T* __restrict__ u, const atspeed_lora_slot* __restrict__ tab,
                                               const SegTable* __restrict__ t, const float* __restrict__ cos_tab,
                                               const float* __restrict__ sin_tab, size_t layer_off, int n_heads, int head_dim, int max_pos) {
  int half = head_dim >> 1;
  int hidden = n_heads * head_dim;
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= t->total_tok * n_heads * half) return;
  int p = i % half;
  int h = (i / half) % n_heads;
  int row = i / (half * n_heads);
  const Seg& sg = t->seg[seg_of_row(t, row)];
  const int ad = seg_adapter(sg);
  const T *bq = nullptr, *bk = nullptr, *bv = nullptr;
  int r16 = 0;
  float scaling = 0.f;
  if (ad) { bq = (const T*)tab[ad].b_q; bk = (const T*)tab[ad].b_k; bv = (const T*)tab[ad].b_v; r16 = tab[ad].r16; scaling = tab[ad].scaling; }
  int lt = row - sg.row0;
  const int ps = rope_pos(sg.pos[lt], max_pos);
  float c = cos_tab[(size_t)ps * half + p], s = sin_tab[(size_t)ps * half + p];
  T* r = qkv + (size_t)row * 3 * hidden;
  const T* ur = u + (size_t)row * LORA_U_LD;
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

// lora_rope_kv_segs_vec_kernel with the row's slot
__global__ void lora_rope_kv_segs_multi_vec_kernel(bf16_t* __restrict__ qkv, const bf16_t* __restrict__ u, const atspeed_lora_slot* __restrict__ tab,
                                                   const SegTable* __restrict__ t, const float* __restrict__ cos_tab,
                                                   const float* __restrict__ sin_tab, size_t layer_off, int n_heads, int head_dim, int max_pos) {
  const int half = head_dim >> 1, groups = half >> 3;
  const int hidden = n_heads * head_dim;
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= t->total_tok * n_heads * groups) return;
  const int gi = i % groups;
  const int h = (i / groups) % n_heads;
  const int row = i / (groups * n_heads);
  const Seg& sg = t->seg[seg_of_row(t, row)];
  const int ad = seg_adapter(sg);
  const bf16_t *bq = nullptr, *bk = nullptr, *bv = nullptr;
  int r16 = 0;
  float scaling = 0.f;
  if (ad) { bq = (const bf16_t*)tab[ad].b_q; bk = (const bf16_t*)tab[ad].b_k; bv = (const bf16_t*)tab[ad].b_v; r16 = tab[ad].r16; scaling = tab[ad].scaling; }
  const int lt = row - sg.row0;
  const int ps = rope_pos(sg.pos[lt], max_pos);
  const float* cp = cos_tab + (size_t)ps * half + gi * 8;
  const float* sp = sin_tab + (size_t)ps * half + gi * 8;
  bf16_t* r = qkv + (size_t)row * 3 * hidden;
  const bf16_t* ur = u + (size_t)row * LORA_U_LD;
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

int ats_lora_rope_kv_segs_multi(void* qkv, const void* u, const atspeed_lora_slot* dev_slots, const SegTable& t, const SegTable* dt,
                                const float* cos_tab, const float* sin_tab, size_t layer_off_bytes, int n_heads, int head_dim, int max_pos,
                                int dtype, hipStream_t st) {
  ATS_REQUIRE(u && dev_slots && dt, ATSPEED_ERR_INVALID, "lora_rope_kv_multi: null argument");
  if (dtype == ATS_HALF && head_dim % 16 == 0) {
    int totalv = t.total_tok * n_heads * (head_dim / 16);
    if (totalv <= 0) return ATSPEED_OK;
    ATS_REQUIRE(((uintptr_t)u & 15) == 0, ATSPEED_ERR_INVALID, "lora_rope_kv_multi: u must be 16-byte aligned");
    lora_rope_kv_segs_multi_vec_kernel<<<(totalv + 255) / 256, 256, 0, st>>>((bf16_t*)qkv, (const bf16_t*)u, dev_slots, dt, cos_tab, sin_tab,
                                                                             layer_off_bytes, n_heads, head_dim, max_pos);
    ATS_LAUNCH_CHECK();
    return ATSPEED_OK;
  }
  int total = t.total_tok * n_heads * (head_dim / 2);
  if (total <= 0) return ATSPEED_OK;
  if (dtype == ATSPEED_F32)
    lora_rope_kv_segs_multi_kernel<float><<<(total + 255) / 256, 256, 0, st>>>((float*)qkv, (const float*)u, dev_slots, dt, cos_tab, sin_tab,
                                                                               layer_off_bytes, n_heads, head_dim, max_pos);
  else
    lora_rope_kv_segs_multi_kernel<bf16_t><<<(total + 255) / 256, 256, 0, st>>>((bf16_t*)qkv, (const bf16_t*)u, dev_slots, dt, cos_tab, sin_tab,
                                                                                layer_off_bytes, n_heads, head_dim, max_pos);
  ATS_LAUNCH_CHECK();
  return ATSPEED_OK;
}

}  // namespace ATS_NS

#ifndef ATS_F16_FLAVOUR          // the C ABI exists once; it picks the flavour by the dtype code
extern "C" int atspeed_lora_shrink(const void* h, const void* norm_w, const void* a_cat, void* u, int32_t rows, int32_t hidden, int32_t r3,
                                   float eps, int32_t dtype, void* stream) {
  ATS_REQUIRE(dtype == ATSPEED_F32 || dtype == ATSPEED_BF16 || dtype == ATSPEED_F16, ATSPEED_ERR_INVALID, "lora_shrink: bad dtype");
  return ATS_KD(dtype, ats_lora_shrink(h, norm_w, a_cat, u, rows, hidden, r3, eps, dtype, (hipStream_t)stream));
}
#endif
