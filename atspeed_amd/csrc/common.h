// Shared device helpers and host-side error plumbing for libatspeed_hip (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string>

#include "../../include/atspeed_hip.h"

// ---------------------------------------------------------------- the 16-bit flavour of a kernel translation unit
// The engine computes in fp32, bf16 or fp16 (ATSPEED_F16: the type the reference loads both models in, code/inference.py:75-100).  bf16 and
// fp16 kernels are the SAME source: gemm.hip, attn.hip and elementwise.hip are compiled twice (Makefile), once per flavour, each into its
// own namespace (ats_bf16 / ats_f16); what differs is confined to this block -- the element conversions, the MFMA instruction of the type
// (v_mfma_f32_16x16x32_{bf16,f16}, v_mfma_f32_32x32x16_{bf16,f16}) and the packed conversion (v_cvt_pk_{bf16,f16}_f32).  `bf16_t` and the
// helper names (bf2f, f2bf, f2bf_pk, bf_lo, bf_hi) keep their names in both flavours: "the engine's 16-bit type".  engine.hip picks the
// namespace by the model's dtype (ATS_K).
typedef unsigned short bf16_t;   // raw bits of the flavour's 16-bit type
#ifdef ATS_F16_FLAVOUR
#define ATS_NS ats_f16
#define ATS_HALF ATSPEED_F16
#define ATS_MFMA_16x16x32_NAME "v_mfma_f32_16x16x32_f16"
#define ATS_CVT_PK_NAME "v_cvt_pk_f16_f32"
typedef __attribute__((ext_vector_type(8))) _Float16 bf16x8_t;
#define ATS_MFMA_16x16x32(a, b, c) __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0)
#define ATS_MFMA_32x32x16(a, b, c) __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0)
#else
#define ATS_NS ats_bf16
#define ATS_HALF ATSPEED_BF16
#define ATS_MFMA_16x16x32_NAME "v_mfma_f32_16x16x32_bf16"
#define ATS_CVT_PK_NAME "v_cvt_pk_bf16_f32"
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8_t;
#define ATS_MFMA_16x16x32(a, b, c) __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0)
#define ATS_MFMA_32x32x16(a, b, c) __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0)
#endif
// a call of a flavoured internal function, by dtype code: ATS_KD(dt, ats_gemm(...)) -> ats_f16::ats_gemm(...) or ats_bf16::ats_gemm(...)
// (the bf16 build also holds the fp32 parity kernels)
#define ATS_KD(dtype, call) ((dtype) == ATSPEED_F16 ? ats_f16::call : ats_bf16::call)
typedef __attribute__((ext_vector_type(8))) short s16x8_t;
typedef __attribute__((ext_vector_type(4))) float f32x4_t;
// 16-byte register value as an SSA vector: HIP's uint4 STRUCT in a register ring ended up in scratch (hipcc 7.2)
typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));

// ---------------------------------------------------------------- host error plumbing
void atspeed_set_error(const char* fmt, ...);

#define ATS_HIP(expr)                                                                              \
  do {                                                                                             \
    hipError_t _e = (expr);                                                                        \
    if (_e != hipSuccess) {                                                                        \
      atspeed_set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
      (void)hipGetLastError(); /* reported here: the next launch check must not find it again */  \
      return ATSPEED_ERR_HIP;                                                                      \
    }                                                                                              \
  } while (0)

#define ATS_REQUIRE(cond, code, ...)     \
  do {                                   \
    if (!(cond)) {                       \
      atspeed_set_error(__VA_ARGS__);    \
      return (code);                     \
    }                                    \
  } while (0)

#define ATS_LAUNCH_CHECK() ATS_HIP(hipGetLastError())

#define ATS_TRY(expr)            \
  do {                           \
    int _s = (expr);             \
    if (_s != ATSPEED_OK) return _s; \
  } while (0)

// per-(thread, device) state: one process may drive several GPUs from one thread, so staging buffers, events and the
// "function attribute set" flags are kept per HIP device, selected by the device current at the call
constexpr int ATS_MAX_DEVICES = 64;
// index of the current HIP device in the per-device tables, or -1 when hipGetDevice fails or the id is beyond the tables: callers
// must not alias another device's staging memory / events (they return ATSPEED_ERR_NO_DEVICE)
inline int ats_cur_device() {
  int d = 0;
  if (hipGetDevice(&d) != hipSuccess || d < 0 || d >= ATS_MAX_DEVICES) return -1;
  return d;
}
struct AtsPerDeviceFlag {
  bool done[ATS_MAX_DEVICES] = {};
  bool never = false;                 // unknown device: "not done yet" every time (the attribute call is simply repeated)
  bool& cur() { const int d = ats_cur_device(); if (d < 0) { never = false; return never; } return done[d]; }
};
// raise a kernel's dynamic-LDS limit above the default, once per (host thread, device)
template <auto KERNEL>
inline int ats_lds_limit(int bytes) {
  static thread_local AtsPerDeviceFlag flag;
  bool& done = flag.cur();
  if (!done) {
    ATS_HIP(hipFuncSetAttribute((const void*)KERNEL, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    done = true;
  }
  return ATSPEED_OK;
}

// ---------------------------------------------------------------- packed GEMM-operand layout
// What the LDS-DMA of the ring GEMMs wants from HBM (measured, tools/probe/dma_depth.hip: 83 GB/s per CU against 55 GB/s): every
// 1 KB DMA piece (16 rows x 64 bytes of K) made of FULL 128-byte lines.  A row-major operand gives it 16 half lines.  In the packed
// layout two consecutive rows share a line per 64-byte k-block:
//   byte b of row r  ->  ((r >> 1) * (row_bytes / 64) + (b >> 6)) * 128 + (r & 1) * 64 + (b & 63)
// (row_bytes % 64 == 0, buffers hold an even number of rows).  The bf16 / fp8 engine keeps every GEMM operand in it -- projection
// weights, lm_head, and the activations a projection reads (RMSNorm output, attention output, SwiGLU output, their e4m3 forms) --
// written that way by their producers; everything else (residual stream, qkv, logits, KV cache, fp32 parity mode) stays row-major.
__host__ __device__ inline size_t ats_pk_byte(size_t row, size_t byte_in_row, size_t row_bytes) {
  return ((row >> 1) * (row_bytes >> 6) + (byte_in_row >> 6)) * 128 + (row & 1) * 64 + (byte_in_row & 63);
}
// element index of (row, col) in an operand of `ld` elements per row, element size 2^esz_log2 bytes, packed or row-major
template <int ESZ>
__host__ __device__ inline size_t ats_opnd_idx(int pk, size_t row, size_t col, size_t ld) {
  return pk ? ats_pk_byte(row, col * ESZ, ld * ESZ) / ESZ : row * ld + col;
}
// The same map as the GEMM kernels' loads and LDS-DMAs use it, in their own index type I (32-bit lane offsets in the LDS-DMA kernels, size_t
// elsewhere): the 16-byte chunk c of the RB bytes of row `row` that one LDS row holds (RB = 64 or 128, c < RB / 16), ld_bytes per row:
//   ats_chunk_byte<RB>(pk, row, ld_bytes, c) == pk ? ats_pk_byte(row, c * 16, ld_bytes) : row * ld_bytes + c * 16
// and the next RB bytes of the row lie ats_kadv<RB>(pk) further on: RB row-major, 2 RB packed (ats_pk_byte(r, b + 64, .) - ats_pk_byte(r, b, .)
// == 128).  ats_pk_byte itself where a kernel computes in size_t anyway (gemm_w4a8_kernel).
template <int RB, typename I, typename R>
__host__ __device__ inline I ats_chunk_byte(int pk, R row, I ld_bytes, int c) {
  static_assert(RB == 64 || RB == 128, "one or two 64-byte k-blocks per LDS row");
  if constexpr (RB == 64) return (pk ? (I)(row >> 1) * (ld_bytes * 2) + (row & 1) * 64 : (I)row * ld_bytes) + (c * 16);
  else return pk ? (I)(row >> 1) * (ld_bytes * 2) + (row & 1) * 64 + (I)(c >> 2) * 128 + (c & 3) * 16 : (I)row * ld_bytes + (I)c * 16;
}
template <int RB> __host__ __device__ constexpr int ats_kadv(int pk) { return pk ? 2 * RB : RB; }

// ---------------------------------------------------------------- GEMM work division (host + device: the walk can be checked on the CPU)
// Workgroup id -> tile (tn, tm) of the ring GEMMs' tiles_n x tiles_m grid, in two steps.  xcd_run: workgroup L runs on XCD L % 8 (private 4 MB
// L2); every XCD gets a contiguous run of the nwg positions, the first nwg % 8 of them one position longer.  band_tile: the positions walk
// bands of GM token-tile rows (the last band may be lower), W-panel-major inside a band.  A bijection of [0, nwg) onto the grid.
struct GemmTile { int tn, tm; };
__host__ __device__ inline int xcd_run(int bid, int nwg) {
  const int q = nwg / 8, r = nwg % 8, x = bid % 8;
  return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + bid / 8;
}
__host__ __device__ inline GemmTile band_tile(int pos, int tiles_n, int tiles_m, int GM) {
  const int band = pos / (GM * tiles_n), rem = pos % (GM * tiles_n);
  const int left = tiles_m - band * GM, band_rows = GM < left ? GM : left;
  return GemmTile{rem / band_rows, band * GM + rem % band_rows};
}
__host__ __device__ inline GemmTile tile_walk(int bid, int tiles_n, int tiles_m, int GM) {
  return band_tile(xcd_run(bid, tiles_n * tiles_m), tiles_n, tiles_m, GM);
}
// `units` units of k dealt to n_split parts: part z takes [part_begin(z), part_begin(z + 1)), the parts' sizes differing by one unit at most
__host__ __device__ inline int part_begin(int z, int units, int n_split) { return (int)((long long)z * units / n_split); }

// counter-based hash shared by the synthetic-weight fill and the sampling kernels (= atspeed_amd/synth.py:hash_u32)
__host__ __device__ inline uint32_t ats_fmix32(uint32_t h) {
  h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;
  return h;
}
__host__ __device__ inline uint32_t ats_hash_u32(uint32_t idx, uint32_t seed) { return ats_fmix32(idx * 0x9E3779B1u + seed); }
// sub-seed of one random stream: purpose | round << 8 | step << 16 | model tag << 24 (oracle/beamsd_sample_ref.py:HashRng.begin)
enum { ATS_RNG_STEP = 1, ATS_RNG_ACCEPT = 2, ATS_RNG_PERM = 3, ATS_RNG_RESID = 4, ATS_RNG_BONUS = 5 };
__host__ __device__ inline uint32_t ats_rng_sub(uint32_t seed, int purpose, int round, int step, int tag) {
  return ats_hash_u32((uint32_t)(purpose & 0xff) | ((uint32_t)(round & 0xff) << 8) | ((uint32_t)(step & 0xff) << 16) | ((uint32_t)(tag & 0xff) << 24), seed);
}

// ---------------------------------------------------------------- device helpers
#if defined(__HIPCC__)
__device__ __forceinline__ float ats_u01(uint32_t h) { return ((float)(h >> 9) + 0.5f) * 1.1920928955078125e-07f; }   // (k + 1/2) 2^-23, exact
__device__ __forceinline__ float ats_gumbel(uint32_t h) { return -logf(-logf(ats_u01(h))); }
typedef __attribute__((ext_vector_type(2))) float ats_f32x2_t;
#ifdef ATS_F16_FLAVOUR
// fp16 flavour: hardware conversions both ways (v_cvt_f32_f16 / v_cvt_f16_f32, round to nearest even; v_cvt_pk_f16_f32 for pairs on gfx950)
typedef __attribute__((ext_vector_type(2))) _Float16 ats_bf16x2_t;
__device__ __forceinline__ float bf2f(bf16_t v) { return (float)__builtin_bit_cast(_Float16, v); }
__device__ __forceinline__ bf16_t f2bf(float f) { return __builtin_bit_cast(bf16_t, (_Float16)f); }
__device__ __forceinline__ uint32_t f2bf_pk(float lo, float hi) {
  ats_f32x2_t v = {lo, hi};
  return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, ats_bf16x2_t));
}
__device__ __forceinline__ float bf_lo(uint32_t pk) { return (float)__builtin_bit_cast(_Float16, (unsigned short)(pk & 0xffffu)); }
__device__ __forceinline__ float bf_hi(uint32_t pk) { return (float)__builtin_bit_cast(_Float16, (unsigned short)(pk >> 16)); }
#else
__device__ __forceinline__ float bf2f(bf16_t v) { return __uint_as_float(((uint32_t)v) << 16); }
// round to nearest even in hardware (v_cvt_pk_bf16_f32 on gfx950: the compiler pairs neighbouring conversions); the six-instruction
// integer form this replaces was a sixth of the ring GEMM's epilogue and most of the attention softmax's VALU work
__device__ __forceinline__ bf16_t f2bf(float f) { return __builtin_bit_cast(bf16_t, (__bf16)f); }
// two values -> one packed register (low half = lo); and the two values back as floats (a bf16 is the high half of its fp32)
typedef __attribute__((ext_vector_type(2))) __bf16 ats_bf16x2_t;
__device__ __forceinline__ uint32_t f2bf_pk(float lo, float hi) {
  ats_f32x2_t v = {lo, hi};
  return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, ats_bf16x2_t));
}
__device__ __forceinline__ float bf_lo(uint32_t pk) { return __uint_as_float(pk << 16); }
__device__ __forceinline__ float bf_hi(uint32_t pk) { return __uint_as_float(pk & 0xffff0000u); }
#endif
// SiLU.  bf16 engine (EXACT = false): the quotient through the hardware reciprocal (v_rcp_f32, 1 ulp of fp32 -- far below the bf16 rounding that
// follows); the correctly rounded fp32 division is a ten-instruction sequence and made the ring GEMM's SwiGLU epilogue VALU-bound (64 outputs per
// thread).  fp32 engine (parity mode): the exact quotient.
template <bool EXACT> __device__ __forceinline__ float ats_silu(float g) {
  const float d = 1.f + __expf(-g);
  if constexpr (EXACT) return g / d;
  else return g * __builtin_amdgcn_rcpf(d);
}
template <typename T> struct Elt;
template <> struct Elt<float> {
  static constexpr int kPerChunk = 4;   // elements per 16-byte chunk
  __device__ static __forceinline__ float load(const float* p) { return *p; }
  __device__ static __forceinline__ void store(float* p, float v) { *p = v; }
};
template <> struct Elt<bf16_t> {
  static constexpr int kPerChunk = 8;
  __device__ static __forceinline__ float load(const bf16_t* p) { return bf2f(*p); }
  __device__ static __forceinline__ void store(bf16_t* p, float v) { *p = f2bf(v); }
};

__device__ __forceinline__ float wave_max_f32(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ float wave_sum_f32(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
// maximum of a 64-bit key over the wave, returned wave-uniform.  Data-parallel-primitive moves instead of ds_bpermute shuffles (a block top-K
// runs this once per extracted key: 12 LDS round trips per call were most of a one-user beam step's 85 us): row_shr 1/2/4/8 leave a 16-lane
// row's maximum in its lane 15 (max is idempotent, an invalid source lane keeps the own value), row_bcast15 / row_bcast31 carry it to
// lane 63, one readlane pair makes it uniform.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ unsigned long long ats_dpp_max_u64(unsigned long long v) {
  const int lo = (int)(unsigned)(v & 0xffffffffull), hi = (int)(unsigned)(v >> 32);
  const unsigned wlo = (unsigned)__builtin_amdgcn_update_dpp(lo, lo, CTRL, ROW_MASK, 0xf, false);
  const unsigned whi = (unsigned)__builtin_amdgcn_update_dpp(hi, hi, CTRL, ROW_MASK, 0xf, false);
  const unsigned long long w = ((unsigned long long)whi << 32) | wlo;
  return w > v ? w : v;
}
__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
  v = ats_dpp_max_u64<0x111, 0xf>(v);        // row_shr:1
  v = ats_dpp_max_u64<0x112, 0xf>(v);        // row_shr:2
  v = ats_dpp_max_u64<0x114, 0xf>(v);        // row_shr:4
  v = ats_dpp_max_u64<0x118, 0xf>(v);        // row_shr:8   -> lane 15 of every row: the row's maximum
  v = ats_dpp_max_u64<0x142, 0xa>(v);        // row_bcast15 into rows 1 and 3
  v = ats_dpp_max_u64<0x143, 0xc>(v);        // row_bcast31 into rows 2 and 3 -> lane 63: the wave's maximum
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v & 0xffffffffull), 63);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), 63);
  return ((unsigned long long)hi << 32) | lo;
}

// monotone float <-> uint32 map: a > b  <=>  ford(a) > ford(b)   (-inf -> 0x007fffff)
__device__ __forceinline__ uint32_t ford(float f) {
  uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
// ford for a selection key whose ties go to the lower id: -0.0 and +0.0 are EQUAL values, so both take +0.0's key (ford alone ranks
// +0.0 above -0.0).  The test is on the bits, an integer compare no floating-point simplification can fold; every other input maps as in ford.
__device__ __forceinline__ uint32_t ford_key(float f) {
  const uint32_t u = __float_as_uint(f);
  return ford(__uint_as_float(u == 0x80000000u ? 0u : u));
}
__device__ __forceinline__ float ford_inv(uint32_t o) {
  uint32_t u = (o & 0x80000000u) ? (o & 0x7fffffffu) : ~o;
  return __uint_as_float(u);
}

// ---------------------------------------------------------------- rounding rules several kernels share
// Kernels that must agree bit for bit (a fused epilogue and the separate pass it replaces, the e4m3 producers, every residual add) call
// ONE definition here; written in the flavour primitives only, so bf16 and fp16 stay the same source.  "16-bit" = the flavour's type.
template <typename T> __device__ __forceinline__ float round_elt(float v) {          // v as the engine's T holds it
  if constexpr (sizeof(T) == 2) return bf2f(f2bf(v));
  else return v;
}

// x * rs of the RMSNorm kernels as T holds it: the product is an fp32 value of its own, then rounded to T.  fp16 flavour: left to itself the
// compiler folds product and conversion into one v_fma_mixlo_f16 in one instantiation of a kernel and keeps v_mul_f32 + v_cvt_f16_f32 in
// another (splitk_resid_rmsnorm_kernel with / without QUANT), and the two did not give the same bits on every element
// (tests/test_segs_gpu.py::test_gemm_fp8_resid_norm); the empty asm keeps the product in a register of its own.
template <typename T> __device__ __forceinline__ float norm_scale(float x, float rs) {
  float p = x * rs;
#ifdef ATS_F16_FLAVOUR
  asm("" : "+v"(p));
#endif
  return round_elt<T>(p);
}

// The rotary pair (x0, x1) = (x[d], x[d + head_dim/2]) of the 16-bit engine, with the contraction spelled out: the separate RoPE pass, the
// slab-summing one and the qkv GEMMs' fused epilogues must round identically (the compiler is otherwise free to pick which product it fuses).
__device__ __forceinline__ float rope_first(float x0, float x1, float c, float s) { return __fmaf_rn(x0, c, -__fmul_rn(x1, s)); }    // x0 cos - x1 sin
__device__ __forceinline__ float rope_second(float x0, float x1, float c, float s) { return __fmaf_rn(x1, c, __fmul_rn(x0, s)); }    // x1 cos + x0 sin
// two pairs at once: x = 16-bit (x[d], x[d+1]), y = (x[d + half], x[d+1 + half]), i.e. the projection's rounded outputs; the rotation in fp32
// on those, one more rounding.  Returns (rotated x, rotated y).
__device__ __forceinline__ uint2 rope_pk(uint32_t x, uint32_t y, float c0, float s0, float c1, float s1) {
  return make_uint2(f2bf_pk(rope_first(bf_lo(x), bf_lo(y), c0, s0), rope_first(bf_hi(x), bf_hi(y), c1, s1)),
                    f2bf_pk(rope_second(bf_lo(x), bf_lo(y), c0, s0), rope_second(bf_hi(x), bf_hi(y), c1, s1)));
}
// four pairs: the form of the GEMM epilogues (a lane holds four adjacent columns and their partners)
__device__ __forceinline__ void rope_pk(const uint2& x, const uint2& y, const float4& c, const float4& s, uint2& first, uint2& second) {
  const uint2 a = rope_pk(x.x, y.x, c.x, s.x, c.y, s.y), b = rope_pk(x.y, y.y, c.z, s.z, c.w, s.w);
  first = make_uint2(a.x, b.x);
  second = make_uint2(a.y, b.y);
}
// rotation index of a token position: clamped to the cos / sin tables
__device__ __forceinline__ int rope_pos(int ps, int max_pos) { return ps < 0 ? 0 : (ps >= max_pos ? max_pos - 1 : ps); }
// row `slot` of one layer's K or V cache (cache = the user's layer-0 base, H elements per row)
template <typename T = bf16_t> __device__ __forceinline__ T* kv_row(void* cache, size_t layer_off, int slot, int H) {
  return reinterpret_cast<T*>(reinterpret_cast<char*>(cache) + layer_off) + (size_t)slot * H;
}

// Residual add h = round(h + round(proj)): the projection's output is a T tensor before the add (HF: o_proj / down_proj return the dtype).
__device__ __forceinline__ uint32_t resid_pk(uint32_t h, uint32_t p) { return f2bf_pk(bf_lo(h) + bf_lo(p), bf_hi(h) + bf_hi(p)); }
template <typename T> __device__ __forceinline__ float resid_add(T* h, float proj) {   // in memory; returns what *h now holds
  const float v = Elt<T>::load(h) + round_elt<T>(proj);
  Elt<T>::store(h, v);
  return round_elt<T>(v);
}

// LoRA side path beside a q / k / v projection (lora.hip; peft's `result + lora_B(lora_A(x)) * scaling` in T with fp32 accumulation inside
// each matmul).  Every intermediate is a T tensor:
//   u = round(sum_k xn[k] A[j][k])            lora_A's output: lora_u<T> of the fp32 sum (xn = the layer's RMSNorm output as rmsnorm_kernel rounds it)
//   d = round(sum_j u[j] B[c][j])             lora_B's output
//   y = round(base16 + round(scaling * d))    base16 = the projection's T output; RoPE (rope_pk) then works on y
// lora_add takes the fp32 sum of d.  The fp32 engine (parity mode) rounds nothing.
template <typename T> __device__ __forceinline__ float lora_u(float acc) { return round_elt<T>(acc); }
template <typename T> __device__ __forceinline__ float lora_add(float base16, float d_acc, float scaling) {
  float p = scaling * round_elt<T>(d_acc);
  if constexpr (sizeof(T) == 2) {
    asm("" : "+v"(p));                       // the scaled product is a value of its own before it is rounded (as norm_scale)
    return round_elt<T>(base16 + round_elt<T>(p));
  } else return base16 + p;
}

// SwiGLU: gate and up rounded to T first (the reference's two projections are T tensors), SiLU and the product in fp32, one rounding.  The
// fp32 engine (parity mode) rounds nothing and takes the exact quotient.
__device__ __forceinline__ uint32_t swiglu_pk(float g0, float g1, float u0, float u1) {
  const uint32_t gp = f2bf_pk(g0, g1), up = f2bf_pk(u0, u1);
  return f2bf_pk(ats_silu<false>(bf_lo(gp)) * bf_lo(up), ats_silu<false>(bf_hi(gp)) * bf_hi(up));
}
template <typename T> __device__ __forceinline__ float swiglu(float g, float u) {      // the caller's store rounds
  return ats_silu<sizeof(T) == 4>(round_elt<T>(g)) * round_elt<T>(u);
}
// four adjacent accumulators -> two packed 16-bit words (a lane's four columns of a row); the (gate, up) form: four SwiGLU outputs
__device__ __forceinline__ uint2 f2bf_pk4(float a, float b, float c, float d) { return make_uint2(f2bf_pk(a, b), f2bf_pk(c, d)); }
__device__ __forceinline__ uint2 f2bf_pk4(const f32x4_t& v) { return f2bf_pk4(v[0], v[1], v[2], v[3]); }
__device__ __forceinline__ uint2 swiglu_pk4(const f32x4_t& g, const f32x4_t& u) {
  return make_uint2(swiglu_pk(g[0], g[1], u[0], u[1]), swiglu_pk(g[2], g[3], u[2], u[3]));
}

// Online softmax: (mx, sm) = running maximum and sum of exp(x - mx); merged with another such pair (om, os).  Two empty pairs stay empty.
__device__ __forceinline__ void lse_merge(float& mx, float& sm, float om, float os) {
  const float nm = fmaxf(mx, om);
  sm = (nm > -INFINITY) ? sm * __expf(mx - nm) + os * __expf(om - nm) : 0.f;
  mx = nm;
}

// OCP e4m3 with a per-row scale: scale = max|x| / 448 (1 for an all-zero row), q = e4m3(clamp(x / scale, +-448)), x the 16-bit-rounded value
// (the fused producers quantise what the separate pass would read back).  inv = 1 / scale.
__device__ __forceinline__ float e4m3_scale(float amax) { return amax > 0.f ? amax * (1.0f / 448.0f) : 1.0f; }
__device__ __forceinline__ float e4m3_fit(float f, float inv) { return fminf(fmaxf(f * inv, -448.f), 448.f); }
__device__ __forceinline__ uint32_t e4m3_cvt4(float c0, float c1, float c2, float c3) {  // four fitted values -> four bytes, the first lowest
  int w = 0;
  w = __builtin_amdgcn_cvt_pk_fp8_f32(c0, c1, w, false);
  w = __builtin_amdgcn_cvt_pk_fp8_f32(c2, c3, w, true);
  return (uint32_t)w;
}
__device__ __forceinline__ uint32_t e4m3_pk4(float f0, float f1, float f2, float f3, float inv) {
  return e4m3_cvt4(e4m3_fit(f0, inv), e4m3_fit(f1, inv), e4m3_fit(f2, inv), e4m3_fit(f3, inv));
}
__device__ __forceinline__ uint2 e4m3_pk8(const uint4& v, float inv) {                  // v: eight 16-bit values
  const bf16_t* e = reinterpret_cast<const bf16_t*>(&v);
  float f[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) f[j] = e4m3_fit(bf2f(e[j]), inv);
  return make_uint2(e4m3_cvt4(f[0], f[1], f[2], f[3]), e4m3_cvt4(f[4], f[5], f[6], f[7]));
}

// Four adjacent columns gn .. gn + 3 of a row, p = the address of column gn: one vector store if all four are inside N and the stride allows
// it (vec), else element by element up to N.  16-bit: packed conversions; RESID: the residual add on what p holds.
__device__ __forceinline__ void store4(float* p, const f32x4_t& v, int gn, int N, bool vec) {
  if (gn + 3 < N && vec) *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  else
#pragma unroll
    for (int r = 0; r < 4; ++r) if (gn + r < N) p[r] = v[r];
}
template <bool RESID = false>
__device__ __forceinline__ void store4(bf16_t* p, const f32x4_t& v, int gn, int N, bool vec) {
  if (gn + 3 < N && vec) {
    uint2 o = f2bf_pk4(v);
    if constexpr (RESID) { const uint2 h = *reinterpret_cast<const uint2*>(p); o.x = resid_pk(h.x, o.x); o.y = resid_pk(h.y, o.y); }
    *reinterpret_cast<uint2*>(p) = o;
  } else {
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (gn + r < N) {
        if constexpr (RESID) resid_add(p + r, v[r]);
        else p[r] = f2bf(v[r]);
      }
  }
}
// A GEMM epilogue's output by its kind, c = the output's base and idx the element: fp32 store (F32), residual add on what c holds (RESID),
// else a plain store as T.  One value; and a lane's four adjacent columns (store4's arguments).
template <typename T, bool F32, bool RESID> __device__ __forceinline__ void store_epi(void* c, size_t idx, float v) {
  if constexpr (F32) reinterpret_cast<float*>(c)[idx] = v;
  else if constexpr (RESID) resid_add(reinterpret_cast<T*>(c) + idx, v);
  else Elt<T>::store(reinterpret_cast<T*>(c) + idx, v);
}
template <bool F32, bool RESID> __device__ __forceinline__ void store4_epi(void* c, size_t idx, const f32x4_t& v, int gn, int N, bool vec) {
  if constexpr (F32) store4(reinterpret_cast<float*>(c) + idx, v, gn, N, vec);
  else store4<RESID>(reinterpret_cast<bf16_t*>(c) + idx, v, gn, N, vec);
}

// Sum / maximum over a workgroup of NW waves through its __shared__ red[NW].  The per-wave partials are combined left to right, ((r0 + r1) + r2) + ...:
// the RMSNorm statistics depend on that order.  block_put + barrier + red_*: for a kernel that reduces two values behind one barrier.
// None of them opens with a barrier: a caller that reuses red[] while lanes may still read the previous result puts one in front.
template <int NW> __device__ __forceinline__ void block_put(float wave_value, float (&red)[NW]) { if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = wave_value; }
template <int NW> __device__ __forceinline__ float red_sum(const float (&red)[NW]) {
  float t = red[0];
#pragma unroll
  for (int w = 1; w < NW; ++w) t += red[w];
  return t;
}
template <int NW> __device__ __forceinline__ float red_max(const float (&red)[NW]) {
  float t = red[0];
#pragma unroll
  for (int w = 1; w < NW; ++w) t = fmaxf(t, red[w]);
  return t;
}
template <int NW> __device__ __forceinline__ float block_sum(float v, float (&red)[NW]) {
  v = wave_sum_f32(v);
  block_put(v, red);
  __syncthreads();
  return red_sum(red);
}
template <int NW> __device__ __forceinline__ float block_max(float v, float (&red)[NW]) {
  v = wave_max_f32(v);
  block_put(v, red);
  __syncthreads();
  return red_max(red);
}
// the same two for uint32_t (counts, ford keys): exact, so no order to keep
template <int NW> __device__ __forceinline__ uint32_t block_sum(uint32_t v, uint32_t (&red)[NW]) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  uint32_t t = red[0];
#pragma unroll
  for (int w = 1; w < NW; ++w) t += red[w];
  return t;
}
template <int NW> __device__ __forceinline__ uint32_t block_max(uint32_t v, uint32_t (&red)[NW]) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { const uint32_t u = (uint32_t)__shfl_xor((int)v, o, 64); v = u > v ? u : v; }
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  uint32_t t = red[0];
#pragma unroll
  for (int w = 1; w < NW; ++w) t = red[w] > t ? red[w] : t;
  return t;
}

// V consecutive floats of every split-K slab, summed in slab order.  The loads of four slabs are issued before their adds: with a runtime
// slab count the plain loop waited out one memory round trip per slab (8 slabs = 8 x ~2 us; seen as 19 us reduce kernels behind
// 15 us GEMMs in the one-user trace).
template <int V>
__device__ __forceinline__ void sum_slabs(const float* __restrict__ p, size_t slab_stride, int splits, float (&acc)[V]) {
  typedef float vf __attribute__((ext_vector_type(V)));
#pragma unroll
  for (int i = 0; i < V; ++i) acc[i] = 0.f;
  int z = 0;
  for (; z + 4 <= splits; z += 4) {
    vf q[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) q[u] = *reinterpret_cast<const vf*>(p + (size_t)(z + u) * slab_stride);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
#pragma unroll
      for (int i = 0; i < V; ++i) acc[i] += q[u][i];
    }
  }
  for (; z < splits; ++z) {
    vf q = *reinterpret_cast<const vf*>(p + (size_t)z * slab_stride);
#pragma unroll
    for (int i = 0; i < V; ++i) acc[i] += q[i];
  }
}
#endif
