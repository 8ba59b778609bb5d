// Probe of v_mfma_scale_f32_16x16x128_f8f6f4 with an e2m1 (FP4) A operand (cbsz = 4), an e4m3 B operand (blgp = 0) and per-lane E8M0
// block scales on gfx950 (tuning aid, not part of the product).  Exact small-integer data against a host product.  Checks:
//   1. the lane -> (row, k) map of the FP4 operand, nibble by nibble: one nonzero A element (e2m1 1.0) at (lane, nibble p of its first 16
//      bytes) against a B whose columns 0 / 1 spell k (B[0][k] = (k & 15) + 1, B[1][k] = (k >> 4) + 1, exact in e4m3) -- the output row that
//      lights up is the element's row, columns 0 / 1 its k;
//   2. which lane's scale VGPR scales that element, and which byte of it (opsel 0): one lane at a time gets 2^1 in byte b, the rest unit;
//   3. a full random check (asymmetric B, random e2m1 A, random per-lane scales with random bytes around the live one) a) in the hardware
//      map, b) with A lane group g holding OCP block g (32 consecutive k) and B's bytes placed to meet it.
// Findings (MI355X, ROCm 7): lane l holds row l & 15; nibble p of its 16 bytes is byte p / 2, LOW half first; the k are NOT 32 (l >> 4) + p:
//      lanes  0-15: bytes 0-7 hold k  0..15, bytes 8-15 hold k  32..47      lanes 32-47: k 16..31, 48..63
//      lanes 16-31: bytes 0-7 hold k 64..79, bytes 8-15 hold k 96..111     lanes 48-63: k 80..95, 112..127
//   while the e4m3 B operand keeps the fp8 map (lane l: k = 32 (l >> 4) + j).  Byte 0 of a lane's scale VGPR (opsel 0) scales exactly the 32
//   elements that lane holds, no other lane's.  Consequence (3b): put OCP block g (16 contiguous bytes of the FP4 row) in lane group g and the
//   e4m3 operand of lane group g takes the 16-byte chunks g and 4 + g of its 128-byte k-step -- the F8 form's chunk permutation, kept as is.
// build + run on the GPU box:  hipcc --offload-arch=gfx950 -O3 tools/probe/mx4_probe.hip -o mx4_probe && ./mx4_probe
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <vector>

typedef int v8i __attribute__((ext_vector_type(8)));
typedef float v4f __attribute__((ext_vector_type(4)));

static const float kE2m1[8] = {0.f, 0.5f, 1.f, 1.5f, 2.f, 3.f, 4.f, 6.f};
static float e2m1_to_float(int c) { return (c & 8) ? -kE2m1[c & 7] : kE2m1[c & 7]; }
static float e4m3_to_float(uint8_t v) {
  int s = v >> 7, e = (v >> 3) & 15, m = v & 7;
  float f = e == 0 ? ldexpf((float)m, -9) : ldexpf(1.0f + m / 8.0f, e - 7);
  return s ? -f : f;
}
static uint8_t e4m3_of_small_int(int v) {          // exact for 0..16
  if (v == 0) return 0;
  int e = 0;
  while ((v >> e) > 1) ++e;
  const int m = ((v << 3) >> e) & 7;
  return (uint8_t)(((e + 7) << 3) | m);
}

__global__ void one_mfma(const v8i* a, const v8i* b, const int* sa, v4f* c) {
  v4f acc = {0, 0, 0, 0};
  acc = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a[threadIdx.x], b[threadIdx.x], acc, 4, 0, 0, sa[threadIdx.x], 0, 0x7f7f7f7f);
  c[threadIdx.x] = acc;
}

static void *da, *db, *ds, *dc;
// D[row][col] (row = A row, col = B column) of one MFMA; la: 16 bytes per lane (padded to 32), lb: 32 e4m3 bytes per lane (the fp8 map:
// lane l holds column l & 15, k = 32 (l >> 4) + j, tools/probe/mx16_probe.hip), ls: one scale word per lane
static std::vector<float> run(const std::vector<uint8_t>& la, const std::vector<uint8_t>& lb, const std::vector<int>& ls) {
  (void)hipMemcpy(da, la.data(), 2048, hipMemcpyHostToDevice); (void)hipMemcpy(db, lb.data(), 2048, hipMemcpyHostToDevice);
  (void)hipMemcpy(ds, ls.data(), 256, hipMemcpyHostToDevice);
  one_mfma<<<1, 64>>>((const v8i*)da, (const v8i*)db, (const int*)ds, (v4f*)dc);
  std::vector<float> out(256), d(256);
  (void)hipMemcpy(out.data(), dc, 1024, hipMemcpyDeviceToHost);
  for (int l = 0; l < 64; ++l) for (int reg = 0; reg < 4; ++reg) d[(4 * (l >> 4) + reg) * 16 + (l & 15)] = out[l * 4 + reg];
  return d;
}
static std::vector<uint8_t> lanes_of_b(const std::vector<uint8_t>& B) {
  std::vector<uint8_t> lb(64 * 32);
  for (int l = 0; l < 64; ++l) for (int j = 0; j < 32; ++j) lb[l * 32 + j] = B[(l & 15) * 128 + 32 * (l >> 4) + j];
  return lb;
}

int main() {
  (void)hipMalloc(&da, 2048); (void)hipMalloc(&db, 2048); (void)hipMalloc(&ds, 256); (void)hipMalloc(&dc, 1024);
  // ---- 1. element map
  std::vector<uint8_t> B(16 * 128, 0);
  for (int k = 0; k < 128; ++k) { B[0 * 128 + k] = e4m3_of_small_int((k & 15) + 1); B[1 * 128 + k] = e4m3_of_small_int((k >> 4) + 1); }
  const std::vector<uint8_t> lbk = lanes_of_b(B);
  const std::vector<int> unit(64, 0x7f7f7f7f);
  std::vector<int> row_of(64 * 32, -1), k_of(64 * 32, -1);
  int map_bad = 0;
  for (int l = 0; l < 64; ++l)
    for (int p = 0; p < 32; ++p) {
      std::vector<uint8_t> la(64 * 32, 0);
      la[l * 32 + p / 2] = (uint8_t)(2 << ((p & 1) * 4));     // e2m1 1.0
      const std::vector<float> d = run(la, lbk, unit);
      int hits = 0;
      for (int r = 0; r < 16; ++r)
        if (d[r * 16 + 0] != 0.f) { ++hits; row_of[l * 32 + p] = r; k_of[l * 32 + p] = ((int)d[r * 16 + 0] - 1) + 16 * ((int)d[r * 16 + 1] - 1); }
      const int want_row = l & 15, want_k = 32 * (l >> 4) + p;
      if (hits != 1 || row_of[l * 32 + p] != want_row || k_of[l * 32 + p] != want_k) {
        if (map_bad < 0) printf("  lane %d nibble %d (byte %d, %s half): row %d k %d (hits %d); assumed row %d k %d\n", l, p, p / 2, (p & 1) ? "high" : "low",
                                 row_of[l * 32 + p], k_of[l * 32 + p], hits, want_row, want_k);
        ++map_bad;
      }
    }
  printf("1. e2m1 A map 'lane l: row l & 15, k = 32 (l >> 4) + p, nibble p = byte p / 2, low half first': %s (%d of 2048 nibbles elsewhere)\n",
         map_bad ? "FAIL" : "ok", map_bad);
  // the map as found: per lane group g and 16-nibble half h (bytes 8h .. 8h+7), the first k; every lane must follow it (row l & 15, nibble
  // 16h + q at kstart[g][h] + q, low half of a byte first)
  int kstart[4][2], table_bad = 0;
  for (int g = 0; g < 4; ++g) for (int h = 0; h < 2; ++h) kstart[g][h] = k_of[(16 * g) * 32 + 16 * h];
  for (int l = 0; l < 64; ++l) for (int p = 0; p < 32; ++p)
    if (row_of[l * 32 + p] != (l & 15) || k_of[l * 32 + p] != kstart[l >> 4][p >> 4] + (p & 15)) ++table_bad;
  for (int g = 0; g < 4; ++g) printf("   lanes %2d-%2d: bytes 0-7 hold k %3d..%3d, bytes 8-15 hold k %3d..%3d\n", 16 * g, 16 * g + 15,
                                     kstart[g][0], kstart[g][0] + 15, kstart[g][1], kstart[g][1] + 15);
  printf("1b. every lane follows that table (row l & 15, nibble order low half first): %s (%d nibbles elsewhere)\n", table_bad ? "FAIL" : "ok", table_bad);
  map_bad = table_bad;
  std::vector<int> hw_g(128), hw_p(128);     // hardware k -> (lane group, nibble) of the A operand
  for (int g = 0; g < 4; ++g) for (int p = 0; p < 32; ++p) { const int h = kstart[g][p >> 4] + (p & 15); if (h >= 0 && h < 128) { hw_g[h] = g; hw_p[h] = p; } }
  // ---- 2. scale lane and byte: element (lane l, nibble p) with one lane's scale word at 2^1 in byte b
  int sc_bad = 0;
  for (int l : {0, 5, 17, 38, 63})
    for (int p : {0, 7, 30}) {
      std::vector<uint8_t> la(64 * 32, 0);
      la[l * 32 + p / 2] = (uint8_t)(2 << ((p & 1) * 4));
      const int r = row_of[l * 32 + p];
      if (r < 0) continue;
      for (int b = 0; b < 4; ++b) {
        int who = -1, n = 0;
        for (int L = 0; L < 64; ++L) {
          std::vector<int> ls = unit;
          ls[L] = (int)((0x7f7f7f7fu & ~(0xffu << (8 * b))) | (0x80u << (8 * b)));
          const std::vector<float> d = run(la, lbk, ls);
          if (d[r * 16 + 0] != (float)((k_of[l * 32 + p] & 15) + 1)) { who = L; ++n; }
        }
        const bool ok = b == 0 ? (n == 1 && who == l) : n == 0;
        if (!ok) { ++sc_bad; printf("  element of lane %d nibble %d, scale byte %d: scaled by lane %d (%d lanes act)\n", l, p, b, who, n); }
      }
    }
  printf("2. scale: 'byte 0 of the scale VGPR of the lane that holds the element, no other lane or byte': %s\n", sc_bad ? "FAIL" : "ok");
  // ---- 3. full random check: a) the hardware map with B natural, b) OCP blocks per lane group with B placed through the map
  srand(11);
  std::vector<int> A(16 * 128), S(16 * 4);
  const uint8_t bv[] = {0x00, 0x30, 0x38, 0x3c, 0x40, 0x44, 0xb0, 0xb8, 0xc0, 0x48, 0xc8, 0x50};   // 0, .5, 1, 1.5, 2, 3, -.5, -1, -2, 4, -4, 8
  for (auto& x : A) x = rand() & 15;
  for (int c = 0; c < 16; ++c) for (int k = 0; k < 128; ++k) B[c * 128 + k] = bv[(rand() + 3 * c + k / 32) % 12];   // asymmetric
  for (auto& s : S) s = 124 + rand() % 7;
  int fails = map_bad + sc_bad;
  for (int mode = 0; mode < 2; ++mode) {
    // logical k of A lane group g, nibble p: mode 0 the hardware k itself (kstart table), mode 1 the OCP block order 32 g + p; B's byte j of
    // lane group g' (hardware k 32 g' + j) then holds the logical k of the A nibble that meets it
    auto a_logical = [&](int g, int p) { return mode == 0 ? kstart[g][p >> 4] + (p & 15) : 32 * g + p; };
    std::vector<uint8_t> la(64 * 32, 0), lb(64 * 32);
    std::vector<int> ls(64);
    std::vector<float> ref(256);
    for (int r = 0; r < 16; ++r) for (int c = 0; c < 16; ++c) {
      double s = 0;
      for (int g = 0; g < 4; ++g) for (int p = 0; p < 32; ++p) {
        const int k = a_logical(g, p);
        s += (double)e2m1_to_float(A[r * 128 + k]) * ldexp(1.0, S[r * 4 + g] - 127) * e4m3_to_float(B[c * 128 + k]);
      }
      ref[r * 16 + c] = (float)s;
    }
    for (int l = 0; l < 64; ++l) {
      const int g = l >> 4;
      for (int p = 0; p < 32; ++p) la[l * 32 + p / 2] |= (uint8_t)(A[(l & 15) * 128 + a_logical(g, p)] << ((p & 1) * 4));
      for (int j = 0; j < 32; ++j) { const int h = 32 * g + j; lb[l * 32 + j] = B[(l & 15) * 128 + a_logical(hw_g[h], hw_p[h])]; }
      ls[l] = (int)((((unsigned)rand() * 2654435761u) & ~0xffu) | (unsigned)S[(l & 15) * 4 + g]);
    }
    const std::vector<float> d = run(la, lb, ls);
    int bad = 0;
    for (int i = 0; i < 256; ++i) if (d[i] != ref[i]) { if (bad < 3) printf("  row %d col %d: got %g want %g\n", i / 16, i % 16, d[i], ref[i]); ++bad; }
    printf("3%c. random e2m1 A x asymmetric e4m3 B, random per-lane scales, %s: %s (%d of 256 differ)\n", mode ? 'b' : 'a',
           mode ? "A lane group g = OCP block g (32 consecutive k, 16 contiguous bytes), B bytes permuted by the table" : "A in the hardware map, B natural",
           bad ? "FAIL" : "ok", bad);
    fails += bad;
  }
  return fails ? 1 : 0;
}
