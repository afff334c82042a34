// Micro-benchmark: can the MMD's exact spin Gram run on the FP4 (e2m1) matrix pipe instead of int8?
//   1. exactness + operand map: rows of +-1 packed two features per byte (feature 2i in the low nibble of byte i, +1 = 0x2,
//      -1 = 0xA), lane (r, h) takes the 16 bytes at [row r][16 h] on BOTH sides, the resident side as -2x (nibble ^ 0xE);
//      v_mfma_scale_f32_32x32x64_f8f6f4 with both E8M0 scales 127 must give exactly -2 * (row i . row j); and the pair
//      kernel's form -- inline asm with the scales in registers, the resident side as the B operand -- the same.
//   2. issue rate alone (1 / 2 / 4 accumulator chains), beside the int8 32x32x32 and the bf16 32x32x16 form.
//   3. the pair kernel's mix: G Gram instructions per 64 bf16 32x32x16 on 4 accumulator chains, one wave per SIMD, all CUs:
//      int8 at G = 16 is today's chunk, FP4 at G = 8 the same Gram on the FP4 pipe, G = 0 the floor.
//   hipcc --offload-arch=gfx950 -O3 tools/mfma_fp4_rate.hip -o /tmp/mfma_fp4_rate && /tmp/mfma_fp4_rate
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>
#include <cstdlib>
#include <vector>

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef int i32x16 __attribute__((ext_vector_type(16)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ f32x16 mfma_fp4(i32x4 a, i32x4 b, f32x16 c) {
  const i32x8 a8 = {a[0], a[1], a[2], a[3], 0, 0, 0, 0}, b8 = {b[0], b[1], b[2], b[3], 0, 0, 0, 0};
  return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a8, b8, c, 4, 4, 0, 127, 0, 127);
}

// ---- 1. exactness: one wave, K = 128 (two k-steps), 32 x 32 Gram of packed rows [32][64 bytes] -------------------------------
template <bool ASM>
__global__ __launch_bounds__(64) void gram_check_kernel(const uint8_t* __restrict__ z4, float* __restrict__ out) {
  const int lane = threadIdx.x, r = lane & 31, h = lane >> 5;
  f32x16 c = {0};
  int sc_a = 127, sc_b = 127;
  asm volatile("" : "+v"(sc_a), "+v"(sc_b));
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const i32x4 row = *reinterpret_cast<const i32x4*>(z4 + r * 64 + s * 32 + h * 16);
    if (ASM) {  // A: streamed rows, B: resident rows as -2x
      i32x4 neg = row ^ (i32x4){(int)0xEEEEEEEE, (int)0xEEEEEEEE, (int)0xEEEEEEEE, (int)0xEEEEEEEE};
      // (the compiler keeps no hazard book for inline-asm MFMAs: without this gap behind the vector instruction that wrote
      // `neg` the MFMA read stale operands, 959 of 1024 entries wrong; the kernels' operands are written far from their MFMAs)
      asm volatile("s_nop 15\n\ts_nop 15" : "+v"(neg));
      if (s == 0)
        asm volatile("v_mfma_scale_f32_32x32x64_f8f6f4 %0, %1, %2, 0, %3, %4 op_sel_hi:[0,0,0] cbsz:4 blgp:4"
                     : "=&v"(c) : "v"(row), "v"(neg), "v"(sc_a), "v"(sc_b));
      else
        asm volatile("v_mfma_scale_f32_32x32x64_f8f6f4 %0, %1, %2, %0, %3, %4 op_sel_hi:[0,0,0] cbsz:4 blgp:4"
                     : "+v"(c) : "v"(row), "v"(neg), "v"(sc_a), "v"(sc_b));
    } else {    // A: resident rows as -2x, B: streamed rows
      const i32x4 neg2 = row ^ (i32x4){(int)0xEEEEEEEE, (int)0xEEEEEEEE, (int)0xEEEEEEEE, (int)0xEEEEEEEE};
      c = mfma_fp4(neg2, row, c);
    }
  }
  if (ASM) asm volatile("s_nop 15\n\ts_nop 15" : "+v"(c));  // (the compiler keeps no hazard book for inline-asm MFMAs)
#pragma unroll
  for (int q = 0; q < 16; ++q) out[((q & 3) + 8 * (q >> 2) + 4 * h) * 32 + r] = c[q];   // [A row][B row]
}

// ---- 2. / 3. rates -----------------------------------------------------------------------------------------------------------
// KIND 0 int8 32x32x32, 1 bf16 32x32x16, 2 fp4 32x32x64.  GRAM = Gram instructions per 64 bf16 ones (0: KIND alone, NCH chains).
template <int KIND, int NCH, int GRAM>
__global__ __launch_bounds__(256) void rate_kernel(int iters, int* out) {
  // +-1 / +-2 nibbles on the FP4 side, small ints on the others: the values do not matter to the issue rate, finite ones do
  i32x4 a = {(int)0x2A2A2A2A, (int)0xA2A2A2A2, (int)0x2AA22AA2, (int)0xCC44C4C4}, b = {(int)0x2222AAAA, (int)0xA2A22A2A, (int)0x2A2AA2A2, (int)0xAAAA2222};
  if (KIND == 1) { a = (i32x4){0x3f803f80, 0x3f803f80, 0x3f803f80, 0x3f803f80}; b = a; }
  a[0] ^= (threadIdx.x & 1) << 3;
  i32x16 ci[4];
  f32x16 cf[4], cg[2];
#pragma unroll
  for (int c = 0; c < 4; ++c) { ci[c] = (i32x16){0}; cf[c] = (f32x16){0}; }
  cg[0] = cg[1] = (f32x16){0};
  const bf16x8 ha = __builtin_bit_cast(bf16x8, (i32x4){0x3f803f80, 0x3f803f80, 0x3f803f80, 0x3f803f80});
  for (int it = 0; it < iters; ++it) {
    if (GRAM < 0) {
#pragma unroll
      for (int u = 0; u < 8; ++u)
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
          if (KIND == 0) ci[c] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, b, ci[c], 0, 0, 0);
          if (KIND == 1) cf[c] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), cf[c], 0, 0, 0);
          if (KIND == 2) cf[c] = mfma_fp4(a, b, cf[c]);
        }
    } else {
      // one "chunk": 64 bf16 MFMAs, a Gram instruction after every (64 / GRAM)-th
#pragma unroll
      for (int u = 0; u < 64; ++u) {
        cf[u & 3] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ha, ha, cf[u & 3], 0, 0, 0);
        if (GRAM > 0 && (u % (64 / (GRAM > 0 ? GRAM : 1))) == 0) {
          const int g = (u * 2 / 64) & 1;
          if (KIND == 0) ci[g] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, b, ci[g], 0, 0, 0);
          if (KIND == 2) cg[g] = mfma_fp4(a, b, cg[g]);
        }
        __builtin_amdgcn_sched_barrier(0);
      }
      // keep the accumulators finite over many iterations
#pragma unroll
      for (int c = 0; c < 4; ++c) cf[c][0] = 0.f;
    }
  }
  float acc = 0;
#pragma unroll
  for (int c = 0; c < 4; ++c) acc += (float)ci[c][0] + cf[c][1];
  acc += cg[0][0] + cg[1][0];
  if (acc == 12345.678f) out[0] = 1;
}

static double elapsed_ms(void (*launch)(int, int*), int iters, int* out) {
  hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
  launch(10, out);
  hipEventRecord(e0);
  launch(iters, out);
  hipEventRecord(e1); hipEventSynchronize(e1);
  float ms; hipEventElapsedTime(&ms, e0, e1);
  hipEventDestroy(e0); hipEventDestroy(e1);
  return ms;
}

template <int KIND, int NCH, int GRAM>
void launch_rate(int iters, int* out) { rate_kernel<KIND, NCH, GRAM><<<256, 256>>>(iters, out); }

template <int KIND, int NCH>
void run_alone(const char* name, double ops, int* out) {
  const int iters = 2000;
  const double ms = elapsed_ms(launch_rate<KIND, NCH, -1>, iters, out);
  const double per_simd = (double)iters * 8 * NCH;
  printf("alone  %-26s chains %d : %6.2f ns per MFMA per SIMD, chip %7.1f T(FL)OP/s\n", name, NCH, ms * 1e6 / per_simd,
         per_simd * 1024 * ops / (ms * 1e-3) / 1e12);
}

template <int KIND, int GRAM>
void run_mix(const char* name, int* out) {
  const int iters = 400;
  const double ms = elapsed_ms(launch_rate<KIND, 4, GRAM>, iters, out);
  printf("mix    64 bf16 32x32x16 + %2d %-26s : %8.1f ns per chunk per SIMD (%6.2f ns per instruction)\n", GRAM, name, ms * 1e6 / iters,
         ms * 1e6 / iters / (64 + GRAM));
}

int main() {
  // 1. exactness
  srand(7);
  std::vector<int8_t> z(32 * 128);
  for (auto& v : z) v = (rand() & 1) ? 1 : -1;
  for (int k = 0; k < 128; ++k) z[5 * 128 + k] = z[9 * 128 + k];   // a duplicated row: S = 128
  std::vector<uint8_t> z4(32 * 64);
  for (int r = 0; r < 32; ++r)
    for (int i = 0; i < 64; ++i) {
      const int lo = z[r * 128 + 2 * i] > 0 ? 0x2 : 0xA, hi = z[r * 128 + 2 * i + 1] > 0 ? 0x2 : 0xA;
      z4[r * 64 + i] = (uint8_t)(lo | (hi << 4));
    }
  uint8_t* dz; float* dout; int* out;
  hipMalloc(&dz, z4.size()); hipMalloc(&dout, 32 * 32 * 4); hipMalloc(&out, 4);
  hipMemcpy(dz, z4.data(), z4.size(), hipMemcpyHostToDevice);
  int bad = 0;
  for (int form = 0; form < 2; ++form) {
    if (form == 0) gram_check_kernel<false><<<1, 64>>>(dz, dout);
    else gram_check_kernel<true><<<1, 64>>>(dz, dout);
    std::vector<float> got(32 * 32);
    hipMemcpy(got.data(), dout, 32 * 32 * 4, hipMemcpyDeviceToHost);
    const int mul = -2;
    int nbad = 0;
    for (int i = 0; i < 32; ++i)
      for (int j = 0; j < 32; ++j) {
        int s = 0;
        for (int k = 0; k < 128; ++k) s += z[i * 128 + k] * z[j * 128 + k];
        // (form 1 stores [streamed row][resident row]: the Gram is symmetric)
        if (got[i * 32 + j] != (float)(mul * s)) { if (nbad < 5) printf("  mismatch [%d][%d]: got %g want %d\n", i, j, got[i * 32 + j], mul * s); ++nbad; }
      }
    printf(form == 0 ? "exact  FP4 Gram of +-1 rows (A = -2x by nibble ^ 0xE, scales 127 / 127, K = 128): %d of 1024 entries differ from -2 S\n"
                     : "exact  FP4 Gram of +-1 rows (inline asm, B = -2x, scales 127 / 127 in registers, K = 128): %d of 1024 entries differ from -2 S\n", nbad);
    bad += nbad;
  }

  // 2. alone
  run_alone<0, 1>("i32_32x32x32_i8", 65536, out); run_alone<0, 2>("i32_32x32x32_i8", 65536, out); run_alone<0, 4>("i32_32x32x32_i8", 65536, out);
  run_alone<1, 1>("f32_32x32x16_bf16", 32768, out); run_alone<1, 2>("f32_32x32x16_bf16", 32768, out); run_alone<1, 4>("f32_32x32x16_bf16", 32768, out);
  run_alone<2, 1>("scale_f32_32x32x64 fp4", 131072, out); run_alone<2, 2>("scale_f32_32x32x64 fp4", 131072, out); run_alone<2, 4>("scale_f32_32x32x64 fp4", 131072, out);
  // 3. the pair kernel's mix, each twice (the clock the chip holds is part of the answer)
  for (int rep = 0; rep < 2; ++rep) {
    run_mix<0, 0>("(no Gram)", out);
    run_mix<0, 16>("i32_32x32x32_i8", out);
    run_mix<2, 8>("scale_f32_32x32x64 fp4", out);
    run_mix<0, 8>("i32_32x32x32_i8", out);
    run_mix<2, 16>("scale_f32_32x32x64 fp4", out);
  }
  hipFree(dz); hipFree(dout); hipFree(out);
  return bad != 0;
}
