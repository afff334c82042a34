// Transforms of the Winograd F(4x4, 3x3) kernels (conv_wino4.hip: forward / data gradient; conv_wino4_wgrad.hip: weight
// gradient), one line of a 6x6 / 4x4 tile at a time, in registers.
//   B^T = [4 0 -5 0 1 0; 0 -4 -4 1 1 0; 0 4 -4 -1 1 0; 0 -2 -1 2 1 0; 0 2 -1 -2 1 0; 0 4 0 -5 0 1]
//   A^T = [1 1 1 1 1 0; 0 1 -1 2 -2 0; 0 1 1 4 4 0; 0 1 -1 8 -8 1]
//   G   = [1/4 0 0; -1/6 -1/6 -1/6; -1/6 1/6 -1/6; 1/24 1/12 1/6; 1/24 -1/12 1/6; 0 0 1]   (conv.h: wino4_pack_entry)
#pragma once
#include "conv_wino_common.h"

namespace dvg {

// B^T x for one line of six (12 operations); ZE: x0 = x5 = 0 (the halo of a 4x4 image)
template <bool ZE>
__device__ __forceinline__ void wino4_in6(float& x0, float& x1, float& x2, float& x3, float& x4, float& x5) {
  const float p = __builtin_fmaf(-4.f, x2, x4), q = __builtin_fmaf(-4.f, x1, x3);
  const float r = x4 - x2, s = x3 - x1;
  float t0, t5;
  if constexpr (ZE) {
    t0 = __builtin_fmaf(-5.f, x2, x4);
    t5 = __builtin_fmaf(-5.f, x3, 4.f * x1);
  } else {
    t0 = __builtin_fmaf(4.f, x0, __builtin_fmaf(-5.f, x2, x4));
    t5 = __builtin_fmaf(4.f, x1, __builtin_fmaf(-5.f, x3, x5));
  }
  x0 = t0; x1 = p + q; x2 = p - q; x3 = __builtin_fmaf(2.f, s, r); x4 = __builtin_fmaf(-2.f, s, r); x5 = t5;
}

// The whole 6x6 patch d of a thread, in place: V = B^T d B as six columns, then six rows; ZE: a 4x4 image, whose patch has the
// zero padding as its ring 0 / 5 (a zero column stays zero)
template <bool ZE>
__device__ __forceinline__ void wino4_zero_ring(float (&d)[36]) {
  if constexpr (ZE) {
#pragma unroll
    for (int e = 0; e < 36; ++e)
      if (e / 6 == 0 || e / 6 == 5 || e % 6 == 0 || e % 6 == 5) d[e] = 0.f;
  }
}
template <bool ZE>
__device__ __forceinline__ void wino4_patch_col(int j, float (&d)[36]) {  // B^T d, column j
  if (ZE && (j == 0 || j == 5)) return;
  wino4_in6<ZE>(d[j], d[6 + j], d[12 + j], d[18 + j], d[24 + j], d[30 + j]);
}
template <bool ZE>
__device__ __forceinline__ void wino4_patch_row(int i, float (&d)[36]) {  // (.) B, row i
  wino4_in6<ZE>(d[6 * i], d[6 * i + 1], d[6 * i + 2], d[6 * i + 3], d[6 * i + 4], d[6 * i + 5]);
}
// entry quads q0 .. q0 + 2 (positions 4 q0 .. 4 q0 + 11: two transformed rows) of the entry at LDS address `entry`
__device__ __forceinline__ void wino4_store_quads(uint32_t entry, int q0, const float (&d)[36]) {
#pragma unroll
  for (int q = q0; q < q0 + 3; ++q) {
    const f32x4 o = {d[4 * q], d[4 * q + 1], d[4 * q + 2], d[4 * q + 3]};
    *reinterpret_cast<lds_f32x4*>((uintptr_t)(entry + (uint32_t)(q * 16))) = o;
  }
}

// Half of it: rows 0-2 (HI = 0: from x0 .. x4) or rows 3-5 (HI = 1: from x1 .. x5) of B^T x, the same operations per row
template <bool ZE, bool HI>
__device__ __forceinline__ void wino4_in3(float x0, float x1, float x2, float x3, float x4, float x5, float& o0, float& o1, float& o2) {
  if constexpr (!HI) {
    const float p = __builtin_fmaf(-4.f, x2, x4), q = __builtin_fmaf(-4.f, x1, x3);
    if constexpr (ZE) o0 = __builtin_fmaf(-5.f, x2, x4);
    else o0 = __builtin_fmaf(4.f, x0, __builtin_fmaf(-5.f, x2, x4));
    o1 = p + q; o2 = p - q;
  } else {
    const float r = x4 - x2, s = x3 - x1;
    o0 = __builtin_fmaf(2.f, s, r); o1 = __builtin_fmaf(-2.f, s, r);
    if constexpr (ZE) o2 = __builtin_fmaf(-5.f, x3, 4.f * x1);
    else o2 = __builtin_fmaf(4.f, x1, __builtin_fmaf(-5.f, x3, x5));
  }
}

__device__ __forceinline__ f32x4 vfma(float k, const f32x4& a, const f32x4& b) {
  f32x4 o;
#pragma unroll
  for (int i = 0; i < 4; ++i) o[i] = __builtin_fmaf(k, a[i], b[i]);
  return o;
}

// A^T m for one line of six accumulator tiles -> four (10 operations per component)
__device__ __forceinline__ void wino4_out6(const f32x4& m0, const f32x4& m1, const f32x4& m2, const f32x4& m3, const f32x4& m4,
                                           const f32x4& m5, f32x4& y0, f32x4& y1, f32x4& y2, f32x4& y3) {
  const f32x4 s1 = m1 + m2, d1 = m1 - m2, s2 = m3 + m4, d2 = m3 - m4;
  y0 = (m0 + s1) + s2;
  y1 = vfma(2.f, d2, d1);
  y2 = vfma(4.f, s2, s1);
  y3 = vfma(8.f, d2, d1) + m5;
}

// T s for one line of four source values behind the x2 upsample, T = B^T P (rows 0, 1, 3, 4, 5; row 2 vanishes): five outputs
// (8 operations); ZE: s0 = s3 = 0 (the halo of a 2x2 source image)
template <bool ZE>
__device__ __forceinline__ void wino4_ups5(float s0, float s1, float s2, float s3, float& t0, float& t1, float& t3, float& t4, float& t5) {
  const float dd = s1 - s2;
  if constexpr (ZE) {
    t0 = __builtin_fmaf(-5.f, s1, s2);
    t5 = __builtin_fmaf(-5.f, s2, 4.f * s1);
  } else {
    t0 = __builtin_fmaf(4.f, s0, __builtin_fmaf(-5.f, s1, s2));
    t5 = __builtin_fmaf(4.f, s1, __builtin_fmaf(-5.f, s2, s3));
  }
  t1 = __builtin_fmaf(-8.f, s1, 2.f * s2);
  t3 = -3.f * dd;
  t4 = dd;
}

// B^T x for one line of six WITHOUT its element 2 (the data gradient behind the upsample multiplies rows 0, 1, 3, 4, 5 only):
// five outputs (11 operations); ZE: x0 = x5 = 0
template <bool ZE>
__device__ __forceinline__ void wino4_in5(float x0, float x1, float x2, float x3, float x4, float x5,
                                          float& t0, float& t1, float& t3, float& t4, float& t5) {
  const float p = __builtin_fmaf(-4.f, x2, x4), q = __builtin_fmaf(-4.f, x1, x3);
  const float r = x4 - x2, s = x3 - x1;
  if constexpr (ZE) {
    t0 = __builtin_fmaf(-5.f, x2, x4);
    t5 = __builtin_fmaf(-5.f, x3, 4.f * x1);
  } else {
    t0 = __builtin_fmaf(4.f, x0, __builtin_fmaf(-5.f, x2, x4));
    t5 = __builtin_fmaf(4.f, x1, __builtin_fmaf(-5.f, x3, x5));
  }
  t1 = p + q; t3 = __builtin_fmaf(2.f, s, r); t4 = __builtin_fmaf(-2.f, s, r);
}

// (Q A^T) m for a line whose element 2 is zero, Q = [1 1 0 0; 0 0 1 1] (the 2x2 sum that is the adjoint of the upsample):
// Q A^T = [1 2 0 3 -1 0; 0 2 0 12 -4 1]: five accumulator tiles -> the two source pixels of the line
__device__ __forceinline__ void wino4_out5q(const f32x4& m0, const f32x4& m1, const f32x4& m3, const f32x4& m4, const f32x4& m5,
                                            f32x4& y0, f32x4& y1) {
  const f32x4 a = m1 + m1;
  y0 = (m0 + a) + vfma(3.f, m3, -m4);
  y1 = (a + m5) + vfma(12.f, m3, -4.f * m4);
}

// A^T m for a line whose element 2 is zero (behind the upsample): five accumulator tiles m0, m1, m3, m4, m5 -> four
__device__ __forceinline__ void wino4_out5(const f32x4& m0, const f32x4& m1, const f32x4& m3, const f32x4& m4, const f32x4& m5,
                                           f32x4& y0, f32x4& y1, f32x4& y2, f32x4& y3) {
  const f32x4 s2 = m3 + m4, d2 = m3 - m4;
  y0 = (m0 + m1) + s2;
  y1 = vfma(2.f, d2, m1);
  y2 = vfma(4.f, s2, m1);
  y3 = vfma(8.f, d2, m1) + m5;
}

// A y for one line of four (the ADJOINT of the output transform: 4x4 gradient tile -> 6x6; 8 operations), in place:
// x0..x3 in, x0..x5 out
__device__ __forceinline__ void wino4_dy6(float& x0, float& x1, float& x2, float& x3, float& x4, float& x5) {
  const float e = x0 + x2, o = x1 + x3;
  const float e2 = __builtin_fmaf(4.f, x2, x0), t = __builtin_fmaf(4.f, x3, x1);
  const float y3 = x3;
  x1 = e + o; x2 = e - o; x3 = __builtin_fmaf(2.f, t, e2); x4 = __builtin_fmaf(-2.f, t, e2); x5 = y3;
}

}  // namespace dvg
