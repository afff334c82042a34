// What the entries on bit-packed spin rows share (grbm.hip, correlation.hip, fields.hip, descent.hip, quantum.hip): the ballot
// transpose from rows to per-spin bit columns and back, the address of a strided row, the sampler's float32 local field on such
// columns, and the checks of the C entries' row arguments.  A new packed-row entry starts from here.
// The column convention, once: a TILE is 64 rows, one per lane of a wave; bit r of a spin's 64-bit column is the spin's bit in
// row r of the tile; rows beyond the last (pad rows) read as 0; columns of spins >= n are never stored.
// No device function in here holds a barrier: the callers keep their own.
#pragma once
#include "common.h"

namespace dvg {

// ---------------------------------------------------------------- device
// Lane r holds `word`, word w of row r: 32 ballots give the columns of spins 32 w .. 32 w + 31; lane b < 32 keeps bit b's.
__device__ __forceinline__ unsigned long long bit_column(uint32_t word, int lane) {
  unsigned long long col = 0ull;
#pragma unroll
  for (int b = 0; b < 32; ++b) {
    const unsigned long long m = __builtin_amdgcn_ballot_w64(((word >> b) & 1u) != 0u);
    if (lane == b) col = m;
  }
  return col;
}

// Row idx of the `total` = groups x rows flattened (group, row) rows, reached through the strides (in words); null beyond the last.
__device__ __forceinline__ const uint32_t* packed_row(const uint32_t* bits, int64_t idx, int64_t total, int64_t rows,
                                                      int64_t row_stride, int64_t groups, int64_t group_stride) {
  const uint32_t* row = nullptr;
  if (idx < total) {
    const int64_t g = groups == 1 ? 0 : idx / rows;
    row = bits + g * group_stride + (idx - g * rows) * row_stride;
  }
  return row;
}

// The whole tile (lane r holds `row`, null for a pad row) as column halves in LDS: lo[spin] rows 0..31, lo[n + spin] rows 32..63;
// lane r only ever needs the half that holds its own bit.  Wave `wave` of WAVES takes the words wave, wave + WAVES, ..
template <int WAVES>
__device__ __forceinline__ void tile_columns_halves(const uint32_t* row, int W, int n, int wave, int lane, uint32_t* lo) {
  for (int w = wave; w < W; w += WAVES) {
    const uint32_t word = row ? row[w] : 0u;
    const unsigned long long col = bit_column(word, lane);
    const int i = 32 * w + lane;
    if (lane < 32 && i < n) {
      lo[i] = (uint32_t)col;
      lo[n + i] = (uint32_t)(col >> 32);
    }
  }
}

// The way back: the column halves of the tile `tile` to the words of its rows, dense in bits_out ([total][W]).  Wave `wave` of
// WAVES takes the row pairs (r, r + 32), r = wave, wave + WAVES, ..; for word w lane l reads column half lo[32 w + l] (l < 32) or
// lo[n + 32 w + l - 32] (0 for spins >= n: the pad bits), the ballot of bit r is word w of row r (low half) and of row r + 32
// (high half), kept by lane w mod 32 of either half; after 32 words (or the last) lanes 0..31 store consecutive words of row
// r, lanes 32..63 of row r + 32.  `mine`: the halves that hold the lane's bit.  Rows beyond `total` are not stored.
template <int WAVES>
__device__ __forceinline__ void tile_rows_from_halves(const uint32_t* mine, int W, int n, int wave, int lane, int64_t tile,
                                                      int64_t total, uint32_t* bits_out) {
  const int half = lane & 31;
  for (int r = wave; r < 32; r += WAVES) {
    const int64_t ridx = tile * 64 + r + (lane < 32 ? 0 : 32);
    uint32_t* dst = bits_out + ridx * W;
    for (int w0 = 0; w0 < W; w0 += 32) {
      const int nw = W - w0 < 32 ? W - w0 : 32;
      uint32_t word = 0u;
      for (int w = 0; w < nw; ++w) {
        const int i = 32 * (w0 + w) + half;
        const uint32_t c = i < n ? mine[i] : 0u;
        const unsigned long long m = __builtin_amdgcn_ballot_w64(((c >> r) & 1u) != 0u);
        if (half == w) word = lane < 32 ? (uint32_t)m : (uint32_t)(m >> 32);
      }
      if (half < nw && ridx < total) dst[w0 + half] = word;
    }
  }
}

// clamp(rn(prefactor x), lo, hi): the sampler's scaled, clamped h_i or J_e
__device__ __forceinline__ float scaled_clamped(float prefactor, float x, float lo, float hi) {
  return fminf(fmaxf(__fmul_rn(prefactor, x), lo), hi);
}

// s_i = +1 in this lane's row: `mine` the column halves that hold the lane's bit, to_sign = 31 - (lane mod 32)
__device__ __forceinline__ bool spin_is_up(const uint32_t* mine, int i, int to_sign) {
  return ((mine[i] << to_sign) & 0x80000000u) != 0u;
}

// s_i f_i > 0: the flip lowers the energy (f_i = 0 is stable)
__device__ __forceinline__ bool spin_is_unstable(bool up, float f) { return up ? f > 0.0f : f < 0.0f; }

// The sampler's float32 local field of the wave-uniform spin i for the 64 rows of the tile, one per lane, bit for bit
// (-ffp-contract=off): the CSR row is loaded 64 entries at a time, entry t by lane t (neighbour, and the coupling scaled and
// clamped), and handed out with v_readlane; the neighbour's column half is read at one address per 32-lane half (a broadcast),
// the lane's own bit goes onto the coupling's sign and one v_add_f32 adds it, in the order of the CSR row.
__device__ __forceinline__ float local_field(int i, int lane, const uint32_t* mine, int to_sign, const int32_t* __restrict__ adj_ptr,
                                             const int32_t* __restrict__ adj_idx, const int32_t* __restrict__ adj_eid,
                                             const float* __restrict__ h, const float* __restrict__ J, float prefactor, float h_lo,
                                             float h_hi, float j_lo, float j_hi) {
  const int p0 = adj_ptr[i], p1 = adj_ptr[i + 1];
  float f = scaled_clamped(prefactor, h[i], h_lo, h_hi);
  for (int c0 = p0; c0 < p1; c0 += 64) {
    const int cnt = p1 - c0 < 64 ? p1 - c0 : 64;
    int jj = 0;
    uint32_t Jv = 0u;
    if (lane < cnt) {
      jj = adj_idx[c0 + lane];
      Jv = __float_as_uint(scaled_clamped(prefactor, J[adj_eid[c0 + lane]], j_lo, j_hi));
    }
    for (int k = 0; k < cnt; ++k) {
      const int j = __builtin_amdgcn_readlane(jj, k);
      const uint32_t w = (uint32_t)__builtin_amdgcn_readlane((int)Jv, k);
      f = __fadd_rn(f, __uint_as_float(w ^ ((~mine[j] << to_sign) & 0x80000000u)));  // s_j > 0 ? Js : -Js
    }
  }
  return f;
}

// ---------------------------------------------------------------- host: the checks of the C entries, `name` the entry's
// DVG_E_INVALID: the geometry of the rows, W the words of a row
static inline int check_row_geometry(const char* name, int64_t rows, int64_t groups, int64_t row_stride, int64_t W,
                                     int64_t group_stride) {
  DVG_REQUIRE(rows >= 1, "%s: rows=%lld must be at least 1", name, (long long)rows);
  DVG_REQUIRE(groups >= 1, "%s: groups=%lld must be at least 1", name, (long long)groups);
  DVG_REQUIRE(row_stride >= W, "%s: row_stride=%lld is less than the %lld words of a row", name, (long long)row_stride,
              (long long)W);
  DVG_REQUIRE(group_stride >= 0, "%s: group_stride=%lld is negative", name, (long long)group_stride);
  return DVG_OK;
}

// DVG_E_UNSUPPORTED: more rows than an index holds
static inline int check_row_count(const char* name, int64_t rows, int64_t groups) {
  if ((__int128)groups * rows >= ((__int128)1 << 62)) {
    set_error("%s: groups=%lld x rows=%lld rows are 2^62 or more", name, (long long)groups, (long long)rows);
    return DVG_E_UNSUPPORTED;
  }
  return DVG_OK;
}

// DVG_E_UNSUPPORTED: more spins than max_n; `why` in place of the LDS of a tile's columns where another limit is meant
static inline int check_spin_count(const char* name, int n, int max_n, const char* why = nullptr) {
  if (n > max_n) {
    if (why) set_error("%s: n=%d > %d (%s)", name, n, max_n, why);
    else set_error("%s: n=%d > %d (a tile's bit columns are kept in %d KiB of LDS)", name, n, max_n, max_n * 8 / 1024);
    return DVG_E_UNSUPPORTED;
  }
  return DVG_OK;
}

// A launch with more than 64 KiB of dynamic LDS: raise the kernel's limit to max_bytes, once per device and call site.
#define DVG_RAISE_LDS_ABOVE_64K(lds, kernel, max_bytes)                                                    \
  do {                                                                                                     \
    static std::atomic<uint64_t> attr_done{0};                                                             \
    if ((lds) > 64 * 1024) DVG_TRY(dvg::raise_dynamic_lds(attr_done, (const void*)(kernel), (max_bytes))); \
  } while (0)

}  // namespace dvg
