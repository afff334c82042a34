// Zero-temperature descent of bit-packed spin rows to local minima of the energy (dvg_grbm_descend_packed, "DVG descent v1",
// include/dvg.h): colour class by colour class every unstable spin flips, sweep after sweep until a sweep flips nothing or
// max_sweeps have run.  One stream-ordered launch, no workgroup waiting on another, no atomics on global memory.
#include "common.h"
#include "graph.h"
#include "packed_rows.h"
#include <cmath>

namespace dvg {

// A TILE is 64 consecutive rows of the flattened (group, row) index -- one per lane; workgroup b of DS_WAVES waves takes the
// tiles b, b + gridDim.x, ..  A row's result depends on that row alone, so the grid cannot show in any output.
// Per tile: the ballot transpose (tile_columns_halves, packed_rows.h) puts the per-spin bit columns in LDS as halves lo[spin] (rows
// 0..31) and hi[spin] = lo[n + spin] (rows 32..63).  Then the sweeps.  In class k wave v takes the spins order[class_ptr[k] +
// v], order[class_ptr[k] + v + DS_WAVES], ..: a spin is wave-uniform, its CSR row is loaded 64 entries at a time, entry t by
// lane t (neighbour, and the coupling scaled and clamped as the sampler's), and handed out with v_readlane; the neighbour's
// column half is read at one address per 32-lane half (a broadcast), the lane's own bit goes onto the coupling's sign and one
// v_add_f32 adds it: the sampler's float32 field, bit for bit (-ffp-contract=off).  The 64-bit ballot of "unstable" over the
// lanes is the set of rows that flip this spin: lane 0 XORs its halves into lo[i] and hi[i].  No spin of a class reads another
// spin of it, so the waves need no order inside a class; one barrier sits between classes.  Rows beyond the last ride along
// with their ballot bit forced to 0; rows that are at a fixed point ride along and cannot flip.
// The exit: every wave leaves the OR of its ballots of the sweep in its slot moved[sweep parity][wave] before the sweep's last
// barrier; behind it every thread ORs the DS_WAVES slots -- one value for the whole workgroup, so the loop's exit is
// workgroup-uniform and no barrier is reached by a part of it.  (Two sets of slots: a wave may be writing sweep s + 1's while
// another still reads sweep s's; sweep s + 2's are written behind sweep s + 1's barrier.)  A row's `sweeps` is the number of
// sweeps whose OR has its bit; its flips are counted in the lane, per wave, and the waves' counts meet in LDS at the end, as
// the fields kernel's partial sums do.  Only when the last permitted sweep still flipped something (and `unstable` is asked
// for) one more pass over all spins, wave v the spins v, v + DS_WAVES, .., counts the unstable spins without flipping.
// The way back (tile_rows_from_halves, packed_rows.h): wave v takes the row pairs (r, r + 32), r = v, v + DS_WAVES, .., and
// ballots the column halves back into the rows' words.
// LDS: 8 n bytes of columns + DS_WAVES 512 bytes of row counts + 2 DS_WAVES 8 bytes of slots: 8.25 KiB + 8 n bytes, 72.25 KiB at
// n = 8192.  Banks (ds_read_b32 / ds_write_b32: dword mod 32 in 32-lane halves): the transpose writes 32 consecutive dwords;
// the sweeps read one column address per half (a broadcast) and one lane writes; the way back reads 32 consecutive dwords per
// half; the row counts are [wave][lane], consecutive lanes on consecutive dwords; the slots are read at one address by all
// lanes (a broadcast).  No conflict by the rule.
constexpr int DS_WAVES = 16, DS_THREADS = DS_WAVES * 64, DS_MAX_N = 8192, DS_MAX_GRID = 1024, DS_MAX_SWEEPS = 65536;
constexpr int DS_FIXED_LDS = DS_WAVES * 64 * 8 + 2 * DS_WAVES * 8, DS_LDS_MAX = DS_MAX_N * 8 + DS_FIXED_LDS;

// (bits and bits_out may be the same rows: a tile's rows are read whole, behind a barrier, before any of them is written)
__global__ __launch_bounds__(DS_THREADS) void grbm_descend_packed_kernel(
    const uint32_t* bits, int64_t rows, int64_t row_stride, int64_t groups, int64_t group_stride, int n, int W, int n_colours,
    const int32_t* __restrict__ order, const int32_t* __restrict__ class_ptr, const int32_t* __restrict__ adj_ptr,
    const int32_t* __restrict__ adj_idx, const int32_t* __restrict__ adj_eid, const float* __restrict__ h,
    const float* __restrict__ J, float prefactor, float h_lo, float h_hi, float j_lo, float j_hi, int max_sweeps,
    uint32_t* bits_out, int32_t* __restrict__ sweeps_out, int32_t* __restrict__ flips_out, int32_t* __restrict__ unstable_out) {
  extern __shared__ __align__(16) unsigned char ds_smem[];
  unsigned long long* moved = reinterpret_cast<unsigned long long*>(ds_smem);  // [2][DS_WAVES]  the waves' rows that moved
  int* rowf = reinterpret_cast<int*>(moved + 2 * DS_WAVES);                    // [DS_WAVES][64] the waves' flip counts
  int* rowu = rowf + DS_WAVES * 64;                                            // [DS_WAVES][64] the waves' unstable counts
  uint32_t* lo = reinterpret_cast<uint32_t*>(rowu + DS_WAVES * 64);            // [n] rows 0..31 of the tile, then [n] rows 32..63
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const uint32_t* mine = lane < 32 ? lo : lo + n;  // the halves that hold this lane's bit
  const int to_sign = 31 - (lane & 31);
  const int64_t total = groups * rows, n_tiles = (total + 63) >> 6;
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int64_t idx = tile * 64 + lane;
    const bool live = idx < total;
    tile_columns_halves<DS_WAVES>(packed_row(bits, idx, total, rows, row_stride, groups, group_stride), W, n, wave, lane, lo);
    __syncthreads();
    // ---- the sweeps
    int n_sweeps = 0, n_flips = 0, sweep = 0;
    unsigned long long any = 0ull;  // the rows that moved in the last sweep run: one value for the whole workgroup
    for (;;) {
      unsigned long long mv = 0ull;
      for (int k = 0; k < n_colours; ++k) {
        if (k) __syncthreads();
        const int u1 = class_ptr[k + 1];
        for (int u = class_ptr[k] + wave; u < u1; u += DS_WAVES) {
          const int i = order[u];
          const float f = local_field(i, lane, mine, to_sign, adj_ptr, adj_idx, adj_eid, h, J, prefactor, h_lo, h_hi, j_lo, j_hi);
          const bool up = spin_is_up(mine, i, to_sign);
          const bool flip = live && spin_is_unstable(up, f);
          const unsigned long long m = __builtin_amdgcn_ballot_w64(flip);
          n_flips += flip ? 1 : 0;
          if (m != 0ull) {
            if (lane == 0) {
              lo[i] ^= (uint32_t)m;
              lo[n + i] ^= (uint32_t)(m >> 32);
            }
            mv |= m;
          }
        }
      }
      ++sweep;
      unsigned long long* slot = moved + (sweep & 1) * DS_WAVES;
      if (lane == 0) slot[wave] = mv;
      __syncthreads();
      unsigned long long all = slot[0];
#pragma unroll
      for (int v = 1; v < DS_WAVES; ++v) all |= slot[v];
      any = ((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(all >> 32)) << 32) |
            (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)all);
      n_sweeps += (int)((any >> lane) & 1ull);
      if (any == 0ull || sweep >= max_sweeps) break;
    }
    // ---- cut off: the last permitted sweep still flipped something -- count what is left, flipping nothing
    int n_unstable = 0;
    if (unstable_out && any != 0ull) {
      for (int i = wave; i < n; i += DS_WAVES) {
        const float f = local_field(i, lane, mine, to_sign, adj_ptr, adj_idx, adj_eid, h, J, prefactor, h_lo, h_hi, j_lo, j_hi);
        const bool up = spin_is_up(mine, i, to_sign);
        n_unstable += (live && spin_is_unstable(up, f)) ? 1 : 0;
      }
    }
    rowf[wave * 64 + lane] = n_flips;
    rowu[wave * 64 + lane] = n_unstable;
    __syncthreads();
    if (wave == 0 && live) {
      int fl = rowf[lane], un = rowu[lane];
#pragma unroll
      for (int v = 1; v < DS_WAVES; ++v) {
        fl += rowf[v * 64 + lane];
        un += rowu[v * 64 + lane];
      }
      if (sweeps_out) sweeps_out[idx] = n_sweeps;
      if (flips_out) flips_out[idx] = fl;
      if (unstable_out) unstable_out[idx] = un;
    }
    // ---- the way back: column bits to the rows' words
    tile_rows_from_halves<DS_WAVES>(mine, W, n, wave, lane, tile, total, bits_out);
    __syncthreads();  // (the columns, the counts and the slots are rewritten by the next tile)
  }
}

}  // namespace dvg

using namespace dvg;

extern "C" int dvg_grbm_descend_packed(const dvg_graph_t* g, const float* linear, const float* quadratic, float prefactor,
                                       float h_lo, float h_hi, float j_lo, float j_hi, const uint32_t* bits, int64_t rows,
                                       int64_t row_stride, int64_t groups, int64_t group_stride, int max_sweeps,
                                       uint32_t* bits_out, int32_t* sweeps, int32_t* flips, int32_t* unstable,
                                       dvg_stream_t stream) {
  DVG_REQUIRE(g, "grbm_descend_packed: g is null");
  DVG_REQUIRE(linear, "grbm_descend_packed: linear is null");
  DVG_REQUIRE(quadratic, "grbm_descend_packed: quadratic is null");
  DVG_REQUIRE(bits, "grbm_descend_packed: bits is null");
  DVG_REQUIRE(bits_out, "grbm_descend_packed: bits_out is null");
  const int n = g->n;
  const int64_t W = ((int64_t)n + 31) / 32;
  DVG_TRY(check_row_geometry("grbm_descend_packed", rows, groups, row_stride, W, group_stride));
  DVG_REQUIRE(std::isfinite(prefactor), "grbm_descend_packed: prefactor=%g is not finite", (double)prefactor);
  DVG_REQUIRE(max_sweeps >= 1 && max_sweeps <= DS_MAX_SWEEPS, "grbm_descend_packed: max_sweeps=%d must be in 1 .. %d", max_sweeps,
              DS_MAX_SWEEPS);
  {
    // the words the input may touch against the words the output holds; the one permitted meeting is the dense input itself
    const __int128 in_words = (__int128)(groups - 1) * group_stride + (__int128)(rows - 1) * row_stride + W;
    const __int128 out_words = (__int128)groups * rows * W;
    const __int128 a0 = (__int128)(uintptr_t)bits, a1 = a0 + 4 * in_words;
    const __int128 b0 = (__int128)(uintptr_t)bits_out, b1 = b0 + 4 * out_words;
    const bool dense = row_stride == W && (groups == 1 || (__int128)group_stride == (__int128)rows * W);
    DVG_REQUIRE(!(a0 < b1 && b0 < a1) || (a0 == b0 && dense),
                "grbm_descend_packed: bits_out=%p overlaps the words of bits=%p (in place needs bits_out == bits and a dense input: "
                "row_stride == W, group_stride == rows W)", (const void*)bits_out, (const void*)bits);
  }
  DVG_TRY(check_row_count("grbm_descend_packed", rows, groups));
  DVG_TRY(check_spin_count("grbm_descend_packed", n, DS_MAX_N));
  const int64_t n_tiles = ceil_div(groups * rows, 64);
  const int grid = (int)(n_tiles < DS_MAX_GRID ? n_tiles : DS_MAX_GRID);
  hipStream_t s = (hipStream_t)stream;
  const size_t lds = (size_t)n * 8 + (size_t)DS_FIXED_LDS;
  DVG_RAISE_LDS_ABOVE_64K(lds, grbm_descend_packed_kernel, DS_LDS_MAX);
  DVG_LAUNCH_WORK(K_DESCEND, (double)n * (double)(groups * rows), grbm_descend_packed_kernel, dim3((unsigned)grid),
                  dim3(DS_THREADS), lds, s, bits, rows, row_stride, groups, group_stride, n, (int)W, g->n_colours, g->order,
                  g->class_ptr, g->adj_ptr, g->adj_idx, g->adj_eid, linear, quadratic, prefactor, h_lo, h_hi, j_lo, j_hi, max_sweeps,
                  bits_out, sweeps, flips, unstable);
  return DVG_OK;
}
