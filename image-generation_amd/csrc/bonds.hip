// Bond rows and link overlaps of bit-packed spin rows (include/dvg.h): dvg_packed_bonds ("DVG bonds v1") turns packed spin rows
// into packed rows of the graph's bonds t_e = s_i s_j, dvg_packed_overlap_link ("DVG link overlap v1") counts, over all pairs of
// rows, the spin distance d and the bond distance l together.  Pure bit operations and integer atomics; one stream-ordered
// launch each, no workgroup waiting on another.
#include "common.h"
#include "graph.h"
#include "packed_rows.h"

namespace dvg {

// ---------------------------------------------------------------- bond rows (dvg_packed_bonds)
// A TILE is 64 consecutive rows of the flattened (group, row) index -- one per lane; workgroup b of BD_WAVES waves takes the
// tiles b, b + gridDim.x, ..  (one tile each up to BD_GRID tiles).  Per tile:
//   1. tile_columns_halves (packed_rows.h): the per-spin bit columns in LDS as halves lo[spin] (rows 0..31), lo[n + spin] (rows
//      32..63).
//   2. behind a barrier thread t takes the edges t, t + BD_THREADS, ..: consecutive lanes read consecutive edge_i, edge_j (and
//      quadratic) -- the edge list once per tile, coalesced -- and write the bond's column halves bl[e], bl[E + e] =
//      ~(col_i ^ col_j) ^ flip: flip = 0 in product mode; in satisfied mode all-ones where J_e > 0 (the bond is satisfied where
//      the spins differ), 0 where J_e < 0, and where J_e is neither (+0, -0, NaN) the column is all-ones: t_e = +1 in every row.
//   3. behind a second barrier tile_rows_from_halves with (n, W) replaced by (E, WE) ballots the bond columns back into the
//      words of the tile's rows, dense in bonds_out; bits >= E of the last word come out 0, rows beyond the last are not stored.
// A third barrier ends the tile: the columns are rewritten by the next one.  Every loop is bounded by W, E or WE.
// LDS: 8 (n + E) bytes, 81 KiB on the 1024-spin Zephyr graph (E = 9352); n + E <= BD_MAX_TERMS = 16384 keeps it within 128 KiB.
// Banks (ds_read_b32 / ds_write_b32: dword mod 32 in 32-lane halves): the transposes read and write 32 consecutive dwords; step 2
// writes consecutive dwords and reads lo[i], lo[j] wherever the edge list points -- data-dependent, up to 32-way where a half's
// edges meet on one bank (a hub's edges read one address: a broadcast), and bounded by E / BD_THREADS rounds per tile.
constexpr int BD_WAVES = 16, BD_THREADS = BD_WAVES * 64, BD_MAX_N = 8192, BD_MAX_TERMS = 16384, BD_LDS_MAX = BD_MAX_TERMS * 8;
constexpr int64_t BD_GRID = 1 << 20;

__global__ __launch_bounds__(BD_THREADS) void packed_bonds_kernel(const uint32_t* __restrict__ bits, int64_t rows, int64_t row_stride,
                                                                   int64_t groups, int64_t group_stride, int n, int W, int E, int WE,
                                                                   const int32_t* __restrict__ edge_i, const int32_t* __restrict__ edge_j,
                                                                   const float* __restrict__ J, uint32_t* __restrict__ bonds_out) {
  extern __shared__ __align__(16) unsigned char bd_smem[];
  uint32_t* lo = reinterpret_cast<uint32_t*>(bd_smem);  // [n] rows 0..31 of the tile, then [n] rows 32..63
  uint32_t* bl = lo + 2 * n;                            // [E] rows 0..31 of the bonds, then [E] rows 32..63
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const uint32_t* mine = lane < 32 ? bl : bl + E;  // the halves that hold this lane's bit
  const int64_t total = groups * rows, n_tiles = (total + 63) >> 6;
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int64_t idx = tile * 64 + lane;
    tile_columns_halves<BD_WAVES>(packed_row(bits, idx, total, rows, row_stride, groups, group_stride), W, n, wave, lane, lo);
    __syncthreads();
    for (int e = tid; e < E; e += BD_THREADS) {
      const int i = edge_i[e], j = edge_j[e];
      uint32_t x0 = ~(lo[i] ^ lo[j]), x1 = ~(lo[n + i] ^ lo[n + j]);
      if (J) {
        const float Je = J[e];
        if (Je > 0.0f) x0 = ~x0, x1 = ~x1;
        else if (!(Je < 0.0f)) x0 = ~0u, x1 = ~0u;
      }
      bl[e] = x0;
      bl[E + e] = x1;
    }
    __syncthreads();
    tile_rows_from_halves<BD_WAVES>(mine, WE, E, wave, lane, tile, total, bonds_out);
    __syncthreads();  // (the columns are rewritten by the next tile)
  }
}

// ---------------------------------------------------------------- link overlaps (dvg_packed_overlap_link)
// All pairs (row of A, row of B) of a group, as packed_overlap_kernel (grbm.hip) takes them: a TILE is 64 rows, a UNIT is (group,
// A tile ta, a span of B tiles), a workgroup of 256 threads walks the units `blockIdx.x + i gridDim.x`, and thread (ty, tx) =
// (tid >> 4, tid & 15) keeps the 4 x 4 block of pairs (rows 4 ty .. 4 ty + 3 of A) x (rows 4 tx .. 4 tx + 3 of B).  Here a pair
// has TWO counts: d over the W spin words and l over the WE bond words.  For a tile pair the spin words are staged and counted
// first, then the bond words -- two K loops through the same two LDS tiles (LK_KC = 16 words of the rows at a time, word-major
// T[k][row], the last word masked to n or E, rows beyond the last read as 0), two 4 x 4 accumulators; per word one 128-bit
// read of each tile serves 16 XOR + popcount-accumulate steps.  The bond loop is WE / W of the work (about nine times the spin
// loop on the solver graphs).  Neither tile is kept across tile pairs: both loops restage A, which costs 8 loads a thread
// beside 256 popcounts.
// Self mode (B = A): units take the tiles tb >= ta only and count r < r'.
// Counters, in LDS across the workgroup's units: h[d] and lh[l], 32-bit, += 1; ls[d] and lq[d], 64-bit, += l and l l.  One
// copy each: lanes of a half that meet on one d serialise on ls and lq whatever h does, and the distances of unrelated rows
// spread over about sqrt(n) and sqrt(E) bins.
// FLUSH RULE.  A workgroup adds its nonzero counters onto the outputs with 64-bit integer atomics at its end and after every
// LK_FLUSH_TILES = 2^12 tile pairs = 2^24 pairs at the most since the last flush: no 32-bit counter can pass 2^24.  The 64-bit
// counters cannot wrap anywhere: the host rejects pairs E^2 >= 2^63, and every partial sum of l l (of l a fortiori) over any
// subset of the call's pairs is below that.  Integer addition commutes: the order of the workgroups does not matter.
// LDS: 8 KiB of tiles + 16 (n + 1) + 4 (n + 1) + 4 (E + 1) bytes: 36 KiB on the 512-spin Zephyr graph (four workgroups a CU),
// 152 KiB at the limits n = 4096, E = 16384.
// LDS banks: the tiles are laid out, staged and read exactly as packed_overlap_kernel's (row r of word k at T[k][r ^ 4 k]; its
// comment has the bank walk).  Counter adds: bank = d or l mod 32 (ds_add_u32), 2 d mod 64 (ds_add_u64): data-dependent.
constexpr int LK_THREADS = 256, LK_TILE = 64, LK_KC = 16, LK_MAX_N = 4096, LK_MAX_E = 16384, LK_FLUSH_TILES = 1 << 12;
constexpr int LK_TILE_LDS = 2 * LK_KC * LK_TILE * 4, LK_UNITS = 2048, LK_GRID = 1024;
constexpr int LK_LDS_MAX = LK_TILE_LDS + 20 * (LK_MAX_N + 1) + 4 * (LK_MAX_E + 1);

__device__ __forceinline__ void lk_flush(unsigned long long* ls, unsigned long long* lq, unsigned int* h, unsigned int* lh, int n,
                                         int E, int tid, unsigned long long* __restrict__ hist,
                                         unsigned long long* __restrict__ link_hist, unsigned long long* __restrict__ link_sum,
                                         unsigned long long* __restrict__ link_sq) {
  for (int d = tid; d <= n; d += LK_THREADS) {
    const unsigned int c = h[d];
    if (c) {  // (no pair at d: ls[d] and lq[d] are 0 as well)
      const unsigned long long s = ls[d], q = lq[d];
      atomicAdd(hist + d, (unsigned long long)c);
      if (s) atomicAdd(link_sum + d, s);
      if (q) atomicAdd(link_sq + d, q);
      h[d] = 0u;
      ls[d] = 0ull;
      lq[d] = 0ull;
    }
  }
  for (int l = tid; l <= E; l += LK_THREADS) {
    const unsigned int c = lh[l];
    if (c) {
      atomicAdd(link_hist + l, (unsigned long long)c);
      lh[l] = 0u;
    }
  }
}

// acc[i][j] += popc over the Wx words of (row a0 + 4 ty + i of ag) ^ (row b0 + 4 tx + j of bg), the last word under last_mask
__device__ __forceinline__ void lk_count(unsigned int (&acc)[4][4], uint32_t* As, uint32_t* Bs, const uint32_t* __restrict__ ag,
                                         int64_t a_rs, int64_t a0, int64_t rows_a, const uint32_t* __restrict__ bg, int64_t b_rs,
                                         int64_t b0, int64_t rows_b, int Wx, uint32_t last_mask, int tx, int ty) {
  for (int k0 = 0; k0 < Wx; k0 += LK_KC) {
    const int kc = Wx - k0 < LK_KC ? Wx - k0 : LK_KC, kc4 = (kc + 3) & ~3;
    __syncthreads();  // (the words of the last chunk have been read)
    if (tx < kc4) {
      const int k = k0 + tx;
      const uint32_t m = k == Wx - 1 ? last_mask : ~0u;
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        const int row = ty + 16 * p;
        const int64_t ra = a0 + row, rb = b0 + row;
        As[tx * LK_TILE + (row ^ (4 * tx))] = (tx < kc && ra < rows_a) ? ag[ra * a_rs + k] & m : 0u;
        Bs[tx * LK_TILE + (row ^ (4 * tx))] = (tx < kc && rb < rows_b) ? bg[rb * b_rs + k] & m : 0u;
      }
    }
    __syncthreads();
    for (int kk = 0; kk < kc4; kk += 4) {
#pragma unroll
      for (int k = kk; k < kk + 4; ++k) {
        const uint4 av = *reinterpret_cast<const uint4*>(As + k * LK_TILE + 4 * (ty ^ (k & 15)));
        const uint4 bv = *reinterpret_cast<const uint4*>(Bs + k * LK_TILE + 4 * (tx ^ (k & 15)));
        const uint32_t ar[4] = {av.x, av.y, av.z, av.w}, br[4] = {bv.x, bv.y, bv.z, bv.w};
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[i][j] += __popc(ar[i] ^ br[j]);
      }
    }
  }
}

__global__ __launch_bounds__(LK_THREADS) void packed_overlap_link_kernel(
    const uint32_t* __restrict__ a, const uint32_t* __restrict__ a_bonds, int64_t rows_a, int64_t a_rs, int64_t a_gs, int64_t ab_rs,
    int64_t ab_gs, const uint32_t* __restrict__ b, const uint32_t* __restrict__ b_bonds, int64_t rows_b, int64_t b_rs, int64_t b_gs,
    int64_t bb_rs, int64_t bb_gs, int self, int n, int W, int E, int WE, int64_t nta, int64_t ntb, int64_t span, int64_t ns,
    int64_t units, unsigned long long* __restrict__ hist, unsigned long long* __restrict__ link_hist,
    unsigned long long* __restrict__ link_sum, unsigned long long* __restrict__ link_sq) {
  extern __shared__ __align__(16) unsigned char lk_smem[];
  uint32_t* As = reinterpret_cast<uint32_t*>(lk_smem);  // [LK_KC][64], row r of word k at [k][r ^ 4 k]
  uint32_t* Bs = As + LK_KC * LK_TILE;
  unsigned long long* ls = reinterpret_cast<unsigned long long*>(Bs + LK_KC * LK_TILE);  // [n + 1]
  unsigned long long* lq = ls + (n + 1);                                                 // [n + 1]
  unsigned int* h = reinterpret_cast<unsigned int*>(lq + (n + 1));                       // [n + 1]
  unsigned int* lh = h + (n + 1);                                                        // [E + 1]
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  for (int i = tid; i <= n; i += LK_THREADS) ls[i] = 0ull, lq[i] = 0ull, h[i] = 0u;
  for (int i = tid; i <= E; i += LK_THREADS) lh[i] = 0u;
  const uint32_t spin_mask = (n & 31) ? (1u << (n & 31)) - 1u : ~0u, bond_mask = (E & 31) ? (1u << (E & 31)) - 1u : ~0u;
  int since = 0;  // tile pairs since the last flush
  for (int64_t u = blockIdx.x; u < units; u += gridDim.x) {
    const int64_t s = u % ns, rest = u / ns, ta = rest % nta, g = rest / nta;
    int64_t tb0 = s * span;
    const int64_t tb1 = tb0 + span < ntb ? tb0 + span : ntb;
    if (self && tb0 < ta) tb0 = ta;
    const int64_t a0 = ta * LK_TILE;
    for (int64_t tb = tb0; tb < tb1; ++tb) {
      const int64_t b0 = tb * LK_TILE;
      unsigned int dd[4][4], ll[4][4];
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) dd[i][j] = 0u, ll[i][j] = 0u;
      lk_count(dd, As, Bs, a + g * a_gs, a_rs, a0, rows_a, b + g * b_gs, b_rs, b0, rows_b, W, spin_mask, tx, ty);
      lk_count(ll, As, Bs, a_bonds + g * ab_gs, ab_rs, a0, rows_a, b_bonds + g * bb_gs, bb_rs, b0, rows_b, WE, bond_mask, tx, ty);
      // the tile's 16 pairs of this thread, by their rows inside the tiles: li < na, lj < nb exist; on the diagonal tile of self
      // mode li < lj is counted
      const int na = rows_a - a0 < LK_TILE ? (int)(rows_a - a0) : LK_TILE, nb = rows_b - b0 < LK_TILE ? (int)(rows_b - b0) : LK_TILE;
      const bool diag = self && ta == tb;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int li = 4 * ty + i;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int lj = 4 * tx + j;
          if (li < na && lj < nb && (!diag || li < lj)) {
            const unsigned int d = dd[i][j], l = ll[i][j];
            atomicAdd(h + d, 1u);
            atomicAdd(lh + l, 1u);
            atomicAdd(ls + d, (unsigned long long)l);
            atomicAdd(lq + d, (unsigned long long)l * l);
          }
        }
      }
      if (++since == LK_FLUSH_TILES) {  // (uniform over the workgroup)
        __syncthreads();
        lk_flush(ls, lq, h, lh, n, E, tid, hist, link_hist, link_sum, link_sq);
        since = 0;  // (the next adds sit behind the barriers of the next tile pair's staging)
      }
    }
  }
  __syncthreads();
  lk_flush(ls, lq, h, lh, n, E, tid, hist, link_hist, link_sum, link_sq);
}

}  // namespace dvg

using namespace dvg;

// Bond rows of bit-packed spin rows ("DVG bonds v1", include/dvg.h): packed in, packed out, never unpacked.
extern "C" int dvg_packed_bonds(const dvg_graph_t* g, const float* quadratic, const uint32_t* bits, int64_t rows, int64_t row_stride,
                                int64_t groups, int64_t group_stride, uint32_t* bonds_out, dvg_stream_t stream) {
  DVG_REQUIRE(g, "packed_bonds: g is null");
  DVG_REQUIRE(bits, "packed_bonds: bits is null");
  DVG_REQUIRE(bonds_out, "packed_bonds: bonds_out is null");
  const int n = g->n, E = g->n_edges;
  DVG_REQUIRE(E >= 1, "packed_bonds: the graph has no edge (n_edges=%d)", E);
  const int64_t W = ((int64_t)n + 31) / 32, WE = ((int64_t)E + 31) / 32;
  DVG_TRY(check_row_geometry("packed_bonds", rows, groups, row_stride, W, group_stride));
  DVG_TRY(check_row_count("packed_bonds", rows, groups));
  DVG_TRY(check_spin_count("packed_bonds", n, BD_MAX_N, "the limit of the packed-row entries"));
  if ((int64_t)n + E > BD_MAX_TERMS) {
    set_error("packed_bonds: n=%d + n_edges=%d > %d (a tile's spin and bond columns are kept in %d KiB of LDS)", n, E, BD_MAX_TERMS,
              BD_LDS_MAX / 1024);
    return DVG_E_UNSUPPORTED;
  }
  {
    // the words the input may touch against the words the output holds: they must not meet (behind the row count: a range
    // of 2^62 rows meets everything)
    const __int128 in_words = (__int128)(groups - 1) * group_stride + (__int128)(rows - 1) * row_stride + W;
    const __int128 out_words = (__int128)groups * rows * WE;
    const __int128 a0 = (__int128)(uintptr_t)bits, a1 = a0 + 4 * in_words;
    const __int128 b0 = (__int128)(uintptr_t)bonds_out, b1 = b0 + 4 * out_words;
    DVG_REQUIRE(!(a0 < b1 && b0 < a1), "packed_bonds: bonds_out=%p overlaps the words of bits=%p", (const void*)bonds_out,
                (const void*)bits);
  }
  const int64_t n_tiles = ceil_div(groups * rows, 64);
  hipStream_t s = (hipStream_t)stream;
  const size_t lds = ((size_t)n + (size_t)E) * 8;
  DVG_RAISE_LDS_ABOVE_64K(lds, packed_bonds_kernel, BD_LDS_MAX);
  DVG_LAUNCH(K_GRBM_SUFFSTATS, packed_bonds_kernel, dim3((unsigned)(n_tiles < BD_GRID ? n_tiles : BD_GRID)), dim3(BD_THREADS), lds, s,
             bits, rows, row_stride, groups, group_stride, n, (int)W, E, (int)WE, g->edge_i, g->edge_j, quadratic, bonds_out);
  return DVG_OK;
}

// Spin and bond distances of all pairs of bit-packed rows, exactly ("DVG link overlap v1", include/dvg.h).
extern "C" int dvg_packed_overlap_link(const uint32_t* a, const uint32_t* a_bonds, int64_t rows_a, int64_t a_row_stride,
                                       int64_t a_group_stride, int64_t a_bond_row_stride, int64_t a_bond_group_stride,
                                       const uint32_t* b, const uint32_t* b_bonds, int64_t rows_b, int64_t b_row_stride,
                                       int64_t b_group_stride, int64_t b_bond_row_stride, int64_t b_bond_group_stride, int groups,
                                       int n, int n_edges, int64_t* hist, int64_t* link_hist, int64_t* link_sum, int64_t* link_sq,
                                       int accumulate, dvg_stream_t stream) {
  DVG_REQUIRE(a, "packed_overlap_link: a is null");
  DVG_REQUIRE(a_bonds, "packed_overlap_link: a_bonds is null");
  DVG_REQUIRE(hist, "packed_overlap_link: hist is null");
  DVG_REQUIRE(link_hist, "packed_overlap_link: link_hist is null");
  DVG_REQUIRE(link_sum, "packed_overlap_link: link_sum is null");
  DVG_REQUIRE(link_sq, "packed_overlap_link: link_sq is null");
  DVG_REQUIRE(rows_a >= 1, "packed_overlap_link: rows_a=%lld must be at least 1", (long long)rows_a);
  DVG_REQUIRE(groups >= 1, "packed_overlap_link: groups=%d must be at least 1", groups);
  DVG_REQUIRE(n >= 1, "packed_overlap_link: n=%d must be at least 1", n);
  DVG_REQUIRE(n_edges >= 1, "packed_overlap_link: n_edges=%d must be at least 1", n_edges);
  const int64_t W = ((int64_t)n + 31) / 32, WE = ((int64_t)n_edges + 31) / 32;
  DVG_REQUIRE(a_row_stride >= W, "packed_overlap_link: a_row_stride=%lld is less than the %lld words of a row",
              (long long)a_row_stride, (long long)W);
  DVG_REQUIRE(a_group_stride >= 0, "packed_overlap_link: a_group_stride=%lld is negative", (long long)a_group_stride);
  DVG_REQUIRE(a_bond_row_stride >= WE, "packed_overlap_link: a_bond_row_stride=%lld is less than the %lld words of a bond row",
              (long long)a_bond_row_stride, (long long)WE);
  DVG_REQUIRE(a_bond_group_stride >= 0, "packed_overlap_link: a_bond_group_stride=%lld is negative", (long long)a_bond_group_stride);
  const int self = b == nullptr;
  if (self) {
    b = a, b_bonds = a_bonds, rows_b = rows_a, b_row_stride = a_row_stride, b_group_stride = a_group_stride;
    b_bond_row_stride = a_bond_row_stride, b_bond_group_stride = a_bond_group_stride;
  } else {
    DVG_REQUIRE(b_bonds, "packed_overlap_link: b_bonds is null");
    DVG_REQUIRE(rows_b >= 1, "packed_overlap_link: rows_b=%lld must be at least 1", (long long)rows_b);
    DVG_REQUIRE(b_row_stride >= W, "packed_overlap_link: b_row_stride=%lld is less than the %lld words of a row",
                (long long)b_row_stride, (long long)W);
    DVG_REQUIRE(b_group_stride >= 0, "packed_overlap_link: b_group_stride=%lld is negative", (long long)b_group_stride);
    DVG_REQUIRE(b_bond_row_stride >= WE, "packed_overlap_link: b_bond_row_stride=%lld is less than the %lld words of a bond row",
                (long long)b_bond_row_stride, (long long)WE);
    DVG_REQUIRE(b_bond_group_stride >= 0, "packed_overlap_link: b_bond_group_stride=%lld is negative",
                (long long)b_bond_group_stride);
  }
  if (n > LK_MAX_N || n_edges > LK_MAX_E) {
    set_error("packed_overlap_link: n=%d > %d or n_edges=%d > %d (a workgroup keeps the n + 1 and n_edges + 1 bins of its counters "
              "in %d KiB of LDS)", n, LK_MAX_N, n_edges, LK_MAX_E, LK_LDS_MAX / 1024);
    return DVG_E_UNSUPPORTED;
  }
  if (rows_a >= (1ll << 31)) {
    set_error("packed_overlap_link: rows_a=%lld must be below 2^31, as in packed_overlap", (long long)rows_a);
    return DVG_E_UNSUPPORTED;
  }
  if (rows_b >= (1ll << 31)) {
    set_error("packed_overlap_link: rows_b=%lld must be below 2^31, as in packed_overlap", (long long)rows_b);
    return DVG_E_UNSUPPORTED;
  }
  if ((__int128)rows_a * rows_b * groups >= ((__int128)1 << 62)) {
    set_error("packed_overlap_link: groups=%d x rows_a=%lld x rows_b=%lld pairs are 2^62 or more", groups, (long long)rows_a,
              (long long)rows_b);
    return DVG_E_UNSUPPORTED;
  }
  const __int128 pairs = self ? (__int128)groups * rows_a * (rows_a - 1) / 2 : (__int128)groups * rows_a * rows_b;
  if (pairs * n_edges * n_edges >= ((__int128)1 << 63)) {
    set_error("packed_overlap_link: pairs=%lld x n_edges=%d^2 is 2^63 or more (link_sq would wrap)", (long long)pairs, n_edges);
    return DVG_E_UNSUPPORTED;
  }
  hipStream_t s = (hipStream_t)stream;
  const size_t lds = (size_t)LK_TILE_LDS + 20 * (size_t)(n + 1) + 4 * (size_t)(n_edges + 1);
  // units: (group, A tile, span of B tiles); B is split only as far as it takes to fill the chip
  const int64_t nta = ceil_div(rows_a, LK_TILE), ntb = ceil_div(rows_b, LK_TILE), base = (int64_t)groups * nta;
  int64_t ns = base >= LK_UNITS ? 1 : ceil_div(LK_UNITS, base);
  ns = ns > ntb ? ntb : ns;
  const int64_t span = ceil_div(ntb, ns);
  ns = ceil_div(ntb, span);
  const int64_t units = base * ns;
  DVG_RAISE_LDS_ABOVE_64K(lds, packed_overlap_link_kernel, LK_LDS_MAX);
  if (!accumulate) {
    DVG_CHECK_HIP(hipMemsetAsync(hist, 0, sizeof(int64_t) * (size_t)(n + 1), s));
    DVG_CHECK_HIP(hipMemsetAsync(link_hist, 0, sizeof(int64_t) * (size_t)(n_edges + 1), s));
    DVG_CHECK_HIP(hipMemsetAsync(link_sum, 0, sizeof(int64_t) * (size_t)(n + 1), s));
    DVG_CHECK_HIP(hipMemsetAsync(link_sq, 0, sizeof(int64_t) * (size_t)(n + 1), s));
  }
  DVG_LAUNCH(K_GRBM_SUFFSTATS, packed_overlap_link_kernel, dim3((unsigned)(units < LK_GRID ? units : LK_GRID)), dim3(LK_THREADS), lds,
             s, a, a_bonds, rows_a, a_row_stride, a_group_stride, a_bond_row_stride, a_bond_group_stride, b, b_bonds, rows_b,
             b_row_stride, b_group_stride, b_bond_row_stride, b_bond_group_stride, self, n, (int)W, n_edges, (int)WE, nta, ntb, span, ns,
             units, reinterpret_cast<unsigned long long*>(hist), reinterpret_cast<unsigned long long*>(link_hist),
             reinterpret_cast<unsigned long long*>(link_sum), reinterpret_cast<unsigned long long*>(link_sq));
  return DVG_OK;
}
