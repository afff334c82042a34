// Local fields of bit-packed spin rows and what follows from them spin by spin (dvg_grbm_fields_packed, "DVG fields v1",
// include/dvg.h): the pseudo-log-likelihood of a row, its number of unstable spins, the Rao-Blackwellised moment sums and the
// fields themselves.  Two stream-ordered launches (the second only for the pooled sums), no workgroup waiting on another.
#include "common.h"
#include "graph.h"
#include "packed_rows.h"
#include <cmath>

namespace dvg {

// ---------------------------------------------------------------- 1. rows: fields, per-row outputs, per-slab pooled sums
// A TILE is 64 consecutive rows of the flattened (group, row) index -- one per lane.  A SLAB is `tiles_per_slab` consecutive
// tiles; workgroup `blockIdx.x` of FP_WAVES waves takes slab blockIdx.x, tile by tile.  The split into slabs is a function of the
// number of tiles alone (fp_slabs below), never of the device.
// Per tile: the ballot transpose (tile_columns_halves, packed_rows.h) puts the per-spin bit columns in LDS as halves lo[spin] (rows
// 0..31) and hi[spin] (rows 32..63); behind the barrier the tile's spins are walked in BLOCKS of 64.
//   Phase A, lane = row.  Wave v takes the spins i0 + v, i0 + v + FP_WAVES, .. of the block.  A spin is wave-uniform: its CSR
//   row is loaded 64 entries at a time, entry t by lane t (neighbour, and the coupling scaled and clamped as the sampler's), and
//   handed out with v_readlane; the neighbour's column half is read at one address per 32-lane half (a broadcast), the lane's
//   own bit goes onto the coupling's sign (a shift by 31 - (lane mod 32), a per-lane constant) and one v_add_f32 adds it: the
//   sampler's float32 field, bit for bit (-ffp-contract=off).  Then z, and in float64 e = exp(-|z|), nlp = max(s z, 0) +
//   log1p(e) and m = -+(1 - e) / (1 + e).  The row's nlp and unstable count accumulate in the lane; m (0 for rows beyond the
//   last) and f go to the block's stashes ms[spin][row] and fs[spin][row].
//   Phase B, behind a barrier, lane = a directed CSR entry q = (i -> j) of the block's spins (they are contiguous in the CSR):
//   its owner i by bisection of the block's 65 row pointers (in LDS), j's 64-bit column from LDS, then the 64 rows in order:
//   acc += s_rj m_ri, the sign XORed onto the double's high word -- eight rows at a time, then the eight sums (short chains,
//   small partial sums).  Threads 0..63 of the last wave add up sum_r m_ri of spin i0 + t the same way.  Either sum is added
//   onto the slab's partial in the workspace -- part[slab][i] for spins, part[slab][n + q] for entries -- by the one thread
//   that owns the element in every tile of the slab (the first tile stores): program order, no atomics.  field_out: thread (row, spin) = (t / 64 + FP_WAVES k, t mod 64) stores fs[spin][row]: a wave writes 64
//   consecutive floats of one row, 256 contiguous bytes.
// The waves' per-row partial sums meet in LDS and wave 0 adds them in wave order, as in the energy kernel.
// LDS: 8 n bytes of columns + FP_WAVES 768 bytes of row partials + 64 x 65 doubles (ms) + 64 x 65 floats (fs) + 65 pointers:
// 61.0 KiB + 8 n bytes, 125 KiB at n = 8192.  Banks (ds_read_b32 / ds_write_b32: dword mod 32 in 32-lane halves; ds_read_b64:
// dword mod 64 in 32-lane halves; ds_write_b64: dword mod 32 in groups of 16 lanes): the transpose writes 32 consecutive dwords;
// phase A reads one column address per half (broadcast) and writes ms[i][lane], fs[i][lane], consecutive lanes on consecutive
// elements.  Phase B: consecutive lanes hold consecutive q, so the owners in a 32-lane half are fewer than 32 consecutive
// spins, a stash row is 65 doubles = 130 dwords, and spin u's element r sits at dword 130 u + 2 r = 2 u + 2 r mod 64: fewer than
// 32 consecutive u at one r touch each bank pair at most once, equal u broadcast.  The spin sums read ms[t][r], the same
// pattern with 32 consecutive u.  The field stores read fs[spin][row] at dword 65 spin + row: 32 consecutive spins, each bank
// once.  No conflict by the rule.
// FP_WAVES = 16 against 8, measured: 1024 rows of 1024 spins (16 workgroups, each alone on its CU) 302.7 against 382.3 us,
// 51 200 rows of 512 spins 748.6 against 686.7 us; 16 kept for the size at which the margin over the stock path is thin.
constexpr int FP_WAVES = 16, FP_THREADS = FP_WAVES * 64, FP_MAX_N = 8192, FP_MAX_SLABS = 512, FP_STRIDE = 65;
constexpr int FP_PART_LDS = FP_WAVES * 64 * 12, FP_MS_LDS = 64 * FP_STRIDE * 8, FP_FS_LDS = 64 * FP_STRIDE * 4, FP_PTR_LDS = 272;
constexpr int FP_FIXED_LDS = FP_PART_LDS + FP_MS_LDS + FP_FS_LDS + FP_PTR_LDS, FP_LDS_MAX = FP_MAX_N * 8 + FP_FIXED_LDS;

// m with the sign of bit `r mod 32` of `word` (set: +m, clear: -m), exactly
__device__ __forceinline__ double fp_signed(double m, uint32_t word, int r) {
  const uint32_t flip = (~word << (31 - (r & 31))) & 0x80000000u;
  return __hiloint2double(__double2hiint(m) ^ (int)flip, __double2loint(m));
}

__global__ __launch_bounds__(FP_THREADS) void grbm_fields_packed_kernel(
    const uint32_t* __restrict__ bits, int64_t rows, int64_t row_stride, int64_t groups, int64_t group_stride, int n, int W,
    int n_adj, const int32_t* __restrict__ adj_ptr, const int32_t* __restrict__ adj_idx, const int32_t* __restrict__ adj_eid,
    const float* __restrict__ h, const float* __restrict__ J, float prefactor, float h_lo, float h_hi, float j_lo, float j_hi,
    float two_beta, int64_t tiles_per_slab, double* __restrict__ log_pl, int32_t* __restrict__ unstable,
    double* __restrict__ part, float* __restrict__ field_out) {
  extern __shared__ __align__(16) unsigned char fp_smem[];
  double* ms = reinterpret_cast<double*>(fp_smem);                         // [64][FP_STRIDE]  m of (spin of the block, row)
  double* rowp = ms + 64 * FP_STRIDE;                                      // [FP_WAVES][64]   the waves' nlp sums
  float* fs = reinterpret_cast<float*>(rowp + FP_WAVES * 64);              // [64][FP_STRIDE]  f of (spin of the block, row)
  int* rowu = reinterpret_cast<int*>(fs + 64 * FP_STRIDE);                 // [FP_WAVES][64]   the waves' unstable counts
  int* bptr = rowu + FP_WAVES * 64;                                        // [65 (+3)]        adj_ptr of the block's spins
  uint32_t* lo = reinterpret_cast<uint32_t*>(bptr + FP_PTR_LDS / 4);       // [n] rows 0..31 of the tile, then [n] rows 32..63
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const uint32_t* mine = lane < 32 ? lo : lo + n;  // the halves that hold this lane's bit
  const int to_sign = 31 - (lane & 31);
  const bool want_pl = log_pl != nullptr, want_cond = part != nullptr, want_f = field_out != nullptr;
  const bool want_m = want_pl || want_cond, staged = want_cond || want_f;
  const int64_t total = groups * rows, n_tiles = (total + 63) >> 6;
  const int64_t tile0 = (int64_t)blockIdx.x * tiles_per_slab;
  const int64_t tile1 = tile0 + tiles_per_slab < n_tiles ? tile0 + tiles_per_slab : n_tiles;
  double* slab = want_cond ? part + (int64_t)blockIdx.x * ((int64_t)n + n_adj) : nullptr;
  for (int64_t tile = tile0; tile < tile1; ++tile) {
    const bool first = tile == tile0;
    const int64_t idx = tile * 64 + lane;
    const uint32_t* row = packed_row(bits, idx, total, rows, row_stride, groups, group_stride);  // (null: a row beyond the last)
    tile_columns_halves<FP_WAVES>(row, W, n, wave, lane, lo);
    __syncthreads();
    double nlp_acc = 0.0;
    int unst = 0;
    for (int i0 = 0; i0 < n; i0 += 64) {
      const int nb = n - i0 < 64 ? n - i0 : 64;  // spins of this block
      if (staged && tid <= nb) bptr[tid] = adj_ptr[i0 + tid];
      // ---- phase A: lane = row
      for (int u = wave; u < nb; u += FP_WAVES) {
        const int i = i0 + u;
        const float f = local_field(i, lane, mine, to_sign, adj_ptr, adj_idx, adj_eid, h, J, prefactor, h_lo, h_hi, j_lo, j_hi);
        const bool up = spin_is_up(mine, i, to_sign);
        unst += spin_is_unstable(up, f) ? 1 : 0;
        double m = 0.0;
        if (want_m) {
          const float z = scaled_clamped(two_beta, f, -87.0f, 87.0f);
          const double zd = (double)z, e = exp(-fabs(zd));
          if (want_pl) nlp_acc += fmax(up ? zd : -zd, 0.0) + log1p(e);
          if (want_cond) {
            const double q = (1.0 - e) / (1.0 + e);
            m = row ? (z > 0.0f ? -q : q) : 0.0;
          }
        }
        if (want_cond) ms[u * FP_STRIDE + lane] = m;
        if (want_f) fs[u * FP_STRIDE + lane] = f;
      }
      if (!staged) continue;
      __syncthreads();
      // ---- phase B: lane = a directed entry of the block's spins
      if (want_cond) {
        const int qb = bptr[0], qe = bptr[nb];
        for (int q = qb + tid; q < qe; q += FP_THREADS) {
          int a = 0, b = nb;  // the owner: bptr[a] <= q < bptr[a + 1]
          while (b - a > 1) {
            const int mid = (a + b) >> 1;
            if (bptr[mid] <= q) a = mid; else b = mid;
          }
          const int j = adj_idx[q];
          const uint32_t c_lo = lo[j], c_hi = lo[n + j];
          const double* mrow = ms + a * FP_STRIDE;
          double acc = 0.0;
#pragma unroll
          for (int g8 = 0; g8 < 8; ++g8) {  // eight rows at a time, then the eight sums: short chains, small partial sums
            const uint32_t cw = g8 < 4 ? c_lo : c_hi;
            double t8 = fp_signed(mrow[8 * g8], cw, 8 * g8);
#pragma unroll
            for (int r = 8 * g8 + 1; r < 8 * g8 + 8; ++r) t8 += fp_signed(mrow[r], cw, r);
            acc += t8;
          }
          double* dst = slab + n + q;
          *dst = first ? acc : *dst + acc;
        }
        const int t = tid - (FP_THREADS - 64);
        if (t >= 0 && t < nb) {
          const double* mrow = ms + t * FP_STRIDE;
          double acc = 0.0;
#pragma unroll
          for (int g8 = 0; g8 < 8; ++g8) {
            double t8 = mrow[8 * g8];
#pragma unroll
            for (int r = 8 * g8 + 1; r < 8 * g8 + 8; ++r) t8 += mrow[r];
            acc += t8;
          }
          double* dst = slab + i0 + t;
          *dst = first ? acc : *dst + acc;
        }
      }
      if (want_f && lane < nb) {
        for (int r = wave; r < 64; r += FP_WAVES) {
          const int64_t ridx = tile * 64 + r;
          if (ridx < total) field_out[ridx * n + i0 + lane] = fs[lane * FP_STRIDE + r];
        }
      }
      __syncthreads();  // (the stashes and bptr are rewritten by the next block)
    }
    rowp[wave * 64 + lane] = nlp_acc;
    rowu[wave * 64 + lane] = unst;
    __syncthreads();
    if (wave == 0 && idx < total) {
      double s = rowp[lane];
      int c = rowu[lane];
#pragma unroll
      for (int v = 1; v < FP_WAVES; ++v) {
        s += rowp[v * 64 + lane];
        c += rowu[v * 64 + lane];
      }
      if (want_pl) log_pl[idx] = -s;
      if (unstable) unstable[idx] = c;
    }
    __syncthreads();  // (the columns and the row partials are rewritten by the next tile)
  }
}

// ---------------------------------------------------------------- 2. pooled sums: the slabs' partials in slab order
// Thread x < n: cond_sum[x] (+)= sum over the slabs of part[slab][x].  Thread n + e: cond_pair[e] (+)= sum over the slabs of
// (part[slab][n + q1] + part[slab][n + q2]), q1 / q2 the edge's entry in the CSR row of edge_i[e] / of edge_j[e], found by
// walking the two rows.  The slabs' sum is formed first and added onto the output once.
// sum over the slabs k < slabs of a[k stride] (+ b[k stride]) in a fixed radix-8 tree: eight slabs in order, eight such sums in
// order, eight of those -- FP_MAX_SLABS = 8^3; partial sums stay small, so a pooled sum of T unit addends keeps an error of a few
// T u where one long chain would gather up to T^2 u / 2 on rows that repeat
__device__ __forceinline__ double fp_tree(const double* __restrict__ a, const double* __restrict__ b, int64_t stride, int slabs) {
  double s2 = 0.0;
  for (int k2 = 0; k2 < slabs; k2 += 64) {
    double s1 = 0.0;
    for (int k1 = k2; k1 < slabs && k1 < k2 + 64; k1 += 8) {
      double s0 = 0.0;
      for (int k = k1; k < slabs && k < k1 + 8; ++k) s0 += b ? a[k * stride] + b[k * stride] : a[k * stride];
      s1 += s0;
    }
    s2 += s1;
  }
  return s2;
}
static_assert(FP_MAX_SLABS == 512, "fp_tree is three levels of eight");

__global__ __launch_bounds__(256) void grbm_fields_reduce_kernel(const double* __restrict__ part, int slabs, int n, int n_edges,
                                                                 int n_adj, const int32_t* __restrict__ ei,
                                                                 const int32_t* __restrict__ ej, const int32_t* __restrict__ adj_ptr,
                                                                 const int32_t* __restrict__ adj_eid, double* __restrict__ cond_sum,
                                                                 double* __restrict__ cond_pair, int accumulate) {
  const int x = blockIdx.x * 256 + threadIdx.x;
  if (x >= n + n_edges) return;
  const int64_t stride = (int64_t)n + n_adj;
  double s = 0.0;
  if (x < n) {
    s = fp_tree(part + x, nullptr, stride, slabs);
    cond_sum[x] = accumulate ? cond_sum[x] + s : s;
    return;
  }
  const int e = x - n;
  int q1 = -1, q2 = -1;
  for (int q = adj_ptr[ei[e]]; q < adj_ptr[ei[e] + 1] && q1 < 0; ++q)
    if (adj_eid[q] == e) q1 = q;
  for (int q = adj_ptr[ej[e]]; q < adj_ptr[ej[e] + 1] && q2 < 0; ++q)
    if (adj_eid[q] == e) q2 = q;
  if (q1 >= 0 && q2 >= 0) s = fp_tree(part + n + q1, part + n + q2, stride, slabs);
  cond_pair[e] = accumulate ? cond_pair[e] + s : s;
}

// the slabs of n_tiles tiles: at most FP_MAX_SLABS, each `*tiles_per_slab` consecutive tiles -- a function of n_tiles alone
static inline int fp_slabs(int64_t n_tiles, int64_t* tiles_per_slab) {
  *tiles_per_slab = ceil_div(n_tiles, FP_MAX_SLABS);
  return (int)ceil_div(n_tiles, *tiles_per_slab);
}

static inline bool fp_rows_ok(int64_t rows, int64_t groups) {
  return rows >= 1 && groups >= 1 && (__int128)groups * rows < ((__int128)1 << 62);
}

}  // namespace dvg

using namespace dvg;

extern "C" size_t dvg_grbm_fields_packed_workspace_bytes(const dvg_graph_t* g, int64_t rows, int64_t groups) {
  if (!g || g->n < 1 || g->n > FP_MAX_N || g->n_edges < 0 || !fp_rows_ok(rows, groups)) return 0;
  const int64_t n_tiles = ceil_div(groups * rows, 64);
  const int64_t slabs = n_tiles < FP_MAX_SLABS ? n_tiles : FP_MAX_SLABS;  // (never fewer than the launch uses: monotone in rows)
  return (size_t)slabs * ((size_t)g->n + 2 * (size_t)g->n_edges) * sizeof(double);
}

extern "C" int dvg_grbm_fields_packed(const dvg_graph_t* g, const float* linear, const float* quadratic, float prefactor,
                                      float h_lo, float h_hi, float j_lo, float j_hi, float beta, const uint32_t* bits,
                                      int64_t rows, int64_t row_stride, int64_t groups, int64_t group_stride, double* log_pl,
                                      int32_t* unstable, double* cond_sum, double* cond_pair, float* field_out, int accumulate,
                                      void* ws, size_t ws_bytes, dvg_stream_t stream) {
  DVG_REQUIRE(g, "grbm_fields_packed: g is null");
  DVG_REQUIRE(linear, "grbm_fields_packed: linear is null");
  DVG_REQUIRE(quadratic, "grbm_fields_packed: quadratic is null");
  DVG_REQUIRE(bits, "grbm_fields_packed: bits is null");
  DVG_REQUIRE(log_pl || unstable || cond_sum || cond_pair || field_out,
              "grbm_fields_packed: no output requested (log_pl, unstable, cond_sum with cond_pair and field_out are all null)");
  DVG_REQUIRE((cond_sum != nullptr) == (cond_pair != nullptr),
              "grbm_fields_packed: cond_sum and cond_pair are given together or not at all (%s is null)",
              cond_sum ? "cond_pair" : "cond_sum");
  const bool pooled = cond_sum != nullptr;
  if (pooled) {
    DVG_REQUIRE(ws, "grbm_fields_packed: ws is null (the pooled sums need the workspace)");
    DVG_REQUIRE(((uintptr_t)ws & 15) == 0, "grbm_fields_packed: ws=%p is not aligned to 16 bytes", ws);
  }
  const int n = g->n;
  const int64_t W = ((int64_t)n + 31) / 32;
  DVG_TRY(check_row_geometry("grbm_fields_packed", rows, groups, row_stride, W, group_stride));
  DVG_REQUIRE(std::isfinite(prefactor), "grbm_fields_packed: prefactor=%g is not finite", (double)prefactor);
  DVG_REQUIRE(std::isfinite(beta) && beta >= 0.0f, "grbm_fields_packed: beta=%g must be finite and at least 0", (double)beta);
  DVG_TRY(check_row_count("grbm_fields_packed", rows, groups));
  DVG_TRY(check_spin_count("grbm_fields_packed", n, FP_MAX_N));
  const int64_t n_tiles = ceil_div(groups * rows, 64);
  int64_t tiles_per_slab = 0;
  const int slabs = fp_slabs(n_tiles, &tiles_per_slab);
  const int n_adj = 2 * g->n_edges;
  if (pooled) {
    const size_t need = dvg_grbm_fields_packed_workspace_bytes(g, rows, groups);
    if (ws_bytes < need) {
      set_error("grbm_fields_packed: ws_bytes=%zu is less than the %zu bytes of dvg_grbm_fields_packed_workspace_bytes", ws_bytes, need);
      return DVG_E_WORKSPACE;
    }
  }
  hipStream_t s = (hipStream_t)stream;
  const size_t lds = (size_t)n * 8 + (size_t)FP_FIXED_LDS;
  DVG_RAISE_LDS_ABOVE_64K(lds, grbm_fields_packed_kernel, FP_LDS_MAX);
  const float two_beta = 2.0f * beta;
  DVG_LAUNCH_WORK(K_FIELDS_ROWS, (double)n * (double)(groups * rows), grbm_fields_packed_kernel, dim3((unsigned)slabs),
                  dim3(FP_THREADS), lds, s, bits, rows, row_stride, groups, group_stride, n, (int)W, n_adj, g->adj_ptr, g->adj_idx,
                  g->adj_eid, linear, quadratic, prefactor, h_lo, h_hi, j_lo, j_hi, two_beta, tiles_per_slab, log_pl, unstable,
                  pooled ? reinterpret_cast<double*>(ws) : nullptr, field_out);
  if (pooled)
    DVG_LAUNCH(K_FIELDS_REDUCE, grbm_fields_reduce_kernel, dim3((unsigned)ceil_div((int64_t)n + g->n_edges, 256)), dim3(256), 0, s,
               reinterpret_cast<const double*>(ws), slabs, n, g->n_edges, n_adj, g->edge_i, g->edge_j, g->adj_ptr, g->adj_eid,
               cond_sum, cond_pair, accumulate);
  return DVG_OK;
}
