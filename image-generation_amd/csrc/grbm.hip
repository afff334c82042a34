// GRBM energy and its backward (weighted sufficient statistics).
// Energy: plugin GraphRestrictedBoltzmannMachine.__call__ as used at
// /root/reference/src/losses.py:61;  E(x) = x.h + sum_e J_e x_i x_j.
#include "common.h"
#include "graph.h"
#include "packed_rows.h"

namespace dvg {

// one wavefront per row; double accumulation (cheap here, removes summation-order noise
// from the difference of two means that the quasi-NLL takes)
__global__ __launch_bounds__(256) void grbm_energy_kernel(const float* __restrict__ x, int64_t rows, int n,
                                                          int n_edges, const int32_t* __restrict__ ei,
                                                          const int32_t* __restrict__ ej,
                                                          const float* __restrict__ h,
                                                          const float* __restrict__ J,
                                                          float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const float* xr = x + row * n;
  double acc = 0.0;
  for (int i = lane; i < n; i += 64) acc += (double)xr[i] * (double)h[i];
  for (int e = lane; e < n_edges; e += 64) acc += (double)(xr[ei[e]] * xr[ej[e]]) * (double)J[e];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
  if (lane == 0) out[row] = (float)acc;
}

constexpr int SS_SLABS = 64;

// partial[slab][idx] = sum over the slab's rows of w_r * x_ri (idx < n) or w_r * x_ri x_rj
__global__ __launch_bounds__(256) void grbm_suffstats_partial(const float* __restrict__ x, int64_t rows, int n,
                                                              int n_edges, const int32_t* __restrict__ ei,
                                                              const int32_t* __restrict__ ej,
                                                              const float* __restrict__ w,
                                                              double* __restrict__ partial) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  const int total = n + n_edges;
  if (idx >= total) return;
  const int slab = blockIdx.y;
  const int64_t per = (rows + SS_SLABS - 1) / SS_SLABS;
  const int64_t r0 = slab * per, r1 = (r0 + per < rows) ? r0 + per : rows;
  int a, b;
  if (idx < n) { a = idx; b = -1; } else { a = ei[idx - n]; b = ej[idx - n]; }
  double acc = 0.0;
  for (int64_t r = r0; r < r1; ++r) {
    const float* xr = x + r * n;
    float v = xr[a];
    if (b >= 0) v *= xr[b];
    acc += (double)(w ? w[r] * v : v);
  }
  partial[(size_t)slab * total + idx] = acc;
}

__global__ __launch_bounds__(256) void grbm_suffstats_reduce(const double* __restrict__ partial, int n, int n_edges,
                                                             float scale, float* __restrict__ acc_lin,
                                                             float* __restrict__ acc_quad, int accumulate) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  const int total = n + n_edges;
  if (idx >= total) return;
  double s = 0.0;
  for (int k = 0; k < SS_SLABS; ++k) s += partial[(size_t)k * total + idx];
  float v = (float)(s * (double)scale);
  float* dst = idx < n ? acc_lin + idx : acc_quad + (idx - n);
  *dst = accumulate ? *dst + v : v;
}

// ---------------------------------------------------------------- moments of bit-packed rows (dvg_grbm_moments_packed)
// rows (rows, W) uint32, one bit per spin (the traced draw's records).  A TILE is 64 rows -- one per lane of a wave.  A workgroup
// takes `tiles_per_block` consecutive tiles and turns them into per-spin BIT COLUMNS in LDS, cols[tile][spin] = a 64-bit word
// whose bit r is the spin's bit in row r of the tile: a wave takes (tile, word w) jobs, lane r reads word w of row r (rows
// beyond the last read as 0), and 32 ballots give the columns of spins 32 w .. 32 w + 31, which lanes 0..31 keep one each
// and store side by side.  Behind the barrier a thread walks spins and edges; over the T rows of a tile
//   sum_r s_i = T - 2 popc(~col_i & tail),   sum_r s_i s_j = T - 2 popc((col_i ^ col_j) & tail),   tail = the T low bits,
// summed over the workgroup's tiles in a register, then ONE integer atomic per spin / edge and workgroup: integer addition
// commutes, so the result does not depend on the order the workgroups arrive in.  Columns of spins >= n are never stored.
constexpr int MP_WAVES = 16, MP_LDS = 64 * 1024;

__global__ __launch_bounds__(MP_WAVES * 64) void grbm_moments_packed_kernel(const uint32_t* __restrict__ bits, int64_t rows, int n,
                                                                            int W, int n_edges, const int32_t* __restrict__ ei,
                                                                            const int32_t* __restrict__ ej, int tiles_per_block,
                                                                            unsigned long long* __restrict__ spin_sum,
                                                                            unsigned long long* __restrict__ pair_sum) {
  extern __shared__ __align__(16) unsigned char mp_smem[];
  unsigned long long* cols = reinterpret_cast<unsigned long long*>(mp_smem);  // [tiles_per_block][n]
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int64_t n_tiles = (rows + 63) >> 6;
  const int64_t tile0 = (int64_t)blockIdx.x * tiles_per_block;
  if (tile0 >= n_tiles) return;  // (the whole workgroup: the grid is ceil(n_tiles / tiles_per_block))
  const int kt = (int)(n_tiles - tile0 < tiles_per_block ? n_tiles - tile0 : tiles_per_block);
  for (int job = wave; job < kt * W; job += MP_WAVES) {
    const int k = job / W, w = job - k * W;
    const int64_t r = (tile0 + k) * 64 + lane;
    const unsigned long long col = bit_column(r < rows ? bits[r * W + w] : 0u, lane);
    const int i = 32 * w + lane;
    if (lane < 32 && i < n) cols[(size_t)k * n + i] = col;
  }
  __syncthreads();
  const int64_t rows_here = (rows - tile0 * 64 < (int64_t)kt * 64) ? rows - tile0 * 64 : (int64_t)kt * 64;
  const int last = (int)(rows_here - (int64_t)(kt - 1) * 64);  // rows of the workgroup's last tile: 1..64
  const unsigned long long tail = last >= 64 ? ~0ull : (1ull << last) - 1ull;
  for (int idx = tid; idx < n + n_edges; idx += MP_WAVES * 64) {
    const int a = idx < n ? idx : ei[idx - n], b = idx < n ? -1 : ej[idx - n];
    long long minus = 0;  // rows in which the spin, or the product of the pair, is -1
    for (int k = 0; k < kt; ++k) {
      const unsigned long long ca = cols[(size_t)k * n + a];
      const unsigned long long x = b < 0 ? ~ca : ca ^ cols[(size_t)k * n + b];
      minus += __popcll(k == kt - 1 ? x & tail : x);
    }
    const long long sum = (long long)rows_here - 2 * minus;
    atomicAdd(idx < n ? spin_sum + idx : pair_sum + (idx - n), (unsigned long long)sum);  // (two's complement: the signed sum)
  }
}

// ---------------------------------------------------------------- autocorrelation of bit-packed traces (dvg_trace_autocorr)
// bits (C, M, W) uint32: chain c's record m is a packed row.  A workgroup owns (spin word w, a slab of chains, a chunk of
// AC_LAGS lags) and walks its chains `batch` at a time -- as many as 64 KiB of LDS hold, 16 at the most -- so that a pass's
// loads are all in flight at once and the two barriers of a pass are paid once per batch:
//   transpose  a wave takes a block k of 64 consecutive records, lane r reads word w of record 64 k + r (records >= M read as
//              0), and 32 ballots give the 64-bit TIME columns of spins 32 w .. 32 w + 31 -- the moments kernel's idiom along
//              time instead of across rows -- stored as cols[chain][spin][k], k < K = ceil(M / 64);
//   lags       behind the barrier a 32-lane half wave takes a lag t = 64 a + b and its lanes the 32 spins.  Over the P = M - t
//              pairs (m, m + t):  sum s(m) s(m + t) = P - 2 popc((x ^ (x >> t)) & low(P)),  the shifted column taken word by
//              word as a two-word funnel shift (b == 0: no shift, never one by 64), the word behind the last read as 0, the
//              last word masked to the pairs left -- the zero padding behind record M is never counted as a spin.  The lag
//              t = 0 is the constant P; its half wave counts popc(~x & low(M)) instead: the chain's own sum, M - 2 of it.
// The popcounts of a thread's AC_PER lags stay in registers across the slab; then ONE 64-bit integer atomic per (lag, spin)
// and workgroup.  Integer addition commutes: the result does not depend on the order the workgroups arrive in.
// LDS: a spin's column has a stride of Kp = K | 1 words.  The lag loop's reads are ds_read_b64 of cols[spin][k] at one k
// per 32-lane group: dword 2 Kp spin + 2 k, and Kp odd makes 2 Kp spin mod 64 take the 32 even banks once each -- no
// conflict by the bank rule (bank = dword mod 64, groups of 32 lanes); the transpose's ds_write_b64 (groups of 16 lanes,
// dword mod 32) likewise.
constexpr int AC_WAVES = 16, AC_PER = 8, AC_LAGS = 2 * AC_WAVES * AC_PER, AC_MAX_RECORDS = 16384, AC_BATCH = 16;
constexpr int AC_LDS_MAX = 32 * ((AC_MAX_RECORDS / 64) | 1) * 8;

__global__ __launch_bounds__(AC_WAVES * 64) void trace_autocorr_kernel(const uint32_t* __restrict__ bits, int n_chains, int M,
                                                                       int n, int W, int max_lag, int chains_per_block,
                                                                       int batch, unsigned long long* __restrict__ lag_sum,
                                                                       unsigned long long* __restrict__ spin_sum,
                                                                       int32_t* __restrict__ chain_sum) {
  extern __shared__ __align__(16) unsigned char ac_smem[];
  unsigned long long* cols = reinterpret_cast<unsigned long long*>(ac_smem);  // [batch][32][Kp]
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, half = tid >> 5, sp = tid & 31;
  const int w = blockIdx.x, K = (M + 63) >> 6, Kp = K | 1;
  const int c0 = blockIdx.y * chains_per_block;
  const int c1 = n_chains - c0 < chains_per_block ? n_chains : c0 + chains_per_block;  // (c0 < n_chains: the grid is ceil)
  const int t0 = blockIdx.z * AC_LAGS + half;  // this thread's lags: t0 + 32 r
  const int i = 32 * w + sp;
  unsigned long long minus[AC_PER];  // pairs whose product is -1 (lag 0: records whose spin is -1), over the slab
#pragma unroll
  for (int r = 0; r < AC_PER; ++r) minus[r] = 0ull;
  for (int cb = c0; cb < c1; cb += batch) {
    const int nb = c1 - cb < batch ? c1 - cb : batch;  // the chains of this pass
    for (int job = wave; job < nb * K; job += AC_WAVES) {
      const int j = job / K, k = job - j * K;
      const int m = 64 * k + lane;
      const unsigned long long column = bit_column(m < M ? bits[((int64_t)(cb + j) * M + m) * W + w] : 0u, lane);
      if (lane < 32) cols[(j * 32 + lane) * Kp + k] = column;
    }
    __syncthreads();
    if (i < n) {
#pragma unroll
      for (int r = 0; r < AC_PER; ++r) {
        const int t = t0 + 32 * r;
        if (t > max_lag) break;
        const int P = M - t, a = t >> 6, b = t & 63, nw = (P + 63) >> 6;
        const int rem = P - 64 * (nw - 1);  // pairs of the last word: 1..64
        const unsigned long long tail = rem >= 64 ? ~0ull : (1ull << rem) - 1ull;
#pragma unroll 1
        for (int j = 0; j < nb; ++j) {
          const unsigned long long* col = cols + (j * 32 + sp) * Kp;
          unsigned int cnt = 0;
          if (t == 0) {
#pragma unroll 1
            for (int k = 0; k < nw; ++k) {
              const unsigned long long x = ~col[k];
              cnt += __popcll(k == nw - 1 ? x & tail : x);
            }
            if (chain_sum) chain_sum[(int64_t)(cb + j) * n + i] = M - 2 * (int)cnt;
          } else {
            unsigned long long lo = col[a];  // (64 (k + a) + b < M for every k < nw: k + a < K)
#pragma unroll 1
            for (int k = 0; k < nw; ++k) {
              const unsigned long long hi = k + a + 1 < K ? col[k + a + 1] : 0ull;
              const unsigned long long y = b ? (lo >> b) | (hi << (64 - b)) : lo;
              const unsigned long long x = col[k] ^ y;
              cnt += __popcll(k == nw - 1 ? x & tail : x);
              lo = hi;
            }
          }
          minus[r] += cnt;
        }
      }
    }
    __syncthreads();  // (the next pass's transpose overwrites the columns)
  }
  if (i >= n) return;
  const long long chains = c1 - c0;
#pragma unroll
  for (int r = 0; r < AC_PER; ++r) {
    const int t = t0 + 32 * r;
    if (t > max_lag) break;
    const long long pairs = chains * (long long)(M - t);
    if (t == 0) {
      atomicAdd(spin_sum + i, (unsigned long long)(pairs - 2 * (long long)minus[r]));  // (two's complement: the signed sum)
      atomicAdd(lag_sum + i, (unsigned long long)pairs);
    } else {
      atomicAdd(lag_sum + (int64_t)t * n + i, (unsigned long long)(pairs - 2 * (long long)minus[r]));
    }
  }
}

// ---------------------------------------------------------------- overlaps of bit-packed rows (dvg_packed_overlap)
// All pairs (row of A, row of B) of a group: d = popc(x ^ y) over the spins < n, GEMM-shaped on bits.  A TILE is 64 rows.  A
// UNIT is (group, A tile ta, a span of B tiles); a workgroup of 256 threads walks the units `blockIdx.x + i gridDim.x`.  For
// each B tile of the span it stages, OV_KC = 16 words of the rows at a time, both tiles in LDS word-major -- T[k][row], 64
// rows of one word side by side, the last word masked to n, rows beyond the last read as 0 -- and thread (ty, tx) = (tid >> 4,
// tid & 15) keeps the 4 x 4 block of pairs (rows 4 ty .. 4 ty + 3 of A) x (rows 4 tx .. 4 tx + 3 of B): per word one 128-bit
// read of each tile serves 16 XOR + popcount-accumulate steps.  With W <= 16 (n <= 512) the A tile is staged once per unit.
// Self mode (B = A): units take the tiles tb >= ta only and count r < r'; with `nearest` they take every tb (a row's nearest
// partner may lie on either side of it), count r < r' as before and take the minimum over r != r'.
// Histogram: LDS counters h[d][copy], copy = lane & (copies - 1), `copies` = the largest power of two <= 8 for which
// (n + 1) copies words fit OV_HIST_LDS (8 up to n = 1055, 1 at 8192).  The distances of unrelated rows crowd into about sqrt(n)
// bins; copies spread the lanes that meet on one distance over several addresses.  Measured at n = 512 on rows of fair coins
// the update costs nothing one can see at 1, 8 or 32 copies (the popcounts bound the kernel), so the copies are kept few: a
// small LDS footprint lets four workgroups share a CU, which is what the time does depend on.  The counters live across the
// workgroup's units and are flushed once, nonzero bins only, with 64-bit integer atomics (and every OV_FLUSH_TILES tiles =
// 2^28 pairs, so that a 32-bit counter cannot wrap).  Integer addition commutes: the order of the workgroups does not matter.
// nearest: a thread keeps min over its B rows of (d << 32 | row of B) per A row across the unit's span; 16 lanes combine by
// shuffles; one store per A row and unit where the unit spans all of B, else one unsigned 64-bit atomic minimum onto the
// output, which the host filled with 0xFF bytes (-1 = no partner = the unsigned maximum).  The minimum of the keys is the
// smallest distance and, among equals, the smallest row.
// LDS banks (bank = dword mod 64 for ds_read_b128 in its four 16-lane groups, mod 32 for ds_write_b32 and ds_add_u32 in
// 32-lane halves): row r of word k sits at T[k][r ^ 4 k].  Reads: 16 lanes of a group hold 16 different tx or one ty (two
// over lanes l and l + 16): B gives the 16 slots of one 256-byte row, each bank once; A is one or two addresses, broadcast.
// Staging: lane (ty, tx) writes word k = tx of row ty + 16 p -- a 32-lane half holds rows r, r + 1 and k = 0 .. 15, bank
// (r ^ 4 k) mod 32: two addresses per bank at the most, which costs a ds_write_b32 nothing.  The XOR is there for that: plain
// T[k][r] would put the 16 words of a row on one bank.  Histogram adds: bank = (8 d + lane mod 8) mod 32 -- lanes of a half
// that share a distance and a copy add to one address and serialise, lanes whose distances differ by a multiple of 4 share a
// bank: data-dependent, up to 32-way in the worst case (all pairs at one distance with one copy), and not seen in the time.
constexpr int OV_THREADS = 256, OV_TILE = 64, OV_KC = 16, OV_MAX_N = 8192, OV_HIST_LDS = 33 * 1024, OV_MAX_COPIES = 8;
constexpr int OV_TILE_LDS = 2 * OV_KC * OV_TILE * 4, OV_FLUSH_TILES = 1 << 16, OV_UNITS = 2048, OV_GRID = 1024;

__device__ __forceinline__ void ov_flush(unsigned int* h, int n, int copies, int tid, unsigned long long* __restrict__ hist) {
  for (int d = tid; d <= n; d += OV_THREADS) {
    unsigned long long s = 0ull;
    for (int c = 0; c < copies; ++c) {
      const int at = d * copies + ((c + tid) & (copies - 1));  // (rotated by the lane: each bank once)
      s += h[at];
      h[at] = 0u;
    }
    if (s) atomicAdd(hist + d, s);
  }
}

template <bool NEAREST>
__global__ __launch_bounds__(OV_THREADS) void packed_overlap_kernel(
    const uint32_t* __restrict__ a, int64_t rows_a, int64_t a_rs, int64_t a_gs, const uint32_t* __restrict__ b, int64_t rows_b,
    int64_t b_rs, int64_t b_gs, int self, int n, int W, int copies, int64_t nta, int64_t ntb, int64_t span, int64_t ns,
    int64_t units, unsigned long long* __restrict__ hist, unsigned long long* __restrict__ nearest) {
  extern __shared__ __align__(16) unsigned char ov_smem[];
  uint32_t* As = reinterpret_cast<uint32_t*>(ov_smem);  // [OV_KC][64], row r of word k at [k][r ^ 4 k]
  uint32_t* Bs = As + OV_KC * OV_TILE;
  unsigned int* h = Bs + OV_KC * OV_TILE;  // [n + 1][copies]
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4, cp = tid & (copies - 1);
  for (int i = tid; i < (n + 1) * copies; i += OV_THREADS) h[i] = 0u;
  const uint32_t last_mask = (n & 31) ? (1u << (n & 31)) - 1u : ~0u;
  const bool resident = W <= OV_KC;  // the A tile is whole in LDS: staged once per unit
  int since = 0;                     // tiles since the last flush
  for (int64_t u = blockIdx.x; u < units; u += gridDim.x) {
    const int64_t s = u % ns, rest = u / ns, ta = rest % nta, g = rest / nta;
    int64_t tb0 = s * span;
    const int64_t tb1 = tb0 + span < ntb ? tb0 + span : ntb;
    if (self && !NEAREST && tb0 < ta) tb0 = ta;
    const uint32_t* ag = a + g * a_gs;
    const uint32_t* bg = b + g * b_gs;
    const int64_t a0 = ta * OV_TILE;
    unsigned long long best[4] = {~0ull, ~0ull, ~0ull, ~0ull};
    for (int64_t tb = tb0; tb < tb1; ++tb) {
      const int64_t b0 = tb * OV_TILE;
      unsigned int acc[4][4];
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0u;
      for (int k0 = 0; k0 < W; k0 += OV_KC) {
        const int kc = W - k0 < OV_KC ? W - k0 : OV_KC, kc4 = (kc + 3) & ~3;
        __syncthreads();  // (the words of the last chunk have been read)
        if (tx < kc4) {
          const int k = k0 + tx;
          const uint32_t m = k == W - 1 ? last_mask : ~0u;
          if (!resident || tb == tb0) {
#pragma unroll
            for (int p = 0; p < 4; ++p) {
              const int row = ty + 16 * p;
              const int64_t r = a0 + row;
              As[tx * OV_TILE + (row ^ (4 * tx))] = (tx < kc && r < rows_a) ? ag[r * a_rs + k] & m : 0u;
            }
          }
#pragma unroll
          for (int p = 0; p < 4; ++p) {
            const int row = ty + 16 * p;
            const int64_t r = b0 + row;
            Bs[tx * OV_TILE + (row ^ (4 * tx))] = (tx < kc && r < rows_b) ? bg[r * b_rs + k] & m : 0u;
          }
        }
        __syncthreads();
        for (int kk = 0; kk < kc4; kk += 4) {
#pragma unroll
          for (int k = kk; k < kk + 4; ++k) {
            const uint4 av = *reinterpret_cast<const uint4*>(As + k * OV_TILE + 4 * (ty ^ (k & 15)));
            const uint4 bv = *reinterpret_cast<const uint4*>(Bs + k * OV_TILE + 4 * (tx ^ (k & 15)));
            const uint32_t ar[4] = {av.x, av.y, av.z, av.w}, br[4] = {bv.x, bv.y, bv.z, bv.w};
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
              for (int j = 0; j < 4; ++j) acc[i][j] += __popc(ar[i] ^ br[j]);
          }
        }
      }
      // the tile's 16 pairs of this thread, by their rows inside the tiles: li < na, lj < nb exist; on the diagonal tile of
      // self mode li < lj is counted and li != lj has a partner; tiles below the diagonal (self mode with nearest) count nothing
      const int na = rows_a - a0 < OV_TILE ? (int)(rows_a - a0) : OV_TILE, nb = rows_b - b0 < OV_TILE ? (int)(rows_b - b0) : OV_TILE;
      const bool diag = self && ta == tb, below = self && tb < ta;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int li = 4 * ty + i;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int lj = 4 * tx + j;
          const bool valid = li < na && lj < nb;
          if (valid && !below && (!diag || li < lj)) atomicAdd(h + acc[i][j] * copies + cp, 1u);
          if (NEAREST && valid && (!diag || li != lj)) {
            const unsigned long long key = ((unsigned long long)acc[i][j] << 32) | (unsigned long long)(b0 + lj);
            best[i] = key < best[i] ? key : best[i];
          }
        }
      }
      if (++since == OV_FLUSH_TILES) {  // (uniform over the workgroup)
        __syncthreads();
        ov_flush(h, n, copies, tid, hist);
        since = 0;
      }
    }
    if (NEAREST) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        unsigned long long v = best[i];
#pragma unroll
        for (int off = 1; off < 16; off <<= 1) {
          const unsigned long long o = __shfl_xor(v, off, 64);
          v = o < v ? o : v;
        }
        const int64_t r = a0 + 4 * ty + i;
        if (tx == 0 && r < rows_a) {
          if (ns == 1) nearest[g * rows_a + r] = v;  // (this unit saw every row of B)
          else if (v != ~0ull) atomicMin(nearest + g * rows_a + r, v);
        }
      }
    }
  }
  __syncthreads();
  ov_flush(h, n, copies, tid, hist);
}

// ---------------------------------------------------------------- energies of bit-packed rows (dvg_grbm_energy_packed)
// E(row) = sum_i hs_i s_i + sum_e Js_e s_i s_j in float64, hs / Js the scaled, clamped float32 fields the sampler draws from.
// A TILE is 64 consecutive rows of the flattened (group, row) index -- one per lane; a workgroup of EN_WAVES waves takes the
// tiles `blockIdx.x + k gridDim.x` (one tile each up to EN_GRID tiles).  It turns its tile into per-spin BIT COLUMNS in LDS with
// the ballots of the moments kernel: a wave takes the words w = wave, wave + EN_WAVES, .., lane r reads word w of its row (rows
// beyond the last read as 0), 32 ballots give the 64-bit columns of spins 32 w .. 32 w + 31 (bit r = the spin's bit in row r),
// kept by lanes 0..31; columns of spins >= n are never stored.  A column is stored as its two halves, lo[spin] (rows 0..31) and
// hi[spin] (rows 32..63): lane r only ever needs the half that holds its own bit.
// Behind the barrier wave v takes the terms v per .. v per + per - 1 of the n + n_edges terms (spins first, then edges in the
// order of the edge list), per = ceil((n + n_edges) / EN_WAVES), 64 terms at a time: lane t loads the block's t-th h_i or J_e
// and scales and clamps it -- clamp(rn(prefactor h_i), h_lo, h_hi), once per term and tile, never per row -- then the wave
// walks the block.  A term is WAVE-UNIFORM: its number (a scalar loop counter), i and j (scalar loads), its field (v_readlane
// from the lane that holds it) and the mask x = ~col_i (the rows in which s_i = -1) or col_i ^ col_j (the rows in which s_i s_j
// = -1), read from LDS at one address per 32-lane half.  Lane r moves its own bit of x into bit 31 with a shift by 31 - (r mod
// 32) -- a per-lane constant, not a per-term amount -- and XORs it onto the float32 field's sign; the conversion to float64 is
// exact, and one float64 accumulator per lane takes the terms in order.  The waves' partial sums meet in LDS, part[wave][lane];
// behind a second barrier wave 0 adds them in wave order and its lanes store 64 consecutive doubles (rows beyond the last are
// not stored).  The order of the additions is fixed by (n, n_edges) alone: no atomics, the same bits on every call.  A
// workgroup's next tile needs no third barrier: the columns are rewritten behind barrier 2, which every wave passes with its
// terms done, and part[] behind the next tile's barrier 1, which wave 0 reaches with its sums read.
// LDS: 8 n bytes of columns + EN_WAVES 512 bytes of partial sums (72 KiB at n = 8192).  Banks (bank = dword mod 32 for
// ds_read_b32 and ds_write_b32 in 32-lane halves, dword mod 64 for ds_read_b64 in 32-lane halves, mod 32 for ds_write_b64 in
// groups of 16 lanes): the term loop's ds_read_b32 is one address per half -- a broadcast; the transpose writes lo[32 w + l] and
// hi[32 w + l], l < 32: 32 consecutive dwords, each bank once; part[wave][lane] is written and read with consecutive lanes on
// consecutive doubles, each bank once per group.  No conflict by the rule.
constexpr int EN_WAVES = 16, EN_UNROLL = 4, EN_MAX_N = 8192, EN_PART_LDS = EN_WAVES * 64 * 8, EN_LDS_MAX = EN_MAX_N * 8 + EN_PART_LDS;
constexpr int64_t EN_GRID = 1 << 20;

// field of the block's term k (held by lane k) with this lane's bit of the mask `minus` as its sign, exactly in float64
__device__ __forceinline__ double en_term(uint32_t fields, int k, uint32_t minus, int to_sign) {
  const uint32_t field = (uint32_t)__builtin_amdgcn_readlane((int)fields, k);
  return (double)__uint_as_float(field ^ ((minus << to_sign) & 0x80000000u));
}

__global__ __launch_bounds__(EN_WAVES * 64) void grbm_energy_packed_kernel(
    const uint32_t* __restrict__ bits, int64_t rows, int64_t row_stride, int64_t groups, int64_t group_stride, int n, int W,
    int n_edges, const int32_t* __restrict__ ei, const int32_t* __restrict__ ej, const float* __restrict__ h,
    const float* __restrict__ J, float prefactor, float h_lo, float h_hi, float j_lo, float j_hi, double* __restrict__ out) {
  extern __shared__ __align__(16) unsigned char en_smem[];
  uint32_t* lo = reinterpret_cast<uint32_t*>(en_smem);  // [n] rows 0..31 of the tile, then [n] rows 32..63
  double* part = reinterpret_cast<double*>(lo + 2 * n);  // [EN_WAVES][64]
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t* mine = lane < 32 ? lo : lo + n;  // the halves that hold this lane's bit
  const int to_sign = 31 - (lane & 31);
  const int terms = n + n_edges, per = (terms + EN_WAVES - 1) / EN_WAVES;
  const int t0 = wave * per < terms ? wave * per : terms, t1 = t0 + per < terms ? t0 + per : terms;  // this wave's terms
  const int i1 = t1 < n ? t1 : n, e0 = (t0 > n ? t0 : n) - n, e1 = t1 - n;  // spins t0 .. i1 - 1 and edges e0 .. e1 - 1 of them
  const int64_t total = groups * rows, n_tiles = (total + 63) >> 6;
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int64_t idx = tile * 64 + lane;
    tile_columns_halves<EN_WAVES>(packed_row(bits, idx, total, rows, row_stride, groups, group_stride), W, n, wave, lane, lo);
    __syncthreads();
    double acc = 0.0;
    for (int b0 = t0; b0 < i1; b0 += 64) {
      const int cnt = i1 - b0 < 64 ? i1 - b0 : 64;
      const uint32_t hs = lane < cnt ? __float_as_uint(scaled_clamped(prefactor, h[b0 + lane], h_lo, h_hi)) : 0u;
      int k = 0;
      for (; k + EN_UNROLL <= cnt; k += EN_UNROLL) {  // (unrolled by hand: the reads of EN_UNROLL terms in flight together)
        uint32_t x[EN_UNROLL];
#pragma unroll
        for (int u = 0; u < EN_UNROLL; ++u) x[u] = ~mine[b0 + k + u];
#pragma unroll
        for (int u = 0; u < EN_UNROLL; ++u) acc += en_term(hs, k + u, x[u], to_sign);
      }
      for (; k < cnt; ++k) acc += en_term(hs, k, ~mine[b0 + k], to_sign);
    }
    for (int b0 = e0; b0 < e1; b0 += 64) {
      const int cnt = e1 - b0 < 64 ? e1 - b0 : 64;
      const uint32_t Js = lane < cnt ? __float_as_uint(scaled_clamped(prefactor, J[b0 + lane], j_lo, j_hi)) : 0u;
      int k = 0;
      for (; k + EN_UNROLL <= cnt; k += EN_UNROLL) {
        uint32_t x[EN_UNROLL];
#pragma unroll
        for (int u = 0; u < EN_UNROLL; ++u) x[u] = mine[ei[b0 + k + u]] ^ mine[ej[b0 + k + u]];
#pragma unroll
        for (int u = 0; u < EN_UNROLL; ++u) acc += en_term(Js, k + u, x[u], to_sign);
      }
      for (; k < cnt; ++k) acc += en_term(Js, k, mine[ei[b0 + k]] ^ mine[ej[b0 + k]], to_sign);
    }
    part[wave * 64 + lane] = acc;
    __syncthreads();
    if (wave == 0 && idx < total) {
      double s = part[lane];
#pragma unroll
      for (int v = 1; v < EN_WAVES; ++v) s += part[v * 64 + lane];
      out[idx] = s;
    }
  }
}

}  // namespace dvg

using namespace dvg;

extern "C" int dvg_grbm_energy(const dvg_graph_t* g, const float* x, int64_t rows, const float* linear,
                               const float* quadratic, float* energy_out, dvg_stream_t stream) {
  DVG_REQUIRE(g && x && linear && quadratic && energy_out, "grbm_energy: null argument");
  DVG_REQUIRE(rows >= 0, "grbm_energy: rows=%lld", (long long)rows);
  if (rows == 0) return DVG_OK;
  hipStream_t s = (hipStream_t)stream;
  DVG_LAUNCH(K_GRBM_ENERGY, grbm_energy_kernel, dim3((unsigned)ceil_div(rows, 4)), dim3(256), 0, s, x, rows,
             g->n, g->n_edges, g->edge_i, g->edge_j, linear, quadratic, energy_out);
  return DVG_OK;
}

extern "C" size_t dvg_grbm_suffstats_workspace_bytes(const dvg_graph_t* g) {
  return g ? sizeof(double) * (size_t)SS_SLABS * (size_t)(g->n + g->n_edges) : 0;
}

extern "C" int dvg_grbm_suffstats(const dvg_graph_t* g, const float* x, int64_t rows, const float* row_weight,
                                  float scale, float* acc_linear, float* acc_quadratic, int accumulate,
                                  void* ws, size_t ws_bytes, dvg_stream_t stream) {
  DVG_REQUIRE(g && x && acc_linear && acc_quadratic && ws, "grbm_suffstats: null argument");
  DVG_REQUIRE(rows > 0, "grbm_suffstats: rows=%lld", (long long)rows);
  if (ws_bytes < dvg_grbm_suffstats_workspace_bytes(g)) {
    set_error("grbm_suffstats: workspace %zu < %zu", ws_bytes, dvg_grbm_suffstats_workspace_bytes(g));
    return DVG_E_WORKSPACE;
  }
  hipStream_t s = (hipStream_t)stream;
  const int total = g->n + g->n_edges;
  const unsigned nb = (unsigned)ceil_div(total, 256);
  DVG_LAUNCH(K_GRBM_SUFFSTATS, grbm_suffstats_partial, dim3(nb, SS_SLABS), dim3(256), 0, s, x, rows, g->n,
             g->n_edges, g->edge_i, g->edge_j, row_weight, (double*)ws);
  DVG_LAUNCH(K_GRBM_SUFFSTATS, grbm_suffstats_reduce, dim3(nb), dim3(256), 0, s, (const double*)ws, g->n,
             g->n_edges, scale, acc_linear, acc_quadratic, accumulate);
  return DVG_OK;
}

// Exact integer moments of bit-packed rows (include/dvg.h): the traced draw's records, never unpacked.
extern "C" int dvg_grbm_moments_packed(const dvg_graph_t* g, const uint32_t* bits, int64_t rows, int64_t* spin_sum,
                                       int64_t* pair_sum, int accumulate, dvg_stream_t stream) {
  DVG_REQUIRE(g && bits && spin_sum && pair_sum, "grbm_moments_packed: null argument");
  DVG_REQUIRE(rows >= 1, "grbm_moments_packed: rows=%lld must be at least 1", (long long)rows);
  const int n = g->n, W = (n + 31) / 32;
  if ((size_t)n * 8 > (size_t)MP_LDS) {
    set_error("grbm_moments_packed: n=%d > %d (a tile's bit columns are kept in %d KiB of LDS)", n, MP_LDS / 8, MP_LDS / 1024);
    return DVG_E_UNSUPPORTED;
  }
  hipStream_t s = (hipStream_t)stream;
  if (!accumulate) {
    DVG_CHECK_HIP(hipMemsetAsync(spin_sum, 0, sizeof(int64_t) * (size_t)n, s));
    if (g->n_edges > 0) DVG_CHECK_HIP(hipMemsetAsync(pair_sum, 0, sizeof(int64_t) * (size_t)g->n_edges, s));
  }
  // tiles per workgroup: enough workgroups to fill the chip (about 128), as few atomics as that allows, within the LDS
  const int64_t n_tiles = ceil_div(rows, 64);
  const int64_t fit = MP_LDS / ((int64_t)n * 8);
  int64_t per = ceil_div(n_tiles, 128);
  per = per < 1 ? 1 : per > fit ? fit : per;
  if (ceil_div(n_tiles, per) > 0x7fffffff) {
    set_error("grbm_moments_packed: rows=%lld is more than one launch takes", (long long)rows);
    return DVG_E_UNSUPPORTED;
  }
  DVG_LAUNCH(K_GRBM_SUFFSTATS, grbm_moments_packed_kernel, dim3((unsigned)ceil_div(n_tiles, per)), dim3(MP_WAVES * 64),
             (size_t)per * n * 8, s, bits, rows, n, W, g->n_edges, g->edge_i, g->edge_j, (int)per,
             reinterpret_cast<unsigned long long*>(spin_sum), reinterpret_cast<unsigned long long*>(pair_sum));
  return DVG_OK;
}

// Float64 energies of bit-packed rows under the sampler's scaled, clamped fields ("DVG energy v1", include/dvg.h): the rows
// are never unpacked.
extern "C" int dvg_grbm_energy_packed(const dvg_graph_t* g, const float* linear, const float* quadratic, float prefactor,
                                      float h_lo, float h_hi, float j_lo, float j_hi, const uint32_t* bits, int64_t rows,
                                      int64_t row_stride, int64_t groups, int64_t group_stride, double* energy_out,
                                      dvg_stream_t stream) {
  DVG_REQUIRE(g, "grbm_energy_packed: g is null");
  DVG_REQUIRE(linear, "grbm_energy_packed: linear is null");
  DVG_REQUIRE(quadratic, "grbm_energy_packed: quadratic is null");
  DVG_REQUIRE(bits, "grbm_energy_packed: bits is null");
  DVG_REQUIRE(energy_out, "grbm_energy_packed: energy_out is null");
  const int n = g->n;
  const int64_t W = ((int64_t)n + 31) / 32;
  DVG_TRY(check_row_geometry("grbm_energy_packed", rows, groups, row_stride, W, group_stride));
  DVG_REQUIRE(std::isfinite(prefactor), "grbm_energy_packed: prefactor=%g is not finite", (double)prefactor);
  DVG_TRY(check_row_count("grbm_energy_packed", rows, groups));
  DVG_TRY(check_spin_count("grbm_energy_packed", n, EN_MAX_N));
  hipStream_t s = (hipStream_t)stream;
  const int64_t n_tiles = ceil_div(groups * rows, 64);
  const size_t lds = (size_t)n * 8 + (size_t)EN_PART_LDS;
  DVG_RAISE_LDS_ABOVE_64K(lds, grbm_energy_packed_kernel, EN_LDS_MAX);
  DVG_LAUNCH(K_GRBM_SUFFSTATS, grbm_energy_packed_kernel, dim3((unsigned)(n_tiles < EN_GRID ? n_tiles : EN_GRID)),
             dim3(EN_WAVES * 64), lds, s, bits, rows, row_stride, groups, group_stride, n, (int)W, g->n_edges, g->edge_i, g->edge_j,
             linear, quadratic, prefactor, h_lo, h_hi, j_lo, j_hi, energy_out);
  return DVG_OK;
}

// Exact lagged products of a bit-packed trace's spins ("DVG acf v1", include/dvg.h): the records are never unpacked.
extern "C" int dvg_trace_autocorr(const uint32_t* bits, int n_chains, int n_records, int n, int max_lag, int64_t* lag_sum,
                                  int64_t* spin_sum, int32_t* chain_sum, int accumulate, dvg_stream_t stream) {
  DVG_REQUIRE(bits, "trace_autocorr: bits is null");
  DVG_REQUIRE(lag_sum, "trace_autocorr: lag_sum is null");
  DVG_REQUIRE(spin_sum, "trace_autocorr: spin_sum is null");
  DVG_REQUIRE(n_chains >= 1, "trace_autocorr: n_chains=%d must be at least 1", n_chains);
  DVG_REQUIRE(n_records >= 1, "trace_autocorr: n_records=%d must be at least 1", n_records);
  DVG_REQUIRE(n >= 1, "trace_autocorr: n=%d must be at least 1", n);
  DVG_REQUIRE(max_lag >= 0 && max_lag < n_records, "trace_autocorr: max_lag=%d must lie in 0 .. n_records - 1 = %d", max_lag,
              n_records - 1);
  if (n_records > AC_MAX_RECORDS) {
    set_error("trace_autocorr: n_records=%d > %d (the time columns of 32 spins are kept in %d KiB of LDS)", n_records,
              AC_MAX_RECORDS, AC_LDS_MAX / 1024);
    return DVG_E_UNSUPPORTED;
  }
  const int64_t W = ((int64_t)n + 31) / 32;
  // the largest index: n_chains n_records W words of bits (the outputs' (max_lag + 1) n and n_chains n are below 2^62)
  if ((int64_t)n_chains * n_records > (INT64_MAX / 4) / W) {
    set_error("trace_autocorr: n_chains=%d x n_records=%d x %lld words is more than one launch indexes", n_chains, n_records,
              (long long)W);
    return DVG_E_UNSUPPORTED;
  }
  hipStream_t s = (hipStream_t)stream;
  if (!accumulate) {
    DVG_CHECK_HIP(hipMemsetAsync(lag_sum, 0, sizeof(int64_t) * (size_t)(max_lag + 1) * (size_t)n, s));
    DVG_CHECK_HIP(hipMemsetAsync(spin_sum, 0, sizeof(int64_t) * (size_t)n, s));
  }
  // chains per workgroup: enough workgroups to fill the chip (about 128, the moments kernel's aim), as few atomics as that allows
  const int64_t chunks = ceil_div((int64_t)max_lag + 1, AC_LAGS);  // <= 64
  int64_t slabs = ceil_div(128, W * chunks);
  slabs = slabs > n_chains ? n_chains : slabs;
  const int64_t per = ceil_div(n_chains, slabs);
  slabs = ceil_div(n_chains, per);
  const int K = (n_records + 63) / 64;
  const size_t per_chain = (size_t)32 * (size_t)(K | 1) * 8;  // a chain's 32 time columns
  int64_t batch = (int64_t)(64 * 1024 / per_chain);             // chains per pass: what 64 KiB hold, 1 .. AC_BATCH
  batch = batch < 1 ? 1 : batch > AC_BATCH ? AC_BATCH : batch;
  batch = batch > per ? per : batch;
  const size_t lds = (size_t)batch * per_chain;
  DVG_RAISE_LDS_ABOVE_64K(lds, trace_autocorr_kernel, AC_LDS_MAX);
  DVG_LAUNCH(K_GRBM_SUFFSTATS, trace_autocorr_kernel, dim3((unsigned)W, (unsigned)slabs, (unsigned)chunks), dim3(AC_WAVES * 64),
             lds, s, bits, n_chains, n_records, n, (int)W, max_lag, (int)per, (int)batch, reinterpret_cast<unsigned long long*>(lag_sum),
             reinterpret_cast<unsigned long long*>(spin_sum), chain_sum);
  return DVG_OK;
}

// Exact Hamming-distance histogram and nearest rows of bit-packed rows ("DVG overlap v1", include/dvg.h): never unpacked.
extern "C" int dvg_packed_overlap(const uint32_t* a, int64_t rows_a, int64_t a_row_stride, int64_t a_group_stride,
                                  const uint32_t* b, int64_t rows_b, int64_t b_row_stride, int64_t b_group_stride, int groups,
                                  int n, int64_t* hist, int64_t* nearest, int accumulate, dvg_stream_t stream) {
  DVG_REQUIRE(a, "packed_overlap: a is null");
  DVG_REQUIRE(hist, "packed_overlap: hist is null");
  DVG_REQUIRE(rows_a >= 1, "packed_overlap: rows_a=%lld must be at least 1", (long long)rows_a);
  DVG_REQUIRE(groups >= 1, "packed_overlap: groups=%d must be at least 1", groups);
  DVG_REQUIRE(n >= 1, "packed_overlap: n=%d must be at least 1", n);
  const int64_t W = ((int64_t)n + 31) / 32;
  DVG_REQUIRE(a_row_stride >= W, "packed_overlap: a_row_stride=%lld is less than the %lld words of a row", (long long)a_row_stride,
              (long long)W);
  DVG_REQUIRE(a_group_stride >= 0, "packed_overlap: a_group_stride=%lld is negative", (long long)a_group_stride);
  const int self = b == nullptr;
  if (self) {
    b = a, rows_b = rows_a, b_row_stride = a_row_stride, b_group_stride = a_group_stride;
  } else {
    DVG_REQUIRE(rows_b >= 1, "packed_overlap: rows_b=%lld must be at least 1", (long long)rows_b);
    DVG_REQUIRE(b_row_stride >= W, "packed_overlap: b_row_stride=%lld is less than the %lld words of a row",
                (long long)b_row_stride, (long long)W);
    DVG_REQUIRE(b_group_stride >= 0, "packed_overlap: b_group_stride=%lld is negative", (long long)b_group_stride);
  }
  if (n > OV_MAX_N) {
    set_error("packed_overlap: n=%d > %d (a workgroup keeps the n + 1 bins of the histogram as 32-bit counters in %d KiB of LDS)",
              n, OV_MAX_N, OV_HIST_LDS / 1024);
    return DVG_E_UNSUPPORTED;
  }
  if (rows_a >= (1ll << 31)) {
    set_error("packed_overlap: rows_a=%lld must be below 2^31 (a row index is the low half of a nearest element)", (long long)rows_a);
    return DVG_E_UNSUPPORTED;
  }
  if (rows_b >= (1ll << 31)) {
    set_error("packed_overlap: rows_b=%lld must be below 2^31 (a row index is the low half of a nearest element)", (long long)rows_b);
    return DVG_E_UNSUPPORTED;
  }
  if ((__int128)rows_a * rows_b * groups >= ((__int128)1 << 62)) {
    set_error("packed_overlap: groups=%d x rows_a=%lld x rows_b=%lld pairs are 2^62 or more", groups, (long long)rows_a,
              (long long)rows_b);
    return DVG_E_UNSUPPORTED;
  }
  hipStream_t s = (hipStream_t)stream;
  int copies = OV_MAX_COPIES;
  while (copies > 1 && (size_t)(n + 1) * copies * 4 > (size_t)OV_HIST_LDS) copies >>= 1;
  const size_t lds = (size_t)OV_TILE_LDS + (size_t)(n + 1) * copies * 4;
  // units: (group, A tile, span of B tiles); B is split only as far as it takes to fill the chip
  const int64_t nta = ceil_div(rows_a, OV_TILE), ntb = ceil_div(rows_b, OV_TILE), base = (int64_t)groups * nta;
  int64_t ns = base >= OV_UNITS ? 1 : ceil_div(OV_UNITS, base);
  ns = ns > ntb ? ntb : ns;
  const int64_t span = ceil_div(ntb, ns);
  ns = ceil_div(ntb, span);
  const int64_t units = base * ns;
  if (!accumulate) DVG_CHECK_HIP(hipMemsetAsync(hist, 0, sizeof(int64_t) * (size_t)(n + 1), s));
  if (nearest && ns > 1) DVG_CHECK_HIP(hipMemsetAsync(nearest, 0xFF, sizeof(int64_t) * (size_t)groups * (size_t)rows_a, s));
  const dim3 grid((unsigned)(units < OV_GRID ? units : OV_GRID));
  if (nearest) {
    DVG_LAUNCH(K_GRBM_SUFFSTATS, packed_overlap_kernel<true>, grid, dim3(OV_THREADS), lds, s, a, rows_a, a_row_stride,
               a_group_stride, b, rows_b, b_row_stride, b_group_stride, self, n, (int)W, copies, nta, ntb, span, ns, units,
               reinterpret_cast<unsigned long long*>(hist), reinterpret_cast<unsigned long long*>(nearest));
  } else {
    DVG_LAUNCH(K_GRBM_SUFFSTATS, packed_overlap_kernel<false>, grid, dim3(OV_THREADS), lds, s, a, rows_a, a_row_stride,
               a_group_stride, b, rows_b, b_row_stride, b_group_stride, self, n, (int)W, copies, nta, ntb, span, ns, units,
               reinterpret_cast<unsigned long long*>(hist), reinterpret_cast<unsigned long long*>(nearest));
  }
  return DVG_OK;
}
