// GRBM energy and its backward (weighted sufficient statistics).
// Energy: plugin GraphRestrictedBoltzmannMachine.__call__ as used at
// /root/reference/src/losses.py:61;  E(x) = x.h + sum_e J_e x_i x_j.
#include "common.h"
#include "graph.h"

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
    const uint32_t word = r < rows ? bits[r * W + w] : 0u;
    unsigned long long col = 0ull;
#pragma unroll
    for (int b = 0; b < 32; ++b) {
      const unsigned long long m = __builtin_amdgcn_ballot_w64(((word >> b) & 1u) != 0u);
      if (lane == b) col = m;
    }
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
      const uint32_t word = m < M ? bits[((int64_t)(cb + j) * M + m) * W + w] : 0u;
      unsigned long long column = 0ull;
#pragma unroll
      for (int b = 0; b < 32; ++b) {
        const unsigned long long v = __builtin_amdgcn_ballot_w64(((word >> b) & 1u) != 0u);
        if (lane == b) column = v;
      }
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
  static std::atomic<uint64_t> attr_done{0};
  if (lds > 64 * 1024) DVG_TRY(raise_dynamic_lds(attr_done, (const void*)trace_autocorr_kernel, AC_LDS_MAX));
  DVG_LAUNCH(K_GRBM_SUFFSTATS, trace_autocorr_kernel, dim3((unsigned)W, (unsigned)slabs, (unsigned)chunks), dim3(AC_WAVES * 64),
             lds, s, bits, n_chains, n_records, n, (int)W, max_lag, (int)per, (int)batch, reinterpret_cast<unsigned long long*>(lag_sum),
             reinterpret_cast<unsigned long long*>(spin_sum), chain_sum);
  return DVG_OK;
}
