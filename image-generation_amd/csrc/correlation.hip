// Full pair-correlation sums of bit-packed spin rows (dvg_packed_correlation, "DVG corr v1", include/dvg.h):
//   pair_sum[i][j] = sum over the T pooled rows of s_i s_j for EVERY pair of spins, spin_sum[i] = sum of s_i -- the spins x spins
// product X^T X of the +-1 rows, on their bits.  Two stream-ordered launches, no workgroup waiting on another.
#include "common.h"
#include "packed_rows.h"

namespace dvg {

// ---------------------------------------------------------------- 1. transpose: packed rows -> bit columns in the workspace
// cols[spin][k], k < Kp: a 64-bit word whose bit r is the spin's bit in the pooled row 64 k + r (pooled row p = row p % rows of
// group p / rows, reached through the strides).  Kp = ceil(T / 64) rounded up to CR_KC words, so that a column is a whole number
// of the product kernel's chunks; rows beyond T read as 0, which makes every pad bit and pad word 0.  Columns of spins >= n are
// never produced.  A workgroup of CT_TILES waves takes a JOB = (CT_TILES consecutive row tiles k, CT_WORDS words w of the rows =
// 32 CT_WORDS spins): wave v's lane r reads word w of pooled row 64 (CT_TILES job + v) + r, and 32 ballots -- the moments
// kernel's idiom -- give the columns of spins 32 w .. 32 w + 31, kept by lanes 0..31 and put in LDS as cs[tile][spin]; behind the
// barrier thread (spin, tile) = (tid / CT_TILES, tid % CT_TILES) stores cols[spin][CT_TILES job + tile]: CT_TILES lanes write 64
// contiguous bytes of a column.  The jobs `blockIdx.x + i gridDim.x` of a workgroup share their spins: a thread adds up
// popc(column word) = the rows in which its spin is +1 (zero padding counts as nothing), 8 lanes combine by shuffles, and ONE
// 64-bit atomic per spin and workgroup adds 2 plus - (real rows seen) onto spin_sum.
// LDS banks: cs[tile][spin] has a row stride of CT_STRIDE = 68 words of 64 bits.  The ballot lanes write 32 consecutive words;
// the store pass reads dword 136 tile + 2 spin with ds_read_b64 (bank = dword mod 64 in 32-lane halves): 8 tiles x 4 consecutive
// spins (first a multiple of 4) = 8 tile + 2 spin mod 64, each bank pair once.
constexpr int CT_TILES = 8, CT_WORDS = 2, CT_STRIDE = 68, CT_GRID = 1 << 16;

__global__ __launch_bounds__(CT_TILES * 64) void packed_correlation_transpose_kernel(
    const uint32_t* __restrict__ bits, int64_t rows, int64_t row_stride, int64_t groups, int64_t group_stride, int n, int W,
    int64_t Kp, unsigned long long* __restrict__ cols, unsigned long long* __restrict__ spin_sum) {
  __shared__ unsigned long long cs[CT_TILES * CT_STRIDE];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t total = groups * rows, jobs = Kp / CT_TILES;
  const int spin = 32 * CT_WORDS * (int)blockIdx.y + tid / CT_TILES, tile = tid % CT_TILES;  // (of the store pass)
  long long plus = 0, seen = 0;
  for (int64_t job = blockIdx.x; job < jobs; job += gridDim.x) {
    const int64_t idx = (job * CT_TILES + wave) * 64 + lane;
    const uint32_t* row = packed_row(bits, idx, total, rows, row_stride, groups, group_stride);  // (null: a row beyond the last)
#pragma unroll
    for (int ww = 0; ww < CT_WORDS; ++ww) {
      const int w = CT_WORDS * (int)blockIdx.y + ww;
      const unsigned long long col = bit_column((row && w < W) ? row[w] : 0u, lane);
      if (lane < 32) cs[wave * CT_STRIDE + 32 * ww + lane] = col;
    }
    __syncthreads();
    if (spin < n) {
      const unsigned long long c = cs[tile * CT_STRIDE + tid / CT_TILES];
      cols[(int64_t)spin * Kp + job * CT_TILES + tile] = c;
      plus += __popcll(c);
    }
    const int64_t left = total - job * CT_TILES * 64;  // real rows of this job: 0 .. 64 CT_TILES
    seen += left < 0 ? 0 : left < CT_TILES * 64 ? left : CT_TILES * 64;
    __syncthreads();  // (cs is rewritten by the next job)
  }
  if (spin_sum) {
#pragma unroll
    for (int off = 1; off < CT_TILES; off <<= 1) plus += __shfl_xor(plus, off, 64);
    if (tile == 0 && spin < n) atomicAdd(spin_sum + spin, (unsigned long long)(2 * plus - seen));  // (two's complement)
  }
}

// ---------------------------------------------------------------- 2. the column product on bits
// A TILE is 64 spins.  A workgroup of 256 threads owns (column tile I, column tile J >= I, a SLAB of row words): blockIdx.y
// numbers the upper tile pairs row by row, blockIdx.x the slabs.  A column is walked as 32-bit words (two per 64 rows), a CHUNK
// of CR_KC32 = 32 of them = 1024 rows at a time: both tiles' chunks are staged in LDS word-major, T[k][spin], and thread (ty, tx) =
// (tid >> 4, tid & 15) keeps the 4 x 4 block of pairs (spins 4 ty .. 4 ty + 3 of I) x (spins 4 tx .. 4 tx + 3 of J) as 32-bit
// counts in registers: per word one 128-bit read of each tile serves 16 XOR + popcount-accumulate steps -- the inner loop of
// packed_overlap_kernel with rows and spins swapped.  On a diagonal tile pair (I = J) one staged tile serves both sides.
// Padding: the zero bits behind row T are 0 in both columns of a pair, so their XOR is 0 and `minus` (the rows in which s_i s_j =
// -1) never counts them; `rows_in_slab` counts real rows only, and sum = rows_in_slab - 2 minus needs no tail mask.  Columns of
// spins >= n (the last tile of an n that is no multiple of 64) are staged as 0 and their sums are not written.
// Wrap: a slab is at most CR_SLAB_CHUNKS chunks = CR_SLAB_ROWS = 2^18 rows, and a count is at most the rows of its slab: no
// 32-bit count can pass 2^18, and rows_in_slab - 2 minus fits an int32.
// End of slab: the 64 x 64 sums go to LDS as int32 (over the staging area), then thread t adds elements t, t + 256, .. of the
// tile -- a wave 64 consecutive j of one i, 512 contiguous bytes -- with one 64-bit atomic each onto pair_sum[i][j], and for
// I != J a second pass adds the transposed tile onto pair_sum[j][i] in the same shape.  A diagonal tile pair holds both
// triangles already and is written once.  Integer addition commutes: the result does not depend on arrival order.
// LDS banks (ds_read_b128: bank = dword mod 64 in four 16-lane groups; ds_write_b32: dword mod 32 in 32-lane halves): spin c of
// word k sits at T[k][c ^ 4 (k >> 2)].  Reads: a 16-lane group holds 16 tx (the 16 slots of one 256-byte row, each bank once)
// and one ty (one address, broadcast).  Staging: thread (c, q) = (tid >> 3, tid & 7) reads the 16 bytes k = 4 q .. 4 q + 3 of
// column c and c + 32 and writes them to T[4 q + e][c ^ 4 q]: a 32-lane half holds 4 consecutive c (first a multiple of 4) and
// 8 q: banks (c & 3) | ((c ^ 4 q) & 28), each once.  The int32 tile has a row stride of 65: the transposed pass reads
// consecutive i at one j, 65 i + j, each bank once.
constexpr int CR_THREADS = 256, CR_TILE = 64, CR_KC = 16, CR_KC32 = 2 * CR_KC, CR_CHUNK_ROWS = 64 * CR_KC, CR_SLAB_CHUNKS = 256;
constexpr int64_t CR_SLAB_ROWS = (int64_t)CR_SLAB_CHUNKS * CR_CHUNK_ROWS;  // 262144 = 2^18
static_assert(CR_SLAB_ROWS == 1 << 18, "functional.PACKED_CORRELATION_SLAB_ROWS and DESIGN.md state this bound");
constexpr int CR_MAX_N = 8192, CR_TARGET_WGS = 512;
constexpr int CR_LDS_WORDS = 2 * CR_KC32 * CR_TILE > CR_TILE * 65 ? 2 * CR_KC32 * CR_TILE : CR_TILE * 65;

__device__ __forceinline__ void cr_stage(uint32_t* T, const uint32_t* __restrict__ cols32, int64_t col_words, int64_t k32, int c0,
                                         int n, int tid) {
  const int q = tid & 7;
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const int c = (tid >> 3) + 32 * p;
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (c0 + c < n) v = *reinterpret_cast<const uint4*>(cols32 + (int64_t)(c0 + c) * col_words + k32 + 4 * q);
    const int slot = c ^ (4 * q);
    T[(4 * q + 0) * CR_TILE + slot] = v.x;
    T[(4 * q + 1) * CR_TILE + slot] = v.y;
    T[(4 * q + 2) * CR_TILE + slot] = v.z;
    T[(4 * q + 3) * CR_TILE + slot] = v.w;
  }
}

__global__ __launch_bounds__(CR_THREADS) void packed_correlation_kernel(const uint32_t* __restrict__ cols32, int64_t total,
                                                                        int64_t chunks, int64_t slab_chunks, int n, int nt,
                                                                        unsigned long long* __restrict__ pair_sum) {
  __shared__ __align__(16) uint32_t smem[CR_LDS_WORDS];
  uint32_t* As = smem;                      // [CR_KC32][64], spin c of word k at [k][c ^ 4 (k >> 2)]
  uint32_t* Bs = smem + CR_KC32 * CR_TILE;  // (the same words as As on a diagonal tile pair)
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  int I = 0, J = (int)blockIdx.y;  // the blockIdx.y-th pair I <= J, row by row
  while (J >= nt - I) {
    J -= nt - I;
    ++I;
  }
  J += I;
  const bool diag = I == J;
  const int i0 = I * CR_TILE, j0 = J * CR_TILE;
  const int64_t c_begin = (int64_t)blockIdx.x * slab_chunks, c_end = c_begin + slab_chunks < chunks ? c_begin + slab_chunks : chunks;
  const int64_t row_begin = c_begin * CR_CHUNK_ROWS, row_end = c_end * CR_CHUNK_ROWS < total ? c_end * CR_CHUNK_ROWS : total;
  const int rows_in_slab = (int)(row_end - row_begin);  // real rows: 1 .. CR_SLAB_ROWS
  const int64_t col_words = chunks * CR_KC32;
  const uint32_t* Bt = diag ? As : Bs;
  unsigned int acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = 0u;
  for (int64_t ch = c_begin; ch < c_end; ++ch) {
    __syncthreads();  // (the words of the last chunk have been read)
    cr_stage(As, cols32, col_words, ch * CR_KC32, i0, n, tid);
    if (!diag) cr_stage(Bs, cols32, col_words, ch * CR_KC32, j0, n, tid);
    __syncthreads();
#pragma unroll 8
    for (int k = 0; k < CR_KC32; ++k) {
      const uint4 av = *reinterpret_cast<const uint4*>(As + k * CR_TILE + 4 * (ty ^ (k >> 2)));
      const uint4 bv = *reinterpret_cast<const uint4*>(Bt + k * CR_TILE + 4 * (tx ^ (k >> 2)));
      const uint32_t ar[4] = {av.x, av.y, av.z, av.w}, br[4] = {bv.x, bv.y, bv.z, bv.w};
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] += __popc(ar[i] ^ br[j]);
    }
  }
  __syncthreads();
  int* out = reinterpret_cast<int*>(smem);  // [64][65]
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) out[(4 * ty + i) * 65 + 4 * tx + j] = rows_in_slab - 2 * (int)acc[i][j];
  __syncthreads();
  for (int e = tid; e < CR_TILE * CR_TILE; e += CR_THREADS) {
    const int a = e >> 6, b = e & 63;
    if (i0 + a < n && j0 + b < n)
      atomicAdd(pair_sum + (int64_t)(i0 + a) * n + (j0 + b), (unsigned long long)(long long)out[a * 65 + b]);
    if (!diag && j0 + a < n && i0 + b < n)
      atomicAdd(pair_sum + (int64_t)(j0 + a) * n + (i0 + b), (unsigned long long)(long long)out[b * 65 + a]);
  }
}

// words of 64 bits per column: ceil(T / 64) rounded up to whole chunks
static inline int64_t cr_col_words(int64_t total) { return ceil_div(ceil_div(total, 64), CR_KC) * CR_KC; }

}  // namespace dvg

using namespace dvg;

extern "C" size_t dvg_packed_correlation_workspace_bytes(int64_t rows, int64_t groups, int n) {
  if (rows < 1 || groups < 1 || n < 1 || n > CR_MAX_N || (__int128)groups * rows >= ((__int128)1 << 62)) return 0;
  const int64_t chunks = cr_col_words(groups * rows) / CR_KC;
  if (ceil_div(chunks, CR_SLAB_CHUNKS) > 0x7fffffff) return 0;
  return (size_t)n * (size_t)chunks * CR_KC * sizeof(uint64_t);
}

extern "C" int dvg_packed_correlation(const uint32_t* bits, int64_t rows, int64_t row_stride, int64_t groups, int64_t group_stride,
                                      int n, int64_t* spin_sum, int64_t* pair_sum, int accumulate, void* ws, size_t ws_bytes,
                                      dvg_stream_t stream) {
  DVG_REQUIRE(bits, "packed_correlation: bits is null");
  DVG_REQUIRE(pair_sum, "packed_correlation: pair_sum is null");
  DVG_REQUIRE(ws, "packed_correlation: ws is null");
  DVG_REQUIRE(((uintptr_t)ws & 15) == 0, "packed_correlation: ws=%p is not aligned to 16 bytes", ws);
  DVG_REQUIRE(n >= 1, "packed_correlation: n=%d must be at least 1", n);
  const int64_t W = ((int64_t)n + 31) / 32;
  DVG_TRY(check_row_geometry("packed_correlation", rows, groups, row_stride, W, group_stride));
  DVG_TRY(check_spin_count("packed_correlation", n, CR_MAX_N, "the limit of the packed-row entries"));
  DVG_TRY(check_row_count("packed_correlation", rows, groups));
  const int64_t total = groups * rows, Kp = cr_col_words(total), chunks = Kp / CR_KC;
  if (ceil_div(chunks, CR_SLAB_CHUNKS) > 0x7fffffff) {
    set_error("packed_correlation: groups=%lld x rows=%lld is more than one launch takes", (long long)groups, (long long)rows);
    return DVG_E_UNSUPPORTED;
  }
  const size_t need = (size_t)n * (size_t)Kp * sizeof(uint64_t);
  if (ws_bytes < need) {
    set_error("packed_correlation: ws_bytes=%zu is less than the %zu bytes of dvg_packed_correlation_workspace_bytes", ws_bytes, need);
    return DVG_E_WORKSPACE;
  }
  hipStream_t s = (hipStream_t)stream;
  if (!accumulate) {
    DVG_CHECK_HIP(hipMemsetAsync(pair_sum, 0, sizeof(int64_t) * (size_t)n * (size_t)n, s));
    if (spin_sum) DVG_CHECK_HIP(hipMemsetAsync(spin_sum, 0, sizeof(int64_t) * (size_t)n, s));
  }
  const int64_t jobs = Kp / CT_TILES;
  DVG_LAUNCH(K_CORR_TRANSPOSE, packed_correlation_transpose_kernel,
             dim3((unsigned)(jobs < CT_GRID ? jobs : CT_GRID), (unsigned)ceil_div(W, CT_WORDS)), dim3(CT_TILES * 64), 0, s, bits, rows,
             row_stride, groups, group_stride, n, (int)W, Kp, reinterpret_cast<unsigned long long*>(ws),
             reinterpret_cast<unsigned long long*>(spin_sum));
  // slabs: the rows are split as far as it takes to fill the chip (36 upper tile pairs at n = 512), and never less than the
  // 32-bit counts allow
  const int nt = (int)ceil_div(n, CR_TILE);
  const int64_t pairs = (int64_t)nt * (nt + 1) / 2;
  int64_t slabs = ceil_div(CR_TARGET_WGS, pairs);
  slabs = slabs > chunks ? chunks : slabs;
  int64_t slab_chunks = ceil_div(chunks, slabs);
  slab_chunks = slab_chunks > CR_SLAB_CHUNKS ? CR_SLAB_CHUNKS : slab_chunks;
  slabs = ceil_div(chunks, slab_chunks);
  DVG_LAUNCH_WORK(K_CORR_PRODUCT, (double)n * (double)n * (double)total, packed_correlation_kernel,
                  dim3((unsigned)slabs, (unsigned)pairs), dim3(CR_THREADS), 0, s, reinterpret_cast<const uint32_t*>(ws), total, chunks,
                  slab_chunks, n, nt, reinterpret_cast<unsigned long long*>(pair_sum));
  return DVG_OK;
}
