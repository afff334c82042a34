// Population annealing's resampling step ("DVG PA v1", include/dvg.h): systematic resampling of weighed chains in exact
// integer arithmetic.  Per population of R chains: the maximum log weight, the integer weights k_c = trunc(spec_exp(lw_c -
// max) 2^32), their uint64 prefix sums S, one Philox offset V, and for child j the smallest c with S_c > floor((j K + V) / R);
// then the parents' state rows are gathered.  A population of up to PR_TILE chains is one workgroup (max, weights and scan in
// LDS, the search over LDS); larger ones take stream-ordered launches -- block maxima, block sums, a scan of the sums, the
// prefix sums of every block, the search over them in global memory -- and no workgroup ever waits for another.
#include "common.h"
#include "philox.h"

namespace dvg {

constexpr int PR_THREADS = 256;                 // four waves
constexpr int PR_ITEMS = 4;                     // consecutive chains per thread
constexpr int PR_TILE = PR_THREADS * PR_ITEMS;  // chains per workgroup
constexpr int PR_MAX_R = 1 << 20;               // K = sum k <= 2^52: j q, j rem + V and S stay below 2^53
constexpr int PR_GATHER_BLOCKS = 2048;          // grid-stride cap of the gather: 8 blocks of 256 threads per CU

// k_c of the definition: one float64 subtraction, rounded to float32, clamped, spec_exp, scaled by 2^32 (exact), truncated
__device__ __forceinline__ uint64_t pr_weight(double lw, double m) {
  float z = __double2float_rn(__dsub_rn(lw, m));
  z = fminf(fmaxf(z, -87.0f), 0.0f);
  return __double2ull_rz(__dmul_rn((double)spec_exp(z), 4294967296.0));
}

__device__ __forceinline__ double pr_block_max(double v, double* red) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = fmax(v, __shfl_xor(v, o));
  const int tid = threadIdx.x;
  if ((tid & 63) == 0) red[tid >> 6] = v;
  __syncthreads();
  v = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
  __syncthreads();
  return v;
}

// Inclusive scan of the workgroup's PR_TILE values, PR_ITEMS consecutive ones per thread: k[] becomes the inclusive prefix
// sums within the workgroup; returns the workgroup's total.
__device__ __forceinline__ uint64_t pr_block_scan(uint64_t (&k)[PR_ITEMS], uint64_t* red) {
#pragma unroll
  for (int i = 1; i < PR_ITEMS; ++i) k[i] += k[i - 1];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  uint64_t incl = k[PR_ITEMS - 1];
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint64_t up = __shfl_up(incl, o);
    if (lane >= o) incl += up;
  }
  if (lane == 63) red[wave] = incl;
  __syncthreads();
  uint64_t before = incl - k[PR_ITEMS - 1], total = 0;
#pragma unroll
  for (int w = 0; w < PR_THREADS / 64; ++w) {
    if (w < wave) before += red[w];
    total += red[w];
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < PR_ITEMS; ++i) k[i] += before;
  return total;
}

// V of the definition: uniform in [0, K) from the population's own Philox word
__device__ __forceinline__ uint64_t pr_offset(uint32_t first_chain_id, uint32_t step, uint32_t k0, uint32_t k1, uint64_t K) {
  const u32x4 o = philox4x32_10(0u, first_chain_id, step, STREAM_RESAMPLE, k0, k1);
  return __umul64hi(((uint64_t)o.x << 32) | o.y, K);
}

// the smallest c in 0 .. R-1 with S[c] > t (S is non-decreasing and S[R-1] = K > t); never leaves 0 .. R-1 whatever S holds
template <class Ptr>
__device__ __forceinline__ int pr_search(Ptr S, int R, uint64_t t) {
  int lo = 0, hi = R - 1;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (S[mid] > t) hi = mid; else lo = mid + 1;
  }
  return lo;
}

__device__ __forceinline__ void pr_emit(int base, int j, int c, const int32_t* family_in, int32_t* family_out, int32_t* parent_out) {
  parent_out[base + j] = base + c;
  if (family_out) family_out[base + j] = family_in ? family_in[base + c] : base + c;
}

// ---------------------------------------------------------------- one workgroup per population, R <= PR_TILE
__global__ __launch_bounds__(PR_THREADS) void population_small_kernel(const double* __restrict__ lw, int R, uint32_t chain_id0,
                                                                      uint32_t k0, uint32_t k1, uint32_t step,
                                                                      const int32_t* __restrict__ family_in,
                                                                      int32_t* __restrict__ family_out,
                                                                      int32_t* __restrict__ parent_out,
                                                                      uint64_t* __restrict__ weight_out) {
  __shared__ uint64_t S[PR_TILE];
  __shared__ uint64_t red[PR_THREADS / 64];
  const int tid = threadIdx.x, base = blockIdx.x * R, c0 = tid * PR_ITEMS;
  double v[PR_ITEMS], m = -INFINITY;
#pragma unroll
  for (int i = 0; i < PR_ITEMS; ++i) {
    v[i] = c0 + i < R ? lw[base + c0 + i] : -INFINITY;
    m = fmax(m, v[i]);
  }
  m = pr_block_max(m, reinterpret_cast<double*>(red));
  uint64_t k[PR_ITEMS];
#pragma unroll
  for (int i = 0; i < PR_ITEMS; ++i) {
    k[i] = c0 + i < R ? pr_weight(v[i], m) : 0;
    if (weight_out && c0 + i < R) weight_out[base + c0 + i] = k[i];
  }
  const uint64_t K = pr_block_scan(k, red);
#pragma unroll
  for (int i = 0; i < PR_ITEMS; ++i) S[c0 + i] = k[i];
  __syncthreads();
  const uint64_t V = pr_offset(chain_id0 + (uint32_t)base, step, k0, k1, K);
  const uint64_t q = K / (uint64_t)R, rem = K % (uint64_t)R;
  for (int j = tid; j < R; j += PR_THREADS) {
    const uint64_t t = (uint64_t)j * q + ((uint64_t)j * rem + V) / (uint64_t)R;
    pr_emit(base, j, pr_search(S, R, t), family_in, family_out, parent_out);
  }
}

// ---------------------------------------------------------------- populations of more than PR_TILE chains: separate launches
// grid (P, nb): block (p, b) holds chains b PR_TILE .. of population p; the workspace's rows are [p nb + b]
__global__ __launch_bounds__(PR_THREADS) void population_block_max_kernel(const double* __restrict__ lw, int R,
                                                                          double* __restrict__ bmax) {
  __shared__ double red[PR_THREADS / 64];
  const int tid = threadIdx.x, c0 = blockIdx.y * PR_TILE + tid * PR_ITEMS;
  const int64_t base = (int64_t)blockIdx.x * R;
  double m = -INFINITY;
#pragma unroll
  for (int i = 0; i < PR_ITEMS; ++i)
    if (c0 + i < R) m = fmax(m, lw[base + c0 + i]);
  m = pr_block_max(m, red);
  if (tid == 0) bmax[(int64_t)blockIdx.x * gridDim.y + blockIdx.y] = m;
}

// WRITE = false: the block's sum of k into bsum.  WRITE = true: the block's prefix sums, its offset boff added, into S (and
// k into weight_out).  Both recompute the population's maximum from the nb block maxima (the maximum is exact in any order).
template <bool WRITE>
__global__ __launch_bounds__(PR_THREADS) void population_block_sum_kernel(const double* __restrict__ lw, int R,
                                                                          const double* __restrict__ bmax,
                                                                          uint64_t* __restrict__ bsum,
                                                                          const uint64_t* __restrict__ boff,
                                                                          uint64_t* __restrict__ S,
                                                                          uint64_t* __restrict__ weight_out) {
  __shared__ uint64_t red[PR_THREADS / 64];
  const int tid = threadIdx.x, nb = gridDim.y, c0 = blockIdx.y * PR_TILE + tid * PR_ITEMS;
  const int64_t base = (int64_t)blockIdx.x * R, row = (int64_t)blockIdx.x * nb;
  double m = -INFINITY;
  for (int b = tid; b < nb; b += PR_THREADS) m = fmax(m, bmax[row + b]);
  m = pr_block_max(m, reinterpret_cast<double*>(red));
  uint64_t k[PR_ITEMS];
#pragma unroll
  for (int i = 0; i < PR_ITEMS; ++i) {
    k[i] = c0 + i < R ? pr_weight(lw[base + c0 + i], m) : 0;
    if (WRITE && weight_out && c0 + i < R) weight_out[base + c0 + i] = k[i];
  }
  const uint64_t total = pr_block_scan(k, red);
  if (!WRITE) {
    if (tid == 0) bsum[row + blockIdx.y] = total;
  } else {
    const uint64_t off = boff[row + blockIdx.y];
#pragma unroll
    for (int i = 0; i < PR_ITEMS; ++i)
      if (c0 + i < R) S[base + c0 + i] = k[i] + off;
  }
}

// grid (P): the exclusive scan of a population's nb <= PR_TILE block sums, its K and its offset V
__global__ __launch_bounds__(PR_THREADS) void population_scan_sums_kernel(const uint64_t* __restrict__ bsum, int nb, int R,
                                                                          uint32_t chain_id0, uint32_t k0, uint32_t k1,
                                                                          uint32_t step, uint64_t* __restrict__ boff,
                                                                          uint64_t* __restrict__ KV) {
  __shared__ uint64_t red[PR_THREADS / 64];
  const int tid = threadIdx.x, b0 = tid * PR_ITEMS;
  const int64_t row = (int64_t)blockIdx.x * nb;
  uint64_t k[PR_ITEMS], own[PR_ITEMS];
#pragma unroll
  for (int i = 0; i < PR_ITEMS; ++i) own[i] = k[i] = b0 + i < nb ? bsum[row + b0 + i] : 0;
  const uint64_t K = pr_block_scan(k, red);
#pragma unroll
  for (int i = 0; i < PR_ITEMS; ++i)
    if (b0 + i < nb) boff[row + b0 + i] = k[i] - own[i];
  if (tid == 0) {
    KV[2 * blockIdx.x] = K;
    KV[2 * blockIdx.x + 1] = pr_offset(chain_id0 + (uint32_t)((int64_t)blockIdx.x * R), step, k0, k1, K);
  }
}

// grid (P, ceil(R / PR_THREADS)): child j of population p searches the population's S in global memory
__global__ __launch_bounds__(PR_THREADS) void population_search_kernel(const uint64_t* __restrict__ S, int R,
                                                                       const uint64_t* __restrict__ KV,
                                                                       const int32_t* __restrict__ family_in,
                                                                       int32_t* __restrict__ family_out,
                                                                       int32_t* __restrict__ parent_out) {
  const int j = blockIdx.y * PR_THREADS + threadIdx.x;
  if (j >= R) return;
  const int base = blockIdx.x * R;
  const uint64_t K = KV[2 * blockIdx.x], V = KV[2 * blockIdx.x + 1];
  const uint64_t q = K / (uint64_t)R, rem = K % (uint64_t)R;
  const uint64_t t = (uint64_t)j * q + ((uint64_t)j * rem + V) / (uint64_t)R;
  pr_emit(base, j, pr_search(S + base, R, t), family_in, family_out, parent_out);
}

// ---------------------------------------------------------------- the gather: state_out[j] = state_in[parent[j]]
// A row is `upr` units of T; unit u of the call is unit u % upr of row u / upr.  n bytes in and n bytes out per chain.
template <class T>
__global__ __launch_bounds__(PR_THREADS) void population_gather_kernel(const T* __restrict__ in, T* __restrict__ out,
                                                                       const int32_t* __restrict__ parent, int64_t units,
                                                                       int upr) {
  const int64_t stride = (int64_t)gridDim.x * PR_THREADS;
  for (int64_t u = (int64_t)blockIdx.x * PR_THREADS + threadIdx.x; u < units; u += stride) {
    const int64_t j = u / upr;
    const int col = (int)(u - j * upr);
    out[u] = in[(int64_t)parent[j] * upr + col];
  }
}

template <class T>
static int launch_gather(const int8_t* in, int8_t* out, const int32_t* parent, int n_chains, int n, hipStream_t s) {
  const int upr = n / (int)sizeof(T);
  const int64_t units = (int64_t)n_chains * upr;
  const int64_t blocks = ceil_div(units, PR_THREADS);
  DVG_LAUNCH(K_GRBM_SUFFSTATS, population_gather_kernel<T>, dim3((unsigned)(blocks < PR_GATHER_BLOCKS ? blocks : PR_GATHER_BLOCKS)),
             dim3(PR_THREADS), 0, s, reinterpret_cast<const T*>(in), reinterpret_cast<T*>(out), parent, units, upr);
  return DVG_OK;
}

// slots of the block maxima / sums / offsets of the large path: P ceil(R / PR_TILE) <= n_chains / PR_TILE + P, P < n_chains / PR_TILE
static size_t pr_slots(int n_chains) { return (size_t)n_chains / PR_TILE * 2 + 2; }

}  // namespace dvg

using namespace dvg;

extern "C" size_t dvg_population_resample_workspace_bytes(int n_chains) {
  if (n_chains < 1) return 0;
  // S [n_chains], then bmax, bsum, boff [slots] and (K, V) [2 slots]
  return align_up(sizeof(uint64_t) * ((size_t)n_chains + 5 * pr_slots(n_chains)), 256);
}

extern "C" int dvg_population_resample(const double* log_weight, int n_chains, int n_populations, uint32_t chain_id0,
                                       uint64_t seed, uint32_t step, const int8_t* state_in, int8_t* state_out, int n,
                                       const int32_t* family_in, int32_t* family_out, int32_t* parent_out,
                                       uint64_t* weight_out, void* ws, size_t ws_bytes, dvg_stream_t stream) {
  DVG_REQUIRE(log_weight, "population_resample: log_weight is null");
  DVG_REQUIRE(parent_out, "population_resample: parent_out is null");
  DVG_REQUIRE(ws, "population_resample: ws is null");
  DVG_REQUIRE(n_chains >= 1, "population_resample: n_chains=%d must be at least 1", n_chains);
  DVG_REQUIRE(n_populations >= 1, "population_resample: n_populations=%d must be at least 1", n_populations);
  DVG_REQUIRE(n_chains % n_populations == 0, "population_resample: n_chains=%d is not a multiple of n_populations=%d", n_chains,
              n_populations);
  DVG_REQUIRE((state_in == nullptr) == (state_out == nullptr),
              "population_resample: state_in and state_out go together, %s is null", state_in ? "state_out" : "state_in");
  if (state_in) {
    DVG_REQUIRE(n >= 1, "population_resample: n=%d must be at least 1 with a state", n);
    DVG_REQUIRE(state_in != state_out, "population_resample: state_in == state_out (the gather is out of place)");
  }
  DVG_REQUIRE(!family_out || family_in != family_out, "population_resample: family_in == family_out (the gather is out of place)");
  if (ws_bytes < dvg_population_resample_workspace_bytes(n_chains)) {
    set_error("population_resample: workspace %zu < %zu", ws_bytes, dvg_population_resample_workspace_bytes(n_chains));
    return DVG_E_WORKSPACE;
  }
  const int P = n_populations, R = n_chains / n_populations;
  if (R > PR_MAX_R) {
    set_error("population_resample: R = n_chains / n_populations = %d > %d (the sum of a population's 32-bit weights must stay below 2^53)",
              R, PR_MAX_R);
    return DVG_E_UNSUPPORTED;
  }
  hipStream_t s = (hipStream_t)stream;
  const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
  if (!family_out) family_in = nullptr;
  if (R <= PR_TILE) {
    DVG_LAUNCH(K_GRBM_SUFFSTATS, population_small_kernel, dim3((unsigned)P), dim3(PR_THREADS), 0, s, log_weight, R, chain_id0, k0,
               k1, step, family_in, family_out, parent_out, weight_out);
  } else {
    const int nb = (int)ceil_div(R, PR_TILE);  // <= 1024 = PR_TILE: one workgroup scans a population's block sums
    const size_t slots = pr_slots(n_chains);
    uint64_t* S = (uint64_t*)ws;
    double* bmax = (double*)(S + n_chains);
    uint64_t* bsum = (uint64_t*)(bmax + slots);
    uint64_t* boff = bsum + slots;
    uint64_t* KV = boff + slots;
    const dim3 tiles((unsigned)P, (unsigned)nb);  // (nb <= 1024 and R / PR_THREADS <= 4096 fit a grid's y)
    DVG_LAUNCH(K_GRBM_SUFFSTATS, population_block_max_kernel, tiles, dim3(PR_THREADS), 0, s, log_weight, R, bmax);
    DVG_LAUNCH(K_GRBM_SUFFSTATS, population_block_sum_kernel<false>, tiles, dim3(PR_THREADS), 0, s, log_weight, R,
               (const double*)bmax, bsum, (const uint64_t*)nullptr, (uint64_t*)nullptr, (uint64_t*)nullptr);
    DVG_LAUNCH(K_GRBM_SUFFSTATS, population_scan_sums_kernel, dim3((unsigned)P), dim3(PR_THREADS), 0, s, (const uint64_t*)bsum, nb,
               R, chain_id0, k0, k1, step, boff, KV);
    DVG_LAUNCH(K_GRBM_SUFFSTATS, population_block_sum_kernel<true>, tiles, dim3(PR_THREADS), 0, s, log_weight, R,
               (const double*)bmax, (uint64_t*)nullptr, (const uint64_t*)boff, S, weight_out);
    DVG_LAUNCH(K_GRBM_SUFFSTATS, population_search_kernel, dim3((unsigned)P, (unsigned)ceil_div(R, PR_THREADS)), dim3(PR_THREADS),
               0, s, (const uint64_t*)S, R, (const uint64_t*)KV, family_in, family_out, parent_out);
  }
  if (state_in) {
    const uintptr_t both = (uintptr_t)state_in | (uintptr_t)state_out | (uintptr_t)n;
    if (both % 16 == 0) DVG_TRY(launch_gather<uint4>(state_in, state_out, parent_out, n_chains, n, s));
    else if (both % 4 == 0) DVG_TRY(launch_gather<uint32_t>(state_in, state_out, parent_out, n_chains, n, s));
    else DVG_TRY(launch_gather<uint8_t>(state_in, state_out, parent_out, n_chains, n, s));
  }
  return DVG_OK;
}
