// Isoenergetic cluster moves (dvg_gibbs_cluster_move, "DVG ICM v1", include/dvg.h): the holders of one rung in two twin ladders
// exchange their spins on one connected cluster of the sites where they disagree.  Integers only; one stream-ordered launch,
// no atomics, no workgroup waiting on another, no allocation.
#include "common.h"
#include "graph.h"
#include "philox.h"

namespace dvg {

// A JOB is (twin pair p, rung r); a workgroup takes the jobs blockIdx.x, blockIdx.x + gridDim.x, ..: a job reads and writes
// the two rows of its holders and nothing else, so neither the grid nor the order can show in any output.
// A job's two bit sets live in LDS as 64-bit words, one per CHUNK of 64 consecutive spins: D[c] (the sites where the rows
// disagree) and C[c] (the cluster so far).  Wave w owns the chunks w, w + waves, ..: lane l of it is spin 64 c + l.
//   in:    a ballot per chunk of (a[i] < 0) != (b[i] < 0) gives D[c]; consecutive lanes read consecutive bytes of both rows.
//   root:  every thread sums the chunks' popcounts (one address for all lanes: a broadcast), k; the Philox word; the chunk
//          and the bit of element ((uint64)word k) >> 32 of D.  C = that bit.
//   grow:  a pass sets C[c] |= D[c] & (a neighbour is in C): a chunk with no site of D outside C is skipped (wave-uniform);
//          otherwise the lanes of such sites walk their CSR row until a neighbour's bit of C is set, one ballot, lane 0
//          stores.  Only the owner writes C[c]; the other waves' words are read while they grow -- any value read is a subset
//          of the component, C only grows, and a pass in which nobody stored read the final words, so the fixed point is the
//          component whatever the interleaving.  Passes repeat while __syncthreads_or reports a store; each such pass adds
//          a site, so n passes bound the loop on any graph and state.
//   out:   the lanes of C exchange their two bytes: the cluster's bytes of the two rows are the only ones written.
// LDS: 16 bytes per chunk, n / 4 bytes, 16 KiB at n = 65536.  Banks (ds_read_b64: dword mod 64 in 32-lane halves, ds_write_b64
// by one lane): the neighbour gather reads words of C at arbitrary chunks -- equal chunks are one address (a broadcast), and
// up to 32 chunks (n <= 2048) distinct words lie on distinct banks, so the gather is free of conflicts there; beyond, words
// c and c + 32 share their banks and a gather costs at most ceil(chunks / 32) cycles.  Every other access is wave-uniform.
#ifndef DVG_CLUSTER_WAVES
#define DVG_CLUSTER_WAVES 0  // 0: a wave per chunk, CL_MAX_WAVES at the most (a fixed count: the A/B builds of tools/cluster_rate.py)
#endif
constexpr int CL_MAX_WAVES = 16, CL_MAX_N = 65536, CL_MAX_GRID = 4096;

__global__ __launch_bounds__(CL_MAX_WAVES * 64) void gibbs_cluster_kernel(
    int8_t* state, const int32_t* __restrict__ rung, int64_t n_jobs, int R, int rung_from, int n,
    const int32_t* __restrict__ adj_ptr, const int32_t* __restrict__ adj_idx, uint32_t chain_id0, uint32_t k0, uint32_t k1,
    uint32_t move, uint32_t* __restrict__ size_out, uint32_t* __restrict__ differ_out) {
  extern __shared__ __align__(16) unsigned long long cl_words[];  // [chunks] D, then [chunks] C
  const int chunks = (n + 63) >> 6;
  unsigned long long* D = cl_words;
  unsigned long long* C = cl_words + chunks;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), waves = (int)(blockDim.x >> 6);
  for (int64_t job = blockIdx.x; job < n_jobs; job += gridDim.x) {
    const int64_t p = job / R;
    const int r = (int)(job - p * R);
    // ---- the holders of rung r in the ladders 2p and 2p + 1: the lowest chain of each whose clamped rung is r
    int64_t a = -1, b = -1;
    if (r >= rung_from) {
      if (rung) {
        for (int j = R - 1; j >= 0; --j) {
          const int64_t ca = 2 * p * R + j, cb = ca + R;
          if (min(max(rung[ca], 0), R - 1) == r) a = ca;
          if (min(max(rung[cb], 0), R - 1) == r) b = cb;
        }
      } else {  // (R == 1)
        a = 2 * p;
        b = a + 1;
      }
    }
    uint32_t k = 0, size = 0;
    if (a >= 0 && b >= 0) {  // (the same for every thread of the workgroup)
      int8_t* ra = state + a * n;
      int8_t* rb = state + b * n;
      for (int c = wave; c < chunks; c += waves) {
        const int i = c * 64 + lane;
        const unsigned long long m = __builtin_amdgcn_ballot_w64(i < n && ((ra[i] < 0) != (rb[i] < 0)));
        if (lane == 0) {
          D[c] = m;
          C[c] = 0ull;
        }
      }
      __syncthreads();
      for (int c = 0; c < chunks; ++c) k += (uint32_t)__builtin_popcountll(D[c]);
      if (k) {
        const uint32_t word = philox4x32_10((uint32_t)r, chain_id0 + (uint32_t)(2 * p * R), move, STREAM_ICM, k0, k1).x;
        uint32_t t = (uint32_t)(((uint64_t)word * k) >> 32);  // (< k: the walk below ends inside D)
        int c0 = 0;
        for (uint32_t pc; t >= (pc = (uint32_t)__builtin_popcountll(D[c0])); ++c0) t -= pc;
        unsigned long long m = D[c0];
        for (; t; --t) m &= m - 1ull;
        if (tid == 0) C[c0] = m & (0ull - m);
        __syncthreads();
        // ---- grow to the fixed point
        for (int pass = 0; pass < n; ++pass) {
          int stored = 0;
          for (int c = wave; c < chunks; c += waves) {
            const unsigned long long cm = C[c], open = D[c] & ~cm;
            if (!open) continue;
            bool add = false;
            if ((open >> lane) & 1ull) {
              const int i = c * 64 + lane, e1 = adj_ptr[i + 1];
              for (int e = adj_ptr[i]; e < e1 && !add; ++e) {
                const int j = adj_idx[e];
                add = (C[j >> 6] >> (j & 63)) & 1ull;
              }
            }
            const unsigned long long g = __builtin_amdgcn_ballot_w64(add);
            if (g) {
              if (lane == 0) C[c] = cm | g;
              stored = 1;
            }
          }
          if (!__syncthreads_or(stored)) break;
        }
        // ---- the way out: the cluster's sites change places
        for (int c = wave; c < chunks; c += waves) {
          const int i = c * 64 + lane;
          if ((C[c] >> lane) & 1ull) {
            const int8_t x = ra[i], y = rb[i];
            ra[i] = y;
            rb[i] = x;
          }
        }
        for (int c = 0; c < chunks; ++c) size += (uint32_t)__builtin_popcountll(C[c]);
      }
    }
    if (tid == 0) {
      if (size_out) size_out[job] = size;
      if (differ_out) differ_out[job] = k;
    }
    __syncthreads();  // (the words are rewritten by the next job)
  }
}

}  // namespace dvg

using namespace dvg;

extern "C" int dvg_gibbs_cluster_move(const dvg_graph_t* g, int8_t* state, const int32_t* rung, int n_chains, int n_replicas,
                                      int rung_from, uint32_t chain_id0, uint64_t seed, uint32_t move, uint32_t* size_out,
                                      uint32_t* differ_out, dvg_stream_t stream) {
  DVG_REQUIRE(g, "gibbs_cluster_move: g is null");
  DVG_REQUIRE(state, "gibbs_cluster_move: state is null");
  DVG_REQUIRE(n_replicas >= 1 && n_replicas <= 16, "gibbs_cluster_move: n_replicas=%d must be 1 .. 16", n_replicas);
  DVG_REQUIRE(rung || n_replicas == 1, "gibbs_cluster_move: rung is null with n_replicas=%d (only single chains need no table)",
              n_replicas);
  DVG_REQUIRE(n_chains >= 2, "gibbs_cluster_move: n_chains=%d must be at least 2 (a pair of twins)", n_chains);
  DVG_REQUIRE(n_chains % (2 * n_replicas) == 0, "gibbs_cluster_move: n_chains=%d is not a multiple of 2 n_replicas=%d (twin ladders)",
              n_chains, 2 * n_replicas);
  DVG_REQUIRE(rung_from >= 0 && rung_from < n_replicas, "gibbs_cluster_move: rung_from=%d must be 0 .. %d", rung_from, n_replicas - 1);
  const int n = g->n;
  DVG_REQUIRE(n >= 1, "gibbs_cluster_move: the graph has n=%d spins", n);
  if (n > CL_MAX_N) {
    set_error("gibbs_cluster_move: n=%d > %d (a job's two bit sets are kept in %d KiB of LDS)", n, CL_MAX_N, CL_MAX_N / 4 / 1024);
    return DVG_E_UNSUPPORTED;
  }
  const int chunks = (n + 63) / 64;
  const int64_t n_jobs = (int64_t)n_chains / 2;  // pairs x R
  const int grid = (int)(n_jobs < CL_MAX_GRID ? n_jobs : CL_MAX_GRID);
  const int waves = DVG_CLUSTER_WAVES ? DVG_CLUSTER_WAVES : (chunks < CL_MAX_WAVES ? chunks : CL_MAX_WAVES);
  // work = spins x jobs (x the passes, which only the device knows: per pass)
  DVG_LAUNCH_WORK(K_CLUSTER, (double)n * (double)n_jobs, gibbs_cluster_kernel, dim3((unsigned)grid), dim3((unsigned)waves * 64),
                  (size_t)chunks * 16, (hipStream_t)stream, state, rung, n_jobs, n_replicas, rung_from, n, g->adj_ptr, g->adj_idx,
                  chain_id0, (uint32_t)seed, (uint32_t)(seed >> 32), move, size_out, differ_out);
  return DVG_OK;
}
