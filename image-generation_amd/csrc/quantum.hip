// Simulated quantum annealing draws (dvg_gibbs_sample_quantum, "DVG SQA v1", include/dvg.h): path-integral Monte Carlo of the
// transverse-field Ising model -- chains of P Trotter slices of the sampler's n spins, Gibbs-sampled class by class under a
// per-sweep table of the slices' classical beta and of the ferromagnetic coupling kappa along imaginary time.  One
// stream-ordered launch, no workgroup waiting on another, no atomics.
#include "common.h"
#include "graph.h"
#include "packed_rows.h"
#include "philox.h"
#include <cmath>

namespace dvg {

// A TILE is 64 lanes = 64 / P consecutive chains x P slices: lane l holds chain tile (64 / P) + l / P, slice l mod P -- row
// tile 64 + l of the dense [n_chains][P][W] packed rows.  Workgroup b of QA_WAVES waves takes the tiles b, b + gridDim.x, ..; a
// chain's result depends on that chain alone, so the grid cannot show in any output.
// Per tile: the ballot transpose (tile_columns_halves, packed_rows.h) -- or, with `init`, one ballot per spin of the INIT
// stream's bit -- puts the per-spin bit columns in LDS as halves lo[spin] (lanes 0..31) and lo[n + spin] (lanes 32..63).  Then
// the sweeps.  In class k wave v takes the spins order[class_ptr[k] + v], order[class_ptr[k] + v + QA_WAVES], ..: a spin is
// wave-uniform; its classical field is local_field (packed_rows.h) for all 64 slices at once -- it does not depend on the
// spin's own column, so one sum serves both half-steps -- and so is the lane's random word.  The spin's 64-bit column is
// read once (one address for all lanes, made scalar); the neighbours of lane l along imaginary time are the column's bits
// (l & ~(P - 1)) | ((l +- 1) & (P - 1)), two shifts.  The even lanes decide on it and their ballot replaces the column's even
// bits, in registers; the odd lanes decide on the merged column; lane 0 stores both halves once.  No spin of a class reads
// another spin of it, so the waves need no order inside a class; one barrier sits behind every class.  Lanes beyond
// n_chains P ride along with their ballot bits forced to 0 and store nothing (a chain's slices share a tile, so a live lane's
// neighbours are live).
// The way out: samples_out from bit "slice 0" of each of the tile's chains, consecutive threads on consecutive spins; the
// rows through tile_rows_from_halves (packed_rows.h), which writes the pad bits as 0.
// LDS: 8 n bytes of columns, 64 KiB at n = 8192.  Banks (ds_read_b32 / ds_write_b32: dword mod 32 in 32-lane halves): the
// transpose writes 32 consecutive dwords; the INIT ballots and the sweeps have one lane write; the field sum and the column
// read take one address per half (a broadcast); the way back and samples_out read consecutive dwords.  No conflict by the rule.
constexpr int QA_WAVES = 8, QA_THREADS = QA_WAVES * 64, QA_MAX_N = 8192, QA_MAX_GRID = 1024;

// s = +1 for this lane's slice: bf = rn(beta_slice f), the neighbours' bits `up`, `dn` of the spin's column, u the lane's
// uniform -- z0 = rn(bf - rn(kappa nb)), then the last lines of the plain draw's decision at two_beta f = rn(2 z0)
__device__ __forceinline__ bool quantum_decide(float bf, float kappa, unsigned long long col, int up, int dn, float u) {
  const float nb = (float)(2 * (int)(((col >> up) & 1ull) + ((col >> dn) & 1ull)) - 2);  // s[k-1] + s[k+1]: -2, 0, 2
  const float z0 = __fsub_rn(bf, __fmul_rn(kappa, nb));
  const float z = fminf(fmaxf(__fmul_rn(2.0f, z0), -87.0f), 87.0f);
  const float tt = spec_exp(z);
  return __fmul_rn(u, __fadd_rn(1.0f, tt)) < 1.0f;
}

__global__ __launch_bounds__(QA_THREADS) void gibbs_quantum_kernel(
    uint32_t* slices, int n_chains, int log2_slices, int n, int W, int n_colours, const int32_t* __restrict__ order,
    const int32_t* __restrict__ class_ptr, const int32_t* __restrict__ adj_ptr, const int32_t* __restrict__ adj_idx,
    const int32_t* __restrict__ adj_eid, const float* __restrict__ h, const float* __restrict__ J, float prefactor, float h_lo,
    float h_hi, float j_lo, float j_hi, const float* __restrict__ beta_slice, const float* __restrict__ kappa, uint32_t chain_id0,
    uint32_t k0, uint32_t k1, uint32_t sweep0, int n_sweeps, int init, float* __restrict__ samples_out) {
  extern __shared__ __align__(16) uint32_t qa_lo[];  // [n] lanes 0..31 of the tile, then [n] lanes 32..63
  uint32_t* lo = qa_lo;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const uint32_t* mine = lane < 32 ? lo : lo + n;  // the halves that hold this lane's bit
  const int to_sign = 31 - (lane & 31);
  const int P = 1 << log2_slices, per_tile = 64 >> log2_slices;  // slices of a chain, chains of a tile
  const int slice = lane & (P - 1), first = lane & ~(P - 1);
  const int up = first | ((lane + 1) & (P - 1)), dn = first | ((lane - 1) & (P - 1));
  const bool even = (lane & 1) == 0;
  constexpr unsigned long long EVEN = 0x5555555555555555ull;
  const int64_t total = (int64_t)n_chains << log2_slices, n_tiles = (total + 63) >> 6;
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int64_t chain = tile * per_tile + (lane >> log2_slices);
    const bool live = chain < n_chains;
    const uint32_t cid = chain_id0 + (uint32_t)chain;
    if (init) {
      for (int i = wave; i < n; i += QA_WAVES) {
        const u32x4 r = philox4x32_10((uint32_t)i, cid, sweep0, STREAM_INIT | ((uint32_t)slice << 8), k0, k1);
        const unsigned long long m = __builtin_amdgcn_ballot_w64(live && (r.x >> 31) != 0u);
        if (lane == 0) {
          lo[i] = (uint32_t)m;
          lo[n + i] = (uint32_t)(m >> 32);
        }
      }
    } else {
      tile_columns_halves<QA_WAVES>(live ? slices + (tile * 64 + lane) * W : nullptr, W, n, wave, lane, lo);
    }
    __syncthreads();
    // ---- the sweeps
    for (int k = 0; k < n_sweeps; ++k) {
      const float bs = beta_slice[k], kp = kappa[k];
      const uint32_t t = sweep0 + (uint32_t)k;
      for (int c = 0; c < n_colours; ++c) {
        const int u1 = class_ptr[c + 1];
        for (int u = class_ptr[c] + wave; u < u1; u += QA_WAVES) {
          const int i = order[u];
          const float f = local_field(i, lane, mine, to_sign, adj_ptr, adj_idx, adj_eid, h, J, prefactor, h_lo, h_hi, j_lo, j_hi);
          const float bf = __fmul_rn(bs, f);
          const float unit = u32_to_unit(philox4x32_10((uint32_t)i, cid, t, STREAM_SQA | ((uint32_t)slice << 8), k0, k1).x);
          unsigned long long col = ((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)lo[n + i]) << 32) |
                                   (uint32_t)__builtin_amdgcn_readfirstlane((int)lo[i]);
          const unsigned long long ev = __builtin_amdgcn_ballot_w64(live && even && quantum_decide(bf, kp, col, up, dn, unit));
          col = (col & ~EVEN) | ev;
          const unsigned long long od = __builtin_amdgcn_ballot_w64(live && !even && quantum_decide(bf, kp, col, up, dn, unit));
          col = (col & EVEN) | od;
          if (lane == 0) {
            lo[i] = (uint32_t)col;
            lo[n + i] = (uint32_t)(col >> 32);
          }
        }
        __syncthreads();
      }
    }
    // ---- the way out: slice 0 of each chain as float32 +-1, then the rows
    if (samples_out) {
      for (int e = tid; e < per_tile * n; e += QA_THREADS) {
        const int cl = e / n, i = e - cl * n, b = cl << log2_slices;
        const int64_t ch = tile * per_tile + cl;
        if (ch < n_chains) samples_out[ch * n + i] = (((b < 32 ? lo[i] : lo[n + i]) >> (b & 31)) & 1u) ? 1.0f : -1.0f;
      }
    }
    tile_rows_from_halves<QA_WAVES>(mine, W, n, wave, lane, tile, total, slices);
    __syncthreads();  // (the columns are rewritten by the next tile)
  }
}

}  // namespace dvg

using namespace dvg;

extern "C" int dvg_gibbs_sample_quantum(const dvg_graph_t* g, const float* linear, const float* quadratic, float prefactor,
                                        float h_lo, float h_hi, float j_lo, float j_hi, const float* beta_slice,
                                        const float* kappa, uint32_t* slices, int n_chains, int n_slices, uint32_t chain_id0,
                                        uint64_t seed, uint32_t sweep0, int n_sweeps, int init, float* samples_out,
                                        dvg_stream_t stream) {
  DVG_REQUIRE(g, "gibbs_quantum: g is null");
  DVG_REQUIRE(linear, "gibbs_quantum: linear is null");
  DVG_REQUIRE(quadratic, "gibbs_quantum: quadratic is null");
  DVG_REQUIRE(beta_slice, "gibbs_quantum: beta_slice is null");
  DVG_REQUIRE(kappa, "gibbs_quantum: kappa is null (a draw without slices is dvg_gibbs_sample_annealed)");
  DVG_REQUIRE(slices, "gibbs_quantum: slices is null");
  DVG_REQUIRE(n_chains >= 1, "gibbs_quantum: n_chains=%d must be at least 1", n_chains);
  DVG_REQUIRE(n_sweeps >= 1, "gibbs_quantum: n_sweeps=%d must be at least 1 (the tables have an entry per sweep)", n_sweeps);
  DVG_REQUIRE(n_slices >= 2 && n_slices <= 64 && (n_slices & (n_slices - 1)) == 0,
              "gibbs_quantum: n_slices=%d must be a power of two in 2 .. 64", n_slices);
  DVG_REQUIRE(std::isfinite(prefactor), "gibbs_quantum: prefactor=%g is not finite", (double)prefactor);
  const int n = g->n;
  DVG_TRY(check_spin_count("gibbs_quantum", n, QA_MAX_N));
  const int64_t total = (int64_t)n_chains * n_slices;
  if (total >= ((int64_t)1 << 31)) {
    set_error("gibbs_quantum: n_chains=%d x n_slices=%d rows are 2^31 or more", n_chains, n_slices);
    return DVG_E_UNSUPPORTED;
  }
  const int W = (n + 31) / 32, log2_slices = __builtin_ctz((unsigned)n_slices);
  const int64_t n_tiles = ceil_div(total, 64);
  const int grid = (int)(n_tiles < QA_MAX_GRID ? n_tiles : QA_MAX_GRID);
  // work = site updates of the draw
  DVG_LAUNCH_WORK(K_QUANTUM, (double)total * n * n_sweeps, gibbs_quantum_kernel, dim3((unsigned)grid), dim3(QA_THREADS),
                  (size_t)n * 8, (hipStream_t)stream, slices, n_chains, log2_slices, n, W, g->n_colours, g->order, g->class_ptr,
                  g->adj_ptr, g->adj_idx, g->adj_eid, linear, quadratic, prefactor, h_lo, h_hi, j_lo, j_hi, beta_slice, kappa,
                  chain_id0, (uint32_t)seed, (uint32_t)(seed >> 32), sweep0, n_sweeps, init, samples_out);
  return DVG_OK;
}
