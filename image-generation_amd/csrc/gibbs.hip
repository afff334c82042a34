// Many-chain graph-coloured block-Gibbs sampler for the GRBM prior (stands in for
// the QPU draw of /root/reference/src/model_wrapper.py:309-316).  Bit-exact
// against oracle/gibbs.py ("DVG block-Gibbs v1").
//
// Mapping: a workgroup stages the graph once into LDS (h, CSR neighbours with
// their couplings; coalesced HBM reads of the J/h tensors) and each group of LPC
// lanes of a wavefront owns one chain whose +-1 state lives in LDS for all sweeps.
// Within a colour class spins are conditionally independent, so the lanes update
// them simultaneously; classes are separated by a wavefront-level fence only (no
// workgroup barrier: chains never interact).
#include <cstdlib>
#include <type_traits>
#include <utility>

#include "common.h"
#include "gibbs_plan.h"
#include "graph.h"
#include "philox.h"

namespace dvg {

struct GibbsArgs {
  const int32_t *order, *class_ptr, *adj_idx, *adj_eid;
  const int32_t *adj_row, *adj_src4;  // padded-row image (graph.h)
  const int32_t *lane_spin, *lane_eid;  // lane-major image (graph.h); null: none for this graph
  const uint16_t* lane_off;
  int n_rows;                           // fast kernel: rows of that image
  const float *linear, *quadratic;
  int n, n_batches, max_batches, n_colours;
  float prefactor, h_lo, h_hi, j_lo, j_hi, two_beta;
  int8_t* state;
  float* samples_out;
  int n_chains;
  uint32_t chain_id0, k0, k1, sweep0;
  const uint32_t* sweep0_dev;  // non-null: read the first-sweep index from device memory (graph replay)
  int n_sweeps, init;
};

// Conditional draws (dvg_gibbs_sample_clamped): some spins of a chain are HELD at the value they have in `state` -- left
// out of their colour class, nothing else changed (they still feed their neighbours' field sums).  The kernels carry the
// held path as a compile-time variant, HELD, whose argument block is the plain one plus the flags: the instantiations
// of the plain draw keep their arguments and their code.
struct GibbsHeldArgs : GibbsArgs {
  const uint8_t* clamp;   // [n_chains or 1][n]: nonzero = held
  int64_t clamp_stride;   // n (a row per chain) or 0 (one row for all chains)
};
// Annealed draws (dvg_gibbs_sample_annealed): the inverse temperature of a sweep is looked up in a device table, by the
// sweep's index within the call and, with a row per chain, by the chain.  A second compile-time variant, SCHED, carried
// the same way: the plain block plus the table.  (HELD with SCHED: no such draw.)
struct GibbsSchedArgs : GibbsArgs {
  const float* betas;   // [n_chains or 1][n_sweeps]: beta of sweep k of the call (finite, >= 0: not checked)
  int64_t beta_stride;  // n_sweeps (a row per chain) or 0 (one row for all chains)
};
// AIS draws (dvg_gibbs_sample_ais): the annealed draw, weighed -- per chain the energy of its state under the scaled, clamped
// (h, J), carried along from the local fields the updates compute anyway, and the log importance weight
// -sum_k (beta_k - beta_{k-1}) E^(k) of annealed importance sampling ("DVG AIS v1", include/dvg.h).  SCHED is a mode: 0 fixed
// beta, GIBBS_TABLE the table, GIBBS_WEIGH the table and the two float64 accumulators.  The spins are the annealed draw's.
struct GibbsAisArgs : GibbsSchedArgs {
  float beta_from;         // beta_{-1}: the inverse temperature the start states are a sample of
  double* log_weight_out;  // [n_chains]
  double* energy_out;      // [n_chains] or null
};
// Exchange draws (dvg_gibbs_sample_tempered, "DVG PT v1" in include/dvg.h): replica exchange.  The chains come in ladders of
// n_replicas consecutive chains; a chain sweeps at the beta of the RUNG it holds, carries its energy as the AIS draw does, and
// every swap_every sweeps neighbouring rungs of a ladder change hands on a Metropolis coin.  A fourth mode of SCHED,
// GIBBS_EXCHANGE: the plain block plus the ladder and the three outputs.  A workgroup holds whole ladders (gibbs_exchange_plan).
struct GibbsExchangeArgs : GibbsArgs {
  const float* ladder;   // [n_replicas]: beta of rung r
  int n_replicas, swap_every;
  int32_t* rung;         // [n_chains] in/out: the rung chain c holds
  double* energy_out;    // [n_chains] by rung, or null
  uint32_t* accept_out;  // [n_chains]: element q R + r = accepted exchanges of the pair (r, r + 1) of ladder q; or null
};
// Traced draws (dvg_gibbs_sample_traced, "DVG trace v1" in include/dvg.h): the plain draw, with the chain's state written out
// after chosen sweeps as one BIT per spin.  A fifth mode of SCHED, GIBBS_TRACE: the plain block plus the trace and which sweeps
// it takes.  It runs at the fixed beta: the branches that read a beta table are `TABLE` (GIBBS_TABLE, GIBBS_WEIGH), not SCHED != 0.
struct GibbsTraceArgs : GibbsArgs {
  uint32_t* trace;       // [n_chains][n_records][(n + 31) / 32]: bit b of word w = spin 32 w + b is +1
  int burn_in, thin;     // sweep k of the call is recorded iff k + 1 > burn_in and (k + 1 - burn_in) % thin == 0
  int n_records;         // (n_sweeps - burn_in) / thin
};
// Traced exchange draws (dvg_gibbs_sample_tempered_traced, "DVG PT trace v1" in include/dvg.h): the exchange draw, with a
// history BY RUNG written out behind the exchange block of chosen sweeps -- the packed row of the chain that now holds rung r,
// its carried energy, and by chain the rung it holds.  A sixth mode of SCHED, GIBBS_EXCHANGE_TRACE: the exchange block plus
// the three outputs and which sweeps they take.  The kernels treat it as GIBBS_EXCHANGE everywhere (`EXCH`); `XTRACE` adds
// the record step alone.
struct GibbsExchangeTraceArgs : GibbsExchangeArgs {
  uint32_t* trace;         // [n_chains][n_records][(n + 31) / 32] by rung: row q R + r = the chain of ladder q holding rung r
  double* energy_trace;    // [n_chains][n_records] by rung, or null
  uint8_t* rung_trace;     // [n_chains][n_records] by chain, or null
  int burn_in, thin;       // the rule of GibbsTraceArgs
  int n_records;           // (n_sweeps - burn_in) / thin
};
// Per-chain-field draws (dvg_gibbs_sample_fields, "DVG field v1" in include/dvg.h): the plain draw, with chain c sampling the
// model whose linear vector is rn(linear + its row of `fields`) -- soft evidence, where HELD is the hard kind.  A seventh mode
// of SCHED, GIBBS_FIELD: the plain block plus the rows.  The rolled kernel alone carries it: a chain's scaled, clamped hs row
// lives in LDS behind the state rows and stands in for the image's shared one; the update is the plain draw's.
struct GibbsFieldArgs : GibbsArgs {
  const float* fields;    // [n_chains or 1][n]: added to `linear`, in its raw units (finite: not checked)
  int64_t field_stride;   // n (a row per chain) or 0 (one row for all chains)
};
// Weighed per-chain-field draws (dvg_gibbs_sample_fields_ais, "DVG field AIS v1" in include/dvg.h): the per-chain-field draw on
// the beta table of the AIS draw, with the field's STRENGTH looked up per sweep as well -- row_k = clamp(rn(prefactor *
// rn(linear + rn(lambda_k * field)))) -- and the AIS draw's two accumulators, which also take the energy step of the row's
// change at the head of a sweep.  An eighth mode of SCHED, GIBBS_FIELD_WEIGH: the AIS block plus the rows and the strengths.
// The kernels treat it as GIBBS_FIELD where a spin's hs is read (`FIELD`) and as GIBBS_WEIGH at the head and the end (`AIS`);
// `FWEIGH` adds the row step alone.  R chains share a row of `fields` (chain c reads row c / R).
struct GibbsFieldAisArgs : GibbsAisArgs {
  const float* fields;    // [ceil(n_chains / R) or 1][n]
  int64_t field_stride;   // n or 0
  int row_chains;         // R >= 1
  const float* scales;    // [n_chains or 1][n_sweeps]: lambda of sweep k of the call; null: 1 throughout (the row never changes)
  int64_t scale_stride;   // n_sweeps or 0
  float scale_from;       // lambda_{-1}: the strength the start states are a sample under (scales == null: 1)
};
constexpr int GIBBS_TABLE = 1, GIBBS_WEIGH = 2, GIBBS_EXCHANGE = 3, GIBBS_TRACE = 4, GIBBS_EXCHANGE_TRACE = 5, GIBBS_FIELD = 6,
              GIBBS_FIELD_WEIGH = 7;
template <bool HELD, int SCHED = 0>
using GibbsArgsT = std::conditional_t<
    SCHED == GIBBS_FIELD_WEIGH, GibbsFieldAisArgs,
    std::conditional_t<
    SCHED == GIBBS_FIELD, GibbsFieldArgs,
    std::conditional_t<
        SCHED == GIBBS_EXCHANGE_TRACE, GibbsExchangeTraceArgs,
        std::conditional_t<
            SCHED == GIBBS_TRACE, GibbsTraceArgs,
            std::conditional_t<SCHED == GIBBS_EXCHANGE, GibbsExchangeArgs,
                               std::conditional_t<SCHED == GIBBS_WEIGH, GibbsAisArgs,
                                                  std::conditional_t<SCHED == GIBBS_TABLE, GibbsSchedArgs,
                                                                     std::conditional_t<HELD, GibbsHeldArgs, GibbsArgs>>>>>>>>;

// A chain's start state, its LPC lanes each taking spins l, l + LPC, ...: from the INIT stream (init) or from `state`.
// HELD (a conditional draw): held spins from `state` always, free ones as above.
template <int LPC, bool HELD, typename Args>
__device__ __forceinline__ void gibbs_load_chain(const Args& a, _Float16* st, int chain, int l, uint32_t cid, uint32_t sweep0) {
  const int n = a.n;
  if constexpr (HELD) {
    const int8_t* src = a.state + (size_t)chain * n;
    const uint8_t* held = a.clamp + (int64_t)chain * a.clamp_stride;
    for (int i = l; i < n; i += LPC) {
      if (a.init && held[i] == 0) {
        u32x4 r = philox4x32_10((uint32_t)i, cid, sweep0, STREAM_INIT, a.k0, a.k1);
        st[i] = (r.x >> 31) ? (_Float16)1.0f : (_Float16)-1.0f;
      } else {
        st[i] = (_Float16)(float)src[i];
      }
    }
  } else if (a.init) {
    for (int i = l; i < n; i += LPC) {
      u32x4 r = philox4x32_10((uint32_t)i, cid, sweep0, STREAM_INIT, a.k0, a.k1);
      st[i] = (r.x >> 31) ? (_Float16)1.0f : (_Float16)-1.0f;
    }
  } else {
    const int8_t* src = a.state + (size_t)chain * n;
    for (int i = l; i < n; i += LPC) st[i] = (_Float16)(float)src[i];
  }
}
__device__ __forceinline__ float clampf(float v, float lo, float hi) { return fminf(fmaxf(v, lo), hi); }

// ---------------------------------------------------------------- the LDS image and the neighbour sum (round 4)
// The local field of a spin is  f = h_i + sum over its CSR row, IN ROW ORDER, of (s_j > 0 ? +J : -J)  in float32, each add
// rounded (oracle/gibbs.py, "DVG block-Gibbs v1").  Rounds 1-3 spent ~12 VALU and 3.4 LDS instructions per neighbour on it
// (index clamping, three address computations, compare / select / add); this form spends 3 and 1.5, for the same bits:
//   * the state of a chain is kept as float16 +-1 in LDS, and the add is ONE v_fma_mix_f32:  fma(s, J, f) = rn(s J + f)
//     with s J = +-J exact, i.e. exactly rn(f +- J) -- the same single rounding as the add it replaces;
//   * rows are padded to whole batches of 4 entries (J = 0, any valid state: rn(f +- 0) = f; only the LAST partial sum
//     can see a pad, and a -0 turned +0 there is the same exp(0)), so a batch is one ds_read_b128 of couplings and one
//     ds_read_b64 of four 16-bit state offsets at immediate offsets from one address -- no per-neighbour index math;
//   * every lane walks the same NB batches per round (NB = 5: 20 neighbours, the degree of the Zephyr graphs); a lane
//     whose row is shorter reads the image's all-zero batch instead (one compare / select per BATCH), so the loads of a
//     round are one straight line: 2 NB reads, then 4 NB state reads, then 4 NB dependent fmas.
typedef float gf32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t gu32x2 __attribute__((ext_vector_type(2)));

struct GibbsLds {
  float* hs;         // [n]  clamped prefactor * h
  float* w;          // [4 (n_batches + 1)]  clamped prefactor * J per padded entry; the last batch is the zero batch
  uint32_t* row;     // [n]  (first batch << 8) | batches
  int32_t* cls;      // [n_colours + 1]
  uint16_t* off;     // [4 (n_batches + 1)]  byte offset of the neighbour's state inside a chain's state row
  uint16_t* order;   // [n]
  _Float16* state;   // [chains][n_pad]
};
// (gibbs_lds_layout: gibbs_plan.h)
__device__ __forceinline__ GibbsLds gibbs_carve(unsigned char* smem, int n, int n_batches, int n_colours) {
  size_t o[7];
  gibbs_lds_layout(n, n_batches, n_colours, o);
  GibbsLds L;
  L.hs = reinterpret_cast<float*>(smem + o[0]);
  L.w = reinterpret_cast<float*>(smem + o[1]);
  L.row = reinterpret_cast<uint32_t*>(smem + o[2]);
  L.cls = reinterpret_cast<int32_t*>(smem + o[3]);
  L.off = reinterpret_cast<uint16_t*>(smem + o[4]);
  L.order = reinterpret_cast<uint16_t*>(smem + o[5]);
  L.state = reinterpret_cast<_Float16*>(smem + o[6]);
  return L;
}

// stage the graph (coalesced reads of h, J and the padded-row image), all threads of the workgroup; ends with a barrier
template <int NT, int OFF_SCALE = 2>  // OFF_SCALE: bytes between two spins of a chain's state (2: a row per chain; 32: [spin][16 chains])
__device__ __forceinline__ void gibbs_stage(const GibbsArgs& a, const GibbsLds& L, int tid) {
  const int n = a.n;
  for (int i = tid; i < n; i += NT) {
    L.hs[i] = clampf(__fmul_rn(a.prefactor, a.linear[i]), a.h_lo, a.h_hi);
    L.order[i] = (uint16_t)a.order[i];
    L.row[i] = (uint32_t)a.adj_row[i];
  }
  const int n_ent = 4 * a.n_batches;
  for (int q = tid; q < n_ent + 4; q += NT) {
    const int src = q < n_ent ? a.adj_src4[q] : -1;
    L.w[q] = src >= 0 ? clampf(__fmul_rn(a.prefactor, a.quadratic[a.adj_eid[src]]), a.j_lo, a.j_hi) : 0.0f;
    L.off[q] = src >= 0 ? (uint16_t)(OFF_SCALE * a.adj_idx[src]) : (uint16_t)0;
  }
  for (int i = tid; i <= a.n_colours; i += NT) L.cls[i] = a.class_ptr[i];
  __syncthreads();
}

__device__ __forceinline__ float gibbs_signed_add(_Float16 s, float w, float f) {
  // rn(s w + f), s = +-1: v_fma_mix_f32 with a float16 first operand
  return __builtin_fmaf((float)s, w, f);
}

// f + (the row's signed couplings, in row order); max_batches is uniform (the graph's longest row).  `st`: the chain's
// state -- its row, or with the state stored [spin][chains] (gibbs_slot_kernel, which stages the offsets as 2 x chains x
// spin) the lane's chain column.
// (FIX: the image holds exactly GIBBS_NB batches per spin, spin i's at GIBBS_NB i -- rowinfo = that index; no per-batch select)
template <bool FIX = false>
__device__ __forceinline__ float gibbs_field(float f, uint32_t rowinfo, const GibbsLds& L, const void* st, int zero_batch,
                                             int max_batches) {
  const int first = FIX ? (int)rowinfo : (int)(rowinfo >> 8), nb = FIX ? GIBBS_NB : (int)(rowinfo & 255u);
  const unsigned char* stb = reinterpret_cast<const unsigned char*>(st);
  for (int b0 = 0; b0 < (FIX ? GIBBS_NB : max_batches); b0 += GIBBS_NB) {
    gf32x4 w[GIBBS_NB];
    gu32x2 o[GIBBS_NB];
#pragma unroll
    for (int j = 0; j < GIBBS_NB; ++j) {
      const int bi = (FIX || b0 + j < nb) ? first + b0 + j : zero_batch;
      w[j] = *reinterpret_cast<const gf32x4*>(L.w + 4 * bi);
      o[j] = *reinterpret_cast<const gu32x2*>(L.off + 4 * bi);
    }
    _Float16 h[GIBBS_NB][4];
#pragma unroll
    for (int j = 0; j < GIBBS_NB; ++j) {
      h[j][0] = *reinterpret_cast<const _Float16*>(stb + (o[j][0] & 0xffffu));
      h[j][1] = *reinterpret_cast<const _Float16*>(stb + (o[j][0] >> 16));
      h[j][2] = *reinterpret_cast<const _Float16*>(stb + (o[j][1] & 0xffffu));
      h[j][3] = *reinterpret_cast<const _Float16*>(stb + (o[j][1] >> 16));
    }
#pragma unroll
    for (int j = 0; j < GIBBS_NB; ++j) {
      f = gibbs_signed_add(h[j][0], w[j][0], f);
      f = gibbs_signed_add(h[j][1], w[j][1], f);
      f = gibbs_signed_add(h[j][2], w[j][2], f);
      f = gibbs_signed_add(h[j][3], w[j][3], f);
    }
  }
  return f;
}

__device__ __forceinline__ _Float16 gibbs_decide(float f, float two_beta, uint32_t word) {
  const float z = clampf(__fmul_rn(two_beta, f), -87.0f, 87.0f);
  const float tt = spec_exp(z);
  const float b = __fmul_rn(u32_to_unit(word), __fadd_rn(1.0f, tt));
  return (b < 1.0f) ? (_Float16)1.0f : (_Float16)-1.0f;
}

// AIS: one spin's addend of the start energy, 1/2 s (hs + f) -- exact in float64
__device__ __forceinline__ double gibbs_start_energy(_Float16 s, float hs, float f) {
  return 0.5 * (double)(float)s * ((double)hs + (double)f);
}
// AIS: the energy change of an update decided on the field f, (s_new - s_old) f = +-2 f or 0 -- exact in float32
__device__ __forceinline__ double gibbs_energy_step(float s_new, float s_old, float f) {
  return (double)__fmul_rn(__fsub_rn(s_new, s_old), f);
}
// AIS: sum of a chain's LPC lane shares, in every lane of the chain (its lanes are active together)
template <int LPC>
__device__ __forceinline__ double gibbs_chain_sum(double v) {
#pragma unroll
  for (int m = LPC / 2; m >= 1; m >>= 1) v += __shfl_xor(v, m, LPC);
  return v;
}

// ---------------------------------------------------------------- the exchange step (GIBBS_EXCHANGE)
// Which chain a workgroup's chain slot s = wave CPW + sub works on.  The other draws: chain b SLOTS + s in workgroup b,
// SLOTS = WAVES CPW.  The exchange draw: a workgroup holds SLOTS / R whole ladders, slot s = (ladder lq of the workgroup,
// replica j); the SLOTS % R slots behind the last ladder idle, as do the slots of ladders beyond the draw's.
struct GibbsSlot { int chain; bool valid; int lq, j; };
template <bool EXCH, int WAVES, int CPW, typename Args>
__device__ __forceinline__ GibbsSlot gibbs_slot(const Args& a, int wave, int sub) {
  GibbsSlot r{};
  if constexpr (EXCH) {
    constexpr int SLOTS = WAVES * CPW;
    const int s = wave * CPW + sub;
    const int R = a.n_replicas, per_block = SLOTS / R;
    r.lq = s / R; r.j = s - r.lq * R;
    const int q = (int)blockIdx.x * per_block + r.lq;
    r.chain = q * R + r.j;
    r.valid = r.lq < per_block && r.chain < a.n_chains;  // (n_chains is a multiple of R: whole ladders)
  } else {
    r.chain = (blockIdx.x * WAVES + wave) * CPW + sub;
    r.valid = r.chain < a.n_chains;
  }
  return r;
}
struct GibbsExchangeLds { double* mail; uint32_t* acc; float* ladder; };
__device__ __forceinline__ GibbsExchangeLds gibbs_exchange_carve(unsigned char* smem, size_t form_bytes, int slots) {
  size_t o[3];
  gibbs_exchange_lds_layout(form_bytes, slots, o);
  return {reinterpret_cast<double*>(smem + o[0]), reinterpret_cast<uint32_t*>(smem + o[1]), reinterpret_cast<float*>(smem + o[2])};
}
// before the workgroup's first barrier: counters to zero, the ladder into LDS
template <int NT, int SLOTS>
__device__ __forceinline__ void gibbs_exchange_stage(const GibbsExchangeArgs& a, const GibbsExchangeLds& X, int tid) {
  for (int i = tid; i < SLOTS; i += NT) X.acc[i] = 0u;
  for (int i = tid; i < GIBBS_MAX_REPLICAS; i += NT) X.ladder[i] = i < a.n_replicas ? a.ladder[i] : 0.0f;
}
// Exchange number x, first half: the chain's energy (the sum of its lanes' shares) into mailbox x & 1 at (ladder, rung).  All
// lanes of a valid chain call it together; a WORKGROUP BARRIER follows, reached by every wave of the workgroup.
template <int LPC, int SLOTS>
__device__ __forceinline__ void gibbs_exchange_post(const GibbsExchangeLds& X, int R, uint32_t x, int lq, int rung, int l, double e) {
  const double E = gibbs_chain_sum<LPC>(e);
  if (l == 0) X.mail[(x & 1u) * SLOTS + lq * R + rung] = E;
}
// ... second half, behind the barrier: the chain whose rung belongs to a pair (r, r + 1) of this exchange's parity reads both
// energies and decides -- its partner evaluates the same expression on the same operands and decides the same.  Mailbox x & 1
// is written again at exchange x + 2, behind barrier x + 1, which no wave passes before every reader of x has arrived.
__device__ __forceinline__ void gibbs_exchange_decide(const GibbsExchangeArgs& a, const GibbsExchangeLds& X, int slots, int R, uint32_t x,
                                                      int lq, uint32_t ladder_id, int l, int& rung, float& beta) {
  const int par = (int)(x & 1u);
  const bool lower = (rung & 1) == par && rung + 1 < R, upper = (rung & 1) != par && rung >= 1;
  if (!(lower || upper)) return;
  const int r = lower ? rung : rung - 1;
  const double* m = X.mail + (x & 1u) * slots + lq * R;
  const double ea = m[r], eb = m[r + 1];
  const double db = (double)X.ladder[r + 1] - (double)X.ladder[r], de = eb - ea;
  const double d = db * de;
  const u32x4 w = philox4x32_10((uint32_t)r, ladder_id, x, STREAM_SWAP, a.k0, a.k1);
  const bool accept = d >= 0.0 || (double)u32_to_unit(w.x) < exp(d);
  if (accept) {
    rung = lower ? r + 1 : r;
    beta = X.ladder[rung];
    if (lower && l == 0) X.acc[lq * R + r] += 1u;  // (this pair's only writer)
  }
}

// ---------------------------------------------------------------- the record step (GIBBS_TRACE)
// A chain's state row is n_pad = (n + 15) & ~15 float16 of +-1: the information is the sign bit.  Lane l of the chain's LPC
// builds words l, l + LPC, ... < W = (n + 31) / 32 of the record: word w from halfwords 32 w .. 32 w + 31 of the row, four
// 128-bit LDS reads of 8 halfwords each.  A read that would start at or behind n_pad reads the row's LAST 8 halfwords instead
// (n_pad is a multiple of 8, so a read is inside the row or outside it as a whole; the address is clamped, not the read
// predicated: the four reads of a word are issued back to back and waited for once): the last word of a graph with
// n_pad % 32 == 16 ends in mid-word, with the next chain's row, the sinks or the held flags behind it, and nothing behind the
// row is read.  Bits of spins >= n (the row's own pad, whatever it holds, and the clamped reads) are forced to 0.  The sign
// bits of a read's four dwords (bits 15 and 31 of each) are gathered side by side, not one by one into one accumulator:
// shallow dependency chains -- at one wave per SIMD nothing else hides them (the first form, 32 dependent shift-ors behind
// predicated reads, cost 0.35 us per record; profiles/gibbs_trace.txt).  The stores: consecutive lanes, consecutive words.
// Called behind the last class's fence of a sweep by the lanes that wrote the row -- one wave in every form: no workgroup
// barrier.
// A16: the rows are 16-byte aligned (the lane-major image; the padded-row image of the rolled form aligns them to 4 only, and
// the compiler splits the read as the target needs).
typedef uint32_t gu32x4 __attribute__((ext_vector_type(4)));
typedef gu32x4 gu32x4_a4 __attribute__((aligned(4)));
template <int LPC, bool A16>
__device__ __forceinline__ void gibbs_record(const _Float16* st, int n, int n_pad, int l, uint32_t* rec) {
  const int W = (n + 31) >> 5;
  for (int w = l; w < W; w += LPC) {
    uint32_t u[4];  // per read: the signs of halfwords 0, 2, 4, 6 at bits 0, 2, 4, 6 and of 1, 3, 5, 7 at bits 16, 18, 20, 22
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int h0 = min(32 * w + 8 * q, n_pad - 8);
      gu32x4 v;
      if constexpr (A16) v = *reinterpret_cast<const gu32x4*>(st + h0);
      else v = *reinterpret_cast<const gu32x4_a4*>(st + h0);
      u[q] = ((v[0] >> 15) & 0x00010001u) | (((v[1] >> 15) & 0x00010001u) << 2) | (((v[2] >> 15) & 0x00010001u) << 4) |
             (((v[3] >> 15) & 0x00010001u) << 6);
    }
    const uint32_t a = u[0] | (u[1] << 8), b = u[2] | (u[3] << 8);  // 16 halfwords each: even ones at bits 0..14, odd at 16..30
    // bit b: halfword 32 w + b has its sign bit set
    const uint32_t minus = ((a | (a >> 15)) & 0xffffu) | (((b | (b >> 15)) & 0xffffu) << 16);
    const int left = n - 32 * w;  // (>= 1)
    rec[w] = ~minus & (left >= 32 ? 0xffffffffu : (1u << left) - 1u);
  }
}

// The record step of GIBBS_EXCHANGE_TRACE, behind the exchange block of a recorded sweep: the lanes of a VALID chain, together.
// `row` = q R + (the rung the chain holds now), `m` the record.  The chain's own LDS row and registers only: no workgroup
// barrier, no LDS of its own.  The energy is the sum of a COPY of the lanes' shares: `e` itself goes on as it was, so the draw's
// later sums (the next exchange's, energy_out's) add the same shares in the same order as the draw without records.
template <int LPC, bool A16>
__device__ __forceinline__ void gibbs_exchange_record(const GibbsExchangeTraceArgs& a, const _Float16* st, int n, int n_pad, int l,
                                                      int chain, size_t row, uint32_t m, int rung, double e) {
  const size_t M = (size_t)a.n_records;
  gibbs_record<LPC, A16>(st, n, n_pad, l, a.trace + (row * M + m) * gibbs_held_words(n));
  if (a.energy_trace) {  // (a kernel argument: uniform)
    const double E = gibbs_chain_sum<LPC>(e);
    if (l == 0) a.energy_trace[row * M + m] = E;
  }
  if (a.rung_trace && l == 0) a.rung_trace[(size_t)chain * M + m] = (uint8_t)rung;
}

// ---------------------------------------------------------------- the sweep loop's control (gibbs_kernel, gibbs_fast_kernel)
// What a draw mode does around the neighbour sums is the same in both chain-per-lanes kernels and is written here once; the
// kernels keep the field code, its schedule and the start-energy walk.  The modes of SCHED:
//   0: the plain draw (and, HELD, the conditional one) at the fixed beta of the argument block.
//   GIBBS_TABLE: the annealed draw -- a lane reads its chain's beta of a sweep one sweep ahead (one load per sweep and lane;
//     with the shared row every lane of a wave reads one address, with a row per chain the LPC lanes of a chain).
//   GIBBS_WEIGH: the AIS draw -- the table, and a lane keeps its share `e` of the chain's energy (the start addends of its
//     spins, then every update it makes) and its share `lw` of the log weight; lane 0 of the chain stores the sums.
//   GIBBS_EXCHANGE: the energy share as above, beta the ladder's entry of the rung the chain holds; at an exchange the
//     workgroup meets at a barrier (gibbs_exchange_post / _decide).  The exchanges are counted from (sweep0, swap_every) alone.
//   GIBBS_TRACE: the plain draw; behind a recorded sweep's last fence the chain's lanes pack its row (gibbs_record).  Which
//     sweeps: a countdown in scalar registers (`rec_at`, the next recorded k + 1), no division per sweep.
//   GIBBS_EXCHANGE_TRACE: the exchange draw (EXCH); behind the exchange block of a recorded sweep the lanes of a valid chain
//     write its record to the row of the rung it NOW holds (gibbs_exchange_record), on the same countdown.
//   GIBBS_FIELD: the plain draw's control -- the fixed beta, nothing at the head or the tail of a sweep; what differs is where
//     the rolled kernel reads a spin's hs (FIELD: the chain's own row).  The lane-major kernel has no such instantiation.
//   GIBBS_FIELD_WEIGH: the AIS draw's control on the field draw's rows (FIELD and AIS both hold).  With a table of strengths
//     (FWEIGH and a.scales) the rolled kernel rewrites the chain's row before the head of a sweep (gibbs_field_step) and leaves
//     the lane's share of the energy step in `d`; the head weighs it.  A lane reads its chain's strength a sweep ahead, as beta.
// What the exchange modes rest on, in either kernel:
//   * EVERY wave of a workgroup reaches EVERY barrier: the ones in gibbs_sweep_tail and the one in gibbs_finish.  The kernels
//     let no wave leave or skip the sweep loop under EXCH -- the lanes of an idle slot run it without a spin to update;
//   * idle slots count the records down as the others do and record nothing;
//   * the traced exchange draw sums `e` from a COPY (gibbs_exchange_record): the shares go on as in the draw without records.
template <int SCHED>
struct GibbsMode {
  static constexpr bool FWEIGH = SCHED == GIBBS_FIELD_WEIGH;
  static constexpr bool AIS = SCHED == GIBBS_WEIGH || FWEIGH, XTRACE = SCHED == GIBBS_EXCHANGE_TRACE;
  static constexpr bool EXCH = SCHED == GIBBS_EXCHANGE || XTRACE, ENERGY = AIS || EXCH;
  static constexpr bool TABLE = SCHED == GIBBS_TABLE || AIS, TRACE = SCHED == GIBBS_TRACE;
  static constexpr bool FIELD = SCHED == GIBBS_FIELD || FWEIGH;
};
// a lane's control registers; a mode leaves those of the others at zero and the compiler drops them
struct GibbsControl {
  const float* bt;        // TABLE: this chain's row of the table
  float beta_next;        // TABLE: the entry of the coming sweep, read a sweep ahead of its first use; EXCH: the rung's beta
  float beta_prev;        // AIS: the beta of the sweep before (first: beta_from)
  int rung;               // EXCH: the rung the chain holds
  double e, lw;           // ENERGY, AIS: the lane's shares of the chain's energy and log weight
  const float* sc;        // FWEIGH: this chain's row of the table of strengths; null: none
  float lam_next;         // FWEIGH: the strength of the coming sweep, read a sweep ahead
  double d;               // FWEIGH: the lane's share of d_k, the energy step of the row's change at the head of the coming sweep
  uint32_t rec_at, rec_m;  // TRACE, XTRACE: the next recorded sweep (as k + 1) and its record
};
// before the first sweep (and the start-energy walk): the lanes of a valid chain or, EXCH, of any slot
template <int SCHED, typename Args>
__device__ __forceinline__ GibbsControl gibbs_begin(const Args& a, const GibbsExchangeLds& X, const GibbsSlot& slot) {
  using M = GibbsMode<SCHED>;
  GibbsControl c{};
  if constexpr (M::EXCH) {
    if (slot.valid) c.rung = a.init ? slot.j : min(max(a.rung[slot.chain], 0), a.n_replicas - 1);
    c.beta_next = X.ladder[c.rung];
  } else if constexpr (M::TABLE) {
    c.bt = a.betas + (int64_t)slot.chain * a.beta_stride;
    c.beta_next = c.bt[0];
  }
  if constexpr (M::AIS) c.beta_prev = a.beta_from;
  if constexpr (M::FWEIGH) {
    if (a.scales) {  // (a kernel argument: uniform)
      c.sc = a.scales + (int64_t)slot.chain * a.scale_stride;
      c.lam_next = c.sc[0];
    }
  }
  if constexpr (M::TRACE || M::XTRACE) c.rec_at = (uint32_t)a.burn_in + (uint32_t)a.thin;
  return c;
}
// head of sweep t: its two_beta; AIS: the weight step on the energy before the sweep
template <int SCHED, typename Args>
__device__ __forceinline__ float gibbs_sweep_head(const Args& a, uint32_t t, uint32_t sweep0, GibbsControl& c) {
  using M = GibbsMode<SCHED>;
  if constexpr (M::EXCH) {
    return __fmul_rn(2.0f, c.beta_next);
  } else if constexpr (M::TABLE) {
    const float two_beta = __fmul_rn(2.0f, c.beta_next);
    if constexpr (M::AIS) {
      c.lw -= ((double)c.beta_next - (double)c.beta_prev) * c.e;
      if constexpr (M::FWEIGH) {  // (d: what gibbs_field_step left; without a table of strengths it stays 0)
        c.lw -= (double)c.beta_next * c.d;
        c.e += c.d;
      }
      c.beta_prev = c.beta_next;
    }
    const uint32_t kn = t - sweep0 + 1u;
    if (kn < (uint32_t)a.n_sweeps) c.beta_next = c.bt[kn];
    if constexpr (M::FWEIGH) {
      if (c.sc && kn < (uint32_t)a.n_sweeps) c.lam_next = c.sc[kn];
    }
    return two_beta;
  } else {
    return a.two_beta;
  }
}
// tail of sweep t, behind its last class's fence.  `st`: the chain's row, `l` the lane's index in the chain; A16: gibbs_record's.
template <int LPC, int SLOTS, int SCHED, bool A16, typename Args>
__device__ __forceinline__ void gibbs_sweep_tail(const Args& a, const GibbsExchangeLds& X, const GibbsSlot& slot, const _Float16* st,
                                                 int l, uint32_t t, uint32_t sweep0, GibbsControl& c) {
  using M = GibbsMode<SCHED>;
  const int n = a.n, n_pad = (n + 15) & ~15;
  if constexpr (M::TRACE) {  // (every lane here is a valid chain's)
    if (t - sweep0 + 1u == c.rec_at && c.rec_m < (uint32_t)a.n_records) {
      gibbs_record<LPC, A16>(st, n, n_pad, l, a.trace + ((size_t)slot.chain * a.n_records + c.rec_m) * gibbs_held_words(n));
      c.rec_at += (uint32_t)a.thin;
      ++c.rec_m;
    }
  }
  if constexpr (M::EXCH) {
    // (t, swap_every: kernel arguments -- the same in every wave of every workgroup)
    if ((t + 1u) % (uint32_t)a.swap_every == 0u) {
      const uint32_t x = (t + 1u) / (uint32_t)a.swap_every;
      if (slot.valid) gibbs_exchange_post<LPC, SLOTS>(X, a.n_replicas, x, slot.lq, c.rung, l, c.e);
      __syncthreads();
      if (slot.valid)
        gibbs_exchange_decide(a, X, SLOTS, a.n_replicas, x, slot.lq, a.chain_id0 + (uint32_t)(slot.chain - slot.j), l, c.rung,
                              c.beta_next);
    }
  }
  if constexpr (M::XTRACE) {
    if (t - sweep0 + 1u == c.rec_at && c.rec_m < (uint32_t)a.n_records) {
      if (slot.valid)
        gibbs_exchange_record<LPC, A16>(a, st, n, n_pad, l, slot.chain, (size_t)(slot.chain - slot.j + c.rung), c.rec_m, c.rung, c.e);
      c.rec_at += (uint32_t)a.thin;
      ++c.rec_m;
    }
  }
}
// the way out, behind the last sweep: state (and EXCH: rung) by chain; samples, energies and counters by chain or, EXCH, by rung
template <int LPC, int SCHED, typename Args>
__device__ __forceinline__ void gibbs_finish(const Args& a, const GibbsExchangeLds& X, const GibbsSlot& slot, const _Float16* st, int l,
                                             const GibbsControl& c) {
  using M = GibbsMode<SCHED>;
  const int n = a.n, chain = slot.chain;
  size_t row = (size_t)chain;
  if constexpr (M::EXCH) {
    __syncthreads();  // the counters are final
    if (!slot.valid) return;
    row = (size_t)(chain - slot.j + c.rung);
  }
  int8_t* dst = a.state + (size_t)chain * n;
  for (int i = l; i < n; i += LPC) {
    const float v = (float)st[i];
    dst[i] = (int8_t)v;
    if (a.samples_out) a.samples_out[row * n + i] = v;
  }
  if constexpr (M::EXCH) {
    const double e = gibbs_chain_sum<LPC>(c.e);
    if (l == 0) {
      a.rung[chain] = c.rung;
      if (a.energy_out) a.energy_out[row] = e;
      if (a.accept_out) a.accept_out[chain] = X.acc[slot.lq * a.n_replicas + slot.j];
    }
  } else if constexpr (M::AIS) {
    const double e = gibbs_chain_sum<LPC>(c.e), lw = gibbs_chain_sum<LPC>(c.lw);
    if (l == 0) {
      if (!M::FWEIGH || a.log_weight_out) a.log_weight_out[chain] = lw;  // (the field kind alone may go unweighed)
      if (a.energy_out) a.energy_out[chain] = e;
    }
  }
}

// ---------------------------------------------------------------- a chain's row of hs (GIBBS_FIELD, GIBBS_FIELD_WEIGH)
// the chain's row of `fields`, and the strength its start states were drawn under
template <int SCHED, typename Args>
__device__ __forceinline__ const float* gibbs_field_row(const Args& a, int chain) {
  if constexpr (GibbsMode<SCHED>::FWEIGH) return a.fields + (int64_t)(chain / a.row_chains) * a.field_stride;
  else return a.fields + (int64_t)chain * a.field_stride;
}
// entry i of the row at strength lam: clamp(rn(prefactor * rn(linear + rn(lam * field)))); the field kind has no strength (1: the
// product is the field itself, bit for bit)
template <int SCHED, typename Args>
__device__ __forceinline__ float gibbs_field_entry(const Args& a, const float* fr, int i, float lam) {
  const float fi = GibbsMode<SCHED>::FWEIGH ? __fmul_rn(lam, fr[i]) : fr[i];
  return clampf(__fmul_rn(a.prefactor, __fadd_rn(a.linear[i], fi)), a.h_lo, a.h_hi);
}
// FWEIGH with a table of strengths, before the head of a sweep: the lanes that own the row's entries (i = l, l + LPC, ...: as at
// load) recompute them at the sweep's strength from `linear` and the chain's row of `fields` (global memory: L2 serves them),
// rewrite them in place and return their share of  d_k = sum_i (row_k[i] - row_{k-1}[i]) s_i  (each addend exact in float64).
// The caller fences behind it: a spin is not updated by the lane that owns its row entry.
template <int LPC, int SCHED, typename Args>
__device__ __forceinline__ double gibbs_field_step(const Args& a, const float* fr, float* hc, const _Float16* st, int l, float lam) {
  double d = 0.0;
  for (int i = l; i < a.n; i += LPC) {
    const float now = gibbs_field_entry<SCHED>(a, fr, i, lam);
    d += ((double)now - (double)hc[i]) * (double)(float)st[i];
    hc[i] = now;
  }
  return d;
}

// LPC = lanes per chain (16, 32 or 64); WAVES waves per workgroup.  The rolled schedule: any graph; Philox per update.
// HELD: the chain's held flags sit behind the state rows, one bit per spin, and a held spin is passed over in its class.
// EXCH: the lanes of an idle slot find every class empty.  The rows are aligned to 4 bytes (gibbs_record's A16 = false).
// FIELD: the chain's row of hs = clamp(rn(prefactor * rn(linear + field))) sits behind the state rows, float32 [n_pad] per chain
// slot, written once when the chain is loaded by the lanes that read it (one wave: the fence below orders it); every read of
// the image's shared hs goes to it instead.  FWEIGH with a table of strengths: the same lanes rewrite the row at the head of
// every sweep (gibbs_field_step), and one more fence stands before the first class.
template <int LPC, int WAVES, bool HELD = false, int SCHED = 0>
__global__ __launch_bounds__(WAVES * 64) void gibbs_kernel(GibbsArgsT<HELD, SCHED> a) {
  static_assert(!(HELD && SCHED), "no annealed conditional draw");
  using M = GibbsMode<SCHED>;
  constexpr bool EXCH = M::EXCH;
  extern __shared__ __align__(16) unsigned char smem[];
  const int n = a.n;
  const GibbsLds L = gibbs_carve(smem, n, a.n_batches, a.n_colours);
  const int n_pad = (n + 15) & ~15;
  const int tid = threadIdx.x;
  constexpr int CPW = 64 / LPC;  // chains per wave
  [[maybe_unused]] GibbsExchangeLds X{};
  if constexpr (EXCH) {
    X = gibbs_exchange_carve(smem, gibbs_lds_bytes(n, a.n_batches, a.n_colours, WAVES * CPW), WAVES * CPW);
    gibbs_exchange_stage<WAVES * 64, WAVES * CPW>(a, X, tid);
  }
  gibbs_stage<WAVES * 64>(a, L, tid);

  const int wave = tid >> 6, lane = tid & 63;
  const int sub = lane / LPC, l = lane % LPC;
  const GibbsSlot slot = gibbs_slot<EXCH, WAVES, CPW>(a, wave, sub);
  const int chain = slot.chain;
  const bool valid = slot.valid;
  _Float16* st = L.state + (size_t)(wave * CPW + sub) * n_pad;
  const uint32_t cid = a.chain_id0 + (uint32_t)chain;
  // HELD: bit (i & 31) of word (i >> 5) of the chain's row of flags
  [[maybe_unused]] uint32_t* hb = nullptr;
  if constexpr (HELD)
    hb = reinterpret_cast<uint32_t*>(L.state + (size_t)WAVES * CPW * n_pad) + (size_t)(wave * CPW + sub) * gibbs_held_words(n);
  // where a spin's hs is read: the image's row, or (FIELD) the chain's own
  const float* hsv = L.hs;
  [[maybe_unused]] float* hc = nullptr;
  if constexpr (M::FIELD) {
    hc = reinterpret_cast<float*>(L.state + (size_t)WAVES * CPW * n_pad) + (size_t)(wave * CPW + sub) * n_pad;
    hsv = hc;
  }

  // (read before the chains start: a fresh chain's start configuration is keyed by the sweep index it starts at, so
  // non-persistent draws do not all restart from one configuration)
  const uint32_t sweep0 = a.sweep0_dev ? *a.sweep0_dev : a.sweep0;
  if (valid) {
    gibbs_load_chain<LPC, HELD>(a, st, chain, l, cid, sweep0);
    if constexpr (HELD) {
      // (a lane packs whole words: 32 consecutive flags each)
      const uint8_t* held = a.clamp + (int64_t)chain * a.clamp_stride;
      for (int w = l; w < gibbs_held_words(n); w += LPC) {
        uint32_t bits = 0u;
        for (int b = 0; b < 32 && 32 * w + b < n; ++b) bits |= (held[32 * w + b] != 0 ? 1u : 0u) << b;
        hb[w] = bits;
      }
    }
    if constexpr (M::FIELD) {
      const float* fr = gibbs_field_row<SCHED>(a, chain);
      float lam = 1.0f;
      if constexpr (M::FWEIGH) lam = a.scales ? a.scale_from : 1.0f;
      for (int i = l; i < n; i += LPC) hc[i] = gibbs_field_entry<SCHED>(a, fr, i, lam);
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
  __builtin_amdgcn_wave_barrier();

  if (valid || EXCH) {
    GibbsControl ctl = gibbs_begin<SCHED>(a, X, slot);
    if constexpr (M::ENERGY) {
      for (int i = l; i < (valid ? n : 0); i += LPC) {
        const float hsi = hsv[i];
        ctl.e += gibbs_start_energy(st[i], hsi, gibbs_field(hsi, L.row[i], L, st, a.n_batches, a.max_batches));
      }
    }
    for (uint32_t t = sweep0; t < sweep0 + (uint32_t)a.n_sweeps; ++t) {
      const uint32_t tq = t >> 2, tw = t & 3u;
      if constexpr (M::FWEIGH) {
        if (a.scales) {  // (a kernel argument: uniform)
          ctl.d = gibbs_field_step<LPC, SCHED>(a, gibbs_field_row<SCHED>(a, chain), hc, st, l, ctl.lam_next);
          __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
          __builtin_amdgcn_wave_barrier();
        }
      }
      const float two_beta = gibbs_sweep_head<SCHED>(a, t, sweep0, ctl);
      for (int k = 0; k < a.n_colours; ++k) {
        const int lo = L.cls[k], hi = (EXCH && !valid) ? lo : L.cls[k + 1];  // (an idle slot: every class empty)
        for (int p = lo + l; p < hi; p += LPC) {
          const int i = L.order[p];
          if constexpr (HELD) {
            if ((hb[i >> 5] >> (i & 31)) & 1u) continue;
          }
          const float f = gibbs_field(hsv[i], L.row[i], L, st, a.n_batches, a.max_batches);
          const u32x4 r = philox4x32_10((uint32_t)i, cid, tq, STREAM_GIBBS, a.k0, a.k1);
          const _Float16 s_new = gibbs_decide(f, two_beta, pick(r, tw));
          if constexpr (M::ENERGY) ctl.e += gibbs_energy_step((float)s_new, (float)st[i], f);
          st[i] = s_new;
        }
        // the next class reads what this one wrote (same wave): order LDS traffic
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
        __builtin_amdgcn_wave_barrier();
      }
      gibbs_sweep_tail<LPC, WAVES * CPW, SCHED, false>(a, X, slot, st, l, t, sweep0, ctl);
    }
    gibbs_finish<LPC, SCHED>(a, X, slot, st, l, ctl);
  }
}

// The rolled schedule with the 16 chains of a workgroup side by side in LDS (round 6), for the large graphs that keep it
// (c5: 1024 spins, one 16-wave workgroup per CU, four waves per SIMD).  Same image, same arithmetic, same order, same random
// stream as gibbs_kernel -- what changes is who does what.  gibbs_kernel gives a wave one chain, its 64 lanes 64 spins of a
// colour class: every neighbour read is a gather of 64 random halfwords of the chain's state row -- ~11 cycles of the CU's
// one LDS pipe per instruction (64 lanes over 64 banks at random: 4-5 deep), 20 per update, 16 waves: the draw is bound by
// bank conflicts, which is why neither a quarter of the Philox calls nor two fewer dependent table reads per update moved
// it (both built and measured this round: 1203 / 1193 against 1207 us), and why the lane-major form on twice the CUs takes
// half the time.  Here a wave's lanes are 4 spins x 16 chains, and the state is stored [spin][chain]: a neighbour read is
// four runs of sixteen consecutive halfwords (8 banks each), the table reads four addresses broadcast to sixteen lanes.
// All 16 waves now work on the same 16 chains, so a colour class ends in a workgroup barrier instead of a wave fence
// (5 per sweep).  A lane's (class, pass) slots are static (the host lists them: GibbsSlots, gibbs_plan.h), the slot loop unrolled.

template <int K, int MAXS, int SB, bool FIX>  // SB: bytes between two spins in the state image (2 x chains per workgroup)
struct GibbsSlotLoop {
  static __device__ __forceinline__ void run(const GibbsArgs& a, const GibbsSlots& sl, const GibbsLds& L, unsigned char* stc,
                                             bool valid, uint32_t cid, uint32_t tq, uint32_t tw, bool fresh,
                                             const uint32_t (&ir)[MAXS], uint32_t (&cy)[MAXS], uint32_t (&cz)[MAXS],
                                             uint32_t (&cw)[MAXS]) {
    if (K >= sl.n) return;
    // (FIX: the descriptor is the spin alone, two slots per register -- the word cache leaves no room for one each)
    const uint32_t desc = FIX ? (ir[K >> 1] >> (16 * (K & 1))) & 0xffffu : ir[K];
    if (valid && desc != (FIX ? 0xffffu : 0xffffffffu)) {
      // (opaque copy: everything derived from the descriptor -- batch indices, table addresses, the state address -- is
      // invariant over the sweeps, and hoisted out of the sweep loop it costs ~12 registers per slot: spills)
      uint32_t irk = desc;
      asm volatile("" : "+v"(irk));
      const int i = FIX ? (int)irk : (int)(irk >> 21);
      const float f = gibbs_field<FIX>(L.hs[i], FIX ? (uint32_t)(GIBBS_NB * i) : (irk & 0x1fffffu), L, stc, a.n_batches, a.max_batches);
      // the four words of a (spin, sweep >> 2) counter serve four sweeps: drawn once, three kept (with the LDS gathers out
      // of the way the kernel is bound by its vector instructions, and a Philox call is 100 of an update's 190)
      uint32_t word;
      if (fresh) {
        const u32x4 r = philox4x32_10((uint32_t)i, cid, tq, STREAM_GIBBS, a.k0, a.k1);
        word = pick(r, tw);
        cy[K] = r.y; cz[K] = r.z; cw[K] = r.w;
      } else {
        word = tw == 1u ? cy[K] : (tw == 2u ? cz[K] : cw[K]);
      }
      *reinterpret_cast<_Float16*>(stc + SB * i) = gibbs_decide(f, a.two_beta, word);
    }
    if ((sl.last_mask >> K) & 1u) __syncthreads();  // the next class reads what this one wrote -- all 16 waves, the same chains
    GibbsSlotLoop<K + 1, MAXS, SB, FIX>::run(a, sl, L, stc, valid, cid, tq, tw, fresh, ir, cy, cz, cw);
  }
};
template <int MAXS, int SB, bool FIX>
struct GibbsSlotLoop<MAXS, MAXS, SB, FIX> {
  static __device__ __forceinline__ void run(const GibbsArgs&, const GibbsSlots&, const GibbsLds&, unsigned char*, bool, uint32_t,
                                             uint32_t, uint32_t, bool, const uint32_t (&)[MAXS], uint32_t (&)[MAXS],
                                             uint32_t (&)[MAXS], uint32_t (&)[MAXS]) {}
};

// CH chains per workgroup (16; 8: the draws of few chains -- twice the workgroups, runs of 4 banks).  FIX: graphs of at most
// 20 neighbours per spin whose image fits with every spin's row padded to five batches (c5's do, with 2 KB to spare): the
// batch tables are then addressed by the spin alone -- 5 compares, 5 selects and 10 address computations less per update.
template <int MAXS, int CH, bool FIX>
__global__ __launch_bounds__(1024) void gibbs_slot_kernel(GibbsArgs a, GibbsSlots sl) {
  extern __shared__ __align__(16) unsigned char smem[];
  constexpr int WAVES = 16, SP = 64 / CH, SB = 2 * CH;  // spins per wave and pass; bytes between two spins of the state image
  const int n = a.n;
  const int tid = threadIdx.x;
  GibbsLds L;
  if constexpr (FIX) {
    size_t o[5];
    gibbs_fix_layout(n, o);
    L.hs = reinterpret_cast<float*>(smem + o[0]);
    L.w = reinterpret_cast<float*>(smem + o[1]);
    L.off = reinterpret_cast<uint16_t*>(smem + o[2]);
    L.order = reinterpret_cast<uint16_t*>(smem + o[3]);
    L.state = reinterpret_cast<_Float16*>(smem + o[4]);
    L.row = nullptr; L.cls = nullptr;
    for (int i = tid; i < n; i += WAVES * 64) {
      L.hs[i] = clampf(__fmul_rn(a.prefactor, a.linear[i]), a.h_lo, a.h_hi);
      L.order[i] = (uint16_t)a.order[i];
    }
    for (int q = tid; q < 20 * n; q += WAVES * 64) {
      const int i = q / 20, e = q - 20 * i;
      const uint32_t ri = (uint32_t)a.adj_row[i];
      const int src = (e >> 2) < (int)(ri & 255u) ? a.adj_src4[4 * (int)(ri >> 8) + e] : -1;
      L.w[q] = src >= 0 ? clampf(__fmul_rn(a.prefactor, a.quadratic[a.adj_eid[src]]), a.j_lo, a.j_hi) : 0.0f;
      L.off[q] = src >= 0 ? (uint16_t)(SB * a.adj_idx[src]) : (uint16_t)0;
    }
    __syncthreads();
  } else {
    L = gibbs_carve(smem, n, a.n_batches, a.n_colours);
    gibbs_stage<WAVES * 64, SB>(a, L, tid);
  }

  const int wave = tid >> 6, lane = tid & 63;
  const int g = lane / CH, c = lane % CH;  // spin of the wave's SP, chain of the workgroup's CH
  const int chain = blockIdx.x * CH + c;
  const bool valid = chain < a.n_chains;
  unsigned char* stc = reinterpret_cast<unsigned char*>(L.state) + 2 * c;  // state[spin][chain]: spin i at stc + SB i
  const uint32_t cid = a.chain_id0 + (uint32_t)chain;
  const uint32_t sweep0 = a.sweep0_dev ? *a.sweep0_dev : a.sweep0;
  if (valid) {
    // (64 (wave, spin-of-four) pairs walk the chain's spins)
    if (a.init) {
      for (int i = wave * SP + g; i < n; i += 16 * SP) {
        u32x4 r = philox4x32_10((uint32_t)i, cid, sweep0, STREAM_INIT, a.k0, a.k1);
        *reinterpret_cast<_Float16*>(stc + SB * i) = (r.x >> 31) ? (_Float16)1.0f : (_Float16)-1.0f;
      }
    } else {
      const int8_t* src = a.state + (size_t)chain * n;
      for (int i = wave * SP + g; i < n; i += 16 * SP) *reinterpret_cast<_Float16*>(stc + SB * i) = (_Float16)(float)src[i];
    }
  }
  // this lane's spin of every slot and its row descriptor (spin << 21 | first batch << 8 | batches), read once (11 bits
  // of spin, 13 of first batch: the launcher checks); words 1..3 of the slot's current Philox counter
  uint32_t ir[MAXS], cy[MAXS], cz[MAXS], cw[MAXS];
#pragma unroll
  for (int k = 0; k < MAXS; ++k) {
    const int p = k < sl.n ? sl.lo[k] + wave * SP + g : 0;
    const bool has = k < sl.n && p < sl.hi[k];
    const int i = has ? L.order[p] : 0;
    if (FIX) { if (!(k & 1)) ir[k >> 1] = 0u; ir[k >> 1] |= (has ? (uint32_t)i : 0xffffu) << (16 * (k & 1)); }
    else ir[k] = has ? ((uint32_t)i << 21) | L.row[i] : 0xffffffffu;
    cy[k] = 0u; cz[k] = 0u; cw[k] = 0u;
  }
  __syncthreads();  // every chain's start state is in place
  for (uint32_t t = sweep0; t < sweep0 + (uint32_t)a.n_sweeps; ++t) {
    // (static slot indices: the slot registers must never be indexed at run time.  A plain unrolled loop with the `k >= n`
    // exit was left rolled by the compiler, the arrays in scratch; a generic lambda per slot lost the LDS address space of
    // the image -- flat loads -- and put the batch arrays in scratch: a recursive template it is.)
    GibbsSlotLoop<0, MAXS, SB, FIX>::run(a, sl, L, stc, valid, cid, t >> 2, t & 3u, t == sweep0 || (t & 3u) == 0u, ir, cy, cz, cw);
  }
  if (valid) {
    int8_t* dst = a.state + (size_t)chain * n;
    for (int i = wave * SP + g; i < n; i += 16 * SP) {
      const float v = (float)*reinterpret_cast<const _Float16*>(stc + SB * i);
      dst[i] = (int8_t)v;
      if (a.samples_out) a.samples_out[(size_t)chain * n + i] = v;
    }
  }
}

// Fast path for graphs of at most 20 rows per lane -- a row being one pass of LPC spins of a colour class -- and
// at most 4 MB <= 20 neighbours per spin: every graph the shipped solvers produce up to 1024 spins.  Same arithmetic,
// same order, same random stream as gibbs_kernel (bit-exact); what changes is the schedule and the LDS image:
//   * a lane owns the same spin of every row in every sweep, so its spin index and clamped field offset are read once,
//     before the sweep loop, and live in registers;
//   * the neighbour tables are stored LANE-MAJOR (graph.h, `lane_eid` / `lane_off`): batch j of row k of lane l sits at
//     ((k MB + j) LPC + l), so a batch read is one ds_read_b128 / ds_read_b64 at an IMMEDIATE offset from a per-lane base
//     -- consecutive lanes read consecutive 16-byte words (no bank conflicts, where the per-row image scattered them) and
//     the ~25 compare / select / address instructions per row of the per-row walk are gone; a lane without a spin in a
//     row, or a spin of fewer than MB batches, finds J = 0 there;
//   * the passes of a colour class are independent of each other and are computed two at a time (NR = 2: classes of more
//     than LPC spins -- c3, c5), side by side: at one wave per SIMD a single row leaves the wave waiting out its LDS
//     round trips and a chain of 20 dependent adds with nothing else to issue;
//   * the state offsets of a step are read one step AHEAD, the couplings first, the stores are unconditional (a sink
//     for lanes without a spin): a step is one straight line of code with one LDS round trip waited out;
//   * Philox words are drawn once per (spin, sweep >> 2) and serve four sweeps, as the counter layout intends.
// (Rounds 3-5 history, c3 draw alone: the per-row image with register-resident row descriptors 1.00 ms; lane-major
// 0.73; two passes side by side 0.68; offsets one step ahead + straight-line steps 0.54.  Forms that lost: two waves
// per chain with 4-wave workgroups (faster alone, twice the workgroups beside the encoder: slower step); a wave PAIR per
// chain in 8-wave workgroups meeting at a barrier per class (0.61 ms); 8 or 2 waves per workgroup (step +0.2 ms).)
// (LDS: gibbs_lane_lds_bytes, gibbs_plan.h)

// One colour-class step of the fast schedule: NRUN rows (slots k, k + 1) side by side -- per row the same reads and
// the same adds, in row order.  The rows' state offsets `o` were read one step AHEAD (they do not depend on the state);
// this step issues its state reads and coupling reads, then reads the NEXT step's offsets (`ol_next`) while those are in
// flight, so that of the two dependent LDS round trips per step (tables, then state) only the second one is waited out.
template <int MB, int LPC, int NR, int NRUN>
__device__ __forceinline__ void gibbs_lane_class(float (&f)[NR], gu32x2 (&o)[NR][MB], const unsigned char* wlk,
                                                 const unsigned char* ol_next, const unsigned char* stb) {
  _Float16 h[NRUN][MB][4];
  gf32x4 w[NRUN][MB];
  // (the couplings first: nothing they wait for, and the LDS serves them while the state addresses are computed)
#pragma unroll
  for (int j = 0; j < MB; ++j) {
#pragma unroll
    for (int r = 0; r < NRUN; ++r) w[r][j] = *reinterpret_cast<const gf32x4*>(wlk + (size_t)(r * MB + j) * LPC * 16);
  }
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int j = 0; j < MB; ++j) {
#pragma unroll
    for (int r = 0; r < NRUN; ++r) {
      h[r][j][0] = *reinterpret_cast<const _Float16*>(stb + (o[r][j][0] & 0xffffu));
      h[r][j][1] = *reinterpret_cast<const _Float16*>(stb + (o[r][j][0] >> 16));
      h[r][j][2] = *reinterpret_cast<const _Float16*>(stb + (o[r][j][1] & 0xffffu));
      h[r][j][3] = *reinterpret_cast<const _Float16*>(stb + (o[r][j][1] >> 16));
    }
  }
#pragma unroll
  for (int r = 0; r < NR; ++r) {
#pragma unroll
    for (int j = 0; j < MB; ++j) o[r][j] = *reinterpret_cast<const gu32x2*>(ol_next + (size_t)(r * MB + j) * LPC * 8);
  }
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int j = 0; j < MB; ++j) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
#pragma unroll
      for (int r = 0; r < NRUN; ++r) f[r] = gibbs_signed_add(h[r][j][e], w[r][j][e], f[r]);
    }
  }
}

// The modes are those of the sweep loop's control above.  What is this form's own:
// HELD: a lane owns the same spin in a slot for the whole draw, so its held flags are one bit per slot in a register; a
// held slot draws no random word and stores to the sink.
// ENERGY: one walk over the steps before the first sweep for the start energy (the fields of the start state; no decision,
// no store), then one convert and one float64 add per update; the value a slot's spin has is one bit per slot in a
// register (`up`), like `held`.
// EXCH: the lanes of an idle slot own no spin in any row (every store of theirs goes to the sink), and a wave of idle slots
// alone passes over the steps (`rows_on`), not over the barriers.  The rows are 16-byte aligned (gibbs_record's A16 = true).
template <int LPC, int WAVES, int MB, int NR, int MAXS, bool HELD = false, int SCHED = 0>
__global__ __launch_bounds__(WAVES * 64) void gibbs_fast_kernel(GibbsArgsT<HELD, SCHED> a) {
  static_assert(!(HELD && SCHED), "no annealed conditional draw");
  static_assert(!GibbsMode<SCHED>::FIELD, "the per-chain-field draw takes the rolled form alone: this image keeps h in registers");
  using M = GibbsMode<SCHED>;
  constexpr bool EXCH = M::EXCH, ENERGY = M::ENERGY;
  extern __shared__ __align__(16) unsigned char smem[];
  const int n = a.n, n_pad = (n + 15) & ~15;
  const int n_rows = a.n_rows;
  const int tid = threadIdx.x;
  // LDS: couplings [n_rows MB][LPC] x 16 B | state offsets [n_rows MB][LPC] x 8 B | state [chains][n_pad] float16 | sinks
  gf32x4* wimg = reinterpret_cast<gf32x4*>(smem);
  gu32x2* oimg = reinterpret_cast<gu32x2*>(smem + (size_t)n_rows * MB * LPC * 16);
  _Float16* state = reinterpret_cast<_Float16*>(smem + (size_t)n_rows * MB * LPC * 24);
  {
    // one (row, batch, lane) cell per thread and trip: four edge ids and four offsets in two coalesced loads, four
    // gathered couplings; two cells in flight
    const int n_cell = n_rows * MB * LPC;
    const int4* eid4 = reinterpret_cast<const int4*>(a.lane_eid);
    const gu32x2* off4 = reinterpret_cast<const gu32x2*>(a.lane_off);
    auto coupling = [&](int e) {
      return e >= 0 ? clampf(__fmul_rn(a.prefactor, a.quadratic[e]), a.j_lo, a.j_hi) : 0.0f;
    };
    for (int q = tid; q < n_cell; q += 2 * WAVES * 64) {
      const int q1 = q + WAVES * 64;
      const bool two = q1 < n_cell;
      const int4 e0 = eid4[q], e1 = two ? eid4[q1] : int4{-1, -1, -1, -1};
      const gu32x2 o0 = off4[q], o1 = two ? off4[q1] : gu32x2{0u, 0u};
      const gf32x4 w0 = {coupling(e0.x), coupling(e0.y), coupling(e0.z), coupling(e0.w)};
      const gf32x4 w1 = {coupling(e1.x), coupling(e1.y), coupling(e1.z), coupling(e1.w)};
      wimg[q] = w0; oimg[q] = o0;
      if (two) { wimg[q1] = w1; oimg[q1] = o1; }
    }
  }

  constexpr int CPW = 64 / LPC;
  const int wave = tid >> 6, lane = tid & 63;
  const int sub = lane / LPC, l = lane % LPC;
  const GibbsSlot slot = gibbs_slot<EXCH, WAVES, CPW>(a, wave, sub);
  const int chain = slot.chain;
  const bool valid = slot.valid;
  _Float16* st = state + (size_t)(wave * CPW + sub) * n_pad;
  const uint32_t cid = a.chain_id0 + (uint32_t)chain;
  [[maybe_unused]] GibbsExchangeLds X{};
  if constexpr (EXCH) {
    X = gibbs_exchange_carve(smem, gibbs_lane_lds_bytes(n_rows, MB, LPC, n, WAVES * CPW), WAVES * CPW);
    gibbs_exchange_stage<WAVES * 64, WAVES * CPW>(a, X, tid);
    // (an idle slot's row: the neighbour reads of its lanes find spins, not what LDS held before)
    if (!valid)
      for (int i = l; i < n; i += LPC) st[i] = (_Float16)1.0f;
  }

  // (read before the chains start: a fresh chain's start configuration is keyed by the sweep index it starts at, so
  // non-persistent draws do not all restart from one configuration)
  const uint32_t sweep0 = a.sweep0_dev ? *a.sweep0_dev : a.sweep0;
  if (valid) {
    // (gibbs_load_chain, spelled out for the plain start: as one call it changes this kernel's register allocation)
    if constexpr (HELD) {
      gibbs_load_chain<LPC, true>(a, st, chain, l, cid, sweep0);
    } else if (a.init) {
      for (int i = l; i < n; i += LPC) {
        u32x4 r = philox4x32_10((uint32_t)i, cid, sweep0, STREAM_INIT, a.k0, a.k1);
        st[i] = (r.x >> 31) ? (_Float16)1.0f : (_Float16)-1.0f;
      }
    } else {
      const int8_t* src = a.state + (size_t)chain * n;
      for (int i = l; i < n; i += LPC) st[i] = (_Float16)(float)src[i];
    }
  }
  // this lane's spin in each row (-1: none) and its clamped field offset
  int sp[MAXS];
  float hs[MAXS];
  [[maybe_unused]] uint32_t held = 0u;  // HELD: bit k = the spin of slot k is held in this lane's chain
#pragma unroll
  for (int k = 0; k < MAXS; ++k) {
    sp[k] = (valid && k < n_rows) ? a.lane_spin[k * LPC + l] : -1;
    hs[k] = sp[k] >= 0 ? clampf(__fmul_rn(a.prefactor, a.linear[sp[k]]), a.h_lo, a.h_hi) : 0.f;
    if constexpr (HELD) {
      if (sp[k] >= 0 && a.clamp[(int64_t)chain * a.clamp_stride + sp[k]] != 0) held |= 1u << k;
    }
  }
  __syncthreads();  // the tables are staged
  if constexpr (!EXCH) {
    if (!valid) return;
  }
  // the rows the wave walks (EXCH: a wave whose slots all idle has none -- it passes over the steps, not over the barriers)
  const int rows_on = (EXCH && __builtin_amdgcn_ballot_w64(valid) == 0) ? 0 : n_rows;

  // the byte a lane stores its slot-k decision to: its spin's, or its own entry of the wave's sink when it has none
  // (an unconditional store keeps a class step one straight line of code)
  _Float16* sink = state + (size_t)WAVES * CPW * n_pad + (size_t)wave * 64 + lane;
  const unsigned char* wl = smem + (size_t)l * 16;
  const unsigned char* ol = smem + (size_t)n_rows * MB * LPC * 16 + (size_t)l * 8;
  const unsigned char* stb = reinterpret_cast<const unsigned char*>(st);
  // the lane updates a spin in slot K (else its decision goes to the sink)
#define DVG_GIBBS_FREE(K) (HELD ? (sp[K] >= 0 && ((held >> (K)) & 1u) == 0u) : sp[K] >= 0)
  u32x4 rr[MAXS];
#pragma unroll
  for (int k = 0; k < MAXS; ++k) rr[k] = u32x4{0u, 0u, 0u, 0u};
  gu32x2 o[NR][MB];                  // the coming step's state offsets
#pragma unroll
  for (int r = 0; r < NR; ++r) {
#pragma unroll
    for (int j = 0; j < MB; ++j) o[r][j] = *reinterpret_cast<const gu32x2*>(ol + (size_t)(r * MB + j) * LPC * 8);
  }
  GibbsControl ctl = gibbs_begin<SCHED>(a, X, slot);
  [[maybe_unused]] uint32_t up = 0u;  // ENERGY: bit k = the spin of slot k is +1
  if constexpr (ENERGY) {
    // the sweep loop's walk over the steps, on the start state (it leaves `o` at step 0's offsets again)
#pragma unroll
    for (int c = 0; c < MAXS / NR; ++c) {
      const int k0 = NR * c, k1 = k0 + NR - 1;
      if (k0 >= rows_on) continue;
      const unsigned char* wlk = wl + (size_t)k0 * MB * LPC * 16;
      const unsigned char* ol_next = ol + (size_t)(k0 + NR < n_rows ? k0 + NR : 0) * MB * LPC * 8;
      float f[NR];
#pragma unroll
      for (int r = 0; r < NR; ++r) f[r] = hs[k0 + r];
      bool both = false;
      if constexpr (NR == 2) both = __builtin_amdgcn_ballot_w64(sp[k1] >= 0) != 0;
      if (both) gibbs_lane_class<MB, LPC, NR, NR>(f, o, wlk, ol_next, stb);
      else gibbs_lane_class<MB, LPC, NR, 1>(f, o, wlk, ol_next, stb);
#pragma unroll
      for (int r = 0; r < NR; ++r) {  // (a row the step left out has no spin in any lane of the wave)
        if (sp[k0 + r] >= 0) {
          const _Float16 s = st[sp[k0 + r]];
          ctl.e += gibbs_start_energy(s, hs[k0 + r], f[r]);
          if ((float)s > 0.0f) up |= 1u << (k0 + r);
        }
      }
    }
  }
  // AIS: slot K's decision S on the field F goes into the lane's energy share; lanes that update no spin there add 0
#define DVG_GIBBS_WEIGH(K, S, F)                                                                            \
  if constexpr (ENERGY) {                                                                                    \
    const bool fr = DVG_GIBBS_FREE(K);                                                                      \
    const float sn = (float)(S), so = ((up >> (K)) & 1u) ? 1.0f : -1.0f;                                    \
    ctl.e += gibbs_energy_step(fr ? sn : so, so, F);                                                        \
    if (fr) up = (up & ~(1u << (K))) | (sn > 0.0f ? 1u << (K) : 0u);                                        \
  }
  for (uint32_t t = sweep0; t < sweep0 + (uint32_t)a.n_sweeps; ++t) {
    const uint32_t tq = t >> 2, tw = t & 3u;
    const float two_beta = gibbs_sweep_head<SCHED>(a, t, sweep0, ctl);
    if (t == sweep0 || tw == 0u) {
#pragma unroll
      for (int k = 0; k < MAXS; ++k)
        if (DVG_GIBBS_FREE(k)) rr[k] = philox4x32_10((uint32_t)sp[k], cid, tq, STREAM_GIBBS, a.k0, a.k1);
    }
    // word tw of a slot's four, as two bit-selects under wave-uniform masks (a uniform `?:` becomes scalar branches,
    // four per slot and sweep)
    const uint32_t m1 = 0u - (tw & 1u), m2 = 0u - (tw >> 1);
#define DVG_GIBBS_WORD(K) (((((rr[K].x & ~m1) | (rr[K].y & m1)) & ~m2)) | (((rr[K].z & ~m1) | (rr[K].w & m1)) & m2))
#pragma unroll
    for (int c = 0; c < MAXS / NR; ++c) {
      const int k0 = NR * c, k1 = k0 + NR - 1;
      if (k0 >= rows_on) {  // (AIS: with the early exit the compiler left this loop rolled at 20 slots, the slot registers in scratch)
        if constexpr (ENERGY) continue;
        else break;
      }
      const unsigned char* wlk = wl + (size_t)k0 * MB * LPC * 16;
      const unsigned char* ol_next = ol + (size_t)(k0 + NR < n_rows ? k0 + NR : 0) * MB * LPC * 8;
      float f[NR];
#pragma unroll
      for (int r = 0; r < NR; ++r) f[r] = hs[k0 + r];
      bool both = false;
      if constexpr (NR == 2) both = __builtin_amdgcn_ballot_w64(sp[k1] >= 0) != 0;
      if (both) {
        gibbs_lane_class<MB, LPC, NR, NR>(f, o, wlk, ol_next, stb);
        const _Float16 s0 = gibbs_decide(f[0], two_beta, DVG_GIBBS_WORD(k0));
        const _Float16 s1 = gibbs_decide(f[NR - 1], two_beta, DVG_GIBBS_WORD(k1));
        DVG_GIBBS_WEIGH(k0, s0, f[0])
        DVG_GIBBS_WEIGH(k1, s1, f[NR - 1])
        *(DVG_GIBBS_FREE(k0) ? st + sp[k0] : sink) = s0;
        *(DVG_GIBBS_FREE(k1) ? st + sp[k1] : sink) = s1;
      } else {  // one row (NR = 2: the step's second row is empty for the whole wave)
        gibbs_lane_class<MB, LPC, NR, 1>(f, o, wlk, ol_next, stb);
        const _Float16 s0 = gibbs_decide(f[0], two_beta, DVG_GIBBS_WORD(k0));
        DVG_GIBBS_WEIGH(k0, s0, f[0])
        *(DVG_GIBBS_FREE(k0) ? st + sp[k0] : sink) = s0;
      }
      // the next class reads what this one wrote (same wave): order LDS traffic.  (Passes of one class are independent
      // of each other, so a fence between them is harmless.)
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
      __builtin_amdgcn_wave_barrier();
    }
    gibbs_sweep_tail<LPC, WAVES * CPW, SCHED, true>(a, X, slot, st, l, t, sweep0, ctl);
  }
#undef DVG_GIBBS_WORD
#undef DVG_GIBBS_WEIGH
#undef DVG_GIBBS_FREE
  gibbs_finish<LPC, SCHED>(a, X, slot, st, l, ctl);
}

// ---------------------------------------------------------------- host: plan (gibbs_plan.h), fill arguments, launch
template <bool HELD, int SCHED>
using GibbsKernelT = void (*)(GibbsArgsT<HELD, SCHED>);

// the instantiation a plan names; null: it has none.  The tables expand from the lists the plan chose from.
template <bool HELD, int SCHED>
static GibbsKernelT<HELD, SCHED> gibbs_kernel_of(const GibbsDrawPlan& p) {
  if constexpr (!GibbsMode<SCHED>::FIELD) {  // (the field kinds are planned rolled on every graph and have no lane-major instantiation)
#define DVG_GIBBS_LANE_ENTRY(LPC, W, MB, NR, MAXS)                                                      \
  if (p.form == GF_LANE && p.lpc == LPC && p.waves == W && p.mb == MB && p.nr == NR && p.maxs == MAXS)  \
    return gibbs_fast_kernel<LPC, W, MB, NR, MAXS, HELD, SCHED>;
    DVG_GIBBS_LANE_KERNELS(DVG_GIBBS_LANE_ENTRY)
#undef DVG_GIBBS_LANE_ENTRY
  }
#define DVG_GIBBS_ROLLED_ENTRY(LPC, W) \
  if (p.form == GF_ROLLED && p.lpc == LPC && p.waves == W) return gibbs_kernel<LPC, W, HELD, SCHED>;
  DVG_GIBBS_ROLLED_KERNELS(DVG_GIBBS_ROLLED_ENTRY)
#undef DVG_GIBBS_ROLLED_ENTRY
  return nullptr;
}
static void (*gibbs_slot_kernel_of(const GibbsDrawPlan& p))(GibbsArgs, GibbsSlots) {
#define DVG_GIBBS_SLOT_ENTRY(MAXS, CH, FIX) \
  if (p.form == GF_SLOTS && p.maxs == MAXS && p.ch == CH && p.fix == FIX) return gibbs_slot_kernel<MAXS, CH, FIX>;
  DVG_GIBBS_SLOT_KERNELS(DVG_GIBBS_SLOT_ENTRY)
#undef DVG_GIBBS_SLOT_ENTRY
  return nullptr;
}

template <typename... A>
static int gibbs_launch(void (*kern)(A...), const GibbsDrawPlan& p, const GibbsArgs& a, hipStream_t s, A... args) {
  if (!kern) {  // (a plan without an instantiation is an error, never another kernel)
    set_error("gibbs: lane image (%d lanes per chain, %d batches, %d rows in steps of %d) has no kernel", p.lpc, p.mb, a.n_rows, p.nr);
    return DVG_E_UNSUPPORTED;
  }
  if (p.lds > 64 * 1024)
    DVG_CHECK_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds));
  // work = spin updates of the draw (bench.py's sampler roofline)
  DVG_LAUNCH_WORK(K_GIBBS, (double)a.n_chains * a.n * a.n_sweeps, kern, dim3(p.grid), dim3(p.threads), p.lds, s, args...);
  return DVG_OK;
}

}  // namespace dvg

using namespace dvg;

// Every draw: plan, attach the lane image, launch.  The exchange draws have a planner of their own (the replica count is an
// input) and the same tables; with the records (GIBBS_EXCHANGE_TRACE) the same plan, the same forms, the same LDS.
template <bool HELD, int SCHED = 0>
static int gibbs_draw(const dvg_graph_t* g, GibbsArgsT<HELD, SCHED>& a, hipStream_t s) {
  constexpr GibbsDrawKind KIND = HELD                     ? GK_HELD
                                 : GibbsMode<SCHED>::EXCH ? GK_EXCHANGE
                                 : SCHED == GIBBS_FIELD_WEIGH ? GK_FIELD_WEIGH
                                 : SCHED == GIBBS_WEIGH   ? GK_WEIGH
                                 : SCHED == GIBBS_TABLE   ? GK_TABLE
                                 : SCHED == GIBBS_TRACE   ? GK_TRACE
                                 : SCHED == GIBBS_FIELD   ? GK_FIELD
                                                          : GK_PLAIN;
  GibbsDrawPlan p;
  if constexpr (KIND == GK_EXCHANGE) {
    DVG_TRY(gibbs_exchange_plan(g->shape, a.n_chains / a.n_replicas, a.n_replicas, opt(OPT_GIBBS_GENERIC), &p, nullptr));
  } else {
    DVG_TRY(gibbs_draw_plan(g->shape, a.n_chains, KIND, opt(OPT_GIBBS_GENERIC), &p));
  }
  if (p.form == GF_LANE) {
    a.lane_spin = g->lane_spin; a.lane_eid = g->lane_eid; a.lane_off = g->lane_off; a.n_rows = g->shape.lane_rows;
  }
  if constexpr (KIND == GK_PLAIN) {
    if (p.form == GF_SLOTS) return gibbs_launch(gibbs_slot_kernel_of(p), p, a, s, a, p.slots);
  }
  return gibbs_launch(gibbs_kernel_of<HELD, SCHED>(p), p, a, s, a);
}

// What every draw checks, under its entry point's name `who`.  `missing`: the entry point's own null argument, if any
// (its message).  `table`: an annealed draw (an entry per sweep: at least one).  `stride`: the per-chain stride of the
// entry point's [n_chains or 1][row] array and the names of the two in its signature (null: it has no such array).
struct GibbsStride { const char* name; int64_t value; const char* row_name; int row; };
static int gibbs_check(const char* who, const dvg_graph_t* g, bool tensors, const char* missing, int n_chains, int n_sweeps,
                       bool table, const GibbsStride* stride) {
  DVG_REQUIRE(g && tensors, "%s: null argument", who);
  DVG_REQUIRE(!missing, "%s: %s", who, missing);
  DVG_REQUIRE(n_chains > 0 && n_sweeps >= (table ? 1 : 0), "%s: n_chains=%d n_sweeps=%d%s", who, n_chains, n_sweeps,
              table ? " (the table has an entry per sweep: at least one)" : "");
  DVG_REQUIRE(g->n <= 32767, "%s: graph too large (n=%d: 16-bit state offsets)", who, g->n);
  DVG_REQUIRE(!stride || stride->value == 0 || stride->value == stride->row,
              "%s: %s=%lld is neither 0 (one shared row) nor %s=%d (a row per chain)", who, stride->name,
              (long long)stride->value, stride->row_name, stride->row);
  return DVG_OK;
}

static void gibbs_fill_args(GibbsArgs& a, const dvg_graph_t* g, const float* linear, const float* quadratic, float prefactor,
                            float h_lo, float h_hi, float j_lo, float j_hi, float beta, int8_t* state, int n_chains,
                            uint32_t chain_id0, uint64_t seed, uint32_t sweep0, int n_sweeps, int init, float* samples_out,
                            const dvg_step_state_t* dyn) {
  a.order = g->order; a.class_ptr = g->class_ptr;
  a.adj_idx = g->adj_idx; a.adj_eid = g->adj_eid; a.adj_row = g->adj_row; a.adj_src4 = g->adj_src4;
  a.linear = linear; a.quadratic = quadratic;
  a.n = g->n; a.n_batches = g->shape.n_batches; a.max_batches = g->shape.max_batches; a.n_colours = g->n_colours;
  a.prefactor = prefactor; a.h_lo = h_lo; a.h_hi = h_hi; a.j_lo = j_lo; a.j_hi = j_hi;
  a.two_beta = 2.0f * beta;
  a.state = state; a.samples_out = samples_out; a.n_chains = n_chains;
  a.chain_id0 = chain_id0; a.k0 = (uint32_t)seed; a.k1 = (uint32_t)(seed >> 32);
  a.sweep0 = sweep0; a.n_sweeps = n_sweeps; a.init = init;
  a.sweep0_dev = dyn ? &dyn->sweep0 : nullptr;
  a.lane_spin = nullptr; a.lane_eid = nullptr; a.lane_off = nullptr; a.n_rows = 0;
}

extern "C" int dvg_gibbs_sample(const dvg_graph_t* g, const float* linear, const float* quadratic,
                                float prefactor, float h_lo, float h_hi, float j_lo, float j_hi,
                                float beta, int8_t* state, int n_chains, uint32_t chain_id0,
                                uint64_t seed, uint32_t sweep0, int n_sweeps, int init,
                                float* samples_out, const dvg_step_state_t* dyn, dvg_stream_t stream) {
  DVG_TRY(gibbs_check("gibbs", g, linear && quadratic && state, nullptr, n_chains, n_sweeps, false, nullptr));
  GibbsArgs a;
  gibbs_fill_args(a, g, linear, quadratic, prefactor, h_lo, h_hi, j_lo, j_hi, beta, state, n_chains, chain_id0, seed, sweep0,
                  n_sweeps, init, samples_out, dyn);
  return gibbs_draw<false>(g, a, (hipStream_t)stream);
}

// The conditional draw: spins with a nonzero flag in `clamp` are held at their value in `state` (include/dvg.h).
extern "C" int dvg_gibbs_sample_clamped(const dvg_graph_t* g, const float* linear, const float* quadratic,
                                        float prefactor, float h_lo, float h_hi, float j_lo, float j_hi,
                                        float beta, int8_t* state, int n_chains, uint32_t chain_id0,
                                        uint64_t seed, uint32_t sweep0, int n_sweeps, int init,
                                        const uint8_t* clamp, int64_t clamp_chain_stride,
                                        float* samples_out, const dvg_step_state_t* dyn, dvg_stream_t stream) {
  const GibbsStride stride{"clamp_chain_stride", clamp_chain_stride, "n", g ? g->n : 0};
  DVG_TRY(gibbs_check("gibbs_clamped", g, linear && quadratic && state,
                      clamp ? nullptr : "null clamp (a draw that holds nothing is dvg_gibbs_sample)", n_chains, n_sweeps, false, &stride));
  GibbsHeldArgs a;
  gibbs_fill_args(a, g, linear, quadratic, prefactor, h_lo, h_hi, j_lo, j_hi, beta, state, n_chains, chain_id0, seed, sweep0,
                  n_sweeps, init, samples_out, dyn);
  a.clamp = clamp; a.clamp_stride = clamp_chain_stride;
  return gibbs_draw<true>(g, a, (hipStream_t)stream);
}

// The annealed draw: sweep k of the call on chain c runs at betas[c * beta_chain_stride + k] (include/dvg.h).
extern "C" int dvg_gibbs_sample_annealed(const dvg_graph_t* g, const float* linear, const float* quadratic,
                                         float prefactor, float h_lo, float h_hi, float j_lo, float j_hi,
                                         const float* betas, int64_t beta_chain_stride,
                                         int8_t* state, int n_chains, uint32_t chain_id0, uint64_t seed,
                                         uint32_t sweep0, int n_sweeps, int init, float* samples_out,
                                         const dvg_step_state_t* dyn, dvg_stream_t stream) {
  const GibbsStride stride{"beta_chain_stride", beta_chain_stride, "n_sweeps", n_sweeps};
  DVG_TRY(gibbs_check("gibbs_annealed", g, linear && quadratic && state,
                      betas ? nullptr : "null betas (a draw at one fixed beta is dvg_gibbs_sample)", n_chains, n_sweeps, true, &stride));
  GibbsSchedArgs a;
  gibbs_fill_args(a, g, linear, quadratic, prefactor, h_lo, h_hi, j_lo, j_hi, 0.0f, state, n_chains, chain_id0, seed, sweep0,
                  n_sweeps, init, samples_out, dyn);
  a.betas = betas; a.beta_stride = beta_chain_stride;
  return gibbs_draw<false, GIBBS_TABLE>(g, a, (hipStream_t)stream);
}

// The AIS draw: the annealed draw plus, per chain, its log importance weight and its final energy (include/dvg.h).
extern "C" int dvg_gibbs_sample_ais(const dvg_graph_t* g, const float* linear, const float* quadratic,
                                    float prefactor, float h_lo, float h_hi, float j_lo, float j_hi,
                                    const float* betas, int64_t beta_chain_stride, float beta_from,
                                    int8_t* state, int n_chains, uint32_t chain_id0, uint64_t seed,
                                    uint32_t sweep0, int n_sweeps, int init, float* samples_out,
                                    double* log_weight_out, double* energy_out,
                                    const dvg_step_state_t* dyn, dvg_stream_t stream) {
  const GibbsStride stride{"beta_chain_stride", beta_chain_stride, "n_sweeps", n_sweeps};
  DVG_TRY(gibbs_check("gibbs_ais", g, linear && quadratic && state,
                      !betas ? "null betas"
                      : !log_weight_out ? "null log_weight_out (a draw that is not weighed is dvg_gibbs_sample_annealed)" : nullptr,
                      n_chains, n_sweeps, true, &stride));
  DVG_REQUIRE(beta_from >= 0.0f && beta_from <= 3.4028234663852886e38f, "gibbs_ais: beta_from=%g must be finite and >= 0", (double)beta_from);
  DVG_REQUIRE(init == 0 || beta_from == 0.0f,
              "gibbs_ais: init=%d with beta_from=%g (fresh chains are uniform: a sample at beta 0 and at no other)", init, (double)beta_from);
  GibbsAisArgs a;
  gibbs_fill_args(a, g, linear, quadratic, prefactor, h_lo, h_hi, j_lo, j_hi, 0.0f, state, n_chains, chain_id0, seed, sweep0,
                  n_sweeps, init, samples_out, dyn);
  a.betas = betas; a.beta_stride = beta_chain_stride;
  a.beta_from = beta_from; a.log_weight_out = log_weight_out; a.energy_out = energy_out;
  return gibbs_draw<false, GIBBS_WEIGH>(g, a, (hipStream_t)stream);
}

// What both traced draws check of the sweeps they record, under the entry point's name `who`; `plain`: the draw without a trace.
static int gibbs_record_check(const char* who, const char* plain, int n_sweeps, int burn_in, int thin) {
  DVG_REQUIRE(burn_in >= 0, "%s: burn_in=%d must be at least 0", who, burn_in);
  DVG_REQUIRE(thin >= 1, "%s: thin=%d must be at least 1", who, thin);
  DVG_REQUIRE(burn_in <= n_sweeps && n_sweeps - burn_in >= thin,  // (n_sweeps >= burn_in + thin, without the sum's overflow)
              "%s: n_sweeps=%d, burn_in=%d, thin=%d record nothing (a draw that records nothing is %s)", who, n_sweeps, burn_in, thin,
              plain);
  return DVG_OK;
}

// The exchange draw ("DVG PT v1", include/dvg.h): ladders of n_replicas chains, each at the beta of the rung it holds; every
// swap_every sweeps the chains of neighbouring rungs of a ladder exchange them on a Metropolis coin.
// what both exchange draws check, under the entry point's name `who`; `missing`: the entry point's own null argument, if any
static int gibbs_exchange_check(const char* who, const dvg_graph_t* g, const float* linear, const float* quadratic, const float* ladder,
                                int n_replicas, int swap_every, const int8_t* state, const int32_t* rung, int n_chains, int n_sweeps,
                                const char* missing, const dvg_step_state_t* dyn) {
  DVG_TRY(gibbs_check(who, g, linear && quadratic && state,
                      !ladder ? "null ladder (a draw at one fixed beta is dvg_gibbs_sample)" : !rung ? "null rung" : missing,
                      n_chains, n_sweeps, false, nullptr));
  DVG_REQUIRE(n_sweeps >= 1, "%s: n_sweeps=%d (a draw of at least one sweep)", who, n_sweeps);
  DVG_REQUIRE(n_replicas >= 2 && n_replicas <= GIBBS_MAX_REPLICAS, "%s: n_replicas=%d is not in 2..%d", who, n_replicas,
              GIBBS_MAX_REPLICAS);
  DVG_REQUIRE(n_chains % n_replicas == 0, "%s: n_chains=%d is not a multiple of n_replicas=%d (whole ladders)", who, n_chains,
              n_replicas);
  DVG_REQUIRE(swap_every >= 1, "%s: swap_every=%d must be at least 1", who, swap_every);
  DVG_REQUIRE(!dyn, "%s: dyn must be NULL (the exchanges of a call are counted on the host, from its sweep0)", who);
  return DVG_OK;
}

extern "C" int dvg_gibbs_sample_tempered(const dvg_graph_t* g, const float* linear, const float* quadratic,
                                         float prefactor, float h_lo, float h_hi, float j_lo, float j_hi,
                                         const float* ladder, int n_replicas, int swap_every,
                                         int8_t* state, int32_t* rung, int n_chains, uint32_t chain_id0, uint64_t seed,
                                         uint32_t sweep0, int n_sweeps, int init, float* samples_out,
                                         double* energy_out, uint32_t* accept_out,
                                         const dvg_step_state_t* dyn, dvg_stream_t stream) {
  DVG_TRY(gibbs_exchange_check("gibbs_tempered", g, linear, quadratic, ladder, n_replicas, swap_every, state, rung, n_chains, n_sweeps,
                               nullptr, dyn));
  GibbsExchangeArgs a;
  gibbs_fill_args(a, g, linear, quadratic, prefactor, h_lo, h_hi, j_lo, j_hi, 0.0f, state, n_chains, chain_id0, seed, sweep0,
                  n_sweeps, init, samples_out, nullptr);
  a.ladder = ladder; a.n_replicas = n_replicas; a.swap_every = swap_every;
  a.rung = rung; a.energy_out = energy_out; a.accept_out = accept_out;
  return gibbs_draw<false, GIBBS_EXCHANGE>(g, a, (hipStream_t)stream);
}

// The traced exchange draw ("DVG PT trace v1", include/dvg.h): dvg_gibbs_sample_tempered, with a history by rung -- packed
// state, carried energy -- and the rung walk by chain written out behind the exchange block of the recorded sweeps.
extern "C" int dvg_gibbs_sample_tempered_traced(const dvg_graph_t* g, const float* linear, const float* quadratic,
                                                float prefactor, float h_lo, float h_hi, float j_lo, float j_hi,
                                                const float* ladder, int n_replicas, int swap_every,
                                                int8_t* state, int32_t* rung, int n_chains, uint32_t chain_id0, uint64_t seed,
                                                uint32_t sweep0, int n_sweeps, int init, float* samples_out,
                                                double* energy_out, uint32_t* accept_out,
                                                uint32_t* trace_out, double* energy_trace_out, uint8_t* rung_trace_out,
                                                int burn_in, int thin, const dvg_step_state_t* dyn, dvg_stream_t stream) {
  DVG_TRY(gibbs_exchange_check("gibbs_tempered_traced", g, linear, quadratic, ladder, n_replicas, swap_every, state, rung, n_chains,
                               n_sweeps, trace_out ? nullptr : "null trace_out (a draw that records nothing is dvg_gibbs_sample_tempered)",
                               dyn));
  DVG_TRY(gibbs_record_check("gibbs_tempered_traced", "dvg_gibbs_sample_tempered", n_sweeps, burn_in, thin));
  GibbsExchangeTraceArgs a;
  gibbs_fill_args(a, g, linear, quadratic, prefactor, h_lo, h_hi, j_lo, j_hi, 0.0f, state, n_chains, chain_id0, seed, sweep0,
                  n_sweeps, init, samples_out, nullptr);
  a.ladder = ladder; a.n_replicas = n_replicas; a.swap_every = swap_every;
  a.rung = rung; a.energy_out = energy_out; a.accept_out = accept_out;
  a.trace = trace_out; a.energy_trace = energy_trace_out; a.rung_trace = rung_trace_out;
  a.burn_in = burn_in; a.thin = thin; a.n_records = (n_sweeps - burn_in) / thin;
  return gibbs_draw<false, GIBBS_EXCHANGE_TRACE>(g, a, (hipStream_t)stream);
}

// The traced draw ("DVG trace v1", include/dvg.h): dvg_gibbs_sample, with the chains' states after the recorded sweeps
// written out one bit per spin.
extern "C" int dvg_gibbs_sample_traced(const dvg_graph_t* g, const float* linear, const float* quadratic,
                                       float prefactor, float h_lo, float h_hi, float j_lo, float j_hi,
                                       float beta, int8_t* state, int n_chains, uint32_t chain_id0,
                                       uint64_t seed, uint32_t sweep0, int n_sweeps, int init,
                                       float* samples_out, uint32_t* trace_out, int burn_in, int thin,
                                       const dvg_step_state_t* dyn, dvg_stream_t stream) {
  DVG_TRY(gibbs_check("gibbs_traced", g, linear && quadratic && state,
                      trace_out ? nullptr : "null trace_out (a draw that records nothing is dvg_gibbs_sample)", n_chains, n_sweeps,
                      false, nullptr));
  DVG_TRY(gibbs_record_check("gibbs_traced", "dvg_gibbs_sample", n_sweeps, burn_in, thin));
  DVG_REQUIRE(!dyn, "gibbs_traced: dyn must be NULL (the draw is one-off: the recorded sweeps are counted from the host's sweep0)");
  GibbsTraceArgs a;
  gibbs_fill_args(a, g, linear, quadratic, prefactor, h_lo, h_hi, j_lo, j_hi, beta, state, n_chains, chain_id0, seed, sweep0,
                  n_sweeps, init, samples_out, nullptr);
  a.trace = trace_out; a.burn_in = burn_in; a.thin = thin; a.n_records = (n_sweeps - burn_in) / thin;
  return gibbs_draw<false, GIBBS_TRACE>(g, a, (hipStream_t)stream);
}

// The per-chain-field draw ("DVG field v1", include/dvg.h): chain c samples the model whose linear vector is
// rn(linear + fields[c * field_chain_stride + .]); everything behind that add is dvg_gibbs_sample's.
extern "C" int dvg_gibbs_sample_fields(const dvg_graph_t* g, const float* linear, const float* quadratic,
                                       float prefactor, float h_lo, float h_hi, float j_lo, float j_hi,
                                       float beta, int8_t* state, int n_chains, uint32_t chain_id0,
                                       uint64_t seed, uint32_t sweep0, int n_sweeps, int init,
                                       const float* fields, int64_t field_chain_stride,
                                       float* samples_out, const dvg_step_state_t* dyn, dvg_stream_t stream) {
  const GibbsStride stride{"field_chain_stride", field_chain_stride, "n", g ? g->n : 0};
  DVG_TRY(gibbs_check("gibbs_fields", g, linear && quadratic && state,
                      fields ? nullptr : "null fields (a draw without fields is dvg_gibbs_sample)", n_chains, n_sweeps, false, &stride));
  DVG_REQUIRE(!dyn, "gibbs_fields: dyn must be NULL (the draw is one-off, not part of a captured step)");
  GibbsFieldArgs a;
  gibbs_fill_args(a, g, linear, quadratic, prefactor, h_lo, h_hi, j_lo, j_hi, beta, state, n_chains, chain_id0, seed, sweep0,
                  n_sweeps, init, samples_out, nullptr);
  a.fields = fields; a.field_stride = field_chain_stride;
  return gibbs_draw<false, GIBBS_FIELD>(g, a, (hipStream_t)stream);
}

// The weighed per-chain-field draw ("DVG field AIS v1", include/dvg.h): the per-chain-field draw along a path in (beta, field
// strength), both looked up per sweep, with the AIS draw's log weight and energy per chain; R chains share a row of `fields`.
extern "C" int dvg_gibbs_sample_fields_ais(const dvg_graph_t* g, const float* linear, const float* quadratic,
                                           float prefactor, float h_lo, float h_hi, float j_lo, float j_hi,
                                           const float* betas, int64_t beta_chain_stride, float beta_from,
                                           const float* scales, int64_t scale_chain_stride, float scale_from,
                                           int8_t* state, int n_chains, uint32_t chain_id0, uint64_t seed,
                                           uint32_t sweep0, int n_sweeps, int init,
                                           const float* fields, int64_t field_chain_stride, int field_row_chains,
                                           float* samples_out, double* log_weight_out, double* energy_out,
                                           const dvg_step_state_t* dyn, dvg_stream_t stream) {
  const char* who = "gibbs_fields_ais";
  const GibbsStride stride{"field_chain_stride", field_chain_stride, "n", g ? g->n : 0};
  DVG_TRY(gibbs_check(who, g, linear && quadratic && state,
                      !fields  ? "null fields (a weighed draw without fields is dvg_gibbs_sample_ais)"
                      : !betas ? "null betas"
                               : nullptr,
                      n_chains, n_sweeps, true, &stride));
  DVG_REQUIRE(beta_chain_stride == 0 || beta_chain_stride == n_sweeps,
              "%s: beta_chain_stride=%lld is neither 0 (one shared row) nor n_sweeps=%d (a row per chain)", who,
              (long long)beta_chain_stride, n_sweeps);
  DVG_REQUIRE(scale_chain_stride == 0 || scale_chain_stride == n_sweeps,
              "%s: scale_chain_stride=%lld is neither 0 (one shared row) nor n_sweeps=%d (a row per chain)", who,
              (long long)scale_chain_stride, n_sweeps);
  DVG_REQUIRE(field_row_chains >= 1, "%s: field_row_chains=%d must be at least 1", who, field_row_chains);
  DVG_REQUIRE(beta_from >= 0.0f && beta_from <= 3.4028234663852886e38f, "%s: beta_from=%g must be finite and >= 0", who, (double)beta_from);
  DVG_REQUIRE(scale_from >= -3.4028234663852886e38f && scale_from <= 3.4028234663852886e38f, "%s: scale_from=%g must be finite", who,
              (double)scale_from);
  DVG_REQUIRE(init == 0 || beta_from == 0.0f,
              "%s: init=%d with beta_from=%g (fresh chains are uniform: a sample at beta 0 and at no other)", who, init, (double)beta_from);
  DVG_REQUIRE(!dyn, "%s: dyn must be NULL (the draw is one-off, not part of a captured step)", who);
  GibbsFieldAisArgs a;
  gibbs_fill_args(a, g, linear, quadratic, prefactor, h_lo, h_hi, j_lo, j_hi, 0.0f, state, n_chains, chain_id0, seed, sweep0,
                  n_sweeps, init, samples_out, nullptr);
  a.betas = betas; a.beta_stride = beta_chain_stride;
  a.beta_from = beta_from; a.log_weight_out = log_weight_out; a.energy_out = energy_out;
  a.fields = fields; a.field_stride = field_chain_stride; a.row_chains = field_row_chains;
  a.scales = scales; a.scale_stride = scale_chain_stride; a.scale_from = scale_from;
  return gibbs_draw<false, GIBBS_FIELD_WEIGH>(g, a, (hipStream_t)stream);
}

// The launch geometry dvg_gibbs_sample would use for `n_chains` chains on this graph (nothing is launched): workgroups,
// threads per workgroup, LDS bytes per workgroup.  The host side sizes what runs BESIDE the draw with it (the encoder
// forward's Winograd launches take whole CUs: ModelWrapper leaves the draw's CUs out of their persistent grid).
extern "C" int dvg_gibbs_launch_info(const dvg_graph_t* g, int n_chains, int* workgroups, int* threads, size_t* lds_bytes) {
  DVG_REQUIRE(g && n_chains > 0, "gibbs_launch_info: null graph / no chains");
  GibbsDrawPlan p;
  DVG_TRY(gibbs_draw_plan(g->shape, n_chains, GK_PLAIN, opt(OPT_GIBBS_GENERIC), &p));
  if (workgroups) *workgroups = p.grid;
  if (threads) *threads = p.threads;
  if (lds_bytes) *lds_bytes = p.lds;
  return DVG_OK;
}
