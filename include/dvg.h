/* dvg.h — C ABI of libdvg.so: the MI355X (gfx950) DVAE + GRBM training path.
 *
 * This is the drop-in boundary.  The reference is pure Python
 * over PyTorch and the un-vendored `dwave-pytorch-plugin`; each entry point
 * below replaces the arithmetic behind one reference call site (cited per
 * function).  The reference-side binding is a ctypes stub, shown in
 * INTEGRATION.md and implemented in image-generation_amd/_lib.py.
 *
 * Conventions
 *   - plain pointers and sizes only; every `float*`/`int8_t*`/... argument not
 *     marked [host] is a DEVICE pointer owned by the caller (torch owns memory);
 *   - every function enqueues its work on `stream` (a hipStream_t passed as
 *     void*) and returns without synchronising; no hidden allocation except
 *     inside dvg_graph_create;
 *   - return value: 0 (DVG_OK) or a negative DVG_E_* code; the message is
 *     available from dvg_last_error() (thread-local); nothing throws or exits;
 *   - process-wide state, all of it listed here: (1) the optional per-kernel
 *     profiler (dvg_prof_*), (2) the GEMM-operand mode set by
 *     dvg_set_conv_precision (one atomic int; a forward call and its backward
 *     call must run in the same mode, which the library checks per workspace),
 *     (3) one library-owned side stream + event ring per device, created under
 *     a mutex by the first *_workspace_bytes query or backward call on that
 *     device and used for the fork/join inside dvg_encoder_bwd /
 *     dvg_decoder_bwd, (4) eight kernel-form switches (dvg_set_option: named
 *     integers, relaxed atomics, read per call), each selecting between two
 *     TESTED forms of the same function; the product path is every switch's
 *     default and no caller in this repository sets one outside tests and A/B
 *     measurements (round 4 had 32, among them grid-sizing knobs that
 *     ModelWrapper set per model: those are compile-time constants now; round
 *     5 had 16: the A/B references of forms a default replaced and the test
 *     knobs live behind include/dvg_dev.h, dvg_dev_set_option, since round 6).  A
 *     switch is process-wide: flipping one between a forward call and its
 *     backward call is caught per workspace (the forward records the plan, a
 *     backward under another plan fails with DVG_E_INVALID instead of reading
 *     what its forward never wrote),
 *     (5) host-side bookkeeping keyed by workspace pointer: the mode and plan a
 *     forward call ran under (checked by its backward call) and the mark of a
 *     dvg_decoder_prepare in flight (one event per workspace), (6) per device, a
 *     pool of 32 sets of tile counters in device memory for the dynamically
 *     scheduled Winograd grids (option wino_dynamic): a launch takes the next
 *     set and leaves it zeroed; more than 32 such launches in flight at once
 *     on one device are not supported.
 *     Nothing else persists between calls; entry points are re-entrant per
 *     (stream, workspace).  HIP is initialised lazily by the
 *     first call in each process (the Dash app runs training in a spawned
 *     worker: /root/reference/app.py:37-43).
 */
#ifndef DVG_H
#define DVG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DVG_OK 0
#define DVG_E_INVALID (-1)     /* bad argument (shape, null pointer, unsupported size) */
#define DVG_E_HIP (-2)         /* a HIP runtime call failed */
#define DVG_E_WORKSPACE (-3)   /* caller workspace too small */
#define DVG_E_UNSUPPORTED (-4) /* valid request this build cannot serve */

typedef void *dvg_stream_t; /* hipStream_t */

int dvg_version(void);
/* sha256 (first 16 hex digits) of the kernel sources this library was built from (csrc, include/dvg.h): profiles
 * under profiles/ carry the hash of the library they were measured on, bench.py drops the ones that do not match. */
const char *dvg_source_hash(void);
const char *dvg_last_error(void);

/* Device-resident per-step values, for steps replayed from a captured hipGraph.  A function handed a
 * non-NULL `dyn` (DEVICE pointer) reads these fields at run time instead of its by-value arguments of the
 * same meaning; the host rewrites the struct (one small async copy) before each replay.  NULL = by-value. */
typedef struct {
  uint32_t sweep0;         /* dvg_gibbs_sample: global index of the first sweep */
  uint32_t reserved;
  uint64_t gumbel_offset;  /* dvg_gumbel_fwd: Philox offset */
  uint64_t dropout_offset; /* dvg_decoder_fwd: Philox offset */
  float adam_step_size[2]; /* dvg_adam_step (slot 0 / 1): lr / (1 - beta1^t) */
  float adam_bc2_sqrt[2];  /*                              sqrt(1 - beta2^t) */
} dvg_step_state_t;

/* ------------------------------------------------------------------ graph
 * The GRBM graph as the sampler and the energy kernels need it.  Built on the
 * host by image-generation_amd/graphs.py::build_plan from what the reference
 * derives at /root/reference/src/utils/common.py:123-126 and hands to
 * GraphRestrictedBoltzmannMachine(nodes, edges)
 * (/root/reference/src/model_wrapper.py:202-206).  All arrays [host], int32.
 * The handle owns small device copies (the only allocation in this library).
 */
typedef struct dvg_graph dvg_graph_t;
int dvg_graph_create(int n, int n_edges, const int32_t *edge_i, const int32_t *edge_j,
                     const int32_t *order, const int32_t *class_ptr, int n_colours,
                     const int32_t *adj_ptr, const int32_t *adj_idx, const int32_t *adj_eid,
                     dvg_graph_t **out);
int dvg_graph_destroy(dvg_graph_t *g);

/* ------------------------------------------------------------------ sampler
 * Replaces the QPU draw `sampler.sample_ising(h, J, num_reads=...)` issued by
 * GraphRestrictedBoltzmannMachine.sample (/root/reference/src/model_wrapper.py:309-316,
 * :369-376; /root/reference/src/utils/persistent_qpu_sampler.py:71-78) with
 * `n_sweeps` sweeps of the graph-coloured block-Gibbs sampler defined in
 * oracle/gibbs.py, on `n_chains` chains with global ids chain_id0 ... .
 *   linear (n), quadratic (n_edges): raw GRBM parameters; the kernel applies
 *     hs = clamp(prefactor*h, h_lo, h_hi), Js = clamp(prefactor*J, j_lo, j_hi)
 *     (the plugin's to_ising) and samples p(s) ~ exp(-beta (hs.s + s.Js.s)).
 *   state (n_chains, n) int8 +-1: in/out (persistent chains).  init != 0 draws
 *     the start state from the INIT stream first, keyed by (spin, chain id, sweep0):
 *     chains restarted on every draw (non-persistent mode) start each draw elsewhere.
 *   samples_out (n_chains, n) float32 +-1, or NULL.
 *   sweep0: global index of the first sweep (keeps the random stream moving).
 */
int dvg_gibbs_sample(const dvg_graph_t *g, const float *linear, const float *quadratic,
                     float prefactor, float h_lo, float h_hi, float j_lo, float j_hi, float beta,
                     int8_t *state, int n_chains, uint32_t chain_id0, uint64_t seed,
                     uint32_t sweep0, int n_sweeps, int init, float *samples_out,
                     const dvg_step_state_t *dyn, dvg_stream_t stream);
/* The conditional draw: dvg_gibbs_sample with some spins of a chain HELD and the others redrawn from their conditionals
 * under the same (h, J).  By definition a held spin is left out of its colour class ("DVG block-Gibbs v1" keys every
 * random word by (spin, chain id, sweep), so nothing else moves): oracle/gibbs.py::gibbs_sweeps called with the held
 * spins filtered out of `order` / `class_ptr` is the draw, bit for bit.
 *   clamp: DEVICE pointer, uint8; a nonzero entry holds that spin of that chain.  clamp_chain_stride = n: one row of n
 *     flags per chain; = 0: one row shared by all chains; anything else, or clamp == NULL, is DVG_E_INVALID (a draw
 *     that holds nothing is dvg_gibbs_sample).
 *   A held spin keeps the value it has in `state` on entry, enters its neighbours' field sums as any spin does (same CSR
 *     order, same single-rounded adds) and is written back unchanged to `state` and `samples_out`.
 *   init != 0 draws the INIT-stream start value of the FREE spins only; held spins still come from `state`.
 *   For a free spin every operation and every Philox counter is dvg_gibbs_sample's; with no flag set the two agree bit
 *     for bit.  Every other argument as for dvg_gibbs_sample; a graph whose image does not fit the LDS with the flags
 *     beside it is DVG_E_UNSUPPORTED. */
int dvg_gibbs_sample_clamped(const dvg_graph_t *g, const float *linear, const float *quadratic,
                             float prefactor, float h_lo, float h_hi, float j_lo, float j_hi, float beta,
                             int8_t *state, int n_chains, uint32_t chain_id0, uint64_t seed,
                             uint32_t sweep0, int n_sweeps, int init,
                             const uint8_t *clamp, int64_t clamp_chain_stride, float *samples_out,
                             const dvg_step_state_t *dyn, dvg_stream_t stream);
/* The per-chain-field draw ("DVG field v1"): dvg_gibbs_sample with a linear field of its own per chain -- soft evidence,
 * where dvg_gibbs_sample_clamped is the hard kind: a chain is leaned towards a configuration, not nailed to it.  Chain c
 * samples the model whose linear vector is
 *     lin_c[i] = rn(linear[i] + fields[c * field_chain_stride + i])      one float32 add,
 * and everything behind that add is "DVG block-Gibbs v1" unchanged: hs_c[i] = clamp(rn(prefactor * lin_c[i]), h_lo, h_hi), the
 * CSR-order signed adds starting from hs_c[i], two_beta, spec_exp, the decision, the Philox counter (spin, chain id,
 * sweep >> 2, STREAM_GIBBS), the INIT stream.  So oracle/gibbs.py::gibbs_sweeps called once per chain with
 * scaled_fields(linear + fields[c], ...) and that chain's id is the draw, bit for bit.
 *   fields: DEVICE pointer, float32, in the raw units of `linear` (the prefactor and the range apply to the sum).
 *     field_chain_stride = n: one row of n entries per chain; = 0: one row shared by all chains; anything else, or
 *     fields == NULL, is DVG_E_INVALID (a draw without fields is dvg_gibbs_sample).  The values are NOT checked on the device: a
 *     field that is not finite gives that chain a draw without meaning, never an access out of bounds.
 *   With all fields zero the draw is dvg_gibbs_sample's, bit for bit; with stride 0 it is dvg_gibbs_sample's on
 *     rn(linear + row), bit for bit.  A chain's result is a function of its id, its row, the model and the graph alone: not
 *     of the other chains, not of the launch geometry.
 *   DVG_E_INVALID, before any launch: what dvg_gibbs_sample rejects; fields == NULL; a stride that is neither 0 nor n;
 *     dyn != NULL (the draw is one-off, not part of a captured step).  It takes the rolled kernel form on every graph
 *     (csrc/gibbs_plan.h), a float32 row of hs_c per chain beside the state rows in LDS -- workgroups of fewer chains on large
 *     graphs; DVG_E_UNSUPPORTED if the graph's image does not fit the LDS with one chain's rows beside it.  Every other argument as
 *     for dvg_gibbs_sample.  Its annealed and weighed form is dvg_gibbs_sample_fields_ais; no held, exchange or traced form of
 *     this draw. */
int dvg_gibbs_sample_fields(const dvg_graph_t *g, const float *linear, const float *quadratic,
                            float prefactor, float h_lo, float h_hi, float j_lo, float j_hi, float beta,
                            int8_t *state, int n_chains, uint32_t chain_id0, uint64_t seed,
                            uint32_t sweep0, int n_sweeps, int init,
                            const float *fields, int64_t field_chain_stride, float *samples_out,
                            const dvg_step_state_t *dyn, dvg_stream_t stream);
/* The annealed draw: dvg_gibbs_sample with beta looked up per sweep, and optionally per chain, as
 * neal.SimulatedAnnealingSampler's beta_range / num_sweeps / beta_schedule_type offer it.  Sweep k of the call (global
 * index sweep0 + k) on chain c runs at  beta = betas[c * beta_chain_stride + k];  everything else is "DVG block-Gibbs v1"
 * unchanged -- the field sum, z = clamp(rn(two_beta * f), -87, 87) with two_beta = 2 * beta (exact), spec_exp, the Philox
 * counter (spin, chain id, sweep >> 2, STREAM_GIBBS), the decision, the INIT stream.  So oracle/gibbs.py::gibbs_sweeps called
 * once per sweep (that sweep's beta, sweep0 + k, one sweep) on the chains that share a table row is the draw, bit for bit.
 *   betas: DEVICE pointer, float32.  beta_chain_stride = 0: one row of n_sweeps entries shared by all chains; = n_sweeps:
 *     a row per chain (temperature ladders: chains of one model at different temperatures in one launch); anything else,
 *     betas == NULL or n_sweeps < 1 is DVG_E_INVALID.  The values must be finite and >= 0; they are NOT checked on the
 *     device (beta = 0: every spin a fair coin).
 *   dyn: as for dvg_gibbs_sample (the sweep index comes from the device); the table index is always relative to the
 *     call's first sweep.
 *   Every other argument as for dvg_gibbs_sample; with every entry equal to `beta` the two agree bit for bit.  No
 *     annealed form of dvg_gibbs_sample_clamped. */
int dvg_gibbs_sample_annealed(const dvg_graph_t *g, const float *linear, const float *quadratic,
                              float prefactor, float h_lo, float h_hi, float j_lo, float j_hi,
                              const float *betas, int64_t beta_chain_stride,
                              int8_t *state, int n_chains, uint32_t chain_id0, uint64_t seed,
                              uint32_t sweep0, int n_sweeps, int init, float *samples_out,
                              const dvg_step_state_t *dyn, dvg_stream_t stream);
/* The AIS draw ("DVG AIS v1"): dvg_gibbs_sample_annealed with the same arguments -- its spins, random words and betas, bit
 * for bit -- plus, per chain, the log importance weight of annealed importance sampling and the energy of the returned
 * state, accumulated inside the kernel from the local fields the updates compute anyway.  With hs, Js the scaled, clamped
 * float32 fields, s^(k) the chain's state before sweep k of the call, beta_k = betas[c * beta_chain_stride + k] and
 * beta_{-1} = beta_from, everything below in float64 unless marked:
 *   f_i(s)   the float32 field exactly as v1 computes it (hs_i, then the CSR-order signed adds, each rounded);
 *   E_0      = sum_i 1/2 s_i (hs_i + f_i(s^(0)))  (each addend exact; with exact fields: sum hs_i s_i + sum_e Js_e s_i s_j);
 *   every update of spin i adds  (s_new - s_old) f_i,  f_i the float32 field the decision used (+-2 f_i or 0, exact);
 *   E^(k)    = E_0 plus the updates of sweeps 0 .. k-1;
 *   log_weight_out[c] = -sum_{k=0}^{n_sweeps-1} (beta_k - beta_{k-1}) E^(k)   (the differences of float32 values: exact);
 *   energy_out[c]     = E^(n_sweeps), the energy of the returned state (may be NULL).
 * Only the order of the float64 additions is the implementation's.  The estimate:  log Z(beta_last) ~= log Z(beta_from)
 * + logsumexp_c(log_weight) - log n_chains,  with log Z(0) = n log 2.  Fresh chains (init != 0) come from the INIT stream,
 * uniform +-1, which is the beta = 0 distribution and no other: init != 0 needs beta_from == 0.  DVG_E_INVALID, before any
 * launch: what dvg_gibbs_sample_annealed rejects, log_weight_out == NULL, init != 0 with beta_from != 0, beta_from negative
 * or not finite.  Both outputs are DEVICE pointers, float64, [n_chains].  No weighed form of dvg_gibbs_sample_clamped. */
int dvg_gibbs_sample_ais(const dvg_graph_t *g, const float *linear, const float *quadratic,
                         float prefactor, float h_lo, float h_hi, float j_lo, float j_hi,
                         const float *betas, int64_t beta_chain_stride, float beta_from,
                         int8_t *state, int n_chains, uint32_t chain_id0, uint64_t seed,
                         uint32_t sweep0, int n_sweeps, int init, float *samples_out,
                         double *log_weight_out, double *energy_out,
                         const dvg_step_state_t *dyn, dvg_stream_t stream);
/* The weighed per-chain-field draw ("DVG field AIS v1"): dvg_gibbs_sample_fields along a path in (beta, field strength), both
 * looked up per sweep, with the log importance weight and the energy of "DVG AIS v1" per chain.  The use: start from draws of the
 * prior, turn a chain's evidence on over the sweeps, weigh each step -- the weights of the chains that share a row estimate
 * log (Z_row / Z), the log evidence of that row under the prior, and the chains end as annealed posterior draws.
 *   Rows.  fields, field_chain_stride: as for dvg_gibbs_sample_fields, except that with field_chain_stride == n chain c reads
 *     row r = c / field_row_chains (R >= 1; c counts from 0 within the call): R consecutive chains share a row, which is stored
 *     once; fields then has ceil(n_chains / R) rows.  With stride 0 all chains read row 0 and R is ignored.
 *   Tables.  betas, beta_chain_stride, beta_from: as for dvg_gibbs_sample_ais (stride 0 or n_sweeps; finite and >= 0, not checked
 *     on the device).  scales: DEVICE pointer, float32, the field strength lambda of every sweep, or NULL: 1 throughout;
 *     scale_chain_stride = 0: one row of n_sweeps entries shared by all chains, = n_sweeps: a row per chain.  The values must be
 *     finite (not checked on the device).  scale_from: the strength the start states are a sample under.
 *   For chain c with row r and sweep k of the call (global index sweep0 + k), in float32:
 *     lambda_k  = scales ? scales[c * scale_chain_stride + k] : 1,     lambda_{-1} = scales ? scale_from : 1
 *     row_k[i]  = clamp(rn(prefactor * rn(linear[i] + rn(lambda_k * fields[r][i]))), h_lo, h_hi)
 *   Sweep k is one "DVG block-Gibbs v1" sweep at beta_k = betas[c * beta_chain_stride + k] with hs = row_k: the CSR-order signed
 *     adds starting from row_k[i], two_beta = 2 * beta_k, spec_exp, the decision, the Philox counter (spin, chain id,
 *     (sweep0 + k) >> 2, STREAM_GIBBS), the INIT stream.  With lambda == 1, row_k is hs_c of "DVG field v1", bit for bit.
 *   The energy is carried as in "DVG AIS v1": E = sum_i 1/2 s_i (row_{-1}[i] + f_i(s; row_{-1})) at the start, and every update
 *     adds (s_new - s_old) f_i, f_i the float32 field the decision used.  At the head of sweep k, with s the state before the
 *     sweep, in float64:
 *       d_k    = sum_i ((double)row_k[i] - (double)row_{k-1}[i]) * s_i           (each addend exact)
 *       log_w -= (beta_k - beta_{k-1}) * E  +  beta_k * d_k                      (beta_{-1} = beta_from)
 *       E     += d_k
 *     so that log_w = -sum_k [beta_k E_k(s^(k)) - beta_{k-1} E_{k-1}(s^(k))], E_k the energy under row_k: the AIS weight along
 *     any path in (beta, lambda).  With scales == NULL, d_k is identically 0 and is not computed.  Only the order of the float64
 *     additions is the implementation's.
 *   log_weight_out[c] = log_w, energy_out[c] = E behind the last sweep: DEVICE pointers, float64, [n_chains].  Either may be
 *     NULL; without log_weight_out this is the annealed per-chain-field draw, unweighed.
 *   The estimate, over the chains that share a row:  log Z(beta_last, lambda_last) - log Z(beta_from, scale_from) ~=
 *     logsumexp(log_w) - log(count).  Fresh chains (init != 0) are uniform: init != 0 needs beta_from == 0.
 *   With scales == NULL and every beta equal to beta_from the spins are dvg_gibbs_sample_fields' and log_w == 0 exactly; with
 *     all fields zero the spins, weights and energies are dvg_gibbs_sample_ais'.  A chain's result is a function of its id, its
 *     row, its table rows, the model and the graph alone.
 *   DVG_E_INVALID, before any launch (nothing is written): what dvg_gibbs_sample_fields and dvg_gibbs_sample_ais each reject
 *     (log_weight_out == NULL excepted); a scale stride that is neither 0 nor n_sweeps; field_row_chains < 1; scale_from not
 *     finite; dyn != NULL.  The kernel form and its LDS are dvg_gibbs_sample_fields' (csrc/gibbs_plan.h: GK_FIELD_WEIGH). */
int dvg_gibbs_sample_fields_ais(const dvg_graph_t *g, const float *linear, const float *quadratic,
                                float prefactor, float h_lo, float h_hi, float j_lo, float j_hi,
                                const float *betas, int64_t beta_chain_stride, float beta_from,
                                const float *scales, int64_t scale_chain_stride, float scale_from,
                                int8_t *state, int n_chains, uint32_t chain_id0, uint64_t seed,
                                uint32_t sweep0, int n_sweeps, int init,
                                const float *fields, int64_t field_chain_stride, int field_row_chains,
                                float *samples_out, double *log_weight_out, double *energy_out,
                                const dvg_step_state_t *dyn, dvg_stream_t stream);
/* The exchange draw ("DVG PT v1"): parallel tempering (replica exchange).  Chains of one model run side by side at the
 * inverse temperatures of a LADDER and, every few sweeps, chains on neighbouring rungs exchange their rungs on a Metropolis
 * coin, inside the kernel: the chain at the target beta keeps being fed states that crossed between modes where it is hot.
 *   Ladders, chains, rungs.  n_chains = Q * R: Q ladders of R = n_replicas consecutive chains; chain c belongs to ladder
 *     q = c / R and has id chain_id0 + c.  ladder: DEVICE pointer, float32 [R], beta of rung r (ascending is usual, not
 *     required, not checked; finite and >= 0, not checked).  A chain keeps its state row and its id for the whole draw; what
 *     moves between chains is the rung.  rung: DEVICE pointer, int32 [n_chains], in/out, values 0 .. R-1, a permutation
 *     within each ladder (values outside are clamped into the range; anything but a permutation gives a draw without
 *     meaning, never an access out of bounds).  init != 0: the start state comes from the INIT stream as in every draw, and
 *     the kernel writes rung[c] = c % R, ignoring the input.
 *   Sweeps and energies.  Sweep k of the call has global index t = sweep0 + k and is a v1 sweep of chain c at
 *     beta = ladder[rung[c]] (two_beta = 2 * beta) -- what dvg_gibbs_sample_annealed does with that value in the chain's row,
 *     same Philox counters (spin, chain id, t >> 2, STREAM_GIBBS).  Each chain carries the energy E_c of "DVG AIS v1" in
 *     float64: the start walk sum_i 1/2 s_i (hs_i + f_i), then (s_new - s_old) f_i per update.
 *   Exchanges.  After sweep t, if (t + 1) % swap_every == 0, exchange number x = (t + 1) / swap_every takes place: in every
 *     ladder q, for r = x & 1, (x & 1) + 2, ... while r + 1 < R, with a the chain holding rung r and b the chain holding r + 1,
 *       d    = ((double)ladder[r+1] - (double)ladder[r]) * (E_b - E_a)     float64: two subtractions, one product;
 *       word = philox4x32_10(ctr = (r, chain_id0 + q R, x, STREAM_SWAP = 4), key = seed).x,  u = (word >> 8) 2^-24;
 *       accept iff d >= 0 or u < exp(d) (float64 exp); on accept a takes rung r + 1 and b takes rung r.
 *     The pairs of one exchange are disjoint: their order does not matter.  Only the order of the float64 additions of an
 *     energy, and the last bit of exp, are the implementation's.
 *   Outputs.  state and rung are stored BY CHAIN, so that a later call continues the draw; samples_out (n_chains, n) float32
 *     and energy_out [n_chains] float64 BY RUNG: row / element q R + rung[c] is chain c's final state and its energy;
 *     accept_out [n_chains] uint32: element q R + r = the accepted exchanges of the pair (r, r + 1) of ladder q in this call
 *     (written, not added to; element q R + R - 1 is 0).  samples_out, energy_out and accept_out may each be NULL.
 *   Continuation.  A call of S sweeps, and two calls of S1 + S2 = S sweeps that hand state and rung on with sweep0 advanced
 *     by S1, are the same draw but for the second call's start energies, summed afresh: the same spins and rungs whenever no
 *     acceptance is a near tie.
 *   DVG_E_INVALID, before any launch: what dvg_gibbs_sample rejects, ladder == NULL, rung == NULL, n_replicas outside 2..16,
 *     n_chains not a multiple of n_replicas, swap_every < 1, n_sweeps < 1, dyn != NULL (the draw is one-off, not part of a
 *     captured step: the workgroup barriers of its exchanges are counted from the host's sweep0).  A workgroup holds whole
 *     ladders; DVG_E_UNSUPPORTED if the graph's image with the exchange's mailboxes beside it exceeds the LDS.  No exchange
 *     form of dvg_gibbs_sample_clamped. */
int dvg_gibbs_sample_tempered(const dvg_graph_t *g, const float *linear, const float *quadratic,
                              float prefactor, float h_lo, float h_hi, float j_lo, float j_hi,
                              const float *ladder, int n_replicas, int swap_every,
                              int8_t *state, int32_t *rung, int n_chains, uint32_t chain_id0, uint64_t seed,
                              uint32_t sweep0, int n_sweeps, int init, float *samples_out,
                              double *energy_out, uint32_t *accept_out,
                              const dvg_step_state_t *dyn, dvg_stream_t stream);
/* The traced draw ("DVG trace v1"): dvg_gibbs_sample with a history of the chains written from inside the kernel.  The
 * spins, the random words, the INIT stream, state and samples_out are dvg_gibbs_sample's with the same arguments, bit for
 * bit; the chains' states after chosen sweeps are written out as well, one BIT per spin.
 *   Which sweeps are recorded.  Sweep k of the call is 0-based and has global index sweep0 + k.  It is recorded, after its
 *     last colour class, iff  k + 1 > burn_in  and  (k + 1 - burn_in) % thin == 0.
 *   Number of records.  M = (n_sweeps - burn_in) / thin, rounded down; record m (0 .. M-1) holds the state after sweep
 *     k = burn_in + thin (m + 1) - 1.  The last sweep of the call is recorded iff (n_sweeps - burn_in) % thin == 0.
 *   Layout.  W = (n + 31) / 32 words per record;  trace_out[(c M + m) W + w]  holds the packed spins of chain c at record m:
 *     bit b of word w is 1 iff spin 32 w + b is +1; bits of spins >= n are 0.  trace_out: DEVICE pointer, uint32,
 *     n_chains M W words; nothing is written beyond it.  dvg_grbm_moments_packed sums moments over such rows.
 *   Continuation.  The record rule counts from the call's first sweep: two calls of S1 + S2 sweeps that hand `state` on with
 *     sweep0 advanced by S1 record, at burn_in = 0 and thin = 1, what one call of S1 + S2 sweeps records.
 *   DVG_E_INVALID, before any launch: what dvg_gibbs_sample rejects; trace_out == NULL; burn_in < 0; thin < 1; M < 1 (a draw
 *     that records nothing is dvg_gibbs_sample); dyn != NULL (the draw is one-off, not part of a captured step: the recorded
 *     sweeps are counted from the host's sweep0).  It takes the kernel forms of the annealed draw (csrc/gibbs_plan.h) and
 *     their LDS: a record is packed from the state rows where they lie.  The traced form of dvg_gibbs_sample_tempered is
 *     dvg_gibbs_sample_tempered_traced; no traced form of dvg_gibbs_sample_clamped, _annealed or _ais. */
int dvg_gibbs_sample_traced(const dvg_graph_t *g, const float *linear, const float *quadratic,
                            float prefactor, float h_lo, float h_hi, float j_lo, float j_hi, float beta,
                            int8_t *state, int n_chains, uint32_t chain_id0, uint64_t seed,
                            uint32_t sweep0, int n_sweeps, int init, float *samples_out,
                            uint32_t *trace_out, int burn_in, int thin,
                            const dvg_step_state_t *dyn, dvg_stream_t stream);
/* The traced exchange draw ("DVG PT trace v1"): dvg_gibbs_sample_tempered with a history of the LADDER written from inside
 * the kernel -- per rung the state and the energy of the chain holding it, per chain the rung it holds.  With the same
 * arguments the spins, the random words, the exchanges, state, rung, samples_out, energy_out and accept_out are "DVG PT v1"'s,
 * bit for bit: the records add nothing to any decision.
 *   Which sweeps are recorded.  The rule of "DVG trace v1": sweep k of the call (0-based, global index sweep0 + k) iff
 *     k + 1 > burn_in  and  (k + 1 - burn_in) % thin == 0;  M = (n_sweeps - burn_in) / thin records, rounded down; record m
 *     belongs to sweep k = burn_in + thin (m + 1) - 1.
 *   When the record is taken.  After the sweep's last colour class AND after the exchange that follows that sweep, if one is
 *     due ((sweep0 + k + 1) % swap_every == 0): a record shows who holds each rung as the next sweep will find it.  When the
 *     call's last sweep is recorded ((n_sweeps - burn_in) % thin == 0), the last record is samples_out packed, its energies
 *     are energy_out and its rungs are rung on exit.
 *   Layout.  W = (n + 31) / 32; ladder q = c / R, j = c % R, R = n_replicas.  All three are DEVICE pointers; nothing is
 *     written beyond the sizes given.
 *       trace_out[((q R + r) M + m) W + w]   uint32, n_chains M W words, BY RUNG: the packed state, at record m, of the chain
 *         of ladder q that holds rung r then -- bit b of word w is 1 iff spin 32 w + b is +1, bits of spins >= n are 0.  As
 *         (Q, R, M, W), [:, R-1] is the history of the target: at every record a sample at ladder[R-1].
 *       energy_trace_out[(q R + r) M + m]    float64, n_chains M, BY RUNG: that chain's carried energy E_c ("DVG PT v1": the
 *         start walk plus (s_new - s_old) f_i per update) at record m.  May be NULL.
 *       rung_trace_out[c M + m]              uint8, n_chains M, BY CHAIN: the rung chain c holds at record m.  May be NULL.
 *     Only the order of the float64 additions of a recorded energy is the implementation's (it sums a copy of the chain's
 *     partial sums: the carried energy itself goes on unchanged).
 *   Continuation.  As "DVG PT v1"; the record rule counts from the call's first sweep: two calls of S1 + S2 sweeps that hand
 *     state and rung on with sweep0 advanced by S1 record, at burn_in = 0 and thin = 1, what one call of S1 + S2 sweeps
 *     records -- but for the second call's start energies, summed afresh.
 *   DVG_E_INVALID, before any launch: what dvg_gibbs_sample_tempered rejects (dyn != NULL included); trace_out == NULL (a
 *     draw that records nothing is dvg_gibbs_sample_tempered); burn_in < 0; thin < 1; M < 1.  DVG_E_UNSUPPORTED as the exchange
 *     draw: it takes that draw's plan, kernel forms and LDS unchanged -- a record is packed from the chain's own state row and
 *     registers, behind the exchange's barrier, and adds no barrier.  A rejected call writes nothing. */
int dvg_gibbs_sample_tempered_traced(const dvg_graph_t *g, const float *linear, const float *quadratic,
                                     float prefactor, float h_lo, float h_hi, float j_lo, float j_hi,
                                     const float *ladder, int n_replicas, int swap_every,
                                     int8_t *state, int32_t *rung, int n_chains, uint32_t chain_id0, uint64_t seed,
                                     uint32_t sweep0, int n_sweeps, int init, float *samples_out,
                                     double *energy_out, uint32_t *accept_out,
                                     uint32_t *trace_out, double *energy_trace_out, uint8_t *rung_trace_out, int burn_in, int thin,
                                     const dvg_step_state_t *dyn, dvg_stream_t stream);
/* The simulated-quantum-annealing draw ("DVG SQA v1"): path-integral (Trotter-slice) Monte Carlo of the transverse-field Ising
 * model, the closest classical stand-in for a quantum annealer's read.  A chain is P = n_slices copies ("slices") of the n
 * spins, s[k][i] = +-1; P is a power of two, 2 <= P <= 64; the slices are periodic, the neighbours of slice k are (k +- 1) mod P
 * (for P = 2 the other slice counts twice).  With hs, Js the scaled, clamped float32 fields of dvg_gibbs_sample, sweep q of the
 * call reads two float32 numbers from DEVICE tables shared by all chains:
 *   beta_slice[q] >= 0  multiplies the classical energy of every slice (beta / P times whatever ramp the caller wants);
 *   kappa[q] >= 0       the dimensionless ferromagnetic coupling between neighbouring slices of the same spin,
 *                       -1/2 ln tanh(beta Gamma_q / P) for a transverse field Gamma_q.
 * One sweep at fixed tables is Gibbs sampling of
 *   p(s) ~ exp(-beta_slice sum_k E(s[k]) + kappa sum_k sum_i s[k][i] s[k+1][i]),   E(s) = hs.s + sum_e Js_e s_i s_j.
 * The decision for site (i, k) of chain id c in global sweep t = sweep0 + q; every operation float32, round to nearest, no
 * contraction:
 *   f   the v1 local field of spin i in slice k: hs_i, then for each entry of spin i's CSR row in row order rn(f +- Js);
 *   nb  = s[k-1][i] + s[k+1][i], in {-2, 0, 2};
 *   z0  = rn(rn(beta_slice[q] f) - rn(kappa[q] nb));   z = clamp(rn(2 z0), -87, 87);   tt = spec_exp(z);
 *   u   = u32_to_unit(w),  w = word .x of philox4x32_10(i, c, t, STREAM_SQA | (k << 8), key = seed),  STREAM_SQA = 6 -- the
 *         full sweep index, not t >> 2;
 *   s[k][i] = +1  iff  rn(u rn(1 + tt)) < 1   (the last two lines of v1's decision, unchanged).
 * Order inside a sweep: for colour class 0 .. n_colours - 1, first every (i in the class, k even), then every (i in the class,
 * k odd); each such set is an independent set of the product graph, so together equals one after another.  f does not depend
 * on spin i's other slices: one sum serves both half-steps.
 * Start state with init != 0: s[k][i] = +1 iff bit 31 of philox4x32_10(i, c, sweep0, STREAM_INIT | (k << 8)).x is set -- slice
 * 0 is dvg_gibbs_sample's start state; otherwise the chains start from `slices` as given.
 *   slices: DEVICE, in/out, [n_chains][n_slices][W = (n + 31) / 32] uint32 in the layout of "DVG trace v1" (bit b of word w = spin
 *     32 w + b is +1): packed rows with groups = n_chains, rows = n_slices for every packed-row entry below.  Bits of spins >= n
 *     are ignored on input and written as 0.
 *   samples_out: DEVICE, [n_chains][n] float32 +-1, slice 0 of every chain, or NULL.
 *   Chain ids are chain_id0 + 0 .. n_chains - 1.  A chain's result is a function of its id, the tables, the fields and the
 *   graph alone, never of the other chains or of how chains are placed on workgroups.
 * DVG_E_INVALID, before any HIP call: g, linear, quadratic, beta_slice, kappa or slices null; n_chains < 1; n_sweeps < 1;
 * n_slices not a power of two in 2 .. 64; a non-finite prefactor.  DVG_E_UNSUPPORTED: n > 8192 (a tile's bit columns are kept
 * in 64 KiB of LDS); n_chains n_slices >= 2^31.  A rejected call writes nothing.  The table values are NOT checked on the
 * device.  No dyn: the draw is not part of a captured training step.  The call enqueues on `stream`, allocates nothing and
 * uses no atomics. */
int dvg_gibbs_sample_quantum(const dvg_graph_t *g, const float *linear, const float *quadratic,
                             float prefactor, float h_lo, float h_hi, float j_lo, float j_hi,
                             const float *beta_slice, const float *kappa,
                             uint32_t *slices, int n_chains, int n_slices, uint32_t chain_id0, uint64_t seed,
                             uint32_t sweep0, int n_sweeps, int init, float *samples_out, dvg_stream_t stream);
/* The isoenergetic cluster move ("DVG ICM v1"): Houdayer's move on any topology (Zhu, Ochoa, Katzgraber 2015).  Two replicas at
 * the same temperature exchange their spins on one connected cluster of the sites where they disagree: the pair's total
 * energy does not change, so the move has no acceptance test, and it carries whole domains from one replica to the other.
 * Integers only: spins, the graph, one Philox word.
 *   Layout.  state (n_chains, n) int8 +-1, DEVICE, changed in place, and rung [n_chains] int32, DEVICE, read only, both BY
 *     CHAIN as "DVG PT v1" hands them on; R = n_replicas; ladder q = chains q R .. q R + R - 1.  Ladders 2p and 2p + 1 are
 *     TWINS: their chain ids differ, so they are independent draws of the same ladder.  n_replicas == 1 with rung == NULL:
 *     chains 2p and 2p + 1 are twins and both hold rung 0.
 *   Holder.  The holder of rung r in a ladder is its lowest-numbered chain whose rung, clamped into 0 .. R-1, equals r.  A
 *     ladder without a holder for r: the job (p, r) does nothing and reports 0, 0.  Distinct r give distinct chains whatever
 *     the table holds; nothing is read or written out of bounds.
 *   Job.  For every twin pair p = 0 .. n_chains / (2 R) - 1 and every rung r with rung_from <= r < R, with a the holder in
 *     ladder 2p and b the holder in ladder 2p + 1:
 *       D    = { i : state[a][i] < 0  differs from  state[b][i] < 0 }, in ascending spin order;  k = |D|;
 *              differ_out[p R + r] = k;  k == 0: nothing moves, size_out[p R + r] = 0;  otherwise
 *       word = philox4x32_10(ctr = (r, chain_id0 + 2 p R, move, STREAM_ICM = 7), key = seed).x   (the id mod 2^32);
 *       root = element number ((uint64)word * k) >> 32 of D;
 *       the cluster = the connected component of root in the subgraph of g induced on D -- every edge of the graph counts,
 *              whatever its coupling;
 *       for every i of the cluster state[a][i] and state[b][i] change places (both change sign there);
 *       size_out[p R + r] = the size of the cluster.
 *     Elements with r < rung_from are written as 0.  size_out, differ_out: DEVICE, uint32 [n_chains / 2], each may be NULL.
 *   What follows: D is the same before and after the move; the same call again with the same `move` restores state;
 *     E(a) + E(b) is unchanged for any (h, J) on this graph.  Energies are no argument: "DVG PT v1" sums a chain's start
 *     energy afresh at every call.
 * DVG_E_INVALID, before any HIP call: g or state null; n_replicas outside 1 .. 16; rung null with n_replicas > 1;
 * n_chains < 2 or not a multiple of 2 n_replicas; rung_from outside 0 .. R-1.  DVG_E_UNSUPPORTED: n > 65536 (a job's two bit
 * sets, D and the cluster, are kept in 16 KiB of LDS).  A rejected call writes nothing.  One stream-ordered launch on `stream`,
 * no allocation, no atomics, no workgroup waiting on another; a job's result is a function of that job alone. */
int dvg_gibbs_cluster_move(const dvg_graph_t *g, int8_t *state, const int32_t *rung, int n_chains,
                           int n_replicas, int rung_from, uint32_t chain_id0, uint64_t seed, uint32_t move,
                           uint32_t *size_out, uint32_t *differ_out, dvg_stream_t stream);
/* The launch geometry dvg_gibbs_sample uses for n_chains chains on this graph (nothing is launched; any out pointer may
 * be NULL): workgroups, threads per workgroup, LDS bytes per workgroup.  For callers that size what runs BESIDE the draw
 * (tools and A/B measurements; since round 5 the Winograd grids beside the draw deal their tile blocks dynamically and
 * no caller needs it on the product path; the reference has no counterpart -- its draw is a QPU call,
 * /root/reference/src/model_wrapper.py:309-316). */
int dvg_gibbs_launch_info(const dvg_graph_t *g, int n_chains, int *workgroups, int *threads, size_t *lds_bytes);

/* ------------------------------------------------------------------ GRBM
 * Energy  E(x) = x.h + sum_e J_e x_i x_j  per row: the plugin's
 * GraphRestrictedBoltzmannMachine.__call__ as used by nll_loss
 * (/root/reference/src/losses.py:61).  x (rows, n) float32.
 */
int dvg_grbm_energy(const dvg_graph_t *g, const float *x, int64_t rows, const float *linear,
                    const float *quadratic, float *energy_out, dvg_stream_t stream);
/* Backward of the energy = weighted sufficient statistics:
 *   acc_linear[i]    (+)= scale * sum_r w_r x_ri ;
 *   acc_quadratic[e] (+)= scale * sum_r w_r x_ri x_rj      (w_r = 1 when row_weight is NULL).
 * accumulate == 0 overwrites.  With w = 1, scale = 1/rows this is the data (or, negated, the
 * model) half of the quasi-NLL gradient of /root/reference/src/losses.py:61.  Deterministic
 * (fixed-order two-stage reduction in double).  ws: dvg_grbm_suffstats_workspace_bytes(g). */
size_t dvg_grbm_suffstats_workspace_bytes(const dvg_graph_t *g);
int dvg_grbm_suffstats(const dvg_graph_t *g, const float *x, int64_t rows, const float *row_weight,
                       float scale, float *acc_linear, float *acc_quadratic, int accumulate,
                       void *ws, size_t ws_bytes, dvg_stream_t stream);
/* Moments of bit-packed spin rows, exactly: bits (rows, W = (n + 31) / 32) uint32 in the layout of dvg_gibbs_sample_traced
 * (bit b of word w of a row = spin 32 w + b is +1; bits of spins >= n are ignored and may hold anything).
 *   spin_sum[i] (+)= sum_r s_ri ;   pair_sum[e] (+)= sum_r s_ri s_rj   over the graph's edge list (i, j) = (edge_i[e], edge_j[e]).
 * Both outputs are DEVICE pointers, int64, [n] and [n_edges]; the sums are exact integers (popcounts of bit columns:
 * sum_r s_i = T - 2 popc(~col_i), sum_r s_i s_j = T - 2 popc(col_i ^ col_j) over T rows), combined with integer atomics:
 * deterministic.  accumulate == 0 overwrites.  The rows are never unpacked: n / 8 bytes of traffic per row.
 * DVG_E_INVALID: a null pointer, rows < 1.  DVG_E_UNSUPPORTED: n > 8192 (a tile's bit columns are kept in 64 KiB of LDS). */
int dvg_grbm_moments_packed(const dvg_graph_t *g, const uint32_t *bits, int64_t rows,
                            int64_t *spin_sum, int64_t *pair_sum, int accumulate, dvg_stream_t stream);
/* Energies of bit-packed spin rows in float64 ("DVG energy v1"), under the fields every draw uses.  Rows are packed as in
 * "DVG trace v1": W = (n + 31) / 32 words, bit b of word w = spin 32 w + b is +1; bits of spins >= n are ignored and may hold
 * anything.  Strides count words, as in dvg_packed_overlap: row r of group g starts at bits + g group_stride + r row_stride.  A
 * flat set is groups = 1, row_stride = W; a trace (C, M, W) is groups = C, group_stride = M W, rows = M, row_stride = W; slices
 * of either need no copy.
 *   Fields.  hs_i = clamp(rn(prefactor linear_i), h_lo, h_hi),  Js_e = clamp(rn(prefactor quadratic_e), j_lo, j_hi)  in float32,
 *     one rounding each: what dvg_gibbs_sample and its kin draw from (oracle/gibbs.py::scaled_fields).  prefactor = 1 with
 *     infinite clamps gives the raw GRBM energy of dvg_grbm_energy.
 *   Value.  energy_out[g rows + r] = sum_i (double)hs_i s_i + sum_e (double)Js_e s_i s_j  over the graph's edge list (i, j) =
 *     (edge_i[e], edge_j[e]), s = +-1 the row's spins.  Every addend is exact in float64; only the order of the float64
 *     additions is the implementation's, and it is fixed by (n, n_edges) alone: no floating-point atomics, two calls on the
 *     same input return the same bits.  energy_out: DEVICE pointer, float64, groups rows elements; nothing is written beyond.
 * linear [n], quadratic [n_edges] and bits are DEVICE pointers.  The call enqueues on `stream`, allocates nothing and needs no
 * workspace.  The rows are never unpacked: n / 8 bytes of traffic per row.
 * DVG_E_INVALID, before any HIP call: g, linear, quadratic, bits or energy_out null; rows < 1; groups < 1; row_stride < W;
 * group_stride < 0; a non-finite prefactor.  DVG_E_UNSUPPORTED: groups rows >= 2^62; n > 8192 (a tile's bit columns are kept
 * in 64 KiB of LDS, beside 8 KiB of partial sums). */
int dvg_grbm_energy_packed(const dvg_graph_t *g, const float *linear, const float *quadratic,
                           float prefactor, float h_lo, float h_hi, float j_lo, float j_hi,
                           const uint32_t *bits, int64_t rows, int64_t row_stride,
                           int64_t groups, int64_t group_stride,
                           double *energy_out, dvg_stream_t stream);
/* Local fields of bit-packed spin rows and the per-spin statistics built on them ("DVG fields v1"): the pseudo-log-likelihood
 * of a row, its number of unstable spins, the Rao-Blackwellised moment sums and the fields themselves.  Rows are packed as in
 * "DVG trace v1" and addressed by (rows, row_stride, groups, group_stride) in words exactly as in dvg_grbm_energy_packed; T =
 * groups rows, row r of group g has the flat index t = g rows + r.
 *   Fields.  hs, Js: the scaled, clamped float32 fields of "DVG energy v1" (oracle/gibbs.py::scaled_fields).
 *   Local field.  The sampler's, bit for bit ("DVG block-Gibbs v1"): in float32 f = hs_i, then for each entry of spin i's CSR
 *     row in row order f = rn(f + (s_j > 0 ? Js : -Js)); an isolated spin has f = hs_i.
 *   Logit.  z = clamp(rn(two_beta f), -87, 87), two_beta = rn(2 beta) in float32: what the Gibbs update feeds to spec_exp.
 *   Per spin, in float64 from (double)z and s = s_i:  a = s z;  nlp = max(a, 0) + log1p(exp(-|a|)) = -log P(s_i | rest);
 *     e = exp(-|z|);  m = -sign(z) (1 - e) / (1 + e) = E[s_i | rest], m = 0 at z = 0.  A spin is UNSTABLE iff s_i f > 0 in
 *     float32 (the flip lowers the energy by 2 s_i f); f = 0 is stable.
 *   Outputs, all DEVICE pointers, each of the four optional (NULL), at least one given:
 *     log_pl[T]      float64: -sum_i nlp of the row
 *     unstable[T]    int32: the row's number of unstable spins; 0 = a local minimum of the energy
 *     cond_sum[n], cond_pair[n_edges]   float64, given together or not at all: cond_sum[i] (+)= sum_r m_ri, cond_pair[e] (+)=
 *                    sum_r (m_ri s_rj + m_rj s_ri) for (i, j) = (edge_i[e], edge_j[e]); accumulate == 0 overwrites both, 1
 *                    adds the call's sums onto their contents (one addition per element)
 *     field_out[T n] float32: the local fields, row-major
 *   The pseudo-likelihood's residual sums follow from these and the exact integers of dvg_grbm_moments_packed: sum_r (s_i - m_i)
 *   = spin_sum_i - cond_sum_i, and 2 pair_sum_e - cond_pair_e for an edge; they are not returned separately.
 *   Determinism.  No floating-point atomics; the order of every float64 addition is fixed by (n, n_edges, rows, groups) alone
 *   -- a row's nlp in a fixed order of its spins, the pooled sums row by row inside a slab of rows and then slab by slab, the
 *   split into at most 512 slabs a function of T alone -- never by the device's CU count or arrival order: two calls return
 *   the same bits.  Nothing is written beyond the sizes above.
 *   ws: DEVICE memory aligned to 16 bytes, dvg_grbm_fields_packed_workspace_bytes(g, rows, groups) bytes, needed for the pooled
 *       sums only (otherwise ignored, may be NULL): min(ceil(T / 64), 512) slabs of n + 2 n_edges float64 partial sums, reduced
 *       in slab order by a second kernel.  The query is monotone in rows and groups and 0 for arguments the entry rejects.
 * linear [n], quadratic [n_edges] and bits are DEVICE pointers; the call enqueues on `stream` and allocates nothing.
 * DVG_E_INVALID, before any HIP call: g, linear, quadratic or bits null; no output requested; cond_sum without cond_pair or the
 * reverse; ws null or not aligned to 16 bytes when the pooled sums are asked for; rows < 1; groups < 1; row_stride < W;
 * group_stride < 0; a non-finite prefactor; beta not finite or < 0.  DVG_E_UNSUPPORTED: groups rows >= 2^62; n > 8192 (a tile's
 * bit columns are kept in 64 KiB of LDS).  DVG_E_WORKSPACE: ws_bytes below the query.  A rejected call writes nothing. */
size_t dvg_grbm_fields_packed_workspace_bytes(const dvg_graph_t *g, int64_t rows, int64_t groups);
int dvg_grbm_fields_packed(const dvg_graph_t *g, const float *linear, const float *quadratic,
                           float prefactor, float h_lo, float h_hi, float j_lo, float j_hi, float beta,
                           const uint32_t *bits, int64_t rows, int64_t row_stride,
                           int64_t groups, int64_t group_stride,
                           double *log_pl, int32_t *unstable, double *cond_sum, double *cond_pair,
                           float *field_out, int accumulate,
                           void *ws, size_t ws_bytes, dvg_stream_t stream);
/* Zero-temperature descent of bit-packed spin rows to local minima of the energy ("DVG descent v1"): what takes the rows that
 * dvg_grbm_fields_packed counts unstable spins in to a row without any.  Rows are packed as in "DVG trace v1" and addressed by
 * (rows, row_stride, groups, group_stride) in words exactly as in dvg_grbm_energy_packed; T = groups rows, row r of group g has
 * the flat index t = g rows + r.  Bits of spins >= n in the input are ignored.
 *   Fields.  hs, Js: the scaled, clamped float32 fields of "DVG energy v1" (oracle/gibbs.py::scaled_fields).
 *   Local field.  The sampler's, bit for bit: in float32 f = hs_i, then for each entry of spin i's CSR row in row order
 *     f = rn(f + (s_j > 0 ? Js : -Js)), no contraction; an isolated spin has f = hs_i.
 *   Unstable.  A spin is unstable iff s_i f_i > 0 in float32; f_i = 0 is stable: the rule of "DVG fields v1".
 *   Sweep.  The colour classes k = 0 .. n_colours - 1 in the graph's order (order, class_ptr); in class k every unstable spin
 *     of the class flips.  A class is an independent set, so flipping together equals flipping one after another in `order`.
 *   A row runs sweeps 1, 2, .. until a sweep flips none of its spins -- the row is then a fixed point of the rule -- or
 *   max_sweeps sweeps have run.  A row's result is a function of that row, the fields and the graph alone: never of the other
 *   rows, their number, or how rows are placed on workgroups.  The rule has no randomness and no floating-point sum across
 *   rows; two calls return the same bits.
 *   Outputs, DEVICE pointers:
 *     bits_out[T W]  required, dense: the final rows; bits of spins >= n are written as 0
 *     sweeps[T]      int32, optional (NULL): the number of sweeps in which the row flipped at least one spin -- the first
 *                    sweeps[t] sweeps; a row that starts at a minimum gets 0
 *     flips[T]       int32, optional: the row's flips in all; a spin may flip in more than one sweep, so this can exceed the
 *                    Hamming distance moved
 *     unstable[T]    int32, optional: the unstable spins of the returned row as dvg_grbm_fields_packed counts them; 0 =
 *                    converged; non-zero only where sweeps[t] == max_sweeps (a row whose last permitted sweep still flipped
 *                    something is given one more field pass without flips; that pass runs only then)
 *   In place: bits_out == bits is allowed when the input is itself dense (row_stride == W, and groups == 1 or group_stride ==
 *   rows W).
 *   Termination.  A flip lowers the exact energy by 2 s_i F_i, F_i the exact field; the rule tests the rounded f_i, and the
 *   two can differ in sign only below float32 rounding of the field.  So the energy falls strictly with every flip whenever the
 *   float32 sums are exact (fields on a coarse binary grid), and every row then ends at a fixed point; otherwise a monotone
 *   energy is NOT promised and the descent is merely capped by max_sweeps.
 * linear [n], quadratic [n_edges] and bits are DEVICE pointers.  The call enqueues on `stream`, allocates nothing, takes no
 * workspace and uses no atomics on global memory.
 * DVG_E_INVALID, before any HIP call: g, linear, quadratic, bits or bits_out null; rows < 1; groups < 1; row_stride < W;
 * group_stride < 0; a non-finite prefactor; max_sweeps outside 1 .. 65536 (with n <= 8192 a flip count then fits an int32); the
 * input's word range overlapping bits_out in any way other than the exact alias above.  DVG_E_UNSUPPORTED: groups rows >= 2^62;
 * n > 8192 (a tile's bit columns are kept in 64 KiB of LDS).  A rejected call writes nothing. */
int dvg_grbm_descend_packed(const dvg_graph_t *g, const float *linear, const float *quadratic,
                            float prefactor, float h_lo, float h_hi, float j_lo, float j_hi,
                            const uint32_t *bits, int64_t rows, int64_t row_stride,
                            int64_t groups, int64_t group_stride,
                            int max_sweeps, uint32_t *bits_out, int32_t *sweeps, int32_t *flips, int32_t *unstable,
                            dvg_stream_t stream);
/* Autocorrelation sums of a bit-packed trace, exactly ("DVG acf v1"): bits (n_chains C, n_records M, W = (n + 31) / 32)
 * uint32 in the layout of "DVG trace v1" (bit b of word w = spin 32 w + b is +1; bits of spins >= n are ignored and may hold
 * anything).  With s_i(c, m) = +-1 the spin of chain c at record m, and L = max_lag:
 *   lag_sum[t n + i]   (+)= sum_c sum_{m = 0}^{M - 1 - t} s_i(c, m) s_i(c, m + t)   for t = 0 .. L, i < n;  lag_sum[0][i] = C M
 *   spin_sum[i]        (+)= sum_c sum_m s_i(c, m)
 *   chain_sum[c n + i]   = sum_m s_i(c, m)      int32; optional (NULL: not written); always overwritten, never accumulated
 * All three are DEVICE pointers; lag_sum and spin_sum are int64.  accumulate == 0 overwrites them, 1 adds onto them (pooling
 * several traces).  Every value is an exact integer: a chain's records are transposed into one M-bit time column per spin
 * and  sum_m s(m) s(m + t) = (M - t) - 2 popc((x ^ (x >> t)) & low(M - t));  workgroups combine through integer atomics only,
 * so the result is deterministic.  Nothing is written beyond (L + 1) n, n and C n elements.  The entry needs n only, no graph.
 * DVG_E_INVALID, before any HIP call: bits, lag_sum or spin_sum null; n_chains, n_records or n < 1; max_lag < 0 or
 * max_lag >= n_records.  DVG_E_UNSUPPORTED: n_records > 16384 (the time columns of 32 spins are kept in 64 KiB of LDS);
 * C M W beyond what one launch indexes. */
int dvg_trace_autocorr(const uint32_t *bits, int n_chains, int n_records, int n, int max_lag,
                       int64_t *lag_sum, int64_t *spin_sum, int32_t *chain_sum,
                       int accumulate, dvg_stream_t stream);
/* Hamming distances between bit-packed spin rows, exactly ("DVG overlap v1"): their histogram -- the overlap distribution
 * P(q), q = 1 - 2 d / n -- and every row's nearest partner.  Rows are packed as in "DVG trace v1": W = (n + 31) / 32 words,
 * bit b of word w = spin 32 w + b is +1; bits of spins >= n are ignored and may hold anything.  Strides count words: row r
 * of group g of A starts at a + g a_group_stride + r a_row_stride, B likewise.  A flat set is groups = 1, row_stride = W; a
 * trace (C, M, W) at equal times is rows = C, row_stride = M W, groups = M, group_stride = W; b_group_stride = 0 compares
 * every group of A with one shared B.  d(x, y) = popc((x ^ y) over the spins < n).
 *   cross mode (b != NULL): in every group all rows_a rows_b pairs (row of A, row of B);
 *   self mode  (b == NULL): in every group the rows_a (rows_a - 1) / 2 unordered pairs r < r' of A, never the diagonal;
 *                           rows_b and the strides of B are ignored.
 *   hist[d] (+)= the number of pairs at distance d, d = 0 .. n, summed over the groups; int64 [n + 1]; accumulate == 0
 *              overwrites, 1 adds onto it (pooling calls)
 *   nearest[g rows_a + r] = d_min 2^32 + r_min: the smallest distance from row r of A to a row of B of group g (self mode: to
 *              another row r' != r of A) and the SMALLEST row that attains it; -1 where there is no partner (self mode,
 *              rows_a == 1).  int64 [groups rows_a]; optional (NULL: not written); always overwritten, never accumulated
 * Both are DEVICE pointers.  Every value is an exact integer; workgroups combine through integer atomics only (64-bit adds
 * onto hist, unsigned 64-bit minima onto nearest, which is first filled with 0xFF bytes where B is split over workgroups), so
 * the result is deterministic.  Nothing is written beyond n + 1 and groups rows_a elements.  The entry needs n only, no graph.
 * DVG_E_INVALID, before any HIP call: a or hist null; rows_a, groups or n < 1; b != NULL with rows_b < 1; a row stride < W
 * (of B only when b != NULL); a group stride < 0.  DVG_E_UNSUPPORTED: n > 8192 (a workgroup keeps the n + 1 bins of the
 * histogram in LDS as 32-bit counters, in up to 8 copies as 33 KiB hold them: 8 up to n = 1055, 1 at 8192); rows_a or rows_b >=
 * 2^31 (a row index is the low half of a nearest element); groups rows_a rows_b >= 2^62. */
int dvg_packed_overlap(const uint32_t *a, int64_t rows_a, int64_t a_row_stride, int64_t a_group_stride,
                       const uint32_t *b, int64_t rows_b, int64_t b_row_stride, int64_t b_group_stride,
                       int groups, int n,
                       int64_t *hist, int64_t *nearest, int accumulate, dvg_stream_t stream);
/* The bonds of bit-packed spin rows as bit-packed rows ("DVG bonds v1"): t_e = s_i s_j on the graph's edges (i, j) = (edge_i[e],
 * edge_j[e]).  Input rows are packed as in "DVG trace v1" (W = (n + 31) / 32 words, bit b of word w = spin 32 w + b is +1; bits of
 * spins >= n are ignored and may hold anything) and addressed by (rows, row_stride, groups, group_stride) in words exactly as in
 * dvg_grbm_energy_packed.
 *   Output.  bonds_out: DEVICE, dense [groups rows][WE], WE = (E + 31) / 32, E = n_edges, indexed by the flattened t = g rows + r.
 *     Bit b of word w is bond e = 32 w + b in the graph's edge order -- the order of edge_i / edge_j given to dvg_graph_create
 *     and of quadratic -- and is set iff t_e = +1: a bond row is a packed +-1 row of E "spins" in the same convention, and every
 *     entry on packed rows takes it with n = E.  Bits >= E of the last word are written 0; nothing is written beyond groups
 *     rows WE words.  bits and bonds_out must not overlap.
 *   Value.  quadratic == NULL (product mode): t_e = s_i s_j.  quadratic given (DEVICE, [n_edges]; satisfied mode): t_e = +1 iff
 *     the bond is satisfied under E(s) = hs.s + sum_e Js_e s_i s_j:  J_e > 0: t_e = -s_i s_j;  J_e < 0: t_e = s_i s_j;  a J_e
 *     that is neither (+0, -0, NaN): t_e = +1.  Only the sign of the raw quadratic is read -- prefactor and ranges keep it, so
 *     the entry takes neither.  The popcount of a satisfied-mode bond row is the row's number of satisfied couplings.
 *   Pure bit operations: the result is a function of the input alone and two calls give the same words.  The call enqueues
 *   on `stream`, allocates nothing and needs no workspace.
 * DVG_E_INVALID, before any HIP call: g, bits or bonds_out null; a graph with no edge; rows < 1; groups < 1; row_stride < W;
 * group_stride < 0; the input's word range overlapping bonds_out.  DVG_E_UNSUPPORTED: groups rows >= 2^62; n > 8192 or n + E >
 * 16384 (a tile's spin and bond columns are kept in 8 (n + E) bytes of LDS, 128 KiB at the most).  A rejected call writes
 * nothing. */
int dvg_packed_bonds(const dvg_graph_t *g, const float *quadratic,
                     const uint32_t *bits, int64_t rows, int64_t row_stride, int64_t groups, int64_t group_stride,
                     uint32_t *bonds_out, dvg_stream_t stream);
/* Spin and bond distances between bit-packed rows, together and exactly ("DVG link overlap v1"): the link overlap q_l(a, b) =
 * (1 / E) sum_e t_e(a) t_e(b) = 1 - 2 l / E beside the spin overlap q = 1 - 2 d / n of the same pair.  The pairs are those of
 * "DVG overlap v1", with the same strides in words: cross mode (b != NULL) all rows_a rows_b pairs of every group, self mode (b
 * == NULL) the unordered pairs r < r' of A (rows_b, b_bonds and the strides of B are ignored), b_group_stride = 0 (and
 * b_bond_group_stride = 0) one B shared by the groups.  Each side brings its spin rows (a, b: W = (n + 31) / 32 words) and its
 * bond rows (a_bonds, b_bonds: WE = (n_edges + 31) / 32 words, as dvg_packed_bonds writes them) under strides of their own, so
 * that entry's dense output and views of it both work; row r of group g of the bonds of A starts at a_bonds + g
 * a_bond_group_stride + r a_bond_row_stride.  Bits of spins >= n and of bonds >= E = n_edges are ignored.  For a pair,
 * d = popc(x ^ y over the spins < n) and l = popc(t(x) ^ t(y) over the bonds < E):
 *   hist[d]      (+)= 1        int64 [n + 1]   equal to dvg_packed_overlap's hist on the same rows, bit for bit
 *   link_hist[l] (+)= 1        int64 [E + 1]
 *   link_sum[d]  (+)= l        int64 [n + 1]
 *   link_sq[d]   (+)= l l      int64 [n + 1]
 * All four are required DEVICE pointers; accumulate == 0 overwrites them, 1 adds onto their contents.  Every value is an exact
 * integer; workgroups combine through 64-bit integer atomics only, so the result is deterministic.  Nothing is written beyond
 * those sizes.  The entry needs n and n_edges only, no graph.
 * DVG_E_INVALID, before any HIP call: a, a_bonds, hist, link_hist, link_sum or link_sq null; b != NULL with b_bonds null;
 * rows_a, groups, n or n_edges < 1; b != NULL with rows_b < 1; a row stride < W or a bond row stride < WE (of B only when b !=
 * NULL); a group stride < 0.  DVG_E_UNSUPPORTED: n > 4096 or n_edges > 16384 (a workgroup keeps its counters in LDS, 20 (n + 1) +
 * 4 (n_edges + 1) bytes); rows_a or rows_b >= 2^31; groups rows_a rows_b >= 2^62; pairs n_edges^2 >= 2^63 (link_sq would wrap). */
int dvg_packed_overlap_link(const uint32_t *a, const uint32_t *a_bonds, int64_t rows_a, int64_t a_row_stride,
                            int64_t a_group_stride, int64_t a_bond_row_stride, int64_t a_bond_group_stride,
                            const uint32_t *b, const uint32_t *b_bonds, int64_t rows_b, int64_t b_row_stride,
                            int64_t b_group_stride, int64_t b_bond_row_stride, int64_t b_bond_group_stride,
                            int groups, int n, int n_edges,
                            int64_t *hist, int64_t *link_hist, int64_t *link_sum, int64_t *link_sq,
                            int accumulate, dvg_stream_t stream);
/* Which bit-packed spin rows are the same state, and how often each state occurs, exactly ("DVG distinct v1"): the equivalence
 * classes of the rows under equality on the spins < n.  Rows are packed as in "DVG trace v1": W = (n + 31) / 32 words, bit b of
 * word w = spin 32 w + b is +1.  Strides count words, as in dvg_grbm_energy_packed: row r of group g starts at bits + g
 * group_stride + r row_stride; a flat set is groups = 1, row_stride = W; slices of a trace need no copy.  The T = groups rows
 * rows are pooled under the flattened index t = g rows + r.  The KEY of a row is its W words with the bits of spins >= n
 * cleared: pad bits may hold anything and never distinguish rows.  With D the number of distinct keys:
 *   first[t]      = the smallest t' whose key equals the key of t                                   int32 [T]
 *   n_distinct[0] = D                                                                                int64 [1], required
 *   classes are numbered in the order of their first occurrence:
 *   rep[d]        = the d-th smallest value that first takes (rep is increasing, rep[0] = 0)         int32 [T], d < D written
 *   id[t]         = the d with rep[d] == first[t]                                                    int32 [T]
 *   count[d]      = the number of t with id[t] == d (the counts sum to T)                            int64 [T], d < D written
 *   with other != NULL, a flat set of rows_other rows of the same n, row u at other + u other_row_stride:
 *   other_id[u]   = the d whose key equals the key of row u of other, -1 if there is none            int32 [rows_other]
 *   other_hits[d] = the number of u with other_id[u] == d                                            int64 [T], d < D written
 *   Rows of other are looked up, never inserted: they add no class and change none of the outputs above.
 * first, id, rep, count, other_id and other_hits are each optional (NULL: not written); rep, count and other_hits are owned by
 * the caller with room for T elements, and nothing is written beyond their first D.  All pointers are DEVICE pointers.  Every
 * value is an exact integer and the result is a function of the input alone -- not of the arrival order of threads, of the
 * grid or of the hash: two calls return the same bits.  The entry needs n only, no graph; it allocates nothing and enqueues
 * on `stream`.
 *   How: an open-addressing table of int32 row indices in the workspace, capacity the power of two >= 2 T, filled with EMPTY
 *   = -1.  A row hashes its key to a start slot and probes linearly: atomicCAS(EMPTY -> t) at device scope claims a free slot;
 *   a slot that holds t' is compared with the row word by word from the read-only input (no hash is stored: every match is a
 *   full comparison) -- equal: atomicMin(slot, t), done; different: the next slot.  A slot's class never changes once set and
 *   the rows of a class walk one probe sequence, so a class ends in exactly one slot, holding its smallest index.  A row is
 *   held by a group of lanes (16 bytes each where bits and the strides are multiples of 16 bytes).  Then separate
 *   stream-ordered launches: first[t] and the class sizes (integer atomics); the flags first[t] == t compacted in order by
 *   block sums, a scan of the sums and apply (as dvg_population_resample: no workgroup waits for another); id, rep, count; the
 *   read-only lookups of other.  Every probe loop is bounded by the capacity and no thread waits for another.  A probe that
 *   exhausts the bound cannot happen at load <= 0.5; if it did, n_distinct[0] = -1 and no other output is defined.
 *   ws: DEVICE memory, aligned to 4 bytes, of dvg_packed_distinct_workspace_bytes(rows, groups, n) bytes (the table and 16
 *       bytes per row: about 24 to 32 T bytes); the query is > 0, monotone in rows, and 0 for arguments the entry rejects.
 * DVG_E_INVALID, before any HIP call: bits, n_distinct or ws null (or ws not aligned to 4 bytes); rows, groups or n < 1;
 * row_stride < W; group_stride < 0; other != NULL with rows_other < 1 or other_row_stride < W; other_id or other_hits given
 * with other == NULL.  DVG_E_UNSUPPORTED: T >= 2^31 or rows_other >= 2^31 (a row index is an int32).  DVG_E_WORKSPACE:
 * ws_bytes below the query.  A rejected call writes nothing. */
size_t dvg_packed_distinct_workspace_bytes(int64_t rows, int64_t groups, int n);
int dvg_packed_distinct(const uint32_t *bits, int64_t rows, int64_t row_stride, int64_t groups, int64_t group_stride, int n,
                        const uint32_t *other, int64_t rows_other, int64_t other_row_stride,
                        int32_t *first, int32_t *id, int32_t *rep, int64_t *count, int64_t *n_distinct,
                        int32_t *other_id, int64_t *other_hits,
                        void *ws, size_t ws_bytes, dvg_stream_t stream);
/* The full pair-correlation sums of bit-packed spin rows, exactly ("DVG corr v1"): s_i s_j summed over the rows for EVERY pair
 * of spins, not the graph's edges only (dvg_grbm_moments_packed) -- the spins x spins product of the +-1 rows, taken on their
 * bits.  Rows are packed as in "DVG trace v1": W = (n + 31) / 32 words, bit b of word w = spin 32 w + b is +1; bits of spins
 * >= n are ignored and may hold anything.  Strides count words, as in dvg_grbm_energy_packed: row r of group g starts at bits +
 * g group_stride + r row_stride; a flat set is groups = 1, row_stride = W; slices of a trace need no copy.  All T = groups rows
 * rows are pooled.
 *   pair_sum[i n + j] (+)= sum over the T rows of s_i s_j, every i, j < n: int64 [n][n], both triangles written and equal, the
 *              diagonal gets T
 *   spin_sum[i] (+)= sum over the T rows of s_i: int64 [n]; optional (NULL: not written)
 *   accumulate == 0 overwrites both, 1 adds onto their contents (pooling calls)
 * Both are DEVICE pointers.  Every value is an exact integer, T - 2 popc(col_i ^ col_j) over the spins' bit columns; workgroups
 * combine through 64-bit integer atomics only, so the result does not depend on arrival order and two calls return the same
 * bits.  Nothing is written beyond n n and n elements.  The entry needs n only, no graph.  It enqueues two kernels on `stream`
 * (rows -> bit columns in the workspace, then the column product) and allocates nothing.
 *   ws: DEVICE memory, aligned to 16 bytes, of dvg_packed_correlation_workspace_bytes(rows, groups, n) bytes: the size of the
 *       input rounded up to 1024 rows (n columns of ceil(T / 1024) 128 bytes); the query is > 0, monotone in rows, and 0 for
 *       arguments the entry rejects.
 * DVG_E_INVALID, before any HIP call: bits, pair_sum or ws null (or ws not aligned to 16 bytes); rows, groups or n < 1;
 * row_stride < W; group_stride < 0.  DVG_E_UNSUPPORTED: n > 8192 (as the other packed-row entries); groups rows >= 2^62, or
 * more than one launch takes (2^49 rows).  DVG_E_WORKSPACE: ws_bytes below the query.  A rejected call writes nothing. */
size_t dvg_packed_correlation_workspace_bytes(int64_t rows, int64_t groups, int n);
int dvg_packed_correlation(const uint32_t *bits, int64_t rows, int64_t row_stride,
                           int64_t groups, int64_t group_stride, int n,
                           int64_t *spin_sum, int64_t *pair_sum, int accumulate,
                           void *ws, size_t ws_bytes, dvg_stream_t stream);
/* Population annealing's resampling step ("DVG PA v1"): weighed chains -- dvg_gibbs_sample_ais returns each chain's log weight
 * -- are resampled in proportion to their weights: heavy chains are copied, light ones dropped, and the children are equally
 * weighted.  n_chains = P R: P = n_populations independent populations of R consecutive chains each; population p holds the
 * chains p R .. p R + R - 1.  Per population, with lw its R log weights (float64):
 *   1. m = max lw (exact in any order).
 *   2. d_c = lw_c - m, one float64 subtraction;  z_c = clamp((float)d_c, -87, 0), the conversion rounding to the nearest
 *      float32;  w_c = spec_exp(z_c), the bit-specified float32 exp of csrc/philox.h and oracle/gibbs.py;
 *      k_c = (uint64)((double)w_c 2^32): the scaling is exact, the conversion truncates, 0 <= k_c <= 2^32.  The heaviest chain
 *      has k = 2^32; a chain whose w_c is below 2^-32 (more than 32 log 2 ~= 22.2 below the maximum; -inf too) has k = 0 and
 *      never a child.  NaN and +inf are not allowed and not checked.
 *   3. S_c = k_0 + ... + k_c in uint64,  K = S_{R-1}:  2^32 <= K <= 2^52 as R <= 2^20.
 *   4. o = philox4x32_10(ctr = (0, chain_id0 + p R, step, STREAM_RESAMPLE = 5), key = seed) (the key split lo / hi as in every
 *      stream);  r64 = (o.x << 32) | o.y;  V = mulhi64(r64, K), in [0, K) and uniform to within K / 2^64 <= 2^-12 per value.
 *   5. Systematic resampling: q = K / R, rem = K % R (integers); child j = 0 .. R-1 points at
 *      t_j = j q + (j rem + V) / R  (integer division, every term below 2^53)  = floor((j K + V) / R) < K,
 *      and its parent is the smallest c with S_c > t_j.
 *   6. parent_out[p R + j] = p R + c;  state_out[p R + j] = state_in[p R + c], a row of n int8;  family_out[p R + j] =
 *      family_in[p R + c], or p R + c, the parent's global index, where family_in == NULL;  weight_out[p R + c] = k_c.
 * Everything is integer or bit-specified float arithmetic: the result is a function of (lw, seed, chain_id0, step) alone, no
 * last bit is the implementation's.  A chain gets floor(R k_c / K) or ceil(R k_c / K) children; the parents of a population
 * are non-decreasing; equal weights give the identity; and as the counter holds the population's own first chain id, a call
 * on the populations a .. b alone with chain_id0 advanced by a R gives that slice of the whole call (rank-sharded chains).
 * The float32 weights bias the resampling by <= 2^-24 relative per chain; an estimate of log Z uses the float64 log weights,
 * not k.
 *   All pointers are DEVICE pointers.  log_weight float64 [n_chains]; parent_out int32 [n_chains], required; state_in /
 *   state_out int8 (n_chains, n), both or neither; family_out int32 [n_chains] and weight_out uint64 [n_chains] optional
 *   (NULL: not written); family_in is read only with family_out.  Out of place.  Nothing is written beyond n_chains elements
 *   or rows of any output.  The entry needs no graph, enqueues on `stream` and allocates nothing; ws: a workspace of at least
 *   dvg_population_resample_workspace_bytes(n_chains) bytes.  Populations of up to 1024 chains take one workgroup each; larger
 *   ones separate stream-ordered launches (block sums, a scan of the sums, apply): no workgroup waits for another.
 * DVG_E_INVALID, before any HIP call: log_weight, parent_out or ws null; n_chains < 1, n_populations < 1, n_chains not a
 * multiple of n_populations; exactly one of state_in, state_out null; n < 1 with a state; state_in == state_out; family_in ==
 * family_out != NULL.  DVG_E_WORKSPACE: ws_bytes below the query.  DVG_E_UNSUPPORTED: R > 2^20 (K must stay below 2^53). */
size_t dvg_population_resample_workspace_bytes(int n_chains);
int dvg_population_resample(const double *log_weight, int n_chains, int n_populations,
                            uint32_t chain_id0, uint64_t seed, uint32_t step,
                            const int8_t *state_in, int8_t *state_out, int n,
                            const int32_t *family_in, int32_t *family_out,
                            int32_t *parent_out, uint64_t *weight_out,
                            void *ws, size_t ws_bytes, dvg_stream_t stream);

/* ------------------------------------------------------------------ input pipeline
 * The reference's per-image transform Resize((S,S)) -> ToTensor() -> round
 * (/root/reference/src/model_wrapper.py:70-77) over a whole data set: src (n_images, in, in) uint8 ->
 * out (n_images, 1, out, out) float32 in {0, 1}.  Bit-exact restatement of PIL's two-pass BILINEAR
 * resampling (8-bit intermediate, 22-bit fixed-point coefficients), which is what torchvision's Resize
 * applies to the PIL images MNIST yields; sides up to 64. */
int dvg_resize_binarise(const uint8_t *src, int64_t n_images, int in_size, int out_size, float *out,
                        dvg_stream_t stream);
/* out[r] = table[idx[r]], rows of row_floats floats (the shuffled mini-batch of a device-resident data
 * set: DataLoader(shuffle=True), /root/reference/src/model_wrapper.py:103).  idx: DEVICE int64.  An index
 * outside [0, rows) is not dereferenced; *bad_index_flag (DEVICE int, may be NULL) is set to 1. */
int dvg_gather_rows(const float *table, int64_t rows, int64_t row_floats, const int64_t *idx, int64_t n,
                    float *out, int *bad_index_flag, dvg_stream_t stream);

/* ------------------------------------------------------------------ latent -> discrete
 * Default latent_to_discrete of DiscreteVariationalAutoencoder
 * (/root/reference/src/model_wrapper.py:184-188 passes None -> plugin default):
 * Gumbel-softmax over logits [l, 0], temperature tau, hard, R replicas, mapped
 * to spins +-1 with the straight-through gradient.
 *   logits (B, n); gumbels (B, R, n, 2) Gumbel(0,1) noise or NULL (then drawn
 *   on device from Philox stream GUMBEL with (seed, offset));
 *   spins (B, R, n) out; dspin (B, R, n) out: d spin / d logit, kept for bwd.
 */
int dvg_gumbel_fwd(const float *logits, int64_t B, int n, int R, float tau, const float *gumbels,
                   uint64_t seed, uint64_t offset, float *spins, float *dspin,
                   const dvg_step_state_t *dyn, dvg_stream_t stream);
/* grad_logits (B, n) = sum_r grad_spins[b,r,:] * dspin[b,r,:] */
int dvg_gumbel_bwd(const float *grad_spins, const float *dspin, int64_t B, int n, int R,
                   float *grad_logits, dvg_stream_t stream);
/* the same with TWO gradients wrt the spins (grad_spins2 may be NULL): grad_logits = sum_r (g1 + g2) * dspin.  The step
 * has two -- through the decoder (MSE) and from the MMD, /root/reference/src/model_wrapper.py:322-326 backpropagates
 * their sum -- and adding them here saves a pass over (B, R, n). */
int dvg_gumbel_bwd2(const float *grad_spins, const float *grad_spins2, const float *dspin, int64_t B, int n, int R,
                    float *grad_logits, dvg_stream_t stream);
/* out[0] = a[0] + b[0] on the device (dvae_loss = mse + mmd, /root/reference/src/model_wrapper.py:322, without a host
 * synchronisation and without a framework kernel in the captured step) */
int dvg_scalar_add(const float *a, const float *b, float *out, dvg_stream_t stream);
/* "heaviside" mode (/root/reference/src/utils/common.py:160-173): spins (B,1,n) = 2*H(l)-1 with
 * H(0)=0; the backward is the identity and needs no kernel. */
int dvg_heaviside_fwd(const float *logits, int64_t numel, float *spins, dvg_stream_t stream);

/* ------------------------------------------------------------------ MMD
 * GaussianKernel(n_kernels) + maximum_mean_discrepancy_loss(x, y, kernel)
 * (/root/reference/src/model_wrapper.py:273, :320).  One fused pass computes the
 * loss and d loss / d x (y carries no gradient in the reference: it is drawn
 * under torch.no_grad(), model_wrapper.py:308).  Never materialises the
 * (nx+ny)^2 kernel matrix.
 */
typedef struct {
  int32_t n_kernels;   /* 7 in the reference */
  float factor;        /* bandwidth multiplier base, 2.0 */
  float bandwidth;     /* > 0: fixed base bandwidth; <= 0: data-driven sum(D)/(N^2-N) */
  int32_t squared;     /* 0: Euclidean distance (default), 1: squared distance */
  int32_t reduce_mean; /* 0: kernels summed (default), 1: averaged */
  int32_t biased;      /* 0: unbiased estimator (default), 1: biased (plain means) */
} dvg_mmd_cfg_t;
size_t dvg_mmd_workspace_bytes(int64_t nx, int64_t ny, int dim);
/* Executed matrix work of one dvg_mmd_fwd_bwd call with gradient on +-1 (spin) rows of this shape, by MFMA type: int8
 * FLOPs of the Gram tiles, bf16 FLOPs of the gradient GEMM and the number of bf16 terms a weight is split into (0 / 0 / 0
 * when the shape is served by the f32 kernels).  For roofline pricing (bench.py); launches nothing. */
int dvg_mmd_spin_flops(int64_t nx, int64_t ny, int dim, double *int8_flops, double *bf16_flops, int *bf16_terms);
int dvg_mmd_fwd_bwd(const float *x, int64_t nx, const float *y, int64_t ny, int dim,
                    const dvg_mmd_cfg_t *cfg, float *loss_out /* device scalar */,
                    float *grad_x /* (nx, dim) or NULL */, void *ws, size_t ws_bytes,
                    dvg_stream_t stream);

/* ------------------------------------------------------------------ encoder
 * Encoder.forward / backward (/root/reference/src/encoder.py:18-49): 4 x
 * [conv3x3 -> BatchNorm2d -> MaxPool2d(2) -> LeakyReLU] (no LeakyReLU after the
 * last) with channels [1,32,64,128,n], then Linear(4,1) per channel.
 * Parameter tensors are in the checkpoint layout (conv weight (Cout,Cin,3,3)).
 * images (B,1,32,32) -> logits (B,n).  `ws` carries the saved activations from
 * fwd to bwd (size from dvg_encoder_workspace_bytes) and must stay untouched in
 * between.  training != 0: batch statistics, running stats updated in place
 * (momentum 0.1, unbiased variance), num_batches_tracked += 1.
 */
typedef struct {
  const float *conv_w[4], *conv_b[4]; /* Conv2d weight / bias */
  const float *bn_g[4], *bn_b[4];     /* BatchNorm2d weight / bias */
  float *bn_rm[4], *bn_rv[4];         /* running_mean / running_var (updated when training) */
  int64_t *bn_nbt[4];                 /* num_batches_tracked (may be NULL) */
  const float *proj_w, *proj_b;       /* Linear(4,1) */
} dvg_encoder_params_t;
typedef struct {
  float *conv_w[4], *conv_b[4], *bn_g[4], *bn_b[4], *proj_w, *proj_b;
} dvg_encoder_grads_t;
size_t dvg_encoder_workspace_bytes(int64_t B, int n_latents);
int dvg_encoder_fwd(const dvg_encoder_params_t *p, int n_latents, const float *images, int64_t B,
                    int training, float *logits, void *ws, size_t ws_bytes, dvg_stream_t stream);
int dvg_encoder_bwd(const dvg_encoder_params_t *p, int n_latents, const float *images, int64_t B,
                    const float *grad_logits, const dvg_encoder_grads_t *grads, void *ws,
                    size_t ws_bytes, dvg_stream_t stream);

/* ------------------------------------------------------------------ decoder
 * Decoder.forward / backward (/root/reference/src/decoder.py:18-62):
 * Linear(n,4n) -> (n,2,2) -> 4 x [ConvTranspose2d 3x3 -> BatchNorm2d ->
 * Dropout2d(0.2) -> Upsample x2 -> LeakyReLU] with channels [n,128,64,32,1] ->
 * ConvTranspose2d(1,1).  spins (N = B*R, n) -> out (N,1,32,32).
 * ConvTranspose weights in checkpoint layout (Cin,Cout,3,3).
 * dropout_keep[l]: (N, C_l) float {0,1} keep-masks, or NULL to draw them on
 * device (Philox stream DROPOUT, (seed, offset)); ignored unless training.
 */
typedef struct {
  const float *lin_w, *lin_b;         /* increase_latent_dim (4n,n), (4n) */
  const float *conv_w[5], *conv_b[5]; /* convtrans.{0,5,10,15,20} */
  const float *bn_g[4], *bn_b[4];
  float *bn_rm[4], *bn_rv[4];
  int64_t *bn_nbt[4];
} dvg_decoder_params_t;
typedef struct {
  float *lin_w, *lin_b, *conv_w[5], *conv_b[5], *bn_g[4], *bn_b[4];
} dvg_decoder_grads_t;
size_t dvg_decoder_workspace_bytes(int64_t N, int n_latents);
int dvg_decoder_fwd(const dvg_decoder_params_t *p, int n_latents, const float *spins, int64_t N,
                    int training, const float *const dropout_keep[4], uint64_t seed,
                    uint64_t offset, float *out, void *ws, size_t ws_bytes, const dvg_step_state_t *dyn,
                    dvg_stream_t stream);
/* The part of a forward call that depends on the parameters and the dropout stream alone (weight packs, the composed
 * Linear o ConvTranspose weights, the Dropout2d keep-masks), enqueued on `stream` ahead of time: a training step hands
 * in a stream forked off its main stream where the step starts, so that these launches (~190 us at B R = 32768) run
 * beside the encoder instead of between the spins and the decoder's first GEMM.  The next
 * dvg_decoder_fwd_ex(..., prepared = 1, ...) on the same workspace waits for them (an event recorded here) and skips
 * its own prologue; it fails unless it is called with the same parameters, N, training flag, seed / offset / dyn and
 * kernel-form options, which must not change in between.  A forward call with prepared = 0 (dvg_decoder_fwd) joins a
 * prologue in flight on its workspace and then ignores it.  Device-drawn dropout masks only. */
int dvg_decoder_prepare(const dvg_decoder_params_t *p, int n_latents, int64_t N, int training, uint64_t seed,
                        uint64_t offset, void *ws, size_t ws_bytes, const dvg_step_state_t *dyn,
                        dvg_stream_t stream);
int dvg_decoder_fwd_ex(const dvg_decoder_params_t *p, int n_latents, const float *spins, int64_t N,
                       int training, const float *const dropout_keep[4], uint64_t seed, uint64_t offset,
                       float *out, void *ws, size_t ws_bytes, const dvg_step_state_t *dyn, int prepared,
                       dvg_stream_t stream);
int dvg_decoder_bwd(const dvg_decoder_params_t *p, int n_latents, const float *spins, int64_t N,
                    const float *grad_out, const dvg_decoder_grads_t *grads,
                    float *grad_spins /* (N,n) or NULL */, void *ws, size_t ws_bytes,
                    dvg_stream_t stream);
/* The same with the join of the weight-gradient chain left to the caller: grad_spins is complete in `stream` order when
 * the call returns, the PARAMETER gradients only after dvg_stream_join_side(stream) or after the next dvg_encoder_bwd /
 * dvg_decoder_bwd call on `stream` has returned (their weight-gradient chains run on the same library side stream, in
 * order, and their own join covers what was queued before).  A training step whose decoder backward is followed by the
 * encoder backward overlaps the tail of the decoder's weight-gradient chain (the Linear layer's, ~1 ms at B R = 32768)
 * with the head of the encoder's data-gradient chain this way.  defer_join = 0 is dvg_decoder_bwd. */
int dvg_decoder_bwd_ex(const dvg_decoder_params_t *p, int n_latents, const float *spins, int64_t N,
                       const float *grad_out, const dvg_decoder_grads_t *grads, float *grad_spins, void *ws,
                       size_t ws_bytes, int defer_join, dvg_stream_t stream);
/* Orders `stream` behind everything queued so far on the library's side stream of the current device (no-op when the
 * side stream is disabled). */
int dvg_stream_join_side(dvg_stream_t stream);
/* The decoder with the reconstruction loss fused behind it -- Decoder.forward + mse_loss of the training step
 * (/root/reference/src/model_wrapper.py:297-305) as ONE pair of calls.  An addition to the surface above, not a
 * replacement: dvg_decoder_fwd_ex + dvg_mse_fwd_bwd + dvg_decoder_bwd_ex compute the same loss (to rounding of its double
 * partial sums) and the same gradients BIT FOR BIT (tests/test_gpu_nets.py); what the pair saves is memory traffic.
 * The reconstruction (N,1,32,32) and its gradient are never written: the final ConvTranspose2d(1,1), the squared error
 * against images (N / R, 1024) -- replica r of image b is decoder row b R + r --, the final layer's data gradient and the
 * 1-channel stage's BatchNorm / Dropout2d / LeakyReLU backward run in one pass per image, and the passes of the backward
 * call that need the loss gradient form it again from the stage's saved pre-BatchNorm output (1.1 GB -> 0.23 GB of HBM
 * traffic at N = 32768).  Training mode only; needs option dec_tail_fused != 0 (the default).
 * loss_out = mean((recon - image)^2); the gradient seeded into the backward is grad_scale * d loss / d recon, as in
 * dvg_mse_fwd_bwd, and dvg_decoder_bwd_mse_ex must be given the same images, R and grad_scale as the forward call on
 * this workspace.  Every other argument as in dvg_decoder_fwd_ex / dvg_decoder_bwd_ex. */
int dvg_decoder_fwd_mse_ex(const dvg_decoder_params_t *p, int n_latents, const float *spins, int64_t N,
                           const float *const dropout_keep[4], uint64_t seed, uint64_t offset, const float *images,
                           int R, float grad_scale, float *loss_out, void *ws, size_t ws_bytes,
                           const dvg_step_state_t *dyn, int prepared, dvg_stream_t stream);
int dvg_decoder_bwd_mse_ex(const dvg_decoder_params_t *p, int n_latents, const float *spins, int64_t N,
                           const float *images, int R, float grad_scale, const dvg_decoder_grads_t *grads,
                           float *grad_spins, void *ws, size_t ws_bytes, int defer_join, dvg_stream_t stream);
/* The caller's promise about the `spins` of the NEXT forward call on workspace `ws` (dvg_decoder_fwd, dvg_decoder_fwd_ex,
 * dvg_decoder_fwd_mse_ex): pm1 != 0 declares that every element is exactly +1.0f or -1.0f, as the output of
 * dvg_gumbel_fwd is.  The library never looks at the data to find out (no host sync).  The forward call takes the
 * declaration -- it holds for that one call; a call without a declaration in front of it has made none -- and the
 * backward call on the same workspace sees what its forward was given.  With the promise the decoder's input layer
 * (Linear(n,4n), or its composition with the first ConvTranspose2d at large batches) multiplies the spins as exact bf16
 * values with the float32 weights carried as three bf16 pieces, three exact products on the bf16 matrix pipe summed in
 * float32, in its forward GEMM and its weight-gradient GEMM under DVG_PRECISION_F32 and DVG_PRECISION_F32_SPLIT3:
 * float32-class results (the products themselves are exact) at a fraction of the f32 matrix time.
 * A FALSE promise is not detected: the spins are rounded to bf16 (8 significant bits) in those two GEMMs, every result
 * stays finite, float32 accuracy is lost.  Host-side bookkeeping only; call it from the thread that makes the forward
 * call.  (Development option dec_spin_gemm = 0 ignores every declaration.) */
int dvg_decoder_declare_spins(const void *ws, int pm1);

/* ------------------------------------------------------------------ MSE
 * torch.nn.functional.mse_loss(reconstructed, images.unsqueeze(1).repeat(1,R,...))
 * (/root/reference/src/model_wrapper.py:302-305), fused with its gradient:
 * loss_out = mean((recon - image)^2); grad_recon = grad_scale * 2 (recon - image) / numel.
 * recon (B,R,1024), images (B,1024).
 */
size_t dvg_mse_workspace_bytes(void);
int dvg_mse_fwd_bwd(const float *recon, const float *images, int64_t B, int R, float grad_scale,
                    float *loss_out, float *grad_recon /* or NULL */, void *ws, size_t ws_bytes,
                    dvg_stream_t stream);

/* ------------------------------------------------------------------ Adam
 * torch.optim.Adam with coupled L2 weight decay, as configured at
 * /root/reference/src/model_wrapper.py:208-217, on one flat parameter buffer.
 * g <- grad_scale*g + wd*p;  m,v updated; p -= lr/(1-b1^t) * m / (sqrt(v/(1-b2^t)) + eps).
 */
int dvg_adam_step(float *p, const float *g, float *m, float *v, int64_t numel, float lr,
                  float beta1, float beta2, float eps, float weight_decay, int64_t step,
                  float grad_scale, const dvg_step_state_t *dyn, int dyn_slot, dvg_stream_t stream);

/* ------------------------------------------------------------------ stream anchor
 * Enqueues one empty kernel on `stream`.  For callers that capture a step into a hipGraph with a side stream forked
 * off `stream`: the HIP graph executor keeps the first KERNEL node captured after a fork on the parent's hardware
 * queue and replays nodes in capture order, so "record event; dvg_stream_anchor(stream); enqueue the side work;
 * enqueue the rest of the main work" keeps the main chain on its queue (a queue change costs ~10-15 us per hop, and
 * far more when it lands behind a long kernel) while the side work is still submitted early.
 */
int dvg_stream_anchor(dvg_stream_t stream);

/* ------------------------------------------------------------------ arithmetic mode of the convolution GEMMs
 * Process-wide switch read by dvg_encoder_fwd/bwd and dvg_decoder_fwd/bwd (a forward call and its backward call must
 * run in the same mode).  DVG_PRECISION_F32 (default): float32 operands, the <= 1e-5 relative loss parity against the
 * reference's CPU path.  DVG_PRECISION_BF16_INPUTS: "bf16 GEMM inputs, f32 accumulate" for the forward and
 * data-gradient GEMMs of encoder and decoder -- what a `torch.autocast(bfloat16)` run of src/encoder.py:28-30 /
 * src/decoder.py:28,34-38 would feed its convolutions; weight gradients, BatchNorm, losses and Adam stay float32.
 * DVG_PRECISION_F32_SPLIT3: float32 operands of the same GEMMs carried as three bf16 pieces each (x = hi + mid + lo,
 * exact) and multiplied as the six piece products down to 2^-16 on the bf16 MFMA with float32 accumulation: what is
 * dropped is below 2^-23 of a product, i.e. float32-class results (same parity bars as DVG_PRECISION_F32) at 6/16 of
 * the f32 MFMA's matrix time.
 * (The library reads no environment variable: the host side -- `CONV_PRECISION` in the YAML, bench.py --precision --
 * calls dvg_set_conv_precision.)
 */
#define DVG_PRECISION_F32 0
#define DVG_PRECISION_BF16_INPUTS 1
#define DVG_PRECISION_F32_SPLIT3 2
int dvg_set_conv_precision(int mode);
int dvg_get_conv_precision(void);

/* ------------------------------------------------------------------ kernel-form options
 * The library has ONE path per operation by default; a handful of named integer options select alternative kernel forms
 * of the same function (A/B measurements; tests that compare two forms).  They are part of this boundary -- nothing in
 * the library reads the environment.  Names and meanings: dvg_option_name(i) / dvg_option_doc(i), i < dvg_option_count();
 * INTEGRATION.md lists them.  Options may be changed between calls; a backward call whose forward ran under another plan
 * fails with DVG_E_INVALID.  dvg_reset_options restores every default. */
int dvg_option_count(void);
const char *dvg_option_name(int index);
const char *dvg_option_doc(int index);
int dvg_set_option(const char *name, int64_t value);
int dvg_get_option(const char *name, int64_t *value);
int dvg_reset_options(void);

/* ------------------------------------------------------------------ profiler
 * Optional per-kernel HIP-event timing inside the library (used by bench.py for
 * the `roofline` object).  Off by default.  `kernel_mask` bit i enables kernel id i
 * (ids/names: dvg_prof_num_kernels / dvg_prof_kernel_name); an enabled kernel gets
 * one event pair recorded on the caller's stream around each of its launches.
 */
int dvg_prof_enable(uint64_t kernel_mask);
int dvg_prof_reset(void);
int dvg_prof_num_kernels(void);
const char *dvg_prof_kernel_name(int id);
/* synchronises the recorded events; returns total milliseconds and launch count */
int dvg_prof_query(int id, double *total_ms, int64_t *launches);
/* algorithmic work (FLOPs for the GEMM-shaped kernels, 0 otherwise) summed over the timed launches */
int dvg_prof_query_work(int id, double *work);
/* sum over the kernel's launches of duration x the share of the chip's CUs the launch's grid was sized for (1 for every
 * kernel but the CU-budgeted persistent Winograd grids): the time base of roofline fractions "of the CUs it was given" */
int dvg_prof_query_share(int id, double *share_ms);

#ifdef __cplusplus
}
#endif
#endif /* DVG_H */
