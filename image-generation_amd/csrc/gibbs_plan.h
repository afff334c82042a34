// The kernel form of one Gibbs draw (gibbs.hip): decided ONCE per C-ABI call from (graph shape, chains, draw kind, option
// gibbs_generic), and everything the form implies -- template parameters, slots, grid, LDS -- derived here and nowhere
// else.  gibbs.hip keeps the kernels, their argument blocks and one table per kernel family that maps the plan's integers
// to an instantiation.  Host code only, apart from the LDS layout functions the kernels carve their images with.
// (The DRAW plan: Python's graphs.GibbsPlan is the graph's plan -- colouring and CSR.)
#pragma once
#include "common.h"

namespace dvg {

constexpr int GIBBS_NB = 5;                  // batches of 4 neighbours per round of the neighbour sum
constexpr size_t GIBBS_LDS_MAX = 160 * 1024;

// ---------------------------------------------------------------- LDS layouts: the kernels and the plan size them here
// The padded-row image of the rolled and slots forms (gibbs.hip: GibbsLds); returns the bytes in front of the state rows.
__host__ __device__ __forceinline__ size_t gibbs_lds_layout(int n, int n_batches, int n_colours, size_t off[7]) {
  size_t b = 0;
  off[0] = b; b += sizeof(float) * (size_t)((n + 3) & ~3);
  off[1] = b; b += sizeof(float) * 4 * (size_t)(n_batches + 1);
  off[2] = b; b += sizeof(uint32_t) * (size_t)n;
  off[3] = b; b += sizeof(int32_t) * (size_t)(n_colours + 1);
  b = (b + 7) & ~(size_t)7;
  off[4] = b; b += sizeof(uint16_t) * 4 * (size_t)(n_batches + 1);
  off[5] = b; b += sizeof(uint16_t) * (size_t)((n + 1) & ~1);
  off[6] = b;
  return b;
}
// ... with the float16 state rows of `chains` chains behind it
__host__ __device__ __forceinline__ size_t gibbs_lds_bytes(int n, int n_batches, int n_colours, int chains) {
  size_t o[7];
  return gibbs_lds_layout(n, n_batches, n_colours, o) + 2 * (size_t)chains * ((n + 15) & ~15);
}
// words of one chain's row of held flags in LDS (the rolled form of a conditional draw), one bit per spin
__host__ __device__ __forceinline__ int gibbs_held_words(int n) { return (n + 31) >> 5; }
// bytes of one chain's row of scaled, clamped linear terms in LDS (the rolled form of a per-chain-field draw): float32, n_pad entries
__host__ __device__ __forceinline__ size_t gibbs_field_row_bytes(int n) { return sizeof(float) * (size_t)((n + 15) & ~15); }

// LDS of the fixed-row image (slots form, FIX): h [n] | couplings [n][20] | state offsets [n][20] | order [n] | state [n_pad][CH]
__host__ __device__ __forceinline__ size_t gibbs_fix_layout(int n, size_t off[5]) {
  size_t b = 0;
  off[0] = b; b += sizeof(float) * (size_t)((n + 3) & ~3);
  off[1] = b; b += sizeof(float) * 20 * (size_t)n;
  off[2] = b; b += sizeof(uint16_t) * 20 * (size_t)n;
  off[3] = b; b += sizeof(uint16_t) * (size_t)((n + 7) & ~7);
  off[4] = b;
  return b;
}

// The lane-major form: tables | one state row per chain | a 64-entry sink per wave (where lanes without a spin in a slot store)
__host__ __device__ __forceinline__ size_t gibbs_lane_lds_bytes(int slots, int mb, int lpc, int n, int chains) {
  return (size_t)slots * mb * lpc * 24 + 2 * (size_t)chains * ((n + 15) & ~15) + 2 * 64 * (size_t)((chains * lpc + 63) / 64);
}

// The exchange draw (replica exchange, "DVG PT v1"): behind the form's own image of `form_bytes` bytes, for the `slots`
// chain slots of a workgroup: two mailboxes of float64 chain energies [2][slots], indexed (ladder in workgroup, rung) |
// accepted-exchange counters [slots], indexed (ladder in workgroup, lower rung) | the ladder's betas [16].  Returns the
// bytes of the whole image.
constexpr int GIBBS_MAX_REPLICAS = 16;
__host__ __device__ __forceinline__ size_t gibbs_exchange_lds_layout(size_t form_bytes, int slots, size_t off[3]) {
  size_t b = (form_bytes + 7) & ~(size_t)7;
  off[0] = b; b += sizeof(double) * 2 * (size_t)slots;
  off[1] = b; b += sizeof(uint32_t) * (size_t)slots;
  off[2] = b; b += sizeof(float) * GIBBS_MAX_REPLICAS;
  return b;
}

// ---------------------------------------------------------------- the instantiations, each family listed ONCE
// The plan's "has a kernel" test and the tables of gibbs.hip that map a plan to a function pointer both expand from these.
// Lane-major (gibbs_fast_kernel): (LPC, WAVES, MB, NR, MAXS).  A shape takes the FIRST entry with its lpc, mb and nr, its
// one-wave rule (WAVES == 1) and MAXS >= its rows.
#define DVG_GIBBS_LANE_KERNELS(X)                                                                       \
  X(16, 1, 4, 1, 12) X(16, 4, 4, 1, 12) X(16, 1, 5, 1, 12) X(16, 4, 5, 1, 12)                           \
  X(32, 1, 4, 1, 12) X(32, 4, 4, 1, 12) X(32, 1, 5, 1, 12) X(32, 4, 5, 1, 12)                           \
  X(64, 1, 4, 1, 12) X(64, 4, 4, 1, 12) X(64, 1, 5, 1, 12) X(64, 4, 5, 1, 12)                           \
  X(64, 4, 4, 1, 20) X(64, 4, 5, 1, 20)                                                                 \
  X(64, 4, 4, 2, 12) X(64, 4, 5, 2, 12) X(64, 4, 4, 2, 20) X(64, 4, 5, 2, 20)
// Rolled (gibbs_kernel): (LPC, WAVES)
#define DVG_GIBBS_ROLLED_KERNELS(X) X(16, 1) X(16, 4) X(32, 1) X(32, 4) X(64, 1) X(64, 4) X(64, 16)
// Chains side by side (gibbs_slot_kernel, the plain draw only): (MAXS, CH, FIX)
#define DVG_GIBBS_SLOT_KERNELS(X)                                                 \
  X(18, 16, true) X(20, 16, true) X(18, 16, false) X(20, 16, false)               \
  X(18, 8, true) X(20, 8, true) X(18, 8, false) X(20, 8, false)

// ---------------------------------------------------------------- the graph, as far as the choice depends on it
// Nothing here lives on the device.  The lane-major image (graph.h): lane_lpc lanes work on a chain -- the smallest of
// 16 / 32 / 64 that covers the largest class in one pass, 64 otherwise; passes are grouped in steps of lane_nr rows (2 when
// any class takes more than one pass); lane_mb batches per row (4 or 5); lane_rows rows in all.  A graph has the image
// (lane_has) when its rows are at most 20 (64 lanes) or 12 (16 / 32 lanes) and no spin has more than 20 neighbours.
struct GibbsGraphShape {
  int n, n_colours, max_class;
  int n_batches, max_batches;  // padded-row image: batches over all rows; the longest row's batches
  int32_t class_ptr[65];       // host copy (n_colours <= 64)
  bool lane_has;
  int lane_lpc, lane_mb, lane_nr, lane_rows;
};
// pure; n_colours in 1..64, class_ptr [n_colours + 1], adj_ptr [n + 1]
GibbsGraphShape gibbs_graph_shape(int n, int n_colours, const int32_t* class_ptr, const int32_t* adj_ptr);

// ---------------------------------------------------------------- the draw
// plain: dvg_gibbs_sample; held: _clamped (kernels' HELD); table: _annealed (SCHED = GIBBS_TABLE); weigh: _ais (GIBBS_WEIGH);
// exchange: _tempered (GIBBS_EXCHANGE) and _tempered_traced (GIBBS_EXCHANGE_TRACE: the same plan, a record is packed from the
// chain's own row and registers) -- planned by gibbs_exchange_plan, which needs the replica count as well;
// trace: _traced (GIBBS_TRACE) -- the table kind's choices (no slots form), the table kind's LDS: a record is packed from the
// state rows where they lie;
// field: _fields (GIBBS_FIELD) -- the rolled form on every graph: the instantiation the table kind takes under gibbs_generic = 1,
// its WAVES stepped down within DVG_GIBBS_ROLLED_KERNELS until the image fits with a float32 row of hs per chain slot behind the
// state rows (6 bytes per spin and chain where the other kinds keep 2);
// field_weigh: _fields_ais (GIBBS_FIELD_WEIGH) -- the field kind's plan, the same LDS image: the weights are registers
enum GibbsDrawKind : int { GK_PLAIN = 0, GK_HELD, GK_TABLE, GK_WEIGH, GK_EXCHANGE, GK_TRACE, GK_FIELD, GK_FIELD_WEIGH };
constexpr bool gibbs_field_kind(GibbsDrawKind k) { return k == GK_FIELD || k == GK_FIELD_WEIGH; }
//   GF_ROLLED  gibbs_kernel<lpc, waves, HELD, SCHED>: any graph
//   GF_LANE    gibbs_fast_kernel<lpc, waves, mb, nr, maxs, HELD, SCHED>: graphs with a lane-major image
//   GF_SLOTS   gibbs_slot_kernel<maxs, ch, fix>: ch chains of a 16-wave workgroup side by side; the plain draw only
enum GibbsForm : int { GF_ROLLED = 0, GF_LANE, GF_SLOTS };

// a lane's static (class, pass) slots of the slots form; pass = 16 waves x (64 / ch) spins
struct GibbsSlots { int n; uint32_t last_mask; int16_t lo[20], hi[20]; };

struct GibbsDrawPlan {
  GibbsForm form;
  int lpc, waves;    // rolled, lane-major (others: 0)
  int mb, nr, maxs;  // lane-major; maxs also the slots form's 18 / 20
  int ch;            // slots
  bool fix;          // slots: the fixed-row image (at most 20 neighbours per spin and it fits)
  GibbsSlots slots;  // slots
  int chains_per_block, grid, threads;
  size_t lds;        // dynamic LDS bytes (held rolled form: the flag words included; field kind: the hs rows included)
};

// Pure: the same arguments give the same plan.  generic_option: option gibbs_generic as the call read it.
// DVG_E_UNSUPPORTED (and the error message) when the form the graph must take needs more than 160 KiB of LDS.
int gibbs_draw_plan(const GibbsGraphShape& g, int n_chains, GibbsDrawKind kind, int64_t generic_option, GibbsDrawPlan* out);

// The exchange draw's plan: n_ladders ladders of n_replicas (2..16) consecutive chains.  A ladder's chains hand rungs over
// in LDS, so a workgroup must hold whole ladders.  Form: the table kind's plan for n_ladders * n_replicas chains if its
// workgroup holds a ladder; else the same family at 4 waves if that does; else the rolled form (64, 16), which serves every
// graph and holds 16 chains.  A workgroup holds chains_per_block / n_replicas ladders (*ladders_per_block; its other slots
// idle), grid = ceil(n_ladders / that), lds = the form's own image plus gibbs_exchange_lds_layout.  Pure.
int gibbs_exchange_plan(const GibbsGraphShape& g, int n_ladders, int n_replicas, int64_t generic_option, GibbsDrawPlan* out,
                        int* ladders_per_block);

}  // namespace dvg
