// The Gibbs draw's plan (gibbs_plan.h): which graphs get a lane-major image, and which kernel form a draw takes.
#include "gibbs_plan.h"

#include <algorithm>

namespace dvg {

GibbsGraphShape gibbs_graph_shape(int n, int n_colours, const int32_t* class_ptr, const int32_t* adj_ptr) {
  GibbsGraphShape g{};
  g.n = n; g.n_colours = n_colours;
  for (int k = 0; k <= n_colours; ++k) g.class_ptr[k] = class_ptr[k];
  for (int k = 0; k < n_colours; ++k) g.max_class = std::max(g.max_class, class_ptr[k + 1] - class_ptr[k]);
  // padded-row image: row i occupies ceil(deg / 4) batches
  for (int i = 0; i < n; ++i) {
    const int b = (adj_ptr[i + 1] - adj_ptr[i] + 3) / 4;
    g.max_batches = std::max(g.max_batches, b);
    g.n_batches += b;
  }
  const int lpc = g.max_class <= 16 ? 16 : g.max_class <= 32 ? 32 : 64;
  const int nr = g.max_class > lpc ? 2 : 1;
  int rows = 0;
  for (int c = 0; c < n_colours; ++c) {
    const int passes = (class_ptr[c + 1] - class_ptr[c] + lpc - 1) / lpc;
    rows += nr * ((passes + nr - 1) / nr);
  }
  // (the caps are the largest MAXS of DVG_GIBBS_LANE_KERNELS per lane count, 5 batches its largest MB; 16-bit state offsets)
  if (rows <= (lpc == 64 ? 20 : 12) && g.max_batches <= 5 && n <= 32767) {
    g.lane_has = true;
    g.lane_lpc = lpc; g.lane_mb = g.max_batches <= 4 ? 4 : 5; g.lane_nr = nr; g.lane_rows = rows;
  }
  return g;
}

// pass = 16 waves x (64 / ch) spins; false: more than 20 (class, pass) slots, or a graph beyond the slot registers' bit fields
static bool gibbs_make_slots(const GibbsGraphShape& g, int ch, GibbsSlots* out) {
  if (g.n_colours > 64 || g.n >= 2048 || g.n_batches >= 8192) return false;
  GibbsSlots sl{};
  const int pass = 16 * (64 / ch);
  for (int k = 0; k < g.n_colours; ++k) {
    const int lo = g.class_ptr[k], hi = g.class_ptr[k + 1];
    for (int p = lo; p < hi; p += pass) {
      if (sl.n >= 20) return false;
      sl.lo[sl.n] = (int16_t)p; sl.hi[sl.n] = (int16_t)hi;
      if (p + pass >= hi) sl.last_mask |= 1u << sl.n;
      ++sl.n;
    }
  }
  *out = sl;
  return sl.n > 0;
}

static int gibbs_plan_finish(const GibbsGraphShape& g, int n_chains, GibbsDrawPlan* p, const char* what) {
  p->grid = (int)ceil_div(n_chains, p->chains_per_block);
  if (p->lds > GIBBS_LDS_MAX) {
    set_error("gibbs: graph (n=%d, %d neighbour batches) needs %zu B of LDS%s > 160 KiB", g.n, g.n_batches, p->lds, what);
    return DVG_E_UNSUPPORTED;
  }
  return DVG_OK;
}

static int gibbs_plan_slots(const GibbsGraphShape& g, int n_chains, int ch, GibbsDrawPlan* p) {
  size_t fo[5];
  const size_t lds_fix = gibbs_fix_layout(g.n, fo) + 2 * (size_t)ch * ((g.n + 15) & ~15);
  p->form = GF_SLOTS;
  p->ch = ch;
  p->fix = g.max_batches <= GIBBS_NB && lds_fix <= GIBBS_LDS_MAX;
  // (18 slots: c5's graphs; the word registers of two more slots are what spills at 128 registers per wave)
  p->maxs = p->slots.n <= 18 ? 18 : 20;
  p->chains_per_block = ch; p->threads = 1024;
  p->lds = p->fix ? lds_fix : gibbs_lds_bytes(g.n, g.n_batches, g.n_colours, ch);
  return gibbs_plan_finish(g, n_chains, p, "");
}

// what a chain slot of the rolled form keeps in LDS behind the state rows: the held kind a row of flag bits, the field kind a
// float32 row of hs
static size_t gibbs_rolled_extra(const GibbsGraphShape& g, GibbsDrawKind kind) {
  return kind == GK_HELD ? sizeof(uint32_t) * (size_t)gibbs_held_words(g.n) : gibbs_field_kind(kind) ? gibbs_field_row_bytes(g.n) : 0;
}
static size_t gibbs_rolled_lds(const GibbsGraphShape& g, GibbsDrawKind kind, int lpc, int waves) {
  const int chains = waves * (64 / lpc);
  return gibbs_lds_bytes(g.n, g.n_batches, g.n_colours, chains) + (size_t)chains * gibbs_rolled_extra(g, kind);
}

static int gibbs_plan_rolled(const GibbsGraphShape& g, int n_chains, GibbsDrawKind kind, int lpc, int waves, GibbsDrawPlan* p) {
  if (gibbs_field_kind(kind)) {
    // The hs rows triple a chain's LDS: the largest WAVES of the list at this LPC, no larger than the one chosen, that fits
    // (1024 spins: ~105 KB of tables and 6 KB per chain -- 4 chains, not 16).  Nothing fits: the chosen one, reported below.
    int fit = 0;
#define DVG_GIBBS_ROLLED_FIT(LPC, W) \
  if (LPC == lpc && W <= waves && W > fit && gibbs_rolled_lds(g, kind, LPC, W) <= GIBBS_LDS_MAX) fit = W;
    DVG_GIBBS_ROLLED_KERNELS(DVG_GIBBS_ROLLED_FIT)
#undef DVG_GIBBS_ROLLED_FIT
    if (fit) waves = fit;
  }
  p->form = GF_ROLLED;
  p->lpc = lpc; p->waves = waves;
  p->chains_per_block = waves * (64 / lpc); p->threads = waves * 64;
  p->lds = gibbs_rolled_lds(g, kind, lpc, waves);
  return gibbs_plan_finish(g, n_chains, p,
                           kind == GK_HELD    ? " (the held flags of a conditional draw included)"
                           : gibbs_field_kind(kind) ? " (the field rows of a per-chain-field draw included)"
                                              : "");
}

// The held draw takes the plain draw's choices, with two exceptions: it has no chains-side-by-side form, so the large
// graphs' many-chain draws run the rolled kernel in 16-wave workgroups, and the A/B forms 3 and 4 count as 0.
// The annealed draw, weighed or not, and the traced draw: the same two exceptions.
// The per-chain-field draw: the table kind's plan under gibbs_generic = 1, whatever the option -- the rolled form alone keeps
// hs where a row per chain can stand in for it -- with the workgroup stepped down to what fits (gibbs_plan_rolled).  Weighed
// (GK_FIELD_WEIGH) it keeps that plan: the accumulators are registers, the rows rewritten where they lie.
int gibbs_draw_plan(const GibbsGraphShape& g, int n_chains, GibbsDrawKind kind, int64_t generic_option, GibbsDrawPlan* out) {
  GibbsDrawPlan& p = *out;
  p = GibbsDrawPlan{};
  const bool variant = kind != GK_PLAIN;
  // (option gibbs_generic = 1 forces the rolled reference schedule: A/B runs and the bit-exactness test of the fast one;
  // 2 = the fast schedule without its two-passes-side-by-side form)
  const int64_t form = gibbs_field_kind(kind) ? 1 : (variant && generic_option >= 3) ? 0 : generic_option;
  // (4: the chains-side-by-side schedule in 8-chain workgroups whatever the size: A/B runs; graphs whose classes do not
  // make slots take what 0 gives them)
  if (!variant && form == 4 && gibbs_make_slots(g, 8, &p.slots)) return gibbs_plan_slots(g, n_chains, 8, &p);
  // Graphs of more than 12 rows per lane (1024 spins: ~140 KB of tables, one 4-chain workgroup per CU) take the fast
  // schedule only for draws of at most 512 chains: it is the LATENCY form (c5-size graph, 2048 chains x 50 sweeps: 0.59 ms
  // alone against the rolled 16-wave form's 1.20) and costs the same CU-time -- but it takes every CU's LDS while it
  // runs, and the c5 step, whose encoder AND decoder forward hide behind a 1.2 ms draw on half the chip, got slower
  // with it (2.88 -> 3.01 ms: `profiles/r05_gibbs_c5_forms.txt`).  (3: the fast schedule whatever the size: A/B runs)
  if (form != 1 && g.lane_has && (g.lane_rows <= 12 || n_chains <= 512 || form == 3)) {
    const int lpc = g.lane_lpc, mb = g.lane_mb, rows = g.lane_rows;
    const int nr = form == 2 ? 1 : g.lane_nr;  // (2: a two-row image walked one row at a time -- empty rows and all)
    // Waves per workgroup.  Measured on the c2 step with the draw overlapped with the encoder forward: 4 -> 1.237 ms,
    // 8 -> 1.273, 16 -> 1.391: the sweep loop does contend for issue slots, fatter workgroups do not pay for the CUs they
    // free (round 5, c3: 8 or 2 waves instead of 4: step +0.2 ms).  Small graphs with few chains (c2: 128 spins, 256
    // chains -> 32 four-wave workgroups on 256 CUs): one wave per workgroup spreads the draw over four times as many
    // CUs at a few KB of tables each (c2 step 1.082 -> 1.060 ms).  Larger graphs keep four waves: every extra workgroup
    // stages its own copy of the tables.
    const bool small = gibbs_lane_lds_bytes(rows, mb, lpc, g.n, 0) <= 16 * 1024 && n_chains <= 1024 && rows <= 12;
    // (a lane image the fast form cannot serve -- more than 160 KiB of LDS: 20 rows x 5 batches at n_pad > 1216;
    // or a shape without an instantiation: two rows per step with a single small class -- falls through to the rolled
    // schedule, which serves every graph, instead of failing the draw)
#define DVG_GIBBS_LANE_PLAN(LPC, W, MB, NR, MAXS)                                                           \
  if (p.form != GF_LANE && lpc == LPC && mb == MB && nr == NR && rows <= MAXS && (W == 1) == small &&       \
      gibbs_lane_lds_bytes(rows, MB, LPC, g.n, W * (64 / LPC)) <= GIBBS_LDS_MAX) {                          \
    p.form = GF_LANE;                                                                                       \
    p.lpc = LPC; p.waves = W; p.mb = MB; p.nr = NR; p.maxs = MAXS;                                          \
  }
    DVG_GIBBS_LANE_KERNELS(DVG_GIBBS_LANE_PLAN)
#undef DVG_GIBBS_LANE_PLAN
    if (p.form == GF_LANE) {
      p.chains_per_block = p.waves * (64 / lpc); p.threads = p.waves * 64;
      p.lds = gibbs_lane_lds_bytes(rows, mb, lpc, g.n, p.chains_per_block);
      return gibbs_plan_finish(g, n_chains, &p, "");
    }
  }
  // The rolled schedule: graphs without a lane image (more than 20 rows per lane, more than 20 neighbours per spin).
  // Large graphs (c5: 1024 spins, 2|E| = 16 K -> ~105 KB of tables): one workgroup per CU fits, so the workgroup must
  // carry the CU's whole latency-hiding: 16 waves = 16 chains share one LDS copy of the graph (2 waves left 7/8 of
  // the issue slots empty: 7.3 ms per 2048-chain, 50-sweep draw).
  if (gibbs_lds_bytes(g.n, g.n_batches, g.n_colours, 4) > 72 * 1024) {
    // ... with static (class, pass) slots when the classes make at most 20 of them (gibbs_slot_kernel; option
    // gibbs_generic = 1 keeps the plain rolled kernel: the reference of the bit-exactness tests)
    if (!variant && form != 1 && gibbs_make_slots(g, 16, &p.slots)) return gibbs_plan_slots(g, n_chains, 16, &p);
    return gibbs_plan_rolled(g, n_chains, kind, 64, 16, &p);
  }
  // Lanes per chain: the smallest of 16 / 32 / 64 that covers the largest colour class in one pass, else 64; one wave per
  // workgroup for small graphs with few chains, as above.
  const bool small = gibbs_lds_bytes(g.n, g.n_batches, g.n_colours, 0) <= 16 * 1024 && n_chains <= 1024;
  return gibbs_plan_rolled(g, n_chains, kind, g.max_class <= 16 ? 16 : g.max_class <= 32 ? 32 : 64, small ? 1 : 4, &p);
}

int gibbs_exchange_plan(const GibbsGraphShape& g, int n_ladders, int n_replicas, int64_t generic_option, GibbsDrawPlan* out,
                        int* ladders_per_block) {
  GibbsDrawPlan& p = *out;
  const int R = n_replicas, n_chains = n_ladders * R;
  DVG_TRY(gibbs_draw_plan(g, n_chains, GK_TABLE, generic_option, &p));
  if (p.chains_per_block < R) {
    // (every one-wave entry of both lists has its four-wave twin)
    if (p.waves == 1 && 4 * p.chains_per_block >= R) {
      p.waves = 4;
      p.chains_per_block *= 4; p.threads = 4 * 64;
      p.lds = p.form == GF_LANE ? gibbs_lane_lds_bytes(g.lane_rows, p.mb, p.lpc, g.n, p.chains_per_block)
                                : gibbs_lds_bytes(g.n, g.n_batches, g.n_colours, p.chains_per_block);
    } else {
      p = GibbsDrawPlan{};
      DVG_TRY(gibbs_plan_rolled(g, n_chains, GK_TABLE, 64, 16, &p));
    }
  }
  const int per_block = p.chains_per_block / R;
  size_t o[3];
  p.lds = gibbs_exchange_lds_layout(p.lds, p.chains_per_block, o);
  p.grid = (int)ceil_div(n_ladders, per_block);
  if (ladders_per_block) *ladders_per_block = per_block;
  if (p.lds > GIBBS_LDS_MAX) {
    set_error("gibbs: graph (n=%d, %d neighbour batches) needs %zu B of LDS (the mailboxes of an exchange draw included) > 160 KiB",
              g.n, g.n_batches, p.lds);
    return DVG_E_UNSUPPORTED;
  }
  return DVG_OK;
}

}  // namespace dvg
