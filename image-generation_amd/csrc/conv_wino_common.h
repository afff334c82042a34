// What the four Winograd translation units (conv_wino.hip, conv_wino4.hip: forward / data gradient; conv_wino_wgrad.hip,
// conv_wino4_wgrad.hip: weight gradient) decide in ONE place: how a CU budget becomes a persistent grid and whether its
// tile blocks are dealt dynamically, how a weight gradient's reduction is split into slabs, how a weight pack and the slab
// sum are launched, and the LDS address-space types they all cast through.
// The host part needs no device (tools/wino_geometry_check.cpp sweeps it under the sanitizers).
#pragma once
#include "conv.h"
#include "conv_tile.h"

namespace dvg {

// ------------------------------------------------------------------------------------------------------------- host
// The CU budget of a persistent grid of `ny` column blocks: 0 = the whole chip, at least one workgroup per column block
static inline int wino_cu_budget(int cus, int ny) {
  if (cus <= 0) cus = 256;
  if (cus < ny) cus = ny;
  return cus > 256 ? 256 : cus;
}
// ... its width: one workgroup per CU of the budget, at most one per tile block
static inline int wino_grid_width(int cus, int ny, int nblk) {
  int gx = wino_cu_budget(cus, ny) / ny;
  if (gx < 1) gx = 1;
  return gx > nblk ? nblk : gx;
}
// ... shrunk to its round count (the static deal): the narrowest grid that still needs ceil(nblk / gx) rounds
static inline int wino_grid_static(int gx, int nblk) {
  const int rounds = (nblk + gx - 1) / gx;
  return (nblk + rounds - 1) / rounds;
}

// The persistent grid of a forward / data-gradient launch: `gx` workgroups per column block and whether its tile blocks
// are dealt dynamically (the kernels: conv_wino.hip) or round-robin.  `may_deal`: the option, the launch's shape and a set
// of tile counters allow the dynamic deal.
// (The dynamic deal hands every workgroup TWO blocks up front: a launch of fewer than about three rounds keeps the
// static deal, where the grid is shrunk to its round count -- an evaluation forward at the 256-block threshold would
// otherwise be done by half the grid in two rounds.  Dynamic launches of one device must be ordered on ONE stream:
// the counters are a per-device pool that the launch's last workgroup re-zeroes.)
struct WinoGridPlan { int gx; bool dynamic; };
static inline WinoGridPlan wino_grid_plan(int cus, int ny, int nblk, bool may_deal) {
  WinoGridPlan p;
  p.gx = wino_grid_width(cus, ny, nblk);
  p.dynamic = may_deal && nblk >= 3 * p.gx;
  if (!p.dynamic) p.gx = wino_grid_static(p.gx, nblk);
  return p;
}
// ... with the launch's tile counters (null: round-robin; the pool hands out none before the device's streams exist)
struct WinoGrid { int gx; int* dyn; };
static inline WinoGrid wino_persistent_grid(int cus, int ny, int nblk, bool may_deal) {
  int* dyn = nullptr;
  if (opt(OPT_WINO_DYNAMIC) != 0 && wino_grid_plan(cus, ny, nblk, may_deal).dynamic) dyn = dyn_tile_counters();
  return WinoGrid{wino_grid_plan(cus, ny, nblk, dyn != nullptr).gx, dyn};
}

// The share of the chip a whole-CU grid of `wgs` workgroups was sized for (ProfScope: common.h)
static inline float wino_work_share(unsigned wgs) { return (float)(wgs > 256u ? 256u : wgs) / 256.0f; }

// The slab split of a weight gradient whose reduction runs over `chunks`, with `wgs` workgroups per slab: one workgroup per
// CU of the budget, every workgroup at least 8 chunks deep.  `want` slabs of `per` chunks; the last may be shorter, and
// `nsplit` of them are not empty.
struct WinoSlabs { int want, per, nsplit; };
static inline WinoSlabs wino_slab_split(int chunks, int wgs, int cus) {
  WinoSlabs g;
  g.want = cus / wgs;
  if (g.want < 1) g.want = 1;
  if (g.want > chunks / 8) g.want = chunks / 8 > 0 ? chunks / 8 : 1;
  g.per = (chunks + g.want - 1) / g.want;
  g.nsplit = (chunks + g.per - 1) / g.per;
  return g;
}

// Launch of a weight-pack kernel (w, map, u, extra...): one thread per (reduction channel, output channel) entry
template <typename Kern, typename... Extra>
static inline int launch_wino_pack(Kern pack_kernel, const float* w, const WeightMap& map, float* u, hipStream_t s, Extra... extra) {
  int64_t gx = ceil_div((int64_t)map.Ca * map.Cb, 256);
  if (gx > 1024) gx = 1024;
  DVG_LAUNCH(K_WEIGHT_PACK, pack_kernel, dim3((unsigned)gx), dim3(256), 0, s, w, map, u, extra...);
  return DVG_OK;
}

// Sum of the weight-gradient slabs [nslabs][positions][pairs] in place into slab 0 (conv_wino_wgrad.hip:
// wino_wgrad_slabsum_kernel); ups: the 16-position form behind the upsample, whose vanishing positions are never written
int launch_wino_wgrad_slabsum(float* slabs, int nslabs, int64_t pairs, int positions, int ups, hipStream_t s);

// ----------------------------------------------------------------------------------------------------------- device
typedef __attribute__((address_space(3))) void lds_void_t;
typedef __attribute__((address_space(3))) unsigned char lds_byte_t;
typedef __attribute__((address_space(3))) const f32x4 lds_cf32x4;
typedef __attribute__((address_space(3))) f32x4 lds_f32x4;
typedef __attribute__((address_space(3))) const float lds_cf32;
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) f32x2 lds_f32x2;

}  // namespace dvg
