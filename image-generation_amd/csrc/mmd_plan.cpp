// The MMD call's plan (mmd_plan.h): all of its policy -- thresholds, split counts, which shape takes which form -- and
// every size derived from it.  Host code only.
#include "mmd_plan.h"

namespace dvg {

MmdOptions mmd_options() {
  auto tri = [](int64_t v) { return v < 0 ? -1 : (v ? 1 : 0); };
  return MmdOptions{tri(opt(OPT_MMD_W128)), tri(opt(OPT_MMD_D256)), opt(OPT_MMD_GRAM_FP4) != 0};
}

// ---- the LDS images, each written once ----
static size_t max2(size_t a, size_t b) { return a > b ? a : b; }
static size_t i8_panel_bytes(int d) { return (size_t)MMD_BJ * ((d < MMD_I8_PANEL ? d : MMD_I8_PANEL) + 16); }  // one Z panel of int8 rows
// float32 pair body (mmd_main_body<nfb>): Z tile, X tile, G^T, row sums, loss partials
static size_t lds_f32_body(int nfb) {
  return sizeof(float) * (size_t)(MMD_BJ * MMD_PITCH + MMD_BI * MMD_PITCH + nfb * 32 * MMD_PITCH + 4 * 32 + 2) + sizeof(double) * 256;
}
// spin pair body (mmd_pm1_body<nfb>; fq: mmd_pm1_fq_body<nfb / 4>): both pair tables, row sums, loss partials, the resident
// X rows, one Z panel overlaid with G^T; fq: that overlay in 16-byte units and the weight-fragment exchange behind it
static size_t lds_spin_body(int d, int nfb, bool fq) {
  size_t zg = max2(i8_panel_bytes(d), sizeof(float) * nfb * 32 * MMD_PITCH);
  if (fq) zg = (zg + 15) / 16 * 16 + 16 * 24 * 64;
  return 2 * (size_t)(d + 1) * 16 + sizeof(float) * 128 + sizeof(double) * 256 + (size_t)MMD_BI * (d + 16) + zg;
}
// distance-sum kernels: 2 KiB of reduction scratch in front of the float32 tiles every one of them can fall back to ...
static size_t lds_dist_f32() { return 2048 + sizeof(float) * (MMD_BJ + MMD_BI) * MMD_PITCH; }
// ... of the int8 tiles (mmd_distsum_kernel), of the distance table + one Z panel (mmd_distsum_spin_kernel), of the table
// in whole KiB + two chunks of 32 rows (mmd_distsum_spin256_kernel)
static size_t lds_dist_i8(int d) { return 2048 + (size_t)(MMD_BJ + MMD_BI) * ((d < MMD_I8_PANEL ? d : MMD_I8_PANEL) + 16); }
static size_t lds_dist_spin(int d) { return 2048 + ((size_t)(d + 1) * 4 + 15) / 16 * 16 + i8_panel_bytes(d); }
static size_t lds_dist_spin256(int d) { return 2048 + ((size_t)(d + 1) * 4 + 1023) / 1024 * 1024 + 2 * (size_t)32 * d; }
static size_t lds_prep_fused(int d) { return (size_t)32 * (d + 16); }

static MmdLaunch launch_of(int64_t gx, int64_t gy, int64_t gz, size_t lds) {
  return MmdLaunch{{(unsigned)gx, (unsigned)gy, (unsigned)gz}, {0, 0, 0}, lds};
}

MmdPlan mmd_plan(int64_t nx, int64_t ny, int d, const MmdOptions& o) {
  MmdPlan p{};
  p.nx = nx; p.ny = ny; p.d = d;
  p.spin = d <= 1024;  // LDS: table + resident X rows + one Z panel
  const int fbt = d / 32;
  const int64_t rbx = ceil_div(nx, MMD_BI), rb32 = rbx + ceil_div(ny, MMD_BI);  // 32-row blocks = the 128-row kernel's chunks
  const int64_t rb128x = ceil_div(nx, 128), rb128 = rb128x + ceil_div(ny, 128);  // 128-row blocks = the 32-row kernels' tiles
  const int64_t tiles = rb128, chunks = rb32;

  // float32 body: 16 feature blocks (512 accumulator registers) would spill
  const int f32_nfb = fbt <= 2 ? 2 : (fbt <= 4 ? 4 : 8);
  const int f32_slices = (fbt + f32_nfb - 1) / f32_nfb;
  // column splits of the 32-row pair kernels: aim for MMD_TARGET_BLOCKS blocks, never more splits than tiles
  int64_t s32 = ceil_div(MMD_TARGET_BLOCKS, rbx * f32_slices);
  if (s32 > tiles) s32 = tiles;
  if (s32 < 1) s32 = 1;
  if (s32 > 16) s32 = 16;

  // 128-row-block pair kernel: d = 128 .. 512 in steps of 128 (16 d / 32 accumulator registers per lane), and enough
  // rows of x that 128-row blocks fill the chip with at most 4 column splits of >= 16 chunks each.
  // d = 1024: the rows still fit the registers -- 128 of them hold a lane's 1024 int8 features -- and the LDS image fits
  // with 128-feature slices of G^T, W128<32, 4>: eight feature slices per row block, each redoing the int8 Gram (32 of its
  // 48 MFMAs per chunk).  256-feature slices (four of them: the Gram redone 4 instead of 8 times, 48 instead of 40 KB
  // staged for 64 instead of 48 MFMAs per chunk) need the LDS of one pair table, W128<32, 8, true>: possible when no
  // block's chunk range spans the x / y boundary, i.e. when the x chunks are a whole number of column splits (c5's
  // per-GPU slice, 2048 + 2048 rows: 64 + 64 chunks in 4 splits of 32).
  auto splits_wanted = [&](int64_t z) {
    int64_t S = ceil_div(MMD_TARGET_BLOCKS, rb128x * z);
    if (S > chunks / 16) S = chunks / 16;
    return S < 1 ? (int64_t)1 : S;
  };
  const int64_t split_cap = o.w128 == 1 ? 16 : 4;
  auto capped = [&](int64_t S) { return S > split_cap ? split_cap : S; };
  int z128 = d == 1024 ? 8 : 1;
  if (d == 1024 && rbx % ceil_div(chunks, capped(splits_wanted(4))) == 0) z128 = 4;
  const int64_t s128 = splits_wanted(z128);
  // (the kernel addresses both chunk images through 32-bit buffer offsets: the int8 rows and the bf16 transposed copy,
  // 2 (nx + ny) d bytes, must stay below 2^31 -- larger problems keep the 32-row kernels' 64-bit pointers)
  const bool w128_shape = d % 128 == 0 && (d <= 512 || d == 1024) && (int64_t)(nx + ny) * (int64_t)d * 2 < 2147483647LL;
  const bool w128 = w128_shape && (o.w128 == 1 || (o.w128 != 0 && s128 <= 4 && rb128x * s128 * z128 >= 128));

  // distance sum by the 256-row-block spin kernel
  const bool d256 = p.spin && o.d256 != 0 && d % 128 == 0 && d <= 512 && (ceil_div(nx + ny, 256) >= 32 || o.d256 == 1) &&
                    (nx + ny) * (int64_t)d < 2147483647LL;
  // FP4 Gram: the packed row pitches with a 1 KiB DMA piece per wave (d / 2 = 128, 256 bytes).  The copy's place in the
  // workspace depends on the shape alone: the option may be flipped between calls on one workspace.
  const bool fp4_shape = p.spin && (d == 256 || d == 512);
  p.gram = fp4_shape && (d256 || w128) && o.gram_fp4 ? MG_FP4 : MG_INT8;

  // ---- the pair form ----
  int64_t pair_rows = rb32;
  p.splits = (int)s32;
  p.slices = f32_slices;  // (MP_FQ: what its float32 body needs, NFB = min(8, 4 nfbw) = f32_nfb at these widths)
  if (w128) {
    // One feature slice per block wherever the accumulators fit the 512-register file (d = 512: 256 of them hold G^T,
    // the compiler places the Gram tile and the operands in the other half without spills): the Gram and the lookups
    // are then computed once.
    p.pair = MP_W128;
    p.nst = fbt; p.nft = fbt / z128; p.one = d == 1024 && z128 == 4;
    p.gated_nfb = f32_nfb;
    p.splits = (int)capped(s128);
    p.slices = z128;
    pair_rows = rb128;
  } else if (p.spin && d % 128 == 0 && d <= 512) {
    p.pair = MP_FQ;
    p.nfbw = d / 128;
  } else if (p.spin) {
    // feature blocks per slice: the largest of 8/4/2/1 that divides d / 32 (no feature guards in the spin body; 16 blocks
    // = 256 accumulator registers makes the compiler shuffle accumulators through scratch)
    p.pair = MP_SLICED;
    p.nfb = fbt % 8 == 0 ? 8 : (fbt % 4 == 0 ? 4 : (fbt % 2 == 0 ? 2 : 1));
    p.slices = fbt / p.nfb;
  } else {
    p.pair = MP_F32;
    p.nfb = f32_nfb;
  }
  const size_t pair_lds = p.pair == MP_SLICED ? max2(lds_spin_body(d, p.nfb, false), lds_f32_body(p.nfb))
                        : p.pair == MP_FQ     ? max2(lds_spin_body(d, 4 * p.nfbw, true), lds_f32_body(f32_nfb))
                        : p.pair == MP_F32    ? lds_f32_body(p.nfb) : 0;
  p.pair_launch = launch_of(pair_rows, p.splits, p.slices, pair_lds);
  if (w128) {
    // General (not +-1) rows cannot be known on the host without a sync: the float32 kernel is launched behind the spin
    // kernel with the same split count and stands down on the device flag; a capped 1-D grid whose blocks walk the
    // logical grid (it writes the same loss_part / grad_part slots when it does run).
    const int64_t total = rb32 * p.splits * f32_slices;
    p.gated = launch_of(total < 512 ? total : 512, 1, 1, lds_f32_body(f32_nfb));
    p.gated.logical[0] = (int)rb32; p.gated.logical[1] = p.splits; p.gated.logical[2] = f32_slices;
  }
  p.gram_passes = w128 ? z128 : 1;  // (the 128-row-block kernel recomputes the x-row Gram per feature slice)
  p.bf16_terms = !p.spin ? 0 : (w128 ? 2 : 3);

  // The pair kernels number their loss partials by their own grids and exactly one layout runs (the 128-row kernel or
  // the float32 kernel behind it): the slots the other layouts would have filled must read as zero in the final sum.
  int64_t parts = s32 * rb32;
  if (w128 && p.splits * z128 * rb128 > parts) parts = p.splits * z128 * rb128;
  if (w128 && p.splits * rb32 > parts) parts = p.splits * rb32;
  p.loss_parts = (int)parts;
  const int64_t grad_slabs = p.splits > s32 ? p.splits : s32, numel = nx * (int64_t)d;
  p.final_grad = launch_of(p.splits > 1 ? (ceil_div(numel, 256) > 2048 ? 2048 : ceil_div(numel, 256)) : 1, 1, 1, 0);

  // ---- pass 1 (distance sum): spin-capable shapes launch the folded 128-row form, ceil(T/2) x S1 blocks of about
  // (T+1)/S1 tiles each, two blocks per CU wanted; other shapes one block per 32-row block
  int64_t GX1, S1;
  if (d256) {
    p.dist = MD_SPIN256; p.dist_ns = fbt;
    GX1 = 64;  // 8 chunk streams (one per XCD) x 64 blocks of equal work: exactly two resident blocks per CU
    S1 = 8;
  } else if (p.spin) {
    p.dist = MD_SPIN; p.dist_ns = d <= 128 ? 4 : (d <= 512 ? 16 : 32);
    GX1 = (tiles + 1) / 2;
    S1 = ceil_div(512, GX1);
    if (S1 > tiles + 1) S1 = tiles + 1;
    if (S1 > 32) S1 = 32;
  } else {
    p.dist = MD_F32;
    GX1 = rb32;
    S1 = ceil_div(1024, GX1);
    if (S1 > tiles) S1 = tiles;
    if (S1 > 16) S1 = 16;
  }
  if (S1 < 1) S1 = 1;
  p.dist_splits = (int)S1;
  p.distsum = launch_of(GX1, S1, 1, max2(lds_dist_f32(), p.dist == MD_SPIN256 ? lds_dist_spin256(d) : p.dist == MD_SPIN ? lds_dist_spin(d) : lds_dist_i8(d)));

  // row norms, int8 copy, +-1 flag (spin shapes: and the transposed bf16 copy, in one pass over the rows)
  const int64_t ztb_y = ceil_div(ny, MMD_BJ) * 4;
  p.ztb_x = ceil_div(nx, MMD_BJ) * 4;
  p.prep = p.spin ? launch_of(p.ztb_x + ztb_y, 1, 1, lds_prep_fused(d)) : launch_of(ceil_div(nx + ny, 4), 1, 1, 0);

  // ---- workspace ----
  size_t off = 0;
  auto take = [&](size_t bytes) { const size_t r = off; off = align_up(off + bytes, 256); return r; };
  p.off_sq = take(sizeof(float) * (size_t)(nx + ny));
  p.off_coef = take(sizeof(float) * 16);
  p.off_dist = take(sizeof(double) * (size_t)(S1 * GX1));
  p.off_loss = take(sizeof(double) * 3 * (size_t)parts);
  p.off_grad = take(grad_slabs > 1 ? sizeof(float) * (size_t)grad_slabs * (size_t)nx * (size_t)d : 0);
  p.off_flag = take(sizeof(int));
  p.off_zi8 = take((size_t)(nx + ny) * (size_t)d);
  p.off_zt = take(p.spin ? (size_t)(p.ztb_x + ztb_y) * (size_t)d * 32 * sizeof(uint16_t) : 0);
  p.off_tab = take(p.spin ? 2 * (size_t)(d + 1) * 16 : 0);
  p.off_zi4 = take(fp4_shape ? (size_t)(nx + ny) * (size_t)(d / 2) : 0);
  p.total = off;
  return p;
}

void mmd_spin_flops(const MmdPlan& p, bool grad, double* int8_flops, double* bf16_flops) {
  const double nx = (double)p.nx, ny = (double)p.ny, d = (double)p.d;
  *int8_flops = 2.0 * (p.gram_passes * nx * (nx + ny) + ny * ny) * d;
  *bf16_flops = grad ? p.bf16_terms * 2.0 * nx * (nx + ny) * d : 0.0;
}
double mmd_spin_work(const MmdPlan& p, bool grad) {
  double i8, b16;
  mmd_spin_flops(p, grad, &i8, &b16);
  return 0.5 * i8 + b16;
}
double mmd_f32_work(const MmdPlan& p) {
  const double N = (double)(p.nx + p.ny);
  return 2.0 * N * N * p.d + 2.0 * (double)p.nx * N * p.d;
}

}  // namespace dvg
