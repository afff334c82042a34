// The kernel forms of one MMD call (mmd.hip): decided ONCE per C-ABI call from (shape, option snapshot), and everything a
// form implies -- template parameters, column splits, grids, LDS images, loss-partial count, workspace layout, priced
// matrix work -- derived here and nowhere else.  mmd.hip keeps the kernels, the kernel argument (MmdArgs) and one
// dispatcher per kernel family that maps the plan's integers to an instantiation.
#pragma once
#include "common.h"

namespace dvg {

constexpr int MMD_BI = 32;          // rows (i) per block of the 32-row kernels
constexpr int MMD_BJ = 128;         // columns (j) per tile: 4 waves x 32
constexpr int MMD_PITCH = 33;
constexpr int MMD_I8_PANEL = 512;   // features of the int8 rows staged at once
constexpr int64_t MMD_TARGET_BLOCKS = 256;  // column splits of the pair kernels aim for this many blocks

// Options may be flipped between calls (the tests do, inside one process): a C-ABI call reads them ONCE, here.
// mmd_w128 / mmd_d256: -1 by size, 0 never, 1 wherever the shape allows; mmd_gram_fp4: off / on.
struct MmdOptions { int w128, d256; bool gram_fp4; };
MmdOptions mmd_options();

//   MP_F32     mmd_main_kernel<nfb>: the float32 body alone (d beyond the spin path's LDS budget)
//   MP_SLICED  mmd_pair_kernel<nfb>: spin body over d / (32 nfb) feature slices, float32 body for general rows
//   MP_FQ      mmd_pair_fq_kernel<nfbw>: feature-quarter spin body (d = 128, 256, 384, 512)
//   MP_W128    mmd_pair_w128_kernel<nst, nft, one, gram == MG_FP4>: 128-row blocks (large spin problems), with
//              mmd_main_kernel<gated_nfb> launched behind it for rows that turn out not to be +-1
enum MmdPairForm : int { MP_F32 = 0, MP_SLICED, MP_FQ, MP_W128 };
//   MD_F32     mmd_distsum_kernel
//   MD_SPIN    mmd_distsum_spin_kernel<dist_ns>
//   MD_SPIN256 mmd_distsum_spin256_kernel<dist_ns, gram == MG_FP4>: 256-row blocks
enum MmdDistForm : int { MD_F32 = 0, MD_SPIN, MD_SPIN256 };
// the matrix pipe of the exact spin Gram, for the kernels that have the choice (MD_SPIN256, MP_W128)
enum MmdGram : int { MG_INT8 = 0, MG_FP4 };

struct MmdLaunch {
  unsigned grid[3];
  int logical[3];  // the gated float32 launch: the grid its blocks walk (MmdArgs.vgx / vgy / vgz); other launches: 0
  size_t lds;      // dynamic LDS bytes (MP_W128's pair launch: W128<...>::LDS_BYTES of the instantiation instead)
};

struct MmdPlan {
  int64_t nx, ny;
  int d;
  bool spin;  // the shape is served by the +-1 kernels (the float32 bodies stand down on the device flag)
  MmdPairForm pair;
  int nfb, nfbw, nst, nft;  // template parameters of the pair form (those it does not have: 0)
  bool one;
  int gated_nfb;  // NFB of the gated float32 launch behind MP_W128 (other forms: 0, no such launch)
  MmdDistForm dist;
  int dist_ns;    // NS / NST of the distance-sum form (MD_F32: 0)
  MmdGram gram;
  int splits;       // column splits of the pair launch and of the gated launch behind it (MmdArgs.S)
  int slices;       // feature slices of the pair launch (grid z)
  int dist_splits;  // column splits of the distance-sum launch
  int loss_parts;   // loss partials the final kernel sums: the largest count any layout of this plan writes
  int gram_passes, bf16_terms;  // how often the spin pair kernel computes the x-row Gram; bf16 products per pair and feature
  MmdLaunch prep, distsum, pair_launch, gated, final_grad;  // (final_grad: with a gradient asked for; without: one block)
  int64_t ztb_x;  // 32-row blocks of x in the transposed copy (whole 128-row tiles): where y starts
  size_t off_sq, off_coef, off_dist, off_loss, off_grad, off_flag, off_zi8, off_zt, off_tab, off_zi4, total;
};

// pure: the same arguments give the same plan
MmdPlan mmd_plan(int64_t nx, int64_t ny, int d, const MmdOptions& o);

// Executed matrix work of the pair launch.  Spin forms, in bf16-MFMA-equivalent FLOPs (what bench.py prices against the
// dense bf16 peak): the int8 Gram of every visited pair (x rows against all rows, y rows against y rows; gram_passes times
// for the x rows) and bf16_terms products per pair and feature of the gradient GEMM.  mmd_f32_work: Gram + gradient
// GEMM of the float32 body.
void mmd_spin_flops(const MmdPlan& p, bool grad, double* int8_flops, double* bf16_flops);
double mmd_spin_work(const MmdPlan& p, bool grad);  // the int8 Gram at twice the bf16 rate
double mmd_f32_work(const MmdPlan& p);

}  // namespace dvg
