// The kernel form of every MFMA convolution layer of the two networks: decided ONCE per C-ABI call from (shape, training
// flag, option snapshot), and everything a (layer, pass, form) triple implies -- weight pack, BatchNorm partial rows,
// scratch sizes, launch geometry, launcher -- derived here and nowhere else.  encoder.cpp / decoder.cpp keep what is
// theirs: buffers, streams, fork/join order, the BN / activation passes, the composed layer's weight-space algebra.
// The VALU layers (encoder layer 0, decoder layer 3, the final ConvTranspose) are not GEMM forms and have no ConvLayer.
#pragma once
#include "conv.h"

namespace dvg {

//   CF_DIRECT  implicit GEMM over the 9 taps (conv_igemm.hip); behind the upsample: fused into the gather
//   CF_FOLD    Upsample(x2) + 3x3 as 4 class GEMMs with pre-summed taps (ConvArgs.fold)
//   CF_D22     3x3 on 2x2 images as one dense map per image (WM_CONVT_D22_FWD)
//   CF_LC0     ... composed with the Linear layer in front of it (decoder.cpp: Wc = Wlin . Weff)
//   CF_WINO2   Winograd F(2x2,3x3) (conv_wino.hip, conv_wino_wgrad.hip); behind the upsample 9 of 16 positions
//   CF_WINO4   Winograd F(4x4,3x3) (conv_wino4.hip, conv_wino4_wgrad.hip); behind the upsample 25 of 36 positions
enum ConvForm : int { CF_DIRECT = 0, CF_FOLD, CF_D22, CF_LC0, CF_WINO2, CF_WINO4, CF_COUNT };
enum ConvPass : int { PASS_FWD = 0, PASS_DGRAD, PASS_WGRAD };

// Options are relaxed atomics that may be flipped between calls, and a backward call runs on another thread than its
// forward: a C-ABI call reads them ONCE, here, and plans from the copy.
struct PlanOptions {
  int precision;    // conv_precision_mode()
  int launch_mode;  // conv_launch_mode(): operand form of the direct GEMMs, i.e. the format of their weight packs
  int64_t v[OPT_COUNT];  // every option's value, by Opt (common.h)
};
PlanOptions plan_options();

// M: output-resolution pixels of the batch; Cin, Cout: of the forward pass; L: log2 of the output side; ups: the input is
// stored at half resolution (nearest Upsample(x2) in front of the layer); convt: ConvTranspose2d checkpoint layout (the
// decoder's layers) instead of Conv2d; form: by ConvPass
struct ConvLayer {
  int64_t M;
  int Cin, Cout, L;
  bool ups, convt;
  ConvForm form[3];
  // CF_WINO4 forward / data-gradient launches of the encoder: the block shape of 32 tiles x 64 output channels instead of
  // 64 x 32 (conv_wino4.hip; same bits -- no part of the signature)
  bool block64[2] = {false, false};
};

// The planners (pure functions).  Encoder: y[1..3] (y[0], the VALU layer, is left alone); an evaluation-mode plan has no
// backward, its two gradient forms read CF_DIRECT.  Decoder: y[0..2]; N = decoder rows (batch x replicas).
void plan_encoder_layers(int64_t B, int n, bool training, const PlanOptions& o, ConvLayer y[4]);
void plan_decoder_layers(int64_t N, int n, const PlanOptions& o, ConvLayer y[3]);
// policy + shape of one encoder forward launch of a training call (dvg_dev_conv_wino_ok)
bool plan_enc_wino_fwd(int64_t M, int Cin, int Cout, int L, bool training, const PlanOptions& o);
// CUs an encoder Winograd launch of the pass is sized for (ConvArgs.wino_cus; 0: the launcher's default)
int plan_enc_wino_cus(const PlanOptions& o, ConvPass pass, bool training);
// the bit of dev option enc_wino4_mask that gives encoder layer l's (1..3) F(4x4,3x3) forward / data-gradient launch the
// 64-channel block shape: the bit of the form itself, 16 higher
inline int enc_wino4_block64_bit(int l, bool dgrad) { return 16 + (dgrad ? 2 + l : l - 1); }

// workspace layouts: the offset (in floats) of a buffer of `count` floats, in 256-byte granules
inline size_t bump(size_t& o, size_t count) {
  const size_t r = o;
  o += (count + 63) & ~(size_t)63;
  return r;
}

// ---- derived from (layer, pass, form) ----
// the pack a forward / data-gradient launch reads, and its size in floats
PackJob conv_layer_pack(const ConvLayer& y, ConvPass pass, const float* w, float* wp);
size_t conv_layer_pack_floats(const ConvLayer& y, ConvPass pass);
int conv_layer_stats_blocks(const ConvLayer& y);  // BatchNorm partial rows the forward launch writes
// the geometry half of the launch arguments -- M, Cin, Cout, L, ntaps, ups, poolsum, fold, wino_um, bias_mod of ConvArgs
// (set by launch_conv_layer), M, Cin, Cout, L, ntaps, ups, fold, ksplit of WgradArgs; the pointers, bias_perm, force_f32
// and wino_cus are the caller's
void conv_layer_wgrad_geometry(const ConvLayer& y, WgradArgs& wa);
// the scratch the layer's launches need, as running maxima: weight-gradient slabs, split-K buffer of the other two passes
void conv_layer_scratch(const ConvLayer& y, size_t& slabs, size_t& splitk);
// forward / data gradient: `a` carries the pointers (in, wp, bias, out, stats, splitk_ws) and wino_cus
int launch_conv_layer(const ConvLayer& y, ConvPass pass, ConvArgs a, hipStream_t s);
// weight gradient and the reduce pass that follows it, into the checkpoint layout grad_w (not CF_LC0: the composed
// weight's gradient is followed by the decoder's weight-space algebra, decoder.cpp launches it itself)
int launch_conv_layer_wgrad(const ConvLayer& y, const float* in, const float* dy, float* slabs, float* grad_w, int wino_cus, hipStream_t s);

// What of a plan determines the contents a forward call leaves in its workspace for the backward call: the forward and
// data-gradient forms (weight-gradient choices shape nothing there), the pack format and the flags below.  Bit 31 of the
// signature is the training flag (plan_forward_flag), the rest those fields as mixed-radix digits.
struct PlanKey { bool tail, l0_fused, training, mse; };
constexpr uint32_t PLAN_SIG_TRAINING = 1u << 31;
uint32_t plan_signature(const ConvLayer* y, int nlayers, const PlanOptions& o, const PlanKey& k);
// the error of a backward call whose signature differs from its forward's (returns DVG_E_INVALID)
int plan_mismatch_error(const char* who, const char* options, const char* dev_options, const char* also);

}  // namespace dvg
