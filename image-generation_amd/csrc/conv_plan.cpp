// conv_plan.h: the option snapshot, the two planners (all policy), and what follows from a (layer, pass, form) triple.
#include "conv_plan.h"

#include <algorithm>

namespace dvg {

PlanOptions plan_options() {
  PlanOptions o;
  o.precision = conv_precision_mode(); o.launch_mode = conv_launch_mode(0, 0);  // (the same for every shape)
  for (int i = 0; i < OPT_COUNT; ++i) o.v[i] = opt((Opt)i);
  return o;
}

// ------------------------------------------------------------------------------------------------------------ policy
namespace {
// The bf16-input mode means bf16-rounded operands for every forward / data-gradient launch: the float32 Winograd forms
// would silently compute those layers in float32 (and the direct kernel on the bf16 MFMA is the faster one there).  In
// the f32x3 mode they are strict float32 arithmetic on 4/9 of the multiplications: faster than the split direct kernel
// and at least as exact.  Weight gradients are float32 in every operand mode.
bool wino_mode_ok(const PlanOptions& o, ConvPass pass) { return pass == PASS_WGRAD || o.precision != 1; }

// encoder Winograd launches of a training call: from this many workgroups' worth of tile blocks up (measured, n = 512
// model: 1024 / 512 / 256 -> B = 512: 2.16 / 2.13 / 2.06 ms, B = 1024: 3.03 / 2.82 / 2.82, B = 2048: 4.67 / 4.60 / 4.53;
// c2: 0.920 / 0.924 / 0.953 -- 512 is the lowest value that costs c2 nothing: with its one 256-block launch switched the
// step measured 3.5 % slower, the draw's 128 one-wave workgroups leave the persistent grid 128 CUs there)
constexpr int WINO_MIN_BLOCKS = 512;

// Option enc_wino: 0 never, 1 every launch the shape allows, -1 (default) by size: evaluation-mode forward launches from
// 256 workgroups' worth of tile blocks (round 3), launches of a training call from WINO_MIN_BLOCKS (all of c3's,
// the larger ones of mid-size batches; small launches keep the direct form's finer tiles).  Inside a training step the
// form pays only with its grid sized to the CUs the launch can get (ConvArgs.wino_cus, the WINO_CUS_* constants): 256
// persistent workgroups beside the sampler's 64 resident ones leave 64 of them waiting for a CU for a whole round.
// `Cout`: of the launch (a data gradient's is the layer's Cin).
bool enc_wino_wanted(const PlanOptions& o, int64_t M, int Cout, ConvPass pass, bool training) {
  if (o.v[OPT_ENC_WINO] == 0 || !wino_mode_ok(o, pass)) return false;
  if (o.v[OPT_ENC_WINO] >= 1) return true;
  return conv_wino_blocks(M, Cout) >= (training ? WINO_MIN_BLOCKS : 256);
}

// Option enc_wino4 gates EVERY F(4x4,3x3) launch -- forward, data gradient and weight gradient, encoder and decoder --
// among the launches that run in the Winograd domain; which of them take it is a per-launch mask (dev options
// enc_wino4_mask / dec_wino4_mask, measured per launch inside the c3 step: options.cpp says why each bit is what it is).
bool wino4_bit(const PlanOptions& o, int64_t mask, int bit) { return o.v[OPT_ENC_WINO4] != 0 && ((mask >> bit) & 1); }

// The F(4x4,3x3) block shape of 32 tiles x 64 channels halves the input transforms per matrix operation and deals items of
// twice the work: a launch takes it where its mask bit is set, the shape allows and every workgroup of its CU budget still
// gets two items or more (below that the coarser deal costs what the transforms save).  `Cout`: of the launch.
bool wino4_block64(const PlanOptions& o, int l, bool dgrad, int64_t M, int Cin, int Cout, int L, int cus) {
  if (!wino4_bit(o, o.v[OPT_ENC_WINO4_MASK], enc_wino4_block64_bit(l, dgrad)) || !conv_wino4_block64_shape(M, Cin, Cout, L)) return false;
  return (int64_t)conv_wino4_stats_blocks(M) * (Cout / 64) >= 2 * (int64_t)(cus > 0 && cus < 256 ? cus : 256);
}

bool is_wino(ConvForm f) { return f == CF_WINO2 || f == CF_WINO4; }
// checkpoint layout of the layer's 9-tap weight, forward / data-gradient orientation
WeightMap map9(const ConvLayer& y, bool dgrad) {
  const int mode = y.convt ? (dgrad ? WM_CONVT_DGRAD : WM_CONVT_FWD) : (dgrad ? WM_CONV_DGRAD : WM_CONV_FWD);
  return dgrad ? WeightMap{mode, y.Cout, y.Cin, 9} : WeightMap{mode, y.Cin, y.Cout, 9};
}
}  // namespace

bool plan_enc_wino_fwd(int64_t M, int Cin, int Cout, int L, bool training, const PlanOptions& o) {
  return conv_wino_shape(M, Cin, Cout, L) && enc_wino_wanted(o, M, Cout, PASS_FWD, training);
}

int plan_enc_wino_cus(const PlanOptions& o, ConvPass pass, bool training) {
  // (a training call's forward runs beside the step's sampler draw, which holds its CUs: the tile blocks are dealt
  // dynamically, so the grid is sized to the chip and the workgroups that get their CU late, when the draw ends,
  // take what is left; under option wino_dynamic = 0 -- the static deal, A/B -- a quarter of the chip is left out)
  if (pass == PASS_FWD) return (training && o.v[OPT_WINO_DYNAMIC] == 0) ? 192 : 0;
  // (the layer's weight-gradient chain runs beside its data gradient on the side stream)
  if (pass == PASS_DGRAD) return o.v[OPT_ENC_DGRAD_CUS] > 0 ? (int)o.v[OPT_ENC_DGRAD_CUS] : WINO_CUS_ENC_DGRAD;
  return (int)o.v[OPT_ENC_WGRAD_CUS];
}

void plan_encoder_layers(int64_t B, int n, bool training, const PlanOptions& o, ConvLayer y[4]) {
  const int ch[5] = {1, 32, 64, 128, n};
  for (int l = 1; l < 4; ++l) {
    ConvLayer& c = y[l];
    c.M = B * (1024 >> (2 * l)); c.Cin = ch[l]; c.Cout = ch[l + 1]; c.L = 5 - l; c.ups = false; c.convt = false;
    c.form[PASS_FWD] = c.form[PASS_DGRAD] = c.form[PASS_WGRAD] = CF_DIRECT;
    c.block64[PASS_FWD] = c.block64[PASS_DGRAD] = false;
    if (plan_enc_wino_fwd(c.M, c.Cin, c.Cout, c.L, training, o))
      c.form[PASS_FWD] = wino4_bit(o, o.v[OPT_ENC_WINO4_MASK], l - 1) && conv_wino4_shape(c.M, c.Cin, c.Cout, c.L) ? CF_WINO4 : CF_WINO2;
    c.block64[PASS_FWD] = c.form[PASS_FWD] == CF_WINO4 &&
                          wino4_block64(o, l, false, c.M, c.Cin, c.Cout, c.L, plan_enc_wino_cus(o, PASS_FWD, training));
    if (!training) continue;  // (no backward follows an evaluation-mode forward)
    if (conv_wino_shape(c.M, c.Cout, c.Cin, c.L) && enc_wino_wanted(o, c.M, c.Cin, PASS_DGRAD, true))
      c.form[PASS_DGRAD] = wino4_bit(o, o.v[OPT_ENC_WINO4_MASK], 2 + l) && conv_wino4_shape(c.M, c.Cout, c.Cin, c.L) ? CF_WINO4 : CF_WINO2;
    c.block64[PASS_DGRAD] = c.form[PASS_DGRAD] == CF_WINO4 &&
                            wino4_block64(o, l, true, c.M, c.Cout, c.Cin, c.L, plan_enc_wino_cus(o, PASS_DGRAD, true));
    // (the weight gradient takes the form with the layer's other training launches: the size rule counts the FORWARD's
    // tile blocks, so under it the forward's shape has to qualify too)
    if (conv_wino_wgrad_shape(c.M, c.Cin, c.Cout, c.L) && enc_wino_wanted(o, c.M, c.Cout, PASS_WGRAD, true) &&
        (o.v[OPT_ENC_WINO] >= 1 || conv_wino_shape(c.M, c.Cin, c.Cout, c.L)))
      c.form[PASS_WGRAD] = wino4_bit(o, o.v[OPT_ENC_WINO4_MASK], 5 + l) && conv_wino4_wgrad_shape(c.M, c.Cin, c.Cout, c.L) ? CF_WINO4 : CF_WINO2;
  }
}

void plan_decoder_layers(int64_t N, int n, const PlanOptions& o, ConvLayer y[3]) {
  const int ch[4] = {n, 128, 64, 32};
  for (int l = 0; l < 3; ++l) {
    ConvLayer& c = y[l];
    c.M = N * ((int64_t)4 << (2 * l)); c.Cin = ch[l]; c.Cout = ch[l + 1]; c.L = l + 1; c.ups = l > 0; c.convt = true;
    c.block64[PASS_FWD] = c.block64[PASS_DGRAD] = false;  // (the decoder's F(4x4,3x3) launches have 32 output channels or 8-16 chunks)
    ConvForm base = CF_DIRECT;
    // Option dec_d22 = 0 keeps the 9-tap form for the first layer (A/B runs, tests).  Option dec_lc0: 0 never compose
    // the Linear layer with it, 1 always (tests), -1 (default) from 4096 rows up at c3's 256 latent spins -- measured
    // there in round 4 -- and from N n >= 2^20 in general: the two layers cost 2 (4 n^2 + 16 n C) FLOPs per row and
    // pass, the composed map 2 (4 n C), forming it ~128 C n^2 per step; at c5's n = 1024 the crossover measured between
    // 512 and 1024 rows, and at its 2048 rows the step went 2.57 -> 2.18 ms.  The composed form has the LDS-DMA GEMMs
    // only (their K-major float32 packs double as plain row-major matrices): every operand mode has them, the
    // register-staged A/B form does not.
    if (l == 0 && o.v[OPT_DEC_D22] != 0)
      base = o.v[OPT_DEC_LC0] != 0 && (o.v[OPT_DEC_LC0] > 0 || N >= 4096 || N * (int64_t)n >= (1 << 20)) && conv_pack_is_f32_kmajor(o.launch_mode) ? CF_LC0 : CF_D22;
    // option dec_fold = 0 keeps the upsample-fused 9-tap form (A/B runs)
    if (c.ups && o.v[OPT_DEC_FOLD] != 0 && conv_fold_ok(c.M / 4)) base = CF_FOLD;
    c.form[PASS_FWD] = c.form[PASS_DGRAD] = c.form[PASS_WGRAD] = base;
    // Option dec_wino: -1 (default) forward, data gradient and weight gradient of the layers behind the upsample from
    // 8192 decoder rows up; 1 whenever the shape allows, 0 never.  (Round 4's one-wave-per-SIMD data gradient measured
    // neutral inside the c3 step and stayed off; the two-waves-per-SIMD kernel of round 5 pays: 8.48 -> 8.32 ms, same box.)
    if (!c.ups || o.v[OPT_DEC_WINO] == 0 || (o.v[OPT_DEC_WINO] < 0 && N < 8192)) continue;
    if (wino_mode_ok(o, PASS_FWD) && conv_wino_shape(c.M, c.Cin, c.Cout, c.L))
      c.form[PASS_FWD] = wino4_bit(o, o.v[OPT_DEC_WINO4_MASK], l - 1) && c.L <= 3 && conv_wino4_shape(c.M, c.Cin, c.Cout, c.L) ? CF_WINO4 : CF_WINO2;
    if (wino_mode_ok(o, PASS_DGRAD) && conv_wino_shape(c.M, c.Cout, c.Cin, c.L))
      c.form[PASS_DGRAD] = wino4_bit(o, o.v[OPT_DEC_WINO4_MASK], l + 1) && c.L <= 3 && conv_wino4_shape(c.M, c.Cout, c.Cin, c.L) ? CF_WINO4 : CF_WINO2;
    if (conv_wino_wgrad_shape(c.M, c.Cin, c.Cout, c.L)) c.form[PASS_WGRAD] = CF_WINO2;  // (no F(4x4) weight gradient behind the upsample)
  }
}

// ------------------------------------------------------------------------------- derived from (layer, pass, form)
PackJob conv_layer_pack(const ConvLayer& y, ConvPass pass, const float* w, float* wp) {
  const bool d = pass == PASS_DGRAD;
  const ConvForm f = y.form[pass];
  const int Ca = d ? y.Cout : y.Cin, Cb = d ? y.Cin : y.Cout;
  if (f == CF_D22 || f == CF_LC0)  // (the composed weight is formed FROM the dense map's packs: decoder.cpp)
    return PackJob{w, wp, WeightMap{d ? WM_CONVT_D22_DGRAD : WM_CONVT_D22_FWD, 4 * Ca, 4 * Cb, 1}, 0, y.M / 4};
  if (f == CF_FOLD)  // (forward: 4 classes x M/4 source rows = M GEMM rows; data gradient: M/4 source rows)
    return PackJob{w, wp, WeightMap{d ? WM_CONVT_FOLD_DGRAD : WM_CONVT_FOLD_FWD, Ca, Cb, 16}, 0, d ? y.M / 4 : y.M};
  // PackJob.wino: Winograd launches read U = G g G^T; behind the upsample the F(4x4) pack keeps 25 of 36 positions
  return PackJob{w, wp, map9(y, d), 0, y.M, f == CF_WINO2 ? 1 : f == CF_WINO4 ? (y.ups ? 3 : 2) : 0};
}

size_t conv_layer_pack_floats(const ConvLayer& y, ConvPass pass) {
  const ConvForm f = y.form[pass];
  const int per = f == CF_DIRECT ? 9 : f == CF_WINO4 ? (y.ups ? 28 : 36) : 16;  // (fold: 16 (class, tap) pairs; dense: 4 x 4 pixel pairs)
  return conv_pack_floats((size_t)per * y.Cin * y.Cout);
}

int conv_layer_stats_blocks(const ConvLayer& y) {
  const ConvForm f = y.form[PASS_FWD];
  if (f == CF_WINO4) return conv_wino4_stats_blocks(y.M);
  if (f == CF_WINO2) return conv_wino_stats_blocks(y.M, y.Cout);
  if (f == CF_FOLD) return conv_stats_blocks_fold(y.M / 4, y.Cout);
  // dense 2x2 forms: the GEMM has M/4 rows of 4 C columns; a row block's partials [4 C][2] read as 4 rows of [C][2]
  if (f == CF_D22 || f == CF_LC0) return 4 * conv_stats_blocks(y.M / 4, 4 * y.Cout);
  return conv_stats_blocks(y.M, y.Cout);
}

void conv_layer_geometry(const ConvLayer& y, ConvPass pass, ConvArgs& a) {
  const bool d = pass == PASS_DGRAD;
  const ConvForm f = y.form[pass];
  a.M = y.M; a.Cin = d ? y.Cout : y.Cin; a.Cout = d ? y.Cin : y.Cout; a.L = y.L; a.ntaps = 9;
  a.ups = !d && y.ups; a.poolsum = d && y.ups;  // (data gradient behind the upsample: each 2x2 quad summed in the epilogue)
  a.fold = 0; a.wino_um = 0; a.bias_mod = 0;
  a.wino4_block64 = f == CF_WINO4 && !y.ups && y.block64[pass];
  if (f == CF_FOLD) { a.M = y.M / 4; a.L = y.L - 1; a.ntaps = d ? 16 : 4; a.ups = a.poolsum = 0; a.fold = d ? 2 : 1; }  // rows = SOURCE pixels
  if (f == CF_D22 || f == CF_LC0) {
    // rows = images, columns = (pixel, channel): the same memory as [M][C]; composed: straight from / to the spins
    a.M = y.M / 4; a.L = 0; a.ntaps = 1;
    const int Ci = f == CF_LC0 ? y.Cin : 4 * y.Cin, Co = 4 * y.Cout;
    a.Cin = d ? Co : Ci; a.Cout = d ? Ci : Co;
    if (!d && f == CF_D22) a.bias_mod = y.Cout;  // (the composed bias is a full row)
  }
  // behind the upsample: Winograd on the upsampled map (forward), the fine-grid data gradient with the 2x2 sum folded
  // into its output transform
  if (is_wino(f)) { a.ups = a.poolsum = 0; a.wino_um = y.ups ? (d ? 2 : 1) : 0; }
}

void conv_layer_wgrad_geometry(const ConvLayer& y, WgradArgs& wa) {
  const ConvForm f = y.form[PASS_WGRAD];
  wa.M = y.M; wa.Cin = y.Cin; wa.Cout = y.Cout; wa.L = y.L; wa.ntaps = 9; wa.ups = y.ups; wa.fold = 0;
  if (f == CF_FOLD) { wa.M = y.M / 4; wa.L = y.L - 1; wa.ntaps = 16; wa.ups = 0; wa.fold = 1; }
  if (f == CF_D22 || f == CF_LC0) { wa.M = y.M / 4; wa.Cin = f == CF_LC0 ? y.Cin : 4 * y.Cin; wa.Cout = 4 * y.Cout; wa.L = 0; wa.ntaps = 1; wa.ups = 0; }
  wa.ksplit = wa.fold ? wgrad_fold_ksplit(wa.M, wa.Cin, wa.Cout) : wgrad_ksplit(wa.M, wa.Cin, wa.Cout, wa.ntaps);
}

void conv_layer_scratch(const ConvLayer& y, size_t& slabs, size_t& splitk) {
  for (ConvPass pass : {PASS_FWD, PASS_DGRAD}) {
    if (is_wino(y.form[pass])) continue;
    ConvArgs a;
    conv_layer_geometry(y, pass, a);
    splitk = std::max(splitk, conv_splitk_floats(a.fold == 1 ? a.M * 4 : a.M, a.Cin, a.Cout, a.ntaps, a.poolsum));  // (GEMM rows over all classes)
  }
  const ConvForm f = y.form[PASS_WGRAD];
  WgradArgs wa;
  conv_layer_wgrad_geometry(y, wa);
  const size_t direct = (size_t)wa.ksplit * wa.ntaps * wa.Cin * wa.Cout;
  slabs = std::max(slabs, f == CF_WINO4 ? conv_wino4_wgrad_slab_floats(y.M, y.Cin, y.Cout) : f == CF_WINO2 ? conv_wino_wgrad_slab_floats(y.M, y.Cin, y.Cout, y.L) : direct);
}

int launch_conv_layer(const ConvLayer& y, ConvPass pass, ConvArgs a, hipStream_t s) {
  conv_layer_geometry(y, pass, a);
  if (y.form[pass] == CF_WINO4) return launch_conv_wino4(a, s);
  if (y.form[pass] == CF_WINO2) return launch_conv_wino(a, s);
  return launch_conv_igemm(a, s);
}

int launch_conv_layer_wgrad(const ConvLayer& y, const float* in, const float* dy, float* slabs, float* grad_w, int wino_cus, hipStream_t s) {
  const ConvForm f = y.form[PASS_WGRAD];
  DVG_REQUIRE(f != CF_LC0, "conv plan: the composed layer's weight gradient is the decoder's own sequence");
  if (f == CF_WINO4) return launch_conv_wino4_wgrad(in, dy, y.M, y.Cin, y.Cout, y.L, slabs, map9(y, false), grad_w, s, wino_cus);
  if (f == CF_WINO2) return launch_conv_wino_wgrad(in, dy, y.M, y.Cin, y.Cout, y.L, slabs, map9(y, false), grad_w, s, y.ups, wino_cus);
  WgradArgs wa;
  wa.in = in; wa.dy = dy; wa.slabs = slabs;
  conv_layer_wgrad_geometry(y, wa);
  DVG_TRY(launch_conv_wgrad(wa, s));
  if (f == CF_D22) return launch_wgrad_d22_reduce(slabs, wa.ksplit, y.Cin, y.Cout, grad_w, s);
  if (f == CF_FOLD) return launch_wgrad_fold_reduce(slabs, wa.ksplit, y.Cin, y.Cout, grad_w, s);
  return launch_wgrad_reduce(slabs, wa.ksplit, map9(y, false), grad_w, s);
}

// --------------------------------------------------------------------------------------------------------- signature
uint32_t plan_signature(const ConvLayer* y, int nlayers, const PlanOptions& o, const PlanKey& k) {
  uint32_t h = 0;  // mixed-radix digits: distinct plans never collide (3 layers: 6^6 x 8 x 8 < 2^31)
  auto push = [&](uint32_t digit, uint32_t radix) { h = h * radix + digit; };
  for (int l = 0; l < nlayers; ++l) { push((uint32_t)y[l].form[PASS_FWD], CF_COUNT); push((uint32_t)y[l].form[PASS_DGRAD], CF_COUNT); }
  push((uint32_t)o.launch_mode, 8); push(k.tail, 2); push(k.l0_fused, 2); push(k.mse, 2);
  return (h & ~PLAN_SIG_TRAINING) | (k.training ? PLAN_SIG_TRAINING : 0u);
}

int plan_mismatch_error(const char* who, const char* options, const char* dev_options, const char* also) {
  set_error("%s: a kernel-form option changed since the forward call on this workspace (dvg_set_option: %s; dvg_dev_set_option: %s)%s", who, options, dev_options, also);
  return DVG_E_INVALID;
}

}  // namespace dvg
