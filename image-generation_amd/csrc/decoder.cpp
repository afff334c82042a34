// dvg_decoder_fwd / dvg_decoder_bwd: Decoder.forward of /root/reference/src/decoder.py:54-62 and its backward.
//   Linear(n,4n) as a 1-tap MFMA GEMM writing NHWC (N,2x2,n) directly;
//   layers 0-2 (n->128 @2x2, 128->64 @4x4, 64->32 @8x8): MFMA implicit GEMM with the x2 nearest upsample of the
//   previous stage fused into the gather (never materialised); layer 3 (32->1 @16x16) and the final 1->1 @32x32
//   ConvTranspose: VALU kernels.  Each of layers 0-3 is followed by BN(batch stats) -> Dropout2d -> LeakyReLU.
//   Backward data-gradients of the upsample-fused layers sum each 2x2 quad in the MFMA epilogue.
#include <algorithm>

#include "conv_plan.h"
#include "kernels.h"

using namespace dvg;

namespace {

struct DecPlan {
  int64_t N;
  int n;
  int ch[5];
  int64_t M[4];
  int L[4];
  int nblk[4];
  size_t X0, Y[4], Xs[4], mean[4], invstd[4], stats[4], mask[4];
  size_t wp_lin, wpd_lin, bias_lin, wp[3], wpd[3];
  size_t dXbuf, dYl[4], slabs, partA, partB[4], partL, partW, partF, partT, msep, splitk;
  int ksplit_lin;
  ConvLayer conv[3];  // layers 0-2: geometry and kernel form per pass (conv_plan.h); layer 3 and the final one are VALU layers
  uint32_t signature[2];  // what the backward relies on the forward having done (conv_plan.h); [1]: the fused-MSE kind of call pair
  // Large batches: Linear(n, 4n) and layer 0 have nothing but a reshape between them, so the pair is ONE linear map per
  // image, spins (n) -> the 4 x 128 pre-BatchNorm values, with the composed weight Wc = Wlin . Weff (a 2 n x 4n x 512
  // weight-space product per step).  Forward, data gradient and weight gradient then cost 3 x 2 N n 512 FLOPs instead of
  // 3 x 2 N (n 4n + 4n 512); the gradients of BOTH original parameter tensors follow by the chain rule in weight space
  // (dWlin = dWc . Weff^T, dWeff = Wlin^T . dWc + blin (x) dbc).  X0 is never materialised.
  bool lc0;   // = layer 0 runs in the composed form (CF_LC0, all three passes)
  bool tail;  // layer 2's BN/Dropout/LeakyReLU folded into layer 3's kernels (special.hip: DecActIn)
  size_t WcT, Wc, bc, dbc, dWc, dWcT, T1, dWeff, partC;
  size_t total_floats;
};

DecPlan dec_plan(int64_t N, int n, const PlanOptions& opts) {
  DecPlan p{};
  p.N = N; p.n = n;
  const int ch[5] = {n, 128, 64, 32, 1};
  for (int i = 0; i < 5; ++i) p.ch[i] = ch[i];
  p.tail = opts.v[OPT_DEC_TAIL_FUSED] != 0;
  plan_decoder_layers(N, n, opts, p.conv);
  p.lc0 = p.conv[0].form[PASS_FWD] == CF_LC0;
  // (the decoder's plan does not depend on the training flag, and its backward has never asked for a training-mode forward)
  for (int mse = 0; mse < 2; ++mse) p.signature[mse] = plan_signature(p.conv, 3, opts, PlanKey{p.tail, false, true, mse != 0});
  size_t o = 0;
  p.X0 = bump(o, (size_t)N * 4 * n);
  p.wp_lin = bump(o, conv_pack_floats((size_t)n * 4 * n));
  p.wpd_lin = bump(o, conv_pack_floats((size_t)n * 4 * n));
  p.bias_lin = bump(o, (size_t)4 * n);
  p.ksplit_lin = wgrad_ksplit(N, n, 4 * n, 1);
  size_t max_slab = (size_t)p.ksplit_lin * n * 4 * n;
  size_t max_dx = (size_t)N * 4 * n;
  size_t max_split = std::max(conv_splitk_floats(N, n, 4 * n, 1, 0), conv_splitk_floats(N, 4 * n, n, 1, 0));
  const int cmax = 4 * n;
  for (int l = 0; l < 4; ++l) {
    p.L[l] = l + 1;
    p.M[l] = N * ((int64_t)4 << (2 * l));
    const int C = ch[l + 1];
    p.nblk[l] = l == 3 ? dec_conv3_blocks(N) : conv_layer_stats_blocks(p.conv[l]);
    p.Y[l] = bump(o, (size_t)p.M[l] * C);
    p.Xs[l] = bump(o, (size_t)p.M[l] * C);
    p.mean[l] = bump(o, C);
    p.invstd[l] = bump(o, C);
    p.stats[l] = bump(o, (size_t)(p.nblk[l] + BN_FOLD_ROWS) * C * 2);  // + scratch rows of launch_bn_finalize
    p.mask[l] = bump(o, (size_t)N * C);
    if (l < 3) {
      p.wp[l] = bump(o, conv_layer_pack_floats(p.conv[l], PASS_FWD));
      p.wpd[l] = bump(o, conv_layer_pack_floats(p.conv[l], PASS_DGRAD));
      conv_layer_scratch(p.conv[l], max_slab, max_split);
    }
    const size_t act = (size_t)p.M[l] * C;
    if (act > max_dx) max_dx = act;  // dXs[l] has the shape of Xs[l]
  }
  if (p.lc0) {  // the composed weight (both orientations) and bias, their gradients, the weight-space products
    const int C = ch[1];
    p.WcT = bump(o, (size_t)4 * C * n);
    p.Wc = bump(o, (size_t)n * 4 * C);
    p.bc = bump(o, (size_t)4 * C);
    p.dbc = bump(o, (size_t)4 * C);
    p.dWc = bump(o, (size_t)n * 4 * C);
    p.dWcT = bump(o, (size_t)4 * C * n);
    p.T1 = bump(o, (size_t)4 * n * n);
    p.dWeff = bump(o, (size_t)4 * n * 4 * C);
    p.partC = bump(o, (size_t)EW_BLOCKS * 4 * C);
  }
  p.dXbuf = bump(o, max_dx);
  // one dY buffer per layer: a layer's weight gradient (side stream) may still be reading its dY when the data-gradient
  // chain reaches the next layers, and a shared buffer would make the caller's stream wait on the side stream
  for (int l = 0; l < 4; ++l) p.dYl[l] = bump(o, (size_t)p.M[l] * ch[l + 1]);
  p.slabs = bump(o, max_slab);
  p.partA = bump(o, (size_t)EW_BLOCKS * 2 * cmax);
  // one bias-gradient partial buffer per layer: their column sums run on the side stream, behind the main chain
  for (int l = 0; l < 4; ++l) p.partB[l] = bump(o, (size_t)(l >= 2 ? STREAM_BLOCKS : EW_BLOCKS) * ch[l + 1]);  // (l = 2, 3: rows of the fused tail)
  p.partL = bump(o, (size_t)EW_BLOCKS * cmax);
  p.partF = bump(o, (size_t)EW_BLOCKS * 10);
  p.partW = bump(o, (size_t)STREAM_BLOCKS * 288);
  // the fused tail (dvg_decoder_fwd_mse_ex): the 1-channel stage's (sum dz, sum dz zhat) partials, written by the FORWARD call
  // and read by the backward call (a buffer of their own: partA is every other stage's scratch), and the MSE partials (doubles)
  p.partT = bump(o, (size_t)STREAM_BLOCKS * 2);
  p.msep = bump(o, (size_t)STREAM_BLOCKS * 2);
  p.splitk = bump(o, max_split);
  p.total_floats = o;
  return p;
}

int check_common(const dvg_decoder_params_t* p, int n, int64_t N, const void* ws, size_t ws_bytes, const DecPlan& pl) {
  DVG_REQUIRE(p && ws, "decoder: null params/workspace");
  DVG_REQUIRE(n >= 32 && n % 32 == 0 && n <= 4096, "decoder: n_latents=%d must be a multiple of 32", n);
  DVG_REQUIRE(N >= 1 && N <= (1 << 22), "decoder: batch*replicas %lld out of range", (long long)N);
  DVG_REQUIRE(p->lin_w && p->lin_b, "decoder: null linear parameter");
  for (int l = 0; l < 5; ++l) DVG_REQUIRE(p->conv_w[l] && p->conv_b[l], "decoder: null conv parameter %d", l);
  for (int l = 0; l < 4; ++l)
    DVG_REQUIRE(p->bn_g[l] && p->bn_b[l] && p->bn_rm[l] && p->bn_rv[l], "decoder: null BN parameter %d", l);
  if (ws_bytes < pl.total_floats * sizeof(float)) {
    set_error("decoder: workspace %zu < %zu bytes", ws_bytes, pl.total_floats * sizeof(float));
    return DVG_E_WORKSPACE;
  }
  return DVG_OK;
}

}  // namespace

extern "C" size_t dvg_decoder_workspace_bytes(int64_t N, int n_latents) {
  dvg::side_stream_warm();  // the backward's fork/join context exists before any step is captured
  if (N < 1 || n_latents < 32 || n_latents % 32) return 0;
  return dec_plan(N, n_latents, plan_options()).total_floats * sizeof(float);
}

namespace {
// Everything of a forward call that depends on the parameters (and the dropout stream) alone: the weight packs, the
// composed Linear o ConvTranspose weights and bias, the Dropout2d keep-masks.  dvg_decoder_fwd runs it at its head;
// dvg_decoder_prepare runs it ahead of time, beside whatever produces the spins.
int dec_prologue(const dvg_decoder_params_t* p, int n, int64_t N, int training, const float* const dropout_keep[4],
                 uint64_t seed, uint64_t offset, float* W, const DecPlan& pl, const dvg_step_state_t* dyn, hipStream_t s) {
  {  // all weight packs of the network (forward AND data-gradient layouts) in one launch
    PackJob jobs[8];
    jobs[0] = PackJob{p->lin_w, W + pl.wp_lin, WeightMap{WM_LIN_FWD, n, 4 * n, 1}, 0, N};
    jobs[1] = PackJob{p->lin_w, W + pl.wpd_lin, WeightMap{WM_LIN_DGRAD, 4 * n, n, 1}, 0, N};
    for (int l = 0; l < 3; ++l)
      for (ConvPass pass : {PASS_FWD, PASS_DGRAD}) jobs[2 + 2 * l + pass] = conv_layer_pack(pl.conv[l], pass, p->conv_w[l], W + (pass == PASS_FWD ? pl.wp[l] : pl.wpd[l]));
    DVG_TRY(launch_weight_pack_multi(jobs, 8, s));
  }
  if (pl.lc0) {
    // composed weight, both orientations (K-major operands of the forward and of the data-gradient GEMM), and bias:
    //   WcT[o][i] = sum_j Weff[j][o] Wlin[i][j]   rows of the dense-2x2 forward pack [o][j]  x  the Linear dgrad pack [i][j]
    //   Wc[i][o]                                    rows of the Linear dgrad pack [i][j]       x  the dense-2x2 forward pack
    const int C = pl.ch[1];
    ConvArgs a;
    a.bias = nullptr; a.stats = nullptr; a.L = 0; a.ntaps = 1; a.ups = 0; a.poolsum = 0; a.splitk_ws = nullptr;
    a.force_f32 = 1;  // products of WEIGHTS: float32 in every operand mode (the modes are about the network's activations)
    a.in = W + pl.wp[0]; a.wp = W + pl.wpd_lin; a.out = W + pl.WcT; a.M = 4 * C; a.Cin = 4 * n; a.Cout = n;
    DVG_TRY(launch_conv_igemm(a, s));
    a.in = W + pl.wpd_lin; a.wp = W + pl.wp[0]; a.out = W + pl.Wc; a.M = n; a.Cin = 4 * n; a.Cout = 4 * C;
    DVG_TRY(launch_conv_igemm(a, s));
    DVG_TRY(launch_lc0_bias(p->lin_b, W + pl.wp[0], p->conv_b[0], n, C, W + pl.bc, s));
  }
  if (training) {  // Dropout2d keep-masks of all four stages: copied in (parity runs) or drawn on device, one launch
    bool given = dropout_keep != nullptr;
    for (int l = 0; l < 4 && given; ++l) given = dropout_keep[l] != nullptr;
    if (given) {
      for (int l = 0; l < 4; ++l)
        DVG_CHECK_HIP(hipMemcpyAsync(W + pl.mask[l], dropout_keep[l], sizeof(float) * (size_t)N * pl.ch[l + 1],
                                     hipMemcpyDeviceToDevice, s));
    } else {
      DVG_REQUIRE(dropout_keep == nullptr || (!dropout_keep[0] && !dropout_keep[1] && !dropout_keep[2] && !dropout_keep[3]),
                  "decoder_fwd: give all four dropout masks or none");
      float* masks[4] = {W + pl.mask[0], W + pl.mask[1], W + pl.mask[2], W + pl.mask[3]};
      DVG_TRY(launch_dropout_masks(N, &pl.ch[1], masks, seed, offset, dyn ? &dyn->dropout_offset : nullptr, s));
    }
  }
  return DVG_OK;
}

uint64_t prologue_signature(const dvg_decoder_params_t* p, int n, int64_t N, int training, uint64_t seed, uint64_t offset,
                            const dvg_step_state_t* dyn, const DecPlan& pl) {
  uint64_t h = 0xcbf29ce484222325ull;
  auto mix = [&](uint64_t v) { h = (h ^ v) * 0x100000001b3ull; };
  mix((uint64_t)n); mix((uint64_t)N); mix((uint64_t)training); mix(seed); mix(dyn ? ~0ull : offset); mix((uint64_t)(uintptr_t)dyn);
  mix(pl.signature[0]); mix((uint64_t)(uintptr_t)p->lin_w); mix((uint64_t)(uintptr_t)p->conv_w[0]);  // (the signature covers the operand mode: the pack format)
  return h;
}
}  // namespace

// The weight-only part of the NEXT dvg_decoder_fwd_ex(prepared = 1) on this workspace, enqueued on `stream` now: a
// stream of the caller's that is forked off its main stream where the step starts, so that the packs, weight-space
// products and mask draws (~190 us at B R = 32768) run beside the encoder instead of between the spins and the
// decoder's first GEMM; the forward call joins them (an event recorded here, waited for there).  The parameters must not
// change between the two calls; device-drawn dropout masks only (injected masks: call dvg_decoder_fwd, which copies them).
extern "C" int dvg_decoder_prepare(const dvg_decoder_params_t* p, int n, int64_t N, int training, uint64_t seed,
                                   uint64_t offset, void* ws, size_t ws_bytes, const dvg_step_state_t* dyn,
                                   dvg_stream_t stream) {
  const DecPlan pl = dec_plan(N > 0 ? N : 1, (n >= 32 && n % 32 == 0) ? n : 32, plan_options());
  DVG_TRY(check_common(p, n, N, ws, ws_bytes, pl));
  hipStream_t s = (hipStream_t)stream;
  DVG_TRY(dec_prologue(p, n, N, training, nullptr, seed, offset, (float*)ws, pl, dyn, s));
  return prep_arm(ws, prologue_signature(p, n, N, training, seed, offset, dyn, pl), s);
}

namespace {
// The MSE against `images` ([N / R][1024]; replica r of image b = decoder row b R + r) fused behind the decoder
// (dvg_decoder_fwd_mse_ex / dvg_decoder_bwd_mse_ex): the reconstruction and its gradient are never written.
struct MseTail { const float* images; int R; float grad_scale; float* loss_out; };
float mse_gscale(const MseTail& mt, int64_t N) { return (float)(2.0 * (double)mt.grad_scale / ((double)N * 1024.0)); }  // (dvg_mse_fwd_bwd's)

int decoder_fwd_impl(const dvg_decoder_params_t* p, int n, const float* spins, int64_t N, int training,
                     const float* const dropout_keep[4], uint64_t seed, uint64_t offset, float* out, const MseTail* mt,
                     void* ws, size_t ws_bytes, const dvg_step_state_t* dyn, int prepared, dvg_stream_t stream) {
  const DecPlan pl = dec_plan(N > 0 ? N : 1, (n >= 32 && n % 32 == 0) ? n : 32, plan_options());
  // the caller's declaration for THIS call that `spins` holds only +-1 (dvg_decoder_declare_spins): taken whatever becomes
  // of the call, recorded for the backward call on this workspace
  const int spin_pm1 = spin_promise_note_forward(ws) ? 1 : 0;
  DVG_TRY(check_common(p, n, N, ws, ws_bytes, pl));
  conv_precision_note_forward(ws);
  plan_note_forward(ws, pl.signature[mt != nullptr]);
  DVG_REQUIRE(spins && (out || mt), "decoder_fwd: null spins/out");
  if (mt) {
    DVG_REQUIRE(training, "decoder_fwd_mse: training-mode calls only (the fused tail produces the backward's sums)");
    DVG_REQUIRE(pl.tail, "decoder_fwd_mse: needs option dec_tail_fused != 0");
    DVG_REQUIRE(mt->images && mt->loss_out && mt->R >= 1 && N % mt->R == 0, "decoder_fwd_mse: images / loss_out / R (N=%lld R=%d)", (long long)N, mt->R);
  }
  hipStream_t s = (hipStream_t)stream;
  float* W = (float*)ws;
  {
    // a prologue in flight on this workspace is joined whatever it was prepared for (it writes what this call reads
    // or rewrites); it is USED only when the caller says so and it was prepared for exactly this call
    bool armed = false, matched = false;
    DVG_TRY(prep_join(ws, prologue_signature(p, n, N, training, seed, offset, dyn, pl), s, &armed, &matched));
    DVG_REQUIRE(!prepared || (armed && matched && dropout_keep == nullptr),
                "decoder_fwd: prepared = 1 without a matching dvg_decoder_prepare on this workspace (same parameters, N, "
                "training flag, dropout seed / offset, kernel-form options; device-drawn masks)");
    if (!prepared) DVG_TRY(dec_prologue(p, n, N, training, dropout_keep, seed, offset, W, pl, dyn, s));
  }
  if (!pl.lc0) {  // Linear(n, 4n) -> X0 (N, 2x2 Morton, n)
    ConvArgs a;
    a.in = spins; a.wp = W + pl.wp_lin; a.bias = p->lin_b; a.bias_perm = n; a.out = W + pl.X0; a.stats = nullptr;  // bias'[p*n + c] = b[c*4 + p]
    a.M = N; a.Cin = n; a.Cout = 4 * n; a.L = 0; a.ntaps = 1; a.ups = 0; a.poolsum = 0;
    a.splitk_ws = W + pl.splitk;
    a.spin_a = spin_pm1;
    DVG_TRY(launch_conv_igemm(a, s));
  }
  const float* x = W + pl.X0;
  for (int l = 0; l < 4; ++l) {
    const int C = pl.ch[l + 1];
    if (l < 3) {
      ConvArgs a;
      a.in = x; a.wp = W + pl.wp[l]; a.bias = p->conv_b[l]; a.out = W + pl.Y[l];
      a.stats = training ? W + pl.stats[l] : nullptr;
      if (l == 0 && pl.lc0) { a.in = spins; a.wp = W + pl.WcT; a.bias = W + pl.bc; a.spin_a = spin_pm1; }  // straight from the spins through the composed weight
      a.splitk_ws = W + pl.splitk; a.wino_cus = WINO_CUS_DEC;
      DVG_TRY(launch_conv_layer(pl.conv[l], PASS_FWD, a, s));
    } else if (pl.tail) {  // layer 2's activation happens while layer 3 stages its input (Xs[2] is never written)
      const DecActIn in{W + pl.Y[2], W + pl.mean[2], W + pl.invstd[2], p->bn_g[2], p->bn_b[2], training ? W + pl.mask[2] : nullptr};
      DVG_TRY(launch_dec_conv3_fwd_act(in, N, p->conv_w[3], p->conv_b[3], W + pl.Y[3], W + pl.stats[3], s));
    } else {
      DVG_TRY(launch_dec_conv3_fwd(x, N, p->conv_w[3], p->conv_b[3], W + pl.Y[3], W + pl.stats[3], s));
    }
    DVG_TRY(launch_bn_finalize(W + pl.stats[l], pl.nblk[l], C, pl.M[l], training, W + pl.mean[l], W + pl.invstd[l],
                               p->bn_rm[l], p->bn_rv[l], p->bn_nbt[l], s));
    const float* mask = training ? W + pl.mask[l] : nullptr;
    if ((l == 2 || l == 3) && pl.tail) continue;  // (activated by the next layer's kernels while they stage their input)
    DVG_TRY(launch_dec_bn_act_fwd(W + pl.Y[l], pl.M[l], C, 2 * pl.L[l], W + pl.mean[l], W + pl.invstd[l], p->bn_g[l],
                                  p->bn_b[l], mask, W + pl.Xs[l], s));
    x = W + pl.Xs[l];
  }
  if (mt) {
    // final layer -> MSE -> the final layer's data gradient -> the 1-channel stage's backward sums, one pass per image
    const DecActIn in3{W + pl.Y[3], W + pl.mean[3], W + pl.invstd[3], p->bn_g[3], p->bn_b[3], W + pl.mask[3]};
    DVG_TRY(launch_dec_tail_mse_sums(in3, N, p->conv_w[4], p->conv_b[4], mt->images, mt->R, mse_gscale(*mt, N), W + pl.partT,
                                     (double*)(W + pl.msep), s));
    DVG_TRY(launch_mse_final((const double*)(W + pl.msep), dec_final_dgrad_blocks(N), 1.0 / ((double)N * 1024.0), mt->loss_out, s));
  } else if (pl.tail) {
    const DecActIn in3{W + pl.Y[3], W + pl.mean[3], W + pl.invstd[3], p->bn_g[3], p->bn_b[3], training ? W + pl.mask[3] : nullptr};
    DVG_TRY(launch_dec_final_fwd_act(in3, N, p->conv_w[4], p->conv_b[4], out, s));
  } else {
    DVG_TRY(launch_dec_final_fwd(x, N, p->conv_w[4], p->conv_b[4], out, s));
  }
  return DVG_OK;
}
}  // namespace

extern "C" int dvg_decoder_declare_spins(const void* ws, int pm1) {
  DVG_REQUIRE(ws, "decoder_declare_spins: null workspace");
  spin_promise_declare(ws, pm1 != 0);
  return DVG_OK;
}

extern "C" int dvg_decoder_fwd_ex(const dvg_decoder_params_t* p, int n, const float* spins, int64_t N, int training,
                                  const float* const dropout_keep[4], uint64_t seed, uint64_t offset, float* out, void* ws,
                                  size_t ws_bytes, const dvg_step_state_t* dyn, int prepared, dvg_stream_t stream) {
  return decoder_fwd_impl(p, n, spins, N, training, dropout_keep, seed, offset, out, nullptr, ws, ws_bytes, dyn, prepared, stream);
}

extern "C" int dvg_decoder_fwd_mse_ex(const dvg_decoder_params_t* p, int n, const float* spins, int64_t N,
                                      const float* const dropout_keep[4], uint64_t seed, uint64_t offset, const float* images,
                                      int R, float grad_scale, float* loss_out, void* ws, size_t ws_bytes,
                                      const dvg_step_state_t* dyn, int prepared, dvg_stream_t stream) {
  const MseTail mt{images, R, grad_scale, loss_out};
  return decoder_fwd_impl(p, n, spins, N, 1, dropout_keep, seed, offset, nullptr, &mt, ws, ws_bytes, dyn, prepared, stream);
}

extern "C" int dvg_decoder_fwd(const dvg_decoder_params_t* p, int n, const float* spins, int64_t N, int training,
                               const float* const dropout_keep[4], uint64_t seed, uint64_t offset, float* out, void* ws,
                               size_t ws_bytes, const dvg_step_state_t* dyn, dvg_stream_t stream) {
  return dvg_decoder_fwd_ex(p, n, spins, N, training, dropout_keep, seed, offset, out, ws, ws_bytes, dyn, 0, stream);
}

extern "C" int dvg_decoder_bwd(const dvg_decoder_params_t* p, int n, const float* spins, int64_t N,
                               const float* grad_out, const dvg_decoder_grads_t* g, float* grad_spins, void* ws,
                               size_t ws_bytes, dvg_stream_t stream) {
  return dvg_decoder_bwd_ex(p, n, spins, N, grad_out, g, grad_spins, ws, ws_bytes, 0, stream);
}

extern "C" int dvg_stream_join_side(dvg_stream_t stream) {
  hipStream_t s = (hipStream_t)stream, s2 = side_stream(s);
  if (s2 != s) DVG_TRY(stream_order_after(s, s2));
  return DVG_OK;
}

namespace {
int decoder_bwd_impl(const dvg_decoder_params_t* p, int n, const float* spins, int64_t N, const float* grad_out,
                     const MseTail* mt, const dvg_decoder_grads_t* g, float* grad_spins, void* ws, size_t ws_bytes,
                     int defer_join, dvg_stream_t stream) {
  const DecPlan pl = dec_plan(N > 0 ? N : 1, (n >= 32 && n % 32 == 0) ? n : 32, plan_options());
  DVG_TRY(check_common(p, n, N, ws, ws_bytes, pl));
  DVG_REQUIRE(conv_precision_matches_forward(ws), "decoder_bwd: the GEMM operand mode (dvg_set_conv_precision) changed since the forward call on this workspace");
  if (!plan_matches_forward(ws, pl.signature[mt != nullptr]))
    return plan_mismatch_error("decoder_bwd", "dec_fold / dec_d22 / dec_lc0 / dec_wino / enc_wino4", "igemm_dma / dec_tail_fused / dec_wino4_mask", ", or the forward call was not of the same kind (dvg_decoder_fwd_ex / dvg_decoder_fwd_mse_ex)");
  DVG_REQUIRE(spins && (grad_out || mt) && g, "decoder_bwd: null argument");
  const int spin_pm1 = spin_promise_of_forward(ws) ? 1 : 0;  // what the forward call on this workspace was promised about `spins`
  if (mt) DVG_REQUIRE(pl.tail && mt->images && mt->R >= 1 && N % mt->R == 0, "decoder_bwd_mse: images / R (N=%lld R=%d), option dec_tail_fused", (long long)N, mt->R);
  DVG_REQUIRE(g->lin_w && g->lin_b, "decoder_bwd: null linear gradient buffer");
  for (int l = 0; l < 5; ++l) DVG_REQUIRE(g->conv_w[l] && g->conv_b[l], "decoder_bwd: null conv gradient buffer %d", l);
  for (int l = 0; l < 4; ++l) DVG_REQUIRE(g->bn_g[l] && g->bn_b[l], "decoder_bwd: null BN gradient buffer %d", l);
  hipStream_t s = (hipStream_t)stream;
  hipStream_t s2 = side_stream(s);  // weight-gradient chain (streams.cpp); the data-gradient chain stays on `s`
  ColsumBatch sums;  // the bias / small-weight column sums of the whole call: ONE launch at the end of the side chain
  float* W = (float*)ws;
  float* dX = W + pl.dXbuf;
  float* partA = W + pl.partA;
  float* partW = W + pl.partW;

  // final ConvTranspose2d(1,1): gradient wrt Xs[3] (16x16, quad-summed) on the caller's stream; its weight/bias
  // gradient on the side stream (main-chain kernel first: see the fork note below)
  {
    hipEvent_t start = nullptr;
    if (s2 != s) DVG_TRY(stream_mark(s, &start));
    const DecActIn in3{W + pl.Y[3], W + pl.mean[3], W + pl.invstd[3], p->bn_g[3], p->bn_b[3], W + pl.mask[3]};
    if (mt) {
      // (the sums are in partT since the forward call: dvg_decoder_fwd_mse_ex)
    } else if (pl.tail) {  // ... as the 1-channel stage's BatchNorm-backward sums (no reduce pass below; dX itself is not stored)
      DVG_TRY(launch_dec_final_dgrad_bn(grad_out, N, p->conv_w[4], in3, partA, s));
    } else {
      DVG_TRY(launch_dec_final_dgrad(grad_out, N, p->conv_w[4], dX, s));
    }
    if (s2 != s) DVG_TRY(stream_wait_mark(s2, start));
    if (mt) DVG_TRY(launch_dec_final_wgrad_mse(in3, N, p->conv_w[4], p->conv_b[4], mt->images, mt->R, mse_gscale(*mt, N), W + pl.partF, s2));
    else if (pl.tail) DVG_TRY(launch_dec_final_wgrad_act(in3, N, grad_out, W + pl.partF, s2));  // (Xs[3] does not exist)
    else DVG_TRY(launch_dec_final_wgrad(W + pl.Xs[3], N, grad_out, W + pl.partF, s2));
    DVG_REQUIRE(sums.add2(W + pl.partF, EW_BLOCKS, 10, 9, g->conv_w[4], 1, g->conv_b[4]), "decoder_bwd: column-sum batch full");
  }

  // (the fused conv3 backward leaves its two column sums to the batch below)
  for (int l = 3; l >= 0; --l) {
    const int Cin = pl.ch[l], C = pl.ch[l + 1];
    const float* Y = W + pl.Y[l];
    const float* Xs = W + pl.Xs[l];
    const float* mask = W + pl.mask[l];  // backward only exists for a training-mode forward
    float* dY = W + pl.dYl[l];
    const DecActIn in2{W + pl.Y[2], W + pl.mean[2], W + pl.invstd[2], p->bn_g[2], p->bn_b[2], W + pl.mask[2]};
    if (l == 2 && pl.tail) {
      // the (sum dz, sum dz zhat) partials came out of layer 3's fused backward below; dY2 = its second pass
      DVG_TRY(launch_colsum2(partA, dec_tail_blocks(N), 2 * C, C, g->bn_b[l], C, g->bn_g[l], s));
      DVG_TRY(launch_dec_conv3_bwd_apply(in2, N, W + pl.dYl[3], p->conv_w[3], g->bn_b[l], g->bn_g[l], dY, W + pl.partB[l], s));
    } else if (l == 3 && pl.tail) {
      // the 1-channel stage: its sums came out of the final layer's data-gradient pass above; dY3 = that pass again
      const DecActIn in3{W + pl.Y[3], W + pl.mean[3], W + pl.invstd[3], p->bn_g[3], p->bn_b[3], W + pl.mask[3]};
      DVG_TRY(launch_colsum2(mt ? W + pl.partT : partA, dec_final_dgrad_blocks(N), 2 * C, C, g->bn_b[l], C, g->bn_g[l], s));
      if (mt)
        DVG_TRY(launch_dec_tail_mse_apply(in3, N, p->conv_w[4], p->conv_b[4], mt->images, mt->R, mse_gscale(*mt, N), g->bn_b[l],
                                          g->bn_g[l], dY, W + pl.partB[l], s));
      else
        DVG_TRY(launch_dec_final_dgrad_apply(grad_out, N, p->conv_w[4], in3, g->bn_b[l], g->bn_g[l], dY, W + pl.partB[l], s));
    } else {
      DVG_TRY(launch_dec_bn_act_bwd_reduce(Y, Xs, pl.M[l], C, 2 * pl.L[l], W + pl.mean[l], W + pl.invstd[l], p->bn_g[l],
                                           p->bn_b[l], mask, dX, partA, s));
      DVG_TRY(launch_colsum2(partA, EW_BLOCKS, 2 * C, C, g->bn_b[l], C, g->bn_g[l], s));
      DVG_TRY(launch_dec_bn_act_bwd_apply(Y, Xs, pl.M[l], C, 2 * pl.L[l], W + pl.mean[l], W + pl.invstd[l], p->bn_g[l],
                                          p->bn_b[l], mask, dX, g->bn_b[l], g->bn_g[l], dY, W + pl.partB[l], s));
    }
    // Fork: dY is ready.  The caller's-stream kernel is enqueued BEFORE the side-stream ones: when the call is being
    // captured into a hipGraph, the first child captured after a fork inherits the parent's hardware queue, and a
    // data-gradient chain that changes queue at every layer pays a cross-queue signal (~10-15 us) per hop.
    hipEvent_t dy_ready = nullptr;
    if (s2 != s) DVG_TRY(stream_mark(s, &dy_ready));
    const float* xin = l == 0 ? W + pl.X0 : W + pl.Xs[l - 1];
    if (l == 3) {
      // data gradient and weight-gradient partials in ONE pass over the images on the caller's stream (special.hip); only
      // the column sums go to the side stream (no fork here: they are in the batch at the end of the side chain).  (The two
      // separate kernels this replaced were retired in round 3.)
      const int w3_blocks = stream_blocks(N);  // partial rows of the weight gradient
      if (pl.tail) DVG_TRY(launch_dec_conv3_bwd_reduce(in2, N, dY, p->conv_w[3], partW, partA, s));
      else DVG_TRY(launch_dec_conv3_bwd(xin, N, dY, p->conv_w[3], dX, partW, s));
      DVG_REQUIRE(sums.add(W + pl.partB[l], pl.tail ? dec_final_dgrad_blocks(N) : EW_BLOCKS, C, C, 1.0f, g->conv_b[l], 0, 0) &&
                  sums.add(partW, w3_blocks, 288, 288, 1.0f, g->conv_w[3], 32, 9),  // [tap][ci] -> [ci][tap]
                  "decoder_bwd: column-sum batch full");
      continue;
    }
    // Composed Linear + layer 0: one data-gradient GEMM straight to the spins, one weight-gradient GEMM for dWc, and the
    // gradients of the two original weights / biases by the chain rule in weight space (side stream).
    const bool lc0 = l == 0 && pl.lc0;
    if (!lc0 || grad_spins) {
      ConvArgs a;
      a.in = dY; a.wp = W + (lc0 ? pl.Wc : pl.wpd[l]); a.bias = nullptr; a.out = lc0 ? grad_spins : dX; a.stats = nullptr;
      a.splitk_ws = W + pl.splitk; a.wino_cus = WINO_CUS_DEC;
      DVG_TRY(launch_conv_layer(pl.conv[l], PASS_DGRAD, a, s));
    }
    if (s2 != s) DVG_TRY(stream_wait_mark(s2, dy_ready));
    DVG_REQUIRE(sums.add(W + pl.partB[l], (l == 2 && pl.tail) ? dec_tail_blocks(N) : EW_BLOCKS, C, C, 1.0f, g->conv_b[l], 0, 0),
                "decoder_bwd: column-sum batch full");
    if (!lc0) {
      DVG_TRY(launch_conv_layer_wgrad(pl.conv[l], xin, dY, W + pl.slabs, g->conv_w[l], WINO_CUS_DEC, s2));
      continue;
    }
    const int n4 = 4 * n, C4 = 4 * C;
    // dbc[o] = column sums of dY seen as [N][4 C]
    DVG_TRY(launch_rowsum_partial(dY, N, C4, W + pl.partC, s2));
    DVG_TRY(launch_colsum(W + pl.partC, EW_BLOCKS, C4, C4, 1.0f, W + pl.dbc, 0, 0, s2));
    DVG_TRY(launch_lc0_lin_bias_grad(W + pl.dbc, W + pl.wpd[0], n, C, g->lin_b, s2));
    // dWc[i][o] = sum_images spins[i] dY[o]  (and its transpose)
    WgradArgs wa;
    wa.in = spins; wa.dy = dY; wa.slabs = W + pl.slabs; wa.spin_x = spin_pm1;
    conv_layer_wgrad_geometry(pl.conv[0], wa);
    DVG_TRY(launch_conv_wgrad(wa, s2));
    DVG_TRY(launch_slab_sum(W + pl.slabs, wa.ksplit, n, C4, W + pl.dWc, W + pl.dWcT, s2));
    ConvArgs b;
    b.bias = nullptr; b.stats = nullptr; b.L = 0; b.ntaps = 1; b.ups = 0; b.poolsum = 0; b.splitk_ws = nullptr;
    b.force_f32 = 1;  // weight-space products (see the forward call)
    // T1[j][i] = sum_o Weff[j][o] dWc[i][o]: rows of the dense-2x2 data-gradient pack [j][o] x dWc as the K-major operand
    b.in = W + pl.wpd[0]; b.wp = W + pl.dWc; b.out = W + pl.T1; b.M = n4; b.Cin = C4; b.Cout = n;
    DVG_TRY(launch_conv_igemm(b, s2));
    DVG_TRY(launch_lc0_rows_to_linear(W + pl.T1, n, g->lin_w, s2));
    // dWeff[j][o] = sum_i Wlin[i][j] dWc[i][o]: rows of the Linear forward pack [j][i] x dWc^T [o][i]
    b.in = W + pl.wp_lin; b.wp = W + pl.dWcT; b.out = W + pl.dWeff; b.M = n4; b.Cin = n; b.Cout = C4;
    DVG_TRY(launch_conv_igemm(b, s2));
    DVG_TRY(launch_lc0_rank1_add(W + pl.dWeff, p->lin_b, W + pl.dbc, n, C, s2));  // (+ the Linear bias' share of X0)
    DVG_TRY(launch_wgrad_d22_reduce(W + pl.dWeff, 1, Cin, C, g->conv_w[l], s2));
  }
  // dX now holds the gradient wrt X0 (N, 4n) in (p, c) order.  Linear backward (composed form: done with layer 0 above):
  if (!pl.lc0) {
    hipEvent_t dx_ready = nullptr;  // dX is final
    if (s2 != s) DVG_TRY(stream_mark(s, &dx_ready));
    if (grad_spins) {
      ConvArgs a;
      a.in = dX; a.wp = W + pl.wpd_lin; a.bias = nullptr; a.out = grad_spins; a.stats = nullptr;
      a.M = N; a.Cin = 4 * n; a.Cout = n; a.L = 0; a.ntaps = 1; a.ups = 0; a.poolsum = 0;
      a.splitk_ws = W + pl.splitk;
      DVG_TRY(launch_conv_igemm(a, s));
    }
    if (s2 != s) DVG_TRY(stream_wait_mark(s2, dx_ready));
    DVG_TRY(launch_rowsum_partial(dX, N, 4 * n, W + pl.partL, s2));
    DVG_REQUIRE(sums.add(W + pl.partL, EW_BLOCKS, 4 * n, 4 * n, 1.0f, g->lin_b, n, 4), "decoder_bwd: column-sum batch full");  // j' = p*n+c -> c*4+p
    WgradArgs wa;
    wa.in = spins; wa.dy = dX; wa.slabs = W + pl.slabs; wa.spin_x = spin_pm1;
    wa.M = N; wa.Cin = n; wa.Cout = 4 * n; wa.L = 0; wa.ntaps = 1; wa.ups = 0; wa.ksplit = pl.ksplit_lin;
    DVG_TRY(launch_conv_wgrad(wa, s2));
    DVG_TRY(launch_wgrad_reduce(W + pl.slabs, pl.ksplit_lin, WeightMap{WM_LIN_FWD, n, 4 * n, 1}, g->lin_w, s2));
  }
  DVG_TRY(launch_colsum_batch(sums, s2));
  if (!defer_join) DVG_TRY(stream_order_after(s, s2));  // join (deferred: dvg_stream_join_side / the next backward call)
  return DVG_OK;
}
}  // namespace

extern "C" int dvg_decoder_bwd_ex(const dvg_decoder_params_t* p, int n, const float* spins, int64_t N,
                                  const float* grad_out, const dvg_decoder_grads_t* g, float* grad_spins, void* ws,
                                  size_t ws_bytes, int defer_join, dvg_stream_t stream) {
  return decoder_bwd_impl(p, n, spins, N, grad_out, nullptr, g, grad_spins, ws, ws_bytes, defer_join, stream);
}

extern "C" int dvg_decoder_bwd_mse_ex(const dvg_decoder_params_t* p, int n, const float* spins, int64_t N,
                                      const float* images, int R, float grad_scale, const dvg_decoder_grads_t* g,
                                      float* grad_spins, void* ws, size_t ws_bytes, int defer_join, dvg_stream_t stream) {
  const MseTail mt{images, R, grad_scale, nullptr};
  return decoder_bwd_impl(p, n, spins, N, nullptr, &mt, g, grad_spins, ws, ws_bytes, defer_join, stream);
}
