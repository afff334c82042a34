// Development hooks (include/dvg_dev.h): direct launches of the MFMA GEMM kernels for unit tests / micro-benchmarks.
#include "conv_plan.h"
#include "gibbs_plan.h"
#include "mmd_plan.h"
#include "../../include/dvg_dev.h"
using namespace dvg;

extern "C" int dvg_dev_conv_igemm(const float* in, const float* w, int mode, float* wp, const float* bias, float* out,
                                  float* stats, int64_t M, int Cin, int Cout, int L, int ntaps, int ups, int poolsum,
                                  int repack, float* splitk_ws, dvg_stream_t stream) {
  DVG_REQUIRE(in && w && wp && out, "dev_conv_igemm: null argument");
  hipStream_t s = (hipStream_t)stream;
  if (repack) DVG_TRY(launch_weight_pack(w, WeightMap{mode, Cin, Cout, ntaps}, wp, s, conv_launch_mode(M, Cout)));
  ConvArgs a;
  a.in = in; a.wp = wp; a.bias = bias; a.out = out; a.stats = stats;
  a.M = M; a.Cin = Cin; a.Cout = Cout; a.L = L; a.ntaps = ntaps; a.ups = ups; a.poolsum = poolsum;
  a.splitk_ws = splitk_ws;
  a.spin_a = opt(OPT_DEV_SPIN_OPERAND) != 0;  // (test knob: the +-1 promise for `in`)
  return launch_conv_igemm(a, s);
}
// The form launch_conv_igemm gives that launch under the current options and operand mode (conv_igemm_form; needs no device)
extern "C" int dvg_dev_conv_igemm_form(int64_t M, int Cin, int Cout, int L, int ntaps, int ups, int poolsum, int out[5]) {
  DVG_REQUIRE(out && M > 0 && Cin >= 32 && Cout >= 32 && Cin % 32 == 0 && Cout % 32 == 0 && (ntaps == 9 || ntaps == 1),
              "dev_conv_igemm_form: bad argument");
  ConvArgs a;
  a.in = a.wp = a.bias = nullptr; a.out = a.stats = a.splitk_ws = nullptr;
  a.M = M; a.Cin = Cin; a.Cout = Cout; a.L = L; a.ntaps = ntaps; a.ups = ups; a.poolsum = poolsum;
  a.spin_a = opt(OPT_DEV_SPIN_OPERAND) != 0;
  const IgemmForm f = conv_igemm_form(a, true);
  out[0] = f.bm; out[1] = f.bn; out[2] = f.pm; out[3] = f.ksplit; out[4] = f.posmajor;
  return DVG_OK;
}

// The same layer in the Winograd F(2x2,3x3) form (conv_wino.hip): `u` takes the 16 Cin Cout transformed weights; stats rows =
// dvg_dev_conv_wino_stats_blocks.  DVG_E_INVALID when the shape does not qualify (dvg_dev_conv_wino_shape).  um as in
// dvg_dev_conv_wino4: 1 = the forward behind the x2 upsample, 2 = its data gradient; cus: CUs the persistent grid is sized for.
extern "C" int dvg_dev_conv_wino(const float* in, const float* w, int mode, float* u, const float* bias, float* out,
                                 float* stats, int64_t M, int Cin, int Cout, int L, int cus, int um, dvg_stream_t stream) {
  DVG_REQUIRE(in && w && u && out, "dev_conv_wino: null argument");
  hipStream_t s = (hipStream_t)stream;
  DVG_TRY(launch_wino_weight_pack(w, WeightMap{mode, Cin, Cout, 9}, u, s));
  ConvArgs a;
  a.in = in; a.wp = u; a.bias = bias; a.out = out; a.stats = stats;
  a.M = M; a.Cin = Cin; a.Cout = Cout; a.L = L; a.ntaps = 9; a.ups = 0; a.poolsum = 0;
  a.splitk_ws = nullptr; a.wino_cus = cus; a.wino_um = um;
  return launch_conv_wino(a, s);
}
extern "C" int dvg_dev_conv_wino_shape(int64_t M, int Cin, int Cout, int L) { return conv_wino_shape(M, Cin, Cout, L) ? 1 : 0; }
// The same layer in the Winograd F(4x4,3x3) form (conv_wino4.hip): `u` takes the 36 Cin Cout transformed weights; stats rows =
// M / 1024.  DVG_E_INVALID when the shape does not qualify (dvg_dev_conv_wino4_shape).  The launch stands for the encoder layer
// of its image side (L = 4, 3, 2: layers 1, 2, 3; mode 0 the forward, 1 the data gradient): with that launch's block-shape bit
// of dev option enc_wino4_mask set it runs in the 64-channel block shape wherever the shape allows (the product's item-count
// rule is policy, not shape: conv_plan.cpp).
extern "C" int dvg_dev_conv_wino4(const float* in, const float* w, int mode, float* u, const float* bias, float* out,
                                  float* stats, int64_t M, int Cin, int Cout, int L, int cus, int um, dvg_stream_t stream) {
  DVG_REQUIRE(in && w && u && out, "dev_conv_wino4: null argument");
  hipStream_t s = (hipStream_t)stream;
  DVG_TRY(launch_wino4_weight_pack(w, WeightMap{mode, Cin, Cout, 9}, u, s, um != 0));
  ConvArgs a;
  a.in = in; a.wp = u; a.bias = bias; a.out = out; a.stats = stats;
  a.M = M; a.Cin = Cin; a.Cout = Cout; a.L = L; a.ntaps = 9; a.ups = 0; a.poolsum = 0;
  a.splitk_ws = nullptr; a.wino_cus = cus; a.wino_um = um;
  const int64_t mask = opt(OPT_ENC_WINO4_MASK);
  a.wino4_block64 = um == 0 && L >= 2 && L <= 4 && ((mask >> enc_wino4_block64_bit(5 - L, mode != 0)) & 1) && conv_wino4_block64_shape(M, Cin, Cout, L);
  return launch_conv_wino4(a, s);
}
extern "C" int dvg_dev_conv_wino4_shape(int64_t M, int Cin, int Cout, int L) { return conv_wino4_shape(M, Cin, Cout, L) ? 1 : 0; }
extern "C" int dvg_dev_conv_wino_ok(int64_t M, int Cin, int Cout, int L) { return plan_enc_wino_fwd(M, Cin, Cout, L, true, plan_options()) ? 1 : 0; }

// The plan of a network call under the current options and operand mode (conv_plan.h); needs no device.
extern "C" int dvg_dev_plan_forms(int network, int64_t rows, int n_latents, int training, int out[15]) {
  DVG_REQUIRE(out && (network == 0 || network == 1) && rows >= 1 && n_latents >= 32 && n_latents % 32 == 0, "dev_plan_forms: bad argument");
  const PlanOptions o = plan_options();
  ConvLayer y[4];
  if (network == 0) plan_encoder_layers(rows, n_latents, training != 0, o, y);
  else plan_decoder_layers(rows, n_latents, o, y);
  for (int l = 0; l < 4; ++l)
    for (int pass = 0; pass < 3; ++pass)
      out[3 * l + pass] = (network == 0 ? l == 0 : l == 3) ? -1 : (int)y[l].form[pass];
  const ConvForm f0 = y[0].form[PASS_FWD];
  out[12] = network == 1 && (f0 == CF_D22 || f0 == CF_LC0);
  out[13] = network == 1 && f0 == CF_LC0;
  out[14] = network == 1 && o.v[OPT_DEC_TAIL_FUSED] != 0;
  return DVG_OK;
}
// The plan of an MMD call under the current options (mmd_plan.h); needs no device.
extern "C" int dvg_dev_mmd_plan(int64_t nx, int64_t ny, int dim, int64_t out[24]) {
  DVG_REQUIRE(out && nx >= 2 && ny >= 2 && dim >= 32 && dim % 32 == 0, "dev_mmd_plan: bad argument");
  const MmdPlan p = mmd_plan(nx, ny, dim, mmd_options());
  const int64_t v[24] = {p.pair, p.nfb, p.nfbw, p.nst, p.nft, p.one, p.dist, p.dist_ns, p.gram, p.splits, p.slices, p.gated_nfb,
                         p.loss_parts, (int64_t)p.total, p.dist_splits, p.gram_passes, p.bf16_terms,
                         p.pair_launch.grid[0], p.pair_launch.grid[1], p.pair_launch.grid[2], p.distsum.grid[0], p.distsum.grid[1],
                         p.gated_nfb ? (int64_t)p.gated.grid[0] : 0, p.final_grad.grid[0]};
  for (int i = 0; i < 24; ++i) out[i] = v[i];
  return DVG_OK;
}
// The plan of a Gibbs draw under the current option gibbs_generic (gibbs_plan.h); reads host arrays only, needs no device.
extern "C" int dvg_dev_gibbs_draw_plan(int n, int n_colours, const int32_t* class_ptr, const int32_t* adj_ptr, int n_chains,
                                       int kind, int64_t out[19]) {
  DVG_REQUIRE(out && class_ptr && adj_ptr && n > 0 && n_colours > 0 && n_colours <= 64 && n_chains > 0 && kind >= GK_PLAIN &&
                  (kind <= GK_WEIGH || kind == GK_TRACE || gibbs_field_kind((GibbsDrawKind)kind)),
              "dev_gibbs_draw_plan: bad argument");
  const GibbsGraphShape g = gibbs_graph_shape(n, n_colours, class_ptr, adj_ptr);
  GibbsDrawPlan p;
  DVG_TRY(gibbs_draw_plan(g, n_chains, (GibbsDrawKind)kind, opt(OPT_GIBBS_GENERIC), &p));
  const int64_t v[19] = {p.form, p.lpc, p.waves, p.mb, p.nr, p.maxs, p.ch, p.fix, p.slots.n, p.chains_per_block, p.grid, p.threads,
                         (int64_t)p.lds, g.lane_has, g.lane_lpc, g.lane_mb, g.lane_nr, g.lane_rows, g.n_batches};
  for (int i = 0; i < 19; ++i) out[i] = v[i];
  return DVG_OK;
}
// ... and of an exchange draw (dvg_gibbs_sample_tempered) of n_ladders ladders of n_replicas chains: out[0..18] as above,
// out[19] the ladders a workgroup holds
extern "C" int dvg_dev_gibbs_exchange_plan(int n, int n_colours, const int32_t* class_ptr, const int32_t* adj_ptr, int n_ladders,
                                           int n_replicas, int64_t out[20]) {
  DVG_REQUIRE(out && class_ptr && adj_ptr && n > 0 && n_colours > 0 && n_colours <= 64 && n_ladders > 0 && n_replicas >= 2 &&
                  n_replicas <= GIBBS_MAX_REPLICAS && (int64_t)n_ladders * n_replicas <= 0x7fffffff,
              "dev_gibbs_exchange_plan: bad argument");
  const GibbsGraphShape g = gibbs_graph_shape(n, n_colours, class_ptr, adj_ptr);
  GibbsDrawPlan p;
  int per_block = 0;
  DVG_TRY(gibbs_exchange_plan(g, n_ladders, n_replicas, opt(OPT_GIBBS_GENERIC), &p, &per_block));
  const int64_t v[20] = {p.form, p.lpc, p.waves, p.mb, p.nr, p.maxs, p.ch, p.fix, p.slots.n, p.chains_per_block, p.grid, p.threads,
                         (int64_t)p.lds, g.lane_has, g.lane_lpc, g.lane_mb, g.lane_nr, g.lane_rows, g.n_batches, per_block};
  for (int i = 0; i < 20; ++i) out[i] = v[i];
  return DVG_OK;
}
extern "C" int dvg_dev_conv_wino_stats_blocks(int64_t M, int Cout) { return conv_wino_stats_blocks(M, Cout); }

extern "C" size_t dvg_dev_conv_splitk_floats(int64_t M, int Cin, int Cout, int ntaps, int poolsum) {
  return conv_splitk_floats(M, Cin, Cout, ntaps, poolsum);
}

extern "C" int dvg_dev_conv_stats_blocks(int64_t M, int Cout) { return conv_stats_blocks(M, Cout); }

extern "C" size_t dvg_dev_wgrad_slab_floats(int64_t M, int Cin, int Cout, int ntaps) {
  return (size_t)wgrad_ksplit(M, Cin, Cout, ntaps) * ntaps * Cin * Cout;
}

extern "C" int dvg_dev_conv_wgrad(const float* in, const float* dy, float* slabs, float* grad_w, int mode, int64_t M,
                                  int Cin, int Cout, int L, int ntaps, int ups, dvg_stream_t stream) {
  DVG_REQUIRE(in && dy && slabs && grad_w, "dev_conv_wgrad: null argument");
  hipStream_t s = (hipStream_t)stream;
  WgradArgs wa;
  wa.in = in; wa.dy = dy; wa.slabs = slabs; wa.M = M; wa.Cin = Cin; wa.Cout = Cout; wa.L = L; wa.ntaps = ntaps;
  wa.ups = ups; wa.ksplit = wgrad_ksplit(M, Cin, Cout, ntaps);
  wa.spin_x = opt(OPT_DEV_SPIN_OPERAND) != 0;  // (test knob: the +-1 promise for `in`)
  DVG_TRY(launch_conv_wgrad(wa, s));
  return launch_wgrad_reduce(slabs, wa.ksplit, WeightMap{mode, Cin, Cout, ntaps}, grad_w, s);
}
// The kernel launch_conv_wgrad takes for that launch under the current options and operand mode (conv_wgrad_form; needs no device)
extern "C" int dvg_dev_conv_wgrad_form(int64_t M, int Cin, int Cout, int ntaps, int ups, int out[5]) {
  DVG_REQUIRE(out && M > 0 && Cin >= 32 && Cout >= 32 && Cin % 32 == 0 && Cout % 32 == 0 && (ntaps == 9 || ntaps == 1),
              "dev_conv_wgrad_form: bad argument");
  WgradArgs wa;
  wa.in = wa.dy = nullptr; wa.slabs = nullptr; wa.M = M; wa.Cin = Cin; wa.Cout = Cout; wa.L = 0; wa.ntaps = ntaps;
  wa.ups = ups; wa.ksplit = 1;
  wa.spin_x = opt(OPT_DEV_SPIN_OPERAND) != 0;
  const WgradForm f = conv_wgrad_form(wa);
  out[0] = f.ba; out[1] = f.bb; out[2] = f.dma; out[3] = f.tap1; out[4] = f.spin;
  return DVG_OK;
}

extern "C" size_t dvg_dev_wino_wgrad_slab_floats(int64_t M, int Cin, int Cout, int L) {
  return conv_wino_wgrad_shape(M, Cin, Cout, L) ? conv_wino_wgrad_slab_floats(M, Cin, Cout, L) : 0;
}

extern "C" int dvg_dev_conv_wino_wgrad(const float* in, const float* dy, float* slabs, float* grad_w, int mode, int64_t M,
                                       int Cin, int Cout, int L, int ups, int cus, dvg_stream_t stream) {
  DVG_REQUIRE(in && dy && slabs && grad_w, "dev_conv_wino_wgrad: null argument");
  return launch_conv_wino_wgrad(in, dy, M, Cin, Cout, L, slabs, WeightMap{mode, Cin, Cout, 9}, grad_w, (hipStream_t)stream, ups, cus);
}

// The same weight gradient in the Winograd F(4x4,3x3) form (conv_wino4_wgrad.hip): slabs of dvg_dev_wino4_wgrad_slab_floats()
// floats (0 = the shape does not qualify)
extern "C" size_t dvg_dev_wino4_wgrad_slab_floats(int64_t M, int Cin, int Cout, int L) {
  return conv_wino4_wgrad_shape(M, Cin, Cout, L) ? conv_wino4_wgrad_slab_floats(M, Cin, Cout) : 0;
}

extern "C" int dvg_dev_conv_wino4_wgrad(const float* in, const float* dy, float* slabs, float* grad_w, int mode, int64_t M,
                                        int Cin, int Cout, int L, int cus, dvg_stream_t stream) {
  DVG_REQUIRE(in && dy && slabs && grad_w, "dev_conv_wino4_wgrad: null argument");
  return launch_conv_wino4_wgrad(in, dy, M, Cin, Cout, L, slabs, WeightMap{mode, Cin, Cout, 9}, grad_w, (hipStream_t)stream, cus);
}
