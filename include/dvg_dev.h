/* dvg_dev.h — development hooks of libdvg.so: direct access to the two MFMA GEMM kernels, used by
 * the kernel-level unit tests and micro-benchmarks (tests/test_gpu_kernels.py, scratch/).  NOT part of
 * the drop-in boundary (include/dvg.h); signatures may change between rounds.
 * Tensors are in the library's internal layout: NHWC float32, pixels of each image in Morton order. */
#ifndef DVG_DEV_H
#define DVG_DEV_H
#include "dvg.h"
#ifdef __cplusplus
extern "C" {
#endif
/* mode: 0 Conv2d fwd, 1 Conv2d dgrad, 2 ConvTranspose2d fwd, 3 ConvTranspose2d dgrad, 4 Linear fwd, 5 Linear dgrad
 * (csrc/conv.h WeightMode).  w: checkpoint-layout weight; wp: scratch for the packed copy (ntaps*Cin*Cout floats).
 * out[m][co] = sum_{tap,ci} in[nbr(m,tap)][ci] * Wp[tap][ci][co] (+bias); stats: [blocks][Cout][2] or NULL. */
int dvg_dev_conv_igemm(const float *in, const float *w, int mode, float *wp, const float *bias, float *out,
                       float *stats, int64_t M, int Cin, int Cout, int L, int ntaps, int ups, int poolsum,
                       int repack, float *splitk_ws, dvg_stream_t stream);
size_t dvg_dev_conv_splitk_floats(int64_t M, int Cin, int Cout, int ntaps, int poolsum);
/* The form that launch takes under the current options and operand mode (csrc/conv.h: conv_igemm_form, the launcher's own
 * decision; needs no device): out[0], out[1] = the block tile BM x BN; out[2] = the operand form, the PM argument of
 * conv_igemm_kernel (0 float32 through registers, 3 float32 by LDS-DMA, 4 f32x3, 5 bf16 inputs, 6 spin A under dev option
 * dev_spin_operand); out[3] = the split-K count of a launch that has a workspace (1: unsplit); out[4] = position-major tiles. */
int dvg_dev_conv_igemm_form(int64_t M, int Cin, int Cout, int L, int ntaps, int ups, int poolsum, int out[5]);
/* The same stride-1 3x3 layer in the Winograd F(2x2,3x3) form the encoder uses from 256 workgroups up (option enc_wino):
 * `u` = scratch of 16*Cin*Cout floats (transformed weights), `stats` rows = dvg_dev_conv_wino_stats_blocks(M, Cout).
 * Replaces (with the implicit GEMM above) /root/reference/src/encoder.py:28-36's nn.Conv2d calls. */
int dvg_dev_conv_wino(const float *in, const float *w, int mode, float *u, const float *bias, float *out, float *stats,
                      int64_t M, int Cin, int Cout, int L, int cus, int um, dvg_stream_t stream);
/* (cus = CUs the persistent grid is sized for, 0 = 256; um as in dvg_dev_conv_wino4 below: 1 = Upsample(x2) + 3x3 forward,
 * `in` = the source map ([M / 4][Cin]), M and L of the output grid, 9 of 16 positions; 2 = its data gradient, `in` = the
 * fine-grid gradient, `out` = the source map's gradient ([M / 4][Cout]).  Cout % 64 == 0 runs conv_wino8_kernel<2,2,8,um>,
 * any other Cout % 32 == 0 conv_wino8_kernel<4,1,4,um>.)
 * ... whether the form can run the shape at all (whatever option enc_wino says) */
int dvg_dev_conv_wino_shape(int64_t M, int Cin, int Cout, int L);
/* ... whether a training call's forward launch of this shape takes that form under the current options and operand mode */
int dvg_dev_conv_wino_ok(int64_t M, int Cin, int Cout, int L);
/* The kernel form every MFMA convolution layer of a network call takes under the current options and operand mode
 * (csrc/conv_plan.h; needs no device).  network: 0 encoder (rows = batch), 1 decoder (rows = batch x replicas).
 * out[3 l + pass], l = 0..3, pass 0 forward / 1 data gradient / 2 weight gradient: 0 direct implicit GEMM, 1 folded
 * upsample, 2 dense 2x2 map, 3 Linear composed with that map, 4 Winograd F(2x2,3x3), 5 Winograd F(4x4,3x3); -1 for the
 * VALU layers (encoder layer 0, decoder layer 3).  out[12..14] = the decoder's d22 / lc0 / tail flags (encoder: 0).
 * The decoder's plan does not depend on `training`; an evaluation-mode encoder plan reads 0 for its gradients. */
int dvg_dev_plan_forms(int network, int64_t rows, int n_latents, int training, int out[15]);
/* The kernel forms an MMD call (dvg_mmd_fwd_bwd) of this shape takes under the current options (csrc/mmd_plan.h; needs no
 * device).  out[0] pair form: 0 float32 only (mmd_main_kernel<out[1]>), 1 sliced spin (mmd_pair_kernel<out[1]>), 2 feature-
 * quarter (mmd_pair_fq_kernel<out[2]>), 3 128-row block (mmd_pair_w128_kernel<out[3], out[4], out[5], FP4>); out[1..5] =
 * NFB, NFBW, NST, NFT, ONE (0 where the form has no such parameter).  out[6] distance-sum form: 0 float32
 * (mmd_distsum_kernel), 1 mmd_distsum_spin_kernel<out[7]>, 2 mmd_distsum_spin256_kernel<out[7], FP4>.  out[8] matrix pipe of
 * the exact spin Gram in the kernels that have the choice: 0 int8, 1 FP4.  out[9] column splits, out[10] feature slices
 * (grid z) of the pair launch; out[11] NFB of the gated float32 launch behind the 128-row-block kernel (0: none);
 * out[12] loss partials the final kernel sums; out[13] = dvg_mmd_workspace_bytes; out[14] column splits of the distance
 * sum; out[15], out[16] Gram passes and bf16 terms as dvg_mmd_spin_flops prices them; out[17..19] grid of the pair
 * launch, out[20..21] of the distance sum (when no bandwidth is given), out[22] of the gated launch, out[23] of the final
 * kernel when a gradient is asked for. */
int dvg_dev_mmd_plan(int64_t nx, int64_t ny, int dim, int64_t out[24]);
/* The kernel form a Gibbs draw of n_chains chains takes on a graph under the current option gibbs_generic
 * (csrc/gibbs_plan.h; reads the host arrays of the graph's colouring and CSR only, needs no device).  kind: 0 plain
 * (dvg_gibbs_sample), 1 held (_clamped), 2 table (_annealed), 3 weigh (_ais), 5 trace (_traced: the table kind's plan; 4, the
 * exchange draw, is planned by dvg_dev_gibbs_exchange_plan), 6 field (_fields: rolled on every graph, out[12] with the
 * chains' rows of hs).  out[0] form: 0 rolled (gibbs_kernel<out[1],
 * out[2], ..>), 1 lane-major (gibbs_fast_kernel<out[1], out[2], out[3], out[4], out[5], ..>), 2 chains side by side
 * (gibbs_slot_kernel<out[5], out[6], out[7]>); out[1..7] = LPC, WAVES, MB, NR, MAXS, CH, FIX (0 where the form has no such
 * parameter); out[8] the slots form's (class, pass) slots; out[9] chains per workgroup; out[10] workgroups, out[11] threads
 * per workgroup, out[12] LDS bytes per workgroup (what dvg_gibbs_launch_info reports for kind 0); out[13] whether the
 * graph gets a lane-major image, out[14..17] its lanes per chain, batches per row, rows per step and rows (csrc/graph.h);
 * out[18] the padded-row image's batches.  DVG_E_UNSUPPORTED: the form the
 * graph must take needs more than 160 KiB of LDS. */
int dvg_dev_gibbs_draw_plan(int n, int n_colours, const int32_t *class_ptr, const int32_t *adj_ptr, int n_chains, int kind,
                            int64_t out[19]);
/* The same for an exchange draw (dvg_gibbs_sample_tempered) of n_ladders ladders of n_replicas (2..16) chains
 * (csrc/gibbs_plan.h, gibbs_exchange_plan: the table kind's form if its workgroup holds a ladder, else that family at four
 * waves, else the rolled form (64, 16)).  out[0..18] as above -- out[9] chain SLOTS per workgroup, out[10] workgroups =
 * ceil(n_ladders / out[19]), out[12] with the mailboxes, counters and ladder -- and out[19] the whole ladders a workgroup holds. */
int dvg_dev_gibbs_exchange_plan(int n, int n_colours, const int32_t *class_ptr, const int32_t *adj_ptr, int n_ladders,
                                int n_replicas, int64_t out[20]);
/* The same layer in the Winograd F(4x4,3x3) form (csrc/conv_wino4.hip: 36 position GEMMs per 4x4 output tile, 2.25 multiplies
 * per output where F(2x2,3x3) issues 4.0): `u` = scratch of 36*Cin*Cout floats, `stats` rows = M / 1024 (tile blocks of 64
 * tiles), cus = CUs the persistent grid is sized for (0 = 256).  Shapes: whole 1024-pixel blocks of 4x4 / 8x8 / 16x16 images. */
int dvg_dev_conv_wino4(const float *in, const float *w, int mode, float *u, const float *bias, float *out, float *stats,
                       int64_t M, int Cin, int Cout, int L, int cus, int um, dvg_stream_t stream);
/* (um = 1: Upsample(x2) + 3x3 forward, `in` = the source map ([M / 4][Cin]), 25 of 36 positions; um = 2: its data gradient,
 * `in` = the fine-grid gradient, `out` = the source map's gradient ([M / 4][Cout]))
 * (um = 0: the launch stands for the encoder layer of its image side -- L = 4, 3, 2: layers 1, 2, 3; mode 0 the forward, 1 the
 * data gradient -- and follows that launch's block-shape bit of dev option enc_wino4_mask (bits 16-21): set and Cout % 64 == 0,
 * it runs blocks of 32 tiles x 64 output channels instead of 64 x 32; same bits) */
int dvg_dev_conv_wino4_shape(int64_t M, int Cin, int Cout, int L);
/* ... and the layer's weight gradient in that form (csrc/conv_wino4_wgrad.hip): slabs of dvg_dev_wino4_wgrad_slab_floats()
 * floats (0 = the shape does not qualify); cus: CUs the grid is sized for (0 = the training step's budget). */
size_t dvg_dev_wino4_wgrad_slab_floats(int64_t M, int Cin, int Cout, int L);
int dvg_dev_conv_wino4_wgrad(const float *in, const float *dy, float *slabs, float *grad_w, int mode, int64_t M, int Cin,
                             int Cout, int L, int cus, dvg_stream_t stream);
int dvg_dev_conv_wino_stats_blocks(int64_t M, int Cout);
int dvg_dev_conv_stats_blocks(int64_t M, int Cout);
/* grad_w (checkpoint layout, `mode` = the layer's FORWARD mode) = sum_m in[nbr(m,tap)] (x) dy[m]; slabs: scratch of
 * dvg_dev_wgrad_slab_floats() floats. */
size_t dvg_dev_wgrad_slab_floats(int64_t M, int Cin, int Cout, int ntaps);
int dvg_dev_conv_wgrad(const float *in, const float *dy, float *slabs, float *grad_w, int mode, int64_t M, int Cin,
                       int Cout, int L, int ntaps, int ups, dvg_stream_t stream);
/* The kernel that launch takes under the current options and operand mode (csrc/conv.h: conv_wgrad_form, the launcher's own
 * decision; needs no device): out[0], out[1] = the channel tile (Cin x Cout: 32 / 64 each, 128 x 128 for the 1-tap DMA
 * kernel); out[2] = 1 LDS-DMA (conv_wgrad9_dma_kernel<out[0] / 32, out[1] / 32, ..> or conv_wgrad1_dma_kernel), 0 register-
 * staged; out[3] = 1 the 1-tap DMA kernel; out[4] = its spin form (conv_wgrad1_dma_kernel<true>, dev option dev_spin_operand). */
int dvg_dev_conv_wgrad_form(int64_t M, int Cin, int Cout, int ntaps, int ups, int out[5]);
/* The same weight gradient in the Winograd F(2x2,3x3) form (conv_wino_wgrad.hip; ups = 1: `in` is the source map of an Upsample(x2) + 3x3 layer): slabs of
 * dvg_dev_wino_wgrad_slab_floats() floats (0 = the shape does not qualify). */
size_t dvg_dev_wino_wgrad_slab_floats(int64_t M, int Cin, int Cout, int L);
int dvg_dev_conv_wino_wgrad(const float *in, const float *dy, float *slabs, float *grad_w, int mode, int64_t M, int Cin,
                            int Cout, int L, int ups, int cus, dvg_stream_t stream); /* cus: CUs the grid is sized for (0 = the training step's budget) */
/* Where the encoder's workspace (dvg_encoder_workspace_bytes) keeps what a forward call saved, as FLOAT offsets:
 * out[0..3] = pre-BatchNorm convolution outputs Y[l] ([B * HW_l][C_l], Morton NHWC), out[4..7] = pooled stage outputs
 * Xp[l], out[8..11] = batch means, out[12..15] = batch inverse standard deviations.  Diagnostics only.  (Y[0] is only
 * written under option enc_l0_fused = 0: the default recomputes layer 0 wherever its output is needed.) */
int dvg_dev_encoder_layout(int64_t B, int n_latents, size_t out[16]);
/* A/B references and test knobs: the kernel forms a default of the library replaced (register-staged GEMMs, the stored
 * encoder layer 0, the unfused decoder tail, the static Winograd tile deal, the rolled sampler schedule, forced MMD
 * kernels) and the tile threshold the small fixtures lower.  Same semantics as dvg_set_option / dvg_get_option
 * (include/dvg.h), a separate name space: the product's boundary carries eight switches, these are not among them.
 * dvg_reset_options restores both kinds. */
int dvg_dev_option_count(void);
const char *dvg_dev_option_name(int index);
const char *dvg_dev_option_doc(int index);
int dvg_dev_set_option(const char *name, int64_t value);
int dvg_dev_get_option(const char *name, int64_t *value);
#ifdef __cplusplus
}
#endif
#endif
