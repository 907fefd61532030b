/*
 * jpdse.h -- C ABI of libjpdse_hip.so: the MI355X (gfx950) kernels behind the JPD-SE
 * training hot path.
 *
 * The reference (SenseBrain/JPD-SE) is pure Python on torch.nn -> cuDNN and has no FFI of
 * its own; each entry point below replaces the torch.nn call sites cited next to it
 * (paths relative to the reference root, `networks.py` =
 * ctu/models/pix2pixHD_networks/networks.py, `model.py` = ctu/models/pix2pixHD_model.py).
 *
 * Conventions
 *   - every function returns 0 on success or a negative JPDSE_E* code; the message is
 *     available from jpdse_last_error() (thread local);
 *   - nothing here allocates, frees, synchronises or throws: all buffers are caller-owned
 *     device memory, borrowed for the duration of the enqueue on `stream` (hipStream_t
 *     passed as void*);
 *   - activations are NHWC, channel count stored rounded up to a multiple of 8
 *     (JPDSE_CPAD): storage channels >= logical channels, the padding lanes are zero;
 *   - filters are passed as fp32 "master" tensors in KRSC order (= the memory order of a
 *     torch OIHW tensor in channels_last format; for ConvTranspose2d's IOHW weight the same
 *     memory order is [Cin][R][S][Cout]) and packed per step into compute-dtype GEMM panels;
 *   - dtype: JPDSE_F32 computes on v_mfma_f32_32x32x2_f32 (exact fp32 fma chains),
 *     JPDSE_BF16 on v_mfma_f32_32x32x16_bf16 with fp32 accumulation; statistics, loss
 *     reductions, weight gradients, Adam state are always fp32.
 */
#ifndef JPDSE_H_
#define JPDSE_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define JPDSE_ABI_VERSION 2   /* 2 (round 4): + jpdse_conv_dgrad_nsum_slots / _fused_nsums, jpdse_inorm_bwd_from_sums; round 3 had already added
                                * jpdse_loss_finalize, jpdse_conv_fwd_pool, jpdse_conv_dgrad_fused_lrelu, jpdse_input_builder, jpdse_copy, jpdse_prof_hbm_* under version 1;
                                * the learned codec (jpdse_binarize_fwd, jpdse_code_stats[_workspace_size], jpdse_code_export) was added to
                                * version 2 later, and so were the evaluation metrics (jpdse_eval_metrics[_workspace_size]) and their
                                * per-class form (jpdse_eval_metrics_sem[_workspace_size]), and the receiver side of the codec
                                * (jpdse_code_import), and the MS-SSIM training loss (jpdse_msssim_loss[_workspace_size]), and the input
                                * builder for more than 64 storage channels (jpdse_input_builder_wide), and the entropy-coded bitstream
                                * (jpdse_code_entropy_*), and the coded label and instance maps (jpdse_semantics_*), and the
                                * context-model rate term (jpdse_code_rate_loss[_workspace_size]), and the semantics-weighted
                                * distortion (jpdse_sem_weighted_loss), and the code-length map (jpdse_code_cost[_table,
                                * _workspace_size]), and the code-length maps of the vector quantizer's two coders
                                * (jpdse_vq_index_cost[_workspace_size], jpdse_vq_plane_cost[_workspace_size]): purely additive,
                                * nothing existing changed */

enum { JPDSE_F32 = 0, JPDSE_BF16 = 1 };
enum { JPDSE_PAD_ZERO = 0, JPDSE_PAD_REFLECT = 1 };
enum { JPDSE_ACT_NONE = 0, JPDSE_ACT_RELU = 1, JPDSE_ACT_LRELU = 2, JPDSE_ACT_TANH = 3 };
enum {
  JPDSE_OK = 0,
  JPDSE_EINVAL = -1,      /* bad descriptor / null pointer / unsupported combination */
  JPDSE_EWORKSPACE = -2,  /* workspace smaller than *_workspace_size() */
  JPDSE_ELAUNCH = -3,     /* hipLaunchKernel / runtime error (message carries hipGetErrorString) */
  JPDSE_EARCH = -4        /* device is not gfx950 */
};

#define JPDSE_CPAD(c) (((c) + 7) & ~7)

/* ---- library ------------------------------------------------------------------------ */
int jpdse_version(void);
const char* jpdse_last_error(void);
/* 0 when device `device` is gfx950; JPDSE_EARCH otherwise (no reference counterpart). */
int jpdse_arch_check(int device);

/* Kernel timer used by bench.py's roofline figure (no reference counterpart): after
 * jpdse_prof_select(1, Ks, kdim, max) every implicit-GEMM launch with CPAD(out channels) == Ks
 * and GEMM reduction length == kdim is bracketed by hipEvents on its own stream;
 * jpdse_prof_collect waits for them and returns the summed kernel time, the summed algorithmic
 * FLOPs (2*M*Ks*kdim per launch) and the number of launches, then resets the log.
 * Not thread safe; select with enable = 0 to switch it off. */
int jpdse_prof_select(int32_t enable, int32_t Ks, int64_t kdim, int32_t max_launches);
int jpdse_prof_collect(double* total_ms, double* total_flops, int64_t* launches);
/* The same sums for the other regions of the selected layer, WITHOUT resetting the log (call before jpdse_prof_collect):
 * cls 1 = the reflect ring of the data gradient -- ring_frame_kernel, or the strip GEMMs + fold (time only, their FLOPs belong to the data
 * gradient counted in class 0), cls 2 = the weight-gradient launches (K == Ks, 9 * CPAD(C) == kdim). */
int jpdse_prof_collect_class(int32_t cls, double* total_ms, double* total_flops, int64_t* launches);
/* The same for the HBM-bound calls (bench.py "roofline_hbm"; north_star: "HBM GB/s on the norm/activation kernels"): after
 * jpdse_prof_hbm_select(1, max) every jpdse_inorm_fwd / jpdse_inorm_fwd_from_moments (class JPDSE_HBM_INORM_FWD),
 * jpdse_inorm_bwd (JPDSE_HBM_INORM_BWD) and jpdse_adam_step (JPDSE_HBM_ADAM) call is bracketed by a hipEvent pair on its own
 * stream (all kernels of the call: moments, finalize, apply) until `max` regions are used.  jpdse_prof_hbm_collect waits for
 * the regions of one class and returns their summed time, their summed ALGORITHMIC bytes -- InstanceNorm forward 3 x the
 * tensor (x read by the moment pass and by the apply pass, y written; + the residual when there is one; 2 x when the moments
 * came from the conv epilogue), backward 5 x (x and dy read twice, dx written), Adam 28 B per parameter (+ 2 B when it also
 * writes the bf16 forward panel) -- and their count.  jpdse_prof_hbm_select(0, 0) switches the timer off and clears the log. */
#define JPDSE_HBM_INORM_FWD 0
#define JPDSE_HBM_INORM_BWD 1
#define JPDSE_HBM_ADAM 2
int jpdse_prof_hbm_select(int32_t enable, int32_t max_regions);
int jpdse_prof_hbm_collect(int32_t cls, double* total_ms, double* total_bytes, int64_t* regions);

/* ---- convolution family ------------------------------------------------------------- */
/* One descriptor covers nn.Conv2d as used by:
 *   ReflectionPad2d(3)+Conv2d 7x7            networks.py:210,246,160,175
 *   Conv2d 3x3 stride 2 pad 1                networks.py:215,162
 *   ReflectionPad2d(1)+Conv2d 3x3 (ResBlock) networks.py:275,283,291,298
 *   Conv2d 4x4 stride 2|1 pad 2 (PatchGAN)   networks.py:430,437,444,449
 *   VGG19 Conv2d 3x3 pad 1 + ReLU            networks.py:477-492
 * and, with the roles of fwd/dgrad swapped by the caller, nn.ConvTranspose2d 3x3 stride 2
 * pad 1 output_padding 1 (networks.py:244,170): convT.forward == dgrad of the Conv2d with
 * K=Cin_T, C=Cout_T; convT.dgrad == that Conv2d's fwd; convT.wgrad == its wgrad with
 * (x, dy) = (dy_T, x_T).  jpdse_convT_* below are exactly those aliases. */
typedef struct jpdse_conv_desc {
  int32_t dtype;      /* JPDSE_F32 | JPDSE_BF16: activations and packed filters */
  int32_t N, H, W, C; /* input  [N,H,W,CPAD(C)] */
  int32_t K;          /* output channels; output is [N,OH,OW,CPAD(K)] */
  int32_t R, S;       /* filter height, width */
  int32_t stride;     /* 1 | 2 */
  int32_t pad;        /* symmetric padding */
  int32_t pad_mode;   /* JPDSE_PAD_ZERO | JPDSE_PAD_REFLECT (reflect requires stride 1) */
  int32_t act;        /* fwd epilogue after bias: JPDSE_ACT_* */
  float slope;        /* LeakyReLU negative slope */
} jpdse_conv_desc;

int jpdse_conv_out_shape(const jpdse_conv_desc* d, int32_t* OH, int32_t* OW);
/* Introspection of the host-side plan (no device work; callable without a GPU).  Writes 54
 * int32: {Cs,Ks,Hp,Wp,OH,OW,Lk_fwd,n_phases,PT,PB,PL,PR,DH,DW} then for each of 4 stride
 * phases of the data gradient {qh,qw,Uh,Uw,i0h,cnth,i0w,cntw,Lk,pack_offset_bytes}. */
int jpdse_conv_plan_query(const jpdse_conv_desc* d, int32_t* out, int32_t n);
/* bytes of the packed forward / data-gradient filter panels */
size_t jpdse_conv_fwd_pack_size(const jpdse_conv_desc* d);
size_t jpdse_conv_dgrad_pack_size(const jpdse_conv_desc* d);
/* master fp32 KRSC -> compute-dtype panels (either output pointer may be NULL to skip) */
int jpdse_conv_pack_weights(const jpdse_conv_desc* d, const float* w_krsc, void* fwd_pack,
                            void* dgrad_pack, void* stream);
/* Batched re-packing of the data-gradient panels of many layers in ONE launch (per optimizer step every
 * conv of the stepped network needs a fresh panel).  jpdse_conv_pack_entries (host only, no GPU work)
 * appends one entry per stride phase of layer `d` to `out` and returns their number, or -1 when the
 * layer cannot be batched (a phase whose panel rows are padded): use jpdse_conv_pack_weights
 * for those.  The caller fills `block0` with the running sum of `blocks` over its whole table, uploads
 * the table once and calls jpdse_conv_pack_run(table_dev, n, total_blocks) after each optimizer step. */
typedef struct jpdse_pack_entry {
  const float* w;   /* fp32 KRSC master */
  void* out;        /* this phase's panel inside the layer's dgrad pack */
  int32_t K, Ks, C, Cs, R, S, st, qh, qw, Uh, Uw, Lk, gx, gy;
  int32_t out_f32;  /* 1: the panel is fp32 (JPDSE_F32 layers), 0: bf16 (ABI version 2) */
  int32_t reserved_;
  int64_t blocks;   /* thread blocks this entry needs */
  int64_t block0;   /* first block of this entry in the launch */
} jpdse_pack_entry;
int jpdse_conv_pack_entries(const jpdse_conv_desc* d, const float* w_krsc, void* dgrad_pack,
                            jpdse_pack_entry* out, int32_t max_entries);
int jpdse_conv_pack_run(const jpdse_pack_entry* table_dev, int32_t n_entries, int64_t total_blocks,
                        void* stream);
/* workspace needed by fwd / dgrad / wgrad (max over the three) */
size_t jpdse_conv_workspace_size(const jpdse_conv_desc* d);
/* y = act(conv(pad(x)) + bias); bias may be NULL (convs feeding an affine-less
 * InstanceNorm: the bias is cancelled exactly by the mean subtraction). */
int jpdse_conv_fwd(const jpdse_conv_desc* d, const void* x, const void* fwd_pack,
                   const float* bias, void* y, void* ws, size_t ws_bytes, void* stream);
/* Forward of a conv that feeds an affine-less InstanceNorm, with the norm's moment pass fused into the conv's epilogue
 * (networks.py:204,216,245: conv -> norm): also writes moments[n][c][slot] = (mean, M2 = sum (y - mean)^2) of the STORED
 * (rounded) values over the pixels of block `slot` of image n -- every slot covers H*W / slots pixels; taken about a per-block
 * pilot value, so a channel with |mean| >> std keeps its variance --, fp32 [N][CPAD(K)][slots][2] with slots = jpdse_conv_moment_slots(d) (0: this layer's kernel has no such
 * epilogue -- use jpdse_conv_fwd + jpdse_inorm_fwd).  No bias (the norm cancels it), d->act must be JPDSE_ACT_NONE.
 * jpdse_inorm_fwd_from_moments then replaces jpdse_inorm_fwd's moment pass. */
int32_t jpdse_conv_moment_slots(const jpdse_conv_desc* d);
int jpdse_conv_fwd_moments(const jpdse_conv_desc* d, const void* x, const void* fwd_pack, void* y, float* moments,
                           void* ws, size_t ws_bytes, void* stream);
/* dx = d(loss)/d(x) given dy = d(loss)/d(pre-activation output) */
/* y as jpdse_conv_fwd and, in the same call, y_pool = MaxPool2d(2, 2)(y) [N][OH/2][OW/2][CPAD(K)] -- the conv -> ReLU ->
 * MaxPool2d chain of VGG19 (networks.py:477-492).  Kernels that keep their output tile in LDS write both from one epilogue
 * (the pool pass over y is saved); the others run the pool kernel behind the conv.  Equal to jpdse_conv_fwd + jpdse_maxpool2_fwd. */
int jpdse_conv_fwd_pool(const jpdse_conv_desc* d, const void* x, const void* fwd_pack, const float* bias,
                        void* y, void* y_pool, void* ws, size_t ws_bytes, void* stream);
int jpdse_conv_dgrad(const jpdse_conv_desc* d, const void* dy, const void* dgrad_pack, void* dx,
                     void* ws, size_t ws_bytes, void* stream);
/* dx = conv_dgrad(dy) * (x > 0): `x` is this conv's own INPUT [N,H,W,CPAD(C)], which must be a
 * ReLU output (or a max-pool of one).  Equals jpdse_conv_dgrad followed by the backward of the
 * ReLU that produced x -- the chain conv -> ReLU(inplace) -> conv of VGG19 (networks.py:477-492)
 * -- with the mask applied in the GEMM epilogue instead of a separate pass over dx. */
int jpdse_conv_dgrad_relu(const jpdse_conv_desc* d, const void* dy, const void* dgrad_pack,
                          const void* x, void* dx, void* ws, size_t ws_bytes, void* stream);
/* dx = (conv_dgrad(dy) + addend) * (x > 0); `x` (ReLU mask, see above) and `addend` (same shape as dx)
 * may each be NULL.  The addend is the other branch of a gradient fan-in: the skip connection of a
 * ResnetBlock (`out = x + self.conv_block(x)`, networks.py:303-305) or the loss gradient arriving at
 * a VGG19 tap -- summed in the GEMM epilogue instead of a separate add pass. */
int jpdse_conv_dgrad_fused(const jpdse_conv_desc* d, const void* dy, const void* dgrad_pack,
                           const void* x, const void* addend, void* dx, void* ws, size_t ws_bytes,
                           void* stream);
/* LeakyReLU form of the above: dx = r * (x > 0 ? 1 : slope) with r = conv_dgrad(dy) + addend rounded to
 * the tensor dtype.  `x` (required) is this conv's own input, the OUTPUT of LeakyReLU(slope) -- the chain
 * Conv2d -> LeakyReLU(0.2) -> Conv2d of NLayerDiscriminator (networks.py:430-437) -- so dx is the
 * gradient w.r.t. that LeakyReLU's pre-activation; equal, bit for bit, to jpdse_conv_dgrad_fused(x = NULL)
 * followed by jpdse_act_bwd(JPDSE_ACT_LRELU). */
int jpdse_conv_dgrad_fused_lrelu(const jpdse_conv_desc* d, const void* dy, const void* dgrad_pack,
                                 const void* x, float slope, const void* addend, void* dx, void* ws,
                                 size_t ws_bytes, void* stream);
/* jpdse_conv_dgrad_fused / _fused_lrelu (slope 0: the ReLU form) over a batch with more gradient images than saved forward
 * ones -- the PatchGAN walked backwards once for loss_G and loss_D: d->N counts the images of dy / dx; gradient image n reads
 * the mask of image n >= alias ? n - alias : n of `x` (which holds d->N - alias images; alias 0: one mask image per gradient
 * image), and only images n < addend_n take `addend` (which holds addend_n images; 0: every image does).  Each image's
 * result equals, bit for bit, that of the un-batched call on a batch that contains it with the same kernel.  2 alias <= N; with
 * both a mask and an addend the batch has one cut: addend_n == alias (or alias 0).  Only the routes of
 * the PatchGAN's layers take such a call; the others are refused (JPDSE_EINVAL). */
int jpdse_conv_dgrad_batched(const jpdse_conv_desc* d, const void* dy, const void* dgrad_pack, const void* x, float slope,
                             const void* addend, int32_t alias, int32_t addend_n, void* dx, void* ws, size_t ws_bytes,
                             void* stream);
/* jpdse_conv_dgrad_fused whose output dx is the gradient w.r.t. the OUTPUT of an InstanceNorm2d (+ activation): the chains
 * conv -> InstanceNorm -> ReLU -> [pad] conv and x + conv_block(x) of ResnetBlock (networks.py:283-305).  The norm's backward
 * needs, per (image, channel), sum dz and sum dz * yhat with yhat = (norm_x - mean) rstd and dz = dx act'(yhat); the epilogue
 * that writes dx forms them per block from the values it stores and norm_x (the norm's INPUT, same shape as dx), norm_stats
 * ([N][CPAD(C)][2] = (mean, rstd) of jpdse_inorm_fwd) and writes sums [N][CPAD(C)][slots][2], slots =
 * jpdse_conv_dgrad_nsum_slots(d) (0: this layer's data-gradient kernel has no such epilogue -- use jpdse_conv_dgrad_fused +
 * jpdse_inorm_bwd).  jpdse_inorm_bwd_from_sums then replaces jpdse_inorm_bwd's own pass over (x, dy) for the sums. */
int32_t jpdse_conv_dgrad_nsum_slots(const jpdse_conv_desc* d);
int jpdse_conv_dgrad_fused_nsums(const jpdse_conv_desc* d, const void* dy, const void* dgrad_pack, const void* x,
                                 const void* addend, void* dx, const void* norm_x, const float* norm_stats,
                                 int32_t norm_act, float norm_slope, float* sums, void* ws, size_t ws_bytes, void* stream);
/* dw (fp32, KRSC master layout) = d(loss)/d(w); overwritten (beta = 0) */
int jpdse_conv_wgrad(const jpdse_conv_desc* d, const void* x, const void* dy, float* dw_krsc,
                     void* ws, size_t ws_bytes, void* stream);

/* nn.ConvTranspose2d aliases: `d` describes the *underlying* Conv2d (its input is the
 * transposed conv's OUTPUT: N,H,W,C = output geometry, K = transposed conv's Cin). */
int jpdse_convT_fwd(const jpdse_conv_desc* d, const void* x, const void* dgrad_pack, void* y,
                    void* ws, size_t ws_bytes, void* stream);
/* jpdse_convT_fwd with the moments of its output (see jpdse_conv_fwd_moments); slots for the UNDERLYING conv descriptor */
int32_t jpdse_convT_moment_slots(const jpdse_conv_desc* d);
int jpdse_convT_fwd_moments(const jpdse_conv_desc* d, const void* x, const void* dgrad_pack, void* y, float* moments,
                            void* ws, size_t ws_bytes, void* stream);
int jpdse_convT_dgrad(const jpdse_conv_desc* d, const void* dy, const void* fwd_pack, void* dx,
                      void* ws, size_t ws_bytes, void* stream);
int jpdse_convT_wgrad(const jpdse_conv_desc* d, const void* x, const void* dy, float* dw,
                      void* ws, size_t ws_bytes, void* stream);

/* ---- InstanceNorm2d(affine=False, eps) fused with activation / residual --------------- */
/* networks.py:31 (norm), :204,:216,:229,:245 (ReLU), :438,:446 (LeakyReLU 0.2),
 * :304 (x + conv_block(x): residual added after the second norm of a ResnetBlock). */
typedef struct jpdse_inorm_desc {
  int32_t dtype;
  int32_t N, H, W, C;
  int32_t act;          /* NONE | RELU | LRELU */
  float slope;
  float eps;            /* 1e-5 */
  int32_t has_residual; /* y = act(norm(x)) + residual */
  int32_t alias;        /* jpdse_inorm_bwd only, 0 = off (must be 0 in every other call): the backward runs over more gradient
                         * images than saved forward ones.  N counts the images of dy / dx; gradient image n reads x and stats of
                         * image n >= alias ? n - alias : n (x, stats hold N - alias images; 2 alias <= N).  InstanceNorm acts per image: each
                         * image's dx equals, bit for bit, that of the un-aliased call on a batch that contains it.  The PatchGAN
                         * walked backwards once for loss_G and loss_D uses it. */
} jpdse_inorm_desc;
size_t jpdse_inorm_workspace_size(const jpdse_inorm_desc* d);
/* stats: fp32 [N][CPAD(C)][2] = (mean, rstd), kept for backward */
int jpdse_inorm_fwd(const jpdse_inorm_desc* d, const void* x, const void* residual, void* y,
                    float* stats, void* ws, size_t ws_bytes, void* stream);
/* jpdse_inorm_fwd with the moment pass replaced by the per-block moments a conv epilogue wrote (jpdse_conv_fwd_moments):
 * a finalize over the `slots` blocks of each (image, channel) -- Chan's parallel-variance merge of the (mean, M2) slots in a
 * fixed order --, then the apply pass. */
int jpdse_inorm_fwd_from_moments(const jpdse_inorm_desc* d, const void* x, const float* moments, int32_t slots,
                                 const void* residual, void* y, float* stats, void* stream);
/* jpdse_inorm_bwd with the per-channel sums taken from the per-block slots a data-gradient epilogue wrote
 * (jpdse_conv_dgrad_fused_nsums): the slots of each (image, channel) are added in slot order, then the apply pass.
 * ws: jpdse_inorm_workspace_size(d) bytes. */
int jpdse_inorm_bwd_from_sums(const jpdse_inorm_desc* d, const void* x, const float* stats, const void* dy,
                              const float* sums, int32_t slots, void* dx, void* ws, size_t ws_bytes, void* stream);
/* dx from (x, stats, dy); the residual branch's gradient is dy itself */
int jpdse_inorm_bwd(const jpdse_inorm_desc* d, const void* x, const float* stats, const void* dy,
                    void* dx, void* ws, size_t ws_bytes, void* stream);

/* ---- pooling ------------------------------------------------------------------------ */
/* nn.AvgPool2d(3, stride=2, padding=1, count_include_pad=False)  networks.py:180,387 */
int jpdse_avgpool3s2_fwd(int32_t dtype, int32_t N, int32_t H, int32_t W, int32_t C, const void* x,
                         void* y, void* stream);
int jpdse_avgpool3s2_bwd(int32_t dtype, int32_t N, int32_t H, int32_t W, int32_t C, const void* dy,
                         void* dx, void* stream);
/* nn.MaxPool2d(2,2) inside VGG19 features (networks.py:477) */
int jpdse_maxpool2_fwd(int32_t dtype, int32_t N, int32_t H, int32_t W, int32_t C, const void* x,
                       void* y, void* stream);
int jpdse_maxpool2_bwd(int32_t dtype, int32_t N, int32_t H, int32_t W, int32_t C, const void* x,
                       const void* dy, void* dx, void* stream);

/* ---- elementwise pieces of the loss graph ----------------------------------------------- */
/* dz = dy * act'(.) evaluated from the activation OUTPUT y (ReLU, LeakyReLU, Tanh backward) */
int jpdse_act_bwd(int32_t dtype, int64_t n, int32_t act, float slope, const void* y, const void* dy,
                  void* dz, void* stream);
/* out = a + b (gradient fan-in where autograd would add) */
int jpdse_add(int32_t dtype, int64_t n, const void* a, const void* b, void* out, void* stream);
/* out[c] = sum over pixels of dy[p][c]  (bias gradients), fp32 [CPAD(C)] */
size_t jpdse_channel_sum_workspace_size(int64_t npix, int32_t C);
int jpdse_channel_sum(int32_t dtype, int64_t npix, int32_t C, const void* dy, float* out, void* ws,
                      size_t ws_bytes, void* stream);
/* dst[p][dst_c0 + i] = src[p][src_c0 + i], i < nch: torch.cat along channels
 * (model.py:455,595,733) and its backward (slice). */
int jpdse_channel_copy(int32_t dtype, int64_t npix, const void* src, int32_t src_cs, int32_t src_c0,
                       void* dst, int32_t dst_cs, int32_t dst_c0, int32_t nch, void* stream);
/* out = base with channels [c0, c0+nch) taken from img: `torch.cat((input_label, image), dim=1)`
 * (pix2pixHD_model.py:456,595) when the label/edge channels of `base` are already in place --
 * one pass instead of a copy of base plus a channel copy.  cs / img_cs: channel storage of
 * base,out / img. */
int jpdse_concat_channels(int32_t dtype, int64_t npix, const void* base, int32_t cs, const void* img,
                          int32_t img_cs, int32_t c0, int32_t nch, void* out, void* stream);
/* dst = src, nbytes a multiple of 16, both 16-byte aligned (assembling the batched [fake ; real] VGG19 input: networks.py:124-139) */
int jpdse_copy(int64_t nbytes, const void* src, void* dst, void* stream);
/* fill n elements with zero */
int jpdse_zero(int32_t dtype, int64_t n, void* p, void* stream);
/* dst = (dst_dtype) src, fp32 <-> bf16, n a multiple of 8: the gradient buckets of the optional bf16 all-reduce
 * (no reference counterpart: the reference has no collective, ctu/parsers/base_parser.py:234-237) */
int jpdse_cast(int32_t src_dtype, int32_t dst_dtype, int64_t n, const void* src, void* dst, void* stream);

/* ---- API-boundary layout conversion ---------------------------------------------------- */
/* fp32 NCHW (the x_dict tensors of ctu_dataset.py:124-128) -> NHWC compute dtype, C padded */
int jpdse_nchw_to_nhwc(int32_t dtype, int32_t N, int32_t C, int32_t H, int32_t W, const float* src,
                       void* dst, void* stream);
int jpdse_nhwc_to_nchw(int32_t dtype, int32_t N, int32_t C, int32_t H, int32_t W, const void* src,
                       float* dst, void* stream);
/* One-hot scatter of the label map + 4-neighbour instance-edge map, written to channels
 * [0, num_labels] of an NHWC tensor with `cs` storage channels (model.py:375-394,774-783).
 * label: fp32 [N,1,H,W] integer-valued; instance: int64 [N,1,H,W]. */
int jpdse_onehot_edge(int32_t dtype, int32_t N, int32_t H, int32_t W, int32_t num_labels,
                      const float* label, const int64_t* instance, void* dst, int32_t cs,
                      void* stream);

/* The whole input builder of a train step in ONE pass (model.py:375-394 one-hot + edges, :595 and :456 the two torch.cat):
 * for i < n_dst (1..3), dst[i] ([N,H,W,cs] NHWC) receives channels [0, num_labels) = one-hot(label), channel num_labels =
 * instance edge, channels [c0, c0 + nch) = img[i] ([N,H,W,img_cs] NHWC, same dtype; NULL: those lanes are zeroed and filled
 * in later by jpdse_insert_channels), every other lane zero.  The generator input and both halves of the discriminator
 * input are three destinations of one call: the label planes are read once and no intermediate "base" tensor exists. */
int jpdse_input_builder(int32_t dtype, int32_t N, int32_t H, int32_t W, int32_t num_labels, const float* label,
                        const int64_t* instance, int32_t n_dst, void* const* dst, const void* const* img, int32_t cs,
                        int32_t img_cs, int32_t c0, int32_t nch, void* stream);
/* The same pass for wide label sets (ADE20K: 151 one-hot lanes + edge + 3 image lanes = 160 storage channels).
 * jpdse_input_builder has one kernel per storage width up to 64 channels and refuses anything wider; this entry point takes
 * the same arguments with the same meaning for ANY cs % 8 == 0 with num_labels < cs: the vector count per pixel is a
 * run-time value of the one kernel behind it.  A label id >= num_labels lights no lane; lanes of [c0, c0 + nch) come from
 * img[i] (zero where img[i] is NULL); every other lane is zero.  Refusals are those of jpdse_input_builder, without the
 * width limit. */
int jpdse_input_builder_wide(int32_t dtype, int32_t N, int32_t H, int32_t W, int32_t num_labels, const float* label,
                             const int64_t* instance, int32_t n_dst, void* const* dst, const void* const* img, int32_t cs,
                             int32_t img_cs, int32_t c0, int32_t nch, void* /* hipStream_t */ stream);
/* dst[..., c0 : c0 + nch] = img[..., 0 : nch] in place (the generated image into the discriminator input, model.py:456):
 * touches only the 16-byte vectors of dst that hold those channels. */
int jpdse_insert_channels(int32_t dtype, int64_t npix, void* dst, int32_t cs, const void* img, int32_t img_cs, int32_t c0,
                          int32_t nch, void* stream);

/* ---- losses ------------------------------------------------------------------------- */
/* All reductions are fp32 and deterministic (two-stage).  `count` is the LOGICAL element
 * count the mean divides by (padding lanes are zero in both operands).
 * out[0] = mean |a-b|  (nn.L1Loss: networks.py:131, model.py:207,218) */
size_t jpdse_loss_workspace_size(int64_t n);
/* Deferred second stage.  Every jpdse_*_fwd / jpdse_l1_fwd_bwd below accepts out == NULL: the block partials then stay in `ws`
 * (which must not be reused before they are consumed) and ONE jpdse_loss_finalize call reduces any number of such terms --
 * out[0] = inv_count * sum(partial[0 .. n)) in index order, per term -- instead of one tiny launch per term (the train step has 20:
 * pix2pixHD_model.py:205-221).  n = jpdse_loss_partial_count(work items): 16-byte vectors of `a` for the L1 / MSE terms, pixels for
 * jpdse_mse_const_fwd.  `terms` is a HOST array (copied into the launch). */
typedef struct jpdse_loss_term {
  const float* partial;
  int32_t n;
  float inv_count;
  float* out;
} jpdse_loss_term;
int32_t jpdse_loss_partial_count(int64_t work_items);
int jpdse_loss_finalize(const jpdse_loss_term* terms, int32_t n_terms, void* stream);
int jpdse_l1_fwd(int32_t dtype, int64_t n, int64_t count, const void* a, const void* b, float* out,
                 void* ws, size_t ws_bytes, void* stream);
/* da = scale * (*gout) * sign(a-b) / count ; gout is a DEVICE scalar (no host sync) */
int jpdse_l1_bwd(int32_t dtype, int64_t n, int64_t count, const void* a, const void* b,
                 const float* gout, float scale, void* da, void* stream);
/* as jpdse_l1_bwd when `a` is the output of a ReLU and the gradient is wanted w.r.t. its
 * pre-activation: zero where a <= 0 (VGGLoss taps relu{1..5}_1, networks.py:124-139 -- fuses the
 * ReLU backward of torchvision's in-place nn.ReLU into the loss gradient). */
int jpdse_l1_bwd_relu(int32_t dtype, int64_t n, int64_t count, const void* a, const void* b,
                      const float* gout, float scale, void* da, void* stream);
/* L1Loss forward and backward in ONE pass over a, b: out[0] = mean|a-b| and
 * da = scale/count * sign(a-b) (* [a > 0] when relu_a).  Valid because the upstream gradient of every
 * L1 term of loss_G is a constant known at forward time (the loss weights of
 * pix2pixHD_trainer.py:48-56): saves re-reading both operands in the backward pass. */
int jpdse_l1_fwd_bwd(int32_t dtype, int64_t n, int64_t count, const void* a, const void* b, float* out,
                     float scale, int32_t relu_a, void* da, void* ws, size_t ws_bytes, void* stream);
/* out[0] = mean (a-b)^2 (nn.MSELoss distortion: model.py:219-220) */
int jpdse_mse_fwd(int32_t dtype, int64_t n, int64_t count, const void* a, const void* b, float* out,
                  void* ws, size_t ws_bytes, void* stream);
int jpdse_mse_bwd(int32_t dtype, int64_t n, int64_t count, const void* a, const void* b,
                  const float* gout, float scale, void* da, void* stream);
/* LSGAN: out[0] = mean over the LOGICAL channel 0 of (x - target)^2 (networks.py:90,112-119).
 * x is the 1-channel PatchGAN map stored with `cs` channels. */
int jpdse_mse_const_fwd(int32_t dtype, int64_t npix, int32_t cs, float target, const void* x,
                        float* out, void* ws, size_t ws_bytes, void* stream);
int jpdse_mse_const_bwd(int32_t dtype, int64_t npix, int32_t cs, float target, const void* x,
                        const float* gout, float scale, void* dx, void* stream);

/* Evaluation distortion on de-normalised, clipped, uint8-TRUNCATED images (ctu/utils/misc.py:64-95 `tensor2im`,
 * pix2pixHD_model.py:636-641): q(x) = uint8(clip((x * std[c] + mean[c]) * 255, 0, 255)) evaluated in IEEE double as
 * numpy does, then out[0] = mean |q(a) - q(b)| (mse = 0) or mean (q(a) - q(b))^2 (mse = 1) over npix * C elements,
 * on the 0..255 scale.  a, b: NHWC images with CPAD(C) storage channels, each fp32 or bf16; mean / std: HOST arrays
 * of C doubles (opt.normalize_mean / opt.normalize_std).  Replaces two device->host copies + numpy per call. */
size_t jpdse_quant_loss_workspace_size(void);
int jpdse_quant_loss(int32_t dtype_a, int32_t dtype_b, int64_t npix, int32_t C, const void* a, const void* b,
                     const double* mean, const double* std, int32_t mse, float* out, void* ws, size_t ws_bytes,
                     void* stream);

/* ---- learned codec: the encoder's stochastic binarizer and its bitstream --------------------------------------------
 * t, b: NHWC [N][H][W][CPAD(C)] in `dtype`.  Element e = (c*H + y)*W + x is the logical NCHW index inside an image. */
/* Binarizer (ctu/quantizers/binarize.py:13-65; t is the stored tanh output of the 1x1 conv).  train != 0:
 * b = ((1.0f - t) / 2.0f <= u) ? +1 : -1 (SoftSignFunction.forward, binarize.py:17-24) with t widened to fp32 and
 * u = (w >> 8) * 2^-24, w = word (e & 3) of Philox4x32-10(counter = (e >> 2, n_global0 + n, draw lo, draw hi),
 * key = (seed lo, seed hi)) -- the reference draws u with torch's uniform_; here it is a pure function of (seed, image index in
 * the global batch, draw, e), so codes do not depend on how a batch is split.  u != NULL (fp32 NCHW [N][C][H][W]) replaces
 * the generator.  train == 0: b = sign(t), sign(0) = 0 (DifferentiableSign eval, binarize.py:41-44).  Padding lanes of b
 * are written as 0.  The backward is the straight-through estimator (binarize.py:26-28): db passes unchanged. */
int jpdse_binarize_fwd(int32_t dtype, int32_t N, int32_t H, int32_t W, int32_t C, const void* t, void* b, int32_t train,
                       uint64_t seed, uint64_t draw, int64_t n_global0, const float* u, void* stream);
/* Per-image counts (model.py:468-491, get_eval_rate: torch.mean((b + 1) / 2) = (n_pos + n_zero / 2) / (C*H*W)):
 * counts[n][0] = #(b == +1), counts[n][1] = #(b == 0), int32, over the logical elements.  Deterministic (integer sums,
 * fixed order); ws: jpdse_code_stats_workspace_size() bytes. */
size_t jpdse_code_stats_workspace_size(int32_t dtype, int32_t N, int32_t H, int32_t W, int32_t C);
int jpdse_code_stats(int32_t dtype, int32_t N, int32_t H, int32_t W, int32_t C, const void* b, int32_t* counts, void* ws,
                     size_t ws_bytes, void* stream);
/* Code export (model.py:557-563 get_code: (code.view(N, -1) + 1) / 2).  packed == 0: out = fp32 [N][C*H*W] in NCHW flatten
 * order; packed != 0: out = uint8 [N][ceil(C*H*W / 8)], bit (b > 0) of element 8k+j in bit 7-j of byte k (np.packbits order). */
int jpdse_code_export(int32_t dtype, int32_t N, int32_t H, int32_t W, int32_t C, const void* b, int32_t packed, void* out,
                      void* stream);
/* Code import, the inverse of jpdse_code_export (no reference counterpart: the reference never decodes a stored code).
 * b = NHWC [N][H][W][CPAD(C)] in `dtype`: element e of image n becomes +1 or -1, never 0; every padding lane c >= C is
 * written as 0.  packed != 0: in = uint8 [N][ceil(C*H*W / 8)], element 8k+j = bit 7-j of byte k, every image starting on a
 * byte as jpdse_code_export writes it; the unused low bits of an image's last byte are ignored.  packed == 0: in = fp32
 * [N][C*H*W], in > 0.5f gives +1 and anything else (NaN included) -1.  So import(export(b)) == b except where b == 0 (the
 * eval binarizer's sign(0)): that element was exported as bit 0 (or 0.5) and comes back as -1 -- what a receiver sees.
 * A NULL pointer, a non-positive extent or a bad dtype is JPDSE_EINVAL before any launch. */
int jpdse_code_import(int32_t dtype, int32_t N, int32_t H, int32_t W, int32_t C, const void* in, int32_t packed, void* b,
                      void* /* hipStream_t */ stream);

/* ---- learned codec: entropy-coded bitstream (no reference counterpart; format: DESIGN.md 4.8) ---------------------------
 * A lossless, context-adaptive binary range coder over the bits (b > 0) of the code b = NHWC [N][H][W][CPAD(C)]: every
 * (image, channel) pair is one stream of H*W symbols in raster order with 16 adaptive probabilities (context = the coded
 * neighbours left | up << 1 | upleft << 2 | upright << 3), coded by the carry-propagating range coder of LZMA.  The payload
 * of one image is C little-endian uint32 stream lengths followed by the C streams in channel order.  Bit-exact and
 * deterministic: the same code gives the same bytes on every call.
 * Limits: N <= 65535, W <= 4096 and a payload capacity below 2^31 bytes; anything else is JPDSE_EINVAL before any launch, as
 * are a NULL pointer, a bad dtype, a non-positive extent and a buffer or row stride that is too small. */
/* Bytes one image's payload can never exceed: C * (4 + H*W + 8) (a symbol costs less than 6.05 bits); 0 for
 * a shape outside the limits.  Host only. */
size_t jpdse_code_entropy_capacity(int32_t H, int32_t W, int32_t C);
/* Host only; 0 for a shape outside the limits. */
size_t jpdse_code_entropy_workspace_size(int32_t N, int32_t H, int32_t W, int32_t C);
/* out: DEVICE uint8 [N][out_stride], out_stride >= jpdse_code_entropy_capacity(); image n's payload is the first sizes[n]
 * bytes of row n, the rest of the row is not written.  sizes, status: DEVICE int32 [N]; status[n] != 0: a stream of image n
 * outgrew its H*W + 8 bytes and was cut (the derived bound says it cannot; nothing is ever written past a capacity).
 * An exact 0 of the eval binarizer is coded as bit 0, as jpdse_code_export stores it.  ws:
 * jpdse_code_entropy_workspace_size() bytes. */
int jpdse_code_entropy_encode(int32_t dtype, int32_t N, int32_t H, int32_t W, int32_t C, const void* b, uint8_t* out,
                              int64_t out_stride, int32_t* sizes, int32_t* status, void* ws, size_t ws_bytes,
                              void* /* hipStream_t */ stream);
/* in: DEVICE uint8 [N][in_stride], payload n in the first sizes[n] bytes of row n; sizes: HOST int32 [N], checked against
 * [4 C, in_stride] before any launch.  b: every logical lane becomes +1 or -1 and every padding lane 0 -- what
 * jpdse_code_import writes for the raw code.  The length tables inside the payloads are device data and are not trusted: a
 * stream is clipped to its row, bytes past a stream's end read as 0 and the symbol count is fixed at H*W, so no payload can
 * make the call read outside `in` or write outside `b`. */
int jpdse_code_entropy_decode(int32_t dtype, int32_t N, int32_t H, int32_t W, int32_t C, const uint8_t* in, int64_t in_stride,
                              const int32_t* sizes, void* b, void* /* hipStream_t */ stream);

/* ---- learned codec: coded label and instance maps (no reference counterpart; format: DESIGN.md 4.9) ---------------------
 * A lossless, context-adaptive coder for the two integer maps the receiver of the learned codec needs.  Plane 0 (bit 0 of
 * plane_mask) is the label map, float32 [N][1][H][W] with integer values 0..255; plane 1 (bit 1) the instance map, int64
 * [N][1][H][W] with values 0..2^31-1 -- the tensors jpdse_input_builder reads.  Every plane of every image is cut into
 * strips of strip_rows rows (the last may be shorter); a strip is one independent stream: per pixel "equal to the left
 * one" / "equal to the upper one" in 11 adaptive contexts, else an 8- or 32-bit literal, through the range coder of the
 * entropy-coded bitstream above.  The payload of one plane of one image is S = ceil(H / strip_rows) little-endian uint32
 * stream lengths followed by the S streams in strip order.  Bit-exact and deterministic.
 * A stream's slot is its strip's raw size (1 or 4 bytes per pixel) + 8 bytes; a stream that needs more is cut and flagged,
 * and the caller stores that plane raw.
 * Limits: N <= 65535 (a grid dimension), S <= 65535 (compaction reads S lengths per stream: at most 2^32 reads per image),
 * and a capacity below 2^31 bytes (offsets inside a row are int32); anything else is JPDSE_EINVAL before any launch, as are
 * a NULL pointer, a non-positive extent or strip_rows, a plane mask outside 1..3, a missing buffer of a plane the mask
 * names and a row stride that is too small. */
/* Bytes of one image's row: per present plane 4 S + (H*W*raw + 8 S), label plane first; 0 for a shape outside the limits.
 * Plane 1's payload starts at jpdse_semantics_capacity(H, W, strip_rows, 1) when both planes are present.  Host only. */
size_t jpdse_semantics_capacity(int32_t H, int32_t W, int32_t strip_rows, int32_t plane_mask);
/* Host only; 0 for a shape outside the limits. */
size_t jpdse_semantics_workspace_size(int32_t N, int32_t H, int32_t W, int32_t strip_rows, int32_t plane_mask);
/* out: DEVICE uint8 [N][out_stride], out_stride >= jpdse_semantics_capacity(); sizes, status: DEVICE int32 [N][2], indexed
 * by plane; the entries of an absent plane are not written.  The payload of plane p of image n is the first sizes[n][p]
 * bytes at its plane offset of row n.  status[n][p] bit 0: a stream was cut (store the plane raw); bit 1: a value was out
 * of range (a label that is not an integer in [0, 255], an instance value outside [0, 2^31)): the payload is not usable.
 * label / inst may be NULL when the mask does not name their plane.  ws: jpdse_semantics_workspace_size() bytes. */
int jpdse_semantics_encode(int32_t N, int32_t H, int32_t W, int32_t strip_rows, int32_t plane_mask, const float* label,
                           const int64_t* inst, uint8_t* out, int64_t out_stride, int32_t* sizes, int32_t* status, void* ws,
                           size_t ws_bytes, void* /* hipStream_t */ stream);
/* in: DEVICE uint8 [N][in_stride]; the label payload of image n starts at byte 0 of row n and, with both planes, the
 * instance payload at inst_offset (ignored with one plane: that plane starts at 0).  sizes: DEVICE int32 [N][2] by plane;
 * sizes[n][p] <= 0: plane p of image n is not coded here and its output is left alone (the caller fills it from a raw
 * plane).  Nothing on the device is trusted: a size is clipped to the plane's part of the row, a table entry outside it
 * reads as 0, streams are clipped, bytes past a stream's end read as 0 and every strip decodes exactly its pixel count, so
 * no payload can make the call read outside `in` or write outside label / inst.  bad: DEVICE int32 [N], written by the
 * call: bit 0 a decoded label >= num_labels (1..256), bit 1 a decoded instance value >= 2^31. */
int jpdse_semantics_decode(int32_t N, int32_t H, int32_t W, int32_t strip_rows, int32_t plane_mask, int32_t num_labels,
                           const uint8_t* in, int64_t in_stride, int64_t inst_offset, const int32_t* sizes, float* label,
                           int64_t* inst, int32_t* bad, void* /* hipStream_t */ stream);

/* ---- evaluation metrics: L1, MSE and MS-SSIM of a reconstruction in one pass (test.py:114-125) --------------------------
 * fake (fp32 or bf16) and real (fp32): NHWC [N][H][W][CPAD(3)] normalised images; both are quantised with q() of
 * jpdse_quant_loss (the same device function) and compared on the 0..255 scale.  out: DEVICE array of doubles
 * [N][4 + 2*5]; per image
 *   out[0] = sum |q(fake) - q(real)|, out[1] = sum (q(fake) - q(real))^2 over the 3*H*W elements (integers, exact),
 *   out[2] = 3*H*W, out[3] = 0 (reserved),
 *   out[4..8] = cs_1..cs_5, out[9..13] = ssim_1..ssim_5: the per-scale means of the MS-SSIM maps (Wang, Simoncelli, Bovik
 *   2003; DESIGN.md 4.5: 11x11 Gaussian window of sigma 1.5 applied "valid" per channel, C1 = (0.01*255)^2,
 *   C2 = (0.03*255)^2, scales linked by a 2x2 mean).
 * The caller forms ms_ssim = prod_{j<5} cs_j^w_j * ssim_5^w_5 and PSNR in float64 from one read-back.  C must be 3 and
 * min(H, W) >= 176 (the fifth scale still holds one window), else JPDSE_EINVAL before any launch.  No floating-point
 * atomics: partials are combined in a fixed order, two calls give bit-identical `out`.  ws:
 * jpdse_eval_metrics_workspace_size() bytes (0 for an unsupported shape). */
size_t jpdse_eval_metrics_workspace_size(int32_t N, int32_t H, int32_t W, int32_t C);
int jpdse_eval_metrics(int32_t dtype_fake, int32_t dtype_real, int32_t N, int32_t H, int32_t W, int32_t C, const void* fake,
                       const void* real, const double* mean, const double* std, double* out, void* ws, size_t ws_bytes,
                       void* stream);
/* The same pass with the two integer sums also split by semantic class (the intent of get_sem_wise_distortion,
 * pix2pixHD_model.py:646-706, which cannot run as written).  label: DEVICE fp32 [N][1][H][W], integer-valued, the map
 * jpdse_input_builder reads; n_classes in [1, 256].  cls: DEVICE int64 [N][n_classes + 1][3]; row k of image n =
 * (sum |q(fake) - q(real)|, sum (q(fake) - q(real))^2, pixels) over the 3 channels of the pixels labelled k.  Row n_classes
 * collects every pixel whose label is outside [0, n_classes) or not an integer (NaN included), so per image the rows add up
 * to out[0], out[1] and H*W exactly.  `out` is what jpdse_eval_metrics writes for the same images, bit for bit; the images
 * are read once and the label map once.  Integer sums throughout: two calls give bit-identical cls.  A bad n_classes or a
 * NULL pointer is JPDSE_EINVAL before any launch; ws: jpdse_eval_metrics_sem_workspace_size() bytes (0 for an unsupported
 * shape or n_classes). */
size_t jpdse_eval_metrics_sem_workspace_size(int32_t N, int32_t H, int32_t W, int32_t C, int32_t n_classes);
/* The seventeen arguments travel in one struct, like the descriptors of the conv and norm families: the first fields are the
 * arguments of jpdse_eval_metrics with the same names and meanings. */
typedef struct jpdse_eval_metrics_sem_args {
  int32_t dtype_fake, dtype_real, N, H, W, C;
  const void* fake;    /* NHWC [N][H][W][CPAD(3)], fp32 or bf16 */
  const void* real;    /* NHWC fp32 */
  const float* label;  /* device fp32 [N][1][H][W] */
  int32_t n_classes;   /* 1..256 */
  const double* mean;  /* host, 3 doubles */
  const double* std;   /* host, 3 doubles */
  double* out;         /* device [N][14] */
  int64_t* cls;        /* device [N][n_classes + 1][3] */
  void* ws;
  size_t ws_bytes;
  void* stream;
} jpdse_eval_metrics_sem_args;
int jpdse_eval_metrics_sem(const jpdse_eval_metrics_sem_args* args);

/* ---- MS-SSIM training loss: --distortion_loss_fn ms_ssim (no reference counterpart) --------------------------
 * out[0] = mean_n (1 - ms_ssim_n) of fake against real, both NHWC [N][H][W][CPAD(3)] normalised images of the SAME `dtype`
 * (fp32 or bf16), de-normalised per channel (u = v * std[c] + mean[c]) and neither clipped nor quantised: L = 1, C1 = 1e-4,
 * C2 = 9e-4, otherwise the MS-SSIM of jpdse_eval_metrics (11x11 Gaussian window of sigma 1.5 applied "valid" per channel,
 * five scales linked by a 2x2 mean, ms_ssim_n = prod_{j<5} cs_j^w_j * ssim_5^w_5).  An image with one of those five means
 * <= 0 has ms_ssim_n = 0 and a gradient of exact zeros.  `out` is a DEVICE fp32 slot written by the call's own final kernel
 * (no jpdse_loss_finalize term).  stats (optional, DEVICE doubles [N][11]): cs_1..5, ssim_1..5, ms_ssim_n.
 * dfake != NULL: the same call also writes dfake = scale * d out[0] / d fake in fake's dtype and layout (padding lanes 0).
 * No atomics: two calls on the same buffers give bit-identical out, stats and dfake.  C must be 3 and min(H, W) >= 176, else
 * JPDSE_EINVAL before any launch; ws: jpdse_msssim_loss_workspace_size() bytes (0 for an unsupported shape; with_grad != 0
 * includes the coefficient maps and gradient planes a call with dfake needs). */
size_t jpdse_msssim_loss_workspace_size(int32_t N, int32_t H, int32_t W, int32_t C, int32_t with_grad);
typedef struct jpdse_msssim_loss_args {
  int32_t dtype, N, H, W, C;
  const void* fake;    /* NHWC [N][H][W][CPAD(3)] in `dtype` */
  const void* real;    /* the same shape and dtype */
  const double* mean;  /* host, 3 doubles */
  const double* std;   /* host, 3 doubles */
  float* out;          /* device fp32 slot */
  double* stats;       /* device [N][11], or NULL */
  void* dfake;         /* device, fake's shape and dtype, or NULL: forward only */
  float scale;         /* read when dfake != NULL */
  void* ws;
  size_t ws_bytes;
  void* stream;
} jpdse_msssim_loss_args;
int jpdse_msssim_loss(const jpdse_msssim_loss_args* args);

/* ---- learned codec: context-model rate term, --lambda_rate (no reference counterpart) ---------------------
 * The expected length of the code under a static form of the entropy-coded bitstream's context model, and its gradient
 * w.r.t. the binarizer's tanh output.  b, t, grad: NHWC [N][H][W][CPAD(C)] in `dtype`.  One stream per (image n, channel c);
 * bit = b > 0 (an exact 0 of the eval binarizer is bit 0); ctx = left | up << 1 | upleft << 2 | upright << 3 over the bits
 * of the same stream, a neighbour outside the frame counting as 0 -- the rule of jpdse_code_entropy_encode.
 *   n0 / n1 [n][c][k] = positions of the stream with ctx == k and bit 0 / 1                            (int32)
 *   p1 = (n1 + 1) / (n0 + n1 + 2),  cost1 = -log2(p1),  cost0 = -log2(1 - p1)                          (per stream and ctx)
 *   e = (1 + t) / 2 * cost1[ctx] + (1 - t) / 2 * cost0[ctx]                                            (per element)
 *   per_image[n] = sum_{c,y,x} e / pixels,   out[0] = sum_n per_image[n] / N                           (bits per image pixel)
 *   grad = scale * (cost1[ctx] - cost0[ctx]) / (2 * N * pixels)       (ctx and the costs are constants: stop-gradient)
 * t == NULL ("hard mode"): t := +1 where b > 0 and -1 elsewhere, so out[0] is the static conditional-entropy estimate of the
 * code.  The arithmetic is fp32 (the sums over partials fp64); grad is rounded once on its store, its padding lanes are
 * written as 0.  The counts are integer atomics and every floating-point sum has a fixed order: two calls on the same
 * buffers give bit-identical out, per_image, grad and counts.
 * Limits: N <= 65535, C <= 64 * 65535 and H * W <= 2^30 (a count fits an int32).  A NULL args, b or out, a bad dtype, a
 * non-positive extent or `pixels`, a NaN scale with grad, a shape beyond the limits and a workspace that is missing or too
 * small are all JPDSE_EINVAL before any launch.  ws: jpdse_code_rate_workspace_size() bytes (0 for a shape outside the
 * limits; host only). */
size_t jpdse_code_rate_workspace_size(int32_t N, int32_t H, int32_t W, int32_t C);
typedef struct jpdse_code_rate_args {
  int32_t dtype, N, H, W, C;
  int64_t pixels;      /* the image's H*W behind "per pixel" (not the code's) */
  const void* b;       /* the code as the binarizer wrote it */
  const void* t;       /* the tanh output, or NULL: hard mode */
  void* grad;          /* scale * d out[0] / d t in `dtype`, or NULL: value only */
  float scale;         /* read when grad != NULL */
  float* out;          /* device fp32 slot: R, unscaled */
  float* per_image;    /* device fp32 [N], or NULL */
  int32_t* counts;     /* device int32 [N][C][16][2], (n0, n1) per context, or NULL */
  void* ws;
  size_t ws_bytes;
  void* stream;
} jpdse_code_rate_args;
int jpdse_code_rate_loss(const jpdse_code_rate_args* args);

/* ---- learned codec: code-length map and per-class rate (no reference counterpart) -------------------------
 * The exact cost, symbol by symbol, that the adaptive model of the entropy-coded bitstream above assigns to a code.
 * b: NHWC [N][h][w][CPAD(C)] in `dtype`.  Every (image, channel) pair is one stream of h*w symbols in raster order, bit = b > 0
 * (an exact 0 is bit 0), with 16 adaptive 11-bit probabilities q of bit 0 starting at 1024, selected by
 * ctx = left | up << 1 | upleft << 2 | upright << 3 and updated q -= q >> 5 (bit 1) / q += (2048 - q) >> 5 (bit 0): the model
 * of jpdse_code_entropy_encode, statement for statement.  A symbol coded with q (before its update) costs T[q] for bit 0 and
 * T[2048 - q] for bit 1, T[v] = round(-log2(v / 2048) * 65536) for v in 1 .. 2047 and T[0] = T[2048] = 0: integers in units
 * of 2^-16 bit, at most T[31] = 396218 (6.05 bits).  All sums below are 64-bit integer sums of those units: order-free, two
 * calls give identical bits.
 *   symbol[n][y][x][c]   uint32, the cost of the symbol (LOGICAL channels, no padding lanes); optional
 *   cell[n][y][x]        = sum_c symbol: the rate map
 *   channel[n][c]        = sum_{y,x} symbol
 *   class_units[n][k]    = sum over the pixels p of image n with class k of cell[n][y(p) / s][x(p) / s], s = H / h = W / w: a
 *                          cell's units go undivided to each of its s*s pixels, the caller divides by s*s
 *   class_pixels[n][k]   = pixels of image n with class k
 * label: DEVICE fp32 [N][1][H][W]; the class of a pixel is jpdse_eval_metrics_sem's: its label when that is an integer in
 * [0, n_classes), else the extra last row k = n_classes (NaN included); both class tables are [N][n_classes + 1].  So
 * sum_k class_units[n][k] == s*s * sum cell[n] and sum_c channel[n][c] == sum cell[n], exactly.  label == NULL: no class
 * tables; H, W, n_classes and the two class pointers are not read.
 * The cost is the model's ideal code length, not a size: per stream |8 * stream bytes - units / 65536| <= 48 + h*w / 64 bits
 * (DESIGN.md 4.12).
 * JPDSE_EINVAL before any launch: a NULL args, b, cell or channel (with a label: class_units, class_pixels); a bad dtype; a
 * non-positive extent; w > 4096 (the walk keeps a row's bits in LDS, as the encoder does); N > 65535, C > 64 * 65535 or
 * N*h*w*C > 2^40; with a label: H, W that are not the same power-of-two multiple s >= 1 of h, w, n_classes outside [1, 256],
 * H*W*C > 2^40.  A workspace that is missing or too small is JPDSE_EWORKSPACE.  ws: jpdse_code_cost_workspace_size() bytes
 * (host only; 0 for a shape the call refuses or n_classes outside [0, 256], 0 standing for "no label map"). */
/* Host only: out[v] = T[v], v = 0 .. 2048, built in fp64. */
int jpdse_code_cost_table(uint32_t* out /* [2049] */);
size_t jpdse_code_cost_workspace_size(int32_t N, int32_t h, int32_t w, int32_t C, int32_t n_classes);
typedef struct jpdse_code_cost_args {
  int32_t dtype, N, h, w, C;
  const void* b;           /* the code */
  int32_t H, W;            /* the image's extents behind the label map */
  const float* label;      /* device fp32 [N][1][H][W], or NULL: no class tables */
  int32_t n_classes;       /* 1..256 with a label */
  uint32_t* symbol;        /* device uint32 [N][h][w][C], or NULL: aggregates only */
  uint64_t* cell;          /* device [N][h][w] */
  uint64_t* channel;       /* device [N][C] */
  uint64_t* class_units;   /* device [N][n_classes + 1], or NULL without a label */
  uint64_t* class_pixels;  /* device [N][n_classes + 1], or NULL without a label */
  void* ws;
  size_t ws_bytes;
  void* stream;
} jpdse_code_cost_args;
int jpdse_code_cost(const jpdse_code_cost_args* args);

/* ---- semantics-weighted distortion: --class_distortion_weights / --edge_distortion_weight (no reference counterpart;
 * DESIGN.md 4.11) ----------------------------------------------------------------------------------------------------------
 * The l1 / mse training distortion with a weight per pixel taken from the label and instance maps, and its gradient, in one
 * pass.  fake, real, dfake: NHWC [N][H][W][CPAD(C)] in `dtype` (padding lanes zero).
 *   w(p)   = table[label(p)] * (edge_w if edge(p) else 1)
 *            label(p) is truncated toward zero; a value outside [0, n_table) -- negative, >= n_table, NaN -- has weight 1
 *   edge(p): the id of p differs from the id of its left, right, upper or lower neighbour inside the same image (no wrap
 *            from a row's end to the next row, no neighbour across the image border or across images; the rule of the
 *            reference's get_edges, pix2pixHD_model.py:774-783).  Ids are compared as 64-bit integers.
 *   out[0] = sum_p sum_c w(p) f(d) / (N H W C),  d = fake - real,  f(d) = |d| (JPDSE_SEM_L1) or d^2 (JPDSE_SEM_MSE)
 *   dfake  = scale * w(p) * sign(d) / (N H W C)  (l1; sign(0) = 0 as jpdse_l1_fwd_bwd)   or   scale * w(p) * 2 d / (N H W C)
 * The normaliser is the element count, not sum w: a table of ones with edge_w = 1 IS jpdse_l1_fwd / jpdse_mse_fwd, and dfake
 * is then bit-identical to jpdse_l1_fwd_bwd's / jpdse_mse_bwd's (*gout = 1).  inst == NULL or edge_w == 1: no edge term, the ids
 * are not read.  `table` is a HOST array of n_table floats, copied into the launch.  `out` is a DEVICE fp32 slot written by
 * the call's own final kernel (no jpdse_loss_finalize term).  The arithmetic is fp32, the sum over block partials fp64; the
 * grid and every order of summation are fixed and there are no atomics: two calls on the same buffers give bit-identical
 * out and dfake.  ws: jpdse_loss_workspace_size() bytes.
 * JPDSE_EINVAL before any launch: a NULL args, fake, real, label, table or out; a bad dtype or kind; a non-positive extent or
 * N * H * W >= 2^31; n_table outside 1 .. JPDSE_SEM_TABLE; a table entry or edge_w that is negative or not finite; a NaN
 * scale with dfake; a workspace that is missing or too small. */
#define JPDSE_SEM_TABLE 256
enum { JPDSE_SEM_L1 = 0, JPDSE_SEM_MSE = 1 };
typedef struct jpdse_sem_loss_args {
  int32_t dtype, N, H, W, C;
  int32_t kind;        /* JPDSE_SEM_L1 or JPDSE_SEM_MSE */
  const void* fake;
  const void* real;
  const float* label;  /* device float32 [N][H][W] */
  const int64_t* inst; /* device int64 [N][H][W], or NULL: no edge term */
  const float* table;  /* host, n_table floats: the class weights of labels 0 .. n_table - 1 */
  int32_t n_table;
  float edge_w;
  float scale;         /* read when dfake != NULL */
  float* out;          /* device fp32 slot */
  void* dfake;         /* device, fake's shape and dtype, or NULL: value only */
  void* ws;
  size_t ws_bytes;
  void* stream;
} jpdse_sem_loss_args;
int jpdse_sem_weighted_loss(const jpdse_sem_loss_args* args);

/* ---- soft-to-hard vector quantizer: ctu.quantizers.S2HVQ (reference ctu/quantizers/s2h_vq.py) ------------
 * M vectors of D components against a learnable code book of L centres.  x: row-major [M][D] in `dtype` (fp32 or bf16);
 * code_book: fp32 [L][D]; every [M][L] matrix (p, dp, onehot, s, ds) is fp32, index is int32 [M].  Arithmetic is fp32.
 *   score        d[m][k]  = sum_j (x[m][j] - c[k][j])^2, j ascending: the direct form (s2h_vq.py:85-87), not the expansion
 *                           |x|^2 - 2 x.c + |c|^2, which cancels and changes the nearest centre
 *   soft_fwd     p[m][k]  = exp(-sigma (d[m][k] - dmin[m])) / sum_l exp(-sigma (d[m][l] - dmin[m])), dmin[m] = min_k d[m][k]:
 *                           finite for every finite x and every sigma > 0 (a row that is numerically one-hot included)
 *   hard_fwd     index[m] = the k of the smallest d[m][k], the LOWEST k on a tie; onehot[m][k] = (k == index[m]) when the
 *                           pointer is given.  A NaN score never wins; a row of NaNs gives some index inside [0, L)
 *   soft_bwd     g[m][k]  = p[m][k] (dp[m][k] - sum_l p[m][l] dp[m][l]),  dd = -sigma g
 *                dx[m][j] = 2 sum_k dd[m][k] (x[m][j] - c[k][j]), k ascending, stored in x's dtype
 *                dcode_book[k][j] = -2 sum_m dd[m][k] (x[m][j] - c[k][j]): fp32 partials per block in the workspace (m
 *                           ascending inside a block's tiles), merged in block order.  dx or dcode_book may be NULL
 *   decode       y[m]     = c[index[m]] in `dtype` (s2h_vq.py:182-183: the reference always decodes hard)
 *   decode_bwd   dcode_book[k] = sum over {m : index[m] == k} of dy[m], m ascending inside a block's tiles, the same merge
 *                An index outside [0, L) reads as centre 0 and sets bit 0 of the device int32 word `status` (a plain store;
 *                the word is never cleared by the library); it never causes an access outside the code book
 *   argmax       index[m] = the k of the largest s[m][k], the lowest k on a tie
 *   pmf          pmf[k]   = (sum_m s[m][k]) / M (s2h_vq.py:312): fp32 sums per block, merged in block order in fp64
 *   pmf_bwd      ds[m][k] = dpmf[k] / M
 * No atomics; the grids and every order of summation depend on (M, D, L) alone: two calls on the same buffers give
 * bit-identical results.  ws: jpdse_vq_workspace_size(M, D, L) bytes (host only; 0 for a shape outside the limits) serve
 * soft_bwd, decode_bwd and pmf of that shape; soft_bwd reads it only with a dcode_book.
 * JPDSE_EINVAL before any launch: a NULL args or required pointer; a bad dtype; D outside 1 .. 32, L outside 2 .. 512, M < 1,
 * M * L >= 2^31; a sigma that is not finite and positive; a workspace that is missing or too small.  No call allocates,
 * synchronises or throws. */
size_t jpdse_vq_workspace_size(int32_t M, int32_t D, int32_t L);
typedef struct jpdse_vq_soft_fwd_args {
  int32_t dtype, M, D, L;
  float sigma;
  const void* x;
  const float* code_book;
  float* p;                /* [M][L] */
  void* stream;
} jpdse_vq_soft_fwd_args;
int jpdse_vq_soft_fwd(const jpdse_vq_soft_fwd_args* args);
typedef struct jpdse_vq_hard_fwd_args {
  int32_t dtype, M, D, L;
  const void* x;
  const float* code_book;
  int32_t* index;          /* [M] */
  float* onehot;           /* [M][L], or NULL: indices only */
  void* stream;
} jpdse_vq_hard_fwd_args;
int jpdse_vq_hard_fwd(const jpdse_vq_hard_fwd_args* args);
typedef struct jpdse_vq_soft_bwd_args {
  int32_t dtype, M, D, L;
  float sigma;
  const float* dp;         /* [M][L] */
  const float* p;          /* [M][L], as soft_fwd stored it */
  const void* x;
  const float* code_book;
  void* dx;                /* [M][D] in `dtype`, or NULL */
  float* dcode_book;       /* [L][D], or NULL */
  void* ws;
  size_t ws_bytes;
  void* stream;
} jpdse_vq_soft_bwd_args;
int jpdse_vq_soft_bwd(const jpdse_vq_soft_bwd_args* args);
typedef struct jpdse_vq_decode_args {
  int32_t dtype, M, D, L;
  const int32_t* index;
  const float* code_book;
  void* y;                 /* [M][D] in `dtype` */
  int32_t* status;         /* device word */
  void* stream;
} jpdse_vq_decode_args;
int jpdse_vq_decode(const jpdse_vq_decode_args* args);
typedef struct jpdse_vq_decode_bwd_args {
  int32_t dtype, M, D, L;
  const int32_t* index;
  const void* dy;          /* [M][D] in `dtype` */
  float* dcode_book;       /* [L][D] */
  int32_t* status;         /* device word */
  void* ws;
  size_t ws_bytes;
  void* stream;
} jpdse_vq_decode_bwd_args;
int jpdse_vq_decode_bwd(const jpdse_vq_decode_bwd_args* args);
typedef struct jpdse_vq_argmax_args {
  int32_t M, L;
  const float* s;          /* [M][L] */
  int32_t* index;
  void* stream;
} jpdse_vq_argmax_args;
int jpdse_vq_argmax(const jpdse_vq_argmax_args* args);
typedef struct jpdse_vq_pmf_args {
  int32_t M, L;
  const float* s;          /* [M][L] */
  float* pmf;              /* [L] */
  void* ws;
  size_t ws_bytes;
  void* stream;
} jpdse_vq_pmf_args;
int jpdse_vq_pmf(const jpdse_vq_pmf_args* args);
typedef struct jpdse_vq_pmf_bwd_args {
  int32_t M, L;
  const float* dpmf;       /* [L] */
  float* ds;               /* [M][L] */
  void* stream;
} jpdse_vq_pmf_bwd_args;
int jpdse_vq_pmf_bwd(const jpdse_vq_pmf_bwd_args* args);

/* ---- soft-to-hard vector quantizer: code-book fit, one Lloyd (k-means) iteration per pass (vq_fit.hip) -------
 * x, code_book, d[m][k] and the limits are those of the quantizer above; a(m) = the nearest centre of x[m], the lowest k on a tie:
 * the index jpdse_vq_hard_fwd gives on the same inputs.  The STATE is five device tensors the caller owns:
 *   counts   int64 [L]     n[k] = the number of vectors with a(m) = k
 *   sums     fp64  [L][D]  s[k][j] = the sum of x[m][j] over the members of k
 *   sse      fp64  [L]     e[k] = the sum of the fp32 distances d[m][a(m)] over the members of k
 *   far_dist fp32  [L]     the largest member distance of k, -1 for a centre without members
 *   far_vec  fp32  [L][D]  the member that attains it (components converted to fp32; zeros without members); of equal distances
 *                          the earliest: the lowest m inside a call, and an earlier call before a later one
 *   lloyd_accum   one pass over x under a fixed code book.  first != 0 initialises the state, first == 0 adds to it (a later call
 *                 replaces far_dist / far_vec only on a strictly greater distance): any number of batches stream through one
 *                 iteration.  x is read once (and at most L rows once more, for far_vec); the index is never stored.  Per-block
 *                 fp32 partials in the workspace, merged in ascending block order in fp64 into the state.
 *   lloyd_update  the next code book from a state, in place in code_book, one block:
 *                 n[k] > 0:  c[k][j] = (float)(s[k][j] / (double)n[k])
 *                 n[k] == 0 and reseed: donors are the centres with n >= 2 and far_dist > 0, ranked by e descending, the lower k
 *                 first on equal e; the i-th dead centre in ascending k takes far_vec of the i-th donor, bit for bit, while i <
 *                 the number of donors; further dead centres, and all of them without reseed, keep c[k].  A donor keeps its mean.
 *                 report: int32 [2] = (dead centres, reseeded centres).
 * No atomics; every output element has one writer and every sum an order fixed by (M, D, L): two calls on the same buffers give
 * identical bits.  ws: jpdse_vq_lloyd_workspace_size(M, D, L) bytes (host only; 0 for a shape outside the limits).
 * JPDSE_EINVAL before any launch: a NULL args or pointer, a bad dtype, a shape outside the limits, a workspace that is missing or
 * too small.  No call allocates, synchronises or throws. */
size_t jpdse_vq_lloyd_workspace_size(int32_t M, int32_t D, int32_t L);
typedef struct jpdse_vq_lloyd_accum_args {
  int32_t dtype, M, D, L;
  int32_t first;
  const void* x;
  const float* code_book;
  int64_t* counts;         /* [L] */
  double* sums;            /* [L][D] */
  double* sse;             /* [L] */
  float* far_dist;         /* [L] */
  float* far_vec;          /* [L][D] */
  void* ws;
  size_t ws_bytes;
  void* stream;
} jpdse_vq_lloyd_accum_args;
int jpdse_vq_lloyd_accum(const jpdse_vq_lloyd_accum_args* args);
typedef struct jpdse_vq_lloyd_update_args {
  int32_t D, L, reseed;
  float* code_book;        /* [L][D], updated in place */
  const int64_t* counts;
  const double* sums;
  const double* sse;
  const float* far_dist;
  const float* far_vec;
  int32_t* report;         /* [2] */
  void* stream;
} jpdse_vq_lloyd_update_args;
int jpdse_vq_lloyd_update(const jpdse_vq_lloyd_update_args* args);

/* ---- soft-to-hard vector quantizer: coded index stream (no reference counterpart; format: DESIGN.md 4.14) ------------------
 * A lossless, order-0 adaptive L-ary range coder for the indices of the quantizer, and its decoder.  index: DEVICE int32 [M],
 * the row-major [n][code_len] code, every value in [0, L).  The M indices are dealt to S independent streams by interleaving:
 * stream s holds the symbols s, s + S, s + 2 S, ..., cnt_s = ceil((M - s) / S) of them.  A symbol is nb = max(1, bit_length(L - 1))
 * binary decisions, most significant bit first, through a bit tree (m = 1; code the bit with prob[m]; m = m << 1 | bit) of 2^nb
 * adaptive probabilities per stream (entry 0 unused); a decision is the adaptive binary decision of
 * jpdse_code_entropy_encode: 11-bit probabilities of bit 0 starting at 1024, shift 5, the carry rule, the unstored first byte,
 * the flush of five bytes.  A stream stores at most nb * cnt_s + 8 bytes (its slot).
 * Payload: S little-endian uint32 stream lengths, then the S streams in order.
 *   capacity(M, L, S)  = 4 S + the sum of the slots = nb M + 12 S: the most a payload can take; `out` must hold that many
 *   encode             writes the payload to out, its size to *size, and *status: bit 0 a stream was cut at its slot (the
 *                      bound makes that unreachable), bit 1 an index outside [0, L) was met and coded as 0.  Both device
 *                      words are written by the call's last kernel with plain stores
 *   decode             reads a payload of in_bytes bytes (device data it does not trust: a length that points outside the
 *                      payload is clipped to it, a byte past a stream's end reads as 0) and writes exactly M indices, all in
 *                      [0, L): a decoded value >= L (possible when L is no power of two) is written as L - 1 and sets bit 1
 *                      of *status with a plain store (the word is never cleared by the library)
 * Plain loads and stores, no atomics: two calls give identical bytes.  Every loop is bounded by M, nb or the bytes pending.
 * Limits: 2 <= L <= 512, M >= 1, 1 <= S <= min(M, 65535), nb M < 2^31 and capacity < 2^31.  Both size queries are host-only
 * and return 0 outside the limits.  JPDSE_EINVAL before any launch: a NULL args or pointer, a value outside the limits,
 * out_bytes below the capacity, a workspace that is missing or below jpdse_vq_index_workspace_size(), in_bytes below the
 * 4 S of the table or >= 2^31. */
size_t jpdse_vq_index_capacity(int32_t M, int32_t L, int32_t S);
size_t jpdse_vq_index_workspace_size(int32_t M, int32_t L, int32_t S);
typedef struct jpdse_vq_index_encode_args {
  int32_t M, L, S;
  const int32_t* index;    /* device [M] */
  uint8_t* out;            /* device, out_bytes >= capacity */
  int64_t out_bytes;
  int32_t* size;           /* device word: the payload's bytes */
  int32_t* status;         /* device word */
  void* ws;
  size_t ws_bytes;
  void* stream;
} jpdse_vq_index_encode_args;
int jpdse_vq_index_encode(const jpdse_vq_index_encode_args* args);
typedef struct jpdse_vq_index_decode_args {
  int32_t M, L, S;
  const uint8_t* in;       /* device, in_bytes: the payload */
  int64_t in_bytes;
  int32_t* index;          /* device [M] */
  int32_t* status;         /* device word */
  void* stream;
} jpdse_vq_index_decode_args;
int jpdse_vq_index_decode(const jpdse_vq_index_decode_args* args);

/* ---- soft-to-hard vector quantizer: coded index planes (no reference counterpart; format: DESIGN.md 4.19) ------------------
 * The code of ONE image as the feature map it is, coded with a spatial context.  index: DEVICE int32 [h * w * G], pixel by
 * pixel in raster order, groups ascending inside a pixel (cell (y, x, g) at (y * w + x) * G + g), every value in [0, L).  The
 * plane of a group is cut into K = ceil(h / strip_rows) strips of strip_rows rows (the last may be shorter); stream
 * s = k * G + g is strip k of group g: cnt_s = rows_k * w symbols in raster order, its own table, no look above the strip.
 * Per symbol v, with Lf / U / UL the left / upper / upper-left cell of the group inside the strip (a comparison with a cell
 * that does not exist is false):
 *   1. if Lf exists: the bit v == Lf with table entry (Lf == U) | (UL == Lf) << 1 | (UL == U) << 2
 *   2. if no bit 1 yet, U exists and U != Lf (true without Lf): the bit v == U with entry 8 + (UL == Lf), or 10 without Lf
 *   3. if no bit 1 yet: v through the bit tree of the index stream above, node m at entry 10 + m
 * A table is 10 + 2^nb adaptive probabilities, nb = max(1, bit_length(L - 1)); a decision is the adaptive binary decision of
 * jpdse_code_entropy_encode.  A stream stores at most (nb + 2) * cnt_s + 8 bytes (its slot).
 * Payload: S = K G little-endian uint32 stream lengths, then the S streams in order.
 *   capacity(...)      = 4 S + the sum of the slots = (nb + 2) h w G + 12 S; `out` must hold that many
 *   encode             writes the payload to out, its size to *size, and *status: bit 0 a stream was cut at its slot (the
 *                      bound makes that unreachable), bit 1 an index outside [0, L) was met; it is coded, and seen by later
 *                      symbols as their neighbour, as 0.  Both device words are written by the call's last kernel
 *   decode             reads a payload of in_bytes bytes (device data it does not trust: a length that points outside the
 *                      payload is clipped to it, a byte past a stream's end reads as 0) and writes exactly h w G indices, all
 *                      in [0, L): a literal is taken as read; a decoded value >= L is written, and seen by later symbols, as
 *                      L - 1 and sets bit 1 of *status with a plain store (the word is never cleared by the library)
 * Plain loads and stores, no atomics: two calls give identical bytes.  Every loop is bounded by cnt_s, nb or the bytes pending.
 * Limits: 2 <= L <= 512, h, w, G, strip_rows >= 1, S <= 65535, h w G < 2^31 and capacity < 2^31.  Both size queries are
 * host-only and return 0 outside the limits.  JPDSE_EINVAL before any launch: a NULL args or pointer, a value outside the
 * limits, out_bytes below the capacity, a workspace that is missing or below jpdse_vq_plane_workspace_size(), in_bytes below
 * the 4 S of the table or >= 2^31. */
size_t jpdse_vq_plane_capacity(int32_t h, int32_t w, int32_t G, int32_t L, int32_t strip_rows);
size_t jpdse_vq_plane_workspace_size(int32_t h, int32_t w, int32_t G, int32_t L, int32_t strip_rows);
typedef struct jpdse_vq_plane_encode_args {
  int32_t h, w, G, L, strip_rows;
  const int32_t* index;    /* device [h * w * G] */
  uint8_t* out;            /* device, out_bytes >= capacity */
  int64_t out_bytes;
  int32_t* size;           /* device word: the payload's bytes */
  int32_t* status;         /* device word */
  void* ws;
  size_t ws_bytes;
  void* stream;
} jpdse_vq_plane_encode_args;
int jpdse_vq_plane_encode(const jpdse_vq_plane_encode_args* args);
typedef struct jpdse_vq_plane_decode_args {
  int32_t h, w, G, L, strip_rows;
  const uint8_t* in;       /* device, in_bytes: the payload */
  int64_t in_bytes;
  int32_t* index;          /* device [h * w * G] */
  int32_t* status;         /* device word */
  void* stream;
} jpdse_vq_plane_decode_args;
int jpdse_vq_plane_decode(const jpdse_vq_plane_decode_args* args);

/* ---- soft-to-hard vector quantizer: code-length maps of the two coders (no reference counterpart) ----------
 * The exact cost, symbol by symbol, that the adaptive model of the coded index stream (index_cost) or of the coded index
 * planes (plane_cost) above assigns to the indices of ONE image.  index: DEVICE int32, in the layout of the matching encode
 * call.  A binary decision coded with the probability q of bit 0 (before its update q -= q >> 5 for bit 1, q += (2048 - q) >> 5
 * for bit 0) costs T[q] for bit 0 and T[2048 - q] for bit 1, T the table of jpdse_code_cost_table: integers in units of
 * 2^-16 bit.  The cost of a symbol is the sum over the decisions its coder spends on it, entries and conditions as stated
 * above, statement for statement:
 *   index_cost   symbol m lies in stream m % S and costs the nb bit-tree decisions of that stream's table, in stream order;
 *                it belongs to cell m / G and group m % G (G >= 1 divides M; G need not divide S)
 *   plane_cost   symbol (y, x, g) lies in stream k * G + g and costs its left-match flag (rule 1, if coded), its upper-match
 *                flag (rule 2, if coded) and, if neither matched, the nb literal decisions (rule 3); cell y * w + x, group g
 * An index outside [0, L) is priced as the coder codes it -- as 0, and seen as 0 by its neighbours -- and sets bit 1 of
 * *status, which the call writes (0 otherwise).  All sums are 64-bit integer sums of units: order-free, two calls give
 * identical bits.
 *   symbol[m]            uint32, the cost of the symbol at its own position in the index tensor; optional
 *   cell[i]              = sum_g symbol[i * G + g], i < M / G: the rate map
 *   group[g]             = sum_i symbol[i * G + g]
 *   stream_units[s]      = the sum of the costs of the symbols of stream s
 *   stream_decisions[s]  = the binary decisions stream s coded: nb * cnt_s for index_cost, data dependent for plane_cost
 *   class_units[k], class_pixels[k]   the class tables of jpdse_code_cost for N = 1, same rule, same kernel: a cell's units go
 *                        undivided to each of the s*s pixels it covers, row n_classes collects the pixels without a class
 * So sum cell == sum group == sum stream_units, and sum_k class_units[k] == s*s * sum cell, exactly.
 * label: DEVICE fp32 [1][1][H][W], H = s h and W = s w with s a power of two; index_cost reads the cell grid h, w
 * (h * w * G == M) with a label only.  label == NULL: no class tables; h, w (index_cost), H, W, n_classes and the two class
 * pointers are not read.
 * The cost is the model's ideal code length, not a size: per stream
 *   |8 * stream bytes - stream_units / 65536| <= 48 + stream_decisions / 64 bits.
 * Plain loads and stores; the only atomics are the integer ones of the class tables.  Every loop is bounded by the shape.
 * Limits: those of the matching encode call; G >= 1 dividing M; with a label those of jpdse_code_cost's label path
 * (n_classes in [1, 256], H*W*G <= 2^40).  JPDSE_EINVAL before any launch: a NULL args, index, cell, group, stream_units,
 * stream_decisions or status (with a label: class_units, class_pixels), a value outside the limits, a workspace that is not
 * 16-byte aligned.  A workspace that is missing or too small is JPDSE_EWORKSPACE.  ws: the size query's bytes (host only; 0
 * for a shape the call refuses or n_classes outside [0, 256], 0 standing for "no label map"). */
size_t jpdse_vq_index_cost_workspace_size(int32_t M, int32_t L, int32_t S, int32_t G, int32_t n_classes);
typedef struct jpdse_vq_index_cost_args {
  int32_t M, L, S, G;
  const int32_t* index;        /* device [M] */
  int32_t h, w;                /* the cell grid, h * w * G == M; read with a label only */
  int32_t H, W;                /* the image's extents behind the label map */
  const float* label;          /* device fp32 [1][1][H][W], or NULL: no class tables */
  int32_t n_classes;           /* 1..256 with a label */
  uint32_t* symbol;            /* device uint32 [M], or NULL: aggregates only */
  uint64_t* cell;              /* device [M / G] */
  uint64_t* group;             /* device [G] */
  uint64_t* stream_units;      /* device [S] */
  uint32_t* stream_decisions;  /* device [S] */
  int32_t* status;             /* device word */
  uint64_t* class_units;       /* device [n_classes + 1], or NULL without a label */
  uint64_t* class_pixels;      /* device [n_classes + 1], or NULL without a label */
  void* ws;
  size_t ws_bytes;
  void* stream;
} jpdse_vq_index_cost_args;
int jpdse_vq_index_cost(const jpdse_vq_index_cost_args* args);
size_t jpdse_vq_plane_cost_workspace_size(int32_t h, int32_t w, int32_t G, int32_t L, int32_t strip_rows, int32_t n_classes);
typedef struct jpdse_vq_plane_cost_args {
  int32_t h, w, G, L, strip_rows;
  const int32_t* index;        /* device [h * w * G] */
  int32_t H, W;                /* the image's extents behind the label map */
  const float* label;          /* device fp32 [1][1][H][W], or NULL: no class tables */
  int32_t n_classes;           /* 1..256 with a label */
  uint32_t* symbol;            /* device uint32 [h * w * G], or NULL: aggregates only */
  uint64_t* cell;              /* device [h * w] */
  uint64_t* group;             /* device [G] */
  uint64_t* stream_units;      /* device [S], S = ceil(h / strip_rows) * G */
  uint32_t* stream_decisions;  /* device [S] */
  int32_t* status;             /* device word */
  uint64_t* class_units;       /* device [n_classes + 1], or NULL without a label */
  uint64_t* class_pixels;      /* device [n_classes + 1], or NULL without a label */
  void* ws;
  size_t ws_bytes;
  void* stream;
} jpdse_vq_plane_cost_args;
int jpdse_vq_plane_cost(const jpdse_vq_plane_cost_args* args);

/* ---- vector-quantizer bottleneck: quantize in one call, [M][L] never in memory (vq_bottleneck.hip) ---------
 * The quantizer above as a layer: features in, features out.  x, y, dy, dx: row-major [M][D] in `dtype`; code_book: fp32
 * [L][D]; d[m][k] and p[m][k] as defined above (the direct score, j ascending; the row minimum subtracted, the entry at the
 * minimum exactly 1 before the division).
 *   quantize_fwd  index[m] = the k of the smallest d[m][k], the LOWEST k on a tie, a NaN never wins (a row of NaNs: 0)
 *                 y[m]     = c[index[m]] when hard_forward: a bit-exact gather, rounded to nearest-even for bf16; otherwise
 *                            y[m][j] = sum_k p[m][k] c[k][j], k ascending (the division by the row sum applied to the sum)
 *                 pmf[k]   = (sum_m p[m][k]) / M when the pointer is given: fp32 sums per block (m ascending inside a tile's
 *                            parts, parts and tiles in order), merged in block order in fp64
 *   quantize_bwd  the gradient of the SOFT form whatever hard_forward was (straight-through); p is recomputed from x
 *                 dp[m][k] = <dy[m], c[k]> + dpmf[k] / M (dpmf may be NULL: no second term)
 *                 g = p (dp - <p, dp>), dd = -sigma g
 *                 dx[m][j] = 2 sum_k dd[m][k] (x[m][j] - c[k][j]), k ascending, in `dtype`
 *                 dcode_book[k][j] = sum_m (p[m][k] dy[m][j] - 2 dd[m][k] (x[m][j] - c[k][j])): fp32 partials per block, merged
 *                 in block order.  dx or dcode_book may be NULL
 * No atomics; grids and orders of summation depend on (M, D, L) alone: two calls give identical bits.  ws:
 * jpdse_vq_quantize_workspace_size(M, D, L) bytes (host only; 0 outside the limits), read only with a pmf or a dcode_book.
 * JPDSE_EINVAL before any launch: the limits and refusals of the quantizer above (D 1 .. 32, L 2 .. 512, M >= 1, M * L < 2^31,
 * sigma finite and positive, NULL args or required pointer, bad dtype, workspace missing or too small). */
size_t jpdse_vq_quantize_workspace_size(int32_t M, int32_t D, int32_t L);
typedef struct jpdse_vq_quantize_fwd_args {
  int32_t dtype, M, D, L;
  float sigma;
  int32_t hard_forward;
  const void* x;
  const float* code_book;
  void* y;                 /* [M][D] in `dtype` */
  int32_t* index;          /* [M] */
  float* pmf;              /* [L], or NULL */
  void* ws;
  size_t ws_bytes;
  void* stream;
} jpdse_vq_quantize_fwd_args;
int jpdse_vq_quantize_fwd(const jpdse_vq_quantize_fwd_args* args);
typedef struct jpdse_vq_quantize_bwd_args {
  int32_t dtype, M, D, L;
  float sigma;
  const void* dy;          /* [M][D] in `dtype` */
  const void* x;
  const float* code_book;
  const float* dpmf;       /* [L], or NULL */
  void* dx;                /* [M][D] in `dtype`, or NULL */
  float* dcode_book;       /* [L][D], or NULL */
  void* ws;
  size_t ws_bytes;
  void* stream;
} jpdse_vq_quantize_bwd_args;
int jpdse_vq_quantize_bwd(const jpdse_vq_quantize_bwd_args* args);

/* ---- vector-quantizer bottleneck: the rate term on per-group histograms (vq_bottleneck.hip) -----------------
 * Vectors m = 0 .. M - 1 fall into G >= 1 groups, G | M, g(m) = m % G (4.15's layout m = pixel * (cout / D) + group), n = M / G
 * vectors per group.  p[m][k] is the soft assignment above (here e[m][k] * (1 / s[m]): one division per vector); with `hard`
 * the one-hot of quantize_fwd's index[m].
 *   hist[g][k]  = sum over m with g(m) = g of p[m][k]
 *   q[g][k]     = hist[g][k] / n
 *   bits        = - sum_g sum_k hist[g][k] log2 q[g][k], terms with hist <= 0 dropped
 *   rate        = bits / denom                 (denom = N H W: bits per pixel of the local batch; denom = M: bits per index)
 *   dhist[g][k] = scale (-(log2 q[g][k] + 1 / ln 2)) / denom where hist > 0, else 0: scale * d rate / d hist
 *   rate_fwd    one launch sums p (recomputed from x; [M][L] is never stored) into one fp32 partial [G][L] per block, a second
 *               launch of one block merges the partials in block order in fp64, forms q, bits, rate and dhist in fp64 and
 *               writes hist, rate and dhist as fp32.  hist or dhist may be NULL.  Order of the fp32 sums: G a power of two
 *               <= 64 whose per-wave table fits LDS -- the lanes of a wave that share a group (lane % G) are added across
 *               the wave with xor-shuffles, offsets 32, 16, .. G in that order (hard: counted from a ballot, exact), the G
 *               owner lanes add the result into the wave's own LDS table tile after tile, and the waves of a block are merged
 *               in wave order; any other G -- m ascending inside a tile, tiles of a block in order.  bits: every thread of the
 *               final block adds its entries i = g L + k in ascending i (i = t, t + 1024, ..), the 1024 sums are added in
 *               ascending t, 32 at a time, then the 32 in order.
 *   quantize_bwd_grouped   quantize_bwd with dp[m][k] = <dy[m], c[k]> + dhist[g(m)][k] (no division by M: dhist is the gradient
 *               w.r.t. the un-normalised sums); everything after dp as above.  dhist NULL: exactly quantize_bwd with dpmf NULL.
 * No atomics; grids, tiles and orders of summation depend on (M, D, L, G) alone: two calls give identical bits.  ws of
 * rate_fwd: jpdse_vq_rate_workspace_size(M, D, L, G) bytes (host only; 0 outside the limits); of quantize_bwd_grouped:
 * jpdse_vq_quantize_workspace_size, with a dcode_book.  JPDSE_EINVAL before any launch: the limits and refusals of the calls
 * above, and G < 1, M % G != 0, G * L > 65536, scale or denom not finite, denom <= 0, NULL rate. */
size_t jpdse_vq_rate_workspace_size(int32_t M, int32_t D, int32_t L, int32_t G);
typedef struct jpdse_vq_rate_fwd_args {
  int32_t dtype, M, D, L, G;
  float sigma;
  int32_t hard;
  const void* x;           /* [M][D] in `dtype` */
  const float* code_book;  /* [L][D] */
  float scale, denom;
  float* hist;             /* [G][L], or NULL */
  float* rate;             /* [1] */
  float* dhist;            /* [G][L], or NULL */
  void* ws;
  size_t ws_bytes;
  void* stream;
} jpdse_vq_rate_fwd_args;
int jpdse_vq_rate_fwd(const jpdse_vq_rate_fwd_args* args);
typedef struct jpdse_vq_quantize_bwd_grouped_args {
  int32_t dtype, M, D, L, G;
  float sigma;
  const void* dy;          /* [M][D] in `dtype` */
  const void* x;
  const float* code_book;
  const float* dhist;      /* [G][L], or NULL */
  void* dx;                /* [M][D] in `dtype`, or NULL */
  float* dcode_book;       /* [L][D], or NULL */
  void* ws;
  size_t ws_bytes;
  void* stream;
} jpdse_vq_quantize_bwd_grouped_args;
int jpdse_vq_quantize_bwd_grouped(const jpdse_vq_quantize_bwd_grouped_args* args);

/* ---- soft-to-hard vector quantizer: entropy-constrained assignment (vq_ec.hip) ---------------------------------
 * Vectors and groups as in the rate term above (G | M, g(m) = m % G).  d[m][k] is the direct score of jpdse_vq_hard_fwd.
 *   ec_assign   index[m] = arg-min_k d[m][k] + bias[g(m)][k], the lowest k on equal cost.  bias fp32 [G][L], or NULL for all
 *               zero; the caller scales it (the kernel knows nothing about code lengths); one fp32 add per centre after the
 *               score loop, so a zero or NULL bias gives jpdse_vq_hard_fwd's index for index.  +inf is a legal entry: that
 *               centre is never chosen while another of its row is finite; a row of +inf alone gives index 0.
 *               hist int32 [G][L], or NULL: hist[g][k] = the vectors of group g with index k (exact).
 *               sse fp64 [G], or NULL: sse[g] = the sum of the chosen d[m][index[m]] over group g, WITHOUT the bias; each d is
 *               widened to fp64 before it is added.
 *   ec_lengths  n[g] = sum_k hist[g][k]; bias[g][k] = lambda (log2 n[g] - log2 hist[g][k]) in fp64, rounded to fp32; +inf
 *               where hist[g][k] <= 0; exact zeros everywhere when lambda == 0.  bits fp64 [G]: bits[g] = sum_k hist[g][k]
 *               (log2 n[g] - log2 hist[g][k]), the ideal code length of the group under its own histogram.  bias or bits may be
 *               NULL, not both.
 * No atomics: every block sums into a table of its own, the tables are merged in block order; two calls give identical bits.
 * ws of ec_assign, with a hist or an sse: jpdse_vq_ec_workspace_size(M, D, L, G) bytes, 8-byte aligned (host only; 0 outside the
 * limits 1 <= D <= 32, 2 <= L <= 512, M >= 1, M * L < 2^31, G >= 1, M % G == 0, G * L <= 65536).  JPDSE_EINVAL before any
 * launch: those limits, a bad dtype, NULL x, code_book or index, a workspace too small; ec_lengths: L, G * L, a lambda that
 * is negative or not finite, NULL hist, bias and bits both NULL. */
size_t jpdse_vq_ec_workspace_size(int32_t M, int32_t D, int32_t L, int32_t G);
typedef struct jpdse_vq_ec_assign_args {
  int32_t dtype, M, D, L, G;
  const void* x;           /* [M][D] in `dtype` */
  const float* code_book;  /* [L][D] */
  const float* bias;       /* [G][L], or NULL */
  int32_t* index;          /* [M] */
  int32_t* hist;           /* [G][L], or NULL */
  double* sse;             /* [G], or NULL */
  void* ws;
  size_t ws_bytes;
  void* stream;
} jpdse_vq_ec_assign_args;
int jpdse_vq_ec_assign(const jpdse_vq_ec_assign_args* args);
typedef struct jpdse_vq_ec_lengths_args {
  int32_t G, L;
  double lambda;
  const int32_t* hist;     /* [G][L] */
  float* bias;             /* [G][L], or NULL */
  double* bits;            /* [G], or NULL */
  void* stream;
} jpdse_vq_ec_lengths_args;
int jpdse_vq_ec_lengths(const jpdse_vq_ec_lengths_args* args);

/* ---- residual vector quantizer: S stages in one call (vq_residual.hip) ------------------------------------------
 * x, y, dy, dx: row-major [M][D] in `dtype`; books: fp32 [S][L][D], S <= JPDSE_VQ_RES_MAX_STAGES; n_stages <= S of them in use;
 * index: int32 [n_stages][M], stage-major.  With r_1 = x widened to fp32:
 *   index[s][m] = arg-min_k |r_s - C_s[k]|^2, the direct score of jpdse_vq_hard_fwd, the LOWEST k on a tie
 *   r_{s+1}     = r_s - C_s[index[s][m]]: one fp32 subtraction per component, never rounded between the stages
 *   y[m]        = C_1[index[0][m]] + .. + C_n[index[n-1][m]]: fp32, stage order, starting from the first centre, rounded once
 *   res_fwd     one launch; sse fp64 [n_stages] or NULL: sse[s] = sum_m |r_{s+2}|^2 (the error after stage s), every square formed
 *               and added in fp64, per block, the blocks merged in order; residual fp32 [M][D] or NULL: r_{n_stages+1}.
 *               n_stages == 0 is legal: y = 0 and residual = x widened.
 *   res_decode  y from the indices, bit for bit res_fwd's; an index outside [0, L) reads as centre 0 and sets *status to 1.
 *   res_bwd     the gradient of the SOFT form of every stage (straight-through, as quantize_bwd), stages descending, h_{n+1} = 0:
 *               a_s = dy - h_{s+1}; (u_s, dbooks[s]) = quantize_bwd at the input r_s (recomputed from x and index by the
 *               subtractions above) with the upstream gradient a_s and no dpmf; h_s = h_{s+1} + u_s; dx = h_1.  dbooks fp32
 *               [n_stages][L][D]: fp32 partials per block, merged in block order.  dx or dbooks may be NULL.
 * No atomics; grids and orders of summation depend on (M, D, L, n_stages) alone: two calls give identical bits.  ws:
 * jpdse_vq_res_workspace_size(M, D, L, n_stages) bytes, 8-byte aligned (host only; 0 outside the limits), read only with an sse
 * or a dbooks.  JPDSE_EINVAL before any launch: D 1 .. 32, L 2 .. 512, M >= 1, M * L < 2^31, S 1 .. 8, n_stages 0 .. S (decode,
 * bwd: 1 .. S), sigma finite and positive, NULL args or required pointer, bad dtype, workspace missing or too small. */
#define JPDSE_VQ_RES_MAX_STAGES 8
size_t jpdse_vq_res_workspace_size(int32_t M, int32_t D, int32_t L, int32_t S);
typedef struct jpdse_vq_res_fwd_args {
  int32_t dtype, M, D, L, S, n_stages;
  const void* x;
  const float* books;
  void* y;
  int32_t* index;
  double* sse;             /* [n_stages], or NULL */
  float* residual;         /* [M][D], or NULL */
  void* ws;
  size_t ws_bytes;
  void* stream;
} jpdse_vq_res_fwd_args;
int jpdse_vq_res_fwd(const jpdse_vq_res_fwd_args* args);
/* res_rows_fwd: index and y of res_fwd, bit for bit, by one thread per vector with the residual in registers: no
 * sse, no residual, no workspace.  n_stages 1 .. S; otherwise res_fwd's limits and JPDSE_EINVAL before any launch. */
typedef struct jpdse_vq_res_rows_fwd_args {
  int32_t dtype, M, D, L, S, n_stages;
  const void* x;
  const float* books;
  void* y;
  int32_t* index;          /* [n_stages][M] */
  void* stream;
} jpdse_vq_res_rows_fwd_args;
int jpdse_vq_res_rows_fwd(const jpdse_vq_res_rows_fwd_args* args);
typedef struct jpdse_vq_res_decode_args {
  int32_t dtype, M, D, L, S, n_stages;
  const int32_t* index;
  const float* books;
  void* y;
  int32_t* status;         /* [1] */
  void* stream;
} jpdse_vq_res_decode_args;
int jpdse_vq_res_decode(const jpdse_vq_res_decode_args* args);
typedef struct jpdse_vq_res_bwd_args {
  int32_t dtype, M, D, L, S, n_stages;
  float sigma;
  const void* dy;
  const void* x;
  const float* books;
  const int32_t* index;
  void* dx;                /* [M][D] in `dtype`, or NULL */
  float* dbooks;           /* [n_stages][L][D], or NULL */
  void* ws;
  size_t ws_bytes;
  void* stream;
} jpdse_vq_res_bwd_args;
int jpdse_vq_res_bwd(const jpdse_vq_res_bwd_args* args);

/* res_ec_assign (vq_res_ec.hip): the entropy-constrained code of the first n_stages stages, one thread per
 * vector as res_rows_fwd.  G groups, g(m) = m % G, G | M.  bias fp32 [n_stages][G][L], or NULL for all zero; per stage
 *   index[s][m] = arg-min_k d(r_s, C_s[k]) + bias[s][g(m)][k], d the score of res_rows_fwd, the bias one fp32 add after the score
 *                 loop; strict <: the lowest k on equal cost, a +inf cost never replaces anything, a row of +inf alone gives 0
 *   r_{s+1}, y    as above.  y may be NULL (the rounds before the last): then no sum is formed.
 *   hist          int32 [n_stages][G][L]: hist[s][g][k] = the vectors of group g with index[s] == k (exact)
 *   sse           fp64 [n_stages][G]: the sum over group g of the chosen d(r_s, C_s[index[s][m]]) WITHOUT the bias, each widened
 *                 to fp64: the squared error of the stage prefix 1 .. s.  hist and sse are both given or both NULL.
 * A NULL bias gives res_rows_fwd's index and y bit for bit.  No atomics: every block sums into a table of its own, the tables are
 * merged in block order; grid and owners depend on (M, D, L, G, n_stages) alone: two calls give identical bits.  ws, with hist and
 * sse: jpdse_vq_res_ec_workspace_size(M, D, L, G, n_stages) bytes, 8-byte aligned (host only; 0 outside the limits).
 * JPDSE_EINVAL before any launch: res_rows_fwd's limits (n_stages 1 .. S), G >= 1, M % G == 0, G * L <= 65536, n_stages * G * L <=
 * 65536, NULL args, x, books or index, one of hist and sse without the other, a workspace missing, too small or misaligned. */
size_t jpdse_vq_res_ec_workspace_size(int32_t M, int32_t D, int32_t L, int32_t G, int32_t n_stages);
typedef struct jpdse_vq_res_ec_assign_args {
  int32_t dtype, M, D, L, S, n_stages, G;
  const void* x;
  const float* books;
  const float* bias;       /* [n_stages][G][L], or NULL */
  void* y;                 /* [M][D] in `dtype`, or NULL */
  int32_t* index;          /* [n_stages][M] */
  int32_t* hist;           /* [n_stages][G][L], or NULL */
  double* sse;             /* [n_stages][G], or NULL */
  void* ws;
  size_t ws_bytes;
  void* stream;
} jpdse_vq_res_ec_assign_args;
int jpdse_vq_res_ec_assign(const jpdse_vq_res_ec_assign_args* args);

/* ---- residual vector quantizer: the rate term (vq_res_rate.hip, vq_residual.hip) ---------------------------------
 * The rate term on per-group histograms above (4.16), for the first n_stages of S stages.  Vectors m = 0 .. M - 1, G >= 1 groups,
 * G | M, g(m) = m % G.  The chain is the hard forward's, exactly as in res_rows_fwd: r_1 = x, k_s the arg-min of the score of r_s
 * against C_s (the lowest index on a tie), r_{s+1} = r_s - C_s[k_s] in fp32.
 *   p_s[m][k]      = softmax_k(-sigma |r_s[m] - C_s[k]|^2), formed as e * (1 / sum) with the row minimum subtracted, as rate_fwd
 *   hist[s][g][k]  = sum over m with g(m) = g of p_s[m][k]
 *   q              = hist / (M / G)
 *   bits[s]        = - sum_g sum_k hist[s][g][k] log2 q[s][g][k], terms with hist <= 0 dropped
 *   rates[s]       = bits[s] / denom;  rate = rates[0] + .. + rates[n_stages - 1]: the fp32 sum of the fp32 values, stage order
 *   dhist[s][g][k] = scale (-(log2 q + 1 / ln 2)) / denom where hist > 0, else exactly 0
 *   res_rate_fwd   one launch, one thread per vector with the residual in registers and the stage loop inside the thread, sums
 *                  p_s (recomputed from r_s; [M][L] is never stored, x is read once) into one fp32 partial [n_stages][G][L] per
 *                  block; a second launch of one block merges the partials in block order in fp64, forms q, bits, rates and dhist
 *                  in fp64 and writes fp32.  rate [1] and rates [n_stages] are always written; hist and dhist may be NULL.  y and
 *                  index: both or neither; given, they are res_rows_fwd's results bit for bit.  Order of the fp32 sums: rate_fwd's
 *                  two paths -- G a power of two <= 64 whose per-wave tables [n_stages][G][L + 1] fit LDS (4, 2 or 1 waves per block
 *                  within 48 KiB, else one wave within 144 KiB): xor-shuffles over the lanes of a group, offsets 32, 16, .. G, the
 *                  waves of a block merged in wave order; any other case: m ascending inside a tile of 256, tiles in order.
 *   res_bwd_grouped   res_bwd with dp_s[m][k] = <a_s[m], C_s[k]> + dhist[s][g(m)][k]; everything after dp as res_bwd.  dhist NULL:
 *                  exactly res_bwd's launch; dhist all zero: res_bwd's bits.
 * For S = 1 both calls give rate_fwd's and quantize_bwd_grouped's quantities.  No atomics; grid, tile, path and every order of
 * summation depend on (M, D, L, G, n_stages) alone: two calls give identical bits.  ws of res_rate_fwd:
 * jpdse_vq_res_rate_workspace_size(M, D, L, G, n_stages) bytes, at most 16 MiB (host only; 0 outside the limits); of
 * res_bwd_grouped: res_bwd's.  JPDSE_EINVAL before any launch, outputs untouched: res_bwd's limits (n_stages 1 .. S), G < 1,
 * M % G != 0, G * L > 65536, n_stages * G * L > 65536, sigma not finite or <= 0, scale or denom not finite, denom <= 0, NULL x,
 * books, rate or rates, one of y and index without the other, a workspace missing or too small. */
size_t jpdse_vq_res_rate_workspace_size(int32_t M, int32_t D, int32_t L, int32_t G, int32_t n_stages);
typedef struct jpdse_vq_res_rate_fwd_args {
  int32_t dtype, M, D, L, S, n_stages, G;
  float sigma, scale, denom;
  const void* x;           /* [M][D] in `dtype` */
  const float* books;      /* [S][L][D] */
  float* rate;             /* [1] */
  float* rates;            /* [n_stages] */
  float* hist;             /* [n_stages][G][L], or NULL */
  float* dhist;            /* [n_stages][G][L], or NULL */
  void* y;                 /* [M][D] in `dtype`, or NULL */
  int32_t* index;          /* [n_stages][M], or NULL */
  void* ws;
  size_t ws_bytes;
  void* stream;
} jpdse_vq_res_rate_fwd_args;
int jpdse_vq_res_rate_fwd(const jpdse_vq_res_rate_fwd_args* args);
typedef struct jpdse_vq_res_bwd_grouped_args {
  jpdse_vq_res_bwd_args bwd;
  int32_t G;
  const float* dhist;      /* [n_stages][G][L], or NULL */
} jpdse_vq_res_bwd_grouped_args;
int jpdse_vq_res_bwd_grouped(const jpdse_vq_res_bwd_grouped_args* args);

/* ---- residual vector quantizer: a stage depth per cell (vq_residual.hip) ------------------------------------------
 * x [M][D], books [S][L][D] and n = n_stages <= S stages in use as above; G >= 1 vectors per cell, G | M: the cell of vector m is
 * m / G (one NHWC pixel of the feature map holds G consecutive vectors).  depth: int32 [M / G], values in 1 .. S; a value outside
 * is clamped to 1 .. S on the device.  n_m = min(n, depth[m / G]).
 *   res_rows_fwd_depth   row m is quantized exactly as res_rows_fwd with n_stages = n_m quantizes it: the same score, strict <,
 *                        r - c, a = c / a += c in stage order, rounded once.  index [n][M]: index[s][m] = -1 for s >= n_m.
 *   res_decode_depth     y[m] = the sum of the first n_m centres of row m, bit for bit the forward's y; index[s][m] for s >= n_m is
 *                        never read; an index outside [0, L) inside the depth reads as centre 0 and sets *status to 1.
 *   res_bwd_depth        res_bwd's recursion per row with h_{n_m + 1} = 0: dx[m] is res_bwd's at n_stages = n_m bit for bit;
 *                        dbooks[s] sums over the rows with n_m > s only, a row outside a stage adds exactly nothing to it (a stage
 *                        without a row gets zeros).  The same workspace and block-order merge as res_bwd; no atomics.
 *   depth_map            depth[i][cy][cx] = the maximum over the step x step pixels of the cell of table[class of the pixel]; the
 *                        class of a pixel is its label when that is an integer in [0, n_classes) (the rule of code_cost's class
 *                        attribution), and any other pixel, NaN included, takes default_depth.  label fp32 [N][1][H][W], table
 *                        int32 [n_classes], depth int32 [N][H / step][W / step].  The values are stored as they are: the three
 *                        calls above clamp.
 * Grid, tile and path are functions of (M, D, L, n_stages) alone: two calls give identical bits, and with every depth >= n_stages
 * y, index, dx and dbooks are those of the calls without a depth, bit for bit.  JPDSE_EINVAL before any launch, outputs untouched:
 * the limits of the call without a depth, G < 1, M % G != 0, NULL depth, a workspace missing or too small; depth_map: N, H, W < 1,
 * step < 1 or not dividing H and W, N * H * W >= 2^31, n_classes outside 0 .. 65536, a NULL label, depth, or table with classes. */
typedef struct jpdse_vq_res_rows_fwd_depth_args {
  jpdse_vq_res_rows_fwd_args fwd;
  int32_t G;
  const int32_t* depth;    /* [M / G] */
} jpdse_vq_res_rows_fwd_depth_args;
int jpdse_vq_res_rows_fwd_depth(const jpdse_vq_res_rows_fwd_depth_args* args);
typedef struct jpdse_vq_res_decode_depth_args {
  jpdse_vq_res_decode_args dec;
  int32_t G;
  const int32_t* depth;    /* [M / G] */
} jpdse_vq_res_decode_depth_args;
int jpdse_vq_res_decode_depth(const jpdse_vq_res_decode_depth_args* args);
typedef struct jpdse_vq_res_bwd_depth_args {
  jpdse_vq_res_bwd_args bwd;
  int32_t G;
  const int32_t* depth;    /* [M / G] */
} jpdse_vq_res_bwd_depth_args;
int jpdse_vq_res_bwd_depth(const jpdse_vq_res_bwd_depth_args* args);
typedef struct jpdse_vq_depth_map_args {
  int32_t N, H, W, step, n_classes, default_depth;
  const float* label;      /* [N][1][H][W] */
  const int32_t* table;    /* [n_classes], or NULL with n_classes == 0 */
  int32_t* depth;          /* [N][H / step][W / step] */
  void* stream;
} jpdse_vq_depth_map_args;
int jpdse_vq_depth_map(const jpdse_vq_depth_map_args* args);

/* ---- optimizer ---------------------------------------------------------------------- */
/* torch.optim.Adam (model.py:275,279) over a table of tensors, one launch.  `table` is a
 * device array of jpdse_adam_entry; bias corrections are computed from `step` (1-based). */
typedef struct jpdse_adam_entry {
  float* p;       /* parameter (fp32 master) */
  const float* g; /* gradient */
  float* m;       /* exp_avg */
  float* v;       /* exp_avg_sq */
  int64_t n;      /* elements */
  int64_t block0; /* first 1024-element block of this tensor in the launch */
  void* cast_bf16; /* optional: bf16 copy of the UPDATED parameter, same element order (the forward
                    * GEMM panel of a conv whose panel is a plain cast of the KRSC master); NULL = none */
} jpdse_adam_entry;
int jpdse_adam_step(const jpdse_adam_entry* table, int32_t n_entries, int64_t total_blocks,
                    float lr, float beta1, float beta2, float eps, int32_t step, float grad_scale,
                    void* stream);

#ifdef __cplusplus
}
#endif
#endif /* JPDSE_H_ */
