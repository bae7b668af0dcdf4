/*
 * ir2rgb_hip.h -- C ABI of libir2rgb_hip.so (MI355X / gfx950).
 *
 * This is the drop-in boundary for the ir2rgb hot path: what the reference binds through
 * three pybind11 extension modules (correlation_cuda / resample2d_cuda / channelnorm_cuda)
 * and what its models/networks.py obtains from cuDNN, expressed as plain C entry points
 * that take raw device pointers, explicit sizes and a HIP stream.  No torch types cross it.
 *
 * Conventions
 *   - every pointer is a device pointer unless the name ends in `_host`;
 *   - tensors are dense, in the layout named in the comment of each function;
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream); all work is
 *     enqueued asynchronously on it, nothing synchronises the host;
 *   - return value: 0 on success, a positive hipError_t if a launch failed, or a negative
 *     IR2RGB_E* code for argument errors detected on the host.  Nothing throws.
 *   - "reference" paths are relative to /root/reference.
 */
#ifndef IR2RGB_HIP_H
#define IR2RGB_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IR2RGB_OK 0
#define IR2RGB_EINVAL (-1)  /* bad size / parameter combination            */
#define IR2RGB_ENOSUP (-2)  /* valid in the reference, not implemented here */
#define IR2RGB_EALIGN (-3)  /* pointer or pitch not aligned as required     */

/* element types of activation / weight buffers */
#define IR2RGB_F32 0
#define IR2RGB_BF16 1
#define IR2RGB_F16 2

/* library / build identification: "ir2rgb_hip <version> gfx950" */
const char *ir2rgb_version(void);

/* ------------------------------------------------------------------------------------------
 * FlowNet2 operators (fp32, NCHW)
 * ------------------------------------------------------------------------------------------ */

/* Output geometry of the cost volume.
 * Replaces the sizing arithmetic in
 *   models/flownet2_pytorch/networks/correlation_package/correlation_cuda.cc:25-42. */
int ir2rgb_correlation_out_shape(int C, int H, int W, int pad_size, int kernel_size, int max_displacement,
                                 int stride1, int stride2, int *outC, int *outH, int *outW);

/* Cost volume forward.  in1,in2 [N,C,H,W] -> out [N,outC,outH,outW]; out is fully written
 * (no pre-zeroing needed).  Unlike the reference no padded channels-last scratch copies
 * (rInput1/rInput2) are needed.
 * Replaces correlation_cuda.forward:
 *   correlation_package/correlation_cuda.cc:10-87 and
 *   correlation_package/correlation_cuda_kernel.cu:46-147, :336-427.
 * Status: operator API (the reference's fp32 NCHW boundary, BASELINE config 3: 65 us at [1,256,64,128] = 0.48 TB/s, fp32 VALU
 * bound).  The FlowNet2 pipeline of this package does not call it: FlowNetC's cost volume is taken from the half NHWC conv3
 * outputs by ir2rgb_correlation_nhwc_half below (18.6 us); both are parity-tested against the same oracle. */
int ir2rgb_correlation_fwd(const float *in1, const float *in2, float *out, int N, int C, int H, int W,
                           int pad_size, int kernel_size, int max_displacement, int stride1, int stride2,
                           void *stream);

/* Cost volume backward.  gout [N,outC,outH,outW] -> gin1, gin2 [N,C,H,W] (fully written).
 * stride1 must be 1 (the reference's launch geometry writes out of bounds otherwise).
 * Replaces correlation_cuda.backward:
 *   correlation_package/correlation_cuda.cc:89-167 and
 *   correlation_package/correlation_cuda_kernel.cu:150-334, :430-564. */
int ir2rgb_correlation_bwd(const float *in1, const float *in2, const float *gout, float *gin1, float *gin2,
                           int N, int C, int H, int W, int pad_size, int kernel_size, int max_displacement,
                           int stride1, int stride2, void *stream);

/* The cost volume of FlowNetC as it sits in the FlowNet2 pipeline (reference FlowNetC.py:27, :101-103: Correlation(pad 20,
 * kernel 1, max displacement 20, stride1 1, stride2 2) followed by LeakyReLU(0.1) and the concatenation with conv_redir):
 * a, b = half-precision NHWC feature maps [N][H][W][lda / ldb], channels [offa, offa+C) / [offb, offb+C) -- the outputs of
 * conv3 as ir2rgb_conv2d_fwd leaves them.  out_mode 0: out = fp32 [N][441][H][W], the layout of ir2rgb_correlation_fwd;
 * out_mode 1: out = half NHWC [N][H][W][ldo], channels [offo, offo+441) = LeakyReLU_slope(correlation) (slope 1: none).
 * Products of half inputs are exact in fp32; the result differs from ir2rgb_correlation_fwd on the same (half-rounded)
 * inputs only by the order of the fp32 additions.  Banded MFMA products (correlation_mfma.hip).  C in {128, 256},
 * W <= 128, otherwise IR2RGB_ENOSUP (use ir2rgb_correlation_fwd). */
int ir2rgb_correlation_nhwc_half(const void *a, int lda, int offa, const void *b, int ldb, int offb, void *out,
                                 int out_mode, int ldo, int offo, float slope, int N, int C, int H, int W, int dtype,
                                 void *stream);

/* Flow warp forward.  img [N,C,H,W], flow [N,2,H,W] (pixels; channel 0 = dx, 1 = dy)
 * -> out [N,C,H,W].  kernel_size must be 1 (the only value the reference passes; larger
 * values make its kernel read out of bounds).
 * Replaces resample2d_cuda.forward:
 *   resample2d_package/resample2d_cuda.cc:6-13, resample2d_kernel.cu:15-64, :192-232. */
int ir2rgb_resample2d_fwd(const float *img, const float *flow, float *out, int N, int C, int H, int W,
                          int kernel_size, void *stream);

/* Flow warp backward.  gout [N,C,H,W] -> gimg [N,C,H,W] (zeroed here, then scattered with
 * float atomics), gflow [N,2,H,W].  Keeps the reference's truncation-vs-floor quirk.
 * Replaces resample2d_cuda.backward:
 *   resample2d_package/resample2d_cuda.cc:15-24, resample2d_kernel.cu:67-190, :234-310. */
int ir2rgb_resample2d_bwd(const float *img, const float *flow, const float *gout, float *gimg, float *gflow,
                          int N, int C, int H, int W, int kernel_size, void *stream);

/* Channel L2 norm forward.  in [N,C,H,W] -> out [N,1,H,W].  norm_deg is accepted and
 * ignored exactly as in the reference.
 * Replaces channelnorm_cuda.forward:
 *   channelnorm_package/channelnorm_cuda.cc:6-13, channelnorm_kernel.cu:18-60, :98-129. */
int ir2rgb_channelnorm_fwd(const float *in, float *out, int N, int C, int H, int W, int norm_deg, void *stream);

/* Channel L2 norm backward.  gin = gout * in / (out + 1e-9).
 * Replaces channelnorm_cuda.backward:
 *   channelnorm_package/channelnorm_cuda.cc:16-25, channelnorm_kernel.cu:63-96, :131-177. */
int ir2rgb_channelnorm_bwd(const float *in, const float *out, const float *gout, float *gin, int N, int C,
                           int H, int W, int norm_deg, void *stream);

/* Fused FlowNet2 step: warped = resample2d(img2, flow); diff = img1 - warped;
 * norm = channelnorm(diff).  Any of warped / diff / norm may be NULL to skip that output.
 * Fuses the three-launch sequence at models/flownet2_pytorch/models.py:109-111 (and
 * :121-123, :133-137, :146-150) and the confidence test of models/flownet.py:50,56-57
 * (conf = norm^2 < 0.02 is left to the caller). */
int ir2rgb_warp_diff_norm_fwd(const float *img1, const float *img2, const float *flow, float *warped,
                              float *diff, float *norm, int N, int C, int H, int W, void *stream);

/* ------------------------------------------------------------------------------------------
 * Generator / discriminator convolutions (half precision NHWC, fp32 accumulate, MFMA)
 *
 * These replace what reference models/networks.py gets from torch.nn.Conv2d /
 * ConvTranspose2d (+ ReflectionPad2d) -> cuDNN for the dense layers of
 * CompositeGeneratorModule (:141-171), CompositeLocalGeneratorModule (:253-271),
 * ResnetBlock (:556-580) and NLayerDiscriminator (:678-699).
 * ------------------------------------------------------------------------------------------ */
typedef struct ir2rgb_conv_desc {
    int N, Hin, Win, Cin;   /* input  [N,Hin,Win,Cin]  NHWC, Cin % 64 == 0 */
    int Hout, Wout, Cout;   /* output [N,Hout,Wout,Cout] NHWC              */
    int kh, kw, stride_h, stride_w, pad_h, pad_w;
    int pad_mode;           /* 0: zero padding, 1: reflection padding (nn.ReflectionPad2d), 2: ADJOINT of reflection
                             * padding: the call is the data gradient of a reflection-padded 3x3 / stride-1 / pad-1
                             * convolution (x = its output gradient, wpacked = its adjoint-packed weights, y = the
                             * input gradient, same H x W); only where ir2rgb_conv2d_kernel_name() says
                             * "conv3x3_patch_kernel", IR2RGB_ENOSUP otherwise (then: zero padding 2 on the padded
                             * grid + ir2rgb_fold_reflect) */
    int transposed;         /* 0: Conv2d, 1: ConvTranspose2d (stride 1 or 2 per axis; Hout/Wout carry output_padding) */
    int dtype;              /* IR2RGB_BF16 or IR2RGB_F16: activations and packed weights */
    int act;                /* fused after bias: 0 none, 1 LeakyReLU(0.2), 2 LeakyReLU(0.1), 3 ReLU */
    int out_f32;            /* 0: y is half NHWC, 1: y is fp32 NHWC (head convolutions) */
    /* channel-slice views (0 = dense): x holds ldx channels per pixel of which [ci_off, ci_off+Cin) are
     * read; y holds ldy channels per pixel of which [co_off, co_off+Cout) are written.  Lets producers
     * write straight into the concatenation buffers of the FlowNet2 decoders (torch.cat, FlowNetS.py etc.) */
    int ldx, ci_off, ldy, co_off;
    /* 1: the rows of the statistics buffer are cut per sample -- rows [n * R / N, (n + 1) * R / N) hold sample n only
     * (R = ir2rgb_conv2d_stats_rows) -- so that BatchNorm can treat groups of samples as separate forwards (the
     * discriminators' real / generated batches, reference discriminator.py:154-166, run as ONE convolution).  Costs
     * partly filled pixel tiles at every sample's end; not for transposed convolutions.  0: tiles run over the batch. */
    int stats_per_sample;
} ir2rgb_conv_desc;

/* Number of half elements of the packed weight buffer for this convolution (< 0: error). */
long ir2rgb_conv2d_packed_weight_elems(const ir2rgb_conv_desc *d);

/* Rows of the per-tile BatchNorm statistics buffer written by ir2rgb_conv2d_fwd:
 * stats_partial is [rows][2][Cout] fp32 (sum, sum of squares over the tile's pixels). */
int ir2rgb_conv2d_stats_rows(const ir2rgb_conv_desc *d);

/* Repack torch-layout fp32 weights (Conv2d [Cout,Cin,kh,kw]; ConvTranspose2d [Cin,Cout,kh,kw])
 * into the K-contiguous half-precision layout the MFMA kernel streams. */
int ir2rgb_conv2d_pack_weight(const ir2rgb_conv_desc *d, const float *w, void *wpacked, void *stream);

/* Packs the ADJOINT weights of a stride-1 Conv2d for its data-gradient convolution: `d` describes
 * the adjoint convolution (Cin = forward Cout, Cout = forward Cin) and w is the FORWARD weight
 * [d->Cin, d->Cout, kh, kw]; the channel swap and the tap reversal happen in the packing pass. */
int ir2rgb_conv2d_pack_weight_adjoint(const ir2rgb_conv_desc *d, const float *w, void *wpacked, void *stream);

/* Batched packing -- all packed copies of a network refreshed by ONE launch after an optimizer step
 * (the reference has no counterpart: cuDNN reads torch-layout weights, networks.py convolutions).
 * A job is the argument list of ir2rgb_conv2d_pack_weight[_adjoint].  _table_bytes returns the size
 * of the job table (negative IR2RGB_E* on error); _build writes it into HOST memory (16-byte
 * aligned) and returns the entry count (<= 4 per job, one per weight class; negative on error) and
 * the launch's block count; the caller copies the table to 16-byte aligned device memory once -- it
 * stays valid while the job pointers do -- and calls _run every time the weights changed.  All jobs
 * of a table share one dtype. */
typedef struct ir2rgb_pack_job {
    ir2rgb_conv_desc desc;
    const float *w;
    void *wpacked;
    int adjoint;
    int reserved;
} ir2rgb_pack_job;
long ir2rgb_conv2d_pack_batch_table_bytes(const ir2rgb_pack_job *jobs, int njobs);
int ir2rgb_conv2d_pack_batch_build(const ir2rgb_pack_job *jobs, int njobs, void *table_host, long table_bytes,
                                   int *nblocks);
int ir2rgb_conv2d_pack_batch_run(const void *table_dev, int nentries, int nblocks, int dtype, void *stream);

/* y = act(conv(x) + bias); bias and stats_partial may be NULL.  x, wpacked, y 16-byte aligned. */
int ir2rgb_conv2d_fwd(const ir2rgb_conv_desc *d, const void *x, const void *wpacked, const float *bias, void *y,
                      float *stats_partial, void *stream);

/* The same with a caller-owned workspace, which lets layers with too few output tiles for the chip split their input
 * channels over two workgroups per tile (the 1024 -> 1024 3x3 convolutions of ResnetBlock, networks.py:556-580, at
 * 32 x 64 and their data gradients: 128 tiles of 128 px x 128 cout for 256 CUs).  ir2rgb_conv2d_fwd_workspace_bytes:
 * 0 = this descriptor has no use for one (pass NULL), < 0 = error.  The workspace is 16-byte aligned, must be ZERO
 * when first used and is left ready for the next launch by every launch (tickets advance by a fixed amount per
 * launch; the partial sums need no initialisation); launches that share one must be ordered (same stream).
 * Results are bit-identical from launch to launch: two partial sums are added, in either order. */
long ir2rgb_conv2d_fwd_workspace_bytes(const ir2rgb_conv_desc *d);
int ir2rgb_conv2d_fwd_ws(const ir2rgb_conv_desc *d, const void *x, const void *wpacked, const float *bias, void *y,
                         float *stats_partial, void *workspace, long workspace_bytes, void *stream);

/* Name of the device kernel ir2rgb_conv2d_fwd launches for `d` ("conv3x3_patch_kernel",
 * "conv_igemm_kernel", "conv_igemm_classes_kernel"; "" for an invalid descriptor): for profiles. */
const char *ir2rgb_conv2d_kernel_name(const ir2rgb_conv_desc *d);

/* Training-mode BatchNorm2d statistics (reference norm_layer = nn.BatchNorm2d, networks.py:41-48).
 * Reduces the [rows][2][C] partial sums written by ir2rgb_conv2d_fwd over `count` pixels into
 * scale = gamma*invstd and shift = beta - mean*scale, and updates running_mean / running_var
 * in place (momentum form of torch: new = (1-m)*old + m*batch, unbiased variance).  gamma, beta,
 * running_*, mean_out, invstd_out may be NULL.  stat_updates >= 1: the momentum update is applied
 * that many times (a forward that stands for several identical forwards of the reference, e.g.
 * compute_loss_D evaluating netD on the same real frames twice per step, discriminator.py:154-166). */
int ir2rgb_bn_finalize(const float *stats_partial, int rows, int C, long count, const float *gamma,
                       const float *beta, float *running_mean, float *running_var, float momentum, float eps,
                       float *scale, float *shift, float *mean_out, float *invstd_out, int stat_updates,
                       void *stream);

/* The same with two more inputs.
 * conv_bias (may be NULL): the statistics are those of the convolution output WITHOUT its bias.  BatchNorm subtracts
 *   the batch mean, so the bias of the convolution in front of it (nn.Conv2d(..., bias=True) + norm_layer,
 *   networks.py:141-171) cancels exactly; leaving it out of the half-precision activations keeps a constant input
 *   (e.g. the all-zero previous frames of no_first_img, generator.py:219-220) exactly constant, as it is in fp32.
 *   Only the running mean sees it: running_mean follows mean + conv_bias, as nn.BatchNorm2d's does.
 * frozen != 0: module.eval() -- no batch statistics (stats_partial / rows / count unused), scale and shift come
 *   from running_mean / running_var (both required):  scale = gamma*rsqrt(running_var+eps),
 *   shift = beta - (running_mean - conv_bias)*scale; mean_out = running_mean - conv_bias; nothing is updated. */
int ir2rgb_bn_finalize_ex(const float *stats_partial, int rows, int C, long count, const float *gamma,
                          const float *beta, const float *conv_bias, float *running_mean, float *running_var,
                          float momentum, float eps, float *scale, float *shift, float *mean_out,
                          float *invstd_out, int stat_updates, int frozen, void *stream);

/* ir2rgb_bn_finalize_ex (training mode, frozen = 0) and ir2rgb_bn_apply in ONE launch, for convolutions that wrote at
 * most IR2RGB_BN_FUSED_MAX_ROWS partial rows (the residual blocks).  The same device functions (csrc/bn.h) on sums taken
 * in the same order: results are bit-identical to the two calls.  C % 64 == 0.  x / y / res1 / res2 as in ir2rgb_bn_apply (y may alias x). */
#define IR2RGB_BN_FUSED_MAX_ROWS 128
int ir2rgb_bn_finalize_apply(const float *stats_partial, int rows, int C, long count, const float *gamma,
                             const float *beta, const float *conv_bias, float *running_mean, float *running_var,
                             float momentum, float eps, float *scale, float *shift, float *mean_out,
                             float *invstd_out, int stat_updates, const void *x, const void *res1, const void *res2,
                             void *y, long npix, int act, int dtype, void *stream);

/* y = act(x*scale[c] + shift[c]) + res1 + res2 on NHWC half tensors of npix pixels x C channels
 * (C % 8 == 0).  act: 0 none, 1 ReLU, 2 LeakyReLU(0.2).  res1/res2 may be NULL; y may alias x.
 * Covers norm+activation (networks.py:141-171, :253-271, :678-699), the ResnetBlock skip
 * (:585) and the encoder sum (:192, :290-291). */
int ir2rgb_bn_apply(const void *x, const float *scale, const float *shift, const void *res1, const void *res2,
                    void *y, long npix, int C, int act, int dtype, void *stream);

/* Layout converters between the reference's NCHW fp32 tensors and NHWC half. */
int ir2rgb_nchw_f32_to_nhwc_half(const float *in, void *out, int N, int C, int H, int W, int dtype, void *stream);
int ir2rgb_nhwc_half_to_nchw_f32(const void *in, float *out, int N, int C, int H, int W, int dtype, void *stream);

/* x-direction im2col of a small-channel NCHW fp32 image into 64-channel NHWC half:
 *   out[n][y][ox][ci*KW + kx] = in[n][ci][y][pad(ox*stride_w + kx - pad_w)],  Cin*KW <= 64.
 * Turns the first layers (ReflectionPad2d(3)+Conv7x7 on 9/6 channels, networks.py:141,:150,
 * :253-255; Conv4x4 s2 p2 on 6/13 channels, :680) into KH x 1 convolutions for the MFMA kernel. */
int ir2rgb_xexpand(const float *in, void *out, int N, int Cin, int H, int W, int Wout, int KW, int stride_w,
                   int pad_w, int pad_mode, int dtype, void *stream);
/* Same with Cx = 64 or 128 output channels (Cin*KW <= Cx): the 12-channel 7x7 first layer of FlowNetS. */
int ir2rgb_xexpand_cx(const float *in, void *out, int N, int Cin, int H, int W, int Wout, int KW, int stride_w,
                      int pad_w, int pad_mode, int Cx, int dtype, void *stream);

/* NCHW fp32 [N,C,H,W] -> channels [c_off, c_off+C) of an NHWC half buffer with ld channels per pixel,
 * with an optional fused activation (0 none, 2 LeakyReLU(0.1): corr_activation, FlowNetC.py:32). */
int ir2rgb_nchw_f32_to_nhwc_half_slice(const float *in, void *out, int N, int C, int H, int W, int ld, int c_off,
                                       int act, int dtype, void *stream);

/* Finish of a separable head: T [N,H,W,CT] fp32 holds, in channel co*KH+ky, the horizontal
 * part of a KHxKW convolution; out[n][co][y][x] = f(sum_ky T[n][refl(y+ky-pad)][x][co*KH+ky] + bias[co]).
 * acts packs one nibble per output channel: 0 -> linear * mul, 1 -> tanh, 2 -> sigmoid.
 * (ReflectionPad2d(3)+Conv7x7 heads with tanh / *20 / sigmoid, networks.py:166,:170-171,:200-201) */
int ir2rgb_head_finish(const float *T, const float *bias, float *out, int N, int H, int W, int Cout, int KH,
                       int CT, int pad_h, unsigned acts, float mul, void *stream);

/* Temporal blend of the generator (networks.py:89-100, :207-209):
 *   warp = grid_sample(prev, grid + flow_normalised, bilinear, border)   [align_corners quirk kept]
 *   out  = raw * w + warp * (1 - w)
 * raw [N,3,H,W], prev [N,Cp,H,W] (its LAST 3 channels are warped), flow [N,2,H,W], w [N,1,H,W]. */
int ir2rgb_warp_blend_fwd(const float *raw, const float *prev, const float *flow, const float *w, float *out,
                          float *warp_out, int N, int Cp, int H, int W, void *stream);

/* ------------------------------------------------------------------------------------------
 * Backward companions (HBM-bound).  The data gradient of every convolution is itself an
 * ir2rgb_conv2d_fwd call (transposed <-> strided, flipped weights); these cover the rest of
 * what torch.autograd + cuDNN do for the reference's loss.backward() (train_vid2vid.py:166-169).
 * ------------------------------------------------------------------------------------------ */

/* Rows R of the scratch needed by ir2rgb_bn_bwd: `partial` must hold (R*2 + 3)*C floats
 * ([R][2][C] pixel-range partial sums; the tail of 3*C floats is reserved: nothing is written there).
 * < 0: error; C must be a power of two in [64, 2048]. */
int ir2rgb_bn_bwd_blocks(long npix, int C);

/* Backward of activation + training-mode BatchNorm2d on NHWC half tensors:
 *   g' = gz * act'(y*scale+shift);  dbeta = sum g';  dgamma = sum g'*yhat;
 *   gy = scale * (g' - dbeta/n - yhat*dgamma/n),  yhat = (y-mean)*invstd.
 * scale, shift, mean and invstd are given together or not at all (anything else: IR2RGB_EINVAL).  With all four
 * NULL (no norm layer): gy = gz * act'(y) and dbeta = sum gy (the bias gradient).
 * act: 0 none, 1 ReLU, 2 LeakyReLU(0.2), or-ed with
 *   IR2RGB_BN_BWD_FROZEN: the statistics were frozen (evaluation-mode BatchNorm, ir2rgb_bn_finalize_ex(frozen)):
 *     gy = scale * g', dgamma / dbeta as above;
 *   IR2RGB_BN_BWD_ACCUMULATE: dgamma / dbeta are ADDED to what the two vectors hold (the later sample groups of a layer
 *     whose batch is several independent forwards).
 * gy may alias gz. */
#define IR2RGB_BN_BWD_FROZEN 16
#define IR2RGB_BN_BWD_ACCUMULATE 32
int ir2rgb_bn_bwd(const void *gz, const void *y, const float *scale, const float *shift, const float *mean,
                  const float *invstd, void *gy, float *dgamma, float *dbeta, float *partial, long npix, int C,
                  int act, int dtype, void *stream);

/* dst[i] = idx[i] >= 0 ? src[idx[i]] : 0 (fp32; n elements): rearranged copies of a weight tensor (x-im2col layout of
 * the first layers, zero-padded widths) from a precomputed index map, refreshed after every optimizer step. */
int ir2rgb_gather_f32(const float *src, const int *idx, float *dst, long n, void *stream);

/* AvgPool2d(3, stride 2, padding 1, count_include_pad=False) on fp32 planes: the image pyramids of the multi-scale
 * discriminators (reference networks.py:639, :658-666) and of the generator inputs (base_model.py:64-82).
 * backward 0: x [planes][H][W] -> y [planes][Ho][Wo], Ho = (H-1)/2 + 1;  backward 1: x = the gradient
 * [planes][Ho][Wo] -> y = the input gradient [planes][H][W]. */
int ir2rgb_avgpool3s2(const float *x, float *y, long planes, int H, int W, int backward, void *stream);

/* Gradient of a thin fp32 convolution output (the 1-channel PatchGAN logits, NLayerDiscriminator's last
 * layer, networks.py:676-677) prepared for the MFMA kernels: gz [N,Cout,H,W] fp32, Cout <= 8 ->
 * g64 [N,H,W,64] and g8 [N,H,W,8] NHWC half (channels >= Cout zero; data- / weight-gradient operands) and
 * dbias[Cout] = sum over N,H,W of gz (deterministic). */
int ir2rgb_thin_grad_expand(const float *gz, void *g64, void *g8, float *dbias, int N, int Cout, int H, int W,
                            int dtype, void *stream);

/* Adjoint of nn.ReflectionPad2d: dxpad [N,H+2*pad_h,W+2*pad_w,C] -> dx [N,H,W,C] (NHWC half). */
int ir2rgb_fold_reflect(const void *dxpad, void *dx, int N, int H, int W, int C, int pad_h, int pad_w, int dtype,
                        void *stream);

/* Backward of ir2rgb_head_finish: gout/out [N,Cout,H,W] fp32 (out = the forward result) ->
 * dT [N,H,W,CT] half (gradient w.r.t. the separable row responses, channels >= Cout*KH zeroed)
 * and dbias [Cout] fp32. */
int ir2rgb_head_finish_bwd(const float *gout, const float *out, void *dT, float *dbias, float *partial, int N, int H, int W,
                           int Cout, int KH, int CT, int pad_h, unsigned acts, float mul, int dtype, void *stream);
/* Rows of 8 floats `partial` must hold for ir2rgb_head_finish_bwd (one per workgroup: the bias gradient is summed in a
 * fixed order by a second, one-workgroup kernel -- no float atomics, bit-reproducible). */
int ir2rgb_head_finish_bwd_rows(int N, int H, int W);

/* Backward of ir2rgb_warp_blend_fwd w.r.t. raw, flow and w (prev is a detached input on the
 * training path, reference generator.py:153-154). */
int ir2rgb_warp_blend_bwd(const float *gout, const float *raw, const float *prev, const float *flow, const float *w,
                          float *graw, float *gflow, float *gw, int N, int Cp, int H, int W, void *stream);

/* Adjoint of ir2rgb_xexpand: dxe [N,H,Wout,64] half -> din [N,Cin,H,W] fp32. */
int ir2rgb_xexpand_bwd(const void *dxe, float *din, int N, int Cin, int H, int W, int Wout, int KW, int stride_w,
                       int pad_w, int pad_mode, int dtype, void *stream);

/* Weight gradient of a convolution described by `d` (same descriptor as the forward call) on the
 * matrix cores: x is the forward input [N,Hin,Win,Cin], gy the gradient w.r.t. the forward output
 * [N,Hout,Wout,Cout] (both NHWC half, channels % 8 == 0); dw receives the gradient in the torch
 * weight layout, fp32 ([Cout,Cin,kh,kw], or [Cin,Cout,kh,kw] when d->transposed).  `workspace`
 * holds ir2rgb_conv2d_wgrad_workspace_elems(d) floats.  Reflection padding is honoured by the
 * gather (no padded copy).  Replaces cuDNN's backward-filter in the reference's loss.backward(). */
long ir2rgb_conv2d_wgrad_workspace_elems(const ir2rgb_conv_desc *d);
int ir2rgb_conv2d_wgrad(const ir2rgb_conv_desc *d, const void *x, const void *gy, float *dw, float *workspace,
                        void *stream);

/* dw += the same weight gradient (a parameter that is used several times in one backward pass: the discriminators are
 * applied to two or three inputs per window, discriminator.py:154-166): the sum with the earlier contributions happens in
 * the kernel's own finish pass instead of in a separate add.  Workspace: ir2rgb_conv2d_wgrad_acc_workspace_elems. */
int ir2rgb_conv2d_wgrad_acc(const ir2rgb_conv_desc *d, const void *x, const void *gy, float *dw, float *workspace,
                            void *stream);
long ir2rgb_conv2d_wgrad_acc_workspace_elems(const ir2rgb_conv_desc *d);

/* FlowNet2 flow up-sampler ConvTranspose2d(2,2,4,2,1) (reference FlowNetC.py:47-50 etc.): in [N,2,h,w]
 * fp32 NCHW, weight [2,2,4,4], bias [2] or NULL -> channels [c_off, c_off+2) of an NHWC half buffer
 * [N,2h,2w,ld]. */
int ir2rgb_flow_upsample_slice(const float *in, const float *weight, const float *bias, void *out, int N, int h,
                               int w, int ld, int c_off, int dtype, void *stream);

/* ------------------------------------------------------------------------------------------
 * Scalar losses of the loop body, a group of terms per launch.  Replaces the chains of torch
 * elementwise + reduction kernels behind criterionFeat (nn.L1Loss on discriminator features,
 * reference discriminator.py:199-210), criterionGAN (least-squares GANLoss, models/networks.py
 * GANLoss / loss.py) and the confidence-masked L1 terms (criterionFlow, loss.py MaskedL1Loss).
 *   kind 0: weight * mean |a - b|          a, b half tensors of identical dense layout, n % 8 == 0
 *   kind 1: weight * mean (a - target)^2   a fp32
 *   kind 2: weight * mean |a*m - b*m|      a, b fp32 NCHW [N,C,H,W] (b NULL = zeros), mask fp32
 *                                          [N,1,H,W]; hw = H*W, chw = C*H*W
 * Every term adds into out[slot] (slot 0..3).  The sums are deterministic (per-block partials added
 * in block order).  ga, when not NULL, receives d out[slot] / d a scaled by gout[slot] (same dtype
 * and layout as a).
 * ------------------------------------------------------------------------------------------ */
#define IR2RGB_LOSS_MAX_ITEMS 32
typedef struct ir2rgb_loss_item {
    const void *a;
    const void *b;
    void *ga;
    const void *mask;
    long n;
    long hw;
    long chw;
    float weight;
    float target;
    int kind;
    int slot;
} ir2rgb_loss_item;

/* Floats of `partial` scratch that ir2rgb_loss_multi_fwd needs. */
int ir2rgb_loss_partial_elems(void);
/* out[0 .. max slot] = the summed terms: every slot up to the largest one named is written, and one of them that no
 * term names receives 0; slots above the largest named one are not written. */
int ir2rgb_loss_multi_fwd(const ir2rgb_loss_item *items, int count, int dtype, float *partial, float *out,
                          void *stream);
/* Writes items[i].ga for every item that has one; gout = gradient w.r.t. out (device, fp32). */
int ir2rgb_loss_multi_bwd(const ir2rgb_loss_item *items, int count, int dtype, const float *gout, void *stream);

/* ------------------------------------------------------------------------------------------
 * torch.optim.Adam step (weight_decay 0, amsgrad off) of one optimizer in one launch; replaces the
 * per-tensor torch kernels behind optimizer_G/D/D_T.step() (reference train_vid2vid.py:93-105).
 *   table  : device array of { float *p; const float *g; float *m; float *v; long n; } (40 bytes each)
 *   blocks : device array of int pairs (tensor index, chunk index): one workgroup updates elements
 *            [chunk*E, min(n, (chunk+1)*E)) of its tensor, E = ir2rgb_adam_chunk_elems(); the caller
 *            lists every chunk of every tensor exactly once
 *   step   : 1-based step count (bias corrections 1 - beta^step are evaluated on the host in double)
 * ------------------------------------------------------------------------------------------ */
int ir2rgb_adam_chunk_elems(void);
int ir2rgb_adam_step(const void *table, const void *blocks, int nblocks, float lr, float beta1, float beta2, float eps,
                     int step, void *stream);

/* ------------------------------------------------------------------------------------------
 * Checked optimizer steps, decided on the device (adam.hip; the scale's update: loss_scale.hip).  f16 training
 * multiplies its losses by `scale` before backward() (dynamic loss scaling); any compute dtype may guard its steps.  Per
 * optimizer and window the step (1) reads the stored gradient once: finite? sum of squares, (2) applies the rule below,
 * (3) takes the Adam step on g * factor or -- after an inf or a NaN -- leaves p, m, v and the step count alone bit for
 * bit; once per window (4) the scale moves by torch._amp_update_scale_'s rule.  The host never reads the decision: the
 * step count, the coefficients of the step being taken, the factor and the scale live in device blocks, laid out as the
 * structs below (plain C layout; the *_state_bytes queries answer their sizes, so that a caller need not repeat them).
 * With g the stored gradient (of the scaled loss when scaler_state is given) and inv = scaler_state's inv_scale, or
 * exactly 1 when scaler_state is NULL, all in double:
 *     norm = sqrt(sum g^2) * inv,  c = min(1, max_norm / (norm + 1e-6)),  factor = (float)(inv * c)
 * and the step is ir2rgb_adam_step on fl(g * factor), one rounded product per element.  This is
 * torch.nn.utils.clip_grad_norm_ applied after the unscaling, except that torch evaluates c in fp32.  max_norm +inf
 * never clips: c is exactly 1 and factor is inv_scale, or 1.0 without a scaler.  c < 1 counts as clipped.
 *   table, blocks, nblocks : as for ir2rgb_adam_step
 *   partial     : device scratch of ir2rgb_grad_check_partial_bytes(nblocks) bytes, 8-byte aligned: one
 *                 { double sumsq; float nonfinite; float reserved; } row per workgroup, summed in row order
 *   opt_state   : ir2rgb_adam_state, 8-byte aligned, one per optimizer.  ir2rgb_loss_scale_update, ir2rgb_ema_step and
 *                 ir2rgb_loss_log_push read the skip decision (found_inf) from it
 *   guard_state : ir2rgb_grad_guard_state, 4-byte aligned, zeroed by the caller, one per optimizer, or NULL (no figures
 *                 and counters are kept).  After a non-finite gradient grad_norm is that gradient's (inf or NaN),
 *                 clip_coef and factor are 0, `skipped` is incremented and `steps` is not
 *   scaler_state : ir2rgb_loss_scale_state, 4-byte aligned, one per trainer, or NULL (inv is 1)
 * All three blocks are written by the kernels only.
 * IR2RGB_EINVAL: NULL table / blocks / partial / opt_state, NULL scaler_state / opt_states of the update,
 * nblocks < 0, a beta outside [0, 1), max_norm <= 0 or NaN, count outside [0, 8], growth_interval < 0, growth < 1,
 * backoff outside (0, 1]; IR2RGB_EALIGN: partial / opt_state / opt_states off an 8-byte boundary, guard_state /
 * scaler_state off a 4-byte one.  Both before any launch.
 * ------------------------------------------------------------------------------------------ */
typedef struct ir2rgb_adam_state {
    int step;            /* successful (not skipped) steps so far */
    float step_size, beta1, beta2, omb1, omb2, bc2_sqrt, eps;   /* coefficients of the step being taken (AdamCoef) */
    float found_inf;     /* 1 when the last checked gradient held an inf or a NaN, else 0 */
    float factor;        /* what the step multiplies every stored gradient element by: (float)(inv * c); 0 after found_inf */
    double grad_sumsq;   /* sum of squares of the last checked gradient, unscaled (x inv_scale^2) */
} ir2rgb_adam_state;

typedef struct ir2rgb_loss_scale_state {
    float scale, inv_scale;   /* inv_scale = (float)(1.0 / (double)scale) */
    int growth_tracker;       /* consecutive unskipped windows since the last change of the scale */
    int skipped;              /* windows skipped so far (for logging) */
} ir2rgb_loss_scale_state;

typedef struct ir2rgb_grad_guard_state {
    float grad_norm;     /* unscaled global L2 norm of the last checked gradient */
    float clip_coef;     /* c of the last check (1 when nothing was clipped, 0 after a skipped step) */
    float factor;        /* opt_state's factor of the last check */
    int steps;           /* steps taken under this guard */
    int clipped;         /* of those, steps with c < 1 */
    int skipped;         /* steps skipped because the gradient held an inf or a NaN */
    int reserved[2];
} ir2rgb_grad_guard_state;

/* Size in bytes of ir2rgb_adam_state (which 0) or ir2rgb_loss_scale_state (which 1); IR2RGB_EINVAL otherwise. */
long ir2rgb_loss_scale_state_bytes(int which);
long ir2rgb_grad_guard_state_bytes(void);
long ir2rgb_grad_check_partial_bytes(int nblocks);
/* Two launches.  Every workgroup of the first reads its chunk of g only (16-byte loads where adam_kernel takes them) and
 * writes its partial row: finiteness decided per element from the value, squares accumulated in double in a fixed
 * order, no atomics.  The second (one workgroup) sums the rows and writes found_inf, grad_sumsq = sumsq * inv^2 and
 * factor, and guard_state when it is given; if the gradient is finite it advances `step` and evaluates that step's
 * coefficients in double from lr, beta1, beta2, eps -- the expressions of ir2rgb_adam_step's host code.
 * nblocks 0: the second launch alone (a finite, empty gradient). */
int ir2rgb_grad_check(const void *table, const void *blocks, int nblocks, void *partial, void *opt_state,
                      void *guard_state, const void *scaler_state, float max_norm, float lr, float beta1, float beta2,
                      float eps, void *stream);
/* ir2rgb_adam_step on g * factor with the coefficients ir2rgb_grad_check left in opt_state; touches nothing when
 * opt_state's found_inf is set.  nblocks 0: IR2RGB_OK, nothing is launched. */
int ir2rgb_adam_step_checked(const void *table, const void *blocks, int nblocks, const void *opt_state, void *stream);
/* opt_states: device array of `count` (<= 8) addresses of the ir2rgb_adam_state blocks stepped this window.  Any
 * found_inf: scale *= backoff, tracker 0, skipped += 1.  Otherwise the tracker is incremented and, when it reaches
 * growth_interval, reset, with scale *= growth unless that product is not finite.  growth_interval 0: a static
 * scale -- the scale and the tracker never change, skipped still counts. */
int ir2rgb_loss_scale_update(void *scaler_state, const void *opt_states, int count, float growth, float backoff,
                             int growth_interval, void *stream);

/* ------------------------------------------------------------------------------------------
 * Exponential moving average of the generator's parameters (ema.hip): e <- e + alpha * (p - e) for every tensor
 * of a table, one streaming launch per window after the generator's optimizer step.  The three operations are
 * rounded one by one in fp32 (no fused multiply-add), so p == e leaves e unchanged bit for bit; inf and NaN
 * propagate as IEEE has them.
 *   table  : device array of { const float *p; float *e; long n; } (24 bytes each); p is only read
 *   blocks : device array of int pairs (tensor index, chunk index), as for ir2rgb_adam_step, with the same
 *            chunk size ir2rgb_adam_chunk_elems()
 *   ema_state : ir2rgb_ema_state, 4-byte aligned, zeroed (or seeded) by the caller, written by the kernels only
 *   opt_state : the generator optimizer's ir2rgb_adam_state (8-byte aligned) or NULL.  When it is given and its
 *            found_inf is set, the window's step was skipped: e and `updates` stay as they are and `skipped` is
 *            incremented.  NULL: every call updates.  The host never reads the decision.
 *   beta, warmup : for the n-th update taken (n = `updates` after its increment) the decay is
 *            beta_n = min(beta, (1 + n) / (10 + n)) while warmup != 0 and n < 2^20, else beta -- the quotient one
 *            correctly rounded fp32 division of the two integers -- and alpha = 1 - beta_n, one rounded fp32
 *            subtraction, evaluated on the device.
 * IR2RGB_EINVAL: NULL table / blocks / ema_state, nblocks < 0, beta outside [0, 1); IR2RGB_EALIGN: ema_state off
 * a 4-byte boundary, opt_state off an 8-byte one.  Both before any launch.  nblocks 0: IR2RGB_OK, nothing is
 * launched and the state is not touched.
 * ------------------------------------------------------------------------------------------ */
typedef struct ir2rgb_ema_state {
    int updates;         /* averages taken so far */
    int skipped;         /* windows left out because the optimizer's step was skipped */
    float alpha;         /* 1 - beta_n of the last update taken */
    int reserved;
} ir2rgb_ema_state;

long ir2rgb_ema_state_bytes(void);
int ir2rgb_ema_step(const void *table, const void *blocks, int nblocks, void *ema_state, const void *opt_state,
                    float beta, int warmup, void *stream);

/* ------------------------------------------------------------------------------------------
 * Device loss log (loss_log.hip): one launch per training window records the window's loss scalars without a host
 * round trip.  ring is fp32 [capacity][IR2RGB_LOSS_LOG_SLOTS]; state is an ir2rgb_loss_log_state, 8-byte aligned,
 * zeroed by the caller before the first push.  Both are written by the kernel only.
 *   srcs    : HOST array of `count` device addresses, each one fp32 value (4-byte aligned); they are copied into the
 *             kernel's argument block, so the array is free again when the call returns
 *   present : bit i set = slot i has a value this window; an entry of srcs whose bit is clear is not looked at
 *   opt_states, n_opts : HOST array of the ir2rgb_adam_state addresses of the optimizers stepped this window with a
 *             loss scaler (n_opts 0: no scaler).  If any of them holds found_inf the window was skipped
 * The kernel writes row `state->count % capacity`: the value of every present slot, IR2RGB_LOSS_LOG_ABSENT in the
 * others (a finite number no loss takes, so the ring holds a NaN only where a loss was one).  Unless the window was
 * skipped, each present value is added to sum[slot] in double and n[slot] is incremented; a skipped window increments
 * `skipped` instead.  `count` is incremented.  Values are passed through as they are, inf and NaN included.
 * IR2RGB_EINVAL: NULL srcs / ring / state, count outside [0, 32], a bit of `present` at or above `count`, a NULL
 * source whose bit is set, capacity <= 0, n_opts outside [0, 8], a NULL optimizer state; IR2RGB_EALIGN: a source or
 * ring off a 4-byte boundary, state or an optimizer state off an 8-byte one.  Both before any launch.
 * ------------------------------------------------------------------------------------------ */
#define IR2RGB_LOSS_LOG_SLOTS 32
#define IR2RGB_LOSS_LOG_OPTIMIZERS 8
#define IR2RGB_LOSS_LOG_ABSENT (-3.402823466e+38f) /* -FLT_MAX */

typedef struct ir2rgb_loss_log_state {
    double sum[IR2RGB_LOSS_LOG_SLOTS];  /* per slot: sum of the values pushed since the caller last zeroed it */
    long long n[IR2RGB_LOSS_LOG_SLOTS]; /* per slot: how many values that sum holds */
    long long skipped;                  /* windows left out of the sums because their optimizer steps were skipped */
    long long count;                    /* windows pushed so far; the caller's reset leaves it alone (ring position) */
} ir2rgb_loss_log_state;

int ir2rgb_loss_log_push(const void *const *srcs, unsigned present, int count, float *ring, int capacity, void *state,
                         const void *const *opt_states, int n_opts, void *stream);

/* ------------------------------------------------------------------------------------------
 * Frame I/O of frame-by-frame inference (frame_io.hip): the 8-bit image boundary and the recurrence state
 * as device-resident histories.  A history is fp32 [T][C][H][W], oldest frame first; both entry points move
 * slots 1..T-1 down to 0..T-2 in place (same element index, same thread) and fill slot T-1.  Rows whose
 * width is a multiple of 4 with 16-byte aligned bases take 16-byte accesses, everything else the scalar
 * form; float pointers that are not 4-byte aligned are IR2RGB_EALIGN.  No buffer may alias another.
 * ------------------------------------------------------------------------------------------ */

/* One new input frame.  frame: uint8 [H][W][C] interleaved (src_f32 0) or an already normalised fp32
 * [C][H][W] frame (src_f32 1); C in {1, 3}.  hist0 [T][C][H][W] receives (float(v) / 255 - 0.5) / 0.5 with
 * correctly rounded divisions, i.e. transforms.ToTensor + Normalize(0.5, 0.5) (reference
 * data/transform.py:82-85).  hist1, when not NULL, is the half-resolution history
 * [T][C][(H-1)/2+1][(W-1)/2+1] and receives AvgPool2d(3, 2, 1, count_include_pad=False) of the new frame
 * (base_model.py:64-82), bit-identical to ir2rgb_avgpool3s2 of the new hist0 slot.  Coarser levels: call
 * ir2rgb_avgpool3s2 on the newest slot of the level above. */
int ir2rgb_frame_push_u8(const void *frame, float *hist0, float *hist1, int T, int C, int H, int W, int src_f32,
                         void *stream);

/* One generated frame.  x: fp32 [3][H][W] (the output of ir2rgb_warp_blend_fwd or ir2rgb_head_finish) ->
 * the newest slot of hist [T][3][H][W] (torch.cat([prev[1:], fake_B]), generator.py:214) and, when img_u8 is
 * not NULL, the uint8 [H][W][3] image trunc(clip((x + 1) / 2 * 255, 0, 255)) in fp32 in that order
 * (util.tensor2im, util/util.py:45-67). */
int ir2rgb_frame_finish_u8(const float *x, float *hist, uint8_t *img_u8, int T, int H, int W, void *stream);

/* ------------------------------------------------------------------------------------------
 * Video scores (video_metrics.hip): the reference's scripts/ssim_metric.py per frame, in fp64 on the device.
 * orig, pred: uint8 [N][H][W][3], N in [1, 65535], H, W >= 7, 3*H*W < 2^31.  For every frame n
 *   gray  = (r/255)*0.2125 + (g/255)*0.7154 + (b/255)*0.0721              skimage.color.rgb2gray
 *   R     = max(gray(orig)) - min(gray(pred))                              the script's dynamic_range, or
 *           range[n] when `range` (device, N doubles) is not NULL
 *   l2    = sqrt(sum (gray(orig) - gray(pred))^2)                          np.linalg.norm in mse_single_frame
 *   ssim  = mean over the (H-6)*(W-6) windows inside the image of
 *           ((2 ux uy + C1)(2 vxy + C2)) / ((ux^2 + uy^2 + C1)(vx + vy + C2)),  C1 = (0.01 R)^2, C2 = (0.03 R)^2,
 *           window 7x7, uniform weights, sample covariance (49/48): skimage's compare_ssim defaults
 * and out[n] = {ssim, l2, R}.  No special cases (an all-black pair gives NaN, as in NumPy).  R never passes
 * through the host.  All sums have a fixed order: results are bit-reproducible.
 * The workspace is the caller's: ir2rgb_video_metrics_workspace_bytes(N, H, W) bytes (negative for invalid
 * sizes), fully written before it is read, so it needs no zeroing and carries nothing between calls.
 * ir2rgb_video_metrics_tile(0 / 1) -> rows / columns of windows one workgroup evaluates (host only).
 * IR2RGB_EINVAL: NULL orig / pred / out / workspace, sizes out of range, workspace too small;
 * IR2RGB_EALIGN: out, range or workspace not on an 8-byte boundary.  Both before any launch.
 * ------------------------------------------------------------------------------------------ */
long ir2rgb_video_metrics_workspace_bytes(int N, int H, int W);
int ir2rgb_video_metrics_tile(int which);
int ir2rgb_video_metrics_u8(const uint8_t *orig, const uint8_t *pred, const double *range, double *out, void *workspace,
                            long workspace_bytes, int N, int H, int W, void *stream);

/* ------------------------------------------------------------------------------------------
 * Temporal consistency (warp_error.hip): the warp error of consecutive frames, the trainer's G_Warp term
 * (reference models/discriminator.py:137-138, MaskedL1Loss, Model.resample) as a score, in fp64 on the device.
 * prev, cur: uint8 [N][H][W][3]; flow: fp32 [N][2][H][W], x then y, in pixels, from cur to prev; weight: fp32
 * [N][1][H][W] or NULL (= 1).  N in [1, 65535], H, W >= 2, 3*H*W < 2^31.  For every pair n and pixel (y, x)
 *   gx = (-1 + x * (2 / (W - 1))) + fx / ((W - 1) / 2),  ix = ((gx + 1) * W - 1) * 0.5 clamped to [0, W - 1]
 *   x0 = floor(ix), x1 = min(x0 + 1, W - 1), ax = ix - x0; likewise y0, y1, ay       (get_grid + grid_sample(
 *                                                    align_corners=False, padding_mode="border"), as warp_blend)
 *   w_c = (1-ay)(1-ax) prev[y0][x0][c] + (1-ay) ax prev[y0][x1][c] + ay (1-ax) prev[y1][x0][c] + ay ax prev[y1][x1][c]
 *   d_c = cur[y][x][c] - w_c;  S1 = sum m |d_c|,  S2 = sum m d_c^2,  SC = sum m
 * and out[n] = {warp_l1 = S1 / (127.5 * 3 * H * W), warp_mse = S2 / (255^2 * 3 * SC), coverage = SC / (H * W)}.
 * No special cases: SC = 0 gives NaN; a NaN flow vector or weight stays in its own pair's row; an infinite flow
 * lands on the border.  No address leaves the frame whatever flow holds.  All sums have a fixed order: results
 * are bit-reproducible and pairs never mix.
 * The workspace is the caller's: ir2rgb_warp_error_workspace_bytes(N, H, W) bytes (negative for invalid sizes),
 * fully written before it is read.  Two launches.  W % 4 == 0 with flow and weight on 16-byte and cur on 4-byte
 * boundaries takes 16-byte loads, everything else the scalar form of the same code.
 * IR2RGB_EINVAL: NULL prev / cur / flow / out / workspace, sizes out of range, workspace too small;
 * IR2RGB_EALIGN: out or workspace off an 8-byte, flow or weight off a 4-byte boundary.  Both before any launch.
 * ------------------------------------------------------------------------------------------ */
long ir2rgb_warp_error_workspace_bytes(int N, int H, int W);
int ir2rgb_warp_error_u8(const uint8_t *prev, const uint8_t *cur, const float *flow, const float *weight, double *out,
                         void *workspace, long workspace_bytes, int N, int H, int W, void *stream);

/* ------------------------------------------------------------------------------------------
 * Colour scores (colour_metrics.hip): RGB PSNR and the CIELAB error of pred against orig, per frame, in fp64 on
 * the device -- what the gray-only scores above cannot see.  orig, pred: uint8 [N][H][W][3]; lin: 256 doubles on
 * the device, the sRGB decoding of a byte (c = v/255; c/12.92 if c <= 0.04045 else ((c + 0.055)/1.055)^2.4),
 * formed once by the caller.  N in [1, 65535], H, W >= 1, 3*H*W < 2^31.  For every pixel of either frame
 *   r, g, b = lin[R], lin[G], lin[B]
 *   tX = (0.412453 r + 0.357580 g + 0.180423 b) / 0.95047,  tY = (0.212671 r + 0.715160 g + 0.072169 b) / 1.0,
 *   tZ = (0.019334 r + 0.119193 g + 0.950227 b) / 1.08883                 (scikit-image's rgb2lab: D65, 2 degrees)
 *   f(t) = cbrt(t) if t > 0.008856 else 7.787 t + 16/116
 *   L = 116 f(tY) - 16,  a = 500 (f(tX) - f(tY)),  b = 200 (f(tY) - f(tZ))
 * and with dL, da, db the differences orig - pred:  dE = sqrt(dL^2 + da^2 + db^2) (CIE76),  dC = sqrt(da^2 + db^2),
 *   out[n] = {mse = sum (orig - pred)^2 / (3 H W) in byte units,  psnr = 10 log10(65025 / mse),
 *             delta_e = sum dE / (H W),  delta_l = sum |dL| / (H W),  delta_c = sum dC / (H W)}.
 * No special cases: identical frames give {0, +inf, 0, 0, 0}.  mse is exact (a sum of integers below 2^53); the
 * Lab sums have a fixed order: results are bit-reproducible and frames never mix.
 * The workspace is the caller's: ir2rgb_colour_metrics_workspace_bytes(N, H, W) bytes (negative for invalid
 * sizes), fully written before it is read.  Two launches.  W % 4 == 0 with orig and pred on 4-byte boundaries
 * takes dword loads, everything else the scalar form of the same code.
 * IR2RGB_EINVAL: NULL orig / pred / lin / out / workspace, sizes out of range, workspace too small;
 * IR2RGB_EALIGN: out, lin or workspace off an 8-byte boundary.  Both before any launch.
 * ------------------------------------------------------------------------------------------ */
long ir2rgb_colour_metrics_workspace_bytes(int N, int H, int W);
int ir2rgb_colour_metrics_u8(const uint8_t *orig, const uint8_t *pred, const double *lin, double *out, void *workspace,
                             long workspace_bytes, int N, int H, int W, void *stream);

/* ------------------------------------------------------------------------------------------
 * Frame scaling (frame_scale.hip): the loader's Image.resize(..., BICUBIC), crop and flip (reference
 * data/transform.py:64-113) on uint8 frames, equal to Pillow's 8-bit resampler byte for byte.
 *   src [N][Hs][Ws][C] uint8, C in {1, 3}  --scale-->  [new_h][new_w]  --crop-->  rows [crop_y, crop_y + Hc),
 *   columns [crop_x, crop_x + Wc)  --flip (0 / 1): columns mirrored-->  dst uint8 [N][Hc][Wc][C] (dst_f32 0) or fp32
 *   [N][C][Hc][Wc] = (float(v) / 255 - 0.5) / 0.5 with correctly rounded operations (dst_f32 1), the value
 *   ir2rgb_frame_push_u8 files for that byte.
 * Tables (device, int32), one pair per axis that changes size, computed on the host in double in Pillow's operation
 * order (ir2rgb_amd/transform.py: resample_coeffs): bounds [out][2] = {xmin, xmax}, coef [out][ksize] with 22
 * fraction bits, ksize = 2 * ceil(2 * max(in / out, 1)) + 1.  An axis whose size does not change takes NULL tables and
 * ksize 0: that pass copies.  Per pass out = clamp((2^21 + sum_{x < xmax} px[xmin + x] * coef[x]) >> 22, 0, 255) in
 * int32; the horizontal pass runs first and is rounded to uint8.  Two launches, integers only but for the fp32 store.
 * The workspace is the caller's: ir2rgb_frame_scale_workspace_bytes(...) bytes (negative for invalid sizes) -- the
 * horizontally scaled source rows that the kept output rows read, kept columns only.  It is fully written before it
 * is read.  Rows of Wc * C bytes that are a multiple of 4 with 4-byte aligned workspace and dst take dword accesses in
 * the vertical pass, everything else the scalar form.  No buffer may alias another.
 * IR2RGB_EINVAL: NULL src / dst / workspace, sizes or crop window out of range, workspace too small, tables missing,
 * given for an unchanged axis, or of another ksize; IR2RGB_EALIGN: tables or an fp32 dst off a 4-byte boundary.
 * ------------------------------------------------------------------------------------------ */
long ir2rgb_frame_scale_workspace_bytes(int N, int C, int Hs, int Ws, int new_h, int new_w, int crop_y, int crop_x, int Hc,
                                        int Wc);
int ir2rgb_frame_scale_u8(const uint8_t *src, void *dst, uint8_t *workspace, long workspace_bytes, const int *xbounds,
                          const int *xcoef, int xksize, const int *ybounds, const int *ycoef, int yksize, int N, int C, int Hs,
                          int Ws, int new_h, int new_w, int crop_y, int crop_x, int Hc, int Wc, int flip, int dst_f32,
                          void *stream);

/* ------------------------------------------------------------------------------------------
 * Training snapshots (visuals.hip): the panels the reference's util.save_all_tensors (util/util.py:13-104) makes
 * on the host, composed on the device.  Every source is fp32 [C][H][W], contiguous; out is uint8 [n][H][W][3],
 * one panel per slot, a one-channel panel written to all three bytes.  Kinds:
 *   IR2RGB_PANEL_IMAGE_NORM  C in {1, 3}: trunc(clip((x + 1) / 2 * 255, 0, 255))      util.tensor2im(x)
 *   IR2RGB_PANEL_IMAGE_UNIT  C in {1, 3}: trunc(clip(x * 255, 0, 255))                util.tensor2im(x, normalize=False)
 *   IR2RGB_PANEL_FLOW        C = 2: util.tensor2flow's coding, (u, v) -> HSV -> RGB with
 *       mag = sqrt(u^2 + v^2), [mn, mx] = its range over the panel (NaN magnitudes ignored),
 *       H = trunc(atan2(v, u) in [0, 2 pi) * 90 / pi) mod 180, S = 255,
 *       V = trunc((mag - mn) * 255 / (mx - mn)); 0 everywhere when mx == mn, 0 for a NaN magnitude,
 *       and the integer 8-bit HSV -> RGB with hue in [0, 180): i = H / 30, r = H % 30,
 *       t = (2 V r + 30) / 60, q = (2 V (30 - r) + 30) / 60, p = 0, sectors (V,t,p) (q,V,p) (p,V,t) (p,q,V) (t,p,V) (V,p,q).
 *   fp32 with correctly rounded operations in the order written (NaN -> 0 in all three kinds); results are
 *   bit-reproducible.
 * panels is a HOST array; it is copied into the launch's arguments, nothing is uploaded.  The workspace is the
 * caller's: ir2rgb_visuals_workspace_bytes(number of FLOW panels, H, W) bytes of fp32 (min, max) rows (negative
 * for invalid sizes), fully written before it is read; it may be NULL when no panel is a FLOW panel.  Two
 * launches with a FLOW panel, one without.  16-byte aligned sources with W % 4 == 0 and a 4-byte aligned out take
 * 16-byte loads and dword stores, everything else the scalar form.  No buffer may alias out or the workspace.
 * IR2RGB_EINVAL: NULL panels / out / source, n outside [1, 16], H or W < 1, H * W * 3 > 2^31 - 1, an unknown
 * kind, a channel count that does not fit the kind, a NULL workspace with a FLOW panel; IR2RGB_EALIGN: a source
 * or the workspace off a 4-byte boundary.  Both before any launch.
 * ------------------------------------------------------------------------------------------ */
#define IR2RGB_VISUALS_MAX_PANELS 16
#define IR2RGB_PANEL_IMAGE_NORM 0
#define IR2RGB_PANEL_IMAGE_UNIT 1
#define IR2RGB_PANEL_FLOW 2
typedef struct ir2rgb_panel {
    const float *src;
    int kind;
    int channels;
} ir2rgb_panel;

long ir2rgb_visuals_workspace_bytes(int n_flow_panels, int H, int W);
int ir2rgb_visuals_u8(const ir2rgb_panel *panels, int n, int H, int W, float *workspace, uint8_t *out, void *stream);

/* ------------------------------------------------------------------------------------------
 * JPEG output (jpeg.hip): baseline JPEG files of uint8 frames, equal byte for byte to the files Pillow (libjpeg)
 * writes with Image.save(f, "JPEG", quality=q, subsampling=..., restart_marker_rows=restart_rows); the rules are
 * restated in ir2rgb_amd/jpeg.py (jpeg_reference), which is the definition.
 *   src [N][H][W][C] uint8, C in {1, 3}.  mode IR2RGB_JPEG_444 / _420 (C = 3: YCbCr, interleaved MCUs) or IR2RGB_JPEG_L
 *   (one component: channel 0 at pixel stride C, so a one-channel panel of a three-channel stack needs no copy).
 *   out [N][capacity] uint8: file n = the header, then the scan with FF D0+(i mod 8) after every restart_rows MCU
 *   rows, then FF D9; lengths [N] int32 = its size.  Bytes of out past the length are not written.
 * header (device, header_bytes bytes) is everything up to and including SOS, built on the host; tables (device,
 * uint32 [672]) come from the same host objects: quantisation [2][64] in natural order (luminance, chrominance), DC
 * codes [2][16] and AC codes [2][256] indexed by symbol as (code length << 16 | code).  max_dc_len / max_ac_len
 * (1..16) are the longest code lengths of those tables; lengths read from the tables are clamped to them and
 * quantisation entries to [1, 255].
 * Capacity: a block codes to at most bits = (max_dc_len + 11) + 63 * (max_ac_len + 10) bits -- its DC code, and at
 * most 63 AC codes of at most max_ac_len + 10 bits, since every AC code (a coefficient, ZRL, EOB) accounts for at
 * least one of the 63 positions that no other code accounts for.  A restart interval of B = restart_rows * MCUs per
 * row * blocks per MCU blocks is at most ceil(B * bits / 8) bytes with its padding, twice that after byte stuffing
 * (rounded up to 16), plus 2 marker bytes: ir2rgb_jpeg_capacity_bytes = header_bytes + intervals * that.
 * The workspace is the caller's, ir2rgb_jpeg_workspace_bytes(...) bytes (both counts negative for invalid sizes):
 * the quantised blocks int16 [N][blocks][64] in coding and zigzag order, the byte count of every interval, and one
 * capacity-sized scratch region per interval.  Every part is written before it is read.  Three launches whatever N
 * and the pixels are; integers only.  No buffer may alias out or the workspace.
 * IR2RGB_EINVAL: a NULL pointer, N outside [1, 65535], H or W outside [1, 65535], C or mode unknown or C != 3 in a
 * colour mode, restart_rows < 1 or an interval above 65535 MCUs, header_bytes < 1, code lengths outside [1, 16],
 * capacity or workspace_bytes too small, a worst-case file above 2^31 - 1 bytes; IR2RGB_EALIGN: workspace off a
 * 16-byte, tables or lengths off a 4-byte boundary.  Both before any launch.
 * ------------------------------------------------------------------------------------------ */
#define IR2RGB_JPEG_444 0
#define IR2RGB_JPEG_420 1
#define IR2RGB_JPEG_L 2
#define IR2RGB_JPEG_TABLE_WORDS 672

long ir2rgb_jpeg_workspace_bytes(int N, int H, int W, int mode, int restart_rows, int max_dc_len, int max_ac_len);
long ir2rgb_jpeg_capacity_bytes(int H, int W, int mode, int restart_rows, int header_bytes, int max_dc_len, int max_ac_len);
int ir2rgb_jpeg_encode_u8(const uint8_t *src, uint8_t *out, int *lengths, void *workspace, long workspace_bytes,
                          const uint8_t *header, int header_bytes, const unsigned *tables, int N, int C, int H, int W, int mode,
                          int restart_rows, int max_dc_len, int max_ac_len, long capacity, void *stream);

/* ------------------------------------------------------------------------------------------
 * JPEG input (jpeg_decode.hip): baseline JPEG files decoded into uint8 frames, equal pixel for pixel to what Pillow
 * (libjpeg-turbo) decodes, np.asarray(Image.open(f)); the rules are restated in ir2rgb_amd/jpeg_decode.py
 * (decode_reference for the pixels, entropy_model for the parallel entropy decode), which is the definition.
 *   files: the scan bytes (everything behind SOS up to the closing marker, still byte-stuffed, restart markers
 *   included) of N files, one after the other, any alignment; file_offsets int32 [N + 1]: file n is bytes
 *   [file_offsets[n], file_offsets[n + 1]) of files.
 *   segments int32 [N][n_segments][4]: one record per restart interval, (begin, end, first MCU, MCUs) with the byte
 *   range relative to the file's scan bytes and without the marker; a file without DRI has one record; records a file
 *   does not use are all zero.  tables int32 [N][IR2RGB_JPEGD_TABLE_WORDS], per file: the quantisation table of every
 *   component [3][64] in natural order; the Huffman table slot (0..1) of every component, DC [3] then AC [3], 2 words
 *   unused; four Huffman tables DC 0, DC 1, AC 0, AC 1 of 288 words: limit [16], offset [16], values [256] -- the code of
 *   a 16-bit window w has the smallest length l with w < limit[l - 1] and the symbol values[offset[l - 1] + (w >> (16 -
 *   l))].  All files of a call share H, W and mode (IR2RGB_JPEG_444 / _420 / _422: three components, YCbCr, luminance
 *   sampled 1x1 / 2x2 / 2x1; IR2RGB_JPEG_L: one component); tables, restart intervals and sizes are per file.
 *   out [N][H][W][C_out] uint8; C_out = 3 in mode L replicates the channel.  status [N] int32: 0, or the IR2RGB_JPEGD_E*
 *   bits of the damage the decode of file n met (the pixels of such a file are unspecified but written).
 * A segment's bytes are cut into subsequences of sub_bytes (>= 1; enlarged per segment to ceil(bytes /
 * IR2RGB_JPEGD_THREADS) when it has more than that many), which one workgroup decodes in parallel by relaxation: see
 * jpeg_decode.hip.  The result does not depend on sub_bytes.  Every read of files stays inside the record's range
 * clamped to the file's; no decoded value is used as an index unclamped; records are clamped to the frame's MCUs.
 * The workspace is the caller's, ir2rgb_jpeg_decode_workspace_bytes(...) bytes (negative for invalid sizes): the
 * coefficients int16 [N][blocks][64], the component planes on their block grids, and (status bits, relaxation rounds)
 * int32 [N][n_segments][2] at its end.  Every part is written before it is read.  Three launches whatever N and the
 * files are; integers only.  No buffer may alias out, status or the workspace.
 * IR2RGB_EINVAL: a NULL pointer, N or n_segments outside [1, 65535], H or W outside [1, 65535], C_out or mode
 * unknown or C_out != 3 in a colour mode, sub_bytes < 1, workspace_bytes too small, more than 2^31 - 1 coefficient
 * bytes; IR2RGB_EALIGN: workspace off a 16-byte, file_offsets, segments, tables or status off a 4-byte boundary.
 * Both before any launch.
 * ------------------------------------------------------------------------------------------ */
#define IR2RGB_JPEG_422 3
#define IR2RGB_JPEGD_TABLE_WORDS 1352
#define IR2RGB_JPEGD_THREADS 512
#define IR2RGB_JPEGD_ECODE 1     /* 16 bits that are no Huffman code */
#define IR2RGB_JPEGD_EINDEX 2    /* a coefficient index past 63 */
#define IR2RGB_JPEGD_EBLOCKS 4   /* the segment does not hold its MCUs' blocks */
#define IR2RGB_JPEGD_ELEFTOVER 8 /* more than the padding is left behind the last block */
#define IR2RGB_JPEGD_ESEGMENT 16 /* a segment record outside the frame's MCUs */

long ir2rgb_jpeg_decode_workspace_bytes(int N, int H, int W, int mode, int n_segments);
int ir2rgb_jpeg_decode_u8(const uint8_t *files, const int *file_offsets, const int *segments, const int *tables, uint8_t *out,
                          int *status, void *workspace, long workspace_bytes, int N, int C_out, int H, int W, int mode,
                          int n_segments, int sub_bytes, void *stream);

/* ------------------------------------------------------------------------------------------
 * Raw thermal input (thermal_agc.hip): a camera's automatic gain control on the device, integers only.  x: uint16
 * [N][H][W], N consecutive frames of one sequence (2-byte aligned, nothing more) -> out uint8 [N][H][W][channels],
 * channels 1 or 3 (the byte repeated).  Per frame: the 65536-bin histogram, clipped at plateau in mode 0 (plateau
 * equalisation) and taken as it is in mode 1 (percentile window with tail_ppm parts per million cut at either end),
 * is blended in Q16 into the damped histogram S with weight 65536 - a_q (a_q = round(damping 65536) in 0..65535);
 * the table comes from the running sum of S.  The definition, which the kernels equal bit for bit, is
 * ir2rgb_amd.thermal.agc_reference; thermal_agc.hip restates it.
 *   state   int64 [65537] on the device, the caller's, kept from call to call: S, and in word 65536 the
 *           sequence-start flag -- 0: the next frame starts a sequence (S = g << 16); the call sets it to 1.  A new
 *           sequence is a memset of that word; the rest of a fresh state may hold anything.
 *   lut     uint8 [N][65536], levels int32 [N][2] ((v0, v1) or (lo, hi)): written per frame.
 * The workspace is the caller's, ir2rgb_thermal_agc_workspace_bytes(N, H, W) bytes (negative for invalid sizes): the
 * per-frame histograms.  IT MUST BE ALL ZERO ON ENTRY and is all zero again when the call's work is done (the table
 * pass zeroes what it has read), so a caller clears it once, when it allocates it.
 * N in [1, 65535], H, W >= 1, H W <= 2^26.  Three launches whatever the frames hold, no host synchronisation.
 * IR2RGB_EINVAL: a NULL pointer, sizes or parameters out of range (plateau < 1, tail_ppm outside [0, 500000)),
 * workspace too small; IR2RGB_EALIGN: x off a 2-byte, levels off a 4-byte, state, lut or workspace off a 16-byte
 * boundary.  Both before any launch.
 * ------------------------------------------------------------------------------------------ */
long ir2rgb_thermal_agc_workspace_bytes(int N, int H, int W);
int ir2rgb_thermal_agc_u16(const uint16_t *x, uint8_t *out, long long *state, uint8_t *lut, int *levels, void *workspace,
                           long workspace_bytes, int N, int H, int W, int channels, int mode, int plateau, int a_q,
                           int tail_ppm, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* IR2RGB_HIP_H */
