/* sfamd.h -- C ABI of libsfamd.so, the MI355X (gfx950) video-backbone forward/backward engine.
 *
 * The reference (facebookresearch/SlowFast) has no native layer: every FLOP of its hot path is a
 * torch.nn call inside the slowfast/models package.  Each entry point below therefore cites the torch
 * call site(s) it replaces.  Conventions:
 *   - plain pointers + sizes, no torch types; every pointer is a DEVICE pointer unless noted;
 *   - activations are fp16, channels-last: a logical (N,C,T,H,W) tensor stored N,T,H,W,C with a row
 *     pitch `ld` (elements) >= C so channel-slice views need no copy; C % 8 == 0, 16-byte aligned;
 *   - statistics, affine parameters, weights and weight gradients are fp32;
 *   - the callee allocates nothing and never synchronises; work is enqueued on `stream`
 *     (a hipStream_t passed as void*); return 0 on success, negative on error (sf_last_error()).
 */
#ifndef SFAMD_H
#define SFAMD_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define SF_ABI_VERSION 38
typedef void* sf_stream_t;

/* Geometry of one nn.Conv3d (groups == 1).  Ci is the channel count of the activation buffer
 * (the stem's 3-channel clip is zero-padded to 8), Cw the channel count of the fp32 weight. */
typedef struct sf_conv_desc {
    int32_t N, Ci, Ti, Hi, Wi;
    int32_t Co, To, Ho, Wo; /* To/Ho/Wo may be smaller than the conv formula: trailing outputs are dropped */
    int32_t kT, kH, kW;
    int32_t sT, sH, sW;
    int32_t pT, pH, pW;
    int32_t dT, dH, dW;
    int32_t Cw;
    int32_t ldx, ldy; /* row pitch of the input / output activation buffers, in elements */
    int32_t Cow;      /* channel count of the fp32 weight on the OUTPUT side (0 = Co): activation buffers hold Co =
                         Cow rounded up to 8 channels, the pad channels are produced as exact zeros (X3D widths 54, 108) */
} sf_conv_desc;

int sf_abi_version(void);
const char* sf_backend(void);     /* "gfx950" (product) or "hostsim" (CPU test build of the same sources) */
/* The 16-bit storage type this build of the library keeps activations / packed weights in and feeds the MFMAs with (every
 * `void*` activation or packed-weight argument below points at elements of THAT type; "fp16" in the comments of this header
 * means it).  The reference runs its mixed-precision path under torch.cuda.amp.autocast (tools/train_net.py:101-118), which
 * admits float16 and bfloat16; libsfamd.so is the float16 build, libsfamd_bf16.so (same sources, -DSF_ACT_BF16) the bfloat16
 * one.  Accumulation, statistics and parameter gradients are fp32 in both. */
#define SF_ACT_FP16 0
#define SF_ACT_BF16_ID 1
int sf_act_dtype(void);
const char* sf_last_error(void); /* host string, thread-local */
/* Build provenance: the first 16 hex digits of the sha256 over the kernel sources and this header the binary was compiled
 * from (slowfast_amd/build_ext.py:source_id passes it as -DSF_BUILD_ID).  The Python binding recomputes it from the sources
 * beside the binary and refuses a library built from anything else. */
const char* sf_build_id(void);

/* ---- Conv3d -- replaces nn.Conv3d at resnet_helper.py:331-369 (BottleneckTransform a/b/c),
 * resnet_helper.py:485-493 (ResBlock.branch1), stem_helper.py:182-189 (ResNetBasicStem.conv),
 * video_model_builder.py:147-154 (FuseFastToSlow.conv_f2s), and their autograd backward. */
int sf_conv_weight_ld(const sf_conv_desc* d, int32_t* ldf, int32_t* ldd);
/* fp32 [Co][Cw][kT][kH][kW] -> fp16 forward operand wf[Co][ldf] and (optional) dgrad operand wd[Ci][ldd] */
int sf_prep_weights(const sf_conv_desc* d, const float* w, void* wf, void* wd, sf_stream_t stream);
/* The same packing for MANY weights in one launch (a training step re-packs every layer after the optimizer update: one
 * launch instead of one per nn.Conv3d / nn.Linear).  `items` is a DEVICE array the caller uploads once; sf_prep_item_fill
 * writes the host copy of one entry from a descriptor (an nn.Linear [N][K] is the 1x1x1 case Co=N, Ci=Cw=K: wf = fp16
 * weight, wd = its transpose).  An item is cut into sf_prep_item_blocks(item) bricks; blk_item / blk_off (device, int32):
 * workgroup b packs brick blk_off[b] (0 .. blocks-1) of items[blk_item[b]]. */
typedef struct sf_prep_item {
    const float* w;   /* fp32 [Cow][Cw][taps] */
    void* wf;         /* fp16 [Co][ldf] */
    void* wd;         /* fp16 [Cp][ldd], or NULL */
    int32_t Co, Cow, Cw, Cp, taps, ldf, ldd;
    int32_t pad;      /* brick shape, written by sf_prep_item_fill */
} sf_prep_item;
int sf_prep_item_fill(const sf_conv_desc* d, const float* w, void* wf, void* wd, sf_prep_item* item);
int64_t sf_prep_item_blocks(const sf_prep_item* item);
int sf_prep_weights_batch(const sf_prep_item* items, const int32_t* blk_item, const int32_t* blk_off, int32_t nblocks,
                          sf_stream_t stream);
/* number of 128-row tiles = rows of `stat_part` */
int sf_conv_fwd_mtiles(const sf_conv_desc* d);
/* y = conv(act(x)), act(x) = x or relu?(x*in_scale + in_shift) applied on the fly (zero padding is
 * applied AFTER act, as in the reference where the padded tensor is the post-ReLU activation).
 * stat_part (optional) receives per-tile per-channel sum / sum of squares of y (bias included): [mtiles][2][Co] fp32. */
int sf_conv_fwd(const sf_conv_desc* d, const void* x, const void* wf, const float* in_scale, const float* in_shift,
                int in_relu, const float* bias, void* y, float* stat_part, sf_stream_t stream);
/* Inference-fused convolution (the eval / multi-view test path, tools/test_net.py:25-151):
 * eval-mode nn.BatchNorm3d is an affine map of its input, so the caller folds it into the weights (wf = pack(w * scale))
 * and a bias (shift); the nn.ReLU and the residual addition of resnet_helper.py:377-392, 512-521 run in the epilogue:
 *   y = act(conv(x) + bias [+ resid]),   act = ReLU when out_relu.   bias [Co] fp32 (may be NULL), resid [M][ldr] fp16. */
int sf_conv_fwd_fused(const sf_conv_desc* d, const void* x, const void* wf, const float* bias, const void* resid,
                      int32_t ldr, int out_relu, void* y, sf_stream_t stream);
/* dx = conv_transpose(dy, w) (+ resid), dx pitch = d->ldx, dy pitch = d->ldy.  resid_bits (optional, with resid): the
 * 1-bit ReLU mask sf_bn_act wrote for the block input ([positions][Ci/8] bytes): only residual elements whose bit is set
 * are added -- the masked block-output gradient of the identity shortcut (resnet_helper.py:512-521 backward) without
 * materialising it. */
int sf_conv_dgrad(const sf_conv_desc* d, const void* dy, const void* wd, const void* resid, int32_t ldr,
                  const void* resid_bits, void* dx, sf_stream_t stream);
/* sf_conv_dgrad + the reduction pass of the BatchNorm backward(s) that consume dx (round 3).  The gradient dx this call
 * stores is dz of a BatchNorm-ReLU whose backward first needs the per-channel sums of g and g * y over the positions
 * (sf_bn_bwd_reduce), g = dz under the ReLU mask.  The epilogue takes them from the fp16 tile it stores -- one read of the y
 * tile instead of a pass over dz and y, one launch less:
 *   - inner activations of a block (BottleneckTransform b / c reading relu(a_bn(a(x))) / relu(b_bn(b(.))),
 *     resnet_helper.py:377-392): mask = (bn_y * mask_scale + mask_shift > 0), mask_bits NULL;
 *   - a block INPUT that is the previous block's output relu(bn_c(yc) + shortcut) (resnet_helper.py:512-521): mask_bits = the
 *     1-bit image sf_bn_act wrote for that output ([positions][Ci/8]), bn_y = yc (a projection shortcut's own BatchNorm keeps
 *     its separate reduction pass).
 * bn_part[row][2][Ci] fp32, one row per M tile of the kernel that ran (fixed order: deterministic); *bn_rows = rows written,
 * to be passed to sf_bn_bwd_finalize as nblk -- or 0 when the geometry keeps the separate pass (strided data gradients): the
 * table is then untouched and the caller runs sf_bn_bwd_reduce.  The table holds ceil(positions / 128) rows (bn_part_rows);
 * bn_rows is a HOST pointer. */
int sf_conv_dgrad_bn(const sf_conv_desc* d, const void* dy, const void* wd, const void* resid, int32_t ldr,
                     const void* resid_bits, void* dx, const float* mask_scale, const float* mask_shift,
                     const void* mask_bits, const void* bn_y, int32_t bn_ldy, float* bn_part, int32_t bn_part_rows,
                     int32_t* bn_rows, sf_stream_t stream);
/* dw[Co][Cw][taps] = (zero_first ? 0 : dw) + out_scale * sum_m dy[m] (x) act(x)[m].  The reduction over positions
 * is split; `workspace` (>= sf_conv_wgrad_workspace(d) bytes, caller-owned) holds the per-split partials, which a
 * second kernel sums in a fixed order (no atomics: results are run-to-run reproducible). */
int64_t sf_conv_wgrad_workspace(const sf_conv_desc* d);
/* `rowtab` (optional): the per-output-row table {first input position, tap-validity mask} of the large-K kernel.  It
 * depends on the geometry only: build it once with sf_conv_wgrad_rowtab into sf_conv_wgrad_rowtab_bytes(d) bytes (0: this
 * geometry takes another kernel, pass NULL) and hand it to every call; NULL rebuilds it in the workspace per call. */
int64_t sf_conv_wgrad_rowtab_bytes(const sf_conv_desc* d);
int sf_conv_wgrad_rowtab(const sf_conv_desc* d, void* tab, sf_stream_t stream);
int sf_conv_wgrad(const sf_conv_desc* d, const void* x, const float* in_scale, const float* in_shift, int in_relu,
                  const void* dy, float* dw, float out_scale, int zero_first, void* workspace, int64_t workspace_bytes,
                  const void* rowtab, sf_stream_t stream);
/* ---- Grouped (1,3,3) Conv3d (ABI 38) -- replaces nn.Conv3d(groups=num_groups) at resnet_helper.py:346-358 (BottleneckTransform.b
 * of the ResNeXt configurations, RESNET.NUM_GROUPS > 1) and its autograd backward.  The descriptor is read as: Ci == Co == C, the
 * channel count of the activation on both sides; Cw == Cg = C / groups, the channels per group of the fp32 weight
 * [C][Cg][1][3][3]; Cow 0.  Supported: kernel (1,3,3), stride (1,1,1) or (1,2,2), dilation (1,k,k) with padding (0,k,k) for k = 1, 2,
 * Cg in {4, 8, 16, 32, 64}, C a multiple of the bundle width B = max(32, Cg).  Anything else fails with a message that names what
 * was asked for, and writes nothing.  A bundle is a run of B consecutive channels; its packed weight is the dense [B][9*B]
 * operand with zeros off the diagonal blocks, and the bundle index is a grid dimension of the implicit-GEMM kernel.
 * sf_gconv_prep_weights: wf[C][9*B] (row co, column tap*B + ci - bundle base) and, optionally, the data-gradient operand
 *   wd[C][9*B] (row ci, column (8 - tap)*B + co - bundle base: transposed within each block, taps mirrored).  Every element of both
 *   is written by the kernel.
 * sf_gconv_fwd: y = act(conv(x) + bias), act = ReLU when out_relu (the eval form with BatchNorm folded in); bias [C] fp32 or NULL;
 *   stat_part (optional) as sf_conv_fwd writes it: [sf_conv_fwd_mtiles(d)][2][C], sums of the fp32 accumulators.
 * sf_gconv_dgrad: dx = conv_transpose(dy, w), dx pitch d->ldx, dy pitch d->ldy.
 * sf_gconv_wgrad: dw[C][Cg][9] = (zero_first ? 0 : dw) + out_scale * dL/dw.  Per bundle the B x 9B product is formed in
 *   `workspace` (>= sf_gconv_wgrad_workspace(d) bytes) and only its diagonal blocks are summed, in a fixed order (no atomics:
 *   run-to-run identical), and stored. */
int sf_gconv_prep_weights(const sf_conv_desc* d, const float* w, void* wf, void* wd, sf_stream_t stream);
int sf_gconv_fwd(const sf_conv_desc* d, const void* x, const void* wf, const float* bias, int out_relu, void* y,
                 float* stat_part, sf_stream_t stream);
int sf_gconv_dgrad(const sf_conv_desc* d, const void* dy, const void* wd, void* dx, sf_stream_t stream);
int64_t sf_gconv_wgrad_workspace(const sf_conv_desc* d);
int sf_gconv_wgrad(const sf_conv_desc* d, const void* x, const void* dy, float* dw, float out_scale, int zero_first,
                   void* workspace, int64_t workspace_bytes, sf_stream_t stream);
/* Block-final BatchNorm backward fused into both gradients of the block's last convolution (ABI 32; resnet_helper.py:361-369,
 * :512-521).  Replaces the three calls sf_bn_bwd_apply(dz, mask_bits, yc, coef) -> dy_c, sf_conv_wgrad(act, dy_c) and
 * sf_conv_dgrad_bn(dy_c, wd) for a 1x1x1 unit-stride unpadded convolution d: dy_c = (f16)(k1 * g + k2 + k3 * yc) is formed per row
 * tile on chip, rounded exactly as sf_bn_bwd_apply stores it, and never written to memory.
 * sf_conv_c_bwd_plan: 1 when d takes this path (Ci % 8 == 0 <= 64, Co % 32 == 0 <= 256, no fused input BatchNorm (in_affine == 0),
 * the 1-bit form of the block-output mask (mask_bits != 0); never a function of the row count), else 0 (the caller keeps the three
 * calls); *tile_rows = rows per row tile, *workspace_bytes = size of `workspace`.
 * sf_conv_c_bwd: dz [M][lddz] gradient w.r.t. the block output, mask_bits [M][Co/8] (sf_bn_act), yc [M][ldyc] the raw output of d,
 * coef [3][Co] from sf_bn_bwd_finalize, act [M][d->ldx] the input of d, wd the packed data-gradient operand.  Outputs: d_in
 * [M][ld_in] (d->ldy is not used), dw as sf_conv_wgrad writes it (out_scale, zero_first).  Optional (bn_part != NULL), exactly as
 * sf_conv_dgrad_bn with mask_scale / mask_shift: the sums of g and g * bn_y over the stored d_in, g = d_in under
 * (bn_y * bn_scale + bn_shift > 0), one row [2][Ci] per row tile in tile order; bn_part_rows >= ceil(M / tile_rows);
 * *bn_rows (HOST pointer) = rows written.  Deterministic: no atomics, fixed summation order for a given workgroup count. */
int sf_conv_c_bwd_plan(const sf_conv_desc* d, int in_affine, int mask_bits, int32_t* tile_rows, int64_t* workspace_bytes);
int sf_conv_c_bwd(const sf_conv_desc* d, const void* dz, int32_t lddz, const void* mask_bits, const void* yc, int32_t ldyc,
                  const float* coef, const void* act, const void* wd, const float* bn_scale, const float* bn_shift,
                  const void* bn_y, int32_t bn_ldy, float* bn_part, int32_t bn_part_rows, int32_t* bn_rows, void* d_in,
                  int32_t ld_in, float* dw, float out_scale, int zero_first, void* workspace, int64_t workspace_bytes,
                  sf_stream_t stream);
/* The same fusion for the projection shortcut of a stage's first block (ABI 36; ResBlock.branch1 + branch1_bn, resnet_helper.py:485-499,
 * :512-521): replaces sf_bn_bwd_apply(dz, mask_bits, y1, coef) -> dy1, sf_conv_wgrad(x, dy1) and sf_conv_dgrad(dy1, wd) of a 1x1x1
 * unpadded, undilated convolution d of stride (1,1,1), or (1,2,2) with Hi == 2 Ho and Wi == 2 Wo, bit for bit.
 * sf_conv_proj_bwd_plan: 1 when d takes this path (Ci % 8 == 0 <= 128, Co % 32 == 0 <= 256, in_affine == 0, mask_bits != 0), else 0;
 * *workspace_bytes = size of `workspace`.  The test hook SF_CBWD=0 switches this path off together with sf_conv_c_bwd.
 * sf_conv_proj_bwd: dz [Mo][lddz], mask_bits [Mo][Co/8], y1 [Mo][ldy1] the raw output of d, coef [3][Co] from sf_bn_bwd_finalize,
 * x [Mi][d->ldx] the block input, wd the packed data-gradient operand (Mo / Mi = output / input positions).  Outputs: d_in [Mi][ld_in],
 * EVERY row written (the input rows a stride of 2 never samples are +0), dw as sf_conv_wgrad writes it. */
int sf_conv_proj_bwd_plan(const sf_conv_desc* d, int in_affine, int mask_bits, int64_t* workspace_bytes);
int sf_conv_proj_bwd(const sf_conv_desc* d, const void* dz, int32_t lddz, const void* mask_bits, const void* y1, int32_t ldy1,
                     const float* coef, const void* x, const void* wd, void* d_in, int32_t ld_in, float* dw, float out_scale,
                     int zero_first, void* workspace, int64_t workspace_bytes, sf_stream_t stream);

/* ---- BatchNorm3d -- replaces nn.BatchNorm3d built by batchnorm_helper.py:16-37 (get_norm) at every
 * *_bn call site of resnet_helper.py / stem_helper.py / video_model_builder.py:155-159, plus the
 * nn.ReLU and the residual add of resnet_helper.py:512-521. */
/* Creal <= C: number of real channels (length of gamma/beta/running stats); channels [Creal, C) are zero padding of the
 * activation buffer and get scale = shift = 0.
 * `part` is scratch: long tables are folded in place before the final reduction (contents are destroyed).
 * nblk > 0: training (partials -> batch statistics, running stats updated when non-null);
 * nblk == 0: eval (running statistics).  Outputs scale = gamma*rstd, shift = beta - mean*scale. */
int sf_bn_finalize(float* part, int32_t nblk, int32_t C, int32_t Creal, float count, const float* gamma, const float* beta,
                   float* running_mean, float* running_var, float momentum, float eps, float* scale, float* shift,
                   float* save_mean, float* save_rstd, sf_stream_t stream);
/* out = relu?( y*scale+shift [+ r*rscale+rshift | + r] ); scale == NULL means identity.  mask_out (optional): [M][C/8]
 * bytes, bit e of byte (m, c/8) = out[m][c+e] > 0 -- the ReLU mask the backward kernels read instead of `out` (1/16 of
 * the bytes). */
int sf_bn_act(int64_t M, int32_t C, const void* y, int32_t ldy, const float* scale, const float* shift, const void* r,
              int32_t ldr, const float* rscale, const float* rshift, int relu, void* out, int32_t ldo, void* mask_out,
              sf_stream_t stream);
int sf_bn_bwd_blocks(int64_t M, int32_t C); /* rows of `part` for the two calls below */
/* part[blk][0][c] = sum g, part[blk][1][c] = sum g*y, g = dz masked by (zmask > 0) or by
 * (y*scale+shift > 0) when relu_self.  ldm == 0 with a non-NULL zmask: zmask is the BIT mask written by sf_bn_act
 * ([M][C/8] bytes); same convention in sf_bn_bwd_apply. */
int sf_bn_bwd_reduce(int64_t M, int32_t C, const void* dz, int32_t lddz, const void* zmask, int32_t ldm, const void* y,
                     int32_t ldy, const float* scale, const float* shift, int relu_self, float* part,
                     sf_stream_t stream);
/* dgamma/dbeta (fp32, unscaled by inv_loss_scale) and coef[3][C] with dy = k1*g + k2 + k3*y */
int sf_bn_bwd_finalize(float* part, int32_t nblk, int32_t C, int32_t Creal, float count, const float* gamma, const float* mean,
                       const float* rstd, float inv_loss_scale, float* dgamma, float* dbeta, int accumulate,
                       float* coef, sf_stream_t stream);
int sf_bn_bwd_apply(int64_t M, int32_t C, const void* dz, int32_t lddz, const void* zmask, int32_t ldm, const void* y,
                    int32_t ldy, const float* scale, const float* shift, int relu_self, const float* coef, void* dy,
                    int32_t lddy, void* gout, int32_t ldg, sf_stream_t stream);

/* ---- nn.MaxPool3d([1,kH,kW],[1,sH,sW],[0,pH,pW]) fused with the producer's BN(+ReLU) --
 * stem_helper.py:190-201 (bn -> relu -> pool_layer). */
int sf_pool_fwd(int32_t N, int32_t T, int32_t H, int32_t W, int32_t C, int32_t kH, int32_t kW, int32_t sH, int32_t sW,
                int32_t pH, int32_t pW, const void* y, int32_t ldy, const float* scale, const float* shift, int relu,
                void* out, int32_t ldo, void* argmax, int32_t cls, sf_stream_t stream);
/* g[N,T,H,W,C] = gradient w.r.t. the BatchNorm output (pool + ReLU backward) from the forward's byte argmax table
 * [N,T,Ho,Wo][C] (window-local index kh*kW+kw of the first maximum, as recorded by torch's max_pool3d; with relu, 0xFF for a
 * window whose maximum is not positive -- the ReLU mask `pooled > 0` -- written by sf_pool_fwd(relu = 1), kH*kW <= 255).
 * `pooled` / `ldp` are kept in the signature and not read (round 6); `relu` must be the forward's. */
int sf_pool_bwd(int32_t N, int32_t T, int32_t H, int32_t W, int32_t C, int32_t kH, int32_t kW, int32_t sH, int32_t sW,
                int32_t pH, int32_t pW, const void* pooled, int32_t ldp, const void* argmax, int relu,
                const void* dout, int32_t lddo, void* g, int32_t ldg, int32_t cls, sf_stream_t stream);
/* cls != 0 (both calls): TOKEN tensors -- every sample's T*H*W rows are preceded by one cls-token row that passes
 * through the pool unchanged; replaces attention_pool(x, pool_skip=nn.MaxPool3d) of attention.py:13-45, 485-498. */

/* ---- nn.MaxPool3d(pool_size, stride = pool_size, padding 0) in front of conv_phi / conv_g of the Nonlocal block
 * (nonlocal_helper.py:96-114); argmax: byte table [N,To,Ho,Wo][C] */
int sf_pool3d_fwd(int32_t N, int32_t T, int32_t H, int32_t W, int32_t C, int32_t kT, int32_t kH, int32_t kW, const void* x,
                  int32_t ldx, void* out, int32_t ldo, void* argmax, sf_stream_t stream);
int sf_pool3d_bwd(int32_t N, int32_t T, int32_t H, int32_t W, int32_t C, int32_t kT, int32_t kH, int32_t kW,
                  const void* argmax, const void* dout, int32_t lddo, void* dx, int32_t lddx, sf_stream_t stream);

/* ---- layout: clips arrive NCTHW fp32 (tools/train_net.py:79-98) */
int sf_ncthw_to_cl(const float* x, int32_t N, int32_t C, int64_t S, int32_t Cp, void* out, sf_stream_t stream);
int sf_cl_to_ncthw(const void* x, int32_t ld, int32_t N, int32_t C, int64_t S, float* out, sf_stream_t stream);

/* =====================================================================================================
 * Token-space entry points (MViT pooled attention, Mlp; also used by Nonlocal and X3D).  Token tensors are fp16
 * [rows][C] with a row pitch in elements (multiple of 8); parameters, statistics and their gradients are fp32.
 * ===================================================================================================== */

/* Batched GEMM  Y[z][m][n] = sum_k A[z][m][k] * W[z][n][k] (+ bias[n]) (+ resid[z][m][n]),  z = b*bh + j,
 * operand z at base + b*s?_b + j*s?_h (elements).  nbatch = 1, bh = 1 is a plain nn.Linear forward
 * (y = x W^T + b: attention.py:193,195,482; common.py:19-21) or its data gradient (W = weight^T operand).
 * In attention: scores = q k^T (attention.py:355) and attn @ v (:379) per (batch, head). */
int sf_bgemm(int64_t M, int32_t N, int32_t K, const void* A, int32_t lda, const void* W, int32_t ldw, const float* bias,
             const void* resid, int32_t ldr, void* Y, int32_t ldy, int32_t nbatch, int32_t bh, int64_t sa_b, int64_t sa_h,
             int64_t sw_b, int64_t sw_h, int64_t sy_b, int64_t sy_h, int64_t sr_b, int64_t sr_h, int32_t resid_row0,
             float alpha, sf_stream_t stream);
/* alpha scales the products before bias / residual (0 = 1): the 1/N normalisation of the Nonlocal "dot_product"
 * affinity (nonlocal_helper.py:130-132). */
/* resid_row0: the residual is added to rows m >= resid_row0 only (residual pooling skips the cls row,
 * attention.py:381-385).  N need not be a multiple of 8 when ldy covers N rounded up to 8 (pad columns <- 0). */
/* fp32 side rows of a token residual stream (round 4).  MultiScaleBlock adds two branch outputs per block to the stream
 * (attention.py:500-510: x = x_res + drop_path(x_block); x = x + drop_path(x_mlp)); the reference keeps that stream in fp32
 * (autocast leaves additions alone).  Rows m with m % period == 0 (period = tokens per sample: the class-token rows; period 1:
 * every row) carry an fp32 copy at side row m / period, pitch ld floats.  `in`: residual operand rows (NULL: the 16-bit
 * residual operand is used for them too), `out`: the sums.  The 16-bit output row is round(out row). */
typedef struct sf_rows32 {
    const float* in;
    float* out;
    int32_t ld, period;
} sf_rows32;
/* nn.Linear forward with the residual addition of the stream in its epilogue: Y = A W^T + bias + resid, side rows summed from
 * the fp32 accumulators (attention.py:393 proj, common.py:31 fc2 followed by attention.py:502 / :510). */
int sf_gemm_rows32(int64_t M, int32_t N, int32_t K, const void* A, int32_t lda, const void* W, int32_t ldw, const float* bias,
                   const void* resid, int32_t ldr, void* Y, int32_t ldy, const sf_rows32* side, sf_stream_t stream);
/* Batched "TN" GEMM  Out[z][r][c] = scale * sum_m P[z][m][r] * X[z][m][c]  (fp16 out): the attention gradients
 * dV = P^T dO and dK = dS^T q (autograd of attention.py:355,379). */
int sf_bgemm_tn(int64_t M, int32_t R, int32_t Kc, const void* P, int32_t ldp, const void* X, int32_t ldx, void* Out,
                int32_t ldo, float scale, int32_t nbatch, int32_t bh, int64_t sp_b, int64_t sp_h, int64_t sx_b,
                int64_t sx_h, int64_t so_b, int64_t so_h, sf_stream_t stream);

/* nn.LayerNorm(C, eps) over the last dim (attention.py:240-268, 428, 456; video_model_builder.py:1032) */
int sf_layernorm_fwd(int64_t M, int32_t C, const void* x, int32_t ldx, const float* gamma, const float* beta, float eps,
                     void* y, int32_t ldy, float* mean, float* rstd, sf_stream_t stream);
/* same; rows that have an fp32 side copy (side->in) are normalised from it (norm1 / norm2 / the final norm reading the stream) */
int sf_layernorm_fwd_rows32(int64_t M, int32_t C, const void* x, int32_t ldx, const float* gamma, const float* beta, float eps,
                            void* y, int32_t ldy, float* mean, float* rstd, const sf_rows32* side, sf_stream_t stream);
int sf_layernorm_bwd_blocks(int64_t M, int32_t C);   /* rows of `part` */
/* dx = LN backward (+ resid); part[blk][0][c] = sum dy*xhat, part[blk][1][c] = sum dy -> sf_colsum_finalize */
int sf_layernorm_bwd(int64_t M, int32_t C, const void* dy, int32_t lddy, const void* x, int32_t ldx, const float* gamma,
                     const float* mean, const float* rstd, const void* resid, int32_t ldr, void* dx, int32_t lddx,
                     float* part, sf_stream_t stream);
/* same, and part[blk][2][c] = sum of resid, part[blk][3][c] = sum of the stored dx (part is [blocks][4][C]): the bias gradients of
 * the Linear layers on either side of the LayerNorm -- in MultiScaleBlock (attention.py:491-514) mlp.fc2.bias from
 * resid = d(block output) and attn.proj.bias from dx -- without a column-sum pass of their own */
int sf_layernorm_bwd_sums(int64_t M, int32_t C, const void* dy, int32_t lddy, const void* x, int32_t ldx, const float* gamma,
                          const float* mean, const float* rstd, const void* resid, int32_t ldr, void* dx, int32_t lddx,
                          float* part, sf_stream_t stream);
/* column sums of an [M][C] tensor (bias gradients): part[blk][0][c] */
int sf_colsum_blocks(int64_t M, int32_t C);
int sf_colsum(int64_t M, int32_t C, const void* x, int32_t ldx, float* part, sf_stream_t stream);
/* out0[c % fold] (+)= scale * sum_blk part[blk][0][c], out1 likewise from part[blk][1][c] (either may be NULL);
 * `part` is scratch (folded in place) */
int sf_colsum_finalize(float* part, int32_t nblk, int32_t C, int32_t fold, float* out0, float* out1, float scale,
                       int accumulate, sf_stream_t stream);
/* n finalizes in one launch (the backward of a MultiScaleBlock ends in ~9: LayerNorm affine gradients, bias gradients;
 * attention.py:428-514).  `items` is a HOST array, passed to the kernel by value; two items must not share an output; tables of
 * more than 2048 partial rows go through sf_colsum_finalize. */
typedef struct sf_colfin_item {
    float* part;
    int32_t nblk, C, fold;
    float* out0;
    float* out1;
    float scale;
    int32_t accumulate;
    int32_t row_stride;   /* table rows of [2][C] floats between two partial rows (0 / 1: dense; 2: the pairs of a [blk][4][C] table) */
} sf_colfin_item;
int sf_colsum_finalize_batch(const sf_colfin_item* items, int32_t n, sf_stream_t stream);
/* out[i] (+)= scale * sum_b part[b*row_len + offset + i] */
int sf_rows_sum(const float* part, int32_t nblk, int64_t row_len, int64_t offset, int32_t n, float* out, float scale,
                int accumulate, sf_stream_t stream);
/* nn.GELU (exact erf; common.py:20) on contiguous arrays of n elements (n % 8 == 0) */
int sf_gelu_fwd(int64_t n, const void* h, void* a, sf_stream_t stream);
int sf_gelu_bwd(int64_t n, const void* h, const void* da, void* dh, sf_stream_t stream);

/* Depthwise Conv3d(C, C, k, stride, padding, groups = C) on channels-last rows; C may be heads*Cw with one weight
 * [Cw][taps] shared by the heads (MViT pool_q/k/v, attention.py:227-266); cls != 0: token tensors whose cls row is
 * routed around the convolution (attention.py:24-36).  Also X3DTransform.b (resnet_helper.py:214-224) and the
 * X3D stem's (5,1,1) temporal conv (stem_helper.py:267-275).  ldx / ldy = pitches of input / output rows.
 * Any kernel extent with kT*kH*kW*Cw <= 12288 (LDS weight image): 3x3x3 / (5,1,1) take the W-blocked stencils, wider planes
 * (MViTv1's stride+1 pooling kernels 1x5x5, 1x9x9) the generic ones, their weight gradient in chunks of 9 taps. */
typedef struct sf_dw_desc {
    int32_t N, C, Cw, cls;
    int32_t Ti, Hi, Wi, To, Ho, Wo;
    int32_t kT, kH, kW, sT, sH, sW, pT, pH, pW;
    int32_t ldx, ldy;
    int32_t Cwreal;   /* rows of the fp32 weight (0 = Cw); channels [Cwreal, Cw) are zero padding (X3D widths 54, 108) */
} sf_dw_desc;
int sf_dwconv_fwd_blocks(const sf_dw_desc* d);       /* rows of stat_part */
/* rows of the statistics table of sf_dwconv_fwd that belong to one sample when the table is sample-major (rows [n * r, (n + 1) * r)
 * = sample n), else 0: per-sample channel sums (SE squeeze, operators.py:38-45) can then be read from the table (ABI 23) */
int sf_dwconv_fwd_sample_rows(const sf_dw_desc* d);
/* stat_part (optional): [blocks][2][C] per-block sum / sum of squares of the outputs (BatchNorm statistics) */
int sf_dwconv_fwd(const sf_dw_desc* d, const void* x, const float* w, void* y, float* stat_part, sf_stream_t stream);
int sf_dwconv_dgrad(const sf_dw_desc* d, const void* dy, const float* w, void* dx, sf_stream_t stream);
/* ... that also leaves the per-workgroup column sums of dx (cls row included) in slot 0 of sum_part[sf_dwconv_dgrad_sum_rows(d)][2][C]
 * (slot 1 unspecified); rows == 0: the kernel this geometry takes cannot.  MViT's qkv bias gradient = the column sums of d(qkv),
 * which the three pooling data gradients write (attention.py:318-330) (ABI 23) */
int sf_dwconv_dgrad_sum_rows(const sf_dw_desc* d);
int sf_dwconv_dgrad_sums(const sf_dw_desc* d, const void* dy, const float* w, void* dx, float* sum_part, sf_stream_t stream);
int64_t sf_dwconv_wgrad_workspace(const sf_dw_desc* d);
int sf_dwconv_wgrad(const sf_dw_desc* d, const void* x, const void* dy, float* dw, float out_scale, int zero_first,
                    void* workspace, int64_t workspace_bytes, sf_stream_t stream);
/* PAIR forms (ABI 23): two depthwise convolutions of the SAME geometry d on two tensors (x, x2) with separate weights in one launch
 * per direction -- MViT pool_k / pool_v of a block (attention.py:227-266).  sf_dwconv_pair_ok(d) == 1 when the geometry is taken
 * (3x3x3 / padding 1 plane sweeps in all three directions, C % 32 == 0); results equal two single calls bit for bit.
 * sf_dwconv_wgrad_pair needs 2 x sf_dwconv_wgrad_workspace(d) bytes. */
int sf_dwconv_pair_ok(const sf_dw_desc* d);
int sf_dwconv_fwd_pair(const sf_dw_desc* d, const void* x, const void* x2, const float* w, const float* w2, void* y, void* y2,
                       sf_stream_t stream);
int sf_dwconv_dgrad_pair(const sf_dw_desc* d, const void* dy, const void* dy2, const float* w, const float* w2, void* dx, void* dx2,
                         sf_stream_t stream);
int sf_dwconv_wgrad_pair(const sf_dw_desc* d, const void* x, const void* x2, const void* dy, const void* dy2, float* dw, float* dw2,
                         float out_scale, int zero_first, int zero_first2, void* workspace, int64_t workspace_bytes,
                         sf_stream_t stream);

/* Pooled attention (attention.py:354-385).  Tokens are [B][N][heads*D]; scores [B][heads][Nq][lds]. */
typedef struct sf_attn_desc {
    int32_t B, heads, D, cls;
    int32_t Nq, qT, qH, qW;        /* Nq = cls + qT*qH*qW */
    int32_t Nk, kT, kH, kW;        /* Nk = cls + kT*kH*kW */
    int32_t rows_h, rows_w, rows_t; /* rows of rel_pos_h / rel_pos_w / rel_pos_t */
} sf_attn_desc;
/* Decomposed relative positions (cal_rel_pos_spatial / cal_rel_pos_temporal, attention.py:64-147).  The contractions
 * with the tables run as GEMMs over the concatenated table Tab = [rel_pos_h; rel_pos_w; rel_pos_t]:
 *   forward   G = q_unscaled Tab^T (sf_bgemm), rq[(b,q,head)][kH+kW+kT] = G[row][column of table row j]   (gather)
 *   backward  E[row][column of table row j] = drq[row][j] (scatter, zero elsewhere); dq += E Tab (sf_bgemm);
 *             dTab = E^T q (sf_conv_wgrad on the 1x1x1 geometry).
 * idx_h [qH][kH], idx_w [qW][kW], idx_t [qT][kT] are the reference's dist_* tables as int32; cls rows get zeros. */
int sf_relpos_gather(const sf_attn_desc* d, const void* G, int32_t ldg, const int32_t* idx_h, const int32_t* idx_w,
                     const int32_t* idx_t, float* rq, sf_stream_t stream);
int sf_relpos_scatter(const sf_attn_desc* d, const float* drq, const int32_t* idx_h, const int32_t* idx_w,
                      const int32_t* idx_t, void* E, int32_t lde, sf_stream_t stream);
/* The concatenated table Tab = [rel_pos_h; rel_pos_w; rel_pos_t] (fp32 parameters, D columns) as 16-bit GEMM operands:
 * t16 [TRp][D] (rows beyond the tables zero, TRp % 8 == 0) and t16t = t16^T [D][TRp]; and back: rows of dtab [TRp][D] fp32
 * into the three parameter gradients (acc_*: accumulate instead of overwrite). */
int sf_relpos_pack(const float* rel_h, const float* rel_w, const float* rel_t, int32_t rows_h, int32_t rows_w, int32_t rows_t,
                   int32_t D, int32_t TRp, void* t16, void* t16t, sf_stream_t stream);
int sf_relpos_unpack(const float* dtab, int32_t rows_h, int32_t rows_w, int32_t rows_t, int32_t D, float* grad_h, float* grad_w,
                     float* grad_t, int32_t acc_h, int32_t acc_w, int32_t acc_t, sf_stream_t stream);
/* in place: s <- softmax_k(scale*s + bias), bias from rq (NULL = none); pad columns [Nk, lds) <- 0 */
int sf_softmax_fwd(const sf_attn_desc* d, void* s, int32_t lds, float scale, const float* rq, sf_stream_t stream);
/* in place: dp <- scale * P*(dp - sum_k P*dp); drq (optional) <- per-(kh|kw|kt) sums of the unscaled dS */
int sf_softmax_bwd(const sf_attn_desc* d, void* dp, const void* prob, int32_t lds, float scale, float* drq,
                   sf_stream_t stream);
/* Fused attention core -- replaces attention.py:355-385 (scores, decomposed rel-pos bias, softmax, attn @ v, residual
 * pooling) without materialising the [B, heads, Nq, Nk] score tensors (online softmax, fp32 statistics).
 *   o[b][q][head*D + :] = softmax_k(scale * q.k + bias(q, k)) v  (+ q on the rows >= cls when `residual`)
 * q, o, dq: [B][Nq][.] rows of pitch ldq / ldo / lddq; k, v, dk, dv: [B][Nk][.] rows of pitch ldk / lddk; head h occupies
 * columns [h*D, (h+1)*D), D in {32, 64, 96, 128}.  rq (optional) is sf_relpos_gather's output
 * [(b*Nq + q)*heads + head][kH + kW + kT] fp32 and `onehot` the constant fp16 matrix [roundup(Nk, 32)][64] with
 * onehot[key][j] = 1 for j in {kh, kH + kw, kH + kW + kt} of a non-cls key (zero rows for the cls key and the padding):
 * bias(q, key) = sum_j rq[q][j] onehot[key][j] runs on the matrix cores.  lse / delta are
 * [(b*heads + head)*Nq + q] fp32 scratch (caller-owned) that the forward / backward fill.  sf_attn_bwd returns dq (incl.
 * the residual's dout on the rows >= cls), dk, dv and drq (the bias gradient, input of sf_relpos_scatter); `workspace`
 * (>= sf_attn_bwd_workspace(d) bytes, may be 0) holds the dK/dV partials of the query splits. */
int sf_attn_fwd(const sf_attn_desc* d, const void* q, int32_t ldq, const void* k, const void* v, int32_t ldk, float scale,
                const float* rq, const void* onehot, int32_t residual, void* o, int32_t ldo, float* lse,
                sf_stream_t stream);
int64_t sf_attn_bwd_workspace(const sf_attn_desc* d);
int sf_attn_bwd(const sf_attn_desc* d, const void* q, int32_t ldq, const void* k, const void* v, int32_t ldk, float scale,
                const float* rq, const void* onehot, int32_t residual, const void* o, const void* dout, int32_t ldo,
                const float* lse, float* delta, void* dq, int32_t lddq, void* dk, void* dv, int32_t lddk, float* drq,
                void* workspace, int64_t workspace_bytes, sf_stream_t stream);
/* RoI head -- replaces head_helper.py:85-97 / 116-133 (ResNetRoIHead): AvgPool3d([T,1,1]) then ROIAlign(res x res,
 * spatial_scale, sampling_ratio 0, aligned) fused with MaxPool2d(res).
 *   sf_tmean_fwd: m[b][hw][c] = mean_t x[b][t][hw][c]   (x channels-last fp16 rows of pitch ldx, m fp32 [B*HW][C])
 *   sf_roi_align_max_fwd: out[r][col0 + c] = max over the res*res bins of ROIAlign(m, rois[r]) (rois [R][5] fp32 =
 *       batch index, x1, y1, x2, y2 in input pixels); argmax [R][C] uint8 records the winning bin
 *   sf_roi_align_max_bwd: dm (pre-zeroed by the caller, fp32) += the gradient routed to the arg-max bin's bilinear samples
 *       (fp32 atomics: overlapping boxes); sf_tmean_bwd: dx[b][t][hw][c] = dm[b][hw][c] / T.
 * ROIAlign is detectron2.layers.ROIAlign in the reference (not vendored): see oracle/video_ref.py:roi_align. */
int sf_tmean_fwd(int32_t B, int32_t T, int64_t HW, int32_t C, const void* x, int32_t ldx, float* m, sf_stream_t stream);
int sf_tmean_bwd(int32_t B, int32_t T, int64_t HW, int32_t C, const float* dm, void* dx, int32_t lddx, sf_stream_t stream);
int sf_roi_align_max_fwd(int32_t R, int32_t B, int32_t H, int32_t W, int32_t C, int32_t res, float scale, int32_t aligned,
                         const float* m, const float* rois, float* out, int32_t ldo, int32_t col0, void* argmax,
                         sf_stream_t stream);
int sf_roi_align_max_bwd(int32_t R, int32_t B, int32_t H, int32_t W, int32_t C, int32_t res, float scale, int32_t aligned,
                         const float* rois, const float* dout, int32_t lddo, int32_t col0, const void* argmax, float* dm,
                         sf_stream_t stream);
/* Linear layers of the Mlp with the GELU fused into the GEMM epilogue (slowfast/models/common.py:25-34):
 *   mode 1 (fc1 forward):   Y = A W^T + bias,  aux = gelu(Y)        (Y is kept for the backward)
 *   mode 2 (fc2 data grad):  Y = (A W^T) * gelu'(aux)                (aux = the saved pre-activation)
 * A [M][K], W [N][K], Y / aux [M][N] fp16, row pitches in elements. */
int sf_gemm_act(int64_t M, int32_t N, int32_t K, const void* A, int32_t lda, const void* W, int32_t ldw, const float* bias,
                void* Y, int32_t ldy, int32_t mode, void* aux, int32_t ldaux, sf_stream_t stream);
/* sf_gemm_act + the column sums of the tile it stores (round 3): colsum_part[row][2][N] fp32, slot 0 of every row = the sum of
 * Y over the rows of one M tile (slot 1 unused), *colsum_rows (HOST pointer) = rows written.  With mode 2 (Y = d(loss)/d(fc1
 * output)) the sums are the bias gradient of the Mlp's fc1 (common.py:25-34) once folded by sf_colsum_finalize -- the
 * separate sf_colsum pass over the widest gradient tensor of every block goes away.  colsum_part holds ceil(M / 128) rows. */
int sf_gemm_act_colsum(int64_t M, int32_t N, int32_t K, const void* A, int32_t lda, const void* W, int32_t ldw,
                       const float* bias, void* Y, int32_t ldy, int32_t mode, void* aux, int32_t ldaux,
                       float* colsum_part, int32_t colsum_part_rows, int32_t* colsum_rows, sf_stream_t stream);
/* Input side -- replaces tensor_normalize (slowfast/datasets/utils.py:278-297), the THWC -> CTHW
 * permute (datasets/kinetics.py:375-408) and pack_pathway_output (datasets/utils.py:78-111) for one pathway:
 *   out[n][to][h][w][c] = ((frames[n][t_index[to]][h][w][s] / 255) - mean[s]) / std[s]   (s = c, or 2 - c when `reverse`),
 * frames uint8 [N][Tin][H][W][3] on the device, out fp16 [N][Tout][H][W][4] (4th channel zero) = the buffer the stems read
 * as W pairs; t_index [Tout] int32 on the device (NULL = identity; the Slow pathway passes linspace(0, T-1, T/alpha)). */
int sf_pack_clip_u8(const void* frames, int32_t N, int32_t Tin, int32_t H, int32_t W, const int32_t* t_index, int32_t Tout,
                    float mean0, float mean1, float mean2, float std0, float std1, float std2, int32_t reverse, void* out,
                    sf_stream_t stream);
/* MixUp / CutMix of the batch (ABI 25) -- replaces mixup_fn(inputs[0], labels) of the training loop (tools/train_net.py:109-111,
 * slowfast/datasets/mixup.py).  Sample i is mixed with sample B-1-i (x.flip(0)).  lam and one_minus_lam are the host's doubles
 * lam and 1.0 - lam, EACH rounded to float (1.0f - (float)lam is a different number); every blend is
 * fl(fl(a * lam) + fl(b * one_minus_lam)) with no contraction, bit for bit x.mul_(lam).add_(x.flip(0).mul_(1 - lam)).
 * Kernel launches only; scalars travel as kernel arguments (the calls run eagerly, outside a captured graph).
 *
 * sf_mix_clip_f32: dense fp32 clip [B][C][T][H][W].  dst == src mixes in place, any other dst must not overlap src.
 *   mode 0 (mixup):  dst[i] = src[i] * lam + src[B-1-i] * one_minus_lam; the box is ignored.  The middle sample of an odd batch
 *                    is mixed with itself (not the identity).
 *   mode 1 (cutmix): rows yl..yh-1, columns xl..xh-1 of every (c, t) plane of dst[i] come from src[B-1-i]; everything else is
 *                    src[i] (in place: untouched; an empty box launches nothing).  lam / one_minus_lam are ignored. */
int sf_mix_clip_f32(const float* src, float* dst, int32_t B, int32_t C, int32_t T, int32_t H, int32_t W, int32_t mode,
                    float lam, float one_minus_lam, int32_t yl, int32_t yh, int32_t xl, int32_t xh, sf_stream_t stream);
/* sf_pack_clip_u8 with the batch mixed in fp32 BETWEEN the normalisation and the rounding to the 16-bit storage type (mixing
 * the packed buffer afterwards would round twice): frame n and -- for mixup, or inside the cutmix box -- frame N-1-n are
 * normalised as sf_pack_clip_u8 does, mixed as sf_mix_clip_f32 does, rounded once.  Arguments of sf_pack_clip_u8 + the mix. */
int sf_pack_clip_u8_mix(const void* frames, int32_t N, int32_t Tin, int32_t H, int32_t W, const int32_t* t_index, int32_t Tout,
                        float mean0, float mean1, float mean2, float std0, float std1, float std2, int32_t reverse, void* out,
                        int32_t mode, float lam, float one_minus_lam, int32_t yl, int32_t yh, int32_t xl, int32_t xh,
                        sf_stream_t stream);
/* mixup_target() (datasets/mixup.py:40-64) in one launch: out[i][k] = v(i, k) * lam + v(B-1-i, k) * one_minus_lam, where
 * v(i, k) = on_value when k == labels[i] and off_value otherwise (floats rounded from the host's doubles 1 - s + s / K and
 * s / K, s = label smoothing).  labels int64 [B] on the device, out fp32 [B][K] (may be a step's static label buffer). */
int sf_mix_targets(const int64_t* labels, int32_t B, int32_t K, float on_value, float off_value, float lam, float one_minus_lam,
                   float* out, sf_stream_t stream);
/* Random erasing of the batch (ABI 26) -- replaces RandomErasing.__call__ on the normalised host clip
 * (slowfast/datasets/random_erasing.py, called at datasets/kinetics.py:437-447 before pack_pathway_output).  The boxes are drawn
 * on the host and arrive as one table of int32 words, given twice: table_host is validated and sizes the grid, table_dev (the
 * same words in device memory) is what the kernels read.  Layout: nrows rows of 12 words
 *   n, t0, t1, top, left, h, w, key_lo, key_hi, colour word offset, end, 0
 * (sample, frames [t0, t1), rows [top, top + h), columns [left, left + w), Philox key, offset of the row's (t1 - t0) x C colours
 * from the table start, first row of the next sample), the rows of a sample adjacent in draw order and samples ascending; then
 * N + 1 words first_row[n]; then the colours as float bits.  Where rows of a sample overlap the LAST one decides an element.
 * mode 0 (const) writes 0.0f, 1 (rand) the row's colour of (frame, channel), 2 (pixel) a standard normal that depends on
 * (key, idx) only, idx = ((c * T + t) * H + y) * W + x: Philox4x32-10 with the row's key and counter (idx >> 2, 0, 0, 0), whose
 * outputs r0..r3 serve elements idx & 3 = 0..3 through Box-Muller on u = r * 2^-32 + 2^-33:
 * z0 = sqrt(-2 ln u(r0)) sin(2 pi u(r1)), z1 = sqrt(-2 ln u(r0)) cos(2 pi u(r1)), z2 / z3 likewise from (r2, r3).
 * Kernel launches only.
 *
 * sf_erase_clip_f32: dense fp32 clip [N][C][T][H][W].  dst == src erases in place (only erased elements are written, nothing is
 *   read, a table without boxes launches nothing); any other dst must not overlap src and receives the whole erased clip. */
int sf_erase_clip_f32(const float* src, float* dst, int32_t N, int32_t C, int32_t T, int32_t H, int32_t W, int32_t mode,
                      const int32_t* table_host, const int32_t* table_dev, int32_t nrows, int32_t table_words,
                      sf_stream_t stream);
/* sf_pack_clip_u8 with erasing, then MixUp / CutMix, in fp32 BETWEEN the normalisation and the rounding to the 16-bit storage
 * type: frame n and its mixing partner N-1-n are each normalised as sf_pack_clip_u8 does and erased with their own rows
 * (C = 3, T = Tin, c and t are the SOURCE channel and frame: before the channel reversal and t_index), blended as
 * sf_pack_clip_u8_mix does, rounded once.  table_host == table_dev == NULL erases nothing; mix_mode -1 mixes nothing, 0 / 1 as
 * the mode of sf_mix_clip_f32. */
int sf_pack_clip_u8_aug(const void* frames, int32_t N, int32_t Tin, int32_t H, int32_t W, const int32_t* t_index, int32_t Tout,
                        float mean0, float mean1, float mean2, float std0, float std1, float std2, int32_t reverse, void* out,
                        int32_t erase_mode, const int32_t* table_host, const int32_t* table_dev, int32_t nrows,
                        int32_t table_words, int32_t mix_mode, float lam, float one_minus_lam, int32_t yl, int32_t yh,
                        int32_t xl, int32_t xh, sf_stream_t stream);
/* Spatial sampling of the batch (ABI 27) -- replaces utils.spatial_sampling on the normalised host clip
 * (slowfast/datasets/utils.py:114-185, called at datasets/kinetics.py:410-435: short-side scale jitter or random resized crop,
 * i.e. a bilinear F.interpolate of every frame, then a crop and a horizontal flip).  frames is uint8 [N][T][Hs][Ws][3], every
 * sample padded to the batch's largest frame.  The draw arrives as one table of int32 words, given twice as the erase table is:
 * crop_host is validated, crop_dev (the same words in device memory) is what the kernels read.  Layout: N rows of 12 words
 *   src_h, src_w, win_y, win_x, win_h, win_w, res_h, res_w, off_y, off_x, flip, 0
 * (valid frame size; the source window that is resized; the size it is resized to; the S x S crop inside the resized image;
 * horizontal flip).  Every row must satisfy 0 < src <= (Hs, Ws), the window inside the valid size with positive lengths,
 * 0 <= off <= res - S, flip 0 / 1, all sizes below 65536.  Output pixel (oy, ox), per axis in fp32, in this order:
 *   r = o + off (x axis: o = S-1-ox when flip);  sc = (float)win_len / (float)res_len;  f = max(sc * (r + 0.5f) - 0.5f, 0);
 *   i0 = (int)f;  l1 = f - i0;  l0 = 1 - l1;  i1 = i0 + (i0 < win_len - 1)
 * with taps at win + i0 / i1 (i1 clamps to the WINDOW, not the frame), each normalised as sf_pack_clip_u8 does, then
 * l0y * (l0x * a + l1x * b) + l1y * (l0x * c + l1x * d), no contraction.  win_len == res_len gives the normalised source
 * pixel bit for bit.  Kernel launches only.
 *
 * sf_sample_clip_u8: out is the dense fp32 clip [N][3][T][S][S] (channels in mean order) that sf_erase_clip_f32 and
 *   sf_mix_clip_f32 take in place. */
int sf_sample_clip_u8(const void* frames, int32_t N, int32_t T, int32_t Hs, int32_t Ws, const int32_t* crop_host,
                      const int32_t* crop_dev, int32_t S, float mean0, float mean1, float mean2, float std0, float std1,
                      float std2, float* out, sf_stream_t stream);
/* sf_pack_clip_u8_aug with every sample -- and its mixing partner N-1-n, through ITS row -- sampled first: sample, erase, mix
 * in fp32, one rounding to the 16-bit storage type into the N,Tout,S,S,4 W-pair buffer.  S must be even.  The erase table is
 * the one of sf_pack_clip_u8_aug for the CROPPED clip (C = 3, T = Tin, H = W = S), the cutmix box lies in the S x S plane. */
int sf_pack_clip_u8_sample(const void* frames, int32_t N, int32_t Tin, int32_t Hs, int32_t Ws, const int32_t* t_index,
                           int32_t Tout, float mean0, float mean1, float mean2, float std0, float std1, float std2,
                           int32_t reverse, void* out, const int32_t* crop_host, const int32_t* crop_dev, int32_t S,
                           int32_t erase_mode, const int32_t* table_host, const int32_t* table_dev, int32_t nrows,
                           int32_t table_words, int32_t mix_mode, float lam, float one_minus_lam, int32_t yl, int32_t yh,
                           int32_t xl, int32_t xh, sf_stream_t stream);
/* Colour augmentation of the AVA batch on the device (ABI 28) -- replaces transform.color_jitter, lighting_jitter and
 * color_normalization and the BGR -> RGB reordering of Ava._images_and_boxes_preprocessing (slowfast/datasets/ava_dataset.py:306-333).
 * clip is the dense fp32 [N][3][T][HW] clip sf_sample_clip_u8 writes with mean 0 and std 1: the [0, 1] image in the frames' byte
 * order (BGR for AVA).  The draw arrives as one table of 32-bit words, given twice as the crop table is: table_host is validated
 * and decides what is launched, table_dev is what the kernels read.  Layout: N rows of 16 words
 *   op of slot 0, 1, 2 (0 brightness, 1 contrast, 2 saturation, -1 none; no op twice), 0,
 *   alpha and 1 - alpha of slot 0, 1, 2 (float bits, each the host's double rounded once),
 *   the addition to input channel 0, 1, 2 (float bits), 0, 0, 0
 * Per pixel, fp32 without contraction, in slot order: brightness v * a; contrast v * a + m * (1 - a) with m the mean over the
 * frame of gray = (0.299f * v[2] + 0.587f * v[1]) + 0.114f * v[0] as the values stand at that slot; saturation
 * v * a + gray(v) * (1 - a); then v + add[c], (v - mean[c]) / std[c], and output channel c = input channel (reverse ? 2 - c : c).
 * In place.  Kernel launches only, no atomics: two calls give the same bits.
 *
 * sf_color_frame_means_f32: means[n * T + t] for the frames of every sample whose row has a contrast slot (the others are left
 *   untouched; no such row: nothing is launched).  A frame is reduced in sf_color_chunks(HW) chunks of a fixed number of
 *   pixels; partials needs N * T * sf_color_chunks(HW) floats.  sf_color_sum_depth(): the longest chain of additions a term of a
 *   frame's sum passes through (what an error bound of the mean is derived from).
 * sf_color_clip_f32: the streaming pass; means may be NULL when no row has a contrast slot. */
int sf_color_chunks(int64_t HW);
int sf_color_sum_depth(void);
int sf_color_frame_means_f32(const float* clip, int32_t N, int32_t T, int64_t HW, const int32_t* table_host,
                             const int32_t* table_dev, float* partials, float* means, sf_stream_t stream);
int sf_color_clip_f32(float* clip, int32_t N, int32_t T, int64_t HW, const int32_t* table_host, const int32_t* table_dev,
                      const float* means, float mean0, float mean1, float mean2, float std0, float std1, float std2,
                      int32_t reverse, sf_stream_t stream);
/* RandAugment of the batch on the device (ABI 29) -- replaces the PIL loop of rand_augment_transform(AUG.AA_TYPE) on the decoded
 * frames (slowfast/datasets/kinetics.py:389-400, datasets/rand_augment.py).  src / dst are dense uint8 [N][T][Hs][Ws][3] buffers
 * (RGB byte order, every sample padded to the batch's largest frame); one call is one LAYER of the draw.  The layer's table is N
 * rows of 20 words, given twice as the crop table is: table_host is validated and decides what is launched, table_dev is what
 * the kernels read.  Layout of a row:
 *   class (0 copy, 1 lookup table, 2 Color, 3 Sharpness, 4 affine gather), op (0 AutoContrast, 1 Equalize, 2 Invert, 3 Rotate,
 *   4 Posterize, 5 Solarize, 6 SolarizeAdd, 7 Color, 8 Contrast, 9 Brightness, 10 Sharpness, 11 ShearX, 12 ShearY,
 *   13 TranslateXRel, 14 TranslateYRel), the integer argument (bits 0 .. 8, threshold 0 .. 256, added value 0 .. 255), the blend
 *   factor (float bits), the filter (0 bilinear, 1 bicubic), the valid size h, w of the sample's frames, 0, and the six
 *   coefficients of PIL's inverse affine matrix as fp64 (low word, high word) pairs, computed by the caller.
 * Inside a sample's h x w region the bytes are PIL's, bit for bit (the arithmetic: csrc/sf_randaug.h); outside it dst is a copy
 * of src.  Kernel launches only; the only atomics are integer adds: two calls give the same bits.
 *
 * sf_randaug_chunk(): the pixels of a frame one workgroup counts / streams.
 * sf_randaug_hist_u8: hist[(n * T + t) * 1024 + c * 256 + v] = how many valid pixels of frame (n, t) have value v in channel c
 *   (R, G, B, L = (R*19595 + G*38470 + B*7471 + 0x8000) >> 16), for the samples whose row is AutoContrast, Equalize or Contrast;
 *   the others are left untouched, and with no such row nothing is launched.
 * sf_randaug_layer_u8: builds the lookup tables of the table rows into lut (N * T * 768 bytes; no such row: not launched, lut
 *   may be NULL) and streams the layer, src -> dst.  hist may be NULL when no row needs a histogram. */
int sf_randaug_chunk(void);
int sf_randaug_hist_u8(const void* src, int32_t N, int32_t T, int32_t Hs, int32_t Ws, const int32_t* table_host,
                       const int32_t* table_dev, int32_t* hist, sf_stream_t stream);
int sf_randaug_layer_u8(const void* src, void* dst, int32_t N, int32_t T, int32_t Hs, int32_t Ws, const int32_t* table_host,
                        const int32_t* table_dev, const int32_t* hist, void* lut, sf_stream_t stream);
/* SSL colour augmentation of the batch on the device (ABI 33) -- replaces transform.color_jitter_video_ssl
 * (slowfast/datasets/transform.py:1073-1121, GaussianBlur at :1145-1157; applied at datasets/kinetics.py:378-387): torchvision's
 * ColorJitter (brightness, contrast, saturation, hue in a drawn order), RandomGrayscale and PIL's Gaussian blur on ONE image per
 * clip, the (T * h) x w stack of its frames.  src / dst are dense uint8 [N][T][Hs][Ws][3] buffers as above.  The draw is the
 * caller's: ONE table of N rows of 16 int32 words, given twice (table_host is validated and decides what is launched; table_dev,
 * the same words in device memory, is what the kernels read).  A row holds the flags (1 jitter, 2 grey, 4 blur, 8 grey before
 * the jitter), the op order (four 4-bit fields: 0 brightness, 1 contrast, 2 saturation, 3 hue, 7 nothing), the three blend
 * factors (float bits), the hue shift 0 .. 255, the box blur's integer radius (0 or 1) and its two 8.24 fixed-point weights,
 * h, w, and five zeros (csrc/sf_sslcolor.h).  Inside a sample's h x w region the bytes are PIL's, bit for bit; outside it the
 * streaming pass copies src and the blur passes write nothing.  Kernel launches only; the only atomics are integer adds.
 *
 * sf_sslcolor_hist_u8: hist[n * 256 + v] = how many valid pixels of clip n have L = v after the ops drawn before contrast, for the
 *   clips that drew contrast; the others are left untouched, and with no such row nothing is launched.
 * sf_sslcolor_stream_u8: the jitter and grey of every row, src -> dst; dst may be src itself (in place: rows without jitter and
 *   grey are skipped, and nothing is launched when there is no other row) or a buffer that does not overlap it (rows without
 *   them are copied).  hist may be NULL when no row drew contrast.
 * sf_sslcolor_blur_rows_u8 / _cols_u8: the three box iterations along the rows / the stacked columns of the clips with the blur
 *   flag, src -> dst (another buffer), valid region only; no such row: nothing is launched.  Ws <= 4096. */
int sf_sslcolor_hist_u8(const void* src, int32_t N, int32_t T, int32_t Hs, int32_t Ws, const int32_t* table_host,
                        const int32_t* table_dev, int32_t* hist, sf_stream_t stream);
int sf_sslcolor_stream_u8(const void* src, void* dst, int32_t N, int32_t T, int32_t Hs, int32_t Ws, const int32_t* table_host,
                          const int32_t* table_dev, const int32_t* hist, sf_stream_t stream);
int sf_sslcolor_blur_rows_u8(const void* src, void* dst, int32_t N, int32_t T, int32_t Hs, int32_t Ws, const int32_t* table_host,
                             const int32_t* table_dev, sf_stream_t stream);
int sf_sslcolor_blur_cols_u8(const void* src, void* dst, int32_t N, int32_t T, int32_t Hs, int32_t Ws, const int32_t* table_host,
                             const int32_t* table_dev, sf_stream_t stream);
/* Stochastic depth -- replaces drop_path() (slowfast/models/common.py:46-59) at the two residual additions of
 * MultiScaleBlock (attention.py:500-510): y[m] = (resid ? resid[m] : 0) + scale[m / rows_per_sample] * x[m], with
 * scale[b] = floor(keep_prob + u_b) / keep_prob sampled by the caller.  Rows are fp16 [M][C], C % 8 == 0. */
int sf_row_scale_add(const void* x, int32_t ldx, const float* scale, int64_t rows_per_sample, const void* resid,
                     int32_t ldr, void* y, int32_t ldy, int64_t M, int32_t C, sf_stream_t stream);
/* same with fp32 side rows of the stream (sf_rows32 above): side rows read side->in (or resid), write side->out */
int sf_row_scale_add_rows32(const void* x, int32_t ldx, const float* scale, int64_t rows_per_sample, const void* resid,
                            int32_t ldr, void* y, int32_t ldy, int64_t M, int32_t C, const sf_rows32* side, sf_stream_t stream);
/* xt[b][head][c][k] = x[b][k][head*D + c], zero for k in [Nk, ldk): K-contiguous operand for P.V and dS.K */
int sf_transpose_heads(const void* x, int32_t ldx, void* xt, int32_t ldk, int32_t B, int32_t Nk, int32_t heads, int32_t D,
                       sf_stream_t stream);

/* =====================================================================================================
 * X3D: SE block (operators.py:15-59), Swish (pytorchvideo), X3DHead average pool (head_helper.py:413-438).
 * Rows of a tensor are (n, pos), S positions per sample, C channels (padded to 8).
 * ===================================================================================================== */
int sf_sample_chunks(int64_t S, int32_t C);          /* part needs N * chunks * 2 * C floats */
/* out[n][c] = mean_pos relu?(y*scale + shift)  (nn.AdaptiveAvgPool3d(1) of SE on the BatchNorm output; the X3DHead
 * AvgPool3d over the whole (T,H,W) extent after conv_5_bn + ReLU); scale/shift NULL = identity */
int sf_sample_mean(int32_t N, int64_t S, int32_t C, const void* y, int32_t ldy, const float* scale, const float* shift,
                   int relu, float* part, float* out, sf_stream_t stream);
/* h = relu(W1 m + b1), gate = sigmoid(W2 h + b2) per sample; m, gate rows have pitch Cp >= C (pad gate = 0) */
int sf_se_gate_fwd(int32_t N, int32_t C, int32_t Cp, int32_t F, const float* m, const float* w1, const float* b1,
                   const float* w2, const float* b2, float* h, float* gate, sf_stream_t stream);
/* z = act(gate[n][c] * (y*scale + shift)), act = swish (x*sigmoid(x)) or relu; gate NULL = 1 */
int sf_gate_act_fwd(int32_t N, int64_t S, int32_t C, const void* y, int32_t ldy, const float* scale, const float* shift,
                    const float* gate, int swish, void* z, int32_t ldz, sf_stream_t stream);
/* dgate[n][c] = sum_pos dz * act'(gate*u) * u,  u = y*scale + shift */
int sf_gate_grad(int32_t N, int64_t S, int32_t C, const void* y, int32_t ldy, const float* scale, const float* shift,
                 const void* dz, int32_t lddz, const float* gate, int swish, float* part, float* dgate, sf_stream_t stream);
/* per-sample backward of the gate: dpre2 = dgate*g*(1-g), dpre1 = (W2^T dpre2) masked by h > 0, dm = W1^T dpre1 */
int sf_se_gate_bwd(int32_t N, int32_t C, int32_t Cp, int32_t F, const float* gate, const float* h, const float* w1,
                   const float* w2, const float* dgate, float* dpre2, float* dpre1, float* dm, sf_stream_t stream);
/* out[i][j] (+)= scale * sum_n a[n*lda + i] * b[n*ldb + j]  (SE weight/bias gradients; b NULL: J = 1, b = 1) */
int sf_outer_sum(const float* a, int32_t lda, const float* b, int32_t ldb, int32_t N, int32_t I, int32_t J, float* out,
                 float scale, int accumulate, sf_stream_t stream);
/* du = dz * act'(gate*u) * gate + dmean[n][c] / S  (gradient w.r.t. the BatchNorm output u); dmean NULL = 0 */
int sf_gate_act_bwd(int32_t N, int64_t S, int32_t C, const void* y, int32_t ldy, const float* scale, const float* shift,
                    const float* gate, int swish, const void* dz, int32_t lddz, const float* dmean, void* du, int32_t lddu,
                    sf_stream_t stream);
/* the same pass, also leaving the per-workgroup column sums of du and du * y in bn_part[sf_gate_act_bwd_bn_rows()][2][C]: the
 * reduction half of the backward of the BatchNorm in front of the gate (X3DTransform.b_bn, resnet_helper.py:226-250), which
 * sf_bn_bwd_finalize takes in place of sf_bn_bwd_reduce's table (ABI 23) */
/* one pass for the backward of SE-gated Swish: du0 = dz * act'(gate * u) * gate stored, sums[N][3][C] = per-sample sums of
 * dz * act'(gate * u) * u (the gate's gradient), du0 and du0 * y; part: [N * sf_sample_chunks(S, C)][4][C] scratch (ABI 23) */
int sf_gate_bwd_sums(int32_t N, int64_t S, int32_t C, const void* y, int32_t ldy, const float* scale, const float* shift,
                     const void* dz, int32_t lddz, const float* gate, int swish, void* du0, int32_t lddu, float* part,
                     float* sums, sf_stream_t stream);
/* sf_bn_bwd_apply for a gradient that lacks a per-sample constant: dy = k1 * (dz + sample_add[row / S][c]) + k2 + k3 * y (ABI 23) */
int sf_bn_bwd_apply_sample(int64_t M, int32_t C, const void* dz, int32_t lddz, const void* y, int32_t ldy, const float* coef,
                           const float* sample_add, int64_t S, void* dy, int32_t lddy, sf_stream_t stream);
int sf_gate_act_bwd_bn_rows(int32_t N, int64_t S, int32_t C);
int sf_gate_act_bwd_bn(int32_t N, int64_t S, int32_t C, const void* y, int32_t ldy, const float* scale, const float* shift,
                       const float* gate, int swish, const void* dz, int32_t lddz, const float* dmean, void* du, int32_t lddu,
                       float* bn_part, sf_stream_t stream);

/* ---- training-step glue on the flat gradient memory -- replaces tools/train_net.py:150-172 (GradScaler.unscale_ / step /
 * update, clip_grad_norm_ / clip_grad_value_, optimizer.get_grad_norm_, misc.check_nan_losses) and optimizer.step()
 * (slowfast/models/optimizer.py:100-140: SGD with momentum / dampening / nesterov, AdamW), SURVEY.md 8f-1.  No host sync:
 * everything the next launch needs travels through the control block `ctl` (8 fp32 words in device memory):
 *   [0] loss scale  [1] growth tracker  [2] found_inf of this step  [3] global gradient norm (unscaled, mean over ranks)
 *   [4] multiplier applied to the raw gradients = clip_coef / (world * scale)  [5] clean optimizer steps  [6] skipped steps. */
int sf_flat_blocks(int64_t n);                                  /* rows of `part` ([rows][2] fp32) for sf_flat_sumsq */
int sf_flat_sumsq(const float* g, int64_t n, float* part, sf_stream_t stream);     /* g: any 4-byte aligned range of the buffer (a
                                                                 * bucket at a time: the partial rows simply add up) */
/* one workgroup: norm / found_inf / clip coefficient into ctl; GradScaler.update() when `dynamic` */
int sf_step_control(const float* part, int32_t nblk, float* ctl, float world, float clip_norm, int dynamic, float growth,
                    float backoff, int32_t growth_interval, sf_stream_t stream);
/* segs: [nseg] {int64 start, int64 end, int32 group, int32 pad}; blk_seg / blk_off: per launched block its segment and its first
 * element inside it (multiples of 1024); lr / wd: HOST arrays, one entry per parameter group.  Skipped when ctl[2] != 0. */
int sf_flat_sgd(float* param, const float* grad, float* mom, const void* segs, const int32_t* blk_seg, const int32_t* blk_off,
                int32_t nblocks, const float* ctl, const float* lr, const float* wd, int32_t ngroups, float clip_val,
                float momentum, float dampening, int nesterov, sf_stream_t stream);
int sf_flat_adamw(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, const void* segs, const int32_t* blk_seg,
                  const int32_t* blk_off, int32_t nblocks, const float* ctl, const float* lr, const float* wd, int32_t ngroups,
                  float clip_val, float beta1, float beta2, float eps, sf_stream_t stream);
/* Table-driven update (ABI 24): sf_flat_sgd / sf_flat_adamw with the per-group hyper-parameters in DEVICE memory and no cap on
 * the number of groups -- slowfast/models/optimizer.py:146-237 (get_param_groups makes 2 * (MVIT.DEPTH + 2) groups and set_lr
 * rescales every one of them each iteration; a captured graph reads the table on replay, so the schedule survives capture).
 * hyper: [ngroups][4] fp32 {lr, weight_decay, lars_group (0 / 1), reserved}, 16-byte aligned, indexed by the segment's group.
 * trust: NULL, or [nseg] fp32 written by sf_flat_lars_trust; with it the LARS wrapper of optimizer.py:262-359 applies
 * (trust_coefficient mode, clip=False): a parameter with trust[seg] != 0 takes g = (g + wd * p) * trust[seg], and EVERY member
 * of a lars_group group steps with weight decay 0.  Same arithmetic per element as the two entry points above; 16-byte loads /
 * stores where a block's first element is 16-byte aligned in every buffer.  Skipped when ctl[2] != 0. */
int sf_flat_sgd_tab(float* param, const float* grad, float* mom, const void* segs, const int32_t* blk_seg, const int32_t* blk_off,
                    int32_t nblocks, const float* ctl, const float* hyper, const float* trust, float clip_val, float momentum,
                    float dampening, int nesterov, sf_stream_t stream);
int sf_flat_adamw_tab(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, const void* segs, const int32_t* blk_seg,
                      const int32_t* blk_off, int32_t nblocks, const float* ctl, const float* hyper, const float* trust,
                      float clip_val, float beta1, float beta2, float eps, sf_stream_t stream);
/* LARS trust ratios (optimizer.py:321-359), after sf_step_control (reads ctl[4]) and before the table-driven update.  Two
 * launches, no atomics: per-block sum p^2 / sum g_eff^2 (g_eff = clip_val(grad * ctl[4]), the gradient the update sees) in
 * double into part [nblocks][2], then one workgroup per segment sums its rows seg_row[s] .. seg_row[s + 1] - 1 ([nseg + 1] int32)
 * in a fixed order and writes trust[s] = trust_coef * |p| / (|g| + |p| * wd + eps); 0 = "leave the gradient alone" for a segment
 * whose flags word (the segment table's `pad`) has bit 0 clear (1-D parameter), whose group has lars_group 0, or whose |p| or
 * |g| is zero.  Both launches return at once when ctl[2] != 0 (trust keeps its previous content). */
int sf_flat_lars_trust(const float* param, const float* grad, const void* segs, const int32_t* blk_seg, const int32_t* blk_off,
                       int32_t nblocks, const int32_t* seg_row, int32_t nseg, const float* ctl, const float* hyper, double* part,
                       float* trust, float clip_val, float trust_coef, float eps, sf_stream_t stream);

/* MaskFeat step glue (ABI 30) -- the HOG regression targets of masked-feature pre-training (slowfast/models/operators.py:62-112,
 * models/masked.py:254-281) in one launch, and the mask-token substitution after the patch embedding (masked.py:546-579).
 * sf_hog_targets_f32: clip is the dense fp32 [B][3][T][H][W] clip; frames 0, ts, 2 ts, ... are used (Tu = ceil(T / ts)); cells
 * are 8 x 8 pixels, 9 bins; fs = tokens per side of the target grid, u = (H / 8) / fs cells per token side.  out is fp32
 * [B][Tu * fs * fs][27 * u * u]: token (t, i, j) is row (t * fs + i) * fs + j and feature ((c * 9 + bin) * u + dh) * u + dw is bin
 * `bin` of colour channel c of cell (i * u + dh, j * u + dw).  Arithmetic: reflect-pad by 1; gx = (l0 - r0) + 2 (l1 - r1) + (l2 - r2)
 * and gy likewise from the upper / lower neighbours, differences first (exact zeros on reflected borders and flat regions);
 * norm = sqrt(gx^2 + gy^2); bin = floor(atan2(gx, gy) / pi * 9) mod 9 with gx == 0 in bin 0; per-cell sums of norm, divided by
 * max(L2 norm over the 9 bins, 1e-12).  Fixed summation order (no atomics).  Rejected: H != W, H % (8 * fs) != 0, u > 17. */
int sf_hog_targets_f32(const float* clip, int32_t B, int32_t T, int32_t H, int32_t W, int32_t ts, int32_t fs, float* out,
                       sf_stream_t stream);
/* x is the 16-bit token tensor [B][cls + T*H*W][C] (row pitch ldx) the patch embedding wrote (embed + bias + pos, cls row in
 * front); mask the loader's uint8 window table [B][Tw][Hw][Ww] with Tw == T, H % Hw == 0, W % Ww == 0 (token (t, h, w) reads
 * window (t, h / (H / Hw), w / (W / Ww))).  Forward, in place: every masked patch row becomes round16(mask_token + pos row)
 * (pos: fp32 [cls + T*H*W][C] or NULL -> round16(mask_token)); other rows are not touched.  Backward: dx = dy with the masked rows
 * zeroed; dpos (fp32 [cls + T*H*W][C] or NULL) = per-row sum over the batch of dy on masked rows, every row written; part is
 * fp32 [sf_mask_tokens_bwd_blocks(cls + T*H*W, C)][2][C], whose slot-0 column sums are d(mask_token) (fold it with
 * sf_colsum_finalize: fixed order, no atomics). */
int sf_mask_tokens_fwd(void* x, int32_t ldx, int32_t B, int32_t cls, int32_t T, int32_t H, int32_t W, int32_t C, const void* mask,
                       int32_t Tw, int32_t Hw, int32_t Ww, const float* mask_token, const float* pos, sf_stream_t stream);
int sf_mask_tokens_bwd_blocks(int32_t rows, int32_t C);
int sf_mask_tokens_bwd(const void* dy, int32_t lddy, void* dx, int32_t lddx, int32_t B, int32_t cls, int32_t T, int32_t H,
                       int32_t W, int32_t C, const void* mask, int32_t Tw, int32_t Hw, int32_t Ww, float* dpos, float* part,
                       sf_stream_t stream);

/* MAE step glue (ABI 31) -- the kept-token gather in front of the encoder, the token assembly in front of the decoder
 * (slowfast/models/masked.py:283-445) and the pixel regression targets (masked.py:178-230).
 * ids is the int32 [B][L] ids_restore table, L = T'H'W' (the reference's argsort(argsort(noise))): patch row l of sample b is
 * kept iff r = ids[b][l] < K (compared unsigned) and then lives at kept position r.  No entry of the table, whatever its
 * value, makes a kernel read or write outside its buffers; a table that is not a permutation gives undefined values.
 * Token tensors are 16-bit rows in the activation type with a row pitch (ld*, elements, % 8 == 0); C % 8 == 0, C <= 2048,
 * cls in {0, 1}, 0 < K <= L.
 * sf_token_keep_fwd: x [B][cls + L][C] (the patch embedding's output: bias, position embedding and cls row included) ->
 * y [B][cls + K][C]: the cls row copied, source row l with r < K written to row cls + r.
 * sf_token_keep_bwd: dx[b][cls + l] = r < K ? dy[b][cls + r] : 0, cls row copied; every row of dx [B][cls + L][C] is written.
 * sf_token_restore_fwd: e [B][cls + K][C], mask_token fp32 [C], dpos fp32 [cls + L][C] ->
 * y[b][cls + l] = round16((r < K ? e[b][cls + r] : mask_token) + dpos[cls + l]), y[b][0] = round16(e[b][0] + dpos[0]) with cls.
 * sf_token_restore_bwd: one pass over dy [B][cls + L][C]: de[b][cls + r] = dy[b][cls + l] for kept rows (cls row copied);
 * d_dpos (fp32 [cls + L][C] or NULL) = sum over the batch of dy, in batch order; part is fp32
 * [sf_token_restore_bwd_blocks(cls + L, C)][2][C] whose slot-0 column sums are d(mask_token) (fold it with sf_colsum_finalize:
 * fixed order, no atomics). */
int sf_token_keep_fwd(const void* x, int32_t ldx, void* y, int32_t ldy, int32_t B, int32_t cls, int32_t L, int32_t K, int32_t C,
                      const int32_t* ids, sf_stream_t stream);
int sf_token_keep_bwd(const void* dy, int32_t lddy, void* dx, int32_t lddx, int32_t B, int32_t cls, int32_t L, int32_t K,
                      int32_t C, const int32_t* ids, sf_stream_t stream);
int sf_token_restore_fwd(const void* e, int32_t lde, void* y, int32_t ldy, int32_t B, int32_t cls, int32_t L, int32_t K,
                         int32_t C, const int32_t* ids, const float* mask_token, const float* dpos, sf_stream_t stream);
int sf_token_restore_bwd_blocks(int32_t rows, int32_t C);
int sf_token_restore_bwd(const void* dy, int32_t lddy, void* de, int32_t ldde, int32_t B, int32_t cls, int32_t L, int32_t K,
                         int32_t C, const int32_t* ids, float* d_dpos, float* part, sf_stream_t stream);
/* sf_pixel_targets_f32: clip is the dense fp32 [B][3][T][H][W] clip, p the patch side, ts the temporal patch stride; u = 1 takes
 * frames 0, ts, 2 ts, ... (MASK.TIME_STRIDE_LOSS), u = ts all frames.  out is fp32 [B][(T / ts) * (H / p) * (W / p)][u * p * p * 3]:
 * token (t, i, j) is row (t * (H / p) + i) * (W / p) + j, feature ((uu * p + pp) * p + qq) * 3 + c is pixel (i * p + pp, j * p + qq)
 * of channel c of frame t * ts + uu (the order of _patchify).  norm != 0: each row becomes (d - mean(d)) / sqrt(var(d) + 1e-6)
 * with d_i = x_i - x_0 (shifted by the row's first element: a constant patch gives exact zeros), var unbiased; both sums in a
 * fixed two-level order (64 lanes serially, then a 6-step fold).  Each used pixel is read once.  Rejected: H != W, H % p,
 * T % ts, u not in {1, ts}, u * p * p * 3 > 8192. */
int sf_pixel_targets_f32(const float* clip, int32_t B, int32_t T, int32_t H, int32_t W, int32_t ts, int32_t u, int32_t p,
                         int32_t norm, float* out, sf_stream_t stream);

/* MoCo step glue (ABI 34) -- slowfast/models/contrastive.py: Normalize, the "moco" branch of forward, _dequeue_and_enqueue,
 * _update_history.  Everything is fp32 in every build; no floating-point atomics, every sum has one fixed order.
 * sf_l2norm_rows: out[r] (dense [n][C]) = x[s] / sqrt(sum_c x[s][c]^2), s = perm ? perm[r] : r, x rows ld floats apart.  No
 * epsilon: a zero row gives NaN, as the reference's Normalize does.  perm (int32 [n]) is NOT checked here: the caller hands in
 * a permutation of 0 .. n-1.
 * sf_moco_nce_slabs, then sf_moco_nce_finalize with the same arguments: f [n][C] raw query features, key [V][n][C]
 * normalised keys, queue [K][C], inv_T = 1 / T -> logits [V n][1 + K] (row v n + i: column 0 = (q_i . key_v,i) / T, column
 * 1 + j = (q_i . queue_j) / T, q = f / |f|), loss[0] = mean over the V n rows of (logsumexp - column 0), df [n][C] = d loss / d f.
 * The queue is read once (by the first call); ws is sf_moco_nce_workspace(n, V, K, C) bytes, 16-byte aligned, and carries the
 * per-slab softmax partials from the first call to the second.  Rejected: C not a multiple of 64 or > 256, n C > 8192, V > 16,
 * K < 1.
 * sf_queue_enqueue: keys [views][rows][C] are written to queue [K][C] block after block at ptr[0] (device int64), which wraps to
 * 0 on reaching K and is stored back.  If ptr[0] < 0 or one of the writes would pass K, NOTHING is written, ptr stays and
 * err[0] (device int32) is set to 1 -- never an out-of-bounds store.  K % rows != 0 is rejected.
 * sf_ema_update: hist[i] = fl(fl(p[i] * mm[1]) + fl(hist[i] * mm[0])), mm = device float[2] {m, 1 - m}: three separately
 * rounded operations, the bits of torch's `p * (1.0 - m) + hist * m`. */
int sf_l2norm_rows(int32_t n, int32_t C, const float* x, int32_t ld, const int32_t* perm, float* out, sf_stream_t stream);
int64_t sf_moco_nce_workspace(int32_t n, int32_t V, int32_t K, int32_t C);
int sf_moco_nce_slabs(int32_t n, int32_t V, int32_t K, int32_t C, const float* f, const float* key, const float* queue,
                      float inv_T, float* logits, float* df, float* loss, void* ws, int64_t ws_bytes, sf_stream_t stream);
int sf_moco_nce_finalize(int32_t n, int32_t V, int32_t K, int32_t C, const float* f, const float* key, const float* queue,
                         float inv_T, float* logits, float* df, float* loss, void* ws, int64_t ws_bytes, sf_stream_t stream);
int sf_queue_enqueue(int32_t K, int32_t C, int32_t rows, int32_t views, const float* keys, float* queue, int64_t* ptr,
                     int32_t* err, sf_stream_t stream);
int sf_ema_update(int64_t n, const float* p, float* hist, const float* mm, sf_stream_t stream);

/* BYOL similarity loss (ABI 35) -- slowfast/models/contrastive.py: Normalize on the predictor output, sim_loss (:237-243) and its
 * loop over the keys in the "byol" branch of forward (:531-535), with the backward.  fp32 in every build, no floating-point
 * atomics, every sum has one fixed order.
 * sf_byol_sim_rows, then sf_byol_sim_finalize with the same arguments: p [n] rows of C floats ld floats apart (the RAW predictor
 * output), key [V][n][C] dense normalised keys, inv_T = 1 / T ->
 *   loss[0] = sum_v [ -mean_i((q_i . key_v,i) / T) ] / V,  q_i = p_i / |p_i|,
 *   df [n][C] dense = d loss / d p = -(1 / (V n T)) (S_i - q_i (q_i . S_i)) / |p_i|,  S_i = sum_v key_v,i.
 * No epsilon: a zero row gives NaN in its df row and in the loss, as the reference's Normalize does.  ws is
 * sf_byol_sim_workspace(n, V, C) bytes (the per-row terms, from the first call to the second).  Accepted: n >= 1, 1 <= V <= 16,
 * 1 <= C <= 4096, ld >= C; anything else returns -1 (the workspace query too) before anything is written. */
int64_t sf_byol_sim_workspace(int32_t n, int32_t V, int32_t C);
int sf_byol_sim_rows(int32_t n, int32_t V, int32_t C, const float* p, int32_t ld, const float* key, float inv_T, float* df,
                     float* loss, void* ws, int64_t ws_bytes, sf_stream_t stream);
int sf_byol_sim_finalize(int32_t n, int32_t V, int32_t C, const float* p, int32_t ld, const float* key, float inv_T, float* df,
                         float* loss, void* ws, int64_t ws_bytes, sf_stream_t stream);

/* SimCLR NT-Xent loss (ABI 37) -- slowfast/models/contrastive.py: Normalize on both crops' features and the "simclr" branch of
 * forward (:692-754), with the backward.  fp32 in every build, plain fp32 products, no floating-point atomics, every sum has one
 * fixed order.  sf_simclr_norm, sf_simclr_rows, sf_simclr_grad, in this order with the same arguments: a, b [n] rows of C floats
 * lda / ldb floats apart (the RAW features of the two crops), inv_T = 1 / T.  With x = [a; b] (M = 2 n rows), q_i = x_i / |x_i|,
 * s_ij = q_i . q_j, p(i) = (i + n) mod M, E_ij = exp((s_ij - 1) / T) for j != i (the diagonal is never formed), D_i = sum_j E_ij:
 *   loss[0] = (1 / M) sum_i ((1 - s_i,p(i)) / T + log D_i)     (= mean_i -log(exp(s_i,p(i) / T) / sum_{j != i} exp(s_ij / T)))
 *   g_k = sum_{j != k} E_kj (1 / D_k + 1 / D_j) q_j - 2 q_p(k),   dx_k = (1 / (M T)) (g_k - q_k (q_k . g_k)) / |x_k|
 *   da [n][C] dense = dx_0 .. dx_{n-1} = d loss / d a,   db [n][C] dense = dx_n .. dx_{M-1} = d loss / d b
 *   q_out [n][C] dense, or null = q_0 .. q_{n-1}, the normalised rows of a (written by sf_simclr_norm)
 * No epsilon: a zero row makes the loss and EVERY element of da and db NaN (it enters every D_j), as in the reference.  ws is
 * sf_simclr_workspace(n, C) bytes, 16-byte aligned (q, |x|, D, the row terms and the M x M matrix E, from call to call).
 * Accepted: 1 <= n <= 1024, 1 <= C <= 1024, lda, ldb >= C; anything else returns -1 (the workspace query too) before anything is
 * written. */
int64_t sf_simclr_workspace(int32_t n, int32_t C);
int sf_simclr_norm(int32_t n, int32_t C, const float* a, int32_t lda, const float* b, int32_t ldb, float inv_T, float* da, float* db,
                   float* loss, float* q_out, void* ws, int64_t ws_bytes, sf_stream_t stream);
int sf_simclr_rows(int32_t n, int32_t C, const float* a, int32_t lda, const float* b, int32_t ldb, float inv_T, float* da, float* db,
                   float* loss, float* q_out, void* ws, int64_t ws_bytes, sf_stream_t stream);
int sf_simclr_grad(int32_t n, int32_t C, const float* a, int32_t lda, const float* b, int32_t ldb, float inv_T, float* da, float* db,
                   float* loss, float* q_out, void* ws, int64_t ws_bytes, sf_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SFAMD_H */
