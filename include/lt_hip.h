/*
 * lt_hip.h -- flat C ABI of liblt_hip.so: hand-written HIP kernels (gfx950 / MI355X) for the
 * volumetric-triangulation forward path of karfly/learnable-triangulation-pytorch.
 *
 * The reference has no FFI/operator registry: the boundary it offers is a set
 * of Python callables whose arithmetic is done by ATen kernels.  Each entry point below replaces the
 * ATen kernels behind one of those callables; the Python host in
 * learnable-triangulation-pytorch_amd/mvn/ keeps the callables' names and signatures and binds
 * these symbols with ctypes (INTEGRATION.md shows the stub a reference maintainer would add).
 *
 * Conventions
 *   - plain pointers and sizes only; every pointer is DEVICE memory unless the name ends in _host;
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream); all work is enqueued on
 *     it and nothing synchronises, allocates or frees: every call is hipGraph-capturable;
 *   - return value: 0 = LT_OK, negative = error; lt_last_error() holds a message (thread local);
 *   - activations are channels-last: 2D maps N,H,W,C and volumes N,D,H,W,C, element type `dtype`
 *     (LT_F32, or LT_BF16 with fp32 accumulation); 2D tensors are the D == 1 case of 3D;
 *   - thread-safe for distinct streams.
 */
#ifndef LT_HIP_H
#define LT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LT_ABI_VERSION 1

enum { LT_F32 = 0, LT_BF16 = 1,
       LT_FP8 = 2 /* OCP e4m3 ("e4m3fn", torch.float8_e4m3fn; what gfx950's v_cvt_pk_fp8_f32 and fp8 MFMAs use), one byte per element: operands of
                     lt_conv_fwd only (BASELINE config 5: fp8 MFMA for the V2V 3D convolutions of the training step) */ };
enum { LT_OK = 0, LT_ERR_INVALID = -1, LT_ERR_UNSUPPORTED = -2, LT_ERR_LAUNCH = -3 };

/* view-aggregation modes of op.unproject_heatmaps (mvn/utils/op.py:149-164) */
enum { LT_AGG_SUM = 0, LT_AGG_MAX = 1, LT_AGG_SOFTMAX = 2, LT_AGG_CONF = 3,
       LT_AGG_CONF_NORM = 4 /* 'conf_norm': confidences divided by their sum over views first (triangulation.py:268-269) */ };

/* epilogue flags of lt_conv_fwd */
enum {
    LT_EPI_RELU_PRE = 1,  /* ReLU before the residual add  (Upsample3DBlock + skip, v2v.py:121-136) */
    LT_EPI_RELU_POST = 2, /* ReLU after the residual add   (Bottleneck / Res3DBlock, pose_resnet.py:92-93, v2v.py:42) */
    LT_EPI_STORE_F32 = 4, /* store fp32 even when dtype is bf16 (V2V logits feeding the soft-argmax) */
    LT_EPI_SIGMOID = 8,   /* v = 1/(1+exp(-v)) last (GlobalAveragePoolingHead, pose_resnet.py:160) */
    LT_EPI_RES_F32 = 64,  /* with LT_EPI_STORE_F32 on a bf16 convolution: the residual is fp32 too (the mixed-precision training step adds the input
                             gradient that is already there in the epilogue of the next input-gradient convolution) */
    LT_BN_FROZEN = 32,    /* lt_bn_act_bwd only: mean / var are FROZEN running statistics (a BatchNorm module in eval() inside a training step):
                             dy = gamma invstd g, without the batch-statistics terms; dgamma / dbeta as usual */
    LT_BN_Y_BF16 = 128,   /* lt_bn_act_fwd / lt_bn_act_bwd: the convolution output y is a bf16 tensor (the mixed-precision training step stores it in
                             16 bits; lt_bn_stats_fwd takes dtype = LT_BF16 for the same tensor); C % 4 == 0 */
    LT_ACT_BF16 = 256     /* lt_bn_act_fwd / lt_bn_act_bwd / lt_act_bwd: the 16-bit-activation training step (BASELINE config 5: "fp16 activations" -- bf16 here,
                             the 16-bit type whose MFMA products need no loss scaling): every activation-shaped tensor of the call other than y -- residual
                             and z (forward); dz, residual, dy, dres (backward) -- is a bf16 tensor behind the same pointer argument; the separate bf16
                             copies (z_bf16 / dy_bf16) must be NULL; C % 4 == 0 for the BatchNorm calls.  Statistics, gamma / beta and their gradients stay fp32. */
};

const char* lt_last_error(void);
int lt_abi_version(void);
/* fills CU count, LDS bytes per CU and the gcn arch name (e.g. "gfx950") of the current device */
int lt_device_info(int* cu_count, int* lds_per_cu, char* arch, int arch_len);

/* ---------------------------------------------------------------------------------------------
 * Generalised convolution = implicit GEMM on MFMA (fp32: v_mfma_f32_32x32x2_f32 / 16x16x4_f32,
 * exact fp32; bf16: v_mfma_f32_32x32x16_bf16 / 16x16x32_bf16, fp32 accumulate).
 * Replaces F.conv2d / F.conv3d / F.conv_transpose2d / F.conv_transpose3d + eval BatchNorm + ReLU +
 * residual add as used by PoseResNet.forward (mvn/models/pose_resnet.py:293-318, :75-95),
 * process_features (mvn/models/triangulation.py:238-240) and V2VModel.forward (mvn/models/v2v.py:7-66,
 * :164-169).
 *
 *   for every phase p, every point o = (n, od, oh, ow) of the iteration space N x Do x Ho x Wo and
 *   every output channel co:
 *     acc = sum_{tap t, ci} x[n, od*sd - pd + dd_t, oh*sh - ph + dh_t, ow*sw - pw + dw_t, ci]
 *                           * w_p[co][t*Cin + ci]                      (out-of-range taps read 0)
 *     v   = (acc + bias[co]) * scale[co] + shift[co]    (conv bias, then eval BatchNorm as ATen evaluates it:
 *                                                         scale = weight/sqrt(var+eps), shift = bias_bn - mean*scale;
 *                                                         NULL = 0 / 1 / 0; arrays hold cout_pad floats)
 *     if RELU_PRE v = max(v,0);  if residual v += residual[same place as y];  if RELU_POST v = max(v,0)
 *     y[n, od*osd + ood_p, oh*osh + ooh_p, ow*osw + oow_p, co] = v
 *
 * dtype == LT_FP8: x and the weights are e4m3 bytes (per-tensor scaled by the caller: x ~ sx * x8, w ~ sw * w8, see lt_quant_fp8), the
 * products run on v_mfma_f32_*_fp8_fp8 with fp32 accumulation, the result is stored as fp32 (LT_EPI_STORE_F32, a residual is fp32 too:
 * LT_EPI_RES_F32) or -- without LT_EPI_STORE_F32, Cout % 8 == 0 -- as bf16 (y and the residual are bf16 tensors: the 16-bit-activation training
 * step); the caller passes sx * sw in `scale` and the convolution's bias in `shift` (bias = NULL).  Cin >= 16, k_pad % 128 == 0 (one 128-byte
 * K step = 128 elements); generic implicit-GEMM kernel only.
 *
 * A plain convolution is one phase with out_stride 1 / out_off 0; a stride-2 transposed convolution
 * is 2^nd phases (one per output parity) with out_stride 2.  A single one-tap phase with unit strides,
 * zero pads and equal input / iteration / output extents IS a pointwise (1x1) convolution -- its tap must
 * be (0,0,0,0) -- and takes a fast path without tap or bounds logic.
 * -------------------------------------------------------------------------------------------*/
#define LT_CONV_MAX_PHASES 8

typedef struct lt_conv_phase {
    const void* weight;  /* [cout_pad][k_pad] elements of `dtype`, k = tap*Cin + ci, zero padded      */
    const int32_t* taps; /* ntaps x 4 int32: dd, dh, dw, element offset ((dd*H + dh)*W + dw)*Cin     */
    int32_t ntaps;
    int32_t out_off[3];  /* ood, ooh, oow                                                            */
    const void* weight_frag; /* optional (NULL = none): the same bf16 weights in an MFMA fragment order, so that a kernel can read
                                its weight operand with coalesced loads instead of staging it through LDS */
    int32_t weight_frag_layout; /* 0 = none; 1 = lt_conv_pack_weights (Cout % 256 == 0 layers, 288 x 256 / 144 x 256 kernels on the 16x16x32 MFMA);
                                   2 = lt_conv_pack_weights_t32 (3x3x3 64->64 / 32->64 / 128->128 / 16->32 halo kernel; round 5: the 2D halo kernel for 256->256
                                       layers on maps of 24 n x 8 m pixels -- 3x3 / stride 1 / pad 1, or the four 2 x 2-tap phases of a 4x4 / stride-2 /
                                       pad-1 transposed convolution, every phase packed with its own ntaps; taps must lie within one pixel of the output pixel);
                                   3 = lt_conv_pack_weights32 (288 x 256 kernel on the 32x32x16 MFMA) */
} lt_conv_phase;

typedef struct lt_conv_desc {
    int32_t dtype;              /* LT_F32 | LT_BF16                                                  */
    int32_t N, D, H, W, Cin;    /* input tensor (Cin a power of two, >= 16 bytes per pixel)           */
    int32_t Do, Ho, Wo;         /* iteration space per sample                                        */
    int32_t stride[3], pad[3];  /* sd,sh,sw / pd,ph,pw                                               */
    int32_t OD, OH, OW;         /* output tensor spatial dims                                        */
    int32_t out_stride[3];      /* osd, osh, osw                                                     */
    int32_t Cout, ldc;          /* real output channels; output pixel stride in elements (>= Cout)   */
    int32_t cout_pad, k_pad;    /* padded weight dims: cout_pad % tile_n == 0, k_pad % (128 B) == 0  */
    int32_t nphase;
    int32_t flags;              /* LT_EPI_*                                                          */
    int32_t tile;               /* 0 = choose; else one of LT_TILE_* (tests / tuning)                */
    int32_t stages;             /* 0 = choose; 2 or 3 = LDS-DMA ring depth of the v2 kernels (tuning)       */
    lt_conv_phase phase[LT_CONV_MAX_PHASES];
} lt_conv_desc;

/* bf16 weights [cout_pad][k_pad] (cout_pad % 16 == 0, k_pad % 32 == 0) -> cout_pad * k_pad elements in fragment order
 * ([k_pad / 32][cout_pad / 16][64 lanes][8]: lane l holds column 16 t + (l & 15), K elements 32 s + 8 (l >> 4) .. + 7). */
int lt_conv_pack_weights(const void* weight, int32_t cout_pad, int32_t k_pad, void* packed, void* stream);
/* The fragment order of the TRANSPOSED product (weights as the first MFMA operand), used by the 3x3x3 64 -> 64 halo kernel:
 * [tap][cin / 16][cout_pad / 32][64 lanes][8]; lane (r = l & 31, h = l >> 5) holds output channel
 * 32 b + 16 (r >> 4) + 8 ((r >> 2) & 1) + 4 ((r >> 3) & 1) + (r & 3), K elements 16 g + 8 h .. + 7 of the tap.
 * lt_conv_phase.weight_frag_layout says which of the orders weight_frag holds; a kernel only uses the one it was written for. */
int lt_conv_pack_weights_t32(const void* weight, int32_t cout_pad, int32_t k_pad, int32_t cin, int32_t ntaps, void* packed,
                             void* stream);
/* B-fragment order of the 32x32x16 MFMA (layout 3, conv_igemm7): [k_pad / 32][cout_pad / 32][2 K halves][64 lanes][8]; lane l of
 * fragment (step, block, kk) holds column 32 block + (l & 31), K elements 32 step + 16 kk + 8 (l >> 5) .. + 7.  cout_pad % 32 == 0. */
int lt_conv_pack_weights32(const void* weight, int32_t cout_pad, int32_t k_pad, void* packed, void* stream);

enum { LT_TILE_AUTO = 0,
       /* v1: register-staged tiles (kept for A/B runs and as a cross-check) */
       LT_TILE_128x128 = 1, LT_TILE_128x64 = 2, LT_TILE_256x32 = 3, LT_TILE_256x16 = 4, LT_TILE_64x64 = 5,
       /* v2 (default): LDS-DMA staging + LDS-transposed 16-byte epilogue */
       LT_TILE2_128x128 = 11, LT_TILE2_128x64 = 12, LT_TILE2_256x32 = 13, LT_TILE2_256x16 = 14, LT_TILE2_64x64 = 15,
       /* stride-1 3^3 / 7^3 conv3d with the input halo tile resident in LDS (auto-selected where it applies) */
       LT_TILE_HALO = 20,
       /* 288-row tile, eight waves, three-stage ring (bf16, auto-selected for the wide ResNet levels) */
       LT_TILE3_288 = 30,
       LT_TILE_DIRECT = 99 /* scalar fp32 VALU kernel, debug cross-check only */ };

int lt_conv_fwd(const lt_conv_desc* desc, const void* x, const float* bias, const float* scale, const float* shift,
                const void* residual, void* y, void* stream);
/* lt_conv_fwd whose residual is COMPUTED instead of read: y = relu_post((acc + bias) * scale + shift + W_skip . skip.x[same voxel]) -- the second
 * convolution of a Res3DBlock whose skip connection is a 1x1x1 convolution + BatchNorm (mvn/models/v2v.py:20-42, the 16 -> 32 block at :76).  The caller
 * folds the skip branch's BatchNorm scale into W_skip (fp32 product, then one bf16 rounding) and its (bias * scale + shift) into `shift`; the skip
 * convolution's own launch, its Cout-channel output and the read of that tensor disappear.  Covered: bf16, 3x3x3 / stride 1 / pad 1, 32 -> 32 channels,
 * skip.cin == 16, shapes the column-walk halo kernel takes (D % 4 == 0 with D >= 8, H % 8 == 0, W % 8 == 0, N * (H / 8) * (W / 8) a multiple of 8 and
 * >= 256, no LT_EPI_RELU_PRE / LT_EPI_STORE_F32) -- anything else returns LT_ERR_UNSUPPORTED (there is no fallback: callers ask before they record).
 * skip.x: N,D,H,W,cin channels-last bf16;  skip.weight_frag: lt_conv_pack_weights_t32 of [32][16] (ntaps 1, cin 16). */
typedef struct lt_conv_skip {
    const void* x;
    int32_t cin;
    const void* weight_frag;
} lt_conv_skip;
int lt_conv_skip_fwd(const lt_conv_desc* desc, const void* x, const float* bias, const float* scale, const float* shift,
                     const lt_conv_skip* skip, void* y, void* stream);
/* A 1x1 convolution over the channel concatenation of TWO tensors, the second one optionally subsampled:
 *   acc[m][co] = sum_{ci < Cin} x[m][ci] w[co][ci]  +  sum_{cj < second.cin} x2[n, oh * s, ow * s, cj] w[co][Cin + cj]        (m = (n, oh, ow))
 * followed by lt_conv_fwd's epilogue.  It is the last 1x1 convolution of a Bottleneck block TOGETHER with the block's `downsample` branch
 * (mvn/models/pose_resnet.py:75-95: out = bn3(conv3(t2)); residual = downsample(x); out += residual; relu -- the first blocks of layer2-4, whose
 * downsample is a stride-2 1x1 convolution + BatchNorm of the block input): the caller folds both BatchNorm scales into the two weight blocks (fp32
 * product, one bf16 rounding), passes scale = NULL and shift = shift3 + shift_d, and the downsample's launch, its C-channel output and the read of
 * that tensor as the residual disappear.  desc: the pointwise convolution over x ([N][Ho][Wo][Cin], one phase, one tap) with k_pad = Cin + second.cin
 * and weights [cout_pad][k_pad] = [w3 | w_d], ALSO given in fragment layout 3 (lt_conv_pack_weights32); bf16, Cin % 32 == 0, second.cin % 32 == 0,
 * k_pad % 64 == 0, cout_pad % 256 == 0; second: x2 [N][H][W][cin] with H = stride * Ho, W = stride * Wo, stride 1 or 2.  Anything else:
 * LT_ERR_UNSUPPORTED (one kernel, no fallback). */
typedef struct lt_conv_cat2 {
    const void* x;
    int32_t cin, H, W, stride;
} lt_conv_cat2;
int lt_conv_cat2_fwd(const lt_conv_desc* desc, const void* x, const lt_conv_cat2* second, const float* bias, const float* scale, const float* shift,
                     const void* residual, void* y, void* stream);
/* weight padding rule (every tile's N divides it): cout_pad = 16 if Cout <= 16, 32 if <= 32, 64 if <= 64,
 * else Cout rounded up to a multiple of 128; bias/scale/shift arrays hold cout_pad floats. */
int lt_conv_cout_pad(int32_t cout);
/* Samples per launch of lt_conv_fwd / lt_conv_skip_fwd / lt_conv_cat2_fwd for tensors of `per_sample` elements per sample (the largest of input,
 * output, second source).  The kernels index ONE launch with 32-bit element offsets; the entry points accept any batch and walk batches beyond 2^31
 * elements per tensor in chunks of this many samples, every per-sample pointer advanced in 64 bits (BASELINE config 4 at 32 samples per GPU --
 * 32 x 128^3 voxels x 32 channels = 2^31 elements -- is one call; reference: mvn/models/triangulation.py:245-355 has no such limit).  Returns N
 * when the whole batch fits, a multiple of 8 where possible otherwise, 0 when a single sample is too large. */
int32_t lt_conv_chunk_samples(int32_t N, int64_t per_sample);

/* ---- kernel selection (host only: no GPU needed) ----------------------------------------------------------------------------------------------------
 * The rules by which a plan host (lt_engine.PlanBuilder, lt_plan_create_vol) picks a fused launch, a split-K tap-group count or the fragment layout of a
 * convolution's weights.  Activations are given as their channels-last shape (N, D, H, W, C) (D = 1 for 2D maps), weights as their state-dict shape
 * (lt_wshape).  The rules hold for weights fixed when the plan is built.  Each reads its A/B switches at every call; a switch is on when it is set to
 * anything but "" or "0".  Boolean rules return 1 / 0. */
typedef struct lt_wshape {
    int32_t nd;                /* 4 (Conv2d / ConvTranspose2d) or 5 (3D) */
    int64_t s[5];
} lt_wshape;
/* lt_conv_skip_fwd: the second 3x3x3 32 -> 32 convolution of a Res3DBlock with its 1x1x1 16 -> 32 skip convolution computed in the launch, on shapes
 * the column-walk halo kernel takes in every sample chunk (LT_NO_CONV_SKIP, LT_HALO_NO_COL, LT_HALO_NO_PERSIST, LT_CONV_NO_HALO: off) */
int lt_sel_conv_skip(int32_t dtype, const int32_t x[5], const lt_wshape* w, const int32_t skip_x[5], const lt_wshape* skip_w);
/* which kernel lt_conv_fwd gives a bf16 7x7x7 / stride 1 / pad 3 convolution 32 -> (9..16) of x: 1 = the column walk (>= 256 whole columns of >= 2
 * tiles of 4 x 8 x 8 voxels, their count a multiple of 8), 0 = one tile per workgroup (LT_HALO_NO_COL7: always 0) */
int lt_sel_halo7_col(int32_t dtype, const int32_t x[5]);
/* the bf16 MFMA of conv2d_halo_kernel's instantiation (tile_rows, nphase) = (8, 1), (4, 1) (the 3x3) or (8, 4) (the transposed 4x4): 16 = 16x16x32,
 * 32 = 32x32x16; 0 = no such instantiation (LT_H2D_MF32: 32 everywhere) */
int lt_sel_halo2d_mfma(int32_t tile_rows, int32_t nphase);
/* ... and of the 3x3x3 32 -> 32 column walk's instantiation kind: 0 = bf16 store, 1 = computed skip residual (lt_conv_skip_fwd), 2 = fp32 store
 * (always 32); 0 = no such kind (LT_HALO_COL_MF32: 32 everywhere) */
int lt_sel_halo_col_mfma(int32_t kind);
/* lt_conv_cat2_fwd: a Bottleneck's 1x1 expand of t2 and its 1x1 stride-s downsample of x as one launch, from 200 tiles of 288 x 256 on
 * (LT_NO_CONV_CAT2, LT_CONV_NO_V7, LT_CONV_NO_V3: off; LT_CAT2_ANY_SIZE: any size) */
int lt_sel_conv_cat2(int32_t dtype, const int32_t t2[5], const lt_wshape* w_expand, const int32_t x[5], const lt_wshape* w_down, int32_t stride_down);
/* split-K tap groups S (1 = not split) of a 3x3x3 / stride 1 / pad 1 convolution with >= 128 input channels on at most 8^3 voxels; d: its descriptor
 * (the flags carry LT_EPI_STORE_F32 / LT_EPI_SIGMOID, which rule it out, as does transposed) (LT_CONV_NO_SPLITK: off) */
int lt_sel_splitk_slices(const lt_conv_desc* d, const lt_wshape* w, int32_t transposed);
/* lt_bottleneck_fwd: an identity Bottleneck (C, P) = (256, 64) or (512, 128), stride 1, H % 8 == 0, W % 16 == 0 (LT_NO_BNECK: off) */
int lt_sel_bottleneck(int32_t dtype, const int32_t x[5], const lt_wshape w[3], const int32_t strides[3]);
/* lt_bottleneck_ds_fwd: ResNet layer1's first Bottleneck 64 -> 64 -> 256 with its stride-1 downsample (LT_NO_BNECK, LT_NO_BNECK_DS: off) */
int lt_sel_bottleneck_ds(int32_t dtype, const int32_t x[5], const lt_wshape w[3], const int32_t strides[3], const lt_wshape* w_down, int32_t stride_down);
/* lt_expand_reduce_fwd: the 1x1 256 -> 1024 expand of a Bottleneck and the 1x1 1024 -> 256 reduce of the next one, from 36 x 96 pixels on
 * (LT_NO_XR: off; LT_XR_ANY_SIZE: any size) */
int lt_sel_expand_reduce(int32_t dtype, const int32_t t2[5], const int32_t res[5], const lt_wshape* w_expand, const lt_wshape* w_reduce);
/* lt_stem_pool_fwd: the 7x7 / stride 2 / pad 3 stem convolution to 64 channels of an 8-channel (padded) map with a 3x3 / stride 2 / pad 1 max pool
 * (pool = kernel, stride, pad) */
int lt_sel_stem_pool(int32_t dtype, const int32_t x[5], const lt_wshape* w, int32_t stride, int32_t pad, const int32_t pool[3]);
/* lt_pwchain_fwd: a chain of nlayers pointwise convolutions from 32 channels, inner widths 32, the last <= 32, over a multiple of 64 voxels */
int lt_sel_pwchain(int32_t dtype, const int32_t x[5], int32_t nlayers, const lt_wshape* w);
/* weight_frag_layout for every phase of the convolution d (0 = none): 2 for conv2d_halo_kernel (a 3x3 256 -> 256 on 24-wide maps or a 4x4 / stride-2
 * transposed 256 -> 256, from 60 tiles of 8 x 24 pixels on, d->tile == LT_TILE_AUTO, no residual; LT_CONV_NO_H2D, LT_CONV_V1, LT_DECONV_NO_H2D (the
 * transposed ones): off; LT_H2D_ANY_SIZE: any size) and for conv3d_halo_wreg_kernel (3x3x3 64 -> 64, 32 -> 64, 128 -> 128, 16 -> 32), 3 for conv_igemm7
 * and 1 for conv_igemm6 (cout_pad % 256 == 0, k_pad % 64 == 0: 1 for pointwise layers with k_pad <= 256 and under LT_CONV_NO_V7).  bf16 only. */
int lt_sel_frag_layout(const lt_conv_desc* d, const lt_wshape* w, int32_t transposed, int32_t has_residual);

/* max pooling, channels-last, window k / stride s / zero-size padding p per dim (padding never wins):
 * F.max_pool2d(x,3,2,1) (pose_resnet.py:297) and F.max_pool3d(x,2,2) (v2v.py:51) */
int lt_maxpool_fwd(int32_t dtype, const void* x, void* y, int32_t N, int32_t D, int32_t H, int32_t W, int32_t C,
                   const int32_t k[3], const int32_t s[3], const int32_t p[3], void* stream);

/* x.mean over all pixels per channel (GlobalAveragePoolingHead.forward, pose_resnet.py:168-170):
 * x N,HW,C channels-last -> y N,C */
int lt_global_avgpool(int32_t dtype, const void* x, void* y, int32_t N, int32_t HW, int32_t C, void* stream);

/* images N,C,H,W fp32 (the reference's input layout, datasets/utils.py:45-52) -> N,H,W,c_pad `dtype`,
 * channels >= C zero filled */
int lt_nchw_to_nhwc(int32_t dtype, const float* x, void* y, int32_t N, int32_t C, int32_t HW, int32_t c_pad, void* stream);
/* channels-last `dtype` (pixel stride ld) -> N,C,HW fp32 (API outputs) */
int lt_nhwc_to_nchw_f32(int32_t dtype, const void* x, float* y, int32_t N, int32_t C, int32_t HW, int32_t ld, void* stream);

/* The reduction half of a split-K convolution: lt_conv_fwd run with S tap-group PHASES (identity epilogue, LT_EPI_STORE_F32, phase p
 * writing depth slice p of a [N][S * Do][Ho][Wo][C] fp32 tensor) leaves S partial sums per output; this adds them in the order p = 0 ..
 * S-1 (fp32) and applies the convolution's real epilogue -- (sum + bias) * scale + shift, LT_EPI_RELU_PRE, residual add, LT_EPI_RELU_POST
 * -- like the conv kernels do.  partial: [N][S][rows_per_sample][C] fp32; residual / y: [N][rows_per_sample][C] of `dtype`.  Used for
 * V2V's 3^3 128 -> 128 layers at the 8^3 / 4^3 / 2^3 levels (mvn/models/v2v.py:78-90), whose 54-step K loop is latency-bound. */
int lt_splitk_reduce(int32_t dtype, const float* partial, int32_t S, int64_t N, int64_t rows_per_sample, int32_t C, const float* bias,
                     const float* scale, const float* shift, const void* residual, void* y, int32_t flags, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Voxel-grid construction: mvn/models/triangulation.py:298-339 + volumetric.rotate_coord_volume
 * (mvn/utils/volumetric.py:102-114), fp32 in the reference's operation order:
 *   X = R_b * ((pos_b + step*idx) - center_b) + center_b        idx = (i,j,k), 'ij' meshgrid
 * pos/center: B x 3 fp32, rot: B x 9 fp32 row-major.  coords: B,V,V,V,3 fp32.
 * cmu_transfer != 0 applies permute(0,2,1,3) + flip(axis 1) (triangulation.py:336-339).
 * -------------------------------------------------------------------------------------------*/
int lt_coord_volumes(const float* pos, const float* center, const float* rot, float step, int32_t B, int32_t V,
                     int32_t cmu_transfer, float* coords, void* stream);
/* volumetric.rotate_coord_volume (mvn/utils/volumetric.py:102-114) for an arbitrary point set:
 * y[i] = rot (3x3 row-major, device) * x[i], i < n; x, y: n x 3 fp32 */
int lt_rotate_points(const float* x, const float* rot, float* y, int64_t n, void* stream);

/* ---------------------------------------------------------------------------------------------
 * op.unproject_heatmaps (mvn/utils/op.py:99-166) fused with
 * multiview.project_3d_points_to_image_plane_without_distortion (mvn/utils/multiview.py:89-110):
 * per voxel and view: project, z<=0 mask, perspective divide, the reference's (h,w)-swapped
 * normalisation, bilinear sample (zeros padding, align_corners=True), then aggregate over views.
 *   feats : B,NV,h,w,C channels-last `dtype`     proj: B,NV,3,4 fp32
 *   coords: B,v0,v1,v2,3 fp32 (any grid; arbitrary point sets use v0 = v1 = 1)
 *   conf  : B,NV,C fp32 (LT_AGG_CONF*)           out : B,v0,v1,v2,C channels-last `dtype`
 * One 16-byte channel vector per lane (a voxel's C channels = consecutive lanes -> every bilinear tap
 * and every output voxel is one contiguous run); 4x4x16 voxel bricks per workgroup keep the projected
 * footprint compact in L1/L2; with B % 8 == 0 sample b is pinned to XCD b % 8 (private L2).
 * Precondition of all four entries below, documented and not guarded: proj and coords (or pos, center, rot, step
 * of the grid entries) are FINITE.  A NaN or infinite pixel coordinate gives a NaN sample in the reference's CPU
 * grid_sample and a zero sample in both kernels here (their in-range tests are float comparisons, which a NaN
 * fails); nobody should rely on either.  Feature maps may hold anything; only a masked view's map is never read.
 *
 * ONE operation, described by lt_unproject_desc; the variant is WHICH POINTERS ARE SET:
 *   coords set                              the coordinate form: the voxel centres are read (pos, center, rot, coords_out NULL)
 *   pos, center, rot, coords_out set        the grid form: the model's cuboid grid, v0 = v1 = v2 = V (coords NULL); see lt_unproject_grid_fwd
 *   view_mask set                           over the valid views of every sample (lt_unproject_masked_fwd); NULL: every view is valid
 *   frame_of set, F frames                  B cuboids over F frames (lt_unproject_indexed_fwd); view_mask, if set, is per frame
 *   view_base set, T images                 a ragged batch, NV = NVcap (lt_unproject_ragged_fwd)
 * Kernel instantiation: view_base -> ragged; else frame_of -> indexed (nullable mask); else view_mask -> masked; else plain.
 * view_base together with view_mask or frame_of, and any backward with view_base, have no kernel: LT_ERR_UNSUPPORTED.  Both of coords and
 * the cuboid set, or neither: LT_ERR_INVALID.  All checks precede any device work.
 *   lt_unproject_desc_fwd            out: B,v0,v1,v2,C channels-last `dtype` (grid form: coords_out is written too)
 *   lt_unproject_desc_bwd_workspace  host only: bytes for `items` samples (cuboids, with frame_of) walked at once; items = B: the whole batch,
 *                                    items = 1: the least lt_unproject_desc_bwd takes; 0 where the gather does not take C.  The two layouts:
 *                                    lt_unproject_bwd (plain, masked) and lt_unproject_indexed_bwd (frame_of) below
 *   lt_unproject_desc_bwd            grad_out, grad_feats, grad_conf, the workspace and its chunked walk as lt_unproject_bwd / lt_unproject_indexed_bwd
 *                                    below; in the grid form it reads the coords_out its forward wrote, so one descriptor serves both directions
 * The eleven lt_unproject_*_fwd / *_bwd entries and the two workspace queries below are shorthands: each fills a descriptor and calls these.
 * -------------------------------------------------------------------------------------------*/
typedef struct lt_unproject_desc {
    int32_t dtype;
    const void* feats;           /* B,NV,h,w,C (frame_of: F,NV,h,w,C; view_base: T,h,w,C) */
    const float* proj;
    const float* coords;         /* coordinate form: read; NULL in the grid form */
    const float *pos, *center, *rot;   /* grid form: all set, with coords_out */
    float step;
    int32_t cmu_transfer;
    float* coords_out;
    const float* conf;           /* LT_AGG_CONF*: the confidences; else NULL */
    const uint8_t* view_mask;    /* NULL: every view valid */
    const int32_t* frame_of;     /* set: B cuboids over F frames */
    int32_t F;
    const int32_t* view_base;    /* set: ragged, T images in all, NV = NVcap */
    int32_t T;
    int32_t B, NV, C, h, w, v0, v1, v2, agg;
} lt_unproject_desc;
int lt_unproject_desc_fwd(const lt_unproject_desc* desc, void* out, void* stream);
size_t lt_unproject_desc_bwd_workspace(const lt_unproject_desc* desc, int32_t items);
int lt_unproject_desc_bwd(const lt_unproject_desc* desc, const float* grad_out, float* grad_feats, float* grad_conf, void* workspace,
                          size_t workspace_bytes, void* stream);
int lt_unproject_fwd(int32_t dtype, const void* feats, const float* proj, const float* coords, const float* conf,
                     void* out, int32_t B, int32_t NV, int32_t C, int32_t h, int32_t w, int32_t v0, int32_t v1,
                     int32_t v2, int32_t agg, void* stream);
/* The same over the cuboid grid of the model (triangulation.py:298-339) described by lt_coord_volumes' arguments instead of a
 * coordinate tensor: the voxel centres are computed in registers (bit-identical to lt_coord_volumes) and WRITTEN to coords_out
 * (B,V,V,V,3 fp32, a returned tensor of the forward) on the way -- the 12 bytes per voxel are never read back.  Fused for bf16,
 * C = 32, 4 or 8 views, view softmax, V % 16 == 0; any other configuration runs lt_coord_volumes + lt_unproject_fwd inside. */
int lt_unproject_grid_fwd(int32_t dtype, const void* feats, const float* proj, const float* pos, const float* center, const float* rot,
                          float step, int32_t cmu_transfer, float* coords_out, const float* conf, void* out, int32_t B, int32_t NV,
                          int32_t C, int32_t h, int32_t w, int32_t V, int32_t agg, void* stream);
/* lt_unproject_fwd / lt_unproject_grid_fwd over the VALID views of every sample: view_mask is DEVICE (B, NV) uint8, non-zero = valid.  Sample b
 * gets what the unmasked entry gives for its views {v : view_mask[b][v]} alone, in increasing v: a masked view's feature map is never read
 * (NaN there cannot leak), it is not projected into, and it takes no part in the sum, the max, the softmax's max or denominator, the conf sum
 * or conf_norm's normaliser.  A sample without a valid view writes zeros.  fp32 and every generic configuration: bit-identical to the
 * unmasked entry on the compacted views; the fused bf16 kernel (C = 32, 4 or 8 views, view softmax, bricked volume) keeps its own masked
 * variant, whose arithmetic and order with an all-ones mask are exactly the unmasked kernel's, and in which a masked view costs no loads,
 * no blend and no exp2 (the mask is uniform over a workgroup: one scalar branch per view).  A null view_mask is LT_ERR_INVALID. */
int lt_unproject_masked_fwd(int32_t dtype, const void* feats, const float* proj, const float* coords, const float* conf, const uint8_t* view_mask,
                            void* out, int32_t B, int32_t NV, int32_t C, int32_t h, int32_t w, int32_t v0, int32_t v1, int32_t v2, int32_t agg,
                            void* stream);
int lt_unproject_grid_masked_fwd(int32_t dtype, const void* feats, const float* proj, const float* pos, const float* center, const float* rot,
                                 float step, int32_t cmu_transfer, float* coords_out, const float* conf, const uint8_t* view_mask, void* out,
                                 int32_t B, int32_t NV, int32_t C, int32_t h, int32_t w, int32_t V, int32_t agg, void* stream);
/* Several cuboids per frame: lt_unproject_masked_fwd / lt_unproject_grid_masked_fwd with the views taken through an index.  Cuboid p of the P
 * reads the maps, projections, confidences and mask of frame frame_of[p] of the F:
 *   by frame  (F): feats F,NV,h,w,C   proj F,NV,3,4   conf F,NV,C   view_mask F,NV uint8 or NULL = every view valid
 *   by cuboid (P): coords / coords_out P,v0,v1,v2,3   out P,v0,v1,v2,C   pos, center P,3   rot P,9
 *   frame_of: DEVICE (P) int32 in [0, F), any order; a frame may have no cuboid.
 * The result is bit-identical to the masked (view_mask) or unmasked (NULL) entry on feats, proj, conf and view_mask gathered by frame_of, without
 * the P / F copies of the maps: the kernel choice is the unindexed call's own rule (the fused bf16 kernel for C = 32, 4 or 8 views, view softmax,
 * bricked volume; a grid call without one runs lt_coord_volumes over the P cuboids first), each kernel as the indexed instantiation of its masked
 * form.  A workgroup reads its cuboid's frame once, as a scalar, and clamps it into [0, F-1]: an index outside that range cannot make the kernel
 * read outside feats -- it reads a wrong frame instead; callers check their indices (both plan hosts refuse a bad one before any launch).
 * With P % 8 == 0 cuboid p is pinned to XCD p % 8 like a sample of the unindexed entries; LT_UNPROJ_PIN=frame (A/B, read per call) pins cuboid p
 * to XCD frame_of[p] % 8 instead, so that the cuboids of one frame share an L2 (LT_UNPROJ_PIN=cuboid: the default; same bits either way).
 * frame_of NULL, F < 1 or P < 1: LT_ERR_INVALID; P * chunks >= 2^31 workgroups: LT_ERR_UNSUPPORTED. */
int lt_unproject_indexed_fwd(int32_t dtype, const void* feats, const float* proj, const float* coords, const float* conf, const uint8_t* view_mask,
                             const int32_t* frame_of, void* out, int32_t F, int32_t P, int32_t NV, int32_t C, int32_t h, int32_t w, int32_t v0,
                             int32_t v1, int32_t v2, int32_t agg, void* stream);
int lt_unproject_grid_indexed_fwd(int32_t dtype, const void* feats, const float* proj, const float* pos, const float* center, const float* rot,
                                  float step, int32_t cmu_transfer, float* coords_out, const float* conf, const uint8_t* view_mask,
                                  const int32_t* frame_of, void* out, int32_t F, int32_t P, int32_t NV, int32_t C, int32_t h, int32_t w, int32_t V,
                                  int32_t agg, void* stream);
/* Ragged view batches: samples with different numbers of views, without padding.  The T = sum(n_b) views of the B samples lie sample-major
 * (sample 0's views first):
 *   by view   (T): feats T,h,w,C   proj T,3,4   conf T,C or NULL
 *   by sample (B): coords / coords_out B,v0,v1,v2,3   out B,v0,v1,v2,C   pos, center B,3   rot B,9
 *   view_base: DEVICE (B + 1) int32, the exclusive prefix sum of the counts: sample b reads rows view_base[b] + v, v < n_b = view_base[b+1] - view_base[b].
 *   NVcap: the most views a sample may have, 1..32; it selects the kernel as NV does for the other entries (4 or 8 with bf16, C = 32, view softmax and
 *          a bricked volume: the fused kernel; NVcap <= 8: the register-resident generic kernel; else the recomputing one).
 * The kernels are the ragged instantiations of the masked forms: sample b's validity bits are the prefix (1 << n_b) - 1, so the result is bit-identical
 * to lt_unproject_masked_fwd / lt_unproject_grid_masked_fwd on the inputs padded to (B, NVcap) with a prefix mask -- and with every n_b = NVcap to the
 * unmasked entries on the same tensors seen as (B, NVcap, ...).  A view slot past n_b issues no feature load, and the fused kernel, which projects into
 * every slot, loads the projection of the sample's last view in such a slot's place: no address outside the T rows is formed for a load.  A workgroup
 * reads its sample's two offsets once, as scalars, and clamps n_b into [0, min(NVcap, T)] and the first row into [0, T - n_b]: a bad table cannot make
 * the kernel read outside feats, proj or conf -- it reads wrong views instead; callers check their counts.  n_b = 0 writes zeros.
 * NULL feats, proj, out, view_base (coords, or pos / center / rot / coords_out), B < 1, T < 1, NVcap outside [1, 32], a bad dtype or aggregation code:
 * LT_ERR_INVALID before any device work. */
int lt_unproject_ragged_fwd(int32_t dtype, const void* feats, const float* proj, const float* coords, const float* conf, const int32_t* view_base,
                            void* out, int32_t B, int32_t T, int32_t NVcap, int32_t C, int32_t h, int32_t w, int32_t v0, int32_t v1, int32_t v2,
                            int32_t agg, void* stream);
int lt_unproject_grid_ragged_fwd(int32_t dtype, const void* feats, const float* proj, const float* pos, const float* center, const float* rot,
                                 float step, int32_t cmu_transfer, float* coords_out, const float* conf, const int32_t* view_base, void* out,
                                 int32_t B, int32_t T, int32_t NVcap, int32_t C, int32_t h, int32_t w, int32_t V, int32_t agg, void* stream);
/* The seam of the cascade (lt_plan_forward_cascade, CascadeTriangulationNet): the pelvis and cuboid algebra of VolumetricTriangulationNet.forward
 * (triangulation.py:284-296) on joints that are already on the device, bit-identical to what the host route writes into a plan's geometry block.
 *   keypoints_3d: DEVICE (B, J, 3) fp32.  kind LT_KIND_MPII: base = joint 6; LT_KIND_COCO: base = (joint 11 + joint 12) / 2, added and halved in fp32.
 *   base is promoted to fp64; position = base - cuboid_side / 2 in fp64; center = fp32(base), pos = fp32(position): DEVICE (B, 3) fp32 each, the
 *   pos / center arguments of lt_unproject_grid_fwd and lt_coord_volumes.  One lane per (sample, axis).
 * J < 7 (mpii) / 13 (coco), B < 1, an unknown kind or a null pointer is LT_ERR_INVALID before anything is enqueued. */
enum { LT_KIND_MPII = 0, LT_KIND_COCO = 1 };
int lt_cuboid_from_keypoints(const float* keypoints_3d, int32_t B, int32_t J, int32_t kind, double cuboid_side, float* pos, float* center,
                             void* stream);

/* ---------------------------------------------------------------------------------------------
 * op.integrate_tensor_3d_with_coordinates (mvn/utils/op.py:84-96):
 *   p = softmax_over_voxels(mult * logits[b,j,:])  (or relu(mult*logits) when softmax == 0)
 *   kp[b,j,:] = sum_vox p * coords[b,vox,:]
 * logits: fp32, element (b,j,vox) at b*J*nvox + vox*ld + j when channels_last (dense rows: ld == J;
 * ld > J is LT_ERR_UNSUPPORTED, ld < J LT_ERR_INVALID) else b*J*nvox.. (b*J + j)*nvox + vox.
 * J <= 32 (more: LT_ERR_UNSUPPORTED).  probs: B,J,nvox fp32 (always joint-major, the API layout) or
 * NULL: the joints are bitwise the same with and without it.  workspace: lt_softargmax3d_workspace() bytes.
 * PRECONDITION: every logit is FINITE.  The online softmax rescales its running sums by
 * exp(m_old - m_new); a lane whose first logit is -inf computes exp(-inf - -inf) = NaN there, where
 * torch.softmax gives that voxel probability 0 (+inf and NaN are NaN in torch too).  No layer of
 * these networks produces an infinity in front of the soft-argmax, and nothing is checked on the device.
 * -------------------------------------------------------------------------------------------*/
size_t lt_softargmax3d_workspace(int32_t B, int32_t J, int64_t nvox);
int lt_softargmax3d_fwd(const float* logits, const float* coords, float mult, int32_t softmax, int32_t channels_last,
                        int32_t ld, float* kp, float* probs, int32_t B, int32_t J, int64_t nvox, void* workspace,
                        void* stream);
/* lt_softargmax3d_fwd plus per-joint statistics of the 3D heatmap, out of the same pass that writes the probabilities (mvn.utils.volumetric.keypoint_stats
 * states them in numpy fp64).  Arguments, layouts, limits and refusals are lt_softargmax3d_fwd's (stats or peak_index NULL: LT_ERR_INVALID); kp and
 * probs are bit for bit what it writes for the same arguments; probs may be NULL (the same pass without the stores).  workspace:
 * lt_softargmax3d_stats_workspace() bytes.  stats: B,J,8 fp32 records {peak, mass, cxx, cxy, cxz, cyy, cyz, czz}; peak_index: B,J int32.
 * Per (b, j), with x_i = fp32(mult * logit_i) over the nvox voxels (the one rounding the kernels make):
 *   softmax != 0, p = softmax(x):
 *     peak_index  the smallest flat voxel index i at which x_i is maximal (the index order of probs[b, j])
 *     peak        p at peak_index; equal to probs[b, j, peak_index] bit for bit (that value is 1 / S)
 *     mass        1.0f
 *     centre      the returned fp32 joint kp[b, j]
 *     cov         sum_i p_i (c_i - centre)(c_i - centre)^T, mm^2, in the frame of coords (rotated cuboids need no special handling)
 *   softmax == 0, w = relu(x), joints unnormalised as in lt_softargmax3d_fwd:
 *     mass        sum_i w_i
 *     peak_index  as above, on x (not on w)
 *     peak        relu(x_peak) / mass, one fp32 division
 *     centre      kp[b, j] / mass, one fp32 division per coordinate of the two returned numbers
 *     cov         sum_i (w_i / mass)(c_i - centre)(c_i - centre)^T
 *     mass == 0 gives peak = 0 and cov = 0
 * The moments are taken about the centre, never as a difference of raw second moments.  Lanes accumulate in fp32, the chunk partials are combined
 * in fp64 in a fixed order, there are no float atomics: two calls give equal bits.  nvox must fit an int32. */
size_t lt_softargmax3d_stats_workspace(int32_t B, int32_t J, int64_t nvox);
int lt_softargmax3d_stats_fwd(const float* logits, const float* coords, float mult, int32_t softmax, int32_t channels_last, int32_t ld,
                              float* kp, float* probs, float* stats, int32_t* peak_index, int32_t B, int32_t J, int64_t nvox, void* workspace,
                              void* stream);

/* op.integrate_tensor_2d (mvn/utils/op.py:11-47) on N,J,h,w fp32 heatmaps (joint-major): 2D
 * soft-argmax; writes coords N,J,2 (x,y) and the normalised heatmaps (or NULL). */
int lt_softargmax2d_fwd(const float* heatmaps, float mult, int32_t softmax, float* coords, float* probs, int32_t NJ,
                        int32_t h, int32_t w, void* stream);
/* lt_softargmax2d_fwd plus per-heatmap statistics out of its third pass, the one that writes the probabilities (mvn.utils.multiview.heatmap_stats_2d
 * states them in numpy fp64).  Arguments and layout are lt_softargmax2d_fwd's; coords and probs are bit for bit what it writes; probs may be NULL (the
 * same pass without its store).  stats: NJ,5 fp32 records {peak, mass, cxx, cxy, cyy}; peak_index: NJ int32.
 * Per heatmap, with x_i = fp32(mult * hm_i) (the one rounding the kernel makes) and the flat index i = y * w + x, pixel centres c_i = (x, y):
 *   softmax != 0, p = softmax(x):
 *     peak_index  the smallest i at which x_i is maximal
 *     peak        p at peak_index; equal to probs[peak_index] bit for bit
 *     mass        1.0f
 *     centre      the returned fp32 (coords_x, coords_y)
 *     cov         sum_i p_i (c_i - centre)(c_i - centre)^T, heatmap pixels^2
 *   softmax == 0, w = relu(x) (the returned heatmaps stay unnormalised):
 *     mass        sum_i w_i
 *     peak_index  as above, on x (not on w)
 *     peak        relu(x_peak) / mass, one fp32 division
 *     centre      the returned coordinates
 *     cov         sum_i (w_i / mass)(c_i - centre)(c_i - centre)^T
 *     mass == 0 gives peak = 0 and cov = 0 (the coordinates are NaN, as lt_softargmax2d_fwd's)
 * The moments are taken about the centre, never as a difference of raw second moments.  Lanes accumulate in fp32, the waves' partials are combined in
 * fp64 in a fixed order, the (largest x, smallest index) pair by compare-and-select; there are no atomics: two calls give equal bits.
 * LT_ERR_INVALID: stats, peak_index, heatmaps or coords NULL, a size < 1.  LT_ERR_UNSUPPORTED: h * w does not fit an int32. */
int lt_softargmax2d_stats_fwd(const float* heatmaps, float mult, int32_t softmax, float* coords, float* probs, float* stats, int32_t* peak_index,
                              int32_t NJ, int32_t h, int32_t w, void* stream);
/* Backward of the two ops above and of lt_triangulate_dlt (training of AlgebraicTriangulationNet, train.py:189-236): what autograd derives in the
 * reference through softmax / sums (op.py:23-45) and through torch.svd (multiview.py:163).  lt_softargmax2d_bwd: probs / coords are the forward's
 * outputs, grad_coords N*J,2 -> grad_heatmaps (both modes; a gradient on the returned heatmaps is not supported).  lt_triangulate_dlt_bwd:
 * grad_out B,J,3 -> grad_points B,NV,J,2 and grad_conf B,NV,J (may be NULL); fp64 inside, the forward's SVD recomputed. */
int lt_softargmax2d_bwd(const float* probs, const float* coords, const float* grad_coords, float mult, int32_t softmax, float* grad_heatmaps,
                        int32_t NJ, int32_t h, int32_t w, void* stream);
int lt_triangulate_dlt_bwd(const float* proj, const float* points, const float* conf, const float* grad_out, float* grad_points, float* grad_conf,
                           int32_t B, int32_t NV, int32_t J, void* stream);
/* integrate_tensor_2d's backward with a gradient on BOTH outputs: grad_coords N*J,2 (may be NULL: a zero coordinate gradient, bit for bit) and
 * grad_probs N*J,h,w on the returned heatmaps (may be NULL: the result is then bit-identical to lt_softargmax2d_bwd, which stays as it is).
 *   softmax:  grad_heatmaps_i = [coordinate term of lt_softargmax2d_bwd] + mult * p_i * (gp_i - sum_k p_k gp_k)
 *   ReLU:     grad_heatmaps_i = [coordinate term] + mult * [e_i > 0] * gp_i        (the returned heatmaps are relu(mult * h), un-normalised)
 * Fixed-order sums, no atomics.  LT_ERR_INVALID: probs, coords or grad_heatmaps NULL, both gradients NULL, a size < 1, h * w >= 2^31. */
int lt_softargmax2d_bwd_full(const float* probs, const float* coords, const float* grad_coords, const float* grad_probs, float mult, int32_t softmax,
                             float* grad_heatmaps, int32_t NJ, int32_t h, int32_t w, void* stream);
/* 2D heatmap targets and the heatmap loss of the backbone's own training (the reference's op.py:169-196 and the MSE against its renders); all fp32.
 * lt_render_gaussians_2d: points n,2 as (x, y) in heatmap pixels, sigmas n,2 -> out n,h,w:
 *     out[i, y, x] = exp(-((x - px)^2 / sx^2 + (y - py)^2 / sy^2) / 2) / norm,   norm = 2 pi sx sx if normalize else 1
 *   (sigma_x TWICE in the normaliser, as gaussian_2d_pdf of the reference has it).
 * lt_heatmap_mse_fwd: pred NJ,h,w contiguous, validity NJ or NULL (= all 1) ->
 *     terms[i] = validity[i] * sum_xy (pred - G)^2          (G: the render above, never written to memory; the loss is sum(terms) / (h w max(1, sum validity)))
 *     grad_pred (may be NULL) = 2 validity[i] (pred - G) / (h w max(1, sum validity)), written in the same pass; terms keep their bits either way.
 *   A heatmap with validity == 0 gets terms = 0 and an all-zero gradient row, and its points / sigmas are NEVER read (a NaN keypoint of a missing
 *   annotation does not leak).  sum validity is re-added in a fixed order by every workgroup: no host round trip, no atomics, equal bits every call.
 * LT_ERR_INVALID: a NULL pointer other than validity / grad_pred, a size < 1, h * w >= 2^31.  LT_ERR_UNSUPPORTED: h + w > 8192. */
int lt_render_gaussians_2d(const float* points, const float* sigmas, float* out, int32_t n, int32_t h, int32_t w, int32_t normalize, void* stream);
int lt_heatmap_mse_fwd(const float* pred, const float* points, const float* sigmas, const float* validity, int32_t normalize, float* terms,
                       float* grad_pred, int32_t NJ, int32_t h, int32_t w, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Training-step pieces outside the convolutions: what torch.autograd derives in the
 * reference for op.unproject_heatmaps and op.integrate_tensor_3d_with_coordinates, the fused VolumetricCELoss
 * (mvn/models/loss.py:52-80; the reference walks samples and joints in Python with a .cpu() per sample), and the
 * batch statistics of training-mode BatchNorm.  All gradients are fp32.
 *
 * lt_unproject_bwd (like lt_unproject_masked_bwd and lt_unproject_indexed_bwd below, a shorthand of lt_unproject_desc_bwd; the two workspace queries
 *   are shorthands of lt_unproject_desc_bwd_workspace): grad_out B,v0,v1,v2,C (channels-last, fp32; the coordinate volume's grid shape) -> grad_feats B,NV,h,w,C fp32 (written
 *   completely, no pre-zeroing), grad_conf B,NV,C or NULL.  Autograd semantics of op.py:113-162: nothing flows to the grid / projections;
 *   depth <= 0 samples pass no gradient but their zero takes part in the view softmax, d out/d x_v = w_v (1 + x_v - out); 'max': the first
 *   maximal view.  Tie rule of 'max': the whole gradient of a voxel and channel goes to the LOWEST view index among the views whose sample equals
 *   the maximum (a later view wins only where it is strictly greater), for every NV.  A view at depth <= 0 takes part in max and softmax with the
 *   value 0 -- ties at 0 are the normal case -- and where such a view is that first maximum the gradient is dropped: its four weights are 0.
 *   LT_AGG_CONF: g * conf_v and grad_conf_v = sum over voxels of g * x_v; LT_AGG_CONF_NORM: conf is the RAW head output,
 *   normalised over the views as in the forward (triangulation.py:268-269), grad_conf is the gradient of the raw values.  1 <= NV <= 32
 *   (more is LT_ERR_UNSUPPORTED: the many-view kernels' LDS copies and the finalizer's workgroup are sized by it), C % 4 == 0.  Three
 *   launches over a workspace, K0 taps, K1 per-view gradient of the sampled values, K2 gather; K0 and K2 take any NV.  NV <= 8: K1 keeps
 *   every view's sample in registers (a 4- and an 8-view form), as do the confidence finalizer and the scatter.  9 <= NV <= 32: K1 walks
 *   the views without per-view registers -- sum / conf / conf_norm in groups of 8 views (one group per workgroup, the 8-view kernel's
 *   arithmetic and partial sums: a view's gradients are the bits the 8-view kernel gives for it), softmax / max in three passes over the
 *   views (max, sums, gradients) that sample again in each -- and the finalizer and the scatter have many-view forms of their own.
 *   Workspace per sample and view, each block rounded up to 256 bytes per sample: nvox * C * 4 (dxs, K1's output: 1.04 GB per sample at
 *   31 views, 64^3 voxels, C = 32) + nvox * 20 (tap records) + nbricks * 16 (bounding boxes, nbricks = product of ceil(v / 4)) +
 *   min(2048, ceil(nvox * C / 1024)) * C * 8 (confidence partials).  A deterministic GATHER (bitwise repeatable; no global atomics): workspace from lt_unproject_bwd_workspace (bytes for the
 *   whole batch; with less -- at least one sample's share -- the batch is walked in chunks).  C > 64 or not a power of two (and
 *   LT_UNPROJ_BWD_ATOMICS=1): the round-2 scatter by float atomics (no workspace, not repeatable, no conf_norm).
 * lt_softargmax3d_bwd: probs B,J,nvox and kp B,J,3 are the forward's outputs; grad_kp B,J,3; an optional SPARSE gradient on the
 *   returned probabilities (one voxel per (b,j): gp_idx / gp_val, what lt_volumetric_ce_fwd produces) -> grad_logits
 *   (planar B,J,nvox, or channels-last B,nvox,J when channels_last != 0):  mult * p_i * (a_i - sum_j p_j a_j), a_i = g_kp . X_i + gp_i.
 * lt_volumetric_ce_fwd: per (b,j) the voxel nearest to keypoints_gt (first minimum, like torch.argmin), terms[b,j] =
 *   validity * -log(p + 1e-6), idx[b,j], grad_val[b,j] = d(sum(terms) / (B J)) / d probs[b,j,idx].  The loss is sum(terms) / (B J).
 * lt_bn_stats_fwd: x rows x C channels-last -> per-channel mean and BIASED variance (fp64 accumulation); running statistics
 *   (may be NULL) are updated the way torch does: (1 - momentum) * running + momentum * stat, variance unbiased.
 * -------------------------------------------------------------------------------------------*/
size_t lt_unproject_bwd_workspace(int32_t B, int32_t NV, int32_t C, int32_t v0, int32_t v1, int32_t v2);
int lt_unproject_bwd(int32_t dtype, const void* feats, const float* proj, const float* coords, const float* conf, const float* grad_out,
                     float* grad_feats, float* grad_conf, int32_t B, int32_t NV, int32_t C, int32_t h, int32_t w, int32_t v0, int32_t v1,
                     int32_t v2, int32_t agg, void* workspace, size_t workspace_bytes, void* stream);
/* lt_unproject_bwd over the VALID views of every sample, the backward of lt_unproject_masked_fwd: view_mask is DEVICE (B, NV) uint8, non-zero =
 * valid (NULL is LT_ERR_INVALID).  Sample b gets what autograd derives for the unprojection of its views {v : view_mask[b][v]} alone:
 * grad_feats[b, v] and grad_conf[b, v, :] of a masked view are +0.0 everywhere (the buffers are still written completely, no pre-zeroing); a
 * masked view's feature map, projection matrix and confidence are never read (NaN there cannot leak); max: the first maximal VALID view;
 * conf_norm: the normaliser, and the derivative through it, over the valid views.  A sample without a valid view gets zeros.  The valid
 * views are walked in index order: for NV <= 8 the arithmetic is the unmasked kernel's on the compacted views, operation for operation, and
 * with an all-ones mask every NV gives lt_unproject_bwd's bits.  Same workspace (lt_unproject_bwd_workspace), argument checks, 1 <= NV <= 32
 * and chunked walk of the batch as lt_unproject_bwd.  Gather path only: C > 64 or not a power of two, and LT_UNPROJ_BWD_ATOMICS=1, are
 * LT_ERR_UNSUPPORTED (there is no masked scatter). */
int lt_unproject_masked_bwd(int32_t dtype, const void* feats, const float* proj, const float* coords, const float* conf, const uint8_t* view_mask,
                            const float* grad_out, float* grad_feats, float* grad_conf, int32_t B, int32_t NV, int32_t C, int32_t h, int32_t w,
                            int32_t v0, int32_t v1, int32_t v2, int32_t agg, void* workspace, size_t workspace_bytes, void* stream);
/* Several cuboids per frame, the backward of lt_unproject_indexed_fwd: what autograd derives for the unprojection of feats[frame_of], proj[frame_of],
 * conf[frame_of] (and view_mask[frame_of]) without the P / F copies.
 *   by frame  (F): feats F,NV,h,w,C   proj F,NV,3,4   conf F,NV,C   view_mask F,NV uint8 or NULL = every view valid   grad_feats F,NV,h,w,C fp32
 *                  grad_conf F,NV,C fp32 or NULL
 *   by cuboid (P): coords P,v0,v1,v2,3   grad_out P,v0,v1,v2,C fp32
 *   frame_of: DEVICE (P) int32, any order, read inside the kernels only (a new assignment is just another call) and clamped into [0, F-1] as the
 *   forward does.
 * grad_feats[f] is the sum over the cuboids p with frame_of[p] == f of cuboid p's unindexed gradient, added per cell in (cuboid, brick, voxel) order
 * inside the gather's LDS tile (K2 runs one workgroup per (tile, view, frame) and walks the frame's cuboids in ascending p); grad_conf[f] is the same
 * sum, in fp64 over (cuboid, workgroup) with one rounding, and conf_norm's chain rule is applied once, on that sum.  A frame without a cuboid gets
 * +0.0 everywhere; both outputs are written completely (no pre-zeroing).  Deterministic, no atomics; with frame_of = 0 .. F-1 the bits are those of
 * lt_unproject_bwd (NULL mask) / lt_unproject_masked_bwd.  Layouts, dtypes, aggregations, 1 <= NV <= 32 and the error codes are those entries';
 * gather path only (C a power of two <= 64; LT_UNPROJ_BWD_ATOMICS=1 is LT_ERR_UNSUPPORTED); frame_of NULL, F < 1 or P < 1: LT_ERR_INVALID.
 * Workspace: lt_unproject_indexed_bwd_workspace (host only; 0 where the gather does not take C) = the fp64 confidence partials of ALL P cuboids
 * (nblk1 * NV * C * 8 bytes each, rounded up to 256 in all) + P times one cuboid's dxs, tap records and bounding boxes (lt_unproject_bwd's blocks).
 * With less -- at least the partials plus ONE cuboid's share -- the cuboids are walked in ascending chunks, a later chunk's tile starting from
 * what the earlier ones stored: the same additions in the same order, so both gradients are bit-identical for every workspace size. */
size_t lt_unproject_indexed_bwd_workspace(int32_t P, int32_t NV, int32_t C, int32_t v0, int32_t v1, int32_t v2);
int lt_unproject_indexed_bwd(int32_t dtype, const void* feats, const float* proj, const float* coords, const float* conf, const uint8_t* view_mask,
                             const int32_t* frame_of, const float* grad_out, float* grad_feats, float* grad_conf, int32_t F, int32_t P, int32_t NV,
                             int32_t C, int32_t h, int32_t w, int32_t v0, int32_t v1, int32_t v2, int32_t agg, void* workspace, size_t workspace_bytes,
                             void* stream);
int lt_softargmax3d_bwd(const float* probs, const float* coords, const float* kp, const float* grad_kp, const int32_t* gp_idx,
                        const float* gp_val, float multiplier, int32_t softmax, int32_t channels_last, float* grad_logits, int32_t B,
                        int32_t J, int64_t nvox, void* stream);
/* the same with a DENSE gradient on the returned probabilities as well (gp_dense: B,J,nvox fp32 or NULL -- any loss on the volumes, what the reference's
 * autograd accepts at train.py:222-230): a_i += gp_dense_i; workspace_bj: B * J floats (sum_i p_i gp_dense_i per joint, softmax mode). */
int lt_softargmax3d_bwd_dense(const float* probs, const float* coords, const float* kp, const float* grad_kp, const int32_t* gp_idx,
                              const float* gp_val, const float* gp_dense, float* workspace_bj, float multiplier, int32_t softmax,
                              int32_t channels_last, float* grad_logits, int32_t B, int32_t J, int64_t nvox, void* stream);
int lt_volumetric_ce_fwd(const float* coords, const float* probs, const float* keypoints_gt, const float* validity, float* terms,
                         int32_t* idx, float* grad_val, int32_t B, int32_t J, int64_t nvox, void* stream);
size_t lt_bn_stats_workspace(int64_t rows, int32_t C);
int lt_bn_stats_fwd(int32_t dtype, const void* x, int64_t rows, int32_t C, float* mean, float* var, float* running_mean,
                    float* running_var, float momentum, void* workspace, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Training step around the convolutions (fp32, channels-last rows x C): the reference's modules in training mode
 * (train.py:233-243: zero_grad / backward / step) -- see lt_train.py for the tape that strings them together.
 * lt_bn_act_fwd : z = act(gamma (y - mean) / sqrt(var + eps) + beta, residual) with lt_conv_fwd's LT_EPI_RELU_* flags; mean / var
 *   from lt_bn_stats_fwd (batch statistics).  C % 4 == 0.
 * lt_bn_act_bwd : its autograd: g = dz * relu mask; dbeta = sum g; dgamma = sum g x^; dy = gamma invstd (g - dbeta/n - x^ dgamma/n)
 *   (LT_BN_FROZEN in flags: mean / var are running statistics that do not depend on the batch: dy = gamma invstd g);
 *   dres (may be NULL) = the residual input's gradient, added to the buffer when accumulate_res.  workspace: lt_bn_act_bwd_workspace.
 *   Optional outputs (fine-tuning with frozen parameters; the shape and flag checks come first, so a refusal names what is wrong):
 *     dgamma = dbeta = NULL, dy given : frozen gamma / beta under a layer that still owes dy.  Batch statistics: the same three launches, the two
 *       column sums are finalized into the workspace (its last 2 C floats) instead of caller memory; dy / dres / dy_bf16 bit for bit as with them.
 *       LT_BN_FROZEN: dy = gamma invstd g is elementwise -- ONE launch, no reduce / finalize, workspace may be NULL.
 *     dy = NULL, dgamma and dbeta given : only the parameter gradients (reduce + finalize, no apply pass); dy_bf16 and dres must be NULL too.
 *     exactly one of dgamma / dbeta NULL, or dy, dgamma and dbeta all NULL : LT_ERR_INVALID.
 * lt_act_bwd    : layers without BatchNorm: dy = dz * mask(z, flags) (+ dres); LT_EPI_SIGMOID: dy = dz * z * (1 - z).  LT_EPI_RELU_PRE together
 *   with a residual is refused (LT_ERR_UNSUPPORTED): the sign of v cannot be rebuilt from z = relu(v) + res.
 * lt_channel_sum: out[c] (+)= sum over rows of x[row][c] (bias gradients), fp64 accumulation.
 * lt_maxpool_bwd: dx (pre-zeroed / accumulated) += dy at the first maximal element of every window; overlapping windows (k > s) are walked in
 *   ceil(k / s)^3 classes of mutually disjoint windows, one launch each: no atomics, bitwise repeatable.
 * lt_conv_wgrad : dw[co][tap * Cin + ci] (=|+=) sum_m dy[m][co] * x[m @ tap][ci] over the GEMM rows m = (n, od, oh, ow) of the forward
 *   convolution described by (N, D, H, W, Cin, Do, Ho, Wo, stride, pad, taps); exact-fp32 MFMA, no atomics (the pixel range is cut into
 *   slabs whose partial sums are added in a fixed order: workspace of lt_conv_wgrad_workspace(rows = N*Do*Ho*Wo, cout_pad, k_pad) bytes,
 *   may be 0).  For a transposed convolution swap the roles (dy := the layer's INPUT at its own resolution, x := the output gradient,
 *   stride 2): dw[ci][tap * Cout + co].
 *   accumulate (here and in lt_conv_wgrad_bf16 / lt_conv_wgrad_bf16_nhwc): 0 -> every element of dw [cout_pad][k_pad] is WRITTEN (rows past Cout and
 *   columns past ntaps * Cin with zeros; dw may hold anything before the call); 1 -> the sum is ADDED to what dw holds, one fp32 addition per
 *   element behind the ordered slab sum (dw + (s0 + s1 + ...); a shape with a single slab adds the accumulator to dw in the kernel's own epilogue).
 *   Leading dimensions: dy is read as [rows][ldy >= Cout] and only its channels [0, Cout) are read -- channels [Cout, ldy) may hold anything, NaN
 *   included, and never reach dw; the LDS-brick and pointwise kernels need ldy % 4 == 0 and other values of ldy take the generic kernel.  x of
 *   lt_conv_wgrad and both packed operands of lt_conv_wgrad_bf16 are dense in their channels (the pack takes the source's ld and drops the padding);
 *   lt_conv_wgrad_bf16_nhwc reads x16 as [..][ldx >= Cin] with the same promise for channels [Cin, ldx).
 * lt_adam_step  : torch.optim.Adam's single-tensor update (bias-corrected, eps outside the sqrt).  beta1 / beta2 are doubles: 1 - beta and
 *   1 - beta^step are formed in fp64 and then rounded to fp32, as torch does from its Python floats (1 - 0.999f is 1.3e-5 off 0.001).
 * -------------------------------------------------------------------------------------------*/
int lt_bn_act_fwd(const void* y /* fp32, or bf16 with LT_BN_Y_BF16 */, const float* mean, const float* var, const float* gamma, const float* beta, const void* residual, void* z,
                  void* z_bf16 /* optional: a bf16 copy of z on the way (mixed-precision training), or NULL */, int64_t rows, int32_t C, float eps,
                  int32_t flags, void* stream);
size_t lt_bn_act_bwd_workspace(int64_t rows, int32_t C);
int lt_bn_act_bwd(const void* dz, const void* y /* fp32, or bf16 with LT_BN_Y_BF16 */, const void* residual, const float* mean, const float* var, const float* gamma, const float* beta,
                  void* dy, void* dy_bf16 /* optional bf16 copy of dy, or NULL */, float* dgamma, float* dbeta, void* dres, int32_t accumulate_res,
                  int64_t rows, int32_t C, float eps, int32_t flags, void* workspace, void* stream);
int lt_act_bwd(const void* dz, const void* z, const void* residual, void* dy, void* dres, int32_t accumulate_res, int64_t total, int32_t flags,
               void* stream);
size_t lt_channel_sum_workspace(int64_t rows, int32_t C);
int lt_channel_sum(const float* x, int64_t rows, int32_t C, float* out, int32_t accumulate, void* workspace, void* stream);
/* the same over a tensor of element type `dtype` (LT_F32 | LT_BF16: the 16-bit-activation training step); same workspace */
int lt_channel_sum_dt(int32_t dtype, const void* x, int64_t rows, int32_t C, float* out, int32_t accumulate, void* workspace, void* stream);
int lt_maxpool_bwd(const float* x, const float* dy, float* dx, int32_t N, int32_t D, int32_t H, int32_t W, int32_t C, const int32_t k[3],
                   const int32_t s[3], const int32_t p[3], void* stream);
/* x, dy, dx of element type `dtype` (LT_F32 | LT_BF16); the (up to ceil(k / s)^3) contributions an input collects are added in the class order, in `dtype` */
int lt_maxpool_bwd_dt(int32_t dtype, const void* x, const void* dy, void* dx, int32_t N, int32_t D, int32_t H, int32_t W, int32_t C, const int32_t k[3],
                      const int32_t s[3], const int32_t p[3], void* stream);
size_t lt_conv_wgrad_workspace(int64_t rows, int32_t cout_pad, int32_t k_pad);
int lt_conv_wgrad(const float* dy, const float* x, const int32_t* taps, float* dw, int32_t N, int32_t D, int32_t H, int32_t W, int32_t Cin, int32_t Do,
                  int32_t Ho, int32_t Wo, const int32_t stride[3], const int32_t pad[3], int32_t Cout, int32_t ldy, int32_t cout_pad, int32_t k_pad,
                  int32_t ntaps, int32_t accumulate, void* workspace, void* stream);
/* The same weight gradient on the bf16 MFMA (mixed-precision training, BASELINE config 5): the reduction index is the pixel and the 16-bit MFMA
 * wants 8 consecutive K values per lane, so the operands are IMAGE-OCTET packed -- the one axis no tap ever shifts:
 *   lt_pack_n8_bf16: src [N][P][ld >= C] fp32 (P pixels per image) -> dst [ceil(N / 8)][P][C] elements of 8 bf16 (16 bytes) = the values of images
 *   8g .. 8g+7 at that pixel and channel, zero for images past N; dst is 16-byte aligned, lt_pack_n8_bf16_bytes(N, P, C) bytes.  Only channels
 *   [0, C) of a pixel are read (the padding [C, ld) may hold anything); C, ld multiples of 4 and src 16-byte aligned: the vector kernel.
 *   lt_conv_wgrad_bf16: arguments as lt_conv_wgrad with dy16 = pack of dy [N][Do*Ho*Wo][ldy] and x16 = pack of x [N][D*H*W][Cin]; fp32
 *   accumulation, fixed summation order (slabs + ordered reduce: bitwise repeatable); workspace of lt_conv_wgrad_bf16_workspace(
 *   ceil(N / 8) * Do*Ho*Wo, cout_pad, k_pad) bytes.  Result = lt_conv_wgrad of the bf16-rounded operands up to fp32 summation order. */
size_t lt_pack_n8_bf16_bytes(int32_t N, int64_t P, int32_t C);
int lt_pack_n8_bf16(const float* src, void* dst, int32_t N, int64_t P, int32_t C, int32_t ld, void* stream);
/* the same from a bf16 tensor [N][P][ld] (the operand copy the mixed-precision convolutions read): C, ld multiples of 8, 16-byte aligned */
int lt_pack_n8_from_bf16(const void* src_bf16, void* dst, int32_t N, int64_t P, int32_t C, int32_t ld, void* stream);
size_t lt_conv_wgrad_bf16_workspace(int64_t octet_rows, int32_t cout_pad, int32_t k_pad);
int lt_conv_wgrad_bf16(const void* dy16, const void* x16, const int32_t* taps, float* dw, int32_t N, int32_t D, int32_t H, int32_t W, int32_t Cin, int32_t Do,
                       int32_t Ho, int32_t Wo, const int32_t stride[3], const int32_t pad[3], int32_t Cout, int32_t ldy, int32_t cout_pad, int32_t k_pad,
                       int32_t ntaps, int32_t accumulate, void* workspace, void* stream);
/* The same GEMM straight from the channels-last bf16 tensors, without the packs (the 16-bit-activation step: the activations and their gradients
 * ARE the bf16 operands): dy16 [N][Do*Ho*Wo][ldy], x16 [N][D][H][W][ldx], 16-byte aligned; every lane of the 16x16x32 MFMA reads 4 or 8 consecutive
 * channels of the eight images of its pixel and transposes them in registers (v_perm_b32) into that many operands.  lt_conv_wgrad_bf16_nhwc_ok
 * -> 1 when the shape is covered: Cin a power of two, Cout / ldy multiples of 8 (4 when cout_pad <= 64), Cin / ldx multiples of 4 (8 when
 * cout_pad <= 64), k_pad a multiple of 4, 32-bit element offsets -- and NOT one of the V2V shapes lt_conv_wgrad_bf16 has LDS kernels for (3^3 / stride 1
 * / pad 1 bricks, the 7^3 front layer): those stay on the packed path.  Same result contract, same workspace as lt_conv_wgrad_bf16
 * (reference: autograd of nn.Conv2d / nn.ConvTranspose2d in pose_resnet.py inside train.py:217-243's backward). */
int lt_conv_wgrad_bf16_nhwc_ok(int32_t N, int32_t D, int32_t H, int32_t W, int32_t Cin, int32_t ldx, int32_t Do, int32_t Ho, int32_t Wo, const int32_t stride[3],
                               const int32_t pad[3], int32_t Cout, int32_t ldy, int32_t cout_pad, int32_t k_pad, int32_t ntaps);
int lt_conv_wgrad_bf16_nhwc(const void* dy16, const void* x16, const int32_t* taps, float* dw, int32_t N, int32_t D, int32_t H, int32_t W, int32_t Cin, int32_t ldx,
                            int32_t Do, int32_t Ho, int32_t Wo, const int32_t stride[3], const int32_t pad[3], int32_t Cout, int32_t ldy, int32_t cout_pad,
                            int32_t k_pad, int32_t ntaps, int32_t accumulate, void* workspace, void* stream);
/* What the three entry points above would launch for a shape (host only: no GPU needed, nothing is launched).  The entry points take their kernel,
 * slab count and grid from the very functions these queries call, so the answer cannot drift from the launch.  Arguments as the entry point's, N ..
 * ntaps; a workspace is taken as given (without one lt_conv_wgrad falls back to its generic kernel for the pointwise, 2D-brick and 7^3 shapes).
 *   family         LT_WGRAD_GENERIC (operands straight from L2), _BRICK3D (3^3 LDS bricks), _BRICK2D (3x3 LDS bricks), _POINTWISE (LDS GEMM), _K7 (7^3)
 *   variant        generic: the wave tile, fp32 / packed bf16 0 = 128 x 64, 1 = 64 x 128, 2 = 32 x 256 (co x k), nhwc 0 = 128 x 64, 1 = 64 x 128;
 *                  brick kernels: input channels per workgroup (fp32 3D 32, 2D 128; bf16 16 or 32; nhwc 32); pointwise and 7^3: 0
 *   slabs          S: partial sums the ordered reduce adds (1 for a generic kernel: no workspace, no reduce)
 *   units          what the slabs cut: generic = GEMM rows (pixels; octet rows = ceil(N / 8) * Do*Ho*Wo for the bf16 entry points), brick / 7^3 =
 *                  bricks over (image or octet group, d, h, w), pointwise = chunks of 32 rows
 *   units_per_slab slab s covers units [s * units_per_slab, min(units, (s + 1) * units_per_slab)); a generic kernel's trailing slabs may be empty
 *   grid           the main kernel's grid (x, y, z); xcd_remap: 1 when a generic kernel deals its workgroups to the XCDs in contiguous ranges
 * Returns LT_OK, or the error the entry point would return for the shape (lt_conv_wgrad_bf16_plan with nhwc != 0: LT_ERR_UNSUPPORTED where
 * lt_conv_wgrad_bf16_nhwc_ok says 0).  A change to any slab planner re-checks tests/test_wgrad_plan_cpu.py: it names the case that reaches each branch. */
#define LT_WGRAD_GENERIC 0
#define LT_WGRAD_BRICK3D 1
#define LT_WGRAD_BRICK2D 2
#define LT_WGRAD_POINTWISE 3
#define LT_WGRAD_K7 4
typedef struct lt_wgrad_plan {
    int32_t family, variant, slabs, units_per_slab;
    int64_t units;
    int32_t grid[3];
    int32_t xcd_remap;
} lt_wgrad_plan;
int lt_conv_wgrad_plan(int32_t N, int32_t D, int32_t H, int32_t W, int32_t Cin, int32_t Do, int32_t Ho, int32_t Wo, const int32_t stride[3], const int32_t pad[3],
                       int32_t Cout, int32_t ldy, int32_t cout_pad, int32_t k_pad, int32_t ntaps, lt_wgrad_plan* out);
/* nhwc = 0: lt_conv_wgrad_bf16 (ldx is ignored); nhwc = 1: lt_conv_wgrad_bf16_nhwc */
int lt_conv_wgrad_bf16_plan(int32_t nhwc, int32_t N, int32_t D, int32_t H, int32_t W, int32_t Cin, int32_t ldx, int32_t Do, int32_t Ho, int32_t Wo,
                            const int32_t stride[3], const int32_t pad[3], int32_t Cout, int32_t ldy, int32_t cout_pad, int32_t k_pad, int32_t ntaps,
                            lt_wgrad_plan* out);
/* dst[i] = idx[i] >= 0 ? src[idx[i]] : 0 -- the layout changes between a Parameter's own layout and the GEMM layouts of its layer
 * (forward weights, input-gradient weights, weight-gradient blocks), with index maps built once when a training plan is recorded */
int lt_gather_f32(const float* src, const int32_t* idx, float* dst, int64_t n, void* stream);
/* the same with the result rounded to bf16 (the live weights of the mixed-precision step in the layout its bf16 convolutions read) */
int lt_gather_f32_bf16(const float* src, const int32_t* idx, void* dst_bf16, int64_t n, void* stream);
/* small helpers of the training tape, so that no torch op sits between the launches: y += x; dst[r][c] = c < C ? src[r][c] : 0 (dY of
 * the 17-joint layer widened to the power-of-two channel count lt_conv_fwd wants on its input); zero fill (scatter targets) */
int lt_add_f32(float* y, const float* x, int64_t n, void* stream);
int lt_pad_channels_f32(const float* src, float* dst, int64_t rows, int32_t C, int32_t c_pad, void* stream);
/* the same with a change of element type on the way (src_dtype / dst_dtype: LT_F32 | LT_BF16, round to nearest even; c_pad == C: a plain cast): the fp32 <-> bf16
 * boundaries of the 16-bit-activation training step (loss gradient in, unprojection backward in / out); 16-byte aligned pointers */
int lt_convert_pad(int32_t src_dtype, const void* src, int32_t dst_dtype, void* dst, int64_t rows, int32_t C, int32_t c_pad, void* stream);
int lt_zero(void* p, int64_t nbytes, void* stream);
/* *ptrs[i] += delta for n int64 scalars in device memory (ptrs: device array of n pointers): BatchNorm's num_batches_tracked counters of a
 * whole network in one launch (torch: one `num_batches_tracked += 1` kernel per layer, pose_resnet.py / v2v.py BatchNorm modules in train()) */
int lt_add_i64_multi(const void* ptrs, int32_t n, int64_t delta, void* stream);
/* backward of lt_global_avgpool (GlobalAveragePoolingHead's mean over the map, pose_resnet.py:166-168): dx[n][p][c] (=|+=) dy[n][c] / HW */
int lt_global_avgpool_bwd(const float* dy, float* dx, int32_t N, int32_t HW, int32_t C, int32_t accumulate, void* stream);
/* dy / dx of element type `dtype` (LT_F32 | LT_BF16: the 16-bit-activation training step) */
int lt_global_avgpool_bwd_dt(int32_t dtype, const void* dy, void* dx, int32_t N, int32_t HW, int32_t C, int32_t accumulate, void* stream);
/* fp32 -> bf16, round to nearest even (operands of the mixed-precision training convolutions); 16-byte aligned pointers */
int lt_cast_f32_bf16(const float* src, void* dst, int64_t n, void* stream);
/* ---- fp8 (e4m3) operands for lt_conv_fwd(dtype = LT_FP8): per-tensor amax scaling, scale = amax / 448 (the largest e4m3 value), q = rne(x / scale).
 * lt_amax_f32     : *amax = max(*amax, max_i |x[i]|)  (zero *amax first, e.g. with lt_zero; an exact, order-independent maximum of non-negative
 *                   floats taken with integer atomics on their bit patterns: bitwise repeatable);
 * lt_quant_fp8    : q[i] = e4m3(x[i] / scale) with scale = *amax > 0 ? *amax / 448 : 1; writes the scale to *scale_out (device) -- the caller
 *                   multiplies the two operands' scales into lt_conv_fwd's `scale` array with lt_scale_product;
 * lt_gather_f32_fp8: the same for weights in one pass with the layout change of lt_gather_f32: q[i] = idx[i] >= 0 ? e4m3(src[idx[i]] / scale) : 0;
 * lt_scale_product: dst[i] = *a * *b for i < n. */
int lt_amax_f32(const float* x, int64_t n, float* amax, void* stream);
int lt_quant_fp8(const float* x, void* q, int64_t n, const float* amax, float* scale_out, void* stream);
/* the same two over a tensor of element type `dtype` (LT_F32 | LT_BF16: the bf16 activations / gradients of the 16-bit-activation training step) */
int lt_amax_dt(int32_t dtype, const void* x, int64_t n, float* amax, void* stream);
int lt_quant_fp8_dt(int32_t dtype, const void* x, void* q, int64_t n, const float* amax, float* scale_out, void* stream);
int lt_gather_f32_fp8(const float* src, const int32_t* idx, void* q, int64_t n, const float* amax, float* scale_out, void* stream);
int lt_scale_product(float* dst, int32_t n, const float* a, const float* b, void* stream);
/* many gathers in one launch.  jobs (device memory): njobs records of
 *   { const float* src; const int32_t* idx; float* dst; int64_t n; int32_t first_block; int32_t out_bf16; }   (40 bytes)
 * with first_block = running sum of ceil(n / 1024) over the preceding jobs; total_blocks = that sum over all jobs; out_bf16 != 0: dst is a bf16
 * array (the values are rounded to nearest even). */
int lt_gather_f32_multi(const void* jobs, int32_t njobs, int32_t total_blocks, void* stream);
/* the same update for MANY tensors in one launch.  jobs (device memory): njobs records of
 *   { float* param; const float* grad; float* exp_avg; float* exp_avg_sq; int64_t n; float lr; int32_t first_block; }   (48 bytes)
 * with first_block = running sum of ceil(n / 1024) over the preceding jobs; total_blocks = that sum over all jobs. */
int lt_adam_step_multi(const void* jobs, int32_t njobs, int32_t total_blocks, double beta1, double beta2, float eps, float weight_decay, int32_t step,
                       void* stream);
int lt_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float lr, double beta1, double beta2, float eps,
                 float weight_decay, int32_t step, void* stream);

/* multiview.triangulate_batch_of_points (mvn/utils/multiview.py:141-183): confidence-weighted DLT.
 * proj B,NV,3,4; points B,NV,J,2; conf B,NV,J or NULL; out B,J,3.  Smallest right singular vector
 * of the (2NV x 4) system in fp64: rows formed in fp64 from the fp32 inputs, Givens QR, one-sided Jacobi SVD of R. */
int lt_triangulate_dlt(const float* proj, const float* points, const float* conf, float* out, int32_t B, int32_t NV,
                       int32_t J, void* stream);
/* AlgebraicTriangulationNet after the 2D soft-argmax (reference triangulation.py:166-193), every (sample, joint) in one launch:
 *   confidences = raw / (sum of raw over the views) + 1e-5   (raw: conf_raw[(b * NV + v) * ld_conf + j], the alg_confidences head's sigmoid
 *                                                             outputs; conf_raw NULL = uniform 1, i.e. 1 / NV + 1e-5)
 *   keypoints_2d = keypoints_hm * (scale_x, scale_y)          (heatmap -> image pixels; pass f32(W / w), f32(H / h))
 *   keypoints_3d = the DLT of lt_triangulate_dlt on (keypoints_2d, confidences)
 * keypoints_hm B*NV,J,2 (lt_softargmax2d_fwd's coords); proj B,NV,3,4 at image resolution; outputs keypoints_2d B,NV,J,2 and confidences
 * B,NV,J (either may be NULL), keypoints_3d B,J,3.  Bit-identical to the torch sequence conf / conf.sum(1) + 1e-5, kp * scale,
 * lt_triangulate_dlt: one IEEE rounding per step, no contraction, the view sum in the order of torch's GPU reduction (four
 * interleaved partial sums, view v into partial v % 4; plain view order up to four views).  NV >= 2. */
int lt_alg_tail_fwd(const float* keypoints_hm, const float* conf_raw, int32_t ld_conf, const float* proj, float scale_x, float scale_y,
                    float* keypoints_2d, float* confidences, float* keypoints_3d, int32_t B, int32_t NV, int32_t J, void* stream);
/* lt_alg_tail_fwd over the VALID views of every sample (view_mask: DEVICE (B, NV) uint8, non-zero = valid; NULL is LT_ERR_INVALID):
 *   confidences = raw / (sum of raw over the valid views) + 1e-5 for a valid view, exactly 0 for a masked one; the k-th valid view goes into
 *                 partial k % 4 of the view sum, i.e. what lt_alg_tail_fwd does on the compacted views;
 *   keypoints_2d is written for every view (a masked view's value is unspecified: its keypoints_hm times the scale);
 *   keypoints_3d = the DLT over the rows of the valid views only, in increasing v: a masked view's keypoints and projection matrix do not
 *                  enter the system, so NaN there cannot leak.  Bit-identical to lt_alg_tail_fwd on the compacted views.
 * A sample with fewer than two valid views gets NaN joints (the model and plan layers refuse such a mask before launching). */
int lt_alg_tail_masked_fwd(const float* keypoints_hm, const float* conf_raw, int32_t ld_conf, const float* proj, float scale_x, float scale_y,
                           const uint8_t* view_mask, float* keypoints_2d, float* confidences, float* keypoints_3d, int32_t B, int32_t NV,
                           int32_t J, void* stream);
/* lt_alg_tail_fwd over ragged view batches (the layout of lt_unproject_ragged_fwd): keypoints_hm and keypoints_2d T,J,2, conf_raw T,ld_conf,
 * confidences T,J, proj T,3,4, keypoints_3d B,J,3; view_base DEVICE (B + 1) int32.  Sample b is lt_alg_tail_fwd on its rows view_base[b] ..
 * view_base[b+1] alone: confidences normalised over the sample's views + 1e-5, its k-th view into partial k % 4, the DLT over exactly those rows in
 * order -- bit-identical to lt_alg_tail_masked_fwd on the inputs padded to (B, NVcap) with a prefix mask.  The count is clamped into
 * [0, min(NVcap, T)] and the first row into [0, T - count] on the device; a sample with fewer than two views gets NaN joints (the hosts refuse
 * such counts before launching).  NULL keypoints_hm, proj, keypoints_3d or view_base, B < 1, T < 1, J < 1, NVcap outside [1, 32]: LT_ERR_INVALID. */
int lt_alg_tail_ragged_fwd(const float* keypoints_hm, const float* conf_raw, int32_t ld_conf, const float* proj, float scale_x, float scale_y,
                           const int32_t* view_base, float* keypoints_2d, float* confidences, float* keypoints_3d, int32_t B, int32_t T,
                           int32_t NVcap, int32_t J, void* stream);
/* The algebraic tail with the statistics of its joints (mvn.utils.multiview.triangulation_stats states them in numpy fp64).  view_mask NULL:
 * keypoints_2d, confidences and keypoints_3d are bit for bit lt_alg_tail_fwd's; view_mask DEVICE (B, NV): lt_alg_tail_masked_fwd's (same loops, same
 * dlt_add_view / SVD sequence).  stats2d: the B*NV*J,5 records of lt_softargmax2d_stats_fwd for keypoints_hm.  Additional outputs:
 *   cov2d_img  B,NV,J,3 {xx, xy, yy}, image px^2: S Sigma_hm S, S = diag(scale_x, scale_y), Sigma_hm the record's {cxx, cxy, cyy}; formed in fp64,
 *              rounded once.  It is the spread of the network's heatmap, not a calibrated error bar.
 *   reproj_err B,NV,J, image px: || pi(P_v, X) - keypoints_2d[b, v, j] ||_2, pi the perspective division of P_v [X; 1], X the RETURNED fp32 joint read
 *              back as fp64; fp64, rounded once.
 *   cov3d      B,J,6 {xx, xy, xz, yy, yz, zz}, squared world units of proj (mm^2 for Human3.6M): sum over the valid views of J_v Sigma_v J_v^T, the
 *              first-order propagation with the confidences held fixed; Sigma_v = the RETURNED cov2d_img[b, v, j] read back as fp64 (so a caller can
 *              reproduce cov3d from the outputs alone), J_v = dX / d keypoints_2d[b, v, j] (3 x 2) at the solution, by the formulas of
 *              lt_triangulate_dlt_bwd: w = (lambda I - A^T A)^+ g_v, dL/dA = A (w v^T + v w^T), for g_X = e_0, e_1, e_2 off the forward's one SVD.
 * A masked view adds nothing to cov3d, its reproj_err is a quiet NaN, its cov2d_img is unspecified, and its keypoint, matrix and record never enter
 * the system.  Fewer than two valid views: NaN joints, NaN cov3d.  LT_ERR_INVALID: stats2d, cov2d_img, reproj_err or cov3d NULL; otherwise the
 * refusals of lt_alg_tail_fwd (NV >= 2). */
int lt_alg_tail_stats_fwd(const float* keypoints_hm, const float* conf_raw, int32_t ld_conf, const float* proj, float scale_x, float scale_y,
                          const uint8_t* view_mask, const float* stats2d, float* keypoints_2d, float* confidences, float* keypoints_3d,
                          float* cov2d_img, float* reproj_err, float* cov3d, int32_t B, int32_t NV, int32_t J, void* stream);
/* lt_triangulate_dlt over the valid views (view_mask DEVICE (B, NV) or NULL = all valid) with the two statistics of lt_alg_tail_stats_fwd, for
 * callers that hold the 2D points, the confidences (as they enter the system; NULL = 1) and the 2D covariances cov2d (B,NV,J,3 {xx, xy, yy}) already:
 * out B,J,3; reproj_err B,NV,J; cov3d B,J,6.  Given lt_alg_tail_stats_fwd's keypoints_2d, confidences and cov2d_img it returns that call's joints,
 * reproj_err and cov3d bit for bit.  LT_ERR_INVALID: a NULL pointer other than conf and view_mask, NV < 2. */
int lt_triangulate_dlt_stats(const float* proj, const float* points, const float* conf, const float* cov2d, const uint8_t* view_mask, float* out,
                             float* reproj_err, float* cov3d, int32_t B, int32_t NV, int32_t J, void* stream);

/* RANSACTriangulationNet (reference mvn/models/triangulation.py:17-128), 2D part: the backbone's N,h,w,(ld) fp32 heatmaps ->
 * heatmaps_nchw N,J,h,w (the raw heatmaps the model returns, bit-identical to lt_nhwc_to_nchw_f32) and, in the same pass, the argmax
 * of torch.max(hm.view(N, J, -1), -1): indices N,J int64 (or NULL; a NaN wins with the first NaN's index, a tie goes to the smallest
 * index) and keypoints N,J,2 int64 (or NULL) = (trunc(idx % w * f32(image_w / w)), trunc(idx / w * f32(image_h / h))), the
 * reference's float products stored into an int64 tensor (:45-52).  J <= 32. */
int lt_heatmap_argmax_nchw_f32(const float* heatmaps, int32_t ld, float* heatmaps_nchw, int64_t* indices, int64_t* keypoints,
                               int32_t N, int32_t J, int32_t h, int32_t w, int32_t image_h, int32_t image_w, void* stream);
/* RANSACTriangulationNet.triangulate_ransac (reference :75-128) for every (sample, joint), fp64 inside.  proj B,NV,3,4 fp32;
 * points B,NV,J,2 int64; pairs B,J,n_iters,2 int32 = the 2-view hypotheses to try, in order (the reference's random draws), or
 * NULL = every pair (a, b), a < b, in lexicographic order (exhaustive: always at least as large an inlier set as any draw; n_iters
 * is then ignored).  A draw with an index outside [0, NV) or with two equal indices is skipped (nothing outside the problem is read);
 * the two indices of a valid draw may come in either order.  A hypothesis' inlier set = the pair + every view with reprojection error
 * 1/2 |p - pi(X)| < eps, kept when strictly larger than the best so far (among sets of equal size the first found stays); no valid draw
 * at all: the inlier set is all NV views.  The final DLT on the inliers is refined with direct_opt by minimising scipy's
 * least_squares(loss='huber') objective.  out_kp3d B,J,3 fp32; out_inliers B,J,NV uint8 (1 = inlier) or NULL.  2 <= NV <= 32. */
int lt_triangulate_ransac(const float* proj, const int64_t* points, const int32_t* pairs, int32_t n_iters, double eps, int32_t direct_opt,
                          float* out_kp3d, uint8_t* out_inliers, int32_t B, int32_t NV, int32_t J, void* stream);

/* Per-view image preparation of the reference dataset (mvn/datasets/human36m.py:116-189, mvn/utils/img.py) for a ragged batch of N
 * views in one launch: crop to the bbox with zero fill outside the region (PIL crop), cv2.resize(INTER_AREA) of the uint8 crop to
 * H x W, reproduced branch by branch on 8UC3 (identity, integer factors, general area downscale bit-exact; any upscaled axis is
 * OpenCV's fixed-point bilinear "area mode" with its scalar rounding), then out[n,c,y,x] = lut[c*256 + v] (lut 3 x 256 fp32, e.g. the
 * fp32 of normalize_image) or (float)v when lut is NULL.  Channel order is kept.
 *   src      flat uint8 buffer of HWC 3-channel pixels, src_bytes long;
 *   desc     N x 8 int64: byte offset into src, region height, width, row pitch in bytes, bbox left, upper, right, lower relative to the
 *            region (may lie partly or wholly outside it; a region already cropped to bbox and frame, with the bbox shifted, gives the
 *            same output);
 *   desc_host the same N x 8 records on the host, or NULL: when given, an empty bbox, a region past src_bytes or a bad pitch is
 *            LT_ERR_INVALID before anything is enqueued (without it the device trusts desc; an empty bbox writes zeros);
 *   out      N x 3 x H x W fp32.  W <= 2048, N <= 65535. */
int lt_crop_resize_u8(const uint8_t* src, int64_t src_bytes, const int64_t* desc, const int64_t* desc_host, int32_t N, int32_t H, int32_t W,
                      const float* lut, float* out, void* stream);

/* lt_crop_resize_u8 with on-the-fly lens undistortion in front, for views cut from raw (distorted) frames: crop pixel (y, x) of a view is
 * pixel (upper + y, left + x) of cv2.remap(frame, map1, map2, INTER_CUBIC) (OpenCV 4.x, 8UC3, constant border 0: 4 x 4 taps from
 * (map1.x - 1, map1.y - 1), 15-bit fixed-point Keys weights A = -0.75 of initInterTab2D indexed by map2, taps outside the frame read 0,
 * saturate_u8((sum + (1 << 14)) >> 15)), zero where the bbox leaves the frame; then the same INTER_AREA branches and LUT as
 * lt_crop_resize_u8, one launch for N views.  The maps are built on the host (mvn/utils/img.py:undistort_maps) and only read here.
 *   src      flat uint8 buffer of HWC 3-channel source windows, src_bytes long;
 *   desc     N x 14 int64 per view: [0] byte offset of the source window into src, [1] window height, [2] width, [3] row pitch in
 *            bytes, [4] window x0, [5] y0 in the frame (the window lies inside the frame and must hold every in-frame tap of the
 *            bbox's pixels: mvn/utils/img.py:source_window; a tap outside the window reads 0), [6] frame height, [7] frame width (the
 *            remap's border), [8] bbox left, [9] upper, [10] right, [11] lower in frame coordinates (may leave the frame), [12] byte
 *            offset of the view's map into maps (a multiple of 8), [13] map row pitch in entries (>= frame width);
 *   maps     int16 blocks, 8-byte aligned, maps_bytes long: entry (y, x) of a map = maps[offset / 2 + 4 * (y * pitch + x) + 0..3] =
 *            (map1 x, map1 y, map2, 0) of frame pixel (y, x) (mvn/utils/img.py:device_map); a map covers the whole frame;
 *   desc_host the same N x 14 records on the host, or NULL: when given, an empty bbox, a bad frame size, a window outside the frame or
 *            past src_bytes, a bad pitch, or a map past maps_bytes is LT_ERR_INVALID before anything is enqueued (without it the
 *            device trusts desc; an empty bbox writes zeros);
 *   out      N x 3 x H x W fp32.  W <= 2048, N <= 65535, frame sides <= 32767. */
int lt_undistort_crop_resize_u8(const uint8_t* src, int64_t src_bytes, const int64_t* desc, const int64_t* desc_host, const int16_t* maps,
                                int64_t maps_bytes, int32_t N, int32_t H, int32_t W, const float* lut, float* out, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Chain of up to LT_PWCHAIN_MAX pointwise (1x1x1) convolutions evaluated per voxel without the
 * intermediate activations leaving the registers:  y = L_n(...L_1(x)),
 * L_i(v) = act_i((W_i v + bias_i) * scale_i + shift_i)  (same epilogue constants as lt_conv_fwd).
 * Replaces the tail of V2VModel.forward (mvn/models/v2v.py:157-169: back_layers[1:] =
 * Basic3DBlock(32,32,1) x 2, then output_layer = Conv3d(32, J, 1)): one pass over the volume
 * instead of three.  bf16 activations, 32 input channels, inner widths 32, last width <= 32;
 * intermediate activations are rounded to bf16 exactly where separate launches would store them;
 * the last layer stores fp32: plane == 0 -> rows of ldy == cout[last] floats (channels-last);
 * plane > 0 -> planar, y[((row / plane) * cout[last] + c) * plane + row % plane] with plane = voxels
 * per sample (a multiple of 64 that divides rows) -- the (N, J, V, V, V) layout of the reference's
 * volumes, which is what lt_softargmax3d_fwd streams fastest.  x: rows x 32 bf16 (channels-last
 * volume), rows % 64 == 0.  weight[i]: the lt_conv_fwd packing [32][k_pad[i]] (k = input channel).
 * -------------------------------------------------------------------------------------------*/
#define LT_PWCHAIN_MAX 3
typedef struct {
    int32_t dtype;                       /* LT_BF16 */
    int32_t nlayers;                     /* 1..LT_PWCHAIN_MAX */
    int64_t rows;                        /* voxels */
    int32_t cin;                         /* 32 */
    int32_t ldy;                         /* == cout[nlayers-1] */
    int32_t cout[LT_PWCHAIN_MAX];
    int32_t k_pad[LT_PWCHAIN_MAX];
    int32_t flags[LT_PWCHAIN_MAX];       /* LT_EPI_RELU_POST; LT_EPI_STORE_F32 on the last layer (required) */
    const void* weight[LT_PWCHAIN_MAX];
    const float* bias[LT_PWCHAIN_MAX];   /* 32 entries each (padded), or NULL */
    const float* scale[LT_PWCHAIN_MAX];
    const float* shift[LT_PWCHAIN_MAX];
    int64_t plane;                       /* 0: channels-last output; > 0: planar output, voxels per sample */
} lt_pwchain_desc;
int lt_pwchain_fwd(const lt_pwchain_desc* desc, const void* x, void* y, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The stem of the 2D backbone in one pass: conv 7x7 / stride 2 / pad 3 -> (acc + bias) * scale +
 * shift (eval BatchNorm folded) -> ReLU -> max pool 3x3 / stride 2 / pad 1.  Replaces the first four
 * lines of PoseResNet.forward (mvn/models/pose_resnet.py:293-297: conv1, bn1, relu, maxpool): the
 * half-resolution 64-channel map never goes to HBM.  bf16 only (fp32 plans record lt_conv_fwd +
 * lt_maxpool_fwd); results are identical to those two launches (max commutes with the bf16 rounding).
 * x: N,H,W,8 channels-last (3 image channels zero-padded to 8); y: N,Hp,Wp,64 with Hc = (H-1)/2 + 1,
 * Hp = (Hc-1)/2 + 1.  weight: lt_stem_packed_bytes() bytes filled ONCE per model by
 * lt_stem_pack_weights from the lt_conv_fwd packing [64][k_pad] (k = (kh*7 + kw)*8 + ci, bf16): the
 * kernel's MFMA fragment order, so that a wave reads 1 KB contiguous per K step.
 * -------------------------------------------------------------------------------------------*/
typedef struct {
    int32_t dtype;                       /* LT_BF16 */
    int32_t N, H, W;
    int32_t Cin, Cout;                   /* 8, 64 */
    const void* weight;                  /* packed by lt_stem_pack_weights, 16-byte aligned */
    const float* bias;                   /* 64 entries each, or NULL */
    const float* scale;
    const float* shift;
    int32_t x_layout;                    /* 0: x = N,H,W,8 bf16 (Cin = 8); 1: x = N,3,H,W fp32, the reference's image
                                            tensor (Cin = 3), rounded to bf16 on the fly like lt_nchw_to_nhwc would */
} lt_stem_desc;
size_t lt_stem_packed_bytes(void);
int lt_stem_pack_weights(const void* weight, int32_t k_pad, void* packed, void* stream);
int lt_stem_pool_fwd(const lt_stem_desc* desc, const void* x, void* y, void* stream);

/* ---------------------------------------------------------------------------------------------
 * A whole identity Bottleneck block in one launch: Bottleneck.forward of the reference
 * (mvn/models/pose_resnet.py:75-95 with downsample == None and stride 1):
 *   t1 = relu(bn1(conv1x1(x)));  t2 = relu(bn2(conv3x3(t1), pad 1));  y = relu(bn3(conv1x1(t2)) + x)
 * with eval-mode BatchNorm folded like lt_conv_fwd's epilogue ((acc + bias) * scale + shift).  The two
 * intermediate tensors never leave LDS (they are rounded to bf16 exactly where the three separate launches
 * would store them); x is read once (plus the 1-pixel halo of an 8 x 16 pixel tile) and y written once.
 * x, y: N,H,W,C channels-last bf16, y != x;  (C, P) = (256, 64) or (512, 128) (ResNet layer1 / layer2);
 * H % 8 == 0, W % 16 == 0.  weight[i]: lt_conv_pack_weights_t32 of the lt_conv_fwd packing of layer i
 * (i = 0: [P][C], ntaps 1, cin C;  1: [P][9 P], ntaps 9, cin P;  2: [C][P], ntaps 1, cin P);
 * bias[i] may be NULL; scale / shift hold the layer's output-channel count of floats.
 * -------------------------------------------------------------------------------------------*/
typedef struct {
    int32_t dtype;                       /* LT_BF16 */
    int32_t N, H, W;
    int32_t C, P;                        /* block width, bottleneck width (C == 4 P) */
    const void* weight[3];
    const float* bias[3];
    const float* scale[3];
    const float* shift[3];
} lt_bneck_desc;
int lt_bottleneck_fwd(const lt_bneck_desc* desc, const void* x, void* y, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The FIRST Bottleneck of ResNet layer1 -- the one with a `downsample` branch and stride 1 -- in one launch
 * (mvn/models/pose_resnet.py:75-95 with downsample = conv1x1 + BatchNorm, built at :196-206):
 *   t1 = relu(bn1(conv1x1(x)));  t2 = relu(bn2(conv3x3(t1), pad 1));  y = relu(bn3(conv1x1(t2)) + bn_d(conv1x1_d(x)))
 * Like lt_bottleneck_fwd the two inner tensors stay in LDS; here the residual is not read but COMPUTED from the
 * tile of x that is in LDS already (a second K = Cin GEMM of the output phase), and it is added in fp32 -- the four
 * separate launches round the downsample branch to bf16 first.  x: N,H,W,Cin, y: N,H,W,C channels-last bf16;
 * (Cin, P, C) = (64, 64, 256);  H % 8 == 0, W % 16 == 0.  weight[i]: lt_conv_pack_weights_t32 of the lt_conv_fwd
 * packing of conv1 [P][Cin], conv2 [P][9 P], conv3 [C][P], downsample [C][Cin];  scale / shift [i]: the folded
 * BatchNorm of that layer (ResNet convolutions carry no bias).
 * -------------------------------------------------------------------------------------------*/
typedef struct {
    int32_t dtype;                       /* LT_BF16 */
    int32_t N, H, W;
    int32_t Cin, P, C;                   /* input width, bottleneck width, block width */
    const void* weight[4];               /* conv1, conv2, conv3, downsample */
    const float* scale[4];
    const float* shift[4];
} lt_bneck_ds_desc;
int lt_bottleneck_ds_fwd(const lt_bneck_ds_desc* desc, const void* x, void* y, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The 1x1 EXPAND of one identity Bottleneck block and the 1x1 REDUCE of the next one in one launch
 * (mvn/models/pose_resnet.py:75-95, the seam between two consecutive blocks of a ResNet stage):
 *   y  = relu(bn3(conv1x1_expand(t2)) + residual)          C channels, written once
 *   t1 = relu(bn1'(conv1x1_reduce'(y)))                    P channels, the next block's first activation
 * The reduce consumes y from LDS while the tile is there: the C-channel tensor is not read back from memory.
 * y is rounded to bf16 exactly where the expand's own launch would store it (the reduce sees those values).
 * t2 [M][P], residual / y [M][C], t1 [M][P]: channels-last bf16, M = N * H * W GEMM rows (any M: tiles of
 * 96 / 64 / 32 rows, chosen by M against the device's CU count -- 96 from 7/8 of a round of 96-row tiles on,
 * 64 from 7/16; LT_XR_NPB=3|2|1 forces one -- and a ragged last tile as a second one-workgroup launch with
 * row checks);  (C, P) = (1024, 256): the identity blocks of ResNet layer3.
 * weight[0]: lt_conv_pack_weights_t32 of the expand's lt_conv_fwd packing [C][P] (ntaps 1, cin P);
 * weight[1]: the same of the reduce's [P][C] (ntaps 1, cin C);  scale / shift [i]: the folded BatchNorm of
 * layer i (C / P floats), applied as acc * scale + shift (ResNet convolutions carry no bias).
 * Outputs must not alias the inputs.
 * -------------------------------------------------------------------------------------------*/
typedef struct {
    int32_t dtype;                       /* LT_BF16 */
    int32_t C, P;                        /* block width, bottleneck width (C == 4 P) */
    int64_t M;                           /* GEMM rows */
    const void* weight[2];
    const float* scale[2];
    const float* shift[2];
    const float* consts;                 /* optional (may be NULL): scale[0] | shift[0] | scale[1] | shift[1] back to back (2 C + 2 P floats,
                                            16-byte aligned): the kernel then fetches the four tables with one LDS-DMA instead of four dependent loads */
} lt_xr_desc;
int lt_expand_reduce_fwd(const lt_xr_desc* desc, const void* t2, const void* residual, void* y, void* t1_next, void* stream);

/* ---------------------------------------------------------------------------------------------
 * hipGraph + event helpers (the forward is ~230 launches: replay it as one graph)
 * -------------------------------------------------------------------------------------------*/
int lt_graph_begin(void* stream);
int lt_graph_end(void* stream, void** graph_exec_out);
int lt_graph_launch(void* graph_exec, void* stream);
int lt_graph_destroy(void* graph_exec);
int lt_event_create(void** ev_out);
int lt_event_record(void* ev, void* stream);
int lt_event_elapsed_ms(void* ev_start, void* ev_stop, float* ms_out); /* synchronises on ev_stop */
int lt_event_destroy(void* ev);

/* ---------------------------------------------------------------------------------------------
 * PLAN-LEVEL entry points ("whole-network plan entry points that own pre-packed weights and a hipGraph"; round 6).
 * Everything the Python host does between the reference's module API and the kernel-level calls above lives behind these six symbols, for all three
 * of the reference's models (volumetric: _vol; algebraic and RANSAC: _alg; lt_plan_info / lt_plan_destroy: any plan), so that a
 * host in any language can run the timed forward: layer -> kernel selection with every batch threshold (fused stem, whole-bottleneck launches, the
 * layer3 seam kernel, conv_cat2, the 2D / 3D halo kernels by weight layout, split-K of the tiny V2V levels, the pointwise tail), the eval-BatchNorm fold
 * as ATen evaluates it, weight packing (GEMM layout, MFMA fragment orders, parity phases of the stride-2 transposed convolutions), buffer reuse, the
 * fp64 camera algebra of the reference's forward, and the captured hipGraph.
 *
 * lt_plan_create_vol  = VolumetricTriangulationNet.__init__ + load_state_dict + the first forward's plan recording
 *                       (mvn/models/triangulation.py:204-242, mvn/models/pose_resnet.py:177-377, mvn/models/v2v.py:142-180).
 *   weights: the reference's state_dict -- names as torch writes them ("backbone.layer3.0.conv1.weight", "volume_net.front_layers.0.block.0.bias", ...;
 *   a leading "module." is stripped like train.py:408-410), HOST fp32 arrays in torch's layout; keys the volumetric path does not use
 *   (backbone.final_layer.*, num_batches_tracked) are ignored; a missing key is LT_ERR_INVALID with its name.  The arrays are read during this call only.
 *   One plan = one input shape (B, NV, H, W) and one element type: LT_F32 (exact-fp32 MFMA: the kernel set that meets the 1e-4 joint tolerance) or
 *   LT_BF16 (the throughput set).  Allocates device memory (hipMalloc) that lt_plan_destroy frees.
 * lt_plan_forward_vol = VolumetricTriangulationNet.forward (triangulation.py:245-355) for inference (eval-mode BatchNorm).
 *   images: DEVICE (B, NV, 3, H, W) fp32, the reference's input tensor.  Cameras: HOST fp64 K (B, NV, 3, 3) at IMAGE resolution, R (B, NV, 3, 3),
 *   t (B, NV, 3) -- batch['cameras'][view][sample] of the reference (datasets/utils.py:26), sample-major here; the call rescales K to the heatmap
 *   resolution and forms K [R | t] in fp64 like Camera.update_after_resize / .projection (multiview.py:33-52).  base_points: HOST (B, 3) fp64, the
 *   pelvis the cuboid is centred on (triangulation.py:284-296: batch['pred_keypoints_3d'][b][6] for kind 'mpii').  rot: HOST (B, 9) fp64 row-major
 *   cuboid rotations (triangulation.py:318-328) or NULL = identity (what eval mode draws).
 *   Outputs, DEVICE fp32, written on `stream`: keypoints_3d (B, J, 3) [required]; volumes (B, J, V, V, V) softmaxed / ReLU'd (NULL: kept in a plan
 *   buffer); features (B, NV, 32, h, w) or NULL; coord_volumes (B, V, V, V, 3) or NULL; vol_confidences (B, NV, 32) RAW head outputs or NULL (only for
 *   LT_AGG_CONF / LT_AGG_CONF_NORM plans; the reference returns them divided by their sum over views for 'conf_norm').  cuboids / base_points of the
 *   reference's 7-tuple are host values the caller already has.  Asynchronous; the first call captures the hipGraph (use_graph), later calls replay it.
 *   stream == NULL with use_graph: the legacy default stream cannot be captured, so the forward runs on a stream the plan owns, ordered behind the default
 *   stream's earlier work and in front of its later work by events.  Not thread-safe per plan (one forward of a plan at a time).
 * lt_plan_create_alg  = AlgebraicTriangulationNet (reference triangulation.py:131-200, cfg.model = LT_MODEL_ALG) or RANSACTriangulationNet (:17-128,
 *                       LT_MODEL_RANSAC, eval only) + load_state_dict + the plan recording.  weights as for lt_plan_create_vol; ALG reads the backbone with
 *   backbone.final_layer.* and, with use_confidences, backbone.alg_confidences.*; RANSAC the backbone with backbone.final_layer.*.  Config errors (model,
 *   dtype, shape, RANSAC's num_joints <= 32 and 2 <= NV <= 32) are LT_ERR_INVALID before any device call.  The captured part is the backbone with
 *   final_layer (and the confidence head) and the heatmaps' NCHW pass (RANSAC: lt_heatmap_argmax_nchw_f32); the tail runs eagerly on every call
 *   (ALG: lt_softargmax2d_fwd + lt_alg_tail_fwd; RANSAC: lt_triangulate_ransac over every view pair), so the graph holds no caller pointer.
 * lt_plan_forward_alg = the eval forward of that model.  images: DEVICE (B, NV, 3, H, W) fp32; proj: DEVICE fp32 (B, NV, 3, 4), the reference's
 *   proj_matricies_batch at image resolution.  Outputs, DEVICE, written on `stream`; all but keypoints_3d may be NULL:
 *     ALG     keypoints_3d (B, J, 3) fp32; keypoints_2d (B, NV, J, 2) fp32 image pixels; heatmaps (B, NV, J, h, w) after integrate_tensor_2d
 *             (softmax or ReLU-normalised); confidences (B, NV, J) normalised over the views + 1e-5 (uniform 1 / NV + 1e-5 without the head).
 *     RANSAC  keypoints_3d (B, J, 3) fp32; keypoints_2d (B, NV, J, 2) INT64 argmax pixels; heatmaps (B, NV, J, h, w) raw; confidences zeros.
 *   Streams, graph capture and threading as lt_plan_forward_vol.  lt_plan_forward_vol on an algebraic / RANSAC plan and lt_plan_forward_alg on a
 *   volumetric plan are LT_ERR_INVALID.  lt_plan_info describes any plan: the census fields count the backbone's fused kernels (the V2V ones are 0).
 * -------------------------------------------------------------------------------------------*/
typedef struct lt_plan lt_plan;
typedef struct lt_named_tensor {
    const char* name;        /* state_dict key */
    const float* data;       /* HOST fp32, contiguous, torch's layout (Conv: [Cout][Cin][k..]; ConvTranspose: [Cin][Cout][k..]; Linear: [out][in]) */
    int32_t ndim;            /* 1 .. 5 */
    int64_t shape[5];
} lt_named_tensor;
typedef struct lt_vol_plan_config {
    int32_t dtype;                        /* LT_F32 | LT_BF16 */
    int32_t num_layers;                   /* config.model.backbone.num_layers: 18 | 34 | 50 | 101 | 152 */
    int32_t style_caffe;                  /* config.model.backbone.style == "caffe" */
    int32_t num_joints;                   /* 17 */
    int32_t B, NV, H, W;                  /* samples, views per sample, image size */
    int32_t volume_size;                  /* config.model.volume_size (64) */
    double cuboid_side;                   /* config.model.cuboid_side (2500.0 mm) */
    double volume_multiplier;             /* config.model.volume_multiplier */
    int32_t volume_softmax;               /* config.model.volume_softmax */
    int32_t aggregation;                  /* LT_AGG_* of config.model.volume_aggregation_method */
    int32_t transfer_cmu_to_human36m;     /* config.model.transfer_cmu_to_human36m (triangulation.py:336-339) */
    int32_t use_graph;                    /* capture the forward into a hipGraph at the first call and replay it */
} lt_vol_plan_config;
typedef struct lt_plan_info_t {
    int32_t launches;                     /* ops of one forward (pre + captured + tail) */
    int32_t heatmap_h, heatmap_w;         /* h, w of the feature maps (H / 4, W / 4) */
    double flops;                         /* 2 * MAC of the recorded convolutions */
    int64_t bytes_allocated;              /* device memory owned by the plan */
    int32_t n_expand_reduce, n_bottleneck, n_bottleneck_ds, n_conv_cat2, n_conv2d_halo, n_pwchain, n_stem_pool, n_splitk, n_conv_skip;   /* which fused kernels it recorded */
    int32_t graph_captured;
    const float* logits;                  /* V2V logits (fp32; planar (B, J, V, V, V) when logits_planar, else channels-last (B, V, V, V, J)): valid after a forward, for tests */
    int32_t logits_planar;
} lt_plan_info_t;
int lt_plan_create_vol(const lt_vol_plan_config* cfg, const lt_named_tensor* weights, int32_t nweights, lt_plan** plan_out);
int lt_plan_forward_vol(lt_plan* plan, const float* images, const double* K_host, const double* R_host, const double* t_host, const double* base_points_host,
                        const double* rot_host, float* keypoints_3d, float* volumes, float* features, float* coord_volumes, float* vol_confidences, void* stream);
enum { LT_MODEL_ALG = 1, LT_MODEL_RANSAC = 2 };
typedef struct lt_alg_plan_config {
    int32_t model;                        /* LT_MODEL_ALG (AlgebraicTriangulationNet) | LT_MODEL_RANSAC (RANSACTriangulationNet, eval only) */
    int32_t dtype;                        /* LT_F32 | LT_BF16 */
    int32_t num_layers;                   /* config.model.backbone.num_layers: 18 | 34 | 50 | 101 | 152 */
    int32_t style_caffe;                  /* config.model.backbone.style == "caffe" */
    int32_t num_joints;                   /* 17 */
    int32_t B, NV, H, W;                  /* samples, views per sample, image size */
    int32_t use_confidences;              /* ALG: config.model.use_confidences (the alg_confidences head) */
    int32_t heatmap_softmax;              /* ALG: config.model.heatmap_softmax */
    double heatmap_multiplier;            /* ALG: config.model.heatmap_multiplier */
    int32_t direct_optimization;          /* RANSAC: config.model.direct_optimization */
    double reprojection_error_epsilon;    /* RANSAC: 15 in the reference */
    int32_t use_graph;                    /* capture the forward into a hipGraph at the first call and replay it */
} lt_alg_plan_config;
int lt_plan_create_alg(const lt_alg_plan_config* cfg, const lt_named_tensor* weights, int32_t nweights, lt_plan** plan_out);
int lt_plan_forward_alg(lt_plan* plan, const float* images, const float* proj, float* keypoints_3d, void* keypoints_2d, float* heatmaps,
                        float* confidences, void* stream);
/* The cascade: the reference's two-stage evaluation route (an algebraic run writes pred_results_path, the volumetric run centres its cuboid on that
 * pelvis; eval/human36m_vol_softmax.yaml, use_gt_pelvis: false) as ONE forward.  The plan holds an algebraic and a volumetric plan of the same input shape;
 * the algebraic stage's joints stay on the device, lt_cuboid_from_keypoints turns them into the volumetric plan's cuboid origins behind the geometry copy
 * on the same stream: nothing between the stages waits for the GPU or copies to the host.
 * lt_plan_create_cascade: cfg.alg.model must be LT_MODEL_ALG; cfg.vol's B, NV, H, W must equal cfg.alg's; kind LT_KIND_MPII | LT_KIND_COCO with
 *   alg.num_joints >= 7 / 13.  Any of these wrong (and every config error of the two create calls) is LT_ERR_INVALID before any device call.
 *   alg_weights / vol_weights: the two state dicts, as for lt_plan_create_alg / lt_plan_create_vol (the reference's checkpoints are separate networks).
 * lt_plan_forward_cascade: images DEVICE (B, NV, 3, H, W) fp32; cameras HOST fp64 at IMAGE resolution as for lt_plan_forward_vol, given once: the call
 *   forms the algebraic stage's K [R | t] in fp64 and rounds it to fp32 (datasets/utils.py:prepare_batch) and the heatmap-resolution projections as
 *   lt_plan_forward_vol does.  rot_host as lt_plan_forward_vol (NULL = identity).  Outputs, DEVICE fp32, on `stream`: keypoints_3d (B, J, 3) of the
 *   volumetric stage [required]; alg_keypoints_3d (B, J_alg, 3) of the algebraic stage and base_points (B, 3), the pelvis the cuboid is centred on
 *   (NULL: kept in plan buffers); volumes, features, coord_volumes, vol_confidences as lt_plan_forward_vol.  Both stages run with use_graph as their
 *   configs say.  The result is bit-identical to lt_plan_forward_alg, a copy of its joints to the host, and lt_plan_forward_vol on them.
 * lt_plan_info on a cascade plan sums both stages (heatmap size and logits: the volumetric stage's); lt_plan_forward_vol / lt_plan_forward_alg on a
 * cascade plan, and lt_plan_forward_cascade on any other plan, are LT_ERR_INVALID. */
typedef struct lt_cascade_plan_config {
    lt_alg_plan_config alg;               /* model must be LT_MODEL_ALG */
    lt_vol_plan_config vol;               /* B, NV, H, W must equal alg's */
    int32_t kind;                         /* config.model.kind of the volumetric model: LT_KIND_MPII | LT_KIND_COCO */
} lt_cascade_plan_config;
int lt_plan_create_cascade(const lt_cascade_plan_config* cfg, const lt_named_tensor* alg_weights, int32_t n_alg, const lt_named_tensor* vol_weights,
                           int32_t n_vol, lt_plan** plan_out);
int lt_plan_forward_cascade(lt_plan* plan, const float* images, const double* K_host, const double* R_host, const double* t_host, const double* rot_host,
                            float* keypoints_3d, float* alg_keypoints_3d, float* base_points, float* volumes, float* features, float* coord_volumes,
                            float* vol_confidences, void* stream);
/* Several cuboids per frame (VolumetricTriangulationNet.forward with batch["cuboid_frame"]): the backbone runs once on the cfg->B frames, and
 * the gather (lt_unproject_grid_indexed_fwd), V2V and the soft-argmax run on P cuboids, cuboid p over the views of frame cuboid_frame[p].
 * lt_plan_create_vol_multi: lt_plan_create_vol with cfg->B = the frames F and P >= 1 cuboids.  lt_vol_plan_config and lt_plan_info_t keep their
 *   layout; lt_plan_info reports the frames.  P < 1 (and every config error of lt_plan_create_vol) is LT_ERR_INVALID before any device call.
 * lt_plan_forward_vol_multi: images DEVICE (F, NV, 3, H, W) fp32 and the cameras HOST fp64 (F, NV, ...) as for lt_plan_forward_vol, per FRAME;
 *   cuboid_frame_host HOST (P) int32 in [0, F), any order (a frame may have no cuboid; a value outside is LT_ERR_INVALID before any device call, the
 *   message names the entry); base_points_host HOST (P, 3) fp64 and rot_host HOST (P, 9) fp64 or NULL, per CUBOID.  Outputs, DEVICE fp32:
 *   keypoints_3d (P, J, 3) [required]; volumes (P, J, V, V, V); features (F, NV, 32, h, w); coord_volumes (P, V, V, V, 3); vol_confidences
 *   (F, NV, 32) raw; each NULL as for lt_plan_forward_vol.  The assignment travels with the geometry block's copy, outside the captured graph: a
 *   new assignment on a captured plan is just another forward.
 * lt_plan_forward_vol on a multi plan, and lt_plan_forward_vol_multi on any other plan, are LT_ERR_INVALID.  lt_plan_set_view_mask (mask (F, NV):
 * it applies to every cuboid of its frame) and lt_plan_set_keypoint_stats (P rows) work as on a volumetric plan.  Results are bit-identical to the
 * Python host's. */
int lt_plan_create_vol_multi(const lt_vol_plan_config* cfg, int32_t P, const lt_named_tensor* weights, int32_t nweights, lt_plan** plan_out);
int lt_plan_forward_vol_multi(lt_plan* plan, const float* images, const double* K_host, const double* R_host, const double* t_host,
                              const int32_t* cuboid_frame_host, const double* base_points_host, const double* rot_host, float* keypoints_3d,
                              float* volumes, float* features, float* coord_volumes, float* vol_confidences, void* stream);
/* Ragged view batches at plan level: B samples with different numbers of views, T = sum(n_b) images in all, sample 0's views first (the layout of
 * lt_unproject_ragged_fwd).  cfg->B = the samples, cfg->NV = NVcap, the most views a sample may have (1 .. 32; 4 and 8 reach the fused gather under its
 * usual conditions); the config structs and lt_plan_info_t keep their layout.  The backbone is recorded at T images; the gather is
 * lt_unproject_grid_ragged_fwd, the algebraic tail lt_alg_tail_ragged_fwd.  The B + 1 offsets are formed from view_counts_host (HOST int32[B]) at every
 * forward and travel outside the captured graph: other counts with the same (B, T, NVcap) are another forward of the plan.
 * lt_plan_create_vol_ragged / lt_plan_forward_vol_ragged: as lt_plan_create_vol / lt_plan_forward_vol with images DEVICE (T, 3, H, W), K, R, t HOST fp64 per
 *   image (T), base_points_host and rot_host per sample (B); outputs as lt_plan_forward_vol with features (T, 32, h, w) and vol_confidences (T, 32) (raw).
 *   Counts 1 .. NVcap.  lt_plan_set_keypoint_stats works (B rows).
 * lt_plan_create_alg_ragged / lt_plan_forward_alg_ragged: model LT_MODEL_ALG only; images (T, 3, H, W), proj DEVICE (T, 3, 4); keypoints_3d (B, J, 3),
 *   keypoints_2d (T, J, 2) fp32, heatmaps (T, J, h, w), confidences (T, J).  Counts 2 .. NVcap.
 * LT_ERR_INVALID before any device call: NVcap outside 1 .. 32, T outside [B (algebraic: 2 B), B NVcap], counts outside their range or not summing to T
 * (the message names the sample), the plain forwards (lt_plan_forward_vol, _vol_multi, _alg) on a ragged plan and the ragged forwards on any other plan,
 * lt_plan_set_view_mask on a ragged plan (drop the view from the batch instead).  LT_ERR_UNSUPPORTED: lt_plan_set_alg_keypoint_stats on a ragged plan.
 * Results are bit-identical to the Python host's (batch["view_counts"]). */
int lt_plan_create_vol_ragged(const lt_vol_plan_config* cfg, int32_t T, const lt_named_tensor* weights, int32_t nweights, lt_plan** plan_out);
int lt_plan_forward_vol_ragged(lt_plan* plan, const float* images, const double* K_host, const double* R_host, const double* t_host,
                               const int32_t* view_counts_host, const double* base_points_host, const double* rot_host, float* keypoints_3d,
                               float* volumes, float* features, float* coord_volumes, float* vol_confidences, void* stream);
int lt_plan_create_alg_ragged(const lt_alg_plan_config* cfg, int32_t T, const lt_named_tensor* weights, int32_t nweights, lt_plan** plan_out);
int lt_plan_forward_alg_ragged(lt_plan* plan, const float* images, const float* proj, const int32_t* view_counts_host, float* keypoints_3d,
                               void* keypoints_2d, float* heatmaps, float* confidences, void* stream);
/* Per-sample view masks: mask_host is HOST (B, NV) uint8, non-zero = the view is there, NULL = all valid.  Sample b of every later forward gets what
 * the plan gives for that sample on its valid views alone: the gather skips masked views (lt_unproject_grid_masked_fwd), the algebraic tail normalises
 * the confidences over the valid views and forms the DLT from their rows (lt_alg_tail_masked_fwd: masked confidences are 0); a cascade plan applies the
 * one mask to both stages.  Features, heatmaps and 2D keypoints of masked views are unspecified; the backbone still runs on them.
 *   The FIRST call must come before the plan's first forward: it makes the plan a masked plan (what is launched and captured is chosen there);
 *   afterwards a first call is LT_ERR_INVALID.  Later calls replace the mask; it persists until replaced.  The mask travels with the geometry
 *   block's copy (volumetric / cascade plans: same pinned ring, same hipMemcpyAsync) or, for algebraic plans, by one small copy of its own when it
 *   has changed -- outside the captured graph, so a new mask on a captured plan is just another forward.
 *   LT_ERR_INVALID (the message names the sample): a sample without a valid view (volumetric plans) or with fewer than two (algebraic, cascade).
 *   LT_ERR_UNSUPPORTED: an LT_MODEL_RANSAC plan.  Results are bit-identical to the Python host's forward with batch["view_mask"]. */
int lt_plan_set_view_mask(lt_plan* plan, const uint8_t* mask_host);
/* Per-joint statistics of the volumetric joints (the definitions of lt_softargmax3d_stats_fwd, with the plan's volume_multiplier and volume_softmax):
 * with both pointers non-NULL every later forward of a volumetric or cascade plan also writes stats_dev (DEVICE, B,J,8 fp32 records {peak, mass, cxx,
 * cxy, cxz, cyy, cyz, czz}) and peak_index_dev (DEVICE, B,J int32) on the forward's stream; every other output keeps its bits.  Both NULL: back to the
 * plain tail.  One NULL: LT_ERR_INVALID.  LT_MODEL_ALG / LT_MODEL_RANSAC plans: LT_ERR_UNSUPPORTED.  The tail op is eager and reads these fields when it
 * runs, so the call may come before or after the plan's first forward and nothing is captured again. */
int lt_plan_set_keypoint_stats(lt_plan* plan, float* stats_dev, int32_t* peak_index_dev);
/* Per-joint statistics of the algebraic joints (the definitions of lt_softargmax2d_stats_fwd and lt_alg_tail_stats_fwd, with the plan's
 * heatmap_multiplier and heatmap_softmax): with all five pointers non-NULL every later lt_plan_forward_alg of an LT_MODEL_ALG plan -- and the algebraic
 * stage of every later lt_plan_forward_cascade -- also writes, on the forward's stream, stats2d_dev (DEVICE, B*NV*J,5 fp32 {peak, mass, cxx, cxy, cyy},
 * heatmap px^2), peak_index_dev (B*NV*J int32), cov2d_img_dev (B,NV,J,3, image px^2), reproj_err_dev (B,NV,J, px) and cov3d_dev (B,J,6); every other
 * output keeps its bits, with lt_plan_set_view_mask too.  All five NULL: back to the plain tail.  A mixture: LT_ERR_INVALID.  LT_MODEL_RANSAC and
 * volumetric plans: LT_ERR_UNSUPPORTED.  The algebraic tail is eager and reads these fields when it runs, so the call may come before or after the plan's
 * first forward and nothing is captured again.  Results are bit-identical to the Python host's (AlgebraicTriangulationNet.keypoint_stats). */
int lt_plan_set_alg_keypoint_stats(lt_plan* plan, float* stats2d_dev, int32_t* peak_index_dev, float* cov2d_img_dev, float* reproj_err_dev,
                                   float* cov3d_dev);
int lt_plan_info(const lt_plan* plan, lt_plan_info_t* info);
void lt_plan_destroy(lt_plan* plan);

#ifdef __cplusplus
}
#endif
#endif /* LT_HIP_H */
