/*
 * list_imgenc.h -- C ABI of the image encoder (ResEncoder: ResNet-18 with a stride-1 7x7 stem, inference forward) on
 * the MI355X (gfx950): from the image [B,3,H,W] to the global 128-vector and the five feature maps the query path
 * samples.  Exported from the same liblist_hip.so as include/list_hip.h.
 *
 * Conventions: those of list_voxenc.h (raw device pointers, caller-owned buffers, work enqueued on the caller's stream,
 * no allocation and no synchronisation inside, LIST_OK or a negative ListStatus); the description of a failure is read
 * with list_imgenc_last_error() (thread-local).  Shapes and arguments are checked on the host before any HIP call.
 *
 * Network (fixed).  conv 7x7, pad 3, stride 1, 3 -> 64, BN, ReLU                      -> level 0: 64 x H x W
 *   max-pool 3x3, stride 2, pad 1; layer1 = two BasicBlocks of width 64              -> level 1: 64 x H/2 x W/2
 *   layer2 .. layer4 = two BasicBlocks each of width 128, 256, 512; the first opens with a stride-2 3x3 convolution
 *   and has a 1x1 stride-2 downsample (with its own BN) on the identity              -> levels 2 .. 4 at H/4, H/8, H/16
 *   mean over level 4, fc 512 -> 1000, fc1 1000 -> 128                                -> vec [B][128]
 * A BasicBlock is y = relu(bn1(conv1(x))); out = relu(bn2(conv2(y)) + identity).  No convolution has a bias.  BN is the
 * eval-mode affine y * s + t, s = weight / sqrt(var + eps), t = bias - mean * s, applied right after the convolution.
 *
 * Arithmetic (one mode).  The stem is fp32 (fp32 image, fp32 weights, fmaf).  Every other convolution is an implicit
 * GEMM on the matrix cores: fp16 operands (weights rounded to fp16 once, by list_imgenc_prep_weights; BN is NOT folded
 * into them), fp32 accumulation, fp32 epilogue in the order acc * s + t, plus the identity where there is one, ReLU.
 * Activations between layers are fp16 channels-last in the workspace, rounded to nearest even from the fp32 epilogue
 * value and NOT saturated (a value beyond 65504 becomes an infinity, a non-finite activation propagates).  A level is
 * the fp32 epilogue value of the layer that produces it; the fp16 copy beside it feeds the next layer.  The max-pool
 * reads the fp16 copy of level 0; a NaN wins.  Head: the mean of the fp32 level 4 in pixel order, then fc1 o fc as ONE
 * [128][512] matrix and one bias (composed in float64 by list_imgenc_prep_weights, rounded once), fp32 fmaf in channel
 * order.  No atomics: two calls give identical bits.
 *
 * Layouts.  img: float32 [B][3][H][W] with the four ELEMENT strides given (an NCHW and a channels-last image are both
 * read where they lie).  levels_out[k]: float32 channels-last [B][H >> k][W >> k][C_k], C = 64, 64, 128, 256, 512.
 * vec: float32 [B][128].  H and W: multiples of 16 in [LIST_IMGENC_MIN_HW, LIST_IMGENC_MAX_HW], independent.
 * packed, workspace and the levels are 16-byte aligned, img and vec 4-byte aligned.
 *
 * Call sequence:
 *   bytes = list_imgenc_weight_bytes();
 *   list_imgenc_prep_weights(&params, packed, bytes, stream);          once per set of weights
 *   ws = list_imgenc_workspace_bytes(B, H, W);                         (0: refused, see list_imgenc_last_error)
 *   list_imgenc_forward(&io, stream);
 * The forward is list_imgenc_n_steps() kernel launches; list_imgenc_forward_steps runs a sub-range of them (for
 * per-layer tests and timing: the steps before `step_begin` must have run on the same workspace and outputs).
 */
#ifndef LIST_IMGENC_H
#define LIST_IMGENC_H

#include <stddef.h>
#include <stdint.h>

#include "list_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LIST_IMGENC_N_LEVELS 5
#define LIST_IMGENC_N_CONVS 20      /* the stem, 4 of layer1, 5 each of layer2 .. layer4 (conv1, down, conv2, conv1, conv2) */
#define LIST_IMGENC_MIN_HW 32
#define LIST_IMGENC_MAX_HW 512
#define LIST_IMGENC_VEC 128
#define LIST_IMGENC_FC 1000

/* fp32 parameters of one convolution and the BN behind it, C-contiguous device arrays.  w: [C_out][C_in][k][k]; the
 * four BN arrays have C_out entries. */
typedef struct ListImgencConv {
  const float* w;
  const float* bn_weight;
  const float* bn_bias;
  const float* bn_mean;
  const float* bn_var;
  float bn_eps;
} ListImgencConv;

/* conv[0]: the stem; then in launch order: layer1 (0.conv1, 0.conv2, 1.conv1, 1.conv2), and for layer2 .. layer4
 * (0.conv1, 0.downsample, 0.conv2, 1.conv1, 1.conv2).  fc_w [1000][512], fc_b [1000], fc1_w [128][1000], fc1_b [128]. */
typedef struct ListImgencParams {
  ListImgencConv conv[LIST_IMGENC_N_CONVS];
  const float* fc_w;
  const float* fc_b;
  const float* fc1_w;
  const float* fc1_b;
} ListImgencParams;

typedef struct ListImgencIO {
  const float* img;                 /* [B][3][H][W] by strides */
  int64_t img_sb, img_sc, img_sh, img_sw;   /* element strides */
  int32_t B, H, W;
  const void* packed;
  size_t packed_bytes;
  void* workspace;
  size_t workspace_bytes;
  float* vec;                       /* [B][128] */
  float* levels_out[LIST_IMGENC_N_LEVELS];
} ListImgencIO;

size_t list_imgenc_weight_bytes(void);
int list_imgenc_prep_weights(const ListImgencParams* params, void* packed, size_t packed_bytes, void* stream);
size_t list_imgenc_workspace_bytes(int32_t B, int32_t H, int32_t W);
int list_imgenc_forward(const ListImgencIO* io, void* stream);
int32_t list_imgenc_n_steps(void);
int list_imgenc_forward_steps(const ListImgencIO* io, int32_t step_begin, int32_t step_end, void* stream);
const char* list_imgenc_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* LIST_IMGENC_H */
