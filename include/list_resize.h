/*
 * list_resize.h -- C ABI of the ragged-batch image resize on the MI355X (gfx950): the reference's Pix3D transform
 * (datasets/Datasets.py:330-344: T.RandomHorizontalFlip, T.ColorJitter, T.Resize((224, 224)), T.ToTensor on PIL images) for
 * a batch of raw uint8 images of DIFFERENT sizes, packed into one buffer, behind the host-to-device copy.  Exported from
 * the same liblist_hip.so as include/list_hip.h.
 *
 * Conventions: those of list_augment.h (raw device pointers, caller-owned buffers, work enqueued on the caller's stream, no
 * allocation and no synchronisation inside, LIST_OK or a negative ListStatus; the *_bytes queries return 0 for a refusal);
 * the description of a failure is read with list_resize_last_error() (thread-local).
 *
 * ---- the resize, exactly --------------------------------------------------------------------------------------------------
 * On a PIL image T.Resize is Image.resize(size, BILINEAR): Pillow 12's antialiased, separable resample of an 8-bit RGB
 * image H x W to out_h x out_w with the box being the whole image.  It is restated here so that every output byte equals
 * Pillow's (csrc/resize_math.h is the text; the tests hold it to Pillow 12.2.0, where no rule below was found to disagree).
 *
 * Coefficients.  Per axis `in` -> `out`, in float64, every operation rounded on its own (-ffp-contract=off):
 *   scale = in / out;  fs = max(scale, 1.0);  support = 1.0 * fs;  ksize = (int)ceil(support) * 2 + 1;  ss = 1.0 / fs.
 *   For output index xx:  center = (xx + 0.5) * scale;
 *     xmin = max((int)(center - support + 0.5), 0);   xmax = min((int)(center + support + 0.5), in) - xmin;
 *     w[x] = tri((x + xmin - center + 0.5) * ss) for x < xmax, tri(t) = 1 - |t| if |t| < 1 else 0;
 *     ww = the sum of w in ascending x;  k[x] = w[x] / ww when ww != 0;
 *     K[x] = (int)(0.5 + k[x] * 2^22), or (int)(-0.5 + k[x] * 2^22) for k[x] < 0 (bilinear has none; the rule is kept).
 * A pass along an axis.  Per channel acc = 2^21 + sum over x < xmax of pixel[xmin + x] * K[xx][x] in int32, then
 *   clip(acc >> 22, 0, 255).  The weights are non-negative and sum to about 2^22, so acc < 2^31: list_resize_plan checks
 *   255 * sum(K) + 2^21 < 2^31 for every output where it makes the tables.
 * Order.  (H, W) == (out_h, out_w): copy.  Else, if H > 100 * W and out_h < H (Pillow 12's tall-image rule in
 *   Image.resize): the vertical pass to out_h x W, then the horizontal pass.  Else the horizontal pass to H x out_w, then
 *   the vertical pass.  A pass whose axis already has the target size is skipped.  The intermediate is uint8, clipped as
 *   above.
 * Around it.  The flip (source column W - 1 - x) and the colour steps of list_augment.h act on the SOURCE pixels, before
 *   the resize; ToTensor (float32(level) / float32(255)) acts on the result: the reference's transform order.  Neither the
 *   flip nor the jitter commutes with the resize bit for bit, so the order is part of the definition.
 *
 * ---- the plan ---------------------------------------------------------------------------------------------------------------
 * list_resize_plan fills a caller-owned HOST buffer of list_resize_plan_bytes(...) bytes; the caller copies it to the device
 * (on the stream, ahead of list_resize_fwd) and passes both, as list_augment_fwd's parameters are passed twice.  Layout:
 *   ListResizePlanHeader | ListResizePlanImage [B] | int32 tables
 * Every image is run as TWO stages, each RESIZE_COPY (0), horizontal (1) or vertical (2): stage 0 from the source (flip and
 * colour steps applied to every pixel it reads) to a uint8 intermediate mid_h x mid_w x 3 in the workspace, stage 1 from
 * there to the float output.  Two passes are the two stages in their order; a single pass is stage 0 and stage 1 copies; equal
 * sizes copy twice.  A stage that is a pass has a bounds table [n_out][2] = (xmin, xmax) and a weights table [n_out][ksize]
 * (zero beyond xmax) at the byte offsets of the plan its record gives; a copy has ksize 0 and offsets 0.
 *
 * ---- the calls --------------------------------------------------------------------------------------------------------------
 * images [B] describes the packed source: image i is uint8 [H][W][3], C-contiguous, `offset` bytes into src; any alignment.
 * Sides and the target sizes are 1 ... 16384, B is 1 ... 65535.
 * list_resize_plan_bytes / list_resize_workspace_bytes   host arithmetic: the plan's size, and the size of the workspace that
 *   holds the intermediates (the colour steps run inside stage 0's loads, so there is no jittered copy of the source).
 * list_resize_plan    checks images against src_bytes (offset >= 0, offset + 3 H W <= src_bytes) and fills plan.
 * list_resize_fwd     src uint8 on the device, src_bytes long, never written; dst float32 of logical shape
 *   [B][3][out_h][out_w], written as NCHW (channels_last = 0) or channels-last (1), every element of it.  params_host /
 *   params_device are B ListAugmentParams records (checked as list_augment_fwd checks them), or both NULL for a plain
 *   resize.  Two launches, one per stage: a thread owns one output pixel of its stage, blockIdx.y is the image, so the
 *   image's record, its parameters and every branch on them are uniform over a workgroup.  Integer accumulation, no
 *   atomics, no LDS.  plan_host is re-checked (header, geometry of every record against images' rules, every bounds entry
 *   inside its axis) before anything is launched.
 * list_resize_host    host only: one image uint8 [H][W][3] -> uint8 [out_h][out_w][3], csrc/resize_math.h as the host
 *   compiles it, for tests and tools.
 * Refusals, all before any HIP call: a NULL pointer (params_host and params_device NULL together is the plain resize; one
 * of them alone is refused) is LIST_ERR_ARG; B < 1 or > 65535, a side or target size < 1 or > 16384, a channels_last other
 * than 0 or 1 LIST_ERR_SHAPE; an offset or extent outside src_bytes LIST_ERR_ARG; a plan buffer or a workspace that is too
 * small LIST_ERR_WORKSPACE; a plan_host that is not list_resize_plan's for this B and target size LIST_ERR_ARG; the
 * parameter refusals of list_augment_fwd.
 */
#ifndef LIST_RESIZE_H
#define LIST_RESIZE_H

#include <stddef.h>
#include <stdint.h>

#include "list_augment.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LIST_RESIZE_MAX_SIDE 16384
#define LIST_RESIZE_MAX_BATCH 65535
#define LIST_RESIZE_PLAN_MAGIC 0x5a52534c      /* "LSRZ" */

typedef struct ListResizeImage {
  int64_t offset;                                /* of the image's [H][W][3] bytes in the packed source */
  int32_t H, W;
} ListResizeImage;                               /* 16 bytes */

typedef struct ListResizePlanHeader {
  int64_t plan_bytes;                            /* what list_resize_plan_bytes returned */
  int64_t workspace_bytes;                       /* what list_resize_workspace_bytes returns */
  int64_t src_bytes;                             /* the packed source the offsets were checked against */
  int32_t magic, B, out_h, out_w;
} ListResizePlanHeader;                          /* 40 bytes */

typedef struct ListResizePlanImage {
  int64_t src_offset;                            /* ListResizeImage.offset */
  int64_t mid_offset;                            /* of the uint8 intermediate [mid_h][mid_w][3] in the workspace */
  int32_t H, W;
  int32_t mid_h, mid_w;
  int32_t stage[2];                              /* 0 copy, 1 horizontal pass, 2 vertical pass */
  int32_t ksize[2];                              /* taps per output; 0 for a copy */
  int64_t bounds[2];                             /* byte offset in the plan of int32 [n_out][2]; 0 for a copy */
  int64_t weights[2];                            /* byte offset in the plan of int32 [n_out][ksize]; 0 for a copy */
} ListResizePlanImage;                           /* 80 bytes */

size_t list_resize_plan_bytes(const ListResizeImage* images, int64_t B, int64_t out_h, int64_t out_w);

size_t list_resize_workspace_bytes(const ListResizeImage* images, int64_t B, int64_t out_h, int64_t out_w);

int list_resize_plan(const ListResizeImage* images, int64_t B, int64_t src_bytes, int64_t out_h, int64_t out_w, void* plan,
                     size_t plan_bytes);

int list_resize_fwd(const uint8_t* src, int64_t src_bytes, const void* plan_host, const void* plan_device, size_t plan_bytes,
                    const ListAugmentParams* params_host, const ListAugmentParams* params_device, float* dst,
                    int channels_last, void* workspace, size_t workspace_bytes, void* stream);

int list_resize_host(const uint8_t* src, int64_t H, int64_t W, uint8_t* dst, int64_t out_h, int64_t out_w);

const char* list_resize_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* LIST_RESIZE_H */
