/*
 * list_augment.h -- C ABI of the training-image augmentation on the MI355X (gfx950): the reference's
 * T.RandomHorizontalFlip(0.5) and T.ColorJitter(brightness=0.3, saturation=0.5, hue=0.5) followed by T.ToTensor()
 * (datasets/Datasets.py:24-38,161-174), applied to a batch of raw uint8 images behind the host-to-device copy in one
 * launch.  Exported from the same liblist_hip.so as include/list_hip.h.
 *
 * Conventions: those of list_loss.h (raw device pointers, caller-owned buffers, work enqueued on the caller's stream, no
 * allocation and no synchronisation inside, LIST_OK or a negative ListStatus); the description of a failure is read with
 * list_augment_last_error() (thread-local).
 *
 * ---- the steps, exactly ---------------------------------------------------------------------------------------------------
 * On PIL images ColorJitter is three Pillow operations in a random order, each from uint8 RGB to uint8 RGB.  They are
 * restated here so that every output byte equals Pillow 12's (csrc/augment_math.h is the text; the tests hold it to Pillow
 * over all 2^24 colours).  No product is fused into a sum (-ffp-contract=off).
 *   flip        output column x reads source column W - 1 - x.
 *   brightness  ImageEnhance.Brightness, a blend with black.  In float32: t = f * x; 0 if t <= 0, 255 if t >= 255, else t
 *               truncated.
 *   saturation  ImageEnhance.Color, a blend with convert("L").  L = (19595 R + 38470 G + 7471 B + 0x8000) >> 16; per
 *               channel in float32 t = L + f * (x - L), clipped and truncated as above.
 *   hue         convert("HSV"), H <- (H + shift) mod 256, convert("RGB").
 *               RGB -> HSV: V = maxc; H = S = 0 when maxc == minc; else in float32 cr = maxc - minc, s = cr / maxc,
 *               rc = (maxc - r) / cr and gc, bc likewise; h = bc - gc if r is the maximum, else 2.0 + rc - bc if g is, else
 *               4.0 + gc - rc, evaluated in float64 from the float32 operands and rounded to float32;
 *               h' = fmod((double)h / 6.0 + 1.0, 1.0) rounded to float32; H = clip8((int)((double)h' * 255.0)),
 *               S = clip8((int)((double)s * 255.0)).
 *               HSV -> RGB in float64: R = G = B = V when S == 0; else fh = H * 6.0 / 255.0, fs = S / 255.0, i = floor(fh),
 *               f = fh - i, p = rint(V (1 - fs)), q = rint(V (1 - fs f)), t = rint(V (1 - fs (1 - f))) (to nearest even,
 *               clipped to 0 ... 255), and by i mod 6 the result is (V,t,p), (q,V,p), (p,V,t), (p,q,V), (t,p,V), (V,p,q).
 *               A hue step of shift 0 still makes the round trip, which is lossy, as Pillow's does.
 *               The shift is THIS project's definition: shift = trunc(hue * 255) mod 256 for the drawn hue in [-0.5, 0.5]
 *               (torchvision adds np.uint8(hue * 255) with uint8 wrap-around, whose value for a negative hue is the
 *               conversion's; nothing here is compared with it).  The ABI takes the shift itself, any of 0 ... 255.
 *   ToTensor    float32(level) / float32(255), correctly rounded.
 *
 * ---- per-image parameters: ListAugmentParams ------------------------------------------------------------------------------
 *   ops         which steps run at all: LIST_AUGMENT_FLIP | LIST_AUGMENT_BRIGHTNESS | LIST_AUGMENT_SATURATION |
 *               LIST_AUGMENT_HUE.  0 is plain ToTensor.
 *   order       a permutation of 0 (brightness), 1 (contrast: a no-op, the reference passes none), 2 (saturation), 3 (hue):
 *               the colour steps in the order they run.  The flip comes first (flipping and per-pixel steps commute).
 *   brightness  in [0.7, 1.3], saturation in [0.5, 1.5], hue_shift in [0, 255]; read only when their bit of ops is set.
 *
 * ---- list_augment_fwd -----------------------------------------------------------------------------------------------------
 * src is uint8 [B][H][W][3], C-contiguous, on the device; dst float32 of logical shape [B][3][H][W], written as NCHW
 * (channels_last = 0: dst[((b*3 + c)*H + y)*W + x]) or channels-last (channels_last = 1: dst[((b*H + y)*W + x)*3 + c]),
 * every element of it.  The parameters are passed twice: params_host [B] is read by this call on the host, where it is
 * checked; params_device [B] holds the same records on the device, where the kernel reads them (the caller's copy, on the
 * same stream, ahead of the call).  One launch: a thread owns four consecutive output columns of one row, no workgroup
 * spans two images, so every branch on a parameter is uniform over a workgroup.  When src is 4-byte aligned, dst 16-byte
 * aligned and W a multiple of 4, a thread reads its 12 source bytes as three dwords and stores 16-byte runs; otherwise it
 * reads bytes and stores floats, with the same statements in between.  No LDS, no workspace.
 * Refusals, all before any HIP call: a NULL src, dst, params_host or params_device is LIST_ERR_ARG; B, H or W < 1,
 * B > 65535, H or W > 65536, a channels_last other than 0 or 1 LIST_ERR_SHAPE; ops with a bit beyond the four, an order
 * that is no permutation of 0 ... 3, or a factor outside its range while its step is enabled LIST_ERR_ARG.
 *
 * ---- list_augment_pixel ---------------------------------------------------------------------------------------------------
 * Host only: one pixel rgb_in [3] through the colour steps of *p (the flip bit is ignored) -> rgb_out [3] levels and
 * out [3] = the ToTensor values; either output may be NULL.  The same checks on *p.  It runs csrc/augment_math.h as the
 * host compiles it and is there for tests and tools.
 */
#ifndef LIST_AUGMENT_H
#define LIST_AUGMENT_H

#include <stddef.h>
#include <stdint.h>

#include "list_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

enum {
  LIST_AUGMENT_FLIP = 1,
  LIST_AUGMENT_BRIGHTNESS = 2,
  LIST_AUGMENT_SATURATION = 4,
  LIST_AUGMENT_HUE = 8
};

typedef struct ListAugmentParams {
  int32_t ops;
  int32_t order[4];
  float brightness;
  float saturation;
  int32_t hue_shift;
} ListAugmentParams;                             /* 32 bytes */

int list_augment_fwd(const uint8_t* src, float* dst, int64_t B, int64_t H, int64_t W, int channels_last,
                     const ListAugmentParams* params_host, const ListAugmentParams* params_device, void* stream);

int list_augment_pixel(const uint8_t* rgb_in, const ListAugmentParams* p, uint8_t* rgb_out, float* out);

const char* list_augment_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* LIST_AUGMENT_H */
