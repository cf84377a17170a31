// The checks of one ListAugmentParams record (include/list_augment.h), shared by the units that take such records:
// augment_kernels.hip and resize_kernels.hip.  Include below list_host.h and list_augment.h: the refusal is written into the
// including unit's own error text.
#pragma once

#include "augment_math.h"

// LIST_OK, or the refusal of record i with its message
static int check_params(const ListAugmentParams& p, long long i) {
  if (p.ops & ~(AUGMENT_FLIP | AUGMENT_BRIGHTNESS | AUGMENT_SATURATION | AUGMENT_HUE))
    return fail(LIST_ERR_ARG, "params[%lld].ops = %d: bits beyond flip | brightness | saturation | hue (15)", i, p.ops);
  int seen = 0;
  for (int k = 0; k < 4; ++k)
    if (p.order[k] >= 0 && p.order[k] < 4) seen |= 1 << p.order[k];
  if (seen != 15)
    return fail(LIST_ERR_ARG, "params[%lld].order = (%d, %d, %d, %d): not a permutation of 0 ... 3", i, p.order[0],
                p.order[1], p.order[2], p.order[3]);
  if ((p.ops & AUGMENT_BRIGHTNESS) && !(p.brightness >= 0.7f && p.brightness <= 1.3f))
    return fail(LIST_ERR_ARG, "params[%lld].brightness = %g: outside [0.7, 1.3]", i, (double)p.brightness);
  if ((p.ops & AUGMENT_SATURATION) && !(p.saturation >= 0.5f && p.saturation <= 1.5f))
    return fail(LIST_ERR_ARG, "params[%lld].saturation = %g: outside [0.5, 1.5]", i, (double)p.saturation);
  if ((p.ops & AUGMENT_HUE) && (p.hue_shift < 0 || p.hue_shift > 255))
    return fail(LIST_ERR_ARG, "params[%lld].hue_shift = %d: outside [0, 255]", i, p.hue_shift);
  return LIST_OK;
}
