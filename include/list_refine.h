/*
 * list_refine.h -- C ABI of the coarse-to-fine SDF grid on the MI355X (gfx950): from the SDF on a coarse lattice of
 * an R^3 grid, the fine points whose exact value the iso-surface needs, and the dense volume filled from the lattice,
 * the exact values of those points and trilinear interpolation everywhere else.  Exported from the same
 * liblist_hip.so as include/list_hip.h.
 *
 * Conventions: those of list_hip.h (raw device pointers, caller-owned buffers, work enqueued on the caller's stream,
 * no allocation and no synchronisation inside, LIST_OK or a negative ListStatus), except that the description of a
 * failure is read with list_refine_last_error() (thread-local, like list_last_error()).  Shapes and arguments are
 * checked on the host before any HIP call.
 *
 * Grid.  Fine points (i, j, k), 0 <= i, j, k < R, 2 <= R <= 1290 (R^3 <= INT32_MAX), flat index (i * R + j) * R + k,
 * at lo + idx * (hi - lo) / (R - 1) per axis, computed in double, the last index pinned to hi, rounded to float.
 * Stride s in {2, 4, 8}.  Lattice indices per axis c_m = min(m * s, R - 1), m = 0 .. K - 1,
 * K = ceil((R - 1) / s) + 1; brick b (0 <= b < NB = K - 1) spans the fine indices [c_b, c_{b+1}] on its axis (the
 * last brick may be thinner).  lattice is a C-contiguous float32 [K][K][K] array: the field at the lattice points.
 *
 * Classification.  A brick is active iff one of its 8 corner values is not finite, its corners are not all on the
 * same side of level (inside iff v > level), or some corner has |v - level| < band (float32 arithmetic).  The active
 * set is then dilated by one brick (26-neighbourhood).  A fine point that is not a lattice point is REFINED iff at
 * least one brick that contains it (2 to 8 for a point on a brick face or edge) is in the dilated set.
 *
 * Fill.  volume is a C-contiguous float32 [R][R][R] array: lattice points take their lattice value, refined points
 * their value from values[] (the field at the points list_refine_emit listed), every other point the trilinear
 * interpolation of the 8 corners of brick (min(i / s, NB - 1), ...) with t = (i - c_b) / (c_{b+1} - c_b) per axis,
 * lerp(a, b, t) = a + t * (b - a), along axis 2, then 1, then 0.  Output is deterministic, bit for bit.
 *
 * Call sequence:
 *   bytes = list_refine_workspace_bytes(R, s);                           (0: refused, see list_refine_last_error)
 *   list_refine_count(lattice, R, s, level, band, ws, bytes, total, stream);   total: DEVICE int64[1], the number
 *                                                                              of refined points
 *   copy total to the host (the one synchronisation), allocate coords float32 [n][3] and indices int32 [n];
 *   list_refine_emit(R, s, lo, hi, ws, bytes, coords, indices, n, stream);     refined points in raster order
 *   evaluate the field at coords into values float32 [n];
 *   list_refine_fill(lattice, values, n, R, s, ws, bytes, volume, stream);
 * emit and fill read what list_refine_count left in the workspace: same R, s and workspace in between.  The
 * workspace starts with the brick masks, uint8 [NB][NB][NB] each: active at byte 0, dilated at byte
 * list_refine_mask_offset(R, s).
 */
#ifndef LIST_REFINE_H
#define LIST_REFINE_H

#include <stddef.h>
#include <stdint.h>

#include "list_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LIST_REFINE_MAX_R 1290

size_t list_refine_workspace_bytes(int32_t R, int32_t s);
size_t list_refine_mask_offset(int32_t R, int32_t s);
int list_refine_count(const float* lattice, int32_t R, int32_t s, float level, float band, void* workspace,
                      size_t workspace_bytes, int64_t* total, void* stream);
int list_refine_emit(int32_t R, int32_t s, double lo, double hi, const void* workspace, size_t workspace_bytes,
                     float* coords, int32_t* indices, int64_t n, void* stream);
int list_refine_fill(const float* lattice, const float* values, int64_t n, int32_t R, int32_t s,
                     const void* workspace, size_t workspace_bytes, float* volume, void* stream);
const char* list_refine_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* LIST_REFINE_H */
