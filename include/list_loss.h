/*
 * list_loss.h -- C ABI of the training losses on the MI355X (gfx950) that are not part of the SDF query path: the
 * Chamfer distance of stage 1 (CoarseNet: a predicted coarse cloud against the farthest-point cloud of the ground truth,
 * what the reference takes from pytorch3d.loss.chamfer_distance with its default arguments) and its gradient.
 * Exported from the same liblist_hip.so as include/list_hip.h.
 *
 * Conventions: those of list_hip.h (raw device pointers, caller-owned buffers, work enqueued on the caller's stream,
 * no allocation and no synchronisation inside, LIST_OK or a negative ListStatus), except that the description of a
 * failure is read with list_loss_last_error() (thread-local, like list_last_error()).
 *
 * Clouds are x float32 [B][N][3] and y float32 [B][M][3], C-contiguous, on one device.  1 <= B, N, M <= INT32_MAX and
 * B*N, B*M <= INT32_MAX; anything else is LIST_ERR_SHAPE, a NULL required pointer LIST_ERR_ARG and a workspace smaller
 * than list_chamfer_workspace_bytes(B, N, M) LIST_ERR_WORKSPACE, all refused before any HIP call.  One workspace of
 * that size serves both calls; nothing in it is kept from one call to the next.
 *
 * ---- forward: list_chamfer_fwd -----------------------------------------------------------------------------------------
 * Squared distance of a pair, in float32 with d = p - q and no contraction into fma (the arithmetic of list_eval_nn
 * without its sqrt):   d2(p, q) = (dx*dx + dy*dy) + dz*dz.
 * For every x[b][i]:  d2_xy[b][i] = min_j d2(x[b][i], y[b][j]),  idx_xy[b][i] = the smallest j reaching that minimum.
 * For every y[b][j]:  d2_yx[b][j] = min_i d2(y[b][j], x[b][i]),  idx_yx[b][j] = the smallest i reaching it.
 * Non-finite input: a pair whose d2 is NaN never becomes the minimum; a point none of whose pairs is below +inf gets
 * d2 = +inf and idx = 0; a point with a NaN coordinate gets d2 = NaN (so the loss is NaN).  Every index lies in [0, M)
 * or [0, N) whatever the input, so list_chamfer_bwd never reads out of bounds with them.
 * Loss (pytorch3d's point_reduction = "mean", batch_reduction = "mean", norm = 2), in float64, in this order:
 *   s_xy[b] = sum over i of (double)d2_xy[b][i]: lane t of 256 adds i = t, t + 256, t + 512, ... in turn, then the 256
 *             partials are folded as p[t] += p[t + w] for w = 128, 64, ..., 1 (s_xy[b] = p[0]);  s_yx[b] likewise;
 *   L_xy    = ((s_xy[0] / N + s_xy[1] / N) + ...) + s_xy[B-1] / N,  L_yx likewise with M;
 *   *loss   = (float)(L_xy / B + L_yx / B).
 * There are no float atomics: the minima are combined across workgroups by a 64-bit atomicMin of
 * (float bits of d2 << 32 | index), which is exact for d2 >= 0 and independent of arrival order, so two calls on the
 * same input give the same bits in every output.
 *
 * ---- backward: list_chamfer_bwd ----------------------------------------------------------------------------------------
 * g = *grad_loss (float32, read on the device: autograd's grad_output needs no host synchronisation).  In float64,
 * with differences of the float32 coordinates widened to float64, kx = 2 / (B*N) and ky = 2 / (B*M):
 *   grad_x[b][i] = (float)((g*kx) * (x_i - y_{idx_xy[b][i]}) + (g*ky) * S_x[b][i]),
 *                  S_x[b][i] = sum over j with idx_yx[b][j] == i of (x_i - y_j), per axis;
 *   grad_y[b][j] = (float)((g*ky) * (y_j - x_{idx_yx[b][j]}) + (g*kx) * S_y[b][j]),
 *                  S_y[b][j] = sum over i with idx_xy[b][i] == j of (y_j - x_i).
 * The sources of each target are gathered by a stable counting sort per batch (integer histogram, exclusive scan,
 * placement in source-index order): S is summed in increasing source index when a target has at most 32 sources, and
 * as 64 strided partial sums (lane l adds the l-th, (l+64)-th, ... source in that order) folded by a fixed butterfly
 * when it has more.  Both orders are fixed, so two calls give the same bits.  An index outside [0, M) / [0, N)
 * contributes nothing.  A NULL grad_x or grad_y skips that side (both NULL is LIST_ERR_ARG).
 */
#ifndef LIST_LOSS_H
#define LIST_LOSS_H

#include <stddef.h>
#include <stdint.h>

#include "list_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

size_t list_chamfer_workspace_bytes(int64_t B, int64_t N, int64_t M);

int list_chamfer_fwd(const float* x, const float* y, int64_t B, int64_t N, int64_t M, float* d2_xy, int32_t* idx_xy,
                     float* d2_yx, int32_t* idx_yx, float* loss, void* workspace, size_t workspace_bytes,
                     void* stream);

int list_chamfer_bwd(const float* x, const float* y, int64_t B, int64_t N, int64_t M, const int32_t* idx_xy,
                     const int32_t* idx_yx, const float* grad_loss, float* grad_x, float* grad_y, void* workspace,
                     size_t workspace_bytes, void* stream);

const char* list_loss_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* LIST_LOSS_H */
