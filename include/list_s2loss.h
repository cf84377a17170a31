/*
 * list_s2loss.h -- C ABI of stage 2's training loss on the MI355X (gfx950): the weighted binary cross-entropy of the
 * occupancy head (the reference's executors.py:138-141) and the three values of its SDFLoss (network/losses.py:6-38),
 * with the gradients of the two values that are trained on.  Exported from the same liblist_hip.so as include/list_hip.h.
 *
 * Conventions: those of list_loss.h (raw device pointers, caller-owned buffers, work enqueued on the caller's stream, no
 * allocation and no synchronisation inside, LIST_OK or a negative ListStatus); the description of a failure is read with
 * list_s2loss_last_error() (thread-local).
 *
 * occ is float32 [n_occ] (the sigmoid output, any shape flattened), occ_gt its target, [n_occ] float32
 * (occ_gt_kind = 0) or uint8 (occ_gt_kind = 1; a bool tensor is one), sdf_pred and sdf_gt float32 [B][N], all
 * C-contiguous on one device.  No pointer needs more than its element's alignment.  1 <= n_occ <= 2^36 and
 * 1 <= B, N with B*N <= 2^36, anything else is LIST_ERR_SHAPE and so is an occ_gt_kind other than 0 or 1; a NULL occ,
 * occ_gt, sdf_pred, sdf_gt, out, grad_out or workspace is LIST_ERR_ARG; a workspace smaller than
 * list_s2loss_workspace_bytes(n_occ, B, N) LIST_ERR_WORKSPACE.  Every refusal comes before any HIP call.  Nothing in the
 * workspace is kept from one call to the next (list_s2loss_bwd needs none).
 *
 * ---- forward: list_s2loss_fwd -----------------------------------------------------------------------------------------
 * Per element, o = occ[i] and t = (double)occ_gt[i].  The arguments of the logarithms are formed in float32 exactly as
 * torch forms them in `log(occ + 1e-8)` and `log(1 - occ + 1e-8)`:
 *   a = o + 1e-8f,   b = (1.0f - o) + 1e-8f
 * so a saturated sigmoid (o == 0 or o == 1) gives log(1e-8f) as it does there.  Everything after that is float64 (the
 * logarithm is csrc/s2loss_math.h's: float64 arithmetic, within 4 ulps of float64 on these float32-valued arguments, the
 * non-finite cases as in libm -- far inside what the final rounding to float32 leaves visible):
 *   S1 = sum of t * log((double)a),   S0 = sum of (1 - t) * log((double)b),   n = n_occ
 *   out[0] = occ_loss = (float)(1000 * (-w * S1 / n - (1 - w) * S0 / n))             with w widened to float64
 * Both terms are evaluated for every element (no shortcut for t == 0 or t == 1): a NaN, or an o < -1e-8 (or > 1 + 1e-8),
 * gives a NaN loss as it does in torch.
 * SDF terms, in float64 from the widened float32 p = sdf_pred[i], t = sdf_gt[i], with s = (double)sdf_scale:
 *   out[1] = sdf_loss  = (float)(sum of (t*s - p)^2 / B)
 *   out[2] = realvalue = (float)(1e4 * sum of (t - p/s)^2 / (B*N))
 *   out[3] = accuracy  = (float)(count of ((t > 0.5f) == (p > 0.5f)) / (B*N)), the count an integer
 * Order of every sum, fixed and independent of the device:  G = 1024 workgroups for the occupancy sums, 64 for the SDF
 * sums, of 256 lanes.  The elements are cut into a head of h elements, items of 4 consecutive elements, and a tail of
 * fewer than 4; h in [0, 3] is what brings occ (sdf_pred) to a 16-byte boundary, and the items are read with 16-byte
 * loads (4 target bytes at once) when the target pointer then sits on a 16-byte (uint8: 4-byte) boundary as well.
 * Otherwise h = 0 and an item is one element.  Lane j of workgroup g (thread T = 256*g + j of 256*G) adds its items
 * T, T + 256*G, T + 2*256*G, ... in turn, the elements of an item in index order; thread 0 adds the head before and the
 * tail after its items.  The 256 sums of a workgroup are folded as p[j] += p[j + k] for k = 128, 64, ..., 1, p[0] is the
 * workgroup's partial, and a second launch adds the partials in index order.  There are no float atomics and no
 * last-block counter: two calls on the same buffers give the same bits.
 *
 * ---- backward: list_s2loss_bwd ----------------------------------------------------------------------------------------
 * g0 = grad_out[0], g1 = grad_out[1] (float32 [4] read on the device: autograd's grad_output needs no host
 * synchronisation; [2] and [3] are not read -- realvalue and accuracy are reported, not trained on).  In float64, with a,
 * b, t, s, p as above:
 *   grad_occ[i]      = (float)((g0 * (1000 / n)) * ((-w * t) / a + ((1 - w) * (1 - t)) / b))
 *   grad_sdf_pred[i] = (float)((g1 * (-2 / B)) * (t*s - p))
 * written with plain vector stores (16 bytes per lane where grad_occ / grad_sdf_pred shares occ's / sdf_pred's position
 * in a 16-byte line).  A NULL grad_occ or grad_sdf_pred skips that side; both NULL is LIST_ERR_ARG.
 *
 * ---- diagnostic: list_s2loss_log ----------------------------------------------------------------------------------------
 * out[i] = the forward's logarithm of (double)x[i] as the device computes it, float64 [n] from float32 [n], 1 <= n <= 2^36
 * (LIST_ERR_SHAPE), x and out not NULL (LIST_ERR_ARG).  It is there for the tests, which hold the device's compilation of
 * csrc/s2loss_math.h to the 4 ulps that the host's is held to.
 */
#ifndef LIST_S2LOSS_H
#define LIST_S2LOSS_H

#include <stddef.h>
#include <stdint.h>

#include "list_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

size_t list_s2loss_workspace_bytes(int64_t n_occ, int64_t B, int64_t N);

int list_s2loss_fwd(const float* occ, const void* occ_gt, int occ_gt_kind, int64_t n_occ, const float* sdf_pred,
                    const float* sdf_gt, int64_t B, int64_t N, float sdf_scale, float w, float* out, void* workspace,
                    size_t workspace_bytes, void* stream);

int list_s2loss_bwd(const float* occ, const void* occ_gt, int occ_gt_kind, int64_t n_occ, const float* sdf_pred,
                    const float* sdf_gt, int64_t B, int64_t N, float sdf_scale, float w, const float* grad_out,
                    float* grad_occ, float* grad_sdf_pred, void* stream);

int list_s2loss_log(const float* x, int64_t n, double* out, void* stream);

const char* list_s2loss_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* LIST_S2LOSS_H */
