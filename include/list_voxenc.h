/*
 * list_voxenc.h -- C ABI of the 3-D occupancy encoder (VoxelEncoder2, inference forward) on the MI355X (gfx950):
 * from the occupancy grid [B][R][R][R] to the six feature volumes the query path gathers from.  Exported from the
 * same liblist_hip.so as include/list_hip.h.
 *
 * Conventions: those of list_hip.h (raw device pointers, caller-owned buffers, work enqueued on the caller's stream,
 * no allocation and no synchronisation inside, LIST_OK or a negative ListStatus), except that the description of a
 * failure is read with list_voxenc_last_error() (thread-local, like list_last_error()).  Shapes and arguments are
 * checked on the host before any HIP call.
 *
 * Network.  layers = [1, 1, 1, 1, C4, C5, C6, C7, C8] (n_layers = 9; C4 .. C8 each 16, 32, 64 or 128), stage l maps
 * layers[l] to layers[l + 1] channels; every convolution is 3x3x3, padding 1 (zeros), with a bias:
 *   stage 0, 1   conv, ReLU, BN                                   (1 channel, R^3)
 *   stage 2      conv, sigmoid                                    -> level 0: 1 x R^3
 *   stage l >= 3 conv, ReLU, conv2, ReLU, BN                      -> level l - 2: layers[l + 1] x (R >> (l - 3))^3,
 *                then 2x2x2 max-pooling into the next stage (not after stage 7)
 * BN is the eval-mode affine y * s + t, s = weight / sqrt(var + eps), t = bias - mean * s, applied AFTER the ReLU.
 *
 * Arithmetic (one mode).  The convolutions with one input channel (stages 0 .. 2 and the first of stage 3) run in
 * fp32 with fp32 weights; level 0 is fp32.  Every other convolution is an implicit GEMM on the matrix cores: fp16
 * operands (weights rounded to fp16 once, by list_voxenc_prep_weights), fp32 accumulation, fp32 epilogue.  The
 * activations between those layers and levels 1 .. 5 are fp16, rounded to nearest even from the fp32 epilogue value.
 * The fp16 outputs are NOT saturated: a value beyond 65504 becomes an infinity and a non-finite activation propagates,
 * as it does under autocast.  No atomics: the output is deterministic, bit for bit.
 *
 * Layouts.  occ: float32 [B][R][R][R], C-contiguous.  levels_out[0]: float32 [B][R][R][R] (one channel).
 * levels_out[k], k = 1 .. 5: fp16 channels-last [B][D][D][D][C], D = R >> (k - 1), C = layers[k + 3].
 * R is a multiple of 16, 16 <= R <= LIST_VOXENC_MAX_R.
 *
 * Call sequence:
 *   bytes = list_voxenc_weight_bytes(layers, 9);                         (0: refused, see list_voxenc_last_error)
 *   list_voxenc_prep_weights(stages, layers, 9, packed, bytes, stream);  once per set of weights
 *   ws = list_voxenc_workspace_bytes(B, R, layers, 9);
 *   list_voxenc_forward(occ, B, R, layers, 9, packed, bytes, workspace, ws, levels_out, stream);
 * The forward is list_voxenc_n_steps() kernel launches; list_voxenc_forward_steps runs a sub-range of them (for
 * per-layer timing: the steps before `step_begin` must have run on the same workspace and outputs).
 */
#ifndef LIST_VOXENC_H
#define LIST_VOXENC_H

#include <stddef.h>
#include <stdint.h>

#include "list_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LIST_VOXENC_N_LAYERS 9
#define LIST_VOXENC_N_LEVELS 6
#define LIST_VOXENC_MAX_R 256

/* fp32 parameters of stage l, C-contiguous device arrays.  conv_w: [layers[l + 1]][layers[l]][3][3][3];
 * conv2_w: [layers[l + 1]][layers[l + 1]][3][3][3], stages >= 3 only (NULL before); the four BN arrays have
 * layers[l + 1] entries and are not read for stage 2. */
typedef struct ListVoxencStage {
  const float* conv_w;
  const float* conv_b;
  const float* conv2_w;
  const float* conv2_b;
  const float* bn_weight;
  const float* bn_bias;
  const float* bn_mean;
  const float* bn_var;
  float bn_eps;
} ListVoxencStage;

size_t list_voxenc_weight_bytes(const int32_t* layers, int32_t n_layers);
int list_voxenc_prep_weights(const ListVoxencStage* stages, const int32_t* layers, int32_t n_layers, void* packed,
                             size_t packed_bytes, void* stream);
size_t list_voxenc_workspace_bytes(int32_t B, int32_t R, const int32_t* layers, int32_t n_layers);
int list_voxenc_forward(const float* occ, int32_t B, int32_t R, const int32_t* layers, int32_t n_layers,
                        const void* packed, size_t packed_bytes, void* workspace, size_t workspace_bytes,
                        void* const* levels_out, void* stream);
int32_t list_voxenc_n_steps(const int32_t* layers, int32_t n_layers);
int list_voxenc_forward_steps(const float* occ, int32_t B, int32_t R, const int32_t* layers, int32_t n_layers,
                              const void* packed, size_t packed_bytes, void* workspace, size_t workspace_bytes,
                              void* const* levels_out, int32_t step_begin, int32_t step_end, void* stream);
const char* list_voxenc_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* LIST_VOXENC_H */
