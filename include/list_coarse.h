/*
 * list_coarse.h -- C ABI of the coarse stage (inference forward) on the MI355X (gfx950): everything between the image
 * encoders and the occupancy encoder.  From the image code feat_g [B][F0] to the coarse cloud pc [B][P][3]
 * (TreeGraphDecoder), its 512-wide code (PointMLP and the max over the points), the camera trans_mat [B][4][3]
 * (spatial_transformer) and the occupancy grid occ [B][R][R][R] (LIST.create_occ).  Exported from the same
 * liblist_hip.so as include/list_hip.h.
 *
 * Conventions: those of list_hip.h (raw device pointers, caller-owned buffers, work enqueued on the caller's stream,
 * no allocation and no synchronisation inside, LIST_OK or a negative ListStatus); the description of a failure is read
 * with list_coarse_last_error() (thread-local).  Shapes, pointers and sizes are checked on the host before any HIP call.
 *
 * Network (ListCoarseShape).  Tree decoder: n_features - 1 == n_degrees == L layers, 1 <= L <= LIST_COARSE_MAX_LAYERS;
 * layer l maps `node_l` nodes of features[l] values to node_l * degrees[l] nodes of features[l + 1] values (node_0 = 1):
 *   out[b][n deg + d] = act( sum_{i <= l} W_root[i] tree[i][b][n / (node_l / node_i)]
 *                            + Wc leaky( leaves[b][n] @ W_branch[n][:, d in : (d + 1) in] ) + bias[d] )
 * with leaky(x) = x > 0 ? x : 0.2 x, act = leaky for activation[l] != 0 (then with the bias) and the identity without
 * (then without the bias), and Wc = W_loop[1] W_loop[0] ([out][in]; the module has no nonlinearity between the two),
 * which the CALLER composes (in float64, rounded once to fp32).  features[l], l < L: a multiple of 16, at most 256;
 * features[l], l >= 1: at most 256; features[L] == 3; degrees >= 1; P = prod(degrees) <= 2^22.
 * Point MLP (has_mlp): 3 -> 64 -> 256 -> 512, each a 1x1 convolution with bias, eval-mode BN as y * s + t, then ReLU;
 * coarse[b][c] = max over the P points.  A NaN propagates as torch.max does: into that image's channel only.
 * Camera (has_camera, needs has_mlp): [coarse | feat_g2] (512 + g2 wide) -> Linear(hidden) -> leaky -> BN ->
 * Linear(hidden) -> leaky -> BN -> Linear(12).  1 <= g2 <= 1024, 1 <= hidden <= 256.
 * Occupancy: the grid is cleared, then for every point ijk = clamp(floor((p - bb_min) / bb_extent * (R - 1) + 0.5), 0,
 * R - 1) per axis in fp32, unfused, the division a division; occ[b][i][j][k] = 1.  A point with a non-finite
 * coordinate marks nothing (the torch module casts it to an integer, which is undefined).  1 <= R <= LIST_COARSE_MAX_R.
 *
 * Arithmetic: fp32 throughout.  The two wide layers of the point MLP run on the matrix cores with f32 operands
 * (v_mfma_f32_32x32x2_f32: exact fp32 products, fp32 accumulation); everything else on the vector ALU with fmaf
 * accumulation.  No atomics: the output is deterministic, bit for bit.
 *
 * W_branch (the decoder's weight stream, 268 MB for the default network) is read where the parameter lies:
 * ListCoarseIO.w_branch[l] points at the fp32 C-contiguous [node_l][in][deg * in] array, 16-byte aligned; the packed
 * blob holds no copy of it.  The blob holds, transposed for coalesced reads, Wc, the W_root matrices, the biases and
 * the point-MLP and camera parameters with BN folded to scale and shift (ListCoarseParams: all small).
 * Images are processed 16 per pass over W_branch.
 *
 * Call sequence:
 *   bytes = list_coarse_weight_bytes(&shape);                        (0: refused, see list_coarse_last_error)
 *   list_coarse_prep_weights(&shape, &params, packed, bytes, stream);          once per set of weights
 *   ws = list_coarse_workspace_bytes(&shape, B);
 *   list_coarse_forward(&shape, &io, stream);
 * The forward is list_coarse_n_steps() steps -- one launch per tree layer, then point_mlp, point_max, camera,
 * occ_clear, occ_mark -- and list_coarse_forward_steps runs a sub-range (the steps before `step_begin` must have run
 * on the same workspace and outputs).  A step whose output pointer is NULL launches nothing.
 */
#ifndef LIST_COARSE_H
#define LIST_COARSE_H

#include <stddef.h>
#include <stdint.h>

#include "list_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LIST_COARSE_MAX_LAYERS 8
#define LIST_COARSE_MAX_R 256
#define LIST_COARSE_CODE 512            /* width of the point MLP's output */
#define LIST_COARSE_GROUP 16            /* images per pass over W_branch */
#define LIST_COARSE_TILE 64             /* points per tile of the point MLP */

typedef struct ListCoarseShape {
  int32_t n_features, n_degrees;
  int32_t features[LIST_COARSE_MAX_LAYERS + 1];
  int32_t degrees[LIST_COARSE_MAX_LAYERS];
  int32_t activation[LIST_COARSE_MAX_LAYERS];
  int32_t has_mlp, has_camera;
  int32_t g2, hidden;                   /* camera: width of feat_g2, width of the two hidden layers */
} ListCoarseShape;

/* fp32 C-contiguous device arrays, read by list_coarse_prep_weights only.  Tree layer l: w_root[l][i]:
 * [features[l + 1]][features[i]], i <= l; wc[l]: [features[l + 1]][features[l]]; bias[l]: [degrees[l]][features[l + 1]]
 * (not read when activation[l] == 0).  Point MLP layer k (3 -> 64 -> 256 -> 512): mlp_w[k]: [out][in]; mlp_b, mlp_s,
 * mlp_t: [out] (s, t: the BN scale and shift).  Camera: cam_w[0]: [hidden][512 + g2], cam_w[1]: [hidden][hidden],
 * cam_w[2]: [12][hidden]; cam_b[k]; cam_s[k], cam_t[k] for k < 2. */
typedef struct ListCoarseParams {
  const float* w_root[LIST_COARSE_MAX_LAYERS][LIST_COARSE_MAX_LAYERS];
  const float* wc[LIST_COARSE_MAX_LAYERS];
  const float* bias[LIST_COARSE_MAX_LAYERS];
  const float* mlp_w[3];
  const float* mlp_b[3];
  const float* mlp_s[3];
  const float* mlp_t[3];
  const float* cam_w[3];
  const float* cam_b[3];
  const float* cam_s[2];
  const float* cam_t[2];
} ListCoarseParams;

typedef struct ListCoarseIO {
  int32_t B, R;
  float bb_min, bb_extent;              /* bb_extent = bb_max - bb_min, formed in double and rounded by the caller */
  const float* feat_g;                  /* [B][features[0]] */
  const float* feat_g2;                 /* [B][g2], or NULL: no trans_mat is computed */
  const float* w_branch[LIST_COARSE_MAX_LAYERS];
  const void* packed;
  size_t packed_bytes;
  void* workspace;
  size_t workspace_bytes;
  float* pc;                            /* [B][P][3] */
  float* coarse;                        /* [B][512], or NULL (then no trans_mat either) */
  float* trans_mat;                     /* [B][4][3], or NULL; left untouched when feat_g2 is NULL */
  float* occ;                           /* [B][R][R][R], or NULL */
} ListCoarseIO;

size_t list_coarse_weight_bytes(const ListCoarseShape* shape);
int list_coarse_prep_weights(const ListCoarseShape* shape, const ListCoarseParams* params, void* packed,
                             size_t packed_bytes, void* stream);
size_t list_coarse_workspace_bytes(const ListCoarseShape* shape, int32_t B);
int list_coarse_forward(const ListCoarseShape* shape, const ListCoarseIO* io, void* stream);
int32_t list_coarse_n_steps(const ListCoarseShape* shape);
int list_coarse_forward_steps(const ListCoarseShape* shape, const ListCoarseIO* io, int32_t step_begin,
                              int32_t step_end, void* stream);
const char* list_coarse_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* LIST_COARSE_H */
