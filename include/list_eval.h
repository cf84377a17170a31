/*
 * list_eval.h -- C ABI of the mesh evaluation on the MI355X (gfx950): the three operations behind the reference's
 * eval_mesh (evaluation/eval_util.py: Chamfer-L2, precision/recall/F-score, volumetric IoU), computed where the
 * predicted mesh already sits.  Exported from the same liblist_hip.so as include/list_hip.h.
 *
 * Conventions: those of list_hip.h (raw device pointers, caller-owned buffers, work enqueued on the caller's stream,
 * no allocation and no synchronisation inside, LIST_OK or a negative ListStatus), except that the description of a
 * failure is read with list_eval_last_error() (thread-local, like list_last_error()).
 *
 * Meshes are verts float32 [V][3] and faces int32 [F][3], C-contiguous.  A face with an index outside [0, V) is
 * treated as degenerate: it is never sampled and never intersected (no out-of-bounds read).
 *
 * ---- nearest neighbour: list_eval_nn ----------------------------------------------------------------------------------
 * For every src[i] (float32 [N][3]): dist[i] = sqrt(min_j d2(i, j)) and idx[i] = the smallest j reaching that minimum,
 * over dst (float32 [M][3]), d2 = (dx*dx + dy*dy) + dz*dz in float32 with d = src - dst, no contraction into fma.
 * Brute force: dst tiles are staged in LDS; each lane keeps its src points and their minima in registers.
 * 1 <= M, 0 <= N, both <= INT32_MAX.  M == 0 is LIST_ERR_SHAPE.
 *
 * ---- area-weighted surface sampling: list_eval_sample ------------------------------------------------------------------
 * Face f has area a_f = 0.5 * |(v1 - v0) x (v2 - v0)| in float64 (vertices widened from float32; the cross product
 * c = (e1y*e2z - e1z*e2y, e1z*e2x - e1x*e2z, e1x*e2y - e1y*e2x), |c| = sqrt((cx*cx + cy*cy) + cz*cz)), and
 * cdf = inclusive prefix sum of a (float64; the association of the scan is the library's).  Sample s in [0, n):
 *   splitmix64(x):  z = x + 0x9E3779B97F4A7C15; z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9;
 *                   z = (z ^ z >> 27) * 0x94D049BB133111EB; return z ^ z >> 31          (uint64, wrapping)
 *   u_k(s)       =  (splitmix64(splitmix64(seed) ^ (3 * s + k)) >> 11) * 2^-53,  k = 0, 1, 2      (float64 in [0, 1))
 *   face         =  the first f with cdf[f] > u_0 * cdf[F-1] (the last face of positive area if there is none);
 *                   a face of zero area is never chosen
 *   r = sqrt(u_1), a = 1 - r, b = r * (1 - u_2), c = r * u_2
 *   point        =  float32((a * v0 + b * v1) + c * v2), per axis in float64
 * Output is deterministic for a given (mesh, n, seed).  F == 0 is LIST_ERR_SHAPE.  A total area that is not positive
 * and finite is only known on the device: every face_idx is then -1 and every point NaN.
 *
 * ---- inside test: list_eval_contains -----------------------------------------------------------------------------------
 * The reference's MeshIntersector.query (libmesh/inside_mesh.py with triangle_hash.pyx), in float64:
 *   vertices and points (float64 [Q][3]) are multiplied by rot (row-major float64 3x3, NULL = identity) as
 *   p'_r = (rot[r][0]*x + rot[r][1]*y) + rot[r][2]*z; the bounding box of the triangles' corners gives per axis
 *   scale = (res - 1) / (max - min), translate = 0.5 - scale * min, and every coordinate becomes scale * x + translate;
 *   a point outside 0 <= p <= res on any axis is culled (flags 0);
 *   a triangle is tested against a point iff its xy bounding box, truncated to int and clamped to [0, res-1], covers
 *   the point's cell (int(x), int(y)) (a cell outside [0, res)^2 tests nothing);
 *   check_triangles: strict 0 < u, v, u+v < |detA|, detA == 0 skipped; depth = t1z*|n_z| + alpha*sign(n_z), n_z == 0
 *   skipped; the hit counts toward parity 0 if depth >= z*|n_z|, toward parity 1 if depth < z*|n_z|.
 *   flags[q] bit 0 (LIST_EVAL_INSIDE) = both parities odd, bit 1 (LIST_EVAL_HOLE) = the parities differ.
 * The hash is built on the device: triangles sorted by the cell of their bbox's low corner (a CSR over the res^2
 * cells); a query scans the rows of cells that can hold a covering triangle, plus the list of wide triangles.  Parity
 * does not depend on the order, so flags are deterministic.  Every product and sum is evaluated in the order written
 * above, without contraction, so that a float64 restatement reproduces the flags bit for bit.
 * F == 0 is LIST_ERR_SHAPE.  A bounding box with a zero extent (the reference divides by it) is only known on the
 * device: every flags[q] is then LIST_EVAL_REFUSED and nothing else is computed.
 * 1 <= res <= LIST_EVAL_MAX_HASH_RES.
 */
#ifndef LIST_EVAL_H
#define LIST_EVAL_H

#include <stddef.h>
#include <stdint.h>

#include "list_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

enum ListEvalFlags { LIST_EVAL_INSIDE = 1, LIST_EVAL_HOLE = 2, LIST_EVAL_REFUSED = 128 };
#define LIST_EVAL_MAX_HASH_RES 8192

int list_eval_nn(const float* src, int64_t n_src, const float* dst, int64_t n_dst, float* dist, int32_t* idx,
                 void* stream);

size_t list_eval_sample_workspace_bytes(int64_t n_faces);
int list_eval_sample(const float* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces, int64_t n_samples,
                     uint64_t seed, void* workspace, size_t workspace_bytes, float* points, int32_t* face_idx,
                     void* stream);

size_t list_eval_contains_workspace_bytes(int64_t n_faces, int32_t hash_res);
int list_eval_contains(const float* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces,
                       const double* points, int64_t n_points, const double* rot, int32_t hash_res, void* workspace,
                       size_t workspace_bytes, uint8_t* flags, void* stream);

const char* list_eval_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* LIST_EVAL_H */
