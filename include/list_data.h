/*
 * list_data.h -- C ABI of the training-data preparation on the MI355X (gfx950): the signed distances and the
 * farthest-point clouds that the file-backed datasets read (the reference makes them offline with
 * preprocessing/preprocess.py and preprocessing/farthest_pointcloud.py).  Exported from the same liblist_hip.so as
 * include/list_hip.h.
 *
 * Conventions: those of list_eval.h (raw device pointers, caller-owned buffers, work enqueued on the caller's stream,
 * no allocation and no synchronisation inside, LIST_OK or a negative ListStatus); the description of a failure is
 * read with list_data_last_error() (thread-local).  Meshes are verts float32 [V][3] and faces int32 [F][3],
 * C-contiguous; a face with an index outside [0, V) is skipped (never read, never counted).  Every float32 expression
 * below is evaluated in the order written, without contraction into fma.
 *
 * ---- signed distance: list_data_signed_distance ----------------------------------------------------------------------
 * For every point p (float32 [Q][3]), over the valid faces f = (a, b, c) (corners as float32):
 *   magnitude  the exact distance to the closest triangle.  Per face, float32:
 *              ab = b - a, ac = c - a, n = ab x ac = (ab.y*ac.z - ab.z*ac.y, ab.z*ac.x - ab.x*ac.z, ab.x*ac.y - ab.y*ac.x).
 *              n == (0, 0, 0) (zero area): the closest point is the nearest of the edges ab, ac, bc (in that order, a
 *              later edge only when strictly nearer), each the segment point s + t*e, e the edge, s its start,
 *              t = clamp(dot(p - s, e) / dot(e, e), 0, 1), t = 0 when dot(e, e) == 0.
 *              Otherwise Ericson, Real-Time Collision Detection 5.1.5 (Voronoi regions, tested in this order), with
 *              ap = p - a, bp = p - b, cp = p - c, d1 = dot(ab, ap), d2 = dot(ac, ap), d3 = dot(ab, bp),
 *              d4 = dot(ac, bp), d5 = dot(ab, cp), d6 = dot(ac, cp):
 *                d1 <= 0 and d2 <= 0                              -> a
 *                d3 >= 0 and d4 <= d3                             -> b
 *                vc = d1*d4 - d3*d2 <= 0, d1 >= 0, d3 <= 0         -> a + v*ab,  v = d1 / (d1 - d3)
 *                d6 >= 0 and d5 <= d6                             -> c
 *                vb = d5*d2 - d1*d6 <= 0, d2 >= 0, d6 <= 0         -> a + w*ac,  w = d2 / (d2 - d6)
 *                va = d3*d6 - d5*d4 <= 0, d4 - d3 >= 0, d5 - d6 >= 0 -> b + w*(c - b),  w = (d4 - d3) / ((d4 - d3) + (d5 - d6))
 *                else                                             -> a + ab*v + ac*w,  den = 1 / ((va + vb) + vc),
 *                                                                    v = vb*den, w = vc*den
 *              (a division whose denominator is not > 0 gives 0, so no face produces a NaN; dot(u, v) =
 *              (u.x*v.x + u.y*v.y) + u.z*v.z).  With q the closest point, d2_f = (dx*dx + dy*dy) + dz*dz for
 *              d = p - q.  face_idx = the smallest f reaching min_f d2_f (faces visited in increasing order, strict <),
 *              |sdf| = sqrtf(min_f d2_f).
 *   sign       the generalised winding number w(p) = sum_f theta_f / (2*pi), theta_f = atan2(det, den) with
 *              a' = a - p, b' = b - p, c' = c - p, det = dot(a', b' x c'),
 *              den = ((|a'||b'||c'| + dot(a', b')|c'|) + dot(b', c')|a'|) + dot(c', a')|b'|, |u| = sqrt(dot(u, u))
 *              (Van Oosterom-Strackee: the face's solid angle is 2*theta_f); a zero-area face contributes 0.
 *              The device evaluates theta_f in float32 and sums it in float64, in increasing face order (so the
 *              result is the same bit for bit from run to run); a float64 restatement agrees within ~1e-5 away from
 *              the surface.  sdf = -|sdf| iff w(p) > 0.5 (negative inside, the sdf of SyntheticIM2SDF), else +|sdf|.
 *   winding    (optional, may be NULL) float32(w(p)).
 * With no valid face: sdf = +inf, face_idx = -1, winding = 0.
 * Brute force over the triangles: tiles of the per-face precompute (a, b, c, ab, ac, kind; workspace of
 * list_data_signed_distance_workspace_bytes(F)) are staged in LDS and read as broadcasts; each lane keeps its points,
 * their minima and winding sums in registers.  No atomics.  1 <= F, 1 <= V, 0 <= Q, all <= INT32_MAX; F == 0 is
 * LIST_ERR_SHAPE.
 *
 * ---- boundary samples: list_data_boundary_samples --------------------------------------------------------------------
 * out[i] = points[i] + sigma * n_i, n_i standard normal, for the surface points float32 [M][3]:
 *   u(c)        = the counter-based uniform of list_eval.h, (splitmix64(splitmix64(seed) ^ c) >> 11) * 2^-53
 *   c0          = 2^63 + 6*i + 2*k, k = 0, 1, 2 the axis (disjoint from list_eval_sample's counters 3*s + k < 2^63)
 *   n_{i,k}     = sqrt(-2 * log(1 - u(c0))) * cos(2*pi * u(c0 + 1))                          (Box-Muller, float64)
 *   out[i][k]   = float32(double(points[i][k]) + double(sigma) * n_{i,k})          (float64, rounded to float32 once)
 * sigma == 0 returns the points unchanged (the caller writes sdf = 0 exactly, as the reference does).
 * 0 <= M <= INT32_MAX.  out may not alias points.
 *
 * ---- farthest point sampling: list_data_farthest_points --------------------------------------------------------------
 * pytorch3d.ops.sample_farthest_points(random_start_point=False) over clouds float32 [B][N][3] -> idx int32 [B][K]:
 *   idx[b][0] = 0; m_j = +inf for every j; step s = 1 .. K-1: with l = idx[b][s-1], m_j = min(m_j, d2(j, l)),
 *   d2 = (dx*dx + dy*dy) + dz*dz in float32 (a NaN d2 leaves m_j as it was), and idx[b][s] = the j of the largest
 *   m_j, ties to the SMALLEST j.  Already chosen points have m_j = 0, so a cloud with fewer than K distinct points
 *   repeats indices (as pytorch3d does).
 * One workgroup per cloud, all B in one launch: each lane keeps the minima of its slice of points in registers (and
 * their coordinates too while N <= 16384); per step an argmax over the wave, then over the waves through LDS.
 * 1 <= N <= LIST_DATA_MAX_FPS_POINTS, 1 <= K <= N, 0 <= B <= INT32_MAX, otherwise LIST_ERR_SHAPE.
 */
#ifndef LIST_DATA_H
#define LIST_DATA_H

#include <stddef.h>
#include <stdint.h>

#include "list_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LIST_DATA_MAX_FPS_POINTS 65536

size_t list_data_signed_distance_workspace_bytes(int64_t n_faces);
int list_data_signed_distance(const float* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces,
                              const float* points, int64_t n_points, void* workspace, size_t workspace_bytes,
                              float* sdf, int32_t* face_idx, float* winding, void* stream);

int list_data_boundary_samples(const float* points, int64_t n_points, float sigma, uint64_t seed, float* out,
                               void* stream);

int list_data_farthest_points(const float* clouds, int64_t n_clouds, int64_t n_points, int64_t k, int32_t* idx,
                              void* stream);

const char* list_data_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* LIST_DATA_H */
