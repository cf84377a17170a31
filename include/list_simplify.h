/*
 * list_simplify.h -- C ABI of the mesh simplifier for predicted meshes on the MI355X (gfx950): uniform-grid vertex
 * clustering (Rossignac-Borrel) of an indexed triangle mesh, where list_mc_emit / list_cc_compact left it.  The
 * reference has no such step.  Exported from the same liblist_hip.so as include/list_hip.h.
 *
 * Conventions: those of list_mesh.h (raw device pointers, caller-owned buffers and workspace, work enqueued on the
 * caller's stream, no allocation and no synchronisation inside, LIST_OK or a negative ListStatus); the description of
 * a failure is read with list_simp_last_error() (thread-local).  cells, lo, inv and cell are HOST arrays of 3.
 *
 * ---- the rule -------------------------------------------------------------------------------------------------------
 * Inputs.  verts float32 [V][3], faces int32 [F][3], 0 <= V, F <= INT32_MAX.  cells = (R0, R1, R2), 1 <= Ra <= 1024.
 * Bounds lo[a] < hi[a], finite, float64.  The host computes inv[a] = Ra / (hi[a] - lo[a]) and
 * cell[a] = (hi[a] - lo[a]) / Ra in float64 and passes these doubles, so both sides hold the same bits.
 *
 * Per vertex, per axis, in float64 with every operation rounded on its own (no fused multiply-add):
 *   t = (double)v - lo;  u = clamp(t * inv, 0, R)       a vertex outside the box goes onto the box face
 *   i = min((int64)floor(u), R - 1);  q = llrint((u - i) * 2^30)      ties to even, 0 <= q <= 2^30
 *   key = (i0 * R1 + i1) * R2 + i2 < 2^30
 * A vertex with a non-finite coordinate is invalid: it is in no cluster.  A face with an index outside [0, V) or with
 * an invalid corner is invalid: it is never in the output and its index is never used as an address.
 *
 * Clusters.  A cluster is the set of valid vertices with one key; clusters are numbered in ascending key.  Per cluster
 * and axis S = sum of q (int64, at most 2^31 * 2^30) and n = count.  Its representative, every integer-to-double
 * conversion being exact:  a = S / n, r = S % n (integers);  m = ((double)a + (double)r / (double)n) * 2^-30;
 * p = (float)(lo + ((double)i + m) * cell).
 *
 * Faces.  A valid face whose three corners do not lie in three different clusters is degenerate and dropped.  Every
 * other valid face is kept, in its original order and orientation, with its corners replaced by cluster numbers.
 * Duplicate faces and opposite pairs (a,b,c) / (a,c,b) are ordinary faces and stay: a vertex map sends a closed
 * surface to a mod-2 cycle, so every edge of the output of a closed input lies in an even number of faces; removing
 * duplicates would break that.
 *
 * Output.  Clusters that no kept face uses are dropped and the rest renumbered in ascending key: V' vertices, F' faces.
 * vertex_map int32 [V] holds the output vertex of each input vertex, -1 if it is invalid or its cluster was dropped.
 * totals int64 [6] = {V', F', clusters, invalid vertices, invalid faces, degenerate faces}.  Every output is a function
 * of the inputs alone, bit for bit (the sums are integers: no order of additions changes them), and does not depend on
 * the order of the input vertices; the faces follow the input face order.
 *
 * ---- call sequence --------------------------------------------------------------------------------------------------
 *   bytes = list_simp_workspace_bytes(V, F, cells);                     (0: refused, see list_simp_last_error)
 *   list_simp_count(verts, faces, V, F, cells, lo, inv, ws, bytes, vertex_map, totals, stream);
 *   copy totals (DEVICE int64[6]) to the host, allocate out_verts [V'][3] and out_faces [F'][3];
 *   list_simp_emit(faces, V, F, cells, lo, cell, vertex_map, ws, bytes, out_verts, V', out_faces, F', stream);
 *
 * list_simp_count builds keys, clusters, sums, the face classes and vertex_map, and leaves them in the workspace, which
 * list_simp_emit reads: the same workspace, untouched in between, and the same V, F, cells and faces.  An output row at
 * or past n_out_verts / n_out_faces is skipped, never written.  With V = 0 or F = 0 every call returns LIST_OK and
 * list_simp_count writes the totals (V' = F' = 0); list_simp_workspace_bytes is then small but not 0.
 * No float atomics anywhere; no thread waits for another.
 */
#ifndef LIST_SIMPLIFY_H
#define LIST_SIMPLIFY_H

#include <stddef.h>
#include <stdint.h>

#include "list_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LIST_SIMP_MAX_CELLS 1024
#define LIST_SIMP_N_TOTALS 6

size_t list_simp_workspace_bytes(int64_t V, int64_t F, const int32_t* cells);
int list_simp_count(const float* verts, const int32_t* faces, int64_t V, int64_t F, const int32_t* cells,
                    const double* lo, const double* inv, void* workspace, size_t workspace_bytes, int32_t* vertex_map,
                    int64_t* totals, void* stream);
int list_simp_emit(const int32_t* faces, int64_t V, int64_t F, const int32_t* cells, const double* lo,
                   const double* cell, const int32_t* vertex_map, void* workspace, size_t workspace_bytes,
                   float* out_verts, int64_t n_out_verts, int32_t* out_faces, int64_t n_out_faces, void* stream);
const char* list_simp_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* LIST_SIMPLIFY_H */
