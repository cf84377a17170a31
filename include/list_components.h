/*
 * list_components.h -- C ABI of the connected-component filter for predicted meshes on the MI355X (gfx950): label the
 * components of an indexed triangle mesh, count them, and copy out the kept ones, where list_mc_emit left the mesh.
 * The reference has no such step.  Exported from the same liblist_hip.so as include/list_hip.h.
 *
 * Conventions: those of list_mesh.h (raw device pointers, caller-owned buffers and workspace, work enqueued on the
 * caller's stream, no allocation and no synchronisation inside, LIST_OK or a negative ListStatus); the description of
 * a failure is read with list_cc_last_error() (thread-local).
 *
 * ---- semantics ------------------------------------------------------------------------------------------------------
 * Inputs.  verts float32 [V][3], faces int32 [F][3], 0 <= V, F <= INT32_MAX.  The vertices are the nodes; a face links
 * its three vertices, so two faces that share ONE vertex are connected (vertex connectivity, not edge adjacency).
 * A face with an index outside [0, V) is invalid: it links nothing, belongs to no component, never reaches the output,
 * and its index is never used as an address.  Degenerate faces (a,a,b / a,a,a) and duplicate faces are ordinary faces.
 *
 * Labels.  A vertex's label is the smallest vertex index of its component.  A vertex that no valid face uses belongs
 * to no component: its component id is -1 and it is never in the output.  Components are numbered 0 .. K-1 in
 * increasing order of label.  Each has a face count (its valid faces, duplicates counted), a vertex count and its
 * label (root); counts are int32.
 *
 * Compaction.  keep is one byte per component (non-zero: kept).  Kept vertices stay in their original order and are
 * copied bit for bit; kept faces stay in their original order with their indices remapped.  V' and F' are the sums of
 * the kept components' counts, so the caller allocates the outputs exactly.
 *
 * ---- call sequence --------------------------------------------------------------------------------------------------
 *   bytes = list_cc_workspace_bytes(V, F);                              (0: refused, see list_cc_last_error)
 *   list_cc_begin(faces, V, F, ws, bytes, stream);                      parent[v] = v, which vertices are used
 *   r = 0; do {                                                         n <= LIST_CC_MAX_ROUNDS - r
 *     list_cc_rounds(faces, V, F, ws, bytes, r, n, changed, stream);    changed: DEVICE int32[n]
 *     copy changed to the host; r += n;
 *   } while (changed[n - 1]);                                           a 0 anywhere ends the labelling
 *   list_cc_finish(faces, V, F, ws, bytes, component, roots, face_counts, vertex_counts, totals, stream);
 *   copy totals (DEVICE int64[2] = {K, invalid faces}) and the first K counts to the host, choose keep[K];
 *   list_cc_compact(verts, faces, V, F, component, keep, K, ws, bytes, out_verts, V', out_faces, F', stream);
 *
 * A round is one hook launch over the faces (each face finds its corners' roots and lowers the parent of every
 * larger root to the smallest one with an integer atomic minimum) and one compress launch over the vertices (every
 * vertex points at its root).  changed[i] is 1 iff round first_round + i saw a face with two different roots; once a
 * round of a call saw none, the later rounds of that call do nothing and report 0.  The labelling is complete at the
 * first 0.  first_round + n_rounds > LIST_CC_MAX_ROUNDS is refused with LIST_ERR_UNSUPPORTED: the caller's loop ends
 * with an error, it never spins.  No launch waits for another thread: every stored parent[x] <= x, so every pointer
 * chase descends and ends.
 *
 * list_cc_finish needs the completed labelling in the workspace.  component is int32 [V]; roots, face_counts and
 * vertex_counts have room for V entries each, of which the first K are written.
 * list_cc_compact reads nothing of the labelling from the workspace (it is scratch there): component and keep are its
 * inputs.  A component id >= K, or an output row at or past n_out_verts / n_out_faces, is skipped, never written.
 * With V = 0 or F = 0 every call returns LIST_OK without a launch that reads faces (list_cc_finish still writes
 * component = -1 and totals); list_cc_workspace_bytes is then small but not 0.
 * Results are deterministic: every output is a function of the inputs alone, bit for bit, though the number of rounds
 * a labelling takes may vary from run to run.
 */
#ifndef LIST_COMPONENTS_H
#define LIST_COMPONENTS_H

#include <stddef.h>
#include <stdint.h>

#include "list_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LIST_CC_MAX_ROUNDS 64

size_t list_cc_workspace_bytes(int64_t V, int64_t F);
int list_cc_begin(const int32_t* faces, int64_t V, int64_t F, void* workspace, size_t workspace_bytes, void* stream);
int list_cc_rounds(const int32_t* faces, int64_t V, int64_t F, void* workspace, size_t workspace_bytes,
                   int32_t first_round, int32_t n_rounds, int32_t* changed, void* stream);
int list_cc_finish(const int32_t* faces, int64_t V, int64_t F, void* workspace, size_t workspace_bytes,
                   int32_t* component, int32_t* roots, int32_t* face_counts, int32_t* vertex_counts, int64_t* totals,
                   void* stream);
int list_cc_compact(const float* verts, const int32_t* faces, int64_t V, int64_t F, const int32_t* component,
                    const uint8_t* keep, int64_t K, void* workspace, size_t workspace_bytes, float* out_verts,
                    int64_t n_out_verts, int32_t* out_faces, int64_t n_out_faces, void* stream);
const char* list_cc_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* LIST_COMPONENTS_H */
