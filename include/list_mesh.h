/*
 * list_mesh.h -- C ABI of the marching-cubes mesh extraction on the MI355X (gfx950): the iso-surface of a
 * predicted SDF volume (the reference's test(): marching cubes on the res^3 grid, utils.py:172-182), computed
 * where the volume already sits.  Exported from the same liblist_hip.so as include/list_hip.h.
 *
 * Conventions: those of list_hip.h (raw device pointers, caller-owned buffers, work enqueued on the caller's stream,
 * no allocation and no synchronisation inside, LIST_OK or a negative ListStatus), except that the description of a
 * failure is read with list_mesh_last_error() (thread-local, like list_last_error()).
 *
 * Field.  volume is a C-contiguous float32 [X][Y][Z] array, every axis >= 2, 3*X*Y*Z <= INT32_MAX.  A corner is
 * inside iff v > level (NaN is outside).  This is the surface mcubes.marching_cubes(-v, -level) extracts.
 *
 * Output.  Each grid point owns its +axis-0, +axis-1 and +axis-2 edges and emits one vertex (in that order) per edge
 * whose ends are on different sides; the vertices are in raster order of their points, shared by every triangle that
 * uses them.  A vertex lies at t = (level - v0) / (v1 - v0) along its edge, clamped to [0, 1] (0.5 where t is not
 * finite), mapped per axis to bb_min + (idx + t) * (bb_max - bb_min) / (n - 1).  The triangles follow in raster
 * order of their cells, with their right-hand normals toward decreasing v.  The case tables are
 * csrc/mc_tables.h (tools/gen_mc_tables.py).  Output is deterministic, bit for bit.
 *
 * Call sequence:
 *   bytes = list_mc_workspace_bytes(X, Y, Z);                         (0: shape refused, see list_mesh_last_error)
 *   list_mc_count(volume, X, Y, Z, level, ws, bytes, totals, stream); totals: DEVICE int64[2] = {V, F}
 *   copy totals to the host (the one synchronisation), allocate verts float32 [V][3] and faces int32 [F][3];
 *   list_mc_emit(volume, X, Y, Z, level, bb_min, bb_max, ws, bytes, verts, V, faces, F, stream);
 * list_mc_emit reads what list_mc_count left in the workspace: same volume, shape, level and workspace, with the
 * volume unchanged in between.  It writes no more than V vertices and F faces; F > INT32_MAX is refused.
 */
#ifndef LIST_MESH_H
#define LIST_MESH_H

#include <stddef.h>
#include <stdint.h>

#include "list_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

size_t list_mc_workspace_bytes(int32_t X, int32_t Y, int32_t Z);
int list_mc_count(const float* volume, int32_t X, int32_t Y, int32_t Z, float level, void* workspace,
                  size_t workspace_bytes, int64_t* totals, void* stream);
int list_mc_emit(const float* volume, int32_t X, int32_t Y, int32_t Z, float level, const float bb_min[3],
                 const float bb_max[3], const void* workspace, size_t workspace_bytes, float* verts, int64_t n_verts,
                 int32_t* faces, int64_t n_faces, void* stream);
const char* list_mesh_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* LIST_MESH_H */
