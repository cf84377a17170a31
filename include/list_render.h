/*
 * list_render.h -- C ABI of the z-buffer rasteriser for predicted meshes on the MI355X (gfx950): depth map, face-id map
 * and a shaded picture of an indexed triangle mesh, where list_mc_emit / list_cc_compact left it, from the model's own
 * camera (the 4x3 trans_mat of the spatial transformer) or from an orthographic one.  The reference has only three
 * axis-aligned silhouettes of the volume (utils.render_grid_occupancy).  Exported from the same liblist_hip.so as
 * include/list_hip.h.
 *
 * Conventions: those of list_mesh.h (raw device pointers, caller-owned buffers and workspace, work enqueued on the
 * caller's stream, no allocation and no synchronisation inside, LIST_OK or a negative ListStatus); the description of
 * a failure is read with list_render_last_error() (thread-local).  The camera is read on the host, during the call.
 *
 * ---- semantics (csrc/render_math.h holds every rule as code; list_amd/render.py restates them in numpy) ---------------
 * Inputs.  verts float32 [V][3] in the coordinates list_mc_emit writes (axes in array order), faces int32 [F][3],
 * 0 <= V, F <= INT32_MAX; an image of H rows and W columns, 1 <= H, W <= LIST_RENDER_MAX_SIDE and
 * H * W <= LIST_RENDER_MAX_PIXELS.  Pixel (x, y) is column x of row y; its centre has the coordinates (x, y).
 *
 * Camera.  T is a 4x3 matrix, row-major as trans_mat[b].  A vertex v becomes p = 2 * (v[2], v[1], v[0]) -- the query
 * permutation and scale of models.py:91-92 -- and X, Y, Z = [p, 1] T by the fma chain, in k order, of the query path's
 * projection (csrc/point_math.h: project).
 *   LIST_RENDER_LIST   den = Z + 1e-8f; u = X / den, v = Y / den on the map_size plane, WITHOUT the reference's clamp to
 *                      [0, map_size - 1]; pixel x = u * (W - 1) / (map_size - 1), y = v * (H - 1) / (map_size - 1), in
 *                      float64 from the float32 X, Y, den.  Visibility by 1 / den: larger is nearer.
 *   LIST_RENDER_ORTHO  x = X, y = Y; visibility by Z: smaller is nearer.
 * eye is the camera's centre in homogeneous mesh coordinates (eye[3] = 0: a direction), used by the head-light only.
 *
 * Rules.  Coordinates snap to 1/16 pixel: floor(x * 16 + 0.5) in float64.  A face is dropped whole, and counted, for
 * the first of: a vertex index outside [0, V); a non-finite X, Y or Z (den); LIST camera and a den <= z_near (there is
 * no clipping); a snapped coordinate beyond +-2^24 sub-pixels; zero area after snapping.  Coverage: int64 edge
 * functions with the top-left fill rule, both windings drawn, so two faces that share an edge cover each centre on it
 * exactly once.  Depth at a centre: ((e0 * d0 + e1 * d1) + e2 * d2) / area in float64 -- e: the edge values, d: the
 * vertices' 1 / den or Z -- rounded to float32.  The pixel's winner is the nearest fragment and, among equal float32
 * depths, the lowest face index: one 64-bit key per pixel (monotone depth bits above the face index) and an integer
 * atomic minimum, so the result does not depend on the launch order.
 *
 * Outputs of list_render_rasterize.  face_id int32 [H][W], -1 on background; depth float32 [H][W], den (LIST) or Z
 * (orthographic) recovered from the key, +inf on background; stats int32 [LIST_RENDER_N_STATS], every face in exactly
 * one counter: bad_index, non_finite, behind_near, guard_band, zero_area, offscreen (valid, but no pixel centre of the
 * image in its bounding box), small, large (rasterised by the per-thread / by the workgroup path: a clamped bounding
 * box of at most LIST_RENDER_CAP x LIST_RENDER_CAP pixels is small).
 *
 * list_render_shade.  From face_id (a value outside [0, F), or a face with an index outside [0, V), is background): the
 * face normal n = (b - a) x (c - a) in float32; shade 0: normal map, rgb = round((n / |n| * 0.5 + 0.5) * 255) in mesh axis
 * order; shade 1: head-light grey round(|n . d| / (|n| |d|) * 255), d = eye.xyz - eye.w * a.  background: optional
 * uint8 [H][W][3] (NULL: white).  alpha256 in [0, 256]: out = (alpha256 * shade + (256 - alpha256) * background + 128)
 * >> 8 on the mesh's pixels, the background elsewhere.  rgb uint8 [H][W][3].
 *
 * The steps of list_render_rasterize are four launches -- clear, setup + small faces, large faces, resolve -- of which
 * [step_begin, step_end) run (timing tools; callers pass 0, LIST_RENDER_N_STEPS).  The large-face launch is a fixed grid
 * of LIST_RENDER_LARGE_GROUPS workgroups that read the list's length on the device.
 * Results are deterministic: every output is a function of the inputs alone, bit for bit.
 */
#ifndef LIST_RENDER_H
#define LIST_RENDER_H

#include <stddef.h>
#include <stdint.h>

#include "list_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LIST_RENDER_ORTHO 0
#define LIST_RENDER_LIST 1
#define LIST_RENDER_N_STATS 8
#define LIST_RENDER_N_STEPS 4
#define LIST_RENDER_CAP 8
#define LIST_RENDER_LARGE_GROUPS 256
#define LIST_RENDER_MAX_SIDE 16384
#define LIST_RENDER_MAX_PIXELS (1 << 26)

typedef struct ListRenderCamera {
  float T[12];
  float eye[4];
  int32_t mode;
  int32_t map_size; /* LIST_RENDER_LIST: >= 2 */
} ListRenderCamera;

size_t list_render_workspace_bytes(int64_t F, int64_t H, int64_t W);
int list_render_rasterize(const float* verts, int64_t V, const int32_t* faces, int64_t F, const ListRenderCamera* camera,
                          int64_t H, int64_t W, float z_near, void* workspace, size_t workspace_bytes, int32_t* face_id,
                          float* depth, int32_t* stats, int32_t step_begin, int32_t step_end, void* stream);
int list_render_shade(const float* verts, int64_t V, const int32_t* faces, int64_t F, const int32_t* face_id,
                      const ListRenderCamera* camera, int64_t H, int64_t W, int32_t shade, const uint8_t* background,
                      int32_t alpha256, uint8_t* rgb, void* stream);
const char* list_render_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* LIST_RENDER_H */
