// The z-buffer rasteriser of include/list_render.h on the device.  Every rule is a function of render_math.h; this file
// only decides which thread evaluates it where.
//
//   k_render_clear        keys[pixel] = background, the large-face counter and the stats record = 0.
//   k_render_setup_small  one thread per face: gathers and projects its vertices, snaps, applies the drop rules and
//                         clamps the bounding box.  A box of at most CAP x CAP centres is rasterised by the thread itself
//                         (one 64-bit atomicMin per covered centre); a larger one is appended to the large list (one
//                         integer atomicAdd per wave).  Faces are counted per outcome: ballots per wave, LDS per
//                         workgroup, one atomicAdd per workgroup and counter.
//   k_render_large        LIST_RENDER_LARGE_GROUPS persistent workgroups read the list's length on the device; each takes
//                         faces in turn, repeats the setup (uniform over the workgroup) and strides its 256 lanes over
//                         the bounding box.
//   k_render_resolve      per pixel: key -> face_id, depth; copies the stats record out.
//   k_render_shade        per pixel: face_id -> the face's colour, blended over the background.
//
// CAP = 8: marching-cubes faces of a 128^3 .. 256^3 volume at 224^2 .. 512^2 have boxes of 1 .. 5 centres a side, so
// nearly every face stays in its thread, and a thread's loop is at most 64 centres long beside neighbours of 1 .. 25.
// Nothing here waits for another thread; the atomics are integer minima and sums, so no result depends on an order.
#include <hip/hip_runtime.h>

#include "list_render.h"
#include "list_host.h"
#include "render_math.h"

static_assert(LIST_RENDER_CAP == RENDER_CAP && LIST_RENDER_N_STATS == RENDER_N_STATS, "list_render.h and render_math.h");
static_assert(LIST_RENDER_LIST == RENDER_LIST && LIST_RENDER_ORTHO == RENDER_ORTHO, "list_render.h and render_math.h");

namespace {

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 2048;            // grid-stride above this many workgroups (per-pixel kernels)

typedef unsigned long long Key;

__global__ __launch_bounds__(kThreads) void k_render_clear(Key* __restrict__ keys, int64_t n_pixels,
                                                            int32_t* __restrict__ count, int32_t* __restrict__ stats) {
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n_pixels; i += stride) keys[i] = RENDER_BACKGROUND_KEY;
  if (blockIdx.x == 0) {
    if (threadIdx.x < RENDER_N_STATS) stats[threadIdx.x] = 0;
    if (threadIdx.x == RENDER_N_STATS) *count = 0;
  }
}

// the outcome of face f and, for RENDER_SMALL / RENDER_LARGE, its setup
__device__ __forceinline__ int face_setup(const float* __restrict__ verts, uint32_t V, const int32_t* __restrict__ faces,
                                          int64_t f, const ListRenderCamera& cam, int W, int H, float z_near,
                                          RenderFace& face) {
  const int a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
  if (!((uint32_t)a < V && (uint32_t)b < V && (uint32_t)c < V)) return RENDER_BAD_INDEX;
  const float va[3] = {verts[3 * (int64_t)a], verts[3 * (int64_t)a + 1], verts[3 * (int64_t)a + 2]};
  const float vb[3] = {verts[3 * (int64_t)b], verts[3 * (int64_t)b + 1], verts[3 * (int64_t)b + 2]};
  const float vc[3] = {verts[3 * (int64_t)c], verts[3 * (int64_t)c + 1], verts[3 * (int64_t)c + 2]};
  const RenderVert ra = render_vertex(cam.T, cam.mode, cam.map_size, W, H, z_near, va);
  const RenderVert rb = render_vertex(cam.T, cam.mode, cam.map_size, W, H, z_near, vb);
  const RenderVert rc = render_vertex(cam.T, cam.mode, cam.map_size, W, H, z_near, vc);
  return render_face(ra, rb, rc, W, H, face);
}

// (ix, iy) lies inside the image: face.ix0 .. ix1 / iy0 .. iy1 are clamped to it
__device__ __forceinline__ void fragment(const RenderFace& face, int ix, int iy, int32_t f, int mode, int W,
                                         Key* __restrict__ keys) {
  int64_t e0, e1, e2;
  if (!render_covers(face, ix, iy, e0, e1, e2)) return;
  atomicMin(keys + ((int64_t)iy * W + ix), (Key)render_key(render_depth(face, e0, e1, e2), f, mode));
}

__global__ __launch_bounds__(kThreads) void k_render_setup_small(const float* __restrict__ verts, uint32_t V,
                                                                  const int32_t* __restrict__ faces, int64_t F,
                                                                  ListRenderCamera cam, int W, int H, float z_near,
                                                                  Key* __restrict__ keys, int32_t* __restrict__ list,
                                                                  int32_t* __restrict__ count,
                                                                  int32_t* __restrict__ stats) {
  __shared__ int s_stats[RENDER_N_STATS];
  if (threadIdx.x < RENDER_N_STATS) s_stats[threadIdx.x] = 0;
  __syncthreads();
  const int64_t f = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  const int lane = threadIdx.x & 63;
  int outcome = -1;
  RenderFace face;
  if (f < F) outcome = face_setup(verts, V, faces, f, cam, W, H, z_near, face);
  if (outcome == RENDER_SMALL) {
    for (int iy = face.iy0; iy <= face.iy1; ++iy)
      for (int ix = face.ix0; ix <= face.ix1; ++ix) fragment(face, ix, iy, (int32_t)f, cam.mode, W, keys);
  }
  // the wave's large faces: one atomicAdd reserves their slots (each face is appended once, so a slot is < F)
  const uint64_t big = __ballot(outcome == RENDER_LARGE);
  if (big) {
    const int leader = __ffsll((unsigned long long)big) - 1;
    int base = 0;
    if (lane == leader) base = atomicAdd(count, __popcll(big));
    base = __shfl(base, leader);
    if (outcome == RENDER_LARGE) list[base + __popcll(big & ((1ull << lane) - 1))] = (int32_t)f;
  }
  for (int k = 0; k < RENDER_N_STATS; ++k) {
    const uint64_t m = __ballot(outcome == k);
    if (lane == 0 && m) atomicAdd(&s_stats[k], __popcll(m));
  }
  __syncthreads();
  if (threadIdx.x < RENDER_N_STATS && s_stats[threadIdx.x]) atomicAdd(stats + threadIdx.x, s_stats[threadIdx.x]);
}

__global__ __launch_bounds__(kThreads) void k_render_large(const float* __restrict__ verts, uint32_t V,
                                                            const int32_t* __restrict__ faces, int64_t F,
                                                            ListRenderCamera cam, int W, int H, float z_near,
                                                            Key* __restrict__ keys, const int32_t* __restrict__ list,
                                                            const int32_t* __restrict__ count) {
  int64_t n = *count;                          // written by the launch before this one
  if (n > F) n = F;
  for (int64_t i = blockIdx.x; i < n; i += gridDim.x) {
    const int64_t f = list[i];
    if (f < 0 || f >= F) continue;
    RenderFace face;
    if (face_setup(verts, V, faces, f, cam, W, H, z_near, face) != RENDER_LARGE) continue;
    const int bw = face.ix1 - face.ix0 + 1;
    const int64_t n_centres = (int64_t)bw * (face.iy1 - face.iy0 + 1);
    for (int64_t t = threadIdx.x; t < n_centres; t += kThreads)
      fragment(face, face.ix0 + (int)(t % bw), face.iy0 + (int)(t / bw), (int32_t)f, cam.mode, W, keys);
  }
}

__global__ __launch_bounds__(kThreads) void k_render_resolve(const Key* __restrict__ keys, int64_t n_pixels, int mode,
                                                              const int32_t* __restrict__ stats,
                                                              int32_t* __restrict__ face_id, float* __restrict__ depth,
                                                              int32_t* __restrict__ stats_out) {
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n_pixels; i += stride) {
    const Key k = keys[i];
    face_id[i] = render_key_face(k);
    depth[i] = render_key_depth(k, mode);
  }
  if (blockIdx.x == 0 && threadIdx.x < RENDER_N_STATS) stats_out[threadIdx.x] = stats[threadIdx.x];
}

__global__ __launch_bounds__(kThreads) void k_render_shade(const float* __restrict__ verts, uint32_t V,
                                                            const int32_t* __restrict__ faces, uint32_t F,
                                                            const int32_t* __restrict__ face_id, ListRenderCamera cam,
                                                            int64_t n_pixels, int shade,
                                                            const uint8_t* __restrict__ background, int alpha256,
                                                            uint8_t* __restrict__ rgb) {
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n_pixels; i += stride) {
    int bg[3] = {255, 255, 255};
    if (background) {
      bg[0] = background[3 * i]; bg[1] = background[3 * i + 1]; bg[2] = background[3 * i + 2];
    }
    int out[3] = {bg[0], bg[1], bg[2]};
    const int32_t f = face_id[i];
    if ((uint32_t)f < F) {
      const int a = faces[3 * (int64_t)f], b = faces[3 * (int64_t)f + 1], c = faces[3 * (int64_t)f + 2];
      if ((uint32_t)a < V && (uint32_t)b < V && (uint32_t)c < V) {
        const float va[3] = {verts[3 * (int64_t)a], verts[3 * (int64_t)a + 1], verts[3 * (int64_t)a + 2]};
        const float vb[3] = {verts[3 * (int64_t)b], verts[3 * (int64_t)b + 1], verts[3 * (int64_t)b + 2]};
        const float vc[3] = {verts[3 * (int64_t)c], verts[3 * (int64_t)c + 1], verts[3 * (int64_t)c + 2]};
        float n[3];
        int fg[3];
        render_normal(va, vb, vc, n);
        if (shade == 0) render_shade_normal(n, fg);
        else fg[0] = fg[1] = fg[2] = render_shade_lambert(n, va, cam.eye);
        for (int k = 0; k < 3; ++k) out[k] = render_blend(fg[k], bg[k], alpha256);
      }
    }
    rgb[3 * i] = (uint8_t)out[0];
    rgb[3 * i + 1] = (uint8_t)out[1];
    rgb[3 * i + 2] = (uint8_t)out[2];
  }
}

// ---- workspace: keys u64 [H * W] | large list i32 [F] | large count i32, stats i32 [8] ----
struct Layout {
  size_t keys, list, counters, total;
};

int check_sizes(int64_t V, int64_t F, int64_t H, int64_t W) {
  if (V < 0 || F < 0 || V > INT32_MAX || F > INT32_MAX)
    return fail(LIST_ERR_SHAPE, "V = %lld, F = %lld: both must be in [0, INT32_MAX]", (long long)V, (long long)F);
  if (H < 1 || W < 1 || H > LIST_RENDER_MAX_SIDE || W > LIST_RENDER_MAX_SIDE || H * W > LIST_RENDER_MAX_PIXELS)
    return fail(LIST_ERR_SHAPE, "image of %lld x %lld: each side must be in [1, %d] and H * W <= %d (LIST_RENDER_MAX_SIDE, "
                "LIST_RENDER_MAX_PIXELS)", (long long)H, (long long)W, LIST_RENDER_MAX_SIDE, LIST_RENDER_MAX_PIXELS);
  return LIST_OK;
}

Layout layout(int64_t F, int64_t H, int64_t W) {
  Layout L;
  Carver c;
  L.keys = c.take((size_t)(H * W) * sizeof(Key));
  L.list = c.take((size_t)(F > 0 ? F : 1) * sizeof(int32_t));
  L.counters = c.take((1 + RENDER_N_STATS) * sizeof(int32_t));
  L.total = c.total();
  return L;
}

int check_camera(const ListRenderCamera* cam) {
  if (!cam) return fail(LIST_ERR_ARG, "camera is NULL");
  if (cam->mode != LIST_RENDER_ORTHO && cam->mode != LIST_RENDER_LIST)
    return fail(LIST_ERR_ARG, "camera mode %d: LIST_RENDER_ORTHO (0) or LIST_RENDER_LIST (1)", cam->mode);
  if (cam->mode == LIST_RENDER_LIST && cam->map_size < 2)
    return fail(LIST_ERR_ARG, "camera map_size %d: the LIST camera needs a plane of at least 2 x 2", cam->map_size);
  return LIST_OK;
}

}  // namespace

extern "C" {

const char* list_render_last_error(void) { return g_err; }

size_t list_render_workspace_bytes(int64_t F, int64_t H, int64_t W) {
  if (check_sizes(0, F, H, W) != LIST_OK) return 0;
  return layout(F, H, W).total;
}

int list_render_rasterize(const float* verts, int64_t V, const int32_t* faces, int64_t F, const ListRenderCamera* camera,
                          int64_t H, int64_t W, float z_near, void* workspace, size_t workspace_bytes, int32_t* face_id,
                          float* depth, int32_t* stats, int32_t step_begin, int32_t step_end, void* stream) {
  if (int rc = check_sizes(V, F, H, W)) return rc;
  if (int rc = check_camera(camera)) return rc;
  if (!(z_near >= 0.f) || z_near > 3.0e38f) return fail(LIST_ERR_ARG, "z_near = %g: must be finite and >= 0", (double)z_near);
  if ((V && !verts) || (F && !faces)) return fail(LIST_ERR_ARG, "verts/faces is NULL");
  if (!workspace || !face_id || !depth || !stats) return fail(LIST_ERR_ARG, "workspace/face_id/depth/stats is NULL");
  if (misaligned(workspace, 8)) return fail(LIST_ERR_ARG, "workspace must be aligned to 8 bytes");
  if (int rc = check_step_range("list_render_rasterize", step_begin, step_end, LIST_RENDER_N_STEPS)) return rc;
  const Layout L = layout(F, H, W);
  if (workspace_bytes < L.total) return workspace_too_small(workspace_bytes, L.total, "list_render_workspace_bytes");
  hipStream_t s = (hipStream_t)stream;
  Key* keys = at<Key>(workspace, L.keys);
  int32_t* list = at<int32_t>(workspace, L.list);
  int32_t* count = at<int32_t>(workspace, L.counters);
  int32_t* ws_stats = count + 1;
  const int64_t n_pixels = H * W;
  const dim3 per_pixel(blocks_capped(n_pixels, kThreads, kMaxBlocks)), block(kThreads);
  for (int step = step_begin; step < step_end; ++step) {
    int rc = LIST_OK;
    if (step == 0)
      rc = launch("k_render_clear", k_render_clear, per_pixel, block, s, keys, n_pixels, count, ws_stats);
    else if (step == 1 && F > 0)
      rc = launch("k_render_setup_small", k_render_setup_small, dim3(blocks_for(F, kThreads)), block, s, verts,
                  (uint32_t)V, faces, F, *camera, (int)W, (int)H, z_near, keys, list, count, ws_stats);
    else if (step == 2 && F > 0)
      rc = launch("k_render_large", k_render_large, dim3(LIST_RENDER_LARGE_GROUPS), block, s, verts, (uint32_t)V, faces,
                  F, *camera, (int)W, (int)H, z_near, keys, list, count);
    else if (step == 3)
      rc = launch("k_render_resolve", k_render_resolve, per_pixel, block, s, keys, n_pixels, camera->mode, ws_stats,
                  face_id, depth, stats);
    if (rc) return rc;
  }
  return LIST_OK;
}

int list_render_shade(const float* verts, int64_t V, const int32_t* faces, int64_t F, const int32_t* face_id,
                      const ListRenderCamera* camera, int64_t H, int64_t W, int32_t shade, const uint8_t* background,
                      int32_t alpha256, uint8_t* rgb, void* stream) {
  if (int rc = check_sizes(V, F, H, W)) return rc;
  if (int rc = check_camera(camera)) return rc;
  if (shade != 0 && shade != 1) return fail(LIST_ERR_ARG, "shade = %d: 0 (normal map) or 1 (head-light grey)", shade);
  if (alpha256 < 0 || alpha256 > 256) return fail(LIST_ERR_ARG, "alpha256 = %d: must be in [0, 256]", alpha256);
  if ((V && !verts) || (F && !faces)) return fail(LIST_ERR_ARG, "verts/faces is NULL");
  if (!face_id || !rgb) return fail(LIST_ERR_ARG, "face_id/rgb is NULL");
  const int64_t n_pixels = H * W;
  return launch("k_render_shade", k_render_shade, dim3(blocks_capped(n_pixels, kThreads, kMaxBlocks)), dim3(kThreads),
                (hipStream_t)stream, verts, (uint32_t)V, faces, (uint32_t)F, face_id, *camera, n_pixels, (int)shade,
                background, (int)alpha256, rgb);
}

}  // extern "C"
