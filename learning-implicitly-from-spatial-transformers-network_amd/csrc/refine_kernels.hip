// Coarse-to-fine SDF grid on the device (include/list_refine.h): which fine points of an R^3 grid need an exact
// value, given the field on a coarse lattice, and the dense volume filled from the lattice, those exact values and
// trilinear interpolation.
//
//   refine_classify_kernel  one thread per brick: active from its 8 lattice corners (non-finite, sign, band).
//   refine_dilate_kernel    one thread per brick: OR over its 26-neighbourhood.
//   refine_flag_kernel      one thread per fine point: 1 iff it is no lattice point and a brick holding it is dilated.
//   exclusive scan          hipCUB over the flags: each refined point's slot (raster order of the fine index).
//   refine_total_kernel     the number of refined points into the caller's device int64.
//   refine_emit_kernel      one thread per fine point: a refined point writes its coordinates and flat index.
//   refine_fill_kernel      one thread per fine point: lattice value, refined value or trilinear interpolation.
// No atomics: every output element has exactly one writer, so the results are deterministic.
#include <hip/hip_runtime.h>

#include "list_cub.h"
#include "list_host.h"
#include "list_refine.h"

namespace {

constexpr int kThreads = 256;

struct Dims {
  int R, s, K, NB;
};

Dims dims_of(int32_t R, int32_t s) {
  Dims d;
  d.R = R;
  d.s = s;
  d.K = (R - 1 + s - 1) / s + 1;
  d.NB = d.K - 1;
  return d;
}

// lattice index of fine index i on its axis, -1 where i is no lattice index
__device__ __forceinline__ int lattice_of(int i, const Dims& d) {
  if (i == d.R - 1) return d.K - 1;
  return i % d.s == 0 ? i / d.s : -1;
}

__device__ __forceinline__ int corner_of(int m, const Dims& d) { return min(m * d.s, d.R - 1); }

// the brick whose corners interpolate fine index i
__device__ __forceinline__ int brick_of(int i, const Dims& d) { return min(i / d.s, d.NB - 1); }

__global__ __launch_bounds__(kThreads) void refine_classify_kernel(const float* __restrict__ lattice, Dims d,
                                                                     float level, float band,
                                                                     uint8_t* __restrict__ active) {
  const int64_t nb3 = (int64_t)d.NB * d.NB * d.NB;
  const int64_t b = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (b >= nb3) return;
  const int bx = (int)(b / ((int64_t)d.NB * d.NB)), by = (int)((b / d.NB) % d.NB), bz = (int)(b % d.NB);
  const int64_t K = d.K;
  bool bad = false, any_in = false, any_out = false, near = false;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const int64_t li = ((int64_t)(bx + (c & 1)) * K + (by + ((c >> 1) & 1))) * K + (bz + ((c >> 2) & 1));
    const float v = lattice[li];
    const bool in = v > level;
    bad |= !isfinite(v);
    any_in |= in;
    any_out |= !in;
    near |= fabsf(v - level) < band;
  }
  active[b] = (uint8_t)((bad || (any_in && any_out) || near) ? 1 : 0);
}

__global__ __launch_bounds__(kThreads) void refine_dilate_kernel(const uint8_t* __restrict__ active, Dims d,
                                                                   uint8_t* __restrict__ dilated) {
  const int n = d.NB;
  const int64_t nb3 = (int64_t)n * n * n;
  const int64_t b = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (b >= nb3) return;
  const int bx = (int)(b / ((int64_t)n * n)), by = (int)((b / n) % n), bz = (int)(b % n);
  uint8_t any = 0;
  for (int x = max(bx - 1, 0); x <= min(bx + 1, n - 1); ++x)
    for (int y = max(by - 1, 0); y <= min(by + 1, n - 1); ++y)
      for (int z = max(bz - 1, 0); z <= min(bz + 1, n - 1); ++z) any |= active[((int64_t)x * n + y) * n + z];
  dilated[b] = any;
}

// the bricks holding fine index i on its axis: [lo, hi]
__device__ __forceinline__ void bricks_holding(int i, const Dims& d, int* lo, int* hi) {
  const int m = lattice_of(i, d);
  if (m < 0) {
    *lo = *hi = i / d.s;
  } else {
    *lo = max(m - 1, 0);
    *hi = min(m, d.NB - 1);
  }
}

__global__ __launch_bounds__(kThreads) void refine_flag_kernel(const uint8_t* __restrict__ dilated, Dims d,
                                                                 uint32_t* __restrict__ flags) {
  const int64_t R = d.R, N = R * R * R;
  const int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (p >= N) return;
  const int i = (int)(p / (R * R)), j = (int)((p / R) % R), k = (int)(p % R);
  uint32_t f = 0;
  if (lattice_of(i, d) < 0 || lattice_of(j, d) < 0 || lattice_of(k, d) < 0) {
    int x0, x1, y0, y1, z0, z1;
    bricks_holding(i, d, &x0, &x1);
    bricks_holding(j, d, &y0, &y1);
    bricks_holding(k, d, &z0, &z1);
    const int64_t n = d.NB;
    for (int x = x0; x <= x1; ++x)
      for (int y = y0; y <= y1; ++y)
        for (int z = z0; z <= z1; ++z) f |= dilated[((int64_t)x * n + y) * n + z];
  }
  flags[p] = f;
}

__global__ void refine_total_kernel(const uint32_t* __restrict__ flags, const uint32_t* __restrict__ offsets,
                                    int64_t last, int64_t* __restrict__ total) {
  total[0] = (int64_t)offsets[last] + (int64_t)flags[last];
}

__device__ __forceinline__ float grid_coord(int t, int R, double lo, double hi, double step) {
  const double v = t == R - 1 ? hi : lo + (double)t * step;      // the dense grid's float64 arithmetic, end pinned
  return (float)v;
}

__global__ __launch_bounds__(kThreads) void refine_emit_kernel(const uint32_t* __restrict__ flags,
                                                                 const uint32_t* __restrict__ offsets, int R,
                                                                 double lo, double hi, double step,
                                                                 float* __restrict__ coords,
                                                                 int32_t* __restrict__ indices, int64_t n) {
  const int64_t RR = R, N = RR * RR * RR;
  const int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (p >= N || !flags[p]) return;
  const int64_t o = offsets[p];
  if (o >= n) return;
  const int i = (int)(p / (RR * RR)), j = (int)((p / RR) % RR), k = (int)(p % RR);
  indices[o] = (int32_t)p;
  float* c = coords + 3 * o;
  c[0] = grid_coord(i, R, lo, hi, step);
  c[1] = grid_coord(j, R, lo, hi, step);
  c[2] = grid_coord(k, R, lo, hi, step);
}

__device__ __forceinline__ float lerp(float a, float b, float t) { return a + t * (b - a); }

__global__ __launch_bounds__(kThreads) void refine_fill_kernel(const float* __restrict__ lattice,
                                                                 const float* __restrict__ values, int64_t n,
                                                                 const uint32_t* __restrict__ flags,
                                                                 const uint32_t* __restrict__ offsets, Dims d,
                                                                 float* __restrict__ volume) {
  const int64_t R = d.R, N = R * R * R, K = d.K;
  const int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (p >= N) return;
  const int i = (int)(p / (R * R)), j = (int)((p / R) % R), k = (int)(p % R);
  const int li = lattice_of(i, d), lj = lattice_of(j, d), lk = lattice_of(k, d);
  float out;
  if (li >= 0 && lj >= 0 && lk >= 0) {
    out = lattice[((int64_t)li * K + lj) * K + lk];
  } else if (flags[p]) {
    const int64_t o = offsets[p];
    out = o < n ? values[o] : __builtin_nanf("");
  } else {
    const int bx = brick_of(i, d), by = brick_of(j, d), bz = brick_of(k, d);
    const int cx = corner_of(bx, d), cy = corner_of(by, d), cz = corner_of(bz, d);
    const float tx = (float)(i - cx) / (float)(corner_of(bx + 1, d) - cx);
    const float ty = (float)(j - cy) / (float)(corner_of(by + 1, d) - cy);
    const float tz = (float)(k - cz) / (float)(corner_of(bz + 1, d) - cz);
    float c[2][2];
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
      for (int y = 0; y < 2; ++y) {
        const int64_t base = ((int64_t)(bx + x) * K + (by + y)) * K + bz;
        c[x][y] = lerp(lattice[base], lattice[base + 1], tz);
      }
    out = lerp(lerp(c[0][0], c[0][1], ty), lerp(c[1][0], c[1][1], ty), tx);
  }
  volume[p] = out;
}

// ---- workspace: active u8 [NB^3] | dilated u8 [NB^3] | flags u32 [R^3] | offsets u32 [R^3] | scan scratch ----
struct Layout {
  size_t active, dilated, flags, offsets, scratch, scratch_bytes, total;
};

// LIST_OK, or a refusal with its message
int check_shape(int32_t R, int32_t s) {
  if (s != 2 && s != 4 && s != 8) return fail(LIST_ERR_SHAPE, "stride s = %d: must be 2, 4 or 8", s);
  if (R < 2) return fail(LIST_ERR_SHAPE, "R = %d: the grid needs at least 2 points per axis", R);
  if (R > LIST_REFINE_MAX_R)
    return fail(LIST_ERR_SHAPE, "R = %d: R^3 exceeds INT32_MAX (at most R = %d)", R, LIST_REFINE_MAX_R);
  return LIST_OK;
}

// the regions before the scan scratch: host arithmetic only
void carve(int32_t R, int32_t s, Carver* c, Layout* L) {
  const Dims d = dims_of(R, s);
  const size_t nb3 = (size_t)d.NB * d.NB * d.NB, N = (size_t)R * R * R;
  L->active = c->take(nb3);
  L->dilated = c->take(nb3);
  L->flags = c->take(N * sizeof(uint32_t));
  L->offsets = c->take(N * sizeof(uint32_t));
}

// the layout, or false with the refusal's message set
bool layout(int32_t R, int32_t s, Layout* L) {
  if (!exclusive_sum_scratch<uint32_t>((int64_t)R * R * R, &L->scratch_bytes)) return false;
  Carver c;
  carve(R, s, &c, L);
  L->scratch = c.take(L->scratch_bytes);
  L->total = c.total();
  return true;
}

// shared checks of the entry points that take a workspace
int check_ws(int32_t R, int32_t s, const void* workspace, size_t workspace_bytes, Layout* L) {
  if (int rc = check_shape(R, s)) return rc;
  if (!workspace) return fail(LIST_ERR_ARG, "workspace is NULL");
  if (!layout(R, s, L)) return LIST_ERR_HIP;
  if (workspace_bytes < L->total) return workspace_too_small(workspace_bytes, L->total, "list_refine_workspace_bytes");
  return LIST_OK;
}

}  // namespace

extern "C" {

const char* list_refine_last_error(void) { return g_err; }

size_t list_refine_workspace_bytes(int32_t R, int32_t s) {
  Layout L;
  return check_shape(R, s) == LIST_OK && layout(R, s, &L) ? L.total : 0;
}

size_t list_refine_mask_offset(int32_t R, int32_t s) {
  if (check_shape(R, s) != LIST_OK) return 0;
  Carver c;
  Layout L;
  carve(R, s, &c, &L);
  return L.dilated;
}

int list_refine_count(const float* lattice, int32_t R, int32_t s, float level, float band, void* workspace,
                      size_t workspace_bytes, int64_t* total, void* stream) {
  if (int rc = check_shape(R, s)) return rc;
  if (!lattice || !total) return fail(LIST_ERR_ARG, "lattice/total is NULL");
  if (!isfinite(level)) return fail(LIST_ERR_ARG, "level = %g: must be finite", (double)level);
  if (!(band >= 0.f) || !isfinite(band)) return fail(LIST_ERR_ARG, "band = %g: must be finite and >= 0", (double)band);
  Layout L;
  if (int rc = check_ws(R, s, workspace, workspace_bytes, &L)) return rc;
  const Dims d = dims_of(R, s);
  hipStream_t st = (hipStream_t)stream;
  uint8_t* active = at<uint8_t>(workspace, L.active);
  uint8_t* dilated = at<uint8_t>(workspace, L.dilated);
  uint32_t* flags = at<uint32_t>(workspace, L.flags);
  uint32_t* offsets = at<uint32_t>(workspace, L.offsets);
  const int64_t nb3 = (int64_t)d.NB * d.NB * d.NB, N = (int64_t)R * R * R;
  const dim3 bricks(blocks_for(nb3, kThreads)), points(blocks_for(N, kThreads)), block(kThreads);
  if (int rc = launch("refine_classify_kernel", refine_classify_kernel, bricks, block, st, lattice, d, level, band, active))
    return rc;
  if (int rc = launch("refine_dilate_kernel", refine_dilate_kernel, bricks, block, st, active, d, dilated)) return rc;
  if (int rc = launch("refine_flag_kernel", refine_flag_kernel, points, block, st, dilated, d, flags)) return rc;
  if (int rc = exclusive_sum(at<char>(workspace, L.scratch), L.scratch_bytes, flags, offsets, N, st)) return rc;
  return launch("refine_total_kernel", refine_total_kernel, dim3(1), dim3(1), st, flags, offsets, N - 1, total);
}

int list_refine_emit(int32_t R, int32_t s, double lo, double hi, const void* workspace, size_t workspace_bytes,
                     float* coords, int32_t* indices, int64_t n, void* stream) {
  if (int rc = check_shape(R, s)) return rc;
  if (!isfinite(lo) || !isfinite(hi)) return fail(LIST_ERR_ARG, "lo = %g, hi = %g: must be finite", lo, hi);
  if (n < 0) return fail(LIST_ERR_ARG, "n = %lld", (long long)n);
  if (n > (int64_t)R * R * R) return fail(LIST_ERR_ARG, "n = %lld exceeds R^3", (long long)n);
  if (n && (!coords || !indices)) return fail(LIST_ERR_ARG, "coords/indices is NULL");
  Layout L;
  if (int rc = check_ws(R, s, workspace, workspace_bytes, &L)) return rc;
  if (n == 0) return LIST_OK;
  const int64_t N = (int64_t)R * R * R;
  const double step = (hi - lo) / (R - 1);
  return launch("refine_emit_kernel", refine_emit_kernel, dim3(blocks_for(N, kThreads)), dim3(kThreads),
                (hipStream_t)stream, at<uint32_t>(workspace, L.flags), at<uint32_t>(workspace, L.offsets), R, lo, hi,
                step, coords, indices, n);
}

int list_refine_fill(const float* lattice, const float* values, int64_t n, int32_t R, int32_t s,
                     const void* workspace, size_t workspace_bytes, float* volume, void* stream) {
  if (int rc = check_shape(R, s)) return rc;
  if (!lattice || !volume) return fail(LIST_ERR_ARG, "lattice/volume is NULL");
  if (n < 0) return fail(LIST_ERR_ARG, "n = %lld", (long long)n);
  if (n && !values) return fail(LIST_ERR_ARG, "values is NULL");
  Layout L;
  if (int rc = check_ws(R, s, workspace, workspace_bytes, &L)) return rc;
  const int64_t N = (int64_t)R * R * R;
  return launch("refine_fill_kernel", refine_fill_kernel, dim3(blocks_for(N, kThreads)), dim3(kThreads),
                (hipStream_t)stream, lattice, values, n, at<uint32_t>(workspace, L.flags),
                at<uint32_t>(workspace, L.offsets), dims_of(R, s), volume);
}

}  // extern "C"
