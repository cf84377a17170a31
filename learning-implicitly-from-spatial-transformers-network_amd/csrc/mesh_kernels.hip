// Marching cubes on the device (include/list_mesh.h): the iso-surface of an SDF volume as shared vertices + triangles.
//
//   mc_count_kernel   one pass over the volume: per grid point, its cut-edge mask, its cell's case and the packed
//                     count (vertices | triangles << 32); slabs of the volume march through LDS so that each value is
//                     fetched about once.
//   exclusive scan    hipCUB over the packed counts: each point's first vertex (low 32 bits) and first triangle (high).
//   mc_totals_kernel  V and F into the caller's device int64[2].
//   mc_emit_kernel    per point with something to write: its vertices, and its cell's triangles, whose vertex numbers
//                     come from the scan and the masks of the points owning the cell's edges.
#include <hip/hip_runtime.h>

#include "list_cub.h"
#include "list_host.h"
#include "list_mesh.h"
#include "mc_tables.h"

namespace {

// count tile: 64 points along axis 2 (one wave) x 8 along axis 1, marching over 16 slices of axis 0
constexpr int kTK = 64, kTJ = 8, kTI = 16;
constexpr int kSliceW = kTK + 1, kSliceH = kTJ + 1, kSlice = kSliceW * kSliceH;
constexpr int kCountThreads = kTK * kTJ;
constexpr int kLoadsPerThread = (kSlice + kCountThreads - 1) / kCountThreads;
constexpr int kEmitThreads = 256;

__device__ __forceinline__ bool inside(float v, float level) { return v > level; }   // NaN: outside

// info[p] = case of the cell whose low corner is p (0 where no cell) | cut-edge mask << 8
__global__ __launch_bounds__(kCountThreads) void mc_count_kernel(const float* __restrict__ vol, int X, int Y, int Z,
                                                                  float level, uint64_t* __restrict__ counts,
                                                                  uint16_t* __restrict__ info) {
  __shared__ float s[3][kSliceH][kSliceW];
  const int tx = threadIdx.x, ty = threadIdx.y, tid = ty * kTK + tx;
  const int k0 = blockIdx.x * kTK, j0 = blockIdx.y * kTJ, i0 = blockIdx.z * kTI;
  const int64_t YZ = (int64_t)Y * Z;
  const int n = min(kTI, X - i0);                 // slices i0 .. i0+n-1 own points here; slice i0+n is read too

  float reg[kLoadsPerThread];
  auto fetch = [&](int i) {                       // slice i of the tile and its +1 halo on axes 1 and 2 into registers
#pragma unroll
    for (int r = 0; r < kLoadsPerThread; ++r) {
      const int e = tid + r * kCountThreads;
      const int jj = j0 + e / kSliceW, kk = k0 + e % kSliceW;
      reg[r] = (e < kSlice && i < X && jj < Y && kk < Z) ? vol[i * YZ + (int64_t)jj * Z + kk] : 0.f;
    }
  };
  auto store = [&](int b) {
#pragma unroll
    for (int r = 0; r < kLoadsPerThread; ++r) {
      const int e = tid + r * kCountThreads;
      if (e < kSlice) (&s[b][0][0])[e] = reg[r];
    }
  };
  fetch(i0);
  store(0);
  fetch(i0 + 1);
  store(1);
  __syncthreads();

  const int j = j0 + ty, k = k0 + tx;
  const bool owns = j < Y && k < Z;
  const bool hy = j + 1 < Y, hz = k + 1 < Z;
  for (int st = 0; st < n; ++st) {
    const int i = i0 + st;
    if (st + 1 < n) fetch(i + 2);                 // in flight while this slice is classified
    const int b0 = st % 3, b1 = (st + 1) % 3;
    if (owns) {
      const bool hx = i + 1 < X;
      const bool c0 = inside(s[b0][ty][tx], level), c1 = inside(s[b1][ty][tx], level);
      const bool c2 = inside(s[b0][ty + 1][tx], level), c3 = inside(s[b1][ty + 1][tx], level);
      const bool c4 = inside(s[b0][ty][tx + 1], level), c5 = inside(s[b1][ty][tx + 1], level);
      const bool c6 = inside(s[b0][ty + 1][tx + 1], level), c7 = inside(s[b1][ty + 1][tx + 1], level);
      const uint32_t mask = (hx && c0 != c1 ? 1u : 0u) | (hy && c0 != c2 ? 2u : 0u) | (hz && c0 != c4 ? 4u : 0u);
      uint32_t cs = 0;
      if (hx && hy && hz)
        cs = (uint32_t)c0 | (uint32_t)c1 << 1 | (uint32_t)c2 << 2 | (uint32_t)c3 << 3 | (uint32_t)c4 << 4 |
             (uint32_t)c5 << 5 | (uint32_t)c6 << 6 | (uint32_t)c7 << 7;
      const int64_t p = i * YZ + (int64_t)j * Z + k;
      counts[p] = (uint64_t)__popc(mask) | (uint64_t)kMcTriCount[cs] << 32;
      info[p] = (uint16_t)(cs | mask << 8);
    }
    if (st + 1 < n) store((st + 2) % 3);         // buffer of slice i-1, last read before the previous barrier
    __syncthreads();
  }
}

__global__ void mc_totals_kernel(const uint64_t* __restrict__ counts, const uint64_t* __restrict__ offsets,
                                 int64_t last, int64_t* __restrict__ totals) {
  const uint64_t t = offsets[last] + counts[last];
  totals[0] = (int64_t)(t & 0xffffffffu);
  totals[1] = (int64_t)(t >> 32);
}

__device__ __forceinline__ float edge_t(float v0, float v1, float level) {
  const float t = (level - v0) / (v1 - v0);
  return isfinite(t) ? fminf(fmaxf(t, 0.f), 1.f) : 0.5f;
}

__global__ __launch_bounds__(kEmitThreads) void mc_emit_kernel(
    const float* __restrict__ vol, int X, int Y, int Z, float level, float bx, float by, float bz, float sx, float sy,
    float sz, const uint64_t* __restrict__ offsets, const uint16_t* __restrict__ info, float* __restrict__ verts,
    int64_t n_verts, int32_t* __restrict__ faces, int64_t n_faces) {
  const int64_t YZ = (int64_t)Y * Z, N = X * YZ;
  const int64_t p = (int64_t)blockIdx.x * kEmitThreads + threadIdx.x;
  if (p >= N) return;
  const uint32_t inf = info[p];
  const uint32_t mask = inf >> 8, cs = inf & 0xff;
  const int ntri = kMcTriCount[cs];
  if (mask == 0 && ntri == 0) return;
  const uint64_t off = offsets[p];
  const int i = (int)(p / YZ), j = (int)((p - i * YZ) / Z), k = (int)(p - i * YZ - (int64_t)j * Z);
  if (mask) {
    const float v0 = vol[p];
    const float fx = (float)i * sx + bx, fy = (float)j * sy + by, fz = (float)k * sz + bz;
    int64_t vi = (int64_t)(uint32_t)off;
    if ((mask & 1) && vi < n_verts) {
      const float t = edge_t(v0, vol[p + YZ], level);
      float* o = verts + 3 * vi;
      o[0] = ((float)i + t) * sx + bx; o[1] = fy; o[2] = fz;
    }
    vi += mask & 1;
    if ((mask & 2) && vi < n_verts) {
      const float t = edge_t(v0, vol[p + Z], level);
      float* o = verts + 3 * vi;
      o[0] = fx; o[1] = ((float)j + t) * sy + by; o[2] = fz;
    }
    vi += (mask >> 1) & 1;
    if ((mask & 4) && vi < n_verts) {
      const float t = edge_t(v0, vol[p + 1], level);
      float* o = verts + 3 * vi;
      o[0] = fx; o[1] = fy; o[2] = ((float)k + t) * sz + bz;
    }
  }
  const int64_t t0 = (int64_t)(off >> 32);
  for (int t = 0; t < ntri; ++t) {
    if (t0 + t >= n_faces) break;
    int32_t idx[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      // edge e = 4 * axis + (o1 | o2 << 1): its owner is the cell's low corner moved by o1, o2 on the other two axes
      const int e = kMcTriEdges[cs][3 * t + c], a = e >> 2, o1 = e & 1, o2 = (e >> 1) & 1;
      const int dx = a == 0 ? 0 : o1, dy = a == 0 ? o1 : (a == 1 ? 0 : o2), dz = a == 2 ? 0 : o2;
      const int64_t q = p + dx * YZ + (int64_t)dy * Z + dz;
      const uint32_t mq = (uint32_t)info[q] >> 8;
      idx[c] = (int32_t)((uint32_t)offsets[q] + __popc(mq & ((1u << a) - 1u)));
    }
    int32_t* o = faces + 3 * (t0 + t);
    o[0] = idx[0]; o[1] = idx[1]; o[2] = idx[2];
  }
}

// ---- workspace: counts u64 [N] | offsets u64 [N] | info u16 [N] | scan scratch ----
struct Layout {
  size_t counts, offsets, info, scratch, scratch_bytes, total;
};

// LIST_OK, or a refusal with its message
int check_shape(int32_t X, int32_t Y, int32_t Z) {
  if (X < 2 || Y < 2 || Z < 2)
    return fail(LIST_ERR_SHAPE, "volume %d x %d x %d: every axis must be >= 2", X, Y, Z);
  if (3 * (int64_t)X * Y * Z > INT32_MAX)
    return fail(LIST_ERR_SHAPE, "volume %d x %d x %d: 3 * X * Y * Z exceeds INT32_MAX", X, Y, Z);
  return LIST_OK;
}

// the layout, or false with the refusal's message set
bool layout(int32_t X, int32_t Y, int32_t Z, Layout* L) {
  const size_t N = (size_t)X * Y * Z;
  if (!exclusive_sum_scratch<uint64_t>((int64_t)N, &L->scratch_bytes)) return false;
  Carver c;
  L->counts = c.take(N * sizeof(uint64_t));
  L->offsets = c.take(N * sizeof(uint64_t));
  L->info = c.take(N * sizeof(uint16_t));
  L->scratch = c.take(L->scratch_bytes);
  L->total = c.total();
  return true;
}

// the workspace of the entry points that take one: its layout, then its size
int check_ws(int32_t X, int32_t Y, int32_t Z, size_t workspace_bytes, Layout* L) {
  if (!layout(X, Y, Z, L)) return LIST_ERR_HIP;
  if (workspace_bytes < L->total) return workspace_too_small(workspace_bytes, L->total, "list_mc_workspace_bytes");
  return LIST_OK;
}

}  // namespace

extern "C" {

const char* list_mesh_last_error(void) { return g_err; }

size_t list_mc_workspace_bytes(int32_t X, int32_t Y, int32_t Z) {
  Layout L;
  return check_shape(X, Y, Z) == LIST_OK && layout(X, Y, Z, &L) ? L.total : 0;
}

int list_mc_count(const float* volume, int32_t X, int32_t Y, int32_t Z, float level, void* workspace,
                  size_t workspace_bytes, int64_t* totals, void* stream) {
  if (int rc = check_shape(X, Y, Z)) return rc;
  if (!volume || !workspace || !totals) return fail(LIST_ERR_ARG, "volume/workspace/totals is NULL");
  Layout L;
  if (int rc = check_ws(X, Y, Z, workspace_bytes, &L)) return rc;
  hipStream_t s = (hipStream_t)stream;
  uint64_t* counts = at<uint64_t>(workspace, L.counts);
  uint64_t* offsets = at<uint64_t>(workspace, L.offsets);
  const dim3 grid((Z + kTK - 1) / kTK, (Y + kTJ - 1) / kTJ, (X + kTI - 1) / kTI);
  if (int rc = launch("mc_count_kernel", mc_count_kernel, grid, dim3(kTK, kTJ), s, volume, X, Y, Z, level, counts,
                      at<uint16_t>(workspace, L.info)))
    return rc;
  const int64_t N = (int64_t)X * Y * Z;
  if (int rc = exclusive_sum(at<char>(workspace, L.scratch), L.scratch_bytes, counts, offsets, N, s)) return rc;
  return launch("mc_totals_kernel", mc_totals_kernel, dim3(1), dim3(1), s, counts, offsets, N - 1, totals);
}

int list_mc_emit(const float* volume, int32_t X, int32_t Y, int32_t Z, float level, const float bb_min[3],
                 const float bb_max[3], const void* workspace, size_t workspace_bytes, float* verts, int64_t n_verts,
                 int32_t* faces, int64_t n_faces, void* stream) {
  if (int rc = check_shape(X, Y, Z)) return rc;
  if (!volume || !workspace || !bb_min || !bb_max) return fail(LIST_ERR_ARG, "volume/workspace/bb_min/bb_max is NULL");
  if (n_verts < 0 || n_faces < 0) return fail(LIST_ERR_ARG, "n_verts=%lld n_faces=%lld", (long long)n_verts,
                                              (long long)n_faces);
  if (n_faces > INT32_MAX) return fail(LIST_ERR_SHAPE, "%lld triangles exceed INT32_MAX", (long long)n_faces);
  if (n_verts > INT32_MAX) return fail(LIST_ERR_SHAPE, "%lld vertices exceed INT32_MAX", (long long)n_verts);
  if ((n_verts && !verts) || (n_faces && !faces)) return fail(LIST_ERR_ARG, "verts/faces is NULL");
  Layout L;
  if (int rc = check_ws(X, Y, Z, workspace_bytes, &L)) return rc;
  if (n_verts == 0 && n_faces == 0) return LIST_OK;
  const int dims[3] = {X, Y, Z};
  float scale[3];
  for (int a = 0; a < 3; ++a) scale[a] = (float)(((double)bb_max[a] - (double)bb_min[a]) / (dims[a] - 1));
  const int64_t N = (int64_t)X * Y * Z;
  return launch("mc_emit_kernel", mc_emit_kernel, dim3(blocks_for(N, kEmitThreads)), dim3(kEmitThreads),
                (hipStream_t)stream, volume, X, Y, Z, level, bb_min[0], bb_min[1], bb_min[2], scale[0], scale[1],
                scale[2], at<uint64_t>(workspace, L.offsets), at<uint16_t>(workspace, L.info), verts, n_verts, faces,
                n_faces);
}

}  // extern "C"
