// Training-data preparation on the device (include/list_data.h): signed point-to-mesh distance, boundary samples and
// farthest point sampling.
//
//   face_prep_kernel      per face: corners, edges ab / ac and its kind (valid, zero area, skipped) into the workspace.
//   sdf_kernel<R>         brute force over the faces: face tiles staged in LDS, R points per lane in registers with
//                         their running minimum, closest face and winding sum.
//   boundary_kernel       per point: Box-Muller over the counter-based uniforms of list_eval.h.
//   fps_kernel<P>         one workgroup per cloud, P points per lane: running minima in registers, argmax per step
//                         over the wave (shuffles) and then over the waves (LDS).
#include <math.h>

#include <hip/hip_runtime.h>

#include "list_data.h"
#include "list_host.h"

#pragma clang fp contract(off)

namespace {

// ---- signed distance --------------------------------------------------------------------------------------------------
constexpr int kThreads = 256;
constexpr int kTile = 256;                // faces per LDS tile (one per thread to stage)
constexpr float kKindValid = 0.f, kKindFlat = 1.f, kKindSkip = 2.f;

struct FacePrep {                         // 80 bytes per face: the workspace of list_data_signed_distance
  float4 a;                               // corner a, .w = kind
  float4 b, c, ab, ac;                    // corners b, c and the edges b - a, c - a (.w unused)
};

__global__ __launch_bounds__(kThreads) void face_prep_kernel(const float* __restrict__ verts, int64_t V,
                                                             const int32_t* __restrict__ faces, int64_t F,
                                                             FacePrep* __restrict__ prep) {
  const int64_t f = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (f >= F) return;
  const int32_t i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
  FacePrep o;
  if (!(i0 >= 0 && i0 < V && i1 >= 0 && i1 < V && i2 >= 0 && i2 < V)) {
    o.a = o.b = o.c = o.ab = o.ac = make_float4(0.f, 0.f, 0.f, 0.f);
    o.a.w = kKindSkip;
    prep[f] = o;
    return;
  }
  const float* va = verts + 3 * (int64_t)i0;
  const float* vb = verts + 3 * (int64_t)i1;
  const float* vc = verts + 3 * (int64_t)i2;
  const float abx = vb[0] - va[0], aby = vb[1] - va[1], abz = vb[2] - va[2];
  const float acx = vc[0] - va[0], acy = vc[1] - va[1], acz = vc[2] - va[2];
  const float nx = aby * acz - abz * acy, ny = abz * acx - abx * acz, nz = abx * acy - aby * acx;
  const bool flat = nx == 0.f && ny == 0.f && nz == 0.f;
  o.a = make_float4(va[0], va[1], va[2], flat ? kKindFlat : kKindValid);
  o.b = make_float4(vb[0], vb[1], vb[2], 0.f);
  o.c = make_float4(vc[0], vc[1], vc[2], 0.f);
  o.ab = make_float4(abx, aby, abz, 0.f);
  o.ac = make_float4(acx, acy, acz, 0.f);
  prep[f] = o;
}

__device__ __forceinline__ float dot3(float ux, float uy, float uz, float vx, float vy, float vz) {
  return (ux * vx + uy * vy) + uz * vz;
}

__device__ __forceinline__ float safe_div(float n, float d) { return d > 0.f ? n / d : 0.f; }

// squared distance from p to the segment s + t*e, t clamped to [0, 1]
__device__ __forceinline__ float seg_d2(float px, float py, float pz, float sx, float sy, float sz, float ex, float ey,
                                        float ez) {
  const float ee = dot3(ex, ey, ez, ex, ey, ez);
  float t = ee > 0.f ? dot3(px - sx, py - sy, pz - sz, ex, ey, ez) / ee : 0.f;
  t = fminf(fmaxf(t, 0.f), 1.f);
  const float dx = px - (sx + t * ex), dy = py - (sy + t * ey), dz = pz - (sz + t * ez);
  return (dx * dx + dy * dy) + dz * dz;
}

// Ericson 5.1.5, the closest point of a triangle of non-zero area -> squared distance
__device__ __forceinline__ float tri_d2(float px, float py, float pz, const FacePrep& t) {
  const float ax = t.a.x, ay = t.a.y, az = t.a.z;
  const float abx = t.ab.x, aby = t.ab.y, abz = t.ab.z, acx = t.ac.x, acy = t.ac.y, acz = t.ac.z;
  const float apx = px - ax, apy = py - ay, apz = pz - az;
  const float bpx = px - t.b.x, bpy = py - t.b.y, bpz = pz - t.b.z;
  const float cpx = px - t.c.x, cpy = py - t.c.y, cpz = pz - t.c.z;
  const float d1 = dot3(abx, aby, abz, apx, apy, apz), d2 = dot3(acx, acy, acz, apx, apy, apz);
  const float d3 = dot3(abx, aby, abz, bpx, bpy, bpz), d4 = dot3(acx, acy, acz, bpx, bpy, bpz);
  const float d5 = dot3(abx, aby, abz, cpx, cpy, cpz), d6 = dot3(acx, acy, acz, cpx, cpy, cpz);
  const float vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
  float qx, qy, qz;
  if (d1 <= 0.f && d2 <= 0.f) {
    qx = ax; qy = ay; qz = az;
  } else if (d3 >= 0.f && d4 <= d3) {
    qx = t.b.x; qy = t.b.y; qz = t.b.z;
  } else if (vc <= 0.f && d1 >= 0.f && d3 <= 0.f) {
    const float v = safe_div(d1, d1 - d3);
    qx = ax + v * abx; qy = ay + v * aby; qz = az + v * abz;
  } else if (d6 >= 0.f && d5 <= d6) {
    qx = t.c.x; qy = t.c.y; qz = t.c.z;
  } else if (vb <= 0.f && d2 >= 0.f && d6 <= 0.f) {
    const float w = safe_div(d2, d2 - d6);
    qx = ax + w * acx; qy = ay + w * acy; qz = az + w * acz;
  } else if (va <= 0.f && d4 - d3 >= 0.f && d5 - d6 >= 0.f) {
    const float w = safe_div(d4 - d3, (d4 - d3) + (d5 - d6));
    qx = t.b.x + w * (t.c.x - t.b.x); qy = t.b.y + w * (t.c.y - t.b.y); qz = t.b.z + w * (t.c.z - t.b.z);
  } else {
    const float s = (va + vb) + vc;
    const float den = s > 0.f ? 1.f / s : 0.f;
    const float v = vb * den, w = vc * den;
    qx = (ax + abx * v) + acx * w; qy = (ay + aby * v) + acy * w; qz = (az + abz * v) + acz * w;
  }
  const float dx = px - qx, dy = py - qy, dz = pz - qz;
  return (dx * dx + dy * dy) + dz * dz;
}

// half the solid angle of the triangle seen from p (Van Oosterom-Strackee)
__device__ __forceinline__ float half_solid_angle(float px, float py, float pz, const FacePrep& t) {
  const float ax = t.a.x - px, ay = t.a.y - py, az = t.a.z - pz;
  const float bx = t.b.x - px, by = t.b.y - py, bz = t.b.z - pz;
  const float cx = t.c.x - px, cy = t.c.y - py, cz = t.c.z - pz;
  const float det = dot3(ax, ay, az, by * cz - bz * cy, bz * cx - bx * cz, bx * cy - by * cx);
  const float la = sqrtf(dot3(ax, ay, az, ax, ay, az)), lb = sqrtf(dot3(bx, by, bz, bx, by, bz)),
              lc = sqrtf(dot3(cx, cy, cz, cx, cy, cz));
  const float den = ((la * lb * lc + dot3(ax, ay, az, bx, by, bz) * lc) + dot3(bx, by, bz, cx, cy, cz) * la) +
                    dot3(cx, cy, cz, ax, ay, az) * lb;
  return atan2f(det, den);
}

template <int R>
__global__ __launch_bounds__(kThreads) void sdf_kernel(const FacePrep* __restrict__ prep, int64_t F,
                                                       const float* __restrict__ points, int64_t Q,
                                                       float* __restrict__ sdf, int32_t* __restrict__ face_idx,
                                                       float* __restrict__ winding) {
  __shared__ FacePrep tile[kTile];
  const int tid = threadIdx.x;
  const int64_t base = (int64_t)blockIdx.x * (kThreads * R);
  float px[R], py[R], pz[R], best[R];
  double wsum[R];
  int32_t bi[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int64_t i = base + (int64_t)r * kThreads + tid;
    const bool in = i < Q;
    px[r] = in ? points[3 * i] : 0.f;
    py[r] = in ? points[3 * i + 1] : 0.f;
    pz[r] = in ? points[3 * i + 2] : 0.f;
    best[r] = INFINITY;
    bi[r] = -1;
    wsum[r] = 0.0;
  }
  for (int64_t f0 = 0; f0 < F; f0 += kTile) {
    const bool in = f0 + tid < F;
    const float4* src = reinterpret_cast<const float4*>(prep + (in ? f0 + tid : 0));
    const float4 v0 = src[0], v1 = src[1], v2 = src[2], v3 = src[3], v4 = src[4];
    __syncthreads();                              // the previous tile is no longer read
    if (in) {
      tile[tid].a = v0;
      tile[tid].b = v1;
      tile[tid].c = v2;
      tile[tid].ab = v3;
      tile[tid].ac = v4;
    }
    __syncthreads();
    const int n = (int)min((int64_t)kTile, F - f0);
    for (int t = 0; t < n; ++t) {
      const FacePrep& tri = tile[t];              // same address in every lane: LDS broadcasts
      const float kind = tri.a.w;                 // uniform over the workgroup: no divergence
      if (kind == kKindSkip) continue;
      const int32_t f = (int32_t)(f0 + t);
      if (kind == kKindFlat) {
        const float bcx = tri.c.x - tri.b.x, bcy = tri.c.y - tri.b.y, bcz = tri.c.z - tri.b.z;
#pragma unroll
        for (int r = 0; r < R; ++r) {
          float d = seg_d2(px[r], py[r], pz[r], tri.a.x, tri.a.y, tri.a.z, tri.ab.x, tri.ab.y, tri.ab.z);
          d = fminf(d, seg_d2(px[r], py[r], pz[r], tri.a.x, tri.a.y, tri.a.z, tri.ac.x, tri.ac.y, tri.ac.z));
          d = fminf(d, seg_d2(px[r], py[r], pz[r], tri.b.x, tri.b.y, tri.b.z, bcx, bcy, bcz));
          if (d < best[r]) {                      // strict: ties keep the smaller face
            best[r] = d;
            bi[r] = f;
          }
        }
        continue;
      }
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const float d = tri_d2(px[r], py[r], pz[r], tri);
        if (d < best[r]) {
          best[r] = d;
          bi[r] = f;
        }
        wsum[r] += (double)half_solid_angle(px[r], py[r], pz[r], tri);
      }
    }
  }
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int64_t i = base + (int64_t)r * kThreads + tid;
    if (i < Q) {
      const double w = wsum[r] / (2.0 * M_PI);
      const float mag = sqrtf(best[r]);
      sdf[i] = w > 0.5 ? -mag : mag;
      face_idx[i] = bi[r];
      if (winding) winding[i] = (float)w;
    }
  }
}

// ---- boundary samples -------------------------------------------------------------------------------------------------
__host__ __device__ __forceinline__ uint64_t splitmix64(uint64_t x) {
  uint64_t z = x + 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

__device__ __forceinline__ double uniform01(uint64_t key, uint64_t counter) {
  return (double)(splitmix64(key ^ counter) >> 11) * 0x1.0p-53;
}

__global__ __launch_bounds__(kThreads) void boundary_kernel(const float* __restrict__ points, int64_t M, double sigma,
                                                            uint64_t key, float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= M) return;
  for (int k = 0; k < 3; ++k) {
    const float p = points[3 * i + k];
    if (sigma == 0.0) {
      out[3 * i + k] = p;
      continue;
    }
    const uint64_t c0 = (1ull << 63) + 6 * (uint64_t)i + 2 * (uint64_t)k;
    const double u1 = uniform01(key, c0), u2 = uniform01(key, c0 + 1);
    const double n = sqrt(-2.0 * log(1.0 - u1)) * cos(2.0 * M_PI * u2);
    out[3 * i + k] = (float)((double)p + sigma * n);
  }
}

// ---- farthest point sampling ------------------------------------------------------------------------------------------
constexpr int kFpsThreads = 1024;
constexpr int kFpsWaves = kFpsThreads / 64;
constexpr int kFpsRegPoints = 16;         // up to this many points per lane, their coordinates stay in registers too

// (m, j) beats (bm, bj): larger minimum, ties to the smaller index
__device__ __forceinline__ bool better(float m, int32_t j, float bm, int32_t bj) {
  return m > bm || (m == bm && j < bj);
}

template <int P>
__global__ __launch_bounds__(kFpsThreads) void fps_kernel(const float* __restrict__ clouds, int32_t N, int32_t K,
                                                          int32_t* __restrict__ idx) {
  __shared__ float s_m[2][kFpsWaves];
  __shared__ int32_t s_j[2][kFpsWaves];
  constexpr bool kRegs = P <= kFpsRegPoints;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* __restrict__ cloud = clouds + (int64_t)blockIdx.x * N * 3;
  int32_t* __restrict__ out = idx + (int64_t)blockIdx.x * K;
  float m[P];
  float x[kRegs ? P : 1], y[kRegs ? P : 1], z[kRegs ? P : 1];
#pragma unroll
  for (int p = 0; p < P; ++p) {
    const int32_t j = p * kFpsThreads + tid;
    m[p] = j < N ? INFINITY : -1.f;                // a slot without a point: never updated, never chosen (m_j >= 0)
    if constexpr (kRegs) {
      x[p] = j < N ? cloud[3 * j] : 0.f;
      y[p] = j < N ? cloud[3 * j + 1] : 0.f;
      z[p] = j < N ? cloud[3 * j + 2] : 0.f;
    }
  }
  int32_t sel = 0;
  if (tid == 0) out[0] = 0;
  for (int32_t s = 1; s < K; ++s) {
    const float sx = cloud[3 * sel], sy = cloud[3 * sel + 1], sz = cloud[3 * sel + 2];   // one address: broadcast
    float bm = -2.f;
    int32_t bj = 0;
    int t = tid;
    asm volatile("" : "+v"(t));                    // opaque per step: the P slot indices and addresses are not
                                                   // hoisted out of the step loop (P live registers each)
#pragma unroll
    for (int p = 0; p < P; ++p) {
      const int32_t j = p * kFpsThreads + t;
      float px, py, pz;
      if constexpr (kRegs) {
        px = x[p]; py = y[p]; pz = z[p];
      } else {
        const int32_t jc = 3 * min(j, N - 1);        // a slot without a point reads the last one (m stays -1)
        px = cloud[jc];
        py = cloud[jc + 1];
        pz = cloud[jc + 2];
      }
      const float dx = px - sx, dy = py - sy, dz = pz - sz;
      const float d2 = (dx * dx + dy * dy) + dz * dz;
      if (d2 < m[p]) m[p] = d2;                    // a NaN d2 leaves the minimum as it was
      if (better(m[p], j, bm, bj)) {
        bm = m[p];
        bj = j;
      }
    }
    for (int o = 32; o > 0; o >>= 1) {
      const float om = __shfl_xor(bm, o, 64);
      const int32_t oj = __shfl_xor(bj, o, 64);
      if (better(om, oj, bm, bj)) {
        bm = om;
        bj = oj;
      }
    }
    const int buf = s & 1;                         // double buffered: one barrier per step
    if (lane == 0) {
      s_m[buf][wave] = bm;
      s_j[buf][wave] = bj;
    }
    __syncthreads();
    bm = s_m[buf][0];
    bj = s_j[buf][0];
    for (int w = 1; w < kFpsWaves; ++w)
      if (better(s_m[buf][w], s_j[buf][w], bm, bj)) {
        bm = s_m[buf][w];
        bj = s_j[buf][w];
      }
    sel = bj;                                      // K <= N: some slot holds a point, so 0 <= bj < N
    if (tid == 0) out[s] = sel;
  }
}

}  // namespace

extern "C" {

const char* list_data_last_error(void) { return g_err; }

size_t list_data_signed_distance_workspace_bytes(int64_t n_faces) {
  if (n_faces <= 0 || n_faces > INT32_MAX) {
    fail(LIST_ERR_SHAPE, "%lld faces: need 1 <= F <= INT32_MAX", (long long)n_faces);
    return 0;
  }
  return (size_t)n_faces * sizeof(FacePrep);
}

int list_data_signed_distance(const float* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces,
                              const float* points, int64_t n_points, void* workspace, size_t workspace_bytes,
                              float* sdf, int32_t* face_idx, float* winding, void* stream) {
  if (n_faces <= 0 || n_faces > INT32_MAX)
    return fail(LIST_ERR_SHAPE, "%lld faces: need 1 <= F <= INT32_MAX", (long long)n_faces);
  if (n_verts <= 0 || n_verts > INT32_MAX)
    return fail(LIST_ERR_SHAPE, "%lld vertices: need 1 <= V <= INT32_MAX", (long long)n_verts);
  if (n_points < 0 || n_points > INT32_MAX)
    return fail(LIST_ERR_SHAPE, "%lld points: need 0 <= Q <= INT32_MAX", (long long)n_points);
  if (!verts || !faces || !workspace) return fail(LIST_ERR_ARG, "verts/faces/workspace is NULL");
  if (n_points && (!points || !sdf || !face_idx)) return fail(LIST_ERR_ARG, "points/sdf/face_idx is NULL");
  const size_t need = (size_t)n_faces * sizeof(FacePrep);
  if (workspace_bytes < need)
    return workspace_too_small(workspace_bytes, need, "list_data_signed_distance_workspace_bytes");
  if (n_points == 0) return LIST_OK;
  hipStream_t s = (hipStream_t)stream;
  FacePrep* prep = (FacePrep*)workspace;
  const dim3 block(kThreads);
  if (int rc = launch("face_prep_kernel", face_prep_kernel, dim3(blocks_for(n_faces, kThreads)), block, s, verts,
                      n_verts, faces, n_faces, prep))
    return rc;
  // the most points per lane that still gives >= 1024 workgroups (4 per CU); fewer when Q is small
  auto grid = [&](int R) { return blocks_for(n_points, kThreads * R); };
  auto run = [&](auto kernel, int R) {
    return launch("sdf_kernel", kernel, dim3(grid(R)), block, s, prep, n_faces, points, n_points, sdf, face_idx, winding);
  };
  if (grid(4) >= 1024) return run(sdf_kernel<4>, 4);
  if (grid(2) >= 1024) return run(sdf_kernel<2>, 2);
  return run(sdf_kernel<1>, 1);
}

int list_data_boundary_samples(const float* points, int64_t n_points, float sigma, uint64_t seed, float* out,
                               void* stream) {
  if (n_points < 0 || n_points > INT32_MAX)
    return fail(LIST_ERR_SHAPE, "%lld points: need 0 <= M <= INT32_MAX", (long long)n_points);
  if (n_points == 0) return LIST_OK;
  if (!points || !out) return fail(LIST_ERR_ARG, "points/out is NULL");
  return launch("boundary_kernel", boundary_kernel, dim3(blocks_for(n_points, kThreads)), dim3(kThreads),
                (hipStream_t)stream, points, n_points, (double)sigma, splitmix64(seed), out);
}

int list_data_farthest_points(const float* clouds, int64_t n_clouds, int64_t n_points, int64_t k, int32_t* idx,
                              void* stream) {
  if (n_points < 1 || n_points > LIST_DATA_MAX_FPS_POINTS)
    return fail(LIST_ERR_SHAPE, "N = %lld points per cloud: need 1 <= N <= %d", (long long)n_points,
                LIST_DATA_MAX_FPS_POINTS);
  if (k < 1 || k > n_points)
    return fail(LIST_ERR_SHAPE, "K = %lld samples of N = %lld points: need 1 <= K <= N", (long long)k,
                (long long)n_points);
  if (n_clouds < 0 || n_clouds > INT32_MAX)
    return fail(LIST_ERR_SHAPE, "B = %lld clouds: need 0 <= B <= INT32_MAX", (long long)n_clouds);
  if (n_clouds == 0) return LIST_OK;
  if (!clouds || !idx) return fail(LIST_ERR_ARG, "clouds/idx is NULL");
  hipStream_t s = (hipStream_t)stream;
  const int32_t N = (int32_t)n_points, K = (int32_t)k;
  const int64_t per_lane = cdiv(n_points, kFpsThreads);
  auto run = [&](auto kernel) {
    return launch("fps_kernel", kernel, dim3((unsigned)n_clouds), dim3(kFpsThreads), s, clouds, N, K, idx);
  };
  if (per_lane <= 1) return run(fps_kernel<1>);
  if (per_lane <= 2) return run(fps_kernel<2>);
  if (per_lane <= 4) return run(fps_kernel<4>);
  if (per_lane <= 8) return run(fps_kernel<8>);
  if (per_lane <= 16) return run(fps_kernel<16>);
  if (per_lane <= 32) return run(fps_kernel<32>);
  return run(fps_kernel<64>);
}

}  // extern "C"
