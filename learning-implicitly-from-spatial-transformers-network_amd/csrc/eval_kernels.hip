// Mesh evaluation on the device (include/list_eval.h): nearest neighbours, area-weighted surface sampling and the
// inside test of the reference's eval_mesh.
//
//   nn_kernel<R>           brute-force nearest neighbour: dst tiles staged in LDS, R src points per lane in registers.
//   face_area_kernel       per-face area (float64), then a hipCUB inclusive scan -> cdf.
//   sample_kernel          per sample: counter-based uniforms (splitmix64), binary search in the cdf, sqrt-rule point.
//   tri_kernel             per face: its corners widened to float64 and rotated.
//   bbox_partial_kernel    per block: min/max of the rotated corners;  bbox_final_kernel: scale, translate, refusal.
//   hash_key_kernel        per face: rescaled corners, clamped cell bbox, sort key (cell of its low corner).
//   hipCUB radix sort      (key, face) pairs: the CSR of the res^2 cells;  cell_offsets_kernel: first entry per cell.
//   contains_kernel        per point: parity of the hits over every triangle whose cell bbox covers its cell.
#include <math.h>

#include <hip/hip_runtime.h>

#include "list_cub.h"
#include "list_eval.h"
#include "list_host.h"

#pragma clang fp contract(off)

namespace {

__device__ __forceinline__ bool face_ok(const int32_t* __restrict__ faces, int64_t f, int64_t V, int32_t c[3]) {
  c[0] = faces[3 * f];
  c[1] = faces[3 * f + 1];
  c[2] = faces[3 * f + 2];
  return c[0] >= 0 && c[0] < V && c[1] >= 0 && c[1] < V && c[2] >= 0 && c[2] < V;
}

// ---- nearest neighbour ------------------------------------------------------------------------------------------------
constexpr int kNNThreads = 256;
constexpr int kNNTile = 256;          // dst points per LDS tile (one per thread to stage)

template <int R>
__global__ __launch_bounds__(kNNThreads) void nn_kernel(const float* __restrict__ src, int64_t N,
                                                        const float* __restrict__ dst, int64_t M,
                                                        float* __restrict__ dist, int32_t* __restrict__ idx) {
  __shared__ float4 tile[kNNTile];
  const int tid = threadIdx.x;
  const int64_t base = (int64_t)blockIdx.x * (kNNThreads * R);
  float px[R], py[R], pz[R], best[R];
  int32_t bi[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int64_t i = base + (int64_t)r * kNNThreads + tid;
    const bool in = i < N;
    px[r] = in ? src[3 * i] : 0.f;
    py[r] = in ? src[3 * i + 1] : 0.f;
    pz[r] = in ? src[3 * i + 2] : 0.f;
    best[r] = INFINITY;
    bi[r] = 0;
  }
  for (int64_t j0 = 0; j0 < M; j0 += kNNTile) {
    const int64_t j = j0 + tid;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (j < M) v = make_float4(dst[3 * j], dst[3 * j + 1], dst[3 * j + 2], 0.f);
    __syncthreads();                              // the previous tile is no longer read
    tile[tid] = v;
    __syncthreads();
    const int n = (int)min((int64_t)kNNTile, M - j0);
#pragma unroll 4
    for (int t = 0; t < n; ++t) {
      const float4 q = tile[t];                   // same address in every lane: an LDS broadcast
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const float dx = px[r] - q.x, dy = py[r] - q.y, dz = pz[r] - q.z;
        const float d2 = (dx * dx + dy * dy) + dz * dz;
        if (d2 < best[r]) {                       // strict: ties keep the smaller j
          best[r] = d2;
          bi[r] = (int32_t)(j0 + t);
        }
      }
    }
  }
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int64_t i = base + (int64_t)r * kNNThreads + tid;
    if (i < N) {
      dist[i] = sqrtf(best[r]);
      idx[i] = bi[r];
    }
  }
}

// ---- surface sampling -------------------------------------------------------------------------------------------------
constexpr int kThreads = 256;

__host__ __device__ __forceinline__ uint64_t splitmix64(uint64_t x) {
  uint64_t z = x + 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

__device__ __forceinline__ double uniform01(uint64_t key, uint64_t counter) {
  return (double)(splitmix64(key ^ counter) >> 11) * 0x1.0p-53;
}

__global__ __launch_bounds__(kThreads) void face_area_kernel(const float* __restrict__ verts, int64_t V,
                                                             const int32_t* __restrict__ faces, int64_t F,
                                                             double* __restrict__ area) {
  const int64_t f = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (f >= F) return;
  int32_t c[3];
  if (!face_ok(faces, f, V, c)) {
    area[f] = 0.0;
    return;
  }
  double p[3][3];
  for (int k = 0; k < 3; ++k)
    for (int a = 0; a < 3; ++a) p[k][a] = (double)verts[3 * (int64_t)c[k] + a];
  const double e1x = p[1][0] - p[0][0], e1y = p[1][1] - p[0][1], e1z = p[1][2] - p[0][2];
  const double e2x = p[2][0] - p[0][0], e2y = p[2][1] - p[0][1], e2z = p[2][2] - p[0][2];
  const double cx = e1y * e2z - e1z * e2y, cy = e1z * e2x - e1x * e2z, cz = e1x * e2y - e1y * e2x;
  area[f] = 0.5 * sqrt((cx * cx + cy * cy) + cz * cz);
}

__global__ __launch_bounds__(kThreads) void sample_kernel(const float* __restrict__ verts, int64_t V,
                                                          const int32_t* __restrict__ faces, int64_t F,
                                                          const double* __restrict__ cdf, int64_t n, uint64_t key,
                                                          float* __restrict__ points, int32_t* __restrict__ face_idx) {
  const int64_t s = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (s >= n) return;
  const double total = cdf[F - 1];
  if (!(total > 0.0 && isfinite(total))) {
    face_idx[s] = -1;
    points[3 * s] = points[3 * s + 1] = points[3 * s + 2] = NAN;
    return;
  }
  const uint64_t c0 = 3 * (uint64_t)s;
  const double target = uniform01(key, c0) * total;
  int64_t lo = 0, hi = F;                          // first f with cdf[f] > target
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (cdf[mid] > target) hi = mid; else lo = mid + 1;
  }
  if (lo == F) {                                   // target rounded up to the total: the last face of positive area
    lo = 0;
    hi = F;
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if (cdf[mid] >= total) hi = mid; else lo = mid + 1;
    }
  }
  const int64_t f = lo;
  int32_t c[3];
  face_ok(faces, f, V, c);                        // a chosen face has positive area, so its indices are valid
  const double r = sqrt(uniform01(key, c0 + 1)), u2 = uniform01(key, c0 + 2);
  const double a = 1.0 - r, b = r * (1.0 - u2), cc = r * u2;
  for (int ax = 0; ax < 3; ++ax) {
    const double x0 = verts[3 * (int64_t)c[0] + ax], x1 = verts[3 * (int64_t)c[1] + ax],
                 x2 = verts[3 * (int64_t)c[2] + ax];
    points[3 * s + ax] = (float)((a * x0 + b * x1) + cc * x2);
  }
  face_idx[s] = (int32_t)f;
}

// ---- inside test ------------------------------------------------------------------------------------------------------
constexpr int kRedBlocks = kThreads;                 // bbox_final_kernel: one thread per partial
constexpr int kMaxNarrow = 8;                      // a triangle whose cell bbox spans more cells than this on an axis
                                                   // is "wide": every query scans the wide list
struct ContainsParams {
  double scale[3], translate[3];
  int32_t refused;
  int32_t kx, ky;                                  // widest narrow triangle, in cells
};

__device__ __forceinline__ void rotate(const double* __restrict__ R, double x, double y, double z, double o[3]) {
  if (R) {
    o[0] = (R[0] * x + R[1] * y) + R[2] * z;
    o[1] = (R[3] * x + R[4] * y) + R[5] * z;
    o[2] = (R[6] * x + R[7] * y) + R[8] * z;
  } else {
    o[0] = x;
    o[1] = y;
    o[2] = z;
  }
}

// <int> truncation of a coordinate, clamped to [0, res-1] (NaN -> 0), as triangle_hash.pyx does after its cast
__device__ __forceinline__ int cell_clamp(double x, int res) {
  if (!(x >= 1.0)) return 0;
  if (x >= (double)(res - 1)) return res - 1;
  return (int)x;
}

__global__ __launch_bounds__(kThreads) void tri_kernel(const float* __restrict__ verts, int64_t V,
                                                       const int32_t* __restrict__ faces, int64_t F,
                                                       const double* __restrict__ rot, double* __restrict__ tri) {
  const int64_t f = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (f >= F) return;
  int32_t c[3];
  if (!face_ok(faces, f, V, c)) return;
  for (int k = 0; k < 3; ++k) {
    const float* v = verts + 3 * (int64_t)c[k];
    rotate(rot, (double)v[0], (double)v[1], (double)v[2], tri + 9 * f + 3 * k);
  }
}

// min (rows 0-2) and max (rows 3-5) over the block's threads into s[.][0]; NaN propagates, as numpy's min/max do
__device__ __forceinline__ void block_minmax(const double lo[3], const double hi[3], double (*s)[kThreads]) {
  for (int a = 0; a < 3; ++a) {
    s[a][threadIdx.x] = lo[a];
    s[3 + a][threadIdx.x] = hi[a];
  }
  __syncthreads();
  for (int w = kThreads / 2; w > 0; w >>= 1) {
    if (threadIdx.x < w)
      for (int a = 0; a < 3; ++a) {
        const double l = s[a][threadIdx.x + w], h = s[3 + a][threadIdx.x + w];
        if (l < s[a][threadIdx.x] || l != l) s[a][threadIdx.x] = l;
        if (h > s[3 + a][threadIdx.x] || h != h) s[3 + a][threadIdx.x] = h;
      }
    __syncthreads();
  }
}

__global__ __launch_bounds__(kThreads) void bbox_partial_kernel(const int32_t* __restrict__ faces, int64_t V,
                                                                int64_t F, const double* __restrict__ tri,
                                                                double* __restrict__ partial) {
  __shared__ double s[6][kThreads];
  double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (int64_t f = (int64_t)blockIdx.x * kThreads + threadIdx.x; f < F; f += (int64_t)gridDim.x * kThreads) {
    int32_t c[3];
    if (!face_ok(faces, f, V, c)) continue;
    for (int k = 0; k < 3; ++k)
      for (int a = 0; a < 3; ++a) {
        const double x = tri[9 * f + 3 * k + a];
        lo[a] = x < lo[a] || x != x ? x : lo[a];     // NaN propagates, as numpy's min/max do
        hi[a] = x > hi[a] || x != x ? x : hi[a];
      }
  }
  block_minmax(lo, hi, s);
  if (threadIdx.x < 6) partial[6 * blockIdx.x + threadIdx.x] = s[threadIdx.x][0];
}

// one thread per partial (nblocks <= kRedBlocks == kThreads), reduced like the partials
__global__ __launch_bounds__(kThreads) void bbox_final_kernel(const double* __restrict__ partial, int nblocks, int res,
                                                              ContainsParams* __restrict__ P) {
  __shared__ double s[6][kThreads];
  double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  if ((int)threadIdx.x < nblocks)
    for (int a = 0; a < 3; ++a) {
      lo[a] = partial[6 * threadIdx.x + a];
      hi[a] = partial[6 * threadIdx.x + 3 + a];
    }
  block_minmax(lo, hi, s);
  if (threadIdx.x != 0) return;
  for (int a = 0; a < 3; ++a) {
    lo[a] = s[a][0];
    hi[a] = s[3 + a][0];
  }
  int refused = 0;
  for (int a = 0; a < 3; ++a) {
    const double ext = hi[a] - lo[a];
    if (!(ext > 0.0) || !isfinite(ext)) refused = 1;   // zero extent (or no valid triangle): the reference divides by 0
    P->scale[a] = (double)(res - 1) / ext;
    P->translate[a] = 0.5 - P->scale[a] * lo[a];
  }
  P->refused = refused;
  P->kx = 0;
  P->ky = 0;
}

// box: x0 | x1 << 16 | y0 << 32 | y1 << 48 (clamped cells); key: x0 * res + y0, res^2 for a wide triangle, res^2 + 1 for
// a face that is never tested
__global__ __launch_bounds__(kThreads) void hash_key_kernel(const int32_t* __restrict__ faces, int64_t V, int64_t F,
                                                            int res, double* __restrict__ tri,
                                                            ContainsParams* __restrict__ P,
                                                            uint64_t* __restrict__ box, uint32_t* __restrict__ keys,
                                                            uint32_t* __restrict__ vals) {
  const int64_t f = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  const uint32_t cells = (uint32_t)res * (uint32_t)res;
  int wx = -1, wy = -1;                           // widths of a narrow triangle, -1 otherwise
  int32_t c[3];
  if (f < F) {
    vals[f] = (uint32_t)f;
    if (P->refused || !face_ok(faces, f, V, c)) {
      keys[f] = cells + 1;
      box[f] = 1;                                 // x0 = 1 > x1 = 0: covers nothing
    } else {
      // the parameters into registers first: the stores to tri could alias P, which would serialise every reload
      const double sc[3] = {P->scale[0], P->scale[1], P->scale[2]};
      const double tr[3] = {P->translate[0], P->translate[1], P->translate[2]};
      double* t = tri + 9 * f;
      for (int k = 0; k < 3; ++k)
        for (int a = 0; a < 3; ++a) t[3 * k + a] = sc[a] * t[3 * k + a] + tr[a];
      const int x0 = cell_clamp(fmin(fmin(t[0], t[3]), t[6]), res), x1 = cell_clamp(fmax(fmax(t[0], t[3]), t[6]), res);
      const int y0 = cell_clamp(fmin(fmin(t[1], t[4]), t[7]), res), y1 = cell_clamp(fmax(fmax(t[1], t[4]), t[7]), res);
      box[f] = (uint64_t)x0 | (uint64_t)x1 << 16 | (uint64_t)y0 << 32 | (uint64_t)y1 << 48;
      const bool wide = x1 - x0 > kMaxNarrow || y1 - y0 > kMaxNarrow;
      keys[f] = wide ? cells : (uint32_t)x0 * (uint32_t)res + (uint32_t)y0;
      if (!wide) {
        wx = x1 - x0;
        wy = y1 - y0;
      }
    }
  }
  // widest narrow triangle: reduced over the wave first, then one atomicMax per wave (max is order-independent)
  for (int o = 32; o > 0; o >>= 1) {
    wx = max(wx, __shfl_xor(wx, o, 64));
    wy = max(wy, __shfl_xor(wy, o, 64));
  }
  if ((threadIdx.x & 63) == 0 && wx >= 0) {
    atomicMax(&P->kx, wx);
    atomicMax(&P->ky, wy);
  }
}

// offsets[c] = first sorted entry with key >= c, c in [0, res^2 + 2]
__global__ __launch_bounds__(kThreads) void cell_offsets_kernel(const uint32_t* __restrict__ keys, int64_t F,
                                                                int64_t n_off, uint32_t* __restrict__ offsets) {
  const int64_t c = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (c >= n_off) return;
  int64_t lo = 0, hi = F;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if ((int64_t)keys[mid] >= c) hi = mid; else lo = mid + 1;
  }
  offsets[c] = (uint32_t)lo;
}

__device__ __forceinline__ double sgn(double x) { return x > 0.0 ? 1.0 : (x < 0.0 ? -1.0 : x); }

// one (point, triangle) pair: check_triangles, then the depth test -> 1 (a hit of parity 0), 2 (parity 1) or 0
__device__ __forceinline__ int hit(const double* __restrict__ t, double px, double py, double pz) {
  const double a00 = t[0] - t[6], a01 = t[3] - t[6], a10 = t[1] - t[7], a11 = t[4] - t[7];
  const double y0 = px - t[6], y1 = py - t[7];
  const double det = a00 * a11 - a01 * a10;
  if (!(fabs(det) != 0.0)) return 0;
  const double s = sgn(det), ad = fabs(det);
  const double u = (a11 * y0 - a01 * y1) * s;
  const double v = (-a10 * y0 + a00 * y1) * s;
  const double uv = u + v;
  if (!(0.0 < u && u < ad && 0.0 < v && v < ad && 0.0 < uv && uv < ad)) return 0;
  const double v1x = t[6] - t[0], v1y = t[7] - t[1], v1z = t[8] - t[2];
  const double v2x = t[3] - t[0], v2y = t[4] - t[1], v2z = t[5] - t[2];
  const double n0 = v1y * v2z - v1z * v2y, n1 = v1z * v2x - v1x * v2z, n2 = v1x * v2y - v1y * v2x;
  const double alpha = n0 * (t[0] - px) + n1 * (t[1] - py);
  const double an = fabs(n2);
  if (!(an != 0.0)) return 0;
  const double depth = t[2] * an + alpha * sgn(n2);
  const double zc = pz * an;
  return depth >= zc ? 1 : (depth < zc ? 2 : 0);
}

// the triangles sorted_faces[lo, hi) whose cell bbox covers (cx, cy): hits of parity 0 in bit 0, of parity 1 in bit 1
__device__ __forceinline__ int scan_range(uint32_t lo, uint32_t hi, int cx, int cy, double px, double py, double pz,
                                           const double* __restrict__ tri, const uint64_t* __restrict__ box,
                                           const uint32_t* __restrict__ sorted_faces) {
  int parity = 0;
  for (uint32_t k = lo; k < hi; ++k) {
    const uint32_t f = sorted_faces[k];
    const uint64_t b = box[f];
    const int x0 = (int)(b & 0xffff), x1 = (int)((b >> 16) & 0xffff), y0 = (int)((b >> 32) & 0xffff),
              y1 = (int)(b >> 48);
    if (x0 <= cx && cx <= x1 && y0 <= cy && cy <= y1) parity ^= hit(tri + 9 * (int64_t)f, px, py, pz);
  }
  return parity;
}

__global__ __launch_bounds__(kThreads) void contains_kernel(const double* __restrict__ points, int64_t Q,
                                                            const double* __restrict__ rot, int res,
                                                            const ContainsParams* __restrict__ P,
                                                            const double* __restrict__ tri,
                                                            const uint64_t* __restrict__ box,
                                                            const uint32_t* __restrict__ sorted_faces,
                                                            const uint32_t* __restrict__ offsets,
                                                            uint8_t* __restrict__ flags) {
  const int64_t q = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (q >= Q) return;
  if (P->refused) {
    flags[q] = LIST_EVAL_REFUSED;
    return;
  }
  double p[3];
  rotate(rot, points[3 * q], points[3 * q + 1], points[3 * q + 2], p);
  const double px = P->scale[0] * p[0] + P->translate[0], py = P->scale[1] * p[1] + P->translate[1],
               pz = P->scale[2] * p[2] + P->translate[2];
  const double r = (double)res;
  if (!(0.0 <= px && px <= r && 0.0 <= py && py <= r && 0.0 <= pz && pz <= r)) {
    flags[q] = 0;
    return;
  }
  const int cx = (int)px, cy = (int)py;
  int parity = 0;
  if (cx < res && cy < res) {
    const int kx = P->kx, ky = P->ky;
    const int ylo = max(cy - ky, 0);
    for (int x0 = cx; x0 >= 0 && x0 >= cx - kx; --x0) {   // narrow triangles: low corner within (kx, ky) cells
      const uint32_t row = (uint32_t)x0 * (uint32_t)res;
      parity ^= scan_range(offsets[row + ylo], offsets[row + cy + 1], cx, cy, px, py, pz, tri, box, sorted_faces);
    }
    const uint32_t cells = (uint32_t)res * (uint32_t)res;
    parity ^= scan_range(offsets[cells], offsets[cells + 1], cx, cy, px, py, pz, tri, box, sorted_faces);   // wide
  }
  const bool in0 = parity & 1, in1 = (parity >> 1) & 1;
  flags[q] = (uint8_t)((in0 && in1 ? LIST_EVAL_INSIDE : 0) | (in0 != in1 ? LIST_EVAL_HOLE : 0));
}

// ---- workspaces -------------------------------------------------------------------------------------------------------
struct SampleLayout {
  size_t area, cdf, scratch, scratch_bytes, total;
};

// each layout: true, or false with the refusal's message set
bool sample_layout(int64_t F, SampleLayout* L) {
  if (!inclusive_sum_scratch<double>(F, &L->scratch_bytes)) return false;
  Carver c;
  L->area = c.take(F * sizeof(double));
  L->cdf = c.take(F * sizeof(double));
  L->scratch = c.take(L->scratch_bytes);
  L->total = c.total();
  return true;
}

struct ContainsLayout {
  size_t params, partial, tri, box, keys_in, keys_out, vals_in, vals_out, offsets, scratch, scratch_bytes, total;
  int64_t n_off;
  int key_bits;
};

bool contains_layout(int64_t F, int32_t res, ContainsLayout* L) {
  L->n_off = (int64_t)res * res + 3;
  int bits = 1;
  while (((int64_t)1 << bits) <= (int64_t)res * res + 1) ++bits;
  L->key_bits = bits;
  if (!sort_pairs_scratch<uint32_t, uint32_t>(F, bits, &L->scratch_bytes)) return false;
  Carver c;
  L->params = c.take(sizeof(ContainsParams));
  L->partial = c.take(kRedBlocks * 6 * sizeof(double));
  L->tri = c.take(F * 9 * sizeof(double));
  L->box = c.take(F * sizeof(uint64_t));
  L->keys_in = c.take(F * sizeof(uint32_t));
  L->keys_out = c.take(F * sizeof(uint32_t));
  L->vals_in = c.take(F * sizeof(uint32_t));
  L->vals_out = c.take(F * sizeof(uint32_t));
  L->offsets = c.take(L->n_off * sizeof(uint32_t));
  L->scratch = c.take(L->scratch_bytes);
  L->total = c.total();
  return true;
}

// LIST_OK, or a refusal with its message
int check_n_faces(int64_t F) {
  if (F <= 0 || F > INT32_MAX) return fail(LIST_ERR_SHAPE, "%lld faces: need 1 <= F <= INT32_MAX", (long long)F);
  return LIST_OK;
}

int check_hash_res(int32_t res) {
  if (res < 1 || res > LIST_EVAL_MAX_HASH_RES)
    return fail(LIST_ERR_SHAPE, "hash_res %d: need 1 <= res <= %d", res, LIST_EVAL_MAX_HASH_RES);
  return LIST_OK;
}

int check_faces(int64_t V, int64_t F) {
  if (int rc = check_n_faces(F)) return rc;
  if (V <= 0 || V > INT32_MAX) return fail(LIST_ERR_SHAPE, "%lld vertices: need 1 <= V <= INT32_MAX", (long long)V);
  return LIST_OK;
}

}  // namespace

extern "C" {

const char* list_eval_last_error(void) { return g_err; }

int list_eval_nn(const float* src, int64_t n_src, const float* dst, int64_t n_dst, float* dist, int32_t* idx,
                 void* stream) {
  if (n_dst <= 0 || n_dst > INT32_MAX) return fail(LIST_ERR_SHAPE, "M = %lld dst points: need 1 <= M <= INT32_MAX",
                                                   (long long)n_dst);
  if (n_src < 0 || n_src > INT32_MAX) return fail(LIST_ERR_SHAPE, "N = %lld src points: need 0 <= N <= INT32_MAX",
                                                  (long long)n_src);
  if (n_src == 0) return LIST_OK;
  if (!src || !dst || !dist || !idx) return fail(LIST_ERR_ARG, "src/dst/dist/idx is NULL");
  hipStream_t s = (hipStream_t)stream;
  // the most src points per lane that still gives >= 1024 workgroups (4 per CU); fewer when N is small
  auto grid = [&](int R) { return blocks_for(n_src, kNNThreads * R); };
  const dim3 block(kNNThreads);
  if (grid(4) >= 1024) return launch("nn_kernel", nn_kernel<4>, dim3(grid(4)), block, s, src, n_src, dst, n_dst, dist, idx);
  if (grid(2) >= 1024) return launch("nn_kernel", nn_kernel<2>, dim3(grid(2)), block, s, src, n_src, dst, n_dst, dist, idx);
  return launch("nn_kernel", nn_kernel<1>, dim3(grid(1)), block, s, src, n_src, dst, n_dst, dist, idx);
}

size_t list_eval_sample_workspace_bytes(int64_t n_faces) {
  SampleLayout L;
  return check_n_faces(n_faces) == LIST_OK && sample_layout(n_faces, &L) ? L.total : 0;
}

int list_eval_sample(const float* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces, int64_t n_samples,
                     uint64_t seed, void* workspace, size_t workspace_bytes, float* points, int32_t* face_idx,
                     void* stream) {
  if (int rc = check_faces(n_verts, n_faces)) return rc;
  if (n_samples < 0 || n_samples > INT32_MAX) return fail(LIST_ERR_SHAPE, "n = %lld samples", (long long)n_samples);
  if (!verts || !faces || !workspace) return fail(LIST_ERR_ARG, "verts/faces/workspace is NULL");
  if (n_samples && (!points || !face_idx)) return fail(LIST_ERR_ARG, "points/face_idx is NULL");
  SampleLayout L;
  if (!sample_layout(n_faces, &L)) return LIST_ERR_HIP;
  if (workspace_bytes < L.total)
    return workspace_too_small(workspace_bytes, L.total, "list_eval_sample_workspace_bytes");
  if (n_samples == 0) return LIST_OK;
  hipStream_t s = (hipStream_t)stream;
  const dim3 block(kThreads);
  double* area = at<double>(workspace, L.area);
  double* cdf = at<double>(workspace, L.cdf);
  if (int rc = launch("face_area_kernel", face_area_kernel, dim3(blocks_for(n_faces, kThreads)), block, s, verts,
                      n_verts, faces, n_faces, area))
    return rc;
  if (int rc = inclusive_sum(at<char>(workspace, L.scratch), L.scratch_bytes, area, cdf, n_faces, s)) return rc;
  return launch("sample_kernel", sample_kernel, dim3(blocks_for(n_samples, kThreads)), block, s, verts, n_verts, faces,
                n_faces, cdf, n_samples, splitmix64(seed), points, face_idx);
}

size_t list_eval_contains_workspace_bytes(int64_t n_faces, int32_t hash_res) {
  if (check_n_faces(n_faces) != LIST_OK || check_hash_res(hash_res) != LIST_OK) return 0;
  ContainsLayout L;
  return contains_layout(n_faces, hash_res, &L) ? L.total : 0;
}

int list_eval_contains(const float* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces,
                       const double* points, int64_t n_points, const double* rot, int32_t hash_res, void* workspace,
                       size_t workspace_bytes, uint8_t* flags, void* stream) {
  if (int rc = check_faces(n_verts, n_faces)) return rc;
  if (int rc = check_hash_res(hash_res)) return rc;
  if (n_points < 0 || n_points > INT32_MAX) return fail(LIST_ERR_SHAPE, "%lld points", (long long)n_points);
  if (!verts || !faces || !workspace) return fail(LIST_ERR_ARG, "verts/faces/workspace is NULL");
  if (n_points && (!points || !flags)) return fail(LIST_ERR_ARG, "points/flags is NULL");
  ContainsLayout L;
  if (!contains_layout(n_faces, hash_res, &L)) return LIST_ERR_HIP;
  if (workspace_bytes < L.total)
    return workspace_too_small(workspace_bytes, L.total, "list_eval_contains_workspace_bytes");
  if (n_points == 0) return LIST_OK;
  hipStream_t s = (hipStream_t)stream;
  ContainsParams* P = at<ContainsParams>(workspace, L.params);
  double* partial = at<double>(workspace, L.partial);
  double* tri = at<double>(workspace, L.tri);
  uint64_t* box = at<uint64_t>(workspace, L.box);
  uint32_t* keys_in = at<uint32_t>(workspace, L.keys_in);
  uint32_t* keys_out = at<uint32_t>(workspace, L.keys_out);
  uint32_t* vals_in = at<uint32_t>(workspace, L.vals_in);
  uint32_t* vals_out = at<uint32_t>(workspace, L.vals_out);
  uint32_t* offsets = at<uint32_t>(workspace, L.offsets);
  const int64_t F = n_faces;
  const dim3 per_face(blocks_for(F, kThreads)), block(kThreads);
  if (int rc = launch("tri_kernel", tri_kernel, per_face, block, s, verts, n_verts, faces, F, rot, tri)) return rc;
  const int nred = (int)blocks_capped(F, kThreads, kRedBlocks);
  if (int rc = launch("bbox_partial_kernel", bbox_partial_kernel, dim3(nred), block, s, faces, n_verts, F, tri, partial))
    return rc;
  if (int rc = launch("bbox_final_kernel", bbox_final_kernel, dim3(1), block, s, partial, nred, (int)hash_res, P))
    return rc;
  if (int rc = launch("hash_key_kernel", hash_key_kernel, per_face, block, s, faces, n_verts, F, (int)hash_res, tri, P,
                      box, keys_in, vals_in))
    return rc;
  if (int rc = sort_pairs(at<char>(workspace, L.scratch), L.scratch_bytes, keys_in, keys_out, vals_in, vals_out, F,
                          L.key_bits, s))
    return rc;
  if (int rc = launch("cell_offsets_kernel", cell_offsets_kernel, dim3(blocks_for(L.n_off, kThreads)), block, s,
                      keys_out, F, L.n_off, offsets))
    return rc;
  return launch("contains_kernel", contains_kernel, dim3(blocks_for(n_points, kThreads)), block, s, points, n_points,
                rot, (int)hash_res, P, tri, box, vals_out, offsets, flags);
}

}  // extern "C"
