// The Chamfer loss of stage 1 and its gradient on the device (include/list_loss.h).
//
//   nn_sq_kernel        brute-force nearest neighbour in both directions and every batch in one launch: a workgroup
//                       takes 512 source points (two per lane, packed fp32 arithmetic) against one chunk of 1024
//                       targets staged in LDS tiles, and folds its minima into the 64-bit (d2 bits << 32 | index)
//                       words of the workspace with atomicMin (exact, independent of arrival order).
//   loss_partial_kernel one workgroup per (direction, batch): unpacks the words into d2 / idx (NaN for a source with a
//                       NaN coordinate) and sums d2 in float64 in the fixed order of the header.
//   loss_final_kernel   one lane: the sum over the batch and the two directions.
//   csr_hist_kernel     backward: sources per target, integer counters with wave-grouped atomics (a target that is
//                       the nearest point of thousands of sources costs one atomic per wave, not one per lane).
//   csr_place_kernel    one workgroup per (side, batch): exclusive scan of the counters, then a stable placement of
//                       the sources in source-index order (1024 at a time, bitonic sort of (key, source) in LDS).
//   grad_kernel         one lane per point: direct term plus the sum over its CSR segment (a segment of more than 32
//                       sources is summed by the whole wave).
#include <limits.h>
#include <math.h>

#include <hip/hip_runtime.h>

#include "list_host.h"
#include "list_loss.h"

#pragma clang fp contract(off)

namespace {

typedef float float2v __attribute__((ext_vector_type(2)));

// ---- forward ----------------------------------------------------------------------------------------------------------
constexpr int kFwdThreads = 256;
constexpr int kTile = 256;                       // targets per LDS tile (one per thread to stage)
constexpr int kChunk = 4 * kTile;                // targets per workgroup
constexpr int kSrc = 2 * kFwdThreads;            // sources per workgroup: two per lane, one packed pair

struct FwdGrid {
  int64_t B, N, M;
  int64_t sx, tx;                                // x -> y: source chunks of N, target chunks of M
  int64_t sy, ty;                                // y -> x
};

__device__ __forceinline__ bool has_nan(const float* p) { return isnan(p[0]) || isnan(p[1]) || isnan(p[2]); }

__global__ __launch_bounds__(kFwdThreads) void nn_sq_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                            FwdGrid g, unsigned long long* __restrict__ packed) {
  __shared__ float4 tile[kTile];
  const int tid = threadIdx.x;
  int64_t blk = blockIdx.x;
  const int64_t per_b_x = g.sx * g.tx;
  const bool dir_x = blk < g.B * per_b_x;          // uniform over the workgroup
  if (!dir_x) blk -= g.B * per_b_x;
  const int64_t per_b = dir_x ? per_b_x : g.sy * g.ty, tchunks = dir_x ? g.tx : g.ty;
  const int64_t b = blk / per_b, rem = blk % per_b;
  const int64_t s0 = (rem / tchunks) * kSrc, t0 = (rem % tchunks) * kChunk;
  const int64_t S = dir_x ? g.N : g.M, T = dir_x ? g.M : g.N;
  const float* __restrict__ src = (dir_x ? x : y) + 3 * b * S;
  const float* __restrict__ dst = (dir_x ? y : x) + 3 * b * T;
  unsigned long long* __restrict__ out = packed + (dir_x ? b * g.N : g.B * g.N + b * g.M);

  const int64_t i0 = s0 + tid, i1 = s0 + kFwdThreads + tid;
  float2v px, py, pz;
  px.x = i0 < S ? src[3 * i0] : 0.f;
  py.x = i0 < S ? src[3 * i0 + 1] : 0.f;
  pz.x = i0 < S ? src[3 * i0 + 2] : 0.f;
  px.y = i1 < S ? src[3 * i1] : 0.f;
  py.y = i1 < S ? src[3 * i1 + 1] : 0.f;
  pz.y = i1 < S ? src[3 * i1 + 2] : 0.f;
  float best0 = INFINITY, best1 = INFINITY;
  int32_t bi0 = (int32_t)t0, bi1 = (int32_t)t0;
  const int64_t t_end = min(t0 + (int64_t)kChunk, T);
  for (int64_t j0 = t0; j0 < t_end; j0 += kTile) {
    const int64_t j = j0 + tid;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (j < T) v = make_float4(dst[3 * j], dst[3 * j + 1], dst[3 * j + 2], 0.f);
    __syncthreads();                              // the previous tile is no longer read
    tile[tid] = v;
    __syncthreads();
    const int n = (int)min((int64_t)kTile, t_end - j0);
#pragma unroll 4
    for (int t = 0; t < n; ++t) {
      const float4 q = tile[t];                   // same address in every lane: an LDS broadcast
      // v_pk_add_f32 / v_pk_mul_f32: the same IEEE operations as the scalar forms, two sources per instruction
      const float2v dx = px - q.x, dy = py - q.y, dz = pz - q.z;
      const float2v d2 = (dx * dx + dy * dy) + dz * dz;
      const int32_t jj = (int32_t)(j0 + t);
      if (d2.x < best0) { best0 = d2.x; bi0 = jj; }   // strict: ties keep the smaller j; NaN never wins
      if (d2.y < best1) { best1 = d2.y; bi1 = jj; }
    }
  }
  if (i0 < S)
    atomicMin(&out[i0], ((unsigned long long)__float_as_uint(best0) << 32) | (uint32_t)bi0);
  if (i1 < S)
    atomicMin(&out[i1], ((unsigned long long)__float_as_uint(best1) << 32) | (uint32_t)bi1);
}

constexpr int kRedThreads = 256;

// one workgroup per (direction, batch): blockIdx.x < B is x -> y
__global__ __launch_bounds__(kRedThreads) void loss_partial_kernel(const float* __restrict__ x,
                                                                   const float* __restrict__ y, int64_t B, int64_t N,
                                                                   int64_t M,
                                                                   const unsigned long long* __restrict__ packed,
                                                                   float* __restrict__ d2_xy, int32_t* __restrict__ idx_xy,
                                                                   float* __restrict__ d2_yx, int32_t* __restrict__ idx_yx,
                                                                   double* __restrict__ partial) {
  __shared__ double p[kRedThreads];
  const bool dir_x = (int64_t)blockIdx.x < B;
  const int64_t b = dir_x ? blockIdx.x : blockIdx.x - B;
  const int64_t S = dir_x ? N : M;
  const float* __restrict__ src = (dir_x ? x : y) + 3 * b * S;
  const unsigned long long* __restrict__ w = packed + (dir_x ? b * N : B * N + b * M);
  float* __restrict__ d2 = (dir_x ? d2_xy : d2_yx) + b * S;
  int32_t* __restrict__ idx = (dir_x ? idx_xy : idx_yx) + b * S;
  double acc = 0.0;
  for (int64_t i = threadIdx.x; i < S; i += kRedThreads) {
    const unsigned long long v = w[i];
    const float d = has_nan(src + 3 * i) ? NAN : __uint_as_float((uint32_t)(v >> 32));
    d2[i] = d;
    idx[i] = (int32_t)(uint32_t)v;
    acc += (double)d;
  }
  p[threadIdx.x] = acc;
  __syncthreads();
  for (int w2 = kRedThreads / 2; w2 > 0; w2 >>= 1) {
    if ((int)threadIdx.x < w2) p[threadIdx.x] += p[threadIdx.x + w2];
    __syncthreads();
  }
  if (threadIdx.x == 0) partial[blockIdx.x] = p[0];
}

__global__ void loss_final_kernel(const double* __restrict__ partial, int64_t B, int64_t N, int64_t M,
                                  float* __restrict__ loss) {
  double lx = 0.0, ly = 0.0;
  for (int64_t b = 0; b < B; ++b) lx += partial[b] / (double)N;
  for (int64_t b = 0; b < B; ++b) ly += partial[B + b] / (double)M;
  *loss = (float)(lx / (double)B + ly / (double)B);
}

// ---- backward ---------------------------------------------------------------------------------------------------------
// Side X: targets are the x points, sources the y points with keys idx_yx (needed for grad_x).
// Side Y: targets are the y points, sources the x points with keys idx_xy (needed for grad_y).
struct CsrSide {
  const int32_t* key;          // [B][S] nearest target of each source
  int32_t* count;              // [B][T] sources per target
  int32_t* end;                // [B][T] scan, then cursor: after placement the end of each segment
  int32_t* order;              // [B][S] source indices grouped by target, source-index order inside a segment
  int64_t S, T;
};

struct CsrArgs {
  CsrSide side[2];
  int64_t B;
  int64_t hist_blocks[2];      // csr_hist_kernel: workgroups of side 0, then of side 1 (0 = side skipped)
  int nsides;                  // csr_place_kernel: the sides present, in side[0..nsides)
};

constexpr int kHistThreads = 256;

// (gather_kernels.hip:wave_grouped_add without the position) the lanes of a wave that hold the same key add their
// count with one atomic.  All 64 lanes must be live; `active` = false lanes match nobody and add nothing.
__device__ __forceinline__ void wave_grouped_count(int32_t* __restrict__ bins, int key, bool active) {
  const int lane = threadIdx.x & 63;
  const int k = active ? key : (-1 - lane);
  unsigned lo = 0, hi = 0;
#pragma unroll
  for (int l = 0; l < 64; ++l) {
    const int kl = __builtin_amdgcn_readlane(k, l);
    if (l < 32) lo |= (kl == k) ? (1u << l) : 0u;
    else hi |= (kl == k) ? (1u << (l - 32)) : 0u;
  }
  const unsigned below_lo = lane < 32 ? lo & ((1u << lane) - 1u) : lo;
  const unsigned below_hi = lane < 32 ? 0u : hi & ((1u << (lane - 32)) - 1u);
  if (active && below_lo == 0 && below_hi == 0) atomicAdd(&bins[key], __builtin_popcount(lo) + __builtin_popcount(hi));
}

__global__ __launch_bounds__(kHistThreads) void csr_hist_kernel(CsrArgs a) {
  int64_t blk = blockIdx.x;
  const int s = blk < a.hist_blocks[0] ? 0 : 1;
  if (s) blk -= a.hist_blocks[0];
  const CsrSide c = a.side[s];
  const int64_t n = a.B * c.S;
  const int64_t i = blk * kHistThreads + threadIdx.x;
  const bool in = i < n;
  int32_t key = in ? c.key[i] : -1;
  const int64_t b = in ? i / c.S : 0;
  const bool active = in && key >= 0 && key < c.T;     // an index outside [0, T) contributes nothing
  // one bin per (batch, target): the flat bin index keeps keys of different batches apart
  wave_grouped_count(c.count, active ? (int)(b * c.T + key) : 0, active);
}

constexpr int kPlaceThreads = 1024;

// inclusive scan (sum, or max with MAX) of one int per thread over the workgroup; *total = the last thread's result
template <bool MAX>
__device__ __forceinline__ int block_scan(int v, int* __restrict__ buf, int* total) {
  const int tid = threadIdx.x;
  buf[tid] = v;
  __syncthreads();
  for (int off = 1; off < kPlaceThreads; off <<= 1) {
    const int u = tid >= off ? buf[tid - off] : (MAX ? INT_MIN : 0);
    __syncthreads();
    buf[tid] = MAX ? max(buf[tid], u) : buf[tid] + u;
    __syncthreads();
  }
  const int r = buf[tid];
  *total = buf[kPlaceThreads - 1];
  __syncthreads();                               // buf is free again when this returns
  return r;
}

// one workgroup per (side, batch)
__global__ __launch_bounds__(kPlaceThreads) void csr_place_kernel(CsrArgs a) {
  __shared__ unsigned long long sk[kPlaceThreads];
  __shared__ int buf[kPlaceThreads];
  const int tid = threadIdx.x;
  const CsrSide c = a.side[blockIdx.x / a.B];
  const int64_t b = blockIdx.x % a.B;
  const int32_t* __restrict__ count = c.count + b * c.T;
  int32_t* __restrict__ cur = c.end + b * c.T;
  const int32_t* __restrict__ key = c.key + b * c.S;
  int32_t* __restrict__ order = c.order + b * c.S;
  // exclusive scan of the counters: the first slot of every segment in the batch's slice of `order`
  int carry = 0;
  for (int64_t t0 = 0; t0 < c.T; t0 += kPlaceThreads) {
    const int64_t t = t0 + tid;
    const int v = t < c.T ? count[t] : 0;
    int total;
    const int incl = block_scan<false>(v, buf, &total);
    if (t < c.T) cur[t] = carry + incl - v;
    carry += total;
  }
  __syncthreads();                               // cur[] is complete (global memory, this workgroup only)
  // placement, kPlaceThreads sources at a time in source order: sorting (key << 32 | position in the chunk) makes the
  // sources of one key a run in source order; a source's slot is its key's cursor plus its rank in the run, and the
  // last source of a run moves the cursor past the run
  constexpr unsigned long long kNone = ~0ull;    // an index outside [0, T), or past the end: sorts last, placed nowhere
  for (int64_t c0 = 0; c0 < c.S; c0 += kPlaceThreads) {
    const int64_t s = c0 + tid;
    const int32_t k = s < c.S ? key[s] : -1;
    sk[tid] = (k >= 0 && k < c.T) ? ((unsigned long long)(uint32_t)k << 32) | (uint32_t)tid : kNone;
    __syncthreads();
    for (int width = 2; width <= kPlaceThreads; width <<= 1) {
      for (int j = width >> 1; j > 0; j >>= 1) {
        const int partner = tid ^ j;
        if (partner > tid) {
          const unsigned long long lo = sk[tid], hi = sk[partner];
          const bool up = (tid & width) == 0;
          if ((lo > hi) == up) {
            sk[tid] = hi;
            sk[partner] = lo;
          }
        }
        __syncthreads();
      }
    }
    const unsigned long long v = sk[tid];
    const uint32_t kk = (uint32_t)(v >> 32);
    const bool head = tid == 0 || (uint32_t)(sk[tid - 1] >> 32) != kk;
    const bool tail = tid == kPlaceThreads - 1 || (uint32_t)(sk[tid + 1] >> 32) != kk;
    int unused;
    const int start = block_scan<true>(head ? tid : 0, buf, &unused);
    const bool ok = v != kNone;
    if (ok) order[cur[kk] + (tid - start)] = (int32_t)(c0 + (int64_t)(uint32_t)v);
    __syncthreads();                             // every read of cur[] for this chunk is done
    if (ok && tail) cur[kk] += tid - start + 1;
    __syncthreads();
  }
}

struct GradArgs {
  const float* x;
  const float* y;
  int64_t B, N, M;
  const int32_t* idx_xy;
  const int32_t* idx_yx;
  const float* grad_loss;
  float* grad_x;
  float* grad_y;
  CsrSide csr[2];              // [0]: targets x (sources y), [1]: targets y (sources x); as built by csr_place_kernel
  int64_t blocks_x;            // workgroups of the x side (0 when grad_x is NULL); the y side follows
};

constexpr int kGradThreads = 256;
constexpr int kSerialMax = 32;                   // a longer segment is summed by the whole wave

__global__ __launch_bounds__(kGradThreads) void grad_kernel(GradArgs a) {
  int64_t blk = blockIdx.x;
  const bool sx = blk < a.blocks_x;              // uniform over the workgroup
  if (!sx) blk -= a.blocks_x;
  const int lane = threadIdx.x & 63;
  const int64_t Tn = sx ? a.N : a.M, Sn = sx ? a.M : a.N;     // points of this side, of the other cloud
  const float* __restrict__ self = sx ? a.x : a.y;
  const float* __restrict__ other = sx ? a.y : a.x;
  const int32_t* __restrict__ direct = sx ? a.idx_xy : a.idx_yx;
  const CsrSide c = a.csr[sx ? 0 : 1];
  float* __restrict__ grad = sx ? a.grad_x : a.grad_y;
  const int64_t p = blk * kGradThreads + threadIdx.x;
  const bool active = p < a.B * Tn;
  const int64_t b = active ? p / Tn : 0;
  const float* __restrict__ oth = other + 3 * b * Sn;
  double px = 0.0, py = 0.0, pz = 0.0, dx = 0.0, dy = 0.0, dz = 0.0, rx = 0.0, ry = 0.0, rz = 0.0;
  int32_t st = 0, en = 0;
  if (active) {
    px = self[3 * p];
    py = self[3 * p + 1];
    pz = self[3 * p + 2];
    const int32_t j = direct[p];
    if (j >= 0 && j < Sn) {
      dx = px - (double)oth[3 * (int64_t)j];
      dy = py - (double)oth[3 * (int64_t)j + 1];
      dz = pz - (double)oth[3 * (int64_t)j + 2];
    }
    en = c.end[p];
    st = en - c.count[p];
  }
  const int32_t* __restrict__ ord = c.order + b * Sn;
  if (en - st <= kSerialMax) {
    for (int32_t k = st; k < en; ++k) {
      const int64_t j = ord[k];
      rx += px - (double)oth[3 * j];
      ry += py - (double)oth[3 * j + 1];
      rz += pz - (double)oth[3 * j + 2];
    }
  }
  // long segments (a target that is the nearest point of many sources): the wave sums them one after the other
  unsigned long long longs = __ballot(active && en - st > kSerialMax);
  while (longs) {
    const int l = __ffsll((long long)longs) - 1;
    longs &= longs - 1;
    const int32_t st_l = __shfl(st, l), en_l = __shfl(en, l);
    const double qx = __shfl(px, l), qy = __shfl(py, l), qz = __shfl(pz, l);
    const int64_t b_l = __shfl((long long)b, l);
    const int32_t* __restrict__ ord_l = c.order + b_l * Sn;
    const float* __restrict__ oth_l = other + 3 * b_l * Sn;
    double ax = 0.0, ay = 0.0, az = 0.0;
    for (int32_t k = st_l + lane; k < en_l; k += 64) {
      const int64_t j = ord_l[k];
      ax += qx - (double)oth_l[3 * j];
      ay += qy - (double)oth_l[3 * j + 1];
      az += qz - (double)oth_l[3 * j + 2];
    }
    for (int off = 32; off > 0; off >>= 1) {
      ax += __shfl_xor(ax, off);
      ay += __shfl_xor(ay, off);
      az += __shfl_xor(az, off);
    }
    if (lane == l) {
      rx = ax;
      ry = ay;
      rz = az;
    }
  }
  if (!active) return;
  const double g = (double)*a.grad_loss;
  const double kd = g * (2.0 / ((double)a.B * (double)Tn)), kr = g * (2.0 / ((double)a.B * (double)Sn));
  grad[3 * p] = (float)(kd * dx + kr * rx);
  grad[3 * p + 1] = (float)(kd * dy + kr * ry);
  grad[3 * p + 2] = (float)(kd * dz + kr * rz);
}

// ---- host -------------------------------------------------------------------------------------------------------------
struct Layout {
  size_t packed, partial, cnt[2], end[2], ord[2], total;
};

FwdGrid fwd_grid(int64_t B, int64_t N, int64_t M) {
  return FwdGrid{B, N, M, cdiv(N, kSrc), cdiv(M, kChunk), cdiv(M, kSrc), cdiv(N, kChunk)};
}

// LIST_OK, or a refusal with its message
int check_shape(int64_t B, int64_t N, int64_t M) {
  if (B < 1 || N < 1 || M < 1 || B > INT32_MAX || N > INT32_MAX || M > INT32_MAX)
    return fail(LIST_ERR_SHAPE, "B = %lld, N = %lld, M = %lld: need 1 <= B, N, M <= INT32_MAX", (long long)B,
                (long long)N, (long long)M);
  if (B * N > INT32_MAX || B * M > INT32_MAX)
    return fail(LIST_ERR_SHAPE, "B*N = %lld, B*M = %lld: need both <= INT32_MAX", (long long)(B * N),
                (long long)(B * M));
  const FwdGrid g = fwd_grid(B, N, M);
  if (B * (g.sx * g.tx + g.sy * g.ty) > INT32_MAX)
    return fail(LIST_ERR_SHAPE, "B = %lld, N = %lld, M = %lld: more than INT32_MAX workgroups", (long long)B,
                (long long)N, (long long)M);
  return LIST_OK;
}

// ---- workspace: packed u64 [B (N + M)] | partial f64 [2 B] | per side (targets T, sources S: N, M then M, N):
//                 cnt i32 [B T] | end i32 [B T] | ord i32 [B S] ----
Layout layout(int64_t B, int64_t N, int64_t M) {
  Layout L;
  Carver c;
  L.packed = c.take((size_t)(B * (N + M)) * sizeof(unsigned long long));
  L.partial = c.take((size_t)(2 * B) * sizeof(double));
  const int64_t T[2] = {N, M}, S[2] = {M, N};
  for (int s = 0; s < 2; ++s) {
    L.cnt[s] = c.take((size_t)(B * T[s]) * sizeof(int32_t));
    L.end[s] = c.take((size_t)(B * T[s]) * sizeof(int32_t));
    L.ord[s] = c.take((size_t)(B * S[s]) * sizeof(int32_t));
  }
  L.total = c.total();
  return L;
}

// the workspace of both entry points: its layout, then its size
int check_ws(int64_t B, int64_t N, int64_t M, size_t workspace_bytes, Layout* L) {
  *L = layout(B, N, M);
  if (workspace_bytes < L->total) return workspace_too_small(workspace_bytes, L->total, "list_chamfer_workspace_bytes");
  return LIST_OK;
}

}  // namespace

extern "C" {

const char* list_loss_last_error(void) { return g_err; }

size_t list_chamfer_workspace_bytes(int64_t B, int64_t N, int64_t M) {
  return check_shape(B, N, M) == LIST_OK ? layout(B, N, M).total : 0;
}

int list_chamfer_fwd(const float* x, const float* y, int64_t B, int64_t N, int64_t M, float* d2_xy, int32_t* idx_xy,
                     float* d2_yx, int32_t* idx_yx, float* loss, void* workspace, size_t workspace_bytes,
                     void* stream) {
  if (int rc = check_shape(B, N, M)) return rc;
  if (!x || !y || !d2_xy || !idx_xy || !d2_yx || !idx_yx || !loss || !workspace)
    return fail(LIST_ERR_ARG, "x/y/d2_xy/idx_xy/d2_yx/idx_yx/loss/workspace is NULL");
  Layout L;
  if (int rc = check_ws(B, N, M, workspace_bytes, &L)) return rc;
  hipStream_t s = (hipStream_t)stream;
  unsigned long long* packed = at<unsigned long long>(workspace, L.packed);
  double* partial = at<double>(workspace, L.partial);
  hipError_t e = hipMemsetAsync(packed, 0xFF, (size_t)(B * (N + M)) * sizeof(unsigned long long), s);
  if (e != hipSuccess) return hip_fail(e, "hipMemsetAsync");
  const FwdGrid g = fwd_grid(B, N, M);
  if (int rc = launch("nn_sq_kernel", nn_sq_kernel, dim3((unsigned)(B * (g.sx * g.tx + g.sy * g.ty))),
                      dim3(kFwdThreads), s, x, y, g, packed))
    return rc;
  if (int rc = launch("loss_partial_kernel", loss_partial_kernel, dim3((unsigned)(2 * B)), dim3(kRedThreads), s, x, y,
                      B, N, M, packed, d2_xy, idx_xy, d2_yx, idx_yx, partial))
    return rc;
  return launch("loss_final_kernel", loss_final_kernel, dim3(1), dim3(1), s, partial, B, N, M, loss);
}

int list_chamfer_bwd(const float* x, const float* y, int64_t B, int64_t N, int64_t M, const int32_t* idx_xy,
                     const int32_t* idx_yx, const float* grad_loss, float* grad_x, float* grad_y, void* workspace,
                     size_t workspace_bytes, void* stream) {
  if (int rc = check_shape(B, N, M)) return rc;
  if (!x || !y || !idx_xy || !idx_yx || !grad_loss || !workspace)
    return fail(LIST_ERR_ARG, "x/y/idx_xy/idx_yx/grad_loss/workspace is NULL");
  if (!grad_x && !grad_y) return fail(LIST_ERR_ARG, "grad_x and grad_y are both NULL");
  Layout L;
  if (int rc = check_ws(B, N, M, workspace_bytes, &L)) return rc;
  hipStream_t s = (hipStream_t)stream;
  const bool want[2] = {grad_x != nullptr, grad_y != nullptr};
  auto i32 = [&](size_t off) { return at<int32_t>(workspace, off); };
  CsrSide side[2];
  side[0] = CsrSide{idx_yx, i32(L.cnt[0]), i32(L.end[0]), i32(L.ord[0]), M, N};
  side[1] = CsrSide{idx_xy, i32(L.cnt[1]), i32(L.end[1]), i32(L.ord[1]), N, M};
  CsrArgs a{};
  a.B = B;
  for (int k = 0; k < 2; ++k) {
    if (!want[k]) continue;
    const hipError_t e = hipMemsetAsync(side[k].count, 0, (size_t)(B * side[k].T) * sizeof(int32_t), s);
    if (e != hipSuccess) return hip_fail(e, "hipMemsetAsync");
    a.side[a.nsides] = side[k];
    a.hist_blocks[a.nsides] = cdiv(B * side[k].S, kHistThreads);
    ++a.nsides;
  }
  if (int rc = launch("csr_hist_kernel", csr_hist_kernel, dim3((unsigned)(a.hist_blocks[0] + a.hist_blocks[1])),
                      dim3(kHistThreads), s, a))
    return rc;
  if (int rc = launch("csr_place_kernel", csr_place_kernel, dim3((unsigned)(a.nsides * B)), dim3(kPlaceThreads), s, a))
    return rc;
  GradArgs ga{x, y, B, N, M, idx_xy, idx_yx, grad_loss, grad_x, grad_y, {side[0], side[1]},
              want[0] ? cdiv(B * N, kGradThreads) : 0};
  const int64_t blocks_y = want[1] ? cdiv(B * M, kGradThreads) : 0;
  return launch("grad_kernel", grad_kernel, dim3((unsigned)(ga.blocks_x + blocks_y)), dim3(kGradThreads), s, ga);
}

}  // extern "C"
