// Stage 2's loss and its gradients on the device (include/list_s2loss.h): pure streaming, float64 behind the loads.
//
//   occ_sum_kernel   1024 workgroups: S1 = sum t log(a), S0 = sum (1 - t) log(b) over the occupancy volume, each lane its
//                    grid-strided items in turn (16-byte loads, four items in flight), one float64 pair per workgroup;
//                    the logarithm is s2loss_math.h's (the library routine made this kernel compute-bound).
//   sdf_sum_kernel   64 workgroups, the same walk over sdf_pred / sdf_gt: two float64 sums and the integer count.
//   final_kernel     one workgroup: the partials through LDS, each sum folded in index order, the four values.
//   occ_grad_kernel  backward, one pass: reads occ and its target, writes grad_occ.
//   sdf_grad_kernel  backward: grad_sdf_pred.
//   log_kernel       diagnostic (list_s2loss_log): s2loss_math.h's logarithm as this device computes it.
//
// walk() is the one place that knows how a pair of streams is cut into head, items and tail (struct Cut, made on the
// host from the pointers' alignment); the four kernels differ in the functor it feeds.
#include <math.h>

#include <hip/hip_runtime.h>

#include "list_host.h"
#include "list_s2loss.h"

#pragma clang fp contract(off)

#include "s2loss_math.h"                         // below the pragma: its products and sums are not contracted either

namespace {

constexpr int kThreads = 256;
constexpr int kOccGroups = 1024;                 // constants of the contract: the order of the sums hangs on them,
constexpr int kSdfGroups = 64;                   // so they are no multiple of a CU count read at run time
constexpr int kUnroll = 4;                       // items in flight per lane: 4 x (16 + 16) bytes
constexpr int kGradGroupsMax = 4096;
constexpr int kFoldBatch = 16;                   // final_kernel: partials per LDS read batch; divides both group counts
static_assert(kOccGroups % kFoldBatch == 0 && kSdfGroups % kFoldBatch == 0, "final_kernel reads whole batches");
constexpr int64_t kMaxElems = (int64_t)1 << 36;

// elements [0, head) one by one, then `items` items of W elements from `head` on, then [tail, n) one by one
struct Cut {
  int64_t head, items, tail;
  int width;                                     // W: 4 (16-byte loads) or 1
};

template <typename TB>
__device__ __forceinline__ void load_item4(const float* __restrict__ a, const TB* __restrict__ b, float av[4],
                                           float bv[4]);

template <>
__device__ __forceinline__ void load_item4<float>(const float* __restrict__ a, const float* __restrict__ b,
                                                  float av[4], float bv[4]) {
  const float4 x = *reinterpret_cast<const float4*>(a), y = *reinterpret_cast<const float4*>(b);
  av[0] = x.x, av[1] = x.y, av[2] = x.z, av[3] = x.w;
  bv[0] = y.x, bv[1] = y.y, bv[2] = y.z, bv[3] = y.w;
}

template <>
__device__ __forceinline__ void load_item4<uint8_t>(const float* __restrict__ a, const uint8_t* __restrict__ b,
                                                    float av[4], float bv[4]) {
  const float4 x = *reinterpret_cast<const float4*>(a);
  const uint32_t y = *reinterpret_cast<const uint32_t*>(b);
  av[0] = x.x, av[1] = x.y, av[2] = x.z, av[3] = x.w;
#pragma unroll
  for (int k = 0; k < 4; ++k) bv[k] = (float)((y >> (8 * k)) & 0xffu);
}

template <int W, typename TB>
__device__ __forceinline__ void load_item(const float* __restrict__ a, const TB* __restrict__ b, float av[W],
                                          float bv[W]) {
  if constexpr (W == 4) {
    load_item4<TB>(a, b, av, bv);
  } else {
    av[0] = a[0];
    bv[0] = (float)b[0];
  }
}

// Thread T of `threads` takes items T, T + threads, ... in turn (kUnroll of them loaded before the first is used);
// thread 0 takes the head before and the tail after.  f.one(i, a, b) for a single element, f.item(i, av, bv) for W.
template <int W, typename TB, typename F>
__device__ __forceinline__ void walk(const float* __restrict__ a, const TB* __restrict__ b, const Cut c, int64_t n,
                                     int64_t T, int64_t threads, F& f) {
  if (T == 0)
    for (int64_t i = 0; i < c.head; ++i) f.one(i, a[i], (float)b[i]);
  int64_t it = T;
  for (; it + (kUnroll - 1) * threads < c.items; it += kUnroll * threads) {
    float av[kUnroll][W], bv[kUnroll][W];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const int64_t i = c.head + W * (it + u * threads);
      load_item<W, TB>(a + i, b + i, av[u], bv[u]);
    }
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) f.template item<W>(c.head + W * (it + u * threads), av[u], bv[u]);
  }
  for (; it < c.items; it += threads) {
    float av[W], bv[W];
    const int64_t i = c.head + W * it;
    load_item<W, TB>(a + i, b + i, av, bv);
    f.template item<W>(i, av, bv);
  }
  if (T == 0)
    for (int64_t i = c.tail; i < n; ++i) f.one(i, a[i], (float)b[i]);
}

// the logarithms' arguments, in float32 as torch forms them
__device__ __forceinline__ double arg_a(float o) { return (double)(o + 1e-8f); }
__device__ __forceinline__ double arg_b(float o) { return (double)((1.0f - o) + 1e-8f); }

struct OccSum {
  double s1 = 0.0, s0 = 0.0;
  __device__ __forceinline__ void one(int64_t, float o, float tf) {
    const double t = (double)tf;
    s1 += t * s2loss_log(arg_a(o));
    s0 += (1.0 - t) * s2loss_log(arg_b(o));
  }
  template <int W>
  __device__ __forceinline__ void item(int64_t i, const float* av, const float* bv) {
#pragma unroll
    for (int k = 0; k < W; ++k) one(i + k, av[k], bv[k]);
  }
};

struct SdfSum {
  double s;                                      // sdf_scale
  double e = 0.0, r = 0.0;
  unsigned long long same = 0;
  __device__ __forceinline__ void one(int64_t, float pf, float tf) {
    const double p = (double)pf, t = (double)tf;
    const double d = t * s - p, q = t - p / s;
    e += d * d;
    r += q * q;
    same += (tf > 0.5f) == (pf > 0.5f) ? 1u : 0u;
  }
  template <int W>
  __device__ __forceinline__ void item(int64_t i, const float* av, const float* bv) {
#pragma unroll
    for (int k = 0; k < W; ++k) one(i + k, av[k], bv[k]);
  }
};

// out[i] = val(a[i], b[i]): 16 bytes per lane where the walk is in items of four
template <typename V>
struct Store {
  V v;
  float* __restrict__ out;
  __device__ __forceinline__ void one(int64_t i, float x, float y) { out[i] = v(x, y); }
  template <int W>
  __device__ __forceinline__ void item(int64_t i, const float* av, const float* bv) {
    if constexpr (W == 4) {
      *reinterpret_cast<float4*>(out + i) = make_float4(v(av[0], bv[0]), v(av[1], bv[1]), v(av[2], bv[2]), v(av[3], bv[3]));
    } else {
      out[i] = v(av[0], bv[0]);
    }
  }
};

struct OccGradVal {
  double k, mw, w1;                              // g0 * (1000 / n), -w, 1 - w
  __device__ __forceinline__ float operator()(float o, float tf) const {
    const double t = (double)tf;
    return (float)(k * ((mw * t) / arg_a(o) + (w1 * (1.0 - t)) / arg_b(o)));
  }
};

struct SdfGradVal {
  double k, s;                                   // g1 * (-2 / B), sdf_scale
  __device__ __forceinline__ float operator()(float pf, float tf) const {
    return (float)(k * ((double)tf * s - (double)pf));
  }
};

// p[j] += p[j + k] for k = 128, 64, ..., 1; every lane returns p[0]
template <typename T>
__device__ __forceinline__ T block_fold(T v, T* __restrict__ p) {
  const int tid = threadIdx.x;
  p[tid] = v;
  __syncthreads();
  for (int k = kThreads / 2; k > 0; k >>= 1) {
    if (tid < k) p[tid] += p[tid + k];
    __syncthreads();
  }
  const T r = p[0];
  __syncthreads();                               // p is free again when this returns
  return r;
}

// partial: [2][kOccGroups], S1 then S0
template <typename TB, int W>
__global__ __launch_bounds__(kThreads) void occ_sum_kernel(const float* __restrict__ occ, const TB* __restrict__ gt,
                                                           Cut c, int64_t n, double* __restrict__ partial) {
  __shared__ double p[kThreads];
  OccSum f;
  walk<W, TB>(occ, gt, c, n, (int64_t)blockIdx.x * kThreads + threadIdx.x, (int64_t)kOccGroups * kThreads, f);
  const double s1 = block_fold(f.s1, p), s0 = block_fold(f.s0, p);
  if (threadIdx.x == 0) {
    partial[blockIdx.x] = s1;
    partial[kOccGroups + blockIdx.x] = s0;
  }
}

// partial: [2][kSdfGroups], squared error then squared real-valued error; same: [kSdfGroups]
template <int W>
__global__ __launch_bounds__(kThreads) void sdf_sum_kernel(const float* __restrict__ pred, const float* __restrict__ gt,
                                                           Cut c, int64_t n, double scale, double* __restrict__ partial,
                                                           unsigned long long* __restrict__ same) {
  __shared__ double p[kThreads];
  __shared__ unsigned long long q[kThreads];
  SdfSum f{scale};
  walk<W, float>(pred, gt, c, n, (int64_t)blockIdx.x * kThreads + threadIdx.x, (int64_t)kSdfGroups * kThreads, f);
  const double e = block_fold(f.e, p), r = block_fold(f.r, p);
  const unsigned long long m = block_fold(f.same, q);
  if (threadIdx.x == 0) {
    partial[blockIdx.x] = e;
    partial[kSdfGroups + blockIdx.x] = r;
    same[blockIdx.x] = m;
  }
}

__global__ __launch_bounds__(kThreads) void final_kernel(const double* __restrict__ occ_partial,
                                                         const double* __restrict__ sdf_partial,
                                                         const unsigned long long* __restrict__ same, double n_occ,
                                                         double B, double BN, double w, float* __restrict__ out) {
  __shared__ double po[2 * kOccGroups], ps[2 * kSdfGroups], sum[4];
  __shared__ unsigned long long cnt;
  const int tid = threadIdx.x;
  for (int i = tid; i < 2 * kOccGroups; i += kThreads) po[i] = occ_partial[i];
  for (int i = tid; i < 2 * kSdfGroups; i += kThreads) ps[i] = sdf_partial[i];
  __syncthreads();
  if (tid < 4) {                                 // four chains side by side, each in index order
    const double* __restrict__ src = tid < 2 ? po + tid * kOccGroups : ps + (tid - 2) * kSdfGroups;
    const int m = tid < 2 ? kOccGroups : kSdfGroups;
    // the chain of dependent adds is the floor of this kernel: the next kFoldBatch partials are read from LDS while
    // the current ones are added
    double cur[kFoldBatch], nxt[kFoldBatch], s = 0.0;
#pragma unroll
    for (int k = 0; k < kFoldBatch; ++k) cur[k] = src[k];
    for (int i = 0; i < m; i += kFoldBatch) {
      const int j = i + kFoldBatch < m ? i + kFoldBatch : i;      // (the last batch reads itself again)
#pragma unroll
      for (int k = 0; k < kFoldBatch; ++k) nxt[k] = src[j + k];
#pragma unroll
      for (int k = 0; k < kFoldBatch; ++k) s += cur[k];
#pragma unroll
      for (int k = 0; k < kFoldBatch; ++k) cur[k] = nxt[k];
    }
    sum[tid] = s;
  } else if (tid == 4) {
    unsigned long long m = 0;
    for (int i = 0; i < kSdfGroups; ++i) m += same[i];
    cnt = m;
  }
  __syncthreads();
  if (tid == 0) {
    out[0] = (float)(1000.0 * (-w * sum[0] / n_occ - (1.0 - w) * sum[1] / n_occ));
    out[1] = (float)(sum[2] / B);
    out[2] = (float)(1e4 * sum[3] / BN);
    out[3] = (float)((double)cnt / BN);
  }
}

template <typename TB, int W>
__global__ __launch_bounds__(kThreads) void occ_grad_kernel(const float* __restrict__ occ, const TB* __restrict__ gt,
                                                            Cut c, int64_t n, const float* __restrict__ grad_out,
                                                            double k, double w, float* __restrict__ grad_occ) {
  Store<OccGradVal> f{{(double)grad_out[0] * k, -w, 1.0 - w}, grad_occ};
  walk<W, TB>(occ, gt, c, n, (int64_t)blockIdx.x * kThreads + threadIdx.x, (int64_t)gridDim.x * kThreads, f);
}

template <int W>
__global__ __launch_bounds__(kThreads) void sdf_grad_kernel(const float* __restrict__ pred, const float* __restrict__ gt,
                                                            Cut c, int64_t n, const float* __restrict__ grad_out,
                                                            double k, double scale, float* __restrict__ grad_pred) {
  Store<SdfGradVal> f{{(double)grad_out[1] * k, scale}, grad_pred};
  walk<W, float>(pred, gt, c, n, (int64_t)blockIdx.x * kThreads + threadIdx.x, (int64_t)gridDim.x * kThreads, f);
}

__global__ __launch_bounds__(kThreads) void log_kernel(const float* __restrict__ x, int64_t n, double* __restrict__ out) {
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kThreads)
    out[i] = s2loss_log((double)x[i]);
}

// ---- host -------------------------------------------------------------------------------------------------------------
// Items of four when a (float32), b (elements of b_elem bytes) and, when there is one, out (float32) reach their vector
// alignment after the same number of head elements; else one element per item.
Cut cut(const float* a, const void* b, size_t b_elem, const float* out, int64_t n) {
  if (!misaligned(a, 4)) {
    const int64_t head = (int64_t)((16 - ((uintptr_t)a & 15)) & 15) / 4;
    const bool b_ok = !misaligned((const char*)b + head * (int64_t)b_elem, b_elem == 4 ? 16 : 4);
    const bool out_ok = !out || !misaligned(out + head, 16);
    if (b_ok && out_ok && n >= head + 4) {
      const int64_t items = (n - head) / 4;
      return Cut{head, items, head + 4 * items, 4};
    }
  }
  return Cut{0, n, n, 1};
}

struct Layout {
  size_t occ, sdf, same, total;
};

// ---- workspace: occ partials f64 [2 kOccGroups] | sdf partials f64 [2 kSdfGroups] | same u64 [kSdfGroups] ----
Layout layout() {
  Layout L;
  Carver c;
  L.occ = c.take((size_t)2 * kOccGroups * sizeof(double));
  L.sdf = c.take((size_t)2 * kSdfGroups * sizeof(double));
  L.same = c.take((size_t)kSdfGroups * sizeof(unsigned long long));
  L.total = c.total();
  return L;
}

// LIST_OK, or a refusal with its message
int check_shape(int64_t n_occ, int64_t B, int64_t N, int kind) {
  if (n_occ < 1 || n_occ > kMaxElems)
    return fail(LIST_ERR_SHAPE, "n_occ = %lld: need 1 <= n_occ <= 2^36", (long long)n_occ);
  if (B < 1 || N < 1 || B > kMaxElems / N)
    return fail(LIST_ERR_SHAPE, "B = %lld, N = %lld: need 1 <= B, N and B*N <= 2^36", (long long)B, (long long)N);
  if (kind != 0 && kind != 1)
    return fail(LIST_ERR_SHAPE, "occ_gt_kind = %d: 0 (float32) or 1 (uint8)", kind);
  return LIST_OK;
}

unsigned grad_groups(const Cut& c) { return blocks_capped(c.items, kThreads * kUnroll, kGradGroupsMax); }

}  // namespace

extern "C" {

const char* list_s2loss_last_error(void) { return g_err; }

size_t list_s2loss_workspace_bytes(int64_t n_occ, int64_t B, int64_t N) {
  if (check_shape(n_occ, B, N, 0) != LIST_OK) return 0;
  return layout().total;
}

int list_s2loss_fwd(const float* occ, const void* occ_gt, int occ_gt_kind, int64_t n_occ, const float* sdf_pred,
                    const float* sdf_gt, int64_t B, int64_t N, float sdf_scale, float w, float* out, void* workspace,
                    size_t workspace_bytes, void* stream) {
  if (int rc = check_shape(n_occ, B, N, occ_gt_kind)) return rc;
  const char* null = !occ ? "occ" : !occ_gt ? "occ_gt" : !sdf_pred ? "sdf_pred" : !sdf_gt ? "sdf_gt" : !out ? "out"
                     : !workspace ? "workspace" : nullptr;
  if (null) return fail(LIST_ERR_ARG, "%s is NULL", null);
  const Layout L = layout();
  if (workspace_bytes < L.total) return workspace_too_small(workspace_bytes, L.total, "list_s2loss_workspace_bytes");
  hipStream_t s = (hipStream_t)stream;
  double* occ_partial = at<double>(workspace, L.occ);
  double* sdf_partial = at<double>(workspace, L.sdf);
  unsigned long long* same = at<unsigned long long>(workspace, L.same);
  const dim3 block(kThreads);
  const Cut co = cut(occ, occ_gt, occ_gt_kind ? 1 : 4, nullptr, n_occ);
  auto occ_sum = [&](auto kernel, auto gt) {
    return launch("occ_sum_kernel", kernel, dim3(kOccGroups), block, s, occ, gt, co, n_occ, occ_partial);
  };
  int rc;
  if (occ_gt_kind == 0) {
    const float* gt = (const float*)occ_gt;
    rc = co.width == 4 ? occ_sum(occ_sum_kernel<float, 4>, gt) : occ_sum(occ_sum_kernel<float, 1>, gt);
  } else {
    const uint8_t* gt = (const uint8_t*)occ_gt;
    rc = co.width == 4 ? occ_sum(occ_sum_kernel<uint8_t, 4>, gt) : occ_sum(occ_sum_kernel<uint8_t, 1>, gt);
  }
  if (rc) return rc;
  const int64_t BN = B * N;
  const Cut cs = cut(sdf_pred, sdf_gt, 4, nullptr, BN);
  auto sdf_sum = [&](auto kernel) {
    return launch("sdf_sum_kernel", kernel, dim3(kSdfGroups), block, s, sdf_pred, sdf_gt, cs, BN, (double)sdf_scale,
                  sdf_partial, same);
  };
  if ((rc = cs.width == 4 ? sdf_sum(sdf_sum_kernel<4>) : sdf_sum(sdf_sum_kernel<1>))) return rc;
  return launch("final_kernel", final_kernel, dim3(1), block, s, occ_partial, sdf_partial, same, (double)n_occ,
                (double)B, (double)BN, (double)w, out);
}

int list_s2loss_bwd(const float* occ, const void* occ_gt, int occ_gt_kind, int64_t n_occ, const float* sdf_pred,
                    const float* sdf_gt, int64_t B, int64_t N, float sdf_scale, float w, const float* grad_out,
                    float* grad_occ, float* grad_sdf_pred, void* stream) {
  if (int rc = check_shape(n_occ, B, N, occ_gt_kind)) return rc;
  const char* null = !occ ? "occ" : !occ_gt ? "occ_gt" : !sdf_pred ? "sdf_pred" : !sdf_gt ? "sdf_gt"
                     : !grad_out ? "grad_out" : nullptr;
  if (null) return fail(LIST_ERR_ARG, "%s is NULL", null);
  if (!grad_occ && !grad_sdf_pred) return fail(LIST_ERR_ARG, "grad_occ and grad_sdf_pred are both NULL");
  hipStream_t s = (hipStream_t)stream;
  const dim3 block(kThreads);
  if (grad_occ) {
    const Cut c = cut(occ, occ_gt, occ_gt_kind ? 1 : 4, grad_occ, n_occ);
    const dim3 grid(grad_groups(c));
    const double k = 1000.0 / (double)n_occ, wd = (double)w;
    auto occ_grad = [&](auto kernel, auto gt) {
      return launch("occ_grad_kernel", kernel, grid, block, s, occ, gt, c, n_occ, grad_out, k, wd, grad_occ);
    };
    int rc;
    if (occ_gt_kind == 0) {
      const float* gt = (const float*)occ_gt;
      rc = c.width == 4 ? occ_grad(occ_grad_kernel<float, 4>, gt) : occ_grad(occ_grad_kernel<float, 1>, gt);
    } else {
      const uint8_t* gt = (const uint8_t*)occ_gt;
      rc = c.width == 4 ? occ_grad(occ_grad_kernel<uint8_t, 4>, gt) : occ_grad(occ_grad_kernel<uint8_t, 1>, gt);
    }
    if (rc) return rc;
  }
  if (grad_sdf_pred) {
    const int64_t BN = B * N;
    const Cut c = cut(sdf_pred, sdf_gt, 4, grad_sdf_pred, BN);
    const dim3 grid(grad_groups(c));
    const double k = -2.0 / (double)B;
    auto sdf_grad = [&](auto kernel) {
      return launch("sdf_grad_kernel", kernel, grid, block, s, sdf_pred, sdf_gt, c, BN, grad_out, k, (double)sdf_scale,
                    grad_sdf_pred);
    };
    return c.width == 4 ? sdf_grad(sdf_grad_kernel<4>) : sdf_grad(sdf_grad_kernel<1>);
  }
  return LIST_OK;
}

int list_s2loss_log(const float* x, int64_t n, double* out, void* stream) {
  if (n < 1 || n > kMaxElems) return fail(LIST_ERR_SHAPE, "n = %lld: need 1 <= n <= 2^36", (long long)n);
  if (!x || !out) return fail(LIST_ERR_ARG, "%s is NULL", !x ? "x" : "out");
  return launch("log_kernel", log_kernel, dim3(blocks_capped(n, kThreads, kGradGroupsMax)), dim3(kThreads),
                (hipStream_t)stream, x, n, out);
}

}  // extern "C"
