// The coarse stage on the device (include/list_coarse.h): tree decoder, point MLP with its max, camera, occupancy.
//
//   coarse_tree_kernel<NB>   one TreeGCN layer.  A workgroup owns one (node n, child d) and up to NB <= 16 images: it
//                            streams the in x in slab W_branch[n][:, d in : (d + 1) in] from where the parameter lies
//                            (16-byte loads along the last axis, each element read once per group of 16 images),
//                            keeps leaky(leaves @ slab) in LDS and multiplies it by the composed Wc there; the
//                            ancestor term reads tree[i][b][n / reps] by index.
//   coarse_mlp_kernel        point MLP 3 -> 64 -> 256 -> 512 on a tile of 64 points whose activations stay in LDS: the
//                            first layer on the VALU, the two wide ones on v_mfma_f32_32x32x2_f32 (exact fp32
//                            products); epilogue bias, BN scale and shift, ReLU; the tile's per-channel maximum over
//                            its REAL rows goes to the workspace.
//   coarse_max_kernel        the tiles' maxima reduced in tile order (no atomics); a NaN stays a NaN.
//   coarse_camera_kernel     the three Linear layers of the camera, one workgroup per image.
//   coarse_clear_kernel / coarse_mark_kernel   the occupancy grid.
// The build passes -ffp-contract=off: every fused multiply-add here is an explicit fmaf.
#include <hip/hip_runtime.h>

#include "list_coarse.h"
#include "list_host.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxL = LIST_COARSE_MAX_LAYERS;
constexpr int kGroup = LIST_COARSE_GROUP;
constexpr int kTile = LIST_COARSE_TILE;
constexpr int kCode = LIST_COARSE_CODE;
constexpr int kM1 = 64, kM2 = 256;                      // widths of the point MLP's hidden layers
constexpr int kMaxFeat = 256, kMaxG2 = 1024, kMaxHidden = 256;
constexpr int64_t kMaxPoints = (int64_t)1 << 22;
constexpr float kSlope = 0.2f;

typedef float f32x16 __attribute__((ext_vector_type(16)));

// ---- packed weights and workspace ------------------------------------------------------------------------------------
// Every array is fp32 and starts on a 256-byte boundary.  Matrices are stored TRANSPOSED ([in][out]) so that threads
// on consecutive outputs read consecutive addresses; the first layer of the point MLP ([64][3]) stays as it is.
struct PackedLayout {
  size_t root[kMaxL][kMaxL], wc[kMaxL], bias[kMaxL];
  size_t mlp_w[3], mlp_b[3], mlp_s[3], mlp_t[3];
  size_t cam_w[3], cam_b[3], cam_s[2], cam_t[2];
  size_t total;
};

int mlp_width(int k) { return k == 0 ? 3 : k == 1 ? kM1 : k == 2 ? kM2 : kCode; }
int cam_in(const ListCoarseShape& s, int k) { return k == 0 ? kCode + s.g2 : s.hidden; }
int cam_out(const ListCoarseShape& s, int k) { return k == 2 ? 12 : s.hidden; }

PackedLayout packed_layout(const ListCoarseShape& s) {
  PackedLayout p = {};
  Carver c;
  auto f32 = [&](size_t n) { return c.take(n * sizeof(float)); };
  const int L = s.n_degrees;
  for (int l = 0; l < L; ++l) {
    for (int i = 0; i <= l; ++i) p.root[l][i] = f32((size_t)s.features[i] * s.features[l + 1]);
    p.wc[l] = f32((size_t)s.features[l] * s.features[l + 1]);
    if (s.activation[l]) p.bias[l] = f32((size_t)s.degrees[l] * s.features[l + 1]);
  }
  if (s.has_mlp)
    for (int k = 0; k < 3; ++k) {
      p.mlp_w[k] = f32((size_t)mlp_width(k) * mlp_width(k + 1));
      p.mlp_b[k] = f32(mlp_width(k + 1));
      p.mlp_s[k] = f32(mlp_width(k + 1));
      p.mlp_t[k] = f32(mlp_width(k + 1));
    }
  if (s.has_camera)
    for (int k = 0; k < 3; ++k) {
      p.cam_w[k] = f32((size_t)cam_in(s, k) * cam_out(s, k));
      p.cam_b[k] = f32(cam_out(s, k));
      if (k < 2) { p.cam_s[k] = f32(cam_out(s, k)); p.cam_t[k] = f32(cam_out(s, k)); }
    }
  p.total = c.total();
  return p;
}

int64_t nodes_of(const ListCoarseShape& s, int l) {      // nodes of tree level l (level 0: the image code)
  int64_t n = 1;
  for (int i = 0; i < l; ++i) n *= s.degrees[i];
  return n;
}

struct WorkspaceLayout { size_t level[kMaxL], tile_max, total; };

WorkspaceLayout workspace_layout(const ListCoarseShape& s, int B) {
  WorkspaceLayout w = {};
  Carver c;
  const int L = s.n_degrees;
  for (int l = 1; l < L; ++l) w.level[l] = c.take((size_t)B * nodes_of(s, l) * s.features[l] * sizeof(float));
  if (s.has_mlp) w.tile_max = c.take((size_t)B * cdiv(nodes_of(s, L), kTile) * kCode * sizeof(float));
  w.total = c.total() ? c.total() : 256;
  return w;
}

int check_shape(const ListCoarseShape* s) {
  if (!s) return fail(LIST_ERR_ARG, "shape is NULL");
  if (s->n_degrees < 1 || s->n_degrees > kMaxL)
    return fail(LIST_ERR_SHAPE, "n_degrees = %d: the decoder has 1 to %d layers", s->n_degrees, kMaxL);
  if (s->n_features - 1 != s->n_degrees)
    return fail(LIST_ERR_SHAPE, "n_features = %d, n_degrees = %d: features must be one longer than degrees",
                s->n_features, s->n_degrees);
  const int L = s->n_degrees;
  int64_t P = 1;
  for (int l = 0; l < L; ++l) {
    const int in = s->features[l], out = s->features[l + 1];
    if (in < 16 || in % 16 != 0 || in > kMaxFeat)
      return fail(LIST_ERR_SHAPE, "features[%d] = %d: an input width must be a multiple of 16, at most %d", l, in,
                  kMaxFeat);
    if (out < 1 || out > kMaxFeat)
      return fail(LIST_ERR_SHAPE, "features[%d] = %d: an output width must be in [1, %d]", l + 1, out, kMaxFeat);
    if (s->degrees[l] < 1) return fail(LIST_ERR_SHAPE, "degrees[%d] = %d: must be at least 1", l, s->degrees[l]);
    P *= s->degrees[l];
    if (P > kMaxPoints) return fail(LIST_ERR_SHAPE, "prod(degrees) exceeds %lld points", (long long)kMaxPoints);
  }
  if (s->features[L] != 3)
    return fail(LIST_ERR_SHAPE, "features[%d] = %d: the last layer must give 3 coordinates", L, s->features[L]);
  if (s->has_camera) {
    if (!s->has_mlp) return fail(LIST_ERR_SHAPE, "has_camera without has_mlp: the camera reads the point MLP's code");
    if (s->g2 < 1 || s->g2 > kMaxG2) return fail(LIST_ERR_SHAPE, "g2 = %d: must be in [1, %d]", s->g2, kMaxG2);
    if (s->hidden < 1 || s->hidden > kMaxHidden)
      return fail(LIST_ERR_SHAPE, "hidden = %d: must be in [1, %d]", s->hidden, kMaxHidden);
  }
  return LIST_OK;
}

int check_batch(int32_t B) {
  if (B < 1 || B > 65535) return fail(LIST_ERR_SHAPE, "B = %d: must be in [1, 65535]", B);
  return LIST_OK;
}

int n_steps_of(const ListCoarseShape& s) { return s.n_degrees + 5; }

// ---- prep ------------------------------------------------------------------------------------------------------------
// dst[c][r] = src[r][c] for src [rows][cols]; transpose == 0: a copy
__global__ void coarse_pack_kernel(const float* __restrict__ src, float* __restrict__ dst, int rows, int cols,
                                   int transpose) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= rows * cols) return;
  const int r = i / cols, c = i % cols;
  dst[transpose ? c * rows + r : i] = src[i];
}

// ---- tree layer ------------------------------------------------------------------------------------------------------
struct TreeArgs {
  const float* level[kMaxL];            // level[i]: [B][nodes[i]][feat[i]], i <= depth; level[depth]: the leaves
  const float* rootT[kMaxL];            // [feat[i]][out]
  int32_t nodes[kMaxL], feat[kMaxL];
  const float* wcT;                     // [in][out]
  const float* bias;                    // [deg][out], NULL without activation
  const float* w_branch;                // [node][in][deg * in], the parameter itself
  float* out;                           // [B][node * deg][out]
  int32_t depth, node, in, out_f, deg, B;
};

__device__ __forceinline__ float leaky(float v) { return v > 0.f ? v : kSlope * v; }      // (a NaN stays a NaN)

template <int NB>
__global__ __launch_bounds__(kThreads) void coarse_tree_kernel(TreeArgs a) {
  __shared__ float leavesT[kMaxFeat * NB];              // [in][NB]: one row of the slab meets all images
  __shared__ float g[NB * kMaxFeat];                    // [NB][in]: leaves @ slab, then its leaky
  const int t = threadIdx.x;
  const int n = blockIdx.x / a.deg, d = blockIdx.x % a.deg;
  const int b0 = blockIdx.y * kGroup;
  const int nb = min(NB, a.B - b0);
  const int in = a.in, out = a.out_f;

  const float* leaves = a.level[a.depth];
  for (int idx = t; idx < in * NB; idx += kThreads) {
    const int i = idx / NB, b = idx % NB;
    leavesT[idx] = b < nb ? leaves[((int64_t)(b0 + b) * a.node + n) * in + i] : 0.f;
  }
  __syncthreads();

  // the slab: `in` rows of `in` floats, row stride deg * in.  Thread (rg, c) takes the float4 column c of the rows
  // rg, rg + RG, ...: a wave reads whole runs of consecutive 16-byte words.
  const int C4 = in / 4, RG = kThreads / C4;
  const int c = t % C4, rg = t / C4;
  float acc[NB][4];
#pragma unroll
  for (int b = 0; b < NB; ++b) acc[b][0] = acc[b][1] = acc[b][2] = acc[b][3] = 0.f;
  if (rg < RG) {
    const int64_t stride4 = (int64_t)a.deg * C4;
    const float4* slab = reinterpret_cast<const float4*>(a.w_branch) + (int64_t)n * in * stride4 + (int64_t)d * C4 + c;
#pragma unroll 4
    for (int i = rg; i < in; i += RG) {
      const float4 w = slab[i * stride4];
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        const float x = leavesT[i * NB + b];
        acc[b][0] = fmaf(x, w.x, acc[b][0]);
        acc[b][1] = fmaf(x, w.y, acc[b][1]);
        acc[b][2] = fmaf(x, w.z, acc[b][2]);
        acc[b][3] = fmaf(x, w.w, acc[b][3]);
      }
    }
  }
  // the RG partial sums of a column, added in row-group order
  for (int r = 0; r < RG; ++r) {
    if (rg == r) {
#pragma unroll
      for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          float* p = &g[b * in + 4 * c + k];
          *p = r == 0 ? acc[b][k] : *p + acc[b][k];
        }
    }
    __syncthreads();
  }
  for (int idx = t; idx < NB * in; idx += kThreads) g[idx] = leaky(g[idx]);
  __syncthreads();

  // ancestors + Wc leaky(...) + bias, one thread per (image, output)
  for (int idx = t; idx < nb * out; idx += kThreads) {
    const int b = idx / out, o = idx % out;
    float z = 0.f;
    for (int l = 0; l <= a.depth; ++l) {
      const int reps = a.node / a.nodes[l], f = a.feat[l];
      const float* src = a.level[l] + ((int64_t)(b0 + b) * a.nodes[l] + n / reps) * f;
      const float* w = a.rootT[l] + o;
      for (int i = 0; i < f; ++i) z = fmaf(src[i], w[(int64_t)i * out], z);
    }
    const float* gb = &g[b * in];
    const float* w = a.wcT + o;
    for (int j = 0; j < in; ++j) z = fmaf(gb[j], w[(int64_t)j * out], z);
    if (a.bias) z = leaky(z + a.bias[d * out + o]);
    a.out[((int64_t)(b0 + b) * a.node * a.deg + (int64_t)n * a.deg + d) * out + o] = z;
  }
}

// (a launch error of the forward is reported under the entry point's name, not the kernel's)
int launch_tree(const TreeArgs& a, hipStream_t s) {
  const dim3 grid((unsigned)((int64_t)a.node * a.deg), (unsigned)cdiv(a.B, kGroup));
  const int nb = a.B < kGroup ? a.B : kGroup;
  auto run = [&](auto kernel) { return launch("list_coarse_forward", kernel, grid, dim3(kThreads), s, a); };
  if (nb <= 1) return run(coarse_tree_kernel<1>);
  if (nb <= 2) return run(coarse_tree_kernel<2>);
  if (nb <= 4) return run(coarse_tree_kernel<4>);
  if (nb <= 8) return run(coarse_tree_kernel<8>);
  return run(coarse_tree_kernel<16>);
}

// ---- point MLP -------------------------------------------------------------------------------------------------------
struct MlpArgs {
  const float* pc;                      // [B][P][3]
  const float *w1, *b1, *s1, *t1;       // w1: [64][3]
  const float *w2T, *b2, *s2, *t2;      // w2T: [64][256]
  const float *w3T, *b3, *s3, *t3;      // w3T: [256][512]
  float* tile_max;                      // [B][tiles][512]
  int32_t P, tiles;
};

__device__ __forceinline__ float relu(float v) { return v < 0.f ? 0.f : v; }              // (a NaN stays a NaN)
// max as torch.max takes it: a NaN on either side wins
__device__ __forceinline__ float nanmax(float m, float v) { return (v > m || v != v) ? v : m; }

constexpr int kH1Pad = kM1 + 1, kH2Half = kM2 / 2, kH2Pad = kH2Half + 1;

__global__ __launch_bounds__(kThreads) void coarse_mlp_kernel(MlpArgs a) {
  __shared__ float pts[kTile][3];
  __shared__ float h1[kTile][kH1Pad];
  __shared__ float h2[kTile][kH2Pad];                   // one half (128 channels) of the second layer at a time
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int tile = blockIdx.x, b = blockIdx.y;
  const int r32 = lane & 31, hi = lane >> 5;

  if (t < kTile * 3) {
    const int64_t p = (int64_t)tile * kTile + t / 3;
    pts[t / 3][t % 3] = p < a.P ? a.pc[((int64_t)b * a.P + p) * 3 + t % 3] : 0.f;
  }
  __syncthreads();
  for (int idx = t; idx < kTile * kM1; idx += kThreads) {
    const int c = idx & (kM1 - 1), p = idx >> 6;
    float z = fmaf(a.w1[c * 3 + 2], pts[p][2], fmaf(a.w1[c * 3 + 1], pts[p][1], a.w1[c * 3] * pts[p][0])) + a.b1[c];
    h1[p][c] = relu(z * a.s1[c] + a.t1[c]);
  }
  __syncthreads();

  // third layer: wave w owns output channels [128 w, 128 w + 128): 2 row tiles x 4 column tiles of 32 x 32
  f32x16 acc3[2][4];
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int nt = 0; nt < 4; ++nt)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc3[m][nt][r] = 0.f;

  for (int half = 0; half < 2; ++half) {
    // second layer, channels [128 half, 128 half + 128): wave w owns 32 of them.  A[i][k] = h1[point i][k] (lane:
    // i = lane & 31, k = lane >> 5), B[k][j] = w2T[k][channel j]
    {
      const int cbase = half * kH2Half + wave * 32;
      f32x16 acc2[2];
#pragma unroll
      for (int r = 0; r < 16; ++r) acc2[0][r] = acc2[1][r] = 0.f;
#pragma unroll 8
      for (int k0 = 0; k0 < kM1; k0 += 2) {
        const int kk = k0 + hi;
        const float bv = a.w2T[kk * kM2 + cbase + r32];
        acc2[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(h1[r32][kk], bv, acc2[0], 0, 0, 0);
        acc2[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(h1[32 + r32][kk], bv, acc2[1], 0, 0, 0);
      }
      const int col = cbase + r32;
      const float bias = a.b2[col], sc = a.s2[col], sh = a.t2[col];
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = m * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
          h2[row][col - half * kH2Half] = relu((acc2[m][r] + bias) * sc + sh);
        }
    }
    __syncthreads();
#pragma unroll 4
    for (int k0 = 0; k0 < kH2Half; k0 += 2) {
      const int kk = k0 + hi;
      const float a0 = h2[r32][kk], a1 = h2[32 + r32][kk];
      const float* wrow = a.w3T + (int64_t)(half * kH2Half + kk) * kCode + wave * 128 + r32;
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) {
        const float bv = wrow[nt * 32];
        acc3[0][nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, bv, acc3[0][nt], 0, 0, 0);
        acc3[1][nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, bv, acc3[1][nt], 0, 0, 0);
      }
    }
    __syncthreads();                                    // h2 is rewritten by the next half
  }

  // epilogue and the maximum over the tile's real rows: a row that pads the last tile holds relu(bn(bias)), which
  // can exceed every real value, so it takes no part
  const int valid = min((int64_t)kTile, (int64_t)a.P - (int64_t)tile * kTile);
#pragma unroll
  for (int nt = 0; nt < 4; ++nt) {
    const int col = wave * 128 + nt * 32 + r32;
    const float bias = a.b3[col], sc = a.s3[col], sh = a.t3[col];
    float m = -INFINITY;
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = mt * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
        const float v = relu((acc3[mt][nt][r] + bias) * sc + sh);
        if (row < valid) m = nanmax(m, v);
      }
    m = nanmax(m, __shfl_xor(m, 32));
    if (hi == 0) a.tile_max[((int64_t)b * a.tiles + tile) * kCode + col] = m;
  }
}

__global__ __launch_bounds__(kCode) void coarse_max_kernel(const float* __restrict__ tile_max, float* __restrict__ coarse,
                                                           int tiles) {
  const int b = blockIdx.x, c = threadIdx.x;
  float m = -INFINITY;
  for (int i = 0; i < tiles; ++i) m = nanmax(m, tile_max[((int64_t)b * tiles + i) * kCode + c]);
  coarse[(int64_t)b * kCode + c] = m;
}

// ---- camera ----------------------------------------------------------------------------------------------------------
struct CameraArgs {
  const float *coarse, *feat_g2;        // [B][512], [B][g2]
  const float* wT[3];                   // [K][H]
  const float* b[3];
  const float* s[2];
  const float* t[2];
  float* trans_mat;                     // [B][12]
  int32_t g2, hidden;
};

// y[o] = sum_k x[k] wT[k][o] for o < H: the K range is cut into kThreads / H slices whose sums are added in order
__device__ __forceinline__ float camera_dot(const float* x, int K, const float* __restrict__ wT, int H, float* part) {
  const int t = threadIdx.x, parts = kThreads / H, o = t % H, pr = t / H;
  if (pr < parts) {
    const int slice = (K + parts - 1) / parts, k1 = min(K, (pr + 1) * slice);
    float z = 0.f;
    for (int k = pr * slice; k < k1; ++k) z = fmaf(x[k], wT[(int64_t)k * H + o], z);
    part[pr * H + o] = z;
  }
  __syncthreads();
  float z = 0.f;
  if (t < H)
    for (int p = 0; p < parts; ++p) z += part[p * H + t];
  __syncthreads();
  return z;
}

__global__ __launch_bounds__(kThreads) void coarse_camera_kernel(CameraArgs a) {
  __shared__ float x[kCode + kMaxG2];
  __shared__ float h[2][kMaxHidden];
  __shared__ float part[kThreads];
  const int t = threadIdx.x, b = blockIdx.x, K0 = kCode + a.g2, H = a.hidden;
  for (int k = t; k < K0; k += kThreads)
    x[k] = k < kCode ? a.coarse[(int64_t)b * kCode + k] : a.feat_g2[(int64_t)b * a.g2 + (k - kCode)];
  __syncthreads();
  for (int layer = 0; layer < 2; ++layer) {
    const float z = camera_dot(layer == 0 ? x : h[0], layer == 0 ? K0 : H, a.wT[layer], H, part);
    if (t < H) h[layer][t] = leaky(z + a.b[layer][t]) * a.s[layer][t] + a.t[layer][t];
    __syncthreads();
  }
  const float z = camera_dot(h[1], H, a.wT[2], 12, part);
  if (t < 12) a.trans_mat[(int64_t)b * 12 + t] = z + a.b[2][t];
}

// ---- occupancy -------------------------------------------------------------------------------------------------------
__global__ void coarse_clear_kernel(float4* __restrict__ occ4, int64_t n4, float* __restrict__ occ, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i < n4) occ4[i] = make_float4(0.f, 0.f, 0.f, 0.f);
  if (i < n - 4 * n4) occ[4 * n4 + i] = 0.f;            // the tail of a grid whose size is no multiple of 4
}

// LIST.create_occ, operation for operation in fp32: (p - bb_min) / extent * (R - 1), + 0.5, floor, clamp
__device__ __forceinline__ int voxel_index(float p, float bb_min, float extent, int R) {
  float v = (p - bb_min) / extent;
  v = v * (float)(R - 1);
  v = floorf(v + 0.5f);
  return (int)fminf(fmaxf(v, 0.f), (float)(R - 1));
}

__global__ void coarse_mark_kernel(const float* __restrict__ pc, float* __restrict__ occ, int64_t BP, int P, int R,
                                   float bb_min, float extent) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= BP) return;
  const float x = pc[i * 3], y = pc[i * 3 + 1], z = pc[i * 3 + 2];
  if (!(isfinite(x) && isfinite(y) && isfinite(z))) return;
  const int64_t b = i / P;
  const int ix = voxel_index(x, bb_min, extent, R), iy = voxel_index(y, bb_min, extent, R),
            iz = voxel_index(z, bb_min, extent, R);
  occ[((b * R + ix) * R + iy) * (int64_t)R + iz] = 1.0f;
}

}  // namespace

extern "C" {

const char* list_coarse_last_error(void) { return g_err; }

size_t list_coarse_weight_bytes(const ListCoarseShape* shape) {
  if (check_shape(shape) != LIST_OK) return 0;
  return packed_layout(*shape).total;
}

size_t list_coarse_workspace_bytes(const ListCoarseShape* shape, int32_t B) {
  if (check_shape(shape) != LIST_OK || check_batch(B) != LIST_OK) return 0;
  return workspace_layout(*shape, B).total;
}

int32_t list_coarse_n_steps(const ListCoarseShape* shape) {
  if (check_shape(shape) != LIST_OK) return 0;
  return n_steps_of(*shape);
}

int list_coarse_prep_weights(const ListCoarseShape* shape, const ListCoarseParams* params, void* packed,
                             size_t packed_bytes, void* stream) {
  if (int rc = check_shape(shape)) return rc;
  if (!params || !packed)
    return fail(LIST_ERR_ARG, "list_coarse_prep_weights: %s is NULL", params ? "packed" : "params");
  const ListCoarseShape& S = *shape;
  const PackedLayout P = packed_layout(S);
  if (packed_bytes < P.total) return packed_too_small("list_coarse_prep_weights", packed_bytes, P.total);
  const int L = S.n_degrees;
  for (int l = 0; l < L; ++l) {
    for (int i = 0; i <= l; ++i)
      if (!params->w_root[l][i]) return fail(LIST_ERR_ARG, "list_coarse_prep_weights: w_root[%d][%d] is NULL", l, i);
    if (!params->wc[l]) return fail(LIST_ERR_ARG, "list_coarse_prep_weights: wc[%d] is NULL", l);
    if (S.activation[l] && !params->bias[l]) return fail(LIST_ERR_ARG, "list_coarse_prep_weights: bias[%d] is NULL", l);
  }
  if (S.has_mlp)
    for (int k = 0; k < 3; ++k)
      if (!params->mlp_w[k] || !params->mlp_b[k] || !params->mlp_s[k] || !params->mlp_t[k])
        return fail(LIST_ERR_ARG, "list_coarse_prep_weights: a point-MLP array of layer %d is NULL", k);
  if (S.has_camera)
    for (int k = 0; k < 3; ++k)
      if (!params->cam_w[k] || !params->cam_b[k] || (k < 2 && (!params->cam_s[k] || !params->cam_t[k])))
        return fail(LIST_ERR_ARG, "list_coarse_prep_weights: a camera array of layer %d is NULL", k);

  hipStream_t s = (hipStream_t)stream;
  int rc = LIST_OK;                    // of the first launch that failed; nothing is launched after it
  auto put = [&](const float* src, size_t off, int rows, int cols, int transpose) {
    if (rc == LIST_OK)
      rc = launch("list_coarse_prep_weights", coarse_pack_kernel, dim3(blocks_for((int64_t)rows * cols, kThreads)),
                  dim3(kThreads), s, src, at<float>(packed, off), rows, cols, transpose);
  };
  for (int l = 0; l < L; ++l) {
    const int out = S.features[l + 1];
    for (int i = 0; i <= l; ++i) put(params->w_root[l][i], P.root[l][i], out, S.features[i], 1);
    put(params->wc[l], P.wc[l], out, S.features[l], 1);
    if (S.activation[l]) put(params->bias[l], P.bias[l], S.degrees[l], out, 0);
  }
  if (S.has_mlp)
    for (int k = 0; k < 3; ++k) {
      const int in = mlp_width(k), out = mlp_width(k + 1);
      put(params->mlp_w[k], P.mlp_w[k], out, in, k > 0);
      put(params->mlp_b[k], P.mlp_b[k], 1, out, 0);
      put(params->mlp_s[k], P.mlp_s[k], 1, out, 0);
      put(params->mlp_t[k], P.mlp_t[k], 1, out, 0);
    }
  if (S.has_camera)
    for (int k = 0; k < 3; ++k) {
      put(params->cam_w[k], P.cam_w[k], cam_out(S, k), cam_in(S, k), 1);
      put(params->cam_b[k], P.cam_b[k], 1, cam_out(S, k), 0);
      if (k < 2) {
        put(params->cam_s[k], P.cam_s[k], 1, cam_out(S, k), 0);
        put(params->cam_t[k], P.cam_t[k], 1, cam_out(S, k), 0);
      }
    }
  return rc;
}

int list_coarse_forward_steps(const ListCoarseShape* shape, const ListCoarseIO* io, int32_t step_begin,
                              int32_t step_end, void* stream) {
  if (int rc = check_shape(shape)) return rc;
  if (!io) return fail(LIST_ERR_ARG, "list_coarse_forward: io is NULL");
  const ListCoarseShape& S = *shape;
  const ListCoarseIO& A = *io;
  if (int rc = check_batch(A.B)) return rc;
  if (!A.feat_g || !A.packed || !A.workspace || !A.pc)
    return fail(LIST_ERR_ARG, "list_coarse_forward: %s is NULL",
                !A.feat_g ? "feat_g" : !A.packed ? "packed" : !A.workspace ? "workspace" : "pc");
  const int L = S.n_degrees;
  for (int l = 0; l < L; ++l) {
    if (!A.w_branch[l]) return fail(LIST_ERR_ARG, "list_coarse_forward: w_branch[%d] is NULL", l);
    if (misaligned(A.w_branch[l], 16))
      return fail(LIST_ERR_ARG, "list_coarse_forward: w_branch[%d] is not 16-byte aligned", l);
  }
  if (A.coarse && !S.has_mlp) return fail(LIST_ERR_ARG, "list_coarse_forward: coarse asked for, the shape has no point MLP");
  const bool camera = A.trans_mat && A.feat_g2;
  if (camera && !S.has_camera)
    return fail(LIST_ERR_ARG, "list_coarse_forward: trans_mat asked for, the shape has no camera");
  if (camera && !A.coarse) return fail(LIST_ERR_ARG, "list_coarse_forward: trans_mat asked for without coarse");
  if (A.occ) {
    if (A.R < 1 || A.R > LIST_COARSE_MAX_R)
      return fail(LIST_ERR_SHAPE, "R = %d: must be in [1, %d]", A.R, LIST_COARSE_MAX_R);
    const float big = 3.4028234e38f;    // (comparisons: a NaN fails each of them)
    if (!(A.bb_extent > 0.f && A.bb_extent <= big && A.bb_min >= -big && A.bb_min <= big))
      return fail(LIST_ERR_ARG, "list_coarse_forward: bb_min = %g, bb_extent = %g: the box must be finite and not empty",
                  (double)A.bb_min, (double)A.bb_extent);
  }
  const PackedLayout P = packed_layout(S);
  const WorkspaceLayout W = workspace_layout(S, A.B);
  if (A.packed_bytes < P.total) return packed_too_small("list_coarse_forward", A.packed_bytes, P.total);
  if (A.workspace_bytes < W.total) return workspace_too_small(A.workspace_bytes, W.total, "list_coarse_workspace_bytes");
  if (int rc = check_step_range("list_coarse_forward_steps", step_begin, step_end, n_steps_of(S))) return rc;

  hipStream_t s = (hipStream_t)stream;
  const void* pk = A.packed;
  void* ws = A.workspace;
  auto f = [&](size_t off) { return at<float>(pk, off); };
  const int B = A.B;
  const int64_t Pn = nodes_of(S, L);
  const int tiles = (int)cdiv(Pn, kTile);
  float* tile_max = at<float>(ws, W.tile_max);
  const char* const name = "list_coarse_forward";      // a launch error is reported under the entry point's name

  for (int step = step_begin; step < step_end; ++step) {
    int rc = LIST_OK;
    if (step < L) {
      const int l = step;
      TreeArgs t = {};
      for (int i = 0; i <= l; ++i) {
        t.level[i] = i == 0 ? A.feat_g : at<float>(ws, W.level[i]);
        t.rootT[i] = f(P.root[l][i]);
        t.nodes[i] = (int32_t)nodes_of(S, i);
        t.feat[i] = S.features[i];
      }
      t.wcT = f(P.wc[l]);
      t.bias = S.activation[l] ? f(P.bias[l]) : nullptr;
      t.w_branch = A.w_branch[l];
      t.out = l == L - 1 ? A.pc : at<float>(ws, W.level[l + 1]);
      t.depth = l, t.node = (int32_t)nodes_of(S, l), t.in = S.features[l], t.out_f = S.features[l + 1];
      t.deg = S.degrees[l], t.B = B;
      rc = launch_tree(t, s);
    } else if (step == L) {
      if (!A.coarse) continue;
      MlpArgs m = {A.pc,
                   f(P.mlp_w[0]), f(P.mlp_b[0]), f(P.mlp_s[0]), f(P.mlp_t[0]),
                   f(P.mlp_w[1]), f(P.mlp_b[1]), f(P.mlp_s[1]), f(P.mlp_t[1]),
                   f(P.mlp_w[2]), f(P.mlp_b[2]), f(P.mlp_s[2]), f(P.mlp_t[2]),
                   tile_max, (int32_t)Pn, tiles};
      rc = launch(name, coarse_mlp_kernel, dim3((unsigned)tiles, (unsigned)B), dim3(kThreads), s, m);
    } else if (step == L + 1) {
      if (!A.coarse) continue;
      rc = launch(name, coarse_max_kernel, dim3((unsigned)B), dim3(kCode), s, tile_max, A.coarse, tiles);
    } else if (step == L + 2) {
      if (!camera) continue;
      CameraArgs c = {};
      c.coarse = A.coarse, c.feat_g2 = A.feat_g2;
      for (int k = 0; k < 3; ++k) c.wT[k] = f(P.cam_w[k]), c.b[k] = f(P.cam_b[k]);
      for (int k = 0; k < 2; ++k) c.s[k] = f(P.cam_s[k]), c.t[k] = f(P.cam_t[k]);
      c.trans_mat = A.trans_mat, c.g2 = S.g2, c.hidden = S.hidden;
      rc = launch(name, coarse_camera_kernel, dim3((unsigned)B), dim3(kThreads), s, c);
    } else if (step == L + 3) {
      if (!A.occ) continue;
      const int64_t n = (int64_t)B * A.R * A.R * A.R;
      // a tensor's storage is 16-byte aligned where an allocator made it; a view that is not is cleared by floats
      const int64_t n4 = misaligned(A.occ, 16) ? 0 : n / 4;
      const int64_t work = n4 > n - 4 * n4 ? n4 : n - 4 * n4;
      rc = launch(name, coarse_clear_kernel, dim3(blocks_for(work, kThreads)), dim3(kThreads), s, (float4*)A.occ, n4,
                  A.occ, n);
    } else {
      if (!A.occ) continue;
      const int64_t BP = (int64_t)B * Pn;
      rc = launch(name, coarse_mark_kernel, dim3(blocks_for(BP, kThreads)), dim3(kThreads), s, A.pc, A.occ, BP, (int)Pn,
                  (int)A.R, A.bb_min, A.bb_extent);
    }
    if (rc) return rc;
  }
  return LIST_OK;
}

int list_coarse_forward(const ListCoarseShape* shape, const ListCoarseIO* io, void* stream) {
  if (int rc = check_shape(shape)) return rc;
  return list_coarse_forward_steps(shape, io, 0, n_steps_of(*shape), stream);
}

}  // extern "C"
