// The 3-D occupancy encoder on the device (include/list_voxenc.h): VoxelEncoder2's inference forward, from the
// occupancy grid to the six feature volumes.
//
//   voxenc_stencil_kernel   3x3x3 convolution of a one-channel fp32 volume (stages 0 .. 2): an 8^3 tile and its halo
//                           in LDS, two voxels per thread; epilogue ReLU + BN or sigmoid, fp32 out.
//   voxenc_expand_kernel    the 1 -> C convolution of stage 3 from the same tile: 27 fp32 taps per output channel,
//                           ReLU, fp16 channels-last out.
//   voxenc_conv_kernel      every convolution with C_in >= 16: an implicit GEMM on v_mfma_f32_16x16x32_f16.  A
//                           workgroup owns a 4 x 4 x 8 brick of the output (M = 128 voxels, N = C_out); the 6 x 6 x 10
//                           halo of the input is staged in LDS once per chunk of 32 input channels and read for all 27
//                           taps; the B operand comes from the packed weights, whose layout is the MFMA's own lane
//                           order.  Epilogue bias + ReLU (+ BN), through LDS into 16-byte channels-last stores, and the
//                           2x2x2 max-pooled brick from the same LDS image.
//   voxenc_pack_kernel ...  the prep of list_voxenc_prep_weights.
// fp16 outputs are not saturated (a non-finite activation propagates).  No atomics: one writer per output element.
#include <hip/hip_runtime.h>

#include "list_host.h"
#include "list_voxenc.h"
#include "mfma_common.h"
#include "stage_prep.h"

namespace {

constexpr int kThreads = 256;
constexpr int kStages = LIST_VOXENC_N_LAYERS - 1;       // 8
constexpr int kTaps = 27;
constexpr int kTile = 8;                                // fp32 kernels: 8^3 outputs per workgroup
constexpr int kTileHalo = kTile + 2;
// brick of the MFMA kernel: z, y, x extents (x fastest), halo one voxel each side
constexpr int kBz = 4, kBy = 4, kBx = 8, kBrick = kBz * kBy * kBx;
constexpr int kHz = kBz + 2, kHy = kBy + 2, kHx = kBx + 2, kHalo = kHz * kHy * kHx;
constexpr int kPad = 8;                                 // halfs of padding per LDS row (16 B: rows stay aligned)

// ---- packed weights and workspace ------------------------------------------------------------------------------------
// K order of the MFMA convolutions.  C_in >= 32: chunks of 32 input channels, 27 taps per chunk, one MFMA (K = 32) per
// tap.  C_in == 16: one MFMA covers two taps (14 steps, the 28th tap is zeros).  A step's B operand is stored as
// [n-tile][lane][8 halfs]: lane l holds W[n = 16 nt + (l & 15)][k = 8 (l >> 4) + j].
int conv_steps(int cin) { return cin == 16 ? 14 : (cin / 32) * kTaps; }
size_t wpk_bytes(int cin, int cout) { return (size_t)conv_steps(cin) * (cout / 16) * 64 * 8 * 2; }

struct ConvSlot { size_t w, bias, s, t; };              // byte offsets into the packed blob
struct PackedLayout {
  ConvSlot conv[kStages], conv2[kStages];
  size_t total;
};

PackedLayout packed_layout(const int32_t* layers) {
  PackedLayout p;
  Carver c;
  for (int l = 0; l < kStages; ++l) {
    const int cin = layers[l], cout = layers[l + 1];
    p.conv[l].w = c.take(cin == 1 ? (size_t)cout * kTaps * 4 : wpk_bytes(cin, cout));
    p.conv[l].bias = c.take((size_t)cout * 4);
    p.conv[l].s = p.conv[l].t = 0;
    p.conv2[l] = ConvSlot{0, 0, 0, 0};
    if (l < 2) { p.conv[l].s = c.take((size_t)cout * 4); p.conv[l].t = c.take((size_t)cout * 4); }
    if (l >= 3) {
      p.conv2[l].w = c.take(wpk_bytes(cout, cout));
      p.conv2[l].bias = c.take((size_t)cout * 4);
      p.conv2[l].s = c.take((size_t)cout * 4);
      p.conv2[l].t = c.take((size_t)cout * 4);
    }
  }
  p.total = c.total();
  return p;
}

struct WorkspaceLayout { size_t t0, t1, mid, pooled[kStages], total; };

WorkspaceLayout workspace_layout(int B, int R, const int32_t* layers) {
  WorkspaceLayout w;
  Carver c;
  const size_t r3 = (size_t)R * R * R;
  w.t0 = c.take((size_t)B * r3 * 4);
  w.t1 = c.take((size_t)B * r3 * 4);
  size_t mid = 0;
  for (int l = 3; l < kStages; ++l) {
    const size_t D = (size_t)(R >> (l - 3));
    const size_t b = (size_t)B * D * D * D * layers[l + 1] * 2;
    if (b > mid) mid = b;
  }
  w.mid = c.take(mid);
  for (int l = 0; l < kStages; ++l) w.pooled[l] = 0;
  for (int l = 3; l < kStages - 1; ++l) {
    const size_t D = (size_t)(R >> (l - 2));
    w.pooled[l] = c.take((size_t)B * D * D * D * layers[l + 1] * 2);
  }
  w.total = c.total();
  return w;
}

bool mfma_channels(int c) { return c == 16 || c == 32 || c == 64 || c == 128; }

int check_layers(const int32_t* layers, int32_t n_layers) {
  if (!layers) return fail(LIST_ERR_ARG, "layers is NULL");
  if (n_layers != LIST_VOXENC_N_LAYERS)
    return fail(LIST_ERR_SHAPE, "n_layers = %d: the encoder has %d entries in its layer list", n_layers,
                LIST_VOXENC_N_LAYERS);
  for (int l = 0; l < 4; ++l)
    if (layers[l] != 1)
      return fail(LIST_ERR_SHAPE, "layers[%d] = %d: the first four entries must be 1", l, layers[l]);
  for (int l = 4; l < LIST_VOXENC_N_LAYERS; ++l)
    if (!mfma_channels(layers[l]))
      return fail(LIST_ERR_SHAPE,
                  "layers[%d] = %d: the matrix-core path takes channel counts of 16, 32, 64 or 128 (multiples of 16)",
                  l, layers[l]);
  return LIST_OK;
}

int check_grid(int32_t B, int32_t R) {
  if (B < 1 || B > 65535) return fail(LIST_ERR_SHAPE, "B = %d: must be in [1, 65535]", B);
  if (R < 16 || R % 16 != 0) return fail(LIST_ERR_SHAPE, "R = %d: must be a multiple of 16 (at least 16)", R);
  if (R > LIST_VOXENC_MAX_R) return fail(LIST_ERR_SHAPE, "R = %d: at most %d", R, LIST_VOXENC_MAX_R);
  return LIST_OK;
}

// ---- fp32 one-channel kernels ----------------------------------------------------------------------------------------
// the 10^3 tile (8^3 outputs and their halo) of image b, zeros outside the volume
__device__ __forceinline__ void load_tile(const float* __restrict__ in, int R, int z0, int y0, int x0,
                                          float (&tile)[kTileHalo][kTileHalo][kTileHalo]) {
  for (int i = threadIdx.x; i < kTileHalo * kTileHalo * kTileHalo; i += kThreads) {
    const int hx = i % kTileHalo, hy = (i / kTileHalo) % kTileHalo, hz = i / (kTileHalo * kTileHalo);
    const int z = z0 + hz - 1, y = y0 + hy - 1, x = x0 + hx - 1;
    const bool ok = (unsigned)z < (unsigned)R && (unsigned)y < (unsigned)R && (unsigned)x < (unsigned)R;
    tile[hz][hy][hx] = ok ? in[((int64_t)z * R + y) * R + x] : 0.f;
  }
}

__device__ __forceinline__ void tile_origin(int R, int& z0, int& y0, int& x0) {
  const int nt = R / kTile;
  const int id = blockIdx.x;
  x0 = (id % nt) * kTile;
  y0 = ((id / nt) % nt) * kTile;
  z0 = (id / (nt * nt)) * kTile;
}

// mode 0: ReLU then y * s + t; mode 1: sigmoid.  w: [27], bias / s / t: [1]
__global__ __launch_bounds__(kThreads) void voxenc_stencil_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                                   int R, const float* __restrict__ w,
                                                                   const float* __restrict__ bias,
                                                                   const float* __restrict__ s,
                                                                   const float* __restrict__ t, int mode) {
  __shared__ float tile[kTileHalo][kTileHalo][kTileHalo];
  int z0, y0, x0;
  tile_origin(R, z0, y0, x0);
  const int64_t img = (int64_t)blockIdx.y * R * R * R;
  load_tile(in + img, R, z0, y0, x0, tile);
  float wr[kTaps];
#pragma unroll
  for (int k = 0; k < kTaps; ++k) wr[k] = w[k];
  const float b = bias[0];
  const float sc = mode == 0 ? s[0] : 0.f, sh = mode == 0 ? t[0] : 0.f;
  __syncthreads();
#pragma unroll
  for (int v = 0; v < 2; ++v) {
    const int m = threadIdx.x + v * kThreads;
    const int dx = m & 7, dy = (m >> 3) & 7, dz = m >> 6;
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < kTaps; ++k) acc = fmaf(tile[dz + k / 9][dy + (k / 3) % 3][dx + k % 3], wr[k], acc);
    acc += b;
    float y;
    if (mode == 0) y = list::relu_nan(acc) * sc + sh;
    else y = 1.f / (1.f + expf(-acc));
    out[img + ((int64_t)(z0 + dz) * R + (y0 + dy)) * R + (x0 + dx)] = y;
  }
}

// 1 -> C (C % 8 == 0, C <= 128): w [C][27], bias [C]; out fp16 [B][R][R][R][C], ReLU
__global__ __launch_bounds__(kThreads) void voxenc_expand_kernel(const float* __restrict__ in,
                                                                  _Float16* __restrict__ out, int R, int C,
                                                                  const float* __restrict__ w,
                                                                  const float* __restrict__ bias) {
  __shared__ float tile[kTileHalo][kTileHalo][kTileHalo];
  __shared__ float ws[kTaps][128];
  __shared__ float bs[128];
  int z0, y0, x0;
  tile_origin(R, z0, y0, x0);
  const int64_t img = (int64_t)blockIdx.y * R * R * R;
  load_tile(in + img, R, z0, y0, x0, tile);
  for (int i = threadIdx.x; i < C * kTaps; i += kThreads) ws[i % kTaps][i / kTaps] = w[i];
  for (int i = threadIdx.x; i < C; i += kThreads) bs[i] = bias[i];
  __syncthreads();
#pragma unroll 1
  for (int v = 0; v < 2; ++v) {
    const int m = threadIdx.x + v * kThreads;
    const int dx = m & 7, dy = (m >> 3) & 7, dz = m >> 6;
    float x[kTaps];
#pragma unroll
    for (int k = 0; k < kTaps; ++k) x[k] = tile[dz + k / 9][dy + (k / 3) % 3][dx + k % 3];
    _Float16* o = out + (img + ((int64_t)(z0 + dz) * R + (y0 + dy)) * R + (x0 + dx)) * C;
    for (int c0 = 0; c0 < C; c0 += 8) {
      float acc[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] = 0.f;
#pragma unroll
      for (int k = 0; k < kTaps; ++k)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] = fmaf(x[k], ws[k][c0 + j], acc[j]);
      list::f16x8 h;
#pragma unroll
      for (int j = 0; j < 8; ++j) h[j] = (_Float16)list::relu_nan(acc[j] + bs[c0 + j]);
      *(list::f16x8*)(o + c0) = h;
    }
  }
}

// ---- the MFMA convolution --------------------------------------------------------------------------------------------
struct ConvArgs {
  const _Float16* in;        // [B][D][D][D][CIN]
  _Float16* out;             // [B][D][D][D][16 NT]
  _Float16* pooled;          // [B][D/2][D/2][D/2][16 NT] or null
  const list::f16x8* w;      // packed B operand
  const float* bias;
  const float* s;            // BN scale / shift, or null (ReLU only)
  const float* t;
  int D, CIN;
  int nbx, nby;              // bricks along x and y
};

__device__ __forceinline__ int tap_offset(int tap) {      // halo voxels from a brick voxel to its tap
  return ((tap / 9) * kHy + (tap / 3) % 3) * kHx + tap % 3;
}

template <int CC, int NT>
__global__ __launch_bounds__(kThreads) void voxenc_conv_kernel(ConvArgs a) {
  constexpr int COUT = 16 * NT;
  constexpr int STR = CC + kPad;                       // halfs per staged halo voxel
  constexpr int OSTR = COUT + kPad;                    // halfs per staged output voxel
  constexpr int kStage = kHalo * STR, kOut = kBrick * OSTR;
  __shared__ __attribute__((aligned(16))) _Float16 smem[kStage > kOut ? kStage : kOut];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 15, g = lane >> 4;
  const int D = a.D, CIN = a.CIN;
  const int bid = blockIdx.x;
  const int x0 = (bid % a.nbx) * kBx, y0 = ((bid / a.nbx) % a.nby) * kBy, z0 = (bid / (a.nbx * a.nby)) * kBz;
  const int64_t img = (int64_t)blockIdx.y * D * D * D;

  // m-tile 2 wave + i: the 16 voxels (z = wave, y = 2 i + (r >> 3), x = r & 7) of the brick
  int base[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) base[i] = ((wave * kHy + 2 * i + (r >> 3)) * kHx + (r & 7)) * STR;

  list::f32x4v acc[2][NT];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int n = 0; n < NT; ++n) acc[i][n] = list::f32x4v{0.f, 0.f, 0.f, 0.f};

  const list::f16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
  const list::f16x8* wl = a.w + lane;

  for (int c0 = 0; c0 < CIN; c0 += CC) {
    if (c0) __syncthreads();
    constexpr int VPV = CC / 8;                        // 16-byte vectors per halo voxel
    for (int i = tid; i < kHalo * VPV; i += kThreads) {
      const int hv = i / VPV, v = i % VPV;
      const int hx = hv % kHx, hy = (hv / kHx) % kHy, hz = hv / (kHx * kHy);
      const int z = z0 + hz - 1, y = y0 + hy - 1, x = x0 + hx - 1;
      const bool ok = (unsigned)z < (unsigned)D && (unsigned)y < (unsigned)D && (unsigned)x < (unsigned)D;
      list::f16x8 val = zero8;
      if (ok) val = *(const list::f16x8*)(a.in + (img + ((int64_t)z * D + y) * D + x) * CIN + c0 + v * 8);
      *(list::f16x8*)(smem + hv * STR + v * 8) = val;
    }
    __syncthreads();
    if (CC == 32) {
      const list::f16x8* wc = wl + (size_t)(c0 / 32) * kTaps * NT * 64;
#pragma unroll 1
      for (int tz = 0; tz < 3; ++tz) {
#pragma unroll
        for (int q = 0; q < 9; ++q) {
          const int tap = tz * 9 + q;
          const int off = tap_offset(tap) * STR + g * 8;
          const list::f16x8 a0 = *(const list::f16x8*)(smem + base[0] + off);
          const list::f16x8 a1 = *(const list::f16x8*)(smem + base[1] + off);
#pragma unroll
          for (int n = 0; n < NT; ++n) {
            const list::f16x8 b = wc[(size_t)(tap * NT + n) * 64];
            acc[0][n] = list::mfma16<1>(__builtin_bit_cast(list::bf16x8, a0), __builtin_bit_cast(list::bf16x8, b),
                                        acc[0][n]);
            acc[1][n] = list::mfma16<1>(__builtin_bit_cast(list::bf16x8, a1), __builtin_bit_cast(list::bf16x8, b),
                                        acc[1][n]);
          }
        }
      }
    } else {
      // CIN == 16: lanes 0 .. 31 take tap 2 p, lanes 32 .. 63 tap 2 p + 1, 8 channels each; tap 27 is zeros
#pragma unroll
      for (int p = 0; p < 14; ++p) {
        const int tap = 2 * p + (g >> 1);
        const bool live = tap < kTaps;
        const int off = tap_offset(live ? tap : 0) * STR + (g & 1) * 8;
        list::f16x8 a0 = *(const list::f16x8*)(smem + base[0] + off);
        list::f16x8 a1 = *(const list::f16x8*)(smem + base[1] + off);
        if (!live) { a0 = zero8; a1 = zero8; }
#pragma unroll
        for (int n = 0; n < NT; ++n) {
          const list::f16x8 b = wl[(size_t)(p * NT + n) * 64];
          acc[0][n] = list::mfma16<1>(__builtin_bit_cast(list::bf16x8, a0), __builtin_bit_cast(list::bf16x8, b),
                                      acc[0][n]);
          acc[1][n] = list::mfma16<1>(__builtin_bit_cast(list::bf16x8, a1), __builtin_bit_cast(list::bf16x8, b),
                                      acc[1][n]);
        }
      }
    }
  }

  // epilogue: accumulator (column = lane & 15, row = 4 (lane >> 4) + e) -> fp16 rows of the brick in LDS
  __syncthreads();
  const bool bn = a.s != nullptr;
#pragma unroll
  for (int n = 0; n < NT; ++n) {
    const int ch = n * 16 + r;
    const float bias = a.bias[ch];
    const float sc = bn ? a.s[ch] : 1.f, sh = bn ? a.t[ch] : 0.f;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int m = (2 * wave + i) * 16 + g * 4 + e;
        float v = list::relu_nan(acc[i][n][e] + bias);
        if (bn) v = v * sc + sh;
        smem[m * OSTR + ch] = (_Float16)v;
      }
  }
  __syncthreads();
  constexpr int VPO = COUT / 8;
  for (int i = tid; i < kBrick * VPO; i += kThreads) {
    const int m = i / VPO, v = i % VPO;
    const int z = z0 + (m >> 5), y = y0 + ((m >> 3) & 3), x = x0 + (m & 7);
    if (z < D && y < D && x < D)
      *(list::f16x8*)(a.out + (img + ((int64_t)z * D + y) * D + x) * COUT + v * 8) =
          *(const list::f16x8*)(smem + m * OSTR + v * 8);
  }
  if (a.pooled) {
    const int Dp = D / 2;
    const int64_t imgp = (int64_t)blockIdx.y * Dp * Dp * Dp;
    for (int i = tid; i < (kBrick / 8) * VPO; i += kThreads) {
      const int pm = i / VPO, v = i % VPO;
      const int pz = pm >> 3, py = (pm >> 2) & 1, px = pm & 3;
      const int z = z0 / 2 + pz, y = y0 / 2 + py, x = x0 / 2 + px;
      if (z >= Dp || y >= Dp || x >= Dp) continue;
      list::f16x8 best;
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        const int m = ((2 * pz + (c >> 2)) * kBy + 2 * py + ((c >> 1) & 1)) * kBx + 2 * px + (c & 1);
        const list::f16x8 val = *(const list::f16x8*)(smem + m * OSTR + v * 8);
        if (c == 0) best = val;
        else
#pragma unroll
          for (int j = 0; j < 8; ++j) best[j] = (val[j] > best[j] || val[j] != val[j]) ? val[j] : best[j];
      }
      *(list::f16x8*)(a.pooled + (imgp + ((int64_t)z * Dp + y) * Dp + x) * COUT + v * 8) = best;
    }
  }
}

// (a launch error of the forward is reported under the entry point's name, not the kernel's)
template <int CC>
int launch_conv_nt(const ConvArgs& a, int cout, dim3 grid, hipStream_t s) {
  auto run = [&](auto kernel) { return launch("list_voxenc_forward", kernel, grid, dim3(kThreads), s, a); };
  switch (cout) {
    case 16: return run(voxenc_conv_kernel<CC, 1>);
    case 32: return run(voxenc_conv_kernel<CC, 2>);
    case 64: return run(voxenc_conv_kernel<CC, 4>);
    default: return run(voxenc_conv_kernel<CC, 8>);
  }
}

int launch_conv(ConvArgs a, int B, int cout, hipStream_t s) {
  a.nbx = (a.D + kBx - 1) / kBx;
  a.nby = (a.D + kBy - 1) / kBy;
  const int nbz = (a.D + kBz - 1) / kBz;
  const dim3 grid((unsigned)(a.nbx * a.nby * nbz), (unsigned)B);
  return a.CIN == 16 ? launch_conv_nt<16>(a, cout, grid, s) : launch_conv_nt<32>(a, cout, grid, s);
}

// ---- prep ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void voxenc_pack_kernel(const float* __restrict__ w, int cin, int cout,
                                                                _Float16* __restrict__ out, int total) {
  const int idx = blockIdx.x * kThreads + threadIdx.x;
  if (idx >= total) return;
  const int j = idx & 7, lane = (idx >> 3) & 63, rest = idx >> 9;
  const int nt_count = cout / 16;
  const int nt = rest % nt_count, step = rest / nt_count;
  const int g = lane >> 4, n = nt * 16 + (lane & 15);
  int tap, c;
  if (cin == 16) { tap = 2 * step + (g >> 1); c = 8 * (g & 1) + j; }
  else { tap = step % kTaps; c = (step / kTaps) * 32 + 8 * g + j; }
  out[idx] = tap < kTaps ? (_Float16)w[((int64_t)n * cin + c) * kTaps + tap] : (_Float16)0.f;
}

__global__ __launch_bounds__(kThreads) void voxenc_copy_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                                int n) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i < n) out[i] = in[i];
}

}  // namespace

extern "C" {

const char* list_voxenc_last_error(void) { return g_err; }

size_t list_voxenc_weight_bytes(const int32_t* layers, int32_t n_layers) {
  if (check_layers(layers, n_layers) != LIST_OK) return 0;
  return packed_layout(layers).total;
}

size_t list_voxenc_workspace_bytes(int32_t B, int32_t R, const int32_t* layers, int32_t n_layers) {
  if (check_layers(layers, n_layers) != LIST_OK || check_grid(B, R) != LIST_OK) return 0;
  return workspace_layout(B, R, layers).total;
}

int32_t list_voxenc_n_steps(const int32_t* layers, int32_t n_layers) {
  if (check_layers(layers, n_layers) != LIST_OK) return 0;
  return 3 + 2 * (kStages - 3);
}

int list_voxenc_prep_weights(const ListVoxencStage* stages, const int32_t* layers, int32_t n_layers, void* packed,
                             size_t packed_bytes, void* stream) {
  if (int rc = check_layers(layers, n_layers)) return rc;
  if (!stages || !packed) return fail(LIST_ERR_ARG, "list_voxenc_prep_weights: %s is NULL", stages ? "packed" : "stages");
  const PackedLayout P = packed_layout(layers);
  if (packed_bytes < P.total) return packed_too_small("list_voxenc_prep_weights", packed_bytes, P.total);
  for (int l = 0; l < kStages; ++l) {
    const ListVoxencStage& st = stages[l];
    if (!st.conv_w || !st.conv_b) return fail(LIST_ERR_ARG, "list_voxenc_prep_weights: stage %d: conv_w or conv_b is NULL", l);
    if (l >= 3 && (!st.conv2_w || !st.conv2_b))
      return fail(LIST_ERR_ARG, "list_voxenc_prep_weights: stage %d: conv2_w or conv2_b is NULL", l);
    if (l != 2 && (!st.bn_weight || !st.bn_bias || !st.bn_mean || !st.bn_var))
      return fail(LIST_ERR_ARG, "list_voxenc_prep_weights: stage %d: a BN array is NULL", l);
  }
  hipStream_t s = (hipStream_t)stream;
  const char* const name = "list_voxenc_prep_weights";      // a launch error is reported under the entry point's name
  auto copy = [&](const float* src, size_t off, int n) {
    return launch(name, voxenc_copy_kernel, dim3(blocks_for(n, kThreads)), dim3(kThreads), s, src,
                  at<float>(packed, off), n);
  };
  auto pack = [&](const float* src, int cin, int cout, size_t off) {
    const int total = (int)(wpk_bytes(cin, cout) / 2);
    return launch(name, voxenc_pack_kernel, dim3(blocks_for(total, kThreads)), dim3(kThreads), s, src, cin, cout,
                  at<_Float16>(packed, off), total);
  };
  for (int l = 0; l < kStages; ++l) {
    const ListVoxencStage& st = stages[l];
    const int cin = layers[l], cout = layers[l + 1];
    if (int rc = cin == 1 ? copy(st.conv_w, P.conv[l].w, cout * kTaps) : pack(st.conv_w, cin, cout, P.conv[l].w))
      return rc;
    if (int rc = copy(st.conv_b, P.conv[l].bias, cout)) return rc;
    const ConvSlot* bn_slot = l < 2 ? &P.conv[l] : nullptr;
    if (l >= 3) {
      if (int rc = pack(st.conv2_w, cout, cout, P.conv2[l].w)) return rc;
      if (int rc = copy(st.conv2_b, P.conv2[l].bias, cout)) return rc;
      bn_slot = &P.conv2[l];
    }
    if (!bn_slot) continue;
    list::launch_bn_fold(st.bn_weight, st.bn_bias, st.bn_mean, st.bn_var, st.bn_eps, cout, at<float>(packed, bn_slot->s),
                         at<float>(packed, bn_slot->t), s);
    if (int rc = launched(name)) return rc;
  }
  return LIST_OK;
}

int list_voxenc_forward_steps(const float* occ, int32_t B, int32_t R, const int32_t* layers, int32_t n_layers,
                              const void* packed, size_t packed_bytes, void* workspace, size_t workspace_bytes,
                              void* const* levels_out, int32_t step_begin, int32_t step_end, void* stream) {
  if (int rc = check_layers(layers, n_layers)) return rc;
  if (int rc = check_grid(B, R)) return rc;
  if (!occ || !packed || !workspace || !levels_out)
    return fail(LIST_ERR_ARG, "list_voxenc_forward: %s is NULL",
                !occ ? "occ" : !packed ? "packed" : !workspace ? "workspace" : "levels_out");
  for (int k = 0; k < LIST_VOXENC_N_LEVELS; ++k)
    if (!levels_out[k]) return fail(LIST_ERR_ARG, "list_voxenc_forward: levels_out[%d] is NULL", k);
  const PackedLayout P = packed_layout(layers);
  const WorkspaceLayout W = workspace_layout(B, R, layers);
  if (packed_bytes < P.total) return packed_too_small("list_voxenc_forward", packed_bytes, P.total);
  if (workspace_bytes < W.total) return workspace_too_small(workspace_bytes, W.total, "list_voxenc_workspace_bytes");
  if (int rc = check_step_range("list_voxenc_forward_steps", step_begin, step_end, 3 + 2 * (kStages - 3))) return rc;

  hipStream_t s = (hipStream_t)stream;
  float* t0 = at<float>(workspace, W.t0);
  float* t1 = at<float>(workspace, W.t1);
  _Float16* mid = at<_Float16>(workspace, W.mid);
  auto f = [&](size_t off) { return at<float>(packed, off); };
  const dim3 tiles((unsigned)((R / kTile) * (R / kTile) * (R / kTile)), (unsigned)B);
  const char* const name = "list_voxenc_forward";      // a launch error is reported under the entry point's name

  for (int step = step_begin; step < step_end; ++step) {
    int rc;
    if (step < 3) {                                     // stages 0 .. 2, one channel
      const float* in = step == 0 ? occ : step == 1 ? t0 : t1;
      float* out = step == 0 ? t0 : step == 1 ? t1 : (float*)levels_out[0];
      const ConvSlot& c = P.conv[step];
      rc = launch(name, voxenc_stencil_kernel, tiles, dim3(kThreads), s, in, out, (int)R, f(c.w), f(c.bias),
                  step < 2 ? f(c.s) : nullptr, step < 2 ? f(c.t) : nullptr, step < 2 ? 0 : 1);
    } else {
      const int l = 3 + (step - 3) / 2;
      const bool second = (step - 3) % 2 == 1;
      const int D = R >> (l - 3);
      const int cin = layers[l], cout = layers[l + 1];
      if (!second && l == 3) {
        rc = launch(name, voxenc_expand_kernel, tiles, dim3(kThreads), s, (const float*)levels_out[0], mid, (int)R, cout,
                    f(P.conv[3].w), f(P.conv[3].bias));
      } else {
        ConvArgs a;
        a.D = D;
        if (!second) {
          a.in = at<_Float16>(workspace, W.pooled[l - 1]);
          a.out = mid;
          a.pooled = nullptr;
          a.w = at<list::f16x8>(packed, P.conv[l].w);
          a.bias = f(P.conv[l].bias);
          a.s = a.t = nullptr;
          a.CIN = cin;
        } else {
          a.in = mid;
          a.out = (_Float16*)levels_out[l - 2];
          a.pooled = l < kStages - 1 ? at<_Float16>(workspace, W.pooled[l]) : nullptr;
          a.w = at<list::f16x8>(packed, P.conv2[l].w);
          a.bias = f(P.conv2[l].bias);
          a.s = f(P.conv2[l].s);
          a.t = f(P.conv2[l].t);
          a.CIN = cout;
        }
        rc = launch_conv(a, B, cout, s);
      }
    }
    if (rc) return rc;
  }
  return LIST_OK;
}

int list_voxenc_forward(const float* occ, int32_t B, int32_t R, const int32_t* layers, int32_t n_layers,
                        const void* packed, size_t packed_bytes, void* workspace, size_t workspace_bytes,
                        void* const* levels_out, void* stream) {
  return list_voxenc_forward_steps(occ, B, R, layers, n_layers, packed, packed_bytes, workspace, workspace_bytes,
                                   levels_out, 0, 3 + 2 * (kStages - 3), stream);
}

}  // extern "C"
