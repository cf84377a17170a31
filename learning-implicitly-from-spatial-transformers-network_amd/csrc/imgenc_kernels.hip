// The image encoder on the device (include/list_imgenc.h): ResEncoder's inference forward, from the image to the global
// vector and the five feature maps.
//
//   imgenc_stem_kernel   the 7x7 stem in fp32 on the VALU: a 16 x 16 tile of pixels and its halo in LDS, one pixel and
//                        all 64 output channels per thread, the weights [147][64] read wave-uniformly; BN + ReLU,
//                        fp32 level 0 and its fp16 copy.
//   imgenc_pool_kernel   3x3 stride-2 max-pool of the fp16 copy of level 0 (a NaN wins; padding never wins).
//   imgenc_conv_kernel   every other convolution (3x3 stride 1 or 2, 1x1 stride 2): an implicit GEMM on
//                        v_mfma_f32_16x16x32_f16.  A workgroup owns an 8 x 16 tile of output pixels (M = 128) and
//                        16 NT output channels; the halo of the input tile is staged in LDS once per chunk of 32 input
//                        channels and read for all taps; the B operand comes from the packed weights, whose layout is
//                        the MFMA's own lane order.  Epilogue acc * s + t through LDS in fp32, then per 16-byte
//                        channels-last row: plus the identity, ReLU, the fp16 activation and (for a level) the fp32 map.
//   imgenc_head_kernel   mean of level 4 (four interleaved partial sums per channel, in a fixed order), the composed
//                        fc1 o fc, one workgroup per image.
//   imgenc_pack_kernel ...  the prep of list_imgenc_prep_weights.
// fp16 outputs are not saturated (a non-finite activation propagates).  No atomics: one writer per output element, and
// the order of every sum is fixed by the shapes alone.
#include <hip/hip_runtime.h>

#include "list_host.h"
#include "list_imgenc.h"
#include "mfma_common.h"
#include "stage_prep.h"

namespace {

constexpr int kThreads = 256;
constexpr int kLevels = LIST_IMGENC_N_LEVELS;
constexpr int kConvs = LIST_IMGENC_N_CONVS;
constexpr int kSteps = 22;                              // stem, pool, 19 convolutions, head
constexpr int kStemK = 147, kStemC = 64, kStemTile = 16, kStemHalo = kStemTile + 6;
constexpr int kTy = 8, kTx = 16, kTilePix = kTy * kTx;  // output tile of the MFMA kernel (x fastest)
constexpr int kCC = 32;                                 // input channels per K chunk: one MFMA (K = 32) per tap
constexpr int kPad = 8;                                 // halfs of padding per staged halo pixel (16 B: rows stay aligned)
constexpr int kFPad = 4;                                // floats of padding per staged output pixel
constexpr int kVec = LIST_IMGENC_VEC, kFc = LIST_IMGENC_FC, kC4 = 512;
constexpr int64_t kMaxPixels = (int64_t)1 << 28;        // B * H * W: keeps every grid and 32-bit tile index in range

// ---- the fixed network as a table of launches ---------------------------------------------------------------------------
enum Kind { STEM, POOL, CONV, HEAD };
struct Step {
  Kind kind;
  int cin, cout, ks, stride;
  int shift_out;             // the output is (H >> shift_out) x (W >> shift_out)
  int in, idt;               // workspace activation (by the step that wrote it) read as input / identity; -1: none
  int level;                 // index of the fp32 level written beside the fp16 activation; -1: none
  int relu;
  int conv;                  // index into ListImgencParams.conv / the packed slots
};

struct Net { Step s[kSteps]; };

Net make_net() {
  Net n;
  int k = 0;
  n.s[k++] = Step{STEM, 3, 64, 7, 1, 0, -1, -1, 0, 1, 0};
  n.s[k++] = Step{POOL, 64, 64, 3, 2, 1, 0, -1, -1, 0, -1};
  n.s[k++] = Step{CONV, 64, 64, 3, 1, 1, 1, -1, -1, 1, 1};
  n.s[k++] = Step{CONV, 64, 64, 3, 1, 1, 2, 1, -1, 1, 2};
  n.s[k++] = Step{CONV, 64, 64, 3, 1, 1, 3, -1, -1, 1, 3};
  n.s[k++] = Step{CONV, 64, 64, 3, 1, 1, 4, 3, 1, 1, 4};
  for (int L = 2; L <= 4; ++L) {
    const int b = k, cin = 32 << (L - 1), cout = 2 * cin;
    n.s[k++] = Step{CONV, cin, cout, 3, 2, L, b - 1, -1, -1, 1, b - 1};
    n.s[k++] = Step{CONV, cin, cout, 1, 2, L, b - 1, -1, -1, 0, b};
    n.s[k++] = Step{CONV, cout, cout, 3, 1, L, b, b + 1, -1, 1, b + 1};
    n.s[k++] = Step{CONV, cout, cout, 3, 1, L, b + 2, -1, -1, 1, b + 2};
    n.s[k++] = Step{CONV, cout, cout, 3, 1, L, b + 3, b + 2, L, 1, b + 3};
  }
  n.s[k++] = Step{HEAD, kC4, kVec, 1, 1, 4, -1, -1, -1, 0, -1};
  return n;
}

// ---- packed weights and workspace ------------------------------------------------------------------------------------
// A convolution's B operand: [chunk of 32 input channels][tap][n-tile of 16 output channels][lane][8 halfs]; lane l holds
// W[n = 16 nt + (l & 15)][c = 32 chunk + 8 (l >> 4) + j][tap].
size_t wpk_bytes(const Step& s) { return (size_t)s.cin * s.ks * s.ks * s.cout * 2; }

struct ConvSlot { size_t w, s, t; };
struct PackedLayout { ConvSlot conv[kConvs]; size_t head_w, head_b, total; };

PackedLayout packed_layout(const Net& n) {
  PackedLayout p;
  Carver c;
  for (int k = 0; k < kSteps; ++k) {
    const Step& s = n.s[k];
    if (s.conv < 0) continue;
    p.conv[s.conv].w = c.take(s.kind == STEM ? (size_t)kStemK * kStemC * 4 : wpk_bytes(s));
    p.conv[s.conv].s = c.take((size_t)s.cout * 4);
    p.conv[s.conv].t = c.take((size_t)s.cout * 4);
  }
  p.head_w = c.take((size_t)kC4 * kVec * 4);
  p.head_b = c.take((size_t)kVec * 4);
  p.total = c.total();
  return p;
}

// one fp16 channels-last activation per launch but the head, in launch order
struct WorkspaceLayout { size_t act[kSteps]; size_t total; };

WorkspaceLayout workspace_layout(const Net& n, int B, int H, int W) {
  WorkspaceLayout w;
  Carver c;
  for (int k = 0; k < kSteps; ++k) {
    const Step& s = n.s[k];
    w.act[k] = 0;
    if (s.kind != HEAD) w.act[k] = c.take((size_t)B * (H >> s.shift_out) * (W >> s.shift_out) * s.cout * 2);
  }
  w.total = c.total();
  return w;
}

int check_side(const char* name, int32_t v) {
  if (v % 16 != 0) return fail(LIST_ERR_SHAPE, "%s = %d: must be a multiple of 16", name, v);
  if (v < LIST_IMGENC_MIN_HW || v > LIST_IMGENC_MAX_HW)
    return fail(LIST_ERR_SHAPE, "%s = %d: must be in [%d, %d]", name, v, LIST_IMGENC_MIN_HW, LIST_IMGENC_MAX_HW);
  return LIST_OK;
}

int check_shape(int32_t B, int32_t H, int32_t W) {
  if (B < 1 || B > 65535) return fail(LIST_ERR_SHAPE, "B = %d: must be in [1, 65535]", B);
  if (int rc = check_side("H", H)) return rc;
  if (int rc = check_side("W", W)) return rc;
  if ((int64_t)B * H * W > kMaxPixels)
    return fail(LIST_ERR_SHAPE, "B * H * W = %lld pixels: at most %lld per call", (long long)B * H * W,
                (long long)kMaxPixels);
  return LIST_OK;
}

// ---- stem ------------------------------------------------------------------------------------------------------------
// w: [147][64], k = (c * 7 + ky) * 7 + kx; H and W are multiples of the tile
__global__ __launch_bounds__(kThreads) void imgenc_stem_kernel(const float* __restrict__ img, int64_t sb, int64_t sc,
                                                                int64_t sh, int64_t sw, int H, int W,
                                                                const float* __restrict__ w,
                                                                const float* __restrict__ s,
                                                                const float* __restrict__ t, float* __restrict__ level,
                                                                _Float16* __restrict__ act) {
  __shared__ float tile[3][kStemHalo][kStemHalo + 1];
  const int ntx = W / kStemTile;
  const int x0 = (blockIdx.x % ntx) * kStemTile, y0 = (blockIdx.x / ntx) * kStemTile;
  const int b = blockIdx.y;
  for (int i = threadIdx.x; i < 3 * kStemHalo * kStemHalo; i += kThreads) {
    const int hx = i % kStemHalo, hy = (i / kStemHalo) % kStemHalo, c = i / (kStemHalo * kStemHalo);
    const int y = y0 + hy - 3, x = x0 + hx - 3;
    const bool ok = (unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W;
    tile[c][hy][hx] = ok ? img[b * sb + c * sc + y * sh + x * sw] : 0.f;
  }
  __syncthreads();
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  list::f32x2_t acc2[kStemC / 2];                      // pairs of output channels: v_pk_fma_f32
#pragma unroll
  for (int n = 0; n < kStemC / 2; ++n) acc2[n] = list::f32x2_t{0.f, 0.f};
#pragma unroll 1
  for (int cy = 0; cy < 21; ++cy) {                    // (c, ky)
    const int c = cy / 7, ky = cy % 7;
    const float* wk = w + cy * 7 * kStemC;
#pragma unroll
    for (int kx = 0; kx < 7; ++kx) {
      const float x = tile[c][ty + ky][tx + kx];
      const list::f32x2_t xx = {x, x};
#pragma unroll
      for (int n = 0; n < kStemC / 2; ++n) {
        const list::f32x2_t ww = {wk[kx * kStemC + 2 * n], wk[kx * kStemC + 2 * n + 1]};
        acc2[n] = __builtin_elementwise_fma(xx, ww, acc2[n]);
      }
    }
  }
  float acc[kStemC];
#pragma unroll
  for (int n = 0; n < kStemC / 2; ++n) { acc[2 * n] = acc2[n][0]; acc[2 * n + 1] = acc2[n][1]; }
  const int64_t o = (((int64_t)b * H + (y0 + ty)) * W + (x0 + tx)) * kStemC;
#pragma unroll
  for (int v = 0; v < kStemC / 8; ++v) {
    float r[8];
    list::f16x8 h;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      r[j] = list::relu_nan(acc[v * 8 + j] * s[v * 8 + j] + t[v * 8 + j]);
      h[j] = (_Float16)r[j];
    }
    *(float4*)(level + o + v * 8) = make_float4(r[0], r[1], r[2], r[3]);
    *(float4*)(level + o + v * 8 + 4) = make_float4(r[4], r[5], r[6], r[7]);
    *(list::f16x8*)(act + o + v * 8) = h;
  }
}

// ---- max-pool 3x3, stride 2, pad 1 (C = 64) ---------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void imgenc_pool_kernel(const _Float16* __restrict__ in,
                                                                _Float16* __restrict__ out, int Hi, int Wi,
                                                                int64_t total) {
  const int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x;       // (b, y, x, 8-channel group)
  if (idx >= total) return;
  const int Ho = Hi / 2, Wo = Wi / 2;
  const int v = (int)(idx & 7);
  const int64_t pix = idx >> 3;
  const int x = (int)(pix % Wo), y = (int)((pix / Wo) % Ho);
  const int64_t b = pix / ((int64_t)Wo * Ho);
  list::f16x8 best;
  bool first = true;
#pragma unroll
  for (int dy = 0; dy < 3; ++dy)
#pragma unroll
    for (int dx = 0; dx < 3; ++dx) {
      const int yy = 2 * y - 1 + dy, xx = 2 * x - 1 + dx;
      if ((unsigned)yy >= (unsigned)Hi || (unsigned)xx >= (unsigned)Wi) continue;
      const list::f16x8 val = *(const list::f16x8*)(in + ((b * Hi + yy) * Wi + xx) * 64 + v * 8);
      if (first) { best = val; first = false; }
      else
#pragma unroll
        for (int j = 0; j < 8; ++j) best[j] = (val[j] > best[j] || val[j] != val[j]) ? val[j] : best[j];
    }
  *(list::f16x8*)(out + pix * 64 + v * 8) = best;
}

// ---- the MFMA convolution --------------------------------------------------------------------------------------------
struct ConvArgs {
  const _Float16* in;        // [B][Hi][Wi][CIN]
  const _Float16* idt;       // [B][Ho][Wo][COUT] or null
  _Float16* out;             // [B][Ho][Wo][COUT]
  float* level;              // fp32 [B][Ho][Wo][COUT] or null
  const list::f16x8* w;      // packed B operand
  const float* s;
  const float* t;
  int Hi, Wi, Ho, Wo, CIN, COUT, relu;
  int ntx;                   // tiles along x
};

template <int S, int KS, int NT>
__global__ __launch_bounds__(kThreads) void imgenc_conv_kernel(ConvArgs a) {
  constexpr int TAPS = KS * KS, PADK = KS / 2;
  constexpr int HY = (kTy - 1) * S + KS, HX = (kTx - 1) * S + KS;      // halo of the tile
  constexpr int STR = kCC + kPad;                                      // halfs per staged halo pixel
  constexpr int NW = 16 * NT;                                          // output channels of the workgroup
  constexpr int OSTR = NW + kFPad;                                     // floats per staged output pixel
  constexpr int kStage = HY * HX * STR * 2, kOut = kTilePix * OSTR * 4;
  __shared__ __attribute__((aligned(16))) char smem_raw[kStage > kOut ? kStage : kOut];
  _Float16* smem = (_Float16*)smem_raw;
  float* smf = (float*)smem_raw;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 15, g = lane >> 4;
  const int Hi = a.Hi, Wi = a.Wi, Ho = a.Ho, Wo = a.Wo, CIN = a.CIN, COUT = a.COUT;
  const int x0 = (blockIdx.x % a.ntx) * kTx, y0 = (blockIdx.x / a.ntx) * kTy;
  const int nt0 = blockIdx.y * NT;                                     // first n-tile of the workgroup
  const int ntiles = COUT / 16;
  const int64_t b = blockIdx.z;
  const _Float16* in = a.in + b * Hi * Wi * CIN;

  // m-tile 2 wave + i: the 16 pixels of tile row 2 wave + i
  int base[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) base[i] = (((2 * wave + i) * S) * HX + r * S) * STR + g * 8;

  list::f32x4v acc[2][NT];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int n = 0; n < NT; ++n) acc[i][n] = list::f32x4v{0.f, 0.f, 0.f, 0.f};

  const list::f16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
  const list::f16x8* wl = a.w + (size_t)nt0 * 64 + lane;

  for (int c0 = 0; c0 < CIN; c0 += kCC) {
    if (c0) __syncthreads();
    constexpr int VPV = kCC / 8;                       // 16-byte vectors per halo pixel
    for (int i = tid; i < HY * HX * VPV; i += kThreads) {
      const int hv = i / VPV, v = i % VPV;
      const int hx = hv % HX, hy = hv / HX;
      const int y = y0 * S - PADK + hy, x = x0 * S - PADK + hx;
      const bool ok = (unsigned)y < (unsigned)Hi && (unsigned)x < (unsigned)Wi;
      list::f16x8 val = zero8;
      if (ok) val = *(const list::f16x8*)(in + ((int64_t)y * Wi + x) * CIN + c0 + v * 8);
      *(list::f16x8*)(smem + hv * STR + v * 8) = val;
    }
    __syncthreads();
    const list::f16x8* wc = wl + (size_t)(c0 / kCC) * TAPS * ntiles * 64;
#pragma unroll
    for (int tap = 0; tap < TAPS; ++tap) {
      const int off = ((tap / KS) * HX + tap % KS) * STR;
      const list::f16x8 a0 = *(const list::f16x8*)(smem + base[0] + off);
      const list::f16x8 a1 = *(const list::f16x8*)(smem + base[1] + off);
#pragma unroll
      for (int n = 0; n < NT; ++n) {
        const list::f16x8 bw = wc[(size_t)(tap * ntiles + n) * 64];
        acc[0][n] = list::mfma16<1>(__builtin_bit_cast(list::bf16x8, a0), __builtin_bit_cast(list::bf16x8, bw),
                                    acc[0][n]);
        acc[1][n] = list::mfma16<1>(__builtin_bit_cast(list::bf16x8, a1), __builtin_bit_cast(list::bf16x8, bw),
                                    acc[1][n]);
      }
    }
  }

  // epilogue: accumulator (column = lane & 15, row = 4 (lane >> 4) + e) -> acc * s + t as fp32 rows of the tile in LDS
  __syncthreads();
#pragma unroll
  for (int n = 0; n < NT; ++n) {
    const int ch = (nt0 + n) * 16 + r;
    const float sc = a.s[ch], sh = a.t[ch];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int m = (2 * wave + i) * 16 + g * 4 + e;
        smf[m * OSTR + n * 16 + r] = acc[i][n][e] * sc + sh;
      }
  }
  __syncthreads();
  // per 8 channels of a pixel: + identity, ReLU, the fp16 activation and the fp32 level; pixels outside the map are not stored
  constexpr int VPO = NW / 8;
  for (int i = tid; i < kTilePix * VPO; i += kThreads) {
    const int m = i / VPO, v = i % VPO;
    const int y = y0 + (m >> 4), x = x0 + (m & 15);
    if (y >= Ho || x >= Wo) continue;
    const float4 lo = *(const float4*)(smf + m * OSTR + v * 8), hi = *(const float4*)(smf + m * OSTR + v * 8 + 4);
    float val[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    const int64_t o = ((b * Ho + y) * Wo + x) * COUT + nt0 * 16 + v * 8;
    if (a.idt) {
      const list::f16x8 id = *(const list::f16x8*)(a.idt + o);
#pragma unroll
      for (int j = 0; j < 8; ++j) val[j] += (float)id[j];
    }
    list::f16x8 h;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if (a.relu) val[j] = list::relu_nan(val[j]);
      h[j] = (_Float16)val[j];
    }
    *(list::f16x8*)(a.out + o) = h;
    if (a.level) {
      *(float4*)(a.level + o) = make_float4(val[0], val[1], val[2], val[3]);
      *(float4*)(a.level + o + 4) = make_float4(val[4], val[5], val[6], val[7]);
    }
  }
}

// (a launch error of the forward is reported under the entry point's name, not the kernel's)
template <int S, int KS>
int launch_conv_nt(const ConvArgs& a, int B, int tiles, hipStream_t s) {
  // 64 output channels per workgroup; narrower where that leaves the chip short of workgroups (the order of every
  // element's sum does not depend on the choice)
  const int64_t wg64 = (int64_t)tiles * B * (a.COUT / 64);
  const int nt = wg64 >= 512 ? 4 : wg64 >= 256 ? 2 : 1;
  const dim3 grid((unsigned)tiles, (unsigned)(a.COUT / (16 * nt)), (unsigned)B);
  auto run = [&](auto kernel) { return launch("list_imgenc_forward", kernel, grid, dim3(kThreads), s, a); };
  switch (nt) {
    case 4: return run(imgenc_conv_kernel<S, KS, 4>);
    case 2: return run(imgenc_conv_kernel<S, KS, 2>);
    default: return run(imgenc_conv_kernel<S, KS, 1>);
  }
}

int launch_conv(ConvArgs a, int B, int ks, int stride, hipStream_t s) {
  a.ntx = (a.Wo + kTx - 1) / kTx;
  const int tiles = a.ntx * ((a.Ho + kTy - 1) / kTy);
  if (ks == 1) return launch_conv_nt<2, 1>(a, B, tiles, s);
  return stride == 2 ? launch_conv_nt<2, 3>(a, B, tiles, s) : launch_conv_nt<1, 3>(a, B, tiles, s);
}

// ---- head ------------------------------------------------------------------------------------------------------------
// f4: fp32 [B][hw][512]; wt: [512][128] (the composed matrix, transposed); bias [128].  Mean: thread (q, g) sums channels
// 4 q .. 4 q + 3 over the pixels g, g + 4, ... in order; the four partial sums of a channel are added in the order g = 0 .. 3,
// then divided by hw.  vec[n]: one fmaf chain over k = 0 .. 511, then the bias.
constexpr int kHeadThreads = 512, kHeadGroups = 4;
__global__ __launch_bounds__(kHeadThreads) void imgenc_head_kernel(const float* __restrict__ f4, int hw,
                                                                    const float* __restrict__ wt,
                                                                    const float* __restrict__ bias,
                                                                    float* __restrict__ vec) {
  __shared__ float4 part[kHeadGroups][kC4 / 4];
  __shared__ float mean[kC4];
  const float4* x = (const float4*)(f4 + (int64_t)blockIdx.x * hw * kC4);
  const int q = threadIdx.x & (kC4 / 4 - 1), g = threadIdx.x / (kC4 / 4);
  float4 sum = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 4
  for (int p = g; p < hw; p += kHeadGroups) {
    const float4 v = x[(int64_t)p * (kC4 / 4) + q];
    sum.x += v.x; sum.y += v.y; sum.z += v.z; sum.w += v.w;
  }
  part[g][q] = sum;
  __syncthreads();
  {
    const int ch = threadIdx.x;                        // one channel per thread
    const float* pf = (const float*)part;
    float tot = pf[ch];
#pragma unroll
    for (int k = 1; k < kHeadGroups; ++k) tot += pf[k * kC4 + ch];
    mean[ch] = tot / (float)hw;
  }
  __syncthreads();
  if (threadIdx.x < kVec) {
    float acc = 0.f;
#pragma unroll 16
    for (int k = 0; k < kC4; ++k) acc = fmaf(mean[k], wt[k * kVec + threadIdx.x], acc);
    vec[(int64_t)blockIdx.x * kVec + threadIdx.x] = acc + bias[threadIdx.x];
  }
}

// ---- prep ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void imgenc_pack_kernel(const float* __restrict__ w, int cin, int cout, int ks,
                                                                _Float16* __restrict__ out, int total) {
  const int idx = blockIdx.x * kThreads + threadIdx.x;
  if (idx >= total) return;
  const int j = idx & 7, lane = (idx >> 3) & 63, rest = idx >> 9;
  const int ntiles = cout / 16, taps = ks * ks;
  const int nt = rest % ntiles, tap = (rest / ntiles) % taps, chunk = rest / (ntiles * taps);
  const int n = nt * 16 + (lane & 15), c = chunk * kCC + 8 * (lane >> 4) + j;
  out[idx] = (_Float16)w[((int64_t)n * cin + c) * taps + tap];
}

__global__ __launch_bounds__(kThreads) void imgenc_stem_pack_kernel(const float* __restrict__ w,
                                                                     float* __restrict__ out) {
  const int idx = blockIdx.x * kThreads + threadIdx.x;                 // out[k][n] = w[n][k]
  if (idx < kStemK * kStemC) out[idx] = w[(idx % kStemC) * kStemK + idx / kStemC];
}

// fc1 o fc in float64, rounded once: wt[k][n] = sum_j fc1_w[n][j] fc_w[j][k]; bias[n] = sum_j fc1_w[n][j] fc_b[j] + fc1_b[n]
__global__ __launch_bounds__(kThreads) void imgenc_compose_kernel(const float* __restrict__ fc_w,
                                                                   const float* __restrict__ fc_b,
                                                                   const float* __restrict__ fc1_w,
                                                                   const float* __restrict__ fc1_b,
                                                                   float* __restrict__ wt, float* __restrict__ bias) {
  const int idx = blockIdx.x * kThreads + threadIdx.x;
  if (idx >= (kC4 + 1) * kVec) return;
  const int n = idx % kVec, k = idx / kVec;
  double sum = 0.0;
  if (k < kC4) {
    for (int j = 0; j < kFc; ++j) sum += (double)fc1_w[n * kFc + j] * (double)fc_w[j * kC4 + k];
    wt[k * kVec + n] = (float)sum;
  } else {
    for (int j = 0; j < kFc; ++j) sum += (double)fc1_w[n * kFc + j] * (double)fc_b[j];
    bias[n] = (float)(sum + (double)fc1_b[n]);
  }
}

int check_io(const ListImgencIO* io, const Net& net, const char* what) {
  if (!io) return fail(LIST_ERR_ARG, "%s: io is NULL", what);
  if (int rc = check_shape(io->B, io->H, io->W)) return rc;
  const void* ptrs[] = {io->img, io->packed, io->workspace, io->vec};
  const char* names[] = {"img", "packed", "workspace", "vec"};
  for (int i = 0; i < 4; ++i)
    if (!ptrs[i]) return fail(LIST_ERR_ARG, "%s: %s is NULL", what, names[i]);
  for (int k = 0; k < kLevels; ++k)
    if (!io->levels_out[k]) return fail(LIST_ERR_ARG, "%s: levels_out[%d] is NULL", what, k);
  if (misaligned(io->img, 4) || misaligned(io->vec, 4))
    return fail(LIST_ERR_ARG, "%s: %s is not 4-byte aligned", what, misaligned(io->img, 4) ? "img" : "vec");
  if (misaligned(io->packed, 16) || misaligned(io->workspace, 16))
    return fail(LIST_ERR_ARG, "%s: %s is not 16-byte aligned", what, misaligned(io->packed, 16) ? "packed" : "workspace");
  for (int k = 0; k < kLevels; ++k)
    if (misaligned(io->levels_out[k], 16))
      return fail(LIST_ERR_ARG, "%s: levels_out[%d] is not 16-byte aligned", what, k);
  const size_t need_p = packed_layout(net).total;
  if (io->packed_bytes < need_p) return packed_too_small(what, io->packed_bytes, need_p);
  const size_t need_w = workspace_layout(net, io->B, io->H, io->W).total;
  if (io->workspace_bytes < need_w)
    return workspace_too_small(io->workspace_bytes, need_w, "list_imgenc_workspace_bytes");
  return LIST_OK;
}

}  // namespace

extern "C" {

const char* list_imgenc_last_error(void) { return g_err; }

size_t list_imgenc_weight_bytes(void) { return packed_layout(make_net()).total; }

size_t list_imgenc_workspace_bytes(int32_t B, int32_t H, int32_t W) {
  if (check_shape(B, H, W) != LIST_OK) return 0;
  return workspace_layout(make_net(), B, H, W).total;
}

int32_t list_imgenc_n_steps(void) { return kSteps; }

int list_imgenc_prep_weights(const ListImgencParams* params, void* packed, size_t packed_bytes, void* stream) {
  if (!params || !packed)
    return fail(LIST_ERR_ARG, "list_imgenc_prep_weights: %s is NULL", params ? "packed" : "params");
  if (misaligned(packed, 16)) return fail(LIST_ERR_ARG, "list_imgenc_prep_weights: packed is not 16-byte aligned");
  const Net net = make_net();
  const PackedLayout P = packed_layout(net);
  if (packed_bytes < P.total) return packed_too_small("list_imgenc_prep_weights", packed_bytes, P.total);
  for (int c = 0; c < kConvs; ++c) {
    const ListImgencConv& cv = params->conv[c];
    if (!cv.w) return fail(LIST_ERR_ARG, "list_imgenc_prep_weights: conv[%d].w is NULL", c);
    if (!cv.bn_weight || !cv.bn_bias || !cv.bn_mean || !cv.bn_var)
      return fail(LIST_ERR_ARG, "list_imgenc_prep_weights: conv[%d]: a BN array is NULL", c);
  }
  if (!params->fc_w || !params->fc_b || !params->fc1_w || !params->fc1_b)
    return fail(LIST_ERR_ARG, "list_imgenc_prep_weights: fc_w, fc_b, fc1_w or fc1_b is NULL");
  hipStream_t s = (hipStream_t)stream;
  const char* const name = "list_imgenc_prep_weights";      // a launch error is reported under the entry point's name
  const dim3 block(kThreads);
  for (int k = 0; k < kSteps; ++k) {
    const Step& st = net.s[k];
    if (st.conv < 0) continue;
    const ListImgencConv& cv = params->conv[st.conv];
    const ConvSlot& slot = P.conv[st.conv];
    int rc;
    if (st.kind == STEM) {
      rc = launch(name, imgenc_stem_pack_kernel, dim3(blocks_for(kStemK * kStemC, kThreads)), block, s, cv.w,
                  at<float>(packed, slot.w));
    } else {
      const int total = (int)(wpk_bytes(st) / 2);
      rc = launch(name, imgenc_pack_kernel, dim3(blocks_for(total, kThreads)), block, s, cv.w, st.cin, st.cout, st.ks,
                  at<_Float16>(packed, slot.w), total);
    }
    if (rc) return rc;
    list::launch_bn_fold(cv.bn_weight, cv.bn_bias, cv.bn_mean, cv.bn_var, cv.bn_eps, st.cout, at<float>(packed, slot.s),
                         at<float>(packed, slot.t), s);
    if ((rc = launched(name))) return rc;
  }
  return launch(name, imgenc_compose_kernel, dim3(blocks_for((kC4 + 1) * kVec, kThreads)), block, s, params->fc_w,
                params->fc_b, params->fc1_w, params->fc1_b, at<float>(packed, P.head_w), at<float>(packed, P.head_b));
}

int list_imgenc_forward_steps(const ListImgencIO* io, int32_t step_begin, int32_t step_end, void* stream) {
  const Net net = make_net();
  if (int rc = check_io(io, net, "list_imgenc_forward")) return rc;
  if (int rc = check_step_range("list_imgenc_forward_steps", step_begin, step_end, kSteps)) return rc;
  const PackedLayout P = packed_layout(net);
  const int B = io->B, H = io->H, W = io->W;
  const WorkspaceLayout WS = workspace_layout(net, B, H, W);
  hipStream_t s = (hipStream_t)stream;
  const void* pk = io->packed;
  auto f = [&](size_t off) { return at<float>(pk, off); };
  auto act = [&](int k) { return at<_Float16>(io->workspace, WS.act[k]); };
  const char* const name = "list_imgenc_forward";      // a launch error is reported under the entry point's name

  for (int k = step_begin; k < step_end; ++k) {
    const Step& st = net.s[k];
    const int Ho = H >> st.shift_out, Wo = W >> st.shift_out;
    int rc;
    if (st.kind == STEM) {
      const ConvSlot& c = P.conv[0];
      const dim3 grid((unsigned)((H / kStemTile) * (W / kStemTile)), (unsigned)B);
      rc = launch(name, imgenc_stem_kernel, grid, dim3(kThreads), s, io->img, io->img_sb, io->img_sc, io->img_sh,
                  io->img_sw, H, W, f(c.w), f(c.s), f(c.t), io->levels_out[0], act(k));
    } else if (st.kind == POOL) {
      const int64_t total = (int64_t)B * Ho * Wo * 8;
      rc = launch(name, imgenc_pool_kernel, dim3(blocks_for(total, kThreads)), dim3(kThreads), s, act(st.in), act(k), H,
                  W, total);
    } else if (st.kind == CONV) {
      const ConvSlot& c = P.conv[st.conv];
      ConvArgs a;
      a.in = act(st.in);
      a.idt = st.idt >= 0 ? act(st.idt) : nullptr;
      a.out = act(k);
      a.level = st.level >= 0 ? io->levels_out[st.level] : nullptr;
      a.w = at<list::f16x8>(pk, c.w);
      a.s = f(c.s);
      a.t = f(c.t);
      a.Ho = Ho; a.Wo = Wo;
      a.Hi = Ho * st.stride; a.Wi = Wo * st.stride;
      a.CIN = st.cin; a.COUT = st.cout; a.relu = st.relu;
      rc = launch_conv(a, B, st.ks, st.stride, s);
    } else {
      rc = launch(name, imgenc_head_kernel, dim3((unsigned)B), dim3(kHeadThreads), s,
                  (const float*)io->levels_out[kLevels - 1], Ho * Wo, f(P.head_w), f(P.head_b), io->vec);
    }
    if (rc) return rc;
  }
  return LIST_OK;
}

int list_imgenc_forward(const ListImgencIO* io, void* stream) {
  return list_imgenc_forward_steps(io, 0, kSteps, stream);
}

}  // extern "C"
