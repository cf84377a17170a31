// Training-image augmentation on the device (include/list_augment.h): flip, colour jitter and ToTensor of a uint8 batch in
// one launch.
//
//   augment_kernel<VEC, CL>  a thread owns four consecutive output columns of one row: 12 source bytes in, 12 floats out.
//                            blockIdx.y is the image, so its parameters (one 32-byte record, read through the scalar
//                            cache) and every branch on them are uniform over the workgroup.  VEC: three dword loads and
//                            16-byte stores (the host has checked the alignment and that W is a multiple of 4, so there is
//                            no row tail); else byte loads and float stores, for any base and any W.  CL: dst is
//                            channels-last.  The statements between load and store are csrc/augment_math.h's in both.
//
// No LDS and no workspace.  The hue step costs a few dozen float64 operations per pixel; at the sizes of a training batch
// the launch itself is what the call takes.
#include <math.h>

#include <hip/hip_runtime.h>

#include "list_host.h"
#include "list_augment.h"

#pragma clang fp contract(off)

#include "augment_math.h"                        // below the pragma: its products and sums are not contracted either
#include "augment_check.h"                       // check_params

static_assert(LIST_AUGMENT_FLIP == AUGMENT_FLIP && LIST_AUGMENT_BRIGHTNESS == AUGMENT_BRIGHTNESS &&
              LIST_AUGMENT_SATURATION == AUGMENT_SATURATION && LIST_AUGMENT_HUE == AUGMENT_HUE, "one ops mask");
static_assert(sizeof(ListAugmentParams) == 32, "the binding mirrors a 32-byte record");

namespace {

constexpr int kThreads = 256;
constexpr int kCols = 4;                         // output columns per thread
constexpr int64_t kMaxBatch = 65535, kMaxSide = 65536;      // gridDim.y; H * ceil(W / 4) stays below 2^31

__device__ __forceinline__ int byte_of(const uint32_t w[3], int j) { return (int)((w[j >> 2] >> (8 * (j & 3))) & 0xffu); }

template <bool VEC, bool CL>
__global__ __launch_bounds__(kThreads) void augment_kernel(const uint8_t* __restrict__ src, float* __restrict__ dst, int H,
                                                           int W, int Wq, const ListAugmentParams* __restrict__ params) {
  const uint32_t t = blockIdx.x * (uint32_t)kThreads + threadIdx.x;
  if (t >= (uint32_t)H * (uint32_t)Wq) return;
  const int b = blockIdx.y, y = (int)(t / (uint32_t)Wq), x0 = kCols * (int)(t % (uint32_t)Wq);
  const int n = VEC ? kCols : (W - x0 < kCols ? W - x0 : kCols);
  const ListAugmentParams p = params[b];
  const bool flip = (p.ops & AUGMENT_FLIP) != 0;
  const int64_t line = (int64_t)b * H + y;       // row of the batch
  const uint8_t* __restrict__ row = src + line * W * 3;

  int lv[kCols][3];                              // output column x0 + k: its source pixel, then its result
  if constexpr (VEC) {
    const int s0 = flip ? W - kCols - x0 : x0;   // the run's first source column; flipped, the run is read backwards
    const uint32_t* __restrict__ q = reinterpret_cast<const uint32_t*>(row + 3 * (int64_t)s0);
    const uint32_t w[3] = {q[0], q[1], q[2]};
#pragma unroll
    for (int k = 0; k < kCols; ++k)
#pragma unroll
      for (int c = 0; c < 3; ++c) lv[k][c] = flip ? byte_of(w, 3 * (kCols - 1 - k) + c) : byte_of(w, 3 * k + c);
  } else {
#pragma unroll
    for (int k = 0; k < kCols; ++k) {
      const int col = flip ? W - 1 - x0 - k : x0 + k;
#pragma unroll
      for (int c = 0; c < 3; ++c) lv[k][c] = k < n ? (int)row[3 * (int64_t)col + c] : 0;
    }
  }

  if (p.ops & (AUGMENT_BRIGHTNESS | AUGMENT_SATURATION | AUGMENT_HUE)) {
#pragma unroll
    for (int k = 0; k < kCols; ++k)
      augment_colour(lv[k][0], lv[k][1], lv[k][2], p.ops, p.order, p.brightness, p.saturation, p.hue_shift);
  }

  float out[kCols][3];
#pragma unroll
  for (int k = 0; k < kCols; ++k)
#pragma unroll
    for (int c = 0; c < 3; ++c) out[k][c] = augment_to_float(lv[k][c]);

  if constexpr (CL) {
    float* __restrict__ o = dst + (line * W + x0) * 3;
    if constexpr (VEC) {
      float4* __restrict__ o4 = reinterpret_cast<float4*>(o);
      o4[0] = make_float4(out[0][0], out[0][1], out[0][2], out[1][0]);
      o4[1] = make_float4(out[1][1], out[1][2], out[2][0], out[2][1]);
      o4[2] = make_float4(out[2][2], out[3][0], out[3][1], out[3][2]);
    } else {
#pragma unroll
      for (int k = 0; k < kCols; ++k)
        if (k < n) o[3 * k] = out[k][0], o[3 * k + 1] = out[k][1], o[3 * k + 2] = out[k][2];
    }
  } else {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float* __restrict__ o = dst + (((int64_t)b * 3 + c) * H + y) * W + x0;
      if constexpr (VEC) {
        *reinterpret_cast<float4*>(o) = make_float4(out[0][c], out[1][c], out[2][c], out[3][c]);
      } else {
#pragma unroll
        for (int k = 0; k < kCols; ++k)
          if (k < n) o[k] = out[k][c];
      }
    }
  }
}

}  // namespace

// ---- host (the records are checked by csrc/augment_check.h's check_params) ------------------------------------------
extern "C" {

const char* list_augment_last_error(void) { return g_err; }

int list_augment_fwd(const uint8_t* src, float* dst, int64_t B, int64_t H, int64_t W, int channels_last,
                     const ListAugmentParams* params_host, const ListAugmentParams* params_device, void* stream) {
  const char* null = !src ? "src" : !dst ? "dst" : !params_host ? "params_host" : !params_device ? "params_device" : nullptr;
  if (null) return fail(LIST_ERR_ARG, "%s is NULL", null);
  if (B < 1 || B > kMaxBatch || H < 1 || H > kMaxSide || W < 1 || W > kMaxSide)
    return fail(LIST_ERR_SHAPE, "B = %lld, H = %lld, W = %lld: need 1 <= B <= 65535 and 1 <= H, W <= 65536", (long long)B,
                (long long)H, (long long)W);
  if (channels_last != 0 && channels_last != 1)
    return fail(LIST_ERR_SHAPE, "channels_last = %d: 0 (NCHW) or 1", channels_last);
  for (int64_t i = 0; i < B; ++i)
    if (int rc = check_params(params_host[i], (long long)i)) return rc;
  const int Wq = (int)cdiv(W, kCols);
  const dim3 grid((unsigned)cdiv(H * Wq, kThreads), (unsigned)B), block(kThreads);
  const bool vec = W % kCols == 0 && !misaligned(src, 4) && !misaligned(dst, 16);
  hipStream_t s = (hipStream_t)stream;
  auto run = [&](auto kernel) {
    return launch("augment_kernel", kernel, grid, block, s, src, dst, (int)H, (int)W, Wq, params_device);
  };
  if (vec && channels_last) return run(augment_kernel<true, true>);
  if (vec) return run(augment_kernel<true, false>);
  if (channels_last) return run(augment_kernel<false, true>);
  return run(augment_kernel<false, false>);
}

int list_augment_pixel(const uint8_t* rgb_in, const ListAugmentParams* p, uint8_t* rgb_out, float* out) {
  if (!rgb_in || !p) return fail(LIST_ERR_ARG, "%s is NULL", !rgb_in ? "rgb_in" : "p");
  if (int rc = check_params(*p, 0)) return rc;
  int r = rgb_in[0], g = rgb_in[1], b = rgb_in[2];
  augment_colour(r, g, b, p->ops, p->order, p->brightness, p->saturation, p->hue_shift);
  if (rgb_out) rgb_out[0] = (uint8_t)r, rgb_out[1] = (uint8_t)g, rgb_out[2] = (uint8_t)b;
  if (out) out[0] = augment_to_float(r), out[1] = augment_to_float(g), out[2] = augment_to_float(b);
  return LIST_OK;
}

}  // extern "C"
