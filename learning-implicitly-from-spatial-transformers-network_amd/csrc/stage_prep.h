// Device-side weight prep shared by the opt-in stages that fold eval-mode BN on the device (voxenc_kernels.hip,
// imgenc_kernels.hip).  Not part of the C ABI.
#pragma once

#include <hip/hip_runtime.h>

namespace list {

constexpr int kPrepThreads = 256;

// Eval-mode BN as y * s + t, n channels.  These two statements are THE fold: fp32 add, correctly rounded sqrt and
// division, then (the units are built with -ffp-contract=off) a rounded multiply and a subtract -- what
// stage.bn_affine restates operation for operation.
static __global__ __launch_bounds__(kPrepThreads) void stage_bn_fold_kernel(const float* __restrict__ weight,
                                                                            const float* __restrict__ bias,
                                                                            const float* __restrict__ mean,
                                                                            const float* __restrict__ var, float eps,
                                                                            int n, float* __restrict__ s,
                                                                            float* __restrict__ t) {
  const int i = blockIdx.x * kPrepThreads + threadIdx.x;
  if (i >= n) return;
  const float sc = weight[i] / sqrtf(var[i] + eps);
  s[i] = sc;
  t[i] = bias[i] - mean[i] * sc;
}

inline void launch_bn_fold(const float* weight, const float* bias, const float* mean, const float* var, float eps, int n,
                           float* s, float* t, hipStream_t stream) {
  hipLaunchKernelGGL(stage_bn_fold_kernel, dim3((unsigned)((n + kPrepThreads - 1) / kPrepThreads)), dim3(kPrepThreads),
                     0, stream, weight, bias, mean, var, eps, n, s, t);
}

}  // namespace list
