// Host-only sanitizer build of the C ABI (tests/test_capi_sanitizers.py): list_capi.hip's argument validation,
// workspace carving and chunk arithmetic run under AddressSanitizer + UBSan on the CPU.  Every kernel launcher the
// C ABI calls is replaced by a stub that aborts: the checks exercised here return BEFORE any launch, so reaching a stub
// is a test failure (a validation hole), not a skipped device call.
#include <stdio.h>
#include <stdlib.h>

#include "list_common.h"

namespace list {
[[noreturn]] static void reached(const char* what) {
  fprintf(stderr, "capi_host_asan: launcher %s reached -- a validation path let a call through\n", what);
  abort();
}
#define STUB(sig, name) sig { reached(name); }
STUB(hipError_t launch_prep_img(const ListMap2D*, int, int, int, int, void*, hipStream_t, int), "launch_prep_img")
STUB(hipError_t launch_img_level_rows(const ListMap2D*, void* const*, int, int, int, hipStream_t), "launch_img_level_rows")
STUB(hipError_t launch_proj_resize_sum(const ListMap2D*, int, int, int, int, int, int, void*, hipStream_t, int), "launch_proj_resize_sum")
STUB(hipError_t launch_transpose_vox(const ListMap3D&, int, int, void*, hipStream_t), "launch_transpose_vox")
bool transpose_tile_eligible(const ListMap3D&, const void*) { return false; }
STUB(hipError_t launch_transpose_vox_fused(const ListMap3D*, void* const*, const int*, int, int, hipStream_t), "launch_transpose_vox_fused")
STUB(hipError_t launch_prep_weights(const ListMlpWeights&, const FeatLayout&, const PackedMlp&, char*, hipStream_t), "launch_prep_weights")
STUB(hipError_t launch_split_xi(const float*, unsigned short*, int64_t, hipStream_t), "launch_split_xi")
STUB(hipError_t launch_split(const float*, unsigned short*, unsigned short*, int64_t, int, hipStream_t, int), "launch_split")
STUB(hipError_t launch_sort_points(const GatherParams&, const ListQueryArgs&, const SortBuffers&, bool, hipStream_t), "launch_sort_points")
STUB(hipError_t launch_gather(const GatherParams&, const FeatLayout&, const ListQueryArgs&, const QueryFwdPlan&, int*, hipStream_t), "launch_gather")
bool fused_fc0_eligible(const GemmParams&, int, int) { return true; }
STUB(hipError_t launch_fc0_fused(const FusedFc0Params&, int, hipStream_t), "launch_fc0_fused")
STUB(hipError_t launch_features_out(const GatherParams&, const FeatLayout&, float*, int*, hipStream_t), "launch_features_out")
STUB(hipError_t launch_gather_vox_box(const GatherParams&, const ListVoxLevel&, int, hipStream_t, int), "launch_gather_vox_box")
STUB(hipError_t launch_gather_fixup(const GatherParams&, const FeatLayout&, const ListQueryArgs&, const int*, hipStream_t), "launch_gather_fixup")
STUB(hipError_t launch_percep_pool(const ListPoolArgs&, hipStream_t), "launch_percep_pool")
STUB(hipError_t launch_gemm(const GemmParams&, int, int, hipStream_t), "launch_gemm")
STUB(hipError_t launch_mlp_tail(const GemmParams&, const char*, const float*, const float*, const float*, float*, const int*, int, hipStream_t), "launch_mlp_tail")
STUB(hipError_t launch_prep_weights_bwd(const ListMlpWeights&, const FeatLayout&, const PackedMlpBwd&, char*, hipStream_t), "launch_prep_weights_bwd")
STUB(hipError_t launch_gemm_tn(const GemmTnParams&, int, hipStream_t), "launch_gemm_tn")
STUB(hipError_t launch_wgrad_reduce(const float*, int, int, int, int, const FeatLayout*, const float*, float*, int, hipStream_t), "launch_wgrad_reduce")
STUB(hipError_t launch_grad_scale(const float*, int64_t, int, float*, float*, float*, hipStream_t), "launch_grad_scale")
STUB(hipError_t launch_head(const float*, const int*, int, int, int, const unsigned short*, const float*, const float*, unsigned short*, unsigned short*, int, hipStream_t), "launch_head")
STUB(hipError_t launch_colsum(const unsigned short*, const unsigned short*, int, int, int, int, const float*, const int*, const float*, int, float*, float*, hipStream_t), "launch_colsum")
STUB(hipError_t launch_scatter_vox(const ScatterParams&, const FeatLayout&, const ListVoxLevel*, const VoxGatherBuffers&, const ScatterStreams&), "launch_scatter_vox")
STUB(hipError_t launch_img_map_grad(const QueryBwdPlan&, const ScatterParams&, const FeatLayout&, const ListQueryArgs&, int, const int*, void*, float*, void*, hipStream_t), "launch_img_map_grad")
STUB(hipError_t launch_trans_grad(const ScatterParams&, const FeatLayout&, const ListQueryArgs&, int, float*, hipStream_t), "launch_trans_grad")
STUB(hipError_t launch_rows_to_grad(const ScatterParams&, int, int, int, int*, float*, int64_t, int64_t, int64_t, hipStream_t), "launch_rows_to_grad")
STUB(hipError_t launch_grad_to_rows(const float*, int64_t, int64_t, int64_t, int, int, int, float*, float*, hipStream_t), "launch_grad_to_rows")
STUB(hipError_t launch_img_grad_to_levels(const float*, int, int, int, const ListMap2D*, hipStream_t, int, const float*), "launch_img_grad_to_levels")
}  // namespace list
