// Ragged-batch image resize on the device (include/list_resize.h): Pillow's bilinear resample of uint8 images of different
// sizes, with the flip and the colour steps of list_augment.h on the source pixels and ToTensor on the result.
//
//   resize_stage_kernel<FIRST, CL>  one stage of every image of the batch in one launch.  A thread owns one output pixel of
//                            its image's stage (three channels, three int32 accumulators); blockIdx.y is the image, so its
//                            plan record, its parameters and every branch on them (copy / horizontal / vertical, flip,
//                            colour steps) are uniform over the workgroup; workgroups past an image's last pixel leave at
//                            once.  FIRST: from the packed source to the uint8 intermediate in the workspace, each tap
//                            flipped and jittered as it is read (csrc/augment_math.h); else from the intermediate to the
//                            float output, NCHW or channels-last (CL).  The pass is csrc/resize_math.h's: integer
//                            multiply-adds from one half up, one clip.
//
// Consecutive threads own consecutive output columns: a vertical pass and a copy read and write whole lines; a horizontal
// pass reads spans that overlap from thread to thread and are served by the caches.  No LDS, no atomics, nothing that
// depends on the order of the workgroups: every output byte has one writer.
#include <math.h>
#include <string.h>

#include <vector>

#include <hip/hip_runtime.h>

#include "list_host.h"
#include "list_resize.h"

#pragma clang fp contract(off)

#include "augment_math.h"                        // below the pragma: nothing in them is contracted
#include "augment_check.h"                       // check_params
#include "resize_math.h"

static_assert(sizeof(ListResizeImage) == 16 && sizeof(ListResizePlanHeader) == 40 && sizeof(ListResizePlanImage) == 80,
              "the binding mirrors these records");

namespace {

constexpr int kThreads = 256;
constexpr int64_t kMaxSide = LIST_RESIZE_MAX_SIDE, kMaxBatch = LIST_RESIZE_MAX_BATCH;

template <bool FIRST, bool CL>
__global__ __launch_bounds__(kThreads) void resize_stage_kernel(const uint8_t* __restrict__ in_base, void* __restrict__ out_base,
                                                                const char* __restrict__ plan,
                                                                const ListAugmentParams* __restrict__ params, int out_h,
                                                                int out_w) {
  const int b = blockIdx.y;
  const ListResizePlanImage rec = reinterpret_cast<const ListResizePlanImage*>(plan + sizeof(ListResizePlanHeader))[b];
  const int in_w = FIRST ? rec.W : rec.mid_w;
  const int o_h = FIRST ? rec.mid_h : out_h, o_w = FIRST ? rec.mid_w : out_w;
  const uint32_t t = blockIdx.x * (uint32_t)kThreads + threadIdx.x;
  if (t >= (uint32_t)o_h * (uint32_t)o_w) return;
  const int y = (int)(t / (uint32_t)o_w), x = (int)(t % (uint32_t)o_w);
  const int s = FIRST ? 0 : 1, axis = rec.stage[s];
  const uint8_t* __restrict__ in = in_base + (FIRST ? rec.src_offset : rec.mid_offset);

  int ops = 0;
  ListAugmentParams p = {};
  if (FIRST && params) p = params[b], ops = p.ops;
  const bool flip = (ops & AUGMENT_FLIP) != 0;
  const bool colour = (ops & (AUGMENT_BRIGHTNESS | AUGMENT_SATURATION | AUGMENT_HUE)) != 0;

  // the source pixel (row, col) of this stage, as the pass sees it
  auto pixel = [&](int row, int col, int& r, int& g, int& bl) {
    if (FIRST && flip) col = in_w - 1 - col;
    const uint8_t* q = in + ((int64_t)row * in_w + col) * 3;
    r = q[0], g = q[1], bl = q[2];
    if (FIRST && colour) augment_colour(r, g, bl, ops, p.order, p.brightness, p.saturation, p.hue_shift);
  };

  int lv[3];
  if (axis == RESIZE_COPY) {
    pixel(y, x, lv[0], lv[1], lv[2]);
  } else {
    const int o = axis == RESIZE_HORIZONTAL ? x : y, ksize = rec.ksize[s];
    const int32_t* __restrict__ bounds = reinterpret_cast<const int32_t*>(plan + rec.bounds[s]);
    const int32_t* __restrict__ K = reinterpret_cast<const int32_t*>(plan + rec.weights[s]) + (int64_t)o * ksize;
    const int first = bounds[2 * o], count = bounds[2 * o + 1];
    int acc[3] = {resize_acc0(), resize_acc0(), resize_acc0()};
    for (int k = 0; k < count; ++k) {
      int r, g, bl;
      if (axis == RESIZE_HORIZONTAL) pixel(y, first + k, r, g, bl);
      else pixel(first + k, x, r, g, bl);
      const int w = K[k];
      acc[0] += r * w, acc[1] += g * w, acc[2] += bl * w;
    }
    lv[0] = resize_level(acc[0]), lv[1] = resize_level(acc[1]), lv[2] = resize_level(acc[2]);
  }

  if constexpr (FIRST) {
    uint8_t* __restrict__ o = static_cast<uint8_t*>(out_base) + rec.mid_offset + ((int64_t)y * o_w + x) * 3;
    o[0] = (uint8_t)lv[0], o[1] = (uint8_t)lv[1], o[2] = (uint8_t)lv[2];
  } else {
    float* __restrict__ dst = static_cast<float*>(out_base);
    if constexpr (CL) {
      float* __restrict__ o = dst + (((int64_t)b * o_h + y) * o_w + x) * 3;
      o[0] = augment_to_float(lv[0]), o[1] = augment_to_float(lv[1]), o[2] = augment_to_float(lv[2]);
    } else {
#pragma unroll
      for (int c = 0; c < 3; ++c) dst[(((int64_t)b * 3 + c) * o_h + y) * o_w + x] = augment_to_float(lv[c]);
    }
  }
}

// ---- host -------------------------------------------------------------------------------------------------------------
int check_batch(const ListResizeImage* images, int64_t B, int64_t out_h, int64_t out_w) {
  if (!images) return fail(LIST_ERR_ARG, "images is NULL");
  if (B < 1 || B > kMaxBatch || out_h < 1 || out_h > kMaxSide || out_w < 1 || out_w > kMaxSide)
    return fail(LIST_ERR_SHAPE, "B = %lld, out_h = %lld, out_w = %lld: need 1 <= B <= 65535 and 1 <= out_h, out_w <= 16384",
                (long long)B, (long long)out_h, (long long)out_w);
  for (int64_t i = 0; i < B; ++i)
    if (images[i].H < 1 || images[i].H > kMaxSide || images[i].W < 1 || images[i].W > kMaxSide)
      return fail(LIST_ERR_SHAPE, "images[%lld]: H = %d, W = %d: need 1 <= H, W <= 16384", (long long)i, images[i].H,
                  images[i].W);
  return LIST_OK;
}

// The geometry of image `im` (everything of its record but the offsets), and how many int32 its tables hold
struct Geometry {
  int32_t stage[2], ksize[2], n_out[2], n_in[2], mid_h, mid_w;
  int64_t table_ints(int s) const { return stage[s] == RESIZE_COPY ? 0 : (int64_t)n_out[s] * (2 + ksize[s]); }
  int64_t mid_bytes() const { return (int64_t)mid_h * mid_w * 3; }
};

Geometry geometry(int H, int W, int out_h, int out_w) {
  Geometry g = {};
  resize_stages(H, W, out_h, out_w, g.stage, &g.mid_h, &g.mid_w);
  for (int s = 0; s < 2; ++s) {
    if (g.stage[s] == RESIZE_COPY) continue;
    const bool horizontal = g.stage[s] == RESIZE_HORIZONTAL;
    g.n_in[s] = horizontal ? W : H, g.n_out[s] = horizontal ? out_w : out_h;
    g.ksize[s] = resize_ksize(g.n_in[s], g.n_out[s]);
  }
  return g;
}

size_t plan_bytes_of(const ListResizeImage* images, int64_t B, int64_t out_h, int64_t out_w) {
  int64_t ints = 0;
  for (int64_t i = 0; i < B; ++i) {
    const Geometry g = geometry(images[i].H, images[i].W, (int)out_h, (int)out_w);
    ints += g.table_ints(0) + g.table_ints(1);
  }
  return sizeof(ListResizePlanHeader) + (size_t)B * sizeof(ListResizePlanImage) + (size_t)ints * 4;
}

size_t workspace_bytes_of(const ListResizeImage* images, int64_t B, int64_t out_h, int64_t out_w) {
  int64_t bytes = 0;
  for (int64_t i = 0; i < B; ++i) bytes += geometry(images[i].H, images[i].W, (int)out_h, (int)out_w).mid_bytes();
  return (size_t)bytes;
}

// Fills the tables of one pass at `tables` (bounds, then weights); LIST_OK, or the refusal of an accumulator that could
// reach 2^31
int fill_tables(int n_in, int n_out, int ksize, int32_t* tables, std::vector<double>& scratch) {
  int32_t* bounds = tables;
  int32_t* weights = tables + 2 * (int64_t)n_out;
  scratch.resize((size_t)ksize);
  for (int xx = 0; xx < n_out; ++xx) {
    const int64_t sum = resize_coeffs(n_in, n_out, xx, ksize, &bounds[2 * xx], &bounds[2 * xx + 1],
                                      weights + (int64_t)xx * ksize, scratch.data());
    if (255 * sum + (int64_t)resize_acc0() >= (int64_t)1 << 31)
      return fail(LIST_ERR_SHAPE, "axis %d -> %d, output %d: weights sum to %lld, an int32 accumulator could overflow", n_in,
                  n_out, xx, (long long)sum);
  }
  return LIST_OK;
}

}  // namespace

extern "C" {

const char* list_resize_last_error(void) { return g_err; }

size_t list_resize_plan_bytes(const ListResizeImage* images, int64_t B, int64_t out_h, int64_t out_w) {
  if (check_batch(images, B, out_h, out_w)) return 0;
  return plan_bytes_of(images, B, out_h, out_w);
}

size_t list_resize_workspace_bytes(const ListResizeImage* images, int64_t B, int64_t out_h, int64_t out_w) {
  if (check_batch(images, B, out_h, out_w)) return 0;
  return workspace_bytes_of(images, B, out_h, out_w);
}

int list_resize_plan(const ListResizeImage* images, int64_t B, int64_t src_bytes, int64_t out_h, int64_t out_w, void* plan,
                     size_t plan_bytes) {
  if (!plan) return fail(LIST_ERR_ARG, "plan is NULL");
  if (misaligned(plan, 8)) return fail(LIST_ERR_ARG, "plan is not 8-byte aligned");
  if (int rc = check_batch(images, B, out_h, out_w)) return rc;
  for (int64_t i = 0; i < B; ++i) {
    const int64_t extent = (int64_t)images[i].H * images[i].W * 3;
    if (images[i].offset < 0 || images[i].offset > src_bytes || extent > src_bytes - images[i].offset)
      return fail(LIST_ERR_ARG, "images[%lld]: offset %lld + %lld bytes lies outside src_bytes = %lld", (long long)i,
                  (long long)images[i].offset, (long long)extent, (long long)src_bytes);
  }
  const size_t need = plan_bytes_of(images, B, out_h, out_w);
  if (plan_bytes < need) return fail(LIST_ERR_WORKSPACE, "plan %zu bytes, need %zu (list_resize_plan_bytes)", plan_bytes, need);
  char* base = static_cast<char*>(plan);
  ListResizePlanHeader head = {(int64_t)need, 0, src_bytes, LIST_RESIZE_PLAN_MAGIC, (int32_t)B, (int32_t)out_h, (int32_t)out_w};
  int64_t at = (int64_t)sizeof(ListResizePlanHeader) + B * (int64_t)sizeof(ListResizePlanImage), mid = 0;
  std::vector<double> scratch;
  for (int64_t i = 0; i < B; ++i) {
    const Geometry g = geometry(images[i].H, images[i].W, (int)out_h, (int)out_w);
    ListResizePlanImage rec = {};
    rec.src_offset = images[i].offset, rec.mid_offset = mid, rec.H = images[i].H, rec.W = images[i].W;
    rec.mid_h = g.mid_h, rec.mid_w = g.mid_w;
    mid += g.mid_bytes();
    for (int s = 0; s < 2; ++s) {
      rec.stage[s] = g.stage[s], rec.ksize[s] = g.ksize[s];
      if (g.stage[s] == RESIZE_COPY) continue;
      rec.bounds[s] = at, rec.weights[s] = at + 8 * (int64_t)g.n_out[s];
      if (int rc = fill_tables(g.n_in[s], g.n_out[s], g.ksize[s], reinterpret_cast<int32_t*>(base + at), scratch)) return rc;
      at += 4 * g.table_ints(s);
    }
    memcpy(base + sizeof(ListResizePlanHeader) + (size_t)i * sizeof(ListResizePlanImage), &rec, sizeof(rec));
  }
  head.workspace_bytes = mid;
  memcpy(base, &head, sizeof(head));
  return LIST_OK;
}

int list_resize_fwd(const uint8_t* src, int64_t src_bytes, const void* plan_host, const void* plan_device, size_t plan_bytes,
                    const ListAugmentParams* params_host, const ListAugmentParams* params_device, float* dst,
                    int channels_last, void* workspace, size_t workspace_bytes, void* stream) {
  const char* null = !src ? "src" : !plan_host ? "plan_host" : !plan_device ? "plan_device" : !dst ? "dst"
                     : !workspace ? "workspace" : (params_host && !params_device) ? "params_device"
                     : (params_device && !params_host) ? "params_host" : nullptr;
  if (null) return fail(LIST_ERR_ARG, "%s is NULL", null);
  if (misaligned(plan_host, 8) || misaligned(plan_device, 8) || misaligned(dst, 4))
    return fail(LIST_ERR_ARG, "plan_host and plan_device must be 8-byte aligned, dst 4-byte aligned");
  if (channels_last != 0 && channels_last != 1)
    return fail(LIST_ERR_SHAPE, "channels_last = %d: 0 (NCHW) or 1", channels_last);
  if (plan_bytes < sizeof(ListResizePlanHeader))
    return fail(LIST_ERR_WORKSPACE, "plan %zu bytes, need %zu (list_resize_plan_bytes)", plan_bytes, sizeof(ListResizePlanHeader));
  const char* base = static_cast<const char*>(plan_host);
  ListResizePlanHeader head;
  memcpy(&head, base, sizeof(head));
  if (head.magic != LIST_RESIZE_PLAN_MAGIC || head.B < 1 || head.B > kMaxBatch || head.out_h < 1 || head.out_h > kMaxSide ||
      head.out_w < 1 || head.out_w > kMaxSide)
    return fail(LIST_ERR_ARG, "plan_host is not a plan of list_resize_plan (magic %#x, B = %d, out %d x %d)", head.magic,
                head.B, head.out_h, head.out_w);
  if (head.plan_bytes < 0 || plan_bytes < (size_t)head.plan_bytes)
    return fail(LIST_ERR_WORKSPACE, "plan %zu bytes, need %lld (list_resize_plan_bytes)", plan_bytes, (long long)head.plan_bytes);
  if (head.src_bytes != src_bytes)
    return fail(LIST_ERR_ARG, "src_bytes = %lld, the plan was made for %lld", (long long)src_bytes, (long long)head.src_bytes);
  // every record against the rules it was made by, every bounds entry inside its axis: the kernel indexes by them
  const int64_t B = head.B;
  int64_t at = (int64_t)sizeof(ListResizePlanHeader) + B * (int64_t)sizeof(ListResizePlanImage), mid = 0, most[2] = {0, 0};
  for (int64_t i = 0; i < B; ++i) {
    ListResizePlanImage rec;
    memcpy(&rec, base + sizeof(ListResizePlanHeader) + (size_t)i * sizeof(rec), sizeof(rec));
    if (rec.H < 1 || rec.H > kMaxSide || rec.W < 1 || rec.W > kMaxSide)
      return fail(LIST_ERR_SHAPE, "plan image %lld: H = %d, W = %d: need 1 <= H, W <= 16384", (long long)i, rec.H, rec.W);
    const int64_t extent = (int64_t)rec.H * rec.W * 3;
    if (rec.src_offset < 0 || rec.src_offset > src_bytes || extent > src_bytes - rec.src_offset)
      return fail(LIST_ERR_ARG, "plan image %lld: offset %lld + %lld bytes lies outside src_bytes = %lld", (long long)i,
                  (long long)rec.src_offset, (long long)extent, (long long)src_bytes);
    const Geometry g = geometry(rec.H, rec.W, head.out_h, head.out_w);
    bool same = rec.mid_offset == mid && rec.mid_h == g.mid_h && rec.mid_w == g.mid_w;
    for (int s = 0; s < 2 && same; ++s) {
      same = rec.stage[s] == g.stage[s] && rec.ksize[s] == g.ksize[s];
      if (!same || g.stage[s] == RESIZE_COPY) {
        same = same && rec.bounds[s] == 0 && rec.weights[s] == 0;
        continue;
      }
      same = rec.bounds[s] == at && rec.weights[s] == at + 8 * (int64_t)g.n_out[s] &&
             at + 4 * g.table_ints(s) <= head.plan_bytes;
      if (!same) break;
      const int32_t* bounds = reinterpret_cast<const int32_t*>(base + at);
      for (int o = 0; o < g.n_out[s] && same; ++o)
        same = bounds[2 * o] >= 0 && bounds[2 * o + 1] >= 0 && bounds[2 * o + 1] <= g.ksize[s] &&
               (int64_t)bounds[2 * o] + bounds[2 * o + 1] <= g.n_in[s];
      at += 4 * g.table_ints(s);
    }
    if (!same) return fail(LIST_ERR_ARG, "plan image %lld: its record is not list_resize_plan's for %d x %d -> %d x %d",
                           (long long)i, rec.H, rec.W, head.out_h, head.out_w);
    mid += g.mid_bytes();
    const int64_t px0 = (int64_t)g.mid_h * g.mid_w;
    most[0] = px0 > most[0] ? px0 : most[0];
  }
  most[1] = (int64_t)head.out_h * head.out_w;
  if (workspace_bytes < (size_t)mid) return workspace_too_small(workspace_bytes, (size_t)mid, "list_resize_workspace_bytes");
  if (params_host)
    for (int64_t i = 0; i < B; ++i)
      if (int rc = check_params(params_host[i], (long long)i)) return rc;

  hipStream_t s = (hipStream_t)stream;
  const dim3 block(kThreads);
  const char* plan = static_cast<const char*>(plan_device);
  if (int rc = launch("resize_stage_kernel<first>", resize_stage_kernel<true, false>,
                      dim3(blocks_for(most[0], kThreads), (unsigned)B), block, s, src, workspace, plan, params_device,
                      (int)head.out_h, (int)head.out_w))
    return rc;
  const dim3 grid(blocks_for(most[1], kThreads), (unsigned)B);
  const uint8_t* mids = static_cast<const uint8_t*>(workspace);
  const ListAugmentParams* none = nullptr;
  if (channels_last)
    return launch("resize_stage_kernel<last, channels-last>", resize_stage_kernel<false, true>, grid, block, s, mids,
                  (void*)dst, plan, none, (int)head.out_h, (int)head.out_w);
  return launch("resize_stage_kernel<last>", resize_stage_kernel<false, false>, grid, block, s, mids, (void*)dst, plan, none,
                (int)head.out_h, (int)head.out_w);
}

int list_resize_host(const uint8_t* src, int64_t H, int64_t W, uint8_t* dst, int64_t out_h, int64_t out_w) {
  if (!src || !dst) return fail(LIST_ERR_ARG, "%s is NULL", !src ? "src" : "dst");
  if (H < 1 || H > kMaxSide || W < 1 || W > kMaxSide || out_h < 1 || out_h > kMaxSide || out_w < 1 || out_w > kMaxSide)
    return fail(LIST_ERR_SHAPE, "H = %lld, W = %lld, out_h = %lld, out_w = %lld: need 1 <= every side <= 16384", (long long)H,
                (long long)W, (long long)out_h, (long long)out_w);
  const Geometry g = geometry((int)H, (int)W, (int)out_h, (int)out_w);
  std::vector<uint8_t> mid((size_t)g.mid_bytes());
  std::vector<int32_t> tables;
  std::vector<double> scratch;
  const uint8_t* in = src;
  int in_w = (int)W;
  for (int s = 0; s < 2; ++s) {
    tables.assign((size_t)g.table_ints(s), 0);
    if (g.stage[s] != RESIZE_COPY)
      if (int rc = fill_tables(g.n_in[s], g.n_out[s], g.ksize[s], tables.data(), scratch)) return rc;
    uint8_t* out = s == 0 ? mid.data() : dst;
    const int o_h = s == 0 ? g.mid_h : (int)out_h, o_w = s == 0 ? g.mid_w : (int)out_w;
    resize_pass_host(in, in_w, out, o_h, o_w, g.stage[s], tables.data(), tables.data() + 2 * (int64_t)g.n_out[s], g.ksize[s]);
    in = out, in_w = o_w;
  }
  return LIST_OK;
}

}  // extern "C"
