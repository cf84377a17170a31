// Stand-alone driver of the host side of include/list_resize.h, built with the address and undefined-behaviour sanitizers
// (tests/_resize_case.py: csrc/resize_kernels.hip with its host side sanitized too, linked with this file):
//
//     resize_host H W out_h out_w <in: uint8 [H][W][3]> <out: uint8 [out_h][out_w][3]> <plan: the plan buffer>
//
// It sizes and fills the plan of the one-image batch into a buffer of exactly list_resize_plan_bytes bytes, resizes the
// image with list_resize_host into a buffer of exactly its size, and walks the refusals that need no device.  No kernel
// is launched: every call made here returns before its first HIP call.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "list_resize.h"

#define EXPECT(cond)                                                                                  \
  do {                                                                                                \
    if (!(cond)) {                                                                                    \
      fprintf(stderr, "%s:%d: %s failed (%s)\n", __FILE__, __LINE__, #cond, list_resize_last_error()); \
      return 1;                                                                                       \
    }                                                                                                 \
  } while (0)

static bool read_file(const char* path, std::vector<uint8_t>& data) {
  FILE* f = fopen(path, "rb");
  if (!f) return false;
  const size_t got = fread(data.data(), 1, data.size(), f);
  fclose(f);
  return got == data.size();
}

static bool write_file(const char* path, const void* data, size_t bytes) {
  FILE* f = fopen(path, "wb");
  if (!f) return false;
  const size_t put = fwrite(data, 1, bytes, f);
  return fclose(f) == 0 && put == bytes;
}

int main(int argc, char** argv) {
  if (argc != 8) {
    fprintf(stderr, "usage: %s H W out_h out_w in out plan\n", argv[0]);
    return 2;
  }
  const int64_t H = atoll(argv[1]), W = atoll(argv[2]), out_h = atoll(argv[3]), out_w = atoll(argv[4]);
  std::vector<uint8_t> src((size_t)(H * W * 3));
  if (!read_file(argv[5], src)) return 2;
  const int64_t src_bytes = (int64_t)src.size();

  ListResizeImage image = {0, (int32_t)H, (int32_t)W};
  const size_t need = list_resize_plan_bytes(&image, 1, out_h, out_w);
  EXPECT(need >= sizeof(ListResizePlanHeader) + sizeof(ListResizePlanImage));
  void* plan = malloc(need);                         // exactly: a write past it is the sanitizer's to find
  EXPECT(list_resize_plan(&image, 1, src_bytes, out_h, out_w, plan, need) == LIST_OK);
  ListResizePlanHeader head;
  memcpy(&head, plan, sizeof(head));
  EXPECT(head.magic == LIST_RESIZE_PLAN_MAGIC && head.B == 1 && head.plan_bytes == (int64_t)need);
  EXPECT((size_t)head.workspace_bytes == list_resize_workspace_bytes(&image, 1, out_h, out_w));

  std::vector<uint8_t> dst((size_t)(out_h * out_w * 3));
  EXPECT(list_resize_host(src.data(), H, W, dst.data(), out_h, out_w) == LIST_OK);

  // refusals, none of which reaches the device
  EXPECT(list_resize_plan(&image, 1, src_bytes, out_h, out_w, plan, need - 1) == LIST_ERR_WORKSPACE);
  EXPECT(list_resize_plan(&image, 1, src_bytes - 1, out_h, out_w, plan, need) == LIST_ERR_ARG);
  image.offset = 1;
  EXPECT(list_resize_plan(&image, 1, src_bytes, out_h, out_w, plan, need) == LIST_ERR_ARG);
  image.offset = 0;
  EXPECT(list_resize_plan_bytes(&image, 0, out_h, out_w) == 0 && list_resize_plan_bytes(nullptr, 1, out_h, out_w) == 0);
  EXPECT(list_resize_workspace_bytes(&image, 1, 0, out_w) == 0);
  EXPECT(list_resize_host(nullptr, H, W, dst.data(), out_h, out_w) == LIST_ERR_ARG);
  float out = 0.0f;
  uint8_t ws[8] = {};
  EXPECT(list_resize_fwd(nullptr, src_bytes, plan, plan, need, nullptr, nullptr, &out, 0, ws, sizeof(ws), nullptr) == LIST_ERR_ARG);
  EXPECT(list_resize_fwd(src.data(), src_bytes, plan, plan, need, nullptr, nullptr, &out, 2, ws, sizeof(ws), nullptr) ==
         LIST_ERR_SHAPE);
  EXPECT(list_resize_fwd(src.data(), src_bytes, plan, plan, need - 1, nullptr, nullptr, &out, 0, ws, sizeof(ws), nullptr) ==
         LIST_ERR_WORKSPACE);
  EXPECT(list_resize_fwd(src.data(), src_bytes, plan, plan, need, nullptr, nullptr, &out, 0, ws, 0, nullptr) ==
         LIST_ERR_WORKSPACE);

  const bool ok = write_file(argv[6], dst.data(), dst.size()) && write_file(argv[7], plan, need);
  free(plan);
  return ok ? 0 : 2;
}
