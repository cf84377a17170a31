// Host program of tests/test_vox_adjoint_plan_cpu.py: plan_vox_adjoint (csrc/vox_adjoint_plan.h) on calls read from
// standard input, one per line:
//   name B N R fp16 forked mode gather_buffers box_mode f32_diagnostic offset_shift [edit ...]
// The pyramid is C = 1, 16, 32, 64, 128, 128 at R^3, R^3, (R/2)^3 .. (R/16)^3, dense, 16-byte-aligned, non-null, at the
// column offsets of make_layout for img_C = 1024 (plus offset_shift), Kp = 3648; rows = B * N rounded up to 256, the
// scratch rows x 512 and rows x 256 halfs when fp16.  Edits change one level first: lK.null, lK.C=V, lK.stride+V,
// lK.dims=D,H,W (the level's size, dense) and lK.off=V (its column offset, the shift included).
// Output: one line "name l form/lane/flush" per level.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "vox_adjoint_plan.h"

using namespace list;

int main() {
  alignas(16) static char somewhere[16];
  static const int kC[LIST_N_VOX_LEVELS] = {1, 16, 32, 64, 128, 128};
  static const int kOff[LIST_N_VOX_LEVELS] = {3600, 1024, 1136, 1360, 1808, 2704};
  static const char* kForm[] = {"skip", "gather8", "gather1", "direct_h2", "box", "win", "direct", "scalar", "invalid"};
  static const char* kLane[] = {"gather", "direct", "window", "window2"};
  static const char* kFlush[] = {"st", "f32", "h16", "w0", "w1"};
  char line[1024];
  while (fgets(line, sizeof line, stdin)) {
    char* tok = strtok(line, " \n");
    if (!tok) continue;
    char name[128];
    snprintf(name, sizeof name, "%s", tok);
    long v[10];
    for (int i = 0; i < 10; ++i) {
      tok = strtok(nullptr, " \n");
      if (!tok) { fprintf(stderr, "%s: too few fields\n", name); return 2; }
      v[i] = atol(tok);
    }
    const int B = (int)v[0], N = (int)v[1], R = (int)v[2];
    const bool fp16 = v[3] != 0;
    VoxCall c;
    c.n_valid = B * N; c.rows = (B * N + 255) / 256 * 256; c.B = B; c.Kp = 3648;
    c.dx_f16 = fp16; c.forked = v[4] != 0; c.mode = (int)v[5]; c.gather_buffers = v[6] != 0;
    c.h16_bytes = fp16 ? (size_t)c.rows * 512 * 2 : 0; c.h16w_bytes = fp16 ? (size_t)c.rows * 256 * 2 : 0;
    c.box_mode = (int)v[7]; c.f32_diagnostic = v[8] != 0;
    ListVoxLevel lv[LIST_N_VOX_LEVELS];
    int col_off[LIST_N_VOX_LEVELS];
    for (int l = 0; l < LIST_N_VOX_LEVELS; ++l) {
      const int res = l == 0 ? R : R >> (l - 1);
      ListVoxLevel& gv = lv[l];
      memset(&gv, 0, sizeof gv);
      gv.data = somewhere; gv.C = kC[l]; gv.D = gv.H = gv.W = res;
      gv.image_stride = (int64_t)res * res * res * kC[l];
      col_off[l] = kOff[l] + (int)v[9];
    }
    while ((tok = strtok(nullptr, " \n"))) {
      int l = -1, val = 0, d = 0, h = 0, w = 0;
      if (sscanf(tok, "l%d.dims=%d,%d,%d", &l, &d, &h, &w) == 4 && l >= 0 && l < LIST_N_VOX_LEVELS && d > 0 && h > 0 && w > 0) {
        lv[l].D = d; lv[l].H = h; lv[l].W = w;
        lv[l].image_stride = (int64_t)d * h * w * lv[l].C;
      } else if (sscanf(tok, "l%d.off=%d", &l, &val) == 2 && l >= 0 && l < LIST_N_VOX_LEVELS) {
        col_off[l] = val;
      } else if (sscanf(tok, "l%d.C=%d", &l, &val) == 2 && l >= 0 && l < LIST_N_VOX_LEVELS) {
        lv[l].C = val;
        lv[l].image_stride = (int64_t)lv[l].D * lv[l].H * lv[l].W * val;
      } else if (sscanf(tok, "l%d.stride+%d", &l, &val) == 2 && l >= 0 && l < LIST_N_VOX_LEVELS) {
        lv[l].image_stride += val;
      } else if (tok[0] == 'l' && tok[1] >= '0' && tok[1] < '0' + LIST_N_VOX_LEVELS && !strcmp(tok + 2, ".null")) {
        lv[tok[1] - '0'].data = nullptr;
      } else { fprintf(stderr, "%s: bad edit %s\n", name, tok); return 2; }
    }
    VoxChoice out[LIST_N_VOX_LEVELS];
    plan_vox_adjoint(c, lv, col_off, out);
    for (int l = 0; l < LIST_N_VOX_LEVELS; ++l) {
      const VoxChoice& p = out[l];
      if (p.form == VOX_SKIP) printf("%s %d skip\n", name, l);
      else if (p.form == VOX_WINDOW) printf("%s %d win%d/%s/%s\n", name, l, p.win_floats / 1024, kLane[p.lane], kFlush[p.flush]);
      else printf("%s %d %s/%s/%s\n", name, l, kForm[p.form], kLane[p.lane], kFlush[p.flush]);
    }
  }
  return 0;
}
