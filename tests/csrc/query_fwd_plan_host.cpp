// Host program of tests/test_query_fwd_plan_cpu.py: plan_query_fwd and sort_has_pixel_order (csrc/query_fwd_plan.h) on calls
// read from standard input, one per line: a name, then key=value words (defaults in brackets)
//   prec=fp16|bf16|bf16x3 [fp16]  inf=0|1 [1]  img=map|proj|pfeat|pproj [map]  map16=0|1 [1]  vox16=0|1 [1]  kept=C [64]
//   no_fused=0|1  no_sort=0|1  ms=N [137]  R=N [128]  H1 H2 H3 [512 256 256]  fused=0..3 [1]  box=0|1 [1]  ride=0|1 [1]
//   gather_only=0|1  rows=N [768]  lK.C=V  lK.dims=D,H,W
// The pyramid is C = 1, 16, 32, 64, 128, 128 at R^3, R^3, (R/2)^3 .. (R/16)^3, dense and 16-byte aligned; the vector levels
// are fp16 with vox16, l0 fp32; img_C = 1024; the column offsets are the feature layout's (perceptual block, vector levels,
// scalar levels, xyz, padded to 64); rows = 768.  Output: "name sort l0,..,l5 box=mask img fc0 tail pix=0|1".
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "query_fwd_plan.h"

using namespace list;

int main() {
  alignas(16) static char somewhere[16];
  static const char* kSort[] = {"none", "morton", "morton+pixel"};
  static const char* kVox[] = {"scalar", "box", "near", "plain", "plain+ride", "invalid"};
  static const char* kImg[] = {"none", "f16", "f32", "copy", "projected", "kept", "kept+rowvec"};
  static const char* kFc0[] = {"gemm", "fused", "sampled"};
  static const char* kRv[] = {"-", "head", "lo", "behind_kept"};
  char line[1024];
  while (fgets(line, sizeof line, stdin)) {
    char* tok = strtok(line, " \n");
    if (!tok) continue;
    char name[128];
    snprintf(name, sizeof name, "%s", tok);
    ListQueryArgs a;
    memset(&a, 0, sizeof a);
    a.precision = LIST_PREC_FP16; a.no_activations = 1; a.img_dtype = LIST_MAP_F16; a.img_map = somewhere;
    a.map_size = 137; a.img_C = 1024; a.H1 = 512; a.H2 = 256; a.H3 = 256;
    int C[LIST_N_VOX_LEVELS] = {1, 16, 32, 64, 128, 128};
    int R = 128, vox16 = 1, kept = 64, fused = 1, box = 1, ride = 1, gather_only = 0, rows = 768, l = 0, v = 0;
    int dims[LIST_N_VOX_LEVELS][3] = {};
    while ((tok = strtok(nullptr, " \n"))) {
      char* eq = strchr(tok, '=');
      if (!eq) { fprintf(stderr, "%s: bad word %s\n", name, tok); return 2; }
      *eq = 0;
      const char* val = eq + 1;
      v = atoi(val);
      if (!strcmp(tok, "prec")) a.precision = !strcmp(val, "fp16") ? LIST_PREC_FP16 : !strcmp(val, "bf16") ? LIST_PREC_BF16 : LIST_PREC_BF16X3;
      else if (!strcmp(tok, "inf")) a.no_activations = v;
      else if (!strcmp(tok, "img")) {
        a.img_proj = !strcmp(val, "proj");
        a.percep_feat = !strcmp(val, "pfeat") ? (const float*)somewhere : nullptr;
        a.percep_proj = !strcmp(val, "pproj") ? somewhere : nullptr;
      }
      else if (!strcmp(tok, "map16")) a.img_dtype = v ? LIST_MAP_F16 : LIST_MAP_F32;
      else if (!strcmp(tok, "vox16")) vox16 = v;
      else if (!strcmp(tok, "kept")) kept = v;
      else if (!strcmp(tok, "no_fused")) a.no_fused_fc0 = v;
      else if (!strcmp(tok, "no_sort")) a.no_sort = v;
      else if (!strcmp(tok, "ms")) a.map_size = v;
      else if (!strcmp(tok, "R")) R = v;
      else if (!strcmp(tok, "H1")) a.H1 = v;
      else if (!strcmp(tok, "H2")) a.H2 = v;
      else if (!strcmp(tok, "H3")) a.H3 = v;
      else if (!strcmp(tok, "fused")) fused = v;
      else if (!strcmp(tok, "box")) box = v;
      else if (!strcmp(tok, "ride")) ride = v;
      else if (!strcmp(tok, "gather_only")) gather_only = v;
      else if (!strcmp(tok, "rows")) rows = v;
      else if (sscanf(tok, "l%d", &l) == 1 && l >= 0 && l < LIST_N_VOX_LEVELS && !strcmp(tok + 2, ".dims")) {
        if (sscanf(val, "%d,%d,%d", &dims[l][0], &dims[l][1], &dims[l][2]) != 3 || dims[l][0] <= 0 || dims[l][1] <= 0 || dims[l][2] <= 0) {
          fprintf(stderr, "%s: bad dims %s\n", name, val); return 2;
        }
      }
      else if (sscanf(tok, "l%d", &l) == 1 && l >= 0 && l < LIST_N_VOX_LEVELS && !strcmp(tok + 2, ".C")) C[l] = v;
      else { fprintf(stderr, "%s: bad key %s\n", name, tok); return 2; }
    }
    a.img_kept_C = a.img_proj ? kept : 0;
    int off[LIST_N_VOX_LEVELS], col = a.img_C;
    for (l = 0; l < LIST_N_VOX_LEVELS; ++l) if (C[l] != 1) { off[l] = col; col += LIST_N_STENCIL * C[l]; }
    for (l = 0; l < LIST_N_VOX_LEVELS; ++l) if (C[l] == 1) { off[l] = col; col += LIST_N_STENCIL; }
    const int Kp = (col + 3 + 63) / 64 * 64;
    for (l = 0; l < LIST_N_VOX_LEVELS; ++l) {
      const int res = l == 0 ? R : R >> (l - 1);
      ListVoxLevel& lv = a.vox[l];
      lv.data = somewhere; lv.C = C[l]; lv.D = lv.H = lv.W = res;
      if (dims[l][0]) { lv.D = dims[l][0]; lv.H = dims[l][1]; lv.W = dims[l][2]; }
      lv.image_stride = (int64_t)lv.D * lv.H * lv.W * C[l];
      lv.dtype = (vox16 && C[l] != 1 && C[l] % 8 == 0) ? LIST_MAP_F16 : LIST_MAP_F32;
    }
    const QueryFwdPlan p = plan_query_fwd({&a, Kp, 0, rows, off, fused, box != 0, ride != 0, gather_only != 0});
    printf("%s %s ", name, kSort[p.sort]);
    for (l = 0; l < LIST_N_VOX_LEVELS; ++l)
      printf("%s%s", p.vox[l] != VG_SCALAR ? kVox[p.vox[l]] : p.ride_level >= 0 ? "ride" : "tail", l + 1 < LIST_N_VOX_LEVELS ? "," : "");
    printf(" box=%d %s ", p.box_levels, kImg[p.img]);
    if (gather_only) { printf("- - pix=%d\n", (int)sort_has_pixel_order(a)); continue; }
    printf("%s/%d", kFc0[p.fc0], p.fc0_k);
    if (p.fc0 == FC0_FUSED) printf("/produced%d", p.n_produced);
    if (p.k_gap) printf("/gap%d+%d", p.k_gap_at, p.k_gap);
    printf("/%s %s pix=%d\n", kRv[p.rowvec], p.fused_tail ? "fused" : p.keep_h3 ? "two+h3" : "two", (int)sort_has_pixel_order(a));
  }
  return 0;
}
