// Host program of tests/test_query_bwd_plan_cpu.py: plan_query_bwd (csrc/query_bwd_plan.h) on calls read from standard input, one
// per line: a name, then key=value words (defaults in brackets)
//   prec=fp16|bf16|bf16x3 [fp16]  B=N [2]  N=N [300]  ms=N [137]  no_sort=0|1  pfeat=0|1 (the pre-pooled form)  aux=0|2|3 [3]
//   ask=LIST [mlp,map,levels,trans,vox] of mlp (all eight), w0 b0 w1 b1 w2 b2 w3 b3, map, levels, trans, pfeat, vox; "-": nothing
//   map16=0|1 (grad_img_map_dtype = F16)  unordered=0|1 (LIST_BWD_TRANS_UNORDERED)  heavy=0|1 [1] (the workspace's scratch, or none)
//   pool=0|1 (list_percep_pool_bwd's call: aux = 0, no orders)
// img_C = 1024; rows = B * N padded to 256.  Output, one line:
//   name streams=<stream of main,direct,window,window2> colsum=L wgrad=L forks=<w2+w1|w2|w1|-> dw0=L[/early] main=<2-D stage on main>
//   trans=<none|inline@L|behind_dw0@L> event=0|1 resize=<none|f32|f16>
// with main = none | rows_to_grad | gather+heavy/f32 | gather/f16 | atomic/f32 | invalid, each with "+pix" where the 2-D adjoints
// walk the pixel order.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "query_bwd_plan.h"

using namespace list;

int main() {
  static const char* kLane[] = {"main", "direct", "window", "window2"};
  static const float somewhere[4] = {};
  char line[1024];
  while (fgets(line, sizeof line, stdin)) {
    char* tok = strtok(line, " \n");
    if (!tok) continue;
    char name[128];
    snprintf(name, sizeof name, "%s", tok);
    ListQueryArgs a;
    memset(&a, 0, sizeof a);
    a.precision = LIST_PREC_FP16; a.B = 2; a.N = 300; a.map_size = 137; a.img_C = 1024;
    QueryBwdCall c;
    memset(&c, 0, sizeof c);
    c.a = &a; c.n_aux = 3; c.Ct = a.img_C;
    char ask[256] = "mlp,map,levels,trans,vox";
    int heavy = 1;
    while ((tok = strtok(nullptr, " \n"))) {
      char* eq = strchr(tok, '=');
      if (!eq) { fprintf(stderr, "%s: bad word %s\n", name, tok); return 2; }
      *eq = 0;
      const char* val = eq + 1;
      const int v = atoi(val);
      if (!strcmp(tok, "prec")) a.precision = !strcmp(val, "fp16") ? LIST_PREC_FP16 : !strcmp(val, "bf16") ? LIST_PREC_BF16 : LIST_PREC_BF16X3;
      else if (!strcmp(tok, "B")) a.B = v;
      else if (!strcmp(tok, "N")) a.N = v;
      else if (!strcmp(tok, "ms")) a.map_size = v;
      else if (!strcmp(tok, "no_sort")) a.no_sort = v;
      else if (!strcmp(tok, "pfeat")) a.percep_feat = v ? somewhere : nullptr;
      else if (!strcmp(tok, "aux")) c.n_aux = v;
      else if (!strcmp(tok, "ask")) snprintf(ask, sizeof ask, "%s", val);
      else if (!strcmp(tok, "map16")) c.grad_img_map_f16 = v != 0;
      else if (!strcmp(tok, "unordered")) c.trans_unordered = v != 0;
      else if (!strcmp(tok, "heavy")) heavy = v;
      else if (!strcmp(tok, "pool")) c.pool = v != 0;
      else { fprintf(stderr, "%s: bad key %s\n", name, tok); return 2; }
    }
    for (char* w = strtok(ask, ","); w; w = strtok(nullptr, ",")) {
      MlpGradsAsked& m = c.mlp;
      if (!strcmp(w, "mlp")) m = {true, true, true, true, true, true, true, true};
      else if (!strcmp(w, "w0")) m.w0 = true; else if (!strcmp(w, "b0")) m.b0 = true;
      else if (!strcmp(w, "w1")) m.w1 = true; else if (!strcmp(w, "b1")) m.b1 = true;
      else if (!strcmp(w, "w2")) m.w2 = true; else if (!strcmp(w, "b2")) m.b2 = true;
      else if (!strcmp(w, "w3")) m.w3 = true; else if (!strcmp(w, "b3")) m.b3 = true;
      else if (!strcmp(w, "map")) c.grad_img_map = true;
      else if (!strcmp(w, "levels")) c.grad_img_levels = true;
      else if (!strcmp(w, "trans")) c.grad_trans_mat = true;
      else if (!strcmp(w, "pfeat")) c.grad_percep_feat = true;
      else if (!strcmp(w, "vox")) c.grad_vox = true;
      else if (strcmp(w, "-")) { fprintf(stderr, "%s: bad gradient %s\n", name, w); return 2; }
    }
    c.rows = ((int64_t)a.B * a.N + 255) / 256 * 256;
    c.heavy_bytes = heavy ? img_heavy_bytes(c.rows, c.Ct) : 0;
    const QueryBwdPlan p = plan_query_bwd(c);
    printf("%s streams=%s,%s,%s,%s colsum=%s wgrad=%s forks=%s dw0=%s%s main=", name, kLane[p.stream_of[0]], kLane[p.stream_of[1]],
           kLane[p.stream_of[2]], kLane[p.stream_of[3]], kLane[p.colsum], kLane[p.wgrad],
           p.fork_dw2 ? (p.fork_dw1 ? "w2+w1" : "w2") : p.fork_dw1 ? "w1" : "-", kLane[p.dw0], p.early ? "/early" : "");
    if (p.rows_to_grad) printf("rows_to_grad");
    else if (p.map == MAPGRAD_NONE) printf("none");
    else if (p.map == MAPGRAD_INVALID) printf("invalid");
    else printf("%s%s/%s", p.map == MAPGRAD_GATHER ? "gather" : "atomic", p.heavy ? "+heavy" : "", p.map_f16 ? "f16" : "f32");
    printf("%s trans=", p.pixel_order ? "+pix" : "");
    if (p.trans == TRANSGRAD_NONE) printf("none");
    else printf("%s@%s", p.trans == TRANSGRAD_INLINE ? "inline" : "behind_dw0", kLane[p.trans_lane]);
    printf(" event=%d resize=%s\n", (int)p.dw0_event, !p.resize ? "none" : p.resize_f16 ? "f16" : "f32");
  }
  return 0;
}
