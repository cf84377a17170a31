// Which form and which stream every stage of the query's backward takes behind the MLP chain: the one statement of that rule.
// list_sdf_query_bwd and list_percep_pool_bwd (list_capi.hip) compute it once per call and execute it; launch_img_map_grad
// (bwd_img_kernels.hip) executes the map gradient's part; the voxel levels between dW0 and the 2-D adjoints are
// plan_vox_adjoint's (vox_adjoint_plan.h).  Every form and order gives the same gradients, only slower:
// tests/test_query_bwd_plan_cpu.py pins the choice (plain C++17 on list_hip.h, built by a host compiler).
// The call, top-down (lanes in brackets; a hand-over makes the second stream continue behind the first one's work so far):
//   head, chain   scale, dZ3, dH2, dH1 [main]; each column sum [colsum, behind a hand-over from main]; dW2, dW1 [wgrad, behind a
//                 hand-over from main where fork_dw2 / fork_dw1]
//   early form    hand-over window -> main, dW0 [main], hand-over direct -> main; window2 is never forked
//   else          dX [main]; hand-overs main -> direct, window, window2; dW0 [window] and its event; the voxel levels; on main
//                 rows-to-gradient or the map gradient, the trans_mat gradient in line, the adjoint resize; the trans_mat
//                 gradient behind dW0's event [trans lane]; hand-overs direct, window, window2 -> main
// The stage events (ListQueryGradArgs.stage_events) are recorded by list_sdf_query_bwd, never by a launcher, on main behind
// their stage (WGRAD2 / WGRAD1 / WGRAD0 forked: the enqueue time only; the early form: DGRAD0 .. TRANS behind dW0) -- but IMG and
// TRANS on the trans_mat gradient's lane, right ahead of it and right behind it: in line, IMG closes the map gradient (or
// rows-to-gradient) ahead of the resize; behind dW0's event, IMG follows the wait, so that with two auxiliary streams (trans lane
// = main) it covers the resize as well.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "list_hip.h"
#include "query_fwd_plan.h"         // sort_has_pixel_order, kSortImages, kSortPixCells
#include "vox_adjoint_plan.h"       // VoxLane

namespace list {

// map-side gather of the perceptual-map gradient: chunks of its heavy groups (bwd_img_kernels.hip, kHeavyChunk =
// 1024 candidates).  Every point is a candidate of at most 4 groups, so the chunks of groups above 1024 candidates
// number at most 4 rows / 1024 whole ones plus one partial chunk per heavy group (<= 4 rows / 1024 of those).
inline int img_heavy_max_chunks(int64_t rows) { return (int)(8 * rows / 1024 + 8); }
inline size_t img_heavy_bytes(int64_t rows, int Ct) {
  return 256 + (size_t)kSortImages * kSortPixCells * 4 + (size_t)img_heavy_max_chunks(rows) * 8 + 256 +
         (size_t)img_heavy_max_chunks(rows) * 4 * Ct * 4;
}

struct MlpGradsAsked { bool w0, b0, w1, b1, w2, b2, w3, b3; };      // ListMlpGrads, as flags
struct QueryBwdCall {
  const ListQueryArgs* a;          // validated; read: B, map_size, no_sort, percep_feat (as a flag), precision
  MlpGradsAsked mlp;
  bool grad_img_map, grad_img_map_f16, grad_img_levels, grad_trans_mat, grad_percep_feat, grad_vox;     // grad_vox: any level
  int n_aux;                       // auxiliary streams the caller gave: 0, 2 or 3 (ListQueryGradArgs.aux_streams)
  int64_t rows;                    // padded rows of the call
  int Ct;                          // channels of the perceptual map
  size_t heavy_bytes;              // scratch of the gather's heavy groups; 0: none
  bool trans_unordered;            // LIST_BWD_TRANS_UNORDERED=1 (diagnostic, below)
  bool pool;                       // list_percep_pool_bwd's call: a point set without orders, on the main stream only
};

// lanes: VoxLane, in ScatterStreams' order; its first one (the voxel-side gather's) is the caller's stream
constexpr VoxLane kLaneMain = VOX_LANE_GATHER;
// the perceptual map's gradient: not asked | every map pixel gathers the candidates of its <= 4 pixel cells (k_img_grad_gather; no
// atomics, written once) | memset + k_img_grad_atomic | a half-precision map (the intermediate of the adjoint resize) without
// the gather form or without fp16 operands: list_sdf_query_bwd refuses it before it plans (hipErrorInvalidValue otherwise)
enum MapGradForm { MAPGRAD_NONE, MAPGRAD_GATHER, MAPGRAD_ATOMIC, MAPGRAD_INVALID };
// the trans_mat gradient: not asked | right behind the map gradient, ahead of the adjoint resize | behind dW0's event
enum TransGradForm { TRANSGRAD_NONE, TRANSGRAD_INLINE, TRANSGRAD_BEHIND_DW0 };

struct QueryBwdPlan {
  bool forked;                     // the stages run side by side on the caller's auxiliary streams (ScatterParams.forked)
  VoxLane stream_of[4];            // by lane: the lane whose stream it runs on (main; direct, window, window2 = aux_streams[0 .. 2])
  VoxLane colsum, wgrad;           // the column sums; dW2 and dW1
  bool fork_dw2, fork_dw1;         // a hand-over main -> wgrad lane ahead of dW2 / dW1
  bool early;                      // no gradient behind dX is asked: the early form (above), dW0 on main
  VoxLane dw0;
  bool rows_to_grad;               // the pre-pooled form's grad_percep_feat, on main
  bool pixel_order;                // the 2-D adjoints walk the points in the forward's pixel order (order_img, row_of), else in row order
  MapGradForm map;                 // on main
  bool heavy, map_f16;             // MAPGRAD_GATHER: the heavy groups are planned; the map holds halfs at the gradient scale
  TransGradForm trans;
  VoxLane trans_lane;
  bool dw0_event;                  // dW0's event exists (recorded on the window lane, waited for on the trans lane)
  bool resize, resize_f16;         // the adjoint resize runs inside the call, on main behind the map gradient; it reads halfs
};

// The 2-D adjoints have the pixel order, and the map gradient takes the gather form, iff the forward's sort left one and
// every image has a slot of its own in the sort's key (B > kSortImages: images share slots, the pixel bins of a slot mix them)
inline bool map_grad_gathers(const ListQueryArgs& a) { return sort_has_pixel_order(a) && a.B <= kSortImages; }

inline QueryBwdPlan plan_query_bwd(const QueryBwdCall& c) {
  const ListQueryArgs& a = *c.a;
  const bool forked = !c.pool && c.n_aux >= 2;
  const bool prepooled = !c.pool && a.percep_feat != nullptr;
  QueryBwdPlan p;
  p.forked = forked;
  // window2 is the third auxiliary stream, or main when there are only two
  p.stream_of[kLaneMain] = kLaneMain;
  p.stream_of[VOX_LANE_DIRECT] = forked ? VOX_LANE_DIRECT : kLaneMain;
  p.stream_of[VOX_LANE_WINDOW] = forked ? VOX_LANE_WINDOW : kLaneMain;
  p.stream_of[VOX_LANE_WINDOW2] = forked && c.n_aux >= 3 ? VOX_LANE_WINDOW2 : kLaneMain;
  // The bias / fc_out.weight column sums feed nothing downstream: forked, they leave the chain of dependent GEMMs
  // and run on the atomics' stream, which has nothing to do until dX exists (same kernels, same order among
  // themselves -- they share the `colsum` scratch).
  p.colsum = p.stream_of[VOX_LANE_DIRECT];
  // forked: the weight gradients feed nothing downstream either -- they queue up on the window stream, in the order
  // dW2, dW1, dW0 because they share the split-K slab, while the data-gradient chain continues on main
  p.wgrad = p.stream_of[VOX_LANE_WINDOW];
  p.fork_dw2 = forked && c.mlp.w2;
  p.fork_dw1 = forked && c.mlp.w1;
  p.early = !c.pool && !(c.grad_img_map || c.grad_trans_mat || c.grad_percep_feat || c.grad_vox);
  p.dw0 = p.early ? kLaneMain : p.wgrad;               // (early: behind a hand-over window -> main, dW0 shares the slab with dW2 / dW1)
  // dX is ready on main.  From here the work is a DAG of stages bound by different units: dW0 (MFMA; needs only
  // dZ1 and X) and the 16^3 LDS-window level on one stream, the atomic-rate-bound levels on another, the 8^3 window level
  // on the third (aux_streams[2]; without it, behind the gathers), the gathers (voxel-side gather, perceptual map,
  // trans_mat) on main.  Without auxiliary streams: the same order, in line.
  p.rows_to_grad = !p.early && prepooled && c.grad_percep_feat;
  // ---- the map gradient
  p.pixel_order = !c.pool && map_grad_gathers(a);
  p.map_f16 = c.grad_img_map_f16;
  p.map = (p.early || prepooled || !c.grad_img_map) ? MAPGRAD_NONE
          : (p.map_f16 && (!p.pixel_order || a.precision != LIST_PREC_FP16)) ? MAPGRAD_INVALID
          : p.pixel_order ? MAPGRAD_GATHER : MAPGRAD_ATOMIC;
  // The heavy groups (bwd_img_kernels.hip): the scratch holds them and the groups fit its group_base.  Both hold for every call
  // list_sdf_query_bwd accepts -- its workspace layout sets img_heavy_bytes(rows, Kp) aside with Kp >= Ct, and the gather form
  // has B <= kSortImages images of map_size * ceil(map_size / 4) <= kSortPixCells groups; list_percep_pool_bwd never gathers
  p.heavy = p.map == MAPGRAD_GATHER && c.heavy_bytes != 0 && c.heavy_bytes >= img_heavy_bytes(c.rows, c.Ct) &&
            (int64_t)a.B * a.map_size * ((a.map_size + 3) / 4) <= (int64_t)kSortImages * kSortPixCells;
  // ---- the trans_mat gradient
  // Forked, k_trans_grad must not run while dW0 does.  Whenever one of its waves shared a SIMD with the weight-gradient
  // GEMM's (2 x 216 + 80 registers = the whole file in the split formats), ONE point's v-derivative came out different --
  // d_trans_mat off by 1e-4 .. 7e-3 of its largest entry in 4 - 59 of 60 calls, depending on what else ran (tools/
  // trans_noise_probe2.py, profiles/r04b_trans_mat_interference.txt: never with dW0 left out, never in line, never once
  // the kernel held more registers or LDS than fit beside dW0; its inputs, its LDS records and every other gradient
  // were bit-stable).  It was later localised to the one ds_bpermute pair of the kernel's loop, which is gone
  // (bwd_img_kernels.hip); the order stays as a second fence and removes the overlap: map gradient, adjoint
  // resize (it needs only the map gradient), then -- behind dW0's event -- the trans_mat gradient.  In line the stages
  // keep their order (and their stage events their meaning).
  // (LIST_BWD_TRANS_UNORDERED=1, diagnostic: the old order -- the stage right behind the map gradient, beside dW0 --
  // for tools/trans_noise_probe2.py)
  p.trans = (p.early || prepooled || !c.grad_trans_mat) ? TRANSGRAD_NONE
            : (forked && !c.trans_unordered) ? TRANSGRAD_BEHIND_DW0 : TRANSGRAD_INLINE;
  // ... on aux_streams[2] where there is one (idle once the 8^3 window level is done; window2 is main otherwise)
  // instead of at the end of main: training step 6.43 -> 6.36 ms, 6.52 -> 6.32 with the points on the clamp
  p.trans_lane = p.trans == TRANSGRAD_BEHIND_DW0 ? p.stream_of[VOX_LANE_WINDOW2] : kLaneMain;
  p.dw0_event = p.trans == TRANSGRAD_BEHIND_DW0;
  // ---- the adjoint resize: needs only the map gradient
  p.resize = p.map != MAPGRAD_NONE && c.grad_img_levels;
  p.resize_f16 = p.resize && p.map_f16;
  return p;
}

}  // namespace list
