// Which launches a forward query makes and in which form: the one statement of that rule.  list_sdf_query_fwd,
// list_query_plan and list_gather_features_fwd (list_capi.hip) compute it once per call; launch_sort_points and launch_gather
// (gather_kernels.hip) execute it.  Every form gives the right SDF, only slower: tests/test_query_fwd_plan_cpu.py pins the
// choice (plain C++17 on list_hip.h, built by a host compiler).
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "list_hip.h"
#include "vox_adjoint_plan.h"       // stencil_reach, kWindowReach

namespace list {

constexpr int kSortImages = 64;       // image slots in the point sort's key (b % 64)
constexpr int kSortPixCells = 8192;   // pixel-order bins per image of the point sort (>= ms * ceil(ms / 4))
constexpr int kBoxPts = 64;           // points per workgroup of the matrix-core gather (gather_box_kernels.hip)

// The point sort also produces the pixel order (order_img, row_of) that the 2-D gather kernel -- and, behind a training
// forward, the backward's map-side gather -- walks: sort on, per-point 2-D samples, the map fits the pixel bins
inline bool sort_has_pixel_order(const ListQueryArgs& a) {
  return !a.no_sort && !a.percep_feat && a.map_size * ((a.map_size + 3) / 4) <= kSortPixCells;
}

struct QueryFwdCall {
  const ListQueryArgs* a;          // validated (check_query_common); read: precision, img_dtype, map_size, img_C, img_kept_C,
                                   //   H1 .. H3, the flags, percep_feat / percep_proj (as flags), vox
  int Kp, img_off, rows;           // FeatLayout; rows of a chunk (a multiple of kRowTile)
  const int* vox_off;              // first column of X of every voxel level
  // LIST_FUSED_FC0: 1 unset; 0 ("0") keeps the unfused pair (2-D gather kernel + k_gemm_nt_pp); 2 ("x") runs the 128 x 512
  // tile with every K-tile from X (tile-shape diagnostic: the 2-D gather still runs); 3 ("3") forces it for bf16x3
  int fused_fc0_mode;
  bool gather_box, tail_ride;      // LIST_GATHER_BOX, LIST_TAIL_RIDE: false ("0") keeps k_gather_vox_near / k_gather_tail (A/B runs)
  bool gather_only;                // list_gather_features_fwd: no sort, no MLP
};

enum SortForm { SORT_NONE, SORT_MORTON, SORT_MORTON_PIXEL };
// a voxel level: C == 1, written by k_gather_tail or by the level that carries the ride | k_gather_vox_box | k_gather_vox_near |
// k_gather_vox | k_gather_vox writing the scalar level, xyz and the padding too | a channel count / dtype the dispatch does
// not know (hipErrorInvalidValue)
enum VoxGather { VG_SCALAR, VG_BOX, VG_NEAR, VG_PLAIN, VG_PLAIN_RIDE, VG_INVALID };
// the 2-D gather: no launch (fc_0 produces every perceptual column) | k_gather_img on an fp16 / fp32 map | k_copy_percep |
// the projected map (percep_proj) into the row vector | the kept channels of list_prep_img_proj's map alone, in the order of
// the rows | ... and the projected channels into the row vector
enum ImgGather { IMG_NONE, IMG_SAMPLE_F16, IMG_SAMPLE_F32, IMG_COPY, IMG_PROJECTED, IMG_KEPT, IMG_KEPT_ROWVEC };
// fc_0: k_gemm_nt_pp | k_fc0_fused, the 128 x 512 tile with n_produced leading K-tiles produced on chip | the 256 x 256 ping-pong
// kernel whose epilogue samples the projected channels (EPI_RELU_SAMPLE)
enum Fc0Form { FC0_GEMM, FC0_FUSED, FC0_SAMPLED };
// the fp32 row vector fc_0 adds in its epilogue: none | the head of the row's perceptual block (percep_proj) | the lo plane
// of X, unused by fp16 operands: rows * Kp * 2 >= rows * H1 * 4 | behind the kept columns (split formats: 4 B per column)
enum RowvecHome { ROWVEC_NONE, ROWVEC_X_HEAD, ROWVEC_X_LO, ROWVEC_BEHIND_KEPT };

struct QueryFwdPlan {
  SortForm sort;
  VoxGather vox[LIST_N_VOX_LEVELS];
  int ride_level;                  // the VG_PLAIN_RIDE level, or -1: k_gather_tail launches
  int box_levels;                  // bit l: level l is VG_BOX
  ImgGather img;
  Fc0Form fc0;
  int fc0_k, k_gap_at, k_gap;      // K of the fc_0 launch; K-tiles k_gap_at .. are read k_gap tiles further on (GemmParams)
  int n_produced;                  // FC0_FUSED
  RowvecHome rowvec;
  bool fused_tail, keep_h3;        // fc_1 + fc_2 + fc_out as k_mlp_tail_f16, or two GEMMs that keep H3 for a backward
};

// the stencil stays within one cell (what the window levels of the adjoint ask, from 16 channels on)
inline bool vox_level_is_near(const ListVoxLevel& lv) { return stencil_reach(lv) < kWindowReach && lv.C >= 16; }
// what the matrix-core gather accepts: fp16 maps and an fp16 feature matrix in 16-B pieces, 128 channels
inline bool gather_box_eligible(const QueryFwdCall& c, const ListVoxLevel& lv, int col_off) {
  if (!c.gather_box || c.a->precision != LIST_PREC_FP16 || lv.dtype != LIST_MAP_F16 || lv.C != 128) return false;
  if ((col_off % 8) != 0 || (c.Kp % 8) != 0 || (lv.image_stride % 8) != 0) return false;
  if (lv.W > 31 || lv.H > 31 || lv.D > 31) return false;       // 5-bit cell indices in the tile records
  return (c.rows % kBoxPts) == 0;
}

inline QueryFwdPlan plan_query_fwd(const QueryFwdCall& c) {
  const ListQueryArgs& a = *c.a;
  const bool fp16 = a.precision == LIST_PREC_FP16, map16 = a.img_dtype == LIST_MAP_F16;
  const int mode = c.fused_fc0_mode;
  QueryFwdPlan p;
  p.fc0 = FC0_GEMM; p.box_levels = 0; p.ride_level = -1;
  // ---- fc_0.  Both on-chip forms: inference forwards only -- list_sdf_query_bwd reads the WHOLE feature matrix (d fc_0.weight
  // = dZ1^T . X, the perceptual columns included), so a forward that a backward may follow materialises it -- with H1 = 512
  // and the perceptual block leading whole K-tiles
  const bool on_chip = !c.gather_only && a.no_activations && !a.no_fused_fc0 && a.H1 == 512 && a.img_C % 64 == 0 &&
                       c.img_off == 0 && c.Kp % 64 == 0;
  // k_fc0_fused (fused_fc0_kernels.hip) produces the per-point 2-D sample itself: no pre-pooled features, no projected map
  // (list_prep_img_proj's map leaves 2 perceptual K-tiles of 43: not worth the 128-row tile); fp16 operands with fp16 maps,
  // the bf16 formats with fp32 maps (the pairs the standard path takes too).  bf16x3 keeps the unfused path: its packed
  // weight is twice as long (hi + lo), and a 128-row tile streams ALL of it (7.3 MB per tile, 9.3 GB per 160 k points) --
  // measured (round 4): fc_0 1.15 -> 2.15 ms, step 3.58 -> 4.20 ms
  if (on_chip && mode != 0 && !a.percep_feat && !a.percep_proj && !a.img_proj && fp16 == map16 && a.img_C > 0 &&
      (a.precision != LIST_PREC_BF16X3 || mode == 3))
    p.fc0 = FC0_FUSED;
  // fp16 inference forwards on list_prep_img_proj's map: behind the kept-channels-only 2-D gather (modes 0 and 2 keep the
  // row-vector pair here too, as they keep the unfused pair on the standard path)
  if (on_chip && mode != 0 && mode != 2 && a.img_proj && fp16 && map16) p.fc0 = FC0_SAMPLED;
  p.n_produced = p.fc0 == FC0_FUSED && mode != 2 ? a.img_C / (fp16 ? 64 : 32) : 0;
  const int ktile = fp16 ? 64 : 32;                    // columns per 128-byte K-tile of X
  const int gap = a.img_proj ? a.img_C - a.img_kept_C : 0;
  p.fc0_k = c.Kp - (a.percep_proj ? a.img_C : gap);
  p.k_gap_at = a.img_proj ? a.img_kept_C / ktile : 0; p.k_gap = gap / ktile;
  p.rowvec = a.percep_proj ? ROWVEC_X_HEAD : !a.img_proj ? ROWVEC_NONE : fp16 ? ROWVEC_X_LO : ROWVEC_BEHIND_KEPT;
  // ---- the 2-D gather
  const bool in_fc0 = (p.fc0 == FC0_FUSED && mode != 2) || (p.fc0 == FC0_SAMPLED && a.img_kept_C == 0);
  p.img = in_fc0 ? IMG_NONE : a.percep_proj ? IMG_PROJECTED : a.img_proj ? (p.fc0 == FC0_SAMPLED ? IMG_KEPT : IMG_KEPT_ROWVEC)
          : a.percep_feat ? IMG_COPY : map16 ? IMG_SAMPLE_F16 : IMG_SAMPLE_F32;
  // ---- the sort.  A forward whose fc_0 samples the map itself (k_fc0_fused, or the sampling epilogue behind the
  // kept-channels gather, which runs in Morton order) sorts by Morton cell only: no projection per point, half the counters,
  // one scan and two index arrays less
  const bool samples_map = p.fc0 == FC0_SAMPLED || (p.fc0 == FC0_FUSED && mode != 2);
  p.sort = (c.gather_only || a.no_sort) ? SORT_NONE : (sort_has_pixel_order(a) && !samples_map) ? SORT_MORTON_PIXEL : SORT_MORTON;
  // ---- voxel levels
  int n_scalar = 0, scalar = 0;
  for (int l = 0; l < LIST_N_VOX_LEVELS; ++l) {
    const ListVoxLevel& lv = a.vox[l];
    const bool known = lv.C == 4 || (lv.C >= 8 && lv.C <= 256 && (lv.C & (lv.C - 1)) == 0);
    if (lv.C == 1) { p.vox[l] = VG_SCALAR; ++n_scalar; scalar = l; }
    else if (!known || (lv.dtype == LIST_MAP_F16 && lv.C < 8)) p.vox[l] = VG_INVALID;
    else if (!vox_level_is_near(lv)) p.vox[l] = VG_PLAIN;
    else if (gather_box_eligible(c, lv, c.vox_off[l])) { p.vox[l] = VG_BOX; p.box_levels |= 1 << l; }
    else p.vox[l] = VG_NEAR;
  }
  // The scalar level rides along with the vector level of the same grid (gather_pair, TailRide): one scalar level, fp32 in
  // place, and the first level of 8 .. 64 channels with its dimensions that takes k_gather_vox
  const ListVoxLevel& s0 = a.vox[scalar];
  for (int l = 0; l < LIST_N_VOX_LEVELS && p.ride_level < 0 && c.tail_ride && n_scalar == 1 && s0.dtype == LIST_MAP_F32; ++l) {
    const ListVoxLevel& lv = a.vox[l];
    if (p.vox[l] == VG_PLAIN && lv.C >= 8 && lv.C <= 64 && lv.D == s0.D && lv.H == s0.H && lv.W == s0.W &&
        (int64_t)lv.D * lv.H * lv.W * lv.C < ((int64_t)1 << 31)) {
      p.ride_level = l; p.vox[l] = VG_PLAIN_RIDE;
    }
  }
  // ---- fc_1, fc_2, fc_out: inference forwards in fp16 as ONE launch (gemm_kernels.hip, k_mlp_tail_f16).  Otherwise H3 is kept
  // with H1 / H2 for list_sdf_query_bwd (its head needs relu(fc_2): mask, dZ3, d fc_out.weight) -- by forwards a backward can
  // follow only: an inference forward that misses the fused tail (bf16 formats, the 256^3 grid of config 4 among them) would
  // write 1 KB per point that nobody reads
  p.fused_tail = !c.gather_only && a.no_activations && fp16 && a.H2 == 256 && a.H3 == 256 && a.H1 % 64 == 0;
  p.keep_h3 = !c.gather_only && !a.no_activations;
  return p;
}

}  // namespace list
