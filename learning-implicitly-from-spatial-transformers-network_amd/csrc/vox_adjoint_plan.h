// Which kernel forms the gradient of voxel level l, on which stream, flushing how: the one statement of that rule, which
// launch_scatter_vox (bwd_scatter_kernels.hip) executes.  Every form gives the right gradient, only slower or at another
// precision grade: tests/test_vox_adjoint_plan_cpu.py pins the choice (plain C++17 on list_hip.h, built by a host compiler).
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "list_hip.h"

namespace list {

constexpr float kDisp = 0.0722f;    // stencil displacement, network/modules.py:205
// voxel-side gather: where the samples are dense enough and the level fits the sort's bins
constexpr int64_t kVoxGatherMaxBins = 4194304;      // cells (B * D * H * W) a level may have
constexpr double kVoxGatherMinDensity = 2.0;         // samples per cell
// a window level: wide channels and a stencil shorter than a voxel (the LDS-window kernel or the matrix-core adjoint)
constexpr float kWindowReach = 0.99f;
// ... whose boxes are small (8^3): 9216 floats of window (36 KB, four workgroups per CU); else (16^3, whose runs need
// ~100-voxel boxes) 18432 (72 KB, two per CU)
constexpr float kSmallBoxReach = 0.34f;
constexpr int kWinFloatsSmall = 9216, kWinFloatsLarge = 18432;
// fp16 image of a window level: kept at the gradient scale times kWinPkScale (headroom: a coarse voxel sums
// thousands of taps); the LDS-window kernel and the matrix-core adjoint flush at this one scale
constexpr float kWinPkScale = 0.0625f;
// the matrix-core adjoint (bwd_box_kernels.hip): its channel count and its points per workgroup
constexpr int kAdjC = 128, kAdjPts = 64;
// Direct forms, persistent grid (workgroups walk the 64-row blocks).  Alone, two workgroups per CU reach the atomic rate
// (512: 1.73 ms for the three fine levels; 128: +28 %, 64: 2.1x -- the rate is partly a per-CU issue
// limit).  Beside other kernels (ListQueryGradArgs.aux_streams) a small grid is better for the whole: the
// atomics of a CU fill its vector-memory queue, and every load of a neighbouring gather kernel waits behind
// them (backward 5.92 ms with 512 workgroups, 5.57 ms with 128).
// (re-measured in round 3 with dW0 capped at 194 registers: DESIGN 5b)
inline int direct_grid_cap(bool forked) { return forked ? 128 : 512; }

// form: no gradient asked for | voxel-side gather, a lane per (voxel, 8 channels) | ... per (voxel, channel) | global
// packed-half atomics, lanes over channel pairs | matrix-core adjoint | LDS window of VoxChoice.win_floats | global fp32
// atomics, lanes over channels | C == 1: a lane per tap | a channel count the dispatch does not know (hipErrorInvalidValue)
enum VoxForm { VOX_SKIP, VOX_GATHER8, VOX_GATHER1, VOX_DIRECT_H2, VOX_BOX, VOX_WINDOW, VOX_DIRECT, VOX_SCALAR, VOX_INVALID };
enum VoxLane { VOX_LANE_GATHER, VOX_LANE_DIRECT, VOX_LANE_WINDOW, VOX_LANE_WINDOW2 };      // ScatterStreams, in its order
// flush: every voxel written once | fp32 atomics into the memset gradient | packed halfs into the direct level's scratch
// (then one pass to fp32) | ... into slot 0 | slot 1 of the window levels' scratch
enum VoxFlush { VOX_FLUSH_STORE, VOX_FLUSH_F32, VOX_FLUSH_H16, VOX_FLUSH_H16W0, VOX_FLUSH_H16W1 };

struct VoxCall {
  int n_valid, rows, B, Kp;        // rows: padded; B: images the points reach
  bool dx_f16, forked;
  int mode;                        // ListQueryGradArgs.vox_adjoint
  bool gather_buffers;             // the voxel-side gather has its keys / bins / records
  size_t h16_bytes, h16w_bytes;    // scratch of the packed-half forms; 0: absent
  // LIST_SCATTER_BOX: which window levels take the matrix-core adjoint -- 0 neither, 1 the 8^3 level, 3 the 16^3 level,
  // 2 both; unset (-1): the 16^3 level, and the 8^3 level when the call is not forked
  int box_mode;
  bool f32_diagnostic;             // LIST_SCATTER_F32=1 (for the tests): the window levels flush fp32 atomics (both kernels)
};
struct VoxChoice { VoxForm form; VoxLane lane; VoxFlush flush; int win_floats; };

// stencil displacement in voxels of the level's longest axis
inline float stencil_reach(const ListVoxLevel& gv) {
  const int big = gv.W > gv.H ? (gv.W > gv.D ? gv.W : gv.D) : (gv.H > gv.D ? gv.H : gv.D);
  return kDisp * 0.5f * (float)(big - 1);
}
inline bool is_window_level(const ListVoxLevel& gv) { return gv.C >= 64 && stencil_reach(gv) < kWindowReach; }
// two window levels at most share the scratch
inline size_t h16w_slot_bytes(size_t h16w_bytes) { return h16w_bytes / 2 / 256 * 256; }
// the level's fp16 image can stand in for its gradient: images back to back, whole 16-B pieces, within `bytes`
inline bool h16_image_fits(const VoxCall& c, const ListVoxLevel& gv, size_t bytes) {
  const size_t n_elem = (size_t)c.B * gv.image_stride;
  return n_elem * 2 <= bytes && n_elem % 8 == 0 && gv.image_stride == (int64_t)gv.D * gv.H * gv.W * gv.C;
}
// what the matrix-core adjoint accepts: 128 channels, 16-B pieces of dX (fp32 dX: bf16 hi + lo operands), channel pairs of
// the fp16 image
inline bool scatter_box_eligible(const VoxCall& c, const ListVoxLevel& gv, int col_off) {
  const int piece = c.dx_f16 ? 8 : 4;
  if (gv.C != kAdjC || (col_off % piece) != 0 || (c.Kp % piece) != 0) return false;
  if (c.dx_f16 && (gv.image_stride % 2) != 0) return false;
  if (gv.W > 255 || gv.H > 255 || gv.D > 255) return false;   // 8-bit coordinates in the run records
  return (c.rows % kAdjPts) == 0;
}

// per level (LIST_N_VOX_LEVELS of each): its gradient (data null: not asked for), its first column of dX, the choice
inline void plan_vox_adjoint(const VoxCall& c, const ListVoxLevel* levels, const int* col_offs, VoxChoice* out) {
  int n_win_pk = 0, n_win_seen = 0;
  for (int l = 0; l < LIST_N_VOX_LEVELS; ++l) {
    const ListVoxLevel& gv = levels[l];
    VoxChoice& r = out[l] = {VOX_SKIP, VOX_LANE_DIRECT, VOX_FLUSH_F32, 0};
    if (!gv.data) continue;
    // voxel-side gather where the samples are dense enough: at least kVoxGatherMinDensity samples per cell
    const int64_t n_vox = (int64_t)c.B * gv.D * gv.H * gv.W;
    const bool window_level = is_window_level(gv), wide = gv.C == 64 || gv.C == 128 || gv.C == 256;
    const bool dense = c.mode == 2 || (c.mode == 0 && !window_level &&
                                       (double)c.n_valid * LIST_N_STENCIL >= kVoxGatherMinDensity * (double)n_vox);
    if (c.gather_buffers && dense && n_vox <= kVoxGatherMaxBins && (gv.C == 16 || gv.C == 32 || wide)) {
      // 16-B pieces of dX and of the gradient, or a lane per channel
      const bool lanes8 = (col_offs[l] % 8) == 0 &&(c.Kp % 8) == 0 && ((uintptr_t)gv.data & 15) == 0;
      r = {lanes8 ? VOX_GATHER8 : VOX_GATHER1, VOX_LANE_GATHER, VOX_FLUSH_STORE, 0};
      continue;
    }
    // the first window level shares its stream with dW0; the second one has a stream to itself (window2: the
    // library's own side stream when the backward is forked, else the caller's).  With both behind the (contended) 2-ms
    // dW0 the window stream ended 0.4 ms after the other two (forked backward 5.16 -> 4.98 ms with the second one behind
    // the gathers on the caller's stream); on its own stream the training step is the same with the synthetic camera
    // and 0.17 - 0.22 ms shorter with the points on the clamp, where the gathers ahead of it are the long ones
    // (profiles/r04b_window_streams_ab.txt, which also has the first level on its own stream: +1.4 ms; with the 16^3 level
    // on the matrix cores the other orders were measured again -- both levels on window2, the 16^3 level behind the
    // gathers: +0.08 / +0.4 ms, profiles/r04b_box_adjoint.txt)
    if (window_level && c.mode != 2) { r.lane = n_win_seen == 0 ? VOX_LANE_WINDOW : VOX_LANE_WINDOW2; ++n_win_seen; }
    // packed-half atomics (see k_scatter_vox_h2): fp16 operands, automatic form choice, C = 32 or a non-window C = 64
    // level, and the level's fp16 image fits the scratch the caller set aside
    if (c.dx_f16 && c.mode == 0 && !window_level && (gv.C == 32 || gv.C == 64) && c.h16_bytes != 0 &&
        h16_image_fits(c, gv, c.h16_bytes)) {
      r.form = VOX_DIRECT_H2; r.flush = VOX_FLUSH_H16;
      continue;
    }
    // window levels, fp16 operands: packed-half flush into the level's fp16 image (its own scratch slot: the window
    // levels run beside the direct ones), then one pass to fp32
    if (window_level && wide) {
      if (c.dx_f16 && c.mode == 0 && c.h16w_bytes != 0 && !c.f32_diagnostic && n_win_pk < 2 &&
          h16_image_fits(c, gv, h16w_slot_bytes(c.h16w_bytes)))
        r.flush = (n_win_pk++ & 1) ? VOX_FLUSH_H16W1 : VOX_FLUSH_H16W0;
      const bool img16 = r.flush != VOX_FLUSH_F32;
      const bool small_box = stencil_reach(gv) < kSmallBoxReach;
      // 128 channels: on the matrix cores (k_scatter_vox_box).  16^3: alone 0.52 -> 0.24 ms, forked step 6.63 -> 6.29 ms.
      // 8^3: alone 0.28 -> 0.12 ms; beside the other streams of the forked backward the VALU kernel is the better
      // neighbour (2 waves of 199 registers per workgroup against 4 of 243: step +0.05 ms with the matrix-core form), so
      // forked calls keep it unless LIST_SCATTER_BOX=2
      const bool box = small_box ? (c.box_mode < 0 ? !c.forked : (c.box_mode == 1 || c.box_mode == 2))
                                 : (c.box_mode < 0 || c.box_mode == 2 || c.box_mode == 3);
      // fp16 dX: into the fp16 image, or (diagnostic) fp32 atomics; fp32 dX (bf16x3, bf16): bf16 hi + lo operands
      if (box && (c.dx_f16 ? (img16 || c.f32_diagnostic) : true) && scatter_box_eligible(c, gv, col_offs[l])) r.form = VOX_BOX;
      else { r.form = VOX_WINDOW; r.win_floats = small_box ? kWinFloatsSmall : kWinFloatsLarge; }
      continue;
    }
    r.form = gv.C == 1 ? VOX_SCALAR : (gv.C == 4 || gv.C == 8 || gv.C == 16 || gv.C == 32 || wide) ? VOX_DIRECT : VOX_INVALID;
  }
}

}  // namespace list
