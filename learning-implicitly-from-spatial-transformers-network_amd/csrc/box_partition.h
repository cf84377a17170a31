// The front end shared by the matrix-core gather of the coarse voxel levels (gather_box_kernels.hip) and its adjoint
// (bwd_box_kernels.hip): the per-point weight records and tap ranges (step 1a), the segment tree that cuts a
// workgroup's 64 Morton-consecutive points into aligned power-of-two runs whose voxel box fits the LDS box (step 1b),
// and the decoded run with its box row -> voxel arithmetic.
#pragma once
#include "list_common.h"
#include "point_math.h"

namespace list {

typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((ext_vector_type(8))) short s16x8;

struct AxisW { int i0; float w0, w1; };                     // base index; w1 = 0 where the +1 tap is skipped
struct RunBox { int lo, n, b, count; };                     // lo / n: x | y << 8 | z << 16 (n = 0: no valid point)

__device__ __forceinline__ s16x4 tr_read16(const char* l) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)l);
}
__device__ __forceinline__ int uni(int x) { return __builtin_amdgcn_readfirstlane(x); }

// fp32 pair -> packed fp16 pair (a in the low half), RNE, no clamp (weights lie in [0, 1])
__device__ __forceinline__ unsigned pk_h2(float a, float b) {
  const f32x2_t v = {a, b};
  return __builtin_bit_cast(unsigned, __builtin_convertvector(v, f16x2_t));
}

// variant of axis `ax` under stencil point j: 0 = centre coordinate, 1 = -d, 2 = +d (network/modules.py:205-214)
__device__ __forceinline__ int variant_of(int ax, int j) { return j == 2 * ax + 1 ? 1 : (j == 2 * ax + 2 ? 2 : 0); }

// ---- partition of the 64 points into runs (one wave, one point per lane) ----------------------------------------
// Tap ranges travel as minima of 16-bit fields (an upper bound hi as 255 - hi): f0 = lo_x | lo_y << 16,
// f1 = lo_z | (255 - hi_x) << 16, f2 = (255 - hi_y) | (255 - hi_z) << 16; images as bmin and ~bmax.  A point that is
// not valid carries the neutral element everywhere.
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ unsigned pk_min16(unsigned a, unsigned b) {
  return __builtin_bit_cast(unsigned, __builtin_elementwise_min(__builtin_bit_cast(u16x2, a), __builtin_bit_cast(u16x2, b)));
}
struct SegBox { unsigned f0, f1, f2; int bmin, nbmax; };
template <int STAGE>
__device__ __forceinline__ int seg_xchg(int v) {
  // the partner half of the aligned 2^(STAGE+1) segment: every lane of a half holds the half's value already, so
  // any lane of the other half will do (quad permutes, then the row mirrors, then across rows)
  if (STAGE == 0) return __builtin_amdgcn_update_dpp(v, v, 0xB1, 0xf, 0xf, true);      // quad_perm [1,0,3,2]
  if (STAGE == 1) return __builtin_amdgcn_update_dpp(v, v, 0x4E, 0xf, 0xf, true);      // quad_perm [2,3,0,1]
  if (STAGE == 2) return __builtin_amdgcn_update_dpp(v, v, 0x141, 0xf, 0xf, true);     // row_half_mirror
  if (STAGE == 3) return __builtin_amdgcn_update_dpp(v, v, 0x140, 0xf, 0xf, true);     // row_mirror
  return __shfl_xor(v, 1 << STAGE);
}
template <int STAGE>
__device__ __forceinline__ void seg_merge(SegBox& b) {
  b.f0 = pk_min16(b.f0, (unsigned)seg_xchg<STAGE>((int)b.f0));
  b.f1 = pk_min16(b.f1, (unsigned)seg_xchg<STAGE>((int)b.f1));
  b.f2 = pk_min16(b.f2, (unsigned)seg_xchg<STAGE>((int)b.f2));
  b.bmin = min(b.bmin, seg_xchg<STAGE>(b.bmin));
  b.nbmax = min(b.nbmax, seg_xchg<STAGE>(b.nbmax));
}
__device__ __forceinline__ bool seg_fits(const SegBox& b, int maxrows, int maxkeys) {
  if (b.bmin == INT_MAX) return true;                         // no valid point
  if (b.bmin != ~b.nbmax) return false;                       // two images
  const int lox = b.f0 & 0xffff, loy = b.f0 >> 16, loz = b.f1 & 0xffff;
  const int hix = 255 - (int)(b.f1 >> 16), hiy = 255 - (int)(b.f2 & 0xffff), hiz = 255 - (int)(b.f2 >> 16);
  const int nx = hix - lox + 1, ny = hiy - loy + 1, nz = hiz - loz + 1;
  const int nfw = (hix >> 2) - (lox >> 2) + 1;
  return nx * ny * nz <= maxrows && nfw * ny * nz <= maxkeys;
}

// ---- step 1a, waves 0..2: axis `axis` of point `lane` of the workgroup (row `row` of the query) ------------------
// ptab [64][3 axes][3 variants]: the weight records of the centre / -d / +d coordinate; pbox [64][4]: the tap range
// lo | hi << 8 of each axis, and (written by axis 0) the point's image, -1 where the point is not valid
__device__ __forceinline__ void box_point_records(const GatherParams& g, int row, int lane, int axis, int W, int H, int D,
                                                  AxisW* ptab, int* pbox) {
  const Pt p = load_point(g, row);
  const float c = axis == 0 ? p.x : (axis == 1 ? p.y : p.z);
  const int S = axis == 0 ? W : (axis == 1 ? H : D);
  const Axis a[3] = {axis_setup(c, S), axis_setup(c - kDisp, S), axis_setup(c + kDisp, S)};
#pragma unroll
  for (int v = 0; v < 3; ++v) {
    AxisW e;
    e.i0 = a[v].i0;
    e.w0 = p.valid ? a[v].w0 : 0.f;
    e.w1 = (p.valid && a[v].has1) ? a[v].w1 : 0.f;
    ptab[(lane * 3 + axis) * 3 + v] = e;
  }
  pbox[lane * 4 + axis] = a[1].i0 | ((a[2].i0 + a[2].has1) << 8);
  if (axis == 0) pbox[lane * 4 + 3] = p.valid ? p.b : -1;
}

// ---- step 1b, wave 0: runs[first point] for the aligned power-of-two runs whose box has at most MAXROWS rows and
// MAXKEYS window keys (a single point always fits: 4 x 4 x 4) ------------------------------------------------------
template <int MAXROWS, int MAXKEYS>
__device__ __forceinline__ void box_cut_runs(const int* pbox, int lane, RunBox* runs) {
  const int4 pb = *(const int4*)(pbox + lane * 4);
  const bool valid = pb.w >= 0;
  SegBox sb;
  sb.f0 = valid ? (unsigned)((pb.x & 255) | ((pb.y & 255) << 16)) : 0x7fff7fffu;
  sb.f1 = valid ? (unsigned)((pb.z & 255) | ((255 - (pb.x >> 8)) << 16)) : 0x7fff7fffu;
  sb.f2 = valid ? (unsigned)((255 - (pb.y >> 8)) | ((255 - (pb.z >> 8)) << 16)) : 0x7fff7fffu;
  sb.bmin = valid ? pb.w : INT_MAX;
  sb.nbmax = valid ? ~pb.w : INT_MAX;
  // a segment that fits contains only segments that fit: the largest fitting level is the same for all its lanes
  int level = 0;
  SegBox best = sb;
#define LIST_SEG_STAGE(S)                                              \
  seg_merge<S>(sb);                                                    \
  if (level == S && seg_fits(sb, MAXROWS, MAXKEYS)) { level = S + 1; best = sb; }
  LIST_SEG_STAGE(0) LIST_SEG_STAGE(1) LIST_SEG_STAGE(2) LIST_SEG_STAGE(3) LIST_SEG_STAGE(4) LIST_SEG_STAGE(5)
#undef LIST_SEG_STAGE
  if ((lane & ((1 << level) - 1)) == 0) {
    const bool any = best.bmin != INT_MAX;
    const int lox = best.f0 & 0xffff, loy = best.f0 >> 16, loz = best.f1 & 0xffff;
    const int hix = 255 - (int)(best.f1 >> 16), hiy = 255 - (int)(best.f2 & 0xffff), hiz = 255 - (int)(best.f2 >> 16);
    RunBox rb;
    rb.count = 1 << level;
    rb.b = any ? best.bmin : 0;
    rb.lo = any ? (lox | (loy << 8) | (loz << 16)) : 0;
    rb.n = any ? ((hix - lox + 1) | ((hiy - loy + 1) << 8) | ((hiz - loz + 1) << 16)) : 0;
    runs[lane] = rb;
  }
}

// ---- a run's box, decoded once per run (workgroup-uniform) ---------------------------------------------------------
// ceil(65536 / n): (v * box_inv(n)) >> 16 == v / n for the box rows and window keys of a run (v < 512, n < 256).
// MAY_BE_EMPTY: n = 0 (a run without a valid point) is divided by 1 instead
template <bool MAY_BE_EMPTY>
__device__ __forceinline__ int box_inv(int n) { return (65536 + n - 1) / (MAY_BE_EMPTY && n <= 0 ? 1 : n); }

struct RunDims {
  int lox, loy, loz, nx, ny, nz, rows, inv_nx, inv_ny;
  // MAY_BE_EMPTY = false: the caller has skipped the run with rows == 0
  template <bool MAY_BE_EMPTY>
  __device__ __forceinline__ void set_inverses() { inv_nx = box_inv<MAY_BE_EMPTY>(nx); inv_ny = box_inv<MAY_BE_EMPTY>(ny); }
  // box row v = (iz * ny + iy) * nx + ix -> its offsets in the box (after set_inverses)
  __device__ __forceinline__ void row_to_xyz(int v, int& ix, int& iy, int& iz) const {
    const int yz = (v * inv_nx) >> 16;
    ix = v - yz * nx;
    iz = (yz * inv_ny) >> 16;
    iy = yz - iz * ny;
  }
};
// lo, n: RunBox's (uniform)
__device__ __forceinline__ RunDims run_dims(int lo, int n) {
  RunDims d;
  d.lox = lo & 255; d.loy = (lo >> 8) & 255; d.loz = lo >> 16;
  d.nx = n & 255; d.ny = (n >> 8) & 255; d.nz = n >> 16;
  d.rows = d.nx * d.ny * d.nz;
  return d;
}

}  // namespace list
