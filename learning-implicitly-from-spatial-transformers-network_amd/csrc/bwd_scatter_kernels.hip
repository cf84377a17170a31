// Backward of the 3-D gathers: dX [rows][Kp] (gradient of the feature matrix, gather order) ->
//   * gradients of the channels-last voxel levels     (adjoint of F.grid_sample 3-D, modules.py:263-265)
// What vox_adjoint_plan.h plans (the 2-D adjoints: bwd_img_kernels.hip).
// HBM / atomic-rate bound: global float atomics run at ~1.3 TB/s chip-wide on MI355X whatever the kernel does,
// so the design goal is FEWER atomic bytes, shaped as runs along the channel axis.  Per voxel level one of
//   * global atomics, lanes over channels            (fine levels: 56 distinct taps per point, nothing to merge)
//   * voxel-side gather over cell-sorted samples      (dense middle level: written once, no atomics)
//   * LDS windows over runs of Morton-ordered points  (coarse levels: summed on chip without atomics -- every
//                                                     thread owns one channel column --, flushed once)
#include <limits.h>
#include <string.h>
#include <type_traits>

#include "list_common.h"
#include "point_math.h"

namespace list {

__device__ __forceinline__ void stencil_rt(const Pt& p, int j, float& x, float& y, float& z) {
  x = p.x + (j == 1 ? -kDisp : j == 2 ? kDisp : 0.f);
  y = p.y + (j == 3 ? -kDisp : j == 4 ? kDisp : 0.f);
  z = p.z + (j == 5 ? -kDisp : j == 6 ? kDisp : 0.f);
}

// ---- voxel levels ----------------------------------------------------------------------------------------
constexpr int kScatterRows = 64;           // points per workgroup (consecutive rows = one Morton neighbourhood)

// Straight to memory: C lanes per (point, stencil point) item, one 4*C-byte atomic run per tap.  This is
// what the levels whose stencil spreads over many voxels use (128^3 .. 32^3): their 56 taps per point are
// all distinct and neighbouring points share few of them, so the cost is the chip's atomic byte rate.
template <int C, int DXH, int T = 256>
__device__ __forceinline__ void scatter_direct(const ScatterParams& sp, const ListVoxLevel& gv, int col_off,
                                               const Pt* __restrict__ pts, int r_begin, int r_end,
                                               int64_t row0, float inv_s) {
  constexpr int per_pass = T / C;
  const int tid = threadIdx.x;
  const int c = tid % C;
  float* __restrict__ gout = (float*)gv.data;
  for (int it = r_begin * LIST_N_STENCIL + tid / C; it < r_end * LIST_N_STENCIL; it += per_pass) {
    const int r = it / LIST_N_STENCIL, j = it - r * LIST_N_STENCIL;
    const Pt p = pts[r];
    if (!p.valid) continue;
    float x, y, z;
    stencil_rt(p, j, x, y, z);
    const Taps t = make_taps(x, y, z, C, gv.D, gv.H, gv.W);
    const float gval = dx_at<DXH>(sp.dx, (row0 + r) * sp.g.Kp + col_off + j * C + c) * inv_s;
    float* base = gout + (int64_t)p.b * gv.image_stride + c;
#pragma unroll
    for (int k = 0; k < 8; ++k) atomicAdd(base + t.o[k], t.w[k] * gval);
  }
}

// Persistent grid (workgroups walk the 64-row blocks; its size: direct_grid_cap, vox_adjoint_plan.h)
template <int C, int DXH>
__global__ __launch_bounds__(256) void k_scatter_vox(ScatterParams sp, ListVoxLevel gv, int col_off, int nblocks) {
  __shared__ Pt pts[kScatterRows];
  const float inv_s = sp.scale[1];
  for (int blk = blockIdx.x; blk < nblocks; blk += gridDim.x) {
    __syncthreads();
    if (threadIdx.x < kScatterRows) pts[threadIdx.x] = load_point(sp.g, blk * kScatterRows + threadIdx.x);
    __syncthreads();
    scatter_direct<C, DXH>(sp, gv, col_off, pts, 0, kScatterRows, (int64_t)blk * kScatterRows, inv_s);
  }
}

// fp16 operands, levels whose tap run is two or more 64-B atomic requests in fp32 (C >= 32): the direct form's
// time follows the atomic BYTES there (same 9 M tap runs per launch: C = 16 / 64 B 0.51 ms, C = 32 / 128 B 0.89 ms),
// so the runs are added as packed halfs (global_atomic_pk_add_f16, lanes over channel PAIRS) into a zeroed fp16 image
// of the level kept at the gradient scale s (the dX operand is s * dX already, fp16), and one streaming pass
// writes (1/s) * image as the fp32 gradient (which then needs no memset).  A voxel of these sparse levels sums a few
// contributions, each rounded to 11 bits -- far inside the fp16 mode's gradient noise; the fp32-grade
// mode never takes this form.
typedef _Float16 half2v __attribute__((ext_vector_type(2)));

// lanes over channel pairs; WIN: a run of k_scatter_vox_win whose box does not fit the window (T threads, the taps at
// the window levels' scale), else k_scatter_vox_h2's block (every thread has an item, the taps at the gradient scale)
template <int C, int T, bool WIN>
__device__ __forceinline__ void scatter_direct_h2(const ScatterParams& sp, const ListVoxLevel& gv, int col_off,
                                                  const Pt* __restrict__ pts, int r_begin, int r_end, int64_t row0,
                                                  _Float16* __restrict__ img16) {
  constexpr int CP = C / 2, per_pass = (T / CP) > 0 ? (T / CP) : 1;
  const int tid = threadIdx.x;
  if (WIN && tid >= per_pass * CP) return;
  const int cp = tid % CP;
  for (int it = r_begin * LIST_N_STENCIL + tid / CP; it < r_end * LIST_N_STENCIL; it += per_pass) {
    const int r = it / LIST_N_STENCIL, j = it - r * LIST_N_STENCIL;
    const Pt p = pts[r];
    if (!p.valid) continue;
    float x, y, z;
    stencil_rt(p, j, x, y, z);
    const Taps t = make_taps(x, y, z, C, gv.D, gv.H, gv.W);
    const unsigned g2 = *(const unsigned*)((const unsigned short*)sp.dx + (row0 + r) * sp.g.Kp + col_off + j * C + 2 * cp);
    float g0 = h2f((unsigned short)(g2 & 0xffffu)), g1 = h2f((unsigned short)(g2 >> 16));
    if (WIN) { g0 *= kWinPkScale; g1 *= kWinPkScale; }
    _Float16* base = img16 + (int64_t)p.b * gv.image_stride + 2 * cp;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      half2v v;
      v.x = (_Float16)(t.w[k] * g0); v.y = (_Float16)(t.w[k] * g1);
      __builtin_amdgcn_global_atomic_fadd_v2f16((__attribute__((address_space(1))) half2v*)(base + t.o[k]), v);
    }
  }
}

template <int C>
__global__ __launch_bounds__(256) void k_scatter_vox_h2(ScatterParams sp, ListVoxLevel gv, int col_off, int nblocks,
                                                        _Float16* __restrict__ img16) {
  __shared__ Pt pts[kScatterRows];
  for (int blk = blockIdx.x; blk < nblocks; blk += gridDim.x) {
    __syncthreads();
    if (threadIdx.x < kScatterRows) pts[threadIdx.x] = load_point(sp.g, blk * kScatterRows + threadIdx.x);
    __syncthreads();
    scatter_direct_h2<C, 256, false>(sp, gv, col_off, pts, 0, kScatterRows, (int64_t)blk * kScatterRows, img16);
  }
}

__global__ __launch_bounds__(256) void k_h16_to_grad(const _Float16* __restrict__ img16, float* __restrict__ out,
                                                     int64_t n8, const float* __restrict__ scale, float unscale) {
  const float inv_s = scale[1] * unscale;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n8; i += (int64_t)gridDim.x * 256) {
    typedef __attribute__((ext_vector_type(4))) unsigned u4;
    const u4 r = __builtin_nontemporal_load((const u4*)img16 + i);
    const unsigned w[4] = {r.x, r.y, r.z, r.w};
    float o[8];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      o[2 * e] = h2f((unsigned short)(w[e] & 0xffffu)) * inv_s;
      o[2 * e + 1] = h2f((unsigned short)(w[e] >> 16)) * inv_s;
    }
    typedef __attribute__((ext_vector_type(4))) float f4;
    __builtin_nontemporal_store((f4){o[0], o[1], o[2], o[3]}, (f4*)out + 2 * i);
    __builtin_nontemporal_store((f4){o[4], o[5], o[6], o[7]}, (f4*)out + 2 * i + 1);
  }
}

// Coarse levels (stencil shorter than a voxel: 16^3 and 8^3, 58 % of all tap contributions): a run of
// Morton-consecutive points touches a small box of voxels, so its contributions are summed in an LDS
// window first and the window is flushed once (8-50x fewer global atomics).  LDS float atomics are slow on
// CDNA (measured ~2.6 clk per LANE), so the window is accumulated WITHOUT atomics: thread (copy k,
// channel c) owns column c of copy k of the window and is the only one that ever touches it -- plain
// ds_read / add / ds_write, the 8 taps of a sample per batch.  A tap that the border clamp folds onto
// its neighbour (weight exactly 0) is redirected to a dummy cell so the 8 addresses of a batch never alias.
// The workgroup's 64 points are cut into runs adaptively: 8-point boxes are merged greedily while the
// merged box fits the window (8^3 level: ~32 points per run, 16^3: ~16); a box that does not fit on its
// own goes straight to memory.
constexpr int kSubPts = 8;                 // granularity of the run planner = points per record chunk
constexpr int kNSub = kScatterRows / kSubPts;
struct Run { int first, count, direct; int ox, oy, oz, nx, ny, nz, b; };

// All 7 stencil samples of a point lie within the 4 x 4 x 4 voxels around the centre's cell when the
// stencil is shorter than a voxel, and they touch only 32 of them (the "plus" the forward's
// k_gather_vox_near reads): 4 x-slots x the centre's 2x2 in (y,z), plus 2 extra y-slots and 2 extra
// z-slots over the centre's 2x2 of the other axes.  The adjoint per point is therefore ONE batch of 32
// read-add-writes with the per-axis 4-slot weight vectors of the centre / minus / plus samples:
//   X[k] = g0 wcx[k] + g1 wmx[k] + g2 wpx[k],  Y[k] = g3 wmy[k] + g4 wpy[k],  Z[k] = g5 wmz[k] + g6 wpz[k]
//   dV[kx][ky][kz] = X[kx] wcy[ky] wcz[kz] + wcx[kx] Y[ky] wcz[kz] + wcx[kx] wcy[ky] Z[kz]
struct NearRec { int o[32]; float wx[3][4], wy[3][4], wz[3][4]; int cell; int pad_[3]; };

__device__ __forceinline__ void slot_weights(const Axis& a, int cbase, float (&w)[4], bool (&used)[4]) {
  const int k0 = a.i0 - cbase;            // 0, 1 or 2
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const bool lo = k == k0, hi = (k == k0 + 1) && a.has1;
    w[k] = lo ? a.w0 : (hi ? a.w1 : 0.f);
    used[k] = used[k] || lo || hi;
  }
}

// The 32 window offsets are a function of the point's BASE CELL and the run's box alone: a slot inside the box gets its
// voxel, whether this point's samples use it or not (an unused slot receives G = 0 exactly), a slot outside the box
// (no point of the run uses it: the box covers every used tap) goes to the dummy cell.  Consecutive points of one base
// cell -- ~4 at 16^3, tens at 8^3 in Morton order -- therefore share their offsets, and the kernel sums their 32
// contributions in registers and touches the window once per cell group (round 3: the per-point read-add-write chain
// was 41 - 47 % of the kernel, profiles/r03_window_adjoint_ablation.txt).
// Built by 16 threads per point (sub = 0..15): every thread derives the nine per-axis records itself (they are cheap)
// and writes two offsets and, for sub < 9, one weight row.
__device__ __forceinline__ void build_near(const Pt& p, int W, int H, int D, const Run& r, int C, NearRec& n, int sub) {
  const float pc[3] = {p.x, p.y, p.z};
  const int S[3] = {W, H, D};
  int base[3];
#pragma unroll
  for (int ax = 0; ax < 3; ++ax) {
    const Axis c = axis_setup(pc[ax], S[ax]), m = axis_setup(pc[ax] - kDisp, S[ax]), q = axis_setup(pc[ax] + kDisp, S[ax]);
    base[ax] = c.i0 - 1;
    bool used[4] = {false, false, false, false};
    float w[3][4];
    slot_weights(c, base[ax], w[0], used);
    slot_weights(m, base[ax], w[1], used);
    slot_weights(q, base[ax], w[2], used);
    float(*dst)[4] = ax == 0 ? n.wx : (ax == 1 ? n.wy : n.wz);
#pragma unroll
    for (int v = 0; v < 3; ++v)
      if (sub == ax * 3 + v) {
#pragma unroll
        for (int k = 0; k < 4; ++k) dst[v][k] = p.valid ? w[v][k] : 0.f;
      }
  }
  const int vol = r.nx * r.ny * r.nz;
  auto cell = [&](int kx, int ky, int kz) -> int {
    const int ix = base[0] + kx - r.ox, iy = base[1] + ky - r.oy, iz = base[2] + kz - r.oz;
    if (!p.valid || ix < 0 || ix >= r.nx || iy < 0 || iy >= r.ny || iz < 0 || iz >= r.nz) return vol * C;   // dummy cell
    return ((iz * r.ny + iy) * r.nx + ix) * C;
  };
#pragma unroll
  for (int e = 0; e < 2; ++e) {
    const int s = 2 * sub + e;                       // window slot 0..31 (order of the forward's shared-tap kernel)
    int kx, ky, kz;
    if (s < 16) { kx = s >> 2; ky = 1 + (s & 1); kz = 1 + ((s >> 1) & 1); }
    else if (s < 24) { kx = 1 + (s & 1); ky = (s & 4) ? 3 : 0; kz = 1 + ((s >> 1) & 1); }
    else { kx = 1 + (s & 1); ky = 1 + ((s >> 1) & 1); kz = (s & 4) ? 3 : 0; }
    n.o[s] = cell(kx, ky, kz);
  }
  if (sub == 15) n.cell = p.valid ? (base[0] + 1) | ((base[1] + 1) << 10) | ((base[2] + 1) << 20) : -1;
}

// kWinFloats (kWinFloatsSmall or kWinFloatsLarge) and kWinPkScale, the fp16 image's scale: vox_adjoint_plan.h
// img16 != nullptr (fp16 operands): the window is flushed as packed halfs into a zeroed fp16 image of the level
// (scale above) and k_h16_to_grad writes the fp32 gradient afterwards -- half the atomic bytes of the flush that
// bounds these levels.
template <int C, int DXH, int kWinFloats>
__global__ __launch_bounds__((C >= 128 ? C : 128)) void k_scatter_vox_win(ScatterParams sp, ListVoxLevel gv,
                                                                             int col_off, _Float16* __restrict__ img16) {
  constexpr int T = C >= 128 ? C : 128;
  constexpr int COPIES = T / C;
  constexpr int MYP = kSubPts / COPIES;              // points per copy per chunk
  constexpr int kCap = kWinFloats / T - 1;           // window voxels (one more cell is the dummy)
  static_assert(C >= 16 && T % C == 0 && kSubPts % COPIES == 0 && T >= kScatterRows, "geometry");
  __shared__ Pt pts[kScatterRows];
  __shared__ int box[kNSub][8];                      // lo x,y,z | hi x,y,z | min image | max image
  __shared__ Run runs[kNSub];
  __shared__ int n_runs;
  __shared__ NearRec nrec[kSubPts];
  __shared__ int grp_off[T / 64][32];
  __shared__ float win[kWinFloats];
  const int tid = threadIdx.x;
  const int c = tid % C, k = tid / C;
  const int blk = xcd_contiguous_block(blockIdx.x, gridDim.x);
  const int W = gv.W, H = gv.H, D = gv.D;
  const int64_t row0 = (int64_t)blk * kScatterRows;
  const float inv_s = sp.scale[1];
  if (tid < kNSub * 8) box[tid >> 3][tid & 7] = ((tid & 7) < 3 || (tid & 7) == 6) ? INT_MAX : INT_MIN;
  if (tid < kScatterRows) pts[tid] = load_point(sp.g, blk * kScatterRows + tid);
  __syncthreads();
  if (tid < kScatterRows && pts[tid].valid) {
    const Pt p = pts[tid];
    int* bx = box[tid / kSubPts];
    const Axis lx = axis_setup(p.x - kDisp, W), hx = axis_setup(p.x + kDisp, W);
    const Axis ly = axis_setup(p.y - kDisp, H), hy = axis_setup(p.y + kDisp, H);
    const Axis lz = axis_setup(p.z - kDisp, D), hz = axis_setup(p.z + kDisp, D);
    atomicMin(&bx[0], lx.i0); atomicMin(&bx[1], ly.i0); atomicMin(&bx[2], lz.i0);
    atomicMax(&bx[3], hx.i0 + hx.has1); atomicMax(&bx[4], hy.i0 + hy.has1); atomicMax(&bx[5], hz.i0 + hz.has1);
    atomicMin(&bx[6], p.b); atomicMax(&bx[7], p.b);
  }
  __syncthreads();
  if (tid == 0) {                                    // plan the runs
    int n = 0, i = 0;
    while (i < kNSub) {
      if (box[i][7] < box[i][6]) { ++i; continue; }  // no valid point
      int lo[3] = {box[i][0], box[i][1], box[i][2]}, hi[3] = {box[i][3], box[i][4], box[i][5]};
      const int b = box[i][6];
      Run r;
      r.first = i * kSubPts; r.count = kSubPts; r.b = b;
      const int64_t v0 = (int64_t)(hi[0] - lo[0] + 1) * (hi[1] - lo[1] + 1) * (hi[2] - lo[2] + 1);
      r.direct = (box[i][6] != box[i][7] || v0 > kCap) ? 1 : 0;
      int jn = i + 1;
      while (!r.direct && jn < kNSub && box[jn][7] >= box[jn][6] && box[jn][6] == b && box[jn][7] == b) {
        int l2[3], h2[3];
        for (int a = 0; a < 3; ++a) { l2[a] = min(lo[a], box[jn][a]); h2[a] = max(hi[a], box[jn][3 + a]); }
        const int64_t v = (int64_t)(h2[0] - l2[0] + 1) * (h2[1] - l2[1] + 1) * (h2[2] - l2[2] + 1);
        if (v > kCap) break;
        for (int a = 0; a < 3; ++a) { lo[a] = l2[a]; hi[a] = h2[a]; }
        r.count += kSubPts; ++jn;
      }
      r.ox = lo[0]; r.oy = lo[1]; r.oz = lo[2];
      r.nx = hi[0] - lo[0] + 1; r.ny = hi[1] - lo[1] + 1; r.nz = hi[2] - lo[2] + 1;
      runs[n++] = r;
      i = jn;
    }
    n_runs = n;
  }
  __syncthreads();
  float* __restrict__ gout = (float*)gv.data;
  const int nr = n_runs;
#pragma unroll 1
  for (int ri = 0; ri < nr; ++ri) {
    Run r = runs[ri];
    // (uniform: the window offsets of a cell group are then scalar arithmetic, not 32 more registers)
    r.first = __builtin_amdgcn_readfirstlane(r.first); r.count = __builtin_amdgcn_readfirstlane(r.count);
    r.direct = __builtin_amdgcn_readfirstlane(r.direct); r.b = __builtin_amdgcn_readfirstlane(r.b);
    r.ox = __builtin_amdgcn_readfirstlane(r.ox); r.oy = __builtin_amdgcn_readfirstlane(r.oy); r.oz = __builtin_amdgcn_readfirstlane(r.oz);
    r.nx = __builtin_amdgcn_readfirstlane(r.nx); r.ny = __builtin_amdgcn_readfirstlane(r.ny); r.nz = __builtin_amdgcn_readfirstlane(r.nz);
    if (r.direct) {
      if (DXH && img16) scatter_direct_h2<C, T, true>(sp, gv, col_off, pts, r.first, r.first + r.count, row0, img16);
      else scatter_direct<C, DXH, T>(sp, gv, col_off, pts, r.first, r.first + r.count, row0, inv_s);
      continue;
    }
    const int nx = r.nx, ny = r.ny, vol = r.nx * r.ny * r.nz;
    float* mine = win + (k * (vol + 1)) * C + c;     // my column of my copy
    for (int v = 0; v <= vol; ++v) mine[v * C] = 0.f;
    // contributions of the current base-cell group: summed in registers, added to the window once per group
    int cur_cell = -2;
    float Gacc[32];
    // the group's 32 window offsets: copied from its first point's record into a per-wave LDS row when the group
    // opens (the record itself is overwritten by the next chunk; DS operations of one wave execute in order)
    int* gro = grp_off[tid >> 6];
    auto add_group = [&]() {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");      // (pairs with the release behind the gro[] stores)
#pragma unroll
      for (int h = 0; h < 2; ++h) {                  // two batches of 16 (addresses are distinct within the 32, or the dummy)
        float v[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) v[q] = mine[gro[16 * h + q]];
#pragma unroll
        for (int q = 0; q < 16; ++q) mine[gro[16 * h + q]] = v[q] + Gacc[16 * h + q];
      }
    };
#pragma unroll 1
    for (int ch = 0; ch < r.count; ch += kSubPts) {
      __syncthreads();                               // previous chunk's records are consumed
      if (tid < kSubPts * 16) build_near(pts[r.first + ch + (tid >> 4)], W, H, D, r, C, nrec[tid >> 4], tid & 15);
      // my points of the chunk: every dX value is requested before the first use
      float gval[MYP][LIST_N_STENCIL];
#pragma unroll
      for (int m = 0; m < MYP; ++m) {
        const int64_t o = (row0 + r.first + ch + k + COPIES * m) * sp.g.Kp + col_off + c;
#pragma unroll
        for (int j = 0; j < LIST_N_STENCIL; ++j) gval[m][j] = dx_at<DXH>(sp.dx, o + j * C);
      }
      __syncthreads();
#pragma unroll
      for (int m = 0; m < MYP; ++m) {                // (unrolled: gval[m] must stay in registers)
        const NearRec& n = nrec[k + COPIES * m];
        const float* g = gval[m];
        float X[4], Y[4], Z[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          X[q] = fmaf(g[2], n.wx[2][q], fmaf(g[1], n.wx[1][q], g[0] * n.wx[0][q]));
          Y[q] = fmaf(g[4], n.wy[2][q], g[3] * n.wy[1][q]);
          Z[q] = fmaf(g[6], n.wz[2][q], g[5] * n.wz[1][q]);
        }
        const int cell = __builtin_amdgcn_readfirstlane(n.cell);          // (the same point for the whole wave)
        if (cell != cur_cell) {
          if (cur_cell != -2) add_group();
          cur_cell = cell;
          if ((tid & 63) < 32) gro[tid & 31] = n.o[tid & 31];
          // lanes 32..63 read offsets that lanes 0..31 stored: a wavefront-scope release here (and the acquire in
          // add_group) keeps the compiler from reusing gro[] loads across the store (the hardware executes the DS
          // operations of one wave in order; the fences cost no instruction beyond an lgkmcnt wait)
          __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
#pragma unroll
          for (int q = 0; q < 32; ++q) Gacc[q] = 0.f;
        }
#pragma unroll
        for (int kx = 0; kx < 4; ++kx)
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const int ky = 1 + (q & 1), kz = 1 + (q >> 1);
            Gacc[kx * 4 + q] += fmaf(X[kx], n.wy[0][ky] * n.wz[0][kz],
                                     n.wx[0][kx] * fmaf(Y[ky], n.wz[0][kz], n.wy[0][ky] * Z[kz]));
          }
#pragma unroll
        for (int e = 0; e < 2; ++e)
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const int ka = 1 + (q & 1), kb = 1 + (q >> 1), ke = e ? 3 : 0;
            Gacc[16 + e * 4 + q] += n.wx[0][ka] * Y[ke] * n.wz[0][kb];
            Gacc[24 + e * 4 + q] += n.wx[0][ka] * n.wy[0][kb] * Z[ke];
          }
      }
    }
    if (cur_cell != -2) add_group();
    __syncthreads();
    if (DXH && img16) {
      _Float16* base16 = img16 + (int64_t)r.b * gv.image_stride;
      for (int i = tid; i < vol * (C / 2); i += T) {
        const int vox = i / (C / 2), cc = 2 * (i - vox * (C / 2));
        float s0 = 0.f, s1 = 0.f;
#pragma unroll
        for (int kk = 0; kk < COPIES; ++kk) {
          const float2 w2 = *(const float2*)(win + (kk * (vol + 1) + vox) * C + cc);
          s0 += w2.x; s1 += w2.y;
        }
        if (s0 == 0.f && s1 == 0.f) continue;
        const int vx = vox % nx, vy = (vox / nx) % ny, vz = vox / (nx * ny);
        half2v v;
        v.x = (_Float16)(s0 * kWinPkScale); v.y = (_Float16)(s1 * kWinPkScale);
        __builtin_amdgcn_global_atomic_fadd_v2f16(
            (__attribute__((address_space(1))) half2v*)(base16 + ((int64_t)((r.oz + vz) * H + (r.oy + vy)) * W + (r.ox + vx)) * C + cc), v);
      }
    } else {
      float* base = gout + (int64_t)r.b * gv.image_stride;
      for (int i = tid; i < vol * C; i += T) {
        const int vox = i / C, cc = i - vox * C;
        float sum = 0.f;
#pragma unroll
        for (int kk = 0; kk < COPIES; ++kk) sum += win[(kk * (vol + 1) + vox) * C + cc];
        if (sum == 0.f) continue;
        const int vx = vox % nx, vy = (vox / nx) % ny, vz = vox / (nx * ny);
        atomicAdd(base + ((int64_t)((r.oz + vz) * H + (r.oy + vy)) * W + (r.ox + vx)) * C + cc, sum * inv_s);
      }
    }
    __syncthreads();                                 // the next run re-zeroes the window
  }
}

// ---- middle levels: every voxel gathers --------------------------------------------------------------------
// Where the samples are dense (32^3: ~37 contributions per voxel) the adjoint is cheaper as a GATHER:
// the (point, stencil) samples are counting-sorted by their base cell, and each voxel sums the samples
// of the <= 8 cells it is a corner of and is written ONCE with a plain store -- no atomics, no memset.
// (The direct scatter of that level moves 2.3 GB through the atomic units, 1.8 ms at the chip's rate.)
struct VoxSample { int off; float fx, fy, fz; };   // dX element offset of the sample's channel 0; w1 per axis
constexpr int kScanPerBlock = 4096;

__global__ __launch_bounds__(256) void k_vs_hist(ScatterParams sp, ListVoxLevel gv, int* __restrict__ keys,
                                                 int* __restrict__ bins) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  const int row = t >> 3, j = t & 7;
  if (row >= sp.g.rows) return;
  int cell = -1;
  if (row < sp.g.n_valid && j < LIST_N_STENCIL) {
    const Pt p = load_point(sp.g, row);
    float x, y, z;
    stencil_rt(p, j, x, y, z);
    const Axis ax = axis_setup(x, gv.W), ay = axis_setup(y, gv.H), az = axis_setup(z, gv.D);
    cell = ((p.b * gv.D + az.i0) * gv.H + ay.i0) * gv.W + ax.i0;
    atomicAdd(&bins[cell], 1);
  }
  keys[t] = cell;
}

// in-place exclusive scan of n ints: per-block scan + block totals, scan of the totals, add back.  256-thread
// workgroups (16 consecutive ints per thread, wave scans by shuffles, one barrier): beside the backward's other streams
// a 1024-thread workgroup waits for a CU with four free wave slots per SIMD (the three launches took 0.6 ms there for
// 1 MB of counters; 0.03 ms alone).
constexpr int kScanThreads = 256, kScanPerThread = kScanPerBlock / kScanThreads;

// exclusive prefix of `sum` over the workgroup's threads; the workgroup total in `total`
__device__ __forceinline__ int block_exclusive(int sum, int* wave_tot, int& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int inc = sum;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int u = __shfl_up(inc, off);
    if (lane >= off) inc += u;
  }
  if (lane == 63) wave_tot[wave] = inc;
  __syncthreads();
  int before = 0;
  total = 0;
#pragma unroll
  for (int w = 0; w < kScanThreads / 64; ++w) {
    const int t = wave_tot[w];
    if (w < wave) before += t;
    total += t;
  }
  return before + inc - sum;
}

__global__ __launch_bounds__(kScanThreads) void k_scan_block(int* __restrict__ a, int n, int* __restrict__ sums) {
  __shared__ int wave_tot[kScanThreads / 64];
  const int i0 = blockIdx.x * kScanPerBlock + threadIdx.x * kScanPerThread;
  int v[kScanPerThread], sum = 0;
#pragma unroll
  for (int e = 0; e < kScanPerThread; ++e) { v[e] = (i0 + e < n) ? a[i0 + e] : 0; sum += v[e]; }
  int total;
  int run = block_exclusive(sum, wave_tot, total);
#pragma unroll
  for (int e = 0; e < kScanPerThread; ++e) { if (i0 + e < n) a[i0 + e] = run; run += v[e]; }
  if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// nb <= 1024 block totals (kVoxGatherMaxBins / kScanPerBlock), one workgroup, 4 per thread
__global__ __launch_bounds__(kScanThreads) void k_scan_sums(int* __restrict__ sums, int nb) {
  __shared__ int wave_tot[kScanThreads / 64];
  const int i0 = threadIdx.x * 4;
  int v[4], sum = 0;
#pragma unroll
  for (int e = 0; e < 4; ++e) { v[e] = (i0 + e < nb) ? sums[i0 + e] : 0; sum += v[e]; }
  int total;
  int run = block_exclusive(sum, wave_tot, total);
#pragma unroll
  for (int e = 0; e < 4; ++e) { if (i0 + e < nb) sums[i0 + e] = run; run += v[e]; }
}

__global__ __launch_bounds__(kScanThreads) void k_scan_add(int* __restrict__ a, int n, const int* __restrict__ sums) {
  const int i0 = blockIdx.x * kScanPerBlock + threadIdx.x * kScanPerThread;
  const int add = sums[blockIdx.x];
#pragma unroll
  for (int e = 0; e < kScanPerThread; ++e)
    if (i0 + e < n) a[i0 + e] += add;
}

// bins: exclusive starts on entry, END offsets on exit
template <int C>
__global__ __launch_bounds__(256) void k_vs_scatter(ScatterParams sp, ListVoxLevel gv, const int* __restrict__ keys,
                                                    int* __restrict__ bins, VoxSample* __restrict__ recs,
                                                    int col_off) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  const int row = t >> 3, j = t & 7;
  if (row >= sp.g.rows) return;
  const int cell = keys[t];
  if (cell < 0) return;
  const Pt p = load_point(sp.g, row);
  float x, y, z;
  stencil_rt(p, j, x, y, z);
  const Axis ax = axis_setup(x, gv.W), ay = axis_setup(y, gv.H), az = axis_setup(z, gv.D);
  VoxSample r;
  r.off = row * sp.g.Kp + col_off + j * C;
  r.fx = ax.w1; r.fy = ay.w1; r.fz = az.w1;
  recs[atomicAdd(&bins[cell], 1)] = r;
}

// the record ranges of the four (y, z) lines a voxel is a corner of (12 independent loads, ahead of the samples): line q
// is (y - (q & 1), z - (q >> 1)); records [lo, mid) lie in cell x-1, [mid, hi) in cell x
struct VoxLines { int lo[4], mid[4], hi[4]; };
__device__ __forceinline__ VoxLines vox_lines(const ListVoxLevel& gv, int64_t vox, const int* __restrict__ ends) {
  const int W = gv.W, H = gv.H, D = gv.D;
  const int x = (int)(vox % W), y = (int)((vox / W) % H), z = (int)((vox / ((int64_t)W * H)) % D);
  const int b = (int)(vox / ((int64_t)W * H * D));
  VoxLines r;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int yy = y - (q & 1), zz = z - (q >> 1);
    r.lo[q] = r.mid[q] = r.hi[q] = 0;
    if (yy < 0 || zz < 0) continue;
    // cells x-1 and x of this (y, z) line are adjacent bins: one contiguous run of records
    const int bin1 = ((b * D + zz) * H + yy) * W + x;          // cell x (corner dx = 0)
    r.mid[q] = bin1 > 0 ? ends[bin1 - 1] : 0;                  // = end of cell x-1
    r.lo[q] = x > 0 ? (bin1 > 1 ? ends[bin1 - 2] : 0) : r.mid[q];
    r.hi[q] = ends[bin1];
  }
  return r;
}
// weight of record s of line q at the voxel (0 past the line's end)
__device__ __forceinline__ float vox_sample_weight(const VoxSample& r, int s, int s_mid, int s_hi, int q) {
  const int dy = q & 1, dz = q >> 1;
  const bool dx = s < s_mid;                                   // the sample lies in cell x-1: corner +1 in x
  const float w = (dx ? r.fx : 1.f - r.fx) * (dy ? r.fy : 1.f - r.fy) * (dz ? r.fz : 1.f - r.fz);
  return s >= s_hi ? 0.f : w;
}

// lanes over channels, 256 / C voxels per workgroup; 8 samples in flight per lane
template <int C, int DXH>
__global__ __launch_bounds__(256) void k_vs_gather(ScatterParams sp, ListVoxLevel gv, const int* __restrict__ ends,
                                                   const VoxSample* __restrict__ recs, int64_t n_vox) {
  constexpr int VPB = 256 / C, NB = 8;
  const int64_t vox = (int64_t)blockIdx.x * VPB + threadIdx.x / C;
  const int c = threadIdx.x % C;
  if (vox >= n_vox) return;
  float acc = 0.f;
  const VoxLines ln = vox_lines(gv, vox, ends);
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int s_mid = ln.mid[q], s_hi = ln.hi[q];
    for (int s = ln.lo[q]; s < s_hi; s += NB) {
      VoxSample r[NB];
#pragma unroll
      for (int u = 0; u < NB; ++u) r[u] = recs[min(s + u, s_hi - 1)];
      float g[NB];
#pragma unroll
      for (int u = 0; u < NB; ++u) g[u] = dx_at<DXH>(sp.dx, (int64_t)r[u].off + c);
#pragma unroll
      for (int u = 0; u < NB; ++u) acc = fmaf(vox_sample_weight(r[u], s + u, s_mid, s_hi, q), g[u], acc);
    }
  }
  ((float*)gv.data)[vox * C + c] = acc * sp.scale[1];
}

// The same sums with a lane per (voxel, 8 channels) instead of per (voxel, channel): a sample costs the wave one 16-B
// record load and one 16-B (fp16 dX) load per EIGHT voxel-samples instead of one of each per voxel-sample -- the kernel
// above is bound by the number of vector-memory instructions (a 2-B load per lane is a whole instruction), not by bytes.
// Every channel still adds its samples in the same order with the same weights: bit-identical results.
// Lanes of a wave belong to 64 / (C / 8) voxels with different sample counts: they idle in the longer lists' tails.
template <int C, int DXH>
__global__ __launch_bounds__(256) void k_vs_gather8(ScatterParams sp, ListVoxLevel gv, const int* __restrict__ ends,
                                                    const VoxSample* __restrict__ recs, int64_t n_vox) {
  constexpr int TPV = C / 8, VPB = 256 / TPV, NB = 4;
  const int64_t vox = (int64_t)blockIdx.x * VPB + threadIdx.x / TPV;
  const int c8 = (threadIdx.x % TPV) * 8;
  if (vox >= n_vox) return;
  float acc[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) acc[e] = 0.f;
  const VoxLines ln = vox_lines(gv, vox, ends);
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int s_mid = ln.mid[q], s_hi = ln.hi[q];
    for (int s = ln.lo[q]; s < s_hi; s += NB) {
      VoxSample r[NB];
#pragma unroll
      for (int u = 0; u < NB; ++u) r[u] = recs[min(s + u, s_hi - 1)];
      float g[NB][8];
#pragma unroll
      for (int u = 0; u < NB; ++u) load8<DXH>(sp.dx, (int64_t)r[u].off + c8, g[u]);
#pragma unroll
      for (int u = 0; u < NB; ++u) {
        const float w = vox_sample_weight(r[u], s + u, s_mid, s_hi, q);
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] = fmaf(w, g[u][e], acc[e]);
      }
    }
  }
  const float inv_s = sp.scale[1];
  float* out = (float*)gv.data + vox * C + c8;
  *(float4*)out = make_float4(acc[0] * inv_s, acc[1] * inv_s, acc[2] * inv_s, acc[3] * inv_s);
  *(float4*)(out + 4) = make_float4(acc[4] * inv_s, acc[5] * inv_s, acc[6] * inv_s, acc[7] * inv_s);
}

template <int C>
static hipError_t gather_level(const ScatterParams& sp, const ListVoxLevel& gv, int col_off, int B, bool lanes8,
                               const VoxGatherBuffers& vb, hipStream_t s) {
  const int64_t n_vox = (int64_t)B * gv.D * gv.H * gv.W;
  const int nb = (int)((n_vox + kScanPerBlock - 1) / kScanPerBlock);
  hipError_t e = hipMemsetAsync(vb.bins, 0, (size_t)n_vox * sizeof(int), s);
  if (e != hipSuccess) return e;
  const dim3 gs((unsigned)((sp.g.rows * 8 + 255) / 256));
  hipLaunchKernelGGL(k_vs_hist, gs, dim3(256), 0, s, sp, gv, vb.keys, vb.bins);
  hipLaunchKernelGGL(k_scan_block, dim3((unsigned)nb), dim3(kScanThreads), 0, s, vb.bins, (int)n_vox, vb.sums);
  hipLaunchKernelGGL(k_scan_sums, dim3(1), dim3(kScanThreads), 0, s, vb.sums, nb);
  hipLaunchKernelGGL(k_scan_add, dim3((unsigned)nb), dim3(kScanThreads), 0, s, vb.bins, (int)n_vox, vb.sums);
  hipLaunchKernelGGL(k_vs_scatter<C>, gs, dim3(256), 0, s, sp, gv, vb.keys, vb.bins, (VoxSample*)vb.recs, col_off);
  const int vpb = lanes8 ? 256 / (C / 8) : 256 / C;             // voxels per workgroup
  const dim3 gg((unsigned)((n_vox + vpb - 1) / vpb));
  auto kernel = lanes8 ? (sp.dx_f16 ? k_vs_gather8<C, 1> : k_vs_gather8<C, 0>) : (sp.dx_f16 ? k_vs_gather<C, 1> : k_vs_gather<C, 0>);
  hipLaunchKernelGGL(kernel, gg, dim3(256), 0, s, sp, gv, vb.bins, (const VoxSample*)vb.recs, n_vox);
  return hipGetLastError();
}

// scalar (C == 1) levels: one lane per (point, stencil point, tap) -- a wave is one point, its 56 taps leave in ONE
// atomic instruction in which the two lanes of an x pair are neighbours (adjacent floats: one 64-B atomic request
// for both), instead of 8 instructions of 56 unrelated addresses each (one lane per sample, a tap per instruction)
template <int DXH>
__global__ __launch_bounds__(256) void k_scatter_vox1(ScatterParams sp, ListVoxLevel gv, int col_off) {
  const int64_t total = (int64_t)sp.g.n_valid * 64;
  for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (int64_t)gridDim.x * 256) {
    const int row = (int)(t >> 6), j = (int)(t >> 3) & 7, k = (int)t & 7;
    if (j >= LIST_N_STENCIL) continue;
    const Pt p = load_point(sp.g, row);
    float x, y, z;
    stencil_rt(p, j, x, y, z);
    const Taps tp = make_taps(x, y, z, 1, gv.D, gv.H, gv.W);
    int o = tp.o[0];
    float w = tp.w[0];
#pragma unroll
    for (int q = 1; q < 8; ++q)
      if (k == q) { o = tp.o[q]; w = tp.w[q]; }
    const float gval = dx_at<DXH>(sp.dx, (int64_t)row * sp.g.Kp + col_off + j) * sp.scale[1];
    atomicAdd((float*)gv.data + (int64_t)p.b * gv.image_stride + o, w * gval);
  }
}

template <int C, int kWinFloats>
static void launch_scatter_vox_win(const ScatterParams& sp, const ListVoxLevel& gv, int col_off, hipStream_t s, _Float16* img16) {
  constexpr int T = C >= 128 ? C : 128;
  const dim3 grid((unsigned)(sp.g.rows / kScatterRows));
  if (sp.dx_f16) hipLaunchKernelGGL((k_scatter_vox_win<C, 1, kWinFloats>), grid, dim3(T), 0, s, sp, gv, col_off, img16);
  else hipLaunchKernelGGL((k_scatter_vox_win<C, 0, kWinFloats>), grid, dim3(T), 0, s, sp, gv, col_off, (_Float16*)nullptr);
}

// packed-half atomics: zero the level's fp16 image, run `scatter` into it, then one pass to the fp32 gradient
// (k_h16_to_grad: 1 / s times `unscale`, the inverse of the image's own scale)
template <class Scatter>
static hipError_t scatter_via_h16(const ScatterParams& sp, const ListVoxLevel& gv, _Float16* img16, size_t n_elem,
                                  float unscale, hipStream_t s, Scatter scatter) {
  hipError_t e = hipMemsetAsync(img16, 0, n_elem * 2, s);
  if (e != hipSuccess) return e;
  e = scatter(img16);
  if (e != hipSuccess) return e;
  const int64_t n8 = (int64_t)(n_elem / 8);
  const int64_t cb = (n8 + 255) / 256;
  hipLaunchKernelGGL(k_h16_to_grad, dim3((unsigned)(cb < 8192 ? cb : 8192)), dim3(256), 0, s,
                     (const _Float16*)img16, (float*)gv.data, n8, sp.scale, unscale);
  return hipGetLastError();
}

// f(std::integral_constant<int, C>) where C is one of Cs, the channel counts a form's kernels exist for
template <int... Cs, class F>
static hipError_t with_channels(int C, F&& f) {
  hipError_t e = hipErrorInvalidValue;
  (void)((C == Cs ? (e = f(std::integral_constant<int, Cs>()), true) : false) || ...);
  return e;
}

// executes plan_vox_adjoint (vox_adjoint_plan.h: which form, which stream, which flush -- nothing is decided here)
hipError_t launch_scatter_vox(const ScatterParams& sp, const FeatLayout& L, const ListVoxLevel grad_vox[LIST_N_VOX_LEVELS],
                              const VoxGatherBuffers& vb, const ScatterStreams& st) {
  // LIST_SCATTER_BOX and LIST_SCATTER_F32: environment, read once
  static const int box_mode = [] { const char* e = getenv("LIST_SCATTER_BOX"); return e ? atoi(e) : -1; }();
  static const bool f32_diagnostic = [] { const char* e = getenv("LIST_SCATTER_F32"); return e && e[0] == '1'; }();
  const int B = (int)((sp.g.p_begin + sp.g.n_valid + sp.g.N - 1) / sp.g.N);
  const VoxCall c = {sp.g.n_valid, sp.g.rows, B, sp.g.Kp, sp.dx_f16 != 0, sp.forked != 0, vb.mode, vb.bins != nullptr,
                     vb.h16 ? vb.h16_bytes : 0, vb.h16w ? vb.h16w_bytes : 0, box_mode, f32_diagnostic};      // (VoxCall's order)
  VoxChoice plan[LIST_N_VOX_LEVELS];
  plan_vox_adjoint(c, grad_vox, L.vox_off, plan);
  const hipStream_t lanes[4] = {st.gather, st.direct, st.window, st.window2};      // by VoxLane
  const int nblocks = sp.g.rows / kScatterRows, cap = direct_grid_cap(c.forked);
  const dim3 pgrid((unsigned)(nblocks < cap ? nblocks : cap));                       // the direct forms' persistent grid
  for (int l = 0; l < LIST_N_VOX_LEVELS; ++l) {
    const VoxChoice& p = plan[l];
    if (p.form == VOX_SKIP) continue;
    const ListVoxLevel& gv = grad_vox[l];
    const int col_off = L.vox_off[l];
    const hipStream_t s = lanes[p.lane];
    // the form's launches; img16: the level's zeroed fp16 image (the packed-half flushes), else null
    auto form = [&](_Float16* img16) -> hipError_t {
      switch (p.form) {
        case VOX_GATHER8: case VOX_GATHER1:
          return with_channels<16, 32, 64, 128, 256>(gv.C, [&](auto cc) {
            return gather_level<decltype(cc)::value>(sp, gv, col_off, c.B, p.form == VOX_GATHER8, vb, s);
          });
        case VOX_DIRECT_H2:
          return with_channels<32, 64>(gv.C, [&](auto cc) {
            hipLaunchKernelGGL(k_scatter_vox_h2<decltype(cc)::value>, pgrid, dim3(256), 0, s, sp, gv, col_off, nblocks, img16);
            return hipSuccess;
          });
        case VOX_BOX: return launch_scatter_vox_box(sp, gv, col_off, img16, s);
        case VOX_WINDOW:
          return with_channels<64, 128, 256>(gv.C, [&](auto cc) {
            constexpr int C = decltype(cc)::value;
            if (p.win_floats == kWinFloatsSmall) launch_scatter_vox_win<C, kWinFloatsSmall>(sp, gv, col_off, s, img16);
            else launch_scatter_vox_win<C, kWinFloatsLarge>(sp, gv, col_off, s, img16);
            return hipGetLastError();
          });
        case VOX_DIRECT:
          return with_channels<4, 8, 16, 32, 64, 128, 256>(gv.C, [&](auto cc) {
            constexpr int C = decltype(cc)::value;
            hipLaunchKernelGGL((sp.dx_f16 ? k_scatter_vox<C, 1> : k_scatter_vox<C, 0>), pgrid, dim3(256), 0, s, sp, gv, col_off, nblocks);
            return hipGetLastError();
          });
        case VOX_SCALAR: {
          const int nb1 = (int)(((int64_t)sp.g.n_valid * 64 + 255) / 256), cap1 = 4 * cap;
          const dim3 grid((unsigned)(nb1 < cap1 ? nb1 : cap1));
          hipLaunchKernelGGL((sp.dx_f16 ? k_scatter_vox1<1> : k_scatter_vox1<0>), grid, dim3(256), 0, s, sp, gv, col_off);
          return hipGetLastError();
        }
        default: return hipErrorInvalidValue;
      }
    };
    const size_t n_elem = (size_t)c.B * gv.image_stride;
    char* const slot1 = (char*)vb.h16w + h16w_slot_bytes(c.h16w_bytes);
    hipError_t e = hipSuccess;
    switch (p.flush) {
      case VOX_FLUSH_H16: e = scatter_via_h16(sp, gv, (_Float16*)vb.h16, n_elem, 1.f, s, form); break;
      case VOX_FLUSH_H16W0: e = scatter_via_h16(sp, gv, (_Float16*)vb.h16w, n_elem, 1.f / kWinPkScale, s, form); break;
      case VOX_FLUSH_H16W1: e = scatter_via_h16(sp, gv, (_Float16*)slot1, n_elem, 1.f / kWinPkScale, s, form); break;
      case VOX_FLUSH_F32: e = hipMemsetAsync((void*)gv.data, 0, n_elem * sizeof(float), s);   // (also ahead of an invalid level)
        [[fallthrough]];
      case VOX_FLUSH_STORE: if (e == hipSuccess) e = form(nullptr);
    }
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace list
