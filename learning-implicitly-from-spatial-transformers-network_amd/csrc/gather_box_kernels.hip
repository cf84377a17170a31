// Coarse voxel levels (stencil shorter than a voxel: the 16^3 and 8^3 x 128-channel levels, 58 % of all tap
// contributions) on the matrix cores: network/modules.py:256-265 for those levels as small GEMMs.
//
// A stencil sample (point p, stencil point j) is a weighted sum of the 2 x 2 x 2 voxels around it,
//   out[(p,j)][c] = sum_v Wt[(p,j)][v] * V[v][c],   Wt = hx[vx] * hy[vy] * hz[vz]   (two non-zeros per axis).
// Samples that share their "window" -- the 2 x 2 cells (y0, y0+1) x (z0, z0+1) and the 8 x-slots starting at
// 4 * (x0 >> 2) -- share the 32 voxel rows V[32][C] of that window, so 16 of them are one MFMA column tile:
//   D^T[c][s] = sum_k V^T[c][k] * Wt^T[k][s],  k = 8 * (2 * dz + dy) + x-slot,  v_mfma_f32_16x16x32_f16,
// with the weights formed per lane directly in the B-fragment layout (8 consecutive k = the 8 x-slots of one
// (dy, dz) cell: the product (hy * hz) times the two non-zero x weights, split hi + lo in fp16 so that the
// products are exact in the fp32 accumulator: same interpolation arithmetic as the scalar kernels up to the
// order of the fp32 sums) and V^T read with ds_read_b64_tr_b16 from a channels-last LDS copy of the voxel box
// that a run of Morton-consecutive points touches (ONE coalesced copy instead of 32 tap requests per point).
//
// Every sample's arithmetic depends on nothing but its own window and weights -- the k position of every voxel
// is a function of absolute voxel coordinates, zero-weight slots add exact zeros -- so results do not depend on
// which points share a workgroup, a run or a tile: sharded == unsharded bit for bit still holds.
// Non-finite voxels inside a window turn 0 * inf into NaN for samples that do not touch them; such rows are
// flagged by fc_0's probe and redone by k_gather_fixup with the reference's skip semantics, like before.
//
// Workgroup = 64 consecutive rows (Morton order), 256 threads:
//   1. per point: the three per-axis weight records of the centre / -d / +d coordinate (AxisW), its tap range;
//   2. wave 0 cuts the 64 points into aligned power-of-two runs whose voxel box fits the LDS box (a segment
//      tree over the tap ranges by wave shuffles; a single point always fits: 4 x 4 x 4);
//   3. per run: the box is copied to LDS (XOR-swizzled 16-B chunks: the transposed reads are bank-conflict
//      free), the run's samples are counting-sorted by window key in LDS and cut into tiles of <= 16 samples,
//      and the four waves walk the tiles: weights -> 16 MFMAs (8 channel tiles x hi / lo) -> 16-B stores of
//      8 consecutive channels per lane straight into the sample's X row.
#include "list_common.h"
#include "point_math.h"
#include "box_partition.h"

namespace list {

constexpr int kBoxSamples = kBoxPts * LIST_N_STENCIL;        // 448 (kBoxPts points per workgroup: query_fwd_plan.h)
constexpr int kBoxMaxKeys = 512;                             // window keys a run may have
constexpr int kBoxNb = 2;                                    // tiles per turn of a wave
constexpr int kBoxRowsBig = 256;                             // LDS box rows, levels wider than 8 voxels
constexpr int kBoxRowsSmall = 128;

template <int C, int MAXROWS> struct BoxLds {
  static constexpr int kRowBytes = 2 * C;
  static constexpr int box = 0;
  static constexpr int ptab = box + MAXROWS * kRowBytes;                 // AxisW [64][3 axes][3 variants]
  static constexpr int run = ptab + kBoxPts * 9 * (int)sizeof(AxisW);    // RunBox [64], indexed by first point
  static constexpr int keyinfo = run + kBoxPts * (int)sizeof(RunBox);    // int [512]: counters, then sample offsets
  static constexpr int tileinfo = keyinfo + kBoxMaxKeys * 4;             // unsigned [448]
  static constexpr int sorted = tileinfo + kBoxSamples * 4;              // short [448]: sample ids in key order
  static constexpr int pbox = sorted + kBoxSamples * 2;                  // int [64][4]: tap range per axis, image
  static constexpr int misc = pbox + kBoxPts * 16;                       // int [8]: tile count
  static constexpr int total = misc + 64;
};

// grid = rows / 64, block = 256
template <int C, int MAXROWS>
__global__ __launch_bounds__(256) void k_gather_vox_box(GatherParams g, ListVoxLevel lv, int col_off) {
  using L = BoxLds<C, MAXROWS>;
  static_assert(C % 128 == 0 && C <= 256, "channel tiles of 32 and a 16-chunk swizzle");
  static_assert(MAXROWS >= 64 && MAXROWS <= 256, "a single point's 4 x 4 x 4 box must fit; row indices are 8-bit");
  constexpr int NT = C / 16;                                  // 16-channel MFMA row tiles
  constexpr int RB = L::kRowBytes;
  constexpr int CH = RB / 16;                                 // 16-B chunks per voxel row
  constexpr int RPP = 256 / CH;                               // box rows per pass of the workgroup
  constexpr int NL = (MAXROWS + RPP - 1) / RPP;               // 16-B loads per thread for a full box
  __shared__ __attribute__((aligned(16))) char smem[L::total];
  AxisW* ptab = (AxisW*)(smem + L::ptab);
  RunBox* runs = (RunBox*)(smem + L::run);
  int* keyinfo = (int*)(smem + L::keyinfo);
  unsigned* tileinfo = (unsigned*)(smem + L::tileinfo);
  short* sorted = (short*)(smem + L::sorted);
  int* pbox = (int*)(smem + L::pbox);
  int* misc = (int*)(smem + L::misc);

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = uni(tid >> 6);
  const int blk = xcd_contiguous_block(blockIdx.x, gridDim.x);
  const int64_t row0 = (int64_t)blk * kBoxPts;
  const int W = lv.W, H = lv.H, D = lv.D;

  // ---- 1a. waves 0..2: axis `wave` of the 64 points -- weight records of the centre / -d / +d coordinate; wave 3: the
  //          key counters -----------------------------------------------------------------------------------------------
  if (wave < 3) {
    box_point_records(g, (int)row0 + lane, lane, wave, W, H, D, ptab, pbox);
  } else {
    for (int k = lane; k < kBoxMaxKeys; k += 64) keyinfo[k] = 0;
  }
  __syncthreads();
  // ---- 1b. wave 0: aligned power-of-two runs whose box fits (segment tree over the tap ranges) ----------------------
  if (wave == 0) box_cut_runs<MAXROWS, kBoxMaxKeys>(pbox, lane, runs);
  __syncthreads();

  const unsigned short* __restrict__ vsrc = (const unsigned short*)lv.data;
  unsigned short* __restrict__ xh = g.x_hi;
  const int q = lane >> 4, col = lane & 15;                  // MFMA lane roles: k block / sample column
  const int tr_r = (lane >> 2) & 3, tr_p = lane & 3;         // transposed read: row within the 4-row block, 4-channel group

  int first = 0;
#pragma unroll 1
  while (first < kBoxPts) {
    const RunBox rb = runs[first];
    const int count = uni(rb.count), rb_b = uni(rb.b);
    RunDims d = run_dims(uni(rb.lo), uni(rb.n));
    d.set_inverses<true>();                                     // (a run without a valid point still zeroes padding rows)
    const int lox = d.lox, loy = d.loy, loz = d.loz, nx = d.nx, ny = d.ny, nz = d.nz, rows = d.rows;
    const int fw0 = lox >> 2;
    const int nfw = rows ? ((lox + nx - 1) >> 2) - fw0 + 1 : 0;
    const int nkeys = nfw * ny * nz;
    const int inv_ny = d.inv_ny, inv_nz = box_inv<true>(nz);    // window key -> (y0, z0, window)

    // ---- 2a. the voxel box: requested now (16-B chunks, lanes over channels: coalesced 256-B rows), landed in LDS
    //          behind the bucketing below ---------------------------------------------------------------------------
    uint4 bv[NL];
    int bdst[NL];
    {
      const int chunk = tid & (CH - 1);
      const int64_t ibase = (int64_t)rb_b * lv.image_stride;
#pragma unroll
      for (int i = 0; i < NL; ++i) {
        const int r = i * RPP + tid / CH;
        bdst[i] = -1;
        if (r < rows) {
          int ix, iy, iz;
          d.row_to_xyz(r, ix, iy, iz);
          const int64_t src = ibase + ((int64_t)((loz + iz) * H + (loy + iy)) * W + (lox + ix)) * C + chunk * 8;
          bv[i] = *(const uint4*)(vsrc + src);
          // physical position: chunk ^ ((ix & 3) << 2), 8-B halfs swapped in odd (iy + iz) cells: the 32 lanes of a
          // transposed read (4 x-slots x 2 cells x 4 channel groups) then hit 32 distinct 8-B bank slots
          const int par = (iy + iz) & 1;
          bdst[i] = (r * RB + ((chunk ^ ((ix & 3) << 2)) << 4)) | (par << 30);
        }
      }
    }

    // ---- 2b. window key of every sample (counters are zero); padding rows: their X columns are zero ----------------
    const int nsamp = count * LIST_N_STENCIL;
    int my_key[2], my_slot[2], my_sid[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int s = tid + 256 * i;
      my_key[i] = -1; my_slot[i] = 0; my_sid[i] = 0;
      if (s >= nsamp) continue;
      const int pl = s / LIST_N_STENCIL, j = s - pl * LIST_N_STENCIL, pt = first + pl;
      if ((int)row0 + pt >= g.n_valid) {                      // padding row
        uint4* o = (uint4*)(xh + (row0 + pt) * g.Kp + col_off + j * C);
#pragma unroll 1
        for (int c8 = 0; c8 < C / 8; ++c8) o[c8] = make_uint4(0u, 0u, 0u, 0u);
        continue;
      }
      const int x0 = ptab[(pt * 3 + 0) * 3 + variant_of(0, j)].i0;
      const int y0 = ptab[(pt * 3 + 1) * 3 + variant_of(1, j)].i0;
      const int z0 = ptab[(pt * 3 + 2) * 3 + variant_of(2, j)].i0;
      const int key = (((x0 >> 2) - fw0) * nz + (z0 - loz)) * ny + (y0 - loy);
      my_key[i] = key;
      my_sid[i] = pt * 8 + j;
      my_slot[i] = atomicAdd(&keyinfo[key], 1);
    }
    __syncthreads();

    // ---- 2c. wave 0: exclusive scan over the keys -> sample offsets, tiles; meanwhile the box lands -----------------
    if (wave == 0) {
      int carry = 0;                                          // tiles << 16 | samples
#pragma unroll 1
      for (int k0 = 0; k0 < nkeys; k0 += 64) {
        const int key = k0 + lane;
        const int cnt = key < nkeys ? keyinfo[key] : 0;
        const int ntl = (cnt + 15) >> 4;
        const int mine = (ntl << 16) | cnt;
        int incl = mine;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
          const int v = __shfl_up(incl, off);
          if (lane >= off) incl += v;
        }
        const int at = carry + incl - mine;
        carry += __shfl(incl, 63);
        if (key < nkeys) {
          keyinfo[key] = at & 0xffff;
          if (cnt) {
            // tiles of this key: start | n << 9 | y0 << 14 | z0 << 19 | window << 24
            const int yz = (key * inv_ny) >> 16, y0 = key - yz * ny;
            const int fw = (yz * inv_nz) >> 16, z0 = yz - fw * nz;
            int tile = at >> 16, start = at & 0xffff;
            for (int i = 0; i < ntl; ++i, ++tile, start += 16) {
              const int n = cnt - 16 * i < 16 ? cnt - 16 * i : 16;
              tileinfo[tile] = (unsigned)start | ((unsigned)n << 9) | ((unsigned)y0 << 14) | ((unsigned)z0 << 19) |
                               ((unsigned)fw << 24);
            }
          }
        }
      }
      if (lane == 0) misc[0] = carry >> 16;                   // number of tiles
    }
#pragma unroll
    for (int i = 0; i < NL; ++i) {
      if (bdst[i] < 0) continue;
      const uint4 w = (bdst[i] >> 30) & 1 ? make_uint4(bv[i].z, bv[i].w, bv[i].x, bv[i].y) : bv[i];
      *(uint4*)(smem + L::box + (bdst[i] & 0x3fffffff)) = w;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 2; ++i)
      if (my_key[i] >= 0) sorted[keyinfo[my_key[i]] + my_slot[i]] = (short)my_sid[i];
    __syncthreads();
    for (int k = tid; k < nkeys; k += 256) keyinfo[k] = 0;    // counters of the next run (nothing below reads them)

    // ---- 2d. tiles: <= 16 samples of one window; two tiles per turn (independent chains of LDS look-ups) -----------
    const int ntiles = uni(misc[0]);
    constexpr int NB = kBoxNb;
#pragma unroll 1
    for (int T = wave; T < ntiles; T += 4 * NB) {
      unsigned bh[NB][4], bl[NB][4];
      int sid[NB], abase[NB][2], aswz[NB][2];
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        const int Tb = T + 4 * b < ntiles ? T + 4 * b : T;    // (a turn's second tile may not exist: recomputed, not stored)
        const unsigned ti = (unsigned)uni((int)tileinfo[Tb]);
        const int start = ti & 511, n = (ti >> 9) & 31, y0 = (ti >> 14) & 31, z0 = (ti >> 19) & 31, fw = ti >> 24;
        // weights of this lane's sample for the 8 x-slots of cell q = (dy, dz): two non-zeros, hi + lo in fp16
        // (no branch: the look-up chains of the turn's tiles overlap; a column beyond n repeats the last sample
        // with weight 0)
        {
          const bool live = col < n;
          sid[b] = sorted[start + (live ? col : n - 1)];
          const int pt = sid[b] >> 3, j = sid[b] & 7;
          const AxisW fx = ptab[(pt * 3 + 0) * 3 + variant_of(0, j)];
          const AxisW fy = ptab[(pt * 3 + 1) * 3 + variant_of(1, j)];
          const AxisW fz = ptab[(pt * 3 + 2) * 3 + variant_of(2, j)];
          const float s = live ? ((q & 1) ? fy.w1 : fy.w0) * ((q >> 1) ? fz.w1 : fz.w0) : 0.f;
          const float wa = s * fx.w0, wb = s * fx.w1;
          const unsigned hi2 = pk_h2(wa, wb);
          const float ra = wa - h2f((unsigned short)(hi2 & 0xffffu)), rb2 = wb - h2f((unsigned short)(hi2 >> 16));
          const unsigned lo2 = pk_h2(ra, rb2);
          const int phi = fx.i0 & 3;                          // x-slot of the base tap in its window
          // slots phi, phi + 1 of the 8-slot fragment (4 registers of two halfs)
          bh[b][0] = phi == 0 ? hi2 : (phi == 1 ? hi2 << 16 : 0u);
          bh[b][1] = phi == 2 ? hi2 : (phi == 3 ? hi2 << 16 : (phi == 1 ? hi2 >> 16 : 0u));
          bh[b][2] = phi == 3 ? hi2 >> 16 : 0u;
          bh[b][3] = 0u;
          bl[b][0] = phi == 0 ? lo2 : (phi == 1 ? lo2 << 16 : 0u);
          bl[b][1] = phi == 2 ? lo2 : (phi == 3 ? lo2 << 16 : (phi == 1 ? lo2 >> 16 : 0u));
          bl[b][2] = phi == 3 ? lo2 >> 16 : 0u;
          bl[b][3] = 0u;
          if (!live) sid[b] = -1;
        }
        if (T + 4 * b >= ntiles) sid[b] = -1;
        // V^T fragments: this lane addresses row tr_r of the 4-row block, cell q, channel group tr_p.  Cells and slots
        // beyond the box carry weight 0 for every sample of the run: they re-read the box's border rows
        const int iy = min(y0 + (q & 1), ny - 1), iz = min(z0 + (q >> 1), nz - 1);
        const int par = (iy + iz) & 1;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int ix = min(max(4 * (fw0 + fw) + 4 * h + tr_r - lox, 0), nx - 1);
          abase[b][h] = L::box + ((iz * ny + iy) * nx + ix) * RB + (tr_p << 4);
          aswz[b][h] = ((ix & 3) << 6) | (par << 3);
        }
      }
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        if (b > 0 && T + 4 * b >= ntiles) break;
        const f16x8 bhi = __builtin_bit_cast(f16x8, make_uint4(bh[b][0], bh[b][1], bh[b][2], bh[b][3]));
        const f16x8 blo = __builtin_bit_cast(f16x8, make_uint4(bl[b][0], bl[b][1], bl[b][2], bl[b][3]));
        // channels of row tile t: 32 (t >> 1) + 8 p + 4 (t & 1) + 0..3 for 4-channel group p -- so that a lane's
        // accumulators of tiles 2u, 2u + 1 are 8 consecutive channels.  All 16 transposed reads first, then the MFMAs
        s16x4 a0[NT], a1[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) {
          const int ct = ((t >> 1) << 6) | ((t & 1) << 3);
          a0[t] = tr_read16(smem + abase[b][0] + (ct ^ aswz[b][0]));
          a1[t] = tr_read16(smem + abase[b][1] + (ct ^ aswz[b][1]));
        }
        f32x4v acc[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) {
          const f16x8 a = __builtin_bit_cast(f16x8, (s16x8){a0[t][0], a0[t][1], a0[t][2], a0[t][3], a1[t][0], a1[t][1], a1[t][2], a1[t][3]});
          f32x4v c = {0.f, 0.f, 0.f, 0.f};
          c = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, bhi, c, 0, 0, 0);
          acc[t] = c;
        }
#pragma unroll
        for (int t = 0; t < NT; ++t) {
          const f16x8 a = __builtin_bit_cast(f16x8, (s16x8){a0[t][0], a0[t][1], a0[t][2], a0[t][3], a1[t][0], a1[t][1], a1[t][2], a1[t][3]});
          acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, blo, acc[t], 0, 0, 0);
        }
        // D^T: column = sample (lane & 15), rows 4 q + reg of tile t = channels 32 (t >> 1) + 8 q + 4 (t & 1) + reg.
        // Plain stores: the four lanes of a sample cover 64 B per instruction and the partial lines merge in L2
        // (non-temporal stores of such pieces took the kernel from 0.085 to 0.30 ms)
        if (sid[b] >= 0) {
          const int pt = sid[b] >> 3, j = sid[b] & 7;
          unsigned short* dst = xh + (row0 + pt) * g.Kp + col_off + j * C + 8 * q;
          typedef __attribute__((ext_vector_type(4))) unsigned u32x4;
#pragma unroll
          for (int u = 0; u < NT / 2; ++u) {
            const uint2 lo = half4_inrange(make_float4(acc[2 * u][0], acc[2 * u][1], acc[2 * u][2], acc[2 * u][3]));
            const uint2 hi = half4_inrange(make_float4(acc[2 * u + 1][0], acc[2 * u + 1][1], acc[2 * u + 1][2], acc[2 * u + 1][3]));
            *(u32x4*)(dst + 32 * u) = (u32x4){lo.x, lo.y, hi.x, hi.y};
          }
        }
      }
    }
    first += count;
    if (first < kBoxPts) __syncthreads();                     // the next run overwrites the box and the lists
  }
}

hipError_t launch_gather_vox_box(const GatherParams& g, const ListVoxLevel& lv, int col_off, hipStream_t s, int order) {
  // the 8^3 level's boxes are small: a 128-row box leaves room for three workgroups per CU
  const int big = lv.W > lv.H ? (lv.W > lv.D ? lv.W : lv.D) : (lv.H > lv.D ? lv.H : lv.D);
  if (big > 8)
    LIST_LAUNCH((k_gather_vox_box<128, kBoxRowsBig>), dim3(g.rows / kBoxPts), dim3(256), 0, s, order, g, lv, col_off);
  else
    LIST_LAUNCH((k_gather_vox_box<128, kBoxRowsSmall>), dim3(g.rows / kBoxPts), dim3(256), 0, s, order, g, lv, col_off);
  return hipGetLastError();
}

}  // namespace list
