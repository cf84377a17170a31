// Adjoint of the matrix-core gather of a coarse voxel level (gather_box_kernels.hip; the reference's autograd of
// network/modules.py:256-265 for the 16^3 and 8^3 x 128-channel levels): the gradient of the voxel box that a run
// of Morton-consecutive points touches is ONE small dense product on the matrix cores,
//   dV^T[c][v] = sum_k dX^T[c][k] * Wt[k][v],   k = (point, stencil slot j = 0..6 and a zero slot),  v = box row,
//   one K-step of a 16x16x32 MFMA = 4 points x 8 slots,
// instead of the read-add-write chain of k_scatter_vox_win (bwd_scatter_kernels.hip) that sums the same terms on the
// VALU, one point and one window slot at a time.  Wt is 94 % zeros (8 taps of <= 128 box rows) and that does not matter:
// the dense product of a workgroup is 15 - 30 MFLOP, a few thousand matrix-core cycles.
//   A = dX^T: the run's dX rows are copied to LDS as 16-bit images ([sample][128], 16-B chunks XOR-swizzled by the
//       stencil slot, 8-B halfs swapped for odd points) and read with ds_read_b64_tr_b16, like the forward's V^T;
//   B = Wt:   formed per lane in the B-fragment layout -- a lane owns ONE box row (its voxel) and the 8 slots of ONE point
//       per K-step, so its 8 values are products of three per-axis factors looked up by comparing the voxel's coordinates
//       with the point's nine axis records; split hi + lo in the operand's 16-bit format so that the products are exact in
//       the fp32 accumulator (same interpolation arithmetic as the VALU kernels up to the order of the fp32 sums);
//   D:        wave w accumulates box-row tiles w and w + 4 (16 rows each) x all 128 channels, 64 accumulator registers.
// One kernel body, three instantiations: what the element type of dX decides (staged image, 16-bit format, MFMA sequence,
// LDS region, flush) is an operand policy below -- fp16 with the packed-half flush, fp16 with the diagnostic fp32 flush,
// and fp32 dX as bf16 hi + lo.
//
// Workgroup = 64 consecutive rows (Morton order), 256 threads; runs = the forward's aligned power-of-two runs whose box
// has at most 128 rows (a single point's 4 x 4 x 4 always fits; at 16^3 that is ~8 points per run).
//
// Measured (fp16 form, config 2, 160 000 points, in-line backward, rocprofv3 kernel trace): 16^3 level 0.519 -> 0.224 ms, 8^3 level
// 0.28 -> 0.118 ms against k_scatter_vox_win; of the 0.239 ms it took before its row -> voxel divisions became multiply-shifts
// (0.224 now) the flush was 0.085 (exposed), the K loop 0.114 -- the weights
// on the VALU more than the 32 MFMAs of a K-step: hi-only weights save 0.02; the per-axis factors read from per-point
// LDS tables instead of compared and selected per lane: 0.224 -> 0.231 ms, dropped --, and 0.08 is what reading 287 MB of
// dX, the point records and the partition take (profiles/r04b_box_adjoint.txt).  fp16 training step: 6.63 -> 6.29 ms.
#include "list_common.h"
#include "point_math.h"
#include "box_partition.h"
#include "mfma_common.h"

namespace list {

// (kAdjPts = 64 points per workgroup, kAdjC = 128 channels and the fp16 image's scale kWinPkScale: vox_adjoint_plan.h)
constexpr int kAdjRows = 128;                     // box rows (8 tiles of 16: two per wave)
constexpr int kAdjChunkPts = 8;                   // points staged per chunk (two K-steps)
constexpr int kAdjNT = kAdjC / 16;                // 16-channel tiles
constexpr int kAdjRowBytes = 2 * kAdjC;                                  // 256: one 16-bit plane of a staged row
constexpr int kAdjStageRows = kAdjChunkPts * LIST_N_STENCIL;             // 56
constexpr int kAdjPlaneBytes = kAdjStageRows * kAdjRowBytes;             // 14336

// LDS: the operand's region (two staging buffers; later the finished box), then the tables every form has
template <int REGION> struct AdjLds {
  static constexpr int stage = 0;
  static constexpr int zero = REGION;                                           // one row of zeros
  static constexpr int ptab = zero + kAdjRowBytes;                              // AxisW [64][3 axes][3 variants]
  static constexpr int run = ptab + kAdjPts * 9 * (int)sizeof(AxisW);           // RunBox [64]
  static constexpr int pbox = run + kAdjPts * (int)sizeof(RunBox);              // int [64][4]
  static constexpr int total = pbox + kAdjPts * 16;
};

// global address of box row (ix, iy, iz) of the run's image, in elements of 128-channel rows
__device__ __forceinline__ int64_t adj_voxel(const RunDims& d, const ListVoxLevel& gv, int ix, int iy, int iz) {
  return ((int64_t)((d.loz + iz) * gv.H + (d.loy + iy)) * gv.W + (d.lox + ix)) * kAdjC;
}

// ---- operand policies: what the element type of dX decides -- the staged image, the weights' 16-bit format, the MFMA
// sequence of a K-step and the flush.  Runs, tiles, lane roles and the weights' arithmetic are the kernel's. -----------

// fp16 dX.  A = dX^T: the rows are copied to LDS as they lie in memory ([sample][128 halfs]).  The finished box goes
// through LDS once more ([row][128 halfs] at the window scale kWinPkScale) so that the flush is the one
// k_scatter_vox_win has: packed-half atomics into img16, the level's zeroed fp16 image, lanes over channel pairs, whole
// 256-B rows per instruction.
// F32OUT (diagnostic, LIST_SCATTER_F32=1): the accumulators go straight to the level's zeroed fp32 gradient as float
// atomics, unrounded -- the form tests/test_box_adjoint_gpu.py compares with the window kernel's fp32 flush at 2e-5.
template <int F32OUT> struct AdjF16 {
  static constexpr int kBufBytes = kAdjPlaneBytes;                              // 2 x [56][256 B]
  static constexpr int kRegion = kAdjRows * kAdjRowBytes;                       // 32768: the box [128][256 B]
  static constexpr bool kScaleInFlush = F32OUT;                                 // 1 / s is read per run (diagnostic form only)
  using L = AdjLds<kRegion>;
  typedef unsigned short Elem;
  typedef uint4 Piece;                                                          // 8 channels of a staged row

  static __device__ __forceinline__ Piece no_piece() { return make_uint4(0u, 0u, 0u, 0u); }
  static __device__ __forceinline__ Piece load_piece(const Elem* src) { return *(const uint4*)src; }
  static __device__ __forceinline__ void store_piece(char* buf, int off, bool odd, const Piece& p) {
    *(uint4*)(buf + off) = odd ? make_uint4(p.z, p.w, p.x, p.y) : p;
  }
  static __device__ __forceinline__ unsigned pk2(float a, float b) { return pk_h2(a, b); }
  static __device__ __forceinline__ float up(unsigned short h) { return h2f(h); }

  // A of a K-step: every transposed read at once, ahead of the weights' VALU work
  struct AFrag { s16x4 a0[kAdjNT], a1[kAdjNT]; };
  static __device__ __forceinline__ AFrag a_frags(const char* a_lo, const char* a_hi, bool, bool, const int (&aoff)[kAdjNT]) {
    AFrag f;
#pragma unroll
    for (int t = 0; t < kAdjNT; ++t) {
      f.a0[t] = tr_read16(a_lo + aoff[t]);
      f.a1[t] = tr_read16(a_hi + aoff[t]);
    }
    return f;
  }
  static __device__ __forceinline__ void mma(const AFrag& f, const int (&)[kAdjNT], const uint4 (&bhi)[2], const uint4 (&blo)[2],
                                             bool own0, bool own1, f32x4v (&acc)[2][kAdjNT]) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      if (i == 0 ? !own0 : !own1) continue;
      const f16x8 bh = __builtin_bit_cast(f16x8, bhi[i]), bl = __builtin_bit_cast(f16x8, blo[i]);
#pragma unroll
      for (int t = 0; t < kAdjNT; ++t) {
        const f16x8 a = __builtin_bit_cast(f16x8, (s16x8){f.a0[t][0], f.a0[t][1], f.a0[t][2], f.a0[t][3], f.a1[t][0], f.a1[t][1], f.a1[t][2], f.a1[t][3]});
        acc[i][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, bh, acc[i][t], 0, 0, 0);
      }
      // the lo plane of the weights: rounding them to fp16 alone would save 16^3 level 0.253 -> 0.230 ms -- not
      // worth the exactness
#pragma unroll
      for (int t = 0; t < kAdjNT; ++t) {
        const f16x8 a = __builtin_bit_cast(f16x8, (s16x8){f.a0[t][0], f.a0[t][1], f.a0[t][2], f.a0[t][3], f.a1[t][0], f.a1[t][1], f.a1[t][2], f.a1[t][3]});
        acc[i][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, bl, acc[i][t], 0, 0, 0);
      }
    }
  }

  // D: column = box row (lane & 15), rows 4 q + reg of tile t = channels 32 (t >> 1) + 8 q + 4 (t & 1) + reg
  static __device__ __forceinline__ void flush(char* smem, const f32x4v (&acc)[2][kAdjNT], const RunDims& d, int rb_b, int wave,
                                               int lane, bool own0, bool own1, const ListVoxLevel& gv, float inv_s,
                                               _Float16* __restrict__ img16) {
    const int q = lane >> 4, col = lane & 15;
    if (F32OUT) {
      float* base = (float*)gv.data + (int64_t)rb_b * gv.image_stride;
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        if (i == 0 ? !own0 : !own1) continue;
        const int v = 16 * (wave + 4 * i) + col;
        if (v >= d.rows) continue;
        int ix, iy, iz;
        d.row_to_xyz(v, ix, iy, iz);
        float* dst = base + adj_voxel(d, gv, ix, iy, iz);
#pragma unroll
        for (int t = 0; t < kAdjNT; ++t)
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float val = acc[i][t][e];
            if (val != 0.f) atomicAdd(dst + 32 * (t >> 1) + 8 * q + 4 * (t & 1) + e, val * inv_s);
          }
      }
      return;
    }
    __syncthreads();                   // every wave is done with the staging buffers: the box takes their place
    // 16-B pieces of 8 consecutive channels, chunk XOR (row & 15) (the 16 rows of a tile land on distinct banks)
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      if (i == 0 ? !own0 : !own1) continue;
      const int v = 16 * (wave + 4 * i) + col;
#pragma unroll
      for (int u = 0; u < kAdjNT / 2; ++u) {
        const f32x4v c0 = acc[i][2 * u], c1 = acc[i][2 * u + 1];
        const uint2 lo = half4_inrange(make_float4(c0[0] * kWinPkScale, c0[1] * kWinPkScale, c0[2] * kWinPkScale, c0[3] * kWinPkScale));
        const uint2 hi = half4_inrange(make_float4(c1[0] * kWinPkScale, c1[1] * kWinPkScale, c1[2] * kWinPkScale, c1[3] * kWinPkScale));
        *(uint4*)(smem + L::stage + v * kAdjRowBytes + (((4 * u + q) ^ col) << 4)) = make_uint4(lo.x, lo.y, hi.x, hi.y);
      }
    }
    __syncthreads();
    // flush: lanes over channel pairs, one box row per wave and pass (its voxel address is scalar arithmetic) -- 256
    // contiguous bytes per atomic instruction (its share: 16^3 level 0.239 -> 0.154 ms, 8^3 0.118 -> 0.104 without it)
    typedef _Float16 half2v __attribute__((ext_vector_type(2)));
    _Float16* base16 = img16 + (int64_t)rb_b * gv.image_stride;
#pragma unroll 1
    for (int v = wave; v < d.rows; v += 4) {
      int ix, iy, iz;
      d.row_to_xyz(v, ix, iy, iz);
      const unsigned bits = *(const unsigned*)(smem + L::stage + v * kAdjRowBytes + ((((lane >> 2) ^ (v & 15)) << 4) | ((lane & 3) << 2)));
      if ((bits & 0x7fff7fffu) == 0u) continue;
      __builtin_amdgcn_global_atomic_fadd_v2f16(
          (__attribute__((address_space(1))) half2v*)(base16 + adj_voxel(d, gv, ix, iy, iz) + 2 * lane),
          __builtin_bit_cast(half2v, bits));
    }
  }
};

// fp32 dX (bf16x3, bf16): BOTH operands split into bf16 hi + lo planes and three MFMAs per product (hi * hi + hi * lo +
// lo * hi on v_mfma_f32_16x16x32_bf16: 16 mantissa bits per operand, the grade of the forward's bf16x3 products), the box
// accumulated in fp32 and flushed as float atomics into the level's zeroed gradient -- 256 contiguous bytes per
// instruction, like k_scatter_vox_win's fp32 flush.
//   staging: the dX rows of 8 points are loaded as fp32, split, and written as two [sample][128] bf16 images (the fp16
//            form's swizzle), the next chunk's fp32 pieces requested a chunk ahead (32 registers);
//   LDS:     64 KB for the fp32 box (the 2 x 2 staging images share it) + 8.5 KB of tables: two workgroups per CU.
struct AdjSplit {
  static constexpr int kBufBytes = 2 * kAdjPlaneBytes;                          // 2 buffers x (hi | lo)
  static constexpr int kRegion = kAdjRows * kAdjC * 4;                          // 65536: the fp32 box
  static constexpr bool kScaleInFlush = false;                                  // 1 / s is read once per workgroup
  using L = AdjLds<kRegion>;
  typedef float Elem;
  struct Piece { float4 a, b; };                                                // 8 channels: 32 B of fp32 in

  static __device__ __forceinline__ Piece no_piece() { return {make_float4(0.f, 0.f, 0.f, 0.f), make_float4(0.f, 0.f, 0.f, 0.f)}; }
  static __device__ __forceinline__ Piece load_piece(const Elem* src) { return {*(const float4*)src, *(const float4*)(src + 4)}; }
  // 16 B of hi and 16 B of lo out
  static __device__ __forceinline__ void store_piece(char* buf, int off, bool odd, const Piece& p) {
    uint2 h0, h1, l0, l1;
    split4(p.a, h0, l0);
    split4(p.b, h1, l1);
    *(uint4*)(buf + off) = odd ? make_uint4(h1.x, h1.y, h0.x, h0.y) : make_uint4(h0.x, h0.y, h1.x, h1.y);
    *(uint4*)(buf + kAdjPlaneBytes + off) = odd ? make_uint4(l1.x, l1.y, l0.x, l0.y) : make_uint4(l0.x, l0.y, l1.x, l1.y);
  }
  static __device__ __forceinline__ unsigned pk2(float a, float b) { return (unsigned)f2bf(a) | ((unsigned)f2bf(b) << 16); }
  static __device__ __forceinline__ float up(unsigned short h) { return bf2f(h); }

  // A of a K-step: addresses only -- the fragments are read per channel half inside mma()
  struct AFrag { const char *lo4, *hi4; int lo_plane, lo_plane_hi4; };
  static __device__ __forceinline__ AFrag a_frags(const char* a_lo, const char* a_hi, bool live_lo, bool live_hi, const int (&)[kAdjNT]) {
    return {a_lo, a_hi, live_lo ? kAdjPlaneBytes : 0, live_hi ? kAdjPlaneBytes : 0};      // (the zero row has no second plane)
  }
  static __device__ __forceinline__ void mma(const AFrag& f, const int (&aoff)[kAdjNT], const uint4 (&bhi)[2], const uint4 (&blo)[2],
                                             bool own0, bool own1, f32x4v (&acc)[2][kAdjNT]) {
    constexpr int NT = kAdjNT;
    // the channel tiles in two halves (their hi and lo fragments are 32 registers per half)
#pragma unroll
    for (int th = 0; th < 2; ++th) {
      bf16x8 ah[NT / 2], al[NT / 2];
#pragma unroll
      for (int tt = 0; tt < NT / 2; ++tt) {
        const int t = th * (NT / 2) + tt;
        const s16x4 h0 = tr_read16(f.lo4 + aoff[t]), h1 = tr_read16(f.hi4 + aoff[t]);
        const s16x4 l0 = tr_read16(f.lo4 + f.lo_plane + aoff[t]), l1 = tr_read16(f.hi4 + f.lo_plane_hi4 + aoff[t]);
        ah[tt] = __builtin_bit_cast(bf16x8, (s16x8){h0[0], h0[1], h0[2], h0[3], h1[0], h1[1], h1[2], h1[3]});
        al[tt] = __builtin_bit_cast(bf16x8, (s16x8){l0[0], l0[1], l0[2], l0[3], l1[0], l1[1], l1[2], l1[3]});
      }
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        if (i == 0 ? !own0 : !own1) continue;
        const bf16x8 bh = __builtin_bit_cast(bf16x8, bhi[i]), bl = __builtin_bit_cast(bf16x8, blo[i]);
#pragma unroll
        for (int tt = 0; tt < NT / 2; ++tt) {
          const int t = th * (NT / 2) + tt;
          acc[i][t] = mfma16<0>(al[tt], bh, acc[i][t]);
          acc[i][t] = mfma16<0>(ah[tt], bl, acc[i][t]);
          acc[i][t] = mfma16<0>(ah[tt], bh, acc[i][t]);
        }
      }
    }
  }

  static __device__ __forceinline__ void flush(char* smem, const f32x4v (&acc)[2][kAdjNT], const RunDims& d, int rb_b, int wave,
                                               int lane, bool own0, bool own1, const ListVoxLevel& gv, float inv_s, _Float16*) {
    const int q = lane >> 4, col = lane & 15;
    __syncthreads();                   // every wave is done with the staging images: the fp32 box takes their place
    // D: column = box row (lane & 15), rows 4 q + reg of tile t = channels 32 (t >> 1) + 8 q + 4 (t & 1) + reg -> one 16-B
    // piece of 4 channels per tile: chunk 8 (t >> 1) + 2 q + (t & 1) of the row's 32, XOR (row & 31)
    float* box = (float*)(smem + L::stage);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      if (i == 0 ? !own0 : !own1) continue;
      const int v = 16 * (wave + 4 * i) + col;
#pragma unroll
      for (int t = 0; t < kAdjNT; ++t) {
        const int chunk = (8 * (t >> 1) + 2 * q + (t & 1)) ^ (v & 31);
        *(float4*)(box + v * kAdjC + chunk * 4) = make_float4(acc[i][t][0], acc[i][t][1], acc[i][t][2], acc[i][t][3]);
      }
    }
    __syncthreads();
    // flush: one box row per wave and pass, two instructions of 64 channels (256 contiguous bytes) each
    float* base = (float*)gv.data + (int64_t)rb_b * gv.image_stride;
#pragma unroll 1
    for (int v = wave; v < d.rows; v += 4) {
      int ix, iy, iz;
      d.row_to_xyz(v, ix, iy, iz);
      float* dst = base + adj_voxel(d, gv, ix, iy, iz);
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int ch = 64 * h + lane;
        const float val = box[v * kAdjC + (((ch >> 2) ^ (v & 31)) << 2) + (ch & 3)];
        if (val != 0.f) atomicAdd(dst + ch, val * inv_s);
      }
    }
  }
};

enum { ADJ_F16_PK = 0, ADJ_F16_F32 = 1, ADJ_SPLIT = 2 };      // k_scatter_vox_box<FORM>
template <int FORM> struct AdjPolicy { using type = AdjF16<FORM>; };
template <> struct AdjPolicy<ADJ_SPLIT> { using type = AdjSplit; };

// grid = rows / 64, block = 256.  gv.data: the level's zeroed fp32 gradient; img16: its zeroed fp16 image (ADJ_F16_PK).
// (243 registers, two workgroups per CU; held to 168 for three the compiler spills 300 B and the kernel takes 2.2x as long)
template <int FORM>
__global__ __launch_bounds__(256, 2) void k_scatter_vox_box(ScatterParams sp, ListVoxLevel gv, int col_off,
                                                          _Float16* __restrict__ img16) {
  using P = typename AdjPolicy<FORM>::type;
  using L = typename P::L;
  static_assert(2 * P::kBufBytes <= P::kRegion, "the two staging buffers share the box's LDS");
  constexpr int RB = kAdjRowBytes;
  constexpr int NT = kAdjNT;
  __shared__ __attribute__((aligned(16))) char smem[L::total];
  AxisW* ptab = (AxisW*)(smem + L::ptab);
  RunBox* runs = (RunBox*)(smem + L::run);
  int* pbox = (int*)(smem + L::pbox);

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = uni(tid >> 6);
  const int blk = xcd_contiguous_block(blockIdx.x, gridDim.x);
  const int64_t row0 = (int64_t)blk * kAdjPts;
  const int W = gv.W, H = gv.H, D = gv.D;

  // ---- 1a. waves 0..2: axis `wave` of the 64 points (as the forward); wave 3: the zero row ---------------------------
  if (wave < 3) {
    box_point_records(sp.g, (int)row0 + lane, lane, wave, W, H, D, ptab, pbox);
  } else {
    *(unsigned*)(smem + L::zero + lane * 4) = 0u;
  }
  __syncthreads();
  // ---- 1b. wave 0: aligned power-of-two runs whose box fits -------------------------------------------------------------
  if (wave == 0) box_cut_runs<kAdjRows, INT_MAX>(pbox, lane, runs);
  __syncthreads();

  const typename P::Elem* __restrict__ dx = (const typename P::Elem*)sp.dx;
  const int q = lane >> 4, col = lane & 15;                    // MFMA lane roles: point of the K-step / box row of the tile
  const int tr_r = (lane >> 2) & 3, tr_p = lane & 3;           // transposed read: slot within the 4-slot block, 4-channel group
  // byte offset of channel tile t in a staged row, as this lane reads it: tile t = channels 32 (t >> 1) + 8 p + 4 (t & 1)
  // + 0..3 for group p (the forward's assignment: a lane's accumulators of tiles 2u, 2u + 1 are 8 consecutive channels);
  // physical position: 16-B chunk ^ (slot & 3) << 2, 8-B halfs swapped for odd points (q & 1: a K-step starts at an even
  // point) -- the 32 lanes of a transposed read (2 points x 4 slots x 4 channel groups) hit 32 distinct 8-B bank slots
  int aoff[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t)
    aoff[t] = ((tr_p << 4) + (((t >> 1) << 6) | ((t & 1) << 3))) ^ ((tr_r << 6) | ((q & 1) << 3));

  float inv_s = 0.f;
  if (!P::kScaleInFlush) inv_s = sp.scale[1];
  int first = 0;
#pragma unroll 1
  while (first < kAdjPts) {
    const RunBox rb = runs[first];
    const int count = uni(rb.count), rb_b = uni(rb.b);
    RunDims d = run_dims(uni(rb.lo), uni(rb.n));
    const int rows = d.rows;
    if (rows == 0) { first += count; continue; }                // no valid point in the run (uniform)
    d.set_inverses<false>();
    const int n_vt = (rows + 15) >> 4;                          // box-row tiles in use
    // this lane's box rows (tiles wave, wave + 4) as absolute voxel coordinates; a row beyond the box matches nothing
    int vx[2], vy[2], vz[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int v = 16 * (wave + 4 * i) + col;
      int ix, iy, iz;
      d.row_to_xyz(v, ix, iy, iz);
      const bool in = v < rows;
      vx[i] = in ? d.lox + ix : -4; vy[i] = in ? d.loy + iy : -4; vz[i] = in ? d.loz + iz : -4;
    }
    const bool own0 = wave < n_vt, own1 = wave + 4 < n_vt;      // (uniform)
    f32x4v acc[2][NT];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int t = 0; t < NT; ++t) acc[i][t] = (f32x4v){0.f, 0.f, 0.f, 0.f};

    // staging of chunk ci: rows (point, slot j < 7) x 16 pieces of 8 channels = 896 pieces, 3.5 per thread; physical
    // position chunk ^ (j & 3) << 2, 8-B halfs swapped for odd points.  The next chunk's pieces are requested a chunk ahead
    const int nchunks = (count + kAdjChunkPts - 1) / kAdjChunkPts;
    typename P::Piece sv[4];
    auto stage_load = [&](int ci) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int i = tid + 256 * e;
        const int r = i >> 4, chunk = i & 15;
        const int pl = r / LIST_N_STENCIL, j = r - pl * LIST_N_STENCIL;
        sv[e] = P::no_piece();
        if (i < kAdjStageRows * 16 && ci * kAdjChunkPts + pl < count)
          sv[e] = P::load_piece(dx + (row0 + first + ci * kAdjChunkPts + pl) * sp.g.Kp + col_off + j * kAdjC + chunk * 8);
      }
    };
    auto stage_store = [&](int ci) {
      char* buf = smem + L::stage + (ci & 1) * P::kBufBytes;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int i = tid + 256 * e;
        if (i >= kAdjStageRows * 16) continue;
        const int r = i >> 4, chunk = i & 15;
        const int pl = r / LIST_N_STENCIL, j = r - pl * LIST_N_STENCIL;
        P::store_piece(buf, r * RB + ((chunk ^ ((j & 3) << 2)) << 4), pl & 1, sv[e]);
      }
    };
    stage_load(0);
#pragma unroll 1
    for (int ci = 0; ci < nchunks; ++ci) {
      stage_store(ci);
      __syncthreads();                 // (one barrier per chunk: the other buffer was last read before the previous barrier)
      if (ci + 1 < nchunks) stage_load(ci + 1);
      const char* buf = smem + L::stage + (ci & 1) * P::kBufBytes;
      // (the MFMAs left out, staging and barriers only: 16^3 level 0.239 -> 0.125 ms, 8^3 0.118 -> 0.070)
#pragma unroll 1
      for (int ks = 0; ks < kAdjChunkPts / 4; ++ks) {
        const int plc = 4 * ks + q;                              // point of the chunk
        const int pl = ci * kAdjChunkPts + plc;                  // point of the run
        if (uni(ci * kAdjChunkPts + 4 * ks) >= count) break;     // (runs of 1, 2, 4 points: uniform)
        const bool live = pl < count;
        const int pt = first + (live ? pl : 0);
        // A: slots 0..3 and 4..7 of this lane's point; slot 7 and points beyond the run read the zero row
        const bool live_hi = live && tr_r < 3;
        const char* a_lo = live ? buf + (plc * LIST_N_STENCIL + tr_r) * RB : smem + L::zero;
        const char* a_hi = live_hi ? buf + (plc * LIST_N_STENCIL + 4 + tr_r) * RB : smem + L::zero;
        const typename P::AFrag a = P::a_frags(a_lo, a_hi, live, live_hi, aoff);
        // B: the 7 weights of (point, slot) at this lane's voxel, per owned tile (the factor of an axis is the record's
        // w0 where the voxel is the base tap, w1 where it is the next one, 0 elsewhere), split hi + lo in the operand's
        // 16-bit format
        const AxisW* rec = ptab + pt * 9;
        float hx[2][3], hy[2][3], hz[2][3];
#pragma unroll
        for (int v = 0; v < 3; ++v) {
          const AxisW fx = rec[v], fy = rec[3 + v], fz = rec[6 + v];
#pragma unroll
          for (int i = 0; i < 2; ++i) {
            const int dxv = vx[i] - fx.i0, dyv = vy[i] - fy.i0, dzv = vz[i] - fz.i0;
            hx[i][v] = dxv == 0 ? fx.w0 : (dxv == 1 ? fx.w1 : 0.f);
            hy[i][v] = dyv == 0 ? fy.w0 : (dyv == 1 ? fy.w1 : 0.f);
            hz[i][v] = dzv == 0 ? fz.w0 : (dzv == 1 ? fz.w1 : 0.f);
          }
        }
        uint4 bhi[2], blo[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          if (i == 0 ? !own0 : !own1) continue;
          const float cx = live ? hx[i][0] : 0.f;                  // (every slot's weight has a centre factor)
          const float yz = hy[i][0] * hz[i][0], xz = cx * hz[i][0], xy = cx * hy[i][0];
          const float w[8] = {cx * yz, hx[i][1] * yz, hx[i][2] * yz, hy[i][1] * xz, hy[i][2] * xz, hz[i][1] * xy, hz[i][2] * xy, 0.f};
          unsigned hi[4], lo[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            hi[e] = P::pk2(w[2 * e], w[2 * e + 1]);
            lo[e] = P::pk2(w[2 * e] - P::up((unsigned short)(hi[e] & 0xffffu)), w[2 * e + 1] - P::up((unsigned short)(hi[e] >> 16)));
          }
          bhi[i] = make_uint4(hi[0], hi[1], hi[2], hi[3]);
          blo[i] = make_uint4(lo[0], lo[1], lo[2], lo[3]);
        }
        P::mma(a, aoff, bhi, blo, own0, own1, acc);
      }
    }
    if (P::kScaleInFlush) inv_s = sp.scale[1];
    P::flush(smem, acc, d, rb_b, wave, lane, own0, own1, gv, inv_s, img16);
    first += count;
    if (first < kAdjPts) __syncthreads();                       // the next run stages over the buffers / the box
  }
}

// a window level (stencil shorter than a voxel) that scatter_box_eligible (vox_adjoint_plan.h) accepts; fp16 dX: the
// packed-half flush into img16, the level's zeroed fp16 image scaled by kWinPkScale (form ADJ_F16_PK), or, img16 null,
// the diagnostic fp32 flush into gv.data (ADJ_F16_F32); fp32 dX: ADJ_SPLIT
hipError_t launch_scatter_vox_box(const ScatterParams& sp, const ListVoxLevel& gv, int col_off, _Float16* img16,
                                  hipStream_t s) {
  const dim3 grid((unsigned)(sp.g.rows / kAdjPts));
  if (!sp.dx_f16) hipLaunchKernelGGL(k_scatter_vox_box<ADJ_SPLIT>, grid, dim3(256), 0, s, sp, gv, col_off, (_Float16*)nullptr);
  else if (img16) hipLaunchKernelGGL(k_scatter_vox_box<ADJ_F16_PK>, grid, dim3(256), 0, s, sp, gv, col_off, img16);
  else hipLaunchKernelGGL(k_scatter_vox_box<ADJ_F16_F32>, grid, dim3(256), 0, s, sp, gv, col_off, img16);
  return hipGetLastError();
}

}  // namespace list
