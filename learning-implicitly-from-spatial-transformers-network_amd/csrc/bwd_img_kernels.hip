// Backward of the 2-D gathers: dX [rows][Kp] (gradient of the feature matrix, gather order) ->
//   * gradient of the prepared 137^2 perceptual map   (adjoint of F.grid_sample 2-D, modules.py:46-52)
//   * gradient of trans_mat                           (through modules.py:37-45: matmul, divide, clamp)
//   * gradients of the five encoder maps              (adjoint of F.interpolate, modules.py:26-35)
//   * the pre-pooled form's [B][C][N] gradient and list_percep_pool_bwd's rows
// What query_bwd_plan.h plans (the voxel levels: bwd_scatter_kernels.hip).  For the perceptual map no atomics at all where
// the points are already in pixel order (forward's second sort): every map pixel GATHERS the contributions of the <= 4
// pixel cells around it and is written once.
#include <limits.h>
#include <string.h>

#include "list_common.h"
#include "point_math.h"

namespace list {

// ---- perceptual map ------------------------------------------------------------------------------------------
// Per-point record of the 2-D sample, in pixel order (slot -> point): everything the map gradient
// needs, so that the per-pixel gather reads 32 B per candidate instead of re-projecting.
struct ImgRec { int x0, y0; int row; int b; float wx0, wx1, wy0, wy1; };
static_assert(sizeof(ImgRec) == 32, "ImgRec is 32 bytes");

// the projection of network/modules.py:37-47 with the intermediate values the chain rule needs
struct ProjFull { float X, Y, den, u_raw, v_raw; int pass_u, pass_v; float ix, iy; int x0, y0; float wx0, wx1, wy0, wy1; };

__device__ __forceinline__ ProjFull project_full(const float* __restrict__ T, float px, float py, float pz,
                                                 int ms, float clamp_hi) {
  ProjFull r;
  float X = px * T[0], Y = px * T[1], Z = px * T[2];
  X = fmaf(py, T[3], X); Y = fmaf(py, T[4], Y); Z = fmaf(py, T[5], Z);
  X = fmaf(pz, T[6], X); Y = fmaf(pz, T[7], Y); Z = fmaf(pz, T[8], Z);
  X = X + T[9]; Y = Y + T[10]; Z = Z + T[11];
  r.X = X; r.Y = Y; r.den = Z + 1e-8f;
  r.u_raw = __fdiv_rn(X, r.den); r.v_raw = __fdiv_rn(Y, r.den);
  r.pass_u = (r.u_raw >= 0.f && r.u_raw <= clamp_hi) ? 1 : 0;     // torch.clamp backward mask
  r.pass_v = (r.v_raw >= 0.f && r.v_raw <= clamp_hi) ? 1 : 0;
  const float u = clamp_keep_nan(r.u_raw, clamp_hi), v = clamp_keep_nan(r.v_raw, clamp_hi);
  const float half = (float)(ms - 1) * 0.5f;
  const float gx = __fdiv_rn(u - half, half), gy = __fdiv_rn(v - half, half);
  r.ix = (gx + 1.f) * half; r.iy = (gy + 1.f) * half;
  const float fx = floorf(r.ix), fy = floorf(r.iy);
  r.wx1 = r.ix - fx; r.wx0 = (fx + 1.f) - r.ix;
  r.wy1 = r.iy - fy; r.wy0 = (fy + 1.f) - r.iy;
  r.x0 = min(max((int)fx, 0), ms - 1); r.y0 = min(max((int)fy, 0), ms - 1);
  return r;
}

__device__ __forceinline__ Pt load_point_raw(const GatherParams& g, int pt) {
  Pt p;
  p.valid = true;
  const int64_t gp = g.p_begin + pt;
  p.b = (int)(gp / g.N);
  const int n = (int)(gp - (int64_t)p.b * g.N);
  const float* q = g.query + (int64_t)p.b * g.q_sb + (int64_t)n * g.q_sn;
  p.x = q[(int64_t)g.perm0 * g.q_sc] * g.scale;
  p.y = q[(int64_t)g.perm1 * g.q_sc] * g.scale;
  p.z = q[(int64_t)g.perm2 * g.q_sc] * g.scale;
  return p;
}

// slot -> (point, X row): pixel order when the forward built one, else row order
__device__ __forceinline__ void slot_point(const GatherParams& g, int slot, int& pt, int& row) {
  if (g.order_img) { pt = g.order_img[slot]; row = g.row_of[pt]; }
  else { row = slot; pt = g.order ? g.order[slot] : slot; }
}

__global__ __launch_bounds__(256) void k_img_records(GatherParams g, const float* __restrict__ trans_mat, int ms,
                                                     float clamp_hi, ImgRec* __restrict__ recs) {
  const int slot = blockIdx.x * 256 + threadIdx.x;
  if (slot >= g.n_valid) return;
  int pt, row;
  slot_point(g, slot, pt, row);
  const Pt p = load_point_raw(g, pt);
  const ProjFull pr = project_full(trans_mat + p.b * 12, p.x, p.y, p.z, ms, clamp_hi);
  ImgRec r;
  r.x0 = pr.x0; r.y0 = pr.y0; r.row = row; r.b = p.b;
  r.wx0 = pr.wx0; r.wx1 = pr.wx1; r.wy0 = pr.wy0; r.wy1 = pr.wy1;
  // zeros padding, as in the forward (Proj::dead, point_math.h): under a clamp beyond the map (network/modules.py:43 with
  // map_size < 137) a tap outside the map gives no value, so it takes no gradient -- x0 / y0 are clamped INTO the map, and
  // their weights would otherwise land on its last column / row.  (A NaN weight stays NaN, as there.)
  const float fx = floorf(pr.ix), fy = floorf(pr.iy), last = (float)(ms - 1);
  if (!(fx >= 0.f && fx <= last) && r.wx0 == r.wx0) r.wx0 = 0.f;
  if (!(fx + 1.f <= last) && r.wx1 == r.wx1) r.wx1 = 0.f;
  if (!(fy >= 0.f && fy <= last) && r.wy0 == r.wy0) r.wy0 = 0.f;
  if (!(fy + 1.f <= last) && r.wy1 == r.wy1) r.wy1 = 0.f;
  recs[slot] = r;
}

// One workgroup per (image, map row Y, group of 4 map columns); thread t owns channels 4t .. 4t+3 (and
// +1024 ...).  Candidates = the points of the <= 4 pixel cells (rows Y-1, Y; column groups cx-1, cx)
// whose 2x2 footprint can reach the group; each contributes w(tap) * dX[row][img_off + c].
//
// Heavy groups (round 4).  Projections that pile onto the clamp of network/modules.py:43 -- an untrained spatial
// transformer puts ~90 % of the points there -- fill a handful of border cells with tens of thousands of candidates,
// which ONE workgroup then walked one after the other (measured: this stage 0.36 -> 2.58 ms at 98 % of the points on the
// clamp, the training step 6.7 -> 8.7 ms).  A group with more than kHeavyChunk candidates is therefore cut into chunks of
// kHeavyChunk: k_img_heavy_plan numbers the chunks (one scan over the groups), k_img_heavy_partial sums each chunk in its
// own workgroup into a partial row, and the group's own workgroup adds the partial rows in chunk order instead of
// walking the candidates (no atomics: as reproducible as before).
constexpr int kImgCand = 128;
constexpr int kHeavyChunk = 1024;

__device__ __forceinline__ void img_group_cells(const int* __restrict__ bins, int slot_img, int Y, int cx, int cw,
                                                int (&beg)[4], int (&end)[4]) {
  // candidate slot ranges of the 4 cells (bins hold END offsets after the forward's scatter pass)
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int yy = Y - 1 + (k >> 1), cc = cx - 1 + (k & 1);
    beg[k] = end[k] = 0;
    if (yy < 0 || cc < 0) continue;
    const int bin = slot_img * kSortPixCells + min(yy * cw + cc, kSortPixCells - 1);
    beg[k] = bin > 0 ? bins[bin - 1] : 0;
    end[k] = bins[bin];
  }
}

// candidates [s_begin, s_end) of the record array: acc[t][e] += w(tap of map column X0 + t, row Y) * dX[row][c + e]
template <int DXH>
__device__ __forceinline__ void img_accumulate(const ScatterParams& sp, const ImgRec* __restrict__ recs, ImgRec* cand,
                                               int s_begin, int s_end, int b, int Y, int X0, int qd, int nq,
                                               int img_off, float (&acc)[4][4]) {
  for (int s0 = s_begin; s0 < s_end; s0 += kImgCand) {
    const int n = min(kImgCand, s_end - s0);
    __syncthreads();
    if ((int)threadIdx.x < n) cand[threadIdx.x] = recs[s0 + threadIdx.x];
    __syncthreads();
    for (int i = 0; i < n; ++i) {
      const ImgRec r = cand[i];
      if (r.b != b) continue;                            // a clamped bin index may mix images: never, but cheap
      const float wy = (r.y0 == Y) ? r.wy0 : ((r.y0 + 1 == Y) ? r.wy1 : 0.f);
      if ((r.y0 != Y && r.y0 + 1 != Y) || r.x0 + 1 < X0 || r.x0 > X0 + 3) continue;
      if (qd >= nq) continue;
      float gv[4];
      const int64_t o = (int64_t)r.row * sp.g.Kp + img_off + qd * 4;
      if (DXH) {
        const uint2 h = *(const uint2*)((const unsigned short*)sp.dx + o);
        gv[0] = h2f((unsigned short)(h.x & 0xffff)); gv[1] = h2f((unsigned short)(h.x >> 16));
        gv[2] = h2f((unsigned short)(h.y & 0xffff)); gv[3] = h2f((unsigned short)(h.y >> 16));
      } else {
        const float4 f = *(const float4*)((const float*)sp.dx + o);
        gv[0] = f.x; gv[1] = f.y; gv[2] = f.z; gv[3] = f.w;
      }
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int X = X0 + t;
        const float wx = (r.x0 == X) ? r.wx0 : ((r.x0 + 1 == X) ? r.wx1 : 0.f);
        const float w = wx * wy;
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[t][e] = fmaf(w, gv[e], acc[t][e]);
      }
    }
  }
}

// chunk bookkeeping of the heavy groups (device memory in the backward workspace)
struct ImgHeavy {
  int* total;            // [1] chunks in use
  int* group_base;       // [groups] first chunk of a heavy group, -1: light
  int* chunk_group;      // [max_chunks]
  int* chunk_index;      // [max_chunks] index of the chunk inside its group
  float* partial;        // [max_chunks][4][Ct]
  int max_chunks;
};

// 1024 groups per workgroup: S_g = ceil(n_g / kHeavyChunk) for groups above kHeavyChunk candidates; a workgroup that
// holds such groups scans their S_g and takes a run of chunk slots from the global counter (*h.total, zeroed by the
// launcher; the runs need no particular order).  Without heavy groups -- the usual case -- it leaves after one barrier.
__global__ __launch_bounds__(1024) void k_img_heavy_plan(const int* __restrict__ bins, int b_first, int B, int ms,
                                                         ImgHeavy h) {
  __shared__ int part[1024];
  __shared__ int run_base;
  const int cw = (ms + 3) / 4;
  const int groups = B * ms * cw;
  const int g = blockIdx.x * 1024 + threadIdx.x;
  int S = 0;
  if (g < groups) {
    const int cx = g % cw, Y = (g / cw) % ms, b = g / (cw * ms);
    int beg[4], end[4];
    img_group_cells(bins, (b - b_first) % kSortImages, Y, cx, cw, beg, end);
    const int n = (end[0] - beg[0]) + (end[1] - beg[1]) + (end[2] - beg[2]) + (end[3] - beg[3]);
    S = n > kHeavyChunk ? (n + kHeavyChunk - 1) / kHeavyChunk : 0;
  }
  if (!__syncthreads_or(S > 0)) {
    if (g < groups) h.group_base[g] = -1;
    return;
  }
  part[threadIdx.x] = S;
  __syncthreads();
  for (int off = 1; off < 1024; off <<= 1) {
    const int v = (int)threadIdx.x >= off ? part[threadIdx.x - off] : 0;
    __syncthreads();
    part[threadIdx.x] += v;
    __syncthreads();
  }
  if (threadIdx.x == 1023) run_base = atomicAdd(h.total, part[1023]);
  __syncthreads();
  if (g >= groups) return;
  const int base = run_base + part[threadIdx.x] - S;
  const bool fits = S > 0 && base + S <= h.max_chunks;         // (the layout's bound holds all of them; belt and braces)
  h.group_base[g] = fits ? base : -1;
  // (every slot below min(*total, max_chunks) names a valid group, fitting or not: the partial kernel reads group_base)
  for (int i = 0; i < S && base + i < h.max_chunks; ++i) { h.chunk_group[base + i] = g; h.chunk_index[base + i] = i; }
}

// one workgroup per chunk slot: the partial sums of candidates [ci * kHeavyChunk, (ci + 1) * kHeavyChunk) of the group's
// four cells taken as one list
template <int DXH>
__global__ __launch_bounds__(256) void k_img_heavy_partial(ScatterParams sp, const ImgRec* __restrict__ recs,
                                                           const int* __restrict__ bins, int b_first, int ms, int Ct,
                                                           int img_off, ImgHeavy h) {
  __shared__ ImgRec cand[kImgCand];
  const int slot = blockIdx.x;
  if (slot >= min(*h.total, h.max_chunks)) return;
  const int g = h.chunk_group[slot], ci = h.chunk_index[slot];
  if (h.group_base[g] < 0) return;                               // (a run that did not fit: its group walks its candidates)
  const int cw = (ms + 3) / 4;
  const int cx = g % cw, Y = (g / cw) % ms, b = g / (cw * ms);
  int beg[4], end[4];
  img_group_cells(bins, (b - b_first) % kSortImages, Y, cx, cw, beg, end);
  const int nq = Ct / 4;
  const int lo = ci * kHeavyChunk, hi = lo + kHeavyChunk;           // positions in the concatenated candidate list
  for (int q0 = 0; q0 < nq; q0 += 256) {
    const int qd = q0 + threadIdx.x;
    float acc[4][4];
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[t][e] = 0.f;
    int pos = 0;
    for (int k = 0; k < 4; ++k) {
      const int len = end[k] - beg[k];
      const int a0 = max(lo - pos, 0), a1 = min(hi - pos, len);
      if (a0 < a1) img_accumulate<DXH>(sp, recs, cand, beg[k] + a0, beg[k] + a1, b, Y, 4 * cx, qd, nq, img_off, acc);
      pos += len;
    }
    if (qd < nq) {
#pragma unroll
      for (int t = 0; t < 4; ++t)
        *(float4*)(h.partial + ((int64_t)slot * 4 + t) * Ct + qd * 4) = make_float4(acc[t][0], acc[t][1], acc[t][2], acc[t][3]);
    }
  }
}

// GH (fp16 operands only): the map gradient is the intermediate of the adjoint resize in the same call -- written as
// halfs AT the gradient scale s (the sums of a pixel's <= 4 cells of s * dX values: saturating conversion), and
// k_img_grad_level<1> multiplies by 1 / s at its end
template <int DXH, int GH = 0>
__global__ __launch_bounds__(256) void k_img_grad_gather(ScatterParams sp, const ImgRec* __restrict__ recs,
                                                         const int* __restrict__ bins, int b_first, int ms,
                                                         int Ct, int img_off, float* __restrict__ out, ImgHeavy h) {
  __shared__ ImgRec cand[kImgCand];
  const int cw = (ms + 3) / 4;
  const int cx = blockIdx.x % cw;
  const int Y = (blockIdx.x / cw) % ms;
  const int b = blockIdx.x / (cw * ms);
  const int slot_img = (b - b_first) % kSortImages;
  const int X0 = 4 * cx;
  const float inv_s = sp.scale[1];
  const int nq = Ct / 4;                                   // channel quads

  int beg[4], end[4];
  img_group_cells(bins, slot_img, Y, cx, cw, beg, end);
  const int hbase = h.group_base ? h.group_base[blockIdx.x] : -1;
  const int n_all = (end[0] - beg[0]) + (end[1] - beg[1]) + (end[2] - beg[2]) + (end[3] - beg[3]);
  float acc[4][4];
  for (int q0 = 0; q0 < nq; q0 += 256) {
    const int qd = q0 + threadIdx.x;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[t][e] = 0.f;
    if (hbase >= 0) {
      // heavy group: its chunks were summed by k_img_heavy_partial; add the partial rows in chunk order
      const int S = (n_all + kHeavyChunk - 1) / kHeavyChunk;
      if (qd < nq)
        for (int i = 0; i < S; ++i)
#pragma unroll
          for (int t = 0; t < 4; ++t) {
            const float4 v = *(const float4*)(h.partial + ((int64_t)(hbase + i) * 4 + t) * Ct + qd * 4);
            acc[t][0] += v.x; acc[t][1] += v.y; acc[t][2] += v.z; acc[t][3] += v.w;
          }
    } else {
      for (int k = 0; k < 4; ++k)
        img_accumulate<DXH>(sp, recs, cand, beg[k], end[k], b, Y, X0, qd, nq, img_off, acc);
    }
    if (qd < nq) {
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int X = X0 + t;
        if (X >= ms) continue;
        const int64_t o = ((int64_t)(b * ms + Y) * ms + X) * Ct + qd * 4;
        if (GH) {
          *(uint2*)((unsigned short*)out + o) = half4(make_float4(acc[t][0], acc[t][1], acc[t][2], acc[t][3]));
        } else {
          float4 v = make_float4(acc[t][0] * inv_s, acc[t][1] * inv_s, acc[t][2] * inv_s, acc[t][3] * inv_s);
          *(float4*)(out + o) = v;
        }
      }
    }
  }
}

// Fallback without a pixel order (maps wider than the sort's bins, or no_sort): atomics, lanes over channels.
template <int DXH>
__global__ __launch_bounds__(256) void k_img_grad_atomic(ScatterParams sp, const ImgRec* __restrict__ recs, int ms,
                                                         int Ct, int img_off, float* __restrict__ out) {
  const int slot0 = blockIdx.x * kGatherRows;
  const float inv_s = sp.scale[1];
  for (int i = 0; i < kGatherRows; ++i) {
    const int slot = slot0 + i;
    if (slot >= sp.g.n_valid) return;
    const ImgRec r = recs[slot];
    const int x1 = min(r.x0 + 1, ms - 1), y1 = min(r.y0 + 1, ms - 1);
    float* base = out + (int64_t)r.b * ms * ms * Ct;
    float* p00 = base + (int64_t)(r.y0 * ms + r.x0) * Ct; float* p01 = base + (int64_t)(r.y0 * ms + x1) * Ct;
    float* p10 = base + (int64_t)(y1 * ms + r.x0) * Ct;   float* p11 = base + (int64_t)(y1 * ms + x1) * Ct;
    for (int c = threadIdx.x; c < Ct; c += 256) {
      const float gval = dx_at<DXH>(sp.dx, (int64_t)r.row * sp.g.Kp + img_off + c) * inv_s;
      atomicAdd(p00 + c, r.wx0 * r.wy0 * gval); atomicAdd(p01 + c, r.wx1 * r.wy0 * gval);
      atomicAdd(p10 + c, r.wx0 * r.wy1 * gval); atomicAdd(p11 + c, r.wx1 * r.wy1 * gval);
    }
  }
}

// ---- trans_mat ------------------------------------------------------------------------------------------------
// d(feature_c)/d(ix) = wy0 (m01 - m00) + wy1 (m11 - m10), d/d(iy) = wx0 (m10 - m00) + wx1 (m11 - m01)
// (grid_sampler_2d_backward; a tap outside the map counts as zero); then ix = (gx+1)*half, gx = (u-half)/half,
// u = clamp(X/den), den = Z + 1e-8, [X Y Z] = [p 1] . T.
template <int F16>
__device__ __forceinline__ float map_at(const void* __restrict__ m, int64_t i) {
  return F16 ? h2f(((const unsigned short*)m)[i]) : ((const float*)m)[i];
}

struct TransPt { int64_t o00; int sx, sy; int row, b, valid; float wx0, wx1, wy0, wy1; float X, Y, den; int pass_u, pass_v;
                 float px, py, pz; };

// grid = rows/64, block = 256: the first 64 threads project the workgroup's points (pixel order), then
// the workgroup walks them with lanes over channel octets (16-B loads of the four taps and of dX), a
// whole number of points per pass; wave shuffles + LDS reduce the two coordinate derivatives per point.
template <int F16, int DXH>
__global__ __launch_bounds__(256) void k_trans_grad(ScatterParams sp, const void* __restrict__ img_map,
                                                    const float* __restrict__ trans_mat, int ms, int Ct,
                                                    float clamp_hi, int img_off, float* __restrict__ grad_T) {
  __shared__ TransPt tp[kGatherRows];
  __shared__ float s_gx[kGatherRows][8], s_gy[kGatherRows][8];     // per point: <= 4 waves x 2 halves of partials
  const int blk = xcd_contiguous_block(blockIdx.x, gridDim.x);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t img_stride = (int64_t)ms * ms * Ct;
  if (threadIdx.x < kGatherRows) {
    TransPt t;
    const int slot = blk * kGatherRows + threadIdx.x;
    t.valid = slot < sp.g.n_valid ? 1 : 0;
    int pt = 0, row = 0;
    if (t.valid) slot_point(sp.g, slot, pt, row);
    const Pt p = load_point_raw(sp.g, pt);
    const ProjFull pr = project_full(trans_mat + p.b * 12, p.x, p.y, p.z, ms, clamp_hi);
    t.o00 = p.b * img_stride + (int64_t)(pr.y0 * ms + pr.x0) * Ct;
    t.sx = pr.x0 + 1 < ms ? Ct : -1;                       // -1: the tap lies outside the map (counts as zero)
    t.sy = pr.y0 + 1 < ms ? ms * Ct : -1;
    t.row = row; t.b = p.b;
    t.wx0 = pr.wx0; t.wx1 = pr.wx1; t.wy0 = pr.wy0; t.wy1 = pr.wy1;
    t.X = pr.X; t.Y = pr.Y; t.den = pr.den; t.pass_u = pr.pass_u; t.pass_v = pr.pass_v;
    t.px = p.x; t.py = p.y; t.pz = p.z;
    tp[threadIdx.x] = t;
#pragma unroll
    for (int w = 0; w < 8; ++w) { s_gx[threadIdx.x][w] = 0.f; s_gy[threadIdx.x][w] = 0.f; }
  }
  __syncthreads();
  const int lq = Ct / 8;                                   // lanes that cover one point
  if (Ct % 8 == 0 && img_off % 8 == 0 && lq >= 4 && lq <= 256 && 256 % lq == 0) {
    const int ppp = 256 / lq;                              // points per pass
    const int pp = threadIdx.x / lq, q = threadIdx.x - pp * lq;
    for (int i = 0; i < kGatherRows; i += ppp) {
      const TransPt& t = tp[i + pp];
      float gx = 0.f, gy = 0.f;
      if (t.valid) {
        float g[8], m00[8], m01[8], m10[8], m11[8];
        load8<DXH>(sp.dx, (int64_t)t.row * sp.g.Kp + img_off + q * 8, g);
        const int64_t o = t.o00 + q * 8;
        load8<F16>(img_map, o, m00);
        load8<F16>(img_map, o + (t.sx > 0 ? t.sx : 0), m01);
        load8<F16>(img_map, o + (t.sy > 0 ? t.sy : 0), m10);
        load8<F16>(img_map, o + (t.sx > 0 ? t.sx : 0) + (t.sy > 0 ? t.sy : 0), m11);
        const float kx = t.sx > 0 ? 1.f : 0.f, ky = t.sy > 0 ? 1.f : 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float a01 = m01[e] * kx, a10 = m10[e] * ky, a11 = m11[e] * kx * ky;
          gx = fmaf(g[e], t.wy0 * (a01 - m00[e]) + t.wy1 * (a11 - a10), gx);
          gy = fmaf(g[e], t.wx0 * (a10 - m00[e]) + t.wx1 * (a11 - a01), gy);
        }
      }
      // lanes of one point sit in whole waves (lq >= 64) or in aligned sub-wave groups (lq < 64).  Whole waves: the two
      // 32-lane halves keep partials of their own (row-level DPP adds only) -- with the halves combined by __shfl_xor(.,
      // 32), a ds_bpermute_b32 behind this loop's loads, ONE point's gy came out different in up to 59 of 60 forked calls
      // whenever the wave shared its CU with the weight-gradient GEMM (ds_read_b64_tr_b16 + LDS-DMA); without that one
      // instruction pair: 0 of 240 (profiles/r04b_trans_mat_interference.txt)
      if (lq >= 64) {
        for (int off = 16; off > 0; off >>= 1) { gx += __shfl_xor(gx, off); gy += __shfl_xor(gy, off); }
        if ((lane & 31) == 0) {
          const int slot = 2 * (wave % (lq / 64)) + (lane >> 5);
          s_gx[i + pp][slot] = gx; s_gy[i + pp][slot] = gy;
        }
      } else {
        for (int off = lq >> 1; off > 0; off >>= 1) { gx += __shfl_xor(gx, off); gy += __shfl_xor(gy, off); }
        if ((lane & (lq - 1)) == 0) { s_gx[i + pp][0] = gx; s_gy[i + pp][0] = gy; }
      }
    }
  } else {
    // unusual channel counts: one wave per point, scalar channels
    for (int i = wave; i < kGatherRows; i += 4) {
      const TransPt& t = tp[i];
      float gx = 0.f, gy = 0.f;
      if (t.valid)
        for (int c = lane; c < Ct; c += 64) {
          const float g = dx_at<DXH>(sp.dx, (int64_t)t.row * sp.g.Kp + img_off + c);
          const float m00 = map_at<F16>(img_map, t.o00 + c);
          const float m01 = t.sx > 0 ? map_at<F16>(img_map, t.o00 + t.sx + c) : 0.f;
          const float m10 = t.sy > 0 ? map_at<F16>(img_map, t.o00 + t.sy + c) : 0.f;
          const float m11 = (t.sx > 0 && t.sy > 0) ? map_at<F16>(img_map, t.o00 + t.sx + t.sy + c) : 0.f;
          gx = fmaf(g, t.wy0 * (m01 - m00) + t.wy1 * (m11 - m10), gx);
          gy = fmaf(g, t.wx0 * (m10 - m00) + t.wx1 * (m11 - m01), gy);
        }
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) { gx += __shfl_xor(gx, off); gy += __shfl_xor(gy, off); }
      if (lane == 0) { s_gx[i][0] = gx; s_gy[i][0] = gy; }
    }
  }
  __syncthreads();
  if (threadIdx.x >= kGatherRows) return;
  // chain rule per point, then one reduction per image present in the workgroup
  float d[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) d[k] = 0.f;
  const TransPt t = tp[threadIdx.x];
  const int b = t.valid ? t.b : -1;
  if (t.valid) {
    const float* px_ = s_gx[threadIdx.x];
    const float* py_ = s_gy[threadIdx.x];
    const float gix = ((px_[0] + px_[1]) + (px_[2] + px_[3])) + ((px_[4] + px_[5]) + (px_[6] + px_[7]));
    const float giy = ((py_[0] + py_[1]) + (py_[2] + py_[3])) + ((py_[4] + py_[5]) + (py_[6] + py_[7]));
    const float half = (float)(ms - 1) * 0.5f;
    const float inv_s = sp.scale[1];
    // d/d(gx) = half * d/d(ix)  (grid_sampler unnormalize);  d/du = (1/half) * d/d(gx)
    const float du = t.pass_u ? __fdiv_rn(gix * half, half) * inv_s : 0.f;
    const float dv = t.pass_v ? __fdiv_rn(giy * half, half) * inv_s : 0.f;
    if (du != 0.f || dv != 0.f) {           // (clamped projections contribute exactly nothing, also when den == 0)
      const float dX = __fdiv_rn(du, t.den), dY = __fdiv_rn(dv, t.den);
      const float dZ = -(__fdiv_rn(du * t.X, t.den * t.den) + __fdiv_rn(dv * t.Y, t.den * t.den));
      const float h[4] = {t.px, t.py, t.pz, 1.f};
#pragma unroll
      for (int k = 0; k < 4; ++k) { d[3 * k] = h[k] * dX; d[3 * k + 1] = h[k] * dY; d[3 * k + 2] = h[k] * dZ; }
    }
  }
  // threads 0..63 are wave 0: reduce per image with shuffles
  int bmin = b < 0 ? INT_MAX : b, bmax = b;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    bmin = min(bmin, __shfl_xor(bmin, off));
    bmax = max(bmax, __shfl_xor(bmax, off));
  }
  for (int bi = bmin; bi <= bmax && bmax >= 0; ++bi) {
#pragma unroll
    for (int k = 0; k < 12; ++k) {
      float v = (b == bi) ? d[k] : 0.f;
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
      if (threadIdx.x == 0 && v != 0.f) atomicAdd(grad_T + bi * 12 + k, v);
    }
  }
}

// executes the map gradient of plan_query_bwd (query_bwd_plan.h: the form, the heavy groups, the map's element type -- nothing is
// decided here).  bins_pix: the forward's pixel bins (MAPGRAD_GATHER); heavy: img_heavy_bytes() of scratch (plan.heavy), carved
// [total | group_base | chunk_group | chunk_index | partial rows]
hipError_t launch_img_map_grad(const QueryBwdPlan& plan, const ScatterParams& sp, const FeatLayout& L, const ListQueryArgs& a,
                               int B, const int* bins_pix, void* recs, float* grad_img_map, void* heavy, hipStream_t s) {
  if (plan.map == MAPGRAD_NONE) return hipSuccess;
  if (plan.map == MAPGRAD_INVALID) return hipErrorInvalidValue;
  const int ms = a.map_size, Ct = L.img_C;
  ImgRec* rc = (ImgRec*)recs;
  hipLaunchKernelGGL(k_img_records, dim3((unsigned)((sp.g.n_valid + 255) / 256)), dim3(256), 0, s, sp.g,
                     a.trans_mat, ms, a.clamp_hi, rc);
  if (plan.map == MAPGRAD_ATOMIC) {
    hipError_t e = hipMemsetAsync(grad_img_map, 0, (size_t)B * ms * ms * Ct * sizeof(float), s);
    if (e != hipSuccess) return e;
    auto kernel = sp.dx_f16 ? k_img_grad_atomic<1> : k_img_grad_atomic<0>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)((sp.g.n_valid + kGatherRows - 1) / kGatherRows)), dim3(256), 0, s, sp, rc, ms, Ct,
                       L.img_off, grad_img_map);
    return hipGetLastError();
  }
  const dim3 grid((unsigned)(B * ms * ((ms + 3) / 4)));
  const int b_first = (int)(sp.g.p_begin / sp.g.N);
  ImgHeavy h;
  memset(&h, 0, sizeof(h));
  if (plan.heavy) {
    char* hb = (char*)heavy;
    h.max_chunks = img_heavy_max_chunks(sp.g.rows);
    h.total = (int*)hb; hb += 256;
    h.group_base = (int*)hb; hb += (size_t)kSortImages * kSortPixCells * 4;
    h.chunk_group = (int*)hb; hb += (size_t)h.max_chunks * 4;
    h.chunk_index = (int*)hb; hb += (size_t)h.max_chunks * 4;
    hb = (char*)(((uintptr_t)hb + 255) & ~(uintptr_t)255);
    h.partial = (float*)hb;
    hipError_t ez = hipMemsetAsync(h.total, 0, sizeof(int), s);
    if (ez != hipSuccess) return ez;
    hipLaunchKernelGGL(k_img_heavy_plan, dim3((grid.x + 1023) / 1024), dim3(1024), 0, s, bins_pix, b_first, B, ms, h);
    auto partial = sp.dx_f16 ? k_img_heavy_partial<1> : k_img_heavy_partial<0>;
    hipLaunchKernelGGL(partial, dim3((unsigned)h.max_chunks), dim3(256), 0, s, sp, rc, bins_pix, b_first, ms, Ct, L.img_off, h);
  }
  auto kernel = plan.map_f16 ? k_img_grad_gather<1, 1> : sp.dx_f16 ? k_img_grad_gather<1> : k_img_grad_gather<0>;
  hipLaunchKernelGGL(kernel, grid, dim3(256), 0, s, sp, rc, bins_pix, b_first, ms, Ct, L.img_off, grad_img_map, h);
  return hipGetLastError();
}

hipError_t launch_trans_grad(const ScatterParams& sp, const FeatLayout& L, const ListQueryArgs& a, int B,
                             float* grad_trans_mat, hipStream_t s) {
  hipError_t e = hipMemsetAsync(grad_trans_mat, 0, (size_t)B * 12 * sizeof(float), s);
  if (e != hipSuccess) return e;
  const bool f16 = a.img_dtype == LIST_MAP_F16;
  auto kernel = f16 ? (sp.dx_f16 ? k_trans_grad<1, 1> : k_trans_grad<1, 0>) : (sp.dx_f16 ? k_trans_grad<0, 1> : k_trans_grad<0, 0>);
  hipLaunchKernelGGL(kernel, dim3((unsigned)(sp.g.rows / kGatherRows)), dim3(256), 0, s, sp, a.img_map, a.trans_mat, a.map_size,
                     L.img_C, a.clamp_hi, L.img_off, grad_trans_mat);
  return hipGetLastError();
}

// ---- adjoint of the resize (list_prep_img_maps) ----------------------------------------------------------
// out[b][c][ys][xs] = sum over map pixels (oy, ox) whose bilinear footprint contains (ys, xs) of
// wy * wx * G[b][oy][ox][coff + c], with the forward's own index/weight arithmetic (prep_kernels.hip).
// One workgroup per (image, source row ys, 64 channels), separable:
//   1. R[ox][c] = sum_oy wy(oy, ys) G[b][oy][ox][c]   threads = (4 channels, 16 x lanes), 16-B loads that
//      run 256 B along the channels; every thread keeps its <= 20 columns in registers;
//   2. out[c][xs] = sum_ox wx(ox, xs) R[ox][c]          R through LDS, per-xs tap lists in CSR form;
//   3. the [64][W] tile turns through LDS so the NCHW writes run along x.
constexpr int kAdjMaxMs = 320;             // largest supported map_size
constexpr int kAdjCg = 32;                 // channels per workgroup (A/B: 64 = 72 KB of LDS, two workgroups per CU)
constexpr int kAdjXl = 256 / (kAdjCg / 4); // x lanes of phase 1 (a lane owns 4 channels)
constexpr int kAdjCols = (kAdjMaxMs + kAdjXl - 1) / kAdjXl;

// the forward's footprint of map index o on a source axis of S pixels
__device__ __forceinline__ void adj_footprint(int o, int S, int ms, int& i0, int& i1, float& w0, float& w1) {
  const float sc = ms > 1 ? (float)(S - 1) / (float)(ms - 1) : 0.f;
  const float f = sc * (float)o;
  i0 = min((int)f, S - 1);
  i1 = i0 + (i0 < S - 1 ? 1 : 0);
  w1 = f - (float)i0;
  w0 = 1.f - w1;
}

constexpr int kAdjTileW = 128;             // source columns per pass of phases 2-3

// All levels in ONE launch: a level's workgroups are few (896 - 1792) and each is a chain of dependent steps (tap
// lists, the row loop, two LDS phases), so five launches in a row cost ~0.11 ms each whatever their bytes; side by
// side the small levels fill the gaps of the large ones.
struct AdjLevels { ListMap2D m[LIST_N_IMG_LEVELS]; int coff[LIST_N_IMG_LEVELS], maxper[LIST_N_IMG_LEVELS],
                   wg_begin[LIST_N_IMG_LEVELS], n; };

// GH: G holds halfs at the gradient scale (k_img_grad_gather<1, 1>); out = (1 / s) * adjoint
template <int GH>
__global__ __launch_bounds__(256) void k_img_grad_level(const float* __restrict__ G, int ms, int Ct, AdjLevels lv,
                                                        const float* __restrict__ scale) {
  int l = 0;
#pragma unroll
  for (int i = 1; i < LIST_N_IMG_LEVELS; ++i)
    if (i < lv.n && (int)blockIdx.x >= lv.wg_begin[i]) l = i;
  const ListMap2D m = lv.m[l];
  const int coff = lv.coff[l], maxper = lv.maxper[l];
  const int cgroups = (m.C + kAdjCg - 1) / kAdjCg;
  const int widx = (int)blockIdx.x - lv.wg_begin[l];
  const int bx = widx / cgroups, by = widx - bx * cgroups;      // (image, source row) and 64-channel group
  extern __shared__ __attribute__((aligned(16))) float dyn[];
  // dynamic LDS: R[ms][kAdjCg] | tile[kAdjCg][kAdjTileW + 1] | wy[ms] | wx[W][maxper] | ox_first[W] | ox_cnt[W]
  float* R = dyn;
  float* tile = R + ms * kAdjCg;
  float* s_wy = tile + kAdjCg * (kAdjTileW + 1);
  float* s_wx = s_wy + ms;
  int* ox_first = (int*)(s_wx + m.W * maxper);
  int* ox_cnt = ox_first + m.W;
  __shared__ int oy_range[2];
  const int ys = bx % m.H;
  const int b = bx / m.H;
  const int c0 = by * kAdjCg;
  if (threadIdx.x == 0) { oy_range[0] = INT_MAX; oy_range[1] = INT_MIN; }
  __syncthreads();
  // map rows that touch source row ys: footprints are monotone, so they form one contiguous range
  for (int o = threadIdx.x; o < ms; o += 256) {
    int i0, i1; float w0, w1;
    adj_footprint(o, m.H, ms, i0, i1, w0, w1);
    const bool hit = i0 == ys || i1 == ys;
    s_wy[o] = hit ? (i0 == ys ? w0 : 0.f) + (i1 == ys ? w1 : 0.f) : 0.f;
    if (hit) { atomicMin(&oy_range[0], o); atomicMax(&oy_range[1], o); }
  }
  // map columns that touch source column xs: first column, count, weights
  const float scx = ms > 1 ? (float)(m.W - 1) / (float)(ms - 1) : 0.f;
  for (int xs = threadIdx.x; xs < m.W; xs += 256) {
    int o = 0;
    if (scx > 0.f) o = max(0, (int)floorf((float)(xs - 1) / scx) - 2);
    int i0, i1; float w0, w1;
    for (; o < ms; ++o) {                                  // skip columns that end before xs
      adj_footprint(o, m.W, ms, i0, i1, w0, w1);
      if (i1 >= xs) break;
    }
    ox_first[xs] = o;
    int n = 0;
    for (; o < ms && n < maxper; ++o, ++n) {
      adj_footprint(o, m.W, ms, i0, i1, w0, w1);
      if (i0 > xs) break;
      s_wx[xs * maxper + n] = (i0 == xs ? w0 : 0.f) + (i1 == xs ? w1 : 0.f);
    }
    ox_cnt[xs] = n;
  }
  __syncthreads();
  // ---- phase 1
  const int cq = threadIdx.x % (kAdjCg / 4), xl = threadIdx.x / (kAdjCg / 4);
  const int nc4 = min(kAdjCg, m.C - c0) / 4;               // channel quads that exist (C % 4 == 0)
  float4 acc[kAdjCols];
#pragma unroll
  for (int k = 0; k < kAdjCols; ++k) acc[k] = make_float4(0.f, 0.f, 0.f, 0.f);
  if (cq < nc4) {
    const int oy1 = oy_range[1];
    for (int oy = oy_range[0]; oy <= oy1; ++oy) {
      const float wy = s_wy[oy];
      const int64_t go = ((int64_t)(b * ms + oy) * ms) * Ct + coff + c0 + cq * 4;
#pragma unroll
      for (int k = 0; k < kAdjCols; ++k) {
        const int ox = xl + kAdjXl * k;
        if (ox < ms) {
          float4 v;
          if (GH) {
            const uint2 h = *(const uint2*)((const unsigned short*)G + go + (int64_t)ox * Ct);
            v = make_float4(h2f((unsigned short)(h.x & 0xffff)), h2f((unsigned short)(h.x >> 16)),
                            h2f((unsigned short)(h.y & 0xffff)), h2f((unsigned short)(h.y >> 16)));
          } else {
            v = *(const float4*)(G + go + (int64_t)ox * Ct);
          }
          acc[k].x = fmaf(wy, v.x, acc[k].x); acc[k].y = fmaf(wy, v.y, acc[k].y);
          acc[k].z = fmaf(wy, v.z, acc[k].z); acc[k].w = fmaf(wy, v.w, acc[k].w);
        }
      }
    }
  }
#pragma unroll
  for (int k = 0; k < kAdjCols; ++k) {
    const int ox = xl + kAdjXl * k;
    if (ox < ms) *(float4*)(R + ox * kAdjCg + cq * 4) = acc[k];
  }
  __syncthreads();
  // ---- phases 2 and 3, kAdjTileW source columns at a time
  const int c = threadIdx.x % kAdjCg, xq = threadIdx.x / kAdjCg;
  float* out = const_cast<float*>(m.data) + (int64_t)b * m.sb + (int64_t)ys * m.sh;
  for (int x0 = 0; x0 < m.W; x0 += kAdjTileW) {
    const int wt = min(kAdjTileW, m.W - x0);
    for (int xs = xq; xs < wt; xs += 256 / kAdjCg) {
      const int first = ox_first[x0 + xs], n = ox_cnt[x0 + xs];
      const float* wx = s_wx + (x0 + xs) * maxper;
      float a = 0.f;
      for (int e = 0; e < n; ++e) a = fmaf(wx[e], R[(first + e) * kAdjCg + c], a);
      tile[c * (kAdjTileW + 1) + xs] = GH ? a * scale[1] : a;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < kAdjCg * wt; i += 256) {
      const int cc = i / wt, xs = i - cc * wt;
      if (c0 + cc < m.C)
        out[(int64_t)(c0 + cc) * m.sc + (int64_t)(x0 + xs) * m.sw] = tile[cc * (kAdjTileW + 1) + xs];
    }
    __syncthreads();
  }
}

// ---- pre-pooled form: [B][C][N] <-> rows --------------------------------------------------------------------
// out[b][c][n] = (1/s) dX[row of point (b,n)][img_off + c]: the gradient of VoxelDecoder2.forward's third
// argument.  64 points x 64 channels per workgroup, turned through LDS so reads run along c, writes along n.
template <int DXH>
__global__ __launch_bounds__(256) void k_rows_to_grad(const void* __restrict__ dx, int Kp, int img_off,
                                                      const int* __restrict__ row_of, float* __restrict__ out,
                                                      int64_t sb, int64_t sc, int64_t sn, int N, int C,
                                                      const float* __restrict__ scale) {
  __shared__ float tile[64][65];
  const int nt = (N + 63) / 64;
  const int b = blockIdx.x / nt, n0 = (blockIdx.x % nt) * 64, c0 = blockIdx.y * 64;
  const int cl = threadIdx.x & 63, q = threadIdx.x >> 6;
  for (int i = q; i < 64; i += 4) {
    const int n = n0 + i;
    float v = 0.f;
    if (n < N && c0 + cl < C) {
      const int pt = b * N + n;
      const int row = row_of ? row_of[pt] : pt;
      v = dx_at<DXH>(dx, (int64_t)row * Kp + img_off + c0 + cl);
    }
    tile[i][cl] = v;
  }
  __syncthreads();
  const float inv_s = scale[1];
  for (int i = q; i < 64; i += 4) {
    const int c = c0 + i, n = n0 + cl;
    if (c < C && n < N) out[(int64_t)b * sb + (int64_t)c * sc + (int64_t)n * sn] = tile[cl][i] * inv_s;
  }
}

__global__ __launch_bounds__(256) void k_invert_order(const int* __restrict__ order, int n, int* __restrict__ row_of) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r < n) row_of[order[r]] = r;
}

hipError_t launch_rows_to_grad(const ScatterParams& sp, int img_off, int C, int B, int* row_of_scratch, float* out,
                               int64_t sb, int64_t sc, int64_t sn, hipStream_t s) {
  const int* row_of = nullptr;
  if (sp.g.order) {
    hipLaunchKernelGGL(k_invert_order, dim3((unsigned)((sp.g.n_valid + 255) / 256)), dim3(256), 0, s, sp.g.order,
                       sp.g.n_valid, row_of_scratch);
    row_of = row_of_scratch;
  }
  const dim3 grid((unsigned)(B * ((sp.g.N + 63) / 64)), (unsigned)((C + 63) / 64));
  auto kernel = sp.dx_f16 ? k_rows_to_grad<1> : k_rows_to_grad<0>;
  hipLaunchKernelGGL(kernel, grid, dim3(256), 0, s, sp.dx, sp.g.Kp, img_off, row_of, out, sb, sc, sn, sp.g.N, C, sp.scale);
  return hipGetLastError();
}

// dx[b*N + n][c] = src[b][c][n], rows beyond B*N zero; scale = {1, 1}
__global__ __launch_bounds__(256) void k_grad_to_rows(const float* __restrict__ src, int64_t sb, int64_t sc, int64_t sn,
                                                      int N, int C, float* __restrict__ dx) {
  __shared__ float tile[64][65];
  const int nt = (N + 63) / 64;
  const int b = blockIdx.x / nt, n0 = (blockIdx.x % nt) * 64, c0 = blockIdx.y * 64;
  const int l = threadIdx.x & 63, q = threadIdx.x >> 6;
  for (int i = q; i < 64; i += 4) {
    const int c = c0 + i, n = n0 + l;
    tile[i][l] = (c < C && n < N) ? src[(int64_t)b * sb + (int64_t)c * sc + (int64_t)n * sn] : 0.f;
  }
  __syncthreads();
  for (int i = q; i < 64; i += 4) {
    const int n = n0 + i, c = c0 + l;
    if (n < N && c < C) dx[((int64_t)b * N + n) * C + c] = tile[l][i];
  }
}

__global__ void k_unit_scale(float* scale) {
  if (threadIdx.x < 4) scale[threadIdx.x] = threadIdx.x < 2 ? 1.f : 0.f;
}

hipError_t launch_grad_to_rows(const float* src, int64_t sb, int64_t sc, int64_t sn, int B, int N, int C, float* dx,
                               float* scale, hipStream_t s) {
  const dim3 grid((unsigned)(B * ((N + 63) / 64)), (unsigned)((C + 63) / 64));
  hipLaunchKernelGGL(k_grad_to_rows, grid, dim3(256), 0, s, src, sb, sc, sn, N, C, dx);
  hipLaunchKernelGGL(k_unit_scale, dim3(1), dim3(64), 0, s, scale);
  return hipGetLastError();
}

hipError_t launch_img_grad_to_levels(const float* grad_img_map, int B, int map_size, int Ct,
                                     const ListMap2D grads[LIST_N_IMG_LEVELS], hipStream_t s, int map_f16,
                                     const float* scale) {
  if (map_size > kAdjMaxMs) return hipErrorInvalidValue;
  AdjLevels lv;
  lv.n = 0;
  int coff = 0;
  int64_t wgs = 0;
  size_t lds = 0;
  for (int i = 0; i < LIST_N_IMG_LEVELS; ++i) {
    const ListMap2D& m = grads[i];
    if (m.data) {
      if (m.C % 4 || coff % 4 || Ct % 4) return hipErrorInvalidValue;
      // map columns per source column: ~2 / scale when up-sampling, at most a few when down-sampling
      const float scx = map_size > 1 ? (float)(m.W - 1) / (float)(map_size - 1) : 0.f;
      int maxper = scx > 0.f ? (int)(2.f / scx) + 4 : map_size;
      if (maxper > map_size) maxper = map_size;
      const size_t need = sizeof(float) * ((size_t)map_size * kAdjCg + kAdjCg * (size_t)(kAdjTileW + 1) + (size_t)map_size +
                                           (size_t)m.W * maxper) + sizeof(int) * 2 * (size_t)m.W;
      if (need > 150 * 1024) return hipErrorInvalidValue;
      if (need > lds) lds = need;
      const int k = lv.n++;
      lv.m[k] = m; lv.coff[k] = coff; lv.maxper[k] = maxper; lv.wg_begin[k] = (int)wgs;
      wgs += (int64_t)B * m.H * ((m.C + kAdjCg - 1) / kAdjCg);
    }
    coff += m.C;
  }
  if (lv.n == 0) return hipSuccess;
  if (wgs >= 2147483647LL) return hipErrorInvalidValue;
  if (map_f16 && !scale) return hipErrorInvalidValue;
  auto kernel = map_f16 ? k_img_grad_level<1> : k_img_grad_level<0>;
  if (lds > 64 * 1024) {
    hipError_t e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(kernel, dim3((unsigned)wgs), dim3(256), lds, s, grad_img_map, map_size, Ct, lv, scale);
  return hipGetLastError();
}

}  // namespace list
