// Uniform-grid vertex clustering of an indexed triangle mesh on the device (include/list_simplify.h; the rule itself is
// csrc/simplify_math.h).
//
//   simp_key_kernel      one thread per vertex: its key (the sentinel `ncells` for an invalid vertex, which so sorts
//                        behind every cluster), val[v] = v, cluster_of[v] = -1, and the number of invalid vertices.
//   hipCUB sort          (key, vertex) by the bits of the key: a cluster's vertices become contiguous.
//   simp_head_kernel / hipCUB inclusive scan      run heads; the scan gives every sorted position its cluster number.
//   simp_sum_kernel      the per-cluster sums of q and the counts.  A wave takes kChunks * 64 consecutive sorted
//                        positions, 64 at a time: a segmented scan over the lanes adds up the runs, the run that
//                        reaches lane 63 is carried into the next step in registers.  A run that lies inside the
//                        wave's range is written with plain stores; only a run that crosses the range's first or last
//                        position is added with 64-bit integer atomicAdd, one add per wave and axis: the whole mesh in
//                        one cell is V / 512 adds on each of its four words.
//   simp_face_kernel     classify the faces, mark the clusters that kept faces use with plain stores of 1.
//   two hipCUB exclusive scans                    output vertex of a used cluster, output row of a kept face.
//   simp_map_kernel      vertex_map and the totals.
//   simp_emit_verts_kernel / simp_emit_faces_kernel
//
// The sums are integers, so no order of additions changes them; there is no float atomic, and nothing here waits for
// another thread: the kernel boundaries are the only synchronisation.
#include <hip/hip_runtime.h>

#include "list_simplify.h"
#include "list_cub.h"
#include "list_host.h"
#include "simplify_math.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxBlocks = 2048;            // grid-stride above this many workgroups
constexpr int kChunks = 8;                  // 64-position steps of one wave of simp_sum_kernel
constexpr int64_t kWaveRange = (int64_t)kChunks * 64;

typedef unsigned long long u64;

struct Grid {
  int32_t R[3];
  double lo[3], inv[3], cell[3];
};

// counters in the workspace
enum { C_INVALID_VERTS = 0, C_INVALID_FACES = 1, C_DEGENERATE = 2, C_N = 4 };

__device__ __forceinline__ int wave_sum(int x) {
  for (int d = 32; d; d >>= 1) x += __shfl_xor(x, d);
  return x;
}

__global__ __launch_bounds__(kThreads) void simp_key_kernel(const float* __restrict__ verts, int64_t V, Grid g,
                                                             uint32_t sentinel, uint32_t* __restrict__ key,
                                                             int32_t* __restrict__ val, int32_t* __restrict__ cluster_of,
                                                             u64* __restrict__ counters) {
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  int bad = 0;
  for (int64_t v = (int64_t)blockIdx.x * kThreads + threadIdx.x; v < V; v += stride) {
    const float p[3] = {verts[3 * v], verts[3 * v + 1], verts[3 * v + 2]};
    uint32_t k = sentinel;
    if (simp_valid_vertex(p)) {
      int32_t i[3], q;
      for (int a = 0; a < 3; ++a) simp_axis(p[a], g.lo[a], g.inv[a], g.R[a], &i[a], &q);
      k = simp_key(i[0], i[1], i[2], g.R[1], g.R[2]);
    } else {
      ++bad;
    }
    key[v] = k;
    val[v] = (int32_t)v;
    cluster_of[v] = -1;
  }
  bad = wave_sum(bad);                      // every lane of the wave is here: the loop has ended for all of them
  if (bad && (threadIdx.x & 63) == 0) atomicAdd(counters + C_INVALID_VERTS, (u64)bad);
}

__global__ __launch_bounds__(kThreads) void simp_head_kernel(const uint32_t* __restrict__ skey, int64_t V,
                                                              uint32_t sentinel, int32_t* __restrict__ head) {
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  for (int64_t j = (int64_t)blockIdx.x * kThreads + threadIdx.x; j < V; j += stride) {
    const uint32_t k = skey[j];
    head[j] = k != sentinel && (j == 0 || skey[j - 1] != k);
  }
}

// One run's sums and count to its cluster: plain stores when no other wave holds a piece of the run
__device__ __forceinline__ void flush(int cid, long long s0, long long s1, long long s2, int n, bool shared,
                                      u64* __restrict__ sums, int32_t* __restrict__ cnt) {
  u64* s = sums + 3 * (size_t)cid;
  if (shared) {
    atomicAdd(s, (u64)s0);
    atomicAdd(s + 1, (u64)s1);
    atomicAdd(s + 2, (u64)s2);
    atomicAdd(cnt + cid, n);
  } else {
    s[0] = (u64)s0;
    s[1] = (u64)s1;
    s[2] = (u64)s2;
    cnt[cid] = n;
  }
}

// sums[] and cnt[] are zero on entry.  incl[j] - 1 is the cluster of sorted position j (for a key below the sentinel).
__global__ __launch_bounds__(kThreads) void simp_sum_kernel(const float* __restrict__ verts, int64_t V, Grid g,
                                                             uint32_t sentinel, const uint32_t* __restrict__ skey,
                                                             const int32_t* __restrict__ perm,
                                                             const int32_t* __restrict__ head,
                                                             const int32_t* __restrict__ incl,
                                                             int32_t* __restrict__ cluster_of, uint32_t* __restrict__ ckey,
                                                             u64* __restrict__ sums, int32_t* __restrict__ cnt) {
  const int lane = threadIdx.x & 63;
  const int64_t begin = ((int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6)) * kWaveRange;
  if (begin >= V) return;                                   // the whole wave
  const int64_t end = begin + kWaveRange < V ? begin + kWaveRange : V;
  // the cluster whose run began before this range, if there is one: other waves add to it too
  int first_cid = -1;
  if (skey[begin] != sentinel && !head[begin]) first_cid = incl[begin] - 1;
  int carry_cid = -1, cn = 0;                               // the run that reached the previous step's lane 63
  long long c0 = 0, c1 = 0, c2 = 0;
  for (int64_t base = begin; base < end; base += 64) {      // every lane of the wave takes every step
    const int64_t j = base + lane;
    int cid = -1, n = 0;
    long long s0 = 0, s1 = 0, s2 = 0;
    if (j < end) {
      const uint32_t k = skey[j];
      if (k != sentinel) {
        cid = incl[j] - 1;
        const int32_t v = perm[j];                          // a value of val[]: in [0, V)
        cluster_of[v] = cid;
        if (head[j]) ckey[cid] = k;
        int32_t i, q;
        simp_axis(verts[3 * (int64_t)v], g.lo[0], g.inv[0], g.R[0], &i, &q);
        s0 = q;
        simp_axis(verts[3 * (int64_t)v + 1], g.lo[1], g.inv[1], g.R[1], &i, &q);
        s1 = q;
        simp_axis(verts[3 * (int64_t)v + 2], g.lo[2], g.inv[2], g.R[2], &i, &q);
        s2 = q;
        n = 1;
      }
    }
    // inclusive scan inside the runs: the lanes of a run are neighbours, so lane - d is in it iff its cluster matches
    for (int d = 1; d < 64; d <<= 1) {
      const int oc = __shfl_up(cid, d);
      const long long t0 = __shfl_up(s0, d), t1 = __shfl_up(s1, d), t2 = __shfl_up(s2, d);
      const int tn = __shfl_up(n, d);
      if (lane >= d && oc == cid) {
        s0 += t0;
        s1 += t1;
        s2 += t2;
        n += tn;
      }
    }
    const int cid0 = __shfl(cid, 0);
    if (carry_cid >= 0 && carry_cid != cid0) {              // this step does not go on with the carried run: it is whole
      if (lane == 0) flush(carry_cid, c0, c1, c2, cn, carry_cid == first_cid, sums, cnt);
      carry_cid = -1;
    }
    if (carry_cid >= 0 && cid == carry_cid) {
      s0 += c0;
      s1 += c1;
      s2 += c2;
      n += cn;
    }
    const int next = __shfl_down(cid, 1);
    // a run's last lane has its sum; lane 63's run may go on in the next step.  A run that ends before lane 63 ends
    // inside the range (positions at or past `end` have cid -1 and come only when end == V).
    if (cid >= 0 && lane != 63 && next != cid) flush(cid, s0, s1, s2, n, cid == first_cid, sums, cnt);
    carry_cid = __shfl(cid, 63);
    c0 = __shfl(s0, 63);
    c1 = __shfl(s1, 63);
    c2 = __shfl(s2, 63);
    cn = __shfl(n, 63);
  }
  if (carry_cid >= 0 && lane == 0) {
    const bool goes_on = end < V && skey[end] != sentinel && !head[end];
    flush(carry_cid, c0, c1, c2, cn, goes_on || carry_cid == first_cid, sums, cnt);
  }
}

// used[] is zero on entry
__global__ __launch_bounds__(kThreads) void simp_face_kernel(const int32_t* __restrict__ faces, int64_t F, uint32_t V,
                                                              const int32_t* __restrict__ cluster_of,
                                                              int32_t* __restrict__ used, int32_t* __restrict__ fflag,
                                                              u64* __restrict__ counters) {
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  int invalid = 0, degenerate = 0;
  for (int64_t f = (int64_t)blockIdx.x * kThreads + threadIdx.x; f < F; f += stride) {
    const int a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
    int keep = 0;
    if ((uint32_t)a < V && (uint32_t)b < V && (uint32_t)c < V) {
      const int ca = cluster_of[a], cb = cluster_of[b], cc = cluster_of[c];
      if (ca < 0 || cb < 0 || cc < 0) {
        ++invalid;
      } else if (ca == cb || cb == cc || ca == cc) {
        ++degenerate;
      } else {
        keep = 1;
        used[ca] = 1;
        used[cb] = 1;
        used[cc] = 1;
      }
    } else {
      ++invalid;
    }
    fflag[f] = keep;
  }
  invalid = wave_sum(invalid);
  degenerate = wave_sum(degenerate);
  if ((threadIdx.x & 63) == 0) {
    if (invalid) atomicAdd(counters + C_INVALID_FACES, (u64)invalid);
    if (degenerate) atomicAdd(counters + C_DEGENERATE, (u64)degenerate);
  }
}

// incl[V - 1]: the number of clusters.  cmap / fpos: the exclusive scans of used / fflag.
__global__ __launch_bounds__(kThreads) void simp_map_kernel(int64_t V, int64_t F, const int32_t* __restrict__ cluster_of,
                                                             const int32_t* __restrict__ incl,
                                                             const int32_t* __restrict__ used,
                                                             const int32_t* __restrict__ cmap,
                                                             const int32_t* __restrict__ fflag,
                                                             const int32_t* __restrict__ fpos,
                                                             const u64* __restrict__ counters,
                                                             int32_t* __restrict__ vertex_map, int64_t* __restrict__ totals) {
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  for (int64_t v = (int64_t)blockIdx.x * kThreads + threadIdx.x; v < V; v += stride) {
    const int c = cluster_of[v];
    vertex_map[v] = c >= 0 && used[c] ? cmap[c] : -1;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    const int64_t K = incl[V - 1];
    totals[SIMP_OUT_VERTS] = K ? (int64_t)cmap[K - 1] + used[K - 1] : 0;
    totals[SIMP_OUT_FACES] = F ? (int64_t)fpos[F - 1] + fflag[F - 1] : 0;
    totals[SIMP_CLUSTERS] = K;
    totals[SIMP_INVALID_VERTS] = (int64_t)counters[C_INVALID_VERTS];
    totals[SIMP_INVALID_FACES] = (int64_t)counters[C_INVALID_FACES];
    totals[SIMP_DEGENERATE_FACES] = (int64_t)counters[C_DEGENERATE];
  }
}

// no vertex: no cluster, and every face is invalid
__global__ void simp_empty_kernel(int64_t F, int64_t* __restrict__ totals) {
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    for (int k = 0; k < SIMP_N_TOTALS; ++k) totals[k] = 0;
    totals[SIMP_INVALID_FACES] = F;
  }
}

// nC: the room of the cluster arrays; the clusters are the first incl[V - 1] <= nC of them
__global__ __launch_bounds__(kThreads) void simp_emit_verts_kernel(int64_t nC, int64_t V, Grid g,
                                                                    const int32_t* __restrict__ incl,
                                                                    const uint32_t* __restrict__ ckey,
                                                                    const u64* __restrict__ sums,
                                                                    const int32_t* __restrict__ cnt,
                                                                    const int32_t* __restrict__ used,
                                                                    const int32_t* __restrict__ cmap,
                                                                    float* __restrict__ out, int64_t n_out) {
  const int64_t K = incl[V - 1] < nC ? incl[V - 1] : nC;
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  for (int64_t c = (int64_t)blockIdx.x * kThreads + threadIdx.x; c < K; c += stride) {
    if (!used[c]) continue;
    const int64_t o = cmap[c];
    if (o < 0 || o >= n_out) continue;
    int32_t i[3];
    simp_key_cell(ckey[c], g.R[1], g.R[2], i);
    const int64_t n = cnt[c];
    if (n < 1) continue;                                    // never for a used cluster
    for (int a = 0; a < 3; ++a) out[3 * o + a] = simp_point((int64_t)sums[3 * c + a], n, i[a], g.lo[a], g.cell[a]);
  }
}

__global__ __launch_bounds__(kThreads) void simp_emit_faces_kernel(const int32_t* __restrict__ faces, int64_t F,
                                                                    uint32_t V, const int32_t* __restrict__ fflag,
                                                                    const int32_t* __restrict__ fpos,
                                                                    const int32_t* __restrict__ vertex_map,
                                                                    int32_t* __restrict__ out, int64_t n_out) {
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  for (int64_t f = (int64_t)blockIdx.x * kThreads + threadIdx.x; f < F; f += stride) {
    if (!fflag[f]) continue;
    const int64_t o = fpos[f];
    if (o < 0 || o >= n_out) continue;
    const int a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
    // a kept face of list_simp_count's faces is valid; other faces than those must not become addresses either
    if ((uint32_t)a >= V || (uint32_t)b >= V || (uint32_t)c >= V) continue;
    out[3 * o] = vertex_map[a];
    out[3 * o + 1] = vertex_map[b];
    out[3 * o + 2] = vertex_map[c];
  }
}

// ---- workspace: key u32 [V] | skey u32 [V] | val i32 [V] | perm i32 [V] | head i32 [V] | incl i32 [V] |
//                 cluster_of i32 [V] | sums u64 [nC][3] | cnt i32 [nC] | ckey u32 [nC] | used i32 [nC] | cmap i32 [nC] |
//                 fflag i32 [F] | fpos i32 [F] | counters u64 [4] | sort / scan scratch;  nC = min(V, R0 * R1 * R2) ----
struct Layout {
  size_t key, skey, val, perm, head, incl, cluster_of, sums, cnt, ckey, used, cmap, fflag, fpos, counters, scratch,
      scratch_bytes, total;
  int64_t nC;
  uint32_t sentinel;
  int end_bit;
};

int check_sizes(int64_t V, int64_t F, const int32_t* cells) {
  if (V < 0 || F < 0 || V > INT32_MAX || F > INT32_MAX)
    return fail(LIST_ERR_SHAPE, "V = %lld, F = %lld: both must be in [0, INT32_MAX]", (long long)V, (long long)F);
  if (!cells) return fail(LIST_ERR_ARG, "cells is NULL");
  for (int a = 0; a < 3; ++a)
    if (cells[a] < 1 || cells[a] > LIST_SIMP_MAX_CELLS)
      return fail(LIST_ERR_SHAPE, "cells = (%d, %d, %d): each must be in [1, %d]", cells[0], cells[1], cells[2],
                  LIST_SIMP_MAX_CELLS);
  return LIST_OK;
}

// the layout, or false with the refusal's message set
bool layout(int64_t V, int64_t F, const int32_t* cells, Layout* L) {
  const int64_t ncells = (int64_t)cells[0] * cells[1] * cells[2];       // <= 2^30
  L->sentinel = (uint32_t)ncells;
  L->end_bit = 1;
  while ((ncells >> L->end_bit) != 0) ++L->end_bit;                     // the sentinel's bits too
  L->nC = V < ncells ? V : ncells;
  size_t ss, sv, sc, sf;
  if (!sort_pairs_scratch<uint32_t, int32_t>(V, L->end_bit, &ss) || !inclusive_sum_scratch<int32_t>(V, &sv) ||
      !exclusive_sum_scratch<int32_t>(L->nC, &sc) || !exclusive_sum_scratch<int32_t>(F, &sf))
    return false;
  const size_t nv = (size_t)V * sizeof(int32_t), nc = (size_t)L->nC * sizeof(int32_t), nf = (size_t)F * sizeof(int32_t);
  Carver c;
  L->key = c.take(nv);
  L->skey = c.take(nv);
  L->val = c.take(nv);
  L->perm = c.take(nv);
  L->head = c.take(nv);
  L->incl = c.take(nv);
  L->cluster_of = c.take(nv);
  L->sums = c.take((size_t)L->nC * 3 * sizeof(u64));
  L->cnt = c.take(nc);
  L->ckey = c.take(nc);
  L->used = c.take(nc);
  L->cmap = c.take(nc);
  L->fflag = c.take(nf);
  L->fpos = c.take(nf);
  L->counters = c.take(C_N * sizeof(u64));
  L->scratch_bytes = ss;
  if (sv > L->scratch_bytes) L->scratch_bytes = sv;
  if (sc > L->scratch_bytes) L->scratch_bytes = sc;
  if (sf > L->scratch_bytes) L->scratch_bytes = sf;
  L->scratch = c.take(L->scratch_bytes);
  L->total = c.total();
  return true;
}

int check_mesh(int64_t V, int64_t F, const int32_t* cells, const void* faces, const void* workspace) {
  if (int rc = check_sizes(V, F, cells)) return rc;
  if (!workspace || (F && !faces)) return fail(LIST_ERR_ARG, "faces/workspace is NULL");
  return LIST_OK;
}

// the workspace: checked last (its size comes from hipCUB, which asks the device)
int check_workspace(int64_t V, int64_t F, const int32_t* cells, size_t workspace_bytes, Layout* L) {
  if (!layout(V, F, cells, L)) return LIST_ERR_HIP;
  if (workspace_bytes < L->total) return workspace_too_small(workspace_bytes, L->total, "list_simp_workspace_bytes");
  return LIST_OK;
}

// a finite double > 0
bool positive(double x) { return x > 0.0 && x <= 1.79769313486231570815e308; }

template <typename K, typename... Args>
int run(const char* name, K kernel, int64_t n, hipStream_t s, Args... args) {
  return launch(name, kernel, dim3(blocks_capped(n, kThreads, kMaxBlocks)), dim3(kThreads), s, args...);
}

int zero(void* p, size_t bytes, hipStream_t s, const char* what) {
  if (!bytes) return LIST_OK;
  const hipError_t e = hipMemsetAsync(p, 0, bytes, s);
  return e == hipSuccess ? LIST_OK : hip_fail(e, what);
}

}  // namespace

extern "C" {

const char* list_simp_last_error(void) { return g_err; }

size_t list_simp_workspace_bytes(int64_t V, int64_t F, const int32_t* cells) {
  Layout L;
  return check_sizes(V, F, cells) == LIST_OK && layout(V, F, cells, &L) ? L.total : 0;
}

int list_simp_count(const float* verts, const int32_t* faces, int64_t V, int64_t F, const int32_t* cells,
                    const double* lo, const double* inv, void* workspace, size_t workspace_bytes, int32_t* vertex_map,
                    int64_t* totals, void* stream) {
  Layout L;
  if (int rc = check_mesh(V, F, cells, faces, workspace)) return rc;
  if (!lo || !inv || !totals || (V && (!verts || !vertex_map)))
    return fail(LIST_ERR_ARG, "verts/lo/inv/vertex_map/totals is NULL");
  Grid g = {};
  for (int a = 0; a < 3; ++a) {
    if (!(lo[a] - lo[a] == 0.0) || !positive(inv[a]))
      return fail(LIST_ERR_ARG, "axis %d: lo = %g, inv = %g: need a finite lo and a finite inv > 0", a, lo[a], inv[a]);
    g.R[a] = cells[a];
    g.lo[a] = lo[a];
    g.inv[a] = inv[a];
  }
  if (int rc = check_workspace(V, F, cells, workspace_bytes, &L)) return rc;
  hipStream_t s = (hipStream_t)stream;
  if (V == 0) return launch("simp_empty_kernel", simp_empty_kernel, dim3(1), dim3(64), s, F, totals);
  void* ws = workspace;
  uint32_t *key = at<uint32_t>(ws, L.key), *skey = at<uint32_t>(ws, L.skey), *ckey = at<uint32_t>(ws, L.ckey);
  int32_t *val = at<int32_t>(ws, L.val), *perm = at<int32_t>(ws, L.perm), *head = at<int32_t>(ws, L.head);
  int32_t *incl = at<int32_t>(ws, L.incl), *cluster_of = at<int32_t>(ws, L.cluster_of), *cnt = at<int32_t>(ws, L.cnt);
  int32_t *used = at<int32_t>(ws, L.used), *cmap = at<int32_t>(ws, L.cmap);
  int32_t *fflag = at<int32_t>(ws, L.fflag), *fpos = at<int32_t>(ws, L.fpos);
  u64 *sums = at<u64>(ws, L.sums), *counters = at<u64>(ws, L.counters);
  char* scratch = at<char>(ws, L.scratch);
  // sums .. cmap are neighbours in the layout: one memset clears sums, cnt, ckey, used and cmap
  if (int rc = zero(sums, L.fflag - L.sums, s, "hipMemsetAsync(sums)")) return rc;
  if (int rc = zero(counters, C_N * sizeof(u64), s, "hipMemsetAsync(counters)")) return rc;
  if (int rc = run("simp_key_kernel", simp_key_kernel, V, s, verts, V, g, L.sentinel, key, val, cluster_of, counters))
    return rc;
  if (int rc = sort_pairs(scratch, L.scratch_bytes, (const uint32_t*)key, skey, (const int32_t*)val, perm, V, L.end_bit, s))
    return rc;
  if (int rc = run("simp_head_kernel", simp_head_kernel, V, s, (const uint32_t*)skey, V, L.sentinel, head)) return rc;
  if (int rc = inclusive_sum(scratch, L.scratch_bytes, (const int32_t*)head, incl, V, s)) return rc;
  if (int rc = launch("simp_sum_kernel", simp_sum_kernel, dim3(blocks_for(cdiv(V, kWaveRange), kWaves)), dim3(kThreads),
                      s, verts, V, g, L.sentinel, (const uint32_t*)skey, (const int32_t*)perm, (const int32_t*)head,
                      (const int32_t*)incl, cluster_of, ckey, sums, cnt))
    return rc;
  if (F) {
    if (int rc = run("simp_face_kernel", simp_face_kernel, F, s, faces, F, (uint32_t)V, (const int32_t*)cluster_of, used,
                     fflag, counters))
      return rc;
    if (int rc = exclusive_sum(scratch, L.scratch_bytes, (const int32_t*)fflag, fpos, F, s)) return rc;
  }
  if (int rc = exclusive_sum(scratch, L.scratch_bytes, (const int32_t*)used, cmap, L.nC, s)) return rc;
  return run("simp_map_kernel", simp_map_kernel, V, s, V, F, (const int32_t*)cluster_of, (const int32_t*)incl,
             (const int32_t*)used, (const int32_t*)cmap, (const int32_t*)fflag, (const int32_t*)fpos,
             (const u64*)counters, vertex_map, totals);
}

int list_simp_emit(const int32_t* faces, int64_t V, int64_t F, const int32_t* cells, const double* lo,
                   const double* cell, const int32_t* vertex_map, void* workspace, size_t workspace_bytes,
                   float* out_verts, int64_t n_out_verts, int32_t* out_faces, int64_t n_out_faces, void* stream) {
  Layout L;
  if (int rc = check_mesh(V, F, cells, faces, workspace)) return rc;
  if (!lo || !cell || (V && !vertex_map)) return fail(LIST_ERR_ARG, "lo/cell/vertex_map is NULL");
  Grid g = {};
  for (int a = 0; a < 3; ++a) {
    if (!(lo[a] - lo[a] == 0.0) || !positive(cell[a]))
      return fail(LIST_ERR_ARG, "axis %d: lo = %g, cell = %g: need a finite lo and a finite cell > 0", a, lo[a], cell[a]);
    g.R[a] = cells[a];
    g.lo[a] = lo[a];
    g.cell[a] = cell[a];
  }
  if (n_out_verts < 0 || n_out_verts > V || n_out_faces < 0 || n_out_faces > F)
    return fail(LIST_ERR_ARG, "n_out_verts = %lld of %lld, n_out_faces = %lld of %lld", (long long)n_out_verts,
                (long long)V, (long long)n_out_faces, (long long)F);
  if ((n_out_verts && !out_verts) || (n_out_faces && !out_faces)) return fail(LIST_ERR_ARG, "out_verts/out_faces is NULL");
  if (int rc = check_workspace(V, F, cells, workspace_bytes, &L)) return rc;
  if (V == 0 || n_out_verts == 0) return LIST_OK;           // no output vertex, so no output face
  hipStream_t s = (hipStream_t)stream;
  const void* ws = workspace;
  if (int rc = run("simp_emit_verts_kernel", simp_emit_verts_kernel, L.nC, s, L.nC, V, g, at<int32_t>(ws, L.incl),
                   at<uint32_t>(ws, L.ckey), at<u64>(ws, L.sums), at<int32_t>(ws, L.cnt), at<int32_t>(ws, L.used),
                   at<int32_t>(ws, L.cmap), out_verts, n_out_verts))
    return rc;
  if (n_out_faces == 0) return LIST_OK;
  return run("simp_emit_faces_kernel", simp_emit_faces_kernel, F, s, faces, F, (uint32_t)V, at<int32_t>(ws, L.fflag),
             at<int32_t>(ws, L.fpos), vertex_map, out_faces, n_out_faces);
}

}  // extern "C"
