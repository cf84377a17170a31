// Connected components of an indexed triangle mesh on the device (include/list_components.h): label, count, number,
// and copy out the kept components in their original order.
//
//   cc_init_kernel      parent[v] = v, used[v] = 0, the per-label counts = 0.
//   cc_mark_kernel      over the faces: used[] of a valid face's corners, and the number of invalid faces.
//   cc_hook_kernel      one round's hook: per valid face the roots of its three corners; every root above the smallest
//                       one gets atomicMin(parent[root], smallest).  Sets the round's changed word if any face saw two roots.
//   cc_compress_kernel  one round's compress: parent[v] = root of v.
//   cc_count_*_kernel   faces / vertices per label: summed per wave (ballot), then per workgroup (LDS), then one integer
//                       atomicAdd per workgroup and label.
//   cc_root_flag_kernel / hipCUB exclusive scan / cc_number_kernel   component ids in increasing order of label.
//   cc_keep_*_kernel / two scans / cc_emit_*_kernel                  compaction.
//
// parent[] is only ever lowered (atomicMin with a smaller root, compress with an ancestor), and every stored value is
// <= its index, so a chase x -> parent[x] descends strictly until parent[x] == x: it ends whatever other threads do and
// however stale a read is.  Nothing here waits for another thread; the kernel boundaries are the only synchronisation
// (DESIGN section 19 has the argument for the stopping rule).
#include <hip/hip_runtime.h>

#include "list_components.h"
#include "list_cub.h"
#include "list_host.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxBlocks = 2048;            // grid-stride above this many workgroups

__device__ __forceinline__ int ld(const int32_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// A read that may come from this CU's cache: it can be older than another workgroup's store of this launch, never older
// than the launch.  Only for the hook's first look.
__device__ __forceinline__ int ld_near(const int32_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// x's root: parent[] descends strictly, so this ends without any other thread's help
__device__ __forceinline__ int find_root(const int32_t* parent, int x) {
  for (int p = ld(parent + x); p != x; p = ld(parent + x)) x = p;
  return x;
}

__device__ __forceinline__ bool valid_face(int a, int b, int c, uint32_t V) {
  return (uint32_t)a < V && (uint32_t)b < V && (uint32_t)c < V;
}

__global__ __launch_bounds__(kThreads) void cc_init_kernel(int64_t V, int32_t* __restrict__ parent,
                                                            uint8_t* __restrict__ used, int32_t* __restrict__ fcount,
                                                            int32_t* __restrict__ vcount, int32_t* __restrict__ invalid) {
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  for (int64_t v = (int64_t)blockIdx.x * kThreads + threadIdx.x; v < V; v += stride) {
    parent[v] = (int32_t)v;
    used[v] = 0;
    fcount[v] = 0;
    vcount[v] = 0;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) *invalid = 0;
}

__global__ __launch_bounds__(kThreads) void cc_mark_kernel(const int32_t* __restrict__ faces, int64_t F, uint32_t V,
                                                            uint8_t* __restrict__ used, int32_t* __restrict__ invalid) {
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  int bad = 0;
  for (int64_t f = (int64_t)blockIdx.x * kThreads + threadIdx.x; f < F; f += stride) {
    const int a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
    if (valid_face(a, b, c, V)) {
      used[a] = 1; used[b] = 1; used[c] = 1;
    } else {
      ++bad;
    }
  }
  if (bad) atomicAdd(invalid, bad);
}

// prev: the previous round's changed word of the same call (nullptr for the call's first round)
__global__ __launch_bounds__(kThreads) void cc_hook_kernel(const int32_t* __restrict__ faces, int64_t F, uint32_t V,
                                                            int32_t* parent, const int32_t* prev, int32_t* changed) {
  if (prev && ld(prev) == 0) return;          // the labelling was complete a round ago
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  bool differ = false;
  for (int64_t f = (int64_t)blockIdx.x * kThreads + threadIdx.x; f < F; f += stride) {
    const int a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
    if (!valid_face(a, b, c, V)) continue;
    // Three equal parents: the corners hang under one node, so they are in one tree, whenever each was read.  After a
    // compress that is nearly every face, for three reads.  It cannot hide work from the stopping rule: if nothing is
    // stored in this launch every read is the launch's start state, where the forest is flat and the parent is the root.
    const int pa = ld_near(parent + a), pb = ld_near(parent + b), pc = ld_near(parent + c);
    if (pa == pb && pb == pc) continue;
    const int ra = find_root(parent, pa), rb = find_root(parent, pb), rc = find_root(parent, pc);
    const int m = min(ra, min(rb, rc));
    // m < r: the stored value stays below its index
    if (ra != m) atomicMin(parent + ra, m);
    if (rb != m && rb != ra) atomicMin(parent + rb, m);
    if (rc != m && rc != ra && rc != rb) atomicMin(parent + rc, m);
    differ |= ra != m || rb != m || rc != m;
  }
  if (differ) __hip_atomic_store(changed, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(kThreads) void cc_compress_kernel(int64_t V, int32_t* parent, const int32_t* changed) {
  if (ld(changed) == 0) return;               // this round's hook stored nothing: the forest is flat already
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  for (int64_t v = (int64_t)blockIdx.x * kThreads + threadIdx.x; v < V; v += stride) {
    const int p = ld(parent + v);
    if (p == (int)v) continue;
    const int r = find_root(parent, p);
    if (r != p) __hip_atomic_store(parent + v, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// counts[label] += 1 per item with label >= 0, with few adds on any one word.  A workgroup takes a contiguous range of
// the items and a wave 64 neighbours at a time, so a wave meets few labels: per step it peels them off one by one
// (ballot of the lanes that hold the first remaining lane's label).  The label the wave is adding up (wcur) stays in
// a register and takes its group's size; any other group is one atomicAdd of its size by one lane.  A step without
// wcur's label flushes it and the next step adopts a new one.  At the end the waves' sums meet in LDS and the
// workgroup adds once per label.  With one component holding nearly every face that is about gridDim.x adds on its
// word instead of n.  Everything is int32, so the result does not depend on the order of the adds.
template <class LabelOf>
__device__ __forceinline__ void count_labels(int64_t n, int32_t* __restrict__ counts, LabelOf label_of) {
  __shared__ int s_label[kWaves], s_n[kWaves];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t per_block = (((n + gridDim.x - 1) / gridDim.x + kThreads - 1) / kThreads) * kThreads;
  const int64_t begin = (int64_t)blockIdx.x * per_block;
  const int64_t end = begin + per_block < n ? begin + per_block : n;
  int wcur = -1, wcnt = 0;                                // the same in every lane of the wave
  for (int64_t base = begin + wave * 64; base < end; base += kThreads) {      // every lane of the wave takes every step
    const int64_t i = base + lane;
    const int l = i < end ? label_of(i) : -1;
    uint64_t rem = __ballot(l >= 0);
    bool met = false;
    while (rem) {
      const int src = __ffsll((unsigned long long)rem) - 1;
      const int g = __shfl(l, src);                       // >= 0, so a lane without a label never matches
      const uint64_t same = __ballot(l == g);
      const int c = __popcll(same);
      if (wcnt == 0) wcur = g;
      if (g == wcur) {
        wcnt += c;
        met = true;
      } else if (lane == src) {
        atomicAdd(counts + g, c);
      }
      rem &= ~same;
    }
    if (!met && wcnt) {
      if (lane == 0) atomicAdd(counts + wcur, wcnt);
      wcnt = 0;
    }
  }
  if (lane == 0) {
    s_label[wave] = wcur;
    s_n[wave] = wcnt;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 0; w < kWaves; ++w) {
      int t = s_n[w];
      if (t == 0) continue;
      for (int u = w + 1; u < kWaves; ++u)
        if (s_label[u] == s_label[w]) {
          t += s_n[u];
          s_n[u] = 0;
        }
      atomicAdd(counts + s_label[w], t);
    }
  }
}

// after the last compress: parent[v] is v's label
__global__ __launch_bounds__(kThreads) void cc_count_faces_kernel(const int32_t* __restrict__ faces, int64_t F,
                                                                   uint32_t V, const int32_t* __restrict__ parent,
                                                                   int32_t* __restrict__ fcount) {
  count_labels(F, fcount, [&](int64_t f) {
    const int a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
    return valid_face(a, b, c, V) ? parent[a] : -1;
  });
}

__global__ __launch_bounds__(kThreads) void cc_count_verts_kernel(int64_t V, const int32_t* __restrict__ parent,
                                                                   const uint8_t* __restrict__ used,
                                                                   int32_t* __restrict__ vcount) {
  count_labels(V, vcount, [&](int64_t v) { return used[v] ? parent[v] : -1; });
}

__global__ __launch_bounds__(kThreads) void cc_root_flag_kernel(int64_t V, const int32_t* __restrict__ parent,
                                                                 const uint8_t* __restrict__ used,
                                                                 int32_t* __restrict__ flag) {
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  for (int64_t v = (int64_t)blockIdx.x * kThreads + threadIdx.x; v < V; v += stride)
    flag[v] = used[v] && parent[v] == (int32_t)v;
}

// number[root] = the root's component id (exclusive scan of the root flags)
__global__ __launch_bounds__(kThreads) void cc_number_kernel(int64_t V, const int32_t* __restrict__ parent,
                                                              const uint8_t* __restrict__ used,
                                                              const int32_t* __restrict__ flag,
                                                              const int32_t* __restrict__ number,
                                                              const int32_t* __restrict__ fcount,
                                                              const int32_t* __restrict__ vcount,
                                                              const int32_t* __restrict__ invalid,
                                                              int32_t* __restrict__ component, int32_t* __restrict__ roots,
                                                              int32_t* __restrict__ face_counts,
                                                              int32_t* __restrict__ vertex_counts,
                                                              int64_t* __restrict__ totals) {
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  for (int64_t v = (int64_t)blockIdx.x * kThreads + threadIdx.x; v < V; v += stride) {
    component[v] = used[v] ? number[parent[v]] : -1;
    if (flag[v]) {
      const int k = number[v];
      roots[k] = (int32_t)v;
      face_counts[k] = fcount[v];
      vertex_counts[k] = vcount[v];
    }
    if (v == V - 1) {
      totals[0] = (int64_t)number[v] + flag[v];
      totals[1] = *invalid;
    }
  }
}

// nothing to label (V == 0 or F == 0): no component, every face invalid iff there is no vertex
__global__ __launch_bounds__(kThreads) void cc_empty_kernel(int64_t V, int32_t* __restrict__ component,
                                                             int64_t* __restrict__ totals, int64_t invalid) {
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  for (int64_t v = (int64_t)blockIdx.x * kThreads + threadIdx.x; v < V; v += stride) component[v] = -1;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    totals[0] = 0;
    totals[1] = invalid;
  }
}

__global__ __launch_bounds__(kThreads) void cc_keep_verts_kernel(int64_t V, const int32_t* __restrict__ component,
                                                                  const uint8_t* __restrict__ keep, uint32_t K,
                                                                  int32_t* __restrict__ vflag) {
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  for (int64_t v = (int64_t)blockIdx.x * kThreads + threadIdx.x; v < V; v += stride) {
    const int c = component[v];
    vflag[v] = (uint32_t)c < K && keep[c] != 0;          // c = -1 or c >= K: not kept, keep[] not read
  }
}

__global__ __launch_bounds__(kThreads) void cc_keep_faces_kernel(const int32_t* __restrict__ faces, int64_t F, uint32_t V,
                                                                  const int32_t* __restrict__ vflag,
                                                                  int32_t* __restrict__ fflag) {
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  for (int64_t f = (int64_t)blockIdx.x * kThreads + threadIdx.x; f < F; f += stride) {
    const int a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
    fflag[f] = valid_face(a, b, c, V) && vflag[a] && vflag[b] && vflag[c];
  }
}

// the vertices as their bits: a copy, not arithmetic
__global__ __launch_bounds__(kThreads) void cc_emit_verts_kernel(const uint32_t* __restrict__ verts, int64_t V,
                                                                  const int32_t* __restrict__ vflag,
                                                                  const int32_t* __restrict__ vmap,
                                                                  uint32_t* __restrict__ out, int64_t n_out) {
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  for (int64_t v = (int64_t)blockIdx.x * kThreads + threadIdx.x; v < V; v += stride) {
    if (!vflag[v]) continue;
    const int64_t o = vmap[v];
    if (o >= n_out) continue;
    out[3 * o] = verts[3 * v];
    out[3 * o + 1] = verts[3 * v + 1];
    out[3 * o + 2] = verts[3 * v + 2];
  }
}

__global__ __launch_bounds__(kThreads) void cc_emit_faces_kernel(const int32_t* __restrict__ faces, int64_t F,
                                                                  const int32_t* __restrict__ fflag,
                                                                  const int32_t* __restrict__ fpos,
                                                                  const int32_t* __restrict__ vmap,
                                                                  int32_t* __restrict__ out, int64_t n_out) {
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  for (int64_t f = (int64_t)blockIdx.x * kThreads + threadIdx.x; f < F; f += stride) {
    if (!fflag[f]) continue;                             // a kept face is valid: its corners index vmap
    const int64_t o = fpos[f];
    if (o >= n_out) continue;
    out[3 * o] = vmap[faces[3 * f]];
    out[3 * o + 1] = vmap[faces[3 * f + 1]];
    out[3 * o + 2] = vmap[faces[3 * f + 2]];
  }
}

// ---- workspace: parent i32 [V] | fcount i32 [V] | vcount i32 [V] | vflag i32 [V] | vscan i32 [V] | fflag i32 [F] |
//                 fscan i32 [F] | used u8 [V] | invalid i32 | scan scratch ----
struct Layout {
  size_t parent, fcount, vcount, vflag, vscan, fflag, fscan, used, invalid, scratch, scratch_bytes, total;
};

int check_sizes(int64_t V, int64_t F) {
  if (V < 0 || F < 0 || V > INT32_MAX || F > INT32_MAX)
    return fail(LIST_ERR_SHAPE, "V = %lld, F = %lld: both must be in [0, INT32_MAX]", (long long)V, (long long)F);
  return LIST_OK;
}

// the layout, or false with the refusal's message set
bool layout(int64_t V, int64_t F, Layout* L) {
  size_t sv, sf;
  if (!exclusive_sum_scratch<int32_t>(V, &sv) || !exclusive_sum_scratch<int32_t>(F, &sf)) return false;
  const size_t nv = (size_t)V * sizeof(int32_t), nf = (size_t)F * sizeof(int32_t);
  Carver c;
  L->parent = c.take(nv);
  L->fcount = c.take(nv);
  L->vcount = c.take(nv);
  L->vflag = c.take(nv);
  L->vscan = c.take(nv);
  L->fflag = c.take(nf);
  L->fscan = c.take(nf);
  L->used = c.take((size_t)V);
  L->invalid = c.take(sizeof(int32_t));
  L->scratch_bytes = sv > sf ? sv : sf;
  L->scratch = c.take(L->scratch_bytes);
  L->total = c.total();
  return true;
}

// the sizes and the pointers every call needs: checked first, before the entry point's own arguments
int check_mesh(int64_t V, int64_t F, const void* faces, const void* workspace) {
  if (int rc = check_sizes(V, F)) return rc;
  if (!workspace || (F && !faces)) return fail(LIST_ERR_ARG, "faces/workspace is NULL");
  return LIST_OK;
}

// the workspace: checked last (its size comes from hipCUB, which asks the device)
int check_workspace(int64_t V, int64_t F, size_t workspace_bytes, Layout* L) {
  if (!layout(V, F, L)) return LIST_ERR_HIP;
  if (workspace_bytes < L->total) return workspace_too_small(workspace_bytes, L->total, "list_cc_workspace_bytes");
  return LIST_OK;
}

// Every kernel here strides over its n items on the same capped grid
template <typename K, typename... Args>
int run(const char* name, K kernel, int64_t n, hipStream_t s, Args... args) {
  return launch(name, kernel, dim3(blocks_capped(n, kThreads, kMaxBlocks)), dim3(kThreads), s, args...);
}

int scan(void* ws, const Layout& L, const int32_t* in, int32_t* out, int64_t n, hipStream_t s) {
  return exclusive_sum(at<char>(ws, L.scratch), L.scratch_bytes, in, out, n, s);
}

}  // namespace

extern "C" {

const char* list_cc_last_error(void) { return g_err; }

size_t list_cc_workspace_bytes(int64_t V, int64_t F) {
  Layout L;
  return check_sizes(V, F) == LIST_OK && layout(V, F, &L) ? L.total : 0;
}

int list_cc_begin(const int32_t* faces, int64_t V, int64_t F, void* workspace, size_t workspace_bytes, void* stream) {
  Layout L;
  if (int rc = check_mesh(V, F, faces, workspace)) return rc;
  if (int rc = check_workspace(V, F, workspace_bytes, &L)) return rc;
  if (V == 0 || F == 0) return LIST_OK;
  hipStream_t s = (hipStream_t)stream;
  int32_t* invalid = at<int32_t>(workspace, L.invalid);
  uint8_t* used = at<uint8_t>(workspace, L.used);
  if (int rc = run("cc_init_kernel", cc_init_kernel, V, s, V, at<int32_t>(workspace, L.parent), used,
                   at<int32_t>(workspace, L.fcount), at<int32_t>(workspace, L.vcount), invalid))
    return rc;
  return run("cc_mark_kernel", cc_mark_kernel, F, s, faces, F, (uint32_t)V, used, invalid);
}

int list_cc_rounds(const int32_t* faces, int64_t V, int64_t F, void* workspace, size_t workspace_bytes,
                   int32_t first_round, int32_t n_rounds, int32_t* changed, void* stream) {
  Layout L;
  if (int rc = check_mesh(V, F, faces, workspace)) return rc;
  if (first_round < 0 || n_rounds < 1) return fail(LIST_ERR_ARG, "first_round = %d, n_rounds = %d", first_round, n_rounds);
  if (!changed) return fail(LIST_ERR_ARG, "changed is NULL");
  if ((int64_t)first_round + n_rounds > LIST_CC_MAX_ROUNDS)
    return fail(LIST_ERR_UNSUPPORTED, "rounds [%d, %lld) pass the cap of %d rounds (LIST_CC_MAX_ROUNDS): the labelling "
                "did not reach its fixpoint", first_round, (long long)first_round + n_rounds, LIST_CC_MAX_ROUNDS);
  if (int rc = check_workspace(V, F, workspace_bytes, &L)) return rc;
  hipStream_t s = (hipStream_t)stream;
  const hipError_t e = hipMemsetAsync(changed, 0, (size_t)n_rounds * sizeof(int32_t), s);
  if (e != hipSuccess) return hip_fail(e, "hipMemsetAsync(changed)");
  if (V == 0 || F == 0) return LIST_OK;
  int32_t* parent = at<int32_t>(workspace, L.parent);
  for (int r = 0; r < n_rounds; ++r) {
    if (int rc = run("cc_hook_kernel", cc_hook_kernel, F, s, faces, F, (uint32_t)V, parent,
                     r ? changed + r - 1 : (const int32_t*)nullptr, changed + r))
      return rc;
    if (int rc = run("cc_compress_kernel", cc_compress_kernel, V, s, V, parent, changed + r)) return rc;
  }
  return LIST_OK;
}

int list_cc_finish(const int32_t* faces, int64_t V, int64_t F, void* workspace, size_t workspace_bytes,
                   int32_t* component, int32_t* roots, int32_t* face_counts, int32_t* vertex_counts, int64_t* totals,
                   void* stream) {
  Layout L;
  if (int rc = check_mesh(V, F, faces, workspace)) return rc;
  if (!totals || (V && (!component || !roots || !face_counts || !vertex_counts)))
    return fail(LIST_ERR_ARG, "component/roots/face_counts/vertex_counts/totals is NULL");
  if (int rc = check_workspace(V, F, workspace_bytes, &L)) return rc;
  hipStream_t s = (hipStream_t)stream;
  if (V == 0 || F == 0) return run("cc_empty_kernel", cc_empty_kernel, V, s, V, component, totals, V == 0 ? F : 0);
  const int32_t* parent = at<int32_t>(workspace, L.parent);
  const uint8_t* used = at<uint8_t>(workspace, L.used);
  int32_t* fcount = at<int32_t>(workspace, L.fcount);
  int32_t* vcount = at<int32_t>(workspace, L.vcount);
  int32_t* flag = at<int32_t>(workspace, L.vflag);
  int32_t* number = at<int32_t>(workspace, L.vscan);
  if (int rc = run("cc_count_faces_kernel", cc_count_faces_kernel, F, s, faces, F, (uint32_t)V, parent, fcount)) return rc;
  if (int rc = run("cc_count_verts_kernel", cc_count_verts_kernel, V, s, V, parent, used, vcount)) return rc;
  if (int rc = run("cc_root_flag_kernel", cc_root_flag_kernel, V, s, V, parent, used, flag)) return rc;
  if (int rc = scan(workspace, L, flag, number, V, s)) return rc;
  return run("cc_number_kernel", cc_number_kernel, V, s, V, parent, used, flag, number, fcount, vcount,
             at<int32_t>(workspace, L.invalid), component, roots, face_counts, vertex_counts, totals);
}

int list_cc_compact(const float* verts, const int32_t* faces, int64_t V, int64_t F, const int32_t* component,
                    const uint8_t* keep, int64_t K, void* workspace, size_t workspace_bytes, float* out_verts,
                    int64_t n_out_verts, int32_t* out_faces, int64_t n_out_faces, void* stream) {
  Layout L;
  if (int rc = check_mesh(V, F, faces, workspace)) return rc;
  if (K < 0 || K > V) return fail(LIST_ERR_ARG, "K = %lld components of %lld vertices", (long long)K, (long long)V);
  if (n_out_verts < 0 || n_out_verts > V || n_out_faces < 0 || n_out_faces > F)
    return fail(LIST_ERR_ARG, "n_out_verts = %lld of %lld, n_out_faces = %lld of %lld", (long long)n_out_verts,
                (long long)V, (long long)n_out_faces, (long long)F);
  if ((V && (!verts || !component)) || (K && !keep)) return fail(LIST_ERR_ARG, "verts/component/keep is NULL");
  if ((n_out_verts && !out_verts) || (n_out_faces && !out_faces)) return fail(LIST_ERR_ARG, "out_verts/out_faces is NULL");
  if (int rc = check_workspace(V, F, workspace_bytes, &L)) return rc;
  if (n_out_verts == 0) return LIST_OK;       // no kept vertex, so no kept face
  hipStream_t s = (hipStream_t)stream;
  int32_t* vflag = at<int32_t>(workspace, L.vflag);
  int32_t* vmap = at<int32_t>(workspace, L.vscan);
  int32_t* fflag = at<int32_t>(workspace, L.fflag);
  int32_t* fpos = at<int32_t>(workspace, L.fscan);
  if (int rc = run("cc_keep_verts_kernel", cc_keep_verts_kernel, V, s, V, component, keep, (uint32_t)K, vflag)) return rc;
  if (int rc = scan(workspace, L, vflag, vmap, V, s)) return rc;
  if (int rc = run("cc_emit_verts_kernel", cc_emit_verts_kernel, V, s, (const uint32_t*)verts, V, vflag, vmap,
                   (uint32_t*)out_verts, n_out_verts))
    return rc;
  if (n_out_faces == 0) return LIST_OK;
  if (int rc = run("cc_keep_faces_kernel", cc_keep_faces_kernel, F, s, faces, F, (uint32_t)V, vflag, fflag)) return rc;
  if (int rc = scan(workspace, L, fflag, fpos, F, s)) return rc;
  return run("cc_emit_faces_kernel", cc_emit_faces_kernel, F, s, faces, F, fflag, fpos, vmap, out_faces, n_out_faces);
}

}  // extern "C"
